// Host-side evaluation of the GEMM / conv routing decision, compiled with g++ by tests/test_gemm_route.py (no GPU needed).
// Reads one case per line from stdin — `name key=value key=value ...`, keys being the fields of RouteIn and RouteOpts
// (magicdrive_amd/csrc/gemm_route.h; options start from the defaults of options.h), `flat=1` selecting gemm_route_flat — and prints one
// line per case: the kernel tag mdx_last_kernel() would report (built by the launchers' own tag helpers), the tile / split-K numbers
// and the pre- and post-step flags, or the error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "../magicdrive_amd/csrc/gemm_route.h"
#include "../magicdrive_amd/csrc/options.h"

using namespace mdx_route;

#define IN_FIELDS(X) X(M) X(N) X(K) X(batch) X(splitk) X(epi) X(c_f32) X(conv) X(Hi) X(Wi) X(Cin) X(Ho) X(Wo) X(kh) X(kw) X(sh) X(sw) X(ph) X(pw) \
    X(cimajor) X(up2) X(upB) X(lda) X(ldw) X(ldc) X(ldr) X(sC) X(rows_per_b) X(col_split) X(ws_bytes) X(has_ws) X(bias) X(temb) X(R) X(Vt) X(Wq) \
    X(ln_csum) X(ln_scratch) X(ln_stats) X(rowstat) X(ln_stats_parts) X(rowstat_parts) X(ln) X(wide) X(r_al16) X(wq_al16) X(bias_al16)
#define OPT_FIELDS(X) X(GEMM_WS) X(GEMM_XL) X(XL_K320) X(XL_MIN_TILES) X(XL_BN) X(XL_GEGLU320) X(GEMM_SMALL_TILES) X(GEMM_BM256) X(GEMM_BM) X(GEMM_BN) \
    X(GEMM_BK) X(GEMM_FLATTEN) X(LN_FUSE) X(LN_STATS) X(GEMM_TIMING)

#define DFLT(key, dflt, doc) static const long D_##key = dflt;
MDX_OPTIONS(DFLT)

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        std::string name, kv;
        if (!(ss >> name)) continue;
        RouteIn in = {};
        in.batch = 1; in.rows_per_b = 1; in.r_al16 = in.wq_al16 = in.bias_al16 = true;
        RouteOpts o;
#define SETD(f) o.f = (int)D_##f;
        OPT_FIELDS(SETD)
        bool flat = false;
        while (ss >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "%s: bad token %s\n", name.c_str(), kv.c_str()); return 2; }
            const std::string k = kv.substr(0, eq);
            const long v = atol(kv.c_str() + eq + 1);
            bool ok = false;
            if (k == "flat") { flat = v != 0; ok = true; }
#define SETI(f) if (k == #f) { in.f = (decltype(in.f))v; ok = true; }
            IN_FIELDS(SETI)
#define SETO(f) if (k == #f) { o.f = (int)v; ok = true; }
            OPT_FIELDS(SETO)
            if (!ok) { fprintf(stderr, "%s: unknown key %s\n", name.c_str(), k.c_str()); return 2; }
        }
        const Route r = flat ? gemm_route_flat(in, o) : gemm_route(in, o);
        if (r.err) {
            char msg[512] = "";
            if (r.msg) snprintf(msg, sizeof msg, r.msg, r.arg);
            printf("%s err=%d msg=%s\n", name.c_str(), r.err, msg);
            continue;
        }
        char tag[128];
        route_tag(r, in, tag, sizeof tag);
        printf("%s err=0 last=%s main=%s bn=%d BM=%d BN=%d BK=%d splitk=%d kchunk=%d normalise_first=%d rowstat_after=%d keep_rowstat=%d keep_ln=%d keep_ln_stats=%d timing=%d\n",
               name.c_str(), r.rowstat_after ? "rowstat_kernel" : tag, tag, r.bn, r.BM, r.BN, r.BK, r.splitk, r.kchunk, (int)r.normalise_first,
               (int)r.rowstat_after, (int)r.keep_rowstat, (int)r.keep_ln, (int)r.keep_ln_stats, (int)r.timing);
    }
    return 0;
}
