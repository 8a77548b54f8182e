// Host-side evaluation of the attention routing decision, compiled with g++ by tests/test_attn_route.py (no GPU needed).
// Reads one case per line from stdin — `name key=value key=value ...`, keys being the fields of AttnIn and AttnOpts
// (magicdrive_amd/csrc/attn_route.h; options start from the defaults of options.h) — and prints one line per case: the family, the
// instance and the kernel tag mdx_last_kernel() would report (attn_route_tag, which the launchers use themselves).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include "../magicdrive_amd/csrc/attn_route.h"
#include "../magicdrive_amd/csrc/options.h"

using namespace mdx_route;

#define IN_FIELDS(X) X(B) X(H) X(Tq) X(Tk) X(d) X(nsrc) X(joint) X(q_prescaled) X(causal) X(v_rowmajor) X(has_tk_dev) X(rows) X(ldk) X(ldv) X(sK) X(sV)
#define OPT_FIELDS(X) X(ATTN2) X(ATTN2_D80) X(ATTN2_QT) X(ATTN2_FOLD) X(ATTN2_RES) X(ATTN2_PF) X(ATTN_NW) X(ATTN_NW4_BLOCKS) X(ATTN_NW8_BLOCKS)

#define DFLT(key, dflt, doc) static const long D_##key = dflt;
MDX_OPTIONS(DFLT)

int main() {
    static const char* const family[] = {"ctx", "short", "attn2-resident", "attn2", "flash"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        std::string name, kv;
        if (!(ss >> name)) continue;
        AttnIn in = {};
        AttnOpts o;
#define SETD(f) o.f = (decltype(o.f))D_##f;
        OPT_FIELDS(SETD)
        while (ss >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "%s: bad token %s\n", name.c_str(), kv.c_str()); return 2; }
            const std::string k = kv.substr(0, eq);
            const long v = atol(kv.c_str() + eq + 1);
            bool ok = false;
#define SETI(f) if (k == #f) { in.f = (decltype(in.f))v; ok = true; }
            IN_FIELDS(SETI)
#define SETO(f) if (k == #f) { o.f = (decltype(o.f))v; ok = true; }
            OPT_FIELDS(SETO)
            if (!ok) { fprintf(stderr, "%s: unknown key %s\n", name.c_str(), k.c_str()); return 2; }
        }
        const AttnRoute r = attn_route(in, o);
        char tag[64];
        attn_route_tag(r, in, tag, sizeof tag);
        printf("%s family=%s d=%d d16=%d nw=%d qt=%d fold=%d pf=%d tag=%s\n", name.c_str(), family[r.family], r.d, r.d16, r.nw, r.qt, (int)r.fold, (int)r.pf, tag);
    }
    return 0;
}
