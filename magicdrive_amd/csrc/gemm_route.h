// gemm_route.h — which main loop runs a GEMM / conv, decided in ONE pure function.
//
// Free of HIP types (plain g++ compiles it): tests/test_gemm_route.py builds tests/gemm_route_check.cpp against this header and checks
// every threshold below on the CPU; launch_gemm_conv (gemm_conv.hip) only EXECUTES the Route it gets back: optional LayerNorm into
// ln_scratch, the main launch, optional split-K reduce, optional row statistics over the finished C.
//
// The four main loops (options.h lists the switches, all settable in-process through mdx_set_option):
//   gemm_ws.hip   K = 320 projections / GEGLU with M >= 8192 (level 0 of the UNet): weights in registers, activations streamed
//   gemm_xl.hip   every 3x3 conv with Cin % 64 == 0 and every GEMM with K % 64 == 0 that yields >= XL_MIN_TILES 256-row tiles:
//                 256 x {160, 256, 320} LDS-DMA tiles (its persistent / W-direct forms are picked inside launch_xl: they depend on the CU count)
//   gemm_conv.hip everything else: 256 / 128 / 64-row register-staged tiles (64 x 64 for small grids), split-K for the 7x13 / 4x7 levels
//   (the batch-flattened form of mdx_gemm_bf16 is an XL launch with col_split set: gemm_route_flat)
#pragma once
#include <cstddef>
#include <cstdio>

#if defined(__HIPCC__) || defined(__HIP__)
#define MDX_ROUTE_HD __host__ __device__ __forceinline__
#else
#define MDX_ROUTE_HD inline
#endif

namespace mdx_route {

constexpr int R_EINVAL = -1, R_EUNSUPPORTED = -3;      // MDX_EINVAL / MDX_EUNSUPPORTED of include/mdx.h (static_assert in gemm_conv.hip)
constexpr int XL_SLOTS = 12;                           // distinct temb rows (images) one 256-row XL tile may span (4x7 images: 11)

// ---- inputs: exactly what routing reads of a GCParams (gemm_conv.hip: route_in) ----
struct RouteIn {
    int M, N, K, batch, splitk, epi;                   // splitk: the caller's (0 = automatic)
    bool c_f32, conv;
    int Hi, Wi, Cin, Ho, Wo, kh, kw, sh, sw, ph, pw;   // conv geometry
    bool cimajor, up2;
    int upB;
    long lda, ldw, ldc, ldr, sC;
    int rows_per_b, col_split;
    long ws_bytes;
    bool has_ws, bias, temb, R, Vt, Wq, ln_csum, ln_scratch, ln_stats, rowstat;
    int ln_stats_parts, rowstat_parts;
    bool ln;                                           // ln_eps > 0
    bool wide;                                         // GCParams.wide as launch_gemm_conv computed it
    bool r_al16, wq_al16, bias_al16;                   // 16-byte alignment of R / Wq / bias (gemm_xd.hip)
};

// ---- snapshot of the option values routing reads ----
struct RouteOpts {
    int GEMM_WS, GEMM_XL, XL_K320, XL_MIN_TILES, XL_BN, XL_GEGLU320, GEMM_SMALL_TILES, GEMM_BM256, GEMM_BM, GEMM_BN, GEMM_BK, GEMM_FLATTEN,
        LN_FUSE, LN_STATS, GEMM_TIMING;
};

enum Main { MAIN_WS, MAIN_XL, MAIN_GENERIC };

struct Route {
    int err;                    // 0, or the MDX_E* code; msg is a printf format taking `arg` (null: no message, the caller falls through)
    const char* msg;
    int arg;
    Main main;
    int bn;                                   // MAIN_XL: tile width
    int BM, BN, BK, splitk, kchunk;           // MAIN_GENERIC
    bool normalise_first;                     // LayerNorm of the A rows into ln_scratch ahead of the main launch
    bool rowstat_after;                       // launch_rowstat over the finished C
    bool keep_rowstat, keep_ln, keep_ln_stats;    // which fused fields the main launch still sees
    bool timing;                              // MAIN_GENERIC: s_memtime stamps into the workspace
};

// ---- "upsampled 2x" conv geometry (GCParams.up2; the kernel side is in gemm_params.h / gemm_xl.hip) ----
// Per axis the output indices fall in classes: 0 even (taps j - 1, j: pad 1), 1 odd (taps j, j + 1: pad 0) and, when n_out = 2 n_in - 1, 2 = the last
// even index alone (its own weights: the +1 tap of the unfolded conv is zero padding there).  Class c covers `cnt` low-res indices from `first`;
// output index = 2 j + par.
struct UpAxis { int cnt, first, pad, par; };
MDX_ROUTE_HD UpAxis up_axis(int c, int n_in, int n_out) {
    const int crop = n_out != 2 * n_in;
    UpAxis a;
    a.cnt = c == 2 ? 1 : n_in - crop;
    a.first = c == 2 ? n_in - 1 : 0;
    a.pad = c == 1 ? 0 : 1;
    a.par = c == 1 ? 1 : 0;
    return a;
}
// 256-row tiles of all phases (phase = y class * x classes + x class, each phase's tiles contiguous in the M-tile index)
MDX_ROUTE_HD int up_mtiles(int upB, int Hi, int Wi, int Ho, int Wo) {
    const int ny = 2 + (Ho != 2 * Hi), nx = 2 + (Wo != 2 * Wi);
    int mt = 0;
    for (int yc = 0; yc < ny; ++yc)
        for (int xc = 0; xc < nx; ++xc) mt += (int)(((long)upB * up_axis(yc, Hi, Ho).cnt * up_axis(xc, Wi, Wo).cnt + 255) / 256);
    return mt;
}

// ---- predicates: can a main loop run this problem at all? (gemm_route decides whether it should) ----
inline bool xl_supported(const RouteIn& p, int bn) {
    const bool conv = p.conv;
    if (p.batch > 1 || p.splitk > 1 || p.c_f32 || (p.N % 4) || (p.K % 64) || p.Vt) return false;
    if (p.col_split && (conv || p.bias || p.temb || p.R || p.epi || (p.sC & 1) || (p.ldc & 1) || p.col_split < 16)) return false;
    if (bn != 256 && bn != 160 && bn != 320) return false;
    if (p.epi == 1 && (bn != 256 || (p.N % 64))) return false;
    // SiLU epilogue: only the prologue's map-encoder convs and the time MLP use it (never >= 160 tiles); instantiating it in gemm_xl.hip cost the
    // 256-wide kernels 17 spilled VGPRs (the residual prefetch went through scratch behind a full vmcnt wait)
    if (p.epi == 2) return false;
    if (conv && p.up2) {
        // upsampled-2x mode: 2x2 phase convs of the low-res input (bias only), 256- or 320-wide tiles; the epilogue's row map divides
        // (pixel inside the image + 256) through fp32 reciprocals: exact below 2^24
        // (the K order of the phase weights is the kernel's own: GCParams.cimajor does not apply)
        if (bn == 160 || p.kh != 2 || p.kw != 2 || (p.Cin % 64) || p.R || p.temb || p.epi || p.col_split) return false;
        if (p.upB < 1 || p.Hi < 1 || p.Wi < 1 || (p.Ho != 2 * p.Hi && p.Ho != 2 * p.Hi - 1) || (p.Wo != 2 * p.Wi && p.Wo != 2 * p.Wi - 1)) return false;
        if ((long)p.Hi * p.Wi + 256 >= (1L << 24) || (long)p.upB * p.Hi * p.Wi >= 0x7fffff00L) return false;
        const long span = ((long)(256 / p.Wi + 3) * p.Wi + 256L + 2 * p.Wi) * p.lda * 2;
        if (span >= 0x40000000L) return false;
        // a cropped axis adds edge classes whose grid is one row / column (or one pixel) per image: 256 tile rows then step through up to 256
        // IMAGES, so the per-lane offsets are bounded only by the whole extent of X (+ the Wi + 1 pixels by which a pad-1 tile's base may lie
        // before X), which must fit the descriptor's 2 GiB window
        if ((p.Ho != 2 * p.Hi || p.Wo != 2 * p.Wi) && ((long)p.upB * p.Hi * p.Wi + p.Wi + 2) * p.lda * 2 >= 0x7fff0000L) return false;
    } else if (conv) {
        if (p.kh != 3 || p.kw != 3 || p.ph != 1 || p.pw != 1 || (p.Cin % 64) || !p.cimajor) return false;   // pad 1: input pixel index monotonic in m
        // voffsets are relative to the tile's first receptive-field pixel: 256 output pixels span < 2^31 bytes for every real shape,
        // but keep the arithmetic honest
        const long span = ((long)(256 / p.Wo + 3) * p.sh * p.Wi + 256L * p.sw + 3 * p.Wi) * p.lda * 2;
        if (span >= 0x40000000L) return false;
    } else if ((long)256 * p.lda * 2 >= 0x40000000L) return false;
    if ((long)bn * p.ldw * 2 >= 0x40000000L) return false;
    if (p.temb && p.epi != 1) {
        const int rows = p.rows_per_b > 0 ? p.rows_per_b : 1;
        if (256 / rows + 2 > XL_SLOTS) return false;
    }
    return true;
}

inline bool ws_supported(const RouteIn& p) {
    return p.K == 320 && p.batch <= 1 && p.splitk <= 1 && !p.c_f32 && !p.temb && (p.epi == 0 || p.epi == 1) && (p.N % 4) == 0 &&
           (p.epi != 1 || (p.N % 64) == 0);
}
// The activation stream of gemm_ws.hip reads A through ONE buffer descriptor based at A (tile offsets are 32-bit byte offsets into its 2 GiB
// window, not rebased per tile): the whole extent of A must fit.  A longer A goes to a main loop that rebases per tile.
inline bool ws_fits_window(const RouteIn& p) { return (long)p.M * p.lda * 2 < 0x7FFF0000L; }
// Whether gemm_ws.hip normalises the A rows itself when LayerNorm is fused in: plain / V^T epilogues with statistics from the streamed rows or
// from the producer; GEGLU only with the producer's statistics (MdxGemmDesc.ln_stats).
inline bool ws_fuses_layernorm(const RouteIn& p) {
    if (!p.ln_csum || (p.ln_stats && p.ln_stats_parts > 4)) return false;
    return p.epi == 0 || (p.epi == 1 && p.ln_stats);
}
// Whether the plain gemm_ws kernel's store phase can emit the row statistics of C (MdxGemmDesc.rowstat_out): 16-byte row walk, one part per 128-column tile.
inline bool ws_emits_rowstat(const RouteIn& p) {
    return p.rowstat && p.epi == 0 && !p.Vt && p.wide && !p.c_f32 && !p.ln && (p.N + 127) / 128 <= p.rowstat_parts;
}
// Does the W-direct kernel (gemm_xd.hip) take this problem?
inline bool xd_supported(const RouteIn& q) {
    if (!q.Wq || q.batch > 1 || q.splitk > 1 || q.c_f32 || q.Vt || q.col_split || q.temb || q.rowstat || q.ln) return false;
    if (q.epi != 0 && q.epi != 1) return false;
    if (q.epi == 1 && (q.R || (q.N % 64))) return false;
    if ((q.K % 128) || q.K < 640 || (q.N % 16) || !q.wide) return false;
    if (q.R && ((q.ldr % 8) || !q.r_al16)) return false;
    if (!q.wq_al16 || (q.bias && !q.bias_al16)) return false;
    if ((long)256 * q.lda * 2 >= 0x40000000L || (long)256 * q.ldc * 2 >= 0x40000000L || (long)256 * q.ldr * 2 >= 0x40000000L) return false;
    if ((long)16 * (q.K >> 5) * 1024 >= 0x40000000L) return false;
    return true;
}

// ---- XL width choice ----
// Time model fitted on MI355X at 384 views (profiles/README.md, round 2): a tile costs a(bn) + b(bn) * K/64 microseconds — b falls with the
// tile width (operand bytes per MAC through the global -> LDS path), a (prologue + the HBM-bound epilogue burst; the 320-wide tile stages C in
// two halves) rises — times the rounds of tiles over the 256 CUs.  Widest first with a strict <: ties go to the wider tile.
struct XlWidth { int bn; unsigned bit; double a, b; };
constexpr unsigned W320 = 1, W256 = 2, W160 = 4, W_ALL = 7;
constexpr XlWidth kXlWidths[3] = {{320, W320, 23.7, 1.896}, {256, W256, 13.4, 1.565}, {160, W160, 16.6, 1.116}};
inline unsigned xl_width_bit(int bn) { return bn == 320 ? W320 : bn == 256 ? W256 : bn == 160 ? W160 : 0u; }

// The cheapest supported width among `widths` whose launch has at least min_tiles tiles (mtiles: 256-row tiles along M); 0 = none.
inline int xl_pick_width(const RouteIn& p, long mtiles, long min_tiles, unsigned widths) {
    int pick = 0;
    double best = 1e300;
    for (const XlWidth& w : kXlWidths) {
        if (!(widths & w.bit) || !xl_supported(p, w.bn)) continue;
        const long t = mtiles * ((p.N + w.bn - 1) / w.bn);
        if (t < min_tiles) continue;
        const double c = (double)((t + 255) / 256) * (w.a + w.b * (p.K / 64.0));
        if (c < best) { best = c; pick = w.bn; }
    }
    return pick;
}

inline Route route_fail(Route r, int code, const char* msg, int arg = 0) { r.err = code; r.msg = msg; r.arg = arg; return r; }
inline Route route_xl(Route r, int bn) { r.main = MAIN_XL; r.bn = bn; return r; }

// One XL launch for a batch-flattened GEMM (mdx_gemm_bf16: col_split set, N = all batches' columns): needs GEMM_XL > 0 and 128 tiles (XL_BN does
// not apply); R_EUNSUPPORTED without a message when the XL kernel does not take it — the caller falls through to per-batch launches.
inline Route gemm_route_flat(const RouteIn& p, const RouteOpts& o) {
    Route r = {};
    const int bn = o.GEMM_XL > 0 ? xl_pick_width(p, (p.M + 255) / 256, 128, W_ALL) : 0;
    return bn ? route_xl(r, bn) : route_fail(r, R_EUNSUPPORTED, nullptr);
}

inline Route gemm_route(RouteIn p, const RouteOpts& o) {
    Route r = {};
    r.main = MAIN_GENERIC;
    const bool conv = p.conv, geglu = p.epi == 1;
    if (!o.LN_STATS) { p.rowstat = false; p.rowstat_parts = 0; p.ln_stats = false; p.ln_stats_parts = 0; }   // A/B: the round-5 data flow
    r.keep_rowstat = p.rowstat; r.keep_ln = p.ln; r.keep_ln_stats = p.ln_stats;
    if (p.up2) {
        // upsampled-2x conv (MdxConvDesc.upsample2x): only the XL main loop knows the mode, 320- or 256-wide; GEMM_XL / XL_MIN_TILES do not apply
        if (!conv) return route_fail(r, R_EINVAL, "upsample2x: conv only");
        int bn = xl_pick_width(p, up_mtiles(p.upB, p.Hi, p.Wi, p.Ho, p.Wo), 0, W320 | W256);
        if ((o.XL_BN == 320 || o.XL_BN == 256) && xl_supported(p, o.XL_BN)) bn = o.XL_BN;
        if (!bn) return route_fail(r, R_EINVAL, "mdx_conv2d: upsample2x needs Cin %% 64 == 0, Ho in {2 Hi, 2 Hi - 1}, Wo in {2 Wi, 2 Wi - 1}, bias-only epilogue, no split-K; with a cropped axis B * Hi * Wi * ldx * 2 < 2^31");
        return route_xl(r, bn);
    }
    if (geglu && (p.N % 64) != 0) return route_fail(r, R_EINVAL, "GEGLU needs packed N %% 64 == 0 (N=%d)", p.N);
    const long mt256 = (p.M + 255) / 256;
    // K = 320 GEGLU with many rows: gemm_ws.hip (384 views: 1642 us) vs the 256 x 256 XL tile (1694-1757 us).  Before the ring of gemm_ws.hip
    // really ran ahead (its DMA builtin drained the VM counter every slab: 1994 us) the XL tile was the faster one; XL_GEGLU320 = 1 selects it again.
    const bool geglu_xl = o.XL_GEGLU320 && o.GEMM_XL == 1 && !conv && geglu && p.K == 320 && p.splitk <= 1 && o.GEMM_WS < 2 &&
                          xl_supported(p, 256) && mt256 * ((p.N + 255) / 256) >= 1024;
    // THE weight-stationary decision.  GEMM_WS: 0 off, 1 when M >= 8192, 2 whenever supported.  With XL_K320 set the XL kernel is asked first and
    // gemm_ws.hip only runs when it declines (ws_first && !ws_taken): the rows are then normalised / the row statistics taken outside the kernel.
    const bool ws_first = !conv && o.GEMM_WS > 0 && p.splitk <= 1 && ws_supported(p) && ws_fits_window(p) && (o.GEMM_WS >= 2 || p.M >= 8192);
    const bool ws_taken = !geglu_xl && ws_first && !(o.XL_K320 && o.GEMM_XL > 0);
    if (p.rowstat) {
        // Row statistics of C for the LayerNorm that reads it next (MdxGemmDesc.rowstat_out): the K = 320 weight-stationary kernel emits them
        // from its store phase; every other route gets them from a small kernel over the finished C (part 0 = whole rows, the rest zeros).
        if (conv || p.batch > 1 || p.epi != 0 || p.c_f32 || p.Vt || p.rowstat_parts < 1) return route_fail(r, R_EINVAL, "rowstat_out: plain 2-D GEMM with 16-bit C only");
        if (!(ws_taken && ws_emits_rowstat(p) && o.LN_FUSE)) {
            r.rowstat_after = true; r.keep_rowstat = false;
            p.rowstat = false; p.rowstat_parts = 0;
        }
    }
    if (p.ln) {
        // LayerNorm fused into this GEMM (MdxGemmDesc.ln_eps): the weight-stationary kernel normalises in-kernel; every other route gets
        // the rows normalised (no affine part: it is in W / bias) into the caller's scratch first.
        if (conv || p.batch > 1) return route_fail(r, R_EINVAL, "fused LayerNorm: plain 2-D GEMM only");
        if (!(ws_taken && ws_fuses_layernorm(p) && o.LN_FUSE)) {
            if (!p.ln_scratch) return route_fail(r, R_EINVAL, "fused LayerNorm: this shape is not normalised in-kernel and no ln_scratch was given");
            r.normalise_first = true; r.keep_ln = r.keep_ln_stats = false;
            p.ln = false; p.ln_csum = false; p.ln_stats = false; p.ln_stats_parts = 0;
        }
    }
    // GEMM_XL: 0 off, 1 cost model (at least XL_MIN_TILES tiles: a launch must give most of the 256 CUs a tile), 2 whenever supported.
    // XL_BN forces a width (benchmarking).  XL_K320 = 1 lets it take the K = 320 projections from gemm_ws.hip as well.
    const unsigned widths = o.XL_BN ? xl_width_bit(o.XL_BN) : W_ALL;
    if (o.GEMM_XL >= 2 && p.splitk <= 1 && p.batch <= 1 && !(p.K == 320 && !conv && !o.XL_K320)) {
        // "whenever supported" (tests / benchmarking): ahead of the automatic split-K below, which would otherwise claim small grids
        if (const int bn = xl_pick_width(p, mt256, 0, widths)) return route_xl(r, bn);
    }
    if (geglu_xl) return route_xl(r, 256);
    if (ws_taken) { r.main = MAIN_WS; return r; }
    int BM, BN = 128;
    if (!geglu && (p.N <= 64 || (p.N % 128 != 0 && p.N <= 192))) BN = 64;
    BM = p.M >= 2048 ? 128 : 64;
    // Small grids (round 6; the reference's own operating point is 1-4 scenes per call, where every launch of the step program lands here): with fewer
    // workgroups than the chip has room for, the SMALLER tile is the faster one — four 64 x 64 workgroups share a CU (37 KB of LDS each) where two
    // 128 x 128 ones fit, and a 4-wave workgroup alone on its CU has nothing to run beside its load phase.  Measured over every GEMM / conv shape
    // of the 1-, 2- and 4-scene step programs under forced tiles (tools/tile_sweep.py, profiles/r06_tile_sweep.log): plain GEMMs are fastest on
    // 64 x 64 up to ~1400 such tiles (9.5 vs 14.7 us at M 2100, N = K = 640; 18.7 vs 28.4 us at M 2184, N = K = 1280); implicit-GEMM convs up to
    // ~40 k (tile, slab) units of work, beyond that on 128 x 128 — never on the 64 x 128 tile rounds 1-5 gave every M < 2048; GEGLU (needs 128
    // columns) on 128 rows from M = 512.  Same k order in every tile: results do not depend on the choice (split-K aside).
    if (o.GEMM_SMALL_TILES && p.batch <= 1) {
        const long t64 = (long)((p.M + 63) / 64) * ((p.N + 63) / 64);
        if (geglu) {
            BM = p.M >= 512 ? 128 : 64;
        } else if (!conv) {
            if (t64 <= 1408) BM = BN = 64;
        } else if (t64 * (long)((p.K + 63) / 64) <= 40000) {
            BM = BN = 64;
        } else if (BN == 128) {
            BM = 128;
        }
    }
    if (o.GEMM_BM256 && BN == 128 && p.M >= o.GEMM_BM256) BM = 256;
    if (o.GEMM_BM == 64 || o.GEMM_BM == 128) BM = o.GEMM_BM;
    if ((o.GEMM_BN == 64 && !geglu) || o.GEMM_BN == 128) BN = o.GEMM_BN;
    // Small-M / huge-K shapes (the 7x13 and 4x7 UNet levels) are split along K into fp32 slabs in the caller's workspace
    const long tiles = (long)((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN) * (p.batch > 1 ? p.batch : 1);
    int splitk = 1;
    if (p.splitk > 0) {
        splitk = p.splitk;  // caller forced
    } else if (p.batch <= 1 && p.has_ws && tiles < 384 && p.K >= 1024 && (p.N % 4) == 0) {
        const long want = (768 + tiles - 1) / tiles;
        const long maxs = p.K / 512;  // keep >= 8 K-slabs per slice
        splitk = (int)(want < maxs ? (want < 32 ? want : 32) : (maxs < 32 ? maxs : 32));
        if (splitk < 1) splitk = 1;
    }
    if (p.batch > 1) splitk = 1;
    if (splitk > 1) {  // fit the fp32 slabs into the caller's workspace
        const long per = (long)p.M * p.N * (long)sizeof(float);
        const long fit = per > 0 ? p.ws_bytes / per : 0;
        if (fit < splitk) splitk = fit < 1 ? 1 : (int)fit;
    }
    const int kchunk = ((p.K + splitk - 1) / splitk + 63) / 64 * 64;   // split-K slices are multiples of the largest slab
    splitk = (p.K + kchunk - 1) / kchunk;
    if (splitk > 1 && !p.has_ws) return route_fail(r, R_EINVAL, "split-K needs a workspace");
    p.splitk = splitk;
    if (splitk == 1 && o.GEMM_XL > 0) {
        if (const int bn = xl_pick_width(p, mt256, o.GEMM_XL >= 2 ? 0 : o.XL_MIN_TILES, widths)) return route_xl(r, bn);
    }
    if (ws_first) { r.main = MAIN_WS; return r; }       // XL_K320 was set but the XL kernel declined the shape
    r.BM = BM; r.BN = BN; r.BK = o.GEMM_BK == 32 ? 32 : 64; r.splitk = splitk; r.kchunk = kchunk;
    r.timing = o.GEMM_TIMING && p.has_ws && splitk == 1;
    return r;
}

// ---- kernel tags (mdx_last_kernel): ONE format per main loop, used by the launchers and by the route test ----
inline void tag_generic(char* s, size_t n, int BM, int BN, int BK, bool conv) {
    snprintf(s, n, "gemm_conv_kernel<%d,%d,%d,%d,%d,%s>", BM, BN, BK, BM == 256 ? 4 : 2, 2, conv ? "conv" : "gemm");
}
inline void tag_xl(char* s, size_t n, int bn, bool conv, bool up2) {
    snprintf(s, n, "gemm_xl_kernel<256x%d,%s>", bn, conv ? (up2 ? "conv,up2x" : "conv") : "gemm");
}
inline void tag_xlp(char* s, size_t n, bool geglu, bool has_r) {
    snprintf(s, n, "gemm_xlp_kernel<256x256,%s%s>", geglu ? "geglu" : "gemm", has_r ? "+res" : "");
}
// ln: 0 none, 1 statistics from the streamed rows, 2 from the producer (ln_stats); rs: emits rowstat
inline const char* tag_ws(bool geglu, bool vt, int ln, bool rs) {
    return geglu ? (ln ? "gemm_ws_kernel<geglu,lns>" : "gemm_ws_kernel<geglu>")
                 : ln == 2 ? (vt ? "gemm_ws_kernel<vT,lns>" : "gemm_ws_kernel<plain,lns>")
                 : ln == 1 ? (vt ? "gemm_ws_kernel<vT,ln>" : "gemm_ws_kernel<plain,ln>")
                           : (vt ? "gemm_ws_kernel<vT>" : rs ? "gemm_ws_kernel<plain,rs>" : "gemm_ws_kernel<plain>");
}
// Tag of the main launch of a route (an XL GEMM may run in its persistent form: that choice is launch_xl's).
inline void route_tag(const Route& r, const RouteIn& p, char* s, size_t n) {
    if (r.main == MAIN_XL) tag_xl(s, n, r.bn, p.conv, p.up2);
    else if (r.main == MAIN_GENERIC) tag_generic(s, n, r.BM, r.BN, r.BK, p.conv);
    else snprintf(s, n, "%s", tag_ws(p.epi == 1, false, !r.keep_ln ? 0 : r.keep_ln_stats ? 2 : 1, r.keep_rowstat));
}

}  // namespace mdx_route
