// attn_route.h — which kernel runs an attention descriptor, decided in ONE pure function.
//
// Free of HIP types (plain g++ compiles it): tests/test_attn_route.py builds tests/attn_route_check.cpp against this header and checks every
// threshold below on the CPU.  mdx_attention_* (attention.hip) asks attn_family before a route's host checks and attn_route after them; the
// launchers only EXECUTE the AttnRoute and keep what depends on the device (grid shape, ATTN_SWZ, ATTN2_VIEWMAP).  The families: ctx
// (attention_ctx.hip: tk_dev != NULL, before every other test), short (attention_short.hip: causal or v_rowmajor), attn2 (attention2.hip: head
// dim 40 / 80 with >= 128 workgroups of 128 queries; short kv sequences RESIDENT in LDS) and flash (attention.hip: everything else).
#pragma once
#include <cstddef>
#include <cstdio>

namespace mdx_route {

struct AttnIn {                 // exactly what routing reads of an MdxAttnDesc
    long B, H, Tq, Tk, d, nsrc;
    bool joint, q_prescaled, causal, v_rowmajor;
    bool has_tk_dev, rows;      // tk_dev != NULL; rows: the mdx_attention_ctx_rows_* entry point (one count per query batch)
    long ldk, ldv, sK, sV;
};
struct AttnOpts {               // snapshot of the option values routing reads (options.h)
    int ATTN2, ATTN2_D80, ATTN2_QT, ATTN2_FOLD, ATTN2_RES, ATTN2_PF, ATTN_NW;
    long ATTN_NW4_BLOCKS, ATTN_NW8_BLOCKS;
};
enum AttnFamily { ATTN_CTX, ATTN_SHORT, ATTN2_RESIDENT, ATTN2_STREAM, ATTN_FLASH };
struct AttnRoute {
    AttnFamily family;
    int d, qt;                  // head dim (ctx, short, attn2 instances); ATTN2_STREAM: 32-query blocks per wave (1 or 2)
    int d16, nw;                // ATTN_FLASH: 16-column chunks of the head dim (7 and 9 have no instance: the entry point refuses them), waves per workgroup
    bool fold, pf;              // attn2: running maximum folded into the QK MFMA (pre-scaled Q); permute-free P
};
constexpr int A2_KV_TILE = 64, A2_RES_TILES = 3;       // attention2.hip: A2_KV, A2_NBUF (static_assert there)

inline AttnFamily attn_family(const AttnIn& p) { return p.has_tk_dev ? ATTN_CTX : (!p.causal && !p.v_rowmajor) ? ATTN_FLASH : ATTN_SHORT; }

// Shapes the lean kernel takes (everything else stays on attention.hip): head dim 40 or 80, enough query blocks to fill the chip,
// 16-byte aligned K rows / V^T rows, matrices within the 2 GiB DMA window.
inline bool attn2_supported(const AttnIn& p, const AttnOpts& o) {
    // d = 80 (level 1, T = 350): 0 never, 1 always, 2 (default) only the two-source cross-view form — measured at 768 views with the
    // round-4 issue path (profiles/r04_attn_d80.log): cross-view 923 vs 1000-1012 us on attention.hip, self 545 vs 517-529 us
    const int d80 = o.ATTN2_D80;
    const bool xview2 = p.nsrc == 2 && !p.joint;
    if (!o.ATTN2 || (p.d != 40 && !(p.d == 80 && (d80 == 1 || (d80 == 2 && xview2))))) return false;
    if (p.Tq < 256 || (long)((p.Tq + 127) / 128) * p.H * p.B < 128) return false;
    if ((p.ldk % 8) || (p.ldv % 8) || (p.sK % 8) || (p.sV % 8) || (p.ldv < ((p.Tk + 7) / 8) * 8)) return false;
    return (long)p.Tk * p.ldk * 2 < 0x40000000L && (long)p.d * p.H * p.ldv * 2 < 0x40000000L;
}

// Waves per workgroup of the flash kernel.  4 waves (128 queries) whenever (batch x heads) alone fills the chip — also for 91- and 28-token
// sequences: every thread of the workgroup stages K / V^T, so the idle query rows cost less than narrower workgroups lose on staging (384
// views, T = 91, d = 160: 4 waves 103 us, 2 waves 152 us, 1 wave 448 us; T = 28: 39 / 44 / 71 us; cross-view at T = 28: 2 waves 73 vs 108 us).
// With few (batch, head) pairs the sequence is split finer so that short sequences still spread over the chip.
inline int attn_waves(const AttnIn& p, const AttnOpts& o) {
    const long blocks4 = (long)((p.Tq + 127) / 128) * p.H * p.B, blocks8 = (long)((p.Tq + 255) / 256) * p.H * p.B;
    if (o.ATTN_NW == 8 || o.ATTN_NW == 4 || o.ATTN_NW == 2 || o.ATTN_NW == 1) return o.ATTN_NW;      // experiments: force 1 / 2 / 4 / 8 waves
    if (p.Tq >= 512 && blocks8 >= o.ATTN_NW8_BLOCKS) return 8;
    if (p.Tq >= 256 && blocks4 >= o.ATTN_NW4_BLOCKS) return 4;
    if ((long)p.H * p.B >= 2 * o.ATTN_NW4_BLOCKS) return (p.Tq <= 32 && p.nsrc == 2) ? 2 : 4;
    return p.Tq >= 64 ? 2 : 1;
}

inline AttnRoute attn_route(const AttnIn& p, const AttnOpts& o) {
    AttnRoute r = {};
    r.family = attn_family(p); r.d = (int)p.d;
    if (r.family != ATTN_FLASH) return r;
    if (!attn2_supported(p, o)) {
        r.d16 = (int)(p.d + 15) / 16; r.nw = attn_waves(p, o);
        return r;
    }
    r.family = ATTN2_STREAM; r.qt = 1;
    if (p.d != 40) return r;                     // d = 80: 32-query waves, no FOLD instance
    // 64 queries per wave (see attn2_kernel) when there are enough queries per head, except where the 32-query FOLD form wins; ATTN2_QT = 1 / 2: force
    const bool two = (o.ATTN2_QT == 0 || o.ATTN2_QT == 2) && p.Tq >= 512;
    // pre-scaled Q (scale * log2 e folded into to_q at pack time): scores are base-2 exponents as they come out of the MFMA
    r.fold = p.q_prescaled && o.ATTN2_FOLD != 0;
    // short kv sequences (the text context): every tile resident in the ring, one workgroup per (batch, head) walks the query blocks (ATTN2_RES: options.h)
    if (r.fold && p.nsrc == 1 && (p.Tk + A2_KV_TILE - 1) / A2_KV_TILE <= A2_RES_TILES &&
        (o.ATTN2_RES == 2 || (o.ATTN2_RES == 1 && p.Tq >= 512 && (long)p.B * p.H >= 1024))) {
        r.family = ATTN2_RESIDENT;
        return r;
    }
    // FOLD frees the registers / VALU slots of the scale-and-subtract: with it the 32-query form (<= 142 VGPRs: three waves per SIMD)
    // is the faster one for one kv source (768 views, T = 1400: self 3157 vs 3332 us, text context 640 vs 795 us; the two-source
    // cross-view form is equal, 5888 vs 5882 us: profiles/r03_attn_qt_fold_ab.log); ATTN2_QT = 2 keeps 64-query waves everywhere.
    // round 4: with the straight-line issue path and four waves per SIMD the 32-query form also wins (by 1-2.5 %) for the two-source launches
    r.qt = (two && (!r.fold || o.ATTN2_QT == 2)) ? 2 : 1;
    r.pf = r.fold && r.qt == 1 && o.ATTN2_PF != 0;       // round 5: permute-free P
    return r;
}

// The name the route's launcher reports through mdx_last_kernel().
inline void attn_route_tag(const AttnRoute& r, const AttnIn& p, char* tag, size_t n) {
    const char* mode = (p.nsrc == 2 && !p.joint) ? "xview" : (p.nsrc > 1 ? "joint" : "self");
    switch (r.family) {
        case ATTN_CTX: snprintf(tag, n, "attn_ctx_kernel<%d,%s%s>", r.d, p.q_prescaled ? "pre" : "scaled", p.rows ? ",rows" : ""); break;
        case ATTN_SHORT: snprintf(tag, n, "attn_short_kernel<%d,%s>", r.d, p.causal ? "causal" : "full"); break;
        case ATTN2_RESIDENT: snprintf(tag, n, "attn2_kernel<%d,resident,q32%s>", r.d, r.fold ? ",fold" : ""); break;
        case ATTN2_STREAM: snprintf(tag, n, "attn2_kernel<%d,%s,q%d%s%s>", r.d, mode, 32 * r.qt, r.fold ? ",fold" : "", r.pf ? ",pf" : ""); break;
        case ATTN_FLASH: snprintf(tag, n, "attn_kernel<%d,%d,%s>", r.d16, r.nw, mode); break;
    }
}

}  // namespace mdx_route
