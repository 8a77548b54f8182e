// attn.h — what the attention sources share: the route functions behind mdx_attention_* (attention.hip), the host checks and the descriptor ->
// parameter fill common to every route, the parameters of the lean kernel (attention2.hip).  `-Dmdx=mdx_f16` separates the two dtype builds.
#pragma once
#include "common.h"
#include "launch.h"
#include "options.h"
#include "attn_route.h"
namespace mdx {
using mdx_route::AttnIn;
using mdx_route::AttnRoute;

struct Attn2Params {
    const bf16_t* Q; const bf16_t* K; const bf16_t* Vt; bf16_t* O;
    const int* kvmap;
    int B, H, Tq, Tk, d, nsrc;
    int joint;         // 1: one softmax over the concatenation of the nsrc sources; 0: per-source softmax, outputs summed (nsrc <= 2)
    long ldq, sQ, ldk, sK, ldv, sV, ldo, sO;
    float scale_log2;  // scale * log2(e); 1 when q_prescaled
    int q_prescaled;   // Q already carries scale * log2(e) (MdxAttnDesc.q_prescaled)
    int qblocks;       // query blocks per (batch, head), filled in by launch_attn2
    int viewmap;       // block order (launch_attn2, option ATTN2_VIEWMAP): 1 = every head and query block of a view on ONE XCD
};

// The layout checks every route shares: Q / K and V^T (row-major: V) rows are read as 16-byte pieces, an O row is written as 8-byte pieces.
inline int need_attn_layout(const char* op, const MdxAttnDesc* a) {
    MDX_NEED(need_int(op, "B", a->B)); MDX_NEED(need_int(op, "H", a->H)); MDX_NEED(need_int(op, "Tq", a->Tq)); MDX_NEED(need_int(op, "Tk", a->Tk));
    MDX_NEED(need_multiple(op, "ldq", a->ldq, 8)); MDX_NEED(need_multiple(op, "ldk", a->ldk, 8)); MDX_NEED(need_multiple(op, "ldv", a->ldv, 8));
    MDX_NEED(need_multiple(op, "sQ", a->sQ, 8)); MDX_NEED(need_multiple(op, "sK", a->sK, 8)); MDX_NEED(need_multiple(op, "sV", a->sV, 8));
    MDX_NEED(need_multiple(op, "ldo", a->ldo, 4)); MDX_NEED(need_multiple(op, "sO", a->sO, 4));
    MDX_NEED(need_aligned(op, "Q", a->Q, 16)); MDX_NEED(need_aligned(op, "K", a->K, 16)); MDX_NEED(need_aligned(op, "Vt", a->Vt, 16));
    MDX_NEED(need_aligned(op, "O", a->O, 8));
    return MDX_OK;
}
// Pointers, sizes, strides and the softmax scale of a checked descriptor, for any route's parameter struct.
template <class P> inline void fill_attn_params(P& p, const MdxAttnDesc* a) {
    p.Q = (const bf16_t*)a->Q; p.K = (const bf16_t*)a->K; p.Vt = (const bf16_t*)a->Vt; p.O = (bf16_t*)a->O;
    p.H = (int)a->H; p.Tq = (int)a->Tq; p.Tk = (int)a->Tk;
    p.ldq = a->ldq; p.sQ = a->sQ; p.ldk = a->ldk; p.sK = a->sK; p.ldv = a->ldv; p.sV = a->sV; p.ldo = a->ldo; p.sO = a->sO;
    // q_prescaled: the caller folded scale * log2(e) into the query projection: scores are base-2 exponents already
    p.scale_log2 = a->q_prescaled ? 1.0f : (float)(a->scale * 1.4426950408889634);
}
// ... plus the kv sources of the kernels that take several (attention.hip, attention2.hip)
template <class P> inline void fill_attn_sources(P& p, const MdxAttnDesc* a) {
    fill_attn_params(p, a);
    p.kvmap = a->kvmap;
    p.B = (int)a->B; p.d = (int)a->d; p.nsrc = (int)a->nsrc; p.joint = (int)a->joint;
}
// What attn_route.h reads of a descriptor; rows: the mdx_attention_ctx_rows_* entry point.
inline AttnIn attn_in(const MdxAttnDesc* a, bool rows = false) {
    return AttnIn{a->B, a->H, a->Tq, a->Tk, a->d, a->nsrc, a->joint != 0, a->q_prescaled != 0, a->causal != 0, a->v_rowmajor != 0,
                  a->tk_dev != nullptr, rows, a->ldk, a->ldv, a->sK, a->sV};
}
// The route of a checked descriptor under the current option values, and the name its launcher reports (mdx_last_kernel).
inline AttnRoute attn_route_of(const MdxAttnDesc* a, bool rows, char (&tag)[64]) {
    const mdx_route::AttnOpts o = {(int)opt(OPT_ATTN2), (int)opt(OPT_ATTN2_D80), (int)opt(OPT_ATTN2_QT), (int)opt(OPT_ATTN2_FOLD), (int)opt(OPT_ATTN2_RES),
                                   (int)opt(OPT_ATTN2_PF), (int)opt(OPT_ATTN_NW), (long)opt(OPT_ATTN_NW4_BLOCKS), (long)opt(OPT_ATTN_NW8_BLOCKS)};
    const AttnIn in = attn_in(a, rows);
    const AttnRoute r = mdx_route::attn_route(in, o);
    mdx_route::attn_route_tag(r, in, tag, sizeof tag);
    return r;
}

// The routes mdx_attention_* hands a descriptor to: each runs its own host checks, then the launch.
int attn_ctx(const MdxAttnDesc* a, hipStream_t st, const char* op, bool rows);    // attention_ctx.hip: tk_dev != NULL
int attn_short(const MdxAttnDesc* a, hipStream_t st, const char* op);             // attention_short.hip: causal / v_rowmajor
int launch_attn2(const Attn2Params& p, const AttnRoute& r, const char* tag, hipStream_t st);      // attention2.hip: ATTN2_RESIDENT / ATTN2_STREAM
// attention3.hip: the pipelined head-dim-40 FOLD form (called from launch_attn2)
bool attn3_supported(const Attn2Params& p);
int launch_attn3(const Attn2Params& p, hipStream_t st);
}  // namespace mdx
