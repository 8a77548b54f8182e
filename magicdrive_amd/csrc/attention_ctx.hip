// attention_ctx.hip — context attention for gfx950 whose key count is read from device memory (MdxAttnDesc.tk_dev).
//
// Serves attn2 (text + camera + box context) of every transformer block of a sampler plan built at a box CAPACITY (denoiser.SamplerPlan
// dynamic_boxes): the reference pads the 3-D boxes of every batch to that batch's maximum (pipeline_bev_controlnet.py:330-343,
// configs/runner/default.yaml bbox_max_length: null), so the context length 1 + 77 + L changes almost every call of a validation run while
// everything else about the plan, and its captured hipGraph, stays the same.  K [Tk][..] and V^T [..][ldv] are valid for Tk = capacity keys;
// a query attends to keys 0 .. n - 1 with n = *tk_dev read when the kernel RUNS (a graph replay sees the value current at replay).
//
// Shape regime: Tq in {1400, 350, 91, 28}, n about 78 .. 250, d in {16, 32, 40, 80, 160} (SD-1.5 head dims + the tiny test nets').
//
// Design — the recommended shape, which is attention.hip's single-source 4-wave kernel with a memory-sourced loop bound:
//   * workgroup = 4 waves = 128 queries of one (batch, head); grid = B * H * ceil(Tq / 128), one dimension (a long product, host-checked).
//   * n is loaded once per workgroup and made wave-uniform (readfirstlane); the tile loop runs ceil(n / 64) times.  NOTHING a workgroup
//     does depends on Tk: addresses are clamped to n - 1, the mask and the zeroing compare with n.  The same n at two capacities therefore
//     gives bit-identical O (tests/test_attn_ctx_gpu.py).
//   * K tile [64 kv][d] and V^T tile [d][64 kv] go through LDS with plain __syncthreads() — no counted waits: these launches are 0.2 - 2 %
//     of a step.  Loads are unconditional from clamped addresses and masked by a select afterwards (attention.hip: a guarded load
//     serialises the tile's memory round trips).
//   * K rows >= n are ZEROED by select, V^T columns >= n are ZEROED by select before the PV MFMA: columns n .. Tk hold other tokens' finite
//     data, columns Tk .. ldv may hold anything, and 0 * NaN must not reach O.  The kv mask (kv >= n -> -inf) is applied in the last tile only.
//   * S^T = K · Q^T as in attention.hip: a lane owns one query column, the online softmax (running maximum, fp32, exp2) is lane-local plus
//     one cross-half exchange per tile.  P is rounded to the storage type before PV; the row sum is taken of the unrounded values.
//   * q_prescaled: scale_log2 = 1 (Q K^T is the base-2 exponent); otherwise scale * log2 e.  The maximum is taken of the raw scores and
//     scaled afterwards (scale > 0), as in attention.hip.
//   * n < 1 or n > Tk cannot raise without a sync: n is clamped to [1, Tk] for addressing and every O row is written as NaN — the
//     loud-miss convention of the DDIM kernel's step index -1.
//   * all of Q / K / V^T / O addressing is 64-bit (batch and row offsets as long).
//   * per-batch form (attn_ctx_rows_kernel, entry points mdx_attention_ctx_rows_*): the same body with n = tk_dev[b] for the workgroup's
//     query batch b — a batched call whose scenes carry different box counts (SamplerPlan dynamic_boxes="scene"): each scene attends to
//     its own boxes as in a one-scene call.  A bad count poisons the O rows of its own batch only.
// LDS strides are attention.hip's (K rows d16 * 16 + 8 elements, V^T rows 64 + 4 elements): its header states both fragment reads
// conflict-free.  For THIS kernel that is taken over from the bank rule (bank = dword address % 64, per 32-lane half), i.e. computed, NOT
// measured: no LDS-conflict counter of this kernel is on file, and correctness does not depend on it.
#include "common.h"
#include "launch.h"
#include "attn.h"

namespace mdx {

struct AttnCtxParams {
    const bf16_t* Q; const bf16_t* K; const bf16_t* Vt; bf16_t* O;
    const int* tk_dev;
    int H, Tq, Tk, qblocks;
    long ldq, sQ, ldk, sK, ldv, sV, ldo, sO;
    float scale_log2;  // scale * log2(e), or 1 with q_prescaled
};

constexpr int CTX_KVT = 64;              // kv tile
constexpr int CTX_VSTR = CTX_KVT + 4;    // V^T LDS row stride (elements)
constexpr int CTX_NW = 4;                // waves per workgroup
#if MDX_F16
constexpr unsigned CTX_NAN2 = 0x7E007E00u;   // two quiet NaNs of the 16-bit type
#else
constexpr unsigned CTX_NAN2 = 0x7FC07FC0u;
#endif

// One count for the whole launch (*tk_dev), or one per query batch (tk_dev[b], int32 [B]): the per-scene box counts of a batched call
// (denoiser.SamplerPlan dynamic_boxes="scene").  Workgroups of one rows launch walk different tile counts, and nothing a workgroup does
// depends on another batch's count.  Everything but the load of the count is the same text (attn_ctx_body.h).
template <int D>
__global__ __launch_bounds__(CTX_NW * 64) void attn_ctx_kernel(AttnCtxParams p) {
#define CTX_LIVE_COUNT (*p.tk_dev)
#include "attn_ctx_body.h"
#undef CTX_LIVE_COUNT
}

template <int D>
__global__ __launch_bounds__(CTX_NW * 64) void attn_ctx_rows_kernel(AttnCtxParams p) {
#define CTX_LIVE_COUNT (p.tk_dev[(long)b])
#include "attn_ctx_body.h"
#undef CTX_LIVE_COUNT
}

template <int D>
static int launch_attn_ctx(const AttnCtxParams& p, long blocks, bool rows, const char* tag, hipStream_t st) {
    if (rows) hipLaunchKernelGGL((attn_ctx_rows_kernel<D>), dim3((unsigned)blocks), dim3(CTX_NW * 64), 0, st, p);
    else hipLaunchKernelGGL((attn_ctx_kernel<D>), dim3((unsigned)blocks), dim3(CTX_NW * 64), 0, st, p);
    return check_launch(tag);
}

// Host checks + launch of both forms.  rows = false: a descriptor with tk_dev != NULL, handed on by mdx_attention_* (attention.hip) before
// every other route; tk_dev points to one int32.  rows = true: mdx_attention_ctx_rows_* below; tk_dev points to int32 [B], one count per query batch.
int attn_ctx(const MdxAttnDesc* a, hipStream_t st, const char* op, bool rows) {
    if (rows && !a) return set_error(MDX_EINVAL, "%s: null descriptor", op);
    if (rows && !a->tk_dev) return set_error(MDX_EINVAL, "%s: tk_dev is NULL: this entry point takes the device address of int32 [B] key counts", op);
    if (rows && a->kvmap) return set_error(MDX_EINVAL, "%s: tk_dev needs kvmap == NULL (batch b of Q attends to batch b of K / V^T)", op);
    if (a->nsrc != 1) return set_error(MDX_EINVAL, "%s: tk_dev needs nsrc == 1 (nsrc=%ld)", op, (long)a->nsrc);
    if (a->joint != 0) return set_error(MDX_EINVAL, "%s: tk_dev needs joint == 0 (joint=%ld)", op, (long)a->joint);
    if (a->causal != 0) return set_error(MDX_EINVAL, "%s: tk_dev needs causal == 0 (causal=%ld)", op, (long)a->causal);
    if (a->v_rowmajor != 0) return set_error(MDX_EINVAL, "%s: tk_dev needs v_rowmajor == 0 (v_rowmajor=%ld): the V^T operand", op, (long)a->v_rowmajor);
    if (a->q_prescaled != 0 && a->q_prescaled != 1) return set_error(MDX_EINVAL, "%s: q_prescaled=%ld must be 0 or 1", op, (long)a->q_prescaled);
    // the running maximum is taken of the raw scores and scaled afterwards: that is only a maximum of the scaled scores for scale > 0
    if (!a->q_prescaled && !(a->scale > 0.0)) return set_error(MDX_EINVAL, "%s: tk_dev: scale=%g must be positive (or q_prescaled == 1)", op, a->scale);
    if (!a->Q || !a->K || !a->Vt || !a->O) return set_error(MDX_EINVAL, "%s: null operand", op);
    MDX_NEED(need_aligned(op, "tk_dev", a->tk_dev, 4));
    if (a->d % 8 || a->d <= 0) return set_error(MDX_EINVAL, "%s: head dim d=%ld must be a positive multiple of 8", op, (long)a->d);
    MDX_NEED(need_attn_layout(op, a));
    if (a->d != 16 && a->d != 32 && a->d != 40 && a->d != 80 && a->d != 160)
        return set_error(MDX_EUNSUPPORTED, "%s: tk_dev: head dim d=%ld has no context-attention kernel instance (d in {16, 32, 40, 80, 160})", op, (long)a->d);
    if (a->Tk > 0 && a->ldv < a->Tk) return set_error(MDX_EINVAL, "%s: tk_dev: ldv=%ld < Tk=%ld (Tk is the capacity)", op, (long)a->ldv, (long)a->Tk);
    if (a->Tq <= 0 || a->Tk <= 0 || a->B <= 0 || a->H <= 0) return MDX_OK;
    const long qblocks = (a->Tq + CTX_NW * 32 - 1) / (CTX_NW * 32);
    const long blocks = a->B * a->H * qblocks;
    MDX_NEED(need_int(op, "B * H * ceil(Tq / 128)", blocks));
    AttnCtxParams p;
    fill_attn_params(p, a);
    p.tk_dev = a->tk_dev; p.qblocks = (int)qblocks;
    char tag[64];
    const AttnRoute r = attn_route_of(a, rows, tag);
    switch (r.d) {
        case 16: return launch_attn_ctx<16>(p, blocks, rows, tag, st);
        case 32: return launch_attn_ctx<32>(p, blocks, rows, tag, st);
        case 40: return launch_attn_ctx<40>(p, blocks, rows, tag, st);
        case 80: return launch_attn_ctx<80>(p, blocks, rows, tag, st);
        default: return launch_attn_ctx<160>(p, blocks, rows, tag, st);
    }
}

}  // namespace mdx

using namespace mdx;

// mdx_attention_ctx_rows_* (_f16 in the fp16 build: launch.h): public (mdx.h), the descriptor of mdx_attention_* with tk_dev -> int32 [B]; MDX_OP_ATTN_ROWS in a program.
extern "C" int mdx_attention_ctx_rows_bf16(const MdxAttnDesc* a, void* stream) {
    return attn_ctx(a, (hipStream_t)stream, MDX_F16 ? "mdx_attention_ctx_rows_f16" : "mdx_attention_ctx_rows_bf16", true);
}
