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
// LDS strides are attention.hip's (K rows d16 * 16 + 8 elements, V^T rows 64 + 4 elements): its header states both fragment reads
// conflict-free.  For THIS kernel that is taken over from the bank rule (bank = dword address % 64, per 32-lane half), i.e. computed, NOT
// measured: no LDS-conflict counter of this kernel is on file, and correctness does not depend on it.
#include "common.h"
#include "launch.h"

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

template <int D>
__global__ __launch_bounds__(CTX_NW * 64) void attn_ctx_kernel(AttnCtxParams p) {
    constexpr int D16 = (D + 15) / 16;  // 16-column chunks of QK^T (a ragged last chunk is zero-filled)
    constexpr int DT = (D16 + 1) / 2;   // 32-row d tiles of O^T
    constexpr int DP = D16 * 16;        // padded head dim for QK^T
    constexpr int KSTR = DP + 8;        // K LDS row stride (elements)
    constexpr int NT = CTX_NW * 64;
    constexpr int KTOT = CTX_KVT * (DP / 8), VTOT = DT * 32 * (CTX_KVT / 8);   // 16-byte chunks per K / V^T tile
    constexpr int KCH = (KTOT + NT - 1) / NT, VCH = (VTOT + NT - 1) / NT;      // chunks per thread (d = 160: 5 + 5)
    static_assert(D % 8 == 0 && D <= 160, "head dim");
    __shared__ __attribute__((aligned(16))) bf16_t Ks[CTX_KVT * KSTR];
    __shared__ __attribute__((aligned(16))) bf16_t Vs[DT * 32 * CTX_VSTR];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int col = lane & 31;
    const int bh = blockIdx.x / p.qblocks, qb = blockIdx.x - bh * p.qblocks;
    const int b = bh / p.H, h = bh - b * p.H;
    const int q = qb * (CTX_NW * 32) + wave * 32 + col;

    // ---- the live key count: one load per workgroup, wave-uniform; out of range -> clamped for addressing, O = NaN ----
    const int n_raw = __builtin_amdgcn_readfirstlane(*p.tk_dev);
    const bool bad = n_raw < 1 || n_raw > p.Tk;
    const int n = min(max(n_raw, 1), p.Tk);

    // ---- Q fragments (B operand of S^T = K Q^T): lane -> query column, 8 consecutive dims ----
    Frag8 qf[D16];
    {
        const bf16_t* qp = p.Q + (long)b * p.sQ + (long)(q < p.Tq ? q : 0) * p.ldq + (long)h * D;
#pragma unroll
        for (int ks = 0; ks < D16; ++ks) {
            const int dd = ks * 16 + half * 8;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (q < p.Tq && dd < D) v = *(const uint4*)(qp + dd);
            qf[ks].u = v;
        }
    }

    f32x16_t oacc[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m_run = -INFINITY;
    float l_run = 0.f;
    const bf16_t* kbase = p.K + (long)b * p.sK + (long)h * D;
    const bf16_t* vbase = p.Vt + (long)b * p.sV + (long)h * D * p.ldv;

    for (int j0 = 0; j0 < n; j0 += CTX_KVT) {
        uint4 kreg[KCH];
        Frag8 vreg[VCH];
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int c = tid + i * NT;
            const int row = c / (DP / 8);
            const int cc = c - row * (DP / 8);
            const bool ok = c < KTOT && j0 + row < n && cc * 8 < D;
            const int rr = min(j0 + row, n - 1), cq = min(cc * 8, D - 8);
            const uint4 v = *(const uint4*)(kbase + (long)rr * p.ldk + cq);
            kreg[i] = ok ? v : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int c = tid + i * NT;
            const int row = c >> 3;
            const int kv0 = j0 + (c & 7) * 8;
            const bool ok = c < VTOT && row < D && kv0 < n;
            Frag8 v;
            // kv0 < n <= Tk <= ldv and both kv0 and ldv are multiples of 8: the 16 bytes at kv0 lie inside the row
            v.u = *(const uint4*)(vbase + (long)min(row, D - 1) * p.ldv + (kv0 < n ? kv0 : 0));
            if (!ok) v.u = make_uint4(0, 0, 0, 0);
            vreg[i] = v;
        }
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int c = tid + i * NT;
            const int row = c / (DP / 8);
            const int cc = c - row * (DP / 8);
            if (c < KTOT) *(uint4*)(Ks + row * KSTR + cc * 8) = kreg[i];
        }
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int c = tid + i * NT;
            if (c < VTOT) {
                Frag8 v = vreg[i];
                const int kv0 = j0 + (c & 7) * 8;
                if (kv0 + 8 > n) {              // columns >= n: other tokens' data or pad — zeroed by select, never multiplied
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (kv0 + e >= n) v.h[e] = 0;
                }
                uint2* dst = (uint2*)(Vs + (c >> 3) * CTX_VSTR + (c & 7) * 8);
                dst[0] = v.d2[0];
                dst[1] = v.d2[1];
            }
        }
        __syncthreads();

        // ---- S^T[kv][q] for two 32-kv sub-tiles ----
        f32x16_t sacc[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[sub][r] = 0.f;
            const bf16_t* kr = Ks + (sub * 32 + col) * KSTR + half * 8;
#pragma unroll
            for (int ks = 0; ks < D16; ++ks) {
                Frag8 kf;
                kf.u = *(const uint4*)(kr + ks * 16);
                sacc[sub] = MDX_MFMA_32x32x16(kf.v, qf[ks].v, sacc[sub]);
            }
        }
        // ---- online softmax (this lane: one query, 32 of the 64 kv) ----
        if (j0 + CTX_KVT > n) {                 // only the last tile has kv >= n to mask (wave-uniform branch)
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kv = j0 + sub * 32 + mfma32_row(r, lane);
                    if (kv >= n) sacc[sub][r] = -INFINITY;
                }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[sub][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * p.scale_log2;
        const float m_new = fmaxf(m_run, mx);       // finite: every tile has >= 1 valid kv (j0 < n)
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // exp2(-inf) = 0 on the first tile
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[sub][r], p.scale_log2, -m_new));
                sacc[sub][r] = pv;
                psum += pv;
            }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;

        // ---- O^T[dd][q] += V^T[dd][kv] * P^T[kv][q] ----
#pragma unroll
        for (int kstep = 0; kstep < 4; ++kstep) {
            const int sub = kstep >> 1, kk = kstep & 1;
            Frag8 pf;
            pf.u.x = pack2bf(sacc[sub][kk * 8 + 0], sacc[sub][kk * 8 + 1]);
            pf.u.y = pack2bf(sacc[sub][kk * 8 + 2], sacc[sub][kk * 8 + 3]);
            pf.u.z = pack2bf(sacc[sub][kk * 8 + 4], sacc[sub][kk * 8 + 5]);
            pf.u.w = pack2bf(sacc[sub][kk * 8 + 6], sacc[sub][kk * 8 + 7]);
            const bf16_t* vr = Vs + col * CTX_VSTR + kstep * 16 + 4 * half;
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                Frag8 vf;
                vf.d2[0] = *(const uint2*)(vr + i * 32 * CTX_VSTR);
                vf.d2[1] = *(const uint2*)(vr + i * 32 * CTX_VSTR + 8);
                oacc[i] = MDX_MFMA_32x32x16(vf.v, pf.v, oacc[i]);
            }
        }
        __syncthreads();
    }
    const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32, 64));

    // ---- store O[q][h*d + dd]: lane has 4 consecutive dd per register group ----
    if (q < p.Tq) {
        bf16_t* op = p.O + (long)b * p.sO + (long)q * p.ldo + (long)h * D;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int dd = i * 32 + 8 * g + 4 * half;
                if (dd < D) {
                    uint2 ov;
                    ov.x = pack2bf(oacc[i][4 * g] * inv, oacc[i][4 * g + 1] * inv);
                    ov.y = pack2bf(oacc[i][4 * g + 2] * inv, oacc[i][4 * g + 3] * inv);
                    if (bad) ov = make_uint2(CTX_NAN2, CTX_NAN2);
                    *(uint2*)(op + dd) = ov;
                }
            }
    }
}

template <int D>
static int launch_attn_ctx(const AttnCtxParams& p, long blocks, bool pre, hipStream_t st) {
    hipLaunchKernelGGL((attn_ctx_kernel<D>), dim3((unsigned)blocks), dim3(CTX_NW * 64), 0, st, p);
    char tag[64];
    snprintf(tag, sizeof tag, "attn_ctx_kernel<%d,%s>", D, pre ? "pre" : "scaled");
    return check_launch(tag);
}

}  // namespace mdx

using namespace mdx;

// Entry for descriptors with tk_dev != NULL; called by the public mdx_attention_* (attention_short.hip) before every other route.
#if MDX_F16
extern "C" int mdx_attention_ctx_f16(const MdxAttnDesc* a, void* stream) {
    const char* op = "mdx_attention_f16";
#else
extern "C" int mdx_attention_ctx_bf16(const MdxAttnDesc* a, void* stream) {
    const char* op = "mdx_attention_bf16";
#endif
    if (a->nsrc != 1) return set_error(MDX_EINVAL, "%s: tk_dev needs nsrc == 1 (nsrc=%ld)", op, (long)a->nsrc);
    if (a->joint != 0) return set_error(MDX_EINVAL, "%s: tk_dev needs joint == 0 (joint=%ld)", op, (long)a->joint);
    if (a->causal != 0) return set_error(MDX_EINVAL, "%s: tk_dev needs causal == 0 (causal=%ld)", op, (long)a->causal);
    if (a->v_rowmajor != 0) return set_error(MDX_EINVAL, "%s: tk_dev needs v_rowmajor == 0 (v_rowmajor=%ld): the V^T operand", op, (long)a->v_rowmajor);
    if (a->q_prescaled != 0 && a->q_prescaled != 1) return set_error(MDX_EINVAL, "%s: q_prescaled=%ld must be 0 or 1", op, (long)a->q_prescaled);
    // the running maximum is taken of the raw scores and scaled afterwards: that is only a maximum of the scaled scores for scale > 0
    if (!a->q_prescaled && !(a->scale > 0.0)) return set_error(MDX_EINVAL, "%s: tk_dev: scale=%g must be positive (or q_prescaled == 1)", op, a->scale);
    if (!a->Q || !a->K || !a->Vt || !a->O) return set_error(MDX_EINVAL, "%s: null operand", op);
    MDX_NEED(need_aligned(op, "tk_dev", a->tk_dev, 4));
    MDX_NEED(need_int(op, "B", a->B)); MDX_NEED(need_int(op, "H", a->H)); MDX_NEED(need_int(op, "Tq", a->Tq)); MDX_NEED(need_int(op, "Tk", a->Tk));
    if (a->d % 8 || a->d <= 0) return set_error(MDX_EINVAL, "%s: head dim d=%ld must be a positive multiple of 8", op, (long)a->d);
    // Q / K rows and V^T rows are read as 16-byte pieces; an O row is written as 8-byte pieces (4 head-dim columns of one query)
    MDX_NEED(need_multiple(op, "ldq", a->ldq, 8)); MDX_NEED(need_multiple(op, "ldk", a->ldk, 8)); MDX_NEED(need_multiple(op, "ldv", a->ldv, 8));
    MDX_NEED(need_multiple(op, "sQ", a->sQ, 8)); MDX_NEED(need_multiple(op, "sK", a->sK, 8)); MDX_NEED(need_multiple(op, "sV", a->sV, 8));
    MDX_NEED(need_multiple(op, "ldo", a->ldo, 4)); MDX_NEED(need_multiple(op, "sO", a->sO, 4));
    MDX_NEED(need_aligned(op, "Q", a->Q, 16)); MDX_NEED(need_aligned(op, "K", a->K, 16)); MDX_NEED(need_aligned(op, "Vt", a->Vt, 16));
    MDX_NEED(need_aligned(op, "O", a->O, 8));
    if (a->d != 16 && a->d != 32 && a->d != 40 && a->d != 80 && a->d != 160)
        return set_error(MDX_EUNSUPPORTED, "%s: tk_dev: head dim d=%ld has no context-attention kernel instance (d in {16, 32, 40, 80, 160})", op, (long)a->d);
    if (a->Tk > 0 && a->ldv < a->Tk) return set_error(MDX_EINVAL, "%s: tk_dev: ldv=%ld < Tk=%ld (Tk is the capacity)", op, (long)a->ldv, (long)a->Tk);
    if (a->Tq <= 0 || a->Tk <= 0 || a->B <= 0 || a->H <= 0) return MDX_OK;
    const long qblocks = (a->Tq + CTX_NW * 32 - 1) / (CTX_NW * 32);
    const long blocks = a->B * a->H * qblocks;
    MDX_NEED(need_int(op, "B * H * ceil(Tq / 128)", blocks));
    AttnCtxParams p;
    p.Q = (const bf16_t*)a->Q; p.K = (const bf16_t*)a->K; p.Vt = (const bf16_t*)a->Vt; p.O = (bf16_t*)a->O;
    p.tk_dev = a->tk_dev;
    p.H = (int)a->H; p.Tq = (int)a->Tq; p.Tk = (int)a->Tk; p.qblocks = (int)qblocks;
    p.ldq = a->ldq; p.sQ = a->sQ; p.ldk = a->ldk; p.sK = a->sK; p.ldv = a->ldv; p.sV = a->sV; p.ldo = a->ldo; p.sO = a->sO;
    p.scale_log2 = a->q_prescaled ? 1.0f : (float)(a->scale * 1.4426950408889634);
    hipStream_t st = (hipStream_t)stream;
    const bool pre = a->q_prescaled != 0;
    switch ((int)a->d) {
        case 16: return launch_attn_ctx<16>(p, blocks, pre, st);
        case 32: return launch_attn_ctx<32>(p, blocks, pre, st);
        case 40: return launch_attn_ctx<40>(p, blocks, pre, st);
        case 80: return launch_attn_ctx<80>(p, blocks, pre, st);
        default: return launch_attn_ctx<160>(p, blocks, pre, st);
    }
}
