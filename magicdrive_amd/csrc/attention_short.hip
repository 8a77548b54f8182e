// attention_short.hip — short-sequence attention for gfx950: V row-major, optional causal mask (MdxAttnDesc.v_rowmajor / .causal, ABI 12).
//
// Replaces the attention of transformers' CLIPTextModel (models/clip/modeling_clip.py: CLIPAttention under CLIPTextTransformer's causal mask;
// the reference pipeline's `text_encoder`, magicdrive/pipeline/pipeline_bev_controlnet.py:148-165): 77 tokens, 12 heads of 64, Q / K / V the
// three column blocks of one fused [M][3C] projection.  mdx_attention_* (attention.hip) hands descriptors with causal or v_rowmajor set to attn_short below.
//
// Shape regime: Tq, Tk <= 128, d in {32, 64}.  Nothing is a multiple of the tile (T = 77), so everything is masked.
//
// Design (one workgroup = 4 waves = 128 query rows = ALL queries of one (batch, head)):
//   * the head's whole K [Tk][d] and V [Tk][d] are staged into LDS once (16-byte loads from clamped rows; rows Tk .. roundup32(Tk) are
//     written as zeros, so no lane reads past the batch's Tk rows and a pad row's 0 * V is 0, never NaN).  One barrier in the kernel.
//   * S^T = K · Q^T as in attention.hip: a lane owns ONE query column, so max / sum are lane-local plus one cross-half shuffle.  All of
//     S^T (up to 4 sub-tiles of 32 kv) stays in registers: one softmax pass, no running maximum and no rescale.
//   * mask: kv >= Tk, and with CAUSAL kv > q, become -inf after scaling.  The scores are scaled first (t = s * scale * log2 e) and the
//     maximum is taken of the scaled values, so the largest probability is exp2(0) = 1 exactly: causal row 0 returns V[0] bit for bit.
//   * causal skip: wave w owns queries 32 w .. 32 w + 31, so the 32-kv sub-tiles above w (QK^T) and the 16-kv MFMA k-steps at or above
//     min(Tk, 32 w + 32) (PV) lie wholly above the tile's diagonal and are not issued.  All of it is wave-uniform.
//   * O^T += V^T · P^T wants V^T[dd][kv] as the A operand: 4 consecutive kv of one head-dim column per 8 bytes.  V is row-major, so the
//     fragment comes from ds_read_b64_tr_b16 on the staged image (cdna guide §5.5 T10): per 16-lane group the instruction reads a block of
//     4 kv rows x 16 columns and hands lane i column i.  Lane 4 q + p of a group supplies the address of row q, columns 4 p .. 4 p + 3.
//     The kv order inside a k-step is the accumulator's (kv = 16 kk + 8 (j >> 2) + 4 half + (j & 3)), so P^T is used as it sits in
//     registers.  The instruction needs EXEC all ones (every branch around it is wave-uniform, 256 threads), 8-byte aligned addresses (row
//     stride and column offsets are multiples of 8 bytes) and a 16-byte aligned LDS base (ONE aligned __shared__ array, carved at a
//     multiple of 16).  V row stride: 48 dwords for d = 64, 16 for d = 32 — by the bank rule (bank = dword address % 64, conflicts counted
//     per 32-lane half) the 4 rows x 16 dwords a half reads then tile the 64 banks.  That is computed from the rule, NOT measured: no
//     LDS-conflict counter or timing of this kernel is on file (correctness does not depend on it).
//   * softmax in fp32 with exp2; P is rounded to the storage type before PV, the row sum is taken of the unrounded values (attention.hip).
#include "common.h"
#include "launch.h"
#include "attn.h"

namespace mdx {

struct AttnShortParams {
    const bf16_t* Q; const bf16_t* K; const bf16_t* Vt; bf16_t* O;    // Vt: V itself, row-major [Tk][ldv] (the descriptor's field name)
    int H, Tq, Tk;
    long ldq, sQ, ldk, sK, ldv, sV, ldo, sO;
    float scale_log2;  // scale * log2(e)
};

constexpr int SHORT_T = 128;     // longest sequence: 4 waves x 32 queries, 4 sub-tiles of 32 kv

typedef __attribute__((ext_vector_type(4))) short tr16x4_t;
typedef tr16x4_t __attribute__((address_space(3))) * lds_tr_ptr_t;

template <int D16, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_short_kernel(AttnShortParams p) {
    constexpr int D = D16 * 16;              // head dim (32 or 64: no ragged chunk)
    constexpr int DT = D / 32;               // 32-row d tiles of O^T
    constexpr int KSTR = D + 8;              // K row stride (elements): ds_read_b128 fragment reads conflict-free (attention.hip)
    constexpr int VSTR = D == 64 ? 96 : 32;  // V row stride (elements): see the header comment
    constexpr int CH = D / 8;                // 16-byte chunks per row
    static_assert((SHORT_T * KSTR * 2) % 16 == 0 && (VSTR * 2) % 8 == 0, "LDS carve / transposed-read alignment");
    __shared__ __attribute__((aligned(16))) bf16_t smem[SHORT_T * KSTR + SHORT_T * VSTR];
    bf16_t* Ks = smem;
    bf16_t* Vs = smem + SHORT_T * KSTR;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: every branch on it is a wave-level branch (EXEC stays all ones)
    const int half = lane >> 5;
    const int col = lane & 31;
    const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
    const int q = wave * 32 + col;

    // ---- stage K and V rows 0 .. roundup32(Tk): clamped loads, rows >= Tk zeroed ----
    {
        const bf16_t* kbase = p.K + (long)b * p.sK + (long)h * D;
        const bf16_t* vbase = p.Vt + (long)b * p.sV + (long)h * D;
        const int rows = (p.Tk + 31) & ~31;
        for (int c = tid; c < rows * CH; c += 256) {
            const int row = c / CH, cc = c - row * CH;
            const int rr = min(row, p.Tk - 1);
            uint4 kv = *(const uint4*)(kbase + (long)rr * p.ldk + cc * 8);
            uint4 vv = *(const uint4*)(vbase + (long)rr * p.ldv + cc * 8);
            if (row >= p.Tk) { kv = make_uint4(0, 0, 0, 0); vv = make_uint4(0, 0, 0, 0); }
            *(uint4*)(Ks + row * KSTR + cc * 8) = kv;
            *(uint4*)(Vs + row * VSTR + cc * 8) = vv;
        }
    }
    // ---- Q fragments (B operand of S^T = K Q^T): lane -> query column, 8 consecutive dims ----
    Frag8 qf[D16];
    {
        const bf16_t* qp = p.Q + (long)b * p.sQ + (long)min(q, p.Tq - 1) * p.ldq + (long)h * D;
#pragma unroll
        for (int ks = 0; ks < D16; ++ks) {
            uint4 v = *(const uint4*)(qp + ks * 16 + half * 8);
            qf[ks].u = q < p.Tq ? v : make_uint4(0, 0, 0, 0);
        }
    }
    __syncthreads();
    if (wave * 32 >= p.Tq) return;           // wave-uniform: this wave has no query (after the only barrier)

    // kv range this wave needs: [0, kend) — the keys at or past kend are masked for every query of the wave
    const int kend = CAUSAL ? min(p.Tk, wave * 32 + 32) : p.Tk;

    // ---- S^T[kv][q], all sub-tiles ----
    f32x16_t sacc[4];
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[sub][r] = 0.f;
        if (sub * 32 < kend) {
            const bf16_t* kr = Ks + (sub * 32 + col) * KSTR + half * 8;
#pragma unroll
            for (int ks = 0; ks < D16; ++ks) {
                Frag8 kf;
                kf.u = *(const uint4*)(kr + ks * 16);
                sacc[sub] = MDX_MFMA_32x32x16(kf.v, qf[ks].v, sacc[sub]);
            }
        }
    }
    // ---- softmax, one pass (this lane: one query, its half of every 32-kv sub-tile) ----
    float mx = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 4; ++sub)
        if (sub * 32 < kend) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kv = sub * 32 + mfma32_row(r, lane);
                float t = sacc[sub][r] * p.scale_log2;
                if (kv >= p.Tk || (CAUSAL && kv > q)) t = -INFINITY;
                sacc[sub][r] = t;
                mx = fmaxf(mx, t);
            }
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // finite: key 0 is valid for every query
    float psum = 0.f;
#pragma unroll
    for (int sub = 0; sub < 4; ++sub)
        if (sub * 32 < kend) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(sacc[sub][r] - mx);
                sacc[sub][r] = pv;
                psum += pv;
            }
        }
    const float inv = 1.0f / (psum + __shfl_xor(psum, 32, 64));

    // ---- O^T[dd][q] += V^T[dd][kv] * P^T[kv][q]; V^T fragments by transposed reads of the row-major image ----
    f32x16_t oacc[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    // lane 4 qq + pp of its 16-lane group g: row qq of the block, columns 4 pp .. 4 pp + 3; the block's columns are 16 (g & 1) .. + 15 of the
    // d tile, its rows start at 4 half of the k-step (second read: 8 rows further)
    const int l16 = lane & 15;
    const bf16_t* vr = Vs + (4 * half + (l16 >> 2)) * VSTR + 16 * ((lane >> 4) & 1) + 4 * (l16 & 3);
#pragma unroll
    for (int kstep = 0; kstep < 8; ++kstep) {
        if (kstep * 16 < kend) {
            const int sub = kstep >> 1, kk = kstep & 1;
            Frag8 pf;
            pf.u.x = pack2bf(sacc[sub][kk * 8 + 0], sacc[sub][kk * 8 + 1]);
            pf.u.y = pack2bf(sacc[sub][kk * 8 + 2], sacc[sub][kk * 8 + 3]);
            pf.u.z = pack2bf(sacc[sub][kk * 8 + 4], sacc[sub][kk * 8 + 5]);
            pf.u.w = pack2bf(sacc[sub][kk * 8 + 6], sacc[sub][kk * 8 + 7]);
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                const bf16_t* va = vr + kstep * 16 * VSTR + i * 32;
                const tr16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr_t)va);
                const tr16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr_t)(va + 8 * VSTR));
                Frag8 vf;
                vf.d2[0] = __builtin_bit_cast(uint2, lo);
                vf.d2[1] = __builtin_bit_cast(uint2, hi);
                oacc[i] = MDX_MFMA_32x32x16(vf.v, pf.v, oacc[i]);
            }
        }
    }

    // ---- store O[q][h*d + dd]: lane has 4 consecutive dd per register group ----
    if (q < p.Tq) {
        bf16_t* op = p.O + (long)b * p.sO + (long)q * p.ldo + (long)h * D;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint2 ov;
                ov.x = pack2bf(oacc[i][4 * g] * inv, oacc[i][4 * g + 1] * inv);
                ov.y = pack2bf(oacc[i][4 * g + 2] * inv, oacc[i][4 * g + 3] * inv);
                *(uint2*)(op + i * 32 + 8 * g + 4 * half) = ov;
            }
    }
}

template <int D16>
static int launch_attn_short(const AttnShortParams& p, long blocks, bool causal, const char* tag, hipStream_t st) {
    if (causal)
        hipLaunchKernelGGL((attn_short_kernel<D16, true>), dim3((unsigned)blocks), dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL((attn_short_kernel<D16, false>), dim3((unsigned)blocks), dim3(256), 0, st, p);
    return check_launch(tag);
}

int attn_short(const MdxAttnDesc* a, hipStream_t st, const char* op) {
    if (a->causal != 0 && a->causal != 1) return set_error(MDX_EINVAL, "%s: causal=%ld must be 0 or 1", op, (long)a->causal);
    if (a->v_rowmajor != 0 && a->v_rowmajor != 1) return set_error(MDX_EINVAL, "%s: v_rowmajor=%ld must be 0 or 1", op, (long)a->v_rowmajor);
    if (!a->v_rowmajor) return set_error(MDX_EINVAL, "%s: causal needs v_rowmajor == 1 (the short-sequence kernel)", op);
    if (!a->Q || !a->K || !a->Vt || !a->O) return set_error(MDX_EINVAL, "%s: null operand", op);
    if (a->nsrc != 1) return set_error(MDX_EINVAL, "%s: v_rowmajor needs nsrc == 1 (nsrc=%ld)", op, (long)a->nsrc);
    if (a->joint != 0) return set_error(MDX_EINVAL, "%s: v_rowmajor needs joint == 0 (joint=%ld)", op, (long)a->joint);
    if (a->q_prescaled != 0) return set_error(MDX_EINVAL, "%s: v_rowmajor needs q_prescaled == 0 (q_prescaled=%ld)", op, (long)a->q_prescaled);
    if (a->causal && a->Tq != a->Tk) return set_error(MDX_EINVAL, "%s: causal needs Tq == Tk (Tq=%ld, Tk=%ld)", op, (long)a->Tq, (long)a->Tk);
    if (a->d % 8 || a->d <= 0) return set_error(MDX_EINVAL, "%s: head dim d=%ld must be a positive multiple of 8", op, (long)a->d);
    MDX_NEED(need_attn_layout(op, a));
    if (a->d != 32 && a->d != 64)
        return set_error(MDX_EUNSUPPORTED, "%s: v_rowmajor: head dim d=%ld has no short-sequence kernel instance (d in {32, 64})", op, (long)a->d);
    if (a->Tq > SHORT_T || a->Tk > SHORT_T)
        return set_error(MDX_EUNSUPPORTED, "%s: v_rowmajor: Tq=%ld, Tk=%ld: the short-sequence kernel serves Tq, Tk <= %d", op, (long)a->Tq, (long)a->Tk, SHORT_T);
    if (a->H > 0 && a->ldv < a->H * a->d) return set_error(MDX_EINVAL, "%s: v_rowmajor: ldv=%ld < H * d", op, (long)a->ldv);
    if (a->Tq <= 0 || a->Tk <= 0 || a->B <= 0 || a->H <= 0) return MDX_OK;
    const long blocks = a->B * a->H;
    MDX_NEED(need_int(op, "B * H", blocks));
    AttnShortParams p;
    fill_attn_params(p, a);
    char tag[64];
    const AttnRoute r = attn_route_of(a, false, tag);
    return r.d == 32 ? launch_attn_short<2>(p, blocks, a->causal != 0, tag, st) : launch_attn_short<4>(p, blocks, a->causal != 0, tag, st);
}

}  // namespace mdx
