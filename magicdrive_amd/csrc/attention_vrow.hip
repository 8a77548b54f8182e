// attention_vrow.hip — flash attention on a ROW-MAJOR V for gfx950, any sequence length: mdx_sdpa_bf16 / _f16 (MdxSdpaDesc, MDX_OP_SDPA).
//
// The general scaled-dot-product-attention call of the library: Q, K and V as a projection writes them, [B][T][H*d] with a token stride —
// so they can be the three column blocks of one fused [M][3C] projection buffer — an optional causal mask and an optional key count per
// batch, read from device memory.  attention.hip / attention2.hip want V^T with the key axis padded to 8 (the producer pays for the layout),
// attention_short.hip reads V in place but only for T <= 128 and d in {32, 64}.  This file is the streaming, online-softmax form of
// attention_short.hip's technique; the entry points of those files and their routes are untouched.
//
// Shape regime: any Tq, Tk >= 1; d % 8 == 0, d <= 160 with attention.hip's instance set (ceil(d / 16) in {1..6, 8, 10}).
//
// Design (one workgroup = NW waves = NW * 32 query rows of one (batch, head); taken from attention.hip unless said otherwise):
//   * Q fragments live in registers for the whole kernel.  K tile [64 kv][d] and V tile [64 kv][d] (row-major, as in memory) are staged
//     into LDS with 16-byte loads, all of a thread's loads of a tile issued back to back from clamped addresses and masked by a select
//     afterwards (a guarded load serialises the tile's memory round trips).
//   * memory safety: a row at or past the batch's key count n (n = Tk, or klen_dev[b]) is never read — the row index is clamped to n - 1 —
//     and is written to LDS as zeros, K and V alike: a pad row contributes 0 * 0 to O, never 0 * garbage.  Head-dim columns d .. of the
//     padded tile are zeros too (they only feed accumulator rows that are not stored).
//   * S^T = K · Q^T: a lane owns ONE query column, so the online-softmax max / sum / rescale are lane-local plus one cross-half exchange
//     per tile, and the P^T registers are directly the B operand of O^T += V^T · P^T.
//   * V^T fragments come from ds_read_b64_tr_b16 on the row-major image (attention_short.hip; cdna guide §5.5 T10): per 16-lane group the
//     instruction reads 4 kv rows x 16 columns and hands lane i column i; lane 4 q + p supplies the address of row q, columns 4 p .. 4 p + 3.
//     The kv order inside a k-step is the accumulator's (kv = 16 kk + 8 (j >> 2) + 4 half + (j & 3)), so P^T is used as it sits in
//     registers.  Preconditions: EXEC all ones — every branch around the reads is wave-uniform (kernel arguments, blockIdx, the wave index
//     and the key count through readfirstlane; the workgroup is NW * 64 threads and no lane leaves early); 8-byte aligned addresses (row
//     stride and column offsets are multiples of 8 bytes); a 16-byte aligned LDS base (ONE aligned __shared__ array, V carved at a
//     multiple of 16 bytes).
//   * LDS strides.  K rows: d16 * 16 + 8 elements (attention.hip's: ds_read_b128 fragment reads).  V rows: (DT | 1) * 32 elements, DT =
//     32-column tiles of the padded head dim — 32, 96, 96, 160, 160 elements for DT = 1 .. 5, i.e. an ODD multiple of 16 dwords.  By the
//     bank rule (bank = dword address % 64, conflicts counted per 32-lane half) the 4 rows x 16 dwords a half reads in one transposed
//     read then tile the 64 banks.  That is COMPUTED from the rule, NOT measured: no LDS-conflict counter of this kernel is on file
//     (correctness does not depend on it).
//   * softmax in fp32 with exp2.  The scores are scaled first (t = s * scale * log2 e), then masked (kv >= n, causal: kv > q -> -inf), and
//     the maximum is taken of the scaled values: the largest probability is exp2(0) = 1 exactly, so Tk = 1 returns V[b, 0] and causal row 0
//     returns V[0] bit for bit (and the sign of scale does not matter).  P is rounded to the storage type before PV; the row sum is taken
//     of the unrounded values (attention.hip).
//   * causal: the tile loop of a workgroup ends at its last query (workgroup-uniform: every wave takes part in staging and in the
//     barriers); a wave skips the QK^T / softmax / PV work of the tiles that lie wholly above its own diagonal (wave-uniform).  Tile 0
//     holds key 0, which every query sees, so the running maximum is finite from the first tile on.
//   * klen_dev: n = klen_dev[b], read once per workgroup when the kernel RUNS (a replayed graph sees the current value), wave-uniform.
//     n outside [1, Tk] cannot raise without a sync: n is clamped for addressing and every O row of that batch is written as NaN (the
//     convention of MdxAttnDesc.tk_dev).  Nothing a workgroup does depends on another batch.
//   * determinism: the per-query arithmetic is lane-local and the kv tiles are walked in order, so neither B nor the waves per workgroup
//     (launch_vrow_nw: attention.hip's rule) changes a bit of a row.
//   * XCD-aware 1-D grid: workgroup L runs on XCD L % 8 (observed dispatch rule; speed only); all query blocks of one (batch, head) go to
//     ONE XCD back to back, so the pair's K / V is fetched into one L2.  All of Q / K / V / O addressing is 64-bit.
#include "common.h"
#include "launch.h"
#include "options.h"

namespace mdx {

struct SdpaParams {
    const bf16_t* Q; const bf16_t* K; const bf16_t* V; bf16_t* O;
    const int* klen;
    int BH, H, Tq, Tk, d, qblocks, causal;
    long ldq, sQ, ldk, sK, ldv, sV, ldo, sO;
    float scale_log2;  // scale * log2(e)
};

constexpr int VR_KVT = 64;       // kv tile
#if MDX_F16
constexpr unsigned VR_NAN2 = 0x7E007E00u;   // two quiet NaNs of the 16-bit type
#else
constexpr unsigned VR_NAN2 = 0x7FC07FC0u;
#endif

typedef __attribute__((ext_vector_type(4))) short vr_tr16x4_t;
typedef vr_tr16x4_t __attribute__((address_space(3))) * vr_lds_tr_ptr_t;

template <int D16, int NW, bool CAUSAL>
__global__ __launch_bounds__(NW * 64) void attn_vrow_kernel(SdpaParams p) {
    constexpr int DT = (D16 + 1) / 2;       // 32-row d tiles of O^T
    constexpr int DP = D16 * 16;            // padded head dim for QK^T
    constexpr int DV = DT * 32;             // padded head dim of the V tile
    constexpr int KSTR = DP + 8;            // K LDS row stride (elements)
    constexpr int VSTR = (DT | 1) * 32;     // V LDS row stride (elements): see the header comment
    constexpr int NT = NW * 64;
    constexpr int KTOT = VR_KVT * (DP / 8), VTOT = VR_KVT * (DV / 8);          // 16-byte chunks per K / V tile
    constexpr int KCH = (KTOT + NT - 1) / NT, VCH = (VTOT + NT - 1) / NT;      // chunks per thread
    constexpr bool UNR = (KCH + VCH) <= 24;                                    // attention.hip: fully issued tile loads, else a streaming loop
    static_assert((VR_KVT * KSTR * 2) % 16 == 0 && (VSTR * 2) % 8 == 0 && VSTR >= DV, "LDS carve / transposed-read alignment");
    __shared__ __attribute__((aligned(16))) bf16_t smem[VR_KVT * KSTR + VR_KVT * VSTR];
    bf16_t* Ks = smem;
    bf16_t* Vs = smem + VR_KVT * KSTR;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: every branch on it is a wave-level branch (EXEC stays all ones)
    const int half = lane >> 5;
    const int col = lane & 31;
    // XCD-aware order: the query blocks of (batch, head) pair bh = 8 * (idx / qblocks) + xcd run back to back on XCD xcd
    const int L = blockIdx.x, xcd = L & 7, idx = L >> 3;
    const int grp = idx / p.qblocks;
    const int bh = grp * 8 + xcd;
    if (bh >= p.BH) return;                  // the whole workgroup, before the first barrier
    const int qb = idx - grp * p.qblocks;
    const int b = bh / p.H, h = bh - b * p.H;
    const int d = p.d;
    const int q0 = qb * (NW * 32) + wave * 32;      // first query of this wave
    const int q = q0 + col;

    // ---- the key count of this batch: one load per workgroup, wave-uniform; out of range -> clamped for addressing, O = NaN ----
    int n_raw = p.Tk;
    if (p.klen) n_raw = __builtin_amdgcn_readfirstlane(p.klen[(long)b]);
    const bool bad = n_raw < 1 || n_raw > p.Tk;
    const int n = min(max(n_raw, 1), p.Tk);
    // causal: the workgroup's loop ends with its last query's key; this wave works on the tiles that start at or below its last query
    const int kend = CAUSAL ? min(n, (qb + 1) * (NW * 32)) : n;
    const int wlast = CAUSAL ? q0 + 31 : 0x7fffffff;

    // ---- Q fragments (B operand of S^T = K Q^T): lane -> query column, 8 consecutive dims ----
    Frag8 qf[D16];
    {
        const bf16_t* qp = p.Q + (long)b * p.sQ + (long)min(q, p.Tq - 1) * p.ldq + (long)h * d;
#pragma unroll
        for (int ks = 0; ks < D16; ++ks) {
            const int dd = ks * 16 + half * 8;
            const uint4 v = *(const uint4*)(qp + min(dd, d - 8));
            qf[ks].u = (q < p.Tq && dd < d) ? v : make_uint4(0, 0, 0, 0);
        }
    }

    f32x16_t oacc[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m_run = -INFINITY;
    float l_run = 0.f;
    const bf16_t* kbase = p.K + (long)b * p.sK + (long)h * d;
    const bf16_t* vbase = p.V + (long)b * p.sV + (long)h * d;
    // transposed reads: lane 4 qq + pp of its 16-lane group g reads row qq of the block, columns 4 pp .. 4 pp + 3; the block's columns are
    // 16 (g & 1) .. + 15 of the d tile, its rows start at 4 half of the k-step (second read: 8 rows further)
    const int l16 = lane & 15;
    const bf16_t* vr = Vs + (4 * half + (l16 >> 2)) * VSTR + 16 * ((lane >> 4) & 1) + 4 * (l16 & 3);

    for (int j0 = 0; j0 < kend; j0 += VR_KVT) {
        // ---- stage the K and V tiles: rows j0 .. j0 + 63, clamped to n - 1 and zeroed from n on ----
        if constexpr (UNR) {
            uint4 kreg[KCH];
            uint4 vreg[VCH];
#pragma unroll
            for (int i = 0; i < KCH; ++i) {
                const int c = tid + i * NT;
                const int row = c / (DP / 8);
                const int cc = c - row * (DP / 8);
                const bool ok = c < KTOT && j0 + row < n && cc * 8 < d;
                const int rr = min(j0 + row, n - 1), cq = min(cc * 8, d - 8);
                const uint4 v = *(const uint4*)(kbase + (long)rr * p.ldk + cq);
                kreg[i] = ok ? v : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < VCH; ++i) {
                const int c = tid + i * NT;
                const int row = c / (DV / 8);
                const int cc = c - row * (DV / 8);
                const bool ok = c < VTOT && j0 + row < n && cc * 8 < d;
                const int rr = min(j0 + row, n - 1), cq = min(cc * 8, d - 8);
                const uint4 v = *(const uint4*)(vbase + (long)rr * p.ldv + cq);
                vreg[i] = ok ? v : make_uint4(0, 0, 0, 0);
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
                const int row = c / (DV / 8);
                const int cc = c - row * (DV / 8);
                if (c < VTOT) *(uint4*)(Vs + row * VSTR + cc * 8) = vreg[i];
            }
        } else {
            for (int c = tid; c < KTOT; c += NT) {
                const int row = c / (DP / 8);
                const int cc = c - row * (DP / 8);
                uint4 v = make_uint4(0, 0, 0, 0);
                if (j0 + row < n && cc * 8 < d) v = *(const uint4*)(kbase + (long)(j0 + row) * p.ldk + cc * 8);
                *(uint4*)(Ks + row * KSTR + cc * 8) = v;
            }
            for (int c = tid; c < VTOT; c += NT) {
                const int row = c / (DV / 8);
                const int cc = c - row * (DV / 8);
                uint4 v = make_uint4(0, 0, 0, 0);
                if (j0 + row < n && cc * 8 < d) v = *(const uint4*)(vbase + (long)(j0 + row) * p.ldv + cc * 8);
                *(uint4*)(Vs + row * VSTR + cc * 8) = v;
            }
        }
        __syncthreads();

        if (j0 <= wlast) {                         // wave-uniform: a tile wholly above this wave's diagonal is skipped (causal)
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
            // ---- online softmax (this lane: one query, 32 of the 64 kv): scale, mask, then the maximum of the scaled values ----
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[sub][r] *= p.scale_log2;
            if (j0 + VR_KVT > n || (CAUSAL && j0 + VR_KVT - 1 > q0)) {      // the last tile and the diagonal tiles (wave-uniform branch)
#pragma unroll
                for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kv = j0 + sub * 32 + mfma32_row(r, lane);
                        if (kv >= n || (CAUSAL && kv > q)) sacc[sub][r] = -INFINITY;
                    }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[sub][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);       // finite: tile 0 holds key 0, which every query sees (n >= 1)
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // exp2(-inf) = 0 on the first tile
            m_run = m_new;
            float psum = 0.f;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(sacc[sub][r] - m_new);
                    sacc[sub][r] = pv;
                    psum += pv;
                }
            l_run = l_run * alpha + psum;
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;

            // ---- O^T[dd][q] += V^T[dd][kv] * P^T[kv][q]; V^T fragments by transposed reads of the row-major image ----
#pragma unroll
            for (int kstep = 0; kstep < 4; ++kstep) {
                const int sub = kstep >> 1, kk = kstep & 1;
                Frag8 pf;
                pf.u.x = pack2bf(sacc[sub][kk * 8 + 0], sacc[sub][kk * 8 + 1]);
                pf.u.y = pack2bf(sacc[sub][kk * 8 + 2], sacc[sub][kk * 8 + 3]);
                pf.u.z = pack2bf(sacc[sub][kk * 8 + 4], sacc[sub][kk * 8 + 5]);
                pf.u.w = pack2bf(sacc[sub][kk * 8 + 6], sacc[sub][kk * 8 + 7]);
#pragma unroll
                for (int i = 0; i < DT; ++i) {
                    const bf16_t* va = vr + kstep * 16 * VSTR + i * 32;
                    const vr_tr16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((vr_lds_tr_ptr_t)va);
                    const vr_tr16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((vr_lds_tr_ptr_t)(va + 8 * VSTR));
                    Frag8 vf;
                    vf.d2[0] = __builtin_bit_cast(uint2, lo);
                    vf.d2[1] = __builtin_bit_cast(uint2, hi);
                    oacc[i] = MDX_MFMA_32x32x16(vf.v, pf.v, oacc[i]);
                }
            }
        }
        __syncthreads();
    }
    const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32, 64));

    // ---- store O[q][h*d + dd]: lane has 4 consecutive dd per register group ----
    if (q < p.Tq) {
        bf16_t* op = p.O + (long)b * p.sO + (long)q * p.ldo + (long)h * d;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int dd = i * 32 + 8 * g + 4 * half;
                if (dd < d) {
                    uint2 ov;
                    ov.x = pack2bf(oacc[i][4 * g] * inv, oacc[i][4 * g + 1] * inv);
                    ov.y = pack2bf(oacc[i][4 * g + 2] * inv, oacc[i][4 * g + 3] * inv);
                    if (bad) ov = make_uint2(VR_NAN2, VR_NAN2);
                    *(uint2*)(op + dd) = ov;
                }
            }
    }
}

template <int D16, int NW>
static int launch_vrow(const SdpaParams& p, const char* op, hipStream_t st) {
    SdpaParams q = p;
    q.qblocks = (p.Tq + NW * 32 - 1) / (NW * 32);
    const long blocks = ((long)p.BH + 7) / 8 * 8 * q.qblocks;
    MDX_NEED(need_int(op, "B * H * query blocks", blocks));
    if (p.causal) hipLaunchKernelGGL((attn_vrow_kernel<D16, NW, true>), dim3((unsigned)blocks), dim3(NW * 64), 0, st, q);
    else hipLaunchKernelGGL((attn_vrow_kernel<D16, NW, false>), dim3((unsigned)blocks), dim3(NW * 64), 0, st, q);
    char tag[64];
    snprintf(tag, sizeof tag, "attn_vrow_kernel<%d,%d,%s>", D16, NW, p.causal ? "causal" : "full");
    return check_launch(tag);
}

template <int D16>
static int launch_vrow_nw(const SdpaParams& p, const char* op, hipStream_t st) {
    // attention.hip's rule (launch_attn_nw, same switches): 4 waves whenever (batch x heads) alone fills the chip, finer splits of the
    // sequence with few (batch, head) pairs.  The choice changes no bit of a result (the per-query arithmetic is lane-local).
    const long blocks4 = (long)((p.Tq + 127) / 128) * p.BH;
    const long blocks8 = (long)((p.Tq + 255) / 256) * p.BH;
    const long thr4 = (long)opt(OPT_ATTN_NW4_BLOCKS);
    const long thr8 = (long)opt(OPT_ATTN_NW8_BLOCKS);
    const int force = (int)opt(OPT_ATTN_NW);     // experiments: force 1 / 2 / 4 / 8 waves
    if (force == 8) return launch_vrow<D16, 8>(p, op, st);
    if (force == 4) return launch_vrow<D16, 4>(p, op, st);
    if (force == 2) return launch_vrow<D16, 2>(p, op, st);
    if (force == 1) return launch_vrow<D16, 1>(p, op, st);
    if (p.Tq >= 512 && blocks8 >= thr8) return launch_vrow<D16, 8>(p, op, st);
    if (p.Tq >= 256 && blocks4 >= thr4) return launch_vrow<D16, 4>(p, op, st);
    if ((long)p.BH >= 2 * thr4) return launch_vrow<D16, 4>(p, op, st);
    if (p.Tq >= 64) return launch_vrow<D16, 2>(p, op, st);
    return launch_vrow<D16, 1>(p, op, st);
}

}  // namespace mdx

using namespace mdx;

extern "C" int mdx_sdpa_bf16(const MdxSdpaDesc* a, void* stream) {
    const char* op = MDX_F16 ? "mdx_sdpa_f16" : "mdx_sdpa_bf16";
    if (!a) return set_error(MDX_EINVAL, "%s: null descriptor", op);
    if (!a->Q || !a->K || !a->V || !a->O) return set_error(MDX_EINVAL, "%s: null operand", op);
    if (a->causal != 0 && a->causal != 1) return set_error(MDX_EINVAL, "%s: causal=%ld must be 0 or 1", op, (long)a->causal);
    MDX_NEED(need_int(op, "B", a->B)); MDX_NEED(need_int(op, "H", a->H)); MDX_NEED(need_int(op, "Tq", a->Tq)); MDX_NEED(need_int(op, "Tk", a->Tk));
    if (a->B < 0 || a->H < 0 || a->Tq < 0 || a->Tk < 0)
        return set_error(MDX_EINVAL, "%s: B=%ld, H=%ld, Tq=%ld, Tk=%ld must not be negative", op, (long)a->B, (long)a->H, (long)a->Tq, (long)a->Tk);
    if (a->causal && a->Tq != a->Tk) return set_error(MDX_EINVAL, "%s: causal needs Tq == Tk (Tq=%ld, Tk=%ld)", op, (long)a->Tq, (long)a->Tk);
    const int d16 = (int)((a->d + 15) / 16);
    if (a->d <= 0 || a->d % 8 || a->d > 160 || d16 == 7 || d16 == 9)
        return set_error(MDX_EUNSUPPORTED, "%s: head dim d=%ld has no kernel instance (d %% 8 == 0, d <= 160, ceil(d / 16) in {1..6, 8, 10})", op, (long)a->d);
    // Q / K / V rows are read as 16-byte pieces; an O row is written as 8-byte pieces (4 head-dim columns of one query)
    MDX_NEED(need_multiple(op, "ldq", a->ldq, 8)); MDX_NEED(need_multiple(op, "ldk", a->ldk, 8)); MDX_NEED(need_multiple(op, "ldv", a->ldv, 8));
    MDX_NEED(need_multiple(op, "sQ", a->sQ, 8)); MDX_NEED(need_multiple(op, "sK", a->sK, 8)); MDX_NEED(need_multiple(op, "sV", a->sV, 8));
    MDX_NEED(need_multiple(op, "ldo", a->ldo, 4)); MDX_NEED(need_multiple(op, "sO", a->sO, 4));
    MDX_NEED(need_aligned(op, "Q", a->Q, 16)); MDX_NEED(need_aligned(op, "K", a->K, 16)); MDX_NEED(need_aligned(op, "V", a->V, 16));
    MDX_NEED(need_aligned(op, "O", a->O, 8)); MDX_NEED(need_aligned(op, "klen_dev", a->klen_dev, 4));
    const long hd = (long)a->H * a->d;
    if (a->ldq < hd) return set_error(MDX_EINVAL, "%s: ldq=%ld < H * d = %ld", op, (long)a->ldq, hd);
    if (a->ldk < hd) return set_error(MDX_EINVAL, "%s: ldk=%ld < H * d = %ld", op, (long)a->ldk, hd);
    if (a->ldv < hd) return set_error(MDX_EINVAL, "%s: ldv=%ld < H * d = %ld", op, (long)a->ldv, hd);
    if (a->ldo < hd) return set_error(MDX_EINVAL, "%s: ldo=%ld < H * d = %ld", op, (long)a->ldo, hd);
    if (a->Tq == 0 || a->Tk == 0 || a->B == 0 || a->H == 0) return MDX_OK;
    MDX_NEED(need_int(op, "B * H", a->B * a->H));
    SdpaParams p;
    p.Q = (const bf16_t*)a->Q; p.K = (const bf16_t*)a->K; p.V = (const bf16_t*)a->V; p.O = (bf16_t*)a->O;
    p.klen = a->klen_dev;
    p.BH = (int)(a->B * a->H); p.H = (int)a->H; p.Tq = (int)a->Tq; p.Tk = (int)a->Tk; p.d = (int)a->d; p.qblocks = 1; p.causal = (int)a->causal;
    p.ldq = a->ldq; p.sQ = a->sQ; p.ldk = a->ldk; p.sK = a->sK; p.ldv = a->ldv; p.sV = a->sV; p.ldo = a->ldo; p.sO = a->sO;
    p.scale_log2 = (float)(a->scale * 1.4426950408889634);
    hipStream_t st = (hipStream_t)stream;
    switch (d16) {
        case 1: return launch_vrow_nw<1>(p, op, st);
        case 2: return launch_vrow_nw<2>(p, op, st);
        case 3: return launch_vrow_nw<3>(p, op, st);
        case 4: return launch_vrow_nw<4>(p, op, st);
        case 5: return launch_vrow_nw<5>(p, op, st);
        case 6: return launch_vrow_nw<6>(p, op, st);
        case 8: return launch_vrow_nw<8>(p, op, st);
        default: return launch_vrow_nw<10>(p, op, st);
    }
}
