// attn_ctx_body.h — the body of attention_ctx.hip's kernels, included once per kernel (inside a function template with `int D` and the
// parameter `AttnCtxParams p`).  CTX_LIVE_COUNT is the expression that loads the live key count: *p.tk_dev for the whole launch
// (attn_ctx_kernel) or p.tk_dev[b] for the workgroup's query batch b (attn_ctx_rows_kernel).  Textual on purpose: with the body shared
// through a __device__ function template the scalar-count kernels came out with a different register allocation than before; this way
// their preprocessed source is unchanged.  The design notes are at the top of attention_ctx.hip.
#ifndef CTX_LIVE_COUNT
#error "define CTX_LIVE_COUNT before including attn_ctx_body.h"
#endif
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
    const int n_raw = __builtin_amdgcn_readfirstlane(CTX_LIVE_COUNT);
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
