// composite.hip — mdx_image_composite_*: composite a kept-region edit with the recorded pictures (MdxCompositeDesc, include/mdx.h).
//
// Per view: a(y, x) = keep[y / f][x / f] (nearest upsample of the latent keep mask), e = min of a over the (2r+1)^2 window (erosion),
// w = (fp32 sum of e over the (2r+1)^2 window) / (2r+1)^2 (the matte), all coordinates clamped to the image; then per pixel and channel
//     g = clamp01(float(round16(fmaf(gen, 0.5, 0.5))))         (the bits of (image / 2 + 0.5).clamp(0, 1).float(); NaN stays NaN)
//     w == 0 : out = g;   w == 1 : out = orig;   else : out = fmaf(w, orig - g, g).
//
// One launch, one workgroup of 256 threads per (view, 32 x 64 pixel tile).  The matte runs out of LDS in four passes over two buffers:
//     A <- the tile's patch of keep cells, halo of 2r pixels included              (staged once, the only read of keep)
//     B <- hmin[ay][ix] = min over the window's columns of row ay                  (TH + 4r rows x TW + 2r columns; reads cells)
//     A <- e[iy][ix]    = min over the window's rows of hmin                       (TH + 2r x TW + 2r)
//     B <- hs[iy][x]    = sequential sum of e over the window's columns            (TH + 2r x TW)
// and each thread sums its 8 pixels' columns of hs sequentially and divides once.  e at a position outside the image is e at the clamped
// position (whose own window is clamped again): what replicate padding of e means.  Then the thread blends its 8 pixels of one row:
// C x 16 bytes of planar gen in, 8 C floats of channels-last orig in and out.  The LDS is sized by (r, f) per launch: 28 KB at r = 4,
// f = 8 (five workgroups per CU), 86 KB at the cap r = 16 with f = 1 (one) — CDNA4 has 160 KB per CU.
// 16-byte accesses where alignment allows (gen: pointer and the three strides; orig / out: pointers and W C % 4 == 0; matte: pointer
// and W % 4 == 0) and the thread's 8 pixels lie inside the row; otherwise scalar accesses: per element the arithmetic is the same
// function, same bits.  fp32 math, no atomics, 64-bit addressing; a view's bits depend on that view's operands only.
#include "common.h"
#include "launch.h"

namespace mdx {

#define CP_T 256
#define CP_TH 32
#define CP_TW 64
#define CP_G 8                       // pixels per thread: CP_TH * CP_TW == CP_T * CP_G
#define CP_RMAX 16

struct CompositeParams { const void* gen; const float* orig; const float* keep; float* out; float* matte; const unsigned char* has;
                         long g_sv, g_sc, g_ld; int C, H, W, f, r, gen_f32, tiles_x, tiles_y, a_floats, gvec, ovec, mvec; };

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// torch.clamp(0, 1): a NaN fails both comparisons and stays, +Inf -> 1, -Inf -> 0 (fminf / fmaxf would swallow the NaN)
__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
__device__ __forceinline__ float plain_value(float x, bool f32) {
    float t = __builtin_fmaf(x, 0.5f, 0.5f);
    if (!f32) t = bf2f(f2bf(t));
    return clamp01(t);
}
__device__ __forceinline__ float composite_value(float w, float o, float g) {
    return w == 0.0f ? g : (w == 1.0f ? o : __builtin_fmaf(w, o - g, g));
}

// one thread's 8 pixels (npx of them inside the row) of row y from column x0, C channels
template <int C>
__device__ __forceinline__ void composite_unit(const CompositeParams& p, int v, int y, int x0, int npx, const float (&w)[CP_G], bool has) {
    const bool full = npx == CP_G;
    const bool f32 = p.gen_f32 != 0;
    float g[C][CP_G];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const long gb = (long)v * p.g_sv + (long)c * p.g_sc + (long)y * p.g_ld + x0;
        float x[CP_G];
        if (f32) {
            const float* gp = (const float*)p.gen + gb;
            if (p.gvec && full) {
                const float4 a = *reinterpret_cast<const float4*>(gp), b = *reinterpret_cast<const float4*>(gp + 4);
                x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
            } else {
#pragma unroll
                for (int k = 0; k < CP_G; ++k) x[k] = k < npx ? gp[k] : 0.0f;
            }
        } else {
            const bf16_t* gp = (const bf16_t*)p.gen + gb;
            if (p.gvec && full) {
                const uint4 u = *reinterpret_cast<const uint4*>(gp);
                const unsigned q[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) { x[2 * k] = bf2f((bf16_t)(q[k] & 0xffffu)); x[2 * k + 1] = bf2f((bf16_t)(q[k] >> 16)); }
            } else {
#pragma unroll
                for (int k = 0; k < CP_G; ++k) x[k] = k < npx ? bf2f(gp[k]) : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < CP_G; ++k) g[c][k] = plain_value(x[k], f32);
    }
    const long ob = (((long)v * p.H + y) * p.W + x0) * C;
    const int cnt = npx * C;
    float res[CP_G * C];
    if (has) {
        float o[CP_G * C];
        if (p.ovec && full) {
#pragma unroll
            for (int q = 0; q < 2 * C; ++q) {
                const float4 t = reinterpret_cast<const float4*>(p.orig + ob)[q];
                o[4 * q] = t.x; o[4 * q + 1] = t.y; o[4 * q + 2] = t.z; o[4 * q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < CP_G * C; ++j) o[j] = j < cnt ? p.orig[ob + j] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < CP_G; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) res[k * C + c] = composite_value(w[k], o[k * C + c], g[c][k]);
    } else {
#pragma unroll
        for (int k = 0; k < CP_G; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) res[k * C + c] = g[c][k];
    }
    if (p.ovec && full) {
#pragma unroll
        for (int q = 0; q < 2 * C; ++q) {
            float4 t; t.x = res[4 * q]; t.y = res[4 * q + 1]; t.z = res[4 * q + 2]; t.w = res[4 * q + 3];
            reinterpret_cast<float4*>(p.out + ob)[q] = t;
        }
    } else {
#pragma unroll
        for (int j = 0; j < CP_G * C; ++j)
            if (j < cnt) p.out[ob + j] = res[j];
    }
}

__global__ __launch_bounds__(CP_T) void composite_kernel(CompositeParams p) {
    extern __shared__ float cp_lds[];
    const int tiles = p.tiles_x * p.tiles_y;
    const int v = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x - (unsigned)v * (unsigned)tiles);
    const int ty0 = (t / p.tiles_x) * CP_TH, tx0 = (t % p.tiles_x) * CP_TW;
    const int tid = threadIdx.x, r = p.r, f = p.f, H = p.H, W = p.W;
    const bool has = !p.has || p.has[v] != 0;                     // uniform over the workgroup
    const int EW = CP_TW + 2 * r, EH = CP_TH + 2 * r, AH = CP_TH + 4 * r;
    float* bufA = cp_lds;
    float* bufB = cp_lds + p.a_floats;
    if (has) {
        // A <- keep cells of the rows / columns clamp(tile -+ 2r)
        const int cy0 = clampi(ty0 - 2 * r, H - 1) / f, cy1 = clampi(ty0 + CP_TH - 1 + 2 * r, H - 1) / f;
        const int cx0 = clampi(tx0 - 2 * r, W - 1) / f, cx1 = clampi(tx0 + CP_TW - 1 + 2 * r, W - 1) / f;
        const int ch = cy1 - cy0 + 1, cw = cx1 - cx0 + 1, wl = W / f;
        const float* kv = p.keep + (long)v * (H / f) * wl;
        for (int i = tid; i < ch * cw; i += CP_T) {
            const int cr = i / cw, cc = i - cr * cw;
            bufA[i] = kv[(long)(cy0 + cr) * wl + cx0 + cc];
        }
        __syncthreads();
        // B <- hmin: row ay is image row clamp(ty0 - 2r + ay), column ix is centred at clamp(tx0 - r + ix); a is constant over a cell,
        // so the min over the window's pixels is the min over the cells they touch
        for (int i = tid; i < AH * EW; i += CP_T) {
            const int ay = i / EW, ix = i - ay * EW;
            const int row = clampi(ty0 - 2 * r + ay, H - 1), cx = clampi(tx0 - r + ix, W - 1);
            const float* crow = bufA + (row / f - cy0) * cw - cx0;
            const int c0 = clampi(cx - r, W - 1) / f, c1 = clampi(cx + r, W - 1) / f;
            float m = crow[c0];
            for (int c = c0 + 1; c <= c1; ++c) m = fminf(m, crow[c]);
            bufB[i] = m;
        }
        __syncthreads();
        // A <- e: row iy is centred at cy = clamp(ty0 - r + iy); image row cy + dy sits at hmin row cy + dy - (ty0 - 2r)
        for (int i = tid; i < EH * EW; i += CP_T) {
            const int iy = i / EW, ix = i - iy * EW;
            const int cy = clampi(ty0 - r + iy, H - 1);
            const float* col = bufB + (cy - ty0 + r) * EW + ix;
            float m = col[0];
            for (int d = 1; d <= 2 * r; ++d) m = fminf(m, col[d * EW]);
            bufA[i] = m;
        }
        __syncthreads();
        // B <- hs: sequential sum over the window's columns
        for (int i = tid; i < EH * CP_TW; i += CP_T) {
            const int iy = i / CP_TW, x = i - iy * CP_TW;
            const float* rowp = bufA + iy * EW + x;
            float s = rowp[0];
            for (int d = 1; d <= 2 * r; ++d) s += rowp[d];
            bufB[i] = s;
        }
        __syncthreads();
    }
    const int ly = tid / (CP_TW / CP_G), lx = tid - ly * (CP_TW / CP_G);
    const int y = ty0 + ly, x0 = tx0 + lx * CP_G;
    if (y >= H || x0 >= W) return;
    const int npx = W - x0 < CP_G ? W - x0 : CP_G;
    float w[CP_G];
    if (has) {
        const float n2 = (float)((2 * r + 1) * (2 * r + 1));
#pragma unroll
        for (int k = 0; k < CP_G; ++k) {
            const float* col = bufB + ly * CP_TW + lx * CP_G + k;
            float s = col[0];
            for (int d = 1; d <= 2 * r; ++d) s += col[d * CP_TW];
            w[k] = s / n2;
        }
    } else {
#pragma unroll
        for (int k = 0; k < CP_G; ++k) w[k] = 0.0f;
    }
    if (p.matte) {
        float* mp = p.matte + ((long)v * H + y) * W + x0;
        if (p.mvec && npx == CP_G) {
            float4 a, b;
            a.x = w[0]; a.y = w[1]; a.z = w[2]; a.w = w[3]; b.x = w[4]; b.y = w[5]; b.z = w[6]; b.w = w[7];
            reinterpret_cast<float4*>(mp)[0] = a;
            reinterpret_cast<float4*>(mp)[1] = b;
        } else {
#pragma unroll
            for (int k = 0; k < CP_G; ++k)
                if (k < npx) mp[k] = w[k];
        }
    }
    switch (p.C) {
        case 1: composite_unit<1>(p, v, y, x0, npx, w, has); break;
        case 2: composite_unit<2>(p, v, y, x0, npx, w, has); break;
        case 3: composite_unit<3>(p, v, y, x0, npx, w, has); break;
        default: composite_unit<4>(p, v, y, x0, npx, w, has); break;
    }
}

}  // namespace mdx

using namespace mdx;

extern "C" int mdx_image_composite_bf16(const MdxCompositeDesc* d, void* stream) {
#if MDX_F16
    const char* op = "mdx_image_composite_f16";
#else
    const char* op = "mdx_image_composite";
#endif
    if (!d) return set_error(MDX_EINVAL, "%s: null descriptor", op);
    if (!d->gen) return set_error(MDX_EINVAL, "%s: gen must not be NULL", op);
    if (!d->orig) return set_error(MDX_EINVAL, "%s: orig must not be NULL", op);
    if (!d->keep) return set_error(MDX_EINVAL, "%s: keep must not be NULL", op);
    if (!d->out) return set_error(MDX_EINVAL, "%s: out must not be NULL", op);
    if (d->gen_f32 != 0 && d->gen_f32 != 1) return set_error(MDX_EINVAL, "%s: gen_f32=%ld must be 0 or 1", op, (long)d->gen_f32);
    MDX_NEED(need_aligned(op, "gen", d->gen, d->gen_f32 ? 4 : 2));
    MDX_NEED(need_aligned(op, "orig", d->orig, 4)); MDX_NEED(need_aligned(op, "keep", d->keep, 4));
    MDX_NEED(need_aligned(op, "out", d->out, 4)); MDX_NEED(need_aligned(op, "matte", d->matte, 4));
    MDX_NEED(need_int(op, "V", d->V)); MDX_NEED(need_int(op, "C", d->C)); MDX_NEED(need_int(op, "H", d->H)); MDX_NEED(need_int(op, "W", d->W));
    MDX_NEED(need_int(op, "f", d->f)); MDX_NEED(need_int(op, "feather", d->feather));
    if (d->V < 0) return set_error(MDX_EINVAL, "%s: V=%ld must not be negative", op, (long)d->V);
    if (d->C < 1 || d->C > 4) return set_error(MDX_EINVAL, "%s: C=%ld must be in [1, 4]", op, (long)d->C);
    if (d->H < 1) return set_error(MDX_EINVAL, "%s: H=%ld must be >= 1", op, (long)d->H);
    if (d->W < 1) return set_error(MDX_EINVAL, "%s: W=%ld must be >= 1", op, (long)d->W);
    if (d->H * d->W > 0x7fffffffL) return set_error(MDX_EINVAL, "%s: H=%ld times W=%ld does not fit a 32-bit int", op, (long)d->H, (long)d->W);
    if (d->f < 1 || d->H % d->f || d->W % d->f) return set_error(MDX_EINVAL, "%s: f=%ld must be >= 1 and divide H=%ld and W=%ld", op, (long)d->f, (long)d->H, (long)d->W);
    if (d->feather < 0 || d->feather > CP_RMAX) return set_error(MDX_EINVAL, "%s: feather=%ld must be in [0, %d]", op, (long)d->feather, CP_RMAX);
    if (d->g_ld < d->W) return set_error(MDX_EINVAL, "%s: g_ld=%ld must be >= W=%ld", op, (long)d->g_ld, (long)d->W);
    if (d->g_sc < 0) return set_error(MDX_EINVAL, "%s: g_sc=%ld must not be negative", op, (long)d->g_sc);
    if (d->g_sv < 0) return set_error(MDX_EINVAL, "%s: g_sv=%ld must not be negative", op, (long)d->g_sv);
    if (d->V == 0) return MDX_OK;
    const int H = (int)d->H, W = (int)d->W, f = (int)d->f, r = (int)d->feather, C = (int)d->C;
    const int tiles_x = (W + CP_TW - 1) / CP_TW, tiles_y = (H + CP_TH - 1) / CP_TH;
    const long blocks = d->V * (long)tiles_x * tiles_y;
    if (blocks > 0x7fffffffL) return set_error(MDX_EINVAL, "%s: V=%ld views of %d tiles need more than 2^31 - 1 workgroups", op, (long)d->V, tiles_x * tiles_y);
    // LDS: A = max(cell patch, e), B = hmin (>= hs).  A span of S pixels touches at most (S + f - 2) / f + 1 cells, and no more than exist.
    const int EW = CP_TW + 2 * r, EH = CP_TH + 2 * r, AH = CP_TH + 4 * r;
    const int crb = std::min(H / f, (CP_TH + 4 * r + f - 2) / f + 1), ccb = std::min(W / f, (CP_TW + 4 * r + f - 2) / f + 1);
    const int a_floats = std::max(crb * ccb, EH * EW), b_floats = AH * EW;
    const size_t smem = (size_t)(a_floats + b_floats) * sizeof(float);
    constexpr size_t smem_cap = (size_t)((CP_TH + 4 * CP_RMAX) * (CP_TW + 4 * CP_RMAX) + (CP_TH + 4 * CP_RMAX) * (CP_TW + 2 * CP_RMAX)) * sizeof(float);
    if (smem > smem_cap) return set_error(MDX_EINVAL, "%s: internal: %zu bytes of LDS exceed the cap %zu", op, smem, smem_cap);
    MDX_NEED(ensure_dyn_smem((const void*)composite_kernel, smem_cap, "composite"));
    const long es = d->gen_f32 ? 4 : 2;
    const int gvec = (((uintptr_t)d->gen | (uintptr_t)(d->g_ld * es) | (uintptr_t)(d->g_sc * es) | (uintptr_t)(d->g_sv * es)) & 15) == 0;
    const int ovec = ((((uintptr_t)d->orig | (uintptr_t)d->out) & 15) == 0) && ((long)W * C) % 4 == 0;
    const int mvec = d->matte && (((uintptr_t)d->matte & 15) == 0) && W % 4 == 0;
    CompositeParams p{d->gen, d->orig, d->keep, d->out, d->matte, d->has, (long)d->g_sv, (long)d->g_sc, (long)d->g_ld,
                      C, H, W, f, r, (int)d->gen_f32, tiles_x, tiles_y, a_floats, gvec, ovec, mvec};
    hipLaunchKernelGGL(composite_kernel, dim3((unsigned)blocks), dim3(CP_T), smem, (hipStream_t)stream, p);
    return check_launch(gvec && ovec ? "composite_kernel" : "composite_kernel_scalar");
}
