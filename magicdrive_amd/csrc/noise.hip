// noise.hip — the two ops whose Gaussian noise is made on the device (philox.h): mdx_latent_renoise_* (below) and mdx_cfg_ddim_eta_step_*
// (the DDIM step with eta > 0, further down).
// mdx_latent_renoise_*: one forward jump of the sampler with noise made on the device (MdxRenoiseDesc, include/mdx.h).
//
// RePaint resampling (Lugmayr et al. 2022) diffuses the sample forward again by `jump` steps with fresh noise and takes the same reverse
// steps once more.  With c = *step_ptr and v = *visit_ptr, read when the kernel runs (a replayed hipGraph sees the current values):
//     current = coef[c - 1][col_p]          the level the scheduler op of step c - 1 left the sample at
//     target  = coef[c - jump][col_t]       the level step c - jump expects
//     r = target / current, sg = sqrt(max(0, fma(-r, r, 1))), x[i] = fma(r, x[i], sg z[i])    q(x_{t+jump} | x_t) in one go
// and a separate one-thread launch behind it (the step_inc_kernel pattern of elementwise.hip: every block of the main launch has read
// the counters by then) sets *step_ptr = c - jump, *visit_ptr = v + 1.  jump < 1, c < 1, c > n_rows or c - jump < 0: x is filled with
// NaN (the library's signal, as ddim_kernel's for a step index of -1) and neither counter changes.
//
// z is a pure function of (seeds[g], v, e) for element e of group g = i / group_elems: Philox4x32-10 with counter
// (lo32(e / 4), hi32(e / 4), v, 0) and key (lo32(seed), hi32(seed)) gives four words for four consecutive e; Box-Muller on (w0, w1) gives
// z[4k], z[4k + 1], on (w2, w3) z[4k + 2], z[4k + 3] (include/mdx.h spells the mapping out).  Nothing depends on n, on the group's
// position or on the instance that served the call: no generator state lives in memory, so a scene has the same noise alone and in a batch.
//
// Two instances of one body, one thread per block of four e: VEC moves the four with one 16-byte access (the launcher asks for a
// 16-byte-aligned x and group_elems % 4 == 0, so every block is whole and aligned); the other moves 1 .. 4 elements one by one (the last
// block of a group whose size is no multiple of four is partial).  Per element the arithmetic is the same function: same bits.  x_in is
// refreshed element by element through store_xin (latent.h: the one copy of the refresh, shared with the scheduler kernels).  No atomics,
// 64-bit addressing.  The transcendentals are the accurate ones (logf, sqrtf, sincospif on the EXACT argument 2 u2): |z - fp64| stays
// below 1e-5 up to the largest radius sqrt(48 ln 2).
#include "common.h"
#include "launch.h"
#include "latent.h"
#include "philox.h"

namespace mdx {

#define RN_T 256

struct RenoiseParams { float* x; const float* coef; int* step; int* visit; const unsigned long long* seeds;
                       long group, bpg; int jump, n_rows, coef_ld, col_t, col_p; XinDst xin; };

__device__ __forceinline__ bool renoise_in_range(int c, int jump, int n_rows) { return jump >= 1 && c >= 1 && c <= n_rows && c - jump >= 0; }

__device__ __forceinline__ float renoise_value(float r, float sg, float x, float z) {
    float nz = sg * z;
    asm("" : "+v"(nz));                                        // a rounded product in both instances, never folded into the fma below
    return __builtin_fmaf(r, x, nz);
}

template <bool VEC>
__global__ __launch_bounds__(RN_T) void renoise_kernel(RenoiseParams p) {
    const int c = *p.step, v = *p.visit;
    const long q = (long)blockIdx.x * RN_T + threadIdx.x;       // block of four relative indices: group g, block k of the group
    const long g = q / p.bpg;
    if (g >= p.xin.n / p.group) return;
    const long k = q - g * p.bpg;
    const long e0 = 4 * k;
    const long i0 = g * p.group + e0;
    const int cnt = VEC ? 4 : (int)(p.group - e0 < 4 ? p.group - e0 : 4);       // VEC: group % 4 == 0, every block is whole
    if (!renoise_in_range(c, p.jump, p.n_rows)) {                // uniform over the launch: poison x, touch nothing else
        for (int j = 0; j < cnt; ++j) p.x[i0 + j] = __builtin_nanf("");
        return;
    }
    const float cur = p.coef[(long)(c - 1) * p.coef_ld + p.col_p], tgt = p.coef[(long)(c - p.jump) * p.coef_ld + p.col_t];
    const float r = tgt / cur;
    const float sg = sqrtf(fmaxf(0.0f, __builtin_fmaf(-r, r, 1.0f)));    // 1 - r r with ONE rounding, pinned (it cancels when r is near 1)
    const unsigned long long seed = p.seeds[g];
    float z[4];
    noise_block(seed, k, (unsigned)v, MDX_NOISE_DOMAIN_RENOISE, z);
    if (VEC) {
        const float4 x = *reinterpret_cast<const float4*>(p.x + i0);
        float4 y;
        y.x = renoise_value(r, sg, x.x, z[0]);
        y.y = renoise_value(r, sg, x.y, z[1]);
        y.z = renoise_value(r, sg, x.z, z[2]);
        y.w = renoise_value(r, sg, x.w, z[3]);
        *reinterpret_cast<float4*>(p.x + i0) = y;
        store_xin(p.xin, i0, y.x); store_xin(p.xin, i0 + 1, y.y); store_xin(p.xin, i0 + 2, y.z); store_xin(p.xin, i0 + 3, y.w);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < cnt) {
                const float y = renoise_value(r, sg, p.x[i0 + j], z[j]);
                p.x[i0 + j] = y;
                store_xin(p.xin, i0 + j, y);
            }
        }
    }
}

// behind renoise_kernel on the same stream: the counters move only when the jump was taken
__global__ void renoise_counters_kernel(int* step, int* visit, int jump, int n_rows) {
    const int c = *step;
    if (!renoise_in_range(c, jump, n_rows)) return;
    *step = c - jump;
    *visit += 1;
}

// ---- mdx_cfg_ddim_eta_step_*: the DDIM step with eta > 0 (MdxDdimEtaDesc, include/mdx.h) ------------------------------------------------
// ddim_kernel's update (elementwise.hip) plus the variance noise of scheduling_ddim.py:415-438, in one pass.  With s = *step_ptr and
// v = *draw_ptr read when the kernel runs, c = coef[s] (the UNCHANGED 4-column table) and (dir, sd) = var[s]:
//     e = cfg_eps(...), x0 = (x - c[1] e) / c[0], det = c[2] x0 + dir e, xn = sd != 0 ? det + rounded(sd z) : det, xn = gv_renoise(xn)
// A given element under gv_mode 2 takes e = gv_noise, dir = c[3] and no noise: it stays on its own add_noise trajectory.  z is noise[i]
// when the caller brings its own (variance_noise), else the block of philox.h with counter word 2 = v in the domain of this op: the
// renoise mapping with counter word 3 = 1.  sd == 0: no Philox is computed and the row's update is det — with dir = c[3], ddim_kernel's
// bits (the same expressions under the same flags).  The two instances are renoise_kernel's: one thread per four relative indices.
struct DdimEtaParams { float* x; const float* eps; const float* coef; const float* var; int* step; int* draw; const unsigned long long* seeds;
                       const float* noise; long group, bpg; int n_rows; float g; XinDst xin; GivenViews gv; };

__device__ __forceinline__ bool ddim_eta_in_range(int s, int n_rows) { return s >= 0 && s < n_rows; }

__device__ __forceinline__ float ddim_eta_value(const DdimEtaParams& p, const float* c, float dir, float sd, int step, long i, float x, float z) {
    float e = cfg_eps(p.eps, p.xin.n, p.xin.cfg, p.g, i);
    const bool given = gv_given(p.gv, i);
    if (given && p.gv.mode == 2) { e = p.gv.noise[i]; dir = c[3]; sd = 0.0f; }
    float x0 = (x - c[1] * e) / c[0];
    float det = c[2] * x0 + dir * e;
    asm("" : "+v"(det));                                       // det is ddim_kernel's value before anything is added to it
    float xn = det;
    if (sd != 0.0f) {
        float nz = sd * z;
        asm("" : "+v"(nz));                                    // a rounded product in both instances (renoise_value's pattern)
        xn = det + nz;
    }
    return gv_renoise(p.gv, given, step, i, c[2], c[3], xn);
}

template <bool VEC>
__global__ __launch_bounds__(RN_T) void ddim_eta_kernel(DdimEtaParams p) {
    const int s = *p.step, v = *p.draw;
    const long q = (long)blockIdx.x * RN_T + threadIdx.x;
    const long g = q / p.bpg;
    if (g >= p.xin.n / p.group) return;
    const long k = q - g * p.bpg;
    const long e0 = 4 * k;
    const long i0 = g * p.group + e0;
    const int cnt = VEC ? 4 : (int)(p.group - e0 < 4 ? p.group - e0 : 4);
    if (!ddim_eta_in_range(s, p.n_rows)) {                      // uniform over the launch: poison x, touch nothing else
        for (int j = 0; j < cnt; ++j) p.x[i0 + j] = __builtin_nanf("");
        return;
    }
    const float* c = p.coef + 4 * (long)s;
    const float dir = p.var[2 * (long)s], sd = p.var[2 * (long)s + 1];
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (sd != 0.0f) {                                           // uniform over the launch
        if (p.noise) {
            for (int j = 0; j < cnt; ++j) z[j] = p.noise[i0 + j];
        } else {
            noise_block(p.seeds[g], k, (unsigned)v, MDX_NOISE_DOMAIN_DDIM_ETA, z);
        }
    }
    if (VEC) {
        const float4 x = *reinterpret_cast<const float4*>(p.x + i0);
        float4 y;
        y.x = ddim_eta_value(p, c, dir, sd, s, i0, x.x, z[0]);
        y.y = ddim_eta_value(p, c, dir, sd, s, i0 + 1, x.y, z[1]);
        y.z = ddim_eta_value(p, c, dir, sd, s, i0 + 2, x.z, z[2]);
        y.w = ddim_eta_value(p, c, dir, sd, s, i0 + 3, x.w, z[3]);
        *reinterpret_cast<float4*>(p.x + i0) = y;
        store_xin(p.xin, i0, y.x); store_xin(p.xin, i0 + 1, y.y); store_xin(p.xin, i0 + 2, y.z); store_xin(p.xin, i0 + 3, y.w);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < cnt) {
                const float y = ddim_eta_value(p, c, dir, sd, s, i0 + j, p.x[i0 + j], z[j]);
                p.x[i0 + j] = y;
                store_xin(p.xin, i0 + j, y);
            }
        }
    }
}

// behind ddim_eta_kernel on the same stream: both counters move only when the step was taken
__global__ void ddim_eta_counters_kernel(int* step, int* draw, int n_rows) {
    if (!ddim_eta_in_range(*step, n_rows)) return;
    *step += 1;
    *draw += 1;
}

}  // namespace mdx

using namespace mdx;

extern "C" int mdx_cfg_ddim_eta_step_bf16(const MdxDdimEtaDesc* d, void* stream) {
#if MDX_F16
    const char* op = "mdx_cfg_ddim_eta_step_f16";
#else
    const char* op = "mdx_cfg_ddim_eta_step";
#endif
    if (!d) return set_error(MDX_EINVAL, "%s: null descriptor", op);
    if (!d->x) return set_error(MDX_EINVAL, "%s: x must not be NULL", op);
    if (!d->eps) return set_error(MDX_EINVAL, "%s: eps must not be NULL", op);
    if (!d->coef) return set_error(MDX_EINVAL, "%s: coef must not be NULL", op);
    if (!d->var) return set_error(MDX_EINVAL, "%s: var must not be NULL", op);
    if (!d->step_ptr) return set_error(MDX_EINVAL, "%s: step_ptr must not be NULL", op);
    if (!d->draw_ptr) return set_error(MDX_EINVAL, "%s: draw_ptr must not be NULL", op);
    if (!d->seeds && !d->noise) return set_error(MDX_EINVAL, "%s: seeds must not be NULL when noise is (one of the two makes z)", op);
    MDX_NEED(need_aligned(op, "x", d->x, 4)); MDX_NEED(need_aligned(op, "eps", d->eps, 4)); MDX_NEED(need_aligned(op, "coef", d->coef, 4));
    MDX_NEED(need_aligned(op, "var", d->var, 4)); MDX_NEED(need_aligned(op, "step_ptr", d->step_ptr, 4)); MDX_NEED(need_aligned(op, "draw_ptr", d->draw_ptr, 4));
    MDX_NEED(need_aligned(op, "seeds", d->seeds, 8)); MDX_NEED(need_aligned(op, "noise", d->noise, 4));
    MDX_NEED(need_int(op, "n_rows", d->n_rows)); MDX_NEED(need_int(op, "gv_last_step", d->gv_last_step));
    if (d->n < 0) return set_error(MDX_EINVAL, "%s: n=%ld must not be negative", op, (long)d->n);
    if (d->group_elems < 1 || d->n % d->group_elems) return set_error(MDX_EINVAL, "%s: group_elems=%ld must be >= 1 and divide n=%ld", op, (long)d->group_elems, (long)d->n);
    if (d->n_rows < 1) return set_error(MDX_EINVAL, "%s: n_rows=%ld must be >= 1", op, (long)d->n_rows);
    if (d->cfg != 0 && d->cfg != 1) return set_error(MDX_EINVAL, "%s: cfg=%ld must be 0 or 1", op, (long)d->cfg);
    MDX_NEED(need_xin(op, d));
    MDX_NEED(need_given_views(op, d));
    if (d->n == 0) return MDX_OK;
    const long bpg = (long)((d->group_elems + 3) / 4);           // blocks of four relative indices per group; the last may be partial
    DdimEtaParams p{d->x, d->eps, d->coef, d->var, d->step_ptr, d->draw_ptr, (const unsigned long long*)d->seeds, d->noise, d->group_elems, bpg,
                    (int)d->n_rows, (float)d->guidance, xin_of(d), given_views_of(d)};
    const bool vec = ((uintptr_t)d->x & 15) == 0 && d->group_elems % 4 == 0;
    const long work = (d->n / p.group) * bpg;
    const long blocks = (work + RN_T - 1) / RN_T;
    if (blocks > 0x7fffffffL) return set_error(MDX_EINVAL, "%s: n=%ld needs more than 2^31 - 1 workgroups", op, (long)d->n);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((ddim_eta_kernel<true>), dim3((unsigned)blocks), dim3(RN_T), 0, st, p);
    else hipLaunchKernelGGL((ddim_eta_kernel<false>), dim3((unsigned)blocks), dim3(RN_T), 0, st, p);
    MDX_NEED(check_launch(vec ? "ddim_eta_kernel" : "ddim_eta_kernel_scalar"));
    hipLaunchKernelGGL(ddim_eta_counters_kernel, dim3(1), dim3(1), 0, st, p.step, p.draw, p.n_rows);
    return check_launch("ddim_eta_counters_kernel", false);
}

extern "C" int mdx_latent_renoise_bf16(const MdxRenoiseDesc* d, void* stream) {
#if MDX_F16
    const char* op = "mdx_latent_renoise_f16";
#else
    const char* op = "mdx_latent_renoise";
#endif
    if (!d) return set_error(MDX_EINVAL, "%s: null descriptor", op);
    if (!d->x) return set_error(MDX_EINVAL, "%s: x must not be NULL", op);
    if (!d->coef) return set_error(MDX_EINVAL, "%s: coef must not be NULL", op);
    if (!d->step_ptr) return set_error(MDX_EINVAL, "%s: step_ptr must not be NULL", op);
    if (!d->visit_ptr) return set_error(MDX_EINVAL, "%s: visit_ptr must not be NULL", op);
    if (!d->seeds) return set_error(MDX_EINVAL, "%s: seeds must not be NULL", op);
    MDX_NEED(need_aligned(op, "x", d->x, 4)); MDX_NEED(need_aligned(op, "coef", d->coef, 4)); MDX_NEED(need_aligned(op, "step_ptr", d->step_ptr, 4));
    MDX_NEED(need_aligned(op, "visit_ptr", d->visit_ptr, 4)); MDX_NEED(need_aligned(op, "seeds", d->seeds, 8));
    MDX_NEED(need_int(op, "coef_ld", d->coef_ld)); MDX_NEED(need_int(op, "jump", d->jump)); MDX_NEED(need_int(op, "n_rows", d->n_rows));
    if (d->n < 0) return set_error(MDX_EINVAL, "%s: n=%ld must not be negative", op, (long)d->n);
    if (d->group_elems < 1 || d->n % d->group_elems) return set_error(MDX_EINVAL, "%s: group_elems=%ld must be >= 1 and divide n=%ld", op, (long)d->group_elems, (long)d->n);
    if (d->jump < 1) return set_error(MDX_EINVAL, "%s: jump=%ld must be >= 1", op, (long)d->jump);
    if (d->n_rows < 1) return set_error(MDX_EINVAL, "%s: n_rows=%ld must be >= 1", op, (long)d->n_rows);
    if (d->col_t < 0 || d->col_t >= d->coef_ld) return set_error(MDX_EINVAL, "%s: col_t=%ld must be in [0, coef_ld=%ld)", op, (long)d->col_t, (long)d->coef_ld);
    if (d->col_p < 0 || d->col_p >= d->coef_ld) return set_error(MDX_EINVAL, "%s: col_p=%ld must be in [0, coef_ld=%ld)", op, (long)d->col_p, (long)d->coef_ld);
    if (d->cfg != 0 && d->cfg != 1) return set_error(MDX_EINVAL, "%s: cfg=%ld must be 0 or 1", op, (long)d->cfg);
    MDX_NEED(need_xin(op, d));
    if (d->n == 0) return MDX_OK;
    const long bpg = (long)((d->group_elems + 3) / 4);           // blocks of four relative indices per group; the last may be partial
    RenoiseParams p{d->x, d->coef, d->step_ptr, d->visit_ptr, (const unsigned long long*)d->seeds, d->group_elems, bpg,
                    (int)d->jump, (int)d->n_rows, (int)d->coef_ld, (int)d->col_t, (int)d->col_p, xin_of(d)};
    const bool vec = ((uintptr_t)d->x & 15) == 0 && d->group_elems % 4 == 0;
    const long work = (d->n / p.group) * bpg;
    const long blocks = (work + RN_T - 1) / RN_T;
    if (blocks > 0x7fffffffL) return set_error(MDX_EINVAL, "%s: n=%ld needs more than 2^31 - 1 workgroups", op, (long)d->n);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((renoise_kernel<true>), dim3((unsigned)blocks), dim3(RN_T), 0, st, p);
    else hipLaunchKernelGGL((renoise_kernel<false>), dim3((unsigned)blocks), dim3(RN_T), 0, st, p);
    MDX_NEED(check_launch(vec ? "renoise_kernel" : "renoise_kernel_scalar"));
    hipLaunchKernelGGL(renoise_counters_kernel, dim3(1), dim3(1), 0, st, p.step, p.visit, p.jump, p.n_rows);
    return check_launch("renoise_counters_kernel", false);
}
