// blend.hip — mdx_latent_blend_*: keep known regions of the latents while sampling (MdxBlendDesc, include/mdx.h).
//
// The per-pixel, fractional form of the schedulers' gv_mode 1 (pipeline_bev_controlnet_given_view.py:283-295): behind the scheduler op of
// step s < last_step, element i with mask value m = mask[i / mask_elems] becomes
//     m == 0 : untouched (x and its x_in copies keep the scheduler op's bits: the element is not even read)
//     m == 1 : t = a cond + sg noise                  (renoise_f, common.h: the expression ddim_kernel / unipc_kernel use)
//     else   : fmaf(m, t - x, x)
// with (a, sg) = coef[s][col_a], coef[s][col_s] = (alpha, sigma) of the NEXT timestep and s = *step_ptr - 1 (the scheduler op has
// already advanced the counter), read when the kernel runs.  s outside [0, last_step) writes nothing.
//
// Two instances of one body: VEC takes four consecutive elements per thread with 16-byte accesses of x / cond / noise (the launcher asks
// for 16-byte-aligned pointers and mask_elems % 4 == 0, so the four share one mask entry and n % 4 == 0); the other takes one element per
// thread.  Per element the arithmetic is the same function: same bits.  x_in is refreshed element by element through store_xin
// (latent.h: the one copy of the refresh, shared with the scheduler kernels; its pixel stride need not keep four channels together).
// No atomics, 64-bit addressing, one launch; the work is ~7 fp32 streams of n elements: at the plan's n = views * h * w * 4 a few
// microseconds behind a step of milliseconds.
#include "common.h"
#include "launch.h"
#include "latent.h"

namespace mdx {

#define BL_T 256

struct BlendParams { float* x; const float* cond; const float* noise; const float* mask; const float* coef; const int* step;
                     long mask_elems; int coef_ld, col_a, col_s, last; XinDst xin; };

__device__ __forceinline__ float blend_value(float m, float a, float sg, float c, float nz, float x) {
    const float t = renoise_f(a, c, sg, nz);
    return m == 1.0f ? t : __builtin_fmaf(m, t - x, x);
}

template <bool VEC>
__global__ __launch_bounds__(BL_T) void blend_kernel(BlendParams p) {
    const int s = *p.step - 1;
    if (s < 0 || s >= p.last) return;                           // uniform over the launch: nothing is written
    const long q = (long)blockIdx.x * BL_T + threadIdx.x;
    const long i = VEC ? 4 * q : q;
    if (i >= p.xin.n) return;                                   // VEC: n % 4 == 0, so i < n means i + 3 < n
    const float m = p.mask[i / p.mask_elems];                   // VEC: mask_elems % 4 == 0, one entry for the four
    if (m == 0.0f) return;
    const float a = p.coef[(long)s * p.coef_ld + p.col_a], sg = p.coef[(long)s * p.coef_ld + p.col_s];
    if (VEC) {
        const float4 c = *reinterpret_cast<const float4*>(p.cond + i);
        const float4 nz = *reinterpret_cast<const float4*>(p.noise + i);
        const float4 x = *reinterpret_cast<const float4*>(p.x + i);
        float4 y;
        y.x = blend_value(m, a, sg, c.x, nz.x, x.x);
        y.y = blend_value(m, a, sg, c.y, nz.y, x.y);
        y.z = blend_value(m, a, sg, c.z, nz.z, x.z);
        y.w = blend_value(m, a, sg, c.w, nz.w, x.w);
        *reinterpret_cast<float4*>(p.x + i) = y;
        store_xin(p.xin, i, y.x); store_xin(p.xin, i + 1, y.y); store_xin(p.xin, i + 2, y.z); store_xin(p.xin, i + 3, y.w);
    } else {
        const float y = blend_value(m, a, sg, p.cond[i], p.noise[i], p.x[i]);
        p.x[i] = y;
        store_xin(p.xin, i, y);
    }
}

}  // namespace mdx

using namespace mdx;

extern "C" int mdx_latent_blend_bf16(const MdxBlendDesc* d, void* stream) {
#if MDX_F16
    const char* op = "mdx_latent_blend_f16";
#else
    const char* op = "mdx_latent_blend";
#endif
    if (!d) return set_error(MDX_EINVAL, "%s: null descriptor", op);
    if (!d->x) return set_error(MDX_EINVAL, "%s: x must not be NULL", op);
    if (!d->cond) return set_error(MDX_EINVAL, "%s: cond must not be NULL", op);
    if (!d->noise) return set_error(MDX_EINVAL, "%s: noise must not be NULL", op);
    if (!d->mask) return set_error(MDX_EINVAL, "%s: mask must not be NULL", op);
    if (!d->coef) return set_error(MDX_EINVAL, "%s: coef must not be NULL", op);
    if (!d->step_ptr) return set_error(MDX_EINVAL, "%s: step_ptr must not be NULL", op);
    MDX_NEED(need_aligned(op, "x", d->x, 4)); MDX_NEED(need_aligned(op, "cond", d->cond, 4)); MDX_NEED(need_aligned(op, "noise", d->noise, 4));
    MDX_NEED(need_aligned(op, "mask", d->mask, 4)); MDX_NEED(need_aligned(op, "coef", d->coef, 4)); MDX_NEED(need_aligned(op, "step_ptr", d->step_ptr, 4));
    MDX_NEED(need_int(op, "coef_ld", d->coef_ld)); MDX_NEED(need_int(op, "last_step", d->last_step));
    if (d->n < 0) return set_error(MDX_EINVAL, "%s: n=%ld must not be negative", op, (long)d->n);
    if (d->mask_elems < 1 || d->n % d->mask_elems) return set_error(MDX_EINVAL, "%s: mask_elems=%ld must be >= 1 and divide n=%ld", op, (long)d->mask_elems, (long)d->n);
    if (d->col_a < 0 || d->col_a >= d->coef_ld) return set_error(MDX_EINVAL, "%s: col_a=%ld must be in [0, coef_ld=%ld)", op, (long)d->col_a, (long)d->coef_ld);
    if (d->col_s < 0 || d->col_s >= d->coef_ld) return set_error(MDX_EINVAL, "%s: col_s=%ld must be in [0, coef_ld=%ld)", op, (long)d->col_s, (long)d->coef_ld);
    if (d->cfg != 0 && d->cfg != 1) return set_error(MDX_EINVAL, "%s: cfg=%ld must be 0 or 1", op, (long)d->cfg);
    MDX_NEED(need_xin(op, d));
    if (d->n == 0) return MDX_OK;
    BlendParams p{d->x, d->cond, d->noise, d->mask, d->coef, d->step_ptr, d->mask_elems, (int)d->coef_ld, (int)d->col_a, (int)d->col_s,
                  (int)d->last_step, xin_of(d)};
    const bool vec = (((uintptr_t)d->x | (uintptr_t)d->cond | (uintptr_t)d->noise) & 15) == 0 && d->mask_elems % 4 == 0;
    const long work = vec ? d->n / 4 : d->n;
    const long blocks = (work + BL_T - 1) / BL_T;
    if (blocks > 0x7fffffffL) return set_error(MDX_EINVAL, "%s: n=%ld needs more than 2^31 - 1 workgroups", op, (long)d->n);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((blend_kernel<true>), dim3((unsigned)blocks), dim3(BL_T), 0, st, p);
    else hipLaunchKernelGGL((blend_kernel<false>), dim3((unsigned)blocks), dim3(BL_T), 0, st, p);
    return check_launch(vec ? "blend_kernel" : "blend_kernel_scalar");
}
