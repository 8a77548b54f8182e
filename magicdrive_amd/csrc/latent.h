// latent.h — what the ops that update the sampler's latents share (mdx_cfg_ddim_step, mdx_cfg_unipc_step, mdx_cfg_ddim_eta_step_*,
// mdx_latent_blend_*, mdx_latent_renoise_*): the refresh of the network's input copy x_in and, for the three scheduler ops, the CFG combine
// and the given views.
// ONE copy of each expression (as renoise_f in common.h), on the device and in the host checks: a new latent op embeds an XinDst in its
// kernel parameters, calls need_xin / xin_of in its entry point and store_xin in its kernel.
#pragma once
#include "common.h"
#include "launch.h"

namespace mdx {

// x_in (MdxDdimDesc.x_in and its namesakes): the model-input copy of the n latents, twice under CFG ([uncond | cond] halves).
//   xin_ld > 0: 16-bit channels-last, xin_c channels per pixel at a pixel stride of xin_ld elements (the pad channels are never written)
//   else      : fp32, flat
struct XinDst { void* x_in; long n; int cfg, xin_c, xin_ld; };

// the model-input copies of element i, whose new value is v; x_in == NULL: nothing is written
__device__ __forceinline__ void store_xin(const XinDst& d, long i, float v) {
    if (!d.x_in) return;
    if (d.xin_ld > 0) {
        const long px = i / d.xin_c;
        const int ch = (int)(i - px * d.xin_c);
        bf16_t* xi = (bf16_t*)d.x_in;
        const bf16_t h = f2bf(v);
        xi[px * d.xin_ld + ch] = h;
        if (d.cfg) xi[(d.n / d.xin_c + px) * d.xin_ld + ch] = h;
    } else {
        float* xi = (float*)d.x_in;
        xi[i] = v;
        if (d.cfg) xi[d.n + i] = v;
    }
}

// classifier-free guidance on eps = [uncond | cond]
__device__ __forceinline__ float cfg_eps(const float* eps, long n, int cfg, float g, long i) {
    if (!cfg) return eps[i];
    const float eu = eps[i], ec = eps[n + i];
    return eu + g * (ec - eu);
}

// given views (pipeline_bev_controlnet_given_view.py:263-291, 380-390; include/mdx.h: MdxDdimDesc.gv_*): mask has one byte per `view`
// consecutive elements; mode 2 steps a given view with its own noise as eps, mode 1 replaces the step's result below step `last`
struct GivenViews { const float* cond; const float* noise; const unsigned char* mask; int mode; long view; int last; };

__device__ __forceinline__ bool gv_given(const GivenViews& gv, long i) { return gv.mode != 0 && gv.mask[i / gv.view] != 0; }

// mode 1: a given element leaves the step as add_noise(cond, noise, next timestep), (a, s) = that timestep's (alpha, sigma)
__device__ __forceinline__ float gv_renoise(const GivenViews& gv, bool given, int step, long i, float a, float s, float xn) {
    return given && gv.mode == 1 && step < gv.last ? renoise_f(a, gv.cond[i], s, gv.noise[i]) : xn;
}

// ---- host: the descriptors name these fields alike, so one check serves all four (include/mdx.h lists the clauses) ----
template <class D> int need_xin(const char* op, const D* d) {
    MDX_NEED(need_int(op, "xin_c", d->xin_c)); MDX_NEED(need_int(op, "xin_ld", d->xin_ld));
    if (d->xin_ld < 0) return set_error(MDX_EINVAL, "%s: xin_ld=%ld must not be negative", op, (long)d->xin_ld);
    MDX_NEED(need_aligned(op, "x_in", d->x_in, d->xin_ld > 0 ? 2 : 4));
    if (d->xin_ld > 0 && (d->xin_c <= 0 || d->xin_c > d->xin_ld || d->n % d->xin_c))
        return set_error(MDX_EINVAL, "%s: xin_c=%ld must be in (0, xin_ld=%ld] and divide n=%ld (x_in channel layout)", op, (long)d->xin_c, (long)d->xin_ld, (long)d->n);
    return MDX_OK;
}
template <class D> XinDst xin_of(const D* d) { return XinDst{d->x_in, d->n, (int)d->cfg, (int)d->xin_c, (int)d->xin_ld}; }

// a NULL gv_mask switches the given views off whatever gv_mode says
template <class D> GivenViews given_views_of(const D* d) {
    return GivenViews{d->gv_cond, d->gv_noise, d->gv_mask, d->gv_mask ? (int)d->gv_mode : 0, d->gv_view_elems, (int)d->gv_last_step};
}
template <class D> int need_given_views(const char* op, const D* d) {
    const GivenViews gv = given_views_of(d);
    if (gv.mode != 0 && (gv.mode < 0 || gv.mode > 2 || !gv.noise || (gv.mode == 1 && !gv.cond) || gv.view <= 0 || d->n % gv.view))
        return set_error(MDX_EINVAL, "%s: given-view mode %d needs gv_noise (+ gv_cond for mode 1) and gv_view_elems dividing n", op, gv.mode);
    return MDX_OK;
}

}  // namespace mdx
