"""-m gpu: composite_kernel (csrc/composite.hip, mdx_image_composite_*, ops.ImageComposite) against a float64 restatement, in both 16-bit
builds and with an fp32 gen, and pipe.composite_images on the tiny nets.

The reference has no composite, so there is no golden: the yardstick is float64 torch on the same inputs (tests/composite_cases.py).
Per case (shape x feather x gen type), on masks of the 1/64 grid where every window sum is exact in fp32:
  w == 0 pixels      out is bit-equal to torch's (gen / 2 + 0.5).clamp(0, 1).float() evaluated on the GPU;
  w == 1 pixels      out is bit-equal to orig;
  fractional pixels  |out - ref64| <= 4 * 2^-24: operands in [0, 1], S exact, one rounding each in the division, in o - g and in the fma;
  matte              |matte - w64| <= 2^-24 (the division); an off-grid mask is held to (2 (2r+1) + 2) * 2^-24: two sequential fp32 sums
                     of 2r+1 terms plus the division.
Each case asserts on the REFERENCE matte that the three regimes hold at least 5 % of the pixels each.  Then the edges of the contract:
a strided gen, orig / out moved by 4 bytes, has == 0 over NaN rows, non-finite gen, guard bands, determinism, the kernel's name.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import composite_cases as CC  # noqa: E402
from magicdrive_amd import _lib as L, ops as O  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
EPS = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def reference_matte(ci, r):
    """float64 [V, H, W] on the CPU, computed once per (case, feather) and never written to."""
    return CC.matte64(CC.keep_mask(ci), CC.CASES[ci][0][3], r)


@functools.lru_cache(maxsize=None)
def operands(ci, dt):
    """(gen [V, 3, H, W] in [-1.2, 1.2] of the given type, orig fp32 [V, H, W, 3] = k / 255), on the CPU, once per (case, type)."""
    V, H, W, _ = CC.CASES[ci][0]
    g = torch.Generator().manual_seed(77 + ci)
    gen = ((torch.rand(V, 3, H, W, generator=g) * 2.4 - 1.2)).to(DTYPES[dt])
    orig = torch.randint(0, 256, (V, H, W, 3), generator=g).float() / 255.0
    return gen, orig


def plain(gen):
    """Today's path, evaluated by torch on the GPU: [V, C, H, W] -> fp32 [V, H, W, C]."""
    return (gen / 2 + 0.5).clamp(0, 1).float().permute(0, 2, 3, 1).contiguous()


def run(gen, orig, keep, r, matte=True, has=None, out=None, matte_buf=None):
    V, C, H, W = gen.shape
    out = torch.empty(V, H, W, C, dtype=torch.float32, device=gen.device) if out is None else out
    m = (torch.empty(V, H, W, dtype=torch.float32, device=gen.device) if matte_buf is None else matte_buf) if matte else None
    O.run_ops([O.ImageComposite(gen, orig, keep, out, r, matte=m, has=has)])
    torch.cuda.synchronize()
    return out, m


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("ci,r", CC.GRID, ids=CC.GRID_IDS)
def test_against_float64(dev, ci, r, dt):
    f = CC.CASES[ci][0][3]
    w64 = reference_matte(ci, r)
    z, o, m = CC.regime_shares(w64)
    assert min(z, o, m) >= 0.05, f"the case does not exercise every regime: w==0 {z:.3f}, w==1 {o:.3f}, between {m:.3f}"
    gen, orig = (t.to(dev) for t in operands(ci, dt))
    keep = CC.keep_mask(ci).to(dev)
    out, matte = run(gen, orig, keep, r)
    assert (L.lib().mdx_last_kernel() or b"").decode().startswith("composite_kernel")
    g = plain(gen)
    w64d = w64.to(dev)
    merr = float((matte.double() - w64d).abs().max())
    print(f"{CC.GRID_IDS[CC.GRID.index((ci, r))]} {dt}: max |matte - w64| = {merr:.3e}")
    assert merr <= EPS
    zero, one = (w64d == 0), (w64d == 1)
    assert torch.equal(matte == 0, zero) and torch.equal(matte == 1, one), "the matte's exact regimes differ from the reference's"
    assert torch.equal(bits(out)[zero], bits(g)[zero]), "w == 0: not the bits of (gen / 2 + 0.5).clamp(0, 1).float()"
    assert torch.equal(bits(out)[one], bits(orig)[one]), "w == 1: not the recorded pixel"
    frac = ~(zero | one)
    ref = g.double() + w64d[..., None] * (orig.double() - g.double())
    err = float((out.double() - ref)[frac].abs().max())
    print(f"{CC.GRID_IDS[CC.GRID.index((ci, r))]} {dt}: max |out - ref64| on fractional pixels = {err:.3e}")
    assert err <= 4 * EPS
    assert f * keep.shape[1] == gen.shape[2]


@pytest.mark.parametrize("ci,r", [(1, 3), (1, 8), (2, 16), (3, 5), (0, 0)])
def test_matte_of_an_off_grid_mask(dev, ci, r):
    """Uniform random fractions: the window sums round.  Bound: two sequential fp32 sums of 2r+1 terms (each partial sum carries at most
    half an ulp of a value below the final sum, relative to the final quotient <= 1) plus the division: (2 (2r+1) + 2) * 2^-24."""
    (V, H, W, f), _, _ = CC.CASES[ci]
    keep = torch.rand(V, H // f, W // f, generator=torch.Generator().manual_seed(5 + ci))
    gen, orig = (t.to(dev) for t in operands(ci, "bf16"))
    _, matte = run(gen, orig, keep.to(dev), r)
    err = float((matte.double().cpu() - CC.matte64(keep, f, r)).abs().max())
    print(f"off-grid {(V, H, W, f)} r={r}: max |matte - w64| = {err:.3e}, bound {(2 * (2 * r + 1) + 2) * EPS:.3e}")
    assert err <= (2 * (2 * r + 1) + 2) * EPS


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("pad", [6, 8])
def test_strided_gen(dev, dt, pad):
    """A channel slice of a wider tensor with a row stride greater than W (pad 8 keeps 16-byte rows, pad 6 does not): the bits of the dense call."""
    ci, r = 1, 3
    V, H, W, f = CC.CASES[ci][0]
    gen, orig = (t.to(dev) for t in operands(ci, dt))
    keep = CC.keep_mask(ci).to(dev)
    want, wm = run(gen, orig, keep, r)
    wide = torch.full((V, 5, H, W + pad), float("nan"), dtype=gen.dtype, device=dev)
    wide[:, 1:4, :, :W] = gen
    view = wide[:, 1:4, :, :W]
    assert view.stride() == (5 * H * (W + pad), H * (W + pad), W + pad, 1) and not view.is_contiguous()
    got, gm = run(view, orig, keep, r)
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(gm), bits(wm))


@pytest.mark.parametrize("ci,r", [(1, 3), (3, 2)])
def test_misaligned_orig_and_out(dev, ci, r):
    """orig and out moved by 4 bytes (no 16-byte rows any more): the bits of the aligned call."""
    gen, orig = (t.to(dev) for t in operands(ci, "f16"))
    keep = CC.keep_mask(ci).to(dev)
    want, wm = run(gen, orig, keep, r)
    n = orig.numel()
    ob, ub, mb = (torch.zeros(n + 1, device=dev), torch.zeros(n + 1, device=dev), torch.zeros(wm.numel() + 1, device=dev))
    o2, u2, m2 = ob[1:].view(orig.shape), ub[1:].view(orig.shape), mb[1:].view(wm.shape)
    o2.copy_(orig)
    assert o2.data_ptr() % 16 == 4 and u2.data_ptr() % 16 == 4 and o2.is_contiguous()
    got, gm = run(gen, o2, keep, r, out=u2, matte_buf=m2)
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(gm), bits(wm))
    assert (L.lib().mdx_last_kernel() or b"").decode().startswith("composite_kernel")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_view_without_a_picture(dev, dt):
    """has == 0: the plain bits and a zero matte, even when the view's orig and keep rows hold NaN (they are not read); the other views are
    what they are in the call without `has`."""
    ci, r = 0, 3
    gen, orig = (t.to(dev) for t in operands(ci, dt))
    keep = CC.keep_mask(ci).to(dev)
    want, wm = run(gen, orig, keep, r)
    orig2, keep2 = orig.clone(), keep.clone()
    orig2[1], keep2[1] = float("nan"), float("nan")
    has = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev)
    got, gm = run(gen, orig2, keep2, r, has=has)
    assert torch.equal(bits(got[1]), bits(plain(gen)[1])) and not bool(gm[1].any())
    for v in (0, 2):
        assert torch.equal(bits(got[v]), bits(want[v])) and torch.equal(bits(gm[v]), bits(wm[v]))
    ones = torch.ones(3, dtype=torch.uint8, device=dev)
    all_on, _ = run(gen, orig, keep, r, has=ones)
    assert torch.equal(bits(all_on), bits(want))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_non_finite_gen(dev, dt):
    """NaN, +Inf, -Inf in gen: on a fully kept pixel the recorded pixel stands; on a regenerated pixel NaN stays NaN and +-Inf become
    1 / 0, as torch.clamp does."""
    ci, r = 1, 3
    w64 = reference_matte(ci, r)
    gen, orig = (t.to(dev).clone() for t in operands(ci, dt))
    keep = CC.keep_mask(ci).to(dev)
    kept = (w64[0] == 1).nonzero()[:3].tolist()
    regen = (w64[0] == 0).nonzero()[:3].tolist()
    vals = [float("nan"), float("inf"), float("-inf")]
    for (y, x), val in zip(kept + regen, vals + vals):
        gen[0, :, y, x] = val
    out, _ = run(gen, orig, keep, r)
    for y, x in kept:
        assert torch.equal(bits(out[0, y, x]), bits(orig[0, y, x]))
    (yn, xn), (yp, xp), (ym, xm) = regen
    assert bool(torch.isnan(out[0, yn, xn]).all()) and bool((out[0, yp, xp] == 1).all()) and bool((out[0, ym, xm] == 0).all())
    finite = torch.isfinite(gen).all(dim=1)[0]
    assert bool(torch.isfinite(out[0][finite]).all())


@pytest.mark.parametrize("ci,r,dt", [(0, 3, "bf16"), (1, 8, "f32"), (3, 5, "f16"), (2, 16, "bf16")])
def test_guard_bands_are_untouched(dev, ci, r, dt):
    """out and matte inside larger NaN-filled buffers: nothing before or after them is written."""
    gen, orig = (t.to(dev) for t in operands(ci, dt))
    keep = CC.keep_mask(ci).to(dev)
    want, wm = run(gen, orig, keep, r)
    G = 1024
    ob = torch.full((orig.numel() + 2 * G,), float("nan"), device=dev)
    mb = torch.full((wm.numel() + 2 * G,), float("nan"), device=dev)
    got, gm = run(gen, orig, keep, r, out=ob[G:-G].view(orig.shape), matte_buf=mb[G:-G].view(wm.shape))
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(gm), bits(wm))
    for buf in (ob, mb):
        assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[-G:]).all())


@pytest.mark.parametrize("dt", list(DTYPES))
def test_determinism_and_independence_of_views(dev, dt):
    """Two launches give equal bits; view v alone gives the bits it has in the batch; the call without a matte gives the same out."""
    ci, r = 2, 8
    gen, orig = (t.to(dev) for t in operands(ci, dt))
    keep = CC.keep_mask(ci).to(dev)
    a, am = run(gen, orig, keep, r)
    b, bm = run(gen, orig, keep, r)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(am), bits(bm))
    c, none = run(gen, orig, keep, r, matte=False)
    assert none is None and torch.equal(bits(c), bits(a))
    for v in range(gen.shape[0]):
        s, sm = run(gen[v:v + 1], orig[v:v + 1], keep[v:v + 1], r)
        assert torch.equal(bits(s[0]), bits(a[v])) and torch.equal(bits(sm[0]), bits(am[v]))
    f, fm = O.image_composite(gen, orig, keep, r, return_matte=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(f), bits(a)) and torch.equal(bits(fm), bits(am))


def test_program_path(dev):
    """The op through mdx_program_run gives the eager call's bits (V == 0 is a row of tests/test_composite_contract.py)."""
    ci, r = 0, 1
    gen, orig = (t.to(dev) for t in operands(ci, "bf16"))
    keep = CC.keep_mask(ci).to(dev)
    want, _ = run(gen, orig, keep, r)
    out = torch.zeros_like(want)
    prog = O.build_program([O.ImageComposite(gen, orig, keep, out, r)])
    prog.run(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want))


# ---- pipeline level: tiny nets, two scenes ----------------------------------------------------------------------------------------------

STEPS = 2


@pytest.fixture(scope="module")
def pipeline_runs(dev):
    from helpers import given_view_inputs, scene
    from magicdrive_amd.networks import spec
    from magicdrive_amd.networks.autoencoder_kl import AutoencoderKL
    from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
    from magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view import StableDiffusionBEVControlNetGivenViewPipeline
    cfg = spec.TINY_CONFIG
    vae = AutoencoderKL.from_config(spec.VAE_TINY_CONFIG, 5)
    pipe = StableDiffusionBEVControlNetGivenViewPipeline(vae=vae, unet=UNet2DConditionModelMultiview.from_config(cfg, 0),
                                                         controlnet=BEVControlNetModel.from_config(cfg, 1)).to(dev)
    sc, cl = scene(cfg, 2, 5), given_view_inputs()                # given views: (0, 0), (0, 3), (1, 5)
    g = torch.Generator().manual_seed(9)
    masks = [[None] * 6 for _ in range(2)]
    for (i, j), (y0, y1, x0, x1) in (((0, 0), (5, 12, 10, 30)), ((0, 3), (0, 6, 0, 9)), ((1, 5), (20, 28, 35, 50))):
        m = torch.ones(28, 50)
        m[max(y0 - 1, 0):y1 + 1, max(x0 - 1, 0):x1 + 1] = torch.randint(1, 64, (28, 50), generator=g)[max(y0 - 1, 0):y1 + 1, max(x0 - 1, 0):x1 + 1].float() / 64
        m[y0:y1, x0:x1] = 0.0
        masks[i][j] = m
    pics = [[None] * 6 for _ in range(2)]
    pics[0][0] = torch.randint(0, 256, (224, 400, 3), generator=g, dtype=torch.uint8)
    pics[1][5] = torch.randint(0, 256, (224, 400, 3), generator=g, dtype=torch.uint8).numpy()      # (0, 3): a given view WITHOUT a picture
    kw = dict(prompt=None, image=sc["bev_map"], camera_param=sc["camera_param"], height=224, width=400, conditional_latents=cl,
              num_inference_steps=STEPS, guidance_scale=2.0, latents=sc["latents"], prompt_embeds=sc["prompt_embeds"],
              negative_prompt_embeds=sc["negative_prompt_embeds"], bev_controlnet_kwargs={"bboxes_3d_data": sc["bboxes_3d_data"]})
    pipe.keep_masks, pipe.health = masks, "final"
    res = {}
    res["off_np"] = pipe(output_type="np", **kw)
    res["latent"] = pipe(output_type="latent", **kw).images.clone()
    ref = vae.decode((res["latent"] / 0.18215).reshape(-1, 4, 28, 50).to(next(vae.parameters()).dtype)).sample
    ref = ref.reshape(2, -1, *ref.shape[1:])
    res["parent_np"] = (ref / 2 + 0.5).clamp(0, 1).cpu().permute(0, 1, 3, 4, 2).float().numpy()
    pipe.composite_images, pipe.composite_feather = pics, 3
    res["on_np"] = pipe(output_type="np", **kw)
    res["on_pil"] = pipe(output_type="pil", **kw)
    res["on_tuple"] = pipe(output_type="np", return_dict=False, **kw)
    pipe.composite_images = None
    torch.cuda.synchronize()
    res["pics"], res["masks"] = pics, masks
    return res


def test_pipeline_switch_off_is_the_parent_path(pipeline_runs):
    r = pipeline_runs
    assert r["off_np"].matte is None
    assert r["off_np"].images.dtype == np.float32 and np.array_equal(r["off_np"].images.view(np.int32), r["parent_np"].view(np.int32))


def test_pipeline_composite(pipeline_runs):
    from magicdrive_amd.dataset import edit_matte
    r = pipeline_runs
    on, off = r["on_np"], r["off_np"]
    assert on.matte.shape == (2, 6, 224, 400) and on.matte.dtype == np.float32 and on.images.shape == off.images.shape == (2, 6, 224, 400, 3)
    assert len(r["on_tuple"]) == 2 and np.array_equal(r["on_tuple"][0], on.images) and r["on_tuple"][1] is None
    with_pic = {(0, 0), (1, 5)}
    for i in range(2):
        for j in range(6):
            if (i, j) not in with_pic:                            # a None entry: the switch-off call's view, a zero matte
                assert np.array_equal(on.images[i, j].view(np.int32), off.images[i, j].view(np.int32)) and not on.matte[i, j].any()
                continue
            w = on.matte[i, j]
            want = edit_matte(r["masks"][i][j], 8, 3).numpy()
            assert np.abs(w.astype(np.float64) - want).max() <= 2.0 ** -24
            one, zero = w == 1, w == 0
            assert one.mean() > 0.05 and zero.mean() > 0.05 and (~(one | zero)).mean() > 0.01
            rec = np.asarray(r["pics"][i][j])
            assert np.array_equal(np.asarray(r["on_pil"].images[i][j])[one], rec[one]), "a fully kept pixel is not the recorded byte"
            assert np.array_equal(on.images[i, j][one], (rec[one].astype(np.float32) / np.float32(255)))
            assert np.array_equal(on.images[i, j][zero].view(np.int32), off.images[i, j][zero].view(np.int32)), "a regenerated pixel is not the plain path's"
            band = ~(one | zero)
            lo = np.minimum(off.images[i, j], rec / 255.0)[band] - 1e-6
            hi = np.maximum(off.images[i, j], rec / 255.0)[band] + 1e-6
            assert ((on.images[i, j][band] >= lo) & (on.images[i, j][band] <= hi)).all()
    # the latents and the health records (which see the raw decoded tensor) do not know about the composite
    assert np.array_equal(on.health.final, off.health.final) and np.array_equal(on.health.image_nonfinite, off.health.image_nonfinite)
    assert on.health.ok == off.health.ok == [True, True]
