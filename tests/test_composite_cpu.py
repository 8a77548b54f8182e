"""CPU: the matte of the kept-region composite as magicdrive_amd.dataset.edit_matte states it in torch, and the pipeline's refusals.

The masks are those of the GPU cases (tests/composite_cases.py).  The three properties that make erosion + mean of one radius the right
matte are asserted on them, edit_matte is compared with a float64 evaluation that calls no pooling routine, and every refusal of
pipe.composite_images is shown to be raised on the host before the sampler's own "no CPU path" error.
"""
import numpy as np
import pytest
import torch

import composite_cases as CC
from magicdrive_amd.dataset import edit_matte


@pytest.mark.parametrize("ci,r", CC.GRID, ids=CC.GRID_IDS)
def test_matte_properties(ci, r):
    (V, H, W, f), _, _ = CC.CASES[ci]
    keep = CC.keep_mask(ci)
    w = edit_matte(keep, f, r)
    assert tuple(w.shape) == (V, H, W) and w.dtype == torch.float32
    a = keep.repeat_interleave(f, dim=1).repeat_interleave(f, dim=2)
    assert float(w.min()) >= 0.0 and float(w.max()) <= 1.0
    assert bool((w[a == 0] == 0).all()), "generated content is attenuated inside the regenerated region"
    assert bool((w <= a).all()), "the matte exceeds the keep mask somewhere: the band is not inside the kept region"
    far = CC.all_ones_within(keep, f, 2 * r)
    assert bool(far.any()) and bool((w[far] == 1).all()), "a pixel 2r away from every edit is not fully kept"
    band = (w > 0) & (w < 1)
    assert bool((a[band] > 0).all()) and not bool((band & far).any())
    z, o, m = CC.regime_shares(CC.matte64(keep, f, r))
    assert min(z, o) >= 0.05 and m >= 0.05, (z, o, m)


@pytest.mark.parametrize("ci", range(len(CC.CASES)))
def test_feather_zero_is_the_nearest_upsample(ci):
    f = CC.CASES[ci][0][3]
    keep = CC.keep_mask(ci)
    assert torch.equal(edit_matte(keep, f, 0), keep.repeat_interleave(f, dim=1).repeat_interleave(f, dim=2))
    assert torch.equal(edit_matte(keep[0], f, 0), edit_matte(keep, f, 0)[0])         # any leading shape, none included


@pytest.mark.parametrize("ci,r", CC.GRID, ids=CC.GRID_IDS)
def test_matte_agrees_with_float64(ci, r):
    """On the 1/64 grid every window sum is exact in fp32 (at most 33^2 terms of k / 64 <= 1: below 2^24 / 64), so the only rounding is the
    division: half an ulp of a value <= 1, 2^-25.  The bound asserted is the issue's 2^-24."""
    f = CC.CASES[ci][0][3]
    keep = CC.keep_mask(ci)
    w64 = CC.matte64(keep, f, r)
    err = float((edit_matte(keep, f, r).double() - w64).abs().max())
    print(f"case {CC.GRID_IDS[CC.GRID.index((ci, r))]}: max |w32 - w64| = {err:.3e}")
    assert err <= 2.0 ** -24
    assert float((edit_matte(keep.double(), f, r) - w64).abs().max()) <= 2.0 ** -50     # a float64 mask stays float64


def test_edit_matte_refuses_bad_arguments():
    k = torch.ones(2, 3)
    for bad in (dict(factor=0), dict(factor=2.0), dict(feather=-1), dict(feather=17), dict(feather=1.5), dict(feather=True)):
        kw = dict(factor=8, feather=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            edit_matte(k, **kw)
    with pytest.raises(ValueError):
        edit_matte(torch.ones(3), 8, 1)
    assert tuple(edit_matte(np.ones((2, 3), dtype=np.float32), 4, 16).shape) == (8, 12)     # a window wider than the image


class _Net:
    cfg = {"neighboring_view_pair": {i: [(i - 1) % 6, (i + 1) % 6] for i in range(6)}}

    def __init__(self):
        self._p = object()

    def packed(self):
        return self._p


def test_composite_refusals_come_before_any_device_work():
    """A pipeline that was never moved to a device: a call that passes the composite checks ends at the sampler's own "no CPU path" error;
    every refusal is a ValueError raised before that."""
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import BEVStableDiffusionPipelineOutput
    from magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view import StableDiffusionBEVControlNetGivenViewPipeline
    lat = lambda: torch.zeros(4, 28, 50)
    cl = [[lat(), None, None, lat(), None, None], [None] * 5 + [lat()]]
    masks = [[torch.full((28, 50), 0.5), None, None, None, None, None], [None] * 6]
    pic8 = lambda: torch.zeros(224, 400, 3, dtype=torch.uint8)
    ok = [[pic8(), None, None, np.zeros((224, 400, 3), dtype=np.uint8), None, None], [None] * 5 + [torch.rand(224, 400, 3)]]
    kw = dict(prompt=None, image=torch.zeros(2, 8, 200, 200), camera_param=torch.zeros(2, 6, 3, 7), height=224, width=400,
              prompt_embeds=torch.zeros(2, 77, 8), negative_prompt_embeds=torch.zeros(2, 77, 8), output_type="np")

    def call(pics, keep=masks, feather=4, **extra):
        pipe = StableDiffusionBEVControlNetGivenViewPipeline(unet=_Net(), controlnet=_Net())
        assert pipe.composite_images is None and pipe.composite_feather == 4
        pipe.keep_masks, pipe.composite_images, pipe.composite_feather = keep, pics, feather
        return pipe(conditional_latents=cl, **dict(kw, **extra))

    with pytest.raises(RuntimeError, match="no CPU path"):
        call(ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(ok, feather=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        call([[None] * 6, [None] * 6], feather=16)
    bad = lambda i, j, v: [[v if (a, b) == (i, j) else m for b, m in enumerate(r)] for a, r in enumerate(ok)]
    for pics, what in ((bad(0, 1, pic8()), r"composite_images\[0\]\[1\].*without a conditional latent"),
                       (bad(0, 0, torch.zeros(400, 224, 3, dtype=torch.uint8)), r"composite_images\[0\]\[0\].*shape"),
                       (bad(0, 0, torch.zeros(3, 224, 400)), r"composite_images\[0\]\[0\].*shape"),
                       (bad(0, 3, np.zeros((224, 400), dtype=np.uint8)), r"composite_images\[0\]\[3\].*shape"),
                       (bad(1, 5, torch.full((224, 400, 3), 1.5)), r"composite_images\[1\]\[5\].*\[0, 1\]"),
                       (bad(1, 5, torch.full((224, 400, 3), -0.01)), r"composite_images\[1\]\[5\].*\[0, 1\]"),
                       (bad(1, 5, torch.full((224, 400, 3), float("nan"))), r"composite_images\[1\]\[5\].*finite"),
                       (bad(0, 0, torch.zeros(224, 400, 3, dtype=torch.int32)), r"composite_images\[0\]\[0\].*dtype"),
                       (ok[:1], "B x N_cam"), ([ok[0][:5], ok[1]], "B x N_cam"), (ok[0], "B x N_cam")):
        with pytest.raises(ValueError, match=what):
            call(pics)
    for feather in (-1, 17, 2.5, True, None):
        with pytest.raises(ValueError, match="composite_feather"):
            call(ok, feather=feather)
    with pytest.raises(ValueError, match="without keep_masks"):
        call(ok, keep=None)
    with pytest.raises(ValueError, match="output_type='latent'"):
        call(ok, output_type="latent")
    # accepted pictures as host tensors: uint8 -> k / 255 in fp32, None -> has 0
    pipe = StableDiffusionBEVControlNetGivenViewPipeline(unet=_Net(), controlnet=_Net())
    pipe.keep_masks = masks
    ramp = (torch.arange(224 * 400 * 3) % 256).to(torch.uint8).reshape(224, 400, 3)
    pipe.composite_images = [[ramp, None, None, ramp.numpy(), None, None], [None] * 5 + [ramp.float() / 255]]
    orig, has, feather = pipe._checked_composite((cl, True), 224, 400, "pil")
    assert tuple(orig.shape) == (12, 224, 400, 3) and orig.dtype == torch.float32 and has.dtype == torch.uint8 and feather == 4
    assert has.tolist() == [1, 0, 0, 1, 0, 0] + [0] * 5 + [1]
    want = torch.from_numpy((np.arange(256, dtype=np.float64) / 255).astype(np.float32))[ramp.long()]
    assert torch.equal(orig[0], want) and torch.equal(orig[3], want) and torch.equal(orig[11], want) and not bool(orig[1].any())
    # the recorded byte survives numpy_to_pil_double's (x * 255).round().astype(uint8) for every k
    k = np.arange(256)
    assert np.array_equal((((k / 255).astype(np.float32)) * 255).round().astype("uint8"), k.astype("uint8"))
    assert BEVStableDiffusionPipelineOutput(images=None, nsfw_content_detected=None).matte is None
