"""Upsample2D's 3x3 conv folded over its 2x nearest resize (packing.fold_upsample_conv, MdxConvDesc.upsample2x), checked without a GPU:
the fold identity to fp32 round-off, the index-map rule that admits it, plan parity of the folded plans in the torch interpreter against
the default (resize + conv) plans of the same weights, and the FLOP accounting."""
import os

import pytest
import torch
import torch.nn.functional as F

import plan_interp
from helpers import rel_l2
from magicdrive_amd import denoiser as DN, flops, ops as O, packing as PK
from magicdrive_amd.engine import Builder, PackedNet, upsample_conv_folds
from magicdrive_amd.networks import spec
from magicdrive_amd.vae import VaeDecodePlan

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CPU = torch.device("cpu")

# (low-res size) -> (output size): the UNet decoder's three stages at 224x400, the VAE decoder's / hires sizes, and a size cropped on H only
# ((7, 13) -> (14, 25) is cropped on W only, (4, 7) -> (7, 13) on both axes)
SIZES = [((4, 7), (7, 13)), ((7, 13), (14, 25)), ((14, 25), (28, 50)), ((28, 50), (56, 100)), ((54, 96), (108, 192)), ((6, 9), (11, 18))]


def rel_max(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("lo,hi", SIZES)
def test_fold_identity(lo, hi):
    """Sum of the phase convs on the low-res input == conv3x3(pad 1) of the nearest-resized input, to round-off: rel <= 1e-5 in fp32 (the
    fp64 evaluation of the same F.conv2d is the yardstick: F.conv2d in fp32 against it stays inside the same bound) and 1e-12 in fp64."""
    g = torch.Generator().manual_seed(lo[0] * 1000 + lo[1])
    B, Cin, Cout = 2, 8, 6
    x = torch.randn(B, Cin, *lo, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64) * (9 * Cin) ** -0.5
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    ref64 = F.conv2d(F.interpolate(x, size=hi, mode="nearest"), w, b, padding=1)
    crop = (hi[0] != 2 * lo[0], hi[1] != 2 * lo[1])
    wf64 = PK.fold_upsample_conv(w, *crop, dtype=None)
    assert wf64.shape == ((2 + crop[0]) * (2 + crop[1]), Cout, 2, 2, Cin)
    got64 = PK.folded_upsample_conv_reference(x, wf64, *hi, bias=b)
    e64 = rel_max(got64, ref64)
    ref32 = F.conv2d(F.interpolate(x.float(), size=hi, mode="nearest"), w.float(), b.float(), padding=1)
    got32 = PK.folded_upsample_conv_reference(x.float(), PK.fold_upsample_conv(w.float(), *crop, dtype=None), *hi, bias=b.float())
    e32, e32_self = rel_max(got32.double(), ref64), rel_max(ref32.double(), ref64)
    print(f"[fold identity {lo}->{hi}] fp64 {e64:.2e}  fp32 {e32:.2e}  (F.conv2d fp32 vs fp64 {e32_self:.2e})")
    assert e64 <= 1e-12, e64
    assert e32_self <= 1e-5 and e32 <= 1e-5, (e32, e32_self)


@pytest.mark.parametrize("lo,hi", SIZES)
def test_nearest_map_is_shift(lo, hi):
    for n, n_out in zip(lo, hi):
        assert torch.equal(PK.nearest_index(n, n_out), torch.arange(n_out, dtype=torch.int32) >> 1)
        assert PK.upsample_fold_ok(n, n_out)
    assert upsample_conv_folds(CPU, True, *lo, *hi, 64)
    assert not upsample_conv_folds(CPU, None, *lo, *hi, 64)          # CPU plans keep the pair unless forced
    assert not upsample_conv_folds(CPU, True, *lo, *hi, 32)          # the XL route needs whole 64-channel blocks
    # on GPU devices the decision does not depend on the batch: a 1-scene and a 96-scene plan run the same weights
    cuda = torch.device("cuda")
    assert upsample_conv_folds(cuda, None, *lo, *hi, 1280, B=576) and upsample_conv_folds(cuda, None, *lo, *hi, 1280, B=6)
    if hi[0] != 2 * lo[0] or hi[1] != 2 * lo[1]:                       # cropped axis: X must fit the kernel's 2 GiB window
        assert not upsample_conv_folds(cuda, True, *lo, *hi, 64, B=(1 << 31) // (lo[0] * lo[1] * 128) + 1)


def test_other_maps_keep_the_pair():
    """A resize whose map is not o >> 1 (any size but 2 n / 2 n - 1) is never folded."""
    for n, n_out in ((5, 8), (4, 9), (7, 12), (3, 3)):
        assert not PK.upsample_fold_ok(n, n_out)
        assert not upsample_conv_folds(CPU, True, n, n, n_out, n_out, 64)


def run_folded_conv(op):
    """Torch evaluation of O.Conv(upsample2x=True) for this file's interpreter runs: the phase convs, fp32 accumulation, one rounding."""
    y = PK.folded_upsample_conv_reference(op.X.float().permute(0, 3, 1, 2), op.Wt.float(), op.Y.shape[1], op.Y.shape[2],
                                          None if op.bias is None else op.bias.float())
    op.Y.copy_(y.permute(0, 2, 3, 1).to(op.Y.dtype))


@pytest.fixture
def folded_interp(monkeypatch):
    plain = plan_interp.DISPATCH[O.Conv]
    monkeypatch.setitem(plan_interp.DISPATCH, O.Conv, lambda op: run_folded_conv(op) if op.upsample2x else plain(op))


def _unet_plans():
    cfg = spec.TINY_CONFIG
    usd = spec.random_state_dict(spec.unet_param_shapes(cfg), 0)
    plans = []
    for fold in (None, True):
        Builder.fold_upsample = fold
        try:
            plans.append(DN.UNetPlan(cfg, PackedNet(usd, CPU), CPU, 6, 8, (28, 50)))
        finally:
            Builder.fold_upsample = None
    return plans


def test_unet_plan_parity(folded_interp):
    """The tiny UNet plan with the fold forced on the CPU device against the default plan of the same weights and inputs.  The two differ by
    one 16-bit rounding of the folded weights (and the accumulation order); the limit is the one tests/test_plan_cpu.py holds the same
    plans to against the reference's goldens (3e-2 per view)."""
    base, fold = _unet_plans()
    names = lambda p: [type(op).__name__ for op in p.ops]
    ups_b = [op for op in base.ops if isinstance(op, O.Upsample)]
    assert len(ups_b) == 3 and not any(getattr(op, "upsample2x", False) for op in base.ops)          # default CPU plan: unchanged op set
    fc = [op for op in fold.ops if getattr(op, "upsample2x", False)]
    assert len(fc) == 3 and not any(isinstance(op, O.Upsample) for op in fold.ops) and len(fold.ops) == len(base.ops) - 3
    assert [tuple(op.Wt.shape[:1]) for op in fc] == [(9,), (6,), (4,)]          # (4,7)->(7,13): both axes cropped, (7,13)->(14,25): W, (14,25)->(28,50): none
    assert set(names(fold)) <= set(names(base))
    g = torch.Generator().manual_seed(5)
    for p in (base, fold):
        g.manual_seed(5)
        p.sample_nchw.copy_(torch.randn(p.sample_nchw.shape, generator=g))
        p.temb.t.copy_(torch.full(p.temb.t.shape, 500.0))
        p.ctx.copy_(torch.randn(p.ctx.shape, generator=g))
        for dst in p.res_in:
            dst.copy_(torch.randn(dst.shape, generator=g) * 0.1)
        p.mid_in.copy_(torch.randn(p.mid_in.shape, generator=g) * 0.1)
        plan_interp.run(p.ops)
    per_view = max(rel_l2(fold.out_nchw[i], base.out_nchw[i]) for i in range(6))
    print(f"[folded vs unfused tiny UNet plan] worst view rel L2 {per_view:.3e}")
    assert per_view < 3e-2, per_view
    # same algorithmic work, three ops fewer
    assert flops.program_flops(fold.ops)["total"] == flops.program_flops(base.ops)["total"]
    assert all(flops.op_flops(op) == 2.0 * op.Y.shape[0] * op.Y.shape[1] * op.Y.shape[2] * op.Y.shape[3] * 9 * op.X.shape[3] for op in fc)


def test_vae_decode_plan_parity(folded_interp):
    """The tiny VAE decode plan with the fold forced: against diffusers' golden image at the limit of tests/test_plan_cpu.py (3e-2) and against
    the default plan.  Its upsamplers have 64, 64 and 32 channels: the first two fold, the third keeps the pair (Cin % 64)."""
    G = torch.load(os.path.join(GOLD, "tiny_vae_decode.pt"))
    vcfg = spec.VAE_TINY_CONFIG
    sd = spec.random_state_dict(spec.vae_decoder_param_shapes(vcfg), G["weights_seed"])
    z = torch.randn(2, 4, 7, 13, generator=torch.Generator().manual_seed(G["z_seed"]))
    imgs = []
    for fold in (None, True):
        VaeDecodePlan.fold_upsample = fold
        try:
            plan = VaeDecodePlan(vcfg, PackedNet(sd, CPU), CPU, 2, (7, 13))
        finally:
            VaeDecodePlan.fold_upsample = None
        nf = sum(1 for op in plan.ops if getattr(op, "upsample2x", False))
        nu = sum(1 for op in plan.ops if isinstance(op, O.Upsample))
        assert (nf, nu) == ((2, 1) if fold else (0, 3))
        plan.z_in.copy_(z)
        plan_interp.run(plan.ops)
        imgs.append(plan.out_nhwc.permute(0, 3, 1, 2).clone())
        total = flops.program_flops(plan.ops)["total"]
        imgs.append(total)
    (img0, f0, img1, f1) = imgs
    e_gold, e_pair = rel_l2(img1, G["image"].float()), rel_l2(img1, img0)
    print(f"[folded tiny VAE decode plan] vs golden {e_gold:.3e}  vs unfused plan {e_pair:.3e}")
    assert e_gold < 3e-2 and e_pair < 3e-2, (e_gold, e_pair)
    assert f0 == f1


def test_step_program_flops_unchanged_by_the_fold():
    """flops.program_flops of the SD-1.5 step program: folded == unfolded (the folded conv reports the 9-tap count of what it replaces)."""
    cfg = spec.SD15_CONFIG
    z = lambda shapes: {k: torch.zeros(1).expand(s) for k, s in shapes.items()}      # shape-only weights

    class ShapeNet(PackedNet):
        def _get(self, tag, keys, fn):
            ck = (tag,) + tuple(keys)
            if ck not in self.cache:
                self.cache[ck] = fn(*[torch.zeros(self.sd[k].shape) for k in keys])
            return self.cache[ck]

    totals, counts = [], []
    for fold in (None, True):
        Builder.fold_upsample = fold
        try:
            un = ShapeNet(z(spec.unet_param_shapes(cfg)), CPU); cn = ShapeNet(z(spec.controlnet_param_shapes(cfg)), CPU)
            sp = DN.SamplerPlan(cfg, un, cn, CPU, 1, False, 32, (28, 50), num_steps=50)
        finally:
            Builder.fold_upsample = None
        totals.append(flops.program_flops(sp.step_ops)["total"])
        counts.append(len(sp.step_ops))
        for op in sp.step_ops:
            op.lower()
    assert totals[0] == totals[1] and abs(totals[0] / 1e12 - 2.298) < 0.01, totals
    assert counts[1] == counts[0] - 3, counts
