"""CPU: what SamplerPlan(keep_regions=True), pipe.keep_masks and dataset.box_keep_mask do before any kernel runs (the kernel itself is
tests/test_latent_blend_gpu.py, the sampler tests/test_region_keep_gpu.py).

  keep_regions=False  the prologue and step op lists are, op for op, those of today's given-view plan;
  keep_regions=True   exactly one op more per step — an ops.LatentBlend behind the scheduler op and in front of the health trace op — and the
                      scheduler op carries no given-view fields; modes 0 and 2 refuse the switch;
  load_inputs         the first sample is m * add_noise(cond, noise, t_0) + (1 - m) * noise; whole-view masks give the given-view plan's bits;
  the plan key        unchanged with pipe.keep_masks = None, one trailing ("regions",) with it set;
  pipe.keep_masks     every refusal is a ValueError raised before the call touches a device;
  box_keep_mask       exact coverage fractions of an axis-aligned rectangle, all ones for a box outside the image, dilation, range.
"""
import numpy as np
import pytest
import torch

from helpers import cfg_inputs, given_view_inputs, scene, state_dicts
from magicdrive_amd import denoiser as DN, ops as O, schedulers
from magicdrive_amd.dataset import box_keep_mask, project_box_corners
from magicdrive_amd.engine import PackedNet
from magicdrive_amd.networks import spec
from test_health_plan_cpu import signature

CPU = torch.device("cpu")
STEPS = 3


@pytest.fixture(scope="module")
def nets():
    cfg = spec.TINY_CONFIG
    usd, csd = state_dicts(cfg)
    return cfg, PackedNet(usd, CPU), PackedNet(csd, CPU)


def plan(nets, **kw):
    cfg, un, cn = nets
    return DN.SamplerPlan(cfg, un, cn, CPU, 2, True, 3, (28, 50), num_steps=STEPS, guidance_scale=2.0, **kw)


@pytest.mark.parametrize("kw", [{}, {"scheduler_kind": "unipc"}, {"fork": True}, {"health": "trace"}, {"scheduler_kind": "unipc", "health": "trace", "dynamic_boxes": "scene"}],
                         ids=["ddim", "unipc", "fork", "trace", "unipc+trace+scene_boxes"])
def test_keep_regions_adds_one_op_behind_the_scheduler(nets, kw):
    base = plan(nets, given_view_mode=1, **kw)
    off = plan(nets, given_view_mode=1, keep_regions=False, **kw)
    assert signature(off.prologue_ops) == signature(base.prologue_ops) and signature(off.step_ops) == signature(base.step_ops)
    assert off.fork_at == base.fork_at and not off.keep_regions and not hasattr(off, "keep")

    on = plan(nets, given_view_mode=1, keep_regions=True, **kw)
    assert signature(on.prologue_ops) == signature(base.prologue_ops) and on.fork_at == base.fork_at
    assert len(on.step_ops) == len(base.step_ops) + 1
    sched = "cfg+unipc" if kw.get("scheduler_kind") == "unipc" else "cfg+ddim"
    k = [i for i, op in enumerate(on.step_ops) if isinstance(op, O.LatentBlend)]
    assert len(k) == 1
    k = k[0]
    assert on.step_ops[k - 1].name == sched and base.step_ops[k - 1].name == sched
    assert signature(on.step_ops[:k - 1]) == signature(base.step_ops[:k - 1]) and signature(on.step_ops[k + 1:]) == signature(base.step_ops[k:])
    if kw.get("health") == "trace":
        assert k == len(on.step_ops) - 2 and isinstance(on.step_ops[-1], O.GroupStats)      # the records see the blended latents
    else:
        assert k == len(on.step_ops) - 1
    # the scheduler op: its given-view fields off, everything else as in the given-view plan
    s_on, s_base = on.step_ops[k - 1], base.step_ops[k - 1]
    assert s_on.gv_mode == 0 and s_on.gv_mask is None and s_on.gv_cond is None and s_on.gv_noise is None and s_base.gv_mode == 1
    d_on, d_base = s_on.lower()[1], s_base.lower()[1]
    assert (d_on.n, d_on.cfg, d_on.guidance, d_on.xin_c, d_on.xin_ld) == (d_base.n, d_base.cfg, d_base.guidance, d_base.xin_c, d_base.xin_ld)
    assert (d_on.gv_mode, d_on.gv_mask, d_on.gv_cond, d_on.gv_noise) == (0, None, None, None)
    # the blend op: the plan's own buffers, one mask value per latent pixel, the scheduler's table columns, every step but the last
    b = on.step_ops[k]
    assert b.x.data_ptr() == on.x.data_ptr() and b.cond.data_ptr() == on.gv_cond.data_ptr() and b.noise.data_ptr() == on.gv_noise.data_ptr()
    assert b.mask.data_ptr() == on.keep.data_ptr() and tuple(on.keep.shape) == (12, 28, 50) and on.keep.dtype == torch.float32
    assert b.coef is on.coef and b.step is on.step_ctr and b.x_in.data_ptr() == on.x_in.data_ptr() and b.cfg is True
    code, d = b.lower()
    ld, ca, cs = (12, 10, 11) if sched == "cfg+unipc" else (4, 2, 3)
    assert code == 18 and (d.n, d.mask_elems, d.coef_ld, d.col_a, d.col_s, d.last_step, d.cfg, d.xin_c, d.xin_ld) == (12 * 28 * 50 * 4, 4, ld, ca, cs, STEPS - 1, 1, 4, 8)
    assert d.step_ptr == on.step_ctr.data_ptr() and d.x_in == on.x_in.data_ptr()
    if kw.get("scheduler_kind") == "unipc":                # the history buffers belong to the scheduler op alone
        assert {s_on.x_last.data_ptr(), s_on.m1.data_ptr(), s_on.m2.data_ptr()}.isdisjoint({b.x.data_ptr(), b.cond.data_ptr(), b.noise.data_ptr()})


@pytest.mark.parametrize("mode", [0, 2])
def test_keep_regions_needs_mode_1(nets, mode):
    with pytest.raises(AssertionError, match="keep_regions"):
        plan(nets, given_view_mode=mode, keep_regions=True)


@pytest.mark.parametrize("sched_kind", ["ddim", "unipc"])
def test_load_inputs_blends_the_first_sample(nets, sched_kind):
    from oracle import denoiser as D
    cfg = nets[0]
    _, csd = state_dicts(cfg)
    sc = scene(cfg, 2, 3)
    sch = schedulers.DDIMScheduler() if sched_kind == "ddim" else schedulers.UniPCMultistepScheduler()
    ts = sch.set_timesteps(STEPS)
    ts = sch.timesteps if ts is None else ts
    cam, text, bev, boxes = cfg_inputs(D, csd, sc)
    cl = given_view_inputs()
    gm = torch.tensor([[v is not None for v in r] for r in cl])
    gl = torch.zeros(2, 6, 4, 28, 50)
    for i, r in enumerate(cl):
        for j, v in enumerate(r):
            if v is not None:
                gl[i, j] = v
    lat = torch.stack([sc["latents"]] * 6, 1)
    coef = sch.coefficient_table()
    gv = plan(nets, given_view_mode=1, scheduler_kind=sched_kind)
    gv.load_inputs(lat, cam, text, bev, boxes, ts, coef, given_mask=gm, given_latents=gl)
    on = plan(nets, given_view_mode=1, keep_regions=True, scheduler_kind=sched_kind)
    whole = gm.float().view(2, 6, 1, 1).expand(2, 6, 28, 50)
    on.load_inputs(lat, cam, text, bev, boxes, ts, coef, given_mask=gm, given_latents=gl, keep_mask=whole)
    assert torch.equal(on.x, gv.x) and torch.equal(on.x_in, gv.x_in) and torch.equal(on.keep, whole.reshape(12, 28, 50))
    assert torch.equal(on.gv_cond, gv.gv_cond) and torch.equal(on.gv_noise, gv.gv_noise)
    # fractions: m t0 + (1 - m) noise, t0 = the given-view plan's first sample of a given view
    m = whole * torch.rand(2, 6, 28, 50, generator=torch.Generator().manual_seed(1))
    m[0, 0, :4] = 1.0; m[0, 0, 4:8] = 0.0
    on.load_inputs(lat, cam, text, bev, boxes, ts, coef, given_mask=gm, given_latents=gl, keep_mask=m)
    mm = m.reshape(12, 28, 50, 1)
    noise = gv.gv_noise
    t0 = torch.where(gm.view(12, 1, 1, 1), gv.x, noise)
    want = mm * t0 + (1 - mm) * noise
    assert torch.allclose(on.x, want, rtol=0, atol=1e-6)
    assert torch.equal(on.x[0, :4], gv.x[0, :4]) and torch.equal(on.x[0, 4:8], noise[0, 4:8])          # exact 1 and exact 0: the terms themselves
    assert torch.equal(on.x.view(2, 6, 28, 50, 4)[~gm], noise.view(2, 6, 28, 50, 4)[~gm])
    with pytest.raises(AssertionError):
        on.load_inputs(lat, cam, text, bev, boxes, ts, coef, given_mask=gm, given_latents=gl)              # a regions plan needs its mask
    with pytest.raises(AssertionError):
        gv.load_inputs(lat, cam, text, bev, boxes, ts, coef, given_mask=gm, given_latents=gl, keep_mask=m)


class _Net:
    cfg = {"neighboring_view_pair": {i: [(i - 1) % 6, (i + 1) % 6] for i in range(6)}}

    def __init__(self):
        self._p = object()

    def packed(self):
        return self._p


def test_plan_key_is_unchanged_without_masks():
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    pipe = StableDiffusionBEVControlNetPipeline(unet=_Net(), controlnet=_Net())
    assert pipe.keep_masks is None
    args = (3, 0, True, 5, 28, 50, 4, 2, 1, 77, "ddim", 1, torch.bfloat16, True)
    today = (3, 0, True, 5, 28, 50, 4, 2.0, 1.0, 77, "ddim", 1, torch.bfloat16, id(pipe.unet.packed()), id(pipe.controlnet.packed()), True)
    assert pipe._plan_key(*args) == today and pipe._plan_key(*args, None, regions=False) == today
    assert pipe._plan_key(*args, regions=True) == today + (("regions",),)
    assert pipe._plan_key(*args, "trace", regions=True) == today + (("health", "trace"), ("regions",))


def test_keep_masks_refusals_come_before_any_device_work():
    """A pipeline that was never moved to a device: a call that passes the mask checks ends at the sampler's own "no CPU path" error; every
    refusal of the masks is a ValueError raised before that."""
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    from magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view import StableDiffusionBEVControlNetGivenViewPipeline
    lat = lambda: torch.zeros(4, 28, 50)
    cl = [[lat(), None, None, lat(), None, None], [None] * 5 + [lat()]]
    ok = [[torch.full((28, 50), 0.5), None, None, None, None, None], [None] * 5 + [torch.ones(28, 50)]]
    kw = dict(prompt=None, image=torch.zeros(2, 8, 200, 200), camera_param=torch.zeros(2, 6, 3, 7), height=224, width=400,
              prompt_embeds=torch.zeros(2, 77, 8), negative_prompt_embeds=torch.zeros(2, 77, 8), output_type="latent")

    def call(masks, cond=cl, **extra):
        pipe = StableDiffusionBEVControlNetGivenViewPipeline(unet=_Net(), controlnet=_Net())
        pipe.keep_masks = masks
        return pipe(conditional_latents=cond, **dict(kw, **extra))

    with pytest.raises(RuntimeError, match="no CPU path"):
        call(ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(None)
    bad = lambda i, j, v: [[v if (a, b) == (i, j) else m for b, m in enumerate(r)] for a, r in enumerate(ok)]
    for masks, what in ((bad(0, 1, torch.ones(28, 50)), r"keep_masks\[0\]\[1\].*without a conditional latent"),
                        (bad(0, 0, torch.ones(50, 28)), r"keep_masks\[0\]\[0\].*shape"),
                        (bad(0, 0, torch.ones(1, 28, 50)), r"keep_masks\[0\]\[0\].*shape"),
                        (bad(1, 5, torch.full((28, 50), 1.5)), r"keep_masks\[1\]\[5\].*\[0, 1\]"),
                        (bad(1, 5, torch.full((28, 50), -0.01)), r"keep_masks\[1\]\[5\].*\[0, 1\]"),
                        (bad(0, 0, torch.full((28, 50), float("nan"))), r"keep_masks\[0\]\[0\].*finite"),
                        (bad(0, 0, torch.full((28, 50), float("inf"))), r"keep_masks\[0\]\[0\].*finite"),
                        (ok[:1], "B x N_cam"), ([ok[0][:5], ok[1]], "B x N_cam")):
        with pytest.raises(ValueError, match=what):
            call(masks)
    with pytest.raises(ValueError, match="conditional_latents_change_every_input=True"):
        call(ok, conditional_latents_change_every_input=False)
    plain = StableDiffusionBEVControlNetPipeline(unet=_Net(), controlnet=_Net())
    plain.keep_masks = ok
    with pytest.raises(ValueError, match="no given views"):
        plain(**kw)
    # accepted masks as one host tensor: None on a given view -> ones, a view without a latent -> zeros
    pipe = StableDiffusionBEVControlNetGivenViewPipeline(unet=_Net(), controlnet=_Net())
    pipe.keep_masks = ok
    m = pipe._checked_keep_masks((cl, True), 224, 400)
    assert tuple(m.shape) == (2, 6, 28, 50) and m.dtype == torch.float32 and m.device.type == "cpu"
    assert (m[0, 0] == 0.5).all() and (m[0, 3] == 1).all() and (m[1, 5] == 1).all() and (m[0, 1] == 0).all() and m.sum() == 28 * 50 * 2.5


def _rect(x0, y0, x1, y1):
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


def _coverage_of_rect(r, H, W, f):
    """Exact: the fraction of the f x f image pixels of every latent pixel whose centre lies inside the rectangle."""
    x0, y0, x1, y1 = r
    cx, cy = np.arange(W) + 0.5, np.arange(H) + 0.5
    img = np.outer((cy >= y0) & (cy <= y1), (cx >= x0) & (cx <= x1)).astype(np.float64)
    return img.reshape(H // f, f, W // f, f).mean(axis=(1, 3))


def test_box_keep_mask_rectangles_are_exact():
    H, W, f = 48, 80, 8
    one = torch.ones(1, 1, dtype=torch.bool)
    for r in ((12, 4, 28, 20), (12.3, 4.2, 27.6, 19.7), (12.6, 4.6, 27.4, 19.4), (8, 8, 16, 16), (0, 0, 80, 48), (-50, -50, 20, 20), (70.2, 41.5, 500, 400),
              (33, 9, 34, 30), (12.6, 3, 12.9, 40)):
        m = box_keep_mask(torch.tensor([[_rect(*r)]], dtype=torch.float32), one, (H, W), (H // f, W // f), dilate=0)
        assert tuple(m.shape) == (1, 6, 10) and m.dtype == torch.float32
        assert np.array_equal(m[0].double().numpy(), 1.0 - _coverage_of_rect(r, H, W, f)), r
    # the hand-checked case: [12, 28] x [4, 20] covers half of latent columns 1 and 3 and of latent rows 0 and 2, all of column 2 / row 1
    m = box_keep_mask(torch.tensor([[_rect(12, 4, 28, 20)]], dtype=torch.float32), one, (H, W), (6, 10), dilate=0)
    want = torch.ones(6, 10)
    want[:3, 1:4] = 1 - torch.tensor([[0.25, 0.5, 0.25], [0.5, 1.0, 0.5], [0.25, 0.5, 0.25]])
    assert torch.equal(m[0], want)
    # a union, a box that is not kept, points that are not finite, a second view without boxes
    c = torch.full((2, 3, 6, 2), float("nan"))
    c[0, 0, :4] = torch.tensor(_rect(0, 0, 16, 8), dtype=torch.float32)
    c[0, 1, :4] = torch.tensor(_rect(8, 0, 24, 16), dtype=torch.float32)
    c[0, 2, :4] = torch.tensor(_rect(40, 24, 80, 48), dtype=torch.float32)
    kept = torch.tensor([[True, True, False], [False, False, False]])
    m = box_keep_mask(c, kept, (H, W), (6, 10), dilate=0)
    want = torch.ones(6, 10); want[0, :3] = 0; want[1, 1:3] = 0
    assert torch.equal(m[0], want) and torch.equal(m[1], torch.ones(6, 10))


def test_box_keep_mask_outside_dilate_and_range():
    H, W = 48, 80
    one = torch.ones(1, 1, dtype=torch.bool)
    for r in ((-40, -40, -1, -1), (81, 5, 120, 30), (10, 49, 30, 90), (-1e7, 60, 1e7, 70)):
        for dilate in (0, 1, 3):
            assert torch.equal(box_keep_mask(torch.tensor([[_rect(*r)]], dtype=torch.float32), one, (H, W), (6, 10), dilate=dilate), torch.ones(1, 6, 10)), r
    c = torch.tensor([[_rect(32, 16, 48, 32)]], dtype=torch.float32)                      # latent pixels [2:4, 4:6], fully covered
    for dilate in (0, 1, 2):
        m = box_keep_mask(c, one, (H, W), (6, 10), dilate=dilate)
        want = torch.ones(6, 10)
        want[max(2 - dilate, 0):4 + dilate, max(4 - dilate, 0):6 + dilate] = 0
        assert torch.equal(m[0], want), dilate
    assert torch.equal(box_keep_mask(c, one, (H, W), (6, 10)), box_keep_mask(c, one, (H, W), (6, 10), dilate=1))       # the default
    # fractions are dilated by their maximum; the result stays in [0, 1]
    g = torch.Generator().manual_seed(0)
    pts = torch.rand(3, 5, 8, 2, generator=g) * torch.tensor([120.0, 80.0]) - 20.0
    m = box_keep_mask(pts, torch.rand(3, 5, generator=g) > 0.2, (H, W), (6, 10), dilate=1)
    m0 = box_keep_mask(pts, torch.ones(3, 5, dtype=torch.bool), (H, W), (6, 10), dilate=0)
    assert tuple(m.shape) == (3, 6, 10) and bool(((m >= 0) & (m <= 1)).all()) and bool(((m0 >= 0) & (m0 <= 1)).all())
    assert bool(((m0 > 0) & (m0 < 1)).any())                                              # slanted hulls: fractions occur
    frac = box_keep_mask(torch.tensor([[_rect(36, 20, 44, 28)]], dtype=torch.float32), one, (H, W), (6, 10), dilate=1)   # a quarter of 4 latent pixels
    assert torch.equal(frac[0, 1:5, 3:7], torch.full((4, 4), 0.75)) and frac.sum() == 60 - 16 * 0.25
    with pytest.raises(AssertionError):
        box_keep_mask(c, one, (50, 80), (6, 10))


def test_project_box_corners_drops_what_is_behind_the_camera():
    """A camera at the origin looking along +z (identity lidar2camera): a box in front projects through K, a box behind is not kept, a
    box that straddles the camera plane is clipped at the near plane and yields finite points only."""
    K = torch.eye(4); K[0, 0] = K[1, 1] = 100.0; K[0, 2], K[1, 2] = 40.0, 24.0
    l2i = K.unsqueeze(0)
    aug = torch.eye(4).unsqueeze(0)
    boxes = torch.tensor([[0.0, 0.0, 10.0, 2.0, 2.0, 2.0, 0.0],          # centre of the bottom face at depth 10: z in [10, 12]
                          [0.0, 0.0, -10.0, 2.0, 2.0, 2.0, 0.0],         # behind
                          [0.0, 0.0, -1.0, 2.0, 2.0, 2.0, 0.0]])         # z in [-1, 1]: straddles
    c, kept = project_box_corners(boxes, l2i, aug)
    assert tuple(c.shape) == (1, 3, 20, 2) and kept.tolist() == [[True, False, True]]
    assert torch.isfinite(c[0, 0, :8]).all() and torch.isnan(c[0, 0, 8:]).all() and torch.isnan(c[0, 1]).all()
    near_x = 40.0 + 100.0 * torch.tensor([-1.0, 1.0]) / 10.0
    assert torch.allclose(c[0, 0, :8, 0].min(), near_x[0]) and torch.allclose(c[0, 0, :8, 0].max(), near_x[1])
    fin = torch.isfinite(c[0, 2]).all(dim=1)
    assert int(fin[:8].sum()) == 4 and int(fin[8:].sum()) == 4                          # 4 corners in front, 4 edges cross the near plane
    m = box_keep_mask(c, kept, (48, 80), (6, 10), dilate=0)
    assert float(m[0].min()) == 0.0 and bool((m[0, 2:4, 4:6] == 0).all())               # the image centre is covered by both kept boxes
    e, k = project_box_corners(torch.zeros(0, 7), l2i, aug)
    assert tuple(e.shape) == (1, 0, 20, 2) and tuple(k.shape) == (1, 0)
    assert torch.equal(box_keep_mask(e, k, (48, 80), (6, 10)), torch.ones(1, 6, 10))
