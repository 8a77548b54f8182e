"""-m gpu: pipe.keep_masks / SamplerPlan(keep_regions=True) on the tiny nets — 2 scenes, 4 steps, CFG on, DDIM and UniPC, bf16 and fp16.

The kernel's numerics are judged by tests/test_latent_blend_gpu.py; here the sampler around it:
  - masks that are whole views of 0 / 1 give latents bit-identical to the existing given-view call with the same conditional_latents (a view
    with a latent and a mask of zeros = that view not given);
  - fractional masks: a twin plan built WITHOUT regions replays its step, then ops.LatentBlend is launched eagerly on the twin's buffers —
    the region plan (one captured graph per step) and the twin agree bit for bit after every step: placement behind the scheduler op, the
    counter row, the x_in refresh, the CFG halves;
  - through a callback, pixels with m == 1 hold add_noise(cond, noise, t_next) after every step but the last;
  - keep_masks = None gives the bits and the plan keys of today's call;
  - two scene chunks on two streams: the bits of each scene's own call, and the one-chunk call up to the rounding of its other batch shape;
  - health="trace" records the blended latents and changes no bit; use_graph=False gives the graph's bits; under box_bucket and under
    scene_boxes whole-view masks are still that switch's own given-view call.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import cfg_inputs, check, given_view_inputs, rel_l2, scene, state_dicts  # noqa: E402
from magicdrive_amd import denoiser as DN, ops as O, schedulers  # noqa: E402
from magicdrive_amd.engine import PackedNet  # noqa: E402
from magicdrive_amd.networks import spec  # noqa: E402

STEPS = 4
CASES = ["ddim-bf16", "unipc-bf16", "ddim-f16", "unipc-f16"]
_PIPES = {}


def get_pipe(dev, case):
    """One pipeline per (scheduler, 16-bit type), shared by the tests of this file; every test leaves its switches as it found them."""
    if case not in _PIPES:
        from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
        from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
        from magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view import StableDiffusionBEVControlNetGivenViewPipeline
        sched, dt = case.split("-")
        kw = {"torch_dtype": torch.float16} if dt == "f16" else {}
        cfg = spec.TINY_CONFIG
        pipe = StableDiffusionBEVControlNetGivenViewPipeline(unet=UNet2DConditionModelMultiview.from_config(cfg, 0, **kw),
                                                             controlnet=BEVControlNetModel.from_config(cfg, 1, **kw)).to(dev)
        if sched == "unipc":
            pipe.scheduler = schedulers.UniPCMultistepScheduler.from_config(pipe.scheduler.config)
        _PIPES[case] = pipe
    return _PIPES[case]


def inputs(case, n=2, L=5):
    sc = scene(spec.TINY_CONFIG, n, L)
    if case.endswith("f16"):
        sc["prompt_embeds"], sc["negative_prompt_embeds"] = sc["prompt_embeds"].half(), sc["negative_prompt_embeds"].half()
    return sc


def one_scene(sc, i):
    out = {k: (v[i:i + 1] if isinstance(v, torch.Tensor) else v) for k, v in sc.items()}
    if sc.get("bboxes_3d_data") is not None:
        out["bboxes_3d_data"] = {k: v[i:i + 1] for k, v in sc["bboxes_3d_data"].items()}
    return out


def call(pipe, sc, cl, **kw):
    out = pipe(prompt=None, image=sc["bev_map"], camera_param=sc["camera_param"], height=224, width=400, conditional_latents=cl,
               num_inference_steps=STEPS, guidance_scale=2.0, latents=sc["latents"], prompt_embeds=sc["prompt_embeds"],
               negative_prompt_embeds=sc["negative_prompt_embeds"], output_type="latent", bev_controlnet_kwargs={"bboxes_3d_data": sc["bboxes_3d_data"]}, **kw)
    torch.cuda.synchronize()
    return out


def fractional_masks(cl, seed=5):
    """One (28, 50) mask per given view: a block of exact ones, a block of exact zeros, fractions elsewhere; None on views that are not given."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for r in cl:
        row = []
        for v in r:
            if v is None:
                row.append(None)
                continue
            m = torch.rand(28, 50, generator=g)
            m[:9, :20] = 1.0
            m[12:20, 25:] = 0.0
            row.append(m)
        out.append(row)
    return out


@pytest.mark.parametrize("case", CASES)
def test_whole_view_masks_are_the_given_view_call(dev, case):
    pipe = get_pipe(dev, case)
    sc, cl = inputs(case), given_view_inputs()
    assert pipe.keep_masks is None
    pipe._plans.clear()
    want = call(pipe, sc, cl).images.clone()
    n_plans = len(pipe._plans)
    try:
        pipe.keep_masks = [[None if v is None else torch.ones(28, 50) for v in r] for r in cl]
        ones = call(pipe, sc, cl).images.clone()
        pipe.keep_masks = [[None] * 6, [None] * 6]                          # None on a given view: the whole view
        nones = call(pipe, sc, cl).images.clone()
        # a latent under a mask of zeros is a view that is not given
        cl_more = [list(r) for r in cl]
        cl_more[1][2] = torch.randn(4, 28, 50, generator=torch.Generator().manual_seed(3))
        pipe.keep_masks = [[None] * 6, [None, None, torch.zeros(28, 50), None, None, None]]
        zeros = call(pipe, sc, cl_more).images.clone()
    finally:
        pipe.keep_masks = None
    assert len(pipe._plans) == n_plans + 1, "one region plan serves every mask"
    assert torch.equal(ones, want), f"{case}: whole-view masks of ones differ from the given-view call"
    assert torch.equal(nones, want) and torch.equal(zeros, want)
    assert torch.equal(call(pipe, sc, cl).images, want) and len(pipe._plans) == n_plans + 1


@pytest.mark.parametrize("case", CASES)
def test_fractional_masks_against_a_twin_without_regions(dev, case):
    from oracle import denoiser as D
    sched_kind, dt = case.split("-")
    dtype = torch.float16 if dt == "f16" else torch.bfloat16
    cfg = spec.TINY_CONFIG
    usd, csd = state_dicts(cfg)
    un, cn = PackedNet(usd, dev, dtype), PackedNet(csd, dev, dtype)
    mk = lambda **kw: DN.SamplerPlan(cfg, un, cn, dev, 2, True, 5, (28, 50), num_steps=STEPS, guidance_scale=2.0, scheduler_kind=sched_kind, **kw)
    sc = scene(cfg, 2, 5)
    sch = schedulers.DDIMScheduler() if sched_kind == "ddim" else schedulers.UniPCMultistepScheduler()
    sch.set_timesteps(STEPS)
    cam, text, bev, boxes = cfg_inputs(D, csd, sc)
    cl = given_view_inputs()
    gm = torch.tensor([[v is not None for v in r] for r in cl])
    gl = torch.stack([torch.stack([torch.zeros(4, 28, 50) if v is None else v for v in r]) for r in cl])
    keep = torch.stack([torch.stack([torch.zeros(28, 50) if m is None else m for m in r]) for r in fractional_masks(cl)])
    lat = torch.stack([sc["latents"]] * 6, 1)
    region, twin = mk(given_view_mode=1, keep_regions=True), mk()
    region.compile(); twin.compile()
    assert len(region.step_ops) == len(twin.step_ops) + 1
    region.load_inputs(lat, cam, text, bev, boxes, sch.timesteps, sch.coefficient_table(), given_mask=gm, given_latents=gl, keep_mask=keep)
    twin.load_inputs(lat, cam, text, bev, boxes, sch.timesteps, sch.coefficient_table())
    twin.x.copy_(region.x); twin.x_in.copy_(region.x_in)                   # the blended first sample
    blend = O.LatentBlend(twin.x.view(-1), region.gv_cond.view(-1), region.gv_noise.view(-1), region.keep.view(-1), twin.coef, twin.step_ctr,
                          last_step=STEPS - 1, x_in=twin.x_in.view(-1, twin.x_in.shape[-1]), cfg=True, xin_c=4)
    assert O.dtype_code(blend) == O.dtype_code(region.step_ops[-1])
    st = DN.device_stream(dev)
    region.prologue.run(st); twin.prologue.run(st)
    m = region.keep.unsqueeze(-1).expand_as(region.x)
    for s in range(STEPS):
        region.step.launch(st)                                             # captured: scheduler op + blend op inside one graph
        twin.step.launch(st)
        unblended = twin.x.clone()
        O.run_ops([blend])
        torch.cuda.synchronize()
        assert int(region.step_ctr.item()) == int(twin.step_ctr.item()) == s + 1
        assert torch.equal(region.x.view(torch.int32), twin.x.view(torch.int32)), f"{case}: latents differ after step {s}"
        assert torch.equal(region.x_in.view(torch.int16), twin.x_in.view(torch.int16)), f"{case}: x_in differs after step {s}"
        assert torch.equal(region.eps, twin.eps)
        if s < STEPS - 1:
            assert torch.equal(twin.x[m == 0], unblended[m == 0]) and not torch.equal(twin.x[m == 1], unblended[m == 1])
        else:
            assert torch.equal(twin.x, unblended), "the last step's output stays the scheduler's"
        if sched_kind == "unipc":
            assert torch.equal(region.x_last, twin.x_last) and torch.equal(region.m1, twin.m1) and torch.equal(region.m2, twin.m2)
    assert torch.isfinite(region.x).all()
    region.release(); twin.release()


@pytest.mark.parametrize("case", ["ddim-bf16", "unipc-f16"])
def test_callback_sees_the_renoised_known_pixels(dev, case):
    pipe = get_pipe(dev, case)
    sc, cl = inputs(case), given_view_inputs()
    masks = fractional_masks(cl)
    seen = []
    try:
        pipe.keep_masks = masks
        out = call(pipe, sc, cl, callback=lambda i, t, lat: seen.append((i, int(t), lat.float().cpu().clone())))
        graphed = out.images.clone()
        pipe.use_graph = False
        eager = call(pipe, sc, cl).images.clone()
    finally:
        pipe.keep_masks, pipe.use_graph = None, True
    assert [i for i, _, _ in seen] == list(range(STEPS))
    assert torch.equal(graphed, eager), "use_graph=False must give the captured graph's bits"
    coef = pipe.scheduler.coefficient_table().float()
    ca, cs = (2, 3) if case.startswith("ddim") else (10, 11)
    noise = torch.stack([sc["latents"]] * 6, 1).float()                                   # the same initial noise for every view
    ts = [t for _, t, _ in seen]
    for i, t, lat in seen:
        for b, r in enumerate(cl):
            for v, c in enumerate(r):
                if c is None:
                    continue
                one = (masks[b][v] == 1).expand(4, 28, 50)
                assert one.any()
                if i < STEPS - 1:
                    want = coef[i, ca] * c.float() + coef[i, cs] * noise[b, v]
                    got = lat[b, v]
                    if lat.dtype == torch.float32 and sc["prompt_embeds"].dtype == torch.float32:
                        assert torch.equal(got[one], want[one]), f"step {i} view ({b}, {v})"
                    else:                                                             # the callback's latents are cast to the embeddings' type
                        assert torch.equal(got[one], want.to(sc["prompt_embeds"].dtype).float()[one]), f"step {i} view ({b}, {v})"
                    if hasattr(pipe.scheduler, "add_noise"):
                        ref = pipe.scheduler.add_noise(c.float(), noise[b, v], torch.tensor([ts[i + 1]]))
                        assert torch.allclose(want, ref, rtol=0, atol=2e-6 * float(ref.abs().max()))
                    frac = ((masks[b][v] > 0) & (masks[b][v] < 1)).expand(4, 28, 50)
                    assert not torch.equal(got[frac], want.to(got.dtype)[frac])
    assert torch.isfinite(graphed).all()


def test_none_is_todays_call_and_key(dev):
    case = "unipc-bf16"
    pipe = get_pipe(dev, case)
    sc, cl = inputs(case, L=3), given_view_inputs()
    pipe._plans.clear()
    want = call(pipe, sc, cl).images.clone()
    keys_before = list(pipe._plans._d)
    assert len(keys_before) == 1 and not any(isinstance(e, tuple) and e and e[0] == "regions" for e in keys_before[0])
    n = len(keys_before[0])
    try:
        pipe.keep_masks = fractional_masks(cl)
        other = call(pipe, sc, cl).images.clone()
    finally:
        pipe.keep_masks = None
    keys = list(pipe._plans._d)
    assert len(keys) == 2 and keys[0] == keys_before[0] and keys[1] == keys_before[0] + (("regions",),) and len(keys[1]) == n + 1
    assert not torch.equal(other, want)
    assert torch.equal(call(pipe, sc, cl).images, want) and list(pipe._plans._d)[-1] == keys_before[0] and len(pipe._plans) == 2
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    plain = StableDiffusionBEVControlNetPipeline(unet=pipe.unet, controlnet=pipe.controlnet).to(dev)
    plain.keep_masks = fractional_masks(cl)
    with pytest.raises(ValueError, match="no given views"):
        plain(prompt=None, image=sc["bev_map"], camera_param=sc["camera_param"], height=224, width=400, prompt_embeds=sc["prompt_embeds"],
              negative_prompt_embeds=sc["negative_prompt_embeds"], output_type="latent")


@pytest.mark.parametrize("case", ["ddim-bf16", "unipc-f16"])
def test_two_chunks_on_two_streams(dev, case):
    pipe = get_pipe(dev, case)
    sc, cl = inputs(case), given_view_inputs()
    masks = fractional_masks(cl)
    pipe._plans.clear()
    try:
        pipe.keep_masks = masks
        single = call(pipe, sc, cl).images.clone()
        alone = []
        for i in range(2):
            pipe.keep_masks = [masks[i]]
            alone.append(call(pipe, one_scene(sc, i), [cl[i]]).images.clone())
        pipe.keep_masks = masks
        pipe.streams, pipe.min_scenes_per_stream = 2, 1
        n0 = len(pipe._plans)
        chunked = call(pipe, sc, cl).images.clone()
        assert len(pipe._plans) == n0 + 2, "expected one plan per chunk"
    finally:
        pipe.keep_masks, pipe.streams, pipe.min_scenes_per_stream = None, None, 16
    # a chunk is a one-scene plan: the masks, latents and noise of ITS scene, the bits of that scene's own call
    assert torch.equal(chunked, torch.cat(alone)), f"{case}: a chunk differs from its scene's own call"
    # the one-chunk call runs the same arithmetic at another batch shape: equal up to the rounding the repository allows a sampler run
    # against its reference (tests/test_e2e_gpu.py: 2.2e-2 relative L2 for this configuration)
    e = rel_l2(chunked, single)
    print(f"[{case}] two chunks vs one chunk: rel-L2 {e:.3e}")
    check("region call: two chunks vs one chunk", e, 2.2e-2)


@pytest.mark.parametrize("case", ["ddim-bf16", "unipc-f16"])
def test_health_box_bucket_and_scene_boxes_compose(dev, case):
    pipe = get_pipe(dev, case)
    pipe._plans.clear()
    sc, cl = inputs(case), given_view_inputs()
    masks = fractional_masks(cl)
    whole = [[None if v is None else torch.ones(28, 50) for v in r] for r in cl]
    try:
        pipe.keep_masks = masks
        base = call(pipe, sc, cl).images.clone()
        pipe.health = "trace"
        out = call(pipe, sc, cl)
        assert torch.equal(out.images, base), "health='trace' changed the region call's latents"
        h = out.health
        assert h.ok == [True, True] and h.trace.shape == (STEPS, 2, 6, 4) and (h.trace[..., 1] > 0).all()
        # the records describe the BLENDED latents (the blend op precedes the record op).  The last row is the absmax of the fp32 latents;
        # the call returns them in the embeddings' type, and rounding is monotonic: the rounded record is the returned tensor's absmax
        assert torch.equal(torch.from_numpy(h.final[..., 1].copy()).to(base.dtype), base.abs().amax(dim=(2, 3, 4)).cpu())
        pipe.health = None
        # under box_bucket and under scene_boxes: whole-view masks are still, bit for bit, that switch's own given-view call
        for switch in (dict(box_bucket=8), dict(scene_boxes=True)):
            for k, v in switch.items():
                setattr(pipe, k, v)
            pipe.keep_masks = None
            want = call(pipe, sc, cl).images.clone()
            pipe.keep_masks = whole
            got = call(pipe, sc, cl).images.clone()
            pipe.keep_masks = masks
            frac = call(pipe, sc, cl).images
            assert torch.equal(got, want), f"{case} {switch}: whole-view masks differ from the given-view call"
            assert torch.isfinite(frac).all() and not torch.equal(frac, want)
            pipe.box_bucket, pipe.scene_boxes = None, False
    finally:
        pipe.keep_masks, pipe.health, pipe.box_bucket, pipe.scene_boxes = None, None, None, False
