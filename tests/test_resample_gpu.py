"""-m gpu: pipe.resample / SamplerPlan(resample=) on the tiny nets of tests/test_region_keep_gpu.py — 2 scenes, CFG on, DDIM, bf16 and fp16.

The kernel's arithmetic is judged by tests/test_latent_renoise_gpu.py; here the orchestration around it:
  (a) resample = (2, 1) and (10, 3) at 4 steps are schedules without a jump: the bits of the plain keep_masks call;
  (b) resample = (2, 2) at 6 steps launches exactly 10 steps and 2 jumps (counted through the callback and the plan's visit counter), walks
      the timesteps RePaint's index list names, differs from the plain call and is bit-identical on a second call with the same seed;
  (c) a twin driven by this test — the pipeline's own plan, its step program, a fresh ops.LatentRenoise on the plan's buffers launched
      eagerly, the same action list — gives the pipeline's bits exactly, and the counters move as the list says;
  (d) two chunks on two streams, the forked one-scene plan, use_graph=False and health="trace" all run: a chunk has the bits of its scene's
      own (forked) call, the eager loop the graph's bits, the trace changes no bit, and the two-chunk call equals the one-chunk call up to
      what tests/test_region_keep_gpu.py::test_two_chunks_on_two_streams allows (2.2e-2 relative L2);
  (e) with one generator per scene, a scene's seed — hence its jump noise — is the same in a call of its own and inside a batch, and it is
      shared by the scene's views.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import check, given_view_inputs, rel_l2  # noqa: E402
from magicdrive_amd import denoiser as DN, ops as O  # noqa: E402
from magicdrive_amd.schedulers import resample_actions, resample_indices  # noqa: E402
from philox_ref import noise_ref  # noqa: E402
from test_region_keep_gpu import fractional_masks, get_pipe, inputs, one_scene  # noqa: E402


def call(pipe, sc, cl, steps, **kw):
    out = pipe(prompt=None, image=sc["bev_map"], camera_param=sc["camera_param"], height=224, width=400, conditional_latents=cl,
               num_inference_steps=steps, guidance_scale=2.0, latents=sc["latents"], prompt_embeds=sc["prompt_embeds"],
               negative_prompt_embeds=sc["negative_prompt_embeds"], output_type="latent", bev_controlnet_kwargs={"bboxes_3d_data": sc["bboxes_3d_data"]}, **kw)
    torch.cuda.synchronize()
    return out


def gens(base, n=2):
    """One generator per scene (the list form): the latents are passed in, so each generator's first draw is its scene's jump seed."""
    return [torch.Generator().manual_seed(base + i) for i in range(n)]


def resample_plans(pipe):
    return [p for k, p in pipe._plans._d.items() if any(isinstance(e, tuple) and e and e[0] == "resample" for e in k)]


@pytest.mark.parametrize("case", ["ddim-bf16", "ddim-f16"])
def test_schedules_without_a_jump_are_the_plain_call(dev, case):
    pipe = get_pipe(dev, case)
    sc, cl = inputs(case), given_view_inputs()
    try:
        pipe.keep_masks = fractional_masks(cl)
        want = call(pipe, sc, cl, 4).images.clone()
        for rs in ((2, 1), (10, 3)):
            assert resample_actions(4, *rs) == ["step"] * 4
            pipe.resample = rs
            got = call(pipe, sc, cl, 4, generator=gens(5)).images
            assert torch.equal(got, want), f"{case}: resample={rs} takes no jump but differs from the plain call"
    finally:
        pipe.keep_masks, pipe.resample = None, None


@pytest.mark.parametrize("case", ["ddim-bf16", "ddim-f16"])
def test_ten_steps_two_jumps_and_reproducible(dev, case):
    pipe = get_pipe(dev, case)
    sc, cl = inputs(case), given_view_inputs()
    pipe._plans.clear()
    seen = []
    try:
        pipe.keep_masks = fractional_masks(cl)
        plain = call(pipe, sc, cl, 6).images.clone()
        keys_before = list(pipe._plans._d)
        pipe.resample = (2, 2)
        first = call(pipe, sc, cl, 6, generator=gens(11), callback=lambda i, t, lat: seen.append((i, int(t)))).images.clone()
        plan, = resample_plans(pipe)
        assert int(plan.visit_ctr) == 2 and int(plan.step_ctr) == 6
        again = call(pipe, sc, cl, 6, generator=gens(11)).images.clone()
        other = call(pipe, sc, cl, 6, generator=gens(12)).images.clone()
        keys = list(pipe._plans._d)
    finally:
        pipe.keep_masks, pipe.resample = None, None
    acts = resample_actions(6, 2, 2)
    assert acts.count("step") == 10 and acts.count(("jump", 2)) == 2
    assert [i for i, _ in seen] == list(range(10)), "the callback counts step launches"
    ts = pipe.scheduler.timesteps.tolist()
    rev = [t for j, t in enumerate(resample_indices(6, acts)) if j == 0 or t < resample_indices(6, acts)[j - 1]]      # the reverse steps of RePaint's list
    assert [t for _, t in seen] == [ts[6 - 1 - k] for k in rev] == [ts[s] for s in (0, 1, 2, 3, 2, 3, 4, 5, 4, 5)]
    assert len(keys) == len(keys_before) + 1 and keys[-1] == keys_before[-1] + (("resample", 2),), "one trailing key entry, one plan for every seed"
    assert torch.isfinite(first).all() and not torch.equal(first, plain), "two jumps must change the sample"
    assert torch.equal(first, again), f"{case}: the same seed must give the same bits"
    assert not torch.equal(first, other), "another seed, another jump noise"


def test_twin_driven_by_the_action_list(dev):
    case = "ddim-bf16"
    pipe = get_pipe(dev, case)
    sc, cl = inputs(case), given_view_inputs()
    pipe._plans.clear()
    rec = {}
    try:
        pipe.keep_masks, pipe.resample, pipe.fork_max_scenes = fractional_masks(cl), (2, 2), 0      # the linear step program, as in a chunk
        want = call(pipe, sc, cl, 6, generator=gens(21)).images.clone()
        plan, = resample_plans(pipe)
        assert plan.fork_at is None and plan.step is not None
        load = plan.load_inputs
        plan.load_inputs = lambda *a, **k: (rec.update(a=a, k=k), load(*a, **k))[1]
        assert torch.equal(call(pipe, sc, cl, 6, generator=gens(21)).images, want)
        del plan.load_inputs
    finally:
        pipe.keep_masks, pipe.resample, pipe.fork_max_scenes = None, None, 31
    assert rec["k"]["seeds"].tolist() == [int(torch.empty(1, dtype=torch.int64).random_(generator=g)) for g in gens(21)]
    plan.load_inputs(*rec["a"], **rec["k"])                      # the call's inputs again: first sample, counters at zero
    jump = O.LatentRenoise(plan.x.view(-1), plan.coef, plan.step_ctr, plan.visit_ctr, plan.seeds, jump=2, x_in=plan.x_in.view(-1, plan.x_in.shape[-1]),
                           cfg=True, xin_c=4)
    assert O.dtype_code(jump) == O.dtype_code(plan.jump_ops[0])
    st = DN.device_stream(dev)
    plan.prologue.run(st)
    c = v = 0
    for act in resample_actions(6, 2, 2):
        if act == "step":
            plan.step.launch(st)
            c += 1
        else:
            before = plan.x.clone()
            O.run_ops([jump])
            c, v = c - act[1], v + 1
            assert not torch.equal(plan.x, before)
        torch.cuda.synchronize()
        assert (int(plan.step_ctr), int(plan.visit_ctr)) == (c, v)
    assert (c, v) == (6, 2)
    got = plan.latents().to(want.dtype)
    assert torch.equal(got, want), "the twin (step program + eager LatentRenoise on the plan's buffers) differs from the pipeline"


def test_chunks_fork_eager_and_health_run(dev):
    case = "ddim-bf16"
    pipe = get_pipe(dev, case)
    sc, cl = inputs(case), given_view_inputs()
    masks = fractional_masks(cl)
    pipe._plans.clear()
    try:
        pipe.keep_masks, pipe.resample = masks, (2, 2)
        single = call(pipe, sc, cl, 6, generator=gens(31)).images.clone()
        batch_plan, = resample_plans(pipe)
        batch_seeds = batch_plan.seeds.clone()
        pipe.use_graph = False
        eager = call(pipe, sc, cl, 6, generator=gens(31)).images.clone()
        pipe.use_graph = True
        pipe.health = "trace"
        traced = call(pipe, sc, cl, 6, generator=gens(31))
        pipe.health = None
        alone, alone_seeds = [], []
        for i in range(2):                                          # one scene: the forked plan
            pipe.keep_masks = [masks[i]]
            alone.append(call(pipe, one_scene(sc, i), [cl[i]], 6, generator=[gens(31)[i]]).images.clone())
            p1, = [p for p in resample_plans(pipe) if p.b == 1]      # one plan serves both scenes; the chunk plans do not exist yet
            assert p1.fork_at is not None and int(p1.visit_ctr) == 2
            alone_seeds.append(p1.seeds.clone())
        pipe.keep_masks = masks
        pipe.streams, pipe.min_scenes_per_stream = 2, 1
        chunked = call(pipe, sc, cl, 6, generator=gens(31)).images.clone()
    finally:
        pipe.keep_masks, pipe.resample, pipe.streams, pipe.min_scenes_per_stream, pipe.use_graph, pipe.health = None, None, None, 16, True, None
    assert torch.equal(eager, single), "use_graph=False must give the captured graphs' bits"
    assert torch.equal(traced.images, single), "health='trace' changed the resampled latents"
    h = traced.health
    assert h.ok == [True, True] and h.trace.shape == (6, 2, 6, 4) and (h.trace[..., 1] > 0).all(), "rows are indexed by step: a revisit overwrites its row"
    # (e) a scene's seed is its own: the same alone and in the batch, one value for the scene's six views, the generator's first draw
    for i in range(2):
        want = int(torch.empty(1, dtype=torch.int64).random_(generator=gens(31)[i]))
        assert alone_seeds[i].tolist() == [want] * 6 == batch_seeds[6 * i:6 * i + 6].tolist()
        z_alone = noise_ref(int(alone_seeds[i][0]), 1, 64)
        z_batch = noise_ref(int(batch_seeds[6 * i]), 1, 64)
        assert (z_alone == z_batch).all() and np.isfinite(z_alone).all()
    assert batch_seeds[0] != batch_seeds[6]
    # (d) a chunk is a one-scene plan with its scene's seed: the bits of that scene's own call; the one-chunk call up to rounding
    assert torch.equal(chunked, torch.cat(alone)), "a chunk differs from its scene's own call"
    e = rel_l2(chunked, single)
    print(f"[{case}] resample (2, 2): two chunks vs one chunk: rel-L2 {e:.3e}")
    check("resampled region call: two chunks vs one chunk", e, 2.2e-2)
