"""-m gpu: per-scene box counts on one plan.  attn_ctx_rows_kernel (csrc/attention_ctx.hip, mdx_attention_ctx_rows_*, ops.Attn.tk_rows): the
key count of query batch b is tk_rows[b], read from device memory when the kernel runs; SamplerPlan(dynamic_boxes="scene") and pipe.scene_boxes on
the tiny nets against each scene's batch-1 call and the reference golden (tests/golden/tiny_pipeline_scene_boxes.pt: one scene per reference call).

No tolerance is new: the kernel's bounds are those of tests/test_attn_ctx_gpu.py (0.3 for what must fail, 0.05 against the fp32 reference; the
pooled bound of that file carries over through bit-identity with the scalar-count kernel), LOOP_BOUND and GOLDEN_BOUND those of
tests/test_box_bucket_gpu.py."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import scene_boxes_data as SB  # noqa: E402
from helpers import check, given_view_inputs, parity_log, rel_l2  # noqa: E402
from magicdrive_amd import _lib as L  # noqa: E402
from magicdrive_amd import ops as O  # noqa: E402
from magicdrive_amd import schedulers  # noqa: E402
from magicdrive_amd.networks import spec  # noqa: E402

B, H = 4, 2
DIMS = (16, 40, 80, 160)
TQS = (28, 130)                # a partial wave; two workgroups
CAPS = (72, 136)
DTYPES = (torch.bfloat16, torch.float16)
NAN = float("nan")
PAD = 8
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
LOOP_BOUND = 2.5e-2              # tests/test_e2e_gpu.py::test_sampler_loop_tiny
GOLDEN_BOUND = 2.2e-2            # tests/test_e2e_gpu.py::test_pipeline_call_matches_reference_goldens (cfg)


def count_vectors(Tk):
    """Both sides of the 64-key tile edge and both ends of the range, mixed within one launch."""
    return ([1, 63, 64, 65], [Tk, 65, 1, 64], [64, Tk, 63, 1])


def rup8(x):
    return (x + 7) // 8 * 8


def make(d, Tq, Tk, ns, pre, dtype):
    """q [B,Tq,C], k [B,Tk,C] with the rows >= ns[b] of batch b scaled x8, vt [B,C,ldv] with ldv = roundup8(Tk) + 8 (columns Tk..ldv NaN), and the
    fp32 reference of every batch over its own first ns[b] keys: a kernel that uses another batch's count, or the capacity, is wrong by O(1)."""
    g = torch.Generator(device="cuda").manual_seed(1000 * d + 10 * Tq + Tk + sum(ns))
    C = H * d
    q = torch.randn(B, Tq, C, generator=g, device="cuda")
    k = torch.randn(B, Tk, C, generator=g, device="cuda")
    v = torch.randn(B, Tk, C, generator=g, device="cuda")
    for b, n in enumerate(ns):
        k[b, n:] *= 8.0
    scale = d ** -0.5
    if pre:
        q = q * (scale * LOG2E)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    vt = torch.full((B, C, rup8(Tk) + PAD), NAN, dtype=dtype, device="cuda")
    vt[:, :, :Tk] = v.transpose(1, 2)
    ref = torch.cat([reference(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], d, LN2 if pre else scale) for b, n in enumerate(ns)])
    return q, k, v, vt, ref


def reference(q, k, v, d, factor):
    Bq, Tq, C = q.shape
    qh = q.float().view(Bq, Tq, H, d).transpose(1, 2)
    kh = k.float().view(Bq, -1, H, d).transpose(1, 2)
    vh = v.float().view(Bq, -1, H, d).transpose(1, 2)
    att = torch.softmax(qh @ kh.transpose(-1, -2) * factor, -1)
    return (att @ vh).transpose(1, 2).reshape(Bq, Tq, C)


def rows_of(ns):
    return torch.tensor(list(ns), dtype=torch.int32, device="cuda")


def run_rows(q, k, vt, Tk, rows, d, pre):
    o = torch.full_like(q, NAN)
    O.run_ops([O.Attn(q, k, vt, o, heads=H, Tk=Tk, scale=d ** -0.5, q_prescaled=pre, tk_rows=rows)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    assert kern == f"attn_ctx_kernel<{d},{'pre' if pre else 'scaled'},rows>", kern
    return o


def run_scalar(q, k, vt, Tk, n, d, pre):
    """The scalar-count kernel (tk_dev -> one int32), on whatever batches it is given."""
    o = torch.full_like(q, NAN)
    O.run_ops([O.Attn(q, k, vt, o, heads=H, Tk=Tk, scale=d ** -0.5, q_prescaled=pre, tk_dev=torch.tensor([n], dtype=torch.int32, device="cuda"))])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    assert kern == f"attn_ctx_kernel<{d},{'pre' if pre else 'scaled'}>", kern
    return o


def per_batch_scalar(q, k, vt, Tk, ns, d, pre):
    return torch.cat([run_scalar(q[b:b + 1], k[b:b + 1], vt[b:b + 1], Tk, n, d, pre) for b, n in enumerate(ns)])


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("d", DIMS)
def test_per_batch_key_count_every_edge(dev, d, dtype):
    """(a) bit-identical to the scalar-count kernel on every batch's slice, (b) NaN poison at and past n_b changes nothing, (c) the scalar kernel
    at the batch maximum misses the short batches by > 0.3 while the rows kernel is within 0.05 of the fp32 reference."""
    kind = "bf16" if dtype == torch.bfloat16 else "fp16"
    worst = 0.0
    for pre in (False, True):
        for Tq in TQS:
            for Tk in CAPS:
                for ns in count_vectors(Tk):
                    q, k, v, vt, ref = make(d, Tq, Tk, ns, pre, dtype)
                    o = run_rows(q, k, vt, Tk, rows_of(ns), d, pre)
                    assert torch.isfinite(o).all(), (Tq, Tk, ns, pre)
                    # (a)
                    want = per_batch_scalar(q, k, vt, Tk, ns, d, pre)
                    assert torch.equal(o, want), f"differs from the scalar-count kernel: Tq={Tq} Tk={Tk} ns={ns} pre={pre}"
                    # (b)
                    kp, vp = k.clone(), vt.clone()
                    for b, n in enumerate(ns):
                        kp[b, n:] = NAN
                        vp[b, :, n:] = NAN          # columns n_b .. Tk and the pad columns Tk .. ldv
                    assert torch.equal(run_rows(q, kp, vp, Tk, rows_of(ns), d, pre), o), f"poison leaks: Tq={Tq} Tk={Tk} ns={ns} pre={pre}"
                    # (c)
                    at_max = run_scalar(q, k, vt, Tk, max(ns), d, pre)
                    for b, n in enumerate(ns):
                        e = rel(o[b], ref[b])
                        worst = max(worst, e)
                        assert e < 0.05, (Tq, Tk, ns, pre, b, e)
                        if n < max(ns):
                            assert rel(at_max[b], ref[b]) > 0.3, (Tq, Tk, ns, pre, b)
                        else:
                            assert torch.equal(at_max[b], o[b])
    print(f"[attn_ctx rows d={d} {kind}] worst per-batch rel-L2 vs fp32 {worst:.3e}")
    parity_log(f"scene_boxes:attn_ctx_rows:d{d}:{kind}", worst_rel_l2_vs_fp32=worst, limit=0.05)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("d", (40, 160))
def test_one_count_out_of_range_poisons_its_own_batch_only(dev, d, dtype):
    """A count outside [1, Tk] cannot raise without a sync: every O row of THAT batch is NaN (addressing as for a clamped count; K has exactly Tk
    rows, V^T rows end at ldv), the other batches are bit-identical to the scalar-count kernel's."""
    Tq, Tk = 130, 72
    good = [65, 1, 72, 64]
    q, k, v, vt, _ = make(d, Tq, Tk, good, False, dtype)
    vt = vt[:, :, :rup8(Tk)].contiguous()
    want = per_batch_scalar(q, k, vt, Tk, good, d, False)
    for slot, bad in ((1, 0), (3, Tk + 1), (0, -5), (2, 2 ** 31 - 1)):
        ns = list(good)
        ns[slot] = bad
        o = run_rows(q, k, vt, Tk, rows_of(ns), d, False)
        for b in range(B):
            if b == slot:
                assert torch.isnan(o[b]).all(), (slot, bad)
            else:
                assert torch.equal(o[b], want[b]), (slot, bad, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_graph_replay_reads_the_current_counts(dev, dtype):
    """One captured launch, replayed after the counts changed: each replay equals the eager run for its counts; first and third are bit-identical."""
    d, Tq, Tk = 40, 130, 136
    va, vb = [1, 63, 64, 65], [136, 65, 1, 64]
    q, k, v, vt, _ = make(d, Tq, Tk, va, True, dtype)
    eager = {tuple(ns): run_rows(q, k, vt, Tk, rows_of(ns), d, True) for ns in (va, vb)}
    assert not torch.equal(eager[tuple(va)], eager[tuple(vb)])
    rows = rows_of(va)
    o = torch.full_like(q, NAN)
    prog = O.build_program([O.Attn(q, k, vt, o, heads=H, Tk=Tk, scale=d ** -0.5, q_prescaled=True, tk_rows=rows)])
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for ns in (va, vb, va):
        rows.copy_(rows_of(ns))            # an ordinary stream-ordered write between replays
        o.fill_(NAN)
        prog.launch(st)
        outs.append(o.clone())
    torch.cuda.synchronize()
    prog.destroy()
    assert torch.equal(outs[0], eager[tuple(va)]) and torch.equal(outs[1], eager[tuple(vb)]) and torch.equal(outs[2], outs[0])


# ---- plan and pipeline, tiny nets --------------------------------------------------------------------------------------------------------
def _pipe(dev, cfg, scheduler=None, torch_dtype=None, given_view=False):
    from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    from magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view import StableDiffusionBEVControlNetGivenViewPipeline
    kw = {} if torch_dtype is None else {"torch_dtype": torch_dtype}
    cls = StableDiffusionBEVControlNetGivenViewPipeline if given_view else StableDiffusionBEVControlNetPipeline
    pipe = cls(unet=UNet2DConditionModelMultiview.from_config(cfg, 0, **kw), controlnet=BEVControlNetModel.from_config(cfg, 1, **kw)).to(dev)
    if scheduler is not None:
        pipe.scheduler = scheduler.from_config(pipe.scheduler.config)
    return pipe


def _call(pipe, sc, steps, gs, **kw):
    return pipe(prompt=None, image=sc["bev_map"], camera_param=sc["camera_param"], height=224, width=400, num_inference_steps=steps,
                guidance_scale=gs, latents=sc["latents"], prompt_embeds=sc["prompt_embeds"], negative_prompt_embeds=sc["negative_prompt_embeds"],
                output_type="latent", bev_controlnet_kwargs={"bboxes_3d_data": sc["bboxes_3d_data"]}, **kw).images.clone()


@pytest.fixture(scope="module")
def golden():
    G = torch.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_pipeline_scene_boxes.pt"))
    G["scenes"] = [SB.unpack_scene(p) for p in G["scenes"]]
    return G


def test_pipeline_scene_boxes_equals_every_scenes_batch_1_call(dev, golden):
    """One pipe() call with scenes of 0, 2 and 5 boxes, scene_boxes on at box_bucket 8: every scene against its own batch-1 call (exact plan) and
    against the reference run one scene per call; the padded call (feature off) is measured beside it.  Then other counts on the same plan
    object: nothing is rebuilt or recaptured."""
    cfg = spec.TINY_CONFIG
    steps, gs, scenes = golden["steps"], golden["guidance"], golden["scenes"]
    exact, mine = _pipe(dev, cfg), _pipe(dev, cfg)
    assert mine.scene_boxes is False
    mine.scene_boxes, mine.box_bucket = True, 8
    bat = SB.batched(scenes)
    out = _call(mine, bat, steps, gs)
    padded = _call(exact, bat, steps, gs)
    torch.cuda.synchronize()
    (plan,) = mine._plans.values()
    assert plan.scene_boxes and plan.dynamic_boxes and plan.cond.L == 8 and plan.b == 3
    assert plan.cond.live.view(6, 6)[:, 0].tolist() == [78, 80, 83] * 2
    assert (8, "scene") in next(iter(mine._plans._d))            # the plan key's box entry
    programs = (plan.prologue, plan.step, plan.step_cn, plan.step_enc, plan.step_tail)
    for i, (sc, k) in enumerate(zip(scenes, golden["counts"])):
        alone = _call(exact, sc, steps, gs)
        torch.cuda.synchronize()
        e, ep = rel_l2(out[i:i + 1], alone), rel_l2(padded[i:i + 1], alone)
        eg, eg1 = rel_l2(out[i:i + 1], golden["latents"][i]), rel_l2(alone, golden["latents"][i])
        print(f"[pipe.scene_boxes, {k} boxes] vs its batch-1 call: {e:.4e} (padded batch {ep:.4e}); vs reference batch-1 golden {eg:.4f} (batch-1 call {eg1:.4f})")
        parity_log(f"scene_boxes:pipeline_tiny:{k}_boxes", scene_vs_batch1=e, padded_vs_batch1=ep, scene_vs_golden=eg, batch1_vs_golden=eg1,
                   loop_limit=LOOP_BOUND, golden_limit=GOLDEN_BOUND)
        check(f"tiny pipeline, scene_boxes vs the scene's batch-1 call, {k} boxes", e, LOOP_BOUND)
        check(f"tiny pipeline, scene_boxes vs reference batch-1 golden, {k} boxes", eg, GOLDEN_BOUND)
    # other counts, other padding, the same plan: scenes in another order, padded to 7 by the caller
    perm = [2, 0, 1]
    bat2 = SB.batched([scenes[j] for j in perm], 7)
    out2 = _call(mine, bat2, steps, gs)
    torch.cuda.synchronize()
    assert len(mine._plans) == 1 and next(iter(mine._plans.values())) is plan
    assert (plan.prologue, plan.step, plan.step_cn, plan.step_enc, plan.step_tail) == programs
    assert plan.cond.live.view(6, 6)[:, 0].tolist() == [83, 78, 80] * 2
    for pos, j in enumerate(perm):
        check(f"tiny pipeline, scene_boxes, second call on the same plan, scene {j}", rel_l2(out2[pos:pos + 1], out[j:j + 1]), LOOP_BOUND)
    # a call without boxes keeps its own exact plan
    _call(mine, scenes[0], steps, gs)
    torch.cuda.synchronize()
    assert sorted((p.cond.L, p.scene_boxes) for p in mine._plans.values()) == [(0, False), (8, True)]


@pytest.mark.parametrize("case", ["fork_b1", "unipc", "fp16", "given_view"])
def test_pipeline_scene_boxes_forked_plan_unipc_fp16_given_view(dev, golden, case):
    """The forked one-scene plan (the 2-box scene padded to 5 by the caller: ControlNet and UNet encoder on two streams, both reading the counts),
    the UniPC scheduler, fp16 models (the _f16 build of the kernel inside a plan) and the given-view pipeline."""
    cfg = spec.TINY_CONFIG
    scenes = golden["scenes"]
    sched = schedulers.UniPCMultistepScheduler if case == "unipc" else None
    tdt = torch.float16 if case == "fp16" else None
    gv = case == "given_view"
    exact, mine = _pipe(dev, cfg, sched, tdt, gv), _pipe(dev, cfg, sched, tdt, gv)
    mine.scene_boxes, mine.box_bucket = True, 8
    if case == "fork_b1":
        sel, bat = [1], SB.batched(scenes[1:2], 5)
    elif gv:
        sel, bat = [1, 2], SB.batched(scenes[1:])
    else:
        sel, bat = [0, 1, 2], SB.batched(scenes)
    cl = given_view_inputs() if gv else None
    kw = (lambda rows: dict(conditional_latents=[cl[r] for r in rows], conditional_latents_change_every_input=True)) if gv else (lambda rows: {})
    out = _call(mine, bat, 5, 2.0, **kw(range(len(sel))))
    torch.cuda.synchronize()
    for pos, j in enumerate(sel):
        alone = _call(exact, scenes[j], 5, 2.0, **kw([pos]))
        torch.cuda.synchronize()
        e = rel_l2(out[pos:pos + 1], alone)
        parity_log(f"scene_boxes:pipeline_tiny:{case}:{golden['counts'][j]}_boxes", scene_vs_batch1=e, limit=LOOP_BOUND)
        check(f"tiny pipeline {case}, scene_boxes vs the scene's batch-1 call, {golden['counts'][j]} boxes", e, LOOP_BOUND)
    (plan,) = mine._plans.values()
    assert plan.dtype == (torch.float16 if case == "fp16" else torch.bfloat16)
    assert plan.scene_boxes and plan.cond.L == 8 and (plan.fork_at is not None) and plan.scheduler_kind == ("unipc" if case == "unipc" else "ddim")
    assert plan.given_view_mode == (1 if gv else 0)
    assert plan.cond.live.view(2, len(sel), 6)[0, :, 0].tolist() == [78 + golden["counts"][j] for j in sel]
