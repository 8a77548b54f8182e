"""CPU: the plans built with keep_regions, resample and stochastic are executed (tests/plan_interp.py) for the first time, and a cached
plan is shown to carry nothing from one call to the next (tests/call_state.py).  TINY_CONFIG, latent 28 x 50, 2 steps.

  executed   each new plan against the closed form the GPU pipeline tests use for its feature: the twin without regions of
             tests/test_region_keep_gpu.py (a plain plan plus one hand-built ops.LatentBlend on its buffers: same bits after every step),
             the action-list twin of tests/test_resample_gpu.py (a plan without resample driven by the list, with a hand-built
             ops.LatentRenoise on its buffers: same bits, the counters as the list says), and closed_form() of
             tests/test_ddim_eta_gpu.py (conv_out zeroed: eps is exactly 0 and the latents are a float64 formula of the initial latents,
             the seeds and the counters, with that test's derived bound).  What is checked is the lowering — which views, which counter,
             which seeds, which order — not the interpreter's arithmetic, which both sides share.
  poison     every plan of call_state.PLANS: build, poison every byte its programs write, load_inputs(B), run — bit-identical, behind
             every action, to a freshly built plan that runs B alone.
  omissions  the instrument proves itself: with ONE reset of load_inputs left out (call_state.NoReset through monkeypatch) the same
             comparison differs, or the interpreter refuses a wild integer."""
import numpy as np
import pytest
import torch

import call_state as CS
from helpers import state_dicts
from magicdrive_amd import ops as O, schedulers
from magicdrive_amd.engine import PackedNet
from magicdrive_amd.networks import spec
from test_ddim_eta_gpu import closed_form

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def tiny():
    cfg = spec.TINY_CONFIG
    usd, csd = state_dicts(cfg)
    return cfg, csd, PackedNet(usd, CPU), PackedNet(csd, CPU)


@pytest.fixture(scope="module")
def tiny_zero_eps():
    """conv_out zeroed: the noise prediction is exactly 0 whatever the conditions are (tests/test_ddim_eta_gpu.py: zero_eps_pipe)."""
    cfg = spec.TINY_CONFIG
    usd, csd = state_dicts(cfg)
    usd["conv_out.weight"].zero_(); usd["conv_out.bias"].zero_()
    return cfg, csd, PackedNet(usd, CPU), PackedNet(csd, CPU)


def loaded(nets, which):
    plan = CS.build_plan(nets, which, CPU)
    args, kw = CS.inputs(nets, which, "B")
    plan.load_inputs(*args, **kw)
    return plan, args, kw


# ---- the new plans, executed ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", ["ddim", "unipc"])
def test_region_plan_is_its_twin_plus_a_blend(tiny, sched):
    which = dict(CS.PLANS["regions"], sched=sched)
    region, args, kw = loaded(tiny, which)
    twin = CS.build_plan(tiny, dict(sched=sched), CPU)
    twin.load_inputs(*args)
    assert len(region.step_ops) == len(twin.step_ops) + 1 and isinstance(region.step_ops[-1], O.LatentBlend)
    twin.x.copy_(region.x); twin.x_in.copy_(region.x_in)                   # the blended first sample
    steps = region.num_steps
    blend = O.LatentBlend(twin.x.view(-1), region.gv_cond.view(-1), region.gv_noise.view(-1), region.keep.view(-1), twin.coef, twin.step_ctr,
                          last_step=steps - 1, x_in=twin.x_in.view(-1, twin.x_in.shape[-1]), cfg=False, xin_c=4)
    m = region.keep.unsqueeze(-1).expand_as(region.x)
    assert (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).any()
    for p in (region, twin):
        for op in p.prologue_ops:
            CS.interp(op)
    for s in range(steps):
        for p in (region, twin):
            for op in p.step_ops:
                CS.interp(op)
        unblended = twin.x.clone()
        CS.interp(blend)
        assert int(region.step_ctr) == int(twin.step_ctr) == s + 1
        assert torch.equal(region.x, twin.x) and torch.equal(region.x_in, twin.x_in) and torch.equal(region.eps, twin.eps), f"step {s}"
        if s < steps - 1:
            assert torch.equal(twin.x[m == 0], unblended[m == 0]) and not torch.equal(twin.x[m == 1], unblended[m == 1])
        else:
            assert torch.equal(twin.x, unblended), "the last step's output stays the scheduler's"
        if sched == "unipc":
            assert torch.equal(region.x_last, twin.x_last) and torch.equal(region.m1, twin.m1) and torch.equal(region.m2, twin.m2)
    assert torch.isfinite(region.x).all()


def drive(plan, acts, jump_ops):
    """Run `acts` with `jump_ops` standing for a jump; returns the (step, visit) counters seen behind every action."""
    for op in plan.prologue_ops:
        CS.interp(op)
    seen = []
    for a in acts:
        for op in (plan.step_ops if a == "step" else jump_ops):
            CS.interp(op)
        seen.append(int(plan.step_ctr))
    return seen


def counters(acts):
    c, out = 0, []
    for a in acts:
        c = c + 1 if a == "step" else c - a[1]
        out.append(c)
    return out


def test_resample_plan_is_its_twin_driven_by_the_action_list(tiny):
    acts = CS.actions("regions_resample")
    assert acts == ["step", "step", ("jump", 1), "step"], "the shortest list with one jump and one revisited step"
    plan, args, kw = loaded(tiny, "regions_resample")
    twin = CS.build_plan(tiny, "regions", CPU)
    twin.load_inputs(*args, **{k: v for k, v in kw.items() if k != "seeds"})
    assert len(plan.step_ops) == len(twin.step_ops) and len(plan.jump_ops) == 1 and not twin.jump_ops
    visit = torch.zeros(1, dtype=torch.int32)
    jump = O.LatentRenoise(twin.x.view(-1), twin.coef, twin.step_ctr, visit, kw["seeds"].repeat_interleave(6), jump=CS.RESAMPLE[0],
                           x_in=twin.x_in.view(-1, twin.x_in.shape[-1]), cfg=False, xin_c=4)
    assert drive(plan, acts, plan.jump_ops) == drive(twin, acts, [jump]) == counters(acts) == [1, 2, 1, 2]
    assert int(plan.visit_ctr) == int(visit) == 1
    assert torch.equal(plan.x, twin.x) and torch.equal(plan.x_in, twin.x_in) and torch.isfinite(plan.x).all()
    # the jump changed the sample: the same list without it ends elsewhere
    plain, _, _ = loaded(tiny, "regions")
    drive(plain, ["step", "step"], [])
    assert not torch.equal(plain.x, plan.x)


def closed_form_views(plan, nets, which, acts, views):
    """Worst |latents - closed form| / derived bound over `views` of scene 0 (tests/test_ddim_eta_gpu.py: closed_form, eps == 0)."""
    args, kw = CS.inputs(nets, which, "B")
    sch = schedulers.DDIMScheduler(); sch.set_timesteps(plan.num_steps)
    assert torch.equal(plan.coef, sch.coefficient_table()) and torch.equal(plan.var, kw["var"])
    ref, bound = closed_form(args[0][0, 0], int(kw["seeds"][0]), sch.coefficient_table(), kw["var"], actions=acts)
    got = plan.x.view(6, -1).double().numpy()
    return max(float((np.abs(got[v] - ref) / bound).max()) for v in views)


def test_stochastic_plan_has_its_closed_form(tiny_zero_eps):
    plan, args, kw = loaded(tiny_zero_eps, "eta")
    acts = CS.actions("eta")
    assert sum(isinstance(op, O.DdimEtaStep) for op in plan.step_ops) == 1 and not any(isinstance(op, O.DdimStep) for op in plan.step_ops)
    assert drive(plan, acts, []) == [1, 2] and int(plan.draw_ctr) == 2
    assert not plan.eps.any(), "conv_out is zero: eps must be exactly 0"
    worst = closed_form_views(plan, tiny_zero_eps, "eta", acts, range(6))
    print(f"[eta plan on the interpreter] worst |latents - closed form| / derived bound = {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(plan.x_in[..., :4], plan.x.to(plan.x_in.dtype)) and not plan.x_in[..., 4:].any()


def test_stochastic_region_resample_plan_closed_form_and_twin(tiny_zero_eps):
    """Everything on at once.  A view that is not given is regenerated whole (its mask is 0: the blend leaves it alone), so it follows the
    closed form of the action list with draw = 0, 1, 2 and visit = 0 — a revisited step draws fresh noise.  The given view is held to the
    action-list twin: a plan without resample, a hand-built jump on its buffers."""
    which = "eta_regions_resample_trace"
    acts = CS.actions(which)
    plan, args, kw = loaded(tiny_zero_eps, which)
    assert plan.jump_ops[0].seeds is plan.seeds and plan.step_ops[-3].seeds is plan.seeds, "one seed tensor for both streams"
    assert [type(op).__name__ for op in plan.step_ops[-3:]] == ["DdimEtaStep", "LatentBlend", "GroupStats"]
    assert drive(plan, acts, plan.jump_ops) == [1, 2, 1, 2]
    assert (int(plan.draw_ctr), int(plan.visit_ctr)) == (3, 1), "the jump moves step_ctr back and leaves draw_ctr alone"
    free = [v for v in range(6) if not bool(kw["given_mask"][0, v])]
    assert len(free) == 5
    worst = closed_form_views(plan, tiny_zero_eps, which, acts, free)
    print(f"[eta + regions + resample plan on the interpreter] worst |latents - closed form| / derived bound = {worst:.3f}")
    assert worst <= 1.0
    twin = CS.build_plan(tiny_zero_eps, dict(given=1, keep_regions=True, stochastic=True, health="trace"), CPU)
    twin.load_inputs(*args, **kw)
    visit = torch.zeros(1, dtype=torch.int32)
    jump = O.LatentRenoise(twin.x.view(-1), twin.coef, twin.step_ctr, visit, twin.seeds, jump=CS.RESAMPLE[0], x_in=twin.x_in.view(-1, twin.x_in.shape[-1]),
                           cfg=False, xin_c=4)
    drive(twin, acts, [jump])
    assert torch.equal(plan.x, twin.x) and torch.equal(plan.x_in, twin.x_in) and torch.equal(plan.health_table(), twin.health_table())
    h = plan.health_table()
    assert tuple(h.shape) == (2, 6, 4) and (h[:, :, 0] == 0).all() and (h[:, :, 1] > 0).all()


# ---- poison every byte the programs write, then load a call and run it ---------------------------------------------------------------------
_FRESH = {}


def fresh_trail(nets, which):
    """What a freshly built plan leaves behind every action of call B: computed once per plan, never written to."""
    if which not in _FRESH:
        plan, _, _ = loaded(nets, which)
        _FRESH[which] = CS.run_interpreted(plan, CS.actions(which))
    return _FRESH[which]


def poisoned_trail(nets, which, omit=(), monkeypatch=None):
    """Build, poison, load_inputs(B) — with the resets of the attributes `omit` left out — and run.  In front of the poison the inputs of
    call A are loaded (never run): what no op writes — masks, seeds, tables, key counts, box slots, text rows — then holds another call's
    legal values, boxes at the capacity and every view given, instead of the zeros of a new plan."""
    plan = CS.build_plan(nets, which, CPU)
    args, kw = CS.inputs(nets, which, "A")
    plan.load_inputs(*args, **kw)
    assert CS.poison(plan) > 0
    args, kw = CS.inputs(nets, which, "B")
    if omit:
        with monkeypatch.context() as mp:
            for name in omit:
                mp.setattr(plan, name, CS.NoReset(getattr(plan, name)))
            plan.load_inputs(*args, **kw)
        assert all(isinstance(getattr(plan, name), torch.Tensor) for name in omit)
    else:
        plan.load_inputs(*args, **kw)
    return CS.run_interpreted(plan, CS.actions(which))


def test_the_poison_fills_what_the_programs_write_and_nothing_else(tiny):
    which = "eta_regions_resample_trace"
    plan = CS.build_plan(tiny, which, CPU)
    before = {k: v.clone() for k, v in dict(coef=plan.coef, var=plan.var, seeds=plan.seeds, keep=plan.keep, gv_cond=plan.gv_cond, ctx_text=plan.cond.ctx[:, 1:78],
                                            box_in=plan.cond.box_in, w=plan.step_ops[0].Wt, pads=plan.x_in[..., 4:]).items()}
    n = CS.poison(plan)
    # written by ops: the latents, the model input's latent channels, eps, every counter, the health table, the camera and box tokens,
    # the temb tables, pooled activations, workspaces
    assert torch.isnan(plan.x).all() and torch.isnan(plan.x_in[..., :4]).all() and torch.isnan(plan.eps).all() and torch.isnan(plan._health).all()
    assert torch.isnan(plan.cond.ctx[:, 0]).all() and torch.isnan(plan.cond.ctx[:, 78:]).all() and torch.isnan(plan.bld.ws).all()
    for ctr in (plan.step_ctr, plan.visit_ctr, plan.draw_ctr):
        assert int(ctr) == 0x5A5A5A5A
    # not written by any op: they keep their bits
    now = dict(coef=plan.coef, var=plan.var, seeds=plan.seeds, keep=plan.keep, gv_cond=plan.gv_cond, ctx_text=plan.cond.ctx[:, 1:78], box_in=plan.cond.box_in,
               w=plan.step_ops[0].Wt, pads=plan.x_in[..., 4:])
    for k, v in before.items():
        assert torch.equal(now[k], v), k
    assert n > plan.x.numel() * 4
    # every op's every output view lies inside the poison: nothing the walker would call an output was left out
    for op in plan.step_ops[:40] + plan.jump_ops:
        for v in CS.P.out_views(op).values():
            assert not torch.isfinite(v.float()).any() if v.is_floating_point() else int(v.reshape(-1)[0]) == 0x5A5A5A5A, op.name


@pytest.mark.parametrize("which", list(CS.PLANS))
def test_a_poisoned_plan_gives_the_bits_of_a_fresh_one(tiny, which):
    want = fresh_trail(tiny, which)
    assert torch.isfinite(want[-1]["latents"]).all()
    if which == "scene_boxes_b2":
        plan, _, _ = loaded(tiny, which)
        assert len(set(plan.cond.live.tolist())) > 1, "the two scenes must attend to different key counts"
    got = poisoned_trail(tiny, which)
    assert CS.differences(got, want) == [], "a carry-over: bytes an op writes, load_inputs does not reset, and an op reads before this call wrote them"


# (plan, the attributes whose reset is left out).  Each must be seen: a difference somewhere in the trail, or a refusal of the interpreter.
OMISSIONS = {
    "step_ctr.zero_": ("health_final", ["step_ctr"]),
    "visit_ctr.zero_": ("regions_resample", ["visit_ctr"]),
    "draw_ctr.zero_": ("eta", ["draw_ctr"]),
    "unipc history zero_": ("unipc_given1", ["x_last", "m1", "m2"]),
    "m1.zero_": ("unipc_given1", ["m1"]),
    "_health.zero_ (trace)": ("health_trace", ["_health"]),
    "gv_cond.copy_": ("regions", ["gv_cond"]),
    "gv_noise.copy_": ("given2", ["gv_noise"]),
    "x.copy_": ("eta", ["x"]),
}


# Resets nothing can see, kept in load_inputs all the same.  unipc_kernel (csrc/elementwise.hip) uses x_last and m2 only under
# `if (c[2] != 0.f)`, which row 0 of every UniPC table fails (the first step has no corrector), and overwrites both in its last line
# (x_last <- xc, m2 <- m1): the first step of a call replaces them before anything reads them.  m1 IS read by that step (c[9] * m1, m2 <- m1).
DEAD = {"x_last.zero_": ("unipc_given1", ["x_last"]), "m2.zero_": ("unipc_given1", ["m2"])}


@pytest.mark.parametrize("what", list(DEAD))
def test_a_dead_reset_stays_dead(tiny, monkeypatch, what):
    """If this fails the kernel has begun to read the state before writing it: move the entry to OMISSIONS."""
    which, omit = DEAD[what]
    sch = schedulers.UniPCMultistepScheduler(); sch.set_timesteps(2)
    assert float(sch.coefficient_table()[0, 2]) == 0.0, "row 0 of a UniPC table must switch the corrector off"
    assert CS.differences(poisoned_trail(tiny, which, omit, monkeypatch), fresh_trail(tiny, which)) == []


@pytest.mark.parametrize("what", list(OMISSIONS))
def test_a_missing_reset_is_seen(tiny, monkeypatch, what):
    which, omit = OMISSIONS[what]
    want = fresh_trail(tiny, which)
    try:
        got = poisoned_trail(tiny, which, omit, monkeypatch)
    except (IndexError, AssertionError, RuntimeError, ValueError, OverflowError) as e:      # a wild integer in front of the interpreter
        print(f"[{what}] refused: {type(e).__name__}: {str(e)[:120]}")
        return
    diff = CS.differences(got, want)
    print(f"[{what}] differs in {diff}")
    assert diff, f"load_inputs without {what} gave the fresh plan's bits: the instrument is blind to this state"
