"""CPU: the per-op parity walker (tests/op_parity.py) can see errors, and its fp64 references are right.

The executor here is the torch interpreter tests/plan_interp.py (fp32 math, storage rounding), on TINY plans as in tests/test_plan_cpu.py: walked
clean, every op of every plan meets every condition; with one op's output altered after the interpreter ran it, the walk fails at that op and at
no other.  The forms a TINY plan does not lower (fused q/k/v with V^T, fused LayerNorm, GEGLU with LayerNorm, the folded 2x upsample conv, key
counts, absent cross-view slots, the short causal attention, the gather with an added row) are checked on small hand-built ops."""
import dataclasses
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import op_parity as P
import plan_interp
from call_state import interp           # the interpreter, one op (an attention with key counts: batch by batch over its first n keys)
from helpers import cfg_inputs, given_view_inputs, scene, state_dicts
from magicdrive_amd import _lib as L, denoiser as DN, ops as O, packing, schedulers
from magicdrive_amd.engine import PackedNet
from magicdrive_amd.networks import spec
from oracle import denoiser as D

CPU = torch.device("cpu")
BF = torch.bfloat16
F64 = torch.float64


@pytest.fixture(scope="module")
def tiny():
    cfg = spec.TINY_CONFIG
    usd, csd = state_dicts(cfg)
    return cfg, usd, csd, PackedNet(usd, CPU), PackedNet(csd, CPU)


def sampler(tiny, b=1, do_cfg=True, steps=2, sched="ddim", given=0, **kw):
    cfg, usd, csd, un, cn = tiny
    sc = scene(cfg, b, 5)
    sch = schedulers.DDIMScheduler() if sched == "ddim" else schedulers.UniPCMultistepScheduler()
    ts = sch.set_timesteps(steps)
    if do_cfg:
        cam, text, bev, boxes = cfg_inputs(D, csd, sc)
    else:
        cam, text, bev, boxes = sc["camera_param"], sc["prompt_embeds"], sc["bev_map"], sc["bboxes_3d_data"]
    sp = DN.SamplerPlan(cfg, un, cn, CPU, b, do_cfg, 5, (28, 50), num_steps=steps, guidance_scale=2.0, scheduler_kind=sched, given_view_mode=given, **kw)
    gv = {}
    if given:
        cl = given_view_inputs()[:b]
        lat = torch.zeros(b, 6, 4, 28, 50)
        for i, r in enumerate(cl):
            for j, v in enumerate(r):
                if v is not None:
                    lat[i, j] = v
        gv = dict(given_mask=torch.tensor([[v is not None for v in r] for r in cl]), given_latents=lat)
    sp.load_inputs(torch.stack([sc["latents"]] * 6, 1), cam, text, bev, boxes, ts, sch.coefficient_table(), **gv)
    return sp


def walk_plan(sp, steps, execute=interp, **kw):
    recs = P.walk(sp.prologue_ops, execute, plan="tiny", **kw)
    for _ in range(steps):
        recs += P.walk(sp.step_ops, execute, plan="tiny", **kw)
    return recs


# ---- clean runs ---------------------------------------------------------------------------------------------------------------------------
def test_clean_walk_cfg_forked_health_trace(tiny):
    sp = sampler(tiny, fork=True, health="trace")
    assert (len(sp.prologue_ops), len(sp.step_ops)) == (85, 598)          # 683 ops: the plan the walker was sized on
    assert isinstance(sp.step_ops[-1], O.GroupStats) and sp.step_ops[-1].row is sp.step_ctr
    recs = walk_plan(sp, 2)
    assert len(recs) == 85 + 2 * 598 and sp.step_ctr.item() == 2
    assert {r.cls for r in recs} >= {"Gemm", "Conv", "Attn", "GroupNorm", "LayerNorm", "Ew", "Layout", "Fourier", "Gather", "TimeEmb", "DdimStep", "GroupStats"}
    assert all(r.rule == "close" for r in recs)
    # the health table holds what the walk judged: one record per step and view, nothing non-finite
    h = sp.health_table()
    assert tuple(h.shape) == (2, 6, 4) and (h[:, :, 0] == 0).all() and (h[:, :, 1] > 0).all()


def test_clean_walk_unipc_given_views(tiny):
    sp = sampler(tiny, sched="unipc", given=1)
    assert isinstance(sp.step_ops[-1], O.UniPCStep) and sp.step_ops[-1].gv_mode == 1
    recs = walk_plan(sp, 2)
    assert len(recs) == len(sp.prologue_ops) + 2 * len(sp.step_ops)


def test_clean_walk_scene_boxes_two_scenes(tiny):
    sp = sampler(tiny, b=2, do_cfg=False, dynamic_boxes="scene")
    rows = [op for op in sp.step_ops if isinstance(op, O.Attn) and op.tk_rows is not None]
    assert rows and len(set(sp.cond.live.tolist())) > 1, "the two scenes must attend to different key counts"
    recs = walk_plan(sp, 2)
    assert len(recs) == len(sp.prologue_ops) + 2 * len(sp.step_ops)


# ---- seeded faults ------------------------------------------------------------------------------------------------------------------------
def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))


def f_no_bias(op, pre):                     # (a)
    op.C.copy_((op.C.float() - op.bias).to(op.C.dtype))


def f_next_temb_row(op, pre):               # (b)
    s = int(op.sel.item())
    Cout = op.Y.shape[3]
    row = lambda k: torch.as_strided(op.temb, (op.Y.shape[0], Cout), (op.temb_b_stride, 1), op.temb.storage_offset() + k * op.temb_sel_stride)
    op.Y.copy_((op.Y.float() + (row(s + 1) - row(s))[:, None, None, :]).to(op.Y.dtype))


def f_zero_block(op, pre):                  # (c)
    op.C[16:32, 16:32] = 0


def f_one_past(op, pre):                    # (d): row 3, one column past the slice
    C = op.C
    assert C.stride(0) > C.shape[1]
    torch.as_strided(C, (1,), (1,), C.storage_offset() + 3 * C.stride(0) + C.shape[1]).add_(1.0)


def f_residual_twice(op, pre):              # (e)
    op.C.copy_((op.C.float() + pre["R"].float()).to(op.C.dtype))


def f_geglu_swapped(op, pre):               # (f)
    raw = op.A.float() @ op.W.float().T + op.bias
    r = raw.reshape(raw.shape[0], -1, 2, 32)
    op.C.copy_((r[:, :, 1] * _gelu(r[:, :, 0])).reshape(raw.shape[0], -1).to(op.C.dtype))


def f_exp_for_exp2(op, pre):                # (g)
    assert op.q_prescaled and op.kvmap is None
    B, Tq, C = op.Q.shape
    h = lambda x: x.float().reshape(B, -1, op.heads, C // op.heads).transpose(1, 2)
    p = torch.softmax(h(op.Q) @ h(op.K).transpose(-1, -2), -1)           # exp(s - max): base e where the contract says base 2
    o = p @ h(op.Vt[:, :, :op.Tk].transpose(1, 2))
    op.O.copy_(o.transpose(1, 2).reshape(B, Tq, C).to(op.O.dtype))


def f_own_view(op, pre):                    # (h)
    B = op.Q.shape[0]
    own = torch.arange(B, dtype=torch.int32).repeat_interleave(op.nsrc)
    plan_interp.run([dataclasses.replace(op, kvmap=own)], lower_check=False)


def f_half_groups(op, pre):                 # (i)
    plan_interp.run([dataclasses.replace(op, groups=op.groups // 2)], lower_check=False)


def f_stale_cond_half(op, pre):             # (j)
    npx = op.x.numel() // op.xin_c
    op.x_in[npx:, :op.xin_c] = pre["x_in"][npx:, :op.xin_c]


def f_touch_input(op, pre):                 # (k)
    op.X[1, 1] += 1.0


def pick(ops, pred):
    hit = [i for i, op in enumerate(ops) if pred(op)]
    assert hit, "no op of the plan has the form this fault needs"
    return hit[0]


def test_every_seeded_fault_fails_at_its_op_and_nowhere_else(tiny):
    sp = sampler(tiny, fork=True, health="trace")
    ops = sp.step_ops
    named = lambda suffix: (lambda op: op.name.endswith(suffix))
    sites = {
        "a": (pick(ops, lambda op: op.name.startswith("zero_conv.") and op.bias is not None and float(op.bias.abs().max()) > 0), f_no_bias, "values"),
        "b": (pick(ops, lambda op: isinstance(op, O.Conv) and op.name.endswith("conv1") and op.temb is not None and op.temb_sel_stride > 0), f_next_temb_row, "values"),
        "c": (pick(ops, named("d1.a0.tb0.ff.out")), f_zero_block, "values"),
        "d": (pick(ops, lambda op: op.name == "zero_conv.1" and op.C.stride(0) > op.C.shape[1]), f_one_past, "borders"),
        "e": (pick(ops, lambda op: isinstance(op, O.Gemm) and op.name.endswith("proj_out") and op.R is not None and op.R.data_ptr() != op.C.data_ptr()), f_residual_twice, "values"),
        "f": (pick(ops, lambda op: isinstance(op, O.Gemm) and op.epilogue == L.EPI_GEGLU), f_geglu_swapped, "values"),
        "g": (pick(ops, lambda op: isinstance(op, O.Attn) and op.q_prescaled and op.kvmap is None and op.Tk <= 400 and op.Tk == op.Q.shape[1]), f_exp_for_exp2, "values"),
        "h": (pick(ops, lambda op: isinstance(op, O.Attn) and op.nsrc == 2 and op.Q.shape[1] <= 400), f_own_view, "values"),
        "i": (pick(ops, lambda op: isinstance(op, O.GroupNorm) and op.groups % 2 == 0 and op.X.shape[1] <= 400 and op.X.data_ptr() != op.Y.data_ptr()), f_half_groups, "values"),
        "j": (pick(ops, lambda op: isinstance(op, O.DdimStep)), f_stale_cond_half, "values"),
        "k": (pick(ops, lambda op: isinstance(op, O.LayerNorm) and op.X.data_ptr() != op.Y.data_ptr()), f_touch_input, "inputs"),
    }
    by_index = {i: (tag, fn, cond) for tag, (i, fn, cond) in sites.items()}
    assert len(by_index) == len(sites), "two faults picked the same op"
    index_of = {id(op): i for i, op in enumerate(ops)}

    def faulty(op):
        hook = by_index.get(index_of.get(id(op)))
        if hook is None:
            return interp(op)
        pre = {k: v.clone() for k, v in vars(op).items() if isinstance(v, torch.Tensor) and k in ("R", "x_in")}
        interp(op)
        hook[1](op, pre)

    P.walk(sp.prologue_ops, interp, plan="tiny")
    recs = P.walk(ops, faulty, plan="tiny", stop=False)
    assert len(recs) == len(ops)
    failed = {r.index: r.failures for r in recs if r.failures}
    assert set(failed) == set(by_index), (sorted(failed), {t: i for t, (i, _, _) in sites.items()}, [str(f[0]) for f in failed.values()])
    for i, (tag, _, cond) in by_index.items():
        assert {f.condition for f in failed[i]} == {cond}, (tag, [str(f) for f in failed[i]])
        assert all(f.index == i and f.op_name == ops[i].name for f in failed[i])
    # stop=True (the default): the first failing condition raises and names the op
    sp2_first = sites["c"][0]
    with pytest.raises(P.OpParityError) as e:
        P.walk(ops[sp2_first:sp2_first + 1], faulty, plan="tiny")
    assert e.value.op_name == ops[sp2_first].name


# ---- the five op classes added since: keep regions, resampling, stochastic DDIM, sdpa, composite --------------------------------------------
def test_no_op_class_is_without_fields_reference_or_interpreter():
    """Every op record of magicdrive_amd/ops.py has its FIELDS entry (naming every tensor field the class declares) and its fp64 reference;
    every one that can occur in a SamplerPlan has its interpreter case.  The next new op cannot be forgotten silently."""
    classes = [c for c in vars(O).values() if isinstance(c, type) and dataclasses.is_dataclass(c) and hasattr(c, "opcode")]
    assert len(classes) >= 21 and {O.Sdpa, O.LatentBlend, O.LatentRenoise, O.DdimEtaStep, O.ImageComposite} <= set(classes)
    for c in classes:
        assert c in P.FIELDS and c in P.REFERENCE, f"op_parity has no FIELDS / REFERENCE entry for {c.__name__}"
        f = P.FIELDS[c]
        known = set(f.inputs) | set(f.outputs) | set(f.scratch)
        tensors = {fl.name for fl in dataclasses.fields(c) if "Tensor" in str(fl.type)}
        assert tensors <= known, f"{c.__name__}: tensor fields {sorted(tensors - known)} are in no Fields entry"
    outside_a_sampler_plan = {O.Sdpa, O.ImageComposite}      # ops.sdpa / the text encoder's own plan; the picture stage behind the VAE
    for c in set(classes) - outside_a_sampler_plan:
        assert c in plan_interp.DISPATCH, f"plan_interp has no case for {c.__name__}"


def everything_on(tiny):
    """Stochastic DDIM + keep regions + resample + health trace, one scene, 2 steps: DdimEtaStep, LatentBlend, GroupStats, one jump program."""
    import call_state as CS
    cfg, usd, csd, un, cn = tiny
    nets = (cfg, csd, un, cn)
    sp = CS.build_plan(nets, "eta_regions_resample_trace", CPU)
    args, kw = CS.inputs(nets, "eta_regions_resample_trace", "B")
    sp.load_inputs(*args, **kw)
    return sp, CS.actions("eta_regions_resample_trace")


def f_jump_stream(op, pre):                 # DdimEtaStep: the noise of the jump's domain (counter word 3 = 0) for the step's
    import philox_ref as PH
    n, s, v = op.x.numel(), int(op.step.item()) - 1, int(op.draw.item()) - 1
    z = lambda fn: torch.from_numpy(np.concatenate([fn(int(sd), v, n // op.seeds.numel()) for sd in op.seeds.tolist()])).float()
    op.x.add_(op.var[s, 1] * (z(PH.noise_ref) - z(PH.eta_noise_ref)))
    plan_interp._refresh_x_in(op, op.x)


def f_alpha_sigma_swapped(op, pre):         # LatentBlend: the two coefficient columns taken for each other
    op.x.copy_(pre["x"]); op.x_in.copy_(pre["x_in"])
    plan_interp.run([dataclasses.replace(op, col_a=3, col_s=2)], lower_check=False)


def f_visit_not_advanced(op, pre):          # LatentRenoise: the jump counter stays: the next jump would repeat this one's noise
    op.visit -= 1


def test_new_sampler_ops_walk_clean_and_each_fault_fails_at_its_op(tiny):
    sp, acts = everything_on(tiny)
    assert acts == ["step", "step", ("jump", 1), "step"]
    hooks = {O.DdimEtaStep: f_jump_stream, O.LatentBlend: f_alpha_sigma_swapped, O.LatentRenoise: f_visit_not_advanced}

    def faulty(op):
        hook = hooks.get(type(op))
        pre = {k: getattr(op, k).clone() for k in ("x", "x_in")} if hook else None
        interp(op)
        if hook:
            hook(op, pre)

    recs = P.walk(sp.prologue_ops, interp, plan="tiny")
    new = lambda ops: [i for i, op in enumerate(ops) if type(op) in hooks]
    # step 0 clean, every op judged: DdimEtaStep with generated noise, LatentBlend at row 0, the trace record of the blended latents
    recs += P.walk(sp.step_ops, interp, plan="tiny")
    assert {"DdimEtaStep", "LatentBlend", "GroupStats"} <= {r.cls for r in recs} and len(recs) == len(sp.prologue_ops) + len(sp.step_ops)
    # step 1 (the last: the blend writes nothing), the jump, step 1 again — clean
    for a in acts[1:]:
        ops = sp.step_ops if a == "step" else sp.jump_ops
        got = P.walk(ops, interp, compare=new(ops), plan="tiny")
        assert [r.cls for r in got] == (["DdimEtaStep", "LatentBlend"] if a == "step" else ["LatentRenoise"])
    assert (int(sp.step_ctr), int(sp.draw_ctr), int(sp.visit_ctr)) == (2, 3, 1)
    # the same trajectory again with one fault per class: caught at its op and nowhere else
    sp, acts = everything_on(tiny)
    P.walk(sp.prologue_ops, interp, compare=(), plan="tiny")
    recs = P.walk(sp.step_ops, faulty, plan="tiny", stop=False)                       # step 0: eta step and blend both write
    failed = {r.cls: {f.condition for f in r.failures} for r in recs if r.failures}
    assert failed == {"DdimEtaStep": {"values"}, "LatentBlend": {"values"}}, {r.name: [str(f) for f in r.failures] for r in recs if r.failures}
    assert sum(bool(r.failures) for r in recs) == 2
    P.walk(sp.step_ops, interp, compare=(), plan="tiny")
    recs = P.walk(sp.jump_ops, faulty, plan="tiny", stop=False)
    assert [(r.cls, {f.condition for f in r.failures}) for r in recs] == [("LatentRenoise", {"values"})], [str(f) for f in recs[0].failures]
    assert "visit" in str(recs[0].failures[0])


def run_sdpa(op, causal_shift=0):
    """A stand-in executor of ops.Sdpa (fp32 torch; the product has only the kernel): causal_shift = -1 hides the diagonal too."""
    B, Tq, C = op.Q.shape
    Tk, H = op.K.shape[1], op.heads
    h = lambda x: x.float().reshape(B, -1, H, C // H).transpose(1, 2)
    s = h(op.Q) @ h(op.K).transpose(-1, -2) * op.scale
    j = torch.arange(Tk)
    if op.causal:
        s = s.masked_fill(j[None, :] > torch.arange(Tq)[:, None] + causal_shift, -math.inf)
    if op.klen is not None:
        s = s.masked_fill((j[None, :] >= op.klen[:, None])[:, None, None, :], -math.inf)
    op.O.copy_((torch.softmax(s, -1) @ h(op.V)).transpose(1, 2).reshape(B, Tq, C).to(op.O.dtype))


def run_composite(op, erode=True):
    """A stand-in executor of ops.ImageComposite from the product's own statement of the matte (dataset.edit_matte); erode=False: the
    window mean of the un-eroded mask, a feather that bleeds into the regenerated region."""
    from magicdrive_amd.dataset.regions import edit_matte
    f = op.gen.shape[2] // op.keep.shape[1]
    if erode:
        w = edit_matte(op.keep, f, op.feather)
    else:
        r = op.feather
        a = op.keep.repeat_interleave(f, -2).repeat_interleave(f, -1)
        w = F.avg_pool2d(F.pad(a[:, None], (r, r, r, r), mode="replicate"), 2 * r + 1, 1)[:, 0]
    if op.has is not None:
        w = w * (op.has != 0).view(-1, 1, 1)
    g = (op.gen / 2 + 0.5).clamp(0, 1).float().permute(0, 2, 3, 1)
    w4 = w[..., None]
    op.out.copy_(torch.where(w4 == 0, g, torch.where(w4 == 1, op.orig, torch.addcmul(g, w4, op.orig - g))))
    if op.matte is not None:
        op.matte.copy_(w)


def test_sdpa_and_composite_walk_clean_and_each_fault_fails_at_its_op():
    import composite_cases as CC
    g = torch.Generator().manual_seed(12)
    B, H, d, T = 2, 3, 16, 33
    qkv = torch.randn(B, T, 3 * H * d, generator=g).to(BF)                  # the column blocks of one projection buffer, passed as they are
    q, k, v = qkv[..., :H * d], qkv[..., H * d:2 * H * d], qkv[..., 2 * H * d:]
    o1, o2, o3 = (torch.zeros(B, T, H * d, dtype=BF) for _ in range(3))
    ci, r = 1, 3
    (V, Hh, W, f), _, _ = CC.CASES[ci]
    gen = (torch.rand(V, 3, Hh, W, generator=g) * 2.4 - 1.2).to(BF)
    orig = torch.randint(0, 256, (V, Hh, W, 3), generator=g).float() / 255.0
    keep = CC.keep_mask(ci)
    out, matte = torch.zeros(V, Hh, W, 3), torch.zeros(V, Hh, W)
    out2 = torch.zeros(V, Hh, W, 3)
    prog = [O.Sdpa(q, k, v, o1, heads=H, scale=d ** -0.5, name="plain"),
            O.Sdpa(q, k, v, o2, heads=H, scale=d ** -0.5, causal=True, name="causal"),
            O.Sdpa(q, k, v, o3, heads=H, scale=d ** -0.5, klen=torch.tensor([T, 7], dtype=torch.int32), name="klen"),
            O.ImageComposite(gen, orig, keep, out, r, matte=matte, name="feathered"),
            O.ImageComposite(gen, orig, keep, out2, 0, has=torch.tensor([1, 0], dtype=torch.uint8), name="has")]

    def clean(op):
        (run_sdpa if isinstance(op, O.Sdpa) else run_composite)(op)
    recs = P.walk(prog, clean)
    assert [r_.cls for r_ in recs] == ["Sdpa"] * 3 + ["ImageComposite"] * 2
    w = P.reference(prog[3])["matte"]
    assert (w == 0).any() and (w == 1).any() and ((w > 0) & (w < 1)).any(), "the case must hold every regime of the matte"
    assert torch.equal(out2[1], (gen[1] / 2 + 0.5).clamp(0, 1).float().permute(1, 2, 0)), "has == 0: the plain picture"

    def faulty(op):
        if op.name == "causal":
            run_sdpa(op, causal_shift=-1)
        elif op.name == "feathered":
            run_composite(op, erode=False)
        else:
            clean(op)
    recs = P.walk(prog, faulty, stop=False)
    assert [bool(r_.failures) for r_ in recs] == [False, True, False, True, False], [[str(f_) for f_ in r_.failures] for r_ in recs]
    assert {f_.condition for f_ in recs[1].failures} <= {"values", "finite"} and {f_.condition for f_ in recs[3].failures} == {"values"}


# ---- the fused forms, by hand at K = 320 --------------------------------------------------------------------------------------------------
def ln_block(M=96, K=320, N=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x0 = (rn(M, K) * 1.5 + 0.7).to(BF)
    gamma, beta = 1.0 + rn(K, sc=0.3), rn(K, sc=0.3)
    W = rn(N, K, sc=K ** -0.5)
    Wp = (W * gamma).to(BF)
    return x0, Wp, (W @ beta).float(), Wp.float().sum(1)


def part_stats(x, cols):
    xf = x.float()
    return torch.stack([torch.stack([xf[:, a:b].sum(1), (xf[:, a:b] ** 2).sum(1)], -1) for a, b in cols])


def test_fused_layernorm_consumer_with_wrong_statistics_fails_at_the_consumer():
    """(l): producer (rowstat out) -> fused-LayerNorm consumer (ln_stats in).  The reference takes mean / rstd from the rows of A, never from
    ln_stats, so statistics of the wrong part count fail the CONSUMER."""
    x0, Wp, b, cs = ln_block()
    M, K = x0.shape
    h = torch.zeros(M, K, dtype=BF)
    st = torch.zeros(3, M, 2)
    C = torch.zeros(M, Wp.shape[0], dtype=BF)
    prog = [O.Gemm(x0, torch.eye(K).to(BF), h, rowstat=st, name="producer"),
            O.Gemm(h, Wp, C, bias=b, ln_eps=1e-5, ln_csum=cs, ln_stats=st, name="consumer")]
    recs = P.walk(prog, interp)
    assert len(recs) == 2

    def wrong_parts(op):
        interp(op)
        if op.name == "consumer":            # the statistics in three column parts, the consumer told there are two
            parts = part_stats(op.A, [(0, 128), (128, 256), (256, 320)])
            plan_interp.run([dataclasses.replace(op, ln_stats=parts[:2].contiguous())], lower_check=False)
    recs = P.walk(prog, wrong_parts, stop=False)
    assert [bool(r.failures) for r in recs] == [False, True] and {f.condition for f in recs[1].failures} == {"values"}


def test_hand_built_fused_forms_walk_clean():
    """Forms only the SD-1.5-size plans lower, small, through the interpreter: fused q/k/v with V^T next to the q/k block (pad columns past vt_T),
    the same with the LayerNorm fused in, GEGLU with LayerNorm from given statistics, a joint-softmax attention over three sources, a conv
    with pad_end, an fp32 GEMM with a step-selected temb row."""
    g = torch.Generator().manual_seed(1)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x0, Wp, b, cs = ln_block(M=96, N=3 * 128)
    Bv, T, Cc = 2, 48, 128
    qk = torch.zeros(96, 2 * Cc, dtype=BF); vt = torch.full((Bv, Cc, 56), 7.0, dtype=BF)
    qk2 = torch.zeros_like(qk); vt2 = torch.full_like(vt, 7.0)
    xg, Wg, bg, csg = ln_block(M=64, N=512, seed=2)
    Cg = torch.zeros(64, 256, dtype=BF)
    q = rn(3, 40, 64).to(BF); k = rn(3, 24, 64).to(BF); v = torch.zeros(3, 64, 32, dtype=BF); v[:, :, :24] = rn(3, 64, 24).to(BF)
    o = torch.zeros(3, 40, 64, dtype=BF)
    X = rn(2, 9, 11, 16).to(BF); Wt = rn(8, 3, 3, 16, sc=0.1).to(BF); Y = torch.zeros(2, 4, 5, 8, dtype=BF)
    tab = rn(4, 3, 32); sel = torch.tensor([2], dtype=torch.int32); A = rn(12, 64).to(BF); W = rn(32, 64, sc=0.1).to(BF); Cf = torch.zeros(12, 32)
    prog = [O.Gemm(x0, Wp[:, :], qk, Vt=vt, vt_from=2 * Cc, vt_T=T, name="qkv"),
            O.Gemm(x0, Wp, qk2, bias=None, Vt=vt2, vt_from=2 * Cc, vt_T=T, ln_eps=1e-5, ln_csum=cs, name="ln+qkv"),
            O.Gemm(xg, Wg, Cg, bias=bg, epilogue=L.EPI_GEGLU, ln_eps=1e-5, ln_csum=csg, ln_stats=part_stats(xg, [(0, 128), (128, 320)]), name="ln+geglu"),
            O.Attn(q, k, v, o, heads=2, Tk=24, scale=32 ** -0.5, kvmap=torch.tensor([0, 1, 2, 1, 2, 0, 2, 0, 1], dtype=torch.int32), nsrc=3, joint=True, name="joint"),
            O.Conv(X, Wt, Y, stride=(2, 2), pad=(0, 0), pad_end=(1, 1), epilogue=L.EPI_SILU, name="pad_end"),
            O.Gemm(A, W, Cf, temb=tab, sel=sel, temb_sel_stride=96, temb_b_stride=32, rows_per_b=4, name="temb")]
    recs = P.walk(prog, interp)
    assert len(recs) == len(prog) and (vt[:, :, T:] == 7.0).all()


# ---- the references of the forms the interpreter does not have ----------------------------------------------------------------------------
@pytest.mark.parametrize("Ho,Wo", [(10, 14), (9, 14), (10, 13), (9, 13)])
def test_reference_upsample2x_is_conv3x3_of_the_nearest_resize(Ho, Wo):
    g = torch.Generator().manual_seed(Ho * 31 + Wo)
    B, Hi, Wi, Cin, Cout = 2, 5, 7, 8, 4
    x = torch.randn(B, Hi, Wi, Cin, generator=g, dtype=F64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=F64)
    bias = torch.randn(Cout, generator=g)
    wf = packing.fold_upsample_conv(w, Ho != 2 * Hi, Wo != 2 * Wi, dtype=None)
    got = P.reference(O.Conv(x, wf, torch.zeros(B, Ho, Wo, Cout), bias=bias, upsample2x=True))["Y"]
    big = x[:, torch.arange(Ho) // 2][:, :, torch.arange(Wo) // 2]          # in the resized image pixel o reads source o >> 1
    want = F.conv2d(big.permute(0, 3, 1, 2), w, bias.double(), padding=1).permute(0, 2, 3, 1)
    assert (got - want).abs().max() < 1e-12


def test_reference_conv_matches_the_fp64_backend():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 9, 11, 6, generator=g, dtype=F64); w = torch.randn(5, 3, 3, 6, generator=g, dtype=F64)
    for stride, pad, pad_end in (((1, 1), (1, 1), None), ((2, 2), (1, 1), None), ((2, 1), (2, 1), None), ((2, 2), (0, 0), (1, 1))):
        pe = pad_end or pad
        Ho, Wo = (9 + pad[0] + pe[0] - 3) // stride[0] + 1, (11 + pad[1] + pe[1] - 3) // stride[1] + 1
        got = P.reference(O.Conv(x, w, torch.zeros(2, Ho, Wo, 5), stride=stride, pad=pad, pad_end=pad_end))["Y"]
        xp = F.pad(x.permute(0, 3, 1, 2), (pad[1], pe[1], pad[0], pe[0]))
        want = F.conv2d(xp, w.permute(0, 3, 1, 2), stride=stride).permute(0, 2, 3, 1)
        assert (got - want).abs().max() < 1e-12, (stride, pad, pad_end)


def _sdpa64(q, k, v, H, scale, mask=None):
    B, Tq, C = q.shape
    h = lambda x: x.reshape(x.shape[0], x.shape[1], H, C // H).transpose(1, 2)
    s = h(q) @ h(k).transpose(-1, -2) * scale
    if mask is not None:
        s = s.masked_fill(~mask, -math.inf)
    return (torch.softmax(s, -1) @ h(v)).transpose(1, 2).reshape(B, Tq, C)


def test_reference_attention_forms():
    g = torch.Generator().manual_seed(4)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    B, H, T, C = 3, 2, 20, 32
    q, k, v = rn(B, T, C), rn(B, T, C), rn(B, T, C)
    o = torch.zeros(B, T, C)
    sc = (C // H) ** -0.5
    # short, V row-major, causal
    got = P.reference(O.Attn(q, k, v, o, heads=H, Tk=T, scale=sc, causal=True, v_rowmajor=True))["O"]
    assert (got - _sdpa64(q, k, v, H, sc, torch.ones(T, T, dtype=torch.bool).tril())).abs().max() < 1e-12
    vt = torch.zeros(B, C, 24, dtype=F64); vt[:, :, :T] = v.transpose(1, 2); vt[:, :, T:] = math.nan       # pad columns never reach O
    # q_prescaled: probabilities are exp2(Q K^T - max)
    got = P.reference(O.Attn(q, k, vt, o, heads=H, Tk=T, scale=123.0, q_prescaled=True))["O"]
    assert (got - _sdpa64(q, k, v, H, math.log(2.0))).abs().max() < 1e-12
    # one count per batch: keys past the count are ignored (NaN there must not matter); a count outside [1, Tk] gives NaN rows for that batch only
    kn = k.clone(); kn[0, 7:] = math.nan; vn = vt.clone(); vn[0, :, 7:] = math.nan
    got = P.reference(O.Attn(q, kn, vn, o, heads=H, Tk=T, scale=sc, tk_rows=torch.tensor([7, T, 0], dtype=torch.int32)))["O"]
    assert (got[0] - _sdpa64(q[:1], k[:1, :7], v[:1, :7], H, sc)[0]).abs().max() < 1e-12
    assert (got[1] - _sdpa64(q[1:2], k[1:2], v[1:2], H, sc)[0]).abs().max() < 1e-12 and torch.isnan(got[2]).all()
    got = P.reference(O.Attn(q, k, vt, o, heads=H, Tk=T, scale=sc, tk_dev=torch.tensor([T + 1], dtype=torch.int32)))["O"]
    assert torch.isnan(got).all()
    # summed sources with absent slots: present ones summed, none present -> zeros
    kv = torch.tensor([1, 2, -1, 0, -1, -1], dtype=torch.int32)
    got = P.reference(O.Attn(q, k, vt, o, heads=H, Tk=T, scale=sc, kvmap=kv, nsrc=2))["O"]
    assert (got[0] - (_sdpa64(q[:1], k[1:2], v[1:2], H, sc) + _sdpa64(q[:1], k[2:3], v[2:3], H, sc))[0]).abs().max() < 1e-12
    assert (got[1] - _sdpa64(q[1:2], k[:1], v[:1], H, sc)[0]).abs().max() < 1e-12 and (got[2] == 0).all()


def test_reference_gather_with_added_row_and_null_blend():
    g = torch.Generator().manual_seed(5)
    Tt = torch.randn(9, 16, generator=g, dtype=F64); add = torch.randn(4, 16, generator=g, dtype=F64); null = torch.randn(16, generator=g, dtype=F64)
    idx = torch.tensor([3, -1, 8, 0, 2, 2]); mask = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8)
    got = P.reference(O.Gather(Tt, torch.zeros(6, 16), idx, mask=mask, null_row=null, add=add))["Y"]
    for i in range(6):
        assert torch.equal(got[i], (Tt[idx[i]] if mask[i] else null) + add[i % 4])


def test_walk_refuses_what_it_has_no_reference_for():
    @dataclasses.dataclass
    class NewOp:
        X: torch.Tensor
        name: str = "new"

    with pytest.raises(NotImplementedError, match="NewOp"):
        P.walk([NewOp(torch.zeros(2))], lambda op: None)
    op = O.Ew(L.EW_COPY, torch.ones(2, 8, dtype=BF), torch.zeros(2, 8, dtype=BF))
    op.extra = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="extra"):
        P.walk([op], interp)
    with pytest.raises(NotImplementedError, match="kind"):
        P.walk([O.Ew(99, torch.ones(2, 8, dtype=BF), torch.zeros(2, 8, dtype=BF))], lambda op: None)
    # an executor that does nothing fails the values condition, and the walk counts what it judged
    with pytest.raises(P.OpParityError, match="values"):
        P.walk([O.Ew(L.EW_COPY, torch.ones(2, 8, dtype=BF), torch.zeros(2, 8, dtype=BF), name="copy")], lambda op: None)


def test_gemm_columns_up_to_roundup4_may_be_zero_filled_and_nothing_else():
    """include/mdx.h: a GEMM with N % 4 != 0 needs ldc >= roundup4(N); the kernels zero-fill those columns (tests/test_tails_gpu.py).  The border
    condition allows exactly that: unchanged or zero."""
    g = torch.Generator().manual_seed(6)
    A = torch.randn(5, 16, generator=g).to(BF); W = torch.randn(6, 16, generator=g).to(BF)
    buf = torch.full((5, 12), 3.0, dtype=BF)
    op = O.Gemm(A, W, buf[:, :6], name="n6")
    assert len(P.walk([op], interp)) == 1                                  # the interpreter leaves columns 6, 7 alone

    def zero_fill(o):
        interp(o); buf[:, 6:8] = 0
    assert len(P.walk([op], zero_fill)) == 1
    for bad in (lambda: buf[:, 6:7].fill_(1.0), lambda: buf[:, 8:9].zero_()):

        def spill(o, bad=bad):
            interp(o); bad()
        buf.fill_(3.0)
        with pytest.raises(P.OpParityError, match="borders"):
            P.walk([op], spill)
