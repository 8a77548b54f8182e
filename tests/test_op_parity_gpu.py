"""-m gpu: every op of the real plans, run alone through libmdx (ops.run_ops) and judged at kernel-level tolerance against fp64 on the inputs
it actually received (tests/op_parity.py: values, finite, borders, inputs, no op skipped).

The kernel tests hold every kernel to helpers.close() on descriptors built by hand; the descriptors the engine lowers were judged only through
whole networks at 2-3 % per pass.  Here the same criterion meets the production forms where they exist: at TINY width every op of every plan
in both 16-bit types, at SD-1.5 width the sampler plan (fused q/k/v with V^T, fused LayerNorm from given statistics, GEGLU, step-selected
temb rows, channel-slice outputs) part by part, and the VAE plans at 224 x 400.  Each case writes one `op_parity:<plan>:<part>:<type>` line to
the parity log: op count, worst err / tol and worst rel L2 with their ops, the kernel tags seen."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import op_parity as P
from helpers import cfg_inputs, given_view_inputs, parity_log, scene, state_dicts
from magicdrive_amd import _lib as L, denoiser as DN, ops as O, schedulers
from magicdrive_amd.engine import PackedNet
from magicdrive_amd.networks import spec
from magicdrive_amd.text_encoder import TextEncoderPlan
from magicdrive_amd.vae import VaeDecodePlan, VaeEncodePlan
from oracle import denoiser as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16]
KIND = {torch.bfloat16: "bf16", torch.float16: "f16"}
HW = (28, 50)


def execute(op):
    O.run_ops([op])


def last_kernel():
    return (L.lib().mdx_last_kernel() or b"").decode()


def judged(plan, part, dtype, recs, expect):
    assert len(recs) == expect, (plan, part, len(recs), expect)
    s = P.summary(recs)
    parity_log(f"op_parity:{plan}:{part}:{KIND[dtype]}", **s)
    print(f"[op_parity {plan} {part} {KIND[dtype]}] {s}")
    return s


class Nets:
    """Seeded weights of one config, packed once per 16-bit type (module scope: the plans below share them)."""

    def __init__(self, cfg, dev):
        self.cfg, self.dev = cfg, dev
        self.usd, self.csd = state_dicts(cfg)
        self.packed = {}

    def __call__(self, dtype):
        if dtype not in self.packed:
            self.packed[dtype] = (PackedNet(self.usd, self.dev, dtype), PackedNet(self.csd, self.dev, dtype))
        return self.packed[dtype]


@pytest.fixture(scope="module")
def tiny(dev):
    return Nets(spec.TINY_CONFIG, dev)


@pytest.fixture(scope="module")
def sd15(dev):
    yield Nets(spec.SD15_CONFIG, dev)
    _plans.clear()                            # the SD-1.5 plan's buffers go with the module


def sampler(nets, dtype, b, do_cfg, L_box, steps=2, sched="ddim", given=0, **kw):
    cfg, dev = nets.cfg, nets.dev
    un, cn = nets(dtype)
    sc = scene(cfg, b, L_box, HW)
    sch = schedulers.DDIMScheduler() if sched == "ddim" else schedulers.UniPCMultistepScheduler()
    ts = sch.set_timesteps(steps)
    if do_cfg:
        cam, text, bev, boxes = cfg_inputs(D, nets.csd, sc)
    else:
        cam, text, bev, boxes = sc["camera_param"], sc["prompt_embeds"], sc["bev_map"], sc["bboxes_3d_data"]
    sp = DN.SamplerPlan(cfg, un, cn, dev, b, do_cfg, L_box, HW, num_steps=steps, guidance_scale=2.0, scheduler_kind=sched, given_view_mode=given, **kw)
    gv = {}
    if given:
        cl = given_view_inputs(HW)[:b]
        lat = torch.zeros(b, 6, 4, *HW)
        for i, r in enumerate(cl):
            for j, v in enumerate(r):
                if v is not None:
                    lat[i, j] = v
        gv = dict(given_mask=torch.tensor([[v is not None for v in r] for r in cl]), given_latents=lat)
    sp.load_inputs(torch.stack([sc["latents"]] * 6, 1), cam, text, bev, boxes, ts, sch.coefficient_table(), **gv)
    return sp


# ---- TINY width: every op of every plan, both 16-bit types ----------------------------------------------------------------------------------
TINY_SAMPLERS = {
    "cfg_fork_trace": dict(b=1, do_cfg=True, fork=True, health="trace"),
    "unipc_given1": dict(b=1, do_cfg=True, sched="unipc", given=1),
    "scene_boxes_b2": dict(b=2, do_cfg=False, dynamic_boxes="scene"),
    # kept regions (one ops.LatentBlend behind the scheduler op), resampling (one jump program, launched between the two steps) and
    # stochastic DDIM (ops.DdimEtaStep in the scheduler op's place): built and loaded as tests/call_state.py does, CFG on
    "regions_unipc": dict(call_state=dict(do_cfg=True, sched="unipc", given=1, keep_regions=True)),
    "regions_resample": dict(call_state=dict(do_cfg=True, given=1, keep_regions=True, resample=1)),
    "eta_regions_resample": dict(call_state=dict(do_cfg=True, given=1, keep_regions=True, resample=1, stochastic=True)),
}
NEW_KERNELS = {"regions_unipc": ("blend_kernel",), "regions_resample": ("blend_kernel", "renoise_kernel"),
               "eta_regions_resample": ("blend_kernel", "renoise_kernel", "ddim_eta_kernel")}


def call_state_sampler(nets, dtype, which):
    import call_state as CS
    un, cn = nets(dtype)
    four = (nets.cfg, nets.csd, un, cn)
    sp = CS.build_plan(four, which, nets.dev)
    args, kw = CS.inputs(four, which, "B")
    sp.load_inputs(*args, **kw)
    return sp


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("which", list(TINY_SAMPLERS))
def test_tiny_sampler_plan_every_op(dev, tiny, which, dtype):
    how = TINY_SAMPLERS[which]
    sp = call_state_sampler(tiny, dtype, how["call_state"]) if "call_state" in how else sampler(tiny, dtype, L_box=5, **how)
    walk = lambda ops: P.walk(ops, execute, kernel=last_kernel, plan="tiny." + which)
    recs = walk(sp.prologue_ops) + walk(sp.step_ops)
    if sp.jump_ops:                           # step 0, one jump back to it, step 0 again: the jump op is walked too
        recs += walk(sp.jump_ops)
        assert (sp.step_ctr.item(), sp.visit_ctr.item()) == (0, 1)
    recs += walk(sp.step_ops)
    assert sp.step_ctr.item() == 2 - len(sp.jump_ops)
    s = judged("tiny." + which, "all", dtype, recs, len(sp.prologue_ops) + 2 * len(sp.step_ops) + len(sp.jump_ops))
    for tag in NEW_KERNELS.get(which, ()):
        assert any(k.startswith(tag) for k in s["kernels"]), (tag, s["kernels"])


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_sdpa_program_every_op(dev, dtype):
    """A program that holds ops.Sdpa, at the shapes of tests/test_sdpa_gpu.py::test_program_executor, plus its causal and key-count forms."""
    B, H, d, Tq, Tk = 2, 3, 80, 33, 65
    g = torch.Generator(device="cuda").manual_seed(9)
    q, k, v, k2, v2 = (torch.randn(B, T, H * d, generator=g, device="cuda").to(dtype) for T in (Tq, Tk, Tk, Tq, Tq))
    new = lambda: torch.zeros(B, Tq, H * d, dtype=dtype, device=dev)
    prog = [O.Sdpa(q, k, v, new(), heads=H, scale=d ** -0.5, name="sdpa"),
            O.Sdpa(q, k2, v2, new(), heads=H, scale=d ** -0.5, causal=True, name="sdpa.causal"),
            O.Sdpa(q, k, v, new(), heads=H, scale=d ** -0.5, klen=torch.tensor([Tk, 7], dtype=torch.int32, device=dev), name="sdpa.klen")]
    s = judged("sdpa.program", "all", dtype, P.walk(prog, execute, kernel=last_kernel, plan="sdpa.program"), len(prog))
    assert all(k.startswith("attn_vrow_kernel<") for k in s["kernels"]), s["kernels"]


def test_composite_program_every_op(dev):
    """A program that holds ops.ImageComposite, at the shapes of tests/test_composite_gpu.py::test_program_path, with and without the matte."""
    import composite_cases as CC
    from test_composite_gpu import operands
    ci, r = 0, 1
    gen, orig = (t.to(dev) for t in operands(ci, "bf16"))
    keep = CC.keep_mask(ci).to(dev)
    V, _, H, W = gen.shape
    out = lambda: torch.zeros(V, H, W, 3, device=dev)
    prog = [O.ImageComposite(gen, orig, keep, out(), r, name="composite"),
            O.ImageComposite(gen, orig, keep, out(), r, matte=torch.zeros(V, H, W, device=dev), has=torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev), name="composite.matte+has")]
    s = judged("composite.program", "all", torch.bfloat16, P.walk(prog, execute, kernel=last_kernel, plan="composite.program"), len(prog))
    assert all(k.startswith("composite_kernel") for k in s["kernels"]), s["kernels"]


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_tiny_controlnet_and_unet_plans_every_op(dev, tiny, dtype):
    cfg = tiny.cfg
    un, cn = tiny(dtype)
    sc = scene(cfg, 2, 5, HW)
    lat = torch.randn(2, 6, 4, *HW, generator=torch.Generator().manual_seed(7))
    t = torch.tensor([981.0, 501.0]).repeat_interleave(6)
    cp = DN.ControlNetPlan(cfg, cn, dev, 2, 5, HW)
    cp.sample_nchw.copy_(lat.reshape(-1, 4, *HW)); cp.temb.t.copy_(t)
    cp.cond.load(sc["camera_param"], sc["prompt_embeds"], sc["bev_map"], sc["bboxes_3d_data"])
    judged("tiny.controlnet", "all", dtype, P.walk(cp.ops, execute, kernel=last_kernel, plan="tiny.controlnet"), len(cp.ops))
    up = DN.UNetPlan(cfg, un, dev, 12, cp.cond.ctx.shape[1], HW)
    up.sample_nchw.copy_(lat.reshape(-1, 4, *HW)); up.temb.t.copy_(t); up.ctx.copy_(cp.cond.ctx)
    for dst, src in zip(up.res_in, cp.down_out):
        dst.copy_(src)
    up.mid_in.copy_(cp.mid_out)
    judged("tiny.unet", "all", dtype, P.walk(up.ops, execute, kernel=last_kernel, plan="tiny.unet"), len(up.ops))


def vae_plans(vcfg, dev, dtype, n, latent_hw, seed=11):
    sd = spec.random_state_dict(spec.vae_decoder_param_shapes(vcfg), seed)
    sd.update(spec.random_state_dict(spec.vae_encoder_param_shapes(vcfg), seed + 1000))
    net = PackedNet(sd, dev, dtype)
    h, w = latent_hw
    dec = VaeDecodePlan(vcfg, net, dev, n, latent_hw)
    dec.z_in.copy_(torch.randn(n, 4, h, w, generator=torch.Generator().manual_seed(2)) * 0.8)
    enc = VaeEncodePlan(vcfg, net, dev, n, (8 * h, 8 * w))
    enc.x_in.copy_(torch.rand(n, 3, 8 * h, 8 * w, generator=torch.Generator().manual_seed(3)) * 2 - 1)
    return dec, enc


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_tiny_vae_plans_every_op(dev, dtype):
    dec, enc = vae_plans(spec.VAE_TINY_CONFIG, dev, dtype, 2, (7, 13))
    judged("tiny.vae_decode", "all", dtype, P.walk(dec.ops, execute, kernel=last_kernel, plan="tiny.vae_decode"), len(dec.ops))
    judged("tiny.vae_encode", "all", dtype, P.walk(enc.ops, execute, kernel=last_kernel, plan="tiny.vae_encode"), len(enc.ops))


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_tiny_text_encoder_plan_every_op(dev, dtype):
    g = torch.load(os.path.join(ROOT, "tests", "golden", "clip_text_tiny.pt"))
    sd = {k: v.float() for k, v in g["state_dict"].items()}
    ids = g["input_ids"]
    plan = TextEncoderPlan(g["config"], PackedNet(sd, dev, dtype), dev, ids.shape[0], ids.shape[1])
    plan.ids.copy_(ids.reshape(-1))
    recs = P.walk(plan.ops, execute, kernel=last_kernel, plan="tiny.text_encoder")
    judged("tiny.text_encoder", "all", dtype, recs, len(plan.ops))
    assert any(r.cls == "Attn" and "short" in r.kernel for r in recs), sorted({r.kernel for r in recs})


# ---- SD-1.5 width -----------------------------------------------------------------------------------------------------------------------------
SD15_PLANS = {
    "sd15": (dict(b=1, do_cfg=False, fork=True), DTYPES),
    "sd15.cfg_dynamic": (dict(b=1, do_cfg=True, fork=True, dynamic_boxes=True), [torch.bfloat16]),
}
PARTS = ("prologue", "controlnet", "unet_encoder", "tail")
_plans = {}


def sd15_plan(nets, which, dtype):
    """One plan per (configuration, type), built once; every case reloads the inputs (a fresh trajectory: step counter zero)."""
    key = (which, dtype)
    if key not in _plans:
        _plans.clear()                        # one SD-1.5 plan's buffers at a time
        _plans[key] = sampler(nets, dtype, L_box=32, **SD15_PLANS[which][0])
    return _plans[key]


def carries_step_state(op):
    return any(getattr(op, f, None) is not None for f in ("sel", "step", "row"))


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("which,dtype", [(w, dt) for w, (_, dts) in SD15_PLANS.items() for dt in dts],
                         ids=[f"{w}-{KIND[dt]}" for w, (_, dts) in SD15_PLANS.items() for dt in dts])
def test_sd15_sampler_plan_part(dev, sd15, which, dtype, part):
    """Each case runs the parts before its own unjudged and judges its own: every op in step 1, in step 2 the ops that read the step counter
    (sel, step, row) — the only ones whose descriptor addresses something else than in step 1."""
    sp = sd15_plan(sd15, which, dtype)
    kw = SD15_PLANS[which][0]
    sc = scene(sd15.cfg, 1, 32, HW)
    sch = schedulers.DDIMScheduler(); ts = sch.set_timesteps(2)
    cam, text, bev, boxes = cfg_inputs(D, sd15.csd, sc) if kw["do_cfg"] else (sc["camera_param"], sc["prompt_embeds"], sc["bev_map"], sc["bboxes_3d_data"])
    sp.load_inputs(torch.stack([sc["latents"]] * 6, 1), cam, text, bev, boxes, ts, sch.coefficient_table())
    a, b = sp.fork_at
    n = len(sp.step_ops)
    lo, hi = {"prologue": (0, 0), "controlnet": (0, a), "unet_encoder": (a, b), "tail": (b, n)}[part]
    walk = lambda ops, compare: P.walk(ops, execute, compare=compare, kernel=last_kernel, plan=which)
    recs = walk(sp.prologue_ops, all if part == "prologue" else ())
    expect = len(sp.prologue_ops) if part == "prologue" else 0
    if part != "prologue":
        recs += walk(sp.step_ops, range(lo, hi))
        second = [i for i in range(lo, hi) if carries_step_state(sp.step_ops[i])]
        assert second, "every part of a step has ops that read the step counter"
        recs += walk(sp.step_ops, second)
        expect = (hi - lo) + len(second)
        assert sp.step_ctr.item() == 2
    s = judged(which, part, dtype, recs, expect)
    if part == "unet_encoder":                # the forms that exist only at this width were really judged
        ops = sp.step_ops[lo:hi]
        assert any(isinstance(op, O.Gemm) and op.Vt is not None for op in ops)
        assert any(isinstance(op, O.Gemm) and op.ln_eps > 0 and op.ln_stats is not None for op in ops)
        assert any(isinstance(op, O.Gemm) and op.rowstat is not None for op in ops)
        assert any(isinstance(op, O.Gemm) and op.epilogue == L.EPI_GEGLU for op in ops)
        assert any(isinstance(op, O.Conv) and op.sel is not None for op in ops)
    if which == "sd15.cfg_dynamic" and part != "prologue":
        assert any(isinstance(op, O.Attn) and op.tk_dev is not None for op in sp.step_ops[lo:hi])


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("which", ["decode", "encode"])
def test_sd15_vae_plan_half(dev, which, half):
    dtype = torch.bfloat16
    dec, enc = vae_plans(spec.VAE_SD15_CONFIG, dev, dtype, 1, HW)
    ops = dec.ops if which == "decode" else enc.ops
    mid = len(ops) // 2
    chosen = range(0, mid) if half == 0 else range(mid, len(ops))
    recs = P.walk(ops, execute, compare=chosen, kernel=last_kernel, plan="sd15.vae_" + which)
    judged("sd15.vae_" + which, f"half{half}", dtype, recs, len(chosen))


def test_walker_sees_seeded_faults_on_the_device(dev, tiny):
    """The conditions are proven against seeded faults on the CPU (tests/test_op_parity_cpu.py); this repeats two of them with libmdx as the
    executor, so the device path of the walker (snapshots, storages, fp64 on the GPU) is known to see an error too: one 16 x 16 block of a
    GEMM output zeroed, and one element written one column past a channel-slice output.  Each fails at its op and nowhere else."""
    sp = sampler(tiny, torch.bfloat16, b=1, do_cfg=True, L_box=5, fork=True)
    ops = sp.step_ops
    block = next(i for i, op in enumerate(ops) if isinstance(op, O.Gemm) and op.name.endswith("ff.out"))
    spill = next(i for i, op in enumerate(ops) if isinstance(op, O.Gemm) and op.name == "zero_conv.1" and op.C.stride(0) > op.C.shape[1])
    index_of = {id(op): i for i, op in enumerate(ops)}

    def faulty(op):
        O.run_ops([op])
        i = index_of[id(op)]
        if i == block:
            op.C[16:32, 16:32] = 0
        elif i == spill:
            C = op.C
            torch.as_strided(C, (1,), (1,), C.storage_offset() + 3 * C.stride(0) + C.shape[1]).add_(1.0)

    P.walk(sp.prologue_ops, execute, compare=())
    recs = P.walk(ops, faulty, kernel=last_kernel, plan="tiny.faults", stop=False)
    failed = {r.index: {f.condition for f in r.failures} for r in recs if r.failures}
    assert failed == {block: {"values"}, spill: {"borders"}}, failed
