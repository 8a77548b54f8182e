"""CPU: one sampler plan for a bucket of box counts — the host-side contract of MdxAttnDesc.tk_dev (through the loaded library; the checks run
before any launch), the lowering of a dynamic SamplerPlan, ConditioningBuffers.load at a capacity, and the pipeline's bucket arithmetic.
The kernel itself is tests/test_attn_ctx_gpu.py; the plan on the GPU is tests/test_box_bucket_gpu.py."""
import ctypes
import dataclasses
import os
import types

import pytest
import torch

import plan_interp
from helpers import cfg_inputs, rel_l2, scene, state_dicts
from magicdrive_amd import _lib as L, denoiser as DN, ops as O, schedulers
from magicdrive_amd.engine import PackedNet
from magicdrive_amd.networks import spec
from oracle import denoiser as D

CPU = torch.device("cpu")
MDX_OK, MDX_EINVAL, MDX_EUNSUPPORTED = 0, -1, -3


# ---- descriptor contract ---------------------------------------------------------------------------------------------------------
class _Host:
    """A 64-byte aligned host block: the checks below return before anything is launched, so no pointer is ever dereferenced."""

    def __init__(self):
        self.buf = (ctypes.c_char * 8192)()
        self.base = (ctypes.addressof(self.buf) + 63) // 64 * 64


def _desc(h, **kw):
    d = L.MdxAttnDesc()
    d.Q = d.K = d.Vt = d.O = h.base
    d.tk_dev = h.base + 4096
    d.B, d.H, d.Tq, d.Tk, d.d, d.nsrc = 1, 1, 0, 8, 16, 1          # Tq = 0: a descriptor that passes every check launches nothing
    d.ldq = d.ldk = d.ldo = 16
    d.ldv = 8
    d.sQ = d.sK = d.sV = d.sO = 128
    d.scale = 0.25
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(d, entry="mdx_attention_bf16"):
    rc = getattr(L.lib(), entry)(ctypes.byref(d), None)
    return rc, (L.lib().mdx_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ["mdx_attention_bf16", "mdx_attention_f16"])
def test_tk_dev_descriptor_contract(entry):
    h = _Host()
    assert _call(_desc(h), entry)[0] == MDX_OK                                   # Tq = 0
    assert _call(_desc(h, q_prescaled=1), entry)[0] == MDX_OK
    for field, bad in (("nsrc", 2), ("joint", 1), ("causal", 1), ("v_rowmajor", 1)):
        kw = {field: bad}
        if field == "nsrc":
            kw["kvmap"] = h.base
        rc, msg = _call(_desc(h, **kw), entry)
        assert rc == MDX_EINVAL and "tk_dev" in msg and field in msg and entry in msg, (field, rc, msg)
    rc, msg = _call(_desc(h, d=48), entry)
    assert rc == MDX_EUNSUPPORTED and "d=48" in msg, (rc, msg)
    for dd in (16, 32, 40, 80, 160):
        assert _call(_desc(h, d=dd, ldq=dd, ldk=dd, ldo=dd), entry)[0] == MDX_OK
    rc, msg = _call(_desc(h, tk_dev=h.base + 4098), entry)
    assert rc == MDX_EINVAL and "tk_dev" in msg and "aligned" in msg, (rc, msg)
    rc, msg = _call(_desc(h, ldv=0), entry)                                     # Tk is the capacity: ldv >= Tk still holds
    assert rc == MDX_EINVAL and "ldv" in msg, (rc, msg)
    for bad_scale in (0.0, -0.25, float("nan")):                                  # the maximum is taken of raw scores: scale must be positive
        rc, msg = _call(_desc(h, scale=bad_scale), entry)
        assert rc == MDX_EINVAL and "scale" in msg, (bad_scale, rc, msg)
        assert _call(_desc(h, scale=bad_scale, q_prescaled=1), entry)[0] == MDX_OK       # ignored with q_prescaled
    rc, msg = _call(_desc(h, Vt=h.base + 8), entry)                             # alignment as for the V^T form
    assert rc == MDX_EINVAL and "Vt" in msg, (rc, msg)
    # tk_dev == NULL: the old contract, e.g. causal without v_rowmajor is refused by the short-sequence entry as before
    rc, msg = _call(_desc(h, tk_dev=None, causal=1), entry)
    assert rc == MDX_EINVAL and "tk_dev" not in msg


def test_attn_desc_layout_unchanged():
    names = [f[0] for f in L.MdxAttnDesc._fields_]
    assert names == "Q K Vt O kvmap tk_dev B H Tq Tk d nsrc ldq sQ ldk sK ldv sV ldo sO scale joint q_prescaled causal v_rowmajor".split()
    assert ctypes.sizeof(L.MdxAttnDesc) == 25 * 8 and L.MdxAttnDesc.tk_dev.offset == 40 and L.MdxAttnDesc.B.offset == 48
    from magicdrive_amd.integration import attn_processor as AP
    assert [f[0] for f in AP.MdxAttnDesc._fields_] == names and ctypes.sizeof(AP.MdxAttnDesc) == 200
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdx.h")).read()
    body = hdr[hdr.index("typedef struct MdxAttnDesc {"):hdr.index("} MdxAttnDesc;")]
    assert "const int32_t* kvmap; const int32_t* tk_dev;" in body and "reserved_p" not in body.split("/*")[0]
    assert L.ABI_VERSION == 12 and L.lib().mdx_abi_version() == 12


# ---- op layer ---------------------------------------------------------------------------------------------------------------------
def test_attn_op_lowers_and_validates_tk_dev():
    B, T, S, C = 2, 9, 16, 32
    q = torch.zeros(B, T, C, dtype=torch.bfloat16); k = torch.zeros(B, S, C, dtype=torch.bfloat16)
    vt = torch.zeros(B, C, S, dtype=torch.bfloat16); o = torch.zeros_like(q)
    live = torch.tensor([11], dtype=torch.int32)
    _, d = O.Attn(q, k, vt, o, heads=2, Tk=S, scale=0.25, tk_dev=live).lower()
    assert d.tk_dev == live.data_ptr() and d.Tk == S
    _, d0 = O.Attn(q, k, vt, o, heads=2, Tk=S, scale=0.25).lower()
    assert not d0.tk_dev
    for bad in (torch.tensor([11], dtype=torch.int64), torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError):
            O.Attn(q, k, vt, o, heads=2, Tk=S, scale=0.25, tk_dev=bad).lower()
    with pytest.raises(ValueError):
        O.Attn(q, k, vt, o, heads=2, Tk=S, scale=0.25, tk_dev=live, kvmap=torch.zeros(2 * B, dtype=torch.int32), nsrc=2).lower()


# ---- plan -------------------------------------------------------------------------------------------------------------------------
def run_dynamic(ops, lower_check=True):
    """tests/plan_interp.py knows nothing of tk_dev: an op that carries it is interpreted as the attention over its first tk_dev[0] keys."""
    for op in ops:
        if isinstance(op, O.Attn) and op.tk_dev is not None:
            if lower_check:
                op.lower()
            n = int(op.tk_dev.item())
            assert 1 <= n <= op.Tk
            plan_interp.run([dataclasses.replace(op, K=op.K[:, :n], Tk=n, tk_dev=None)], lower_check=False)
        else:
            plan_interp.run([op], lower_check=lower_check)


@pytest.fixture(scope="module")
def tiny():
    cfg = spec.TINY_CONFIG
    usd, csd = state_dicts(cfg)
    return cfg, usd, csd, PackedNet(usd, CPU), PackedNet(csd, CPU)


@pytest.mark.parametrize("fork", [False, True])
def test_dynamic_plan_carries_tk_dev_on_the_context_attention_only(tiny, fork):
    cfg, usd, csd, un, cn = tiny
    sp = DN.SamplerPlan(cfg, un, cn, CPU, 1, True, 8, (28, 50), num_steps=2, fork=fork, dynamic_boxes=True)
    ex = DN.SamplerPlan(cfg, un, cn, CPU, 1, True, 8, (28, 50), num_steps=2, fork=fork)
    assert sp.cond.live.dtype == torch.int32 and sp.cond.live.numel() == 1
    assert not any(getattr(op, "tk_dev", None) is not None for op in sp.prologue_ops)
    attn = [op for op in sp.step_ops if isinstance(op, O.Attn)]
    ctx_attn = [op for op in attn if op.name.endswith(".attn2")]
    assert ctx_attn and len(ctx_attn) < len(attn)
    for op in attn:
        if op.name.endswith(".attn2"):
            assert op.tk_dev is sp.cond.live and op.Tk == 1 + 77 + 8 and op.nsrc == 1
            assert op.lower()[1].tk_dev == sp.cond.live.data_ptr()
        else:                                   # self and cross-view attention are untouched
            assert op.tk_dev is None and not op.lower()[1].tk_dev
    if fork:                                    # both branches of a forked plan (ControlNet | UNet encoder) and the tail hold context attentions
        a, b = sp.fork_at
        for part in (sp.step_ops[:a], sp.step_ops[a:b], sp.step_ops[b:]):
            assert any(isinstance(op, O.Attn) and op.tk_dev is sp.cond.live for op in part)
    # the exact plan is the same program without the field
    assert [type(op).__name__ + ":" + getattr(op, "name", "") for op in ex.step_ops] == [type(op).__name__ + ":" + getattr(op, "name", "") for op in sp.step_ops]
    assert not any(getattr(op, "tk_dev", None) is not None for op in ex.prologue_ops + ex.step_ops)
    with pytest.raises(AssertionError):
        DN.SamplerPlan(cfg, un, cn, CPU, 1, True, 0, (28, 50), num_steps=2, dynamic_boxes=True)


def test_load_at_a_capacity_and_same_result_as_the_exact_plan(tiny):
    """A capacity-8 plan loaded with 5 (then 3) boxes: the live count, the masked-out tail slots, and — through the interpreter — the latents of
    the exact L = 5 plan after one step (positions < L are the same computation; the rows L .. capacity exist and are never attended to)."""
    cfg, usd, csd, un, cn = tiny
    steps = 1
    sch = schedulers.DDIMScheduler(); ts = sch.set_timesteps(steps)
    outs = {}
    dyn = DN.SamplerPlan(cfg, un, cn, CPU, 1, True, 8, (28, 50), num_steps=steps, guidance_scale=2.0, dynamic_boxes=True)
    for Lb in (5, 3):
        sc = scene(cfg, 1, Lb)
        cam, text, bev, boxes = cfg_inputs(D, csd, sc)
        lat6 = torch.stack([sc["latents"]] * 6, 1)
        dyn.load_inputs(lat6, cam, text, bev, boxes, ts, sch.coefficient_table())
        assert dyn.cond.live.item() == 1 + 77 + Lb
        m = dyn.cond.box_mask.view(12, 8)
        assert not m[:, Lb:].any() and m[6:, :Lb].any() and dyn.cond.box_mask.sum().item() == boxes["masks"].expand(2, 6, Lb).sum().item()
        run_dynamic(dyn.prologue_ops)
        assert torch.isfinite(dyn.cond.ctx.float()).all()
        run_dynamic(dyn.step_ops)
        ex = DN.SamplerPlan(cfg, un, cn, CPU, 1, True, Lb, (28, 50), num_steps=steps, guidance_scale=2.0)
        ex.load_inputs(lat6, cam, text, bev, boxes, ts, sch.coefficient_table())
        plan_interp.run(ex.prologue_ops)
        plan_interp.run(ex.step_ops, lower_check=False)
        assert rel_l2(dyn.cond.ctx[:, :78 + Lb], ex.cond.ctx) < 1e-3, "context rows < L differ from the exact plan's"
        e = rel_l2(dyn.latents(), ex.latents())
        assert e < 1e-3, (Lb, e)          # same arithmetic on the same rows; only the CPU matmul's blocking may differ with M
        outs[Lb] = dyn.latents().clone()
    assert not torch.equal(outs[5], outs[3])
    # too many boxes for the capacity, and the exact plan's own assert, stay loud
    big = scene(cfg, 1, 9)
    cam, text, bev, boxes = cfg_inputs(D, csd, big)
    with pytest.raises(AssertionError):
        dyn.load_inputs(torch.stack([big["latents"]] * 6, 1), cam, text, bev, boxes, ts, sch.coefficient_table())
    with pytest.raises(AssertionError):
        ex.load_inputs(torch.stack([big["latents"]] * 6, 1), cam, text, bev, boxes, ts, sch.coefficient_table())


# ---- pipeline key arithmetic --------------------------------------------------------------------------------------------------------
def test_bucket_capacities_and_unchanged_default():
    from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    from magicdrive_amd.networks.unet_addon_rawbox import BEVControlNetModel
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline as P
    cfg = spec.TINY_CONFIG
    pipe = P(unet=UNet2DConditionModelMultiview.from_config(cfg, 0), controlnet=BEVControlNetModel.from_config(cfg, 1))
    assert pipe.box_bucket is None                       # the default: exact plans
    # (plan box count, dynamic, the box entry of the plan key); the entry is the int L_box itself — today's key — whenever the plan is exact
    assert [pipe._box_plan_geometry(Lb) for Lb in (0, 5, 9)] == [(0, False, 0), (5, False, 5), (9, False, 9)]
    assert all(type(pipe._box_plan_geometry(Lb)[2]) is int for Lb in (0, 5, 9))
    pipe.box_bucket = 8
    assert [pipe._box_plan_geometry(Lb)[:2] for Lb in (1, 7, 8, 9)] == [(8, True), (8, True), (8, True), (16, True)]
    assert pipe._box_plan_geometry(9)[2] == (16, "dynamic") and pipe._box_plan_geometry(7)[2] == pipe._box_plan_geometry(1)[2] != 8
    assert pipe._box_plan_geometry(0) == (0, False, 0)   # no boxes: its own exact plan, today's key
    geo = lambda bucket, Lb: P._box_plan_geometry(types.SimpleNamespace(box_bucket=bucket), Lb)
    assert geo(1, 5)[:2] == (5, True) and geo(16, 17)[:2] == (32, True)
    for bad in (0, -8, 2.5, True):
        with pytest.raises(ValueError):
            geo(bad, 5)
