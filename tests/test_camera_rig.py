"""CPU: camera rigs that are not a ring — neighboring_view_pair with 0, 1 or 2 neighbours per view in the default `add` mode
(BasicMultiviewTransformerBlock._construct_attn_input, blocks.py:106-121: one attention per (view, neighbour) pair of WHATEVER list a view
has; :213-217 sums per view what came back, zeros for an empty list).

Goldens: tests/golden/tiny_forward_rig.pt (tools/make_golden.py rig), the REAL reference UNet on
  chain5  {0:[1], 1:[0,2], 2:[1,3], 3:[2,4], 4:[3]}   a five-camera open chain: the end cameras have one neighbour
  asym3   {0:[1,2], 1:[0], 2:[]}                      an empty list; not symmetric under any relabelling of the views
Neither rig is symmetric the way the six-camera ring is, so a wrong neighbour index shows.
"""
import ctypes
import hashlib
import json
import os

import pytest
import torch

import plan_interp
from helpers import rel_l2, scene, state_dicts
from magicdrive_amd import denoiser as DN, engine, flops, ops as O
from magicdrive_amd.engine import PackedNet
from magicdrive_amd.networks import spec
from magicdrive_amd.networks.base import arch_config_from_json
from magicdrive_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
from oracle import denoiser as D

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CPU = torch.device("cpu")
HW = (28, 50)


def rig_cfg(rig, **kw):
    cfg = dict(spec.TINY_CONFIG)
    cfg["neighboring_view_pair"] = {int(k): list(v) for k, v in rig.items()}
    cfg.update(kw)
    return cfg


def mirrored(rig):
    """The rig with the views relabelled v -> n-1-v."""
    n = len(rig)
    return {n - 1 - k: [n - 1 - x for x in v] for k, v in rig.items()}


@pytest.fixture(scope="module")
def tiny():
    usd, csd = state_dicts(spec.TINY_CONFIG)
    return usd, csd, PackedNet(usd, CPU), torch.load(os.path.join(GOLD, "tiny_forward_rig.pt"))


def rig_inputs(G, name, csd):
    """Inputs of one rig of the fixture and the (oracle) ControlNet outputs the UNet consumes: the ControlNet has no cross-view attention."""
    rig = G["rigs"][name]
    n = len(rig)
    cfg = rig_cfg(rig)
    sc = scene(cfg, 1, G["boxes"], HW, seed=G["scene_seed"], n_cam=n)
    lat = torch.randn(1, n, 4, *HW, generator=torch.Generator().manual_seed(G["lat_seed"][name]))
    t = G["timesteps"][name]
    with torch.no_grad():
        d, m, ctx = D.controlnet_forward(csd, cfg, lat, t, sc["camera_param"], sc["bboxes_3d_data"], sc["prompt_embeds"], sc["bev_map"])
    return cfg, n, lat, t, d, m, ctx


@pytest.fixture(scope="module")
def inputs(tiny):
    usd, csd, un, G = tiny
    return {name: rig_inputs(G, name, csd) for name in G["rigs"]}


# ---------------------------------------------------------------- the plan interpreter's attention, with absent sources
def run_attn_rig(op: O.Attn):
    """plan_interp.run_attn for a kv map with absent slots (include/mdx.h: joint == 0, kvmap[b * nsrc + s] < 0 = query batch b has no source
    in slot s; O = sum over the slots present, zeros when none is).  plan_interp.run_attn indexes the map with Python semantics: -1 would
    silently read the last view."""
    if op.kvmap is None or op.joint or not bool((op.kvmap < 0).any()):
        return plan_interp.run_attn(op)
    Q, K, Vt = op.Q.float(), op.K.float(), op.Vt.float()[:, :, :op.Tk]
    B, Tq, Cc = Q.shape
    H = op.heads
    d = Cc // H
    out = torch.zeros(B, Tq, Cc)
    kvmap = op.kvmap.view(B, op.nsrc)
    qh = Q.view(B, Tq, H, d).transpose(1, 2)
    sc = 0.6931471805599453 if op.q_prescaled else op.scale
    for b in range(B):
        for s in range(op.nsrc):
            kv = int(kvmap[b, s])
            if kv < 0:
                continue
            kh = K[kv].view(op.Tk, H, d).transpose(0, 1)
            vh = Vt[kv].transpose(0, 1).reshape(op.Tk, H, d).transpose(0, 1)
            att = torch.softmax(qh[b] @ kh.transpose(-1, -2) * sc, -1)
            out[b] += (att @ vh).transpose(0, 1).reshape(Tq, Cc)
    op.O.copy_(out.to(op.O.dtype))


def run_plan(ops):
    with torch.no_grad():
        for op in ops:
            op.lower()
            (run_attn_rig if isinstance(op, O.Attn) else plan_interp.DISPATCH[type(op)])(op)


def unet_plan(cfg, un, n, lat, t, d, m, ctx):
    up = DN.UNetPlan(cfg, un, CPU, n, ctx.shape[1], HW)
    up.sample_nchw.copy_(lat.reshape(-1, 4, *HW)); up.temb.t.copy_(t.float().repeat_interleave(n)); up.ctx.copy_(ctx)
    for dst, src in zip(up.res_in, d):
        dst.copy_(src)
    up.mid_in.copy_(m)
    return up


# ---------------------------------------------------------------- oracle and op graph vs the real reference
@pytest.mark.parametrize("name", ["chain5", "asym3"])
def test_oracle_matches_reference_on_rig(tiny, inputs, name):
    usd, csd, un, G = tiny
    cfg, n, lat, t, d, m, ctx = inputs[name]
    with torch.no_grad():
        e = D.unet_forward(usd, cfg, lat.reshape(-1, 4, *HW), t.repeat_interleave(n), ctx, d, m)
        e_mirror = D.unet_forward(usd, rig_cfg(mirrored(G["rigs"][name])), lat.reshape(-1, 4, *HW), t.repeat_interleave(n), ctx, d, m)
    assert rel_l2(e, G["eps_" + name].float()) < 2e-3          # golden eps stored as fp16
    if name == "asym3":                                        # (the chain is its own mirror image)
        assert rel_l2(e_mirror, G["eps_" + name].float()) > 1e-2


@pytest.mark.parametrize("name", ["chain5", "asym3"])
def test_unet_plan_matches_reference_on_rig(tiny, inputs, name):
    """The UNet op graph of a rig (kv map with absent slots, per-view out-bias table) in the CPU interpreter vs the real reference."""
    usd, csd, un, G = tiny
    cfg, n, lat, t, d, m, ctx = inputs[name]
    up = unet_plan(cfg, un, n, lat, t, d, m, ctx)
    run_plan(up.ops)
    per_view = max(rel_l2(up.out_nchw[i], G["eps_" + name][i].float()) for i in range(n))
    assert per_view < 3e-2, per_view
    if name == "asym3":                                        # view order: the mirrored rig misses the golden
        up2 = unet_plan(rig_cfg(mirrored(G["rigs"][name])), un, n, lat, t, d, m, ctx)
        run_plan(up2.ops)
        assert max(rel_l2(up2.out_nchw[i], G["eps_" + name][i].float()) for i in range(n)) > 2 * per_view


@pytest.mark.parametrize("mode", ["gated", "none"])
def test_unet_plan_rig_other_connectors_match_oracle(mode):
    """The per-view bias table of the gated / identity connector (PackedNet.gated_affine_rows): op graph vs the oracle on asym3."""
    cfg = rig_cfg({0: [1, 2], 1: [0], 2: []}, zero_module_type=mode)
    usd = spec.random_state_dict(spec.unet_param_shapes(cfg), 0)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(3, 4, *HW, generator=g)
    ctx = torch.randn(3, 9, cfg["cross_attention_dim"], generator=g)
    t = torch.tensor([300])
    with torch.no_grad():
        e = D.unet_forward(usd, cfg, lat, t.repeat_interleave(3), ctx)
    up = DN.UNetPlan(cfg, PackedNet(usd, CPU), CPU, 3, 9, HW, with_residuals=False)
    up.sample_nchw.copy_(lat); up.temb.t.copy_(t.float().repeat_interleave(3)); up.ctx.copy_(ctx)
    run_plan(up.ops)
    assert max(rel_l2(up.out_nchw[i], e[i]) for i in range(3)) < 3e-2


# ---------------------------------------------------------------- engine lowering
def xview_attn_ops(ops):
    return [op for op in ops if isinstance(op, O.Attn) and op.kvmap is not None]


def out_bias_gemms(ops):
    return [op for op in ops if isinstance(op, O.Gemm) and op.name.endswith(".attn4.out+connector")]


def plan_of(rig, n_scene=1, **kw):
    cfg = rig_cfg(rig, **kw)
    usd = spec.random_state_dict(spec.unet_param_shapes(cfg), 0)
    return cfg, usd, DN.UNetPlan(cfg, PackedNet(usd, CPU), CPU, n_scene * len(rig), 9, HW, with_residuals=False)


def test_chain5_lowers_to_two_slots_with_absent_ends():
    rig = {0: [1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3]}
    cfg, usd, up = plan_of(rig, n_scene=2)
    attn = xview_attn_ops(up.ops)
    assert attn
    want = [1, -1, 0, 2, 1, 3, 2, 4, 3, -1] + [6, -1, 5, 7, 6, 8, 7, 9, 8, -1]       # the second scene's views are 5..9
    for op in attn:
        assert op.nsrc == 2 and not op.joint and op.kvmap.tolist() == want
        _, d = op.lower()
        assert d.nsrc == 2 and d.joint == 0 and d.B == 10
    # FLOPs count the pairs attended: 8 of the 10 slots per scene
    op = attn[0]
    B, Tq, C = op.Q.shape
    assert flops.op_flops(op) == 4.0 * 16 * Tq * op.Tk * C


def test_out_bias_table_rows_are_count_times_bias():
    """Mixed counts: attn4's out-bias is an fp32 table [n_views][C] added per T rows, row v = W_c (count(v) b_o) + b_c; no bias vector."""
    rig = {0: [1, 2], 1: [0], 2: []}
    for mode in ("zero_linear", "gated"):
        cfg, usd, up = plan_of(rig, n_scene=2, zero_module_type=mode)
        gemms = out_bias_gemms(up.ops)
        assert gemms
        for op in gemms:
            pre = [k for k in usd if k.endswith("attn4.to_out.0.bias")]
            C = op.W.shape[0]
            T = op.A.shape[0] // 6
            assert op.bias is None and op.temb is not None and op.temb.dtype == torch.float32 and tuple(op.temb.shape) == (6, C)
            assert (op.rows_per_b, op.temb_b_stride, op.temb_sel_stride, op.sel, op.rowstat, op.Wq) == (T, C, 0, None, None, None)
            _, d = op.lower()
            assert (d.rows_per_b, d.temb_b_stride) == (T, C) and d.temb and not d.bias
            # which block this is: the one whose folded weight matches
            hit = 0
            for kb in pre:
                p = kb[:-len("attn4.to_out.0.bias")]
                bo, wo = usd[kb].float(), usd[p + "attn4.to_out.0.weight"].float()
                if wo.shape[0] != C:
                    continue
                if mode == "zero_linear":
                    wc, bc = usd[p + "connector.weight"].float(), usd[p + "connector.bias"].float()
                    w = wc @ wo
                    rows = [wc @ (c * bo) + bc for c in (2, 1, 0)]
                else:
                    gate = torch.tanh(usd[p + "connector.alpha"].float().reshape(-1))
                    w = gate[:, None] * wo
                    rows = [gate * bo * c for c in (2, 1, 0)]
                if not torch.equal(w.to(op.W.dtype), op.W):
                    continue
                hit += 1
                for v in range(6):
                    assert torch.allclose(op.temb[v], rows[v % 3], rtol=1e-6, atol=1e-7), (op.name, v)
                assert torch.equal(op.temb[2], op.temb[5]) and not torch.equal(op.temb[0], op.temb[1])
            assert hit == 1, op.name


def test_all_single_rig_lowers_to_one_source():
    """Every view has exactly one neighbour: one kv source per view, the out-bias once, as one vector."""
    cfg, usd, up = plan_of({0: [1], 1: [0]})
    for op in xview_attn_ops(up.ops):
        assert op.nsrc == 1 and op.kvmap.tolist() == [1, 0] and op.lower()[1].nsrc == 1
    for op in out_bias_gemms(up.ops):
        assert op.temb is None and op.bias is not None
    p = "down_blocks.0.attentions.0.transformer_blocks.0."
    want = usd[p + "connector.weight"].float() @ usd[p + "attn4.to_out.0.bias"].float() + usd[p + "connector.bias"].float()
    assert torch.allclose(out_bias_gemms(up.ops)[0].bias, want, rtol=1e-6, atol=1e-7)


def program_fingerprint(ops):
    """Per op: (type, name, sha1 of every non-pointer field of the lowered descriptor and of which pointers are set)."""
    out = []
    for op in ops:
        code, d = op.lower()
        rec = [int(code)]
        for fname, ftype in d._fields_:
            v = getattr(d, fname)
            if ftype is ctypes.c_void_p:
                rec.append([fname, v is not None and v != 0])
            elif isinstance(v, (int, float)):
                rec.append([fname, v])
            else:
                rec.append([fname, bytes(v).hex()])
        out.append([type(op).__name__, op.name, hashlib.sha1(json.dumps(rec).encode()).hexdigest()[:16]])
    return out


def ring_plan(n_scene=2):
    cfg = dict(spec.TINY_CONFIG)
    usd = spec.random_state_dict(spec.unet_param_shapes(cfg), 0)
    net = PackedNet(usd, CPU)
    up = DN.UNetPlan(cfg, net, CPU, 6 * n_scene, 9, HW, with_residuals=False)
    up.packed_storages = {t.untyped_storage().data_ptr() for t in net.cache.values()}       # what the plan reads of the packed weights
    return up


def test_six_ring_program_is_the_recorded_one():
    """The six-camera ring lowers to the op program recorded before camera rigs existed (tests/golden/ring6_program.json: type, name and a
    digest of every scalar descriptor field per op of the tiny UNet plan, two scenes)."""
    with open(os.path.join(GOLD, "ring6_program.json")) as f:
        want = json.load(f)
    got = program_fingerprint(ring_plan().ops)
    assert len(got) == len(want["ops"])
    for g, w in zip(got, want["ops"]):
        assert g == w, (g, w)


def test_six_ring_program_matches_uniform_two_neighbour_lowering(monkeypatch):
    """Descriptor for descriptor, weights included: the ring through the rig code path vs the lowering every view used to get (kv map of two
    sources per view without absent slots, 2 b_o folded through the connector as ONE bias vector)."""
    new = ring_plan()

    orig_init = engine.Builder.__init__

    def two_neighbour_init(self, cfg, device, n_views, n_cam, *a, **kw):
        orig_init(self, cfg, device, n_views, n_cam, *a, **kw)
        pair = {int(k): [int(x) for x in v] for k, v in cfg["neighboring_view_pair"].items()}
        assert all(len(v) == 2 for v in pair.values())
        kv = [(i // n_cam) * n_cam + nb for i in range(n_views) for nb in pair[i % n_cam]]
        self.kvmap = torch.tensor(kv, dtype=torch.int32, device=device)
        self.xv_nsrc, self.xv_counts, self.xv_bo_scale = 2, None, 2.0

    monkeypatch.setattr(engine.Builder, "__init__", two_neighbour_init)
    old = ring_plan()
    assert len(new.ops) == len(old.ops)
    assert program_fingerprint(new.ops) == program_fingerprint(old.ops)
    import dataclasses
    for a, b in zip(new.ops, old.ops):
        assert type(a) is type(b) and a.name == b.name
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, torch.Tensor):
                assert isinstance(y, torch.Tensor) and x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape) and x.stride() == y.stride(), (a.name, f.name)
                packed = x.untyped_storage().data_ptr() in new.packed_storages                  # packed weights / biases (activations are uninitialised)
                assert packed == (y.untyped_storage().data_ptr() in old.packed_storages), (a.name, f.name)
                if packed or f.name == "kvmap":
                    assert torch.equal(x, y), (a.name, f.name)
            else:
                assert x == y, (a.name, f.name)
    for op in xview_attn_ops(new.ops):
        B, Tq, C = op.Q.shape
        assert flops.op_flops(op) == 4.0 * B * Tq * op.Tk * C * op.nsrc


# ---------------------------------------------------------------- errors
def test_three_neighbours_in_add_mode_is_not_implemented():
    cfg = rig_cfg({0: [1, 2, 3], 1: [0], 2: [0], 3: [0]})
    with pytest.raises(NotImplementedError, match=r"view 0 lists 3 neighbours"):
        engine.Builder(cfg, CPU, 4, 4)


def test_ragged_concat_is_a_runtime_error():
    with pytest.raises(RuntimeError):
        engine.Builder(rig_cfg({0: [1], 1: [0, 2], 2: [1]}, neighboring_attn_type="concat"), CPU, 3, 3)
    engine.Builder(rig_cfg({0: [1], 1: [0]}, neighboring_attn_type="concat"), CPU, 2, 2)          # equal counts: served
    engine.Builder(rig_cfg({0: [1], 1: [0, 2], 2: []}, neighboring_attn_type="self"), CPU, 3, 3)   # self ignores the lists


def test_rig_without_any_neighbour_is_a_runtime_error():
    with pytest.raises(RuntimeError):                           # the reference: torch.cat of an empty list (blocks.py:119)
        engine.Builder(rig_cfg({0: [], 1: []}), CPU, 2, 2)


@pytest.mark.parametrize("rig", [{0: [1], 2: [0]}, {0: [1], 1: [2]}, {0: [1], 1: [-1]}, {1: [2], 2: [1]}])
def test_bad_rig_is_a_value_error_at_load(rig, tmp_path):
    with pytest.raises(ValueError, match="neighboring_view_pair"):
        UNet2DConditionModelMultiview.from_config(rig_cfg(rig), 0)
    with pytest.raises(ValueError, match="neighboring_view_pair"):
        arch_config_from_json({"neighboring_view_pair": {str(k): v for k, v in rig.items()}})
    with open(tmp_path / "config.json", "w") as f:
        json.dump({"neighboring_view_pair": {str(k): v for k, v in rig.items()}}, f)
    with pytest.raises(ValueError, match="neighboring_view_pair"):
        UNet2DConditionModelMultiview.from_pretrained(str(tmp_path))


def test_chain5_model_builds_a_plan():
    """from_config on the open chain, then the plan build: an AssertionError ("exactly 2 neighbours per view") before rigs were served."""
    cfg = rig_cfg({0: [1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3]})
    unet = UNet2DConditionModelMultiview.from_config(cfg, 0)
    up = DN.UNetPlan(unet.cfg, unet.packed(), CPU, 5, 9, HW, with_residuals=False)
    assert xview_attn_ops(up.ops) and all(op.temb is not None for op in out_bias_gemms(up.ops))
