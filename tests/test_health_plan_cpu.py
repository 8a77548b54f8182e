"""CPU: what SamplerPlan(health=...) and pipe.health do to the op programs and to the plan key (no kernel runs here; the records themselves are
tests/test_group_stats_gpu.py and tests/test_health_gpu.py).

  health=None    the prologue and step op lists are, op for op, those of a plan built without the argument;
  health="trace" exactly one op more per step program — an ops.GroupStats over the latents, behind the scheduler op, row-selected by the step
                 counter — and nothing else; in the forked form it is the last op of the tail part;
  health="final" nothing in the step program; one op of its own for run_health();
  the plan key   unchanged with the switch off, one trailing entry with it on.
tests/plan_interp.py does not know the op and is not run on a health-on plan.
"""
import pytest
import torch

from helpers import state_dicts
from magicdrive_amd import denoiser as DN, ops as O
from magicdrive_amd.engine import PackedNet
from magicdrive_amd.networks import spec

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


def signature(ops):
    """What an op list does, without its buffers' addresses: type, name, and shape / stride / dtype of every tensor field."""
    out = []
    for op in ops:
        t = tuple((k, tuple(v.shape), tuple(v.stride()), v.dtype) for k, v in sorted(vars(op).items()) if isinstance(v, torch.Tensor))
        s = tuple((k, v) for k, v in sorted(vars(op).items()) if isinstance(v, (int, float, str, bool, tuple)))
        out.append((type(op).__name__, t, s))
    return out


@pytest.mark.parametrize("kw", [{}, {"scheduler_kind": "unipc"}, {"fork": True}, {"dynamic_boxes": "scene"}], ids=["ddim", "unipc", "fork", "scene_boxes"])
def test_health_modes_change_only_what_they_say(nets, kw):
    base = plan(nets, **kw)
    off = plan(nets, health=None, **kw)
    assert signature(off.prologue_ops) == signature(base.prologue_ops) and signature(off.step_ops) == signature(base.step_ops)
    assert off.fork_at == base.fork_at and off.health_table() is None and off.health_ops == [] and base.health is None
    sched = "cfg+unipc" if kw.get("scheduler_kind") == "unipc" else "cfg+ddim"
    assert base.step_ops[-1].name == sched

    tr = plan(nets, health="trace", **kw)
    assert signature(tr.prologue_ops) == signature(base.prologue_ops)
    assert len(tr.step_ops) == len(base.step_ops) + 1 and signature(tr.step_ops[:-1]) == signature(base.step_ops)
    assert tr.fork_at == base.fork_at                      # forked: the extra op is the last one of the tail part
    last = tr.step_ops[-1]
    assert isinstance(last, O.GroupStats) and tr.step_ops[-2].name == sched and tr.health_ops == []
    assert last.row is tr.step_ctr and last.X.data_ptr() == tr.x.data_ptr() and tuple(last.X.shape) == (2 * 6, 28 * 50 * 4) and last.X.dtype == torch.float32
    # the scheduler op has advanced the counter before the record op runs: step s writes storage row s + 1 = row s of the table
    assert tuple(last.out.shape) == (STEPS + 1, 12, 4) and tuple(tr.health_table().shape) == (STEPS, 12, 4)
    assert tr.health_table().data_ptr() == last.out[1].data_ptr()
    code, d = last.lower()
    assert code == 16 and (d.G, d.n, d.sG, d.n_rows, d.f32) == (12, 5600, 5600, STEPS + 1, 1) and d.row_dev == tr.step_ctr.data_ptr() and d.out % 16 == 0

    fi = plan(nets, health="final", **kw)
    assert signature(fi.prologue_ops) == signature(base.prologue_ops) and signature(fi.step_ops) == signature(base.step_ops)
    assert len(fi.health_ops) == 1 and isinstance(fi.health_ops[0], O.GroupStats) and fi.health_ops[0].row is None
    assert fi.health_ops[0].X.data_ptr() == fi.x.data_ptr() and tuple(fi.health_table().shape) == (1, 12, 4)
    code, d = fi.health_ops[0].lower()
    assert (d.G, d.n, d.n_rows, d.row_dev) == (12, 5600, 1, None)


def test_load_inputs_zeroes_the_table(nets):
    from helpers import cfg_inputs, scene
    from magicdrive_amd import schedulers
    from oracle import denoiser as D
    cfg = nets[0]
    _, csd = state_dicts(cfg)
    tr = plan(nets, health="trace")
    tr._health.fill_(7.0)
    sc = scene(cfg, 2, 3)
    sch = schedulers.DDIMScheduler(); ts = sch.set_timesteps(STEPS)
    cam, text, bev, boxes = cfg_inputs(D, csd, sc)
    tr.load_inputs(torch.stack([sc["latents"]] * 6, 1), cam, text, bev, boxes, ts, sch.coefficient_table())
    assert (tr._health == 0).all() and tr.step_ctr.item() == 0


def test_bad_mode_is_refused(nets):
    with pytest.raises(AssertionError, match="health="):
        plan(nets, health="on")


def test_group_stats_lowering_refuses_what_the_kernel_cannot_take():
    x = torch.zeros(4, 10)
    with pytest.raises(ValueError, match="dense"):
        O.GroupStats(x.t(), torch.zeros(10, 4)).lower()
    with pytest.raises(ValueError, match="out must be"):
        O.GroupStats(x, torch.zeros(4, 3)).lower()
    with pytest.raises(ValueError, match="needs `row`"):
        O.GroupStats(x, torch.zeros(2, 4, 4)).lower()
    with pytest.raises(ValueError, match="fp32 or 16-bit"):
        O.GroupStats(x.double(), torch.zeros(4, 4)).lower()
    code, d = O.GroupStats(x[:, :8], torch.zeros(4, 4)).lower()           # padded groups: stride 10, 8 elements each
    assert (d.G, d.n, d.sG, d.f32) == (4, 8, 10, 1)
    assert O.dtype_code(O.GroupStats(x.half(), torch.zeros(4, 4))) == 1 and O.dtype_code(O.GroupStats(x.bfloat16(), torch.zeros(4, 4))) == 0
    assert [O.GroupStats.chain_length(n, True) for n in (1, 1024, 1025, 5600)] == [12, 12, 13, 17]
    assert [O.GroupStats.chain_length(n, False) for n in (1, 2048, 2049, 268800)] == [13, 13, 14, 144]


class _Net:
    def __init__(self):
        self._p = object()

    def packed(self):
        return self._p


def test_plan_key_is_unchanged_with_the_switch_off():
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    pipe = StableDiffusionBEVControlNetPipeline(unet=_Net(), controlnet=_Net())
    assert pipe.health is None and pipe.health_action == "flag" and pipe.health_absmax is None
    args = (3, 0, True, 5, 28, 50, 4, 2, 1, 77, "ddim", 0, torch.bfloat16, True)
    today = (3, 0, True, 5, 28, 50, 4, 2.0, 1.0, 77, "ddim", 0, torch.bfloat16, id(pipe.unet.packed()), id(pipe.controlnet.packed()), True)
    assert pipe._plan_key(*args) == today and pipe._plan_key(*args, None) == today
    for mode in ("final", "trace"):
        key = pipe._plan_key(*args, mode)
        assert key[:-1] == today and key[-1] == ("health", mode)
