"""CPU: mdx_latent_renoise_* (include/mdx.h: MdxRenoiseDesc) and what stands on it before any kernel runs.

  the noise reference   a numpy Philox4x32-10 reproducing the Random123 known answers, and the documented mapping words -> normals in
                        float64 (noise_ref); tests/test_latent_renoise_gpu.py and tests/test_resample_gpu.py judge the kernel with it;
  the schedule          schedulers.resample_actions, expanded back to RePaint indices, equals the index lists recorded from the reference's
                        RePaintScheduler.set_timesteps (tests/golden/repaint_indices.json), and the step counter never leaves [0, num_steps];
  the host contract     one valid descriptor and, per sentence of the header contract, mutations that violate only that sentence
                        (table-driven like tests/test_latent_blend_contract.py: fake pointers, refused where a device is visible);
  binding, op record    sizes / offsets against the C header, ops.LatentRenoise.lower();
  the plan              SamplerPlan(resample=) owns visit_ctr, seeds and one jump program; the step program is unchanged op for op;
  the pipeline          pipe.resample refusals are raised on the host before any device work; the plan key gains one trailing entry.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from magicdrive_amd import _lib as L
from philox_ref import noise_ref, noise_words, philox4x32_10, shared_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: must not run where a launch could succeed")


# ---- the noise reference (tests/philox_ref.py holds the one copy) ----------------------------------------------------------------
def test_philox_known_answers():
    h = lambda s: np.array([int(x, 16) for x in s.split()], dtype=np.uint32)
    for ctr, key, want in (("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                           ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                           ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")):
        got = philox4x32_10(h(ctr), h(key))
        assert (got == h(want)).all(), (ctr, key, [hex(int(x)) for x in got])


def test_noise_reference_is_a_standard_normal_and_bounded():
    z = noise_ref(seed=0x1234_5678_9ABC_DEF0, visit=3, count=1 << 18)
    assert np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(48 * np.log(2)) + 1e-12
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    # another visit or another seed shares no block; a later block does not depend on where the evaluation starts
    assert shared_blocks(noise_words(7, 0, 1 << 16), noise_words(7, 1, 1 << 16)) == 0
    assert shared_blocks(noise_words(7, 0, 1 << 16), noise_words(8, 0, 1 << 16)) == 0
    assert (noise_ref(7, 2, 40)[8:12] == noise_ref(7, 2, 4, first_block=2)).all()


# ---- the schedule ----------------------------------------------------------------------------------------------------------------
def _golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "repaint_indices.json")))["cases"]


@pytest.mark.parametrize("case,length", [("6,2,2", 14), ("20,5,3", 80), ("50,10,10", 770), ("6,2,1", 6), ("4,10,3", 4)])
def test_resample_actions_are_repaints_index_list(case, length):
    from magicdrive_amd.schedulers import resample_actions, resample_indices
    n, jl, jn = (int(v) for v in case.split(","))
    want = _golden()[case]
    assert len(want) == length
    if case == "6,2,2":
        assert want == [5, 4, 3, 2, 3, 4, 3, 2, 1, 0, 1, 2, 1, 0]
    acts = resample_actions(n, jl, jn)
    assert all(a == "step" or a == ("jump", jl) for a in acts)
    assert resample_indices(n, acts) == want
    # each ascending run of jump_length indices is ONE jump
    runs = sum(1 for i in range(1, len(want)) if want[i] > want[i - 1] and (i < 2 or want[i - 1] < want[i - 2]))
    assert acts.count(("jump", jl)) == runs and acts.count("step") + jl * runs == len(want)
    if jn == 1 or jl >= n:
        assert acts == ["step"] * n
    c = 0
    for a in acts:                                    # the device-side counter along the list
        assert 0 <= c <= n
        if a == "step":
            assert c < n, "a step past the last row of the tables"
            c += 1
        else:
            assert c >= 1 and c - a[1] >= 0
            c -= a[1]
    assert c == n and acts[-1] == "step"


def test_resample_actions_refuse_bad_arguments():
    from magicdrive_amd.schedulers import resample_actions
    for bad in ((0, 2, 2), (6, 0, 2), (6, 2, 0), (6, 2.0, 2), (6, 2, True), (6, -1, 2)):
        with pytest.raises(ValueError):
            resample_actions(*bad)


# ---- the host contract -----------------------------------------------------------------------------------------------------------
OK, EINVAL = 0, -1
BIG = 1 << 31
P = lambda k: 0x10000000 * k        # fake, 256 MiB apart, aligned to everything
OP = L.OP_LATENT_RENOISE
N = 6 * 28 * 50 * 4


def renoise(**kw):
    """The jump op of a DDIM plan of one scene: 6 views of 28 x 50 x 4 latents (one seed per view), CFG, 16-bit x_in with 8 channels per pixel."""
    d = dict(x=P(1), x_in=P(2), coef=P(3), step_ptr=P(4), visit_ptr=P(5), seeds=P(6), n=N, group_elems=N // 6, jump=5, n_rows=20, coef_ld=4,
             col_t=0, col_p=2, cfg=1, xin_c=4, xin_ld=8)
    d.update(kw); return d


# (sentence of include/mdx.h, descriptor, what mdx_last_error() must name)
TABLE = [
    ("x, coef, step_ptr, visit_ptr, seeds not NULL", renoise(x=0), "x must not be NULL"),
    ("x, coef, step_ptr, visit_ptr, seeds not NULL", renoise(coef=0), "coef must not be NULL"),
    ("x, coef, step_ptr, visit_ptr, seeds not NULL", renoise(step_ptr=0), "step_ptr must not be NULL"),
    ("x, coef, step_ptr, visit_ptr, seeds not NULL", renoise(visit_ptr=0), "visit_ptr must not be NULL"),
    ("x, coef, step_ptr, visit_ptr, seeds not NULL", renoise(seeds=0), "seeds must not be NULL"),
    ("x, coef, step_ptr, visit_ptr 4-byte aligned", renoise(x=P(1) + 2), "x must be 4-byte"),
    ("x, coef, step_ptr, visit_ptr 4-byte aligned", renoise(coef=P(3) + 1), "coef must be 4-byte"),
    ("x, coef, step_ptr, visit_ptr 4-byte aligned", renoise(step_ptr=P(4) + 2), "step_ptr must be 4-byte"),
    ("x, coef, step_ptr, visit_ptr 4-byte aligned", renoise(visit_ptr=P(5) + 3), "visit_ptr must be 4-byte"),
    ("seeds 8-byte aligned", renoise(seeds=P(6) + 4), "seeds must be 8-byte"),
    ("x_in at its element's alignment (4 / 2 bytes)", renoise(x_in=P(2) + 1), "x_in must be 2-byte"),
    ("x_in at its element's alignment (4 / 2 bytes)", renoise(x_in=P(2) + 2, xin_ld=0, xin_c=0), "x_in must be 4-byte"),
    ("n not negative", renoise(n=-4, group_elems=1), "n=-4"),
    ("group_elems >= 1 and divides n", renoise(group_elems=0), "group_elems=0"),
    ("group_elems >= 1 and divides n", renoise(group_elems=-4), "group_elems=-4"),
    ("group_elems >= 1 and divides n", renoise(group_elems=9), "group_elems=9"),
    ("jump and n_rows fit a 32-bit int and are >= 1", renoise(jump=0), "jump=0"),
    ("jump and n_rows fit a 32-bit int and are >= 1", renoise(jump=-2), "jump=-2"),
    ("jump and n_rows fit a 32-bit int and are >= 1", renoise(jump=BIG), "jump="),
    ("jump and n_rows fit a 32-bit int and are >= 1", renoise(n_rows=0), "n_rows=0"),
    ("jump and n_rows fit a 32-bit int and are >= 1", renoise(n_rows=-1), "n_rows=-1"),
    ("jump and n_rows fit a 32-bit int and are >= 1", renoise(n_rows=BIG), "n_rows="),
    ("0 <= col_t, col_p < coef_ld", renoise(col_t=4), "col_t=4"),
    ("0 <= col_t, col_p < coef_ld", renoise(col_t=-1), "col_t=-1"),
    ("0 <= col_t, col_p < coef_ld", renoise(col_p=4), "col_p=4"),
    ("0 <= col_t, col_p < coef_ld", renoise(col_p=-2), "col_p=-2"),
    ("0 <= col_t, col_p < coef_ld", renoise(coef_ld=0, col_t=0, col_p=0), "col_t=0"),
    ("cfg in {0, 1}", renoise(cfg=2), "cfg=2"),
    ("cfg in {0, 1}", renoise(cfg=-1), "cfg=-1"),
    ("xin_c, xin_ld, coef_ld fit a 32-bit int", renoise(xin_c=BIG), "xin_c="),
    ("xin_c, xin_ld, coef_ld fit a 32-bit int", renoise(xin_ld=BIG), "xin_ld="),
    ("xin_c, xin_ld, coef_ld fit a 32-bit int", renoise(coef_ld=BIG), "coef_ld="),
    ("xin_ld is not negative", renoise(xin_ld=-8), "xin_ld=-8"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", renoise(xin_c=0), "xin_c=0"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", renoise(xin_c=-4), "xin_c=-4"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", renoise(xin_c=16), "xin_c=16"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", renoise(xin_c=11, xin_ld=16), "xin_c=11"),
]


def _desc(fields):
    d = L.MdxRenoiseDesc()
    names = {f[0] for f in d._fields_}
    for k, v in fields.items():
        assert k in names, k
        setattr(d, k, v)
    return d


def _call(path, d):
    lib = L.lib()
    if path == "program":
        prog = L.Program([(OP, d, L.DTYPE_BF16)])
        rc = lib.mdx_program_run(ctypes.byref(prog.buf), 1, None)
    else:
        fn = getattr(lib, L.entry_name(OP, L.DTYPE_F16 if path == "f16" else L.DTYPE_BF16))
        rc = fn(ctypes.byref(d), None)
    return rc, (lib.mdx_last_error() or b"").decode()


@no_device
@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("clause,fields,names", TABLE, ids=[f"{i}-{n}" for i, (_, _, n) in enumerate(TABLE)])
def test_violation_is_rejected_on_the_host(clause, fields, names, path):
    rc, msg = _call(path, _desc(fields))
    assert rc == EINVAL, f"[{clause}] via {path}: rc={rc} (want {EINVAL}): {msg!r}"
    assert names in msg, f"[{clause}] via {path}: message {msg!r} does not name {names!r}"
    if path == "program":
        assert msg.startswith("op 0 (opcode %d)" % OP), msg
    elif path == "f16":
        assert "mdx_latent_renoise_f16" in msg, msg


@no_device
@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("fields", [renoise(n=0), renoise(n=0, x_in=0), renoise(n=0, xin_ld=0, xin_c=0, cfg=0), renoise(n=0, group_elems=7)],
                         ids=["n0", "n0-no-x_in", "n0-fp32-x_in", "n0-any-group"])
def test_empty_problem_launches_nothing(fields, path):
    """n == 0 returns MDX_OK before any launch: on a machine without a device a launch attempt would come back MDX_ELAUNCH."""
    rc, msg = _call(path, _desc(fields))
    assert rc == OK, f"rc={rc}: {msg!r}"


@no_device
def test_an_empty_problem_is_still_checked():
    rc, msg = _call("bf16", _desc(renoise(n=0, seeds=P(6) + 4)))
    assert rc == EINVAL and "seeds must be 8-byte" in msg
    rc, msg = _call("bf16", _desc(renoise(n=0, jump=0)))
    assert rc == EINVAL and "jump=0" in msg


def test_every_host_check_has_a_row():
    """Every field a check of the entry point (or of a shared helper of csrc/latent.h it calls) names is named by a row, and every sentence
    the table quotes stands in the header."""
    from test_contract import with_latent_helpers
    body = with_latent_helpers(open(os.path.join(ROOT, "magicdrive_amd", "csrc", "noise.hip")).read().split('extern "C" int mdx_latent_renoise_bf16(')[1])
    fields = set(re.findall(r'need_\w+\(op, "([A-Za-z_]+)"', body)) | set(re.findall(r'"%s: (\w+)=%ld', body)) | set(re.findall(r'"%s: (\w+) must not be NULL"', body))
    assert fields == {"x", "x_in", "coef", "step_ptr", "visit_ptr", "seeds", "n", "group_elems", "jump", "n_rows", "coef_ld", "col_t", "col_p", "cfg",
                      "xin_c", "xin_ld"}, fields
    names = [n for _, _, n in TABLE]
    covered = {f for f in fields if any(n.startswith(f + "=") or n.startswith(f + " must") for n in names)}
    assert fields == covered, sorted(fields - covered)
    flat = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "mdx.h")).read())
    for clause in {c for c, _, _ in TABLE}:
        assert re.sub(r"[\s*]+", " ", clause) in flat, clause


def test_binding_matches_the_header(tmp_path):
    """sizeof / offsetof of MdxRenoiseDesc in the C header equal the ctypes mirror's; the opcode and both symbols are declared and exported;
    the ABI version is still 12 and the op is not a row of DESC_OF_OP."""
    import subprocess
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mdx.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(MdxRenoiseDesc), '
                 'offsetof(MdxRenoiseDesc, visit_ptr), offsetof(MdxRenoiseDesc, seeds), offsetof(MdxRenoiseDesc, n), offsetof(MdxRenoiseDesc, xin_ld), '
                 'MDX_OP_LATENT_RENOISE);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    size, o_visit, o_seeds, o_n, o_ld, code = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    S = L.MdxRenoiseDesc
    assert (size, o_visit, o_seeds, o_n, o_ld) == (ctypes.sizeof(S), S.visit_ptr.offset, S.seeds.offset, S.n.offset, S.xin_ld.offset) and size == 16 * 8
    assert [f[0] for f in S._fields_] == "x x_in coef step_ptr visit_ptr seeds n group_elems jump n_rows coef_ld col_t col_p cfg xin_c xin_ld".split()
    assert size <= L.OP_BYTES - 16
    assert code == L.OP_LATENT_RENOISE == 19 and L.ENTRY_OF_OP[L.OP_LATENT_RENOISE] == "mdx_latent_renoise_bf16"
    assert {"mdx_latent_renoise_bf16", "mdx_latent_renoise_f16"} <= set(L.EXPORTS)
    assert L.OP_LATENT_RENOISE not in L.DESC_OF_OP
    assert L.lib().mdx_abi_version() == 12 and L.ABI_VERSION == 12


def test_op_record_checks_and_flops():
    """ops.LatentRenoise.lower() on CPU views: the plan's fields reach the descriptor, bad records raise; 0 flops, every operand's bytes once."""
    from magicdrive_amd import flops as FL
    from magicdrive_amd import ops as O
    views, h, w, C = 12, 3, 5, 4
    n = views * h * w * C
    x = torch.zeros(n)
    step, visit = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    seeds = torch.zeros(views, dtype=torch.int64)
    x_in = torch.zeros(2 * views * h * w, 8, dtype=torch.float16)
    op = O.LatentRenoise(x, torch.zeros(20, 4), step, visit, seeds, jump=5, x_in=x_in, cfg=True, xin_c=C)
    code, d = op.lower()
    assert code == L.OP_LATENT_RENOISE
    assert (d.n, d.group_elems, d.jump, d.n_rows, d.coef_ld, d.col_t, d.col_p, d.cfg, d.xin_c, d.xin_ld) == (n, h * w * C, 5, 20, 4, 0, 2, 1, C, 8)
    assert (d.x, d.x_in, d.step_ptr, d.visit_ptr, d.seeds) == (x.data_ptr(), x_in.data_ptr(), step.data_ptr(), visit.data_ptr(), seeds.data_ptr())
    assert O.dtype_code(op) == L.DTYPE_F16 and FL.op_flops(op) == 0.0
    assert FL.op_bytes(op) == 4 * 2 * n + 8 * views + 2 * x_in.numel() and FL.kernel_family(op) == "elementwise"
    flat = O.LatentRenoise(x, torch.zeros(20, 6), step, visit, seeds, jump=1, x_in=torch.zeros(n), col_t=1, col_p=5)
    d = flat.lower()[1]
    assert (d.xin_ld, d.xin_c, d.cfg, d.col_t, d.col_p, d.coef_ld) == (0, 0, 0, 1, 5, 6) and O.dtype_code(flat) == L.DTYPE_BF16
    for bad in (dict(seeds=torch.zeros(7, dtype=torch.int64)), dict(seeds=seeds.int()), dict(coef=torch.zeros(20, 12)), dict(x=x.double()),
                dict(x_in=torch.zeros(n)), dict(x_in=x_in[:-1]), dict(step=torch.zeros(1, dtype=torch.int64)), dict(visit=torch.zeros(2, dtype=torch.int32)),
                dict(jump=0), dict(jump=2.0), dict(col_t=4, col_p=2)):
        kw = dict(x=x, coef=torch.zeros(20, 4), step=step, visit=visit, seeds=seeds, jump=5, x_in=x_in, cfg=True, xin_c=C)
        kw.update(bad)
        with pytest.raises(ValueError):
            O.LatentRenoise(**kw).lower()


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def test_plan_owns_one_jump_program_and_the_step_is_unchanged():
    from helpers import cfg_inputs, given_view_inputs, scene, state_dicts
    from magicdrive_amd import denoiser as DN, ops as O, schedulers
    from magicdrive_amd.engine import PackedNet
    from magicdrive_amd.networks import spec
    from oracle import denoiser as D
    from test_health_plan_cpu import signature
    cpu = torch.device("cpu")
    cfg = spec.TINY_CONFIG
    usd, csd = state_dicts(cfg)
    un, cn = PackedNet(usd, cpu), PackedNet(csd, cpu)
    mk = lambda **kw: DN.SamplerPlan(cfg, un, cn, cpu, 2, True, 3, (28, 50), num_steps=6, guidance_scale=2.0, given_view_mode=1, **kw)
    base = mk(keep_regions=True)
    off = mk(keep_regions=True, resample=None)
    on = mk(keep_regions=True, resample=2, health="trace")
    assert base.resample is None and base.jump_ops == [] and not hasattr(base, "visit_ctr") and not hasattr(base, "seeds")
    assert signature(off.step_ops) == signature(base.step_ops) and signature(off.prologue_ops) == signature(base.prologue_ops)
    assert signature(on.step_ops) == signature(mk(keep_regions=True, health="trace").step_ops) and signature(on.prologue_ops) == signature(base.prologue_ops)
    assert len(on.jump_ops) == 1 and isinstance(on.jump_ops[0], O.LatentRenoise)
    j = on.jump_ops[0]
    assert j.x.data_ptr() == on.x.data_ptr() and j.coef is on.coef and j.step is on.step_ctr and j.visit is on.visit_ctr and j.seeds is on.seeds
    assert j.x_in.data_ptr() == on.x_in.data_ptr() and j.cfg is True and j.jump == 2
    assert tuple(on.seeds.shape) == (12,) and on.seeds.dtype == torch.int64 and on.visit_ctr.dtype == torch.int32
    d = j.lower()[1]
    assert (d.n, d.group_elems, d.jump, d.n_rows, d.col_t, d.col_p, d.cfg, d.xin_c) == (on.x.numel(), 28 * 50 * 4, 2, 6, 0, 2, 1, 4)
    for bad in (dict(resample=2), dict(keep_regions=True, resample=2, scheduler_kind="unipc"), dict(keep_regions=True, resample=0),
                dict(keep_regions=True, resample=True)):
        with pytest.raises(AssertionError):
            mk(**bad)
    # load_inputs: one seed per scene, replicated over its views; visit_ctr restarts
    sc = scene(cfg, 2, 3)
    sch = schedulers.DDIMScheduler(); sch.set_timesteps(6)
    cam, text, bev, boxes = cfg_inputs(D, csd, sc)
    cl = given_view_inputs()
    gm = torch.tensor([[v is not None for v in r] for r in cl])
    gl = torch.stack([torch.stack([torch.zeros(4, 28, 50) if v is None else v for v in r]) for r in cl])
    args = (torch.stack([sc["latents"]] * 6, 1), cam, text, bev, boxes, sch.timesteps, sch.coefficient_table())
    kw = dict(given_mask=gm, given_latents=gl, keep_mask=torch.full((2, 6, 28, 50), 0.5) * gm[..., None, None])
    on.visit_ctr.fill_(7)
    on.load_inputs(*args, **kw, seeds=torch.tensor([11, -5]))
    assert on.seeds.tolist() == [11] * 6 + [-5] * 6 and int(on.visit_ctr) == 0 and int(on.step_ctr) == 0
    with pytest.raises(AssertionError):
        on.load_inputs(*args, **kw)
    with pytest.raises(AssertionError):
        base.load_inputs(*args, **kw, seeds=torch.tensor([11, -5]))


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
class _Net:
    cfg = {"neighboring_view_pair": {i: [(i - 1) % 6, (i + 1) % 6] for i in range(6)}}

    def __init__(self):
        self._p = object()

    def packed(self):
        return self._p


def test_plan_key_gains_one_trailing_entry_only_when_set():
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    pipe = StableDiffusionBEVControlNetPipeline(unet=_Net(), controlnet=_Net())
    assert pipe.resample is None
    args = (3, 0, True, 5, 28, 50, 4, 2, 1, 77, "ddim", 1, torch.bfloat16, True)
    today = (3, 0, True, 5, 28, 50, 4, 2.0, 1.0, 77, "ddim", 1, torch.bfloat16, id(pipe.unet.packed()), id(pipe.controlnet.packed()), True)
    assert pipe._plan_key(*args, None, regions=True, resample=None) == today + (("regions",),) == pipe._plan_key(*args, None, regions=True)
    assert pipe._plan_key(*args, None, regions=True, resample=5) == today + (("regions",), ("resample", 5))
    assert pipe._plan_key(*args, "trace", regions=True, resample=2) == today + (("health", "trace"), ("regions",), ("resample", 2))


def test_resample_refusals_come_before_any_device_work():
    """A pipeline that was never moved to a device: an accepted call ends at the sampler's own "no CPU path" error; every refusal of
    pipe.resample is raised before that (and before the masks are looked at)."""
    from magicdrive_amd import schedulers
    from magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view import StableDiffusionBEVControlNetGivenViewPipeline
    lat = lambda: torch.zeros(4, 28, 50)
    cl = [[lat(), None, None, lat(), None, None], [None] * 5 + [lat()]]
    ok = [[torch.full((28, 50), 0.5), None, None, None, None, None], [None] * 5 + [torch.ones(28, 50)]]
    kw = dict(prompt=None, image=torch.zeros(2, 8, 200, 200), camera_param=torch.zeros(2, 6, 3, 7), height=224, width=400,
              prompt_embeds=torch.zeros(2, 77, 8), negative_prompt_embeds=torch.zeros(2, 77, 8), output_type="latent", conditional_latents=cl)

    def call(resample, masks=ok, unipc=False):
        pipe = StableDiffusionBEVControlNetGivenViewPipeline(unet=_Net(), controlnet=_Net())
        if unipc:
            pipe.scheduler = schedulers.UniPCMultistepScheduler.from_config(pipe.scheduler.config)
        pipe.keep_masks, pipe.resample = masks, resample
        return pipe(**kw)

    with pytest.raises(RuntimeError, match="no CPU path"):
        call((5, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        call([10, 1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(None, unipc=True)
    for bad in ((0, 2), (2, 0), (2.0, 2), (2, 2, 2), 5, (True, 2), (-1, 3), "5,2"):
        with pytest.raises(ValueError, match="resample="):
            call(bad)
    with pytest.raises(ValueError, match="without keep_masks"):
        call((5, 2), masks=None)
    with pytest.raises(NotImplementedError, match="multistep history"):
        call((5, 2), unipc=True)
