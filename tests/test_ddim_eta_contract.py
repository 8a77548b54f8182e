"""CPU: mdx_cfg_ddim_eta_step_* (include/mdx.h: MdxDdimEtaDesc) — stochastic DDIM, eta > 0 — and what stands on it before any kernel runs.

  the noise reference   the float64 mapping of tests/test_latent_renoise_contract.py with counter word 3 = 1 (eta_noise_ref): the step's
                        stream, which shares no block with a jump's; tests/test_ddim_eta_gpu.py judges the kernel with it;
  the host contract     one valid descriptor and, per sentence of the header contract, mutations that violate only that sentence
                        (fake pointers, refused where a device is visible: a missing check would come back MDX_ELAUNCH);
  binding, op record    size / offsets against the C header, opcode 21, both symbols, ops.DdimEtaStep.lower();
  the scheduler         DDIMScheduler.variance_table and the contract's update in float64 against what the reference's DDIMScheduler
                        computed (tests/golden/ddim_eta_steps.pt, written by tools/make_golden_ddim_eta.py); the eta = 0 identities;
                        step()'s signature and refusals (the kernel run of step(..., variance_noise=) is in the GPU file);
  the plan              SamplerPlan(stochastic=True): ONE ops.DdimEtaStep in the scheduler op's place, everything else unchanged;
  the pipeline          the plan key gains one trailing ("eta",) only when eta != 0; every refusal comes before any device work.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from magicdrive_amd import _lib as L
from philox_ref import eta_noise_ref, eta_noise_words, noise_words, shared_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: must not run where a launch could succeed")


# ---- the noise reference (tests/philox_ref.py holds the one copy) ----------------------------------------------------------------
def test_step_noise_is_a_standard_normal_in_a_domain_of_its_own():
    z = eta_noise_ref(seed=0x1234_5678_9ABC_DEF0, draw=3, count=1 << 18)
    n = z.size
    assert np.isfinite(z).all() and abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    # equal seed, draw = visit: no block in common with a jump's stream; nor with another draw's
    for seed, v in ((7, 0), (7, 5), (-3, 1)):
        assert shared_blocks(eta_noise_words(seed, v, 1 << 16), noise_words(seed, v, 1 << 16)) == 0
    assert shared_blocks(eta_noise_words(7, 0, 1 << 16), eta_noise_words(7, 1, 1 << 16)) == 0
    assert (eta_noise_ref(7, 2, 40)[8:12] == eta_noise_ref(7, 2, 4, first_block=2)).all()


# ---- the host contract -----------------------------------------------------------------------------------------------------------
OK, EINVAL = 0, -1
BIG = 1 << 31
P = lambda k: 0x10000000 * k        # fake, 256 MiB apart, aligned to everything
OP = L.OP_DDIM_ETA
N = 6 * 28 * 50 * 4


def eta_step(**kw):
    """The scheduler op of a stochastic DDIM plan of one scene: 6 views of 28 x 50 x 4 latents (one seed per view), CFG, 16-bit x_in with 8
    channels per pixel, given views off."""
    d = dict(x=P(1), eps=P(2), coef=P(3), var=P(4), step_ptr=P(5), draw_ptr=P(6), x_in=P(7), seeds=P(8), noise=0, n=N, cfg=1, guidance=2.0,
             xin_c=4, xin_ld=8, group_elems=N // 6, n_rows=20)
    d.update(kw); return d


GV = dict(gv_mask=P(9), gv_noise=P(10), gv_cond=P(11), gv_mode=1, gv_view_elems=N // 6, gv_last_step=19)

# (sentence of include/mdx.h, descriptor, what mdx_last_error() must name)
TABLE = [
    ("x, eps, coef, var, step_ptr, draw_ptr not NULL", eta_step(x=0), "x must not be NULL"),
    ("x, eps, coef, var, step_ptr, draw_ptr not NULL", eta_step(eps=0), "eps must not be NULL"),
    ("x, eps, coef, var, step_ptr, draw_ptr not NULL", eta_step(coef=0), "coef must not be NULL"),
    ("x, eps, coef, var, step_ptr, draw_ptr not NULL", eta_step(var=0), "var must not be NULL"),
    ("x, eps, coef, var, step_ptr, draw_ptr not NULL", eta_step(step_ptr=0), "step_ptr must not be NULL"),
    ("x, eps, coef, var, step_ptr, draw_ptr not NULL", eta_step(draw_ptr=0), "draw_ptr must not be NULL"),
    ("seeds and noise not both NULL", eta_step(seeds=0, noise=0), "seeds must not be NULL"),
    ("x, eps, coef, var, step_ptr, draw_ptr, noise 4-byte aligned", eta_step(x=P(1) + 2), "x must be 4-byte"),
    ("x, eps, coef, var, step_ptr, draw_ptr, noise 4-byte aligned", eta_step(eps=P(2) + 1), "eps must be 4-byte"),
    ("x, eps, coef, var, step_ptr, draw_ptr, noise 4-byte aligned", eta_step(coef=P(3) + 3), "coef must be 4-byte"),
    ("x, eps, coef, var, step_ptr, draw_ptr, noise 4-byte aligned", eta_step(var=P(4) + 2), "var must be 4-byte"),
    ("x, eps, coef, var, step_ptr, draw_ptr, noise 4-byte aligned", eta_step(step_ptr=P(5) + 2), "step_ptr must be 4-byte"),
    ("x, eps, coef, var, step_ptr, draw_ptr, noise 4-byte aligned", eta_step(draw_ptr=P(6) + 1), "draw_ptr must be 4-byte"),
    ("x, eps, coef, var, step_ptr, draw_ptr, noise 4-byte aligned", eta_step(noise=P(12) + 2), "noise must be 4-byte"),
    ("x, eps, coef, var, step_ptr, draw_ptr, noise 4-byte aligned", eta_step(seeds=0, noise=P(12) + 1), "noise must be 4-byte"),
    ("seeds 8-byte aligned", eta_step(seeds=P(8) + 4), "seeds must be 8-byte"),
    ("x_in at its element's alignment (4 / 2 bytes)", eta_step(x_in=P(7) + 1), "x_in must be 2-byte"),
    ("x_in at its element's alignment (4 / 2 bytes)", eta_step(x_in=P(7) + 2, xin_ld=0, xin_c=0), "x_in must be 4-byte"),
    ("n not negative", eta_step(n=-4, group_elems=1), "n=-4"),
    ("group_elems >= 1 and divides n", eta_step(group_elems=0), "group_elems=0"),
    ("group_elems >= 1 and divides n", eta_step(group_elems=-4), "group_elems=-4"),
    ("group_elems >= 1 and divides n", eta_step(group_elems=9), "group_elems=9"),
    ("group_elems >= 1 and divides n", eta_step(seeds=0, noise=P(12), group_elems=0), "group_elems=0"),
    ("n_rows fits a 32-bit int and is >= 1", eta_step(n_rows=0), "n_rows=0"),
    ("n_rows fits a 32-bit int and is >= 1", eta_step(n_rows=-1), "n_rows=-1"),
    ("n_rows fits a 32-bit int and is >= 1", eta_step(n_rows=BIG), "n_rows="),
    ("cfg in {0, 1}", eta_step(cfg=2), "cfg=2"),
    ("cfg in {0, 1}", eta_step(cfg=-1), "cfg=-1"),
    ("xin_c, xin_ld, gv_last_step fit a 32-bit int and xin_ld is not negative", eta_step(xin_c=BIG), "xin_c="),
    ("xin_c, xin_ld, gv_last_step fit a 32-bit int and xin_ld is not negative", eta_step(xin_ld=BIG), "xin_ld="),
    ("xin_c, xin_ld, gv_last_step fit a 32-bit int and xin_ld is not negative", eta_step(**dict(GV, gv_last_step=BIG)), "gv_last_step="),
    ("xin_c, xin_ld, gv_last_step fit a 32-bit int and xin_ld is not negative", eta_step(xin_ld=-8), "xin_ld=-8"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", eta_step(xin_c=0), "xin_c=0"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", eta_step(xin_c=-4), "xin_c=-4"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", eta_step(xin_c=16), "xin_c=16"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", eta_step(xin_c=11, xin_ld=16), "xin_c=11"),
    ("a given-view mode needs gv_noise (mode 1: also gv_cond) and gv_view_elems dividing n", eta_step(**dict(GV, gv_noise=0)), "given-view mode 1"),
    ("a given-view mode needs gv_noise (mode 1: also gv_cond) and gv_view_elems dividing n", eta_step(**dict(GV, gv_cond=0)), "given-view mode 1"),
    ("a given-view mode needs gv_noise (mode 1: also gv_cond) and gv_view_elems dividing n", eta_step(**dict(GV, gv_mode=2, gv_noise=0)), "given-view mode 2"),
    ("a given-view mode needs gv_noise (mode 1: also gv_cond) and gv_view_elems dividing n", eta_step(**dict(GV, gv_mode=3)), "given-view mode 3"),
    ("a given-view mode needs gv_noise (mode 1: also gv_cond) and gv_view_elems dividing n", eta_step(**dict(GV, gv_view_elems=0)), "given-view mode 1"),
    ("a given-view mode needs gv_noise (mode 1: also gv_cond) and gv_view_elems dividing n", eta_step(**dict(GV, gv_view_elems=N // 6 + 1)), "given-view mode 1"),
]


def _desc(fields):
    d = L.MdxDdimEtaDesc()
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
        assert "mdx_cfg_ddim_eta_step_f16" in msg, msg


@no_device
@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("fields", [eta_step(n=0), eta_step(n=0, x_in=0), eta_step(n=0, xin_ld=0, xin_c=0, cfg=0), eta_step(n=0, group_elems=7),
                                    eta_step(n=0, seeds=0, noise=P(12))], ids=["n0", "n0-no-x_in", "n0-fp32-x_in", "n0-any-group", "n0-noise"])
def test_empty_problem_launches_nothing(fields, path):
    """n == 0 returns MDX_OK before any launch: on a machine without a device a launch attempt would come back MDX_ELAUNCH."""
    rc, msg = _call(path, _desc(fields))
    assert rc == OK, f"rc={rc}: {msg!r}"


@no_device
def test_an_empty_problem_is_still_checked():
    rc, msg = _call("bf16", _desc(eta_step(n=0, seeds=P(8) + 4)))
    assert rc == EINVAL and "seeds must be 8-byte" in msg
    rc, msg = _call("bf16", _desc(eta_step(n=0, n_rows=0)))
    assert rc == EINVAL and "n_rows=0" in msg


def test_every_host_check_has_a_row():
    """Every field a check of the entry point (or of a shared helper of csrc/latent.h it calls) names is named by a row, and every sentence
    the table quotes stands in the header."""
    from test_contract import with_latent_helpers
    src = open(os.path.join(ROOT, "magicdrive_amd", "csrc", "noise.hip")).read()
    body = with_latent_helpers(src.split('extern "C" int mdx_cfg_ddim_eta_step_bf16(')[1].split('extern "C"')[0])      # up to the next entry point
    assert "need_xin(" in body and "need_given_views(" in body and "need_aligned(" in body
    fields = set(re.findall(r'need_\w+\(op, "([A-Za-z_]+)"', body)) | set(re.findall(r'"%s: (\w+)=%ld', body)) | set(re.findall(r'"%s: (\w+) must not be NULL', body))
    assert fields == {"x", "eps", "coef", "var", "step_ptr", "draw_ptr", "x_in", "seeds", "noise", "n", "cfg", "xin_c", "xin_ld", "group_elems", "n_rows",
                      "gv_last_step"}, fields
    names = [n for _, _, n in TABLE]
    covered = {f for f in fields if any(n.startswith(f + "=") or n.startswith(f + " must") for n in names)}
    assert fields == covered, sorted(fields - covered)
    assert "given-view mode" in body and any(n.startswith("given-view mode") for n in names)
    flat = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "mdx.h")).read())
    for clause in {c for c, _, _ in TABLE}:
        assert re.sub(r"[\s*]+", " ", clause) in flat, clause


def test_binding_matches_the_header(tmp_path):
    """sizeof / offsetof of MdxDdimEtaDesc in the C header equal the ctypes mirror's; the opcode is 21 and both symbols are declared and
    exported; the ABI version is still 12 and the op is not a row of DESC_OF_OP."""
    import subprocess
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mdx.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(MdxDdimEtaDesc), '
                 'offsetof(MdxDdimEtaDesc, var), offsetof(MdxDdimEtaDesc, draw_ptr), offsetof(MdxDdimEtaDesc, noise), offsetof(MdxDdimEtaDesc, guidance), '
                 'offsetof(MdxDdimEtaDesc, n_rows), offsetof(MdxDdimEtaDesc, gv_last_step), MDX_OP_DDIM_ETA);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    size, o_var, o_draw, o_noise, o_g, o_rows, o_last, code = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    S = L.MdxDdimEtaDesc
    assert (size, o_var, o_draw, o_noise, o_g, o_rows, o_last) == (ctypes.sizeof(S), S.var.offset, S.draw_ptr.offset, S.noise.offset, S.guidance.offset,
                                                                    S.n_rows.offset, S.gv_last_step.offset) and size == 22 * 8
    assert [f[0] for f in S._fields_] == ("x eps coef var step_ptr draw_ptr x_in seeds noise n cfg guidance xin_c xin_ld group_elems n_rows "
                                          "gv_cond gv_noise gv_mask gv_mode gv_view_elems gv_last_step").split()
    assert size <= L.OP_BYTES - 16
    assert code == L.OP_DDIM_ETA == 21 and L.ENTRY_OF_OP[L.OP_DDIM_ETA] == "mdx_cfg_ddim_eta_step_bf16"
    assert L.entry_name(L.OP_DDIM_ETA, L.DTYPE_F16) == "mdx_cfg_ddim_eta_step_f16"
    assert {"mdx_cfg_ddim_eta_step_bf16", "mdx_cfg_ddim_eta_step_f16"} <= set(L.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert "int mdx_cfg_ddim_eta_step_bf16(const MdxDdimEtaDesc* d, void* stream);" in hdr and "int mdx_cfg_ddim_eta_step_f16(const MdxDdimEtaDesc* d, void* stream);" in hdr
    assert L.OP_DDIM_ETA not in L.DESC_OF_OP
    assert L.lib().mdx_abi_version() == 12 and L.ABI_VERSION == 12


def test_op_record_checks_and_flops():
    """ops.DdimEtaStep.lower() on CPU views: the plan's fields reach the descriptor, bad records raise; 0 flops, every operand's bytes once."""
    from magicdrive_amd import flops as FL
    from magicdrive_amd import ops as O
    views, h, w, C = 12, 3, 5, 4
    n = views * h * w * C
    x, eps = torch.zeros(n), torch.zeros(2 * n)
    step, draw = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    seeds = torch.zeros(views, dtype=torch.int64)
    x_in = torch.zeros(2 * views * h * w, 8, dtype=torch.float16)
    coef, var = torch.zeros(20, 4), torch.zeros(20, 2)
    mask = torch.zeros(views, dtype=torch.uint8)
    op = O.DdimEtaStep(x, eps, coef, var, step, draw, seeds=seeds, x_in=x_in, cfg=True, guidance=2.5, xin_c=C, gv_mask=mask, gv_cond=torch.zeros(n),
                       gv_noise=torch.zeros(n), gv_mode=1, gv_last_step=19)
    code, d = op.lower()
    assert code == L.OP_DDIM_ETA
    assert (d.n, d.cfg, d.guidance, d.xin_c, d.xin_ld, d.group_elems, d.n_rows, d.gv_mode, d.gv_view_elems, d.gv_last_step) == (n, 1, 2.5, C, 8, h * w * C, 20, 1, h * w * C, 19)
    assert (d.x, d.eps, d.coef, d.var, d.step_ptr, d.draw_ptr, d.x_in, d.seeds) == tuple(t.data_ptr() for t in (x, eps, coef, var, step, draw, x_in, seeds))
    assert d.noise is None and d.gv_mask == mask.data_ptr()
    assert O.dtype_code(op) == L.DTYPE_F16 and FL.op_flops(op) == 0.0
    assert FL.op_bytes(op) == 4 * 2 * n + 4 * 2 * n + 8 * views + 2 * x_in.numel() and FL.kernel_family(op) == "elementwise"
    z = torch.zeros(n)
    flat = O.DdimEtaStep(x, eps[:n], coef, var, step, draw, noise=z, x_in=torch.zeros(n), n_rows=7)
    d = flat.lower()[1]
    assert (d.xin_ld, d.xin_c, d.cfg, d.group_elems, d.n_rows, d.noise, d.seeds, d.gv_mode) == (0, 0, 0, n, 7, z.data_ptr(), None, 0) and O.dtype_code(flat) == L.DTYPE_BF16
    assert FL.op_bytes(flat) == 4 * 2 * n + 4 * n + 4 * n + 4 * n
    for bad in (dict(seeds=None), dict(seeds=torch.zeros(7, dtype=torch.int64)), dict(seeds=seeds.int()), dict(coef=torch.zeros(20, 12)), dict(var=torch.zeros(20, 4)),
                dict(var=torch.zeros(19, 2)), dict(x=x.double()), dict(eps=eps[:n]), dict(x_in=torch.zeros(n)), dict(x_in=x_in[:-1]), dict(noise=torch.zeros(n - 1)),
                dict(step=torch.zeros(1, dtype=torch.int64)), dict(draw=torch.zeros(2, dtype=torch.int32)), dict(n_rows=0), dict(n_rows=21), dict(n_rows=2.0)):
        kw = dict(x=x, eps=eps, coef=coef, var=var, step=step, draw=draw, seeds=seeds, x_in=x_in, cfg=True, xin_c=C)
        kw.update(bad)
        with pytest.raises(ValueError):
            O.DdimEtaStep(**kw).lower()


# ---- the scheduler ---------------------------------------------------------------------------------------------------------------
ULP = 2.0 ** -23


def _golden():
    g = torch.load(os.path.join(ROOT, "tests", "golden", "ddim_eta_steps.pt"))
    for i in range(g["case"].shape[0]):
        n_steps, index, t = g["case"][i].tolist()
        a_t, a_prev, variance, std = g["scalars"][i].double().tolist()
        sample, eps, z, prev = g["tensors"][i].double().numpy()
        yield dict(n_steps=n_steps, index=index, timestep=t, eta=float(g["eta"][i]), a_t=a_t, a_prev=a_prev, variance=variance, std=std,
                   sample=sample, eps=eps, z=z, prev=prev)


def table_bounds(a_t, a_prev, eta):
    """Absolute bounds on |table - diffusers| for (dir, std) of one step, from the roundings of diffusers' own fp32 evaluation
    (scheduling_ddim.py:_get_variance, :415, :422).  One operation is charged one ulp, 2^-23 relative (torch's pow is not documented
    as correctly rounded).  Counting them:
      variance  6: 1 - a_prev, 1 - a_t, their quotient, a_t / a_prev, 1 - that, the product.  The rounding of a_t / a_prev is
                   amplified by ratio / (1 - ratio) in 1 - ratio: at the last timestep of SD-1.5's schedule ratio = 1 - beta_1 = 0.99915,
                   a factor of about 1200 — the one term of this bound that is not a few ulp;
      std       8: variance's 6 (halved in relative terms by the square root), the power 0.5, the product with eta — and eta itself,
                   a Python float that torch rounds to fp32 (one more ulp on the value, not an operation);
      dir      12: std's 8, the square, the two subtractions of 1 - a_prev - std^2, the power 0.5.
    This side adds ONE rounding per entry: the table is evaluated in double precision from the same fp32 alphas and rounded once."""
    ratio = a_t / a_prev
    rel_var = ULP * (5 + ratio / (1 - ratio))
    var = (1 - a_prev) / (1 - a_t) * (1 - ratio)
    std = eta * var ** 0.5
    rel_std = 0.5 * rel_var + 3 * ULP
    tol_std = std * (rel_std + ULP)
    A, sq = 1 - a_prev, std * std
    B = A - sq
    abs_B = ULP * A + sq * (2 * rel_std + ULP) + ULP * B
    tol_dir = B ** 0.5 * (0.5 * abs_B / B + 2 * ULP)
    return tol_dir, tol_std


def test_variance_table_and_the_update_against_the_reference_scheduler():
    """variance_table(eta) against the reference's std_dev_t within table_bounds; then the contract's update x <- c2 x0 + dir e + std z,
    evaluated in float64 from our two tables, against the reference step's prev_sample.  The reference evaluates the update in fp32
    tensor arithmetic: 9 operations (sqrt(1 - a_t) e, the difference, the quotient, three products, two sums, std z), each charged one
    ulp of the sum S of the absolute values of the terms; the tables' own bounds enter scaled by |e| and |z|."""
    from magicdrive_amd.schedulers import DDIMScheduler
    cases = list(_golden())
    assert len(cases) == 18 and {(c["n_steps"], c["eta"]) for c in cases} == {(n, e) for n in (20, 50) for e in (0.0, 0.3, 1.0)}
    worst_std = worst_step = 0.0
    for c in cases:
        sch = DDIMScheduler(); sch.set_timesteps(c["n_steps"])
        i = c["index"]
        assert i in (0, c["n_steps"] // 2, c["n_steps"] - 1) and int(sch.timesteps[i]) == c["timestep"]
        a_t, a_p = (float(v) for v in sch.alpha_pair(c["timestep"]))
        assert (a_t, a_p) == (c["a_t"], c["a_prev"]), "the fixture's alphas are not this scheduler's"
        coef, var = sch.coefficient_table().double().numpy(), sch.variance_table(c["eta"])
        assert var.dtype == torch.float32 and tuple(var.shape) == (c["n_steps"], 2)
        d, s = var[i].double().tolist()
        tol_dir, tol_std = table_bounds(a_t, a_p, c["eta"])
        assert abs(s - c["std"]) <= tol_std, f"{c['n_steps']} steps eta={c['eta']} row {i}: std {s!r} vs {c['std']!r} (bound {tol_std:.3e})"
        if c["eta"] > 0:
            worst_std = max(worst_std, abs(s - c["std"]) / tol_std)
            assert abs(c["std"] - c["eta"] * c["variance"] ** 0.5) <= 2 * ULP * c["std"]       # the fixture's two records agree
        c0, c1, c2 = coef[i, :3]
        x0 = (c["sample"] - c1 * c["eps"]) / c0
        ref = c2 * x0 + d * c["eps"] + s * c["z"] * (1.0 if c["eta"] > 0 else 0.0)
        S = c2 * (np.abs(c["sample"]) + c1 * np.abs(c["eps"])) / c0 + d * np.abs(c["eps"]) + s * np.abs(c["z"])
        bound = 9 * ULP * S + tol_dir * np.abs(c["eps"]) + tol_std * np.abs(c["z"])
        ratio = float((np.abs(ref - c["prev"]) / bound).max())
        worst_step = max(worst_step, ratio)
        assert ratio <= 1.0, f"{c['n_steps']} steps eta={c['eta']} row {i}: update error / bound = {ratio:.3f}"
    print(f"[ddim eta tables] worst |std - diffusers| / bound = {worst_std:.3f}; worst update error / bound = {worst_step:.3f}")
    # the last step adds noise too: std about 0.02 eta at SD-1.5's schedule (INTEGRATION.md says so)
    last = [c["std"] / c["eta"] for c in cases if c["eta"] > 0 and c["index"] == c["n_steps"] - 1]
    assert last and all(0.015 < v < 0.025 for v in last), last


@pytest.mark.parametrize("n_steps", [1, 4, 20, 50, 999])
def test_eta_zero_table_is_the_deterministic_one(n_steps):
    from magicdrive_amd.schedulers import DDIMScheduler
    for sch in (DDIMScheduler(), DDIMScheduler(beta_schedule="linear", beta_start=0.0001, beta_end=0.02, set_alpha_to_one=True, steps_offset=0)):
        sch.set_timesteps(n_steps)
        v0 = sch.variance_table(0.0)
        assert torch.equal(v0[:, 0].view(torch.int32), sch.coefficient_table()[:, 3].view(torch.int32)) and bool((v0[:, 1] == 0).all())
        assert torch.equal(sch.variance_table(0), v0)
        v1 = sch.variance_table(1.0)
        assert tuple(v1.shape) == (n_steps, 2) and bool(torch.isfinite(v1).all()) and bool((v1[:, 1] >= 0).all()) and bool((v1[:, 0] <= v0[:, 0]).all())
        # dir^2 + std^2 = 1 - a_prev: the step keeps the marginal variance whatever eta is
        assert torch.allclose(v1[:, 0].double() ** 2 + v1[:, 1].double() ** 2, v0[:, 0].double() ** 2, rtol=0, atol=4 * ULP)
        assert torch.allclose(sch.variance_table(0.5)[:, 1], 0.5 * v1[:, 1], rtol=2 * ULP, atol=0)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), "a", None, True):
        with pytest.raises(ValueError, match="eta="):
            sch.variance_table(bad)


def test_step_signature_and_refusals():
    """step(model_output, timestep, sample, eta, use_clipped_model_output, variance_noise, return_dict): diffusers' parameters in its
    order, WITHOUT generator — the reference pipeline refuses a scheduler whose step takes one (pipeline_bev_controlnet.py:94-97)."""
    from magicdrive_amd.schedulers import DDIMScheduler
    params = inspect.signature(DDIMScheduler.step).parameters
    assert list(params) == ["self", "model_output", "timestep", "sample", "eta", "use_clipped_model_output", "variance_noise", "return_dict"]
    assert "generator" not in params
    assert (params["eta"].default, params["use_clipped_model_output"].default, params["variance_noise"].default, params["return_dict"].default) == (0.0, False, None, True)
    sch = DDIMScheduler(); sch.set_timesteps(4)
    x = torch.zeros(2, 4, 3, 5)
    t = int(sch.timesteps[0])
    with pytest.raises(ValueError, match="variance_noise") as ei:
        sch.step(x, t, x, eta=0.5)
    assert "pipe(" in str(ei.value) and "generator" in str(ei.value)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eta="):
            sch.step(x, t, x, eta=bad, variance_noise=x)
    with pytest.raises(ValueError, match="shape"):
        sch.step(x, t, x, eta=0.5, variance_noise=torch.zeros(3))
    with pytest.raises(RuntimeError, match="CUDA tensors"):       # accepted: the next stop is the kernel, which has no host form
        sch.step(x, t, x, eta=0.5, variance_noise=x, use_clipped_model_output=True)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        sch.step(x, t, x)


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def test_stochastic_plan_swaps_exactly_the_scheduler_op():
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
    mk = lambda **kw: DN.SamplerPlan(cfg, un, cn, cpu, 2, True, 3, (28, 50), num_steps=6, guidance_scale=2.0, **kw)
    for kw in ({}, {"fork": True}, {"given_view_mode": 2}, {"given_view_mode": 1, "keep_regions": True, "resample": 2, "health": "trace"}):
        base, off, on = mk(**kw), mk(stochastic=False, **kw), mk(stochastic=True, **kw)
        assert base.stochastic is False and not hasattr(base, "var") and not hasattr(base, "draw_ctr")
        assert signature(off.step_ops) == signature(base.step_ops) and signature(off.prologue_ops) == signature(base.prologue_ops)
        assert signature(on.prologue_ops) == signature(base.prologue_ops) and signature(on.jump_ops) == signature(base.jump_ops) and on.fork_at == base.fork_at
        assert len(on.step_ops) == len(base.step_ops)
        diff = [i for i, (a, b_) in enumerate(zip(signature(on.step_ops), signature(base.step_ops))) if a != b_]
        assert len(diff) == 1, diff
        new, old = on.step_ops[diff[0]], base.step_ops[diff[0]]
        assert isinstance(new, O.DdimEtaStep) and isinstance(old, O.DdimStep) and sum(isinstance(o, (O.DdimStep, O.DdimEtaStep)) for o in on.step_ops) == 1
        for f in ("cfg", "guidance", "xin_c", "gv_mode", "gv_last_step"):
            assert getattr(new, f) == getattr(old, f), f
        assert new.x.data_ptr() == on.x.data_ptr() and new.eps.data_ptr() == on.eps.data_ptr() and new.x_in.data_ptr() == on.x_in.data_ptr()
        assert new.coef is on.coef and new.var is on.var and new.step is on.step_ctr and new.draw is on.draw_ctr and new.seeds is on.seeds and new.noise is None
        assert (new.gv_mask is None) == (old.gv_mask is None) and tuple(on.coef.shape) == (6, 4) and tuple(on.var.shape) == (6, 2)
        assert tuple(on.seeds.shape) == (12,) and on.seeds.dtype == torch.int64 and on.draw_ctr.dtype == torch.int32
        d = new.lower()[1]
        assert (d.n, d.group_elems, d.n_rows, d.cfg, d.xin_c, d.guidance) == (on.x.numel(), 28 * 50 * 4, 6, 1, 4, 2.0)
        if kw.get("resample"):        # ONE seeds tensor for the jumps and the step noise
            assert on.jump_ops[0].seeds is on.seeds and on.jump_ops[0].coef is on.coef
            assert any(isinstance(o, O.LatentBlend) and o.coef is on.coef for o in on.step_ops)
    with pytest.raises(AssertionError):
        mk(stochastic=True, scheduler_kind="unipc")
    # load_inputs: var is data, one seed per scene replicated over its views, draw_ctr restarts; the 4-column table is untouched by eta
    on = mk(stochastic=True)
    sc = scene(cfg, 2, 3)
    sch = schedulers.DDIMScheduler(); sch.set_timesteps(6)
    cam, text, bev, boxes = cfg_inputs(D, csd, sc)
    args = (torch.stack([sc["latents"]] * 6, 1), cam, text, bev, boxes, sch.timesteps, sch.coefficient_table())
    on.draw_ctr.fill_(7)
    on.load_inputs(*args, seeds=torch.tensor([11, -5]), var=sch.variance_table(0.7))
    assert on.seeds.tolist() == [11] * 6 + [-5] * 6 and int(on.draw_ctr) == 0 and int(on.step_ctr) == 0
    assert torch.equal(on.var, sch.variance_table(0.7)) and torch.equal(on.coef, sch.coefficient_table())
    on.load_inputs(*args, seeds=torch.tensor([11, -5]), var=sch.variance_table(0.2))
    assert torch.equal(on.var, sch.variance_table(0.2))
    for bad in (dict(seeds=torch.tensor([11, -5])), dict(var=sch.variance_table(0.7)), dict(seeds=torch.tensor([11, -5]), var=torch.zeros(5, 2))):
        with pytest.raises(AssertionError):
            on.load_inputs(*args, **bad)
    with pytest.raises(AssertionError):
        mk().load_inputs(*args, var=sch.variance_table(0.7))


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
class _Net:
    cfg = {"neighboring_view_pair": {i: [(i - 1) % 6, (i + 1) % 6] for i in range(6)}}

    def __init__(self):
        self._p = object()

    def packed(self):
        return self._p


def test_plan_key_gains_one_trailing_entry_only_when_eta_is_set():
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    pipe = StableDiffusionBEVControlNetPipeline(unet=_Net(), controlnet=_Net())
    args = (3, 0, True, 5, 28, 50, 4, 2, 1, 77, "ddim", 1, torch.bfloat16, True)
    today = (3, 0, True, 5, 28, 50, 4, 2.0, 1.0, 77, "ddim", 1, torch.bfloat16, id(pipe.unet.packed()), id(pipe.controlnet.packed()), True)
    assert pipe._plan_key(*args) == today == pipe._plan_key(*args, stochastic=False)
    assert pipe._plan_key(*args, stochastic=True) == today + (("eta",),)
    assert pipe._plan_key(*args, "trace", regions=True, resample=2, stochastic=True) == today + (("health", "trace"), ("regions",), ("resample", 2), ("eta",))
    assert pipe._plan_key(*args, None, regions=True, resample=5) == today + (("regions",), ("resample", 5))


def test_eta_refusals_come_before_any_device_work():
    """A pipeline that was never moved to a device: an accepted call ends at the sampler's own "no CPU path" error; every refusal of eta
    is raised before that, in both pipelines."""
    from magicdrive_amd import schedulers
    from magicdrive_amd.pipeline.pipeline_bev_controlnet import StableDiffusionBEVControlNetPipeline
    from magicdrive_amd.pipeline.pipeline_bev_controlnet_given_view import StableDiffusionBEVControlNetGivenViewPipeline
    lat = lambda: torch.zeros(4, 28, 50)
    kw = dict(prompt=None, image=torch.zeros(2, 8, 200, 200), camera_param=torch.zeros(2, 6, 3, 7), height=224, width=400,
              prompt_embeds=torch.zeros(2, 77, 8), negative_prompt_embeds=torch.zeros(2, 77, 8), output_type="latent")
    gv = dict(conditional_latents=[[lat(), None, None, lat(), None, None], [None] * 5 + [lat()]])

    def call(cls, eta, unipc=False, **more):
        pipe = cls(unet=_Net(), controlnet=_Net())
        if unipc:
            pipe.scheduler = schedulers.UniPCMultistepScheduler.from_config(pipe.scheduler.config)
        return pipe(eta=eta, **kw, **more)

    for cls, more in ((StableDiffusionBEVControlNetPipeline, {}), (StableDiffusionBEVControlNetGivenViewPipeline, gv)):
        for eta in (0.0, 0.3, 1, 1.0, np.float32(0.5)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call(cls, eta, **more)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(cls, 0.0, unipc=True, **more)
        for bad in (-0.5, float("nan"), float("inf"), "x"):
            with pytest.raises(ValueError, match="eta="):
                call(cls, bad, **more)
            with pytest.raises(ValueError, match="eta="):
                call(cls, bad, unipc=True, **more)
        with pytest.raises(NotImplementedError, match="UniPC"):
            call(cls, 0.5, unipc=True, **more)
