"""CPU: the host-side contract of mdx_latent_blend_* (include/mdx.h: MdxBlendDesc), table-driven like tests/test_sdpa_contract.py.

One valid descriptor and, per sentence of the header contract, mutations that violate only that sentence: each must come back MDX_EINVAL
with a message naming the field — through the bf16 symbol, the _f16 symbol and a one-op mdx_program_run.  Pointers are plain integers
with the wanted alignment: a missing check shows up as a launch attempt (MDX_ELAUNCH on a machine without a device), never as a memory
access; for that reason the tables refuse to run where a device is visible, and the valid descriptor is only ever called with n == 0,
where the contract says nothing is launched.
"""
import ctypes
import os
import re

import pytest
import torch

from magicdrive_amd import _lib as L

no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: must not run where a launch could succeed")

OK, EINVAL = 0, -1
BIG = 1 << 31
P = lambda k: 0x10000000 * k        # fake, 256 MiB apart, aligned to everything
OP = L.OP_LATENT_BLEND
N = 6 * 28 * 50 * 4


def blend(**kw):
    """The op of a DDIM plan of one scene: 6 views of 28 x 50 x 4 latents, CFG, 16-bit x_in with 8 channels per pixel."""
    d = dict(x=P(1), cond=P(2), noise=P(3), mask=P(4), coef=P(5), step_ptr=P(6), x_in=P(7), n=N, mask_elems=4, coef_ld=4, col_a=2, col_s=3,
             last_step=19, cfg=1, xin_c=4, xin_ld=8)
    d.update(kw); return d


# (sentence of include/mdx.h, descriptor, what mdx_last_error() must name)
TABLE = [
    ("x, cond, noise, mask, coef, step_ptr not NULL", blend(x=0), "x must not be NULL"),
    ("x, cond, noise, mask, coef, step_ptr not NULL", blend(cond=0), "cond must not be NULL"),
    ("x, cond, noise, mask, coef, step_ptr not NULL", blend(noise=0), "noise must not be NULL"),
    ("x, cond, noise, mask, coef, step_ptr not NULL", blend(mask=0), "mask must not be NULL"),
    ("x, cond, noise, mask, coef, step_ptr not NULL", blend(coef=0), "coef must not be NULL"),
    ("x, cond, noise, mask, coef, step_ptr not NULL", blend(step_ptr=0), "step_ptr must not be NULL"),
    ("x, cond, noise, mask, coef, step_ptr 4-byte aligned", blend(x=P(1) + 2), "x must be 4-byte"),
    ("x, cond, noise, mask, coef, step_ptr 4-byte aligned", blend(cond=P(2) + 1), "cond must be 4-byte"),
    ("x, cond, noise, mask, coef, step_ptr 4-byte aligned", blend(noise=P(3) + 2), "noise must be 4-byte"),
    ("x, cond, noise, mask, coef, step_ptr 4-byte aligned", blend(mask=P(4) + 3), "mask must be 4-byte"),
    ("x, cond, noise, mask, coef, step_ptr 4-byte aligned", blend(coef=P(5) + 2), "coef must be 4-byte"),
    ("x, cond, noise, mask, coef, step_ptr 4-byte aligned", blend(step_ptr=P(6) + 2), "step_ptr must be 4-byte"),
    ("x_in at its element's alignment (4 / 2 bytes)", blend(x_in=P(7) + 1), "x_in must be 2-byte"),
    ("x_in at its element's alignment (4 / 2 bytes)", blend(x_in=P(7) + 2, xin_ld=0, xin_c=0), "x_in must be 4-byte"),
    ("n not negative", blend(n=-4), "n=-4"),
    ("mask_elems >= 1 and divides n", blend(mask_elems=0), "mask_elems=0"),
    ("mask_elems >= 1 and divides n", blend(mask_elems=-4), "mask_elems=-4"),
    ("mask_elems >= 1 and divides n", blend(mask_elems=9), "mask_elems=9"),
    ("0 <= col_a, col_s < coef_ld", blend(col_a=4), "col_a=4"),
    ("0 <= col_a, col_s < coef_ld", blend(col_a=-1), "col_a=-1"),
    ("0 <= col_a, col_s < coef_ld", blend(col_s=4), "col_s=4"),
    ("0 <= col_a, col_s < coef_ld", blend(col_s=-2), "col_s=-2"),
    ("0 <= col_a, col_s < coef_ld", blend(coef_ld=0, col_a=0, col_s=0), "col_a=0"),
    ("cfg in {0, 1}", blend(cfg=2), "cfg=2"),
    ("cfg in {0, 1}", blend(cfg=-1), "cfg=-1"),
    ("xin_c, xin_ld, coef_ld, last_step fit a 32-bit int", blend(xin_c=BIG), "xin_c="),
    ("xin_c, xin_ld, coef_ld, last_step fit a 32-bit int", blend(xin_ld=BIG), "xin_ld="),
    ("xin_c, xin_ld, coef_ld, last_step fit a 32-bit int", blend(coef_ld=BIG), "coef_ld="),
    ("xin_c, xin_ld, coef_ld, last_step fit a 32-bit int", blend(last_step=BIG), "last_step="),
    ("xin_ld is not negative", blend(xin_ld=-8), "xin_ld=-8"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", blend(xin_c=0), "xin_c=0"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", blend(xin_c=-4), "xin_c=-4"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", blend(xin_c=16), "xin_c=16"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", blend(xin_c=11, xin_ld=16), "xin_c=11"),
]


def _desc(fields):
    d = L.MdxBlendDesc()
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
        assert "mdx_latent_blend_f16" in msg, msg


@no_device
@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("fields", [blend(n=0), blend(n=0, x_in=0), blend(n=0, xin_ld=0, xin_c=0, cfg=0), blend(n=0, coef_ld=12, col_a=10, col_s=11)],
                         ids=["n0", "n0-no-x_in", "n0-fp32-x_in", "n0-unipc"])
def test_empty_problem_launches_nothing(fields, path):
    """n == 0 returns MDX_OK before any launch: on a machine without a device a launch attempt would come back MDX_ELAUNCH."""
    rc, msg = _call(path, _desc(fields))
    assert rc == OK, f"rc={rc}: {msg!r}"


@no_device
def test_an_empty_problem_is_still_checked():
    rc, msg = _call("bf16", _desc(blend(n=0, x=P(1) + 2)))
    assert rc == EINVAL and "x must be 4-byte" in msg
    rc, msg = _call("bf16", _desc(blend(n=0, cfg=3)))
    assert rc == EINVAL and "cfg=3" in msg


def test_every_host_check_has_a_row():
    """Every field a check of the entry point (or of a shared helper of csrc/latent.h it calls) names is named by a row, and every sentence
    the table quotes stands in the header."""
    from test_contract import with_latent_helpers
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    body = with_latent_helpers(open(os.path.join(root, "magicdrive_amd", "csrc", "blend.hip")).read().split('extern "C" int mdx_latent_blend_bf16(')[1])
    fields = set(re.findall(r'need_\w+\(op, "([A-Za-z_]+)"', body)) | set(re.findall(r'"%s: (\w+)=%ld', body)) | set(re.findall(r'"%s: (\w+) must not be NULL"', body))
    assert fields == {"x", "cond", "noise", "mask", "coef", "step_ptr", "x_in", "n", "mask_elems", "coef_ld", "col_a", "col_s", "last_step", "cfg",
                      "xin_c", "xin_ld"}, fields
    names = [n for _, _, n in TABLE]
    covered = {f for f in fields if any(n.startswith(f + "=") or n.startswith(f + " must") for n in names)}
    assert fields == covered, sorted(fields - covered)
    flat = re.sub(r"[\s*]+", " ", open(os.path.join(root, "include", "mdx.h")).read())
    for clause in {c for c, _, _ in TABLE}:
        assert re.sub(r"[\s*]+", " ", clause) in flat, clause


def test_binding_matches_the_header(tmp_path):
    """sizeof / offsetof of MdxBlendDesc in the C header equal the ctypes mirror's; the opcode and both symbols are declared and exported;
    the ABI version is still 12 and the op is not a row of DESC_OF_OP."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mdx.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(MdxBlendDesc), '
                 'offsetof(MdxBlendDesc, step_ptr), offsetof(MdxBlendDesc, x_in), offsetof(MdxBlendDesc, n), offsetof(MdxBlendDesc, xin_ld), '
                 'MDX_OP_LATENT_BLEND);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(c), "-o", str(exe)], check=True)
    size, o_step, o_xin, o_n, o_ld, code = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    S = L.MdxBlendDesc
    assert (size, o_step, o_xin, o_n, o_ld) == (ctypes.sizeof(S), S.step_ptr.offset, S.x_in.offset, S.n.offset, S.xin_ld.offset) and size == 16 * 8
    assert [f[0] for f in S._fields_] == "x cond noise mask coef step_ptr x_in n mask_elems coef_ld col_a col_s last_step cfg xin_c xin_ld".split()
    assert size <= L.OP_BYTES - 16
    assert code == L.OP_LATENT_BLEND == 18 and L.ENTRY_OF_OP[L.OP_LATENT_BLEND] == "mdx_latent_blend_bf16"
    assert {"mdx_latent_blend_bf16", "mdx_latent_blend_f16"} <= set(L.EXPORTS)
    assert L.OP_LATENT_BLEND not in L.DESC_OF_OP
    assert L.lib().mdx_abi_version() == 12 and L.ABI_VERSION == 12


def test_op_record_checks_and_flops():
    """ops.LatentBlend.lower() on CPU views: the plan's fields reach the descriptor, the columns follow the table's width, bad records
    raise; flops.op_flops is 0 and op_bytes counts every operand once (x twice: read and written)."""
    from magicdrive_amd import flops as FL
    from magicdrive_amd import ops as O
    views, h, w, C = 12, 3, 5, 4
    n = views * h * w * C
    x, cond, noise = (torch.zeros(n) for _ in range(3))
    mask = torch.zeros(views * h * w)
    step = torch.zeros(1, dtype=torch.int32)
    x_in = torch.zeros(2 * views * h * w, 8, dtype=torch.float16)
    for ld, cols in ((4, (2, 3)), (12, (10, 11))):
        op = O.LatentBlend(x, cond, noise, mask, torch.zeros(20, ld), step, last_step=19, x_in=x_in, cfg=True, xin_c=C)
        code, d = op.lower()
        assert code == L.OP_LATENT_BLEND and (d.n, d.mask_elems, d.coef_ld, d.col_a, d.col_s, d.last_step, d.cfg, d.xin_c, d.xin_ld) == (n, C, ld, *cols, 19, 1, C, 8)
        assert O.dtype_code(op) == L.DTYPE_F16 and FL.op_flops(op) == 0.0
        assert FL.op_bytes(op) == 4 * (4 * n + mask.numel()) + 2 * x_in.numel() and FL.kernel_family(op) == "elementwise"
    flat = O.LatentBlend(x, cond, noise, mask, torch.zeros(20, 4), step, last_step=19, x_in=torch.zeros(n), col_a=0, col_s=1)
    d = flat.lower()[1]
    assert (d.xin_ld, d.xin_c, d.cfg, d.col_a, d.col_s) == (0, 0, 0, 0, 1) and O.dtype_code(flat) == L.DTYPE_BF16
    for bad in (dict(mask=torch.zeros(7)), dict(mask=mask.double()), dict(coef=torch.zeros(20, 5)), dict(cond=torch.zeros(n - 4)),
                dict(x_in=torch.zeros(n)), dict(x_in=x_in[:-1]), dict(step=torch.zeros(1, dtype=torch.int64)), dict(col_a=4, col_s=3)):
        kw = dict(x=x, cond=cond, noise=noise, mask=mask, coef=torch.zeros(20, 4), step=step, last_step=19, x_in=x_in, cfg=True, xin_c=C)
        kw.update(bad)
        with pytest.raises(ValueError):
            O.LatentBlend(**kw).lower()
