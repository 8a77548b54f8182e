"""CPU: the host-side contract of mdx_group_stats_* (include/mdx.h: MdxStatsDesc), table-driven like tests/test_contract.py.

One valid descriptor and, per clause, ONE mutation that violates only that clause: it must come back MDX_EINVAL with a message naming the
field — through the bf16 symbol, the _f16 symbol and a one-op mdx_program_run.  Pointers are plain integers with the wanted alignment: a
missing check shows up as a launch attempt (MDX_ELAUNCH on a machine without a device), never as a memory access; for that reason the
rejection table refuses to run where a device is visible and the valid descriptor is only ever called with G == 0 or n == 0, where the
contract says nothing is launched.
"""
import ctypes
import os
import re

import pytest
import torch

from magicdrive_amd import _lib as L

no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: must not run where a launch could succeed")

EINVAL, ELAUNCH = -1, -2
BIG = 1 << 31
P = lambda k: 0x10000000 * k        # fake, 256 MiB apart, aligned to everything
OP = L.OP_GROUP_STATS


def stats(**kw):
    d = dict(X=P(1), out=P(2), G=6, n=5600, sG=5600, n_rows=1, f32=1)
    d.update(kw); return d


# (clause of include/mdx.h, descriptor, what mdx_last_error() must name)
TABLE = [
    ("X and out not NULL", stats(X=0), "null operand"),
    ("X and out not NULL", stats(out=0), "null operand"),
    ("f32 in {0, 1}", stats(f32=2), "f32=2"),
    ("f32 in {0, 1}", stats(f32=-1), "f32=-1"),
    ("0 <= n <= 2^24", stats(n=(1 << 24) + 1), "n=16777217"),
    ("0 <= n <= 2^24", stats(n=-1), "n=-1"),
    ("0 <= n <= 2^24", stats(n=BIG), "n="),
    ("0 <= G fits a 32-bit int", stats(G=-1), "G=-1"),
    ("0 <= G fits a 32-bit int", stats(G=BIG), "G="),
    ("sG >= 0", stats(sG=-8), "sG=-8"),
    ("X at its element's natural alignment (4 / 2 bytes)", stats(X=P(1) + 2), "X must be 4-byte"),
    ("X at its element's natural alignment (4 / 2 bytes)", stats(X=P(1) + 1, f32=0), "X must be 2-byte"),
    ("out 16-byte aligned", stats(out=P(2) + 8), "out must be 16-byte"),
    ("out 16-byte aligned", stats(out=P(2) + 4), "out must be 16-byte"),
    ("row_dev 4-byte aligned", stats(row_dev=P(3) + 2, n_rows=4), "row_dev must be 4-byte"),
    ("1 <= n_rows fits a 32-bit int", stats(row_dev=P(3), n_rows=0), "n_rows=0"),
    ("1 <= n_rows fits a 32-bit int", stats(row_dev=P(3), n_rows=-3), "n_rows=-3"),
    ("1 <= n_rows fits a 32-bit int", stats(row_dev=P(3), n_rows=BIG), "n_rows="),
]


def _desc(fields):
    d = L.MdxStatsDesc()
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


@no_device
@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("fields", [stats(G=0), stats(n=0), stats(G=0, f32=0), stats(n=0, row_dev=P(3), n_rows=4)], ids=["G0", "n0", "G0-16bit", "n0-rows"])
def test_empty_problem_launches_nothing(fields, path):
    """G == 0 or n == 0 returns MDX_OK before any launch: on a machine without a device a launch attempt would come back MDX_ELAUNCH."""
    rc, msg = _call(path, _desc(fields))
    assert rc == 0, f"rc={rc}: {msg!r}"


@no_device
def test_an_empty_problem_is_still_checked():
    rc, msg = _call("bf16", _desc(stats(G=0, out=P(2) + 8)))
    assert rc == EINVAL and "out must be 16-byte" in msg


def test_every_host_check_has_a_row():
    """Every field a need_* call of the entry point names is named by a row, and every clause the table quotes stands in the header."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    body = open(os.path.join(root, "magicdrive_amd", "csrc", "stats.hip")).read().split('extern "C" int mdx_group_stats_bf16(')[1]
    fields = set(re.findall(r'need_\w+\(op, "([^"]+)"', body)) | set(re.findall(r'"%s: (\w+)=%ld', body))
    assert fields == {"X", "out", "row_dev", "n_rows", "G", "n", "sG", "f32"}, fields
    names = [n for _, _, n in TABLE]
    missing = sorted(f for f in fields if not any(n.startswith(f + "=") or n.startswith(f + " must be") for n in names))
    assert not missing, missing
    flat = re.sub(r"[\s*]+", " ", open(os.path.join(root, "include", "mdx.h")).read())
    for clause, _, _ in TABLE:
        assert clause in flat, clause


def test_binding_matches_the_header(tmp_path):
    """sizeof(MdxStatsDesc) of the C header equals the ctypes mirror's; the opcode and both symbols are declared and exported."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mdx.h"\nint main(){printf("%zu %zu %zu %d\\n", sizeof(MdxStatsDesc), '
                 'offsetof(MdxStatsDesc, G), offsetof(MdxStatsDesc, f32), MDX_OP_GROUP_STATS);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(c), "-o", str(exe)], check=True)
    size, off_g, off_f32, code = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (size, off_g, off_f32) == (ctypes.sizeof(L.MdxStatsDesc), L.MdxStatsDesc.G.offset, L.MdxStatsDesc.f32.offset)
    assert code == L.OP_GROUP_STATS and L.ENTRY_OF_OP[L.OP_GROUP_STATS] == "mdx_group_stats_bf16"
    assert {"mdx_group_stats_bf16", "mdx_group_stats_f16"} <= set(L.EXPORTS)
    assert L.lib().mdx_abi_version() == 12
