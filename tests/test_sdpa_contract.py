"""CPU: the host-side contract of mdx_sdpa_* (include/mdx.h: MdxSdpaDesc), table-driven like tests/test_group_stats_contract.py.

One valid descriptor and, per sentence of the header contract, ONE mutation that violates only that sentence: it must come back with the
stated code and a message naming the field — through the bf16 symbol, the _f16 symbol and a one-op mdx_program_run.  Pointers are plain
integers with the wanted alignment: a missing check shows up as a launch attempt (MDX_ELAUNCH on a machine without a device), never as a
memory access; for that reason the tables refuse to run where a device is visible, and the valid descriptor is only ever called with B or
Tq equal to 0, where the contract says nothing is launched.
"""
import ctypes
import os
import re

import pytest
import torch

from magicdrive_amd import _lib as L

no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: must not run where a launch could succeed")

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
BIG = 1 << 31
P = lambda k: 0x10000000 * k        # fake, 256 MiB apart, aligned to everything
OP = L.OP_SDPA
H, D, T = 8, 40, 100
C3 = 3 * H * D


def sdpa(**kw):
    """Q, K, V the column blocks of one [B][T][3 H d] buffer, O a buffer of its own."""
    d = dict(Q=P(1), K=P(1) + 2 * H * D, V=P(1) + 4 * H * D, O=P(2), B=2, H=H, Tq=T, Tk=T, d=D,
             ldq=C3, sQ=T * C3, ldk=C3, sK=T * C3, ldv=C3, sV=T * C3, ldo=H * D, sO=T * H * D, scale=D ** -0.5, causal=0)
    d.update(kw); return d


# (sentence of include/mdx.h, descriptor, return code, what mdx_last_error() must name)
TABLE = [
    ("Q, K, V, O not NULL", sdpa(Q=0), EINVAL, "null operand"),
    ("Q, K, V, O not NULL", sdpa(K=0), EINVAL, "null operand"),
    ("Q, K, V, O not NULL", sdpa(V=0), EINVAL, "null operand"),
    ("Q, K, V, O not NULL", sdpa(O=0), EINVAL, "null operand"),
    ("any other d returns MDX_EUNSUPPORTED", sdpa(d=4, H=8, ldo=32), EUNSUPPORTED, "d=4"),
    ("any other d returns MDX_EUNSUPPORTED", sdpa(d=12), EUNSUPPORTED, "d=12"),
    ("any other d returns MDX_EUNSUPPORTED", sdpa(d=168, H=1), EUNSUPPORTED, "d=168"),
    ("any other d returns MDX_EUNSUPPORTED", sdpa(d=104, H=1), EUNSUPPORTED, "d=104"),
    ("any other d returns MDX_EUNSUPPORTED", sdpa(d=112, H=1), EUNSUPPORTED, "d=112"),
    ("any other d returns MDX_EUNSUPPORTED", sdpa(d=136, H=1), EUNSUPPORTED, "d=136"),
    ("any other d returns MDX_EUNSUPPORTED", sdpa(d=144, H=1), EUNSUPPORTED, "d=144"),
    ("any other d returns MDX_EUNSUPPORTED", sdpa(d=0), EUNSUPPORTED, "d=0"),
    ("Q, K, V 16-byte aligned", sdpa(Q=P(1) + 8), EINVAL, "Q must be 16-byte"),
    ("Q, K, V 16-byte aligned", sdpa(K=P(1) + 2 * H * D + 8), EINVAL, "K must be 16-byte"),
    ("Q, K, V 16-byte aligned", sdpa(V=P(1) + 4 * H * D + 2), EINVAL, "V must be 16-byte"),
    ("O 8-byte aligned", sdpa(O=P(2) + 4), EINVAL, "O must be 8-byte"),
    ("klen_dev 4-byte aligned", sdpa(klen_dev=P(3) + 2), EINVAL, "klen_dev must be 4-byte"),
    ("ldq, ldk, ldv, sQ, sK, sV multiples of 8", sdpa(ldq=C3 + 4), EINVAL, "ldq="),
    ("ldq, ldk, ldv, sQ, sK, sV multiples of 8", sdpa(ldk=C3 + 4), EINVAL, "ldk="),
    ("ldq, ldk, ldv, sQ, sK, sV multiples of 8", sdpa(ldv=C3 + 4), EINVAL, "ldv="),
    ("ldq, ldk, ldv, sQ, sK, sV multiples of 8", sdpa(sQ=T * C3 + 4), EINVAL, "sQ="),
    ("ldq, ldk, ldv, sQ, sK, sV multiples of 8", sdpa(sK=T * C3 + 2), EINVAL, "sK="),
    ("ldq, ldk, ldv, sQ, sK, sV multiples of 8", sdpa(sV=T * C3 + 1), EINVAL, "sV="),
    ("ldo, sO multiples of 4", sdpa(ldo=H * D + 2), EINVAL, "ldo="),
    ("ldo, sO multiples of 4", sdpa(sO=T * H * D + 2), EINVAL, "sO="),
    ("ldq, ldk, ldv, ldo >= H*d", sdpa(ldq=H * D - 8), EINVAL, "ldq="),
    ("ldq, ldk, ldv, ldo >= H*d", sdpa(ldk=H * D - 8), EINVAL, "ldk="),
    ("ldq, ldk, ldv, ldo >= H*d", sdpa(ldv=H * D - 8), EINVAL, "ldv="),
    ("ldq, ldk, ldv, ldo >= H*d", sdpa(ldo=H * D - 8), EINVAL, "ldo="),
    ("causal in {0, 1}", sdpa(causal=2), EINVAL, "causal=2"),
    ("causal in {0, 1}", sdpa(causal=-1), EINVAL, "causal=-1"),
    ("causal == 1 needs Tq == Tk", sdpa(causal=1, Tq=T, Tk=T + 1), EINVAL, "causal needs Tq == Tk"),
    ("B, H, Tq, Tk fit a 32-bit int", sdpa(B=BIG), EINVAL, "B="),
    ("B, H, Tq, Tk fit a 32-bit int", sdpa(Tq=BIG), EINVAL, "Tq="),
    ("B, H, Tq, Tk fit a 32-bit int", sdpa(Tk=BIG), EINVAL, "Tk="),
    ("are not negative", sdpa(B=-1), EINVAL, "B=-1"),
    ("are not negative", sdpa(Tk=-3), EINVAL, "Tk=-3"),
]


def _desc(fields):
    d = L.MdxSdpaDesc()
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
@pytest.mark.parametrize("clause,fields,code,names", TABLE, ids=[f"{i}-{n}" for i, (_, _, _, n) in enumerate(TABLE)])
def test_violation_is_rejected_on_the_host(clause, fields, code, names, path):
    rc, msg = _call(path, _desc(fields))
    assert rc == code, f"[{clause}] via {path}: rc={rc} (want {code}): {msg!r}"
    assert names in msg, f"[{clause}] via {path}: message {msg!r} does not name {names!r}"
    if path == "program":
        assert msg.startswith("op 0 (opcode %d)" % OP), msg
    elif path == "f16":
        assert "mdx_sdpa_f16" in msg, msg


@no_device
@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("fields", [sdpa(B=0), sdpa(Tq=0), sdpa(Tk=0), sdpa(H=0), sdpa(B=0, causal=1), sdpa(Tq=0, klen_dev=P(3))],
                         ids=["B0", "Tq0", "Tk0", "H0", "B0-causal", "Tq0-klen"])
def test_empty_problem_launches_nothing(fields, path):
    """B, H, Tq or Tk equal to 0 returns MDX_OK before any launch: on a machine without a device a launch attempt would come back MDX_ELAUNCH."""
    rc, msg = _call(path, _desc(fields))
    assert rc == OK, f"rc={rc}: {msg!r}"


@no_device
def test_an_empty_problem_is_still_checked():
    rc, msg = _call("bf16", _desc(sdpa(B=0, O=P(2) + 4)))
    assert rc == EINVAL and "O must be 8-byte" in msg
    rc, msg = _call("bf16", _desc(sdpa(Tq=0, d=12)))
    assert rc == EUNSUPPORTED and "d=12" in msg


@no_device
def test_mdx_attention_keeps_its_refusals():
    """The new symbol is additive: v_rowmajor with T = 129 or d = 40 is still MDX_EUNSUPPORTED on mdx_attention_*."""
    for kw in (dict(Tq=129, Tk=129, d=64), dict(Tq=77, Tk=77, d=40)):
        a = L.MdxAttnDesc()
        a.Q, a.K, a.Vt, a.O = P(1), P(2), P(3), P(4)
        a.B, a.H, a.nsrc, a.v_rowmajor, a.scale = 1, 2, 1, 1, 0.125
        a.Tq, a.Tk, a.d = kw["Tq"], kw["Tk"], kw["d"]
        a.ldq = a.ldk = a.ldv = a.ldo = 2 * kw["d"]
        a.sQ = a.sK = a.sV = a.sO = 2 * kw["d"] * kw["Tq"]
        assert L.lib().mdx_attention_bf16(ctypes.byref(a), None) == EUNSUPPORTED


def test_every_host_check_has_a_row():
    """Every field a check of the entry point names is named by a row, and every sentence the table quotes stands in the header."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    body = open(os.path.join(root, "magicdrive_amd", "csrc", "attention_vrow.hip")).read().split('extern "C" int mdx_sdpa_bf16(')[1]
    fields = set(re.findall(r'need_\w+\(op, "([A-Za-z_]+)"', body)) | set(re.findall(r'"%s: (?:head dim )?(\w+)=%ld', body))
    assert fields == {"Q", "K", "V", "O", "klen_dev", "B", "H", "Tq", "Tk", "d", "ldq", "ldk", "ldv", "ldo", "sQ", "sK", "sV", "sO", "causal"}, fields
    names = [n for _, _, _, n in TABLE]
    covered = {f for f in fields if any(n.startswith(f + "=") or n.startswith(f + " must be") for n in names)}
    assert fields - covered <= {"H"}, sorted(fields - covered)      # H shares the 32-bit / sign checks of B (rows "B=")
    flat = re.sub(r"[\s*]+", " ", open(os.path.join(root, "include", "mdx.h")).read())
    for clause in {c for c, _, _, _ in TABLE}:
        assert re.sub(r"[\s*]+", " ", clause) in flat, clause


def test_binding_matches_the_header(tmp_path):
    """sizeof / offsetof of MdxSdpaDesc in the C header equal the ctypes mirrors' (_lib and the integration stub); the opcode and both
    symbols are declared and exported; the ABI version is still 12 and the op is not a row of DESC_OF_OP."""
    import subprocess
    from magicdrive_amd.integration import attn_processor as AP
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mdx.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(MdxSdpaDesc), '
                 'offsetof(MdxSdpaDesc, klen_dev), offsetof(MdxSdpaDesc, B), offsetof(MdxSdpaDesc, scale), offsetof(MdxSdpaDesc, causal), '
                 'MDX_OP_SDPA);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(c), "-o", str(exe)], check=True)
    size, o_klen, o_b, o_scale, o_causal, code = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    for S in (L.MdxSdpaDesc, AP.MdxSdpaDesc):
        assert (size, o_klen, o_b, o_scale, o_causal) == (ctypes.sizeof(S), S.klen_dev.offset, S.B.offset, S.scale.offset, S.causal.offset)
        assert [f[0] for f in S._fields_] == "Q K V O klen_dev B H Tq Tk d ldq sQ ldk sK ldv sV ldo sO scale causal".split()
    assert size <= L.OP_BYTES - 16
    assert code == L.OP_SDPA == 17 and L.ENTRY_OF_OP[L.OP_SDPA] == "mdx_sdpa_bf16"
    assert {"mdx_sdpa_bf16", "mdx_sdpa_f16"} <= set(L.EXPORTS)
    assert L.OP_SDPA not in L.DESC_OF_OP
    assert L.lib().mdx_abi_version() == 12 and L.ABI_VERSION == 12


def test_op_record_checks_and_flops():
    """ops.Sdpa.lower() on CPU views: strides of a fused [B, T, 3C] buffer reach the descriptor; bad records raise; flops.op_flops counts
    4 B Tq Tk H d, halved under causal."""
    from magicdrive_amd import flops as FL
    from magicdrive_amd import ops as O
    B, Tq, C = 2, 10, 64
    qkv = torch.zeros(B, Tq, 3 * C, dtype=torch.bfloat16)
    o = torch.zeros(B, Tq, C, dtype=torch.bfloat16)
    op = O.Sdpa(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], o, heads=2, scale=0.5, causal=True)
    code, d = op.lower()
    assert code == L.OP_SDPA and (d.B, d.H, d.Tq, d.Tk, d.d, d.causal) == (B, 2, Tq, Tq, 32, 1)
    assert (d.ldq, d.ldk, d.ldv, d.ldo, d.sQ, d.sO) == (3 * C, 3 * C, 3 * C, C, Tq * 3 * C, Tq * C)
    assert d.K - d.Q == 2 * C and d.V - d.Q == 4 * C and not d.klen_dev and d.scale == 0.5
    assert FL.op_flops(op) == 4.0 * B * Tq * Tq * C / 2
    full = O.Sdpa(qkv[:, :, :C], qkv[:, :4, C:2 * C], qkv[:, :4, 2 * C:], o, heads=2, scale=0.5)
    assert FL.op_flops(full) == 4.0 * B * Tq * 4 * C and full.lower()[1].Tk == 4
    assert O.dtype_code(op) == L.DTYPE_BF16 and O.dtype_code(O.Sdpa(qkv.half(), qkv.half(), qkv.half(), o.half(), 2, 1.0)) == L.DTYPE_F16
    with pytest.raises(ValueError):
        O.Sdpa(qkv[:, :, :C], qkv[:, :4, C:2 * C], qkv[:, :4, 2 * C:], o, heads=2, scale=0.5, causal=True).lower()      # causal, Tq != Tk
    with pytest.raises(ValueError):
        O.Sdpa(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], o.float(), heads=2, scale=0.5).lower()            # one 16-bit type
    with pytest.raises(ValueError):
        O.Sdpa(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], o, heads=2, scale=0.5, klen=torch.zeros(B, dtype=torch.int64)).lower()
    with pytest.raises(RuntimeError):
        O.sdpa(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], 2)                                                 # CPU tensors
    with pytest.raises(TypeError):
        O.sdpa(qkv[:, :, :C].float(), qkv[:, :, C:2 * C].float(), qkv[:, :, 2 * C:].float(), 2)
