"""CPU: the host contract of the attention routes that do not start in attention.hip's own checks — the short-sequence route (causal /
v_rowmajor, csrc/attention_short.hip), the context route (tk_dev, csrc/attention_ctx.hip) and its per-batch entry point
mdx_attention_ctx_rows_*.

ONE table of layout violations (csrc/attn.h: need_attn_layout, the checks every attention route shares) is applied to a valid descriptor of
each route, and one table per route holds the route's own clauses.  Each row breaks exactly one check and records the code and the message
text behind the entry point's name as they were before the routes shared one entry point and one check block; bf16 symbol, _f16 symbol and
a one-op mdx_program_run.  Pointers are plain integers (as in tests/test_contract.py): the tests refuse to run where a device is visible.
"""
import ctypes

import pytest
import torch

from magicdrive_amd import _lib as L

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: must not run where a launch could succeed")

EINVAL, EUNSUPPORTED = -1, -3
BIG = 1 << 31
P = lambda k: 0x10000000 * k        # fake, 256 MiB apart, aligned to everything

# route -> (opcode, a valid descriptor)
_BASE = dict(Q=P(1), K=P(2), Vt=P(3), O=P(4), B=2, H=2, Tq=8, Tk=8, nsrc=1, scale=0.25)
ROUTES = {
    "short": (L.OP_ATTN, dict(_BASE, d=32, v_rowmajor=1, ldq=192, ldk=192, ldv=192, ldo=64, sQ=1536, sK=1536, sV=1536, sO=512)),
    "ctx": (L.OP_ATTN, dict(_BASE, d=16, tk_dev=P(6), ldq=32, ldk=32, ldv=8, ldo=32, sQ=256, sK=256, sV=256, sO=256)),
    "rows": (L.OP_ATTN_ROWS, dict(_BASE, d=16, tk_dev=P(6), ldq=32, ldk=32, ldv=8, ldo=32, sQ=256, sK=256, sV=256, sO=256)),
}

# (mutation, text behind "<entry point>: "): need_attn_layout
LAYOUT = [
    (dict(B=BIG), "B=%d does not fit a 32-bit int" % BIG), (dict(H=BIG), "H=%d does not fit a 32-bit int" % BIG),
    (dict(Tq=BIG), "Tq=%d does not fit a 32-bit int" % BIG), (dict(Tk=BIG), "Tk=%d does not fit a 32-bit int" % BIG),
    (dict(ldq=100), "ldq=100 must be a multiple of 8"), (dict(ldk=100), "ldk=100 must be a multiple of 8"), (dict(ldv=196), "ldv=196 must be a multiple of 8"),
    (dict(sQ=2052), "sQ=2052 must be a multiple of 8"), (dict(sK=2052), "sK=2052 must be a multiple of 8"), (dict(sV=2052), "sV=2052 must be a multiple of 8"),
    (dict(ldo=66), "ldo=66 must be a multiple of 4"), (dict(sO=1026), "sO=1026 must be a multiple of 4"),
    (dict(Q=P(1) + 8), "Q must be 16-byte aligned"), (dict(K=P(2) + 8), "K must be 16-byte aligned"), (dict(Vt=P(3) + 8), "Vt must be 16-byte aligned"),
    (dict(O=P(4) + 4), "O must be 8-byte aligned"),
]

# (route, mutation, code, text behind "<entry point>: ")
OWN = [
    ("short", dict(causal=2), EINVAL, "causal=2 must be 0 or 1"),
    ("short", dict(v_rowmajor=3), EINVAL, "v_rowmajor=3 must be 0 or 1"),
    ("short", dict(causal=1, v_rowmajor=0), EINVAL, "causal needs v_rowmajor == 1 (the short-sequence kernel)"),
    ("short", dict(K=0), EINVAL, "null operand"),
    ("short", dict(nsrc=2, kvmap=P(5)), EINVAL, "v_rowmajor needs nsrc == 1 (nsrc=2)"),
    ("short", dict(joint=1), EINVAL, "v_rowmajor needs joint == 0 (joint=1)"),
    ("short", dict(q_prescaled=1), EINVAL, "v_rowmajor needs q_prescaled == 0 (q_prescaled=1)"),
    ("short", dict(causal=1, Tk=16), EINVAL, "causal needs Tq == Tk (Tq=8, Tk=16)"),
    ("short", dict(d=36), EINVAL, "head dim d=36 must be a positive multiple of 8"),
    ("short", dict(d=0), EINVAL, "head dim d=0 must be a positive multiple of 8"),
    ("short", dict(d=40), EUNSUPPORTED, "v_rowmajor: head dim d=40 has no short-sequence kernel instance (d in {32, 64})"),
    ("short", dict(causal=1, Tq=136, Tk=136), EUNSUPPORTED, "v_rowmajor: Tq=136, Tk=136: the short-sequence kernel serves Tq, Tk <= 128"),
    ("short", dict(Tk=129), EUNSUPPORTED, "v_rowmajor: Tq=8, Tk=129: the short-sequence kernel serves Tq, Tk <= 128"),
    ("short", dict(ldv=56), EINVAL, "v_rowmajor: ldv=56 < H * d"),
    ("short", dict(B=1 << 16, H=1 << 16, ldv=1 << 21), EINVAL, "B * H=%d does not fit a 32-bit int" % (1 << 32)),
    ("ctx", dict(nsrc=2), EINVAL, "tk_dev needs nsrc == 1 (nsrc=2)"),
    ("ctx", dict(joint=1), EINVAL, "tk_dev needs joint == 0 (joint=1)"),
    ("ctx", dict(causal=1), EINVAL, "tk_dev needs causal == 0 (causal=1)"),
    ("ctx", dict(v_rowmajor=1), EINVAL, "tk_dev needs v_rowmajor == 0 (v_rowmajor=1): the V^T operand"),
    ("ctx", dict(q_prescaled=2), EINVAL, "q_prescaled=2 must be 0 or 1"),
    ("ctx", dict(scale=0.0), EINVAL, "tk_dev: scale=0 must be positive (or q_prescaled == 1)"),
    ("ctx", dict(scale=-0.25), EINVAL, "tk_dev: scale=-0.25 must be positive (or q_prescaled == 1)"),
    ("ctx", dict(O=0), EINVAL, "null operand"),
    ("ctx", dict(tk_dev=P(6) + 2), EINVAL, "tk_dev must be 4-byte aligned"),
    ("ctx", dict(d=12), EINVAL, "head dim d=12 must be a positive multiple of 8"),
    ("ctx", dict(d=24), EUNSUPPORTED, "tk_dev: head dim d=24 has no context-attention kernel instance (d in {16, 32, 40, 80, 160})"),
    ("ctx", dict(Tk=16), EINVAL, "tk_dev: ldv=8 < Tk=16 (Tk is the capacity)"),
    ("ctx", dict(B=1 << 16, H=1 << 16), EINVAL, "B * H * ceil(Tq / 128)=%d does not fit a 32-bit int" % (1 << 32)),
    ("rows", dict(tk_dev=0), EINVAL, "tk_dev is NULL: this entry point takes the device address of int32 [B] key counts"),
    ("rows", dict(kvmap=P(5)), EINVAL, "tk_dev needs kvmap == NULL (batch b of Q attends to batch b of K / V^T)"),
    ("rows", dict(nsrc=2), EINVAL, "tk_dev needs nsrc == 1 (nsrc=2)"),
    ("rows", dict(scale=0.0), EINVAL, "tk_dev: scale=0 must be positive (or q_prescaled == 1)"),
    ("rows", dict(tk_dev=P(6) + 2), EINVAL, "tk_dev must be 4-byte aligned"),
    ("rows", dict(d=24), EUNSUPPORTED, "tk_dev: head dim d=24 has no context-attention kernel instance (d in {16, 32, 40, 80, 160})"),
    ("rows", dict(B=1 << 16, H=1 << 16), EINVAL, "B * H * ceil(Tq / 128)=%d does not fit a 32-bit int" % (1 << 32)),
]
ROWS = [(r, m, EINVAL, t) for r in ROUTES for m, t in LAYOUT] + OWN
_IDS = [f"{r}-{i}-{t[:40]}" for i, (r, _, _, t) in enumerate(ROWS)]


def _call(path, route, mutation):
    opcode, fields = ROUTES[route]
    d = L.MdxAttnDesc()
    names = {f[0] for f in d._fields_}
    for k, v in {**fields, **mutation}.items():
        assert k in names, k
        setattr(d, k, v)
    lib = L.lib()
    if path == "program":
        prog = L.Program([(opcode, d, L.DTYPE_BF16)])
        rc = lib.mdx_program_run(ctypes.byref(prog.buf), 1, None)
    else:
        rc = getattr(lib, L.entry_name(opcode, L.DTYPE_F16 if path == "f16" else L.DTYPE_BF16))(ctypes.byref(d), None)
    return opcode, rc, (lib.mdx_last_error() or b"").decode()


@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("route,mutation,code,text", ROWS, ids=_IDS)
def test_single_violation_code_and_message(route, mutation, code, text, path):
    opcode, rc, msg = _call(path, route, mutation)
    assert rc == code, f"{route} via {path}: rc={rc} (want {code}): {msg!r}"
    entry = L.entry_name(opcode, L.DTYPE_F16 if path == "f16" else L.DTYPE_BF16)
    assert msg.endswith(f"{entry}: {text}"), f"{route} via {path}: {msg!r}"
    if path == "program":
        assert msg.startswith("op 0 (opcode %d)" % opcode), msg


def test_null_descriptor():
    lib = L.lib()
    for name, text in (("mdx_attention_bf16", "mdx_attention_bf16: null operand"), ("mdx_attention_f16", "mdx_attention_bf16: null operand"),
                       ("mdx_attention_ctx_rows_bf16", "mdx_attention_ctx_rows_bf16: null descriptor"),
                       ("mdx_attention_ctx_rows_f16", "mdx_attention_ctx_rows_f16: null descriptor")):
        assert getattr(lib, name)(None, None) == EINVAL
        assert (lib.mdx_last_error() or b"").decode() == text, name
