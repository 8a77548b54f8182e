"""CPU: the x_in contract that the four latent ops share (csrc/latent.h: need_xin; magicdrive_amd/ops.py: _lower_xin).

mdx_cfg_ddim_step, mdx_cfg_unipc_step, mdx_latent_blend_* and mdx_latent_renoise_* all refresh the model-input copy x_in, and one host
check and one lowering serve them.  Here ONE table of x_in violations is applied to a valid descriptor of each op — through the bf16
symbol, the _f16 symbol and a one-op mdx_program_run — and the message behind the op's name must be the same text for all four; ONE
accept / reject table of x_in tensors is applied to the four IR records.  Pointers of the descriptor tables are plain integers (as in
tests/test_contract.py): those tests refuse to run where a device is visible.
"""
import ctypes

import pytest
import torch

from magicdrive_amd import _lib as L
from magicdrive_amd import ops as O

no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: must not run where a launch could succeed")

EINVAL = -1
BIG = 1 << 31
P = lambda k: 0x10000000 * k        # fake, 256 MiB apart, aligned to everything
N = 6 * 28 * 50 * 4
XIN = dict(x_in=P(9), n=N, cfg=1, xin_c=4, xin_ld=8)       # 16-bit, 8 channels per pixel, both CFG halves

# op -> (opcode, descriptor type, name in messages, the op's own valid fields)
OPS = {
    "ddim": (L.OP_DDIM, L.MdxDdimDesc, "mdx_cfg_ddim_step", dict(x=P(1), eps=P(2), coef=P(3), step_ptr=P(4))),
    "unipc": (L.OP_UNIPC, L.MdxUniPCDesc, "mdx_cfg_unipc_step", dict(x=P(1), eps=P(2), coef=P(3), step_ptr=P(4), x_last=P(5), m1=P(6), m2=P(7))),
    "blend": (L.OP_LATENT_BLEND, L.MdxBlendDesc, "mdx_latent_blend",
              dict(x=P(1), cond=P(2), noise=P(3), mask=P(4), coef=P(5), step_ptr=P(6), mask_elems=4, coef_ld=4, col_a=2, col_s=3, last_step=19)),
    "renoise": (L.OP_LATENT_RENOISE, L.MdxRenoiseDesc, "mdx_latent_renoise",
                dict(x=P(1), coef=P(3), step_ptr=P(4), visit_ptr=P(5), seeds=P(6), group_elems=N // 6, jump=5, n_rows=20, coef_ld=4, col_t=0, col_p=2)),
}

# (clause of include/mdx.h, mutation of XIN, what mdx_last_error() must name)
VIOLATIONS = [
    ("xin_ld is not negative", dict(xin_ld=-8), "xin_ld=-8"),
    ("x_in at its element's alignment (4 / 2 bytes)", dict(x_in=P(9) + 1), "x_in must be 2-byte"),
    ("x_in at its element's alignment (4 / 2 bytes)", dict(x_in=P(9) + 2, xin_ld=0, xin_c=0), "x_in must be 4-byte"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", dict(xin_c=0), "xin_c=0"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", dict(xin_c=-4), "xin_c=-4"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", dict(xin_c=16), "xin_c=16"),
    ("xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n", dict(xin_c=11, xin_ld=16), "xin_c=11"),
    ("xin_c, xin_ld fit a 32-bit int", dict(xin_c=BIG), "xin_c=%d does not fit" % BIG),
    ("xin_c, xin_ld fit a 32-bit int", dict(xin_ld=BIG), "xin_ld=%d does not fit" % BIG),
]
_IDS = [f"{i}-{names}" for i, (_, _, names) in enumerate(VIOLATIONS)]


def _desc(op, mutation):
    _, cls, _, own = OPS[op]
    d = cls()
    names = {f[0] for f in d._fields_}
    for k, v in {**own, **XIN, **mutation}.items():
        assert k in names, (op, k)
        setattr(d, k, v)
    return d


def _call(path, op, d):
    lib, opcode = L.lib(), OPS[op][0]
    if path == "program":
        prog = L.Program([(opcode, d, L.DTYPE_BF16)])
        rc = lib.mdx_program_run(ctypes.byref(prog.buf), 1, None)
    else:
        fn = getattr(lib, L.entry_name(opcode, L.DTYPE_F16 if path == "f16" else L.DTYPE_BF16))
        rc = fn(ctypes.byref(d), None)
    return rc, (lib.mdx_last_error() or b"").decode()


@no_device
@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("clause,mutation,names", VIOLATIONS, ids=_IDS)
def test_x_in_violation_is_rejected_on_the_host(clause, mutation, names, op, path):
    rc, msg = _call(path, op, _desc(op, mutation))
    assert rc == EINVAL, f"{op} [{clause}] via {path}: rc={rc} (want {EINVAL}): {msg!r}"
    assert names in msg, f"{op} [{clause}] via {path}: message {msg!r} does not name {names!r}"
    if path == "program":
        assert msg.startswith("op 0 (opcode %d)" % OPS[op][0]), msg


@no_device
@pytest.mark.parametrize("clause,mutation,names", VIOLATIONS, ids=_IDS)
def test_the_message_is_the_same_for_the_four_ops(clause, mutation, names):
    tails = {}
    for op, (_, _, name, _) in OPS.items():
        rc, msg = _call("bf16", op, _desc(op, mutation))
        assert rc == EINVAL and msg.startswith(name + ": "), (op, rc, msg)
        tails[op] = msg[len(name) + 2:]
    assert len(set(tails.values())) == 1 and names in tails["ddim"], tails


def test_the_violation_clauses_stand_in_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdx.h")).read()
    ddim_block = re.sub(r"[\s*]+", " ", hdr.split("mdx_cfg_ddim_step — fused")[1].split("typedef struct MdxDdimDesc")[0])
    for clause in {c for c, _, _ in VIOLATIONS} - {"xin_c, xin_ld fit a 32-bit int"}:
        assert clause in ddim_block, clause
    assert "xin_c, xin_ld, gv_last_step fit a 32-bit int" in ddim_block


# ---- the IR records: one accept / reject table of x_in tensors --------------------------------------------------------------------
VIEWS, PIX, C = 2, 15, 4
NL = VIEWS * PIX * C                # latent elements


def _record(op, x_in, cfg, xin_c):
    f = lambda *s: torch.zeros(*s)
    step = torch.zeros(1, dtype=torch.int32)
    kw = dict(x_in=x_in, cfg=cfg, xin_c=xin_c)
    if op == "ddim":
        return O.DdimStep(f(NL), f((2 if cfg else 1) * NL), f(20, 4), step, **kw)
    if op == "unipc":
        return O.UniPCStep(f(NL), f((2 if cfg else 1) * NL), f(20, 12), step, f(NL), f(NL), f(NL), **kw)
    if op == "blend":
        return O.LatentBlend(f(NL), f(NL), f(NL), f(VIEWS * PIX), f(20, 4), step, last_step=19, **kw)
    return O.LatentRenoise(f(NL), f(20, 4), step, torch.zeros(1, dtype=torch.int32), torch.zeros(VIEWS, dtype=torch.int64), jump=2, **kw)


# name -> (x_in of c * NL latents, xin_c, lowered (xin_c, xin_ld))
ACCEPT = {
    "none": (lambda cn: None, C, (0, 0)),
    "fp32-flat": (lambda cn: torch.zeros(cn), C, (0, 0)),
    "bf16-ld4": (lambda cn: torch.zeros(cn // C, 4, dtype=torch.bfloat16), C, (C, 4)),
    "f16-ld4": (lambda cn: torch.zeros(cn // C, 4, dtype=torch.float16), C, (C, 4)),
    "bf16-ld8": (lambda cn: torch.zeros(cn // C, 8, dtype=torch.bfloat16), C, (C, 8)),
    "f16-ld8": (lambda cn: torch.zeros(cn // C, 8, dtype=torch.float16), C, (C, 8)),
}
REJECT = {
    "fp32-wrong-size": (lambda cn: torch.zeros(cn - C), C),
    "fp32-non-contiguous": (lambda cn: torch.zeros(2 * cn)[::2], C),
    "16-bit-1d": (lambda cn: torch.zeros(cn, dtype=torch.float16), C),
    "16-bit-column-slice": (lambda cn: torch.zeros(cn // C, 16, dtype=torch.float16)[:, :8], C),
    "xin_c-0": (lambda cn: torch.zeros(cn // C, 8, dtype=torch.float16), 0),
    "rows-times-xin_c": (lambda cn: torch.zeros(cn // C - 1, 8, dtype=torch.float16), C),
    "ld-below-xin_c": (lambda cn: torch.zeros(cn // C, 2, dtype=torch.float16), C),
    "float64": (lambda cn: torch.zeros(cn, dtype=torch.float64), C),
}


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("op", list(OPS))
def test_ir_records_accept_and_reject_the_same_x_in(op, cfg):
    cn = (2 if cfg else 1) * NL
    for name, (make, xin_c, want) in ACCEPT.items():
        x_in = make(cn)
        code, d = _record(op, x_in, cfg, xin_c).lower()
        assert code == OPS[op][0] and (d.xin_c, d.xin_ld, d.cfg, d.n) == (*want, int(cfg), NL), (op, name)
        assert (d.x_in or 0) == (0 if x_in is None else x_in.data_ptr()), (op, name)
    for name, (make, xin_c) in REJECT.items():
        with pytest.raises(ValueError):
            _record(op, make(cn), cfg, xin_c).lower()
            pytest.fail(f"{op} cfg={cfg}: x_in {name!r} was accepted")
