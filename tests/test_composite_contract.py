"""CPU: the host-side contract of mdx_image_composite_* (include/mdx.h: MdxCompositeDesc), table-driven like tests/test_latent_blend_contract.py.

One valid descriptor and, per sentence of the header contract, mutations that violate only that sentence: each must come back MDX_EINVAL
with a message naming the field — through the bf16 symbol, the _f16 symbol and a one-op mdx_program_run.  Pointers are plain integers
with the wanted alignment: a missing check shows up as a launch attempt (MDX_ELAUNCH on a machine without a device), never as a memory
access; for that reason the tables refuse to run where a device is visible, and the valid descriptor is only ever called with V == 0,
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
OP = L.OP_IMAGE_COMPOSITE
H, W = 224, 400


def comp(**kw):
    """The op of one scene's decode: 6 views of 3 x 224 x 400, 16-bit planar gen, masks at 28 x 50, a matte, every view with a picture."""
    d = dict(gen=P(1), orig=P(2), keep=P(3), out=P(4), matte=P(5), has=P(6), V=6, C=3, H=H, W=W, f=8, feather=4, gen_f32=0,
             g_sv=3 * H * W, g_sc=H * W, g_ld=W)
    d.update(kw); return d


# (sentence of include/mdx.h, descriptor, what mdx_last_error() must name)
TABLE = [
    ("gen, orig, keep, out not NULL", comp(gen=0), "gen must not be NULL"),
    ("gen, orig, keep, out not NULL", comp(orig=0), "orig must not be NULL"),
    ("gen, orig, keep, out not NULL", comp(keep=0), "keep must not be NULL"),
    ("gen, orig, keep, out not NULL", comp(out=0), "out must not be NULL"),
    ("gen at its element's alignment (2 / 4 bytes)", comp(gen=P(1) + 1), "gen must be 2-byte"),
    ("gen at its element's alignment (2 / 4 bytes)", comp(gen=P(1) + 2, gen_f32=1), "gen must be 4-byte"),
    ("orig, keep, out, matte 4-byte aligned", comp(orig=P(2) + 2), "orig must be 4-byte"),
    ("orig, keep, out, matte 4-byte aligned", comp(keep=P(3) + 1), "keep must be 4-byte"),
    ("orig, keep, out, matte 4-byte aligned", comp(out=P(4) + 2), "out must be 4-byte"),
    ("orig, keep, out, matte 4-byte aligned", comp(matte=P(5) + 3), "matte must be 4-byte"),
    ("V not negative", comp(V=-1), "V=-1"),
    ("C in [1, 4]", comp(C=0), "C=0"),
    ("C in [1, 4]", comp(C=5), "C=5"),
    ("H, W >= 1", comp(H=0), "H=0"),
    ("H, W >= 1", comp(W=0, g_ld=0), "W=0"),
    ("H, W >= 1", comp(H=-8), "H=-8"),
    ("f >= 1 and divides H and W", comp(f=0), "f=0"),
    ("f >= 1 and divides H and W", comp(f=-8), "f=-8"),
    ("f >= 1 and divides H and W", comp(f=32), "f=32"),         # divides 224, not 400
    ("f >= 1 and divides H and W", comp(f=25), "f=25"),         # divides 400, not 224
    ("feather in [0, 16]", comp(feather=-1), "feather=-1"),
    ("feather in [0, 16]", comp(feather=17), "feather=17"),
    ("gen_f32 in {0, 1}", comp(gen_f32=2), "gen_f32=2"),
    ("gen_f32 in {0, 1}", comp(gen_f32=-1), "gen_f32=-1"),
    ("g_ld >= W", comp(g_ld=W - 1), "g_ld=399"),
    ("g_sc, g_sv not negative", comp(g_sc=-1), "g_sc=-1"),
    ("g_sc, g_sv not negative", comp(g_sv=-1), "g_sv=-1"),
    ("feather and H * W fit a 32-bit int", comp(V=BIG), "V="),
    ("feather and H * W fit a 32-bit int", comp(C=BIG), "C="),
    ("feather and H * W fit a 32-bit int", comp(H=BIG), "H="),
    ("feather and H * W fit a 32-bit int", comp(W=BIG, g_ld=BIG), "W="),
    ("feather and H * W fit a 32-bit int", comp(f=BIG), "f="),
    ("feather and H * W fit a 32-bit int", comp(feather=BIG), "feather="),
    ("feather and H * W fit a 32-bit int", comp(H=1 << 16, W=1 << 16, g_ld=1 << 16, f=1), "H=65536 times W=65536"),
]


def _desc(fields):
    d = L.MdxCompositeDesc()
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
        assert "mdx_image_composite_f16" in msg, msg


@no_device
@pytest.mark.parametrize("path", ["bf16", "f16", "program"])
@pytest.mark.parametrize("fields", [comp(V=0), comp(V=0, matte=0, has=0), comp(V=0, gen_f32=1, feather=16, f=1), comp(V=0, C=4, feather=0, g_ld=W + 8, g_sc=0, g_sv=0),
                                    comp(V=0, has=P(6) + 1)],
                         ids=["v0", "v0-no-matte-no-has", "v0-fp32-gen", "v0-strides", "v0-odd-has"])
def test_empty_problem_launches_nothing(fields, path):
    """V == 0 returns MDX_OK before any launch: on a machine without a device a launch attempt would come back MDX_ELAUNCH."""
    rc, msg = _call(path, _desc(fields))
    assert rc == OK, f"rc={rc}: {msg!r}"


@no_device
def test_an_empty_problem_is_still_checked():
    rc, msg = _call("bf16", _desc(comp(V=0, out=P(4) + 2)))
    assert rc == EINVAL and "out must be 4-byte" in msg
    rc, msg = _call("bf16", _desc(comp(V=0, feather=17)))
    assert rc == EINVAL and "feather=17" in msg


def test_every_host_check_has_a_row():
    """Every field a check of the entry point names is named by a row, and every sentence the table quotes stands in the header."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    body = open(os.path.join(root, "magicdrive_amd", "csrc", "composite.hip")).read().split('extern "C" int mdx_image_composite_bf16(')[1].split("if (d->V == 0) return MDX_OK;")[0]
    fields = set(re.findall(r'need_\w+\(op, "([A-Za-z_0-9]+)"', body)) | set(re.findall(r'"%s: (\w+)=%ld', body)) | set(re.findall(r'"%s: (\w+) must not be NULL"', body))
    assert fields == {"gen", "orig", "keep", "out", "matte", "V", "C", "H", "W", "f", "feather", "gen_f32", "g_ld", "g_sc", "g_sv"}, fields
    names = [n for _, _, n in TABLE]
    covered = {f for f in fields if any(n.startswith(f + "=") or n.startswith(f + " must") for n in names)}
    assert fields == covered, sorted(fields - covered)
    flat = re.sub(r"[\s*]+", " ", open(os.path.join(root, "include", "mdx.h")).read())
    for clause in {c for c, _, _ in TABLE}:
        assert re.sub(r"[\s*]+", " ", clause) in flat, clause


def test_binding_matches_the_header(tmp_path):
    """sizeof / offsetof of MdxCompositeDesc in the C header equal the ctypes mirror's; the opcode and both symbols are declared and exported;
    the ABI version is still 12 and the op is not a row of DESC_OF_OP."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mdx.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(MdxCompositeDesc), '
                 'offsetof(MdxCompositeDesc, has), offsetof(MdxCompositeDesc, V), offsetof(MdxCompositeDesc, gen_f32), offsetof(MdxCompositeDesc, g_sv), '
                 'offsetof(MdxCompositeDesc, g_ld), MDX_OP_IMAGE_COMPOSITE);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(c), "-o", str(exe)], check=True)
    size, o_has, o_v, o_f32, o_sv, o_ld, code = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    S = L.MdxCompositeDesc
    assert (size, o_has, o_v, o_f32, o_sv, o_ld) == (ctypes.sizeof(S), S.has.offset, S.V.offset, S.gen_f32.offset, S.g_sv.offset, S.g_ld.offset) and size == 16 * 8
    assert [f[0] for f in S._fields_] == "gen orig keep out matte has V C H W f feather gen_f32 g_sv g_sc g_ld".split()
    assert size <= L.OP_BYTES - 16
    assert code == L.OP_IMAGE_COMPOSITE == 20 and L.ENTRY_OF_OP[L.OP_IMAGE_COMPOSITE] == "mdx_image_composite_bf16"
    assert {"mdx_image_composite_bf16", "mdx_image_composite_f16"} <= set(L.EXPORTS)
    assert L.OP_IMAGE_COMPOSITE not in L.DESC_OF_OP
    assert L.lib().mdx_abi_version() == 12 and L.ABI_VERSION == 12


def test_op_record_checks_and_flops():
    """ops.ImageComposite.lower() on CPU views: shapes, strides and the factor reach the descriptor, the build follows gen's 16-bit type,
    bad records raise; flops.op_flops is 0 and op_bytes counts every operand once."""
    from magicdrive_amd import flops as FL
    from magicdrive_amd import ops as O
    V, C, Hh, Ww, f = 2, 3, 16, 24, 8
    orig, out = torch.zeros(V, Hh, Ww, C), torch.zeros(V, Hh, Ww, C)
    keep, matte, has = torch.zeros(V, Hh // f, Ww // f), torch.zeros(V, Hh, Ww), torch.ones(V, dtype=torch.uint8)
    for dt, code, f32 in ((torch.float16, L.DTYPE_F16, 0), (torch.bfloat16, L.DTYPE_BF16, 0), (torch.float32, L.DTYPE_BF16, 1)):
        gen = torch.zeros(V, C, Hh, Ww, dtype=dt)
        op = O.ImageComposite(gen, orig, keep, out, 3, matte=matte, has=has)
        opcode, d = op.lower()
        assert opcode == L.OP_IMAGE_COMPOSITE and (d.V, d.C, d.H, d.W, d.f, d.feather, d.gen_f32) == (V, C, Hh, Ww, f, 3, f32)
        assert (d.g_sv, d.g_sc, d.g_ld) == (C * Hh * Ww, Hh * Ww, Ww) and d.matte and d.has
        assert O.dtype_code(op) == code and FL.op_flops(op) == 0.0 and FL.kernel_family(op) == "elementwise"
        assert FL.op_bytes(op) == gen.numel() * gen.element_size() + 4 * (2 * orig.numel() + keep.numel() + matte.numel()) + V
    wide = torch.zeros(V, C + 2, Hh, Ww + 8, dtype=torch.float16)[:, 1:C + 1, :, :Ww]      # a channel slice of a wider tensor with a longer row pitch
    d = O.ImageComposite(wide, orig, keep, out, 0).lower()[1]
    assert (d.g_sv, d.g_sc, d.g_ld, d.matte, d.has) == ((C + 2) * Hh * (Ww + 8), Hh * (Ww + 8), Ww + 8, None, None)
    assert d.gen == wide.data_ptr()
    gen = torch.zeros(V, C, Hh, Ww, dtype=torch.float16)
    for bad in (dict(gen=gen.permute(0, 1, 3, 2)), dict(gen=gen.double()), dict(gen=gen[:, :, :, ::2]), dict(orig=orig.half()), dict(orig=orig[:, :, :, :2]),
                dict(out=out.permute(0, 3, 1, 2)), dict(keep=torch.zeros(V, 2, 4)), dict(keep=torch.zeros(V, 4, 3)), dict(keep=keep.double()),
                dict(feather=17), dict(feather=-1), dict(feather=2.0), dict(matte=torch.zeros(V, Hh, Ww + 1)), dict(has=torch.ones(V)),
                dict(has=torch.ones(V + 1, dtype=torch.uint8)), dict(gen=torch.zeros(V, 5, Hh, Ww, dtype=torch.float16))):
        kw = dict(gen=gen, orig=orig, keep=keep, out=out, feather=3, matte=matte, has=has)
        kw.update(bad)
        with pytest.raises(ValueError):
            O.ImageComposite(**kw).lower()


def test_functional_form_has_no_cpu_path():
    from magicdrive_amd import ops as O
    with pytest.raises(RuntimeError, match="MI355X only"):
        O.image_composite(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8, 3), torch.zeros(1, 1, 1), 0)
