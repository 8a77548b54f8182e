"""-m gpu: the register-resident GroupNorm (mdx_groupnorm_resident_*, gn_resident_kernel) forced with GN_RESIDENT = 2 against fp32
F.group_norm, at the limits tests/test_kernels_gpu.py::test_groupnorm holds the other GroupNorm kernels to (helpers.close).

Every (HW, C) of the site grid, bf16 and fp16; B = 2 or 3 (image indexing, the grid's padding to 8 images), SiLU on / off and eps
1e-5 / 1e-6 alternate over the grid so that every HW and every C meets both.  Input and output are channel slices of wider buffers
(ldx, ldy > C), the output buffer is NaN-filled with a guard row on either side: nothing outside the view may change.  The default op
(two streaming stages where they apply) runs on the same input and is held to the same reference.  Two runs are bit-equal."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import close  # noqa: E402
from magicdrive_amd import _lib as L  # noqa: E402
from magicdrive_amd import gn_route as GR  # noqa: E402
from magicdrive_amd import ops as O  # noqa: E402

HWS = [1, 28, 91, 350, 1399, 1400]
CS = [320, 640, 960, 1280, 1920, 2560]
G = 32
MDX_EUNSUPPORTED = -3


def tag():
    return (L.lib().mdx_last_kernel() or b"").decode()


def make_input(B, HW, C, dtype, dev):
    g = torch.Generator().manual_seed(1000 * HW + C)
    x = torch.randn(B, HW, C, generator=g) * 2 + 0.7
    if C == 960:
        x = x + 6.0                                            # |mean| >> std (the 960-channel case of test_groupnorm)
    xbig = torch.zeros(B, HW, C + 64, dtype=dtype, device=dev)
    xbig[:, :, 32:32 + C] = x.to(dtype).to(dev)
    gam = torch.randn(C, generator=g).to(dev); bet = torch.randn(C, generator=g).to(dev)
    return xbig[:, :, 32:32 + C], gam, bet


def guarded_output(B, HW, C, dtype, dev):
    """NaN-filled [1 + B * HW + 1][C + 32] buffer; the op writes columns 16 .. 16 + C of rows 1 .. B * HW."""
    ybig = torch.full((B * HW + 2, C + 32), float("nan"), dtype=dtype, device=dev)
    return ybig, ybig[1:1 + B * HW].view(B, HW, C + 32)[:, :, 16:16 + C]


def guards_intact(ybig, C):
    return bool(torch.isnan(ybig[0]).all() and torch.isnan(ybig[-1]).all() and torch.isnan(ybig[:, :16]).all() and torch.isnan(ybig[:, 16 + C:]).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("HW", HWS)
def test_resident_groupnorm(dev, HW, C, dtype):
    i, j = HWS.index(HW), CS.index(C)
    B = 2 + (i // 2 + j) % 2
    silu = (i + j) % 2 == 0
    eps = 1e-5 if (i + j // 2) % 2 == 0 else 1e-6
    x, gam, bet = make_input(B, HW, C, dtype, dev)
    assert GR.gn_resident_plan(B, HW, C, G, x.stride(1), C + 32, 16, 0) > 0
    outs = []
    with L.options(GN_RESIDENT=2):
        for _ in range(2):
            ybig, y = guarded_output(B, HW, C, dtype, dev)
            O.run_ops([O.GroupNormResident(x, y, gam, bet, groups=G, eps=eps, silu=silu)])
            assert tag() == "gn_resident_kernel"
            outs.append((ybig, y))
    # the default op on the same input (GN_ONE_KERNEL_ELEMS = 0: the streaming stages wherever they apply)
    ybig2, y2 = guarded_output(B, HW, C, dtype, dev)
    ws = torch.empty(1 << 20, dtype=torch.float32, device=dev)
    with L.options(GN_ONE_KERNEL_ELEMS=0):
        O.run_ops([O.GroupNorm(x, y2, gam, bet, groups=G, eps=eps, silu=silu, ws=ws)])
        assert (tag() == "gn_stats_kernel+gn_apply_kernel") == (HW * C >= 32768), tag()
    torch.cuda.synchronize()
    ref = F.group_norm(x.float().cpu().transpose(1, 2), G, gam.cpu(), bet.cpu(), eps)
    if silu:
        ref = F.silu(ref)
    ref = ref.transpose(1, 2)
    name = f"{B}x{HW}x{C} {'silu' if silu else 'plain'} eps={eps:g} {str(dtype)[6:]}"
    close(outs[0][1], ref, name="groupnorm resident " + name)
    close(y2, ref, name="groupnorm default " + name)
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)), "two runs differ"
    assert guards_intact(outs[0][0], C) and guards_intact(ybig2, C), "wrote outside the output view"
    assert not torch.isnan(outs[0][1].float()).any()


def test_resident_through_a_program(dev):
    """MDX_OP_GROUPNORM_RESIDENT in an op program: same bits as the direct call."""
    B, HW, C = 3, 350, 640
    x, gam, bet = make_input(B, HW, C, torch.bfloat16, dev)
    ys = []
    with L.options(GN_RESIDENT=2):
        for via_program in (False, True):
            _, y = guarded_output(B, HW, C, torch.bfloat16, dev)
            op = O.GroupNormResident(x, y, gam, bet, groups=G, eps=1e-5, silu=True)
            if via_program:
                prog = O.build_program([op])
                assert prog.buf[0].opcode == L.OP_GROUPNORM_RESIDENT == 15
                prog.run(torch.cuda.current_stream().cuda_stream)
            else:
                O.run_ops([op])
            torch.cuda.synchronize()
            ys.append(y.clone())
    assert torch.equal(ys[0], ys[1])


def _raw_call(x, y, gam, bet, dtype=L.DTYPE_BF16):
    code, d = O.GroupNormResident(x, y, gam, bet, groups=G, eps=1e-5, silu=True).lower()
    fn = getattr(L.lib(), L.entry_name(code, dtype))
    rc = fn(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, (L.lib().mdx_last_error() or b"").decode()


def test_unsupported_shapes_write_nothing(dev):
    """MDX_EUNSUPPORTED and an untouched output: rows that are not 16-byte multiples, a misaligned view, fewer than 8 channels per
    group, a slab that does not fit, a tensor under the one-launch floor (mode 1) and the switch at 0."""
    bf = torch.bfloat16
    def buffers(B, HW, C, xoff=32, xpad=64, yoff=16, ypad=32):
        xb = torch.randn(B, HW, C + xpad, device=dev).to(bf)
        yb = torch.full((B, HW, C + ypad), float("nan"), dtype=bf, device=dev)
        return xb[:, :, xoff:xoff + C], yb[:, :, yoff:yoff + C], yb
    gb = lambda C: (torch.ones(C, device=dev), torch.zeros(C, device=dev))
    cases = [
        ("ldx % 8", 2, (2, 91, 640), dict(xpad=68)),
        ("ldy % 8", 2, (2, 91, 640), dict(ypad=36)),
        ("X alignment", 2, (2, 91, 640), dict(xoff=4)),
        ("Y alignment", 2, (2, 91, 640), dict(yoff=4)),
        ("cpg 4", 2, (2, 91, 128), {}),
        ("slab", 2, (2, 4489, 320), {}),
        ("floor", 1, (2, 350, 640), {}),
        ("off", 0, (40, 350, 640), {}),
    ]
    for what, mode, (B, HW, C), kw in cases:
        x, y, yb = buffers(B, HW, C, **kw)
        with L.options(GN_RESIDENT=mode):
            rc, msg = _raw_call(x, y, *gb(C))
        assert rc == MDX_EUNSUPPORTED and "mdx_groupnorm_resident" in msg, (what, rc, msg)
        assert torch.isnan(yb).all(), what
    # the same tensors are served once the reason is gone (mode 2 lifts the floor; mode 1 takes the large tensor)
    for mode, (B, HW, C) in ((2, (2, 350, 640)), (1, (40, 350, 640))):
        x, y, yb = buffers(B, HW, C)
        with L.options(GN_RESIDENT=mode):
            rc, msg = _raw_call(x, y, *gb(C))
        assert rc == 0 and tag() == "gn_resident_kernel", (rc, msg)
        assert not torch.isnan(y.float()).any() and torch.isnan(yb[:, :, :16]).all() and torch.isnan(yb[:, :, 16 + C:]).all()


def test_default_route_is_untouched(dev):
    """mdx_groupnorm_* never takes the resident kernel, whatever GN_RESIDENT says."""
    x, gam, bet = make_input(40, 350, 640, torch.bfloat16, dev)
    ws = torch.empty(1 << 20, dtype=torch.float32, device=dev)
    for mode in (0, 1, 2):
        y = torch.zeros(40, 350, 640, dtype=torch.bfloat16, device=dev)
        with L.options(GN_RESIDENT=mode):
            O.run_ops([O.GroupNorm(x, y, gam, bet, groups=G, eps=1e-5, silu=True, ws=ws)])
            assert tag() == "gn_stats_kernel+gn_apply_kernel"
    torch.cuda.synchronize()
