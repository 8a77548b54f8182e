"""-m gpu: the upsampled-2x conv (MdxConvDesc.upsample2x, csrc/gemm_xl.hip with four taps per channel block) at the shapes the UNet decoder
and the VAE decoder run it at: parity against the unfused pair (nearest resize + 3x3 conv) on the GPU and against fp32 torch on the same
16-bit inputs, at the tolerance tests/test_routes_gpu.py::test_xl_conv applies to a 3x3 conv (helpers.close, xformers' table for the storage
type), in bf16 and fp16; the route through mdx_last_kernel; the host checks of what the mode cannot serve."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import close
from magicdrive_amd import _lib as L
from magicdrive_amd import ops as O
from magicdrive_amd import packing as PK


def rnd(*shape, scale=1.0, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)


def ws_buf(mb=64):
    return torch.empty(mb * 1024 * 1024 // 4, dtype=torch.float32, device="cuda")


def last_kernel():
    return (L.lib().mdx_last_kernel() or b"").decode()


# B, low-res (H, W), output (H, W), Cin, Cout
SHAPES = [
    pytest.param(48, (4, 7), (7, 13), 1280, 1280, id="unet.u0-both-axes-cropped"),
    pytest.param(24, (7, 13), (14, 25), 1280, 1280, id="unet.u1-W-cropped"),
    pytest.param(24, (14, 25), (28, 50), 640, 640, id="unet.u2"),
    pytest.param(12, (28, 50), (56, 100), 512, 512, id="vae.up0"),
    pytest.param(12, (56, 100), (112, 200), 512, 512, id="vae.up1"),
    pytest.param(12, (112, 200), (224, 400), 256, 256, id="vae.up2"),
    pytest.param(12, (54, 96), (108, 192), 512, 512, id="vae.up0-hires"),
    pytest.param(13, (6, 9), (11, 18), 128, 200, id="H-cropped-ragged-N"),
    pytest.param(40, (7, 13), (14, 25), 64, 204, id="W-cropped-narrow-stores"),           # Cout % 8 == 4: the 8-byte store branch of the row map
]


@pytest.mark.parametrize("dtype,kind", [(torch.bfloat16, "bf16"), (torch.float16, "f16")])
@pytest.mark.parametrize("B,lo,hi,Cin,Cout", SHAPES)
def test_upsample2x_conv(dev, B, lo, hi, Cin, Cout, dtype, kind):
    x = rnd(B, *lo, Cin, seed=1, dtype=dtype)
    w = rnd(Cout, Cin, 3, 3, scale=(Cin * 9) ** -0.5, seed=2)
    b = rnd(Cout, seed=3)
    wide = torch.full((B, *hi, Cout + 64), float("nan"), dtype=dtype, device=dev)          # the decoder writes a channel slice of the next concat buffer
    y = wide[..., :Cout]
    wf = PK.fold_upsample_conv(w.cpu(), hi[0] != 2 * lo[0], hi[1] != 2 * lo[1], dtype).to(dev)
    O.run_ops([O.Conv(x, wf, y, bias=b, ws=ws_buf(), upsample2x=True)])
    k = last_kernel()
    torch.cuda.synchronize()
    assert k.startswith("gemm_xl_kernel<256x") and k.endswith(",conv,up2x>"), k
    assert torch.isnan(wide[..., Cout:].float()).all() and not torch.isnan(y.float()).any()
    # the pair it replaces, on the GPU
    up = torch.empty(B, *hi, Cin, dtype=dtype, device=dev)
    y2 = torch.full((B, *hi, Cout), float("nan"), dtype=dtype, device=dev)
    O.run_ops([O.Upsample(x, up, PK.nearest_index(lo[0], hi[0]).to(dev), PK.nearest_index(lo[1], hi[1]).to(dev)),
               O.Conv(up, PK.pack_conv_weight(w.cpu(), dtype).to(dev), y2, bias=b, ws=ws_buf())])
    torch.cuda.synchronize()
    ref = F.conv2d(F.interpolate(x.float().permute(0, 3, 1, 2), size=hi, mode="nearest"), w.to(dtype).float(), b, padding=1).permute(0, 2, 3, 1)
    name = f"upsample2x {B}x{lo}->{hi} {Cin}->{Cout} {kind} {k}"
    close(y2, ref, name=name + " [unfused pair vs fp32]", kind=kind)
    close(y, ref, name=name + " [folded vs fp32]", kind=kind)
    close(y, y2.float(), name=name + " [folded vs unfused pair]", kind=kind)


@pytest.mark.parametrize("B,lo,hi,C", [(192, (7, 13), (14, 25), 1280), (192, (14, 25), (28, 50), 640), (12, (28, 50), (56, 100), 512),
                                       (12, (56, 100), (112, 200), 512), (12, (112, 200), (224, 400), 256)])
def test_upsample2x_route(dev, B, lo, hi, C):
    """u1, u2 and the VAE's three upsamplers run on the XL main loop (both tile widths serve the mode)."""
    x = rnd(B, *lo, C, seed=1, dtype=torch.bfloat16)
    wf = PK.fold_upsample_conv(rnd(C, C, 3, 3, scale=(C * 9) ** -0.5, seed=2).cpu(), hi[0] != 2 * lo[0], hi[1] != 2 * lo[1]).to(dev)
    y = torch.empty(B, *hi, C, dtype=torch.bfloat16, device=dev)
    outs = {}
    for bn in (0, 256, 320):
        with L.options(XL_BN=bn):
            O.run_ops([O.Conv(x, wf, y, bias=None, ws=ws_buf(), upsample2x=True)])
            k = last_kernel()
            torch.cuda.synchronize()
        assert k.startswith("gemm_xl_kernel<256x") and k.endswith(",conv,up2x>") and (not bn or f"<256x{bn}," in k), (bn, k)
        outs[bn] = y.clone()
    assert torch.equal(outs[256], outs[320]) and torch.equal(outs[0], outs[256])          # same reduction order in both tiles


def test_upsample2x_rejects_what_it_cannot_serve(dev):
    lib = L.lib()
    x = rnd(2, 7, 13, 64, dtype=torch.bfloat16)
    wf = PK.fold_upsample_conv(torch.randn(64, 64, 3, 3), False, True).to(dev)
    y = torch.empty(2, 14, 25, 64, dtype=torch.bfloat16, device=dev)
    _, d = O.Conv(x, wf, y, upsample2x=True).lower()
    assert lib.mdx_conv2d_bf16(L.C.byref(d), None) == 0
    with L.options(CONV_CIMAJOR=0):            # the A/B switch of the 3x3 convs' K order does not reach this mode (its K order is the kernel's own)
        assert lib.mdx_conv2d_bf16(L.C.byref(d), None) == 0
    torch.cuda.synchronize()
    bad = [("Wo", 24), ("Ho", 16), ("kh", 3), ("sh", 2), ("epilogue", L.EPI_SILU), ("splitk", 2), ("upsample2x", 2), ("R", y.data_ptr()), ("Cin", 32)]
    for field, value in bad:
        _, d = O.Conv(x, wf, y, upsample2x=True).lower()
        setattr(d, field, value)
        assert lib.mdx_conv2d_bf16(L.C.byref(d), None) != 0, field
    # a cropped axis has edge classes whose tile rows step a whole image each: X must then fit the kernel's 2 GiB window as a whole.
    # B = 64, 56x100 -> 111x199 with X a channel slice of pitch 4096 is 2.9 GB; the exact-2x size of the same X is served (no edge class)
    big = torch.empty(64 * 56 * 100 * 4096, dtype=torch.bfloat16, device=dev).view(64, 56, 100, 4096)
    big[..., :64].normal_()
    wf9 = PK.fold_upsample_conv(torch.randn(64, 64, 3, 3), True, True).to(dev)
    _, d = O.Conv(big[..., :64], wf9, torch.empty(64, 111, 199, 64, dtype=torch.bfloat16, device=dev), upsample2x=True).lower()
    assert lib.mdx_conv2d_bf16(L.C.byref(d), None) != 0 and b"2^31" in (lib.mdx_last_error() or b"")
    wf4 = PK.fold_upsample_conv(torch.randn(64, 64, 3, 3), False, False).to(dev)
    _, d = O.Conv(big[..., :64], wf4, torch.empty(64, 112, 200, 64, dtype=torch.bfloat16, device=dev), upsample2x=True).lower()
    assert lib.mdx_conv2d_bf16(L.C.byref(d), None) == 0
    torch.cuda.synchronize()
