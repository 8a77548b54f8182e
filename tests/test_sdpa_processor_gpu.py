"""-m gpu: INTEGRATION.md §2 executed with the zero-copy binding — MdxSdpaProcessor (ctypes on the C-ABI only, mdx_sdpa_*) against torch's
F.scaled_dot_product_attention through the same q/k/v/out layers and against MdxAttnProcessor, the module and the limit of
tests/test_integration_gpu.py; plus the proof that nothing is copied: no zero-filled tensor, no transposed tensor."""
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

from magicdrive_amd.integration import attn_processor as AP
from magicdrive_amd.integration.attn_processor import MdxAttnProcessor, MdxSdpaProcessor
from test_integration_gpu import Attention, sdpa_processor

LIMIT = 1.5e-2          # tests/test_integration_gpu.py's own: bf16 q/k/v/p rounding inside the kernel

CASES = [(320, None, 8, 1400, None), (640, 768, 8, 350, 110), (1280, 768, 8, 91, 78), (512, None, 8, 300, None)]


def module_and_inputs(dev, C, cross, heads, T, S):
    torch.manual_seed(0)
    attn = Attention(C, cross or C, heads, C // heads).to(dev)
    x = torch.randn(6, T, C, device=dev)
    ctx = torch.randn(6, S, cross, device=dev) if cross else None
    return attn, x, ctx


@pytest.mark.parametrize("C,cross,heads,T,S", CASES)
def test_sdpa_processor_binding_matches_sdpa(dev, C, cross, heads, T, S):
    attn, x, ctx = module_and_inputs(dev, C, cross, heads, T, S)
    with torch.no_grad():
        attn.set_processor(sdpa_processor); ref = attn(x, ctx)
        attn.set_processor(MdxSdpaProcessor()); out = attn(x, ctx)
        attn.set_processor(MdxAttnProcessor()); old = attn(x, ctx)
    rel = ((out - ref).norm() / ref.norm()).item()
    rel_old = ((out - old).norm() / old.norm()).item()
    print(f"[sdpa processor C={C} T={T} S={S}] rel-L2 vs F.sdpa {rel:.3e}, vs MdxAttnProcessor {rel_old:.3e}")
    assert out.shape == ref.shape and torch.isfinite(out).all() and rel < LIMIT, rel
    assert rel_old < LIMIT, rel_old
    with pytest.raises(NotImplementedError):
        MdxSdpaProcessor()(attn, x, ctx, attention_mask=torch.ones(1, device=dev))
    with pytest.raises(RuntimeError):
        MdxSdpaProcessor()(attn.cpu(), x.cpu())


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=["fp16", "bf16"])
def test_sdpa_processor_runs_16_bit_modules_in_their_own_type(dev, dtype):
    attn, x, ctx = module_and_inputs(dev, 640, 768, 8, 350, 110)
    attn, x, ctx = attn.to(dtype), x.to(dtype), ctx.to(dtype)
    with torch.no_grad():
        attn.set_processor(sdpa_processor); ref = attn(x, ctx)
        attn.set_processor(MdxSdpaProcessor()); out = attn(x, ctx)
    rel = ((out.float() - ref.float()).norm() / ref.float().norm()).item()
    assert out.dtype == dtype and torch.isfinite(out).all() and rel < LIMIT, rel


def test_sdpa_processor_copies_nothing(dev):
    """Zero-copy: inside the processor torch.zeros is never called and no transposed tensor is made; the kernel it reaches is the row-major one,
    and it is handed the projections' own memory."""
    import ctypes
    attn, x, ctx = module_and_inputs(dev, 640, 768, 8, 350, 110)
    lib = AP._mdx()
    lib.mdx_last_kernel.restype = ctypes.c_char_p
    seen = {}
    real_v = attn.to_v.forward

    def to_v(t):
        seen["v"] = real_v(t)
        return seen["v"]

    real_transpose, real_zeros = torch.Tensor.transpose, torch.zeros
    n = {"transpose": 0, "zeros": 0}

    def transpose(self, *a, **kw):
        n["transpose"] += 1
        return real_transpose(self, *a, **kw)

    def zeros(*a, **kw):
        n["zeros"] += 1
        return real_zeros(*a, **kw)

    with torch.no_grad(), mock.patch.object(attn.to_v, "forward", to_v), mock.patch.object(torch, "zeros", zeros), \
            mock.patch.object(torch.Tensor, "transpose", transpose):
        attn.set_processor(MdxSdpaProcessor())
        out = attn(x, ctx)
        torch.cuda.synchronize()
    assert n == {"transpose": 0, "zeros": 0}, n
    assert (lib.mdx_last_kernel() or b"").decode().startswith("attn_vrow_kernel<")
    assert seen["v"].shape == (6, 110, 640)
    # the counters do count: the existing processor makes both the zero-filled and the transposed tensor
    with torch.no_grad(), mock.patch.object(torch, "zeros", zeros), mock.patch.object(torch.Tensor, "transpose", transpose):
        attn.set_processor(MdxAttnProcessor())
        old = attn(x, ctx)
    assert n["zeros"] == 1 and n["transpose"] >= 1, n
    assert ((out - old).norm() / old.norm()).item() < LIMIT
