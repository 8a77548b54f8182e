"""Host-side weight / index packing for the libmdx kernels (runs once at load time).

Reference state-dict tensors (diffusers / MagicDrive layout) -> the layouts the kernels read:
  * conv filters  [Cout, Cin, kh, kw]  -> [Cout, kh, kw, Cin] bf16  (K-contiguous for the implicit GEMM)
  * GEGLU proj    [2F, K] (value rows | gate rows, attention.py:259-280) -> 32-row interleave so one
    MFMA wave tile holds a feature's value and gate in the same register slot
  * nearest-neighbour source indices for Upsample2D (resnet.py:154-163), torch's float32 rule
  * Upsample2D's 3x3 conv folded over its 2x nearest resize: 2x2 phase filters on the low-res input (MdxConvDesc.upsample2x)
"""
from __future__ import annotations

import numpy as np
import torch


def pack_conv_weight(w: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    assert w.dim() == 4
    return w.detach().permute(0, 2, 3, 1).contiguous().to(dtype)


def pack_linear_weight(w: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    assert w.dim() == 2
    return w.detach().contiguous().to(dtype)


def pack_geglu(w: torch.Tensor, b: torch.Tensor, dtype=torch.bfloat16):
    """[2F, K] with rows [value(F) | gate(F)] -> rows [v0..31, g0..31, v32..63, g32..63, ...]."""
    two_f, k = w.shape
    f = two_f // 2
    assert two_f == 2 * f and f % 32 == 0, f"GEGLU inner dim {f} must be a multiple of 32"
    wv = w[:f].reshape(f // 32, 32, k)
    wg = w[f:].reshape(f // 32, 32, k)
    wp = torch.stack([wv, wg], dim=1).reshape(two_f, k)
    bv = b[:f].reshape(f // 32, 32)
    bg = b[f:].reshape(f // 32, 32)
    bp = torch.stack([bv, bg], dim=1).reshape(two_f)
    return wp.contiguous().to(dtype), bp.contiguous().to(torch.float32)


def pack_wq(w: torch.Tensor) -> torch.Tensor:
    """Row-major linear weight [N, K] (16-bit, K % 32 == 0) -> MFMA-fragment order for the W-direct GEMM (include/mdx.h: MdxGemmDesc.Wq,
    csrc/gemm_xd.hip):  Wq[n // 16][k // 32][((k % 32) // 8) * 16 + n % 16][k % 8], N padded with zero rows to a multiple of 256.
    A pure permutation: one contiguous KiB per 16-column x 32-deep block."""
    n, k = w.shape
    assert k % 32 == 0, f"pack_wq: K={k} must be a multiple of 32"
    npad = round_up(n, 256)
    wp = w if npad == n else torch.cat([w, torch.zeros(npad - n, k, dtype=w.dtype, device=w.device)], 0)
    return wp.reshape(npad // 16, 16, k // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(npad, k)


def nearest_index(n_in: int, n_out: int) -> torch.Tensor:
    """Source index of F.interpolate(mode='nearest', size=n_out): min(floor(dst * (in/out)), in-1) in fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    src = np.minimum(np.floor(dst * scale).astype(np.int64), n_in - 1)
    return torch.from_numpy(src.astype(np.int32))


# ---- Upsample2D fold: conv3x3(pad 1) o nearest-2x  ==  four 2x2 phase convs of the low-res input (include/mdx.h: MdxConvDesc.upsample2x) ----
# In the resized image pixel o reads source o >> 1, so along one axis the taps (o - 1, o, o + 1) of an output index read two sources:
#   class 0  even o = 2 j       sources (j - 1, j)   weights (w0, w1 + w2)
#   class 1  odd  o = 2 j + 1   sources (j, j + 1)   weights (w0 + w1, w2)
#   class 2  the last even index when n_out = 2 n_in - 1: its +1 tap is the conv's zero padding, not source j -> (w0, w1)
# An exact-2x axis has classes 0, 1; a cropped one 0, 1, 2 (0 and 1 then stop one source index earlier).

def upsample_fold_ok(n_in: int, n_out: int) -> bool:
    """The fold is valid where the nearest map is o >> 1 and the size is 2 n or 2 n - 1."""
    return n_in >= 1 and n_out in (2 * n_in, 2 * n_in - 1) and bool(torch.equal(nearest_index(n_in, n_out), torch.arange(n_out, dtype=torch.int32) >> 1))


def upsample_axis_classes(n_in: int, n_out: int):
    """[(count, first source index, pad, parity)] per class of one axis: class c covers sources first .. first + count - 1 and writes
    output index 2 j + parity; its two taps read sources j - pad, j - pad + 1."""
    crop = int(n_out != 2 * n_in)
    cls = [(n_in - crop, 0, 1, 0), (n_in - crop, 0, 0, 1)]
    if crop:
        cls.append((1, n_in - 1, 1, 0))
    return cls


def _fold_axis(w: torch.Tensor, dim: int, c: int) -> torch.Tensor:
    w0, w1, w2 = w.unbind(dim)
    pair = (w0, w1 + w2) if c == 0 else (w0 + w1, w2) if c == 1 else (w0, w1)
    return torch.stack(pair, dim)


def fold_upsample_conv(w: torch.Tensor, crop_h: bool, crop_w: bool, dtype=torch.bfloat16) -> torch.Tensor:
    """3x3 filter [Cout, Cin, 3, 3] -> phase filters [ny * nx, Cout, 2, 2, Cin] (set yc * nx + xc), summed in the precision of `w`
    (fp32 at pack time) and rounded ONCE to `dtype` (None: not rounded)."""
    assert w.dim() == 4 and w.shape[2:] == (3, 3)
    ny, nx = 2 + int(crop_h), 2 + int(crop_w)
    sets = [_fold_axis(_fold_axis(w.detach(), 2, yc), 3, xc).permute(0, 2, 3, 1) for yc in range(ny) for xc in range(nx)]
    out = torch.stack(sets, 0).contiguous()
    return out if dtype is None else out.to(dtype)


def folded_upsample_conv_reference(x: torch.Tensor, wf: torch.Tensor, Ho: int, Wo: int, bias=None) -> torch.Tensor:
    """What the upsampled-2x conv computes, in torch: x [B, Cin, Hi, Wi], wf from fold_upsample_conv -> [B, Cout, Ho, Wo] (x's dtype)."""
    import torch.nn.functional as F
    B, _, Hi, Wi = x.shape
    ycls, xcls = upsample_axis_classes(Hi, Ho), upsample_axis_classes(Wi, Wo)
    assert wf.shape[0] == len(ycls) * len(xcls)
    y = x.new_zeros(B, wf.shape[1], Ho, Wo)
    for yc, (hn, h0, hp, hpar) in enumerate(ycls):
        for xc, (wn, w0, wp, wpar) in enumerate(xcls):
            if hn == 0 or wn == 0:
                continue
            w = wf[yc * len(xcls) + xc].to(x.dtype).permute(0, 3, 1, 2)                      # [Cout, Cin, 2, 2]
            xp = F.pad(x, (1, 1, 1, 1))                                                     # source s sits at s + 1
            win = xp[:, :, h0 - hp + 1:h0 - hp + 1 + hn + 1, w0 - wp + 1:w0 - wp + 1 + wn + 1]
            y[:, :, 2 * h0 + hpar:2 * (h0 + hn - 1) + hpar + 1:2, 2 * w0 + wpar:2 * (w0 + wn - 1) + wpar + 1:2] = F.conv2d(win, w)
    return y if bias is None else y + bias.to(x.dtype)[None, :, None, None]


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m
