"""TEST INFRASTRUCTURE shared by tests/test_composite_cpu.py and tests/test_composite_gpu.py: the case grid, the keep masks and the
float64 restatement of the kept-region composite (include/mdx.h: MdxCompositeDesc; magicdrive_amd.dataset.edit_matte).

A case is (V, H, W, f) with its feathers and ONE rectangle of keep cells: the mask is ones everywhere, zeros inside the rectangle and a
one-cell rim of random multiples of 1/64 (strictly between 0 and 1) around it, drawn per view.  The shapes are the smallest that cross a
32 x 64 tile edge with a ragged remainder and a halo as wide as a tile."""
import torch

# (V, H, W, f), feathers, rectangle of zero cells (y0, y1, x0, x1)
CASES = [
    ((3, 16, 24, 8), (0, 1, 3), (0, 1, 0, 1)),
    ((2, 40, 72, 8), (0, 1, 3, 8), (1, 3, 2, 5)),
    ((2, 96, 128, 8), (8, 16), (0, 4, 0, 5)),
    ((2, 36, 20, 4), (0, 2, 5), (6, 9, 0, 2)),
]
GRID = [(ci, r) for ci, (_, feathers, _) in enumerate(CASES) for r in feathers]
GRID_IDS = ["%dx%dx%df%d-r%d" % (*CASES[ci][0], r) for ci, r in GRID]


def keep_mask(ci: int) -> torch.Tensor:
    """fp32 [V, H / f, W / f] on the 1/64 grid, on the CPU; the same tensor for every caller (seeded by the case index)."""
    (V, H, W, f), _, (y0, y1, x0, x1) = CASES[ci]
    h, w = H // f, W // f
    g = torch.Generator().manual_seed(1000 + ci)
    m = torch.ones(V, h, w)
    rim = torch.randint(1, 64, (V, h, w), generator=g).float() / 64.0
    ry0, ry1, rx0, rx1 = max(y0 - 1, 0), min(y1 + 1, h), max(x0 - 1, 0), min(x1 + 1, w)
    m[:, ry0:ry1, rx0:rx1] = rim[:, ry0:ry1, rx0:rx1]
    m[:, y0:y1, x0:x1] = 0.0
    return m


def matte64(keep: torch.Tensor, f: int, r: int) -> torch.Tensor:
    """The definition, written out in float64 with explicit clamped indices (no pooling call): a = nearest upsample, e = min of a over
    the (2r+1)^2 window, w = (sum of e over the window) / (2r+1)^2, every coordinate clamped to the image."""
    a = keep.double().repeat_interleave(f, dim=-2).repeat_interleave(f, dim=-1)
    H, W = a.shape[-2:]
    iy, ix = torch.arange(H), torch.arange(W)
    e = a
    if r > 0:
        rows = torch.stack([a[..., (iy + d).clamp(0, H - 1), :] for d in range(-r, r + 1)]).amin(dim=0)
        e = torch.stack([rows[..., (ix + d).clamp(0, W - 1)] for d in range(-r, r + 1)]).amin(dim=0)
    s = sum(e[..., (iy + d).clamp(0, H - 1), :] for d in range(-r, r + 1))
    s = sum(s[..., (ix + d).clamp(0, W - 1)] for d in range(-r, r + 1))
    return s / float((2 * r + 1) ** 2)


def all_ones_within(keep: torch.Tensor, f: int, dist: int) -> torch.Tensor:
    """bool [.., H, W]: every a within Chebyshev distance `dist` (clamped to the image) equals 1."""
    a = keep.double().repeat_interleave(f, dim=-2).repeat_interleave(f, dim=-1)
    H, W = a.shape[-2:]
    iy, ix = torch.arange(H), torch.arange(W)
    rows = torch.stack([a[..., (iy + d).clamp(0, H - 1), :] for d in range(-dist, dist + 1)]).amin(dim=0)
    return torch.stack([rows[..., (ix + d).clamp(0, W - 1)] for d in range(-dist, dist + 1)]).amin(dim=0) == 1.0


def regime_shares(w: torch.Tensor):
    """(share of w == 0, of w == 1, of 0 < w < 1) of a reference matte."""
    n = float(w.numel())
    z, o = float((w == 0).sum()) / n, float((w == 1).sum()) / n
    return z, o, 1.0 - z - o
