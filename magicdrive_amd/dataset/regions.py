"""Keep masks for box editing: which latent pixels of a recorded view may stay while some boxes are regenerated.

`pipe.keep_masks` of StableDiffusionBEVControlNetGivenViewPipeline takes, per view, an (h, w) tensor in [0, 1] at latent resolution:
1 keeps the known latent, 0 regenerates it, a fraction mixes (ops.LatentBlend).  A latent pixel covers 8 x 8 image pixels and a box
edge falls inside it, so the mask is the COVERAGE of each latent pixel by the projected boxes, not a yes / no:

    corners, kept = project_box_corners(sample["gt_bboxes_3d"][edited], sample["lidar2image"], sample["img_aug_matrix"])
    pipe.keep_masks = [list(box_keep_mask(corners, kept, (224, 400), (28, 50)))]

Host-side input marshalling like the rest of this package (numpy / PIL / torch on the CPU, once per scene).  The projection is the one
the sample format carries (samples.box_corners, lidar2image = K @ lidar2camera of samples.precompute_cam_ext, then img_aug_matrix on
(u, v, depth) as the data pipeline that wrote the samples applies it).
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from .samples import box_corners

# the 12 edges of a box in samples.box_corners' corner order (x0y0z0, x0y0z1, x0y1z1, x0y1z0, x1y0z0, x1y0z1, x1y1z1, x1y1z0)
BOX_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))


def project_box_corners(boxes, lidar2image, img_aug_matrix, near: float = 0.1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(N, >=7) lidar boxes -> (corners_2d (n_cam, N, 20, 2) image pixels, kept (n_cam, N) bool).

    Per view and box: the 8 corners with depth > `near`, plus the points where the box's 12 edges cross the plane depth = near — the
    vertices of the box clipped to the half space in front of the camera, whose projection is convex.  Slots that are not used (a corner
    behind the plane, an edge that does not cross it) hold NaN; box_keep_mask ignores them.  kept[v, n]: some corner of box n lies in front
    of view v's near plane; a box wholly behind the camera is not kept and all its slots are NaN."""
    b = torch.as_tensor(boxes, dtype=torch.float32)
    l2i = np.asarray(lidar2image, dtype=np.float64)
    aug = np.asarray(img_aug_matrix, dtype=np.float64)
    n_cam = len(l2i)
    if b.numel() == 0:
        return torch.full((n_cam, 0, 20, 2), float("nan")), torch.zeros(n_cam, 0, dtype=torch.bool)
    c3 = box_corners(b).numpy().astype(np.float64)                                          # (N, 8, 3)
    hom = np.concatenate([c3, np.ones(c3.shape[:2] + (1,))], axis=-1)                       # (N, 8, 4)
    out = np.full((n_cam, len(c3), 20, 2), np.nan)
    kept = np.zeros((n_cam, len(c3)), dtype=bool)
    e0, e1 = np.array([e[0] for e in BOX_EDGES]), np.array([e[1] for e in BOX_EDGES])
    for v in range(n_cam):
        p = (hom @ l2i[v].T)[..., :3]                                                       # (N, 8, 3) = (u z, v z, z)
        front = p[..., 2] > near
        kept[v] = front.any(axis=1)
        pa, pb = p[:, e0], p[:, e1]                                                         # (N, 12, 3)
        za, zb = pa[..., 2], pb[..., 2]
        cross = (za > near) != (zb > near)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(cross, (near - za) / (zb - za), np.nan)
        pts = np.concatenate([np.where(front[..., None], p, np.nan), pa + t[..., None] * (pb - pa)], axis=1)       # (N, 20, 3)
        with np.errstate(divide="ignore", invalid="ignore"):
            uvz = np.stack([pts[..., 0] / pts[..., 2], pts[..., 1] / pts[..., 2], pts[..., 2]], axis=-1)
        out[v] = uvz @ aug[v][:2, :3].T + aug[v][:2, 3]
    return torch.from_numpy(out).float(), torch.from_numpy(kept)


def _convex_hull(pts: np.ndarray) -> List[Tuple[float, float]]:
    """Andrew's monotone chain: the hull of (P, 2) points, counter-clockwise, without collinear points."""
    p = sorted(set(map(tuple, pts.tolist())))
    if len(p) <= 2:
        return p

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower: List[Tuple[float, float]] = []
    for q in p:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], q) <= 0:
            lower.pop()
        lower.append(q)
    upper: List[Tuple[float, float]] = []
    for q in reversed(p):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], q) <= 0:
            upper.pop()
        upper.append(q)
    return lower[:-1] + upper[:-1]


def _clip_to_rect(poly: List[Tuple[float, float]], W: float, H: float) -> List[Tuple[float, float]]:
    """Sutherland-Hodgman: a convex polygon clipped to [0, W] x [0, H]."""
    for axis, bound, keep_below in ((0, 0.0, False), (0, W, True), (1, 0.0, False), (1, H, True)):
        if not poly:
            return poly
        inside = (lambda q: q[axis] <= bound) if keep_below else (lambda q: q[axis] >= bound)
        out: List[Tuple[float, float]] = []
        for k, cur in enumerate(poly):
            prev = poly[k - 1]
            if inside(cur) != inside(prev):
                t = (bound - prev[axis]) / (cur[axis] - prev[axis])
                x = (prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1]))
                out.append((bound, x[1]) if axis == 0 else (x[0], bound))
            if inside(cur):
                out.append(cur)
        poly = out
    return poly


def _snap_to_pixels(poly: List[Tuple[float, float]]) -> List[Tuple[int, int]]:
    """A polygon in continuous image coordinates -> integer PIL vertices.  PIL's polygon takes whole pixel indices and fills its outline
    inclusively, so each vertex is snapped to the outermost pixel whose CENTRE (index + 0.5) it still encloses, seen from the polygon's
    centroid: ceil(x - 0.5) on the low side, floor(x - 0.5) on the high side, per axis.  An axis-aligned edge then includes exactly the
    pixels whose centres lie inside it; a slanted edge is off by less than one image pixel.  [] when no pixel centre can lie inside."""
    xs, ys = [q[0] for q in poly], [q[1] for q in poly]
    if np.ceil(min(xs) - 0.5) > np.floor(max(xs) - 0.5) or np.ceil(min(ys) - 0.5) > np.floor(max(ys) - 0.5):
        return []
    cx, cy = sum(xs) / len(xs), sum(ys) / len(ys)
    snap = lambda u, c: int(np.ceil(u - 0.5)) if u < c else int(np.floor(u - 0.5))
    return [(snap(x, cx), snap(y, cy)) for x, y in poly]


def box_keep_mask(corners_2d, kept, image_hw, latent_hw, dilate: int = 1) -> torch.Tensor:
    """Keep mask (n_cam, h, w) fp32 in [0, 1] for regenerating the given boxes: 1 - coverage of each latent pixel.

    corners_2d (n_cam, N, P, 2): projected points of every box in image pixels (x right, y down; pixel (px, py) is the square
      [px, px + 1) x [py, py + 1)), e.g. project_box_corners' output; non-finite points are ignored.
    kept (n_cam, N) bool: the boxes that count in each view; a box behind the camera is not kept and is dropped.
    image_hw / latent_hw: (H, W) of the pictures the corners refer to and (h, w) of the latents; H / h and W / w must be integers (the
      VAE factor, 8).
    The region of a view is the UNION of the convex hulls of its kept boxes, each clipped to the image.  It is rasterised at image
    resolution with PIL (an image pixel counts when its centre lies inside a hull: exact for axis-aligned edges, within one image pixel
    for slanted ones, see _snap_to_pixels), mean-pooled over the H / h x W / w image pixels of
    every latent pixel — the coverage fraction — and max-dilated by `dilate` latent pixels (the network's receptive field smears a box
    into its neighbourhood; dilate = 0: the bare coverage).  Returns 1 - that: 1 keeps, 0 regenerates."""
    from PIL import Image, ImageDraw
    pts = np.asarray(torch.as_tensor(corners_2d, dtype=torch.float32).numpy(), dtype=np.float64)
    kp = np.asarray(torch.as_tensor(kept).numpy(), dtype=bool)
    assert pts.ndim == 4 and pts.shape[-1] == 2 and kp.shape == pts.shape[:2], f"corners_2d {pts.shape} / kept {kp.shape}"
    (H, W), (h, w) = image_hw, latent_hw
    assert h > 0 and w > 0 and H % h == 0 and W % w == 0, f"image {image_hw} is not a whole multiple of the latent {latent_hw}"
    assert int(dilate) == dilate and dilate >= 0, f"dilate={dilate!r}: an integer >= 0"
    fy, fx = H // h, W // w
    cover = torch.zeros(len(pts), h, w, dtype=torch.float32)
    for v in range(len(pts)):
        img = Image.new("L", (W, H), 0)
        draw = ImageDraw.Draw(img)
        any_box = False
        for n in np.nonzero(kp[v])[0]:
            q = pts[v, n]
            q = q[np.isfinite(q).all(axis=1)]
            hull = _clip_to_rect(_convex_hull(q), float(W), float(H)) if len(q) >= 3 else []
            snapped = _snap_to_pixels(hull) if len(hull) >= 3 else []
            if snapped:
                draw.polygon(snapped, fill=1)
                any_box = True
        if any_box:
            a = torch.from_numpy(np.asarray(img, dtype=np.float32))
            cover[v] = a.reshape(h, fy, w, fx).mean(dim=(1, 3))
    if dilate > 0:
        cover = torch.nn.functional.max_pool2d(cover.unsqueeze(1), 2 * int(dilate) + 1, stride=1, padding=int(dilate)).squeeze(1)
    return (1.0 - cover).clamp_(0.0, 1.0)


def edit_matte(keep, factor: int, feather: int) -> torch.Tensor:
    """The matte of a kept-region composite, (..., h, w) keep masks in [0, 1] -> (..., h * factor, w * factor) fp32 weights of the
    RECORDED picture: the definition the library's op computes on the device (ops.ImageComposite, include/mdx.h: MdxCompositeDesc), in
    plain torch on the tensor's own device.  The product path never calls this: it is the documented meaning of the op and what
    CPU-only callers use.

        a = keep repeated `factor` times along both axes (nearest upsample);
        e = min of a over the (2 feather + 1)^2 window, the image padded by edge replication (erosion);
        w = mean of e over the same window, padded likewise.

    feather is in IMAGE pixels, 0 to 16; 0 returns a.  w = 0 wherever a = 0 (generated content is never attenuated inside the
    regenerated region), w = 1 wherever every a within Chebyshev distance 2 feather is 1, and the transition band of width 2 feather lies
    inside the kept region, where both sources show the same picture up to the VAE's error.  Next to the image border w = 0 may reach a
    few pixels past a = 0: the clamped window is cut by the border."""
    import torch.nn.functional as F
    k = torch.as_tensor(keep)
    if not k.dtype.is_floating_point:
        k = k.float()
    if k.dim() < 2:
        raise ValueError(f"edit_matte: keep must be (..., h, w), got {tuple(k.shape)}")
    if not (isinstance(factor, int) and not isinstance(factor, bool) and factor >= 1):
        raise ValueError(f"edit_matte: factor={factor!r} must be an integer >= 1")
    if not (isinstance(feather, int) and not isinstance(feather, bool) and 0 <= feather <= 16):
        raise ValueError(f"edit_matte: feather={feather!r} must be an integer in [0, 16]")
    a = k.repeat_interleave(factor, dim=-2).repeat_interleave(factor, dim=-1)
    if feather == 0:
        return a.float() if a.dtype != torch.float64 else a
    r, n = feather, 2 * feather + 1
    x = a.reshape(-1, 1, *a.shape[-2:])

    def pad(t):                     # edge replication of any width (F.pad's replicate mode needs the pad to be smaller than the image)
        iy = torch.arange(-r, t.shape[-2] + r, device=t.device).clamp_(0, t.shape[-2] - 1)
        ix = torch.arange(-r, t.shape[-1] + r, device=t.device).clamp_(0, t.shape[-1] - 1)
        return t[..., iy, :][..., ix]

    e = -F.max_pool2d(-pad(x), n, stride=1)
    w = F.avg_pool2d(pad(e), n, stride=1)
    return w.reshape(a.shape)
