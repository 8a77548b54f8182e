"""Algorithmic FLOP / byte accounting of an op program (2 FLOPs per MAC), per kernel family.

This is the de-duplicated work the HIP path executes (SURVEY.md §8d "F_step"): cross-view projections once
per view, context K/V and the map encoder in the prologue.  tools/count_flops.py cross-checks the totals
against the reference's as-executed FLOPs counted on the oracle.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, Iterable

from . import ops as O


def kernel_family(op) -> str:
    if isinstance(op, O.Conv):
        return "conv_direct" if op.direct else "gemm_conv_kernel<conv>"
    if isinstance(op, O.Gemm):
        return "gemm_conv_kernel<gemm>"
    if isinstance(op, O.Attn):
        return "attn_kernel"
    if isinstance(op, O.Sdpa):
        return "attn_vrow_kernel"
    if isinstance(op, O.GroupNorm):
        return "groupnorm_kernel"
    if isinstance(op, O.LayerNorm):
        return "layernorm_kernel"
    return "elementwise"


def op_flops(op) -> float:
    """Algorithmic FLOPs of one op (2 per MAC).  Attention counts QK^T + PV over every (query, key) pair: 4 * B * Tq * Tk * H * d;
    ops.Sdpa with `causal` counts half of that (the masked pairs above the diagonal are not work the algorithm asks for)."""
    if isinstance(op, O.Gemm):
        C = op.C
        batch = C.shape[0] if C.dim() == 3 else 1
        M = C.shape[-2]
        N = op.W.shape[-2]
        K = op.W.shape[-1]
        return 2.0 * batch * M * N * K
    if isinstance(op, O.Conv):
        B, Ho, Wo, Cout = op.Y.shape
        if getattr(op, "upsample2x", False):               # the algorithmic count of what it replaces: 9 taps at the output size (4 are executed)
            return 2.0 * B * Ho * Wo * Cout * 9 * op.Wt.shape[-1]
        _, kh, kw, Cin = op.Wt.shape
        return 2.0 * B * Ho * Wo * Cout * kh * kw * Cin
    if isinstance(op, O.Attn):
        B, Tq, C = op.Q.shape
        if op.kvmap is not None and not op.joint:          # summed cross-view form: a negative kv map entry is an absent source — count the pairs attended
            present = getattr(op.kvmap, "_mdx_present", None)
            if present is None:
                present = int((op.kvmap >= 0).sum())
            if present != B * op.nsrc:
                return 4.0 * present * Tq * op.Tk * C
        return 4.0 * B * Tq * op.Tk * C * op.nsrc          # QK^T + PV
    if isinstance(op, O.Sdpa):
        # convention: QK^T + PV over every (query, key) pair, 4 * B * Tq * Tk * H * d; under `causal` half of it (the pairs above the
        # diagonal are masked: T (T + 1) / 2 of T^2 pairs, counted as T^2 / 2).  A key count (klen) lives on the device and is not counted.
        B, Tq, C = op.Q.shape
        f = 4.0 * B * Tq * op.K.shape[1] * C
        return f / 2 if op.causal else f
    return 0.0


def op_bytes(op) -> float:
    """Algorithmic HBM bytes (each operand once)."""
    def nb(t):
        return 0 if t is None else t.numel() * t.element_size()
    if isinstance(op, O.Gemm):
        return nb(op.A) + nb(op.W) + nb(op.C) + nb(op.R)
    if isinstance(op, O.Conv):
        return nb(op.X) + nb(op.Wt) + nb(op.Y) + nb(op.R)
    if isinstance(op, O.Attn):
        return nb(op.Q) + op.nsrc * (nb(op.K) + op.K.shape[0] * op.K.shape[2] * op.Tk * 2) // max(op.nsrc, 1) + nb(op.O)
    if isinstance(op, O.Sdpa):
        return nb(op.Q) + nb(op.K) + nb(op.V) + nb(op.O)
    if isinstance(op, (O.GroupNorm, O.LayerNorm)):
        return nb(op.X) + nb(op.Y)
    if isinstance(op, O.LatentBlend):
        # 0 MFMA flops (op_flops), bytes only, every operand once: x read and written, cond, noise, the mask, the x_in copies
        return 2 * nb(op.x) + nb(op.cond) + nb(op.noise) + nb(op.mask) + nb(op.x_in)
    if isinstance(op, O.LatentRenoise):
        # 0 MFMA flops; x read and written, the seeds, the x_in copies (the noise is never in memory)
        return 2 * nb(op.x) + nb(op.seeds) + nb(op.x_in)
    if isinstance(op, O.DdimEtaStep):
        # 0 MFMA flops; x read and written, eps, the seeds or the caller's noise, the x_in copies (generated noise is never in memory)
        return 2 * nb(op.x) + nb(op.eps) + (nb(op.noise) if op.noise is not None else nb(op.seeds)) + nb(op.x_in)
    if isinstance(op, O.ImageComposite):
        # 0 MFMA flops; gen and orig read, out (and the matte) written, the keep cells and the has bytes
        return nb(op.gen) + nb(op.orig) + nb(op.keep) + nb(op.out) + nb(op.matte) + nb(op.has)
    if isinstance(op, (O.Ew, O.Upsample, O.Layout)):
        return nb(op.X) + nb(op.Y) * (2 if getattr(op, "kind", 0) == 1 else 1)
    return 0.0


def program_flops(ops: Iterable) -> Dict[str, float]:
    out: Dict[str, float] = defaultdict(float)
    for op in ops:
        out[kernel_family(op)] += op_flops(op)
    out["total"] = sum(v for k, v in out.items() if k != "total")
    return dict(out)
