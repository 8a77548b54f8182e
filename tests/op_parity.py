"""TEST INFRASTRUCTURE: per-op parity of a lowered plan.  Nothing in magicdrive_amd imports this.

reference(op) restates every op of magicdrive_amd/ops.py in plain fp64 torch, from include/mdx.h, on whatever device the op's tensors
live on (it never calls libmdx, and it shares no code with tests/plan_interp.py: the CPU self-test walks the interpreter with it).

walk(ops, execute) runs a program op by op.  Before an op it snapshots every tensor the op reads and the whole storage behind every tensor it
writes; after `execute(op)` it computes the fp64 reference FROM THE SNAPSHOT and holds the op alone to the kernel-level criterion:

  values    16-bit outputs: helpers.close() against fp64, unchanged.  fp32 outputs: the bounds the kernel tests apply to the same kernels
            (tails_data.F32_REL_L2 for GEMM / conv, ABS_BOUND for TimeEmb and the scheduler ops, ops.GroupStats.chain_length for the records;
            LatentBlend, LatentRenoise, DdimEtaStep and ImageComposite: the per-element bounds of tests/test_latent_blend_gpu.py,
            test_latent_renoise_gpu.py, test_ddim_eta_gpu.py and test_composite_gpu.py, stated next to their references, with the device
            noise of tests/philox_ref.py; a latent op's 16-bit x_in is also the rounding of the stored x, bit for bit).
  finite    every output element, except where include/mdx.h says NaN (a key count outside [1, Tk]).
  borders   every byte of an output's storage outside the output view keeps its bits (the other half of a concat buffer, the q / k block next
            to a fused V^T, the V^T pad columns past vt_T, the pad channels of x_in).  Scratch (ws, ln_scratch) is exempt; the columns
            N .. roundup4(N) of a GEMM output may be zero-filled (slack_views).
  inputs    every operand that is not an output is bit-identical afterwards.
  no skip   an op class or a tensor field without a reference raises; the number of judged ops is the number asked for.

The inputs of an op are what the executor produced for the ops before it, so errors do not accumulate and a failure names one op.
"""
import contextlib
import dataclasses
import math

import numpy as np
import torch

import helpers
import philox_ref as PH
import tails_data as T
import values_data as V
from magicdrive_amd import _lib as L
from magicdrive_amd import ops as O

F64 = torch.float64
H16 = (torch.bfloat16, torch.float16)
U24 = 2.0 ** -24


class OpParityError(AssertionError):
    """One op missed one condition."""

    def __init__(self, index, op, kernel, condition, detail):
        self.index, self.op_name, self.kernel, self.condition, self.detail = index, getattr(op, "name", ""), kernel, condition, detail
        super().__init__(f"op[{index}] {type(op).__name__} '{self.op_name}' kernel '{kernel}': {condition}: {detail}")


# ---- which field is what ---------------------------------------------------------------------------------------------------------------
# inputs: read only.  outputs: written (inout: also read).  scratch: may hold anything afterwards.  Every tensor field of an op must be listed.
@dataclasses.dataclass(frozen=True)
class Fields:
    inputs: tuple
    outputs: tuple
    scratch: tuple = ()


_GN = Fields(("X", "gamma", "beta"), ("Y",), ("ws",))
_SCHED = ("eps", "coef", "gv_mask", "gv_cond", "gv_noise")
FIELDS = {
    O.Gemm: Fields(("A", "W", "bias", "R", "temb", "sel", "ln_csum", "ln_stats", "Wq"), ("C", "Vt", "rowstat"), ("ws", "ln_scratch")),
    O.Conv: Fields(("X", "Wt", "bias", "R", "temb", "sel"), ("Y",), ("ws",)),
    O.Attn: Fields(("Q", "K", "Vt", "kvmap", "tk_dev", "tk_rows"), ("O",)),
    O.GroupNorm: _GN,
    O.GroupNormResident: _GN,
    O.LayerNorm: Fields(("X", "gamma", "beta"), ("Y",)),
    O.Softmax: Fields(("X",), ("Y",)),
    O.Ew: Fields(("X",), ("Y",)),
    O.Upsample: Fields(("X", "ymap", "xmap"), ("Y",)),
    O.Layout: Fields(("X",), ("Y",)),
    O.Fourier: Fields(("X", "mask", "null_feat"), ("Y",)),
    O.Gather: Fields(("T", "idx", "mask", "null_row", "add"), ("Y",)),
    O.TimeEmb: Fields(("t",), ("Y",)),
    O.DdimStep: Fields(_SCHED, ("x", "x_in", "step")),
    O.UniPCStep: Fields(_SCHED, ("x", "x_in", "step", "x_last", "m1", "m2")),
    O.GroupStats: Fields(("X", "row"), ("out",)),
    O.Sdpa: Fields(("Q", "K", "V", "klen"), ("O",)),
    O.LatentBlend: Fields(("cond", "noise", "mask", "coef", "step"), ("x", "x_in")),
    O.LatentRenoise: Fields(("coef", "seeds"), ("x", "x_in", "step", "visit")),
    O.DdimEtaStep: Fields(_SCHED + ("var", "seeds", "noise"), ("x", "x_in", "step", "draw")),
    O.ImageComposite: Fields(("gen", "orig", "keep", "has"), ("out", "matte")),
}
LATENT_OPS = (O.LatentBlend, O.LatentRenoise, O.DdimEtaStep)      # fp32 x with a per-element bound of its own, x_in its 16-bit rounding


def fields_of(op) -> Fields:
    f = FIELDS.get(type(op))
    if f is None:
        raise NotImplementedError(f"op_parity: no reference for op class {type(op).__name__}")
    known = set(f.inputs) | set(f.outputs) | set(f.scratch)
    for k, v in vars(op).items():
        if isinstance(v, torch.Tensor) and k not in known:
            raise NotImplementedError(f"op_parity: {type(op).__name__}.{k} is a tensor field without a reference")
    return f


def _int(t):
    return int(t.reshape(-1)[0].item())


def _sel(op):
    return _int(op.sel) if op.sel is not None else 0


def temb_rows(op, n_rows, width):
    """The fp32 rows of the temb table an op addresses, with the op's own strides: row r at sel * temb_sel_stride + r * temb_b_stride."""
    return torch.as_strided(op.temb, (n_rows, width), (op.temb_b_stride, 1), op.temb.storage_offset() + _sel(op) * op.temb_sel_stride)


def _temb_geometry(op):
    if isinstance(op, O.Gemm):
        M = (op.C if op.C.dim() == 2 else op.C[0]).shape[0]
        return -(-M // op.rows_per_b), op.W.shape[-2]
    return op.Y.shape[0], op.Y.shape[3]


def out_views(op, shadow=None):
    """{field: the live view an op writes}.  `shadow` (the snapshot) supplies values read when the kernel runs (the row of a GroupStats)."""
    src = shadow if shadow is not None else op
    if isinstance(op, O.Gemm):
        v = {"C": op.C}
        if op.Vt is not None:
            v["Vt"] = op.Vt[:, :, :op.vt_T]
        if op.rowstat is not None:
            v["rowstat"] = op.rowstat
        return v
    if isinstance(op, (O.Attn, O.Sdpa)):
        return {"O": op.O}
    if isinstance(op, (O.DdimStep, O.UniPCStep) + LATENT_OPS):
        v = {"x": op.x}
        if not isinstance(op, O.LatentBlend):             # the blend reads the counter the scheduler op has advanced
            v["step"] = op.step
        if op.x_in is not None:
            v["x_in"] = op.x_in if op.x_in.dtype == torch.float32 else op.x_in[:, :op.xin_c]
        if isinstance(op, O.UniPCStep):
            v.update(x_last=op.x_last, m1=op.m1, m2=op.m2)
        if isinstance(op, O.LatentRenoise):
            v["visit"] = op.visit
        if isinstance(op, O.DdimEtaStep):
            v["draw"] = op.draw
        return v
    if isinstance(op, O.ImageComposite):
        v = {"out": op.out}
        if op.matte is not None:
            v["matte"] = op.matte
        return v
    if isinstance(op, O.GroupStats):
        if op.row is not None:
            r = _int(src.row)
            n_rows = op.out.shape[0] if op.out.dim() == 3 else 1
            table = op.out if op.out.dim() == 3 else op.out[None]
            return {"out": table[r] if 0 <= r < n_rows else table[:0]}
        return {"out": op.out[0] if op.out.dim() == 3 else op.out}
    return {"Y": op.Y}


def slack_views(op):
    """Views an op MAY write, with zeros only: a GEMM whose N is no multiple of 4 is served by 8-byte stores and zero-fills the columns up to
    roundup4(N) (include/mdx.h asks for ldc >= roundup4(N); tests/test_tails_gpu.py holds the kernels to the zeros)."""
    if isinstance(op, O.Gemm) and op.C.shape[-1] % 4:
        C = op.C
        N = C.shape[-1]
        return [torch.as_strided(C, tuple(C.shape[:-1]) + (-N % 4,), C.stride(), C.storage_offset() + N)]
    return []


# ---- fp64 references, from include/mdx.h -----------------------------------------------------------------------------------------------
def _silu(x):
    return x * torch.sigmoid(x)


def _gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * (0.5 ** 0.5)))


def _epilogue(epi, raw):
    if epi == L.EPI_NONE:
        return raw
    if epi == L.EPI_SILU:
        return _silu(raw)
    if epi == L.EPI_GEGLU:                    # W rows interleaved [32 value | 32 gate]; C has N / 2 columns
        N = raw.shape[-1]
        r = raw.reshape(*raw.shape[:-1], N // 64, 2, 32)
        return (r[..., 0, :] * _gelu_erf(r[..., 1, :])).reshape(*raw.shape[:-1], N // 2)
    raise NotImplementedError(f"op_parity: epilogue {epi}")


def ref_gemm(op):
    A, W = op.A.to(F64), op.W.to(F64)
    if op.ln_eps > 0:                         # LayerNorm of the A rows; mean / rstd from the rows themselves, never from ln_stats
        A = (A - A.mean(-1, keepdim=True)) * torch.rsqrt(A.var(-1, unbiased=False, keepdim=True) + op.ln_eps)
    raw = A @ W.transpose(-1, -2)
    if op.bias is not None:
        raw = raw + op.bias.to(F64)
    if op.temb is not None:
        M = raw.shape[-2]
        nb, N = _temb_geometry(op)
        raw = raw + temb_rows(op, nb, N).to(F64).repeat_interleave(op.rows_per_b, 0)[:M]
    raw = _epilogue(op.epilogue, raw)
    out = {}
    if op.Vt is not None:                     # raw columns >= vt_from go to Vt[m // vt_T][n - vt_from][m % vt_T]
        Bv, Cv = op.Vt.shape[0], op.Vt.shape[1]
        out["Vt"] = raw[:, op.vt_from:].reshape(Bv, op.vt_T, Cv).transpose(1, 2)
        raw = raw[:, :op.vt_from]
    if op.R is not None:
        raw = raw + op.R.to(F64)
    out["C"] = raw
    return out


def _conv_epilogue(op, acc):
    if op.bias is not None:
        acc = acc + op.bias.to(F64)
    if op.temb is not None:
        acc = acc + temb_rows(op, acc.shape[0], acc.shape[3]).to(F64)[:, None, None, :]
    if op.epilogue == L.EPI_SILU:
        acc = _silu(acc)
    elif op.epilogue != L.EPI_NONE:
        raise NotImplementedError(f"op_parity: conv epilogue {op.epilogue}")
    if op.R is not None:
        acc = acc + op.R.to(F64)
    return acc


def _axis_classes(n_in, n_out):
    """MdxConvDesc.upsample2x, one axis: (class, first tap) per output index; the taps are (first, first + 1) of the low-res axis."""
    cls, t0 = [], []
    for o in range(n_out):
        j = o // 2
        if o % 2:
            cls.append(1); t0.append(j)
        elif n_out == 2 * n_in - 1 and o == n_out - 1:
            cls.append(2); t0.append(j - 1)
        else:
            cls.append(0); t0.append(j - 1)
    return cls, t0


def ref_conv_upsample2x(op):
    X, Wt = op.X.to(F64), op.Wt.to(F64)                   # Wt [ny * nx, Cout, 2, 2, Cin]
    B, Hi, Wi, Cin = X.shape
    _, Ho, Wo, Cout = op.Y.shape
    dev = X.device
    Xp = torch.zeros(B, Hi + 2, Wi + 2, Cin, dtype=F64, device=dev)
    Xp[:, 1:Hi + 1, 1:Wi + 1] = X
    cy, ty = _axis_classes(Hi, Ho)
    cx, tx = _axis_classes(Wi, Wo)
    nx = 2 + (Wo != 2 * Wi)
    acc = torch.zeros(B, Ho, Wo, Cout, dtype=F64, device=dev)
    for yc in sorted(set(cy)):
        oys = torch.tensor([o for o in range(Ho) if cy[o] == yc], device=dev)
        tys = torch.tensor([ty[o] + 1 for o in range(Ho) if cy[o] == yc], device=dev)
        for xc in sorted(set(cx)):
            oxs = torch.tensor([o for o in range(Wo) if cx[o] == xc], device=dev)
            txs = torch.tensor([tx[o] + 1 for o in range(Wo) if cx[o] == xc], device=dev)
            w = Wt[yc * nx + xc]
            val = 0
            for a in range(2):
                for b in range(2):
                    val = val + Xp[:, tys + a][:, :, txs + b] @ w[:, a, b, :].T
            acc[:, oys[:, None], oxs[None, :]] = val
    return {"Y": _conv_epilogue(op, acc)}


def ref_conv(op):
    """Sum over the taps of shifted-slice matmuls: no fp64 convolution backend is needed."""
    if op.upsample2x:
        return ref_conv_upsample2x(op)
    X, Wt = op.X.to(F64), op.Wt.to(F64)                   # Wt [Cout, kh, kw, Cin]
    B, Hi, Wi, Cin = X.shape
    Cout, kh, kw, _ = Wt.shape
    sh, sw = op.stride
    ph, pw = op.pad
    _, Ho, Wo, _ = op.Y.shape
    Hp = max(ph + Hi, (Ho - 1) * sh + kh)
    Wp = max(pw + Wi, (Wo - 1) * sw + kw)
    Xp = torch.zeros(B, Hp, Wp, Cin, dtype=F64, device=X.device)
    Xp[:, ph:ph + Hi, pw:pw + Wi] = X
    acc = torch.zeros(B, Ho, Wo, Cout, dtype=F64, device=X.device)
    for ky in range(kh):
        for kx in range(kw):
            acc += Xp[:, ky:ky + (Ho - 1) * sh + 1:sh, kx:kx + (Wo - 1) * sw + 1:sw] @ Wt[:, ky, kx, :].T
    return {"Y": _conv_epilogue(op, acc)}


def _softmax_pv(logits, v, prescaled, valid):
    """logits [H, Tq, n] (already scaled), v [H, n, d], valid bool broadcastable to logits or None -> [H, Tq, d]."""
    if valid is not None:
        logits = logits.masked_fill(~valid, -math.inf)
    m = logits.amax(-1, keepdim=True)
    p = torch.exp2(logits - m) if prescaled else torch.exp(logits - m)
    return (p / p.sum(-1, keepdim=True)) @ v


def ref_attn(op):
    Q, K = op.Q.to(F64), op.K.to(F64)
    B, Tq, C = Q.shape
    H, Tk = op.heads, op.Tk
    d = C // H
    Vs = op.Vt.to(F64) if op.v_rowmajor else op.Vt.to(F64)[:, :, :Tk].transpose(1, 2)        # [Bkv, Tk, C]
    sc = 1.0 if op.q_prescaled else op.scale
    kvmap = op.kvmap.reshape(B, op.nsrc).tolist() if op.kvmap is not None else [[b] for b in range(B)]
    if op.tk_dev is not None:
        counts = [_int(op.tk_dev)] * B
    elif op.tk_rows is not None:
        counts = op.tk_rows.tolist()
    else:
        counts = [Tk] * B
    heads = lambda x: x.reshape(x.shape[0], H, d).transpose(0, 1)                            # [T, C] -> [H, T, d]
    out = torch.zeros(B, Tq, C, dtype=F64, device=Q.device)
    causal = torch.ones(Tq, Tk, dtype=torch.bool, device=Q.device).tril() if op.causal else None
    for b in range(B):
        n = counts[b]
        if n < 1 or n > Tk:                   # include/mdx.h: every O row of the batch is NaN
            out[b] = math.nan
            continue
        q = heads(Q[b])
        srcs = [s for s in kvmap[b] if s >= 0] if not op.joint else kvmap[b]
        if op.joint:
            k = torch.cat([heads(K[s][:n]) for s in srcs], 1)
            v = torch.cat([heads(Vs[s][:n]) for s in srcs], 1)
            srcs_kv = [(k, v)]
        else:
            srcs_kv = [(heads(K[s][:n]), heads(Vs[s][:n])) for s in srcs]
        acc = torch.zeros(H, Tq, d, dtype=F64, device=Q.device)      # no source present: zeros
        for k, v in srcs_kv:
            valid = causal[:, :k.shape[1]] if causal is not None else None
            acc = acc + _softmax_pv(q @ k.transpose(1, 2) * sc, v, op.q_prescaled, valid)
        out[b] = acc.transpose(0, 1).reshape(Tq, C)
    return {"O": out}


def ref_groupnorm(op):
    B, HW, C = op.X.shape
    G = op.groups
    x = op.X.to(F64).reshape(B, HW, G, C // G)
    mean = x.mean((1, 3), keepdim=True)
    var = ((x - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((x - mean) * torch.rsqrt(var + op.eps)).reshape(B, HW, C) * op.gamma.to(F64) + op.beta.to(F64)
    return {"Y": _silu(y) if op.silu else y}


def ref_layernorm(op):
    x = op.X.to(F64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return {"Y": (x - mean) * torch.rsqrt(var + op.eps) * op.gamma.to(F64) + op.beta.to(F64)}


def ref_softmax(op):
    y = torch.zeros(op.Y.shape, dtype=F64, device=op.X.device)       # columns T.. are written as zeros
    y[:, :op.T] = torch.softmax(op.X[:, :op.T].to(F64) * op.scale, -1)
    return {"Y": y}


def ref_ew(op):
    x = op.X.to(F64)
    if op.kind == L.EW_ADD:
        return {"Y": op.Y.to(F64) + x}
    if op.kind == L.EW_COPY:
        return {"Y": x}
    if op.kind == L.EW_SILU:
        return {"Y": _silu(x)}
    if op.kind == L.EW_SCALE:
        return {"Y": x * op.alpha}
    raise NotImplementedError(f"op_parity: elementwise kind {op.kind}")


def ref_upsample(op):
    return {"Y": op.X.to(F64)[:, op.ymap.long()][:, :, op.xmap.long()]}


def ref_layout(op):
    return {"Y": op.X.to(F64).permute(0, 2, 3, 1) if op.to_nhwc else op.X.to(F64).permute(0, 3, 1, 2)}


def ref_fourier(op):
    x = op.X.to(F64)                          # [n, P, 3]
    parts = [x]
    for k in range(op.F):
        parts += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    e = torch.cat(parts, -1).reshape(x.shape[0], -1)
    if op.mask is not None:                   # pos * m + null * (1 - m)
        m = op.mask.to(F64)[:, None]
        null = op.null_feat.to(F64)[None] if op.null_feat is not None else torch.zeros_like(e[:1])
        e = e * m + null * (1 - m)
    return {"Y": e}


def ref_gather(op):
    Tt = op.T.to(F64)
    rows = Tt[op.idx.clamp(0, Tt.shape[0] - 1)]
    if op.mask is not None:
        null = op.null_row.to(F64)[None] if op.null_row is not None else torch.zeros_like(rows[:1])
        rows = torch.where(op.mask.bool()[:, None], rows, null.expand_as(rows))
    if op.add is not None:
        period = op.add.shape[0]
        rows = rows + op.add.to(F64)[torch.arange(rows.shape[0], device=rows.device) % period]
    return {"Y": rows}


def ref_timeemb(op):
    dim = op.Y.shape[1]
    half = dim // 2
    f = torch.exp(-math.log(op.max_period) * torch.arange(half, dtype=F64, device=op.t.device) / (half - op.freq_shift))
    a = op.t.to(F64)[:, None] * f[None]
    return {"Y": torch.cat([torch.cos(a), torch.sin(a)], -1) if op.flip_sin_to_cos else torch.cat([torch.sin(a), torch.cos(a)], -1)}


def _sched_common(op):
    n = op.x.numel()
    s = _int(op.step)
    c = op.coef[s].to(F64)
    eps = op.eps.to(F64).reshape(-1)
    e = eps[:n] + op.guidance * (eps[n:] - eps[:n]) if op.cfg else eps
    given = None
    if op.gv_mode:
        given = op.gv_mask.bool().repeat_interleave(n // op.gv_mask.numel())
        if op.gv_mode == 2:
            e = torch.where(given, op.gv_noise.to(F64).reshape(-1), e)
    return n, s, c, e, given


def _sched_outputs(op, xn, s, extra):
    out = {"x": xn.reshape(op.x.shape), "step": op.step.to(F64) + 1}
    if op.x_in is not None:
        c = 2 if op.cfg else 1
        if op.x_in.dtype == torch.float32:
            out["x_in"] = xn.repeat(c).reshape(op.x_in.shape)
        else:
            out["x_in"] = xn.reshape(-1, op.xin_c).repeat(c, 1)
    out.update(extra)
    return out


def ref_ddim(op):
    n, s, c, e, given = _sched_common(op)
    x = op.x.to(F64).reshape(-1)
    x0 = (x - c[1] * e) / c[0]
    xn = c[2] * x0 + c[3] * e
    if op.gv_mode == 1 and s < op.gv_last_step:
        xn = torch.where(given, c[2] * op.gv_cond.to(F64).reshape(-1) + c[3] * op.gv_noise.to(F64).reshape(-1), xn)
    return _sched_outputs(op, xn, s, {})


def ref_unipc(op):
    n, s, c, e, given = _sched_common(op)
    x, x_last, m1, m2 = (t.to(F64).reshape(-1) for t in (op.x, op.x_last, op.m1, op.m2))
    mt = c[0] * x + c[1] * e
    xc = c[3] * x_last + c[4] * m1 + c[5] * m2 + c[6] * mt if float(c[2]) != 0 else x
    xn = c[7] * xc + c[8] * mt + c[9] * m1
    if op.gv_mode == 1 and s < op.gv_last_step:
        xn = torch.where(given, c[10] * op.gv_cond.to(F64).reshape(-1) + c[11] * op.gv_noise.to(F64).reshape(-1), xn)
    return _sched_outputs(op, xn, s, {"x_last": xc.reshape(op.x_last.shape), "m1": mt.reshape(op.m1.shape), "m2": m1.reshape(op.m2.shape)})


def group_stats64(X):
    """fp64 (nonfinite, absmax, sum, sumsq, sum |x|) per group of X [G, ...] over its finite elements."""
    x = X.to(F64).reshape(X.shape[0], -1)
    fin = torch.isfinite(x)
    xz = torch.where(fin, x, torch.zeros_like(x))
    return (~fin).sum(1).to(F64), xz.abs().amax(1), xz.sum(1), (xz * xz).sum(1), xz.abs().sum(1)


def ref_group_stats(op):
    bad, amax, s, q, _ = group_stats64(op.X)
    rec = torch.stack([bad, amax, s, q], -1)
    if op.row is not None:
        r = _int(op.row)
        n_rows = op.out.shape[0] if op.out.dim() == 3 else 1
        if not 0 <= r < n_rows:               # a row outside the table writes nothing
            return {"out": torch.zeros((0,) + tuple(op.out.shape[-2:]), dtype=F64, device=op.X.device)}
    return {"out": rec}


def ref_sdpa(op):
    """MdxSdpaDesc: softmax(scale Q K^T + mask) V per head; causal: key j visible to query i iff j <= i; klen: batch b sees its first
    klen[b] keys, a count outside [1, Tk] gives NaN rows for that batch."""
    Q, K, Vv = op.Q.to(F64), op.K.to(F64), op.V.to(F64)
    B, Tq, C = Q.shape
    Tk, H = K.shape[1], op.heads
    d = C // H
    heads = lambda x: x.reshape(x.shape[0], H, d).transpose(0, 1)
    counts = op.klen.tolist() if op.klen is not None else [Tk] * B
    out = torch.zeros(B, Tq, C, dtype=F64, device=Q.device)
    causal = torch.ones(Tq, Tk, dtype=torch.bool, device=Q.device).tril() if op.causal else None
    for b in range(B):
        n = counts[b]
        if n < 1 or n > Tk:
            out[b] = math.nan
            continue
        s = heads(Q[b]) @ heads(K[b, :n]).transpose(1, 2) * op.scale
        if causal is not None:
            s = s.masked_fill(~causal[:, :n], -math.inf)
        out[b] = (torch.softmax(s, -1) @ heads(Vv[b, :n])).transpose(0, 1).reshape(Tq, C)
    return {"O": out}


# The four latent ops below return, next to their outputs, "_bound": {field: per-element absolute bound, fp64} — the bound the op's own
# kernel test applies to the same kernel — and "_written": the elements of x the contract says are written (their x_in copies must be the
# 16-bit rounding of the stored x, bit for bit, as every one of those kernel tests asserts).
NOISE_LIMIT = 1e-5                            # tests/test_latent_renoise_gpu.py: |z_fp32 - z_fp64| of the documented evaluation
ULP = 2.0 ** -23                              # tests/test_ddim_eta_contract.py: one fp32 operation charged one ulp


def _xin_ref(op, xn, written):
    """x_in after a latent op: the new latents in every CFG half where the op wrote them, the snapshot's value elsewhere."""
    c = 2 if op.cfg else 1
    old = op.x_in.to(F64)
    if op.x_in.dtype == torch.float32:
        return torch.where(written.repeat(c), xn.repeat(c), old.reshape(-1)).reshape(op.x_in.shape)
    new = xn.reshape(-1, op.xin_c).repeat(c, 1)
    return torch.where(written.reshape(-1, op.xin_c).repeat(c, 1), new, old[:, :op.xin_c])


def _group_noise(seeds, counter, n, fn, device):
    """fp64 [n]: fn(seed, counter, n / groups) of every group, in order (tests/philox_ref.py)."""
    ge = n // seeds.numel()
    return torch.from_numpy(np.concatenate([fn(int(s), counter, ge) for s in seeds.tolist()])).to(device)


def ref_latent_blend(op):
    """MdxBlendDesc.  Bound (tests/test_latent_blend_gpu.py): 4 * 2^-24 * (|a cond| + |sg noise| + |x|) where something is written; an
    m == 0 element keeps its bits."""
    n = op.x.numel()
    x = op.x.to(F64).reshape(-1)
    s = _int(op.step) - 1
    ld = op.coef.shape[1]
    ca, cs = (op.col_a, op.col_s) if min(op.col_a, op.col_s) >= 0 else O.LatentBlend.COLUMNS[ld]
    if s < 0 or s >= op.last_step:
        xn, written, bound = x, torch.zeros(n, dtype=torch.bool, device=x.device), torch.zeros_like(x)
    else:
        a, sg = op.coef[s, ca].to(F64), op.coef[s, cs].to(F64)
        m = op.mask.to(F64).reshape(-1).repeat_interleave(n // op.mask.numel())
        ac, sn = a * op.cond.to(F64).reshape(-1), sg * op.noise.to(F64).reshape(-1)
        t = ac + sn
        xn = torch.where(m == 0, x, torch.where(m == 1, t, x + m * (t - x)))
        written = m != 0
        bound = torch.where(written, 4 * U24 * (ac.abs() + sn.abs() + x.abs()), torch.zeros_like(x))
    out = {"x": xn.reshape(op.x.shape), "_bound": {"x": bound.reshape(op.x.shape)}, "_written": written}
    if op.x_in is not None:
        out["x_in"] = _xin_ref(op, xn, written)
    return out


def ref_latent_renoise(op):
    """MdxRenoiseDesc, with the contract's fp32 r and sg (a correctly rounded division, 1 - r r with one rounding, a correctly rounded
    square root) as tests/test_latent_renoise_gpu.py takes them.  Bound (the same test): 1e-5 sg + 4 * 2^-24 |ref|."""
    n = op.x.numel()
    x = op.x.to(F64).reshape(-1)
    c, v = _int(op.step), _int(op.visit)
    ld, rows = op.coef.shape[1], op.coef.shape[0]
    ct, cp = (op.col_t, op.col_p) if min(op.col_t, op.col_p) >= 0 else O.LatentRenoise.COLUMNS[ld]
    keep = {"step": op.step.to(F64), "visit": op.visit.to(F64)}
    if op.jump < 1 or c < 1 or c > rows or c - op.jump < 0:      # x is filled with NaN, x_in and both counters are left alone
        out = {"x": torch.full(op.x.shape, math.nan, dtype=F64, device=x.device), "_bound": {}, "_written": torch.zeros(n, dtype=torch.bool, device=x.device), **keep}
        if op.x_in is not None:
            out["x_in"] = _xin_ref(op, x, out["_written"])
        return out
    r32 = op.coef[c - op.jump, ct].float() / op.coef[c - 1, cp].float()
    r = r32.to(F64)
    sg = (1.0 - r * r).float().clamp_min(0).sqrt().to(F64)
    z = _group_noise(op.seeds, v, n, PH.noise_ref, x.device)
    xn = r * x + sg * z
    written = torch.ones(n, dtype=torch.bool, device=x.device)
    out = {"x": xn.reshape(op.x.shape), "step": op.step.to(F64) - op.jump, "visit": op.visit.to(F64) + 1,
           "_bound": {"x": (NOISE_LIMIT * sg + 4 * U24 * xn.abs()).reshape(op.x.shape)}, "_written": written}
    if op.x_in is not None:
        out["x_in"] = _xin_ref(op, xn, written)
    return out


def ref_ddim_eta(op):
    """MdxDdimEtaDesc.  Bound: the scheduler-level one of tests/test_ddim_eta_gpu.py for the kernel's own roundings, 9 * ULP * S with
    S = c2 (|x| + c1 |e|) / c0 + dir |e| + std |z| and ULP = 2^-23, plus the 1e-5 std of a generated z (tests/test_latent_renoise_gpu.py);
    the table terms of that test are absent because var IS this op's table.  Under CFG |e| stands for |eps_u| + g |eps_c - eps_u|, the sum of
    the magnitudes the three roundings of the guidance combine act on (it bounds |e|, and 3 * 2^-24 of it bounds their error: within the
    18 * 2^-24 S of the nine operations).  A gv_mode 1 element is two products and a sum: the kernel test's 2 * 2^-24 (|c2 cond| + |c3 noise| + |t|)."""
    n = op.x.numel()
    x = op.x.to(F64).reshape(-1)
    s, v = _int(op.step), _int(op.draw)
    rows = op.coef.shape[0] if op.n_rows < 0 else op.n_rows
    keep = {"step": op.step.to(F64), "draw": op.draw.to(F64)}
    if s < 0 or s >= rows:
        out = {"x": torch.full(op.x.shape, math.nan, dtype=F64, device=x.device), "_bound": {}, "_written": torch.zeros(n, dtype=torch.bool, device=x.device), **keep}
        if op.x_in is not None:
            out["x_in"] = _xin_ref(op, x, out["_written"])
        return out
    c = op.coef[s].to(F64)
    dirv, std = (torch.full_like(x, float(t)) for t in op.var[s].to(F64))
    eps = op.eps.to(F64).reshape(-1)
    if op.cfg:
        g = float(np.float32(op.guidance))
        e = eps[:n] + g * (eps[n:] - eps[:n])
        emag = eps[:n].abs() + g * (eps[n:] - eps[:n]).abs()
    else:
        e, emag = eps, eps.abs()
    given = torch.zeros(n, dtype=torch.bool, device=x.device)
    if op.gv_mode:
        given = op.gv_mask.bool().repeat_interleave(n // op.gv_mask.numel())
        if op.gv_mode == 2:
            gn = op.gv_noise.to(F64).reshape(-1)
            e, emag = torch.where(given, gn, e), torch.where(given, gn.abs(), emag)
            dirv, std = torch.where(given, c[3], dirv), torch.where(given, torch.zeros_like(std), std)
    if op.noise is not None:
        z, zerr = op.noise.to(F64).reshape(-1), 0.0
    else:
        z, zerr = _group_noise(op.seeds, v, n, PH.eta_noise_ref, x.device), NOISE_LIMIT
    x0 = (x - c[1] * e) / c[0]
    xn = c[2] * x0 + dirv * e + std * z
    S = c[2] * (x.abs() + c[1] * emag) / c[0] + dirv * emag + std * z.abs()
    bound = 9 * ULP * S + zerr * std
    if op.gv_mode == 1 and s < op.gv_last_step:
        cc, nn = c[2] * op.gv_cond.to(F64).reshape(-1), c[3] * op.gv_noise.to(F64).reshape(-1)
        xn = torch.where(given, cc + nn, xn)
        bound = torch.where(given, 2 * U24 * (cc.abs() + nn.abs() + (cc + nn).abs()), bound)
    written = torch.ones(n, dtype=torch.bool, device=x.device)
    out = {"x": xn.reshape(op.x.shape), "step": op.step.to(F64) + 1, "draw": op.draw.to(F64) + 1, "_bound": {"x": bound.reshape(op.x.shape)}, "_written": written}
    if op.x_in is not None:
        out["x_in"] = _xin_ref(op, xn, written)
    return out


def _matte64(keep, f, r):
    """MdxCompositeDesc's matte in fp64: a = nearest upsample of keep, e = min of a over the (2r+1)^2 window, w = the mean of e over the
    (2r+1)^2 window, every coordinate clamped to the image."""
    a = keep.to(F64).repeat_interleave(f, dim=-2).repeat_interleave(f, dim=-1)
    if r == 0:
        return a
    H, W = a.shape[-2:]
    iy, ix = torch.arange(H, device=a.device), torch.arange(W, device=a.device)
    win = range(-r, r + 1)
    e = torch.stack([a[..., (iy + k).clamp(0, H - 1), :] for k in win]).amin(0)
    e = torch.stack([e[..., (ix + k).clamp(0, W - 1)] for k in win]).amin(0)
    s = torch.stack([e[..., (iy + k).clamp(0, H - 1), :] for k in win]).sum(0)
    s = torch.stack([s[..., (ix + k).clamp(0, W - 1)] for k in win]).sum(0)
    return s / float((2 * r + 1) ** 2)


def ref_image_composite(op):
    """MdxCompositeDesc.  g is the contract's own value, bit for bit: fmaf(gen, 0.5, 0.5) is ONE fp32 rounding of the exact sum, then the
    rounding to gen's 16-bit type, then the clamp.  Bounds (tests/test_composite_gpu.py): the matte within 2^-24 for masks on the 1/64 grid
    (every window sum exact), within (2 (2r+1) + 2) * 2^-24 for any other mask; out bit-equal to g where w == 0 and to orig where w == 1,
    within 4 * 2^-24 between — plus, off the grid only, the matte's own bound times |orig - g|, which is how far that error can move the
    mix.  has[v] == 0: out = g, matte = 0."""
    gen = op.gen
    r = int(op.feather)
    V, Cc, H, W = gen.shape
    f = H // op.keep.shape[1]
    g32 = (gen.to(F64) * 0.5 + 0.5).float()
    if gen.dtype != torch.float32:
        g32 = g32.to(gen.dtype).float()
    g = g32.clamp(0, 1).to(F64).permute(0, 2, 3, 1)
    w = _matte64(op.keep, f, r)
    orig = op.orig.to(F64)
    on_grid = bool((op.keep.to(F64) * 64 == (op.keep.to(F64) * 64).round()).all())
    mb = U24 if on_grid else (2 * (2 * r + 1) + 2) * U24
    if op.has is not None:
        absent = (op.has == 0).view(V, 1, 1)
        w = torch.where(absent, torch.zeros_like(w), w)
        orig = torch.where(absent[..., None], g, orig)        # the orig and keep rows of such a view are not read
    w4 = w[..., None]
    zero, one = w4 == 0, w4 == 1
    ref = torch.where(zero, g, torch.where(one, orig, g + w4 * (orig - g)))
    ob = torch.where(zero | one, torch.zeros_like(ref), 4 * U24 + (0.0 if on_grid else mb) * (orig - g).abs())
    exact = (w == 0) | (w == 1)
    out = {"out": ref, "_bound": {"out": ob, "matte": torch.where(exact, torch.zeros_like(w), torch.full_like(w, mb)) if on_grid else torch.full_like(w, mb)}}
    if op.matte is not None:
        out["matte"] = w
    return out


REFERENCE = {O.Gemm: ref_gemm, O.Conv: ref_conv, O.Attn: ref_attn, O.GroupNorm: ref_groupnorm, O.GroupNormResident: ref_groupnorm,
             O.LayerNorm: ref_layernorm, O.Softmax: ref_softmax, O.Ew: ref_ew, O.Upsample: ref_upsample, O.Layout: ref_layout,
             O.Fourier: ref_fourier, O.Gather: ref_gather, O.TimeEmb: ref_timeemb, O.DdimStep: ref_ddim, O.UniPCStep: ref_unipc,
             O.GroupStats: ref_group_stats, O.Sdpa: ref_sdpa, O.LatentBlend: ref_latent_blend, O.LatentRenoise: ref_latent_renoise,
             O.DdimEtaStep: ref_ddim_eta, O.ImageComposite: ref_image_composite}


def reference(op):
    """{output field: fp64 tensor of the shape of out_views(op)[field]} — every output field except Gemm.rowstat, which include/mdx.h
    defines on the STORED C (rowstat_reference).  Keys that start with "_" are not outputs (the latent ops' bounds)."""
    fields_of(op)
    with torch.no_grad():
        return REFERENCE[type(op)](op)


def rowstat_reference(C_stored):
    """(sum, sum of squares) per row of the stored C over all its columns: what a consumer gets by adding the parts."""
    c = C_stored.to(F64)
    return torch.stack([c.sum(-1), (c * c).sum(-1)], -1)


# ---- emulations for the "twice the emulation" rule -------------------------------------------------------------------------------------
def emulate(op, field):
    """The fp32 rounding model of tests/values_data.py for an op form whose documented rounding may be wider than close()'s table, or None.
    `op` is a snapshot.  Models, not the code under test."""
    with torch.no_grad():
        if isinstance(op, O.Gemm) and op.C.dim() == 2 and op.temb is None and op.C.dtype in H16:
            dt = op.C.dtype
            zero = torch.zeros(op.W.shape[0], dtype=torch.float32, device=op.A.device)
            bias = op.bias.float() if op.bias is not None else zero
            if op.ln_eps > 0:
                acc = V.emu_ln_fused(op.A, op.W, bias, op.ln_csum.float(), torch.float32, eps=op.ln_eps)
                acc = _epilogue(op.epilogue, acc)
                if field == "Vt":
                    Bv, Cv = op.Vt.shape[0], op.Vt.shape[1]
                    return acc[:, op.vt_from:].reshape(Bv, op.vt_T, Cv).transpose(1, 2).to(dt)
                if op.Vt is not None:
                    acc = acc[:, :op.vt_from]
                if op.R is not None:
                    acc = acc.to(dt).float() + op.R.float()
                return acc.to(dt)
            if field == "C" and op.epilogue == L.EPI_NONE and op.Vt is None:
                d = dict(A=op.A, W=op.W, bias=bias, R=op.R)
                return V.emu_gemm(d, dt, use_bias=True, use_R=op.R is not None, staged=True)
        if isinstance(op, (O.GroupNorm, O.GroupNormResident)) and field == "Y":
            return V.emu_gn(op.X, op.groups, op.gamma.float(), op.beta.float(), op.eps, op.silu)
    return None


# ---- the walker ------------------------------------------------------------------------------------------------------------------------
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    t = t.contiguous()
    return t.view(_INT_OF[t.element_size()]) if t.is_floating_point() else t


def _storage_bytes(t):
    s = t.untyped_storage()
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(s, 0, (s.nbytes(),))


def _byte_mask(t):
    """bool per byte of t's storage: the bytes of the view t."""
    es = t.element_size()
    nbytes = t.untyped_storage().nbytes()
    m = torch.zeros(nbytes // es, dtype=torch.bool, device=t.device)
    if t.numel():
        torch.as_strided(m, t.shape, t.stride(), t.storage_offset()).fill_(True)
    mb = m.repeat_interleave(es) if es > 1 else m
    if mb.numel() < nbytes:
        mb = torch.cat([mb, torch.zeros(nbytes - mb.numel(), dtype=torch.bool, device=t.device)])
    return mb


def _snap(t):
    return t.detach().clone(memory_format=torch.contiguous_format)


def snapshot(op):
    """A copy of the op whose tensor fields are clones taken now (temb: the addressed rows, re-addressed as a dense table)."""
    f = fields_of(op)
    rep = {}
    for k, v in vars(op).items():
        if not isinstance(v, torch.Tensor):
            continue
        if k in f.scratch:
            rep[k] = None
        elif k == "temb":
            nb, width = _temb_geometry(op)
            rep[k] = _snap(temb_rows(op, nb, width))
        else:
            rep[k] = _snap(v)
    if getattr(op, "temb", None) is not None:
        rep.update(sel=None, temb_sel_stride=0, temb_b_stride=rep["temb"].shape[1])
    return dataclasses.replace(op, **rep)


def metrics(out, ref, kind):
    """The three quantities helpers.close() asserts on, computed the same way."""
    out = out.float(); ref = ref.float().to(out.device)
    scale = ref.abs().mean().item() + 1e-6
    err = (out - ref).abs()
    tol = helpers.XF_ATOL[kind] * scale + helpers.XF_RTOL[kind] * ref.abs()
    rel = (err.pow(2).sum().sqrt() / (ref.pow(2).sum().sqrt() + 1e-12)).item()
    return dict(rel_l2=rel, worst=(err / tol).max().item(), frac=(err > tol).float().mean().item())


def rel_l2_64(out, ref):
    return float((out.to(F64) - ref).norm() / (ref.norm() + 1e-300))


_LOG = helpers.parity_log      # the real logger, whatever _quiet_parity_log has swapped in


@contextlib.contextmanager
def _quiet_parity_log():
    """One summary line per case goes to the parity log, not one per op output."""
    keep = helpers.parity_log
    helpers.parity_log = lambda *a, **k: None
    try:
        yield
    finally:
        helpers.parity_log = keep


@dataclasses.dataclass
class Record:
    index: int
    name: str
    cls: str
    kernel: str
    rel_l2: float = 0.0          # worst over the op's outputs
    worst: float = 0.0           # worst err / tol over the op's 16-bit outputs (fp32 outputs: error / bound)
    rule: str = "close"
    emu_rel_l2: float = None
    failures: list = dataclasses.field(default_factory=list)


def _judge_xin_bits(op, aux, fail):
    """A latent op's 16-bit x_in: every CFG half of a written element is the rounding of the STORED x, bit for bit."""
    if op.x_in is None or op.x_in.dtype == torch.float32 or not bool(aux["_written"].any()):
        return
    wr = aux["_written"].reshape(-1, op.xin_c)
    want = op.x.reshape(-1, op.xin_c).to(op.x_in.dtype)
    halves = op.x_in[:, :op.xin_c].reshape(2 if op.cfg else 1, -1, op.xin_c)
    for hf in range(halves.shape[0]):
        if not torch.equal(_bits(halves[hf][wr]), _bits(want[wr])):
            fail("values", f"x_in half {hf} is not the 16-bit rounding of the stored x")


def _judge_values(op, shadow, field, out, ref, rec, plan, fail, aux=None):
    """Values + finite for one output field.  aux: everything reference() returned (the latent ops' bounds)."""
    aux = aux or {}
    if out.numel() == 0:
        if ref.numel() != 0:
            fail("values", f"{field}: nothing to write but the reference has {ref.numel()} elements")
        return
    if tuple(out.shape) != tuple(ref.shape):
        fail("values", f"{field}: shape {tuple(out.shape)} vs reference {tuple(ref.shape)}")
        return
    nan = torch.isnan(ref)
    if bool(nan.any()):                       # the contract says NaN here (key count out of range)
        if not bool(torch.isnan(out[nan]).all()):
            fail("finite", f"{field}: the contract asks for NaN rows")
        if bool(nan.all()):
            return
        out, ref = out[~nan], ref[~nan]
    if not bool(torch.isfinite(out.float()).all()):
        fail("finite", f"{field}: {int((~torch.isfinite(out.float())).sum())} non-finite elements")
        return
    if not out.is_floating_point():           # the step counter
        if not torch.equal(out.to(F64), ref):
            fail("values", f"{field}: {out.tolist()} != {ref.tolist()}")
        return
    if out.dtype in H16:
        kind = "bf16" if out.dtype == torch.bfloat16 else "f16"
        m = metrics(out, ref, kind)
        rec.rel_l2, rec.worst = max(rec.rel_l2, m["rel_l2"]), max(rec.worst, m["worst"])
        try:
            helpers.close(out, ref, name=f"{rec.name}.{field}", kind=kind)
        except AssertionError as e:
            emu = emulate(shadow, field)
            if emu is None:
                fail("values", str(e)); return
            me = metrics(emu, ref, kind)
            limit = 4e-3 if kind == "bf16" else 6e-4
            if me["frac"] <= 1e-4 and me["worst"] <= 1.5 and me["rel_l2"] < limit:
                fail("values", f"the emulation passes close() (rel_l2 {me['rel_l2']:.3e}) and the kernel does not: {e}"); return
            rec.rule, rec.emu_rel_l2 = "2x emulation", me["rel_l2"]
            _LOG(f"op_parity:{plan}:{rec.name}", field=field, kind=kind, rel_l2=m["rel_l2"], emulation_rel_l2=me["rel_l2"])
            if not m["rel_l2"] <= 2 * me["rel_l2"]:
                fail("values", f"{field}: rel_l2 {m['rel_l2']:.3e} > 2 x emulation {me['rel_l2']:.3e}")
        return
    # fp32 outputs
    o64 = out.to(F64)
    if isinstance(op, LATENT_OPS + (O.ImageComposite,)):          # a per-element bound from the op's own kernel test (see the references)
        b = aux.get("_bound", {})
        if field == "x_in":                   # an fp32 x_in holds x itself, once per CFG half
            bx = b.get("x")
            bound = bx.reshape(-1).repeat(2 if op.cfg else 1).reshape(out.shape) if bx is not None else torch.zeros_like(ref)
        else:
            bound = b[field]
        err = (o64 - ref).abs()
        w = float((err / bound.clamp_min(1e-300)).max())          # a bound of zero (an element the contract leaves alone or copies) asks for the bits
        rec.rel_l2, rec.worst = max(rec.rel_l2, rel_l2_64(o64, ref)), max(rec.worst, min(w, 1e30))
        if not w <= 1.0:
            at = int((err / bound.clamp_min(1e-300)).reshape(-1).argmax())
            fail("values", f"{field}: |err| / bound = {w:.3e} at element {at} (|err| {float(err.reshape(-1)[at]):.3e}, bound {float(bound.reshape(-1)[at]):.3e})")
    elif isinstance(op, (O.Gemm, O.Conv)):
        rel = rel_l2_64(o64, ref)
        rec.rel_l2, rec.worst = max(rec.rel_l2, rel), max(rec.worst, rel / T.F32_REL_L2)
        if not rel < T.F32_REL_L2:
            fail("values", f"{field}: fp32 rel_l2 {rel:.3e} >= {T.F32_REL_L2}")
    elif isinstance(op, (O.TimeEmb, O.DdimStep, O.UniPCStep)):
        if isinstance(op, O.TimeEmb):
            atol = T.ABS_BOUND["timeemb"]
        elif isinstance(op, O.DdimStep):
            atol = T.ABS_BOUND["ddim"]
        else:
            atol = T.UNIPC_ATOL_REL * float(ref.abs().max())
        bound = atol + 1e-5 * ref.abs()       # torch.allclose(atol=..., rtol=1e-5), as the kernel tests apply it
        w = float(((o64 - ref).abs() / bound.clamp_min(1e-300)).max())      # a bound of zero (a state buffer that is still zero) asks for zero
        rec.rel_l2, rec.worst = max(rec.rel_l2, rel_l2_64(o64, ref)), max(rec.worst, w)
        if not w <= 1.0:
            fail("values", f"{field}: |err| / (atol {atol:.2e} + 1e-5 |ref|) = {w:.3f}")
    elif isinstance(op, (O.Ew, O.Layout, O.Upsample)):      # fp32 copies / sums: one fp32 rounding
        rel = rel_l2_64(o64, ref)
        rec.rel_l2 = max(rec.rel_l2, rel)
        if not rel < T.F32_REL_L2:
            fail("values", f"{field}: fp32 rel_l2 {rel:.3e} >= {T.F32_REL_L2}")
    else:
        raise NotImplementedError(f"op_parity: no fp32 bound for {type(op).__name__}.{field}")


def _judge_group_stats(op, shadow, out, rec, fail):
    if out.numel() == 0:
        return
    bad, amax, s, q, sabs = group_stats64(shadow.X)
    n = shadow.X.numel() // max(1, shadow.X.shape[0])
    k = O.GroupStats.chain_length(n, shadow.X.dtype == torch.float32)
    if not torch.equal(out[:, 0].to(F64), bad):
        fail("values", f"nonfinite {out[:, 0].tolist()} != {bad.tolist()}")
    if not torch.equal(_bits(out[:, 1]), _bits(amax.float())):
        fail("values", "absmax is not bit-exact")
    es, eq = (out[:, 2].to(F64) - s).abs(), (out[:, 3].to(F64) - q).abs()
    w = max(float((es / (k * U24 * sabs).clamp_min(1e-300)).max()), float((eq / (k * U24 * q).clamp_min(1e-300)).max()))
    rec.worst = max(rec.worst, w)
    if not w <= 1.0:
        fail("values", f"sum / sumsq error over the k(n) = {k} chain bound: {w:.3f}")
    if not bool(torch.isfinite(out).all()):
        fail("finite", "record not finite")


def walk(ops, execute, compare=all, kernel=None, plan="", stop=True):
    """Run `ops` in order through execute(op); judge the ops `compare` selects (all: every op; else a predicate (index, op) -> bool, or a
    collection of indices).  kernel(): name of the kernel the last op launched ("" without one).  Returns the Records of the judged ops;
    a missed condition raises OpParityError at once (stop=False: it is recorded in Record.failures and the walk goes on).
    Whatever execute() or the device synchronisation raises ends the walk: nothing more is launched."""
    if compare is all:
        want = lambda i, op: True
    elif callable(compare):
        want = compare
    else:
        chosen = set(compare)
        want = lambda i, op: i in chosen
    asked = sum(1 for i, op in enumerate(ops) if want(i, op))
    records = []
    with torch.no_grad(), _quiet_parity_log():
        for i, op in enumerate(ops):
            cuda = any(isinstance(v, torch.Tensor) and v.is_cuda for v in vars(op).values())
            if not want(i, op):
                execute(op)
                if cuda:
                    torch.cuda.synchronize()
                continue
            f = fields_of(op)
            sel_before = _snap(op.sel) if getattr(op, "sel", None) is not None else None
            shadow = snapshot(op)
            views = out_views(op, shadow)
            # storages behind the outputs, and the bytes of them the op may write
            stor = {}
            for k, v in views.items():
                key = v.untyped_storage().data_ptr()
                if key not in stor:
                    stor[key] = [v, _storage_bytes(v).clone(), _byte_mask(v)]
                else:
                    stor[key][2] |= _byte_mask(v)
            slack = []
            for v in slack_views(op):
                stor[v.untyped_storage().data_ptr()][2] |= _byte_mask(v)
                slack.append((v, _snap(v)))
            checked_inputs = []
            for k in f.inputs:
                v = getattr(op, k, None)
                if not isinstance(v, torch.Tensor):
                    continue
                live = temb_rows(op, *_temb_geometry(op)) if k == "temb" else v
                key = v.untyped_storage().data_ptr()
                if key in stor and v.numel() and k != "temb" and bool((_byte_mask(v) & stor[key][2]).any()):
                    continue                  # an in / out operand (R aliased to C): read from the snapshot, free to change
                snap = sel_before if k == "sel" else getattr(shadow, k)
                checked_inputs.append((k, live, snap))
            execute(op)
            if cuda:
                torch.cuda.synchronize()      # a HIP error surfaces here and ends the walk
            kern = kernel() if kernel is not None else ""
            rec = Record(i, getattr(op, "name", ""), type(op).__name__, kern)

            def fail(condition, detail, rec=rec, op=op, i=i, kern=kern):
                err = OpParityError(i, op, kern, condition, detail)
                if stop:
                    raise err
                rec.failures.append(err)
            ref = reference(shadow)
            for k, v in views.items():
                if k == "rowstat":
                    got, wantst = v.to(F64).sum(0), rowstat_reference(op.C)
                    e = float(((got - wantst).abs() / (wantst.abs() + 1.0)).max()) if bool(torch.isfinite(v).all()) else math.inf
                    rec.worst = max(rec.worst, e / T.ROWSTAT_BOUND)
                    if not e < T.ROWSTAT_BOUND:
                        fail("values", f"rowstat: sum of the parts vs the stored C: {e:.3e} >= {T.ROWSTAT_BOUND}")
                elif isinstance(op, O.GroupStats):
                    _judge_group_stats(op, shadow, v, rec, fail)
                else:
                    if k not in ref:
                        raise NotImplementedError(f"op_parity: {type(op).__name__}.{k} has no reference")
                    _judge_values(op, shadow, k, v, ref[k], rec, plan, fail, aux=ref)
            if isinstance(op, LATENT_OPS):
                _judge_xin_bits(op, ref, fail)
            for key, (v, before, mask) in stor.items():
                moved = (_storage_bytes(v) != before) & ~mask
                if bool(moved.any()):
                    at = int(moved.nonzero()[0])
                    fail("borders", f"byte {at} of a {before.numel()}-byte storage, outside the output view, was changed ({int(moved.sum())} bytes in all)")
            for v, before in slack:
                if not bool(((_bits(v) == _bits(before)) | (v == 0)).all()):
                    fail("borders", "the columns between N and roundup4(N) may be zero-filled, nothing else")
            for k, live, snap in checked_inputs:
                if not torch.equal(_bits(live), _bits(snap)):
                    fail("inputs", f"operand {k} was modified")
            records.append(rec)
            del shadow, views, stor, ref, checked_inputs
    assert len(records) == asked, f"op_parity: judged {len(records)} ops, asked for {asked}"
    return records


def summary(records):
    """What a case writes to the parity log: op count, worst err / tol and worst rel L2 with their ops, the kernel tags seen."""
    if not records:
        return dict(ops=0)
    w = max(records, key=lambda r: r.worst)
    r = max(records, key=lambda r: r.rel_l2)
    return dict(ops=len(records), worst_err_over_tol=w.worst, worst_op=f"[{w.index}] {w.name}", worst_rel_l2=r.rel_l2, worst_rel_l2_op=f"[{r.index}] {r.name}",
                kernels=sorted({x.kernel for x in records if x.kernel}), emulation_rule=sorted({x.name for x in records if x.rule != "close"}))
