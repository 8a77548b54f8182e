"""Value-domain test data: input generators, fp64 references, derived error bounds and fp32 emulations of the kernels' rounding points.

Pure torch on the CPU (no GPU import): tests/test_values_cpu.py proves the generators' stated conditions and that the bounds are neither
impossibly tight (an honest fp32 emulation stays under them) nor toothless (a deliberately wrong emulation exceeds them);
tests/test_values_gpu.py feeds the same data to the HIP kernels.

Every reference is fp64 on the 16-bit-ROUNDED inputs.  No limit in this file comes from what a kernel measured:

    u32 = 2^-24, u16 = 2^-8 (bf16) / 2^-11 (fp16), sub16 = 2^-25 (fp16: half the subnormal spacing, where |ref| < 2^-14) / 0 (bf16)

GEMM / conv (B_gemm):  |out - ref| <= u16 |ref| + sub16 + (1 + u16) (K + 3) u32 S,   S = |A| |W|^T + |bias| + |temb| + |R|
    (K + 3) u32 S is the textbook forward error of a length-K fp32 dot product plus three fp32 additions in ANY summation order (Higham,
    Accuracy and Stability of Numerical Algorithms, section 3.1: gamma_n <= n u / (1 - n u)), so split-K slabs are included; the store rounds
    the fp32 value once (u16, or the subnormal spacing), which also scales the fp32 error by at most (1 + u16).

Attention (B_attn), p = the fp64 softmax row:
    |O - ref| <= u16 |ref| + (2 u16 + 2 ds + 2^-20) sum_j p_j |v_j|  (+ 2^-24 sum_j |v_j| in the fp16 build)
    P is rounded to 16 bits before PV (one u16) and the row sum is taken from 16-bit probabilities too (one u16); ds = (d + 2) u32 scale
    max_j sum_i |q_i k_ji| is the fp32 error of a score, i.e. a relative error of e^s, in the numerator and in the denominator; 2^-20 covers
    v_exp_f32; probabilities below 2^-14 are subnormal in fp16 and carry an absolute error of up to 2^-25 relative to a row sum >= 1/2
    (the subtracted maximum is at most one 16-bit grid step above the true one).  The store rounds once (u16 |ref|).
"""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
FP16 = torch.float16
U32 = 2.0 ** -24
LOG2E = 1.4426950408889634
TILE = 64                 # keys per kv tile of every attention kernel
DEFER = 4.0               # attention2.hip: A2_DEFER, log2 units
ERF_ERR = 2.7e-5          # csrc/common.h: |erf_poly_f - erf| <= 2.7e-5


def u16(dtype):
    return 2.0 ** -8 if dtype == BF16 else 2.0 ** -11


def sub16(dtype):
    return 2.0 ** -25 if dtype == FP16 else 0.0


def sub_term(ref, dtype):
    """Half the subnormal spacing of the storage type where |ref| is below its smallest normal: 2^-25 below 2^-14 in fp16 (sub16).  bf16 has
    fp32's exponent range, so for every ordinary input its term is zero (sub16 = 0); only the exhaustive sweeps reach its subnormals
    (|ref| < 2^-126, spacing 2^-133), where no store can do better than half a step."""
    if dtype == FP16:
        return torch.where(ref.abs() < 2.0 ** -14, torch.full_like(ref, sub16(dtype)), torch.zeros_like(ref))
    return torch.where(ref.abs() < 2.0 ** -126, torch.full_like(ref, 2.0 ** -134), torch.zeros_like(ref))


def kind_of(dtype):
    return "bf16" if dtype == BF16 else "f16"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=gen(seed)) * scale


def ratio(out, ref, bound):
    """worst |out - ref| / bound over the tensor (fp64); a zero bound demands an exact result; a non-finite `out` is infinitely wrong."""
    out = out.detach().to("cpu", F64); ref = ref.to(F64); bound = bound.to(F64)
    err = (out - ref).abs()
    err = torch.where(torch.isfinite(out), err, torch.full_like(err, math.inf))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    return float(r.max()) if r.numel() else 0.0


# --------------------------------------------------------------------------------------------------------------------------------------
# G: GEMM / conv
# --------------------------------------------------------------------------------------------------------------------------------------
def B_gemm(ref, S, K, dtype):
    """The GEMM / conv bound of the module docstring (ref, S fp64)."""
    ref = ref.to(F64)
    return u16(dtype) * ref.abs() + sub_term(ref, dtype) + (1 + u16(dtype)) * (K + 3) * U32 * S.to(F64)


def B_gemm_residual(ref, S, x1, K, dtype):
    """The bound of a GEMM whose epilogue adds the residual to the STAGED 16-bit tile — the arithmetic of every main loop's coalesced epilogue
    (gemm_params.h: add2bf; gemm_ws.hip, gemm_xl.hip, gemm_xd.hip likewise) and of the 16-bit reference network, which stores linear(x) before
    it adds the residual:  out = round16(round16(acc + bias) + R).  x1 = the exact A W^T + bias.  Two roundings instead of the one B_gemm allows:
        |out - ref| <= u16 |ref| + sub(ref) + (1 + u16) (u16 |x1| + sub(x1)) + (1 + u16)^2 (K + 3) u32 S
    the first store contributes u16 |x1| (or half a subnormal step), which the second store scales by at most (1 + u16); the fp32 errors
    (dot product, bias, the one fp32 addition of R) pass through both.  Where R cancels x1 this is far above u16 |ref|: the price of that
    epilogue, stated instead of hidden.  The split-K reduction adds R in fp32 and is held to B_gemm."""
    ref = ref.to(F64); x1 = x1.to(F64)
    u = u16(dtype)
    return u * ref.abs() + sub_term(ref, dtype) + (1 + u) * (u * x1.abs() + sub_term(x1, dtype)) + (1 + u) ** 2 * (K + 3) * U32 * S.to(F64)


G_PATTERNS = ("G1", "G2", "G3", "G4")
G3_HOT = 4.0              # the last row of A in G3 is this many times the row that holds max |ref|


def _pow2_into(x, lo):
    """The power of two s with s * x in [lo, 2 lo)."""
    return 2.0 ** (math.floor(math.log2(lo)) - math.floor(math.log2(x)))


def gemm_inputs(pattern, M, N, K, dtype, seed=0):
    """dict(A [M,K], W [N,K] in the storage type, bias fp32 [N], R [M,N] in the storage type) on the CPU.
    G1: three of the K columns of A are x300 (one in the first, one in a middle and one in the LAST k-slab of 8).
    G2: A[:, K/2:] = -A[:, :K/2] + 2^-6 N(0,1), W[:, K/2:] = W[:, :K/2]: the product cancels to ~1 % of S = |A||W|^T (side operands 2^-6 N(0,1)).
    G3 (fp16): A times the power of two that puts max |A W^T| over rows 0..M-2 into [2^14, 2^15); row M-1 = G3_HOT x the row holding that
        maximum, so part of it overflows fp16.  W is N(0,1) / 4 (not K^-1/2) so that the hot row of A itself stays far below 65504.
    G4: A and W each x 2^-12 (side operands x 2^-24): operands and results in the fp16 subnormal range."""
    A = randn(M, K, seed=seed + 1); W = randn(N, K, seed=seed + 2, scale=K ** -0.5)
    bias = randn(N, seed=seed + 3); R = randn(M, N, seed=seed + 4)
    if pattern == "G1":
        A[:, [5, K // 2 + 1, K - 2]] *= 300.0
    elif pattern == "G2":
        h = K // 2
        A[:, h:2 * h] = -A[:, :h] + randn(M, h, seed=seed + 5, scale=2.0 ** -6)
        W[:, h:2 * h] = W[:, :h]
        bias *= 2.0 ** -6; R *= 2.0 ** -6
    elif pattern == "G3":
        assert dtype == FP16, "G3 is the fp16 range pattern"
        W = randn(N, K, seed=seed + 2, scale=0.25)
        A16, W16 = A.to(dtype), W.to(dtype)
        ref0 = (A16[:M - 1].double() @ W16.double().T).abs()
        s = _pow2_into(float(ref0.max()), 2.0 ** 14)
        r_star = int(ref0.max(1).values.argmax())
        A = A16.float() * s                                    # exact: a power of two, far from overflow and from the subnormals
        A[M - 1] = G3_HOT * A[r_star]
        assert float(A.abs().max()) < 32768.0
        bias = bias * s * 0.25; R = R * s * 0.25
        W = W16.float()
    elif pattern == "G4":
        A *= 2.0 ** -12; W *= 2.0 ** -12; bias *= 2.0 ** -24; R *= 2.0 ** -24
    else:
        raise ValueError(pattern)
    return dict(A=A.to(dtype), W=W.to(dtype), bias=bias.float(), R=R.to(dtype))


def gemm_ref(d, use_bias=False, use_R=False):
    """(ref, S) in fp64: A W^T (+ bias + R) and the same contraction on absolute values."""
    A, W = d["A"].double(), d["W"].double()
    ref = A @ W.T; S = A.abs() @ W.abs().T
    if use_bias:
        ref = ref + d["bias"].double(); S = S + d["bias"].double().abs()
    if use_R:
        ref = ref + d["R"].double(); S = S + d["R"].double().abs()
    return ref, S


def conv_inputs(pattern, B, H, Wd, Cin, Cout, dtype, seed=0):
    """dict(x [B,H,W,Cin], w [Cout,3,3,Cin]) in the storage type: the G patterns along the input-channel axis (the contraction is over
    (tap, channel): G1 scales three channels, G2 mirrors the channel halves).  G3: scaled as for the GEMM (maximum over the output rows
    0..H-4, which see no hot input); the LAST TWO image rows are
    G3_HOT times larger, so the last output row (whose 3x3 window sees only those rows and the zero pad) partly overflows fp16."""
    x = randn(B, H, Wd, Cin, seed=seed + 1); w = randn(Cout, 3, 3, Cin, seed=seed + 2, scale=(9 * Cin) ** -0.5)
    if pattern == "G1":
        x[..., [5, Cin // 2 + 1, Cin - 2]] *= 300.0
    elif pattern == "G2":
        h = Cin // 2
        x[..., h:] = -x[..., :h] + randn(B, H, Wd, h, seed=seed + 5, scale=2.0 ** -6)
        w[..., h:] = w[..., :h]
    elif pattern == "G3":
        assert dtype == FP16
        w = randn(Cout, 3, 3, Cin, seed=seed + 2, scale=0.25)
        x16, w16 = x.to(dtype), w.to(dtype)
        ref0 = conv_ref(dict(x=x16, w=w16))[0][:, :H - 3].abs()            # the output rows that see no hot input row
        s = _pow2_into(float(ref0.max()), 2.0 ** 14)
        x = x16.float() * s
        x[:, H - 2:] *= G3_HOT
        assert float(x.abs().max()) < 32768.0
        w = w16.float()
    elif pattern == "G4":
        x *= 2.0 ** -12; w *= 2.0 ** -12
    else:
        raise ValueError(pattern)
    return dict(x=x.to(dtype), w=w.to(dtype))


def conv_ref(d):
    """(ref, S) [B,H,W,Cout] in fp64 for the 3x3 / stride 1 / pad 1 conv; K = 9 Cin."""
    x = d["x"].double().permute(0, 3, 1, 2); w = d["w"].double().permute(0, 3, 1, 2)
    return F.conv2d(x, w, padding=1).permute(0, 2, 3, 1), F.conv2d(x.abs(), w.abs(), padding=1).permute(0, 2, 3, 1)


def g3_check(out, ref, bound, hot, dtype, x1=None):
    """The G3 assertions as numbers: (worst err / bound over the elements that cannot overflow, #inf mismatches among the hot elements,
    excluded share of the hot elements).  `hot`: bool mask of the hot row(s).  An element cannot overflow when |ref| + bound < 65504; on the hot
    elements isinf(out) must equal isinf(ref.to(fp16)) with the same sign, except where |ref| is within 2 u16 (relative) of the fp16 overflow
    threshold 65520 — there the fp32 sum may legitimately land on either side; hot elements that do not overflow obey the bound as well.
    x1 (the staged-residual epilogue, B_gemm_residual): the first store overflows on its own when |x1| reaches the threshold, so an element is
    safe only if x1 cannot overflow either, and hot elements whose x1 may overflow while ref clearly does not join the excluded share."""
    out = out.detach().to("cpu"); ref = ref.to(F64)
    safe = (ref.abs() + bound) < 65504.0
    band = 2 * u16(dtype) * 65520.0
    stage = torch.zeros_like(safe)
    if x1 is not None:
        safe &= (x1.abs() + bound) < 65504.0
        stage = (x1.abs() >= 65520.0 - band) & (ref.abs() < 65520.0 - band)
    r_safe = ratio(out.double()[safe], ref[safe], bound[safe])
    want = ref.to(FP16)
    excl = hot & (((ref.abs() - 65520.0).abs() <= band) | stage)
    chk = hot & ~excl
    o16 = out.to(FP16)
    mism = int(((torch.isinf(o16) != torch.isinf(want)) | (torch.isinf(want) & (o16 != want)))[chk].sum())
    nan = int(torch.isnan(o16).sum())
    return r_safe, mism + nan, float(excl.sum()) / max(1, int(hot.sum()))


def emu_gemm(d, dtype, use_bias=False, use_R=False, drop_last=0, rtz=False, staged=False, flush=False, three_roundings=False):
    """fp32 emulation: fp32 products and sums, one rounding to the storage type; staged: the residual is added to the stored 16-bit value and
    the sum is rounded again (B_gemm_residual).  WRONG kernels: drop_last skips the last k-slab; flush treats subnormal 16-bit operands as
    zero; three_roundings also rounds the product before the bias is added."""
    A, W = d["A"].float(), d["W"].float()
    if flush:
        tiny = float(torch.finfo(dtype).tiny)
        A = torch.where(A.abs() < tiny, torch.zeros_like(A), A); W = torch.where(W.abs() < tiny, torch.zeros_like(W), W)
    K = A.shape[1] - drop_last
    acc = A[:, :K] @ W[:, :K].T
    if three_roundings: acc = acc.to(dtype).float()
    if use_bias: acc = acc + d["bias"]
    if use_R: acc = (acc.to(dtype).float() if staged else acc) + d["R"].float()
    return round_toward_zero(acc, dtype) if rtz else acc.to(dtype)


def round_toward_zero(x32, dtype):
    """fp32 -> 16-bit by truncation (the WRONG store): the nearest-even result stepped one ulp toward zero wherever it overshot."""
    y = x32.to(dtype)
    over = (y.float().abs() > x32.abs()) & torch.isfinite(x32)
    bits = y.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(dtype)      # sign-magnitude: one step down in magnitude


# --------------------------------------------------------------------------------------------------------------------------------------
# E: exhaustive 16-bit sweeps
# --------------------------------------------------------------------------------------------------------------------------------------
def all_bits(dtype):
    """Every bit pattern of the storage type, in pattern order [65536]."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


def finite_bits(dtype):
    x = all_bits(dtype)
    return x[torch.isfinite(x.float())]


def sweep_perm():
    """The fixed permutation EW_ADD adds the set to itself through."""
    return torch.randperm(65536, generator=gen(7))


def ulp16(x, dtype):
    """Spacing of the storage type at |x| (fp64 in, fp64 out), the subnormal spacing below the smallest normal."""
    mant, emin = (7, -126) if dtype == BF16 else (10, -14)
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** (emin - 1)))).clamp_min(emin)
    return torch.pow(torch.full_like(e, 2.0), e - mant)


def sweep_ref(op, x, dtype, y0=None, alpha=0.37):
    """(fp64 result, the fp32 CPU torch result of the same op) of one sweep operation on 16-bit inputs."""
    xd, xf = x.double(), x.float()
    if op == "SILU":
        return xd * torch.sigmoid(xd), F.silu(xf)
    if op == "SCALE":
        return xd * float(torch.tensor(alpha, dtype=F32)), xf * alpha
    if op == "ADD":
        return y0.double() + xd, y0.float() + xf
    return xd, xf


FP32_FLOOR = 2.0 ** -119  # see sweep_check


def sweep_check(out, ref64, ref32, dtype, floor=0.0):
    """(#elements violating the sweep contract, worst |out - round16(ref64)| in 16-bit ulps over the finite ones).  Contract: NaN exactly where
    the fp32 torch op gives NaN; +-inf where that result, rounded to the type, is +-inf (same sign); every other result finite and within one
    16-bit ulp of the fp64 result rounded to the type (fp32 evaluation error << half a 16-bit ulp: only the two neighbours are possible).
    floor (SiLU only: pass FP32_FLOOR): one corner of bf16 is outside what ANY fp32 evaluation of x / (1 + e^-x) can give, the fp32 torch op included: for -x > 126 ln 2 = 87.3
    the reciprocal of 1 + e^-x is an fp32 denormal (and e^-x overflows at 88.7), while x sigmoid(x) is still a normal bf16 number of
    magnitude < 88 * 2^-126 < 2^-119.  For the SiLU sweeps an absolute error of up to FP32_FLOOR = 2^-119 is therefore accepted beside the
    one-ulp rule; every other operation is exact or one multiplication / addition in fp32 and gets no floor."""
    out = out.detach().to("cpu")
    t16 = ref32.to(dtype)
    nan_bad = torch.isnan(out) != torch.isnan(t16)
    inf_bad = (torch.isinf(out) != torch.isinf(t16)) | (torch.isinf(t16) & (out != t16))
    fin = torch.isfinite(t16) & torch.isfinite(out)
    want = ref64.to(dtype).double()
    d = (out.double() - want).abs() / ulp16(want, dtype)
    d = torch.where(fin & ((out.double() - want).abs() > floor), d, torch.zeros_like(d))
    return int((nan_bad | inf_bad | (d > 1.0)).sum()), float(d.max())


def copy_set(dtype):
    """fp32 inputs of the fp32 -> 16-bit copy: every 16-bit value, its two fp32 neighbours, the exact midpoints between adjacent 16-bit values
    (ties to even; in fp16 also the midpoint 65520 above the largest finite value and the subnormals), a few values far beyond the range."""
    v = finite_bits(dtype).float()
    v = torch.unique(v)                                               # sorted, -0 == +0 merged
    mids = ((v[:-1].double() + v[1:].double()) / 2).float()           # exact in fp32: one more mantissa bit
    top = float(v[-1]); step = float(v[-1] - v[-2])
    beyond = torch.tensor([top + step / 2, -(top + step / 2)], dtype=F64).float()       # the tie that overflows (finite in fp32 for both types)
    base = torch.cat([v, mids, beyond, torch.tensor([-0.0])])
    up = torch.nextafter(base, torch.full_like(base, math.inf)); dn = torch.nextafter(base, torch.full_like(base, -math.inf))
    extra = torch.tensor([math.inf, -math.inf, math.nan, 1e10, -1e10, 3.0e38, -3.0e38, 1e-45, -1e-45], dtype=F32)
    x = torch.cat([base, up, dn, extra])
    pad = (-x.numel()) % 8
    return torch.cat([x, torch.zeros(pad)])


def same_bits_or_nan(a, b):
    """Bit-exact, NaN compared as NaN-ness (not the payload): number of differing elements."""
    a = a.detach().to("cpu"); b = b.detach().to("cpu")
    both_nan = torch.isnan(a) & torch.isnan(b)
    return int(((a.view(torch.int16) != b.view(torch.int16)) & ~both_nan).sum())


GEGLU_H = (1.0, -3.0, 0.01)


def geglu_inputs(dtype, K):
    """Two-hot A [3 n, K] (A[m][0] = h_m, A[m][1] = g_m: g every finite pattern, h each of GEGLU_H) and the unpacked W [2 F, K], F = 64:
    column 0 feeds every value slot, column 1 every gate slot.  Returns (A, W fp32, h, g) — pack W with packing.pack_geglu."""
    g = finite_bits(dtype)
    n = g.numel()
    h = torch.tensor(GEGLU_H).to(dtype).repeat_interleave(n)
    g = g.repeat(len(GEGLU_H))
    A = torch.zeros(g.numel(), K, dtype=dtype)
    A[:, 0] = h; A[:, 1] = g
    Fh = 64
    W = torch.zeros(2 * Fh, K)
    W[:Fh, 0] = 1.0; W[Fh:, 1] = 1.0
    return A, W, h, g


def geglu_ref(h, g, dtype):
    """(ref fp64 [M], bound [M]): h gelu(g) with the exact erf; bound = u16 |ref| + sub16 + 1.35e-5 |h g| (|erf error| <= 2.7e-5 enters as
    0.5 h g (erf~ - erf)); where the fp64 result overflows the type the bound is infinite and the caller compares the infinity instead."""
    hd, gd = h.double(), g.double()
    ref = hd * 0.5 * gd * (1.0 + torch.erf(gd * 0.7071067811865476))
    return ref, u16(dtype) * ref.abs() + sub_term(ref, dtype) + 0.5 * ERF_ERR * (hd * gd).abs()


def geglu_check(out_col, ref, bound, dtype):
    """(worst err / bound over the elements that cannot overflow, number of elements that must overflow and are not the reference's infinity).
    The store overflows when the fp32 value reaches thr = the largest finite value plus half a step (65520 in fp16).  That value is within
    1.35e-5 + a few u32 (relative) of ref, far inside the 2 u16 band that G3 excludes around the threshold: below thr (1 - 2 u16) the
    result must be finite and within the bound, above thr (1 + 2 u16) it must be the infinity of ref's sign; only the band is left open."""
    out_col = out_col.detach().to("cpu")
    thr = float(torch.finfo(dtype).max) * (1.0 + u16(dtype) / 2) if dtype == BF16 else 65520.0
    fin = ref.abs() < thr * (1 - 2 * u16(dtype))
    r = ratio(out_col.double()[fin], ref[fin], bound[fin])
    ovf = ref.abs() > thr * (1 + 2 * u16(dtype))
    bad = int((out_col.float()[ovf] != torch.sign(ref[ovf]).float() * math.inf).sum())
    return r, bad


_ERF_C = (4.074397617e-08, -1.944883433e-06, 4.106127751e-05, -5.110412727e-04, 4.235439367e-03, -2.510287440e-02, 1.110793533e-01,
          -3.753149504e-01, 1.128268531e+00)


def emu_geglu(h, g, dtype, clamp=3.0):
    """fp32 emulation of the epilogue: the degree-8 erf polynomial of csrc/common.h in Horner form, clamped at |z| = clamp (2.0: the WRONG one)."""
    hf, gf = h.float(), g.float()
    z = (gf * 0.70710678118654752440).clamp(-clamp, clamp)
    u = z * z
    p = torch.full_like(u, _ERF_C[0])
    for c in _ERF_C[1:]:
        p = p * u + c
    hx = 0.5 * gf
    return (hf * (hx * (z * p) + hx)).to(dtype)


# --------------------------------------------------------------------------------------------------------------------------------------
# N: norms
# --------------------------------------------------------------------------------------------------------------------------------------
N_PATTERNS = ("zero_group", "channel_means", "common_mean", "hot_pixel")


def mean_levels(dtype):
    return (0.0, 8.0, 64.0) if dtype == BF16 else (0.0, 64.0, 1000.0)


def gn_inputs(pattern, B, HW, C, G, dtype, seed=0):
    """x [B,HW,C] in the storage type, gamma, beta fp32 [C].
    zero_group: group 3 of every image is all zero (a zero-initialised conv) beside ordinary groups;
    channel_means: channel c has mean +-level[c % 3] (sign by c % 2) and unit spread;
    common_mean: every element is level[2] + N(0,1) — the whole group far from zero, |mean| / sigma = 64 (bf16) or 1000 (fp16);
    hot_pixel: one pixel of group 5 in image 0 is x1000."""
    x = randn(B, HW, C, seed=seed + 1)
    cpg = C // G
    if pattern == "zero_group":
        x[:, :, 3 * cpg:4 * cpg] = 0.0
    elif pattern == "channel_means":
        lv = torch.tensor(mean_levels(dtype))
        c = torch.arange(C)
        x = x + lv[c % 3] * (1.0 - 2.0 * (c % 2))
    elif pattern == "common_mean":
        x = x + mean_levels(dtype)[2]
    elif pattern == "hot_pixel":
        x[0, HW // 3, 5 * cpg:6 * cpg] *= 1000.0
    else:
        raise ValueError(pattern)
    return x.to(dtype), 1.0 + randn(C, seed=seed + 2, scale=0.3), randn(C, seed=seed + 3, scale=0.3)


def gn_ref(x, G, gamma, beta, eps, silu):
    y = F.group_norm(x.double().transpose(1, 2), G, gamma.double(), beta.double(), eps).transpose(1, 2)
    return F.silu(y) if silu else y


def emu_gn(x, G, gamma, beta, eps, silu, naive=False):
    """fp32 emulation: two-pass statistics (what pivot-shifted / Chan-combined sums are equivalent to), or — naive, the WRONG one —
    E[x^2] - E[x]^2 from raw fp32 sums."""
    B, HW, C = x.shape
    xf = x.float().reshape(B, HW, G, C // G)
    if naive:
        mean = xf.mean((1, 3), keepdim=True); var = (xf * xf).mean((1, 3), keepdim=True) - mean * mean
    else:
        mean = xf.mean((1, 3), keepdim=True); var = ((xf - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((xf - mean) * torch.rsqrt(var.clamp_min(0) + eps)).reshape(B, HW, C) * gamma + beta
    return (F.silu(y) if silu else y).to(x.dtype)


def ln_inputs(pattern, M, C, dtype, seed=0):
    """x [M,C]: the norm patterns per ROW — rows 3, 4 all zero; row r offset by +-level[r % 3]; one element of row 5 x1000."""
    x = randn(M, C, seed=seed + 1)
    if pattern == "zero_group":
        x[3:5] = 0.0
    elif pattern == "channel_means":
        lv = torch.tensor(mean_levels(dtype))
        r = torch.arange(M)
        x = x + (lv[r % 3] * (1.0 - 2.0 * (r % 2)))[:, None]
    elif pattern == "common_mean":
        x = x + mean_levels(dtype)[2]
    elif pattern == "hot_pixel":
        x[5, C // 3] *= 1000.0
    else:
        raise ValueError(pattern)
    return x.to(dtype), 1.0 + randn(C, seed=seed + 2, scale=0.3), randn(C, seed=seed + 3, scale=0.3)


LN_OFFSET_LIMITS = dict(fused=2e-2, scratch=1e-2, drift=2e-2)     # tests/test_kernels_gpu.py::test_gemm_fused_layernorm_large_common_offset_routes_agree


def ln_offset_inputs(M, K, N, dtype, seed=0):
    """x = 1000 + 10 N(0,1) [M,K] in the storage type; the LayerNorm affine folded into W' (16-bit), b' = W beta, csum = row sums of W'."""
    x = (randn(M, K, seed=seed + 1, scale=10.0) + 1000.0).to(dtype)
    W = randn(N, K, seed=seed + 2, scale=K ** -0.5)
    gamma = 1.0 + randn(K, seed=seed + 5, scale=0.3); beta = randn(K, seed=seed + 6, scale=0.3)
    Wp = (W * gamma[None, :]).to(dtype)
    return dict(x=x, Wp=Wp, b=(W @ beta).float(), csum=Wp.float().sum(1), W=W, gamma=gamma, beta=beta)


def ln_lin_ref(x, Wp, b, eps=1e-5, stored=None):
    """fp64 LayerNorm -> Linear on the same W'; stored: the 16-bit type a route keeps the normalised rows in (ln_scratch)."""
    xd = x.double()
    xh = (xd - xd.mean(-1, keepdim=True)) * (xd.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    if stored is not None:
        xh = xh.to(stored).double()
    return xh @ Wp.double().T + b.double()


def emu_ln_fused(x, Wp, b, csum, dtype, eps=1e-5):
    """fp32 emulation of the fused route: one-pass fp32 sums, rstd (acc - mean csum) + bias, one rounding."""
    xf = x.float()
    K = xf.shape[1]
    mean = xf.sum(1, keepdim=True) / K
    var = (xf * xf).sum(1, keepdim=True) / K - mean * mean
    rstd = torch.rsqrt(var.clamp_min(0) + eps)
    return (rstd * (xf @ Wp.float().T - mean * csum[None, :]) + b).to(dtype)


def rel_l2(a, b):
    a = a.detach().to("cpu", F64); b = b.detach().to("cpu", F64)
    return float((a - b).norm() / (b.norm() + 1e-300))


# --------------------------------------------------------------------------------------------------------------------------------------
# A: attention
# --------------------------------------------------------------------------------------------------------------------------------------
A_PATTERNS = ("A1", "A2_3.9", "A2_4.1", "A2_12", "A2_3.9_desc", "A2_4.1_desc", "A2_12_desc", "A3", "A4", "A5")
A1_MARGIN = 40.0          # nats


def attn_inputs(pattern, B, H, Tq, Tk, d, dtype, seed=0, Bkv=None, live=None):
    """q [B,Tq,H d], k, v [Bkv,Tk,H d] in the storage type (Bkv = B unless given), the same construction in every head.
    A1 block one-hot: Q_t = c e_a(t) + 0.05 N, K_j = c e_b(j) + 0.05 N, a(t) = floor(t d / Tq), b(j) = floor(j d / Tk), scale c^2 = 48 nats;
    A2 staircase: key j = (64 floor(j / 64), j % 64, 0.05 N ...) — both coordinates exact small integers in either type — and every query =
       (g, g, 0.05 N ...) with scale g = step ln 2 / 64: the logit rises by `step` log2 units per tile of 64 keys; "_desc": keys reversed;
    A3 common shift: Q_t = (+-c, 1.2 N ...), K_j = (c, 1.2 N ...) with scale c^2 = 250: every logit of a row is +250 (even t) or -250 (odd t) +- ~3 nats;
    A4 V outliers: N(0,1) Q, K; channel 3 of every head of V x1000, 1 % of the keys with their whole V row x100 (x1000 where both apply);
    A5 flat: all K rows equal — O is the mean of V.
    live: the number of keys the kernel attends to when Tk is a capacity (the patterns are laid out over the live keys; the dead ones
    repeat the last class / continue the staircase, so a kernel that read them would show)."""
    Bkv = B if Bkv is None else Bkv
    n = Tk if live is None else live
    scale = d ** -0.5
    q = randn(B, Tq, H, d, seed=seed + 1); k = randn(Bkv, Tk, H, d, seed=seed + 2); v = randn(Bkv, Tk, H, d, seed=seed + 3)
    if pattern == "A1":
        c = math.sqrt(48.0 / scale)
        a = (torch.arange(Tq) * d) // Tq; b = ((torch.arange(Tk) * d) // n).clamp_max(d - 1)
        q = 0.05 * q + c * F.one_hot(a, d)[None, :, None, :]
        k = 0.05 * k + c * F.one_hot(b, d)[None, :, None, :]
    elif pattern.startswith("A2"):
        step = float(pattern.split("_")[1])
        g = step * math.log(2.0) / (TILE * scale)
        j = torch.arange(Tk)
        if pattern.endswith("desc"):
            j = (n - 1 - j).abs()
        q = 0.05 * q; k = 0.05 * k
        q[..., 0] = g; q[..., 1] = g
        k[..., 0] = ((j // TILE) * TILE).float()[None, :, None]; k[..., 1] = (j % TILE).float()[None, :, None]
    elif pattern == "A3":
        c = math.sqrt(250.0 / scale)
        q = 1.2 * q; k = 1.2 * k
        q[..., 0] = (c * (1.0 - 2.0 * (torch.arange(Tq) % 2)))[None, :, None]
        k[..., 0] = c
    elif pattern == "A4":
        hot = torch.rand(Tk, generator=gen(seed + 4)) < 0.01
        hot[Tk // 2] = True
        v[:, hot] *= 100.0
        v[..., 3] = torch.where(hot[None, :, None], v[..., 3] * 10.0, v[..., 3] * 1000.0)
    elif pattern == "A5":
        k = k[:, :1].expand(Bkv, Tk, H, d).clone()
    else:
        raise ValueError(pattern)
    return q.reshape(B, Tq, H * d).to(dtype), k.reshape(Bkv, Tk, H * d).to(dtype), v.reshape(Bkv, Tk, H * d).to(dtype)


def prescale(q, d):
    """(Q' for the kernel, Q for the reference): Q' = round16(Q scale log2 e), the reference gets Q' / (scale log2 e) in fp64."""
    f = d ** -0.5 * LOG2E
    qp = (q.float() * f).to(q.dtype)
    return qp, qp.double() / f


def _heads(x, H):
    B, T, C = x.shape
    return x.double().reshape(B, T, H, C // H).transpose(1, 2)         # [B,H,T,d]


def attn_logits(q, k, H, scale, causal=False, count=None):
    """fp64 logits [B,H,Tq,Tk] in nats with masked entries at -inf, and |q| |k|^T scale (the magnitude sum of every score)."""
    qh, kh = _heads(q, H), _heads(k, H)
    s = qh @ kh.transpose(-1, -2) * scale
    mag = qh.abs() @ kh.abs().transpose(-1, -2) * scale
    Tq, Tk = s.shape[-2:]
    mask = torch.zeros(Tq, Tk, dtype=torch.bool)
    if causal:
        mask |= torch.arange(Tk)[None, :] > torch.arange(Tq)[:, None]
    if count is not None:
        mask |= (torch.arange(Tk) >= count)[None, :]
    return s.masked_fill(mask, -math.inf), mag.masked_fill(mask, 0.0)


def attn_ref(q, k, v, H, scale, dtype, causal=False, count=None):
    """(ref, bound) [B,Tq,H d] fp64 for ONE kv source: B_attn of the module docstring WITHOUT the store term u16 |ref| (attn_bound adds it once
    after the sources are summed).  q may already be fp64 (the pre-scaled reference)."""
    d = q.shape[2] // H
    s, mag = attn_logits(q, k, H, scale, causal, count)
    p = torch.softmax(s, -1)
    vh = _heads(v, H)
    ref = p @ vh
    spv = p @ vh.abs()
    ds = (d + 2) * U32 * mag.max(-1, keepdim=True).values
    bound = (2 * u16(dtype) + 2 * ds + 2.0 ** -20) * spv
    if dtype == FP16:
        live = torch.isfinite(s).double()                          # [B,H,Tq,Tk]: the keys this query sees
        bound = bound + 2.0 ** -24 * (live @ vh.abs())
    back = lambda t: t.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)
    return back(ref), back(bound)


def attn_bound(ref, inner, dtype):
    return u16(dtype) * ref.abs() + inner


def attn_ref_sources(q, k, v, H, scale, dtype, srcs, joint):
    """Several kv sources per query batch: srcs(i) -> the kv batch indices of query batch i.  joint: ONE softmax over the concatenated
    sources; else the sum of the per-source attentions (every term carries its own error, the sum is stored once)."""
    refs, inners = [], []
    for i in range(q.shape[0]):
        js = srcs(i)
        if joint:
            r, b = attn_ref(q[i:i + 1], torch.cat([k[j] for j in js])[None], torch.cat([v[j] for j in js])[None], H, scale, dtype)
        else:
            parts = [attn_ref(q[i:i + 1], k[j:j + 1], v[j:j + 1], H, scale, dtype) for j in js]
            r = sum(p_[0] for p_ in parts); b = sum(p_[1] for p_ in parts)
            b = b + len(js) * U32 * sum(p_[0].abs() for p_ in parts)            # the fp32 additions of the partial outputs
        refs.append(r); inners.append(b)
    return torch.cat(refs), torch.cat(inners)


def a1_margin(q, k, H, scale, causal=False, count=None):
    """Smallest (own-class logit - other-class logit) over all queries, nats: own class = the keys with b(j) = a(t)."""
    s, _ = attn_logits(q, k, H, scale, causal, count)
    Tq, Tk = s.shape[-2:]
    d = q.shape[2] // H
    n = Tk if count is None else count
    a = (torch.arange(Tq) * d) // Tq; b = ((torch.arange(Tk) * d) // n).clamp_max(d - 1)
    own = (a[:, None] == b[None, :]) & torch.isfinite(s[0, 0])
    assert own.any(1).all(), "a query without a visible key of its own class"
    lo = s.masked_fill(~own, math.inf).min(-1).values
    hi = s.masked_fill(own, -math.inf).max(-1).values
    return float((lo - hi).min())


def a2_steps(q, k, H, scale):
    """Realised rise of the row maximum between consecutive FULL tiles, log2 units: (min, max) over queries, heads and tile pairs."""
    s, _ = attn_logits(q, k, H, scale)
    nfull = s.shape[-1] // TILE
    assert nfull >= 2, "the staircase condition needs two full tiles"
    tm = s[..., :nfull * TILE].reshape(*s.shape[:-1], nfull, TILE).max(-1).values * LOG2E
    dlt = tm[..., 1:] - tm[..., :-1]
    return float(dlt.min()), float(dlt.max())


def _group_any(over, size=32):
    """any() over groups of `size` consecutive queries (the wave ballot), broadcast back to every query of the group."""
    Tq = over.shape[-1]
    o = F.pad(over, (0, (-Tq) % size)).reshape(*over.shape[:-1], -1, size)
    return o.any(-1, keepdim=True).expand_as(o).reshape(*over.shape[:-1], -1)[..., :Tq]


def emu_attn(q, k, v, H, scale, dtype, pre=False, fold=False, causal=False, count=None, skip_rescale_tile=None, wrong_rebase=False):
    """fp32 emulation of the tile loop with the kernels' rounding points: fp32 scores, the online softmax written out tile by tile with a
    DEFERRED maximum (raised only when a tile exceeds it by more than DEFER log2 units, decided per 32-query group like the wave ballot),
    P rounded to the type before PV, the row sum taken from the rounded P, fp32 accumulators, one rounding on store.
    pre: q is the pre-scaled Q' (scores are base-2 exponents as they come out of the product).
    fold: the FOLD form (needs pre) — the maximum lives on the 16-bit grid and a raise re-bases the tile by delta = m_new - m_old.
    WRONG forms: skip_rescale_tile = t leaves O un-rescaled at tile t; wrong_rebase adds delta instead of subtracting it."""
    assert pre or not fold
    B, Tq, C = q.shape
    d = C // H
    qh = _heads(q, H).float(); kh = _heads(k, H).float(); vh = _heads(v, H).float()
    t = qh @ kh.transpose(-1, -2)
    if not pre:
        t = t * (scale * LOG2E)
    Tk = t.shape[-1]
    n = Tk if count is None else count
    if causal:
        t = t.masked_fill(torch.arange(Tk)[None, :] > torch.arange(Tq)[:, None], -math.inf)
    t = t[..., :n]; vh = vh[:, :, :n]
    m = torch.zeros(B, H, Tq) if fold else torch.full((B, H, Tq), -math.inf)
    l = torch.zeros(B, H, Tq); Oa = torch.zeros(B, H, Tq, d)
    for ti, j0 in enumerate(range(0, n, TILE)):
        x = t[..., j0:j0 + TILE]
        mx = x.max(-1).values
        trig = torch.ones_like(mx, dtype=torch.bool) if ti == 0 else _group_any((mx - m) > DEFER)
        if fold:
            rel = mx - m
            inc = rel if ti == 0 else rel.clamp_min(0)
            m_new = torch.where(trig, (m + inc).to(dtype).float(), m)
            delta = m_new - m
            alpha = torch.zeros_like(m) if ti == 0 else torch.exp2(-delta)
            xr = (x - m[..., None]) + delta[..., None] if (wrong_rebase and ti > 0) else (x - m[..., None]) - delta[..., None]
        else:
            m_new = torch.where(trig, torch.maximum(m, mx), m)
            alpha = torch.where(m_new == -math.inf, torch.ones_like(m), torch.exp2(m - m_new))
            xr = x - torch.where(m_new == -math.inf, torch.zeros_like(m_new), m_new)[..., None]
        if skip_rescale_tile is None or ti != skip_rescale_tile:
            Oa = Oa * alpha[..., None]
        p16 = torch.exp2(xr).to(dtype).float()
        Oa = Oa + p16 @ vh[:, :, j0:j0 + TILE]
        l = l * alpha + p16.sum(-1)
        m = m_new
    out = (Oa / l[..., None]).to(dtype)
    return out.transpose(1, 2).reshape(B, Tq, C)


# --------------------------------------------------------------------------------------------------------------------------------------
# S: Fourier and timestep embeddings
# --------------------------------------------------------------------------------------------------------------------------------------
def fourier_inputs(n=37, P=8, seed=0):
    """fp32 [n,P,3] with |x| up to 2000: the pixel magnitudes of camera intrinsics (focal lengths ~1260, principal points ~800 / 450)."""
    x = (torch.rand(n, P, 3, generator=gen(seed + 1)) * 2.0 - 1.0) * 2000.0
    x[0, 0] = torch.tensor([2000.0, -2000.0, 1266.417])
    x[0, 1] = torch.tensor([0.0, 816.267, 491.507])
    return x.float()


def fourier_ref(x, Fq, dtype):
    """(ref, bound) [n, P (3 + 6 F)] fp64: [x, sin(f0 x), cos(f0 x), ...], f = 2^k; fp64 sin / cos of the fp32 product (exact here: a power of
    two).  bound = u16 |ref| + 2^-21: one store rounding plus an fp32 sin / cos good to a few ulp of 1 (2^-21 = 4 ulp at 1)."""
    xd = x.double()
    parts = [xd]
    for i in range(Fq):
        a = (x * float(2 ** i)).double()
        parts += [torch.sin(a), torch.cos(a)]
    ref = torch.cat(parts, -1).reshape(x.shape[0], -1)
    return ref, u16(dtype) * ref.abs() + 2.0 ** -21


TIMESTEPS = (0.0, 1.0, 999.0, 1000.5)


def timeemb_ref(t, dim=320, max_period=10000.0):
    """fp64 diffusers formula, flip_sin_to_cos, shift 0: [cos(t w_k) | sin(t w_k)], w_k = max_period^(-k / half)."""
    half = dim // 2
    w = torch.exp(-math.log(max_period) * torch.arange(half, dtype=F64) / half)
    e = t.double()[:, None] * w[None]
    return torch.cat([torch.cos(e), torch.sin(e)], -1)


# --------------------------------------------------------------------------------------------------------------------------------------
# the shapes of the GPU cases (the smallest that reach each route), shared with the CPU checks
# --------------------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = dict(tile64=(300, 192, 320), splitk=(168, 640, 2560), ws=(300, 328, 320), xl=(600, 320, 640))
GEMM_SHAPES.update(tile64_res=GEMM_SHAPES["tile64"], splitk_res=GEMM_SHAPES["splitk"], xl_res=GEMM_SHAPES["xl"])      # the same routes with bias + R
STAGED_RESIDUAL = ("ws", "tile64_res", "xl_res")                   # routes whose epilogue adds R to the staged 16-bit tile (B_gemm_residual)
SIDE_OPERANDS = STAGED_RESIDUAL + ("splitk_res",)                  # routes run with bias + R


def gemm_bound(d, route, K, dtype):
    """(ref, bound, x1 or None, single) of a G case on `route`: B_gemm, or B_gemm_residual where the residual meets a staged tile; `single` is
    the one-rounding B_gemm in either case (logged beside the verdict)."""
    side = route in SIDE_OPERANDS
    ref, S = gemm_ref(d, side, side)
    single = B_gemm(ref, S, K, dtype)
    if route not in STAGED_RESIDUAL:
        return ref, single, None, single
    x1 = gemm_ref(d, True, False)[0]
    return ref, B_gemm_residual(ref, S, x1, K, dtype), x1, single
CONV_SHAPE = (1, 12, 20, 64, 64)                                   # B, H, W, Cin, Cout
ATTN_SHAPES = dict(                                                 # B, H, Tq, Tk, d
    generic=(1, 2, 130, 200, 64), attn2=(6, 8, 300, 300, 40), resident=(6, 8, 300, 150, 40), sources=(6, 8, 300, 300, 40),
    short=(2, 2, 77, 77, 64), ctx=(2, 2, 300, 128, 40))
CTX_COUNT = 77
