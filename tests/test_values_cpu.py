"""CPU: the value-domain test data (tests/values_data.py) is what it claims to be.

1. every generator meets its stated condition (A1 margin, A2 step, G2 ratio, G3 range and excluded share);
2. an fp32 torch emulation with the kernels' rounding points stays at err / bound <= 1 for every family, pattern and type — the bounds
   are not impossibly tight;
3. one deliberately wrong emulation per family exceeds its bound or limit — the bounds are not toothless.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import values_data as V
from helpers import close

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]


def small(shape):
    """The route's Tq, Tk, d with one batch and two heads: the patterns are the same in every (batch, head)."""
    B, H, Tq, Tk, d = shape
    return 1, 2, Tq, Tk, d


# ---- 1. generator conditions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("route", list(V.ATTN_SHAPES))
def test_a1_margin_is_at_least_40_nats(route, dtype):
    B, H, Tq, Tk, d = small(V.ATTN_SHAPES[route])
    q, k, _ = V.attn_inputs("A1", B, H, Tq, Tk, d, dtype, live=V.CTX_COUNT if route == "ctx" else None)
    kw = dict(causal=route == "short", count=V.CTX_COUNT if route == "ctx" else None)
    assert V.a1_margin(q, k, H, d ** -0.5, **kw) >= V.A1_MARGIN
    assert V.a1_margin(V.prescale(q, d)[1], k, H, d ** -0.5, **kw) >= V.A1_MARGIN
    # all mass of the first query in the first tile, of the last query in the last (partly masked) tile
    p = torch.softmax(V.attn_logits(q, k, H, d ** -0.5, **kw)[0], -1)[0, 0]
    n = V.CTX_COUNT if route == "ctx" else Tk
    assert p[0, :V.TILE].sum() > 1 - 1e-12 and p[-1, (n - 1) // V.TILE * V.TILE:n].sum() > 1 - 1e-12


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pattern", [p for p in V.A_PATTERNS if p.startswith("A2")])
@pytest.mark.parametrize("route", ["generic", "attn2", "resident"])
def test_a2_realised_step_is_within_02_of_its_target(route, pattern, dtype):
    B, H, Tq, Tk, d = small(V.ATTN_SHAPES[route])
    q, k, _ = V.attn_inputs(pattern, B, H, Tq, Tk, d, dtype)
    want = float(pattern.split("_")[1]) * (-1.0 if pattern.endswith("desc") else 1.0)
    for qq in (q, V.prescale(q, d)[1]):
        lo, hi = V.a2_steps(qq, k, H, d ** -0.5)
        assert want - 0.2 <= lo <= hi <= want + 0.2, (lo, hi, want)
    if "3.9" in pattern:
        assert abs(lo) < V.DEFER and abs(hi) < V.DEFER
    else:
        assert abs(lo) > V.DEFER and abs(hi) > V.DEFER


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a3_logits_sit_250_nats_from_zero_and_a5_is_the_mean(dtype):
    B, H, Tq, Tk, d = small(V.ATTN_SHAPES["attn2"])
    q, k, v = V.attn_inputs("A3", B, H, Tq, Tk, d, dtype)
    s = V.attn_logits(q, k, H, d ** -0.5)[0]
    assert ((s[:, :, 0::2] - 250).abs().max() < 12) and ((s[:, :, 1::2] + 250).abs().max() < 12)
    assert (s.max(-1).values - s.min(-1).values).median() > 3
    q, k, v = V.attn_inputs("A5", B, H, Tq, Tk, d, dtype)
    ref = V.attn_ref(q, k, v, H, d ** -0.5, dtype)[0]
    assert (ref - v.double().mean(1, keepdim=True)).abs().max() < 1e-12


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("route", list(V.GEMM_SHAPES) + ["conv"])
def test_g2_cancels_to_a_hundredth_of_s(route, dtype):
    if route == "conv":
        ref, S = V.conv_ref(V.conv_inputs("G2", *V.CONV_SHAPE, dtype))
        assert (S / ref.abs()).median() >= 100
        return
    d = V.gemm_inputs("G2", *V.GEMM_SHAPES[route], dtype)
    for side in (False, True):
        ref, S = V.gemm_ref(d, side, side)
        assert (S / ref.abs()).median() >= 100, float((S / ref.abs()).median())


@pytest.mark.parametrize("route", list(V.GEMM_SHAPES) + ["conv"])
def test_g3_range_and_excluded_share(route):
    dtype = torch.float16
    if route == "conv":
        B, H, Wd, Cin, Cout = V.CONV_SHAPE
        ref, S = V.conv_ref(V.conv_inputs("G3", *V.CONV_SHAPE, dtype))
        cold, hot_ref = ref[:, :H - 3], ref[:, H - 1]
    else:
        M = V.GEMM_SHAPES[route][0]
        d = V.gemm_inputs("G3", *V.GEMM_SHAPES[route], dtype)
        assert torch.isfinite(d["A"].float()).all() and torch.isfinite(d["R"].float()).all()
        ref, S = V.gemm_ref(d)
        cold, hot_ref = ref[:M - 1], ref[M - 1]
    assert 2.0 ** 14 <= float(cold.abs().max()) < 2.0 ** 15
    excl = ((hot_ref.abs() - 65520.0).abs() <= 2 * V.u16(dtype) * 65520.0).double().mean()
    assert excl <= 0.02, float(excl)
    inf = torch.isinf(hot_ref.to(dtype))
    assert inf.any() and not inf.all(), "the hot row must hold overflowing and finite elements"


def test_g4_lands_in_the_fp16_subnormal_range():
    d = V.gemm_inputs("G4", *V.GEMM_SHAPES["tile64"], torch.float16)
    ref, _ = V.gemm_ref(d)
    assert float(d["W"].float().abs().max()) < 2.0 ** -14 and float(ref.abs().max()) < 2.0 ** -14
    assert (d["A"].float() != 0).float().mean() > 0.9 and (d["W"].float() != 0).float().mean() > 0.9


# ---- 2. + 3. GEMM / conv -------------------------------------------------------------------------------------------------------------
def g_patterns(dtype):
    return [p for p in V.G_PATTERNS if p != "G3" or dtype == torch.float16]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("route", list(V.GEMM_SHAPES))
def test_gemm_emulation_within_bound_and_wrong_kernels_outside(route, dtype):
    M, N, K = V.GEMM_SHAPES[route]
    side, staged = route in V.SIDE_OPERANDS, route in V.STAGED_RESIDUAL
    emu = lambda d, **kw: V.emu_gemm(d, dtype, side, side, staged=staged, **kw)
    for pattern in g_patterns(dtype):
        d = V.gemm_inputs(pattern, M, N, K, dtype)
        ref, bound, x1, single = V.gemm_bound(d, route, K, dtype)
        out = emu(d)
        if pattern == "G3":
            hot = torch.zeros_like(ref, dtype=torch.bool); hot[M - 1] = True
            r, mism, excl = V.g3_check(out, ref, bound, hot, dtype, x1)
            assert r <= 1 and mism == 0 and excl <= 0.02, (route, r, mism, excl)
            continue
        assert V.ratio(out, ref, bound) <= 1, (route, pattern, V.ratio(out, ref, bound))
        if pattern == "G4" and dtype == torch.float16:
            # 8 products of ~2^-24 vanish below half a subnormal step; the error G4 exists for in fp16 is a kernel that flushes subnormal operands
            wrong = V.ratio(emu(d, flush=True), ref, bound)
            assert wrong > 2, (route, wrong)
        else:
            wrong = V.ratio(emu(d, drop_last=8), ref, bound)
            assert wrong > 10, (route, pattern, wrong)
    d = V.gemm_inputs("G1", M, N, K, dtype)
    ref, bound, x1, single = V.gemm_bound(d, route, K, dtype)
    assert V.ratio(emu(d, rtz=True), ref, bound) > 1                 # a truncating store: up to 2 u16
    if staged:      # the two-rounding bound is not a blank cheque: a third rounding (the product stored before the bias) exceeds it,
        assert V.ratio(emu(d, three_roundings=True), ref, bound) > 1          # and the staged epilogue really is outside the one-rounding bound
        assert V.ratio(emu(d), ref, single) > 1


def conv_emu(d, dtype, drop_last=0, flush=False):
    x, w = d["x"].float(), d["w"].float().clone()
    if drop_last:
        w[:, 2, 2, -drop_last:] = 0.0                               # the last k-slab of the (tap, channel) contraction
    if flush:
        tiny = float(torch.finfo(dtype).tiny)
        x = torch.where(x.abs() < tiny, torch.zeros_like(x), x); w = torch.where(w.abs() < tiny, torch.zeros_like(w), w)
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_conv_emulation_within_bound_and_wrong_kernels_outside(dtype):
    B, H, Wd, Cin, Cout = V.CONV_SHAPE
    for pattern in g_patterns(dtype):
        d = V.conv_inputs(pattern, B, H, Wd, Cin, Cout, dtype)
        ref, S = V.conv_ref(d)
        bound = V.B_gemm(ref, S, 9 * Cin, dtype)
        out = conv_emu(d, dtype)
        if pattern == "G3":
            hot = torch.zeros_like(ref, dtype=torch.bool); hot[:, H - 1] = True
            r, mism, excl = V.g3_check(out, ref, bound, hot, dtype)
            assert r <= 1 and mism == 0 and excl <= 0.02, (r, mism, excl)
            continue
        assert V.ratio(out, ref, bound) <= 1, pattern
        if pattern == "G4" and dtype == torch.float16:
            assert V.ratio(conv_emu(d, dtype, flush=True), ref, bound) > 2
        else:
            assert V.ratio(conv_emu(d, dtype, drop_last=8), ref, bound) > 10, pattern


# ---- 2. + 3. sweeps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sweep_emulations(dtype):
    x = V.all_bits(dtype)
    y0 = x[V.sweep_perm()]
    xf = x.float()
    emu = {"SILU": xf * (1.0 / (1.0 + torch.exp(-xf))), "SCALE": xf * 0.37, "ADD": y0.float() + xf, "COPY": xf}
    for op, val in emu.items():
        ref64, ref32 = V.sweep_ref(op, x, dtype, y0)
        bad, worst = V.sweep_check(val.to(dtype), ref64, ref32, dtype, floor=V.FP32_FLOOR if op == "SILU" else 0.0)
        assert bad == 0 and worst <= 1, (op, bad, worst)
    # WRONG: a kernel that flushes bf16 results below 2^-119 passes only where the floor applies (SiLU), nowhere else
    if dtype == torch.bfloat16:
        flushed = torch.where(xf.abs() < 2.0 ** -119, torch.zeros_like(xf), xf).to(dtype)
        ref64, ref32 = V.sweep_ref("COPY", x, dtype)
        assert V.sweep_check(flushed, ref64, ref32, dtype)[0] > 1000
    # WRONG: a store that adds an ulp of error on top of the rounding (two steps away) is caught
    ref64, ref32 = V.sweep_ref("SCALE", x, dtype)
    two_off = (ref32.to(dtype).view(torch.int16) + 2).view(dtype)
    assert V.sweep_check(two_off, ref64, ref32, dtype)[0] > 60000


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_copy_set_holds_ties_and_a_truncating_store_fails_it(dtype):
    x = V.copy_set(dtype)
    want = x.to(dtype)
    assert x.numel() % 8 == 0 and V.same_bits_or_nan(want, want) == 0
    fin = torch.isfinite(x) & torch.isfinite(want.float())
    ties = fin & ((x.double() - want.double()).abs() == V.ulp16(want.double(), dtype) / 2)
    assert ties.sum() > 30000, "the exact midpoints between adjacent 16-bit values"
    assert torch.isinf(want[torch.isfinite(x)]).any(), "finite fp32 values that overflow the type"
    if dtype == torch.float16:
        assert (want.float().abs()[fin] < 2.0 ** -14).sum() > 3000, "subnormal results"
    assert V.same_bits_or_nan(V.round_toward_zero(x, dtype), want) > 30000          # WRONG: round toward zero on store


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_geglu_emulation_within_bound_and_erf_clamped_at_2_outside(dtype):
    _, _, h, g = V.geglu_inputs(dtype, 8)
    ref, bound = V.geglu_ref(h, g, dtype)
    r, bad = V.geglu_check(V.emu_geglu(h, g, dtype), ref, bound, dtype)
    assert r <= 1 and bad == 0, (r, bad)
    r, _ = V.geglu_check(V.emu_geglu(h, g, dtype, clamp=2.0), ref, bound, dtype)
    assert r > 50, r


# ---- 2. + 3. norms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("pattern", V.N_PATTERNS)
def test_groupnorm_emulation_passes_close(pattern, silu, dtype):
    x, gamma, beta = V.gn_inputs(pattern, 2, 100, 320, 32, dtype)
    close(V.emu_gn(x, 32, gamma, beta, 1e-5, silu), V.gn_ref(x, 32, gamma, beta, 1e-5, silu), name=f"values cpu gn {pattern}", kind=V.kind_of(dtype))


def test_groupnorm_naive_variance_fails_close():
    """WRONG: E[x^2] - E[x]^2 in fp32 at |mean| = 1000, unit spread (the fp16 pattern): x^2 ~ 1e6 has an fp32 spacing of 1/16, the size of
    the variance's own rounding budget."""
    x, gamma, beta = V.gn_inputs("common_mean", 2, 100, 320, 32, torch.float16)
    with pytest.raises(AssertionError):
        close(V.emu_gn(x, 32, gamma, beta, 1e-5, False, naive=True), V.gn_ref(x, 32, gamma, beta, 1e-5, False), name="values cpu gn naive", kind="f16")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pattern", V.N_PATTERNS)
def test_layernorm_emulation_passes_close(pattern, dtype):
    x, gamma, beta = V.ln_inputs(pattern, 37, 320, dtype)
    out = F.layer_norm(x.float(), (320,), gamma, beta, 1e-5).to(dtype)
    close(out, F.layer_norm(x.double(), (320,), gamma.double(), beta.double(), 1e-5), name=f"values cpu ln {pattern}", kind=V.kind_of(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_layernorm_emulation_within_the_three_limits(dtype):
    d = V.ln_offset_inputs(300, 320, 320, dtype)
    fused = V.emu_ln_fused(d["x"], d["Wp"], d["b"], d["csum"], dtype)
    xh = F.layer_norm(d["x"].float(), (320,), None, None, 1e-5).to(dtype)
    scratch = (xh.float() @ d["Wp"].float().T + d["b"]).to(dtype)
    lim = V.LN_OFFSET_LIMITS
    assert V.rel_l2(fused, V.ln_lin_ref(d["x"], d["Wp"], d["b"])) < lim["fused"]
    assert V.rel_l2(scratch, V.ln_lin_ref(d["x"], d["Wp"], d["b"], stored=dtype)) < lim["scratch"]
    assert V.rel_l2(fused, scratch) < lim["drift"]
    # WRONG: the mean term with the wrong sign
    xf = d["x"].float()
    mean = xf.mean(1, keepdim=True); rstd = torch.rsqrt(xf.var(1, unbiased=False, keepdim=True) + 1e-5)
    wrong = (rstd * (xf @ d["Wp"].float().T + mean * d["csum"][None]) + d["b"]).to(dtype)
    assert not V.rel_l2(wrong, V.ln_lin_ref(d["x"], d["Wp"], d["b"])) < lim["fused"]


# ---- 2. + 3. attention ---------------------------------------------------------------------------------------------------------------
def attn_case(route, pattern, dtype, pre):
    B, H, Tq, Tk, d = small(V.ATTN_SHAPES[route])
    q, k, v = V.attn_inputs(pattern, B, H, Tq, Tk, d, dtype, live=V.CTX_COUNT if route == "ctx" else None)
    kw = dict(causal=route == "short", count=V.CTX_COUNT if route == "ctx" else None)
    qk, qr = V.prescale(q, d) if pre else (q, q)
    ref, inner = V.attn_ref(qr, k, v, H, d ** -0.5, dtype, **kw)
    return qk, k, v, H, d, kw, ref, V.attn_bound(ref, inner, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pattern", V.A_PATTERNS)
@pytest.mark.parametrize("route,pre,fold", [("generic", False, False), ("attn2", False, False), ("attn2", True, True), ("resident", True, True),
                                            ("short", False, False), ("ctx", False, False), ("ctx", True, False)])
def test_attention_emulation_within_bound(route, pre, fold, pattern, dtype):
    if route == "short" and pattern == "A5":
        return                                  # the causal route gets A1-A4
    qk, k, v, H, d, kw, ref, bound = attn_case(route, pattern, dtype, pre)
    out = V.emu_attn(qk, k, v, H, d ** -0.5, dtype, pre=pre, fold=fold, **kw)
    assert torch.isfinite(out.float()).all()
    assert V.ratio(out, ref, bound) <= 1, V.ratio(out, ref, bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attention_wrong_emulations_exceed_the_bound(dtype):
    # a skipped O rescale on the LAST tile that raises the maximum (a later rescale would hide the slip): a rise of 12 log2 units, and one just
    # over the deferral threshold
    for pattern in ("A2_12", "A2_4.1"):
        qk, k, v, H, d, kw, ref, bound = attn_case("generic", pattern, dtype, False)
        assert V.ratio(V.emu_attn(qk, k, v, H, d ** -0.5, dtype, skip_rescale_tile=2), ref, bound) > 10, pattern
    # a rebase with the wrong sign (FOLD)
    for pattern in ("A2_4.1", "A2_12", "A1"):
        qk, k, v, H, d, kw, ref, bound = attn_case("attn2", pattern, dtype, True)
        out = V.emu_attn(qk, k, v, H, d ** -0.5, dtype, pre=True, fold=True, wrong_rebase=True)
        assert V.ratio(out, ref, bound) > 10, pattern


# ---- 2. + 3. Fourier / timestep embeddings -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fourier_emulation_within_bound(dtype):
    x = V.fourier_inputs()
    assert float(x.abs().max()) == 2000.0
    ref, bound = V.fourier_ref(x, 4, dtype)
    parts = [x]
    for i in range(4):
        parts += [torch.sin(x * float(2 ** i)), torch.cos(x * float(2 ** i))]
    out = torch.cat(parts, -1).reshape(x.shape[0], -1).to(dtype)
    assert V.ratio(out, ref, bound) <= 1
    # WRONG: the argument reduced in 16-bit precision
    parts = [x]
    for i in range(4):
        a = (x * float(2 ** i)).to(dtype).float()
        parts += [torch.sin(a), torch.cos(a)]
    assert V.ratio(torch.cat(parts, -1).reshape(x.shape[0], -1).to(dtype), ref, bound) > 10


def test_timestep_embedding_emulation_within_2e4():
    t = torch.tensor(V.TIMESTEPS)
    ref = V.timeemb_ref(t)
    half = 160
    e = t[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)[None]
    out = torch.cat([torch.cos(e), torch.sin(e)], -1)
    assert (out.double() - ref).abs().max() < 2e-4
    assert not (torch.cat([torch.sin(e), torch.cos(e)], -1).double() - ref).abs().max() < 2e-4       # WRONG: sin / cos halves swapped
