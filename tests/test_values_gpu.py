"""-m gpu: every kernel on the value ranges a trained network produces (tests/values_data.py: generators, fp64 references, derived bounds).

The rest of the suite varies shapes, strides and routes on unit-scale Gaussians; this file varies the VALUES at the smallest shapes that
reach each route: outlier channels, cancelling sums, the fp16 range and its subnormals, every 16-bit bit pattern through the element-wise
kernels and the GELU / SiLU epilogues, norms far from zero mean, attention rows that are one-hot, that climb a staircase across the
deferred-maximum threshold, that sit 250 nats from zero.  Both storage types; every case asserts the kernel it meant to reach
(mdx_last_kernel) and logs worst |err| / bound as values:<family>:<case>:<route>:<dtype> (helpers.parity_log).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from magicdrive_amd import _lib as L
from magicdrive_amd import ops as O
from magicdrive_amd import packing as PK

import values_data as V  # noqa: E402
from helpers import XF_ATOL, XF_RTOL, close, parity_log  # noqa: E402
from test_edges_gpu import Guarded, last_kernel, rnd  # noqa: E402
from test_kernels_gpu import attn2_route, rowstat_ref  # noqa: E402

F32 = torch.float32
DTYPES = [torch.bfloat16, torch.float16]
KIND = {torch.bfloat16: "bf16", torch.float16: "f16"}
NAN = float("nan")


def log(family, case, route, dtype, worst, **extra):
    parity_log(f"values:{family}:{case}:{route}:{KIND[dtype]}", worst_err_over_bound=float(worst), **extra)


def close_logged(out, ref, family, case, route, dtype):
    """helpers.close() (the xformers table of the storage type), with its worst err / tol also logged under the values: name."""
    o = out.detach().float().cpu().double(); r = ref.double()
    tol = XF_ATOL[KIND[dtype]] * (r.float().abs().mean().item() + 1e-6) + XF_RTOL[KIND[dtype]] * r.abs()
    log(family, case, route, dtype, ((o - r).abs() / tol).max())
    close(out, ref, name=f"values:{family}:{case}:{route}", kind=KIND[dtype])


def nan_buf(n, dev):
    return torch.full((n,), NAN, dtype=F32, device=dev)


# --------------------------------------------------------------------------------------------------------------------------------------
# G: GEMM / conv values
# --------------------------------------------------------------------------------------------------------------------------------------
GEMM_ROUTES = {
    "tile64": dict(opts={}, splitk=1, expect=("gemm_conv_kernel<64,64,",)),
    "splitk": dict(opts={}, splitk=5, expect=("gemm_conv_kernel<",)),
    "ws": dict(opts=dict(GEMM_WS=2), splitk=0, expect=("gemm_ws_kernel<plain>",)),
    "xl": dict(opts=dict(GEMM_XL=2), splitk=0, expect=("gemm_xl_kernel<256x", "gemm_xlp_kernel<256x")),
    # the same main loops with bias + residual: the coalesced epilogues add R to the staged 16-bit tile (two roundings: B_gemm_residual),
    # the split-K reduction adds it in fp32 (one rounding: B_gemm)
    "tile64_res": dict(opts={}, splitk=1, expect=("gemm_conv_kernel<64,64,",)),
    "splitk_res": dict(opts={}, splitk=5, expect=("gemm_conv_kernel<",)),
    "xl_res": dict(opts=dict(GEMM_XL=2), splitk=0, expect=("gemm_xl_kernel<256x", "gemm_xlp_kernel<256x")),
}
G_CASES = [(p, dt) for dt in DTYPES for p in V.G_PATTERNS if p != "G3" or dt == torch.float16]
G_IDS = [f"{p}-{KIND[dt]}" for p, dt in G_CASES]
GEMM_CASES = [pytest.param(route, p, dt, id=f"{route}-{p}-{KIND[dt]}") for route in GEMM_ROUTES for p, dt in G_CASES]


def g_verdict(out, ref, bound, pattern, hot, dtype, family_case_route, x1=None, single=None):
    extra = {} if x1 is None else dict(bound="two roundings", over_single_rounding_bound=V.ratio(out, ref, single) if pattern != "G3" else None)
    if pattern == "G3":
        r, mism, excl = V.g3_check(out, ref, bound, hot, dtype, x1)
        log(*family_case_route, dtype, r, inf_mismatches=mism, excluded_share=excl, **extra)
        assert excl <= 0.02 and mism == 0, (mism, excl)
    else:
        r = V.ratio(out, ref, bound)
        log(*family_case_route, dtype, r, **extra)
        assert torch.isfinite(out.float()).all()
    assert r <= 1.0, f"{family_case_route}: worst err / bound = {r:.3f}"


@pytest.mark.parametrize("route,pattern,dtype", GEMM_CASES)
def test_gemm_values(dev, route, pattern, dtype):
    """G1 outlier channels, G2 cancellation, G3 fp16 range with an overflowing row, G4 subnormal-range operands on the generic 64x64 tile,
    forced split-K 5, the weight-stationary kernel (bias + residual) and the XL kernel, against B_gemm; the generic tile, split-K and XL once
    more with bias + residual.  Where the residual is added to the staged 16-bit tile (ws, tile64_res, xl_res) the bound is the two-rounding
    B_gemm_residual — against the one-rounding B_gemm those routes measure up to 25x (G4 / G1, where R cancels the product; logged as
    over_single_rounding_bound); split-K adds R in fp32 and is held to B_gemm."""
    r = GEMM_ROUTES[route]
    M, N, K = V.GEMM_SHAPES[route]
    d = V.gemm_inputs(pattern, M, N, K, dtype)
    C = Guarded((M, N), N, 0, dtype, dev)
    ws = nan_buf(1 << 22, dev)
    kw = dict(bias=d["bias"].to(dev), R=d["R"].to(dev)) if route in V.SIDE_OPERANDS else {}
    with L.options(**r["opts"]):
        O.run_ops([O.Gemm(d["A"].to(dev), d["W"].to(dev), C.view, splitk=r["splitk"], ws=ws, **kw)])
        kern = last_kernel()
    torch.cuda.synchronize()
    assert kern.startswith(r["expect"]), kern
    if route == "splitk":
        assert not torch.isnan(ws[:5 * M * N]).any() and torch.isnan(ws[5 * M * N:]).all(), "five fp32 slabs expected in the workspace"
    ref, bound, x1, single = V.gemm_bound(d, route, K, dtype)
    hot = torch.zeros_like(ref, dtype=torch.bool); hot[M - 1] = True
    g_verdict(C.view.cpu(), ref, bound, pattern, hot, dtype, ("G", pattern, route), x1, single)
    assert C.border_intact()


@pytest.mark.parametrize("pattern,dtype", G_CASES, ids=G_IDS)
@pytest.mark.parametrize("route,opts,expect", [("conv64", {}, ("gemm_conv_kernel<64,64,",)), ("convxl", dict(GEMM_XL=2), ("gemm_xl_kernel<256x",))])
def test_conv_values(dev, route, opts, expect, pattern, dtype):
    """The G patterns through the 3x3 conv (K = 9 Cin) on the generic tile and on the XL kernel, against B_gemm with S = conv2d(|x|, |w|)."""
    B, H, Wd, Cin, Cout = V.CONV_SHAPE
    d = V.conv_inputs(pattern, B, H, Wd, Cin, Cout, dtype)
    y = torch.full((B, H, Wd, Cout), NAN, dtype=dtype, device=dev)
    with L.options(**opts):
        O.run_ops([O.Conv(d["x"].to(dev), d["w"].to(dev), y, ws=nan_buf(1 << 20, dev))])
        kern = last_kernel()
    torch.cuda.synchronize()
    assert kern.startswith(expect) and (route != "convxl" or kern.endswith(",conv>")), kern
    ref, S = V.conv_ref(d)
    hot = torch.zeros_like(ref, dtype=torch.bool); hot[:, H - 1] = True
    g_verdict(y.cpu(), ref, V.B_gemm(ref, S, 9 * Cin, dtype), pattern, hot, dtype, ("G", pattern, route))


# --------------------------------------------------------------------------------------------------------------------------------------
# E: exhaustive 16-bit sweeps
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("op", ["SILU", "SCALE", "ADD", "COPY"])
def test_elementwise_every_bit_pattern(dev, op, dtype):
    """Every bit pattern of the storage type through EW_SILU / EW_SCALE (0.37) / EW_ADD (against a fixed permutation of the set) / EW_COPY, on
    ew_vec8_kernel and, through a one-element-offset view, on ew_scalar_kernel: values_data.sweep_check, and the two kernels agree bitwise (EW_ADD: NaN + NaN as NaN-ness)."""
    code = {"ADD": L.EW_ADD, "COPY": L.EW_COPY, "SILU": L.EW_SILU, "SCALE": L.EW_SCALE}[op]
    Cc = 8
    x = V.all_bits(dtype).reshape(-1, Cc); y0 = V.all_bits(dtype)[V.sweep_perm()].reshape(-1, Cc)
    ref64, ref32 = V.sweep_ref(op, x, dtype, y0)
    outs = []
    for ld, off, expect in ((Cc, 0, "ew_vec8_kernel"), (Cc + 3, 1, "ew_scalar_kernel")):
        X = Guarded(tuple(x.shape), ld, off, dtype, dev, fill=x.to(dev))
        Y = Guarded(tuple(x.shape), ld, off, dtype, dev, fill=y0.to(dev) if op == "ADD" else None)
        O.run_ops([O.Ew(code, X.view, Y.view, alpha=0.37)])
        kern = last_kernel()
        torch.cuda.synchronize()
        assert kern == expect, kern
        out = Y.view.cpu()
        bad, worst = V.sweep_check(out, ref64, ref32, dtype, floor=V.FP32_FLOOR if op == "SILU" else 0.0)
        log("E", op, expect, dtype, worst, violations=bad)
        assert bad == 0 and worst <= 1.0, (expect, bad, worst)
        outs.append(out)
    if op == "ADD":      # an fp32 add of two NaNs returns the payload of whichever operand the compiler put first, and it may order the two
        diff = V.same_bits_or_nan(outs[0], outs[1])     # kernels' adds differently: two NaNs count as equal here, whatever their payload
        assert diff == 0, f"ew_vec8_kernel and ew_scalar_kernel differ in {diff} elements"
    else:
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "ew_vec8_kernel and ew_scalar_kernel differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_copy_fp32_to_16_bit_exact_with_ties(dev, dtype):
    """fp32 -> 16-bit EW_COPY on every 16-bit value, its fp32 neighbours and the exact midpoints (ties to even; overflow to inf, subnormals):
    bit-exact against x.to(dtype), NaN compared as NaN-ness."""
    x = V.copy_set(dtype)[None, :]
    Y = Guarded(tuple(x.shape), x.shape[1], 0, dtype, dev)
    O.run_ops([O.Ew(L.EW_COPY, x.to(dev), Y.view)])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern == "ew_scalar_kernel", kern
    diff = V.same_bits_or_nan(Y.view.cpu(), x.to(dtype))
    log("E", "COPY_f32", kern, dtype, float(diff), violations=diff)
    assert diff == 0 and Y.border_intact(), f"{diff} of {x.numel()} conversions differ from round-to-nearest-even"


GEGLU_ROUTES = {
    "tile": dict(K=8, opts={}, expect=("gemm_conv_kernel<",)),
    "ws": dict(K=320, opts=dict(GEMM_WS=2), expect=("gemm_ws_kernel<geglu>",)),
    "xl": dict(K=64, opts=dict(GEMM_XL=2), expect=("gemm_xl_kernel<256x", "gemm_xlp_kernel<256x")),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("route", list(GEGLU_ROUTES))
def test_geglu_epilogue_every_gate_pattern(dev, route, dtype):
    """h gelu(g) for every finite 16-bit gate g and h in {1, -3, 0.01} through the GEGLU epilogue of each main loop (two-hot A rows, W routing
    column 0 to every value slot and column 1 to every gate slot): |err| <= u16 |ref| + sub16 + 1.35e-5 |h g| (the 2.7e-5 erf error csrc/common.h
    claims, through 0.5 h g erf), the reference's infinity where h gelu(g) overflows the type."""
    r = GEGLU_ROUTES[route]
    A, W, h, g = V.geglu_inputs(dtype, r["K"])
    Wp, bp = PK.pack_geglu(W, torch.zeros(W.shape[0]), dtype)
    C = torch.full((A.shape[0], W.shape[0] // 2), NAN, dtype=dtype, device=dev)
    with L.options(**r["opts"]):
        O.run_ops([O.Gemm(A.to(dev), Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU, ws=nan_buf(1 << 22, dev))])
        kern = last_kernel()
    torch.cuda.synchronize()
    assert kern.startswith(r["expect"]), kern
    ref, bound = V.geglu_ref(h, g, dtype)
    worst, bad = 0.0, 0
    for col in (C.float().amax(1), C.float().amin(1)):          # every column of a row holds the same product: its extremes (amax / amin propagate NaN)
        w_, b_ = V.geglu_check(col.to(dtype), ref, bound, dtype)
        worst, bad = max(worst, w_), bad + b_
    log("E", "GEGLU", route, dtype, worst, overflow_mismatches=bad)
    assert worst <= 1.0 and bad == 0, (worst, bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_conv_silu_epilogue_every_pattern(dev, dtype):
    """Every finite 16-bit pattern through the SiLU epilogue of the conv kernel (1x1 conv, identity weights): the sweep contract of EW_SILU."""
    x = V.finite_bits(dtype)
    Cc = 64
    Wd = 34 if dtype == torch.bfloat16 else 32
    x = x.reshape(1, -1, Wd, Cc)
    w = torch.eye(Cc).reshape(Cc, 1, 1, Cc).to(dtype)
    y = torch.full(tuple(x.shape), NAN, dtype=dtype, device=dev)
    O.run_ops([O.Conv(x.to(dev), w.to(dev), y, pad=(0, 0), epilogue=L.EPI_SILU)])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern.startswith("gemm_conv_kernel<") and kern.endswith(",conv>"), kern
    ref64, ref32 = V.sweep_ref("SILU", x, dtype)
    bad, worst = V.sweep_check(y.cpu(), ref64, ref32, dtype, floor=V.FP32_FLOOR)
    log("E", "SILU", "conv_epilogue", dtype, worst, violations=bad)
    assert bad == 0 and worst <= 1.0, (bad, worst)


# --------------------------------------------------------------------------------------------------------------------------------------
# N: norms
# --------------------------------------------------------------------------------------------------------------------------------------
GN_PATHS = {"one_launch": dict(shape=(2, 100, 320, 32), opts={}, ws=False, expect="groupnorm_kernel"),
            "two_stage": dict(shape=(2, 128, 320, 32), opts=dict(GN_ONE_KERNEL_ELEMS=0), ws=True, expect="gn_stats_kernel+gn_apply_kernel")}


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("pattern", V.N_PATTERNS)
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("path", list(GN_PATHS))
def test_groupnorm_values(dev, path, silu, pattern, dtype):
    """An all-zero group beside ordinary ones (bitwise round16(act(beta)) there), per-channel means up to 64 (bf16) / 1000 (fp16), the whole
    tensor at that mean, one pixel x1000: the one-launch kernel and the two-stage path, close() against fp64."""
    p = GN_PATHS[path]
    B, HW, Cc, G = p["shape"]
    x, gamma, beta = V.gn_inputs(pattern, B, HW, Cc, G, dtype)
    Y = Guarded((B, HW, Cc), Cc, 0, dtype, dev)
    with L.options(**p["opts"]):
        O.run_ops([O.GroupNorm(x.to(dev), Y.view, gamma.to(dev), beta.to(dev), G, 1e-5, silu=silu, ws=nan_buf(1 << 18, dev) if p["ws"] else None)])
        kern = last_kernel()
    torch.cuda.synchronize()
    assert kern == p["expect"], kern
    close_logged(Y.view, V.gn_ref(x, G, gamma, beta, 1e-5, silu), "N", f"gn_{pattern}_{'silu' if silu else 'plain'}", path, dtype)
    assert Y.border_intact()
    if pattern == "zero_group":
        cpg = Cc // G
        b = beta[3 * cpg:4 * cpg].double()
        want = (F.silu(b) if silu else b).to(dtype)
        got = Y.view[:, :, 3 * cpg:4 * cpg].cpu()
        assert torch.equal(got.view(torch.int16), want.expand_as(got).contiguous().view(torch.int16)), "an all-zero group must give round16(act(beta)) exactly"


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("pattern", V.N_PATTERNS)
@pytest.mark.parametrize("Cc", [320, 1280])
def test_layernorm_values(dev, Cc, pattern, dtype):
    M = 37
    x, gamma, beta = V.ln_inputs(pattern, M, Cc, dtype)
    Y = Guarded((M, Cc), Cc, 0, dtype, dev)
    O.run_ops([O.LayerNorm(x.to(dev), Y.view, gamma.to(dev), beta.to(dev), 1e-5)])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern == "layernorm_kernel", kern
    ref = F.layer_norm(x.double(), (Cc,), gamma.double(), beta.double(), 1e-5)
    close_logged(Y.view, ref, "N", f"ln_{pattern}", f"C{Cc}", dtype)
    assert Y.border_intact()
    if pattern == "zero_group":
        got = Y.view[3:5].cpu()
        assert torch.equal(got.view(torch.int16), beta.to(dtype).expand_as(got).contiguous().view(torch.int16))


def run_producer(dev, A, W, bias, dtype, producer, parts=3):
    """A GEMM that leaves rowstat_out: (stored C, statistics, kernel tag).  "ws": the weight-stationary kernel's store phase; "rowstat_kernel":
    a forced split-K 2 GEMM followed by the statistics pass."""
    M, N = A.shape[0], W.shape[0]
    X = torch.full((M, N), NAN, dtype=dtype, device=dev)
    st = torch.full((parts, M, 2), NAN, dtype=F32, device=dev)
    with L.options(GEMM_WS=2):
        O.run_ops([O.Gemm(A.to(dev), W.to(dev), X, bias=bias.to(dev), rowstat=st, splitk=0 if producer == "ws" else 2, ws=nan_buf(1 << 20, dev))])
        kern = last_kernel()
    torch.cuda.synchronize()
    assert kern == ("gemm_ws_kernel<plain,rs>" if producer == "ws" else "rowstat_kernel"), kern
    return X, st


def rowstat_error(X, st, producer):
    N = X.shape[1]
    got = st.double().cpu()
    assert torch.isfinite(got).all()
    nt = (N + 127) // 128 if producer == "ws" else 1
    want = rowstat_ref(X, [(128 * k, min(N, 128 * k + 128)) for k in range(nt)] if nt > 1 else [(0, N)])
    assert (got[nt:] == 0).all(), "unused parts must be exactly zero"
    return ((got[:nt] - want).abs() / (want.abs() + 1.0)).max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("case", ["G1", "offset1000"])
@pytest.mark.parametrize("producer", ["ws", "rowstat_kernel"])
def test_rowstat_out_values(dev, producer, case, dtype):
    """(sum, sum of squares) of the stored rows under outlier channels (G1) and under a +1000 common offset, from both producers, against fp64
    sums of the stored values at the 2e-5 relative limit of test_gemm_row_statistics_out."""
    M, N, K = 300, 320, 320
    if case == "G1":
        d = V.gemm_inputs("G1", M, N, K, dtype)
        A, W, bias = d["A"], d["W"], d["bias"]
    else:
        A, W, bias = rnd(M, K, seed=1, dtype=dtype), (10.0 * torch.eye(K)).to(dtype), torch.full((N,), 1000.0)
    X, st = run_producer(dev, A, W, bias, dtype, producer)
    err = rowstat_error(X, st, producer)
    log("N", f"rowstat_{case}", producer, dtype, err / 2e-5, rel_err=err)
    assert err < 2e-5, err


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_fused_layernorm_large_offset_every_route(dev, dtype):
    """x = 1000 + 10 N(0,1) (|mean| / sigma = 100), K = 320, M = 300, N = 320 under GEMM_WS = 2: the in-kernel statistics route <plain,ln>, the
    producer-statistics routes <plain,lns> (statistics written by gemm_ws_kernel<plain,rs> and by rowstat_kernel through rowstat_out) and
    <geglu,lns>, and the scratch routes (GEMM_WS = 0).  Each against the fp64 LayerNorm -> Linear on the same W', and the fused routes against
    the scratch route, at the three rel-L2 limits of test_gemm_fused_layernorm_large_common_offset_routes_agree (2e-2, 1e-2, 2e-2: fp32 sums
    of 320 squares of ~1e6 carry ~1 % of the variance as rounding error whatever the storage type)."""
    M, K, N = 300, 320, 320
    lim = V.LN_OFFSET_LIMITS
    d = V.ln_offset_inputs(M, K, N, dtype)
    A0, W0, b0 = rnd(M, K, seed=1, dtype=dtype), (10.0 * torch.eye(K)).to(dtype), torch.full((K,), 1000.0)
    X, st_ws = run_producer(dev, A0, W0, b0, dtype, "ws")
    X2, st_rk = run_producer(dev, A0, W0, b0, dtype, "rowstat_kernel")
    assert torch.equal(X, X2), "the two producers store different rows"
    xc = X.cpu()
    assert abs(float(xc.float().mean()) - 1000.0) < 2 and 8 < float(xc.float().std(1).mean()) < 12
    Wp, b, cs = d["Wp"].to(dev), d["b"].to(dev), d["csum"].to(dev)
    Fh = 320
    Wg = V.randn(2 * Fh, K, seed=12, scale=K ** -0.5); bg = V.randn(2 * Fh, seed=13)
    Wgf, bgf = Wg * d["gamma"][None, :], bg + Wg @ d["beta"]
    Wgp, bgp = PK.pack_geglu(Wgf, bgf, dtype)

    def run(opts, expect, geglu=False, stats=None):
        C = torch.full((M, Fh if geglu else N), NAN, dtype=dtype, device=dev)
        scratch = torch.full((M, K), NAN, dtype=dtype, device=dev)
        kw = dict(bias=bgp.to(dev), epilogue=L.EPI_GEGLU, ln_csum=Wgp.float().sum(1).to(dev)) if geglu else dict(bias=b, ln_csum=cs)
        with L.options(**opts):
            O.run_ops([O.Gemm(X, Wgp.to(dev) if geglu else Wp, C, ln_eps=1e-5, ln_scratch=scratch, ln_stats=stats, ws=nan_buf(1 << 20, dev), **kw)])
            kern = last_kernel()
        torch.cuda.synchronize()
        assert kern.startswith(expect), kern
        assert bool(torch.isnan(scratch.float()).all()) == (",ln" in kern), "a fused route must not touch ln_scratch; the others must fill it"
        assert torch.isfinite(C.float()).all()
        return C.cpu()

    def geglu_of(proj):
        h, g = proj.chunk(2, dim=-1)
        return h * F.gelu(g)

    ref = V.ln_lin_ref(xc, d["Wp"], d["b"]); ref_s = V.ln_lin_ref(xc, d["Wp"], d["b"], stored=dtype)
    gref = geglu_of(V.ln_lin_ref(xc, Wgf.to(dtype), bgf)); gref_s = geglu_of(V.ln_lin_ref(xc, Wgf.to(dtype), bgf, stored=dtype))
    scr = run(dict(GEMM_WS=0), "gemm_conv_kernel<")
    gscr = run(dict(GEMM_WS=0), "gemm_conv_kernel<", geglu=True)
    e = V.rel_l2(scr, ref_s); log("N", "ln_offset1000", "scratch", dtype, e / lim["scratch"], rel_l2=e)
    assert e < lim["scratch"], e
    e = V.rel_l2(gscr, gref_s); log("N", "ln_offset1000", "scratch_geglu", dtype, e / lim["scratch"], rel_l2=e)
    assert e < lim["scratch"], e
    fused = {"plain,ln": run(dict(GEMM_WS=2), "gemm_ws_kernel<plain,ln>"),
             "plain,lns<-ws": run(dict(GEMM_WS=2), "gemm_ws_kernel<plain,lns>", stats=st_ws),
             "plain,lns<-rowstat_kernel": run(dict(GEMM_WS=2), "gemm_ws_kernel<plain,lns>", stats=st_rk),
             "geglu,lns<-ws": run(dict(GEMM_WS=2), "gemm_ws_kernel<geglu,lns>", geglu=True, stats=st_ws),
             "geglu,lns<-rowstat_kernel": run(dict(GEMM_WS=2), "gemm_ws_kernel<geglu,lns>", geglu=True, stats=st_rk)}
    for name, out in fused.items():
        g_ = name.startswith("geglu")
        e, drift = V.rel_l2(out, gref if g_ else ref), V.rel_l2(out, gscr if g_ else scr)
        log("N", "ln_offset1000", name, dtype, max(e / lim["fused"], drift / lim["drift"]), rel_l2=e, drift_vs_scratch=drift)
        assert e < lim["fused"] and drift < lim["drift"], (name, e, drift)
    e = V.rel_l2(fused["plain,lns<-ws"], fused["plain,ln"])
    assert e < lim["drift"], e


# --------------------------------------------------------------------------------------------------------------------------------------
# A: attention values
# --------------------------------------------------------------------------------------------------------------------------------------
RING = {0: [5, 1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3, 5], 5: [4, 0]}
ATTN_ROUTES = {          # shape key, pre-scaled Q, options, extra
    "generic": dict(shape="generic", pre=False),
    "attn2": dict(shape="attn2", pre=False), "attn2_pre": dict(shape="attn2", pre=True),
    "resident": dict(shape="resident", pre=True, opts=dict(ATTN2_RES=2)),
    "xview": dict(shape="sources", pre=False, nsrc=2), "xview_pre": dict(shape="sources", pre=True, nsrc=2),
    "joint": dict(shape="sources", pre=False, nsrc=2, joint=True), "joint_pre": dict(shape="sources", pre=True, nsrc=2, joint=True),
    "short_causal": dict(shape="short", pre=False, causal=True),
    "ctx": dict(shape="ctx", pre=False, count=V.CTX_COUNT), "ctx_pre": dict(shape="ctx", pre=True, count=V.CTX_COUNT),
}


def expected_attn_kernel(route, r, d, Tq):
    if route == "generic":
        return "attn_kernel<4,"
    if route == "resident":
        return "attn2_kernel<40,resident,q32,fold>"
    if route == "short_causal":
        return f"attn_short_kernel<{d},causal>"
    if route.startswith("ctx"):
        return f"attn_ctx_kernel<{d},{'pre' if r['pre'] else 'scaled'}>"
    tag = attn2_route(d, Tq, xview=r.get("nsrc", 1) == 2 and not r.get("joint"), pre=r["pre"])
    assert tag.startswith("attn2_kernel<"), f"{route}: this shape must still reach attention2.hip, attn2_route says {tag}"
    return tag.replace(",self,", ",joint,") if r.get("joint") else tag


@functools.lru_cache(maxsize=None)
def attn_case(shape, pattern, dtype, pre, causal, count, nsrc, joint):
    """Inputs and the fp64 reference / bound of one case, computed once per (shape, pattern, type, form) and shared by the routes that use it."""
    B, H, Tq, Tk, d = V.ATTN_SHAPES[shape]
    q, k, v = V.attn_inputs(pattern, B, H, Tq, Tk, d, dtype, live=count)
    qk, qr = V.prescale(q, d) if pre else (q, q)
    if nsrc == 1:
        ref, inner = V.attn_ref(qr, k, v, H, d ** -0.5, dtype, causal=causal, count=count)
    else:
        ref, inner = V.attn_ref_sources(qr, k, v, H, d ** -0.5, dtype, lambda i: [(i // 6) * 6 + c for c in RING[i % 6]], joint)
    return qk, k, v, ref, V.attn_bound(ref, inner, dtype)


A_CASES = [(route, p) for route in ATTN_ROUTES for p in V.A_PATTERNS if not (route == "short_causal" and p == "A5")]


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("route,pattern", A_CASES, ids=[f"{r}-{p}" for r, p in A_CASES])
def test_attention_values(dev, route, pattern, dtype):
    """A1 block one-hot rows (margin >= 40 nats; all mass in the first tile for the first queries, in the last, partly masked tile for the last),
    A2 staircases that lift the row maximum by 3.9 / 4.1 / 12 log2 units per tile (just under / over A2_DEFER, a large step; ascending and
    descending), A3 logits at +-250 nats, A4 V outliers (a channel x1000, 1 % of the rows x100), A5 equal keys — on attention.hip, attention2.hip
    (plain, pre-scaled = FOLD, resident, two-source cross-view and joint), the causal short-sequence kernel and the device-count context kernel.
    Against B_attn (values_data), finite everywhere."""
    r = ATTN_ROUTES[route]
    B, H, Tq, Tk, d = V.ATTN_SHAPES[r["shape"]]
    nsrc, joint, causal, count = r.get("nsrc", 1), r.get("joint", False), r.get("causal", False), r.get("count")
    q, k, v, ref, bound = attn_case(r["shape"], pattern, dtype, r["pre"], causal, count, nsrc, joint)
    Cc = H * d
    if causal:
        vt = v.to(dev)                                                 # V row-major
    else:
        pad = 8 if count else 0
        vt = torch.full((B, Cc, PK.round_up(Tk, 8) + pad), NAN, dtype=dtype, device=dev)      # NaN in the kv pad
        vt[:, :, :Tk] = v.to(dev).transpose(1, 2)
    Ov = Guarded((B, Tq, Cc), Cc, 0, dtype, dev)
    kw = {}
    if nsrc == 2:
        kw = dict(kvmap=torch.tensor([(i // 6) * 6 + RING[i % 6][s] for i in range(B) for s in range(2)], dtype=torch.int32, device=dev), nsrc=2, joint=joint)
    if count:
        kw = dict(tk_dev=torch.tensor([count], dtype=torch.int32, device=dev))
    with L.options(**r.get("opts", {})):
        expect = expected_attn_kernel(route, r, d, Tq)
        O.run_ops([O.Attn(q.to(dev), k.to(dev), vt, Ov.view, heads=H, Tk=Tk, scale=d ** -0.5, q_prescaled=r["pre"], causal=causal, v_rowmajor=causal, **kw)])
        kern = last_kernel()
    torch.cuda.synchronize()
    assert kern.startswith(expect), (kern, expect)
    out = Ov.view.cpu()
    worst = V.ratio(out, ref, bound)
    log("A", pattern, route, dtype, worst, kernel=kern)
    assert torch.isfinite(out.float()).all(), "non-finite output"
    assert worst <= 1.0, f"{route} {pattern}: worst err / bound = {worst:.3f}"
    assert Ov.border_intact()


# --------------------------------------------------------------------------------------------------------------------------------------
# S: Fourier and timestep embeddings
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_fourier_embed_pixel_magnitudes(dev, dtype):
    """F = 4 on |x| up to 2000 (arguments up to 16000 rad): fp64 sin / cos of the fp32 product, u16 |ref| + 2^-21."""
    x = V.fourier_inputs()
    n, Pn, _ = x.shape
    Y = Guarded((n, Pn * 27), Pn * 27, 0, dtype, dev)
    O.run_ops([O.Fourier(x.to(dev), Y.view, 4)])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern == "fourier_kernel", kern
    ref, bound = V.fourier_ref(x, 4, dtype)
    worst = V.ratio(Y.view.cpu(), ref, bound)
    log("S", "fourier_2000", kern, dtype, worst)
    assert worst <= 1.0 and Y.border_intact(), worst


def test_timestep_embedding_at_the_ends_of_the_schedule(dev):
    """t in {0, 1, 999, 1000.5}, dim 320, against the fp64 formula at the atol 2e-4 of test_fourier_gather_timeemb."""
    t = torch.tensor(V.TIMESTEPS)
    te = torch.full((len(V.TIMESTEPS), 320), NAN, dtype=F32, device=dev)
    O.run_ops([O.TimeEmb(t.to(dev), te)])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern == "timeemb_kernel", kern
    err = (te.cpu().double() - V.timeemb_ref(t)).abs().max().item()
    parity_log("values:S:timeemb:timeemb_kernel:f32", worst_err_over_bound=err / 2e-4, max_err=err)
    assert err < 2e-4, err
