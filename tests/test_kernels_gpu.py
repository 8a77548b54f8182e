"""-m gpu: every HIP kernel behind the C-ABI vs a plain PyTorch fp32 reference of the same op.

Inputs are bf16-rounded first so the comparison isolates the kernel's own arithmetic
(fp32 accumulate, one bf16 rounding on store).  Tolerances follow xformers' bf16 table
(third_party/xformers/xformers/ops/fmha/common.py:209-219): atol 2e-2, rtol 5e-3 at unit scale;
we scale atol by the output magnitude.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from magicdrive_amd import _lib as L
from magicdrive_amd import ops as O
from magicdrive_amd import packing as PK

BF = torch.bfloat16


def rnd(*shape, scale=1.0, seed=0, dtype=BF, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


from helpers import close, rel_l2  # noqa: E402  (xformers table, every element; measured values logged)


def ws_buf(dev, mb=64):
    return torch.empty(mb * 1024 * 1024 // 4, dtype=torch.float32, device=dev)


@pytest.mark.parametrize("M,N,K,bias,res,f32out", [
    (8400, 320, 320, True, True, False),
    (2100, 640, 2560, True, False, False),
    (546, 1280, 1280, False, True, False),
    (168, 1280, 5120, True, True, False),     # auto split-K
    (50, 1280, 320, True, False, True),       # fp32 output, tiny M
    (777, 96, 136, True, False, False),       # ragged everything, BN=64
    (130, 20, 8, False, False, False),
])
def test_gemm(dev, M, N, K, bias, res, f32out):
    A = rnd(M, K, seed=1); W = rnd(N, K, scale=K ** -0.5, seed=2)
    b = rnd(N, seed=3, dtype=torch.float32) if bias else None
    R = rnd(M, N, seed=4, dtype=torch.float32 if f32out else BF) if res else None
    C = torch.full((M, N), float("nan"), dtype=torch.float32 if f32out else BF, device=dev)
    O.run_ops([O.Gemm(A, W, C, bias=b, R=R, ws=ws_buf(dev))])
    torch.cuda.synchronize()
    ref = A.float().cpu() @ W.float().cpu().T
    if bias: ref += b.cpu()
    if res: ref += R.float().cpu()
    close(C, ref, name=f"gemm {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,res,inplace", [(8200, 640, False, False), (9001, 100, True, False), (8333, 320, True, True), (16384, 1280, False, False)])
def test_gemm_weight_stationary(dev, M, N, res, inplace):
    """K = 320, M >= 8192 takes gemm_ws.hip (weights in registers, persistent M walk): ragged M, N not a multiple of the
    128-column tile, N % 8 != 0 (narrow epilogue), strided C view, residual aliased with C (in-place accumulate)."""
    K = 320
    A = rnd(M, K, seed=1); W = rnd(N, K, scale=K ** -0.5, seed=2); b = rnd(N, seed=3, dtype=torch.float32)
    Cbig = torch.full((M, N + 24), float("nan"), dtype=BF, device=dev)
    C = Cbig[:, 8:8 + N]
    R = None
    if res:
        R0 = rnd(M, N, seed=4)
        if inplace: C.copy_(R0); R = C
        else: R = R0
    O.run_ops([O.Gemm(A, W, C, bias=b, R=R, ws=ws_buf(dev))])
    torch.cuda.synchronize()
    ref = A.float().cpu() @ W.float().cpu().T + b.cpu()
    if res: ref += R0.float().cpu()
    close(C, ref, name=f"ws gemm {M}x{N}")
    assert torch.isnan(Cbig[:, :8].float()).all() and torch.isnan(Cbig[:, 8 + N:].float()).all(), "wrote outside the C view"


@pytest.mark.parametrize("Bv,T", [(6, 1400), (7, 1176)])
def test_gemm_fused_qkv_transposed_v(dev, Bv, T):
    """Fused q/k/v projection (MdxGemmDesc.Vt): columns [0, 2C) to C row-major, columns [2C, 3C) transposed to V^T[view][channel][token]
    — what the attention kernel consumes; ragged last M tile, views that do not align with the 128-row tiles."""
    Cc = 320
    M = Bv * T
    X = rnd(M, Cc, seed=1); W = rnd(3 * Cc, Cc, scale=Cc ** -0.5, seed=2)
    qk = torch.full((M, 2 * Cc), float("nan"), dtype=BF, device=dev)
    Vt = torch.full((Bv, Cc, T), float("nan"), dtype=BF, device=dev)
    O.run_ops([O.Gemm(X, W, qk, Vt=Vt, vt_from=2 * Cc, vt_T=T)])
    torch.cuda.synchronize()
    ref = X.float().cpu() @ W.float().cpu().T
    close(qk, ref[:, :2 * Cc], name="fused qk")
    close(Vt, ref[:, 2 * Cc:].reshape(Bv, T, Cc).transpose(1, 2), name="fused V^T")
    with pytest.raises(L.MdxError):          # not expressible outside the weight-stationary kernel: loud, no fallback
        O.run_ops([O.Gemm(rnd(M, 640, seed=3), rnd(3 * Cc, 640, seed=4), qk, Vt=Vt, vt_from=2 * Cc, vt_T=T)])


def ln_fold(W, gamma, beta, dtype):
    """LayerNorm affine folded into the Linear that follows it (engine.PackedNet.ln_lin): W' (16-bit), b' = W beta, column sums of W'."""
    Wp = (W * gamma[None, :]).to(dtype)
    return Wp, (W @ beta).float(), Wp.float().sum(1)


def ln_ref(x, Wp, b, eps=1e-5, stored=False):
    """stored: the route under test keeps a 16-bit normalised copy (ln_scratch) — the reference rounds it too, as for any LayerNorm -> GEMM pair."""
    xf = x.float().cpu()
    xh = (xf - xf.mean(-1, keepdim=True)) * (xf.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    if stored: xh = xh.to(x.dtype).float()
    return xh @ Wp.float().cpu().T + b.cpu()


@pytest.mark.parametrize("M,N,res,route", [(8400, 320, False, "ws"), (9001, 640, True, "ws"), (8333, 328, False, "ws"), (16384, 960, False, "ws"),
                                           (2100, 320, False, "small"), (8400, 320, True, "no_ws"), (8400, 640, False, "xl")])
def test_gemm_fused_layernorm(dev, M, N, res, route):
    """LayerNorm fused into the K = 320 projection (MdxGemmDesc.ln_eps): raw rows in, statistics taken inside gemm_ws.hip from the slabs it
    streams, rstd (acc - mean csum) + bias in the epilogue — against LayerNorm -> Linear in fp32 on the same 16-bit W'.  Rows with a large
    common offset exercise the one-pass variance; every route that cannot fuse (small M, weight-stationary kernel off, XL forced) must give
    the same result through ln_scratch."""
    K = 320
    x = rnd(M, K, scale=1.5, seed=1).float() + 0.7
    x[::7] += 12.0                                                   # |mean| = 8 sigma on every 7th row
    x = x.to(BF)
    W = rnd(N, K, scale=K ** -0.5, seed=2, dtype=torch.float32); gamma = 1.0 + rnd(K, scale=0.3, seed=5, dtype=torch.float32)
    beta = rnd(K, scale=0.3, seed=6, dtype=torch.float32)
    Wp, b, cs = ln_fold(W, gamma, beta, BF)
    R = rnd(M, N, seed=4) if res else None
    C = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    scratch = torch.full((M, K), float("nan"), dtype=BF, device=dev)
    opts = {"ws": {}, "small": {}, "no_ws": {"GEMM_WS": 0}, "xl": {"GEMM_XL": 2, "XL_K320": 1}}[route]
    with L.options(**opts):
        O.run_ops([O.Gemm(x, Wp, C, bias=b, R=R, ln_eps=1e-5, ln_csum=cs, ln_scratch=scratch, ws=ws_buf(dev))])
        kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    fused = route == "ws"
    assert (kern == "gemm_ws_kernel<plain,ln>") == fused, kern
    assert torch.isnan(scratch.float()).all() == fused, "the fused route must not touch ln_scratch; the others must fill it"
    ref = ln_ref(x, Wp, b, stored=not fused)
    if res: ref += R.float().cpu()
    close(C, ref, name=f"ln+gemm {M}x{N} {route}")
    if not fused:
        with pytest.raises(L.MdxError):                              # no scratch, no silent un-normalised product
            with L.options(**opts):
                O.run_ops([O.Gemm(x, Wp, C, bias=b, R=R, ln_eps=1e-5, ln_csum=cs, ws=ws_buf(dev))])


def test_gemm_fused_layernorm_large_common_offset_routes_agree(dev):
    """the fused route takes a ONE-pass variance E[x^2] - mean^2 in fp32 and forms rstd (acc - mean csum); both cancel when
    |mean| >> sigma, while the ln_scratch routes normalise with the two-pass layernorm_kernel first.  Rows with |mean| / sigma = 100 at
    16-bit magnitudes of ~1e3 (hidden states with an outlier offset) bound the routing-dependent drift: fp32 sums of 320 squares of
    ~1e6 carry ~1 % of the variance as rounding error, i.e. <= 0.5 % in rstd — the size of one bf16 rounding.  Both routes vs the fp32
    reference, and against each other."""
    M, K, N = 8400, 320, 320
    x = (rnd(M, K, scale=10.0, seed=1).float() + 1000.0).to(BF)
    W = rnd(N, K, scale=K ** -0.5, seed=2, dtype=torch.float32); gamma = 1.0 + rnd(K, scale=0.3, seed=5, dtype=torch.float32)
    beta = rnd(K, scale=0.3, seed=6, dtype=torch.float32)
    Wp, b, cs = ln_fold(W, gamma, beta, BF)
    outs = {}
    for route, opts in (("ws", {}), ("no_ws", {"GEMM_WS": 0})):
        C = torch.empty(M, N, dtype=BF, device=dev)
        scratch = torch.empty(M, K, dtype=BF, device=dev)
        with L.options(**opts):
            O.run_ops([O.Gemm(x, Wp, C, bias=b, ln_eps=1e-5, ln_csum=cs, ln_scratch=scratch, ws=ws_buf(dev))])
            kern = (L.lib().mdx_last_kernel() or b"").decode()
        assert (kern == "gemm_ws_kernel<plain,ln>") == (route == "ws"), kern
        outs[route] = C.float().cpu()
    torch.cuda.synchronize()
    ref = ln_ref(x, Wp, b)
    e_ws, e_scr = rel_l2(outs["ws"], ref), rel_l2(outs["no_ws"], ln_ref(x, Wp, b, stored=True))
    drift = rel_l2(outs["ws"], outs["no_ws"])
    from helpers import parity_log
    parity_log("ln_fused_large_common_offset", fused_vs_fp32=e_ws, scratch_route_vs_fp32=e_scr, fused_vs_scratch_route=drift)
    print(f"[fused LayerNorm, |mean| = 100 sigma] fused vs fp32 {e_ws:.4f}, scratch route vs fp32 {e_scr:.4f}, fused vs scratch route {drift:.4f}")
    assert e_ws < 2e-2 and e_scr < 1e-2 and drift < 2e-2, (e_ws, e_scr, drift)


@pytest.mark.parametrize("Bv,T", [(6, 1400), (7, 1176)])
def test_gemm_fused_layernorm_qkv_transposed_v(dev, Bv, T):
    """norm1 -> to_q / to_k / to_v as the engine emits it at level 0: LayerNorm fused, q/k row-major, V transposed, bias = W beta on all three."""
    Cc = 320
    M = Bv * T
    x = (rnd(M, Cc, scale=1.3, seed=1).float() - 0.4).to(BF)
    W = rnd(3 * Cc, Cc, scale=Cc ** -0.5, seed=2, dtype=torch.float32); gamma = 1.0 + rnd(Cc, scale=0.3, seed=5, dtype=torch.float32)
    beta = rnd(Cc, scale=0.3, seed=6, dtype=torch.float32)
    Wp, b, cs = ln_fold(W, gamma, beta, BF)
    qk = torch.full((M, 2 * Cc), float("nan"), dtype=BF, device=dev)
    Vt = torch.full((Bv, Cc, T), float("nan"), dtype=BF, device=dev)
    O.run_ops([O.Gemm(x, Wp, qk, bias=b, Vt=Vt, vt_from=2 * Cc, vt_T=T, ln_eps=1e-5, ln_csum=cs)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern == "gemm_ws_kernel<vT,ln>", kern
    ref = ln_ref(x, Wp, b)
    close(qk, ref[:, :2 * Cc], name="ln + fused qk")
    close(Vt, ref[:, 2 * Cc:].reshape(Bv, T, Cc).transpose(1, 2), name="ln + fused V^T")


def rowstat_ref(Cmat, parts_cols):
    """(sum, sum of squares) of the STORED rows per column part, fp64 on the host."""
    cf = Cmat.double().cpu()
    return torch.stack([torch.stack([cf[:, a:b].sum(1), (cf[:, a:b] ** 2).sum(1)], -1) for a, b in parts_cols])


@pytest.mark.parametrize("M,N,res,parts,route", [(8400, 320, True, 3, "ws"), (9001, 320, False, 4, "ws"), (8333, 328, True, 3, "ws"), (16384, 640, True, 5, "ws"),
                                                 (2100, 320, True, 3, "small"), (8400, 320, True, 3, "no_ws"), (8400, 320, False, 2, "few_parts")])
def test_gemm_row_statistics_out(dev, M, N, res, parts, route):
    """MdxGemmDesc.rowstat_out (ABI 9): the projection that writes a LayerNorm's input also leaves (sum, sum of squares) of every STORED row —
    rounded, residual added — per 128-column tile of the weight-stationary kernel's store phase (a DPP row-rotation tree over the 16 lanes of
    a row segment), unused parts zero; every other route (small M, kernel off, fewer parts than tiles) runs rowstat_kernel over the finished C
    (part 0 = whole row).  Against fp64 sums of the stored values; bit-identical across runs (fixed summation order)."""
    K = 320
    A = rnd(M, K, seed=1); W = rnd(N, K, scale=K ** -0.5, seed=2); b = rnd(N, seed=3, dtype=torch.float32)
    R = (rnd(M, N, seed=4).float() * 2 + 3).to(BF) if res else None               # a common offset: the sums are not tiny
    C = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    opts = {"no_ws": {"GEMM_WS": 0}}.get(route, {})
    outs = []
    for _ in range(2):
        st = torch.full((parts, M, 2), float("nan"), dtype=torch.float32, device=dev)
        with L.options(**opts):
            O.run_ops([O.Gemm(A, W, C, bias=b, R=R, rowstat=st, ws=ws_buf(dev))])
            kern = (L.lib().mdx_last_kernel() or b"").decode()
        torch.cuda.synchronize()
        outs.append(st.clone())
    fused = route == "ws"
    assert (kern == "gemm_ws_kernel<plain,rs>") == fused and (fused or kern == "rowstat_kernel"), kern
    assert torch.equal(outs[0], outs[1]), "row statistics differ between two runs"
    ref = A.float().cpu() @ W.float().cpu().T + b.cpu()
    if res: ref += R.float().cpu()
    close(C, ref, name=f"gemm+rowstat {M}x{N} {route}")
    st = outs[0].double().cpu()
    nt = (N + 127) // 128
    if fused:
        want = rowstat_ref(C, [(128 * k, min(N, 128 * k + 128)) for k in range(nt)])
        assert (st[nt:] == 0).all(), "parts beyond the N-tiles must be zero"
        got = st[:nt]
    else:
        want = rowstat_ref(C, [(0, N)])
        assert (st[1:] == 0).all()
        got = st[:1]
    err = ((got - want).abs() / (want.abs() + 1.0)).max().item()
    assert err < 2e-5, err                                              # fp32 sums of <= 128 (or N) 16-bit values
    tot = rowstat_ref(C, [(0, N)])[0]
    assert ((st.sum(0) - tot).abs() / (tot.abs() + 1.0)).max().item() < 2e-5        # what a consumer does: add all parts


def _ln_stats_of(x, parts, dev):
    """Row statistics as a producer would have left them: the row split into `parts` column ranges (the last ones may be empty / zero)."""
    xf = x.float()
    K = xf.shape[1]
    st = torch.zeros(parts, xf.shape[0], 2, dtype=torch.float32, device=dev)
    edges = [0, 128, 256, K] if parts >= 3 else [0, K]
    for k in range(len(edges) - 1):
        st[k, :, 0] = xf[:, edges[k]:edges[k + 1]].sum(1)
        st[k, :, 1] = (xf[:, edges[k]:edges[k + 1]] ** 2).sum(1)
    return st


@pytest.mark.parametrize("M,N,res,parts", [(8400, 320, False, 3), (9001, 640, True, 3), (8333, 328, False, 4), (16384, 960, False, 1)])
def test_gemm_fused_layernorm_given_statistics(dev, M, N, res, parts):
    """MdxGemmDesc.ln_stats: the fused LayerNorm takes mean / rstd from the producer's (sum, sum of squares) parts — hand-counted loads behind
    the first slab's barrier, published in LDS two barriers before the epilogue — instead of summing the streamed rows in every N-tile's
    workgroup.  Same reference and tolerance as the in-kernel form; the scratch buffer stays untouched."""
    K = 320
    x = rnd(M, K, scale=1.5, seed=1).float() + 0.7
    x[::7] += 12.0
    x = x.to(BF)
    W = rnd(N, K, scale=K ** -0.5, seed=2, dtype=torch.float32); gamma = 1.0 + rnd(K, scale=0.3, seed=5, dtype=torch.float32)
    beta = rnd(K, scale=0.3, seed=6, dtype=torch.float32)
    Wp, b, cs = ln_fold(W, gamma, beta, BF)
    R = rnd(M, N, seed=4) if res else None
    C = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    scratch = torch.full((M, K), float("nan"), dtype=BF, device=dev)
    O.run_ops([O.Gemm(x, Wp, C, bias=b, R=R, ln_eps=1e-5, ln_csum=cs, ln_scratch=scratch, ln_stats=_ln_stats_of(x, parts, dev), ws=ws_buf(dev))])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern == "gemm_ws_kernel<plain,lns>" and torch.isnan(scratch.float()).all(), kern
    ref = ln_ref(x, Wp, b)
    if res: ref += R.float().cpu()
    close(C, ref, name=f"ln(stats)+gemm {M}x{N}")
    # a route that cannot fuse ignores the statistics and normalises into the scratch buffer: same result up to the rounding of the copy
    with L.options(GEMM_WS=0):
        O.run_ops([O.Gemm(x, Wp, C, bias=b, R=R, ln_eps=1e-5, ln_csum=cs, ln_scratch=scratch, ln_stats=_ln_stats_of(x, parts, dev), ws=ws_buf(dev))])
    torch.cuda.synchronize()
    ref2 = ln_ref(x, Wp, b, stored=True)
    if res: ref2 += R.float().cpu()
    close(C, ref2, name=f"ln(stats ignored)+gemm {M}x{N}")


@pytest.mark.parametrize("Bv,T", [(6, 1400), (7, 1176)])
def test_gemm_fused_layernorm_given_statistics_qkv(dev, Bv, T):
    """norm1 -> to_q / to_k / to_v with the producer's statistics: the q/k launch and the transposed-V launch both read them."""
    Cc = 320
    M = Bv * T
    x = (rnd(M, Cc, scale=1.3, seed=1).float() - 0.4).to(BF)
    W = rnd(3 * Cc, Cc, scale=Cc ** -0.5, seed=2, dtype=torch.float32); gamma = 1.0 + rnd(Cc, scale=0.3, seed=5, dtype=torch.float32)
    beta = rnd(Cc, scale=0.3, seed=6, dtype=torch.float32)
    Wp, b, cs = ln_fold(W, gamma, beta, BF)
    qk = torch.full((M, 2 * Cc), float("nan"), dtype=BF, device=dev)
    Vt = torch.full((Bv, Cc, T), float("nan"), dtype=BF, device=dev)
    O.run_ops([O.Gemm(x, Wp, qk, bias=b, Vt=Vt, vt_from=2 * Cc, vt_T=T, ln_eps=1e-5, ln_csum=cs, ln_stats=_ln_stats_of(x, 3, dev))])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern == "gemm_ws_kernel<vT,lns>", kern
    ref = ln_ref(x, Wp, b)
    close(qk, ref[:, :2 * Cc], name="ln(stats) + fused qk")
    close(Vt, ref[:, 2 * Cc:].reshape(Bv, T, Cc).transpose(1, 2), name="ln(stats) + fused V^T")


@pytest.mark.parametrize("M,F_", [(8250, 320), (8400, 1280)])
def test_gemm_fused_layernorm_geglu_given_statistics(dev, M, F_):
    """norm3 -> ff.net.0 folded (round 6): with the producer's row statistics the GEGLU epilogue applies rstd (acc - mean csum) + bias to the value
    and the gate columns; the scratch buffer stays untouched.  Without statistics the same descriptor still goes through the scratch route."""
    K = 320
    x = (rnd(M, K, scale=1.4, seed=1).float() + 0.5).to(BF)
    W = rnd(2 * F_, K, scale=K ** -0.5, seed=2, dtype=torch.float32, dev="cpu"); b = rnd(2 * F_, seed=3, dtype=torch.float32, dev="cpu")
    gamma = 1.0 + rnd(K, scale=0.3, seed=5, dtype=torch.float32, dev="cpu"); beta = rnd(K, scale=0.3, seed=6, dtype=torch.float32, dev="cpu")
    Wf, bf_ = W * gamma[None, :], b + W @ beta
    Wp, bp = PK.pack_geglu(Wf, bf_, BF)
    C = torch.zeros(M, F_, dtype=BF, device=dev)
    scratch = torch.full((M, K), float("nan"), dtype=BF, device=dev)
    O.run_ops([O.Gemm(x, Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU, ln_eps=1e-5, ln_csum=Wp.float().sum(1).to(dev), ln_scratch=scratch,
                      ln_stats=_ln_stats_of(x, 3, dev), ws=ws_buf(dev))])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern == "gemm_ws_kernel<geglu,lns>" and torch.isnan(scratch.float()).all(), kern
    h, g = ln_ref(x, Wf.to(BF), bf_).chunk(2, dim=-1)
    close(C, h * F.gelu(g), name=f"ln(stats)+geglu {M}x{F_}")


def test_gemm_fused_layernorm_geglu_goes_through_scratch(dev):
    """ln_eps on a GEGLU projection (norm3 -> ff.net.0) WITHOUT producer statistics is accepted by the C-ABI but not fused (gemm_ws.hip: in-kernel
    sums in 20 N-tiles measured slower than the LayerNorm pass): the rows are normalised into ln_scratch, then the ordinary GEGLU kernel runs on
    the folded weights."""
    M, F_, K = 8250, 320, 320
    x = (rnd(M, K, scale=1.4, seed=1).float() + 0.5).to(BF)
    W = rnd(2 * F_, K, scale=K ** -0.5, seed=2, dtype=torch.float32, dev="cpu"); b = rnd(2 * F_, seed=3, dtype=torch.float32, dev="cpu")
    gamma = 1.0 + rnd(K, scale=0.3, seed=5, dtype=torch.float32, dev="cpu"); beta = rnd(K, scale=0.3, seed=6, dtype=torch.float32, dev="cpu")
    Wf, bf_ = W * gamma[None, :], b + W @ beta
    Wp, bp = PK.pack_geglu(Wf, bf_, BF)
    C = torch.zeros(M, F_, dtype=BF, device=dev)
    scratch = torch.full((M, K), float("nan"), dtype=BF, device=dev)
    O.run_ops([O.Gemm(x, Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU, ln_eps=1e-5, ln_csum=Wp.float().sum(1).to(dev), ln_scratch=scratch, ws=ws_buf(dev))])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern == "gemm_ws_kernel<geglu>" and not torch.isnan(scratch.float()).any(), kern
    h, g = ln_ref(x, Wf.to(BF), bf_, stored=True).chunk(2, dim=-1)
    close(C, h * F.gelu(g), name="ln(scratch)+geglu")


def test_gemm_weight_stationary_geglu_ragged(dev):
    M, F_, K = 8250, 320, 320
    A = rnd(M, K, seed=1); W = rnd(2 * F_, K, scale=K ** -0.5, seed=2, dtype=torch.float32, dev="cpu")
    b = rnd(2 * F_, seed=3, dtype=torch.float32, dev="cpu")
    Wp, bp = PK.pack_geglu(W, b, BF)
    C = torch.zeros(M, F_, dtype=BF, device=dev)
    O.run_ops([O.Gemm(A, Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU)])
    torch.cuda.synchronize()
    h, g = (A.float().cpu() @ W.to(BF).float().T + b).chunk(2, dim=-1)
    close(C, h * F.gelu(g), name="ws geglu ragged")


def test_gemm_forced_splitk_matches(dev):
    M, N, K = 546, 640, 5760
    A = rnd(M, K, seed=1); W = rnd(N, K, scale=K ** -0.5, seed=2); b = rnd(N, seed=3, dtype=torch.float32)
    C1 = torch.zeros(M, N, dtype=BF, device=dev); C2 = torch.zeros_like(C1)
    O.run_ops([O.Gemm(A, W, C1, bias=b, splitk=1), O.Gemm(A, W, C2, bias=b, splitk=6, ws=ws_buf(dev))])
    torch.cuda.synchronize()
    ref = A.float().cpu() @ W.float().cpu().T + b.cpu()
    close(C1, ref, name="splitk=1"); close(C2, ref, name="splitk=6")


@pytest.mark.parametrize("sk", [2, 3, 5, 8, 13])
@pytest.mark.parametrize("kind", ["plain", "temb_res", "silu", "geglu"])
def test_splitk_reduce_epilogues(dev, sk, kind):
    """splitk_reduce_kernel (round 6: every load requested before the first is consumed, slabs four in flight through clamped addresses) with each epilogue it
    applies, at slab counts on both sides of a multiple of four — against the fp32 reference, bit-identical to a second run, and within rounding of the
    one-pass (splitk = 1) launch, whose reduction order differs only in where the k range is cut."""
    M, K = 168, 2560
    A = rnd(M, K, seed=1)
    ws = ws_buf(dev)
    if kind == "geglu":
        F_ = 640
        W = rnd(2 * F_, K, scale=K ** -0.5, seed=2, dtype=torch.float32, dev="cpu"); b = rnd(2 * F_, seed=3, dtype=torch.float32, dev="cpu")
        Wp, bp = PK.pack_geglu(W, b, BF)
        mk = lambda C, s_: O.Gemm(A, Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU, splitk=s_, ws=ws)
        h, g = (A.float().cpu() @ W.to(BF).float().T + b).chunk(2, dim=-1)
        ref = h * F.gelu(g); N = F_
    else:
        N = 648                                                     # N % 8 != 0: the narrow-store layout of the fp32 slabs' consumer
        W = rnd(N, K, scale=K ** -0.5, seed=2); b = rnd(N, seed=3, dtype=torch.float32)
        R = rnd(M, N, seed=4) if kind == "temb_res" else None
        tb = rnd(3, 6, N, seed=5, dtype=torch.float32) if kind == "temb_res" else None      # [step][image][N]; rows_per_b = 28
        sel = torch.tensor([2], dtype=torch.int32, device=dev) if kind == "temb_res" else None
        epi = 2 if kind == "silu" else 0
        mk = lambda C, s_: O.Gemm(A, W, C, bias=b, R=R, temb=tb, sel=sel, temb_sel_stride=6 * N if tb is not None else 0, temb_b_stride=N if tb is not None else 0,
                                  rows_per_b=28, epilogue=epi, splitk=s_, ws=ws)
        ref = A.float().cpu() @ W.float().cpu().T + b.cpu()
        if tb is not None: ref = ref + tb[2].cpu().repeat_interleave(28, dim=0)
        if epi == 2: ref = F.silu(ref)
        if R is not None: ref = ref + R.float().cpu()
    outs = []
    for s_ in (sk, sk, 1):
        C = torch.full((M, N), float("nan"), dtype=BF, device=dev)
        O.run_ops([mk(C, s_)])
        torch.cuda.synchronize()
        outs.append(C)
    close(outs[0], ref, name=f"split-K {sk} {kind}")
    assert torch.equal(outs[0], outs[1]), "split-K reduce is not deterministic"
    assert rel_l2(outs[0], outs[2]) < 4e-3, rel_l2(outs[0], outs[2])


def test_gemm_strided_views_and_temb(dev):
    # A and C are column slices of wider buffers; temb row chosen by a device-side selector
    M, N, K = 2 * 350, 640, 320
    Abig = rnd(M, 2 * K, seed=5); Cbig = torch.zeros(M, 3 * N, dtype=BF, device=dev)
    W = rnd(N, K, scale=K ** -0.5, seed=6)
    temb = rnd(5, 2, N, seed=7, dtype=torch.float32)      # [sel][b][N]
    sel = torch.tensor([3], dtype=torch.int32, device=dev)
    A = Abig[:, K:]; C = Cbig[:, N:2 * N]
    O.run_ops([O.Gemm(A, W, C, temb=temb, sel=sel, temb_sel_stride=2 * N, temb_b_stride=N, rows_per_b=350)])
    torch.cuda.synchronize()
    ref = A.float().cpu() @ W.float().cpu().T + temb[3].cpu().repeat_interleave(350, 0)
    close(C, ref, name="gemm strided+temb")
    assert Cbig[:, :N].abs().max().item() == 0 and Cbig[:, 2 * N:].abs().max().item() == 0


@pytest.mark.parametrize("M,F_,K", [(2100, 2560, 640), (8400, 1280, 320), (546, 5120, 1280), (100, 128, 32)])
def test_gemm_geglu(dev, M, F_, K):
    A = rnd(M, K, seed=1); W = rnd(2 * F_, K, scale=K ** -0.5, seed=2, dtype=torch.float32, dev="cpu")
    b = rnd(2 * F_, seed=3, dtype=torch.float32, dev="cpu")
    Wp, bp = PK.pack_geglu(W, b, BF)
    C = torch.zeros(M, F_, dtype=BF, device=dev)
    O.run_ops([O.Gemm(A, Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU, ws=ws_buf(dev))])
    torch.cuda.synchronize()
    proj = A.float().cpu() @ W.to(BF).float().T + b
    h, g = proj.chunk(2, dim=-1)
    close(C, h * F.gelu(g), name="geglu")


@pytest.mark.parametrize("M,F_,K", [(8400, 1280, 320), (2100, 2560, 640)])
def test_gemm_geglu_large_gates(dev, M, F_, K):
    """The erf of the GEGLU epilogues is a degree-8 polynomial clamped at |z| = 3 (csrc/common.h, |error| <= 2.7e-5 against an exact erf): gates far out in
    both tails (|g| up to ~12, where the clamp acts and gelu(g) is g or 0 to rounding) must still sit inside the storage type's table — this test also
    runs in the fp16 build (tests/test_fp16_gpu.py), whose table is 5x tighter.  Reference: fp64 x * gelu(g) with the exact erf."""
    A = rnd(M, K, seed=1); W = rnd(2 * F_, K, scale=K ** -0.5, seed=2, dtype=torch.float32, dev="cpu")
    b = rnd(2 * F_, seed=3, dtype=torch.float32, dev="cpu")
    W[F_:] *= 16.0; b[F_:] *= 4.0                              # the gate half: std ~8 instead of ~0.5
    Wp, bp = PK.pack_geglu(W, b, BF)
    C = torch.zeros(M, F_, dtype=BF, device=dev)
    O.run_ops([O.Gemm(A, Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU, ws=ws_buf(dev))])
    torch.cuda.synchronize()
    proj = A.double().cpu() @ W.to(BF).double().T + b.double()
    h, g = proj.chunk(2, dim=-1)
    assert (g.abs() > 4).float().mean() > 0.5 and g.abs().max() > 20
    close(C, (h * F.gelu(g)).float(), name="geglu large gates")


@pytest.mark.parametrize("Bt,T,Cc", [(6, 1400, 320), (6, 350, 640), (3, 91, 1280), (2, 28, 64)])
def test_gemm_batched_vt(dev, Bt, T, Cc):
    # V^T[b] = Wv @ X[b]^T into a kv-padded buffer
    ldv = PK.round_up(T, 8)
    X = rnd(Bt, T, Cc, seed=1); Wv = rnd(Cc, Cc, scale=Cc ** -0.5, seed=2)
    Vt = torch.zeros(Bt, Cc, ldv, dtype=BF, device=dev)
    O.run_ops([O.Gemm(Wv, X, Vt[:, :, :T])])
    torch.cuda.synchronize()
    ref = torch.einsum("ck,btk->bct", Wv.float().cpu(), X.float().cpu())
    close(Vt[:, :, :T], ref, name="batched V^T")
    assert Vt[:, :, T:].abs().max().item() == 0 if ldv > T else True


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,pad,res,temb", [
    (2, 28, 50, 320, 320, 3, (1, 1), (1, 1), True, True),
    (2, 28, 50, 320, 320, 3, (2, 2), (1, 1), False, False),
    (6, 4, 7, 1280, 1280, 3, (1, 1), (1, 1), True, True),        # split-K regime
    (3, 7, 13, 2560, 1280, 3, (1, 1), (1, 1), False, True),
    (1, 40, 40, 8, 16, 3, (1, 1), (1, 1), False, False),
    (1, 41, 40, 16, 32, 3, (2, 2), (2, 1), False, False),        # map-encoder style asymmetric pad
    (1, 22, 20, 96, 256, 3, (2, 1), (2, 1), False, False),
    (2, 14, 25, 640, 640, 1, (1, 1), (0, 0), True, False),       # 1x1
    (4, 28, 50, 320, 320, 3, (1, 1), (1, 1), True, True),        # M >= 4096
    (13, 14, 25, 640, 192, 3, (1, 1), (1, 1), False, True),      # tiles straddle images (350 px each), ragged M and N
    (48, 7, 13, 128, 320, 3, (1, 1), (1, 1), True, False),       # 91-pixel images: a 128-row tile covers 2-3 of them
])
def test_conv_mfma(dev, B, H, W, Cin, Cout, k, stride, pad, res, temb):
    x = rnd(B, H, W, Cin, seed=1)
    w = rnd(Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5, seed=2, dtype=torch.float32, dev="cpu")
    b = rnd(Cout, seed=3, dtype=torch.float32)
    Ho = (H + 2 * pad[0] - k) // stride[0] + 1; Wo = (W + 2 * pad[1] - k) // stride[1] + 1
    y = torch.zeros(B, Ho, Wo, Cout, dtype=BF, device=dev)
    R = rnd(B, Ho, Wo, Cout, seed=4) if res else None
    tb = rnd(B, Cout, seed=5, dtype=torch.float32) if temb else None
    O.run_ops([O.Conv(x, PK.pack_conv_weight(w, BF).to(dev), y, bias=b, R=R, temb=tb, temb_b_stride=Cout if temb else 0,
                      stride=stride, pad=pad, ws=ws_buf(dev))])
    torch.cuda.synchronize()
    ref = F.conv2d(x.float().cpu().permute(0, 3, 1, 2), w.to(BF).float(), b.cpu(), stride=stride, padding=pad)
    if temb: ref += tb.cpu()[:, :, None, None]
    ref = ref.permute(0, 2, 3, 1)
    if res: ref = ref + R.float().cpu()
    close(y, ref, name="conv")


def test_conv_silu_epilogue(dev):
    x = rnd(1, 20, 20, 16, seed=1)
    w = rnd(16, 16, 3, 3, scale=0.1, seed=2, dtype=torch.float32, dev="cpu"); b = rnd(16, seed=3, dtype=torch.float32)
    y = torch.zeros(1, 20, 20, 16, dtype=BF, device=dev)
    O.run_ops([O.Conv(x, PK.pack_conv_weight(w, BF).to(dev), y, bias=b, epilogue=L.EPI_SILU)])
    torch.cuda.synchronize()
    ref = F.silu(F.conv2d(x.float().cpu().permute(0, 3, 1, 2), w.to(BF).float(), b.cpu(), padding=1)).permute(0, 2, 3, 1)
    close(y, ref, name="conv+silu")


@pytest.mark.parametrize("case", ["conv_in", "conv_out", "linear189", "map_in"])
def test_conv_direct(dev, case):
    if case == "conv_in":
        B, H, W, Cin, Cout, k, xf, yf = 2, 28, 50, 4, 320, 3, True, False
    elif case == "conv_out":
        B, H, W, Cin, Cout, k, xf, yf = 2, 28, 50, 320, 4, 3, False, True
    elif case == "linear189":
        B, H, W, Cin, Cout, k, xf, yf = 12, 1, 1, 189, 768, 1, False, False
    else:
        B, H, W, Cin, Cout, k, xf, yf = 1, 30, 30, 8, 16, 3, False, False
    x = rnd(B, H, W, Cin, seed=1, dtype=torch.float32 if xf else BF)
    w = rnd(Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5, seed=2, dtype=torch.float32, dev="cpu"); b = rnd(Cout, seed=3, dtype=torch.float32)
    y = torch.zeros(B, H, W, Cout, dtype=torch.float32 if yf else BF, device=dev)
    pad = (k // 2, k // 2)
    O.run_ops([O.Conv(x, PK.pack_conv_weight(w, BF).to(dev), y, bias=b, pad=pad, direct=True)])
    torch.cuda.synchronize()
    ref = F.conv2d(x.float().cpu().permute(0, 3, 1, 2), w.to(BF).float(), b.cpu(), padding=pad).permute(0, 2, 3, 1)
    close(y, ref, name=case)


@pytest.mark.parametrize("B,H,W,Cin", [(48, 28, 50, 320), (47, 28, 50, 320), (24, 54, 96, 320), (64, 28, 50, 128)])
def test_conv_out_weight_stationary(dev, B, H, W, Cin):
    """conv_out at sampler batch sizes (M >= 65536 pixels) runs the weight-stationary K-parallel kernel (round 4: weights in registers,
    16 pixels per wave, packed dot products): vs F.conv2d in fp32, fp32 output like the sampler's eps; 47 views: a wave whose pixel run
    crosses the end of the tensor; Cin = 128: lanes without a chunk.  The two routes agree to fp32 summation order."""
    Cout, k = 4, 3
    x = rnd(B, H, W, Cin, seed=1)
    w = rnd(Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5, seed=2, dtype=torch.float32, dev="cpu"); b = rnd(Cout, seed=3, dtype=torch.float32)
    wp = PK.pack_conv_weight(w, BF).to(dev)
    y = torch.full((B, H, W, Cout), float("nan"), dtype=torch.float32, device=dev)
    O.run_ops([O.Conv(x, wp, y, bias=b, pad=(1, 1), direct=True)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    assert kern == "conv_direct_kpar_ws_kernel", kern
    y0 = torch.full_like(y, float("nan"))
    with L.options(CONV_OUT_WS=0):
        O.run_ops([O.Conv(x, wp, y0, bias=b, pad=(1, 1), direct=True)])
        assert (L.lib().mdx_last_kernel() or b"").decode() == "conv_direct_kpar_kernel"
    torch.cuda.synchronize()
    ref = F.conv2d(x.float().cpu().permute(0, 3, 1, 2), w.to(BF).float(), b.cpu(), padding=1).permute(0, 2, 3, 1)
    assert rel_l2(y, ref) < 2e-5 and rel_l2(y0, ref) < 2e-5, (rel_l2(y, ref), rel_l2(y0, ref))
    assert (y.cpu() - ref).abs().max() < 1e-4


def ref_attention(q, k, v, heads, scale):
    # xformers tests/test_mem_eff_attention.py:214-264 semantics (BMHK), fp32
    B, Tq, Cc = q.shape
    d = Cc // heads
    qh = q.view(B, Tq, heads, d).transpose(1, 2)
    kh = k.view(k.shape[0], -1, heads, d).transpose(1, 2)
    vh = v.view(v.shape[0], -1, heads, d).transpose(1, 2)
    att = (qh @ kh.transpose(-1, -2) * scale).softmax(-1)
    return (att @ vh).transpose(1, 2).reshape(B, Tq, Cc)


@pytest.mark.parametrize("B,heads,Tq,Tk,d", [
    (6, 8, 1400, 1400, 40), (6, 8, 350, 350, 80), (6, 8, 91, 91, 160), (6, 8, 28, 28, 160),
    (6, 8, 1400, 110, 40), (6, 8, 350, 78, 80), (3, 8, 91, 110, 160),
    (2, 2, 100, 70, 16), (2, 4, 65, 33, 8), (1, 2, 64, 64, 32), (1, 1, 130, 200, 64), (1, 1, 40, 129, 96), (1, 1, 33, 65, 128),
])
def test_attention(dev, B, heads, Tq, Tk, d):
    Cc = heads * d
    q = rnd(B, Tq, Cc, seed=1); k = rnd(B, Tk, Cc, seed=2); v = rnd(B, Tk, Cc, seed=3)
    ldv = PK.round_up(Tk, 8)
    vt = torch.full((B, Cc, ldv), float("nan"), dtype=BF, device=dev)   # garbage in the kv pad must not leak
    vt[:, :, :Tk] = v.transpose(1, 2)
    o = torch.zeros(B, Tq, Cc, dtype=BF, device=dev)
    scale = d ** -0.5
    O.run_ops([O.Attn(q, k, vt, o, heads=heads, Tk=Tk, scale=scale)])
    torch.cuda.synchronize()
    ref = ref_attention(q.float().cpu(), k.float().cpu(), v.float().cpu(), heads, scale)
    close(o, ref, name=f"attn {B},{heads},{Tq},{Tk},{d}")


def test_attention_strided_qk_buffer(dev):
    # Q and K are the two halves of one fused projection buffer [B, T, 2C]
    B, heads, T, d = 2, 8, 350, 80
    Cc = heads * d
    qk = rnd(B, T, 2 * Cc, seed=1); v = rnd(B, T, Cc, seed=3)
    vt = torch.zeros(B, Cc, PK.round_up(T, 8), dtype=BF, device=dev); vt[:, :, :T] = v.transpose(1, 2)
    o = torch.zeros(B, T, Cc, dtype=BF, device=dev)
    O.run_ops([O.Attn(qk[:, :, :Cc], qk[:, :, Cc:], vt, o, heads=heads, Tk=T, scale=d ** -0.5)])
    torch.cuda.synchronize()
    ref = ref_attention(qk[:, :, :Cc].float().cpu(), qk[:, :, Cc:].float().cpu(), v.float().cpu(), heads, d ** -0.5)
    close(o, ref, name="attn strided")


def test_attention_softmax_rescale_branch(dev):
    # §5.4 rule 26: force the running max to jump in a late kv tile
    B, heads, Tq, Tk, d = 1, 1, 64, 320, 64
    q = rnd(B, Tq, d, seed=1); k = rnd(B, Tk, d, seed=2); v = rnd(B, Tk, d, seed=3)
    k[0, 250] = q[0, 5] * 6.0      # spike for query 5 in the 4th tile
    k[0, 10] = q[0, 9] * 6.0       # and an early one that later tiles must not disturb
    vt = torch.zeros(B, d, Tk, dtype=BF, device=dev); vt[:] = v.transpose(1, 2)
    o = torch.zeros(B, Tq, d, dtype=BF, device=dev)
    O.run_ops([O.Attn(q, k, vt, o, heads=1, Tk=Tk, scale=d ** -0.5)])
    torch.cuda.synchronize()
    ref = ref_attention(q.double().cpu(), k.double().cpu(), v.double().cpu(), 1, d ** -0.5)
    close(o, ref, name="attn rescale")


@pytest.mark.parametrize("b,heads,T,d", [(1, 8, 1400, 40), (2, 8, 350, 80), (2, 8, 91, 160), (1, 2, 50, 16)])
def test_attention_crossview_two_sources(dev, b, heads, T, d):
    # blocks.py:106-222 'add' mode: view i attends to its left and right neighbour separately; outputs summed
    ncam = 6
    pair = {0: [5, 1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3, 5], 5: [4, 0]}
    Cc = heads * d; B = b * ncam
    q = rnd(B, T, Cc, seed=1); k = rnd(B, T, Cc, seed=2); v = rnd(B, T, Cc, seed=3)
    vt = torch.zeros(B, Cc, PK.round_up(T, 8), dtype=BF, device=dev); vt[:, :, :T] = v.transpose(1, 2)
    kvmap = torch.tensor([(i // ncam) * ncam + pair[i % ncam][s] for i in range(B) for s in range(2)], dtype=torch.int32, device=dev)
    o = torch.zeros(B, T, Cc, dtype=BF, device=dev)
    O.run_ops([O.Attn(q, k, vt, o, heads=heads, Tk=T, scale=d ** -0.5, kvmap=kvmap, nsrc=2)])
    torch.cuda.synchronize()
    qc, kc, vc = q.float().cpu(), k.float().cpu(), v.float().cpu()
    ref = torch.zeros(B, T, Cc)
    for i in range(B):
        for s in range(2):
            j = (i // ncam) * ncam + pair[i % ncam][s]
            ref[i] += ref_attention(qc[i:i + 1], kc[j:j + 1], vc[j:j + 1], heads, d ** -0.5)[0]
    close(o, ref, name="attn cross-view")


@pytest.mark.parametrize("B,HW,Cc,G,silu,eps", [(2, 1400, 320, 32, True, 1e-5), (2, 350, 1920, 32, True, 1e-5), (3, 91, 1280, 32, False, 1e-6),
                                                   (2, 100, 32, 32, True, 1e-5), (1, 28, 2560, 32, True, 1e-5), (2, 64, 64, 8, False, 1e-5),
                                                   # the streaming two-stage kernels: 960-channel concat input, many images (chunking
                                                   # by batch), 2560 channels (two channel vectors per thread), chunk tails (HW = 1399)
                                                   (2, 1400, 960, 32, True, 1e-5), (40, 350, 640, 32, True, 1e-5), (7, 91, 2560, 32, True, 1e-5),
                                                   (3, 1399, 320, 32, False, 1e-6), (600, 28, 1280, 32, True, 1e-5)])
def test_groupnorm(dev, B, HW, Cc, G, silu, eps):
    x = (rnd(B, HW, Cc, seed=1).float() * 2 + 0.7).to(BF)
    if Cc == 960: x = (x.float() + 6.0).to(BF)                      # |mean| >> std: the pivot keeps the variance conditioned
    gam = rnd(Cc, seed=2, dtype=torch.float32); bet = rnd(Cc, seed=3, dtype=torch.float32)
    y = torch.zeros_like(x)
    O.run_ops([O.GroupNorm(x, y, gam, bet, groups=G, eps=eps, silu=silu)])
    k1 = (L.lib().mdx_last_kernel() or b"").decode()
    y2 = torch.zeros_like(x)      # with a workspace: the two-stage coalesced path for big maps (GN_ONE_KERNEL_ELEMS = 0: also for these few-image cases,
    with L.options(GN_ONE_KERNEL_ELEMS=0):   # which the round-6 rule keeps on the one-launch kernel up to 4 M elements)
        O.run_ops([O.GroupNorm(x, y2, gam, bet, groups=G, eps=eps, silu=silu, ws=ws_buf(dev, 4))])
        k2 = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert k1 == "groupnorm_kernel" and (k2 == "gn_stats_kernel+gn_apply_kernel") == (HW * Cc >= 32768), (k1, k2)
    if B * HW * Cc > (4 << 20) or HW * Cc < 32768:      # default rule with a workspace: one launch up to 4 M elements, the streaming passes above
        y3 = torch.zeros_like(x)
        O.run_ops([O.GroupNorm(x, y3, gam, bet, groups=G, eps=eps, silu=silu, ws=ws_buf(dev, 4))])
        k3 = (L.lib().mdx_last_kernel() or b"").decode()
        assert k3 == k2 and torch.equal(y3, y2), (k3, k2)
    else:
        y3 = torch.zeros_like(x)
        O.run_ops([O.GroupNorm(x, y3, gam, bet, groups=G, eps=eps, silu=silu, ws=ws_buf(dev, 4))])
        assert (L.lib().mdx_last_kernel() or b"").decode() == "groupnorm_kernel" and torch.equal(y3, y)
    ref = F.group_norm(x.float().cpu().transpose(1, 2), G, gam.cpu(), bet.cpu(), eps)
    if silu: ref = F.silu(ref)
    close(y, ref.transpose(1, 2), name="groupnorm")
    close(y2, ref.transpose(1, 2), name="groupnorm two-stage")


@pytest.mark.parametrize("B,HW,Cc", [(6, 89600, 128), (3, 22400, 256), (2, 5600, 512)])
def test_groupnorm_many_chunks_finalize(dev, B, HW, Cc):
    """Few large images (the VAE decoder's maps): hundreds of chunks per image — the chunk partials are combined ONCE by gn_finalize_kernel (a fixed
    lane tree) instead of by every apply workgroup.  Against torch, bit-identical across two runs, and the same route with the finalize step
    switched off agrees to rounding."""
    G = 32
    x = (rnd(B, HW, Cc, seed=1).float() * 1.5 + 0.4).to(BF)
    gam = rnd(Cc, seed=2, dtype=torch.float32); bet = rnd(Cc, seed=3, dtype=torch.float32)
    ws = ws_buf(dev, 4)
    ys = []
    for opts in ({}, {}, {"GN_FINALIZE_CHUNKS": 0}):
        y = torch.zeros_like(x)
        with L.options(**opts):
            O.run_ops([O.GroupNorm(x, y, gam, bet, groups=G, eps=1e-6, silu=True, ws=ws)])
        torch.cuda.synchronize()
        ys.append(y)
    ref = F.silu(F.group_norm(x.float().cpu().transpose(1, 2), G, gam.cpu(), bet.cpu(), 1e-6)).transpose(1, 2)
    close(ys[0], ref, name=f"groupnorm finalize {B}x{HW}x{Cc}")
    assert torch.equal(ys[0], ys[1]), "not deterministic"
    assert rel_l2(ys[0], ys[2]) < 3e-3


def test_groupnorm_channel_slice_view(dev):
    big = rnd(2, 50, 96, seed=1)
    x = big[:, :, 32:96]
    gam = rnd(64, seed=2, dtype=torch.float32); bet = rnd(64, seed=3, dtype=torch.float32)
    y = torch.zeros(2, 50, 64, dtype=BF, device=dev)
    O.run_ops([O.GroupNorm(x, y, gam, bet, groups=32, eps=1e-5)])
    torch.cuda.synchronize()
    ref = F.group_norm(x.float().cpu().transpose(1, 2), 32, gam.cpu(), bet.cpu(), 1e-5).transpose(1, 2)
    close(y, ref, name="groupnorm view")


@pytest.mark.parametrize("M,Cc", [(8400, 320), (2100, 640), (546, 1280), (37, 64), (5, 2048), (8403, 320), (2101, 640), (1, 320)])
def test_layernorm(dev, M, Cc):
    x = (rnd(M, Cc, seed=1).float() * 3 - 0.5).to(BF)
    gam = rnd(Cc, seed=2, dtype=torch.float32); bet = rnd(Cc, seed=3, dtype=torch.float32)
    y = torch.zeros_like(x)
    O.run_ops([O.LayerNorm(x, y, gam, bet)])
    torch.cuda.synchronize()
    close(y, F.layer_norm(x.float().cpu(), (Cc,), gam.cpu(), bet.cpu()), name="layernorm")


def test_elementwise_family(dev):
    x = rnd(700, 320, seed=1); y0 = rnd(700, 320, seed=2)
    y = y0.clone()
    O.run_ops([O.Ew(L.EW_ADD, x, y)])
    close(y, x.float().cpu() + y0.float().cpu(), name="add")
    # concat by two strided copies
    a = rnd(300, 64, seed=3); b = rnd(300, 40, seed=4)
    cat = torch.zeros(300, 104, dtype=BF, device=dev)
    O.run_ops([O.Ew(L.EW_COPY, a, cat[:, :64]), O.Ew(L.EW_COPY, b, cat[:, 64:])])
    assert torch.equal(cat.cpu(), torch.cat([a, b], 1).cpu())
    # fp32 copy / scale / silu
    f = rnd(10, 7, seed=5, dtype=torch.float32); g = torch.zeros_like(f)
    O.run_ops([O.Ew(L.EW_COPY, f, g)]); assert torch.equal(f.cpu(), g.cpu())
    O.run_ops([O.Ew(L.EW_SCALE, f, g, alpha=0.5)]); assert torch.allclose(g.cpu(), f.cpu() * 0.5)
    O.run_ops([O.Ew(L.EW_SILU, f, g)]); assert torch.allclose(g.cpu(), F.silu(f.cpu()), atol=1e-5)
    # nearest upsample to an explicit size (4x7 -> 7x13)
    u = rnd(2, 4, 7, 64, seed=6); up = torch.zeros(2, 7, 13, 64, dtype=BF, device=dev)
    O.run_ops([O.Upsample(u, up, PK.nearest_index(4, 7).to(dev), PK.nearest_index(7, 13).to(dev))])
    ref = F.interpolate(u.float().cpu().permute(0, 3, 1, 2), size=(7, 13), mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(up.float().cpu(), ref)
    assert (L.lib().mdx_last_kernel() or b"").decode() == "ew_upsample_vec8_kernel"
    u = rnd(2, 14, 25, 20, seed=6); up = torch.zeros(2, 28, 50, 20, dtype=BF, device=dev)       # C % 8 != 0: the scalar path
    O.run_ops([O.Upsample(u, up, PK.nearest_index(14, 28).to(dev), PK.nearest_index(25, 50).to(dev))])
    ref = F.interpolate(u.float().cpu().permute(0, 3, 1, 2), size=(28, 50), mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(up.float().cpu(), ref)
    # layouts
    n = rnd(2, 4, 28, 50, seed=7, dtype=torch.float32); h = torch.zeros(2, 28, 50, 4, dtype=torch.float32, device=dev)
    O.run_ops([O.Layout(n, h, True)]); assert torch.equal(h.cpu(), n.permute(0, 2, 3, 1).cpu())
    back = torch.zeros_like(n)
    O.run_ops([O.Layout(h, back, False)]); assert torch.equal(back.cpu(), n.cpu())
    hb = torch.zeros(2, 28, 50, 4, dtype=BF, device=dev)
    O.run_ops([O.Layout(n, hb, True)]); assert torch.equal(hb.cpu(), n.permute(0, 2, 3, 1).to(BF).cpu())
    torch.cuda.synchronize()


def test_fourier_gather_timeemb(dev):
    # embedder.py:15-40 order: [x, sin(f0 x), cos(f0 x), sin(f1 x), ...]
    n, Pn, Fq = 37, 8, 4
    x = rnd(n, Pn, 3, scale=20.0, seed=1, dtype=torch.float32)
    mask = (torch.arange(n) % 3 != 0).to(torch.uint8).to(dev)
    null = rnd(Pn * 27, seed=2, dtype=torch.float32)
    y = torch.zeros(n, Pn * 27, dtype=BF, device=dev)
    O.run_ops([O.Fourier(x, y, Fq, mask=mask, null_feat=null)])
    xc = x.cpu()
    parts = [xc]
    for f in [1.0, 2.0, 4.0, 8.0]:
        parts += [torch.sin(xc * f), torch.cos(xc * f)]
    ref = torch.cat(parts, -1).reshape(n, -1)
    m = mask.cpu().float()[:, None]
    ref = ref * m + null.cpu()[None] * (1 - m)
    close(y, ref, rtol=1e-2, atol_rel=5e-3, name="fourier")
    # gather with -1 indices under mask 0
    T = rnd(10, 64, seed=3); idx = torch.tensor([0, 9, -1, 3, -1], dtype=torch.int64, device=dev)
    mk = torch.tensor([1, 1, 0, 1, 0], dtype=torch.uint8, device=dev); nr = rnd(64, seed=4)
    out = torch.zeros(5, 64, dtype=BF, device=dev)
    O.run_ops([O.Gather(T, out, idx, mask=mk, null_row=nr)])
    exp = torch.stack([T[0], T[9], nr, T[3], nr]).cpu()
    assert torch.equal(out.cpu(), exp)
    # timestep embedding vs the diffusers formula (embeddings.py:24-64, flip_sin_to_cos=True, shift 0)
    t = torch.tensor([981.0, 501.0, 1.0, 0.0], device=dev)
    te = torch.zeros(4, 320, dtype=torch.float32, device=dev)
    O.run_ops([O.TimeEmb(t, te)])
    half = 160
    expo = -math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half
    emb = t.cpu()[:, None] * torch.exp(expo)[None]
    ref = torch.cat([torch.cos(emb), torch.sin(emb)], -1)
    assert torch.allclose(te.cpu(), ref, atol=2e-4), (te.cpu() - ref).abs().max()
    torch.cuda.synchronize()


def test_cfg_ddim_and_graph_replay(dev):
    n = 6 * 4 * 28 * 50
    x0 = rnd(n, seed=1, dtype=torch.float32); x = x0.clone()
    eps = rnd(2 * n, seed=2, dtype=torch.float32)
    coef = torch.tensor([[0.9, 0.4359, 0.95, 0.3122], [0.95, 0.3122, 0.99, 0.1411]], dtype=torch.float32, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    xin = torch.zeros(2 * n, dtype=torch.float32, device=dev)
    op = O.DdimStep(x, eps, coef, step, x_in=xin, cfg=True, guidance=2.0)
    prog = O.build_program([op])
    st = torch.cuda.current_stream().cuda_stream
    prog.run(st)
    torch.cuda.synchronize()

    def ref_step(xc, c):
        e = eps[:n].cpu() + 2.0 * (eps[n:].cpu() - eps[:n].cpu())
        p0 = (xc - c[1] * e) / c[0]
        return c[2] * p0 + c[3] * e
    r1 = ref_step(x0.cpu(), coef[0].cpu())
    assert torch.allclose(x.cpu(), r1, atol=1e-5) and step.item() == 1
    assert torch.equal(xin[:n].cpu(), x.cpu()) and torch.equal(xin[n:].cpu(), x.cpu())
    # replay through a captured hipGraph: picks row 1 of the table via the device-side counter
    prog.launch(st)
    torch.cuda.synchronize()
    assert torch.allclose(x.cpu(), ref_step(r1, coef[1].cpu()), atol=1e-5) and step.item() == 2


@pytest.mark.parametrize("rows,T,ld", [(91 * 2, 91, 96), (300, 1400, 1400), (5, 7, 8)])
def test_softmax_rows(dev, rows, T, ld):
    """mdx_softmax_rows: fp32 scores (row pitch ld) -> bf16 probabilities, pad columns written as zeros."""
    X = torch.randn(rows, ld, generator=torch.Generator().manual_seed(1)).mul(3.0).to(dev)
    Y = torch.full((rows, ld), float("nan"), dtype=BF, device=dev)
    O.run_ops([O.Softmax(X, Y, T, scale=0.37)])
    torch.cuda.synchronize()
    ref = torch.softmax(X[:, :T].cpu() * 0.37, dim=-1)
    assert torch.allclose(Y[:, :T].float().cpu(), ref, atol=2e-3, rtol=1e-2)
    assert (Y[:, T:].float() == 0).all() and abs(Y[:, :T].float().sum(-1).mean().item() - 1.0) < 5e-3


@pytest.mark.parametrize("mode", [1, 2])
def test_cfg_ddim_given_views(dev, mode):
    """MdxDdimDesc.gv_*: views 1 and 4 of 6 are known.  Mode 1: after every step but the last they are replaced by
    coef[2] * cond + coef[3] * noise; mode 2: their noise prediction is the initial noise."""
    V, ve = 6, 4 * 28 * 50
    n = V * ve
    x = rnd(n, seed=1, dtype=torch.float32); x0 = x.clone()
    eps = rnd(2 * n, seed=2, dtype=torch.float32)
    cond = rnd(n, seed=3, dtype=torch.float32); noise = rnd(n, seed=4, dtype=torch.float32)
    mask = torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.uint8, device=dev)
    coef = torch.tensor([[0.9, 0.4359, 0.95, 0.3122], [0.95, 0.3122, 0.99, 0.1411]], dtype=torch.float32, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    xin = torch.zeros(2 * n, dtype=torch.float32, device=dev)
    prog = O.build_program([O.DdimStep(x, eps, coef, step, x_in=xin, cfg=True, guidance=2.0, gv_mask=mask, gv_cond=cond, gv_noise=noise,
                                       gv_mode=mode, gv_last_step=1)])
    st = torch.cuda.current_stream().cuda_stream
    g = mask.cpu().bool().repeat_interleave(ve)
    e = eps[:n].cpu() + 2.0 * (eps[n:].cpu() - eps[:n].cpu())
    if mode == 2:
        e = torch.where(g, noise.cpu(), e)
    ref = x0.cpu()
    for s_ in range(2):
        (prog.run if s_ == 0 else prog.launch)(st)
        torch.cuda.synchronize()
        c = coef[s_].cpu()
        ref = c[2] * (ref - c[1] * e) / c[0] + c[3] * e
        if mode == 1 and s_ < 1:
            ref = torch.where(g, c[2] * cond.cpu() + c[3] * noise.cpu(), ref)
        assert torch.allclose(x.cpu(), ref, atol=1e-5), (mode, s_, (x.cpu() - ref).abs().max())
        assert torch.equal(xin[:n].cpu(), x.cpu()) and torch.equal(xin[n:].cpu(), x.cpu())
    with pytest.raises(ValueError):          # host-side descriptor validation
        O.run_ops([O.DdimStep(x, eps, coef, step, gv_mask=mask, gv_noise=None, gv_cond=cond, gv_mode=1, cfg=True)])


def test_cfg_unipc_matches_oracle_scheduler(dev):
    """mdx_cfg_unipc_step driven for a whole 8-step trajectory (warm-up, order 2, lower-order final) against
    oracle.denoiser.UniPC with the same per-step eps; also checks the bf16 padded model-input copy."""
    from magicdrive_amd import schedulers
    from oracle import denoiser as D
    npx, Cc = 6 * 28 * 50, 4
    n = npx * Cc
    sch = schedulers.UniPCMultistepScheduler(); ts = sch.set_timesteps(8)
    o = D.UniPC(); o.set_timesteps(8)
    x = rnd(n, seed=1, dtype=torch.float32); xo = x.cpu().clone()
    eps = torch.zeros(2 * n, dtype=torch.float32, device=dev)
    coef = sch.coefficient_table().to(dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    xl, m1, m2 = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(3))
    xin = torch.full((2 * npx, 8), 7.0, dtype=BF, device=dev)
    prog = O.build_program([O.UniPCStep(x, eps, coef, step, xl, m1, m2, x_in=xin, cfg=True, guidance=2.0, xin_c=Cc)])
    st = torch.cuda.current_stream().cuda_stream
    for i, t in enumerate(ts.tolist()):
        e = torch.randn(2 * n, generator=torch.Generator().manual_seed(100 + i))
        eps.copy_(e)
        (prog.run if i == 0 else prog.launch)(st)          # eager once, then hipGraph replays picking row i by the device counter
        torch.cuda.synchronize()
        xo = o.step(e[:n] + 2.0 * (e[n:] - e[:n]), t, xo)
        assert torch.allclose(x.cpu(), xo, atol=3e-5 * float(xo.abs().max()), rtol=1e-5), (i, (x.cpu() - xo).abs().max())
    assert step.item() == 8
    exp = x.cpu().view(npx, Cc).to(BF)
    assert torch.equal(xin[:npx, :Cc].cpu(), exp) and torch.equal(xin[npx:, :Cc].cpu(), exp) and (xin[:, Cc:].float() == 7.0).all()


def test_error_paths(dev):
    A = rnd(16, 12, seed=1); W = rnd(8, 12, seed=2); C = torch.zeros(16, 8, dtype=BF, device=dev)
    with pytest.raises(L.MdxError):
        O.run_ops([O.Gemm(A, W, C)])            # K % 8 != 0
    q = rnd(1, 8, 12, seed=1)
    with pytest.raises(L.MdxError):
        O.run_ops([O.Attn(q, q, torch.zeros(1, 12, 8, dtype=BF, device=dev), torch.zeros_like(q), heads=1, Tk=8, scale=1.0)])  # d=12


def test_ddim_scheduler_step_device_timestep_hit_and_miss(dev):
    """DDIMScheduler.step as user code drives it (scheduling_ddim.py:325-445): a DEVICE-side timestep selects its coefficient row without a
    host sync; a timestep that is not in the scheduler's list cannot raise there, so the kernel poisons the result with NaN (ADVICE r3:
    round 3 silently used row 0), while a host-side timestep still raises ValueError."""
    from magicdrive_amd import schedulers
    from oracle import denoiser as D
    s = schedulers.DDIMScheduler(); ts = s.set_timesteps(10)
    o = D.DDIM(); o.set_timesteps(10)
    x = torch.randn(2, 4, 28, 50, device=dev); e = torch.randn(2, 4, 28, 50, device=dev)
    t = ts[3]
    got = s.step(e, t.to(dev), x).prev_sample
    want = o.step(e.cpu(), int(t), x.cpu())
    assert rel_l2(got, want) < 1e-6
    assert rel_l2(s.step(e, int(t), x).prev_sample, want) < 1e-6
    miss = s.step(e, torch.tensor(int(t) + 1, device=dev), x).prev_sample
    torch.cuda.synchronize()
    assert torch.isnan(miss).all()
    with pytest.raises(ValueError):
        s.step(e, int(t) + 1, x)


def test_cfg_ddim_bf16_padded_model_input(dev):
    # x_in as the channels-last bf16 copy with pixel stride 8 that conv_in's MFMA path reads
    npx, Cc = 6 * 28 * 50, 4
    n = npx * Cc
    x = rnd(n, seed=1, dtype=torch.float32); x0 = x.clone()
    eps = rnd(2 * n, seed=2, dtype=torch.float32)
    coef = torch.tensor([[0.9, 0.4359, 0.95, 0.3122]], dtype=torch.float32, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    xin = torch.full((2 * npx, 8), 7.0, dtype=BF, device=dev)
    O.run_ops([O.DdimStep(x, eps, coef, step, x_in=xin, cfg=True, guidance=2.0, xin_c=Cc)])
    torch.cuda.synchronize()
    e = eps[:n].cpu() + 2.0 * (eps[n:].cpu() - eps[:n].cpu())
    c = coef[0].cpu()
    ref = c[2] * (x0.cpu() - c[1] * e) / c[0] + c[3] * e
    assert torch.allclose(x.cpu(), ref, atol=1e-5)
    exp = x.cpu().view(npx, Cc).to(BF)           # the copy is the bf16 rounding of the kernel's own fp32 result
    assert torch.equal(xin[:npx, :Cc].cpu(), exp) and torch.equal(xin[npx:, :Cc].cpu(), exp)
    assert (xin[:, Cc:].float() == 7.0).all(), "pad channels must not be touched"


def test_unipc_scheduler_host_step_on_gpu(dev):
    """`UniPCMultistepScheduler.step()` (the reference's host API, scheduling_unipc_multistep.py:518-600) on the fused kernel: diffusers' full-loop
    known-answer test (test_scheduler_unipc.py:205-209: mean |x| = 0.2521) and step-by-step agreement with the oracle's restatement."""
    from magicdrive_amd.schedulers import UniPCMultistepScheduler
    from oracle import denoiser as D
    kw = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", solver_order=2, solver_type="bh1")
    s = UniPCMultistepScheduler(**kw); ref = D.UniPC(**kw); ref.set_timesteps(10)
    n = 4 * 3 * 8 * 8
    x_ref = (torch.arange(n).reshape(3, 8, 8, 4) / n).permute(3, 0, 1, 2).contiguous()
    sample = x_ref.clone().to(dev)
    for t in s.set_timesteps(10):
        sample = s.step(sample * t / (t + 1), t, sample).prev_sample
        x_ref = ref.step(x_ref * t / (t + 1), int(t), x_ref)
        assert (sample.cpu() - x_ref).abs().max().item() < 2e-5
    assert abs(sample.abs().mean().item() - 0.2521) < 1e-3


@pytest.mark.parametrize("T,Tk,d,expect", [(91, 91, 160, "attn_kernel<10,4,self>"), (28, 28, 160, "attn_kernel<10,4,self>"), (91, 78, 160, "attn_kernel<10,4,self>"),
                                            (28, 78, 80, "attn_kernel<5,4,self>")])
def test_attention_short_sequences_many_heads(dev, T, Tk, d, expect):
    """Level-2 / mid-block shapes at a batch where (views x heads) alone fills the chip: 128-query workgroups with mostly idle query rows
    (attention.hip: launch_attn_nw) — rows >= Tq must neither be stored nor disturb the valid ones."""
    B, heads = 66, 8
    Cc = heads * d
    q = rnd(B, T, Cc, seed=1); k = rnd(B, Tk, Cc, seed=2); v = rnd(B, Tk, Cc, seed=3)
    vt = torch.full((B, Cc, PK.round_up(Tk, 8)), float("nan"), dtype=BF, device=dev); vt[:, :, :Tk] = v.transpose(1, 2)
    o = torch.full((B, T + 3, Cc), 7.0, dtype=BF, device=dev)
    O.run_ops([O.Attn(q, k, vt, o[:, :T], heads=heads, Tk=Tk, scale=d ** -0.5)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern == expect, kern
    close(o[:, :T], ref_attention(q.float().cpu(), k.float().cpu(), v.float().cpu(), heads, d ** -0.5), name=f"attn short {T},{Tk},{d}")
    assert (o[:, T:].float() == 7.0).all(), "rows past Tq were written"


def test_attention_short_crossview_many_heads(dev):
    ncam = 6
    pair = {0: [5, 1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3, 5], 5: [4, 0]}
    B, heads, T, d = 66, 8, 28, 160
    Cc = heads * d
    q = rnd(B, T, Cc, seed=1); k = rnd(B, T, Cc, seed=2); v = rnd(B, T, Cc, seed=3)
    vt = torch.zeros(B, Cc, PK.round_up(T, 8), dtype=BF, device=dev); vt[:, :, :T] = v.transpose(1, 2)
    kvmap = torch.tensor([(i // ncam) * ncam + pair[i % ncam][s] for i in range(B) for s in range(2)], dtype=torch.int32, device=dev)
    o = torch.zeros(B, T, Cc, dtype=BF, device=dev)
    O.run_ops([O.Attn(q, k, vt, o, heads=heads, Tk=T, scale=d ** -0.5, kvmap=kvmap, nsrc=2)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern == "attn_kernel<10,2,xview>", kern
    qc, kc, vc = q.float().cpu(), k.float().cpu(), v.float().cpu()
    ref = torch.zeros(B, T, Cc)
    for i in range(B):
        for s_ in range(2):
            j = (i // ncam) * ncam + pair[i % ncam][s_]
            ref[i] += ref_attention(qc[i:i + 1], kc[j:j + 1], vc[j:j + 1], heads, d ** -0.5)[0]
    close(o, ref, name="attn short cross-view")


@pytest.mark.parametrize("b,heads,T,d,nsrc,expect", [
    (2, 8, 1400, 40, 2, "attn2_kernel<40,joint,q64>"),      # concat: two neighbours, one softmax (level 0)
    (1, 8, 1400, 40, 6, "attn2_kernel<40,joint,q64>"),      # self: all six cameras of a scene
    (2, 8, 350, 80, 2, "attn_kernel<5,4,joint>"),           # attention.hip
    (2, 8, 91, 160, 6, "attn_kernel<10,2,joint>"),
])
@pytest.mark.parametrize("pre", [False, True])
def test_attention_joint_sources(dev, b, heads, T, d, nsrc, expect, pre):
    """MdxAttnDesc.joint: ONE softmax over the concatenation of the nsrc kv sources (neighboring_attn_type concat / self, blocks.py:122-138)
    — not the sum of per-source attentions."""
    ncam = 6
    pair = {0: [5, 1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3, 5], 5: [4, 0]}
    Cc = heads * d; B = b * ncam
    q = rnd(B, T, Cc, seed=1); k = rnd(B, T, Cc, seed=2); v = rnd(B, T, Cc, seed=3)
    vt = torch.full((B, Cc, PK.round_up(T, 8)), float("nan"), dtype=BF, device=dev); vt[:, :, :T] = v.transpose(1, 2)
    srcs = lambda i: [(i // ncam) * ncam + c for c in (range(ncam) if nsrc == ncam else pair[i % ncam])]
    kvmap = torch.tensor([j for i in range(B) for j in srcs(i)], dtype=torch.int32, device=dev)
    o = torch.zeros(B, T, Cc, dtype=BF, device=dev)
    qpre = d ** -0.5 * 1.4426950408889634
    qref = q
    if pre:                                  # MdxAttnDesc.q_prescaled (every kernel takes it; head dim 40 folds the maximum into the MFMA)
        q = (q.float() * qpre).to(BF); qref = q.float() / qpre
        if d == 40:                           # pre-scaled head dim 40: attention3.hip (round 5); with ATTN3 = 0 the 32-query FOLD form of attention2.hip
            expect = "attn3_kernel<40,joint>" if L.get_option("ATTN3") else expect.replace("q64>", "q32,fold,pf>" if L.get_option("ATTN2_PF") else "q32,fold>")
    O.run_ops([O.Attn(q, k, vt, o, heads=heads, Tk=T, scale=d ** -0.5, kvmap=kvmap, nsrc=nsrc, joint=True, q_prescaled=pre)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern == expect, kern
    qc, kc, vc = qref.float().cpu(), k.float().cpu(), v.float().cpu()
    ref = torch.zeros(B, T, Cc)
    for i in range(B):
        js = srcs(i)
        ref[i] = ref_attention(qc[i:i + 1], torch.cat([kc[j] for j in js])[None], torch.cat([vc[j] for j in js])[None], heads, d ** -0.5)[0]
    close(o, ref, name=f"attn joint {nsrc} sources{' prescaled' if pre else ''}")


# ---- attention2.hip (head dim 40, >= 128 workgroups; 80 behind MDX_ATTN2_D80): routes asserted, the rare branches forced ---------
QPRE = lambda d: d ** -0.5 * 1.4426950408889634     # what engine.q_prescale folds into to_q


def prescale_q(q, d, pre):
    """(Q for the kernel, Q for the reference): pre = the q_prescaled form — Q' = bf16(Q * scale * log2 e); the reference gets Q' / that
    factor, i.e. the same rounded values."""
    if not pre:
        return q, q
    qp = (q.float() * QPRE(d)).to(BF)
    return qp, (qp.float() / QPRE(d))


def attn2_route(d, Tq, xview=False, pre=False):
    """Kernel mdx_attention_bf16 must pick for (d, Tq) under the library's current switches (csrc/options.h;
    tests/test_routes_gpu.py::test_forced_attention_routes re-runs these tests with ATTN2_QT=1, ATTN2_D80=1 and ATTN2=0)."""
    mode = "xview" if xview else "self"
    d80 = L.get_option("ATTN2_D80")              # 0 never, 1 always, 2 (default): only the two-source cross-view form
    if L.get_option("ATTN2") == 0 or (d == 80 and not (d80 == 1 or (d80 == 2 and xview))):
        return "attn_kernel<"                                       # attention.hip (prefix)
    fold = ",fold" if (pre and d == 40 and L.get_option("ATTN2_FOLD")) else ""
    if fold and L.get_option("ATTN3"):             # round 5: the pipelined, permute-free form takes every head-dim-40 FOLD launch
        return f"attn3_kernel<40,{mode}>"
    qt = L.get_option("ATTN2_QT")                  # 0: automatic = 64-query waves, except FOLD launches (32: four waves per SIMD)
    q = 64 if (d == 40 and Tq >= 512 and qt != 1 and (qt == 2 or not fold)) else 32
    if fold and q == 32 and L.get_option("ATTN2_PF"):      # round 5: the permute-free form takes the 32-query FOLD launches
        return f"attn2_kernel<{d},{mode},q32,fold,pf>"
    return f"attn2_kernel<{d},{mode},q{q}{fold}>"


ATTN2_CASES = [
    (6, 8, 1400, 1400, 40),      # 22 tiles, the last one 56 kv wide; 64-query waves: the last workgroup has 2 idle waves and a half wave (attention3: 128-query
                                 # workgroups, the last one with 3 full waves and one of 24 queries; an odd number of tile pairs + the masked tile)
    (6, 8, 1400, 78, 40),        # context: 2 tiles, pad columns inside a 16-byte chunk (NaN-poisoned below)
    (6, 8, 1400, 64, 40),        # exactly one full tile: no masked tile at all
    (6, 8, 1400, 129, 40),       # last tile 1 kv wide
    (6, 8, 350, 350, 80),
    (6, 8, 350, 110, 80),
    (3, 8, 777, 333, 40),        # ragged query block (777 = 3 x 256 + 9 = 6 x 128 + 9)
    (6, 8, 300, 300, 40),        # below 512 queries: 32-query waves
    (6, 8, 1400, 192, 40),       # three full tiles, no masked tile (attention3: pair loop + a full final tile)
    (6, 8, 1400, 256, 40),       # four full tiles (attention3: the remainder of two)
    (6, 8, 1290, 1283, 40),      # a wave with NO query (idle: stages and synchronises only) beside the scrub of a 3-kv last tile
    (6, 8, 640, 17, 40),         # a lone partial tile: first = final = masked
]


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("B,heads,Tq,Tk,d", ATTN2_CASES)
def test_attention2(dev, B, heads, Tq, Tk, d, pre):
    """pre: Q pre-scaled by scale * log2(e) (MdxAttnDesc.q_prescaled) — head dim 40 then runs the FOLD instances (running maximum
    subtracted inside the QK MFMA), head dim 80 the plain ones with a unit scale."""
    Cc = heads * d
    q = rnd(B, Tq, Cc, seed=1); k = rnd(B, Tk, Cc, seed=2); v = rnd(B, Tk, Cc, seed=3)
    q, qref = prescale_q(q, d, pre)
    ldv = PK.round_up(Tk, 8)
    vt = torch.full((B, Cc, ldv), float("nan"), dtype=BF, device=dev)   # garbage in the kv pad must not leak
    vt[:, :, :Tk] = v.transpose(1, 2)
    o = torch.full((B, Tq, Cc), float("nan"), dtype=BF, device=dev)
    O.run_ops([O.Attn(q, k, vt, o, heads=heads, Tk=Tk, scale=d ** -0.5, q_prescaled=pre)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern.startswith(attn2_route(d, Tq, pre=pre)), kern
    ref = ref_attention(qref.float().cpu(), k.float().cpu(), v.float().cpu(), heads, d ** -0.5)
    close(o, ref, name=f"attn2 {B},{heads},{Tq},{Tk},{d}{' prescaled' if pre else ''}")


@pytest.mark.parametrize("B,heads,Tq,Tk", [(6, 8, 1400, 78), (6, 8, 1400, 110), (6, 8, 1400, 64), (6, 8, 1400, 129), (3, 8, 777, 150), (6, 8, 300, 32),
                                           (2, 8, 1400, 192), (6, 8, 512, 17)])
def test_attention2_resident_short_kv(dev, B, heads, Tq, Tk):
    """Round 4: the text-context form (kv sequences of <= 3 tiles: S = 1 + 77 + boxes) with K / V^T RESIDENT in LDS and one workgroup per
    (view, head) walking the query blocks (attn2_kernel<.., RES>; ATTN2_RES=2 forces the route at test batch sizes).  Partial last tiles of
    every kind: 14 / 46 / 1 / 22 valid kv (<= 32: only the first 32-kv sub-tile is multiplied), none (64, 192), a lone 17-kv tile."""
    d = 40
    Cc = heads * d
    q = rnd(B, Tq, Cc, seed=1); k = rnd(B, Tk, Cc, seed=2); v = rnd(B, Tk, Cc, seed=3)
    # a score spike in the LAST tile for one query (the deferred maximum must re-base there) and an early one
    k[0, Tk - 1, :d] = q[0, 7, :d] * 6.0
    k[0, 3, d:2 * d] = q[0, 9, d:2 * d] * 6.0
    q, qref = prescale_q(q, d, True)
    ldv = PK.round_up(Tk, 8)
    vt = torch.full((B, Cc, ldv), float("nan"), dtype=BF, device=dev)   # garbage in the kv pad must not leak
    vt[:, :, :Tk] = v.transpose(1, 2)
    o = torch.full((B, Tq, Cc), float("nan"), dtype=BF, device=dev)
    with L.options(ATTN2_RES=2):
        O.run_ops([O.Attn(q, k, vt, o, heads=heads, Tk=Tk, scale=d ** -0.5, q_prescaled=True)])
        kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern == "attn2_kernel<40,resident,q32,fold>", kern
    ref = ref_attention(qref.double().cpu(), k.double().cpu(), v.double().cpu(), heads, d ** -0.5)
    close(o, ref, name=f"attn2 resident {B},{heads},{Tq},{Tk}")
    # same inputs through the streaming form: the two routes agree to rounding
    o2 = torch.full((B, Tq, Cc), float("nan"), dtype=BF, device=dev)
    with L.options(ATTN2_RES=0):
        O.run_ops([O.Attn(q, k, vt, o2, heads=heads, Tk=Tk, scale=d ** -0.5, q_prescaled=True)])
    torch.cuda.synchronize()
    assert rel_l2(o, o2) < 4e-3, rel_l2(o, o2)


@pytest.mark.parametrize("wgs", [1, 3, 0])
@pytest.mark.parametrize("Tq,Tk,xview", [(1290, 150, False), (1290, 150, True), (1400, 64, False), (520, 17, True), (1290, 1283, False)])
def test_attention3_persistent_items(dev, wgs, Tq, Tk, xview):
    """attention3.hip is persistent: the workgroups of an XCD walk its (view, head, 128-query block) items, the K / V^T stream continues across
    an item seam and an item's last step already multiplies the next item's first scores.  Forced here to ONE and to three workgroups per XCD
    (every workgroup walks many items: 11 blocks x 8 heads per view) and left automatic; partial last tiles (scrub + mask), single-tile items
    (Tk = 64: first tile = last tile; Tk = 17: one partial tile, two sources), a block whose waves 1-3 have no query (Tq = 1290: they sit the
    item out and must rejoin the pipeline in the next one), a late score spike in a later item."""
    B, heads, d = 11, 8, 40
    Cc = heads * d
    q = rnd(B, Tq, Cc, seed=1); k = rnd(B, Tk, Cc, seed=2); v = rnd(B, Tk, Cc, seed=3)
    k[0, Tk - 1, :d] = q[0, Tq // 2, :d] * 6.0
    k[9, 0, d:2 * d] = q[9, Tq - 1, d:2 * d] * 6.0
    q, qref = prescale_q(q, d, True)
    vt = torch.full((B, Cc, PK.round_up(Tk, 8)), float("nan"), dtype=BF, device=dev); vt[:, :, :Tk] = v.transpose(1, 2)
    o = torch.full((B, Tq, Cc), float("nan"), dtype=BF, device=dev)
    srcs = lambda i: [(i + 10) % B, (i + 1) % B]
    kw = dict(kvmap=torch.tensor([j for i in range(B) for j in srcs(i)], dtype=torch.int32, device=dev), nsrc=2) if xview else {}
    with L.options(ATTN3=1, ATTN3_WGS=wgs, ATTN2_RES=0):     # (ATTN3 is off by default: measured slower than attention2.hip)
        O.run_ops([O.Attn(q, k, vt, o, heads=heads, Tk=Tk, scale=d ** -0.5, q_prescaled=True, **kw)])
        kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    if kern.startswith("attn2_kernel"):
        pytest.skip("product build: attention3.hip is not linked in (make ATTN3=1 builds it; round 6)")
    assert kern == f"attn3_kernel<40,{'xview' if xview else 'self'}>", kern
    qc, kc, vc = qref.double().cpu(), k.double().cpu(), v.double().cpu()
    if xview:
        ref = torch.zeros(B, Tq, Cc, dtype=torch.float64)
        for i in range(B):
            for j in srcs(i):
                ref[i] += ref_attention(qc[i:i + 1], kc[j:j + 1], vc[j:j + 1], heads, d ** -0.5)[0]
    else:
        ref = ref_attention(qc, kc, vc, heads, d ** -0.5)
    close(o, ref, name=f"attn3 persistent wgs={wgs} {Tq},{Tk}{' xview' if xview else ''}")


@pytest.mark.parametrize("pre", [False, True])
def test_attention2_softmax_rescale_branch(dev, pre):
    """cdna guide rule 26 on the new kernel: the running max jumps in a LATE kv tile for one query (and early for another) by far more
    than the deferral threshold, so the O accumulators (16x16 layout) must be rescaled with the alpha of the right query lane — while
    the other queries of the same wave, whose max did not move, are multiplied by exactly 1; fp64 reference."""
    B, heads, Tq, Tk, d = 6, 8, 512, 448, 40
    Cc = heads * d
    q = rnd(B, Tq, Cc, seed=1); k = rnd(B, Tk, Cc, seed=2); v = rnd(B, Tk, Cc, seed=3)
    for h in range(heads):
        k[0, 400, h * d:(h + 1) * d] = q[0, 5 + h, h * d:(h + 1) * d] * 6.0       # spike in the 7th tile for query 5 + h of head h
        k[1, 10, h * d:(h + 1) * d] = q[1, 200 + 17 * h, h * d:(h + 1) * d] * 6.0  # an early one that later tiles must not disturb
        k[2, 30, h * d:(h + 1) * d] = q[2, 100 + h, h * d:(h + 1) * d] * -9.0      # a strongly NEGATIVE score in the first tile (FOLD: the first tile re-bases from m = 0)
    q[3] = q[3] * 0.01                                                              # a view whose scores are all tiny: the maximum never exceeds the deferral threshold
    vt = torch.zeros(B, Cc, Tk, dtype=BF, device=dev); vt[:] = v.transpose(1, 2)
    o = torch.zeros(B, Tq, Cc, dtype=BF, device=dev)
    q, qref = prescale_q(q, d, pre)
    O.run_ops([O.Attn(q, k, vt, o, heads=heads, Tk=Tk, scale=d ** -0.5, q_prescaled=pre)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern.startswith(attn2_route(40, Tq, pre=pre)), kern
    ref = ref_attention(qref.double().cpu(), k.double().cpu(), v.double().cpu(), heads, d ** -0.5)
    close(o, ref, name=f"attn2 rescale{' prescaled' if pre else ''}")


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("b,heads,T,d", [(1, 8, 1400, 40), (3, 8, 350, 80), (2, 8, 700, 40)])
def test_attention2_crossview(dev, b, heads, T, d, pre):
    ncam = 6
    pair = {0: [5, 1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3, 5], 5: [4, 0]}
    Cc = heads * d; B = b * ncam
    q = rnd(B, T, Cc, seed=1); k = rnd(B, T, Cc, seed=2); v = rnd(B, T, Cc, seed=3)
    vt = torch.full((B, Cc, PK.round_up(T, 8)), float("nan"), dtype=BF, device=dev); vt[:, :, :T] = v.transpose(1, 2)
    kvmap = torch.tensor([(i // ncam) * ncam + pair[i % ncam][s] for i in range(B) for s in range(2)], dtype=torch.int32, device=dev)
    o = torch.zeros(B, T, Cc, dtype=BF, device=dev)
    q, qref = prescale_q(q, d, pre)
    O.run_ops([O.Attn(q, k, vt, o, heads=heads, Tk=T, scale=d ** -0.5, kvmap=kvmap, nsrc=2, q_prescaled=pre)])
    kern = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    assert kern.startswith(attn2_route(d, T, xview=True, pre=pre)), kern
    qc, kc, vc = qref.float().cpu(), k.float().cpu(), v.float().cpu()
    ref = torch.zeros(B, T, Cc)
    for i in range(B):
        for s in range(2):
            j = (i // ncam) * ncam + pair[i % ncam][s]
            ref[i] += ref_attention(qc[i:i + 1], kc[j:j + 1], vc[j:j + 1], heads, d ** -0.5)[0]
    close(o, ref, name=f"attn2 cross-view{' prescaled' if pre else ''}")


# ---- one smallest shape per attention family: the kernel the library reports is the one csrc/attn_route.h names -------------------
ROUTE_FAMILIES = {
    "flash": dict(name="flash", B=1, H=1, Tq=33, d=16, pre=False, kmult=1),
    "attn2": dict(name="attn2", B=8, H=8, Tq=256, d=40, pre=False, kmult=1),
    "resident": dict(name="resident", B=8, H=8, Tq=256, Tk=192, d=40, pre=True, kmult=1, opts={"ATTN2_RES": 2}),
    "short": dict(name="short", B=2, H=2, Tq=5, d=32, pre=False, kmult=3, causal=True, rowmajor=True),
    "ctx": dict(name="ctx", B=2, H=2, Tq=33, Tk=40, d=16, pre=False, kmult=1, ctx="dev", live=27),
}


@pytest.fixture(scope="module")
def family_routes(tmp_path_factory):
    """What tests/attn_route_check.cpp (g++, the header alone) says for the five descriptors."""
    import attn_route_table as T
    cases = {k: dict(T.DEFAULTS, **c) for k, c in ROUTE_FAMILIES.items()}
    out = T.evaluate([f"{k} {T.route_line(c)}" for k, c in cases.items()], tmp_path_factory.mktemp("attn_route"))
    if out is None:
        pytest.skip("no g++")
    return out


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
@pytest.mark.parametrize("family", list(ROUTE_FAMILIES))
def test_attention_family_runs_the_kernel_the_route_header_names(dev, family_routes, family, f16):
    import attn_route_table as T
    tag, o, ref = T.run_case(dict(T.DEFAULTS, **ROUTE_FAMILIES[family], f16=f16), values=True)
    want = family_routes[family]
    assert tag == want["tag"], (tag, want)
    assert want["family"] == {"resident": "attn2-resident"}.get(family, family), want
    close(o, ref, name=f"attn family {family}", kind="f16" if f16 else "bf16")
