"""-m gpu: the LEAST aligned descriptors the C-ABI still accepts (include/mdx.h, "Requirements" / "Served"), numerically.

tests/test_contract.py pins what the entry points refuse; this file runs what they accept at the edge of that contract and checks that the
fallback kernel such a descriptor is routed to computes the same thing as the default one.  Every case: inputs rounded to the storage type,
a plain fp32 / fp64 torch reference on the CPU, outputs as views inside a larger NaN-filled buffer whose border must still be NaN afterwards,
helpers.close() with the table of the storage type (fp32 outputs: the 2e-5 bound of test_conv_out_weight_stationary), and an assertion on
mdx_last_kernel().  Both storage types, passed as kind= (no module constants are patched).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from magicdrive_amd import _lib as L
from magicdrive_amd import ops as O
from magicdrive_amd import packing as PK

from helpers import check, close, rel_l2  # noqa: E402
from test_kernels_gpu import ln_fold, ln_ref, ref_attention, rowstat_ref  # noqa: E402  (shared references)

F32 = torch.float32
DTYPES = [torch.bfloat16, torch.float16]
KIND = {torch.bfloat16: "bf16", torch.float16: "f16"}
NAN = float("nan")


def rnd(*shape, scale=1.0, seed=0, dtype=torch.bfloat16, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def last_kernel():
    return (L.lib().mdx_last_kernel() or b"").decode()


class Guarded:
    """A [*lead, rows, cols] view with row stride ld, `off` elements into a row of a NaN-filled buffer that has `pad` spare rows at both ends."""

    def __init__(self, shape, ld, off, dtype, dev, pad=2, fill=None):
        *lead, rows, cols = shape
        assert off + cols <= ld
        nl = int(math.prod(lead)) if lead else 1
        self.buf = torch.full(((nl * rows + 2 * pad) * ld,), NAN, dtype=dtype, device=dev)
        strides = []
        s = rows * ld
        for n in reversed(lead):
            strides.insert(0, s); s *= n
        self.view = self.buf.as_strided(tuple(shape), tuple(strides) + (ld, 1), pad * ld + off)
        if fill is not None:
            self.view.copy_(fill)

    def border_intact(self):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        mask.as_strided(self.view.shape, self.view.stride(), self.view.storage_offset()).fill_(False)
        return bool(torch.isnan(self.buf[mask].float()).all())


def side(n, off, seed, dev, scale=1.0, shift=0.0):
    """fp32 side operand (bias / temb / gamma / beta) as a slice `off` floats into a larger NaN-filled buffer."""
    buf = torch.full((n + off + 8,), NAN, dtype=F32, device=dev)
    buf[off:off + n] = rnd(n, seed=seed, dtype=F32, scale=scale) + shift
    return buf[off:off + n]


# --------------------------------------------------------------------------------------------------------------------------------------
# GEMM: 8-byte aligned C / R views on every main loop
# --------------------------------------------------------------------------------------------------------------------------------------
GEMM_ROUTES = {
    "tile64": dict(opts={}, M=200, K=136, splitk=1, expect="gemm_conv_kernel<64,64,"),
    "tile128": dict(opts=dict(GEMM_BM=128, GEMM_BN=128), M=300, K=136, splitk=1, expect="gemm_conv_kernel<128,128,"),
    "ws": dict(opts={}, M=8200, K=320, splitk=0, expect="gemm_ws_kernel<plain>"),
    "xl": dict(opts=dict(GEMM_XL=2), M=520, K=128, splitk=0, expect="gemm_xl_kernel<256x"),
    "splitk": dict(opts={}, M=100, K=1024, splitk=3, expect="gemm_conv_kernel<"),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("route", list(GEMM_ROUTES))
def test_gemm_narrow_c_and_r_views(dev, route, dtype):
    """C starts 4 elements into a wider buffer (8-byte, not 16-byte aligned), ldc % 8 == 4, N % 8 == 4; R likewise with its own offset and
    pitch: the 8-byte epilogue of each main loop (the 16-byte one must not be taken)."""
    r = GEMM_ROUTES[route]
    M, K, N = r["M"], r["K"], 132
    A = rnd(M, K, seed=1, dtype=dtype); W = rnd(N, K, scale=K ** -0.5, seed=2, dtype=dtype)
    b = side(N, 4, 3, dev)
    C = Guarded((M, N), 140, 4, dtype, dev)
    R = Guarded((M, N), 148, 12, dtype, dev, fill=rnd(M, N, seed=4, dtype=dtype))
    ws = torch.full((1 << 18,), NAN, dtype=F32, device=dev)
    with L.options(**r["opts"]):
        O.run_ops([O.Gemm(A, W, C.view, bias=b, R=R.view, splitk=r["splitk"], ws=ws)])
        kern = last_kernel()
    torch.cuda.synchronize()
    assert kern.startswith(r["expect"]), kern
    if route == "splitk":
        assert not torch.isnan(ws[:3 * M * N]).any() and torch.isnan(ws[3 * M * N:]).all(), "three fp32 slabs expected in the workspace"
    ref = A.float().cpu() @ W.float().cpu().T + b.cpu() + R.view.float().cpu()
    close(C.view, ref, name=f"edge gemm narrow C/R {route}", kind=KIND[dtype])
    assert C.border_intact() and R.border_intact()


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("sk,slabs", [(1, 0), (2, 2), (5, 5), (0, 4)])
def test_gemm_fp32_c_with_residual_through_splitk(dev, sk, slabs, dtype):
    """fp32 C WITH an fp32 residual through split-K 1, forced 2 and 5 and the automatic choice (4 slabs here), bias and a temb table row
    chosen through sel_ptr.  Alignments are the weakest the contract allows: C, R, bias, temb 16 bytes into their buffers, ldc / ldr / the
    temb strides multiples of 4 only, rows_per_b = 50 (divides no tile).  The number of slabs found in the workspace pins the split."""
    M, N, K = 96, 132, 2048
    A = rnd(M, K, seed=1, dtype=dtype); W = rnd(N, K, scale=K ** -0.5, seed=2, dtype=dtype)
    b = side(N, 4, 3, dev)
    tbs, tss = 136, 2 * 136 + 4
    tbuf = torch.full((4 + 3 * tss + 8,), NAN, dtype=F32, device=dev)
    temb = tbuf[4:4 + 3 * tss]
    tab = rnd(3, 2, N, seed=5, dtype=F32)
    for s_ in range(3):
        for bb in range(2):
            temb[s_ * tss + bb * tbs: s_ * tss + bb * tbs + N] = tab[s_, bb]
    sel = torch.tensor([2], dtype=torch.int32, device=dev)
    C = Guarded((M, N), 136, 4, F32, dev)
    R = Guarded((M, N), 140, 8, F32, dev, fill=rnd(M, N, seed=4, dtype=F32))
    ws = torch.full((1 << 18,), NAN, dtype=F32, device=dev)
    O.run_ops([O.Gemm(A, W, C.view, bias=b, R=R.view, temb=temb, sel=sel, temb_sel_stride=tss, temb_b_stride=tbs, rows_per_b=50, splitk=sk, ws=ws)])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern.startswith("gemm_conv_kernel<"), kern
    assert not torch.isnan(ws[:slabs * M * N]).any() and torch.isnan(ws[slabs * M * N:]).all(), f"{slabs} fp32 slabs expected in the workspace"
    ref = A.double().cpu() @ W.double().cpu().T + b.double().cpu() + tab[2].double().cpu().repeat_interleave(50, 0)[:M] + R.view.double().cpu()
    assert torch.isfinite(C.view).all()
    check(f"edge gemm fp32 C+R split-K {sk} {KIND[dtype]} rel_l2", rel_l2(C.view, ref), 2e-5)
    assert C.border_intact() and R.border_intact()


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_gemm_batched_with_strides_bias_residual(dev, dtype):
    """batch > 1 with sA != 0, bias, R with sR and C with sC at the weakest allowed multiples (sC, sR % 8 == 4; sA % 16 == 8)."""
    Bt, M, N, K = 3, 70, 68, 72
    ldc, ldr = 76, 84
    Abuf = rnd(Bt * (M * K + 8), seed=1, dtype=dtype)
    A = Abuf.as_strided((Bt, M, K), (M * K + 8, K, 1))
    W = rnd(Bt, N, K, scale=K ** -0.5, seed=2, dtype=dtype)
    b = side(N, 4, 3, dev)
    Cb = torch.full((Bt * (M * ldc + 4) + 16,), NAN, dtype=dtype, device=dev)
    C = Cb.as_strided((Bt, M, N), (M * ldc + 4, ldc, 1), 4)
    Rb = torch.full((Bt * (M * ldr + 4) + 16,), NAN, dtype=dtype, device=dev)
    R = Rb.as_strided((Bt, M, N), (M * ldr + 4, ldr, 1), 4)
    R.copy_(rnd(Bt, M, N, seed=4, dtype=dtype))
    O.run_ops([O.Gemm(A, W, C, bias=b, R=R)])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern.startswith("gemm_conv_kernel<"), kern
    ref = torch.einsum("bmk,bnk->bmn", A.float().cpu(), W.float().cpu()) + b.cpu() + R.float().cpu()
    close(C, ref, name="edge gemm batched strides", kind=KIND[dtype])
    mask = torch.ones_like(Cb, dtype=torch.bool)
    mask.as_strided(C.shape, C.stride(), 4).fill_(False)
    assert torch.isnan(Cb[mask].float()).all()


# --------------------------------------------------------------------------------------------------------------------------------------
# row statistics under every route, and producer -> consumer
# --------------------------------------------------------------------------------------------------------------------------------------
ROWSTAT_ROUTES = {
    # forced XL leaves K = 320 to the weight-stationary kernel: ONE routing decision serves the statistics branch and the launch
    "xl2": dict(opts=dict(GEMM_XL=2), M=8400, N=320, splitk=0, kern="gemm_ws_kernel<plain,rs>"),
    "xl_k320": dict(opts=dict(XL_K320=1), M=8400, N=320, splitk=0, kern="rowstat_kernel"),
    "ws2_small_m": dict(opts=dict(GEMM_WS=2), M=300, N=320, splitk=0, kern="gemm_ws_kernel<plain,rs>"),
    "ln_fuse0": dict(opts=dict(LN_FUSE=0), M=8400, N=320, splitk=0, kern="rowstat_kernel"),
    "splitk": dict(opts={}, M=300, N=320, splitk=2, kern="rowstat_kernel"),
    "narrow_c": dict(opts={}, M=8300, N=324, splitk=0, kern="rowstat_kernel"),       # N % 8 != 0, C 8 bytes into its buffer: the element loop
}


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("route", list(ROWSTAT_ROUTES))
def test_rowstat_out_under_forced_routes(dev, route, dtype):
    """rowstat_out under the routes test_gemm_row_statistics_out does not force; the statistics buffer starts as NaN, so a route that
    ignored it (or zeroed too little) shows.  fp64 sums of the STORED C, the 2e-5 relative bound of that test, unused parts exactly zero."""
    r = ROWSTAT_ROUTES[route]
    M, N, K, parts = r["M"], r["N"], 320, 4
    A = rnd(M, K, seed=1, dtype=dtype); W = rnd(N, K, scale=K ** -0.5, seed=2, dtype=dtype); b = rnd(N, seed=3, dtype=F32)
    narrow = route == "narrow_c"
    C = Guarded((M, N), N + 12 if narrow else N, 4 if narrow else 0, dtype, dev)
    st = torch.full((parts, M, 2), NAN, dtype=F32, device=dev)
    ws = torch.empty(1 << 20, dtype=F32, device=dev)
    with L.options(**r["opts"]):
        O.run_ops([O.Gemm(A, W, C.view, bias=b, rowstat=st, splitk=r["splitk"], ws=ws)])
        kern = last_kernel()
    torch.cuda.synchronize()
    assert kern == r["kern"], kern
    close(C.view, A.float().cpu() @ W.float().cpu().T + b.cpu(), name=f"edge rowstat C {route}", kind=KIND[dtype])
    assert C.border_intact()
    got = st.double().cpu()
    assert torch.isfinite(got).all(), "statistics buffer not fully written"
    nt = (N + 127) // 128 if kern.startswith("gemm_ws") else 1
    cols = [(128 * k, min(N, 128 * k + 128)) for k in range(nt)] if nt > 1 else [(0, N)]
    want = rowstat_ref(C.view, cols)
    assert (got[nt:] == 0).all(), "unused parts must be exactly zero"
    check(f"edge rowstat {route} {KIND[dtype]}", ((got[:nt] - want).abs() / (want.abs() + 1.0)).max().item(), 2e-5)


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_rowstat_out_behind_the_w_direct_kernel(dev, dtype):
    """XD = 1 with Wq at a shape the persistent 256-wide form takes (>= 2 x CUs tiles, 16-byte C rows): the W-direct kernel cannot emit the
    statistics and must never see the pointer — the GEMM runs on it exactly as without rowstat_out (bit-identical C), rowstat_kernel
    follows: part 0 = whole rows, the other parts exactly zero."""
    M, N, K, parts = 70000, 1280, 640, 4
    A = rnd(M, K, scale=0.5, seed=1, dtype=dtype); W = rnd(N, K, scale=0.05, seed=2, dtype=dtype); b = rnd(N, seed=3, dtype=F32)
    Wq = PK.pack_wq(W)
    ws = torch.empty(1 << 22, dtype=F32, device=dev)
    C0 = torch.full((M, N), NAN, dtype=dtype, device=dev); C = torch.full((M, N), NAN, dtype=dtype, device=dev)
    st = torch.full((parts, M, 2), NAN, dtype=F32, device=dev)
    with L.options(XD=1):
        O.run_ops([O.Gemm(A, W, C0, bias=b, ws=ws, Wq=Wq)])
        k0 = last_kernel()
        O.run_ops([O.Gemm(A, W, C, bias=b, ws=ws, Wq=Wq, rowstat=st)])
        k1 = last_kernel()
    torch.cuda.synchronize()
    assert k0.startswith("gemm_xd_kernel<256x256,gemm>") and k1 == "rowstat_kernel", (k0, k1)
    assert torch.equal(C, C0), "rowstat_out changed the GEMM's route"
    idx = torch.randint(0, M, (2048,), generator=torch.Generator().manual_seed(5)); idx[:8] = torch.arange(M - 8, M)
    idx = idx.to(dev)
    close(C[idx], A[idx].float().cpu() @ W.float().cpu().T + b.cpu(), name="edge rowstat C xd", kind=KIND[dtype])
    assert torch.isfinite(st).all() and (st[1:] == 0).all(), "part 0 + exact zeros expected"
    want = rowstat_ref(C[idx], [(0, N)])
    check(f"edge rowstat xd {KIND[dtype]}", ((st[:1, idx].double().cpu() - want).abs() / (want.abs() + 1.0)).max().item(), 2e-5)


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("consumer", ["plain", "vT", "geglu"])
@pytest.mark.parametrize("producer", ["ws", "rowstat_kernel"])
def test_rowstat_producer_feeds_fused_layernorm_consumer(dev, producer, consumer, dtype):
    """One program: a GEMM with rowstat_out, then the GEMM that carries the LayerNorm of its output and reads those statistics through
    ln_stats — a plain projection, the fused q/k + transposed-V projection, and the GEGLU projection (which fuses ONLY with producer
    statistics) — once behind the weight-stationary producer (one part per 128-column tile), once behind a split-K producer
    (rowstat_kernel: part 0 + zeros).  Reference: LayerNorm -> Linear (-> GEGLU / V^T scatter) in fp32 on the producer's STORED output."""
    Bv, T, K = 6, 1400, 320
    M = Bv * T
    A0 = rnd(M, K, seed=1, dtype=dtype); W0 = rnd(K, K, scale=K ** -0.5, seed=2, dtype=dtype); b0 = rnd(K, seed=3, dtype=F32) + 0.5
    gamma = 1.0 + rnd(K, scale=0.3, seed=5, dtype=F32, dev="cpu"); beta = rnd(K, scale=0.3, seed=6, dtype=F32, dev="cpu")
    X = torch.full((M, K), NAN, dtype=dtype, device=dev)
    st = torch.full((3, M, 2), NAN, dtype=F32, device=dev)
    scratch = torch.full((M, K), NAN, dtype=dtype, device=dev)
    ws = torch.empty(M * K * 2 + 1024, dtype=F32, device=dev)
    first = O.Gemm(A0, W0, X, bias=b0, rowstat=st, splitk=2 if producer != "ws" else 0, ws=ws)
    if consumer == "plain":
        N = 328
        W = rnd(N, K, scale=K ** -0.5, seed=4, dtype=F32, dev="cpu")
        Wp, b, cs = ln_fold(W, gamma, beta, dtype)
        C = torch.full((M, N), NAN, dtype=dtype, device=dev)
        second = O.Gemm(X, Wp.to(dev), C, bias=b.to(dev), ln_eps=1e-5, ln_csum=cs.to(dev), ln_scratch=scratch, ln_stats=st, ws=ws)
        expect = "gemm_ws_kernel<plain,lns>"
    elif consumer == "vT":
        W = rnd(3 * K, K, scale=K ** -0.5, seed=4, dtype=F32, dev="cpu")
        Wp, b, cs = ln_fold(W, gamma, beta, dtype)
        C = torch.full((M, 2 * K), NAN, dtype=dtype, device=dev)
        Vt = torch.full((Bv, K, T), NAN, dtype=dtype, device=dev)
        second = O.Gemm(X, Wp.to(dev), C, bias=b.to(dev), Vt=Vt, vt_from=2 * K, vt_T=T, ln_eps=1e-5, ln_csum=cs.to(dev), ln_stats=st)
        expect = "gemm_ws_kernel<vT,lns>"
    else:
        F_ = 320
        W = rnd(2 * F_, K, scale=K ** -0.5, seed=4, dtype=F32, dev="cpu"); bl = rnd(2 * F_, seed=7, dtype=F32, dev="cpu")
        Wf, bf_ = W * gamma[None, :], bl + W @ beta
        Wp, bp = PK.pack_geglu(Wf, bf_, dtype)
        C = torch.full((M, F_), NAN, dtype=dtype, device=dev)
        second = O.Gemm(X, Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU, ln_eps=1e-5, ln_csum=Wp.float().sum(1).to(dev), ln_scratch=scratch,
                        ln_stats=st, ws=ws)
        expect = "gemm_ws_kernel<geglu,lns>"
    prog = O.build_program([first, second])
    prog.run(torch.cuda.current_stream().cuda_stream)
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern == expect and torch.isnan(scratch.float()).all(), kern
    s_ = st.cpu()
    assert torch.isfinite(s_).all()
    assert (s_[1:] != 0).any() if producer == "ws" else (s_[1:] == 0).all()
    tag = f"edge rowstat -> ln_stats chain ({producer} -> {consumer})"
    if consumer == "plain":
        close(C, ln_ref(X, Wp, b), name=tag, kind=KIND[dtype])
    elif consumer == "vT":
        ref = ln_ref(X, Wp, b)
        close(C, ref[:, :2 * K], name=tag + " qk", kind=KIND[dtype])
        close(Vt, ref[:, 2 * K:].reshape(Bv, T, K).transpose(1, 2), name=tag + " V^T", kind=KIND[dtype])
    else:
        h, g = ln_ref(X, Wf.to(dtype), bf_).chunk(2, dim=-1)
        close(C, h * F.gelu(g), name=tag, kind=KIND[dtype])


# --------------------------------------------------------------------------------------------------------------------------------------
# direct conv
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_conv_direct_cout8_kpar_and_misaligned_view(dev, dtype):
    """Cout = 8 with K = 9 x 64: conv_direct_kpar_kernel<8>; the same problem through an X view with ldx % 8 != 0 must land on
    conv_direct_simple_kernel and agree.  SiLU epilogue, temb row through sel_ptr, residual."""
    B, H, Wd, Cin, Cout = 2, 9, 7, 64, 8
    x = rnd(B, H, Wd, Cin, seed=1, dtype=dtype)
    Wt = rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, seed=2, dtype=dtype)
    b = side(Cout, 1, 3, dev)
    temb = rnd(3, B, Cout, seed=5, dtype=F32); sel = torch.tensor([1], dtype=torch.int32, device=dev)
    Rr = rnd(B, H, Wd, Cout, seed=4, dtype=dtype)
    ref = F.conv2d(x.float().cpu().permute(0, 3, 1, 2), Wt.float().cpu().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    ref = F.silu(ref + b.cpu() + temb[1].cpu()[:, None, None, :]) + Rr.float().cpu()
    outs = []
    for ldx, expect in ((Cin, "conv_direct_kpar_kernel"), (Cin + 4, "conv_direct_simple_kernel")):
        X = Guarded((B, H, Wd, Cin), ldx, 0, dtype, dev, fill=x)
        Y = Guarded((B, H, Wd, Cout), 12, 3, dtype, dev)
        O.run_ops([O.Conv(X.view, Wt, Y.view, bias=b, R=Rr, temb=temb, sel=sel, temb_sel_stride=B * Cout, temb_b_stride=Cout,
                          epilogue=L.EPI_SILU, direct=True)])
        kern = last_kernel()
        torch.cuda.synchronize()
        assert kern == expect, kern
        close(Y.view, ref, name=f"edge conv direct Cout=8 {expect}", kind=KIND[dtype])
        assert Y.border_intact()
        outs.append(Y.view.float().cpu())
    check(f"edge conv direct kpar vs simple {KIND[dtype]}", rel_l2(outs[0], outs[1]), 4e-3 if dtype == torch.bfloat16 else 6e-4)   # one storage rounding


# --------------------------------------------------------------------------------------------------------------------------------------
# norms
# --------------------------------------------------------------------------------------------------------------------------------------
def gn_ref(x, G, gamma, beta, eps, silu):
    xf = x.double().cpu()
    B, HW, Cc = xf.shape
    y = F.group_norm(xf.transpose(1, 2), G, gamma.double().cpu(), beta.double().cpu(), eps).transpose(1, 2)
    return F.silu(y) if silu else y


# (C, G, ld, off): the widest vector that divides C / G, ld and the view's byte offset is 4, 2 or 1 elements
# (the "cpg" cases keep C % 8 != 0 so that the two-stage path has to decline them too)
GN_CASES = [("cpg12", 36, 3, 36, 0), ("cpg6", 18, 3, 18, 0), ("cpg5", 20, 4, 20, 0), ("cpg4", 12, 3, 12, 0), ("cpg2", 6, 3, 6, 0), ("cpg1", 3, 3, 3, 0),
            ("view+4", 64, 4, 80, 4), ("view+2", 64, 4, 80, 2), ("view+1", 64, 4, 80, 1),
            ("ld%8=4", 64, 4, 68, 0), ("ld%8=2", 64, 4, 66, 0), ("ld odd", 64, 4, 65, 0)]


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("case,Cc,G,ld,off", GN_CASES, ids=[c[0] for c in GN_CASES])
def test_groupnorm_narrow_vector_widths(dev, case, Cc, G, ld, off, dtype):
    """GroupNorm at vector widths 4, 2 and 1, reached by channels per group, by a channel-slice view and by the row pitch; |mean| >> std.
    With a workspace and the one-launch size limit switched off the two-stage path must decline every one of them (it needs 16-byte rows)
    and the result must not change by a bit."""
    B, HW = 2, 40000 // Cc
    x = (rnd(B, HW, Cc, seed=1, dtype=F32) * 0.5 + 20.0).to(dtype)
    gamma = side(Cc, 4, 2, dev, shift=1.0); beta = side(Cc, 4, 3, dev)        # both 16 bytes into their buffers: the weakest allowed
    assert gamma.data_ptr() % 32 == 16 and beta.data_ptr() % 32 == 16
    X = Guarded((B, HW, Cc), ld, off, dtype, dev, fill=x)
    ws = torch.empty(1 << 18, dtype=F32, device=dev)
    outs = []
    for use_ws in (False, True):
        Y = Guarded((B, HW, Cc), ld, off, dtype, dev)
        with L.options(GN_ONE_KERNEL_ELEMS=0):
            O.run_ops([O.GroupNorm(X.view, Y.view, gamma, beta, G, 1e-5, silu=True, ws=ws if use_ws else None)])
            kern = last_kernel()
        torch.cuda.synchronize()
        assert HW * Cc >= 32768 and (Cc % 8 or ld % 8 or off % 8), "every case must be one the two-stage path would take but for its alignment"
        assert kern == "groupnorm_kernel", kern
        close(Y.view, gn_ref(x, G, gamma, beta, 1e-5, True), name=f"edge groupnorm {case} ws={use_ws}", kind=KIND[dtype])
        assert Y.border_intact()
        outs.append(Y.view.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_groupnorm_more_channels_per_group_than_the_lds_table(dev, dtype):
    """4096 channels in one group (> GN_MAX_CPG = 2560): with a workspace the two-stage path serves it; without one the documented
    MDX_EUNSUPPORTED comes back (the limit belongs to the one-launch kernel only)."""
    B, HW, Cc, G = 2, 24, 4096, 1
    x = (rnd(B, HW, Cc, seed=1, dtype=F32) * 0.7 + 1.5).to(dtype)
    gamma = rnd(Cc, seed=2, dtype=F32) + 1.0; beta = rnd(Cc, seed=3, dtype=F32)
    y = torch.full_like(x, NAN)
    ws = torch.empty(1 << 18, dtype=F32, device=dev)
    with L.options(GN_ONE_KERNEL_ELEMS=0):
        O.run_ops([O.GroupNorm(x, y, gamma, beta, G, 1e-5, ws=ws)])
        kern = last_kernel()
        torch.cuda.synchronize()
        with pytest.raises(L.MdxError, match="channels per group"):
            O.run_ops([O.GroupNorm(x, y, gamma, beta, G, 1e-5)])
    assert kern == "gn_stats_kernel+gn_apply_kernel", kern
    close(y, gn_ref(x, G, gamma, beta, 1e-5, False), name="edge groupnorm cpg 4096 two-stage", kind=KIND[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_layernorm_row_views_with_guard_columns(dev, dtype):
    M, Cc = 37, 64
    x = (rnd(M, Cc, seed=1, dtype=F32) * 1.3 + 0.6).to(dtype)
    gamma = side(Cc, 4, 2, dev, shift=1.0); beta = side(Cc, 4, 3, dev)
    assert gamma.data_ptr() % 32 == 16 and beta.data_ptr() % 32 == 16
    X = Guarded((M, Cc), 80, 8, dtype, dev, fill=x)
    Y = Guarded((M, Cc), 72, 8, dtype, dev)
    O.run_ops([O.LayerNorm(X.view, Y.view, gamma, beta, 1e-5)])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern == "layernorm_kernel", kern
    ref = F.layer_norm(x.double().cpu(), (Cc,), gamma.double().cpu(), beta.double().cpu(), 1e-5)
    close(Y.view, ref, name="edge layernorm row views", kind=KIND[dtype])
    assert Y.border_intact()


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_softmax_rows_ragged_large_scores(dev, dtype):
    """T % 64 != 0, rows % 4 != 0, ldy > T (pad columns written as zeros), |scale * x| up to ~80, one row of equal scores; fp64 reference."""
    rows, T, ldx, ldy, scale = 7, 77, 96, 80, 0.125
    x = rnd(rows, ldx, seed=1, dtype=F32, scale=160.0).clamp(-640, 640)
    x[3, :] = 5.0
    Yb = torch.full((rows + 4, ldy), NAN, dtype=dtype, device=dev)
    Y = Yb[2:2 + rows]
    O.run_ops([O.Softmax(x, Y, T, scale)])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern == "softmax_rows_kernel", kern
    ref = torch.zeros(rows, ldy, dtype=torch.float64)
    ref[:, :T] = (x[:, :T].double().cpu() * scale).softmax(-1)
    assert (Y[:, T:] == 0).all() and torch.isnan(Yb[:2].float()).all() and torch.isnan(Yb[2 + rows:].float()).all()
    close(Y, ref, name="edge softmax ragged large scores", kind=KIND[dtype])


# --------------------------------------------------------------------------------------------------------------------------------------
# element-wise
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("Cc", [40, 36])
@pytest.mark.parametrize("kind", ["ADD", "COPY", "SILU", "SCALE"])
def test_elementwise_scalar_and_vec8_agree_bitwise(dev, kind, Cc, dtype):
    """16-bit ADD / COPY / SILU / SCALE on ew_vec8_kernel and, through views one element into a wider buffer, on ew_scalar_kernel: the same
    arithmetic in the same order, so equal bit for bit; and against the fp32 reference.  C = 36 (C % 8 != 0) takes the scalar kernel even
    for contiguous, 16-byte aligned tensors."""
    M = 33
    code = {"ADD": L.EW_ADD, "COPY": L.EW_COPY, "SILU": L.EW_SILU, "SCALE": L.EW_SCALE}[kind]
    x = rnd(M, Cc, seed=1, dtype=dtype, scale=2.0); y0 = rnd(M, Cc, seed=2, dtype=dtype)
    xf, yf = x.float().cpu(), y0.float().cpu()
    ref = {"ADD": yf + xf, "COPY": xf, "SILU": F.silu(xf), "SCALE": xf * 0.37}[kind]
    outs = []
    for ld, off, expect in ((Cc, 0, "ew_vec8_kernel" if Cc % 8 == 0 else "ew_scalar_kernel"), (Cc + 3, 1, "ew_scalar_kernel")):
        X = Guarded((M, Cc), ld, off, dtype, dev, fill=x)
        Y = Guarded((M, Cc), ld, off, dtype, dev, fill=y0 if kind == "ADD" else None)
        O.run_ops([O.Ew(code, X.view, Y.view, alpha=0.37)])
        kern = last_kernel()
        torch.cuda.synchronize()
        assert kern == expect, kern
        close(Y.view, ref, name=f"edge ew {kind} C={Cc} off={off} {expect}", kind=KIND[dtype])
        assert Y.border_intact()
        outs.append(Y.view.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_elementwise_type_conversions_and_layouts(dev, dtype):
    """fp32 -> 16-bit and 16-bit -> fp32 copies, NCHW <-> NHWC in both directions for 16-bit and mixed types with odd C, H, W."""
    M, Cc = 9, 13
    xf = rnd(M, Cc, seed=1, dtype=F32); xh = xf.to(dtype)
    Yh = Guarded((M, Cc), 17, 1, dtype, dev); Yf = Guarded((M, Cc), 15, 1, F32, dev)
    O.run_ops([O.Ew(L.EW_COPY, xf, Yh.view)])
    assert last_kernel() == "ew_scalar_kernel"
    O.run_ops([O.Ew(L.EW_COPY, xh, Yf.view)])
    assert last_kernel() == "ew_scalar_kernel"
    torch.cuda.synchronize()
    close(Yh.view, xf, name="edge ew fp32->16", kind=KIND[dtype])
    assert torch.equal(Yf.view, xh.float()) and Yh.border_intact() and Yf.border_intact()
    B, Cn, H, Wd = 2, 5, 7, 3
    for src_t, dst_t in ((dtype, dtype), (F32, dtype), (dtype, F32)):
        nchw = rnd(B, Cn, H, Wd, seed=2, dtype=src_t)
        Yv = Guarded((B, H, Wd, Cn), 7, 1, dst_t, dev)
        O.run_ops([O.Layout(nchw, Yv.view, True)])
        assert last_kernel() == "ew_scalar_kernel"
        torch.cuda.synchronize()
        want = nchw.permute(0, 2, 3, 1)
        if dst_t == F32 or src_t == dst_t:
            assert torch.equal(Yv.view.float(), want.float())
        else:
            close(Yv.view, want, name="edge layout fp32 nchw -> 16-bit nhwc", kind=KIND[dtype])
        assert Yv.border_intact()
        Xv = Guarded((B, H, Wd, Cn), 7, 1, src_t, dev, fill=want)
        back = torch.full((B, Cn, H, Wd), NAN, dtype=dst_t, device=dev)
        O.run_ops([O.Layout(Xv.view, back, False)])
        assert last_kernel() == "ew_scalar_kernel"
        torch.cuda.synchronize()
        if dst_t == F32 or src_t == dst_t:
            assert torch.equal(back.float(), nchw.float())
        else:
            close(back, nchw, name="edge layout fp32 nhwc -> 16-bit nchw", kind=KIND[dtype])


# --------------------------------------------------------------------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------------------------------------------------------------------
ATTN_REFUSED = (104, 112, 136, 144)         # include/mdx.h: no kernel instance for ceil(d / 16) = 7, 9 (tests/test_contract.py pins the code)


def _attn_case(dev, dtype, B, H, Tq, Tk, d, qk_halves=False):
    Cc = H * d
    q = rnd(B, Tq, Cc, seed=1, dtype=dtype); k = rnd(B, Tk, Cc, seed=2, dtype=dtype); v = rnd(B, Tk, Cc, seed=3, dtype=dtype)
    if qk_halves:                            # Q and K as the halves of one buffer (self-attention: Tq == Tk)
        qk = torch.cat([q, k], dim=2)
        Qv, Kv = qk[:, :, :Cc], qk[:, :, Cc:]
    else:                                    # rows wider than H * d, NaN beyond the last head
        Qv = Guarded((B, Tq, Cc), Cc + 8, 0, dtype, dev, fill=q).view
        Kv = Guarded((B, Tk, Cc), Cc + 8, 0, dtype, dev, fill=k).view
    ldv = (Tk + 7) // 8 * 8 + 8
    vt = torch.full((B, Cc, ldv), NAN, dtype=dtype, device=dev)          # NaN in the kv pad
    vt[:, :, :Tk] = v.transpose(1, 2)
    Ov = Guarded((B, Tq, Cc), Cc + 12, 4, dtype, dev)                    # ldo % 8 == 4, O 8 bytes into its buffer
    ref = ref_attention(q.float().cpu(), k.float().cpu(), v.float().cpu(), H, d ** -0.5)
    return Qv, Kv, vt, Ov, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("d", [24, 48, 56, 72, 88, 104, 112, 120, 136, 144, 152])
def test_attention_every_head_dim_the_header_promises(dev, d, dtype):
    """Every d % 8 == 0 up to 160 that test_attention does not run, ragged Tq x Tk = 130 x 77, NaN in the kv pad and beyond the last head of
    the Q / K rows, O as an 8-byte aligned view with ldo % 8 == 4 and NaN guards: a padded 16-column chunk that reads or writes past d shows.
    The four head dims without a kernel instance return the documented MDX_EUNSUPPORTED."""
    B, H, Tq, Tk = 1, 2, 130, 77
    Qv, Kv, vt, Ov, ref = _attn_case(dev, dtype, B, H, Tq, Tk, d)
    assert Ov.view.stride(1) % 8 == 4 and Ov.view.data_ptr() % 16 == 8
    op = O.Attn(Qv, Kv, vt, Ov.view, heads=H, Tk=Tk, scale=d ** -0.5)
    if d in ATTN_REFUSED:
        with pytest.raises(L.MdxError, match="no kernel instance"):
            O.run_ops([op])
        return
    O.run_ops([op])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern.startswith(f"attn_kernel<{(d + 15) // 16},"), kern
    close(Ov.view, ref, name=f"edge attn d={d}", kind=KIND[dtype])
    assert Ov.border_intact()


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("B,d,T,prefix", [(2, 64, 130, "attn_kernel<4,"), (6, 40, 300, "attn2_kernel<40,self,q32>")])
def test_attention_o_view_ldo_4_mod_8_qk_halves(dev, B, d, T, prefix, dtype):
    """O with ldo % 8 == 4 at an 8-byte offset, Q and K as halves of one buffer: the generic kernel and the head-dim-40 kernel."""
    H = 8                                    # the head-dim-40 kernel wants ceil(T / 128) * H * B >= 128 workgroups
    Qv, Kv, vt, Ov, ref = _attn_case(dev, dtype, B, H, T, T, d, qk_halves=True)
    assert Ov.view.stride(1) % 8 == 4 and Ov.view.data_ptr() % 16 == 8
    O.run_ops([O.Attn(Qv, Kv, vt, Ov.view, heads=H, Tk=T, scale=d ** -0.5)])
    kern = last_kernel()
    torch.cuda.synchronize()
    assert kern.startswith(prefix), kern
    close(Ov.view, ref, name=f"edge attn O view d={d}", kind=KIND[dtype])
    assert Ov.border_intact()
