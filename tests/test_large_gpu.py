"""-m gpu: every kernel on tensors that cross 2^31 bytes, 2^32 bytes or 2^31 elements.

The fast main loops read through buffer descriptors with a 2 GiB window (xl_dma.h, attention2.hip, gemm_ws.hip: loads past the window return
zeros, silently) and every kernel mixes int and long index arithmetic by hand; the other kernel suites stop at 688 MB.  A full fp32 reference
of a 4 GiB tensor does not fit a test, and every op here is independent per row / image / batch item, so the inputs are PERIODIC: a small
random base, expanded on the GPU by an index (row m = base[m % P], P = 4099 rows — prime, no common factor with the 128 / 256-row tiles — or
image b = base[b % P], P = 3 or 5 images whose pixel count is no multiple of 128).  The plain fp32 reference of the base, expanded by the same
index, then checks EVERY element of the big output (helpers.close_periodic: the three limits of helpers.close over the whole tensor); where the
reduction order of a row does not depend on its position, rows m and m + P must also be bit-identical.  Outputs sit between NaN guard rows
(64 rows / one image on each side) and are NaN-filled before the launch; every case asserts the kernel the library reports and the size of the
tensor that crosses the mark.  bf16 only: the index arithmetic is shared with the _f16 instantiations.
"""
import gc

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import close_periodic, periodic_mismatch  # noqa: E402
from magicdrive_amd import _lib as L  # noqa: E402
from magicdrive_amd import ops as O  # noqa: E402
from magicdrive_amd import packing as PK  # noqa: E402

BF = torch.bfloat16
NAN = float("nan")
G2, G4, E31 = 2 ** 31, 2 ** 32, 2 ** 31
P_ROWS = 4099
M_BIG = 1_680_017                        # x 1280 columns of 16 bits = 4.30 GB: past 2^31 B, 2^32 B and 2^31 elements


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)


def ws_buf(mb=64):
    return torch.empty(mb * 1024 * 1024 // 4, dtype=torch.float32, device="cuda")


def nbytes(t):
    return t.numel() * t.element_size()


def need(gb):
    """Skip only when the device shows less free memory than this case states it needs."""
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < gb * 1e9:
        pytest.skip(f"needs {gb} GB of free device memory, {free / 1e9:.1f} GB free")


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def expand(base, n, period=None):
    """[n, ...] with slice m = base[m % period]."""
    period = base.shape[0] if period is None else period
    return base.index_select(0, torch.arange(n, device=base.device) % period)


def guarded(shape, dtype, g):
    """(whole allocation, view of `shape`) with g NaN guard slices along dim 0 on each side; the view is NaN-filled too."""
    full = torch.full((shape[0] + 2 * g, *shape[1:]), NAN, dtype=dtype, device="cuda")
    return full, full[g:g + shape[0]]


def guards_intact(full, g):
    return bool(torch.isnan(full[:g]).all()) and bool(torch.isnan(full[-g:]).all())


def run_one(op, **opts):
    with L.options(**opts):
        O.run_ops([op])
        k = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    return k


def bit_periodic(out, period, name):
    n, first = periodic_mismatch(out, period)
    assert n == 0, f"{name}: {n} dim-0 slices differ from the slice one period ({period}) earlier, first at {first}"


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM
def gemm_base(K, N, bias=True, res=False, P=P_ROWS, res_dtype=BF):
    A = rnd(P, K, seed=1); W = rnd(N, K, scale=K ** -0.5, seed=2)
    b = rnd(N, seed=3, dtype=torch.float32) if bias else None
    R = rnd(P, N, seed=4, dtype=res_dtype) if res else None
    ref = A.float() @ W.float().T
    if bias: ref += b
    if res: ref += R.float()
    return A, W, b, R, ref


@pytest.mark.parametrize("inplace", [False, True])
def test_gemm_ws_k320_c_crosses_4g(dev, inplace):
    """Case 1: weight-stationary K = 320 -> N = 1280 with bias; plain, and with the residual aliased to C."""
    need(8)
    M, K, N = M_BIG, 320, 1280
    Ab, W, b, Rb, ref = gemm_base(K, N, res=inplace)
    A = expand(Ab, M)
    full, C = guarded((M, N), BF, 64)
    R = None
    if inplace:
        C.copy_(expand(Rb, M)); R = C
    assert nbytes(C) > G4 and C.numel() > E31
    k = run_one(O.Gemm(A, W, C, bias=b, R=R, ws=ws_buf()))
    assert k == "gemm_ws_kernel<plain>", k
    assert guards_intact(full, 64), "wrote outside the C view"
    close_periodic(C, ref, P_ROWS, name=f"large ws gemm 320->1280 inplace={inplace}")
    bit_periodic(C, P_ROWS, "ws gemm")


def test_gemm_ws_geglu_c_crosses_4g(dev):
    """Case 2: weight-stationary GEGLU, 2560 packed weight rows, C 1280 wide."""
    need(8)
    M, K, F_ = M_BIG, 320, 1280
    Ab = rnd(P_ROWS, K, seed=1)
    W = rnd(2 * F_, K, scale=K ** -0.5, seed=2, dtype=torch.float32); b = rnd(2 * F_, seed=3, dtype=torch.float32)
    Wp, bp = PK.pack_geglu(W.cpu(), b.cpu(), BF)
    h, g = (Ab.float() @ W.to(BF).float().T + b).chunk(2, dim=-1)
    ref = h * F.gelu(g)
    A = expand(Ab, M)
    full, C = guarded((M, F_), BF, 64)
    assert nbytes(C) > G4 and C.numel() > E31
    k = run_one(O.Gemm(A, Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU, ws=ws_buf()))
    assert k == "gemm_ws_kernel<geglu>", k
    assert guards_intact(full, 64)
    close_periodic(C, ref, P_ROWS, name="large ws geglu 320->1280")
    bit_periodic(C, P_ROWS, "ws geglu")


@pytest.mark.parametrize("ln", [False, True])
def test_gemm_fused_qkv_transposed_v_qk_crosses_2g(dev, ln):
    """Case 3: fused q/k/v with transposed V, 1199 views of 1400 tokens (periodic by whole views, P = 3): qk [M, 640] = 2.15 GB;
    without and with the fused LayerNorm (in-kernel statistics)."""
    import test_kernels_gpu as T
    need(7)
    Bv, Tt, Cc, Pv = 1199, 1400, 320, 3
    M, P = Bv * Tt, Pv * Tt
    if ln:
        xb = (rnd(P, Cc, scale=1.3, seed=1).float() - 0.4).to(BF)
        W = rnd(3 * Cc, Cc, scale=Cc ** -0.5, seed=2, dtype=torch.float32); gamma = 1.0 + rnd(Cc, scale=0.3, seed=5, dtype=torch.float32)
        beta = rnd(Cc, scale=0.3, seed=6, dtype=torch.float32)
        Wp, b, cs = T.ln_fold(W, gamma, beta, BF)
        ref = T.ln_ref(xb, Wp, b).to(dev)
        kw = dict(bias=b, ln_eps=1e-5, ln_csum=cs)
    else:
        xb = rnd(P, Cc, seed=1); Wp = rnd(3 * Cc, Cc, scale=Cc ** -0.5, seed=2)
        ref = xb.float() @ Wp.float().T
        kw = {}
    X = expand(xb, M)
    fq, qk = guarded((M, 2 * Cc), BF, 64)
    fv, Vt = guarded((Bv, Cc, Tt), BF, 1)
    assert nbytes(qk) > G2
    k = run_one(O.Gemm(X, Wp, qk, Vt=Vt, vt_from=2 * Cc, vt_T=Tt, **kw))
    assert k == ("gemm_ws_kernel<vT,ln>" if ln else "gemm_ws_kernel<vT>"), k
    assert guards_intact(fq, 64) and guards_intact(fv, 1)
    close_periodic(qk, ref[:, :2 * Cc], P, name=f"large fused qk ln={ln}")
    close_periodic(Vt, ref[:, 2 * Cc:].reshape(Pv, Tt, Cc).transpose(1, 2).contiguous(), Pv, name=f"large fused V^T ln={ln}")
    bit_periodic(qk, P, "fused qk"); bit_periodic(Vt, Pv, "fused V^T")


@pytest.mark.parametrize("persist", [1, 0])
def test_gemm_xl_a_crosses_4g(dev, persist):
    """Case 4: K = 1280 -> N = 320 with residual, A = 4.30 GB; the persistent 256 x 256 XL kernel and the per-tile one (XL_PERSIST=0)."""
    need(8)
    M, K, N = M_BIG, 1280, 320
    Ab, W, b, Rb, ref = gemm_base(K, N, res=True)
    A = expand(Ab, M); R = expand(Rb, M)
    assert nbytes(A) > G4 and A.numel() > E31
    full, C = guarded((M, N), BF, 64)
    k = run_one(O.Gemm(A, W, C, bias=b, R=R, ws=ws_buf()), XL_BN=256, XL_PERSIST=persist)
    assert k == ("gemm_xlp_kernel<256x256,gemm+res>" if persist else "gemm_xl_kernel<256x256,gemm>"), k
    assert guards_intact(full, 64)
    close_periodic(C, ref, P_ROWS, name=f"large xl gemm 1280->320 persist={persist}")
    bit_periodic(C, P_ROWS, "xl gemm")


@pytest.mark.parametrize("xd", [0, 1])
def test_gemm_xl_xd_c_crosses_4g(dev, xd):
    """Case 5: K = 640 -> N = 1280 (A 2.15 GB, C 4.30 GB) on the XL kernel and through the W-direct kernel (option XD with Wq), which stores C and
    reads R through bounded descriptors."""
    need(11)
    M, K, N = M_BIG, 640, 1280
    Ab, W, b, Rb, ref = gemm_base(K, N, res=bool(xd))
    A = expand(Ab, M)
    R = expand(Rb, M) if xd else None
    assert nbytes(A) > G2
    full, C = guarded((M, N), BF, 64)
    assert nbytes(C) > G4 and C.numel() > E31
    k = run_one(O.Gemm(A, W, C, bias=b, R=R, ws=ws_buf(), Wq=PK.pack_wq(W)), XD=xd)
    assert k.startswith("gemm_xd_kernel" if xd else "gemm_xlp_kernel<256x256,gemm"), k
    assert guards_intact(full, 64)
    close_periodic(C, ref, P_ROWS, name=f"large gemm 640->1280 xd={xd}")
    bit_periodic(C, P_ROWS, "xl / xd gemm")


def test_gemm_generic_c_crosses_4g(dev):
    """Case 6: the shape of case 1 forced onto the generic gemm_conv_kernel."""
    need(8)
    M, K, N = M_BIG, 320, 1280
    Ab, W, b, _, ref = gemm_base(K, N)
    A = expand(Ab, M)
    full, C = guarded((M, N), BF, 64)
    assert nbytes(C) > G4 and C.numel() > E31
    k = run_one(O.Gemm(A, W, C, bias=b, ws=ws_buf()), GEMM_XL=0, GEMM_WS=0)
    assert k.startswith("gemm_conv_kernel<128,128,64"), k
    assert guards_intact(full, 64)
    close_periodic(C, ref, P_ROWS, name="large generic gemm 320->1280")
    bit_periodic(C, P_ROWS, "generic gemm")


def test_gemm_f32_c_crosses_4g(dev):
    """Case 7: fp32 C (c_is_f32), M = 840,011, N = 1280, K = 320: C = 4.30 GB (the generic kernel is the only main loop with an fp32 store)."""
    need(8)
    M, K, N = 840_011, 320, 1280
    Ab, W, b, Rb, ref = gemm_base(K, N, res=True, res_dtype=torch.float32)
    A = expand(Ab, M)
    full, C = guarded((M, N), torch.float32, 64)
    assert nbytes(C) > G4
    C.copy_(expand(Rb, M))                                   # residual aliased to C: a second 4.3 GB fp32 tensor would not add a case
    k = run_one(O.Gemm(A, W, C, bias=b, R=C, ws=ws_buf()))
    assert k.startswith("gemm_conv_kernel<128,128,64"), k
    assert guards_intact(full, 64)
    close_periodic(C, ref, P_ROWS, name="large fp32-C gemm 320->1280")
    bit_periodic(C, P_ROWS, "fp32-C gemm")


def test_gemm_k320_a_past_the_weight_stationary_window(dev):
    """Case 8: K = 320, M = 3,355,500, N = 64: A = 2.15 GB does not fit the ONE 2 GiB descriptor window of gemm_ws.hip (its tile offsets are
    relative to A, not to the tile).  include/mdx.h serves the shape: the dispatcher must give it to a main loop that rebases per tile
    (launch_gemm_ws used to be chosen and to refuse it with MDX_EINVAL)."""
    need(6)
    M, K, N = 3_355_500, 320, 64
    Ab, W, b, _, ref = gemm_base(K, N)
    A = expand(Ab, M)
    assert nbytes(A) > G2
    full, C = guarded((M, N), BF, 64)
    k = run_one(O.Gemm(A, W, C, bias=b, ws=ws_buf()))
    assert k.startswith(("gemm_xl_kernel<256x", "gemm_xlp_kernel<256x")), k
    assert guards_intact(full, 64)
    close_periodic(C, ref, P_ROWS, name="large gemm 320->64, A past the ws window")
    bit_periodic(C, P_ROWS, "k320 gemm past the ws window")
    # a few rows fewer fit the window: the weight-stationary kernel keeps the shape, with the same result
    M2 = 0x7FFF0000 // (2 * K) - 1
    full2, C2 = guarded((M2, N), BF, 64)
    k2 = run_one(O.Gemm(A[:M2], W, C2, bias=b, ws=ws_buf()))
    assert k2 == "gemm_ws_kernel<plain>", k2
    assert guards_intact(full2, 64)
    close_periodic(C2, ref, P_ROWS, name="large gemm 320->64, A just inside the ws window")


# ---------------------------------------------------------------------------------------------------------------------------
# convolution
def conv_base(P, H, W_, Cin, Cout, xdtype=BF):
    x = rnd(P, H, W_, Cin, seed=1, dtype=xdtype)
    w = rnd(Cout, Cin, 3, 3, scale=(Cin * 9) ** -0.5, seed=2, dtype=torch.float32); b = rnd(Cout, seed=3, dtype=torch.float32)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.to(BF).float(), b, padding=1).permute(0, 2, 3, 1).contiguous()
    return x, w, b, ref


@pytest.mark.parametrize("route", ["xl", "generic"])
def test_conv3x3_x_crosses_4g(dev, route):
    """Case 9: 3x3 conv, 28 x 50, Cin = 960 -> Cout = 320, 1598 images (period 5): X = 4.30 GB; XL conv route and the generic kernel."""
    need(8)
    B, H, W_, Cin, Cout, P = 1598, 28, 50, 960, 320, 5
    xb, w, b, ref = conv_base(P, H, W_, Cin, Cout)
    x = expand(xb, B)
    assert nbytes(x) > G4 and x.numel() > E31
    full, y = guarded((B, H, W_, Cout), BF, 1)
    k = run_one(O.Conv(x, PK.pack_conv_weight(w.cpu(), BF).to(dev), y, bias=b, pad=(1, 1), ws=ws_buf()), **({} if route == "xl" else {"GEMM_XL": 0}))
    assert (k.startswith("gemm_xl_kernel<256x") and k.endswith(",conv>")) if route == "xl" else k.startswith("gemm_conv_kernel<128,128,64"), k
    assert guards_intact(full, 1)
    close_periodic(y, ref, P, name=f"large conv3x3 960->320 {route}")
    bit_periodic(y, P, "conv3x3")


@pytest.mark.parametrize("B,lo,hi,Cin,Cout", [(1200, (28, 50), (56, 100), 64, 320), (4800, (7, 13), (14, 25), 64, 1280)], ids=["exact2x", "W-cropped"])
def test_conv_upsample2x_y_crosses_4g(dev, B, lo, hi, Cin, Cout):
    """Cases 10 / 11: the upsampled-2x conv with Y = 4.30 GB, exact 2x and with a cropped axis (X stays far below the documented 2^31 bytes)."""
    need(8)
    P = 3
    xb = rnd(P, *lo, Cin, seed=1)
    w = rnd(Cout, Cin, 3, 3, scale=(Cin * 9) ** -0.5, seed=2, dtype=torch.float32); b = rnd(Cout, seed=3, dtype=torch.float32)
    ref = F.conv2d(F.interpolate(xb.float().permute(0, 3, 1, 2), size=hi, mode="nearest"), w.to(BF).float(), b, padding=1).permute(0, 2, 3, 1).contiguous()
    x = expand(xb, B)
    wf = PK.fold_upsample_conv(w.cpu(), hi[0] != 2 * lo[0], hi[1] != 2 * lo[1], BF).to(dev)
    full, y = guarded((B, *hi, Cout), BF, 1)
    assert nbytes(y) > G4 and y.numel() > E31 and nbytes(x) < G2
    k = run_one(O.Conv(x, wf, y, bias=b, ws=ws_buf(), upsample2x=True))
    assert k.startswith("gemm_xl_kernel<256x") and k.endswith(",conv,up2x>"), k
    assert guards_intact(full, 1)
    close_periodic(y, ref, P, name=f"large upsample2x {lo}->{hi} {Cin}->{Cout}")
    bit_periodic(y, P, "upsample2x conv")


@pytest.mark.parametrize("case,B,H,W_,Cin,Cout,opts,expect", [
    ("conv_out_ws", 4795, 28, 50, 320, 4, {}, "conv_direct_kpar_ws_kernel"),                       # case 12
    ("vae_conv_out", 188, 224, 400, 128, 3, {}, "conv_direct_kpar_ws_kernel"),                     # case 13: Cout < 4 on the weight-stationary kernel
    ("conv_out_kpar", 4795, 28, 50, 320, 4, {"CONV_OUT_WS": 0}, "conv_direct_kpar_kernel"),        # case 14
])
def test_conv_direct_x_crosses_4g(dev, case, B, H, W_, Cin, Cout, opts, expect):
    """Cases 12-14: mdx_conv2d_direct with a 4.3 GB 16-bit X and fp32 Y on the K-parallel kernels."""
    need(6)
    P = 3
    xb, w, b, ref = conv_base(P, H, W_, Cin, Cout)
    x = expand(xb, B)
    assert nbytes(x) > G4 and x.numel() > E31
    full, y = guarded((B, H, W_, Cout), torch.float32, 1)
    k = run_one(O.Conv(x, PK.pack_conv_weight(w.cpu(), BF).to(dev), y, bias=b, pad=(1, 1), direct=True), **opts)
    assert k == expect, k
    assert guards_intact(full, 1)
    close_periodic(y, ref, P, name=f"large direct conv {case}")
    bit_periodic(y, P, case)


def test_conv_direct_conv_in_y_crosses_4g(dev):
    """Case 15: conv_direct_simple_kernel as conv_in: fp32 X with 4 channels, 16-bit Y with 320 channels, 4795 images: Y = 4.30 GB."""
    need(6)
    B, H, W_, Cin, Cout, P = 4795, 28, 50, 4, 320, 3
    xb, w, b, ref = conv_base(P, H, W_, Cin, Cout, xdtype=torch.float32)
    x = expand(xb, B)
    full, y = guarded((B, H, W_, Cout), BF, 1)
    assert nbytes(y) > G4 and y.numel() > E31
    k = run_one(O.Conv(x, PK.pack_conv_weight(w.cpu(), BF).to(dev), y, bias=b, pad=(1, 1), direct=True))
    assert k == "conv_direct_simple_kernel", k
    assert guards_intact(full, 1)
    close_periodic(y, ref, P, name="large direct conv_in")
    bit_periodic(y, P, "conv_in")


# ---------------------------------------------------------------------------------------------------------------------------
# attention: head dim 40, 8 heads, T = 1400, Q and K the two halves of one [B, 1400, 640] buffer (4.30 GB), period 3 batch items
AB, AH, AT, AD, AP = 2397, 8, 1400, 40, 3


def attn_inputs(pre, Tk=AT, shared_qk=True):
    import test_kernels_gpu as T
    Cc = AH * AD
    qb = rnd(AP, AT, Cc, seed=1); kb = rnd(AP, Tk, Cc, seed=2); vb = rnd(AP, Tk, Cc, seed=3)
    qb, qref = T.prescale_q(qb, AD, pre)
    vtb = torch.full((AP, Cc, PK.round_up(Tk, 8)), NAN, dtype=BF, device="cuda")     # garbage in the kv pad must not leak
    vtb[:, :, :Tk] = vb.transpose(1, 2)
    vt = expand(vtb, AB)
    if shared_qk:
        qk = expand(torch.cat([qb, kb], dim=2), AB)
        assert nbytes(qk) > G4 and qk.numel() > E31 and nbytes(vt) > G2
        q, k = qk[:, :, :Cc], qk[:, :, Cc:]
    else:
        q, k = expand(qb, AB), expand(kb, AB)
    return q, k, vt, qref.float(), kb.float(), vb.float()


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("old", [False, True], ids=["attention2", "attention"])
def test_attention_self_qk_crosses_4g(dev, pre, old):
    """Cases 16 / 18: self-attention on attn2_kernel (plain and pre-scaled Q) and on attention.hip (ATTN2=0)."""
    import test_kernels_gpu as T
    need(10)
    q, k, vt, qr, kr, vr = attn_inputs(pre)
    ref = T.ref_attention(qr, kr, vr, AH, AD ** -0.5)
    full, o = guarded((AB, AT, AH * AD), BF, 1)
    assert nbytes(o) > G2
    with L.options(**({"ATTN2": 0} if old else {})):
        expect = T.attn2_route(AD, AT, pre=pre)
        kern = run_one(O.Attn(q, k, vt, o, heads=AH, Tk=AT, scale=AD ** -0.5, q_prescaled=pre))
    assert kern.startswith(expect) and kern.startswith("attn_kernel<" if old else "attn2_kernel<40,self"), (kern, expect)
    assert guards_intact(full, 1)
    close_periodic(o, ref, AP, name=f"large self-attention pre={pre} {kern}")


@pytest.mark.parametrize("pre", [False, True])
def test_attention_crossview_qk_crosses_4g(dev, pre):
    """Case 17: the two-source cross-view form; the kvmap sends query batch i to key batches B - 1 - i (low to the highest and back) and
    (i + 1200) % B — both keep the period: B = 3 x 799 and 1200 = 3 x 400."""
    import test_kernels_gpu as T
    need(10)
    q, k, vt, qr, kr, vr = attn_inputs(pre)
    i = torch.arange(AB)
    kvmap = torch.stack([AB - 1 - i, (i + 1200) % AB], 1).reshape(-1).to(torch.int32).to(dev)
    ref = torch.stack([sum(T.ref_attention(qr[r:r + 1], kr[j:j + 1], vr[j:j + 1], AH, AD ** -0.5)[0] for j in ((2 - r) % 3, r)) for r in range(AP)])
    full, o = guarded((AB, AT, AH * AD), BF, 1)
    assert nbytes(o) > G2
    expect = T.attn2_route(AD, AT, xview=True, pre=pre)
    kern = run_one(O.Attn(q, k, vt, o, heads=AH, Tk=AT, scale=AD ** -0.5, kvmap=kvmap, nsrc=2, q_prescaled=pre))
    assert kern.startswith(expect) and kern.startswith("attn2_kernel<40,xview"), (kern, expect)
    assert guards_intact(full, 1)
    close_periodic(o, ref, AP, name=f"large cross-view attention pre={pre} {kern}")


def test_attention_resident_short_kv_o_crosses_2g(dev):
    """Case 19: the resident short-kv route (Tk = 78 text context) at the same B: O = 2.15 GB."""
    import test_kernels_gpu as T
    need(6)
    Tk = 78
    q, k, vt, qr, kr, vr = attn_inputs(True, Tk=Tk, shared_qk=False)
    ref = T.ref_attention(qr, kr, vr, AH, AD ** -0.5)
    full, o = guarded((AB, AT, AH * AD), BF, 1)
    assert nbytes(o) > G2 and nbytes(q) > G2
    kern = run_one(O.Attn(q, k, vt, o, heads=AH, Tk=Tk, scale=AD ** -0.5, q_prescaled=True))
    assert kern == "attn2_kernel<40,resident,q32,fold>", kern
    assert guards_intact(full, 1)
    close_periodic(o, ref, AP, name="large resident short-kv attention")


# ---------------------------------------------------------------------------------------------------------------------------
# normalisation and row ops
def gn_case(B, HW, Cc, P, silu, eps):
    xb = (rnd(P, HW, Cc, seed=1).float() * 2 + 0.7).to(BF)
    gam = rnd(Cc, seed=2, dtype=torch.float32); bet = rnd(Cc, seed=3, dtype=torch.float32)
    ref = F.group_norm(xb.float().transpose(1, 2), 32, gam, bet, eps)
    if silu: ref = F.silu(ref)
    x = expand(xb, B)
    assert nbytes(x) > G4 and x.numel() > E31
    return x, gam, bet, ref.transpose(1, 2).contiguous()


@pytest.mark.parametrize("two_stage", [False, True], ids=["one-launch", "two-stage"])
def test_groupnorm_crosses_4g(dev, two_stage):
    """Case 20: GroupNorm + SiLU on [1598, 1400, 960], 32 groups, period 3 images: the one-launch kernel (no workspace) and the two streaming passes."""
    need(10)
    B, HW, Cc, P = 1598, 1400, 960, 3
    x, gam, bet, ref = gn_case(B, HW, Cc, P, True, 1e-5)
    full, y = guarded((B, HW, Cc), BF, 1)
    k = run_one(O.GroupNorm(x, y, gam, bet, groups=32, eps=1e-5, silu=True, ws=ws_buf(4) if two_stage else None))
    assert k == ("gn_stats_kernel+gn_apply_kernel" if two_stage else "groupnorm_kernel"), k
    assert guards_intact(full, 1)
    close_periodic(y, ref, P, name=f"large groupnorm 1598x1400x960 {k}")


def test_groupnorm_many_chunks_finalize_crosses_4g(dev):
    """Case 21: GroupNorm on [188, 89600, 128]: hundreds of chunks per image, partials combined by gn_finalize_kernel."""
    need(10)
    B, HW, Cc, P = 188, 89600, 128, 3
    x, gam, bet, ref = gn_case(B, HW, Cc, P, True, 1e-6)
    full, y = guarded((B, HW, Cc), BF, 1)
    k = run_one(O.GroupNorm(x, y, gam, bet, groups=32, eps=1e-6, silu=True, ws=ws_buf(4)))
    assert k == "gn_stats_kernel+gn_apply_kernel", k
    assert guards_intact(full, 1)
    close_periodic(y, ref, P, name="large groupnorm 188x89600x128 finalize")


def test_layernorm_crosses_4g(dev):
    """Case 22: LayerNorm on [1,680,017, 1280]."""
    need(10)
    M, Cc = M_BIG, 1280
    xb = (rnd(P_ROWS, Cc, seed=1).float() * 3 - 0.5).to(BF)
    gam = rnd(Cc, seed=2, dtype=torch.float32); bet = rnd(Cc, seed=3, dtype=torch.float32)
    ref = F.layer_norm(xb.float(), (Cc,), gam, bet)
    x = expand(xb, M)
    full, y = guarded((M, Cc), BF, 64)
    assert nbytes(x) > G4 and nbytes(y) > G4 and y.numel() > E31
    k = run_one(O.LayerNorm(x, y, gam, bet))
    assert k == "layernorm_kernel", k
    assert guards_intact(full, 64)
    close_periodic(y, ref, P_ROWS, name="large layernorm")
    bit_periodic(y, P_ROWS, "layernorm")


def test_gemm_layernorm_scratch_and_rowstat_c_crosses_4g(dev):
    """Case 23: fused-LayerNorm descriptor with the weight-stationary kernel off (GEMM_WS=0): rows normalised into ln_scratch, a
    non-weight-stationary GEMM, then rowstat_kernel over the finished C [1,680,017, 1280]."""
    import test_kernels_gpu as T
    need(9)
    M, K, N = M_BIG, 320, 1280
    xb = (rnd(P_ROWS, K, scale=1.5, seed=1).float() + 0.7).to(BF)
    W = rnd(N, K, scale=K ** -0.5, seed=2, dtype=torch.float32); gamma = 1.0 + rnd(K, scale=0.3, seed=5, dtype=torch.float32)
    beta = rnd(K, scale=0.3, seed=6, dtype=torch.float32)
    Wp, b, cs = T.ln_fold(W, gamma, beta, BF)
    ref = T.ln_ref(xb, Wp, b, stored=True).to(dev)
    x = expand(xb, M)
    full, C = guarded((M, N), BF, 64)
    assert nbytes(C) > G4 and C.numel() > E31
    scratch = torch.full((M, K), NAN, dtype=BF, device=dev)
    fs, st = guarded((M, 2), torch.float32, 64)
    k = run_one(O.Gemm(x, Wp, C, bias=b, ln_eps=1e-5, ln_csum=cs, ln_scratch=scratch, rowstat=st.view(1, M, 2), ws=ws_buf()), GEMM_WS=0)
    assert k == "rowstat_kernel", k
    assert guards_intact(full, 64) and guards_intact(fs, 64) and not torch.isnan(scratch).any()
    close_periodic(C, ref, P_ROWS, name="large ln(scratch)+gemm 320->1280")
    bit_periodic(C, P_ROWS, "ln(scratch)+gemm"); bit_periodic(st, P_ROWS, "row statistics")
    # (sum, sum of squares) of the STORED rows, fp64: the first period, and the last rows of the tensor
    for lo, hi in ((0, P_ROWS), (M - P_ROWS, M)):
        cf = C[lo:hi].double()
        want = torch.stack([cf.sum(1), (cf ** 2).sum(1)], -1)
        err = ((st[lo:hi].double() - want).abs() / (want.abs() + 1.0)).max().item()
        assert err < 2e-5, (lo, err)


def test_softmax_rows_x_crosses_4g(dev):
    """Case 24: mdx_softmax_rows on fp32 X [767,011, 1400] = 4.30 GB, bf16 Y."""
    need(8)
    rows, T_ = 767_011, 1400
    xb = rnd(P_ROWS, T_, scale=3.0, seed=1, dtype=torch.float32)
    ref = torch.softmax(xb * 0.37, dim=-1)
    x = expand(xb, rows)
    assert nbytes(x) > G4
    full, y = guarded((rows, T_), BF, 64)
    assert nbytes(y) > G2
    k = run_one(O.Softmax(x, y, T_, scale=0.37))
    assert k == "softmax_rows_kernel", k
    assert guards_intact(full, 64)
    close_periodic(y, ref, P_ROWS, name="large softmax rows")
    bit_periodic(y, P_ROWS, "softmax rows")


# ---------------------------------------------------------------------------------------------------------------------------
# element-wise
@pytest.mark.parametrize("Cc,expect", [(1280, "ew_vec8_kernel"), (100, "ew_scalar_kernel")])
def test_elementwise_add_copy_cross_2g_elements(dev, Cc, expect):
    """Cases 25 / 26: ADD and COPY over just more than 2^31 16-bit elements on the 16-byte kernel (C = 1280) and on the scalar kernel (C = 100,
    with the destination a column slice of a wider buffer)."""
    need(10)
    M = E31 // Cc + 37
    pad = 0 if Cc % 8 == 0 else 2
    xb = rnd(P_ROWS, Cc, seed=1); yb = rnd(P_ROWS, Cc, seed=2)
    x = expand(xb, M)
    full = torch.full((M + 128, Cc + 2 * pad), NAN, dtype=BF, device=dev)
    y = full[64:64 + M, pad:pad + Cc]
    assert x.numel() > E31 and y.numel() > E31 and nbytes(x) > G4
    for kind, ref in ((L.EW_COPY, xb.float()), (L.EW_ADD, xb.float() + yb.float())):
        if kind == L.EW_ADD:
            for lo in range(0, M, 1 << 20):                     # Y += X over a periodic Y (filled in pieces: no third 4.3 GB tensor)
                hi = min(M, lo + (1 << 20))
                y[lo:hi] = yb.index_select(0, torch.arange(lo, hi, device=dev) % P_ROWS)
        k = run_one(O.Ew(kind, x, y))
        assert k == expect, k
        assert guards_intact(full, 64) and (pad == 0 or (bool(torch.isnan(full[:, :pad]).all()) and bool(torch.isnan(full[:, pad + Cc:]).all()))), "wrote outside the Y view"
        close_periodic(y, ref, P_ROWS, name=f"large ew kind={kind} C={Cc}")
        bit_periodic(y, P_ROWS, f"ew kind={kind}")
        if kind == L.EW_COPY:
            assert torch.equal(y[M - P_ROWS:], x[M - P_ROWS:]) and torch.equal(y[:P_ROWS], xb)


def test_elementwise_upsample_y_crosses_4g(dev):
    """Case 27: MDX_EW_UPSAMPLE on the 16-byte kernel, 14x25 -> 28x50 x 640 channels, 2397 images: Y = 4.30 GB."""
    need(7)
    B, Cc, P = 2397, 640, 3
    ub = rnd(P, 14, 25, Cc, seed=6)
    ref = F.interpolate(ub.float().permute(0, 3, 1, 2), size=(28, 50), mode="nearest").permute(0, 2, 3, 1).contiguous()
    u = expand(ub, B)
    full, up = guarded((B, 28, 50, Cc), BF, 1)
    assert nbytes(up) > G4 and up.numel() > E31
    k = run_one(O.Upsample(u, up, PK.nearest_index(14, 28).to(dev), PK.nearest_index(25, 50).to(dev)))
    assert k == "ew_upsample_vec8_kernel", k
    assert guards_intact(full, 1)
    close_periodic(up, ref, P, name="large ew upsample")
    bit_periodic(up, P, "ew upsample")
    assert torch.equal(up[B - P:].float(), ref.index_select(0, torch.arange(B - P, B, device=dev) % P))


def test_layout_nchw_nhwc_crosses_2_30_elements(dev):
    """Case 28: NCHW -> NHWC and back in fp32 at just over 2^30 elements (4.30 GB each)."""
    need(10)
    B, Cc, H, W_, P = 2397, 320, 28, 50, 3
    nb = rnd(P, Cc, H, W_, seed=7, dtype=torch.float32)
    n = expand(nb, B)
    assert n.numel() > 2 ** 30 and nbytes(n) > G4
    fh, h = guarded((B, H, W_, Cc), torch.float32, 1)
    k = run_one(O.Layout(n, h, True))
    assert k == "ew_scalar_kernel", k
    assert guards_intact(fh, 1)
    close_periodic(h, nb.permute(0, 2, 3, 1).contiguous(), P, name="large nchw->nhwc")
    bit_periodic(h, P, "nchw->nhwc")
    assert torch.equal(h[:P], nb.permute(0, 2, 3, 1)) and torch.equal(h[B - P:], n[B - P:].permute(0, 2, 3, 1))
    del n
    torch.cuda.empty_cache()
    fb, back = guarded((B, Cc, H, W_), torch.float32, 1)
    k = run_one(O.Layout(h, back, False))
    assert k == "ew_scalar_kernel", k
    assert guards_intact(fb, 1)
    close_periodic(back, nb, P, name="large nhwc->nchw")
    bit_periodic(back, P, "nhwc->nchw")
    assert torch.equal(back[:P], nb) and torch.equal(back[B - P:], nb.index_select(0, torch.arange(B - P, B, device=dev) % P))
