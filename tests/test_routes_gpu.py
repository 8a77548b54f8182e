"""-m gpu: parity of every GEMM / conv MAIN LOOP at the shapes the bench batch (64 scenes/GPU = 384 views) routes to it.

Round-1 review: `gemm_pp` and `conv3x3` (and now `gemm_xl`) are selected by shape inside the library, and no test shape met their
conditions, so 20 % of the timed step ran on kernels no GPU test executed.  Every case here ASSERTS the route through
`mdx_last_kernel()` (the library reports which main loop a descriptor went to) and compares against a plain PyTorch fp32
reference of the same op on bf16-rounded inputs (computed on the GPU with torch: the shapes are too big for a CPU reference in
seconds).  Tolerance: xformers' bf16 table scaled by the output magnitude (tests/test_kernels_gpu.py: close()).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from magicdrive_amd import _lib as L
from magicdrive_amd import ops as O
from magicdrive_amd import packing as PK

BF = torch.bfloat16


def rnd(*shape, scale=1.0, seed=0, dtype=BF, dev="cuda"):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)


from helpers import close  # noqa: E402  (xformers table, every element; measured values logged)


def ws_buf(mb=64):
    return torch.empty(mb * 1024 * 1024 // 4, dtype=torch.float32, device="cuda")


def run_one(op):
    O.run_ops([op])
    k = (L.lib().mdx_last_kernel() or b"").decode()
    torch.cuda.synchronize()
    return k


# ---------------------------------------------------------------------------------------------------------------------------
# gemm_xl.hip — GEMM
@pytest.mark.parametrize("M,N,K,bias,res,inplace,epi,expect", [
    (41037, 1280, 1280, True, True, False, 0, "gemm_xl_kernel<256x"),              # ragged M, residual
    (41000, 640, 640, True, False, False, 2, "gemm_conv_kernel<128,128,64"),        # SiLU epilogue: declined by XL (xl_supported), generic tile
    (82000, 320, 1280, True, True, True, 0, "gemm_xl_kernel<256x"),        # ff.out at level 0: in-place residual (R == C)
    (82000, 160, 640, True, False, False, 0, "gemm_xl_kernel<256x"),       # one 160-wide N tile
    (41000, 644, 640, False, False, False, 0, "gemm_xl_kernel<256x"),               # N % 8 != 0: narrow stores, ragged last N tile
    (45000, 1920, 640, True, False, False, 0, "gemm_xl_kernel<256x"),               # fused q|k|v width at level 1
    (40960, 256, 64, True, False, False, 0, "gemm_xl_kernel<256x"),        # a single K slab (prologue == whole loop)
    (40960, 512, 128, False, True, False, 0, "gemm_xl_kernel<256x"),       # two slabs
    (40960, 512, 192, True, True, False, 0, "gemm_xl_kernel<256x"),        # three slabs (odd count: both ring buffers end mid-cycle)
])
@pytest.mark.parametrize("persist", [1, 0])
def test_xl_gemm(dev, M, N, K, bias, res, inplace, epi, expect, persist):
    """persist: XL_PERSIST — the persistent 256 x 256 kernel (gemm_xlp_kernel) takes the plain-epilogue shapes with >= 512 tiles and
    16-byte C rows; with the option off every shape runs gemm_xl_kernel."""
    with L.options(XL_PERSIST=persist):
        _xl_gemm(dev, M, N, K, bias, res, inplace, epi, expect, persist)


def _xl_gemm(dev, M, N, K, bias, res, inplace, epi, expect, persist):
    A = rnd(M, K, seed=1); W = rnd(N, K, scale=K ** -0.5, seed=2)
    b = rnd(N, seed=3, dtype=torch.float32) if bias else None
    Cbig = torch.full((M, N + 24), float("nan"), dtype=BF, device=dev)
    C = Cbig[:, 8:8 + N] if (N % 8 == 0) else Cbig[:, 4:4 + N]          # strided view; 16-byte aligned only when N % 8 == 0
    R = R0 = None
    if res:
        R0 = rnd(M, N, seed=4)
        if inplace:
            C.copy_(R0); R = C
        else:
            R = R0
    k = run_one(O.Gemm(A, W, C, bias=b, R=R, epilogue=epi, ws=ws_buf()))
    if expect.startswith("gemm_xl_kernel") and persist:
        # the persistent kernel must take exactly the shapes it is built for (256-wide choice, wide rows, >= 512 tiles)
        tiles256 = ((M + 255) // 256) * ((N + 255) // 256)
        if k.startswith("gemm_xlp_kernel"):
            assert N % 8 == 0 and tiles256 >= 512 and k == f"gemm_xlp_kernel<256x256,gemm{'+res' if res else ''}>", k
        else:
            assert k.startswith(expect) and k.endswith(",gemm>"), f"routed to {k!r}, expected {expect!r}"
    else:
        assert k.startswith(expect) and k.endswith(",gemm>"), f"routed to {k!r}, expected {expect!r}"
    ref = A.float() @ W.float().T
    if bias: ref += b
    if epi == 2: ref = F.silu(ref)
    if res: ref += R0.float()
    close(C, ref, name=f"xl gemm {M}x{N}x{K}")
    lo = 8 if N % 8 == 0 else 4
    assert torch.isnan(Cbig[:, :lo].float()).all() and torch.isnan(Cbig[:, lo + N:].float()).all(), "wrote outside the C view"


@pytest.mark.parametrize("persist", [1, 0])
def test_xl_gemm_geglu(dev, persist):
    """Packed GEGLU at the bench shape of level 1 (N = 8C = 5120, K = 640): value / gate tiles meet in one lane."""
    with L.options(XL_PERSIST=persist):
        _xl_gemm_geglu(dev, persist)


def _xl_gemm_geglu(dev, persist):
    M, F_, K = 40960 + 100, 2560, 640
    A = rnd(M, K, seed=1); W = rnd(2 * F_, K, scale=K ** -0.5, seed=2, dtype=torch.float32); b = rnd(2 * F_, seed=3, dtype=torch.float32)
    Wp, bp = PK.pack_geglu(W.cpu(), b.cpu(), BF)
    C = torch.zeros(M, F_, dtype=BF, device=dev)
    k = run_one(O.Gemm(A, Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU, ws=ws_buf()))
    assert k == ("gemm_xlp_kernel<256x256,geglu>" if persist else "gemm_xl_kernel<256x256,gemm>"), k
    h, g = (A.float() @ W.to(BF).float().T + b).chunk(2, dim=-1)
    close(C, h * F.gelu(g), name="xl geglu")


def test_xl_gemm_temb_rows(dev):
    """The per-(step, image) addend rows: tiles of 256 rows over images of 91 rows (3-4 images per tile), row picked by a device selector."""
    T, nb, N, K = 91, 480, 1280, 640
    M = T * nb
    A = rnd(M, K, seed=1); W = rnd(N, K, scale=K ** -0.5, seed=2)
    temb = rnd(3, nb, N, seed=7, dtype=torch.float32)
    sel = torch.tensor([2], dtype=torch.int32, device=dev)
    C = torch.zeros(M, N, dtype=BF, device=dev)
    k = run_one(O.Gemm(A, W, C, temb=temb, sel=sel, temb_sel_stride=nb * N, temb_b_stride=N, rows_per_b=T, ws=ws_buf()))
    assert k.startswith("gemm_xl_kernel<256x"), k
    ref = A.float() @ W.float().T + temb[2].repeat_interleave(T, 0)
    close(C, ref, name="xl gemm temb rows")


# ---------------------------------------------------------------------------------------------------------------------------
# gemm_xl.hip — 3x3 convolution (implicit GEMM: per-lane tap masks -> zero-filling LDS-DMA)
def conv_ref(x, w, b, stride, pad, tb, R, epi=0):
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.to(BF).float(), b, stride=stride, padding=pad)
    if tb is not None: ref = ref + tb[:, :, None, None]
    if epi == 2: ref = F.silu(ref)
    ref = ref.permute(0, 2, 3, 1)
    if R is not None: ref = ref + R.float()
    return ref


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,res,temb,expect", [
    (48, 28, 50, 320, 320, (1, 1), True, True, "gemm_xl_kernel<256x"),      # level 0 resnet conv; tiles straddle image rows
    (120, 14, 25, 640, 640, (1, 1), True, False, "gemm_xl_kernel<256x"),             # 350-px images: every tile crosses an image
    (480, 7, 13, 1280, 1280, (1, 1), True, True, "gemm_xl_kernel<256x"),             # 91-px images: 3-4 images (temb rows) per tile
    (1470, 4, 7, 1280, 1280, (1, 1), False, True, "gemm_xl_kernel<256x"),            # 28-px images: 10-11 images per tile (the bench's mid block)
    (240, 28, 50, 320, 320, (2, 2), False, False, "gemm_xl_kernel<256x"),   # Downsample2D: stride 2, 28x50 -> 14x25
    (420, 9, 11, 64, 256, (1, 1), False, False, "gemm_xl_kernel<256x"),     # one channel block; odd sizes
    (130, 14, 25, 1920, 640, (1, 1), False, True, "gemm_xl_kernel<256x"),            # up-block concat width, ragged M tile
])
def test_xl_conv(dev, B, H, W, Cin, Cout, stride, res, temb, expect):
    x = rnd(B, H, W, Cin, seed=1)
    w = rnd(Cout, Cin, 3, 3, scale=(Cin * 9) ** -0.5, seed=2, dtype=torch.float32)
    b = rnd(Cout, seed=3, dtype=torch.float32)
    Ho = (H + 2 - 3) // stride[0] + 1; Wo = (W + 2 - 3) // stride[1] + 1
    y = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=BF, device=dev)
    R = rnd(B, Ho, Wo, Cout, seed=4) if res else None
    tb = rnd(B, Cout, seed=5, dtype=torch.float32) if temb else None
    ref = conv_ref(x, w, b, stride, (1, 1), tb, R)
    k = run_one(O.Conv(x, PK.pack_conv_weight(w.cpu(), BF).to(dev), y, bias=b, R=R, temb=tb, temb_b_stride=Cout if temb else 0,
                       stride=stride, pad=(1, 1), ws=ws_buf()))
    assert k.startswith(expect) and k.endswith(",conv>"), f"routed to {k!r}, expected {expect!r}"
    close(y, ref, name=f"xl conv {B}x{H}x{W} {Cin}->{Cout} {k}")


def test_xl320_edge_tile_reads_no_residual_past_its_buffer(dev):
    """tests/xl320_edge_case.py in a child process (a GPU memory fault aborts the process that raised it): the 320-wide tile's second
    128-row half may start past M; its residual prefetch has to stay inside R even when R closes its allocation."""
    import os, subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "xl320_edge_case.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok conv_err" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-1200:])


def geglu_case(M, F_, K, expect=None):
    dev = torch.device("cuda")
    A = rnd(M, K, seed=1); W = rnd(2 * F_, K, scale=K ** -0.5, seed=2, dtype=torch.float32); b = rnd(2 * F_, seed=3, dtype=torch.float32)
    Wp, bp = PK.pack_geglu(W.cpu(), b.cpu(), BF)
    C = torch.zeros(M, F_, dtype=BF, device=dev)
    k = run_one(O.Gemm(A, Wp.to(dev), C, bias=bp.to(dev), epilogue=L.EPI_GEGLU, ws=ws_buf()))
    h, g = (A.float() @ W.to(BF).float().T + b).chunk(2, dim=-1)
    close(C, h * F.gelu(g), name=f"geglu {M}x{F_}x{K} ({k})")
    assert expect is None or k.startswith(expect), (k, expect)
    return k


def test_k320_geglu_large_route(dev):
    """The level-0 GEGLU shape class (K = 320, >= 1024 tiles of 256 x 256): the weight-stationary kernel by default; the XL tile with
    XL_GEGLU320=1 runs in test_forced_routes[geglu320xl]."""
    assert geglu_case(26400, 1280, 320) == "gemm_ws_kernel<geglu>"


# ---------------------------------------------------------------------------------------------------------------------------
# Batch-flattened GEMM (GCParams.col_split): the per-view V^T projections of levels 1 / 2 / mid as ONE XL launch whose epilogue
# scatters token columns to their view.  Even tokens-per-view (4-byte pair stores), odd (element stores, pairs straddling views),
# a ragged last tile; the kv pad columns of the destination must stay untouched.
@pytest.mark.parametrize("Bt,T,Cc", [(60, 350, 640), (240, 91, 1280), (384, 28, 1280), (64, 351, 640)])
def test_flattened_batched_vt(dev, Bt, T, Cc):
    ldv = PK.round_up(T, 8)
    X = rnd(Bt, T, Cc, seed=1); Wv = rnd(Cc, Cc, scale=Cc ** -0.5, seed=2)
    Vt = torch.full((Bt, Cc, ldv), 7.0, dtype=BF, device=dev)
    k = run_one(O.Gemm(Wv, X, Vt[:, :, :T]))
    assert k.startswith("gemm_xl_kernel<256x") and k.endswith(",gemm>"), k
    ref = torch.einsum("ck,btk->bct", Wv.float(), X.float())
    close(Vt[:, :, :T], ref, name=f"flattened V^T {Bt}x{T}x{Cc} ({k})")
    if ldv > T:
        assert (Vt[:, :, T:].float() == 7.0).all(), "kv pad columns were written"


# ---------------------------------------------------------------------------------------------------------------------------
# Forced routes, in-process: the routing switches are library options (csrc/options.h, mdx_set_option): every XL tile width on small
# ragged shapes (GEMM_XL=2: whenever supported), the other main loops (generic tile, gemm_ws) with the XL kernel switched
# off at the shapes the round-1 review listed, and the attention kernels' other instantiations.
def gemm_case(M, N, K, bias=True, res=False, epi=0, expect=None):
    dev = torch.device("cuda")
    A = rnd(M, K, seed=1); W = rnd(N, K, scale=K ** -0.5, seed=2)
    b = rnd(N, seed=3, dtype=torch.float32) if bias else None
    R = rnd(M, N, seed=4) if res else None
    C = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    k = run_one(O.Gemm(A, W, C, bias=b, R=R, epilogue=epi, ws=ws_buf()))
    ref = A.float() @ W.float().T
    if bias: ref += b
    if epi == 2: ref = F.silu(ref)
    if res: ref += R.float()
    close(C, ref, name=f"gemm {M}x{N}x{K} ({k})")
    assert expect is None or k.startswith(expect), (k, expect)      # (str.startswith takes a tuple of alternatives)
    return k


def conv_case(B, H, W, Cin, Cout, stride=(1, 1), res=True, temb=True, expect=None):
    dev = torch.device("cuda")
    x = rnd(B, H, W, Cin, seed=1)
    w = rnd(Cout, Cin, 3, 3, scale=(Cin * 9) ** -0.5, seed=2, dtype=torch.float32); b = rnd(Cout, seed=3, dtype=torch.float32)
    Ho = (H - 1) // stride[0] + 1; Wo = (W - 1) // stride[1] + 1
    y = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=BF, device=dev)
    R = rnd(B, Ho, Wo, Cout, seed=4) if res else None
    tb = rnd(B, Cout, seed=5, dtype=torch.float32) if temb else None
    k = run_one(O.Conv(x, PK.pack_conv_weight(w.cpu(), BF).to(dev), y, bias=b, R=R, temb=tb, temb_b_stride=Cout if temb else 0, stride=stride, pad=(1, 1), ws=ws_buf()))
    close(y, conv_ref(x, w, b, stride, (1, 1), tb, R), name=f"conv {B}x{H}x{W} {Cin}->{Cout} ({k})")
    assert expect is None or k.startswith(expect), (k, expect)
    return k


@pytest.mark.parametrize("bn", [320, 256, 160])
@pytest.mark.parametrize("raster", [0, 1, 2])
def test_forced_xl_widths(dev, bn, raster):
    with L.options(GEMM_XL=2, XL_BN=bn, XL_RASTER=raster):
        g, c = f"gemm_xl_kernel<256x{bn},gemm>", f"gemm_xl_kernel<256x{bn},conv>"
        gemm_case(2000, 640, 640, res=True, expect=g)                 # ragged M (7.8 tiles), N = 2-4 tiles (too few tiles for the persistent walk)
        gemm_case(777, 324, 128, bias=False, expect=g)                # N % 8 != 0: narrow stores; ragged everything; two slabs
        gemm_case(5000, 320, 64, expect=g)                            # one slab
        gemm_case(5000, 320, 64, epi=2, expect="gemm_conv_kernel<")   # SiLU epilogues stay off the XL kernel even when it is forced
        gemm_case(3000, 1280, 960, res=True, expect=g)                # 15 slabs (K < 1024: no automatic split-K)
        gemm_case(30000, 1600, 128, res=True, expect=(g, "gemm_xlp_kernel<256x256") if bn == 256 else g)   # 118 M-tiles x 5-10 N-tiles: several XCD panels, ragged last N-group
        conv_case(6, 28, 50, 320, 320, expect=c)                      # level-0 resnet conv
        conv_case(12, 14, 25, 128, 640, res=False, expect=c)          # 350-px images, 2 channel blocks
        conv_case(40, 7, 13, 64, 320, temb=True, expect=c)            # 91-px images: temb slots
        conv_case(100, 4, 7, 128, 160, expect=c)                      # 28-px images: 10 images per tile
        conv_case(6, 28, 50, 64, 320, stride=(2, 2), res=False, temb=False, expect=c)
        if bn == 256:
            geglu_case(3000, 640, 320, expect=g)


def test_forced_no_xl(dev):
    """The main loops that serve small batches (XL declines below XL_MIN_TILES tiles), forced at larger shapes."""
    with L.options(GEMM_XL=0):
        gemm_case(8736, 1280, 1280, res=True, expect="gemm_conv_kernel<128,128,64")
        geglu_case(8736, 5120, 1280, expect="gemm_conv_kernel<128,128,64")
        gemm_case(4500, 2560, 1280, res=True, expect="gemm_conv_kernel<128,128,64")          # ragged M
        conv_case(96, 7, 13, 1280, 1280, expect="gemm_conv_kernel<128,128,64")               # 8736 rows, tiles span 3-4 images
        conv_case(24, 14, 25, 1920, 1280, res=False, expect="gemm_conv_kernel<128,128,64")
        conv_case(16, 28, 50, 320, 320, expect="gemm_conv_kernel<128,128,64")
        conv_case(600, 4, 7, 320, 320, expect="gemm_conv_kernel<128,128,64")                  # 4x7 images
        conv_case(22, 28, 28, 640, 640, expect="gemm_conv_kernel<128,128,64")                 # 28-px rows straddling 128-row tiles
        gemm_case(537600, 320, 320, res=True, expect="gemm_ws_kernel<plain>")                 # bench row count
        geglu_case(26400, 1280, 320, expect="gemm_ws_kernel<geglu>")                          # K = 320 GEGLU on the weight-stationary kernel
        # small grids (round 6: GEMM_SMALL_TILES): 64 x 64 tiles for plain GEMMs / small convs, 128 x 128 for larger convs below 2048 rows, and the
        # rounds 1-5 rule (128 rows from M = 2048, else 64 x 128) with the option off
        gemm_case(2100, 640, 640, res=True, expect="gemm_conv_kernel<64,64,64")
        conv_case(6, 28, 50, 320, 320, expect="gemm_conv_kernel<64,64,64")
        conv_case(6, 7, 13, 2560, 1280, expect="gemm_conv_kernel<128,128,64")                 # 128 x 128 tiles (+ automatic split-K)
        with L.options(GEMM_SMALL_TILES=0):
            gemm_case(2100, 640, 640, res=True, expect="gemm_conv_kernel<128,128,64")
            gemm_case(546, 1280, 1280, res=True, expect="gemm_conv_kernel<64,128,64")
            conv_case(6, 7, 13, 2560, 1280, expect="gemm_conv_kernel<64,128,64")


def test_forced_geglu320_on_xl(dev):
    with L.options(XL_GEGLU320=1):
        assert geglu_case(26400, 1280, 320) in ("gemm_xl_kernel<256x256,gemm>", "gemm_xlp_kernel<256x256,geglu>")


@pytest.mark.parametrize("mode,opts", [("attn_q32", {"ATTN2_QT": 1}), ("attn_q64", {"ATTN2_QT": 2}), ("attn_d80", {"ATTN2_D80": 1}), ("attn_d80_off", {"ATTN2_D80": 0}),
                                       ("attn_old", {"ATTN2": 0}), ("attn_nofold", {"ATTN2_FOLD": 0}), ("attn_bh_order", {"ATTN2_VIEWMAP": 0, "ATTN_SWZ": 1}),
                                       ("attn_nopf", {"ATTN2_PF": 0}), ("attn_nopf_q64", {"ATTN2_PF": 0, "ATTN2_QT": 2})])
def test_forced_attention_routes(dev, mode, opts):
    """attention2.hip's other instantiations (32- / 64-query waves; head dim 80 on / off; the per-(view, head) block order of rounds 2-3)
    and attention.hip at the same shapes, through the tests of tests/test_kernels_gpu.py (their route assertions follow the current
    switches)."""
    import test_kernels_gpu as T
    with L.options(**opts):
        for pre in (False, True):
            for case in T.ATTN2_CASES:
                T.test_attention2(dev, *case, pre)
            T.test_attention2_softmax_rescale_branch(dev, pre)
            for case in [(1, 8, 1400, 40), (3, 8, 350, 80), (2, 8, 700, 40)]:
                T.test_attention2_crossview(dev, *case, pre)


@pytest.mark.parametrize("M,N,K,res", [
    (268800, 640, 640, True),        # C x C + residual at level 1, the bench row count: 1050 x 3 tiles, the last N-tile half empty
    (268800, 1280, 640, False),      # q|k projection at level 1
    (69888, 1280, 1280, True),       # level 2
    (131072 + 77, 768, 192, True),   # ragged M (the last tile of some walks is an edge tile: conservative wait), 3 slabs, 3 N-tiles
    (140000, 512, 64, False),        # ONE slab per tile: the ring is refilled for the next tile while this one is stored
    (140000, 512, 128, True),        # two slabs
])
def test_persistent_xl_gemm_bench_shapes(dev, M, N, K, res):
    """gemm_xlp_kernel at the bench batch's shapes and at the corners of its tile walk (K of one / two / three slabs, ragged last
    M-tile, half-empty last N-tile, in-place residual), vs torch; and bit-identical to the non-persistent kernel (same reduction order,
    same epilogue arithmetic)."""
    A = rnd(M, K, seed=1); W = rnd(N, K, scale=K ** -0.5, seed=2); b = rnd(N, seed=3, dtype=torch.float32)
    R = rnd(M, N, seed=4) if res else None
    outs = {}
    for persist in (1, 0):
        C = torch.full((M, N), float("nan"), dtype=BF, device=dev)
        with L.options(XL_PERSIST=persist):
            k = run_one(O.Gemm(A, W, C, bias=b, R=R, ws=ws_buf()))
        assert k.startswith("gemm_xlp_kernel<256x256" if persist else "gemm_xl_kernel<256x256"), (persist, k)
        outs[persist] = C
    ref = A.float() @ W.float().T + b
    if res: ref += R.float()
    close(outs[1], ref, name=f"persistent xl gemm {M}x{N}x{K}")
    assert torch.equal(outs[1], outs[0]), "persistent and per-tile kernels must agree bit for bit"


# ---------------------------------------------------------------------------------------------------------------------------
# gemm_xd.hip — the W-direct persistent GEMM (option XD, off by default; MdxGemmDesc.Wq)
@pytest.mark.parametrize("M,N,K,epi,res,bias,ldx", [
    (130000, 1280, 640, 0, False, True, 0),          # qk at level 1 (ten units per tile: every unit of a tile drains the previous one)
    (201600 - 37, 640, 640, 0, True, True, 64),      # to_out + residual: ragged M, 2.5 N-tiles (column tail dropped by the descriptor), C a column slice of a wider buffer
    (70000, 5120, 640, 1, False, True, 0),           # GEGLU at level 1
    (52416, 1280, 1280, 0, True, False, 0),          # level 2 + residual, no bias (zero-record bias descriptor)
    (130000, 1296, 768, 0, False, True, 0),          # twelve units: one generic pair behind the ten drain units, 16-column tail tile
    (52416, 1280, 5120, 0, True, True, 0),           # ff.out at level 2: 80 units
])
def test_xd_gemm_matches_persistent_xl_bit_for_bit(dev, M, N, K, epi, res, bias, ldx):
    """Same descriptor with XD = 1 (gemm_xd_kernel) and XD = 0 (gemm_xlp_kernel): identical arithmetic per element, so the outputs must be
    EQUAL (incl. the untouched columns of a wider C buffer), and both are within the bf16 tolerance of the fp32 reference.  The XD launch is
    repeated: its register loads are hand-counted asynchronous operations, and the one bug this kernel had (register copies of in-flight
    loads at the tile loop's back-edge, see tests/test_xd_isa.py) showed in one launch out of ten."""
    A = rnd(M, K, scale=0.5, seed=1); W = rnd(N, K, scale=0.05, seed=2)
    bv = torch.randn(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    if epi == 1:
        W, bv = PK.pack_geglu(W.float(), bv, BF)
    No = N // 2 if epi == 1 else N
    Cbuf = torch.zeros(M, No + ldx, dtype=BF, device="cuda")
    R = rnd(M, No, seed=4) if res else None
    Wq = PK.pack_wq(W)
    op = O.Gemm(A, W, Cbuf[:, :No], bias=bv if bias else None, R=R, epilogue=epi, ws=ws_buf(), Wq=Wq)
    outs = {}
    for xd in (0, 1):
        with L.options(XD=xd):
            Cbuf.fill_(7.0)
            k = run_one(op)
            assert k.startswith("gemm_xd_kernel" if xd else "gemm_xlp_kernel"), k
            outs[xd] = Cbuf.clone()
    assert torch.equal(outs[1], outs[0]), f"{(outs[1] != outs[0]).sum().item()} elements differ"
    with L.options(XD=1):
        for it in range(12):
            Cbuf.fill_(7.0)
            run_one(op)
            assert torch.equal(Cbuf, outs[0]), f"launch {it}: {(Cbuf != outs[0]).sum().item()} elements differ"
    idx = torch.randint(0, M, (1024,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    idx[:8] = torch.arange(M - 8, M, device="cuda")
    ref = A[idx].float() @ W.float().t()
    if bias:
        ref = ref + bv[None, :]
    if epi == 1:
        r4 = ref.reshape(-1, N // 64, 2, 32)
        ref = (r4[:, :, 0] * F.gelu(r4[:, :, 1])).reshape(-1, No)
    ref = ref.to(BF).float()
    if res:
        ref = ref + R[idx].float()
    close(outs[1][idx, :No], ref, name=f"xd_gemm_{M}x{N}x{K}")
    if ldx:
        assert bool((outs[1][:, No:] == 7.0).all())


def test_xd_fp16_build(dev):
    """The fp16 build of the W-direct kernel (v_mfma_f32_16x16x32_f16) against its own LDS-both persistent kernel."""
    H = torch.float16
    M, N, K = 70000, 1280, 640
    A = rnd(M, K, scale=0.5, seed=1, dtype=H); W = rnd(N, K, scale=0.05, seed=2, dtype=H)
    R = rnd(M, N, seed=4, dtype=H)
    C = torch.zeros(M, N, dtype=H, device="cuda")
    op = O.Gemm(A, W, C, R=R, ws=ws_buf(), Wq=PK.pack_wq(W))
    outs = {}
    for xd in (0, 1):
        with L.options(XD=xd):
            C.zero_()
            O.run_ops([op])
            k = (L.lib().mdx_last_kernel() or b"").decode()
            torch.cuda.synchronize()
            assert k.startswith("gemm_xd_kernel" if xd else "gemm_xlp_kernel"), k
            outs[xd] = C.clone()
    assert torch.equal(outs[1], outs[0])


def test_set_option_rejects_unknown_key():
    with pytest.raises(L.MdxError):
        L.set_option("NO_SUCH_SWITCH", 1)


# ---------------------------------------------------------------------------------------------------------------------------
# The route table (tests/golden/gemm_routes.json, recorded by tools/route_table.py from the library before routing moved into csrc/gemm_route.h):
# every threshold of the routing decision, one launch per case, asserted through mdx_last_kernel().
import gemm_route_table as RT  # noqa: E402

ROUTE_CASES = [c for c in RT.load() if c["gpu"]]


@pytest.mark.parametrize("c", ROUTE_CASES, ids=[c["name"] for c in ROUTE_CASES])
def test_route_table(dev, c):
    tag, _ = RT.run_case(c)
    assert tag == c["tag"], (c["name"], tag, c["tag"])
