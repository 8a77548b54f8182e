"""Tile-tail test data: every kernel at "one less / exact / one more" of its own tile, walk and vector constants, at the smallest shapes.

Pure torch on the CPU (no GPU import).  tests/test_tails_cpu.py proves that the cases below hit every residue class they claim, that each
GEMM / conv case resolves (csrc/gemm_route.h, through tests/gemm_route_check.cpp) to the kernel it names, and that the tail-weighted inputs
make every tail error visible to helpers.close(); tests/test_tails_gpu.py feeds the same cases to the HIP kernels.

Why weighted inputs: with N(0, 1) operands a softmax that also counts one zero-filled phantom key past Tk stays at 0.7 tol of close(), a GEMM
that drops its last 8-wide k chunk changes every element by a little.  So the LAST k chunk, row, columns, bias entry, key, element are made
to matter (generators below), and `mutants()` restates the reference with exactly one such tail error: close() must reject all of them.

    edges(c)         the members of {1, c-1, c, c+1, 2c-1, 2c, 2c+1} a family's divisibility rule allows
    cells(family)    the residue classes the family must hit, derived from CONSTANTS
    cases(family)    the concrete shapes: each axis swept fully while the others alternate between two awkward values
    hits(case)       the cells a case covers, worked out from its numbers (not declared by hand)

Where the cases follow the code rather than a first reading of the plan:
  * edges(c, div): under a rule n % div == 0 the literal seven points keep only c and 2c, so they are also taken in units of div.
  * attention2.hip takes Tq >= 256 with ceil(Tq / 128) H B >= 128 only: its query sweep is {255 (claims attention.hip), 256, 257, 300, 511, 512,
    513} at B = H = 8; every Tk in 1..200 runs on the plain and the FOLD + PF form, the option routes (FOLD off, PF off, QT 1 / 2, d = 80) run the
    32- and 64-key edges and three tiles.
  * the XL slot table serves 25 rows per image (256 / 25 + 2 = 12); 23 is the first width it declines, and that case claims the generic tile.
  * GEMM_BM256 is decided before GEMM_BN applies: the 256-row tile needs the width rule itself to say 128, narrower cases claim 64 x 128.
  * the persistent XL forms need 16-byte C rows: N = 496 / 248 (W-direct: 240) instead of 500 (xlp_cases; the list depends on the CU count).
  * a conv whose image is one pixel wide or high under pad 1 never reads its last tap: the k-tail weight and the k8 mutants sit on the last
    tap that does read the image (last_live_tap), so those cases keep their k-tail check.
  * norms: the common offset grows with the row (norm_offset) and the last element is +2 offsets; softmax: offset -12 and last logit +12
    (SOFTMAX_OFFSET / SOFTMAX_SPIKE say why): with the plain +4 / +8 a divisor off by one stays under close() on long rows.
"""
import functools
import math

import torch
import torch.nn.functional as F

import values_data as V

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
FP16 = torch.float16
LOG2E = V.LOG2E

# --------------------------------------------------------------------------------------------------------------------------------------
# the constants the sweeps are derived from, each with the csrc/ line it mirrors
# --------------------------------------------------------------------------------------------------------------------------------------
CONSTANTS = {          # key: (value, "file:line[-line]", text that must stand on the cited lines — tests/test_tails_cpu.py reads it back)
    "gemm_conv.tiles": (((64, 64), (128, 128), (64, 128), (128, 64), (256, 128)), "gemm_conv.hip:439-443", "else rc = MDX_GC(64, 64);"),
    "gemm_conv.BK": ((64, 32), "gemm_conv.hip:438", "BK == 32 ? MDX_GC2"),
    "gemm_conv.wave_rows": (32, "gemm_conv.hip:43", "TM = BM / (WM * 32)"),
    "gemm_conv.kchunk": (64, "gemm_route.h:285", "+ 63) / 64 * 64"),
    "gemm_conv.k_vec": (8, "gemm_conv.hip:42", "KCH = BK / 8"),
    "gemm_ws.BM": (128, "gemm_ws.hip:85", "BM = 128, BN = 128, BK = 64, KS = 20, NSLAB = 5"),
    "gemm_ws.BK": (64, "gemm_ws.hip:85", "BK = 64"),
    "gemm_ws.NSLAB": (5, "gemm_ws.hip:85", "NSLAB = 5"),
    "gemm_ws.ROWS_PASS": ((64, 128), "gemm_ws.hip:88", "ROWS_PASS = GEGLU ? 128 : 64"),
    "gemm_ws.LNS_MAXP": (4, "gemm_ws.hip:220", "LNS_MAXP = 4"),
    "gemm_xl.BM": (256, "gemm_xl.hip:69", "BM = 256, NTH = 512"),
    "gemm_xl.BN": ((160, 256, 320), "gemm_route.h:163", "kXlWidths[3] = {{320, W320, 23.7, 1.896}, {256, W256, 13.4, 1.565}, {160, W160"),
    "gemm_xl.BK": (64, "gemm_route.h:92", "(p.K % 64)"),
    "gemm_xl.XL_SLOTS": (12, "gemm_route.h:26", "XL_SLOTS = 12"),
    "gemm_xl.raster_mt": (64, "gemm_xl.hip:1070-1081", "q.mt >= 64"),
    "attn.KVT": (64, "attention.hip:44", "KVT = 64"),
    "attn.NW": ((1, 2, 4, 8), "attention.hip:353", "launch_attn<D16, 1>(p, tag, st)"),
    "attn.wave_q": (32, "attention.hip:333", "NW * 32"),
    "attn2.A2_KV": (64, "attention2.hip:40", "A2_KV = 64"),
    "attn2.sub": (32, "attention2.hip:523", "A2_KV <= 32"),
    "attn2.min_Tq": (256, "attn_route.h:43", "p.Tq < 256"),
    "attn2.q64_Tq": (512, "attn_route.h:72", "p.Tq >= 512"),
    "attn2.res_tiles": (3, "attention2.hip:38", "#define A2_RING 3"),
    "attn_short.SHORT_T": (128, "attention_short.hip:41", "SHORT_T = 128"),
    "attn_short.sub": (32, "attention_short.hip:41", "4 sub-tiles of 32 kv"),
    "gn.vec": ((8, 4, 2, 1), "norm.hip:519-522", "for (int v = 8; v > 1; v >>= 1)"),
    "gn.threads": (1024, "norm.hip:21", "GN_THREADS = 1024"),
    "gn2.U": (4, "norm.hip:184", "GN2_U = 4"),
    "ln.vec": (8, "norm.hip:362", "nv = p.C / 8"),
    "ln.lanes": (64, "norm.hip:374", "lane + 64 * i"),
    "ln.MAXV": (4, "norm.hip:574", "layernorm_kernel<4, 1, AFFINE>"),
    "softmax.lanes": (64, "norm.hip:546", "c += 64"),
    "ew.vec": (8, "elementwise.hip:539", "p.C % 8 == 0"),
    "ew.block": (256, "elementwise.hip:228", "__launch_bounds__(256) void ew_scalar_kernel"),
}


def const(key):
    return CONSTANTS[key][0]


def edges(c, div=1, lo=1):
    """Sorted valid members of {1, c-1, c, c+1, 2c-1, 2c, 2c+1} under the rule n % div == 0, n >= lo.  With div > 1 the literal set keeps
    only c and 2c, so the same seven points are also taken in units of the rule: {div, c-div, c, c+div, 2c-div, 2c, 2c+div}."""
    s = {1, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1}
    if div > 1:
        s |= {div, c - div, c + div, 2 * c - div, 2 * c + div}
    return sorted(n for n in s if n >= lo and n % div == 0)


def roundup(x, m):
    return (x + m - 1) // m * m


# --------------------------------------------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------------------------------------------
def gemm_case(M, N, K, opts, tag, **kw):
    c = dict(kind="gemm", M=M, N=N, K=K, opts=dict(opts), tag=tag, bias=False, R=False, temb=0, epi=0, c_f32=False, batch=1, splitk=0,
             vt=None, ln=None, rowstat=0, wq=False)
    c.update(kw)
    return c


GENERIC_TILES = {                       # route -> (BM, BN, BK, forcing options)
    "t64": (64, 64, 64, dict(GEMM_BM=64, GEMM_BN=64)),
    "t128": (128, 128, 64, dict(GEMM_BM=128, GEMM_BN=128)),
    "t64x128": (64, 128, 64, dict(GEMM_BM=64, GEMM_BN=128)),
    "t128x64": (128, 64, 64, dict(GEMM_BM=128, GEMM_BN=64)),
    "t256": (256, 128, 64, dict(GEMM_BM256=1, GEMM_BN=128)),
    "t64k32": (64, 64, 32, dict(GEMM_BM=64, GEMM_BN=64, GEMM_BK=32)),
    "t128k32": (128, 128, 32, dict(GEMM_BM=128, GEMM_BN=128, GEMM_BK=32)),
}
NARROW_N = (1, 2, 3, 5, 66, 127)
GENERIC_EPI = ("none", "bias", "bias+R", "temb1", "temb7", "temb50", "silu", "geglu64", "geglu128", "geglu192", "c_f32", "batch3")


def generic_tag(BM, BN, BK, conv=False):
    return "gemm_conv_kernel<%d,%d,%d,%d,2,%s>" % (BM, BN, BK, 4 if BM == 256 else 2, "conv" if conv else "gemm")


def _generic_k_points(BK):
    v = const("gemm_conv.k_vec")
    return sorted({v, BK - v, BK, BK + v, 2 * BK - v, 2 * BK, 2 * BK + v, 3 * BK - v, 3 * BK} - {0})


def _generic_cells(route):
    BM, BN, BK, _ = GENERIC_TILES[route]
    ce = [("M", m) for m in sorted(set(edges(const("gemm_conv.wave_rows")) + edges(BM)))]
    ce += [("N4", n) for n in edges(BN, 4)] + [("N8", r) for r in (0, 4)] + [("Nnarrow", n) for n in NARROW_N]
    ce += [("K", kmod, slabs) for kmod in (8, BK - 8, 0) for slabs in (1, 2, 3)]
    ce += [("epi", e) for e in GENERIC_EPI] + [("splitk", "last_slice_8"), ("splitk", "fewer_than_asked")]
    return ce


def _generic_cases(route):
    BM, BN, BK, force = GENERIC_TILES[route]
    opts = dict(GEMM_WS=0, GEMM_XL=0, **force)
    tag = lambda geglu=False: generic_tag(BM, 128 if geglu else BN, BK)      # GEMM_BN = 64 does not apply to GEGLU (gemm_route.h:267)
    Ns, Ks = (68, 136), (72, 136)
    if route == "t256":
        # GEMM_BM256 looks at the tile width BEFORE GEMM_BN is applied (gemm_route.h:265-267): the 256-row tile needs the width rule itself to
        # say 128 (no small-grid rule; N > 192 or N % 128 == 0).  The narrower cases claim the 64 x 128 tile they really get.
        opts["GEMM_SMALL_TILES"] = 0
        Ns = (196, 264)
    out = _generic_cases_(route, BM, BN, BK, opts, tag, Ns, Ks)
    if route == "t256":
        for c in out:
            auto128 = c["epi"] == 1 or not (c["N"] <= 64 or (c["N"] % 128 != 0 and c["N"] <= 192))
            c["tag"] = generic_tag(256 if auto128 else 64, 128, BK)
    return out


def _generic_cases_(route, BM, BN, BK, opts, tag, Ns, Ks):
    out = []
    for i, m in enumerate(sorted(set(edges(32) + edges(BM)))):
        out.append(gemm_case(m, Ns[i % 2], Ks[i % 2], opts, tag(), bias=True))
    for i, n in enumerate(edges(BN, 4)):
        out.append(gemm_case((37, 2 * BM + 5)[i % 2], n, Ks[i % 2], opts, tag(), bias=True, R=(i % 2 == 1)))
    for i, n in enumerate(NARROW_N):
        out.append(gemm_case((37, BM + 5)[i % 2], n, Ks[i % 2], opts, tag()))
    for i, k in enumerate(_generic_k_points(BK)):
        out.append(gemm_case((37, BM + 5)[i % 2], Ns[i % 2], k, opts, tag(), bias=True))
    M, N, K = BM + 36, Ns[0], 136
    out += [gemm_case(M, N, K, opts, tag()), gemm_case(M, N, K, opts, tag(), bias=True), gemm_case(M, N, K, opts, tag(), bias=True, R=True)]
    out += [gemm_case(M, N, K, opts, tag(), bias=True, temb=r) for r in (1, 7, 50)]
    out += [gemm_case(M, N, K, opts, tag(), bias=True, epi=2)]
    out += [gemm_case(M, n, K, opts, tag(True), bias=True, epi=1) for n in (64, 128, 192)]
    out += [gemm_case(M, N, K, opts, tag(), bias=True, R=True, c_f32=True), gemm_case(M, N, K, opts, tag(), bias=True, batch=3)]
    out += [gemm_case(M, N, 136, opts, tag(), bias=True, R=True, splitk=3), gemm_case(M, N, 72, opts, tag(), bias=True, splitk=4)]
    return out


def splitk_plan(K, splitk):
    """(slices, kchunk) as gemm_route.h:285-286 rounds a forced split."""
    kchunk = roundup(-(-K // max(1, splitk)), const("gemm_conv.kchunk"))
    return -(-K // kchunk), kchunk


def _generic_hits(c, route):
    BM, BN, BK, _ = GENERIC_TILES[route]
    h = {("M", c["M"]), ("K", c["K"] % BK, -(-c["K"] // BK))}
    if c["N"] % 4 == 0:
        h |= {("N4", c["N"]), ("N8", c["N"] % 8)}
    else:
        h.add(("Nnarrow", c["N"]))
    if c["splitk"] > 1:
        n, kc = splitk_plan(c["K"], c["splitk"])
        if c["K"] - (n - 1) * kc == 8: h.add(("splitk", "last_slice_8"))
        if n < c["splitk"]: h.add(("splitk", "fewer_than_asked"))
        return h
    e = ("geglu%d" % c["N"] if c["epi"] == 1 else "silu" if c["epi"] == 2 else "c_f32" if c["c_f32"] else "batch3" if c["batch"] == 3 else
         "temb%d" % c["temb"] if c["temb"] else "bias+R" if c["R"] else "bias" if c["bias"] else "none")
    h.add(("epi", e))
    return h


# ---- weight-stationary GEMM ----
_RP, _WBM = const("gemm_ws.ROWS_PASS")[0], const("gemm_ws.BM")
WS_K = const("gemm_ws.NSLAB") * const("gemm_ws.BK")                        # 320
WS_MT = (1, 7, 8, 9, 15, 17, 25)                                           # M tiles over 8 walkers (WS_SLOTS = 8): 0..4 tiles each, seams at 8 / 16 / 24
WS_R = (0, 1, _RP - 1, _RP, _RP + 1, _WBM - 1)                             # rows missing from the last tile: around one 64-row store pass
WS_N = sorted(set(edges(_WBM, 4)) | {WS_K, WS_K + 8})
WS_GEGLU_N = (64, 128, 192, 320)
WS_VT = [(v, t) for v in (1, 3) for t in (8, 56, 64, 72, 120, 136)]
WS_OPTS = dict(GEMM_WS=2, WS_SLOTS=8)


def _ws_cells(route):
    if route == "plain":
        return [("mt", m) for m in WS_MT] + [("r", r) for r in WS_R] + [("N", n) for n in WS_N] + [("default", 1)]
    if route == "geglu":
        return [("N", n) for n in WS_GEGLU_N] + [("r", r) for r in (0, 1, 127)]
    if route == "vt":
        return [("vt", v, t) for v, t in WS_VT]
    if route == "ln":
        return [("ln", "ln")] + [("lns", p) for p in range(1, const("gemm_ws.LNS_MAXP") + 1)] + [("r", r) for r in (1, 65)]
    return [("rowstat", "parts==tiles"), ("rowstat", "parts>tiles"), ("r", 1), ("r", 65)]


def _ws_cases(route):
    out = []
    if route == "plain":
        Ns = (132, 328)
        for i, (mt, r) in enumerate([(mt, r) for mt in WS_MT for r in WS_R]):
            out.append(gemm_case(128 * mt - r, Ns[i % 2], WS_K, WS_OPTS, "gemm_ws_kernel<plain>", bias=True, R=(i % 3 == 0)))
        for i, n in enumerate(WS_N):
            out.append(gemm_case((200, 1100)[i % 2], n, WS_K, WS_OPTS, "gemm_ws_kernel<plain>", bias=True, R=(i % 2 == 0)))
        out.append(gemm_case(8192 + 65, 132, WS_K, {}, "gemm_ws_kernel<plain>", bias=True))           # the default route (GEMM_WS = 1: M >= 8192)
    elif route == "geglu":
        for i, n in enumerate(WS_GEGLU_N):
            for m in (128 * 3 - (0, 1, 127)[i % 3], 128 * 9 - (1, 127, 0)[i % 3]):
                out.append(gemm_case(m, n, WS_K, WS_OPTS, "gemm_ws_kernel<geglu>", bias=True, epi=1))
    elif route == "vt":
        for i, (v, t) in enumerate(WS_VT):
            out.append(gemm_case(v * t, 128 + (40, 136)[i % 2], WS_K, WS_OPTS, "gemm_ws_kernel<vT>", bias=(i % 2 == 0), vt=(v, t)))
    elif route == "ln":
        for i, (ln, tag) in enumerate([(("ln", 0), "gemm_ws_kernel<plain,ln>")] + [(("lns", p), "gemm_ws_kernel<plain,lns>") for p in (1, 2, 3, 4)]):
            for m in (128 * 2 - 1, 128 * 9 - 65):
                out.append(gemm_case(m, (132, 328)[i % 2], WS_K, WS_OPTS, tag, bias=True, R=(i % 2 == 1), ln=ln))
    else:
        for parts in (3, 4):
            for m in (128 * 2 - 1, 128 * 9 - 65):
                out.append(gemm_case(m, 320, WS_K, WS_OPTS, "gemm_ws_kernel<plain,rs>", bias=True, R=(parts == 4), rowstat=parts))
    return out


def _ws_hits(c, route):
    mt = -(-c["M"] // 128)
    h = {("r", 128 * mt - c["M"])}
    if route == "plain":
        h |= {("mt", mt), ("N", c["N"])}
        if not c["opts"]: h.add(("default", 1))
    elif route == "geglu":
        h.add(("N", c["N"]))
    elif route == "vt":
        h = {("vt",) + tuple(c["vt"])}
    elif route == "ln":
        h.add(("ln", "ln") if c["ln"][0] == "ln" else ("lns", c["ln"][1]))
    else:
        nt = -(-c["N"] // 128)
        h.add(("rowstat", "parts==tiles" if c["rowstat"] == nt else "parts>tiles"))
    return h


# ---- XL GEMM ----
XL_K = tuple(n * const("gemm_xl.BK") for n in (1, 2, 3))
XL_TEMB = (25, 26, 28, 91, 300)            # 25 is still served: 256 / 25 + 2 = 12 slots; the first width the slot table declines is 23
XL_TEMB_DECLINED = max(r for r in range(1, 256) if 256 // r + 2 > const("gemm_xl.XL_SLOTS"))       # 23


def xl_tag(bn):
    return "gemm_xl_kernel<256x%d,gemm>" % bn


def _xl_opts(bn, **kw):
    return dict(GEMM_XL=2, XL_BN=bn, XL_PERSIST=0, **kw)


def _xl_cells(bn):
    ce = [("M", m) for m in edges(256)] + [("N", n) for n in edges(bn, 4)] + [("K", k) for k in XL_K]
    ce += [("temb", r) for r in XL_TEMB] + [("temb_declined", XL_TEMB_DECLINED), ("epi", "R"), ("epi", "bias")] + [("raster", r) for r in (0, 1, 2)]
    if bn == 256:
        ce += [("epi", "geglu")]
    return ce


def _xl_cases(bn):
    out = []
    Ns = (bn - 4, bn + 8)
    for i, m in enumerate(edges(256)):
        out.append(gemm_case(m, Ns[i % 2], XL_K[i % 3], _xl_opts(bn), xl_tag(bn), bias=True, R=(i % 2 == 0)))
    for i, n in enumerate(edges(bn, 4)):
        out.append(gemm_case((255, 513)[i % 2], n, XL_K[i % 3], _xl_opts(bn), xl_tag(bn), bias=(i % 2 == 0), R=(i % 2 == 1)))
    for r in XL_TEMB:
        out.append(gemm_case(2 * r + 257, Ns[1], 128, _xl_opts(bn), xl_tag(bn), bias=True, temb=r))
    # a tile may span more temb rows than the slot table holds: the XL kernel declines, the generic 64 x 64 tile runs
    out.append(gemm_case(2 * XL_TEMB_DECLINED + 257, Ns[1], 128, _xl_opts(bn), generic_tag(64, 64, 64), bias=True, temb=XL_TEMB_DECLINED))
    if bn == 256:
        out += [gemm_case(m, n, 128, _xl_opts(bn), xl_tag(bn), bias=True, epi=1) for m, n in ((255, 256), (513, 576))]
    # the XCD tile orders start at 64 M-tiles; raster 2 with forced panels that divide neither 131 M-tiles nor 3 N-tiles
    for r in (0, 1, 2):
        out.append(gemm_case(131 * 256 - 5, 2 * bn + 12, 64, _xl_opts(bn, XL_RASTER=r, XL_GM=2, XL_GN=2), xl_tag(bn), bias=True))
    return out


def _xl_hits(c, bn):
    if c["opts"].get("XL_RASTER") is not None:
        mt, nt = -(-c["M"] // 256), -(-c["N"] // bn)
        assert mt >= 2 * const("gemm_xl.raster_mt") and mt % 2 and nt % 2, "the forced 2 x 2 panels must not divide the tile grid"
        return {("raster", c["opts"]["XL_RASTER"])}
    if c["temb"]:
        return {("temb_declined", c["temb"])} if not c["tag"].startswith("gemm_xl") else {("temb", c["temb"])}
    h = {("M", c["M"]), ("N", c["N"]), ("K", c["K"])}
    if c["epi"] == 1: h = {("epi", "geglu")}
    if c["R"]: h.add(("epi", "R"))
    if c["bias"]: h.add(("epi", "bias"))
    return h


def xlp_cases(form, cus):
    """The persistent forms of the 256 x 256 XL GEMM walk the tiles with one workgroup per CU from 2 x CUs tiles on (gemm_xl.hip:1092):
    tile counts {2 CUs, 2 CUs + 1, 3 CUs - 1, 3 CUs + 1} in row-major tile order (XL_RASTER = 0: the count is the number of real tiles), a
    ragged last M tile, the first case with two N tiles; form "xlp": K = 128, "xd" (W-direct, Wq given, XD = 1): K = 640, N % 16 == 0.
    The forms need 16-byte C rows (N % 8 == 0), so N = 496 stands for the plan's 500.  Not in FAMILIES (the list depends on the device);
    the inputs are those of every other GEMM case."""
    out = []
    for i, nblk in enumerate((2 * cus, 2 * cus + 1, 3 * cus - 1, 3 * cus + 1)):
        nt = 2 if i == 0 else 1
        tag = ("gemm_xd_kernel<256x256,gemm" if form == "xd" else "gemm_xlp_kernel<256x256,gemm") + ("+res>" if i % 2 else ">")
        out.append(gemm_case(256 * (nblk // nt) - 37, 496 if nt == 2 else (240 if form == "xd" else 248), 640 if form == "xd" else 128,
                             dict(GEMM_XL=2, XL_BN=256, XL_RASTER=0, XD=int(form == "xd")), tag, bias=True, R=bool(i % 2), wq=form == "xd", nblk=nblk))
    return out


# ---- implicit-GEMM conv ----
def last_live_tap(c):
    """(ky, kx) of the last filter tap that reads a pixel of the image for at least one output pixel: (k-1, k-1) unless the image is one
    pixel high / wide under pad 1, where the taps past it only ever see zero padding.  The k-tail weight and the k8 mutants sit there."""
    def last(n_in, n_out, pad):
        return max(t for t in range(c["k"]) if any(0 <= o * c["stride"] - pad + t < n_in for o in range(n_out)))
    return last(c["Hi"], c["Ho"], c["pad"][0]), last(c["Wi"], c["Wo"], c["pad"][1])


def conv_case(B, Hi, Wi, Cin, Cout, k, stride, pad, opts, tag, pad_end=None, **kw):
    ph, pw = pad
    phe, pwe = pad_end if pad_end is not None else pad
    Ho, Wo = (Hi + ph + phe - k) // stride + 1, (Wi + pw + pwe - k) // stride + 1
    assert Ho >= 1 and Wo >= 1
    c = dict(kind="conv", B=B, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=tuple(pad), pad_end=(phe, pwe), Ho=Ho, Wo=Wo,
             M=B * Ho * Wo, N=Cout, K=k * k * Cin, opts=dict(opts), tag=tag, bias=True, R=False, temb=0, epi=0, splitk=0)
    c.update(kw)
    return c


CONV_CIN = (8, 16, 24, 40, 64, 72, 128)
CONV_COUT = (4, 8, 12, 64, 68)
CONV_HOWO = (1, 35, 63, 64, 65)
CONV_XL_WO = (1, 3, 7, 13, 50, 257)
CONV_TILES = {                          # route -> (BM, BN, BK, forcing options, the two awkward Cout values, the Cout sweep)
    "generic": (64, 64, 64, dict(GEMM_BM=64, GEMM_BN=64), (12, 68), CONV_COUT),
    "t128": (128, 128, 64, dict(GEMM_BM=128, GEMM_BN=128), (12, 68), CONV_COUT),
    "t64k32": (64, 64, 32, dict(GEMM_BM=64, GEMM_BN=64, GEMM_BK=32), (12, 68), CONV_COUT),
    # the 256-row tile needs the width rule itself to say 128 (N > 192 or N % 128 == 0) before GEMM_BN applies, and no small-grid rule
    "t256": (256, 128, 64, dict(GEMM_BM256=1, GEMM_BN=128, GEMM_SMALL_TILES=0), (196, 264), (196, 200, 204, 256, 264)),
}
_CONV_GEO = {                                   # Ho * Wo -> (Hi, Wi, k, stride, pad, pad_end)
    1: (3, 3, 3, 1, (0, 0), None), 35: (5, 7, 3, 1, (1, 1), None), 63: (9, 7, 1, 1, (0, 0), None),
    64: (16, 15, 3, 2, (1, 1), None), 65: (10, 27, 3, 2, (0, 0), (1, 1)),
}


def _conv_cells(route):
    if route == "xl":
        return [("Wo", w) for w in CONV_XL_WO] + [("Cin", c) for c in (64, 128)]
    ce = [("k", k) for k in (1, 3)] + [("stride", s) for s in (1, 2)] + [("pad", p) for p in ((0, 0), (1, 1), (2, 1))] + [("pad_end", "asym")]
    ce += [("HoWo", n) for n in CONV_HOWO] + [("Cin", c) for c in CONV_CIN] + [("Cout", c) for c in CONV_TILES[route][5]]
    ce += [("order", o) for o in ("cimajor", "tapmajor")] + [("splitk", 2), ("splitk", 3), ("temb", 3)]
    return ce


def _conv_cases(route):
    out = []
    if route == "xl":
        opts = dict(GEMM_XL=2, XL_BN=256)
        for i, wo in enumerate(CONV_XL_WO):
            Hi = {1: 5, 3: 9, 7: 5, 13: 2, 50: 5, 257: 1}[wo]                  # a temb case needs Ho * Wo >= 26 (XL_SLOTS)
            out.append(conv_case(3, Hi, wo, (64, 128)[i % 2], (68, 264)[i % 2], 3, 1, (1, 1), opts,
                                 "gemm_xl_kernel<256x256,conv>", R=(i % 2 == 0), temb=(3 if i % 2 else 0)))
        return out
    BM, BN, BK, force, (ca, cb), couts = CONV_TILES[route]
    CONV_OPTS = dict(GEMM_XL=0, **force)
    tag = generic_tag(BM, BN, BK, conv=True)
    for i, n in enumerate(CONV_HOWO):
        Hi, Wi, k, s, pad, pe = _CONV_GEO[n]
        out.append(conv_case(3, Hi, Wi, (24, 72)[i % 2], (ca, cb)[i % 2], k, s, pad, CONV_OPTS, tag, pad_end=pe, temb=3, R=(i % 2 == 0)))
    for i, cin in enumerate(CONV_CIN):
        out.append(conv_case(3, 5, 7, cin, (ca, cb)[i % 2], 3, 1, (1, 1), CONV_OPTS, tag, temb=(3 if i % 2 else 0)))
        out.append(conv_case(3, 9, 7, cin, (cb, ca)[i % 2], 1, 1, (0, 0), CONV_OPTS, tag))
    for i, co in enumerate(couts):
        out.append(conv_case(3, 5, 7, (24, 64)[i % 2], co, 3, (1, 2)[i % 2], (1, 1), CONV_OPTS, tag, R=(i % 2 == 1)))
    out.append(conv_case(3, 9, 8, 40, ca, 3, 2, (2, 1), CONV_OPTS, tag))
    out.append(conv_case(3, 9, 8, 64, cb, 3, 1, (2, 1), CONV_OPTS, tag, temb=3))
    for sk in (2, 3):
        out.append(conv_case(3, 5, 7, 24, ca, 3, 1, (1, 1), CONV_OPTS, tag, splitk=sk, temb=3, R=True))
    return out


def _conv_hits(c, route):
    if route == "xl":
        return {("Wo", c["Wo"]), ("Cin", c["Cin"])}
    h = {("k", c["k"]), ("stride", c["stride"]), ("pad", c["pad"]), ("HoWo", c["Ho"] * c["Wo"]), ("Cin", c["Cin"]), ("Cout", c["Cout"])}
    if c["pad_end"] != c["pad"]: h.add(("pad_end", "asym"))
    if c["k"] > 1: h.add(("order", "cimajor" if c["Cin"] % 64 == 0 else "tapmajor"))
    if c["splitk"]: h.add(("splitk", c["splitk"]))
    if c["temb"]: h.add(("temb", c["B"]))
    return h


# ---- attention ----
def attn_case(B, H, Tq, Tk, d, opts, tag, **kw):
    c = dict(kind="attn", B=B, H=H, Tq=Tq, Tk=Tk, d=d, opts=dict(opts), tag=tag, ldv_extra=0, pre=False, causal=False, rowmajor=False,
             nsrc=1, joint=False, kvmap=None, Bkv=B)
    c.update(kw)
    return c


_WQ = const("attn.wave_q")                   # a workgroup of NW waves owns NW x 32 queries: 64 (2 waves), 128 (4), 256 (8); 16 = one MFMA row block
ATTN_TQ = sorted(set(edges(_WQ // 2) + edges(const("attn.KVT")) + edges(4 * _WQ)) | {8 * _WQ - 1, 8 * _WQ + 1})
ATTN_D = (8, 16, 40, 72, 96, 120, 160)
ATTN_JOINT = (1, 2, 3, 6, 8)
ATTN_TK = tuple(range(1, 201))
ATTN_ADD_MAPS = {"both": [[1, 2], [2, 0], [0, 1]], "absent": [[1, -1], [-1, 0], [-1, -1]]}


def _attn_cells(nw):
    ce = [("Tq", t) for t in ATTN_TQ] + [("Tk", t) for t in ATTN_TK] + [("ldv", e) for e in (0, 8)] + [("d", d) for d in ATTN_D]
    return ce + [("add", k) for k in ATTN_ADD_MAPS] + [("joint", n) for n in ATTN_JOINT]


def _attn_cases(nw):
    opts = dict(ATTN2=0, ATTN_NW=nw)
    tag = lambda d, mode="self": "attn_kernel<%d,%d,%s>" % ((d + 15) // 16, nw, mode)
    out = []
    for i, tq in enumerate(ATTN_TQ):
        d = (16, 40)[i % 2]
        out.append(attn_case(1, 2, tq, (77, 129)[i % 2], d, opts, tag(d), ldv_extra=8 * (i % 2)))
    for tk in ATTN_TK:
        out.append(attn_case(1, 2, (17, 33)[tk % 2], tk, 16, opts, tag(16), ldv_extra=8 * (tk % 3 == 0)))
    for i, d in enumerate(ATTN_D):
        out.append(attn_case(1, 2, 33, (77, 129)[i % 2], d, opts, tag(d), ldv_extra=8 * (i % 2)))
    for i, (name, m) in enumerate(ATTN_ADD_MAPS.items()):
        out.append(attn_case(3, 2, 33, (77, 129)[i % 2], 16, opts, tag(16, "xview"), nsrc=2, kvmap=m))
    for i, n in enumerate(ATTN_JOINT):
        m = [[(b + s) % 8 for s in range(n)] for b in range(2)]
        out.append(attn_case(2, 2, 33, (77, 129)[i % 2], 16, opts, tag(16, "joint" if n > 1 else "self"), nsrc=n, joint=True, kvmap=m, Bkv=8))
    return out


def _attn_hits(c, nw):
    if c["joint"]: return {("joint", c["nsrc"])}
    if c["nsrc"] == 2:
        return {("add", "absent" if any(j < 0 for r in c["kvmap"] for j in r) else "both")}
    return {("Tq", c["Tq"]), ("Tk", c["Tk"]), ("ldv", c["ldv_extra"]), ("d", c["d"])}


# attention2.hip: head dim 40 (80), Tq >= 256 and ceil(Tq / 128) H B >= 128: B = 8, H = 8.  Shorter query sequences never reach it; the
# one below the threshold (255) is listed and claims the attention.hip kernel it really gets.
ATTN2_TQ = (255, 256, 257, 300, 511, 512, 513)
ATTN2_SRC_TK = sorted(set(edges(const("attn2.sub")) + edges(const("attn2.A2_KV"))))
ATTN2_FULL_TK = ("plain", "fold_pf")          # every Tk in 1..200; the option routes run the sub-tile / tile edges and three tiles
ATTN2_ROUTES = {        # route -> (d, pre, options, tag below 512 queries, tag from 512 queries)
    "plain": (40, False, {}, "q32", "q64"),
    "fold_pf": (40, True, {}, "q32,fold,pf", "q32,fold,pf"),
    "fold": (40, True, dict(ATTN2_PF=0), "q32,fold", "q32,fold"),
    "nofold": (40, True, dict(ATTN2_FOLD=0), "q32", "q64"),
    "qt1": (40, False, dict(ATTN2_QT=1), "q32", "q32"),
    "qt2_fold": (40, True, dict(ATTN2_QT=2), "q32,fold,pf", "q64,fold"),
    "d80": (80, False, dict(ATTN2_D80=1), "q32", "q32"),
}


def _attn2_tag(route, Tq, mode="self"):
    d, pre, o, lo, hi = ATTN2_ROUTES[route]
    return "attn2_kernel<%d,%s,%s>" % (d, mode, hi if Tq >= const("attn2.q64_Tq") else lo)


def _attn2_cells(route):
    if route == "resident":
        return [("Tk", t) for t in range(1, 193)] + [("Tk_streams", 193)]
    if route in ("xview", "joint"):
        return [("Tk", t) for t in ATTN2_SRC_TK]
    return [("Tq", t) for t in ATTN2_TQ] + [("Tk", t) for t in (ATTN_TK if route in ATTN2_FULL_TK else ATTN2_SRC_TK + [191, 192, 193])]


def _attn2_cases(route):
    B, H = 8, 8
    out = []
    if route == "resident":
        opts = dict(ATTN2_RES=2)
        for tk in range(1, 194):
            tag = "attn2_kernel<40,resident,q32,fold>" if tk <= const("attn2.A2_KV") * const("attn2.res_tiles") else "attn2_kernel<40,self,q32,fold,pf>"
            out.append(attn_case(B, H, (256, 300)[tk % 2], tk, 40, opts, tag, pre=True, ldv_extra=8 * (tk % 3 == 0)))
        return out
    if route in ("xview", "joint"):
        for i, tk in enumerate(ATTN2_SRC_TK):
            pre = bool(i % 2)
            m = [[(b + 1) % B, (b + 7) % B] for b in range(B)]
            tag = "attn2_kernel<40,%s,%s>" % (route, "q32,fold,pf" if pre else "q32")
            out.append(attn_case(B, H, (256, 300)[i % 2], tk, 40, dict(ATTN2_RES=0), tag, pre=pre, nsrc=2, joint=(route == "joint"), kvmap=m))
        return out
    d, pre, o, lo, hi = ATTN2_ROUTES[route]
    opts = dict(ATTN2_RES=0, **o)
    for i, tq in enumerate(ATTN2_TQ):
        tag = _attn2_tag(route, tq) if tq >= const("attn2.min_Tq") else "attn_kernel<%d,2,self>" % ((d + 15) // 16)
        out.append(attn_case(B, H, tq, (77, 129)[i % 2], d, opts, tag, pre=pre, ldv_extra=8 * (i % 2)))
    for tk in (ATTN_TK if route in ATTN2_FULL_TK else ATTN2_SRC_TK + [191, 192, 193]):
        tq = (256, 300)[tk % 2]
        out.append(attn_case(B, H, tq, tk, d, opts, _attn2_tag(route, tq), pre=pre, ldv_extra=8 * (tk % 3 == 0)))
    return out


def _attn2_hits(c, route):
    if route == "resident" and "resident" not in c["tag"]:
        return {("Tk_streams", c["Tk"])}
    return {("Tq", c["Tq"]), ("Tk", c["Tk"])}


_SS, _ST = const("attn_short.sub"), const("attn_short.SHORT_T")
SHORT_T = (1, _SS - 1, _SS, _SS + 1, 2 * _SS, 77, _ST - 1, _ST)


def _short_cells(d):
    return [("causal", t) for t in range(1, 129)] + [("full", a, b) for a in SHORT_T for b in SHORT_T]


def _short_cases(d):
    out = [attn_case(2, 2, t, t, d, {}, "attn_short_kernel<%d,causal>" % d, causal=True, rowmajor=True) for t in range(1, 129)]
    out += [attn_case(2, 2, a, b, d, {}, "attn_short_kernel<%d,full>" % d, rowmajor=True) for a in SHORT_T for b in SHORT_T]
    return out


def _short_hits(c, d):
    return {("causal", c["Tq"])} if c["causal"] else {("full", c["Tq"], c["Tk"])}


# ---- norms, softmax, element-wise ----
_GT = const("gn.threads")                    # one workgroup of 1024 threads per (image, group), 8-wide vectors: 128 threads' worth of pixels
GN_HW = (1, 2, 3, 31, _GT // 8 - 1, _GT // 8, _GT // 8 + 1, _GT - 1, _GT + 1)
GN_CPG = tuple(sorted(const("gn.vec"))) + (10, 40, 80)      # every vector width, then widths 2 / 8 / 8 again at larger groups
LN_C_ALL = tuple(range(const("ln.vec"), const("ln.vec") * const("ln.lanes") * const("ln.MAXV") + 1, const("ln.vec")))       # 8 .. 2048
LN_M = (1, 3, 4, 63, 65)
_SL = const("softmax.lanes")
SM_T = tuple(range(1, 4 * _SL + 45)) + (16 * _SL - 1, 16 * _SL, 16 * _SL + 1, 64 * _SL + 1)       # 1..300, 1023, 1024, 1025, 4097
_EV, _EB = const("ew.vec"), const("ew.block")
EW_C = tuple(range(1, 2 * _EV + 2)) + (8 * _EV - 1, 8 * _EV, 8 * _EV + 1)
EW_M = (1, _EB - 1, _EB + 1)
EW_OPS = ("ADD", "COPY", "SILU", "SCALE")
LAYOUT_C, LAYOUT_HW = (1, 3, 4, 5, 8, 9), (1, 63, 64, 65)


def _norm_cells(family):
    if family == "groupnorm":
        return [("HW", h) for h in GN_HW] + [("cpg", c) for c in GN_CPG] + [("silu", s) for s in (0, 1)]
    if family == "layernorm":
        return [("C", c) for c in LN_C_ALL] + [("M", m, c) for m in LN_M for c in (8, 320, 2048)] + [("ldx>C", 1)]
    if family == "softmax":
        return [("T", t) for t in SM_T] + [("rows", r) for r in (1, 5)] + [("pad", 1)]
    if family == "elementwise":
        return [("C", c, k) for c in EW_C for k in ("scalar", "vec8") if k == "scalar" or c % 8 == 0] + [("M", m) for m in EW_M] + [("op", o) for o in EW_OPS]
    if family == "layout":
        return [("C", c) for c in LAYOUT_C] + [("HW", n) for n in LAYOUT_HW] + [("upsample", "2Hi-1")]
    raise KeyError(family)


def _norm_cases(family):
    out = []
    if family == "groupnorm":
        for i, hw in enumerate(GN_HW):
            cpg = (10, 8)[i % 2]
            out.append(dict(kind="groupnorm", B=2, HW=hw, C=3 * cpg, G=3, silu=i % 2, opts={}, tag="groupnorm_kernel"))
        for i, cpg in enumerate(GN_CPG):
            out.append(dict(kind="groupnorm", B=2, HW=(129, 31)[i % 2], C=3 * cpg, G=3, silu=(i + 1) % 2, opts={}, tag="groupnorm_kernel"))
    elif family == "layernorm":
        out += [dict(kind="layernorm", M=5, C=c, ldx_extra=8 * (c % 16 == 0), opts={}, tag="layernorm_kernel") for c in LN_C_ALL]
        out += [dict(kind="layernorm", M=m, C=c, ldx_extra=8, opts={}, tag="layernorm_kernel") for m in LN_M for c in (8, 320, 2048)]
    elif family == "softmax":
        out += [dict(kind="softmax", rows=(1, 5)[t % 2], T=t, ldy=roundup(t, 8) + 8 * (t % 3 == 0), opts={}, tag="softmax_rows_kernel") for t in SM_T]
    elif family == "elementwise":
        for i, c in enumerate(EW_C):
            for vec in (False, True):
                if vec and c % 8: continue
                for op in EW_OPS:
                    out.append(dict(kind="ew", op=op, M=EW_M[i % 3], C=c, vec=vec, opts={}, tag="ew_vec8_kernel" if vec else "ew_scalar_kernel"))
    elif family == "layout":
        for c in LAYOUT_C:
            for n in LAYOUT_HW:
                H, W = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13)}[n]
                out.append(dict(kind="layout", B=2, C=c, H=H, W=W, opts={}, tag="ew_scalar_kernel"))
        for c, tag in ((8, "ew_upsample_vec8_kernel"), (5, "ew_scalar_kernel")):
            out.append(dict(kind="upsample", B=2, C=c, Hi=4, Wi=7, Ho=7, Wo=13, opts={}, tag=tag))
    return out


def _norm_hits(c, family):
    if family == "groupnorm":
        return {("HW", c["HW"]), ("cpg", c["C"] // c["G"]), ("silu", c["silu"])}
    if family == "layernorm":
        h = {("C", c["C"]), ("M", c["M"], c["C"])}
        if c["ldx_extra"]: h.add(("ldx>C", 1))
        return h
    if family == "softmax":
        h = {("T", c["T"]), ("rows", c["rows"])}
        if c["ldy"] > c["T"]: h.add(("pad", 1))
        return h
    if family == "elementwise":
        return {("C", c["C"], "vec8" if c["vec"] else "scalar"), ("M", c["M"]), ("op", c["op"])}
    if c["kind"] == "upsample":
        assert c["Ho"] == 2 * c["Hi"] - 1
        return {("upsample", "2Hi-1")}
    return {("C", c["C"]), ("HW", c["H"] * c["W"])}


# ---- direct conv: the three kernels of elementwise.hip:490-510 ----
DIRECT_COUT = (1, 2, 3, 4, 5, 8, 9)
DIRECT_CIN = (4, 64, 128, 320, 336, 344)
DIRECT_WS_M = (65536, 65537, 65551, 65599)
DIRECT_LINEAR_K = (189, 216)


def direct_tag(c):
    """elementwise.hip:490-510: K-parallel from K >= 512 with Cout <= 8 and 16-byte channel rows; weight-stationary with Cout <= 4, at most
    384 (tap, 8-channel) chunks and M >= 65536."""
    kpar = c["Cout"] <= 8 and c["Cin"] % 8 == 0 and c["K"] >= 512
    if kpar and c["Cout"] <= 4 and c["k"] * c["k"] * (c["Cin"] // 8) <= 384 and c["M"] >= 65536:
        return "conv_direct_kpar_ws_kernel"
    return "conv_direct_kpar_kernel" if kpar else "conv_direct_simple_kernel"


def _direct_case(B, Hi, Wi, Cin, Cout, k, pad, **kw):
    c = conv_case(B, Hi, Wi, Cin, Cout, k, 1, pad, {}, "", **kw)
    c["kind"] = "conv_direct"
    c["tag"] = direct_tag(c)
    return c


def _direct_cells():
    ce = [("Cout", n) for n in DIRECT_COUT] + [("Cin", n) for n in DIRECT_CIN] + [("linear", k) for k in DIRECT_LINEAR_K] + [("ws_M", m) for m in DIRECT_WS_M]
    return ce + [("ws_Cin", 320), ("ws_Cin", 336), ("leaves_ws", 344)] + [("kernel", k) for k in ("simple", "kpar", "kpar_ws")]


def _direct_cases():
    out = [_direct_case(2, 5, 7, (64, 128)[i % 2], co, 3, (1, 1), R=(i % 2 == 0)) for i, co in enumerate(DIRECT_COUT)]
    out += [_direct_case(2, 5, 7, ci, (3, 4)[i % 2], 3, (1, 1), epi=2 * (i % 2)) for i, ci in enumerate(DIRECT_CIN)]
    out += [_direct_case(2, 5, 7, k, 5, 1, (0, 0)) for k in DIRECT_LINEAR_K]
    for i, m in enumerate(DIRECT_WS_M):          # one image row of M pixels below a 3-row input without padding: every tap inside the image
        out.append(_direct_case(1, 3, m + 2, 64, (3, 4)[i % 2], 3, (0, 0), R=(i % 2 == 1)))
    out += [_direct_case(1, 256, 256, ci, 4, 3, (1, 1)) for ci in (320, 336, 344)]
    return out


def _direct_hits(c):
    kern = c["tag"][len("conv_direct_"):-len("_kernel")]
    h = {("kernel", kern)}
    if c["k"] == 1: return h | {("linear", c["K"])}
    if c["M"] >= 65536:
        if c["Cin"] == 64: h.add(("ws_M", c["M"]))
        else: h.add(("ws_Cin", c["Cin"]) if kern == "kpar_ws" else ("leaves_ws", c["Cin"]))
        return h
    return h | {("Cout", c["Cout"]), ("Cin", c["Cin"])}


# ---- two-stage GroupNorm (norm.hip:473-513) ----
GN2_C = (64, 320, 2560, 5120)


def gn2_plan(B, HW, C):
    """(pixel rows per chunk, chunks) as mdx_groupnorm_bf16 cuts an image: norm.hip:484-492."""
    C8 = C // 8
    rows = 1 if C8 >= 256 else 256 // C8
    pch = max(-(-HW // max(1, 4096 // B)), rows * const("gn2.U"))
    pch = min(roundup(pch, rows), HW)
    return pch, -(-HW // pch)


def _gn2_cells():
    return [("C", c) for c in GN2_C] + [("tail", t) for t in ("1", "all-but-1")] + [("fin", v) for v in (0, 16)] + [("rev", v) for v in (0, 1)] + \
           [("silu", v) for v in (0, 1)] + [("finalize", v) for v in (0, 1)]


def _gn2_cases():
    out = []
    for i, (C, tail) in enumerate([(C, t) for C in GN2_C for t in (0, 1)]):
        rows = 1 if C // 8 >= 256 else 256 // (C // 8)
        pch = rows * const("gn2.U")
        HW = 17 * pch + 1 if tail == 0 else 18 * pch - 1                 # 18 chunks: more than GN_FINALIZE_CHUNKS = 16
        assert gn2_plan(2, HW, C) == (pch, 18) and HW * C >= 32768
        out.append(dict(kind="groupnorm", B=2, HW=HW, C=C, G=32, silu=(i // 4) % 2, ws=True,
                        opts=dict(GN_ONE_KERNEL_ELEMS=0, GN_FINALIZE_CHUNKS=(0, 16)[i % 2], GN_REVERSE=(i // 2) % 2), tag="gn_stats_kernel+gn_apply_kernel"))
    return out


def _gn2_hits(c):
    pch, n = gn2_plan(c["B"], c["HW"], c["C"])
    tail = c["HW"] - (n - 1) * pch
    fin = c["opts"]["GN_FINALIZE_CHUNKS"]
    h = {("C", c["C"]), ("fin", fin), ("rev", c["opts"]["GN_REVERSE"]), ("silu", c["silu"]), ("finalize", int(fin > 0 and n > fin))}
    if tail == 1: h.add(("tail", "1"))
    if tail == pch - 1: h.add(("tail", "all-but-1"))
    return h


# ---- the LayerNorm pre-step into ln_scratch and the row-statistics post-step of the routes that cannot fuse them (gemm_conv.hip:427-483) ----
STEP_OPTS = dict(GEMM_WS=0, GEMM_XL=0, GEMM_BM=64, GEMM_BN=64)
ROWSTAT_NARROW = (12, 324)                      # C % 8 != 0: the element loop of rowstat_kernel (norm.hip:603-605)


def _steps_cells(step):
    ce = [("C", c) for c in LN_C_ALL] + [("M", m, c) for m in LN_M for c in (8, 320, 2048)]
    return ce + ([("narrow", n) for n in ROWSTAT_NARROW] if step == "rowstat" else [])


def _steps_cases(step):
    tag = generic_tag(64, 64, 64)
    shapes = [(5, c) for c in LN_C_ALL] + [(m, c) for m in LN_M for c in (8, 320, 2048)]
    if step == "ln":
        return [gemm_case(m, 8, c, STEP_OPTS, tag, bias=True, ln=("scratch", 0)) for m, c in shapes]
    return [gemm_case(m, c, 8, STEP_OPTS, "rowstat_kernel", bias=True, rowstat=2) for m, c in shapes + [(5, n) for n in ROWSTAT_NARROW]]


def _steps_hits(c, step):
    C = c["K"] if step == "ln" else c["N"]
    return {("narrow", C)} if C % 8 else {("C", C), ("M", c["M"], C)}


# ---- Fourier embedding, gather, timestep embedding, the DDIM step (elementwise.hip:327-455: one thread per output element / feature) ----
MISC_N = (1, 63, 65)
FOURIER_F = (0, 1, 16)
DDIM_N = (1, 3, 255, 256, 257, 1025)
DDIM_C = 4


def _misc_cells():
    ce = [("fourier", n, f) for n in MISC_N for f in FOURIER_F] + [("gather", n) for n in MISC_N] + [("timeemb", n) for n in MISC_N]
    ce += [("ddim_flat", n) for n in DDIM_N] + [("ddim_padded", n, ld) for n in DDIM_N for ld in (4, 8)] + [("ddim_gv", m) for m in (1, 2)] + [("cfg", v) for v in (0, 1)]
    return ce


def _misc_cases():
    out = [dict(kind="fourier", n=n, P=2, F=f, opts={}, tag="fourier_kernel") for n in MISC_N for f in FOURIER_F]
    out += [dict(kind="gather", n=n, C=(8, 72, 64)[i], add=i % 2, opts={}, tag="gather_add_kernel" if i % 2 else "gather_kernel") for i, n in enumerate(MISC_N)]
    out += [dict(kind="timeemb", n=n, dim=320, opts={}, tag="timeemb_kernel") for n in MISC_N]
    for i, n in enumerate(DDIM_N):               # x_in as a flat fp32 copy, and as 16-bit channels-last rows of DDIM_C channels with pitch 4 / 8
        out.append(dict(kind="ddim", n=n, cfg=i % 2, xin_ld=0, gv=0, opts={}, tag="ddim_kernel"))
        out += [dict(kind="ddim", n=DDIM_C * n, cfg=(i + j) % 2, xin_ld=ld, gv=0, opts={}, tag="ddim_kernel") for j, ld in enumerate((4, 8))]
    out += [dict(kind="ddim", n=DDIM_C * 257, cfg=1, xin_ld=8, gv=m, opts={}, tag="ddim_kernel") for m in (1, 2)]      # 4 views of 257 elements
    return out


def _misc_hits(c):
    k = c["kind"]
    if k == "fourier": return {("fourier", c["n"], c["F"])}
    if k in ("gather", "timeemb"): return {(k, c["n"])}
    h = {("cfg", c["cfg"])}
    if c["gv"]: return h | {("ddim_gv", c["gv"])}
    return h | ({("ddim_padded", c["n"] // DDIM_C, c["xin_ld"])} if c["xin_ld"] else {("ddim_flat", c["n"])})


FAMILIES = {}
for _r in GENERIC_TILES:
    FAMILIES["gemm_generic:" + _r] = (functools.partial(_generic_cells, _r), functools.partial(_generic_cases, _r), functools.partial(_generic_hits, route=_r))
for _r in ("plain", "geglu", "vt", "ln", "rowstat"):
    FAMILIES["gemm_ws:" + _r] = (functools.partial(_ws_cells, _r), functools.partial(_ws_cases, _r), functools.partial(_ws_hits, route=_r))
for _bn in const("gemm_xl.BN"):
    FAMILIES["gemm_xl:%d" % _bn] = (functools.partial(_xl_cells, _bn), functools.partial(_xl_cases, _bn), functools.partial(_xl_hits, bn=_bn))
for _r in list(CONV_TILES) + ["xl"]:
    FAMILIES["conv:" + _r] = (functools.partial(_conv_cells, _r), functools.partial(_conv_cases, _r), functools.partial(_conv_hits, route=_r))
for _nw in const("attn.NW"):
    FAMILIES["attn:nw%d" % _nw] = (functools.partial(_attn_cells, _nw), functools.partial(_attn_cases, _nw), functools.partial(_attn_hits, nw=_nw))
for _r in list(ATTN2_ROUTES) + ["resident", "xview", "joint"]:
    FAMILIES["attn2:" + _r] = (functools.partial(_attn2_cells, _r), functools.partial(_attn2_cases, _r), functools.partial(_attn2_hits, route=_r))
for _d in (32, 64):
    FAMILIES["attn_short:d%d" % _d] = (functools.partial(_short_cells, _d), functools.partial(_short_cases, _d), functools.partial(_short_hits, d=_d))
for _f in ("groupnorm", "layernorm", "softmax", "elementwise", "layout"):
    FAMILIES[_f] = (functools.partial(_norm_cells, _f), functools.partial(_norm_cases, _f), functools.partial(_norm_hits, family=_f))


FAMILIES["misc"] = (_misc_cells, _misc_cases, _misc_hits)
FAMILIES["conv_direct"] = (_direct_cells, _direct_cases, _direct_hits)
FAMILIES["groupnorm2"] = (_gn2_cells, _gn2_cases, _gn2_hits)
for _s in ("ln", "rowstat"):
    FAMILIES["gemm_steps:" + _s] = (functools.partial(_steps_cells, _s), functools.partial(_steps_cases, _s), functools.partial(_steps_hits, step=_s))


def cells(family):
    return list(FAMILIES[family][0]())


@functools.lru_cache(maxsize=None)
def _cases_cached(family):
    return tuple(FAMILIES[family][1]())


def cases(family):
    return list(_cases_cached(family))


def hits(family, case):
    return FAMILIES[family][2](case)


def label(c):
    skip = ("kind", "opts", "tag")
    return c["kind"] + "(" + ",".join(f"{k}={v}" for k, v in c.items() if k not in skip and v not in (None, False, 0, {})) + ")"


def math_key(c):
    """What the reference of a case depends on (not the route): cases with the same key share their sensitivity verdict."""
    return tuple(sorted((k, repr(v)) for k, v in c.items() if k not in ("opts", "tag", "ldv_extra", "ldx_extra", "ldy", "vec")))


# --------------------------------------------------------------------------------------------------------------------------------------
# route lines for tests/gemm_route_check.cpp (as gemm_route_table.route_lines builds them; the views of the GPU test: lda = K + 8, C / R
# 16-byte aligned with ldc = roundup8(nout) + 8 when nout % 8 == 0, else roundup4(nout) + 4)
# --------------------------------------------------------------------------------------------------------------------------------------
WS_BYTES = 4 << 20


VT_FROM = 128                  # fused V^T cases: columns 0..127 go to C, the rest transposed to Vt (vt_from % 128 == 0)


def out_cols(c):
    """Columns of the C / R views."""
    if c["kind"] == "gemm" and c["vt"]:
        return VT_FROM
    return c["N"] // 2 if c["epi"] == 1 else c["N"]


def ldc_of(c):
    n = out_cols(c)
    return roundup(n, 8) + 8 if n % 8 == 0 else roundup(n, 4) + 4


def route_line(c):
    n = out_cols(c)
    ldc = ldc_of(c)
    f = dict(M=c["M"], N=c["N"], K=c["K"], epi=c["epi"], splitk=c["splitk"], ldc=ldc, ldr=ldc if c["R"] else 0, wide=int(n % 8 == 0 and not c.get("c_f32")),
             has_ws=1, ws_bytes=WS_BYTES, bias=int(c["bias"]), R=int(c["R"]), temb=int(c["temb"] > 0))
    if c["kind"] == "gemm":
        ln = c["ln"]
        f.update(lda=c["K"] + 8, ldw=c["K"] + 8, batch=c["batch"], c_f32=int(c["c_f32"]), rows_per_b=c["temb"] or 1, ln=int(ln is not None),
                 ln_csum=int(ln is not None), ln_scratch=int(bool(ln and ln[0] == "scratch")), ln_stats=int(bool(ln and ln[1])), ln_stats_parts=ln[1] if ln else 0,
                 rowstat=int(c["rowstat"] > 0), rowstat_parts=c["rowstat"])
    else:
        f.update(conv=1, lda=c["Cin"] + 8, ldw=c["K"], rows_per_b=c["Ho"] * c["Wo"], Hi=c["Hi"], Wi=c["Wi"], Cin=c["Cin"], Ho=c["Ho"], Wo=c["Wo"],
                 kh=c["k"], kw=c["k"], sh=c["stride"], sw=c["stride"], ph=c["pad"][0], pw=c["pad"][1], cimajor=int(c["k"] > 1 and c["Cin"] % 64 == 0))
    opts = {k: v for k, v in c["opts"].items() if k in ROUTE_OPTS}
    return " ".join(f"{k}={v}" for k, v in {**f, **opts}.items())


ROUTE_OPTS = ("GEMM_WS", "GEMM_XL", "XL_K320", "XL_MIN_TILES", "XL_BN", "XL_GEGLU320", "GEMM_SMALL_TILES", "GEMM_BM256", "GEMM_BM", "GEMM_BN",
              "GEMM_BK", "GEMM_FLATTEN", "LN_FUSE", "LN_STATS", "GEMM_TIMING")


# --------------------------------------------------------------------------------------------------------------------------------------
# tail-weighted inputs (seeded, rounded to the storage type before any reference sees them)
# --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _base(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def randn(*shape, seed=0, scale=1.0):
    if math.prod(shape) > (1 << 22):          # large operands are not worth keeping
        return _base.__wrapped__(tuple(shape), seed) * scale
    return _base(tuple(shape), seed) * scale


def attn_offset(d):
    """a with a^2 d^-1/2 = 6: q[..., 0] = a, k[..., 0] = -a put a common -6 on every logit."""
    return math.sqrt(6.0 * math.sqrt(d))


def norm_offset(n):
    """Common offset of a norm row / group of n elements: +4, raised to sqrt(n) / 4 for long rows — a divisor off by one changes the variance
    by about offset^2 / n (relative), which the +4 of the short rows no longer lifts over close() beyond n ~ 256."""
    return max(4.0, math.sqrt(n) / 4.0)


SOFTMAX_SPIKE = 12.0         # ... and the last logit is +12, not +8: its probability then stays above 0.96 for every T here.  In [0.5, 0.6) an honest fp16
                             # store (half an ulp = 2^-12) is itself over the fp16 table's 4e-4 |ref|, which +8 reaches at T of a thousand or two
SOFTMAX_OFFSET = -12.0       # the softmax offset is NEGATIVE: a phantom zero logit must outweigh the row (at +4 it would add 1 to a sum of ~e^12)


def inputs(c, dtype, seed=0):
    """The rounded operands of a case on the CPU (dict of tensors; side operands fp32)."""
    k = c["kind"]
    if k == "gemm":
        M, N, K, Bt = c["M"], c["N"], c["K"], c["batch"]
        lead = (Bt,) if Bt > 1 else ()
        A = randn(*lead, M, K, seed=seed + 1).clone(); W = randn(*lead, N, K, seed=seed + 2, scale=K ** -0.5).clone()
        A[..., K - 8:] *= 4.0; A[..., M - 1, :] *= 2.0
        if c["epi"] == 1:
            W[..., N // 2 - 4:N // 2, :] *= 2.0
        else:
            W[..., max(0, N - 4):, :] *= 2.0
        d = dict(A=A.to(dtype), W=W.to(dtype))
        if c["ln"] is not None:                      # raw rows with their own offsets; W carries a folded gamma (values_data.ln_offset_inputs)
            d["A"] = (A * 1.5 + 0.7 + 6.0 * (torch.arange(M) % 7 == 0)[:, None]).to(dtype)
        if c["bias"]:
            b = randn(N, seed=seed + 3).clone(); b[(N // 2 if c["epi"] == 1 else N) - 1] += 3.0
            d["bias"] = b.float()
        if c["R"]:
            d["R"] = randn(*lead, M, out_cols(c), seed=seed + 4).to(F32 if c["c_f32"] else dtype)
        if c["temb"]:
            d["temb"] = randn(-(-M // c["temb"]), N, seed=seed + 5).float()
        return d
    if k in ("conv", "conv_direct"):
        x = randn(c["B"], c["Hi"], c["Wi"], c["Cin"], seed=seed + 1).clone()
        w = randn(c["Cout"], c["k"], c["k"], c["Cin"], seed=seed + 2, scale=c["K"] ** -0.5).clone()
        ky, kx = last_live_tap(c)
        w[:, ky, kx, max(0, c["Cin"] - 8):] *= 4.0             # the last 8 channels of the last tap that reads the image at all
        w[max(0, c["Cout"] - 4):] *= 2.0
        b = randn(c["Cout"], seed=seed + 3).clone(); b[-1] += 3.0
        d = dict(x=x.to(dtype), w=w.to(dtype), bias=b.float())
        if c["R"]: d["R"] = randn(c["B"], c["Ho"], c["Wo"], c["Cout"], seed=seed + 4).to(dtype)
        if c["temb"]: d["temb"] = randn(c["B"], c["Cout"], seed=seed + 5).float()
        return d
    if k == "attn":
        B, H, Tq, Tk, dd = c["B"], c["H"], c["Tq"], c["Tk"], c["d"]
        q = randn(B, Tq, H, dd, seed=seed + 1).clone(); kk = randn(c["Bkv"], Tk, H, dd, seed=seed + 2).clone(); v = randn(c["Bkv"], Tk, H, dd, seed=seed + 3).clone()
        a = attn_offset(dd)
        q[..., 0] = a; kk[..., 0] = -a
        v[:, Tk - 1] += 3.0
        q = q.reshape(B, Tq, H * dd).to(dtype)
        d = dict(q=q, k=kk.reshape(c["Bkv"], Tk, H * dd).to(dtype), v=v.reshape(c["Bkv"], Tk, H * dd).to(dtype))
        if c["pre"]:
            d["q"], d["qref"] = V.prescale(q, dd)
        return d
    if k == "groupnorm":
        B, HW, C, G = c["B"], c["HW"], c["C"], c["G"]
        cpg = C // G
        off = norm_offset(HW * cpg)
        x = randn(B, HW, C, seed=seed + 1) + off
        x[:, HW - 1, cpg - 1::cpg] += 2.0 * off                 # the last element of every group
        return dict(x=x.to(dtype), gamma=(1.0 + randn(C, seed=seed + 2, scale=0.3)).float(), beta=randn(C, seed=seed + 3, scale=0.3).float())
    if k == "layernorm":
        M, C = c["M"], c["C"]
        off = norm_offset(C)
        x = randn(M, C, seed=seed + 1) + off
        x[:, C - 1] += 2.0 * off
        return dict(x=x.to(dtype), gamma=(1.0 + randn(C, seed=seed + 2, scale=0.3)).float(), beta=randn(C, seed=seed + 3, scale=0.3).float())
    if k == "softmax":
        x = randn(c["rows"], c["T"], seed=seed + 1) + SOFTMAX_OFFSET
        x[:, -1] += SOFTMAX_SPIKE
        return dict(x=x.float(), scale=1.0)
    if k == "ew":
        x = randn(c["M"], c["C"], seed=seed + 1, scale=2.0).clone(); y0 = randn(c["M"], c["C"], seed=seed + 2).clone()
        x[:, -1] = 5.0 + torch.arange(c["M"]) % 3; y0[:, -1] = -9.0
        return dict(x=x.to(dtype), y0=y0.to(dtype), alpha=0.37)
    if k == "layout":
        x = randn(c["B"], c["C"], c["H"], c["W"], seed=seed + 1).clone()
        x[:, -1, -1, -1] = 7.0 + torch.arange(c["B"])
        return dict(x=x.to(dtype))
    if k == "upsample":
        x = randn(c["B"], c["Hi"], c["Wi"], c["C"], seed=seed + 1).clone()
        x[:, -1, -1, -1] = 7.0 + torch.arange(c["B"])
        return dict(x=x.to(dtype))
    if k == "fourier":                           # |x| <= 0.5: arguments up to 2^15 / 2 rad at F = 16, the range tests/test_values_gpu.py holds the kernel to
        x = (torch.rand(c["n"], c["P"], 3, generator=torch.Generator().manual_seed(seed + 1)) - 0.5).float()
        return dict(x=x, mask=(torch.arange(c["n"]) % 3 != 1).to(torch.uint8), null=randn(c["P"] * (3 + 6 * c["F"]), seed=seed + 2).float())
    if k == "gather":
        rows = 10
        idx = (torch.arange(c["n"]) * 7) % rows
        idx[-1] = rows - 1
        return dict(table=randn(rows, c["C"], seed=seed + 1).to(dtype), idx=idx.long(), add=randn(3, c["C"], seed=seed + 2).to(dtype))
    if k == "timeemb":
        return dict(t=((torch.arange(c["n"]) * 15.5 + 903.25) % 1000.0).float())
    if k == "ddim":
        n = c["n"]
        d = dict(x=randn(n, seed=seed + 1).float(), eps=randn((2 if c["cfg"] else 1) * n, seed=seed + 2).float(),
                 coef=torch.tensor([[0.9, 0.4359, 0.95, 0.3122], [0.95, 0.3122, 0.99, 0.1411]]), guidance=2.0)
        if c["gv"]:
            d.update(cond=randn(n, seed=seed + 3).float(), noise=randn(n, seed=seed + 4).float(), mask=torch.tensor([0, 1, 0, 1], dtype=torch.uint8))
        return d
    raise KeyError(k)


# --------------------------------------------------------------------------------------------------------------------------------------
# fp64 references, with at most one tail error (`mut`)
# --------------------------------------------------------------------------------------------------------------------------------------
def _gelu64(g):
    return 0.5 * g * (1.0 + torch.erf(g * 0.7071067811865476))


def _epilogue(c, x, d, mut):
    """bias, temb rows, activation, residual on the fp64 product x [*, M, N]; shared by the GEMM and the conv reference."""
    M, N = x.shape[-2:]
    if c["bias"]:
        b = d["bias"].to(x.device, F64)
        if mut == "bias_shifted_by_4":
            b = torch.roll(b, min(4, N - 1))
        x = x + b
    if c["temb"]:
        rpb = c["temb"] if c["kind"] == "gemm" else c["Ho"] * c["Wo"]
        img = torch.arange(M, device=x.device) // rpb
        if mut == "temb_row_of_previous_image":
            img = torch.where(img == img.max(), img - 1, img)
        x = x + d["temb"].to(x.device, F64)[img]
    if c["epi"] == 2:
        x = F.silu(x)
    elif c["epi"] == 1:
        x = x[..., :N // 2] * _gelu64(x[..., N // 2:])
    if c["R"]:
        x = x + d["R"].to(F64).reshape(x.shape)
    if mut == "drop_last_row":
        x = x.clone(); x[..., -1, :] = 0.0
    if mut == "last_cols_from_previous":
        w = min(4, x.shape[-1] // 2)
        x = x.clone(); x[..., -w:] = x[..., -2 * w:-w]
    return x


def _ln64(x, eps=1e-5):
    return (x - x.mean(-1, keepdim=True)) * (x.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()


def gemm_eval(c, d, mut=None):
    """fp64 epi(A W^T + bias + temb[row]) + R of a GEMM case [*, M, N out] (GEGLU: W rows are [value | gate], unpacked; a fused LayerNorm
    normalises the A rows first)."""
    A, W = d["A"].double(), d["W"].double()
    if c["ln"] is not None:
        A = _ln64(A)
        if c["ln"][0] == "scratch":                  # the route keeps the normalised rows in 16 bits (ln_scratch): the reference rounds them too
            A = A.to(d["A"].dtype).double()
    if mut == "drop_last_k8":
        A = A[..., :-8]; W = W[..., :-8]
    elif mut == "double_last_k8":
        A = A.clone(); A[..., -8:] *= 2.0
    x = A @ W.transpose(-1, -2) if A.shape[-1] else torch.zeros(*A.shape[:-1], W.shape[-2], dtype=F64, device=A.device)
    return _epilogue(c, x, d, mut)


def conv_eval(c, d, mut=None):
    """fp64 conv [B, Ho, Wo, Cout] with stride, start pad and end pad (values_data.conv_ref is the 3x3 / stride 1 / pad 1 case of it)."""
    x = d["x"].double().permute(0, 3, 1, 2); w = d["w"].double().permute(0, 3, 1, 2)
    if mut in ("drop_last_k8", "double_last_k8"):
        ky, kx = last_live_tap(c)
        w = w.clone(); w[:, -8:, ky, kx] *= (0.0 if mut == "drop_last_k8" else 2.0)
    (ph, pw), (phe, pwe) = c["pad"], c["pad_end"]
    y = F.conv2d(F.pad(x, (pw, pwe, ph, phe)), w, stride=c["stride"]).permute(0, 2, 3, 1)
    B, Ho, Wo, Co = y.shape
    return _epilogue(c, y.reshape(B * Ho * Wo, Co), d, mut).reshape(B, Ho, Wo, Co)


def _attn64(q, k, v, H, scale, mask=None):
    B, Tq, C = q.shape
    dd = C // H
    qh = q.double().reshape(B, Tq, H, dd).transpose(1, 2); kh = k.double().reshape(B, -1, H, dd).transpose(1, 2)
    vh = v.double().reshape(B, -1, H, dd).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * scale
    if mask is not None:
        s = s.masked_fill(mask.to(s.device), -math.inf)
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Tq, C)


def attn_sources(c):
    """kv batches of query batch b (negative: absent slot)."""
    return (lambda b: c["kvmap"][b]) if c["kvmap"] is not None else (lambda b: [b])


def attn_eval(c, d, mut=None):
    """fp64 attention [B, Tq, H d]: one softmax per source summed (an absent slot contributes nothing, no source at all gives zeros), or one
    softmax over the concatenated sources (joint); causal: query t sees keys 0..t."""
    q = d.get("qref", d["q"]).double(); k, v = d["k"].double(), d["v"].double()
    H, scale = c["H"], c["d"] ** -0.5
    srcs = attn_sources(c)
    outs = []
    for b in range(c["B"]):
        js = [j for j in srcs(b) if j >= 0]
        parts = [(k[j], v[j]) for j in js]
        if parts and mut == "drop_last_key":
            parts[-1] = (parts[-1][0][:-1], parts[-1][1][:-1])
        if parts and mut == "phantom_zero_key":
            z = torch.zeros(1, k.shape[-1], dtype=F64, device=k.device)
            parts[-1] = (torch.cat([parts[-1][0], z]), torch.cat([parts[-1][1], z]))
        parts = [p for p in parts if p[0].shape[0]]
        if c["joint"] and parts:
            parts = [(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))]
        o = torch.zeros(c["Tq"], q.shape[-1], dtype=F64, device=q.device)
        for kk, vv in parts:
            mask = None
            if c["causal"]:
                t = torch.arange(c["Tq"])[:, None]; j = torch.arange(kk.shape[0])[None, :]
                mask = (j > (t + 1 if mut == "causal_off_by_one" else t)) & (j < c["Tk"])      # a phantom key is past the mask's extent: visible
            o = o + _attn64(q[b:b + 1], kk[None], vv[None], H, scale, mask)[0]
        outs.append(o)
    out = torch.stack(outs)
    if mut == "last_query_from_previous":
        out[:, -1] = out[:, -2]
    return out


def _stats_mut(x, dims, mut):
    """(mean, var) over `dims` of x (the last listed dim's last index is "the last element"), with the counting errors of the norm mutants."""
    n = 1
    for dm in dims: n *= x.shape[dm]
    s1 = x.sum(dims, keepdim=True); s2 = (x * x).sum(dims, keepdim=True)
    if mut == "drop_last_element":
        last = x
        for dm in dims: last = last.narrow(dm, last.shape[dm] - 1, 1)
        s1 = s1 - last; s2 = s2 - last * last; n -= 1
    if mut == "count_one_more": n += 1
    if mut == "count_one_less": n -= 1
    mean = s1 / n
    return mean, s2 / n - mean * mean


def norm_eval(c, d, mut=None):
    k = c["kind"]
    x = d["x"].double()
    if k == "softmax":
        e = torch.exp((x - x.max(-1, keepdim=True).values) * d["scale"])
        den = e.sum(-1, keepdim=True)
        if mut == "count_one_more": den = den + torch.exp(-x.max(-1, keepdim=True).values * d["scale"])
        if mut in ("count_one_less", "drop_last_element"): den = den - e[:, -1:]
        p = e / den
        if mut == "drop_last_element": p = p.clone(); p[:, -1] = 0.0
        return p
    g, b = d["gamma"].to(x.device, F64), d["beta"].to(x.device, F64)
    if k == "layernorm":
        if mut is None:
            return F.layer_norm(x, (c["C"],), g, b, 1e-5)
        mean, var = _stats_mut(x, (1,), mut)
        return (x - mean) * (var + 1e-5).rsqrt() * g + b
    B, HW, C = x.shape
    if mut is None:
        y = V.gn_ref(x, c["G"], g, b, 1e-5, False)
    else:
        xg = x.reshape(B, HW, c["G"], C // c["G"])
        mean, var = _stats_mut(xg, (1, 3), mut)
        y = ((xg - mean) * (var + 1e-5).rsqrt()).reshape(B, HW, C) * g + b
    return F.silu(y) if c["silu"] else y


def ew_eval(c, d, mut=None):
    k = c["kind"]
    x = d["x"].double()
    if k == "ew":
        y = {"ADD": lambda: d["y0"].double() + x, "COPY": lambda: x, "SILU": lambda: x * torch.sigmoid(x),
             "SCALE": lambda: x * float(torch.tensor(d["alpha"], dtype=F32))}[c["op"]]()
    elif k == "layout":
        y = x.permute(0, 2, 3, 1)                                # NCHW -> NHWC (the way back is checked bit for bit against the input)
    else:
        from magicdrive_amd.packing import nearest_index
        y = x[:, nearest_index(c["Hi"], c["Ho"]).long()][:, :, nearest_index(c["Wi"], c["Wo"]).long()]
    if mut == "last_element_from_previous":
        shape = y.shape
        y = y.clone().reshape(-1, shape[-1]) if shape[-1] > 1 else y.clone().reshape(1, -1)       # one channel: the last element of the tensor
        y[:, -1] = y[:, -2]
        y = y.reshape(shape)
    return y


def misc_eval(c, d, mut=None):
    k = c["kind"]
    if k == "fourier":
        y = V.fourier_ref(d["x"].cpu(), c["F"], BF16)[0].to(d["x"].device)
        m = d["mask"].to(y.device).double()[:, None]
        y = y * m + d["null"].to(y.device).double()[None] * (1 - m)
    elif k == "gather":
        y = d["table"].double()[d["idx"]]
        if c["add"]:
            y = y + d["add"].double()[torch.arange(c["n"], device=y.device) % 3]
    elif k == "timeemb":
        y = V.timeemb_ref(d["t"].cpu(), c["dim"]).to(d["t"].device)
    else:
        n = c["n"]
        x, eps, (c0, c1, c2, c3) = d["x"].double(), d["eps"].double(), [float(v) for v in d["coef"][0]]
        e = eps[:n] + float(d["guidance"]) * (eps[n:] - eps[:n]) if c["cfg"] else eps
        if c["gv"]:
            g = d["mask"].to(x.device).bool().repeat_interleave(n // 4)
            if c["gv"] == 2: e = torch.where(g, d["noise"].double(), e)
        y = c2 * (x - c1 * e) / c0 + c3 * e
        if c["gv"] == 1:                          # not the last step (gv_last_step = 1): the known views are re-noised
            y = torch.where(g, c2 * d["cond"].double() + c3 * d["noise"].double(), y)
        y = y[None]
    if mut == "last_element_from_previous":
        y = y.clone(); y[:, -1] = y[:, -2]
    return y


EVAL = dict(fourier=misc_eval, gather=misc_eval, timeemb=misc_eval, ddim=misc_eval, gemm=gemm_eval, conv=conv_eval, conv_direct=conv_eval, attn=attn_eval, groupnorm=norm_eval, layernorm=norm_eval, softmax=norm_eval, ew=ew_eval, layout=ew_eval,
            upsample=ew_eval)


def reference(c, d):
    return EVAL[c["kind"]](c, d)


MUTANTS = dict(
    gemm=("drop_last_k8", "double_last_k8", "drop_last_row", "last_cols_from_previous", "bias_shifted_by_4", "temb_row_of_previous_image"),
    attn=("drop_last_key", "phantom_zero_key", "last_query_from_previous", "causal_off_by_one"),
    norm=("count_one_more", "count_one_less", "drop_last_element"),
    ew=("last_element_from_previous",))
MUTANTS["conv"] = MUTANTS["conv_direct"] = MUTANTS["gemm"]
for _k in ("groupnorm", "layernorm", "softmax"): MUTANTS[_k] = MUTANTS["norm"]
for _k in ("layout", "upsample", "fourier", "gather", "timeemb", "ddim"): MUTANTS[_k] = MUTANTS["ew"]

# The ONLY exemptions, by rule (tests/test_tails_cpu.py holds every other (case, mutant) pair to close()):
EXEMPTIONS = (
    "a drop mutant where the extent is 1: drop_last_row at M = 1, drop_last_key at Tk = 1 (one source), drop_last_element at n = 1",
    "count_one_less where n = 1",
    "a bias / temb mutant where the case has none (temb: fewer than two images); causal_off_by_one where the case is not causal",
    "a from-previous mutant where there is no previous: last_cols_from_previous / bias_shifted_by_4 at one output column, "
    "last_query_from_previous at Tq = 1, causal_off_by_one at T = 1, last_element_from_previous at one element",
    "last_query_from_previous where every query attends to ONE key in total (Tk = 1, not causal; summed sources have one key each): all rows of O are equal, so the mutant is the reference",
)


def _norm_n(c):
    return {"groupnorm": lambda: c["HW"] * (c["C"] // c["G"]), "layernorm": lambda: c["C"], "softmax": lambda: c["T"]}[c["kind"]]()


def applicable(c, mut):
    k = c["kind"]
    if k in ("gemm", "conv", "conv_direct"):
        nout = out_cols(c)
        if mut == "drop_last_row": return c["M"] > 1
        if mut == "last_cols_from_previous": return nout > 1
        if mut == "bias_shifted_by_4": return bool(c["bias"]) and c["N"] > 1
        if mut == "temb_row_of_previous_image":
            return bool(c["temb"]) and (c["M"] > c["temb"] if k == "gemm" else c["B"] > 1)
        return True
    if k == "attn":
        keys = c["Tk"] * (max(len([j for j in r if j >= 0]) for r in c["kvmap"]) if c["joint"] else 1)         # keys of one softmax
        if mut == "drop_last_key": return keys > 1
        if mut == "last_query_from_previous": return c["Tq"] > 1 and (keys > 1 or c["causal"])
        if mut == "causal_off_by_one": return c["causal"] and c["Tq"] > 1
        return True
    if k in ("groupnorm", "layernorm", "softmax"):
        return _norm_n(c) > 1 if mut in ("count_one_less", "drop_last_element") else True
    if k in ("fourier", "gather", "timeemb", "ddim"):
        return k != "ddim" or c["n"] > 1
    total = {"ew": lambda: c["M"] * c["C"], "layout": lambda: c["B"] * c["C"] * c["H"] * c["W"], "upsample": lambda: c["B"] * c["C"] * c["Ho"] * c["Wo"]}[k]()
    return total > 1


ABS_BOUND = dict(timeemb=2e-4, ddim=1e-5)      # fp32 outputs held to the absolute bounds of tests/test_kernels_gpu.py instead of close()
F32_REL_L2 = 2e-5             # fp32 GEMM / conv outputs: rel L2 against fp64 (test_kernels_gpu.py::test_conv_out_weight_stationary's bound, tests/test_tails_gpu.py)
ROWSTAT_BOUND = 2e-5          # MdxGemmDesc.rowstat_out: |sum - fp64 sum of the stored C| / (|sum| + 1) (test_kernels_gpu.py::test_gemm_row_statistics_out)
UNIPC_ATOL_REL = 3e-5         # UniPC latents: atol = this x max |ref| (test_kernels_gpu.py::test_cfg_unipc_matches_oracle_scheduler)


def store_dtype(c, dtype):
    return F32 if c["kind"] in ABS_BOUND else dtype


def mutants(c, d, dtype):
    """{name: the fp64 reference recomputed with that one tail error, rounded once to the type it is stored in} for every applicable mutant."""
    return {m: EVAL[c["kind"]](c, d, mut=m).to(store_dtype(c, dtype)) for m in MUTANTS[c["kind"]] if applicable(c, m)}
