"""-m gpu: every kernel at "one less / exact / one more" of its own tile, walk and vector constants (tests/tails_data.py), at the smallest shapes.

One parametrized test per family and forced route; each test loops over its cases.  Per case: the kernel tag (mdx_last_kernel), helpers.close()
against the fp64 reference with the table of the storage type (fp32 outputs: the 2e-5 bound of test_conv_out_weight_stationary), every output
finite, and the poison discipline — every operand is a view inside a larger buffer whose every element outside the valid extent (row pads,
rows past M, K rows past Tk, V^T columns Tk..ldv, the workspace) is NaN, outputs start as NaN, the border must be bit-intact afterwards, and a
second run with 1e4 in place of the NaN must give the same bits: what lies outside the extents never reaches the output.  Stray accesses are
detected by VALUE; no buffer sits at the end of an allocation.  tests/test_tails_cpu.py proves on the CPU that close() rejects each of the
tail errors these inputs are weighted for.  Worst err / tol and rel L2 per family and storage type go to the parity log as tails:<family>:<type>.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from magicdrive_amd import _lib as L
from magicdrive_amd import ops as O
from magicdrive_amd import packing as PK

import tails_data as T  # noqa: E402
import values_data as V  # noqa: E402
from helpers import XF_ATOL, XF_RTOL, close, parity_log  # noqa: E402
from test_edges_gpu import Guarded, last_kernel, side  # noqa: E402
from test_kernels_gpu import rowstat_ref  # noqa: E402

F32 = torch.float32
F64 = torch.float64
DTYPES = [torch.bfloat16, torch.float16]
KIND = {torch.bfloat16: "bf16", torch.float16: "f16"}
NAN = float("nan")
POISONS = (NAN, 1e4)
EPI = {0: L.EPI_NONE, 1: L.EPI_GEGLU, 2: L.EPI_SILU}


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def box(shape, ld, off, dtype, dev, poison, fill=None):
    """test_edges_gpu.Guarded with a choice of poison; a view without `fill` (an output) starts as NaN.  .snap: the buffer as issued."""
    g = Guarded(shape, ld, off, dtype, dev)
    if poison == poison:
        g.buf.fill_(poison)
    g.view.copy_(fill) if fill is not None else g.view.fill_(NAN)
    g.snap = g.buf.clone()
    return g


def intact(g):
    """Everything outside the view still holds the bits it was issued with."""
    mask = torch.ones_like(g.buf, dtype=torch.bool)
    mask.as_strided(g.view.shape, g.view.stride(), g.view.storage_offset()).fill_(False)
    return bool((bits(g.buf)[mask] == bits(g.snap)[mask]).all())


def side_of(vals, off, dev, poison):
    """test_edges_gpu.side: an fp32 side operand `off` floats into a larger poisoned buffer, holding `vals`."""
    s = side(vals.numel(), off, 0, dev)
    if poison == poison:
        s._base.fill_(poison)
    s.copy_(vals.reshape(-1))
    return s


def flat(n, dtype, dev, poison):
    return torch.full((n,), poison, dtype=dtype, device=dev)


def to_dev(d, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def measure(out, ref, kind):
    """(worst err / tol, rel L2) with close()'s formula."""
    o = out.double(); r = ref.double().to(o.device)
    err = (o - r).abs()
    tol = XF_ATOL[kind] * (r.abs().mean() + 1e-6) + XF_RTOL[kind] * r.abs()
    return float((err / tol).max()), float(err.pow(2).sum().sqrt() / (r.pow(2).sum().sqrt() + 1e-12))


class Tally:
    def __init__(self, family, dtype):
        self.family, self.kind, self.worst, self.rel, self.n, self.fails, self.notes = family, KIND[dtype], 0.0, 0.0, 0, [], {}

    def add(self, out, ref):
        w, r = measure(out, ref, self.kind)
        self.worst = max(self.worst, w); self.rel = max(self.rel, r); self.n += 1
        return w, r

    def done(self):
        parity_log(f"tails:{self.family}:{self.kind}", cases=self.n, worst_err_over_tol=self.worst, rel_l2=self.rel, failures=len(self.fails), **self.notes)
        assert not self.fails, (len(self.fails), self.fails[:12])
        assert self.n > 0


def verdict(tally, c, outs_by_poison, refs, boxes_ok, kern, residual_bound=None):
    """The per-case assertions, collected instead of raised so that one run shows every failing case of a family.
    outs_by_poison: [list of output tensors under NaN poison, the same under 1e4]; refs: fp64 references of those outputs (None: bit checks only)."""
    lab = T.label(c)
    if kern != c["tag"]:
        tally.fails.append((lab, "kernel", kern, c["tag"]))
    if not boxes_ok:
        tally.fails.append((lab, "border or pad not bit-intact"))
    a, b = outs_by_poison
    for i, (x, y) in enumerate(zip(a, b)):
        if not torch.equal(bits(x), bits(y)):
            tally.fails.append((lab, f"output {i} depends on what lies outside the extents ({int((bits(x) != bits(y)).sum())} elements differ)"))
    for i, (x, r) in enumerate(zip(a, refs)):
        if r is None:
            continue
        if not bool(torch.isfinite(x.float()).all()):
            tally.fails.append((lab, f"output {i} not finite ({int((~torch.isfinite(x.float())).sum())} elements)"))
            continue
        if x.dtype == F32:
            rel = V.rel_l2(x, r)
            if not rel < T.F32_REL_L2:
                tally.fails.append((lab, f"fp32 output {i}: rel_l2 {rel:.3e} >= 2e-5"))
            continue
        w, rel = tally.add(x, r)
        try:
            close(x, r, name=f"tails:{tally.family}:{lab}", kind=tally.kind)
        except AssertionError as e:
            if residual_bound is not None and i == 0:
                # a residual added to the staged 16-bit tile rounds twice (values_data.B_gemm_residual): held to that derived bound instead,
                # with the close() ratio logged beside it
                rb = V.ratio(x, r.cpu(), residual_bound())
                tally.notes[f"staged_residual:{lab}"] = dict(close_ratio=round(w, 3), bound_ratio=round(rb, 3))
                if rb <= 1.0:
                    continue
            tally.fails.append((lab, str(e)[:300]))


# --------------------------------------------------------------------------------------------------------------------------------------
# GEMM
# --------------------------------------------------------------------------------------------------------------------------------------
def ln_stats(A, parts, dev):
    """(sum, sum of squares) of the raw rows as a producer leaves them: column parts [0,128) [128,256) [256,320), whole rows for one part."""
    K = A.shape[1]
    cuts = {1: [0, K], 2: [0, 128, K], 3: [0, 128, 256, K], 4: [0, 128, 256, K]}[parts]
    st = torch.zeros(parts, A.shape[0], 2, dtype=F32, device=dev)
    a = A.double()
    for i in range(len(cuts) - 1):
        st[i, :, 0] = a[:, cuts[i]:cuts[i + 1]].sum(1).float(); st[i, :, 1] = (a[:, cuts[i]:cuts[i + 1]] ** 2).sum(1).float()
    return st


def run_gemm(c, d, dtype, dev, poison, opts=None):
    M, N, K, Bt = c["M"], c["N"], c["K"], c["batch"]
    lead = (Bt,) if Bt > 1 else ()
    nout = T.out_cols(c)
    ldc = T.ldc_of(c)
    W, bias = d["W"], d.get("bias")
    if c["epi"] == 1:
        W, bias = PK.pack_geglu(W.float().cpu(), bias.cpu(), dtype)
        W, bias = W.to(dev), bias.to(dev)
    A = box(lead + (M, K), K + 8, 0, dtype, dev, poison, fill=d["A"])
    Wb = box(lead + (N, K), K + 8, 0, dtype, dev, poison, fill=W)
    cdt = F32 if c["c_f32"] else dtype
    ncols = T.roundup(nout, 4)                        # N % 4 != 0: the columns up to roundup4(N) are written as zeros (include/mdx.h)
    C = box(lead + (M, ncols), ldc, 0, cdt, dev, poison)
    boxes = [C]
    kw = {}
    if c["R"]:
        R = box(lead + (M, nout), ldc, 0, cdt, dev, poison, fill=d["R"]); boxes.append(R); kw["R"] = R.view
    if bias is not None:
        kw["bias"] = side_of(bias, 4, dev, poison)
    if c["temb"]:
        nimg, tbs = d["temb"].shape[0], N + 4
        tb = flat(nimg * tbs + 8, F32, dev, poison)
        tb[4:4 + nimg * tbs].view(nimg, tbs)[:, :N] = d["temb"]
        kw.update(temb=tb[4:], temb_b_stride=tbs, rows_per_b=c["temb"])
    ws = flat(T.WS_BYTES // 4, F32, dev, poison)
    outs = [C.view[..., :nout]]
    if c["vt"]:
        views, vt_T = c["vt"]
        Vt = box((views, N - T.VT_FROM, vt_T), vt_T + 8, 0, dtype, dev, poison); boxes.append(Vt)
        kw.update(Vt=Vt.view, vt_from=T.VT_FROM, vt_T=vt_T)
        outs.append(Vt.view)
    if c["ln"] is not None:
        kw.update(ln_eps=1e-5, ln_csum=d["W"].float().sum(1).contiguous())
        if c["ln"][1]:
            kw["ln_stats"] = ln_stats(d["A"], c["ln"][1], dev)
        if c["ln"][0] == "scratch":                   # a contiguous [M, lda] buffer: the rows the pre-step writes are exactly the box's view
            S = box((M, K), K + 8, 0, dtype, dev, poison); boxes.append(S)
            kw["ln_scratch"] = S.buf[2 * (K + 8):(2 + M) * (K + 8)]
            outs.append(S.view)
    if c["wq"]:                                       # W once more in fragment order (packing.pack_wq), contiguous, 32 bytes into a poisoned buffer
        wq = PK.pack_wq(d["W"])
        wbuf = flat(wq.numel() + 32, dtype, dev, poison)
        wbuf[16:16 + wq.numel()] = wq.reshape(-1)
        kw["Wq"] = wbuf[16:16 + wq.numel()].view(wq.shape)
    if c["rowstat"]:
        st = flat(c["rowstat"] * M * 2, F32, dev, poison).view(c["rowstat"], M, 2)
        kw["rowstat"] = st; outs.append(st)
    with L.options(**(c["opts"] if opts is None else opts)):
        O.run_ops([O.Gemm(A.view, Wb.view, C.view[..., :nout], epilogue=EPI[c["epi"]], splitk=c["splitk"], ws=ws, **kw)])
        kern = last_kernel()
    torch.cuda.synchronize()
    ok = all(intact(b) for b in boxes) and bool((C.view[..., nout:] == 0).all())
    if c["splitk"] > 1:
        n = T.splitk_plan(K, c["splitk"])[0] * M * N
        ok = ok and bool(torch.isfinite(ws[:n]).all()) and bool(torch.equal(bits(ws[n:]), bits(flat(ws.numel() - n, F32, dev, poison))))
    return [o.clone() for o in outs], ok, kern


def gemm_refs(c, d):
    ref = T.reference(c, d)
    if c["vt"]:
        views, vt_T = c["vt"]
        return [ref[:, :T.VT_FROM], ref[:, T.VT_FROM:].reshape(views, vt_T, -1).transpose(1, 2)]
    if c["ln"] is not None and c["ln"][0] == "scratch":
        return [ref, T._ln64(d["A"].double())]
    return [ref] + ([None] if c["rowstat"] else [])


def residual_bound_of(c, d, dtype):
    """values_data.B_gemm_residual for a plain GEMM with a 16-bit residual, else None."""
    if not (c["R"] and c["epi"] == 0 and not c["c_f32"] and c["ln"] is None and c["splitk"] <= 1):
        return None

    def bound():
        c0 = dict(c, R=False)
        x1 = T.reference(c0, d)
        ab = {k: (v.abs() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
        S = T.reference(c, ab)
        return V.B_gemm_residual(T.reference(c, d).cpu(), S.cpu(), x1.cpu(), c["K"], dtype)
    return bound


GEMM_FAMS = [f for f in T.FAMILIES if f.startswith("gemm_")]


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("family", GEMM_FAMS)
def test_gemm_tails(dev, family, dtype):
    tally = Tally(family, dtype)
    for c in T.cases(family):
        d = to_dev(T.inputs(c, dtype), dev)
        runs = [run_gemm(c, d, dtype, dev, p) for p in POISONS]
        verdict(tally, c, [r[0] for r in runs], gemm_refs(c, d), runs[0][1] and runs[1][1], runs[0][2], residual_bound_of(c, d, dtype))
        if c["rowstat"]:
            C, st = runs[0][0][0], runs[0][0][-1].double().cpu()
            nt = -(-c["N"] // 128) if c["tag"].startswith("gemm_ws") else 1          # rowstat_kernel: part 0 = whole rows, the rest zeros
            want = rowstat_ref(C, [(128 * k, min(c["N"], 128 * k + 128)) for k in range(nt)] if c["tag"].startswith("gemm_ws") else [(0, c["N"])])
            err = float(((st[:nt] - want).abs() / (want.abs() + 1.0)).max()) if bool(torch.isfinite(st).all()) else math.inf
            if not (err < T.ROWSTAT_BOUND and bool((st[nt:] == 0).all())):
                tally.fails.append((T.label(c), f"row statistics: {err:.3e} (bound 2e-5), unused parts zero: {bool((st[nt:] == 0).all())}"))
    tally.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_generic_tiles_64_and_128_give_the_same_bits(dev, dtype):
    """gemm_route.h: "Same k order in every tile: results do not depend on the choice (split-K aside)" — every generic case of the 64 x 64
    and the 128 x 128 sweep without split-K, run on both tiles."""
    seen, diff, n = set(), [], 0
    for c in T.cases("gemm_generic:t64") + T.cases("gemm_generic:t128"):
        key = T.math_key(c)
        if key in seen or c["splitk"] > 1:
            continue
        seen.add(key)
        d = to_dev(T.inputs(c, dtype), dev)
        o = {}
        for r in ("t64", "t128"):
            o[r], _, kern = run_gemm(c, d, dtype, dev, NAN, opts=dict(GEMM_WS=0, GEMM_XL=0, **T.GENERIC_TILES[r][3]))
            BM = T.GENERIC_TILES[r][0]
            assert kern.startswith("gemm_conv_kernel<%d,%d," % (BM, 128 if c["epi"] == 1 else BM)), kern
        if not torch.equal(bits(o["t64"][0]), bits(o["t128"][0])):
            diff.append((T.label(c), int((bits(o["t64"][0]) != bits(o["t128"][0])).sum())))
        n += 1
    parity_log(f"tails:generic_tiles_bit_identity:{KIND[dtype]}", cases=n, differing=len(diff))
    assert n > 60 and not diff, diff[:12]


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("walk", [0, 1, 2, 3], ids=["2cus", "2cus+1", "3cus-1", "3cus+1"])
@pytest.mark.parametrize("form", ["xlp", "xd"])
def test_xl_persistent_walk_tails(dev, form, walk, dtype):
    """The persistent forms of the 256 x 256 XL GEMM (tails_data.xlp_cases: one workgroup per CU walks 2 CUs, 2 CUs + 1, 3 CUs - 1, 3 CUs + 1
    real tiles, a ragged last M tile, two N tiles in the first case, with and without a residual; the W-direct form with Wq and K = 640).
    The assertions of every other GEMM case — tag, close() of the WHOLE C against fp64, finite, borders, the same bits under both poisons —
    and the same bits from the non-persistent kernel."""
    c = T.xlp_cases(form, L.device_info()["cus"])[walk]
    tally = Tally(f"gemm_xl:{form}:{walk}", dtype)
    d = to_dev(T.inputs(c, dtype), dev)
    runs = [run_gemm(c, d, dtype, dev, p) for p in POISONS]
    verdict(tally, c, [r[0] for r in runs], gemm_refs(c, d), runs[0][1] and runs[1][1], runs[0][2], residual_bound_of(c, d, dtype))
    plain, ok, kern = run_gemm(c, d, dtype, dev, NAN, opts=dict(c["opts"], XL_PERSIST=0))
    if kern != "gemm_xl_kernel<256x256,gemm>" or not ok:
        tally.fails.append((T.label(c), "non-persistent run", kern, ok))
    if not torch.equal(bits(plain[0]), bits(runs[0][0][0])):
        tally.fails.append((T.label(c), "persistent and non-persistent kernels differ", int((bits(plain[0]) != bits(runs[0][0][0])).sum())))
    tally.done()


# --------------------------------------------------------------------------------------------------------------------------------------
# implicit-GEMM conv
# --------------------------------------------------------------------------------------------------------------------------------------
def run_conv(c, d, dtype, dev, poison):
    B, Cin, Cout = c["B"], c["Cin"], c["Cout"]
    X = box((B, c["Hi"], c["Wi"], Cin), Cin + 8, 0, dtype, dev, poison, fill=d["x"])
    Y = box((B, c["Ho"], c["Wo"], Cout), T.ldc_of(c), 0, dtype, dev, poison)
    boxes = [Y]
    kw = dict(bias=side_of(d["bias"], 4, dev, poison))
    if c["R"]:
        R = box((B, c["Ho"], c["Wo"], Cout), T.ldc_of(c), 0, dtype, dev, poison, fill=d["R"]); boxes.append(R); kw["R"] = R.view
    if c["temb"]:
        tbs = Cout + 4
        tb = flat(B * tbs + 8, F32, dev, poison)
        tb[4:4 + B * tbs].view(B, tbs)[:, :Cout] = d["temb"]
        kw.update(temb=tb[4:], temb_b_stride=tbs)
    ws = flat(T.WS_BYTES // 4, F32, dev, poison)
    with L.options(**c["opts"]):
        O.run_ops([O.Conv(X.view, d["w"].contiguous(), Y.view, stride=(c["stride"],) * 2, pad=c["pad"], pad_end=c["pad_end"], splitk=c["splitk"], ws=ws,
                          epilogue=EPI[c["epi"]], direct=c["kind"] == "conv_direct", **kw)])
        kern = last_kernel()
    torch.cuda.synchronize()
    return [Y.view.clone()], all(intact(b) for b in boxes), kern


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("family", [f for f in T.FAMILIES if f.startswith("conv")])
def test_conv_tails(dev, family, dtype):
    tally = Tally(family, dtype)
    for c in T.cases(family):
        d = to_dev(T.inputs(c, dtype), dev)
        runs = [run_conv(c, d, dtype, dev, p) for p in POISONS]
        verdict(tally, c, [r[0] for r in runs], [T.reference(c, d)], runs[0][1] and runs[1][1], runs[0][2])
    tally.done()


# --------------------------------------------------------------------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------------------------------------------------------------------
def run_attn(c, d, dtype, dev, poison):
    B, H, Tq, Tk, dd, Bkv = c["B"], c["H"], c["Tq"], c["Tk"], c["d"], c["Bkv"]
    Cc = H * dd
    Ob = box((B, Tq, Cc), Cc + 12, 4, dtype, dev, poison)               # 8-byte aligned, ldo % 8 == 4
    if c["rowmajor"]:                                                    # Q | K | V as the column blocks of one buffer, rows past Tq / Tk poisoned
        Tm = max(Tq, Tk) + 2
        buf = box((B, Tm, 3 * Cc), 3 * Cc + 8, 0, dtype, dev, poison).view
        buf.fill_(poison)
        buf[:, :Tq, :Cc] = d["q"]; buf[:, :Tk, Cc:2 * Cc] = d["k"]; buf[:, :Tk, 2 * Cc:] = d["v"]
        Q, K, Vv = buf[:, :Tq, :Cc], buf[:, :Tk, Cc:2 * Cc], buf[:, :Tk, 2 * Cc:]
    else:
        Q = box((B, Tq, Cc), Cc + 8, 0, dtype, dev, poison, fill=d["q"]).view
        Kb = box((Bkv, Tk + 2, Cc), Cc + 8, 0, dtype, dev, poison).view  # two poisoned rows past Tk in EVERY kv batch
        Kb.fill_(poison); Kb[:, :Tk] = d["k"]
        K = Kb[:, :Tk]
        Vv = box((Bkv, Cc, Tk), T.roundup(Tk, 8) + c["ldv_extra"], 0, dtype, dev, poison, fill=d["v"].transpose(1, 2)).view
    kw = {}
    if c["kvmap"] is not None:
        kw.update(kvmap=torch.tensor([j for r in c["kvmap"] for j in r], dtype=torch.int32, device=dev), nsrc=c["nsrc"], joint=c["joint"])
    with L.options(**c["opts"]):
        O.run_ops([O.Attn(Q, K, Vv, Ob.view, heads=H, Tk=Tk, scale=dd ** -0.5, q_prescaled=c["pre"], causal=c["causal"], v_rowmajor=c["rowmajor"], **kw)])
        kern = last_kernel()
    torch.cuda.synchronize()
    return [Ob.view.clone()], intact(Ob), kern


ATTN_FAMS = [f for f in T.FAMILIES if f.startswith("attn")]


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("family", ATTN_FAMS)
def test_attention_tails(dev, family, dtype):
    tally = Tally(family, dtype)
    for c in T.cases(family):
        d = to_dev(T.inputs(c, dtype), dev)
        runs = [run_attn(c, d, dtype, dev, p) for p in POISONS]
        verdict(tally, c, [r[0] for r in runs], [T.reference(c, d)], runs[0][1] and runs[1][1], runs[0][2])
    tally.done()


# --------------------------------------------------------------------------------------------------------------------------------------
# norms, softmax, element-wise
# --------------------------------------------------------------------------------------------------------------------------------------
def run_norm(c, d, dtype, dev, poison):
    k = c["kind"]
    if k == "softmax":
        rows, Tn, ldy = c["rows"], c["T"], c["ldy"]
        X = box((rows, Tn), Tn + 3, 0, F32, dev, poison, fill=d["x"])
        Yb = box((rows, ldy), ldy, 0, dtype, dev, poison)                # dense rows; the columns T..ldy belong to the op (written as zeros)
        O.run_ops([O.Softmax(X.view, Yb.view, Tn, d["scale"])])
        kern = last_kernel()
        torch.cuda.synchronize()
        return [Yb.view[:, :Tn].clone()], intact(Yb) and bool((Yb.view[:, Tn:] == 0).all()), kern
    gamma, beta = side_of(d["gamma"], 4, dev, poison), side_of(d["beta"], 4, dev, poison)
    if k == "layernorm":
        M, Cc = c["M"], c["C"]
        X = box((M, Cc), Cc + c["ldx_extra"], 0, dtype, dev, poison, fill=d["x"])
        Y = box((M, Cc), Cc + 8, 0, dtype, dev, poison)
        O.run_ops([O.LayerNorm(X.view, Y.view, gamma, beta, 1e-5)])
    else:
        B, HW, Cc = c["B"], c["HW"], c["C"]
        ld = T.roundup(Cc, 8) + 8                                        # 16-byte rows: the channels per group alone decide the vector width
        X = box((B, HW, Cc), ld, 0, dtype, dev, poison, fill=d["x"])
        Y = box((B, HW, Cc), ld, 0, dtype, dev, poison)
        ws = flat(1 << 16, F32, dev, poison) if c.get("ws") else None    # the two-stage path's partials: what the workspace held must not matter
        with L.options(**c["opts"]):
            O.run_ops([O.GroupNorm(X.view, Y.view, gamma, beta, c["G"], 1e-5, silu=bool(c["silu"]), ws=ws)])
    kern = last_kernel()
    torch.cuda.synchronize()
    return [Y.view.clone()], intact(Y), kern


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("family", ["groupnorm", "groupnorm2", "layernorm", "softmax"])
def test_norm_tails(dev, family, dtype):
    tally = Tally(family, dtype)
    for c in T.cases(family):
        d = to_dev(T.inputs(c, dtype), dev)
        runs = [run_norm(c, d, dtype, dev, p) for p in POISONS]
        verdict(tally, c, [r[0] for r in runs], [T.reference(c, d)], runs[0][1] and runs[1][1], runs[0][2])
    tally.done()


EW_CODE = dict(ADD=L.EW_ADD, COPY=L.EW_COPY, SILU=L.EW_SILU, SCALE=L.EW_SCALE)


def run_ew(c, d, dtype, dev, poison):
    k = c["kind"]
    if k == "ew":
        M, Cc = c["M"], c["C"]
        ld, off = (Cc + 8, 0) if c["vec"] else (Cc + 3, 1)
        X = box((M, Cc), ld, off, dtype, dev, poison, fill=d["x"])
        Y = box((M, Cc), ld, off, dtype, dev, poison, fill=d["y0"] if c["op"] == "ADD" else None)
        O.run_ops([O.Ew(EW_CODE[c["op"]], X.view, Y.view, alpha=d["alpha"])])
        kern = last_kernel()
        torch.cuda.synchronize()
        return [Y.view.clone()], intact(Y), kern
    if k == "upsample":
        B, Cc = c["B"], c["C"]
        ld = Cc + 8 if Cc % 8 == 0 else Cc + 3
        X = box((B, c["Hi"], c["Wi"], Cc), ld, 0, dtype, dev, poison, fill=d["x"])
        Y = box((B, c["Ho"], c["Wo"], Cc), ld, 0, dtype, dev, poison)
        O.run_ops([O.Upsample(X.view, Y.view, PK.nearest_index(c["Hi"], c["Ho"]).to(dev), PK.nearest_index(c["Wi"], c["Wo"]).to(dev))])
        kern = last_kernel()
        torch.cuda.synchronize()
        return [Y.view.clone()], intact(Y), kern
    B, Cc, H, W = c["B"], c["C"], c["H"], c["W"]                        # NCHW -> NHWC into a guarded view, and back
    Y = box((B, H, W, Cc), Cc + 3, 1, dtype, dev, poison)
    O.run_ops([O.Layout(d["x"].contiguous(), Y.view, True)])
    kern = last_kernel()
    back = torch.full((B, Cc, H, W), NAN, dtype=dtype, device=dev)
    O.run_ops([O.Layout(Y.view, back, False)])
    torch.cuda.synchronize()
    return [Y.view.clone(), back], intact(Y) and torch.equal(bits(back), bits(d["x"])), kern


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("family", ["elementwise", "layout"])
def test_elementwise_tails(dev, family, dtype):
    tally = Tally(family, dtype)
    for c in T.cases(family):
        d = to_dev(T.inputs(c, dtype), dev)
        runs = [run_ew(c, d, dtype, dev, p) for p in POISONS]
        refs = [T.reference(c, d)] + ([None] if c["kind"] == "layout" else [])
        verdict(tally, c, [r[0] for r in runs], refs, runs[0][1] and runs[1][1], runs[0][2])
    tally.done()


# --------------------------------------------------------------------------------------------------------------------------------------
# Fourier embedding, gather, timestep embedding, the DDIM step
# --------------------------------------------------------------------------------------------------------------------------------------
def seg(vals, dev, poison, dtype=None):
    """A 1-D operand 8 elements into a larger poisoned buffer (a box of one row)."""
    v = vals.reshape(1, -1)
    return box(tuple(v.shape), v.shape[1] + 16, 8, dtype or vals.dtype, dev, poison, fill=v)


def run_misc(c, d, dtype, dev, poison):
    """-> (outputs, borders intact, kernel, {output index: (fp64 reference, absolute bound)} for the outputs held to an existing absolute bound)."""
    k = c["kind"]
    if k == "fourier":
        width = c["P"] * (3 + 6 * c["F"])
        Y = box((c["n"], width), width + 5, 1, dtype, dev, poison)
        O.run_ops([O.Fourier(d["x"].contiguous(), Y.view, c["F"], mask=d["mask"], null_feat=d["null"])])
        kern = last_kernel()
        torch.cuda.synchronize()
        return [Y.view.clone()], intact(Y), kern, {}
    if k == "gather":
        Cc = c["C"]
        Tb = box((10, Cc), Cc + 8, 0, dtype, dev, poison, fill=d["table"])
        Y = box((c["n"], Cc), Cc + 8, 0, dtype, dev, poison)
        add = box((3, Cc), Cc + 8, 0, dtype, dev, poison, fill=d["add"]).view if c["add"] else None
        O.run_ops([O.Gather(Tb.view, Y.view, d["idx"], add=add)])
        kern = last_kernel()
        torch.cuda.synchronize()
        return [Y.view.clone()], intact(Y), kern, {}
    if k == "timeemb":
        Y = box((c["n"], c["dim"]), c["dim"] + 4, 0, F32, dev, poison)
        O.run_ops([O.TimeEmb(d["t"], Y.view)])
        kern = last_kernel()
        torch.cuda.synchronize()
        return [Y.view.clone()], intact(Y), kern, {0: T.ABS_BOUND["timeemb"]}      # the absolute bound of test_fourier_gather_timeemb
    n, cf = c["n"], 2 if c["cfg"] else 1
    X = seg(d["x"], dev, poison)
    eps = seg(d["eps"], dev, poison)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    kw, boxes = {}, [X]
    if c["xin_ld"]:
        px = cf * n // T.DDIM_C
        Xin = box((px, c["xin_ld"]), c["xin_ld"], 0, dtype, dev, poison)     # dense rows: the pad columns 4.. belong to the caller and stay NaN
        kw.update(x_in=Xin.view, xin_c=T.DDIM_C)
    else:
        Xin = box((1, cf * n), cf * n + 16, 8, F32, dev, poison)
        kw.update(x_in=Xin.view[0])
    boxes.append(Xin)
    if c["gv"]:
        kw.update(gv_mask=d["mask"], gv_cond=seg(d["cond"], dev, poison).view[0], gv_noise=seg(d["noise"], dev, poison).view[0], gv_mode=c["gv"], gv_last_step=1)
    O.run_ops([O.DdimStep(X.view[0], eps.view[0], d["coef"], step, cfg=bool(c["cfg"]), guidance=d["guidance"], **kw)])
    kern = last_kernel()
    torch.cuda.synchronize()
    xn = X.view[0]
    if c["xin_ld"]:
        want = xn.view(-1, T.DDIM_C).to(dtype).repeat(cf, 1)
        ok = torch.equal(bits(Xin.view[:, :T.DDIM_C]), bits(want)) and bool(torch.isnan(Xin.view[:, T.DDIM_C:].float()).all())
    else:
        ok = torch.equal(bits(Xin.view[0]), bits(xn.repeat(cf)))
    return [X.view.clone()], all(intact(b) for b in boxes) and ok and int(step) == 1, kern, {0: T.ABS_BOUND["ddim"]}      # atol of test_cfg_ddim_and_graph_replay


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_misc_tails(dev, dtype):
    """Fourier features at F = 0 / 1 / 16, gather (with and without the periodic addend), timestep embedding at n = 1 / 63 / 65; the DDIM step at
    n = 1 .. 1025 with a flat fp32 and a padded 16-bit model-input copy and both given-view modes.  16-bit outputs: close(), the Fourier features
    also within values_data.fourier_ref's bound; fp32 outputs: the absolute bounds the existing tests of these kernels use."""
    tally = Tally("misc", dtype)
    for c in T.cases("misc"):
        d = to_dev(T.inputs(c, dtype), dev)
        runs = [run_misc(c, d, dtype, dev, p) for p in POISONS]
        ref = T.reference(c, d)
        absb = runs[0][3]
        verdict(tally, c, [r[0] for r in runs], [None if absb else ref], runs[0][1] and runs[1][1], runs[0][2])
        out = runs[0][0][0]
        if absb:
            err = float((out.double() - ref).abs().max()) if bool(torch.isfinite(out).all()) else math.inf
            if not err < absb[0]:
                tally.fails.append((T.label(c), f"max abs error {err:.3e} >= {absb[0]:.0e}"))
        if c["kind"] == "fourier":
            r64, bound = V.fourier_ref(d["x"].cpu(), c["F"], dtype)
            live = d["mask"].cpu().bool()
            w = V.ratio(out.cpu()[live], r64[live], bound[live]) if bool(live.any()) else 0.0
            if not w <= 1.0:
                tally.fails.append((T.label(c), f"fourier: worst err / bound {w:.3f}"))
    tally.done()


UNIPC_CASES = [(px, (4, 8)[i % 2], 0) for i, px in enumerate(T.DDIM_N)] + [(257, 8, 1), (257, 4, 2)]       # (pixels, x_in pitch, given-view mode)


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
def test_unipc_step_tails(dev, dtype):
    """The fused CFG + UniPC step at n / 4 in {1, 3, 255, 256, 257, 1025} pixels of 4 channels with the padded 16-bit model-input copy (pitch 4 and
    8), and both given-view modes on 4 views of 257 elements: three steps (warm-up, order 2 twice) against oracle.denoiser.UniPC with the same
    eps, at the tolerance of test_cfg_unipc_matches_oracle_scheduler (3e-5 max|x| + 1e-5 |x|).  Given views (mask 0 1 0 1): mode 2 feeds the
    oracle the initial noise as their prediction; mode 1 re-noises them after every step before gv_last_step = 2 with the scheduler's
    add_noise at the next timestep.  Every buffer sits inside a poisoned buffer whose border must stay bit-intact, and the result must not
    depend on the poison.  Logged: the worst |x - oracle| / bound over all steps."""
    from magicdrive_amd import schedulers
    from oracle import denoiser as D
    fails, worst, n_cases = [], 0.0, 0
    for px, ld, gv in UNIPC_CASES:
        n = T.DDIM_C * px
        finals = []
        g = torch.tensor([0, 1, 0, 1], dtype=torch.uint8)
        gmask = g.bool().repeat_interleave(n // 4) if gv else None
        cond, noise = T.randn(n, seed=3).float(), T.randn(n, seed=4).float()
        for poison in POISONS:
            sch = schedulers.UniPCMultistepScheduler(); ts = sch.set_timesteps(8)
            o = D.UniPC(); o.set_timesteps(8)
            x0 = T.randn(n, seed=1).float()
            X = seg(x0, dev, poison); xo = x0.clone()
            eps = seg(torch.zeros(2 * n), dev, poison)
            state = [seg(torch.zeros(n), dev, poison) for _ in range(3)]
            Xin = box((2 * px, ld), ld, 0, dtype, dev, poison)
            step = torch.zeros(1, dtype=torch.int32, device=dev)
            kw = dict(gv_mask=g.to(dev), gv_cond=seg(cond, dev, poison).view[0], gv_noise=seg(noise, dev, poison).view[0], gv_mode=gv, gv_last_step=2) if gv else {}
            op = O.UniPCStep(X.view[0], eps.view[0], sch.coefficient_table().to(dev), step, *[b.view[0] for b in state], x_in=Xin.view, cfg=True,
                             guidance=2.0, xin_c=T.DDIM_C, **kw)
            tl = ts.tolist()
            for k_, t in enumerate(tl[:3]):
                e = T.randn(2 * n, seed=100 + k_).float()
                eps.view[0].copy_(e)
                O.run_ops([op])
                kern = last_kernel()
                torch.cuda.synchronize()
                ec = e[:n] + 2.0 * (e[n:] - e[:n])
                if gv == 2:
                    ec = torch.where(gmask, noise, ec)
                xo = o.step(ec, t, xo)
                if gv == 1 and k_ < 2:
                    xo = torch.where(gmask, sch.add_noise(cond, noise, tl[k_ + 1]), xo)
                got = X.view[0].cpu()
                ratio = float(((got - xo).abs() / (3e-5 * float(xo.abs().max()) + 1e-5 * xo.abs())).max()) if bool(torch.isfinite(got).all()) else math.inf
                worst = max(worst, ratio)
                if kern != "unipc_kernel" or not ratio <= 1.0:
                    fails.append((px, ld, gv, k_, kern, ratio))
            want = X.view[0].view(px, T.DDIM_C).to(dtype).repeat(2, 1)
            if not (all(intact(b) for b in [X, eps, Xin] + state) and torch.equal(bits(Xin.view[:, :T.DDIM_C]), bits(want))
                    and bool(torch.isnan(Xin.view[:, T.DDIM_C:].float()).all()) and int(step) == 3):
                fails.append((px, ld, gv, "border, pad columns or model-input copy"))
            finals.append(X.view.clone())
        if not torch.equal(bits(finals[0]), bits(finals[1])):
            fails.append((px, ld, gv, "result depends on what lies outside the extents"))
        n_cases += 1
    parity_log(f"tails:unipc:{KIND[dtype]}", cases=n_cases, worst_err_over_bound=worst, failures=len(fails))
    assert not fails, fails[:10]
