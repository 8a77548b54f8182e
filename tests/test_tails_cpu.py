"""CPU: the tile-tail cases of tests/tails_data.py are what they claim to be.

    coverage      cases(family) hits every cell of cells(family), for every family
    route         every GEMM / conv case resolves (csrc/gemm_route.h through tests/gemm_route_check.cpp, the harness of test_gemm_route.py)
                  to the kernel tag it claims; a case a main loop declines claims the fallback it really gets
    sensitivity   for every case and both storage types the fp64 reference rounded once passes helpers.close() and every applicable mutant
                  (one tail error each) fails it; the exemptions are tails_data.EXEMPTIONS, by rule
    references    at the tiniest case of each family the fp64 reference equals a literal Python-loop evaluation to 1e-12
"""
import math
import os

import pytest
import torch

import gemm_route_table as G
import helpers
import tails_data as T
import values_data as V

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [torch.bfloat16, torch.float16]
KIND = {torch.bfloat16: "bf16", torch.float16: "f16"}
FAMS = list(T.FAMILIES)


@pytest.mark.parametrize("family", FAMS)
def test_cases_hit_every_cell(family):
    want = set(T.cells(family))
    got = set()
    for c in T.cases(family):
        got |= T.hits(family, c)
    assert want and not (want - got), (family, sorted(want - got, key=str))


def test_edges_and_constants():
    assert T.edges(64) == [1, 63, 64, 65, 127, 128, 129]
    assert T.edges(128, 4) == [4, 124, 128, 132, 252, 256, 260]
    assert T.edges(1) == [1, 2, 3]
    csrc = os.path.join(os.path.dirname(HERE), "magicdrive_amd", "csrc")
    for key, (value, cite, text) in T.CONSTANTS.items():            # every citation is read back: the text stands on the cited lines
        fname, span = cite.split(":")
        lo, hi = (int(v) for v in (span.split("-") if "-" in span else (span, span)))
        lines = open(os.path.join(csrc, fname)).read().splitlines()
        assert text in "\n".join(lines[lo - 1:hi]), (key, cite, text)
    # the constants that are plain numbers in the sources, read back from the cited lines
    src = lambda f: open(os.path.join(csrc, f)).read()
    assert "constexpr int BM = 128, BN = 128, BK = 64, KS = 20, NSLAB = 5;" in src("gemm_ws.hip")
    assert "constexpr int ROWS_PASS = GEGLU ? 128 : 64;" in src("gemm_ws.hip")
    assert "constexpr int BM = 256, NTH = 512;" in src("gemm_xl.hip")
    assert "constexpr int KVT = 64;" in src("attention.hip")
    assert "constexpr int A2_KV = 64, A2_NW = 4, A2_NT = 256, A2_NBUF = A2_RING;" in src("attention2.hip") and "#define A2_RING 3" in src("attention2.hip")
    assert "constexpr int SHORT_T = 128;" in src("attention_short.hip")
    assert "constexpr int XL_SLOTS = 12;" in src("gemm_route.h")
    assert "if (p.Tq < 256 || (long)((p.Tq + 127) / 128) * p.H * p.B < 128) return false;" in src("attn_route.h")


# --------------------------------------------------------------------------------------------------------------------------------------
# route
# --------------------------------------------------------------------------------------------------------------------------------------
ROUTED = [(f, i, c) for f in FAMS for i, c in enumerate(T.cases(f)) if c["kind"] in ("gemm", "conv")]


XLP = [(f"xlp:{form}#{i}", c) for form in ("xlp", "xd") for i, c in enumerate(T.xlp_cases(form, 256))]


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """gemm_route_table.evaluate: the harness of test_gemm_route.py."""
    lines = [f"{f}#{i} {T.route_line(c)}" for f, i, c in ROUTED] + [f"{name} {T.route_line(c)}" for name, c in XLP]
    out = G.evaluate(lines, tmp_path_factory.mktemp("route"))
    if out is None:
        pytest.skip("no g++")
    return out


def test_persistent_xl_cases_reach_the_256_wide_xl_route(routes):
    """The persistent / W-direct form is picked inside launch_xl (it depends on the CU count): the route function must hand these cases to the
    256-wide XL main loop, and each has the tile count it names, in whole tiles, with a ragged last M tile."""
    for name, c in XLP:
        r = routes[name]
        assert r["err"] == "0" and r["main"] == "gemm_xl_kernel<256x256,gemm>", (T.label(c), r)
        assert -(-c["M"] // 256) * -(-c["N"] // 256) == c["nblk"] and c["M"] % 256 and c["N"] % 8 == 0, T.label(c)


@pytest.mark.parametrize("family", sorted({f for f, _, _ in ROUTED}))
def test_claimed_kernel_is_what_the_route_function_picks(routes, family):
    n = 0
    for f, i, c in ROUTED:
        if f != family:
            continue
        r = routes[f"{f}#{i}"]
        assert r["err"] == "0", (T.label(c), r)
        want = c["tag"]
        if c["kind"] == "gemm" and c["vt"]:
            # the fused V^T output goes straight to launch_gemm_ws (gemm_conv.hip: mdx_gemm_bf16) once ws_supported holds: the route function,
            # asked about the same problem without Vt under GEMM_WS = 2, must name the weight-stationary kernel
            want = "gemm_ws_kernel<plain>"
        assert r["last"] == want, (T.label(c), r["last"], want)
        if c["splitk"] > 1:
            assert (int(r["splitk"]), int(r["kchunk"])) == T.splitk_plan(c["K"], c["splitk"]), (T.label(c), r)
        if c["kind"] == "gemm" and c["rowstat"]:
            fused = c["tag"].startswith("gemm_ws")
            assert (r["rowstat_after"], r["keep_rowstat"]) == (("0", "1") if fused else ("1", "0")), r
        if c["kind"] == "gemm" and c["ln"]:
            fused = c["ln"][0] != "scratch"
            assert (r["normalise_first"], r["keep_ln"]) == (("0", "1") if fused else ("1", "0")), r
        n += 1
    assert n


def test_xl_slot_table_boundary():
    """256 / rows_per_b + 2 <= XL_SLOTS: 25 and 24 rows per image are served, 23 is the first width the XL kernel declines."""
    slots = T.const("gemm_xl.XL_SLOTS")
    assert 256 // 25 + 2 <= slots and 256 // 24 + 2 <= slots and 256 // T.XL_TEMB_DECLINED + 2 > slots


# --------------------------------------------------------------------------------------------------------------------------------------
# sensitivity
# --------------------------------------------------------------------------------------------------------------------------------------
def _passes(out, ref, kind):
    try:
        helpers.close(out, ref, kind=kind, name="tails-cpu")
    except AssertionError:
        return False
    return True


@pytest.fixture(autouse=True)
def _no_parity_log(monkeypatch):
    monkeypatch.setattr(helpers, "parity_log", lambda *a, **k: None)


_VERDICTS = {}


@pytest.mark.parametrize("dtype", DTYPES, ids=KIND.values())
@pytest.mark.parametrize("family", FAMS)
def test_honest_rounding_passes_and_every_mutant_fails(family, dtype):
    undetected, refused = [], []
    n_mut = 0
    for c in T.cases(family):
        key = (T.math_key(c), dtype)
        if key not in _VERDICTS:                     # cases that differ only in their route share one reference
            d = T.inputs(c, dtype)
            ref = T.reference(c, d)
            assert torch.isfinite(ref).all(), T.label(c)
            if c["kind"] in T.ABS_BOUND:           # fp32 outputs: the absolute bound the GPU test holds them to
                ok = lambda out: float((out.double() - ref).abs().max()) < T.ABS_BOUND[c["kind"]]
            else:
                ok = lambda out: _passes(out, ref, KIND[dtype])
            _VERDICTS[key] = (ok(ref.to(T.store_dtype(c, dtype))), {name: ok(m) for name, m in T.mutants(c, d, dtype).items()})
        honest, muts = _VERDICTS[key]
        if not honest:
            refused.append(T.label(c))
        n_mut += len(muts)
        undetected += [(T.label(c), name) for name, passed in muts.items() if passed]
    assert not refused, ("the honest reference, rounded once, is refused", refused[:10])
    assert not undetected, (len(undetected), undetected[:20])
    assert n_mut > 0


def test_mutant_applicability_is_by_rule_only():
    """Every (case, mutant) pair left out of the sensitivity test falls under one of tails_data.EXEMPTIONS, restated here from the case's numbers."""
    for f in FAMS:
        for c in T.cases(f):
            for m in T.MUTANTS[c["kind"]]:
                if T.applicable(c, m):
                    continue
                k = c["kind"]
                if k in ("gemm", "conv", "conv_direct"):
                    ok = ((m == "drop_last_row" and c["M"] == 1) or (m == "last_cols_from_previous" and T.out_cols(c) == 1)
                          or (m == "bias_shifted_by_4" and (not c["bias"] or c["N"] == 1))
                          or (m == "temb_row_of_previous_image" and (not c["temb"] or (c["M"] <= c["temb"] if k == "gemm" else c["B"] == 1))))
                elif k == "attn":
                    one_key = c["Tk"] == 1 and (not c["joint"] or max(sum(j >= 0 for j in r) for r in c["kvmap"]) <= 1)
                    ok = ((m == "drop_last_key" and one_key) or (m == "causal_off_by_one" and (not c["causal"] or c["Tq"] == 1))
                          or (m == "last_query_from_previous" and (c["Tq"] == 1 or (one_key and not c["causal"]))))
                elif k in ("groupnorm", "layernorm", "softmax"):
                    ok = m in ("count_one_less", "drop_last_element") and T._norm_n(c) == 1
                else:
                    ok = m == "last_element_from_previous" and T.reference(c, T.inputs(c, torch.bfloat16)).numel() == 1
                assert ok, (T.label(c), m)


# --------------------------------------------------------------------------------------------------------------------------------------
# the references against literal loops
# --------------------------------------------------------------------------------------------------------------------------------------
def _close12(a, b):
    return float((a.double() - b.double()).abs().max()) <= 1e-12 * max(1.0, float(b.double().abs().max()))


def test_gemm_reference_against_loops_and_values_data():
    dt = torch.bfloat16
    c = T.gemm_case(5, 4, 16, {}, "", bias=True, R=True, temb=2)
    d = T.inputs(c, dt)
    ref = T.reference(c, d)
    for m in range(5):
        for n in range(4):
            acc = 0.0
            for k in range(16):
                acc += float(d["A"][m, k]) * float(d["W"][n, k])
            acc += float(d["bias"][n]) + float(d["temb"][m // 2, n]) + float(d["R"][m, n])
            assert abs(acc - float(ref[m, n])) <= 1e-12 * max(1.0, abs(acc))
    c = T.gemm_case(6, 64, 16, {}, "", bias=True, epi=1)                     # GEGLU: value half x gelu(gate half), exact erf
    d = T.inputs(c, dt)
    ref = T.reference(c, d)
    for m in (0, 5):
        for n in (0, 31):
            h = sum(float(d["A"][m, k]) * float(d["W"][n, k]) for k in range(16)) + float(d["bias"][n])
            g = sum(float(d["A"][m, k]) * float(d["W"][32 + n, k]) for k in range(16)) + float(d["bias"][32 + n])
            want = h * 0.5 * g * (1.0 + math.erf(g / math.sqrt(2.0)))
            assert abs(want - float(ref[m, n])) <= 1e-12 * max(1.0, abs(want))
    c = T.gemm_case(37, 68, 72, {}, "", bias=True, R=True)                   # the shared reference of the value-range tests agrees
    d = T.inputs(c, dt)
    assert _close12(T.reference(c, d), V.gemm_ref(d, True, True)[0])


def test_conv_reference_against_loops_stride2_asymmetric_pad():
    dt = torch.float16
    c = T.conv_case(2, 4, 5, 8, 3, 3, 2, (0, 0), {}, "", pad_end=(1, 1), temb=3, R=True)
    d = T.inputs(c, dt)
    ref = T.reference(c, d)
    assert ref.shape == (2, c["Ho"], c["Wo"], 3) and (c["Ho"], c["Wo"]) == (2, 2)
    for b in range(2):
        for oy in range(c["Ho"]):
            for ox in range(c["Wo"]):
                for co in range(3):
                    acc = 0.0
                    for ky in range(3):
                        for kx in range(3):
                            iy, ix = oy * 2 + ky, ox * 2 + kx
                            if iy < 4 and ix < 5:
                                for ci in range(8):
                                    acc += float(d["x"][b, iy, ix, ci]) * float(d["w"][co, ky, kx, ci])
                    acc += float(d["bias"][co]) + float(d["temb"][b, co]) + float(d["R"][b, oy, ox, co])
                    assert abs(acc - float(ref[b, oy, ox, co])) <= 1e-12 * max(1.0, abs(acc))
    c = T.conv_case(1, 5, 7, 8, 4, 3, 1, (1, 1), {}, "", bias=False)         # values_data.conv_ref is the 3x3 / stride 1 / pad 1 case
    d = T.inputs(c, dt)
    assert _close12(T.reference(c, d), V.conv_ref(d)[0])


def _loop_attention(q, ks, vs, H, scale, causal=False):
    """One softmax over the keys of `ks` (a list of [Tk, C] sources, concatenated) per head, literally."""
    Tq, C = q.shape
    dd = C // H
    k = [row for s in ks for row in s.tolist()]; v = [row for s in vs for row in s.tolist()]
    out = torch.zeros(Tq, C, dtype=torch.float64)
    for t in range(Tq):
        for h in range(H):
            n = min(len(k), t + 1) if causal else len(k)
            logit = [sum(float(q[t, h * dd + i]) * k[j][h * dd + i] for i in range(dd)) * scale for j in range(n)]
            mx = max(logit)
            e = [math.exp(x - mx) for x in logit]
            for i in range(dd):
                out[t, h * dd + i] = sum(e[j] * v[j][h * dd + i] for j in range(n)) / sum(e)
    return out


def test_attention_reference_against_loops_joint_add_causal():
    dt = torch.bfloat16
    joint = T.attn_case(2, 2, 3, 5, 8, {}, "", nsrc=3, joint=True, kvmap=[[0, 1, 2], [2, 3, 0]], Bkv=4)
    add = T.attn_case(3, 2, 3, 5, 8, {}, "", nsrc=2, kvmap=[[1, 2], [-1, 0], [-1, -1]])
    causal = T.attn_case(1, 2, 4, 4, 8, {}, "", causal=True, rowmajor=True)
    for c in (joint, add, causal):
        d = T.inputs(c, dt)
        ref = T.reference(c, d)
        q, k, v = d["q"].double(), d["k"].double(), d["v"].double()
        for b in range(c["B"]):
            js = [j for j in T.attn_sources(c)(b) if j >= 0]
            if c["joint"]:
                want = _loop_attention(q[b], [k[j] for j in js], [v[j] for j in js], 2, 8 ** -0.5)
            else:
                want = sum((_loop_attention(q[b], [k[j]], [v[j]], 2, 8 ** -0.5, c["causal"]) for j in js), torch.zeros(c["Tq"], 16, dtype=torch.float64))
            assert _close12(ref[b], want), (T.label(c), b)
    # and against the shared references of the value-range tests
    c = T.attn_case(1, 2, 17, 33, 16, {}, "")
    d = T.inputs(c, dt)
    assert _close12(T.reference(c, d), V.attn_ref(d["q"], d["k"], d["v"], 2, 0.25, dt)[0])
    d = T.inputs(joint, dt)
    assert _close12(T.reference(joint, d), V.attn_ref_sources(d["q"], d["k"], d["v"], 2, 8 ** -0.5, dt, T.attn_sources(joint), True)[0])
    d = T.inputs(causal, dt)
    assert _close12(T.reference(causal, d), V.attn_ref(d["q"], d["k"], d["v"], 2, 8 ** -0.5, dt, causal=True)[0])
    # the common logit offset is -6 and leaves the softmax alone
    a = float(torch.tensor(T.attn_offset(16)).to(dt))
    assert abs(a * a * 0.25 - 6.0) < 0.05


def test_norm_and_softmax_references_against_loops():
    dt = torch.float16
    c = dict(kind="groupnorm", B=1, HW=3, C=4, G=2, silu=1, opts={}, tag="")
    d = T.inputs(c, dt)
    ref = T.reference(c, d)
    x = d["x"].double()
    for g in range(2):
        vals = [float(x[0, p, g * 2 + j]) for p in range(3) for j in range(2)]
        mean = sum(vals) / 6; var = sum((t - mean) ** 2 for t in vals) / 6
        for p in range(3):
            for j in range(2):
                ch = g * 2 + j
                y = (float(x[0, p, ch]) - mean) / math.sqrt(var + 1e-5) * float(d["gamma"][ch]) + float(d["beta"][ch])
                y = y / (1.0 + math.exp(-y))
                assert abs(y - float(ref[0, p, ch])) <= 1e-12 * max(1.0, abs(y))
    c = dict(kind="layernorm", M=2, C=8, ldx_extra=0, opts={}, tag="")
    d = T.inputs(c, dt)
    ref = T.reference(c, d)
    for r in range(2):
        vals = [float(t) for t in d["x"][r]]
        mean = sum(vals) / 8; var = sum((t - mean) ** 2 for t in vals) / 8
        for j in range(8):
            y = (vals[j] - mean) / math.sqrt(var + 1e-5) * float(d["gamma"][j]) + float(d["beta"][j])
            assert abs(y - float(ref[r, j])) <= 1e-12 * max(1.0, abs(y))
    c = dict(kind="softmax", rows=2, T=5, ldy=8, opts={}, tag="")
    d = T.inputs(c, dt)
    ref = T.reference(c, d)
    for r in range(2):
        vals = [float(t) for t in d["x"][r]]
        e = [math.exp(t - max(vals)) for t in vals]
        for j in range(5):
            assert abs(e[j] / sum(e) - float(ref[r, j])) <= 1e-12
