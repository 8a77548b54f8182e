"""CPU: the GEMM / conv routing decision (magicdrive_amd/csrc/gemm_route.h), evaluated by tests/gemm_route_check.cpp (g++) for every case of
tests/golden/gemm_routes.json.  The golden tags are what mdx_last_kernel() reported on the GPU for the library BEFORE routing moved into
gemm_route.h (tools/route_table.py); what a tag does not show (split-K, pre- and post-steps, errors, the CPU-only cases) is compared with
values worked out by hand from the rules."""
import os

import pytest

import gemm_route_table as T

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    out = T.evaluate([f"{name} {kv}" for c in T.load() for name, kv in T.route_lines(c)], tmp_path_factory.mktemp("route"))
    if out is None:
        pytest.skip("no g++")
    return out


def final(routes, c):
    """The route a case ends on: a flat case declines (no message) to the per-batch launches."""
    if c["kind"] != "flat":
        return routes[c["name"]]
    flat_ok = c["opts"].get("GEMM_FLATTEN", 1) and routes[c["name"] + "#flat"]["err"] == "0"
    return routes[c["name"] + ("#flat" if flat_ok else "#batch")]


GPU_CASES = [c for c in T.load() if c["gpu"]]


@pytest.mark.parametrize("c", GPU_CASES, ids=[c["name"] for c in GPU_CASES])
def test_route_tag_matches_recorded_kernel(routes, c):
    r = final(routes, c)
    assert r["err"] == "0", r
    want = c["tag"]
    if want.startswith("gemm_xlp_kernel<256x256,"):
        # the persistent form of the 256-wide XL GEMM is chosen inside launch_xl (it depends on the CU count): same route, same epilogue
        assert want == "gemm_xlp_kernel<256x256,%s%s>" % ("geglu" if c["epi"] == 1 else "gemm", "+res" if c["res"] else "")
        want = "gemm_xl_kernel<256x256,gemm>"
    assert r["last"] == want, (r, want)


# What the tag does not show.  Worked out from the rules (the issue's "behaviour to keep"), not from the code's output:
#   split-K: tiles < 384, K >= 1024 -> want = ceil(768 / tiles) capped by K / 512 and 32, shrunk to ws_bytes / (4 M N); kchunk = ceil(K / splitk) rounded
#   up to 64, splitk = ceil(K / kchunk).  sk_tiles383: 383 tiles of 64 x 64, want 3, K / 512 = 2.  sk_ws_small: want 5 of 8, 8 MiB / 2.5 MiB = 3 slabs,
#   ceil(4096 / 3) = 1366 -> 1408.  sk_conv: M 546 (5 tiles of 128) x N 1280 (10): 50 tiles, want 16 of 45, 23040 / 16 = 1440 -> 1472, ceil(23040 / 1472) = 16.
#   small_off_m546: 9 x 10 tiles of 64 x 128, want 9, K / 512 = 2.  sk_forced: 3 forced, ceil(2048 / 3) = 683 -> 704.
EXPECT = {
    "sk_tiles383": dict(BM="64", BN="64", splitk="2", kchunk="512"), "sk_tiles384": dict(splitk="1", kchunk="1024"),
    "sk_k960": dict(splitk="1", kchunk="960"), "sk_k1024": dict(splitk="2", kchunk="512"), "sk_kcap": dict(splitk="4", kchunk="512"),
    "sk_cap32": dict(splitk="32", kchunk="1024"), "sk_ws_small": dict(splitk="3", kchunk="1408"), "sk_forced": dict(splitk="3", kchunk="704"),
    "sk_conv": dict(BM="128", BN="128", splitk="16", kchunk="1472"), "small_off_m546": dict(BM="64", BN="128", splitk="2", kchunk="640"),
    "sk_before_xl": dict(main="gemm_conv_kernel<64,64,64,2,2,gemm>", splitk="2", kchunk="512"),
    "sk_forced_xl_first": dict(main="gemm_xl_kernel<256x160,gemm>"),    # one round of 64 tiles: 16.6 + 1.116 * 16 is the cheapest
    "sk_no_ws": dict(err="-1", msg="split-K needs a workspace"),
    "force_bk32": dict(BK="32", kchunk="640"),
    # M * lda * 2 = 0x7FFF0000 - 896 / 0x7FFF0000: the window holds the first only; the longer A goes to the XL kernel, where one 320-wide N-tile
    # (33.2 us a round) beats two 160-wide ones (2 x 22.2) and two 256-wide ones (2 x 21.2)
    "ws_window_under": dict(main="gemm_ws_kernel<plain>"), "ws_window_at": dict(main="gemm_xl_kernel<256x320,gemm>", bn="320"),
    "geglu_bad_n": dict(err="-1", msg="GEGLU needs packed N % 64 == 0 (N=96)"),
    "up2_not_conv": dict(err="-1", msg="upsample2x: conv only"), "up2_cin32": dict(err="-1"),
    "up2_whole": dict(bn="256"), "up2_cropped": dict(bn="256"), "up2_noxl": dict(bn="256"), "up2_bn320": dict(bn="320"), "up2_bn160": dict(bn="256"),
    "flat_127#flat": dict(err="-3", msg=""), "flat_128#flat": dict(bn="160"), "flat_noxl#flat": dict(err="-3", msg=""),
    # LayerNorm / row statistics: fused in gemm_ws.hip when it takes the launch and can; else a pre-step into ln_scratch / a post-step over C
    "ln_fused": dict(normalise_first="0", keep_ln="1", keep_ln_stats="0"), "ln_fused_stats": dict(normalise_first="0", keep_ln="1", keep_ln_stats="1"),
    "ln_geglu_stats": dict(normalise_first="0", keep_ln="1", keep_ln_stats="1"), "ln_geglu_no_stats": dict(normalise_first="1", keep_ln="0", main="gemm_ws_kernel<geglu>"),
    "ln_fuse_off": dict(normalise_first="1", keep_ln="0"), "ln_stats_off": dict(normalise_first="1", keep_ln="0", keep_ln_stats="0"),
    "ln_small_m": dict(normalise_first="1", keep_ln="0", main="gemm_conv_kernel<64,64,64,2,2,gemm>"), "ln_stats_5_parts": dict(normalise_first="1", keep_ln="0"),
    "ln_no_scratch": dict(err="-1", msg="fused LayerNorm: this shape is not normalised in-kernel and no ln_scratch was given"),
    "ln_conv": dict(err="-1", msg="fused LayerNorm: plain 2-D GEMM only"),
    "rowstat_ws": dict(rowstat_after="0", keep_rowstat="1"), "rowstat_ws_few_parts": dict(rowstat_after="1", keep_rowstat="0", main="gemm_ws_kernel<plain>"),
    "rowstat_small_m": dict(rowstat_after="1", keep_rowstat="0"), "rowstat_fuse_off": dict(rowstat_after="1", keep_rowstat="0", main="gemm_ws_kernel<plain>"),
    "rowstat_stats_off": dict(rowstat_after="0", keep_rowstat="0", main="gemm_ws_kernel<plain>"),
    "rowstat_epi": dict(err="-1", msg="rowstat_out: plain 2-D GEMM with 16-bit C only"),
    # XL_K320 set, 4 tiles (< XL_MIN_TILES): the XL kernel declines, gemm_ws.hip runs, and because it was not THE first choice the rows are
    # normalised first / the statistics taken afterwards
    "k320_declined": dict(main="gemm_ws_kernel<plain>", normalise_first="0", rowstat_after="0"),
    "k320_declined_ln": dict(main="gemm_ws_kernel<plain>", normalise_first="1", keep_ln="0"),
    "k320_declined_rowstat": dict(main="gemm_ws_kernel<plain>", rowstat_after="1", keep_rowstat="0", last="rowstat_kernel"),
}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_route_details_worked_out_by_hand(routes, name):
    got = routes[name]
    for k, v in EXPECT[name].items():
        assert got.get(k) == v, (name, k, v, got)


def test_every_cpu_only_case_has_an_expectation():
    for c in T.load():
        assert c["gpu"] or c["name"] in EXPECT, c["name"]
