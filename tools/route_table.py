#!/usr/bin/env python
"""Record which kernel the built library routes each case of the GEMM / conv route table to.

    python tools/route_table.py --jsonl profiles/route_refactor_new.jsonl            # tag + SHA-256 of the output per case
    MDX_LIB_PATH=<other build> python tools/route_table.py --jsonl ... --golden tests/golden/gemm_routes.json

Each case is issued once (tests/gemm_route_table.py: run_case); `gpu: False` cases exist for the CPU test only (tests/test_gemm_route.py works
their expectation out by hand) and are written to the golden file without a tag.  Shapes sit on the thresholds of csrc/gemm_route.h.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NOXL = {"GEMM_XL": 0}


def g(name, M, N, K, **kw):
    return dict(name=name, M=M, N=N, K=K, **kw)


def conv(name, B, H, W, Cin, Cout, **kw):
    return dict(name=name, kind="conv", B=B, H=H, W=W, Cin=Cin, Cout=Cout, **kw)


CASES = [
    # gemm_ws: M = 8191 / 8192 at K = 320; its 2 GiB window (M * lda * 2 against 0x7FFF0000 = 2 * 448 * 2396672; CPU only)
    g("ws_m8191", 8191, 320, 320), g("ws_m8192", 8192, 320, 320),
    g("ws_window_under", 2396671, 320, 320, lda=448, gpu=False), g("ws_window_at", 2396672, 320, 320, lda=448, gpu=False),
    g("ws_off", 8192, 320, 320, opts={"GEMM_WS": 0}), g("ws_always", 1000, 320, 320, opts={"GEMM_WS": 2}),
    # XL_MIN_TILES: 63 / 64 tiles (N = 160: one N-tile at every width)
    g("xl_tiles63", 63 * 256, 160, 640), g("xl_tiles64", 64 * 256, 160, 640),
    g("xl_forced_small", 777, 324, 128, bias=False, opts={"GEMM_XL": 2}), g("xl_silu_declined", 5000, 320, 64, epi=2, opts={"GEMM_XL": 2}),
    # small grids: 1408 / 1409 tiles of 64 x 64; a 1 x 1 conv at 40000 = 1600 * 25 and 40001 = 3077 * 13 (tile, slab) units
    g("small_1408", 1408 * 64, 64, 64, opts=NOXL), g("small_1409", 1409 * 64, 64, 64, opts=NOXL),
    conv("small_conv_40000", 4, 40, 40, 1600, 1024, k=1), conv("small_conv_40001", 181, 8, 8, 832, 1088, k=1),
    g("small_off", 2100, 640, 640, res=True, opts={"GEMM_XL": 0, "GEMM_SMALL_TILES": 0}), g("small_off_m546", 546, 1280, 1280, res=True, opts={"GEMM_XL": 0, "GEMM_SMALL_TILES": 0}),
    g("small_on", 2100, 640, 640, res=True, opts=NOXL),
    # automatic split-K: tiles 383 / 384, K 960 / 1024, the K / 512 cap, the 32 cap, a workspace of 3 slabs where 5 are wanted, forced without one
    g("sk_tiles383", 383 * 64, 64, 1024, opts=NOXL), g("sk_tiles384", 384 * 64, 64, 1024, opts=NOXL),
    g("sk_k960", 1024, 640, 960, opts=NOXL), g("sk_k1024", 1024, 640, 1024, opts=NOXL), g("sk_kcap", 1024, 640, 2048, opts=NOXL),
    g("sk_cap32", 64, 64, 32768, opts=NOXL), g("sk_ws_small", 1024, 640, 4096, ws_mb=8, opts=NOXL),
    g("sk_forced", 1024, 640, 2048, splitk=3, opts=NOXL), g("sk_no_ws", 1024, 640, 2048, splitk=4, ws_null=True, gpu=False),
    g("sk_before_xl", 64 * 256, 64, 1024), g("sk_forced_xl_first", 64 * 256, 64, 1024, opts={"GEMM_XL": 2}),
    conv("sk_conv", 6, 7, 13, 2560, 1280, res=True, temb=True, opts=NOXL),
    # geglu_xl (XL_GEGLU320): 1023 = 33 * 31 / 1024 = 32 * 32 tiles of 256 x 256
    g("geglu320_1023", 33 * 256, 31 * 256, 320, epi=1, opts={"XL_GEGLU320": 1}), g("geglu320_1024", 32 * 256, 32 * 256, 320, epi=1, opts={"XL_GEGLU320": 1}),
    g("geglu320_default", 32 * 256, 32 * 256, 320, epi=1), g("geglu_forced_xl", 3000, 1280, 320, epi=1, opts={"GEMM_XL": 2, "XL_BN": 256}),
    g("geglu_generic_m511", 511, 1280, 640, epi=1), g("geglu_generic_m512", 512, 1280, 640, epi=1), g("geglu_bad_n", 512, 96, 640, epi=1, gpu=False),
    # the batch-flattened form: 127 / 128 tiles of 256 x 160
    dict(name="flat_127", kind="flat", Bt=1270, T=16, Cc=256), dict(name="flat_128", kind="flat", Bt=1271, T=16, Cc=256),
    dict(name="flat_off", kind="flat", Bt=1271, T=16, Cc=256, opts={"GEMM_FLATTEN": 0}), dict(name="flat_noxl", kind="flat", Bt=1271, T=16, Cc=256, opts=NOXL),
    # upsampled-2x conv: whole and with both axes cropped; GEMM_XL = 0 and XL_MIN_TILES do not apply; XL_BN overrides
    dict(name="up2_whole", kind="up2", B=8, H=14, W=25, Cin=64, Cout=320, Ho=28, Wo=50), dict(name="up2_cropped", kind="up2", B=8, H=14, W=25, Cin=64, Cout=320, Ho=27, Wo=49),
    dict(name="up2_noxl", kind="up2", B=8, H=14, W=25, Cin=64, Cout=320, Ho=28, Wo=50, opts=NOXL),
    dict(name="up2_bn320", kind="up2", B=8, H=14, W=25, Cin=64, Cout=320, Ho=28, Wo=50, opts={"XL_BN": 320}),
    dict(name="up2_bn160", kind="up2", B=8, H=14, W=25, Cin=64, Cout=320, Ho=28, Wo=50, opts={"XL_BN": 160}),
    dict(name="up2_cin32", kind="up2", B=8, H=14, W=25, Cin=32, Cout=320, Ho=28, Wo=50, gpu=False), dict(name="up2_not_conv", kind="up2", B=8, H=14, W=25, Cin=64, Cout=320, Ho=28, Wo=50, conv=0, gpu=False),
    # convs: XL at >= 64 tiles, generic below; forced
    conv("conv_xl", 12, 28, 50, 320, 320, res=True, temb=True), conv("conv_63", 63, 16, 16, 64, 160), conv("conv_64", 64, 16, 16, 64, 160),
    conv("conv_forced_xl", 6, 28, 50, 320, 320, res=True, temb=True, opts={"GEMM_XL": 2}), conv("conv_stride2", 6, 28, 50, 64, 320, stride=2, opts={"GEMM_XL": 2}),
    conv("conv_noxl", 16, 28, 50, 320, 320, res=True, temb=True, opts=NOXL),
    # forced tiles
    g("bm256", 8736, 1280, 1280, res=True, opts={"GEMM_XL": 0, "GEMM_BM256": 4096}), g("noxl_big", 8736, 1280, 1280, res=True, opts=NOXL),
    g("force_bm64", 8736, 1280, 1280, opts={"GEMM_XL": 0, "GEMM_BM": 64}), g("force_bn64", 8736, 1280, 1280, opts={"GEMM_XL": 0, "GEMM_BN": 64}),
    g("force_bk32", 2100, 640, 640, opts={"GEMM_XL": 0, "GEMM_BK": 32}),
    # XL_K320: the XL kernel takes the K = 320 projection, or declines and gemm_ws.hip runs behind the pre- / post-steps
    g("k320_xl", 8192, 320, 320, opts={"XL_K320": 1}), g("k320_declined", 1000, 320, 320, opts={"XL_K320": 1, "GEMM_WS": 2}),
    g("k320_declined_ln", 1000, 320, 320, ln=True, opts={"XL_K320": 1, "GEMM_WS": 2}), g("k320_declined_rowstat", 1000, 320, 320, rowstat=3, opts={"XL_K320": 1, "GEMM_WS": 2}),
    # LayerNorm / row statistics: fused on gemm_ws.hip, the three fall-backs, the A/B switches
    g("ln_fused", 8192, 960, 320, ln=True), g("ln_fused_stats", 8192, 960, 320, ln=True, ln_stats=1), g("ln_geglu_stats", 8192, 2560, 320, epi=1, ln=True, ln_stats=1),
    g("ln_geglu_no_stats", 8192, 2560, 320, epi=1, ln=True), g("ln_fuse_off", 8192, 960, 320, ln=True, opts={"LN_FUSE": 0}),
    g("ln_stats_off", 8192, 2560, 320, epi=1, ln=True, ln_stats=1, opts={"LN_STATS": 0}), g("ln_small_m", 1000, 960, 320, ln=True),
    g("ln_no_scratch", 1000, 960, 320, ln=True, ln_scratch=False, gpu=False), g("ln_stats_5_parts", 8192, 960, 320, ln=True, ln_stats=5),
    g("rowstat_ws", 8192, 320, 320, rowstat=3), g("rowstat_ws_few_parts", 8192, 320, 320, rowstat=2), g("rowstat_small_m", 1000, 320, 320, rowstat=3),
    g("rowstat_fuse_off", 8192, 320, 320, rowstat=3, opts={"LN_FUSE": 0}), g("rowstat_stats_off", 8192, 320, 320, rowstat=3, opts={"LN_STATS": 0}),
    g("rowstat_epi", 8192, 320, 320, rowstat=3, epi=2, gpu=False), conv("ln_conv", 6, 28, 50, 320, 320, ln=True, gpu=False),
]
# width ties: N = 320 / 640 / 960 / 1280 at K = 320 (gemm_ws.hip off) / 640 / 2880
for n in (320, 640, 960, 1280):
    for k in (320, 640, 2880):
        CASES.append(g(f"width_n{n}_k{k}", 64 * 256, n, k, opts={"GEMM_WS": 0} if k == 320 else {}))
# every XL width forced (tests/test_routes_gpu.py: test_forced_xl_widths)
for bn in (320, 256, 160):
    CASES.append(g(f"forced_bn{bn}", 2000, 640, 640, res=True, opts={"GEMM_XL": 2, "XL_BN": bn}))
    CASES.append(conv(f"forced_conv_bn{bn}", 12, 14, 25, 128, 640, opts={"GEMM_XL": 2, "XL_BN": bn}))
    CASES.append(g(f"cost_model_bn{bn}", 64 * 256, 640, 640, opts={"XL_BN": bn}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jsonl", required=True)
    ap.add_argument("--golden", help="also write the case table with the tags of this run (the content of tests/golden/gemm_routes.json) here")
    a = ap.parse_args()
    import gemm_route_table as T
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    out = []
    os.makedirs(os.path.dirname(os.path.abspath(a.jsonl)), exist_ok=True)
    with open(a.jsonl, "w") as f:
        for c in CASES:
            full = dict(T.DEFAULTS, **c)
            tag = None
            if full["gpu"]:
                try:
                    tag, sha = T.run_case(full)
                except (ValueError, RuntimeError) as e:      # a refused descriptor is a result too
                    tag, sha = "refused", str(e)[:160]
                f.write(json.dumps({"name": c["name"], "tag": tag, "sha256": sha}) + "\n")
                f.flush()
                print(c["name"], tag, sha[:12], flush=True)
            out.append(dict(c, tag=tag))
    if a.golden:
        with open(a.golden, "w") as f:
            f.write('{"cases": [\n' + ",\n".join(json.dumps(c) for c in out) + "\n]}\n")


if __name__ == "__main__":
    main()
