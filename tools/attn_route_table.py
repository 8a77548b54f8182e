#!/usr/bin/env python
"""Record which kernel the built library routes each case of the attention route table to (the sibling of tools/route_table.py).

    python tools/attn_route_table.py --golden tests/golden/attn_routes.json
    MDX_LIB_PATH=<other build> python tools/attn_route_table.py --golden ...

Each case is issued once (tests/attn_route_table.py: run_case) and written with the tag mdx_last_kernel() reported.  The cases are the
attention sites of the real plans (8 heads; head dim 40 / 80 / 160 / 160 at 1400 / 350 / 91 / 28 tokens; Q pre-scaled; 12 views = one scene
with guidance, 144 = twelve) as self, cross-view, joint and text-context attention, the CLIP text encoder's, the tiny test nets', and the
level-0 / level-1 sites under each forced setting of tests/test_routes_gpu.py.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEVELS = [(1400, 40), (350, 80), (91, 160), (28, 160)]


def sites(B, tag, opts=None, levels=LEVELS):
    out = []
    o = dict(opts=opts) if opts else {}
    for T, d in levels:
        n = f"{tag}_t{T}_d{d}"
        out += [dict(name=f"self_{n}", B=B, Tq=T, d=d, **o), dict(name=f"xview_{n}", B=B, Tq=T, d=d, nsrc=2, **o),
                dict(name=f"joint2_{n}", B=B, Tq=T, d=d, nsrc=2, joint=True, **o), dict(name=f"text78_{n}", B=B, Tq=T, Tk=78, d=d, kmult=1, **o),
                dict(name=f"text110_{n}", B=B, Tq=T, Tk=110, d=d, kmult=1, **o)]
    return out


CASES = sites(12, "b12") + sites(144, "b144")
for T, d in LEVELS:
    CASES += [dict(name=f"joint6_b12_t{T}_d{d}", B=12, Tq=T, d=d, nsrc=6, joint=True),
              dict(name=f"ctx_b12_t{T}_d{d}", B=12, Tq=T, Tk=128, d=d, kmult=1, ctx="dev", live=91),
              dict(name=f"ctxrows_b12_t{T}_d{d}", B=12, Tq=T, Tk=128, d=d, kmult=1, ctx="rows", live=91)]
CASES += [
    # the CLIP text encoder: 77 tokens, 12 heads of 64, Q | K | V of one projection, causal; its tiny test net; the full-mask form
    dict(name="clip_b1", B=1, H=12, Tq=77, d=64, kmult=3, pre=False, causal=True, rowmajor=True),
    dict(name="clip_b2", B=2, H=12, Tq=77, d=64, kmult=3, pre=False, causal=True, rowmajor=True),
    dict(name="clip_tiny", B=2, H=2, Tq=77, d=32, kmult=3, pre=False, causal=True, rowmajor=True),
    dict(name="short_full", B=2, H=2, Tq=77, d=32, kmult=3, pre=False, rowmajor=True),
    # the tiny test nets: head dim 16 / 32, a plain (not pre-scaled) caller
    dict(name="tiny_self_d16", B=12, H=2, Tq=1400, d=16), dict(name="tiny_self_d32", B=12, H=2, Tq=350, d=32), dict(name="tiny_xview_d16", B=12, H=2, Tq=28, d=16, nsrc=2),
    dict(name="tiny_text_d16", B=12, H=2, Tq=1400, Tk=78, d=16, kmult=1), dict(name="tiny_ctx_d16", B=12, H=2, Tq=91, Tk=96, d=16, kmult=1, ctx="dev", live=80),
    dict(name="plain_self_d40", B=12, Tq=1400, d=40, pre=False), dict(name="plain_xview_d40", B=12, Tq=1400, d=40, nsrc=2, pre=False),
    dict(name="plain_text_d40", B=12, Tq=1400, Tk=78, d=40, kmult=1, pre=False), dict(name="plain_xview_d80", B=12, Tq=350, d=80, nsrc=2, pre=False),
    dict(name="wide_ldv_d40", B=12, Tq=1400, Tk=78, d=40, kmult=1, ldv_extra=8),
]
FORCED = [("attn2_off", {"ATTN2": 0}), ("qt1", {"ATTN2_QT": 1}), ("qt2", {"ATTN2_QT": 2}), ("d80_0", {"ATTN2_D80": 0}), ("d80_1", {"ATTN2_D80": 1}),
          ("res0", {"ATTN2_RES": 0}), ("res2", {"ATTN2_RES": 2}), ("pf0", {"ATTN2_PF": 0}), ("pf0_qt2", {"ATTN2_PF": 0, "ATTN2_QT": 2}), ("fold0", {"ATTN2_FOLD": 0}),
          ("nw1", {"ATTN_NW": 1}), ("nw2", {"ATTN_NW": 2}), ("nw4", {"ATTN_NW": 4}), ("nw8", {"ATTN_NW": 8})]
for tag, opts in FORCED:
    CASES += sites(12, tag, opts, LEVELS[:2])
    if tag.startswith("nw"):               # the flash kernels' wave counts also where they are the default route
        CASES += [dict(name=f"self_{tag}_t91_d160", B=12, Tq=91, d=160, opts=opts), dict(name=f"xview_{tag}_t28_d160", B=12, Tq=28, d=160, nsrc=2, opts=opts)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--golden", required=True, help="write the case table with the tags of this run (the content of tests/golden/attn_routes.json) here")
    a = ap.parse_args()
    import attn_route_table as T
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    out = []
    for c in CASES:
        tag = T.run_case(dict(T.DEFAULTS, **c))
        print(c["name"], tag, flush=True)
        out.append(dict(c, tag=tag))
    os.makedirs(os.path.dirname(os.path.abspath(a.golden)), exist_ok=True)
    with open(a.golden, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(c) for c in out) + "\n]}\n")


if __name__ == "__main__":
    main()
