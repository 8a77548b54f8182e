"""CPU: the attention routing decision (magicdrive_amd/csrc/attn_route.h), evaluated by tests/attn_route_check.cpp (g++) for every case of
tests/golden/attn_routes.json.  The golden tags are what mdx_last_kernel() reported on the GPU for the library BEFORE routing moved into
attn_route.h (tools/attn_route_table.py); the threshold edges are compared with values worked out by hand from the rules."""
import pytest

import attn_route_table as T

CASES = T.load()


def line(**kw):
    """A dense self-attention descriptor (K rows H d wide, V^T rows roundup8(Tk) long) with overrides; option keys pass through."""
    f = dict(B=8, H=8, Tq=256, d=40, nsrc=1)
    f.update(kw)
    f.setdefault("Tk", f["Tq"])
    C = f["H"] * f["d"]
    f.setdefault("ldk", C); f.setdefault("sK", f["Tk"] * f["ldk"])
    f.setdefault("ldv", (f["Tk"] + 7) // 8 * 8); f.setdefault("sV", C * f["ldv"])
    return " ".join(f"{k}={v}" for k, v in f.items())


# Worked out from the rules (the issue's "behaviour to keep"), not from the code's output.  Defaults: ATTN2 1, D80 2, QT 0, FOLD 1, RES 1, PF 1, NW 0,
# NW4_BLOCKS 256, NW8_BLOCKS 2^40.
EDGES = {
    # ---- selection order: tk_dev before everything; causal or v_rowmajor -> short ----
    "ctx_first": (line(has_tk_dev=1, causal=1, v_rowmajor=1, d=16), "attn_ctx_kernel<16,scaled>"),
    "ctx_pre_rows": (line(has_tk_dev=1, rows=1, q_prescaled=1, d=160), "attn_ctx_kernel<160,pre,rows>"),
    "short_causal": (line(causal=1, v_rowmajor=1, d=64, Tq=77), "attn_short_kernel<64,causal>"),
    "short_rowmajor_only": (line(v_rowmajor=1, d=32, Tq=77), "attn_short_kernel<32,full>"),
    "short_causal_only": (line(causal=1, d=32, Tq=77), "attn_short_kernel<32,causal>"),      # the short route refuses it (v_rowmajor == 0)
    # ---- attn2 takes a launch: Tq 255 / 256 (B H = 64: 2 blocks of 128 each -> 128 workgroups) ----
    # 255: flash; blocks4 = 2 * 64 = 128 < 256, H B = 64 < 512, Tq >= 64 -> 2 waves
    "a2_tq255": (line(Tq=255), "attn_kernel<3,2,self>"),
    "a2_tq256": (line(Tq=256), "attn2_kernel<40,self,q32>"),
    # workgroups 127 / 128: Tq = 256 (2 blocks), H = 1: B = 63 -> 126, B = 64 -> 128; Tq = 16256 (127 blocks) / 16257 (128) at B = H = 1
    "a2_wg126": (line(Tq=256, H=1, B=63), "attn_kernel<3,2,self>"),
    "a2_wg127": (line(Tq=16256, H=1, B=1), "attn_kernel<3,2,self>"),
    "a2_wg128": (line(Tq=16257, H=1, B=1), "attn2_kernel<40,self,q64>"),
    "a2_off": (line(Tq=256, ATTN2=0), "attn_kernel<3,2,self>"),
    # head dim: 80 only as the two-source summed form by default; D80 = 1 always, 0 never; joint two-source is not "xview"
    "a2_d80_self": (line(d=80, Tq=384), "attn_kernel<5,2,self>"),
    "a2_d80_xview": (line(d=80, Tq=384, nsrc=2), "attn2_kernel<80,xview,q32>"),
    "a2_d80_joint": (line(d=80, Tq=384, nsrc=2, joint=1), "attn_kernel<5,2,joint>"),
    "a2_d80_always": (line(d=80, Tq=384, ATTN2_D80=1), "attn2_kernel<80,self,q32>"),
    "a2_d80_never": (line(d=80, Tq=384, nsrc=2, ATTN2_D80=0), "attn_kernel<5,2,xview>"),
    "a2_d80_pre_q512": (line(d=80, Tq=512, nsrc=2, q_prescaled=1), "attn2_kernel<80,xview,q32>"),       # d = 80: q32, no fold
    "a2_d48": (line(d=48, Tq=256), "attn_kernel<3,2,self>"),
    # strides: multiples of 8; ldv >= roundup8(Tk): Tk = 77 -> 80, ldv = 72 is 80 - 8
    "a2_ldk4": (line(ldk=324), "attn_kernel<3,2,self>"), "a2_sK4": (line(sK=256 * 320 + 4), "attn_kernel<3,2,self>"),
    "a2_sV4": (line(sV=320 * 256 + 4), "attn_kernel<3,2,self>"), "a2_ldv4": (line(ldv=260), "attn_kernel<3,2,self>"),
    "a2_ldv_short": (line(Tk=77, ldv=72), "attn_kernel<3,2,self>"), "a2_ldv_exact": (line(Tk=77, ldv=80), "attn2_kernel<40,self,q32>"),
    # the 2 GiB window: Tk ldk 2 < 2^30 with K a column block of q|k (ldk = 640, so that V^T at 640 roundup8(Tk) stays far below):
    # Tk = 838860 -> 1073740800 (under), 838861 -> 1073742080 (over);
    # d H ldv 2 = 640 ldv: ldv = 1677720 -> 1073740800 (under), 1677728 -> 1073745920 (over), Tk small so that only V^T decides
    "a2_kwin_under": (line(Tk=838860, ldk=640), "attn2_kernel<40,self,q32>"), "a2_kwin_over": (line(Tk=838861, ldk=640), "attn_kernel<3,2,self>"),
    "a2_vwin_under": (line(Tk=64, ldv=1677720), "attn2_kernel<40,self,q32>"), "a2_vwin_over": (line(Tk=64, ldv=1677728), "attn_kernel<3,2,self>"),
    # ---- inside attn2: q64 from Tq = 512 (not pre-scaled); pre-scaled: fold -> pf q32 unless QT = 2 forces q64 at Tq >= 512 ----
    "a2_tq511": (line(Tq=511), "attn2_kernel<40,self,q32>"), "a2_tq512": (line(Tq=512), "attn2_kernel<40,self,q64>"),
    "a2_tq512_qt1": (line(Tq=512, ATTN2_QT=1), "attn2_kernel<40,self,q32>"),
    "a2_pre_tq512": (line(Tq=512, q_prescaled=1), "attn2_kernel<40,self,q32,fold,pf>"),
    "a2_pre_tq512_qt2": (line(Tq=512, q_prescaled=1, ATTN2_QT=2), "attn2_kernel<40,self,q64,fold>"),
    "a2_pre_tq511_qt2": (line(Tq=511, q_prescaled=1, ATTN2_QT=2), "attn2_kernel<40,self,q32,fold,pf>"),
    "a2_pre_nopf": (line(Tq=512, q_prescaled=1, ATTN2_PF=0), "attn2_kernel<40,self,q32,fold>"),
    "a2_pre_nofold": (line(Tq=512, q_prescaled=1, ATTN2_FOLD=0), "attn2_kernel<40,self,q64>"),
    "a2_pre_xview": (line(Tq=512, q_prescaled=1, nsrc=2), "attn2_kernel<40,xview,q32,fold,pf>"),
    "a2_pre_joint6": (line(Tq=512, q_prescaled=1, nsrc=6, joint=1), "attn2_kernel<40,joint,q32,fold,pf>"),
    # ---- resident: d 40, fold, one source, ceil(Tk / 64) <= 3, RES 2 or (RES 1, Tq >= 512, B H >= 1024) ----
    "res_bh1023": (line(B=93, H=11, Tq=512, Tk=78, q_prescaled=1), "attn2_kernel<40,self,q32,fold,pf>"),       # 93 * 11 = 1023
    "res_bh1024": (line(B=128, H=8, Tq=512, Tk=78, q_prescaled=1), "attn2_kernel<40,resident,q32,fold>"),
    "res_tq511": (line(B=128, H=8, Tq=511, Tk=78, q_prescaled=1), "attn2_kernel<40,self,q32,fold,pf>"),
    "res_tk192": (line(B=128, H=8, Tq=512, Tk=192, q_prescaled=1), "attn2_kernel<40,resident,q32,fold>"),      # 3 tiles
    "res_tk193": (line(B=128, H=8, Tq=512, Tk=193, q_prescaled=1), "attn2_kernel<40,self,q32,fold,pf>"),       # 4 tiles
    "res_forced": (line(Tq=256, Tk=192, q_prescaled=1, ATTN2_RES=2), "attn2_kernel<40,resident,q32,fold>"),
    "res_forced_tk193": (line(Tq=256, Tk=193, q_prescaled=1, ATTN2_RES=2), "attn2_kernel<40,self,q32,fold,pf>"),
    "res_off": (line(B=128, H=8, Tq=512, Tk=78, q_prescaled=1, ATTN2_RES=0), "attn2_kernel<40,self,q32,fold,pf>"),
    "res_not_prescaled": (line(B=128, H=8, Tq=512, Tk=78), "attn2_kernel<40,self,q64>"),
    "res_nofold": (line(B=128, H=8, Tq=512, Tk=78, q_prescaled=1, ATTN2_FOLD=0), "attn2_kernel<40,self,q64>"),
    "res_two_sources": (line(B=128, H=8, Tq=512, Tk=78, q_prescaled=1, nsrc=2, ATTN2_RES=2), "attn2_kernel<40,xview,q32,fold,pf>"),
    # ---- flash waves (d = 160: never attn2).  NW4_BLOCKS = 256: H B = 511 = 7 * 73 / 512 = 8 * 64 ----
    "nw_hb511_t28": (line(d=160, B=73, H=7, Tq=28), "attn_kernel<10,1,self>"),               # 511 < 512, Tq < 64 -> 1 wave
    "nw_hb512_t28": (line(d=160, B=64, H=8, Tq=28), "attn_kernel<10,4,self>"),
    "nw_hb512_t32_two": (line(d=160, B=64, H=8, Tq=32, nsrc=2), "attn_kernel<10,2,xview>"),
    "nw_hb512_t33_two": (line(d=160, B=64, H=8, Tq=33, nsrc=2), "attn_kernel<10,4,xview>"),
    "nw_hb512_t32_joint2": (line(d=160, B=64, H=8, Tq=32, nsrc=2, joint=1), "attn_kernel<10,2,joint>"),      # the rule reads nsrc, not joint
    "nw_hb511_t32_two": (line(d=160, B=73, H=7, Tq=32, nsrc=2), "attn_kernel<10,1,xview>"),
    "nw_t63": (line(d=160, B=2, Tq=63), "attn_kernel<10,1,self>"), "nw_t64": (line(d=160, B=2, Tq=64), "attn_kernel<10,2,self>"),
    # 4 waves from Tq = 256 with ceil(Tq / 128) H B >= 256: B = 16, H = 8: 2 * 128 = 256; B = 15: 240 and H B = 120 < 512 -> 2 waves
    "nw_t256_b256": (line(d=160, B=16, Tq=256), "attn_kernel<10,4,self>"), "nw_t256_b240": (line(d=160, B=15, Tq=256), "attn_kernel<10,2,self>"),
    "nw_t255_b256": (line(d=160, B=16, Tq=255), "attn_kernel<10,2,self>"),
    # 8 waves: never by default (2^40 blocks); with NW8_BLOCKS = 64: Tq = 512 -> 2 blocks of 256 * 32 = 64; Tq = 511 falls to the 4-wave rule (4 * 32 = 128 < 256 -> 2 waves)
    "nw8_default": (line(d=160, B=64, Tq=1400), "attn_kernel<10,4,self>"),
    "nw8_t512": (line(d=160, B=4, Tq=512, ATTN_NW8_BLOCKS=64), "attn_kernel<10,8,self>"),
    "nw8_t511": (line(d=160, B=4, Tq=511, ATTN_NW8_BLOCKS=64), "attn_kernel<10,2,self>"),
    "nw8_blocks63": (line(d=160, B=4, Tq=512, ATTN_NW8_BLOCKS=65), "attn_kernel<10,2,self>"),
    # a forced wave count wins; a value outside {1, 2, 4, 8} is the heuristic
    "nw_force1": (line(d=160, B=64, Tq=1400, ATTN_NW=1), "attn_kernel<10,1,self>"), "nw_force2": (line(d=160, B=64, Tq=1400, ATTN_NW=2), "attn_kernel<10,2,self>"),
    "nw_force4": (line(d=160, B=1, Tq=28, ATTN_NW=4), "attn_kernel<10,4,self>"), "nw_force8": (line(d=160, B=1, Tq=28, ATTN_NW=8), "attn_kernel<10,8,self>"),
    "nw_force3": (line(d=160, B=1, Tq=28, ATTN_NW=3), "attn_kernel<10,1,self>"),
    # d16 = ceil(d / 16): 1 .. 6, 8, 10 have instances; 7 (d 104, 112) and 9 (d 136, 144) are named as they are and refused by the entry point
    "d16_1": (line(d=8, Tq=33, B=1, H=1), "attn_kernel<1,1,self>"), "d16_1b": (line(d=16, Tq=33, B=1, H=1), "attn_kernel<1,1,self>"),
    "d16_2": (line(d=24, Tq=33, B=1, H=1), "attn_kernel<2,1,self>"), "d16_6": (line(d=96, Tq=33, B=1, H=1), "attn_kernel<6,1,self>"),
    "d16_7": (line(d=104, Tq=33, B=1, H=1), "attn_kernel<7,1,self>"), "d16_7b": (line(d=112, Tq=33, B=1, H=1), "attn_kernel<7,1,self>"),
    "d16_8": (line(d=120, Tq=33, B=1, H=1), "attn_kernel<8,1,self>"), "d16_9": (line(d=136, Tq=33, B=1, H=1), "attn_kernel<9,1,self>"),
    "d16_9b": (line(d=144, Tq=33, B=1, H=1), "attn_kernel<9,1,self>"), "d16_10": (line(d=152, Tq=33, B=1, H=1), "attn_kernel<10,1,self>"),
}
FAMILY = {"attn_ctx_kernel": "ctx", "attn_short_kernel": "short", "attn_kernel": "flash"}


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    lines = [f"{c['name']} {T.route_line(c)}" for c in CASES] + [f"{name} {kv}" for name, (kv, _) in EDGES.items()]
    out = T.evaluate(lines, tmp_path_factory.mktemp("route"))
    if out is None:
        pytest.skip("no g++")
    return out


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_route_tag_matches_recorded_kernel(routes, c):
    assert routes[c["name"]]["tag"] == c["tag"], (routes[c["name"]], c["tag"])


@pytest.mark.parametrize("name", sorted(EDGES))
def test_threshold_edges_worked_out_by_hand(routes, name):
    want = EDGES[name][1]
    got = routes[name]
    assert got["tag"] == want, (name, EDGES[name][0], got)
    head = want.split("<")[0]
    assert got["family"] == (("attn2-resident" if ",resident," in want else "attn2") if head == "attn2_kernel" else FAMILY[head]), got


def test_the_table_covers_the_plans_and_the_forced_settings():
    """Every family is in the recorded table, and every forced setting of tests/test_routes_gpu.py::test_forced_attention_routes."""
    heads = {c["tag"].split("<")[0] for c in CASES}
    assert heads == {"attn_kernel", "attn2_kernel", "attn_short_kernel", "attn_ctx_kernel"}, heads
    assert any(",resident," in c["tag"] for c in CASES) and any(c["tag"].endswith(",rows>") for c in CASES)
    forced = {tuple(sorted(c["opts"].items())) for c in CASES}
    for opts in ({"ATTN2": 0}, {"ATTN2_QT": 1}, {"ATTN2_QT": 2}, {"ATTN2_D80": 0}, {"ATTN2_D80": 1}, {"ATTN2_RES": 0}, {"ATTN2_RES": 2}, {"ATTN2_PF": 0},
                 {"ATTN2_FOLD": 0}, {"ATTN_NW": 1}, {"ATTN_NW": 2}, {"ATTN_NW": 4}, {"ATTN_NW": 8}):
        assert tuple(sorted(opts.items())) in forced, opts
