"""CPU: the route of the register-resident GroupNorm.  csrc/gn_route.h (built with g++ through tests/gn_route_check.cpp) and its Python
mirror magicdrive_amd/gn_route.py agree on every GroupNorm site of the SD-1.5 step program at 224x400 and 432x768 and on the edges of the
rule; plans built on the CPU never contain the resident op; forcing it on replaces GroupNorm ops one for one (same op count, same FLOP /
byte accounting)."""
import os
import shutil
import subprocess

import pytest
import torch

from magicdrive_amd import denoiser as DN, flops, gn_route as GR, ops as O
from magicdrive_amd.engine import Builder, PackedNet
from magicdrive_amd.networks import spec

HERE = os.path.dirname(os.path.abspath(__file__))
CPU = torch.device("cpu")
FLOOR = 4 << 20          # default of the option GN_ONE_KERNEL_ELEMS


class ShapeNet(PackedNet):
    """Shape-only weights: the plan builder reads shapes, nothing is packed."""

    def _get(self, tag, keys, fn):
        ck = (tag,) + tuple(keys)
        if ck not in self.cache:
            self.cache[ck] = fn(*[torch.zeros(self.sd[k].shape) for k in keys])
        return self.cache[ck]


def sd15_plan(latent, mode=None):
    cfg = spec.SD15_CONFIG if latent == (28, 50) else spec.with_plus_map_embedder(spec.SD15_CONFIG, latent)
    z = lambda shapes: {k: torch.zeros(1).expand(s) for k, s in shapes.items()}
    Builder.gn_resident = mode
    try:
        un = ShapeNet(z(spec.unet_param_shapes(cfg)), CPU); cn = ShapeNet(z(spec.controlnet_param_shapes(cfg)), CPU)
        return DN.SamplerPlan(cfg, un, cn, CPU, 1, False, 32, latent, num_steps=50)
    finally:
        Builder.gn_resident = None


@pytest.fixture(scope="module")
def plans():
    return {lat: sd15_plan(lat) for lat in ((28, 50), (54, 96))}


def site_shapes(plan):
    """(HW, C, G, ldx, ldy) of every GroupNorm of the step program, duplicates removed."""
    out = []
    for op in plan.step_ops:
        if isinstance(op, O.GroupNorm):
            s = (op.X.shape[1], op.X.shape[2], op.groups, op.X.stride(1), op.Y.stride(1))
            if s not in out:
                out.append(s)
    return out


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to evaluate csrc/gn_route.h"
    exe = str(tmp_path_factory.mktemp("gn_route") / "gn_route_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "gn_route_check.cpp")], check=True)

    def run(cases):
        text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
        lines = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(lines) == len(cases) + 1
        return [tuple(int(v) for v in l.split()) for l in lines[:-1]], [int(v) for v in lines[-1].split()[1:]]
    return run


def brute_ks(HW, C, G):
    """{k: vectors per thread} of every k the kernel could run, from the statement of its limits (not from gn_route.py): k divides G, at most
    32 groups and 1024 channels per workgroup, channels per group even and >= 8, whole 16-byte vectors per block row, <= 22 vectors per thread
    with 1024 // vpr rows per pass."""
    cpg = C // G
    ks = {}
    for k in range(1, min(G, 32) + 1):
        if G % k or cpg < 8 or cpg % 2 or (k * cpg) % 8 or k * cpg > 1024:
            continue
        rows = 1024 // (k * cpg // 8)
        if -(-HW // rows) <= 22:
            ks[k] = -(-HW // rows)
    return ks


def brute_choice(ks):
    """The widest block of <= 4 vectors per thread (two workgroups per CU) when there is one, else the widest."""
    pair = [k for k, nv in ks.items() if nv <= 4]
    return max(pair) if pair else (max(ks) if ks else 0)


def test_constants_match(header):
    _, consts = header([])
    assert consts == [GR.GNR_THREADS, GR.GNR_MAX_NV, GR.GNR_MAX_CH, GR.GNR_MAX_K, GR.GNR_PAIR_NV, GR.GNR_ONE_KERNEL_ELEMS] == [1024, 22, 1024, 32, 4, FLOOR]


def test_every_site_shape(plans, header):
    """Header == mirror == the choice from the brute-force list, at 6, 192 and 576 views of every site of both resolutions."""
    cases = []
    for lat, plan in plans.items():
        shapes = site_shapes(plan)
        assert len(shapes) >= 10, shapes
        for (HW, C, G, ldx, ldy) in shapes:
            for B in (6, 192, 576):
                for floor in (FLOOR, 0):
                    cases.append((B, HW, C, G, ldx, ldy, 16, floor))
    got, _ = header(cases)
    served = set()
    for c, (k, nv) in zip(cases, got):
        B, HW, C, G, ldx, ldy, al, floor = c
        assert k == GR.gn_resident_plan(*c), c
        ks = brute_ks(HW, C, G)
        want = brute_choice(ks) if B * HW * C > floor else 0
        assert k == want, (c, k, ks)
        assert nv == (GR.gn_resident_nv(HW, C, G, k) if k else 0)
        if k:
            assert 1 <= nv <= 22 and (k * (C // G)) % 8 == 0 and G % k == 0
            served.add((HW, C))
    # the 224x400 program: every site is served at 576 views; level 0 (1400 px) runs the blocks of the design table
    for (HW, C, G, ldx, ldy) in site_shapes(plans[(28, 50)]):
        assert GR.gn_resident_plan(576, HW, C, G, ldx, ldy, 16) > 0, (HW, C)
    assert GR.gn_resident_plan(576, 1400, 320, 32, 320, 320, 16) == 8          # cpg 10: 160-byte rows, 224 KB, 14 vectors per thread
    assert GR.gn_resident_plan(576, 1400, 640, 32, 640, 640, 16) == 4          # cpg 20: 160-byte rows, 224 KB
    assert GR.gn_resident_plan(576, 1400, 960, 32, 960, 960, 16) == 4          # cpg 30: 240-byte rows, 336 KB, 21 vectors per thread
    assert GR.gn_resident_nv(1400, 960, 32, 4) == 21 and GR.gn_resident_nv(1400, 320, 32, 8) == 14
    # the deeper levels have a block of <= 4 vectors per thread: two workgroups per CU (the k the per-site sweep measured fastest)
    for HW, C, k in ((350, 320, 8), (350, 640, 4), (350, 1280, 2), (91, 640, 16), (91, 1280, 8), (91, 1920, 4), (91, 2560, 4), (28, 1280, 16), (28, 2560, 8)):
        assert GR.gn_resident_plan(576, HW, C, 32, C, C, 16) == k and GR.gn_resident_nv(HW, C, 32, k) <= 4, (HW, C)
    assert GR.gn_resident_plan(576, 350, 960, 32, 960, 960, 16) == 16 and GR.gn_resident_plan(576, 350, 1920, 32, 1920, 1920, 16) == 8      # none: the widest
    # 432x768, level 0 (5184 px): 320 channels need k % 4 == 0 -> at least 26 vectors per thread: not served; the deeper levels are
    assert GR.gn_resident_plan(576, 5184, 320, 32, 320, 320, 16) == 0
    assert (1296, 640) in served


def test_largest_slab_that_fits_and_first_that_does_not(header):
    # C = 320, G = 32 (cpg 10): k = 8 holds 22 x 102 rows, k = 4 (the narrowest aligned block) 22 x 204 rows
    cases = [(64, HW, 320, 32, 320, 320, 16, 0) for HW in (2244, 2245, 4488, 4489)]
    got, _ = header(cases)
    assert [k for k, _ in got] == [8, 4, 4, 0] == [GR.gn_resident_plan(*c) for c in cases]
    assert [nv for _, nv in got] == [22, 12, 22, 0]
    # C = 960 (cpg 30): k = 4 -> 15 vectors per row, 68 rows per pass
    cases = [(64, HW, 960, 32, 960, 960, 16, 0) for HW in (22 * 68, 22 * 68 + 1)]
    got, _ = header(cases)
    assert [k for k, _ in got] == [4, 0] == [GR.gn_resident_plan(*c) for c in cases]


@pytest.mark.parametrize("cpg,mult,widest", [(10, 4, 32), (20, 2, 32), (30, 4, 32), (40, 1, 16), (60, 2, 16), (80, 1, 8)])
def test_k_alignment_rule(header, cpg, mult, widest):
    """k * cpg * 2 bytes must be a multiple of 16: k a multiple of `mult`; one pixel row always fits, so HW = 1 gives the widest block
    (at most 1024 channels)."""
    C = 32 * cpg
    for k in (1, 2, 4, 8, 16, 32):
        ok = k % mult == 0 and k * cpg <= 1024
        assert bool(GR.gn_resident_nv(1, C, 32, k)) == ok, (cpg, k)
    c = (8, 1, C, 32, C, C, 16, 0)
    got, _ = header([c])
    assert got[0][0] == widest == GR.gn_resident_plan(*c)


def test_conditions_that_refuse(header):
    base = dict(B=576, HW=350, C=640, G=32, ldx=640, ldy=640, al=16, floor=FLOOR)
    def case(**kw):
        d = dict(base, **kw)
        return (d["B"], d["HW"], d["C"], d["G"], d["ldx"], d["ldy"], d["al"], d["floor"])
    cases = [case(), case(ldx=644), case(ldy=1284), case(ldx=1288, ldy=1920), case(al=8), case(al=2), case(ldx=632), case(C=630), case(C=128, ldx=128, ldy=128),
             case(C=288, ldx=288, ldy=288), case(B=18, HW=350, C=640), case(B=19), case(B=18, floor=0), case(HW=1 << 22, ldx=640), case(G=0)]
    want = [4, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 4, 4, 0, 0]
    got, _ = header(cases)
    assert [k for k, _ in got] == want == [GR.gn_resident_plan(*c) for c in cases]
    # 18 x 350 x 640 = 4 032 000 <= 4 Mi elements: the one-launch kernel keeps it; 19 images are above the floor


def test_cpu_plans_hold_no_resident_op(plans):
    cfg = spec.TINY_CONFIG
    usd = spec.random_state_dict(spec.unet_param_shapes(cfg), 0)
    tiny = DN.UNetPlan(cfg, PackedNet(usd, CPU), CPU, 6, 8, (28, 50))
    assert any(isinstance(op, O.GroupNorm) for op in tiny.ops) and not any(isinstance(op, O.GroupNormResident) for op in tiny.ops)
    for plan in plans.values():
        assert not any(isinstance(op, O.GroupNormResident) for op in plan.step_ops)


def test_forced_plan_same_count_same_flops(plans):
    base = plans[(28, 50)]
    forced = sd15_plan((28, 50), mode=2)
    assert len(forced.step_ops) == len(base.step_ops)
    kinds = lambda p: [O.GroupNorm if isinstance(op, O.GroupNorm) else type(op) for op in p.step_ops]
    assert kinds(forced) == kinds(base)
    n_res = sum(isinstance(op, O.GroupNormResident) for op in forced.step_ops)
    n_gn = sum(isinstance(op, O.GroupNorm) for op in base.step_ops)
    assert n_res == n_gn > 50, (n_res, n_gn)           # mode 2: every site of the 224x400 program is served
    fb, ff = flops.program_flops(base.step_ops), flops.program_flops(forced.step_ops)
    assert fb == ff and abs(ff["total"] / 1e12 - 2.298) < 0.01
    assert sum(flops.op_bytes(op) for op in forced.step_ops) == sum(flops.op_bytes(op) for op in base.step_ops)
    for a, b in zip(base.step_ops, forced.step_ops):
        assert flops.kernel_family(a) == flops.kernel_family(b)
    for op in forced.step_ops:
        if isinstance(op, O.GroupNormResident):
            code, d = op.lower()
            assert code == 15 and d.C == op.X.shape[2]
    # mode 1 at one scene (12 views through the nets): only the tensors above the one-launch floor change
    by_rule = sd15_plan((28, 50), mode=1)
    for op in by_rule.step_ops:
        if isinstance(op, O.GroupNorm):
            B, HW, C = op.X.shape
            assert isinstance(op, O.GroupNormResident) == (B * HW * C > FLOOR), (B, HW, C)
