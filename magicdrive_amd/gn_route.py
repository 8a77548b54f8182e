"""Python mirror of csrc/gn_route.h: does the register-resident GroupNorm (ops.GroupNormResident, gn_resident_kernel) take a tensor,
and with how many groups per workgroup?  engine.Builder.groupnorm asks it when it builds a plan; the library asks the header when the op
runs.  tests/test_gn_resident_cpu.py compiles the header and compares the two on every site shape."""
from __future__ import annotations

GNR_THREADS = 1024
GNR_MAX_NV = 22
GNR_MAX_CH = 1024
GNR_MAX_K = 32
GNR_PAIR_NV = 4
GNR_ONE_KERNEL_ELEMS = 4 << 20


def gn_resident_nv(HW: int, C: int, G: int, k: int) -> int:
    """Vectors per thread when a workgroup takes k groups of an HW x C map with G groups, or 0 when it cannot."""
    if HW <= 0 or C <= 0 or G <= 0 or C % G or k <= 0 or k > GNR_MAX_K or G % k:
        return 0
    cpg = C // G
    ch = k * cpg
    if cpg < 8 or cpg % 2 or ch % 8 or ch > GNR_MAX_CH:
        return 0
    vpr = ch // 8
    rpp = GNR_THREADS // vpr
    nv = (HW + rpp - 1) // rpp
    return nv if nv <= GNR_MAX_NV else 0


def gn_resident_plan(B: int, HW: int, C: int, G: int, ldx: int, ldy: int, alignment: int, min_elems: int = GNR_ONE_KERNEL_ELEMS) -> int:
    """k (groups per workgroup) the resident kernel runs [B][HW][C] at, or 0: not served / not worth it."""
    if B <= 0 or HW <= 0 or C <= 0 or G <= 0 or C % G:
        return 0
    if ldx < C or ldy < C or ldx % 8 or ldy % 8 or alignment < 16:
        return 0
    if HW * max(ldx, ldy) >= (1 << 31) or B > 0x7fffffff // G:
        return 0
    if B * HW * C <= min_elems:
        return 0
    ks = range(min(G, GNR_MAX_K), 0, -1)
    for k in ks:                       # two workgroups per CU: the widest block of at most GNR_PAIR_NV vectors per thread
        if 0 < gn_resident_nv(HW, C, G, k) <= GNR_PAIR_NV:
            return k
    for k in ks:                       # else the widest block that fits
        if gn_resident_nv(HW, C, G, k):
            return k
    return 0
