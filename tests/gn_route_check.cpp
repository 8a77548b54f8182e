// Evaluates magicdrive_amd/csrc/gn_route.h on the CPU (tests/test_gn_resident_cpu.py builds this with g++).
// stdin: one case per line, "B HW C G ldx ldy alignment min_elems"; stdout: "k nv" per case (nv = vectors per thread at that k, 0 with k = 0).
#include <cstdio>
#include "../magicdrive_amd/csrc/gn_route.h"

int main() {
    long B, HW, C, G, ldx, ldy, al, me;
    while (std::scanf("%ld %ld %ld %ld %ld %ld %ld %ld", &B, &HW, &C, &G, &ldx, &ldy, &al, &me) == 8) {
        const int k = mdx_route::gn_resident_plan(B, HW, C, G, ldx, ldy, al, me);
        std::printf("%d %d\n", k, k ? mdx_route::gn_resident_nv(HW, C, G, k) : 0);
    }
    std::printf("consts %d %d %d %d %d %ld\n", mdx_route::GNR_THREADS, mdx_route::GNR_MAX_NV, mdx_route::GNR_MAX_CH, mdx_route::GNR_MAX_K,
                mdx_route::GNR_PAIR_NV, mdx_route::GNR_ONE_KERNEL_ELEMS);
    return 0;
}
