// gn_route.h — does the register-resident GroupNorm (norm.hip: gn_resident_kernel) take a tensor, and with how many groups per workgroup?
//
// Free of HIP types (plain g++ compiles it): tests/test_gn_resident_cpu.py builds a small program against this header and compares it with the
// Python mirror magicdrive_amd/gn_route.py on every site shape; mdx_groupnorm_resident_* only EXECUTES the k it gets back.
//
// The kernel: one 1024-thread workgroup per (image, block of k groups).  The block's HW x (k * C/G) slab is loaded ONCE into registers
// (16 bytes per load), reduced to the k means, then to the k centred sums of squares, normalised and stored: the tensor crosses memory
// twice (read, write) where gn_stats_kernel + gn_apply_kernel cross it three times.  Thread layout: a row of the slab is vpr = k * cpg / 8
// 16-byte vectors; thread t owns vector column t % vpr of the rows t / vpr, t / vpr + rpp, ... (rpp = 1024 / vpr rows per pass), so the
// channels — hence the groups — of a thread's vectors never change, and nv = ceil(HW / rpp) vectors per thread hold the slab.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define MDX_GN_ROUTE_HD __host__ __device__ __forceinline__
#else
#define MDX_GN_ROUTE_HD inline
#endif

namespace mdx_route {

constexpr int GNR_THREADS = 1024;      // one workgroup per CU: 16 waves, 128 VGPRs per lane
constexpr int GNR_MAX_NV = 22;         // 16-byte vectors a thread may hold (88 of its 128 VGPRs: 24 spill to scratch; the largest site slab, 1400 px x 120 channels, needs 21)
constexpr int GNR_MAX_CH = 1024;       // channels per workgroup (k * cpg): one gamma / beta per thread, the scale / shift tables in LDS; row segments up to 2 KB
constexpr int GNR_MAX_K = 32;          // groups per workgroup (the per-group statistics in LDS)
constexpr int GNR_PAIR_NV = 4;         // up to this many vectors per thread the kernel needs <= 64 VGPRs: TWO workgroups share a CU
constexpr long GNR_ONE_KERNEL_ELEMS = 4L << 20;      // default of the option GN_ONE_KERNEL_ELEMS (options.h)

// vectors per thread when a workgroup takes k groups of an HW x C map with G groups, or 0 when it cannot
MDX_GN_ROUTE_HD int gn_resident_nv(long HW, long C, long G, long k) {
    if (HW <= 0 || C <= 0 || G <= 0 || C % G || k <= 0 || k > GNR_MAX_K || G % k) return 0;
    const long cpg = C / G, ch = k * cpg;
    // a 16-byte vector may straddle two groups, never three (cpg >= 8), and a channel pair never does (cpg even); whole vectors per row and per block (ch % 8)
    if (cpg < 8 || cpg % 2 || ch % 8 || ch > GNR_MAX_CH) return 0;
    const long vpr = ch / 8, rpp = GNR_THREADS / vpr;
    const long nv = (HW + rpp - 1) / rpp;
    return nv <= GNR_MAX_NV ? (int)nv : 0;
}

// k (groups per workgroup) the resident kernel runs [B][HW][C] at, or 0: not served / not worth it.
//   alignment   largest power of two (bytes, capped wherever the caller likes >= 16) dividing both X and Y
//   min_elems   tensors of at most this many elements stay on the one-launch kernel (GN_ONE_KERNEL_ELEMS; 0 with GN_RESIDENT = 2)
// Choice of k: the widest block of at most GNR_PAIR_NV vectors per thread when there is one — two workgroups per CU, one's loads and stores
// under the other's arithmetic — else the widest block that fits (the longest contiguous row segments, k * cpg * 2 bytes per pixel row).
// Measured per site with every k (tools/gn_bench.py --sweep-k, profiles/gn_resident_sweep.json): the fastest k of every site of the 224x400
// step program at 576 and at 192 views is the one this rule gives, or within the spread of it.
MDX_GN_ROUTE_HD int gn_resident_plan(long B, long HW, long C, long G, long ldx, long ldy, long alignment, long min_elems = GNR_ONE_KERNEL_ELEMS) {
    if (B <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % G) return 0;
    if (ldx < C || ldy < C || ldx % 8 || ldy % 8 || alignment < 16) return 0;              // 16-byte loads / stores of every row segment
    const long ldm = ldx > ldy ? ldx : ldy;
    if (HW * ldm >= (1L << 31) || B > 0x7fffffffL / G) return 0;                            // 32-bit pixel offsets inside an image, 32-bit grid
    if (B * HW * C <= min_elems) return 0;                                                  // the one-launch kernel wins below (norm.hip)
    const long kmax = G < GNR_MAX_K ? G : GNR_MAX_K;
    for (long k = kmax; k >= 1; --k) {
        const int nv = gn_resident_nv(HW, C, G, k);
        if (nv && nv <= GNR_PAIR_NV) return (int)k;
    }
    for (long k = kmax; k >= 1; --k)
        if (gn_resident_nv(HW, C, G, k)) return (int)k;
    return 0;
}

}  // namespace mdx_route
