// stats.hip — mdx_group_stats_*: per-group sample-health record of a tensor, in one pass, without atomics and without a host sync.
//
// Input: G groups of n contiguous elements, group g at X + g * sG (fp32, or the 16-bit type of the build).  Output, per group, four fp32:
//     {nonfinite, absmax, sum, sumsq}
//   nonfinite  number of NaN / +-Inf elements (an integer count, converted once at the end: exact, n <= 2^24)
//   absmax     largest |x| over the FINITE elements (0 without one): an integer maximum over the sign-cleared fp32 bit patterns — bit-exact
//   sum, sumsq sum of x and of x * x over the finite elements, fp32 accumulation (x * x enters through one fma: a single rounding per term)
// A non-finite element is recognised by its EXPONENT BITS (all ones) and its bit pattern is replaced by +0 before any arithmetic, so the
// record does not depend on how the compiler treats NaN / Inf comparisons (-ffast-math, -ffinite-math-only).
//
// Reduction order (fixed: the bits of a record depend on the group's n elements only, never on G, the other groups or the launch):
//   one workgroup of T = 256 threads per group.  V = elements of one 16-byte piece (4 fp32 / 8 16-bit); P = n / V full pieces.
//   1. thread t owns pieces t, t + T, t + 2T, ... and keeps V accumulators: acc[j] += element j of every piece, in piece order;
//   2. acc[0..V) are combined as a balanced tree (((a0 + a1) + (a2 + a3)) + ...);
//   3. the n % V tail elements (index P * V + r) are loaded as scalars: thread r adds element P * V + r to its value;
//   4. wave-64 butterfly: 6 levels of v += shfl_xor(v, 32 / 16 / 8 / 4 / 2 / 1) — commutative, so every lane holds the same bits;
//   5. the 4 wave values go through LDS; thread 0 adds them as (w0 + w1) + (w2 + w3) and stores the record with one 16-byte store.
//   The vector path (16-byte loads) needs 16-byte-aligned group starts; any other alignment takes the SAME order with scalar loads.
//
// Longest addition chain, i.e. the most fp32 roundings between an input and the stored sum:
//     k(n) = ceil(ceil(n / V) / 256) + log2(V) + 1 + 6 + 2        (V = 4: fp32 input, V = 8: 16-bit input)
//            own pieces              tree    tail  wave  LDS
//   so |sum - exact| <= k(n) * 2^-24 * sum|x| and |sumsq - exact| <= k(n) * 2^-24 * sum x^2 to first order (tests/test_group_stats_gpu.py).
//   sumsq overflows to +Inf above ~1.8e19 per element; absmax is the field to threshold on.
//
// Row select: row = row_dev ? *row_dev : 0 is read when the kernel RUNS (a replayed hipGraph sees the current value, as MdxDdimDesc.step_ptr);
// the records go to out + (row * G + g) * 4; a row outside [0, n_rows) writes nothing.
//
// Cost: one read of the tensor.  A workgroup keeps 4 x 16-byte loads per thread in flight (16 KiB per CU); at the decoded-image size
// (224 * 400 * 3 16-bit elements per view) a thread walks 132 pieces.
#include "common.h"
#include "launch.h"

namespace mdx {

#define GS_T 256

#if MDX_F16
#define GS_EXP16 0x7C00u
#else
#define GS_EXP16 0x7F80u
#endif

struct StatsParams { const void* X; float* out; const int* row_dev; long sG; int n; int n_rows; int G; };

struct GsAcc {
    float s, q;
    unsigned amax;
    int bad;
};

// one fp32 bit pattern into (sum, sumsq) accumulators, the absmax bits and the non-finite count
__device__ __forceinline__ void gs_take(unsigned bits, float& s, float& q, unsigned& amax, int& bad) {
    const bool nf = (bits & 0x7F800000u) == 0x7F800000u;
    bad += nf ? 1 : 0;
    bits = nf ? 0u : bits;
    const unsigned a = bits & 0x7FFFFFFFu;
    amax = a > amax ? a : amax;
    const float x = __uint_as_float(bits);
    s += x;
    q = __builtin_fmaf(x, x, q);
}
// fp32 bit pattern of a 16-bit element; a non-finite one (exponent bits all ones in ITS format) becomes a non-finite fp32 pattern
__device__ __forceinline__ unsigned gs_bits16(unsigned h) {
    h &= 0xFFFFu;
    if ((h & GS_EXP16) == GS_EXP16) return 0x7F800000u;
    return __float_as_uint(bf2f((bf16_t)h));
}

template <bool F32, bool VEC>
__global__ __launch_bounds__(GS_T) void group_stats_kernel(StatsParams p) {
    constexpr int V = F32 ? 4 : 8;
    const int row = p.row_dev ? *p.row_dev : 0;
    if (row < 0 || row >= p.n_rows) return;                     // uniform over the launch: nothing is written
    const int t = threadIdx.x;
    const long g = blockIdx.x;
    const int n = p.n;
    const int P = n / V;
    const float* xf = (const float*)p.X + g * p.sG;
    const bf16_t* xh = (const bf16_t*)p.X + g * p.sG;

    float s[V], q[V];
    unsigned amax = 0;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) { s[j] = 0.f; q[j] = 0.f; }

    // piece `pc` (< P, so its V elements lie inside the group) as V fp32 bit patterns
    auto load_piece = [&](int pc, unsigned (&b)[V]) {
        if (F32) {
            if (VEC) {
                const uint4 u = *reinterpret_cast<const uint4*>(xf + (long)pc * 4);
                b[0] = u.x; b[1] = u.y; b[2] = u.z; b[3] = u.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = __float_as_uint(xf[(long)pc * 4 + j]);
            }
        } else {
            if (VEC) {
                const uint4 u = *reinterpret_cast<const uint4*>(xh + (long)pc * 8);
                const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) { b[2 * j] = gs_bits16(w[j]); b[2 * j + 1] = gs_bits16(w[j] >> 16); }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) b[j] = gs_bits16(xh[(long)pc * 8 + j]);
            }
        }
    };
    int pc = t;
    for (; pc + 3 * GS_T < P; pc += 4 * GS_T) {                 // four loads in flight, consumed in piece order
        unsigned b0[V], b1[V], b2[V], b3[V];
        load_piece(pc, b0); load_piece(pc + GS_T, b1); load_piece(pc + 2 * GS_T, b2); load_piece(pc + 3 * GS_T, b3);
#pragma unroll
        for (int j = 0; j < V; ++j) gs_take(b0[j], s[j], q[j], amax, bad);
#pragma unroll
        for (int j = 0; j < V; ++j) gs_take(b1[j], s[j], q[j], amax, bad);
#pragma unroll
        for (int j = 0; j < V; ++j) gs_take(b2[j], s[j], q[j], amax, bad);
#pragma unroll
        for (int j = 0; j < V; ++j) gs_take(b3[j], s[j], q[j], amax, bad);
    }
    for (; pc < P; pc += GS_T) {
        unsigned b0[V];
        load_piece(pc, b0);
#pragma unroll
        for (int j = 0; j < V; ++j) gs_take(b0[j], s[j], q[j], amax, bad);
    }
    // balanced tree over the V accumulators
#pragma unroll
    for (int w = 1; w < V; w *= 2)
#pragma unroll
        for (int j = 0; j < V; j += 2 * w) { s[j] += s[j + w]; q[j] += q[j + w]; }
    float sum = s[0], sq = q[0];
    // tail: element P * V + t for t < n % V (scalar loads; the last one is element n - 1)
    if (t < n - P * V) {
        const long i = (long)P * V + t;
        const unsigned b = F32 ? __float_as_uint(xf[i]) : gs_bits16(xh[i]);
        gs_take(b, sum, sq, amax, bad);
    }
    // wave-64 butterfly
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        sq += __shfl_xor(sq, o, 64);
        const unsigned oa = (unsigned)__shfl_xor((int)amax, o, 64);
        amax = oa > amax ? oa : amax;
        bad += __shfl_xor(bad, o, 64);
    }
    __shared__ float l_sum[GS_T / 64], l_sq[GS_T / 64];
    __shared__ unsigned l_amax[GS_T / 64];
    __shared__ int l_bad[GS_T / 64];
    const int wave = t >> 6;
    if ((t & 63) == 0) { l_sum[wave] = sum; l_sq[wave] = sq; l_amax[wave] = amax; l_bad[wave] = bad; }
    __syncthreads();
    if (t == 0) {
        const float S = (l_sum[0] + l_sum[1]) + (l_sum[2] + l_sum[3]);
        const float Q = (l_sq[0] + l_sq[1]) + (l_sq[2] + l_sq[3]);
        unsigned A = l_amax[0];
#pragma unroll
        for (int w = 1; w < GS_T / 64; ++w) A = l_amax[w] > A ? l_amax[w] : A;
        const int Bd = (l_bad[0] + l_bad[1]) + (l_bad[2] + l_bad[3]);
        float4 rec;
        rec.x = (float)Bd; rec.y = __uint_as_float(A); rec.z = S; rec.w = Q;
        *reinterpret_cast<float4*>(p.out + ((long)row * p.G + g) * 4) = rec;
    }
}

}  // namespace mdx

using namespace mdx;

extern "C" int mdx_group_stats_bf16(const MdxStatsDesc* d, void* stream) {
    const char* op = "mdx_group_stats";
    if (!d || !d->X || !d->out) return set_error(MDX_EINVAL, "%s: null operand", op);
    if (d->f32 != 0 && d->f32 != 1) return set_error(MDX_EINVAL, "%s: f32=%ld must be 0 (the 16-bit type of the build) or 1 (fp32)", op, (long)d->f32);
    if (d->n < 0 || d->n > (1L << 24)) return set_error(MDX_EINVAL, "%s: n=%ld must be in [0, 2^24] (the non-finite count is stored as fp32)", op, (long)d->n);
    if (d->G < 0) return set_error(MDX_EINVAL, "%s: G=%ld must not be negative", op, (long)d->G);
    MDX_NEED(need_int(op, "G", d->G));
    if (d->sG < 0) return set_error(MDX_EINVAL, "%s: sG=%ld must not be negative", op, (long)d->sG);
    MDX_NEED(need_aligned(op, "X", d->X, d->f32 ? 4 : 2));
    MDX_NEED(need_aligned(op, "out", d->out, 16));
    if (d->row_dev) {
        MDX_NEED(need_aligned(op, "row_dev", d->row_dev, 4));
        MDX_NEED(need_int(op, "n_rows", d->n_rows));
        if (d->n_rows < 1) return set_error(MDX_EINVAL, "%s: n_rows=%ld must be >= 1 with row_dev", op, (long)d->n_rows);
    }
    if (d->G == 0 || d->n == 0) return MDX_OK;
    StatsParams p{d->X, d->out, d->row_dev, d->sG, (int)d->n, d->row_dev ? (int)d->n_rows : 1, (int)d->G};
    const int es = d->f32 ? 4 : 2;
    const bool vec = ((uintptr_t)d->X & 15) == 0 && (d->G == 1 || (d->sG * es) % 16 == 0);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)d->G), block(GS_T);
    if (d->f32) {
        if (vec) hipLaunchKernelGGL((group_stats_kernel<true, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((group_stats_kernel<true, false>), grid, block, 0, st, p);
    } else {
        if (vec) hipLaunchKernelGGL((group_stats_kernel<false, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((group_stats_kernel<false, false>), grid, block, 0, st, p);
    }
    return check_launch(vec ? "group_stats_kernel" : "group_stats_kernel_scalar");
}
