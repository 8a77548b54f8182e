/*
 * mdx.h — C-ABI of libmdx.so, the MI355X (gfx950) kernel library behind
 * magicdrive_amd's drop-in for MagicDrive's per-step denoiser.
 *
 * Boundary: the reference has no FFI of its own — its hot path is
 * Python calling torch ATen / xformers.  The lowest replaceable interface is
 *   - xformers.ops.memory_efficient_attention(q, k, v, attn_bias, p, scale, op)
 *       third_party/xformers/xformers/ops/fmha/__init__.py:115-196, called from
 *       third_party/diffusers/src/diffusers/models/attention_processor.py:1165-1171
 *   - ATen conv2d / addmm / native_group_norm / native_layer_norm / gelu / silu as
 *       invoked by third_party/diffusers/src/diffusers/models/{resnet.py:590-640,
 *       attention.py:259-280, transformer_2d.py:276-315, embeddings.py:24-64}
 *   - the scheduler update third_party/diffusers/src/diffusers/schedulers/
 *       scheduling_ddim.py:325-445 and CFG combine magicdrive/pipeline/
 *       pipeline_bev_controlnet.py:426-431.
 * Every entry point below replaces one of those call sites (cited per function).
 *
 * Conventions
 *   - plain C: pointers, 64-bit integers and doubles only; no torch types.  Every
 *     descriptor field is 8 bytes wide so a ctypes.Structure mirrors it 1:1.
 *   - all device pointers are caller-owned HBM; nothing is allocated or freed here
 *     except graph handles; no implicit synchronisation: work is enqueued on the
 *     hipStream_t passed as `stream` (void*), so calls are hipGraph-capturable.
 *   - activations are channels-last: a feature map is [B][H][W][C] == a token
 *     matrix [B*H*W][C]; "ld*" are row (pixel/token) strides in ELEMENTS.
 *   - bf16 = upper 16 bits of IEEE fp32, round-to-nearest-even on store; all
 *     accumulation, softmax, normalisation statistics and scheduler math in fp32.
 *   - return 0 on success, negative MDX_E* otherwise; never throws.
 *     mdx_last_error() returns a thread-local message for the last failure.
 */
#ifndef MDX_H_
#define MDX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDX_OK 0
#define MDX_EINVAL (-1)      /* bad descriptor (shape/alignment/unsupported size) */
#define MDX_ELAUNCH (-2)     /* hip launch / runtime error */
#define MDX_EUNSUPPORTED (-3)

#define MDX_ABI_VERSION 12

/* ---- epilogue flags shared by GEMM / conv ------------------------------- */
#define MDX_EPI_NONE 0
#define MDX_EPI_GEGLU 1      /* W rows interleaved [32 value | 32 gate]; C has N/2 cols:
                                C = value * gelu_erf(gate)   (attention.py:259-280) */
#define MDX_EPI_SILU 2       /* C = silu(acc + bias)  (map_embedder.py:66-76, bbox_embedder.py:145-152) */

/*
 * mdx_gemm_bf16 — C[M,N] = epi(A[M,K] · W[N,K]^T + bias[N] + temb[row(m),N]) + R[M,N]
 * Replaces ATen addmm/mm for every nn.Linear on the path and every 1x1 conv
 * (attention_processor.py:141-157 to_q/k/v/out, attention.py:200-216 FeedForward,
 * transformer_2d.py:155-165 proj_in/out, blocks.py:81-83 connector,
 * unet_addon_rawbox.py:221-272 zero-convs).
 * batch > 1: independent problems, pointer p advances by s*[batch index] elements
 * (used to emit V^T = W_v · X_b^T per view with sA = 0).
 * temb: optional fp32 table; row added to output row m is
 *        temb[sel*temb_sel_stride + (m / rows_per_b)*temb_b_stride + n]
 * where sel = *sel_ptr (device int32, 0 if null) — lets a captured graph pick the
 * current step's row of a table precomputed for all DDIM steps.
 * splitk: 0 = let the library choose (it splits K for small-M/huge-K shapes so the launch fills
 * 256 CUs), 1 = never, >1 = forced.  Splitting needs ws: fp32 [splitk][M][N] scratch of ws_bytes.
 * Requirements (each checked on the host before anything is launched; a violation returns MDX_EINVAL and mdx_last_error() names the field):
 *   - M, N, K, batch, rows_per_b, splitk fit a 32-bit int.
 *   - K % 8 == 0; lda % 8 == 0 and ldw % 8 == 0; A and W 16-byte aligned (rows are read as 16-byte pieces).
 *   - ldc % 4 == 0 and ldr % 4 == 0; C and R 8-byte aligned (16-bit C / R move as 8-byte pieces; the 16-byte epilogue is taken only when
 *     N % 8 == 0, ldc, ldr, sC, sR % 8 == 0 and both pointers are 16-byte aligned — anything less is SERVED by the 8-byte epilogue).
 *   - c_is_f32: C and R must be 16-byte aligned (fp32 rows move as float4, also in the split-K reduction).
 *   - bias and temb must be 16-byte aligned, temb_sel_stride % 4 == 0 and temb_b_stride % 4 == 0 (read as float4); sel_ptr 4-byte aligned.
 *   - ws must be 16-byte aligned (the split-K slabs are read as float4).  ws_bytes too small for the slabs reduces or disables the split
 *     (SERVED); a split with ws_bytes > 0 and ws == NULL is refused.
 *   - batch > 1: sA % 8 == 0, sW % 8 == 0, sC % 4 == 0, sR % 4 == 0.
 *   - N % 4 != 0 needs a plain epilogue (no bias / temb / R / epilogue / forced split-K) and ldc >= roundup4(N).
 *   - MDX_EPI_GEGLU needs N % 64 == 0.
 */
typedef struct MdxGemmDesc {
    const void* A; const void* W; void* C; const void* R;
    const float* bias; const float* temb; const int32_t* sel_ptr; float* ws;
    int64_t M, N, K;
    int64_t lda, ldw, ldc, ldr;
    int64_t batch, sA, sW, sC, sR;
    int64_t temb_sel_stride, temb_b_stride, rows_per_b;
    int64_t epilogue, splitk;
    int64_t c_is_f32;           /* 1: C (and R) are fp32 instead of bf16 */
    int64_t ws_bytes;           /* size of ws; split-K is reduced (or disabled) to fit */
    /* Optional transposed second output (fused q/k/v projection: the attention kernel wants V^T[view][channel][token]):
     * raw columns n >= vt_from are NOT written to C but to Vt[b][n - vt_from][t] with b = m / vt_T, t = m % vt_T
     * (element strides vt_stride per view, vt_ld per channel).  C then has vt_from columns.  Needs K == 320, vt_from % 128 == 0,
     * vt_T % 8 == 0, M % 8 == 0, 16-byte aligned Vt rows, no bias / epilogue on those columns (diffusers' to_v has none) —
     * it is implemented by the weight-stationary kernel only; anything else is rejected with MDX_EINVAL.  That kernel reads A through one
     * 2 GiB window: with Vt the whole extent of A, M * lda * 2 bytes, must stay below 0x7FFF0000 (3.35 M rows of 320), else MDX_EINVAL.
     * (Without Vt there is no such limit: a K = 320 GEMM whose A is longer runs on a main loop that rebases per tile.)  Vt = NULL: off. */
    void* Vt;
    int64_t vt_from, vt_T, vt_ld, vt_stride;
    /* Optional LayerNorm of the A rows, fused into the projection that consumes them (BasicTransformerBlock: norm1 -> attn1.to_q/k/v,
     * norm2 -> attn2.to_q, attention.py:85-120; BasicMultiviewTransformerBlock norm4 -> attn4, blocks.py:190-205).  ln_eps > 0: A holds
     * the RAW rows (K = the whole row); the caller has folded the affine part into the operands,
     *     W' = W diag(gamma),  bias' = bias + W beta,  ln_csum[n] = sum_k W'[n][k]   (sum of the 16-bit W' values, fp32),
     * and the result is  C[m][n] = rstd_m (sum_k A[m][k] W'[n][k] - mean_m ln_csum[n]) + bias'[n]  (+ R) with mean / rstd of row m over K
     * (biased variance, as torch.nn.LayerNorm).  The K = 320 weight-stationary kernel takes the statistics from the rows it streams
     * (the tokens are read once; no normalised copy exists); every other route first writes (A - mean) rstd to ln_scratch ([M][lda]
     * 16-bit, 16-byte aligned) and multiplies that — same weights, same result up to the rounding of the normalised copy.
     * The fused route takes a plain epilogue (optionally Vt); one batch, no split-K.  ln_eps = 0: off. */
    double ln_eps;
    const float* ln_csum;
    void* ln_scratch;
    /* Row statistics out of the PRODUCER's epilogue (ABI 9).  The LayerNorms of a transformer block normalise tensors that a
     * C x C projection has just written (proj_in -> norm1, attn1.to_out + residual -> norm2, attn2.to_out + residual -> norm4 / norm3,
     * connector(attn4.to_out) + residual -> norm3: attention.py:123-200, blocks.py:190-222).  rowstat_out != NULL: besides C the GEMM writes
     *     rowstat_out[(p * M + m) * 2 + {0, 1}] = (sum, sum of squares) of the STORED values C[m][n] (rounded to the 16-bit type, residual added)
     * over the columns n of part p, for rowstat_parts parts that together cover [0, N); parts a route does not need are written as zeros, so a
     * consumer simply adds all parts.  Fixed summation order (deterministic).  Plain epilogue, one batch, 16-bit C, no Vt; rowstat_parts >= 1.
     * The K = 320 weight-stationary kernel emits them from its store phase (one part per 128-column tile); every other route runs a small
     * statistics kernel over C behind the GEMM (part 0 = the whole row).
     * ln_stats != NULL (with ln_eps > 0): the fused LayerNorm takes mean / rstd of row m from these sums — written by the producer of A through
     * its rowstat_out, ln_stats_parts parts of M rows — instead of recomputing them from the rows it streams (in every N-tile's workgroup: 8x for
     * a fused q/k/v projection).  With given statistics the GEGLU epilogue can carry the LayerNorm too (norm3 -> ff.net.0).  Routes that do not
     * normalise in-kernel ignore ln_stats and normalise into ln_scratch as before. */
    float* rowstat_out;
    int64_t rowstat_parts;
    const float* ln_stats;
    int64_t ln_stats_parts;
    /* Optional second copy of W in MFMA-fragment order (ABI 10), for the W-direct persistent kernel (csrc/gemm_xd.hip: the weights go
     * global -> registers past the LDS, the finished tile is stored under the next tile's main loop):
     *     Wq[n / 16][k / 32][lane][8]  with lane = ((k % 32) / 8) * 16 + n % 16,  element = W[n][k + (0..7)],
     * i.e. the 64 lanes' operands of one 16-column x 32-deep block are one contiguous KiB; N padded with zero blocks to a multiple of 256
     * (roundup(N, 256) * K elements; magicdrive_amd/packing.py: pack_wq).  GEGLU: W (and so Wq) rows in the [32 value | 32 gate] order.
     * The library uses it when the shape goes to the 256-wide persistent tile and K % 128 == 0, K >= 640 (plain / GEGLU epilogue, optional
     * residual, no temb / Vt / split-K); otherwise it is ignored and W is read.  W must be given either way.  NULL: off. */
    const void* Wq;
} MdxGemmDesc;
int mdx_gemm_bf16(const MdxGemmDesc* d, void* stream);

/*
 * mdx_conv2d_bf16 — channels-last implicit-GEMM convolution on MFMA:
 *   Y[b,oy,ox,co] = epi( Σ_{ky,kx,ci} X[b, oy*sh-ph+ky, ox*sw-pw+kx, ci] · Wt[co][ky][kx][ci]
 *                        + bias[co] + temb[b,co] ) + R[b,oy,ox,co]
 * Replaces ATen conv2d in ResnetBlock2D.conv1/conv2 (resnet.py:590-640, temb add :617-618,
 * residual add :638), Downsample2D (resnet.py:198-222), Upsample2D.conv (resnet.py:165-170),
 * the BEV map encoder (map_embedder.py:66-76).  Weights are pre-packed [Cout][kh][kw][Cin].
 * ldx/ldy/ldr: pixel strides in elements (a tensor may be a channel slice of a wider one).
 * Requirements (host-checked, MDX_EINVAL, the message names the field):
 *   - Cin % 8 == 0 (smaller Cin goes through mdx_conv2d_direct) and Cout % 4 == 0; no GEGLU epilogue.
 *   - every size field, Ho * Wo, B * Ho * Wo and kh * kw * Cin fit a 32-bit int.
 *   - ldx % 8 == 0, X and Wt 16-byte aligned; ldy % 4 == 0 and ldr % 4 == 0, Y and R 8-byte aligned (the 16-byte epilogue is taken when
 *     Cout, ldy, ldr % 8 == 0 and both are 16-byte aligned; less is served by the 8-byte one).
 *   - bias and temb must be 16-byte aligned, temb_sel_stride % 4 == 0, temb_b_stride % 4 == 0; sel_ptr 4-byte aligned; ws 16-byte aligned.
 */
typedef struct MdxConvDesc {
    const void* X; const void* Wt; void* Y; const void* R;
    const float* bias; const float* temb; const int32_t* sel_ptr; float* ws;
    int64_t B, Hi, Wi, Cin, Ho, Wo, Cout;
    int64_t kh, kw, sh, sw, ph, pw;
    int64_t ldx, ldy, ldr;
    int64_t temb_sel_stride, temb_b_stride;
    int64_t epilogue, splitk;
    int64_t ws_bytes;
    /* ABI 11 (the field was reserved1): 1 = "upsampled 2x" mode — Y = conv3x3_pad1(nearest_resize(X, Ho x Wo)) computed from the LOW-RES X
     * [B,Hi,Wi,Cin] without the resized tensor.  In the resized image every 2 x 2 block holds one pixel of X, so an output pixel's nine taps
     * read four pixels of X: per output parity ("phase") the 3x3 filter folds into a 2x2 one.  Per axis the output indices fall in classes
     *     0  even  o = 2 j      taps (j - 1, j)   weights (w0, w1 + w2)
     *     1  odd   o = 2 j + 1  taps (j, j + 1)   weights (w0 + w1, w2)
     *     2  the last even index when n_out = 2 n_in - 1 (its +1 tap is the conv's zero padding): taps (j - 1, j), weights (w0, w1)
     * with 2 classes on an exact-2x axis and 3 on a cropped one (classes 0 / 1 then stop one index earlier).
     * Wt = [ny * nx][Cout][2][2][Cin], set yc * nx + xc = the outer combination of the axis classes (magicdrive_amd/packing.py:
     * fold_upsample_conv); kh = kw = 2 describe one set, sh = sw = 1, ph / pw are ignored.
     * Needs Cin % 64 == 0, Ho in {2 Hi, 2 Hi - 1}, Wo in {2 Wi, 2 Wi - 1}, Hi * Wi + 256 < 2^24, on a cropped axis the whole extent of X (B * Hi * Wi * ldx * 2 bytes) below 2^31, and a bias-only epilogue (no R / temb /
     * activation / split-K): anything else is MDX_EINVAL — the mode has one route (csrc/gemm_xl.hip) and no fallback.  0 = ordinary conv. */
    int64_t upsample2x;
} MdxConvDesc;
int mdx_conv2d_bf16(const MdxConvDesc* d, void* stream);

/*
 * mdx_conv2d_direct — small-channel / odd-K convolution or linear on the vector ALU
 * (fp32 accumulate): conv_in (Cin=4, unet_2d_condition.py:262-265), conv_out (Cout=4, :497-500),
 * cam2token (K=189, unet_addon_rawbox.py:106), bbox_proj (K=216, bbox_embedder.py:72).
 * x_is_f32 / y_is_f32 select fp32 I/O (latents and eps stay fp32).
 * Served at every alignment: operands need only their element's natural alignment (2 bytes for 16-bit, 4 for fp32 X / Y / R / bias / temb /
 * sel_ptr); the 16-byte K-parallel kernels are taken for a 16-bit X (x_is_f32 == 0) when Cout <= 8, Cin % 8 == 0, ldx % 8 == 0, kh * kw * Cin >= 512 and X, Wt are 16-byte
 * aligned, the one-thread-per-output kernel otherwise.  Requirements (MDX_EINVAL): natural alignment as above; no GEGLU epilogue; every size
 * field, Ho * Wo, B * Ho * Wo and kh * kw * Cin must fit a 32-bit int.
 */
typedef struct MdxConvDirectDesc {
    const void* X; const void* Wt; void* Y; const void* R;
    const float* bias; const float* temb; const int32_t* sel_ptr; void* reserved_p;
    int64_t B, Hi, Wi, Cin, Ho, Wo, Cout;
    int64_t kh, kw, sh, sw, ph, pw;
    int64_t ldx, ldy, ldr;
    int64_t temb_sel_stride, temb_b_stride;
    int64_t epilogue, x_is_f32, y_is_f32, reserved0;
} MdxConvDirectDesc;
int mdx_conv2d_direct(const MdxConvDirectDesc* d, void* stream);

/*
 * mdx_attention_bf16 — fused softmax(Q K^T * scale) V, flash style (no T×T matrix in HBM).
 * Replaces xformers.ops.memory_efficient_attention (fmha/__init__.py:115-196; CUTLASS kernel
 * kernel_forward.h) / F.scaled_dot_product_attention (attention_processor.py:1193-1272) for
 * attn1 (self), attn2 (text+camera+box context) and attn4 (cross-view, blocks.py:106-222).
 *   Q : [B][Tq][..]  element (b,t,h,j) at Q + b*sQ + t*ldq + h*d + j
 *   K : [Bkv][Tk][..] same addressing with sK, ldk
 *   Vt: [Bkv][H*d][ldv]  V transposed — element (b,h,j,t) at Vt + b*sV + (h*d+j)*ldv + t
 *   O : [B][Tq][H*d] with sO, ldo
 * nsrc key/value sources per query batch: for query batch b they are the batches kvmap[b*nsrc + s] (identity if kvmap == NULL).
 *   joint == 0, nsrc ∈ {1,2}: every source has its own softmax and the normalised outputs are SUMMED — neighboring_attn_type "add",
 *     blocks.py:112-121, 213-217 (left + right neighbour; the doubled out-bias is the caller's business);
 *   joint == 1, nsrc ∈ {1..8}: ONE softmax over the concatenation of the sources' keys — "concat" (the two neighbours, blocks.py:122-134)
 *     and "self" (all cameras of the scene, blocks.py:135-138).
 *   Absent source slot (joint == 0 with a kvmap; camera rigs whose views have one neighbour or none — an open chain's end cameras, a camera
 *     that overlaps nobody): kvmap[b*nsrc + s] < 0 means "query batch b has no source in slot s".  O of b is the sum over the slots that are
 *     present; slot order does not matter ([a, -1] and [-1, a] give bit-identical O); with every slot absent (nsrc == 2: both, nsrc == 1: the
 *     one) every O row of b is written as zeros.  A negative entry was an out-of-bounds read before, so no valid caller changes (ABI 12 stays).
 *     Under joint == 1 a negative entry remains the caller's error (the reference's "concat" cannot be ragged: its torch.cat fails).
 * Requirements (host-checked, MDX_EINVAL, the message names the field):
 *   - d % 8 == 0, 0 < d <= 160.  Kernel instances exist for ceil(d / 16) in {1..6, 8, 10}, a ragged last 16-column chunk is masked:
 *     SUPPORTED d = 8 .. 96 (every multiple of 8), 120, 128, 152, 160;  d = 104, 112, 136, 144 return MDX_EUNSUPPORTED.
 *   - ldq, ldk, ldv, sQ, sK, sV must be multiples of 8 and Q, K, Vt 16-byte aligned (rows are read as 16-byte pieces); ldv >= Tk.
 *   - ldo % 4 == 0, sO % 4 == 0 and O must be 8-byte aligned (an O row is written as 8-byte pieces — ldo % 8 == 4 is served).
 *   - B, H, Tq, Tk fit a 32-bit int; joint must be 0 or 1; nsrc must be 1..2 (joint: 1..8); nsrc > 1 needs a kvmap (4-byte aligned);
 *     q_prescaled must be 0 or 1.
 * Short sequences, V row-major, causal mask (ABI 12; CLIP's text encoder, transformers/models/clip/modeling_clip.py: CLIPAttention with the
 * causal mask of CLIPTextTransformer — 77 tokens, 12 heads of 64).  With causal == 0 and v_rowmajor == 0 everything above holds unchanged.
 *   v_rowmajor == 1: the third operand is V itself, [Bkv][Tk][H*d] — element (b,t,h,j) at Vt + b*sV + t*ldv + h*d + j, ldv a token stride —
 *     so Q, K and V can be the three column blocks of one fused [M][3C] projection buffer.  One kernel serves it (csrc/attention_short.hip:
 *     one workgroup per (batch, head), the head's whole K and V in LDS, one softmax pass, V transposed by the LDS read):
 *       - SERVED: Tq <= 128, Tk <= 128 and d in {32, 64};  any other d, or a larger Tq / Tk, returns MDX_EUNSUPPORTED.
 *       - nsrc must be 1, joint 0, q_prescaled 0 (MDX_EINVAL, the message names the field); kvmap is ignored.
 *       - ldq, ldk, ldv, sQ, sK, sV multiples of 8, ldv >= H*d, Q, K, Vt 16-byte aligned; O as above.
 *   causal == 1: query t sees keys 0..t.  Needs v_rowmajor == 1 and Tq == Tk (MDX_EINVAL otherwise); causal must be 0 or 1.
 * Key count from device memory (tk_dev, the former reserved_p; the struct's size and layout are unchanged and NULL is the old contract, so the
 * ABI version stays 12).  For the text + camera + box context of a sampler plan built at a box capacity (the reference pads the boxes of every
 * batch to that batch's maximum, pipeline_bev_controlnet.py:330-343, so the context length differs from call to call).  With tk_dev == NULL
 * everything above holds unchanged, bit for bit.
 *   tk_dev != NULL: a device pointer to ONE int32, 4-byte aligned.  Tk is then the CAPACITY: K is valid for Tk rows, V^T for Tk columns
 *     (ldv >= Tk as above).  The kernel reads n = *tk_dev on the device when it RUNS - a replayed hipGraph sees the value current at
 *     replay - and queries attend to keys 0 .. n-1 only; what keys n .. Tk-1 and the V^T pad columns hold never reaches O (NaN included).
 *     The work done depends on n, not on Tk: the same n at two capacities gives bit-identical O.
 *       - n < 1 or n > Tk cannot be reported without a sync: n is clamped to [1, Tk] for addressing and EVERY O row is written as NaN.
 *       - SERVED (csrc/attention_ctx.hip): nsrc == 1, joint == 0, causal == 0, v_rowmajor == 0 - anything else returns MDX_EINVAL, the
 *         message names the field; kvmap is ignored.  q_prescaled may be 0 or 1; with 0, scale must be > 0 (MDX_EINVAL).
 *       - d in {16, 32, 40, 80, 160};  any other d returns MDX_EUNSUPPORTED.
 *       - alignment / strides: as for the V^T form above (ldq, ldk, ldv, sQ, sK, sV multiples of 8; Q, K, Vt 16-byte, O 8-byte aligned;
 *         ldo, sO multiples of 4); B * H * ceil(Tq / 128) must fit a 32-bit int.
 * One key count per query batch (mdx_attention_ctx_rows_bf16 / _f16, MDX_OP_ATTN_ROWS; additive symbols, the ABI version stays 12).  The
 * SAME descriptor, read differently in one field: tk_dev points to int32 [B] and batch b of Q attends to keys 0 .. tk_dev[b]-1 of batch b of
 * K / V^T - the scenes of a batched call attend to their own boxes, as each would in a call of its own.  Everything of the tk_dev paragraph
 * above holds per batch: counts are read when the kernel runs, the work of a workgroup depends on its own batch's count only (O of a batch is
 * bit-identical to mdx_attention_* with that count on that batch alone), and a count outside [1, Tk] writes NaN to the O rows of THAT batch.
 *   - tk_dev == NULL, kvmap != NULL, nsrc != 1, joint, causal or v_rowmajor != 0 return MDX_EINVAL (the message names the field); d, alignment
 *     and strides as in the tk_dev paragraph.  mdx_attention_* itself never reads more than one count.
 */
typedef struct MdxAttnDesc {
    const void* Q; const void* K; const void* Vt; void* O;
    const int32_t* kvmap; const int32_t* tk_dev;   /* tk_dev: NULL, or the device address of the live key count (see above; was reserved_p) */
    int64_t B, H, Tq, Tk, d, nsrc;
    int64_t ldq, sQ, ldk, sK, ldv, sV, ldo, sO;
    double scale;
    int64_t joint;
    int64_t q_prescaled;   /* 1: Q already carries scale * log2(e) (folded into the to_q weights when they were packed): `scale` is ignored,
                            * Q K^T is used as the base-2 exponent directly — lets the head-dim-40 kernel subtract the running maximum
                            * inside the QK MFMA (attention2.hip: FOLD).  0: plain Q, softmax(scale * Q K^T) as in the reference. */
    int64_t causal;        /* ABI 12.  1: query t attends to keys 0..t only (needs v_rowmajor == 1 and Tq == Tk).  0: every key. */
    int64_t v_rowmajor;    /* ABI 12.  1: `Vt` holds V row-major [Bkv][Tk][H*d] with token stride ldv (short-sequence kernel).  0: V^T as above. */
} MdxAttnDesc;
int mdx_attention_bf16(const MdxAttnDesc* d, void* stream);
int mdx_attention_ctx_rows_bf16(const MdxAttnDesc* d, void* stream);

/*
 * mdx_groupnorm_bf16 — GroupNorm(+SiLU) over channels-last [B][HW][C]
 * (ATen native_group_norm + silu: resnet.py:596-598, 626-630; transformer_2d.py:278;
 *  unet_2d_condition_multiview.py:519-521).  Statistics in fp32, pivot-shifted / Chan-combined (no E[x^2]-E[x]^2
 * cancellation); with a workspace, large maps take a two-stage fully coalesced path (deterministic, no atomics).
 * Served: X / Y at any 2-byte alignment and any ldx, ldy >= C — the one-launch kernel picks a vector width of 8, 4, 2 or 1 elements from
 * C / G, ldx, ldy and the two pointers; the two-stage path is taken only for C % 8 == 0, ldx, ldy % 8 == 0 and 16-byte aligned X / Y.
 * Requirements (MDX_EINVAL): G > 0 and C % G == 0; 0 < C <= ldx, ldy; B, HW, C, G fit a 32-bit int; gamma, beta must be 16-byte aligned
 * (read as float4); ws, when given, must be 16-byte aligned.
 * MDX_EUNSUPPORTED: more than 2560 channels per group on the one-launch kernel (its LDS gamma / beta table) — such a group is served only
 * where the two-stage path applies (workspace given, C % 8 == 0, C <= 5120, aligned, more than GN_ONE_KERNEL_ELEMS elements).
 */
typedef struct MdxGroupNormDesc {
    const void* X; void* Y; const float* gamma; const float* beta;
    int64_t B, HW, C, G, ldx, ldy;
    double eps;
    int64_t silu;
    float* ws; int64_t ws_bytes;   /* optional scratch for the two-stage (coalesced) path: B*chunks*G*3 floats */
} MdxGroupNormDesc;
int mdx_groupnorm_bf16(const MdxGroupNormDesc* d, void* stream);

/*
 * mdx_groupnorm_resident_bf16 — the same operation on the same descriptor through ONE kernel that reads the tensor once (additive symbols, the
 * ABI version stays 12; MDX_OP_GROUPNORM_RESIDENT; mdx_last_kernel() = "gn_resident_kernel").  One workgroup per (image, block of k groups) keeps its
 * HW x (k * C / G) slab in registers: fp32 mean, then the centred sum of squares from the registers (exact two-pass variance),
 * normalise (+SiLU), store.  Deterministic; `ws` is not used.  k comes from csrc/gn_route.h (gn_resident_plan).
 * MDX_EINVAL: every requirement of mdx_groupnorm_bf16 above.
 * MDX_EUNSUPPORTED, nothing launched and nothing written: option GN_RESIDENT = 0; X or Y not 16-byte aligned, ldx or ldy not a multiple
 * of 8, fewer than 8 channels per group, no k with k * C / G a multiple of 8 whose slab fits (1024 threads x 24 vectors of 16 bytes,
 * at most 2560 channels); and, unless GN_RESIDENT = 2, B * HW * C <= GN_ONE_KERNEL_ELEMS.  It never falls back to another kernel, and
 * mdx_groupnorm_bf16 never routes here.
 */
int mdx_groupnorm_resident_bf16(const MdxGroupNormDesc* d, void* stream);

/* mdx_layernorm_bf16 — LayerNorm over the last dim of [M][C] (attention.py:85,104,120; blocks.py:67-71).
 * Requirements (MDX_EINVAL): C, ldx, ldy must be multiples of 8, 0 < C <= ldx, ldy; X, Y, gamma, beta must be 16-byte aligned (rows move as
 * 16-byte pieces, gamma / beta as float4); M fits a 32-bit int.  C > 2048 returns MDX_EUNSUPPORTED. */
typedef struct MdxLayerNormDesc {
    const void* X; void* Y; const float* gamma; const float* beta;
    int64_t M, C, ldx, ldy;
    double eps;
    int64_t reserved0;
} MdxLayerNormDesc;
int mdx_layernorm_bf16(const MdxLayerNormDesc* d, void* stream);

/* mdx_softmax_rows — Y[r][0..T) = softmax(scale * X[r][0..T)) row by row, fp32 in (the fp32 scores of a Q K^T GEMM), bf16 out;
 * columns T..ldy-1 of Y are written as zeros (so Y can be the K-padded A operand of the P V GEMM).  Used by the VAE decoder's
 * single-head, 512-channel mid-block attention (attention_processor.py:495-558 with upcast_softmax; unet_2d_blocks.py:433-445),
 * whose head dim is outside the fused attention kernel's range.
 * Requirements (MDX_EINVAL): 0 < T <= ldx, ldy; rows, T, ldy fit a 32-bit int; X 4-byte, Y 2-byte aligned (element accesses only). */
typedef struct MdxSoftmaxDesc {
    const float* X; void* Y;
    int64_t rows, T, ldx, ldy;
    double scale;
    int64_t reserved0;
} MdxSoftmaxDesc;
int mdx_softmax_rows(const MdxSoftmaxDesc* d, void* stream);

/* ---- small element-wise kernels ---------------------------------------- */
#define MDX_EW_ADD 1          /* Y[m, :C] += X[m, :C]            (unet_2d_condition_multiview.py:464-488) */
#define MDX_EW_COPY 2         /* Y[m, :C]  = X[m, :C]  (concat halves: unet_2d_blocks.py:1990, 2090) */
#define MDX_EW_UPSAMPLE 3     /* nearest resize [B,Hi,Wi,C] -> [B,Ho,Wo,C] (resnet.py:154-163) */
#define MDX_EW_NCHW_TO_NHWC 4 /* X fp32/bf16 NCHW -> Y NHWC */
#define MDX_EW_NHWC_TO_NCHW 5
#define MDX_EW_SILU 6
#define MDX_EW_SCALE 7        /* Y = X * alpha */
/* Served at every alignment: X / Y need their element's natural alignment only (2 bytes, 4 for fp32), any ldx / ldy; the 16-byte kernels
 * (ew_vec8_kernel, ew_upsample_vec8_kernel) are taken for 16-bit X and Y with C % 8 == 0, ldx, ldy % 8 == 0 and 16-byte aligned pointers,
 * ew_scalar_kernel otherwise.  Requirements (MDX_EINVAL): a known kind; natural alignment; C, B, Hi, Wi, Ho, Wo fit a 32-bit int;
 * MDX_EW_UPSAMPLE needs ymap / xmap. */
typedef struct MdxEwDesc {
    const void* X; void* Y; const int32_t* ymap; const int32_t* xmap;
    int64_t kind, M, C, ldx, ldy;
    int64_t B, Hi, Wi, Ho, Wo;
    int64_t x_is_f32, y_is_f32;
    double alpha;
} MdxEwDesc;
int mdx_elementwise(const MdxEwDesc* d, void* stream);

/*
 * mdx_fourier_embed — NeRF embedding [x, sin(2^k x), cos(2^k x)]_{k<F} of 3-vectors
 * (magicdrive/networks/embedder.py:15-40) for camera columns (unet_addon_rawbox.py:288-305) and
 * box corners with the masked null blend pos*m + null*(1-m) (bbox_embedder.py:165-176).
 *   X fp32 [n][P][3]  ->  Y bf16 [n][P*(3+6F)] ; mask (uint8 [n]) and null (fp32 [P*(3+6F)]) optional.
 * Requirements (MDX_EINVAL): 0 <= F <= 16; P fits a 32-bit int; natural alignment of X, null_feat (4) and Y (2).  Element accesses only.
 */
typedef struct MdxFourierDesc {
    const float* X; void* Y; const uint8_t* mask; const float* null_feat;
    int64_t n, P, F, ldy;
} MdxFourierDesc;
int mdx_fourier_embed(const MdxFourierDesc* d, void* stream);

/*
 * mdx_gather_rows — Y[i,:] = m[i] ? T[idx[i],:] : null[:]  (class-token lookup with null blend,
 * bbox_embedder.py:179-180; idx may be -1 where mask is 0).
 * Optional added row (ABI 12; the fields were reserved_p / reserved0): add != NULL gives
 *     Y[i,:] = (m[i] ? T[idx[i],:] : null[:]) + add[i % add_period, :]
 * with add a 16-bit [add_period][ldt] table, the sum taken in fp32 and rounded once — token + position embedding of a text encoder
 * (transformers/models/clip/modeling_clip.py: CLIPTextEmbeddings) in one launch.  add == NULL: the plain gather, unchanged.
 * Requirements (MDX_EINVAL): C and n_rows fit a 32-bit int, n_rows must be positive; idx 8-byte aligned, T / Y / null_row 2-byte aligned;
 * with add: add 2-byte aligned, add_period positive.
 */
typedef struct MdxGatherDesc {
    const void* T; void* Y; const int64_t* idx; const uint8_t* mask; const void* null_row; const void* add;
    int64_t n, C, ldt, ldy, n_rows, add_period;
} MdxGatherDesc;
int mdx_gather_rows(const MdxGatherDesc* d, void* stream);

/*
 * mdx_timestep_embedding — sinusoidal timestep features, fp32 math
 * (diffusers/models/embeddings.py:24-64 with flip_sin_to_cos, downscale_freq_shift):
 *   Y[i, :] = [cos(t_i * f_j) | sin(t_i * f_j)]  (flip) , f_j = exp(-ln(max_period) * j / (half - shift))
 * Requirements (MDX_EINVAL): dim fits a 32-bit int, ldy >= dim; t and Y 4-byte aligned.
 */
typedef struct MdxTimeEmbDesc {
    const float* t; float* Y;   /* Y fp32 [n][ldy] */
    int64_t n, dim, flip_sin_to_cos, ldy;
    double freq_shift, max_period;
} MdxTimeEmbDesc;
int mdx_timestep_embedding(const MdxTimeEmbDesc* d, void* stream);

/*
 * mdx_cfg_ddim_step — fused classifier-free-guidance combine + DDIM update, fp32:
 *   eps = eps_u + g (eps_c - eps_u)                      pipeline_bev_controlnet.py:426-431
 *   x0  = (x - sqrt(1-a_t) eps) / sqrt(a_t) ; x <- sqrt(a_prev) x0 + sqrt(1-a_prev) eps
 *                                                        scheduling_ddim.py:379-425 (eta = 0)
 * coef: fp32 [n_steps][4] = {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)}; row = *step_ptr.
 * eps holds [uncond | cond] halves of n elements each when cfg != 0.  After the update the
 * kernel increments *step_ptr (single thread) so a replayed graph walks the table, and also
 * refreshes the model-input copy(ies) `x_in` (duplicated [uncond | cond] for CFG):
 *   xin_ld == 0 : x_in is fp32, flat, same layout as x;
 *   xin_ld  > 0 : x_in is bf16 channels-last with pixel stride xin_ld >= xin_c (x has xin_c channels per
 *                 pixel; the pad channels are never written) — the layout conv_in's MFMA path reads.
 * Requirements (MDX_EINVAL; the same hold for mdx_cfg_unipc_step): x, eps, coef, step_ptr 4-byte aligned; xin_c, xin_ld, gv_last_step fit a
 * 32-bit int; xin_ld is not negative; x_in at its element's alignment (4 / 2 bytes); xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c
 * dividing n; a given-view mode needs gv_noise (mode 1: also gv_cond) and gv_view_elems dividing n.  The x_in clauses are one check for
 * every op that refreshes x_in (these two, mdx_cfg_ddim_eta_step_*, mdx_latent_blend_*, mdx_latent_renoise_*): same rule, same message behind
 * the op's name.
 */
typedef struct MdxDdimDesc {
    float* x; const float* eps; const float* coef; int32_t* step_ptr; void* x_in; void* reserved_p;
    int64_t n, cfg;
    double guidance;
    int64_t xin_c, xin_ld;
    /* Given views (StableDiffusionBEVControlNetGivenViewPipeline, magicdrive/pipeline/pipeline_bev_controlnet_given_view.py:263-291,
     * :380-390): gv_mask[i / gv_view_elems] != 0 marks the views whose clean latents gv_cond are known; gv_noise is the initial
     * noise of every view (same layout as x).
     *   gv_mode 1 (conditional_latents_change_every_input): after the update of step s < gv_last_step a given view is replaced by
     *     add_noise(cond, noise, next timestep) = coef[s][2] * cond + coef[s][3] * noise (what the reference does at the top of
     *     the next iteration); the last step's output is kept.
     *   gv_mode 2: the combined noise prediction of a given view is replaced by gv_noise before the update.
     *   gv_mode 0 / gv_mask NULL: off. */
    const float* gv_cond; const float* gv_noise; const uint8_t* gv_mask;
    int64_t gv_mode, gv_view_elems, gv_last_step;
} MdxDdimDesc;
int mdx_cfg_ddim_step(const MdxDdimDesc* d, void* stream);

/*
 * mdx_cfg_unipc_step — fused classifier-free-guidance combine + one UniPC (order <= 2, B(h), predict-x0)
 * predictor-corrector update, fp32 (scheduling_unipc_multistep.py:256-300, 302-405, 407-516, 518-600 — the
 * sampler tools/test.py really uses, misc/test_utils.py:129).  Every quantity of the update is a linear
 * combination with per-step scalar coefficients, computed on the host from the timestep list:
 *   e   = eps_u + g (eps_c - eps_u)
 *   m_t = a x + b e                                   (x0 prediction)
 *   x_c = corr ? cl x_last + c1 m1 + c2 m2 + ct m_t : x   (UniC with the previous step's order)
 *   x  <- px x_c + pt m_t + p1 m1                      (UniP with this step's order)
 *   x_last <- x_c ; m2 <- m1 ; m1 <- m_t
 * coef: fp32 [n_steps][12] = {a, b, corr, cl, c1, c2, ct, px, pt, p1, an, sn}; row = *step_ptr, incremented after.
 * x_last, m1, m2: fp32 state buffers of n elements (zeroed by the caller before the first step).
 * x_in / xin_c / xin_ld as in MdxDdimDesc.
 * gv_* (ABI 8): given views exactly as in MdxDdimDesc — what demo/run_cond_on_view.py runs (its pipe comes from build_pipe, which
 * installs UniPC: magicdrive/misc/test_utils.py:129).  Re-noising is scheduler-independent (scheduling_unipc_multistep.py add_noise:
 * x = sqrt(acp_t) cond + sqrt(1 - acp_t) noise), so gv_mode 1 replaces a given view's PREDICTOR output of step s < gv_last_step by
 * an * cond + sn * noise with (an, sn) = coef[s][10..11] = (alpha, sigma) of the NEXT timestep; the multistep history (x_last, m1,
 * m2) keeps the values computed from the overwritten samples, as the reference's scheduler state does.  gv_mode 2 replaces the
 * combined noise prediction by gv_noise.
 */
typedef struct MdxUniPCDesc {
    float* x; const float* eps; const float* coef; int32_t* step_ptr; void* x_in; float* x_last; float* m1; float* m2;
    int64_t n, cfg;
    double guidance;
    int64_t xin_c, xin_ld;
    const float* gv_cond; const float* gv_noise; const uint8_t* gv_mask;
    int64_t gv_mode, gv_view_elems, gv_last_step;
} MdxUniPCDesc;
int mdx_cfg_unipc_step(const MdxUniPCDesc* d, void* stream);

/*
 * mdx_group_stats_bf16 / _f16 — per-group sample-health record of a tensor: one pass, no atomics, no host sync (additive symbols, the ABI
 * version stays 12; MDX_OP_GROUP_STATS; csrc/stats.hip).  The library's other error signal is a NaN written into a result (mdx_cfg_ddim_step
 * at a step index of -1, MdxAttnDesc.tk_dev out of range); this op is how a caller that never looks at the values themselves — a sampling
 * driver that hands latents to the VAE and the VAE's output to a PNG encoder — gets to see it, per view, without leaving the stream.
 *   X   : G groups of n contiguous elements, group g at X + g * sG (element strides).  f32 == 1: fp32 (the latents of a sampler plan,
 *         fp32 NHWC [views][h][w][4]: one group = one view) in either build; f32 == 0: the 16-bit type of the build (decoded images,
 *         activations).
 *   out : fp32 [n_rows][G][4], record of group g = {nonfinite, absmax, sum, sumsq}:
 *           nonfinite  count of NaN / +-Inf elements (fp32, exact: n <= 2^24), recognised by their exponent bits, not by comparisons;
 *           absmax     largest magnitude over the FINITE elements, 0 without one (bit-exact);
 *           sum, sumsq over the finite elements, fp32 accumulation in a fixed order: one workgroup per group, per-thread strided
 *                      16-byte pieces, wave-64 butterfly, fixed-order combine of the waves through LDS — the bits of a record depend on
 *                      the group's own n elements only (not on G or on the other groups); the longest addition chain is
 *                      k(n) = ceil(ceil(n / V) / 256) + log2(V) + 9 with V = 4 (fp32) or 8 (16-bit) elements per piece.
 *   row_dev : NULL, or a device pointer to ONE int32 (4-byte aligned), e.g. a plan's step counter.  The records of a launch go to row
 *         *row_dev of `out`, read on the device when the kernel RUNS (a replayed hipGraph sees the value current at replay, like
 *         MdxDdimDesc.step_ptr); a row outside [0, n_rows) writes NOTHING.  NULL: row 0, n_rows is ignored.
 * The 16-byte loads are taken when X is 16-byte aligned and (G == 1 or sG * element size is a multiple of 16); any other alignment is
 * SERVED by scalar loads in the same summation order (same bits).  Nothing is read outside [X + g * sG, X + g * sG + n).
 * Contract, checked on the host before the launch (MDX_EINVAL, the message names the field): X and out not NULL; f32 in {0, 1}; 0 <= n <= 2^24; 0 <= G fits a 32-bit int;
 * sG >= 0; X at its element's natural alignment (4 / 2 bytes); out 16-byte aligned (a record is one 16-byte store); with row_dev: row_dev
 * 4-byte aligned, 1 <= n_rows fits a 32-bit int.  G == 0 or n == 0: MDX_OK, nothing is launched and nothing written.
 */
typedef struct MdxStatsDesc {
    const void* X; float* out; const int32_t* row_dev;
    int64_t G, n, sG, n_rows, f32;
} MdxStatsDesc;
int mdx_group_stats_bf16(const MdxStatsDesc* d, void* stream);

/*
 * mdx_sdpa_bf16 / _f16 — scaled-dot-product attention on Q, K and V as a projection writes them, for any sequence length (additive symbols,
 * the ABI version stays 12; MDX_OP_SDPA; csrc/attention_vrow.hip; mdx_last_kernel() starts with "attn_vrow_kernel<").  V is read ROW-MAJOR,
 * in place: no V^T operand, no padded key axis.  mdx_attention_* and its routes are unchanged and never come here.
 *   Q [B][Tq][H*d], K [B][Tk][H*d], V [B][Tk][H*d], O [B][Tq][H*d], 16-bit: element (b,t,h,j) of X at X + b*sX + t*ldx + h*d + j (element
 *   strides).  Batch b of Q attends to batch b of K / V.
 * Result: O[b,q,h,:] = softmax_j(scale * Q[b,q,h,:] . K[b,j,h,:] + mask) . V[b,j,h,:].  Softmax in fp32 with exp2: the scores are scaled, then
 *   masked, and the maximum is taken of the scaled values (Tk == 1 returns V[b,0] and causal row 0 returns V[b,0] bit for bit); P is rounded to
 *   the storage type before the PV product, the row sum is taken of the unrounded values (as mdx_attention_*).
 * Shapes: any Tq, Tk >= 1; Tq != Tk is allowed without causal.  d % 8 == 0, d <= 160 and ceil(d / 16) in {1..6, 8, 10} (the instance set of
 *   mdx_attention_*); any other d returns MDX_EUNSUPPORTED, the message names d.
 * Aliasing: Q, K and V may be the column blocks of one [B][T][3*H*d] buffer (ldq = ldk = ldv = 3*H*d).  O must not alias them.
 * Contract, checked on the host before the launch (MDX_EINVAL, the message names the field): Q, K, V, O not NULL; Q, K, V 16-byte aligned, ldq, ldk, ldv, sQ, sK, sV multiples
 *   of 8; O 8-byte aligned, ldo, sO multiples of 4; ldq, ldk, ldv, ldo >= H*d; klen_dev 4-byte aligned; B, H, Tq, Tk fit a 32-bit int and
 *   are not negative; causal in {0, 1}; causal == 1 needs Tq == Tk.
 * causal == 1: key j is visible to query i iff j <= i.
 * klen_dev: NULL, or int32 [B] on the device: batch b attends to keys [0, klen_dev[b]); with causal, key j is visible iff j <= i and
 *   j < klen_dev[b].  The counts are read when the kernel RUNS, so a replayed graph sees a value written since capture.  A count outside
 *   [1, Tk] writes NaN to every O row of that batch and to no other batch (the convention of MdxAttnDesc.tk_dev).  A batch with the full
 *   count Tk has the bits of the klen_dev == NULL call.
 * Memory safety: the kernel never reads a K or V row at or past Tk (with klen_dev: at or past the count) of its batch; the tail rows of a
 *   staged tile are loaded from a clamped row and zeroed, so a pad row contributes 0 * 0, never 0 * garbage.  All addressing is 64-bit.
 * Range: the PV product accumulates un-normalised in fp32 (sum_j p_j v_j with p_j <= 1, up to Tk terms), as in mdx_attention_*: |V| * Tk
 *   must stay below the fp32 maximum.  Every fp16 value qualifies; bf16 values within a factor Tk of the type's maximum can overflow to Inf.
 * Empty calls: B, H, Tq or Tk equal to 0 launches nothing and returns MDX_OK (after the checks above).
 * Determinism: the summation order is fixed; the bits of batch b's rows depend on batch b's operands alone, not on B and not on the
 *   waves per workgroup the launcher picks.
 */
typedef struct MdxSdpaDesc {
    const void* Q; const void* K; const void* V; void* O;
    const int32_t* klen_dev;
    int64_t B, H, Tq, Tk, d;
    int64_t ldq, sQ, ldk, sK, ldv, sV, ldo, sO;
    double scale;
    int64_t causal;
} MdxSdpaDesc;
int mdx_sdpa_bf16(const MdxSdpaDesc* d, void* stream);

/*
 * mdx_latent_blend_bf16 / _f16 — keep known REGIONS of the latents while sampling: per-pixel, fractional masks for given views (additive
 * symbols, the ABI version stays 12; MDX_OP_LATENT_BLEND; csrc/blend.hip; mdx_last_kernel() starts with "blend_kernel").  The per-pixel form of
 * gv_mode 1 of MdxDdimDesc / MdxUniPCDesc (pipeline_bev_controlnet_given_view.py:283-295), as an op of its own placed BEHIND the scheduler
 * op of a step; the scheduler descriptors are untouched.  The two builds differ only in the 16-bit type of x_in.
 *   x     : fp32 [n] latents, the scheduler op's output, updated in place;
 *   cond  : fp32 [n] known clean latents, noise : fp32 [n] initial noise, both in x's layout;
 *   mask  : fp32 [n / mask_elems]: m = mask[i / mask_elems] belongs to element i (mask_elems = the channel count of an NHWC latent: one
 *           value per latent pixel).  1 keeps the known latent, 0 keeps the sampler's, a fraction mixes.  The values are device data and
 *           taken as they are; callers validate them (the pipeline does, on the host);
 *   coef, step_ptr : the scheduler op's table and counter.  The scheduler op has already advanced *step_ptr, so the step just finished is
 *           s = *step_ptr - 1, read when the kernel RUNS (a replayed hipGraph sees the current value).  s < 0 or s >= last_step writes
 *           NOTHING: the last step's output stays the scheduler's, as in gv_mode 1.  Otherwise a = coef[s * coef_ld + col_a] and
 *           sg = coef[s * coef_ld + col_s]: (alpha, sigma) of the NEXT timestep — columns 2, 3 of a DDIM row (coef_ld 4), 10, 11 of a
 *           UniPC row (coef_ld 12).
 * For every i < n, with t = a * cond[i] + sg * noise[i] (the expression of the schedulers' gv_mode 1 line, one helper in csrc/common.h:
 * a mask of ones gives the bits of that path):
 *   m == 0 : x[i] and its x_in copies are not touched (they keep the scheduler op's bits);
 *   m == 1 : x[i] = t;
 *   else   : x[i] = fmaf(m, t - x[i], x[i]).
 * Every written element also refreshes x_in as the scheduler kernels do: xin_ld == 0: fp32, flat; xin_ld > 0: the build's 16-bit type,
 * channels-last with pixel stride xin_ld (the pad channels are never written); cfg != 0: both [uncond | cond] halves.  x_in NULL: no copy.
 * fp32 math, no atomics, 64-bit addressing.  16-byte accesses when x, cond, noise are 16-byte aligned and mask_elems % 4 == 0; any other
 * case is SERVED by scalar accesses with the same bits.  Nothing is read or written past n elements, n / mask_elems mask entries, or the
 * x_in pixels of n / xin_c rows (twice that many rows when cfg != 0).
 * Contract, checked on the host before the launch (MDX_EINVAL, the message names the field): x, cond, noise, mask, coef, step_ptr not
 * NULL (x_in may be NULL); x, cond, noise, mask, coef, step_ptr 4-byte aligned, x_in at its element's alignment (4 / 2 bytes); n not
 * negative; mask_elems >= 1 and divides n; 0 <= col_a, col_s < coef_ld; cfg in {0, 1}; xin_c, xin_ld, coef_ld, last_step fit a 32-bit int
 * and xin_ld is not negative; xin_ld > 0 needs 0 < xin_c <= xin_ld and xin_c dividing n.  n == 0: MDX_OK (after the checks), nothing is
 * launched.
 */
typedef struct MdxBlendDesc {
    float* x; const float* cond; const float* noise; const float* mask; const float* coef;
    const int32_t* step_ptr; void* x_in;
    int64_t n, mask_elems, coef_ld, col_a, col_s, last_step, cfg, xin_c, xin_ld;
} MdxBlendDesc;
int mdx_latent_blend_bf16(const MdxBlendDesc* d, void* stream);

/*
 * mdx_latent_renoise_bf16 / _f16 — one forward jump of the sampler with Gaussian noise made on the device: the resampling move of RePaint
 * (Lugmayr et al. 2022; scheduling_repaint.py undo_step, `jump` of them in one go), for kept-region edits (additive symbols, the ABI
 * version stays 12; MDX_OP_LATENT_RENOISE; csrc/noise.hip; mdx_last_kernel() starts with "renoise_kernel").  An op of its own, launched
 * BETWEEN steps; no scheduler or blend descriptor changes.  The two builds differ only in the 16-bit type of x_in.
 *   x         : fp32 [n] latents, updated in place;   x_in : the model-input copies, as in MdxBlendDesc (may be NULL);
 *   coef      : the scheduler's table, n_rows rows of coef_ld floats;
 *   step_ptr  : int32, the scheduler op's counter, READ AND WRITTEN;   visit_ptr : int32 jump counter, READ AND WRITTEN;
 *   seeds     : uint64 [n / group_elems], device memory: one seed per group of group_elems consecutive elements (a view).
 * With c = *step_ptr and v = *visit_ptr, both read when the kernel RUNS (a replayed hipGraph sees the current values):
 *   current level: the sample is where the scheduler op of step c - 1 left it, sqrt(abar) = coef[(c - 1) * coef_ld + col_p] (DDIM row: col_p = 2);
 *   target level : the one step c - jump expects, coef[(c - jump) * coef_ld + col_t] (DDIM row: col_t = 0);
 *   r = target / current, sg = sqrtf(fmaxf(0, 1 - r * r)) (fp32; 1 - r * r is fmaf(-r, r, 1): one rounding), and for every i < n:
 *   x[i] = fmaf(r, x[i], sg * z[i]) with the product sg * z[i] rounded
 * — q(x_{t+jump} | x_t), the distribution of `jump` single undo steps.  Every written element refreshes x_in as the scheduler kernels do:
 * xin_ld == 0: fp32, flat; xin_ld > 0: the build's 16-bit type, channels-last with pixel stride xin_ld (pad channels never written);
 * cfg != 0: both [uncond | cond] halves.  Then a separate one-thread launch (every block of the first has read the counters by then)
 * sets *step_ptr = c - jump and *visit_ptr = v + 1.
 * Out of range — jump < 1, c < 1, c > n_rows or c - jump < 0 — is a caller error discovered on the device: x is filled with NaN (the
 * library's signal, as for a DDIM step index of -1), x_in and both counters are left alone.
 * The noise z, to the bit of its inputs: element i belongs to group g = i / group_elems with relative index e = i - g * group_elems.
 * One Philox4x32-10 call (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) with counter
 * (lo32(e / 4), hi32(e / 4), v, 0) and key (lo32(seeds[g]), hi32(seeds[g])) yields (w0, w1, w2, w3) for four consecutive e.
 * u1(w) = ((w >> 8) + 1) * 2^-24 in (0, 1], u2(w) = (w >> 8) * 2^-24 in [0, 1), both exact in fp32.
 * z[4k + 0] = sqrt(-2 ln u1(w0)) * cos(2 pi u2(w1)), z[4k + 1] the same radius with sin; z[4k + 2], z[4k + 3] from (w2, w3) likewise
 * (fp32 evaluation, within 1e-5 of the exact value).  Group g's noise depends on seeds[g], v and e only: not on n, not on the group's
 * position, not on the instance that served the call.
 * fp32 math, no atomics, 64-bit addressing.  16-byte accesses when x is 16-byte aligned and group_elems % 4 == 0; any other case is
 * SERVED by scalar accesses with the same bits.  Nothing is read or written past n elements, n / group_elems seeds, or the x_in pixels
 * of n / xin_c rows (twice that many rows when cfg != 0).
 * Contract, checked on the host before the launch (MDX_EINVAL, the message names the field): x, coef, step_ptr, visit_ptr, seeds not
 * NULL (x_in may be NULL); x, coef, step_ptr, visit_ptr 4-byte aligned, seeds 8-byte aligned, x_in at its element's alignment
 * (4 / 2 bytes); n not negative; group_elems >= 1 and divides n; jump and n_rows fit a 32-bit int and are >= 1; 0 <= col_t, col_p <
 * coef_ld; cfg in {0, 1}; xin_c, xin_ld, coef_ld fit a 32-bit int and xin_ld is not negative; xin_ld > 0 needs 0 < xin_c <= xin_ld and
 * xin_c dividing n.  n == 0: MDX_OK (after the checks), nothing is launched.
 */
typedef struct MdxRenoiseDesc {
    float* x; void* x_in; const float* coef; int32_t* step_ptr; int32_t* visit_ptr; const uint64_t* seeds;
    int64_t n, group_elems, jump, n_rows, coef_ld, col_t, col_p, cfg, xin_c, xin_ld;
} MdxRenoiseDesc;
int mdx_latent_renoise_bf16(const MdxRenoiseDesc* d, void* stream);

/*
 * mdx_cfg_ddim_eta_step_bf16 / _f16 — the DDIM step with eta > 0: classifier-free guidance, the DDIM update, the variance noise of
 * scheduling_ddim.py:415-438, the given views and the x_in refresh in one pass, with the noise made on the device (additive symbols, the
 * ABI version stays 12; MDX_OP_DDIM_ETA; csrc/noise.hip; mdx_last_kernel() starts with "ddim_eta_kernel").  It stands in the place of
 * mdx_cfg_ddim_step in a step program; mdx_cfg_ddim_step itself is unchanged.  The two builds differ only in the 16-bit type of x_in.
 *   x, eps, coef, step_ptr, x_in, cfg, guidance, xin_c, xin_ld, gv_* : as in MdxDdimDesc; coef is the UNCHANGED table of 4 columns;
 *   var       : fp32 [n_rows][2] = {dir, std} per step: std = eta sqrt(variance), dir = sqrt(1 - a_prev - std^2) (eta = 0: dir = coef[.][3]);
 *   draw_ptr  : int32, how many steps of this op have run in this call, READ AND WRITTEN;
 *   seeds     : uint64 [n / group_elems], device memory: one seed per group of group_elems consecutive elements (a view);   or
 *   noise     : fp32 [n], the caller's own standard normal noise (DDIMScheduler.step's variance_noise); when not NULL it is z and seeds
 *               is not read.
 * With s = *step_ptr and v = *draw_ptr, both read when the kernel RUNS (a replayed hipGraph sees the current values), c = coef + 4 s and
 * (dir, std) = var[s], for every i < n:
 *   e   = cfg != 0 ? eps[i] + guidance (eps[n + i] - eps[i]) : eps[i];      a given element under gv_mode 2: e = gv_noise[i]
 *   x0  = (x[i] - c[1] e) / c[0];   det = c[2] x0 + dir e                    a given element under gv_mode 2: dir = c[3], std = 0
 *   xn  = std != 0 ? det + (std * z[i]) : det                                the product std * z[i] is rounded before it is added
 *   x[i] = gv_mode 1, given, s < gv_last_step ? c[2] gv_cond[i] + c[3] gv_noise[i] : xn
 * and every written element refreshes x_in as mdx_cfg_ddim_step does.  A gv_mode 2 element therefore stays exactly on its own add_noise
 * trajectory.  A row with std == 0 computes no noise and, with dir = c[3], gives the bits of mdx_cfg_ddim_step on the same operands.
 * Then a separate one-thread launch (every block of the first has read the counters by then) sets *step_ptr = s + 1, *draw_ptr = v + 1.
 * Out of range — s < 0 or s >= n_rows — is a caller error discovered on the device: x is filled with NaN, x_in and both counters are
 * left alone.
 * The generated noise z, to the bit of its inputs: the mapping of mdx_latent_renoise_* with counter word 3 = 1.  Element i belongs to
 * group g = i / group_elems with relative index e = i - g * group_elems; one Philox4x32-10 call with counter
 * (lo32(e / 4), hi32(e / 4), v, 1) and key (lo32(seeds[g]), hi32(seeds[g])) yields (w0, w1, w2, w3) for four consecutive e, and
 * u1, u2 and z[4k + 0 .. 3] follow from the words exactly as there (fp32 evaluation, within 1e-5 of the exact value).  Counter word 3 is
 * the stream's domain: 0 = a jump of mdx_latent_renoise_*, 1 = a step of this op.  Philox is a bijection of the counter under one key,
 * so the two streams never share a block, even with equal seed, equal element and v equal to the jump's visit count: one seed per scene
 * serves both.  A resample jump moves *step_ptr back and leaves *draw_ptr alone: a revisited step draws fresh noise.
 * fp32 math, no atomics, 64-bit addressing.  16-byte accesses of x when x is 16-byte aligned and group_elems % 4 == 0; any other case is
 * SERVED by scalar accesses with the same bits.  Nothing is read or written past n elements of x / noise / gv_cond / gv_noise, n (2 n
 * when cfg != 0) of eps, n / group_elems seeds, n / gv_view_elems mask bytes, or the x_in pixels of n / xin_c rows (twice when cfg != 0).
 * Contract, checked on the host before the launch (MDX_EINVAL, the message names the field): x, eps, coef, var, step_ptr, draw_ptr not
 * NULL (x_in may be NULL); seeds and noise not both NULL; x, eps, coef, var, step_ptr, draw_ptr, noise 4-byte aligned, seeds 8-byte
 * aligned, x_in at its element's alignment (4 / 2 bytes); n not negative; group_elems >= 1 and divides n; n_rows fits a 32-bit int and
 * is >= 1; cfg in {0, 1}; xin_c, xin_ld, gv_last_step fit a 32-bit int and xin_ld is not negative; xin_ld > 0 needs
 * 0 < xin_c <= xin_ld and xin_c dividing n; a given-view mode needs gv_noise (mode 1: also gv_cond) and gv_view_elems dividing n.
 * n == 0: MDX_OK (after the checks), nothing is launched.
 */
typedef struct MdxDdimEtaDesc {
    float* x; const float* eps; const float* coef; const float* var; int32_t* step_ptr; int32_t* draw_ptr; void* x_in;
    const uint64_t* seeds; const float* noise;
    int64_t n, cfg;
    double guidance;
    int64_t xin_c, xin_ld, group_elems, n_rows;
    const float* gv_cond; const float* gv_noise; const uint8_t* gv_mask;
    int64_t gv_mode, gv_view_elems, gv_last_step;
} MdxDdimEtaDesc;
int mdx_cfg_ddim_eta_step_bf16(const MdxDdimEtaDesc* d, void* stream);

/*
 * mdx_image_composite_bf16 / _f16 — composite a kept-region edit with the recorded pictures: every pixel outside the edited regions
 * becomes the recorded pixel again, bit for bit, and a feathered band inside the kept region hides the seam (additive symbols, the ABI
 * version stays 12; MDX_OP_IMAGE_COMPOSITE; csrc/composite.hip; mdx_last_kernel() starts with "composite_kernel").  An op on the VAE
 * decoder's output, outside the sampler's plan.  The two builds differ only in the 16-bit type of gen (gen_f32 == 0).
 *   gen   : [V][C][H][W] decoder output in [-1, 1], planar: element (v, c, y, x) at gen + v * g_sv + c * g_sc + y * g_ld + x (strides in
 *           elements); the build's 16-bit type, or fp32 when gen_f32 == 1;
 *   orig  : fp32 [V][H][W][C] recorded pictures in [0, 1], contiguous;
 *   keep  : fp32 [V][H / f][W / f] keep masks at latent resolution, contiguous: 1 keeps, 0 regenerates.  The values are device data and
 *           taken as they are; callers validate them (the pipeline does, on the host);
 *   out   : fp32 [V][H][W][C], contiguous: the composited pictures, the layout decode_latents hands to numpy;
 *   matte : NULL, or fp32 [V][H][W], contiguous: receives w;
 *   has   : NULL (every view has a picture), or uint8 [V]: has[v] == 0 is a view without a picture — out = g, matte = 0, and the orig and
 *           keep rows of that view are NOT read.
 * The matte of a view, with r = feather image pixels and every coordinate clamped to the image (edge replicate):
 *   a(y, x) = keep[y / f][x / f];
 *   e(y, x) = min of a over the (2r+1)^2 window around (y, x)                                   (erosion);
 *   w(y, x) = S / (2r+1)^2, S the fp32 sum of e over the (2r+1)^2 window around (y, x)          (one IEEE division).
 * S is summed along the row first, then down the column, each sequentially.  For masks on the 1/64 grid every sum is exact, whatever the
 * order.  r == 0: w = a.  w = 0 wherever a = 0, w = 1 wherever every a within Chebyshev distance 2r is 1, and the transition band of
 * width 2r lies inside the kept region.  Next to the image border w = 0 may reach a few pixels past a = 0 (the clamped window is cut).
 * The blend, per pixel and channel, with round16 = rounding to gen's 16-bit type (not applied when gen_f32):
 *   g = clamp01(float(round16(fmaf(gen, 0.5, 0.5))))      the bits of (image / 2 + 0.5).clamp(0, 1).float(): NaN stays NaN, +Inf -> 1, -Inf -> 0;
 *   w == 0 : out = g;   w == 1 : out = orig (a non-finite gen does not reach a fully kept pixel);   else : out = fmaf(w, orig - g, g).
 * One launch, one workgroup per (view, 32 x 64 pixel tile); the tile's patch of keep cells with its halo of 2r pixels is staged in LDS
 * once and both separable passes run out of LDS.  fp32 math, no atomics, 64-bit addressing, deterministic: a view's bits depend on that
 * view's operands only — not on V, not on the tile walk, not on whether matte is given.  16-byte accesses of gen when gen and the byte
 * sizes of g_ld, g_sc, g_sv are multiples of 16, of orig / out when both are 16-byte aligned and W * C % 4 == 0, of matte when it is
 * 16-byte aligned and W % 4 == 0; any other case is SERVED by scalar accesses with the same bits.  Nothing is read or written outside
 * the described extents: W elements of each gen row, V * H * W * C floats of orig / out, V * (H / f) * (W / f) of keep, V * H * W of matte,
 * V bytes of has.
 * Contract, checked on the host before the launch (MDX_EINVAL, the message names the field): gen, orig, keep, out not NULL (matte and
 * has may be NULL); gen at its element's alignment (2 / 4 bytes); orig, keep, out, matte 4-byte aligned; V not negative; C in [1, 4];
 * H, W >= 1; f >= 1 and divides H and W; feather in [0, 16]; gen_f32 in {0, 1}; g_ld >= W; g_sc, g_sv not negative; V, C, H, W, f,
 * feather and H * W fit a 32-bit int.  V == 0: MDX_OK (after the checks), nothing is launched.
 */
typedef struct MdxCompositeDesc {
    const void* gen; const float* orig; const float* keep; float* out; float* matte; const uint8_t* has;
    int64_t V, C, H, W, f, feather, gen_f32;
    int64_t g_sv, g_sc, g_ld;
} MdxCompositeDesc;
int mdx_image_composite_bf16(const MdxCompositeDesc* d, void* stream);

/* ---- program = array of ops, executed in order on one stream ------------ */
#define MDX_OP_GEMM 1
#define MDX_OP_CONV 2
#define MDX_OP_CONV_DIRECT 3
#define MDX_OP_ATTN 4
#define MDX_OP_GROUPNORM 5
#define MDX_OP_LAYERNORM 6
#define MDX_OP_EW 7
#define MDX_OP_FOURIER 8
#define MDX_OP_GATHER 9
#define MDX_OP_TIMEEMB 10
#define MDX_OP_DDIM 11
#define MDX_OP_UNIPC 12
#define MDX_OP_SOFTMAX 13
#define MDX_OP_ATTN_ROWS 14   /* MdxAttnDesc through mdx_attention_ctx_rows_*: tk_dev -> int32 [B] */
#define MDX_OP_GROUPNORM_RESIDENT 15   /* MdxGroupNormDesc through mdx_groupnorm_resident_* */
#define MDX_OP_GROUP_STATS 16          /* MdxStatsDesc through mdx_group_stats_* */
#define MDX_OP_SDPA 17                 /* MdxSdpaDesc through mdx_sdpa_* */
#define MDX_OP_LATENT_BLEND 18         /* MdxBlendDesc through mdx_latent_blend_* */
#define MDX_OP_LATENT_RENOISE 19       /* MdxRenoiseDesc through mdx_latent_renoise_* */
#define MDX_OP_IMAGE_COMPOSITE 20      /* MdxCompositeDesc through mdx_image_composite_* */
#define MDX_OP_DDIM_ETA 21             /* MdxDdimEtaDesc through mdx_cfg_ddim_eta_step_* */

/* 16-bit storage / MFMA operand type of an op's activations and weights.  The reference samples in fp16 (magicdrive/misc/test_utils.py:95
 * `weight_dtype = torch.float16`); BASELINE.json's benchmark configuration names bf16.  Every op entry point exists in both builds:
 * mdx_<op>_bf16 / mdx_<op> (bf16) and mdx_<op>_f16 (IEEE fp16) — same descriptors, fp32 accumulation, fp32 side inputs (bias, temb,
 * norm affine, latents).  A program carries the choice per op. */
#define MDX_DTYPE_BF16 0
#define MDX_DTYPE_F16 1

#define MDX_OP_BYTES 512
typedef struct MdxOp {
    int64_t opcode;
    int64_t dtype;                           /* MDX_DTYPE_* */
    unsigned char desc[MDX_OP_BYTES - 16];   /* one of the Mdx*Desc above, zero padded */
} MdxOp;

/* the fp16 build of the op entry points above (identical descriptors and semantics; 16-bit tensors hold IEEE fp16) */
int mdx_gemm_f16(const MdxGemmDesc* d, void* stream);
int mdx_conv2d_f16(const MdxConvDesc* d, void* stream);
int mdx_conv2d_direct_f16(const MdxConvDirectDesc* d, void* stream);
int mdx_attention_f16(const MdxAttnDesc* d, void* stream);
int mdx_groupnorm_f16(const MdxGroupNormDesc* d, void* stream);
int mdx_groupnorm_resident_f16(const MdxGroupNormDesc* d, void* stream);
int mdx_layernorm_f16(const MdxLayerNormDesc* d, void* stream);
int mdx_elementwise_f16(const MdxEwDesc* d, void* stream);
int mdx_fourier_embed_f16(const MdxFourierDesc* d, void* stream);
int mdx_gather_rows_f16(const MdxGatherDesc* d, void* stream);
int mdx_timestep_embedding_f16(const MdxTimeEmbDesc* d, void* stream);
int mdx_cfg_ddim_step_f16(const MdxDdimDesc* d, void* stream);
int mdx_cfg_unipc_step_f16(const MdxUniPCDesc* d, void* stream);
int mdx_softmax_rows_f16(const MdxSoftmaxDesc* d, void* stream);
int mdx_attention_ctx_rows_f16(const MdxAttnDesc* d, void* stream);
int mdx_group_stats_f16(const MdxStatsDesc* d, void* stream);
int mdx_sdpa_f16(const MdxSdpaDesc* d, void* stream);
int mdx_latent_blend_f16(const MdxBlendDesc* d, void* stream);
int mdx_latent_renoise_f16(const MdxRenoiseDesc* d, void* stream);
int mdx_image_composite_f16(const MdxCompositeDesc* d, void* stream);
int mdx_cfg_ddim_eta_step_f16(const MdxDdimEtaDesc* d, void* stream);

/* Run ops[0..n) in order on `stream`.  Stops at the first failing op (returns its code;
 * mdx_last_error() names the op index followed by the op's own message).  Every op goes through the entry point of its dtype, so each
 * requirement listed above holds here and for the _f16 symbols unchanged. */
int mdx_program_run(const MdxOp* ops, int64_t n, void* stream);

/* Capture ops[0..n) into a hipGraph (stream capture on an internal stream) and instantiate it.
 * The pointers inside the ops are baked into the graph; per-replay variation comes only from
 * device memory (sel_ptr / step_ptr tables). */
int mdx_graph_create(const MdxOp* ops, int64_t n, void** graph_out);
int mdx_graph_launch(void* graph, void* stream);
int mdx_graph_destroy(void* graph);

int mdx_abi_version(void);
/* Hash of the kernel sources this library was built from (csrc/Makefile: sha256 over every .hip / .h, first 16 hex digits).  Counter
 * summaries under profiles/ record it; bench.py drops counters whose build differs from the library it is timing. */
const char* mdx_build_id(void);
const char* mdx_last_error(void);
/* Name of the kernel the calling thread's last op launched (the one doing the op's work; which GEMM / conv main loop a
 * descriptor is routed to is decided inside the library by shape).  Measurement aid: bench.py groups its per-launch HIP-event
 * timings by this name so they can be compared with rocprofv3's kernel statistics. */
const char* mdx_last_kernel(void);
/* Tuning / routing switches (magicdrive_amd/csrc/options.h lists every key with its default and meaning, e.g. "GEMM_XL", "XL_BN",
 * "ATTN2"): process-wide named integers that the launchers read on every call.  mdx_set_option returns MDX_EINVAL for an unknown
 * key.  The reference has no counterpart (its kernel choice lives inside xformers' dispatch, ops/fmha/dispatch.py, and cuDNN's
 * heuristics); they exist so that parity tests can force every main loop in-process and a profile can A/B a route.  mdx_option_name(i)
 * enumerates the keys (NULL past the end).  Captured graphs keep the route they were captured with. */
int mdx_set_option(const char* key, int64_t value);
int mdx_get_option(const char* key, int64_t* value_out);
const char* mdx_option_name(int64_t index);

/* Device facts for bench/roofline bookkeeping: out[0]=CU count, out[1]=clock kHz, out[2]=HBM bytes. */
int mdx_device_info(int64_t* out3);

#ifdef __cplusplus
}
#endif
#endif /* MDX_H_ */
