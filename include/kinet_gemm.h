/* kinet_amd C-ABI: MFMA GEMM and implicit-GEMM NHWC convolution with fused epilogues.
 *
 * Replaces, on the detection hot path, the cuBLAS/cuDNN work the reference delegates
 * to PyTorch ("Dense ops on the hot path"):
 *   nn.Linear in MSDeformAttn          (ms_deform_attn.py:27-30)
 *   FFN linear1/linear2                (deformable_transformer.py:273-276, 350-353)
 *   nn.MultiheadAttention in/out proj  (deformable_transformer.py:345, :371)
 *   class / bbox MLP heads             (deformable_detr.py:98-108, detr.py:937-951)
 *   ResNet convs + FrozenBatchNorm2d   (backbone.py:22-58, :102)  -- BN folded into scale/bias
 *   input_proj 1x1 / 3x3-s2 convs      (deformable_detr.py:63-71)
 *
 *   C[m, n] = epi( sum_k A[m, k] * B[n, k] )
 *   epi(v)  = relu?( v * scale[n] + bias[n] + R[m, n] ),  rows with row_mask[m] != 0 -> 0
 *
 * A, B, C, R row-major with leading dims lda, ldb, ldc, ldr (elements).  B is the
 * PyTorch weight layout (out_features, in_features), i.e. K-contiguous.  scale/bias
 * are f32 (NULL = 1 / 0).  in_dtype in {F32, BF16, F16} for A and B; out_dtype for C
 * and R in {F32, BF16, F16}.  bf16/f16 run v_mfma_f32_16x16x32_{bf16,f16}; f32 runs the
 * exact-f32 v_mfma_f32_16x16x4_f32 (parity mode).  Requirements: K % 8 == 0, lda/ldb
 * multiples of 8, 16-byte aligned A/B.
 */
#ifndef KINET_GEMM_H_
#define KINET_GEMM_H_

#include "kinet_common.h"

#ifdef __cplusplus
extern "C" {
#endif

int kinet_gemm(const void* A, const void* B, void* C, int M, int N, int K,
               int lda, int ldb, int ldc, int in_dtype,
               const float* scale, const float* bias, const void* R, int ldr,
               int relu, int out_dtype, const uint8_t* row_mask, int reserved,
               kinet_stream_t stream);

/* Extended form: A2 (optional, same layout as A) is added to A at load time
 * (q = src + pos feeding a projection, deformable_transformer.py:292, :369, :377);
 * ln_gamma/ln_beta (optional, f32, N <= 320) apply LayerNorm(eps) over each output row
 * after the bias + residual add -- the post-norm of a transformer sub-layer
 * (deformable_transformer.py:287, :294, :364, :374, :380) fused into the GEMM epilogue. */
int kinet_gemm_ex(const void* A, const void* A2, const void* B, void* C, int M, int N, int K,
                  int lda, int ldb, int ldc, int in_dtype,
                  const float* scale, const float* bias, const void* R, int ldr, int relu,
                  const float* ln_gamma, const float* ln_beta, float ln_eps,
                  int out_dtype, const uint8_t* row_mask, kinet_stream_t stream);

/* Convolution, NHWC activations, weights (Cout, KH, KW, Cin) = PyTorch OIHW permuted.
 *   X (batch, Hin, Win, Cin) with Cin % 8 == 0 (pad channels with zeros otherwise)
 *   Y (batch, Hout, Wout, Cout) written with row stride ldy (>= Cout) so outputs can land
 *   directly inside a larger flattened buffer; R residual with the same layout (ldr).
 *   Hout = (Hin + 2*pad - KH) / stride + 1 (dilation 1). */
int kinet_conv2d(const void* X, const void* Wt, void* Y, int batch, int Hin, int Win, int Cin,
                 int Hout, int Wout, int Cout, int KH, int KW, int stride, int pad,
                 int in_dtype, const float* scale, const float* bias, const void* R, int ldr,
                 int relu, int ldy, kinet_stream_t stream);

/* kinet_conv2d with separate vertical / horizontal stride and padding
 * (Hout = (Hin + 2*pad_h - KH)/stride_h + 1, Wout = (Win + 2*pad_w - KW)/stride_w + 1);
 * used for the tap-folded ResNet stem (kinet_pack_image_kwfold). */
int kinet_conv2d_ex(const void* X, const void* Wt, void* Y, int batch, int Hin, int Win, int Cin,
                    int Hout, int Wout, int Cout, int KH, int KW, int stride_h, int stride_w, int pad_h,
                    int pad_w, int in_dtype, const float* scale, const float* bias, const void* R, int ldr,
                    int relu, int ldy, kinet_stream_t stream);

/* value_proj for MSDA: C = (A @ B^T + bias) with rows masked, stored HEAD-MAJOR:
 * row r = b*rows_per_batch + s, column n = g*head_dim + d  ->  C[((g*batch + b)*rows_per_batch + s)*head_dim + d]
 * i.e. (N/head_dim, batch, rows_per_batch, head_dim) -- the layout kinet_msda_fused_forward
 * gathers from best (ms_deform_attn.py:64-67 produce the same values in (N, S, M, D)).
 * out_dtype: in_dtype, or KINET_F16 from KINET_BF16 operands (f16 values feed the sampling
 * kernel's mixed-precision FMA; post-LayerNorm projections are far inside f16 range). */
int kinet_gemm_headmajor(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb,
                         int in_dtype, int out_dtype, const float* bias, const uint8_t* row_mask,
                         int rows_per_batch, int head_dim, kinet_stream_t stream);

/* kinet_gemm_headmajor with A + A2 as the left operand (the position embedding added at load
 * time, `with_pos_embed` of deformable_transformer.py:278); the MSDA offsets / logits
 * projection of the encoder writes (M, N, Lq, L*P*3) head-major this way
 * (kinet_msda_encoder_forward).  a2_rows: 0 = A2 has M rows like A; else A2 has a2_rows rows
 * (>= 32, dividing M) and row m adds A2 row m % a2_rows -- one frame's position embedding
 * shared by every frame of an unpadded batch (the same values the reference adds per frame). */
int kinet_gemm_headmajor_ex(const void* A, const void* A2, const void* B, void* C, int M, int N, int K,
                            int lda, int ldb, int in_dtype, int out_dtype, const float* bias,
                            const uint8_t* row_mask, int rows_per_batch, int head_dim, int a2_rows,
                            kinet_stream_t stream);

/* Split head-major store (round 5, the head_dim-36 MSDA value of configs 3-5): the weight rows
 * are ordered [every head's first head_dim channels | every head's last tail_dim channels];
 * columns [0, split_cols) go head-major (split_cols/head_dim, B, S, head_dim) to C and columns
 * [split_cols, N) head-major (heads, B, S, tail_dim) right after that plane, at
 * C + split_cols*M elements.  kinet_msda_encoder_forward_split reads the two planes.  Replaces
 * the value_proj + view of ms_deform_attn.py:64-66 for that kernel. */
int kinet_gemm_headmajor_split(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb,
                               int in_dtype, int out_dtype, const float* bias, const uint8_t* row_mask,
                               int rows_per_batch, int head_dim, int split_cols, int tail_dim,
                               kinet_stream_t stream);

/* Split-K forms for small-M / long-K problems (few output tiles): K is cut into `ksplit`
 * slices (rounded to whole 64-element K-steps) whose f32 partial tiles go to `workspace`
 * (ksplit * M * N floats, caller-allocated), then one finalize pass sums the slices and
 * applies the same epilogue (scale/bias, residual, ReLU, LayerNorm for N <= 1024, row mask)
 * into C / Y.  Deterministic (no atomics). */
int kinet_gemm_splitk(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                      int in_dtype, const float* scale, const float* bias, const void* R, int ldr, int relu,
                      const float* ln_gamma, const float* ln_beta, float ln_eps, int out_dtype,
                      const uint8_t* row_mask, float* workspace, int ksplit, kinet_stream_t stream);
int kinet_conv2d_splitk(const void* X, const void* Wt, void* Y, int batch, int Hin, int Win, int Cin,
                        int Hout, int Wout, int Cout, int KH, int KW, int stride, int pad, int in_dtype,
                        const float* scale, const float* bias, const void* R, int ldr, int relu, int ldy,
                        float* workspace, int ksplit, kinet_stream_t stream);

/* ResNet stem from the image (torchvision conv1, 7x7 / stride 2 / pad 3, 3 -> 64, + folded
 * FrozenBN + ReLU; the reference's backbone.py:102 body, IntermediateLayerGetter input): img
 * f32 NCHW (N, 3, H, W) -> Y NHWC (N, (H-1)/2+1, (W-1)/2+1, 64) in dtype (KINET_BF16 /
 * KINET_F16).  Replaces kinet_pack_image_kwfold + kinet_conv2d_ex over the folded layout
 * (same values: the image is rounded to dtype once, the tap-folded rows are built in LDS);
 * w_packed = the folded stem weights (64, 7, 1, 24) of that path; scale / bias (64) f32. */
int kinet_stem_conv_image(const float* img, const void* w_packed, const float* scale, const float* bias,
                          void* Y, int N, int H, int W, int dtype, kinet_stream_t stream);

/* The stem above followed by torchvision's maxpool (3x3 / stride 2 / pad 1, backbone.py:102's
 * ResNet body) in one launch: the conv map is never written.  Y NHWC (N, Hp, Wp, 64) with
 * Ho = (H-1)/2+1, Hp = (Ho-1)/2+1 (Wo, Wp alike), bit-identical to kinet_maxpool2d_3x3s2 of
 * kinet_stem_conv_image's output.  A workgroup walks a 62-conv-column strip downwards over
 * `seg_tiles` 4-row tiles carrying the conv row the next tile's pool window needs; seg_tiles = 0
 * lets the launcher choose (the value only moves work between workgroups, never the result). */
int kinet_stem_pool_image(const float* img, const void* w_packed, const float* scale, const float* bias, void* Y,
                          int N, int H, int W, int dtype, int seg_tiles, kinet_stream_t stream);

/* Diagnostic kernel-selection knob (no reference counterpart; used by the kernel
 * benchmarks to A/B GEMM kernels in one process).  bit 1: allow the 512-thread
 * 256x256-tile LDS-DMA kernel for large-M problems; bit 2: never use the
 * resident-weight streaming kernel; bit 8 (256): keep K = 512 problems off it (the
 * tiled kernel, as before round 3); bit 1024: never the direct 3x3 64 -> 64 channel
 * convolution (the implicit GEMM instead); bit 2048: strided 1x1 convolutions (the stage-2
 * downsample) on the implicit-GEMM kernel instead of the resident-weight conv-row kernel;
 * bit 268435456: the resident-weight kernel's 4-wave column groups everywhere (round 6 runs the
 * x + pos projections, K = 512 / N = 256, residual N > 256 and K = 288 N > 384 launches on
 * 8-wave groups); bit 1073741824: 32-column head-major stores without the LDS transpose.
 * All of these select among bit-identical kernels.  Returns the previous flags.  Per CALLING THREAD: torch
 * runs autograd backward for device tensors on its own engine thread, so flags set here do
 * NOT reach the backward kernels launched through autograd (only forward / direct calls). */
int kinet_gemm_set_flags(int flags);

/* How a tiled launch is chosen.  One host-side planner (csrc/gemm_plan.h) holds every tile
 * heuristic: from the sizes, the operand class, the calling thread's flags and forced tile, the
 * launch-fill policy and the device's compute-unit count it yields one or two launches, each an
 * entry of the one table of kernel instantiations plus a row range.  The launcher reads kernel,
 * workgroup size, grid and the kinet_gemm_last_kernel record from that entry alone; a tile the
 * table has no entry for, for these operands, is KINET_ERR_ARG before any kernel starts. */

/* Diagnostic tile override of the tiled kernel (0, 0 = heuristic), per calling thread: any tile of
 * the planner's table without the LayerNorm epilogue -- 32x64, {64,128}x{64,128}, and the 8-wave
 * 256x128 / 128x256 / 256x256 LDS-DMA tiles, which exist for 16-bit operands without A2 only: a
 * launch that has no instantiation of the forced tile returns KINET_ERR_ARG before any kernel
 * starts.  Ignored by the fused-LayerNorm launches. */
int kinet_gemm_force_tile(int bm, int bn);

/* The planner's answer for a described problem, without touching a device (no reference
 * counterpart; works on a machine without a GPU): what kinet_gemm(_ex), kinet_gemm_headmajor* or
 * kinet_conv2d(_ex) would launch once the call reaches the tiled kernel, i.e. when none of the
 * special-cased kernels of kinet_gemm_last_kernel (families 4-7) takes it.  conv: an implicit
 * convolution with K = KH*KW*Cin (a 1x1 stride-1 convolution is a plain GEMM: conv = 0); ln: fused
 * LayerNorm; a2: an A2 operand; kchunk: the K-slice length of a split-K launch, else 0; hm_rows:
 * rows_per_batch of a head-major store, else 0; in_dtype: a kinet_dtype; cus: the compute-unit
 * count to plan for (256 on MI355X).  Reads the calling thread's kinet_gemm_set_flags /
 * kinet_gemm_force_tile and the launch-fill policy like a real call.  *n_launches = 0 (M or N is
 * 0), 1 or 2; launches[3*i .. 3*i+2] = {kernel in the packing of kinet_gemm_last_kernel, first
 * row, number of row tiles} of launch i (room for 6 ints).  The launches cover rows [0, M) once,
 * in order.  KINET_ERR_ARG where the real call returns it for want of a tile. */
int kinet_gemm_plan(int M, int N, int K, int Cin, int conv, int ln, int a2, int kchunk, int hm_rows,
                    int in_dtype, int cus, int* n_launches, int* launches);

/* Split-K factor the Python layer uses for a GEMM / convolution of these sizes (ln: fused
 * LayerNorm): > 1 for K >= 1024 problems whose tile grid fills the compute units less than twice
 * over, else 1.  It looks at the planner's base 4-wave tile of a plain GEMM only, not at the full
 * plan. */
int kinet_gemm_ksplit(int M, int N, int K, int ln);

/* Which kernel served the calling thread's last GEMM / convolution call (host-side record, no
 * reference counterpart; tests assert through it that the kernel they mean to test ran):
 * (family << 20) | (bm << 10) | bn.  family: 0 none yet, 1 tiled (gemm_kernel), 2 tiled with
 * LDS-DMA staging (flag 16 and the 128x320 LayerNorm tile), 3 the 8-wave LDS-DMA tiles,
 * 4 resident-weight GEMM, 5 resident-weight conv, 6 direct 3x3 64 -> 64 conv, 7 stem conv,
 * 8 split-K (bm, bn: the tile of the partial-sum grid).  bm, bn: the tile of the last grid
 * launched by the tiled families, 0 for the special-cased kernels. */
int kinet_gemm_last_kernel(void);

/* Which instantiation of the resident-weight kernel (csrc/gemm_rw.hip gemm_rw_kernel, families 4 and 5
 * above and kinet_msda_sample_records) the calling thread's last launch was, and its grid (host-side
 * record, no reference counterpart; tests assert the instantiation they mean to test through it).
 * out[0 .. 14] = KC (K / 32), NT (16-column tiles per wave), BMR (rows per row tile), NS (ring slots),
 * NW (waves), OCC (workgroups per CU the launch is sized for), HAS_R, LN, HAS_A2, CR (conv-row mode),
 * PREP (sampling-record epilogue), the output element size in bytes, grid.x (P, workgroups per
 * column group), grid.y (column groups), the number of row tiles.  All zeros before the first such
 * launch and after a kinet_gemm* / kinet_conv2d* call that another kernel family served. */
int kinet_gemm_rw_last_config(int* out);

/* Diagnostic bound on the resident-weight kernel's grid.x, per calling thread (0 = none, the
 * default): P = min(P, max_p) after the launcher's own sizing, at least 1.  The kernel is persistent
 * (workgroup x walks row tiles x, x + P, ...), so the bound only changes which workgroup computes
 * which tile and how often a slot of its LDS ring is reused: outputs are bit-identical for every
 * value -- a small problem can walk a wrapping ring this way.  Returns the previous value. */
int kinet_gemm_rw_grid_cap(int max_p);

/* How a resident-weight launch is chosen.  One host-side planner (csrc/gemm_rw_plan.h) holds every
 * eligibility rule and variant heuristic of gemm_rw_kernel: from the described problem, the calling
 * thread's flags and grid cap and the device's compute-unit count it yields "not eligible" (another
 * kernel family serves the call) or one entry of the one table of kernel instantiations plus its
 * grid.  The launcher reads kernel, workgroup size, grid and the kinet_gemm_rw_last_config record from
 * that entry alone.
 *
 * kinet_gemm_rw_plan: the planner's answer for a described problem, without touching a device (no
 * reference counterpart; works on a machine without a GPU).  problem[KINET_RWP_FIELDS], indexed by the
 * enum below: kind 0 = kinet_gemm(_ex) / kinet_gemm_headmajor* (once the call reaches the
 * resident-weight dispatch: no split-K, flag 4 clear), 1 = kinet_conv2d(_ex) of a convolution that is
 * not a plain GEMM (the direct 3x3 and stem kernels are asked before it), 2 = kinet_msda_sample_records
 * (N = heads * 48, output f16).  Dtypes are kinet_dtypes; RESIDUAL / LN / A2 / ROW_MASK say whether the
 * operand is given, *_ALIGNED whether its pointer is 16-byte aligned; HM_* are rows_per_batch, head_dim,
 * split_cols and tail_dim of a head-major store (0 otherwise); CIN .. WOUT the convolution geometry
 * (STRIDE / PAD vertical).  cus: the compute-unit count to plan for (256 on MI355X).  Reads the calling
 * thread's kinet_gemm_set_flags and kinet_gemm_rw_grid_cap like a real call.  *eligible = 0 / 1;
 * config[0 .. 14] = the record kinet_gemm_rw_last_config would return after the launch (zeros if not
 * eligible). */
enum {
    KINET_RWP_KIND, KINET_RWP_M, KINET_RWP_N, KINET_RWP_K, KINET_RWP_IN_DTYPE, KINET_RWP_OUT_DTYPE, KINET_RWP_RESIDUAL,
    KINET_RWP_LN, KINET_RWP_A2, KINET_RWP_LDC, KINET_RWP_LDR, KINET_RWP_C_ALIGNED, KINET_RWP_R_ALIGNED,
    KINET_RWP_A2_ALIGNED, KINET_RWP_HM_ROWS, KINET_RWP_HM_D, KINET_RWP_HM_SPLIT, KINET_RWP_HM_D2, KINET_RWP_CIN,
    KINET_RWP_KW, KINET_RWP_STRIDE, KINET_RWP_STRIDE_W, KINET_RWP_PAD, KINET_RWP_PAD_W, KINET_RWP_WIN, KINET_RWP_WOUT,
    KINET_RWP_ROW_MASK, KINET_RWP_FIELDS
};
int kinet_gemm_rw_plan(const int* problem, int cus, int* eligible, int* config);

/* Smallest a2_rows (rows of an A2 shared by every frame of the batch) kinet_gemm_headmajor_ex and
 * kinet_msda_sample_records accept: the tallest row tile of a resident-weight variant with an A2,
 * whose addressing lets a tile wrap around the A2 rows at most once (32). */
int kinet_gemm_rw_min_a2_rows(void);

/* C / R alignment: the fused epilogue moves 4 output elements per access whenever ldc (and ldr)
 * are multiples of 4, so kinet_gemm(_ex), kinet_gemm_headmajor* and kinet_conv2d(_ex) return
 * KINET_ERR_ARG for a C (or R) that is not aligned to 4 output elements in that case; other
 * strides, and the split-K forms (element-wise finalize), need element alignment only. */

/* Launch-fill policy (no reference counterpart), process-wide.  1 = "solo": the caller keeps one
 * batch in flight, so no other stream's work fills CUs a launch leaves idle -- shapes whose
 * default tiles cover under 60 % of one round of workgroups per CU (config 5's stage-3 3x3
 * convolutions and D = 256 bottleneck pairs, M = 32,640 rows) switch to tiles half as tall that
 * fill the chip: config 5 on one stream 239 -> 257 frames/s.  0 (default) = throughput mode:
 * with several batches in flight the other streams fill those CUs and the taller tiles' better
 * per-CU efficiency wins (config 5 on 3 streams 294 vs 290 frames/s).  Same outputs bit for bit
 * either way.  Returns the previous policy. */
int kinet_set_solo_launch(int on);

#ifdef __cplusplus
}
#endif

#endif /* KINET_GEMM_H_ */
