/* kinet_amd C-ABI: the proposal stage of two-stage Deformable DETR (deformable_transformer.py
 * :77-122, :180-194) -- encoder-output proposals, per-row top-k, query construction.
 * Conventions: include/kinet_common.h (caller's stream, no allocation, no sync, int status).
 */
#ifndef KINET_TWO_STAGE_H_
#define KINET_TWO_STAGE_H_

#include "kinet_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KINET_TWO_STAGE_MAX_LEVELS 16
#define KINET_TOPK_MAX_K 1024

/* gen_encoder_output_proposals (:92-116), the part that depends only on shapes and masks.
 * level_hw: HOST array of `levels` (H, W) pairs (1 <= levels <= 16, sum H*W == S);
 * mask (B, S) bytes, non-zero = padded, or NULL (nothing padded).
 * Per (frame, level) valid_H counts the unpadded entries of the level's first column and
 * valid_W those of its first row, as the reference does.  Token (i, j) of level l proposes
 *   (x, y, w, h) = ((j + 0.5) / valid_W, (i + 0.5) / valid_H, 0.05 * 2^l, 0.05 * 2^l)
 * in f32 with a correctly rounded division (the reference's torch arithmetic, bit for bit); it
 * is valid when all four lie in (0.01, 0.99) (f32 compares) and the token is not padded.
 *   proposals (B, S, 4) f32 = log(p / (1 - p)) on valid rows, +inf on every other row (no NaN);
 *   keep (B, S) bytes = 1 on valid rows, else 0. */
int kinet_two_stage_proposals(const int* level_hw, int levels, const uint8_t* mask, float* proposals,
                              uint8_t* keep, int B, int S, kinet_stream_t stream);

/* Per-row top-k of an f32 matrix read in place: element (r, i) at scores[r*row_stride +
 * i*elem_stride] (strides in elements; channel 0 of (B, S, C) logits is row_stride S*C,
 * elem_stride C).  out (rows, k) int64: the indices of the k largest entries of each row in
 * torch's descending order -- NaN first (every NaN equal), -0.0 == +0.0 -- ties broken by
 * ascending index, i.e. torch.sort(descending=True, stable=True)[1][:, :k].
 * 1 <= k <= 1024, k <= S <= 2^30; one workgroup per row. */
int kinet_topk_rows(const float* scores, int64_t row_stride, int64_t elem_stride, int rows, int S, int k,
                    int64_t* out, kinet_stream_t stream);

/* Gather + get_proposal_pos_embed (:77-90, :189-193) for the selected proposals:
 * coord_unact (B, S, 4) f32, idx (B, k) int64 in [0, S) (an index outside gives NaN rows),
 * dim_t (128 f32, device) = 10000 ** (2 * (f // 2) / 128) as the caller computes it.
 *   ref (B, k, 4) f32      = sigmoid(coord_unact[b, idx[b, q]])
 *   pos (B, k, 512) dtype  : pos[.., c*128 + f] = sin(ref_c * 2pi / dim_t[f]) for even f,
 *                            cos(ref_c * 2pi / dim_t[f]) for odd f (accurate sinf / cosf). */
int kinet_two_stage_queries(const float* coord_unact, const int64_t* idx, const float* dim_t, float* ref,
                            void* pos, int B, int S, int k, int dtype, kinet_stream_t stream);

/* y[r, :] = row[:] for every r with keep[r] == 0 (the enc_output rows whose input the reference
 * zeroes, :118-121: their output is one constant row).  y (rows, d) and row (d) in dtype,
 * 16-byte aligned, d * sizeof(dtype) a multiple of 16. */
int kinet_two_stage_fill_rows(void* y, const uint8_t* keep, const void* row, int64_t rows, int d, int dtype,
                              kinet_stream_t stream);

/* coord_unact = tmp + proposals, boxes = sigmoid(coord_unact) (:185, deformable_detr.py:258);
 * all (rows, 4) f32, 16-byte aligned.  A +inf proposal gives coord_unact +inf and a box of exactly 1. */
int kinet_two_stage_boxes(const float* tmp, const float* proposals, float* coord_unact, float* boxes,
                          int64_t rows, kinet_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* KINET_TWO_STAGE_H_ */
