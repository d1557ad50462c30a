/* kinet_amd C-ABI: the criterion's `enc_outputs` set of two-stage Deformable DETR (detr.py:870-886)
 * -- the one prediction set with a row per encoder token -- and the two differentiable glue
 * kernels of the proposal stage (deformable_transformer.py:118-121, :185).
 * Conventions: include/kinet_common.h (caller's stream, no allocation, no sync, int status).
 * Every reduction runs in an order fixed by the shapes (no float atomics): reruns are bit-identical.
 */
#ifndef KINET_CRITERION_H_
#define KINET_CRITERION_H_

#include "kinet_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The block-diagonal Hungarian cost of one prediction set with the focal class cost
 * (matcher.py:135-171):
 *   logits (B, Q, C) f32, boxes (B, Q, 4) f32 cxcywh (16-byte aligned), tgt_labels (T) int64 in
 *   [0, C), tgt_boxes (T, 4) f32 cxcywh (16-byte aligned), tgt_start (B + 1) int32 ON THE DEVICE,
 *   non-decreasing, tgt_start[0] = 0, tgt_start[B] = T: image b owns columns
 *   [tgt_start[b], tgt_start[b + 1]).
 *   cost (Q, T) f32 row-major: cost[q, j] = w_bbox * L1(boxes[b, q], tgt_boxes[j])
 *     + w_class * (pos - neg)(sigmoid(logits[b, q, tgt_labels[j]]))
 *     + w_giou * -GIoU(xyxy(boxes[b, q]), xyxy(tgt_boxes[j]))          for the image b that owns j,
 *   pos(p) = alpha (1 - p)^gamma (-log(p + 1e-8)), neg(p) = (1 - alpha) p^gamma (-log(1 - p + 1e-8));
 *   1 - p is formed without cancellation.  A label outside [0, C) gives a NaN column.
 * boxes_ok (one device byte, or NULL): set to 1, then cleared when any of the B*Q prediction boxes
 * or T target boxes fails x1 >= x0 or y1 >= y0 in xyxy form (util/box_ops.py:44-45; a NaN box
 * fails).  T == 0: no launch, boxes_ok untouched, status 0.  gamma >= 0. */
int kinet_match_cost_focal(const float* logits, const float* boxes, const int64_t* tgt_labels,
                           const float* tgt_boxes, const int* tgt_start, float* cost, uint8_t* boxes_ok, int B,
                           int Q, int C, int T, float w_class, float w_bbox, float w_giou, float alpha, float gamma,
                           kinet_stream_t stream);

/* Sigmoid focal classification loss of a prediction set with sparse positives (detr.py:645-703,
 * util/misc.py:634-665):  loss = inv_num_boxes * sum_{r, c} focal(logits[r, c], [(r, c) positive]),
 *   focal(x, t) = alpha_t * bce(x, t) * (1 - p_t)^gamma,  bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|)),
 *   alpha_t = alpha t + (1 - alpha)(1 - t), or 1 when alpha < 0.
 * logits (R, C) f32, 16-byte aligned; the positives are the n >= 0 pairs (pos_rows[i], pos_cls[i])
 * (int64, device; NULL when n == 0), every pair different, rows in [0, R), classes in [0, C) -- a
 * pair outside is ignored.  No one-hot and no (R, C) temporary in either direction; every element
 * is summed once, with its own target (a workgroup first collects the positives of its range).
 * Forward: one f32 at `loss`; workspace: kinet_focal_set_loss_workspace(R, C) floats (block
 * partials, summed in block order).  R * C == 0 writes 0. */
int64_t kinet_focal_set_loss_workspace(int64_t R, int C);
int kinet_focal_set_loss(const float* logits, const int64_t* pos_rows, const int64_t* pos_cls, float* loss,
                         int64_t R, int C, int n, float alpha, float gamma, float inv_num_boxes, float* workspace,
                         kinet_stream_t stream);
/* dlogits (R, C) f32 (16-byte aligned) = dloss[0] * d loss / d logits; dloss one f32 on the device. */
int kinet_focal_set_loss_backward(const float* logits, const int64_t* pos_rows, const int64_t* pos_cls,
                                  const float* dloss, float* dlogits, int64_t R, int C, int n, float alpha,
                                  float gamma, float inv_num_boxes, kinet_stream_t stream);

/* y[r, :] = keep[r] ? x[r, :] : 0 (deformable_transformer.py:118-121: the memory rows of padded and
 * out-of-range tokens are zeroed before enc_output), f32 rows of d floats, d % 4 == 0, x and y
 * 16-byte aligned (y may be x).  A dropped row is exactly 0 whatever x holds.  Applied to the
 * gradient it is its own backward. */
int kinet_two_stage_mask_rows(const float* x, const uint8_t* keep, float* y, int64_t rows, int d,
                              kinet_stream_t stream);

/* Backward of kinet_two_stage_boxes (kinet_two_stage.h) w.r.t. tmp:
 *   d_tmp = d_boxes * b * (1 - b) + d_coord_unact,   b = the forward's boxes, all (rows, 4) f32,
 * 16-byte aligned.  Either of d_boxes / d_coord_unact may be NULL (not both).  Where b * (1 - b) is 0
 * (b == 1: the +inf proposals) the first term is exactly 0 whatever d_boxes holds: no NaN. */
int kinet_two_stage_boxes_backward(const float* d_boxes, const float* d_coord_unact, const float* boxes,
                                   float* d_tmp, int64_t rows, kinet_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* KINET_CRITERION_H_ */
