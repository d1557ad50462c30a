/* kinet_amd C-ABI: the segmentation head of DeformableDETRSegm (detr_segmentation.py: MHAttentionMap
 * :181-216, MaskHeadSmallConv :105-178, PostProcessSegm :219-253).
 * dtype codes and conventions: include/kinet_common.h (caller's stream, caller-provided workspaces,
 * no allocation, no synchronisation, argument errors before any launch).  Activations are NHWC.
 * Rows of a per-query tensor are frame-major: row r = b*Q + q belongs to frame r / Q.  The
 * entry points that broadcast a per-frame operand take `row0`, the global index of their first
 * row, so the head can run over any chunk of rows: nothing reduces across rows, and every
 * reduction inside a row runs in a fixed order, so the result does not depend on the chunking
 * and reruns are bit-identical.
 */
#ifndef KINET_SEGM_H_
#define KINET_SEGM_H_

#include "kinet_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MHAttentionMap.forward after its two projections (:203-214):
 *   out[r, p, n] = softmax over all (n, p) of  scale * qp[r, n*D:(n+1)*D] . kp[b, p, n*D:(n+1)*D]
 * with D = d / heads, b = r / Q, and -inf (so exactly 0 on output) where mask[b, p] != 0 -- ONE
 * softmax jointly over the heads x HW logits of a row, not one per head.  A row whose pixels are
 * all masked is NaN, as in torch.
 * qp (B*Q, d), kp (B, HW, d), out (B*Q, HW, heads) in `dtype` (F32 / BF16 / F16), f32 arithmetic;
 * mask (B, HW) bytes or NULL.  d <= 1024, d % heads == 0, heads in {1, 2, 4, 8, 16, 32}.
 * Two passes over the keys (max and sum online, then the normalised values): no logit buffer. */
int kinet_segm_attention(const void* qp, const void* kp, const uint8_t* mask, void* out, int B, int Q, int HW,
                         int heads, int d, float scale, int dtype, kinet_stream_t stream);

/* lay1 of the mask head (:144-146) on [src | attention] without the concatenation: the
 * convolution is linear, so
 *   y[r] = frame[(row0 + r) / Q] + conv3x3_pad1(att[r]; w_att)
 * where frame (B, H, W, Cout) f32 = conv3x3(src; W[:, :d]) + bias is computed once per frame
 * (kinet_conv2d) and w_att (3, 3, Ca, Cout) f32 holds W[:, d:] with w_att[ky][kx][ci][co] =
 * W[co][d + ci][ky][kx].  att (rows, H, W, Ca) and y (rows, H, W, Cout) in `dtype`; f32 FMAs in
 * the order frame, then (ky, kx, ci).  Ca == 8 (the reference's nheads), Cout <= 512;
 * row0 + rows <= B*Q, rows <= 65535 per call. */
int kinet_segm_lay1(const void* att, const float* w_att, const float* frame, void* y, int rows, int row0, int Q,
                    int B, int H, int W, int Ca, int Cout, int dtype, kinet_stream_t stream);

/* GroupNorm + ReLU of the head (:147-175), optionally followed by the nearest upsampling and the
 * FPN add (:153-156, :161-164, :169-172):
 *   y[r][Y, X, c] = (f ? f[(row0 + r) / Q][Y, X, c] : 0) + relu(GN_groups(x[r]))[sy(Y), sx(X), c]
 * with torch's legacy mode="nearest" rule, sy(Y) = min(floorf(Y * ((float)h / H)), h - 1).
 * x (rows, h, w, C), y (rows, H, W, C), f (B, H, W, C) or NULL, all in `dtype`; gamma / beta f32;
 * statistics per row over (h*w, C / groups) in f32, taken of x - pivot (the rule of
 * kinet_groupnorm) in a fixed order.  C % 8 == 0 (a thread moves 8 channels: x, y, f 16-byte
 * aligned), C <= 2048, groups <= 128; C / groups may be any size (264 / 8 = 33, a vector then spans
 * two groups).  Without f, (H, W) must equal (h, w).  rows <= 65535 per call.
 * ws: kinet_segm_gn_workspace(rows, h*w, groups) floats. */
long kinet_segm_gn_workspace(int rows, int hw, int groups);
int kinet_segm_gn_relu_up_add(const void* x, const float* gamma, const float* beta, const void* f, void* y,
                              int rows, int row0, int Q, int B, int h, int w, int H, int W, int C, int groups,
                              float eps, int dtype, float* ws, kinet_stream_t stream);

/* out_lay (:177): 3x3, pad 1, C -> 1 channel, a direct kernel (an N = 1 implicit GEMM wastes a
 * tile).  x (rows, H, W, C) in `dtype`, wt (3, 3, C) f32 with wt[ky][kx][c] = W[0][c][ky][kx],
 * bias one f32 on the device; y (rows, H, W) f32 = bias + sum over (ky, kx, c) in that order.
 * C <= 64. */
int kinet_segm_out_conv(const void* x, const float* wt, const float* bias, float* y, int rows, int H, int W, int C,
                        int dtype, kinet_stream_t stream);

/* PostProcessSegm.forward (:224-253) for one frame, without the full-resolution intermediate:
 *   p = sigmoid(bilinear_{align_corners=False}(logits -> (max_h, max_w)))[:img_h, :img_w]
 *   out = nearest(p -> (oh, ow))       as uint8 (p > threshold), or as f32 p with return_probs
 * logits (Q, h, w) f32; out (Q, oh, ow).  img_h <= max_h, img_w <= max_w.  The bilinear and
 * nearest index rules are torch's (area_pixel_compute_source_index, legacy nearest). */
int kinet_segm_postprocess(const float* logits, void* out, int Q, int h, int w, int max_h, int max_w, int img_h,
                           int img_w, int oh, int ow, float threshold, int return_probs, kinet_stream_t stream);

/* Tracker masks (the reference tracker's stack / argmax / compare, tracker.py:515-527) for one frame,
 * without the per-track probability maps: every output pixel gets the slot of the track that owns it.
 *   p_t = fresh slot (src[t] >= 0):  the probability kinet_segm_postprocess gives row src[t] of logits
 *         stale slot (src[t] <  0):  1.0f where prev_labels[Y, X] == -src[t]-1, else 0.0f
 *   best = the first t of maximal p_t (torch.argmax: NaN is the greatest, the first occurrence wins)
 *   labels[Y, X] = p_best > threshold ? best : -1
 * so track slot t's exclusive mask is labels == t.  A stale slot is a track that kept last frame's
 * resolved bool mask: torch.stack promotes it to 1.0 / 0.0 among the fresh probabilities.
 * logits (n, h, w) f32 (NULL when n == 0); src T ints on the device (NULL when T == 0); prev_labels
 * (oh, ow) int16 or NULL (every stale slot is then empty); labels (oh, ow) int16, another buffer
 * than prev_labels.  T <= 32767; T == 0 writes -1 everywhere.  A fresh slot >= n counts as 0.0 and
 * reads nothing.  Every pixel is local: reruns are bit-identical. */
int kinet_segm_track_resolve(const float* logits, const int32_t* src, const int16_t* prev_labels, int16_t* labels,
                             int T, int n, int h, int w, int max_h, int max_w, int img_h, int img_w, int oh, int ow,
                             float threshold, kinet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Ragged rows (the multi-sequence tracker's masks): the kept rows of several frames in one call.
 * The three entry points above that broadcast a per-frame operand have a twin that takes
 * `row_frame`, a DEVICE list of one int32 per row of the call: row r reads frame row_frame[r]
 * where the frame-major entry point reads frame (row0 + r) / Q.  The kernels are the same (one
 * body; the frame-major entry points pass NULL), so a row's result is bit-identical to what the
 * frame-major call gives that row.  The list lives on the device, so the kernels guard it: a row
 * whose entry is outside [0, B) reads nothing through it and its output row is left untouched.
 * All other limits are those of the twin.
 * ------------------------------------------------------------------------------------------- */

/* kinet_segm_attention over gathered rows: qp (rows, d), kp (B, HW, d), mask (B, HW) or NULL,
 * out (rows, HW, heads). */
int kinet_segm_attention_rows(const void* qp, const void* kp, const uint8_t* mask, const int32_t* row_frame, void* out,
                              int rows, int B, int HW, int heads, int d, float scale, int dtype, kinet_stream_t stream);

/* kinet_segm_lay1: y[r] = frame[row_frame[r]] + conv3x3_pad1(att[r]; w_att). */
int kinet_segm_lay1_rows(const void* att, const float* w_att, const float* frame, const int32_t* row_frame, void* y,
                         int rows, int B, int H, int W, int Ca, int Cout, int dtype, kinet_stream_t stream);

/* kinet_segm_gn_relu_up_add with f[row_frame[r]] as the FPN operand.  Without f nothing is read per
 * frame: row_frame may be NULL and is not looked at.  ws: kinet_segm_gn_workspace(rows, h*w, groups). */
int kinet_segm_gn_relu_up_add_rows(const void* x, const float* gamma, const float* beta, const void* f,
                                   const int32_t* row_frame, void* y, int rows, int B, int h, int w, int H, int W, int C,
                                   int groups, float eps, int dtype, float* ws, kinet_stream_t stream);

/* kinet_segm_track_resolve for S sequences in one launch, with each slot's pixel count and box.
 * Sequence s owns the slots src[src_off[s] .. src_off[s+1]-1] (entries as above: >= 0 a row of the
 * shared logits (n, h, w), < 0 the stale slot -e-1 of ITS previous map), the frame geometry
 * geom[s] = (img_h, img_w, oh, ow) inside the one padded (max_h, max_w), the (oh, ow) label map at
 * labels + pix_off[s] (elements; pix_off[s+1] - pix_off[s] >= oh*ow) and its previous map at
 * prev_labels + prev_off[s] (prev_off[s] < 0: none, every stale slot is then empty).  labels and
 * prev_labels are two buffers.
 *   labels: per pixel the LOCAL slot t - src_off[s] that owns it or -1, exactly what
 *           kinet_segm_track_resolve writes for that sequence alone (the same device functions);
 *   stats (total, 5) int32: per slot (count, x0, y0, x1, y1), the number of pixels that carry its
 *           label and their half-open box; (0, 0, 0, 0, 0) for a slot without a pixel.
 * src, logits, labels, prev_labels, stats are DEVICE buffers; src_off (S + 1) int32, geom (S, 4)
 * int32, pix_off (S + 1) int64 and prev_off (S) int64 are HOST arrays (checked here, before any
 * launch, and handed to the kernel as arguments, RESOLVE_SEGS = 32 segments per launch: S <= 32
 * is one resolve launch, more take ceil(S / 32)).  A segment holds at most 32767 slots and may be
 * empty (its map is all -1); a segment with oh*ow == 0 has no map and nothing of it is touched.
 * A fresh entry >= n counts as 0.0 and reads nothing.  S == 0, or no slot and no pixel, launches
 * nothing.
 * The statistics are integer counts and extrema: the first 256 slots of a segment gather in an LDS
 * table per workgroup (LDS integer atomics) and merge into stats with global integer atomics,
 * later slots use global atomics directly; integer add / min / max commute, so reruns are
 * bit-identical.  stats is cleared by a memset before and finished by a small kernel after the
 * resolve launch (both on `stream`).  No float atomics.
 * Callers that want one device -> host copy put stats (20 bytes per slot) and labels into one
 * allocation, stats first. */
int kinet_segm_track_resolve_segments(const float* logits, const int32_t* src, const int32_t* src_off,
                                      const int32_t* geom, const int64_t* pix_off, const int16_t* prev_labels,
                                      const int64_t* prev_off, int16_t* labels, int32_t* stats, int S, int total, int n,
                                      int h, int w, int max_h, int max_w, float threshold, kinet_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mask training (csrc/segm_train.hip): the fused mask losses and the backward of the head's own
 * ops.  f32 only (the training path is f32).  No float atomics; every sum is taken in an order
 * fixed by the shapes alone, so reruns are bit-identical.
 * ------------------------------------------------------------------------------------------- */

/* loss_masks (detr.py:763-791) without the full-resolution intermediate:
 *   v = bilinear_{align_corners=False}(logits -> (H, W)),  p = sigmoid(v),  t = target != 0
 *   sums[r] = { sum focal(v, t),  sum p*t,  sum p,  sum t }  over all H*W pixels of row r, with
 *   focal = alpha_t * BCEWithLogits(v, t) * (1 - p_t)^gamma  (util/misc.py:634-665; alpha < 0: no alpha_t)
 *   loss[0] = sum_r sums[r][0] / (H*W) / num_boxes
 *   loss[1] = sum_r (1 - (2*sums[r][1] + 1) / (sums[r][2] + sums[r][3] + 1)) / num_boxes      (dice_loss :616-631)
 * logits (n, h, w) f32, target (n, H, W) bytes, sums (n, 4) f32, loss 2 f32 on the device.
 * The bilinear source index is torch's area_pixel_compute_source_index, the rule of
 * kinet_segm_postprocess.  H >= h and W >= w (ratios >= 1, integer or not); gamma must be 2.
 * n == 0 writes loss = {0, 0} with a memset and launches nothing.  A thread owns runs of 4
 * consecutive target bytes (one 32-bit load where the run lies inside the row); the rows' sums are
 * block partials in ws, added in block order.
 * ws: kinet_segm_mask_loss_workspace(n, H, W) floats. */
long kinet_segm_mask_loss_workspace(int n, int H, int W);
int kinet_segm_mask_loss(const float* logits, const uint8_t* target, float* sums, float* loss, int n, int h, int w,
                         int H, int W, float alpha, float gamma, float num_boxes, float* ws, kinet_stream_t stream);

/* Backward of kinet_segm_mask_loss: dlogits (n, h, w) = d(dloss[0]*loss[0] + dloss[1]*loss[1]) / dlogits,
 * from the forward's inputs and its `sums` (the dice quotient's derivative needs the row sums);
 * dloss 2 f32 on the device.  A gather: one thread per low-resolution pixel walks the
 * full-resolution pixels whose bilinear taps include it (found with the forward's index
 * function, so the two agree on every tap), forms the analytic derivative of both losses there
 * and adds it with the tap's weight, rows then columns ascending.  No workspace. */
int kinet_segm_mask_loss_backward(const float* logits, const uint8_t* target, const float* sums, const float* dloss,
                                  float* dlogits, int n, int h, int w, int H, int W, float alpha, float gamma,
                                  float num_boxes, kinet_stream_t stream);

/* Backward of kinet_segm_attention (f32): with s[r] = sum over (p, n) of att*datt in a fixed order,
 *   dl[r, p, n] = att[r, p, n] * (datt[r, p, n] - s[r])          (exactly 0 where att is 0: masked pixels)
 *   dqp[r, n*D + k] = scale * sum_p dl[r, p, n] * kp[b, p, n*D + k]              (p ascending)
 *   dkp[b, p, n*D + k] = scale * sum_{r in frame b, ascending} dl[r, p, n] * qp[r, n*D + k]
 * att, datt (B*Q, HW, heads); qp, dqp (B*Q, d); kp, dkp (B, HW, d).  dqp or dkp may be NULL (not
 * wanted).  Limits of kinet_segm_attention.  ws: kinet_segm_attention_backward_workspace(B, Q) floats. */
long kinet_segm_attention_backward_workspace(int B, int Q);
int kinet_segm_attention_backward(const float* datt, const float* att, const float* qp, const float* kp, float* dqp,
                                  float* dkp, int B, int Q, int HW, int heads, int d, float scale, float* ws,
                                  kinet_stream_t stream);

/* ReLU + nearest upsample + FPN add of the training head (kinet_segm_gn_relu_up_add without the
 * GroupNorm, which the training path runs as its own Function), f32:
 *   y[r][Y, X, c] = (f ? f[(row0 + r) / Q][Y, X, c] : 0) + relu(x[r])[sy(Y), sx(X), c]
 * with the legacy-nearest rule sy(Y) = min(floorf(Y * ((float)h / H)), h - 1).  x (rows, h, w, C),
 * y (rows, H, W, C), f (B, H, W, C) or NULL ((H, W) must then equal (h, w)).  C % 4 == 0, H >= h,
 * W >= w, row0 + rows <= B*Q. */
int kinet_segm_relu_up_add(const float* x, const float* f, float* y, int rows, int row0, int Q, int B, int h, int w,
                           int H, int W, int C, kinet_stream_t stream);

/* Its backward:
 *   dx[r][y, x, c] = [x[r][y, x, c] > 0] * sum of dy[r][Y, X, c] over the (Y, X) with (sy(Y), sx(X)) = (y, x),
 *                    Y then X ascending (a gather: the children are found with the forward's rule)
 *   df[b][Y, X, c] = sum of dy[r][Y, X, c] over the call's rows of frame b, ascending; 0 for a frame
 *                    without a row in [row0, row0 + rows)
 * dx or df may be NULL (not wanted).  dx depends on its own row only, so it does not depend on
 * how the rows are split over calls; df is the sum over THIS call's rows. */
int kinet_segm_relu_up_add_backward(const float* dy, const float* x, float* dx, float* df, int rows, int row0, int Q,
                                    int B, int h, int w, int H, int W, int C, kinet_stream_t stream);

/* Backward of kinet_segm_out_conv (f32): dy (rows, H, W), x (rows, H, W, C), wt (3, 3, C);
 *   dx[r][y, x, c] = sum over (ky, kx) of dy[r][y - ky + 1, x - kx + 1] * wt[ky][kx][c]
 *   dwt[ky][kx][c] = sum over (r, Y, X) of dy[r][Y, X] * x[r][Y + ky - 1, X + kx - 1, c]
 *   dbias          = sum of dy
 * dwt and dbias are two-stage: per-block partials in ws (a block owns a contiguous run of
 * pixels, its threads' sums added in thread order), then the blocks in order.  dx, or dwt with
 * dbias, may be NULL (not wanted).  C <= 64.  ws: kinet_segm_out_conv_backward_workspace(rows, H, W, C) floats. */
long kinet_segm_out_conv_backward_workspace(int rows, int H, int W, int C);
int kinet_segm_out_conv_backward(const float* dy, const float* x, const float* wt, float* dx, float* dwt,
                                 float* dbias, int rows, int H, int W, int C, float* ws, kinet_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* KINET_SEGM_H_ */
