/* kinet_amd C-ABI: the online tracker's per-frame device work, batched over S sequences that
 * advance in lock-step on one detector forward (kinet_amd.tracker.MultiTracker; the statements of
 * tracker.py:269-557 that touch device tensors).  All arithmetic is f32, no kernel uses atomics
 * and reruns are bit-identical.
 * Conventions: include/kinet_common.h (caller's stream, no allocation, no sync, int status).
 * Index lists live on the device, so the kernels guard them: an entry outside its table is
 * skipped (never read or written through), a segment longer than KINET_TRACK_MAX_ROWS is left
 * untouched.
 *
 * The track bank is a device table of `capacity` rows of (d + 5) f32: the track's last decoder
 * embedding (d), its box (x0, y0, x1, y1 in image pixels) and its score; a track owns one row
 * (its slot) from its first frame to its removal.
 */
#ifndef KINET_TRACK_H_
#define KINET_TRACK_H_

#include "kinet_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows of one sequence (Kmax track queries + Q object queries) and entries of one NMS segment */
#define KINET_TRACK_MAX_ROWS 4096

/* decision byte of kinet_track_decide */
#define KINET_TRACK_DEC_TRACK 1  /* score > track_thresh */
#define KINET_TRACK_DEC_REID 2   /* score > reid_thresh */
#define KINET_TRACK_DEC_DET 4    /* score > detection_thresh */
#define KINET_TRACK_DEC_PERSON 8 /* label == 0 */

/* DeformablePostProcess (deformable_detr.py:286-334) + clip_boxes_to_image + the tracker's four
 * compares (tracker.py:331-349) for S sequences of N = Kmax + Q rows each.
 *   pred_logits (S, N, C) f32, pred_boxes (S, N, 4) f32 cxcywh in [0, 1], sizes (S, 2) f32 (h, w),
 *   n_active, n_inactive (S) int32: sequence s holds K_s = n_active[s] + n_inactive[s] track
 *   queries in rows 0..K_s-1; rows K_s..Kmax-1 are placeholders.
 * Per row: p_c = 1 / (1 + exp(-logit_c)); score = max_c p_c, label = the first c that attains it;
 * box = (cx - w/2, cy - h/2, cx + w/2, cy + h/2) * (W, H, W, H), with clip != 0 clamped to
 * [0, W] x [0, H].  All three compares are strict.
 * out: one packed buffer of S*N*25 bytes,
 *   boxes (S, N, 4) f32 | scores (S, N) f32 | labels (S, N) int32 | decisions (S, N) bytes,
 * so one copy carries the frame for all sequences.  A placeholder row gets zeros in all four,
 * whatever its inputs hold.  N <= KINET_TRACK_MAX_ROWS, 0 <= Kmax <= N, C >= 1. */
int kinet_track_decide(const float* pred_logits, const float* pred_boxes, const float* sizes,
                       const int* n_active, const int* n_inactive, void* out, int S, int N, int C, int Kmax,
                       float track_thresh, float reid_thresh, float detection_thresh, int clip,
                       kinet_stream_t stream);

/* S independent greedy NMS problems (kinet_nms semantics: descending score, ties by position
 * in the list, NaN scores first, a box is dropped when its IoU with a kept higher-ranked box
 * exceeds iou_threshold), one workgroup per segment.  Segment s is the entries
 * offsets[s]..offsets[s+1]-1 of idx; entry e names row idx[e] of a shared bank whose box is at
 * boxes[idx[e] * box_stride .. +3] (xyxy) and whose score is at scores[idx[e] * score_stride]
 * (strides in f32 elements, so the track bank is read in place).  inf_flag (total bytes) or
 * NULL: a non-zero entry competes with score +inf (the detection NMS, where existing tracks
 * always win, tracker.py:519).  keep (total bytes): 1 for a kept entry, else 0; every entry of
 * every segment is written.  offsets (S + 1) int32 ascending with offsets[S] <= total; a
 * segment may be empty and holds at most KINET_TRACK_MAX_ROWS entries. */
int kinet_nms_segments(const float* boxes, int64_t box_stride, const float* scores, int64_t score_stride,
                       int64_t bank_rows, const int* idx, const int* offsets, const uint8_t* inf_flag,
                       uint8_t* keep, int S, int total, float iou_threshold, kinet_stream_t stream);

/* bank[slots[p]] = (hs_embed[rows[p]] | boxes[rows[p]] | scores[rows[p]]) for p < n: rows index
 * the frame's flattened (S*N) outputs -- hs_embed (frame_rows, d) f32, boxes (frame_rows, 4) and
 * scores (frame_rows) as kinet_track_decide wrote them.  A slot named twice takes one of its
 * rows (the caller names each once). */
int kinet_track_commit(const float* hs_embed, const float* boxes, const float* scores, int64_t frame_rows,
                       const int* rows, const int* slots, int n, float* bank, int64_t capacity, int d,
                       kinet_stream_t stream);

/* Next frame's track queries from per-sequence slot lists (tracker.py:287-307): sequence s names
 * slots[offsets[s]..offsets[s+1]-1] (K_s <= Kmax of them).
 *   embeds (S, Kmax, d) f32 = the slots' embeddings, zeros on rows k >= K_s;
 *   boxes (S, Kmax, 4) f32  = ((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0) / (W, H, W, H) with
 *                             sizes (S, 2) f32 (h, w), 0.5 on rows k >= K_s;
 *   mask (S, Kmax + Q) bytes = 1 on rows K_s..Kmax-1 (the placeholders), else 0.
 * 1 <= Kmax, Kmax + Q <= KINET_TRACK_MAX_ROWS. */
int kinet_track_gather(const float* bank, int64_t capacity, int d, const int* slots, const int* offsets,
                       const float* sizes, float* embeds, float* boxes, uint8_t* mask, int S, int Kmax, int Q,
                       kinet_stream_t stream);

/* Tracker.reid's embedding distances (tracker.py:236-244, F.pairwise_distance) for every
 * sequence at once: sequence s pairs its inactive tracks' slots
 * slots[slot_off[s]..slot_off[s+1]-1] (a of them) with the frame rows
 * rows[row_off[s]..row_off[s+1]-1] (b of them, indices into hs_embed (frame_rows, d)) and
 * writes the (a, b) row-major matrix ||bank_embed - hs_embed + 1e-6||_2 at out[out_off[s]..]
 * (out_off (S + 1) int32, out_off[s+1] - out_off[s] == a * b, out_off[S] == total), so one copy
 * carries all sequences. */
int kinet_track_reid_dist(const float* bank, int64_t capacity, const float* hs_embed, int64_t frame_rows, int d,
                          const int* slots, const int* slot_off, const int* rows, const int* row_off,
                          const int* out_off, float* out, int S, int total, kinet_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* KINET_TRACK_H_ */
