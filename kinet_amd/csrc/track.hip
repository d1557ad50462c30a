// The multi-sequence tracker's per-frame device work (include/kinet_track.h): post-process +
// threshold decisions, segmented NMS, the track bank's commit / gather and the re-identification
// distances, each one launch for all sequences.  f32 throughout, no atomics: every output element
// has one writer and a fixed summation order, so reruns are bit-identical.
#include "common.h"
#include "nms_rule.h"
#include "../../include/kinet_track.h"

namespace kinet {
namespace {

constexpr int TRACK_MAX = KINET_TRACK_MAX_ROWS;   // == NMS_MAX of ops.hip

// ---------------------------------------------------------------------------------
// decide: one thread per (sequence, row)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void track_decide_kernel(
    const float* __restrict__ logits, const float* __restrict__ pboxes, const float* __restrict__ sizes,
    const int* __restrict__ n_active, const int* __restrict__ n_inactive, float* __restrict__ boxes,
    float* __restrict__ scores, int* __restrict__ labels, uint8_t* __restrict__ dec, int S, int N, int C, int Kmax,
    float t_track, float t_reid, float t_det, int clip) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= S * N) return;
    const int s = g / N, r = g - s * N;
    const int k = n_active[s] + n_inactive[s];
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    float score = 0.f;
    int label = 0;
    uint8_t d = 0;
    if (!(r >= k && r < Kmax)) {   // not a placeholder (rows >= Kmax are the object queries)
        const float* lg = logits + (long)g * C;
        float best = 1.f / (1.f + expf(-lg[0]));
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float p = 1.f / (1.f + expf(-lg[c]));
            // torch.max: the first maximum, a NaN counts as the largest value
            if (p > best || (p != p && best == best)) best = p, arg = c;
        }
        score = best;
        label = arg;
        const float h = sizes[2 * s], w = sizes[2 * s + 1];
        const float cx = pboxes[4 * (long)g], cy = pboxes[4 * (long)g + 1];
        const float bw = pboxes[4 * (long)g + 2], bh = pboxes[4 * (long)g + 3];
        box.x = (cx - 0.5f * bw) * w;
        box.y = (cy - 0.5f * bh) * h;
        box.z = (cx + 0.5f * bw) * w;
        box.w = (cy + 0.5f * bh) * h;
        if (clip) {
            // clamp(min=0, max=w): fmaxf / fminf would drop a NaN, torch keeps it
            auto clampf = [](float v, float hi) { return v != v ? v : fminf(fmaxf(v, 0.f), hi); };
            box.x = clampf(box.x, w), box.z = clampf(box.z, w);
            box.y = clampf(box.y, h), box.w = clampf(box.w, h);
        }
        d = (score > t_track ? KINET_TRACK_DEC_TRACK : 0) | (score > t_reid ? KINET_TRACK_DEC_REID : 0) |
            (score > t_det ? KINET_TRACK_DEC_DET : 0) | (label == 0 ? KINET_TRACK_DEC_PERSON : 0);
    }
    reinterpret_cast<float4*>(boxes)[g] = box;
    scores[g] = score;
    labels[g] = label;
    dec[g] = d;
}

// ---------------------------------------------------------------------------------
// segmented NMS: nms_kernel of ops.hip on a list of bank rows, one workgroup per segment
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void nms_segments_kernel(
    const float* __restrict__ boxes, long box_stride, const float* __restrict__ scores, long score_stride,
    long bank_rows, const int* __restrict__ idx, const int* __restrict__ offsets, const uint8_t* __restrict__ inf_flag,
    uint8_t* __restrict__ keep, int total, float thresh) {
    __shared__ int order[TRACK_MAX];
    __shared__ uint32_t keys[TRACK_MAX];
    __shared__ int row[TRACK_MAX];
    __shared__ uint8_t supp[TRACK_MAX];
    __shared__ int cur;
    const int beg = offsets[blockIdx.x], end = offsets[blockIdx.x + 1];
    const int n = end - beg;
    if (beg < 0 || end > total || n <= 0 || n > TRACK_MAX) return;   // (uniform over the workgroup)
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int r = idx[beg + i];
        const bool ok = r >= 0 && r < bank_rows;
        row[i] = ok ? r : -1;
        // an entry outside the bank ranks last and is never kept
        keys[i] = !ok ? 0u : (inf_flag && inf_flag[beg + i]) ? nms_score_key(INFINITY)
                                                             : nms_score_key(scores[(long)r * score_stride]);
        supp[i] = ok ? 0 : 1;
        keep[beg + i] = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t si = keys[i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t sj = keys[j];
            r += (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        order[r] = i;
    }
    __syncthreads();
    for (int r = 0; r < n; ++r) {
        if (threadIdx.x == 0) cur = supp[order[r]] ? -1 : order[r];
        __syncthreads();
        const int i = cur;
        if (i >= 0) {
            if (threadIdx.x == 0) keep[beg + i] = 1;
            const float* a = boxes + (long)row[i] * box_stride;
            const float x1 = a[0], y1 = a[1], x2 = a[2], y2 = a[3];
            const float ai = (x2 - x1) * (y2 - y1);
            for (int k = r + 1 + threadIdx.x; k < n; k += blockDim.x) {
                const int j = order[k];
                if (row[j] < 0) continue;
                if (nms_suppresses(x1, y1, x2, y2, ai, boxes + (long)row[j] * box_stride, thresh)) supp[j] = 1;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------
// track bank: one wave per row
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void track_commit_kernel(
    const float* __restrict__ hs, const float* __restrict__ boxes, const float* __restrict__ scores, long frame_rows,
    const int* __restrict__ rows, const int* __restrict__ slots, float* __restrict__ bank, long capacity, int d) {
    const int r = rows[blockIdx.x], t = slots[blockIdx.x];
    if (r < 0 || r >= frame_rows || t < 0 || t >= capacity) return;
    float* dst = bank + (long)t * (d + 5);
    const float* src = hs + (long)r * d;
    for (int c = threadIdx.x; c < d; c += 64) dst[c] = src[c];
    if (threadIdx.x < 4) dst[d + threadIdx.x] = boxes[4 * (long)r + threadIdx.x];
    if (threadIdx.x == 4) dst[d + 4] = scores[r];
}

__global__ __launch_bounds__(64) void track_gather_kernel(
    const float* __restrict__ bank, long capacity, int d, const int* __restrict__ slots, const int* __restrict__ offsets,
    const float* __restrict__ sizes, float* __restrict__ embeds, float* __restrict__ boxes, uint8_t* __restrict__ mask,
    int Kmax, int Q) {
    const int s = blockIdx.x / Kmax, k = blockIdx.x - s * Kmax;
    const int beg = offsets[s];
    const int ks = min(max(offsets[s + 1] - beg, 0), Kmax);
    const int t = k < ks ? slots[beg + k] : -1;
    const bool live = t >= 0 && t < capacity;   // (a slot outside the bank reads as a placeholder)
    const float* src = bank + (long)(live ? t : 0) * (d + 5);
    float* e = embeds + (long)blockIdx.x * d;
    for (int c = threadIdx.x; c < d; c += 64) e[c] = live ? src[c] : 0.f;
    if (threadIdx.x == 0) {
        float4 b = make_float4(0.5f, 0.5f, 0.5f, 0.5f);
        if (live) {
            const float h = sizes[2 * s], w = sizes[2 * s + 1];
            const float x0 = src[d], y0 = src[d + 1], x1 = src[d + 2], y1 = src[d + 3];
            b = make_float4((x0 + x1) / 2.f / w, (y0 + y1) / 2.f / h, (x1 - x0) / w, (y1 - y0) / h);
        }
        reinterpret_cast<float4*>(boxes)[blockIdx.x] = b;
        mask[(long)s * (Kmax + Q) + k] = k >= ks ? 1 : 0;
    }
    if (k == 0)
        for (int q = threadIdx.x; q < Q; q += 64) mask[(long)s * (Kmax + Q) + Kmax + q] = 0;
}

// ---------------------------------------------------------------------------------
// re-identification distances: one wave per (inactive track, detection) pair
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void track_reid_dist_kernel(
    const float* __restrict__ bank, long capacity, const float* __restrict__ hs, long frame_rows, int d,
    const int* __restrict__ slots, const int* __restrict__ slot_off, const int* __restrict__ rows,
    const int* __restrict__ row_off, const int* __restrict__ out_off, float* __restrict__ out, int S) {
    const int e = blockIdx.x;
    int s = 0;
    while (s + 1 < S && out_off[s + 1] <= e) ++s;
    const int local = e - out_off[s];
    const int nb = row_off[s + 1] - row_off[s];
    const int na = slot_off[s + 1] - slot_off[s];
    if (local < 0 || nb <= 0 || local >= na * nb) return;
    const int t = slots[slot_off[s] + local / nb], r = rows[row_off[s] + local % nb];
    if (t < 0 || t >= capacity || r < 0 || r >= frame_rows) {
        if (threadIdx.x == 0) out[e] = INFINITY;   // never matched (reid_sim_threshold is finite)
        return;
    }
    const float* x = bank + (long)t * (d + 5);
    const float* y = hs + (long)r * d;
    float acc = 0.f;
    for (int c = threadIdx.x; c < d; c += 64) {
        const float v = x[c] - y[c] + 1e-6f;
        acc += v * v;
    }
    acc = group_reduce<64, false>(acc);
    if (threadIdx.x == 0) out[e] = sqrtf(acc);
}

}  // namespace
}  // namespace kinet

extern "C" int kinet_track_decide(const float* pred_logits, const float* pred_boxes, const float* sizes,
                                  const int* n_active, const int* n_inactive, void* out, int S, int N, int C, int Kmax,
                                  float track_thresh, float reid_thresh, float detection_thresh, int clip,
                                  kinet_stream_t stream) {
    using namespace kinet;
    KINET_CHECK_ARG(S >= 0 && C >= 1, "track_decide: S=%d C=%d", S, C);
    KINET_CHECK_ARG(N >= 0 && N <= TRACK_MAX, "track_decide: %d rows per sequence (at most %d)", N, TRACK_MAX);
    KINET_CHECK_ARG(Kmax >= 0 && Kmax <= N, "track_decide: Kmax=%d outside [0, N=%d]", Kmax, N);
    const long rows = (long)S * N;
    if (rows == 0) return KINET_OK;
    KINET_CHECK_ARG(pred_logits && pred_boxes && sizes && n_active && n_inactive && out, "track_decide: null pointer");
    KINET_CHECK_ARG(((uintptr_t)out & 15) == 0, "track_decide: out must be 16-byte aligned");
    KINET_CHECK_ARG(rows * (long)C < (1L << 31), "track_decide: S*N*C=%ld does not fit int32", rows * (long)C);
    float* boxes = (float*)out;
    float* scores = boxes + 4 * rows;
    int* labels = (int*)(scores + rows);
    uint8_t* dec = (uint8_t*)(labels + rows);
    hipLaunchKernelGGL(track_decide_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       pred_logits, pred_boxes, sizes, n_active, n_inactive, boxes, scores, labels, dec, S, N, C, Kmax,
                       track_thresh, reid_thresh, detection_thresh, clip);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_nms_segments(const float* boxes, int64_t box_stride, const float* scores, int64_t score_stride,
                                  int64_t bank_rows, const int* idx, const int* offsets, const uint8_t* inf_flag,
                                  uint8_t* keep, int S, int total, float iou_threshold, kinet_stream_t stream) {
    using namespace kinet;
    KINET_CHECK_ARG(S >= 0 && total >= 0, "nms_segments: S=%d total=%d", S, total);
    KINET_CHECK_ARG(box_stride >= 4 && score_stride >= 1 && bank_rows >= 0,
                    "nms_segments: box_stride=%ld score_stride=%ld bank_rows=%ld", (long)box_stride, (long)score_stride,
                    (long)bank_rows);
    if (S == 0 || total == 0) return KINET_OK;
    KINET_CHECK_ARG(boxes && scores && idx && offsets && keep, "nms_segments: null pointer");
    // a segment holds at most `total` entries: short lists run on a quarter of the workgroup
    hipLaunchKernelGGL(nms_segments_kernel, dim3(S), dim3(total <= 256 ? 256 : 1024), 0, (hipStream_t)stream, boxes,
                       (long)box_stride, scores, (long)score_stride, (long)bank_rows, idx, offsets, inf_flag, keep, total,
                       iou_threshold);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_track_commit(const float* hs_embed, const float* boxes, const float* scores, int64_t frame_rows,
                                  const int* rows, const int* slots, int n, float* bank, int64_t capacity, int d,
                                  kinet_stream_t stream) {
    using namespace kinet;
    KINET_CHECK_ARG(n >= 0 && d >= 1 && frame_rows >= 0 && capacity >= 0, "track_commit: n=%d d=%d frame_rows=%ld capacity=%ld",
                    n, d, (long)frame_rows, (long)capacity);
    if (n == 0) return KINET_OK;
    KINET_CHECK_ARG(hs_embed && boxes && scores && rows && slots && bank, "track_commit: null pointer");
    hipLaunchKernelGGL(track_commit_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, hs_embed, boxes, scores,
                       (long)frame_rows, rows, slots, bank, (long)capacity, d);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_track_gather(const float* bank, int64_t capacity, int d, const int* slots, const int* offsets,
                                  const float* sizes, float* embeds, float* boxes, uint8_t* mask, int S, int Kmax, int Q,
                                  kinet_stream_t stream) {
    using namespace kinet;
    KINET_CHECK_ARG(S >= 0 && d >= 1 && Q >= 0 && capacity >= 0, "track_gather: S=%d d=%d Q=%d capacity=%ld", S, d, Q,
                    (long)capacity);
    KINET_CHECK_ARG(Kmax >= 1 && (long)Kmax + Q <= TRACK_MAX, "track_gather: Kmax=%d + Q=%d rows (1 <= Kmax, at most %d rows)",
                    Kmax, Q, TRACK_MAX);
    if (S == 0) return KINET_OK;
    KINET_CHECK_ARG(bank && slots && offsets && sizes && embeds && boxes && mask, "track_gather: null pointer");
    KINET_CHECK_ARG(((uintptr_t)boxes & 15) == 0, "track_gather: boxes must be 16-byte aligned");
    hipLaunchKernelGGL(track_gather_kernel, dim3((unsigned)(S * Kmax)), dim3(64), 0, (hipStream_t)stream, bank,
                       (long)capacity, d, slots, offsets, sizes, embeds, boxes, mask, Kmax, Q);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_track_reid_dist(const float* bank, int64_t capacity, const float* hs_embed, int64_t frame_rows,
                                     int d, const int* slots, const int* slot_off, const int* rows, const int* row_off,
                                     const int* out_off, float* out, int S, int total, kinet_stream_t stream) {
    using namespace kinet;
    KINET_CHECK_ARG(S >= 0 && total >= 0 && d >= 1 && capacity >= 0 && frame_rows >= 0,
                    "track_reid_dist: S=%d total=%d d=%d capacity=%ld frame_rows=%ld", S, total, d, (long)capacity,
                    (long)frame_rows);
    if (S == 0 || total == 0) return KINET_OK;
    KINET_CHECK_ARG(bank && hs_embed && slots && slot_off && rows && row_off && out_off && out,
                    "track_reid_dist: null pointer");
    hipLaunchKernelGGL(track_reid_dist_kernel, dim3(total), dim3(64), 0, (hipStream_t)stream, bank, (long)capacity,
                       hs_embed, (long)frame_rows, d, slots, slot_off, rows, row_off, out_off, out, S);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}
