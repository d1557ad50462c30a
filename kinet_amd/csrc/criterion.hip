// The criterion's enc_outputs set of two-stage Deformable DETR (detr.py:870-886): the block-diagonal
// focal matcher cost and the sigmoid focal classification loss over every encoder token, plus the
// two differentiable glue kernels of the proposal stage (row masking, the box sigmoid's backward).
// C-ABI: include/kinet_criterion.h.  f32 only.  No float atomics: every sum runs in an order fixed
// by the shapes (thread-strided partials, a symmetric butterfly over the wave, the waves and then
// the blocks in index order), so reruns are bit-identical.
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>

#include "../../include/kinet_criterion.h"
#include "common.h"

namespace kinet {
namespace {

// Sum over the 256 threads of a block, the same value in every thread: butterfly over each wave
// (a + b is symmetric, so all lanes hold the same bits), then the four waves in order.
// red: 4 floats of LDS, free for reuse after the call.
__device__ __forceinline__ float block_sum(float v, float* red) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();   // (a previous call's readers are done)
    if (threadIdx.x % 64 == 0) red[threadIdx.x / 64] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// p = sigmoid(v), q = 1 - p (formed without the cancellation of 1 - p), softplus(v), softplus(-v)
struct LogitTerms {
    float p, q, sp_pos, sp_neg;
};

__device__ __forceinline__ LogitTerms logit_terms(float v) {
    const float e = expf(-fabsf(v));
    const float inv = 1.f / (1.f + e);
    const float l = log1pf(e);
    LogitTerms t;
    t.p = v >= 0.f ? inv : e * inv;
    t.q = v >= 0.f ? e * inv : inv;
    t.sp_pos = fmaxf(v, 0.f) + l;
    t.sp_neg = fmaxf(-v, 0.f) + l;
    return t;
}

// x^gamma for x in [0, 1]; gamma == 2 (every config) is a product, as torch's pow(x, 2.0)
__device__ __forceinline__ float pow_gamma(float x, float gamma) { return gamma == 2.f ? x * x : powf(x, gamma); }

// ---------------------------------------------------------------------------------
// block-diagonal matcher cost (matcher.py:135-171)
// ---------------------------------------------------------------------------------
constexpr int MC_ROWS = 16;   // prediction rows of a workgroup
constexpr int MC_COLS = 16;   // lanes along a row's target columns (64 B of contiguous cost per row)

__device__ __forceinline__ float4 to_xyxy(float4 b) {
    return make_float4(b.x - 0.5f * b.z, b.y - 0.5f * b.w, b.x + 0.5f * b.z, b.y + 0.5f * b.w);
}
__device__ __forceinline__ bool box_ok(float4 b) { return b.z >= b.x && b.w >= b.y; }

// grid (ceil(Q / MC_ROWS), B), block (MC_COLS, MC_ROWS): thread (tx, ty) owns prediction row
// q = blockIdx.x * MC_ROWS + ty of image b = blockIdx.y and every MC_COLS-th of the image's columns.
// Every prediction box is checked by the threads tx == 0 (also those of an image without targets),
// the image's target boxes by the workgroups blockIdx.x == 0.
__global__ __launch_bounds__(MC_ROWS* MC_COLS) void match_cost_focal_kernel(
    const float* __restrict__ logits, const float4* __restrict__ boxes, const int64_t* __restrict__ tgt_labels,
    const float4* __restrict__ tgt_boxes, const int* __restrict__ tgt_start, float* __restrict__ cost,
    uint8_t* __restrict__ boxes_ok, int Q, int C, int T, float w_class, float w_bbox, float w_giou, float alpha,
    float gamma) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * MC_ROWS + threadIdx.y;
    const int j0 = max(tgt_start[b], 0), j1 = min(tgt_start[b + 1], T);
    if (boxes_ok && blockIdx.x == 0) {
        for (int j = j0 + (int)(threadIdx.y * MC_COLS + threadIdx.x); j < j1; j += MC_ROWS * MC_COLS)
            if (!box_ok(to_xyxy(tgt_boxes[j]))) *boxes_ok = 0;
    }
    if (q >= Q) return;
    const long row = (long)b * Q + q;
    const float4 pc = boxes[row];
    const float4 pb = to_xyxy(pc);
    if (boxes_ok && threadIdx.x == 0 && !box_ok(pb)) *boxes_ok = 0;
    const float area1 = (pb.z - pb.x) * (pb.w - pb.y);
    const float* lg = logits + row * C;
    float* out = cost + (long)q * T;
    for (int j = j0 + (int)threadIdx.x; j < j1; j += MC_COLS) {
        const int64_t lab = tgt_labels[j];
        float c_class = __builtin_nanf("");
        if (lab >= 0 && lab < C) {
            const LogitTerms t = logit_terms(lg[lab]);
            const float neg = (1.f - alpha) * pow_gamma(t.p, gamma) * -logf(t.q + 1e-8f);
            const float pos = alpha * pow_gamma(t.q, gamma) * -logf(t.p + 1e-8f);
            c_class = pos - neg;
        }
        const float4 tc = tgt_boxes[j];
        const float c_bbox = ((fabsf(pc.x - tc.x) + fabsf(pc.y - tc.y)) + fabsf(pc.z - tc.z)) + fabsf(pc.w - tc.w);
        const float4 tb = to_xyxy(tc);
        const float area2 = (tb.z - tb.x) * (tb.w - tb.y);
        const float iw = fmaxf(fminf(pb.z, tb.z) - fmaxf(pb.x, tb.x), 0.f);
        const float ih = fmaxf(fminf(pb.w, tb.w) - fmaxf(pb.y, tb.y), 0.f);
        const float inter = iw * ih;
        const float uni = area1 + area2 - inter;
        const float iou = inter / uni;
        const float ew = fmaxf(fmaxf(pb.z, tb.z) - fminf(pb.x, tb.x), 0.f);
        const float eh = fmaxf(fmaxf(pb.w, tb.w) - fminf(pb.y, tb.y), 0.f);
        const float earea = ew * eh;
        const float giou = iou - (earea - uni) / earea;
        out[j] = w_bbox * c_bbox + w_class * c_class + w_giou * -giou;
    }
}

// ---------------------------------------------------------------------------------
// focal classification loss with sparse positives (detr.py:645-703)
// ---------------------------------------------------------------------------------
constexpr int FL_VEC_PER_BLOCK = 2048;   // float4 groups a block owns (8 per thread)
constexpr int FL_MAX_BLOCKS = 1024;

struct FocalAlpha {
    float a1, a0;   // alpha_t at t = 1 / t = 0
};
__device__ __forceinline__ FocalAlpha focal_alpha(float alpha) {
    FocalAlpha a;
    a.a1 = alpha >= 0.f ? alpha : 1.f;
    a.a0 = alpha >= 0.f ? 1.f - alpha : 1.f;
    return a;
}

// d/dx: t = 0: a0 p^gamma (p + gamma q softplus(x));  t = 1: -a1 q^gamma (q + gamma p softplus(-x))
__device__ __forceinline__ float dfocal_neg(float x, float a0, float gamma) {
    const LogitTerms t = logit_terms(x);
    return a0 * pow_gamma(t.p, gamma) * (t.p + gamma * t.q * t.sp_pos);
}
__device__ __forceinline__ float dfocal_pos(float x, float a1, float gamma) {
    const LogitTerms t = logit_terms(x);
    return -a1 * pow_gamma(t.q, gamma) * (t.q + gamma * t.p * t.sp_neg);
}

inline int focal_blocks(long total) {
    const long nvec = total / 4;
    const long per = std::max<long>(FL_VEC_PER_BLOCK, (nvec + FL_MAX_BLOCKS - 1) / FL_MAX_BLOCKS);
    return (int)std::max<long>(1, (nvec + per - 1) / per);
}

constexpr int FL_POS_CAP = 64;   // positives of one block's range kept in LDS (more: the global list is searched)

// The positives inside one block's element range [e0, e1): their flattened indices, in LDS.
struct BlockPositives {
    const long* lds;
    int count;   // may exceed FL_POS_CAP: then `lds` holds only the first FL_POS_CAP that arrived
    const int64_t *rows, *cls;
    int n, C;
    long R;
    __device__ __forceinline__ bool has(long flat) const {
        if (count == 0) return false;
        if (count <= FL_POS_CAP) {
            bool hit = false;
            for (int j = 0; j < count; ++j) hit |= lds[j] == flat;
            return hit;
        }
        bool hit = false;
        for (int i = 0; i < n; ++i)
            hit |= rows[i] >= 0 && rows[i] < R && cls[i] >= 0 && cls[i] < C && rows[i] * C + cls[i] == flat;
        return hit;
    }
};

__device__ __forceinline__ float focal_term(float x, bool t, FocalAlpha a, float gamma) {
    const LogitTerms lt = logit_terms(x);
    return t ? a.a1 * lt.sp_neg * pow_gamma(lt.q, gamma) : a.a0 * lt.sp_pos * pow_gamma(lt.p, gamma);
}

// block blk sums focal(x, t) over the float4 groups [blk * per, (blk + 1) * per) of the flattened
// logits, the last block also over the total % 4 trailing elements.  t = 1 at the positives: the
// block first collects those of its range (usually none) and every element is tested against them,
// so no term is added and taken back.  part[blk].
__global__ __launch_bounds__(256) void focal_set_loss_kernel(const float* __restrict__ logits,
                                                             const int64_t* __restrict__ pos_rows,
                                                             const int64_t* __restrict__ pos_cls, int n,
                                                             float* __restrict__ part, long R, int C, long per,
                                                             float alpha, float gamma) {
    __shared__ float red[4];
    __shared__ long spos[FL_POS_CAP];
    __shared__ int scount;
    const FocalAlpha a = focal_alpha(alpha);
    const long total = R * C, nvec = total / 4;
    const long v0 = (long)blockIdx.x * per, v1 = v0 + per < nvec ? v0 + per : nvec;
    const bool last = blockIdx.x == gridDim.x - 1;
    const long e0 = 4 * v0, e1 = last ? total : 4 * v1;
    if (threadIdx.x == 0) scount = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const int64_t r = pos_rows[i], k = pos_cls[i];
        if (r >= 0 && r < R && k >= 0 && k < C && r * C + k >= e0 && r * C + k < e1) {
            const int slot = atomicAdd(&scount, 1);   // (LDS integer counter: membership only, order-free)
            if (slot < FL_POS_CAP) spos[slot] = r * C + k;
        }
    }
    __syncthreads();
    BlockPositives bp{spos, scount, pos_rows, pos_cls, n, C, R};
    const float4* lv = reinterpret_cast<const float4*>(logits);
    float s = 0.f;
    for (long v = v0 + threadIdx.x; v < v1; v += 256) {
        const float4 x = lv[v];
        const long f = 4 * v;
        s += (focal_term(x.x, bp.has(f), a, gamma) + focal_term(x.y, bp.has(f + 1), a, gamma)) +
             (focal_term(x.z, bp.has(f + 2), a, gamma) + focal_term(x.w, bp.has(f + 3), a, gamma));
    }
    if (last && (long)threadIdx.x < total - 4 * nvec) {
        const long f = 4 * nvec + threadIdx.x;
        s += focal_term(logits[f], bp.has(f), a, gamma);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one block: the block partials (thread-strided, then the block's fixed-order sum), times 1 / num_boxes
__global__ __launch_bounds__(256) void focal_set_loss_finalize_kernel(const float* __restrict__ part, int nblk,
                                                                      float* __restrict__ loss, float inv_num_boxes) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = s * inv_num_boxes;
}

__global__ __launch_bounds__(256) void focal_set_loss_backward_kernel(const float* __restrict__ logits,
                                                                      const float* __restrict__ dloss,
                                                                      float* __restrict__ dlogits, long total,
                                                                      float alpha, float gamma, float inv_num_boxes) {
    const float a0 = focal_alpha(alpha).a0;
    const float g = dloss[0] * inv_num_boxes;
    const long nvec = total / 4;
    const float4* lv = reinterpret_cast<const float4*>(logits);
    float4* dv = reinterpret_cast<float4*>(dlogits);
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long)gridDim.x * 256) {
        const float4 x = lv[v];
        dv[v] = make_float4(g * dfocal_neg(x.x, a0, gamma), g * dfocal_neg(x.y, a0, gamma),
                            g * dfocal_neg(x.z, a0, gamma), g * dfocal_neg(x.w, a0, gamma));
    }
    if (blockIdx.x == 0 && (long)threadIdx.x < total - 4 * nvec) {
        const long i = 4 * nvec + threadIdx.x;
        dlogits[i] = g * dfocal_neg(logits[i], a0, gamma);
    }
}

// after the dense pass, on the same stream: the n positive entries take the t = 1 derivative
__global__ __launch_bounds__(256) void focal_set_loss_backward_pos_kernel(const float* __restrict__ logits,
                                                                          const int64_t* __restrict__ pos_rows,
                                                                          const int64_t* __restrict__ pos_cls, int n,
                                                                          const float* __restrict__ dloss,
                                                                          float* __restrict__ dlogits, long R, int C,
                                                                          float alpha, float gamma,
                                                                          float inv_num_boxes) {
    const float a1 = focal_alpha(alpha).a1;
    const float g = dloss[0] * inv_num_boxes;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int64_t r = pos_rows[i], k = pos_cls[i];
        if (r >= 0 && r < R && k >= 0 && k < C) dlogits[r * C + k] = g * dfocal_pos(logits[r * C + k], a1, gamma);
    }
}

// ---------------------------------------------------------------------------------
// proposal-stage glue
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_rows_kernel(const float4* __restrict__ x, const uint8_t* __restrict__ keep,
                                                        float4* __restrict__ y, long rows, int cpr) {
    const long n = rows * cpr;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x)
        y[t] = keep[t / cpr] ? x[t] : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ float sigmoid_grad_term(float d, float b) {
    const float s = b * (1.f - b);
    return s == 0.f ? 0.f : d * s;
}

__global__ __launch_bounds__(256) void boxes_backward_kernel(const float4* __restrict__ d_boxes,
                                                             const float4* __restrict__ d_unact,
                                                             const float4* __restrict__ boxes,
                                                             float4* __restrict__ d_tmp, long rows) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < rows; t += (long)gridDim.x * blockDim.x) {
        float4 o = d_unact ? d_unact[t] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (d_boxes) {
            const float4 d = d_boxes[t], b = boxes[t];
            o.x += sigmoid_grad_term(d.x, b.x);
            o.y += sigmoid_grad_term(d.y, b.y);
            o.z += sigmoid_grad_term(d.z, b.z);
            o.w += sigmoid_grad_term(d.w, b.w);
        }
        d_tmp[t] = o;
    }
}

int stride_grid(long n) {
    long g = (n + 255) / 256;
    if (g > kMaxGridStride) g = kMaxGridStride;
    return (int)(g < 1 ? 1 : g);
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace
}  // namespace kinet

using namespace kinet;

extern "C" int kinet_match_cost_focal(const float* logits, const float* boxes, const int64_t* tgt_labels,
                                      const float* tgt_boxes, const int* tgt_start, float* cost, uint8_t* boxes_ok,
                                      int B, int Q, int C, int T, float w_class, float w_bbox, float w_giou,
                                      float alpha, float gamma, kinet_stream_t stream) {
    KINET_CHECK_ARG(B >= 1 && B <= 65535 && Q >= 1 && C >= 1 && T >= 0,
                    "match_cost_focal: bad sizes B %d Q %d C %d T %d (1 <= B <= 65535, Q >= 1, C >= 1, T >= 0)", B, Q,
                    C, T);
    KINET_CHECK_ARG((long)Q * (long)std::max(T, 1) < (1L << 40), "match_cost_focal: Q * T too large");
    KINET_CHECK_ARG(gamma >= 0.f, "match_cost_focal: gamma must be >= 0");
    if (T == 0) return KINET_OK;
    KINET_CHECK_ARG(logits && boxes && tgt_labels && tgt_boxes && tgt_start && cost, "match_cost_focal: null pointer");
    KINET_CHECK_ARG(aligned16(boxes) && aligned16(tgt_boxes), "match_cost_focal: boxes must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    if (boxes_ok) KINET_CHECK_HIP(hipMemsetAsync(boxes_ok, 1, 1, s));
    const dim3 grid((unsigned)((Q + MC_ROWS - 1) / MC_ROWS), (unsigned)B), block(MC_COLS, MC_ROWS);
    hipLaunchKernelGGL(match_cost_focal_kernel, grid, block, 0, s, logits, (const float4*)boxes, tgt_labels,
                       (const float4*)tgt_boxes, tgt_start, cost, boxes_ok, Q, C, T, w_class, w_bbox, w_giou, alpha,
                       gamma);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int64_t kinet_focal_set_loss_workspace(int64_t R, int C) {
    if (R <= 0 || C <= 0) return 1;
    return focal_blocks((long)R * C);
}

static int focal_args(const char* who, const void* logits, const int64_t* pos_rows, const int64_t* pos_cls, int64_t R,
                      int C, int n, float gamma, float inv_num_boxes) {
    KINET_CHECK_ARG(R >= 0 && C >= 1 && n >= 0, "%s: bad sizes R %ld C %d n %d", who, (long)R, C, n);
    KINET_CHECK_ARG(R < (1L << 40) / C, "%s: R * C too large", who);
    KINET_CHECK_ARG(gamma >= 0.f, "%s: gamma must be >= 0", who);
    KINET_CHECK_ARG(inv_num_boxes > 0.f, "%s: 1 / num_boxes must be positive", who);
    KINET_CHECK_ARG(n == 0 || (pos_rows && pos_cls), "%s: null pointer (positives)", who);
    KINET_CHECK_ARG(R == 0 || (logits && aligned16(logits)), "%s: logits must be a 16-byte aligned pointer", who);
    return KINET_OK;
}

extern "C" int kinet_focal_set_loss(const float* logits, const int64_t* pos_rows, const int64_t* pos_cls, float* loss,
                                    int64_t R, int C, int n, float alpha, float gamma, float inv_num_boxes,
                                    float* workspace, kinet_stream_t stream) {
    if (int rc = focal_args("focal_set_loss", logits, pos_rows, pos_cls, R, C, n, gamma, inv_num_boxes)) return rc;
    KINET_CHECK_ARG(loss && workspace, "focal_set_loss: null pointer (loss / workspace)");
    const hipStream_t s = (hipStream_t)stream;
    const long total = (long)R * C;
    int nblk = 0;
    if (total > 0) {
        nblk = focal_blocks(total);
        const long nvec = total / 4;
        const long per = std::max<long>(FL_VEC_PER_BLOCK, (nvec + FL_MAX_BLOCKS - 1) / FL_MAX_BLOCKS);
        hipLaunchKernelGGL(focal_set_loss_kernel, dim3(nblk), dim3(256), 0, s, logits, pos_rows, pos_cls, n, workspace,
                           (long)R, C, per, alpha, gamma);
        KINET_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(focal_set_loss_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, nblk, loss,
                       inv_num_boxes);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_focal_set_loss_backward(const float* logits, const int64_t* pos_rows, const int64_t* pos_cls,
                                             const float* dloss, float* dlogits, int64_t R, int C, int n, float alpha,
                                             float gamma, float inv_num_boxes, kinet_stream_t stream) {
    if (int rc = focal_args("focal_set_loss_backward", logits, pos_rows, pos_cls, R, C, n, gamma, inv_num_boxes))
        return rc;
    const long total = (long)R * C;
    if (total == 0) return KINET_OK;
    KINET_CHECK_ARG(dloss && dlogits && aligned16(dlogits),
                    "focal_set_loss_backward: dloss and a 16-byte aligned dlogits required");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(focal_set_loss_backward_kernel, dim3(stride_grid(total / 4)), dim3(256), 0, s, logits, dloss,
                       dlogits, total, alpha, gamma, inv_num_boxes);
    KINET_LAUNCH_CHECK();
    if (n > 0) {
        hipLaunchKernelGGL(focal_set_loss_backward_pos_kernel, dim3(stride_grid(n)), dim3(256), 0, s, logits, pos_rows,
                           pos_cls, n, dloss, dlogits, (long)R, C, alpha, gamma, inv_num_boxes);
        KINET_LAUNCH_CHECK();
    }
    return KINET_OK;
}

extern "C" int kinet_two_stage_mask_rows(const float* x, const uint8_t* keep, float* y, int64_t rows, int d,
                                         kinet_stream_t stream) {
    KINET_CHECK_ARG(rows >= 0 && d > 0 && d % 4 == 0, "two_stage_mask_rows: rows %ld, d %d must be a positive multiple of 4",
                    (long)rows, d);
    if (rows == 0) return KINET_OK;
    KINET_CHECK_ARG(x && keep && y, "two_stage_mask_rows: null pointer");
    KINET_CHECK_ARG(aligned16(x) && aligned16(y), "two_stage_mask_rows: 16-byte aligned buffers required");
    const int cpr = d / 4;
    hipLaunchKernelGGL(mask_rows_kernel, dim3(stride_grid(rows * cpr)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)x, keep, (float4*)y, (long)rows, cpr);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_two_stage_boxes_backward(const float* d_boxes, const float* d_coord_unact, const float* boxes,
                                              float* d_tmp, int64_t rows, kinet_stream_t stream) {
    KINET_CHECK_ARG(rows >= 0, "two_stage_boxes_backward: rows %ld", (long)rows);
    KINET_CHECK_ARG(d_boxes || d_coord_unact, "two_stage_boxes_backward: both input gradients are NULL");
    if (rows == 0) return KINET_OK;
    KINET_CHECK_ARG(d_tmp && (boxes || !d_boxes), "two_stage_boxes_backward: null pointer");
    KINET_CHECK_ARG(aligned16(d_boxes) && aligned16(d_coord_unact) && aligned16(boxes) && aligned16(d_tmp),
                    "two_stage_boxes_backward: 16-byte aligned buffers required");
    hipLaunchKernelGGL(boxes_backward_kernel, dim3(stride_grid(rows)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)d_boxes, (const float4*)d_coord_unact, (const float4*)boxes, (float4*)d_tmp,
                       (long)rows);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}
