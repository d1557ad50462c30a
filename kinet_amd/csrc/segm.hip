// The segmentation head of DeformableDETRSegm (detr_segmentation.py): joint-softmax attention map,
// lay1 as a per-frame part plus an 8-channel per-query part, GroupNorm + ReLU (+ nearest upsample +
// FPN add), the 16 -> 1 output convolution and the PostProcessSegm resampling.
// C-ABI: include/kinet_segm.h.  No float atomics: every reduction runs in a fixed order.
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>

#include "../../include/kinet_segm.h"
#include "common.h"
#include "segm_resize.h"

namespace kinet {
namespace {

#define SEGM_DISPATCH(dtype, ...)                      \
    do {                                               \
        if ((dtype) == KINET_BF16) {                   \
            typedef bf16_t T;                          \
            __VA_ARGS__;                               \
        } else if ((dtype) == KINET_F16) {             \
            typedef f16_t T;                           \
            __VA_ARGS__;                               \
        } else {                                       \
            typedef float T;                           \
            __VA_ARGS__;                               \
        }                                              \
    } while (0)

inline bool segm_dtype_ok(int dt) { return dt == KINET_F32 || dt == KINET_BF16 || dt == KINET_F16; }

inline int segm_grid(long total) {
    const long blocks = (total + 255) / 256;
    return (int)(blocks < 1 ? 1 : (blocks > 8L * kMaxGridStride ? 8L * kMaxGridStride : blocks));
}

// The frame whose per-frame operand row r of a call reads: frame-major rows (row_frame == nullptr:
// global row / Q) or a ragged list with one entry per row of the call.  A workgroup-uniform read;
// the kernels leave a row alone when the entry is outside [0, B).
__device__ __forceinline__ int segm_row_frame(const int32_t* __restrict__ row_frame, int r, int global_row, int Q) {
    return row_frame ? row_frame[r] : global_row / Q;
}

// ---------------------------------------------------------------------------------
// attention map: one workgroup per (frame, query) row, items (pixel, head) strided over the
// threads so that a thread keeps its head (256 % heads == 0) and a wave reads whole key rows
// ---------------------------------------------------------------------------------
struct MaxSum {
    float m, s;   // running max and sum of exp(l - m)
};

__device__ __forceinline__ MaxSum ms_merge(MaxSum a, MaxSum b) {
    const float ninf = -__builtin_inff();
    MaxSum r;
    r.m = fmaxf(a.m, b.m);
    const float ea = a.m == ninf ? 0.f : expf(a.m - r.m);
    const float eb = b.m == ninf ? 0.f : expf(b.m - r.m);
    r.s = a.s * ea + b.s * eb;
    return r;
}

template <typename T>
__device__ __forceinline__ float att_logit(const T* __restrict__ krow, const float* __restrict__ q, int D) {
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < D; ++k) acc += q[k] * to_f32(krow[k]);
    return acc;
}

template <typename T>
__global__ __launch_bounds__(256) void segm_attention_kernel(const T* __restrict__ qp, const T* __restrict__ kp,
                                                             const uint8_t* __restrict__ mask,
                                                             const int32_t* __restrict__ row_frame,
                                                             T* __restrict__ out, int B, int Q, int HW, int heads,
                                                             int d, float scale) {
    extern __shared__ float q_s[];   // [d], pre-scaled (the reference scales q, :210)
    __shared__ MaxSum wave_ms[4];
    const int r = blockIdx.x;
    const int b = segm_row_frame(row_frame, r, r, Q);
    if (b < 0 || b >= B) return;   // (a ragged row whose entry names no frame: the whole workgroup leaves)
    const int D = d / heads;
    for (int k = threadIdx.x; k < d; k += 256) q_s[k] = to_f32(qp[(long)r * d + k]) * scale;
    __syncthreads();
    const int n = threadIdx.x % heads, pstep = 256 / heads;
    const float* qn = q_s + n * D;
    const T* kb = kp + (long)b * HW * d + n * D;
    const uint8_t* mb = mask ? mask + (long)b * HW : nullptr;
    const float ninf = -__builtin_inff();
    MaxSum t = {ninf, 0.f};
    for (int p = threadIdx.x / heads; p < HW; p += pstep) {
        if (mb && mb[p]) continue;
        const float l = att_logit(kb + (long)p * d, qn, D);
        const float m = fmaxf(t.m, l);
        t.s = t.s * (t.m == ninf ? 0.f : expf(t.m - m)) + expf(l - m);
        t.m = m;
    }
    // butterfly over the wave (the merge is symmetric, so every lane holds the same pair), then
    // the four waves in order
    for (int o = 32; o >= 1; o >>= 1) {
        MaxSum u = {__shfl_xor(t.m, o), __shfl_xor(t.s, o)};
        t = ms_merge(t, u);
    }
    if (threadIdx.x % 64 == 0) wave_ms[threadIdx.x / 64] = t;
    __syncthreads();
    MaxSum g = wave_ms[0];
    for (int i = 1; i < 4; ++i) g = ms_merge(g, wave_ms[i]);
    const float inv = 1.f / g.s;   // every pixel masked: 1/0 * 0 below = NaN, as torch's softmax of -inf
    T* orow = out + (long)r * HW * heads;
    for (int p = threadIdx.x / heads; p < HW; p += pstep) {
        float v;
        if (mb && mb[p]) {
            v = g.s == 0.f ? __builtin_nanf("") : 0.f;
        } else {
            v = expf(att_logit(kb + (long)p * d, qn, D) - g.m) * inv;
        }
        orow[(long)p * heads + n] = Cvt<T>::from(v);
    }
}

// ---------------------------------------------------------------------------------
// lay1, the per-query part: a workgroup owns a LAY1_TR x LAY1_TW pixel tile of one row, thread c
// owns output channel c with its 72 weights in registers; the attention tile (with halo) sits in
// LDS as f32 and is read as broadcasts.  At most 512 threads, so that the weights and an unrolled
// pixel's attention values fit the register file (at 1024 the compiler spills 93 registers).
// ---------------------------------------------------------------------------------
constexpr int LAY1_TR = 4, LAY1_TW = 32, LAY1_CA = 8;

template <typename T>
__global__ __launch_bounds__(512) void segm_lay1_kernel(const T* __restrict__ att, const float* __restrict__ w_att,
                                                         const float* __restrict__ frame,
                                                         const int32_t* __restrict__ row_frame, T* __restrict__ y,
                                                         int row0, int Q, int B, int H, int W, int Cout) {
    __shared__ float4 tile[LAY1_TR + 2][LAY1_TW + 2][LAY1_CA / 4];
    const int r = blockIdx.z;
    const int b = segm_row_frame(row_frame, r, row0 + r, Q);
    if (b < 0 || b >= B) return;
    const int y0 = blockIdx.y * LAY1_TR, x0 = blockIdx.x * LAY1_TW;
    float* tf = reinterpret_cast<float*>(tile);
    constexpr int TILE_N = (LAY1_TR + 2) * (LAY1_TW + 2) * LAY1_CA;
    for (int i = threadIdx.x; i < TILE_N; i += blockDim.x) {
        const int ci = i % LAY1_CA, tx = (i / LAY1_CA) % (LAY1_TW + 2), ty = i / (LAY1_CA * (LAY1_TW + 2));
        const int yy = y0 + ty - 1, xx = x0 + tx - 1;
        float v = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = to_f32(att[(((long)r * H + yy) * W + xx) * LAY1_CA + ci]);
        tf[i] = v;
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= Cout) return;
    float wreg[9 * LAY1_CA];
#pragma unroll
    for (int k = 0; k < 9 * LAY1_CA; ++k) wreg[k] = w_att[(long)k * Cout + c];
    const int ny = min(LAY1_TR, H - y0), nx = min(LAY1_TW, W - x0);
    for (int ty = 0; ty < ny; ++ty) {
        for (int tx = 0; tx < nx; ++tx) {
            const long pix = (long)(y0 + ty) * W + (x0 + tx);
            float acc = frame[((long)b * H * W + pix) * Cout + c];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int v4 = 0; v4 < LAY1_CA / 4; ++v4) {
                        const float4 a = tile[ty + ky][tx + kx][v4];
                        const float* wk = wreg + (ky * 3 + kx) * LAY1_CA + v4 * 4;
                        acc = fmaf(wk[0], a.x, acc);
                        acc = fmaf(wk[1], a.y, acc);
                        acc = fmaf(wk[2], a.z, acc);
                        acc = fmaf(wk[3], a.w, acc);
                    }
            y[((long)r * H * W + pix) * Cout + c] = Cvt<T>::from(acc);
        }
    }
}

// ---------------------------------------------------------------------------------
// GroupNorm + ReLU (+ nearest upsample + add).  Workspace (floats): stats [rows][2*groups],
// pivots [rows][groups], partials [rows][nblk][2*groups].
// ---------------------------------------------------------------------------------
constexpr int SEGM_GN_PPB = 256;   // pixels per statistics block
constexpr int SEGM_GN_V = 8;       // channels a thread owns (one 16-byte vector of a 16-bit type)

template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ p, float (&v)[SEGM_GN_V]) {
    if constexpr (sizeof(T) == 2) {
        const VecT<T, 8> t = *reinterpret_cast<const VecT<T, 8>*>(p);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = to_f32(t.v[k]);
    } else {
        const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    }
}

template <typename T>
__device__ __forceinline__ void store8(T* __restrict__ p, const float (&v)[SEGM_GN_V]) {
    if constexpr (sizeof(T) == 2) {
        VecT<T, 8> t;
#pragma unroll
        for (int k = 0; k < 8; ++k) t.v[k] = Cvt<T>::from(v[k]);
        *reinterpret_cast<VecT<T, 8>*>(p) = t;
    } else {
        reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
}

// A thread owns 8 consecutive channels (C % 8 == 0) and PP = 256 / (C / 8) pixels run side by side.
// The per-(pixel lane, channel) sums are parked in LDS and each group is summed over (lane, channel)
// in that order; the group pivots are formed once per block.
template <typename T>
__global__ __launch_bounds__(256) void segm_gn_stats_kernel(const T* __restrict__ x, float* __restrict__ part,
                                                            float* __restrict__ piv, int HW, int C, int groups) {
    extern __shared__ float red[];   // [2][PP][C], then [groups] pivots
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * SEGM_GN_PPB, p1 = min(HW, p0 + SEGM_GN_PPB);
    const int cpg = C / groups, CV = C / SEGM_GN_V;
    const int PP = 256 / CV;
    float* piv_s = red + 2 * PP * C;
    for (int g = threadIdx.x; g < groups; g += 256) {
        const float pv = gn_pivot(x, n, HW, C, cpg, g * cpg);
        piv_s[g] = pv;
        if (blockIdx.x == 0) piv[(long)n * groups + g] = pv;
    }
    __syncthreads();
    const int lane = threadIdx.x / CV, c0 = (threadIdx.x % CV) * SEGM_GN_V;
    if (lane < PP) {
        float pv[SEGM_GN_V], s[SEGM_GN_V], q[SEGM_GN_V];
#pragma unroll
        for (int k = 0; k < SEGM_GN_V; ++k) pv[k] = piv_s[(c0 + k) / cpg], s[k] = 0.f, q[k] = 0.f;
        for (int p = p0 + lane; p < p1; p += PP) {
            float v[SEGM_GN_V];
            load8(x + ((long)n * HW + p) * C + c0, v);
#pragma unroll
            for (int k = 0; k < SEGM_GN_V; ++k) {
                const float t = v[k] - pv[k];
                s[k] += t;
                q[k] += t * t;
            }
        }
#pragma unroll
        for (int k = 0; k < SEGM_GN_V; ++k) {
            red[lane * C + c0 + k] = s[k];
            red[(PP + lane) * C + c0 + k] = q[k];
        }
    }
    __syncthreads();
    float* o = part + ((long)n * gridDim.x + blockIdx.x) * 2 * groups;
    for (int g = threadIdx.x; g < groups; g += 256) {
        float s = 0.f, q = 0.f;
        for (int l = 0; l < PP; ++l)
            for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
                s += red[l * C + c];
                q += red[(PP + l) * C + c];
            }
        o[2 * g] = s;
        o[2 * g + 1] = q;
    }
}

// stats[n][i] = the nblk block partials of row n summed in a fixed order: 256 / w threads share one
// of the w = 2*groups outputs (strided over the blocks), then their sums are added in thread order
__global__ __launch_bounds__(256) void segm_gn_finalize_kernel(const float* __restrict__ part,
                                                               float* __restrict__ stats, int nblk, int groups) {
    __shared__ float red[256];
    const int n = blockIdx.x;
    const int w = 2 * groups;   // <= 256
    const int tpo = 256 / w;
    const int i = threadIdx.x % w, k = threadIdx.x / w;
    float a = 0.f;
    if (k < tpo) {
        const float* pp = part + (long)n * nblk * w + i;
        for (int b = k; b < nblk; b += tpo) a += pp[(long)b * w];
    }
    red[threadIdx.x] = a;
    __syncthreads();
    if (k == 0) {
        float t = 0.f;
        for (int j = 0; j < tpo; ++j) t += red[j * w + i];
        stats[(long)n * w + i] = t;
    }
}

// grid (pixel-vector chunks, rows): a thread owns 8 consecutive channels of one output pixel; the
// row's group means and inverse deviations are formed once per block in LDS
template <typename T>
__global__ __launch_bounds__(256) void segm_gn_apply_kernel(const T* __restrict__ x, const float* __restrict__ stats,
                                                            const float* __restrict__ piv,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const T* __restrict__ f,
                                                            const int32_t* __restrict__ row_frame, T* __restrict__ y,
                                                            int row0, int Q, int B, int h, int w, int H, int W, int C,
                                                            int groups, float eps, float sh, float sw) {
    extern __shared__ float mr[];   // [groups] mean, [groups] rstd
    const int n = blockIdx.y;
    const int fb = segm_row_frame(row_frame, n, row0 + n, Q);
    if (row_frame && (fb < 0 || fb >= B)) return;
    const int cpg = C / groups, CV = C / SEGM_GN_V;
    const float cnt = (float)h * (float)w * (float)cpg;
    for (int g = threadIdx.x; g < groups; g += 256) {
        const float* st = stats + ((long)n * groups + g) * 2;
        const float ms = st[0] / cnt;   // of x - pivot
        const float var = fmaxf(st[1] / cnt - ms * ms, 0.f);
        mr[g] = piv[(long)n * groups + g] + ms;
        mr[groups + g] = rsqrtf(var + eps);
    }
    __syncthreads();
    const int total = H * W * CV;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int cv = i % CV, pix = i / CV;
        const int X = pix % W, Y = pix / W;
        const int c0 = cv * SEGM_GN_V;
        // torch's legacy nearest rule (nearest_neighbor_compute_source_index) in f32
        const int sy = min((int)floorf((float)Y * sh), h - 1);
        const int sx = min((int)floorf((float)X * sw), w - 1);
        float v[SEGM_GN_V], o[SEGM_GN_V];
        load8(x + (((long)n * h + sy) * w + sx) * C + c0, v);
        int g = c0 / cpg, next = (g + 1) * cpg;
#pragma unroll
        for (int k = 0; k < SEGM_GN_V; ++k) {
            const int c = c0 + k;
            if (c == next) {
                ++g;
                next += cpg;
            }
            o[k] = fmaxf((v[k] - mr[g]) * mr[groups + g] * gamma[c] + beta[c], 0.f);
        }
        if (f) {
            float fv[SEGM_GN_V];
            load8(f + (((long)fb * H + Y) * W + X) * C + c0, fv);
#pragma unroll
            for (int k = 0; k < SEGM_GN_V; ++k) o[k] += fv[k];
        }
        store8(y + (((long)n * H + Y) * W + X) * C + c0, o);
    }
}

// ---------------------------------------------------------------------------------
// out_lay: one thread per output pixel
// ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void segm_out_conv_kernel(const T* __restrict__ x, const float* __restrict__ wt,
                                                            const float* __restrict__ bias, float* __restrict__ y,
                                                            long total, int H, int W, int C) {
    __shared__ float w_s[9 * 64];
    for (int k = threadIdx.x; k < 9 * C; k += 256) w_s[k] = wt[k];
    __syncthreads();
    const float b0 = bias[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int X = (int)(i % W);
        const long t = i / W;
        const int Y = (int)(t % H);
        const long n = t / H;
        float acc = b0;
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = Y + ky - 1;
            if (yy < 0 || yy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = X + kx - 1;
                if (xx < 0 || xx >= W) continue;
                const T* px = x + ((n * H + yy) * W + xx) * C;
                const float* wk = w_s + (ky * 3 + kx) * C;
                for (int c = 0; c < C; ++c) acc = fmaf(wk[c], to_f32(px[c]), acc);
            }
        }
        y[i] = acc;
    }
}

// ---------------------------------------------------------------------------------
// PostProcessSegm: one thread per output pixel
// ---------------------------------------------------------------------------------
// One output pixel's four taps and weights: the legacy-nearest map of (oy, ox) into the cropped
// (img_h, img_w) probability map, then the bilinear source position in the (h, w) logits.
struct SegmTap {
    long o00, o01, o10, o11;   // offsets inside one (h, w) row of logits
    float ly, lx;
};

__device__ __forceinline__ SegmTap segm_tap(int oy, int ox, int h, int w, int img_h, int img_w, float bh, float bw,
                                            float nh, float nw) {
    // nearest source pixel inside the cropped (img_h, img_w) probability map
    const int my = min((int)floorf((float)oy * nh), img_h - 1);
    const int mx = min((int)floorf((float)ox * nw), img_w - 1);
    int y0, y1, x0, x1;
    SegmTap t;
    bilinear_src(my, bh, h, y0, y1, t.ly);
    bilinear_src(mx, bw, w, x0, x1, t.lx);
    t.o00 = (long)y0 * w + x0, t.o01 = (long)y0 * w + x1;
    t.o10 = (long)y1 * w + x0, t.o11 = (long)y1 * w + x1;
    return t;
}

// sigmoid of the bilinear sample of one row of logits: the per-pixel probability of PostProcessSegm,
// shared by segm_postprocess_kernel and segm_track_resolve_kernel so that both round alike
__device__ __forceinline__ float segm_prob(const float* __restrict__ p, const SegmTap& t) {
    const float top = (1.f - t.lx) * p[t.o00] + t.lx * p[t.o01];
    const float bot = (1.f - t.lx) * p[t.o10] + t.lx * p[t.o11];
    const float v = (1.f - t.ly) * top + t.ly * bot;
    return 1.f / (1.f + expf(-v));
}

// The tracker's pixel rule, shared by the two resolve kernels below so that they agree bit for bit: slot
// t of src[0 .. T) is fresh (src[t] >= 0: the probability of row src[t] of the n rows of logits) or stale
// (src[t] < 0: 1.0 where the previous label `was` is slot -src[t]-1, else 0.0); the label is torch's
// argmax over the slots (first occurrence of the maximum, NaN the greatest) where that maximum exceeds
// the threshold, else -1.  src is read with wave-uniform addresses.
__device__ __forceinline__ int segm_resolve_label(const float* __restrict__ logits, const SegmTap& tap, int was,
                                                  const int32_t* __restrict__ src, int T, int n, long hw,
                                                  float threshold) {
    int best = -1;
    float pbest = 0.f;
    for (int t = 0; t < T; ++t) {
        const int s = src[t];
        float p;
        if (s >= 0) p = s < n ? segm_prob(logits + (long)s * hw, tap) : 0.f;   // (a row outside logits is never read)
        else p = was == -s - 1 ? 1.f : 0.f;
        // argmax: a NaN is taken once and then kept; otherwise strictly greater replaces
        if (best < 0 || (pbest == pbest && (p > pbest || p != p))) {
            best = t;
            pbest = p;
        }
    }
    return pbest > threshold ? best : -1;
}

template <bool PROBS>
__global__ __launch_bounds__(256) void segm_postprocess_kernel(const float* __restrict__ logits, void* __restrict__ out,
                                                               long total, int h, int w, int img_h, int img_w, int oh,
                                                               int ow, float bh, float bw, float nh, float nw,
                                                               float threshold) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % ow);
        const long t = i / ow;
        const int oy = (int)(t % oh);
        const long q = t / oh;
        const SegmTap tap = segm_tap(oy, ox, h, w, img_h, img_w, bh, bw, nh, nw);
        const float prob = segm_prob(logits + q * h * w, tap);
        if (PROBS) ((float*)out)[i] = prob;
        else ((uint8_t*)out)[i] = prob > threshold ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------
// Tracker masks: one thread per output pixel resolves the T track slots into one label
// (segm_resolve_label).  The taps are formed once per pixel.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void segm_track_resolve_kernel(const float* __restrict__ logits,
                                                                 const int32_t* __restrict__ src,
                                                                 const int16_t* __restrict__ prev,
                                                                 int16_t* __restrict__ labels, int T, int n, long total,
                                                                 int h, int w, int img_h, int img_w, int ow, float bh,
                                                                 float bw, float nh, float nw, float threshold) {
    const long hw = (long)h * w;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % ow);
        const int oy = (int)(i / ow);
        const SegmTap tap = segm_tap(oy, ox, h, w, img_h, img_w, bh, bw, nh, nw);
        const int was = prev ? (int)prev[i] : -1;
        labels[i] = (int16_t)segm_resolve_label(logits, tap, was, src, T, n, hw, threshold);
    }
}

// ---------------------------------------------------------------------------------
// Tracker masks of S sequences in one launch: the pixel rule above per segment, plus per slot the
// pixel count and bounding box of its label.  A workgroup owns RESOLVE_PPB consecutive pixels of ONE
// segment's map (the segments' tables ride in the kernel arguments, so the host has checked them);
// the statistics are integers -- count by add, the box as four maxima (x0 and y0 as INT_MAX - x, so
// that an all-zero table is the neutral element) -- gathered in an LDS table of RESOLVE_LDS_SLOTS
// slots with LDS atomics and merged into global memory with one atomic per non-empty (slot, field)
// of the workgroup; slots beyond the table go to global memory directly.  Integer add and max
// commute: reruns are bit-identical.  segm_resolve_stats_finish turns the two coded minima back.
// ---------------------------------------------------------------------------------
constexpr int RESOLVE_SEGS = 32;          // segments per launch (their tables are kernel arguments)
constexpr int RESOLVE_LDS_SLOTS = 256;    // slots of a segment whose statistics gather in LDS
constexpr int RESOLVE_PPB = 1024;         // pixels per workgroup (4 per thread)
constexpr int RESOLVE_CODE = 0x7fffffff;

struct ResolveSeg {
    long pix_off, prev_off;   // elements into labels / prev (prev_off < 0: no previous map)
    int src_off, T;           // the segment's slots are src[src_off .. src_off + T)
    int img_h, img_w, oh, ow;
    int blk0;                 // its first workgroup
    float nh, nw;             // nearest scales img / out, as kinet_segm_track_resolve forms them
};
struct ResolveSegs {
    ResolveSeg s[RESOLVE_SEGS];
};

__global__ __launch_bounds__(256) void segm_track_resolve_segments_kernel(
    const float* __restrict__ logits, const int32_t* __restrict__ src, const int16_t* __restrict__ prev,
    int16_t* __restrict__ labels, int32_t* __restrict__ stats, const ResolveSegs segs, int nseg, int n, int h, int w,
    float bh, float bw, float threshold) {
    __shared__ int tab[5][RESOLVE_LDS_SLOTS];
    // the segment of this workgroup: the last one that starts at or before it (a segment without
    // pixels owns no workgroup and shares its successor's start).  Constant indices: the tables stay
    // in the argument segment.
    ResolveSeg g = segs.s[0];
#pragma unroll
    for (int k = 1; k < RESOLVE_SEGS; ++k)
        if (k < nseg && segs.s[k].blk0 <= (int)blockIdx.x) g = segs.s[k];
    for (int k = threadIdx.x; k < 5 * RESOLVE_LDS_SLOTS; k += 256) (&tab[0][0])[k] = 0;
    __syncthreads();
    const long hw = (long)h * w;
    const long total = (long)g.oh * g.ow;
    const long base = (long)((int)blockIdx.x - g.blk0) * RESOLVE_PPB;
    const int32_t* sseg = src + g.src_off;
    int32_t* gst = stats + (long)g.src_off * 5;
    for (int k = 0; k < RESOLVE_PPB / 256; ++k) {
        const long i = base + k * 256 + threadIdx.x;
        if (i >= total) break;
        const int ox = (int)(i % g.ow);
        const int oy = (int)(i / g.ow);
        const SegmTap tap = segm_tap(oy, ox, h, w, g.img_h, g.img_w, bh, bw, g.nh, g.nw);
        const int was = g.prev_off >= 0 ? (int)prev[g.prev_off + i] : -1;
        const int lab = segm_resolve_label(logits, tap, was, sseg, g.T, n, hw, threshold);
        labels[g.pix_off + i] = (int16_t)lab;
        if (lab >= 0) {
            if (lab < RESOLVE_LDS_SLOTS) {
                atomicAdd(&tab[0][lab], 1);
                atomicMax(&tab[1][lab], RESOLVE_CODE - ox);
                atomicMax(&tab[2][lab], RESOLVE_CODE - oy);
                atomicMax(&tab[3][lab], ox + 1);
                atomicMax(&tab[4][lab], oy + 1);
            } else {
                int32_t* st = gst + (long)lab * 5;
                atomicAdd(st, 1);
                atomicMax(st + 1, RESOLVE_CODE - ox);
                atomicMax(st + 2, RESOLVE_CODE - oy);
                atomicMax(st + 3, ox + 1);
                atomicMax(st + 4, oy + 1);
            }
        }
    }
    __syncthreads();
    const int nt = min(g.T, RESOLVE_LDS_SLOTS);
    for (int t = threadIdx.x; t < nt; t += 256) {
        const int c = tab[0][t];
        if (c == 0) continue;
        int32_t* st = gst + (long)t * 5;
        atomicAdd(st, c);
#pragma unroll
        for (int k = 1; k < 5; ++k) atomicMax(st + k, tab[k][t]);
    }
}

// (count, INT_MAX - x0, INT_MAX - y0, x1, y1) -> (count, x0, y0, x1, y1); a slot without a pixel is all zero already
__global__ __launch_bounds__(256) void segm_resolve_stats_finish(int32_t* __restrict__ stats, int total) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total || stats[(long)t * 5] == 0) return;
    stats[(long)t * 5 + 1] = RESOLVE_CODE - stats[(long)t * 5 + 1];
    stats[(long)t * 5 + 2] = RESOLVE_CODE - stats[(long)t * 5 + 2];
}

}  // namespace
}  // namespace kinet

using namespace kinet;

// The launchers below serve the frame-major entry point (row_frame == nullptr: `rows` rows from
// row0 on, Q per frame) and its ragged twin (row_frame: one device int per row, row0 = 0, Q = 1).
static int segm_attention_launch(const void* qp, const void* kp, const uint8_t* mask, const int32_t* row_frame,
                                 void* out, long rows, int B, int Q, int HW, int heads, int d, float scale, int dtype,
                                 kinet_stream_t stream) {
    KINET_CHECK_ARG(segm_dtype_ok(dtype), "segm_attention: dtype must be f32, bf16 or f16");
    KINET_CHECK_ARG(B >= 0 && Q >= 0 && rows >= 0 && HW > 0, "segm_attention: bad geometry");
    KINET_CHECK_ARG(heads > 0 && heads <= 32 && (heads & (heads - 1)) == 0, "segm_attention: heads must be a power of two <= 32");
    KINET_CHECK_ARG(d > 0 && d <= 1024 && d % heads == 0, "segm_attention: d must be a multiple of heads, <= 1024");
    KINET_CHECK_ARG(rows <= 0x7fffffffL, "segm_attention: too many rows");
    if (rows == 0) return KINET_OK;
    KINET_CHECK_ARG(qp && kp && out, "segm_attention: null pointer");
    SEGM_DISPATCH(dtype, hipLaunchKernelGGL((segm_attention_kernel<T>), dim3((unsigned)rows), dim3(256),
                                            d * sizeof(float), (hipStream_t)stream, (const T*)qp, (const T*)kp, mask,
                                            row_frame, (T*)out, B, Q, HW, heads, d, scale));
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_segm_attention(const void* qp, const void* kp, const uint8_t* mask, void* out, int B, int Q,
                                    int HW, int heads, int d, float scale, int dtype, kinet_stream_t stream) {
    return segm_attention_launch(qp, kp, mask, nullptr, out, (long)(B > 0 ? B : 0) * (Q > 0 ? Q : 0), B, Q, HW, heads,
                                 d, scale, dtype, stream);
}

extern "C" int kinet_segm_attention_rows(const void* qp, const void* kp, const uint8_t* mask, const int32_t* row_frame,
                                         void* out, int rows, int B, int HW, int heads, int d, float scale, int dtype,
                                         kinet_stream_t stream) {
    KINET_CHECK_ARG(rows >= 0 && B >= 0, "segm_attention_rows: bad geometry");
    KINET_CHECK_ARG(rows == 0 || B > 0, "segm_attention_rows: rows without a frame");
    KINET_CHECK_ARG(rows == 0 || row_frame != nullptr, "segm_attention_rows: null pointer (row_frame)");
    return segm_attention_launch(qp, kp, mask, row_frame, out, rows, B, 1, HW, heads, d, scale, dtype, stream);
}

static int segm_lay1_launch(const void* att, const float* w_att, const float* frame, const int32_t* row_frame, void* y,
                            int rows, int row0, int Q, int B, int H, int W, int Ca, int Cout, int dtype,
                            kinet_stream_t stream) {
    KINET_CHECK_ARG(segm_dtype_ok(dtype), "segm_lay1: dtype must be f32, bf16 or f16");
    KINET_CHECK_ARG(Ca == LAY1_CA, "segm_lay1: 8 attention channels only");
    KINET_CHECK_ARG(Cout > 0 && Cout <= 512, "segm_lay1: Cout must be in 1..512");
    KINET_CHECK_ARG(rows >= 0 && row0 >= 0 && Q > 0 && B > 0 && H > 0 && W > 0, "segm_lay1: bad geometry");
    KINET_CHECK_ARG(row_frame != nullptr || (long)row0 + rows <= (long)B * Q,
                    "segm_lay1: rows [row0, row0 + rows) outside the B*Q rows");
    KINET_CHECK_ARG(rows <= 65535 && (H + LAY1_TR - 1) / LAY1_TR <= 65535, "segm_lay1: at most 65535 rows per call");
    if (rows == 0) return KINET_OK;
    KINET_CHECK_ARG(att && w_att && frame && y, "segm_lay1: null pointer");
    const dim3 grid((W + LAY1_TW - 1) / LAY1_TW, (H + LAY1_TR - 1) / LAY1_TR, rows);
    const int threads = (Cout + 63) / 64 * 64;
    SEGM_DISPATCH(dtype, hipLaunchKernelGGL((segm_lay1_kernel<T>), grid, dim3(threads), 0, (hipStream_t)stream,
                                            (const T*)att, w_att, frame, row_frame, (T*)y, row0, Q, B, H, W, Cout));
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_segm_lay1(const void* att, const float* w_att, const float* frame, void* y, int rows, int row0,
                               int Q, int B, int H, int W, int Ca, int Cout, int dtype, kinet_stream_t stream) {
    return segm_lay1_launch(att, w_att, frame, nullptr, y, rows, row0, Q, B, H, W, Ca, Cout, dtype, stream);
}

extern "C" int kinet_segm_lay1_rows(const void* att, const float* w_att, const float* frame, const int32_t* row_frame,
                                    void* y, int rows, int B, int H, int W, int Ca, int Cout, int dtype,
                                    kinet_stream_t stream) {
    KINET_CHECK_ARG(rows <= 0 || row_frame != nullptr, "segm_lay1_rows: null pointer (row_frame)");
    return segm_lay1_launch(att, w_att, frame, row_frame, y, rows, 0, 1, B, H, W, Ca, Cout, dtype, stream);
}

extern "C" long kinet_segm_gn_workspace(int rows, int hw, int groups) {
    if (rows <= 0 || hw <= 0 || groups <= 0) return 0;
    const long nblk = (hw + SEGM_GN_PPB - 1) / SEGM_GN_PPB;
    return (long)rows * groups * (3 + 2 * nblk);
}

static int segm_gn_launch(const void* x, const float* gamma, const float* beta, const void* f,
                          const int32_t* row_frame, void* y, int rows, int row0, int Q, int B, int h, int w, int H, int W,
                          int C, int groups, float eps, int dtype, float* ws, kinet_stream_t stream) {
    KINET_CHECK_ARG(segm_dtype_ok(dtype), "segm_gn: dtype must be f32, bf16 or f16");
    KINET_CHECK_ARG(rows >= 0 && row0 >= 0 && Q > 0 && B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "segm_gn: bad geometry");
    KINET_CHECK_ARG(C > 0 && C <= 2048 && groups > 0 && groups <= 128 && C % groups == 0 && C % SEGM_GN_V == 0,
                    "segm_gn: C must be a multiple of groups and of 8 (C <= 2048, groups <= 128)");
    KINET_CHECK_ARG(row_frame != nullptr || (long)row0 + rows <= (long)B * Q,
                    "segm_gn: rows [row0, row0 + rows) outside the B*Q rows");
    KINET_CHECK_ARG(f != nullptr || (H == h && W == w), "segm_gn: without an FPN operand the output has the input's size");
    KINET_CHECK_ARG(rows <= 65535, "segm_gn: at most 65535 rows per call");
    KINET_CHECK_ARG((long)h * w <= 0x3fffffffL && (long)H * W * (C / SEGM_GN_V) <= 0x3fffffffL, "segm_gn: map too large");
    if (rows == 0) return KINET_OK;
    KINET_CHECK_ARG(x && gamma && beta && y, "segm_gn: null pointer");
    KINET_CHECK_ARG(ws != nullptr, "segm_gn: workspace of kinet_segm_gn_workspace() floats required");
    KINET_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)f) & 15) == 0, "segm_gn: x, y and f must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int HW = h * w;
    const int nblk = (HW + SEGM_GN_PPB - 1) / SEGM_GN_PPB;
    float* stats = ws;
    float* piv = stats + 2L * rows * groups;
    float* part = piv + (long)rows * groups;
    const int PP = 256 / (C / SEGM_GN_V);
    const size_t lds = (2 * (size_t)PP * C + groups) * sizeof(float);
    const long per_row = (long)H * W * (C / SEGM_GN_V);
    const int gx = (int)std::min<long>((per_row + 255) / 256, 4096);
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    SEGM_DISPATCH(dtype, {
        hipLaunchKernelGGL((segm_gn_stats_kernel<T>), dim3(nblk, rows), dim3(256), lds, s, (const T*)x, part, piv, HW,
                           C, groups);
        hipLaunchKernelGGL(segm_gn_finalize_kernel, dim3(rows), dim3(256), 0, s, (const float*)part, stats, nblk,
                           groups);
        hipLaunchKernelGGL((segm_gn_apply_kernel<T>), dim3(gx, rows), dim3(256), 2 * groups * sizeof(float), s,
                           (const T*)x, (const float*)stats, (const float*)piv, gamma, beta, (const T*)f, row_frame,
                           (T*)y, row0, Q, B, h, w, H, W, C, groups, eps, sh, sw);
    });
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_segm_gn_relu_up_add(const void* x, const float* gamma, const float* beta, const void* f, void* y,
                                         int rows, int row0, int Q, int B, int h, int w, int H, int W, int C,
                                         int groups, float eps, int dtype, float* ws, kinet_stream_t stream) {
    return segm_gn_launch(x, gamma, beta, f, nullptr, y, rows, row0, Q, B, h, w, H, W, C, groups, eps, dtype, ws,
                          stream);
}

extern "C" int kinet_segm_gn_relu_up_add_rows(const void* x, const float* gamma, const float* beta, const void* f,
                                              const int32_t* row_frame, void* y, int rows, int B, int h, int w, int H,
                                              int W, int C, int groups, float eps, int dtype, float* ws,
                                              kinet_stream_t stream) {
    KINET_CHECK_ARG(rows <= 0 || f == nullptr || row_frame != nullptr,
                    "segm_gn_rows: null pointer (row_frame: an FPN operand needs the rows' frames)");
    // (without an FPN operand nothing is read per frame: the list is not looked at)
    return segm_gn_launch(x, gamma, beta, f, f ? row_frame : nullptr, y, rows, 0, f ? 1 : (rows > 0 ? rows : 1),
                          f ? B : 1, h, w, H, W, C, groups, eps, dtype, ws, stream);
}

extern "C" int kinet_segm_out_conv(const void* x, const float* wt, const float* bias, float* y, int rows, int H, int W,
                                   int C, int dtype, kinet_stream_t stream) {
    KINET_CHECK_ARG(segm_dtype_ok(dtype), "segm_out_conv: dtype must be f32, bf16 or f16");
    KINET_CHECK_ARG(rows >= 0 && H > 0 && W > 0, "segm_out_conv: bad geometry");
    KINET_CHECK_ARG(C > 0 && C <= 64, "segm_out_conv: C must be in 1..64");
    if (rows == 0) return KINET_OK;
    KINET_CHECK_ARG(x && wt && bias && y, "segm_out_conv: null pointer");
    const long total = (long)rows * H * W;
    SEGM_DISPATCH(dtype, hipLaunchKernelGGL((segm_out_conv_kernel<T>), dim3(segm_grid(total)), dim3(256), 0,
                                            (hipStream_t)stream, (const T*)x, wt, bias, y, total, H, W, C));
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_segm_postprocess(const float* logits, void* out, int Q, int h, int w, int max_h, int max_w,
                                      int img_h, int img_w, int oh, int ow, float threshold, int return_probs,
                                      kinet_stream_t stream) {
    KINET_CHECK_ARG(Q >= 0 && h > 0 && w > 0 && max_h > 0 && max_w > 0 && oh > 0 && ow > 0, "segm_postprocess: bad geometry");
    KINET_CHECK_ARG(img_h > 0 && img_h <= max_h && img_w > 0 && img_w <= max_w,
                    "segm_postprocess: the frame's size must lie inside (max_h, max_w)");
    if (Q == 0) return KINET_OK;
    KINET_CHECK_ARG(logits && out, "segm_postprocess: null pointer");
    const long total = (long)Q * oh * ow;
    // torch's scales: input / output in f32 for both rules
    const float bh = (float)h / (float)max_h, bw = (float)w / (float)max_w;
    const float nh = (float)img_h / (float)oh, nw = (float)img_w / (float)ow;
    if (return_probs)
        hipLaunchKernelGGL((segm_postprocess_kernel<true>), dim3(segm_grid(total)), dim3(256), 0, (hipStream_t)stream,
                           logits, out, total, h, w, img_h, img_w, oh, ow, bh, bw, nh, nw, threshold);
    else
        hipLaunchKernelGGL((segm_postprocess_kernel<false>), dim3(segm_grid(total)), dim3(256), 0, (hipStream_t)stream,
                           logits, out, total, h, w, img_h, img_w, oh, ow, bh, bw, nh, nw, threshold);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_segm_track_resolve(const float* logits, const int32_t* src, const int16_t* prev_labels,
                                        int16_t* labels, int T, int n, int h, int w, int max_h, int max_w, int img_h,
                                        int img_w, int oh, int ow, float threshold, kinet_stream_t stream) {
    KINET_CHECK_ARG(T >= 0 && n >= 0 && h > 0 && w > 0 && max_h > 0 && max_w > 0 && oh > 0 && ow > 0,
                    "segm_track_resolve: bad geometry");
    KINET_CHECK_ARG(T <= 32767, "segm_track_resolve: at most 32767 track slots (labels are int16)");
    KINET_CHECK_ARG(img_h > 0 && img_h <= max_h && img_w > 0 && img_w <= max_w,
                    "segm_track_resolve: the frame's size must lie inside (max_h, max_w)");
    KINET_CHECK_ARG(labels != nullptr, "segm_track_resolve: null pointer (labels)");
    KINET_CHECK_ARG(T == 0 || src != nullptr, "segm_track_resolve: null pointer (src)");
    KINET_CHECK_ARG(n == 0 || logits != nullptr, "segm_track_resolve: null pointer (logits)");
    KINET_CHECK_ARG(labels != prev_labels, "segm_track_resolve: labels and prev_labels must be two buffers");
    const long total = (long)oh * ow;
    const float bh = (float)h / (float)max_h, bw = (float)w / (float)max_w;
    const float nh = (float)img_h / (float)oh, nw = (float)img_w / (float)ow;
    hipLaunchKernelGGL(segm_track_resolve_kernel, dim3(segm_grid(total)), dim3(256), 0, (hipStream_t)stream, logits, src,
                       prev_labels, labels, T, n, total, h, w, img_h, img_w, ow, bh, bw, nh, nw, threshold);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_segm_track_resolve_segments(const float* logits, const int32_t* src, const int32_t* src_off,
                                                 const int32_t* geom, const int64_t* pix_off,
                                                 const int16_t* prev_labels, const int64_t* prev_off, int16_t* labels,
                                                 int32_t* stats, int S, int total, int n, int h, int w, int max_h,
                                                 int max_w, float threshold, kinet_stream_t stream) {
    KINET_CHECK_ARG(S >= 0 && total >= 0 && n >= 0 && h > 0 && w > 0 && max_h > 0 && max_w > 0,
                    "segm_track_resolve_segments: bad geometry");
    if (S == 0) return KINET_OK;
    KINET_CHECK_ARG(src_off && geom && pix_off && prev_off,
                    "segm_track_resolve_segments: null pointer (the segments' host tables)");
    KINET_CHECK_ARG(src_off[0] >= 0 && pix_off[0] >= 0, "segm_track_resolve_segments: negative offset");
    long blocks = 0, pixels = 0;
    bool stale_map = false;
    for (int s = 0; s < S; ++s) {
        const long T = (long)src_off[s + 1] - src_off[s];
        KINET_CHECK_ARG(T >= 0 && pix_off[s + 1] >= pix_off[s], "segm_track_resolve_segments: offsets must ascend");
        KINET_CHECK_ARG(T <= 32767, "segm_track_resolve_segments: at most 32767 track slots per segment (labels are int16)");
        const int32_t* g = geom + 4L * s;
        const long px = (long)g[2] * g[3];
        KINET_CHECK_ARG(g[2] >= 0 && g[3] >= 0 && px <= pix_off[s + 1] - pix_off[s],
                        "segm_track_resolve_segments: a map of (oh, ow) must fit its range of pix_off");
        if (px == 0) continue;   // (no map: nothing of this segment is read or written, its stats stay 0)
        KINET_CHECK_ARG(g[0] > 0 && g[0] <= max_h && g[1] > 0 && g[1] <= max_w,
                        "segm_track_resolve_segments: a frame's size must lie inside (max_h, max_w)");
        blocks += (px + RESOLVE_PPB - 1) / RESOLVE_PPB;
        pixels += px;
        stale_map = stale_map || prev_off[s] >= 0;
    }
    KINET_CHECK_ARG(src_off[S] <= total, "segm_track_resolve_segments: src_off[S] beyond the `total` slots");
    KINET_CHECK_ARG(blocks <= 0x7fffffffL, "segm_track_resolve_segments: maps too large");
    if (pixels == 0 && total == 0) return KINET_OK;
    KINET_CHECK_ARG(pixels == 0 || labels != nullptr, "segm_track_resolve_segments: null pointer (labels)");
    KINET_CHECK_ARG(total == 0 || (src != nullptr && stats != nullptr), "segm_track_resolve_segments: null pointer (src, stats)");
    KINET_CHECK_ARG(n == 0 || logits != nullptr, "segm_track_resolve_segments: null pointer (logits)");
    KINET_CHECK_ARG(!stale_map || prev_labels != nullptr, "segm_track_resolve_segments: null pointer (prev_labels)");
    KINET_CHECK_ARG(labels == nullptr || labels != prev_labels,
                    "segm_track_resolve_segments: labels and prev_labels must be two buffers");
    hipStream_t st = (hipStream_t)stream;
    if (total > 0) KINET_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)total * 5 * sizeof(int32_t), st));
    if (pixels == 0) return KINET_OK;
    const float bh = (float)h / (float)max_h, bw = (float)w / (float)max_w;
    for (int s0 = 0; s0 < S; s0 += RESOLVE_SEGS) {
        ResolveSegs segs = {};
        const int ns = std::min(RESOLVE_SEGS, S - s0);
        int blk = 0;
        for (int k = 0; k < ns; ++k) {
            const int s = s0 + k;
            const int32_t* g = geom + 4L * s;
            ResolveSeg& r = segs.s[k];
            const long px = (long)g[2] * g[3];
            r.pix_off = pix_off[s], r.prev_off = prev_off[s];
            r.src_off = src_off[s], r.T = src_off[s + 1] - src_off[s];
            r.img_h = g[0], r.img_w = g[1], r.oh = g[2], r.ow = g[3];
            r.blk0 = blk;
            r.nh = px ? (float)g[0] / (float)g[2] : 0.f, r.nw = px ? (float)g[1] / (float)g[3] : 0.f;
            blk += (int)((px + RESOLVE_PPB - 1) / RESOLVE_PPB);
        }
        if (blk == 0) continue;
        hipLaunchKernelGGL(segm_track_resolve_segments_kernel, dim3(blk), dim3(256), 0, st, logits, src, prev_labels,
                           labels, stats, segs, ns, n, h, w, bh, bw, threshold);
    }
    if (total > 0)
        hipLaunchKernelGGL(segm_resolve_stats_finish, dim3((total + 255) / 256), dim3(256), 0, st, stats, total);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}
