// Mask training of DeformableDETRSegm: the fused mask losses (bilinear upsample + sigmoid focal +
// dice, forward and backward) and the backward of the head's own ops (joint-softmax attention map,
// ReLU + nearest upsample + FPN add, the C -> 1 output convolution).
// C-ABI: include/kinet_segm.h.  f32 only.  No float atomics: every sum runs in an order fixed by
// the shapes (thread-strided partials, a symmetric butterfly over the wave, the waves and then the
// blocks in index order), so reruns are bit-identical.
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>

#include "../../include/kinet_segm.h"
#include "common.h"
#include "segm_resize.h"

namespace kinet {
namespace {

inline int train_grid(long total) {
    const long blocks = (total + 255) / 256;
    return (int)(blocks < 1 ? 1 : (blocks > 8L * kMaxGridStride ? 8L * kMaxGridStride : blocks));
}

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

// ---------------------------------------------------------------------------------
// fused mask loss
// ---------------------------------------------------------------------------------
// Everything both directions need of one full-resolution pixel: p = sigmoid(v), q = 1 - p (formed
// without the cancellation of 1 - p), softplus(v) and softplus(-v).
struct PixelTerms {
    float p, q, sp_pos, sp_neg;
};

__device__ __forceinline__ PixelTerms pixel_terms(float v) {
    const float e = expf(-fabsf(v));
    const float inv = 1.f / (1.f + e);
    const float l = log1pf(e);
    PixelTerms t;
    t.p = v >= 0.f ? inv : e * inv;
    t.q = v >= 0.f ? e * inv : inv;
    t.sp_pos = fmaxf(v, 0.f) + l;
    t.sp_neg = fmaxf(-v, 0.f) + l;
    return t;
}

// the bilinear sample of one (h, w) row of logits at full-resolution pixel (Y, X)
struct Taps {
    int i0, i1;
    float l;
};

__device__ __forceinline__ Taps taps(int dst, float scale, int in) {
    Taps t;
    bilinear_src(dst, scale, in, t.i0, t.i1, t.l);
    return t;
}

__device__ __forceinline__ float bilinear_at(const float* __restrict__ lg, int w, const Taps& ty, const Taps& tx) {
    const float* r0 = lg + (long)ty.i0 * w;
    const float* r1 = lg + (long)ty.i1 * w;
    const float top = (1.f - tx.l) * r0[tx.i0] + tx.l * r0[tx.i1];
    const float bot = (1.f - tx.l) * r1[tx.i0] + tx.l * r1[tx.i1];
    return (1.f - ty.l) * top + ty.l * bot;
}

constexpr int LOSS_GROUPS_PER_BLOCK = 1024;   // runs of 4 target bytes a block owns (4 per thread)

// grid (nblk, n): block (blk, r) sums a contiguous run of row r's pixels.  The row's bytes are
// cut into 4-byte groups aligned to the ADDRESS (a row of H*W bytes starts anywhere), so that a
// group inside the row is one aligned 32-bit load; the first and last group of a row are read
// byte by byte.  part[r][blk][4].
__global__ __launch_bounds__(256) void mask_loss_kernel(const float* __restrict__ logits,
                                                        const uint8_t* __restrict__ target, float* __restrict__ part,
                                                        int h, int w, int H, int W, float bh, float bw, float alpha) {
    __shared__ float red[4];
    const int r = blockIdx.y;
    const int HW = H * W;
    const uint8_t* trow = target + (long)r * HW;
    const float* lg = logits + (long)r * h * w;
    const int a = (int)((uintptr_t)trow & 3);
    const int ngroups = (HW + a + 3) / 4;
    const int g0 = blockIdx.x * LOSS_GROUPS_PER_BLOCK, g1 = min(ngroups, g0 + LOSS_GROUPS_PER_BLOCK);
    const float a1 = alpha >= 0.f ? alpha : 1.f, a0 = alpha >= 0.f ? 1.f - alpha : 1.f;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int g = g0 + (int)threadIdx.x; g < g1; g += 256) {
        const int i0 = 4 * g - a;   // the row-local pixel of the group's first byte
        uint32_t bytes = 0;
        if (i0 >= 0 && i0 + 4 <= HW) {
            bytes = *reinterpret_cast<const uint32_t*>(trow + i0);
        } else {
            for (int k = 0; k < 4; ++k)
                if (i0 + k >= 0 && i0 + k < HW) bytes |= (uint32_t)trow[i0 + k] << (8 * k);
        }
        const int first = max(i0, 0);
        int Y = first / W, X = first - Y * W;
        Taps ty = taps(Y, bh, h);
        for (int k = first - i0; k < 4 && i0 + k < HW; ++k) {
            const bool t = ((bytes >> (8 * k)) & 0xffu) != 0;
            const float v = bilinear_at(lg, w, ty, taps(X, bw, w));
            const PixelTerms pt = pixel_terms(v);
            const float m = t ? pt.q : pt.p;   // 1 - p_t
            s0 += (t ? a1 * pt.sp_neg : a0 * pt.sp_pos) * (m * m);
            s1 += t ? pt.p : 0.f;
            s2 += pt.p;
            s3 += t ? 1.f : 0.f;
            if (++X == W) {
                X = 0;
                ++Y;
                ty = taps(min(Y, H - 1), bh, h);
            }
        }
    }
    s0 = block_sum(s0, red);
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    s3 = block_sum(s3, red);
    if (threadIdx.x == 0) {
        float* o = part + ((long)r * gridDim.x + blockIdx.x) * 4;
        o[0] = s0, o[1] = s1, o[2] = s2, o[3] = s3;
    }
}

// one block: the rows' block partials in block order, then the two losses over the rows in order
__global__ __launch_bounds__(256) void mask_loss_finalize_kernel(const float* __restrict__ part,
                                                                 float* __restrict__ sums, float* __restrict__ loss,
                                                                 int n, int nblk, float hw, float num_boxes) {
    for (int r = threadIdx.x; r < n; r += 256) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        const float* p = part + (long)r * nblk * 4;
        for (int b = 0; b < nblk; ++b)
            for (int j = 0; j < 4; ++j) s[j] += p[b * 4 + j];
        for (int j = 0; j < 4; ++j) sums[(long)r * 4 + j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float f = 0.f, d = 0.f;
        for (int r = 0; r < n; ++r) {
            const float* s = sums + (long)r * 4;
            f += s[0] / hw;
            d += 1.f - (2.f * s[1] + 1.f) / (s[2] + s[3] + 1.f);
        }
        loss[0] = f / num_boxes;
        loss[1] = d / num_boxes;
    }
}

// The full-resolution positions that can have `src` among their two bilinear taps, with one
// position of slack on each side (the caller tests every candidate with the forward's rule).
__device__ __forceinline__ void bilinear_children(int src, float inv_scale, int out, int& lo, int& hi) {
    lo = max(0, (int)floorf(((float)src - 0.5f) * inv_scale - 0.5f) - 1);
    hi = min(out - 1, (int)ceilf(((float)src + 1.5f) * inv_scale - 0.5f) + 1);
}

__device__ __forceinline__ float tap_weight(const Taps& t, int src) {
    return (t.i0 == src ? 1.f - t.l : 0.f) + (t.i1 == src ? t.l : 0.f);
}

// one thread per low-resolution pixel (r, y, x)
__global__ __launch_bounds__(256) void mask_loss_backward_kernel(const float* __restrict__ logits,
                                                                 const uint8_t* __restrict__ target,
                                                                 const float* __restrict__ sums,
                                                                 const float* __restrict__ dloss,
                                                                 float* __restrict__ dlogits, long total, int h, int w,
                                                                 int H, int W, float bh, float bw, float alpha,
                                                                 float num_boxes) {
    const float a1 = alpha >= 0.f ? alpha : 1.f, a0 = alpha >= 0.f ? 1.f - alpha : 1.f;
    const float gf = dloss[0] / ((float)H * (float)W) / num_boxes;   // per focal term
    const float gd = dloss[1] / num_boxes;                           // per row's dice term
    const float ih = 1.f / bh, iw = 1.f / bw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int x = (int)(i % w);
        const long t_ = i / w;
        const int y = (int)(t_ % h);
        const long r = t_ / h;
        const float* lg = logits + r * h * w;
        const uint8_t* trow = target + r * H * W;
        // dice_r = 1 - N / D with N = 2 sum(p t) + 1, D = sum(p) + sum(t) + 1:
        // d dice_r / d p_i = (N - 2 t_i D) / D^2
        const float* s = sums + r * 4;
        const float Nn = 2.f * s[1] + 1.f, D = s[2] + s[3] + 1.f;
        const float c0 = gd * Nn / (D * D), c1 = gd * (Nn - 2.f * D) / (D * D);
        int Ylo, Yhi, Xlo, Xhi;
        bilinear_children(y, ih, H, Ylo, Yhi);
        bilinear_children(x, iw, W, Xlo, Xhi);
        float acc = 0.f;
        for (int Y = Ylo; Y <= Yhi; ++Y) {
            const Taps ty = taps(Y, bh, h);
            const float wy = tap_weight(ty, y);
            if (wy == 0.f) continue;
            float row = 0.f;
            for (int X = Xlo; X <= Xhi; ++X) {
                const Taps tx = taps(X, bw, w);
                const float wx = tap_weight(tx, x);
                if (wx == 0.f) continue;
                const float v = bilinear_at(lg, w, ty, tx);
                const PixelTerms pt = pixel_terms(v);
                const bool t = trow[(long)Y * W + X] != 0;
                // t = 1: focal = a1 softplus(-v) q^2,  d/dv = -a1 q^2 (q + 2 p softplus(-v))
                // t = 0: focal = a0 softplus(v) p^2,   d/dv =  a0 p^2 (p + 2 q softplus(v))
                const float df = t ? -a1 * pt.q * pt.q * (pt.q + 2.f * pt.p * pt.sp_neg)
                                   : a0 * pt.p * pt.p * (pt.p + 2.f * pt.q * pt.sp_pos);
                row += (gf * df + (t ? c1 : c0) * (pt.p * pt.q)) * wx;
            }
            acc += row * wy;
        }
        dlogits[i] = acc;
    }
}

// ---------------------------------------------------------------------------------
// attention map backward
// ---------------------------------------------------------------------------------
// grid (rows): s[r] = sum att * datt, then dqp[r] (thread c owns channel c, the pixels in order)
__global__ __launch_bounds__(256) void attention_backward_q_kernel(const float* __restrict__ datt,
                                                                   const float* __restrict__ att,
                                                                   const float* __restrict__ kp, float* __restrict__ dqp,
                                                                   float* __restrict__ srow, int Q, int HW, int heads,
                                                                   int d, float scale) {
    __shared__ float red[4];
    const int r = blockIdx.x, b = r / Q;
    const long n = (long)HW * heads;
    const float* a = att + (long)r * n;
    const float* g = datt + (long)r * n;
    float acc = 0.f;
    for (long i = threadIdx.x; i < n; i += 256) acc += a[i] * g[i];
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) srow[r] = s;
    if (!dqp) return;
    const int D = d / heads;
    const float* kb = kp + (long)b * HW * d;
    for (int c = threadIdx.x; c < d; c += 256) {
        const int hd = c / D;
        float q = 0.f;
        for (int p = 0; p < HW; ++p) {
            const float av = a[(long)p * heads + hd];
            q += av * (g[(long)p * heads + hd] - s) * kb[(long)p * d + c];
        }
        dqp[(long)r * d + c] = scale * q;
    }
}

// one thread per (b, p, c): the frame's rows in ascending order
__global__ __launch_bounds__(256) void attention_backward_k_kernel(const float* __restrict__ datt,
                                                                   const float* __restrict__ att,
                                                                   const float* __restrict__ qp,
                                                                   const float* __restrict__ srow,
                                                                   float* __restrict__ dkp, long total, int Q, int HW,
                                                                   int heads, int d, float scale) {
    const int D = d / heads;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % d);
        const long t = i / d;
        const int p = (int)(t % HW);
        const long b = t / HW;
        const int hd = c / D;
        float acc = 0.f;
        for (int q = 0; q < Q; ++q) {
            const long r = b * Q + q;
            const long o = (r * HW + p) * heads + hd;
            acc += att[o] * (datt[o] - srow[r]) * qp[r * d + c];
        }
        dkp[i] = scale * acc;
    }
}

// ---------------------------------------------------------------------------------
// ReLU + nearest upsample + FPN add; a thread moves 4 channels
// ---------------------------------------------------------------------------------
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

__global__ __launch_bounds__(256) void relu_up_add_kernel(const float* __restrict__ x, const float* __restrict__ f,
                                                          float* __restrict__ y, long total, int row0, int Q, int h,
                                                          int w, int H, int W, int C, float sh, float sw) {
    const int CV = C / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int cv = (int)(i % CV);
        long t = i / CV;
        const int X = (int)(t % W);
        t /= W;
        const int Y = (int)(t % H);
        const long r = t / H;
        const int sy = nearest_src(Y, sh, h), sx = nearest_src(X, sw, w);
        const float4 v = ld4(x + ((r * h + sy) * w + sx) * C + cv * 4);
        float4 o = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
        if (f) {
            const float4 fv = ld4(f + ((((long)row0 + r) / Q * H + Y) * W + X) * C + cv * 4);
            o.x += fv.x, o.y += fv.y, o.z += fv.z, o.w += fv.w;
        }
        st4(y + i * 4, o);
    }
}

// the output positions whose nearest source can be `src`, with one position of slack each side
__device__ __forceinline__ void nearest_children(int src, float inv_scale, int out, int& lo, int& hi) {
    lo = max(0, (int)floorf((float)src * inv_scale) - 1);
    hi = min(out - 1, (int)ceilf((float)(src + 1) * inv_scale) + 1);
}

// one thread per (r, y, x, 4 channels) of dx
__global__ __launch_bounds__(256) void relu_up_add_dx_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                             float* __restrict__ dx, long total, int h, int w, int H,
                                                             int W, int C, float sh, float sw) {
    const int CV = C / 4;
    const float ih = 1.f / sh, iw = 1.f / sw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int cv = (int)(i % CV);
        long t = i / CV;
        const int xs = (int)(t % w);
        t /= w;
        const int ys = (int)(t % h);
        const long r = t / h;
        int Ylo, Yhi, Xlo, Xhi;
        nearest_children(ys, ih, H, Ylo, Yhi);
        nearest_children(xs, iw, W, Xlo, Xhi);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int Y = Ylo; Y <= Yhi; ++Y) {
            if (nearest_src(Y, sh, h) != ys) continue;
            for (int X = Xlo; X <= Xhi; ++X) {
                if (nearest_src(X, sw, w) != xs) continue;
                const float4 g = ld4(dy + ((r * H + Y) * W + X) * C + cv * 4);
                acc.x += g.x, acc.y += g.y, acc.z += g.z, acc.w += g.w;
            }
        }
        const float4 v = ld4(x + i * 4);
        st4(dx + i * 4, make_float4(v.x > 0.f ? acc.x : 0.f, v.y > 0.f ? acc.y : 0.f, v.z > 0.f ? acc.z : 0.f,
                                    v.w > 0.f ? acc.w : 0.f));
    }
}

// one thread per (b, Y, X, 4 channels) of df: the call's rows of frame b in ascending order
__global__ __launch_bounds__(256) void relu_up_add_df_kernel(const float* __restrict__ dy, float* __restrict__ df,
                                                             long total, int rows, int row0, int Q, long per_row) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / per_row, o = i % per_row;
        const long lo = std::max<long>(b * Q, row0) - row0, hi = std::min<long>((b + 1) * Q, (long)row0 + rows) - row0;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (long r = lo; r < hi; ++r) {
            const float4 g = ld4(dy + (r * per_row + o) * 4);
            acc.x += g.x, acc.y += g.y, acc.z += g.z, acc.w += g.w;
        }
        st4(df + i * 4, acc);
    }
}

// ---------------------------------------------------------------------------------
// out_lay backward
// ---------------------------------------------------------------------------------
constexpr int OUT_MAX_C = 64;

// one thread per (r, y, x, c) of dx
__global__ __launch_bounds__(256) void out_conv_dx_kernel(const float* __restrict__ dy, const float* __restrict__ wt,
                                                          float* __restrict__ dx, long total, int H, int W, int C) {
    __shared__ float w_s[9 * OUT_MAX_C];
    for (int k = threadIdx.x; k < 9 * C; k += 256) w_s[k] = wt[k];
    __syncthreads();
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        long t = i / C;
        const int x = (int)(t % W);
        t /= W;
        const int y = (int)(t % H);
        const long r = t / H;
        float acc = 0.f;
        for (int ky = 0; ky < 3; ++ky) {
            const int Y = y - ky + 1;
            if (Y < 0 || Y >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int X = x - kx + 1;
                if (X < 0 || X >= W) continue;
                acc = fmaf(dy[(r * H + Y) * W + X], w_s[(ky * 3 + kx) * C + c], acc);
            }
        }
        dx[i] = acc;
    }
}

// Block blk owns the pixels [blk * ppb, (blk + 1) * ppb) of the rows*H*W outputs; thread (lane, c)
// = (tid / C, tid % C) sums its pixels' nine products for channel c (and dy itself for the bias),
// then each of the 9*C + 1 outputs adds the lanes in order.  part[blk][9*C + 1].
__global__ __launch_bounds__(256) void out_conv_dw_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          float* __restrict__ part, long total, long ppb, int H, int W,
                                                          int C) {
    __shared__ float red[10][256];
    const int PP = 256 / C;
    const int lane = threadIdx.x / C, c = threadIdx.x % C;
    float acc[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.f;
    if (lane < PP) {
        const long p0 = (long)blockIdx.x * ppb, p1 = std::min<long>(total, p0 + ppb);
        for (long p = p0 + lane; p < p1; p += PP) {
            const float g = dy[p];
            const int X = (int)(p % W);
            const long t = p / W;
            const int Y = (int)(t % H);
            const long r = t / H;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int yy = Y + ky - 1;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int xx = X + kx - 1;
                    if (yy >= 0 && yy < H && xx >= 0 && xx < W)
                        acc[ky * 3 + kx] = fmaf(g, x[((r * H + yy) * W + xx) * C + c], acc[ky * 3 + kx]);
                }
            }
            acc[9] += g;
        }
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    const int nout = 9 * C + 1;
    for (int o = threadIdx.x; o < nout; o += 256) {
        const int k = o < 9 * C ? o / C : 9, ch = o < 9 * C ? o % C : 0;
        float s = 0.f;
        for (int l = 0; l < PP; ++l) s += red[k][l * C + ch];
        part[(long)blockIdx.x * nout + o] = s;
    }
}

__global__ __launch_bounds__(256) void out_conv_dw_finalize_kernel(const float* __restrict__ part,
                                                                   float* __restrict__ dwt, float* __restrict__ dbias,
                                                                   int nblk, int C) {
    const int nout = 9 * C + 1;
    for (int o = blockIdx.x * 256 + threadIdx.x; o < nout; o += gridDim.x * 256) {
        float s = 0.f;
        for (int b = 0; b < nblk; ++b) s += part[(long)b * nout + o];
        if (o < 9 * C) dwt[o] = s;
        else dbias[0] = s;
    }
}

inline long loss_blocks(int H, int W) {
    const long groups = ((long)H * W + 3 + 3) / 4;   // (+3: a row may start at any byte of a 4-byte word)
    return (groups + LOSS_GROUPS_PER_BLOCK - 1) / LOSS_GROUPS_PER_BLOCK;
}

inline void out_conv_plan(long total, long& ppb, long& nblk) {
    ppb = std::max<long>(1024, (total + kMaxGridStride - 1) / kMaxGridStride);
    nblk = (total + ppb - 1) / ppb;
}

inline bool loss_geometry_ok(int n, int h, int w, int H, int W) {
    return n >= 0 && h > 0 && w > 0 && H >= h && W >= w && (long)H * W <= 0x3fffffffL && n <= 65535;
}

}  // namespace
}  // namespace kinet

using namespace kinet;

extern "C" long kinet_segm_mask_loss_workspace(int n, int H, int W) {
    if (n <= 0 || H <= 0 || W <= 0) return 0;
    return (long)n * loss_blocks(H, W) * 4;
}

extern "C" int kinet_segm_mask_loss(const float* logits, const uint8_t* target, float* sums, float* loss, int n, int h,
                                    int w, int H, int W, float alpha, float gamma, float num_boxes, float* ws,
                                    kinet_stream_t stream) {
    KINET_CHECK_ARG(loss_geometry_ok(n, h, w, H, W),
                    "segm_mask_loss: bad geometry (the target must be at least the logits' size; at most 65535 rows)");
    KINET_CHECK_ARG(gamma == 2.f, "segm_mask_loss: gamma must be 2 (the reference's hard-wired default)");
    KINET_CHECK_ARG(num_boxes > 0.f, "segm_mask_loss: num_boxes must be positive");
    KINET_CHECK_ARG(loss != nullptr, "segm_mask_loss: null pointer (loss)");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        KINET_CHECK_HIP(hipMemsetAsync(loss, 0, 2 * sizeof(float), s));
        return KINET_OK;
    }
    KINET_CHECK_ARG(logits && target && sums, "segm_mask_loss: null pointer");
    KINET_CHECK_ARG(ws != nullptr, "segm_mask_loss: workspace of kinet_segm_mask_loss_workspace() floats required");
    const int nblk = (int)loss_blocks(H, W);
    const float bh = (float)h / (float)H, bw = (float)w / (float)W;   // torch's scales: input / output in f32
    hipLaunchKernelGGL(mask_loss_kernel, dim3(nblk, n), dim3(256), 0, s, logits, target, ws, h, w, H, W, bh, bw, alpha);
    hipLaunchKernelGGL(mask_loss_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, sums, loss, n, nblk,
                       (float)H * (float)W, num_boxes);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_segm_mask_loss_backward(const float* logits, const uint8_t* target, const float* sums,
                                             const float* dloss, float* dlogits, int n, int h, int w, int H, int W,
                                             float alpha, float gamma, float num_boxes, kinet_stream_t stream) {
    KINET_CHECK_ARG(loss_geometry_ok(n, h, w, H, W),
                    "segm_mask_loss_backward: bad geometry (the target must be at least the logits' size; at most 65535 rows)");
    KINET_CHECK_ARG(gamma == 2.f, "segm_mask_loss_backward: gamma must be 2 (the reference's hard-wired default)");
    KINET_CHECK_ARG(num_boxes > 0.f, "segm_mask_loss_backward: num_boxes must be positive");
    if (n == 0) return KINET_OK;
    KINET_CHECK_ARG(logits && target && sums && dloss && dlogits, "segm_mask_loss_backward: null pointer");
    const long total = (long)n * h * w;
    const float bh = (float)h / (float)H, bw = (float)w / (float)W;
    hipLaunchKernelGGL(mask_loss_backward_kernel, dim3(train_grid(total)), dim3(256), 0, (hipStream_t)stream, logits,
                       target, sums, dloss, dlogits, total, h, w, H, W, bh, bw, alpha, num_boxes);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" long kinet_segm_attention_backward_workspace(int B, int Q) {
    return B > 0 && Q > 0 ? (long)B * Q : 0;
}

extern "C" int kinet_segm_attention_backward(const float* datt, const float* att, const float* qp, const float* kp,
                                             float* dqp, float* dkp, int B, int Q, int HW, int heads, int d, float scale,
                                             float* ws, kinet_stream_t stream) {
    KINET_CHECK_ARG(B >= 0 && Q >= 0 && HW > 0, "segm_attention_backward: bad geometry");
    KINET_CHECK_ARG(heads > 0 && heads <= 32 && (heads & (heads - 1)) == 0,
                    "segm_attention_backward: heads must be a power of two <= 32");
    KINET_CHECK_ARG(d > 0 && d <= 1024 && d % heads == 0, "segm_attention_backward: d must be a multiple of heads, <= 1024");
    KINET_CHECK_ARG((long)B * Q <= 0x7fffffffL, "segm_attention_backward: too many rows");
    if ((long)B * Q == 0) return KINET_OK;
    KINET_CHECK_ARG(datt && att && qp && kp, "segm_attention_backward: null pointer");
    KINET_CHECK_ARG(ws != nullptr, "segm_attention_backward: workspace of kinet_segm_attention_backward_workspace() floats required");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(attention_backward_q_kernel, dim3(B * Q), dim3(256), 0, s, datt, att, kp, dqp, ws, Q, HW, heads, d,
                       scale);
    if (dkp) {
        const long total = (long)B * HW * d;
        hipLaunchKernelGGL(attention_backward_k_kernel, dim3(train_grid(total)), dim3(256), 0, s, datt, att, qp,
                           (const float*)ws, dkp, total, Q, HW, heads, d, scale);
    }
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

static int relu_up_add_check(const char* who, int rows, int row0, int Q, int B, int h, int w, int H, int W, int C) {
    KINET_CHECK_ARG(rows >= 0 && row0 >= 0 && Q > 0 && B > 0 && h > 0 && w > 0, "%s: bad geometry", who);
    KINET_CHECK_ARG(H >= h && W >= w, "%s: the output must be at least the input's size", who);
    KINET_CHECK_ARG(C > 0 && C % 4 == 0, "%s: C must be a multiple of 4", who);
    KINET_CHECK_ARG((long)row0 + rows <= (long)B * Q, "%s: rows [row0, row0 + rows) outside the B*Q rows", who);
    KINET_CHECK_ARG((long)H * W * (C / 4) <= 0x3fffffffL, "%s: map too large", who);
    return KINET_OK;
}

extern "C" int kinet_segm_relu_up_add(const float* x, const float* f, float* y, int rows, int row0, int Q, int B, int h,
                                      int w, int H, int W, int C, kinet_stream_t stream) {
    if (int rc = relu_up_add_check("segm_relu_up_add", rows, row0, Q, B, h, w, H, W, C)) return rc;
    KINET_CHECK_ARG(f != nullptr || (H == h && W == w),
                    "segm_relu_up_add: without an FPN operand the output has the input's size");
    if (rows == 0) return KINET_OK;
    KINET_CHECK_ARG(x && y, "segm_relu_up_add: null pointer");
    KINET_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)f) & 15) == 0, "segm_relu_up_add: x, y and f must be 16-byte aligned");
    const long total = (long)rows * H * W * (C / 4);
    hipLaunchKernelGGL(relu_up_add_kernel, dim3(train_grid(total)), dim3(256), 0, (hipStream_t)stream, x, f, y, total,
                       row0, Q, h, w, H, W, C, (float)h / (float)H, (float)w / (float)W);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_segm_relu_up_add_backward(const float* dy, const float* x, float* dx, float* df, int rows, int row0,
                                               int Q, int B, int h, int w, int H, int W, int C, kinet_stream_t stream) {
    if (int rc = relu_up_add_check("segm_relu_up_add_backward", rows, row0, Q, B, h, w, H, W, C)) return rc;
    KINET_CHECK_ARG(rows == 0 || dy != nullptr, "segm_relu_up_add_backward: null pointer (dy)");
    KINET_CHECK_ARG(dx == nullptr || rows == 0 || x != nullptr, "segm_relu_up_add_backward: dx needs x");
    KINET_CHECK_ARG((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dx | (uintptr_t)df) & 15) == 0,
                    "segm_relu_up_add_backward: dy, x, dx and df must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dx && rows) {
        const long total = (long)rows * h * w * (C / 4);
        hipLaunchKernelGGL(relu_up_add_dx_kernel, dim3(train_grid(total)), dim3(256), 0, s, dy, x, dx, total, h, w, H, W,
                           C, (float)h / (float)H, (float)w / (float)W);
    }
    if (df) {
        const long per_row = (long)H * W * (C / 4), total = (long)B * per_row;
        hipLaunchKernelGGL(relu_up_add_df_kernel, dim3(train_grid(total)), dim3(256), 0, s, dy, df, total, rows, row0, Q,
                           per_row);
    }
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" long kinet_segm_out_conv_backward_workspace(int rows, int H, int W, int C) {
    if (rows <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    long ppb, nblk;
    out_conv_plan((long)rows * H * W, ppb, nblk);
    return nblk * (9L * C + 1);
}

extern "C" int kinet_segm_out_conv_backward(const float* dy, const float* x, const float* wt, float* dx, float* dwt,
                                            float* dbias, int rows, int H, int W, int C, float* ws,
                                            kinet_stream_t stream) {
    KINET_CHECK_ARG(rows >= 0 && H > 0 && W > 0, "segm_out_conv_backward: bad geometry");
    KINET_CHECK_ARG(C > 0 && C <= OUT_MAX_C, "segm_out_conv_backward: C must be in 1..64");
    KINET_CHECK_ARG((dwt == nullptr) == (dbias == nullptr), "segm_out_conv_backward: dwt and dbias go together");
    KINET_CHECK_ARG((long)rows * H * W * C <= 0x3fffffffffL, "segm_out_conv_backward: too large");
    hipStream_t s = (hipStream_t)stream;
    if (rows == 0) {
        if (dwt) {
            KINET_CHECK_HIP(hipMemsetAsync(dwt, 0, 9 * (size_t)C * sizeof(float), s));
            KINET_CHECK_HIP(hipMemsetAsync(dbias, 0, sizeof(float), s));
        }
        return KINET_OK;
    }
    KINET_CHECK_ARG(dy != nullptr, "segm_out_conv_backward: null pointer (dy)");
    KINET_CHECK_ARG(dx == nullptr || wt != nullptr, "segm_out_conv_backward: dx needs wt");
    KINET_CHECK_ARG(dwt == nullptr || (x != nullptr && ws != nullptr),
                    "segm_out_conv_backward: dwt needs x and a workspace of kinet_segm_out_conv_backward_workspace() floats");
    const long pixels = (long)rows * H * W;
    if (dx) {
        const long total = pixels * C;
        hipLaunchKernelGGL(out_conv_dx_kernel, dim3(train_grid(total)), dim3(256), 0, s, dy, wt, dx, total, H, W, C);
    }
    if (dwt) {
        long ppb, nblk;
        out_conv_plan(pixels, ppb, nblk);
        hipLaunchKernelGGL(out_conv_dw_kernel, dim3((int)nblk), dim3(256), 0, s, dy, x, ws, pixels, ppb, H, W, C);
        hipLaunchKernelGGL(out_conv_dw_finalize_kernel, dim3((9 * C + 1 + 255) / 256), dim3(256), 0, s,
                           (const float*)ws, dwt, dbias, (int)nblk, C);
    }
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}
