// The proposal stage of two-stage Deformable DETR (deformable_transformer.py:77-122, :180-194):
// encoder-output proposals, per-row top-k selection, gather + proposal position embedding, and
// the two row-wise glue kernels around the enc_output projection.  C-ABI: include/kinet_two_stage.h.
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>

#include "../../include/kinet_two_stage.h"
#include "common.h"

namespace kinet {
namespace {

// ---------------------------------------------------------------------------------
// proposals (:92-116)
// ---------------------------------------------------------------------------------
struct TsLevels {
    int n;
    int h[KINET_TWO_STAGE_MAX_LEVELS], w[KINET_TWO_STAGE_MAX_LEVELS], off[KINET_TWO_STAGE_MAX_LEVELS];
};

__device__ __forceinline__ float logit_f64(float p) {
    return (float)log((double)p / (1.0 - (double)p));
}

// grid (chunks, levels, B): every workgroup counts its level's valid extent (first column /
// first row of the frame's mask, H + W byte reads), then writes a grid-strided share of the level
__global__ __launch_bounds__(256) void proposals_kernel(TsLevels lv, const uint8_t* __restrict__ mask,
                                                        float* __restrict__ prop, uint8_t* __restrict__ keep, int S) {
    const int l = blockIdx.y, b = blockIdx.z;
    const int H = lv.h[l], W = lv.w[l], off = lv.off[l];
    __shared__ int cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint8_t* m = mask ? mask + (long)b * S + off : nullptr;
    if (m) {
        int ch = 0, cw = 0;
        for (int i = threadIdx.x; i < H; i += blockDim.x) ch += m[(long)i * W] ? 0 : 1;
        for (int j = threadIdx.x; j < W; j += blockDim.x) cw += m[j] ? 0 : 1;
        if (ch) atomicAdd(&cnt[0], ch);
        if (cw) atomicAdd(&cnt[1], cw);
        __syncthreads();
    }
    const float vh = m ? (float)cnt[0] : (float)H;
    const float vw = m ? (float)cnt[1] : (float)W;
    const float wh = ldexpf(0.05f, l);   // ones * 0.05 * 2**lvl in f32 (a power-of-two scale: exact)
    const bool wh_ok = wh > 0.01f && wh < 0.99f;
    const float inf = __builtin_inff();
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < H * W; t += gridDim.x * blockDim.x) {
        const int i = t / W, j = t - i * W;
        // correctly rounded f32 division: (0.5f / 50.f) is exactly 0.01f and therefore invalid
        const float x = __fdiv_rn((float)j + 0.5f, vw);
        const float y = __fdiv_rn((float)i + 0.5f, vh);
        const bool ok = wh_ok && x > 0.01f && x < 0.99f && y > 0.01f && y < 0.99f && !(m && m[t]);
        float4 o = make_float4(inf, inf, inf, inf);
        if (ok) {
            const float lw = logit_f64(wh);
            o = make_float4(logit_f64(x), logit_f64(y), lw, lw);
        }
        const long r = (long)b * S + off + t;
        *reinterpret_cast<float4*>(prop + r * 4) = o;
        keep[r] = ok ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------
// top-k per row
// ---------------------------------------------------------------------------------
constexpr int TK_THREADS = 1024;
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int TK_BINS = 2048;
constexpr int TK_CACHE = 36000;   // keys of a row kept in LDS (144 000 B of the CU's 160 KiB)
constexpr int TK_BATCH = 4;       // independent global loads a thread has in flight

// order-preserving integer key of torch's descending order: NaN above everything (all NaN
// equal), -0.0 == +0.0, then the usual sign-flip of the IEEE bits
__device__ __forceinline__ uint32_t topk_key(float v) {
    if (v != v) return 0xFFFFFFFFu;
    uint32_t u = __float_as_uint(v);
    if (v == 0.f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// f(i, key) for every entry i of the row this thread owns (i = tid + n * TK_THREADS, ascending).
// FIRST: read the scores from global memory, TK_BATCH strided loads in flight per thread (an
// entry of channel 0 of (B, S, 91) logits is alone on its cache line: the sweep is latency-bound),
// and with CACHE leave the keys in LDS; later sweeps with CACHE read them back from there.
template <bool CACHE, bool FIRST, typename F>
__device__ __forceinline__ void sweep_keys(const float* __restrict__ row, long es, int S, uint32_t* skeys, F f) {
    const int tid = threadIdx.x;
    if (CACHE && !FIRST) {
        for (int i = tid; i < S; i += TK_THREADS) f(i, skeys[i]);
        return;
    }
    for (int i0 = tid; i0 < S; i0 += TK_BATCH * TK_THREADS) {
        float v[TK_BATCH];
#pragma unroll
        for (int u = 0; u < TK_BATCH; ++u) {
            const int i = i0 + u * TK_THREADS;
            v[u] = i < S ? row[(long)i * es] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < TK_BATCH; ++u) {
            const int i = i0 + u * TK_THREADS;
            if (i < S) {
                const uint32_t key = topk_key(v[u]);
                if (CACHE) skeys[i] = key;
                f(i, key);
            }
        }
    }
}

// One workgroup per row.  (1) radix-select the key T of the k-th largest entry in three passes
// (11 + 11 + 10 bits from the top) of LDS histograms over the entries that match the prefix so
// far; (2) one ordered sweep compacts the entries > T and the first k - #greater entries == T by
// ascending index into LDS; (3) a bitonic sort of the k winners on (key, ~index), descending.
// CACHE (S <= TK_CACHE): the first sweep leaves the row's keys in LDS and the other three read
// them there; longer rows re-read global memory (L2-resident after the first sweep).
template <bool CACHE>
__global__ __launch_bounds__(TK_THREADS) void topk_rows_kernel(const float* __restrict__ scores, long row_stride,
                                                               long elem_stride, int S, int k,
                                                               int64_t* __restrict__ out) {
    __shared__ uint32_t hist[TK_BINS];
    __shared__ uint32_t sel[2];
    __shared__ int wcnt[2][TK_WAVES][2];
    __shared__ unsigned long long win[KINET_TOPK_MAX_K];
    __shared__ uint32_t skeys[CACHE ? TK_CACHE : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = scores + (long)blockIdx.x * row_stride;

    uint32_t prefix = 0, pmask = 0, kr = (uint32_t)k;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        const int nb = pass == 2 ? 1024 : 2048;
        for (int i = tid; i < nb; i += TK_THREADS) hist[i] = 0;
        __syncthreads();
        auto count = [&](int, uint32_t key) {
            if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & (nb - 1)], 1u);
        };
        if (pass == 0)
            sweep_keys<CACHE, true>(row, elem_stride, S, skeys, count);
        else
            sweep_keys<CACHE, false>(row, elem_stride, S, skeys, count);
        __syncthreads();
        if (wave == 0) {
            // lane l owns the `per` bins below nb - l*per, walked from the top
            const int per = nb / 64, top = nb - 1 - lane * per;
            uint32_t s = 0;
            for (int q = 0; q < per; ++q) s += hist[top - q];
            uint32_t incl = s;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            uint32_t c = incl - s;
            if (c < kr && kr <= incl) {
                for (int q = 0; q < per; ++q) {
                    const uint32_t h = hist[top - q];
                    if (c + h >= kr) {
                        sel[0] = (uint32_t)(top - q);
                        sel[1] = kr - c;
                        break;
                    }
                    c += h;
                }
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        kr = sel[1];
        pmask |= (uint32_t)(nb - 1) << shift;
    }
    // prefix is the full key T; kr entries equal to T are taken, G = k - kr are greater
    const uint32_t T = prefix;
    const int G = k - (int)kr;
    int gbase = 0, ebase = 0;
    const int chunks = (S + TK_THREADS - 1) / TK_THREADS;
    auto fetch = [&](int i) -> uint32_t {
        if (i >= S) return 0u;
        return CACHE ? skeys[i] : topk_key(row[(long)i * elem_stride]);
    };
    uint32_t next = fetch(tid);
#pragma unroll 1
    for (int c = 0; c < chunks; ++c) {
        const int i = c * TK_THREADS + tid;
        const uint32_t key = next;
        next = fetch(i + TK_THREADS);   // the next chunk's load is in flight across the barrier
        const bool g = i < S && key > T, e = i < S && key == T;
        const unsigned long long bg = __ballot(g), be = __ballot(e);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int pg = __popcll(bg & below), pe = __popcll(be & below);
        if (lane == 0) {
            wcnt[c & 1][wave][0] = __popcll(bg);
            wcnt[c & 1][wave][1] = __popcll(be);
        }
        __syncthreads();
        int og = 0, oe = 0, tg = 0, te = 0;
#pragma unroll
        for (int w = 0; w < TK_WAVES; ++w) {
            const int ng = wcnt[c & 1][w][0], ne = wcnt[c & 1][w][1];
            if (w < wave) {
                og += ng;
                oe += ne;
            }
            tg += ng;
            te += ne;
        }
        const unsigned long long comp = ((unsigned long long)key << 32) | (uint32_t)(~(uint32_t)i);
        if (g) {
            const int slot = gbase + og + pg;
            if (slot < G) win[slot] = comp;
        } else if (e) {
            const int pos = ebase + oe + pe;
            if (pos < (int)kr && G + pos < k) win[G + pos] = comp;
        }
        gbase += tg;
        ebase += te;
    }
    int n = 1;
    while (n < k) n <<= 1;
    for (int t = k + tid; t < n; t += TK_THREADS) win[t] = 0ull;   // below every real (key, ~index)
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            const int p = tid ^ stride;
            if (tid < n && p > tid) {
                const unsigned long long a = win[tid], b = win[p];
                const bool up = (tid & size) == 0;
                if ((a < b) == up) {
                    win[tid] = b;
                    win[p] = a;
                }
            }
        }
    }
    __syncthreads();
    if (tid < k) out[(long)blockIdx.x * k + tid] = (int64_t)(uint32_t)(~(uint32_t)win[tid]);
}

// ---------------------------------------------------------------------------------
// gather + proposal position embedding (:77-90, :189-193)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void store_pair(float* p, float a, float b) { *reinterpret_cast<float2*>(p) = make_float2(a, b); }
__device__ __forceinline__ void store_pair(bf16_t* p, float a, float b) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)f32_to_bf16(a).x | ((uint32_t)f32_to_bf16(b).x << 16);
}
__device__ __forceinline__ void store_pair(f16_t* p, float a, float b) {
    const f16_t ha = (f16_t)a, hb = (f16_t)b;
    *reinterpret_cast<uint32_t*>(p) =
        (uint32_t)__builtin_bit_cast(uint16_t, ha) | ((uint32_t)__builtin_bit_cast(uint16_t, hb) << 16);
}

// one workgroup per selected proposal: thread (c, m) = (tid / 64, tid % 64) owns the sin / cos
// pair (features 2m, 2m + 1) of box coordinate c
template <typename TO>
__global__ __launch_bounds__(256) void queries_kernel(const float* __restrict__ coord, const int64_t* __restrict__ idx,
                                                      const float* __restrict__ dim_t, float* __restrict__ ref,
                                                      TO* __restrict__ pos, int S, int k) {
    const long q = blockIdx.x;
    const long b = q / k;
    const int c = threadIdx.x >> 6, m = threadIdx.x & 63;
    const int64_t i = idx[q];
    float sg = __builtin_nanf("");
    if (i >= 0 && i < S) {
        const float x = coord[(b * S + i) * 4 + c];
        sg = 1.f / (1.f + expf(-x));
    }
    if (m == 0) ref[q * 4 + c] = sg;
    const float a = sg * 6.283185307179586f;
    store_pair(pos + q * 512 + c * 128 + 2 * m, sinf(a / dim_t[2 * m]), cosf(a / dim_t[2 * m + 1]));
}

// ---------------------------------------------------------------------------------
// glue around the enc_output projection
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fill_rows_kernel(uint4* __restrict__ y, const uint8_t* __restrict__ keep,
                                                        const uint4* __restrict__ row, long rows, int cpr) {
    const long n = rows * cpr;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        const long r = t / cpr;
        if (!keep[r]) y[t] = row[t - r * cpr];
    }
}

__global__ __launch_bounds__(256) void boxes_kernel(const float4* __restrict__ tmp, const float4* __restrict__ prop,
                                                    float4* __restrict__ unact, float4* __restrict__ boxes, long rows) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < rows; t += (long)gridDim.x * blockDim.x) {
        const float4 a = tmp[t], p = prop[t];
        const float4 u = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
        unact[t] = u;
        boxes[t] = make_float4(1.f / (1.f + expf(-u.x)), 1.f / (1.f + expf(-u.y)), 1.f / (1.f + expf(-u.z)),
                               1.f / (1.f + expf(-u.w)));
    }
}

int stride_grid(long n) {
    long g = (n + 255) / 256;
    if (g > kMaxGridStride) g = kMaxGridStride;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace
}  // namespace kinet

using namespace kinet;

extern "C" int kinet_two_stage_proposals(const int* level_hw, int levels, const uint8_t* mask, float* proposals,
                                         uint8_t* keep, int B, int S, kinet_stream_t stream) {
    KINET_CHECK_ARG(level_hw && proposals && keep, "two_stage_proposals: null pointer");
    KINET_CHECK_ARG(levels >= 1 && levels <= KINET_TWO_STAGE_MAX_LEVELS, "two_stage_proposals: levels %d not in [1, %d]",
                    levels, KINET_TWO_STAGE_MAX_LEVELS);
    KINET_CHECK_ARG(B >= 0 && S > 0, "two_stage_proposals: bad sizes B %d S %d", B, S);
    KINET_CHECK_ARG((((uintptr_t)proposals) & 15) == 0, "two_stage_proposals: proposals must be 16-byte aligned");
    TsLevels lv;
    lv.n = levels;
    long off = 0;
    int max_hw = 0;
    for (int l = 0; l < levels; ++l) {
        const int h = level_hw[2 * l], w = level_hw[2 * l + 1];
        KINET_CHECK_ARG(h > 0 && w > 0 && (long)h * w <= S, "two_stage_proposals: bad level %d shape %d x %d", l, h, w);
        lv.h[l] = h;
        lv.w[l] = w;
        lv.off[l] = (int)off;
        off += (long)h * w;
        max_hw = std::max(max_hw, h * w);
    }
    KINET_CHECK_ARG(off == S, "two_stage_proposals: level shapes cover %ld tokens, S is %d", off, S);
    if (B == 0) return KINET_OK;
    KINET_CHECK_ARG(B <= 65535, "two_stage_proposals: B %d above 65535", B);
    const int chunks = std::min((max_hw + 255) / 256, 64);
    hipLaunchKernelGGL(proposals_kernel, dim3(chunks, levels, B), dim3(256), 0, (hipStream_t)stream, lv, mask, proposals,
                       keep, S);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_topk_rows(const float* scores, int64_t row_stride, int64_t elem_stride, int rows, int S, int k,
                               int64_t* out, kinet_stream_t stream) {
    KINET_CHECK_ARG(scores && out, "topk_rows: null pointer");
    KINET_CHECK_ARG(k >= 1 && k <= KINET_TOPK_MAX_K, "topk_rows: k %d not in [1, %d]", k, KINET_TOPK_MAX_K);
    KINET_CHECK_ARG(S >= k && S <= (1 << 30), "topk_rows: S %d must be in [k = %d, 2^30]", S, k);
    KINET_CHECK_ARG(rows >= 0 && elem_stride >= 1 && row_stride >= 0, "topk_rows: bad rows / strides");
    if (rows == 0) return KINET_OK;
    if (S <= TK_CACHE)
        hipLaunchKernelGGL(topk_rows_kernel<true>, dim3(rows), dim3(TK_THREADS), 0, (hipStream_t)stream, scores,
                           (long)row_stride, (long)elem_stride, S, k, out);
    else
        hipLaunchKernelGGL(topk_rows_kernel<false>, dim3(rows), dim3(TK_THREADS), 0, (hipStream_t)stream, scores,
                           (long)row_stride, (long)elem_stride, S, k, out);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_two_stage_queries(const float* coord_unact, const int64_t* idx, const float* dim_t, float* ref,
                                       void* pos, int B, int S, int k, int dtype, kinet_stream_t stream) {
    KINET_CHECK_ARG(coord_unact && idx && dim_t && ref && pos, "two_stage_queries: null pointer");
    KINET_CHECK_ARG(B >= 0 && S > 0 && k >= 1 && k <= KINET_TOPK_MAX_K && k <= S,
                    "two_stage_queries: bad sizes B %d S %d k %d (1 <= k <= %d, k <= S)", B, S, k, KINET_TOPK_MAX_K);
    KINET_CHECK_ARG(dtype == KINET_F32 || dtype == KINET_BF16 || dtype == KINET_F16,
                    "two_stage_queries: unsupported dtype %d", dtype);
    KINET_CHECK_ARG((((uintptr_t)pos) & 7) == 0, "two_stage_queries: pos must be 8-byte aligned");
    if (B == 0) return KINET_OK;
    const dim3 grid((unsigned)((long)B * k)), block(256);
    const hipStream_t s = (hipStream_t)stream;
    if (dtype == KINET_F32)
        hipLaunchKernelGGL(queries_kernel<float>, grid, block, 0, s, coord_unact, idx, dim_t, ref, (float*)pos, S, k);
    else if (dtype == KINET_BF16)
        hipLaunchKernelGGL(queries_kernel<bf16_t>, grid, block, 0, s, coord_unact, idx, dim_t, ref, (bf16_t*)pos, S, k);
    else
        hipLaunchKernelGGL(queries_kernel<f16_t>, grid, block, 0, s, coord_unact, idx, dim_t, ref, (f16_t*)pos, S, k);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_two_stage_fill_rows(void* y, const uint8_t* keep, const void* row, int64_t rows, int d, int dtype,
                                         kinet_stream_t stream) {
    KINET_CHECK_ARG(y && keep && row, "two_stage_fill_rows: null pointer");
    const size_t es = dtype == KINET_F32 || dtype == KINET_BF16 || dtype == KINET_F16 ? dtype_size(dtype) : 0;
    KINET_CHECK_ARG(es != 0, "two_stage_fill_rows: unsupported dtype %d", dtype);
    KINET_CHECK_ARG(rows >= 0 && d > 0 && ((size_t)d * es) % 16 == 0,
                    "two_stage_fill_rows: rows %ld, row bytes %ld must be a multiple of 16", (long)rows, (long)(d * es));
    KINET_CHECK_ARG((((uintptr_t)y | (uintptr_t)row) & 15) == 0, "two_stage_fill_rows: 16-byte aligned buffers required");
    if (rows == 0) return KINET_OK;
    const int cpr = (int)((size_t)d * es / 16);
    hipLaunchKernelGGL(fill_rows_kernel, dim3(stride_grid(rows * cpr)), dim3(256), 0, (hipStream_t)stream, (uint4*)y, keep,
                       (const uint4*)row, (long)rows, cpr);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int kinet_two_stage_boxes(const float* tmp, const float* proposals, float* coord_unact, float* boxes,
                                     int64_t rows, kinet_stream_t stream) {
    KINET_CHECK_ARG(tmp && proposals && coord_unact && boxes, "two_stage_boxes: null pointer");
    KINET_CHECK_ARG(rows >= 0, "two_stage_boxes: rows %ld", (long)rows);
    KINET_CHECK_ARG((((uintptr_t)tmp | (uintptr_t)proposals | (uintptr_t)coord_unact | (uintptr_t)boxes) & 15) == 0,
                    "two_stage_boxes: 16-byte aligned buffers required");
    if (rows == 0) return KINET_OK;
    hipLaunchKernelGGL(boxes_kernel, dim3(stride_grid(rows)), dim3(256), 0, (hipStream_t)stream, (const float4*)tmp,
                       (const float4*)proposals, (float4*)coord_unact, (float4*)boxes, (long)rows);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}
