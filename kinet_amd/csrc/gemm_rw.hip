// Resident-weight streaming GEMM for gfx950: C[M, N] = epilogue(A[M, K] @ W[N, K]^T) for
// large M and K <= 256 -- the deformable-encoder projections (value_proj, output_proj +
// residual + LayerNorm, FFN linear1, sampling offsets / attention logits) and the 1x1
// stride-1 convolutions of the ResNet body (NHWC activations are plain row-major GEMM
// operands).  DESIGN.md "Resident-weight GEMM".
//
// Why a second GEMM: with K = 256 the MFMA work per output byte is small and the tiled
// kernel (gemm.hip) spends its time re-loading W tiles and re-reading A once per N-tile
// through the CU load path.  Here
//  * a workgroup (4 waves) owns a column group of GW = 4*NT*16 output columns for the
//    whole launch; wave w keeps W rows [w*NT*16, (w+1)*NT*16) x K as MFMA A-fragments in
//    VGPRs (NT*KC*4 registers), loaded once;
//  * the workgroup walks row tiles of BMR rows (persistent: tile = blockIdx.x + i*gridDim.x);
//    each A tile (and the residual tile and the row-mask bytes) is staged into an NS-deep
//    LDS ring by LDS-DMA (buffer_load_dwordx4 ... lds, XOR swizzle on the source side,
//    hardware zero fill past the edges), issued NS-1 tiles ahead;  a counted
//    `s_waitcnt vmcnt` + raw s_barrier retires one tile per iteration, so the DMA of later
//    tiles stays in flight across the barrier (cdna_hip_programming.md §5 "Pipelining
//    across barriers");  no VGPR-destination global load appears in the loop, so hipcc
//    never drains the ring with a vmcnt(0) of its own;
//  * W rows are assigned to fragment rows so that every lane ends up holding NT*4
//    CONSECUTIVE output columns of one row: the epilogue (scale/bias, residual, ReLU,
//    LayerNorm across the 4 waves through a tiny LDS exchange, row mask, plain or
//    head-major store) runs straight from the accumulators with 16-byte stores;
//  * the packed outputs of tile i are stored after the barrier of iteration i+1, behind
//    the newest DMA, so outstanding stores never hold up the ring's counted wait.
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/kinet_gemm.h"
#include "../../include/kinet_msda.h"
#include "common.h"
#include "gemm_common.h"
#include "gemm_rw_plan.h"

namespace kinet {
namespace {

// The LDS geometry of an instantiation (rw_lds, gemm_rw_plan.h) as compile-time constants, plus the
// swizzles
template <int KC, int NT, int BMR, int NS, bool HAS_R, bool LN, bool HAS_A2, bool PREP = false, int NW = 4>
struct RwCfg {
    static constexpr RwLds G = rw_lds(RwVariant{KC, NT, BMR, NW, 0, HAS_R, LN, HAS_A2, false, PREP, 0}, NS);
    static constexpr int NTHR = G.NTHR, ROW = G.ROW, CPR = G.CPR, SWM = G.SWM, GW = G.GW;
    static constexpr int A_OPS = G.A_OPS, A_SPAN = G.A_SPAN;
    static constexpr int R_ROW = G.R_ROW, R_CPR = G.R_CPR, R_SWM = G.R_SWM, R_OPS = G.R_OPS, R_OFF = G.R_OFF;
    static constexpr int MASK_OFF = G.MASK_OFF, REF_OFF = G.REF_OFF, REF_OPS = G.REF_OPS, STAGE = G.STAGE;
    static constexpr int PAR = G.PAR, LNS = G.LNS, BYTES = G.BYTES, D = G.D;
    static constexpr bool POW2 = G.POW2, R_POW2 = G.R_POW2;
    // LDS position of 16-byte chunk c of tile row r (an involution: the DMA fills position c
    // with source chunk sw(r, c), a reader of logical chunk q reads position sw(r, q)).  Rows of
    // 36 chunks (K = 288, 576 B = 144 banks: rows r and r + 4 share banks) swap chunks within
    // aligned groups of 4 by (r >> 2) & 3, so 16 rows read at one chunk hit 16 distinct
    // 4-bank groups
    __device__ static constexpr int sw(int r, int c) { return POW2 ? c ^ (r & SWM) : c ^ ((r >> 2) & 3); }
    __device__ static constexpr int rsw(int r, int c) { return R_POW2 ? c ^ (r & R_SWM) : c ^ ((r >> 2) & 3); }
};

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// raw workgroup barrier for LDS traffic only: unlike __syncthreads() it does not drain the
// vector-memory counter, so LDS-DMA issued earlier stays in flight across it
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// the NW waves' partial sums of one row, in wave order
template <int NW>
__device__ __forceinline__ float wave_sum(const float* w) {
    if constexpr (NW == 4) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(w);
        return w4[0] + w4[1] + w4[2] + w4[3];
    } else {
        float s = w[0];
#pragma unroll
        for (int i = 1; i < NW; ++i) s += w[i];
        return s;
    }
}

template <typename TO> struct Pack;
template <> struct Pack<bf16_t> {
    static constexpr int WORDS_PER_4 = 2;
    __device__ static void put(uint32_t* w, const float* v) {
        w[0] = (uint32_t)f32_to_bf16(v[0]).x | ((uint32_t)f32_to_bf16(v[1]).x << 16);
        w[1] = (uint32_t)f32_to_bf16(v[2]).x | ((uint32_t)f32_to_bf16(v[3]).x << 16);
    }
};
template <> struct Pack<f16_t> {
    static constexpr int WORDS_PER_4 = 2;
    __device__ static void put(uint32_t* w, const float* v) {
        const f16_t a = (f16_t)v[0], b = (f16_t)v[1], c = (f16_t)v[2], d = (f16_t)v[3];
        w[0] = (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
        w[1] = (uint32_t)__builtin_bit_cast(uint16_t, c) | ((uint32_t)__builtin_bit_cast(uint16_t, d) << 16);
    }
};
template <> struct Pack<float> {
    static constexpr int WORDS_PER_4 = 4;
    __device__ static void put(uint32_t* w, const float* v) {
        for (int i = 0; i < 4; ++i) w[i] = __float_as_uint(v[i]);
    }
};

__device__ __forceinline__ void unpack8(const u32x4& u, float* v, bool f16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (f16) {
            v[2 * i] = (float)__builtin_bit_cast(f16_t, (uint16_t)(u[i] & 0xffffu));
            v[2 * i + 1] = (float)__builtin_bit_cast(f16_t, (uint16_t)(u[i] >> 16));
        } else {
            v[2 * i] = __uint_as_float(u[i] << 16);
            v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
        }
    }
}

// Sampling records of one (query, head, level) from the 12 projection outputs this lane holds
// (ms_deform_attn.py:69-82 + the bilinear setup of ms_deform_im2col_cuda.cuh:227-233):
//   v = [x0 y0 x1 y1 x2 y2 x3 y3 | logit0..3] of level l (offsets in level pixels, the head's
//   16 logits spread over the 4 lanes lane, lane^16, lane^32, lane^48 -- one per level);
// softmax over the head's 16 logits, the locations (the reference's offsets / (H, W) on (x, y)
// quirk for 2-d refs, :77-82), then per point, with h = y H - 0.5, w = x W - 0.5:
//   * the corner rows / columns outside the level folded into the weight by ONE factor per axis,
//     clamp(min(h + 1, H - h), 0, 1): 1 inside, lh = h + 1 when the top row is -1 (the footprint
//     becomes row 0 with weight a lh), 1 - lh = H - h when the bottom row is H (row H-1 keeps
//     a (1 - lh)), 0 outside the level (cuh:229) -- so the sampler needs no bounds tests (its
//     second row / column only ever gets weight 0); the same for columns;
//   * location = round(clamp(h, 0, H-1) 2^fb) << 16 | round(clamp(w, 0, W-1) 2^fb): the
//     fixed-point corner + fraction, (hl << (16+fb)) | (round(lh 2^fb) << 16) | (wl << fb) |
//     round(lw 2^fb) with a rounded-up fraction carried into the corner (h 2^fb + 0.5 is exact in
//     f32 for every level that fits the 16-bit field); a folded axis has fraction 0; a sample
//     outside the level (weight 0) points at the query's own pixel of the level, which the
//     sampler's strip always stages (finite values assumed: it multiplies that pixel by 0);
//   * weight = f16.
// out: 4 location words, then the 4 weights as 2 packed f16 words.
// max / sum over the 4 lanes lane ^ {0, 16, 32, 48} (the 4 levels of one row): gfx950's row-swap
// permutes (v_permlane16_swap / v_permlane32_swap) return {own, partner} in some order, so one
// op per step combines them -- no LDS round trip as __shfl_xor's ds_bpermute takes
template <bool MAX>
__device__ __forceinline__ float level_reduce(float x) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = MAX ? fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1])) : __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return MAX ? fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1])) : __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// r: the (query, level) reference point (x, y[, w, h]), qmasked: the query's mask byte, both read
// from the tile's LDS stage by the caller
__device__ __forceinline__ void prep_records(const GemmArgs& p, const float4 r, bool qmasked, int Hl, int Wl,
                                             const float (&v)[12], uint32_t* out) {
    const float Hf = (float)Hl, Wf = (float)Wl;
    const float fs = (float)(1 << p.prep_fb);
    const float mx = level_reduce<true>(fmaxf(fmaxf(v[8], v[9]), fmaxf(v[10], v[11])));
    float e[4], es = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        e[q] = __expf(v[8 + q] - mx);
        es += e[q];
    }
    es = level_reduce<false>(es);
    const float ra = qmasked ? 0.f : __builtin_amdgcn_rcpf(es);
    float rx, ry, sx, sy;   // reference point and the offset scale of each axis
    if (p.prep_refd == 2) {
        rx = r.x;
        ry = r.y;
        sx = __builtin_amdgcn_rcpf(Hf);   // :77-79 (offsets / spatial_shapes, (H, W) on (x, y))
        sy = __builtin_amdgcn_rcpf(Wf);
    } else {
        rx = r.x;
        ry = r.y;
        sx = 0.125f * r.z;   // :80-82 (/ n_points * wh * 0.5, n_points = 4)
        sy = 0.125f * r.w;
    }
    const float H1 = Hf - 1.f, W1 = Wf - 1.f;
    // the query's own pixel of this level: where a sample outside the level points (weight 0)
    const int hr = min(max((int)floorf(ry * Hf), 0), Hl - 1), wr = min(max((int)floorf(rx * Wf), 0), Wl - 1);
    const uint32_t own = ((uint32_t)hr << (16 + p.prep_fb)) | ((uint32_t)wr << p.prep_fb);
    float aw[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float x = fmaf(v[2 * q], sx, rx), y = fmaf(v[2 * q + 1], sy, ry);
        const float h = fmaf(y, Hf, -0.5f), w = fmaf(x, Wf, -0.5f);
        const float fh = __builtin_amdgcn_fmed3f(fminf(h + 1.f, Hf - h), 0.f, 1.f);
        const float fw = __builtin_amdgcn_fmed3f(fminf(w + 1.f, Wf - w), 0.f, 1.f);
        aw[q] = e[q] * ra * fh * fw;
        const uint32_t ph = (uint32_t)(int)fmaf(__builtin_amdgcn_fmed3f(h, 0.f, H1), fs, 0.5f);
        const uint32_t pw = (uint32_t)(int)fmaf(__builtin_amdgcn_fmed3f(w, 0.f, W1), fs, 0.5f);
        out[q] = fminf(fh, fw) > 0.f ? (ph << 16) | pw : own;   // fh, fw > 0: inside (-1, H) x (-1, W)
    }
    out[4] = (uint32_t)__builtin_bit_cast(uint16_t, (f16_t)aw[0]) | ((uint32_t)__builtin_bit_cast(uint16_t, (f16_t)aw[1]) << 16);
    out[5] = (uint32_t)__builtin_bit_cast(uint16_t, (f16_t)aw[2]) | ((uint32_t)__builtin_bit_cast(uint16_t, (f16_t)aw[3]) << 16);
}

// CR (conv-row mode): A row m is output pixel (img, oh, ow) of a KH x 1, horizontally
// stride-1 unpadded NHWC convolution (the tap-folded ResNet stem, ops.hip
// pack_image_kwfold_kernel): K = KH*Cin, logical chunk q of the row = 8 channels of tap
// kh = q / (Cin/8) read from input row oh*stride - pad + kh (zeros outside the image and past K)
template <typename T, typename TO, int KC, int NT, int BMR, int NS, bool HAS_R, bool LN, bool HAS_A2, bool CR,
          bool PREP = false, int OCC = 2, int NW = 4>
__global__ __launch_bounds__(NW * 64, OCC) void gemm_rw_kernel(const GemmArgs p, const int n_mtiles) {
    using C_ = RwCfg<KC, NT, BMR, NS, HAS_R, LN, HAS_A2, PREP, NW>;
    constexpr int NTHR = C_::NTHR;
    constexpr int TMR = BMR / 16;             // 16-row MFMA tiles per row tile
    constexpr int GW = C_::GW;
    constexpr int NC = NT * 4;                // consecutive columns per lane
    constexpr int PW = NC / 4 * Pack<TO>::WORDS_PER_4;   // packed 32-bit words per lane-row
    constexpr unsigned OOB = 0x80000000u;
    __shared__ __attribute__((aligned(16))) char lds[C_::BYTES];
    float* par = reinterpret_cast<float*>(lds);
    float* lns = reinterpret_cast<float*>(lds + C_::PAR);
    char* stages = lds + C_::PAR + C_::LNS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int P = gridDim.x, bx = blockIdx.x;
    const int ncol0 = blockIdx.y * GW;
    const int M = p.M, N = p.N;
    const int cnt = bx < n_mtiles ? (n_mtiles - 1 - bx) / P + 1 : 0;

    for (int i = tid; i < GW; i += NTHR) {
        const int n = ncol0 + i;
        const bool ok = n < N;
        par[i] = (ok && p.scale) ? p.scale[n] : 1.f;
        par[GW + i] = (ok && p.bias) ? p.bias[n] : 0.f;
        par[2 * GW + i] = (LN && ok) ? p.ln_g[n] : 0.f;
        par[3 * GW + i] = (LN && ok) ? p.ln_b[n] : 0.f;
    }

    // this wave's W slice as MFMA A-fragments: fragment row i of n-tile a is output column
    // ncol0 + wave*NC*4 + (i>>2)*NC + a*4 + (i&3), so lane group g = lane>>4 of the result
    // holds columns [g*NC, g*NC + NC) of the wave's range -- NC consecutive columns
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, (short)0, p.b_bytes, 0x00020000);
    u32x4 wf[NT][KC];
    {
        const int i = lane & 15;
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const int n = ncol0 + wave * NC * 4 + (i >> 2) * NC + a * 4 + (i & 3);
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int k = c * 32 + (lane >> 4) * 8;
                const unsigned off = (n < N && k < p.K) ? ((unsigned)n * (unsigned)p.ldb + (unsigned)k) * 2u : OOB;
                wf[a][c] = __builtin_amdgcn_raw_buffer_load_b128(rb, off, 0, 0);
            }
        }
    }

    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, (short)0, p.a_bytes, 0x00020000);
    const int a2_bytes = (HAS_A2 && p.a2_rows) ? ((p.a2_rows - 1) * p.lda + p.K) * 2 : p.a_bytes;
    const __amdgpu_buffer_rsrc_t ra2 =
        __builtin_amdgcn_make_buffer_rsrc((void*)(HAS_A2 ? p.A2 : p.A), (short)0, a2_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr =
        __builtin_amdgcn_make_buffer_rsrc((void*)(HAS_R ? p.R : p.A), (short)0, HAS_R ? p.r_bytes : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rm =
        __builtin_amdgcn_make_buffer_rsrc((void*)(p.row_mask ? (const void*)p.row_mask : p.A), (short)0,
                                          p.row_mask ? M : 0, 0x00020000);
    // The row mask of the last partial group of 16 rows (M % 16 != 0), as 16 wave-uniform bits read once
    // by byte loads: the tile DMA below moves the mask 16 bytes at a time, and in the group that straddles
    // the end of the M-byte mask the dword holding the last M % 4 bytes is out of range and reads 0
    // (masked rows among the last M % 4 were stored unmasked).  Bytes past M, and a NULL mask (an empty
    // descriptor), read 0
    const int mtail0 = M & ~15;
    const unsigned tailbits =
        (unsigned)__ballot(__builtin_amdgcn_raw_buffer_load_b8(rm, (unsigned)(mtail0 + (lane & 15)), 0, 0) != 0) & 0xffffu;
    const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(PREP ? (const void*)p.prep_ref : p.A), (short)0, PREP ? M * 16 * p.prep_refd : 0, 0x00020000);

    // per-thread DMA offsets, split into a scalar tile base (m0 * ld) and lane constants
    unsigned a_lo[C_::A_OPS];
    int a_row[C_::A_OPS];
    int cr_kh[C_::A_OPS];
#pragma unroll
    for (int j = 0; j < C_::A_OPS; ++j) {
        const int idx = j * NTHR + tid;
        const int row = idx / C_::CPR, s = idx % C_::CPR;
        a_row[j] = row < BMR ? row : (1 << 30);   // round padding: never in range
        a_lo[j] = ((unsigned)row * (unsigned)p.lda + (unsigned)(C_::sw(row, s) * 8)) * 2u;
        cr_kh[j] = 0;
        if (CR) {
            // tap and in-tap channel offset of logical chunk q (lane constants); chunks past K
            // get a tap index that never lands inside the image
            const int q = C_::sw(row, s), cpt = p.Cin >> 3;
            const int kh = q / cpt;
            cr_kh[j] = q * 8 < p.K ? kh : (1 << 28);
            a_lo[j] = (unsigned)((q - kh * cpt) * 8);
        }
    }
    unsigned r_lo[C_::R_OPS > 0 ? C_::R_OPS : 1];
    int r_row[C_::R_OPS > 0 ? C_::R_OPS : 1];
#pragma unroll
    for (int j = 0; j < C_::R_OPS; ++j) {
        const int idx = j * NTHR + tid;
        const int row = idx / C_::R_CPR, s = idx % C_::R_CPR;
        const int n = ncol0 + C_::rsw(row, s) * 8;
        r_row[j] = (n < N && row < BMR) ? row : (1 << 30);   // columns past N, round padding: never in range
        r_lo[j] = ((unsigned)row * (unsigned)p.ldr + (unsigned)n) * 2u;
    }
    auto issue = [&](int i) {
        const int m0 = (bx + i * P) * BMR;
        char* st = stages + (i % NS) * C_::STAGE;
        const unsigned abase = (unsigned)m0 * (unsigned)p.lda * 2u;
        // conv-row mode: the tile's first pixel on the scalar unit, then row r of the tile is
        // that pixel + r with at most one carry into the next output row (host: Wout >= BMR)
        const int hw = p.Hout * p.Wout;
        const int img0 = CR ? m0 / hw : 0;
        const int oh0 = CR ? (m0 - img0 * hw) / p.Wout : 0;
        const int ow0 = CR ? m0 - img0 * hw - oh0 * p.Wout : 0;
        // A2 of a2_rows rows (row m reads row m % a2_rows): the tile's rows sit in period q0 up
        // to tile row a2_bnd, in q0 + 1 after it (host: a2_rows >= BMR, so at most one wrap)
        unsigned a2_sub = 0u, a2_sub1 = 0u;
        int a2_bnd = 1 << 30;
        if (HAS_A2 && p.a2_rows) {
            const int q0 = m0 / p.a2_rows;
            a2_sub = (unsigned)(q0 * p.a2_rows) * (unsigned)p.lda * 2u;
            a2_sub1 = a2_sub + (unsigned)p.a2_rows * (unsigned)p.lda * 2u;
            a2_bnd = (q0 + 1) * p.a2_rows - m0;
        }
#pragma unroll
        for (int j = 0; j < C_::A_OPS; ++j) {
            unsigned off = m0 + a_row[j] < M ? abase + a_lo[j] : OOB;
            if (CR) {
                int ow = ow0 + a_row[j], oh = oh0, img = img0;
                const bool c1 = ow >= p.Wout;
                ow = c1 ? ow - p.Wout : ow;
                oh = c1 ? oh + 1 : oh;
                const bool c2 = oh >= p.Hout;
                oh = c2 ? 0 : oh;
                img = c2 ? img + 1 : img;
                const int ih = oh * p.stride - p.pad + cr_kh[j];
                const bool ok = m0 + a_row[j] < M && (unsigned)ih < (unsigned)p.Hin;
                off = ok ? ((unsigned)((img * p.Hin + ih) * p.Win + ow * p.stride_w) * (unsigned)p.Cin + a_lo[j]) * 2u : OOB;
            }
            dma16(ra, st + (j * NTHR + wave * 64) * 16, off);
            if (HAS_A2)
                dma16(ra2, st + C_::A_SPAN + (j * NTHR + wave * 64) * 16,
                      off == OOB ? OOB : off - (a_row[j] >= a2_bnd ? a2_sub1 : a2_sub));
        }
        const unsigned rbase = (unsigned)m0 * (unsigned)p.ldr * 2u;
#pragma unroll
        for (int j = 0; j < C_::R_OPS; ++j) {
            const unsigned off = m0 + r_row[j] < M ? rbase + r_lo[j] : OOB;
            dma16(rr, st + C_::R_OFF + (j * NTHR + wave * 64) * 16, off);
        }
        // row-mask bytes m0 .. m0+BMR (every wave writes the same 1 KiB).  A 16-byte access that
        // straddles the end of the M-byte mask reads 0 in its last dword: the rows of the last partial
        // group of 16 get their mask bytes from tailbits once the tile has landed (main loop)
        dma16(rm, st + C_::MASK_OFF, lane < TMR ? (unsigned)(m0 + lane * 16) : OOB);
        // PREP: the tile's reference points, BMR rows x 4 levels x prep_refd f32 (<= 1 KiB; every
        // wave writes the same bytes, rows past M read 0)
        if constexpr (PREP) {
            const unsigned rbytes = (unsigned)(BMR * 16 * p.prep_refd);
#pragma unroll
            for (int j = 0; j < C_::REF_OPS; ++j) {
                const unsigned o = (unsigned)(j * 1024 + lane * 16);
                dma16(rf, st + C_::REF_OFF + j * 1024, o < rbytes ? (unsigned)m0 * 16u * (unsigned)p.prep_refd + o : OOB);
            }
        }
    };

    __syncthreads();   // parameters visible; no DMA in flight yet
#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
        if (s < cnt) issue(s);

    const int cl0 = wave * NC * 4 + (lane >> 4) * NC;   // this lane's first column in the group
    // PREP: this lane's level (lane >> 4, fixed for the launch) and its shape, selected once and
    // pinned in VGPRs.  Selected inside the loop, the compiler turned the select chain into an
    // indexed load from the kernel-argument segment, and that load's s_waitcnt vmcnt(0) before
    // the epilogue also waited for the DMA of the next row tile: the ring's prefetch was exposed
    // once per tile
    int lvl_H = 0, lvl_W = 0;
    if constexpr (PREP) {
        const int l = lane >> 4;
        lvl_H = l == 0 ? p.prep_H[0] : l == 1 ? p.prep_H[1] : l == 2 ? p.prep_H[2] : p.prep_H[3];
        lvl_W = l == 0 ? p.prep_W[0] : l == 1 ? p.prep_W[1] : l == 2 ? p.prep_W[2] : p.prep_W[3];
        asm volatile("" : "+v"(lvl_H), "+v"(lvl_W));
    }
    uint32_t pend[TMR][PW] = {};
    int pend_m0 = 0;
    // packed outputs of one row tile: ALWAYS S buffer stores per lane (offsets past the
    // descriptor for rows / columns outside C and for the dummy call of iteration 0), so the
    // counted waits below know exactly how many vector-memory ops are younger than a DMA
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(p.C, (short)0, p.c_bytes, 0x00020000);
    constexpr int EPC16 = 16 / (int)sizeof(TO);     // elements per 16-byte store
    // store unit: 16 bytes, or 4 columns when a lane's NC columns are not whole 16-byte runs
    // (NT = 3: 12 columns = 16-bit 8-byte units, never straddling a head of 4k columns; the
    // 9-wave K = 288 groups without LayerNorm store 4-column units too: head-major d = 36)
    constexpr int SU = (NC % EPC16 == 0 && !(KC == 9 && NT == 2 && !LN)) ? EPC16 : 4;
    constexpr int NU = NC / SU;                     // store units per lane-row
    constexpr int WPU = SU * (int)sizeof(TO) / 4;   // packed words per unit
    // stores per lane per row tile (PREP: one 16-byte location store + one 8-byte weight store)
    constexpr int S = TMR * (PREP ? 2 : NU);
    static_assert(NS >= 2 && NS <= 4 && (NS - 2) * (C_::D + S) <= 63, "ring depth / vmcnt range");
    // element offset of (row m, column n): m * rs + colpart(n); head-major (hm_rows > 0):
    // ((g*hm_batch + b)*hm_rows + s)*hm_d + d = g*M*hm_d + m*hm_d + d for m = b*hm_rows + s;
    // split head-major (hm_split > 0): columns n >= hm_split in the second plane at
    // hm_split*M elements, row stride hm_d2 (one 4-column unit per head)
    const int rs = PREP ? 96 / (int)sizeof(TO) : (p.hm_rows ? p.hm_d : p.ldc);
    constexpr int NSL = PREP ? 2 : NU;
    unsigned s_lo[TMR][NSL];
    unsigned s_rs[NSL];
    bool s_nok[NSL];
    if constexpr (PREP) {
        // record (head h, row m) at (h*M + m)*96 bytes: [4 levels x 16 B locations | 4 levels x 8 B weights];
        // this lane writes level lane >> 4 of head blockIdx.y*NW + wave
        const unsigned hb = (unsigned)(blockIdx.y * NW + wave) * (unsigned)M;
        const unsigned l = (unsigned)(lane >> 4);
#pragma unroll
        for (int t = 0; t < TMR; ++t) {
            const unsigned r = (hb + (unsigned)(t * 16 + (lane & 15))) * 96u;
            s_lo[t][0] = r + l * 16u;
            s_lo[t][1] = r + 64u + l * 8u;
        }
        s_nok[0] = s_nok[1] = false;
        s_rs[0] = s_rs[1] = (unsigned)rs;
    }
#pragma unroll
    for (int h = 0; h < (PREP ? 0 : NU); ++h) {
        const int n = ncol0 + cl0 + h * SU;
        s_nok[h] = n >= N;
        unsigned colpart = (unsigned)n, r_s = (unsigned)rs;
        if (p.hm_rows) {
            if (p.hm_split && n >= p.hm_split) {
                const int n2 = n - p.hm_split, g = n2 / p.hm_d2;
                colpart = (unsigned)p.hm_split * (unsigned)M + (unsigned)g * (unsigned)M * (unsigned)p.hm_d2 +
                          (unsigned)(n2 - g * p.hm_d2);
                r_s = (unsigned)p.hm_d2;
            } else {
                const int g = n / p.hm_d;
                colpart = (unsigned)g * (unsigned)M * (unsigned)p.hm_d + (unsigned)(n - g * p.hm_d);
            }
        }
        s_rs[h] = r_s;
#pragma unroll
        for (int t = 0; t < TMR; ++t)
            s_lo[t][h] = ((unsigned)(t * 16 + (lane & 15)) * r_s + colpart) * (unsigned)sizeof(TO);
    }
    // head-major outputs of 32-column heads (the d = 256 value projections): each wave's 16 x 64
    // output block is 2 heads; transposed through LDS (the pending tile's ring slot, free after the
    // tile's barrier until the next DMA is issued into it) so each store instruction writes one
    // head plane's 16 rows x 64 B = 1 KiB contiguous instead of 8-byte pieces 64 B apart
    constexpr bool HM32_OK = !PREP && !LN && sizeof(TO) == 2 && NC == 16 && WPU == 4 && TMR * 2048 * NW <= C_::STAGE;
    const bool hm32 = HM32_OK && p.hm_tr && p.hm_rows && p.hm_d == 32 && !p.hm_split && N % 64 == 0;
    int pend_slot = 0;
    auto store_pending = [&](bool valid) {
        if constexpr (HM32_OK) {
            // (iteration 0, nothing pending: the S dummy stores below -- the counted waits take them for
            // granted on this path too -- and pend_slot may be the slot about to be computed)
            if (hm32 && valid) {
                char* scr = stages + pend_slot * C_::STAGE + wave * (TMR * 2048);
                const int g = lane >> 4, r = lane & 15;
#pragma unroll
                for (int t = 0; t < TMR; ++t) {
                    char* b = scr + t * 2048 + (g >> 1) * 1024 + r * 64 + (g & 1) * 32;
                    *reinterpret_cast<u32x4*>(b) = u32x4{pend[t][0], pend[t][1], pend[t][2], pend[t][3]};
                    *reinterpret_cast<u32x4*>(b + 16) = u32x4{pend[t][4], pend[t][5], pend[t][6], pend[t][7]};
                }
                const int hg0 = (ncol0 + wave * 64) >> 5;
                const bool wok = ncol0 + wave * 64 < N;
#pragma unroll
                for (int t = 0; t < TMR; ++t)
#pragma unroll
                    for (int hl = 0; hl < 2; ++hl) {
                        const u32x4 w = *reinterpret_cast<const u32x4*>(scr + t * 2048 + hl * 1024 + lane * 16);
                        const int row = pend_m0 + t * 16 + (lane >> 2);
                        const unsigned off = (wok && row < M) ? (((unsigned)(hg0 + hl) * (unsigned)M + (unsigned)row) * 32u +
                                                                 (unsigned)(lane & 3) * 8u) * 2u
                                                              : OOB;
                        __builtin_amdgcn_raw_buffer_store_b128(w, rc, off, 0, 0);
                    }
                return;
            }
        }
        if constexpr (PREP) {
            const unsigned base = (unsigned)pend_m0 * (unsigned)rs * (unsigned)sizeof(TO);
#pragma unroll
            for (int t = 0; t < TMR; ++t) {
                const bool mok = valid && pend_m0 + t * 16 + (lane & 15) < M;
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{pend[t][0], pend[t][1], pend[t][2], pend[t][3]}, rc,
                                                       mok ? base + s_lo[t][0] : OOB, 0, 0);
                typedef uint32_t u32x2_ __attribute__((ext_vector_type(2)));
                __builtin_amdgcn_raw_buffer_store_b64(u32x2_{pend[t][4], pend[t][5]}, rc, mok ? base + s_lo[t][1] : OOB,
                                                      0, 0);
            }
            return;
        }
#pragma unroll
        for (int t = 0; t < TMR; ++t) {
            const bool mok = valid && pend_m0 + t * 16 + (lane & 15) < M;
#pragma unroll
            for (int h = 0; h < NU; ++h) {
                const unsigned base = (unsigned)pend_m0 * s_rs[h] * (unsigned)sizeof(TO);
                const unsigned off = (mok && !s_nok[h]) ? base + s_lo[t][h] : OOB;
                if constexpr (WPU == 4) {
                    __builtin_amdgcn_raw_buffer_store_b128(
                        u32x4{pend[t][4 * h], pend[t][4 * h + 1], pend[t][4 * h + 2], pend[t][4 * h + 3]}, rc, off, 0, 0);
                } else {
                    typedef uint32_t u32x2_ __attribute__((ext_vector_type(2)));
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2_{pend[t][2 * h], pend[t][2 * h + 1]}, rc, off, 0, 0);
                }
            }
        }
    };

    for (int i = 0; i < cnt; ++i) {
        // retire tile i's DMA.  Younger vector-memory ops: the DMA of the (NS-2) later tiles
        // (D each) and the stores (S each) of the min(i, NS-2) iterations issued after it
        if (i + NS - 2 >= cnt) wait_vmcnt<0>();
        else if (NS <= 2 || i >= NS - 2) wait_vmcnt<(NS - 2) * (C_::D + S)>();
        else if (i == 0) wait_vmcnt<(NS - 2) * C_::D>();
        else wait_vmcnt<(NS - 2) * C_::D + S>();   // i == 1 (NS == 4)
        if (HAS_A2) {
            // q = src + pos rounded to the operand type, exactly as gemm.hip's load-time add:
            // each thread sums the chunks its own DMA delivered (landed: the wait above), once
            // per tile instead of once per wave; the barrier publishes the sums
            char* st = stages + (i % NS) * C_::STAGE;
#pragma unroll
            for (int j = 0; j < C_::A_OPS; ++j) {
                u32x4* pa = reinterpret_cast<u32x4*>(st + (j * NTHR + tid) * 16);
                *pa = Mma<T>::add(*pa, *reinterpret_cast<const u32x4*>(st + C_::A_SPAN + (j * NTHR + tid) * 16));
            }
        }
        lds_barrier();
        // the row tile that holds the last partial group of 16 rows (once per launch, and only with
        // M % 16 != 0): its mask bytes come from tailbits.  After the barrier every wave's copy of
        // the tile's mask DMA has landed; every wave writes the same 16 bytes and reads them back
        // itself, so no second barrier is needed
        if ((bx + i * P) * BMR + BMR > mtail0 && mtail0 < M) {
            char* mk = stages + (i % NS) * C_::STAGE + C_::MASK_OFF + (mtail0 - (bx + i * P) * BMR);
            if (lane < 16) mk[lane] = (char)((tailbits >> lane) & 1u);
        }
        // PREP: the tile's mask bytes and reference points read BEFORE the next tile's DMA is
        // issued: an LDS read after it gets an s_waitcnt vmcnt(0) from the compiler (it cannot
        // prove the DMA's stage disjoint), which would wait for that DMA before the epilogue
        float4 pref[PREP ? TMR : 1];
        bool pmask[PREP ? TMR : 1];
        if constexpr (PREP) {
            const char* sc = stages + (i % NS) * C_::STAGE;
#pragma unroll
            for (int t = 0; t < TMR; ++t) {
                const int rl = t * 16 + (lane & 15), l = lane >> 4;
                pmask[t] = sc[C_::MASK_OFF + rl] != 0;
                pref[t] = *reinterpret_cast<const float4*>(sc + C_::REF_OFF + (rl * 4 + l) * (p.prep_refd == 2 ? 8 : 16));
            }
        }
        // the counted waits above take S stores per iteration for granted, the dummy ones of
        // iteration 0 included.  Seen as a constant false (an iteration 0 that the optimiser peeled
        // off), their S equal stores of zeros to one offset fold into one; an opaque copy of i keeps
        // every iteration's stores S instructions
        int it = i;
        asm volatile("" : "+s"(it));
        store_pending(it > 0);
        if (hm32) lds_barrier();   // every wave done with its transpose scratch (the slot refilled below)
        if (i + NS - 1 < cnt) issue(i + NS - 1);

        const char* st = stages + (i % NS) * C_::STAGE;
        const int m0 = (bx + i * P) * BMR;
        f32x4 acc[NT][TMR];
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int t = 0; t < TMR; ++t) {
                // PREP: the accumulators start at the bias (one LDS read per 4 columns instead of
                // an add per column after the K loop)
                if constexpr (PREP) acc[a][t] = *reinterpret_cast<const f32x4*>(par + GW + cl0 + a * 4);
                else acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
        for (int c = 0; c < KC; ++c)
#pragma unroll
            for (int t = 0; t < TMR; ++t) {
                const int row = t * 16 + (lane & 15);
                const int q = c * 4 + (lane >> 4);
                const int xo = row * C_::ROW + (C_::sw(row, q) << 4);
                const u32x4 xf = *reinterpret_cast<const u32x4*>(st + xo);
#pragma unroll
                for (int a = 0; a < NT; ++a) Mma<T>::run(acc[a][t], wf[a][c], xf);
            }

        // ---- epilogue (registers) ----
        float v[TMR][NC];
        if constexpr (PREP) {
#pragma unroll
            for (int t = 0; t < TMR; ++t) {
#pragma unroll
                for (int j = 0; j < NC; ++j) v[t][j] = acc[j >> 2][t][j & 3];
                prep_records(p, pref[t], pmask[t], lvl_H, lvl_W, v[t], pend[t]);
            }
            pend_m0 = m0;
            continue;
        }
#pragma unroll
        for (int t = 0; t < TMR; ++t) {
            const int rl = t * 16 + (lane & 15);
#pragma unroll
            for (int j = 0; j < NC; ++j)
                v[t][j] = acc[j >> 2][t][j & 3] * par[cl0 + j] + par[GW + cl0 + j];
            if constexpr (HAS_R && NC % 8 == 0) {
#pragma unroll
                for (int h = 0; h < NC / 8; ++h) {
                    const int q = (cl0 >> 3) + h;
                    const u32x4 u = *reinterpret_cast<const u32x4*>(st + C_::R_OFF + rl * C_::R_ROW +
                                                                    (C_::rsw(rl, q) << 4));
                    float r8[8];
                    unpack8(u, r8, std::is_same<TO, f16_t>::value);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[t][h * 8 + e] += r8[e];
                }
            } else if constexpr (HAS_R) {
                // 4-column pieces (NT = 3: a lane's 12 columns start at a multiple of 4)
#pragma unroll
                for (int h = 0; h < NC / 4; ++h) {
                    const int col = cl0 + 4 * h, q = col >> 3;
                    const uint2 u = *reinterpret_cast<const uint2*>(st + C_::R_OFF + rl * C_::R_ROW +
                                                                    (C_::rsw(rl, q) << 4) + ((col >> 2) & 1) * 8);
                    float r8[8];
                    unpack8(u32x4{u.x, u.y, 0u, 0u}, r8, std::is_same<TO, f16_t>::value);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[t][h * 4 + e] += r8[e];
                }
            }
            if (p.relu)
#pragma unroll
                for (int j = 0; j < NC; ++j) v[t][j] = fmaxf(v[t][j], 0.f);
        }
        if (LN) {
            // columns past N are exactly 0 here (zero W rows, zero bias, zero residual)
            float mean[TMR], rstd[TMR];
#pragma unroll
            for (int t = 0; t < TMR; ++t) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < NC; ++j) s += v[t][j];
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                if ((lane >> 4) == 0) lns[(t * 16 + (lane & 15)) * NW + wave] = s;
            }
            lds_barrier();
#pragma unroll
            for (int t = 0; t < TMR; ++t) {
                mean[t] = wave_sum<NW>(lns + (t * 16 + (lane & 15)) * NW) / (float)N;
                float q = 0.f;
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    const float d = (ncol0 + cl0 + j < N) ? v[t][j] - mean[t] : 0.f;
                    q += d * d;
                }
                q += __shfl_xor(q, 16);
                q += __shfl_xor(q, 32);
                if ((lane >> 4) == 0) lns[BMR * NW + (t * 16 + (lane & 15)) * NW + wave] = q;
            }
            lds_barrier();
#pragma unroll
            for (int t = 0; t < TMR; ++t) {
                rstd[t] = rsqrtf(wave_sum<NW>(lns + BMR * NW + (t * 16 + (lane & 15)) * NW) / (float)N + p.ln_eps);
#pragma unroll
                for (int j = 0; j < NC; ++j)
                    v[t][j] = (v[t][j] - mean[t]) * rstd[t] * par[2 * GW + cl0 + j] + par[3 * GW + cl0 + j];
            }
        }
#pragma unroll
        for (int t = 0; t < TMR; ++t) {
            const int rl = t * 16 + (lane & 15);
            if (st[C_::MASK_OFF + rl])
#pragma unroll
                for (int j = 0; j < NC; ++j) v[t][j] = 0.f;
#pragma unroll
            for (int j4 = 0; j4 < NC / 4; ++j4) Pack<TO>::put(&pend[t][j4 * Pack<TO>::WORDS_PER_4], &v[t][j4 * 4]);
        }
        pend_m0 = m0;
        pend_slot = i % NS;
    }
    if (cnt > 0) {
        if (hm32) lds_barrier();   // the last tile's slot: every wave done reading it
        store_pending(true);
    }
}

}  // namespace

thread_local int rw_last_cfg[RW_CFG_FIELDS] = {};   // declared in gemm_common.h
thread_local int rw_grid_cap = 0;                   // kinet_gemm_rw_grid_cap (0 = no cap)

namespace {

template <typename T, typename TO>
constexpr int type_pair = sizeof(TO) == 4 ? (std::is_same<T, bf16_t>::value ? RWT_BF16_F32 : RWT_F16_F32)
                          : std::is_same<T, TO>::value ? (std::is_same<T, bf16_t>::value ? RWT_BF16_BF16 : RWT_F16_F16)
                                                       : RWT_BF16_F16;

// Launch entry I of kRwVariants (gemm_rw_plan.h) for one type pair if `variant` names it.  These are
// the only launches of gemm_rw_kernel, so the table is the list of its instantiations.
template <typename T, typename TO, int I>
void launch_entry(int variant, dim3 grid, hipStream_t stream, const GemmArgs& a, int n_mtiles) {
    constexpr RwVariant v = kRwVariants[I];
    if constexpr ((v.types & type_pair<T, TO>) != 0) {
        if (variant != I) return;
        hipLaunchKernelGGL((gemm_rw_kernel<T, TO, v.kc, v.nt, v.bmr, rw_ring_depth(v), v.has_r, v.ln, v.has_a2, v.cr, v.prep,
                                           v.occ, v.nw>),
                           grid, dim3(v.threads()), 0, stream, a, n_mtiles);
    }
}
template <typename T, typename TO, int... I>
void launch_variant(int variant, dim3 grid, hipStream_t stream, const GemmArgs& a, int n_mtiles,
                    std::integer_sequence<int, I...>) {
    (launch_entry<T, TO, I>(variant, grid, stream, a, n_mtiles), ...);
}

// Plan the problem (gemm_rw_plan.h: every eligibility rule and variant heuristic lives there) and
// run the planned launch: kernel, block, grid and the record all come from its one table entry.
// false = not eligible, nothing launched.
bool launch_planned(RwProblem p, const GemmArgs& a, hipStream_t stream) {
    p.flags = kinet_gemm_flags;
    p.cap = rw_grid_cap;
    p.cus = cu_count();
    RwPlan plan;
    if (!rw_plan(p, plan)) return false;
    GemmArgs ac = a;
    ac.c_bytes = plan.c_bytes;
    ac.hm_tr = plan.hm_tr;
    rw_config_record(plan, p.out_dtype, rw_last_cfg);
    const dim3 grid(plan.P, plan.ng);
    constexpr std::make_integer_sequence<int, kNumRwVariants> all{};
    switch (rw_type_pair(p.in_dtype, p.out_dtype)) {   // (one of these: rw_plan checked the entry's mask)
    case RWT_BF16_BF16: launch_variant<bf16_t, bf16_t>(plan.variant, grid, stream, ac, plan.n_mtiles, all); break;
    case RWT_BF16_F16: launch_variant<bf16_t, f16_t>(plan.variant, grid, stream, ac, plan.n_mtiles, all); break;
    case RWT_BF16_F32: launch_variant<bf16_t, float>(plan.variant, grid, stream, ac, plan.n_mtiles, all); break;
    case RWT_F16_F16: launch_variant<f16_t, f16_t>(plan.variant, grid, stream, ac, plan.n_mtiles, all); break;
    case RWT_F16_F32: launch_variant<f16_t, float>(plan.variant, grid, stream, ac, plan.n_mtiles, all); break;
    }
    return true;
}

bool al16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// the fields of a problem that its GemmArgs carry
RwProblem rw_problem(int kind, const GemmArgs& a, int in_dtype, int out_dtype) {
    RwProblem p{};
    p.kind = kind;
    p.M = a.M; p.N = a.N; p.K = a.K;
    p.in_dtype = in_dtype; p.out_dtype = out_dtype;
    p.r = a.R != nullptr; p.ln = a.ln_g != nullptr; p.a2 = a.A2 != nullptr;
    p.ldc = a.ldc; p.ldr = a.ldr;
    p.c_al16 = al16(a.C); p.r_al16 = al16(a.R); p.a2_al16 = al16(a.A2);
    p.hm_rows = a.hm_rows; p.hm_d = a.hm_d; p.hm_split = a.hm_split; p.hm_d2 = a.hm_d2;
    p.Cin = a.Cin; p.KW = a.KW; p.stride = a.stride; p.stride_w = a.stride_w; p.pad = a.pad; p.pad_w = a.pad_w;
    p.Win = a.Win; p.Wout = a.Wout;
    p.row_mask = a.row_mask != nullptr;
    return p;
}

}  // namespace

// Entry from gemm.hip's dispatcher: launch the resident-weight kernel when the problem
// fits it; false leaves the call to the tiled kernel.
bool launch_rw(const GemmArgs& a, int in_dtype, int out_dtype, hipStream_t stream) {
    return launch_planned(rw_problem(RW_GEMM, a, in_dtype, out_dtype), a, stream);
}

// Entry from gemm.hip's conv dispatcher (same-type convolutions: the tap-folded stem form and the
// strided 1x1, gemm_rw_plan.h); false leaves the call to the tiled kernel.
bool launch_rw_conv(const GemmArgs& a, int in_dtype, hipStream_t stream) {
    RwProblem p = rw_problem(RW_CONV, a, in_dtype, in_dtype);
    p.a2 = false;   // (convolutions take no A2)
    return launch_planned(p, a, stream);
}

}  // namespace kinet

using namespace kinet;

extern "C" int kinet_gemm_rw_last_config(int* out) {
    KINET_CHECK_ARG(out != nullptr, "gemm rw last config: NULL argument");
    for (int i = 0; i < RW_CFG_FIELDS; ++i) out[i] = rw_last_cfg[i];
    return KINET_OK;
}

extern "C" int kinet_gemm_rw_grid_cap(int max_p) {
    const int old = rw_grid_cap;
    rw_grid_cap = max_p > 0 ? max_p : 0;
    return old;
}

extern "C" int kinet_gemm_rw_min_a2_rows(void) { return kRwMinA2Rows; }

extern "C" int kinet_gemm_rw_plan(const int* problem, int cus, int* eligible, int* config) {
    KINET_CHECK_ARG(problem != nullptr && eligible != nullptr && config != nullptr && cus > 0, "gemm_rw_plan: invalid arguments");
    const int* f = problem;
    KINET_CHECK_ARG(f[KINET_RWP_KIND] >= RW_GEMM && f[KINET_RWP_KIND] <= RW_RECORDS && f[KINET_RWP_M] >= 0 &&
                        f[KINET_RWP_N] >= 0 && f[KINET_RWP_K] > 0, "gemm_rw_plan: invalid problem");
    // (what kinet_msda_sample_records checks before it plans)
    KINET_CHECK_ARG(f[KINET_RWP_KIND] != RW_RECORDS || (f[KINET_RWP_K] == 256 && f[KINET_RWP_N] % 192 == 0 && f[KINET_RWP_M] > 0 &&
                                                        f[KINET_RWP_OUT_DTYPE] == KINET_F16),
                    "gemm_rw_plan: records are K = 256, N = heads * 48 with heads %% 4 == 0, M > 0, f16 output");
    RwProblem p{};
    p.kind = f[KINET_RWP_KIND];
    p.M = f[KINET_RWP_M]; p.N = f[KINET_RWP_N]; p.K = f[KINET_RWP_K];
    p.in_dtype = f[KINET_RWP_IN_DTYPE]; p.out_dtype = f[KINET_RWP_OUT_DTYPE];
    p.r = f[KINET_RWP_RESIDUAL] != 0; p.ln = f[KINET_RWP_LN] != 0; p.a2 = f[KINET_RWP_A2] != 0;
    p.ldc = f[KINET_RWP_LDC]; p.ldr = f[KINET_RWP_LDR];
    p.c_al16 = f[KINET_RWP_C_ALIGNED] != 0; p.r_al16 = f[KINET_RWP_R_ALIGNED] != 0; p.a2_al16 = f[KINET_RWP_A2_ALIGNED] != 0;
    p.hm_rows = f[KINET_RWP_HM_ROWS]; p.hm_d = f[KINET_RWP_HM_D]; p.hm_split = f[KINET_RWP_HM_SPLIT]; p.hm_d2 = f[KINET_RWP_HM_D2];
    p.Cin = f[KINET_RWP_CIN]; p.KW = f[KINET_RWP_KW]; p.stride = f[KINET_RWP_STRIDE]; p.stride_w = f[KINET_RWP_STRIDE_W];
    p.pad = f[KINET_RWP_PAD]; p.pad_w = f[KINET_RWP_PAD_W]; p.Win = f[KINET_RWP_WIN]; p.Wout = f[KINET_RWP_WOUT];
    p.row_mask = f[KINET_RWP_ROW_MASK] != 0;
    p.flags = kinet_gemm_flags;
    p.cap = rw_grid_cap;
    p.cus = cus;
    RwPlan plan;
    *eligible = rw_plan(p, plan) ? 1 : 0;
    for (int i = 0; i < RW_CFG_FIELDS; ++i) config[i] = 0;
    if (*eligible) rw_config_record(plan, p.out_dtype, config);
    return KINET_OK;
}

// The MSDA sampling-offsets | attention-weights projection of an encoder call, with the
// softmax, sampling locations and bilinear setup in its epilogue (prep_records): writes the
// head-major sampling records kinet_msda_encoder_forward_records reads.  include/kinet_msda.h.
extern "C" int kinet_msda_sample_records(const void* A, const void* A2, const void* W, const float* bias, int M,
                                         int num_heads, int K, int lda, int in_dtype, const float* ref_points,
                                         int ref_dim, const uint8_t* query_attn_mask, const int64_t* spatial_shapes_host,
                                         int num_levels, int num_point, int frac_bits, void* records,
                                         int a2_rows, kinet_stream_t stream) {
    KINET_CHECK_ARG(a2_rows == 0 || (A2 != nullptr && a2_rows >= kRwMinA2Rows && M % a2_rows == 0),
                    "msda records: a2_rows must be 0 or >= 32 dividing M (got %d)", a2_rows);
    KINET_CHECK_ARG(M >= 0 && num_heads > 0 && num_heads % 4 == 0, "msda records: heads must be a multiple of 4 (got %d)",
                    num_heads);
    KINET_CHECK_ARG(num_levels == 4 && num_point == 4, "msda records: 4 levels x 4 points (got %d, %d)", num_levels,
                    num_point);
    KINET_CHECK_ARG(K == 256 && lda % 8 == 0 && lda >= K, "msda records: K must be 256 (got %d), lda %% 8 == 0", K);
    KINET_CHECK_ARG(in_dtype == KINET_BF16 || in_dtype == KINET_F16, "msda records: bf16 / f16 operands");
    KINET_CHECK_ARG(ref_dim == 2 || ref_dim == 4, "Last dim of reference_points must be 2 or 4, but get %d instead.",
                    ref_dim);
    KINET_CHECK_ARG(frac_bits >= 6 && frac_bits <= 10, "msda records: frac_bits in [6, 10] (got %d)", frac_bits);
    KINET_CHECK_ARG(spatial_shapes_host != nullptr && ref_points != nullptr && records != nullptr && W != nullptr &&
                        bias != nullptr, "msda records: NULL argument");
    KINET_CHECK_ARG((((uintptr_t)A) & 15) == 0 && (((uintptr_t)W) & 15) == 0 && (((uintptr_t)records) & 15) == 0 &&
                        (A2 == nullptr || (((uintptr_t)A2) & 15) == 0) && (((uintptr_t)ref_points) & 15) == 0,
                    "msda records: A, A2, W, refs and records must be 16-byte aligned");
    for (int l = 0; l < 4; ++l) {
        const long long H = spatial_shapes_host[2 * l], Wd = spatial_shapes_host[2 * l + 1];
        KINET_CHECK_ARG(H > 0 && Wd > 0 && H <= (1LL << (16 - frac_bits)) && Wd <= (1LL << (16 - frac_bits)),
                        "msda records: level %d (%lld x %lld) exceeds the %d-bit integer part", l, H, Wd, 16 - frac_bits);
    }
    if (M == 0) return KINET_OK;
    const int N = num_heads * 48;
    const long long ab = ((long long)(M - 1) * lda + K) * 2, bb = (long long)N * K * 2;
    const long long cb = (long long)num_heads * M * 96, rb = (long long)M * 16 * ref_dim;
    KINET_CHECK_ARG(ab < (1LL << 31) && cb < (1LL << 31) && rb < (1LL << 31), "msda records: operands larger than 2 GiB");
    GemmArgs a{};
    a.A = A; a.A2 = A2; a.B = W; a.C = records; a.bias = bias; a.row_mask = query_attn_mask; a.a2_rows = a2_rows;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = K; a.ldc = N;
    a.a_bytes = (int)ab; a.b_bytes = (int)bb; a.c_bytes = (int)cb;
    a.prep_ref = ref_points; a.prep_refd = ref_dim; a.prep_fb = frac_bits;
    for (int l = 0; l < 4; ++l) {
        a.prep_H[l] = (int)spatial_shapes_host[2 * l];
        a.prep_W[l] = (int)spatial_shapes_host[2 * l + 1];
    }
    // (which of the three record variants: rw_plan, RW_RECORDS)
    if (!launch_planned(rw_problem(RW_RECORDS, a, in_dtype, KINET_F16), a, (hipStream_t)stream)) {
        set_error("msda records: no kernel variant for this call");
        return KINET_ERR_ARG;
    }
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}
