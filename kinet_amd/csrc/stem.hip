// Tap-folded ResNet stem convolution for gfx950 (torchvision conv1: 7x7, stride 2, pad 3,
// 3 -> 64 channels, + folded FrozenBatchNorm + ReLU; backbone.py).
//
// Input: pack_image_kwfold's layout (ops.hip) -- F[n][ih][ow][kw*3 + c] (24 channels, the 7
// horizontal taps of output column ow folded in), so the convolution is 7 x 1 with vertical
// stride 2 and no horizontal halo: output (oh, ow) = sum over kh of F[2*oh - 3 + kh][ow][:] . W.
// The implicit-GEMM kernels re-gather every folded row once per output row that uses it
// (7 taps / stride 2 = 3.5x the input through the load path, ~0.7 GB per batch-8 call) and
// with K = 168 a tiled K-loop never gets going.  Here a persistent workgroup walks 4-row x
// 64-column output tiles (the next tile's input loads in flight under the current one):
//  * its 13 folded input rows (2*3 + 7) are loaded ONCE into LDS (39 KiB, 16-byte loads,
//    zeros outside the image) and shared by the 4 output rows (1.6x the input instead of 3.5x);
//  * each wave computes one output row (64 pixels x 64 channels = 16 MFMA tiles) over the
//    6 K-steps of 32 (21 valid 8-channel chunks, the rest zero) with the weights as MFMA
//    A-fragments in registers and the pixel fragments read straight from the folded rows;
//  * epilogue: scale / bias / ReLU on the accumulators, the bf16 tile parked in LDS (16-byte
//    chunks XOR-swizzled by pixel) and written back as whole 128-byte pixel rows.
#include <hip/hip_runtime.h>

#include "../../include/kinet_gemm.h"
#include "common.h"
#include "gemm_common.h"

namespace kinet {
namespace {

constexpr int SK_KH = 7, SK_CG = 24, SK_CO = 64;
constexpr int SK_RH = 4;                              // output rows per workgroup (one per wave)
constexpr int SK_PX = 64;                             // output columns per workgroup
constexpr int SK_ROWS = 2 * (SK_RH - 1) + SK_KH;      // 13 folded input rows
constexpr int SK_ROWB = SK_PX * SK_CG * 2;            // 3072 bytes per folded row segment
constexpr int SK_NCH = SK_KH * SK_CG / 8;             // 21 valid 8-channel chunks of K
constexpr int SK_KS = (SK_NCH + 3) / 4;               // 6 K-steps of 32
constexpr int SK_IN_CH = SK_ROWS * SK_PX * 3;         // 2496 16-byte input chunks
constexpr int SK_IN_OPS = (SK_IN_CH + 255) / 256;     // 10 per thread
static_assert(SK_RH * SK_PX * SK_CO * 2 <= SK_ROWS * SK_ROWB, "output tile fits the input LDS");

template <typename T>
__global__ __launch_bounds__(256, 2) void stem_conv_kernel(const GemmArgs p, const int tiles_x, const int tiles_y,
                                                           const int ntiles) {
    __shared__ __attribute__((aligned(16))) char lds[SK_ROWS * SK_ROWB];
    __shared__ float par[2][SK_CO];             // folded BN scale / bias
    __shared__ __attribute__((aligned(16))) u32x4 wl[4 * SK_KS][64];   // weight fragments (24 KiB)
    constexpr unsigned OOB = 0x80000000u;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < SK_CO) {
        par[0][tid] = p.scale ? p.scale[tid] : 1.f;
        par[1][tid] = p.bias ? p.bias[tid] : 0.f;
    }
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, (short)0, p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, (short)0, p.b_bytes, 0x00020000);

    // persistent: tiles blockIdx.x, +gridDim.x, ...; tile -> (image, 4-row block, 64-column block)
    struct Tile { int n, oh0, ow0; };
    auto decode = [&](int t) {
        const int bx = t % tiles_x, rest = t / tiles_x;
        return Tile{rest / tiles_y, (rest % tiles_y) * SK_RH, bx * SK_PX};
    };
    // folded input rows 2*oh0 - 3 .. +12, columns ow0 .. ow0+63 -> registers (zeros outside)
    u32x4 xin[SK_IN_OPS];
    auto load_in = [&](const Tile& tl) {
        const int ih0 = tl.oh0 * 2 - 3;
#pragma unroll
        for (int i = 0; i < SK_IN_OPS; ++i) {
            const int idx = i * 256 + tid;
            const int r = idx / (SK_PX * 3), rem = idx - r * (SK_PX * 3);
            const int px = rem / 3, part = rem - px * 3;
            const int ih = ih0 + r, ow = tl.ow0 + px;
            const bool ok = idx < SK_IN_CH && (unsigned)ih < (unsigned)p.Hin && ow < p.Win;
            const unsigned off = ok ? ((unsigned)(((tl.n * p.Hin + ih) * p.Win + ow) * SK_CG + part * 8)) * 2u : OOB;
            xin[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0);
        }
    };
    int t = blockIdx.x;
    Tile cur = decode(t);
    load_in(cur);

    // weights (Cout, 168) as MFMA A-fragments, staged once into LDS fragment-major: lane l of
    // fragment (a, s) holds out channel a*16 + (l&15), k = 32*s + 8*(l>>4) .. +7 (zero past K)
    for (int f = wave; f < 4 * SK_KS; f += 4) {
        const int a = f / SK_KS, s = f - a * SK_KS;
        const int k = 32 * s + 8 * (lane >> 4);
        const unsigned off = k < SK_NCH * 8 ? ((unsigned)((a * 16 + (lane & 15)) * p.ldb + k)) * 2u : OOB;
        wl[f][lane] = __builtin_amdgcn_raw_buffer_load_b128(rw, off, 0, 0);
    }
    T* __restrict__ C = (T*)p.C;

    for (; t < ntiles; t += gridDim.x) {
#pragma unroll
        for (int i = 0; i < SK_IN_OPS; ++i) {
            const int idx = i * 256 + tid;
            if (idx < SK_IN_CH) *reinterpret_cast<u32x4*>(lds + idx * 16) = xin[i];   // = r*ROWB + px*48 + part*16
        }
        __syncthreads();
        // the next tile's input loads fly under this tile's MFMAs and epilogue
        const int tn = t + gridDim.x;
        const Tile nxt = decode(tn < ntiles ? tn : t);
        if (tn < ntiles) load_in(nxt);

        // wave w: output row oh0 + w; pixel fragment of K-step s = 8 channels of chunk
        // ci = 4s + (l>>4) (tap kh = ci / 3, part ci % 3) of folded row 2w + kh, pixel l&15
        f32x4 acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[a][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < SK_KS; ++s) {
            const int ci = 4 * s + (lane >> 4);
            const int kh = ci / 3, part = ci - 3 * kh;
            const bool valid = ci < SK_NCH;
            const char* rowp = lds + (2 * wave + (valid ? kh : 0)) * SK_ROWB + part * 16;
            u32x4 wf[4], b[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) wf[a] = wl[a * SK_KS + s][lane];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                b[q] = *reinterpret_cast<const u32x4*>(rowp + (q * 16 + (lane & 15)) * (SK_CG * 2));
                if (!valid) b[q] = u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int a = 0; a < 4; ++a) Mma<T>::run(acc[a][q], wf[a], b[q]);
        }
        __syncthreads();   // every wave done with the input rows: the LDS now takes the output tile

        // epilogue: lane holds channels a*16 + 4*(l>>4) + i of pixel q*16 + (l&15) -> scale /
        // bias / ReLU -> 8 bytes into the parked tile [row][pixel][64 ch] whose 16-byte
        // chunks are XOR-swizzled by (pixel & 7)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int ch0 = a * 16 + 4 * (lane >> 4);
            const f32x4 sc = *reinterpret_cast<const f32x4*>(&par[0][ch0]);
            const f32x4 bi = *reinterpret_cast<const f32x4*>(&par[1][ch0]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int px = q * 16 + (lane & 15);
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i] = acc[a][q][i] * sc[i] + bi[i];
                    if (p.relu) v[i] = fmaxf(v[i], 0.f);
                }
                uint32_t w[2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    w[i] = (uint32_t)__builtin_bit_cast(uint16_t, Cvt<T>::from(v[2 * i])) |
                           ((uint32_t)__builtin_bit_cast(uint16_t, Cvt<T>::from(v[2 * i + 1])) << 16);
                const int chunk = (ch0 >> 3) ^ (px & 7);
                uint32_t* dst =
                    reinterpret_cast<uint32_t*>(lds + (wave * SK_PX + px) * (SK_CO * 2) + chunk * 16 + (ch0 & 4) * 2);
                dst[0] = w[0];
                dst[1] = w[1];
            }
        }
        __syncthreads();

        // whole 128-byte pixel rows, 16 bytes per lane
#pragma unroll
        for (int i = 0; i < SK_RH * SK_PX * 8 / 256; ++i) {
            const int idx = i * 256 + tid;
            const int r = idx / (SK_PX * 8), rem = idx - r * (SK_PX * 8);
            const int px = rem >> 3, c16 = rem & 7;
            const int oh = cur.oh0 + r, ow = cur.ow0 + px;
            if (oh < p.Hout && ow < p.Wout) {
                const u32x4 v =
                    *reinterpret_cast<const u32x4*>(lds + (r * SK_PX + px) * (SK_CO * 2) + ((c16 ^ (px & 7)) * 16));
                *reinterpret_cast<u32x4*>(C + ((long)(cur.n * p.Hout + oh) * p.Wout + ow) * p.ldc + c16 * 8) = v;
            }
        }
        __syncthreads();   // the parked tile is read out before the next input lands in the LDS
        cur = nxt;
    }
}

// ---------------------------------------------------------------------------------------------
// The stem straight from the f32 NCHW image (kinet_stem_conv_image): the same tiles, weights,
// MFMA schedule and epilogue as stem_conv_kernel, but each tile's 13 folded rows are BUILT in
// LDS from the image instead of read from pack_image_kwfold's folded tensor -- that kernel (a
// 205 MB read + 410 MB write at batch 16) and the stem's 1.6x re-reads of its output go away.
//  * the tile's 13 image rows x 3 planes x 133 columns (2*ow0 - 3 ..) load one tile ahead as
//    f32 (wave w: row-planes w, w+4, ..; lane: columns lane, +64, +128), zeros outside the image;
//  * at the tile start they are rounded to T (as pack_image_kwfold does) into an LDS row-plane
//    area, then every 16-byte chunk (row, pixel, part) of the folded rows is assembled from it:
//    element j = 8 part + e of pixel px is plane j % 3, column 2 px + j / 3 (zero for j >= 21).
constexpr int SI_RAWC = 136;                      // row-plane stride (elements), >= 2*63 + 7
constexpr int SI_PAIRS = SK_ROWS * 3;             // 39 row-planes per tile
constexpr int SI_PPW = (SI_PAIRS + 3) / 4;        // per wave (10)

struct StemImgArgs {
    const float* img;
    const void* W;
    const float* scale;
    const float* bias;
    void* Y;
    int N, H, W_, Ho, Wo, ldy;
    int img_bytes, w_bytes;
};

template <typename T>
__global__ __launch_bounds__(256, 2) void stem_img_kernel(const StemImgArgs p, const int tiles_x, const int tiles_y,
                                                          const int ntiles) {
    __shared__ __attribute__((aligned(16))) char lds[SK_ROWS * SK_ROWB];
    __shared__ float par[2][SK_CO];
    __shared__ __attribute__((aligned(16))) u32x4 wl[4 * SK_KS][64];
    __shared__ __attribute__((aligned(16))) uint16_t raw[SI_PAIRS * SI_RAWC];
    constexpr unsigned OOB = 0x80000000u;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < SK_CO) {
        par[0][tid] = p.scale ? p.scale[tid] : 1.f;
        par[1][tid] = p.bias ? p.bias[tid] : 0.f;
    }
    const __amdgpu_buffer_rsrc_t ri = __builtin_amdgcn_make_buffer_rsrc((void*)p.img, (short)0, p.img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, (short)0, p.w_bytes, 0x00020000);
    struct Tile { int n, oh0, ow0; };
    auto decode = [&](int t) {
        const int bx = t % tiles_x, rest = t / tiles_x;
        return Tile{rest / tiles_y, (rest % tiles_y) * SK_RH, bx * SK_PX};
    };
    float xin[SI_PPW][3];
    auto load_in = [&](const Tile& tl) {
        const int ih0 = tl.oh0 * 2 - 3, iw0 = tl.ow0 * 2 - 3;
#pragma unroll
        for (int i = 0; i < SI_PPW; ++i) {
            const int pr = i * 4 + wave;                 // row-plane (wave-uniform)
            const int r = pr / 3, c = pr - 3 * r;
            const int ih = ih0 + r;
            const bool rok = pr < SI_PAIRS && (unsigned)ih < (unsigned)p.H;
            const unsigned rowb = (unsigned)(((tl.n * 3 + c) * p.H + ih) * p.W_);
#pragma unroll
            for (int k3 = 0; k3 < 3; ++k3) {
                const int k = lane + 64 * k3, iw = iw0 + k;
                const bool ok = rok && k < SI_RAWC && (unsigned)iw < (unsigned)p.W_;
                xin[i][k3] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ri, ok ? (rowb + (unsigned)iw) * 4u : OOB, 0, 0));
            }
        }
    };
    int t = blockIdx.x;
    Tile cur = decode(t);
    load_in(cur);
    for (int f = wave; f < 4 * SK_KS; f += 4) {
        const int a = f / SK_KS, s = f - a * SK_KS;
        const int k = 32 * s + 8 * (lane >> 4);
        const unsigned off = k < SK_NCH * 8 ? ((unsigned)((a * 16 + (lane & 15)) * (SK_KH * SK_CG) + k)) * 2u : OOB;
        wl[f][lane] = __builtin_amdgcn_raw_buffer_load_b128(rw, off, 0, 0);
    }
    T* __restrict__ C = (T*)p.Y;

    for (; t < ntiles; t += gridDim.x) {
        // image values -> T row-planes (the rounding pack_image_kwfold applies)
#pragma unroll
        for (int i = 0; i < SI_PPW; ++i) {
            const int pr = i * 4 + wave;
            if (pr < SI_PAIRS) {
#pragma unroll
                for (int k3 = 0; k3 < 3; ++k3) {
                    const int k = lane + 64 * k3;
                    if (k < SI_RAWC) raw[pr * SI_RAWC + k] = __builtin_bit_cast(uint16_t, Cvt<T>::from(xin[i][k3]));
                }
            }
        }
        __syncthreads();
        // folded rows: thread = (row, pixel); its 3 chunks (row, pixel, part) -> lds +
        // ((r*64 + px)*3 + part)*16, element j = 8 part + e from plane j % 3, column 2 px + j / 3
        // (compile-time offsets: no index arithmetic per element)
        for (int rp = tid; rp < SK_ROWS * SK_PX; rp += 256) {
            const int r = rp >> 6, px = rp & (SK_PX - 1);
            const uint16_t* src = raw + r * 3 * SI_RAWC + 2 * px;
            u32x4* dst = reinterpret_cast<u32x4*>(lds + rp * 48);
#pragma unroll
            for (int part = 0; part < 3; ++part) {
                uint32_t w[4];
#pragma unroll
                for (int e2 = 0; e2 < 4; ++e2) {
                    uint32_t h2[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int j = part * 8 + 2 * e2 + h, kw = j / 3, c = j - 3 * kw;
                        h2[h] = j < SK_KH * 3 ? (uint32_t)src[c * SI_RAWC + kw] : 0u;
                    }
                    w[e2] = h2[0] | (h2[1] << 16);
                }
                dst[part] = u32x4{w[0], w[1], w[2], w[3]};
            }
        }
        __syncthreads();
        const int tn = t + gridDim.x;
        const Tile nxt = decode(tn < ntiles ? tn : t);
        if (tn < ntiles) load_in(nxt);

        f32x4 acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[a][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < SK_KS; ++s) {
            const int ci = 4 * s + (lane >> 4);
            const int kh = ci / 3, part = ci - 3 * kh;
            const bool valid = ci < SK_NCH;
            const char* rowp = lds + (2 * wave + (valid ? kh : 0)) * SK_ROWB + part * 16;
            u32x4 wf[4], b[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) wf[a] = wl[a * SK_KS + s][lane];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                b[q] = *reinterpret_cast<const u32x4*>(rowp + (q * 16 + (lane & 15)) * (SK_CG * 2));
                if (!valid) b[q] = u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int a = 0; a < 4; ++a) Mma<T>::run(acc[a][q], wf[a], b[q]);
        }
        __syncthreads();

#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int ch0 = a * 16 + 4 * (lane >> 4);
            const f32x4 sc = *reinterpret_cast<const f32x4*>(&par[0][ch0]);
            const f32x4 bi = *reinterpret_cast<const f32x4*>(&par[1][ch0]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int px = q * 16 + (lane & 15);
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[a][q][i] * sc[i] + bi[i], 0.f);
                uint32_t w[2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    w[i] = (uint32_t)__builtin_bit_cast(uint16_t, Cvt<T>::from(v[2 * i])) |
                           ((uint32_t)__builtin_bit_cast(uint16_t, Cvt<T>::from(v[2 * i + 1])) << 16);
                const int chunk = (ch0 >> 3) ^ (px & 7);
                uint32_t* dst =
                    reinterpret_cast<uint32_t*>(lds + (wave * SK_PX + px) * (SK_CO * 2) + chunk * 16 + (ch0 & 4) * 2);
                dst[0] = w[0];
                dst[1] = w[1];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SK_RH * SK_PX * 8 / 256; ++i) {
            const int idx = i * 256 + tid;
            const int r = idx / (SK_PX * 8), rem = idx - r * (SK_PX * 8);
            const int px = rem >> 3, c16 = rem & 7;
            const int oh = cur.oh0 + r, ow = cur.ow0 + px;
            if (oh < p.Ho && ow < p.Wo) {
                const u32x4 v =
                    *reinterpret_cast<const u32x4*>(lds + (r * SK_PX + px) * (SK_CO * 2) + ((c16 ^ (px & 7)) * 16));
                *reinterpret_cast<u32x4*>(C + ((long)(cur.n * p.Ho + oh) * p.Wo + ow) * p.ldy + c16 * 8) = v;
            }
        }
        __syncthreads();
        cur = nxt;
    }
}

// ---------------------------------------------------------------------------------------------
// Stem + 3x3 / stride 2 / pad 1 max-pool in one launch (kinet_stem_pool_image): the conv map
// (N, Ho, Wo, 64) is never written; Y is the pooled map (N, Hp, Wp, 64).  Every conv value is
// computed exactly as in stem_img_kernel (same folded rows, weights, MFMA order, epilogue), so
// the result is bit-identical to the pool of that kernel's output.
//  * a workgroup walks a strip of 64 conv columns DOWNWARDS in 4-row tiles.  Strips advance by
//    62 conv columns = 31 pooled columns: strip sx covers conv columns 62 sx - 1 .. 62 sx + 62,
//    so the pool's left halo is one recomputed column inside the 64 (64 / 62 recompute);
//  * tile t (conv rows 4t .. 4t+3) yields pooled rows 2t (conv rows 4t-1, 4t, 4t+1) and 2t+1
//    (4t+1 .. 4t+3).  Conv row 4t-1 is row 3 of the tile before: it is CARRIED in registers
//    (two 16-byte chunks per thread, taken from the parked tile) and dropped into the `raw`
//    area -- idle between the folded-row build and the next tile's conversion -- for the pool;
//  * a unit of work is (vertical segment of seg_tiles tiles, image, strip).  A segment that
//    does not start at the image top first computes just conv row 4 t0 - 1 (the `pre` step: 7
//    image rows, each wave one 16-pixel block of that row: a quarter tile of MFMAs);
//  * conv rows / columns outside [0, Ho) x [0, Wo) park as -0.0 (0x8000), the smallest value of
//    the signed 16-bit compare the pool uses: conv values are post-ReLU (sign bit clear, or -0.0),
//    so the signed integer maximum of the 16-bit patterns is the floating-point maximum over the
//    window's in-range taps (the centre tap is always in range).
constexpr int SP_STRIDE = SK_PX - 2;              // conv columns a strip advances by (62)
constexpr int SP_PQ = SP_STRIDE / 2;              // pooled columns per strip (31)
constexpr int SP_PRE_ROW0 = 2 * (SK_RH - 1);      // first folded row conv row 3 of a tile reads (6)
constexpr uint32_t SP_NEG = 0x80008000u;          // two -0.0 in either 16-bit format
static_assert(SK_PX * SK_CO * 2 <= SI_PAIRS * SI_RAWC * 2, "the carried conv row fits the raw area");
static_assert(SK_PX * SK_CO * 2 == 2 * 256 * 16, "the carried row is two 16-byte chunks per thread");
static_assert(SP_PQ * 8 <= 256, "one pooled (column, chunk) item per thread");

struct StemPoolArgs {
    const float* img;
    const void* W;
    const float* scale;
    const float* bias;
    void* Y;
    int N, H, W_, Ho, Wo, Hp, Wp;
    int img_bytes, w_bytes;
    int strips, tiles_y, seg_tiles, nunits;
};

typedef short s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ u32x4 sp_max(const u32x4 a, const u32x4 b) {
    return __builtin_bit_cast(u32x4, __builtin_elementwise_max(__builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b)));
}

// One conv row (tile row `row`: folded rows 2 row .. 2 row + 6) x NQ 16-pixel blocks from qb:
// stem_img_kernel's K loop (same order of sums per element).
template <typename T, int NQ>
__device__ __forceinline__ void sp_row_mma(const char* lds, const u32x4 (*wl)[64], const int row, const int qb,
                                           const int lane, f32x4 (&acc)[4][NQ]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[a][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < SK_KS; ++s) {
        const int ci = 4 * s + (lane >> 4);
        const int kh = ci / 3, part = ci - 3 * kh;
        const bool valid = ci < SK_NCH;
        const char* rowp = lds + (2 * row + (valid ? kh : 0)) * SK_ROWB + part * 16;
        u32x4 wf[4], b[NQ];
#pragma unroll
        for (int a = 0; a < 4; ++a) wf[a] = wl[a * SK_KS + s][lane];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            b[q] = *reinterpret_cast<const u32x4*>(rowp + ((qb + q) * 16 + (lane & 15)) * (SK_CG * 2));
            if (!valid) b[q] = u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int a = 0; a < 4; ++a) Mma<T>::run(acc[a][q], wf[a], b[q]);
    }
}

// stem_img_kernel's epilogue (scale / bias / ReLU, rounded to T, parked [row][pixel][64 ch] with
// the 16-byte chunks XOR-swizzled by pixel & 7); pixels outside the conv map park as -0.0.
template <typename T, int NQ>
__device__ __forceinline__ void sp_row_park(char* lds, const float (*par)[SK_CO], const int row, const int qb,
                                            const int lane, const f32x4 (&acc)[4][NQ], const bool row_ok,
                                            const int ow0, const int Wo) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int ch0 = a * 16 + 4 * (lane >> 4);
        const f32x4 sc = *reinterpret_cast<const f32x4*>(&par[0][ch0]);
        const f32x4 bi = *reinterpret_cast<const f32x4*>(&par[1][ch0]);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int px = (qb + q) * 16 + (lane & 15);
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[a][q][i] * sc[i] + bi[i], 0.f);
            uint32_t w[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                w[i] = (uint32_t)__builtin_bit_cast(uint16_t, Cvt<T>::from(v[2 * i])) |
                       ((uint32_t)__builtin_bit_cast(uint16_t, Cvt<T>::from(v[2 * i + 1])) << 16);
            if (!row_ok || (unsigned)(ow0 + px) >= (unsigned)Wo) w[0] = w[1] = SP_NEG;
            const int chunk = (ch0 >> 3) ^ (px & 7);
            uint32_t* dst = reinterpret_cast<uint32_t*>(lds + (row * SK_PX + px) * (SK_CO * 2) + chunk * 16 + (ch0 & 4) * 2);
            dst[0] = w[0];
            dst[1] = w[1];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256, 2) void stem_pool_kernel(const StemPoolArgs p) {
    __shared__ __attribute__((aligned(16))) char lds[SK_ROWS * SK_ROWB];
    __shared__ float par[2][SK_CO];
    __shared__ __attribute__((aligned(16))) u32x4 wl[4 * SK_KS][64];
    __shared__ __attribute__((aligned(16))) uint16_t raw[SI_PAIRS * SI_RAWC];
    constexpr unsigned OOB = 0x80000000u;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < SK_CO) {
        par[0][tid] = p.scale ? p.scale[tid] : 1.f;
        par[1][tid] = p.bias ? p.bias[tid] : 0.f;
    }
    const __amdgpu_buffer_rsrc_t ri = __builtin_amdgcn_make_buffer_rsrc((void*)p.img, (short)0, p.img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, (short)0, p.w_bytes, 0x00020000);

    // persistent: units blockIdx.x, +gridDim.x, ..; unit -> (segment, image, strip), segment-major
    // so the short last segments of the strips land in the last round.  A step is one tile of the
    // unit's segment, or (pre) conv row 3 of the tile above the segment.
    struct Step { int u, n, sx, t, t1; bool pre; };
    const int per_seg = p.N * p.strips;
    auto first_step = [&](int u) {
        Step s{u, 0, 0, 0, 0, false};
        if (u >= p.nunits) return s;
        const int sg = u / per_seg, rest = u - sg * per_seg;
        s.n = rest / p.strips;
        s.sx = rest - s.n * p.strips;
        const int t0 = sg * p.seg_tiles;
        s.t1 = min(t0 + p.seg_tiles, p.tiles_y);
        s.pre = sg > 0;
        s.t = s.pre ? t0 - 1 : t0;
        return s;
    };
    auto next_step = [&](Step s) {
        if (s.pre || s.t + 1 < s.t1) {
            s.pre = false;
            ++s.t;
            return s;
        }
        return first_step(s.u + (int)gridDim.x);
    };
    // the step's image rows x 3 planes x 133 columns, one step ahead (stem_img_kernel's loads;
    // a pre step needs only the row-planes of folded rows 6 .. 12)
    float xin[SI_PPW][3];
    auto load_in = [&](const Step& st) {
        const int ih0 = st.t * SK_RH * 2 - 3, iw0 = (st.sx * SP_STRIDE - 1) * 2 - 3;
        const int pr0 = st.pre ? SP_PRE_ROW0 * 3 : 0;
#pragma unroll
        for (int i = 0; i < SI_PPW; ++i) {
            const int pr = i * 4 + wave;                 // row-plane (wave-uniform)
            const int r = pr / 3, c = pr - 3 * r;
            const int ih = ih0 + r;
            const bool rok = pr >= pr0 && pr < SI_PAIRS && (unsigned)ih < (unsigned)p.H;
            const unsigned rowb = (unsigned)(((st.n * 3 + c) * p.H + ih) * p.W_);
#pragma unroll
            for (int k3 = 0; k3 < 3; ++k3) {
                const int k = lane + 64 * k3, iw = iw0 + k;
                const bool ok = rok && k < SI_RAWC && (unsigned)iw < (unsigned)p.W_;
                xin[i][k3] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ri, ok ? (rowb + (unsigned)iw) * 4u : OOB, 0, 0));
            }
        }
    };
    Step cur = first_step(blockIdx.x);
    load_in(cur);
    for (int f = wave; f < 4 * SK_KS; f += 4) {
        const int a = f / SK_KS, s = f - a * SK_KS;
        const int k = 32 * s + 8 * (lane >> 4);
        const unsigned off = k < SK_NCH * 8 ? ((unsigned)((a * 16 + (lane & 15)) * (SK_KH * SK_CG) + k)) * 2u : OOB;
        wl[f][lane] = __builtin_amdgcn_raw_buffer_load_b128(rw, off, 0, 0);
    }
    T* __restrict__ Y = (T*)p.Y;
    u32x4* const rawq = reinterpret_cast<u32x4*>(raw);                       // the carried row, parked layout
    const u32x4* const row3 = reinterpret_cast<const u32x4*>(lds + (SK_RH - 1) * SK_PX * SK_CO * 2);
    u32x4 carry[2] = {};                                                     // conv row 4t - 1: chunks tid, tid + 256

    while (cur.u < p.nunits) {
        const int oh0 = cur.t * SK_RH, ow0 = cur.sx * SP_STRIDE - 1;
        const int pr0 = cur.pre ? SP_PRE_ROW0 * 3 : 0;
        if (!cur.pre && cur.t == 0) carry[0] = carry[1] = u32x4{SP_NEG, SP_NEG, SP_NEG, SP_NEG};   // above the image
#pragma unroll
        for (int i = 0; i < SI_PPW; ++i) {
            const int pr = i * 4 + wave;
            if (pr >= pr0 && pr < SI_PAIRS) {
#pragma unroll
                for (int k3 = 0; k3 < 3; ++k3) {
                    const int k = lane + 64 * k3;
                    if (k < SI_RAWC) raw[pr * SI_RAWC + k] = __builtin_bit_cast(uint16_t, Cvt<T>::from(xin[i][k3]));
                }
            }
        }
        __syncthreads();
        for (int rp = tid + (cur.pre ? SP_PRE_ROW0 * SK_PX : 0); rp < SK_ROWS * SK_PX; rp += 256) {
            const int r = rp >> 6, px = rp & (SK_PX - 1);
            const uint16_t* src = raw + r * 3 * SI_RAWC + 2 * px;
            u32x4* dst = reinterpret_cast<u32x4*>(lds + rp * 48);
#pragma unroll
            for (int part = 0; part < 3; ++part) {
                uint32_t w[4];
#pragma unroll
                for (int e2 = 0; e2 < 4; ++e2) {
                    uint32_t h2[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int j = part * 8 + 2 * e2 + h, kw = j / 3, c = j - 3 * kw;
                        h2[h] = j < SK_KH * 3 ? (uint32_t)src[c * SI_RAWC + kw] : 0u;
                    }
                    w[e2] = h2[0] | (h2[1] << 16);
                }
                dst[part] = u32x4{w[0], w[1], w[2], w[3]};
            }
        }
        __syncthreads();
        // raw is idle until the next step's conversion: it takes the carried row for the pool
        if (!cur.pre) {
            rawq[tid] = carry[0];
            rawq[tid + 256] = carry[1];
        }
        const Step nxt = next_step(cur);
        if (nxt.u < p.nunits) load_in(nxt);

        if (cur.pre) {
            f32x4 acc[4][1];
            sp_row_mma<T, 1>(lds, wl, SK_RH - 1, wave, lane, acc);
            __syncthreads();
            sp_row_park<T, 1>(lds, par, SK_RH - 1, wave, lane, acc, true, ow0, p.Wo);
        } else {
            f32x4 acc[4][4];
            sp_row_mma<T, 4>(lds, wl, wave, 0, lane, acc);
            __syncthreads();   // every wave done with the input rows: the LDS now takes the conv tile
            sp_row_park<T, 4>(lds, par, wave, 0, lane, acc, oh0 + wave < p.Ho, ow0, p.Wo);
        }
        __syncthreads();
        carry[0] = row3[tid];
        carry[1] = row3[tid + 256];
        if (!cur.pre && tid < SP_PQ * 8) {
            // thread = (pooled column, 16-byte chunk): horizontal maxima of the carried row and the
            // 4 parked rows, then pooled rows 2t (rows -1, 0, 1) and 2t + 1 (rows 1, 2, 3)
            const int pq = tid >> 3, c16 = tid & 7;
            u32x4 h[SK_RH + 1];
#pragma unroll
            for (int rr = 0; rr <= SK_RH; ++rr) {
                const char* base = rr == 0 ? reinterpret_cast<const char*>(raw) : lds + (rr - 1) * SK_PX * SK_CO * 2;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const int px = 2 * pq + d;
                    const u32x4 v = *reinterpret_cast<const u32x4*>(base + px * (SK_CO * 2) + ((c16 ^ (px & 7)) * 16));
                    h[rr] = d == 0 ? v : sp_max(h[rr], v);
                }
            }
            const int q = cur.sx * SP_PQ + pq, pr = 2 * cur.t;
            if (q < p.Wp) {
                T* yp = Y + ((long)(cur.n * p.Hp + pr) * p.Wp + q) * SK_CO + c16 * 8;
                *reinterpret_cast<u32x4*>(yp) = sp_max(sp_max(h[0], h[1]), h[2]);
                if (pr + 1 < p.Hp) *reinterpret_cast<u32x4*>(yp + (long)p.Wp * SK_CO) = sp_max(sp_max(h[2], h[3]), h[4]);
            }
        }
        __syncthreads();   // the parked tile and the carried row are read out before the next step
        cur = nxt;
    }
}

}  // namespace

// Entry from gemm.hip's conv dispatcher (false = not the stem geometry): the 7 x 1 conv with
// strides (2, 1), pads (3, 0) of 24 folded channels into 64 outputs, 16-bit, no residual.
bool launch_stem_conv(const GemmArgs& a, int dtype, hipStream_t stream) {
    if (dtype != KINET_BF16 && dtype != KINET_F16) return false;
    if (a.KW != 1 || a.Cin != SK_CG || a.K != SK_KH * SK_CG || a.N != SK_CO || a.stride != 2 || a.pad != 3 ||
        a.stride_w != 1 || a.pad_w != 0 || a.Win != a.Wout)
        return false;
    if (a.R != nullptr || a.ln_g != nullptr || a.row_mask != nullptr || a.kchunk != 0 || a.ldc % 8 != 0 ||
        (((uintptr_t)a.C) & 15u) != 0 || a.ldb != SK_KH * SK_CG)
        return false;
    const int hw = a.Hout * a.Wout;
    if (hw <= 0 || a.M % hw != 0) return false;
    const int batch = a.M / hw;
    if (batch == 0) return true;
    const int tiles_x = (a.Wout + SK_PX - 1) / SK_PX, tiles_y = (a.Hout + SK_RH - 1) / SK_RH;
    const long long nt = (long long)tiles_x * tiles_y * batch;
    if (nt >= (1LL << 31)) return false;
    const int grid = nt < 512 ? (int)nt : 512;   // persistent: two workgroups per CU
    if (dtype == KINET_BF16)
        hipLaunchKernelGGL((stem_conv_kernel<bf16_t>), dim3(grid), dim3(256), 0, stream, a, tiles_x, tiles_y, (int)nt);
    else
        hipLaunchKernelGGL((stem_conv_kernel<f16_t>), dim3(grid), dim3(256), 0, stream, a, tiles_x, tiles_y, (int)nt);
    return true;
}

}  // namespace kinet

using namespace kinet;

// torchvision conv1 (7x7 / 2, pad 3, 3 -> 64) + folded FrozenBN + ReLU from the f32 NCHW image
// (backbone.py:102's ResNet stem) -- include/kinet_gemm.h
extern "C" int kinet_stem_conv_image(const float* img, const void* w_packed, const float* scale, const float* bias,
                                     void* Y, int N, int H, int W, int dtype, kinet_stream_t stream) {
    KINET_CHECK_ARG(N >= 0 && H > 0 && W > 0, "stem_conv_image: bad geometry");
    KINET_CHECK_ARG(dtype == KINET_BF16 || dtype == KINET_F16, "stem_conv_image: dtype must be bf16 or f16");
    KINET_CHECK_ARG(img && w_packed && Y, "stem_conv_image: NULL argument");
    KINET_CHECK_ARG((((uintptr_t)Y) & 15u) == 0 && (((uintptr_t)w_packed) & 15u) == 0, "stem_conv_image: Y and weights must be 16-byte aligned");
    if (N == 0) return KINET_OK;
    const long long ib = (long long)N * 3 * H * W * 4;
    KINET_CHECK_ARG(ib < (1LL << 31), "stem_conv_image: image batch larger than 2 GiB (split the call)");
    StemImgArgs a{};
    a.img = img; a.W = w_packed; a.scale = scale; a.bias = bias; a.Y = Y;
    a.N = N; a.H = H; a.W_ = W; a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1; a.ldy = SK_CO;
    a.img_bytes = (int)ib;
    a.w_bytes = SK_CO * SK_KH * SK_CG * 2;
    const int tiles_x = (a.Wo + SK_PX - 1) / SK_PX, tiles_y = (a.Ho + SK_RH - 1) / SK_RH;
    const long long nt = (long long)tiles_x * tiles_y * N;
    KINET_CHECK_ARG(nt < (1LL << 31), "stem_conv_image: too many tiles");
    const int grid = nt < 512 ? (int)nt : 512;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == KINET_BF16)
        hipLaunchKernelGGL((stem_img_kernel<bf16_t>), dim3(grid), dim3(256), 0, s, a, tiles_x, tiles_y, (int)nt);
    else
        hipLaunchKernelGGL((stem_img_kernel<f16_t>), dim3(grid), dim3(256), 0, s, a, tiles_x, tiles_y, (int)nt);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

constexpr int SP_GRID = 512;   // persistent: two workgroups per CU

// Segment length (tiles) for kinet_stem_pool_image's units when the caller leaves it open: the
// one whose busiest workgroup has least to do, walking the kernel's own unit order (unit u ->
// workgroup u % SP_GRID, segment u / columns; a unit costs its tiles, the last segment's being
// fewer, plus 3 quarter tiles for a pre step: tools/stem_pool_ab.py at batch 16 / 28).  Only the
// most even split of each segment count is a candidate; ties go to the longer segments.  With 8
// rounds of whole strips there is nothing to even out.  The last answer is kept per thread: the
// walk is ~1e5 steps for a config-2 batch.
static int stem_pool_seg_tiles(int batch, int strips, int tiles_y) {
    thread_local int key[3] = {0, 0, 0}, val = 0;
    if (key[0] == batch && key[1] == strips && key[2] == tiles_y) return val;
    const long long cols = (long long)batch * strips;
    int best = tiles_y;
    long long best_cost = -1;
    for (int s = 1; s <= tiles_y && cols < 8 * SP_GRID; ++s) {
        const int nseg = (tiles_y + s - 1) / s;
        if (s > 1 && (tiles_y + s - 2) / (s - 1) == nseg) continue;
        long long load[SP_GRID] = {}, cost = 0;   // in quarter tiles
        unsigned u = 0;
        for (int sg = 0; sg < nseg; ++sg) {
            const int len = 4 * (sg + 1 < nseg ? s : tiles_y - sg * s) + (sg > 0 ? 3 : 0);
            for (long long c = 0; c < cols; ++c) load[u++ % SP_GRID] += len;
        }
        for (int b = 0; b < SP_GRID; ++b) cost = load[b] > cost ? load[b] : cost;
        if (best_cost < 0 || cost <= best_cost) best = s, best_cost = cost;
    }
    key[0] = batch, key[1] = strips, key[2] = tiles_y, val = best;
    return best;
}

// The stem above + torchvision's maxpool (3x3 / stride 2 / pad 1) in one launch: img f32 NCHW ->
// Y NHWC (N, Hp, Wp, 64), bit-identical to kinet_maxpool2d_3x3s2 of kinet_stem_conv_image's
// output -- include/kinet_gemm.h
extern "C" int kinet_stem_pool_image(const float* img, const void* w_packed, const float* scale, const float* bias,
                                     void* Y, int N, int H, int W, int dtype, int seg_tiles, kinet_stream_t stream) {
    KINET_CHECK_ARG(N >= 0 && H > 0 && W > 0 && seg_tiles >= 0, "stem_pool_image: bad geometry");
    KINET_CHECK_ARG(dtype == KINET_BF16 || dtype == KINET_F16, "stem_pool_image: dtype must be bf16 or f16");
    KINET_CHECK_ARG(img && w_packed && Y, "stem_pool_image: NULL argument");
    KINET_CHECK_ARG((((uintptr_t)Y) & 15u) == 0 && (((uintptr_t)w_packed) & 15u) == 0, "stem_pool_image: Y and weights must be 16-byte aligned");
    if (N == 0) return KINET_OK;
    const long long ib = (long long)N * 3 * H * W * 4;
    KINET_CHECK_ARG(ib < (1LL << 31), "stem_pool_image: image batch larger than 2 GiB (split the call)");
    StemPoolArgs a{};
    a.img = img; a.W = w_packed; a.scale = scale; a.bias = bias; a.Y = Y;
    a.N = N; a.H = H; a.W_ = W; a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1;
    a.Hp = (a.Ho - 1) / 2 + 1; a.Wp = (a.Wo - 1) / 2 + 1;
    a.img_bytes = (int)ib;
    a.w_bytes = SK_CO * SK_KH * SK_CG * 2;
    a.strips = (a.Wp + SP_PQ - 1) / SP_PQ;
    a.tiles_y = (a.Ho + SK_RH - 1) / SK_RH;
    a.seg_tiles = seg_tiles > 0 ? (seg_tiles < a.tiles_y ? seg_tiles : a.tiles_y)
                                : stem_pool_seg_tiles(N, a.strips, a.tiles_y);
    const long long nu = (long long)N * a.strips * ((a.tiles_y + a.seg_tiles - 1) / a.seg_tiles);
    KINET_CHECK_ARG(nu < (1LL << 30), "stem_pool_image: too many work units");
    a.nunits = (int)nu;
    const int grid = nu < SP_GRID ? (int)nu : SP_GRID;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == KINET_BF16)
        hipLaunchKernelGGL((stem_pool_kernel<bf16_t>), dim3(grid), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((stem_pool_kernel<f16_t>), dim3(grid), dim3(256), 0, s, a);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}
