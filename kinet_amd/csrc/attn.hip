// Attention core on MFMA (gfx950): O = softmax(scale * Q K^T + mask) V per (frame, head), head_dim
// 32 or 36, bf16 / f16 -- nn.MultiheadAttention inside DeformableTransformerDecoderLayer
// (deformable_transformer.py:367-372: a few hundred object + track queries attending to each
// other) and vanilla DETR's dense attention over the feature map.
//
// One workgroup = 64 queries of one (frame, head), 4 waves x 16 queries.  Keys (row-major, padded
// rows: conflict-free fragment reads), values (TRANSPOSED, d-major) and the additive key bias are
// staged in LDS.  Per 32-key block (attn_block) a wave computes S^T = K Q^T (two 16x16x32 MFMAs
// per 32-deep K-step of the head dim), so each lane holds 8 scores of ONE query (lane & 15): the
// online softmax needs only in-lane math + two cross-lane steps, the exp(m_old - m_new) rescale is
// per lane, and the 8 probabilities rounded to the 16-bit type ARE the B operand of
// O^T += V^T P^T (K-slot order {4g..4g+3, 16+4g..16+4g+3}, matched by the two 8-byte reads of
// the transposed values).  Fully masked queries give 0, as the FMA kernel in ops.hip.
//
// Two kernels run that one block step: mha_resident_kernel (the head's keys staged once: Lk <= 384
// at head_dim 32, <= 640 at 36) and mha_stream_kernel (any Lk, keys streamed through LDS in
// tiles).  Head_dim 36 (d = 288, configs 3-5) pads the head dim to two K-steps (dims 36..63 zero in
// the staged keys and in the query fragments) and to three 16-row tiles of O^T (V^T rows 36..47
// zero); its rows are 8-byte aligned only, so global reads / writes move 8-byte pieces.  Which
// kernel a call runs, its grid and its LDS: attn_plan.h.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/kinet_ops.h"
#include "attn_plan.h"
#include "common.h"
#include "gemm_common.h"

namespace kinet {
namespace {

template <int D>
struct AttnCfg {
    static constexpr AttnGeo G = attn_geo(D);
    static constexpr int KROW = G.krow, KSTEPS = G.ksteps, VT = G.vt, PPR = G.ppr, PE = G.piece_bytes / 2, MAXK = G.maxk;
    typedef std::conditional_t<G.piece_bytes == 16, u32x4, uint2> Piece;   // one global piece of a row
    static constexpr int PADP = (KSTEPS * 32 - D) / 4;   // 8-byte pieces of a staged key row's zero pad
    static_assert(G.d == D && PPR * PE == D && sizeof(Piece) == G.piece_bytes, "a row is PPR whole pieces");
    static_assert(KSTEPS * 32 >= D && KROW >= KSTEPS * 32 && (KROW * 2) % 16 == 0, "K-steps inside the staged key row");
    static_assert(VT * 16 >= D && D % 4 == 0, "O^T tiles cover the head dim, stored 4 dims at a time");
};

constexpr int ST_KT = kAttnStreamKT;   // keys per tile
constexpr int ST_VLD = ST_KT + 8;      // transposed value row (elements)
static_assert(kAttnQueries == 64 && kAttnBlock == 256 && ST_KT % 32 == 0 && ST_KT <= kAttnBlock,
              "4 waves x 16 queries; a tile is whole blocks, one mask byte per thread");

// Dims 32s + 8g .. +7 of query row qr as this lane's part of the B operand of S^T (the wave's 16
// queries: lane holds query c16); a dead query and the dims past D are zero.
template <typename T, int D>
__device__ __forceinline__ u32x4 attn_q_frag(const T* qr, bool qok, int g, int s) {
    if (!qok) return u32x4{0u, 0u, 0u, 0u};
    if constexpr (AttnCfg<D>::PE == 8) {
        return *reinterpret_cast<const u32x4*>(qr + 8 * g);
    } else {
        if (s == 0) {
            const uint2 a = *reinterpret_cast<const uint2*>(qr + 8 * g), c = *reinterpret_cast<const uint2*>(qr + 8 * g + 4);
            return u32x4{a.x, a.y, c.x, c.y};
        }
        if (g != 0) return u32x4{0u, 0u, 0u, 0u};
        const uint2 t = *reinterpret_cast<const uint2*>(qr + 32);
        return u32x4{t.x, t.y, 0u, 0u};
    }
}

// The pads no staging store touches: key dims D .. 32 KSTEPS - 1 of n staged rows and value rows
// D .. 16 VT - 1 of width vld.  Nothing to do at head_dim 32.
template <typename T, int D>
__device__ __forceinline__ void attn_zero_pads(T* ks, int n, T* vt, int vld, int tid) {
    typedef AttnCfg<D> C;
    if constexpr (C::PADP > 0) {
        for (int i = tid; i < n * C::PADP; i += 256) {
            const int k = i / C::PADP, part = i - k * C::PADP;
            *reinterpret_cast<uint2*>(ks + k * C::KROW + D + part * 4) = uint2{0u, 0u};
        }
        for (int i = tid; i < (C::VT * 16 - D) * vld; i += 256) vt[D * vld + i] = Cvt<T>::from(0.f);
    }
}

// One 32-key block of the online softmax.  kp: the block's first staged key row, vp: its column
// of the transposed values (rows of vld elements), bp: its key bias.  m / l / o: the running max,
// sum and O^T[d = 16t + 4g + i][query c16] of this lane's query.  PAD: end with the two wait
// states that cover the caller's loop back edge (common.h mfma_window_pad).
template <typename T, int D, bool PAD = true>
__device__ __forceinline__ void attn_block(const T* kp, const T* vp, const float* bp, int vld,
                                           const u32x4 (&qf)[AttnCfg<D>::KSTEPS], float scale, int g, int c16,
                                           float& m, float& l, f32x4 (&o)[AttnCfg<D>::VT]) {
    typedef AttnCfg<D> C;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    {
        const T* r0 = kp + c16 * C::KROW + 8 * g;
        const T* r1 = kp + (16 + c16) * C::KROW + 8 * g;
#pragma unroll
        for (int s = 0; s < C::KSTEPS; ++s) {
            Mma<T>::run(s0, *reinterpret_cast<const u32x4*>(r0 + 32 * s), qf[s]);   // S^T[key 4g + i][query c16]
            Mma<T>::run(s1, *reinterpret_cast<const u32x4*>(r1 + 32 * s), qf[s]);   // S^T[key 16 + 4g + i][query c16]
        }
    }
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp + 4 * g);
    const f32x4 b1 = *reinterpret_cast<const f32x4*>(bp + 16 + 4 * g);
    float sv[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sv[i] = s0[i] * scale + b0[i];
        sv[4 + i] = s1[i] * scale + b1[i];
    }
    float bm = sv[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) bm = fmaxf(bm, sv[i]);
    bm = fmaxf(bm, __shfl_xor(bm, 16));
    bm = fmaxf(bm, __shfl_xor(bm, 32));
    const float mn = fmaxf(m, bm);
    const float alpha = mn == -INFINITY ? 1.f : __expf(m - mn);
    float p[8], ps = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        p[i] = mn == -INFINITY ? 0.f : __expf(sv[i] - mn);
        ps += p[i];
    }
    ps += __shfl_xor(ps, 16);
    ps += __shfl_xor(ps, 32);
    l = l * alpha + ps;
    m = mn;
    u32x4 pb;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        pb[i] = (uint32_t)__builtin_bit_cast(uint16_t, Cvt<T>::from(p[2 * i])) |
                ((uint32_t)__builtin_bit_cast(uint16_t, Cvt<T>::from(p[2 * i + 1])) << 16);
    // A operand: V^T rows d = 16t + c16, K slots 8g + j -> keys 4g + j (j < 4) and
    // 16 + 4g + (j - 4): two 8-byte reads of the transposed values
#pragma unroll
    for (int t = 0; t < C::VT; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[t][i] *= alpha;
        const T* r = vp + (16 * t + c16) * vld + 4 * g;
        const uint2 a0 = *reinterpret_cast<const uint2*>(r), a1 = *reinterpret_cast<const uint2*>(r + 16);
        Mma<T>::run(o[t], u32x4{a0.x, a0.y, a1.x, a1.y}, pb);
    }
    if constexpr (PAD) mfma_window_pad<2>();   // the next block's rescale reads o[] across the back edge
}

// O[query][4g + 16t .. +3] = O^T / l (0 for a query with no live key); orow: the query's head + 4g
template <typename T, int D>
__device__ __forceinline__ void attn_store(T* orow, const f32x4 (&o)[AttnCfg<D>::VT], float l, int g) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int t = 0; t < AttnCfg<D>::VT; ++t) {
        if (16 * t + 4 * g >= D) continue;
        uint32_t w[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
            w[i] = (uint32_t)__builtin_bit_cast(uint16_t, Cvt<T>::from(o[t][2 * i] * inv)) |
                   ((uint32_t)__builtin_bit_cast(uint16_t, Cvt<T>::from(o[t][2 * i + 1] * inv)) << 16);
        *reinterpret_cast<uint2*>(orow + 16 * t) = uint2{w[0], w[1]};
    }
}

// The head's keys resident in LDS: [Lkp][KROW] keys | [16 VT][Lkp + 8] transposed values | [Lkp]
// bias, Lkp = Lk rounded up to whole blocks (attn_resident_lds).
template <typename T, int D>
__global__ __launch_bounds__(256) void mha_resident_kernel(const T* __restrict__ Q, int ldq, const T* __restrict__ Kt,
                                                           int ldk, const T* __restrict__ V, int ldv, T* __restrict__ O,
                                                           int ldo, int Lq, int Lk, float scale,
                                                           const uint8_t* __restrict__ kmask) {
    typedef AttnCfg<D> C;
    typedef typename C::Piece Piece;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Lkp = (Lk + 31) & ~31;
    const int vld = Lkp + 8;
    T* ks = reinterpret_cast<T*>(smem);
    T* vt = ks + Lkp * C::KROW;
    float* kb = reinterpret_cast<float*>(vt + C::VT * 16 * vld);
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c16 = lane & 15;

    // stage keys / transposed values / key bias (keys past Lk: zero rows, -inf bias)
    for (int i = tid; i < Lkp * C::PPR; i += 256) {
        const int k = i / C::PPR, part = i - k * C::PPR;
        Piece kv = Piece{}, vv = Piece{};
        if (k < Lk) {
            kv = *reinterpret_cast<const Piece*>(Kt + ((long)b * Lk + k) * ldk + h * D + part * C::PE);
            vv = *reinterpret_cast<const Piece*>(V + ((long)b * Lk + k) * ldv + h * D + part * C::PE);
        }
        *reinterpret_cast<Piece*>(ks + k * C::KROW + part * C::PE) = kv;
        const T* ve = reinterpret_cast<const T*>(&vv);
#pragma unroll
        for (int j = 0; j < C::PE; ++j) vt[(part * C::PE + j) * vld + k] = ve[j];
    }
    attn_zero_pads<T, D>(ks, Lkp, vt, vld, tid);
    for (int k = tid; k < Lkp; k += 256)
        kb[k] = (k < Lk && !(kmask && kmask[(long)b * Lk + k])) ? 0.f : -INFINITY;

    const int q = blockIdx.x * 64 + wave * 16 + c16;
    const bool qok = q < Lq;
    u32x4 qf[C::KSTEPS];
#pragma unroll
    for (int s = 0; s < C::KSTEPS; ++s) qf[s] = attn_q_frag<T, D>(Q + ((long)b * Lq + q) * ldq + h * D, qok, g, s);
    __syncthreads();

    f32x4 o[C::VT];
#pragma unroll
    for (int t = 0; t < C::VT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    // no pad at head_dim 36, as before the kernels were merged: with three O^T tiles the scan finds
    // no short window across this back edge (tools/mfma_hazard_check.py), and the pad's scheduling
    // barriers cost this loop 4 % ("Key-streaming attention")
    for (int k0 = 0; k0 < Lkp; k0 += 32)
        attn_block<T, D, D == 32>(ks + k0 * C::KROW, vt + k0, kb + k0, vld, qf, scale, g, c16, m, l, o);
    if (qok) attn_store<T, D>(O + ((long)b * Lq + q) * ldo + h * D + 4 * g, o, l, g);
}

// Key-streaming form for any Lk (vanilla DETR attends densely over the stride-32 feature map:
// 1050 keys at 800x1333, encoder self-attention and decoder cross-attention).  Same workgroup and
// the same block step; the keys, transposed values and key bias live in LDS one ST_KT-key tile
// at a time, in two buffers: the global loads of tile t+1 are issued into registers before the
// MFMAs of tile t and written to the other buffer after them (the transposed value layout and
// the padded key rows rule out LDS-DMA, which lands a wave's 1 KiB contiguously), one barrier
// per tile.  A buffer is 19456 B at head_dim 32 (4 workgroups per CU) and 32000 B at head_dim 36
// (2 per CU).  The running max / sum / O^T accumulators carry across tiles exactly as across the
// 32-key blocks of a resident head, so a tile whose keys are all masked leaves them untouched.
template <typename T, int D>
__global__ __launch_bounds__(256) void mha_stream_kernel(const T* __restrict__ Q, int ldq, const T* __restrict__ Kt,
                                                         int ldk, const T* __restrict__ V, int ldv, T* __restrict__ O,
                                                         int ldo, int Lq, int Lk, float scale,
                                                         const uint8_t* __restrict__ kmask) {
    typedef AttnCfg<D> C;
    typedef typename C::Piece Piece;
    constexpr int KS_ELEMS = ST_KT * C::KROW, VT_ELEMS = C::VT * 16 * ST_VLD;
    constexpr int BUF = attn_staged_lds(C::G, ST_KT);
    constexpr int NPIECE = ST_KT * C::PPR, NP = (NPIECE + 255) / 256;
    static_assert(BUF == KS_ELEMS * 2 + VT_ELEMS * 2 + ST_KT * 4, "the plan's tile buffer is [ks | vt | kb]");
    static_assert(BUF % 16 == 0 && (KS_ELEMS * 2) % 16 == 0 && (VT_ELEMS * 2) % 16 == 0, "tile buffer alignment");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // two buffers: [ks | vt | kb]
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c16 = lane & 15;
    const int Lkp = (Lk + 31) & ~31;
    const T* kbase = Kt + (long)b * Lk * ldk + h * D;
    const T* vbase = V + (long)b * Lk * ldv + h * D;

    // register stage of one tile: this thread's key / value pieces and (tid < ST_KT) key mask
    // byte, all left untouched until store_tile so the loads stay in flight; keys past Lk: zero
    // rows, -inf bias
    Piece kr[NP], vr[NP];
    uint8_t mr = 1;
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i = tid + j * 256, k = i / C::PPR, part = i - k * C::PPR;
            kr[j] = Piece{};
            vr[j] = Piece{};
            if (i < NPIECE && k0 + k < Lk) {
                kr[j] = *reinterpret_cast<const Piece*>(kbase + (long)(k0 + k) * ldk + part * C::PE);
                vr[j] = *reinterpret_cast<const Piece*>(vbase + (long)(k0 + k) * ldv + part * C::PE);
            }
        }
        if (tid < ST_KT) {
            const int k = k0 + tid;
            mr = 1;
            if (k < Lk) mr = kmask ? kmask[(long)b * Lk + k] : 0;
        }
    };
    auto store_tile = [&](char* buf) {
        T* ks = reinterpret_cast<T*>(buf);
        T* vt = ks + KS_ELEMS;
        float* kb = reinterpret_cast<float*>(vt + VT_ELEMS);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i = tid + j * 256, k = i / C::PPR, part = i - k * C::PPR;
            if (i < NPIECE) {
                *reinterpret_cast<Piece*>(ks + k * C::KROW + part * C::PE) = kr[j];
                const T* ve = reinterpret_cast<const T*>(&vr[j]);
#pragma unroll
                for (int e = 0; e < C::PE; ++e) vt[(part * C::PE + e) * ST_VLD + k] = ve[e];
            }
        }
        if (tid < ST_KT) kb[tid] = mr ? -INFINITY : 0.f;
    };

    load_tile(0);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        T* ks = reinterpret_cast<T*>(smem + s * BUF);
        attn_zero_pads<T, D>(ks, ST_KT, ks + KS_ELEMS, ST_VLD, tid);
    }
    store_tile(smem);

    const int q = blockIdx.x * 64 + wave * 16 + c16;
    const bool qok = q < Lq;
    const bool wlive = blockIdx.x * 64 + wave * 16 < Lq;   // wave-uniform: any live query
    u32x4 qf[C::KSTEPS];
#pragma unroll
    for (int s = 0; s < C::KSTEPS; ++s) qf[s] = attn_q_frag<T, D>(Q + ((long)b * Lq + q) * ldq + h * D, qok, g, s);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < C::KSTEPS; ++s)
        asm volatile("" ::"v"(qf[s]));   // the query load lands here, not at its first MFMA inside the loop

    f32x4 o[C::VT];
#pragma unroll
    for (int t = 0; t < C::VT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    int cur = 0;
    for (int k0 = 0; k0 < Lkp; k0 += ST_KT, cur ^= 1) {
        const bool more = k0 + ST_KT < Lkp;
        if (more) load_tile(k0 + ST_KT);   // in flight during this tile's MFMAs
        if (wlive) {
            const T* ks = reinterpret_cast<const T*>(smem + cur * BUF);
            const T* vt = ks + KS_ELEMS;
            const float* kb = reinterpret_cast<const float*>(vt + VT_ELEMS);
            const int kend = min(ST_KT, Lkp - k0);
            for (int kk = 0; kk < kend; kk += 32)
                attn_block<T, D>(ks + kk * C::KROW, vt + kk, kb + kk, ST_VLD, qf, scale, g, c16, m, l, o);
        }
        if (more) store_tile(smem + (cur ^ 1) * BUF);   // last read before the previous barrier
        __syncthreads();
    }
    if (qok) attn_store<T, D>(O + ((long)b * Lq + q) * ldo + h * D + 4 * g, o, l, g);
}

template <typename T, int D>
void launch(const AttnPlan& pl, const void* Q, int ldq, const void* Kt, int ldk, const void* V, int ldv, void* O, int ldo,
            int Lq, int Lk, float scale, const uint8_t* key_mask, hipStream_t stream) {
    const auto kernel = pl.kernel == ATTN_K_STREAM ? mha_stream_kernel<T, D> : mha_resident_kernel<T, D>;
    hipLaunchKernelGGL(kernel, dim3(pl.grid[0], pl.grid[1], pl.grid[2]), dim3(pl.block), pl.lds, stream, (const T*)Q, ldq,
                       (const T*)Kt, ldk, (const T*)V, ldv, (T*)O, ldo, Lq, Lk, scale, key_mask);
}

}  // namespace

// Entry from kinet_mha_core (ops.hip): run the MFMA kernel attn_plan() named (ATTN_K_RESIDENT /
// ATTN_K_STREAM, so 16-bit and head_dim 32 / 36) with the plan's grid and LDS.
void launch_mha_mfma(const AttnPlan& pl, const void* Q, int ldq, const void* Kt, int ldk, const void* V, int ldv, void* O,
                     int ldo, int Lq, int Lk, int head_dim, float scale, int dtype, const uint8_t* key_mask,
                     hipStream_t stream) {
#define KINET_ATTN_LAUNCH(T, D) launch<T, D>(pl, Q, ldq, Kt, ldk, V, ldv, O, ldo, Lq, Lk, scale, key_mask, stream)
    if (head_dim == 32) {
        if (dtype == KINET_BF16) KINET_ATTN_LAUNCH(bf16_t, 32);
        else KINET_ATTN_LAUNCH(f16_t, 32);
    } else {
        if (dtype == KINET_BF16) KINET_ATTN_LAUNCH(bf16_t, 36);
        else KINET_ATTN_LAUNCH(f16_t, 36);
    }
#undef KINET_ATTN_LAUNCH
}

}  // namespace kinet
