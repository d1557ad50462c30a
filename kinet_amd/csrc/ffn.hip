// Fused post-norm FFN sub-layer for gfx950: y = LN(x + W2 relu(W1 x + b1) + b2), one launch.
//
// Reference: DeformableTransformerEncoderLayer.forward_ffn (deformable_transformer.py:284-288)
// and the decoder twin (:361-365) -- two GEMMs whose (M, F) hidden tensor (F = 1024, i.e. 4x
// the activations) is written to and re-read from HBM.  Here it never leaves the CU:
//
//  * each wave owns 16*RT rows of x, held for the whole launch in VGPRs as MFMA B-operand
//    fragments (lane l: row l&15, 8 consecutive k);
//  * the weights stream through a 2-slot LDS ring, one 32-unit hidden chunk per slot
//    (W1 rows + W2 columns, pre-packed fragment-major by kinet_ffn_pack so one LDS-DMA
//    wave-instruction moves one 1-KiB operand fragment and every ds_read_b128 is a linear,
//    conflict-free 1 KiB); all waves of the workgroup share the ring;
//  * phase A: H^T(32 x rows) = W1c x^T on v_mfma_f32_16x16x32 -- the accumulator layout
//    puts 4 consecutive hidden units of one row in each lane;  + b1, ReLU, round to the
//    16-bit type: that IS the B operand of phase B once W2's hidden index is permuted the
//    same way (done in the pack), so H goes register -> MFMA with no LDS round trip;
//  * phase B: out^T(D x rows) += W2c H^T, accumulated over the F/32 chunks in VGPRs;
//  * epilogue in registers: + b2 + residual x (re-read, L2-hot), LayerNorm over the row
//    (each row's D outputs live in 4 lanes: in-lane sums + 2 cross-lane steps), 8-byte
//    stores.
// One barrier per chunk: wait own DMA -> barrier -> issue the next chunk's DMA into the
// slot everyone just finished -> compute.  Arithmetic intensity per workgroup = its row
// count (each weight byte feeds 16*RT*WAVES rows), 256 rows at D = 256.
#include <hip/hip_runtime.h>

#include "../../include/kinet_ffn.h"
#include "common.h"
#include "ffn_plan.h"
#include "ffn_sched.h"
#include "gemm_common.h"

namespace kinet {
namespace {

struct FfnArgs {
    const void* X;
    const void* W;
    const float* b1;
    const float* b2;
    const float* ln_g;
    const float* ln_b;
    void* Y;
    float eps;
    int ldx, ldy, M, F;
    int x_bytes, w_bytes, y_bytes;
    int dbg;   // FfnDebug bits of the calling thread (ffn_plan.h); the kernels read FFN_DBG_NO_DMA
    // kinet_attn_out_ffn_fused only (ffn_fused_rt2_kernel<.., PRE>): x = LN1(R + A Wo^T + bo)
    const void* A;   // attention output (M, D), row stride lda
    const void* R;   // residual (M, D), row stride ldr
    const float* bo;
    const float* g1;
    const float* be1;
    float eps1;
    int lda, ldr, a_bytes, r_bytes;
};

thread_local int ffn_debug = 0;    // test-only knobs (kinet_ffn_set_debug, FfnDebug), per calling thread
thread_local int ffn_cap = 0;      // kinet_ffn_grid_cap (0 = no cap), per calling thread
thread_local int ffn_last = -1;    // kFfnKernels index of the calling thread's last launch (kinet_ffn_last_kernel)

// the table entry of an instantiation (ffn_plan.h): each kernel checks its tile and its LDS against it
template <int FAMILY, int D, int RT, int WAVES, int DB = 0, bool PRE = false, int RV = 0>
constexpr FfnKernel ffn_entry() {
    constexpr int i = ffn_kernel_index(FAMILY, D, RT, WAVES, DB, PRE, RV);
    static_assert(i >= 0, "an instantiation the table does not list");
    return kFfnKernels[i];
}
template <int LDS, int ROWS, int NS>
constexpr bool ffn_entry_is(const FfnKernel k) {
    return ffn_kernel_lds(k) == LDS && LDS * k.wg_per_cu <= kFfnLdsLimit && k.tile_rows == ROWS && k.ns == NS;
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// two floats rounded (nearest even, NaN stays NaN: f32_to_bf16's cast) into one 32-bit word, a in
// the low half: the 2-vector conversion is ONE v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 d, a, b; two
// scalar casts glued with a shift and an or were four instructions per word
template <typename T>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    const f32x2 v{a, b};
    if constexpr (std::is_same<T, bf16_t>::value) {
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
    } else {
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
    }
}

template <typename T>
__device__ __forceinline__ void unpack4(u32x2 u, float* v) {
    if constexpr (std::is_same<T, bf16_t>::value) {
        v[0] = __uint_as_float(u[0] << 16); v[1] = __uint_as_float(u[0] & 0xffff0000u);
        v[2] = __uint_as_float(u[1] << 16); v[3] = __uint_as_float(u[1] & 0xffff0000u);
    } else {
        v[0] = (float)__builtin_bit_cast(f16_t, (uint16_t)(u[0] & 0xffffu));
        v[1] = (float)__builtin_bit_cast(f16_t, (uint16_t)(u[0] >> 16));
        v[2] = (float)__builtin_bit_cast(f16_t, (uint16_t)(u[1] & 0xffffu));
        v[3] = (float)__builtin_bit_cast(f16_t, (uint16_t)(u[1] >> 16));
    }
}

// 16-byte pieces of an accumulator chunk row: lane group g holds hidden 4g..4g+3 (a, 2 packed
// words) and 16+4g..16+4g+3 (b).  One v_permlane16_swap per word exchanges between lane groups
// g and g^1 so that even g hold hidden 4g..4g+7 and odd g hold 4g+12..4g+19 (contiguous 8
// each: a row's 64 bytes in four 16-byte lanes); chunk_piece_off is that piece's first hidden
// index.  The swap is its own inverse (residual loads take the same route back).
__device__ __forceinline__ u32x4 chunk_swap(u32x2 a, u32x2 b) {
    const auto s0 = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
    const auto s1 = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
    return u32x4{s0[0], s1[0], s0[1], s1[1]};
}
__device__ __forceinline__ int chunk_piece_off(int g) { return (g & 1) ? 4 * g + 12 : 4 * g; }

template <int N>
__device__ __forceinline__ void ffn_wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// raw workgroup barrier for LDS traffic only: LDS-DMA issued earlier stays in flight
__device__ __forceinline__ void ffn_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// dma16 with a wave-uniform part of the source offset in an SGPR
__device__ __forceinline__ void dma16s(__amdgpu_buffer_rsrc_t r, char* dst, unsigned voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)dst, 16, voff, soff, 0, 0);
}

template <typename T, int D, int RT, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void ffn_fused_kernel(const FfnArgs p, const int ntiles) {
    using G = FfnGeo<D>;
    constexpr int KS = G::KS, NT = G::NT, FR = G::FR;
    static_assert(FR % WAVES == 0, "whole DMA rounds per chunk");
    constexpr int FRW = FR / WAVES;          // LDS-DMA instructions per wave per chunk
    constexpr int XN = RT * KS;              // x-fragment loads per wave per tile
    constexpr int NST = RT * NT / 2;         // 16-byte stores per wave per tile
    static_assert(XN == NST, "one extra-count class");
    constexpr int ROWS = WAVES * 16 * RT;
    constexpr int NS = 4;                    // ring slots: 2 chunks in flight, the chunk in phase A,
                                             // the previous chunk in phase B
    constexpr unsigned OOB = 0x80000000u;
    constexpr int PAR = (FFN_MAX_F + 3 * D) * 4;
    __shared__ __attribute__((aligned(16))) char lds[PAR + NS * G::CHUNK];
    static_assert(ffn_entry_is<sizeof(lds), ROWS, NS>(ffn_entry<FFN_K_FUSED, D, RT, WAVES>()), "ffn_plan.h");
    float* const pb1 = reinterpret_cast<float*>(lds);
    float* const pb2 = pb1 + FFN_MAX_F;
    float* const pg = pb2 + D;
    float* const pbe = pg + D;
    char* const ring = lds + PAR;

    const int P = gridDim.x, bx = blockIdx.x;
    const int cnt = bx < ntiles ? (ntiles - 1 - bx) / P + 1 : 0;
    if (cnt == 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    const int nch = p.F / 32, pfi = nch / 2;
    const bool ln = p.ln_g != nullptr;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, (short)0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, (short)0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.Y, (short)0, p.y_bytes, 0x00020000);

    for (int i = threadIdx.x; i < p.F; i += WAVES * 64) pb1[i] = p.b1[i];
    for (int i = threadIdx.x; i < D; i += WAVES * 64) {
        pb2[i] = p.b2[i];
        pg[i] = ln ? p.ln_g[i] : 1.f;
        pbe[i] = ln ? p.ln_b[i] : 0.f;
    }

    auto load_x = [&](int tile, u32x4 (&dst)[RT][KS]) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int r = tile * ROWS + wave * 16 * RT + 16 * rt + c16;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const unsigned off = r < p.M ? ((unsigned)r * (unsigned)p.ldx + (unsigned)(32 * ks + 8 * g)) * 2u : OOB;
                dst[rt][ks] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
            }
        }
    };
    // global chunk q of this workgroup (hidden chunk c = q mod nch, passed in: a runtime
    // modulo is a ~20-instruction scalar division) -> ring slot q % NS; wave w moves
    // fragments w, w+WAVES, ..
    auto dma_chunk = [&](int q, int c) {
        char* dst = ring + (q % NS) * G::CHUNK;
        const unsigned src = (unsigned)c * (unsigned)G::CHUNK + (unsigned)lane * 16u;
#pragma unroll
        for (int k = 0; k < FRW; ++k) {
            const int f = k * WAVES + wave;
            dma16(rw, dst + f * 1024, src + (unsigned)f * 1024u);
        }
    };
    // VMEM ops a wave issues in chunk iteration (tile t, chunk c) AFTER that iteration's DMA
    // (x prefetch, epilogue stores): they are younger than the DMA of the next two chunks.
    // Every per-chunk index here is wave-uniform scalar work shared by all waves of the CU
    // (one SALU issue per cycle per CU), so no divisions: the caller steps (t, c) back itself.
    auto extra = [&](int c, int t) {
        if (t < 0) return 0;
        return ((c == pfi && t + 1 < cnt) ? XN : 0) + (c == nch - 1 ? NST : 0);
    };

    u32x4 xr[RT][KS], xn[RT][KS];
    load_x(bx, xr);
    __syncthreads();   // parameters in LDS (drains the x loads too: nothing else in flight yet)
    const int total = cnt * nch;
    dma_chunk(0, 0);
    if (total > 1) dma_chunk(1, nch > 1 ? 1 : 0);

    f32x4 acc[RT][NT];
    constexpr int PB = 4;                      // W2 fragments read ahead of phase B
    auto fragA = [&](const char* slot, int ks, int h) {
        return *reinterpret_cast<const u32x4*>(slot + lane * 16 + (h * KS + ks) * 1024);
    };
    auto fragB = [&](const char* slot, int nt) {
        return *reinterpret_cast<const u32x4*>(slot + lane * 16 + (2 * KS + nt) * 1024);
    };
    // ReLU + round one 32-bit word (2 hidden units) of row tile w/4's phase-B operand: lane
    // holds H[row l&15][4g+i] (h0) and [16+4g+i] (h1) = the 8 K slots of the operand in the
    // order kinet_ffn_pack permuted W2 to
    auto hword = [&](const f32x4 (&q0)[RT], const f32x4 (&q1)[RT], int w) {
        const int rt = w >> 2, i = w & 3;
        const f32x4& src = i < 2 ? q0[rt] : q1[rt];
        const int e = 2 * (i & 1);
        return pack2<T>(fmaxf(src[e], 0.f), fmaxf(src[e + 1], 0.f));
    };
    // phase B of one chunk: out[row l&15][sigma(nt, 4g+i)] += W2c . H^T; fw[0..PB) preloaded
    auto phase_b = [&](const char* slot, u32x4 (&fw)[PB + 1], const u32x4 (&hb)[RT]) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if (nt + PB < NT) fw[(nt + PB) % (PB + 1)] = fragB(slot, nt + PB);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) Mma<T>::run(acc[rt][nt], fw[nt % (PB + 1)], hb[rt]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    for (int ti = 0; ti < cnt; ++ti) {
    // consume the x fragments HERE (hipcc places the wait for their loads before this
    // statement, once per tile) so no vmcnt wait of the compiler's lands inside the chunk
    // loop, where it would retire the ring's DMA early
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" ::"v"(xr[rt][ks]));
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // Software pipeline over the hidden chunks: iteration c runs phase A of chunk c with the
    // ReLU/convert of chunk c-1 spread over its steps (VALU beside MFMA), then phase B of
    // chunk c-1; the tile's last chunk gets its phase B after the loop.  Operand fragments are
    // read from the ring two steps ahead and the steps are fenced with sched_barrier: with one
    // wave per SIMD nothing else hides LDS latency, and hipcc otherwise sinks every ds_read
    // next to its MFMA.
    f32x4 hp0[RT], hp1[RT];
    const char* wprev = ring;
    for (int c = 0; c < nch; ++c) {
        const int q = ti * nch + c;
        // retire chunk q: still allowed in flight = everything issued after its DMA
        if (q + 1 < total) {
            int c1 = c - 1, t1 = ti, c2 = c - 2, t2 = ti;
            if (c1 < 0) { c1 += nch; --t1; }
            if (c2 < 0) { c2 += nch; --t2; }
            if (c2 < 0) { c2 += nch; --t2; }   // nch == 1
            const int e = extra(c2, t2) + extra(c1, t1);
            if (p.dbg & 1) ffn_wait_vmcnt<0>();
            else if (e == 0) ffn_wait_vmcnt<FRW>();
            else ffn_wait_vmcnt<FRW + XN>();   // XN == NST; e == 2 XN only waits more
        } else {
            ffn_wait_vmcnt<0>();
        }
        ffn_lds_barrier();     // chunk q visible to all; slot (q+2)%NS free (chunk q-2 done)
        if (q + 2 < total && !(p.dbg & 1)) {
            int cn = c + 2;
            if (cn >= nch) cn -= nch;
            if (cn >= nch) cn -= nch;       // nch == 1
            dma_chunk(q + 2, cn);
        }
        if (c == pfi && ti + 1 < cnt) load_x(bx + (ti + 1) * P, xn);
        const char* wb = ring + (q % NS) * G::CHUNK;
        const bool pipe = c > 0;
        f32x4 h0[RT], h1[RT];
        {
            const f32x4 bb0 = *reinterpret_cast<const f32x4*>(pb1 + c * 32 + 4 * g);
            const f32x4 bb1 = *reinterpret_cast<const f32x4*>(pb1 + c * 32 + 16 + 4 * g);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {   // b1 folded into the accumulator init
                h0[rt] = bb0;
                h1[rt] = bb1;
            }
        }
        u32x4 fa[3][2], fw[PB + 1], hb[RT];
        fa[0][0] = fragA(wb, 0, 0); fa[0][1] = fragA(wb, 0, 1);
        fa[1][0] = fragA(wb, 1, 0); fa[1][1] = fragA(wb, 1, 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + 2 < KS) {
                fa[(ks + 2) % 3][0] = fragA(wb, ks + 2, 0);
                fa[(ks + 2) % 3][1] = fragA(wb, ks + 2, 1);
            } else if (pipe) {
#pragma unroll
                for (int j = 0; j < PB / 2; ++j) {
                    const int nt = (ks + 2 - KS) * (PB / 2) + j;
                    fw[nt] = fragB(wprev, nt);
                }
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                Mma<T>::run(h0[rt], fa[ks % 3][0], xr[rt][ks]);
                Mma<T>::run(h1[rt], fa[ks % 3][1], xr[rt][ks]);
            }
            if (pipe && ks < 4 * RT) hb[ks >> 2][ks & 3] = hword(hp0, hp1, ks);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (pipe) {
#pragma unroll
            for (int w = KS; w < 4 * RT; ++w) hb[w >> 2][w & 3] = hword(hp0, hp1, w);
            phase_b(wprev, fw, hb);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            hp0[rt] = h0[rt];
            hp1[rt] = h1[rt];
        }
        wprev = wb;
    }
    {   // phase B of the tile's last chunk (its slot is still held: the next DMA into it is
        // issued only after the next iteration's barrier)
        u32x4 fw[PB + 1], hb[RT];
#pragma unroll
        for (int j = 0; j < PB; ++j) fw[j] = fragB(wprev, j);
#pragma unroll
        for (int w = 0; w < 4 * RT; ++w) hb[w >> 2][w & 3] = hword(hp0, hp1, w);
        phase_b(wprev, fw, hb);
    }

        // ---- tile epilogue, registers only: + b2 + residual x (= xr), LayerNorm, store ----
        const int tile = bx + ti * P;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int r = tile * ROWS + wave * 16 * RT + 16 * rt + c16;
            float s = 0.f;
#pragma unroll
            for (int kp = 0; kp < KS; ++kp) {
                float x8[8];
                unpack4<T>(u32x2{xr[rt][kp][0], xr[rt][kp][1]}, x8);
                unpack4<T>(u32x2{xr[rt][kp][2], xr[rt][kp][3]}, x8 + 4);
                const f32x4 b2a = *reinterpret_cast<const f32x4*>(pb2 + 32 * kp + 8 * g);
                const f32x4 b2b = *reinterpret_cast<const f32x4*>(pb2 + 32 * kp + 8 * g + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v0 = acc[rt][2 * kp][i] + b2a[i] + x8[i];
                    const float v1 = acc[rt][2 * kp + 1][i] + b2b[i] + x8[4 + i];
                    acc[rt][2 * kp][i] = v0;
                    acc[rt][2 * kp + 1][i] = v1;
                    s += v0 + v1;
                }
            }
            float mean = 0.f, rstd = 1.f;
            if (ln) {
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                mean = s * (1.f / (float)D);
                float qv = 0.f;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float d = acc[rt][nt][i] - mean;
                        qv += d * d;
                    }
                qv += __shfl_xor(qv, 16);
                qv += __shfl_xor(qv, 32);
                rstd = rsqrtf(qv * (1.f / (float)D) + p.eps);
            }
#pragma unroll
            for (int kp = 0; kp < KS; ++kp) {
                const int n0 = 32 * kp + 8 * g;
                float o[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    o[i] = acc[rt][2 * kp][i];
                    o[4 + i] = acc[rt][2 * kp + 1][i];
                }
                if (ln) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = (o[e] - mean) * rstd * pg[n0 + e] + pbe[n0 + e];
                }
                u32x4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = pack2<T>(o[2 * e], o[2 * e + 1]);
                // unconditional (OOB rows dropped by the range check): the store count per
                // tile is fixed, which the counted vmcnt above relies on
                const unsigned off = r < p.M ? ((unsigned)r * (unsigned)p.ldy + (unsigned)n0) * 2u : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, w), ry, off, 0, 0);
            }
        }
        if (ti + 1 < cnt) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) xr[rt][ks] = xn[rt][ks];
        }
    }
}

// 8 waves x 32 rows (two 16-row tiles per wave; the default at D = 256): every 1-KiB weight
// fragment read from the ring feeds two MFMAs -- half the LDS reads per MFMA of the 16-row tile,
// whose 8 waves saturate the LDS read port.  To stay within 256 VGPRs (two waves
// per SIMD) the tile's x fragments are loaded at the tile start instead of one tile ahead and the
// ring holds 3 chunks, staged and recycled by halves (W1 | W2).  The two waves of a SIMD take two
// roles (ffn_sched.h): waves 0-3 run a chunk's phase B behind its own phase A, waves 4-7 run it one
// chunk barrier later (hb kept in registers), so one role's ReLU / convert block and its wait for
// the first fragments fall beside the partner's MFMAs instead of beside the same stretch of the
// same program.  Same packed weights, same sums in the same order per output element as
// ffn_fused_kernel (bit-identical results).
//
// PRE (kinet_attn_out_ffn_fused): the attention out-projection and its post-norm run in front of
// the FFN on the same tile, x = LN1(R + A Wo^T + bo), so x is never written to or read from HBM.
// Wo travels through the ring as PCH chunks ahead of each tile's hidden chunks (fragment (ks, nt)
// = Wo[ffn_sigma(nt, .)][32 ks ..], ks-major: kinet_ffn_pack_attn); the products accumulate in
// acc, idle until phase B, in phase B's output layout -- the columns a lane holds of tile pair
// (2kp, 2kp+1) are the columns of its fragment xr[kp], so + bo + R, LayerNorm and pack2 leave x
// in xr as phase A's operand.  The A (samp) fragments sit in xr until their last MFMA; RV picks
// where the residual is loaded into the registers they free: 0 = all 2 KS after the last
// pre-chunk, 1 = fragments 2(u-1), 2(u-1)+1 at the start of pre-chunk u (their A fragments were
// last used by pre-chunk u-1), only the last pair after the last pre-chunk.
template <typename T, int D, bool PRE = false, int RV = 0>
__global__ __launch_bounds__(512) void ffn_fused_rt2_kernel(const FfnArgs p, const int ntiles) {
    constexpr int RT = 2, WAVES = 8;
    using G = FfnGeo<D>;
    constexpr int KS = G::KS, NT = G::NT, FR = G::FR;
    static_assert(FR % WAVES == 0, "whole DMA rounds per chunk");
    constexpr int FRW = FR / WAVES;
    static_assert(FRW % 2 == 0 && 2 * KS == FR / 2, "a chunk is staged as two halves: W1 | W2");
    constexpr int HW = FRW / 2;              // LDS-DMA instructions per wave per chunk half
    constexpr int ROWS = WAVES * 16 * RT;
    constexpr int NS = kFfnSchedSlots;
    static_assert(WAVES == 2 * kFfnSchedRoleSplit, "SIMD partners w, w + 4 take the two roles");
    constexpr unsigned OOB = 0x80000000u;
    constexpr int PCH = PRE ? KS * NT / FR : 0;   // Wo chunks per tile (FR fragments each)
    static_assert(!PRE || (KS * NT) % FR == 0, "Wo must fill whole ring chunks");
    static_assert(!PRE || (FR % NT == 0 && KS % (FR / NT) == 0), "whole k-steps per Wo chunk");
    constexpr int PAR = (FFN_MAX_F + (PRE ? 6 : 3) * D) * 4;
    __shared__ __attribute__((aligned(16))) char lds[PAR + NS * G::CHUNK];
    static_assert(ffn_entry_is<sizeof(lds), ROWS, NS>(ffn_entry<FFN_K_RT2, D, RT, WAVES, 0, PRE, RV>()), "ffn_plan.h");
    float* const pb1 = reinterpret_cast<float*>(lds);
    float* const pb2 = pb1 + FFN_MAX_F;
    float* const pg = pb2 + D;
    float* const pbe = pg + D;
    float* const pbo = pbe + D;      // PRE only: out-projection bias, LN1 gamma / beta
    float* const pg1 = pbo + D;
    float* const pbe1 = pg1 + D;
    char* const ring = lds + PAR;

    const int P = gridDim.x, bx = blockIdx.x;
    const int cnt = bx < ntiles ? (ntiles - 1 - bx) / P + 1 : 0;
    if (cnt == 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    const int nch = p.F / 32;
    const bool ln = p.ln_g != nullptr;
    // the tile's operand rows: x, or with PRE the attention output A
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(PRE ? p.A : p.X), (short)0,
                                                                        PRE ? p.a_bytes : p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, (short)0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.Y, (short)0, p.y_bytes, 0x00020000);
    const int ldx = PRE ? p.lda : p.ldx;

    for (int i = threadIdx.x; i < p.F; i += WAVES * 64) pb1[i] = p.b1[i];
    for (int i = threadIdx.x; i < D; i += WAVES * 64) {
        pb2[i] = p.b2[i];
        pg[i] = ln ? p.ln_g[i] : 1.f;
        pbe[i] = ln ? p.ln_b[i] : 0.f;
        if constexpr (PRE) {
            pbo[i] = p.bo[i];
            pg1[i] = p.g1[i];
            pbe1[i] = p.be1[i];
        }
    }
    // half `half` of chunk c of the packed stream ([PCH Wo chunks,] then the hidden chunks) -> its
    // half of ring slot q % NS (ffn_sched.h): fragments 16 half + wave, 16 half + 8 + wave
    auto dma_half = [&](int q, int c, int half) {
        char* dst = ring + ffn_sched_slot(q) * G::CHUNK;
        const unsigned src = (unsigned)c * (unsigned)G::CHUNK + (unsigned)lane * 16u;
#pragma unroll
        for (int k = 0; k < HW; ++k) {
            const int f = (half * HW + k) * WAVES + wave;
            if constexpr (PRE) {
                // the wave-uniform part of the source goes in the scalar offset: the unrolled Wo
                // chunks otherwise keep FRW loop-invariant vector addresses each (spilled)
                dma16s(rw, dst + f * 1024, (unsigned)lane * 16u, c * G::CHUNK + f * 1024);
            } else {
                dma16(rw, dst + f * 1024, src + (unsigned)f * 1024u);
            }
        }
    };
    const int ncht = nch + PCH;   // ring chunks per tile
    const int total = ffn_sched_total(cnt, PCH, nch);
    // The one barrier of chunk q, executed by every wave of either role exactly once per chunk: the
    // tile loop, the PCH pre-chunks and the nch hidden chunks have the same trip counts for all
    // waves (cnt, nch and PCH are workgroup-uniform) and each iteration calls this once, so every
    // wave executes ffn_sched_barriers() = cnt (PCH + nch) barriers; the roles differ only in the
    // MFMA work between two of them.  In front of the barrier the wave's DMA of both halves of
    // chunk q has landed: younger are at most LO of chunk q + 1 (HW operations) and EXTRA loads the
    // caller counts (at a tile boundary also the previous tile's stores and this tile's operand
    // loads -- then this waits for some of those too).  Behind it chunk q is visible to all, and
    // every wave has finished interval q - 1: HI of chunk q - 2 and LO of chunk q - 1 have had
    // their last reads, their half-slots take HI of chunk q + 1 and LO of chunk q + 2.
    // u = q's position in its tile's stream
    auto ring_step = [&](int q, int u, auto extra) {
        constexpr int EXTRA = decltype(extra)::value;
        constexpr int MID = ffn_sched_vmcnt(0, 2, HW), END = ffn_sched_vmcnt(0, 1, HW);   // a chunk follows / the last
        if (q + 1 < total) ffn_wait_vmcnt<MID + EXTRA>();
        else ffn_wait_vmcnt<END>();
        ffn_lds_barrier();
#pragma unroll
        for (int i = 0; i < kFfnSchedIssues; ++i) {
            const int ahead = kFfnSchedIssue[i].chunk;
            if (q + ahead < total) {
                int cn = u + ahead;
                if (cn >= ncht) cn -= ncht;
                if (cn >= ncht) cn -= ncht;   // ncht == 1
                dma_half(q + ahead, cn, kFfnSchedIssue[i].half);
            }
        }
    };
    using no_extra = std::integral_constant<int, 0>;
    __syncthreads();   // parameters in LDS
    {   // what the barriers -2 and -1 would have issued: LO(0), HI(0), LO(1)
        dma_half(0, 0, FFN_HALF_LO);
        dma_half(0, 0, FFN_HALF_HI);
        if (total > 1) dma_half(1, ncht > 1 ? 1 : 0, FFN_HALF_LO);
    }
    // The roles are split with the pre-phase only: the plain kernel measured SLOWER staggered (batch-28
    // encoder rows: 541.9 us against 527.1 us with every wave in role 0) where the PRE kernel gained
    // (656.7 against 669.1 us), profiles/ffn_stagger_ab.txt; both run the one half-slot ring protocol
    constexpr bool STAGGER = PRE;
    const int role = STAGGER ? ffn_sched_role(wave) : 0;

    u32x4 xr[RT][KS];
    f32x4 acc[RT][NT];
    for (int ti = 0; ti < cnt; ++ti) {
        const int tile = bx + ti * P;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int r = tile * ROWS + wave * 16 * RT + 16 * rt + c16;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                // (PRE: one select per row, the column as a constant on top -- an OOB offset stays
                // OOB -- so the per-fragment offsets are not 2 KS values kept live across the tile)
                const unsigned off = PRE ? (r < p.M ? ((unsigned)r * (unsigned)ldx + (unsigned)(8 * g)) * 2u : OOB) + 64u * ks
                                         : r < p.M ? ((unsigned)r * (unsigned)ldx + (unsigned)(32 * ks + 8 * g)) * 2u : OOB;
                xr[rt][ks] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
            }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (PRE) {
            const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)p.R, (short)0, p.r_bytes, 0x00020000);
            // residual fragment kp of both row tiles into the registers of the A fragments kp
            auto load_res = [&](int kp) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int r = tile * ROWS + wave * 16 * RT + 16 * rt + c16;
                    const unsigned off = (r < p.M ? ((unsigned)r * (unsigned)p.ldr + (unsigned)(8 * g)) * 2u : OOB) + 64u * kp;
                    xr[rt][kp] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, off, 0, 0));
                }
            };
            constexpr int KPC = FR / NT;   // k-steps per Wo chunk
            constexpr int PDW = RV == 1 ? 2 : 4;   // Wo fragments read ahead of their MFMAs (RV 1: 3 and 4 spill)
#pragma unroll
            for (int u = 0; u < PCH; ++u) {
                const int q = ti * ncht + u;
                // chunk q landed (a hidden chunk always follows: q + 1 < total).  Younger than its
                // halves' DMA: LO of chunk q+1 and, with RV == 1 from u = 2 on, the RT * KPC residual
                // loads of pre-chunk u-1 (those of pre-chunk u-2 are counted as older, whichever side
                // of that iteration's DMA they were issued on); at u = 0 also the previous tile's
                // stores and this tile's A loads, which this then waits for too
                if (RV == 1 && u >= 2) ring_step(q, u, std::integral_constant<int, RT * KPC>{});
                else ring_step(q, u, no_extra{});
                if constexpr (RV == 1) {
                    if (u > 0) {
#pragma unroll
                        for (int k = 0; k < KPC; ++k) load_res((u - 1) * KPC + k);
                    }
                }
                const char* wb = ring + ffn_sched_slot(q) * G::CHUNK;
                auto frag = [&](int f) { return *reinterpret_cast<const u32x4*>(wb + lane * 16 + f * 1024); };
                // x^T(D x rows) += Wo[:, k-steps of this chunk] A^T: fragment f = (k-step f / NT,
                // tile f % NT), each feeding both row tiles; per accumulator the k-steps ascend
                u32x4 fo[FR];
#pragma unroll
                for (int f = 0; f < PDW; ++f) fo[f] = frag(f);
#pragma unroll
                for (int f = 0; f < FR; ++f) {
                    if (f + PDW < FR) fo[f + PDW] = frag(f + PDW);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) Mma<T>::run(acc[rt][f % NT], fo[f], xr[rt][u * KPC + f / NT]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int kp = (RV == 1 ? KS - KPC : 0); kp < KS; ++kp) load_res(kp);
            // x = LN1(acc + bo + R), rounded to T: phase A's operand and the FFN's residual.  acc
            // and xr fill most of the register file here, so one row tile at a time
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                // (the parameters are re-read from LDS for each row tile: held in registers from
                // the first to the second they would not fit)
                asm volatile("" ::: "memory");
                float s = 0.f;
#pragma unroll
                for (int kp = 0; kp < KS; ++kp) {
                    const f32x4 boa = *reinterpret_cast<const f32x4*>(pbo + 32 * kp + 8 * g);
                    const f32x4 bob = *reinterpret_cast<const f32x4*>(pbo + 32 * kp + 8 * g + 4);
                    f32x4 xa, xb;
                    unpack4<T>(u32x2{xr[rt][kp][0], xr[rt][kp][1]}, reinterpret_cast<float*>(&xa));
                    unpack4<T>(u32x2{xr[rt][kp][2], xr[rt][kp][3]}, reinterpret_cast<float*>(&xb));
                    const f32x4 va = acc[rt][2 * kp] + boa + xa;
                    const f32x4 vb = acc[rt][2 * kp + 1] + bob + xb;
                    acc[rt][2 * kp] = va;
                    acc[rt][2 * kp + 1] = vb;
#pragma unroll
                    for (int i = 0; i < 4; ++i) s += va[i] + vb[i];   // the epilogue's order
                }
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                const float mean = s * (1.f / (float)D);
                float qv = 0.f;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float d = acc[rt][nt][i] - mean;
                        qv += d * d;
                    }
                qv += __shfl_xor(qv, 16);
                qv += __shfl_xor(qv, 32);
                const float rstd = rsqrtf(qv * (1.f / (float)D) + p.eps1);
#pragma unroll
                for (int kp = 0; kp < KS; ++kp) {
                    const int n0 = 32 * kp + 8 * g;
                    float o[8];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        o[i] = acc[rt][2 * kp][i];
                        o[4 + i] = acc[rt][2 * kp + 1][i];
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[k] = (o[k] - mean) * rstd * pg1[n0 + k] + pbe1[n0 + k];
#pragma unroll
                    for (int k = 0; k < 4; ++k) xr[rt][kp][k] = pack2<T>(o[2 * k], o[2 * k + 1]);
                    // opaque from here on: otherwise the epilogue's unpack of x is folded into
                    // these conversions and their results stay live (spilled) across the chunk
                    // loop next to the packed words
                    asm volatile("" : "+v"(xr[rt][kp]));
                }
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // ---- the hidden chunks ----
        // Fragments are read ahead of their MFMAs: phase A's two k-steps ahead, phase B's four
        // fragments ahead.  The scheduling barriers keep the compiler from sinking the reads back
        // next to their uses, where each pair of MFMAs waited for its own LDS round trip: 593-599
        // -> 566-569 us per batch-28 encoder FFN, bit-identical
        // (profiles/r06af_ffn_prefetch_ab.txt; 3 or 6 ahead: the same time)
        constexpr int PDA = 2, PDB = 4;
        static_assert(KS >= PDA && NT >= PDB && PDB > PDA, "prefetch depths");
        auto slot_of = [&](int q) { return ring + ffn_sched_slot(q) * G::CHUNK; };
        auto frag = [&](const char* wb, int f) { return *reinterpret_cast<const u32x4*>(wb + lane * 16 + f * 1024); };
        auto read_a = [&](const char* wb, u32x4(&fa)[KS][2], int ks) {
            fa[ks][0] = frag(wb, ks);
            fa[ks][1] = frag(wb, KS + ks);
        };
        auto read_bias = [&](int c, f32x4(&bb)[2]) {
            bb[0] = *reinterpret_cast<const f32x4*>(pb1 + c * 32 + 4 * g);
            bb[1] = *reinterpret_cast<const f32x4*>(pb1 + c * 32 + 16 + 4 * g);
        };
        // phase A of the hidden chunk in slot wb: H^T chunk (32 hidden x 32 rows) = W1c x^T + b1 (bb:
        // folded into the accumulator init), then ReLU + round -> hb.  fa[0 .. PDA) are read already;
        // tail_b: the chunk's own phase B follows, its first PDB reads are spread over the last PDA
        // k-steps (so the ReLU / rounding between the phases overlaps their latency)
        auto phase_a = [&](const char* wb, const f32x4(&bb)[2], u32x4(&fa)[KS][2], u32x4(&fw)[NT], u32x4(&hb)[RT], auto tail_b) {
            f32x4 h0[RT], h1[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                h0[rt] = bb[0];
                h1[rt] = bb[1];
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks + PDA < KS) {
                    read_a(wb, fa, ks + PDA);
                } else if constexpr (decltype(tail_b)::value) {
                    const int t = ks + PDA - KS;
#pragma unroll
                    for (int j = t * PDB / PDA; j < (t + 1) * PDB / PDA; ++j) fw[j] = frag(wb, 2 * KS + j);
                }
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    Mma<T>::run(h0[rt], fa[ks][0], xr[rt][ks]);
                    Mma<T>::run(h1[rt], fa[ks][1], xr[rt][ks]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // ReLU + round: the B operand of phase B (hidden order as kinet_ffn_pack permuted W2).
            // ReLU as a signed-integer max on the bit pattern (one VALU op; fmaxf on an MFMA
            // result costs a canonicalising max first): the same value for every finite input
            auto relu = [](float v) { return __builtin_bit_cast(float, max(__builtin_bit_cast(int, v), 0)); };
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                hb[rt][0] = pack2<T>(relu(h0[rt][0]), relu(h0[rt][1]));
                hb[rt][1] = pack2<T>(relu(h0[rt][2]), relu(h0[rt][3]));
                hb[rt][2] = pack2<T>(relu(h1[rt][0]), relu(h1[rt][1]));
                hb[rt][3] = pack2<T>(relu(h1[rt][2]), relu(h1[rt][3]));
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        // phase B of the chunk in slot ws: out^T += W2c H^T, each W2 fragment feeding both row tiles;
        // fw[0 .. PDB) are read already.  next_a: phase A of hidden chunk cn (slot wn) follows, its
        // bias and first PDA fragment pairs are read during the last PDB steps
        auto phase_b = [&](const char* ws, const char* wn, int cn, f32x4(&bb)[2], u32x4(&fa)[KS][2], u32x4(&fw)[NT],
                           const u32x4(&hb)[RT], auto next_a) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                if (nt + PDB < NT) {
                    fw[nt + PDB] = frag(ws, 2 * KS + nt + PDB);
                } else if constexpr (decltype(next_a)::value) {
                    const int t = nt + PDB - NT;
                    if (t < PDA) read_a(wn, fa, t);
                    else if (t == PDA) read_bias(cn, bb);
                }
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) Mma<T>::run(acc[rt][nt], fw[nt], hb[rt]);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        const int q0 = ti * ncht + PCH;   // the tile's first hidden chunk
        if (ffn_sched_b_lag(role) == 0) {
            // role 0, per interval: A(c), ReLU, B(c)
            for (int c = 0; c < nch; ++c) {
                ring_step(q0 + c, PCH + c, no_extra{});
                const char* wb = slot_of(q0 + c);
                u32x4 fa[KS][2], fw[NT], hb[RT];
                f32x4 bb[2];
                read_bias(c, bb);
#pragma unroll
                for (int i = 0; i < PDA; ++i) read_a(wb, fa, i);
                phase_a(wb, bb, fa, fw, hb, std::true_type{});
                phase_b(wb, wb, 0, bb, fa, fw, hb, std::false_type{});
            }
        } else {
            // role 1, per interval: B(c - 1), A(c), ReLU(c).  hb (and the first PDB W2 fragments of
            // chunk c - 1, read in front of the barrier: that chunk has been visible since the
            // barrier before) stay in registers across the barrier, so the MFMAs start as it
            // releases, while role 0 waits for chunk c's first fragments; each role's ReLU block
            // then runs beside the partner's MFMAs.  The lag ends with the tile: B of the last chunk
            // runs behind its A in the same interval (role 0 is in the tile epilogue by then)
            u32x4 fa[KS][2], fw[NT], hb[RT];
            f32x4 bb[2];
            ring_step(q0, PCH, no_extra{});
            {
                const char* wb = slot_of(q0);
                read_bias(0, bb);
#pragma unroll
                for (int i = 0; i < PDA; ++i) read_a(wb, fa, i);
                phase_a(wb, bb, fa, fw, hb, std::false_type{});
            }
            for (int c = 1; c < nch; ++c) {
                const char* wp = slot_of(q0 + c - 1);
#pragma unroll
                for (int j = 0; j < PDB; ++j) fw[j] = frag(wp, 2 * KS + j);
                ring_step(q0 + c, PCH + c, no_extra{});
                const char* wb = slot_of(q0 + c);
                phase_b(wp, wb, c, bb, fa, fw, hb, std::true_type{});
                phase_a(wb, bb, fa, fw, hb, std::false_type{});
            }
            const char* wl = slot_of(q0 + nch - 1);
#pragma unroll
            for (int j = 0; j < PDB; ++j) fw[j] = frag(wl, 2 * KS + j);
            phase_b(wl, wl, 0, bb, fa, fw, hb, std::false_type{});
        }
        // ---- tile epilogue (as ffn_fused_kernel): + b2 + residual x, LayerNorm, 16-byte stores ----
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int r = tile * ROWS + wave * 16 * RT + 16 * rt + c16;
            float s = 0.f;
#pragma unroll
            for (int kp = 0; kp < KS; ++kp) {
                float x8[8];
                unpack4<T>(u32x2{xr[rt][kp][0], xr[rt][kp][1]}, x8);
                unpack4<T>(u32x2{xr[rt][kp][2], xr[rt][kp][3]}, x8 + 4);
                const f32x4 b2a = *reinterpret_cast<const f32x4*>(pb2 + 32 * kp + 8 * g);
                const f32x4 b2b = *reinterpret_cast<const f32x4*>(pb2 + 32 * kp + 8 * g + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v0 = acc[rt][2 * kp][i] + b2a[i] + x8[i];
                    const float v1 = acc[rt][2 * kp + 1][i] + b2b[i] + x8[4 + i];
                    acc[rt][2 * kp][i] = v0;
                    acc[rt][2 * kp + 1][i] = v1;
                    s += v0 + v1;
                }
            }
            float mean = 0.f, rstd = 1.f;
            if (ln) {
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                mean = s * (1.f / (float)D);
                float qv = 0.f;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float d = acc[rt][nt][i] - mean;
                        qv += d * d;
                    }
                qv += __shfl_xor(qv, 16);
                qv += __shfl_xor(qv, 32);
                rstd = rsqrtf(qv * (1.f / (float)D) + p.eps);
            }
#pragma unroll
            for (int kp = 0; kp < KS; ++kp) {
                const int n0 = 32 * kp + 8 * g;
                float o[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    o[i] = acc[rt][2 * kp][i];
                    o[4 + i] = acc[rt][2 * kp + 1][i];
                }
                if (ln) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = (o[e] - mean) * rstd * pg[n0 + e] + pbe[n0 + e];
                }
                u32x4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = pack2<T>(o[2 * e], o[2 * e + 1]);
                const unsigned off = PRE ? (r < p.M ? ((unsigned)r * (unsigned)p.ldy + (unsigned)(8 * g)) * 2u : OOB) + 64u * kp
                                         : r < p.M ? ((unsigned)r * (unsigned)p.ldy + (unsigned)n0) * 2u : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, w), ry, off, 0, 0);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// ResNet bottleneck pair: block i's conv3 (1x1, D -> F = 4D, + FrozenBN + residual + ReLU) and
// block i+1's conv1 (1x1, F -> D, + FrozenBN + ReLU) in one launch (torchvision Bottleneck as
// instantiated by the reference, backbone.py:94-108).  Same scheme as the FFN: phase A's
// accumulators (the F-wide block output, chunk by chunk) are phase B's operands, so the block
// output is written once (it is the next block's residual) and never re-read by the next conv1.
//  * phase A: H^T(32 x rows) = W3c t2^T + b3 (the BN scales are folded into the packed weight
//    rows, kinet_bottleneck_pack);  + residual, ReLU, round -> stored to Y (two 8-byte pieces
//    per lane and row tile) and used as the B operand of phase B;
//  * the residual slice of each chunk (rows of the tile x 32 channels, 64 B per row) travels
//    with the chunk's weights by LDS-DMA, two chunks ahead, 16-byte pieces XOR-swizzled by
//    row so the 8-byte reads are conflict-free;
//  * phase B: out^T(D x rows) += W1c H^T over the F/32 chunks; epilogue relu(out + b1).
// Weights: kinet_bottleneck_pack(W3 (F, D), W1 (D, F), s3, s1) -- the FFN fragment layout with
// W3 rows scaled by s3 and W1 rows by s1 before rounding.  F == 4D (the bottleneck expansion).
struct PairArgs {
    const void* X;   // t2 (M, D), row stride ldx
    const void* R;   // residual (M, F), dense
    const void* W;   // packed weights (BN scales folded)
    const float* b3;
    const float* b1;
    void* Y;   // block output (M, F), dense
    void* T;   // next conv1 output (M, D), dense
    int ldx, M, F;
    int x_bytes, r_bytes, w_bytes, y_bytes, t_bytes;
};

template <typename T, int D, int RT, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void bneck_pair_kernel(const PairArgs p, const int ntiles) {
    using G = FfnGeo<D>;
    constexpr int KS = G::KS, NT = G::NT, FR = G::FR;
    static_assert(FR % WAVES == 0, "whole DMA rounds per chunk");
    constexpr int FRW = FR / WAVES;             // weight LDS-DMA instructions per wave per chunk
    constexpr int ROWS = WAVES * 16 * RT;
    constexpr int RES = ROWS * 64;              // residual slice per chunk: 32 channels x 2 B per row
    constexpr int RESW = RT;                    // residual LDS-DMA instructions per wave per chunk (1 KiB each)
    constexpr int SLOT = G::CHUNK + RES;
    constexpr int NS = 3;
    constexpr int F4 = 4 * D;
    constexpr int PAR = (F4 + D) * 4;
    constexpr unsigned OOB = 0x80000000u;
    __shared__ __attribute__((aligned(16))) char lds[PAR + NS * SLOT];
    static_assert(ffn_entry_is<sizeof(lds), ROWS, NS>(ffn_entry<FFN_K_PAIR, D, RT, WAVES, D>()), "ffn_plan.h");
    float* const pb3 = reinterpret_cast<float*>(lds);
    float* const pb1 = pb3 + F4;
    char* const ring = lds + PAR;

    const int P = gridDim.x, bx = blockIdx.x;
    const int cnt = bx < ntiles ? (ntiles - 1 - bx) / P + 1 : 0;
    if (cnt == 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    const int F = p.F, nch = F / 32;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, (short)0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)p.R, (short)0, p.r_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, (short)0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.Y, (short)0, p.y_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rt_ = __builtin_amdgcn_make_buffer_rsrc(p.T, (short)0, p.t_bytes, 0x00020000);

    for (int i = threadIdx.x; i < F4; i += WAVES * 64) pb3[i] = p.b3[i];
    for (int i = threadIdx.x; i < D; i += WAVES * 64) pb1[i] = p.b1[i];
    // chunk q = (tile bx + (q / nch) * P, hidden chunk q % nch): its weights + residual slice.
    // Residual piece of lane l in instruction k: row (k*WAVES + wave)*16 + l/4, 16-byte piece
    // (l & 3) ^ ((row >> 2) & 3) of the row's 64 bytes, landing at LDS unit l (row-major).
    auto dma_chunk = [&](int q) {
        const int ti = q / nch, c = q - ti * nch;
        const int tile = bx + ti * P;
        char* dst = ring + (q % NS) * SLOT;
        const unsigned src = (unsigned)c * (unsigned)G::CHUNK + (unsigned)lane * 16u;
#pragma unroll
        for (int k = 0; k < FRW; ++k) {
            const int f = k * WAVES + wave;
            dma16(rw, dst + f * 1024, src + (unsigned)f * 1024u);
        }
#pragma unroll
        for (int k = 0; k < RESW; ++k) {
            const int rl = (k * WAVES + wave) * 16 + (lane >> 2);
            const int r = tile * ROWS + rl;
            const int piece = (lane & 3) ^ ((rl >> 2) & 3);
            const unsigned off =
                r < p.M ? ((unsigned)r * (unsigned)F + (unsigned)(32 * c)) * 2u + (unsigned)piece * 16u : OOB;
            dma16(rr, dst + G::CHUNK + (k * WAVES + wave) * 1024, off);
        }
    };
    const int total = cnt * nch;
    __syncthreads();   // parameters in LDS
    dma_chunk(0);
    if (total > 1) dma_chunk(1);

    u32x4 xr[RT][KS];
    f32x4 acc[RT][NT];
    for (int ti = 0; ti < cnt; ++ti) {
        const int tile = bx + ti * P;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int r = tile * ROWS + wave * 16 * RT + 16 * rt + c16;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const unsigned off = r < p.M ? ((unsigned)r * (unsigned)p.ldx + (unsigned)(32 * ks + 8 * g)) * 2u : OOB;
                xr[rt][ks] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
            }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nch; ++c) {
            const int q = ti * nch + c;
            // chunk q landed.  Younger vector-memory ops (DMA(q) was issued in iteration q-2):
            // chunk q-2's Y stores (RT), chunk q+1's DMA (if any), chunk q-1's Y stores (RT); across
            // a tile start also T stores and x loads (RT*KS >= RT).  At c == 0 only the DMA is
            // counted (waits longer, and right after the prologue nothing else is younger but x)
            if (q + 1 >= total) ffn_wait_vmcnt<0>();
            else if (c == 0) ffn_wait_vmcnt<FRW + RESW>();
            else ffn_wait_vmcnt<FRW + RESW + 2 * RT>();
            ffn_lds_barrier();   // chunk q visible; slot (q+2) % NS (chunk q-1) free
            if (q + 2 < total) dma_chunk(q + 2);
            const char* wb = ring + (q % NS) * SLOT;
            const char* rb = wb + G::CHUNK;
            f32x4 h0[RT], h1[RT];
            {
                const f32x4 ba = *reinterpret_cast<const f32x4*>(pb3 + c * 32 + 4 * g);
                const f32x4 bb = *reinterpret_cast<const f32x4*>(pb3 + c * 32 + 16 + 4 * g);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    h0[rt] = ba;
                    h1[rt] = bb;
                }
            }
            u32x4 fa0 = *reinterpret_cast<const u32x4*>(wb + lane * 16);
            u32x4 fa1 = *reinterpret_cast<const u32x4*>(wb + lane * 16 + KS * 1024);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                u32x4 na0 = fa0, na1 = fa1;
                if (ks + 1 < KS) {
                    na0 = *reinterpret_cast<const u32x4*>(wb + lane * 16 + (ks + 1) * 1024);
                    na1 = *reinterpret_cast<const u32x4*>(wb + lane * 16 + (KS + ks + 1) * 1024);
                }
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    Mma<T>::run(h0[rt], fa0, xr[rt][ks]);
                    Mma<T>::run(h1[rt], fa1, xr[rt][ks]);
                }
                fa0 = na0;
                fa1 = na1;
            }
            // + residual, ReLU, round: the block output (stored) and phase B's operand
            u32x4 hb[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int rl = wave * 16 * RT + 16 * rt + c16;
                const int sw = (c16 >> 2) & 3;
                const u32x2 ra = *reinterpret_cast<const u32x2*>(rb + rl * 64 + (((g >> 1) ^ sw) << 4) + (g & 1) * 8);
                const u32x2 rb2 = *reinterpret_cast<const u32x2*>(rb + rl * 64 + (((2 + (g >> 1)) ^ sw) << 4) + (g & 1) * 8);
                float r0[4], r1[4];
                unpack4<T>(ra, r0);
                unpack4<T>(rb2, r1);
                float v0[4], v1[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v0[j] = fmaxf(h0[rt][j] + r0[j], 0.f);
                    v1[j] = fmaxf(h1[rt][j] + r1[j], 0.f);
                }
                hb[rt][0] = pack2<T>(v0[0], v0[1]);
                hb[rt][1] = pack2<T>(v0[2], v0[3]);
                hb[rt][2] = pack2<T>(v1[0], v1[1]);
                hb[rt][3] = pack2<T>(v1[2], v1[3]);
                const int r = tile * ROWS + rl;
                const unsigned yo = ((unsigned)r * (unsigned)F + (unsigned)(32 * c + chunk_piece_off(g))) * 2u;
                __builtin_amdgcn_raw_buffer_store_b128(chunk_swap(u32x2{hb[rt][0], hb[rt][1]}, u32x2{hb[rt][2], hb[rt][3]}),
                                                       ry, r < p.M ? yo : OOB, 0, 0);
            }
            // phase B: out^T += W1c H^T, each W1 fragment feeding the RT row tiles
            u32x4 fw = *reinterpret_cast<const u32x4*>(wb + lane * 16 + (2 * KS) * 1024);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                u32x4 nw = fw;
                if (nt + 1 < NT) nw = *reinterpret_cast<const u32x4*>(wb + lane * 16 + (2 * KS + nt + 1) * 1024);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) Mma<T>::run(acc[rt][nt], fw, hb[rt]);
                fw = nw;
            }
        }
        // ---- tile epilogue: relu(out + b1), 16-byte stores of 8 consecutive channels ----
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int r = tile * ROWS + wave * 16 * RT + 16 * rt + c16;
#pragma unroll
            for (int kp = 0; kp < KS; ++kp) {
                const int n0 = 32 * kp + 8 * g;
                float o[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    o[i] = fmaxf(acc[rt][2 * kp][i] + pb1[n0 + i], 0.f);
                    o[4 + i] = fmaxf(acc[rt][2 * kp + 1][i] + pb1[n0 + 4 + i], 0.f);
                }
                u32x4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = pack2<T>(o[2 * e], o[2 * e + 1]);
                const unsigned off = r < p.M ? ((unsigned)r * (unsigned)D + (unsigned)n0) * 2u : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, w), rt_, off, 0, 0);
            }
        }
    }
}

// D = 64 (ResNet layer 1): the whole packed weight stream is 64 KiB, so it is loaded into LDS
// ONCE per workgroup and every wave then runs on its own -- no ring, no barrier in the loop.
// The pair is HBM-bound here (per row 128 B in + 512 B residual + 512 B out + 128 B out; 16
// MFMAs of work per 16 rows and chunk), so what matters is bytes in flight: each wave owns a
// 16-row tile and holds the tile's whole residual (8 chunks x 2 pieces per lane = 32 VGPRs);
// as chunk c consumes its residual registers, they are refilled with the NEXT tile's chunk c,
// so every residual load has a whole tile of work to land under, and the next tile's t2 rows
// load at the tile start into a second register set.  Residual loads and block-output stores
// move 16 bytes per lane (chunk_swap: a row's 64 chunk bytes in four lanes).
// DB = the next conv1's output width: 64 inside stage 1, 128 for the pair that ends stage 1
// (its last conv3 -> stage 2's first conv1, 256 -> 128 channels at stride 1); then the weights
// take 96 KiB and one 16-wave workgroup runs per CU.
template <typename T, int DB, int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1024 / (WAVES * 64)) void bneck64_kernel(const PairArgs p, const int ntiles) {
    constexpr int D = 64, F = 256, KS = 2, NT = DB / 16, KSB = DB / 32, FR = 2 * KS + NT, NCH = F / 32;
    constexpr unsigned OOB = 0x80000000u;
    __shared__ __attribute__((aligned(16))) char wl[NCH * FR * 1024];
    __shared__ float pb3[F], pb1[DB];
    static_assert(ffn_entry_is<sizeof(wl) + sizeof(pb3) + sizeof(pb1), 16, 0>(ffn_entry<FFN_K_B64, D, 1, WAVES, DB>()) &&
                      ffn_entry<FFN_K_B64, D, 1, WAVES, DB>().wg_per_cu == 1024 / (WAVES * 64),
                  "ffn_plan.h (the launch bounds' workgroups per CU too)");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, (short)0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)p.R, (short)0, p.r_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, (short)0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.Y, (short)0, p.y_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rt_ = __builtin_amdgcn_make_buffer_rsrc(p.T, (short)0, p.t_bytes, 0x00020000);
    for (int i = threadIdx.x; i < F; i += WAVES * 64) pb3[i] = p.b3[i];
    if (threadIdx.x < DB) pb1[threadIdx.x] = p.b1[threadIdx.x];
    static_assert(NCH * FR % WAVES == 0, "whole DMA rounds");
#pragma unroll
    for (int k = 0; k < NCH * FR / WAVES; ++k) {
        const int f = k * WAVES + wave;
        dma16(rw, wl + f * 1024, (unsigned)f * 1024u + (unsigned)lane * 16u);
    }
    ffn_wait_vmcnt<0>();
    __syncthreads();

    const int nw = gridDim.x * WAVES;
    int tile = blockIdx.x * WAVES + wave;
    if (tile >= ntiles) return;
    auto row_of = [&](int t) { return t * 16 + c16; };
    auto load_x = [&](int t, u32x4 (&dst)[KS]) {
        const int r = row_of(t);
        const bool ok = t < ntiles && r < p.M;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            dst[ks] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                    rx, ok ? ((unsigned)r * (unsigned)p.ldx + (unsigned)(32 * ks + 8 * g)) * 2u : OOB, 0, 0));
    };
    const int poff = chunk_piece_off(g);
    auto res_off = [&](int t, int c) -> unsigned {
        const int r = row_of(t);
        return (t < ntiles && r < p.M) ? ((unsigned)r * (unsigned)F + (unsigned)(32 * c + poff)) * 2u : OOB;
    };
    u32x4 xr[KS], xn[KS];
    u32x4 res[NCH];   // 16-byte pieces (chunk_swap order)
    load_x(tile, xr);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
        res[c] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, res_off(tile, c), 0, 0));
    // first tile landed (once per wave): otherwise the compiler's wait for these registers at the
    // loop head, merged with the back edge, drains every residual load of each later tile there
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
    for (; tile < ntiles; tile += nw) {
        const int next = tile + nw;
        load_x(next, xn);
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int r = row_of(tile);
        const bool rok = r < p.M;
        // opaque per tile: keeps the 64 weight-fragment reads in the loop (hoisted, they would
        // take 256 VGPRs)
        int woff = lane * 16;
        asm volatile("" : "+v"(woff));
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const char* wb = wl + c * FR * 1024 + woff;
            f32x4 h0 = *reinterpret_cast<const f32x4*>(pb3 + c * 32 + 4 * g);
            f32x4 h1 = *reinterpret_cast<const f32x4*>(pb3 + c * 32 + 16 + 4 * g);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                Mma<T>::run(h0, *reinterpret_cast<const u32x4*>(wb + ks * 1024), xr[ks]);
                Mma<T>::run(h1, *reinterpret_cast<const u32x4*>(wb + (KS + ks) * 1024), xr[ks]);
            }
            const u32x4 rq = chunk_swap(u32x2{res[c][0], res[c][1]}, u32x2{res[c][2], res[c][3]});
            float r0[4], r1[4];
            unpack4<T>(u32x2{rq[0], rq[1]}, r0);
            unpack4<T>(u32x2{rq[2], rq[3]}, r1);
            u32x4 hb;
            hb[0] = pack2<T>(fmaxf(h0[0] + r0[0], 0.f), fmaxf(h0[1] + r0[1], 0.f));
            hb[1] = pack2<T>(fmaxf(h0[2] + r0[2], 0.f), fmaxf(h0[3] + r0[3], 0.f));
            hb[2] = pack2<T>(fmaxf(h1[0] + r1[0], 0.f), fmaxf(h1[1] + r1[1], 0.f));
            hb[3] = pack2<T>(fmaxf(h1[2] + r1[2], 0.f), fmaxf(h1[3] + r1[3], 0.f));
            const unsigned yo = ((unsigned)r * (unsigned)F + (unsigned)(32 * c + poff)) * 2u;
            __builtin_amdgcn_raw_buffer_store_b128(chunk_swap(u32x2{hb[0], hb[1]}, u32x2{hb[2], hb[3]}), ry,
                                                   rok ? yo : OOB, 0, 0);
            // this chunk's residual registers now take the next tile's chunk c
            res[c] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, res_off(next, c), 0, 0));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                Mma<T>::run(acc[nt], *reinterpret_cast<const u32x4*>(wb + (2 * KS + nt) * 1024), hb);
        }
#pragma unroll
        for (int kp = 0; kp < KSB; ++kp) {
            const int n0 = 32 * kp + 8 * g;
            u32x4 w;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                w[e] = pack2<T>(fmaxf(acc[2 * kp][2 * e] + pb1[n0 + 2 * e], 0.f),
                                fmaxf(acc[2 * kp][2 * e + 1] + pb1[n0 + 2 * e + 1], 0.f));
                w[2 + e] = pack2<T>(fmaxf(acc[2 * kp + 1][2 * e] + pb1[n0 + 4 + 2 * e], 0.f),
                                    fmaxf(acc[2 * kp + 1][2 * e + 1] + pb1[n0 + 4 + 2 * e + 1], 0.f));
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, w), rt_,
                                                   rok ? ((unsigned)r * (unsigned)DB + (unsigned)n0) * 2u : OOB, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xr[ks] = xn[ks];
    }
}

// Stage 1's FIRST pair with block 0's downsample branch folded in (kinet_bottleneck_pair_ds):
// the identity of block 0 is conv_ds(x0) * s_ds + b_ds, a 1x1 64 -> 256 conv over the same rows,
// so the block output is ONE GEMM with the K dimensions concatenated,
//   Y = relu([t2 | x0] [s3 W3 | s_ds W_ds]^T + (b3 + b_ds)),
// and the 256-channel identity tensor is neither written nor read: per row 128 B (t2) + 128 B
// (x0) in, 512 B (Y) + 128 B (T) out, against 1920 B for the downsample launch + the plain pair.
// Same scheme as bneck64_kernel: weights resident in LDS (12 fragments per chunk: W3, W_ds, W1
// = 96 KiB, one 16-wave workgroup per CU), every wave on its own 16*RT-row tile, phase A takes
// KS steps on t2 and KS more on x0 into the same f32 accumulators (the identity branch is never
// rounded), no residual registers.  RT = 1 loads the next tile's t2 / x0 rows at the tile start
// into a second register set; RT = 2 (ffn_debug 512, A/B) shares each fragment read between two
// row tiles and loads the next tile's rows after the last chunk's phase A.
struct PairDsArgs {
    const void* X;    // t2 (M, 64), row stride ldx
    const void* X0;   // block input (M, 64), row stride ldx0
    const void* W;    // kinet_bottleneck_pack_ds
    const float* b3;  // b3 + b_ds
    const float* b1;
    void* Y;   // block output (M, 256), dense
    void* T;   // next conv1 output (M, 64), dense
    int ldx, ldx0, M;
    int x_bytes, x0_bytes, w_bytes, y_bytes, t_bytes;
};

template <typename T, int RT>
__global__ __launch_bounds__(1024) void bneck64_ds_kernel(const PairDsArgs p, const int ntiles) {
    constexpr int F = 256, DB = 64, WAVES = 16, KS = 2, NT = DB / 16, KSB = DB / 32, FR = 4 * KS + NT, NCH = F / 32;
    constexpr bool PF = RT == 1;
    constexpr unsigned OOB = 0x80000000u;
    __shared__ __attribute__((aligned(16))) char wl[NCH * FR * 1024];
    __shared__ float pb3[F], pb1[DB];
    static_assert(ffn_entry_is<sizeof(wl) + sizeof(pb3) + sizeof(pb1), 16 * RT, 0>(ffn_entry<FFN_K_B64_DS, 64, RT, WAVES, DB>()),
                  "ffn_plan.h");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c16 = lane & 15;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, (short)0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.X0, (short)0, p.x0_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, (short)0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.Y, (short)0, p.y_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rt_ = __builtin_amdgcn_make_buffer_rsrc(p.T, (short)0, p.t_bytes, 0x00020000);
    for (int i = threadIdx.x; i < F; i += WAVES * 64) pb3[i] = p.b3[i];
    if (threadIdx.x < DB) pb1[threadIdx.x] = p.b1[threadIdx.x];
    static_assert(NCH * FR % WAVES == 0, "whole DMA rounds");
#pragma unroll
    for (int k = 0; k < NCH * FR / WAVES; ++k) {
        const int f = k * WAVES + wave;
        dma16(rw, wl + f * 1024, (unsigned)f * 1024u + (unsigned)lane * 16u);
    }
    ffn_wait_vmcnt<0>();
    __syncthreads();

    const int nw = gridDim.x * WAVES;
    int tile = blockIdx.x * WAVES + wave;
    if (tile >= ntiles) return;
    auto row_of = [&](int t, int rt) { return (t * RT + rt) * 16 + c16; };
    auto load_rows = [&](int t, const __amdgpu_buffer_rsrc_t& rs, int ld, u32x4 (&dst)[RT][KS]) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int r = row_of(t, rt);
            const bool ok = t < ntiles && r < p.M;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                dst[rt][ks] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                            rs, ok ? ((unsigned)r * (unsigned)ld + (unsigned)(32 * ks + 8 * g)) * 2u : OOB, 0, 0));
        }
    };
    const int poff = chunk_piece_off(g);
    u32x4 xr[RT][KS], x0r[RT][KS], xn[PF ? RT : 1][KS], x0n[PF ? RT : 1][KS];
    load_rows(tile, rx, p.ldx, xr);
    load_rows(tile, rx0, p.ldx0, x0r);
    // first tile landed (once per wave), as in bneck64_kernel
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
    for (; tile < ntiles; tile += nw) {
        const int next = tile + nw;
        if constexpr (PF) {
            load_rows(next, rx, p.ldx, xn);
            load_rows(next, rx0, p.ldx0, x0n);
        }
        f32x4 acc[RT][NT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // opaque per tile: keeps the 96 weight-fragment reads in the loop
        int woff = lane * 16;
        asm volatile("" : "+v"(woff));
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const char* wb = wl + c * FR * 1024 + woff;
            f32x4 h0[RT], h1[RT];
            {
                const f32x4 ba = *reinterpret_cast<const f32x4*>(pb3 + c * 32 + 4 * g);
                const f32x4 bb = *reinterpret_cast<const f32x4*>(pb3 + c * 32 + 16 + 4 * g);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    h0[rt] = ba;
                    h1[rt] = bb;
                }
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {   // conv3 over t2
                const u32x4 fa0 = *reinterpret_cast<const u32x4*>(wb + ks * 1024);
                const u32x4 fa1 = *reinterpret_cast<const u32x4*>(wb + (KS + ks) * 1024);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    Mma<T>::run(h0[rt], fa0, xr[rt][ks]);
                    Mma<T>::run(h1[rt], fa1, xr[rt][ks]);
                }
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {   // the downsample conv over x0, same accumulators
                const u32x4 fd0 = *reinterpret_cast<const u32x4*>(wb + (2 * KS + ks) * 1024);
                const u32x4 fd1 = *reinterpret_cast<const u32x4*>(wb + (3 * KS + ks) * 1024);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    Mma<T>::run(h0[rt], fd0, x0r[rt][ks]);
                    Mma<T>::run(h1[rt], fd1, x0r[rt][ks]);
                }
            }
            u32x4 hb[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                hb[rt][0] = pack2<T>(fmaxf(h0[rt][0], 0.f), fmaxf(h0[rt][1], 0.f));
                hb[rt][1] = pack2<T>(fmaxf(h0[rt][2], 0.f), fmaxf(h0[rt][3], 0.f));
                hb[rt][2] = pack2<T>(fmaxf(h1[rt][0], 0.f), fmaxf(h1[rt][1], 0.f));
                hb[rt][3] = pack2<T>(fmaxf(h1[rt][2], 0.f), fmaxf(h1[rt][3], 0.f));
                const int r = row_of(tile, rt);
                const unsigned yo = ((unsigned)r * (unsigned)F + (unsigned)(32 * c + poff)) * 2u;
                __builtin_amdgcn_raw_buffer_store_b128(chunk_swap(u32x2{hb[rt][0], hb[rt][1]}, u32x2{hb[rt][2], hb[rt][3]}),
                                                       ry, r < p.M ? yo : OOB, 0, 0);
            }
            if constexpr (!PF) {
                if (c == NCH - 1) {   // t2 / x0 of this tile are done with: the next tile's rows
                    load_rows(next, rx, p.ldx, xr);
                    load_rows(next, rx0, p.ldx0, x0r);
                }
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const u32x4 fw = *reinterpret_cast<const u32x4*>(wb + (4 * KS + nt) * 1024);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) Mma<T>::run(acc[rt][nt], fw, hb[rt]);
            }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int r = row_of(tile, rt);
#pragma unroll
            for (int kp = 0; kp < KSB; ++kp) {
                const int n0 = 32 * kp + 8 * g;
                u32x4 w;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    w[e] = pack2<T>(fmaxf(acc[rt][2 * kp][2 * e] + pb1[n0 + 2 * e], 0.f),
                                    fmaxf(acc[rt][2 * kp][2 * e + 1] + pb1[n0 + 2 * e + 1], 0.f));
                    w[2 + e] = pack2<T>(fmaxf(acc[rt][2 * kp + 1][2 * e] + pb1[n0 + 4 + 2 * e], 0.f),
                                        fmaxf(acc[rt][2 * kp + 1][2 * e + 1] + pb1[n0 + 4 + 2 * e + 1], 0.f));
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, w), rt_,
                                                       r < p.M ? ((unsigned)r * (unsigned)DB + (unsigned)n0) * 2u : OOB, 0, 0);
            }
        }
        if constexpr (PF) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    xr[rt][ks] = xn[rt][ks];
                    x0r[rt][ks] = x0n[rt][ks];
                }
        }
    }
}


// The four packed streams (kinet_ffn_pack, kinet_ffn_pack_attn, kinet_bottleneck_pack,
// kinet_bottleneck_pack_ds) through the one layout function, ffn_pack_src (ffn_plan.h).  F32: the
// sources are f32 and every row is scaled by its FrozenBN scale (in f32) before the one rounding to T;
// otherwise they are T already and are copied.
struct PackSrc {
    const void* W[kFfnPackMats];
    const float* scale[kFfnPackMats];
};

template <typename T, bool F32>
__global__ void ffn_pack_kernel(const PackSrc src, T* __restrict__ out, int kind, int D, int F, int DB) {
    const long total = ffn_pack_total(kind, D, F, DB);
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const FfnPackSrc e = ffn_pack_src(kind, D, F, DB, idx);
        const long at = (long)e.row * e.ld + e.col;
        if constexpr (F32) {
            float v = static_cast<const float*>(src.W[e.mat])[at] * src.scale[e.mat][e.row];
            // keeps the parent's instruction pair, v_mul_f32 then v_cvt_f16_f32 / v_cvt_pk_bf16_f32 (the
            // documented f32 scale + one rounding to T): without it hipcc emits v_fma_mixlo_f16 for the f16
            // kernel here, and a packed f16 buffer no longer matched the f32-scaled, once-rounded gather
            // (tests/test_ffn_pack_gpu.py); profiles/ffn_plan_equiv.log section 2
            asm volatile("" : "+v"(v));
            out[idx] = Cvt<T>::from(v);
        } else {
            out[idx] = static_cast<const T*>(src.W[e.mat])[at];
        }
    }
}

template <bool F32>
int launch_pack(const PackSrc& src, void* packed, int kind, int D, int F, int DB, int dtype, kinet_stream_t stream) {
    const long total = ffn_pack_total(kind, D, F, DB);
    const dim3 grid((int)((total + 255) / 256 < kMaxGridStride ? (total + 255) / 256 : kMaxGridStride)), block(256);
    if (dtype == KINET_BF16)
        hipLaunchKernelGGL((ffn_pack_kernel<bf16_t, F32>), grid, block, 0, (hipStream_t)stream, src, (bf16_t*)packed, kind, D, F, DB);
    else
        hipLaunchKernelGGL((ffn_pack_kernel<f16_t, F32>), grid, block, 0, (hipStream_t)stream, src, (f16_t*)packed, kind, D, F, DB);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

// the argument struct each kernel family takes
template <typename Args>
constexpr bool takes(int family) {
    return std::is_same<Args, FfnArgs>::value    ? family == FFN_K_FUSED || family == FFN_K_RT2
           : std::is_same<Args, PairArgs>::value ? family == FFN_K_PAIR || family == FFN_K_B64
                                                 : family == FFN_K_B64_DS;
}

// Launch entry I of kFfnKernels (ffn_plan.h) for one element type if `kernel` names it.  These are
// the only launches of the five kernel families, so the table is the list of their instantiations.
template <typename T, int I, typename Args>
void launch_entry(int kernel, dim3 grid, hipStream_t s, const Args& a, int tiles) {
    constexpr FfnKernel k = kFfnKernels[I];
    if constexpr (takes<Args>(k.family)) {
        if (kernel != I) return;
        const dim3 block(k.block());
        if constexpr (k.family == FFN_K_FUSED) {
            hipLaunchKernelGGL((ffn_fused_kernel<T, k.d, k.rt, k.waves>), grid, block, 0, s, a, tiles);
        } else if constexpr (k.family == FFN_K_RT2) {
            static_assert(k.rt == 2 && k.waves == 8, "ffn_fused_rt2_kernel is 8 waves x 32 rows");
            hipLaunchKernelGGL((ffn_fused_rt2_kernel<T, k.d, k.pre, k.rv>), grid, block, 0, s, a, tiles);
        } else if constexpr (k.family == FFN_K_PAIR) {
            hipLaunchKernelGGL((bneck_pair_kernel<T, k.d, k.rt, k.waves>), grid, block, 0, s, a, tiles);
        } else if constexpr (k.family == FFN_K_B64) {
            hipLaunchKernelGGL((bneck64_kernel<T, k.db, k.waves>), grid, block, 0, s, a, tiles);
        } else {
            static_assert(k.waves == 16, "bneck64_ds_kernel is 16 waves");
            hipLaunchKernelGGL((bneck64_ds_kernel<T, k.rt>), grid, block, 0, s, a, tiles);
        }
    }
}
template <typename T, typename Args, int... I>
void launch_kernel(const FfnPlan& pl, hipStream_t s, const Args& a, std::integer_sequence<int, I...>) {
    (launch_entry<T, I>(pl.kernel, dim3(pl.grid), s, a, pl.tiles), ...);
}

FfnProblem ffn_problem(int kind, int M, int D, int F, int DB, int cus) {
    return FfnProblem{kind, M, D, F, DB, ffn_debug, solo_launch(), cus, ffn_cap};
}

int refused(const FfnPlan& pl) {
    set_error(pl.why, pl.why_arg[0], pl.why_arg[1]);
    return KINET_ERR_ARG;
}

// Plan the call (ffn_plan.h: every choice, tile count and grid lives there) and run the planned
// launch: kernel, block, grid and the kinet_ffn_last_kernel record all come from its one table entry.
template <typename Args>
int launch_planned(int kind, int M, int D, int F, int DB, int dtype, const Args& a, kinet_stream_t stream) {
    FfnPlan pl;
    if (!ffn_plan(ffn_problem(kind, M, D, F, DB, cu_count()), pl)) return refused(pl);
    ffn_last = pl.kernel;
    constexpr std::make_integer_sequence<int, kNumFfnKernels> all{};
    if (dtype == KINET_BF16) launch_kernel<bf16_t>(pl, (hipStream_t)stream, a, all);
    else launch_kernel<f16_t>(pl, (hipStream_t)stream, a, all);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

// checks the entry points share
bool dt16(int dtype) { return dtype == KINET_BF16 || dtype == KINET_F16; }
template <typename... Q>
bool al16(const Q*... q) { return (((uintptr_t)q | ...) & 15u) == 0; }
// bytes of M rows of stride ld elements, the last one D wide (buffer descriptors: below 2 GiB)
long long extent(int M, int ld, int D) { return ((long long)(M - 1) * ld + D) * 2; }
constexpr long long k2GiB = 1LL << 31;

}  // namespace
}  // namespace kinet

using namespace kinet;

extern "C" int kinet_ffn_set_debug(int flags) {
    const int old = ffn_debug;
    ffn_debug = flags;
    return old;
}

extern "C" int kinet_ffn_grid_cap(int max_wgs) {
    const int old = ffn_cap;
    ffn_cap = max_wgs > 0 ? max_wgs : 0;
    return old;
}

extern "C" int kinet_ffn_last_kernel(void) { return ffn_last; }

extern "C" const char* kinet_ffn_kernel_name(int kernel) {
    return kernel >= 0 && kernel < kNumFfnKernels ? kFfnKernels[kernel].name : nullptr;
}

extern "C" int kinet_ffn_launch_plan(const int* problem, int cus, int* plan_out) {
    KINET_CHECK_ARG(problem != nullptr && plan_out != nullptr && cus > 0, "ffn launch plan: invalid arguments");
    const int* f = problem;
    KINET_CHECK_ARG(f[KINET_FFNP_KIND] >= FFN_FFN && f[KINET_FFNP_KIND] <= FFN_PAIR_DS && f[KINET_FFNP_M] >= 0,
                    "ffn launch plan: invalid problem");
    FfnPlan pl;
    if (!ffn_plan(ffn_problem(f[KINET_FFNP_KIND], f[KINET_FFNP_M], f[KINET_FFNP_D], f[KINET_FFNP_F], f[KINET_FFNP_DB], cus), pl))
        return refused(pl);
    const FfnKernel& k = kFfnKernels[pl.kernel];
    const int rec[KINET_FFNPL_FIELDS] = {pl.kernel, pl.tiles, pl.grid, k.block(), k.waves, k.tile_rows,
                                         k.wg_tiles, k.wg_per_cu, ffn_kernel_lds(k)};
    for (int i = 0; i < KINET_FFNPL_FIELDS; ++i) plan_out[i] = rec[i];
    return KINET_OK;
}

extern "C" int kinet_ffn_sched(int role, int cnt, int pch, int nch, int q, int half_ops, int* out) {
    KINET_CHECK_ARG(out != nullptr && (role == 0 || role == 1) && cnt > 0 && pch >= 0 && nch > 0 && half_ops > 0,
                    "ffn_sched: invalid arguments");
    const int total = ffn_sched_total(cnt, pch, nch);
    KINET_CHECK_ARG(q >= -1 && q < total, "ffn_sched: chunk %d outside [-1, %d)", q, total);
    for (int i = 0; i < KINET_FFNS_FIELDS; ++i) out[i] = -1;
    out[KINET_FFNS_TOTAL] = total;
    out[KINET_FFNS_BARRIERS] = ffn_sched_barriers(role, cnt, pch, nch);
    auto put = [&](int n_field, int field, const FfnHalfList& l) {
        out[n_field] = l.n;
        for (int i = 0; i < l.n; ++i) {
            out[field + 2 * i] = l.e[i].chunk;
            out[field + 2 * i + 1] = l.e[i].half;
        }
    };
    put(KINET_FFNS_N_ISSUE, KINET_FFNS_ISSUE, ffn_sched_issue(q, total));
    out[KINET_FFNS_N_EARLY] = out[KINET_FFNS_N_READ] = 0;
    if (q < 0) return KINET_OK;
    out[KINET_FFNS_BARRIER] = q;
    out[KINET_FFNS_SLOT] = ffn_sched_slot(q);
    out[KINET_FFNS_VMCNT] = ffn_sched_vmcnt(q, total, half_ops);
    put(KINET_FFNS_N_EARLY, KINET_FFNS_EARLY, ffn_sched_early_reads(role, q, pch, nch));
    put(KINET_FFNS_N_READ, KINET_FFNS_READ, ffn_sched_reads(role, q, pch, nch));
    return KINET_OK;
}

extern "C" int kinet_ffn_pack_map(int kind, int D, int F, int DB, int32_t* out) {
    KINET_CHECK_ARG(kind >= FFN_PACK_FFN && kind <= FFN_PACK_ATTN && out != nullptr, "ffn_pack_map: invalid arguments");
    KINET_CHECK_ARG(D > 0 && D % 32 == 0 && F > 0 && F % 32 == 0 && DB > 0 && DB % 32 == 0,
                    "ffn_pack_map: need D, F, DB multiples of 32 (D=%d F=%d DB=%d)", D, F, DB);
    KINET_CHECK_ARG(DB == D || kind == FFN_PACK_PAIR, "ffn_pack_map: DB must be D but for the bottleneck pair (D=%d DB=%d)", D, DB);
    const long long total = ffn_pack_total(kind, D, F, DB);
    for (long long idx = 0; idx < total; ++idx) {
        const FfnPackSrc e = ffn_pack_src(kind, D, F, DB, idx);
        out[3 * idx] = e.mat;
        out[3 * idx + 1] = e.row;
        out[3 * idx + 2] = e.col;
    }
    return KINET_OK;
}

extern "C" int kinet_ffn_pack(const void* W1, const void* W2, void* packed, int D, int F, int dtype,
                              kinet_stream_t stream) {
    KINET_CHECK_ARG(D > 0 && D % 32 == 0 && F > 0 && F % 32 == 0, "ffn_pack: need D %% 32 == 0 and F %% 32 == 0 (D=%d F=%d)", D, F);
    KINET_CHECK_ARG(dt16(dtype), "ffn_pack: dtype must be bf16 or f16");
    return launch_pack<false>(PackSrc{{W1, W2}, {}}, packed, FFN_PACK_FFN, D, F, D, dtype, stream);
}

extern "C" int kinet_ffn_fused(const void* X, int ldx, const void* packed, const float* b1, const float* b2,
                               const float* ln_gamma, const float* ln_beta, float ln_eps, void* Y, int ldy, int M,
                               int D, int F, int dtype, kinet_stream_t stream) {
    KINET_CHECK_ARG(D == 256 || D == 288, kFfnWhyD, D);
    KINET_CHECK_ARG(F > 0 && F % 32 == 0 && F <= FFN_MAX_F, "ffn_fused: F must be a multiple of 32 in [32, %d] (got %d)", FFN_MAX_F, F);
    KINET_CHECK_ARG(M >= 0 && ldx >= D && ldy >= D && ldx % 8 == 0 && ldy % 8 == 0, "ffn_fused: bad M / ldx / ldy");
    KINET_CHECK_ARG(dt16(dtype), "ffn_fused: dtype must be bf16 or f16");
    KINET_CHECK_ARG(b1 != nullptr && b2 != nullptr, "ffn_fused: b1 and b2 are required");
    KINET_CHECK_ARG((ln_gamma == nullptr) == (ln_beta == nullptr), "ffn_fused: LayerNorm needs both gamma and beta");
    KINET_CHECK_ARG(al16(X, Y, packed, b1, b2, ln_gamma, ln_beta),
                    "ffn_fused: X, Y, packed weights, biases and LayerNorm params must be 16-byte aligned");
    if (M == 0) return KINET_OK;
    const long long xb = extent(M, ldx, D);
    KINET_CHECK_ARG(xb < k2GiB, "ffn_fused: X larger than 2 GiB (split the call)");
    FfnArgs a{};
    a.X = X; a.W = packed; a.b1 = b1; a.b2 = b2; a.ln_g = ln_gamma; a.ln_b = ln_beta; a.Y = Y; a.eps = ln_eps;
    a.ldx = ldx; a.ldy = ldy; a.M = M; a.F = F;
    a.x_bytes = (int)xb;
    a.w_bytes = (int)(ffn_pack_total(FFN_PACK_FFN, D, F, D) * 2);
    const long long yb = extent(M, ldy, D);
    KINET_CHECK_ARG(yb < k2GiB, "ffn_fused: Y larger than 2 GiB (split the call)");
    a.y_bytes = (int)yb;
    a.dbg = ffn_debug;
    return launch_planned(FFN_FFN, M, D, F, D, dtype, a, stream);
}

extern "C" int kinet_ffn_pack_attn(const void* Wo, const void* W1, const void* W2, void* packed, int D, int F,
                                   int dtype, kinet_stream_t stream) {
    KINET_CHECK_ARG(D > 0 && D % 32 == 0 && F > 0 && F % 32 == 0, "ffn_pack_attn: need D %% 32 == 0 and F %% 32 == 0 (D=%d F=%d)", D, F);
    KINET_CHECK_ARG(dt16(dtype), "ffn_pack_attn: dtype must be bf16 or f16");
    return launch_pack<false>(PackSrc{{Wo, W1, W2}, {}}, packed, FFN_PACK_ATTN, D, F, D, dtype, stream);
}

extern "C" int kinet_attn_out_ffn_fused(const void* A, int lda, const void* R, int ldr, const void* packed,
                                        const float* bo, const float* g1, const float* be1, float eps1,
                                        const float* b1, const float* b2, const float* g2, const float* be2,
                                        float eps2, void* Y, int ldy, int M, int D, int F, int dtype,
                                        kinet_stream_t stream) {
    KINET_CHECK_ARG(D != 288, kAttnOutWhyD288);
    KINET_CHECK_ARG(D == 256, kAttnOutWhyD, D);
    KINET_CHECK_ARG(F > 0 && F % 32 == 0 && F <= FFN_MAX_F, "attn_out_ffn_fused: F must be a multiple of 32 in [32, %d] (got %d)", FFN_MAX_F, F);
    KINET_CHECK_ARG(M >= 0 && lda >= D && ldr >= D && ldy >= D && lda % 8 == 0 && ldr % 8 == 0 && ldy % 8 == 0,
                    "attn_out_ffn_fused: bad M / lda / ldr / ldy");
    KINET_CHECK_ARG(dt16(dtype), "attn_out_ffn_fused: dtype must be bf16 or f16");
    KINET_CHECK_ARG(bo != nullptr && g1 != nullptr && be1 != nullptr, "attn_out_ffn_fused: bo and the first LayerNorm's gamma and beta are required");
    KINET_CHECK_ARG(b1 != nullptr && b2 != nullptr, "attn_out_ffn_fused: b1 and b2 are required");
    KINET_CHECK_ARG((g2 == nullptr) == (be2 == nullptr), "attn_out_ffn_fused: the second LayerNorm needs both gamma and beta");
    KINET_CHECK_ARG(al16(A, R, Y, packed, bo, g1, be1, b1, b2, g2, be2),
                    "attn_out_ffn_fused: A, R, Y, packed weights, biases and LayerNorm params must be 16-byte aligned");
    if (M == 0) return KINET_OK;
    const long long ab = extent(M, lda, D), rb = extent(M, ldr, D), yb = extent(M, ldy, D);
    KINET_CHECK_ARG(ab < k2GiB && rb < k2GiB && yb < k2GiB, "attn_out_ffn_fused: A, R or Y larger than 2 GiB (split the call)");
    auto overlap = [](const void* u, long long ub, const void* v, long long vb) {
        return (const char*)u < (const char*)v + vb && (const char*)v < (const char*)u + ub;
    };
    KINET_CHECK_ARG(!overlap(Y, yb, A, ab) && !overlap(Y, yb, R, rb), "attn_out_ffn_fused: Y must not alias A or R");
    FfnArgs a{};
    a.W = packed; a.b1 = b1; a.b2 = b2; a.ln_g = g2; a.ln_b = be2; a.Y = Y; a.eps = eps2;
    a.ldy = ldy; a.M = M; a.F = F;
    a.w_bytes = (int)(ffn_pack_total(FFN_PACK_ATTN, D, F, D) * 2);
    a.y_bytes = (int)yb;
    a.dbg = ffn_debug;
    a.A = A; a.R = R; a.bo = bo; a.g1 = g1; a.be1 = be1; a.eps1 = eps1;
    a.lda = lda; a.ldr = ldr; a.a_bytes = (int)ab; a.r_bytes = (int)rb;
    return launch_planned(FFN_ATTN_OUT, M, D, F, D, dtype, a, stream);
}

extern "C" int kinet_bottleneck_pack(const float* W3, const float* W1, const float* s3, const float* s1,
                                     void* packed, int D, int F, int DB, int dtype, kinet_stream_t stream) {
    KINET_CHECK_ARG(D > 0 && D % 32 == 0 && F > 0 && F % 32 == 0 && DB > 0 && DB % 32 == 0,
                    "bottleneck_pack: need D, F, DB multiples of 32 (D=%d F=%d DB=%d)", D, F, DB);
    KINET_CHECK_ARG(dt16(dtype), "bottleneck_pack: dtype must be bf16 or f16");
    KINET_CHECK_ARG(W3 && W1 && s3 && s1 && packed, "bottleneck_pack: null pointer");
    return launch_pack<true>(PackSrc{{W3, W1}, {s3, s1}}, packed, FFN_PACK_PAIR, D, F, DB, dtype, stream);
}

extern "C" int kinet_bottleneck_pair(const void* X, int ldx, const void* R, const void* packed, const float* b3,
                                     const float* b1, void* Y, void* T, int M, int D, int F, int DB, int dtype,
                                     kinet_stream_t stream) {
    KINET_CHECK_ARG(D == 64 || D == 128 || D == 256, kPairWhyD, D);
    KINET_CHECK_ARG(F == 4 * D, "bottleneck_pair: F must be 4 * D (got D=%d F=%d)", D, F);
    KINET_CHECK_ARG(DB == D || (D == 64 && DB == 128), kPairWhyDB, D, DB);
    KINET_CHECK_ARG(M >= 0 && ldx >= D && ldx % 8 == 0, "bottleneck_pair: bad M / ldx");
    KINET_CHECK_ARG(dt16(dtype), "bottleneck_pair: dtype must be bf16 or f16");
    KINET_CHECK_ARG(b3 && b1, "bottleneck_pair: folded BN biases of both convs are required");
    KINET_CHECK_ARG(al16(X, R, packed, Y, T, b3, b1), "bottleneck_pair: tensors and BN biases must be 16-byte aligned");
    if (M == 0) return KINET_OK;
    const long long xb = extent(M, ldx, D), fb = (long long)M * F * 2;
    KINET_CHECK_ARG(xb < k2GiB && fb < k2GiB, "bottleneck_pair: tensors larger than 2 GiB (split the call)");
    PairArgs a{};
    a.X = X; a.R = R; a.W = packed; a.b3 = b3; a.b1 = b1; a.Y = Y; a.T = T;
    a.ldx = ldx; a.M = M; a.F = F;
    a.x_bytes = (int)xb;
    a.r_bytes = (int)fb;
    a.y_bytes = (int)fb;
    a.w_bytes = (int)(ffn_pack_total(FFN_PACK_PAIR, D, F, DB) * 2);
    a.t_bytes = (int)((long long)M * DB * 2);
    return launch_planned(FFN_PAIR, M, D, F, DB, dtype, a, stream);
}

extern "C" int kinet_bottleneck_pack_ds(const float* W3, const float* Wds, const float* W1, const float* s3,
                                        const float* sds, const float* s1, void* packed, int D, int F, int DB,
                                        int dtype, kinet_stream_t stream) {
    KINET_CHECK_ARG(D == 64 && F == 256 && DB == 64,
                    "bottleneck_pack_ds: stage 1 only, D = 64, F = 256, DB = 64 (got D=%d F=%d DB=%d)", D, F, DB);
    KINET_CHECK_ARG(dt16(dtype), "bottleneck_pack_ds: dtype must be bf16 or f16");
    KINET_CHECK_ARG(W3 && Wds && W1 && s3 && sds && s1 && packed, "bottleneck_pack_ds: null pointer");
    return launch_pack<true>(PackSrc{{W3, Wds, W1}, {s3, sds, s1}}, packed, FFN_PACK_DS, D, F, DB, dtype, stream);
}

extern "C" int kinet_bottleneck_pair_ds(const void* X, int ldx, const void* X0, int ldx0, const void* packed,
                                        const float* b3ds, const float* b1, void* Y, void* T, int M, int D, int F,
                                        int DB, int dtype, kinet_stream_t stream) {
    KINET_CHECK_ARG(D == 64, kPairDsWhyD, D);
    KINET_CHECK_ARG(F == 256, "bottleneck_pair_ds: F must be 256 (got %d)", F);
    KINET_CHECK_ARG(DB == 64, kPairDsWhyDB, DB);
    KINET_CHECK_ARG(M >= 0 && ldx >= 64 && ldx % 8 == 0 && ldx0 >= 64 && ldx0 % 8 == 0,
                    "bottleneck_pair_ds: bad M / ldx / ldx0 (row strides >= 64, multiples of 8)");
    KINET_CHECK_ARG(dt16(dtype), "bottleneck_pair_ds: dtype must be bf16 or f16");
    KINET_CHECK_ARG(b3ds && b1, "bottleneck_pair_ds: the combined bias b3 + b_ds and b1 are required");
    KINET_CHECK_ARG(X && X0 && packed && Y && T, "bottleneck_pair_ds: null pointer");
    KINET_CHECK_ARG(al16(X, X0, packed, Y, T, b3ds, b1), "bottleneck_pair_ds: tensors and BN biases must be 16-byte aligned");
    if (M == 0) return KINET_OK;
    const long long xb = extent(M, ldx, D), x0b = extent(M, ldx0, 64);
    const long long fb = (long long)M * F * 2;
    KINET_CHECK_ARG(xb < k2GiB && x0b < k2GiB && fb < k2GiB, "bottleneck_pair_ds: tensors larger than 2 GiB (split the call)");
    PairDsArgs a{};
    a.X = X; a.X0 = X0; a.W = packed; a.b3 = b3ds; a.b1 = b1; a.Y = Y; a.T = T;
    a.ldx = ldx; a.ldx0 = ldx0; a.M = M;
    a.x_bytes = (int)xb;
    a.x0_bytes = (int)x0b;
    a.y_bytes = (int)fb;
    a.w_bytes = (int)(ffn_pack_total(FFN_PACK_DS, D, F, DB) * 2);
    a.t_bytes = (int)((long long)M * DB * 2);
    return launch_planned(FFN_PAIR_DS, M, D, F, DB, dtype, a, stream);
}
