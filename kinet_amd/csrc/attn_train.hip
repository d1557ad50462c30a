// The f32 attention training pair for long key sets (vanilla DETR: every H*W key), on
// v_mfma_f32_16x16x4_f32 (bit-for-bit an f32 fmaf chain, so the numerics are those of the FMA
// kernels):
//  * kinet_mha_train_forward: key-streaming online softmax that also writes the per-row
//    log-sum-exp of the scaled scores over the unmasked keys;
//  * kinet_mha_train_backward: two kernels that recompute the probabilities tile by tile from that
//    log-sum-exp -- by query tile streaming keys (dQ, delta_i = dO_i . O_i), by key tile streaming
//    queries (dK, dV).  No workspace that grows with Lq * Lk, no atomics: every sum runs in a
//    fixed order, reruns are bit-identical.
// Geometry, LDS sizes and the launches: attn_train_plan.h.
//
// Lane maps (l = lane, c = l & 15, g = l >> 4): the A operand is A[row c][k g], the B operand
// B[k g][col c], the result D[row 4g + r][col c] in register r.  Every score tile is computed
// transposed to its use, so that the index the next product sums over lies in the registers: a
// wave's S^T tile (keys 4g + r, query c) is the B operand of O^T = V^T P^T register by register,
// with k = g of step r standing for key 4g + r on both operands; nothing moves between lanes.
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/kinet_grad.h"
#include "attn_train_plan.h"
#include "common.h"

namespace kinet {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int TQ = kAttnTrainQT, TK = kAttnTrainKT, TB = kAttnTrainBlock;
static_assert(TQ == 64 && TK == 64 && TB == 256, "4 waves x 16 rows, 4 16-row blocks per staged tile");

template <int D>
struct TrainCfg {
    static constexpr AttnTrainGeo G = attn_train_geo(D);
    static constexpr int KS = G.ks, DT = G.dt, SA = G.sa, ST = G.st;
    static constexpr int ROW = TK * SA, COL = TK * ST;   // floats of one image
};

struct TrainArgs {
    const float *Q, *K, *V, *O, *dO, *lse_in;
    float *Ow, *lse, *dQ, *dK, *dV, *delta;
    const uint8_t* key_mask;
    int ldq, ldk, ldv, ldo, lddo;
    int Lq, Lk, H;
    float scale;
    const int64_t* dseed;
    uint32_t dthresh;
    float dscale;
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// rows r0 .. r0 + 63 of src (row stride ld, D columns) into a 64-row LDS image of STRIDE floats per
// row; rows past `rows` and columns D .. COLS - 1 are zero
template <int D, int STRIDE, int COLS>
__device__ __forceinline__ void stage(float* dst, const float* __restrict__ src, long ld, int r0, int rows) {
    for (int e = threadIdx.x; e < 64 * COLS; e += TB) {
        const int r = e / COLS, d = e - r * COLS, rr = r0 + r;
        dst[r * STRIDE + d] = (rr < rows && d < D) ? src[(long)rr * ld + d] : 0.f;
    }
}
// both images of one tile from one read of global memory
template <int D, int SA, int ST, int COLS>
__device__ __forceinline__ void stage2(float* row, float* col, const float* __restrict__ src, long ld, int r0, int rows) {
    for (int e = threadIdx.x; e < 64 * COLS; e += TB) {
        const int r = e / COLS, d = e - r * COLS, rr = r0 + r;
        const float v = (rr < rows && d < D) ? src[(long)rr * ld + d] : 0.f;
        if (d < D) row[r * SA + d] = v;
        col[r * ST + d] = v;
    }
}

// this lane's operand registers of one row: element 4s + g of `p` (zero when !ok)
template <int KS>
__device__ __forceinline__ void load_frag(float (&f)[KS], const float* p, int g, bool ok) {
#pragma unroll
    for (int s = 0; s < KS; ++s) f[s] = ok ? p[4 * s + g] : 0.f;
}

// acc[b] += (rows 16b + c of the row image) . frag over the head dim, b = 0..3: four independent chains
template <int KS, int SA>
__device__ __forceinline__ void scores(f32x4 (&acc)[4], const float* img, const float (&frag)[KS], int c, int g) {
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] = mfma4(img[(16 * b + c) * SA + 4 * s + g], frag[s], acc[b]);
}

// out[t] += (col image)^T . w over the 64 staged rows; w[b][r] belongs to staged row 16b + 4g + r
template <int DT, int ST>
__device__ __forceinline__ void accumulate(f32x4 (&out)[DT], const float* img, const f32x4 (&w)[4], int c, int g) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < DT; ++t) out[t] = mfma4(img[(16 * b + 4 * g + r) * ST + 16 * t + c], w[b][r], out[t]);
}

__device__ __forceinline__ float group_sum(float v) {   // over the four lanes c, c + 16, c + 32, c + 48
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// out^T (registers: dim 16t + 4g + r, lane column c) times f into row `p` (D columns)
template <int D, int DT>
__device__ __forceinline__ void store_t(float* p, const f32x4 (&out)[DT], float f, int g) {
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 16 * t + 4 * g + r;
            if (d < D) p[d] = out[t][r] * f;
        }
}

// ------------------------------------------------------------------------------------- forward
template <int D>
__global__ __launch_bounds__(TB) void mha_train_fwd_kernel(TrainArgs a) {
    using C = TrainCfg<D>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Kr = smem;
    float* Vc = Kr + C::ROW;
    float* bias = Vc + C::COL;
    const int b = blockIdx.z, h = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4;
    const int i = blockIdx.x * TQ + wave * 16 + c;
    const bool iv = i < a.Lq;
    const long bh = (long)b * a.H + h;
    float q[C::KS];
    load_frag<C::KS>(q, a.Q + ((long)b * a.Lq + (iv ? i : 0)) * a.ldq + h * D, g, iv);
    const float* Kb = a.K + (long)b * a.Lk * a.ldk + h * D;
    const float* Vb = a.V + (long)b * a.Lk * a.ldv + h * D;
    const uint8_t* km = a.key_mask ? a.key_mask + (long)b * a.Lk : nullptr;
    // dropout: dropped probabilities leave the numerator only (F.dropout after the softmax)
    const uint64_t seed = a.dseed ? (uint64_t)*a.dseed : 0ull;
    const uint64_t drow = ((uint64_t)bh * (uint64_t)a.Lq + (uint64_t)(iv ? i : 0)) * (uint64_t)a.Lk;
    float m = -INFINITY, l = 0.f;   // l: this lane's part of the row sum (its keys 4g + r of every block)
    f32x4 o[C::DT];
#pragma unroll
    for (int t = 0; t < C::DT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.Lk; k0 += TK) {
        __syncthreads();
        stage<D, C::SA, D>(Kr, Kb, a.ldk, k0, a.Lk);
        stage<D, C::ST, 16 * C::DT>(Vc, Vb, a.ldv, k0, a.Lk);
        if (threadIdx.x < TK) {
            const int j = k0 + threadIdx.x;
            bias[threadIdx.x] = (j < a.Lk && !(km && km[j])) ? 0.f : -INFINITY;
        }
        __syncthreads();
        f32x4 s[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        scores<C::KS, C::SA>(s, Kr, q, c, g);
        float tm = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kb][r] = s[kb][r] * a.scale + bias[16 * kb + 4 * g + r];
                tm = fmaxf(tm, s[kb][r]);
            }
        tm = fmaxf(tm, __shfl_xor(tm, 16));
        tm = fmaxf(tm, __shfl_xor(tm, 32));
        const float mn = fmaxf(m, tm);
        const float mu = mn == -INFINITY ? 0.f : mn;     // no unmasked key yet: every exp below is 0
        const float corr = expf(m - mu);
        l *= corr;
#pragma unroll
        for (int t = 0; t < C::DT; ++t) o[t] *= corr;
        m = mn;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = expf(s[kb][r] - mu);
                l += p;
                const int j = k0 + 16 * kb + 4 * g + r;
                s[kb][r] = a.dseed ? (dropout_keep(seed, drow + (uint64_t)j, a.dthresh) ? p * a.dscale : 0.f) : p;
            }
        accumulate<C::DT, C::ST>(o, Vc, s, c, g);
    }
    l = group_sum(l);
    if (!iv) return;
    // a row with no unmasked key: O = 0 (as kinet_mha_core_dropout), lse = -inf
    store_t<D, C::DT>(a.Ow + ((long)b * a.Lq + i) * a.ldo + h * D, o, l > 0.f ? 1.f / l : 0.f, g);
    if (g == 0) a.lse[bh * a.Lq + i] = l > 0.f ? m + logf(l) : -INFINITY;
}

// P_ij from the saved statistics; -inf - -inf never reaches expf
__device__ __forceinline__ float prob(float x, float lse) { return lse == -INFINITY ? 0.f : expf(x - lse); }

// ------------------------------------------------------------------- backward by query tile
// dQ_i = scale * sum_j dS_ij K_j, dS_ij = P_ij (Z_ij dP_ij - delta_i), dP_ij = dO_i . V_j
template <int D>
__global__ __launch_bounds__(TB) void mha_train_dq_kernel(TrainArgs a) {
    using C = TrainCfg<D>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Kr = smem;
    float* Vr = Kr + C::ROW;
    float* Kc = Vr + C::ROW;
    float* bias = Kc + C::COL;
    const int b = blockIdx.z, h = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4;
    const int i = blockIdx.x * TQ + wave * 16 + c;
    const bool iv = i < a.Lq;
    const long bh = (long)b * a.H + h;
    const long row = (long)b * a.Lq + (iv ? i : 0);
    float q[C::KS], go[C::KS];
    load_frag<C::KS>(q, a.Q + row * a.ldq + h * D, g, iv);
    load_frag<C::KS>(go, a.dO + row * a.lddo + h * D, g, iv);
    // delta_i = dO_i . O_i as the diagonal of the wave's O dO^T tile, i.e. by the very chain that gives
    // dP_ij = dO_i . V_j below: with one unmasked key (O_i = V_j bit for bit) dP - delta is exactly 0
    float delta;
    {
        float ov[C::KS];
        load_frag<C::KS>(ov, a.O + row * a.ldo + h * D, g, iv);
        f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < C::KS; ++s) t = mfma4(ov[s], go[s], t);
        // element (row 4g + r, column c) sits in register r of lane (c, g): the diagonal of column c in
        // lane (c, c >> 2), register c & 3
        const int r = c & 3;
        const float diag = r == 0 ? t[0] : r == 1 ? t[1] : r == 2 ? t[2] : t[3];
        delta = __shfl(diag, c + 16 * (c >> 2));
        if (iv && g == 0) a.delta[bh * a.Lq + i] = delta;
    }
    const float lse = iv ? a.lse_in[bh * a.Lq + i] : -INFINITY;
    const float* Kb = a.K + (long)b * a.Lk * a.ldk + h * D;
    const float* Vb = a.V + (long)b * a.Lk * a.ldv + h * D;
    const uint8_t* km = a.key_mask ? a.key_mask + (long)b * a.Lk : nullptr;
    const uint64_t seed = a.dseed ? (uint64_t)*a.dseed : 0ull;
    const uint64_t drow = ((uint64_t)bh * (uint64_t)a.Lq + (uint64_t)(iv ? i : 0)) * (uint64_t)a.Lk;
    f32x4 dq[C::DT];
#pragma unroll
    for (int t = 0; t < C::DT; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.Lk; k0 += TK) {
        __syncthreads();
        stage2<D, C::SA, C::ST, 16 * C::DT>(Kr, Kc, Kb, a.ldk, k0, a.Lk);
        stage<D, C::SA, D>(Vr, Vb, a.ldv, k0, a.Lk);
        if (threadIdx.x < TK) {
            const int j = k0 + threadIdx.x;
            bias[threadIdx.x] = (j < a.Lk && !(km && km[j])) ? 0.f : -INFINITY;
        }
        __syncthreads();
        f32x4 s[4], dp[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s[kb] = dp[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        scores<C::KS, C::SA>(s, Kr, q, c, g);
        scores<C::KS, C::SA>(dp, Vr, go, c, g);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * kb + 4 * g + r;
                const float p = prob(s[kb][r] * a.scale + bias[jl], lse);
                const float z = a.dseed ? (dropout_keep(seed, drow + (uint64_t)(k0 + jl), a.dthresh) ? a.dscale : 0.f) : 1.f;
                s[kb][r] = p * (z * dp[kb][r] - delta);
            }
        accumulate<C::DT, C::ST>(dq, Kc, s, c, g);
    }
    if (iv) store_t<D, C::DT>(a.dQ + row * a.ldq + h * D, dq, a.scale, g);
}

// --------------------------------------------------------------------- backward by key tile
// dK_j = scale * sum_i dS_ij Q_i, dV_j = sum_i P_ij Z_ij dO_i; the wave's 16 keys ride on the lane
// column, the streamed queries on the registers
template <int D>
__global__ __launch_bounds__(TB) void mha_train_dkv_kernel(TrainArgs a) {
    using C = TrainCfg<D>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qr = smem;
    float* Gr = Qr + C::ROW;
    float* Qc = Gr + C::ROW;
    float* Gc = Qc + C::COL;
    float* lse_s = Gc + C::COL;
    float* del_s = lse_s + TQ;
    const int b = blockIdx.z, h = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4;
    const int j = blockIdx.x * TK + wave * 16 + c;
    const bool jv = j < a.Lk;
    const long bh = (long)b * a.H + h;
    const long row = (long)b * a.Lk + (jv ? j : 0);
    float kf[C::KS], vf[C::KS];
    load_frag<C::KS>(kf, a.K + row * a.ldk + h * D, g, jv);
    load_frag<C::KS>(vf, a.V + row * a.ldv + h * D, g, jv);
    const float kbias = (jv && !(a.key_mask && a.key_mask[row])) ? 0.f : -INFINITY;
    const float* Qb = a.Q + (long)b * a.Lq * a.ldq + h * D;
    const float* Gb = a.dO + (long)b * a.Lq * a.lddo + h * D;
    const uint64_t seed = a.dseed ? (uint64_t)*a.dseed : 0ull;
    f32x4 dk[C::DT], dv[C::DT];
#pragma unroll
    for (int t = 0; t < C::DT; ++t) dk[t] = dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < a.Lq; i0 += TQ) {
        __syncthreads();
        stage2<D, C::SA, C::ST, 16 * C::DT>(Qr, Qc, Qb, a.ldq, i0, a.Lq);
        stage2<D, C::SA, C::ST, 16 * C::DT>(Gr, Gc, Gb, a.lddo, i0, a.Lq);
        if (threadIdx.x < TQ) {
            const int i = i0 + threadIdx.x;
            lse_s[threadIdx.x] = i < a.Lq ? a.lse_in[bh * a.Lq + i] : -INFINITY;   // rows past Lq: P = 0
            del_s[threadIdx.x] = i < a.Lq ? a.delta[bh * a.Lq + i] : 0.f;
        }
        __syncthreads();
        f32x4 s[4], dp[4];
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) s[qb] = dp[qb] = f32x4{0.f, 0.f, 0.f, 0.f};
        scores<C::KS, C::SA>(s, Qr, kf, c, g);
        scores<C::KS, C::SA>(dp, Gr, vf, c, g);
#pragma unroll
        for (int qb = 0; qb < 4; ++qb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = 16 * qb + 4 * g + r;
                const float p = prob(s[qb][r] * a.scale + kbias, lse_s[il]);
                float z = 1.f;
                if (a.dseed) {
                    const uint64_t idx = ((uint64_t)bh * (uint64_t)a.Lq + (uint64_t)(i0 + il)) * (uint64_t)a.Lk + (uint64_t)(jv ? j : 0);
                    z = dropout_keep(seed, idx, a.dthresh) ? a.dscale : 0.f;
                }
                s[qb][r] = p * (z * dp[qb][r] - del_s[il]);
                dp[qb][r] = p * z;
            }
        accumulate<C::DT, C::ST>(dv, Gc, dp, c, g);
        accumulate<C::DT, C::ST>(dk, Qc, s, c, g);
    }
    if (!jv) return;
    store_t<D, C::DT>(a.dV + row * a.ldv + h * D, dv, 1.f, g);
    store_t<D, C::DT>(a.dK + row * a.ldk + h * D, dk, a.scale, g);
}

thread_local int train_calls = 0;   // kinet_mha_train_forward launches of the calling thread

int check_problem(const char* who, int batch, int Lq, int Lk, int heads, int head_dim, float dropout_p,
                  const int64_t* dropout_seed, AttnTrainPlan& pl) {
    KINET_CHECK_ARG(batch >= 0 && Lq >= 0 && Lk >= 0 && heads > 0, "%s: bad sizes", who);
    KINET_CHECK_ARG(attn_train_geo(head_dim).d != 0, "%s: head_dim %d not instantiated (32/36)", who, head_dim);
    KINET_CHECK_ARG(batch <= kAttnTrainMaxGridYZ && heads <= kAttnTrainMaxGridYZ, "%s: batch %d / heads %d beyond the grid limit %d",
                    who, batch, heads, kAttnTrainMaxGridYZ);
    KINET_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f && (dropout_p == 0.f || dropout_seed),
                    "%s: dropout p %g must be in [0, 1) with a seed", who, (double)dropout_p);
    pl = attn_train_plan(AttnTrainProblem{head_dim, batch, heads, Lq, Lk});
    return KINET_OK;
}

template <typename Kern>
void launch(Kern kern, const AttnTrainLaunch& ln, const TrainArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(kern, dim3(ln.grid[0], ln.grid[1], ln.grid[2]), dim3(ln.block), ln.lds, s, a);
}

}  // namespace
}  // namespace kinet

using namespace kinet;

extern "C" int kinet_mha_train_plan(const int* problem, int* plan_out) {
    KINET_CHECK_ARG(problem != nullptr && plan_out != nullptr, "mha train plan: invalid arguments");
    const int* f = problem;
    KINET_CHECK_ARG(f[KINET_MHATP_BATCH] >= 0 && f[KINET_MHATP_LQ] >= 0 && f[KINET_MHATP_LK] >= 0 && f[KINET_MHATP_HEADS] > 0,
                    "mha train plan: bad sizes");
    const AttnTrainPlan pl = attn_train_plan(AttnTrainProblem{f[KINET_MHATP_HEAD_DIM], f[KINET_MHATP_BATCH],
                                                              f[KINET_MHATP_HEADS], f[KINET_MHATP_LQ], f[KINET_MHATP_LK]});
    const AttnTrainGeo g = attn_train_geo(f[KINET_MHATP_HEAD_DIM]);
    int* o = plan_out;
    o[KINET_MHATPL_SUPPORTED] = pl.supported;
    o[KINET_MHATPL_DENSE_DEFAULT] = pl.supported && pl.dense_default;
    o[KINET_MHATPL_QT] = kAttnTrainQT;
    o[KINET_MHATPL_KT] = kAttnTrainKT;
    o[KINET_MHATPL_ROW_STRIDE] = g.sa;
    o[KINET_MHATPL_COL_STRIDE] = g.st;
    const AttnTrainLaunch* ls[3] = {&pl.fwd, &pl.dq, &pl.dkv};
    for (int k = 0; k < 3; ++k) {
        int* r = o + KINET_MHATPL_FWD + 5 * k;
        r[0] = ls[k]->grid[0], r[1] = ls[k]->grid[1], r[2] = ls[k]->grid[2], r[3] = ls[k]->block, r[4] = ls[k]->lds;
    }
    return KINET_OK;
}

extern "C" int kinet_mha_train_calls(void) { return train_calls; }

extern "C" int kinet_mha_train_forward(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O,
                                       int ldo, float* lse, int batch, int Lq, int Lk, int heads, int head_dim, float scale,
                                       const uint8_t* key_mask, float dropout_p, const int64_t* dropout_seed,
                                       kinet_stream_t stream) {
    AttnTrainPlan pl;
    if (const int rc = check_problem("mha_train_forward", batch, Lq, Lk, heads, head_dim, dropout_p, dropout_seed, pl)) return rc;
    if (pl.fwd.grid[0] == 0) return KINET_OK;
    KINET_CHECK_ARG(Q && O && lse && (Lk == 0 || (K && V)), "mha_train_forward: null operand");
    const int E = heads * head_dim;
    KINET_CHECK_ARG(ldq >= E && ldk >= E && ldv >= E && ldo >= E, "mha_train_forward: row strides below heads * head_dim = %d", E);
    const bool drop = dropout_p > 0.f;
    TrainArgs a{};
    a.Q = Q, a.K = K, a.V = V, a.Ow = O, a.lse = lse, a.key_mask = key_mask;
    a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.ldo = ldo;
    a.Lq = Lq, a.Lk = Lk, a.H = heads, a.scale = scale;
    a.dseed = drop ? dropout_seed : nullptr, a.dthresh = dropout_thresh(dropout_p), a.dscale = drop ? 1.f / (1.f - dropout_p) : 1.f;
    ++train_calls;
    if (head_dim == 32) launch(mha_train_fwd_kernel<32>, pl.fwd, a, (hipStream_t)stream);
    else launch(mha_train_fwd_kernel<36>, pl.fwd, a, (hipStream_t)stream);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}

extern "C" int64_t kinet_mha_train_backward_workspace(int batch, int Lq, int heads) {
    return attn_train_backward_workspace(batch, Lq, heads);
}

extern "C" int kinet_mha_train_backward(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv,
                                        const float* O, int ldo, const float* dO, int lddo, const float* lse, float* dQ,
                                        float* dK, float* dV, int batch, int Lq, int Lk, int heads, int head_dim, float scale,
                                        const uint8_t* key_mask, float* workspace, float dropout_p,
                                        const int64_t* dropout_seed, kinet_stream_t stream) {
    AttnTrainPlan pl;
    if (const int rc = check_problem("mha_train_backward", batch, Lq, Lk, heads, head_dim, dropout_p, dropout_seed, pl)) return rc;
    if (pl.dq.grid[0] == 0) return KINET_OK;
    KINET_CHECK_ARG(Q && O && dO && lse && dQ && (Lk == 0 || (K && V && dK && dV)), "mha_train_backward: null operand");
    KINET_CHECK_ARG(workspace, "mha_train_backward: needs kinet_mha_train_backward_workspace floats of workspace");
    const int E = heads * head_dim;
    KINET_CHECK_ARG(ldq >= E && ldk >= E && ldv >= E && ldo >= E && lddo >= E,
                    "mha_train_backward: row strides below heads * head_dim = %d", E);
    const bool drop = dropout_p > 0.f;
    TrainArgs a{};
    a.Q = Q, a.K = K, a.V = V, a.O = O, a.dO = dO, a.lse_in = lse, a.dQ = dQ, a.dK = dK, a.dV = dV, a.delta = workspace;
    a.key_mask = key_mask;
    a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.ldo = ldo, a.lddo = lddo;
    a.Lq = Lq, a.Lk = Lk, a.H = heads, a.scale = scale;
    a.dseed = drop ? dropout_seed : nullptr, a.dthresh = dropout_thresh(dropout_p), a.dscale = drop ? 1.f / (1.f - dropout_p) : 1.f;
    hipStream_t s = (hipStream_t)stream;
    if (head_dim == 32) launch(mha_train_dq_kernel<32>, pl.dq, a, s);
    else launch(mha_train_dq_kernel<36>, pl.dq, a, s);
    KINET_LAUNCH_CHECK();
    if (pl.dkv.grid[0] == 0) return KINET_OK;
    if (head_dim == 32) launch(mha_train_dkv_kernel<32>, pl.dkv, a, s);
    else launch(mha_train_dkv_kernel<36>, pl.dkv, a, s);
    KINET_LAUNCH_CHECK();
    return KINET_OK;
}
