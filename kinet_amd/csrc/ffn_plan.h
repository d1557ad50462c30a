// Host-side planning of the launches of ffn.hip (the fused FFN, the attention out-projection + FFN
// and the ResNet bottleneck pairs): the fragment geometry and LDS footprint of each kernel family,
// the table of the instantiations that exist, the named bits of kinet_ffn_set_debug, the pure
// function that turns a described problem into one launch of a table entry (or the refusal's
// message), and the one definition of the packed-weight layout.  ffn.hip generates its kernel
// instantiations and its launcher from the table and packs through ffn_pack_src.  No HIP, no
// thread-locals and no device query in this file: it runs on a machine without a GPU
// (kinet_ffn_launch_plan, kinet_ffn_pack_map, tests/test_ffn_plan_cpu.py).
#pragma once
#include "../../include/kinet_common.h"

#ifdef __HIPCC__
#define KINET_FFN_HD __host__ __device__
#else
#define KINET_FFN_HD
#endif

namespace kinet {

// ---------------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------------
template <int D>
struct FfnGeo {
    static_assert(D % 32 == 0, "D must be a multiple of 32");
    static constexpr int KS = D / 32;        // 32-deep K steps of linear1
    static constexpr int NT = D / 16;        // 16-wide output tiles of linear2
    static constexpr int FR = 2 * KS + NT;   // 1-KiB fragments per 32-unit hidden chunk
    static constexpr int CHUNK = FR * 1024;
};
// FfnGeo<D>::FR for a run-time D
constexpr int ffn_fr(int D) { return 2 * (D / 32) + D / 16; }

constexpr int FFN_MAX_F = 2048;
constexpr int kFfnLdsLimit = 160 * 1024;   // what one workgroup may hold; a CU's LDS

// output column of MFMA row m of phase-B tile nt: lane group g holds, for the tile pair
// (2kp, 2kp+1), the 8 consecutive columns 32kp + 8g .. +7 -- the same columns its phase-A
// x fragment xr[kp] holds, so the residual comes from registers and stores are 16 bytes
KINET_FFN_HD constexpr int ffn_sigma(int nt, int m) { return 32 * (nt >> 1) + 8 * (m >> 2) + 4 * (nt & 1) + (m & 3); }

// ---------------------------------------------------------------------------------
// the instantiations that exist
// ---------------------------------------------------------------------------------
enum FfnFamily {
    FFN_K_FUSED = 0,    // ffn_fused_kernel<T, D, RT, WAVES>
    FFN_K_RT2 = 1,      // ffn_fused_rt2_kernel<T, D, PRE, RV>
    FFN_K_PAIR = 2,     // bneck_pair_kernel<T, D, RT, WAVES>
    FFN_K_B64 = 3,      // bneck64_kernel<T, DB, WAVES>
    FFN_K_B64_DS = 4,   // bneck64_ds_kernel<T, RT>
};

// One instantiation but for the element type (each exists for bf16 and f16).
struct FfnKernel {
    int family;
    int d, rt, waves;    // template selectors; d = the operand width (64 for both bneck64 families)
    int db;              // FFN_K_B64: the next conv1's output width
    bool pre;            // FFN_K_RT2: the attention out-projection pre-phase
    int rv;              // FFN_K_RT2 with pre: where the residual is loaded
    int ns;              // ring slots (0: the weights are resident)
    int tile_rows;       // rows of one of the kernel's `ntiles` row tiles
    int wg_tiles;        // row tiles a workgroup works on at a time: 1 (the ring kernels: the workgroup's
                         // waves share the tile) or `waves` (resident weights: every wave on its own tile)
    int wg_per_cu;       // resident workgroups per CU the grid is sized for
    const char* name;
    constexpr int block() const { return waves * 64; }
    constexpr int wg_rows() const { return tile_rows * wg_tiles; }
};

// LDS bytes of a workgroup: parameter block + ring slots x slot size, or the resident weight block
// + parameters.  ffn.hip static_asserts each kernel's own arrays against these.
constexpr int ffn_fused_lds(int D, int ns, bool pre) { return (FFN_MAX_F + (pre ? 6 : 3) * D) * 4 + ns * ffn_fr(D) * 1024; }
constexpr int bneck_pair_lds(int D, int ns, int rows) { return (4 * D + D) * 4 + ns * (ffn_fr(D) * 1024 + rows * 64); }
// na = 16-bit matrices in phase A (W3; W3 and W_ds), D = 64, F = 256
constexpr int bneck64_lds(int na, int DB) { return (256 / 32) * (na * 4 + DB / 16) * 1024 + (256 + DB) * 4; }
constexpr int ffn_kernel_lds(const FfnKernel& k) {
    return k.family == FFN_K_FUSED || k.family == FFN_K_RT2 ? ffn_fused_lds(k.d, k.ns, k.pre)
           : k.family == FFN_K_PAIR                           ? bneck_pair_lds(k.d, k.ns, k.tile_rows)
           : k.family == FFN_K_B64                            ? bneck64_lds(1, k.db)
                                                              : bneck64_lds(2, 64);
}

constexpr FfnKernel kFfnKernels[] = {
    // family, d, rt, waves, db, pre, rv, ns, tile_rows, wg_tiles, wg_per_cu
    {FFN_K_FUSED, 256, 2, 4, 0, false, 0, 4, 128, 1, 1, "ffn_fused_kernel<256, 2, 4>"},
    {FFN_K_FUSED, 256, 1, 8, 0, false, 0, 4, 128, 1, 1, "ffn_fused_kernel<256, 1, 8>"},
    {FFN_K_FUSED, 256, 1, 4, 0, false, 0, 4, 64, 1, 1, "ffn_fused_kernel<256, 1, 4>"},
    {FFN_K_FUSED, 288, 2, 4, 0, false, 0, 4, 128, 1, 1, "ffn_fused_kernel<288, 2, 4>"},
    {FFN_K_FUSED, 288, 1, 4, 0, false, 0, 4, 64, 1, 1, "ffn_fused_kernel<288, 1, 4>"},
    {FFN_K_RT2, 256, 2, 8, 0, false, 0, 3, 256, 1, 1, "ffn_fused_rt2_kernel<256>"},
    {FFN_K_RT2, 256, 2, 8, 0, true, 0, 3, 256, 1, 1, "ffn_fused_rt2_kernel<256, true>"},
    {FFN_K_RT2, 256, 2, 8, 0, true, 1, 3, 256, 1, 1, "ffn_fused_rt2_kernel<256, true, 1>"},
    {FFN_K_PAIR, 64, 2, 8, 64, false, 0, 3, 256, 1, 2, "bneck_pair_kernel<64, 2, 8>"},
    {FFN_K_PAIR, 128, 1, 8, 128, false, 0, 3, 128, 1, 1, "bneck_pair_kernel<128, 1, 8>"},
    {FFN_K_PAIR, 128, 2, 8, 128, false, 0, 3, 256, 1, 1, "bneck_pair_kernel<128, 2, 8>"},
    {FFN_K_PAIR, 256, 1, 8, 256, false, 0, 3, 128, 1, 1, "bneck_pair_kernel<256, 1, 8>"},
    {FFN_K_PAIR, 256, 2, 8, 256, false, 0, 3, 256, 1, 1, "bneck_pair_kernel<256, 2, 8>"},
    // resident weights: 96 KiB -> one 16-wave workgroup per CU; 64 KiB -> two 8-wave workgroups
    {FFN_K_B64, 64, 1, 16, 128, false, 0, 0, 16, 16, 1, "bneck64_kernel<128, 16>"},
    {FFN_K_B64, 64, 1, 8, 64, false, 0, 0, 16, 8, 2, "bneck64_kernel<64, 8>"},
    {FFN_K_B64_DS, 64, 1, 16, 64, false, 0, 0, 16, 16, 1, "bneck64_ds_kernel<1>"},
    {FFN_K_B64_DS, 64, 2, 16, 64, false, 0, 0, 32, 16, 1, "bneck64_ds_kernel<2>"},
};
constexpr int kNumFfnKernels = (int)(sizeof(kFfnKernels) / sizeof(kFfnKernels[0]));

// the entry with these selectors; -1 = no such instantiation
constexpr int ffn_kernel_index(int family, int d, int rt, int waves, int db = 0, bool pre = false, int rv = 0) {
    for (int i = 0; i < kNumFfnKernels; ++i) {
        const FfnKernel& k = kFfnKernels[i];
        if (k.family == family && k.d == d && k.rt == rt && k.waves == waves && (family < FFN_K_PAIR || k.db == db) &&
            k.pre == pre && k.rv == rv)
            return i;
    }
    return -1;
}

// what must hold for every entry of the table
template <typename F> constexpr bool ffn_every_kernel(F ok) {
    for (int i = 0; i < kNumFfnKernels; ++i)
        if (!ok(kFfnKernels[i])) return false;
    return true;
}
static_assert(ffn_every_kernel([](const FfnKernel& k) { return ffn_kernel_lds(k) <= kFfnLdsLimit; }), "LDS: one workgroup");
static_assert(ffn_every_kernel([](const FfnKernel& k) { return ffn_kernel_lds(k) * k.wg_per_cu <= kFfnLdsLimit; }),
              "LDS: wg_per_cu workgroups per CU");
static_assert(ffn_every_kernel([](const FfnKernel& k) { return k.block() * k.wg_per_cu <= 1024 && k.block() <= 1024; }),
              "wave slots: the wg_per_cu workgroups a grid counts on per CU are at most 16 waves");
static_assert(ffn_every_kernel([](const FfnKernel& k) {
                  return k.ns ? k.wg_tiles == 1 && k.tile_rows == k.waves * 16 * k.rt : k.wg_tiles == k.waves && k.tile_rows == 16 * k.rt;
              }), "a ring kernel's waves share one tile of 16 rt rows each; resident weights: a 16 rt-row tile per wave");
static_assert(ffn_every_kernel([](const FfnKernel& k) { return k.ns == 0 || ffn_fr(k.d) % k.waves == 0; }),
              "whole DMA rounds per chunk");
constexpr bool ffn_kernels_distinct() {
    for (int i = 0; i < kNumFfnKernels; ++i) {
        const FfnKernel& k = kFfnKernels[i];
        if (ffn_kernel_index(k.family, k.d, k.rt, k.waves, k.db, k.pre, k.rv) != i) return false;
    }
    return true;
}
static_assert(ffn_kernels_distinct(), "no entry twice");

// ---------------------------------------------------------------------------------
// diagnostic knobs (kinet_ffn_set_debug), per calling thread
// ---------------------------------------------------------------------------------
enum FfnDebug {
    FFN_DBG_NO_DMA = 1,        // no weight DMA after the prologue (timing only, results are garbage);
                               // not a planning input: it travels to the kernel in FfnArgs::dbg
    FFN_DBG_4W_RT2 = 2,        // the 4-wave x 32-row tile at D = 256
    FFN_DBG_8W_RT1 = 8,        // the 8-wave x 16-row tile (default: 8 waves x 32 rows, ffn_fused_rt2_kernel)
    FFN_DBG_PAIR64_RING = 16,  // kinet_bottleneck_pair at D = 64 on the LDS-ring kernel (bneck_pair_kernel)
    FFN_DBG_ATTN_RV1 = 64,     // kinet_attn_out_ffn_fused stages its residual loads under the Wo chunks (RV = 1)
    FFN_DBG_PAIR_RT1 = 128,    // 128 / 256 = kinet_bottleneck_pair at D = 128 / 256 on 1- / 2-row-tile waves
    FFN_DBG_PAIR_RT2 = 256,
    FFN_DBG_DS_RT2 = 512,      // kinet_bottleneck_pair_ds on 2-row-tile waves (bneck64_ds_kernel<T, 2>)
};

// ---------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------
enum FfnKind { FFN_FFN = 0, FFN_ATTN_OUT = 1, FFN_PAIR = 2, FFN_PAIR_DS = 3 };   // the entry point

// kinet_ffn_fused takes the 8-wave x 32-row tile from this many rows (kinet_attn_out_ffn_fused runs
// on that tile only: kernels.ATTN_OUT_FFN_MIN_ROWS)
constexpr int kFfnRt2MinRows = 16384;

struct FfnProblem {
    int kind;      // FfnKind
    int M, D, F, DB;
    int dbg;       // FfnDebug bits of the calling thread
    bool solo;     // kinet_set_solo_launch: one batch in flight
    int cus;       // compute units of the device
    int cap;       // kinet_ffn_grid_cap of the calling thread (0 = none)
};
struct FfnPlan {
    int kernel;    // index into kFfnKernels
    int tiles;     // the kernel's ntiles: row tiles of FfnKernel::tile_rows rows
    int grid;
    // refusal (ffn_plan() == false): printf format of the entry point's message and its %d arguments
    const char* why;
    int why_arg[2];
};

// the messages of the entry points' checks that the planner repeats
constexpr char kFfnWhyD[] = "ffn_fused: D must be 256 or 288 (got %d)";
constexpr char kAttnOutWhyD288[] =
    "attn_out_ffn_fused: D = 288 is not supported (Wo does not fill whole ring chunks); D must be 256";
constexpr char kAttnOutWhyD[] = "attn_out_ffn_fused: D must be 256 (got %d)";
constexpr char kPairWhyD[] = "bottleneck_pair: D must be 64, 128 or 256 (got %d)";
constexpr char kPairWhyDB[] = "bottleneck_pair: DB must be D, or 128 at D = 64 (got D=%d DB=%d)";
constexpr char kPairDsWhyD[] = "bottleneck_pair_ds: D must be 64 (got %d)";
constexpr char kPairDsWhyDB[] = "bottleneck_pair_ds: DB must be 64 (got %d)";

inline bool ffn_refuse(FfnPlan& pl, const char* why, int a = 0, int b = 0) {
    pl.why = why;
    pl.why_arg[0] = a;
    pl.why_arg[1] = b;
    return false;
}

// ceil(a / b) in 64 bits
constexpr long long ffn_ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// the row tiles of kernel k over M rows
constexpr long long ffn_tiles(int k, int M) { return ffn_ceil_div(M, kFfnKernels[k].tile_rows); }

// The launch of `p`: true with pl.kernel / tiles / grid (M == 0: grid 0, nothing to launch), false with
// pl.why the refusal.
inline bool ffn_plan(const FfnProblem& p, FfnPlan& pl) {
    pl = FfnPlan{};
    pl.kernel = -1;
    const int D = p.D;
    switch (p.kind) {
    case FFN_FFN:
        if (D != 256 && D != 288) return ffn_refuse(pl, kFfnWhyD, D);
        // persistent: one workgroup per CU walks row tiles.  Many rows: 4 waves x 32 rows (128
        // rows share each weight byte; the 2 x D/16 output tiles + 2 x D/32 x-fragments (+ the
        // next tile's prefetch) need > 256 VGPRs, so one wave per SIMD);  few rows (decoder
        // queries): 4 waves x 16 rows, so the rows spread over more CUs
        if (p.M >= kFfnRt2MinRows) {
            if (ffn_fr(D) % 8 == 0) {
                if (p.dbg & FFN_DBG_4W_RT2) {   // A/B knob: 4 waves x 32 rows (one wave per SIMD)
                    pl.kernel = ffn_kernel_index(FFN_K_FUSED, D, 2, 4);
                } else if (p.dbg & FFN_DBG_8W_RT1) {   // A/B knob: 8 waves x 16 rows (the round-3 default)
                    pl.kernel = ffn_kernel_index(FFN_K_FUSED, D, 1, 8);
                } else {
                    // 8 waves x 32 rows: each weight fragment feeds two MFMAs and two waves per SIMD hide
                    // each other's latency (config-2 encoder FFN at batch 16: 419 vs 486 us alone, bench
                    // 1267 vs 1219 frames/s, profiles/r04c_ffn_probe.log, r04c_ab_*.json)
                    pl.kernel = ffn_kernel_index(FFN_K_RT2, D, 2, 8);
                }
            } else {
                pl.kernel = ffn_kernel_index(FFN_K_FUSED, D, 2, 4);
            }
        } else {
            pl.kernel = ffn_kernel_index(FFN_K_FUSED, D, 1, 4);
        }
        break;
    case FFN_ATTN_OUT:
        if (D == 288) return ffn_refuse(pl, kAttnOutWhyD288);
        if (D != 256) return ffn_refuse(pl, kAttnOutWhyD, D);
        // persistent like the FFN's 8-wave x 32-row case, the only tile with the pre-phase.
        // residual loads: all after the last Wo chunk (715 us per batch-28 encoder layer) or, A/B knob,
        // staged under the Wo chunks (732 us: no faster, profiles/attn_out_ffn_probe.txt)
        pl.kernel = ffn_kernel_index(FFN_K_RT2, D, 2, 8, 0, true, (p.dbg & FFN_DBG_ATTN_RV1) ? 1 : 0);
        break;
    case FFN_PAIR:
        if (D != 64 && D != 128 && D != 256) return ffn_refuse(pl, kPairWhyD, D);
        if (D == 64 && p.DB == 128) {
            pl.kernel = ffn_kernel_index(FFN_K_B64, 64, 1, 16, 128);
        } else if (p.DB != D) {
            return ffn_refuse(pl, kPairWhyDB, D, p.DB);
        } else if (D == 64) {
            if (p.dbg & FFN_DBG_PAIR64_RING)   // A/B knob: the LDS-ring pair kernel at D = 64 too
                pl.kernel = ffn_kernel_index(FFN_K_PAIR, 64, 2, 8, 64);
            else
                pl.kernel = ffn_kernel_index(FFN_K_B64, 64, 1, 8, 64);
        } else {
            // one or two 16-row tiles per wave (128- or 256-row workgroup tiles; the same sums per
            // element either way): the 2-tile tile reads each weight fragment once for two MFMAs,
            // but with one batch in flight (kinet_set_solo_launch), when its tiles fill their rounds
            // of one workgroup per CU 1.5x worse than the 1-tile grid, the 1-tile grid wins --
            // config 5's stage-3 pairs (M = 32,640: 128 vs 255 tiles on 256 CUs) 84.7 -> 62.9 us
            // alone (profiles/r06aa_config5_shapes.txt); on 3 streams the other batches fill the
            // idle CUs (neutral, profiles/r06ab_solo_launch_ab.txt).
            // ffn_debug 128 / 256 force the 1- / 2-tile grid (tests, A/B)
            const int k1 = ffn_kernel_index(FFN_K_PAIR, D, 1, 8, D), k2 = ffn_kernel_index(FFN_K_PAIR, D, 2, 8, D);
            const long long cus = p.cus;
            const long long t2 = ffn_tiles(k2, p.M), t1 = ffn_tiles(k1, p.M);
            const double e2 = (double)t2 / (double)(((t2 + cus - 1) / cus) * cus);
            const double e1 = (double)t1 / (double)(((t1 + cus - 1) / cus) * cus);
            const bool one = (p.dbg & FFN_DBG_PAIR_RT1) || (!(p.dbg & FFN_DBG_PAIR_RT2) && p.solo && e1 > 1.5 * e2);
            pl.kernel = one ? k1 : k2;
        }
        break;
    case FFN_PAIR_DS:
        if (D != 64) return ffn_refuse(pl, kPairDsWhyD, D);
        if (p.DB != 64) return ffn_refuse(pl, kPairDsWhyDB, p.DB);
        // one 16-wave workgroup per CU (96 KiB of weights), as bneck64_kernel<T, 128, 16>;
        // A/B knob: two 16-row tiles per wave
        pl.kernel = ffn_kernel_index(FFN_K_B64_DS, 64, (p.dbg & FFN_DBG_DS_RT2) ? 2 : 1, 16, 64);
        break;
    default: return ffn_refuse(pl, "ffn plan: unknown kind %d", p.kind);
    }
    // (every rule above names an entry of the table)
    const FfnKernel& k = kFfnKernels[pl.kernel];
    const long long tiles = ffn_tiles(pl.kernel, p.M);
    const long long wgs = ffn_ceil_div(tiles, k.wg_tiles), cap = (long long)p.cus * k.wg_per_cu;
    pl.tiles = (int)tiles;
    pl.grid = (int)(wgs < cap ? wgs : cap);
    // diagnostics: kinet_ffn_grid_cap bounds the grid -- every kernel walks its tiles by gridDim.x, so the
    // bound only moves tiles between workgroups (tests reach the multi-tile walk at a few tiles)
    if (p.cap > 0 && pl.grid > p.cap) pl.grid = p.cap;
    return true;
}

// ---------------------------------------------------------------------------------
// the packed-weight layout
// ---------------------------------------------------------------------------------
// A packed stream is a run of 1-KiB fragments of 512 16-bit elements, each laid out as the 64 lanes
// of a v_mfma_f32_16x16x32 A operand read it: element e of a fragment belongs to lane e / 8 = (g, c16)
// = (lane / 16, lane % 16) and is its j = e % 8.  Per 32-unit hidden chunk c the stream holds, for
// each of the kind's phase-A matrices (rows = hidden units, D columns), 2 KS fragments (h-tile ht,
// k-step ks) = rows 32 c + 16 ht + c16, columns 32 ks + 8 g + j; then the NT fragments of the phase-B
// matrix (DB rows, F columns), fragment nt = row ffn_sigma(nt, c16), hidden column 32 c + 4 g + j
// (j < 4) or 32 c + 16 + 4 g + j - 4: the hidden index permuted to the phase-A accumulator order.
// FFN_PACK_ATTN puts Wo (D, D) in front, k-step major: fragment (ks, nt) = row ffn_sigma(nt, c16),
// columns 32 ks + 8 g + j.
enum FfnPackKind {
    FFN_PACK_FFN = 0,    // kinet_ffn_pack: W1 (F, D), W2 (D, F); DB = D
    FFN_PACK_PAIR = 1,   // kinet_bottleneck_pack: W3 (F, D), W1 (DB, F)
    FFN_PACK_DS = 2,     // kinet_bottleneck_pack_ds: W3 (F, D), W_ds (F, D), W1 (DB, F)
    FFN_PACK_ATTN = 3,   // kinet_ffn_pack_attn: Wo (D, D), W1 (F, D), W2 (D, F); DB = D
};
constexpr int kFfnPackMats = 3;   // source matrices of a kind, at most

struct FfnPackSrc {
    int mat, row, col;   // source matrix in the kind's argument order, element (row, col)
    int ld;              // the matrix's row length
};

KINET_FFN_HD constexpr int ffn_pack_phase_a(int kind) { return kind == FFN_PACK_DS ? 2 : 1; }
KINET_FFN_HD constexpr long long ffn_pack_total(int kind, int D, int F, int DB) {
    return (long long)(ffn_pack_phase_a(kind) * D + DB) * F + (kind == FFN_PACK_ATTN ? (long long)D * D : 0);
}

// source element of packed element idx of a stream of `kind`
KINET_FFN_HD constexpr FfnPackSrc ffn_pack_src(int kind, int D, int F, int DB, long long idx) {
    const int KS = D / 32, NT = DB / 16, NA = ffn_pack_phase_a(kind);
    const int e = (int)(idx & 511);
    const int lane = e >> 3, j = e & 7, g = lane >> 4, c16 = lane & 15;
    int first = 0;   // the stream's first phase-A matrix
    if (kind == FFN_PACK_ATTN) {
        const long long head = (long long)D * D;
        if (idx < head) {
            const int f = (int)(idx >> 9), ks = f / NT, nt = f - ks * NT;
            return FfnPackSrc{0, ffn_sigma(nt, c16), 32 * ks + 8 * g + j, D};
        }
        idx -= head;
        first = 1;
    }
    const int FR = 2 * KS * NA + NT;
    const long long per_chunk = (long long)FR * 512;
    const int c = (int)(idx / per_chunk);
    const int f = (int)(idx - (long long)c * per_chunk) >> 9;
    if (f < 2 * KS * NA) {
        const int a = f / (2 * KS), ff = f - a * 2 * KS;
        const int ht = ff / KS, ks = ff - ht * KS;
        return FfnPackSrc{first + a, 32 * c + 16 * ht + c16, 32 * ks + 8 * g + j, D};
    }
    const int nt = f - 2 * KS * NA;
    const int h = 32 * c + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
    return FfnPackSrc{first + NA, ffn_sigma(nt, c16), h, F};
}

}  // namespace kinet
