// Host-side planning of the tiled GEMM / implicit-convolution launches of gemm.hip: the table of
// the kernel instantiations that exist, and the pure function that turns a described problem into
// one or two launches of table entries.  gemm.hip generates its kernel instantiations from the
// table and sizes every grid from the entry the plan names, so a grid cannot be sized for one tile
// and run the kernel of another.  No HIP in this file: it runs on a machine without a GPU
// (kinet_gemm_plan, tests/test_gemm_plan_cpu.py).
#pragma once
#include "../../include/kinet_common.h"

namespace kinet {

void set_error(const char* fmt, ...);   // status.hip

// the kernel family of the calling thread's last launch (kinet_gemm_last_kernel)
enum { FAM_NONE = 0, FAM_TILED, FAM_TILED_DMA, FAM_DMA8, FAM_RW, FAM_RW_CONV, FAM_CONV3X3, FAM_STEM, FAM_SPLITK };

// operand classes, as bits of GemmTile::ops
enum { OPS_16 = 1, OPS_F32 = 2, OPS_X3 = 4, OPS_NO_X3 = OPS_16 | OPS_F32, OPS_ALL = OPS_16 | OPS_F32 | OPS_X3 };
inline int gemm_op_class(int in_dtype) {
    return in_dtype == KINET_F32_X3 ? OPS_X3 : in_dtype == KINET_F32 ? OPS_F32 : OPS_16;
}

struct GemmTile {
    int family;
    int bm, bn;      // output tile
    int wm, wn;      // waves along M / N
    bool ln;         // fused LayerNorm epilogue (one tile spans the row)
    int stages;      // LDS-DMA ring slots (gemm_dma_kernel); 0 = register-staged (gemm_kernel)
    int ops;         // operand classes that have the instantiation
    bool no_a2;      // no load-time A2 add
    constexpr int threads() const { return 64 * wm * wn; }
};

constexpr GemmTile kGemmTiles[] = {
    // the 4-wave register-staged tiles: every operand class, A2 added at load time
    {FAM_TILED, 32, 64, 2, 2, false, 0, OPS_ALL, false},
    {FAM_TILED, 64, 64, 2, 2, false, 0, OPS_ALL, false},
    {FAM_TILED, 64, 128, 2, 2, false, 0, OPS_ALL, false},
    {FAM_TILED, 128, 64, 2, 2, false, 0, OPS_ALL, false},
    {FAM_TILED, 128, 128, 2, 2, false, 0, OPS_ALL, false},
    {FAM_TILED, 32, 256, 1, 4, true, 0, OPS_ALL, false},
    {FAM_TILED, 32, 320, 1, 4, true, 0, OPS_ALL, false},
    {FAM_TILED, 64, 256, 1, 4, true, 0, OPS_ALL, false},
    {FAM_TILED, 64, 320, 1, 4, true, 0, OPS_ALL, false},
    // their LDS-DMA staged twins (flag 16; KINET_F32_X3 operands are split into bf16 hi / lo on the
    // way into LDS and A2 is added in registers, so neither can be staged by DMA)
    {FAM_TILED_DMA, 32, 64, 2, 2, false, 3, OPS_NO_X3, true},
    {FAM_TILED_DMA, 64, 64, 2, 2, false, 3, OPS_NO_X3, true},
    {FAM_TILED_DMA, 64, 128, 2, 2, false, 3, OPS_NO_X3, true},
    {FAM_TILED_DMA, 128, 64, 2, 2, false, 3, OPS_NO_X3, true},
    {FAM_TILED_DMA, 128, 128, 2, 2, false, 3, OPS_NO_X3, true},
    {FAM_TILED_DMA, 32, 256, 1, 4, true, 3, OPS_NO_X3, true},
    {FAM_TILED_DMA, 32, 320, 1, 4, true, 3, OPS_NO_X3, true},
    {FAM_TILED_DMA, 64, 256, 1, 4, true, 3, OPS_NO_X3, true},
    {FAM_TILED_DMA, 64, 320, 1, 4, true, 3, OPS_NO_X3, true},
    // tiles that exist as LDS-DMA kernels only (16-bit operands, no A2): the 128 x 320 LayerNorm
    // tile and the 8-wave tiles (LayerNorm on 256-wide rows)
    {FAM_TILED_DMA, 128, 320, 2, 2, true, 2, OPS_16, true},
    {FAM_DMA8, 256, 256, 2, 4, true, 2, OPS_16, true},
    {FAM_DMA8, 256, 256, 2, 4, false, 2, OPS_16, true},
    {FAM_DMA8, 256, 128, 4, 2, false, 3, OPS_16, true},
    {FAM_DMA8, 128, 256, 2, 4, false, 3, OPS_16, true},
};
constexpr int kNumGemmTiles = (int)(sizeof(kGemmTiles) / sizeof(kGemmTiles[0]));

// The entry of tile bm x bn with / without the LayerNorm epilogue: the one staged as `dma` asks
// (flag 16 chooses between twins), or the tile's only entry; -1 = no such tile.
inline int gemm_tile_index(int bm, int bn, bool ln, bool dma) {
    int only = -1;
    for (int i = 0; i < kNumGemmTiles; ++i) {
        const GemmTile& t = kGemmTiles[i];
        if (t.bm != bm || t.bn != bn || t.ln != ln) continue;
        if ((t.stages != 0) == dma) return i;
        if (only < 0) only = i;
    }
    return only;
}
inline bool gemm_tile_serves(const GemmTile& t, int ops, bool a2) { return (t.ops & ops) && !(t.no_a2 && a2); }

// One tiled GEMM / implicit conv as launch() sees it, with everything the choice depends on.
struct GemmProblem {
    int M, N, K, Cin;
    bool conv, ln, a2;          // implicit conv; fused LayerNorm; load-time A2 add
    int kchunk, hm_rows;        // split-K slice length (0: whole K); head-major store
    int ops;                    // operand class (one OPS_ bit)
    int flags;                  // kinet_gemm_set_flags of the calling thread
    int force_bm, force_bn;     // kinet_gemm_force_tile of the calling thread (0: heuristic)
    bool solo;                  // kinet_set_solo_launch
    int cus;                    // compute units of the device
};
// rows [m_begin, m_begin + m_tiles * BM) of the problem on table entry `tile`
struct GemmLaunch {
    int tile, m_begin, m_tiles;
};
struct GemmPlan {
    int n;   // 0 (empty problem), 1 or 2
    GemmLaunch launch[2];
};

// The 4-wave tile of a problem, before the 8-wave and forced-tile rules.
inline void gemm_base_tile(const GemmProblem& a, int& bm, int& bn) {
    if (a.ln) {
        bm = a.M <= 8192 ? 32 : 64;     // small M (decoder queries): more workgroups
        bn = a.N <= 256 ? 256 : 320;
        // rows of 257..320 (d = 288, configs 3-5) at encoder sizes: 128 x 320 LDS-DMA tiles --
        // the 64 x 320 register-staged tile re-reads the whole 320 x K weight through its
        // staging registers for every 64 rows (~100 TF/s at M = 172k)
        if (a.ops == OPS_16 && a.N > 256 && a.M >= 8192 && !a.a2 && a.kchunk == 0) bm = 128;
    } else if (a.kchunk && a.M <= 4096) {
        bm = bn = 64;                   // split-K slices of a small-M, long-K problem
    } else if (a.M <= 4096 && a.N <= 1024) {
        bm = 32;                        // decoder-sized GEMMs: more workgroups
        bn = 64;
    } else {
        // 64x128 (128x64 for N <= 64): fastest main-loop tile on every 3x3 / K >= 512 conv and
        // GEMM shape of the detector at batch 8 (tools/sweep_conv.py) -- more tiles per CU-round
        // than 128x128 and no worse per flop
        bn = a.N <= 64 ? 64 : 128;
        bm = a.N <= 64 ? 128 : 64;
        // big square-ish problems: the 128x128 tile's lower operand traffic per flop wins
        const long t128 = (long)((a.M + 127) / 128) * ((a.N + 127) / 128);
        if (a.N >= 512 && t128 >= 2048) bm = bn = 128;
        // 3x3 convs (K >= 9*128) with >= ~2 rounds of 128x128 tiles over the 512 resident
        // slots: 3-6 % faster than 64x128 at batch 16 (tools/sweep_conv.py 16), neutral at 8
        if (a.conv && a.K >= 1152 && a.N >= 128 && t128 >= 1000) bm = bn = 128;
        // KINET_F32_X3 with N just past a multiple of 128 (d = 288 of the config-4 training
        // GEMMs): 128 x 64 tiles waste 10 % of the columns instead of 25 % -- x3 (44446, 288,
        // 1024) 157 -> 132 us, (44446, 288, 288) 60 -> 51 us (profiles/r05x_x3_tiles.log);
        // flag 33554432 keeps the default (A/B)
        if (a.ops == OPS_X3 && a.N > 64 && a.N % 128 != 0 && a.N % 128 <= 64 && !(a.flags & 33554432)) {
            bm = 128;
            bn = 64;
        }
    }
}

// The launches of one problem; KINET_ERR_ARG (with the message set) if it has none.
inline int gemm_plan(const GemmProblem& a, GemmPlan& plan) {
    plan.n = 0;
    if (a.M == 0 || a.N == 0) return KINET_OK;
    const bool ln = a.ln, b16 = a.ops == OPS_16;
    if (ln && a.N > 320) {
        set_error("gemm: fused LayerNorm needs N <= 320 (got %d)", a.N);
        return KINET_ERR_ARG;
    }
    int bm, bn;
    gemm_base_tile(a, bm, bn);
    // 8-wave LDS-DMA tiles (one workgroup per CU: `cus` slots per round): chosen for long-K
    // problems whose rounds of tiles are well filled (a square 4096^3 bf16 GEMM: 1115 TF/s
    // on 256x256 vs 456 on the 4-wave 128x128 tile, tools/gemm_probe.py); on the detector's
    // conv / GEMM shapes their last, partly filled round costs more than the faster main loop
    // gains (DESIGN.md "GEMM / conv kernel"), so those keep the 4-wave tiles.  Flag 2 forces
    // them wherever eligible.
    bool wave8 = false;
    // (not for head-major stores: only gemm_kernel's epilogue writes them)
    if (b16 && !a.a2 && a.kchunk == 0 && a.hm_rows == 0 && a.M >= 4096 && a.N >= 128 && (!ln || a.N <= 256)) {
        const int tn = (a.N > 128 || ln) ? 256 : 128;
        const long t = (long)((a.M + 255) / 256) * ((a.N + tn - 1) / tn);
        const double eff = (double)a.M * a.N / ((double)((t + a.cus - 1) / a.cus) * a.cus * 256.0 * tn);
        if ((a.flags & 2) || (!ln && a.K >= 1024 && eff >= 0.9)) {
            wave8 = true;
            bm = 256;
            bn = tn;
        }
    }
    const bool forced = a.force_bm && !ln;
    if (forced) {
        bm = a.force_bm;
        bn = a.force_bn;
    }
    // LDS-DMA staging (opt-in, flag 16): measured 0-10 % slower than the register-staged
    // kernel on the detector's conv / GEMM shapes at batch 8 (tools/sweep_conv.py), so the
    // register path stays the default; A2 (load-time add) needs the register path anyway
    // (not for KINET_F32_X3: its operands are split into bf16 hi / lo on the way into LDS)
    const bool dma = !a.a2 && (a.flags & 16) && a.ops != OPS_X3;
    // one launch of the tile grid over rows [m_begin, m_begin + m_tiles * tbm)
    auto add = [&](int tbm, int tbn, long m_begin, long m_tiles) -> int {
        const int i = gemm_tile_index(tbm, tbn, ln, dma);
        if (i < 0 || !gemm_tile_serves(kGemmTiles[i], a.ops, a.a2)) {
            // the 256-row / 256-column tiles exist as 8-wave LDS-DMA kernels only: 16-bit operands,
            // no load-time A2 add
            if (forced && i >= 0)
                set_error("gemm: forced tile %dx%d needs 16-bit operands and no A2 (no such instantiation)", tbm, tbn);
            else
                set_error("gemm: no %dx%d tile for these operands", tbm, tbn);
            return KINET_ERR_ARG;
        }
        if (m_tiles * ((a.N + tbn - 1) / tbn) >= (1L << 31)) {
            set_error("gemm: too many tiles");
            return KINET_ERR_ARG;
        }
        plan.launch[plan.n++] = GemmLaunch{i, (int)m_begin, (int)m_tiles};
        return KINET_OK;
    };
    // Multi-tap convolutions (3x3, 7x1): whole rounds of one-per-CU 8-wave 256-row tiles (the
    // faster main loop: half the LDS reads per MFMA and half the L2 bytes per flop of the
    // 4-wave tiles), then the rows left over -- less than a round -- on the 4-wave tiles in a
    // second launch, instead of a partly filled last round of 8-wave tiles (flag 64: off)
    if (b16 && a.conv && !ln && !a.a2 && a.kchunk == 0 && !a.force_bm && !wave8 && !(a.flags & 64) && a.K > a.Cin &&
        a.N >= 256 && a.M >= 8192) {
        // (256x256 tiles only: at N = 128 the 8-wave 256x128 tile measured no faster per
        // round than the 4-wave 128x128 one, tools/gemm_probe.py)
        const int tn = 256;
        const int nN8 = (a.N + tn - 1) / tn;
        const long mt_all = (a.M + 255) / 256;
        long mfull = (mt_all * nN8 / a.cus) * a.cus / nN8;   // m-tiles that fill whole rounds
        if (mfull > mt_all) mfull = mt_all;
        // less than one round but at least half of one: a single partial round of 8-wave
        // tiles still beats the 4-wave grid (layer-4 3x3 at batch 16: 119 vs 128 us)
        if (mfull == 0 && mt_all * nN8 * 2 >= a.cus) {
            // ... unless one batch is in flight (kinet_set_solo_launch), it fills less than 60 %
            // of the CUs and 128 x 256 tiles (twice as many, same 8-wave main loop, same sums)
            // fill them better: config 5's stage-3 3x3 convs (M = 32,640, N = 256: 128 vs 255
            // tiles) 74.8 -> 48.5 us alone (profiles/r06aa_config5_shapes.txt), but -1 % on 3
            // streams, whose other batches fill the idle CUs (profiles/r06ab_solo_launch_ab.txt)
            const long t128 = (long)((a.M + 127) / 128) * nN8;
            if (a.solo && mt_all * nN8 * 10 < a.cus * 6L && t128 <= a.cus) return add(128, 256, 0, (a.M + 127) / 128);
            mfull = mt_all;
        }
        // a remainder of more than a quarter round: the partly filled last round of 8-wave
        // tiles beats the 4-wave tail (layer-3 3x3 at batch 24: 394 m-tiles = 256 + 138,
        // 140 vs 151 us, profiles/r05f2_conv24.log); flag 8388608 keeps the split (A/B)
        if (mfull >= 1 && (mt_all - mfull) * nN8 * 4 > a.cus && !(a.flags & 8388608)) mfull = mt_all;
        if (mfull >= 1) {
            if (int rc = add(256, tn, 0, mfull)) return rc;
            const long rem = a.M - mfull * 256;
            if (rem <= 0) return KINET_OK;
            return add(64, 128, mfull * 256, (rem + 63) / 64);   // less than a round: the smaller tile
        }
    }
    return add(bm, bn, 0, (a.M + bm - 1) / bm);
}

// Split-K factor for long-K problems with too few output tiles to fill the CUs twice over;
// 1 = no split.  The rule sees the base tile of a plain GEMM only (gemm_base_tile of f32 operands:
// none of the convolution, KINET_F32_X3, 128 x 320 LayerNorm, 8-wave or forced-tile rules), as it
// always has: following the full plan would change which calls split.
inline int gemm_ksplit(int M, int N, int K, bool ln) {
    if (K < 1024 || M <= 0 || N <= 0) return 1;
    GemmProblem p{};
    p.M = M;
    p.N = N;
    p.K = K;
    p.ln = ln;
    p.ops = OPS_F32;
    int bm, bn;
    gemm_base_tile(p, bm, bn);
    if ((long)((M + bm - 1) / bm) * ((N + bn - 1) / bn) >= 512) return 1;
    p.kchunk = 1;   // the tile of the K slices
    gemm_base_tile(p, bm, bn);
    const long tiles = (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn);
    long ks = (768 + tiles - 1) / tiles;
    if (ks > 4) ks = 4;
    if (ks > K / 256) ks = K / 256;
    return ks >= 2 ? (int)ks : 1;
}

}  // namespace kinet
