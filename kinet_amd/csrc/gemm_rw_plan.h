// Host-side planning of the resident-weight GEMM launches of gemm_rw.hip: the LDS geometry of a
// kernel variant, the table of the gemm_rw_kernel instantiations that exist, and the pure function
// that turns a described problem into "not eligible" or one launch of a table entry.  gemm_rw.hip
// generates its kernel instantiations from the table and reads block, grid and the
// kinet_gemm_rw_last_config record from the entry the plan names.  No HIP in this file: it runs on a
// machine without a GPU (kinet_gemm_rw_plan, tests/test_gemm_rw_plan_cpu.py).
#pragma once
#include "../../include/kinet_common.h"

namespace kinet {

// (operand type, output type) pairs, as bits of RwVariant::types
enum { RWT_BF16_BF16 = 1, RWT_BF16_F16 = 2, RWT_BF16_F32 = 4, RWT_F16_F16 = 8, RWT_F16_F32 = 16 };
enum {
    RWT_GEMM = RWT_BF16_BF16 | RWT_BF16_F16 | RWT_BF16_F32 | RWT_F16_F16 | RWT_F16_F32,
    RWT_CONV = RWT_BF16_BF16 | RWT_F16_F16,      // convolutions: same type only
    RWT_RECORDS = RWT_BF16_F16 | RWT_F16_F16,    // sampling records: f16 weights
};
// the pair's bit; 0 = the kernel is built for no such pair
inline int rw_type_pair(int in_dtype, int out_dtype) {
    if (in_dtype == KINET_BF16)
        return out_dtype == KINET_BF16 ? RWT_BF16_BF16 : out_dtype == KINET_F16 ? RWT_BF16_F16 : out_dtype == KINET_F32 ? RWT_BF16_F32 : 0;
    if (in_dtype == KINET_F16) return out_dtype == KINET_F16 ? RWT_F16_F16 : out_dtype == KINET_F32 ? RWT_F16_F32 : 0;
    return 0;
}

// One instantiation of gemm_rw_kernel but for the types and the ring depth (rw_ring_depth below).
struct RwVariant {
    int kc;          // K = 32 * kc
    int nt;          // 16-column tiles per wave
    int bmr;         // rows per row tile
    int nw;          // waves per workgroup
    int occ;         // resident workgroups per CU the launch is sized for (__launch_bounds__)
    bool has_r, ln, has_a2, cr, prep;   // residual, LayerNorm, load-time A2 add, conv-row mode, sampling records
    int types;       // RWT_ bits: the type pairs that have the instantiation
    constexpr int gw() const { return nw * nt * 16; }            // columns per workgroup
    constexpr int threads() const { return nw * 64; }
    constexpr int lds_budget() const { return 160 * 1024 / occ; }   // a CU's LDS over its resident workgroups
};

// The kernel's LDS layout: NW waves per workgroup (4, or 6 / 9 for the d = 288 LayerNorm rows, 8 for
// the wide groups); rows of K = 32*KC 16-bit elements: a power-of-two number of 16-byte chunks, or a
// multiple of 4 (K = 288: 36 chunks).  A tile region whose bytes are not whole DMA rounds (NW*64
// lanes x 16 B) is padded to whole rounds; the padding chunks read zeros (out of range) and nothing
// reads them back.
struct RwLds {
    int NTHR, OPB, ROW, CPR, SWM, GW, A_BYTES, A_OPS, A_SPAN, A2_BYTES;
    int R_ROW, R_CPR, R_SWM, R_OPS, R_BYTES, R_OFF, MASK_OFF, REF_OFF, REF_OPS, STAGE, PAR, LNS, BYTES, D;
    bool POW2, R_POW2;
};
constexpr RwLds rw_lds(const RwVariant& v, int ns) {
    RwLds g{};
    g.NTHR = v.nw * 64;
    g.OPB = g.NTHR * 16;                          // bytes per DMA round
    g.ROW = v.kc * 64;                            // A row bytes (K = 32*KC, 16-bit)
    g.CPR = g.ROW / 16;                           // 16-byte chunks per A row
    g.POW2 = (g.CPR & (g.CPR - 1)) == 0;
    g.SWM = (g.CPR < 16 ? g.CPR : 16) - 1;        // source-side XOR swizzle mask
    g.GW = v.gw();                                // columns per workgroup
    g.A_BYTES = v.bmr * g.ROW;
    g.A_OPS = (g.A_BYTES + g.OPB - 1) / g.OPB;    // DMA instructions per thread per tile
    g.A_SPAN = g.A_OPS * g.OPB;
    g.A2_BYTES = v.has_a2 ? g.A_SPAN : 0;         // second A operand (A + A2)
    g.R_ROW = g.GW * 2;
    g.R_CPR = g.R_ROW / 16;
    g.R_POW2 = (g.R_CPR & (g.R_CPR - 1)) == 0;
    g.R_SWM = (g.R_CPR < 16 ? g.R_CPR : 16) - 1;
    g.R_OPS = v.has_r ? (v.bmr * g.R_ROW + g.OPB - 1) / g.OPB : 0;
    g.R_BYTES = g.R_OPS * g.OPB;
    g.R_OFF = g.A_SPAN + g.A2_BYTES;
    g.MASK_OFF = g.R_OFF + g.R_BYTES;
    g.REF_OFF = g.MASK_OFF + 1024;                // PREP: the tile's reference points
    g.REF_OPS = v.prep ? v.bmr / 16 : 0;          // 1 KiB DMAs: BMR rows x 4 levels x <= 16 B
    g.STAGE = g.REF_OFF + g.REF_OPS * 1024;       // + one DMA of row-mask bytes (+ refs)
    g.PAR = 4 * g.GW * 4;                         // scale, bias, gamma, beta (f32)
    g.LNS = v.ln ? 2 * v.bmr * v.nw * 4 : 0;      // [2][BMR][NW waves] partial sums
    g.BYTES = g.PAR + g.LNS + ns * g.STAGE;
    g.D = g.A_OPS * (v.has_a2 ? 2 : 1) + g.R_OPS + 1 + g.REF_OPS;
    return g;
}
// NS: the deepest DMA ring (<= 4 row tiles) that keeps the workgroup within its share of the CU's LDS
constexpr int rw_ring_depth(const RwVariant& v) {
    const RwLds g = rw_lds(v, 0);
    const int ns = (v.lds_budget() - g.BYTES) / g.STAGE;
    return ns >= 4 ? 4 : ns;
}

// the frame-shared A2 addressing (a2_sub / a2_sub1 / a2_bnd) lets a row tile wrap at most once:
// a2_rows >= BMR.  The entry points require a2_rows >= kRwMinA2Rows, the table BMR <= kRwMinA2Rows
constexpr int kRwMinA2Rows = 32;
static_assert(kRwMinA2Rows == 32, "the entry points' a2_rows messages say 32");

constexpr RwVariant kRwVariants[] = {
    // K = 64 / 128 / 256, 4-wave 256-column groups, two per CU.  16-row tiles when a tile carries a
    // second operand (residual / A2) or the LayerNorm epilogue (which needs them at K = 256 to stay
    // in 256 VGPRs): a 2-4 deep ring then fits; K = 64 rows (128 B) need 32-row tiles for whole
    // 4 KiB DMA rounds.  The plain 16-row entries at K >= 128 serve flag 131072 (tests)
    {2, 4, 32, 4, 2, false, false, false, false, false, RWT_GEMM},
    {2, 4, 32, 4, 2, true, false, false, false, false, RWT_GEMM},
    {2, 4, 32, 4, 2, true, true, false, false, false, RWT_GEMM},
    {2, 4, 32, 4, 2, false, true, false, false, false, RWT_GEMM},
    {2, 4, 32, 4, 2, false, false, true, false, false, RWT_GEMM},
    {4, 4, 32, 4, 2, false, false, false, false, false, RWT_GEMM},
    {4, 4, 16, 4, 2, false, false, false, false, false, RWT_GEMM},
    {4, 4, 16, 4, 2, true, false, false, false, false, RWT_GEMM},
    {4, 4, 16, 4, 2, true, true, false, false, false, RWT_GEMM},
    {4, 4, 16, 4, 2, false, true, false, false, false, RWT_GEMM},
    {4, 4, 16, 4, 2, false, false, true, false, false, RWT_GEMM},
    {8, 4, 32, 4, 2, false, false, false, false, false, RWT_GEMM},
    {8, 4, 16, 4, 2, false, false, false, false, false, RWT_GEMM},
    {8, 4, 16, 4, 2, true, false, false, false, false, RWT_GEMM},
    {8, 4, 16, 4, 2, true, true, false, false, false, RWT_GEMM},
    {8, 4, 16, 4, 2, false, true, false, false, false, RWT_GEMM},
    {8, 4, 16, 4, 2, false, false, true, false, false, RWT_GEMM},
    // + residual with N > 256: 8-wave 512-column groups, one workgroup per CU
    {2, 4, 16, 8, 1, true, false, false, false, false, RWT_GEMM},
    {4, 4, 16, 8, 1, true, false, false, false, false, RWT_GEMM},
    {8, 4, 16, 8, 1, true, false, false, false, false, RWT_GEMM},
    // K = 512 (1 KiB rows): the weight slice stays at 128 VGPRs per wave by narrowing the wave to 32
    // columns (NT = 2): 4-wave 128-column groups, or one 8-wave 256-column group
    {16, 2, 16, 4, 2, false, false, false, false, false, RWT_GEMM},
    {16, 2, 16, 8, 1, false, false, false, false, false, RWT_GEMM},
    // K = 288 (d = 288: configs 3-5): 16-row tiles, 12 columns per lane (NT = 3, 108 weight VGPRs;
    // 180-210 in all: two waves per SIMD).  LayerNorm rows (N <= 288) need the whole row in one
    // workgroup: 9 waves x 32 columns (NT = 2, 126-152 VGPRs; the 6-wave x 48-column group under
    // flag 4194304), one workgroup per CU with a ring of up to 4 tiles in 160 KiB; the other
    // epilogues take 4-wave 192-column groups, two per CU (a row tile is shared by its groups
    // through the XCD's L2, as at K = 256), or 8-wave 384-column groups, one per CU
    {9, 3, 16, 4, 2, false, false, false, false, false, RWT_GEMM},
    {9, 3, 16, 8, 1, false, false, false, false, false, RWT_GEMM},
    {9, 3, 16, 4, 2, true, false, false, false, false, RWT_GEMM},
    {9, 3, 16, 4, 2, false, false, true, false, false, RWT_GEMM},
    {9, 3, 16, 8, 1, false, false, true, false, false, RWT_GEMM},
    {9, 2, 16, 9, 1, true, true, false, false, false, RWT_GEMM},
    {9, 2, 16, 9, 1, false, true, false, false, false, RWT_GEMM},
    {9, 3, 16, 6, 1, true, true, false, false, false, RWT_GEMM},
    {9, 3, 16, 6, 1, false, true, false, false, false, RWT_GEMM},
    // conv-row mode (K <= 256): the strided 1x1 convolution on 256-column groups, the KH x 1
    // tap-folded form on 128-column groups; 16-row tiles under flag 131072 (tests)
    {8, 4, 32, 4, 2, false, false, false, true, false, RWT_CONV},
    {8, 4, 16, 4, 2, false, false, false, true, false, RWT_CONV},
    {8, 2, 32, 4, 2, false, false, false, true, false, RWT_CONV},
    {8, 2, 16, 4, 2, false, false, false, true, false, RWT_CONV},
    // sampling records (K = 256, one head = 48 columns per wave): one 8-wave 384-column group with
    // the load-time add; 4-wave 192-column groups with it (three per CU) and without it (two)
    {8, 3, 16, 8, 1, false, false, true, false, true, RWT_RECORDS},
    {8, 3, 16, 4, 3, false, false, true, false, true, RWT_RECORDS},
    {8, 3, 16, 4, 2, false, false, false, false, true, RWT_RECORDS},
};
constexpr int kNumRwVariants = (int)(sizeof(kRwVariants) / sizeof(kRwVariants[0]));

// the entry with these fields; -1 = no such instantiation
constexpr int rw_variant_index(int kc, int nt, int bmr, int nw, int occ, bool has_r, bool ln, bool has_a2, bool cr, bool prep) {
    for (int i = 0; i < kNumRwVariants; ++i) {
        const RwVariant& v = kRwVariants[i];
        if (v.kc == kc && v.nt == nt && v.bmr == bmr && v.nw == nw && v.occ == occ && v.has_r == has_r && v.ln == ln &&
            v.has_a2 == has_a2 && v.cr == cr && v.prep == prep)
            return i;
    }
    return -1;
}

// what must hold for every entry of the table
template <typename F> constexpr bool rw_every_variant(F ok) {
    for (int i = 0; i < kNumRwVariants; ++i)
        if (!ok(kRwVariants[i])) return false;
    return true;
}
static_assert(rw_every_variant([](const RwVariant& v) { return rw_ring_depth(v) >= 2; }), "LDS budget: a ring of 2+ tiles");
static_assert(rw_every_variant([](const RwVariant& v) { return rw_lds(v, rw_ring_depth(v)).BYTES <= 160 * 1024 / v.occ; }),
              "LDS budget: OCC workgroups per CU");
static_assert(rw_every_variant([](const RwVariant& v) { return !v.has_a2 || v.bmr <= kRwMinA2Rows; }),
              "frame-shared A2: a row tile wraps at most once (a2_rows >= BMR)");
static_assert(rw_every_variant([](const RwVariant& v) {
                  return !v.prep || (v.nt == 3 && (v.nw == 4 || v.nw == 8) && (v.bmr == 16 || v.bmr == 32) && !v.has_r && !v.ln);
              }), "sampling records: one head per wave (12 columns per lane), 16- or 32-row tiles");
static_assert(rw_every_variant([](const RwVariant& v) { return rw_lds(v, 0).POW2 || rw_lds(v, 0).CPR % 4 == 0; }),
              "A rows: power-of-two or multiple-of-4 chunks");
static_assert(rw_every_variant([](const RwVariant& v) { return !v.has_r || rw_lds(v, 0).R_POW2 || rw_lds(v, 0).R_CPR % 4 == 0; }),
              "residual rows: power-of-two or multiple-of-4 chunks");
static_assert(rw_every_variant([](const RwVariant& v) { return v.bmr / 16 <= 64; }), "mask DMA lanes");
constexpr bool rw_variants_distinct() {
    for (int i = 0; i < kNumRwVariants; ++i) {
        const RwVariant& v = kRwVariants[i];
        if (rw_variant_index(v.kc, v.nt, v.bmr, v.nw, v.occ, v.has_r, v.ln, v.has_a2, v.cr, v.prep) != i) return false;
    }
    return true;
}
static_assert(rw_variants_distinct(), "no entry twice");

// One resident-weight launch as its entry point sees it, with everything the choice depends on.
enum { RW_GEMM = 0, RW_CONV = 1, RW_RECORDS = 2 };
struct RwProblem {
    int kind;                       // RW_GEMM (launch_rw), RW_CONV (launch_rw_conv), RW_RECORDS (kinet_msda_sample_records)
    int M, N, K;
    int in_dtype, out_dtype;
    bool r, ln, a2;                 // residual, fused LayerNorm, load-time A2 add
    int ldc, ldr;
    bool c_al16, r_al16, a2_al16;   // 16-byte alignment of C, R, A2
    int hm_rows, hm_d, hm_split, hm_d2;   // head-major store (GemmArgs)
    int Cin, KW, stride, stride_w, pad, pad_w, Win, Wout;   // convolution geometry (RW_CONV)
    bool row_mask;
    int flags;                      // kinet_gemm_set_flags of the calling thread
    int cap;                        // kinet_gemm_rw_grid_cap of the calling thread (0 = none)
    int cus;                        // compute units of the device
};
struct RwPlan {
    int variant;                    // index into kRwVariants
    int n_mtiles, ng, P;            // row tiles; grid.y (column groups); grid.x (workgroups per column group)
    int c_bytes, hm_tr;             // GemmArgs::c_bytes / hm_tr of the launch
};

// The launch of one problem; false = the resident-weight kernel does not take it.
inline bool rw_plan(const RwProblem& a, RwPlan& plan) {
    if (a.in_dtype != KINET_BF16 && a.in_dtype != KINET_F16) return false;
    if (a.N <= 0) return false;   // (no column group to spread the workgroups over)
    const int min_m = (a.flags & 8) ? 256 : 4096;   // smallest M routed here (kinet_gemm_set_flags bit 3: 256)
    int kc, nt = 4, bmr = 16, nw = 4, occ = 2;
    bool cr = false, prep = false;
    long long cb;
    plan.hm_tr = 0;
    if (a.kind == RW_RECORDS) {
        // The MSDA sampling-offsets | attention-weights projection (K = 256, N = heads * 48, checked
        // by the entry point).
        // With the position embedding added on load (A2, the encoder): ONE 8-wave 384-column group per
        // 16-row tile, one workgroup per CU (166 VGPRs, a 4-slot ring): each row tile's x + pos rows
        // are read once.  The two 4-wave 192-column groups before it (three workgroups per CU, a
        // 2-slot ring) were meant to share each row tile through the XCD's L2 (same XCD by linear id),
        // but PMC showed 1.11 GB fetched per batch-28 call against ~0.35 GB of operands: 270 -> 238 us
        // per call, encoder call 0.72-0.74 -> 0.69-0.70 ms, bench 1416 / 1429 -> 1441 / 1446 frames/s
        // interleaved, records bit-identical (profiles/r06am_records_8wave_ab.txt; two 8-wave groups per
        // CU: 245 us, 1435 / 1445).  Flag 268435456 keeps the 4-wave groups (A/B, tests).  Round 4's
        // notes on the 4-wave grid: three per CU beat two with a 4-slot ring under three streams
        // (profiles/r04z_occ_ab.log), four per CU spilled.  The 32-row tile (two MFMA row tiles per
        // wave) is not used here: its epilogue, interleaved by the compiler with the second tile's
        // MFMA chain, differed from the 16-row tile in a few hundred record words from run to run
        // (round 4-5)
        kc = 8;
        nt = 3;
        prep = true;
        if (a.a2 && !(a.flags & 268435456)) {
            nw = 8;
            occ = 1;
        } else if (a.a2) {
            occ = 3;
        }
        cb = (long long)a.M * a.N * 2;
    } else if (a.kind == RW_CONV) {
        // The KH x 1, horizontally stride-1 unpadded conv of the tap-folded stem (K = KH*Cin <= 256)
        // as a resident-weight stream with the conv-row gather (a short-K conv in the tiled kernel
        // exposes a full load latency per 3-step tile), and before it:
        // strided 1x1 (the ResNet downsample of stage 2, 256 -> 512 at stride 2): row m = output
        // pixel, its A row = input pixel (img, 2 oh, 2 ow) -- the conv-row DMA with a horizontal
        // stride; weights resident (K = 256), 256-column groups sharing each row tile through L2.
        // The implicit-GEMM kernel ran it at ~310 TF/s (1.8 TB/s of compulsory bytes)
        if (a.K == 256 && a.Cin == 256 && a.KW == 1 && a.pad == 0 && a.pad_w == 0 && a.stride > 1 &&
            a.stride_w == a.stride && a.M >= min_m && a.Wout >= 32 && a.N % 256 == 0 && !a.r && !a.ln && !a.row_mask &&
            a.ldc % 8 == 0 && a.c_al16 && !(a.flags & 2048)) {
            nt = 4;
        } else {
            if (a.M < min_m || a.K > 256 || a.KW != 1 || a.stride_w != 1 || a.pad_w != 0 || a.Win != a.Wout) return false;
            if (a.Cin % 8 != 0 || a.Wout < 32 || a.N > 128 || a.N % 8 != 0 || a.r || a.ln) return false;
            if (a.ldc % 8 != 0 || !a.c_al16 || a.row_mask) return false;
            nt = 2;
        }
        kc = 8;
        cr = true;
        bmr = (a.flags & 131072) ? 16 : 32;   // tests: 16-row tiles (bit-identical to the 32-row ones)
        cb = ((long long)(a.M - 1) * a.ldc + a.N) * 2;
        if (cb >= (1LL << 31)) return false;
    } else {
        if (a.M < min_m || (a.K != 64 && a.K != 128 && a.K != 256 && a.K != 512 && a.K != 288)) return false;
        if (a.K == 288 && (a.flags & 1048576)) return false;   // flag: K = 288 on the tiled kernels (A/B)
        // K = 512 (the ResNet 1x1 convs into the layer-2 bottlenecks, input_proj of level 0): only
        // N <= 256 without residual / LayerNorm / A2 (at most 2 column groups of 128, which share each
        // row tile through the XCD's L2)
        if (a.K == 512 && (a.N > 256 || a.r || a.ln || a.a2 || (a.flags & 256))) return false;
        if (a.a2 && (a.r || a.ln || !a.a2_al16)) return false;
        if (a.N % 8 != 0 || (a.ln && a.N > (a.K == 288 ? 288 : 256))) return false;
        const bool o16 = a.out_dtype == a.in_dtype || (a.in_dtype == KINET_BF16 && a.out_dtype == KINET_F16);
        const bool o32 = a.out_dtype == KINET_F32;
        if (!o16 && !o32) return false;
        if (o16 ? (a.ldc % 8 != 0) : (a.ldc % 4 != 0)) return false;
        if (!a.c_al16 || (a.r && (!o16 || a.ldr % 8 != 0 || !a.r_al16))) return false;
        // head-major stores: 16-byte units need hm_d % 8 == 0; the K = 288 path stores 4-column
        // units (hm_d % 4 == 0) and takes the split planes (hm_d2 == 4)
        if (a.hm_rows && (a.K == 288 ? (a.hm_d % 4 != 0 || (a.hm_split && (a.hm_d2 != 4 || a.hm_split % a.hm_d != 0)))
                                     : (a.hm_d % 8 != 0 || a.hm_split)))
            return false;
        // output descriptor extent (buffer stores; offsets must stay below 2^31)
        const long long osz = a.out_dtype == KINET_F32 ? 4 : 2;
        cb = a.hm_rows ? (long long)a.M * a.N * osz : ((long long)(a.M - 1) * a.ldc + a.N) * osz;
        if (cb >= (1LL << 31)) return false;
        plan.hm_tr = (a.flags & 1073741824) ? 0 : 1;   // flag: 32-column head-major stores without the LDS transpose (A/B)
        const bool w4 = (a.flags & 268435456) != 0;    // flag: the 4-wave column groups everywhere
        kc = a.K / 32;
        if (a.K == 288) {
            nt = 3;
            if (a.a2) {
                // x + pos rows (the d = 288 offsets / logits and value projections): one 8-wave group of
                // up to 384 columns per row tile, so each tile's x + pos rows are read once -- as the
                // records GEMM (kinet_msda_sample_records); flag 268435456: the 4-wave 192-column groups
                if (a.N > 192 && a.N <= 384 && !w4) nw = 8;
            } else if (a.ln) {
                // LayerNorm rows: 9 waves x 32 columns (one 288-column group; flag 4194304: the 6-wave x
                // 48-column groups, A/B and tests); without LayerNorm 4-wave 192-column groups (one 9-wave
                // group measured within noise, round 5: profiles/r05s_split_nine_waves.log)
                nw = (a.flags & 4194304) ? 6 : 9;
                if (nw == 9) nt = 2;
            } else if (!a.r && a.N > 384 && !w4) {
                // N > 384 (the d = 288 decoder's six value projections in one launch, N = 1728): 8-wave
                // 384-column groups, one workgroup per CU -- half as many groups fetch each row tile:
                // 1048 -> 948 us in config 3 (profiles/r06ar_wide_8wave_ab.txt); at 192 < N <= 384 (the
                // value projection's split planes) 89 vs 91 us, bench within noise: not taken (r06at)
                nw = 8;
            }
        } else if (a.K == 512) {
            nt = 2;
            // N == 256 (config 2's level-0 input projection, 512 -> 256): one 8-wave 256-column group
            // per row tile, one workgroup per CU, so each tile's 1 KiB rows are read once (the two
            // 4-wave 128-column groups fetched 2x the operand, profiles/pmc_traffic.json)
            if (a.N > 128 && a.N <= 256 && !w4) nw = 8;
        } else if (a.r && !a.ln && a.N > 256 && !w4) {
            // + residual with N > 256 (the stage-end conv3s, 128 -> 512 and 256 -> 1024): 8-wave
            // 512-column groups, one workgroup per CU, so each row tile's x rows are fetched by half as
            // many groups (one instead of two at N = 512); flag 268435456: the 4-wave 256-column groups
            // (plain epilogues keep the 4-wave groups: 8-wave 512-column groups ran config 2's six decoder
            // value projections (N = 1536) slower, 669 vs 648 us, profiles/r06ar_wide_8wave_ab.txt)
            nw = 8;
        } else if (kc == 2 || (!a.r && !a.ln && !a.a2)) {
            // 32-row tiles: K = 64 whatever the epilogue, and tiles without a second operand or
            // LayerNorm.  Flag 131072 (tests): the same problem on 16-row tiles -- the 32-row tiles' two
            // MFMA row tiles per wave (TMR = 2) must give the 16-row tiles' results bit for bit
            bmr = (kc >= 4 && (a.flags & 131072)) ? 16 : 32;
        }
        if (nw != 4) occ = 1;   // the 6-, 8- and 9-wave groups: one workgroup per CU
    }
    plan.variant = rw_variant_index(kc, nt, bmr, nw, occ, a.r, a.ln, a.a2, cr, prep);
    // (every rule above names an entry of the table; a type pair the entry is not built for -- a
    // convolution or the records into another type -- is not served)
    if (plan.variant < 0 || !(kRwVariants[plan.variant].types & rw_type_pair(a.in_dtype, a.out_dtype))) return false;
    const RwVariant& v = kRwVariants[plan.variant];
    plan.n_mtiles = (a.M + v.bmr - 1) / v.bmr;
    plan.ng = (a.N + v.gw() - 1) / v.gw();
    // OCC resident workgroups per CU over all groups: never more than the cus * OCC slots (a second
    // round of workgroups would double the launch), and a multiple of 8 so the column groups
    // of one row tile land on one XCD (linear id bx + y*P) and share its L2 copy of the tile
    const int slots = a.cus * v.occ;
    int P = slots / plan.ng >= 8 ? slots / plan.ng / 8 * 8 : slots / plan.ng;
    if (P > plan.n_mtiles) P = plan.n_mtiles;
    // diagnostics (host side, per calling thread): kinet_gemm_rw_grid_cap bounds P -- the kernel is
    // persistent, so P only decides which workgroup walks which row tiles; kinet_gemm_rw_last_config
    // reads the record back
    if (a.cap > 0) P = P > a.cap ? a.cap : (P < 1 ? 1 : P);
    plan.P = P;
    plan.c_bytes = (int)cb;
    return true;
}

// the kinet_gemm_rw_last_config record of a planned launch
constexpr int RW_CFG_FIELDS = 15;
inline void rw_config_record(const RwPlan& p, int out_dtype, int* out) {
    const RwVariant& v = kRwVariants[p.variant];
    const int cfg[RW_CFG_FIELDS] = {v.kc, v.nt, v.bmr, rw_ring_depth(v), v.nw, v.occ, v.has_r, v.ln, v.has_a2, v.cr, v.prep,
                                    out_dtype == KINET_F32 ? 4 : 2, p.P, p.ng, p.n_mtiles};
    for (int i = 0; i < RW_CFG_FIELDS; ++i) out[i] = cfg[i];
}

}  // namespace kinet
