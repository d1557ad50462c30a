// Host-side planning of the MSDA launches of msda.hip and msda_enc.hip: which kernel family and
// which of its instantiations a described problem runs, with what grid, block, dynamic LDS and
// run-time scalars -- or why it is refused -- and the encoder sampler's strip plan.  The launchers
// fill an MsdaProblem, call msda_plan() and expand the MsdaPlan; kinet_msda_launch_plan and
// kinet_msda_encoder_plan_ex answer from the same functions.  No HIP, no thread-locals and no
// device query in this file: it runs on a machine without a GPU (tests/test_msda_plan_cpu.py).
#pragma once
#include "../../include/kinet_common.h"

namespace kinet {

constexpr int kMsdaThreads = 256;           // workgroup of every family but the list kernel and the fast kernel at L = 4
constexpr int kMsdaMaxLevels = 16;
constexpr long long kMsdaLdsLimit = 160 * 1024;

// sizeof the device structs the LDS formulas below count (msda.hip static_asserts each)
constexpr int kLevelInfoBytes = 4 * kMsdaMaxLevels * 4;
constexpr int kTap4Bytes = 32, kTap4dBytes = 48;
constexpr int kBwdTapF32Bytes = 40, kBwdTapF64Bytes = 64;
constexpr int kHTapBytes = 32;

// kinet_msda_fused_last_kernel packs family << 8 | detail
constexpr int kFusedGeneric = 1, kFusedFast = 2, kFusedEncoder = 3;

enum MsdaKind { MSDA_FORWARD = 0, MSDA_FUSED = 1, MSDA_BACKWARD = 2 };
enum MsdaFamily {
    MSDA_K_NONE = 0,         // an empty call: nothing is launched
    MSDA_K_FWD = 1,          // msda_fwd_kernel<T, TL, VEC, FUSED>
    MSDA_K_FUSED = 2,        // msda_fused_kernel<T, VEC>
    MSDA_K_FUSED_FAST = 3,   // msda_fused_fast_kernel<T, TO, TL, L, 4, MH, SG>
    MSDA_K_BWD_LIST = 4,     // msda_bwd_list_kernel<T, TL, VEC, NJ, SP>
    MSDA_K_BWD = 5,          // msda_bwd_kernel<T, TL, GA, VEC, POW2, ALN>
};

// backward kernel choice (kinet_msda_backward_tune; 0 = automatic for every field): mode -1 = the
// direct-atomic kernel, 1 = the list kernel for any call, 2 = the list kernel with queries in index
// order, 3 = the list kernel with four samples' loads in flight; log2ns = hash rows, qc = queries
// per workgroup, threads = workgroup size, flush_at = queries per pass
struct BwdTune {
    int mode, log2ns, qc, threads, flush_at;
};

struct MsdaProblem {
    int kind;                                  // MsdaKind
    int N, S, M, D, L, Lq, P;
    int value_dtype, out_dtype, loc_dtype;     // kinet_dtype; loc: sampling locations / offsets+logits
    long long vsb, vss, vsm;                   // value strides in elements (forward: vss = the row stride)
    int value_align;                           // value pointer % 16 (fused)
    BwdTune tune;                              // backward
    int dbg;                                   // backward: kinet_msda_backward_debug word, passed through
    int cus;                                   // compute units of the device
};

constexpr int kMsdaKeepLast = -2;   // MsdaPlan::last: leave the thread's last-kernel record as it is

struct MsdaPlan {
    int family;                                // MsdaFamily
    int vec, fused, l, nj, sp, pow2, aln, sg;  // template selectors of the family (0 where it has none)
    int grid[3], block, lds;                   // lds: dynamic LDS bytes
    // run-time scalars of the launch: qt queries x lpq lanes (forward, direct backward; na of the
    // lpq lanes hold channels); QT queries per wave x MH heads per workgroup (fused); passes of QP
    // queries, qc queries per workgroup, 2^log2ns hash rows, blocked walk (list)
    int qt, lpq, na, QT, MH, QP, qc, log2ns, blocked, head_bytes, dbg;
    int last;                                  // the kinet_msda_*_last_kernel code the call records
    // refusal (msda_plan() == false): printf format of the message and its %lld arguments
    const char* why;
    long long why_arg[7];
    bool why_early;   // backward: refused before the workspace check and the grad_value memset
};

// ceil(a / b) in 64 bits (Lq + b - 1 may pass 2^31)
inline int msda_ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

inline int msda_esize(int dt) {
    return dt == KINET_F64 ? 8 : (dt == KINET_BF16 || dt == KINET_F16) ? 2 : 4;
}

// ---------------------------------------------------------------------------------
// lanes: vec contiguous channels per lane, lpq lanes per (query, head), qt queries per workgroup
// ---------------------------------------------------------------------------------
struct Cfg {
    int vec, lpq, qt;
};

inline Cfg pick_cfg(int D, int M, int esize) {
    Cfg c{1, D, 1};
    const int maxvec = 16 / esize;
    for (int v = maxvec; v >= 1; v >>= 1) {
        if (D % v == 0) { c.vec = v; break; }
    }
    c.lpq = D / c.vec;
    const int groups = kMsdaThreads / c.lpq;
    c.qt = groups / M;
    return c;
}

inline bool msda_refuse(MsdaPlan& pl, const char* why, long long a = 0, long long b = 0, bool early = false) {
    pl.why = why;
    pl.why_arg[0] = a;
    pl.why_arg[1] = b;
    pl.why_early = early;
    return false;
}

// the size rules every MSDA entry point checks first
inline bool msda_check_sizes(const MsdaProblem& p, MsdaPlan& pl) {
    if (!(p.N >= 0 && p.S >= 0 && p.M > 0 && p.D > 0 && p.L > 0 && p.Lq >= 0 && p.P > 0)) {
        const long long sizes[7] = {p.N, p.S, p.M, p.D, p.L, p.Lq, p.P};
        for (int i = 0; i < 7; ++i) pl.why_arg[i] = sizes[i];
        pl.why = "msda: invalid sizes N=%lld S=%lld M=%lld D=%lld L=%lld Lq=%lld P=%lld";
        return false;
    }
    if (p.L > kMsdaMaxLevels) return msda_refuse(pl, "msda: num_levels %lld > %lld", p.L, kMsdaMaxLevels);
    if (!((long long)p.S * p.M * p.D < (1LL << 31))) return msda_refuse(pl, "msda: S*M*D too large for one image");
    return true;
}

inline bool msda_plan_forward(const MsdaProblem& p, MsdaPlan& pl) {
    const int es = msda_esize(p.value_dtype);
    const Cfg c = pick_cfg(p.D, p.M, es);
    if (!(c.qt >= 1)) return msda_refuse(pl, "msda: heads*channels/vec (%lld*%lld) exceeds one workgroup", p.M, c.lpq);
    const long long vld = p.vss == 0 ? (long long)p.M * p.D : p.vss;
    if (!(vld >= (long long)p.M * p.D && vld % c.vec == 0)) return msda_refuse(pl, "msda: value row stride %lld invalid", vld);
    if (!((long long)p.S * vld < (1LL << 31))) return msda_refuse(pl, "msda: S*value_ld too large for one image");
    if (p.N == 0 || p.Lq == 0) return true;
    const long long tap = es == 8 ? kTap4dBytes : kTap4Bytes;
    const long long nsamp = (long long)c.qt * p.M * p.L * p.P;
    const long long lds = kLevelInfoBytes + nsamp * tap;
    if (!(lds <= kMsdaLdsLimit)) return msda_refuse(pl, "msda: LDS request %lld too large", lds);
    pl.family = MSDA_K_FWD;
    pl.vec = c.vec;
    pl.qt = c.qt;
    pl.lpq = c.lpq;
    pl.grid[0] = msda_ceil_div(p.Lq, c.qt);
    pl.grid[1] = p.N;
    pl.block = kMsdaThreads;
    pl.lds = (int)lds;
    return true;
}

inline bool msda_plan_fused(const MsdaProblem& p, MsdaPlan& pl) {
    const int es = msda_esize(p.value_dtype);
    const Cfg c = pick_cfg(p.D, p.M, es);
    pl.last = -1;
    if (!(c.lpq <= 64)) return msda_refuse(pl, "msda fused: head_dim/vec (%lld) exceeds a wave", c.lpq);
    if (p.N == 0 || p.Lq == 0) return true;
    if (es == 2) {
        // specialised kernel: head_dim 32, (L, P) in {(4, 4), (8, 4)}, 16-byte aligned vectors
        const long long head_bytes = ((long long)(p.S - 1) * p.vss + p.D) * es;
        if (p.D == 32 && p.P == 4 && (p.L == 4 || p.L == 8) && p.vss % 8 == 0 && p.vsb % 8 == 0 && p.vsm % 8 == 0 &&
            p.value_align == 0 && head_bytes < (1LL << 31)) {
            pl.family = MSDA_K_FUSED_FAST;
            pl.l = p.L;
            pl.QT = 16;
            // L = 4: 2 heads (waves) per workgroup, 2 samples per gather group: 12.5 KiB LDS and
            // 52 VGPRs, 12 workgroups per CU (encoder call 271 -> 258 us vs 4 heads x 4)
            pl.MH = p.L == 4 ? 2 : kMsdaThreads / 64;
            pl.sg = p.L == 4 ? 2 : 4;
            pl.grid[0] = msda_ceil_div(p.Lq, 16);
            pl.grid[1] = p.N;
            pl.grid[2] = msda_ceil_div(p.M, pl.MH);
            pl.block = pl.MH * 64;
            pl.head_bytes = (int)head_bytes;
            pl.last = kFusedFast << 8 | p.L;
            return true;
        }
    }
    if (!(p.out_dtype == p.value_dtype && p.loc_dtype == KINET_F32))
        return msda_refuse(pl, "msda fused: output dtype != value dtype or f16 offsets/logits need head_dim 32, "
                               "L*P in {16, 32}, P = 4 and aligned strides");
    if (!(p.vsb % c.vec == 0 && p.vss % c.vec == 0 && p.vsm % c.vec == 0 && p.value_align == 0))
        return msda_refuse(pl, "msda fused: value strides must keep %lld-element vectors aligned", c.vec);
    const int QT = 64 / c.lpq;             // queries per wave (= per workgroup)
    const int MH = kMsdaThreads / 64;      // one head per wave
    const int LP = p.L * p.P;
    const long long nsamp = (long long)MH * QT * LP;
    const bool pow2 = (LP & (LP - 1)) == 0 && LP <= 64;
    const long long lds = kLevelInfoBytes + nsamp * kTap4Bytes + (pow2 ? 0 : nsamp * 4);
    if (!(lds <= kMsdaLdsLimit)) return msda_refuse(pl, "msda fused: LDS request %lld too large", lds);
    pl.family = MSDA_K_FUSED;
    pl.vec = c.vec;
    pl.lpq = c.lpq;
    pl.QT = QT;
    pl.MH = MH;
    pl.grid[0] = msda_ceil_div(p.Lq, QT);
    pl.grid[1] = p.N;
    pl.grid[2] = msda_ceil_div(p.M, MH);
    pl.block = kMsdaThreads;
    pl.lds = (int)lds;
    pl.last = kFusedGeneric << 8 | c.vec;
    return true;
}

inline bool msda_plan_backward(const MsdaProblem& p, MsdaPlan& pl) {
    const int es = msda_esize(p.value_dtype);
    const bool f64 = es == 8;   // f64 accumulates grad_value in f64: no list kernel, no ALN scatter
    const Cfg c = pick_cfg(p.D, p.M, es);
    if (!(c.qt >= 1))
        return msda_refuse(pl, "msda: heads*channels/vec (%lld*%lld) exceeds one workgroup", p.M, c.lpq, true);
    const int LP = p.L * p.P;
    const int nj = (p.D + 15) / 16;
    const BwdTune& tn = p.tune;
    pl.dbg = p.dbg;
    if (p.N == 0 || p.Lq == 0) {
        pl.last = -1;
        return true;
    }
    // encoder calls (queries = the value pixels, Lq == S): rows summed on chip per pass
    // (msda_bwd_list_kernel); mode 1 forces it, mode -1 forbids it
    if (!f64 && tn.mode >= 0 && (p.Lq == p.S || tn.mode == 1) && c.lpq <= 16 && nj <= 4) {
        // 256 threads, passes of 16 queries (8 x 2 pixel blocks), 1024-row hash: 35 KB of LDS,
        // 4 workgroups per CU -- 1.03 ms at the config-4 encoder call; 512 threads x 32 queries
        // 1.05, 512 x 16 1.40 (tools/msda_bwd_probe.py --sweep, profiles/r03p_msda_bwd_probe.log)
        const int threads = tn.threads ? tn.threads : 256;
        const int log2ns = tn.log2ns ? tn.log2ns : 10;
        if (!(threads >= 64 && threads <= 512 && threads % 64 == 0))
            return msda_refuse(pl, "msda backward tune: threads %lld is no multiple of 64 in [64, 512]", threads);
        // the kernel hashes with >> (32 - log2ns) and sizes its table 1 << log2ns
        if (!(log2ns >= 1 && log2ns <= 30))
            return msda_refuse(pl, "msda backward tune: log2_rows %lld outside [1, 30]", log2ns);
        // phase 3 of the kernel gives every channel of a row its own thread (D <= 64 follows from
        // nj <= 4 today; the rule keeps a wider nj from dropping grad_value rows)
        if (p.D <= threads) {
            const int QP = tn.flush_at > 0 ? tn.flush_at : threads / 16;   // queries per pass
            const long long nsmp = (long long)QP * LP;
            const long long lds = kLevelInfoBytes + (3LL << log2ns) * 4 + 4 * 4 + nsmp * 4 * (8 + 4) +
                                  (long long)QP * p.D * 4 + nsmp * kHTapBytes;
            if (!(QP >= 1 && lds <= kMsdaLdsLimit))
                return msda_refuse(pl, "msda backward: pass of %lld queries x %lld samples does not fit LDS", QP, LP);
            // query chunk per workgroup: as long as the grid still fills the chip 4 times over
            int qc = tn.qc;
            if (qc <= 0) {
                qc = QP;   // one pass per workgroup: 1.08 ms at the config-4 encoder call (2 passes 1.11, 4 1.18)
                while (qc > QP && (long long)p.N * p.M * msda_ceil_div(p.Lq, qc) < 4LL * p.cus) qc >>= 1;
            }
            qc = qc / QP * QP > QP ? qc / QP * QP : QP;
            // encoder calls: queries in 8 x QP/8 pixel blocks (fewer distinct rows per pass than a
            // run of QP pixels); the grid over-covers the block count (edge blocks) and each
            // workgroup loops over chunks, so any level geometry is covered
            const int blocked = (p.Lq == p.S && QP % 8 == 0 && tn.mode != 2) ? 1 : 0;
            const int nq = blocked ? msda_ceil_div(p.S, QP) : msda_ceil_div(p.Lq, qc);
            pl.family = MSDA_K_BWD_LIST;
            pl.vec = c.vec;
            pl.nj = nj;
            pl.sp = tn.mode == 3 ? 4 : 2;
            pl.grid[0] = blocked ? nq + nq / 8 + 2 * p.L : nq;
            pl.grid[1] = p.N;
            pl.grid[2] = p.M;
            pl.block = threads;
            pl.lds = (int)lds;
            pl.na = c.lpq;
            pl.QP = QP;
            pl.qc = qc;
            pl.log2ns = log2ns;
            pl.blocked = blocked;
            pl.last = 1;
            return true;
        }
    }
    pl.last = 0;
    // groups padded to a power of two (reductions by shuffles instead of LDS atomics)
    int lpq = c.lpq, qt = c.qt;
    if ((lpq & (lpq - 1)) != 0) {
        int p2 = 1;
        while (p2 < lpq) p2 <<= 1;
        if (p2 <= 64 && (kMsdaThreads / p2) / p.M >= 1) {
            lpq = p2;
            qt = (kMsdaThreads / p2) / p.M;
        }
    }
    const bool pow2 = (lpq & (lpq - 1)) == 0 && lpq <= 64;
    const bool aln = !f64 && lpq == 16 && c.vec == 4 && (p.M * p.D) % 16 == 0 && p.D <= 48;
    const long long nsamp = (long long)qt * p.M * p.L * p.P;
    const long long acc = f64 ? 8 : 4;
    const long long lds = kLevelInfoBytes + nsamp * (f64 ? kBwdTapF64Bytes : kBwdTapF32Bytes) + (pow2 ? 0 : nsamp * 3 * acc);
    if (!(lds <= kMsdaLdsLimit)) return msda_refuse(pl, "msda backward: LDS request %lld too large", lds);
    pl.family = MSDA_K_BWD;
    pl.vec = c.vec;
    pl.pow2 = pow2;   // (aln implies it: 16-lane groups)
    pl.aln = aln;
    pl.qt = qt;
    pl.lpq = lpq;
    pl.na = c.lpq;
    pl.grid[0] = msda_ceil_div(p.Lq, qt);
    pl.grid[1] = p.N;
    pl.block = kMsdaThreads;
    pl.lds = (int)lds;
    return true;
}

// The launch of `p`: true with pl.family naming the kernel (MSDA_K_NONE: an empty call, nothing to
// launch), false with pl.why the refusal.  pl.last is valid either way.
inline bool msda_plan(const MsdaProblem& p, MsdaPlan& pl) {
    pl = MsdaPlan{};
    pl.grid[0] = pl.grid[1] = pl.grid[2] = 1;
    pl.last = kMsdaKeepLast;
    if (!msda_check_sizes(p, pl)) return false;
    switch (p.kind) {
        case MSDA_FORWARD: return msda_plan_forward(p, pl);
        case MSDA_FUSED: return msda_plan_fused(p, pl);
        case MSDA_BACKWARD: return msda_plan_backward(p, pl);
    }
    return msda_refuse(pl, "msda plan: unknown kind %lld", p.kind);
}

// ---------------------------------------------------------------------------------
// encoder sampler (msda_enc.hip): the strip plan
// ---------------------------------------------------------------------------------
constexpr int EQT = 16;            // queries per wave tile
constexpr int EMAP_PIX = 2544;     // LDS map pixels of 64 B (162,816 B; the level table fits beside)
// head_dim 36 (TAIL): the value as a 32-channel plane + a 4-channel TAIL plane (8 B per pixel,
// kinet_gemm_headmajor_split); the LDS map holds both, 72 B per pixel: 2256 main pixels, then the
// tail map (pixel x at ETB + 8x, the same pixel indexing as the main map).  Both fills round up
// (main: pieces of 16 pixels, tail: 256-byte pieces), so the main budget is a multiple of 16 (its
// last piece must not reach the tail map) and the tail's rounded fill stays inside the array
constexpr int EMAP_T = 2256;
constexpr int EL = 4;              // levels (the configs' value; host-checked)
constexpr int EHALO = 4;           // rows staged beyond a strip's query rows on each side

// launch plan (host): levels [0, fl) are gathered from the head map, levels [fl, EL) staged
// per strip: region l = 1 margin pixel + cap[l] rows x W + 1 margin pixel at map pixel base[l]
struct EncPlan {
    int fl, nstrip, zpix, used;
    int cap[EL], base[EL];
};

// LDS regions for strips of 1/n of the image: rows ceil(H/n) + 3 (pixel centres, the +1 corner
// row, a tile spilling into the next row) + 2*EHALO, at most the whole level + the two zero rows
inline bool plan_layout(const int64_t* shapes, int fl, int n, EncPlan& pl, int budget = EMAP_PIX) {
    int wmax = 0;
    for (int l = fl; l < EL; ++l) wmax = wmax > (int)shapes[2 * l + 1] ? wmax : (int)shapes[2 * l + 1];
    long long pos = ((long long)wmax + 2 + 15) / 16 * 16;   // zero margin: a whole 2x2 footprint of any level
    pl.zpix = (int)pos;
    for (int l = 0; l < EL; ++l) pl.cap[l] = pl.base[l] = 0;
    for (int l = fl; l < EL; ++l) {
        const long long H = shapes[2 * l], W = shapes[2 * l + 1];
        const long long strip = (H + n - 1) / n + 3 + 2 * EHALO;
        const long long cap = H + 2 < strip ? H + 2 : strip;
        pl.cap[l] = (int)cap;
        pl.base[l] = (int)pos;
        pos += (cap * W + 2 + 15) / 16 * 16;
        if (pos > budget) return false;
    }
    pl.used = (int)pos;
    pl.fl = fl;
    pl.nstrip = n;
    return true;
}

// the fewest gathered levels whose staged levels fit with strips of at least 16 tiles, then the
// fewest strips (>= what fits) whose workgroups fill >= 90 % of their last round of one per CU;
// forced_strips (kinet_msda_encoder_set_strips, 0 = none) is honoured when that many strips fit
inline bool enc_plan(const int64_t* shapes, int batch, int heads, int num_query, EncPlan& pl, bool tail, int cus,
                     int forced_strips) {
    const int budget = tail ? EMAP_T : EMAP_PIX;
    const int maps = batch * heads;
    const int ntile = (num_query + EQT - 1) / EQT;
    const int nmax = ntile / EQT > 1 ? ntile / EQT : 1;
    for (int fl = 0; fl < EL; ++fl) {
        int nmin = 0;
        for (int n = 1; n <= nmax && n <= 64; ++n)
            if (plan_layout(shapes, fl, n, pl, budget)) {
                nmin = n;
                break;
            }
        if (!nmin) continue;
        int n = nmin;
        const int cmax = 2 * nmin + cus / (maps > 1 ? maps : 1);
        for (int c = nmin; c <= (nmax < cmax ? nmax : cmax); ++c) {
            const long long wgs = (long long)maps * c, rounds = (wgs + cus - 1) / cus;
            if (wgs * 10 >= rounds * cus * 9) {
                n = c;
                break;
            }
        }
        if (forced_strips >= nmin && forced_strips <= (nmax < 64 ? nmax : 64) &&
            plan_layout(shapes, fl, forced_strips, pl, budget))
            return true;
        return plan_layout(shapes, fl, n, pl, budget);
    }
    return false;
}

}  // namespace kinet
