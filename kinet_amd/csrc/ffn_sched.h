// The ring schedule of ffn_fused_rt2_kernel (ffn.hip) as pure functions: which chunk halves each
// wave role reads between two chunk barriers, which half-slots are restaged after a barrier, the
// vmcnt argument in front of it and the barrier's index.  The kernel takes its constants from
// here; kinet_ffn_sched answers from the same functions and tests/test_ffn_sched_cpu.py replays
// them against an event model of the ring (read-after-DMA, restage-after-read, barrier parity,
// vmcnt by counting).  No HIP in this file.
//
// The stream.  A workgroup walks `cnt` row tiles; per tile the ring carries `pch` pre-chunks (Wo of
// kinet_attn_out_ffn_fused; 0 otherwise) and then `nch` hidden chunks: chunk q = 0 .. total - 1 of
// the workgroup, total = cnt (pch + nch), lives in slot q % kFfnSchedSlots.  Every chunk is staged
// as two halves: fragments 0 .. FR/2 - 1 (FFN_HALF_LO: W1 of a hidden chunk) and FR/2 .. FR - 1
// (FFN_HALF_HI: its W2); each wave issues the same number of LDS-DMA operations per half.
//
// One barrier per chunk, for every wave: barrier q opens interval q.  In front of it a wave waits
// for its own DMA of both halves of chunk q; behind it it issues HI of chunk q + 1, then LO of
// chunk q + 2.  LO keeps two intervals of lead, HI one.
//
// Roles.  Waves 0 .. 3 (role 0) run, in the interval of hidden chunk c, phase A(c), ReLU, phase
// B(c).  Their SIMD partners, waves 4 .. 7 (role 1), run B(c - 1), A(c), ReLU(c): phase B lags one
// interval, so each role's ReLU / convert block and its first LDS reads fall beside the partner's
// MFMAs.  The lag ends with the tile: after A of the tile's last chunk role 1 runs that chunk's B in
// the same interval.  Pre-chunks are read whole by both roles in their own interval.  So HI of a
// hidden chunk q is read in interval q (role 0; role 1 at a tile's last chunk) or q + 1 (role 1),
// the first fragments of it already in front of barrier q + 1; HI's slot is restaged behind barrier
// q + 2 (as HI of q + 3), LO's behind barrier q + 1 (as LO of q + 3).
#pragma once

namespace kinet {

constexpr int kFfnSchedSlots = 3;      // ring slots (FfnKernel::ns of the FFN_K_RT2 entries)
constexpr int kFfnSchedRoleSplit = 4;  // waves below it are role 0, the others role 1 (SIMD partners w, w + 4)

enum FfnHalf { FFN_HALF_LO = 0, FFN_HALF_HI = 1 };

struct FfnChunkHalf {
    int chunk, half;
};
constexpr int kFfnSchedMaxIssue = 3, kFfnSchedMaxRead = 3;
struct FfnHalfList {
    int n;
    FfnChunkHalf e[3];
};

constexpr int ffn_sched_total(int cnt, int pch, int nch) { return cnt * (pch + nch); }
constexpr int ffn_sched_slot(int q) { return q % kFfnSchedSlots; }
constexpr int ffn_sched_role(int wave) { return wave < kFfnSchedRoleSplit ? 0 : 1; }
// intervals by which a role's phase B trails its phase A inside a tile
constexpr int ffn_sched_b_lag(int role) { return role; }

// what is issued behind a barrier, oldest first, as (chunks ahead, half); the prologue issues the
// halves these would have issued behind barriers -2 and -1
constexpr FfnChunkHalf kFfnSchedIssue[2] = {{1, FFN_HALF_HI}, {2, FFN_HALF_LO}};
constexpr int kFfnSchedIssues = 2;

// halves issued behind barrier q (q = -1: in the prologue, in front of barrier 0), in order
constexpr FfnHalfList ffn_sched_issue(int q, int total) {
    FfnHalfList l{};
    if (q < 0) {
        for (int b = -2; b < 0; ++b)
            for (int i = 0; i < kFfnSchedIssues; ++i) {
                const int c = b + kFfnSchedIssue[i].chunk;
                if (c >= 0 && c < total) l.e[l.n++] = FfnChunkHalf{c, kFfnSchedIssue[i].half};
            }
        // LO of chunk 0 comes from barrier -2's rule and HI of chunk 0 from barrier -1's: LO(0),
        // HI(0), LO(1) -- already oldest first
        return l;
    }
    for (int i = 0; i < kFfnSchedIssues; ++i) {
        const int c = q + kFfnSchedIssue[i].chunk;
        if (c < total) l.e[l.n++] = FfnChunkHalf{c, kFfnSchedIssue[i].half};
    }
    return l;
}

// DMA operations of a wave that may stay in flight at the wait in front of barrier q: the halves
// issued after both halves of chunk q, i.e. LO of chunk q + 1 (`half_ops` operations per half);
// nothing once the stream ends.  The kernel adds the loads it knows to be younger still.
constexpr int ffn_sched_vmcnt(int q, int total, int half_ops) { return q + 1 < total ? half_ops : 0; }

// position of chunk q in its tile: pre-chunk u (hidden = -1) or hidden chunk c (pre = -1)
constexpr int ffn_sched_pre(int q, int pch, int nch) { return q % (pch + nch) < pch ? q % (pch + nch) : -1; }
constexpr int ffn_sched_hidden(int q, int pch, int nch) { return q % (pch + nch) < pch ? -1 : q % (pch + nch) - pch; }

// halves a role reads between barrier q and barrier q + 1, in program order
constexpr FfnHalfList ffn_sched_reads(int role, int q, int pch, int nch) {
    FfnHalfList l{};
    const int c = ffn_sched_hidden(q, pch, nch), lag = ffn_sched_b_lag(role);
    if (c < 0 || lag == 0) {
        l.e[l.n++] = FfnChunkHalf{q, FFN_HALF_LO};
        l.e[l.n++] = FfnChunkHalf{q, FFN_HALF_HI};
        return l;
    }
    if (c > 0) l.e[l.n++] = FfnChunkHalf{q - 1, FFN_HALF_HI};   // the lagging phase B
    l.e[l.n++] = FfnChunkHalf{q, FFN_HALF_LO};
    if (c == nch - 1) l.e[l.n++] = FfnChunkHalf{q, FFN_HALF_HI};   // the lag ends with the tile
    return l;
}

// halves a role reads ahead in front of barrier q (behind barrier q - 1): the first fragments of
// the lagging phase B, so that its MFMAs start as the barrier releases
constexpr FfnHalfList ffn_sched_early_reads(int role, int q, int pch, int nch) {
    FfnHalfList l{};
    if (ffn_sched_b_lag(role) > 0 && ffn_sched_hidden(q, pch, nch) > 0) l.e[l.n++] = FfnChunkHalf{q - 1, FFN_HALF_HI};
    return l;
}

// s_barrier instructions a role executes behind the prologue: one per chunk whatever the role (the
// roles differ only in what lies between two barriers)
constexpr int ffn_sched_barriers(int /*role*/, int cnt, int pch, int nch) { return ffn_sched_total(cnt, pch, nch); }

}  // namespace kinet
