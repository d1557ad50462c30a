// Host-side planning of the f32 attention training pair (attn_train.hip: kinet_mha_train_forward /
// kinet_mha_train_backward, every product on v_mfma_f32_16x16x4_f32): the per-head-dim geometry,
// the LDS footprints of the three kernels, and the pure function that turns a described problem
// into their launches.  The launchers launch what the plan names; kinet_mha_train_plan answers
// from the same function.  No HIP, no thread-locals and no device query in this file: it runs on
// a machine without a GPU (tests/test_attn_train_plan_cpu.py).
#pragma once
#include "../../include/kinet_common.h"

namespace kinet {

// One head dim's geometry.  A staged tile of 64 rows (keys, or queries in the dK/dV kernel) is
// kept in up to two LDS images, one per way an MFMA reads it (ds_read_b32: 32 banks, the two
// 32-lane halves of a wave are served separately):
//   * "row" image, `sa` floats per row: lane (c = l & 15, g = l >> 4) reads row c, column 4s + g
//     (the A operand of S^T = K Q^T).  sa = 2 * odd puts rows c = 0..15 on the 16 even banks, g on
//     the odd neighbour: conflict-free.
//   * "col" image, `st` floats per row, columns padded with zeros to `dt` 16-wide tiles: the lane
//     reads row 4g + r, column 16t + c (the A operand of O^T = V^T P^T).  st = 4 (mod 8) puts rows
//     4g + r of g = 0, 1 sixteen banks apart: conflict-free.
struct AttnTrainGeo {
    int d;
    int ks;     // 4-deep K-steps over the head dim: d / 4
    int dt;     // 16-row tiles of the transposed outputs (O^T, dQ^T, dK^T, dV^T): ceil(d / 16)
    int sa, st;
};
constexpr AttnTrainGeo kAttnTrainGeo[] = {
    {32, 8, 2, 34, 36},
    {36, 9, 3, 38, 52},
};
// the row of head dim d; d = 0 in the result: the pair refuses it
constexpr AttnTrainGeo attn_train_geo(int d) {
    for (const AttnTrainGeo& g : kAttnTrainGeo)
        if (g.d == d) return g;
    return AttnTrainGeo{};
}

constexpr int kAttnTrainQT = 64;             // queries per tile: 4 waves x 16
constexpr int kAttnTrainKT = 64;             // keys per tile: 4 16-key blocks, one accumulator each
constexpr int kAttnTrainBlock = 256;
constexpr int kAttnTrainLdsLimit = 160 * 1024;
constexpr int kAttnTrainMaxGridYZ = 65535;   // heads / batch ride on grid y / z

// Shortest key set for which the dense layers (models/transformer.py) take this pair rather than
// kinet_mha_core_dropout / kinet_mha_backward.  0: every dense call -- no crossover shows in
// profiles/detr_train_bench.jsonl ("attn_ab" lines: 1050x1050, 100x1050, 100x100 at B = 2 and 2100x2100
// at B = 8, p = 0 and 0.1): this pair's median is 1.56-2.70x ahead and the min-max ranges never overlap,
// the 100x100 decoder self-attention included (40.9 against 67.3 us).
constexpr int kAttnTrainMinLk = 0;

constexpr int attn_train_row_lds(const AttnTrainGeo& g) { return kAttnTrainKT * g.sa * 4; }
constexpr int attn_train_col_lds(const AttnTrainGeo& g) { return kAttnTrainKT * g.st * 4; }
// forward: K rows, V columns, the additive key bias
constexpr int attn_train_fwd_lds(const AttnTrainGeo& g) {
    return attn_train_row_lds(g) + attn_train_col_lds(g) + kAttnTrainKT * 4;
}
// dQ kernel: K rows and columns, V rows, the key bias
constexpr int attn_train_dq_lds(const AttnTrainGeo& g) {
    return 2 * attn_train_row_lds(g) + attn_train_col_lds(g) + kAttnTrainKT * 4;
}
// dK/dV kernel: Q and dO rows and columns, the tile's lse and delta
constexpr int attn_train_dkv_lds(const AttnTrainGeo& g) {
    return 2 * attn_train_row_lds(g) + 2 * attn_train_col_lds(g) + 2 * kAttnTrainQT * 4;
}

constexpr bool attn_train_geo_fits() {
    for (const AttnTrainGeo& g : kAttnTrainGeo)
        if (g.ks * 4 != g.d || g.dt * 16 < g.d || g.st < g.dt * 16 || g.sa < g.d || g.sa % 4 != 2 || g.st % 8 != 4 ||
            attn_train_fwd_lds(g) > kAttnTrainLdsLimit || attn_train_dq_lds(g) > kAttnTrainLdsLimit ||
            attn_train_dkv_lds(g) > kAttnTrainLdsLimit)
            return false;
    return true;
}
static_assert(attn_train_geo_fits(), "attention training pair: geometry / LDS of one workgroup");

struct AttnTrainProblem {
    int head_dim, batch, heads, Lq, Lk;
};
struct AttnTrainLaunch {
    int grid[3], block, lds;    // lds: dynamic LDS bytes; a zero grid: nothing to launch
};
struct AttnTrainPlan {
    bool supported;             // head dim 32 / 36, heads and batch within the grid limits
    bool dense_default;         // the dense layers take this pair for this key count
    AttnTrainLaunch fwd, dq, dkv;
};

constexpr int64_t attn_train_backward_workspace(int batch, int Lq, int heads) {
    return batch <= 0 || Lq <= 0 || heads <= 0 ? 0 : (int64_t)batch * heads * Lq;   // delta_i = dO_i . O_i
}

constexpr AttnTrainPlan attn_train_plan(const AttnTrainProblem& p) {
    const AttnTrainGeo g = attn_train_geo(p.head_dim);
    const bool ok = g.d != 0 && p.batch >= 0 && p.heads >= 1 && p.Lq >= 0 && p.Lk >= 0 &&
                    p.batch <= kAttnTrainMaxGridYZ && p.heads <= kAttnTrainMaxGridYZ;
    if (!ok) return AttnTrainPlan{};
    const bool empty = p.batch == 0 || p.Lq == 0;
    const int qt = empty ? 0 : (p.Lq + kAttnTrainQT - 1) / kAttnTrainQT;
    const int kt = empty ? 0 : (p.Lk + kAttnTrainKT - 1) / kAttnTrainKT;
    const int y = empty ? 0 : p.heads, z = empty ? 0 : p.batch;
    return AttnTrainPlan{true, p.Lk >= kAttnTrainMinLk,
                         {{qt, y, z}, kAttnTrainBlock, attn_train_fwd_lds(g)},
                         {{qt, y, z}, kAttnTrainBlock, attn_train_dq_lds(g)},
                         {{kt, kt ? y : 0, kt ? z : 0}, kAttnTrainBlock, attn_train_dkv_lds(g)}};
}

}  // namespace kinet
