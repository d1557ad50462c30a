// Host-side planning of the attention-core launches (kinet_mha_core: the MFMA kernels of attn.hip
// and the FMA kernel of ops.hip): the per-head-dim geometry of the MFMA kernels, their LDS
// footprints, and the pure function that turns a described problem into one launch -- which
// kernel, with what grid, block and dynamic LDS.  mha_core_impl (ops.hip) launches what the plan
// names; kinet_mha_launch_plan answers from the same function.  No HIP, no thread-locals and no
// device query in this file: it runs on a machine without a GPU (tests/test_attn_plan_cpu.py).
#pragma once
#include "../../include/kinet_common.h"

namespace kinet {

// The MFMA kernels' geometry for one head dim (attn.hip's AttnCfg<D> is built from its row).
// The head dim is padded to `ksteps` 32-deep K-steps of S^T = K Q^T and to `vt` 16-row tiles of
// O^T; global rows move in `ppr` pieces of `piece_bytes` (head_dim-36 rows are 8-byte aligned only).
struct AttnGeo {
    int d;
    int krow;          // elements per staged key row: 80 / 144 bytes, conflict-free fragment reads
    int ksteps, vt;
    int piece_bytes, ppr;
    int maxk;          // keys the resident kernel holds; at head_dim 36 the next 32 keys pass the LDS limit
};
constexpr AttnGeo kAttnGeo[] = {
    {32, 40, 1, 2, 16, 4, 384},
    {36, 72, 2, 3, 8, 9, 640},
};
// the row of head dim d; d = 0 in the result: no MFMA kernel for it
constexpr AttnGeo attn_geo(int d) {
    for (const AttnGeo& g : kAttnGeo)
        if (g.d == d) return g;
    return AttnGeo{};
}

constexpr int kAttnStreamKT = 128;         // keys per tile of the streaming kernel
constexpr int kAttnQueries = 64;           // queries per MFMA workgroup: 4 waves x 16
constexpr int kAttnFmaQueries = 16;        // queries per workgroup of the FMA kernel
constexpr int kAttnBlock = 256;            // threads of every attention workgroup
constexpr int kAttnLdsLimit = 160 * 1024;  // what one workgroup may hold; a CU's LDS
constexpr int kAttnMaxGridYZ = 65535;      // heads / batch ride on grid y / z

// LDS bytes of n staged keys: key rows, the values transposed (d-major, rows of n + 8 elements),
// the additive key bias
constexpr int attn_staged_lds(const AttnGeo& g, int n) { return n * g.krow * 2 + g.vt * 16 * (n + 8) * 2 + n * 4; }
// resident kernel: the head's keys rounded up to whole 32-key blocks
constexpr int attn_resident_lds(const AttnGeo& g, int Lk) { return attn_staged_lds(g, (Lk + 31) & ~31); }
// streaming kernel: two tile buffers
constexpr int attn_stream_lds(const AttnGeo& g) { return 2 * attn_staged_lds(g, kAttnStreamKT); }

constexpr bool attn_geo_fits() {
    for (const AttnGeo& g : kAttnGeo)
        if (g.maxk % 32 != 0 || attn_resident_lds(g, g.maxk) > kAttnLdsLimit || attn_stream_lds(g) > kAttnLdsLimit) return false;
    return true;
}
static_assert(attn_geo_fits(), "LDS: one workgroup at the resident cap / two stream buffers");

enum AttnKernel {
    ATTN_K_FMA = 0,        // mha_kernel<T, D> (ops.hip)
    ATTN_K_RESIDENT = 1,   // mha_resident_kernel<T, D>
    ATTN_K_STREAM = 2,     // mha_stream_kernel<T, D>
};

struct AttnProblem {
    int dtype, head_dim;        // kinet_dtype
    int batch, heads, Lq, Lk;
    int ldq, ldk, ldv, ldo;     // row strides in elements
    int align;                  // bytes every one of the Q / K / V / O pointers is a multiple of
    bool dropout;
    int knob;                   // kinet_mha_set_mfma: 0 = FMA only, 2 = streaming for every MFMA call, else by Lk
};
struct AttnPlan {
    int kernel;                 // AttnKernel
    int grid[3], block, lds;    // lds: dynamic LDS bytes
};

// The launch of `p` (an empty batch or Lq gives a zero grid: nothing to launch).  The MFMA kernels
// take 16-bit operands of head dim 32 / 36 whose rows split into whole aligned pieces; the FMA
// kernel takes everything else.
constexpr AttnPlan attn_plan(const AttnProblem& p) {
    const AttnGeo g = attn_geo(p.head_dim);
    const bool mfma = p.knob != 0 && !p.dropout && g.d != 0 && (p.dtype == KINET_BF16 || p.dtype == KINET_F16) &&
                      (p.ldq | p.ldk | p.ldv | p.ldo) % (g.piece_bytes / 2) == 0 && p.align % g.piece_bytes == 0 &&
                      p.Lk >= 1 && p.batch <= kAttnMaxGridYZ && p.heads <= kAttnMaxGridYZ;
    if (!mfma) return AttnPlan{ATTN_K_FMA, {(p.Lq + kAttnFmaQueries - 1) / kAttnFmaQueries, p.heads, p.batch}, kAttnBlock, 0};
    const bool stream = p.knob == 2 || p.Lk > g.maxk;
    return AttnPlan{stream ? ATTN_K_STREAM : ATTN_K_RESIDENT,
                    {(p.Lq + kAttnQueries - 1) / kAttnQueries, p.heads, p.batch},
                    kAttnBlock,
                    stream ? attn_stream_lds(g) : attn_resident_lds(g, p.Lk)};
}

}  // namespace kinet
