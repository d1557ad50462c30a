/* kinet_amd C-ABI: fused transformer FFN sub-layer (linear1 -> ReLU -> linear2 -> +residual
 * -> LayerNorm) in ONE launch, the hidden activations never leave the CU.
 *
 * Replaces, on the detection hot path, the post-norm FFN of the deformable encoder and
 * decoder layers:
 *   DeformableTransformerEncoderLayer.forward_ffn  (deformable_transformer.py:284-288)
 *   DeformableTransformerDecoderLayer.forward_ffn  (deformable_transformer.py:361-365)
 *     y = LayerNorm( x + linear2( relu( linear1(x) ) ) )
 * which the reference runs as two cuBLAS GEMMs + elementwise ops with the (M, F) hidden
 * tensor round-tripping through HBM.
 *
 * Weights are packed once (kinet_ffn_pack) from the PyTorch layouts W1 (F, D), W2 (D, F)
 * into a fragment-major stream of 1-KiB fragments, each laid out exactly as the 64 lanes of a
 * v_mfma_f32_16x16x32 operand read it, so the kernel moves it with LDS-DMA and reads it
 * conflict-free.  packed size = 2*D*F elements.  The layout of this and the three other packed
 * streams below is defined in one place, ffn_pack_src (csrc/ffn_plan.h); kinet_ffn_pack_map
 * writes it out as an index map.
 *
 * dtype: KINET_BF16 or KINET_F16 for X, the packed weights and Y (f32 accumulation, the
 * hidden activations rounded to dtype exactly where the unfused GEMM would store them).
 * b1 (F), b2 (D) f32; ln_gamma/ln_beta (D) f32 or both NULL (then y = x + FFN(x)).
 * D in {256, 288}, F % 32 == 0, ldx/ldy multiples of 8, 16-byte aligned X, Y, packed.
 */
#ifndef KINET_FFN_H_
#define KINET_FFN_H_

#include "kinet_common.h"

#ifdef __cplusplus
extern "C" {
#endif

int kinet_ffn_pack(const void* W1, const void* W2, void* packed, int D, int F, int dtype,
                   kinet_stream_t stream);

int kinet_ffn_fused(const void* X, int ldx, const void* packed, const float* b1, const float* b2,
                    const float* ln_gamma, const float* ln_beta, float ln_eps, void* Y, int ldy,
                    int M, int D, int F, int dtype, kinet_stream_t stream);

/* Encoder layer tail in ONE launch: the deformable attention's out-projection, its residual add
 * and post-norm, then the FFN sub-layer above (DeformableTransformerEncoderLayer.forward,
 * deformable_transformer.py:290-299 after the sampler):
 *   x = LayerNorm1( R + A Wo^T + bo )                      (M, D), never written to memory
 *   y = LayerNorm2( x + linear2( relu( linear1(x) ) ) )     (M, D)
 * A = the sampler's output, row stride lda; R = the layer input (residual), row stride ldr.
 * x is rounded to dtype exactly once, after LayerNorm1 -- the point where the two-launch path
 * (kinet_gemm_ex with the LayerNorm epilogue, then kinet_ffn_fused) stores it -- and that rounded
 * x is both linear1's operand and the FFN's residual.  The out-projection sums run in f32 in
 * ascending k, in another order than the GEMM's, so a rounding of x may differ from the
 * two-launch path's by one ulp of dtype.
 * kinet_ffn_pack_attn: Wo (D, D), W1 (F, D), W2 (D, F) of dtype -> D*D + 2*D*F elements: first
 * Wo as (D/32) * (D/16) 1-KiB MFMA operand fragments, k-step major (ffn_pack_src, kind
 * KINET_FFN_PACK_ATTN), i.e. at D = 256 four ring chunks of 32 fragments; then exactly the stream
 * kinet_ffn_pack writes.
 * kinet_attn_out_ffn_fused: D = 256 only (at D = 288 Wo does not fill whole ring chunks:
 * KINET_ERR_ARG), F % 32 == 0, F <= 2048; lda, ldr, ldy >= D and multiples of 8; every pointer
 * 16-byte aligned; every tensor below 2 GiB; bo, ln1_gamma, ln1_beta (D) f32 required; b1 (F),
 * b2 (D) f32; ln2_gamma / ln2_beta (D) f32 or both NULL (then y = x + FFN(x)); Y must not overlap
 * A or R.  Correct for every M >= 1 (M == 0: nothing is launched); it runs on the 8-wave x
 * 32-row tile, which pays from about 16384 rows. */
int kinet_ffn_pack_attn(const void* Wo, const void* W1, const void* W2, void* packed, int D, int F,
                        int dtype, kinet_stream_t stream);

int kinet_attn_out_ffn_fused(const void* A, int lda, const void* R, int ldr, const void* packed,
                             const float* bo, const float* ln1_gamma, const float* ln1_beta,
                             float ln1_eps, const float* b1, const float* b2, const float* ln2_gamma,
                             const float* ln2_beta, float ln2_eps, void* Y, int ldy, int M, int D,
                             int F, int dtype, kinet_stream_t stream);

/* ResNet bottleneck pair (torchvision Bottleneck as the reference instantiates it,
 * backbone.py:94-108): block i's conv3 + FrozenBN + residual + ReLU and the next block's conv1 +
 * FrozenBN + ReLU, both 1x1 stride 1 over NHWC rows, in ONE launch (phase A = conv3, its
 * rounded output chunk is stored to Y and is phase B's operand; phase B = the next conv1):
 *   Y = relu(X (s3 W3)^T + b3 + R)   (M, F)   -- the block output, the next block's residual
 *   T = relu(Y (s1 W1)^T + b1)       (M, DB)  -- the next block's conv1 output
 * kinet_bottleneck_pack: f32 W3 (F, D), W1 (DB, F), FrozenBN scales s3 (F), s1 (DB) -> the FFN
 * fragment stream ((D + DB) * F elements of dtype) with each weight row scaled before rounding.
 * F = 4 D, D in {64, 128, 256}; DB = D (inside a stage) or, at D = 64, DB = 128 (stage 1's last
 * block -> stage 2's first conv1, which is stride 1 in torchvision's v1.5 Bottleneck); X rows of
 * stride ldx; R, Y, T dense rows; b3 (F), b1 (DB) f32; dtype KINET_BF16 / KINET_F16. */
int kinet_bottleneck_pack(const float* W3, const float* W1, const float* s3, const float* s1,
                          void* packed, int D, int F, int DB, int dtype, kinet_stream_t stream);

int kinet_bottleneck_pair(const void* X, int ldx, const void* R, const void* packed, const float* b3,
                          const float* b1, void* Y, void* T, int M, int D, int F, int DB, int dtype,
                          kinet_stream_t stream);

/* Stage 1's first pair with block 0's downsample branch folded in: the identity of layer1[0] is
 * a 1x1 stride-1 64 -> 256 conv + FrozenBN over the block input X0 (the max-pool output), so the
 * block output is one GEMM over the concatenated K = 64 + 64 and the 256-channel identity tensor
 * is never written or read:
 *   Y = relu(X (s3 W3)^T + X0 (s_ds W_ds)^T + b3ds)   (M, F)   b3ds = b3 + b_ds, summed in f32
 *   T = relu(Y (s1 W1)^T + b1)                        (M, DB)
 * The identity branch stays in the f32 accumulators (the unfused path rounds it to dtype first
 * and applies s_ds in the epilogue), so outputs differ from downsample launch + pair at rounding
 * level.
 * kinet_bottleneck_pack_ds: f32 W3 (F, 64), W_ds (F, 64), W1 (DB, F), scales s3 (F), s_ds (F),
 * s1 (DB) -> (64 + 64 + DB) * F elements of dtype; per 32-channel chunk the W3 fragments, then
 * the W_ds fragments, then the W1 fragments, each row scaled before the one rounding.
 * D = 64, F = 256, DB = 64 only (KINET_ERR_ARG otherwise); X rows of stride ldx >= 64, X0 rows
 * of stride ldx0 >= 64 (multiples of 8); Y, T dense; every tensor below 2 GiB; b3ds (F), b1 (DB)
 * f32; dtype KINET_BF16 / KINET_F16. */
int kinet_bottleneck_pack_ds(const float* W3, const float* Wds, const float* W1, const float* s3,
                             const float* sds, const float* s1, void* packed, int D, int F, int DB,
                             int dtype, kinet_stream_t stream);

int kinet_bottleneck_pair_ds(const void* X, int ldx, const void* X0, int ldx0, const void* packed,
                             const float* b3ds, const float* b1, void* Y, void* T, int M, int D, int F,
                             int DB, int dtype, kinet_stream_t stream);

/* Diagnostics and planning (host side, per calling thread; no reference counterpart).
 * kinet_ffn_set_debug: A/B and test knobs, the FfnDebug bits of csrc/ffn_plan.h; returns the
 * previous value.
 * kinet_ffn_grid_cap: an upper bound on the grid of the four entry points' launches (0 = none,
 * the default); returns the previous value.  Every kernel walks its row tiles by gridDim.x, so a
 * bound only moves tiles between workgroups: same outputs bit for bit (tests reach the multi-tile
 * walk at a few tiles with it).
 * kinet_ffn_launch_plan: the launch kinet_ffn_fused, kinet_attn_out_ffn_fused, kinet_bottleneck_pair
 * or kinet_bottleneck_pair_ds makes for a described problem on a device of `cus` compute units,
 * under the calling thread's debug bits, its kinet_ffn_grid_cap and the kinet_set_solo_launch
 * policy as a real call reads them (csrc/ffn_plan.h; no GPU call).  problem: KINET_FFNP_FIELDS
 * ints, plan_out: KINET_FFNPL_FIELDS ints.  KINET_ERR_ARG with the entry point's message where it refuses D or DB (its other argument
 * checks are not repeated here).  M = 0: grid 0, nothing would be launched.
 * kinet_ffn_last_kernel: KINET_FFNPL_KERNEL of the calling thread's last launch of these four entry
 * points (-1: none yet); kinet_ffn_kernel_name: the instantiation's name but for the element type
 * (NULL: no such index).
 * kinet_ffn_pack_map: the whole layout of a packed stream of `kind` as (source matrix in the pack
 * call's argument order, row, column) per packed element: out holds 3 ints for each of the stream's
 * elements (kinet_ffn_pack: 2 D F; _pack_attn: D D + 2 D F; kinet_bottleneck_pack: (D + DB) F;
 * _pack_ds: (2 D + DB) F).  D, F, DB multiples of 32; DB = D but for KINET_FFN_PACK_PAIR. */
enum kinet_ffn_problem_field {
    KINET_FFNP_KIND = 0,   /* 0 kinet_ffn_fused, 1 kinet_attn_out_ffn_fused, 2 kinet_bottleneck_pair, 3 _pair_ds */
    KINET_FFNP_M, KINET_FFNP_D, KINET_FFNP_F, KINET_FFNP_DB,
    KINET_FFNP_FIELDS
};
enum kinet_ffn_plan_field {
    KINET_FFNPL_KERNEL = 0,   /* index into the table of instantiations (kinet_ffn_kernel_name) */
    KINET_FFNPL_TILES,        /* row tiles of KINET_FFNPL_TILE_ROWS rows */
    KINET_FFNPL_GRID, KINET_FFNPL_BLOCK, KINET_FFNPL_WAVES,
    KINET_FFNPL_TILE_ROWS,
    KINET_FFNPL_WG_TILES,     /* row tiles a workgroup works on at a time */
    KINET_FFNPL_WG_PER_CU,    /* resident workgroups per CU the grid is sized for */
    KINET_FFNPL_LDS,          /* LDS bytes of a workgroup */
    KINET_FFNPL_FIELDS
};
enum kinet_ffn_pack_kind { KINET_FFN_PACK_FFN = 0, KINET_FFN_PACK_PAIR, KINET_FFN_PACK_DS, KINET_FFN_PACK_ATTN };

/* kinet_ffn_sched: the ring schedule of the 8-wave x 32-row FFN kernel (csrc/ffn_sched.h; no GPU
 * call) for a workgroup that walks `cnt` row tiles of `pch` pre-chunks (4 with the attention
 * out-projection, else 0) and `nch` hidden chunks each: what a wave of `role` (0: waves 0-3, 1: waves
 * 4-7) does around the barrier of ring chunk q in [0, cnt (pch + nch)), or in the prologue (q = -1:
 * the issue list only).  A chunk half is a pair (chunk, half), half 0 = fragments 0 .. FR/2 - 1 (W1
 * of a hidden chunk), 1 = the rest (W2); `half_ops` = LDS-DMA operations of a wave per half.  Lists
 * are in program order, unused places -1.  KINET_ERR_ARG outside these ranges. */
enum kinet_ffn_sched_field {
    KINET_FFNS_TOTAL = 0,     /* ring chunks of the workgroup */
    KINET_FFNS_BARRIERS,      /* barriers a wave of this role executes behind the prologue, in all */
    KINET_FFNS_BARRIER,       /* index of the barrier that opens interval q (= q) */
    KINET_FFNS_SLOT,          /* ring slot of chunk q */
    KINET_FFNS_VMCNT,         /* vmcnt argument of the wait in front of barrier q (the ring's own operations) */
    KINET_FFNS_N_ISSUE,       /* halves issued behind barrier q, then 3 (chunk, half) pairs */
    KINET_FFNS_ISSUE,
    KINET_FFNS_N_EARLY = KINET_FFNS_ISSUE + 6,   /* halves read ahead in front of barrier q (behind barrier q - 1) */
    KINET_FFNS_EARLY,
    KINET_FFNS_N_READ = KINET_FFNS_EARLY + 6,    /* halves read between barriers q and q + 1 */
    KINET_FFNS_READ,
    KINET_FFNS_FIELDS = KINET_FFNS_READ + 6
};

int kinet_ffn_set_debug(int flags);
int kinet_ffn_grid_cap(int max_wgs);
int kinet_ffn_launch_plan(const int* problem, int cus, int* plan_out);
int kinet_ffn_last_kernel(void);
const char* kinet_ffn_kernel_name(int kernel);
int kinet_ffn_pack_map(int kind, int D, int F, int DB, int32_t* out);
int kinet_ffn_sched(int role, int cnt, int pch, int nch, int q, int half_ops, int* out);

#ifdef __cplusplus
}
#endif

#endif /* KINET_FFN_H_ */
