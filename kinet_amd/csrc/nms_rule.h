// The two rules nms_kernel (ops.hip) and nms_segments_kernel (track.hip) share, so that one list and a
// segment of the bank are ordered and suppressed alike.
#pragma once
#include <hip/hip_runtime.h>

namespace kinet {

// a score as a monotone integer key: a strict total order even with NaNs (which rank first, as
// torch.sort(descending=True) places them), so every rank is written once
__device__ __forceinline__ uint32_t nms_score_key(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// does the kept box (x1, y1, x2, y2) of area ai suppress box b (xyxy)?  IoU > thresh (torchvision.ops.nms)
__device__ __forceinline__ bool nms_suppresses(float x1, float y1, float x2, float y2, float ai,
                                               const float* __restrict__ b, float thresh) {
    const float w = fmaxf(fminf(x2, b[2]) - fmaxf(x1, b[0]), 0.f);
    const float h = fmaxf(fminf(y2, b[3]) - fmaxf(y1, b[1]), 0.f);
    const float inter = w * h;
    return inter / (ai + (b[2] - b[0]) * (b[3] - b[1]) - inter) > thresh;
}

}  // namespace kinet
