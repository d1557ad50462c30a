// The resize index rules of the segmentation kernels, shared by the inference resampling
// (segm.hip: PostProcessSegm, the tracker's masks) and the fused mask loss (segm_train.hip), so
// that every kernel that upsamples mask logits rounds its source positions alike.
#pragma once
#include <hip/hip_runtime.h>

namespace kinet {

// torch's area_pixel_compute_source_index (align_corners = false) + guard_index_and_lambda
__device__ __forceinline__ void bilinear_src(int dst, float scale, int in, int& i0, int& i1, float& l1) {
    const float real = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    i0 = min((int)floorf(real), in - 1);
    l1 = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
}

// torch's legacy mode="nearest" rule (nearest_neighbor_compute_source_index) in f32
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
    return min((int)floorf((float)dst * scale), in - 1);
}

}  // namespace kinet
