// libvalley_hip_spec_sample.so (include/valley_hip_spec_sample.h): the draw counters of a speculative verify step under seeded
// sampling.  Row j of the step draws the token of sequence index pos + j + 1 (vly_argmax: ctr[j] + ctr_add, ctr_add = 1), so the
// table is pos + j with the position read — and clamped as the step's other kernels clamp it — on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "companion_capi.hpp"
#include "../../include/valley_hip_spec_sample.h"

namespace {

// one wave; lanes 0 .. k store one word each
__global__ void __launch_bounds__(64) spec_counters_kernel(const int32_t* __restrict__ pos_dev, int k, int ctx_max,
                                                           int32_t* __restrict__ ctr) {
    const int j = threadIdx.x;
    if (j > k) return;
    const int p = max(0, min(pos_dev[0], ctx_max - (k + 1)));
    ctr[j] = p + j;
}

}  // namespace

VLY_COMPANION_CAPI(spec_sample, VLY_SPEC_SAMPLE_ABI_VERSION)

extern "C" int vly_spec_counters(const int32_t* pos_dev, int k, int ctx_max, int32_t* ctr, void* stream) {
    if (!pos_dev || !ctr || k < 1 || k > VLY_SPEC_SAMPLE_MAX_DRAFT || ctx_max < k + 1 || ((uintptr_t)pos_dev & 3) || ((uintptr_t)ctr & 3)) {
        set_error("vly_spec_counters: bad args k=%d (1..%d) ctx_max=%d (>= k + 1; pos_dev and ctr required, 4-byte aligned)", k,
                  VLY_SPEC_SAMPLE_MAX_DRAFT, ctx_max);
        return -22;
    }
    hipLaunchKernelGGL(spec_counters_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pos_dev, k, ctx_max, ctr);
    return check_launch("vly_spec_counters");
}
