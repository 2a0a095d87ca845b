// voxnav_trust.hip -- the learner's trust-region gate: sb3 PPO.train's
//   if target_kl is not None and approx_kl_div > 1.5 * target_kl: stop
// decided on the device, so no minibatch waits for a host read of the KL.
// Every fused loss call leaves its approx kl in stats[4]; vn_kl_gate, between
// that call and vn_adam_step, compares it with the threshold and writes the
// word vn_adam_step takes as `skip`.  `stop` is sticky: the minibatch whose KL
// crosses the threshold is logged (ran = 1) and not stepped, and every later
// one is neither (ran = 0), until the caller zeroes the word.  One thread.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "vn_common.h"

using vn_detail::fail;

namespace {

__global__ __launch_bounds__(64) void kl_gate_kernel(const double *__restrict__ stats, int kl_index, double threshold,
                                                     const int32_t *__restrict__ err, int32_t *__restrict__ stop,
                                                     int32_t *__restrict__ skip, uint8_t *__restrict__ ran) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int32_t was = stop[0];
    if (ran) ran[0] = was == 0 ? 1 : 0;
    int32_t now = was;
    if (was == 0 && stats[kl_index] > threshold) {   // strict; a NaN KL does not stop
        now = 1;
        stop[0] = 1;
    }
    skip[0] = (now != 0 || (err && err[0] != 0)) ? 1 : 0;
}

}  // namespace

extern "C" {

int vn_kl_gate(const double *stats, int32_t kl_index, double threshold, const int32_t *err, int32_t *stop,
               int32_t *skip, uint8_t *ran, void *stream) {
    if (!stats || !stop || !skip) return fail(VN_ERR_INVALID, "NULL argument");
    if (kl_index < 0 || kl_index > 15) return fail(VN_ERR_INVALID, "kl_index %d outside 0..15", kl_index);
    if (!(threshold > 0.0) || !std::isfinite(threshold))
        return fail(VN_ERR_INVALID, "threshold must be a positive finite number");
    hipLaunchKernelGGL(kl_gate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats, kl_index, threshold, err, stop,
                       skip, ran);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // extern "C"
