// voxnav_mask.hip -- invalid-action masking on the collector's side (Huang &
// Ontanon 2020; sb3_contrib MaskablePPO's env.action_masks()): the mask of a
// CubicEnv observation and the action / value heads with a masked Categorical
// draw.  include/voxnav.h has the formulas (vn_action_mask,
// vn_policy_head_masked); csrc/voxnav_masked_loss.hip is the learner's side.
//
// The mask is exact, not a heuristic: get_obs casts a ray of length >= 1 in
// all six directions before it builds the window (envs/CubicEnv.py:229-275),
// so each in-bounds neighbour of the agent is known wall (-2) or known free
// (>= 0) in the window (:322-332), which reads -1 only out of bounds.
//
//   action_mask_kernel         16 lanes per agent, 4 agents per wave: lanes
//       0..3 load the facing one-hot obs[64..67], lanes 4..9 the six
//       neighbour cells (ring +y, +x, -y, -x, then +z, -z), one float each, so
//       one load instruction fetches everything four agents need (the 4-5
//       64-B lines of each 320-B row that hold the 10 floats; a lane per agent
//       would spread every load over 64 rows).  A wave ballot of "is the
//       facing" / "is blocked" hands each group its 10 bits; lane 0 rotates
//       the ring by the facing and stores the byte.
//   policy_head_masked_kernel  policy_head_kernel (voxnav_collect.hip) with the
//       allowed set S: the same tiling, dot products and operation order, so a
//       full S gives its bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vn_common.h"

using vn_detail::fail;
using vn_detail::philox_word0;

namespace {

constexpr int MASK_MAX_A = 8;   // HEAD_MAX_A of voxnav_collect.hip

__global__ __launch_bounds__(256) void action_mask_kernel(const float *__restrict__ obs, int64_t ldo, int N,
                                                          uint8_t *__restrict__ mask) {
    const int lane = threadIdx.x & 63, grp = lane >> 4, l = lane & 15;
    const int64_t n = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = n < N;
    // window index (dx+2) 16 + (dy+2) 4 + (dz+2), centre 42
    int col = 64 + l;                                   // l < 4: the facing one-hot
    col = l == 4 ? 46 : l == 5 ? 58 : l == 6 ? 38 : l == 7 ? 26 : l == 8 ? 43 : l == 9 ? 41 : col;
    float v = 0.5f;                                     // neither a facing, a wall nor out of bounds
    if (live && l < 10) v = obs[n * ldo + col];
    // wall: (-2 + 2) / 22 = 0; out of bounds: (-1 + 2) / 22
    const bool bit = l < 4 ? v == 1.0f : (v == 0.0f || v == 1.0f / 22.0f);
    const unsigned bits = (unsigned)(__ballot(bit) >> (16 * grp)) & 0xffffu;
    if (!live || l != 0) return;
    const unsigned fb = bits & 15u;
    const int f = fb ? __ffs(fb) - 1 : 0;               // the index of the 1 in obs[64:68]
    // action a < 4 moves along ring entry (f + a) % 4 (SURVEY.md App. A.1's table)
    const unsigned free4 = ~(bits >> 4) & 15u;
    const unsigned lo = ((free4 >> f) | (free4 << (4 - f))) & 15u;
    const unsigned ud = ~(bits >> 8) & 3u;              // up (+z), down (-z)
    mask[n] = (uint8_t)(lo | (ud << 4));
}

// policy_head_kernel's body (f32 latents) up to the logits, then the draw over
// the allowed actions
__global__ __launch_bounds__(256) void policy_head_masked_kernel(
    const float *__restrict__ lat_pi, const float *__restrict__ lat_vf, int N, int P, const float *__restrict__ wa,
    const float *__restrict__ ba, int A, const float *__restrict__ wv, const float *__restrict__ bv,
    const uint8_t *__restrict__ mask, uint64_t seed, uint64_t t, int64_t gid_base, int deterministic,
    int32_t *__restrict__ actions, float *__restrict__ values, float *__restrict__ logp) {
    extern __shared__ float sw[];  // [A][P] action weights, then [P] value weights
    const int nw = (lat_pi ? A * P : 0);
    for (int i = threadIdx.x; i < nw; i += blockDim.x) sw[i] = wa[i];
    if (lat_vf)
        for (int i = threadIdx.x; i < P; i += blockDim.x) sw[A * P + i] = wv[i];
    __syncthreads();
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int64_t n = (int64_t)blockIdx.x * 16 + g;
    const bool live = n < N;
    float acc[MASK_MAX_A + 1];
#pragma unroll
    for (int a = 0; a <= MASK_MAX_A; ++a) acc[a] = 0.0f;
    if (live) {
        for (int k = l * 4; k < P; k += 64) {
            if (lat_pi) {
                const float4 x = *reinterpret_cast<const float4 *>(lat_pi + n * P + k);
#pragma unroll
                for (int a = 0; a < MASK_MAX_A; ++a) {
                    if (a < A) {
                        const float *w = sw + a * P + k;
                        acc[a] += x.x * w[0];
                        acc[a] += x.y * w[1];
                        acc[a] += x.z * w[2];
                        acc[a] += x.w * w[3];
                    }
                }
            }
            if (lat_vf) {
                const float4 x = *reinterpret_cast<const float4 *>(lat_vf + n * P + k);
                const float *w = sw + A * P + k;
                acc[MASK_MAX_A] += x.x * w[0];
                acc[MASK_MAX_A] += x.y * w[1];
                acc[MASK_MAX_A] += x.z * w[2];
                acc[MASK_MAX_A] += x.w * w[3];
            }
        }
    }
#pragma unroll
    for (int a = 0; a <= MASK_MAX_A; ++a) {
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) acc[a] += __shfl_xor(acc[a], m, 16);
    }
    if (!live || l != 0) return;
    if (lat_vf) values[n] = acc[MASK_MAX_A] + bv[0];
    if (!lat_pi) return;
    const unsigned full = (1u << A) - 1u;
    unsigned S = mask[n] & full;
    S = S ? S : full;                                   // an empty set counts as all allowed
    float lg[MASK_MAX_A];
    float mx = -INFINITY;
#pragma unroll
    for (int a = 0; a < MASK_MAX_A; ++a) {
        lg[a] = (a < A) ? acc[a] + ba[a] : -INFINITY;
        if ((S >> a) & 1u) mx = fmaxf(mx, lg[a]);
    }
    float se = 0.0f;
#pragma unroll
    for (int a = 0; a < MASK_MAX_A; ++a)
        if ((S >> a) & 1u) se += expf(lg[a] - mx);
    const float lse = mx + logf(se);
    const int last = 31 - __clz(S);                     // the highest allowed index
    int act = -1;
    if (deterministic) {
        float best = 0.0f;
#pragma unroll
        for (int a = 0; a < MASK_MAX_A; ++a)
            if (((S >> a) & 1u) && (act < 0 || lg[a] > best)) {
                best = lg[a];
                act = a;
            }
    } else {
        const uint64_t gid = (uint64_t)(gid_base + n);
        const uint32_t w0 = philox_word0(seed, gid, t | (1ull << 63));
        const float u = (float)(w0 >> 8) * (1.0f / 16777216.0f);
        float cdf = 0.0f;
#pragma unroll
        for (int a = 0; a < MASK_MAX_A; ++a) {
            if (((S >> a) & 1u) && a < last) {
                cdf += expf(lg[a] - lse);
                if (u < cdf && act < 0) act = a;        // the first crossing
            }
        }
        act = act < 0 ? last : act;
    }
    float la = lg[0];
#pragma unroll
    for (int a = 1; a < MASK_MAX_A; ++a) la = a == act ? lg[a] : la;
    actions[n] = act;
    logp[n] = la - lse;
}

}  // namespace

extern "C" {

int vn_action_mask(const float *obs, int64_t ldo, int32_t N, uint8_t *mask, void *stream) {
    if (!obs || !mask) return fail(VN_ERR_INVALID, "NULL argument");
    if (N < 1 || ldo < VN_OBS_DIM) return fail(VN_ERR_INVALID, "bad sizes N=%d ldo=%lld", N, (long long)ldo);
    hipLaunchKernelGGL(action_mask_kernel, dim3((unsigned)(((int64_t)N + 15) / 16)), dim3(256), 0, (hipStream_t)stream,
                       obs, ldo, (int)N, mask);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int vn_policy_head_masked(const float *latent_pi, const float *latent_vf, int32_t N, int32_t P, const float *w_action,
                          const float *b_action, int32_t n_actions, const float *w_value, const float *b_value,
                          const uint8_t *mask, uint64_t sample_seed, uint64_t t, int64_t agent_id_base,
                          int32_t deterministic, int32_t *actions, float *values, float *log_probs, void *stream) {
    if (!latent_pi || !mask) return fail(VN_ERR_INVALID, "latent_pi and mask are required");
    if (!w_action || !b_action || !actions || !log_probs) return fail(VN_ERR_INVALID, "NULL action-head argument");
    if (latent_vf && (!w_value || !b_value || !values)) return fail(VN_ERR_INVALID, "NULL value-head argument");
    if (N < 1 || P < 4 || (P & 3) || P > 4096) return fail(VN_ERR_INVALID, "bad sizes N=%d P=%d", N, P);
    if (n_actions < 1 || n_actions > MASK_MAX_A)
        return fail(VN_ERR_INVALID, "n_actions must be in 1..%d (got %d)", MASK_MAX_A, n_actions);
    const size_t lds = (size_t)(n_actions + 1) * P * sizeof(float);
    hipLaunchKernelGGL(policy_head_masked_kernel, dim3((unsigned)(((int64_t)N + 15) / 16)), dim3(256), lds,
                       (hipStream_t)stream, latent_pi, latent_vf, (int)N, (int)P, w_action, b_action, (int)n_actions,
                       w_value, b_value, mask, sample_seed, t, agent_id_base, (int)deterministic, actions, values,
                       log_probs);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // extern "C"
