// voxnav_rnorm.hip -- return-based reward normalisation on the rollout
// buffer (SB3 VecNormalize(norm_reward=True); the rule is stated in
// include/voxnav.h, its arithmetic is csrc/ret_rms.h).  Handle-less and
// stream-ordered like vn_gae; no host read, no floating-point atomics, every
// sum in a fixed order, so the statistics do not depend on the sharding:
//
//   moments_kernel   vn_return_moments: one wave per 64-agent chunk, aligned to
//                    the global chunks because agent_id_base % 64 == 0.  Per
//                    tile of 64 steps: one lane per agent scans the steps
//                    (coalesced rows, as gae_kernel), carries the discounted
//                    return in a register and lays the returns out in LDS;
//                    then one lane per step sums its row over the butterfly's
//                    tree (rr_chunk) -- 64 steps reduce side by side with no
//                    cross-lane traffic.  8 B read per (t, agent).
//   tree_kernel      vn_reward_normalize: one block per step merges the
//                    C_global chunk triples up the binary tree, in LDS tiles
//                    of 512 leaves (an aligned tile is a subtree) and then
//                    over the tile roots; the root goes to the row's slot 0.
//   chain_kernel     one wave: the roots to LDS and the chain-independent
//                    half of the update in parallel, one lane for the T
//                    dependent merges (two dependent f64 divisions a step),
//                    the scales sqrt(var_t + eps) in parallel again, to the
//                    row's slot 0.
//   scale_kernel     rewards[t][i] = clamp(r / scale_t) in f64, rounded once;
//                    4 B read + 4 B written per (t, agent), 16 B a lane where
//                    N and the base allow.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "vn_common.h"
#include "ret_rms.h"

using vn_detail::fail;

namespace {

constexpr int RN_BLOCK = 256;
constexpr int RN_TS = RR_CHUNK;         // steps per LDS tile of the moments scan: one per lane in the reduction
constexpr int RN_LD = RN_TS + 1;        // its row stride in doubles: rows a lane apart fall in different banks
constexpr int RN_U = 16;                // steps whose loads are issued together
constexpr int RN_CHAIN = 1024;          // steps per LDS tile of the chain
constexpr int RN_TILE = 512;            // leaves per LDS tile of the tree (2 per thread)
constexpr int RN_MAX_TILES = 512;       // C_global <= RN_TILE * RN_MAX_TILES = 262144 chunks (16.7 M agents)
constexpr int RN_MAX_STEPS = 65535;     // steps ride gridDim.y

static_assert(sizeof(RrTriple) == 3 * sizeof(double), "a triple is three packed doubles");
static_assert(RN_TILE == 2 * RN_BLOCK && RN_MAX_TILES <= 2 * RN_BLOCK, "one tree node per thread and level");

__global__ __launch_bounds__(RR_CHUNK) void moments_kernel(const float *__restrict__ rew,
                                                           const float *__restrict__ dones, int t0, int t1, int N,
                                                           double gamma, double *__restrict__ ret,
                                                           double *__restrict__ partials) {
    __shared__ double tile[RN_TS * RN_LD];          // [step][agent]
    const int lane = (int)threadIdx.x;
    const int chunk = (int)blockIdx.x, C = (int)gridDim.x;
    const int i = chunk * RR_CHUNK + lane;
    const bool present = i < N;
    const int m = N - chunk * RR_CHUNK < RR_CHUNK ? N - chunk * RR_CHUNK : RR_CHUNK;
    const int col = present ? i : N - 1;
    double acc = present ? ret[i] : 0.0;
    for (int tb = t0; tb < t1; tb += RN_TS) {
        const int cnt = t1 - tb < RN_TS ? t1 - tb : RN_TS;
        for (int ub = 0; ub < cnt; ub += RN_U) {    // lane = agent: the returns of steps tb + ub ..
            float r[RN_U], d[RN_U];
#pragma unroll
            // unpredicated loads: steps past the tile and absent lanes re-read an element of the call's own
            // range (`on ? rew[o] : 0` became a branch per load and one load in flight: 86 -> 30 us)
            for (int u = 0; u < RN_U; ++u) {
                const int t = tb + ub + u < t1 ? tb + ub + u : t1 - 1;
                const size_t o = (size_t)t * N + col;
                r[u] = rew[o];
                d[u] = dones[o];
            }
#pragma unroll
            for (int u = 0; u < RN_U; ++u) {
                if (ub + u < cnt) {
                    acc = rr_return(acc, gamma, r[u]);
                    tile[(ub + u) * RN_LD + lane] = present ? acc : 0.0;
                    if (d[u] != 0.0f) acc = 0.0;
                }
            }
        }
        __syncthreads();
        if (lane < cnt) {                           // lane = step tb + lane: its row's triple
            const RrTriple tr = rr_chunk(tile + lane * RN_LD, m);
            double *p = partials + ((size_t)(tb - t0 + lane) * C + chunk) * 3;
            p[0] = tr.n;
            p[1] = tr.mean;
            p[2] = tr.m2;
        }
        __syncthreads();
    }
    if (present) ret[i] = acc;
}

// `cnt` nodes of arr -> arr[0], level by level; cnt <= 2 * RN_BLOCK, uniform over the block
__device__ __forceinline__ void tree_levels(RrTriple *arr, int cnt) {
    const int tid = (int)threadIdx.x;
    while (cnt > 1) {
        const int half = (cnt + 1) >> 1;
        RrTriple v;
        if (tid < half) {
            v = arr[2 * tid];
            if (2 * tid + 1 < cnt) v = rr_merge(v, arr[2 * tid + 1]);
        }
        __syncthreads();
        if (tid < half) arr[tid] = v;
        __syncthreads();
        cnt = half;
    }
}

__global__ __launch_bounds__(RN_BLOCK) void tree_kernel(double *__restrict__ partials, int C) {
    __shared__ RrTriple tile[RN_TILE];
    __shared__ RrTriple top[RN_MAX_TILES];
    const int tid = (int)threadIdx.x;
    double *row = partials + (size_t)blockIdx.x * C * 3;
    const int ntiles = (C + RN_TILE - 1) / RN_TILE;
    for (int k = 0; k < ntiles; ++k) {
        const int cnt = C - k * RN_TILE < RN_TILE ? C - k * RN_TILE : RN_TILE;
        const double *src = row + (size_t)k * RN_TILE * 3;
        double *dst = reinterpret_cast<double *>(tile);
        for (int j = tid; j < cnt * 3; j += RN_BLOCK) dst[j] = src[j];
        __syncthreads();
        tree_levels(tile, cnt);
        if (tid == 0) top[k] = tile[0];
        __syncthreads();
    }
    tree_levels(top, ntiles);
    if (tid == 0) {                 // every read of the row is behind a barrier by now
        row[0] = top[0].n;
        row[1] = top[0].mean;
        row[2] = top[0].m2;
    }
}

__global__ __launch_bounds__(RR_CHUNK) void chain_kernel(double *__restrict__ partials, int C, int steps,
                                                         double *__restrict__ rms, double epsilon, int update,
                                                         double *__restrict__ scale_out) {
    __shared__ RrTriple batch[RN_CHAIN];
    __shared__ double var_t[RN_CHAIN];
    const int lane = (int)threadIdx.x;
    RrStats s = {rms[0], rms[1], rms[2]};
    if (!update) {                  // launched only with scale_out
        const double sc = rr_scale(s.var, epsilon);
        for (int t = lane; t < steps; t += RR_CHUNK) scale_out[t] = sc;
        return;
    }
    for (int tb = 0; tb < steps; tb += RN_CHAIN) {
        const int cnt = steps - tb < RN_CHAIN ? steps - tb : RN_CHAIN;
        for (int k = lane; k < cnt; k += RR_CHUNK) {
            const double *row = partials + (size_t)(tb + k) * C * 3;
            const RrTriple root = {row[0], row[1], row[2]};
            batch[k] = rr_batch(root);
        }
        __syncthreads();
        if (lane == 0) {
            for (int k = 0; k < cnt; ++k) {
                rr_absorb(s, batch[k]);
                var_t[k] = s.var;
            }
        }
        __syncthreads();
        for (int k = lane; k < cnt; k += RR_CHUNK) {
            const double sc = rr_scale(var_t[k], epsilon);
            partials[(size_t)(tb + k) * C * 3] = sc;
            if (scale_out != nullptr) scale_out[tb + k] = sc;
        }
        __syncthreads();
    }
    if (lane == 0) {
        rms[0] = s.mean;
        rms[1] = s.var;
        rms[2] = s.count;
    }
}

// scales: step t's at scales[t * stride]; NULL: the stored var's, for every step
__global__ __launch_bounds__(RN_BLOCK) void scale_kernel(float *__restrict__ rew, int t0, int N,
                                                         const double *__restrict__ scales, size_t stride,
                                                         const double *__restrict__ rms, double epsilon,
                                                         double clip) {
    const int i = (int)(blockIdx.x * RN_BLOCK + threadIdx.x);
    if (i >= N) return;
    const int t = (int)blockIdx.y;
    const double sc = scales != nullptr ? scales[(size_t)t * stride] : rr_scale(rms[1], epsilon);
    const size_t o = (size_t)(t0 + t) * N + i;
    rew[o] = rr_normalize(rew[o], sc, clip);
}

// the same on four agents a lane: N % 4 == 0 and a 16-byte aligned base
__global__ __launch_bounds__(RN_BLOCK) void scale4_kernel(float4 *__restrict__ rew, int t0, int N4,
                                                          const double *__restrict__ scales, size_t stride,
                                                          const double *__restrict__ rms, double epsilon,
                                                          double clip) {
    const int i = (int)(blockIdx.x * RN_BLOCK + threadIdx.x);
    if (i >= N4) return;
    const int t = (int)blockIdx.y;
    const double sc = scales != nullptr ? scales[(size_t)t * stride] : rr_scale(rms[1], epsilon);
    const size_t o = (size_t)(t0 + t) * N4 + i;
    float4 v = rew[o];
    v.x = rr_normalize(v.x, sc, clip);
    v.y = rr_normalize(v.y, sc, clip);
    v.z = rr_normalize(v.z, sc, clip);
    v.w = rr_normalize(v.w, sc, clip);
    rew[o] = v;
}

int launch_scale(float *rew, int t0, int steps, int N, const double *scales, size_t stride, const double *rms,
                 double epsilon, double clip, hipStream_t s) {
    if (N % 4 == 0 && reinterpret_cast<uintptr_t>(rew) % 16 == 0) {
        const int n4 = N / 4;
        hipLaunchKernelGGL(scale4_kernel, dim3((unsigned)((n4 + RN_BLOCK - 1) / RN_BLOCK), (unsigned)steps),
                           dim3(RN_BLOCK), 0, s, reinterpret_cast<float4 *>(rew), t0, n4, scales, stride, rms, epsilon,
                           clip);
    } else {
        hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((N + RN_BLOCK - 1) / RN_BLOCK), (unsigned)steps),
                           dim3(RN_BLOCK), 0, s, rew, t0, N, scales, stride, rms, epsilon, clip);
    }
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace

extern "C" {

int vn_return_moments(const float *rewards, const float *dones, int32_t t0, int32_t t1, int32_t N,
                      int64_t agent_id_base, double gamma, double *ret, double *partials, void *stream) {
    if (!rewards || !dones || !ret || !partials) return fail(VN_ERR_INVALID, "vn_return_moments: NULL argument");
    if (t0 < 0 || t1 <= t0)
        return fail(VN_ERR_INVALID, "vn_return_moments: steps [t0, t1) must be 0 <= t0 < t1 (got %d, %d)", t0, t1);
    if (N < 1) return fail(VN_ERR_INVALID, "vn_return_moments: N must be >= 1 (got %d)", N);
    if (agent_id_base < 0 || agent_id_base % RR_CHUNK != 0)
        return fail(VN_ERR_INVALID, "vn_return_moments: agent_id_base must be a non-negative multiple of 64 (got %lld): "
                                    "a wave reduces one global chunk of 64 agents", (long long)agent_id_base);
    hipLaunchKernelGGL(moments_kernel, dim3((unsigned)((N + RR_CHUNK - 1) / RR_CHUNK)), dim3(RR_CHUNK), 0,
                       (hipStream_t)stream, rewards, dones, (int)t0, (int)t1, (int)N, gamma, ret, partials);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int vn_reward_normalize(float *rewards, int32_t t0, int32_t t1, int32_t N, double *partials, int32_t C_global,
                        double *rms, double epsilon, double clip, int32_t update, double *scale_out, void *stream) {
    if (!rewards || !rms) return fail(VN_ERR_INVALID, "vn_reward_normalize: NULL argument");
    if (t0 < 0 || t1 <= t0)
        return fail(VN_ERR_INVALID, "vn_reward_normalize: steps [t0, t1) must be 0 <= t0 < t1 (got %d, %d)", t0, t1);
    const int steps = t1 - t0;
    if (steps > RN_MAX_STEPS)
        return fail(VN_ERR_INVALID, "vn_reward_normalize: at most %d steps per call (got %d)", RN_MAX_STEPS, steps);
    if (N < 1) return fail(VN_ERR_INVALID, "vn_reward_normalize: N must be >= 1 (got %d)", N);
    if (!(clip > 0.0) || !std::isfinite(clip))
        return fail(VN_ERR_INVALID, "vn_reward_normalize: clip must be positive and finite (got %g)", clip);
    if (!(epsilon >= 0.0)) return fail(VN_ERR_INVALID, "vn_reward_normalize: epsilon must be >= 0 (got %g)", epsilon);
    hipStream_t s = (hipStream_t)stream;
    if (update) {
        if (!partials) return fail(VN_ERR_INVALID, "vn_reward_normalize: NULL partials with update");
        const int c_own = (N + RR_CHUNK - 1) / RR_CHUNK;
        if (C_global < c_own || C_global > RN_TILE * RN_MAX_TILES)
            return fail(VN_ERR_INVALID, "vn_reward_normalize: C_global %d is not in %d (the chunks of this shard's %d "
                                        "agents) .. %d", C_global, c_own, N, RN_TILE * RN_MAX_TILES);
        hipLaunchKernelGGL(tree_kernel, dim3((unsigned)steps), dim3(RN_BLOCK), 0, s, partials, (int)C_global);
        VN_HIP(hipGetLastError());
        hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(RR_CHUNK), 0, s, partials, (int)C_global, steps, rms, epsilon, 1,
                           scale_out);
        VN_HIP(hipGetLastError());
        return launch_scale(rewards, t0, steps, N, partials, (size_t)C_global * 3, rms, epsilon, clip, s);
    }
    if (scale_out) {
        hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(RR_CHUNK), 0, s, (double *)nullptr, 0, steps, rms, epsilon, 0,
                           scale_out);
        VN_HIP(hipGetLastError());
    }
    return launch_scale(rewards, t0, steps, N, nullptr, 0, rms, epsilon, clip, s);
}

}  // extern "C"
