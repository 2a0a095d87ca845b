// voxnav_episode.hip -- the episode records' kernel unit (vn_episode,
// env_params.h): what vn_episode_records / vn_episode_totals /
// vn_episode_clear launch on the buffer the step kernels update at every
// episode end (episode_end, env_core.h; EpisodeRec, env_plan.h).  These are
// the numbers the reference prints at each episode end
// (envs/CubicEnv.py:212-222) and tabulates in train/evaluate_grid.py:213-247.
// Not a hot path: one call per rollout or per finished step.  The step
// kernels are not instantiated here.

#include "vn_common.h"
#include "env_params.h"
#include "env_plan.h"

namespace {

constexpr int EP_BLOCK = 256;
constexpr int EP_MAX_BLOCKS = 1024;     // vn_episode_totals: grid-stride above EP_BLOCK * EP_MAX_BLOCKS agents
constexpr int EP_TOTALS = 6;            // episodes, finished and the four sums

// one agent's row as int64 [VN_EPISODE_FIELDS], in the header's field order
__global__ __launch_bounds__(EP_BLOCK) void episode_records_kernel(const EpisodeRec *__restrict__ rec, int N,
                                                                   int64_t *__restrict__ out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= N) return;
    const EpisodeRec r = rec[i];
    int64_t *o = out + (size_t)i * VN_EPISODE_FIELDS;
    o[0] = r.episodes;
    o[1] = r.finished;
    o[2] = (int64_t)r.sum_steps;
    o[3] = (int64_t)r.sum_bumps;
    o[4] = (int64_t)r.sum_visited;
    o[5] = (int64_t)r.sum_max_steps;
    o[6] = r.last_steps;
    o[7] = r.last_bumps;
    o[8] = r.last_visited;
    o[9] = r.last_max_steps;
    o[10] = r.last_room;
    o[11] = r.last_flags;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;       // lane 0 holds the wave's sum
}

// The six totals over all agents: each thread sums its agents (grid stride),
// each wave reduces by shuffles, the block's four waves through LDS, and one
// lane per block adds the block's sums to out[6] (zeroed on the stream before
// the launch) with 64-bit integer atomics.  Integer sums: exact, whatever the
// order.  Threads past N contribute zeros and take part in every shuffle and
// barrier, so any N is right (N < 64, N not a multiple of the block).
__global__ __launch_bounds__(EP_BLOCK) void episode_totals_kernel(const EpisodeRec *__restrict__ rec, int N,
                                                                  unsigned long long *__restrict__ out) {
    unsigned long long acc[EP_TOTALS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (size_t i = (size_t)blockIdx.x * EP_BLOCK + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * EP_BLOCK) {
        const EpisodeRec *r = rec + i;      // the totals are the row's first 40 bytes
        acc[0] += r->episodes;
        acc[1] += r->finished;
        acc[2] += r->sum_steps;
        acc[3] += r->sum_bumps;
        acc[4] += r->sum_visited;
        acc[5] += r->sum_max_steps;
    }
    __shared__ unsigned long long part[EP_BLOCK / 64][EP_TOTALS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int f = 0; f < EP_TOTALS; ++f) {
        const unsigned long long w = wave_sum(acc[f]);
        if (lane == 0) part[wave][f] = w;
    }
    __syncthreads();
    if (threadIdx.x < EP_TOTALS) {
        unsigned long long b = 0ull;
#pragma unroll
        for (int w = 0; w < EP_BLOCK / 64; ++w) b += part[w][threadIdx.x];
        if (b) atomicAdd(out + threadIdx.x, b);
    }
}

// zero the rows of the agents with mask[i] != 0 (NULL: all); 4 threads per row, 16 B each
__global__ __launch_bounds__(EP_BLOCK) void episode_clear_kernel(uint4 *__restrict__ rec, int N,
                                                                 const uint8_t *__restrict__ mask) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = c >> 2;
    if (i >= (size_t)N || (mask != nullptr && mask[i] == 0)) return;
    rec[c] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

namespace vn_episode {

int records(const void *episodes, int N, int64_t *out, hipStream_t s) {
    hipLaunchKernelGGL(episode_records_kernel, dim3((unsigned)((N + EP_BLOCK - 1) / EP_BLOCK)), dim3(EP_BLOCK), 0, s,
                       static_cast<const EpisodeRec *>(episodes), N, out);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int totals(const void *episodes, int N, int64_t *out, hipStream_t s) {
    VN_HIP(hipMemsetAsync(out, 0, EP_TOTALS * sizeof(int64_t), s));
    int blocks = (N + EP_BLOCK - 1) / EP_BLOCK;
    if (blocks > EP_MAX_BLOCKS) blocks = EP_MAX_BLOCKS;
    hipLaunchKernelGGL(episode_totals_kernel, dim3((unsigned)blocks), dim3(EP_BLOCK), 0, s,
                       static_cast<const EpisodeRec *>(episodes), N, reinterpret_cast<unsigned long long *>(out));
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int clear(void *episodes, int N, const uint8_t *mask, hipStream_t s) {
    const size_t chunks = (size_t)N * (sizeof(EpisodeRec) / sizeof(uint4));
    hipLaunchKernelGGL(episode_clear_kernel, dim3((unsigned)((chunks + EP_BLOCK - 1) / EP_BLOCK)), dim3(EP_BLOCK), 0, s,
                       static_cast<uint4 *>(episodes), N, mask);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace vn_episode
