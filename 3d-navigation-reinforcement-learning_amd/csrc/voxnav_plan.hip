// voxnav_plan.hip -- vn_plan_frontier's kernel unit: for every CubicEnv agent
// the first action of a shortest known-free path to the nearest cell it knows
// to be free and has not visited, and vn_plan_frontier_dists'
// kernel: that path's length for each of the six first actions and the set of
// the shortest.  The rule itself is
// csrc/env_route.h (shared with the host driver of the CPU tests); this file
// reads the agent's layout-native memory -- the bricked byte map and both
// marked-bit planes, in every belief layout, with export_belief_kernel's rule
// (vs_decode, env_state.h) -- turns it into bit rows over x by wave ballots
// and runs the search in LDS.  Read-only on the env: nothing of it is written,
// the step kernels (voxnav_env.hip) are not touched and not instantiated here.
//
// One wave per agent and one wave per block: the flood's trip count differs
// between agents by orders of magnitude, and with a single wave the barrier
// inside that loop is wave-local and its trip count block-uniform by
// construction.

#include "env_core.h"
#include "env_state.h"
#include "env_route.h"

namespace {

constexpr int PLAN_BLOCK = 64;
static_assert(PLAN_BLOCK == RT_MAX_W, "lane x of the wave holds column x of a row");

// the block's barrier and OR vote for rt_search (one wave: wave-local)
struct WaveBlk {
    __device__ void sync() const { __syncthreads(); }
    __device__ bool any(bool v) const { return __syncthreads_or(v ? 1 : 0) != 0; }
};

// one agent's belief block in the env's layout (rooms of at most 64 x 64: one word per plane row)
struct PlanMem {
    const int8_t *map;
    int ph, nby, pcache;
    uint32_t xp_off, yp_off;
};

__device__ __forceinline__ uint64_t plane_row(const PlanMem &m, uint32_t off, int r, int z) {
    const size_t ix = (size_t)(r * m.ph + z);
    return m.pcache == 2 ? (uint64_t)reinterpret_cast<const uint32_t *>(m.map + off)[ix]      // u32 rows
                         : reinterpret_cast<const uint64_t *>(m.map + off)[ix];
}
// x-plane row (y, z) holds bit x, y-plane row (x, z) bit y, of cells known through a ray mark
__device__ __forceinline__ uint64_t xplane_row(const PlanMem &m, int y, int z) { return plane_row(m, m.xp_off, y, z); }
__device__ __forceinline__ uint64_t yplane_row(const PlanMem &m, int x, int z) { return plane_row(m, m.yp_off, x, z); }

// the belief value of one cell of the room (export_belief_kernel's rule)
__device__ __forceinline__ int cell_value(const PlanMem &m, int x, int y, int z) {
    const uint32_t b = (uint8_t)m.map[(size_t)bcol(x, y, m.nby) * (size_t)m.ph + (size_t)z];
    const bool in_plane = (((xplane_row(m, y, z) >> x) | (yplane_row(m, x, z) >> y)) & 1ull) != 0ull;
    return vs_decode(b, in_plane);
}

__device__ __forceinline__ void plan_store(int32_t *actions, int32_t *dist, int i, int tid, int a, int d) {
    if (tid == 0) {
        actions[i] = a;
        if (dist != nullptr) dist[i] = d;
    }
}

// Lane k < 6 decodes n_k, the cell action k moves to: its belief value, -3 outside the room; the
// value goes to nv[k] and comes back (-3 on the other lanes).
__device__ __forceinline__ int plan_neighbour_values(const PlanMem &m, const RtGeom &g, const Agent &a, int tid,
                                                     int *nv) {
    int v = -3;                                   // outside the room
    if (tid < RT_ACTIONS) {
        int dx, dy, dz;
        rt_move(tid, a.facing, &dx, &dy, &dz);
        const int nx = a.x + dx, ny = a.y + dy, nz = a.z + dz;
        if (rt_inside(g, nx, ny, nz)) v = cell_value(m, nx, ny, nz);
        nv[tid] = v;
    }
    return v;
}

// The rows: a transposition by ballot.  Lane x holds column (x, y) -- 8 cells of it, one 8-byte
// load -- and its y-plane rows (x, z); the x-plane row (y, z) is already the word.  Writes the
// passable rows and the targets (R_0) of the agent's room, row (y, z) at y * ph + z.
__device__ __forceinline__ void plan_build_rows(const PlanMem &m, const Room &R, int ph, int tid, uint64_t *pass,
                                                uint64_t *ra) {
    const uint64_t wmask = rt_width_mask(R.W);
    const bool lane_in = tid < R.W;
    for (int z0 = 0; z0 < R.H; z0 += 8) {
        uint64_t yr[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) yr[k] = (lane_in && z0 + k < R.H) ? yplane_row(m, tid, z0 + k) : 0ull;
        for (int y = 0; y < R.D; ++y) {
            uint64_t col = 0ull;
            if (lane_in)
                col = *reinterpret_cast<const uint64_t *>(m.map + (size_t)bcol(tid, y, m.nby) * (size_t)m.ph + (size_t)z0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int z = z0 + k;
                if (z < R.H) {                    // wave-uniform
                    const uint32_t b = (uint32_t)(col >> (8 * k)) & 0xffu;
                    const uint64_t known = __ballot((b & VS_KNOWN) != 0u) | xplane_row(m, y, z) |
                                           __ballot(((yr[k] >> y) & 1ull) != 0ull);
                    const uint64_t wall = __ballot((b & VS_LATENT) != 0u);
                    const uint64_t fresh = __ballot((b & 0x3fu) == 0u);
                    const uint64_t ps = known & ~wall & wmask;
                    if (tid == k) {
                        pass[y * ph + z] = ps;
                        ra[y * ph + z] = ps & fresh;
                    }
                }
            }
        }
    }
}

// Dynamic LDS (all of the kernel's own LDS, so that its base stays 16-byte aligned): three row
// sets of pd * ph words -- pass, and the flood's two buffers -- then the six neighbours' values.
__global__ __launch_bounds__(PLAN_BLOCK) void plan_frontier_kernel(Params p, const uint8_t *__restrict__ mask,
                                                                    int32_t *__restrict__ actions,
                                                                    int32_t *__restrict__ dist, int pw, int pd) {
    extern __shared__ __attribute__((aligned(16))) uint64_t plan_rows[];
    const int rows = pd * p.ph;
    uint64_t *pass = plan_rows, *ra = plan_rows + rows, *rb = plan_rows + 2 * rows;
    int *nv = reinterpret_cast<int *>(plan_rows + 3 * rows);
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (i >= p.N || (mask != nullptr && mask[i] == 0)) return;      // block-uniform, as every exit below

    const Agent a = unpack(p.hot[i]);
    if (a.room >= p.n_rooms) return plan_store(actions, dist, i, tid, 0, -1);       // (no agent of a reset env)
    const Room R = load_room(p, a.room);
    const RtGeom g{R.W, R.D, R.H, p.ph};
    if (R.W > pw || R.D > pd || R.H > p.ph || !rt_inside(g, a.x, a.y, a.z))
        return plan_store(actions, dist, i, tid, 0, -1);
    const PlanMem m{p.belief + (size_t)i * p.agent_bytes, p.ph, p.nby, p.pcache, p.xp_off, p.yp_off};

    // ---- the six neighbour cells first: lane k decodes n_k.  Almost every call of a closed loop
    // ends here (a neighbour that is itself a target: dist 1), before any row is built.
    const int v = plan_neighbour_values(m, g, a, tid, nv);
    const uint64_t near = __ballot(tid < RT_ACTIONS && v == 0);
    if (near) return plan_store(actions, dist, i, tid, rt_lowest((uint32_t)near), 1);
    if (!__ballot(tid < RT_ACTIONS && v >= 0))    // no passable neighbour: no flood can reach one
        return plan_store(actions, dist, i, tid, 0, -1);

    plan_build_rows(m, R, p.ph, tid, pass, ra);

    // ---- the flood (env_route.h)
    int act = 0, d = -1;
    rt_search(WaveBlk{}, pass, ra, rb, g, a.x, a.y, a.z, a.facing, nv, pw * pd * p.ph, tid, PLAN_BLOCK, &act, &d);
    plan_store(actions, dist, i, tid, act, d);
}

// vn_plan_frontier_dists' stores: lane k < 6 holds dists[k] in dk; lane 0 writes the rest
__device__ __forceinline__ void dists_store(int32_t *actions, int32_t *dist, int32_t *dists, uint8_t *best, int i,
                                            int tid, int dk, int a, int d, uint32_t b) {
    if (tid < RT_ACTIONS) dists[(size_t)i * RT_ACTIONS + tid] = dk;
    if (tid == 0) {
        if (actions != nullptr) actions[i] = a;
        if (dist != nullptr) dist[i] = d;
        if (best != nullptr) best[i] = (uint8_t)b;
    }
}

// The per-action distances (the rule: include/voxnav.h, vn_plan_frontier_dists).  The LDS plan,
// the neighbour test and the rows are plan_frontier_kernel's; the search is rt_search_all.
//
// The neighbour test answers here as well.  When some n_k is a target and the agent's own cell is
// passable, every passable n_k is in R_2 (n_k, the agent's cell, the target neighbour), so its j
// is 0 (a target itself), 1 (one of its own six-neighbours is a target: R_1 is the targets and
// their passable neighbours) or 2 otherwise: lane 6 k + m decodes the cell n_k + e_m, 36 lanes,
// and no row is built.  With the agent's cell not passable (no state an env reaches, and
// vn_import_state refuses one) that path through it does not exist and the flood decides.
__global__ __launch_bounds__(PLAN_BLOCK) void plan_frontier_dists_kernel(Params p, const uint8_t *__restrict__ mask,
                                                                          int32_t *__restrict__ actions,
                                                                          int32_t *__restrict__ dist,
                                                                          int32_t *__restrict__ dists,
                                                                          uint8_t *__restrict__ best, int pw, int pd) {
    extern __shared__ __attribute__((aligned(16))) uint64_t plan_rows[];
    const int rows = pd * p.ph;
    uint64_t *pass = plan_rows, *ra = plan_rows + rows, *rb = plan_rows + 2 * rows;
    int *nv = reinterpret_cast<int *>(plan_rows + 3 * rows);
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (i >= p.N || (mask != nullptr && mask[i] == 0)) return;      // block-uniform, as every exit below

    const Agent a = unpack(p.hot[i]);
    if (a.room >= p.n_rooms) return dists_store(actions, dist, dists, best, i, tid, RT_BLOCKED, 0, -1, 0u);
    const Room R = load_room(p, a.room);
    const RtGeom g{R.W, R.D, R.H, p.ph};
    if (R.W > pw || R.D > pd || R.H > p.ph || !rt_inside(g, a.x, a.y, a.z))
        return dists_store(actions, dist, dists, best, i, tid, RT_BLOCKED, 0, -1, 0u);
    const PlanMem m{p.belief + (size_t)i * p.agent_bytes, p.ph, p.nby, p.pcache, p.xp_off, p.yp_off};

    const int v = plan_neighbour_values(m, g, a, tid, nv);
    const uint32_t near = (uint32_t)__ballot(tid < RT_ACTIONS && v == 0);
    const uint32_t open = (uint32_t)__ballot(tid < RT_ACTIONS && v >= 0);
    if (!open)                                    // no passable neighbour: every entry -2, action 0
        return dists_store(actions, dist, dists, best, i, tid, RT_BLOCKED, 0, -1, 0u);

    if (near) {
        // lane 6 k + m: is n_k + e_m a target?  lane 36: is the agent's own cell passable?
        bool tgt = false, own = false;
        if (tid < RT_ACTIONS * RT_ACTIONS) {
            const int k = tid / RT_ACTIONS, e = tid - k * RT_ACTIONS;
            int dx, dy, dz, ex, ey, ez;
            rt_move(k, a.facing, &dx, &dy, &dz);
            rt_move(e, 0, &ex, &ey, &ez);
            const int cx = a.x + dx + ex, cy = a.y + dy + ey, cz = a.z + dz + ez;
            // n_k outside the room: its entry is -2 whatever this lane finds
            if (rt_inside(g, cx, cy, cz)) tgt = cell_value(m, cx, cy, cz) == 0;
        } else if (tid == RT_ACTIONS * RT_ACTIONS) {
            own = cell_value(m, a.x, a.y, a.z) >= 0;
        }
        const uint64_t tb = __ballot(tgt);
        if (__ballot(own)) {
            int dk = RT_BLOCKED;
            if (tid < RT_ACTIONS) {
                const bool two = ((tb >> (RT_ACTIONS * tid)) & 0x3full) != 0ull;
                dk = v == 0 ? 1 : v > 0 ? (two ? 2 : 3) : RT_BLOCKED;
            }
            return dists_store(actions, dist, dists, best, i, tid, dk, rt_lowest(near), 1, near);
        }
    }

    plan_build_rows(m, R, p.ph, tid, pass, ra);

    int ds[RT_ACTIONS];
    rt_search_all(WaveBlk{}, pass, ra, rb, g, a.x, a.y, a.z, a.facing, nv, pw * pd * p.ph, tid, PLAN_BLOCK, ds);
    const uint32_t b = rt_best_set(ds);
    int dk = RT_BLOCKED;
#pragma unroll
    for (int k = 0; k < RT_ACTIONS; ++k) dk = tid == k ? ds[k] : dk;
    dists_store(actions, dist, dists, best, i, tid, dk, b ? rt_lowest(b) : rt_fallback(nv), rt_min_dist(ds), b);
}

}  // namespace

namespace vn_plan {

int frontier(const void *params, const uint8_t *mask, int32_t *actions, int32_t *dist, int pw, int pd, hipStream_t s) {
    const Params &p = *static_cast<const Params *>(params);
    // three row sets (<= 48 KiB at 64 x 64 x 32) and the neighbours' values
    const size_t lds = (size_t)3 * (size_t)pd * (size_t)p.ph * sizeof(uint64_t) + 8 * sizeof(int);
    hipLaunchKernelGGL(plan_frontier_kernel, dim3((unsigned)p.N), dim3(PLAN_BLOCK), lds, s, p, mask, actions, dist, pw,
                       pd);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int frontier_dists(const void *params, const uint8_t *mask, int32_t *actions, int32_t *dist, int32_t *dists,
                   uint8_t *best, int pw, int pd, hipStream_t s) {
    const Params &p = *static_cast<const Params *>(params);
    const size_t lds = (size_t)3 * (size_t)pd * (size_t)p.ph * sizeof(uint64_t) + 8 * sizeof(int);   // as frontier
    hipLaunchKernelGGL(plan_frontier_dists_kernel, dim3((unsigned)p.N), dim3(PLAN_BLOCK), lds, s, p, mask, actions,
                       dist, dists, best, pw, pd);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace vn_plan
