// voxnav_state.hip -- vn_import_state's kernel unit: the CubicEnv agents'
// memory state rebuilt from exported state rows and dense belief maps, in
// whatever belief layout the env was planned with.  The encoder itself is
// csrc/env_state.h (shared with the host driver of the CPU tests); this file
// is its device launch: one wave per agent, validation first, then the
// agent's own block of every per-agent buffer.  Not a hot path: bounded
// loops, plain vector stores, no wait between waves.  The step kernels
// (voxnav_env.hip) are not touched and not instantiated here.

#include "env_core.h"
#include "env_state.h"

namespace {

constexpr int IMPORT_BLOCK = 64;

// One block (one wave) per agent.  Phase 1 validates the state row and the
// map and ends in a block-wide vote: a rejected agent is counted and nothing
// of it is written.  Every address is formed only from values the checks
// before it accepted (room -> room descriptor -> position -> ray records and
// map cells).  Phase 2 writes the agent's map, planes, stood rows and masks,
// hot state, next seed and obs row.
__global__ __launch_bounds__(IMPORT_BLOCK) void import_state_kernel(Params p, const int64_t *__restrict__ state,
                                                                     const int8_t *__restrict__ belief,
                                                                     const uint8_t *__restrict__ mask, float *obs,
                                                                     int32_t *n_rejected, int pw, int pd) {
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (i >= p.N || (mask != nullptr && mask[i] == 0)) return;      // block-uniform
    __shared__ uint32_t nz[2];
    if (tid == 0) nz[0] = nz[1] = 0u;

    int64_t s[VN_STATE_FIELDS];
    for (int f = 0; f < VN_STATE_FIELDS; ++f) s[f] = state[(size_t)i * VN_STATE_FIELDS + f];
    bool ok = vs_scalars_ok(s, p.n_rooms, p.L);
    Room R{};
    if (ok) {
        R = load_room(p, (int)s[VS_ROOM]);
        ok = vs_pos_ok(s, R.W, R.D, R.H);
    }
    VsAgent a{};
    if (ok) {
        a.x = (int)s[VS_X];
        a.y = (int)s[VS_Y];
        a.z = (int)s[VS_Z];
        a.W = R.W;
        a.D = R.D;
        a.H = R.H;
        a.rays = reinterpret_cast<const uint32_t *>(p.rays + R.ray_off);
        a.dense = belief + (size_t)i * pw * pd * p.ph;
        a.pd = pd;
        a.ph = p.ph;
        a.latent = p.pcache != 0;
        const uint2 rec = p.rays[R.ray_off + (uint32_t)((a.x * R.D + a.y) * R.H + a.z)];
        a.here = vs_rays(rec.x, rec.y, p.L);
        ok = !a.here.wall;
    }
    if (ok) ok = vs_cells_ok(a, tid, IMPORT_BLOCK);
    if (__syncthreads_or(ok ? 0 : 1)) {       // also orders nz's zeroing before the atomics below
        if (tid == 0 && n_rejected != nullptr) atomicAdd(n_rejected, 1);
        return;
    }

    // ---- the agent's memory ----
    const VsLayout l{pw, pd, p.ph, p.nby, p.pcache, p.nwx, p.nwy, p.xp_off, p.yp_off};
    int8_t *map = p.belief + (size_t)i * p.agent_bytes;
    vs_write_map(a, l, map, tid, IMPORT_BLOCK);
    uint32_t xnz = 0u, ynz = 0u;
    vs_write_planes(a, l, map, tid, IMPORT_BLOCK, &xnz, &ynz);
    if (p.stood != nullptr) {                 // plane-set mode 2: stood rows and nonzero-set masks
        if (xnz) atomicOr(&nz[0], xnz);
        if (ynz) atomicOr(&nz[1], ynz);
        if (tid < 32) p.stood[(size_t)i * 32u + (uint32_t)tid] = vs_stood_row(a, tid);
        __syncthreads();
        if (tid == 0) p.pnz[i] = make_uint2(nz[0], nz[1]);
    }

    // ---- hot state (window-record bit clear: pack leaves bit 30 clear) and next seed ----
    Agent g;
    g.x = a.x;
    g.y = a.y;
    g.z = a.z;
    g.facing = (int)s[VS_FACING];
    g.last_action = (int)s[VS_LAST_ACTION];
    g.done = s[VS_DONE] != 0;
    g.last_bump = s[VS_LAST_BUMP] != 0;
    g.near_wall = s[VS_NEAR_WALL] != 0 || a.here.near;
    g.was_near_wall = s[VS_WAS_NEAR_WALL] != 0;
    g.step_count = (uint32_t)vs_clamp_steps(s[VS_STEP_COUNT]);
    g.visited = (uint32_t)s[VS_VISITED];
    g.bumps = (uint32_t)vs_clamp_bumps(s[VS_BUMPS]);
    g.move_mask = a.here.move_mask;
    g.cid = a.here.nf[5];
    g.room = (int)s[VS_ROOM];
    if (tid == 0) {
        p.hot[i] = pack(g);
        p.next_seed[i] = (uint32_t)s[VS_NEXT_SEED];
    }

    // ---- get_obs (:269-311): the window through the LUT, then the tail ----
    if (obs != nullptr) {
        float *row = obs + (size_t)i * VN_OBS_DIM;
        row[tid] = p.lut[vs_window_byte(a, tid)];      // (a latent wall's entry is the unknown cell's)
        if (tid < VN_OBS_DIM - 64) {
            float v = 0.0f;
            if (tid < 4) v = g.facing == tid ? 1.0f : 0.0f;                                     // (:279-280)
            else if (tid == 4) v = p.lut[TAB_ACTION + g.last_action];                           // (:284)
            else if (tid == 5) v = g.was_near_wall ? 1.0f : 0.0f;
            else if (tid == 6) v = g.last_bump ? 1.0f : 0.0f;
            else if (tid == 7) v = p.lut[TAB_CID + g.cid];                                      // (:287)
            else if (tid == 8) v = (float)((double)g.visited / (double)R.total_free);           // (:291)
            row[64 + tid] = v;
        }
    }
}

}  // namespace

namespace vn_state {

int import_state(const void *params, const int64_t *state, const int8_t *belief, const uint8_t *mask, float *obs,
                 int32_t *n_rejected, int pw, int pd, hipStream_t s) {
    const Params &p = *static_cast<const Params *>(params);
    if (n_rejected != nullptr) VN_HIP(hipMemsetAsync(n_rejected, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(import_state_kernel, dim3((unsigned)p.N), dim3(IMPORT_BLOCK), 0, s, p, state, belief, mask, obs,
                       n_rejected, pw, pd);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace vn_state
