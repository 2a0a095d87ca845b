// voxnav_simple.hip -- MI355X (gfx950) kernels of the simpleEnv variant
// (envs/simpleEnv.py).  Split from voxnav_env.hip:
// the CubicEnv step kernel stays there (the C-ABI: voxnav_api.hip); this unit holds the
// simpleEnv step kernels (line layout for rooms <= 32 x 32 x 8, word layout
// up to 64 x 64 x 31, dense maps beyond), their reset kernel and belief
// export, and the launcher voxnav_api.hip's launch_env calls (vn_simple).
// Three headers that only this unit includes hold what the kernels are built
// from: simple_draw.h (an episode's MT19937 draws), simple_bits.h (ray
// directions, the bit-plane belief and its observes), simple_line.h (the line
// layout's lane-pair loads and stores).  Here: the step pieces the kernels
// share, the kernels, and pick(), the one place that maps a call shape to a
// kernel for launch and label.

#include "env_core.h"

#include "simple_draw.h"
#include "simple_bits.h"
#include "simple_line.h"

namespace {

// ============================================================================
// Step pieces shared by the simpleEnv kernels (dense, word and line layout).
// ============================================================================

// an agent at the start of the episode drawn = (start | room << 24, goal)
__device__ __forceinline__ void reset_agent(const Params &p, uint2 drawn, Agent &g, uint32_t &goal, Room &R) {
    g.room = (int)(drawn.x >> 24);
    R = load_room(p, g.room);
    g.x = drawn.x & 0xff;
    g.y = (drawn.x >> 8) & 0xff;
    g.z = (drawn.x >> 16) & 0xff;
    goal = drawn.y;
    g.facing = 0;
    g.last_action = 0;
    g.done = g.last_bump = g.near_wall = g.was_near_wall = false;
    g.step_count = 0;
    g.visited = 1;
    g.bumps = 0;
    g.cid = 0;
    g.move_mask = 0;
}

// the wave zeroes the belief blocks of the agents in `m` (bits: lanes of the
// block that starts at agent block_agent0): all of the block for those in
// `mq`, up to QZ (its last part) for the others
__device__ __forceinline__ void zero_agent_blocks(const Params &p, uint64_t m, uint64_t mq, int block_agent0, int lane) {
    while (m) {
        const int src = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const uint32_t n16 = (((mq >> src) & 1ull) ? p.agent_bytes : p.qz_off) >> 4;
        uint4 *base = reinterpret_cast<uint4 *>(p.belief + (size_t)(block_agent0 + src) * p.agent_bytes);
        for (uint32_t q = (uint32_t)lane; q < n16; q += 64u) base[q] = make_uint4(0u, 0u, 0u, 0u);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// an agent's state into registers (lanes past N: zeros) and back
__device__ __forceinline__ void load_agent(const Params &p, int ai, bool live, Agent &g, uint32_t &goal,
                                           uint32_t &next_seed, Room &R) {
    g = unpack(live ? p.hot[ai] : make_uint4(0u, 0u, 0u, 0u));
    goal = live ? p.goal[ai] : 0u;
    next_seed = live ? p.next_seed[ai] : 0u;
    R = load_room(p, g.room);
}
__device__ __forceinline__ void store_agent(const Params &p, int ai, const Agent &g, uint32_t goal, uint32_t next_seed) {
    p.hot[ai] = pack(g);
    p.goal[ai] = goal;
    p.next_seed[ai] = next_seed;
}

// ============================================================================
// simpleEnv variant (envs/simpleEnv.py): walls are
// the room file's `2` tokens, the belief map holds the reference's
// internal_grid values as int8 (-1 unknown, 0 free, 1 visited, 2 wall),
// dense per agent [pd-major: x][y][z] with z contiguous (PH bytes).  The
// observation is 6 rays x L belief values + 6 distances + last_action
// (obs_dim = 6L + 7).  One lane per agent, 64 agents per block; obs rows are
// staged in LDS and written as one contiguous span per block.
// ============================================================================

// _sense_direction (:301-337) along absolute direction d from the agent's
// cell, using the cell's ray record (free run n to the first wall / edge).
// Writes L obs values, returns the distance count * 0.25.
__device__ __forceinline__ float simple_ray(int8_t *map, const Params &p, int cell, uint2 rec, int d, float *out) {
    const uint32_t e8 = ((d < 4 ? rec.x : rec.y) >> (8 * (d & 3))) & 0xffu;
    const int n = (int)(e8 & 0x7fu);
    const bool at_wall = (e8 & 0x80u) != 0u;
    const int L = p.L;
    const int sx = p.pd * p.ph, sy = p.ph;
    const int stride = d == 0 ? sx : d == 1 ? -sx : d == 2 ? sy : d == 3 ? -sy : d == 4 ? 1 : -1;
    const int m = n < L ? n : L;
    int c = cell;
    for (int s = 0; s < m; ++s) {
        c += stride;
        int v = map[c];
        if (v == -1) {           // unknown -> known free (:328-329)
            map[c] = 0;
            v = 0;
        }
        out[s] = (float)v;
    }
    if (n < L) {
        if (at_wall) map[c + stride] = 2;   // first wall (:321-324)
        else if (n >= 1) map[c] = 2;        // edge: the last in-room cell becomes a wall (:311-319)
        out[n] = 2.0f;
        for (int s = n + 1; s < L; ++s) out[s] = -1.0f;
    }
    return (float)((double)m * 0.25);       // round(count * cell_size, 2) (:337)
}

__device__ __forceinline__ void simple_observe(int8_t *map, const Params &p, const Agent &g, const Room &R,
                                               float *row) {
    const uint2 rec = p.rays[R.ray_off + (uint32_t)((g.x * R.D + g.y) * R.H + g.z)];
    const int cell = (g.x * p.pd + g.y) * p.ph + g.z;
    const int L = p.L;
    const int dirs[6] = {rel_dir(0, g.facing), rel_dir(3, g.facing), rel_dir(1, g.facing),
                         rel_dir(2, g.facing), 4, 5};   // forward, left, right, backward, up, down (:233)
#pragma unroll
    for (int k = 0; k < 6; ++k) row[6 * L + k] = simple_ray(map, p, cell, rec, dirs[k], row + k * L);
    row[6 * L + 6] = (float)g.last_action;
}

// reset for the lanes with `need`: draws, the wave clears every resetting
// agent's map rows x < W (all 64 lanes per agent, 8-byte stores), then each
// agent marks its start cell visited and senses (reset + get_obs(), as the
// reference's callers do, train/evaluate_grid.py:54-55).
__device__ void simple_reset_wave(const Params &p, int8_t *map, bool need, uint32_t seed, Agent &g,
                                  uint32_t &goal, Room &R, float *row, int lane, int block_agent0) {
    uint2 drawn = make_uint2(0u, 0u);
    if (need) drawn = simple_draw(p.envc, seed);
    uint64_t m = __ballot(need);
    while (m) {
        const int src = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const int room = __shfl((int)(drawn.x >> 24), src);
        const Room Rr = load_room(p, room);
        uint64_t *base = reinterpret_cast<uint64_t *>(p.belief + (size_t)(block_agent0 + src) * p.agent_bytes);
        const uint32_t words = (uint32_t)(Rr.W * p.pd * p.ph) >> 3;
        for (uint32_t w = (uint32_t)lane; w < words; w += 64u) base[w] = ~0ull;   // -1 = unknown (:85)
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (need) {
        reset_agent(p, drawn, g, goal, R);
        map[(g.x * p.pd + g.y) * p.ph + g.z] = 1;                              // :86
        simple_observe(map, p, g, R, row);
    }
}

template <bool RESET_ONLY>
__global__ __launch_bounds__(64) void simple_kernel(Params p) {
    extern __shared__ float sstage[];   // [64][obs_dim]
    const int lane = threadIdx.x;
    const int a0 = blockIdx.x * 64;
    const int ai = a0 + lane;
    const bool live = ai < p.N;
    const int OD = p.obs_dim;
    const int rows = min(64, p.N - a0);
    float *row = sstage + lane * OD;
    int8_t *map = p.belief + (size_t)(live ? ai : a0) * p.agent_bytes;
    Agent g;
    uint32_t goal, next_seed;
    Room R;
    load_agent(p, ai, live, g, goal, next_seed, R);

    if (RESET_ONLY) {
        const bool need = live && (!p.mask || p.mask[ai]);
        const uint32_t seed = need ? (uint32_t)p.seeds[ai] : 0u;
        simple_reset_wave(p, map, need, seed, g, goal, R, row, lane, a0);
        if (need) {
            float *o = p.obs + (size_t)ai * OD;
            for (int k = 0; k < OD; ++k) o[k] = row[k];
            p.hot[ai] = pack(g);
            p.goal[ai] = goal;
            p.next_seed[ai] = seed + p.seed_stride;   // modulo 2^32
        }
        return;
    }

    for (int k = 0; k < p.K; ++k) {
        const uint64_t t = p.t0 + (uint64_t)k;
        int a = 0;
        if (live) {
            if (p.actions) {
                a = p.actions[(size_t)k * p.N + ai];
            } else {
                const uint4 w = philox4x32_10(p.policy_seed, p.gid_base + (uint64_t)ai, t >> 2);
                const uint32_t word = (t & 3) == 0 ? w.x : (t & 3) == 1 ? w.y : (t & 3) == 2 ? w.z : w.w;
                a = (int)(((uint64_t)word * 6u) >> 32);
            }
            if (p.actions_out) p.actions_out[(size_t)k * p.N + ai] = a;
        }
        bool trunc = false, term = false, was_done = false;   // was_done: `done` entering the step
        double r = 0.0;
        if (live) {
            // step (:109-150)
            g.step_count += 1;
            trunc = g.step_count >= R.total_free;                      // :111, max_steps = total_free (:409)
            const int d = a < 4 ? rel_dir(a, g.facing) : (a == 4 ? 4 : 5);
            if (a < 4) g.facing = facing_of(d);                        // :164-171
            const uint2 rec = p.rays[R.ray_off + (uint32_t)((g.x * R.D + g.y) * R.H + g.z)];
            const uint32_t e8 = ((d < 4 ? rec.x : rec.y) >> (8 * (d & 3))) & 0x7fu;
            bool bumped = false, explored = false;
            if (e8 >= 1u) {                                              // _mark_visited (:273-298)
                g.x += d == 0 ? 1 : d == 1 ? -1 : 0;
                g.y += d == 2 ? 1 : d == 3 ? -1 : 0;
                g.z += d == 4 ? 1 : d == 5 ? -1 : 0;
                int8_t *c = map + (g.x * p.pd + g.y) * p.ph + g.z;
                const int v = *c;
                if (v == 0 || v == -1) {
                    *c = 1;
                    g.visited += 1;
                    explored = true;
                }
            } else {
                bumped = true;
            }
            g.last_action = a;                                           // :137
            simple_observe(map, p, g, R, row);                           // :139
            // compute_reward (:189-217), f64 in the reference's order
            r = -0.1;
            if (bumped) {
                g.bumps += 1;
                r += -10.0;
            }
            if (a != 2 && a < 4) r += 0.05;                              // last_action == a here
            const int gx = goal & 0xff, gy = (goal >> 8) & 0xff, gz = (goal >> 16) & 0xff;
            was_done = g.done;
            if (g.x == gx && g.y == gy && g.z >= gz && g.z - gz < 5) {   // SPOT_GOAL_HEIGTH = 5 (:201-206)
                g.done = true;
                r += 100.0;
            }
            if (trunc) r += 0.0;                                         // r += -0
            if (explored) r += 1.0;
            term = g.done;
            const size_t o = (size_t)k * p.N + ai;
            if (p.reward) p.reward[o] = (float)r;
            if (p.reward64) p.reward64[o] = r;
            if (p.term) p.term[o] = term;
            if (p.trunc) p.trunc[o] = trunc;
            if ((term || trunc) && p.autoreset && p.terminal_obs) {
                float *to = p.terminal_obs + o * OD;
                for (int q = 0; q < OD; ++q) to[q] = row[q];
            }
        }
        // SB3 VecEnv auto-reset
        // an episode ends: with auto-reset at every ending step; without it at the first one
        // after a reset only (an agent stepped on after its end entered the step with done
        // set or step_count at max_steps, and records nothing more)
        const bool ends = live && (term || trunc) && (p.autoreset || (!was_done && g.step_count - 1u < R.total_free));
        if (__ballot(ends)) {
            if (ends)   // the ended episode's record, before the reset
                episode_end(p.envc, ai, g.step_count, g.bumps, g.visited, R.total_free, (uint32_t)g.room,
                            (term ? EP_TERMINATED : 0u) | (trunc ? EP_TRUNCATED : 0u));
            const bool need = ends && p.autoreset;
            simple_reset_wave(p, map, need, next_seed, g, goal, R, row, lane, a0);
            if (need) next_seed += p.seed_stride;
        }
        __syncthreads();
        float *dst = p.obs + ((size_t)k * p.N + a0) * OD;
        for (int q = lane; q < rows * OD; q += 64) dst[q] = sstage[q];
        __syncthreads();
    }
    if (live) store_agent(p, ai, g, goal, next_seed);
}

// reset for the lanes with `need` (as simple_reset_wave): the wave zeroes
// every resetting agent's planes, then each marks its start cell and senses.
template <int LMAX>
__device__ __forceinline__ void sb_reset_wave(const Params &p, const SPlanes &pl, bool need, uint32_t seed, Agent &g, uint32_t &goal,
                              Room &R, SRows &w, float *row, int lane, int block_agent0) {
    uint2 drawn = make_uint2(0u, 0u);
    if (need) drawn = simple_draw(p.envc, seed);
    zero_agent_blocks(p, __ballot(need), ~0ull, block_agent0, lane);
    if (need) {
        reset_agent(p, drawn, g, goal, R);
        w.wx = 1ull << g.x;                                                     // :86
        w.wy = 1ull << g.y;
        w.wz = 1u << g.z;
        if (p.sline) {                   // line layout: u32 SX[y][z], SY[x][z] (simple_line_kernel)
            reinterpret_cast<uint32_t *>(pl.sx)[g.y * p.ph + g.z] = (uint32_t)w.wx;
            reinterpret_cast<uint32_t *>(pl.sy)[g.x * p.ph + g.z] = (uint32_t)w.wy;
        } else {
            pl.sx[g.y * p.ph + g.z] = w.wx;
            pl.sy[g.x * p.ph + g.z] = w.wy;
            pl.sz[g.x * p.pd + g.y] = w.wz;
        }
        w.rec = p.rays[R.ray_off + (uint32_t)((g.x * R.D + g.y) * R.H + g.z)];
        sb_observe<LMAX>(p, pl, g, w, row);
    }
}

#ifndef VN_SIMPLE_PROF
#define VN_SIMPLE_PROF 0   // diagnostics build: per-section shader-clock totals (vn_debug_simple_prof)
#endif
#if VN_SIMPLE_PROF
__device__ unsigned long long g_simple_prof[16];
#define SB_T_BEGIN                                  \
    uint64_t prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};    \
    uint64_t tprev = __builtin_amdgcn_s_memtime()
#define SB_T(k)                                                    \
    do {                                                           \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();          \
        prof[k] += t_ - tprev;                                     \
        tprev = t_;                                                \
    } while (0)
#define SB_T_END \
    if (lane == 0) simple_prof_flush(prof)
// a stepping wave's section totals (0-6), their sum (7) and the wave count (8)
__device__ __forceinline__ void simple_prof_flush(const uint64_t *prof) {
    uint64_t tot = 0;
    for (int q = 0; q < 7; ++q) {
        atomicAdd(&g_simple_prof[q], (unsigned long long)prof[q]);
        tot += prof[q];
    }
    atomicAdd(&g_simple_prof[7], tot);
    atomicAdd(&g_simple_prof[8], 1ull);
}
#else
#define SB_T_BEGIN (void)0
#define SB_T(k) (void)0
#define SB_T_END (void)0
#endif

// vn_reset for the bit-plane layouts (line and word): 64 agents per block,
// one lane each -- the draws, the cleared planes, the start cell and the
// first observation, then the next episode's draw ahead for the step kernels
// (sp_reset_wave / sl_reset_wave).
template <int LMAX>
__global__ __launch_bounds__(64) void simple_bits_reset_kernel(Params p) {
    extern __shared__ float sstage[];   // [64][obs_dim]
    const int lane = threadIdx.x;
    const int a0 = blockIdx.x * 64;
    const int ai = a0 + lane;
    const bool live = ai < p.N;
    const int OD = p.obs_dim;
    float *row = sstage + lane * OD;
    const SPlanes pl = splanes(p, live ? ai : a0);
    Agent g;
    uint32_t goal, next_seed;   // (next_seed: not used by a reset)
    Room R;
    load_agent(p, ai, live, g, goal, next_seed, R);
    SRows w;
    w.wx = w.wy = 0;
    w.wz = 0;
    w.rec = make_uint2(0u, 0u);
    const bool need = live && (!p.mask || p.mask[ai]);
    const uint32_t seed = need ? (uint32_t)p.seeds[ai] : 0u;
    sb_reset_wave<LMAX>(p, pl, need, seed, g, goal, R, w, row, lane, a0);
    if (need) {
        float *o = p.obs + (size_t)ai * OD;
        for (int k = 0; k < OD; ++k) o[k] = row[k];
        p.hot[ai] = pack(g);
        p.goal[ai] = goal;
        p.next_seed[ai] = seed + p.seed_stride;   // modulo 2^32
    }
    // the next episode's draw ahead (simple_pipe_kernel's sp_reset_wave)
    if (__ballot(need)) {
        const uint32_t s2 = seed + p.seed_stride;
        const uint2 d = need ? simple_draw(p.envc, s2) : make_uint2(0u, 0u);
        if (need) p.predraw[ai] = make_uint4(d.x, d.y, s2, 1u);
    }
}

// ----------------------------------------------------------------------------
// The bit-plane step with a store wave: block = 2 waves, wave 0 steps 64
// agents and stages each step's obs rows, rewards and flags in LDS (double
// buffered), wave 1 writes step k's staging to HBM while wave 0 computes step
// k+1.  vmcnt retires in issue order per wave, so in the one-wave kernel every
// step's loads waited for the previous step's ~8 obs stores per lane to
// complete; here the stepping wave issues no output stores at all (only its
// own S-word / Q updates).  One barrier per step hands a buffer over: the
// store wave has drained its LDS reads of buffer k&1 before it reaches the
// barrier after which wave 0 overwrites that buffer (step k+2).
// LDS: stage[2][64][OD] f32, reward[2][64] f32, flags[2][64] u32.
// ----------------------------------------------------------------------------
// Block barrier that orders only LDS: lgkmcnt(0) then s_barrier.  The store
// wave's HBM stores stay in flight across it (a __syncthreads() would wait
// vmcnt(0), i.e. for every store of the step to complete, before the
// stepping wave may go on).
__device__ __forceinline__ void lds_handoff() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0) alone
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// The store wave of the 2-wave kernels: per step, the block's staged obs rows
// (one contiguous span), rewards and flags from LDS buffer k & 1 to HBM.
__device__ __forceinline__ void store_wave(const Params &p, const float *stage, const float *srew, const uint32_t *sflg,
                                           int lane, int a0, int rows) {
    const int OD = p.obs_dim;
    for (int k = 0; k < p.K; ++k) {
        lds_handoff();                     // step k staged in buffer k & 1
        const int b = k & 1;
        const float *st = stage + b * 64 * OD;
        float *dst = p.obs + ((size_t)k * p.N + a0) * OD;
        if (VN_ABLATE & 16u) {
        } else if (!((rows * OD) & 3) && !(reinterpret_cast<uintptr_t>(dst) & 15u)) {
            const float4 *s4 = reinterpret_cast<const float4 *>(st);
            float4 *d4 = reinterpret_cast<float4 *>(dst);
            for (int q = lane; q < (rows * OD) >> 2; q += 64) obs_store(d4 + q, s4[q]);
        } else {
            for (int q = lane; q < rows * OD; q += 64) __builtin_nontemporal_store(st[q], dst + q);
        }
        if (lane < rows) {
            const size_t o = (size_t)k * p.N + a0 + lane;
            const uint32_t f = sflg[b * 64 + lane];
            if (p.reward) p.reward[o] = srew[b * 64 + lane];
            if (p.term) p.term[o] = (uint8_t)(f & 1u);
            if (p.trunc) p.trunc[o] = (uint8_t)(f >> 1);
        }
    }
}


// ----------------------------------------------------------------------------
// The bit-plane step with a store wave, software-pipelined by one step
// (the default simpleEnv kernel for rooms <= 64 x 64 x 31).  A step's move
// needs only the ray record of the agent's cell, which the previous step
// loaded, so the move of step k+1 is computed -- and the loads at its target
// cell (ray record, the two S words not along the move axis) issued --
// BEFORE step k's observation is built.  Those loads then land while step k
// observes; one stepping wave per SIMD no longer waits a full load round trip
// per step.  The pending move (action, direction, facing, target) is committed
// at the start of the next iteration (visit / S marks in the reference's
// order, :109-150); an auto-reset recomputes it from the start cell.  The
// stepping wave issues no output stores (the store wave does), so waiting for
// its loads never waits for obs stores.
// ----------------------------------------------------------------------------
template <int LMAX>
__device__ __forceinline__ void sp_reset_wave(const Params &p, const SPlanes &pl, bool need, bool live, uint32_t seed,
                                              Agent &g, uint32_t &goal, Room &R, SRows &w, float *row, int lane,
                                              int block_agent0, uint4 &nd, uint32_t *mt_lds) {
    const uint2 drawn = sp_reset_draw(p, need, live, seed, lane, nd, mt_lds);
    zero_agent_blocks(p, __ballot(need), ~0ull, block_agent0, lane);
    if (need) {
        reset_agent(p, drawn, g, goal, R);
        w.wx = 1ull << g.x;                                                     // :86
        w.wy = 1ull << g.y;
        w.wz = 1u << g.z;
        pl.sx[g.y * p.ph + g.z] = w.wx;
        pl.sy[g.x * p.ph + g.z] = w.wy;
        pl.sz[g.x * p.pd + g.y] = w.wz;
        w.rec = p.rays[R.ray_off + (uint32_t)((g.x * R.D + g.y) * R.H + g.z)];
        sb_observe<LMAX>(p, pl, g, w, row);
    }
}

struct SPend {
    int a, d, facing, nx, ny, nz;
    bool moved;
};

template <int LMAX, bool EXT>
__global__ __launch_bounds__(128) void simple_pipe_kernel(Params p) {
    extern __shared__ float sm[];
    const int OD = p.obs_dim;
    float *stage = sm;
    float *srew = sm + 2 * 64 * OD;
    uint32_t *sflg = reinterpret_cast<uint32_t *>(srew + 2 * 64);
    const int lane = threadIdx.x & 63;
    const int a0 = blockIdx.x * 64;
    const int rows = min(64, p.N - a0);

    if (threadIdx.x >= 64) {
        store_wave(p, stage, srew, sflg, lane, a0, rows);
        return;
    }

    // ---- stepping wave ----
    // Every global store of the step loop is issued unconditionally (the
    // evicted S words go through a buffer resource over the block's belief
    // maps; a lane with nothing to store gives an out-of-range offset, which
    // the hardware drops).  vmcnt retires in issue order, so a load can be
    // waited for with the stores issued after it still in flight only when
    // their count is the same on every path; a store skipped by a branch
    // made hipcc wait vmcnt(0) -- for the stores too -- in every step.
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(
        p.belief + (size_t)a0 * p.agent_bytes, 0, (int)((uint32_t)rows * p.agent_bytes), 0x00020000);
    const uint32_t lane_off = (uint32_t)lane * p.agent_bytes;
    const int ai = a0 + lane;
    const bool live = ai < p.N;
    const SPlanes pl = splanes(p, live ? ai : a0);
    Agent g;
    uint32_t goal, next_seed;
    Room R;
    load_agent(p, ai, live, g, goal, next_seed, R);
    uint4 nd = live ? p.predraw[ai] : make_uint4(0u, 0u, 0u, 0u);   // draw ahead (sp_reset_draw)
    SRows w;                                     // S words + ray record at the agent's (committed) cell
    w.wx = w.wy = 0;
    w.wz = 0;
    w.rec = make_uint2(0u, 0u);
    if (live) sb_load_rows(p, pl, g, R, w);
    vn_touch(w.wx);
    vn_touch(w.wy);
    vn_touch(w.wz);
    vn_touch(w.rec.x);
    vn_touch(w.rec.y);
    vn_touch((uint32_t)R.ray_off);
    vn_touch((uint32_t)R.total_free);
    vn_touch((uint32_t)(R.D | (R.H << 8)));

    uint4 r4 = make_uint4(0u, 0u, 0u, 0u);      // Philox block r4blk (4 steps)
    uint64_t r4blk = ~0ull;
    SPend pm;                                    // the pending move
    SRows wn;                                    // ... and the rows at its target (in flight)
    uint64_t cbx = 0ull, cby = 0ull;             // S bits its commit adds to wn's kept rows
    uint32_t cbz = 0u;
    // The S words in w are write-back cached: a mark sets their dirty bits
    // (1 x, 2 y, 4 z); a word is stored when a move replaces it (eviction:
    // its row at the cell being left) and at the end of the launch.  The
    // evicted words of a commit are stored after the next move's loads; a
    // load of an evicted row takes the evicted value (forwarding).
    uint32_t sdirty = 0u, evm = 0u;              // dirty words; evicted words pending store
    uint64_t evx = 0ull, evy = 0ull;             // evicted values ...
    uint32_t evz = 0u;
    int evyx = 0, evxy = 0, evz_ = 0, evxx = 0, evyy = 0;   // ... and their rows: x (y,z)  y (x,z)  z (x,y)
    // the move of launch step k from the committed state; issues the target's loads
    auto premove = [&](int k) {
        const uint64_t t = p.t0 + (uint64_t)k;
        int a;
        if (EXT) {
            a = p.actions[(size_t)k * p.N + (live ? ai : a0)];
        } else {
            if ((t >> 2) != r4blk) {
                r4blk = t >> 2;
                r4 = philox4x32_10(p.policy_seed, p.gid_base + (uint64_t)(live ? ai : a0), t >> 2);
            }
            const uint32_t word = (t & 3) == 0 ? r4.x : (t & 3) == 1 ? r4.y : (t & 3) == 2 ? r4.z : r4.w;
            a = (int)(((uint64_t)word * 6u) >> 32);
        }
        const int d = a < 4 ? rel_dir(a, g.facing) : (a == 4 ? 4 : 5);
        pm.a = a;
        pm.d = d;
        pm.facing = a < 4 ? facing_of(d) : g.facing;                 // :164-171
        pm.moved = (ray_e8(w.rec, d) & 0x7fu) >= 1u;
        pm.nx = g.x + (pm.moved ? (d == 0 ? 1 : d == 1 ? -1 : 0) : 0);
        pm.ny = g.y + (pm.moved ? (d == 2 ? 1 : d == 3 ? -1 : 0) : 0);
        pm.nz = g.z + (pm.moved ? (d == 4 ? 1 : d == 5 ? -1 : 0) : 0);
        wn = w;
        if (pm.moved) {
            // the S word along the move axis is the same row (kept); the other two
            // rows and the ray record are the target's.  These rows never hold
            // the bit the commit of this move sets (they are off the current cell).
            const int ax = d >> 1;
            if (ax != 0) wn.wx = ((evm & 1u) && evyx == pm.ny && evz_ == pm.nz) ? evx : pl.sx[pm.ny * p.ph + pm.nz];
            if (ax != 1) wn.wy = ((evm & 2u) && evxy == pm.nx && evz_ == pm.nz) ? evy : pl.sy[pm.nx * p.ph + pm.nz];
            if (ax != 2) wn.wz = ((evm & 4u) && evxx == pm.nx && evyy == pm.ny) ? evz : pl.sz[pm.nx * p.pd + pm.ny];
            wn.rec = p.rays[R.ray_off + (uint32_t)((pm.nx * R.D + pm.ny) * R.H + pm.nz)];
        }
    };
    if (live && p.K > 0) premove(0);
    SB_T_BEGIN;

    for (int k = 0; k < p.K; ++k) {
        const int b = k & 1;
        float *row = stage + b * 64 * OD + lane * OD;
        bool trunc = false, term = false, was_done = false;   // was_done: `done` entering the step
        int a = 0;
        bool moved = false, explored = false, seen = true;
        if (live) {
            // ---- commit step k (:109-150) ----
            if (p.actions_out) p.actions_out[(size_t)k * p.N + ai] = pm.a;
            g.step_count += 1;
            trunc = g.step_count >= R.total_free;                      // :111, max_steps = total_free (:409)
            g.facing = pm.facing;
            a = pm.a;
            moved = pm.moved;
            if (moved) {                                                 // _mark_visited (:273-298)
                const int ax = pm.d >> 1;
                // the target's S bit from the cached word of the move axis (kept in wn)
                seen = ax == 0 ? ((w.wx >> pm.nx) & 1ull) : ax == 1 ? ((w.wy >> pm.ny) & 1ull) : ((w.wz >> pm.nz) & 1u);
                // evict the dirty words this move replaces (rows at the cell left)
                evm = sdirty & ~(1u << ax);
                evx = w.wx;
                evy = w.wy;
                evz = w.wz;
                evyx = g.y;
                evz_ = g.z;
                evxy = g.x;
                evxx = g.x;
                evyy = g.y;
                sdirty &= 1u << ax;
                g.x = pm.nx;
                g.y = pm.ny;
                g.z = pm.nz;
                w = wn;
            } else {
                evm = 0u;
            }
            // the bits of the previous step's mark that this move's rows were
            // copied without (see below)
            w.wx |= cbx;
            w.wy |= cby;
            w.wz |= cbz;
            cbx = cby = 0ull;
            cbz = 0u;
            g.last_action = a;                                           // :137
            SB_T(0);
            // ---- the next step's move and its loads, issued before this step's
            // S-mark stores (a wait for these loads then never waits for them) ----
            if (k + 1 < p.K) premove(k + 1);
            if (!(VN_ABLATE & 1024u)) {                 // the evicted words, behind the loads
                constexpr uint32_t OFF = 0x80000000u;   // out of range: dropped
                typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
                const u32x2_t vx = {(uint32_t)evx, (uint32_t)(evx >> 32)}, vy = {(uint32_t)evy, (uint32_t)(evy >> 32)};
                __builtin_amdgcn_raw_buffer_store_b64(
                    vx, brs, (evm & 1u) ? lane_off + 8u * (uint32_t)(evyx * p.ph + evz_) : OFF, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(
                    vy, brs, (evm & 2u) ? lane_off + p.sy_off + 8u * (uint32_t)(evxy * p.ph + evz_) : OFF, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(
                    evz, brs, (evm & 4u) ? lane_off + p.sz_off + 4u * (uint32_t)(evxx * p.pd + evyy) : OFF, 0, 0);
            }
            evm = 0u;
            SB_T(1);
            if (moved) {
                // a Q cell (internal_grid 2) is entered without counting, but it
                // is a sensing position all the same, so S is set
                const bool q = (g.move_mask & 1u) && ((pl.qz[g.x * p.pd + g.y] >> g.z) & 1u);
                if (!seen) {
                    const uint64_t bx = 1ull << g.x, by = 1ull << g.y;
                    const uint32_t bz = 1u << g.z;
                    w.wx |= bx;
                    w.wy |= by;
                    w.wz |= bz;
                    // the pending move copied its kept row(s) from w before this
                    // mark (all three if it does not move): carried into its
                    // commit (wn itself is the target of loads in flight)
                    const int nax = pm.moved ? pm.d >> 1 : -1;
                    if (nax <= 0) cbx = bx;
                    if (nax == -1 || nax == 1) cby = by;
                    if (nax == -1 || nax == 2) cbz = bz;
                    sdirty = 7u;
                    if (!q) {
                        g.visited += 1;
                        explored = true;
                    }
                }
            }
            SB_T(2);
            if (!(VN_ABLATE & 4u)) sp_observe<LMAX>(p, pl, g, w, row);   // :139
            SB_T(3);
            // compute_reward (:189-217), f64 in the reference's order
            double r = -0.1;
            if (!moved) {
                g.bumps += 1;
                r += -10.0;
            }
            if (a != 2 && a < 4) r += 0.05;
            const int gx = goal & 0xff, gy = (goal >> 8) & 0xff, gz = (goal >> 16) & 0xff;
            was_done = g.done;
            if (g.x == gx && g.y == gy && g.z >= gz && g.z - gz < 5) {   // SPOT_GOAL_HEIGTH = 5 (:201-206)
                g.done = true;
                r += 100.0;
            }
            if (trunc) r += 0.0;
            if (explored) r += 1.0;
            term = g.done;
            const size_t o = (size_t)k * p.N + ai;
            srew[b * 64 + lane] = (float)r;
            sflg[b * 64 + lane] = (term ? 1u : 0u) | (trunc ? 2u : 0u);
            if (p.reward64) p.reward64[o] = r;
            if ((term || trunc) && p.autoreset && p.terminal_obs) {
                float *to = p.terminal_obs + o * OD;
                for (int q = 0; q < OD; ++q) to[q] = row[q];
            }
        }
        SB_T(4);
        // SB3 VecEnv auto-reset
        // an episode ends: with auto-reset at every ending step; without it at the first one
        // after a reset only (an agent stepped on after its end entered the step with done
        // set or step_count at max_steps, and records nothing more)
        const bool ends = live && (term || trunc) && (p.autoreset || (!was_done && g.step_count - 1u < R.total_free)) &&
                          !(VN_ABLATE & 512u);
        if (__ballot(ends)) {
            if (ends)   // the ended episode's record, before the reset
                episode_end(p.envc, ai, g.step_count, g.bumps, g.visited, R.total_free, (uint32_t)g.room,
                            (term ? EP_TERMINATED : 0u) | (trunc ? EP_TRUNCATED : 0u));
            const bool need = ends && p.autoreset;
            sp_reset_wave<LMAX>(p, pl, need, live, next_seed, g, goal, R, w, row, lane, a0, nd,
                                reinterpret_cast<uint32_t *>(sflg + 2 * 64));
            if (need) {
                next_seed += p.seed_stride;
                cbx = cby = 0ull;
                cbz = 0u;
                sdirty = 0u;                             // the reset stored the start cell's words
                evm = 0u;
                if (k + 1 < p.K) premove(k + 1);                         // from the start cell
                vn_touch(w.rec.x);
                vn_touch(w.rec.y);
                vn_touch((uint32_t)R.ray_off);
                vn_touch((uint32_t)R.total_free);
                vn_touch((uint32_t)(R.D | (R.H << 8)));
            }
        }
        SB_T(5);
        lds_handoff();                         // hand buffer b to the store wave
        SB_T(6);
    }
    SB_T_END;
    if (live) {
        if (sdirty & 1u) pl.sx[g.y * p.ph + g.z] = w.wx;
        if (sdirty & 2u) pl.sy[g.x * p.ph + g.z] = w.wy;
        if (sdirty & 4u) pl.sz[g.x * p.pd + g.y] = w.wz;
        store_agent(p, ai, g, goal, next_seed);
        p.predraw[ai] = nd;
    }
}

// reset of the lanes with `need` (sp_reset_wave in the line layout): the
// wave zeroes every resetting agent's SX / SY lines (and QZ if it holds
// marks), then each marks its start cell in its LDS lines (dirty) and senses
template <int LMAX>
__device__ __forceinline__ void sl_reset_wave(const Params &p, const SPlanes &pl, bool need, bool live, uint32_t seed,
                                              Agent &g, uint32_t &goal, Room &R, SRows &w, float *row, int lane,
                                              int block_agent0, uint4 &nd, uint32_t *mt_lds, uint32_t *lx,
                                              uint32_t *ly) {
    const uint2 drawn = sp_reset_draw(p, need, live, seed, lane, nd, mt_lds);
    // QZ (at the end of the agent's block) is all zero unless the episode marked it
    zero_agent_blocks(p, __ballot(need), __ballot(need && (g.move_mask & 1u)), block_agent0, lane);
    if (need) {
        reset_agent(p, drawn, g, goal, R);
        w.wx = 1ull << g.x;                                                     // :86
        w.wy = 1ull << g.y;
        w.wz = 1u << g.z;
#pragma unroll
        for (int z = 0; z < 8; ++z) {
            lx[z] = z == g.z ? (uint32_t)w.wx : 0u;
            ly[z] = z == g.z ? (uint32_t)w.wy : 0u;
        }
        w.rec = p.rays[R.ray_off + (uint32_t)((g.x * R.D + g.y) * R.H + g.z)];
        sb_observe<LMAX>(p, pl, g, w, row);
    }
}

template <int LMAX, bool EXT>
__global__ __launch_bounds__(128) void simple_line_kernel(Params p) {
    extern __shared__ float sm[];
    const int OD = p.obs_dim;
    float *stage = sm;
    float *srew = sm + 2 * 64 * OD;
    uint32_t *sflg = reinterpret_cast<uint32_t *>(srew + 2 * 64);
    uint32_t *mt_lds = sflg + 2 * 64;
    uint32_t *lines = mt_lds + 64 * MT_WS + 4;   // [3][64][SL_STRIDE] (X, Y, dummy); 16-B aligned
    float4 *clut = reinterpret_cast<float4 *>(lines + 3 * 64 * SL_STRIDE);   // [SL_CLUT] (sl_observe)
    float *srt = reinterpret_cast<float *>(clut + SL_CLUT);   // [16] f32, then [16] f64 rewards (TAB_SREW)
    const double *srt64 = reinterpret_cast<const double *>(srt + 16);
    const int lane = threadIdx.x & 63;
    const int a0 = blockIdx.x * 64;
    const int rows = min(64, p.N - a0);

    if (threadIdx.x >= 64) {
        store_wave(p, stage, srew, sflg, lane, a0, rows);
        return;
    }

    // ---- stepping wave ----
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(
        p.belief + (size_t)a0 * p.agent_bytes, 0, (int)((uint32_t)rows * p.agent_bytes), 0x00020000);
    const uint32_t lane_off = (uint32_t)lane * p.agent_bytes;
    const bool odd = lane & 1;
    const int ai = a0 + lane;
    const bool live = ai < p.N;
    uint32_t *lx = lines + lane * SL_STRIDE;           // SX[g.y]
    uint32_t *ly = lines + (64 + lane) * SL_STRIDE;    // SY[g.x]
    uint32_t *lz = lines + (128 + lane) * SL_STRIDE;   // target of a commit's line write without a line
    sl_build_cell_lut(clut, lane);
    if (lane < 48) srt[lane] = p.lut[TAB_SREW + lane];
    const SPlanes pl = splanes(p, live ? ai : a0);
    Agent g;
    uint32_t goal, next_seed;
    Room R;
    load_agent(p, ai, live, g, goal, next_seed, R);
    uint4 nd = live ? p.predraw[ai] : make_uint4(0u, 0u, 0u, 0u);   // draw ahead (sp_reset_draw)
    auto xline_off = [&](int y) { return lane_off + 32u * (uint32_t)y; };
    auto yline_off = [&](int x) { return lane_off + p.sy_off + 32u * (uint32_t)x; };
    SRows w;                                     // S words + ray record at the agent's (committed) cell
    {
        const SLine l0 = sl_pair_load(brs, live ? xline_off(g.y) : SL_OFF, odd);
        const SLine l1 = sl_pair_load(brs, live ? yline_off(g.x) : SL_OFF, odd);
        sl_lds_put(lx, l0);
        sl_lds_put(ly, l1);
        w.wx = lx[g.z & 7];
        w.wy = ly[g.z & 7];
        w.wz = sl_column(l0, g.x & 31);
        w.rec = live ? p.rays[R.ray_off + (uint32_t)((g.x * R.D + g.y) * R.H + g.z)] : make_uint2(0u, 0u);
    }
    vn_touch((uint32_t)R.ray_off);
    vn_touch((uint32_t)R.total_free);
    vn_touch((uint32_t)(R.D | (R.H << 8)));

    uint4 r4 = make_uint4(0u, 0u, 0u, 0u);      // Philox block r4blk (4 steps)
    uint64_t r4blk = ~0ull;
    SPend pm;                                    // the pending move ...
    SLine lr;                                    // ... the line it brings in (raw pair loads, in flight;
    bool lfwd = false;                           //     or the replaced line: lfwd) ...
    uint32_t lpend = SL_OFF;                     //     (its offset: a re-issue repeats it) ...
    uint2 rn = make_uint2(0u, 0u);               // ... and its target's ray record (in flight)
    uint32_t dirty = 0u;                         // 1: the LDS X line is marked, 2: the Y line
    SLine ev;                                    // the line the last commit replaced, stored after the
    uint32_t ev_off = SL_OFF;                    // next move's loads (a load of it takes it from here)
    ev.h0 = ev.h1 = u32x4_t{0u, 0u, 0u, 0u};
    lr = ev;
    // the move of launch step k from the committed state; issues the target's loads
    // keep: lanes without `act` keep their pending move.  The line loads are
    // re-issued for them too: a lane pair's two loads carry both lanes' lines
    // (sl_pair_issue), so the pair always issues together.
    auto premove = [&](int k, bool act, bool keep) {
        uint32_t loff = (keep && !act) ? lpend : SL_OFF;
        uint32_t rcell = 0u;
        if (act) {
            const uint64_t t = p.t0 + (uint64_t)k;
            int a;
            if (EXT) {
                a = p.actions[(size_t)k * p.N + ai];
            } else {
                if ((t >> 2) != r4blk) {
                    r4blk = t >> 2;
                    r4 = philox4x32_10(p.policy_seed, p.gid_base + (uint64_t)ai, t >> 2);
                }
                const uint32_t word = (t & 3) == 0 ? r4.x : (t & 3) == 1 ? r4.y : (t & 3) == 2 ? r4.z : r4.w;
                a = (int)(((uint64_t)word * 6u) >> 32);
            }
            const int d = a < 4 ? rel_dir(a, g.facing) : (a == 4 ? 4 : 5);
            pm.a = a;
            pm.d = d;
            pm.facing = a < 4 ? facing_of(d) : g.facing;                 // :164-171
            pm.moved = (ray_e8(w.rec, d) & 0x7fu) >= 1u;
            pm.nx = g.x + (pm.moved ? (d == 0 ? 1 : d == 1 ? -1 : 0) : 0);
            pm.ny = g.y + (pm.moved ? (d == 2 ? 1 : d == 3 ? -1 : 0) : 0);
            pm.nz = g.z + (pm.moved ? (d == 4 ? 1 : d == 5 ? -1 : 0) : 0);
            rcell = (uint32_t)((pm.nx * R.D + pm.ny) * R.H + pm.nz);
            // the line a move along x (y) brings in: SY[nx] (SX[ny]); from ev (no
            // request) if it is the line the last commit replaced
            if (pm.moved && d < 4) {
                const uint32_t o = d < 2 ? yline_off(pm.nx) : xline_off(pm.ny);
                if (o != ev_off) loff = o;
            }
        }
        lr = sl_pair_issue(brs, loff, odd);
        lpend = loff;
        const uint2 rc = p.rays[R.ray_off + rcell];
        if (!keep || act) {
            lfwd = loff == SL_OFF;               // forwarded from ev (or unused)
            rn = rc;
        }
    };
    if (p.K > 0) premove(0, live, false);
    SB_T_BEGIN;

    for (int k = 0; k < p.K; ++k) {
        const int b = k & 1;
        float *row = stage + b * 64 * OD + lane * OD;
        bool trunc = false, term = false, was_done = false;   // was_done: `done` entering the step
        int a = 0;
        bool moved = false, explored = false, seen = true;
        if (live) {
            // ---- commit step k (:109-150) ----
            if (p.actions_out) p.actions_out[(size_t)k * p.N + ai] = pm.a;
            g.step_count += 1;
            trunc = g.step_count >= R.total_free;                      // :111, max_steps = total_free (:409)
            g.facing = pm.facing;
            a = pm.a;
            moved = pm.moved;
        }
        {
            // _mark_visited (:273-298); straight-line for every lane: a lane
            // whose move brings no line writes it to its dummy slot
            const int ax = moved ? pm.d >> 1 : 3;
            const bool xy = ax < 2;
            // the target's S bit from the word along the move axis
            seen = !moved || (ax == 0 ? ((w.wx >> pm.nx) & 1ull) : ax == 1 ? ((w.wy >> pm.ny) & 1ull)
                                                                            : ((w.wz >> pm.nz) & 1u));
            // replace the line across the move axis: the old one is stored if marked
            uint32_t *slot = ax == 0 ? ly : ax == 1 ? lx : lz;
            const uint32_t dbit = ax == 0 ? 2u : 1u;
            const SLine lf = sl_pair_finish(lr, odd);
            const SLine ln = lfwd ? ev : lf;
            ev = sl_lds_get(slot);
            ev_off = (xy && (dirty & dbit)) ? (ax == 0 ? yline_off(g.x) : xline_off(g.y)) : SL_OFF;
            dirty &= xy ? ~dbit : ~0u;
            sl_lds_put(slot, ln);
            if (moved) {
                g.x = pm.nx;
                g.y = pm.ny;
                g.z = pm.nz;
                w.rec = rn;
            }
            w.wx = lx[g.z];
            w.wy = ly[g.z];
            const uint32_t col = sl_column(sl_lds_get(lx), g.x);
            if (xy) w.wz = col;
        }
        if (live) {
            g.last_action = a;                                           // :137
        }
        SB_T(0);
        // ---- the replaced line's store, then the next step's move and its
        // loads: vmcnt retires in issue order, so the wait for the loads (a
        // step later) covers the older store at no cost; a store issued after
        // them would be waited for as well (the compiler's counts do not
        // include stores on this target and it waits vmcnt(0) for the last load) ----
        sl_pair_store(brs, ev_off, ev, odd);
        premove(k + 1, live && k + 1 < p.K, false);
        ev_off = SL_OFF;
        SB_T(1);
        if (live) {
            if (moved) {
                // a Q cell (internal_grid 2) is entered without counting, but it
                // is a sensing position all the same, so S is set
                const bool q = (g.move_mask & 1u) && ((pl.qz[g.x * p.pd + g.y] >> g.z) & 1u);
                if (!seen) {
                    w.wx |= 1ull << g.x;
                    w.wy |= 1ull << g.y;
                    w.wz |= 1u << g.z;
                    lx[g.z] = (uint32_t)w.wx;
                    ly[g.z] = (uint32_t)w.wy;
                    dirty = 3u;
                    if (!q) {
                        g.visited += 1;
                        explored = true;
                    }
                }
            }
            SB_T(2);
            if (!(VN_ABLATE & 4u)) sl_observe<LMAX>(p, pl, g, w, row, clut);   // :139
            SB_T(3);
            // compute_reward (:189-217): the reference's f64 sum for the step's
            // events, tabulated on the host in its order (TAB_SREW)
            const int gx = goal & 0xff, gy = (goal >> 8) & 0xff, gz = (goal >> 16) & 0xff;
            const bool hit = g.x == gx && g.y == gy && g.z >= gz && g.z - gz < 5;   // SPOT_GOAL_HEIGTH = 5
            if (!moved) g.bumps += 1;
            was_done = g.done;
            if (hit) g.done = true;
            const uint32_t ev = (moved ? 0u : 1u) | ((a != 2 && a < 4) ? 2u : 0u) | (hit ? 4u : 0u) |
                                (explored ? 8u : 0u);
            term = g.done;
            const size_t o = (size_t)k * p.N + ai;
            srew[b * 64 + lane] = srt[ev];
            sflg[b * 64 + lane] = (term ? 1u : 0u) | (trunc ? 2u : 0u);
            if (p.reward64) p.reward64[o] = srt64[ev];
            if ((term || trunc) && p.autoreset && p.terminal_obs) {
                float *to = p.terminal_obs + o * OD;
                for (int q = 0; q < OD; ++q) to[q] = row[q];
            }
        }
        SB_T(4);
        // SB3 VecEnv auto-reset
        // an episode ends: with auto-reset at every ending step; without it at the first one
        // after a reset only (an agent stepped on after its end entered the step with done
        // set or step_count at max_steps, and records nothing more)
        const bool ends = live && (term || trunc) && (p.autoreset || (!was_done && g.step_count - 1u < R.total_free)) &&
                          !(VN_ABLATE & 512u);
        if (__ballot(ends)) {
            if (ends)   // the ended episode's record, before the reset
                episode_end(p.envc, ai, g.step_count, g.bumps, g.visited, R.total_free, (uint32_t)g.room,
                            (term ? EP_TERMINATED : 0u) | (trunc ? EP_TRUNCATED : 0u));
            const bool need = ends && p.autoreset;
            sl_reset_wave<LMAX>(p, pl, need, live, next_seed, g, goal, R, w, row, lane, a0, nd, mt_lds, lx, ly);
            if (need) {
                next_seed += p.seed_stride;
                dirty = 3u;                              // the start cell's lines (LDS only)
            }
            // from the start cell (the wave's loads are issued together)
            premove(k + 1, need && k + 1 < p.K, true);
        }
        SB_T(5);
        lds_handoff();                         // hand buffer b to the store wave
        SB_T(6);
    }
    SB_T_END;
    sl_pair_store(brs, (live && (dirty & 1u)) ? xline_off(g.y) : SL_OFF, sl_lds_get(lx), odd);
    sl_pair_store(brs, (live && (dirty & 2u)) ? yline_off(g.x) : SL_OFF, sl_lds_get(ly), odd);
    if (live) {
        store_agent(p, ai, g, goal, next_seed);
        p.predraw[ai] = nd;
    }
}

// internal_grid value of one cell from S, Q and the walls (see the layout
// note above the bit-plane kernel)
__device__ int8_t sb_belief_cell(const Params &p, int i, const Room &R, int x, int y, int z) {
    const SPlanes pl = splanes(p, i);
    auto wall = [&](int cx, int cy, int cz) {
        return ((p.rays[R.ray_off + (uint32_t)((cx * R.D + cy) * R.H + cz)].y >> 16) & 1u) != 0u;
    };
    auto sbit = [&](int cx, int cy, int cz) {
        if (p.sline) return ((reinterpret_cast<const uint32_t *>(pl.sx)[cy * p.ph + cz] >> cx) & 1u) != 0u;
        return ((pl.sz[cx * p.pd + cy] >> cz) & 1u) != 0u;
    };
    const bool is_wall = wall(x, y, z);
    if (!is_wall && ((pl.qz[x * p.pd + y] >> z) & 1u)) return 2;
    if (sbit(x, y, z)) return 1;
    static constexpr int DX[6] = {1, -1, 0, 0, 0, 0}, DY[6] = {0, 0, 1, -1, 0, 0}, DZ[6] = {0, 0, 0, 0, 1, -1};
    for (int d = 0; d < 6; ++d) {
        for (int s = 1; s <= p.L; ++s) {   // a sensing position p = c - s * d, free cells in between
            const int px = x - DX[d] * s, py = y - DY[d] * s, pz = z - DZ[d] * s;
            if (px < 0 || px >= R.W || py < 0 || py >= R.D || pz < 0 || pz >= R.H || wall(px, py, pz)) break;
            if (sbit(px, py, pz)) return is_wall ? 2 : 0;
        }
    }
    return -1;
}

__global__ void export_belief_simple_kernel(Params p, int8_t *out, int pw, int pd) {
    const size_t cells = (size_t)pw * pd * p.ph;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= cells * (size_t)p.N) return;
    const int i = (int)(gid / cells);
    const size_t c = gid - (size_t)i * cells;
    const int z = (int)(c % p.ph), y = (int)((c / p.ph) % pd), x = (int)(c / ((size_t)p.ph * pd));
    const Agent g = unpack(p.hot[i]);
    const Room R = load_room(p, g.room);
    int8_t v = -128;
    if (x < R.W && y < R.D && z < R.H && p.sbits)
        v = sb_belief_cell(p, i, R, x, y, z);
    else if (x < R.W && y < R.D && z < R.H)
        v = p.belief[(size_t)i * p.agent_bytes + (size_t)(x * p.pd + y) * p.ph + z];
    out[gid] = v;
}

}  // namespace

namespace vn_simple {

// Params crosses the unit boundary as a pointer: each unit has its own
// (identical) copy of the anonymous-namespace layout from env_params.h.

int ensure_mt(int device) { return ensure_mt_table(device); }

// The simpleEnv kernel of a call shape, picked here for launch and label alike:
// the line layout's step kernel (rooms <= 32 x 32 x 8), the word layout's
// (<= 64 x 64 x 31), the bit-plane reset kernel for both, the dense-map kernel
// for larger rooms; LMAX is L's bucket.
enum Family { LINE, PIPE, BITS_RESET, DENSE };
struct Pick {
    Family fam;
    int lmax;
};
static Pick pick(bool reset_only, int sline, int sbits, int L) {
    const Family fam = (!reset_only && sline) ? LINE : (!reset_only && sbits) ? PIPE : sbits ? BITS_RESET : DENSE;
    return {fam, L <= 4 ? 4 : L <= 8 ? 8 : L <= 10 ? 10 : 16};
}
// LDS: one wave's obs rows; the 2-wave step kernels double-buffer them with the
// rewards and flags and keep the MT rows (PIPE), and the lines, the cell
// table and the reward table as well (LINE)
static size_t lds_bytes(Family fam, int obs_dim) {
    const size_t rows = (size_t)64 * obs_dim * sizeof(float);
    const size_t pipe = 2 * rows + 2 * 64 * 8 + 64 * MT_WS * 4;
    return fam == LINE ? pipe + (4 + 3 * 64 * SL_STRIDE) * 4 + SL_CLUT * 16 + 48 * 4 : fam == PIPE ? pipe : rows;
}

template <int LM>
static void launch_lm(Family fam, bool reset_only, dim3 grid, size_t lds, const Params &p, hipStream_t s) {
    switch (fam) {
    case LINE:   // stepping wave + store wave per 64 agents
        if (p.actions) hipLaunchKernelGGL((simple_line_kernel<LM, true>), grid, dim3(128), lds, s, p);
        else hipLaunchKernelGGL((simple_line_kernel<LM, false>), grid, dim3(128), lds, s, p);
        break;
    case PIPE:   // software-pipelined stepping wave + store wave per 64 agents
        if (p.actions) hipLaunchKernelGGL((simple_pipe_kernel<LM, true>), grid, dim3(128), lds, s, p);
        else hipLaunchKernelGGL((simple_pipe_kernel<LM, false>), grid, dim3(128), lds, s, p);
        break;
    case BITS_RESET:
        hipLaunchKernelGGL((simple_bits_reset_kernel<LM>), grid, dim3(64), lds, s, p);
        break;
    case DENSE:
        if (reset_only) hipLaunchKernelGGL((simple_kernel<true>), grid, dim3(64), lds, s, p);
        else hipLaunchKernelGGL((simple_kernel<false>), grid, dim3(64), lds, s, p);
        break;
    }
}

int launch(bool reset_only, int sline, int sbits, int L, int N, int obs_dim, const void *params, hipStream_t s) {
    const Params &p = *static_cast<const Params *>(params);
    const Pick k = pick(reset_only, sline, sbits, L);
    const dim3 grid((unsigned)((N + 63) / 64));
    const size_t lds = lds_bytes(k.fam, obs_dim);
    if (k.lmax == 4) launch_lm<4>(k.fam, reset_only, grid, lds, p, s);
    else if (k.lmax == 8) launch_lm<8>(k.fam, reset_only, grid, lds, p, s);
    else if (k.lmax == 10) launch_lm<10>(k.fam, reset_only, grid, lds, p, s);
    else launch_lm<16>(k.fam, reset_only, grid, lds, p, s);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

std::string label(bool reset_only, bool ext, int sline, int sbits, int L) {
    char buf[96];
    const Pick k = pick(reset_only, sline, sbits, L);
    const char *tf = (k.fam == DENSE ? reset_only : ext) ? "true" : "false";
    if (k.fam == DENSE) std::snprintf(buf, sizeof(buf), "simple_kernel<%s>", tf);
    else if (k.fam == BITS_RESET) std::snprintf(buf, sizeof(buf), "simple_bits_reset_kernel<%d>", k.lmax);
    else std::snprintf(buf, sizeof(buf), "simple_%s_kernel<%d, %s>", k.fam == LINE ? "line" : "pipe", k.lmax, tf);
    return buf;
}

int export_belief(const void *params, int8_t *out, int pw, int pd, hipStream_t s) {
    const Params &p = *static_cast<const Params *>(params);
    const size_t total = (size_t)p.N * pw * pd * p.ph;
    hipLaunchKernelGGL(export_belief_simple_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, out,
                       pw, pd);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace vn_simple

#if VN_SIMPLE_PROF
extern "C" int vn_debug_simple_prof(unsigned long long *out16, int clear) {
    VN_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_simple_prof), sizeof(unsigned long long) * 16));
    if (clear) {
        unsigned long long z[16] = {0};
        VN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_simple_prof), z, sizeof(z)));
    }
    return VN_OK;
}
#endif
