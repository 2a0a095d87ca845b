// voxnav_env.hip -- MI355X (gfx950) batched voxel-grid exploration env.
//
// The hot path of Noimps/3D-Navigation-Reinforcement-Learning is
// GridAgent.step/reset in envs/CubicEnv.py, run one agent per OS process
// under SB3's SubprocVecEnv (train/Grid_Train.py:191-192).  Here every agent
// is a group of 4 lanes of a 64-wide wavefront (16 agents per wave) and a
// launch advances all N agents by K steps.  See DESIGN.md for the data layout and the roofline.
//
// Layout in HBM
//   hot state   uint4 per agent (16 B, SoA across agents -> coalesced)
//     w0 = x | y<<8 | z<<16 | facing<<21 | last_action<<23 | done<<26
//          | last_bump<<27 | near_wall<<28 | was_near_wall<<29
//     w1 = step_count (24 b, saturating) | cells_insight_down<<24
//     w2 = visited_count (24 b) | room<<24
//     w3 = bump_count (26 b, saturating) | move_mask<<26  (6 b: first cell
//          free in +x,-x,+y,-y,+z,-z -> the next move needs no memory read)
//   belief map  one byte per cell (the reference's internal_grid): bit7
//     known, bit6 wall, bits0-5 visit count saturating at 63 -- the obs
//     clips at 20 (CubicEnv.py:274) and the reward caps at 25 (:180), so
//     the saturation is observationally exact.  Per agent the map is bricked:
//     4x4 (x,y) columns of PH bytes (z contiguous), bricks x-major, so the
//     4x4x4 window is <=4 bricks and an x/y ray crosses <=4 bricks.
//   room tables (tiny, L2 resident): per cell an 8-byte ray record with the
//     free-run length to the first wall/OOB in each of the 6 axis directions
//     (bit7 = ended at a wall) and a wall flag, so a sensing sweep needs one
//     8-byte load instead of 6L grid probes.
//
// Arithmetic follows the reference bit for bit: reward in f64 in the
// reference's operation order (file compiled with -ffp-contract=off), obs
// window values from a 23-entry f32 table built on the host with IEEE f32
// division, obs[68], [71], [72] as f64 quotients rounded to f32.
//
// This file is the CubicEnv kernel unit: the step kernel -- over the plane
// code (env_planes.h), the window tile (env_window.h) and the sensing pass
// and reset (env_sense.h), headers of this unit alone -- the export kernels,
// gae_kernel, and at the end the vn_cubic interface (env_params.h): which
// env_kernel instantiation a call launches, its label, and the exports.
// The C-ABI entry points, VnEnv and the host-side planning (room tables,
// per-agent layout, LUT) are in voxnav_api.hip and env_plan.h.

#include "env_core.h"
#include "env_planes.h"
#include "env_window.h"
#include "env_sense.h"

// Compile-time knobs of this unit still in use as measuring tools and resource
// studies (diagnostics builds only: vn_common.h; scripts/ab.py, env_prof.py,
// env_wt.py, kres.py, placement_probe.py).  VN_ABLATE is in env_core.h,
// VN_WIMG_REP and VN_BRICK_T in env_plan.h; VN_LDS_PAD_U64 (env_kernel: u64
// words of LDS padding, occupancy at a larger footprint) has no default.
#ifndef VN_ENV_PROF
#define VN_ENV_PROF 0             // per-section shader-clock totals of the step loop (vn_debug_env_prof)
#endif
#ifndef VN_ENV_WT
#define VN_ENV_WT 0               // each wave's start / end clock of the last launch, nothing else
#endif
#ifndef VN_PC_BLOCK
#define VN_PC_BLOCK 256           // threads per block of the plane-set kernels
#endif
#ifndef VN_PC_MIN_WAVES
#define VN_PC_MIN_WAVES 4         // plane-set kernels: waves per SIMD the VGPR budget is set for
#endif
#ifndef VN_MIN_WAVES_PER_SIMD
#define VN_MIN_WAVES_PER_SIMD 4   // byte-mark kernels: <= 128 VGPRs, the 16 waves of 256 agents per CU resident at once
#endif

namespace {

// ----------------------------------------------------------------------------
// the step kernel: 4 lanes per agent, K fused steps, SB3 auto-reset
// ----------------------------------------------------------------------------

// compute_reward (envs/CubicEnv.py:169-224) from a step's events, f64 in the
// reference's order, rounded to the f32 rollout buffer.  ev: bits 0-4
// min(center visit count, 25) (pen = min(0.5, 0.02 n) is 0.5 from n = 25 on:
// 25 * 0.02 rounds to 0.5 in f64), 5 moved, 6 was_near_wall, 7 repeated
// non-back move, 8 back after back, 9 explored, 10 done, 11 truncated.
__device__ __forceinline__ double reward_of_events(uint32_t ev, double crash_penalty) {
    double r = -0.05;
    const double pen = (double)(ev & 31u) * 0.02;
    r -= (0.5 < pen) ? 0.5 : pen;
    if (!(ev & 32u)) {
        r += crash_penalty;
    } else {
        if (ev & 64u) r += 0.15;
        if (ev & 128u) r += 0.05;
        if (ev & 256u) r -= 0.5;
    }
    if (ev & 512u) r += 1.0;
    if (ev & 1024u) r += 100.0;
    if (ev & 2048u) r += -5.0;
    return r;
}

constexpr int BLOCK = 256;

#if VN_ENV_PROF || VN_ENV_WT
// per wave of the last profiled launch: start / end on the 100-MHz clock and HW_ID / XCC_ID
__device__ unsigned long long g_env_wt[8192 * 2];
__device__ unsigned int g_env_wid[8192 * 2];
#endif
#if VN_ENV_PROF
__device__ unsigned long long g_env_prof[16];
#define ENV_T(k)                                                   \
    do {                                                           \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();          \
        eprof[k] += t_ - tprev;                                    \
        tprev = t_;                                                \
    } while (0)
#else
#define ENV_T(k) \
    do {         \
    } while (0)
#endif

// EXT: actions come from p.actions (else the Philox random policy).  A
// separate instantiation: with both sources in one loop the action register
// may hold a pending load on entry to every step, and the compiler then waits
// for all outstanding stores of the previous step before the move is known.
// FAST: reward / terminated / truncated requested, actions_out not (the
// rollout-buffer call, reward64 optional): no runtime pointer tests in the
// step loop.
// PC: plane-set mode (see pset_fill).  36 KiB of LDS per 256-thread block
// (u32 rows), so 16 waves fit a CU; measured full episode: 256 threads
// 7.32, 128 7.21, 64 7.18 G env-steps/s (VN_PC_BLOCK).
// rows fwd, right, back, left; cols facing N,E,S,W; dirs 0 +x, 1 -x, 2 +y, 3 -y
constexpr uint32_t kMoveDir = (2u << 0) | (0u << 2) | (3u << 4) | (1u << 6)       // fwd
                              | (0u << 8) | (3u << 10) | (1u << 12) | (2u << 14)   // right
                              | (3u << 16) | (1u << 18) | (2u << 20) | (0u << 22)  // back
                              | (1u << 24) | (2u << 26) | (0u << 28) | (3u << 30); // left
// wave issue priority (s_setprio) while the step's move is computed and its
// loads issued (3), and while the obs flush's stores are issued (2): of the
// 4 waves on a SIMD the one about to put requests in the memory queues goes
// first, the sensing VALU work of the others fills the gaps.  Paired A/B on
// one env allocation (scripts/ab_same.py, profiles/r05/ab_setprio_paired.log):
// box rooms +3.3 % at 20- and 128-step launches, +0.7 % one-step; P-set rooms
// +0-1 %.  Also priority on the reward stores, the shift commit, the launch's
// flush, or level 1 / 2 on the issue: no better.  Runtime switch per call:
// VnTuning::prio bit 0 (issue) / bit 1 (flush) / bit 6 (a base level 0..2
// between the two, plane-set kernels, launches of >= 8 steps: the number of
// the SIMD's other waves that are ahead of this one, wave_progress below; with
// bit 2 the open-loop rotation over the CU's blocks that it replaced), default 67.
// (Bit 3 of the same field is no priority: PRIO_TABLE below, read by launch_ph alone.)
// One runtime level dispatch per step (vn_setprio: the instruction takes an
// immediate): after the issue section; the flush's level stays until the
// next step's issue section raises it (a few instructions later).
constexpr int kPrioIssue = 3;   // while the step's move is computed and its loads issued
constexpr int kPrioFlush = 2;   // while the obs flush's stores are issued
// Params::prio bits the host sets (vn_cubic::launch), beside env_window.h's PRIO_WREC_*:
constexpr int PRIO_ROTATE = 4;          // (user bit) the base level is the open-loop rotation
constexpr int PRIO_TABLE = 8;           // (user bit, read by the host only) a box-exact env launches the table kernels
constexpr int PRIO_BASE = 512;          // a base level applies: bit 6, a plane-set kernel, K >= 8
constexpr int PRIO_TAG_SHIFT = 12;      // bits 12..31: the launch's tag in the progress table

// The progress table of the closed-loop base level: one word per hardware
// wave slot of the device, indexed by where the wave really runs (XCC_ID;
// HW_ID's SE / SH / CU bits 8-15, SIMD bits 4-5, wave id bits 0-2: gfx950 has
// 8 wave slots per SIMD), never by an assumed dispatch order.  A word is
// launch tag << 8 | 4-step blocks the wave has completed (saturating at 255).
// After each block, behind its reward stores, the wave reads its SIMD's row
// of 8 words, takes as the next block's level the number of words of its
// launch that have completed at least as many blocks as it now has -- the
// mates that finished this block before it -- clamped to 2, and lane 0 stores
// the wave's own word (an ordinary vector store, through to L2).  The row is
// wave-uniform, so it is one scalar load: it holds no vector register (the
// plane-set kernels have none to spare at 4 waves per SIMD; a row kept in one
// cost 2 spilled VGPRs) and lgkmcnt does not order it behind the step's
// vector stores.  An invalidate of the scalar cache goes ahead of it (the step
// loop makes no other scalar load); the row then comes from the XCD's L2,
// which every wave of the SIMD writes through to.  Words of another tag (an
// earlier launch, another env of the device, a finished wave: it clears its
// word) are ignored; nothing waits on, polls or loops over the table, and a
// wrong or missing word costs a priority only.  DESIGN.md 7.19.
constexpr int kProgRow = 8;
__device__ __attribute__((aligned(64))) unsigned int g_wave_progress[8 * 256 * 4 * kProgRow];
typedef uint32_t ProgRow __attribute__((ext_vector_type(8)));
// the wave's word index: its SIMD's row is [idx & ~7, idx | 7]
__device__ __forceinline__ uint32_t wave_progress_index() {
    const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_ID
    const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);    // XCC_ID
    return ((((xcc & 7u) << 8 | ((hw >> 8) & 0xffu)) << 2 | ((hw >> 4) & 3u)) << 3) | (hw & 7u);
}
__device__ __forceinline__ ProgRow wave_progress_row(uint32_t idx) {
    typedef const volatile ProgRow __attribute__((address_space(4))) *RowPtr;   // uniform: a scalar load, kept in place
    __builtin_amdgcn_s_dcache_inv();
    __builtin_amdgcn_s_waitcnt(0xc07f);                                         // lgkmcnt(0): the invalidate is done
    return *(RowPtr)(g_wave_progress + (idx & ~(kProgRow - 1u)));
}
__device__ __forceinline__ int wave_progress_level(ProgRow r, uint32_t me) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < kProgRow; ++w) n += (r[w] >= me && (r[w] ^ me) < 256u) ? 1 : 0;
    return n < 2 ? n : 2;
}
// s_setprio with a wave-uniform runtime level (the instruction takes an immediate)
__device__ __forceinline__ void vn_setprio(int v) {
    if (v <= 0) __builtin_amdgcn_s_setprio(0);
    else if (v == 1) __builtin_amdgcn_s_setprio(1);
    else if (v == 2) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(3);
}

// The wave's obs flush of launch step kk: its 16 staged rows (PC: code words
// through the LUT) -> [K][N][80], 1 KiB contiguous per store.
//
// DFL (the deferred flush: step kk's rows stored after step kk + 1's loads
// are issued, full waves only): exactly five store instructions on every
// path, no lane mask and no branch -- kk < 0 (the launch's first step, which
// has no previous rows) stores into the scratch buffer instead -- so the
// compiler's wait for any load issued before them is vmcnt(>= 5): a step's
// loads never wait for the previous step's obs stores to be acknowledged
// (gfx9 counts loads and stores in one in-order vmcnt; a path with fewer
// stores would merge into vmcnt(0) waits).
template <bool PC_, bool DFL = false>
__device__ __forceinline__ void wave_obs_flush(const Params &p, const uint32_t *wst, const float *tab, int kk,
                                               int wave_agent0, int nvalid, int lane, float &abl_sink, int bprio) {
    if (p.prio & 2) __builtin_amdgcn_s_setprio(kPrioFlush);
    // the wave's 16 staged obs rows: contiguous in [K][N][80]
    if (!(VN_ABLATE & 16u)) {
        const float4 *ws4 = reinterpret_cast<const float4 *>(wst);
        float4 *dst4 = reinterpret_cast<float4 *>(p.obs + ((size_t)kk * p.N + wave_agent0) * VN_OBS_DIM);
        if (DFL) dst4 = kk >= 0 ? dst4 : reinterpret_cast<float4 *>(p.scratch);   // (select, not a branch)
        if (VN_ABLATE & 256u)      // diagnostics: the same stores into a 1.3 MB (L2-resident) region
            dst4 = reinterpret_cast<float4 *>(p.obs) + (size_t)((wave_agent0 / 16) & 255) * 320;
        if constexpr (PC_) {
            // staged word f = float4 f of the wave's contiguous [16][80] rows: 1 KiB per store
#pragma unroll
            for (int jj = 0; jj < (64 / GROUP) * (VN_OBS_DIM / 4) / 64; ++jj) {
                const int f = lane + 64 * jj;
                if (VN_ABLATE & 2048u) {          // diagnostics: the stores without the LUT
                    const uint32_t wb = wst[f];
                    if (f < nvalid) obs_store(dst4 + f, make_float4(__uint_as_float(wb), 0.f, 0.f, 0.f));
                } else if (VN_ABLATE & 4096u) {   // diagnostics: the LUT without the stores
                    const float4 v = code_float4(wst[f], tab);
                    abl_sink += v.x + v.y + v.z + v.w;
                } else if (DFL || f < nvalid) {
                    obs_store(dst4 + f, code_float4(wst[f], tab));
                }
            }
        } else {
#pragma unroll
            for (int jj = 0; jj < (64 / GROUP) * (VN_OBS_DIM / 4) / 64; ++jj) {
                const int f = lane + 64 * jj;
                if (DFL || f < nvalid) obs_store(dst4 + f, ws4[f]);
            }
        }
    }
    // back to the base level: the deferred flush sits between the issue section and the
    // sensing; the in-step flush ends the step, and the next issue section follows at once
    if (DFL ? (p.prio & 2) : (p.prio & 3) == 2) vn_setprio(bprio);
}

#if VN_ENV_PROF || VN_ENV_WT
// the wave's start / end clocks and its HW_ID / XCC_ID (lane 0 of the wave)
__device__ __forceinline__ void wave_time_record(uint64_t rkern, uint64_t rend) {
    const unsigned wg = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wg < 8192u) {
        g_env_wt[2 * wg] = rkern;
        g_env_wt[2 * wg + 1] = rend;
        g_env_wid[2 * wg] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        g_env_wid[2 * wg + 1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
}
#endif

// BOX: the ray record computed from the agent's coordinates and its room's size
// (box_ray_rec, env_plan.h) instead of loaded: one vector load (16 distinct
// lines per wave instruction, L2 hits) less per step.  For envs whose every
// room vn_create has proven an exact box against the table (EnvLayout::box);
// plane-set step kernels only, without the deferred flush.  A separate
// instantiation the host picks (launch_ph): no runtime test in the step loop,
// and a general room's kernels are what they were.  DESIGN.md 7.20.
template <int PH, bool EXT, bool FAST, bool RESET_ONLY, int PCM, bool DFL = false, bool BOX = false>
__global__ __launch_bounds__((PCM == 1 || PCM == 2) ? VN_PC_BLOCK : BLOCK,
                             (PCM == 1 || PCM == 2) ? VN_PC_MIN_WAVES : VN_MIN_WAVES_PER_SIMD)
void env_kernel(Params p) {
    constexpr bool PC = PCM == 1 || PCM == 2;   // plane-set mode
    constexpr bool DM = PCM == 3;                // byte-mark mode, deferred plane marks
    static_assert(!BOX || (PC && !RESET_ONLY && !DFL), "BOX is for the plane-set step kernels, in-step flush");
    constexpr bool ARITH_REC = BOX || (VN_ABLATE & 8192u);   // (8192: diagnostics, the BOX path forced on any room)
    using RT = typename std::conditional<PCM == 2, uint32_t, uint64_t>::type;
    constexpr int kAgents = (PC ? VN_PC_BLOCK : BLOCK) / GROUP;
    constexpr bool CW = PC || DM;     // obs staged as code words (STAGE_WORDS), expanded at the flush
    static_assert(!CW || kAgents <= 64, "tc_slot has 64 obs[72] codes per block");
    __shared__ float tab[TAB_SIZE];
    __shared__ __attribute__((aligned(16))) uint64_t tiles[kAgents * TileGeom<PH>::STRIDE];
    // obs rows of the step, staged per wave (STAGE_WORDS) so HBM sees 1 KiB contiguous stores
    constexpr int kStageWords = CW ? STAGE_WORDS : STAGE_WORDS_F;
    __shared__ __attribute__((aligned(16))) uint32_t stage[(kAgents / 16) * kStageWords];
    __shared__ __attribute__((aligned(16))) RT psets[PC ? kAgents * PsetGeom<RT>::STRIDE : 2];
    constexpr bool SB = PCM == 2;
    __shared__ uint32_t stood_lds[SB ? kAgents * kStoodStride : 1];
#ifdef VN_LDS_PAD_U64            // diagnostics: occupancy at a larger LDS footprint
    __shared__ uint64_t lds_pad[VN_LDS_PAD_U64];
    if (p.N < 0) lds_pad[threadIdx.x] = 0ull;
    if (p.N < 0) p.obs[0] = (float)lds_pad[threadIdx.x ^ 1];
#endif
#if VN_ENV_PROF
    const uint64_t tkern = __builtin_amdgcn_s_memtime();
#endif
#if VN_ENV_PROF || VN_ENV_WT
    const uint64_t rkern = __builtin_amdgcn_s_memrealtime();
#endif
    const int q = threadIdx.x & (GROUP - 1);
    const int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) / GROUP);
    const bool active = i < p.N;
    const int ai = active ? i : 0;
    // the agent's state loads are in flight while the block stages its LUT
    const uint4 hot0 = p.hot[ai];
    uint32_t next_seed = p.next_seed[ai];
    const bool wvalid = hot0.x & HOT_WREC;   // the window record holds the start cell's window
    // the record loaded beside the state when the previous step launch wrote them (the host's bit)
    const bool wearly = !RESET_ONLY && (p.prio & PRIO_WREC_EARLY);
    WrecV<PH> wv;
    if (wearly) wrec_load<PH>(p, ai, q, wv);
    // SB: lane q's share of the stood rows (8q .. 8q + 7) and the nonzero-set masks.
    // A short launch (K <= 8) can only reach the rows y - 2 - K ..
    // y + 1 + K: the shares outside them are not loaded (they stay zero in LDS,
    // are never read, and are never written back -- a share is stored only when
    // one of its rows changed, and a reset rewrites all four).  The one-step
    // call reads 1-2 of the 4 shares instead of 128 B per agent.
    uint4 sr0 = make_uint4(0u, 0u, 0u, 0u), sr1 = sr0;
    uint2 nz0 = make_uint2(0u, 0u);
    const bool stood_all = p.K > 8;
    const uint4 *sp_share = reinterpret_cast<const uint4 *>(p.stood + (size_t)ai * 32u + 8u * (uint32_t)q);
    if (SB && !RESET_ONLY) {
        if (stood_all) {
            sr0 = sp_share[0];
            sr1 = sp_share[1];
        }
        nz0 = p.pnz[ai];
    }
    for (int k = threadIdx.x; k < TAB_SIZE; k += blockDim.x) tab[k < 256 ? tab_ix((uint32_t)k) : k] = p.lut[k];
    __syncthreads();
    // a wave without agents leaves (no block-wide barrier follows)
    // (wave-uniform: a scalar, so the flush's row block address costs no VGPR)
    const int wave_agent0 =
        __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + (threadIdx.x & ~63)) / GROUP));
    if (wave_agent0 >= p.N) return;

    uint64_t *tile = tiles + (threadIdx.x / GROUP) * TileGeom<PH>::STRIDE;
    Agent g = unpack(hot0);
    if (SB && !RESET_ONLY && !stood_all) {     // the shares this launch can reach (issued beside the room load)
        const int lo = g.y - 2 - p.K, hi = g.y + 1 + p.K;
        if (8 * q + 7 >= lo && 8 * q <= hi) {
            sr0 = sp_share[0];
            sr1 = sp_share[1];
        }
    }
    Room R = load_room(p, active ? g.room : 0);
    room_touch(R);
    int8_t *map = p.belief + (size_t)ai * p.agent_bytes;
    uint32_t dirty = 0;
    PlaneCache pc_;
    pc_.row = -1;
    pc_.w0 = 0;
    pc_.w[0] = pc_.w[1] = 0ull;
    PendMarks pend;                        // DM: the previous sensing pass's plane marks, not yet applied
    pend.valid = 0;
    RT *ps = psets + (PC ? (threadIdx.x / GROUP) * PsetGeom<RT>::STRIDE : 0);
    uint32_t pdirty = 0;
    Stood st;
    st.row = SB ? stood_lds + (threadIdx.x / GROUP) * kStoodStride : nullptr;
    st.xnz = nz0.x;
    st.ynz = nz0.y;
    st.chg = 0u;
    if (SB && !RESET_ONLY) {
        uint32_t *r = st.row + 8 * q;
        r[0] = sr0.x; r[1] = sr0.y; r[2] = sr0.z; r[3] = sr0.w;
        r[4] = sr1.x; r[5] = sr1.y; r[6] = sr1.z; r[7] = sr1.w;
        __builtin_amdgcn_wave_barrier();
    }

    if (RESET_ONLY) {
        const bool need = active && (p.mask == nullptr || p.mask[i] != 0);
        const uint32_t seed = need ? (uint32_t)p.seeds[i] : 0u;
        group_reset<PH, PC, RT, SB, DM>(p, map, tile, dirty, pc_, ps, pdirty, need, seed, g, R, tab,
                                        need ? p.obs + (size_t)i * VN_OBS_DIM : nullptr, nullptr, 0, q, st, pend);
        if (need) {
            if constexpr (DM) {
                pend_apply<PH>(p, map, pc_, pend, q);
            }
            tile_flush<PH>(p, map, tile, g, R, dirty, q);
            if (PC) pset_flush<RT, SB>(p, map, ps, g, R, pdirty, q, st);
            if (SB) {
                __builtin_amdgcn_wave_barrier();
                // lane q's share of the stood rows back to HBM (as in the epilogue below:
                // a shared helper compiles to a different schedule)
                const uint32_t *r = st.row + 8 * q;
                uint4 *sp = reinterpret_cast<uint4 *>(p.stood + (size_t)i * 32u + 8u * (uint32_t)q);
                sp[0] = make_uint4(r[0], r[1], r[2], r[3]);
                sp[1] = make_uint4(r[4], r[5], r[6], r[7]);
                if (q == 0) p.pnz[i] = make_uint2(st.xnz, st.ynz);
            }
            if (q == 0) {
                p.hot[i] = pack(g);
                p.next_seed[i] = seed + p.seed_stride;
            }
        }
        return;
    }

    // Step 0's move needs no memory: the hot state holds the move mask of the
    // agent's cell and the first action is the Philox draw (or p.actions[i]).
    // The window is filled around the cell after that move (the premove), so
    // the first step has no shift (one dependent load round trip less per
    // launch; a one-step launch has three left: state, window, the new cell's
    // ray record).  The move itself still runs in step 0 as usual.
    uint32_t a16[4] = {0u, 0u, 0u, 0u};          // the actions of the current 16-step chunk
    auto philox_chunk = [&](uint64_t tb) {
        // the agent index through an opaque copy: the compiler would otherwise
        // hoist the loop-invariant first Philox round out of the step loop and
        // keep (or spill) its 64-bit products across it
        int aio = ai;
        asm volatile("" : "+v"(aio));
        const uint4 o = philox4x32_10(p.policy_seed, p.gid_base + (uint64_t)aio, ((tb >> 2) & ~3ull) + (uint64_t)q);
        const uint32_t mine = __umulhi(o.x, 6u) | (__umulhi(o.y, 6u) << 8) | (__umulhi(o.z, 6u) << 16) |
                              (__umulhi(o.w, 6u) << 24);
        a16[0] = group_bcast<0>(mine);
        a16[1] = group_bcast<1>(mine);
        a16[2] = group_bcast<2>(mine);
        a16[3] = group_bcast<3>(mine);
    };
    if (!EXT) philox_chunk(p.t0);
    uint2 rec0 = make_uint2(0u, 0u);                // step 0's ray record, loaded with the fill
    if (active) {
        Agent gf = g;                               // the fill's window center
        if (p.K > 0) {
            int a;
            if (EXT) {
                a = p.actions[i];
            } else {
                const uint32_t w = a16[(uint32_t)(p.t0 >> 2) & 3u];
                a = (int)((w >> (8u * ((uint32_t)p.t0 & 3u))) & 0xffu);
            }
            const int dir = a < 4 ? (int)((kMoveDir >> (2 * (a * 4 + g.facing))) & 3u) : (a == 4) ? 4 : 5;
            if ((g.move_mask >> dir) & 1u) {
                gf.x += (dir == 0) - (dir == 1);
                gf.y += (dir == 2) - (dir == 3);
                gf.z += (dir == 4) - (dir == 5);
            }
            // step 0's ray record depends on the state alone: issued ahead of
            // the fill, so a one-step launch waits for one load round trip
            // after the state instead of two
            if (!ARITH_REC) {
                rec0 = p.rays[R.ray_off + (uint32_t)((gf.x * R.D + gf.y) * R.H + gf.z)];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (!(VN_ABLATE & 16384u)) {   // diagnostics: 16384 skips the launch's fill
            if (PC) pset_fill<RT, SB>(p, map, ps, gf, R, q, st);
            if (wvalid) {                          // the window record of the start cell (wrec_fill)
                if (!wearly) wrec_load<PH>(p, i, q, wv);
                wrec_fill<PH, PC, RT, SB>(p, map, tile, ps, g, gf, R, q, st, wv);
            } else {
                tile_fill<PH, PC, RT, SB>(p, map, tile, ps, gf, R, q, st);
            }
        }
    }
#if VN_ENV_PROF
    uint64_t eprof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t tprev = __builtin_amdgcn_s_memtime();
    const uint64_t tstart = tprev;
#endif
    uint32_t *wst = stage + (threadIdx.x >> 6) * kStageWords;   // this wave's staging block
    const int aslot = (threadIdx.x & 63) >> 2;
    float abl_sink = 0.f;                             // VN_ABLATE 4096 (diagnostics)

    const int lane = threadIdx.x & 63;
    const int nvalid = (p.N - wave_agent0) * (VN_OBS_DIM / 4);       // float4s of the wave's agents (> 0)
    // the step's outputs stored within the step (measured faster than the
    // deferred order, which also needs more VGPRs than the byte-mark kernels
    // have at 4 waves/SIMD)
    //
    // Work striped over the agent's 4 lanes instead of repeated by each:
    //  * Philox: lane q computes the 4-step block cb + q of the
    //    16-step chunk cb..cb+3, so one call per lane covers 16 steps; the
    //    four words are broadcast in the quad;
    //  * the rollout-buffer call (FAST): each step records
    //    its reward events (12 bits) and after the 4-step block lane q
    //    evaluates step q's f64 reward and stores its reward / terminated /
    //    truncated (one store instruction per output per block).
    constexpr bool STRIPE_R = FAST;
    // the wave's obs flush of launch step kk (staged rows -> [K][N][80]); with
    // p.dflush (full waves) step k's rows go out after step k + 1's loads are
    // issued, so those loads do not queue behind them (one in-order vmcnt)
    // (byte-mark kernels only: in the plane-set kernels the deferred path cost 11 spilled VGPRs)
    // Paired A/B (profiles/r05/ab_dflush_paired.log): P3 / P2 +0.9 / +0.7 % at 128-step
    // launches, +0.7 % at 20, -0.3 % one-step (so multi-step launches only).
    // A base priority that rotates over the 4 blocks sharing a CU (blocks b,
    // b + grid/4, ... are dispatched to the same CU, oldest first): the SIMD
    // arbiter favours older waves, so without it the CU's 4 blocks finished in
    // dispatch order, 112 / 118 / 125 / 135 us (p50) in the driver's 20-step
    // launch, and the youngest set the launch's end; rotating the base level
    // every 4 steps brings them to 128 / 127 / 122 / 128 (scripts/env_wt.py,
    // profiles/r05/env_wave_times_rotating.log).  Paired A/B
    // (profiles/r05/ab_rotating_prio_paired.log): box +3.0 % (20-step) /
    // +1.5 % (128-step); the byte-mark kernels -0.5 %, so plane-set only.
    // That rotation is open-loop (VnTuning::prio bit 2 still selects it); the
    // default takes the level from the progress of the SIMD's waves instead
    // (wave_progress above).  The host folds "bit 6, a launch of
    // >= 8 steps" into PRIO_BASE.
    const bool steer = PC && (p.prio & PRIO_BASE) && !(p.prio & PRIO_ROTATE);
    // (neither mode keeps a scalar across the step loop for this: the dispatch rank and the
    // wave's table index are worked out where they are used, once per 4-step block)
    auto base_prio = [&](int kk) -> int {
        if (!(PC && (p.prio & PRIO_BASE) && (p.prio & PRIO_ROTATE))) return 0;
        const int drank = (int)(blockIdx.x / max(1u, gridDim.x / 4u));
        return min((drank + (kk >> 2)) & 3, 2);
    };
    int bprio = base_prio(0);
    if (bprio) vn_setprio(bprio);
    auto progress_word = [&](int kk) -> uint32_t {   // launch tag << 8 | blocks completed before step kk
        return (((uint32_t)p.prio >> PRIO_TAG_SHIFT) << 8) | (uint32_t)min((kk + 3) >> 2, 255);
    };
    // DFL: chosen by the host (launch_ph: VnTuning::dflush, launches of more
    // than one step, every wave full); a separate instantiation, so the
    // waits of the loop see the same five flush stores on every path
    static_assert(!DFL || (!RESET_ONLY && (DM || PC)), "the deferred flush is for step launches of DM / PC kernels");
    for (int k = 0; k < p.K;) {
        const uint64_t tb = p.t0 + (uint64_t)k;
        uint32_t acts = 0;                                    // 4 actions, 8 bits each, by (t & 3)
        if (!EXT) {
            if (k != 0 && (tb & 15u) == 0u) philox_chunk(tb);   // k == 0: the prologue's chunk
            const uint32_t sel = (uint32_t)(tb >> 2) & 3u;
            acts = sel == 0u ? a16[0] : sel == 1u ? a16[1] : sel == 2u ? a16[2] : a16[3];
        }
        if (PC && (p.prio & PRIO_BASE) && (p.prio & PRIO_ROTATE)) {   // the rotating base level, every 4-step block
            bprio = base_prio(k);
            vn_setprio(bprio);
        }                                    // (the closed loop's level: set at the previous block's end)
        const int jn = (4 - (int)(tb & 3u)) < (p.K - k) ? (4 - (int)(tb & 3u)) : (p.K - k);
        uint64_t ev4 = 0;                                     // STRIPE_R: reward events by slot (t & 3), 16 bits each
        const int kb = k;
        for (int j = 0; j < jn; ++j, ++k) {
            bool finished = false, was_done = false;   // was_done: `done` entering the step (the no-auto-reset latch)
            const size_t row = (size_t)k * (size_t)p.N + (size_t)i;
            const uint64_t tt = tb + (uint64_t)j;
            if (active) {
                // DM: the previous step's plane marks, before this step's tile shift reads the entering column
                if constexpr (DM) {
                    if (!(VN_ABLATE & 1048576u)) pend_apply<PH>(p, map, pc_, pend, q);   // diagnostics: skipped
                }
                const int a = EXT ? p.actions[row] : (int)((acts >> (8 * (uint32_t)(tt & 3u))) & 0xffu);
                if (!FAST && p.actions_out && q == 0) p.actions_out[row] = a;

                // step() prologue (:111-116)
                if (p.prio & 1) __builtin_amdgcn_s_setprio(kPrioIssue);
                if (g.near_wall) {
                    g.was_near_wall = true;
                    g.near_wall = false;
                }
                if (g.step_count < 0xffffffu) ++g.step_count;
                const bool truncated = g.step_count >= R.total_free;

                // do_action (:134-166): relative move table by facing -> axis dir
                int dir;
                if (a < 4) {
                    dir = (int)((kMoveDir >> (2 * (a * 4 + g.facing))) & 3u);
                    g.facing = (int)((0x8Du >> (2 * dir)) & 3u);
                } else {
                    dir = (a == 4) ? 4 : 5;
                }
                const bool moved = (g.move_mask >> dir) & 1u;
                if (moved) {
                    g.x += (dir == 0) - (dir == 1);
                    g.y += (dir == 2) - (dir == 3);
                    g.z += (dir == 4) - (dir == 5);
                }
                // the step's loads, all in flight together: entering window
                // column (and plane set), the new cell's ray record, its plane rows
                // (the premove: the launch's window was filled around step 0's cell;
                // `!(k == 0)`, since `k != 0` compiles four kernels differently: DESIGN.md 7.17)
                const bool shifted = moved && dir < 4 && !(k == 0);
                ShiftLoad<PH> sl;
                SetLoad<RT> pl;
                if (shifted) tile_shift_issue<PH, SB>(p, map, tile, dir, g.x, g.y, R, dirty, q, sl, st, g.room);
                if (PC && shifted) pset_shift_issue<RT, SB>(p, map, ps, dir, g.x, g.y, R, pdirty, q, pl, st);
                uint2 rec;
                // BOX: the record of an exact box, from the agent's own room's size (step 0's too)
                if (ARITH_REC) {
                    const RayRec b = box_ray_rec(R.W, R.D, R.H, g.x, g.y, g.z);
                    rec = make_uint2(b.x, b.y);
                } else if (k == 0) {
                    rec = rec0;
                } else {
                    rec = p.rays[R.ray_off + (uint32_t)((g.x * R.D + g.y) * R.H + g.z)];
                }
                if (!PC) plane_prefetch<PH>(p, map, pc_, g.x, g.y, g.z, q);
                // (the deferred flush follows at its own level and restores the base level)
                if ((p.prio & 1) && !(DFL && (p.prio & 2))) vn_setprio(bprio);
                // the previous step's rows, behind this step's loads (k == 0: into scratch);
                // the compiler barrier keeps the loads above (the plane rows' conditional
                // block included) ahead of the five stores
                if constexpr (DFL) {
                    asm volatile("" ::: "memory");
                    wave_obs_flush<CW, true>(p, wst, tab, k - 1, wave_agent0, nvalid, lane, abl_sink, bprio);
                }
                ENV_T(0);
                if (shifted) {
                    if constexpr (PC) {
                        pdirty = pset_shift_commit(ps, pl, pdirty, q);
                        if (sl.in) sl.c.w[0] |= pset_known(ps, sl.ex, sl.ey);
                    }
                    dirty = tile_shift_commit<PH>(tile, sl, dirty);
                }
                if (SB && moved && dir < 4 && q == 0) {       // the agent's new column: stood in
                    const uint32_t o = st.row[g.y], b = 1u << g.x;
                    if (!(o & b)) {
                        st.row[g.y] = o | b;
                        st.chg |= 1u << (g.y >> 3);
                    }
                }
                ENV_T(1);

                bool explored = false;
                const ObsDst dst{p.obs + row * VN_OBS_DIM,
                                 p.terminal_obs ? p.terminal_obs + row * VN_OBS_DIM : nullptr, wst,
                                 p.autoreset != 0, truncated, aslot};
                const int vv = sense_observe<PH, false, PC, RT, DM>(p, map, tile, dirty, pc_, ps, pdirty, g, R,
                                                                    moved, explored, tab, dst, rec, q, pend, k == 0);
                ENV_T(2);

                if constexpr (STRIPE_R) {
                    // the reward's inputs (reward_events), the state updates in place
                    uint32_t ev = (uint32_t)(vv < 25 ? vv : 25) | (moved ? 32u : 0u);
                    if (!moved) {
                        g.last_bump = true;
                        if (g.bumps < 0x3ffffffu) ++g.bumps;
                    } else {
                        g.last_bump = false;
                        if (g.was_near_wall) {
                            g.was_near_wall = false;
                            ev |= 64u;
                        }
                        if (g.last_action != 2 && a == g.last_action && g.last_action < 4) ev |= 128u;
                        if (g.last_action == 2 && a == 2) ev |= 256u;
                    }
                    if (explored) ev |= 512u;
                    was_done = g.done;
                    if (g.visited >= R.finish_visits) {        // visited / total >= 0.84 (:212-215)
                        g.done = true;
                        ev |= 1024u;
                    }
                    if (truncated) ev |= 2048u;
                    g.last_action = a;
                    ev4 |= (uint64_t)ev << (16u * ((uint32_t)tt & 3u));
                    finished = g.done || truncated;
                } else {
                    // compute_reward (:169-224), f64 in the reference's order
                    double r = -0.05;
                    const double pen = (double)vv * 0.02;
                    r -= (0.5 < pen) ? 0.5 : pen;
                    if (!moved) {
                        g.last_bump = true;
                        if (g.bumps < 0x3ffffffu) ++g.bumps;
                        r += p.crash_penalty;
                    } else {
                        g.last_bump = false;
                        if (g.was_near_wall) {
                            g.was_near_wall = false;
                            r += 0.15;
                        }
                        if (g.last_action != 2 && a == g.last_action && g.last_action < 4) r += 0.05;
                        if (g.last_action == 2 && a == 2) r -= 0.5;
                    }
                    if (explored) r += 1.0;
                    was_done = g.done;
                    if (g.visited >= R.finish_visits) {            // visited / total >= 0.84 (:212-215)
                        g.done = true;
                        r += 100.0;
                    }
                    if (truncated) r += -5.0;
                    g.last_action = a;

                    if (q == 0 && !(VN_ABLATE & 128u)) {
                        if (FAST || p.reward) p.reward[row] = (float)r;
                        if (p.reward64) p.reward64[row] = r;
                        if (FAST || p.term) p.term[row] = g.done ? 1 : 0;
                        if (FAST || p.trunc) p.trunc[row] = truncated ? 1 : 0;
                    }
                    finished = g.done || truncated;
                }
            }
            ENV_T(3);
            // an episode ends: with auto-reset at every finished step; without it at the first
            // one after a reset only (an agent stepped on after its end entered the step with
            // done set or step_count at max_steps, and records nothing more).  One rare branch
            // for both: the record's read-modify-write, then the auto-reset.
            const bool ends = finished && (p.autoreset || (!was_done && g.step_count - 1u < R.total_free));
            if (__ballot(ends)) {
                // the ended episode's record, from the state the step left (before the reset below)
                if (ends && q == 0)
                    episode_end(p.envc, i, g.step_count, g.bumps, g.visited, R.total_free, (uint32_t)g.room,
                                (g.done ? EP_TERMINATED : 0u) | (g.step_count >= R.total_free ? EP_TRUNCATED : 0u));
                const bool need = ends && p.autoreset;
                const uint32_t seed = next_seed;
                group_reset<PH, PC, RT, SB, DM>(p, map, tile, dirty, pc_, ps, pdirty, need, seed, g, R, tab,
                                                need ? p.obs + row * VN_OBS_DIM : nullptr, wst, aslot, q, st, pend);
                if (need) next_seed = seed + p.seed_stride;
            }
            ENV_T(4);
            if constexpr (!DFL) wave_obs_flush<CW>(p, wst, tab, k, wave_agent0, nvalid, lane, abl_sink, bprio);
            ENV_T(5);
        }
        if constexpr (STRIPE_R) {
            // lane q: the reward of slot q of the block (steps kb .. kb + jn - 1
            // are slots s0 .. s0 + jn - 1)
            const int s0 = (int)(tb & 3u);
            if (active && q >= s0 && q < s0 + jn && !(VN_ABLATE & 128u)) {
                const uint32_t ev = (uint32_t)(ev4 >> (16 * q)) & 0xffffu;
                const double r = reward_of_events(ev, p.crash_penalty);
                const size_t o = (size_t)(kb + q - s0) * (size_t)p.N + (size_t)i;
                if (VN_ABLATE & 262144u) {          // diagnostics: the block's rewards computed, not stored
                    abl_sink += (float)r + (float)ev;
                } else if (VN_ABLATE & 524288u) {   // diagnostics: the same stores into p.scratch (L2)
                    p.scratch[lane] = (float)r;
                    reinterpret_cast<uint8_t *>(p.scratch + 64)[lane] = (uint8_t)((ev >> 10) & 1u);
                    reinterpret_cast<uint8_t *>(p.scratch + 96)[lane] = (uint8_t)(ev >> 11);
                } else {
                    p.reward[o] = (float)r;
                    if (p.reward64) p.reward64[o] = r;       // the Monitor's exact f64 reward (once per 4-step block)
                    p.term[o] = (uint8_t)((ev >> 10) & 1u);
                    p.trunc[o] = (uint8_t)(ev >> 11);
                }
            }
            ENV_T(6);
        }
        // the next block's base level: the SIMD's waves of this launch that completed this block
        // before this wave did (the next step's issue section applies it); then the wave's own
        // progress word, behind the block's output stores
        if (PC && steer && k < p.K) {   // another block follows
            bprio = wave_progress_level(wave_progress_row(wave_progress_index()), progress_word(k));
            if (!(p.prio & 1)) vn_setprio(bprio);
        }
        if (PC && steer && lane == 0)
            __hip_atomic_store(&g_wave_progress[wave_progress_index()], k < p.K ? progress_word(k) : 0u,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (0: a finished wave is nobody's mate)
    }
    // the launch's last step's rows
    if constexpr (DFL) wave_obs_flush<CW, true>(p, wst, tab, p.K - 1, wave_agent0, nvalid, lane, abl_sink, bprio);
    if (active) {
        if constexpr (DM) {
            pend_apply<PH>(p, map, pc_, pend, q);   // the last step's deferred marks
        }
        if (!(VN_ABLATE & 32768u)) {   // diagnostics: 32768 skips the launch's flush
            tile_flush<PH>(p, map, tile, g, R, dirty, q);
            if (PC) pset_flush<RT, SB>(p, map, ps, g, R, pdirty, q, st);
        }
        const bool wsave = p.prio & PRIO_WREC_SAVE;   // the window record for the next launch (host: K <= wrec_k)
        if (q == 0) {
            uint4 h = pack(g);
            if (wsave) h.x |= HOT_WREC;
            p.hot[i] = h;
            p.next_seed[i] = next_seed;
        }
        if (wsave) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the slots other lanes wrote
            wrec_store<PH>(p, tile, i, q);
        }
    }
    if (SB) {
        const uint32_t c = group_or(st.chg);
        __builtin_amdgcn_wave_barrier();
        if (active && ((c >> q) & 1u)) {     // lane q's share, if one of its rows changed
            const uint32_t *r = st.row + 8 * q;
            uint4 *sp = reinterpret_cast<uint4 *>(p.stood + (size_t)i * 32u + 8u * (uint32_t)q);
            sp[0] = make_uint4(r[0], r[1], r[2], r[3]);
            sp[1] = make_uint4(r[4], r[5], r[6], r[7]);
        }
        if (active && q == 0) p.pnz[i] = make_uint2(st.xnz, st.ynz);   // (8 B; no compare: no register held)
    }
    if ((VN_ABLATE & (4096u | 262144u)) && abl_sink == 12345.f) p.obs[0] = abl_sink;
#if VN_ENV_PROF
    if (FAST && (threadIdx.x & 63) == 0) {
        __builtin_amdgcn_s_waitcnt(0);   // the flush's stores issued and retired
        const uint64_t tend = __builtin_amdgcn_s_memtime();
        const uint64_t rend = __builtin_amdgcn_s_memrealtime();   // before the profile's own atomics
        for (int k = 0; k < 7; ++k) atomicAdd(&g_env_prof[k], (unsigned long long)eprof[k]);
        atomicAdd(&g_env_prof[7], (unsigned long long)(tprev - tstart));
        atomicAdd(&g_env_prof[8], 1ull);
        atomicAdd(&g_env_prof[9], (unsigned long long)(tstart - tkern));   // prologue: LUT, state, fill
        atomicAdd(&g_env_prof[10], (unsigned long long)(tend - tprev));    // epilogue: flush, state
        atomicMax(&g_env_prof[11], (unsigned long long)(tend - tkern));    // longest wave
        wave_time_record(rkern, rend);
    }
#elif VN_ENV_WT
    if (FAST && (threadIdx.x & 63) == 0) {
        __builtin_amdgcn_s_waitcnt(0);   // the wave's stores retired
        const uint64_t rend = __builtin_amdgcn_s_memrealtime();
        wave_time_record(rkern, rend);
    }
#endif
}

// ----------------------------------------------------------------------------
// exports (parity dumps)
// ----------------------------------------------------------------------------
__global__ void export_state_kernel(Params p, int64_t *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.N) return;
    const Agent g = unpack(p.hot[i]);
    const Room R = load_room(p, g.room);
    int64_t *o = out + (size_t)i * VN_STATE_FIELDS;
    o[0] = g.x; o[1] = g.y; o[2] = g.z; o[3] = g.facing; o[4] = g.last_action;
    o[5] = g.step_count; o[6] = g.visited; o[7] = g.bumps;
    o[8] = g.done; o[9] = g.last_bump; o[10] = g.near_wall; o[11] = g.was_near_wall;
    o[12] = g.cid; o[13] = g.room; o[14] = R.total_free; o[15] = p.next_seed[i];
    if (p.variant == VN_VARIANT_SIMPLE) {
        const uint32_t gl = p.goal[i];
        o[9] = gl & 0xff; o[10] = (gl >> 8) & 0xff; o[11] = (gl >> 16) & 0xff; o[12] = 0;
    }
}

__global__ void export_belief_kernel(Params p, int8_t *out, int pw, int pd) {
    const size_t cells = (size_t)pw * pd * p.ph;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= cells * (size_t)p.N) return;
    const int i = (int)(gid / cells);
    const size_t c = gid - (size_t)i * cells;
    const int z = (int)(c % p.ph), y = (int)((c / p.ph) % pd), x = (int)(c / ((size_t)p.ph * pd));
    const Agent g = unpack(p.hot[i]);
    const Room R = load_room(p, g.room);
    int8_t v = -128;
    if (x < R.W && y < R.D && z < R.H) {
        const uint32_t off = bcol(x, y, p.nby) * (uint32_t)p.ph + (uint32_t)z;
        const int8_t *m = p.belief + (size_t)i * p.agent_bytes;
        const uint32_t b = (uint8_t)m[off];
        // a cell is known if its byte says so or a marked-bit plane holds it
        // (plane-set mode records marks outside the window only there)
        uint64_t xr, yr;
        if (p.pcache == 2) {           // u32 plane rows (PsetGeom)
            xr = reinterpret_cast<const uint32_t *>(m + p.xp_off)[(size_t)(y * p.ph + z)];
            yr = reinterpret_cast<const uint32_t *>(m + p.yp_off)[(size_t)(x * p.ph + z)];
        } else {
            xr = reinterpret_cast<const uint64_t *>(m + p.xp_off)[(size_t)(y * p.ph + z) * p.nwx + (x >> 6)];
            yr = reinterpret_cast<const uint64_t *>(m + p.yp_off)[(size_t)(x * p.ph + z) * p.nwy + (y >> 6)];
        }
        const bool known = (b & KNOWN) || ((xr >> (x & 63)) & 1ull) || ((yr >> (y & 63)) & 1ull);
        v = known ? ((b & 0x40u) ? (int8_t)-2 : (int8_t)(b & 0x3fu)) : (int8_t)-1;
    }
    out[gid] = v;
}

// ----------------------------------------------------------------------------
// GAE (SB3 RolloutBuffer.compute_returns_and_advantage), one lane per env,
// reverse scan over T; f32 in numpy's evaluation order, no contraction.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gae_kernel(const float *__restrict__ rew, const float *__restrict__ val,
                                                  const float *__restrict__ starts, const float *__restrict__ last_v,
                                                  const float *__restrict__ dones, int T, int N, float g32, float gl32,
                                                  float *__restrict__ adv, float *__restrict__ ret) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float last = 0.0f;
    float nv = last_v[i];
    float nnt = 1.0f - dones[i];
    for (int t = T - 1; t >= 0; --t) {
        const size_t o = (size_t)t * N + i;
        const float v = val[o];
        const float r = rew[o];
        const float s = (t > 0) ? starts[o] : 0.0f;  // episode_starts[t] feeds step t-1
        const float gv = g32 * nv;
        const float gvn = gv * nnt;
        const float sum = r + gvn;
        const float delta = sum - v;
        const float glnn = gl32 * nnt;
        const float carry = glnn * last;
        last = delta + carry;
        adv[o] = last;
        ret[o] = last + v;
        nv = v;
        nnt = 1.0f - s;
    }
}

// ============================================================================
// host side: which kernel a CubicEnv call launches (vn_cubic, env_params.h)
// ============================================================================

// The deferred obs flush (env_kernel's DFL): step launches of more than one
// step with every wave full, in the kernel modes VnTuning::dflush enables
// (bit 0: byte marks, PCM 3; bit 1: plane sets, PCM 1 / 2).
constexpr bool pcm_dfl_capable(int pcm) { return pcm == 1 || pcm == 2 || pcm == 3; }
static bool use_dfl(int pcm, int N, int K, int dflush_bits) {
    if (!pcm_dfl_capable(pcm) || K <= 1 || N % (64 / GROUP) != 0) return false;
    return (pcm == 3) ? (dflush_bits & 1) != 0 : (dflush_bits & 2) != 0;
}

// The arithmetic ray record (env_kernel's BOX): step launches of a box-exact
// env (Params::box, proven by vn_create) in the plane-set modes, unless the
// call's VnTuning::prio bit 3 asks for the table kernels; the deferred-flush
// instantiation stays on the table (the caller tests that).
constexpr bool pcm_box_capable(int pcm) { return pcm == 1 || pcm == 2; }
static bool use_box(int pcm, const Params &p) { return pcm_box_capable(pcm) && p.box && !(p.prio & PRIO_TABLE); }

template <int PH, bool RESET_ONLY, int PCM>
int launch_ph(int N, hipStream_t s, const Params &p) {
    const int bs = (PCM == 1 || PCM == 2) ? VN_PC_BLOCK : BLOCK;
    const dim3 block((unsigned)bs);
    const dim3 grid((unsigned)(((size_t)N * GROUP + bs - 1) / bs));
    // FAST: the rollout-buffer call (f32 reward, flags; the f64 reward for the
    // Monitor optional, stored once per 4-step block); no action record
    const bool fast = p.reward && p.term && p.trunc && !p.actions_out;
    constexpr bool CAP = pcm_dfl_capable(PCM);
    const bool dfl = CAP && !RESET_ONLY && use_dfl(PCM, N, p.K, p.dflush);
    // (BCAP false: the names below are the table instantiations themselves)
    constexpr bool BCAP = pcm_box_capable(PCM) && !RESET_ONLY;
    const bool box = BCAP && use_box(PCM, p);
    if (RESET_ONLY)
        hipLaunchKernelGGL((env_kernel<PH, false, false, true, PCM>), grid, block, 0, s, p);
    else if (box && p.actions && fast)
        hipLaunchKernelGGL((env_kernel<PH, true, true, false, PCM, false, BCAP>), grid, block, 0, s, p);
    else if (box && p.actions)
        hipLaunchKernelGGL((env_kernel<PH, true, false, false, PCM, false, BCAP>), grid, block, 0, s, p);
    else if (box && fast && !dfl)
        hipLaunchKernelGGL((env_kernel<PH, false, true, false, PCM, false, BCAP>), grid, block, 0, s, p);
    else if (box && !dfl)
        hipLaunchKernelGGL((env_kernel<PH, false, false, false, PCM, false, BCAP>), grid, block, 0, s, p);
    else if (p.actions && fast)
        hipLaunchKernelGGL((env_kernel<PH, true, true, false, PCM>), grid, block, 0, s, p);
    else if (p.actions)
        hipLaunchKernelGGL((env_kernel<PH, true, false, false, PCM>), grid, block, 0, s, p);
    else if (fast && dfl)
        hipLaunchKernelGGL((env_kernel<PH, false, true, false, PCM, CAP>), grid, block, 0, s, p);
    else if (fast)
        hipLaunchKernelGGL((env_kernel<PH, false, true, false, PCM>), grid, block, 0, s, p);
    else if (dfl)
        hipLaunchKernelGGL((env_kernel<PH, false, false, false, PCM, CAP>), grid, block, 0, s, p);
    else
        hipLaunchKernelGGL((env_kernel<PH, false, false, false, PCM>), grid, block, 0, s, p);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

// The kernel mode of a CubicEnv: PCM 1/2 plane sets (PH 8, EnvLayout::pcache),
// PCM 3 byte marks with deferred plane marks (rows of <= 2 words, EnvLayout::defer),
// else PCM 0.
static int env_pcm(int ph, int pcache, int defer) {
    if (ph == 8 && pcache) return pcache;
    return defer ? 3 : 0;
}

template <bool RESET_ONLY>
int launch_pcm(int pcm, const Params &p, hipStream_t s) {
    if (p.ph == 8) {
        if (pcm == 2) return launch_ph<8, RESET_ONLY, 2>(p.N, s, p);
        if (pcm == 1) return launch_ph<8, RESET_ONLY, 1>(p.N, s, p);
        if (pcm == 3) return launch_ph<8, RESET_ONLY, 3>(p.N, s, p);
        return launch_ph<8, RESET_ONLY, 0>(p.N, s, p);
    }
    if (p.ph == 16)
        return pcm == 3 ? launch_ph<16, RESET_ONLY, 3>(p.N, s, p) : launch_ph<16, RESET_ONLY, 0>(p.N, s, p);
    return pcm == 3 ? launch_ph<32, RESET_ONLY, 3>(p.N, s, p) : launch_ph<32, RESET_ONLY, 0>(p.N, s, p);
}

}  // namespace

namespace vn_cubic {

int ensure_mt(int device) { return ensure_mt_table(device); }

int launch(bool reset_only, int defer, int wrec_early, bool *wrec_written, const void *params, hipStream_t s) {
    Params p = *static_cast<const Params *>(params);
    const int pcm = env_pcm(p.ph, p.pcache, defer);
    if (reset_only) {
        *wrec_written = false;
        return launch_pcm<true>(pcm, p, s);
    }
    // the window records (wrec_fill): written by step launches of at most
    // wrec_k steps, loaded beside the state when the previous launch wrote them
    // (VnTuning::wrec_early: instead of after it, one dependent round trip less)
    if (p.K <= p.wrec_k) p.prio |= PRIO_WREC_SAVE;
    if (*wrec_written && wrec_early) p.prio |= PRIO_WREC_EARLY;
    *wrec_written = p.K <= p.wrec_k;
    // the base level (VnTuning::prio bit 6): plane-set kernels, launches of >= 8 steps; the closed
    // loop's table tells launches apart by a tag, a process-wide launch count
    if ((p.prio & 64) && p.K >= 8 && (pcm == 1 || pcm == 2)) {
        static std::atomic<uint32_t> launches{0};
        p.prio |= PRIO_BASE | (int)((launches.fetch_add(1u) + 1u) << PRIO_TAG_SHIFT);
    }
    return launch_pcm<false>(pcm, p, s);
}

// The kernel instantiation launch picks for a call shape of p.K steps
// (diagnostics / bench labels); kept next to launch so the two selections agree.
// The name stops at the DFL argument; *box (when given): whether the call
// launches that name's BOX instantiation (the ray record computed).
std::string label(bool reset_only, bool ext, bool fast, int defer, const void *params, bool *box) {
    const Params &p = *static_cast<const Params *>(params);
    char buf[160];
    const int pcm = env_pcm(p.ph, p.pcache, defer);
    const bool x = !reset_only && ext, f = !reset_only && fast;
    const bool dfl = !reset_only && !x && use_dfl(pcm, p.N, p.K, p.dflush);
    if (box) *box = !reset_only && !dfl && use_box(pcm, p);
    std::snprintf(buf, sizeof(buf), "env_kernel<%d, %s, %s, %s, %d%s>", p.ph, x ? "true" : "false",
                  f ? "true" : "false", reset_only ? "true" : "false", pcm, dfl ? ", true" : "");
    return buf;
}

int export_state(const void *params, int64_t *out, hipStream_t s) {
    const Params &p = *static_cast<const Params *>(params);
    hipLaunchKernelGGL(export_state_kernel, dim3((unsigned)((p.N + 255) / 256)), dim3(256), 0, s, p, out);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int export_belief(const void *params, int8_t *out, int pw, int pd, hipStream_t s) {
    const Params &p = *static_cast<const Params *>(params);
    const size_t total = (size_t)p.N * pw * pd * p.ph;
    hipLaunchKernelGGL(export_belief_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, out, pw, pd);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int gae(const float *rew, const float *val, const float *starts, const float *last_v, const float *dones, int T, int N,
        float g32, float gl32, float *adv, float *ret, hipStream_t s) {
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, rew, val, starts, last_v, dones,
                       T, N, g32, gl32, adv, ret);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace vn_cubic

// diagnostics builds: the profiling exports stay with the device symbols they read
#if VN_ENV_PROF || VN_ENV_WT
// the per-wave start / end clocks and ids of the last profiled launch
extern "C" int vn_debug_env_wavetimes(unsigned long long *t, unsigned int *ids) {
    VN_HIP(hipMemcpyFromSymbol(t, HIP_SYMBOL(g_env_wt), sizeof(unsigned long long) * 8192 * 2));
    VN_HIP(hipMemcpyFromSymbol(ids, HIP_SYMBOL(g_env_wid), sizeof(unsigned int) * 8192 * 2));
    return 0;
}
#endif
#if VN_ENV_PROF
extern "C" int vn_debug_env_prof(unsigned long long *out16, int clear) {
    VN_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_env_prof), sizeof(unsigned long long) * 16));
    if (clear) {
        unsigned long long z[16] = {0};
        VN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_env_prof), z, sizeof(z)));
    }
    return 0;
}
#endif
