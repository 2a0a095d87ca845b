// env_params.h -- what the host side of the env boundary (voxnav_api.hip)
// hands the two kernel units: the launch parameters (Params), the
// env-constant block the reset path reads from device memory (EnvConst), and
// the units' host interfaces (vn_cubic: voxnav_env.hip, vn_simple:
// voxnav_simple.hip, vn_state: voxnav_state.hip, vn_episode: voxnav_episode.hip,
// vn_gather: voxnav_gather.hip, vn_plan: voxnav_plan.hip).  No device code and no
// device symbol.  The structs are
// in an anonymous namespace: each unit has its own (identical) copy, so
// Params crosses the unit boundary as a pointer.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace {

// Env-constant values the (rare, out-of-line) reset path reads from device
// memory, so they need not stay live in SGPRs across the step loop.
struct EnvConst {
    const uint4 *rooms;
    const uint2 *rays;
    const uint32_t *starts;
    int32_t *err;
    int n_rooms, use_room_draw, nby, pcache;
    uint32_t agent_bytes, xp_off, map_bytes, plane_bytes;   // plane_bytes: the planes a reset clears
    const uint4 *wimg;       // plane-set mode: per room, the bricked map with latent wall bits
    uint4 *episodes;         // per agent one EpisodeRec (env_plan.h), 4 x 16 B; here and not in Params: read at episode ends only
};

struct Params {
    const EnvConst *envc;
    uint4 *hot;
    uint32_t *next_seed;
    int8_t *belief;
    const uint4 *rooms;
    const uint2 *rays;
    const uint32_t *starts;
    const float *lut;
    int32_t *err;
    int N, L, nby, ph;
    uint32_t map_bytes;      // byte map (bricked) per agent
    uint32_t agent_bytes;    // stride: byte map + x-plane + y-plane
    uint32_t xp_off, yp_off; // plane offsets inside the agent block
    int nwx, nwy;            // u64 words per plane row
    int n_rooms, use_room_draw, autoreset;
    uint32_t seed_stride;
    double crash_penalty, finish;
    uint64_t gid_base;
    // per call
    int K;
    const int32_t *actions;  // NULL -> Philox random policy
    uint64_t policy_seed, t0;
    int32_t *actions_out;
    float *obs, *reward, *terminal_obs;
    double *reward64;
    uint8_t *term, *trunc;
    const int64_t *seeds;    // reset-only launches
    const uint8_t *mask;
    uint32_t box;            // every room of the set is an exact box (EnvLayout::box): vn_cubic::launch may pick the
                             // BOX kernels, whose ray record is arithmetic (no kernel reads this field)
    int prio;                // step kernel: issue priority (bits, VnTuning::prio; default 67); vn_cubic::launch adds
                             // its own bits above them (window record, base level, bits 12..31 the launch's tag)
    int dflush;              // step kernel: a step's obs flush after the next step's load issue (VnTuning::dflush)
    // simpleEnv variant
    int variant, obs_dim, pd;
    uint32_t *goal;          // per agent gx | gy<<8 | gz<<16
    uint4 *predraw;          // simpleEnv: per agent a reset draw computed ahead {start|room<<24, goal, seed, valid}
    int sbits;               // simpleEnv bit-plane layout (rooms up to 64 x 64 x 31)
    uint32_t sy_off, sz_off, qz_off;
    int sline;               // simpleEnv line layout (rooms up to 32 x 32 x 8; simple_line_kernel)
    const int8_t *wimg;      // plane-set mode (CubicEnv, PH 8, rooms <= 64 x 64): latent-wall room images
    int pcache;
    float *scratch;          // 4 KiB: targets of inactive lanes' output stores
    uint32_t *stood;         // plane-set mode PCM 2: per agent 32 words, stood-column rows (bit x of row y)
    uint2 *pnz;              // ... and per agent the plane sets whose HBM copy may be nonzero (x: rows y', y: cols x')
    int wrec_k;              // step launches of at most wrec_k steps write the window record (VnTuning::wrec_k);
                             // the records follow the hot state in its allocation (wrec_base)
};

}  // namespace

// The CubicEnv unit (voxnav_env.hip).  `params` is a complete Params of the
// call; the kernel mode comes from its ph / pcache and `defer` (EnvLayout).
namespace vn_cubic {
int ensure_mt(int device);
// *wrec_written: whether the env's previous step launch wrote the window
// records; updated for this launch (wrec_early: VnTuning::wrec_early)
int launch(bool reset_only, int defer, int wrec_early, bool *wrec_written, const void *params, hipStream_t s);
std::string label(bool reset_only, bool ext, bool fast, int defer, const void *params, bool *box = nullptr);
int export_state(const void *params, int64_t *out, hipStream_t s);
int export_belief(const void *params, int8_t *out, int pw, int pd, hipStream_t s);
int gae(const float *rew, const float *val, const float *starts, const float *last_v, const float *dones, int T, int N,
        float g32, float gl32, float *adv, float *ret, hipStream_t s);
}  // namespace vn_cubic

// The CubicEnv state import (voxnav_state.hip; the encoder is env_state.h).
// Zeroes *n_rejected (when given) on the stream, then one launch.
namespace vn_state {
int import_state(const void *params, const int64_t *state, const int8_t *belief, const uint8_t *mask, float *obs,
                 int32_t *n_rejected, int pw, int pd, hipStream_t s);
}  // namespace vn_state

// The episode records' unit (voxnav_episode.hip): the buffer the step kernels
// update at episode ends (EnvConst::episodes), read out, reduced and cleared.
namespace vn_episode {
int records(const void *episodes, int N, int64_t *out, hipStream_t s);
int totals(const void *episodes, int N, int64_t *out, hipStream_t s);
int clear(void *episodes, int N, const uint8_t *mask, hipStream_t s);
}  // namespace vn_episode

// The per-agent gather (voxnav_gather.hip; vn_copy_agents): agent i of `dst`
// becomes a copy of agent src_index[i] of `src` -- both complete Params of
// layout-compatible envs (the caller has compared their layout tags), `parts`
// their AgentParts (env_plan.h).  Zeroes *n_rejected (when given) on the
// stream, then one launch.
namespace vn_gather {
int copy_agents(const void *dst, const void *src, const void *parts, const int32_t *src_index, const int64_t *seeds,
                int32_t *n_rejected, hipStream_t s);
}  // namespace vn_gather

// The frontier planner (voxnav_plan.hip; vn_plan_frontier; the rule is
// env_route.h): CubicEnv envs whose padded width and depth are at most 64 (the
// caller has checked).  One launch; reads the env, writes actions / dist only.
namespace vn_plan {
int frontier(const void *params, const uint8_t *mask, int32_t *actions, int32_t *dist, int pw, int pd, hipStream_t s);
// vn_plan_frontier_dists: also the per-action distances [N][6] and the set of best actions (u8 [N])
int frontier_dists(const void *params, const uint8_t *mask, int32_t *actions, int32_t *dist, int32_t *dists,
                   uint8_t *best, int pw, int pd, hipStream_t s);
}  // namespace vn_plan

// The simpleEnv unit (voxnav_simple.hip).
namespace vn_simple {
int ensure_mt(int device);
int launch(bool reset_only, int sline, int sbits, int L, int N, int obs_dim, const void *params, hipStream_t s);
std::string label(bool reset_only, bool ext, int sline, int sbits, int L);
int export_belief(const void *params, int8_t *out, int pw, int pd, hipStream_t s);
}  // namespace vn_simple
