/*
 * voxnav.h -- C-ABI of the MI355X-native batched voxel-grid exploration env
 * (the hot path of Noimps/3D-Navigation-Reinforcement-Learning: envs/CubicEnv.py
 * step/reset, batched the way train/Grid_Train.py batches it through SB3's
 * SubprocVecEnv).  Implemented by libvoxnav.so (HIP, gfx950).
 *
 * Conventions
 *   - every function returns 0 on success and a negative VN_ERR_* code on
 *     failure; vn_last_error() returns a thread-local description.  No C++
 *     exception ever crosses this boundary.
 *   - "device" pointers are HIP device (HBM) pointers owned by the caller
 *     (e.g. torch tensors' data_ptr()), contiguous, naturally aligned.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     All env calls are stream-ordered and asynchronous; none synchronises
 *     the host except to report a launch error.
 *   - one VnEnv per host thread; a VnEnv is bound to one device.
 *
 * Reference interfaces each entry point replaces are cited per function
 * (file:line into the reference tree).
 */
#ifndef VOXNAV_H
#define VOXNAV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VN_ABI_VERSION 2
#define VN_OBS_DIM 80            /* envs/CubicEnv.py:58-62, :295-311 */
#define VN_VARIANT_CUBIC 0       /* envs/CubicEnv.py  (obs 80)                   */
#define VN_VARIANT_SIMPLE 1      /* envs/simpleEnv.py (obs 6L + 7, goal reward)   */
#define VN_MAX_OBS_DIM 103       /* 6 * VN_MAX_L + 7                              */
#define VN_STATE_FIELDS 16
#define VN_MAX_L 16              /* largest supported local_map_length */
#define VN_MAX_W 255
#define VN_MAX_D 255
#define VN_MAX_H 31
#define VN_MAX_ROOMS 256

enum {
    VN_OK = 0,
    VN_ERR_INVALID = -1,     /* bad argument (shape, range, NULL)          */
    VN_ERR_HIP = -2,         /* HIP runtime error                          */
    VN_ERR_ROOM = -3,        /* room has no interior free cell, too big... */
    VN_ERR_OOM = -4
};

typedef struct VnEnv VnEnv;

/*
 * Parsed rooms, exactly what GridAgent.load_room produces per room
 * (envs/CubicEnv.py:402-448): the dense grid with walls (grid == -2)
 * flagged, plus an optional "Start position".  Rooms are in the order the
 * caller wants random.choice to index (the build sorts file names).
 */
typedef struct VnRoomSet {
    int32_t n_rooms;
    const int32_t *whd;          /* [n_rooms][3]  W, D, H                       */
    const uint8_t *walls;        /* concat of W*D*H bytes, index (x*D+y)*H+z;
                                    CubicEnv: value -2 after its 2 -> -2 mapping
                                    (:434), simpleEnv: file value 2 (:282)      */
    const int32_t *fixed_start;  /* [n_rooms][3] or NULL; -1 = draw a start     */
    const int32_t *goal;         /* [n_rooms][3] or NULL; "Goal=" line, -1 =
                                    draw one (simpleEnv :419-426)               */
} VnRoomSet;

/* GridAgent ctor kwargs (envs/CubicEnv.py:17-29) + batching knobs. */
typedef struct VnConfig {
    int32_t local_map_length;    /* L (ctor default 4; Grid_Train uses 10)      */
    int32_t use_room_draw;       /* 1: room_path given -> random.choice(rooms)  */
    int32_t autoreset;           /* SB3 VecEnv auto-reset inside vn_step        */
    int32_t variant;             /* VN_VARIANT_CUBIC / VN_VARIANT_SIMPLE        */
    double crash_penalty;        /* ctor default -2.0                           */
    double finish_percentage;    /* FINISH_PERCENTAGE = 0.84 (CubicEnv.py:12)   */
    int64_t agent_id_base;       /* global id of this shard's agent 0           */
    int64_t seed_stride;         /* next episode seed = seed + stride (mod 2^32)*/
} VnConfig;

typedef struct VnInfo {
    int32_t n_agents;
    int32_t n_rooms;
    int32_t local_map_length;
    int32_t pad_w, pad_d, pad_h; /* belief map padding (max room dims, PH%4==0) */
    int64_t belief_bytes_per_agent;
    int64_t device_bytes;        /* total HBM owned by the env                  */
    int32_t variant;
    int32_t obs_dim;             /* floats per observation row                  */
} VnInfo;

const char *vn_last_error(void);
int vn_abi_version(void);

/* GridAgent.__init__ for N agents on `device` (envs/CubicEnv.py:17-74). */
int vn_create(const VnRoomSet *rooms, int32_t n_agents, const VnConfig *cfg, int32_t device, VnEnv **out);

/*
 * Kernel-mode tuning of one env (A/B timing and the parity tests of the
 * non-default modes).  Every mode computes the same results; the defaults
 * (vn_tuning_default) are what vn_create uses.  The library reads no
 * environment variable: an env's mode is what its VnTuning says.  No
 * reference counterpart.
 */
typedef struct VnTuning {
    /* fixed at creation (they decide the memory layout) */
    int32_t pcache_cap;      /* CubicEnv plane-set mode, capped: -1 no cap (2 = u32
                                rows for rooms <= 32 x 32, 1 = u64 rows for <= 64 x
                                64, picked by room size), 1 at most u64 rows, 0 off
                                (byte marks)                                       */
    int32_t defer;           /* CubicEnv byte-mark mode: -1 auto (plane rows of <= 2
                                words defer each pass's plane marks to the next
                                step), 0 marks in the sensing pass                 */
    int32_t simple_layout;   /* simpleEnv belief layout: 0 auto (line layout for
                                rooms <= 32 x 32 x 8, bit planes of u64 words for
                                <= 64 x 64, else the dense map), 1 keeps the word
                                layout where auto picks lines, 2 forces the dense
                                map                                                */
    /* changeable on a live env (vn_set_tuning; they only pick a launch) */
    int32_t prio;            /* step kernel issue priority, bits: 1 the step's load
                                issue, 2 the obs flush, 64 a base level among the
                                SIMD's waves in launches of >= 8 steps (the wave
                                behind its mates goes first), 4 that level from the
                                open-loop rotation over a CU's blocks instead; and
                                one bit that is no priority, 8: an env whose rooms
                                are all exact boxes (vn_kernel_box) launches the
                                kernels that load the ray record, not the ones that
                                compute it (for paired timing); default 67         */
    int32_t dflush;          /* deferred obs flush (a step's flush after the next
                                step's load issue; launches of more than one step),
                                bits: 1 in the byte-mark kernels, 2 in the plane-set
                                ones; default 1                                    */
    int32_t wrec_k;          /* step launches of at most this many steps write the
                                window record (0: never); default 1                */
    int32_t wrec_early;      /* 1: a window record the previous launch wrote is
                                loaded beside the hot state instead of after it (one
                                dependent round trip less), 0: after; default 1    */
} VnTuning;

/* The defaults, defined here only (callers start from them and override). */
int vn_tuning_default(VnTuning *out);
/* vn_create with a tuning (NULL = defaults).  VN_ERR_INVALID for a field out
 * of range: pcache_cap in {-1, 0, 1, 2}, defer in {-1, 0}, simple_layout in
 * {0, 1, 2}, prio a subset of bits 79, dflush in 0..3, wrec_k >= 0,
 * wrec_early in {0, 1}. */
int vn_create_tuned(const VnRoomSet *rooms, int32_t n_agents, const VnConfig *cfg, int32_t device,
                    const VnTuning *tuning, VnEnv **out);
/* Replace the launch-time fields of a live env (takes effect at the next
 * launch).  VN_ERR_INVALID, with the field named in vn_last_error(), if a
 * creation-time field differs from what the env was created with or a value
 * is out of range; the env is then unchanged. */
int vn_set_tuning(VnEnv *env, const VnTuning *tuning);

int vn_destroy(VnEnv *env);
int vn_get_info(const VnEnv *env, VnInfo *info);

/*
 * GridAgent.reset(seed) for every agent with mask[i] != 0 (mask NULL = all)
 * (envs/CubicEnv.py:77-108, draws :407/:462).  seeds: device int64 [N],
 * each in [0, 2^32) (the reference also calls np.random.seed(seed), :80).
 * obs: device f32 [N][obs_dim]; rows of unmasked agents are left untouched.
 * simpleEnv variant (envs/simpleEnv.py:79-107): its reset neither seeds nor
 * returns an observation; the build seeds the draws with random.seed(seed)
 * and returns get_obs() after the reset (what train/evaluate_grid.py:54-55
 * does), so obs is that first observation.
 */
int vn_reset(VnEnv *env, const int64_t *seeds, const uint8_t *mask, float *obs, void *stream);

/*
 * GridAgent.step(action) for all N agents (envs/CubicEnv.py:110-132;
 * simpleEnv variant: envs/simpleEnv.py:109-150),
 * followed, when cfg.autoreset, by the SB3 VecEnv auto-reset of every agent
 * whose step ended the episode (terminated or truncated).
 *   actions       device i32 [N], each in 0..5
 *   obs           device f32 [N][obs_dim] (post-reset obs for finished agents;
 *                 obs_dim = 80, or 6L+7 for the simpleEnv variant)
 *   reward        device f32 [N]      (may be NULL)  -- f64 reward rounded
 *   reward64      device f64 [N]      (may be NULL)  -- exact f64 reward
 *   terminated    device u8  [N]      (may be NULL)
 *   truncated     device u8  [N]      (may be NULL)
 *   terminal_obs  device f32 [N][obs_dim] (may be NULL) written only for agents
 *                 that finished an episode in this step
 */
int vn_step(VnEnv *env, const int32_t *actions, float *obs, float *reward, double *reward64,
            uint8_t *terminated, uint8_t *truncated, float *terminal_obs, void *stream);

/*
 * k_steps fused steps under the build's uniform random policy
 * (action = (Philox4x32-10(key=policy_seed, ctr=(gid, t0+k))[0] * 6) >> 32).
 * Outputs are [k_steps][N]-major (obs [k_steps][N][80]); actions_out
 * (device i32 [k_steps][N]) may be NULL.
 */
int vn_step_random(VnEnv *env, uint64_t policy_seed, uint64_t t0, int32_t k_steps, int32_t *actions_out,
                   float *obs, float *reward, double *reward64, uint8_t *terminated, uint8_t *truncated,
                   float *terminal_obs, void *stream);

/*
 * k_steps fused steps of caller-given actions: vn_step's semantics per step
 * (auto-reset included), vn_step_random's output layout, one launch -- a
 * recorded action log replayed, or an action plan evaluated, without a launch
 * per step.
 *   actions       device i32 [k_steps][N], each in 0..5
 *   obs           device f32 [k_steps][N][obs_dim]
 *   reward / reward64 / terminated / truncated
 *                 device [k_steps][N] (each may be NULL, as in vn_step)
 *   terminal_obs  device f32 [k_steps][N][obs_dim] (may be NULL): row [k][i] is
 *                 written only where agent i's step k ended an episode
 * The launch is the one vn_step makes, with k_steps steps in it: the same
 * explicit-action kernels, and the window records are written by launches of at
 * most VnTuning::wrec_k steps as for every other call.  k_steps one-step
 * vn_step calls and one vn_step_actions(k_steps) call leave the same outputs
 * and the same env.  VN_ERR_INVALID: k_steps < 1, NULL env / actions / obs.
 * No reference counterpart (the reference steps one env at a time).
 */
int vn_step_actions(VnEnv *env, const int32_t *actions, int32_t k_steps, float *obs, float *reward,
                    double *reward64, uint8_t *terminated, uint8_t *truncated, float *terminal_obs,
                    void *stream);

/*
 * Parity dumps.  state_out: device i64 [N][16] in the field order
 * x, y, z, facing, last_action, step_count, visited_count, bump_count,
 * done, last_bump, near_wall, was_near_wall, cells_insight_down, room,
 * max_steps, next_seed.  simpleEnv variant: fields 9..11 are the goal
 * (gx, gy, gz) and 12 is 0 (it has no last_bump / near-wall state).
 * belief_out: device i8 [N][pad_w][pad_d][pad_h] dense x-major, the
 * reference's internal_grid values (CubicEnv: -2 wall, -1 unknown, 0 free,
 * n visits; simpleEnv: -1 unknown, 0 free, 1 visited, 2 wall;
 * visit counts saturate at 63), cells outside the agent's room read -128.
 */
/*
 * Name of the kernel instantiation a call of this shape launches
 * (k_steps = 0: vn_reset; explicit_actions: vn_step; fast: reward, terminated
 * and truncated requested, no f64 reward or action record).  Diagnostics:
 * lets bench.py and rocprofv3 summaries name the kernel they time.  No
 * reference counterpart.
 */
int vn_kernel_label(const VnEnv *env, int32_t k_steps, int32_t explicit_actions, int32_t fast, char *buf,
                    int32_t len);
/*
 * *box = 1 when a call of this shape launches the BOX instantiation of the
 * kernel vn_kernel_label names (the label stops before that template
 * argument): the step kernel that computes each ray record from the agent's
 * coordinates and its room's size instead of loading it.  vn_create proves,
 * cell by cell against the ray table, that every room of the set is a box of
 * one wall layer around a free interior; such an env's plane-set step
 * launches take it, unless VnTuning::prio bit 8 is set or the deferred flush
 * is chosen.  Results are identical.  0 for every other env and call.
 */
int vn_kernel_box(const VnEnv *env, int32_t k_steps, int32_t explicit_actions, int32_t fast, int32_t *box);
int vn_export_state(VnEnv *env, int64_t *state_out, void *stream);
int vn_export_belief(VnEnv *env, int8_t *belief_out, void *stream);

/*
 * The exports' other direction (CubicEnv variant): every agent with
 * mask[i] != 0 (mask NULL = all) takes the reference attributes of its state
 * row (vn_export_state's field order; field 14, max_steps, is derived and
 * ignored; field 15 is the next auto-reset seed) and the internal_grid of its
 * belief row (vn_export_belief's encoding; a count above 63 is clamped to 63,
 * as the device map saturates; cells outside the agent's room are ignored),
 * and its obs row (device f32 [N][80], may be NULL) receives get_obs() of
 * that agent -- with get_obs's own side effects (envs/CubicEnv.py:254-312,
 * :345-397): the six sensing rays from the agent's cell mark what they see,
 * near_wall is set if a wall is one cell away, cells_insight_down is
 * recomputed.  For a state taken from the exports all of that is the
 * identity.  (The row is get_obs() of the state the last step LEFT: step()
 * takes its own observation before it updates last_action, last_bump and
 * was_near_wall, :120-124, so obs[68..70] of the row that step returned show
 * the values of before the step, which no export holds; the other 77 floats
 * are that row's.)  Afterwards the agent is indistinguishable from one that reached
 * this state by stepping, in whatever belief layout this env was planned with
 * (VnTuning), whichever layout the exporting env had: obs, f64 rewards,
 * flags, exports and the auto-reset seed schedule continue bit for bit.
 * Unmasked agents keep their state, map and obs row.  Stream-ordered; the
 * host is not synchronised.
 *
 * Validation runs on the device before anything of the agent is written.  A
 * rejected agent is left untouched (its obs row too) and counted in
 * *n_rejected (device i32 [1], may be NULL; zeroed by the call first):
 *   room outside the env's rooms; position outside that room or on a wall
 *   cell; facing not 0..3; last_action not 0..5; a flag not 0/1;
 *   cells_insight_down not 0..L; seed outside [0, 2^32); a negative counter,
 *   or a visited_count above the room's cell count; inside the room a value
 *   below -2, -2 where the room has no wall or a value >= 0 where it has one;
 *   the agent's own cell below 1.
 * A step_count above the hot state's 24-bit field (16777215) or a bump_count
 * above its 26-bit field (67108863) is CLAMPED to that maximum, not rejected:
 * the device counters saturate there, so this is the value stepping would
 * have reached.
 * VN_ERR_INVALID (host, nothing launched): NULL env / state / belief, or an
 * env of the simpleEnv variant.
 *
 * Out of scope: a portable import for the simpleEnv variant (its dense map
 * does not determine the device state: a cell the agent stood on that the
 * edge quirk later turned into 2 exports like a quirk-only cell, while
 * knownness is derived from the stood set) -- vn_snapshot_* covers that
 * variant; a collector's or learner's mid-rollout state (LSTM state, rollout
 * buffers, Monitor counters); setters on the GridAgent facade.
 */
int vn_import_state(VnEnv *env, const int64_t *state, const int8_t *belief, const uint8_t *mask, float *obs,
                    int32_t *n_rejected, void *stream);

/*
 * Whole-env raw snapshots (both variants, every layout): an opaque,
 * layout-native copy of every mutable per-agent buffer -- the hot state with
 * the window records behind it, the next seeds, the belief blocks, the
 * goals, the simpleEnv draw-ahead, the episode records, the stood rows and
 * masks -- as
 * stream-ordered device-to-device copies into / from one caller-owned device
 * blob of vn_snapshot_bytes bytes.  The blob has no header: no call reads
 * device memory back.  What its bytes mean is named by vn_snapshot_tag, a
 * host-side hash of the ABI version, variant, N, L, the planned layout, the
 * creation-time tuning, the config and the room tables; vn_snapshot_load
 * returns VN_ERR_INVALID when `tag` is not the env's own and then touches
 * nothing.  After a load (as after an import) the env's "the previous launch
 * wrote every window record" flag is false: the copied hot words keep their
 * record bits and the records were copied with them, so the next launch
 * reads each agent's record after its state instead of beside it -- the
 * records are consumed, the bit is not cleared.  No reference counterpart.
 */
int vn_snapshot_tag(const VnEnv *env, uint64_t *tag);
int vn_snapshot_bytes(const VnEnv *env, int64_t *bytes);
int vn_snapshot_save(VnEnv *env, void *dst, void *stream);
int vn_snapshot_load(VnEnv *env, const void *src, uint64_t tag, void *stream);

/*
 * Per-agent copies between envs (both variants, every layout): agent i of dst
 * becomes a layout-native copy of agent src_index[i] of src (-1: agent i keeps
 * its state).  One launch, stream-ordered, no host synchronisation.
 *   src_index   device i32 [N_dst]
 *   seeds       device i64 [N_dst] or NULL: seeds[i] >= 0 replaces the copied
 *               next auto-reset seed, -1 keeps the source's
 *   n_rejected  device i32 [1] (may be NULL; zeroed by the call first)
 * What is copied: the agent's block of every mutable per-agent buffer -- its
 * hot word and (CubicEnv) the window record behind it, the next seed, the
 * belief block, the goal, the simpleEnv draw-ahead row and (plane-set mode 2)
 * the 32 stood rows and the nonzero-set mask.  The running episode's counters
 * are part of the hot word and travel; the episode records (vn_episode_*)
 * stay with the slot, as after vn_import_state.  The random policy of
 * vn_step_random is keyed by the agent's slot, not by its state: a copy
 * repeats its source only under explicit actions (vn_step, vn_step_actions).
 * Afterwards dst's "the previous launch wrote every window record" flag is
 * false, as after vn_snapshot_load: a copied hot word keeps its record bit and
 * its record came with it.  A simpleEnv draw-ahead row is valid only for the
 * seed it was drawn for, so a seed override leaves the copied row unused.
 *
 * The envs must be on one device and agree in everything vn_snapshot_tag
 * hashes except N, agent_id_base and the size of the episode records (the
 * "layout tag": variant, L, the planned layout, the creation-time tuning, the
 * config, seed_stride included, and the room tables).  Otherwise VN_ERR_INVALID
 * with the reason in vn_last_error(), and nothing is launched.
 *
 * Validation runs on the device before anything of an agent is written.  A
 * rejected destination is left untouched and counted in *n_rejected:
 *   src_index[i] < -1 or >= N_src; seeds[i] < -1 or >= 2^32;
 *   dst == src (allowed) and the source j != i is itself written by this call:
 *   src_index[j] is neither -1 nor j, or seeds[j] is not -1.
 * With that rule an in-place fan-out needs no pre-pass: every decision is a
 * function of src_index and seeds alone, and a block reads only agents that
 * no block writes.  No reference counterpart.
 */
int vn_copy_agents(VnEnv *dst, const VnEnv *src, const int32_t *src_index, const int64_t *seeds,
                   int32_t *n_rejected, void *stream);

/*
 * The frontier planner (CubicEnv variant): for every agent the first action
 * of a shortest path, through cells it knows to be free, to the nearest cell
 * that is known free and not yet visited.  No reference counterpart (the
 * reference has no scripted policy); the classical frontier-exploration
 * baseline, computed on the device from the agent's own belief map.
 *
 * The rule.  Agent i has room (W, D, H), cell a and facing f; v(c) is what
 * vn_export_belief returns for a cell c of its room: -2 wall, -1 unknown,
 * 0 known free and unvisited, n >= 1 visited.
 *   passable(c)  c is inside the room and v(c) >= 0 (unknown cells are not
 *                passable: the planner uses only what the agent knows)
 *   target(c)    v(c) = 0
 *   flood        R_0 = the targets; R_j = (R_j-1 and the six-neighbours of
 *                its cells) that are passable
 *   n_k          k = 0..5: the cell action k moves to from a under facing f
 *                (do_action, envs/CubicEnv.py:135-153: 0-3 forward / right /
 *                backward / left relative to f, 4 is +z, 5 is -z)
 * Found: with j the smallest index such that some passable n_k is in R_j,
 * actions[i] is the lowest such k and dist[i] = j + 1, the number of steps to
 * the target.  Fallback, when the flood stops growing before it reaches a
 * passable n_k: actions[i] is the k whose passable n_k has the smallest
 * v(n_k), ties to the lowest k, or 0 if no n_k is passable; dist[i] = -1.
 * The planner never proposes a move into a cell it does not know to be free,
 * so it never bumps except through that last action-0 case.
 *
 *   mask     device u8 [N] or NULL = all; rows of unmasked agents are left
 *            untouched
 *   actions  device i32 [N]
 *   dist     device i32 [N], may be NULL
 * One launch, stream-ordered, no host synchronisation; nothing of the env is
 * written.  VN_ERR_INVALID, with nothing launched and the reason in
 * vn_last_error(): NULL env or actions; a simpleEnv env; an env whose padded
 * width or depth (VnInfo pad_w, pad_d) exceeds 64.
 */
int vn_plan_frontier(VnEnv *env, const uint8_t *mask, int32_t *actions, int32_t *dist, void *stream);

/*
 * The frontier planner's cost-to-go per action: what vn_plan_frontier knows
 * and does not return.  With passable, target, the flood R_j and n_k as
 * defined there, for agent i and action k = 0..5:
 *   dists[i][k] = j + 1, j the smallest index with n_k in R_j: the number of
 *                 steps to the nearest target when the first step is action k
 *               = -1 if n_k is passable but the flood stops growing (or
 *                 reaches vn_plan_frontier's cap) before it contains n_k
 *               = -2 if n_k is not passable: outside the room, a known wall,
 *                 or unknown
 *   best[i]     a bit set: bit k is set iff dists[i][k] > 0 and equals the
 *               smallest positive entry; 0 when no entry is positive
 *   actions[i], dist[i]  exactly what vn_plan_frontier writes, its fallback
 *               included; when best[i] != 0 they are the lowest set bit of
 *               best[i] and the smallest positive entry
 * An agent vn_plan_frontier answers with (0, -1) before it plans (room index
 * out of range, room larger than the padded size, cell outside its room) gets
 * dists all -2 and best 0.  Two positive entries differ by at most 2 whenever
 * the agent's own cell is passable (one step back and on through the other
 * neighbour), which it is in every state an env reaches by itself.
 *
 *   mask     device u8 [N] or NULL = all; rows of unmasked agents are left
 *            untouched in all four outputs
 *   actions  device i32 [N], may be NULL
 *   dist     device i32 [N], may be NULL
 *   dists    device i32 [N][6]
 *   best     device u8 [N], may be NULL
 * One launch, stream-ordered, no host synchronisation; nothing of the env is
 * written.  VN_ERR_INVALID, with nothing launched: the cases of
 * vn_plan_frontier (actions may be NULL here), and a NULL dists.
 */
int vn_plan_frontier_dists(VnEnv *env, const uint8_t *mask, int32_t *actions, int32_t *dist, int32_t *dists,
                           uint8_t *best, void *stream);

/*
 * Episode records (both variants): what the reference reports at every
 * episode end -- "Goal Reached! Explored X % after N Steps" / "Truncated
 * after N Steps, with B Bumps and X % of cells discovered"
 * (envs/CubicEnv.py:212-222) -- and what train/evaluate_grid.py:213-247
 * builds its results table from: steps, bumps, discovered cells, finished.
 * The step kernels write one 64-byte row per agent at the step that ends an
 * episode, from the state that step left (vn_export_state's fields 5, 7, 6,
 * 14, 13 and `done`), before the in-kernel auto-reset overwrites it; the
 * totals survive any number of episode ends inside one fused launch.
 *
 * An episode ends at the first step after a reset on which terminated or
 * truncated is set.  With autoreset every such step ends one.  Without it an
 * agent that is stepped on after its end records nothing more until it is
 * reset (the reference keeps returning truncated there): a step whose
 * entering state had `done` set or step_count at max_steps does not count.
 * vn_reset of an agent in mid-episode abandons that episode (nothing is
 * counted); vn_import_state leaves the rows untouched; vn_snapshot_save /
 * vn_snapshot_load carry them.  `finished` counts the episodes that ended
 * with `done` set (CubicEnv: the finish percentage reached; simpleEnv: goal
 * reached).  last_flags: bit 0 terminated, bit 1 truncated.  Rows are zero at
 * vn_create.  All three calls are stream-ordered and do not synchronise the
 * host.
 */
#define VN_EPISODE_FIELDS 12
/* device i64 [N][12]: episodes, finished, sum_steps, sum_bumps, sum_visited,
   sum_max_steps, last_steps, last_bumps, last_visited, last_max_steps,
   last_room, last_flags   (envs/CubicEnv.py:212-222) */
int vn_episode_records(VnEnv *env, int64_t *out, void *stream);
/* device i64 [6]: the six totals summed over all agents, reduced on the
   device (exact integer sums, so order-independent and reproducible): the
   per-run aggregates of train/evaluate_grid.py:213-247 */
int vn_episode_totals(VnEnv *env, int64_t *out, void *stream);
/* zero the rows of agents with mask[i] != 0 (NULL = all): a new measuring
   window (train/evaluate_grid.py:213-247 starts each table from zero) */
int vn_episode_clear(VnEnv *env, const uint8_t *mask, void *stream);

/*
 * GAE advantage/return scan (SB3 RolloutBuffer.compute_returns_and_advantage,
 * called from RecurrentPPO.learn at train/Grid_Train.py:228).  All arrays
 * device f32, [T][N]-major; last_values/dones [N].
 */
int vn_gae(const float *rewards, const float *values, const float *episode_starts, const float *last_values,
           const float *dones, int32_t T, int32_t N, double gamma, double gae_lambda, float *advantages,
           float *returns, void *stream);

/*
 * Return-based reward normalisation (SB3 VecNormalize(norm_reward=True):
 * _update_reward / normalize_reward / RunningMeanStd.update_from_moments; the
 * reference's other trainer wraps its env so, GARL/train/train_single.py:26),
 * on the rollout buffer's rewards, before any truncation bootstrap.  This
 * comment is the rule; csrc/ret_rms.h, the kernels (csrc/voxnav_rnorm.hip)
 * and the float64 restatement of the tests follow it.
 *
 * State: mean, var, count f64, initially 0, 1, 1e-4 (RunningMeanStd(epsilon=
 * 1e-4)); ret[N] f64, initially 0.  Constants: gamma (the collector's),
 * epsilon (1e-8), clip (10).
 *
 * Per rollout step t, in order, r[t,i] the raw f32 reward:
 *  1. ret[i] = ret[i] * gamma + (double) r[t,i].
 *  2. The batch moments of ret over all global agents (global id =
 *     agent_id_base + i).  Chunk c holds the ids 64c .. 64c+63; m is the
 *     number of agents present in it (only the last chunk can have m < 64).
 *     Chunk sum: the xor butterfly over 64 lanes, v_j += v_{j xor s} for
 *     s = 1, 2, 4, ..., 32, absent lanes holding +0.0; mean_c = sum / m;
 *     M2_c the same butterfly over (ret - mean_c)^2.  The chunk triples
 *     (n, mean, M2) are merged pairwise up a binary tree over the global
 *     chunk index: at each level node j = merge(node 2j, node 2j+1), a node
 *     without a right sibling passes through.  merge(a, b):
 *         n = n_a + n_b;  d = mean_b - mean_a;
 *         mean = mean_a + (d * n_b) / n;
 *         M2 = (M2_a + M2_b) + (((d * d) * n_a) * n_b) / n.
 *     The root is (n_B, mean_B, M2_B); var_B = M2_B / n_B.
 *  3. The running statistics take the batch by the same merge, as SB3 writes
 *     it: a = (count, mean, var * count), b = (n_B, mean_B, var_B * n_B);
 *     then count = n, mean = mean, var = M2 / n.
 *  4. r'[t,i] = (float) clamp(r[t,i] / sqrt(var + epsilon), -clip, clip),
 *     computed in f64 and rounded once, with the var that includes step t;
 *     written in place.
 *  5. ret[i] = 0 where step t ended an episode (dones[t,i] != 0).
 * Without `update` (SB3's training = False) steps 1-3 and 5 are skipped: ret
 * and the statistics do not change.  Every operation is one IEEE f64
 * + - * / sqrt in the stated order (the library is built without
 * contraction), so the result does not depend on how agents are sharded.
 *
 * Two calls, so that a cross-rank gather of the chunk triples can sit between
 * them.  Both are stream-ordered, read nothing back to the host and use no
 * floating-point atomics.  Arrays are device memory, rewards / dones f32
 * [T][N]-major with T >= t1; row t of dones is episode_starts[t + 1].
 *
 * vn_return_moments: steps [t0, t1) of this shard's N agents: carries ret
 *   (f64 [N], read and written back) and writes the chunk triples
 *   partials[t - t0][c][3] (f64, c < ceil(N / 64) the shard's own chunks).
 *   VN_ERR_INVALID, nothing launched: a NULL pointer, t0 < 0, t1 <= t0,
 *   N < 1, agent_id_base < 0 or not a multiple of 64 (waves are aligned to
 *   global chunks).
 * vn_reward_normalize: steps [t0, t1) of rewards [.][N].  With update != 0:
 *   per step the tree merge of the C_global triples of partials
 *   [t1 - t0][C_global][3] (all ranks' chunks in rank order), then the chain
 *   over the steps that updates rms (f64 [3]: mean, var, count) and gives
 *   sqrt(var_t + epsilon) per step, then step 4.  partials is consumed: the
 *   first triple of each row is overwritten (the row's root, then its scale).
 *   With update == 0 partials may be NULL and one scale from the stored var
 *   is used.  scale_out: f64 [t1 - t0], the per-step scales, or NULL.
 *   VN_ERR_INVALID, nothing launched: NULL rewards / rms (or partials with
 *   update), t0 < 0, t1 <= t0, t1 - t0 > 65535, N < 1, clip <= 0 or not
 *   finite, epsilon < 0, and with update a C_global below ceil(N / 64) (this
 *   shard's own chunks) or above 262144.
 */
int vn_return_moments(const float *rewards, const float *dones, int32_t t0, int32_t t1, int32_t N,
                      int64_t agent_id_base, double gamma, double *ret, double *partials, void *stream);
int vn_reward_normalize(float *rewards, int32_t t0, int32_t t1, int32_t N, double *partials, int32_t C_global,
                        double *rms, double epsilon, double clip, int32_t update, double *scale_out,
                        void *stream);

/*
 * Process options: kernel choices of the entry points that take no handle
 * (the row-layout LSTM and the f32 GEMMs), for A/B timing and the tests of
 * the non-default kernels.  Every choice computes the same function.  Read
 * at each call (relaxed atomics); VN_ERR_INVALID for an unknown option or an
 * out-of-range value.  No reference counterpart.
 */
enum {
    VN_OPT_ROWS_LAYOUT = 0,  /* vn_lstm_rows_fwd's layout (the backward has one): 0 auto
                                (by grid size against the CU count), 1 blocks of 32
                                units, 2 blocks of 16 units; default 0               */
    VN_OPT_ROWS_PRIO = 1,    /* 16-unit row kernels raise the issue priority on the
                                hand-off path: 0 / 1; default 1                      */
    VN_OPT_GEMM_DL = 2,      /* vn_gemm_f32_*: the direct-load kernel where operands
                                allow (0: always the register-staged one); default 1 */
    VN_OPT_GEMM_K32 = 3      /* direct-load GEMM: 32-deep chunks where K allows (half
                                the barriers, twice the LDS): 0 / 1; default 0       */
};
int vn_set_option(int32_t option, int32_t value);
int vn_get_option(int32_t option, int32_t *value);

/* ------------------------------------------------------------------------
 * Rollout collector (sb3_contrib RecurrentPPO.collect_rollouts, reached
 * from model.learn at train/Grid_Train.py:228; policy MlpLstmPolicy with
 * net_arch pi/vf=[256,256,128], lstm_hidden_size=256, :68-80, :196-204).
 * The GEMMs of the policy forward are library GEMMs issued by the caller;
 * these entry points are everything in between.  All device f32 unless
 * stated, stream-ordered.
 * ---------------------------------------------------------------------- */

/*
 * One LSTM step for n_lstm independent LSTMs over N agents (torch nn.LSTM
 * gate order i, f, g, o; RecurrentActorCriticPolicy._process_sequence):
 *   pre = gx + gh + b_ih + b_hh;  c = f*c + i*g;  h = o*tanh(c)
 *   gx       element (b, n, j) at gx[n*gx_row_stride + b*4H + j]  (x @ W_ih^T
 *            for all LSTMs in one GEMM)
 *   gh       [n_lstm][N][4H] (h @ W_hh^T) or NULL when the state is zero
 *   b_ih, b_hh [n_lstm][4H];  h (out), c (in/out) [n_lstm][N][H]
 *   h_store, c_store  [n_lstm][N][H] copies for the rollout buffer, or NULL
 * H must be a multiple of 4; gx_row_stride a multiple of 4, at least
 * n_lstm * 4H (a row may carry padding after its gates).
 */
int vn_lstm_cell(const float *gx, int64_t gx_row_stride, const float *gh, const float *b_ih, const float *b_hh,
                 float *h, float *c, float *h_store, float *c_store, int32_t n_lstm, int32_t N, int32_t H,
                 void *stream);

/*
 * vn_lstm_cell inside a rollout (RolloutCollector.collect, f32 policy): the
 * state is read from the buffer's lstm_c[t] (c_in, before the episode-start
 * mask) and the new (h, c) written only to lstm_h[t+1] / lstm_c[t+1]
 * (h_out, c_out); gh was computed from the unmasked lstm_h[t], so agents
 * with start[n] != 0 take neither gh nor c_in (their masked state is zero:
 * RecurrentActorCriticPolicy._process_sequence).  c_in != c_out; gh, start
 * non-NULL.  Other arguments as vn_lstm_cell.
 */
int vn_lstm_cell_masked(const float *gx, int64_t gx_row_stride, const float *gh, const float *b_ih,
                        const float *b_hh, const float *c_in, const float *start, float *h_out, float *c_out,
                        int32_t n_lstm, int32_t N, int32_t H, void *stream);

/* vn_lstm_cell with bf16 gate pre-activations (uint16_t storage) from bf16
 * GEMMs; the cell math and the (h, c) state stay f32, and h is also written
 * in bf16 to h_bf16 [n_lstm][N][H] (the next GEMMs' input), or NULL. */
int vn_lstm_cell_bf16(const uint16_t *gx, int64_t gx_row_stride, const uint16_t *gh, const float *b_ih,
                      const float *b_hh, float *h, float *c, uint16_t *h_bf16, float *h_store, float *c_store,
                      int32_t n_lstm, int32_t N, int32_t H, void *stream);

/*
 * The whole LSTM step of the bf16 policy path on the matrix cores: gate
 * GEMM [x | h] @ [W_ih | W_hh]^T (v_mfma_f32_32x32x16_bf16, f32 accumulate)
 * with the cell update as its epilogue.
 *   x        f32 [N][obs_dim] (the env's obs; rounded to bf16 in-kernel)
 *   h_in     bf16 [n_lstm][N][H] previous h (masked); h_out bf16, != h_in
 *   w_cat    bf16 [n_lstm][4H][Kp]: W_ih in columns [0, obs_dim), W_hh in
 *            [kx, kx+H), kx = obs_dim rounded up to 8, zeros elsewhere;
 *            Kp a multiple of 64 >= kx + H
 *   bias     f32 [n_lstm][4H] = b_ih + b_hh
 *   c        f32 [n_lstm][N][H] in/out; h32 / h_store / c_store f32 or NULL
 * H must be a multiple of 64.
 */
int vn_lstm_fused_bf16(const float *x, int32_t obs_dim, const uint16_t *h_in, const uint16_t *w_cat, int32_t Kp,
                       const float *bias, float *c, uint16_t *h_out, float *h32, float *h_store, float *c_store,
                       int32_t n_lstm, int32_t N, int32_t H, void *stream);

/*
 * vn_lstm_fused_bf16 inside a rollout (RolloutCollector.collect): the cell
 * state is read from the rollout buffer's previous slot and written only to
 * the next one, so no separate state array is rewritten every step.
 *   c_in   f32 [n_lstm][N][H]: the state entering the step BEFORE the
 *          episode-start mask (the buffer's lstm_c[t]); rows n with
 *          start[n] != 0 are read as zero (RecurrentActorCriticPolicy.
 *          _process_sequence's (1 - episode_start) mask); start f32 [N] or
 *          NULL (no mask)
 *   c_out  f32 [n_lstm][N][H], != c_in: the new state (lstm_c[t+1])
 *   h_store f32 or NULL: the new h (lstm_h[t+1])
 * Other arguments as vn_lstm_fused_bf16.
 */
int vn_lstm_fused_bf16_masked(const float *x, int32_t obs_dim, const uint16_t *h_in, const uint16_t *w_cat,
                              int32_t Kp, const float *bias, const float *c_in, const float *start, float *c_out,
                              uint16_t *h_out, float *h_store, int32_t n_lstm, int32_t N, int32_t H, void *stream);

/*
 * The whole LSTM step of the f32 (reference-dtype) policy path on the f32
 * matrix cores (v_mfma_f32_32x32x2_f32, exact f32 FMA chains): the gate GEMM
 * [x | h] @ [W_ih | W_hh]^T for n_lstm LSTMs with the cell update as its
 * epilogue, so the 4H gate pre-activations never reach memory
 * (RecurrentActorCriticPolicy._process_sequence for actor and critic,
 * sb3_contrib; replaces the two library GEMMs +
 * vn_lstm_cell_masked of one collector step).
 *   x        f32 [N][obs_dim], 16-byte aligned when obs_dim % 4 == 0
 *   h_in     f32 [n_lstm][N][H], != h_out; with start, rows n with
 *            start[n] != 0 are read as zero (the (1 - episode_start) mask)
 *   w_packed f32 [n_lstm][H/64][Kp][4][64]: element [b][ub][k][g][uu] =
 *            Wcat_b[g*H + 64*ub + uu][k], Wcat_b = [W_ih | 0 | W_hh] with
 *            W_ih in columns [0, obs_dim), W_hh in [kx, kx + H), kx =
 *            obs_dim rounded up to 16, Kp = kx + H
 *   bias     f32 [n_lstm][4H] = b_ih + b_hh
 *   c_in     f32 [n_lstm][N][H] (masked like h_in when start != NULL); may be
 *            c_out (in-place state)
 *   c_out, h_out  f32 [n_lstm][N][H]: the new state
 *   start    f32 [N] or NULL
 * H must be a multiple of 64.
 */
int vn_lstm_fused_f32(const float *x, int32_t obs_dim, const float *h_in, const float *w_packed, int32_t Kp,
                      const float *bias, const float *c_in, const float *start, float *c_out, float *h_out,
                      int32_t n_lstm, int32_t N, int32_t H, void *stream);

/*
 * One Linear layer (+ Tanh when tanh_act) of the policy's pi / vf MLPs
 * (MlpExtractor, net_arch [256, 256, 128] with Tanh, train/Grid_Train.py:68-80)
 * for n_branch (1 or 2) branches in one launch, on the f32 matrix cores with
 * the bias and Tanh in the epilogue:  y[i] = tanh(x[i] @ W_i^T + b_i).
 *   x[i]        f32 [M][K] rows with row stride ldx (>= K, % 4), 16-byte aligned
 *   w_packed[i] f32 [Nout/128][K][128]: element [cb][k][j] = W_i[128*cb + j][k]
 *   bias[i]     f32 [Nout];  y[i]  f32 [M][Nout]
 * K a multiple of 16, Nout a multiple of 128.  x, w_packed, bias and y are
 * host arrays of n_branch device pointers.
 */
int vn_linear_f32(int32_t n_branch, const float *const *x, int64_t ldx, const float *const *w_packed,
                  const float *const *bias, float *const *y, int32_t M, int32_t K, int32_t Nout, int32_t tanh_act,
                  void *stream);

/*
 * Action and value heads + Categorical draw (ActorCriticPolicy action_net /
 * value_net and distribution.get_actions / log_prob).
 *   latent_pi [N][P] (NULL: value only), latent_vf [N][P] (NULL: no value)
 *   w_action [n_actions][P], b_action [n_actions], w_value [P], b_value [1]
 *   actions (i32 [N]): Philox4x32-10(key=sample_seed, ctr=(agent_id_base+n,
 *   t | 2^63)) word 0 -> u = (w >> 8) / 2^24, first a with u < cdf[a]
 *   (argmax of the logits when deterministic); log_probs = logit - logsumexp.
 * 1 <= n_actions <= 8 (0 with latent_pi NULL); P a multiple of 4 in
 * 4..4096.  A block keeps the head weights in (n_actions + 1) * P * 4 bytes
 * of dynamic LDS: 147,456 B at the bounds (8 actions, P = 4096), within the
 * CU's 160 KiB.  Anything else returns VN_ERR_INVALID without a launch.
 */
int vn_policy_head(const float *latent_pi, const float *latent_vf, int32_t N, int32_t P, const float *w_action,
                   const float *b_action, int32_t n_actions, const float *w_value, const float *b_value,
                   uint64_t sample_seed, uint64_t t, int64_t agent_id_base, int32_t deterministic, int32_t *actions,
                   float *values, float *log_probs, void *stream);

/* vn_policy_head with bf16 latents (uint16_t storage); math in f32. */
int vn_policy_head_bf16(const uint16_t *latent_pi, const uint16_t *latent_vf, int32_t N, int32_t P,
                        const float *w_action, const float *b_action, int32_t n_actions, const float *w_value,
                        const float *b_value, uint64_t sample_seed, uint64_t t, int64_t agent_id_base,
                        int32_t deterministic, int32_t *actions, float *values, float *log_probs, void *stream);

/*
 * Invalid-action masking (Huang & Ontanon 2020; sb3_contrib MaskablePPO's
 * env.action_masks()), CubicEnv only (csrc/voxnav_mask.hip).
 *
 * vn_action_mask: mask [N] uint8 from obs f32 [N][80] (row stride ldo >= 80
 * floats).  Bit a (0 fwd, 1 right, 2 back, 3 left, 4 up, 5 down) is set iff
 * action a taken now would not bump; bits 6 and 7 are 0.  With f the index of
 * the 1 in obs[64:68] (the facing one-hot, 0 when there is none):
 *   a < 4: (dx, dy) = the step of relative direction a under facing f
 *          (N: fwd +y, right +x, back -y, left -x; E, S, W: that ring turned
 *          once, twice, three times), dz = 0;  a = 4: dz = +1;  a = 5: dz = -1
 *   v = obs[(dx+2) 16 + (dy+2) 4 + (dz+2)]   (the 4x4x4 window, offsets -2..+1
 *          around the centre 42: cells 58 / 26 (+-x), 46 / 38 (+-y), 43 / 41 (+-z))
 *   blocked iff v == 0.0f (known wall: (-2 + 2) / 22) or v == 1.0f / 22.0f
 *          (the window's out-of-bounds code -1)
 * The mask is exact: get_obs casts a ray of length >= 1 in all six directions
 * before it builds the window (envs/CubicEnv.py:229-275), so every in-bounds
 * neighbour is known wall or known free when the window is read (:322-332),
 * and the window reads -1 only out of bounds.  One launch, stream-ordered, no
 * host sync.  VN_ERR_INVALID without a launch: a NULL pointer, N < 1, ldo < 80.
 *
 * vn_policy_head_masked: vn_policy_head (f32) with the draw restricted to the
 * allowed actions S = mask & (2^n_actions - 1) of each agent (mask [N] uint8,
 * required, as is latent_pi; S = 0 counts as all allowed).  Logits outside S
 * take no part in the max, the log-sum-exp or the cdf; sampling takes the
 * first allowed a with u < cdf[a], the cdf running over the allowed actions in
 * index order, and the highest allowed index when none crosses; deterministic:
 * the argmax over S, the lowest index on ties.  log_prob = z[act] - lse_S.
 * The Philox counter and key are vn_policy_head's; values do not depend on
 * the mask; with S full, actions, log_probs and values are vn_policy_head's
 * bits.  Sizes and refusals as vn_policy_head.
 */
int vn_action_mask(const float *obs, int64_t ldo, int32_t N, uint8_t *mask, void *stream);
int vn_policy_head_masked(const float *latent_pi, const float *latent_vf, int32_t N, int32_t P, const float *w_action,
                          const float *b_action, int32_t n_actions, const float *w_value, const float *b_value,
                          const uint8_t *mask, uint64_t sample_seed, uint64_t t, int64_t agent_id_base,
                          int32_t deterministic, int32_t *actions, float *values, float *log_probs, void *stream);

/*
 * The collector's whole policy after the LSTM in ONE launch: the pi and vf
 * MLPs (MlpExtractor, Linear + Tanh per layer; net_arch [256, 256, 128],
 * train/Grid_Train.py:68-80) and the heads + Categorical draw of
 * vn_policy_head (ActorCriticPolicy.forward / predict_values), the
 * activations kept on chip (no latent reaches memory).  Replaces
 * vn_linear_f32 x n_layers + vn_policy_head of one collector step.
 *   n_branch 2: x[0] the pi input, x[1] the vf input; 1: x[0] the vf input
 *               (value only: the truncation bootstrap, last values)
 *   x[b]        f32 [M][K0] rows with row stride ldx (% 4), 16-byte aligned;
 *               K0 % 16 == 0, K0 <= 256
 *   widths      n_layers (1..4) layer widths, each 128 or 256; the last is P
 *   w_t[b * n_layers + l]  f32 W_l [N_l][K_l] packed per MFMA lane (16-byte
 *               aligned): [N_l/32][K_l/8][64][4], element [cb][kg][lane][s] =
 *               W_l[32 cb + lane % 32][8 kg + 4 (lane / 32) + s];
 *               K_0 = K0 rounded up to a multiple of 16 (zero weights past K0),
 *               K_l = widths[l - 1];  bias[b * n_layers + l] [N_l]
 *   w_action [n_actions][P], b_action (pi branch; n_actions <= 8),
 *   w_value [P], b_value [1]
 *   actions / log_probs (pi branch) and values: [M], the draw of
 *   vn_policy_head (Philox4x32-10 key sample_seed, counter (agent_id_base + m,
 *   t | 2^63); argmax when deterministic).
 * Host arrays: x (n_branch), widths (n_layers), w_t and bias (n_branch x n_layers).
 */
int vn_mlp_head_f32(int32_t n_branch, const float *const *x, int64_t ldx, int32_t K0, int32_t n_layers,
                    const int32_t *widths, const float *const *w_t, const float *const *bias, const float *w_action,
                    const float *b_action, int32_t n_actions, const float *w_value, const float *b_value,
                    uint64_t sample_seed, uint64_t t, int64_t agent_id_base, int32_t deterministic, int32_t *actions,
                    float *log_probs, float *values, int32_t M, void *stream);

/*
 * Ordered indices of the agents whose step was a time-limit truncation
 * (SB3 VecEnv: done and info["TimeLimit.truncated"] = truncated and not
 * terminated) -> boot_idx (device i32 [N]) and boot_count (device i32 [1]).
 * terminated / truncated must be 16-byte aligned.
 */
int vn_collect_compact(const uint8_t *terminated, const uint8_t *truncated, int32_t N, int32_t *boot_idx,
                       int32_t *boot_count, void *stream);

/*
 * Append the step's truncated agents (boot_idx / boot_count from
 * vn_collect_compact, device) to the rollout's bootstrap stash, so the
 * bootstrap values are computed once per rollout instead of after a host
 * read of the count every step (collect_rollouts' TimeLimit.truncated loop):
 * stash row base_in[0] + j takes agent a = boot_idx[j]'s terminal obs
 * (f32 [obs_dim]), its critic LSTM state (h_critic rows of H elements of
 * h_bytes = 2 (bf16) or 4 (f32) bytes, c_critic f32 rows; h_critic NULL: no
 * state) and the flat reward index t*N + a; base_out[0] = base_in[0] +
 * count (device i32).  Rows at or past cap are dropped: check the final
 * base <= cap.  Then vn_collect_bootstrap(stash_flat, values, M, gamma,
 * rewards [T][N]) applies them.
 */
int vn_collect_stash(const int32_t *boot_idx, const int32_t *boot_count, const int32_t *base_in, int32_t *base_out,
                     int32_t t, int32_t N, const float *terminal_obs, int32_t obs_dim, const void *h_critic,
                     int32_t h_bytes, const float *c_critic, int32_t H, float *stash_obs, void *stash_h,
                     float *stash_c, int32_t *stash_flat, int32_t cap, void *stream);

/*
 * Truncation bootstrap: rewards[boot_idx[i]] += gamma * terminal_values[i]
 * for i < M (f32, two roundings, as collect_rollouts' numpy update).
 */
int vn_collect_bootstrap(const int32_t *boot_idx, const float *terminal_values, int32_t M, double gamma,
                         float *rewards, void *stream);

/*
 * episode_starts[n] = terminated[n] | truncated[n] (f32 0/1, may be NULL)
 * and, for those agents, zero the LSTM state rows h, c [n_lstm][N][H] and
 * the bf16 copy h_bf16 (may be NULL) (n_lstm = 0: no recurrent state).
 */
int vn_episode_start(const uint8_t *terminated, const uint8_t *truncated, int32_t N, float *episode_starts,
                     float *h, float *c, uint16_t *h_bf16, int32_t n_lstm, int32_t H, void *stream);

/*
 * SB3 Monitor (train/Grid_Train.py:125 wraps every worker) for N agents, one
 * env step: ep_return (f64) += reward (reward64 when non-NULL, else the f32
 * reward), ep_length += 1; where terminated | truncated the finished
 * episode's (return, length) goes to rec_return / rec_length [N] (the
 * caller's row for this step; rec_length 0 = no episode ended) and the
 * counters restart, as Monitor.reset does under the VecEnv auto-reset.
 */
int vn_monitor_step(const double *reward64, const float *reward, const uint8_t *terminated, const uint8_t *truncated,
                    int32_t N, double *ep_return, int32_t *ep_length, double *rec_return, int32_t *rec_length,
                    void *stream);

/*
 * Everything the collector does after its env step t, in one launch:
 * episode_starts[n] = terminated | truncated (may be NULL); the Monitor step
 * (as vn_monitor_step, when ep_return is non-NULL; rec_* are the caller's
 * row t); the truncated (not terminated) agents' terminal obs and critic
 * state appended to the bootstrap stash (as vn_collect_compact +
 * vn_collect_stash, rows claimed atomically from *stash_count -- the
 * running count, read by the caller at a flush; rows past cap are dropped;
 * row order is not agent order, which the per-row bootstrap does not see);
 * and, for n_lstm > 0, the done agents' state rows h, c [n_lstm][N][H]
 * (and h_bf16, may be NULL) zeroed (as vn_episode_start).
 * Replaces sb3_contrib RecurrentPPO.collect_rollouts' per-step bookkeeping
 * after env.step (train/Grid_Train.py:228).
 */
int vn_collect_post_step(const uint8_t *terminated, const uint8_t *truncated, int32_t N, int32_t t,
                         float *episode_starts, const double *reward64, const float *reward, double *ep_return,
                         int32_t *ep_length, double *rec_return, int32_t *rec_length, const float *terminal_obs,
                         int32_t obs_dim, const void *h_critic, int32_t h_bytes, const float *c_critic, int32_t H,
                         float *stash_obs, void *stash_h, float *stash_c, int32_t *stash_flat, int32_t cap,
                         int32_t *stash_count, float *h, float *c, uint16_t *h_bf16, int32_t n_lstm, void *stream);

/* ------------------------------------------------------------------------
 * PPO learner: the LSTM re-run of sb3_contrib RecurrentPPO.train
 * (RecurrentActorCriticPolicy.evaluate_actions -> _process_sequence, from
 * model.learn at train/Grid_Train.py:228), its backward pass, and the
 * Linear layers of the update -- all on the library's own f32 matrix-core
 * kernels.  Gate order i, f, g, o (torch nn.LSTM).  All device f32,
 * stream-ordered.
 * ---------------------------------------------------------------------- */

/*
 * The learner's LSTM time loops on the f32 matrix cores (csrc/voxnav_learn_f32.hip;
 * sb3_contrib RecurrentPPO.train's LSTM re-run, train/Grid_Train.py:228, SURVEY.md
 * App. D.3): one launch per step, the whole product and the cell (or its backward)
 * fused.  vn_lstm_seq_pack_size gives the float counts of the two weight
 * workspaces (packed once per call).
 *   x      [L][B][D]                 w_ih [n_lstm][4H][D]   w_hh [n_lstm][4H][H]
 *   bias   [n_lstm][4H] = b_ih + b_hh
 *   hs, cs [n_lstm][L+1][B][H]       (index 0: the initial state, set by the caller)
 *   act    [L][n_lstm][B][4H]        (out: i, f, g, o after the nonlinearities)
 * Backward: dh_out [n_lstm][L][B][H] (gradient of the outputs), dG [n_lstm][L][B][4H]
 * (out), dc [n_lstm][B][H] (in: zeros = dL/dc_{L-1}; out: dL/dc_0), dh0 [n_lstm][B][H]
 * (out: dL/dh_0) or NULL.  D and H must be multiples of 4.
 */
int vn_lstm_seq_pack_size(int32_t n_lstm, int32_t D, int32_t H, int64_t *fwd_floats, int64_t *bwd_floats);
int vn_lstm_seq_fwd_mfma(const float *x, int32_t D, const float *w_ih, const float *w_hh, const float *bias,
                         float *wpack, float *hs, float *cs, float *act, int32_t n_lstm, int32_t L, int32_t B,
                         int32_t H, void *stream);
int vn_lstm_seq_bwd_mfma(const float *dh_out, const float *w_hh, float *wpack, const float *act, const float *cs,
                         float *dG, float *dc, float *dh0, int32_t n_lstm, int32_t L, int32_t B, int32_t H,
                         void *stream);

/*
 * The learner's LSTM re-run in the row layout (csrc/voxnav_learn_rows.hip; same
 * sb3_contrib RecurrentPPO.train re-run as above, train/Grid_Train.py:228): a
 * minibatch of R whole env rollouts as B = R rows over all L = T steps, a row's
 * state restarted from the buffer at every sequence start; ONE persistent launch
 * per direction with the weights resident in registers and the 8 unit blocks of
 * each (LSTM, 32-row tile) exchanging h (forward) / partial dh (backward) through
 * an in-launch agent-scope hand-off.  D 80, H 256, both LSTMs (actor, critic).
 *   x [L][B][D]; h_store, c_store [T][2][n_env][H] (the rollout buffer's states);
 *   env [L][B] int32 (the row's env), start [L][B] u8 (1: a sequence starts),
 *   keep [L][B] (1 - episode_start); out: hout, hprev (the h_{t-1} used), cprev,
 *   cnew [2][L][B][H], act [2][L][B][4H] (i, f, g, o); cnt: 2 * ceil(B / 32) * 64 u32 (one 256-B line per group counter)
 *   counters (zeroed by the call; 32-row tiles); err: set to 1 if a hand-off timed out.
 * Backward: dh_out [2][L][B][H] (+ the forward's hprev, cprev, cnew, act and x) ->
 * dG [2][L][B][4H] (may be NULL) and, accumulated inside the same launch, the weight gradients
 * dw_hh [2][4H][H], dw_ih [2][4H][D] and db_ih, db_hh [2][4H] (equal values, separate
 * storages: the parameters' own layouts); part:
 * vn_lstm_rows_part_floats floats of workspace.  vn_lstm_rows_supported: 1 when (D, H, B) can run (every
 * block co-resident on this device), else 0 (use vn_lstm_seq_*).
 */
int vn_lstm_rows_supported(int32_t D, int32_t H, int32_t B);
int vn_lstm_rows_part_floats(int32_t B, int64_t *floats);
int vn_lstm_rows_fwd(const float *x, int32_t D, const float *w_ih, const float *w_hh, const float *bias,
                     const float *h_store, const float *c_store, int64_t n_env, const int32_t *env,
                     const uint8_t *start, const float *keep, float *hout, float *hprev, float *cprev, float *cnew,
                     float *act, uint32_t *cnt, int32_t *err, int32_t L, int32_t B, int32_t H, void *stream);
int vn_lstm_rows_bwd(const float *dh_out, const float *w_hh, const float *act, const float *cprev, const float *cnew,
                     const float *hprev, const float *x, const uint8_t *start, float *dG, float *dw_hh,
                     float *dw_ih, float *db_ih, float *db_hh, float *part, uint32_t *cnt, int32_t *err, int32_t L,
                     int32_t B, int32_t H, void *stream);

/*
 * The learner's matrix products on the f32 matrix cores (csrc/voxnav_gemm_f32.hip):
 * every Linear of the PPO update (SB3 MlpExtractor / heads, RecurrentPPO.train) and
 * the LSTM weight gradients -- no library GEMM in the learner.  Batched over `batch`
 * with element strides s*.
 *   vn_gemm_f32_linear  C = act(A [M][K] @ W [N][K]^T + bias)   act 0 none, 1 tanh
 *   vn_gemm_f32_dx      C = dZ [M][K] @ W [K][N], dZ = dy (1 - y^2) (y != NULL) or dy
 *   vn_gemm_f32_tn      C [M][N] = dZ^T B, dZ [K][M] (as above), B [K][N], K split in
 *                       `splits` (workspace: splits*batch*M*N floats), colsum [batch][M]
 *                       = sum_k dZ[k][m] (workspace2: splits*batch*M), accumulate: C +=
 *                       (and colsum +=); C is contiguous [batch][M][N] (sc = M N)
 * Leading dimensions may exceed the row (padding is neither read nor written),
 * batch strides may be 0 or negative, and no pointer needs more than 4-B
 * alignment (aligned operands with K % 16 == 0 take the direct-load kernel; the
 * result does not depend on which kernel runs beyond the summation order).
 * VN_ERR_INVALID, with nothing launched: a NULL operand, output or workspace;
 * M, N, K, batch or splits < 1; act = 1 without bias; colsum without
 * workspace2; sc != M N.
 */
int vn_gemm_f32_linear(const float *a, int64_t lda, int64_t sa, const float *w, int64_t ldw, int64_t sw,
                       const float *bias, int64_t sbias, float *c, int64_t ldc, int64_t sc, int32_t M, int32_t N,
                       int32_t K, int32_t batch, int32_t act, void *stream);
int vn_gemm_f32_dx(const float *dy, const float *y, int64_t ldd, int64_t sd, const float *w, int64_t ldw, int64_t sw,
                   float *c, int64_t ldc, int64_t sc, int32_t M, int32_t N, int32_t K, int32_t batch, void *stream);
int vn_gemm_f32_tn(const float *dy, const float *y, int64_t ldd, int64_t sd, const float *b, int64_t ldb, int64_t sb,
                   float *c, int64_t sc, float *colsum, int32_t M, int32_t N, int32_t K, int32_t batch, int32_t splits,
                   float *workspace, float *workspace2, int32_t accumulate, void *stream);

/* PPO minibatch loss + its gradient to the MLP latents (csrc/voxnav_ppo_loss.hip).
 * Replaces, per minibatch, the heads and loss block of sb3 RecurrentPPO.train /
 * PPO.train (sb3_contrib ppo_recurrent.py train(): evaluate_actions -> ratio ->
 * clipped surrogate / value MSE / entropy -> loss.backward() down to the
 * latents), reached from train/Grid_Train.py:228 (model.learn).
 *   hp, hv [M][F] (row stride ldh): the actor / critic latents (F = 64..256, % 64)
 *   wa [A][F], ba [A] (action_net, A <= 8); wv [F], bv [1] (value_net)
 *   src [M] (NULL: identity): the buffer rows of the samples; actions int32,
 *   advantages, old_log_prob, returns: the rollout buffer, indexed by src
 *   -> dhp, dhv [M][F] contiguous: dloss/dlatent; grad_heads [A F + A + F + 1]:
 *      d action_net.weight, d action_net.bias, d value_net.weight, d value_net.bias;
 *      stats [6] f64: policy loss, value loss, entropy loss, loss, approx kl,
 *      clip fraction.  adv_sums [128] f64 scratch; part / spart: workspaces of
 *      the sizes vn_ppo_loss_part_floats returns (floats / doubles).
 * normalize_advantage: A = (adv - mean) / (std + 1e-8) over the minibatch, std
 * unbiased.  Equal advantages give A = 0.  With M = 1 the unbiased std of one
 * sample is NaN, as torch's: the policy loss, the loss, dhp and the action
 * head's gradients are NaN; the value loss, entropy loss, approx kl, clip
 * fraction, dhv and the value head's gradients do not depend on A and are
 * those of the formula.
 * VN_ERR_INVALID, with nothing launched: a NULL pointer other than src; M < 1;
 * A outside 1..8; F outside 64..256 or no multiple of 64; ldh < F.
 * vn_ppo_loss_part_floats: M, F or A < 1. */
int vn_ppo_loss_part_floats(int32_t M, int32_t F, int32_t A, int64_t *n_part, int64_t *n_spart);
int vn_ppo_loss(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                const float *bv, const int64_t *src, const int32_t *actions, const float *advantages,
                const float *old_log_prob, const float *returns, int32_t M, int32_t F, int32_t A, float clip_range,
                float ent_coef, float vf_coef, int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads,
                double *stats, double *adv_sums, float *part, double *spart, void *stream);

/* vn_ppo_loss with invalid-action masking (csrc/voxnav_masked_loss.hip;
 * sb3_contrib MaskablePPO.train): mask uint8, indexed by src like the other
 * buffers, bit j set where action j was allowed (vn_action_mask of the sample's
 * observation).  With S_i = (mask_i & (2^A - 1)) | (1 << a_i) -- the taken
 * action always counts as allowed, an empty set as full --
 *   lp_ij = z_ij - logsumexp_{k in S_i} z_ik   (j in S_i)
 *   p_ij  = exp(lp_ij)                         (j in S_i), 0 otherwise
 *   H_i   = -sum_{j in S_i} p_ij lp_ij
 *   dz_ij = g_lp_i ([j = a_i] - p_ij) + (ent_coef / M) p_ij (lp_ij + H_i)
 *                                              (j in S_i), exactly 0 otherwise
 * Everything else is vn_ppo_loss's: the ratio, the clip, the advantage
 * normalisation, the value term, stats [6], grad_heads, the workspaces (sizes
 * from vn_ppo_loss_masked_part_floats), the launches and the refusals, plus a
 * NULL mask.  With every S_i full the outputs are vn_ppo_loss's bits. */
int vn_ppo_loss_masked_part_floats(int32_t M, int32_t F, int32_t A, int64_t *n_part, int64_t *n_spart);
int vn_ppo_loss_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                       const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                       const float *advantages, const float *old_log_prob, const float *returns, const uint8_t *mask,
                       int32_t M, int32_t F, int32_t A, float clip_range, float ent_coef, float vf_coef,
                       int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                       double *adv_sums, float *part, double *spart, void *stream);

/* vn_ppo_loss / vn_ppo_loss_masked with the value update clipped
 * (csrc/voxnav_vclip_loss.hip; sb3 PPO.train with clip_range_vf): old_values,
 * indexed by src like returns, are the values the rollout stored.  With
 * c = clip_range_vf, lo_i = old_i - c and hi_i = old_i + c formed in f32,
 *   v'_i = min(max(v_i, lo_i), hi_i)
 *   value loss = (1/M) sum_i (ret_i - v'_i)^2
 *   dv_i = 2 vf_coef (v'_i - ret_i) / M   where lo_i <= v_i <= hi_i (the bounds
 *          inclusive, as torch.clamp's backward), exactly 0 elsewhere
 * -- in exact arithmetic sb3's old + clamp(v - old, -c, c); inside the range
 * v' is v bit for bit, so c = +inf (accepted) gives the unclipped entry's
 * outputs.  Everything else is the unclipped entry's: stats [6] (the value
 * loss and the loss on v'), grad_heads, the workspaces (vn_ppo_loss_part_floats
 * / vn_ppo_loss_masked_part_floats), the launches and the refusals, plus a NULL
 * old_values and a clip_range_vf that is NaN or <= 0. */
int vn_ppo_loss_vclip(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                      const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                      const float *advantages, const float *old_log_prob, const float *returns,
                      const float *old_values, int32_t M, int32_t F, int32_t A, float clip_range, float clip_range_vf,
                      float ent_coef, float vf_coef, int32_t normalize_advantage, float *dhp, float *dhv,
                      float *grad_heads, double *stats, double *adv_sums, float *part, double *spart, void *stream);
int vn_ppo_loss_masked_vclip(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                             const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                             const float *advantages, const float *old_log_prob, const float *returns,
                             const uint8_t *mask, const float *old_values, int32_t M, int32_t F, int32_t A,
                             float clip_range, float clip_range_vf, float ent_coef, float vf_coef,
                             int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                             double *adv_sums, float *part, double *spart, void *stream);

/* Behaviour-cloning minibatch loss + its gradient to the MLP latents
 * (csrc/voxnav_bc_loss.hip), the counterpart of vn_ppo_loss for the DAgger warm
 * start: cross-entropy to the frontier planner's actions (vn_plan_frontier) on
 * the labelled samples, the value MSE and the entropy bonus over all of them.
 *   z = h_pi Wa^T + ba,  lp = log_softmax(z),  p = exp(lp),  H = -sum_j p_j lp_j,  v = h_vf wv + bv
 *   n = sum_i w_i  (w_i in {0,1};  n = M without weights)
 *   loss = (1/max(n,1)) sum_i w_i (-lp_i[a*_i])  -  ent_coef (1/M) sum_i H_i  +  vf_coef (1/M) sum_i (ret_i - v_i)^2
 *   dz_ij = (w_i / max(n,1)) (p_ij - [j = a*_i]) + (ent_coef / M) p_ij (lp_ij + H_i)
 *   dv_i  = 2 vf_coef (v_i - ret_i) / M
 *   dh_pi = dz Wa,  dh_vf = dv wv,  dWa = dz^T h_pi,  dba = sum dz,  dwv,  dbv
 * With n = 0 the cross-entropy term, its gradient and the accuracy are exactly
 * 0; the other terms are unchanged.
 *   hp, hv [M][F] (row stride ldh >= F): the actor / critic latents (F = 64..256, % 64)
 *   wa [A][F], ba [A] (action_net, 1 <= A <= 8); wv [F], bv [1] (value_net)
 *   src [M] (NULL: identity): the buffer rows of the samples; labels int32 (a*,
 *   the expert's actions), weight uint8 (nonzero = labelled; NULL: all
 *   labelled), returns f32: the rollout buffers, indexed by src
 *   -> dhp, dhv [M][F] contiguous: dloss/dlatent; grad_heads [A F + A + F + 1]:
 *      d action_net.weight, d action_net.bias, d value_net.weight, d value_net.bias;
 *      stats [6] f64: cross-entropy, value loss, entropy loss (-mean H), loss,
 *      accuracy (the share of labelled samples whose argmax_j z_j, the lowest j
 *      on ties, equals a*), n / M.  part / spart: workspaces of the sizes
 *      vn_bc_loss_part_floats returns (floats / doubles).
 * Two launches without weights, three with (the labelled count, an exact
 * integer sum that stays on the device); stream-ordered, no host
 * synchronisation; two calls on the same inputs give the same bits.
 * VN_ERR_INVALID, with nothing launched: a NULL pointer other than src and
 * weight; M < 1; A outside 1..8; F outside 64..256 or no multiple of 64;
 * ldh < F.  vn_bc_loss_part_floats: M, F or A < 1. */
int vn_bc_loss_part_floats(int32_t M, int32_t F, int32_t A, int64_t *n_part, int64_t *n_spart);
int vn_bc_loss(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
               const float *bv, const int64_t *src, const int32_t *labels, const uint8_t *weight,
               const float *returns, int32_t M, int32_t F, int32_t A, float ent_coef, float vf_coef, float *dhp,
               float *dhv, float *grad_heads, double *stats, float *part, double *spart, void *stream);

/* vn_bc_loss with a set of equally good actions per sample in place of one
 * label (csrc/voxnav_bc_loss.hip): label_set uint8, indexed by src like the
 * other buffers; bit j of it says that action j is optimal (best of
 * vn_plan_frontier_dists).  S_i = label_set_i & (2^A - 1): bits at or above A
 * are ignored.  A sample is labelled iff S_i != 0 and its weight is nonzero
 * (a NULL weight counts as nonzero); n is the number of labelled samples.
 *   ce_i  = logsumexp_j z_ij - logsumexp_{j in S_i} z_ij      ( = -log sum_{j in S_i} p_ij )
 *   q_ij  = the softmax of z_i restricted to S_i (0 outside S_i)
 *   loss  = (1/max(n,1)) sum_{i labelled} ce_i + the entropy and value terms of vn_bc_loss
 *   dz_ij = (w_i / max(n,1)) (p_ij - q_ij) + the entropy term of vn_bc_loss   (w_i = 1 iff labelled)
 * Everything else -- the value and entropy terms, the outputs, the workspaces
 * (vn_bc_loss_part_floats), the errors -- is vn_bc_loss'.  stats[4] is the
 * share of labelled samples whose argmax (lowest index on ties) lies in S_i,
 * stats[5] = n / M.  A singleton set is vn_bc_loss with that label; the full
 * set gives ce_i = 0 and p - q = 0.  Three launches with or without weights:
 * n depends on the sets, so it is always counted (on the device, an exact
 * integer sum).  Two calls on the same inputs give the same bits. */
int vn_bc_loss_set(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                   const float *bv, const int64_t *src, const uint8_t *label_set, const uint8_t *weight,
                   const float *returns, int32_t M, int32_t F, int32_t A, float ent_coef, float vf_coef, float *dhp,
                   float *dhv, float *grad_heads, double *stats, float *part, double *spart, void *stream);

/* Kickstarted PPO's minibatch loss + its gradient to the MLP latents
 * (csrc/voxnav_ppo_bc_loss.hip): vn_ppo_loss with the cross-entropy of
 * vn_bc_loss (labels) / vn_bc_loss_set (label_set) added under bc_coef, in one
 * pass over the samples.  lp, p, H, v as above; A_i the (optionally
 * normalised) advantage, r_i the ratio and g_lp,i the surrogate's gradient
 * scale of vn_ppo_loss; w_i, n, q_i and ce_i those of vn_bc_loss /
 * vn_bc_loss_set (q_i one-hot at the label, or the softmax of z_i restricted to
 * S_i = label_set_i & (2^A - 1); n the labelled count, with sets only samples
 * with S_i != 0):
 *   loss  = -mean(min(A r, A clamp(r, 1-c, 1+c))) - ent_coef mean(H) + vf_coef mean((ret - v)^2)
 *           + bc_coef (1/max(n,1)) sum_i w_i ce_i
 *   dz_ij = g_lp,i ([j = a_i] - p_ij) + bc_coef (w_i / max(n,1)) (p_ij - q_ij) + (ent_coef / M) p_ij (lp_ij + H_i)
 *   dv_i  = 2 vf_coef (v_i - ret_i) / M
 * dz is formed as (ppo term + bc term) + entropy term: with bc_coef = 0, or
 * with no labelled sample, dhp, dhv, grad_heads and stats[0..5] equal
 * vn_ppo_loss's as values; with all advantages 0, normalize_advantage = 0,
 * finite ratios and bc_coef = 1, dhp, dhv and grad_heads equal vn_bc_loss's
 * (vn_bc_loss_set's).  With n = 0 the cross-entropy, its gradient and the
 * accuracy are exactly 0.
 *   the arguments of vn_ppo_loss, and labels int32 / label_set uint8, weight
 *   uint8 (NULL: every sample labelled), indexed by src like the other buffers
 *   -> dhp, dhv, grad_heads as vn_ppo_loss; stats [9] f64: [0..5] as
 *      vn_ppo_loss, with [3], the loss, including bc_coef ce; [6] the
 *      cross-entropy, [7] the accuracy (labelled samples whose argmax is the
 *      label / lies in the set, over max(n,1)), [8] n / M.  adv_sums [128] f64
 *      scratch; part / spart: workspaces of the sizes
 *      vn_ppo_bc_loss_part_floats returns (floats / 8-byte words: the blocks'
 *      seven f64 sums and the 64 labelled-count words behind them).
 * Up to four launches (the advantage sums when normalize_advantage, the
 * labelled count with weights or sets, the samples, the fixed-order sum);
 * stream-ordered, no host synchronisation, plain stores: two calls on the same
 * inputs give the same bits.
 * VN_ERR_INVALID, with nothing launched: a NULL pointer other than src and
 * weight; M < 1; A outside 1..8; F outside 64..256 or no multiple of 64;
 * ldh < F; bc_coef negative or not finite.  clip_range is taken as vn_ppo_loss
 * takes it.  vn_ppo_bc_loss_part_floats: M, F or A < 1. */
int vn_ppo_bc_loss_part_floats(int32_t M, int32_t F, int32_t A, int64_t *n_part, int64_t *n_spart);
int vn_ppo_bc_loss(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                   const float *bv, const int64_t *src, const int32_t *actions, const float *advantages,
                   const float *old_log_prob, const float *returns, const int32_t *labels, const uint8_t *weight,
                   int32_t M, int32_t F, int32_t A, float clip_range, float ent_coef, float vf_coef, float bc_coef,
                   int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                   double *adv_sums, float *part, double *spart, void *stream);
int vn_ppo_bc_loss_set(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                       const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                       const float *advantages, const float *old_log_prob, const float *returns,
                       const uint8_t *label_set, const uint8_t *weight, int32_t M, int32_t F, int32_t A,
                       float clip_range, float ent_coef, float vf_coef, float bc_coef, int32_t normalize_advantage,
                       float *dhp, float *dhv, float *grad_heads, double *stats, double *adv_sums, float *part,
                       double *spart, void *stream);

/* vn_bc_loss / vn_bc_loss_set / vn_ppo_bc_loss / vn_ppo_bc_loss_set with
 * invalid-action masking (csrc/voxnav_masked_bc_loss.hip,
 * csrc/voxnav_masked_ppo_bc_loss.hip; masked DAgger and masked kickstart): each
 * is its unmasked namesake with one more gathered buffer after weight, mask
 * uint8, indexed by src like the others, bit j set where action j was allowed
 * (vn_action_mask of the sample's observation).  With full = 2^A - 1 and L_i
 * the label's bits where sample i is labelled (its weight nonzero or absent;
 * labels: bit labels_i when 0 <= labels_i < A; label_set: label_set_i & full,
 * labelled only when that is non-empty), else 0, the softmax of sample i runs
 * over
 *   S_i = (mask_i & full) | L_i                 (vn_bc_loss_masked, vn_bc_loss_set_masked)
 *   S_i = (mask_i & full) | (1 << a_i) | L_i    (vn_ppo_bc_loss_masked, vn_ppo_bc_loss_set_masked)
 * with an empty S_i counting as full -- vn_ppo_loss_masked's rule extended by
 * the label, so neither the cross-entropy nor the ratio reads a log-probability
 * outside the support:
 *   lp_ij, p_ij, H_i as vn_ppo_loss_masked's over S_i; the argmax behind the accuracy runs over S_i
 *   q_i   = one-hot at the label, or the softmax of z_i restricted to label_set_i & full, as unmasked
 *   dz_ij = (the ppo term, where there is one, + the bc term) + the entropy term   (j in S_i),
 *           exactly 0 otherwise
 * Everything else is the unmasked entry's: n, bc_coef on the gradient scale,
 * the value term, stats [6] / [9], grad_heads, the launches, the workspaces
 * (sizes from vn_bc_loss_part_floats / vn_ppo_bc_loss_part_floats) and the
 * refusals, plus a NULL mask.  With every S_i full the outputs are the unmasked
 * entry's bits.  vn_ppo_bc_loss[_set]_masked with bc_coef = 0 and the labels
 * inside the masks gives vn_ppo_loss_masked's dhp, dhv, grad_heads and
 * stats[0..5] as values; with all advantages 0, normalize_advantage = 0,
 * bc_coef = 1 and the taken actions inside the masks its gradients equal
 * vn_bc_loss[_set]_masked's. */
int vn_bc_loss_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                      const float *wv, const float *bv, const int64_t *src, const int32_t *labels,
                      const uint8_t *weight, const uint8_t *mask, const float *returns, int32_t M, int32_t F,
                      int32_t A, float ent_coef, float vf_coef, float *dhp, float *dhv, float *grad_heads,
                      double *stats, float *part, double *spart, void *stream);
int vn_bc_loss_set_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                          const float *wv, const float *bv, const int64_t *src, const uint8_t *label_set,
                          const uint8_t *weight, const uint8_t *mask, const float *returns, int32_t M, int32_t F,
                          int32_t A, float ent_coef, float vf_coef, float *dhp, float *dhv, float *grad_heads,
                          double *stats, float *part, double *spart, void *stream);
int vn_ppo_bc_loss_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                          const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                          const float *advantages, const float *old_log_prob, const float *returns,
                          const int32_t *labels, const uint8_t *weight, const uint8_t *mask, int32_t M, int32_t F,
                          int32_t A, float clip_range, float ent_coef, float vf_coef, float bc_coef,
                          int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                          double *adv_sums, float *part, double *spart, void *stream);
int vn_ppo_bc_loss_set_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                              const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                              const float *advantages, const float *old_log_prob, const float *returns,
                              const uint8_t *label_set, const uint8_t *weight, const uint8_t *mask, int32_t M,
                              int32_t F, int32_t A, float clip_range, float ent_coef, float vf_coef, float bc_coef,
                              int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                              double *adv_sums, float *part, double *spart, void *stream);

/* vn_bc_loss_set / vn_ppo_bc_loss_set and their masked forms with a
 * distance-weighted target in place of the set (csrc/voxnav_soft_bc_loss.hip,
 * csrc/voxnav_soft_ppo_bc_loss.hip).  Sample i has the planner's distances
 * d_ik = dists[r ldd + k], k < A: dists int32 with row stride ldd >= A, the
 * values those of vn_plan_frontier_dists (positive = the path length through
 * first action k, -1 unreached, -2 not passable), row r through src like every
 * other gathered buffer.  tau is finite and > 0.
 *   P_i      = { k < A : d_ik > 0 }
 *   labelled : P_i is not empty and the weight is nonzero (a NULL weight counts
 *              as nonzero); n is the labelled count
 *   d*_i     = min over P_i,   delta_ik = d_ik - d*_i
 *   w_ik     = exactly 1 where delta_ik = 0, else expf(-delta_ik / tau)   (k in P_i); 0 outside P_i
 *   q_ik     = w_ik / sum_k w_ik
 *   kl_i     = sum_{k in P_i} q_ik (ln q_ik - lp_ik),  ln q_ik = -delta_ik / tau - ln sum_k w_ik,
 *              a term whose q_ik is 0 being 0
 *   loss     = (1/max(n,1)) sum_{i labelled} kl_i + the entropy and value terms of vn_bc_loss
 *   dz_ij    = (w_i / max(n,1)) (p_ij - q_ij) + the entropy term of vn_bc_loss   (w_i = 1 iff labelled)
 *   accuracy : the argmax (lowest index on ties) has delta = 0
 * The loss is KL(q || pi), not the bare cross-entropy: the gradient is the
 * same and its floor is 0 at every tau, so stats[0] means the same at every
 * tau and equals vn_bc_loss's cross-entropy where P_i is a singleton.
 * tau -> 0+ gives the uniform distribution on the shortest actions (best of
 * vn_plan_frontier_dists): a fixed target, unlike vn_bc_loss_set's, which
 * follows the policy.  A large tau gives the uniform distribution on P_i.  No
 * tau gives a NaN or an inf: at 1e-30 every w with delta > 0 is 0, at 1e30
 * every w is 1.
 * vn_ppo_bc_loss_soft is vn_ppo_bc_loss with this q_i, ce_i = kl_i and this n
 * (PpoBc<> composes it as it composes the other two: with bc_coef = 0 the
 * outputs equal vn_ppo_loss's as values, with all advantages 0,
 * normalize_advantage = 0 and bc_coef = 1 the gradients equal
 * vn_bc_loss_soft's).  The masked forms take mask after weight and run the
 * softmax over S_i of vn_bc_loss_masked / vn_ppo_bc_loss_masked with
 * L_i = P_i where sample i is labelled, else 0: every action the target gives
 * mass to counts as allowed, the KL never reads a log-probability outside the
 * support, dz is exactly 0 outside S_i, and with every S_i full the outputs
 * are the unmasked soft entry's bits.
 * Outputs (stats [6] / [9]), workspaces (vn_bc_loss_part_floats /
 * vn_ppo_bc_loss_part_floats) and launches are the _set entries': n depends on
 * the data, so the count always runs; stream-ordered, no host
 * synchronisation, plain stores: two calls on the same inputs give the same
 * bits.  VN_ERR_INVALID, with nothing launched: the namesake's refusals; a
 * NULL dists; ldd < A; tau not finite or <= 0. */
int vn_bc_loss_soft(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                    const float *bv, const int64_t *src, const int32_t *dists, int64_t ldd, const uint8_t *weight,
                    const float *returns, int32_t M, int32_t F, int32_t A, float tau, float ent_coef, float vf_coef,
                    float *dhp, float *dhv, float *grad_heads, double *stats, float *part, double *spart,
                    void *stream);
int vn_bc_loss_soft_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                           const float *wv, const float *bv, const int64_t *src, const int32_t *dists, int64_t ldd,
                           const uint8_t *weight, const uint8_t *mask, const float *returns, int32_t M, int32_t F,
                           int32_t A, float tau, float ent_coef, float vf_coef, float *dhp, float *dhv,
                           float *grad_heads, double *stats, float *part, double *spart, void *stream);
int vn_ppo_bc_loss_soft(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                        const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                        const float *advantages, const float *old_log_prob, const float *returns,
                        const int32_t *dists, int64_t ldd, const uint8_t *weight, int32_t M, int32_t F, int32_t A,
                        float clip_range, float ent_coef, float vf_coef, float bc_coef, float tau,
                        int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                        double *adv_sums, float *part, double *spart, void *stream);
int vn_ppo_bc_loss_soft_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                               const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                               const float *advantages, const float *old_log_prob, const float *returns,
                               const int32_t *dists, int64_t ldd, const uint8_t *weight, const uint8_t *mask,
                               int32_t M, int32_t F, int32_t A, float clip_range, float ent_coef, float vf_coef,
                               float bc_coef, float tau, int32_t normalize_advantage, float *dhp, float *dhv,
                               float *grad_heads, double *stats, double *adv_sums, float *part, double *spart,
                               void *stream);

/* DAgger's executed action for one collector step (csrc/voxnav_bc_loss.hip):
 * per agent i of N, with the planner's proposal expert[i] / dist[i]
 * (vn_plan_frontier) and the policy's own sample policy[i],
 *   u24 = word 0 of Philox4x32-10 >> 8, key mix_seed, counter (global agent id
 *         agent_id_base + i, t_global | 2^63): the sampler's draw under another key
 *   thr = floor(beta 2^24), computed on the host in double
 *   took_expert[i]  = dist[i] != -1 and u24 < thr
 *   executed[i]     = took_expert[i] ? expert[i] : policy[i]
 *   label_weight[i] = dist[i] != -1
 * Where the planner has only its fallback to offer (dist = -1) the policy acts
 * and the sample carries no label.  executed may be the policy array itself.
 * One launch, stream-ordered.  VN_ERR_INVALID, with nothing launched: a NULL
 * pointer; N < 1; beta outside [0, 1] (a NaN included). */
int vn_dagger_mix(const int32_t *policy, const int32_t *expert, const int32_t *dist, int32_t N, double beta,
                  uint64_t mix_seed, uint64_t t_global, int64_t agent_id_base, int32_t *executed, uint8_t *took_expert,
                  uint8_t *label_weight, void *stream);

/* vn_dagger_mix with best-set execution (csrc/voxnav_soft_bc_loss.hip): the
 * policy's own sample is executed whenever it is among the shortest actions.
 * The draw is vn_dagger_mix's (u24, thr, key mix_seed, counter (global agent
 * id, t_global | 2^63)); best uint8 [N] is vn_plan_frontier_dists' best, and
 * there is one more output, own_best uint8 [N]:
 *   turn            = dist[i] != -1 and u24 < thr
 *   own_best[i]     = dist[i] != -1 and 0 <= policy[i] < 8 and bit policy[i] of best[i]
 *   executed[i]     = (turn and not own_best[i]) ? expert[i] : policy[i]
 *   took_expert[i]  = turn and not own_best[i]
 *   label_weight[i] = dist[i] != -1
 * At beta = 1 every executed action with dist != -1 lies in best: the agent
 * walks a shortest path, and the policy breaks the ties, not the index rule.
 * Where every best[i] is the singleton of expert[i], executed and label_weight
 * are vn_dagger_mix's bits.  executed may be the policy array itself.  One
 * launch, stream-ordered.  VN_ERR_INVALID, with nothing launched: a NULL
 * pointer; N < 1; beta outside [0, 1] (a NaN included). */
int vn_dagger_mix_best(const int32_t *policy, const int32_t *expert, const int32_t *dist, const uint8_t *best,
                       int32_t N, double beta, uint64_t mix_seed, uint64_t t_global, int64_t agent_id_base,
                       int32_t *executed, uint8_t *took_expert, uint8_t *label_weight, uint8_t *own_best,
                       void *stream);

/* The total 2-norm of the parameter gradients (count <= 64 f32 tensors; device
 * pointers and element counts passed by host arrays) and the divisor the
 * fused Adam step applies to them: max(1, (norm + 1e-6) / max_norm), i.e.
 * 1 / torch.nn.utils.clip_grad_norm_'s clamped coefficient (sb3
 * max_grad_norm, sb3_contrib ppo_recurrent.py train()).  work: 256 doubles. */
int vn_grad_norm(const float *const *grads, const int64_t *sizes, int32_t count, float max_norm, float *norm,
                 float *scale, double *work, void *stream);

/* One Adam step over up to 64 f32 parameter tensors (torch.optim.Adam(eps,
 * betas), the optimizer sb3 builds for the policy; train/Grid_Train.py:84-86
 * lr 3e-4): the gradients divided by *clip_scale (vn_grad_norm's divisor; NULL:
 * 1), then torch's fused-Adam update with the bias corrections of `step`
 * (1-based); `steps` (nullable) receive the step count (torch's per-parameter
 * state["step"] scalars).  The gradients are not rewritten.  skip (nullable
 * device int32): when *skip != 0 at run time the launch changes nothing --
 * the learner passes the row-layout LSTM's error word (vn_lstm_rows_fwd/bwd
 * `err`), so gradients from a timed-out launch never reach the parameters.
 * With skip and every counter of `steps` given, the counters are the step
 * count: an applied step advances each by 1 on the device (a skipped one
 * leaves them), and its bias corrections are those of *steps[0] + 1; `step`
 * is the caller's expectation of that number, and a caller that does not
 * read *skip back may pass one that runs ahead after skipped steps.  Two
 * launches then, one otherwise. */
int vn_adam_step(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                 float *const *steps, const int64_t *sizes, int32_t count, const float *clip_scale,
                 const int32_t *skip, float lr,
                 float beta1, float beta2, float eps, int64_t step, void *stream);

/* The learner's KL gate (csrc/voxnav_trust.hip; sb3 PPO.train: approx_kl_div >
 * 1.5 * target_kl stops the update), one stream-ordered launch between a fused
 * loss call and vn_adam_step, all words on the device:
 *   was = *stop;  *ran = (was == 0)                      (ran nullable)
 *   if was == 0 and stats[kl_index] > threshold: *stop = 1   (strict; a NaN does not stop)
 *   *skip = (*stop != 0) || (err && *err != 0)           (err nullable)
 * stop is sticky until the caller zeroes it: the minibatch whose KL crosses
 * the threshold is logged (ran = 1) and not stepped (skip = 1), and every later
 * one is neither.  skip is what vn_adam_step takes as `skip`; err is the
 * row-layout LSTM's error word.  VN_ERR_INVALID, with nothing launched: NULL
 * stats, stop or skip; kl_index outside 0..15; a threshold that is not a
 * positive finite number. */
int vn_kl_gate(const double *stats, int32_t kl_index, double threshold, const int32_t *err, int32_t *stop,
               int32_t *skip, uint8_t *ran, void *stream);

/* A PPO minibatch's rows (sb3 PPO.train over the env-major flattened rollout
 * buffer): sample i has env-major id idx[i] = env * T + t; src[i] receives its
 * row t * N + env of the [T, N]-major buffers and out[i] its observation
 * row (D floats, D % 4 == 0). */
int vn_minibatch_rows(const int64_t *idx, int32_t M, int32_t T, int32_t N, const float *obs, int32_t D, float *out,
                      int64_t *src, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VOXNAV_H */
