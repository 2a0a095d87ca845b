// env_plan.h -- what vn_create works out on the host before it touches the
// device: the room tables (descriptors, ray records, start lists), the
// per-agent memory layout and kernel mode (EnvLayout), the obs LUT and the
// latent-wall room images; and the constants the host tables and the kernels
// share.  Plain C++17 with no HIP include: voxnav_api.hip uploads what these
// functions return, the kernel units (through env_core.h) read the constants,
// and tests/host/env_plan_check.cpp runs the arithmetic under g++ and the
// sanitizers.  Anonymous namespace, like env_core.h: one copy per unit.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "vn_error.h"

// host + device under hipcc, plain inline elsewhere
#ifdef __HIPCC__
#define VN_HD __host__ __device__ __forceinline__
#else
#define VN_HD inline
#endif

// Column index of (x, y) in the bricked map: bricks of 4 x 4 columns, x-major;
// inside a brick y fast ((x & 3) << 2 | (y & 3)), or x fast with VN_BRICK_T 1
// (diagnostics: a lane's 4 window columns -- one y, 4 consecutive x -- are
// then contiguous in the brick row), or 2 x 2 sub-bricks with VN_BRICK_T 2
// (a PH-16 64-B piece holds a 2 x 2 block of columns).
// (The two knob defaults below: a unit that includes vn_common.h includes it
// before this header, so that its knob guard sees what the build defined.)
#ifndef VN_BRICK_T
#define VN_BRICK_T 0
#endif
// Plane-set mode: the latent-wall room images, VN_WIMG_REP copies per room
// ([room][copy][map_bytes]); agent a reads copy a % VN_WIMG_REP (wimg_of).
#ifndef VN_WIMG_REP
#define VN_WIMG_REP 1
#endif

namespace {

using vn_detail::fail;

VN_HD uint32_t bcol(int x, int y, int nby) {
    const uint32_t in = VN_BRICK_T == 2 ? (uint32_t)(((x & 2) << 2) | ((y & 2) << 1) | ((x & 1) << 1) | (y & 1))
                        : VN_BRICK_T ? (uint32_t)(((y & 3) << 2) | (x & 3))
                                     : (uint32_t)(((x & 3) << 2) | (y & 3));
    return ((uint32_t)((x >> 2) * nby + (y >> 2)) << 4) + in;
}

// LDS table: [0,256) obs value of each belief byte; [256,262) f32(a/5);
// [264,281) f32(c/L)   (get_obs :273-275, :284, :287)
constexpr int TAB_ACTION = 256, TAB_CID = 264, TAB_SIZE = 288;
// after the CubicEnv table in the same device buffer: the simpleEnv reward of
// each event code (bit 0 bump, 1 repeated move, 2 goal, 3 explored), 16 f32
// then 16 f64, each the reference's f64 sum in its order (envs/simpleEnv.py:189-217)
constexpr int TAB_SREW = TAB_SIZE, TAB_SREW64 = TAB_SIZE + 16, TAB_ALL = TAB_SIZE + 48;
// Plane-set staging codes: belief-byte values that never occur (bit7 clear but
// not 0x00 / 0x40), whose LUT entries are the obs tail's values: 0.0, 1.0,
// f32(a/5), f32(c/L)   (voxnav_env.hip, STAGE_WORDS)
constexpr uint32_t TC_ZERO = 0x01u, TC_ONE = 0x02u, TC_ACT = 0x08u, TC_CID = 0x10u;

// One agent's episode record (vn_episode_records): the totals over every
// episode the agent ended since vn_create or the last vn_episode_clear, then
// the last ended episode -- the state the ending step left, before any
// auto-reset.  Written by lane q == 0 of the agent (CubicEnv) or the agent's
// lane (simpleEnv) at the step that ends an episode (episode_end, env_core.h).
struct EpisodeRec {
    uint32_t episodes, finished;                             // finished: ended with `done` set
    uint64_t sum_steps, sum_bumps, sum_visited, sum_max_steps;
    uint32_t last_steps, last_bumps, last_visited, last_max_steps, last_room, last_flags;
};
static_assert(sizeof(EpisodeRec) == 64, "one 64-byte row per agent");
constexpr uint32_t EP_TERMINATED = 1u, EP_TRUNCATED = 2u;    // last_flags

// ----------------------------------------------------------------------------
// The per-agent layout and kernel mode of one env: every value the host plans
// once and hands to the kernels (Params, EnvConst) or reports (vn_get_info).
// ----------------------------------------------------------------------------
struct EnvLayout {
    int variant = 0, obs_dim = VN_OBS_DIM;
    int pw = 0, pd = 0, ph = 0;   // padded room dims (ph: a whole column = one 8/16/32-byte access)
    int nbx = 0, nby = 0;         // 4 x 4 bricks per map row / column
    uint32_t map_bytes = 0;       // byte map (bricked) per agent
    uint32_t agent_bytes = 0;     // stride: the map and the planes after it
    uint32_t plane_bytes = 0;     // CubicEnv: the marked-bit planes after the map (what a reset clears)
    int nwx = 1, nwy = 1;         // u64 words per plane row
    uint32_t xp_off = 0, yp_off = 0;               // CubicEnv plane offsets inside the agent block
    uint32_t sy_off = 0, sz_off = 0, qz_off = 0;   // simpleEnv bit-plane offsets
    int sbits = 0;     // simpleEnv bit-plane layouts (rooms <= 64 x 64 x 31), else the dense map
    int sline = 0;     // simpleEnv line layout (simple_line_kernel), rooms <= 32 x 32 x 8
    int defer = 0;     // CubicEnv byte-mark mode with deferred plane marks (PCM 3; rows <= 2 words)
    int pcache = 0;    // CubicEnv plane-set mode (PH 8, rooms <= 64 x 64): see pset_fill
    int box = 0;       // CubicEnv: every room of the set is an exact box (rooms_box_exact; set by vn_create)
    uint32_t episode_bytes = (uint32_t)sizeof(EpisodeRec);   // both variants: the agent's episode record (own buffer)
};

inline EnvLayout plan_layout(int variant, int L, int maxW, int maxD, int maxH, const VnTuning &tun) {
    EnvLayout l;
    l.variant = variant;
    l.obs_dim = variant == VN_VARIANT_SIMPLE ? 6 * L + 7 : VN_OBS_DIM;
    l.nbx = (maxW + 3) / 4;
    l.nby = (maxD + 3) / 4;
    l.ph = maxH <= 8 ? 8 : maxH <= 16 ? 16 : 32;   // whole column = one 8/16/32-byte access
    const bool dense = tun.simple_layout == 2;   // force the dense kernel (tests)
    if (l.variant == VN_VARIANT_SIMPLE && maxW <= 64 && maxD <= 64 && !dense) {
        // bit planes: SX u64 [pd][ph], SY u64 [pw][ph], SZ u32 [pw][pd], QZ u32 [pw][pd]
        l.sbits = 1;
        l.pw = maxW;
        l.pd = maxD;
        l.map_bytes = 0;
        l.nwx = l.nwy = 0;
        // A/B knob: simple_layout 1 keeps the word layout
        l.sline = (maxW <= 32 && maxD <= 32 && l.ph == 8 && tun.simple_layout != 1) ? 1 : 0;
        if (l.sline) {
            // lines: SX u32 [pd][8] (bit x), SY u32 [pw][8] (bit y), QZ u32 [pw][pd]
            l.sy_off = (uint32_t)(32 * l.pd);
            l.sz_off = l.sy_off + (uint32_t)(32 * l.pw);   // (no SZ copy)
            l.qz_off = l.sz_off;
            l.agent_bytes = (l.qz_off + (uint32_t)(4 * l.pw * l.pd) + 63u) & ~63u;
        } else {
            l.sy_off = (uint32_t)(8 * l.pd * l.ph);
            l.sz_off = l.sy_off + (uint32_t)(8 * l.pw * l.ph);
            l.qz_off = l.sz_off + (uint32_t)(4 * l.pw * l.pd);
            l.agent_bytes = (l.qz_off + (uint32_t)(4 * l.pw * l.pd) + 15u) & ~15u;
        }
        l.xp_off = l.yp_off = 0;
    } else if (l.variant == VN_VARIANT_SIMPLE) {
        // dense [pw][pd][ph] int8 map, no planes
        l.pw = maxW;
        l.pd = maxD;
        l.map_bytes = (uint32_t)(l.pw * l.pd * l.ph);
        l.nwx = l.nwy = 0;
        l.xp_off = l.yp_off = l.map_bytes;
        l.agent_bytes = (l.map_bytes + 15u) & ~15u;
    } else {
        l.pw = l.nbx * 4;
        l.pd = l.nby * 4;
        l.map_bytes = (uint32_t)(l.nbx * l.nby * 16 * l.ph);
        l.nwx = (l.pw + 63) / 64;
        l.nwy = (l.pd + 63) / 64;
        // plane-set mode: 2 = u32 rows (rooms <= 32 x 32), 1 = u64 rows (<= 64 x 64), 0 = byte marks
        l.pcache = l.ph != 8 ? 0 : (l.pw <= 32 && l.pd <= 32) ? 2 : (l.nwx == 1 && l.nwy == 1) ? 1 : 0;
        // A/B knob pcache_cap: 0 off, 1 at most u64 rows
        if (tun.pcache_cap >= 0 && tun.pcache_cap < l.pcache) l.pcache = tun.pcache_cap;
        // byte-mark mode with plane rows of <= 2 words: defer each pass's plane marks
        // to the next step (PendMarks) so the row loads hide behind a step
        // (A/B knob defer: 0 marks in the sensing pass)
        l.defer = (l.pcache == 0 && l.nwx <= 2 && l.nwy <= 2 && tun.defer != 0) ? 1 : 0;
        const int rowb = l.pcache == 2 ? 4 : 8;                          // plane row bytes
        l.xp_off = l.map_bytes;                                          // rows (y, z): pd * ph * nwx words
        l.yp_off = l.xp_off + (uint32_t)(l.pd * l.ph * l.nwx * rowb);    // rows (x, z): pw * ph * nwy words
        l.agent_bytes = (l.yp_off + (uint32_t)(l.pw * l.ph * l.nwy * rowb) + 15u) & ~15u;
        l.plane_bytes = l.agent_bytes - l.xp_off;
    }
    return l;
}

// ----------------------------------------------------------------------------
// One agent's share of every mutable per-agent buffer, in bytes (0: the env
// has no such buffer).  The whole-env snapshots (voxnav_api.hip, snap_parts)
// and the per-agent gather (voxnav_gather.hip) both size their copies from
// this plan, so a buffer added here reaches both.  Each buffer is an array of
// N such rows, except that `wrec` follows the N hot words in the hot state's
// allocation and `pnz` follows the N stood blocks in theirs.
// ----------------------------------------------------------------------------
struct AgentParts {
    uint32_t hot = 0;       // the hot word
    uint32_t wrec = 0;      // CubicEnv: the window record, 16 columns x PH bytes
    uint32_t seed = 0;      // the next auto-reset seed
    uint32_t belief = 0;    // the belief block (EnvLayout::agent_bytes)
    uint32_t goal = 0;      // the goal word (allocated in both variants; simpleEnv uses it)
    uint32_t predraw = 0;   // the draw-ahead row (allocated in both variants; simpleEnv uses it)
    uint32_t stood = 0;     // plane-set mode 2: 32 stood rows
    uint32_t pnz = 0;       // plane-set mode 2: the nonzero-set mask (uint2)
    uint32_t episode = 0;   // the episode record: in a snapshot, not in a per-agent copy
    // what a per-agent copy moves
    uint32_t copied() const { return hot + wrec + seed + belief + goal + predraw + stood + pnz; }
};

inline AgentParts agent_parts(const EnvLayout &l) {
    AgentParts a;
    a.hot = 16u;
    a.wrec = l.variant != VN_VARIANT_SIMPLE ? 16u * (uint32_t)l.ph : 0u;
    a.seed = 4u;
    a.belief = l.agent_bytes;
    a.goal = 4u;
    a.predraw = 16u;
    if (l.variant != VN_VARIANT_SIMPLE && l.pcache == 2) {
        a.stood = 32u * 4u;
        a.pnz = 8u;
    }
    a.episode = l.episode_bytes;
    return a;
}

// The snapshot blob: the allocations in snap_parts' order (hot words + window
// records, seeds, belief blocks, goals, draw-ahead rows, episode records,
// stood rows + masks), each rounded up to SNAP_ALIGN bytes.
constexpr size_t SNAP_ALIGN = 256;
inline size_t snap_up(size_t bytes) { return (bytes + SNAP_ALIGN - 1) & ~(SNAP_ALIGN - 1); }
inline size_t snapshot_bytes(const AgentParts &a, size_t n) {
    size_t total = snap_up(n * (a.hot + a.wrec)) + snap_up(n * a.seed) + snap_up(n * a.belief) + snap_up(n * a.goal) +
                   snap_up(n * a.predraw) + snap_up(n * a.episode);
    if (a.stood) total += snap_up(n * (a.stood + a.pnz));
    return total;
}

// ----------------------------------------------------------------------------
// rooms -> descriptors, ray records, start lists
// ----------------------------------------------------------------------------
struct RayRec {   // 8 bytes, uploaded as the kernels' uint2: x = the +x,-x,+y,-y runs, y = +z,-z runs | wall<<16 | edge<<17
    uint32_t x, y;
};

struct RoomTables {
    std::vector<uint32_t> desc;         // 8 words per room (RoomDesc)
    std::vector<RayRec> rays;           // one record per cell, rooms concatenated
    std::vector<uint32_t> starts;       // interior free cells x | y<<8 | z<<16, rooms concatenated
    std::vector<uint32_t> total_free;   // per room
    int maxW = 0, maxD = 0, maxH = 0;
};

inline int build_room_tables(const VnRoomSet &rooms, const VnConfig &cfg, RoomTables *out) {
    const int nr = rooms.n_rooms;
    std::vector<uint32_t> &desc = out->desc;
    std::vector<RayRec> &rays = out->rays;
    std::vector<uint32_t> &starts = out->starts;
    std::vector<uint32_t> &total_free = out->total_free;
    desc.assign((size_t)nr * 8, 0);
    rays.clear();
    starts.clear();
    total_free.assign(nr, 0);
    int maxW = 0, maxD = 0, maxH = 0;
    size_t woff = 0;
    for (int r = 0; r < nr; ++r) {
        const int W = rooms.whd[3 * r], D = rooms.whd[3 * r + 1], H = rooms.whd[3 * r + 2];
        if (W < 1 || W > VN_MAX_W || D < 1 || D > VN_MAX_D || H < 1 || H > VN_MAX_H)
            return fail(VN_ERR_ROOM, "room %d: size %dx%dx%d outside 1..%d x 1..%d x 1..%d", r, W, D, H, VN_MAX_W,
                        VN_MAX_D, VN_MAX_H);
        const uint8_t *wall = rooms.walls + woff;
        auto is_wall = [&](int x, int y, int z) { return wall[((size_t)x * D + y) * H + z] != 0; };
        const uint32_t ray_off = (uint32_t)rays.size(), start_off = (uint32_t)starts.size();
        // interior scan in x -> y -> z order (envs/CubicEnv.py:450-457)
        uint32_t tf = 0;
        for (int x = 1; x < W - 1; ++x)
            for (int y = 1; y < D - 1; ++y)
                for (int z = 1; z < H - 1; ++z)
                    if (!is_wall(x, y, z)) {
                        starts.push_back((uint32_t)x | ((uint32_t)y << 8) | ((uint32_t)z << 16));
                        ++tf;
                    }
        if (tf == 0) return fail(VN_ERR_ROOM, "room %d has no interior free cell (random.choice of [])", r);
        total_free[r] = tf;
        // ray records
        static const int DX[6] = {1, -1, 0, 0, 0, 0}, DY[6] = {0, 0, 1, -1, 0, 0}, DZ[6] = {0, 0, 0, 0, 1, -1};
        for (int x = 0; x < W; ++x)
            for (int y = 0; y < D; ++y)
                for (int z = 0; z < H; ++z) {
                    uint32_t e8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    for (int d = 0; d < 6; ++d) {
                        int n = 0;
                        uint32_t wf = 0;
                        for (int s = 1;; ++s) {
                            const int nx = x + DX[d] * s, ny = y + DY[d] * s, nz = z + DZ[d] * s;
                            if (nx < 0 || nx >= W || ny < 0 || ny >= D || nz < 0 || nz >= H) break;
                            if (is_wall(nx, ny, nz)) {
                                wf = 1;
                                break;
                            }
                            ++n;
                        }
                        if (n > 127) {
                            n = 127;
                            wf = 0;
                        }
                        e8[d] = (uint32_t)n | (wf << 7);
                    }
                    e8[6] = is_wall(x, y, z) ? 1u : 0u;
                    RayRec rec;
                    rec.x = e8[0] | (e8[1] << 8) | (e8[2] << 16) | (e8[3] << 24);
                    rec.y = e8[4] | (e8[5] << 8) | (e8[6] << 16);
                    // bit 17: some ray from this cell ends at the room's edge (not a
                    // wall), i.e. may take the edge-quirk mark (simple_pipe_kernel)
                    for (int d = 0; d < 6; ++d)
                        if (!(e8[d] & 0x80u) && (e8[d] & 0x7fu) >= 1u && (e8[d] & 0x7fu) < 127u) rec.y |= 1u << 17;
                    rays.push_back(rec);
                }
        int32_t fixed = -1;
        if (rooms.fixed_start && rooms.fixed_start[3 * r] >= 0) {
            const int sx = rooms.fixed_start[3 * r], sy = rooms.fixed_start[3 * r + 1],
                      sz = rooms.fixed_start[3 * r + 2];
            if (sx >= W || sy < 0 || sy >= D || sz < 0 || sz >= H)
                return fail(VN_ERR_ROOM, "room %d: start position (%d,%d,%d) outside the room", r, sx, sy, sz);
            fixed = sx | (sy << 8) | (sz << 16);
        }
        int32_t fgoal = -1;
        if (rooms.goal && rooms.goal[3 * r] >= 0) {
            const int gx = rooms.goal[3 * r], gy = rooms.goal[3 * r + 1], gz = rooms.goal[3 * r + 2];
            if (gx >= W || gy < 0 || gy >= D || gz < 0 || gz >= H)
                return fail(VN_ERR_ROOM, "room %d: goal (%d,%d,%d) outside the room", r, gx, gy, gz);
            fgoal = gx | (gy << 8) | (gz << 16);
        }
        uint32_t *d = &desc[(size_t)r * 8];
        d[0] = (uint32_t)W | ((uint32_t)D << 8) | ((uint32_t)H << 16);
        d[1] = tf;
        d[2] = ray_off;
        d[3] = start_off;
        d[4] = (uint32_t)fixed;
        d[5] = (uint32_t)((W + 3) / 4) | ((uint32_t)((D + 3) / 4) << 16);
        {   // done <=> visited / total >= finish in f64 (CubicEnv.py:212-213); monotone in visited
            const double fin = cfg.finish_percentage == 0.0 ? 0.84 : cfg.finish_percentage;
            uint32_t v = 0;
            const uint32_t vmax = (uint32_t)W * D * H + 1;
            while (v < vmax && !((double)v / (double)tf >= fin)) ++v;
            d[6] = v;
        }
        d[7] = (uint32_t)fgoal;
        maxW = W > maxW ? W : maxW;
        maxD = D > maxD ? D : maxD;
        maxH = H > maxH ? H : maxH;
        woff += (size_t)W * D * H;
    }
    out->maxW = maxW;
    out->maxD = maxD;
    out->maxH = maxH;
    return VN_OK;
}

// ----------------------------------------------------------------------------
// Exact boxes: rooms whose ray records are arithmetic
// ----------------------------------------------------------------------------
// The ray record of free cell (x, y, z) of a W x D x H room that is one wall
// layer around a free interior: every run ends at the opposite wall.  The BOX
// step kernels (voxnav_env.hip) compute this instead of loading the record;
// room_is_exact_box below holds it against the table, so both sides read the
// one formula.
VN_HD RayRec box_ray_rec(int W, int D, int H, int x, int y, int z) {
    const uint32_t ex = (uint32_t)(W - 2 - x) | 0x80u, wx = (uint32_t)(x - 1) | 0x80u;
    const uint32_t ey = (uint32_t)(D - 2 - y) | 0x80u, wy = (uint32_t)(y - 1) | 0x80u;
    const uint32_t ez = (uint32_t)(H - 2 - z) | 0x80u, wz = (uint32_t)(z - 1) | 0x80u;
    RayRec r;
    r.x = ex | (wx << 8) | (ey << 16) | (wy << 24);
    r.y = ez | (wz << 8);
    return r;
}

// A room (its W * D * H records, build_room_tables' order) is an exact box when
// the record of every free cell equals box_ray_rec, both words: the six runs
// with their wall flags, and bits 16 / 17 clear.  The comparison is with what a
// kernel would have loaded, cell by cell, not a second reading of the walls: a
// pillar, a second wall layer, an opening in the shell or a run past 127 cells
// each change some free cell's record.  (Wall cells are never stood in: no
// kernel reads their runs.)
inline bool room_is_exact_box(int W, int D, int H, const RayRec *rays) {
    if (W < 3 || D < 3 || H < 3) return false;
    for (int x = 0; x < W; ++x)
        for (int y = 0; y < D; ++y)
            for (int z = 0; z < H; ++z) {
                const RayRec &t = rays[((size_t)x * D + y) * H + z];
                if ((t.y >> 16) & 1u) continue;   // a wall cell
                const RayRec f = box_ray_rec(W, D, H, x, y, z);
                if (t.x != f.x || t.y != f.y) return false;
            }
    return true;
}

// ... and an env is box-exact when every room of its set is (EnvLayout::box)
inline bool rooms_box_exact(const RoomTables &rt) {
    const size_t nr = rt.desc.size() / 8;
    if (nr == 0) return false;
    for (size_t r = 0; r < nr; ++r) {
        const uint32_t whd = rt.desc[8 * r], ray_off = rt.desc[8 * r + 2];
        if (!room_is_exact_box((int)(whd & 0xff), (int)((whd >> 8) & 0xff), (int)((whd >> 16) & 0xff),
                               rt.rays.data() + ray_off))
            return false;
    }
    return true;
}

// LDS table (TAB_SIZE floats, then the simpleEnv rewards: TAB_ALL in all):
// obs value of every belief byte (decode, clip to [-2, 20], (v + 2) / 22 in
// IEEE f32 -- :273-275), f32(a / 5.0) (:284) and f32(c / L) (:287), all
// computed on the host.
inline void fill_lut(int L, float *lut) {
    for (int k = 0; k < TAB_ALL; ++k) lut[k] = 0.0f;
    for (int ev = 0; ev < 16; ++ev) {   // simpleEnv compute_reward (:189-217) by event code, in its order
        volatile double r = -0.1;
        if (ev & 1) r = r + -10.0;
        if (ev & 2) r = r + 0.05;
        if (ev & 4) r = r + 100.0;
        if (ev & 8) r = r + 1.0;        // (the truncation term adds 0.0: no change)
        const double rv = r;
        lut[TAB_SREW + ev] = (float)rv;
        std::memcpy(&lut[TAB_SREW64 + 2 * ev], &rv, sizeof(double));
    }
    for (int b = 0; b < 256; ++b) {
        int v = (b & 0x80) ? ((b & 0x40) ? -2 : (b & 0x3f)) : -1;
        if (v > 20) v = 20;
        volatile float num = (float)(v + 2);
        lut[b] = num / 22.0f;
    }
    // plane-set staging codes (bytes no belief cell holds): tail values
    lut[TC_ZERO] = 0.0f;
    lut[TC_ONE] = 1.0f;
    for (int a = 0; a < 6; ++a) lut[TC_ACT + a] = (float)((double)a / 5.0);
    for (int c = 0; c <= L; ++c) lut[TC_CID + c] = (float)((double)c / (double)L);
    for (int a = 0; a < 6; ++a) lut[TAB_ACTION + a] = (float)((double)a / 5.0);
    for (int c = 0; c <= L; ++c) lut[TAB_CID + c] = (float)((double)c / (double)L);
}

// Plane-set mode, per room: the bricked byte map of a fresh episode -- 0x40
// (latent wall, still unknown) at every wall cell, 0 elsewhere; VN_WIMG_REP
// copies per room.
inline void wall_image(const VnRoomSet &rooms, const EnvLayout &l, std::vector<int8_t> *img) {
    const int nr = rooms.n_rooms;
    img->assign((size_t)nr * VN_WIMG_REP * l.map_bytes, 0);
    size_t wo = 0;
    for (int r = 0; r < nr; ++r) {
        const int W = rooms.whd[3 * r], D = rooms.whd[3 * r + 1], H = rooms.whd[3 * r + 2];
        int8_t *m = img->data() + (size_t)r * VN_WIMG_REP * l.map_bytes;
        for (int x = 0; x < W; ++x)
            for (int y = 0; y < D; ++y)
                for (int z = 0; z < H; ++z)
                    if (rooms.walls[wo + ((size_t)x * D + y) * H + z])
                        m[bcol(x, y, l.nby) * (size_t)l.ph + z] = 0x40;
        wo += (size_t)W * D * H;
        for (int c = 1; c < VN_WIMG_REP; ++c) std::memcpy(m + (size_t)c * l.map_bytes, m, l.map_bytes);
    }
}

}  // namespace
