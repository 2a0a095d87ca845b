// voxnav_api.hip -- the host side of the env boundary (include/voxnav.h):
// VnEnv, the process options, VnTuning validation and every extern "C" env
// entry point.  Host code only: no kernel and no device symbol.  vn_create
// plans on the host (env_plan.h: room tables, EnvLayout, LUT, room images),
// uploads the result and builds the env's Params once; a call copies that
// Params, sets its own pointers and hands it to the variant's kernel unit
// (vn_cubic: voxnav_env.hip, vn_simple: voxnav_simple.hip, the state import
// vn_state: voxnav_state.hip, the episode records vn_episode:
// voxnav_episode.hip, the per-agent gather vn_gather: voxnav_gather.hip;
// env_params.h).  The whole-env snapshots are host code here: device-to-device
// copies of the env's buffers under a tag; the per-agent copies between envs
// (vn_copy_agents) are checked here against the layout tag and run by vn_gather.

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "vn_common.h"
#include "env_params.h"
#include "env_plan.h"

#ifndef VN_WREC_K_DEFAULT
#define VN_WREC_K_DEFAULT 1  // VnTuning::wrec_k default: launches of at most this many steps write the window record
#endif
#ifndef VN_DFLUSH_DEFAULT
#define VN_DFLUSH_DEFAULT 1  // VnTuning::dflush default: bit 0 byte-mark kernels, bit 1 plane-set kernels
#endif

namespace {

using vn_detail::g_last_error;

// one owned device allocation
struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { (void)hipFree(ptr); }
    template <typename T>
    T *as() const { return static_cast<T *>(ptr); }
    hipError_t put(const void *src, size_t n) const { return hipMemcpy(ptr, src, n, hipMemcpyHostToDevice); }
};

}  // namespace

struct VnEnv {
    int device = 0;
    int N = 0;
    VnConfig cfg{};
    VnTuning tuning{};   // validated (check_tuning); launches and vn_kernel_label read the same copy
    EnvLayout lay;
    std::vector<uint32_t> total_free;
    // device buffers (device_bytes: their sum)
    DevBuf rooms, rays, starts, lut;
    DevBuf hot;       // the hot state, then (CubicEnv) the window records: 16 columns x PH bytes per agent (wrec_base)
    DevBuf seed;
    DevBuf belief;    // the belief maps (Params::belief may sit at an offset inside: placement study, vn_create)
    DevBuf err, envc, goal, predraw;
    DevBuf wimg;      // plane-set mode: the latent-wall room images
    DevBuf stood;     // PCM 2: per agent 32 stood rows, then per agent the nonzero-set masks (uint2)
    DevBuf scratch;   // 8 KiB: targets of dummy output stores (the deferred flush's first step)
    DevBuf episodes;  // per agent one EpisodeRec: totals and the last ended episode (vn_episode_records)
    size_t device_bytes = 0;
    Params params{};  // everything but the per-call fields (call_params), built once by vn_create
    bool wrec_written = false;    // the last step launch wrote every agent's window record (wrec_fill)
    uint64_t snap_tag = 0;        // hash of everything that decides what a snapshot's bytes mean (snapshot_tag)
    uint64_t layout_tag = 0;      // ... and of what decides one agent's bytes: the same without N, agent_id_base and
                                  // the episode buffer's size (vn_copy_agents)

    int alloc(DevBuf &b, size_t bytes) {
        const hipError_t he = hipMalloc(&b.ptr, bytes);
        if (he != hipSuccess) return fail(VN_ERR_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(he));
        b.bytes = bytes;
        device_bytes += bytes;
        return VN_OK;
    }
};

namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// The Params of one call: the env's, plus the launch-time tuning (vn_set_tuning
// changes it on a live env: scripts/ab_same.py); the caller sets its pointers.
Params call_params(const VnEnv *e) {
    Params p = e->params;
    p.prio = e->tuning.prio;       // bit 0: the step's load issue, 1: the obs flush, 6: base level (2: the rotation),
                                   // 3: a box-exact env's launches stay on the ray table
    p.dflush = e->tuning.dflush;   // bit 0: the deferred obs flush in the byte-mark kernels (PCM 3), bit 1: in the plane-set ones
    p.wrec_k = e->tuning.wrec_k;   // launches of at most this many steps write the window record
    return p;
}

int launch_env(bool reset_only, VnEnv *e, const Params &p, hipStream_t s) {
    const EnvLayout &l = e->lay;
    if (l.variant == VN_VARIANT_SIMPLE)
        return vn_simple::launch(reset_only, l.sline, l.sbits, e->cfg.local_map_length, e->N, l.obs_dim, &p, s);
    return vn_cubic::launch(reset_only, l.defer, e->tuning.wrec_early, &e->wrec_written, &p, s);
}

// the defaults of every VnTuning field, here only (vn_tuning_default)
constexpr VnTuning kTuningDefault = {/*pcache_cap*/ -1, /*defer*/ -1, /*simple_layout*/ 0, /*prio*/ 67,
                                     /*dflush*/ VN_DFLUSH_DEFAULT, /*wrec_k*/ VN_WREC_K_DEFAULT, /*wrec_early*/ 1};
constexpr int PRIO_USER_BITS = 1 | 2 | 4 | 8 | 64;   // what env_kernel and vn_cubic::launch decode of VnTuning::prio (launch adds its own bits)

int check_tuning(const VnTuning &t) {
    if (t.pcache_cap < -1 || t.pcache_cap > 2)
        return fail(VN_ERR_INVALID, "tuning.pcache_cap must be -1, 0, 1 or 2 (got %d)", t.pcache_cap);
    if (t.defer != -1 && t.defer != 0) return fail(VN_ERR_INVALID, "tuning.defer must be -1 or 0 (got %d)", t.defer);
    if (t.simple_layout < 0 || t.simple_layout > 2)
        return fail(VN_ERR_INVALID, "tuning.simple_layout must be 0, 1 or 2 (got %d)", t.simple_layout);
    if (t.prio & ~PRIO_USER_BITS)
        return fail(VN_ERR_INVALID, "tuning.prio must be a subset of bits %d (got %d)", PRIO_USER_BITS, t.prio);
    if (t.dflush < 0 || t.dflush > 3) return fail(VN_ERR_INVALID, "tuning.dflush must be in 0..3 (got %d)", t.dflush);
    if (t.wrec_k < 0) return fail(VN_ERR_INVALID, "tuning.wrec_k must be >= 0 (got %d)", t.wrec_k);
    if (t.wrec_early != 0 && t.wrec_early != 1)
        return fail(VN_ERR_INVALID, "tuning.wrec_early must be 0 or 1 (got %d)", t.wrec_early);
    return VN_OK;
}

// the process options by VN_OPT_* index: values 0..max, and (below) the defaults
constexpr int32_t kOptionMax[vn_detail::N_OPTIONS] = {2, 1, 1, 1};

// vn_create's device half: the buffers of a planned env, in one order for
// allocation (first failure: VN_ERR_OOM) ...
int alloc_buffers(VnEnv *e, const RoomTables &rt, size_t belief_alloc_bytes, bool belief_contig) {
    const EnvLayout &l = e->lay;
    const AgentParts ap = agent_parts(l);   // the per-agent buffers' row sizes (env_plan.h)
    const size_t n = (size_t)e->N, nr = rt.total_free.size();
    int rc = e->alloc(e->rooms, rt.desc.size() * sizeof(uint32_t));
    if (!rc) rc = e->alloc(e->rays, rt.rays.size() * sizeof(RayRec));
    if (!rc) rc = e->alloc(e->starts, rt.starts.size() * sizeof(uint32_t));
    if (!rc) rc = e->alloc(e->lut, TAB_ALL * sizeof(float));
    if (!rc) rc = e->alloc(e->hot, n * ((size_t)ap.hot + ap.wrec));
    if (!rc) rc = e->alloc(e->seed, n * ap.seed);
    // The belief maps.  A VMM-mapped variant (hipMemCreate / hipMemMap
    // chunks) was measured in round 6 and removed: on that memory the
    // kernels' results differed from the oracle, and it did not remove the
    // P-set kernels' trial-to-trial swing.  The cause of the
    // mismatch is not identified: the logs show marks written by one launch
    // not seen by the first step of the next (Weak #1).
    if (!rc && belief_contig) {
        const hipError_t ce = hipExtMallocWithFlags(&e->belief.ptr, belief_alloc_bytes, hipDeviceMallocContiguous);
        if (ce != hipSuccess)
            return fail(VN_ERR_OOM, "hipExtMallocWithFlags(%zu, contiguous) failed: %s", belief_alloc_bytes,
                        hipGetErrorString(ce));
        e->belief.bytes = belief_alloc_bytes;
        e->device_bytes += belief_alloc_bytes;
    } else if (!rc) {
        rc = e->alloc(e->belief, belief_alloc_bytes);
    }
    if (!rc) rc = e->alloc(e->err, sizeof(int32_t));
    if (!rc) rc = e->alloc(e->envc, sizeof(EnvConst));
    if (!rc) rc = e->alloc(e->goal, n * ap.goal);
    if (!rc) rc = e->alloc(e->predraw, n * ap.predraw);
    if (!rc && l.pcache) rc = e->alloc(e->wimg, nr * VN_WIMG_REP * l.map_bytes);
    if (!rc && ap.stood) rc = e->alloc(e->stood, n * ((size_t)ap.stood + ap.pnz));
    if (!rc) rc = e->alloc(e->scratch, 8192);
    // after every other buffer: none of them moves (allocation placement alone swings the rate)
    if (!rc) rc = e->alloc(e->episodes, n * (size_t)ap.episode);
    return rc;
}

// ... and for the upload (first failure returned; e->params holds the device pointers)
hipError_t upload(VnEnv *e, const VnRoomSet &rooms, const RoomTables &rt, const float *lut) {
    const EnvLayout &l = e->lay;
    const Params &p = e->params;
    const size_t n = (size_t)e->N;
    if (hipError_t he = e->rooms.put(rt.desc.data(), e->rooms.bytes)) return he;
    if (hipError_t he = e->rays.put(rt.rays.data(), e->rays.bytes)) return he;
    if (hipError_t he = e->starts.put(rt.starts.data(), e->starts.bytes)) return he;
    if (hipError_t he = e->lut.put(lut, e->lut.bytes)) return he;
    if (hipError_t he = hipMemset(p.hot, 0, n * sizeof(uint4))) return he;
    if (hipError_t he = hipMemset(p.next_seed, 0, e->seed.bytes)) return he;
    // unknown: 0x00 in the CubicEnv byte encoding, -1 (0xFF) in the dense simpleEnv map; empty bit planes
    if (hipError_t he = hipMemset(p.belief, l.variant == VN_VARIANT_SIMPLE && !l.sbits ? 0xFF : 0x00, (size_t)l.agent_bytes * n))
        return he;
    if (hipError_t he = hipMemset(p.goal, 0, e->goal.bytes)) return he;
    if (hipError_t he = hipMemset(p.predraw, 0, e->predraw.bytes)) return he;
    if (hipError_t he = hipMemset(p.err, 0, e->err.bytes)) return he;
    if (p.stood)
        if (hipError_t he = hipMemset(p.stood, 0, e->stood.bytes)) return he;
    if (hipError_t he = hipMemset(e->episodes.ptr, 0, e->episodes.bytes)) return he;
    if (l.pcache) {
        std::vector<int8_t> img;
        wall_image(rooms, l, &img);
        if (hipError_t he = e->wimg.put(img.data(), img.size())) return he;
    }
    EnvConst ec;
    std::memset(&ec, 0, sizeof(ec));
    ec.rooms = p.rooms;
    ec.rays = p.rays;
    ec.starts = p.starts;
    ec.err = p.err;
    ec.n_rooms = p.n_rooms;
    ec.use_room_draw = p.use_room_draw;
    ec.nby = l.nby;
    ec.agent_bytes = l.agent_bytes;
    ec.xp_off = l.xp_off;
    ec.map_bytes = l.map_bytes;
    ec.plane_bytes = l.plane_bytes;
    ec.pcache = l.pcache;
    ec.wimg = e->wimg.as<const uint4>();
    ec.episodes = e->episodes.as<uint4>();
    if (hipError_t he = e->envc.put(&ec, sizeof(ec))) return he;
    return hipDeviceSynchronize();
}

// the env's Params: the layout, the config and the device buffers (belief_off:
// where the maps start inside their allocation)
Params env_params(const VnEnv *e, size_t belief_off) {
    const EnvLayout &l = e->lay;
    Params p;
    std::memset(&p, 0, sizeof(p));
    p.envc = e->envc.as<const EnvConst>();
    p.hot = e->hot.as<uint4>();
    p.next_seed = e->seed.as<uint32_t>();
    p.belief = e->belief.as<int8_t>() + belief_off;
    p.rooms = e->rooms.as<const uint4>();
    p.rays = e->rays.as<const uint2>();
    p.starts = e->starts.as<const uint32_t>();
    p.lut = e->lut.as<const float>();
    p.err = e->err.as<int32_t>();
    p.N = e->N;
    p.L = e->cfg.local_map_length;
    p.nby = l.nby;
    p.ph = l.ph;
    p.map_bytes = l.map_bytes;
    p.agent_bytes = l.agent_bytes;
    p.xp_off = l.xp_off;
    p.yp_off = l.yp_off;
    p.nwx = l.nwx;
    p.nwy = l.nwy;
    p.n_rooms = (int)e->total_free.size();
    p.use_room_draw = e->cfg.use_room_draw;
    p.autoreset = e->cfg.autoreset;
    p.seed_stride = (uint32_t)(uint64_t)e->cfg.seed_stride;
    p.crash_penalty = e->cfg.crash_penalty;
    p.finish = e->cfg.finish_percentage;
    p.gid_base = (uint64_t)e->cfg.agent_id_base;
    p.K = 1;
    p.variant = l.variant;
    p.obs_dim = l.obs_dim;
    p.pd = l.pd;
    p.goal = e->goal.as<uint32_t>();
    p.predraw = e->predraw.as<uint4>();
    p.sbits = l.sbits;
    p.sy_off = l.sy_off;
    p.sz_off = l.sz_off;
    p.qz_off = l.qz_off;
    p.sline = l.sline;
    p.wimg = e->wimg.as<const int8_t>();
    p.pcache = l.pcache;
    p.box = (uint32_t)l.box;
    p.scratch = e->scratch.as<float>();
    p.stood = e->stood.as<uint32_t>();
    p.pnz = p.stood ? reinterpret_cast<uint2 *>(p.stood + (size_t)e->N * 32u) : nullptr;
    return p;
}

// ---- whole-env snapshots: every mutable per-agent buffer, in one order ----
struct SnapPart {
    void *ptr;
    size_t bytes;
};

// hot state with the window records behind it, next seeds, belief blocks,
// goals, the simpleEnv draw-ahead, the episode records, stood rows with the
// nonzero-set masks; N rows each of the size agent_parts plans (env_plan.h:
// snapshot_bytes lays the blob out in this order, each part on a SNAP_ALIGN
// boundary)
constexpr int SNAP_MAX_PARTS = 7;
int snap_parts(const VnEnv *e, SnapPart out[SNAP_MAX_PARTS]) {
    const AgentParts ap = agent_parts(e->lay);
    const size_t N = (size_t)e->N;
    int n = 0;
    out[n++] = {e->hot.ptr, N * ((size_t)ap.hot + ap.wrec)};
    out[n++] = {e->seed.ptr, N * ap.seed};
    out[n++] = {e->params.belief, N * ap.belief};
    out[n++] = {e->goal.ptr, N * ap.goal};
    out[n++] = {e->predraw.ptr, N * ap.predraw};
    out[n++] = {e->episodes.ptr, N * ap.episode};
    if (ap.stood) out[n++] = {e->stood.ptr, N * ((size_t)ap.stood + ap.pnz)};
    return n;
}

// FNV-1a over the values that decide the bytes' meaning: ABI version, variant,
// N, L, the planned layout, the creation-time tuning, the config and the room
// tables.  Host arithmetic only.
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void *p, size_t n) {
        const unsigned char *c = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
    }
    template <typename T>
    void val(T v) { bytes(&v, sizeof(v)); }
};

// whole_env false: the layout tag -- what decides one agent's bytes, i.e. the
// same list without N, agent_id_base and the episode buffer's size
uint64_t snapshot_tag(const VnEnv *e, const RoomTables &rt, bool whole_env) {
    const EnvLayout &l = e->lay;
    Fnv f;
    f.val<int32_t>(VN_ABI_VERSION);
    f.val<int32_t>(l.variant);
    if (whole_env) f.val<int32_t>(e->N);
    f.val<int32_t>(e->cfg.local_map_length);
    for (const int32_t v : {l.obs_dim, l.pw, l.pd, l.ph, l.nbx, l.nby, l.nwx, l.nwy, l.sbits, l.sline, l.defer, l.pcache})
        f.val<int32_t>(v);
    for (const uint32_t v : {l.map_bytes, l.agent_bytes, l.plane_bytes, l.xp_off, l.yp_off, l.sy_off, l.sz_off, l.qz_off})
        f.val<uint32_t>(v);
    if (whole_env) f.val<uint64_t>((uint64_t)e->episodes.bytes);   // the episode records travel with a snapshot
    f.val<int32_t>(e->tuning.pcache_cap);
    f.val<int32_t>(e->tuning.defer);
    f.val<int32_t>(e->tuning.simple_layout);
    f.val<int32_t>(e->cfg.use_room_draw);
    f.val<int32_t>(e->cfg.autoreset);
    f.val<double>(e->cfg.crash_penalty);
    f.val<double>(e->cfg.finish_percentage);
    if (whole_env) f.val<int64_t>(e->cfg.agent_id_base);
    f.val<int64_t>(e->cfg.seed_stride);
    f.bytes(rt.desc.data(), rt.desc.size() * sizeof(uint32_t));
    f.bytes(rt.rays.data(), rt.rays.size() * sizeof(RayRec));
    f.bytes(rt.starts.data(), rt.starts.size() * sizeof(uint32_t));
    return f.h;
}

}  // namespace

std::atomic<int32_t> vn_detail::g_options[vn_detail::N_OPTIONS] = {{0}, {1}, {1}, {0}};

extern "C" {

const char *vn_last_error(void) { return g_last_error.c_str(); }

int vn_abi_version(void) { return VN_ABI_VERSION; }

int vn_set_option(int32_t option, int32_t value) {
    if (option < 0 || option >= vn_detail::N_OPTIONS) return fail(VN_ERR_INVALID, "unknown option %d", option);
    if (value < 0 || value > kOptionMax[option])
        return fail(VN_ERR_INVALID, "option %d takes 0..%d (got %d)", option, kOptionMax[option], value);
    vn_detail::g_options[option].store(value, std::memory_order_relaxed);
    return VN_OK;
}

int vn_get_option(int32_t option, int32_t *value) {
    if (!value) return fail(VN_ERR_INVALID, "NULL argument");
    if (option < 0 || option >= vn_detail::N_OPTIONS) return fail(VN_ERR_INVALID, "unknown option %d", option);
    *value = vn_detail::option(option);
    return VN_OK;
}

int vn_tuning_default(VnTuning *out) {
    if (!out) return fail(VN_ERR_INVALID, "NULL argument");
    *out = kTuningDefault;
    return VN_OK;
}

int vn_set_tuning(VnEnv *env, const VnTuning *tuning) {
    if (!env || !tuning) return fail(VN_ERR_INVALID, "NULL argument");
    if (const int rc = check_tuning(*tuning)) return rc;
    const VnTuning &cur = env->tuning;
    if (tuning->pcache_cap != cur.pcache_cap)
        return fail(VN_ERR_INVALID, "tuning.pcache_cap is fixed at creation (%d, got %d)", cur.pcache_cap, tuning->pcache_cap);
    if (tuning->defer != cur.defer)
        return fail(VN_ERR_INVALID, "tuning.defer is fixed at creation (%d, got %d)", cur.defer, tuning->defer);
    if (tuning->simple_layout != cur.simple_layout)
        return fail(VN_ERR_INVALID, "tuning.simple_layout is fixed at creation (%d, got %d)", cur.simple_layout,
                    tuning->simple_layout);
    env->tuning = *tuning;
    return VN_OK;
}

int vn_create(const VnRoomSet *rooms, int32_t n_agents, const VnConfig *cfg, int32_t device, VnEnv **out) {
    return vn_create_tuned(rooms, n_agents, cfg, device, nullptr, out);
}

int vn_create_tuned(const VnRoomSet *rooms, int32_t n_agents, const VnConfig *cfg, int32_t device,
                    const VnTuning *tuning, VnEnv **out) {
    if (!rooms || !cfg || !out) return fail(VN_ERR_INVALID, "NULL argument");
    *out = nullptr;
    const VnTuning tun = tuning ? *tuning : kTuningDefault;
    if (const int rc = check_tuning(tun)) return rc;
    if (n_agents <= 0) return fail(VN_ERR_INVALID, "n_agents must be > 0 (got %d)", n_agents);
    if (rooms->n_rooms <= 0 || rooms->n_rooms > VN_MAX_ROOMS)
        return fail(VN_ERR_INVALID, "n_rooms must be in 1..%d (got %d)", VN_MAX_ROOMS, rooms->n_rooms);
    if (!rooms->whd || !rooms->walls) return fail(VN_ERR_INVALID, "rooms->whd / rooms->walls is NULL");
    if (cfg->local_map_length < 1 || cfg->local_map_length > VN_MAX_L)
        return fail(VN_ERR_INVALID, "local_map_length must be in 1..%d (got %d)", VN_MAX_L, cfg->local_map_length);
    if (cfg->variant != VN_VARIANT_CUBIC && cfg->variant != VN_VARIANT_SIMPLE)
        return fail(VN_ERR_INVALID, "variant must be %d (CubicEnv) or %d (simpleEnv), got %d", VN_VARIANT_CUBIC,
                    VN_VARIANT_SIMPLE, cfg->variant);

    // ---- the plan: host arithmetic only (env_plan.h) ----
    RoomTables rt;
    if (const int rc = build_room_tables(*rooms, *cfg, &rt)) return rc;
    float lut[TAB_ALL];
    fill_lut(cfg->local_map_length, lut);

    DeviceGuard dg(device);   // before the env: an error return frees the buffers on `device`
    std::unique_ptr<VnEnv> e(new (std::nothrow) VnEnv());
    if (!e) return fail(VN_ERR_OOM, "host allocation failed");
    e->device = device;
    e->N = n_agents;
    e->cfg = *cfg;
    e->tuning = tun;
    if (e->cfg.finish_percentage == 0.0) e->cfg.finish_percentage = 0.84;
    if (e->cfg.seed_stride == 0) e->cfg.seed_stride = n_agents;
    e->total_free = rt.total_free;
    e->lay = plan_layout(cfg->variant, cfg->local_map_length, rt.maxW, rt.maxD, rt.maxH, tun);
    // every free cell's ray record held against the box formula: the step kernels may compute it (env_kernel's BOX)
    e->lay.box = cfg->variant == VN_VARIANT_CUBIC && rooms_box_exact(rt) ? 1 : 0;
    size_t belief_off = 0;
    bool belief_contig = false;
#ifdef VN_DIAG
    // placement study (diagnostics build): VOXNAV_AGENT_PAD extra bytes of per-agent
    // stride (CubicEnv); VOXNAV_BELIEF_OFFSET bytes into the allocation;
    // VOXNAV_BELIEF_CONTIG=1 a physically contiguous allocation
    // (hipDeviceMallocContiguous)
    if (const char *ap = getenv("VOXNAV_AGENT_PAD"))
        if (cfg->variant != VN_VARIANT_SIMPLE) e->lay.agent_bytes += ((uint32_t)atoi(ap) + 15u) & ~15u;
    if (const char *bo = getenv("VOXNAV_BELIEF_OFFSET")) belief_off = (((size_t)atoll(bo)) + 255u) & ~(size_t)255u;
    const char *bc = getenv("VOXNAV_BELIEF_CONTIG");
    belief_contig = bc && bc[0] == '1';
#endif

    // ---- the device: MT tables, buffers, upload ----
    if (const int rc = vn_cubic::ensure_mt(device)) return rc;
    if (const int rc = vn_simple::ensure_mt(device)) return rc;
    const size_t belief_bytes = (size_t)e->lay.agent_bytes * (size_t)n_agents;
    if (const int rc = alloc_buffers(e.get(), rt, belief_bytes + belief_off, belief_contig)) return rc;
    e->params = env_params(e.get(), belief_off);
    e->snap_tag = snapshot_tag(e.get(), rt, true);
    e->layout_tag = snapshot_tag(e.get(), rt, false);
    if (const hipError_t he = upload(e.get(), *rooms, rt, lut))
        return fail(VN_ERR_HIP, "vn_create upload: %s", hipGetErrorString(he));
    *out = e.release();
    return VN_OK;
}

int vn_destroy(VnEnv *env) {
    if (!env) return VN_OK;
    DeviceGuard dg(env->device);
    (void)hipDeviceSynchronize();
    delete env;
    return VN_OK;
}

int vn_get_info(const VnEnv *env, VnInfo *info) {
    if (!env || !info) return fail(VN_ERR_INVALID, "NULL argument");
    info->n_agents = env->N;
    info->n_rooms = env->params.n_rooms;
    info->local_map_length = env->cfg.local_map_length;
    info->pad_w = env->lay.pw;
    info->pad_d = env->lay.pd;
    info->pad_h = env->lay.ph;
    info->belief_bytes_per_agent = env->lay.agent_bytes;
    info->device_bytes = (int64_t)env->device_bytes;
    info->variant = env->lay.variant;
    info->obs_dim = env->lay.obs_dim;
    return VN_OK;
}

int vn_reset(VnEnv *env, const int64_t *seeds, const uint8_t *mask, float *obs, void *stream) {
    if (!env || !seeds || !obs) return fail(VN_ERR_INVALID, "NULL argument");
    DeviceGuard dg(env->device);
    Params p = call_params(env);
    p.seeds = seeds;
    p.mask = mask;
    p.obs = obs;
    return launch_env(true, env, p, (hipStream_t)stream);
}

int vn_step(VnEnv *env, const int32_t *actions, float *obs, float *reward, double *reward64, uint8_t *terminated,
            uint8_t *truncated, float *terminal_obs, void *stream) {
    if (!env || !actions || !obs) return fail(VN_ERR_INVALID, "NULL argument");
    DeviceGuard dg(env->device);
    Params p = call_params(env);
    p.actions = actions;
    p.obs = obs;
    p.reward = reward;
    p.reward64 = reward64;
    p.term = terminated;
    p.trunc = truncated;
    p.terminal_obs = terminal_obs;
    return launch_env(false, env, p, (hipStream_t)stream);
}

int vn_step_random(VnEnv *env, uint64_t policy_seed, uint64_t t0, int32_t k_steps, int32_t *actions_out, float *obs,
                   float *reward, double *reward64, uint8_t *terminated, uint8_t *truncated, float *terminal_obs,
                   void *stream) {
    if (!env || !obs) return fail(VN_ERR_INVALID, "NULL argument");
    if (k_steps < 1) return fail(VN_ERR_INVALID, "k_steps must be >= 1 (got %d)", k_steps);
    DeviceGuard dg(env->device);
    Params p = call_params(env);
    p.K = k_steps;
    p.policy_seed = policy_seed;
    p.t0 = t0;
    p.actions_out = actions_out;
    p.obs = obs;
    p.reward = reward;
    p.reward64 = reward64;
    p.term = terminated;
    p.trunc = truncated;
    p.terminal_obs = terminal_obs;
    return launch_env(false, env, p, (hipStream_t)stream);
}

int vn_step_actions(VnEnv *env, const int32_t *actions, int32_t k_steps, float *obs, float *reward, double *reward64,
                    uint8_t *terminated, uint8_t *truncated, float *terminal_obs, void *stream) {
    if (!env || !actions || !obs) return fail(VN_ERR_INVALID, "NULL argument");
    if (k_steps < 1) return fail(VN_ERR_INVALID, "k_steps must be >= 1 (got %d)", k_steps);
    DeviceGuard dg(env->device);
    Params p = call_params(env);
    p.K = k_steps;      // vn_step's launch with k_steps steps in it: actions [k_steps][N], t0 = 0
    p.t0 = 0;
    p.actions = actions;
    p.obs = obs;
    p.reward = reward;
    p.reward64 = reward64;
    p.term = terminated;
    p.trunc = truncated;
    p.terminal_obs = terminal_obs;
    return launch_env(false, env, p, (hipStream_t)stream);
}

int vn_kernel_label(const VnEnv *env, int32_t k_steps, int32_t explicit_actions, int32_t fast, char *buf,
                    int32_t len) {
    if (!env || !buf || len < 1) return fail(VN_ERR_INVALID, "NULL argument");
    const EnvLayout &l = env->lay;
    const bool reset_only = k_steps == 0, ext = explicit_actions != 0;
    Params p = call_params(env);
    p.K = k_steps;
    const std::string s = l.variant == VN_VARIANT_SIMPLE
                              ? vn_simple::label(reset_only, ext, l.sline, l.sbits, env->cfg.local_map_length)
                              : vn_cubic::label(reset_only, ext, fast != 0, l.defer, &p);
    std::snprintf(buf, (size_t)len, "%s", s.c_str());
    return (int)s.size() < len ? VN_OK : fail(VN_ERR_INVALID, "buffer too small (%d)", (int)len);
}

int vn_kernel_box(const VnEnv *env, int32_t k_steps, int32_t explicit_actions, int32_t fast, int32_t *box) {
    if (!env || !box) return fail(VN_ERR_INVALID, "NULL argument");
    bool b = false;
    if (env->lay.variant != VN_VARIANT_SIMPLE) {
        Params p = call_params(env);
        p.K = k_steps;
        (void)vn_cubic::label(k_steps == 0, explicit_actions != 0, fast != 0, env->lay.defer, &p, &b);
    }
    *box = b ? 1 : 0;
    return VN_OK;
}

int vn_export_state(VnEnv *env, int64_t *state_out, void *stream) {
    if (!env || !state_out) return fail(VN_ERR_INVALID, "NULL argument");
    DeviceGuard dg(env->device);
    const Params p = call_params(env);
    return vn_cubic::export_state(&p, state_out, (hipStream_t)stream);
}

int vn_export_belief(VnEnv *env, int8_t *belief_out, void *stream) {
    if (!env || !belief_out) return fail(VN_ERR_INVALID, "NULL argument");
    DeviceGuard dg(env->device);
    const Params p = call_params(env);
    if (env->lay.variant == VN_VARIANT_SIMPLE)
        return vn_simple::export_belief(&p, belief_out, env->lay.pw, env->lay.pd, (hipStream_t)stream);
    return vn_cubic::export_belief(&p, belief_out, env->lay.pw, env->lay.pd, (hipStream_t)stream);
}

int vn_import_state(VnEnv *env, const int64_t *state, const int8_t *belief, const uint8_t *mask, float *obs,
                    int32_t *n_rejected, void *stream) {
    if (!env || !state || !belief) return fail(VN_ERR_INVALID, "NULL argument");
    if (env->lay.variant == VN_VARIANT_SIMPLE)
        return fail(VN_ERR_INVALID, "vn_import_state: the simpleEnv variant has no portable import (its dense map "
                                    "does not determine the device state); use vn_snapshot_save / vn_snapshot_load");
    DeviceGuard dg(env->device);
    const Params p = call_params(env);
    // an imported agent's window record is stale (its hot word says so); the
    // other agents' records stay valid and are loaded after the state
    env->wrec_written = false;
    return vn_state::import_state(&p, state, belief, mask, obs, n_rejected, env->lay.pw, env->lay.pd,
                                  (hipStream_t)stream);
}

int vn_episode_records(VnEnv *env, int64_t *out, void *stream) {
    if (!env || !out) return fail(VN_ERR_INVALID, "NULL argument");
    DeviceGuard dg(env->device);
    return vn_episode::records(env->episodes.ptr, env->N, out, (hipStream_t)stream);
}

int vn_episode_totals(VnEnv *env, int64_t *out, void *stream) {
    if (!env || !out) return fail(VN_ERR_INVALID, "NULL argument");
    DeviceGuard dg(env->device);
    return vn_episode::totals(env->episodes.ptr, env->N, out, (hipStream_t)stream);
}

int vn_episode_clear(VnEnv *env, const uint8_t *mask, void *stream) {
    if (!env) return fail(VN_ERR_INVALID, "NULL argument");
    DeviceGuard dg(env->device);
    return vn_episode::clear(env->episodes.ptr, env->N, mask, (hipStream_t)stream);
}

int vn_snapshot_tag(const VnEnv *env, uint64_t *tag) {
    if (!env || !tag) return fail(VN_ERR_INVALID, "NULL argument");
    *tag = env->snap_tag;
    return VN_OK;
}

int vn_snapshot_bytes(const VnEnv *env, int64_t *bytes) {
    if (!env || !bytes) return fail(VN_ERR_INVALID, "NULL argument");
    *bytes = (int64_t)snapshot_bytes(agent_parts(env->lay), (size_t)env->N);
    return VN_OK;
}

int vn_snapshot_save(VnEnv *env, void *dst, void *stream) {
    if (!env || !dst) return fail(VN_ERR_INVALID, "NULL argument");
    DeviceGuard dg(env->device);
    SnapPart parts[SNAP_MAX_PARTS];
    const int n = snap_parts(env, parts);
    char *d = static_cast<char *>(dst);
    for (int k = 0; k < n; ++k) {
        VN_HIP(hipMemcpyAsync(d, parts[k].ptr, parts[k].bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        d += snap_up(parts[k].bytes);
    }
    return VN_OK;
}

int vn_snapshot_load(VnEnv *env, const void *src, uint64_t tag, void *stream) {
    if (!env || !src) return fail(VN_ERR_INVALID, "NULL argument");
    if (tag != env->snap_tag)
        return fail(VN_ERR_INVALID, "vn_snapshot_load: the snapshot's tag %016llx is not this env's (%016llx): "
                                    "another variant, size, layout, tuning, config or room set",
                    (unsigned long long)tag, (unsigned long long)env->snap_tag);
    DeviceGuard dg(env->device);
    SnapPart parts[SNAP_MAX_PARTS];
    const int n = snap_parts(env, parts);
    const char *s = static_cast<const char *>(src);
    for (int k = 0; k < n; ++k) {
        VN_HIP(hipMemcpyAsync(parts[k].ptr, s, parts[k].bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        s += snap_up(parts[k].bytes);
    }
    // the copied hot words carry their window-record bits and the records came
    // with them, so the next launch reads each record after its state
    env->wrec_written = false;
    return VN_OK;
}

int vn_copy_agents(VnEnv *dst, const VnEnv *src, const int32_t *src_index, const int64_t *seeds, int32_t *n_rejected,
                   void *stream) {
    if (!dst || !src || !src_index) return fail(VN_ERR_INVALID, "NULL argument");
    if (dst->device != src->device)
        return fail(VN_ERR_INVALID, "vn_copy_agents: the envs are on devices %d and %d (no cross-device copy)",
                    dst->device, src->device);
    if (dst->layout_tag != src->layout_tag)
        return fail(VN_ERR_INVALID, "vn_copy_agents: the envs' layout tags differ (%016llx, %016llx): another variant, "
                                    "local_map_length, layout, creation-time tuning, config or room set",
                    (unsigned long long)dst->layout_tag, (unsigned long long)src->layout_tag);
    DeviceGuard dg(dst->device);
    const Params pd = call_params(dst), ps = call_params(src);
    // a copied hot word keeps its window-record bit and the record came with
    // it: the next launch reads each record after its state (vn_snapshot_load)
    dst->wrec_written = false;
    const AgentParts ap = agent_parts(dst->lay);
    return vn_gather::copy_agents(&pd, &ps, &ap, src_index, seeds, n_rejected, (hipStream_t)stream);
}

int vn_plan_frontier(VnEnv *env, const uint8_t *mask, int32_t *actions, int32_t *dist, void *stream) {
    if (!env || !actions) return fail(VN_ERR_INVALID, "NULL argument");
    if (env->lay.variant == VN_VARIANT_SIMPLE)
        return fail(VN_ERR_INVALID, "vn_plan_frontier: the simpleEnv variant has no frontier planner (CubicEnv only)");
    if (env->lay.pw > 64 || env->lay.pd > 64)
        return fail(VN_ERR_INVALID, "vn_plan_frontier: padded room %d x %d is wider or deeper than 64 (one 64-bit row "
                                    "over x per (y, z))", env->lay.pw, env->lay.pd);
    DeviceGuard dg(env->device);
    const Params p = call_params(env);
    return vn_plan::frontier(&p, mask, actions, dist, env->lay.pw, env->lay.pd, (hipStream_t)stream);
}

int vn_plan_frontier_dists(VnEnv *env, const uint8_t *mask, int32_t *actions, int32_t *dist, int32_t *dists,
                           uint8_t *best, void *stream) {
    if (!env || !dists) return fail(VN_ERR_INVALID, "NULL argument");
    if (env->lay.variant == VN_VARIANT_SIMPLE)
        return fail(VN_ERR_INVALID, "vn_plan_frontier_dists: the simpleEnv variant has no frontier planner (CubicEnv "
                                    "only)");
    if (env->lay.pw > 64 || env->lay.pd > 64)
        return fail(VN_ERR_INVALID, "vn_plan_frontier_dists: padded room %d x %d is wider or deeper than 64 (one "
                                    "64-bit row over x per (y, z))", env->lay.pw, env->lay.pd);
    DeviceGuard dg(env->device);
    const Params p = call_params(env);
    return vn_plan::frontier_dists(&p, mask, actions, dist, dists, best, env->lay.pw, env->lay.pd, (hipStream_t)stream);
}

#ifdef VN_DIAG
// diagnostics build (placement study): the device address of the belief maps and the per-agent stride
int vn_debug_belief_addr(const VnEnv *env, uint64_t *addr, uint32_t *stride) {
    if (!env || !addr || !stride) return fail(VN_ERR_INVALID, "NULL argument");
    *addr = (uint64_t)(uintptr_t)env->params.belief;
    *stride = env->lay.agent_bytes;
    return VN_OK;
}
#endif

int vn_gae(const float *rewards, const float *values, const float *episode_starts, const float *last_values,
           const float *dones, int32_t T, int32_t N, double gamma, double gae_lambda, float *advantages,
           float *returns, void *stream) {
    if (!rewards || !values || !episode_starts || !last_values || !dones || !advantages || !returns)
        return fail(VN_ERR_INVALID, "NULL argument");
    if (T < 1 || N < 1) return fail(VN_ERR_INVALID, "T and N must be >= 1 (got %d, %d)", T, N);
    const float g32 = (float)gamma;
    const float gl32 = (float)(gamma * gae_lambda);
    return vn_cubic::gae(rewards, values, episode_starts, last_values, dones, T, N, g32, gl32, advantages, returns,
                         (hipStream_t)stream);
}

}  // extern "C"
