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
// This file is the CubicEnv kernel unit: the device code, gae_kernel, and at
// the end the vn_cubic interface (env_params.h) -- which env_kernel
// instantiation a call launches, its label, and the state / belief exports.
// The C-ABI entry points, VnEnv and the host-side planning (room tables,
// per-agent layout, LUT) are in voxnav_api.hip and env_plan.h.

#include "env_core.h"

namespace {

template <int PH>
struct Col {
    static constexpr int NQ = PH / 8;     // 64-bit words per column
    uint64_t w[NQ];
};

template <int PH>
__device__ __forceinline__ void col_zero(Col<PH> &c) {
#pragma unroll
    for (int k = 0; k < Col<PH>::NQ; ++k) c.w[k] = 0ull;
}

template <int PH>
__device__ __forceinline__ void col_load(const int8_t *p, Col<PH> &c) {
    if constexpr (PH == 8) {
        c.w[0] = *reinterpret_cast<const uint64_t *>(p);
    } else {
#pragma unroll
        for (int k = 0; k < PH / 16; ++k) {
            const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(p)[k];
            c.w[2 * k] = v.x;
            c.w[2 * k + 1] = v.y;
        }
    }
}

template <int PH>
__device__ __forceinline__ void col_store(int8_t *p, const Col<PH> &c) {
    if constexpr (PH == 8) {
        *reinterpret_cast<uint64_t *>(p) = c.w[0];
    } else {
#pragma unroll
        for (int k = 0; k < PH / 16; ++k)
            reinterpret_cast<ulonglong2 *>(p)[k] = make_ulonglong2(c.w[2 * k], c.w[2 * k + 1]);
    }
}

// word holding byte i (i in [0, PH)), 0 outside
template <int PH>
__device__ __forceinline__ uint64_t col_word(const Col<PH> &c, int k) {
    if constexpr (PH == 8) {
        return k == 0 ? c.w[0] : 0ull;
    } else {
        uint64_t w = 0;
#pragma unroll
        for (int j = 0; j < Col<PH>::NQ; ++j) w = (k == j) ? c.w[j] : w;
        return w;
    }
}

// byte i (dynamic) of the column; 0 (= unknown) outside [0, PH)
template <int PH>
__device__ __forceinline__ uint32_t col_byte(const Col<PH> &c, int i) {
    const uint64_t w = (i >= 0 && i < PH) ? col_word<PH>(c, i >> 3) : 0ull;
    return (uint32_t)(w >> (8 * (i & 7))) & 0xffu;
}

// the 4 bytes [z-2, z+1] as one u32 (byte 0 = z-2), zeros outside the column
template <int PH>
__device__ __forceinline__ uint32_t col_window(const Col<PH> &c, int z) {
    const int o = z - 2;
    if (o < 0) return (uint32_t)(c.w[0] << (8 * (-o)));
    const int k = o >> 3, sh = 8 * (o & 7);
    const uint64_t lo = col_word<PH>(c, k);
    const uint64_t hi = col_word<PH>(c, k + 1);
    return (uint32_t)(sh ? (lo >> sh) | (hi << (64 - sh)) : lo);
}

template <int PH>
__device__ __forceinline__ void col_or(Col<PH> &c, int i, uint32_t v) {
#pragma unroll
    for (int k = 0; k < Col<PH>::NQ; ++k)
        if ((i >> 3) == k) c.w[k] |= (uint64_t)v << (8 * (i & 7));
}

// col_or that reports whether the column changed
template <int PH>
__device__ __forceinline__ bool col_or_chk(Col<PH> &c, int i, uint32_t v) {
    bool ch = false;
#pragma unroll
    for (int k = 0; k < Col<PH>::NQ; ++k)
        if ((i >> 3) == k) {
            const uint64_t m = (uint64_t)v << (8 * (i & 7));
            ch = (c.w[k] & m) != m;
            c.w[k] |= m;
        }
    return ch;
}

template <int PH>
__device__ __forceinline__ void col_set(Col<PH> &c, int i, uint32_t v) {
#pragma unroll
    for (int k = 0; k < Col<PH>::NQ; ++k)
        if ((i >> 3) == k) c.w[k] = (c.w[k] & ~(0xffull << (8 * (i & 7)))) | ((uint64_t)v << (8 * (i & 7)));
}

// OR byte value `v` into bytes [lo, hi] (inclusive; empty when hi < lo) -- the z rays
template <int PH>
__device__ __forceinline__ bool col_or_range(Col<PH> &c, int lo, int hi, uint32_t v) {
    const uint64_t vv = (uint64_t)v * 0x0101010101010101ull;
    bool ch = false;
#pragma unroll
    for (int k = 0; k < Col<PH>::NQ; ++k) {
        const int a = lo - 8 * k < 0 ? 0 : lo - 8 * k;
        const int b = hi - 8 * k > 7 ? 7 : hi - 8 * k;
        if (a <= b) {
            const uint64_t m = vv & ((~0ull) >> (8 * (7 - b))) & ((~0ull) << (8 * a));
            ch |= (c.w[k] & m) != m;
            c.w[k] |= m;
        }
    }
    return ch;
}

template <int PH>
__device__ __forceinline__ bool col_differs(const Col<PH> &a, const Col<PH> &b) {
    bool d = false;
#pragma unroll
    for (int k = 0; k < Col<PH>::NQ; ++k) d |= a.w[k] != b.w[k];
    return d;
}

// byte (x, y, z) of the bricked map (bcol: env_plan.h)
template <int PH>
__device__ __forceinline__ uint32_t boff(int x, int y, int z, int nby) {
    return bcol(x, y, nby) * (uint32_t)PH + (uint32_t)z;
}

// Destination of the observation row.  With auto-reset, a step that ends the
// episode writes its obs to the terminal row (NULL: dropped) and the reset
// obs goes to the regular row.
struct ObsDst {
    float *row;          // direct HBM row (NULL: none)
    float *term_row;     // terminal-obs HBM row under auto-reset (NULL: dropped)
    uint32_t *stage;     // the wave's LDS staging block (STAGE_WORDS): used instead of `row` when set
    bool select;
    bool truncated;
    int aslot;           // the agent's slot (0..15) in the staging block
};

// Staging block of one wave (16 agents) in plane-set mode: the window bytes
// of each obs row in obs order (byte 16i + 4q + k of agent a at byte a * 64),
// then each agent's 16 tail floats.  The flush expands the bytes through the
// LUT, so the block is 2 KiB per wave instead of the 5 KiB of float rows (the
// byte-mark kernels' format, STAGE_WORDS_F).
constexpr int STAGE_WORDS = 16 * 20;
constexpr int STAGE_WORDS_F = 16 * VN_OBS_DIM;
// Plane-set staging: each obs row is 20 words of 4 byte codes, so the flush
// expands every float4 the same way (no division, no divergence) and stores
// 1 KiB contiguous per instruction.  The window words hold belief bytes; the
// tail words (obs[64..79], get_obs :278-291) hold codes from the belief-byte
// values that never occur (bit7 clear but not 0x00 / 0x40; 0xC1..0xFF), whose
// LUT entries are the tail's values: 0.0, 1.0, f32(a/5), f32(c/L).  obs[72]
// (a quotient with many values) gets a code per agent of the block whose LUT
// entry the agent rewrites each step (tc_slot).  TC_*: env_plan.h, with the LUT.
constexpr uint32_t TC_ZERO4 = TC_ZERO * 0x01010101u;
__device__ __forceinline__ uint32_t tc_slot(int agent_in_block) {        // 64 codes: 0x41..0x60, 0xC1..0xE0
    return agent_in_block < 32 ? 0x41u + (uint32_t)agent_in_block : 0xC1u + (uint32_t)(agent_in_block - 32);
}


struct Rays {
    int nf[6];
    bool wh[6];
};

// sensing mark of ray r at step s on byte z of a window word (its byte 2);
// returns whether the byte changed
__device__ __forceinline__ bool mark_w(uint32_t &w, const Rays &ry, int r, int s) {
    const uint32_t v = s <= ry.nf[r] ? KNOWN : (ry.wh[r] && s == ry.nf[r] + 1) ? WALLB : 0u;
    const uint32_t m = v << 16;
    const bool ch = (w & m) != m;
    w |= m;
    return ch;
}

// ----------------------------------------------------------------------------
// Plane-set mode (PH == 8, rooms <= 64 x 64; VnEnv::pcache).  A sensing mark
// outside the window is recorded only in the marked-bit planes, never as a
// byte: the belief is byte map UNION planes, and a column takes the plane
// bits into its known bits (bit7) when it enters the window.  Wall cells
// carry a latent wall bit (0x40 without 0x80 = still unknown) from the reset
// onwards (copied from a per-room image), so a plane bit alone tells a known
// wall from a known free cell.  The plane rows the window needs stay in LDS
// for the whole launch: the x-plane rows (y', z = 0..7) of the 4 window rows
// y' (slot y' & 3) and the y-plane rows (x', z) of the 4 window columns x'
// (slot 4 + (x' & 3)); in HBM such a set is one 64-byte line.  A move swaps
// one set (written back if dirty, like a tile column), so a ray mark costs an
// LDS word instead of an HBM row write plus one blind byte store per new cell.
// ----------------------------------------------------------------------------
// Stood-column map (PCM 2, rooms <= 32 x 32; VN_STOOD).  In plane-set mode
// only the agent's own column ever reaches the byte map (visit count, z-ray
// marks); every other column of the HBM map stays the room image the reset
// copied, and a plane set stays all-zero in HBM until it is first written
// back dirty.  Two small per-agent records say which is which:
//   * S: one bit per column the agent has stood in (32 rows of u32, kept in
//     LDS for the launch).  A column entering the window that was never stood
//     in is read from the room image (L2-resident, one copy per room) instead
//     of the agent's HBM map -- identical bytes, no HBM read;
//   * xnz / ynz: one bit per x-plane set (row y') / y-plane set (column x')
//     written back since the reset.  An entering set without its bit is zero:
//     no load at all.
// Early in an episode (the bench's window) ~90 % of the entering columns and
// ~70 % of the entering sets are pristine.  The HBM contents are exactly
// those of the unrecorded scheme (only reads are skipped), so the exported
// belief is unchanged.
#ifndef VN_STOOD
#define VN_STOOD 1
#endif
#ifndef VN_DM_CODES
#define VN_DM_CODES 1        // byte-mark kernels stage obs rows as code words too (1.25 instead of 5 KiB of LDS per wave)
#endif
#ifndef VN_STOOD_PART
#define VN_STOOD_PART 1      // launches of <= 8 steps load only the stood-row shares they can reach
#endif
constexpr int kStoodStride = 33;   // u32 per agent in LDS (32 rows + 1: bank spread)
struct Stood {
    uint32_t *row;                 // the agent's S rows in LDS (nullptr when off)
    uint32_t xnz, ynz;             // plane sets whose HBM copy may be nonzero
    uint32_t chg;                  // S shares (rows 8q .. 8q + 7) changed in this launch
};

// RT, the plane row word: uint32_t when every room of the set is at most
// 32 x 32 (PCM 2), else uint64_t.  It is the row width in HBM as well as in
// LDS, so a set is 8 x sizeof(RT) bytes in HBM (32 B for PCM 2: the four sets
// of a window axis are 128 contiguous bytes) and half the LDS for PCM 2 (16
// waves fit a CU).
template <typename RT>
struct PsetGeom {
    static constexpr int STRIDE = sizeof(RT) == 4 ? 8 * 8 + 4 : 8 * 8 + 2;   // RT words per agent, 16-B aligned
};

// lane q's share of a set: rows z = 2q, 2q + 1
template <typename RT>
using PsetShare = typename std::conditional<sizeof(RT) == 8, uint4, uint2>::type;

template <typename RT>
__device__ __forceinline__ PsetShare<RT> pset_zero() {
    if constexpr (sizeof(RT) == 8) return make_uint4(0u, 0u, 0u, 0u);
    else return make_uint2(0u, 0u);
}

template <typename RT>
__device__ __forceinline__ PsetShare<RT> *pset_hbm(const Params &p, int8_t *map, bool xs, int c) {
    return reinterpret_cast<PsetShare<RT> *>(map + (xs ? p.xp_off : p.yp_off) + (uint32_t)c * (8u * sizeof(RT)));
}

template <typename RT>
__device__ __forceinline__ void pset_put(RT *ps, int slot, int q, PsetShare<RT> v) {
    *reinterpret_cast<PsetShare<RT> *>(ps + slot * 8 + 2 * q) = v;
}

template <typename RT>
__device__ __forceinline__ PsetShare<RT> pset_get(const RT *ps, int slot, int q) {
    return *reinterpret_cast<const PsetShare<RT> *>(ps + slot * 8 + 2 * q);
}

// the known bits (byte z: 0x80) the planes hold for column (cx, cy), both in the window
template <typename RT>
__device__ __forceinline__ uint64_t pset_known(const RT *ps, int cx, int cy) {
    const RT *xs = ps + (cy & 3) * 8, *ys = ps + (4 + (cx & 3)) * 8;
    uint64_t k = 0;
#pragma unroll
    for (int z = 0; z < 8; ++z) k |= (uint64_t)(((xs[z] >> cx) | (ys[z] >> cy)) & 1u) << (8 * z + 7);
    return k;
}

// launch start: lane q loads its share of each of the 8 sets
template <typename RT, bool SB = false>
__device__ __forceinline__ void pset_fill(const Params &p, int8_t *map, RT *ps, const Agent &g, const Room &R, int q,
                                          const Stood &st) {
    PsetShare<RT> v[8];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int yy = g.y - 2 + s, xx = g.x - 2 + s;
        v[s] = pset_zero<RT>();
        v[4 + s] = pset_zero<RT>();
        if (yy >= 0 && yy < R.D && (!SB || ((st.xnz >> yy) & 1u))) v[s] = pset_hbm<RT>(p, map, true, yy)[q];
        if (xx >= 0 && xx < R.W && (!SB || ((st.ynz >> xx) & 1u))) v[4 + s] = pset_hbm<RT>(p, map, false, xx)[q];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        pset_put(ps, (g.y - 2 + s) & 3, q, v[s]);
        pset_put(ps, 4 + ((g.x - 2 + s) & 3), q, v[4 + s]);
    }
    __builtin_amdgcn_wave_barrier();
}

// launch end: the dirty sets back to HBM
template <typename RT, bool SB = false>
__device__ __forceinline__ void pset_flush(const Params &p, int8_t *map, const RT *ps, const Agent &g, const Room &R,
                                           uint32_t pdirty, int q, Stood &st) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int yy = g.y - 2 + s, xx = g.x - 2 + s;
        if (((pdirty >> (yy & 3)) & 1u) && yy >= 0 && yy < R.D) {
            pset_hbm<RT>(p, map, true, yy)[q] = pset_get(ps, yy & 3, q);
            if (SB) st.xnz |= 1u << yy;
        }
        if (((pdirty >> (4 + (xx & 3))) & 1u) && xx >= 0 && xx < R.W) {
            pset_hbm<RT>(p, map, false, xx)[q] = pset_get(ps, 4 + (xx & 3), q);
            if (SB) st.ynz |= 1u << xx;
        }
    }
}

template <typename RT>
struct SetLoad {
    PsetShare<RT> v;
    int slot;
};

// after a horizontal move in axis dir to (x, y): the set of the entering
// coordinate (y-plane set of the entering x for an x move, x-plane set of the
// entering y for a y move) replaces the leaving one.  Load first, then the
// write-back (vmcnt retires in issue order).
template <typename RT, bool SB = false>
__device__ __forceinline__ void pset_shift_issue(const Params &p, int8_t *map, const RT *ps, int dir, int x, int y,
                                                 const Room &R, uint32_t pdirty, int q, SetLoad<RT> &sl, Stood &st) {
    const bool xm = dir < 2;
    const int e = xm ? (dir == 0 ? x + 1 : x - 2) : (dir == 2 ? y + 1 : y - 2);
    const int l = (dir == 0 || dir == 2) ? e - 4 : e + 4;
    const int lim = xm ? R.W : R.D;
    sl.slot = xm ? 4 + (e & 3) : (e & 3);
    sl.v = pset_zero<RT>();
    // SB: a set never written back since the reset is zero (no load)
    if (!(VN_ABLATE & 1u) && e >= 0 && e < lim && (!SB || (((xm ? st.ynz : st.xnz) >> e) & 1u)))
        sl.v = pset_hbm<RT>(p, map, !xm, e)[q];
    if (((pdirty >> sl.slot) & 1u) && l >= 0 && l < lim) {
        pset_hbm<RT>(p, map, !xm, l)[q] = pset_get(ps, sl.slot, q);
        if (SB) {
            if (xm) st.ynz |= 1u << l;
            else st.xnz |= 1u << l;
        }
    }
}

template <typename RT>
__device__ __forceinline__ uint32_t pset_shift_commit(RT *ps, const SetLoad<RT> &sl, uint32_t pdirty, int q) {
    pset_put(ps, sl.slot, q, sl.v);
    __builtin_amdgcn_wave_barrier();
    return pdirty & ~(1u << sl.slot);
}

// ----------------------------------------------------------------------------
// Per-agent LDS tile: the 16 window columns, toroidally indexed by
// slot = (x & 3) << 2 | (y & 3).  The window [x-2, x+1] x [y-2, y+1] covers
// each residue pair exactly once, so the tile always holds exactly the
// current window; after a horizontal move the 4 columns entering the window
// take the slots of the 4 leaving it.  Dirty slots are written back on
// eviction and at the end of the launch.
// ----------------------------------------------------------------------------
template <int PH>
struct TileGeom {
    static constexpr int QW = PH / 8;                   // u64 per column
    static constexpr int STRIDE = 16 * QW + 1;          // u64 per agent tile (+1: bank spread)
};

template <int PH>
__device__ __forceinline__ void tile_read(const uint64_t *tile, int slot, Col<PH> &c) {
    const uint64_t *s = tile + slot * TileGeom<PH>::QW;
#pragma unroll
    for (int k = 0; k < Col<PH>::NQ; ++k) c.w[k] = s[k];
}

template <int PH>
__device__ __forceinline__ void tile_write(uint64_t *tile, int slot, const Col<PH> &c) {
    uint64_t *s = tile + slot * TileGeom<PH>::QW;
#pragma unroll
    for (int k = 0; k < Col<PH>::NQ; ++k) s[k] = c.w[k];
}

__device__ __forceinline__ int tslot(int x, int y) { return ((x & 3) << 2) | (y & 3); }

// Plane-set mode: the latent-wall room images, VN_WIMG_REP copies per room
// ([room][copy][map_bytes]); agent a reads copy a % VN_WIMG_REP, so the
// launch's window fill (every agent reading its room's image at once) is
// spread over more L2 lines (diagnostics knob, default one copy: env_plan.h).
__device__ __forceinline__ const int8_t *room_image(const int8_t *wimg, int room, uint32_t map_bytes) {
    const uint32_t agent = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    return wimg + ((size_t)room * VN_WIMG_REP + (VN_WIMG_REP > 1 ? agent % VN_WIMG_REP : 0u)) * map_bytes;
}

// The window bytes [z - 2, z + 1] (byte 0 = z - 2, zeros outside [0, PH)) of
// the 4 tile columns in slots s[0..3], one u32 each, and the whole column of
// slot s[2] (dx = 0; lane 2's center column).  One LDS phase: every read is
// issued before the first result is used and nothing here branches, so the
// step pays one LDS round trip for the window instead of one per dword.
// Each window word comes from one 8-byte piece of its column (PH 8: the
// column, which for slot s[2] is also the center column; else the two dwords
// from z - 2 on, clamped into the column, one two-dword read) and one shift
// that zero-fills below byte 0 and above byte PH - 1; so a sensing pass still
// holds one register per window column, not the column.
template <int PH>
__device__ __forceinline__ void tile_win4(const uint64_t *tile, const int (&s)[4], int z, uint32_t (&win)[4],
                                          Col<PH> &cen) {
    constexpr int NW = PH / 4;
    const int o = z - 2;                                     // -2 .. PH - 3
    const int k0 = o >> 2;                                   // -1 for o = -2, -1
    const int b = NW == 2 ? 0 : (k0 < 0 ? 0 : k0 > NW - 2 ? NW - 2 : k0);   // first dword of the piece
    const int rel = o - 4 * b;                               // window start in the piece: -2 .. 7
    const int l = rel < 0 ? -8 * rel : 0, r = rel < 0 ? 0 : 8 * rel;
    auto piece = [&](int i) -> uint64_t {
        if constexpr (PH == 8) {
            return tile[s[i]];
        } else {
            const uint32_t *cw = reinterpret_cast<const uint32_t *>(tile + s[i] * TileGeom<PH>::QW) + b;
            return (uint64_t)cw[0] | ((uint64_t)cw[1] << 32);
        }
    };
    auto word = [&](uint64_t v) -> uint32_t { return rel < 0 ? (uint32_t)v << l : (uint32_t)(v >> r); };
    uint64_t v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = piece(i);
    if constexpr (PH == 8) cen.w[0] = v[2];
    else tile_read<PH>(tile, s[2], cen);
    // the phase's reads (the caller's plane-row word included) stay ahead of
    // everything below: the scheduler would otherwise sink one of them past
    // the ray record's wait, a round trip of its own
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) win[i] = word(v[i]);
}

// byte z of a tile column
__device__ __forceinline__ void tile_put_byte(uint64_t *tile, int qw, int slot, int z, uint32_t v) {
    reinterpret_cast<uint8_t *>(tile + slot * qw)[z] = (uint8_t)v;
}

// Exchanges inside an agent group (4 lanes = one DPP quad): a quad_perm DPP
// move is one VALU instruction, where __shfl is an LDS permute with its
// latency on the step's dependency chain.  QP = quad_perm control
// (2 bits per destination lane: the source lane in the quad).
#ifndef VN_DPP
#define VN_DPP 1
#endif
template <int QP>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v) {
#if VN_DPP
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, QP, 0xf, 0xf, false);
#else
    const int lane = (int)(threadIdx.x & 3u);
    return (uint32_t)__shfl((int)v, (QP >> (2 * lane)) & 3, GROUP);
#endif
}
template <int SRC>
__device__ __forceinline__ uint32_t group_bcast(uint32_t v) { return quad_perm<SRC * 0x55>(v); }
template <int SRC>
__device__ __forceinline__ int group_bcast(int v) { return (int)quad_perm<SRC * 0x55>((uint32_t)v); }

// OR a 16-bit slot mask over the 4 lanes of the agent group
__device__ __forceinline__ uint32_t group_or(uint32_t m) {
    m |= quad_perm<0xB1>(m);      // lane ^ 1: [1, 0, 3, 2]
    m |= quad_perm<0x4E>(m);      // lane ^ 2: [2, 3, 0, 1]
    return m;
}

struct PlaneCache {      // lane 0: x-plane row, lane 1: y-plane row
    uint64_t w[2];
    int row, w0;         // cached row index and first word; row < 0: invalid
    uint32_t dirty;      // VN_ROW_WB: words 0 / 1 changed since loaded (written back when the row is left)
};

// DM (PCM 3): the cached plane row is write-back -- a pass's new row bits stay
// in the lane's registers until the agent leaves the row (or the launch ends)
// instead of one 8-byte store per step that marks it.
#ifndef VN_ROW_WB
#define VN_ROW_WB 0
#endif

// Fill the tile from HBM (launch start): lane q loads its 4 window columns.
// PC: the plane sets (ps, already filled) add their known bits.
template <int PH, bool PC, typename RT, bool SB = false>
__device__ __forceinline__ void tile_fill(const Params &p, const int8_t *map, uint64_t *tile, const RT *ps,
                                          const Agent &g, const Room &R, int q, const Stood &st) {
    const int cy = g.y + q - 2;
    const int8_t *img = SB ? room_image(p.wimg, g.room, p.map_bytes) : map;
    const uint32_t srow = SB && cy >= 0 && cy < R.D ? st.row[cy] : ~0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cx = g.x + i - 2;
        Col<PH> c;
        col_zero<PH>(c);
        if (cx >= 0 && cx < R.W && cy >= 0 && cy < R.D) {
            // SB: a column never stood in is the room image's
            col_load<PH>((!SB || ((srow >> cx) & 1u) ? map : img) + boff<PH>(cx, cy, 0, p.nby), c);
            if constexpr (PC) c.w[0] |= pset_known(ps, cx, cy);
        }
        tile_write<PH>(tile, tslot(cx, cy), c);
    }
}

// Write the dirty window columns back to HBM (launch end).
template <int PH>
__device__ __forceinline__ void tile_flush(const Params &p, int8_t *map, const uint64_t *tile, const Agent &g,
                                           const Room &R, uint32_t dirty, int q) {
    const int cy = g.y + q - 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cx = g.x + i - 2;
        const int s = tslot(cx, cy);
        if (((dirty >> s) & 1u) && cx >= 0 && cx < R.W && cy >= 0 && cy < R.D) {
            Col<PH> c;
            tile_read<PH>(tile, s, c);
            col_store<PH>(map + boff<PH>(cx, cy, 0, p.nby), c);
        }
    }
}

// Window record (VnTuning::wrec_k): a launch of at most p.wrec_k steps ends by
// storing the agent's 16 tile columns contiguously (16 x PH bytes, in tile
// slot order) and sets HOT_WREC in the hot state; the next launch then fills
// its tile from that record -- 2 (PH 8) / 4 (PH 16) 16-B loads per lane, whole
// 64-B pieces -- instead of 16 column loads spread over the bricks (a PH-16
// brick row puts a lane's 4 columns in 4 different 64-B pieces), and loads
// only the 4 columns the premoved step 0 brings into the window.  The byte
// map stays complete (tile_flush still writes the dirty columns back), so the
// record is a copy: every launch that does not write it clears HOT_WREC
// (pack() leaves bit 30 clear), and only a record written for the agent's
// current (x, y) is ever read.  What the one-step call gains is what its
// fill cost (the collector's policy-in-the-loop env call, reference
// envs/CubicEnv.py:110-132 per SubprocVecEnv worker).
#ifndef VN_WREC
#define VN_WREC 1
#endif
constexpr uint32_t HOT_WREC = 1u << 30;
constexpr int PRIO_WREC_SAVE = 128;    // Params::prio bits set by the host: this launch writes the records,
constexpr int PRIO_WREC_EARLY = 256;   // ... and the previous step launch wrote them (load each with the state)

// the records sit behind the hot state in its allocation: no pointer of
// their own stays live across the step loop (SGPR pressure)
__device__ __forceinline__ uint64_t *wrec_base(const Params &p) { return reinterpret_cast<uint64_t *>(p.hot + p.N); }

template <int PH>
struct WrecV {
    uint4 v[16 * PH / 64];               // lane q's 16-B pieces of the record (piece j: bytes 64 j + 16 q)
};

template <int PH>
__device__ __forceinline__ void wrec_load(const Params &p, int agent, int q, WrecV<PH> &w) {
    const uint4 *src = reinterpret_cast<const uint4 *>(wrec_base(p) + (size_t)agent * (2 * PH));
#pragma unroll
    for (int j = 0; j < 16 * PH / 64; ++j) w.v[j] = src[4 * j + q];
}

template <int PH>
__device__ __forceinline__ void wrec_store(const Params &p, const uint64_t *tile, int agent, int q) {
    constexpr int NI = 16 * PH / 64;           // 16-B pieces per lane
    uint4 *dst = reinterpret_cast<uint4 *>(wrec_base(p) + (size_t)agent * (2 * PH));
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const uint64_t a = tile[8 * j + 2 * q], b = tile[8 * j + 2 * q + 1];
        dst[4 * j + q] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    }
}

// The tile from the record written around g0 (the launch's start cell), then
// the columns entering the window of gf (step 0's premoved cell; at most one
// horizontal move away).  No write-back: the map holds every record column.
template <int PH, bool PC, typename RT, bool SB>
__device__ __forceinline__ void wrec_fill(const Params &p, const int8_t *map, uint64_t *tile, const RT *ps,
                                          const Agent &g0, const Agent &gf, const Room &R, int q, const Stood &st,
                                          const WrecV<PH> &w) {
    constexpr int NI = 16 * PH / 64;
    const bool shifted = gf.x != g0.x || gf.y != g0.y;
    int ex = 0, ey = 0;
    Col<PH> c;
    col_zero<PH>(c);
    if (shifted) {
        if (gf.x != g0.x) {
            ex = gf.x > g0.x ? gf.x + 1 : gf.x - 2;
            ey = gf.y + q - 2;
        } else {
            ex = gf.x + q - 2;
            ey = gf.y > g0.y ? gf.y + 1 : gf.y - 2;
        }
        if (ex >= 0 && ex < R.W && ey >= 0 && ey < R.D) {
            const bool stood = !SB || ((st.row[ey] >> ex) & 1u);
            col_load<PH>((stood ? map : room_image(p.wimg, gf.room, p.map_bytes)) + boff<PH>(ex, ey, 0, p.nby), c);
            if constexpr (PC) c.w[0] |= pset_known(ps, ex, ey);
        }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        tile[8 * j + 2 * q] = (uint64_t)w.v[j].x | ((uint64_t)w.v[j].y << 32);
        tile[8 * j + 2 * q + 1] = (uint64_t)w.v[j].z | ((uint64_t)w.v[j].w << 32);
    }
    // the record's slots are written by all 4 lanes: complete before a lane
    // overwrites an entering slot and before the sensing reads other lanes' slots
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (shifted) tile_write<PH>(tile, tslot(ex, ey), c);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// After a horizontal move in axis dir (0 +x, 1 -x, 2 +y, 3 -y) to (x, y):
// lane q swaps one slot -- writes the leaving column back if dirty and
// issues the load of the entering one into `sl`; tile_shift_commit puts it
// in the slot.  Split so the step's other loads (ray record, plane rows)
// are in flight together with this one.
template <int PH>
struct ShiftLoad {
    Col<PH> c;
    int s;
    uint32_t entering;
    int ex, ey;          // the entering column
    bool in;             // ... inside the room
};

template <int PH, bool SB = false>
__device__ __forceinline__ void tile_shift_issue(const Params &p, int8_t *map, const uint64_t *tile, int dir, int x,
                                                 int y, const Room &R, uint32_t dirty, int q, ShiftLoad<PH> &sl,
                                                 const Stood &st, int room) {
    int ex, ey, lx, ly;
    if (dir < 2) {
        ex = dir == 0 ? x + 1 : x - 2;
        ey = y + q - 2;
        lx = dir == 0 ? ex - 4 : ex + 4;
        ly = ey;
        sl.entering = 0xfu << ((ex & 3) << 2);
    } else {
        ex = x + q - 2;
        ey = dir == 2 ? y + 1 : y - 2;
        lx = ex;
        ly = dir == 2 ? ey - 4 : ey + 4;
        sl.entering = 0x1111u << (ey & 3);
    }
    sl.s = tslot(ex, ey);
    sl.ex = ex;
    sl.ey = ey;
    sl.in = ex >= 0 && ex < R.W && ey >= 0 && ey < R.D;
    // the load first: vmcnt retires in issue order, so a store issued ahead
    // of it would hold its data until the store completes
    col_zero<PH>(sl.c);
    if ((VN_ABLATE & 131072u) && sl.in) {   // diagnostics: the entering column from the room image (L2)
        col_load<PH>(p.wimg + boff<PH>(ex, ey, 0, p.nby), sl.c);
    } else if (!(VN_ABLATE & 1u) && sl.in) {
        // SB: a column never stood in is the room image's (L2), not an HBM read
        const bool stood = !SB || ((st.row[ey] >> ex) & 1u);
        col_load<PH>((stood ? (const int8_t *)map : room_image(p.wimg, room, p.map_bytes)) + boff<PH>(ex, ey, 0, p.nby),
                     sl.c);
    }
    if (!(VN_ABLATE & 8u) && ((dirty >> sl.s) & 1u) && lx >= 0 && lx < R.W && ly >= 0 && ly < R.D) {
        Col<PH> old;
        tile_read<PH>(tile, sl.s, old);
        col_store<PH>(map + boff<PH>(lx, ly, 0, p.nby), old);
    }
}

template <int PH>
__device__ __forceinline__ uint32_t tile_shift_commit(uint64_t *tile, const ShiftLoad<PH> &sl, uint32_t dirty) {
    tile_write<PH>(tile, sl.s, sl.c);
    return dirty & ~sl.entering;
}


// Plane rows of the agent's new cell (lane 0: x-plane row (y, z), lane 1:
// y-plane row (x, z)).  Rooms up to 128 wide keep a whole row (<= 2 words)
// in the cache, loaded here together with the step's other loads; wider
// rooms load a 2-word window lazily inside sense_observe.
template <int PH>
__device__ __forceinline__ void plane_prefetch(const Params &p, int8_t *map, PlaneCache &pc_, int x, int y,
                                               int z, int q) {
    if (q < 2) {
        const bool xr = q == 0;
        const int nw = xr ? p.nwx : p.nwy;
        if (nw <= 2 && !(VN_ABLATE & 2u)) {
            const int rowi = (xr ? y : x) * PH + z;
            if (pc_.row != rowi) {
                uint64_t *pbase = reinterpret_cast<uint64_t *>(map + (xr ? p.xp_off : p.yp_off));
                const uint64_t *prow = pbase + (size_t)rowi * nw;
                // VN_ROW_WB: the left row's changed words go back after the new
                // row's loads are issued (vmcnt retires in issue order)
                const uint64_t o0 = pc_.w[0], o1 = pc_.w[1];
                const int orow = pc_.row;
                const uint32_t od = VN_ROW_WB ? pc_.dirty : 0u;
                pc_.row = rowi;
                pc_.w0 = 0;
                pc_.w[0] = prow[0];
                pc_.w[1] = nw > 1 ? prow[1] : 0ull;
                pc_.dirty = 0u;
                if (VN_ROW_WB && od) {
                    uint64_t *op = pbase + (size_t)orow * nw;
                    if (od & 1u) op[0] = o0;
                    if (od & 2u) op[1] = o1;
                }
            }
        }
    }
}

// VN_ROW_WB: the cached row's changed words to HBM (launch end)
__device__ __forceinline__ void plane_wb_flush(const Params &p, int8_t *map, PlaneCache &pc_, int q) {
    if (VN_ROW_WB && q < 2 && pc_.dirty && pc_.row >= 0) {
        const int nw = q == 0 ? p.nwx : p.nwy;
        uint64_t *op = reinterpret_cast<uint64_t *>(map + (q == 0 ? p.xp_off : p.yp_off)) + (size_t)pc_.row * nw;
        if (pc_.dirty & 1u) op[0] = pc_.w[0];
        if (pc_.dirty & 2u) op[1] = pc_.w[1];
        pc_.dirty = 0u;
    }
}

// Deferred plane marks (byte-mark mode with rows of at most 2 words, PCM 3):
// a sensing pass records its x / y ray spans here, and the marks -- the new
// bits of the agent's plane rows, their HBM words and the blind byte marks
// of the newly known cells outside the window -- are applied at the start of
// the NEXT step (before its entering column is loaded, which may hold such a
// cell), so the plane row loaded for this step (plane_prefetch) has a whole
// step to arrive instead of being waited for inside the sensing.  The cells
// inside the window are marked in the tile by the sensing itself, and a
// reset drops the pending marks of the episode it ends (the planes and the
// map are cleared).
struct PendMarks {
    int valid;
    int x, y, z;
    uint32_t nf4;        // the step's free run lengths +x, -x, +y, -y (8 bits each)
    int pa, pw0, rowi;   // lanes 0 / 1: the x / y row span start, its first word, the row index
    uint64_t pm0, pm1;   // lanes 0 / 1: the span masks of words pw0, pw0 + 1
};

template <int PH>
__device__ __forceinline__ void pend_apply(const Params &p, int8_t *map, PlaneCache &pc_, PendMarks &pend, int q) {
    if (!pend.valid) return;
    pend.valid = 0;
    const int x = pend.x, y = pend.y, z = pend.z, nby = p.nby;
    uint64_t rel = 0;                      // lanes 0/1: new bits relative to the span start pa
    if (q < 2) {
        // the row words: plane_prefetch of the pending step left row rowi in pc_
        const bool xr = q == 0;
        const int nw = xr ? p.nwx : p.nwy;
        uint64_t *prow = reinterpret_cast<uint64_t *>(map + (xr ? p.xp_off : p.yp_off)) + (size_t)pend.rowi * nw;
        const int pofs = pend.pw0 - pc_.w0;
        const uint64_t pn0 = pofs == 0 ? pc_.w[0] : pc_.w[1];
        const uint64_t pn1 = pofs == 0 ? pc_.w[1] : 0ull;
        const uint64_t nwd0 = pend.pm0 & ~pn0, nwd1 = pend.pm1 & ~pn1;
        if (nwd0) {
            const uint64_t nv = pn0 | pend.pm0;
            if (pofs == 0) pc_.w[0] = nv;
            else pc_.w[1] = nv;
            if (VN_ROW_WB) pc_.dirty |= pofs == 0 ? 1u : 2u;
            else if (!(VN_ABLATE & 2097184u)) prow[pend.pw0] = nv;   // 32 | 2097152: diagnostics
        }
        if (nwd1) {
            const uint64_t nv = pn1 | pend.pm1;
            if (pofs == 0) pc_.w[1] = nv;
            if (VN_ROW_WB) pc_.dirty |= 2u;
            else if (!(VN_ABLATE & 2097184u)) prow[pend.pw0 + 1] = nv;
        }
        const int sh = pend.pa - pend.pw0 * 64;   // 0..63
        rel = sh == 0 ? nwd0 : (nwd0 >> sh) | (nwd1 << (64 - sh));
        const int c = (xr ? x : y) - pend.pa;     // the agent's own bit; window cells are c-2 .. c+1
        rel &= ~(c >= 2 ? (0xfull << (c - 2)) : ((1ull << (c + 2)) - 1ull));
    }
    const uint32_t rxl = group_bcast<0>((uint32_t)rel);
    const uint32_t rxh = group_bcast<0>((uint32_t)(rel >> 32));
    const uint32_t ryl = group_bcast<1>((uint32_t)rel);
    const uint32_t ryh = group_bcast<1>((uint32_t)(rel >> 32));
    const int pax = group_bcast<0>(pend.pa), pay = group_bcast<1>(pend.pa);
    const uint64_t lane_sel = 0x1111111111111111ull << q;
    uint64_t mx = (VN_ABLATE & 96u) ? 0ull : (((uint64_t)rxh << 32) | rxl) & lane_sel;
    uint64_t my = (VN_ABLATE & 96u) ? 0ull : (((uint64_t)ryh << 32) | ryl) & lane_sel;
    const int nf0 = (int)(pend.nf4 & 0xffu), nf1 = (int)((pend.nf4 >> 8) & 0xffu);
    const int nf2 = (int)((pend.nf4 >> 16) & 0xffu), nf3 = (int)(pend.nf4 >> 24);
    while (mx) {
        const int pos = pax + __ffsll((unsigned long long)mx) - 1;
        mx &= mx - 1;
        const int d = pos - x;
        const uint32_t v = (d == nf0 + 1 || d == -nf1 - 1) ? WALLB : KNOWN;
        map[boff<PH>(pos, y, z, nby)] = (int8_t)v;
    }
    while (my) {
        const int pos = pay + __ffsll((unsigned long long)my) - 1;
        my &= my - 1;
        const int d = pos - y;
        const uint32_t v = (d == nf2 + 1 || d == -nf3 - 1) ? WALLB : KNOWN;
        map[boff<PH>(x, pos, z, nby)] = (int8_t)v;
    }
}

// One sensing pass (get_obs :254-312 with _sense_direction :345-397 and the
// visit update of _mark_visited/do_action :156-166) on the agent's tile.
// Returns the center cell's visit count after the update.
// PC: plane-set mode (ps = the agent's LDS plane sets, pdirty their dirty bits).
// DM: byte-mark mode with deferred plane marks (PendMarks; PCM 3).
template <int PH, bool FRESH, bool PC, typename RT, bool DM>
__device__ __forceinline__ int sense_observe(const Params &p, int8_t *map, uint64_t *tile, uint32_t &dirty,
                                             PlaneCache &pc_, RT *ps, uint32_t &pdirty, Agent &g,
                                             const Room &R, bool moved, bool &explored, const float *tab, ObsDst dst,
                                             uint2 rec, int q, PendMarks &pend, bool lut_stale = true) {
    const int x = g.x, y = g.y, z = g.z, nby = p.nby, L = p.L;

    // ---- x / y marked-bit plane rows (lane 0: x row (y,z), lane 1: y row (x,z)) ----
    int pa = 0, pw0 = 0, pwend = 0, pcoord = 0, nfp = 0, nfm = 0;
    uint64_t pm[2] = {0, 0};
    uint64_t *prow = nullptr;
    int rowi = 0;
    if (q < 2) {
        const bool xr = q == 0;
        const int nw = xr ? p.nwx : p.nwy;
        rowi = (xr ? y : x) * PH + z;
        prow = reinterpret_cast<uint64_t *>(map + (xr ? p.xp_off : p.yp_off)) + (size_t)rowi * nw;
        pcoord = xr ? x : y;
        // the row words needed depend on the span; fetch lazily below
        (void)nw;
    }
    // PC: lane 0 owns the x-plane row (y, z), lane 1 the y-plane row (x, z), both in LDS
    RT *prow_lds = (PC && q < 2) ? ps + (q == 0 ? (y & 3) : 4 + (x & 3)) * 8 + z : nullptr;

    // ---- this lane's 4 window columns from the tile: the window word
    //      (bytes z-2 .. z+1) of each, and the whole column dx = 0 (lane 2's
    //      center column: visit count and z rays) ----
    const int cy = y + q - 2;
    const bool yin = cy >= 0 && cy < R.D;
    // FRESH: the reset copied the room image (PC: latent walls) to HBM, or
    // cleared it; the tile takes the same columns
    auto fresh_col = [&](int i, Col<PH> &c) {
        col_zero<PH>(c);
        if (PC && yin && x + i - 2 >= 0 && x + i - 2 < R.W)
            col_load<PH>(room_image(p.wimg, g.room, p.map_bytes) + boff<PH>(x + i - 2, cy, 0, nby), c);
    };
    uint32_t win[4];
    Col<PH> cen;
    // PC: the lane's plane-row word, read in the same LDS phase as the window
    // (every lane reads: lanes 2 / 3 the words of lanes 0 / 1, unused)
    RT prw = 0;
    if constexpr (PC) prw = ps[((q & 1) == 0 ? (y & 3) : 4 + (x & 3)) * 8 + z];
    if constexpr (FRESH) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Col<PH> c;
            fresh_col(i, c);
            win[i] = col_window<PH>(c, z);
            if (i == 2) cen = c;
        }
    } else {
        // one LDS phase, ahead of the first use of the ray record: its load's
        // latency and the LDS round trip overlap
        const int ws[4] = {tslot(x - 2, cy), tslot(x - 1, cy), tslot(x, cy), tslot(x + 1, cy)};
        tile_win4<PH>(tile, ws, z, win, cen);
    }
    uint32_t chg = 0;                     // bit i: window column i changed by this pass

    // ---- ray extents from the room's 8-byte record (bit7: ended at a wall) ----
    Rays ry;
    bool near = false;
    uint32_t mm = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const uint32_t e = (r < 4 ? (rec.x >> (8 * r)) : (rec.y >> (8 * (r - 4)))) & 0xffu;
        const int n = (int)(e & 0x7fu);
        const bool wf = (e >> 7) != 0;
        ry.nf[r] = n < L ? n : L;
        ry.wh[r] = wf && n < L;
        near |= (n == 0) && wf;          // wall at step 1 -> near_wall (:378-379)
        mm |= (n > 0 ? 1u : 0u) << r;
    }

    // ---- plane rows: span, cached words, new marks ----
    uint64_t pn[2] = {0, 0};
    int pofs = 0;
    if (q < 2) {
        const bool xr = q == 0;
        const int nw = xr ? p.nwx : p.nwy;
        nfp = xr ? ry.nf[0] : ry.nf[2];
        nfm = xr ? ry.nf[1] : ry.nf[3];
        const bool whp = xr ? ry.wh[0] : ry.wh[2];
        const bool whm = xr ? ry.wh[1] : ry.wh[3];
        pa = pcoord - nfm - (whm ? 1 : 0);                 // marked span [pa, pb]
        const int pb = pcoord + nfp + (whp ? 1 : 0);
        pw0 = pa >> 6;
        pwend = pb >> 6;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const int base = (pw0 + w) * 64;
            const int lo = pa - base < 0 ? 0 : pa - base, hi = pb - base > 63 ? 63 : pb - base;
            pm[w] = (w == 0 || pw0 + 1 <= pwend) && hi >= lo ? ((~0ull) >> (63 - (hi - lo))) << lo : 0ull;
        }
        if (PC) {                          // nw == 1: the row word is in LDS
            pc_.w[0] = prw;
            pc_.w[1] = 0ull;
            pc_.w0 = 0;
        } else if (FRESH) {                // planes were cleared by the reset
            pc_.row = rowi;
            pc_.w0 = nw <= 2 ? 0 : pw0;
            pc_.w[0] = pc_.w[1] = 0ull;
            pc_.dirty = 0u;
        } else if (!DM && nw > 2 && (pc_.row != rowi || pc_.w0 != pw0)) {   // (DM: rows of <= 2 words, prefetched)
            pc_.row = rowi;
            pc_.w0 = pw0;
            pc_.w[0] = prow[pw0];
            pc_.w[1] = pw0 + 1 < nw ? prow[pw0 + 1] : 0ull;
        }                                  // nw <= 2: plane_prefetch holds words 0 and 1
        pofs = pw0 - pc_.w0;               // 0, or 1 when the span starts in word 1
        pn[0] = pofs == 0 ? pc_.w[0] : pc_.w[1];
        pn[1] = pofs == 0 ? pc_.w[1] : 0ull;
    }

    // ---- in-window ray cells, z rays and the center ----
    uint32_t cold = 0;
    if (q == 2) {                       // row dy = 0: -x s=2, -x s=1, center, +x s=1
        chg |= (uint32_t)mark_w(win[0], ry, 1, 2);
        chg |= (uint32_t)mark_w(win[1], ry, 1, 1) << 1;
        chg |= (uint32_t)mark_w(win[3], ry, 0, 1) << 3;
        cold = col_byte<PH>(cen, z);
        col_or_range<PH>(cen, z + 1, z + ry.nf[4], KNOWN);                       // up
        if (ry.wh[4]) col_or<PH>(cen, z + ry.nf[4] + 1, WALLB);
        col_or_range<PH>(cen, z - ry.nf[5], z - 1, KNOWN);                       // down
        if (ry.wh[5]) col_or<PH>(cen, z - ry.nf[5] - 1, WALLB);
        chg |= 4u;                                  // the center count changes every step
    } else {                            // column dx = 0: -y s=2 (q0), -y s=1 (q1), +y s=1 (q3)
        chg |= (uint32_t)mark_w(win[2], ry, q == 3 ? 2 : 3, q == 0 ? 2 : 1) << 2;
    }
    cold = group_bcast<2>(cold);
    int t;
    if (FRESH) {
        t = 1;                                                                  // start cell (:85)
    } else {
        t = decode_count(cold);
        if (moved) {
            if (t == 0) {
                t = 1;
                ++g.visited;
                explored = true;
            } else if (t > 0) {
                t += 1;
            }
        }
        t += 1;
        if (t > 63) t = 63;
    }
    if (q == 2) {
        col_set<PH>(cen, z, KNOWN | (uint32_t)t);
        win[2] = col_window<PH>(cen, z);
    }

    // ---- changed columns back to the tile (dirty), new plane marks to HBM ----
    // (lane 2's center column whole; any other column changed only in byte z)
    uint32_t dm = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool inroom = yin && x + i - 2 >= 0 && x + i - 2 < R.W;
        // after a reset every slot is rewritten (zeros outside the room), so no
        // column of the previous episode's window survives in the tile
        if (FRESH || (inroom && ((chg >> i) & 1u))) {
            const int s = tslot(x + i - 2, cy);
            if (q == 2 && i == 2) {
                tile_write<PH>(tile, s, cen);
            } else if (FRESH) {
                Col<PH> c;
                fresh_col(i, c);
                col_set<PH>(c, z, (win[i] >> 16) & 0xffu);
                tile_write<PH>(tile, s, c);
            } else {
                tile_put_byte(tile, TileGeom<PH>::QW, s, z, win[i] >> 16);
            }
            // PC: an x/y ray mark is also in the planes, so only the agent's own
            // column (visit count, z rays) has to reach HBM
            if (inroom && (!PC || (q == 2 && i == 2))) dm |= 1u << s;
        }
    }
    dirty |= group_or(dm);

    if constexpr (PC) {
        uint32_t pd = 0;
        if (q < 2) {
            const uint64_t nv = pn[0] | pm[0];
            if (nv != pn[0]) {
                *prow_lds = (RT)nv;
                pd = 1u << (q == 0 ? (y & 3) : 4 + (x & 3));
            }
        }
        pdirty |= group_or(pd);
    } else if constexpr (DM) {
        // the marks are applied at the start of the next step (pend_apply)
        pend.valid = 1;
        pend.x = x;
        pend.y = y;
        pend.z = z;
        pend.nf4 = (uint32_t)ry.nf[0] | ((uint32_t)ry.nf[1] << 8) | ((uint32_t)ry.nf[2] << 16) |
                   ((uint32_t)ry.nf[3] << 24);
        pend.pa = pa;
        pend.pw0 = pw0;
        pend.rowi = rowi;
        pend.pm0 = pm[0];
        pend.pm1 = pm[1];
    } else {

    // new marks: row bits set now for the first time.  Those inside the window
    // (d = -2..+1 from the agent) live in the tile; the others get their
    // byte written blind.  A row change makes a burst of new cells, so the
    // burst is spread over the 4 lanes of the group by position mod 4.
    uint64_t rel = 0;                      // lanes 0/1: new bits relative to the span start pa
    if (q < 2) {
        uint64_t nwd[2];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            nwd[w] = pm[w] & ~pn[w];
            if (nwd[w]) {
                const uint64_t nv = pn[w] | pm[w];
                if (pofs + w == 0) pc_.w[0] = nv;
                else if (pofs + w == 1) pc_.w[1] = nv;
                if (!(VN_ABLATE & 32u)) prow[pw0 + w] = nv;
            }
        }
        const int sh = pa - pw0 * 64;      // 0..63
        rel = sh == 0 ? nwd[0] : (nwd[0] >> sh) | (nwd[1] << (64 - sh));
        const int c = pcoord - pa;         // the agent's own bit; window cells are c-2 .. c+1
        rel &= ~(c >= 2 ? (0xfull << (c - 2)) : ((1ull << (c + 2)) - 1ull));
    }
    {
        const uint32_t rxl = group_bcast<0>((uint32_t)rel);
        const uint32_t rxh = group_bcast<0>((uint32_t)(rel >> 32));
        const uint32_t ryl = group_bcast<1>((uint32_t)rel);
        const uint32_t ryh = group_bcast<1>((uint32_t)(rel >> 32));
        const int pax = group_bcast<0>(pa), pay = group_bcast<1>(pa);
        const uint64_t lane_sel = 0x1111111111111111ull << q;
        uint64_t mx = (VN_ABLATE & 96u) ? 0ull : (((uint64_t)rxh << 32) | rxl) & lane_sel;
        uint64_t my = (VN_ABLATE & 96u) ? 0ull : (((uint64_t)ryh << 32) | ryl) & lane_sel;
        while (mx) {
            const int pos = pax + __ffsll((unsigned long long)mx) - 1;
            mx &= mx - 1;
            const int d = pos - x;
            const uint32_t v = (d == ry.nf[0] + 1 || d == -ry.nf[1] - 1) ? WALLB : KNOWN;
            map[boff<PH>(pos, y, z, nby)] = (int8_t)v;
        }
        while (my) {
            const int pos = pay + __ffsll((unsigned long long)my) - 1;
            my &= my - 1;
            const int d = pos - y;
            const uint32_t v = (d == ry.nf[2] + 1 || d == -ry.nf[3] - 1) ? WALLB : KNOWN;
            map[boff<PH>(x, pos, z, nby)] = (int8_t)v;
        }
    }
    }   // !PC

    g.near_wall = g.near_wall || near;
    g.cid = ry.nf[5];
    g.move_mask = mm;

    // ---- observation row: lane q writes obs[16i+4q..+3] and tail float4 q ----
    // two single-address-space destinations (an LDS/global select would
    // compile to flat stores, which occupy the vector-memory path even for LDS)
    const bool to_term = dst.select && (dst.truncated || g.done || g.visited >= R.finish_visits);
    const bool to_stage = !to_term && dst.stage && !(VN_ABLATE & 4u);
    float4 *glb4 = (VN_ABLATE & 4u) ? nullptr
                   : to_term       ? reinterpret_cast<float4 *>(dst.term_row)
                   : dst.stage     ? nullptr
                                   : reinterpret_cast<float4 *>(dst.row);
    float4 tail;                                                  // obs[64 + 4q .. +3]
    constexpr bool CW = PC || (DM && VN_DM_CODES);   // code-word staging (below)
    if (CW && to_stage) {
        tail = make_float4(0.f, 0.f, 0.f, 0.f);       // obs[72] is the agent's LUT entry (below)
    } else if (q == 0) {
        tail = make_float4(g.facing == 0 ? 1.0f : 0.0f, g.facing == 1 ? 1.0f : 0.0f, g.facing == 2 ? 1.0f : 0.0f,
                           g.facing == 3 ? 1.0f : 0.0f);                                            // (:279-280)
    } else if (q == 1) {
        tail = make_float4(tab[TAB_ACTION + g.last_action], g.was_near_wall ? 1.0f : 0.0f, g.last_bump ? 1.0f : 0.0f,
                           tab[TAB_CID + g.cid]);                                                   // (:284-287)
    } else if (q == 2) {
        tail = make_float4((float)((double)g.visited / (double)R.total_free), 0.f, 0.f, 0.f);      // (:291)
    } else {
        tail = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (to_stage && CW) {
        // the row's 20 code words: window bytes in obs order, then lane q's tail word
        LdsU32 *l = (LdsU32 *)dst.stage + dst.aslot * 20;
#pragma unroll
        for (int i = 0; i < 4; ++i) l[4 * i + q] = win[i];
        const uint32_t w0 = TC_ZERO4 + ((TC_ONE - TC_ZERO) << (8 * g.facing));
        const uint32_t w1 = (TC_ACT + (uint32_t)g.last_action) | ((g.was_near_wall ? TC_ONE : TC_ZERO) << 8) |
                            ((g.last_bump ? TC_ONE : TC_ZERO) << 16) | ((TC_CID + (uint32_t)g.cid) << 24);
        const uint32_t c72 = tc_slot((int)(threadIdx.x >> 2));
        // the entry changes only with visited (a newly explored cell, a
        // reset) and is stale at launch start: the f64 division only then
        if (q == 2 && (FRESH || explored || lut_stale))
            const_cast<float *>(tab)[tab_ix(c72)] = (float)((double)g.visited / (double)R.total_free);   // (:291)
        l[16 + q] = q == 0 ? w0 : q == 1 ? w1 : q == 2 ? (c72 | (TC_ZERO4 & 0xffffff00u)) : TC_ZERO4;
    } else if (to_stage) {
        // float rows (20 float4 per agent): the LDS this costs is free in the
        // byte-mark kernels, whose occupancy the VGPRs set
        LdsF4 *l = (LdsF4 *)dst.stage + dst.aslot * 20;
#pragma unroll
        for (int i = 0; i < 4; ++i) l[4 * i + q] = f4v(code_float4(win[i], tab));
        l[16 + q] = f4v(tail);
    } else if (glb4) {
        // explicit address space: no flat stores; non-temporal like the flush
        GlbF4 *gp = (GlbF4 *)glb4;
#pragma unroll
        for (int i = 0; i < 4; ++i) __builtin_nontemporal_store(f4v(code_float4(win[i], tab)), gp + 4 * i + q);
        __builtin_nontemporal_store(f4v(tail), gp + 16 + q);
    }
    return t;
}


// The out-of-line half of reset (envs/CubicEnv.py:77-108): load_room's
// draws (:407, :462-466) for `seed`, then lane q's share of clearing the new
// room's bricks and both marked-bit planes.  Returns x | y<<8 | z<<16 |
// room<<24.  Reads only through `ec` (device memory), so the step loop
// keeps none of this in registers.
template <int PH, bool PC>
__device__ __noinline__ uint32_t reset_prepare(const EnvConst *ec, uint32_t seed, int8_t *map, int q) {
    MtStream mt;
    mt.seed = seed;
    mt.used = 0;
    mt.err = ec->err;
    mt_first_outputs(seed, mt.buf);
    const int room = ec->use_room_draw ? (int)mt.below((uint32_t)ec->n_rooms) : 0;
    const Room R = load_room_c(ec, room);
    uint32_t s;
    if (R.fixed_start >= 0) s = (uint32_t)R.fixed_start;
    else s = ec->starts[R.start_off + mt.below(R.total_free)];
    {
        const int sx = s & 0xff, sy = (s >> 8) & 0xff, sz = (s >> 16) & 0xff;
        const uint2 rec = ec->rays[R.ray_off + (uint32_t)((sx * R.D + sy) * R.H + sz)];
        if ((rec.y >> 16) & 1u) s = ec->starts[R.start_off + mt.below(R.total_free)];   // start in a wall
    }
    // clear the room's bricks to "unknown" (0x00; PC: the room image, 0x40
    // at the walls), 16 B per lane per store
    uint4 *base = reinterpret_cast<uint4 *>(map);
    const uint4 *img = PC ? reinterpret_cast<const uint4 *>(room_image(reinterpret_cast<const int8_t *>(ec->wimg), room,
                                                                       ec->map_bytes))
                         : nullptr;
    const uint32_t per_brick = (uint32_t)PH;          // 16-byte chunks per brick
    const uint32_t total = (uint32_t)(R.nbx * R.nby) * per_brick;
    for (uint32_t c = (uint32_t)q; c < total; c += 4u) {
        const uint32_t brick = c / per_brick, w = c - brick * per_brick;
        const uint32_t bx = brick / (uint32_t)R.nby, by = brick - bx * (uint32_t)R.nby;
        const uint32_t o = (bx * (uint32_t)ec->nby + by) * per_brick + w;
        base[o] = PC ? img[o] : make_uint4(0u, 0u, 0u, 0u);
    }
    // and both marked-bit planes
    uint4 *pl = reinterpret_cast<uint4 *>(map + ec->xp_off);
    const uint32_t pchunks = ec->plane_bytes / 16u;
    for (uint32_t c = (uint32_t)q; c < pchunks; c += 4u) pl[c] = make_uint4(0u, 0u, 0u, 0u);
    return (s & 0xffffffu) | ((uint32_t)room << 24);
}

// ----------------------------------------------------------------------------
// reset (envs/CubicEnv.py:77-108) for the groups with `need`: draws, clear of
// the new room's bricks and planes in HBM by the 4 lanes, a zero tile, then
// sensing from the start cell.  The old episode's dirty tile is dropped.
// ----------------------------------------------------------------------------
template <int PH, bool PC, typename RT, bool SB, bool DM>
__device__ __forceinline__ void group_reset(const Params &p, int8_t *map, uint64_t *tile, uint32_t &dirty,
                                            PlaneCache &pc_, RT *ps, uint32_t &pdirty, bool need,
                                            uint32_t seed, Agent &g, Room &R, const float *tab, float *obs_row,
                                            uint32_t *stage, int aslot, int q, Stood &st, PendMarks &pend) {
    if (need) {
        pend.valid = 0;          // the ended episode's deferred marks: its map and planes are cleared
        const uint32_t drawn = reset_prepare<PH, PC>(p.envc, seed, map, q);
        const int room = (int)(drawn >> 24);
        R = load_room(p, room);
        room_touch(R);           // settled here, not as "maybe pending" in the step loop
        g.room = room;
        g.x = drawn & 0xff;
        g.y = (drawn >> 8) & 0xff;
        g.z = (drawn >> 16) & 0xff;
        g.facing = 0;
        g.last_action = 0;
        g.done = g.last_bump = g.near_wall = g.was_near_wall = false;
        g.step_count = 0;
        g.visited = 1;
        g.bumps = 0;
        g.cid = 0;
        g.move_mask = 0;
        dirty = 0;
        pc_.row = -1;
        pc_.dirty = 0u;                   // the ended episode's cached row: its planes are cleared
        if (PC) {                         // the planes were cleared: empty sets
#pragma unroll
            for (int k = 0; k < 8; ++k) pset_put(ps, 2 * q + (k >> 2), k & 3, pset_zero<RT>());
            pdirty = 0;
        }
        if (SB) {                         // nothing stood in, no set written back (the planes were cleared)
#pragma unroll
            for (int k = 0; k < 8; ++k) st.row[8 * q + k] = 0u;
            st.xnz = st.ynz = 0u;
            st.chg = 0xfu;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (need) {
        if (SB && q == 0) st.row[g.y] |= 1u << g.x;   // the start column
        bool explored = false;
        const uint2 rec = p.rays[R.ray_off + (uint32_t)((g.x * R.D + g.y) * R.H + g.z)];
        sense_observe<PH, true, PC, RT, DM>(p, map, tile, dirty, pc_, ps, pdirty, g, R, false, explored, tab,
                                            ObsDst{obs_row, nullptr, stage, false, false, aslot}, rec, q, pend);
    }
}

// ----------------------------------------------------------------------------
// the step kernel: 4 lanes per agent, K fused steps, SB3 auto-reset
// ----------------------------------------------------------------------------
#ifndef VN_PHILOX16
#define VN_PHILOX16 1        // one Philox call per lane per 16 steps (striped over the quad)
#endif
#ifndef VN_REWARD_STRIPE
#define VN_REWARD_STRIPE 1   // rollout-buffer call: rewards evaluated and stored per 4-step block
#endif

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
constexpr int AGENTS_PER_BLOCK = BLOCK / GROUP;

#ifndef VN_ENV_PROF
#define VN_ENV_PROF 0   // diagnostics build: per-section shader-clock totals of the step loop (vn_debug_env_prof)
#endif
#ifndef VN_ENV_WT
#define VN_ENV_WT 0     // diagnostics build: each wave's start / end clock of the last launch, nothing else
#endif
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
// 7.32, 128 7.21, 64 7.18 G env-steps/s.
#ifndef VN_PC_BLOCK
#define VN_PC_BLOCK 256
#endif
#ifndef VN_PC_MIN_WAVES
#define VN_PC_MIN_WAVES 4   // waves per SIMD the VGPR budget is set for
#endif
// rows fwd, right, back, left; cols facing N,E,S,W; dirs 0 +x, 1 -x, 2 +y, 3 -y
constexpr uint32_t kMoveDir = (2u << 0) | (0u << 2) | (3u << 4) | (1u << 6)       // fwd
                              | (0u << 8) | (3u << 10) | (1u << 12) | (2u << 14)   // right
                              | (3u << 16) | (1u << 18) | (2u << 20) | (0u << 22)  // back
                              | (1u << 24) | (2u << 26) | (0u << 28) | (3u << 30); // left
#ifndef VN_SETPRIO_FLUSH
#define VN_SETPRIO_FLUSH 2   // issue priority for the obs flush's stores (VN_SETPRIO in env_kernel)
#endif
#ifndef VN_STAGE_OBS
#define VN_STAGE_OBS 1
#endif
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
    if (VN_SETPRIO_FLUSH && (p.prio & 2)) __builtin_amdgcn_s_setprio(VN_SETPRIO_FLUSH);
    // the wave's 16 staged obs rows: contiguous in [K][N][80]
    if (VN_STAGE_OBS && !(VN_ABLATE & 16u)) {
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
    if (VN_SETPRIO_FLUSH && (p.prio & 2)) vn_setprio(bprio);
}

template <int PH, bool EXT, bool FAST, bool RESET_ONLY, int PCM, bool DFL = false>
#ifndef VN_MIN_WAVES_PER_SIMD
#define VN_MIN_WAVES_PER_SIMD 4   // <= 128 VGPRs: the 16 waves of 256 agents per CU resident at once
#endif
__global__ __launch_bounds__((PCM == 1 || PCM == 2) ? VN_PC_BLOCK : BLOCK,
                             (PCM == 1 || PCM == 2) ? VN_PC_MIN_WAVES : VN_MIN_WAVES_PER_SIMD) void env_kernel(Params p) {
    constexpr bool PC = PCM == 1 || PCM == 2;   // plane-set mode
    constexpr bool DM = PCM == 3;                // byte-mark mode, deferred plane marks
    using RT = typename std::conditional<PCM == 2, uint32_t, uint64_t>::type;
    constexpr int kAgents = (PC ? VN_PC_BLOCK : BLOCK) / GROUP;
    constexpr bool CW = PC || (DM && VN_DM_CODES);     // obs staged as code words (STAGE_WORDS), expanded at the flush
    static_assert(!CW || kAgents <= 64, "tc_slot has 64 obs[72] codes per block");
    __shared__ float tab[TAB_SIZE];
    __shared__ __attribute__((aligned(16))) uint64_t tiles[kAgents * TileGeom<PH>::STRIDE];
    // obs rows of the step, staged per wave (STAGE_WORDS) so HBM sees 1 KiB contiguous stores
    constexpr int kStageWords = CW ? STAGE_WORDS : STAGE_WORDS_F;
    __shared__ __attribute__((aligned(16))) uint32_t stage[(kAgents / 16) * kStageWords];
    __shared__ __attribute__((aligned(16))) RT psets[PC ? kAgents * PsetGeom<RT>::STRIDE : 2];
    constexpr bool SB = PCM == 2 && VN_STOOD;
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
    const bool wvalid = VN_WREC && (hot0.x & HOT_WREC);   // the window record holds the start cell's window
    // the record loaded beside the state when the previous step launch wrote them (the host's bit)
    const bool wearly = VN_WREC && !RESET_ONLY && (p.prio & PRIO_WREC_EARLY);
    WrecV<PH> wv;
    if (wearly) wrec_load<PH>(p, ai, q, wv);
    // SB: lane q's share of the stood rows (8q .. 8q + 7) and the nonzero-set masks.
    // A short launch (VN_STOOD_PART, K <= 8) can only reach the rows y - 2 - K ..
    // y + 1 + K: the shares outside them are not loaded (they stay zero in LDS,
    // are never read, and are never written back -- a share is stored only when
    // one of its rows changed, and a reset rewrites all four).  The one-step
    // call reads 1-2 of the 4 shares instead of 128 B per agent.
    uint4 sr0 = make_uint4(0u, 0u, 0u, 0u), sr1 = sr0;
    uint2 nz0 = make_uint2(0u, 0u);
    const bool stood_all = !VN_STOOD_PART || p.K > 8;
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
    pc_.dirty = 0u;
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
                plane_wb_flush(p, map, pc_, q);
            }
            tile_flush<PH>(p, map, tile, g, R, dirty, q);
            if (PC) pset_flush<RT, SB>(p, map, ps, g, R, pdirty, q, st);
            if (SB) {
                __builtin_amdgcn_wave_barrier();
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
    // VN_PREMOVE: the window is filled around the cell after that move, so the
    // first step has no shift (one dependent load round trip less per launch;
    // a one-step launch has three left: state, window, the new cell's ray
    // record).  The move itself still runs in step 0 as usual.
#ifndef VN_PREMOVE
#define VN_PREMOVE 1
#endif
    constexpr bool PREMOVE = VN_PREMOVE;
    uint32_t a16[4] = {0u, 0u, 0u, 0u};          // VN_PHILOX16: the actions of the current 16-step chunk
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
    if (!EXT && VN_PHILOX16) philox_chunk(p.t0);
    uint2 rec0 = make_uint2(0u, 0u);                // PREMOVE: step 0's ray record, loaded with the fill
    if (active) {
        Agent gf = g;                               // the fill's window center
        if (PREMOVE && p.K > 0) {
            int a;
            if (EXT) {
                a = p.actions[i];
            } else if (VN_PHILOX16) {
                const uint32_t w = a16[(uint32_t)(p.t0 >> 2) & 3u];
                a = (int)((w >> (8u * ((uint32_t)p.t0 & 3u))) & 0xffu);
            } else {
                const uint4 o = philox4x32_10(p.policy_seed, p.gid_base + (uint64_t)ai, p.t0 >> 2);
                const uint32_t t3 = (uint32_t)p.t0 & 3u;
                a = (int)__umulhi(t3 == 0u ? o.x : t3 == 1u ? o.y : t3 == 2u ? o.z : o.w, 6u);
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
            if (!(VN_ABLATE & 8192u)) {
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
    uint32_t *wst = VN_STAGE_OBS ? stage + (threadIdx.x >> 6) * kStageWords : nullptr;   // this wave's staging block
    const int aslot = (threadIdx.x & 63) >> 2;
    float abl_sink = 0.f;                             // VN_ABLATE 4096 (diagnostics)

    const int lane = threadIdx.x & 63;
    const int nvalid = (p.N - wave_agent0) * (VN_OBS_DIM / 4);       // float4s of the wave's agents (> 0)
    {
    // the step's outputs stored within the step (measured faster than the
    // deferred order, which also needs more VGPRs than the byte-mark kernels
    // have at 4 waves/SIMD)
    //
    // Work striped over the agent's 4 lanes instead of repeated by each:
    //  * Philox (VN_PHILOX16): lane q computes the 4-step block cb + q of the
    //    16-step chunk cb..cb+3, so one call per lane covers 16 steps; the
    //    four words are broadcast in the quad;
    //  * the rollout-buffer call (FAST, VN_REWARD_STRIPE): each step records
    //    its reward events (12 bits) and after the 4-step block lane q
    //    evaluates step q's f64 reward and stores its reward / terminated /
    //    truncated (one store instruction per output per block).
    constexpr bool STRIPE_R = FAST && VN_REWARD_STRIPE;
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
    // VnTuning::prio bit 6 (default on).
    const int drank = (int)(blockIdx.x / max(1u, gridDim.x / 4u));
    auto base_prio = [&](int kk) -> int {
        return (PC && (p.prio & 64) && p.K >= 8) ? min((drank + (kk >> 2)) & 3, 2) : 0;   // launches of >= 8 steps
    };
    int bprio = base_prio(0);
    if (bprio) vn_setprio(bprio);
    // DFL: chosen by the host (launch_ph: VnTuning::dflush, launches of more
    // than one step, every wave full); a separate instantiation, so the
    // waits of the loop see the same five flush stores on every path
    static_assert(!DFL || (!RESET_ONLY && (DM || PC)), "the deferred flush is for step launches of DM / PC kernels");
    constexpr bool dflush = DFL;
    for (int k = 0; k < p.K;) {
    const uint64_t tb = p.t0 + (uint64_t)k;
    uint32_t acts = 0;                                    // 4 actions, 8 bits each, by (t & 3)
    if (!EXT) {
        if (VN_PHILOX16) {
            if (k != 0 && (tb & 15u) == 0u) philox_chunk(tb);   // k == 0: the prologue's chunk
            const uint32_t sel = (uint32_t)(tb >> 2) & 3u;
            acts = sel == 0u ? a16[0] : sel == 1u ? a16[1] : sel == 2u ? a16[2] : a16[3];
        } else {
            const uint4 o = philox4x32_10(p.policy_seed, p.gid_base + (uint64_t)ai, tb >> 2);
            acts = __umulhi(o.x, 6u) | (__umulhi(o.y, 6u) << 8) | (__umulhi(o.z, 6u) << 16) | (__umulhi(o.w, 6u) << 24);
        }
    }
    if (PC && (p.prio & 64) && p.K >= 8) {   // the rotating base level, every 4-step block
        bprio = base_prio(k);
        vn_setprio(bprio);
    }
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
// wave issue priority (s_setprio) while the step's move is computed and its
// loads issued (3), and while the obs flush's stores are issued (2): of the
// 4 waves on a SIMD the one about to put requests in the memory queues goes
// first, the sensing VALU work of the others fills the gaps.  Paired A/B on
// one env allocation (scripts/ab_same.py, profiles/r05/ab_setprio_paired.log):
// box rooms +3.3 % at 20- and 128-step launches, +0.7 % one-step; P-set rooms
// +0-1 %.  Also priority on the reward stores, the shift commit, the launch's
// flush, or level 1 / 2 on the issue: no better.  Runtime switch per call:
// VnTuning::prio bit 0 (issue) / bit 1 (flush) / bit 6 (the rotating base
// level below), default 67; the compile-time VN_SETPRIO / VN_SETPRIO_FLUSH
// (diagnostics build) set the levels.
#ifndef VN_SETPRIO
#define VN_SETPRIO 3
#endif
            if (VN_SETPRIO && (p.prio & 1)) __builtin_amdgcn_s_setprio(VN_SETPRIO);
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
            // (PREMOVE: the launch's window was filled around step 0's cell)
            const bool shifted = moved && dir < 4 && !(PREMOVE && k == 0);
            ShiftLoad<PH> sl;
            SetLoad<RT> pl;
            if (shifted) tile_shift_issue<PH, SB>(p, map, tile, dir, g.x, g.y, R, dirty, q, sl, st, g.room);
            if (PC && shifted) pset_shift_issue<RT, SB>(p, map, ps, dir, g.x, g.y, R, pdirty, q, pl, st);
            uint2 rec;
            if (VN_ABLATE & 8192u) {   // diagnostics: the record computed for a walled box (exact for box rooms only)
                const uint32_t ex = (uint32_t)(R.W - 2 - g.x) | 0x80u, wx = (uint32_t)(g.x - 1) | 0x80u;
                const uint32_t ey = (uint32_t)(R.D - 2 - g.y) | 0x80u, wy = (uint32_t)(g.y - 1) | 0x80u;
                const uint32_t ez = (uint32_t)(R.H - 2 - g.z) | 0x80u, wz = (uint32_t)(g.z - 1) | 0x80u;
                rec = make_uint2(ex | (wx << 8) | (ey << 16) | (wy << 24), ez | (wz << 8));
            } else if (PREMOVE && k == 0) {
                rec = rec0;
            } else {
                rec = p.rays[R.ray_off + (uint32_t)((g.x * R.D + g.y) * R.H + g.z)];
            }
            if (!PC) plane_prefetch<PH>(p, map, pc_, g.x, g.y, g.z, q);
            if (VN_SETPRIO && (p.prio & 1)) vn_setprio(bprio);
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
            }   // !STRIPE_R
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
    }
    if constexpr (DFL) wave_obs_flush<CW, true>(p, wst, tab, p.K - 1, wave_agent0, nvalid, lane, abl_sink, bprio);      // the launch's last step's rows
    }
    if (active) {
        if constexpr (DM) {
            pend_apply<PH>(p, map, pc_, pend, q);   // the last step's deferred marks
            plane_wb_flush(p, map, pc_, q);
        }
        if (!(VN_ABLATE & 32768u)) {   // diagnostics: 32768 skips the launch's flush
            tile_flush<PH>(p, map, tile, g, R, dirty, q);
            if (PC) pset_flush<RT, SB>(p, map, ps, g, R, pdirty, q, st);
        }
        const bool wsave = VN_WREC && (p.prio & PRIO_WREC_SAVE);   // the window record for the next launch (host: K <= wrec_k)
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
        if (active && ((c >> q) & 1u)) {
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
        const unsigned wg = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        if (wg < 8192u) {
            g_env_wt[2 * wg] = rkern;
            g_env_wt[2 * wg + 1] = rend;
            g_env_wid[2 * wg] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
            g_env_wid[2 * wg + 1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        }
    }
#elif VN_ENV_WT
    if (FAST && (threadIdx.x & 63) == 0) {
        __builtin_amdgcn_s_waitcnt(0);   // the wave's stores retired
        const uint64_t rend = __builtin_amdgcn_s_memrealtime();
        const unsigned wg = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        if (wg < 8192u) {
            g_env_wt[2 * wg] = rkern;
            g_env_wt[2 * wg + 1] = rend;
            g_env_wid[2 * wg] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
            g_env_wid[2 * wg + 1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        }
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
    if (RESET_ONLY)
        hipLaunchKernelGGL((env_kernel<PH, false, false, true, PCM>), grid, block, 0, s, p);
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
    return launch_pcm<false>(pcm, p, s);
}

// The kernel instantiation launch picks for a call shape of p.K steps
// (diagnostics / bench labels); kept next to launch so the two selections agree.
std::string label(bool reset_only, bool ext, bool fast, int defer, const void *params) {
    const Params &p = *static_cast<const Params *>(params);
    char buf[160];
    const int pcm = env_pcm(p.ph, p.pcache, defer);
    const bool x = !reset_only && ext, f = !reset_only && fast;
    const bool dfl = !reset_only && !x && use_dfl(pcm, p.N, p.K, p.dflush);
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
