// env_planes.h -- CubicEnv kernel unit (included by voxnav_env.hip only): the
// marked-bit planes of the belief and the exchanges inside an agent's 4 lanes.
#pragma once

#include "env_core.h"

namespace {

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
// Stood-column map (PCM 2, rooms <= 32 x 32).  In plane-set mode
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

// Exchanges inside an agent group (4 lanes = one DPP quad): a quad_perm DPP
// move is one VALU instruction, where __shfl is an LDS permute with its
// latency on the step's dependency chain.  QP = quad_perm control
// (2 bits per destination lane: the source lane in the quad).
template <int QP>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, QP, 0xf, 0xf, false);
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
    uint32_t unused;     // what a write-back experiment left: without it four kernels schedule differently
};

// byte (x, y, z) of the bricked map (bcol: env_plan.h); here, not with the
// window code that uses it most, because pend_apply below writes map bytes too
// and env_window.h needs this header's Stood and pset_known
template <int PH>
__device__ __forceinline__ uint32_t boff(int x, int y, int z, int nby) {
    return bcol(x, y, nby) * (uint32_t)PH + (uint32_t)z;
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
                pc_.row = rowi;
                pc_.w0 = 0;
                pc_.w[0] = prow[0];
                pc_.w[1] = nw > 1 ? prow[1] : 0ull;
            }
        }
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
            if (!(VN_ABLATE & 2097184u)) prow[pend.pw0] = nv;   // 32 | 2097152: diagnostics
        }
        if (nwd1) {
            const uint64_t nv = pn1 | pend.pm1;
            if (pofs == 0) pc_.w[1] = nv;
            if (!(VN_ABLATE & 2097184u)) prow[pend.pw0 + 1] = nv;
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

}  // namespace
