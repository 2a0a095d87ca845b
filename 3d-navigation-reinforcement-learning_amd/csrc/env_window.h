// env_window.h -- CubicEnv kernel unit (included by voxnav_env.hip only): the
// agent's window of belief columns in LDS and its traffic with the byte map.
//
// ----------------------------------------------------------------------------
// Per-agent LDS tile: the 16 window columns, toroidally indexed by
// slot = (x & 3) << 2 | (y & 3).  The window [x-2, x+1] x [y-2, y+1] covers
// each residue pair exactly once, so the tile always holds exactly the
// current window; after a horizontal move the 4 columns entering the window
// take the slots of the 4 leaving it.  Dirty slots are written back on
// eviction and at the end of the launch.
// ----------------------------------------------------------------------------
#pragma once

#include "env_core.h"
#include "env_planes.h"

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

}  // namespace
