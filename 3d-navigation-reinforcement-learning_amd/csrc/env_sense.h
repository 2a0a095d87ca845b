// env_sense.h -- CubicEnv kernel unit (included by voxnav_env.hip only): the
// sensing pass on the agent's tile, with the observation row it writes, and
// the reset that starts an episode with one.
#pragma once

#include "env_core.h"
#include "env_planes.h"
#include "env_window.h"

namespace {

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
    RT pmr = 0;                             // PC: the span mask, in the row's own width
    if constexpr (PC) {
        // a plane row is one RT word (rooms of at most 8 * sizeof(RT) columns): the marked span
        // [pa, pb] lies inside it, so mask and merge are one word of that width
        if (q < 2) {
            const bool xr = q == 0;
            const int nfp1 = xr ? ry.nf[0] : ry.nf[2], nfm1 = xr ? ry.nf[1] : ry.nf[3];
            const bool whp = xr ? ry.wh[0] : ry.wh[2], whm = xr ? ry.wh[1] : ry.wh[3];
            const int a = pcoord - nfm1 - (whm ? 1 : 0), b = pcoord + nfp1 + (whp ? 1 : 0);
            pmr = (RT)((RT)~(RT)0 >> (8 * (int)sizeof(RT) - 1 - (b - a))) << a;
        }
    } else if (q < 2) {
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
        if (FRESH) {                // planes were cleared by the reset
            pc_.row = rowi;
            pc_.w0 = nw <= 2 ? 0 : pw0;
            pc_.w[0] = pc_.w[1] = 0ull;
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
            const RT nv = prw | pmr;
            if (nv != prw) {
                *prow_lds = nv;
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
    constexpr bool CW = PC || DM;   // code-word staging (below)
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

}  // namespace
