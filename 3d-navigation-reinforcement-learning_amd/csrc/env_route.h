// env_route.h -- the frontier planner's rule (vn_plan_frontier, DESIGN.md
// 10.3) on bit rows: from an agent's belief map, the first action of a
// shortest known-free path to the nearest cell that is known free and not yet
// visited.  The map arrives as two sets of 64-bit rows over x, one row per
// (y, z) at index y * ph + z, bit x:
//   pass    cells inside the room whose belief value is >= 0 (known free or
//           visited); unknown cells and walls are not passable
//   target  passable cells whose value is 0
// This header holds the action -> direction table (do_action,
// envs/CubicEnv.py:135-153), one breadth-first flood step on the rows, the
// test of the agent's six neighbour cells, the pick and the fallback, and the
// same search carried on until each of the six neighbours has its own distance
// (vn_plan_frontier_dists).  Plain
// C++17 with no HIP include (like env_plan.h / env_state.h): every function is
// VN_HD, the loops take (tid, nth), and the block's barrier and vote come in
// as a small object, so that the planning kernel (voxnav_plan.hip, one wave
// per agent) and the stand-alone host drivers (tests/host/route_check.cpp and
// route_dists_check.cpp, one thread, under the sanitizers) run the same code.  Anonymous namespace: one
// copy per unit.
#pragma once

#include <cstdint>

#include "env_plan.h"

namespace {

constexpr int RT_ACTIONS = 6;
constexpr int RT_MAX_W = 64;       // one 64-bit row over x

// The move of action k under facing f.  0-3 are forward / right / backward /
// left relative to the facing: the heading moved along is (f + k) mod 4 with
// 0 = +y, 1 = +x, 2 = -y, 3 = -x (the four rows of directions_relative_to_facing);
// 4 is +z, 5 is -z.
VN_HD void rt_move(int k, int f, int *dx, int *dy, int *dz) {
    const int8_t heading[4][2] = {{0, 1}, {1, 0}, {0, -1}, {-1, 0}};
    *dx = *dy = *dz = 0;
    if (k >= 4) {
        *dz = k == 4 ? 1 : -1;
        return;
    }
    const int h = (f + k) & 3;
    *dx = heading[h][0];
    *dy = heading[h][1];
}

// the room and the row stride of one agent's rows
struct RtGeom {
    int W, D, H;     // the agent's room: only rows y < D, z < H exist, only bits x < W may be set
    int ph;          // row index = y * ph + z
};

VN_HD bool rt_inside(const RtGeom &g, int x, int y, int z) {
    return x >= 0 && x < g.W && y >= 0 && y < g.D && z >= 0 && z < g.H;
}

// bits x < W
VN_HD uint64_t rt_width_mask(int W) { return W >= 64 ? ~0ull : ((1ull << W) - 1ull); }

// row (y, z), or 0 outside the room
VN_HD uint64_t rt_row(const uint64_t *rows, const RtGeom &g, int y, int z) {
    return (y >= 0 && y < g.D && z >= 0 && z < g.H) ? rows[y * g.ph + z] : 0ull;
}

// One flood step of row (y, z): the row, its own bits moved one cell in +x
// and -x (a bit leaving the word at either end is dropped) and the four
// neighbour rows, kept where passable.
VN_HD uint64_t rt_flood_row(const uint64_t *pass, const uint64_t *cur, const RtGeom &g, int y, int z) {
    const uint64_t w = cur[y * g.ph + z];
    const uint64_t n = w | (w << 1) | (w >> 1) | rt_row(cur, g, y - 1, z) | rt_row(cur, g, y + 1, z) |
                       rt_row(cur, g, y, z - 1) | rt_row(cur, g, y, z + 1);
    return n & pass[y * g.ph + z];
}

// This thread's rows of one flood step, cur -> nxt (two buffers: every row of
// the step reads the previous set, exact breadth-first order); whether one of
// them grew.
VN_HD bool rt_flood_pass(const uint64_t *pass, const uint64_t *cur, uint64_t *nxt, const RtGeom &g, int tid, int nth) {
    bool grew = false;
    const int rows = g.D * g.H;
    for (int c = tid; c < rows; c += nth) {
        const int y = c / g.H, z = c - y * g.H;
        const uint64_t n = rt_flood_row(pass, cur, g, y, z);
        nxt[y * g.ph + z] = n;
        grew = grew || n != cur[y * g.ph + z];
    }
    return grew;
}

// The neighbour test: bit k is set when n_k, the cell action k moves to from
// (x, y, z) under facing f, is inside the room and in `rows`.
VN_HD uint32_t rt_neighbours_in(const uint64_t *rows, const RtGeom &g, int x, int y, int z, int f) {
    uint32_t m = 0u;
    for (int k = 0; k < RT_ACTIONS; ++k) {
        int dx, dy, dz;
        rt_move(k, f, &dx, &dy, &dz);
        const int nx = x + dx, ny = y + dy, nz = z + dz;
        if (rt_inside(g, nx, ny, nz) && ((rows[ny * g.ph + nz] >> nx) & 1ull)) m |= 1u << k;
    }
    return m;
}

// the pick: the lowest action of a nonzero neighbour mask
VN_HD int rt_lowest(uint32_t m) {
    int k = 0;
    while (k < RT_ACTIONS - 1 && !((m >> k) & 1u)) ++k;
    return k;
}

// The fallback: v[k] is the belief value of n_k (below 0: not passable,
// outside the room included).  The passable neighbour with the smallest value,
// ties to the lowest k; 0 when none is passable.
VN_HD int rt_fallback(const int *v) {
    int best = 0, bv = -1;
    for (int k = 0; k < RT_ACTIONS; ++k)
        if (v[k] >= 0 && (bv < 0 || v[k] < bv)) {
            best = k;
            bv = v[k];
        }
    return best;
}

// The search.  `ra` holds the targets (R_0) on entry, `rb` is the second
// buffer; R_j = (R_j-1 and its six-neighbours) & pass.  Found: the smallest j
// with a neighbour n_k in R_j -- R_j is passable by construction -- gives the
// lowest such k and dist = j + 1.  Fallback (dist -1): the flood stopped
// growing first, or ran `cap` steps (the cells of the padded room: more than
// any flood can grow).
// blk.sync() is the block's barrier and blk.any(v) its barrier with an OR
// vote; both are reached by every thread the same number of times, because
// every exit below depends on values all threads hold alike (rows read after
// a barrier, the vote's result).
template <class Blk>
VN_HD void rt_search(const Blk &blk, const uint64_t *pass, uint64_t *ra, uint64_t *rb, const RtGeom &g, int x, int y,
                     int z, int f, const int *nv, int cap, int tid, int nth, int *action, int *dist) {
    uint64_t *cur = ra, *nxt = rb;
    blk.sync();                                   // pass and R_0 are written
    for (int j = 0;; ++j) {
        const uint32_t hit = rt_neighbours_in(cur, g, x, y, z, f);
        if (hit) {
            *action = rt_lowest(hit);
            *dist = j + 1;
            return;
        }
        if (j >= cap) break;
        if (!blk.any(rt_flood_pass(pass, cur, nxt, g, tid, nth))) break;
        uint64_t *t = cur;
        cur = nxt;
        nxt = t;
    }
    *action = rt_fallback(nv);
    *dist = -1;
}

// ---- the per-action distances (vn_plan_frontier_dists) ----
constexpr int RT_UNREACHED = -1;   // n_k is passable and the flood never contained it
constexpr int RT_BLOCKED = -2;     // n_k is not passable

// The search for all six actions, on the same rows and buffers as rt_search:
// dists[k] = j + 1 with j the smallest index such that n_k is in R_j,
// RT_UNREACHED where the flood stopped growing (or ran `cap` steps) before it
// contained the passable n_k, RT_BLOCKED where n_k is not passable (nv[k] < 0).
// It ends as soon as every passable neighbour has its distance.  The barriers
// follow rt_search's rule: every exit depends on values all threads hold
// alike.  dists is the caller's own array of RT_ACTIONS; the loops over it
// have constant bounds (unrolled, its entries stay in registers).
template <class Blk>
VN_HD void rt_search_all(const Blk &blk, const uint64_t *pass, uint64_t *ra, uint64_t *rb, const RtGeom &g, int x,
                         int y, int z, int f, const int *nv, int cap, int tid, int nth, int *dists) {
    blk.sync();                                   // pass, R_0 and nv are written
    uint32_t want = 0u;
#pragma unroll
    for (int k = 0; k < RT_ACTIONS; ++k) {
        dists[k] = nv[k] >= 0 ? RT_UNREACHED : RT_BLOCKED;
        want |= nv[k] >= 0 ? 1u << k : 0u;
    }
    uint64_t *cur = ra, *nxt = rb;
    for (int j = 0;; ++j) {
        const uint32_t hit = rt_neighbours_in(cur, g, x, y, z, f) & want;   // R_j grows: a neighbour's first j
#pragma unroll
        for (int k = 0; k < RT_ACTIONS; ++k)
            if ((hit >> k) & 1u) dists[k] = j + 1;
        want &= ~hit;
        if (!want || j >= cap) break;
        if (!blk.any(rt_flood_pass(pass, cur, nxt, g, tid, nth))) break;
        uint64_t *t = cur;
        cur = nxt;
        nxt = t;
    }
}

// the smallest positive entry of dists, or -1 when none is positive
VN_HD int rt_min_dist(const int *dists) {
    int m = -1;
#pragma unroll
    for (int k = 0; k < RT_ACTIONS; ++k)
        if (dists[k] > 0 && (m < 0 || dists[k] < m)) m = dists[k];
    return m;
}

// best: bit k is set iff dists[k] is positive and the smallest positive entry
VN_HD uint32_t rt_best_set(const int *dists) {
    const int m = rt_min_dist(dists);
    uint32_t b = 0u;
#pragma unroll
    for (int k = 0; k < RT_ACTIONS; ++k)
        if (m > 0 && dists[k] == m) b |= 1u << k;
    return b;
}

}  // namespace
