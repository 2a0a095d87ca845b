// simple_bits.h -- simpleEnv, bit-plane layouts: ray directions, the S / Q planes and the observation from them.
// Included by voxnav_simple.hip only.
#pragma once

#include "env_core.h"

namespace {

// absolute ray directions of the relative moves (envs/simpleEnv.py:153-158,
// :224-231) in the ray-record byte order 0:+x 1:-x 2:+y 3:-y 4:+z 5:-z
constexpr int kRelDir[4][4] = {
    {2, 0, 3, 1},   // forward  (N, E, S, W)
    {0, 3, 1, 2},   // right
    {3, 1, 2, 0},   // backward
    {1, 2, 0, 3},   // left
};
constexpr uint32_t pack_rel_dir() {
    uint32_t v = 0;
    for (int a = 0; a < 4; ++a)
        for (int f = 0; f < 4; ++f) v |= (uint32_t)kRelDir[a][f] << (2 * (4 * a + f));
    return v;
}
// 2-bit fields in one immediate: no memory lookups on the step's critical path
__device__ __forceinline__ int rel_dir(int a, int facing) {
    return (int)((pack_rel_dir() >> (2 * (4 * a + facing))) & 3u);
}
// +x -> east(1), -x -> west(3), +y -> north(0), -y -> south(2)
__device__ __forceinline__ int facing_of(int d) { return (int)((0x8Du >> (2 * d)) & 3u); }

// obs slot of absolute direction j < 4 for facing f: slot k with rel_dir of
// [fwd, left, right, back][k] == j
constexpr uint32_t pack_obs_slot() {
    uint32_t v = 0;
    const int rel_of_slot[4] = {0, 3, 1, 2};   // forward, left, right, backward (action indices)
    for (int f = 0; f < 4; ++f)
        for (int k = 0; k < 4; ++k) v |= (uint32_t)k << (2 * (4 * f + kRelDir[rel_of_slot[k]][f]));
    return v;
}
__device__ __forceinline__ int obs_slot(int j, int facing) {
    return j >= 4 ? j : (int)((pack_obs_slot() >> (2 * (4 * facing + j))) & 3u);
}

// ============================================================================
// simpleEnv, bit-plane layout (rooms up to 64 x 64 x 31; larger rooms use the
// dense kernel above).  The belief map is not stored as bytes.  Per agent:
//   S  the agent has stood on the cell: internal_grid == 1 (:86, :294), or a
//      visited cell the edge quirk later turned into 2.  Kept in three axis
//      planes so that a ray along any axis is one word:
//      SX[y][z] (bit x, u64), SY[x][z] (bit y, u64), SZ[x][y] (bit z, u32)
//   Q  edge-quirk mark: the last in-room cell of a ray that leaves the room
//      becomes 2 (:311-319).  QZ[x][y] (bit z, u32); agent flag in hot.w
// Every other internal_grid value is a function of S, Q and the walls: the
// positions the agent has sensed from are exactly its S cells (reset and
// every step observe where the agent stands, and every such cell is marked),
// so a cell is known -- 0 if free, 2 if wall -- iff an S cell lies within L
// cells of it along an axis with only free cells in between (:301-337).
// export_belief derives the map; the step reads only S and Q.  In-run obs
// values: Q ? 2 : S ? 1 : 0.
// ============================================================================
struct SPlanes {
    uint64_t *sx, *sy;
    uint32_t *sz, *qz;
};

__device__ __forceinline__ SPlanes splanes(const Params &p, int agent) {
    int8_t *b = p.belief + (size_t)agent * p.agent_bytes;
    SPlanes q;
    q.sx = reinterpret_cast<uint64_t *>(b);
    q.sy = reinterpret_cast<uint64_t *>(b + p.sy_off);
    q.sz = reinterpret_cast<uint32_t *>(b + p.sz_off);
    q.qz = reinterpret_cast<uint32_t *>(b + p.qz_off);
    return q;
}

// cached S words through the agent's cell + the cell's ray record
struct SRows {
    uint64_t wx, wy;
    uint32_t wz;
    uint2 rec;
};

__device__ __forceinline__ uint32_t ray_e8(uint2 rec, int d) {
    return ((d < 4 ? rec.x : rec.y) >> (8 * (d & 3))) & 0xffu;
}

// simple_ray on the bit planes: obs values of ray d (L floats) from the S
// word along the ray axis, Q bits looked up only when the agent has any;
// then the edge-quirk mark.  Returns count * 0.25.
// (scalars by value: a select over struct fields folds into a dynamic load
// from a stack copy of the struct)
template <int LMAX>
__device__ __forceinline__ float sb_ray(const Params &p, const SPlanes &pl, int gx, int gy, int gz, bool hasq,
                                        uint64_t wx, uint64_t wy, uint32_t wz, uint2 rec, int d, float *out,
                                        bool &newq) {
    const uint32_t e8 = ray_e8(rec, d);
    const int n = (int)(e8 & 0x7fu);
    const int L = p.L;
    const int m = n < L ? n : L;
    const int ax = d >> 1;
    const int sgn = (d & 1) ? -1 : 1;
    const uint64_t run = ax == 0 ? wx : ax == 1 ? wy : (uint64_t)wz;
    const int pos = ax == 0 ? gx : ax == 1 ? gy : gz;
#pragma unroll
    for (int s = 0; s < LMAX; ++s) {
        if (s >= L) break;
        float v;
        if (s < m) {
            const int c = pos + sgn * (s + 1);
            uint32_t b = (uint32_t)(run >> c) & 1u;
            if (hasq) {
                const int qx = ax == 0 ? c : gx, qy = ax == 1 ? c : gy, qzz = ax == 2 ? c : gz;
                if ((pl.qz[qx * p.pd + qy] >> qzz) & 1u) b = 2u;
            }
            v = (float)b;
        } else {
            v = s == n ? 2.0f : -1.0f;   // wall / edge terminator, then padding (:321-331)
        }
        out[s] = v;
    }
    if (n < L && !(e8 & 0x80u) && n >= 1) {   // edge quirk (:311-319)
        const int c = pos + sgn * n;
        const int qx = ax == 0 ? c : gx, qy = ax == 1 ? c : gy, qzz = ax == 2 ? c : gz;
        uint32_t *q = pl.qz + qx * p.pd + qy;
        // no Q bit anywhere yet -> the word is 0 (up and down share a column)
        const uint32_t old = (hasq || newq) ? *q : 0u;
        if (!((old >> qzz) & 1u)) *q = old | (1u << qzz);
        newq = true;
    }
    return (float)m * 0.25f;                 // round(count * 0.25, 2) is exact
}

template <int LMAX>
__device__ __forceinline__ void sb_observe(const Params &p, const SPlanes &pl, Agent &g, const SRows &w, float *row) {
    const int L = p.L;
    const bool hasq = g.move_mask & 1u;
    bool newq = false;
    const int dirs[6] = {rel_dir(0, g.facing), rel_dir(3, g.facing), rel_dir(1, g.facing),
                         rel_dir(2, g.facing), 4, 5};   // forward, left, right, backward, up, down (:233)
#pragma unroll
    for (int k = 0; k < 6; ++k)
        row[6 * L + k] = sb_ray<LMAX>(p, pl, g.x, g.y, g.z, hasq, w.wx, w.wy, w.wz, w.rec, dirs[k], row + k * L, newq);
    row[6 * L + 6] = (float)g.last_action;
    if (newq) g.move_mask |= 1u;
}

// sb_observe without divergent branches, for waves in which no lane has Q
// marks or stands where a ray ends at the room's edge (ray record bit 17):
// the rays in ABSOLUTE directions (ray axis, sign and S word fixed per ray),
// each written at the obs slot the agent's facing gives it (obs_slot).  Per
// ray cell s < L: the S bit if s < min(n, L), else 2 at s == n (wall), else -1
// (:301-337).  Otherwise the wave takes sb_observe.
template <int LMAX>
__device__ __forceinline__ void sp_observe(const Params &p, const SPlanes &pl, Agent &g, const SRows &w, float *row) {
    const bool slow = (g.move_mask & 1u) || ((w.rec.y >> 17) & 1u);
    if (__builtin_expect(__ballot(slow) != 0ull, 0)) {
        sb_observe<LMAX>(p, pl, g, w, row);
        return;
    }
    const int L = p.L;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const uint32_t e8 = ray_e8(w.rec, j);
        const int n = (int)(e8 & 0x7fu);
        const int m = n < L ? n : L;
        // t: bit s = the S bit of ray cell s + 1
        uint32_t t;
        if (j == 0) t = (uint32_t)(w.wx >> ((g.x + 1) & 63));
        else if (j == 2) t = (uint32_t)(w.wy >> ((g.y + 1) & 63));
        else if (j == 4) t = w.wz >> ((g.z + 1) & 31);
        else if (j == 1) t = __builtin_bitreverse32((uint32_t)((w.wx << ((64 - g.x) & 63)) >> 32));
        else if (j == 3) t = __builtin_bitreverse32((uint32_t)((w.wy << ((64 - g.y) & 63)) >> 32));
        else t = __builtin_bitreverse32(w.wz << ((32 - g.z) & 31));
        float *out = row + obs_slot(j, g.facing) * L;
#pragma unroll
        for (int s = 0; s < LMAX; ++s) {
            if (s >= L) break;
            const float fb = ((t >> s) & 1u) ? 1.0f : 0.0f;
            const float pad = s == n ? 2.0f : -1.0f;
            out[s] = s < m ? fb : pad;
        }
        row[6 * L + obs_slot(j, g.facing)] = (float)m * 0.25f;   // round(count * 0.25, 2) is exact
    }
    row[6 * L + 6] = (float)g.last_action;
}

// Four ray cells at once: entry (bits | (clamp(m - 4c, -1, 4) + 1) << 4) of
// the table holds the obs values of cells 4c..4c+3 of a ray with min(n, L) = m
// free cells whose S bits (cells 4c..4c+3) are `bits`: the S bit below m, 2 at
// m (the wall / edge terminator -- only reached when n < L), -1 beyond.
constexpr int SL_CLUT = 96;
__device__ __forceinline__ void sl_build_cell_lut(float4 *lut, int lane) {
    for (int e = lane; e < SL_CLUT; e += 64) {
        const int bits = e & 15, r = (e >> 4) - 1;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = i < r ? (float)((bits >> i) & 1) : (i == r ? 2.0f : -1.0f);
        lut[e] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// sp_observe with the 4-cell table, for L == LMAX (the ray cells of a launch
// written without per-cell compares or branches)
template <int LMAX>
__device__ __forceinline__ void sl_observe(const Params &p, const SPlanes &pl, Agent &g, const SRows &w, float *row,
                                           const float4 *clut) {
    const bool slow = (g.move_mask & 1u) || ((w.rec.y >> 17) & 1u);
    if (__builtin_expect(__ballot(slow) != 0ull || p.L != LMAX, 0)) {
        sb_observe<LMAX>(p, pl, g, w, row);
        return;
    }
    constexpr int L = LMAX;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const uint32_t e8 = ray_e8(w.rec, j);
        const int n = (int)(e8 & 0x7fu);
        const int m = n < L ? n : L;
        uint32_t t;   // bit s = the S bit of ray cell s + 1
        if (j == 0) t = (uint32_t)w.wx >> ((g.x + 1) & 31);
        else if (j == 2) t = (uint32_t)w.wy >> ((g.y + 1) & 31);
        else if (j == 4) t = w.wz >> ((g.z + 1) & 31);
        else if (j == 1) t = __builtin_bitreverse32((uint32_t)w.wx << ((32 - g.x) & 31));
        else if (j == 3) t = __builtin_bitreverse32((uint32_t)w.wy << ((32 - g.y) & 31));
        else t = __builtin_bitreverse32(w.wz << ((32 - g.z) & 31));
        const int slot = obs_slot(j, g.facing);
        float *out = row + slot * L;
#pragma unroll
        for (int c = 0; c < (L + 3) / 4; ++c) {
            const int r = min(max(m - 4 * c, -1), 4);
            const float4 q = clut[((t >> (4 * c)) & 15u) | ((uint32_t)(r + 1) << 4)];
            out[4 * c] = q.x;
            if (4 * c + 1 < L) out[4 * c + 1] = q.y;
            if (4 * c + 2 < L) out[4 * c + 2] = q.z;
            if (4 * c + 3 < L) out[4 * c + 3] = q.w;
        }
        row[6 * L + slot] = (float)m * 0.25f;   // round(count * 0.25, 2) is exact
    }
    row[6 * L + 6] = (float)g.last_action;
}

__device__ __forceinline__ void sb_load_rows(const Params &p, const SPlanes &pl, const Agent &g, const Room &R,
                                             SRows &w) {
    w.wx = pl.sx[g.y * p.ph + g.z];
    w.wy = pl.sy[g.x * p.ph + g.z];
    w.wz = pl.sz[g.x * p.pd + g.y];
    w.rec = p.rays[R.ray_off + (uint32_t)((g.x * R.D + g.y) * R.H + g.z)];
}

}  // namespace
