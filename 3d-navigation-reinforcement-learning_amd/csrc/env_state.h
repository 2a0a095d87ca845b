// env_state.h -- the encoder of a CubicEnv agent's memory state: what
// vn_import_state writes for one agent, given its exported state row and its
// dense belief map.  The export kernels (voxnav_env.hip export_state_kernel,
// export_belief_kernel) are the decoders; this header is the other direction
// and the one place where the invariants of the per-agent memory at a launch
// boundary are stated:
//   * the per-cell codec (dense internal_grid value <-> belief byte) and the
//     validation predicates of an imported agent;
//   * the sensing marks of get_obs from the agent's cell (envs/CubicEnv.py
//     :254-312, :345-397), applied to the imported map;
//   * the bricked byte map, both marked-bit planes, the stood-column rows and
//     the nonzero-set masks of every belief layout (EnvLayout::pcache).
// Plain C++17 with no HIP include (like env_plan.h): every function is VN_HD,
// the loops take (tid, nth) so that the import kernel (voxnav_state.hip, one
// wave per agent) and the stand-alone host driver
// (tests/host/env_import_check.cpp, one thread, under the sanitizers) run the
// same code.  Anonymous namespace: one copy per unit.
#pragma once

#include <cstddef>
#include <cstdint>

#include "env_plan.h"

namespace {

// belief byte: bit7 known, bit6 wall, bits0-5 visit count (env_core.h);
// 0x40 alone = latent wall (plane-set modes: a wall cell not yet known)
constexpr uint32_t VS_KNOWN = 0x80u, VS_WALL = 0xC0u, VS_LATENT = 0x40u;
constexpr int VS_COUNT_MAX = 63;                 // the visit count saturates
constexpr int64_t VS_STEP_MAX = 0xffffff;        // step_count: 24 bits of the hot state, saturating
constexpr int64_t VS_BUMP_MAX = 0x3ffffff;       // bump_count: 26 bits, saturating
constexpr int64_t VS_SEED_LIMIT = 1ll << 32;

// the state row's fields (vn_export_state)
enum {
    VS_X = 0, VS_Y, VS_Z, VS_FACING, VS_LAST_ACTION, VS_STEP_COUNT, VS_VISITED, VS_BUMPS, VS_DONE, VS_LAST_BUMP,
    VS_NEAR_WALL, VS_WAS_NEAR_WALL, VS_CID, VS_ROOM, VS_MAX_STEPS, VS_NEXT_SEED
};

// ----------------------------------------------------------------------------
// per-cell codec
// ----------------------------------------------------------------------------
// dense value -> byte.  `latent`: the layout keeps the latent-wall bit at wall
// cells that are still unknown (plane-set modes).  A count above 63 is
// clamped, as the device map saturates.
VN_HD uint32_t vs_encode(int v, bool wall, bool latent) {
    if (v == -2) return VS_WALL;
    if (v < 0) return (wall && latent) ? VS_LATENT : 0u;
    return VS_KNOWN | (uint32_t)(v > VS_COUNT_MAX ? VS_COUNT_MAX : v);
}

// byte (+ whether a marked-bit plane holds the cell) -> dense value: export_belief_kernel's rule
VN_HD int vs_decode(uint32_t b, bool in_plane) {
    const bool known = (b & VS_KNOWN) != 0u || in_plane;
    return known ? ((b & VS_LATENT) ? -2 : (int)(b & 0x3fu)) : -1;
}

// an imported cell inside the room: nothing below -2, -2 only at a wall of
// the room, a known free value only where the room has no wall
VN_HD bool vs_cell_ok(int v, bool wall) { return v >= -2 && (v != -2 || wall) && (v < 0 || !wall); }

VN_HD int64_t vs_clamp_steps(int64_t v) { return v > VS_STEP_MAX ? VS_STEP_MAX : v; }
VN_HD int64_t vs_clamp_bumps(int64_t v) { return v > VS_BUMP_MAX ? VS_BUMP_MAX : v; }

// ----------------------------------------------------------------------------
// validation of the state row.  vs_scalars_ok reads the row alone and runs
// first: only a row that passes it names a room whose descriptor may be
// loaded; vs_pos_ok then needs that room's size, and only a position that
// passes it may index the room's ray records or the agent's map.
// ----------------------------------------------------------------------------
VN_HD bool vs_scalars_ok(const int64_t *s, int n_rooms, int L) {
    bool ok = s[VS_ROOM] >= 0 && s[VS_ROOM] < n_rooms;
    ok = ok && s[VS_FACING] >= 0 && s[VS_FACING] <= 3;
    ok = ok && s[VS_LAST_ACTION] >= 0 && s[VS_LAST_ACTION] <= 5;
    for (int f = VS_DONE; f <= VS_WAS_NEAR_WALL; ++f) ok = ok && (s[f] == 0 || s[f] == 1);
    ok = ok && s[VS_CID] >= 0 && s[VS_CID] <= L;
    ok = ok && s[VS_NEXT_SEED] >= 0 && s[VS_NEXT_SEED] < VS_SEED_LIMIT;
    ok = ok && s[VS_STEP_COUNT] >= 0 && s[VS_VISITED] >= 0 && s[VS_BUMPS] >= 0;
    return ok;
}

// the position inside the room; the visited count at most the room's cells
VN_HD bool vs_pos_ok(const int64_t *s, int W, int D, int H) {
    return s[VS_X] >= 0 && s[VS_X] < W && s[VS_Y] >= 0 && s[VS_Y] < D && s[VS_Z] >= 0 && s[VS_Z] < H &&
           s[VS_VISITED] <= (int64_t)W * D * H;
}

// ----------------------------------------------------------------------------
// the sensing pass of get_obs from the agent's cell
// ----------------------------------------------------------------------------
struct VsRays {
    int nf[6];             // free cells seen in +x, -x, +y, -y, +z, -z (at most L)
    bool wh[6];            // the ray ends at a wall inside the view
    bool near;             // a wall one cell away (near_wall, :378-379)
    bool wall;             // the cell itself is a wall
    uint32_t move_mask;    // bit d: the first cell in direction d is free
};

// from the room's 8-byte ray record of the cell (RayRec, env_plan.h)
VN_HD VsRays vs_rays(uint32_t rx, uint32_t ry, int L) {
    VsRays r;
    r.near = false;
    r.move_mask = 0u;
    for (int d = 0; d < 6; ++d) {
        const uint32_t e = (d < 4 ? (rx >> (8 * d)) : (ry >> (8 * (d - 4)))) & 0xffu;
        const int n = (int)(e & 0x7fu);
        const bool wf = (e >> 7) != 0u;
        r.nf[d] = n < L ? n : L;
        r.wh[d] = wf && n < L;
        r.near = r.near || (n == 0 && wf);
        r.move_mask |= (n > 0 ? 1u : 0u) << d;
    }
    r.wall = ((ry >> 16) & 1u) != 0u;
    return r;
}

// what the pass ORs into the cell at offset (dx, dy, dz) from the agent:
// KNOWN along a free run, WALL at the wall that ends it, 0 elsewhere
VN_HD uint32_t vs_sense_mark(const VsRays &r, int dx, int dy, int dz) {
    int dir, d;
    if (dx != 0 && dy == 0 && dz == 0) {
        dir = dx > 0 ? 0 : 1;
        d = dx > 0 ? dx : -dx;
    } else if (dx == 0 && dy != 0 && dz == 0) {
        dir = dy > 0 ? 2 : 3;
        d = dy > 0 ? dy : -dy;
    } else if (dx == 0 && dy == 0 && dz != 0) {
        dir = dz > 0 ? 4 : 5;
        d = dz > 0 ? dz : -dz;
    } else {
        return 0u;
    }
    return d <= r.nf[dir] ? VS_KNOWN : (r.wh[dir] && d == r.nf[dir] + 1) ? VS_WALL : 0u;
}

// ----------------------------------------------------------------------------
// one agent whose state row passed vs_scalars_ok / vs_pos_ok
// ----------------------------------------------------------------------------
struct VsAgent {
    int x, y, z;
    int W, D, H;             // its room
    const uint32_t *rays;    // the room's ray records, 2 words per cell, cell (x * D + y) * H + z
    const int8_t *dense;     // its imported map [pw][pd][ph]
    int pd, ph;
    VsRays here;             // the rays of its cell
    bool latent;             // the layout keeps latent-wall bytes (plane-set modes)
};

VN_HD bool vs_is_wall(const VsAgent &a, int x, int y, int z) {
    return ((a.rays[2 * (size_t)((x * a.D + y) * a.H + z) + 1] >> 16) & 1u) != 0u;
}

VN_HD int vs_dense(const VsAgent &a, int x, int y, int z) { return a.dense[((size_t)x * a.pd + y) * a.ph + z]; }

// the belief byte of a cell of the room after the import's sensing pass, in
// the full encoding (known bit in the byte)
VN_HD uint32_t vs_cell_byte(const VsAgent &a, int x, int y, int z) {
    return vs_encode(vs_dense(a, x, y, z), vs_is_wall(a, x, y, z), a.latent) |
           vs_sense_mark(a.here, x - a.x, y - a.y, z - a.z);
}

// this thread's share of the map's validation; thread 0 also checks the agent's own cell
VN_HD bool vs_cells_ok(const VsAgent &a, int tid, int nth) {
    bool ok = tid != 0 || vs_dense(a, a.x, a.y, a.z) >= 1;
    const int cells = a.W * a.D * a.H;
    for (int c = tid; c < cells; c += nth) {
        const int z = c % a.H, y = (c / a.H) % a.D, x = c / (a.H * a.D);
        ok = ok && vs_cell_ok(vs_dense(a, x, y, z), vs_is_wall(a, x, y, z));
    }
    return ok;
}

// a column the agent has stood in: one of its cells has a visit count (a
// count never returns to 0 inside an episode, and only standing in a cell
// raises it)
VN_HD bool vs_stood(const VsAgent &a, int x, int y) {
    for (int z = 0; z < a.H; ++z)
        if (vs_dense(a, x, y, z) >= 1) return true;
    return false;
}

// ----------------------------------------------------------------------------
// the agent's memory block (EnvLayout): byte map, x planes, y planes
// ----------------------------------------------------------------------------
struct VsLayout {
    int pw, pd, ph, nby;
    int pcache;              // 0 byte marks, 1 plane sets in u64 rows, 2 in u32 rows
    int nwx, nwy;            // u64 words per plane row (pcache 2: one u32)
    uint32_t xp_off, yp_off;
};

VN_HD VsLayout vs_layout(const EnvLayout &l) {
    return VsLayout{l.pw, l.pd, l.ph, l.nby, l.pcache, l.nwx, l.nwy, l.xp_off, l.yp_off};
}

// The bricked byte map over the room's bricks (what a reset clears): columns
// outside the room and cells above it are 0.
//   byte-mark modes: every cell in the full encoding.
//   plane-set modes: a column the agent has stood in in the full encoding with
//   the latent bit at its unknown walls; every other column as the room image
//   (0x40 at walls, 0 elsewhere) -- its known cells are in the planes.
VN_HD void vs_write_map(const VsAgent &a, const VsLayout &l, int8_t *map, int tid, int nth) {
    const int ncy = 4 * ((a.D + 3) / 4), cols = 4 * ((a.W + 3) / 4) * ncy;
    for (int c = tid; c < cols; c += nth) {
        const int cx = c / ncy, cy = c % ncy;
        const bool in = cx < a.W && cy < a.D;
        const bool full = in && (l.pcache == 0 || vs_stood(a, cx, cy));
        uint64_t *col = reinterpret_cast<uint64_t *>(map + (size_t)bcol(cx, cy, l.nby) * (size_t)l.ph);
        for (int z0 = 0; z0 < l.ph; z0 += 8) {
            uint64_t w = 0;
            for (int k = 0; k < 8; ++k) {
                const int z = z0 + k;
                if (in && z < a.H) {
                    const uint32_t b = full ? vs_cell_byte(a, cx, cy, z) : (vs_is_wall(a, cx, cy, z) ? VS_LATENT : 0u);
                    w |= (uint64_t)b << (8 * k);
                }
            }
            col[z0 / 8] = w;
        }
    }
}

// Both marked-bit planes, every row of the layout: x-plane row (y, z) holds
// bit x, y-plane row (x, z) bit y, of every KNOWN cell of the room -- so a
// cell reads as known through its byte, its x row or its y row alike, and no
// later ray mark finds a new bit at a cell that has a visit count.  Rows of
// u32 in plane-set mode 2, else nwx / nwy u64 words.  *xnz / *ynz: this
// thread's bits of the nonzero-set masks (bit y': some x-plane row (y', z) is
// nonzero; bit x' likewise for the y planes).
VN_HD void vs_write_planes(const VsAgent &a, const VsLayout &l, int8_t *map, int tid, int nth, uint32_t *xnz,
                           uint32_t *ynz) {
    for (int axis = 0; axis < 2; ++axis) {
        const bool xr = axis == 0;
        const int nw = xr ? l.nwx : l.nwy, rows = (xr ? l.pd : l.pw) * l.ph;
        const int lim_r = xr ? a.D : a.W, lim_b = xr ? a.W : a.D;     // row coordinate / bit coordinate limits
        int8_t *base = map + (xr ? l.xp_off : l.yp_off);
        for (int i = tid; i < rows * nw; i += nth) {
            const int w = i % nw, rz = i / nw, z = rz % l.ph, r = rz / l.ph;
            uint64_t bits = 0;
            if (r < lim_r && z < a.H)
                for (int b = 64 * w; b < lim_b && b < 64 * w + 64; ++b) {
                    const uint32_t v = xr ? vs_cell_byte(a, b, r, z) : vs_cell_byte(a, r, b, z);
                    bits |= (uint64_t)((v >> 7) & 1u) << (b & 63);
                }
            if (l.pcache == 2) reinterpret_cast<uint32_t *>(base)[i] = (uint32_t)bits;
            else reinterpret_cast<uint64_t *>(base)[i] = bits;
            if (bits && r < 32) *(xr ? xnz : ynz) |= 1u << r;
        }
    }
}

// plane-set mode 2: stood-column row y (bit x)
VN_HD uint32_t vs_stood_row(const VsAgent &a, int y) {
    uint32_t bits = 0;
    if (y < a.D)
        for (int x = 0; x < a.W && x < 32; ++x) bits |= (vs_stood(a, x, y) ? 1u : 0u) << x;
    return bits;
}

// the observation's window value index o (0..63) -> the cell's offset from
// the agent: obs[16 i + 4 q + k] is cell (x + i - 2, y + q - 2, z + k - 2)
VN_HD uint32_t vs_window_byte(const VsAgent &a, int o) {
    const int cx = a.x + (o >> 4) - 2, cy = a.y + ((o >> 2) & 3) - 2, cz = a.z + (o & 3) - 2;
    if (cx < 0 || cx >= a.W || cy < 0 || cy >= a.D || cz < 0 || cz >= a.H) return 0u;
    return vs_cell_byte(a, cx, cy, cz);
}

}  // namespace
