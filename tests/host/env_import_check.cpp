// env_import_check.cpp -- runs csrc/env_state.h (the encoder behind
// vn_import_state: per-cell codec, validation predicates, the agent's byte
// map, marked-bit planes, stood rows and masks) outside the library, under
// g++ and the host sanitizers (tests/test_state_import_host.py compiles and
// runs it).  It has no expectations of its own: it reads commands on stdin
// and prints what the header computes.
//
//   codec V WALL LATENT            -> byte=HEX
//   decode BYTE_HEX IN_PLANE       -> value=V
//   cell V WALL                    -> ok=0/1
//   clamp STEPS BUMPS              -> steps=.. bumps=..
//   agent PCACHE_CAP DEFER L NROOMS, then NROOMS lines  W D H WALLS
//        (WALLS: W*D*H characters '0' / '1', index (x*D+y)*H+z), then the 16
//        state fields, then OUTSIDE NCELLS and NCELLS lines  x y z v: the
//        dense map is -1 inside the agent's room and OUTSIDE elsewhere, with
//        the listed cells overridden
//        -> verdict=ok / scalars / position / wall / cells, and for an
//        accepted agent the whole encoded block
//
// Every array is a heap block of exactly the size the layout gives it, so an
// index past one is an AddressSanitizer report; the encoder's loops run as
// one thread (tid 0 of 1) and, again, as 64 interleaved shares.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>

#include "env_state.h"

namespace {

template <typename T>
std::unique_ptr<T[]> exact(size_t n) {   // no slack behind the last element
    return std::unique_ptr<T[]>(new T[n]);
}

int do_agent(std::istream &in) {
    VnTuning tun = {-1, -1, 0, 67, 1, 1, 1};
    int L, n;
    if (!(in >> tun.pcache_cap >> tun.defer >> L >> n) || n < 1) return 2;
    auto whd = exact<int32_t>(3 * (size_t)n);
    std::string all;
    for (int r = 0; r < n; ++r) {
        std::string w;
        for (int k = 0; k < 3; ++k) in >> whd[3 * r + k];
        if (!(in >> w)) return 2;
        all += w;
    }
    auto walls = exact<uint8_t>(all.size());
    for (size_t i = 0; i < all.size(); ++i) walls[i] = all[i] == '1' ? 2 : 0;
    VnRoomSet rs = {n, whd.get(), walls.get(), nullptr, nullptr};
    VnConfig cfg = {};
    cfg.local_map_length = L;
    RoomTables rt;
    if (build_room_tables(rs, cfg, &rt)) return 2;
    const EnvLayout lay = plan_layout(VN_VARIANT_CUBIC, L, rt.maxW, rt.maxD, rt.maxH, tun);
    const VsLayout l = vs_layout(lay);

    auto s = exact<int64_t>(VN_STATE_FIELDS);
    for (int f = 0; f < VN_STATE_FIELDS; ++f)
        if (!(in >> s[f])) return 2;
    int outside, ncells;
    if (!(in >> outside >> ncells)) return 2;
    const size_t dn = (size_t)l.pw * l.pd * l.ph;
    auto dense = exact<int8_t>(dn);
    std::memset(dense.get(), outside, dn);
    const bool room_named = s[VS_ROOM] >= 0 && s[VS_ROOM] < n;
    if (room_named) {
        const int W = whd[3 * s[VS_ROOM]], D = whd[3 * s[VS_ROOM] + 1], H = whd[3 * s[VS_ROOM] + 2];
        for (int x = 0; x < W; ++x)
            for (int y = 0; y < D; ++y)
                for (int z = 0; z < H; ++z) dense[((size_t)x * l.pd + y) * l.ph + z] = -1;
    }
    for (int c = 0; c < ncells; ++c) {
        int x, y, z, v;
        if (!(in >> x >> y >> z >> v)) return 2;
        dense[((size_t)x * l.pd + y) * l.ph + z] = (int8_t)v;
    }

    // the kernel's order: the row alone, the room's size, the cell's rays, the map
    if (!vs_scalars_ok(s.get(), n, L)) return std::printf("verdict=scalars\n"), 0;
    const uint32_t *desc = &rt.desc[(size_t)s[VS_ROOM] * 8];
    VsAgent a = {};
    a.W = (int)(desc[0] & 0xff);
    a.D = (int)((desc[0] >> 8) & 0xff);
    a.H = (int)((desc[0] >> 16) & 0xff);
    if (!vs_pos_ok(s.get(), a.W, a.D, a.H)) return std::printf("verdict=position\n"), 0;
    a.x = (int)s[VS_X];
    a.y = (int)s[VS_Y];
    a.z = (int)s[VS_Z];
    // the room's records as a block of their own: an index past the room is a report
    const size_t nrec = (size_t)a.W * a.D * a.H;
    auto rays = exact<uint32_t>(2 * nrec);
    std::memcpy(rays.get(), &rt.rays[desc[2]], nrec * sizeof(RayRec));
    a.rays = rays.get();
    a.dense = dense.get();
    a.pd = l.pd;
    a.ph = l.ph;
    a.latent = l.pcache != 0;
    const size_t own = (size_t)((a.x * a.D + a.y) * a.H + a.z);
    a.here = vs_rays(rays[2 * own], rays[2 * own + 1], L);
    if (a.here.wall) return std::printf("verdict=wall\n"), 0;
    bool ok = true, ok64 = true;
    ok = vs_cells_ok(a, 0, 1);
    for (int t = 0; t < 64; ++t) ok64 = vs_cells_ok(a, t, 64) && ok64;
    if (ok != ok64) return 3;
    if (!ok) return std::printf("verdict=cells\n"), 0;
    std::printf("verdict=ok\n");

    // one thread, then 64 shares into a second block: the same bytes
    auto map = exact<int8_t>(lay.agent_bytes), map64 = exact<int8_t>(lay.agent_bytes);
    std::memset(map.get(), 0x55, lay.agent_bytes);
    std::memset(map64.get(), 0x55, lay.agent_bytes);
    uint32_t xnz = 0, ynz = 0, xnz64 = 0, ynz64 = 0;
    vs_write_map(a, l, map.get(), 0, 1);
    vs_write_planes(a, l, map.get(), 0, 1, &xnz, &ynz);
    for (int t = 63; t >= 0; --t) {
        vs_write_map(a, l, map64.get(), t, 64);
        vs_write_planes(a, l, map64.get(), t, 64, &xnz64, &ynz64);
    }
    if (std::memcmp(map.get(), map64.get(), lay.agent_bytes) || xnz != xnz64 || ynz != ynz64) return 3;

    std::printf("layout=pw:%d pd:%d ph:%d nby:%d pcache:%d nwx:%d nwy:%d xp_off:%u yp_off:%u agent_bytes:%u\n", l.pw,
                l.pd, l.ph, l.nby, l.pcache, l.nwx, l.nwy, l.xp_off, l.yp_off, lay.agent_bytes);
    std::printf("sense=near:%d cid:%d move_mask:%u\n", (int)a.here.near, a.here.nf[5], a.here.move_mask);
    std::printf("map=");                                  // nonzero bytes of the room's bricks (0x55: never written)
    for (uint32_t o = 0; o < lay.map_bytes; ++o)
        if (map[o]) std::printf("%u:%02x ", o, (unsigned)(uint8_t)map[o]);
    const int rowb = l.pcache == 2 ? 4 : 8;
    for (int axis = 0; axis < 2; ++axis) {
        const uint32_t off = axis ? l.yp_off : l.xp_off;
        const int words = (axis ? l.pw * l.nwy : l.pd * l.nwx) * l.ph;
        std::printf("\n%s=", axis ? "yplane" : "xplane");
        for (int i = 0; i < words; ++i) {
            uint64_t w = 0;
            std::memcpy(&w, map.get() + off + (size_t)i * rowb, rowb);
            if (w) std::printf("%d:%" PRIx64 " ", i, w);
        }
    }
    std::printf("\nnz=%x %x\nstood=", xnz, ynz);
    for (int y = 0; y < 32; ++y) std::printf("%x ", vs_stood_row(a, y));
    std::printf("\nwindow=");
    for (int o = 0; o < 64; ++o) std::printf("%02x ", vs_window_byte(a, o));
    // and back: export_belief_kernel's rule over the written block
    std::printf("\ndecoded=");
    for (int x = 0; x < a.W; ++x)
        for (int y = 0; y < a.D; ++y)
            for (int z = 0; z < a.H; ++z) {
                const uint32_t b = (uint8_t)map[(size_t)bcol(x, y, l.nby) * l.ph + z];
                uint64_t xr = 0, yr = 0;
                std::memcpy(&xr, map.get() + l.xp_off + ((size_t)(y * l.ph + z) * l.nwx + (x >> 6)) * rowb, rowb);
                std::memcpy(&yr, map.get() + l.yp_off + ((size_t)(x * l.ph + z) * l.nwy + (y >> 6)) * rowb, rowb);
                std::printf("%d ", vs_decode(b, ((xr >> (x & 63)) & 1u) || ((yr >> (y & 63)) & 1u)));
            }
    std::printf("\n");
    return 0;
}

}  // namespace

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "codec") {
            int v, wall, latent;
            if (!(std::cin >> v >> wall >> latent)) return 2;
            std::printf("byte=%02x\n", vs_encode(v, wall != 0, latent != 0));
        } else if (cmd == "decode") {
            unsigned b;
            int in_plane;
            if (!(std::cin >> std::hex >> b >> std::dec >> in_plane)) return 2;
            std::printf("value=%d\n", vs_decode(b, in_plane != 0));
        } else if (cmd == "cell") {
            int v, wall;
            if (!(std::cin >> v >> wall)) return 2;
            std::printf("ok=%d\n", (int)vs_cell_ok(v, wall != 0));
        } else if (cmd == "clamp") {
            long long st, bu;
            if (!(std::cin >> st >> bu)) return 2;
            std::printf("steps=%lld bumps=%lld\n", (long long)vs_clamp_steps(st), (long long)vs_clamp_bumps(bu));
        } else if (cmd == "agent") {
            if (const int rc = do_agent(std::cin)) return rc;
        } else {
            return 2;
        }
    }
    return 0;
}
