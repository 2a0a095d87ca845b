// test_box_class.cpp -- the exact-box classifier of csrc/env_plan.h
// (room_is_exact_box, rooms_box_exact: which envs may launch the step kernels
// that compute the ray record) on rooms whose class is known by construction.
// Stand-alone: its own main, built under g++ with AddressSanitizer and UBSan
// and run as a child process by tests/test_box_class_host.py.  Prints one line
// per case and exits 1 if any class is wrong.
//
// Every wall array is a heap block of exactly W * D * H bytes, so an index
// past a room is an AddressSanitizer report.
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "env_plan.h"

namespace {

struct TestRoom {
    int W, D, H;
    std::vector<uint8_t> wall;   // index (x * D + y) * H + z
    uint8_t &at(int x, int y, int z) { return wall[((size_t)x * D + y) * H + z]; }
};

// one wall layer around a free interior
TestRoom shell(int W, int D, int H) {
    TestRoom r{W, D, H, std::vector<uint8_t>((size_t)W * D * H, 0)};
    for (int x = 0; x < W; ++x)
        for (int y = 0; y < D; ++y)
            for (int z = 0; z < H; ++z)
                if (x == 0 || x == W - 1 || y == 0 || y == D - 1 || z == 0 || z == H - 1) r.at(x, y, z) = 2;
    return r;
}

// the room tables of a set, as vn_create builds them; false if it rejects the set
bool tables_of(const std::vector<TestRoom> &rooms, RoomTables *rt) {
    const size_t n = rooms.size();
    std::unique_ptr<int32_t[]> whd(new int32_t[3 * n]);
    size_t cells = 0;
    for (size_t r = 0; r < n; ++r) {
        whd[3 * r] = rooms[r].W;
        whd[3 * r + 1] = rooms[r].D;
        whd[3 * r + 2] = rooms[r].H;
        cells += rooms[r].wall.size();
    }
    std::unique_ptr<uint8_t[]> walls(new uint8_t[cells]);
    size_t o = 0;
    for (const TestRoom &r : rooms)
        for (uint8_t b : r.wall) walls[o++] = b;
    VnRoomSet rs = {(int32_t)n, whd.get(), walls.get(), nullptr, nullptr};
    VnConfig cfg = {};
    cfg.local_map_length = 4;
    return build_room_tables(rs, cfg, rt) == VN_OK;
}

int failures = 0;

void expect(const char *name, bool got, bool want) {
    std::printf("%-40s %s (want %s)%s\n", name, got ? "box" : "not a box", want ? "box" : "not a box",
                got == want ? "" : "   <-- WRONG");
    if (got != want) ++failures;
}

// a single room through both entry points: the room's own records, and the set of one
void expect_room(const char *name, const TestRoom &room, bool want) {
    RoomTables rt;
    if (!tables_of({room}, &rt)) {
        std::printf("%-40s rejected by build_room_tables: %s\n", name, vn_detail::g_last_error.c_str());
        ++failures;
        return;
    }
    expect(name, room_is_exact_box(room.W, room.D, room.H, rt.rays.data()), want);
    expect((std::string(name) + " (as a set)").c_str(), rooms_box_exact(rt), want);
}

}  // namespace

int main() {
    // exact boxes
    const int boxes[5][3] = {{3, 3, 3}, {4, 5, 3}, {8, 8, 4}, {32, 32, 8}, {64, 40, 8}};
    for (const auto &b : boxes) {
        char name[64];
        std::snprintf(name, sizeof(name), "box %dx%dx%d", b[0], b[1], b[2]);
        expect_room(name, shell(b[0], b[1], b[2]), true);
    }
    // the formula itself at one cell worked out by hand: 8x8x4, cell (2, 5, 1): runs +x 4, -x 1, +y 1, -y 4,
    // +z 1, -z 0, each ending at a wall
    {
        const RayRec f = box_ray_rec(8, 8, 4, 2, 5, 1);
        const bool ok = f.x == (0x84u | 0x81u << 8 | 0x81u << 16 | 0x84u << 24) && f.y == (0x81u | 0x80u << 8);
        std::printf("%-40s %08x %08x%s\n", "box_ray_rec(8,8,4; 2,5,1)", f.x, f.y, ok ? "" : "   <-- WRONG");
        if (!ok) ++failures;
    }

    // not boxes
    TestRoom pillar = shell(8, 8, 4);
    pillar.at(4, 3, 1) = pillar.at(4, 3, 2) = 2;            // one interior pillar, floor to ceiling
    expect_room("box 8x8x4 with a pillar", pillar, false);

    TestRoom open_top = shell(8, 8, 4);
    open_top.at(3, 3, 3) = 0;                               // a ceiling cell removed: a ray ends at the edge (bit 17)
    expect_room("box 8x8x4, one ceiling cell removed", open_top, false);

    TestRoom thick = shell(8, 8, 4);
    for (int y = 0; y < 8; ++y)
        for (int z = 0; z < 4; ++z) thick.at(1, y, z) = 2;  // a second wall layer on the -x face
    expect_room("box 8x8x4, second wall layer on -x", thick, false);

    {   // 2 x 5 x 5 has no interior (vn_create rejects it): the classifier's own size guard, on a table of
        // wall records only, which a comparison of free cells alone would accept
        std::unique_ptr<RayRec[]> rays(new RayRec[2 * 5 * 5]);
        for (int i = 0; i < 2 * 5 * 5; ++i) rays[i] = RayRec{0u, 1u << 16};
        expect("room 2x5x5", room_is_exact_box(2, 5, 5, rays.get()), false);
    }

    // sets, classed as an env
    {
        RoomTables rt;
        if (!tables_of({shell(8, 8, 4), pillar}, &rt)) ++failures;
        expect("set {box 8x8x4, pillar room}", rooms_box_exact(rt), false);
        RoomTables rt2;
        if (!tables_of({pillar, shell(8, 8, 4)}, &rt2)) ++failures;
        expect("set {pillar room, box 8x8x4}", rooms_box_exact(rt2), false);
        RoomTables rt3;
        if (!tables_of({shell(8, 8, 4), shell(5, 6, 3)}, &rt3)) ++failures;
        expect("set {box 8x8x4, box 5x6x3}", rooms_box_exact(rt3), true);
    }
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
