// env_plan_check.cpp -- runs csrc/env_plan.h (the host arithmetic of
// vn_create) outside the library, under g++ and the host sanitizers
// (tests/test_env_plan.py compiles and runs it).  It has no expectations of
// its own: it reads commands on stdin and prints what the header computes.
//
//   layout VARIANT L W D H PCACHE_CAP DEFER SIMPLE_LAYOUT
//   lut L
//   rooms FINISH N HAS_START HAS_GOAL, then N lines  W D H sx sy sz gx gy gz WALLS
//        (WALLS: W*D*H characters '0' / '1', index (x*D+y)*H+z)
//
// Every input array is a heap block of exactly the size the ABI documents, so
// an index past a caller's array is an AddressSanitizer report.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>

#include "env_plan.h"

namespace {

constexpr VnTuning kAuto = {-1, -1, 0, 67, 1, 1, 1};

void print_layout(const EnvLayout &l) {
    std::printf("layout variant=%d obs_dim=%d pw=%d pd=%d ph=%d nbx=%d nby=%d map_bytes=%u agent_bytes=%u "
                "plane_bytes=%u nwx=%d nwy=%d xp_off=%u yp_off=%u sy_off=%u sz_off=%u qz_off=%u sbits=%d sline=%d "
                "defer=%d pcache=%d\n",
                l.variant, l.obs_dim, l.pw, l.pd, l.ph, l.nbx, l.nby, l.map_bytes, l.agent_bytes, l.plane_bytes, l.nwx,
                l.nwy, l.xp_off, l.yp_off, l.sy_off, l.sz_off, l.qz_off, l.sbits, l.sline, l.defer, l.pcache);
}

template <typename T>
std::unique_ptr<T[]> exact(size_t n) {   // no slack behind the last element
    return std::unique_ptr<T[]>(new T[n]);
}

int do_rooms(std::istream &in) {
    double finish;
    int n, has_start, has_goal;
    if (!(in >> finish >> n >> has_start >> has_goal) || n < 1) return 2;
    auto whd = exact<int32_t>(3 * (size_t)n), fs = exact<int32_t>(3 * (size_t)n), gl = exact<int32_t>(3 * (size_t)n);
    std::string all;
    for (int r = 0; r < n; ++r) {
        std::string w;
        for (int k = 0; k < 3; ++k) in >> whd[3 * r + k];
        for (int k = 0; k < 3; ++k) in >> fs[3 * r + k];
        for (int k = 0; k < 3; ++k) in >> gl[3 * r + k];
        if (!(in >> w)) return 2;
        all += w;
    }
    auto walls = exact<uint8_t>(all.size());
    for (size_t i = 0; i < all.size(); ++i) walls[i] = all[i] == '1' ? 2 : 0;   // the file's wall value
    VnRoomSet rs = {n, whd.get(), walls.get(), has_start ? fs.get() : nullptr, has_goal ? gl.get() : nullptr};
    VnConfig cfg = {};
    cfg.local_map_length = 4;
    cfg.finish_percentage = finish;
    RoomTables rt;
    const int rc = build_room_tables(rs, cfg, &rt);
    std::printf("rc=%d\n", rc);
    if (rc) {
        std::printf("msg=%s\n", vn_detail::g_last_error.c_str());
        return 0;
    }
    std::printf("max=%d %d %d\n", rt.maxW, rt.maxD, rt.maxH);
    std::printf("total_free=");
    for (uint32_t v : rt.total_free) std::printf("%u ", v);
    std::printf("\ndesc=");
    for (uint32_t v : rt.desc) std::printf("%08x ", v);
    std::printf("\nstarts=");
    for (uint32_t v : rt.starts) std::printf("%06x ", v);
    std::printf("\nrays=");
    for (const RayRec &v : rt.rays) std::printf("%08x:%08x ", v.x, v.y);
    // the latent-wall images of the CubicEnv layout these rooms get
    const EnvLayout l = plan_layout(VN_VARIANT_CUBIC, 4, rt.maxW, rt.maxD, rt.maxH, kAuto);
    std::vector<int8_t> img;
    wall_image(rs, l, &img);
    std::printf("\nwimg_geom=%d %d %u %d\nwimg_size=%zu\nwimg_nz=", l.nby, l.ph, l.map_bytes, VN_WIMG_REP, img.size());
    for (size_t i = 0; i < img.size(); ++i)
        if (img[i]) std::printf("%zu:%d ", i, (int)img[i]);
    std::printf("\n");
    return 0;
}

}  // namespace

int main() {
    static_assert(sizeof(RayRec) == 8, "ray records are uploaded as uint2");
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "layout") {
            int variant, L, W, D, H;
            VnTuning t = kAuto;
            if (!(std::cin >> variant >> L >> W >> D >> H >> t.pcache_cap >> t.defer >> t.simple_layout)) return 2;
            print_layout(plan_layout(variant, L, W, D, H, t));
        } else if (cmd == "lut") {
            int L;
            if (!(std::cin >> L)) return 2;
            auto lut = exact<float>(TAB_ALL);
            fill_lut(L, lut.get());
            std::printf("lut=");
            for (int k = 0; k < TAB_ALL; ++k) {
                uint32_t u;
                std::memcpy(&u, &lut[k], 4);
                std::printf("%08x ", u);
            }
            std::printf("\ntab=%d %d %d %d %d %d %u %u %u %u\n", TAB_ACTION, TAB_CID, TAB_SIZE, TAB_SREW, TAB_SREW64,
                        TAB_ALL, TC_ZERO, TC_ONE, TC_ACT, TC_CID);
        } else if (cmd == "rooms") {
            if (const int rc = do_rooms(std::cin)) return rc;
        } else {
            return 2;
        }
    }
    return 0;
}
