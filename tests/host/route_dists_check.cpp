// route_dists_check.cpp -- stand-alone host driver of csrc/env_route.h's search for all six
// actions (rt_search_all, rt_best_set, rt_min_dist: vn_plan_frontier_dists' rule on bit rows),
// built by tests/test_route_dists_host.py with g++ and the sanitizers.  It runs the code the
// planning kernel runs, as one thread.
//
// stdin, any number of:
//   dists W D H ph x y z f  v[0] ... v[W*D*H-1]     dense belief values, [x][y][z]
//       -> "dists d0 d1 d2 d3 d4 d5 best action dist"   (action / dist as the kernel derives them)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "env_route.h"

namespace {

struct HostBlk {   // one thread: the barrier is nothing, the vote is the thread's own
    void sync() const {}
    bool any(bool v) const { return v; }
};

int do_dists() {
    int W, D, H, ph, x, y, z, f;
    if (!(std::cin >> W >> D >> H >> ph >> x >> y >> z >> f)) return 1;
    if (W < 1 || W > RT_MAX_W || D < 1 || H < 1 || H > ph) return 1;
    std::vector<int> v((size_t)W * D * H);
    for (int &c : v)
        if (!(std::cin >> c)) return 1;
    const RtGeom g{W, D, H, ph};
    if (!rt_inside(g, x, y, z) || f < 0 || f > 3) return 1;
    // rows of the padded stride; what lies outside the room stays poisoned so a read of it shows
    std::vector<uint64_t> pass((size_t)D * ph, ~0ull), ra((size_t)D * ph, ~0ull), rb((size_t)D * ph, ~0ull);
    for (int cy = 0; cy < D; ++cy)
        for (int cz = 0; cz < H; ++cz) {
            uint64_t p = 0, t = 0;
            for (int cx = 0; cx < W; ++cx) {
                const int c = v[((size_t)cx * D + cy) * H + cz];
                p |= (uint64_t)(c >= 0) << cx;
                t |= (uint64_t)(c == 0) << cx;
            }
            pass[(size_t)cy * ph + cz] = p & rt_width_mask(W);
            ra[(size_t)cy * ph + cz] = t;
        }
    int nv[RT_ACTIONS];
    for (int k = 0; k < RT_ACTIONS; ++k) {
        int dx, dy, dz;
        rt_move(k, f, &dx, &dy, &dz);
        const int nx = x + dx, ny = y + dy, nz = z + dz;
        nv[k] = rt_inside(g, nx, ny, nz) ? v[((size_t)nx * D + ny) * H + nz] : -3;
    }
    int ds[RT_ACTIONS] = {-9, -9, -9, -9, -9, -9};
    rt_search_all(HostBlk{}, pass.data(), ra.data(), rb.data(), g, x, y, z, f, nv, W * D * ph, 0, 1, ds);
    const uint32_t best = rt_best_set(ds);
    std::printf("dists %d %d %d %d %d %d %u %d %d\n", ds[0], ds[1], ds[2], ds[3], ds[4], ds[5], best,
                best ? rt_lowest(best) : rt_fallback(nv), rt_min_dist(ds));
    return 0;
}

}  // namespace

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd != "dists" || do_dists()) {
            std::fprintf(stderr, "bad input at '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
