// route_check.cpp -- stand-alone host driver of csrc/env_route.h (the frontier
// planner's rule on bit rows), built by tests/test_route_host.py with g++ and
// the sanitizers.  It runs the code the planning kernel runs, as one thread.
//
// stdin, any number of:
//   plan W D H ph x y z f  v[0] ... v[W*D*H-1]     dense belief values, [x][y][z]
//       -> "plan action dist"
//   flood W D H ph y z  pass rows..., cur rows...  D*H hex words each, row (y', z') at y' * H + z'
//       -> "flood word"    one flood step of row (y, z)
//   moves  -> "moves" and the 6 x 4 moves as dx,dy,dz, action-major
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

int do_plan() {
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
    int action = -9, dist = -9;
    rt_search(HostBlk{}, pass.data(), ra.data(), rb.data(), g, x, y, z, f, nv, W * D * ph, 0, 1, &action, &dist);
    std::printf("plan %d %d\n", action, dist);
    return 0;
}

int do_flood() {
    int W, D, H, ph, y, z;
    if (!(std::cin >> W >> D >> H >> ph >> y >> z)) return 1;
    if (D < 1 || H < 1 || H > ph || y < 0 || y >= D || z < 0 || z >= H) return 1;
    std::vector<uint64_t> pass((size_t)D * ph, ~0ull), cur((size_t)D * ph, ~0ull);
    for (std::vector<uint64_t> *rows : {&pass, &cur})
        for (int cy = 0; cy < D; ++cy)
            for (int cz = 0; cz < H; ++cz) {
                std::string s;
                if (!(std::cin >> s)) return 1;
                (*rows)[(size_t)cy * ph + cz] = std::stoull(s, nullptr, 16);
            }
    const RtGeom g{W, D, H, ph};
    std::printf("flood %016llx\n", (unsigned long long)rt_flood_row(pass.data(), cur.data(), g, y, z));
    return 0;
}

}  // namespace

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        int rc = 1;
        if (cmd == "plan") rc = do_plan();
        else if (cmd == "flood") rc = do_flood();
        else if (cmd == "moves") {
            std::printf("moves");
            for (int k = 0; k < RT_ACTIONS; ++k)
                for (int f = 0; f < 4; ++f) {
                    int dx, dy, dz;
                    rt_move(k, f, &dx, &dy, &dz);
                    std::printf(" %d,%d,%d", dx, dy, dz);
                }
            std::printf("\n");
            rc = 0;
        }
        if (rc) {
            std::fprintf(stderr, "bad input at '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
