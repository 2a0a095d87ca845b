// agent_parts_check.cpp -- runs the per-agent plan of csrc/env_plan.h
// (agent_parts, snapshot_bytes: what the whole-env snapshots and the per-agent
// gather size their copies from) outside the library, under g++ and the host
// sanitizers (tests/test_agent_parts_host.py compiles and runs it).  Like
// env_plan_check.cpp it has no expectations of its own: it reads commands on
// stdin and prints what the header computes.
//
//   parts VARIANT L W D H PCACHE_CAP DEFER SIMPLE_LAYOUT N
#include <cstdio>
#include <iostream>
#include <string>

#include "env_plan.h"

int main() {
    constexpr VnTuning kAuto = {-1, -1, 0, 67, 1, 1, 1};
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd != "parts") return 2;
        int variant, L, W, D, H;
        long long n;
        VnTuning t = kAuto;
        if (!(std::cin >> variant >> L >> W >> D >> H >> t.pcache_cap >> t.defer >> t.simple_layout >> n) || n < 1)
            return 2;
        const EnvLayout l = plan_layout(variant, L, W, D, H, t);
        const AgentParts a = agent_parts(l);
        std::printf("parts hot=%u wrec=%u seed=%u belief=%u goal=%u predraw=%u stood=%u pnz=%u episode=%u copied=%u "
                    "agent_bytes=%u ph=%d pcache=%d snapshot_bytes=%zu\n",
                    a.hot, a.wrec, a.seed, a.belief, a.goal, a.predraw, a.stood, a.pnz, a.episode, a.copied(),
                    l.agent_bytes, l.ph, l.pcache, snapshot_bytes(a, (size_t)n));
    }
    return 0;
}
