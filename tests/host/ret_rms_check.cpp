// ret_rms_check.cpp -- stand-alone host driver of csrc/ret_rms.h (the reward
// normalisation's arithmetic), built by tests/test_reward_norm_host.py with
// g++ and the sanitizers.  It runs the functions the kernels run, as one thread.
//
// stdin, any number of cases; every float travels as its bit pattern in hex:
//   run T N t0 t1 training gamma eps clip mean var count  S s[0] .. s[S-1]
//       ret[N] (f64)  rewards[T*N] (f32)  dones[T*N] (0 / 1)
//   S shards of s[k] agents (their sum N, all but the last multiples of 64):
//   each shard's chunk triples are computed on its own slice and concatenated.
//   -> "rms m v c", "ret ...", "scales ..." (t1 - t0 of them), "rew ..." (T*N)
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "ret_rms.h"

namespace {

bool get64(double *v) {
    std::string w;
    if (!(std::cin >> w)) return false;
    const uint64_t b = std::stoull(w, nullptr, 16);
    std::memcpy(v, &b, 8);
    return true;
}

bool get32(float *v) {
    std::string w;
    if (!(std::cin >> w)) return false;
    const uint32_t b = (uint32_t)std::stoul(w, nullptr, 16);
    std::memcpy(v, &b, 4);
    return true;
}

void put64(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    std::printf(" %016" PRIx64, b);
}

void put32(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    std::printf(" %08" PRIx32, b);
}

int do_run() {
    int T, N, t0, t1, training, S;
    double gamma, eps, clip;
    RrStats st;
    if (!(std::cin >> T >> N >> t0 >> t1 >> training)) return 1;
    if (!get64(&gamma) || !get64(&eps) || !get64(&clip) || !get64(&st.mean) || !get64(&st.var) || !get64(&st.count))
        return 1;
    if (!(std::cin >> S) || T < 1 || N < 1 || t0 < 0 || t1 <= t0 || t1 > T || S < 1) return 1;
    std::vector<int> shard(S);
    int sum = 0;
    for (int k = 0; k < S; ++k) {
        if (!(std::cin >> shard[k]) || shard[k] < 1 || (k + 1 < S && shard[k] % RR_CHUNK)) return 1;
        sum += shard[k];
    }
    if (sum != N) return 1;
    std::vector<double> ret(N);
    std::vector<float> rew((size_t)T * N);
    std::vector<int> done((size_t)T * N);
    for (double &v : ret)
        if (!get64(&v)) return 1;
    for (float &v : rew)
        if (!get32(&v)) return 1;
    for (int &v : done)
        if (!(std::cin >> v)) return 1;
    std::vector<double> scales;
    std::vector<RrTriple> nodes;
    for (int t = t0; t < t1; ++t) {
        float *r = rew.data() + (size_t)t * N;
        if (training) {
            for (int i = 0; i < N; ++i) ret[i] = rr_return(ret[i], gamma, r[i]);
            nodes.clear();
            int base = 0;
            for (int k = 0; k < S; ++k) {
                for (int c = 0; c < shard[k]; c += RR_CHUNK) {
                    const int m = shard[k] - c < RR_CHUNK ? shard[k] - c : RR_CHUNK;
                    nodes.push_back(rr_chunk(ret.data() + base + c, m));
                }
                base += shard[k];
            }
            rr_update(st, rr_tree(nodes.data(), (int)nodes.size()));
        }
        const double sc = rr_scale(st.var, eps);
        scales.push_back(sc);
        for (int i = 0; i < N; ++i) r[i] = rr_normalize(r[i], sc, clip);
        if (training)
            for (int i = 0; i < N; ++i)
                if (done[(size_t)t * N + i] != 0) ret[i] = 0.0;
    }
    std::printf("rms");
    put64(st.mean), put64(st.var), put64(st.count);
    std::printf("\nret");
    for (double v : ret) put64(v);
    std::printf("\nscales");
    for (double v : scales) put64(v);
    std::printf("\nrew");
    for (float v : rew) put32(v);
    std::printf("\n");
    return 0;
}

}  // namespace

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd != "run" || do_run() != 0) {
            std::fprintf(stderr, "bad input at '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
