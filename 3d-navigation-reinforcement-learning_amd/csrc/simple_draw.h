// simple_draw.h -- simpleEnv: the MT19937 draws of an episode (room, start, goal).
// Included by voxnav_simple.hip only.
#pragma once

#include "env_core.h"

namespace {

// The first MT_W = 24 outputs of random.seed(seed) in ONE pass of the two
// init_by_array chains (mt_outputs captures 8 per pass; a wave-wide draw of
// 64 lanes would otherwise re-run the chains whenever any lane's rejection
// sampling passed 8 outputs), written to the lane's LDS row (stride MT_WS).
constexpr int MT_W = 24, MT_WS = 25;
__device__ __noinline__ void mt_outputs_wide(uint32_t seed, uint32_t *lds_row) {
    uint32_t p = mix1(c_mt_g[1], c_mt_g[0], seed);
    const uint32_t m1_1 = p;
    p = mt_loop1(p, seed);
    const uint32_t m1b1 = mix1(m1_1, p, seed);   // wrap: i = 1 again, mt[0] = mt[623]
    uint32_t p1 = m1_1, q = m1b1;
    uint32_t lo[MT_W + 1], hi[MT_W];             // F[0 .. MT_W], F[397 .. 397 + MT_W - 1]
#pragma unroll
    for (int i = 2; i <= MT_W; ++i) {
        p1 = mix1(c_mt_g[i], p1, seed);
        q = mix2(p1, q, (uint32_t)i);
        lo[i] = q;
    }
    mt_loop2(p1, q, MT_W + 1, 397, seed);
#pragma unroll
    for (int k = 0; k < MT_W; ++k) {
        const int i = 397 + k;
        p1 = mix1(c_mt_g[i], p1, seed);
        q = mix2(p1, q, (uint32_t)i);
        hi[k] = q;
    }
    mt_loop2(p1, q, 397 + MT_W, MT_N, seed);
    lo[1] = mix2(m1b1, q, 1u);                   // F[1]: loop 2's wrap step
    lo[0] = 0x80000000u;                         // F[0]
#pragma unroll
    for (int j = 0; j < MT_W; ++j) {
        const uint32_t y = (lo[j] & 0x80000000u) | (lo[j + 1] & 0x7fffffffu);
        lds_row[j] = mt_temper(hi[j] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u));
    }
}

// MT output stream over a lane's LDS row of MT_W outputs (mt_outputs_wide),
// blocks past it recomputed one at a time (mt_refill)
struct MtLdsStream {
    const uint32_t *row;
    uint32_t seed;
    int used;
    int32_t *err;
    MtBlock ext;
    __device__ uint32_t next() {
        uint32_t r;
        if (used < MT_W) {
            r = row[used];
        } else {
            if ((used % MT_C) == 0) ext = mt_refill(seed, used, err);
            const int j = used % MT_C;
            r = ext.w[0];
#pragma unroll
            for (int t = 1; t < MT_C; ++t) r = j == t ? ext.w[t] : r;
        }
        ++used;
        return r;
    }
    __device__ uint32_t below(uint32_t n) {
        const int k = 32 - __clz(n);
        uint32_t r = next() >> (32 - k);
        while (r >= n) r = next() >> (32 - k);
        return r;
    }
};

// MT draws of simpleEnv's load_room (:350, :410-426): room, start (drawn if
// absent or on a wall), goal (drawn if absent or on a wall).  Returns
// (start | room<<24, goal).
template <typename MT>
__device__ __attribute__((always_inline)) inline uint2 simple_draw_from(const EnvConst *ec, MT &mt) {
    const int room = ec->use_room_draw ? (int)mt.below((uint32_t)ec->n_rooms) : 0;
    const Room R = load_room_c(ec, room);
    auto is_wall = [&](uint32_t c) {
        const int x = c & 0xff, y = (c >> 8) & 0xff, z = (c >> 16) & 0xff;
        return ((ec->rays[R.ray_off + (uint32_t)((x * R.D + y) * R.H + z)].y >> 16) & 1u) != 0u;
    };
    uint32_t s = R.fixed_start >= 0 ? (uint32_t)R.fixed_start : ec->starts[R.start_off + mt.below(R.total_free)];
    if (is_wall(s)) s = ec->starts[R.start_off + mt.below(R.total_free)];
    uint32_t gl = R.fixed_goal >= 0 ? (uint32_t)R.fixed_goal : ec->starts[R.start_off + mt.below(R.total_free)];
    if (is_wall(gl)) gl = ec->starts[R.start_off + mt.below(R.total_free)];
    return make_uint2((s & 0xffffffu) | ((uint32_t)room << 24), gl & 0xffffffu);
}

__device__ __noinline__ uint2 simple_draw(const EnvConst *ec, uint32_t seed) {
    MtStream mt;
    mt.seed = seed;
    mt.used = 0;
    mt.err = ec->err;
    mt_first_outputs(seed, mt.buf);
    return simple_draw_from(ec, mt);
}

// reset of the lanes with `need` for simple_pipe_kernel: as sb_reset_wave,
// but the MT19937 draw (a ~1.2k-step serial chain, ~15 us) is shared.  A
// lane's draw for its next episode seed is kept in nd = {start | room << 24,
// goal, seed, valid}.  A resetting lane whose nd is for its seed uses it; when
// any resetting lane has none, the wave runs the chain once for EVERY live
// lane (same instructions, so the same time as for one lane): the resetting
// lanes take their draw and the others keep theirs for their next reset.
// Measured: the chain was half of the kernel's time (resets ablated: 2x).
__device__ __forceinline__ uint2 sp_reset_draw(const Params &p, bool need, bool live, uint32_t seed, int lane, uint4 &nd,
                                               uint32_t *mt_lds) {
    const bool have = need && nd.w == 1u && nd.z == seed;
    uint2 drawn = have ? make_uint2(nd.x, nd.y) : make_uint2(0u, 0u);
    if (need) nd.w = 0u;                                   // consumed: the next episode has another seed
    if (__ballot(need && !have)) {
        // one chain pass for the wave: a resetting lane without a draw computes
        // this episode's; one with a draw the episode after it (seed + stride);
        // the others their next episode's if they have none
        const uint32_t s2 = (need && have) ? seed + p.seed_stride : seed;
        mt_outputs_wide(s2, mt_lds + lane * MT_WS);
        MtLdsStream mt;
        mt.row = mt_lds + lane * MT_WS;
        mt.seed = s2;
        mt.used = 0;
        mt.err = p.envc->err;
        const uint2 d2 = live ? simple_draw_from(p.envc, mt) : make_uint2(0u, 0u);
        if (need && !have) drawn = d2;
        else if (live) nd = make_uint4(d2.x, d2.y, s2, 1u);
    }
    return drawn;
}

}  // namespace
