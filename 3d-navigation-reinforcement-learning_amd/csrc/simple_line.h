// simple_line.h -- simpleEnv, line layout: S as 32-B lines, moved by lane pairs.
// Included by voxnav_simple.hip only.
#pragma once

#include "env_core.h"

namespace {

// ============================================================================
// simpleEnv, line layout (the default for rooms up to 32 x 32 x 8, e.g. the
// bench's 32x32x8 box).  Same belief as the bit-plane layout -- S (cells
// stood on) and Q (edge-quirk marks), every other internal_grid value derived
// -- but S is kept as LINES: SX[y] = 8 u32 words over z (bit x), SY[x] = 8 u32
// words over z (bit y), 32 B each; a column's z bits (the up / down rays) are
// bit x of the SX[y] line, so there is no third copy.  The stepping lane keeps
// the two lines through its cell in LDS: a move along x replaces the SY line,
// along y the SX line, along z neither; the line left is stored back if it
// was marked.
// Why (rocprofv3, round 3): the simpleEnv step is bound by the CUs' 64-B
// request rate -- the address unit is busy 87-95 % of the kernel, at 5.7
// requests per env-step, 1.1 of them the evicted S words of the word layout
// (each move replaced 2-3 words; without those stores the kernel ran 1.4x).
// A lane's 32-B line access is 2 x 16 B; lane pairs split it so that both
// halves of one line go out in ONE instruction (a request per line, not per
// half): instruction 1 moves the even lane's line, instruction 2 the odd
// lane's, and the halves are swapped across the pair with one DPP move.
// Every line load / store is issued every step (an out-of-range buffer offset
// when a lane has none: no request, and the same vmcnt count on every path).
// LDS per lane: the X and Y line (12-word stride: 16-B aligned rows).
// QZ (edge-quirk marks) as in the bit-plane layout.
// ============================================================================
constexpr int SL_STRIDE = 12;   // words per LDS line slot
constexpr uint32_t SL_OFF = 0x80000000u;   // out-of-range buffer offset: dropped
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

struct SLine {
    u32x4_t h0, h1;   // words 0-3, 4-7
};

__device__ __forceinline__ uint32_t dpp_swap_pair(uint32_t v) {   // lane i <- lane i ^ 1
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
}
__device__ __forceinline__ u32x4_t dpp_swap_pair4(u32x4_t v) {
    u32x4_t r;
    r.x = dpp_swap_pair(v.x);
    r.y = dpp_swap_pair(v.y);
    r.z = dpp_swap_pair(v.z);
    r.w = dpp_swap_pair(v.w);
    return r;
}

// lane-pair line load: each lane gets the line at its byte offset `off`
// (SL_OFF: none, zeros).  Issue and finish (the swap across the pair, which
// needs the data) are split so the loads stay in flight across a step.  Both
// must run with the whole wave active.
__device__ __forceinline__ SLine sl_pair_issue(__amdgpu_buffer_rsrc_t rs, uint32_t off, bool odd) {
    const uint32_t off_p = dpp_swap_pair(off);
    const uint32_t ae = odd ? off_p : off, ao = odd ? off : off_p;     // the pair's even / odd line
    const uint32_t half = odd ? 16u : 0u;
    SLine r;   // even: h0 = own h0, h1 = partner's h0; odd: h0 = partner's h1, h1 = own h1
    r.h0 = __builtin_amdgcn_raw_buffer_load_b128(rs, ae == SL_OFF ? SL_OFF : ae + half, 0, 0);
    r.h1 = __builtin_amdgcn_raw_buffer_load_b128(rs, ao == SL_OFF ? SL_OFF : ao + half, 0, 0);
    return r;
}
__device__ __forceinline__ SLine sl_pair_finish(const SLine &r, bool odd) {
    const u32x4_t sw = dpp_swap_pair4(odd ? r.h0 : r.h1);
    SLine l;
    l.h0 = odd ? sw : r.h0;
    l.h1 = odd ? r.h1 : sw;
    return l;
}
__device__ __forceinline__ SLine sl_pair_load(__amdgpu_buffer_rsrc_t rs, uint32_t off, bool odd) {
    return sl_pair_finish(sl_pair_issue(rs, off, odd), odd);
}

// lane-pair line store of each lane's line `l` at `off` (SL_OFF: none)
__device__ __forceinline__ void sl_pair_store(__amdgpu_buffer_rsrc_t rs, uint32_t off, const SLine &l, bool odd) {
    const uint32_t off_p = dpp_swap_pair(off);
    const uint32_t ae = odd ? off_p : off, ao = odd ? off : off_p;
    const uint32_t half = odd ? 16u : 0u;
    const u32x4_t sw = dpp_swap_pair4(odd ? l.h0 : l.h1);   // even gets the odd lane's h0, odd the even's h1
    __builtin_amdgcn_raw_buffer_store_b128(odd ? sw : l.h0, rs, ae == SL_OFF ? SL_OFF : ae + half, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(odd ? l.h1 : sw, rs, ao == SL_OFF ? SL_OFF : ao + half, 0, 0);
}

__device__ __forceinline__ void sl_lds_put(uint32_t *slot, const SLine &l) {
    reinterpret_cast<u32x4_t *>(slot)[0] = l.h0;
    reinterpret_cast<u32x4_t *>(slot)[1] = l.h1;
}
__device__ __forceinline__ SLine sl_lds_get(const uint32_t *slot) {
    SLine l;
    l.h0 = reinterpret_cast<const u32x4_t *>(slot)[0];
    l.h1 = reinterpret_cast<const u32x4_t *>(slot)[1];
    return l;
}
// bit z = bit b of word z (the column's S bits from the SX line)
__device__ __forceinline__ uint32_t sl_column(const SLine &l, int b) {
    const uint32_t w[8] = {l.h0.x, l.h0.y, l.h0.z, l.h0.w, l.h1.x, l.h1.y, l.h1.z, l.h1.w};
    uint32_t c = 0;
#pragma unroll
    for (int z = 0; z < 8; ++z) c |= ((w[z] >> b) & 1u) << z;
    return c;
}

}  // namespace
