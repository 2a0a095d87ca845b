// ret_rms.h -- the arithmetic of the return-based reward normalisation
// (vn_return_moments / vn_reward_normalize; the rule is stated once, in
// include/voxnav.h): the discounted-return step, a chunk's moments by the
// 64-lane xor butterfly, the merge of two (n, mean, M2) triples, the binary
// tree over the chunks, the running statistics' update and the scaled,
// clipped reward.  Plain C++17 with no HIP include (like env_route.h): every
// function is VN_HD, so the kernels (voxnav_rnorm.hip) and the stand-alone
// host driver (tests/host/ret_rms_check.cpp, under the sanitizers) run the
// same code.  The kernels spread the tree levels across a block's threads;
// rr_tree is that loop as one thread does it, the same pairs in the same
// order.  Each line is one IEEE f64 operation per operator as written: build
// without contraction (-ffp-contract=off).  Anonymous namespace: one copy per unit.
#pragma once

#include <cmath>
#include <cstdint>

// host + device under hipcc, plain inline elsewhere (the definition of env_plan.h, token for token)
#ifdef __HIPCC__
#define VN_HD __host__ __device__ __forceinline__
#else
#define VN_HD inline
#endif

namespace {

constexpr int RR_CHUNK = 64;       // agents per chunk: one wave

struct RrTriple {                  // count, mean and sum of squared deviations of a set of returns
    double n, mean, m2;
};

struct RrStats {                   // RunningMeanStd: rms[3] of vn_reward_normalize, in this order
    double mean, var, count;
};

// step 1: the discounted return after a step with raw reward r
VN_HD double rr_return(double ret, double gamma, float r) { return ret * gamma + (double)r; }

VN_HD RrTriple rr_merge(const RrTriple &a, const RrTriple &b) {
    RrTriple o;
    o.n = a.n + b.n;
    const double d = b.mean - a.mean;
    o.mean = a.mean + (d * b.n) / o.n;
    o.m2 = (a.m2 + b.m2) + (((d * d) * a.n) * b.n) / o.n;
    return o;
}

// The xor butterfly over 64 lanes, v_j += v_{j xor s} for s = 1, 2, 4, ..., 32, leaves in every lane
// the sum over the balanced binary tree of adjacent pairs (lane j's partner at stage s holds the
// sibling subtree's sum, and f64 addition commutes): ((v0 + v1) + (v2 + v3)) + ...  That tree, over
// leaf(j) for j in [LO, LO + CNT), unrolled at compile time.
template <int LO, int CNT, class Leaf>
VN_HD double rr_pair_tree(const Leaf &leaf) {
    if constexpr (CNT == 1) {
        return leaf(LO);
    } else {
        const double l = rr_pair_tree<LO, CNT / 2>(leaf);
        const double r = rr_pair_tree<LO + CNT / 2, CNT / 2>(leaf);
        return l + r;
    }
}

// step 2, one chunk: the triple of its m present returns v[0 .. m); absent lanes hold +0.0 in both sums
VN_HD RrTriple rr_chunk(const double *v, int m) {
    RrTriple o;
    o.n = (double)m;
    o.mean = rr_pair_tree<0, RR_CHUNK>([&](int j) { return j < m ? v[j] : 0.0; }) / o.n;
    const double mean = o.mean;
    o.m2 = rr_pair_tree<0, RR_CHUNK>([&](int j) {
        const double d = j < m ? v[j] - mean : 0.0;
        return d * d;
    });
    return o;
}

// step 2, the tree over `count` >= 1 chunk triples, in place; the root is returned
VN_HD RrTriple rr_tree(RrTriple *node, int count) {
    while (count > 1) {
        const int half = (count + 1) >> 1;
        for (int j = 0; j < half; ++j)
            node[j] = 2 * j + 1 < count ? rr_merge(node[2 * j], node[2 * j + 1]) : node[2 * j];
        count = half;
    }
    return node[0];
}

// step 3, the part that does not depend on the running statistics: the batch as SB3 hands it to
// update_from_moments, b = (n_B, mean_B, var_B * n_B), from the tree's root
VN_HD RrTriple rr_batch(const RrTriple &root) {
    const double var_b = root.m2 / root.n;
    const RrTriple b = {root.n, root.mean, var_b * root.n};
    return b;
}

// step 3, the chain: the running statistics take the batch b
VN_HD void rr_absorb(RrStats &s, const RrTriple &b) {
    const RrTriple a = {s.count, s.mean, s.var * s.count};
    const RrTriple o = rr_merge(a, b);
    s.mean = o.mean;
    s.var = o.m2 / o.n;
    s.count = o.n;
}

VN_HD void rr_update(RrStats &s, const RrTriple &root) { rr_absorb(s, rr_batch(root)); }

VN_HD double rr_scale(double var, double epsilon) { return sqrt(var + epsilon); }

// step 4
VN_HD float rr_normalize(float r, double scale, double clip) {
    const double x = (double)r / scale;
    return (float)(x < -clip ? -clip : (x > clip ? clip : x));
}

}  // namespace
