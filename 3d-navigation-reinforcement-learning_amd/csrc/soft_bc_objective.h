// soft_bc_objective.h -- the distance-weighted behaviour-cloning objective
// BcSoft (head_loss.h: what an objective supplies) on BcCommon
// (bc_objective.h), and its labelled count.  voxnav_soft_bc_loss.hip states the
// rule; vn_bc_loss_soft[_masked] (there) and vn_ppo_bc_loss_soft[_masked]
// (voxnav_soft_ppo_bc_loss.hip) use it, the masked forms through BcMasked<>
// (masked_bc_objective.h) and PpoBcMasked<> (masked_ppo_bc_objective.h).
// Unit-local (an anonymous namespace): each unit instantiates its own kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bc_objective.h"
#include "head_loss.h"

namespace {

// bc_count_kernel for distance rows: a sample counts when one of its A
// distances is positive and its weight, if any, is nonzero.
__global__ __launch_bounds__(256) void bc_soft_count_kernel(const int32_t *__restrict__ dists, int64_t ldd,
                                                            const uint8_t *__restrict__ wgt,
                                                            const int64_t *__restrict__ src, int M, int A,
                                                            int64_t *__restrict__ cnt) {
    __shared__ int s[256];
    const int t = threadIdx.x;
    const int per = (M + kCntBlocks - 1) / kCntBlocks;
    const int i0 = blockIdx.x * per, i1 = min(M, i0 + per);
    int c = 0;
    for (int i = i0 + t; i < i1; i += 256) {
        const int64_t r = src ? src[i] : i;
        bool any = false;
        for (int k = 0; k < A; ++k) any = any || dists[r * ldd + k] > 0;
        c += (any && (wgt == nullptr || wgt[r] != 0)) ? 1 : 0;
    }
    s[t] = c;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) s[t] += s[t + h];
        __syncthreads();
    }
    if (t == 0) cnt[blockIdx.x] = s[0];
}

// vn_bc_loss_soft: the planner's distance through every first action per
// sample; the target is q_k = w_k / sum w over P = {k : d_k > 0}, w_k = 1 at the
// shortest distance and expf(-(d_k - d*) / tau) elsewhere, and the loss is
// KL(q || pi).  A sample with an empty P is unlabelled.
struct BcSoft : BcCommon {
    const int32_t *dists;       // [rows][ldd], the first A of a row
    int64_t ldd;
    float tau;
    struct Sample {
        int d[head_loss::kMaxA];     // the distances (-2 at and above A)
        uint32_t P, best;       // bits of the positive distances; policy(): of those with delta = 0
        bool has;
        float kl, gce;          // policy(): KL(q || pi), the gradient scale
        float q[head_loss::kMaxA];   // policy(): the target distribution
    };
    __device__ __forceinline__ Sample gather(const Block &, int64_t r, int A) const {
        Sample s;
        const int32_t *row = dists + r * ldd;
        s.P = 0u;
#pragma unroll
        for (int k = 0; k < head_loss::kMaxA; ++k) {
            s.d[k] = k < A ? row[k] : -2;
            s.P |= s.d[k] > 0 ? 1u << k : 0u;
        }
        s.has = wgt ? wgt[r] != 0 : true;
        s.has = s.has && s.P != 0u;
        return s;
    }
    template <int AM>
    __device__ __forceinline__ void policy(const Block &b, Sample &s, const head_loss::Forward<AM> &f, bool ok, float,
                                           float) const {
        int dmin = INT32_MAX;
#pragma unroll
        for (int a = 0; a < AM; ++a) dmin = ((s.P >> a) & 1u) ? min(dmin, s.d[a]) : dmin;
        // e_a = -delta_a / tau (tau tiny: -inf, w = 0; tau huge: -0, w = 1)
        float e[AM], sw = 0.0f;
        s.best = 0u;
#pragma unroll
        for (int a = 0; a < AM; ++a) {
            const bool in = (s.P >> a) & 1u;
            const int delta = in ? s.d[a] - dmin : 0;
            e[a] = -(float)delta / tau;
            s.q[a] = in ? (delta == 0 ? 1.0f : expf(e[a])) : 0.0f;
            s.best |= (in && delta == 0) ? 1u << a : 0u;
            sw += s.q[a];
        }
        const float inv_s = s.P != 0u ? 1.0f / sw : 0.0f;
        const float lsw = logf(sw);
        s.kl = 0.0f;
#pragma unroll
        for (int a = 0; a < AM; ++a) {
            s.q[a] *= inv_s;
            // a term whose q is 0 is 0 (its ln q may be -inf)
            s.kl += s.q[a] > 0.0f ? s.q[a] * ((e[a] - lsw) - f.lpa[a]) : 0.0f;
        }
        s.gce = (s.has && ok) ? b.inv_l : 0.0f;
    }
    template <int AM>
    __device__ __forceinline__ float dz(const Sample &s, const head_loss::Forward<AM> &f, int a) const {
        return s.gce * (f.p[a] - s.q[a]);
    }
    template <int AM>
    __device__ __forceinline__ void stats(const Sample &s, const head_loss::Forward<AM> &f, double *st) const {
        st[0] += s.has ? (double)s.kl : 0.0;
        st[3] += (s.has && ((s.best >> f.amax) & 1u) != 0u) ? 1.0 : 0.0;
    }
};

// L_i of the masked forms (masked_bc_objective.h): every action the target gives mass to
__device__ __forceinline__ unsigned label_bits(const BcSoft::Sample &s, int) { return s.has ? s.P : 0u; }

// what the four soft entries refuse beyond their namesakes' refusals and a NULL dists
inline int check_soft_args(int64_t ldd, int32_t A, float tau) {
    if (ldd < A) return vn_detail::fail(VN_ERR_INVALID, "distance row stride %lld < A", (long long)ldd);
    if (!(std::isfinite(tau) && tau > 0.0f))
        return vn_detail::fail(VN_ERR_INVALID, "tau %g: finite and > 0", (double)tau);
    return VN_OK;
}

}  // namespace
