// ppo_objective.h -- what is PPO's of the head loss (head_loss.h: what an
// objective supplies): the advantage sums of the minibatch and the
// clipped-surrogate objective PpoClip.  voxnav_ppo_loss.hip states the formula;
// vn_ppo_loss (there) and vn_ppo_bc_loss (voxnav_ppo_bc_loss.hip) use them.
// Unit-local (an anonymous namespace): each unit instantiates its own kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "head_loss.h"

namespace {

constexpr int kAdvBlocks = 64; // blocks of the advantage sums

// per-block f64 sums of the minibatch's advantages and their squares
// (kAdvBlocks blocks, a contiguous range each); every loss block adds the
// kAdvBlocks pairs in the same order
__global__ __launch_bounds__(256) void adv_sum_kernel(const float *__restrict__ adv, const int64_t *__restrict__ src,
                                                      int M, double *__restrict__ asum) {
    __shared__ double s1[256], s2[256];
    const int t = threadIdx.x;
    const int per = (M + kAdvBlocks - 1) / kAdvBlocks;
    const int i0 = blockIdx.x * per, i1 = min(M, i0 + per);
    double a1 = 0.0, a2 = 0.0;
    for (int i = i0 + t; i < i1; i += 256) {
        const double a = adv[src ? src[i] : i];
        a1 += a;
        a2 += a * a;
    }
    s1[t] = a1;
    s2[t] = a2;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) {
            s1[t] += s1[t + h];
            s2[t] += s2[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        asum[2 * blockIdx.x] = s1[0];
        asum[2 * blockIdx.x + 1] = s2[0];
    }
}

// The clipped surrogate (head_loss.h: what an objective supplies).  f64 sums
// per block: min-surrogate, squared value error, entropy, kl, clipped.
struct PpoClip {
    static constexpr int kStats = 5;
    const int32_t *act;
    const float *adv, *old_lp;
    const double *asum;         // [kAdvBlocks][2] advantage sums
    int normalize;
    float clip;
    struct Block {
        float mean, den;        // the advantage mean and std + 1e-8
    };
    struct Sample {
        int act;
        float adv, olp;
        float lr, ratio, l1, l2, glp;   // policy()
    };

    // unbiased std; NaN for one sample, as torch (every thread folds the same
    // 64 pairs; the loads are uniform over the block)
    __device__ __forceinline__ Block begin(int M) const {
        float mean = 0.0f, den = 1.0f;
        if (normalize) {
            double a1 = 0.0, a2 = 0.0;
            for (int b = 0; b < kAdvBlocks; ++b) {
                a1 += asum[2 * b];
                a2 += asum[2 * b + 1];
            }
            const double n = M, m = a1 / n;
            const double var = M > 1 ? fmax(0.0, a2 - a1 * m) / (n - 1.0) : __builtin_nan("");
            mean = (float)m;
            den = (float)sqrt(var) + 1e-8f;
        }
        return {mean, den};
    }
    __device__ __forceinline__ Sample gather(const Block &b, int64_t r, int) const {
        Sample s;
        s.act = act[r];
        s.adv = (adv[r] - b.mean) / b.den;
        s.olp = old_lp[r];
        return s;
    }
    template <int AM>
    __device__ __forceinline__ void policy(const Block &, Sample &s, const head_loss::Forward<AM> &f, bool,
                                           float w, float inv_n) const {
        float lp = 0.0f;
#pragma unroll
        for (int a = 0; a < AM; ++a) lp = a == s.act ? f.lpa[a] : lp;
        s.lr = lp - s.olp;
        s.ratio = expf(s.lr);
        const float rc = fminf(fmaxf(s.ratio, 1.0f - clip), 1.0f + clip);
        s.l1 = s.adv * s.ratio;
        s.l2 = s.adv * rc;
        const float m1 = s.l1 < s.l2 ? 1.0f : (s.l1 > s.l2 ? 0.0f : 0.5f);
        const float inr = (s.ratio >= 1.0f - clip && s.ratio <= 1.0f + clip) ? 1.0f : 0.0f;
        s.glp = -inv_n * s.adv * s.ratio * (m1 + (1.0f - m1) * inr) * w;
    }
    template <int AM>
    __device__ __forceinline__ float dz(const Sample &s, const head_loss::Forward<AM> &f, int a) const {
        return s.glp * ((a == s.act ? 1.0f : 0.0f) - f.p[a]);
    }
    template <int AM>
    __device__ __forceinline__ void stats(const Sample &s, const head_loss::Forward<AM> &, double *st) const {
        st[0] += (double)fminf(s.l1, s.l2);
        st[3] += (double)((s.ratio - 1.0f) - s.lr);
        st[4] += fabsf(s.ratio - 1.0f) > clip ? 1.0 : 0.0;
    }
    // stats [6] = policy loss, value loss, entropy loss, loss, approx kl, clip fraction
    __device__ __forceinline__ void finish(const double *v, int M, float ent_coef, float vf_coef,
                                           double *stats) const {
        const double n = M;
        const double pl = -v[0] / n, vl = v[1] / n, el = -v[2] / n;
        stats[0] = pl;
        stats[1] = vl;
        stats[2] = el;
        stats[3] = pl + (double)ent_coef * el + (double)vf_coef * vl;
        stats[4] = v[3] / n;
        stats[5] = v[4] / n;
    }
};

}  // namespace
