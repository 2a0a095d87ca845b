// bc_objective.h -- what is behaviour cloning's of the head loss (head_loss.h:
// what an objective supplies): the labelled count of the minibatch and the two
// cross-entropy objectives BcLabel / BcSet on BcCommon.  voxnav_bc_loss.hip
// states the formulas; vn_bc_loss / vn_bc_loss_set (there), vn_ppo_bc_loss /
// vn_ppo_bc_loss_set (voxnav_ppo_bc_loss.hip) and their masked forms
// (masked_bc_objective.h) use them.
// Unit-local (an anonymous namespace): each unit instantiates its own kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "head_loss.h"

namespace {

constexpr int kCntBlocks = 64; // blocks of the labelled count

// per-block counts of the minibatch's labelled samples (kCntBlocks blocks, a
// contiguous range each): integers, so their sum is exact in any order.  SET
// (label sets): a sample counts when its set has a bit below A and its weight,
// if any, is nonzero; else when its weight (given) is nonzero.
template <bool SET>
__global__ __launch_bounds__(256) void bc_count_kernel(const uint8_t *__restrict__ set,
                                                       const uint8_t *__restrict__ wgt,
                                                       const int64_t *__restrict__ src, int M, uint32_t amask,
                                                       int64_t *__restrict__ cnt) {
    __shared__ int s[256];
    const int t = threadIdx.x;
    const int per = (M + kCntBlocks - 1) / kCntBlocks;
    const int i0 = blockIdx.x * per, i1 = min(M, i0 + per);
    int c = 0;
    for (int i = i0 + t; i < i1; i += 256) {
        const int64_t r = src ? src[i] : i;
        if constexpr (SET) c += ((set[r] & amask) != 0u && (wgt == nullptr || wgt[r] != 0)) ? 1 : 0;
        else c += wgt[r] != 0 ? 1 : 0;
    }
    s[t] = c;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) s[t] += s[t + h];
        __syncthreads();
    }
    if (t == 0) cnt[blockIdx.x] = s[0];
}

// What the two cross-entropy objectives share (head_loss.h: what an objective
// supplies).  f64 sums per block: cross-entropy, squared value error, entropy,
// correct argmax.
struct BcCommon {
    static constexpr int kStats = 4;
    const uint8_t *wgt;         // 1 = labelled (NULL: all)
    const int64_t *cnt;         // [kCntBlocks] labelled counts (read when counted)
    int counted;                // launch (1) ran: weights, or label sets
    struct Block {
        float inv_l;            // 1 / max(n, 1) with n the labelled count
    };

    // the labelled count n of the minibatch (M when nothing was counted)
    __device__ __forceinline__ int64_t labelled(int M) const {
        if (!counted) return M;
        int64_t n = 0;
        for (int b = 0; b < kCntBlocks; ++b) n += cnt[b];
        return n;
    }
    // (every thread folds the same 64 integers; the loads are uniform over the block)
    __device__ __forceinline__ Block begin(int M) const {
        const int64_t n_lab = labelled(M);
        return {1.0f / (float)(n_lab > 0 ? n_lab : 1)};
    }
    // stats [6] = cross-entropy, value loss, entropy loss, loss, accuracy, labelled share
    __device__ __forceinline__ void finish(const double *v, int M, float ent_coef, float vf_coef,
                                           double *stats) const {
        const int64_t nl = labelled(M);
        const double n = M, dl = (double)(nl > 0 ? nl : 1);
        const double ce = v[0] / dl, vl = v[1] / n, el = -v[2] / n;
        stats[0] = ce;
        stats[1] = vl;
        stats[2] = el;
        stats[3] = ce + (double)ent_coef * el + (double)vf_coef * vl;
        stats[4] = v[3] / dl;
        stats[5] = (double)nl / n;
    }
};

// vn_bc_loss: one expert action per sample
struct BcLabel : BcCommon {
    const int32_t *lab;
    struct Sample {
        int lab;
        bool has;
        float lp, gce;          // policy(): the label's log-probability, the cross-entropy's gradient scale
    };
    __device__ __forceinline__ Sample gather(const Block &, int64_t r, int) const {
        Sample s;
        s.lab = lab[r];
        s.has = wgt ? wgt[r] != 0 : true;
        return s;
    }
    template <int AM>
    __device__ __forceinline__ void policy(const Block &b, Sample &s, const head_loss::Forward<AM> &f, bool ok, float,
                                           float) const {
        s.lp = 0.0f;
#pragma unroll
        for (int a = 0; a < AM; ++a) s.lp = a == s.lab ? f.lpa[a] : s.lp;
        s.gce = (s.has && ok) ? b.inv_l : 0.0f;
    }
    template <int AM>
    __device__ __forceinline__ float dz(const Sample &s, const head_loss::Forward<AM> &f, int a) const {
        return s.gce * (f.p[a] - (a == s.lab ? 1.0f : 0.0f));
    }
    template <int AM>
    __device__ __forceinline__ void stats(const Sample &s, const head_loss::Forward<AM> &f, double *st) const {
        st[0] += s.has ? (double)(-s.lp) : 0.0;
        st[3] += (s.has && f.amax == s.lab) ? 1.0 : 0.0;
    }
};

// vn_bc_loss_set: a set of equally good actions per sample (a uint8 bit set);
// the target of the cross-entropy is the softmax restricted to the set, and a
// sample with an empty set is unlabelled
struct BcSet : BcCommon {
    const uint8_t *lab;         // the label sets
    struct Sample {
        uint32_t S;             // the label set, bits below A
        bool has;
        float lp, gce;          // policy(): the whole set's log-probability, the gradient scale
        float q[head_loss::kMaxA];   // policy(): the target distribution
    };
    __device__ __forceinline__ Sample gather(const Block &, int64_t r, int A) const {
        Sample s;
        s.S = (uint32_t)lab[r] & ((1u << A) - 1u);
        s.has = wgt ? wgt[r] != 0 : true;
        s.has = s.has && s.S != 0u;
        return s;
    }
    template <int AM>
    __device__ __forceinline__ void policy(const Block &b, Sample &s, const head_loss::Forward<AM> &f, bool ok, float,
                                           float) const {
        const uint32_t S = s.S;
        // logsumexp over S around S's own maximum: a set far below the top logit keeps its digits
        float zs = -INFINITY, ses = 0.0f;
#pragma unroll
        for (int a = 0; a < AM; ++a) zs = ((S >> a) & 1u) ? fmaxf(zs, f.z[a]) : zs;
#pragma unroll
        for (int a = 0; a < AM; ++a) {
            s.q[a] = ((S >> a) & 1u) ? expf(f.z[a] - zs) : 0.0f;
            ses += s.q[a];
        }
        const float inv_s = S != 0u ? 1.0f / ses : 0.0f;
#pragma unroll
        for (int a = 0; a < AM; ++a) s.q[a] *= inv_s;
        s.lp = S != 0u ? (zs + logf(ses)) - (f.zmax + f.lse) : 0.0f;
        s.gce = (s.has && ok) ? b.inv_l : 0.0f;
    }
    template <int AM>
    __device__ __forceinline__ float dz(const Sample &s, const head_loss::Forward<AM> &f, int a) const {
        return s.gce * (f.p[a] - s.q[a]);
    }
    template <int AM>
    __device__ __forceinline__ void stats(const Sample &s, const head_loss::Forward<AM> &f, double *st) const {
        st[0] += s.has ? (double)(-s.lp) : 0.0;
        st[3] += (s.has && ((s.S >> f.amax) & 1u) != 0u) ? 1.0 : 0.0;
    }
};

}  // namespace
