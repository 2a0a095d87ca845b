// ppo_bc_objective.h -- kickstarted PPO's objective PpoBc<Bc> (head_loss.h:
// what an objective supplies), composed of PpoClip (ppo_objective.h) and
// BcLabel or BcSet (bc_objective.h): their members run as they are, on their
// own parts of the block and sample records.  voxnav_ppo_bc_loss.hip states the
// formula; vn_ppo_bc_loss / vn_ppo_bc_loss_set (there) and their masked forms
// (voxnav_masked_ppo_bc_loss.hip) use it.
// Unit-local (an anonymous namespace): each unit instantiates its own kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bc_objective.h"
#include "head_loss.h"
#include "ppo_objective.h"

namespace {

template <class Bc>
struct PpoBc {
    static constexpr int kStats = 7;
    PpoClip ppo;
    Bc bc;
    float bc_coef;
    struct Block {
        PpoClip::Block p;
        typename Bc::Block b;
    };
    struct Sample {
        PpoClip::Sample p;
        typename Bc::Sample b;
    };

    __device__ __forceinline__ Block begin(int M) const { return {ppo.begin(M), bc.begin(M)}; }
    __device__ __forceinline__ Sample gather(const Block &b, int64_t r, int A) const {
        return {ppo.gather(b.p, r, A), bc.gather(b.b, r, A)};
    }
    template <int AM>
    __device__ __forceinline__ void policy(const Block &b, Sample &s, const head_loss::Forward<AM> &f, bool ok, float w,
                                           float inv_n) const {
        ppo.policy(b.p, s.p, f, ok, w, inv_n);
        bc.policy(b.b, s.b, f, ok, w, inv_n);
        s.b.gce *= bc_coef;     // bc_coef = 1: the cross-entropy's own scale, bit for bit
    }
    template <int AM>
    __device__ __forceinline__ float dz(const Sample &s, const head_loss::Forward<AM> &f, int a) const {
        return ppo.dz(s.p, f, a) + bc.dz(s.b, f, a);
    }
    // PPO's slots are the block's 0, 3, 4; the cross-entropy objective's 0 and 3 land in 5 and 6
    template <int AM>
    __device__ __forceinline__ void stats(const Sample &s, const head_loss::Forward<AM> &f, double *st) const {
        ppo.stats(s.p, f, st);
        double t[BcCommon::kStats] = {0.0, 0.0, 0.0, 0.0};
        bc.stats(s.b, f, t);
        st[5] += t[0];
        st[6] += t[3];
    }
    // stats [9] = vn_ppo_loss's six (the loss with bc_coef ce added), cross-entropy, accuracy, labelled share
    __device__ __forceinline__ void finish(const double *v, int M, float ent_coef, float vf_coef,
                                           double *stats) const {
        double p[6], b[6];
        ppo.finish(v, M, ent_coef, vf_coef, p);
        const double vb[BcCommon::kStats] = {v[5], v[1], v[2], v[6]};
        bc.finish(vb, M, ent_coef, vf_coef, b);
        p[3] = p[3] + (double)bc_coef * b[0];
        for (int k = 0; k < 6; ++k) stats[k] = p[k];
        stats[6] = b[0];
        stats[7] = b[4];
        stats[8] = b[5];
    }
};

}  // namespace
