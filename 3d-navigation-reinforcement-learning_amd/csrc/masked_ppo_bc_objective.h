// masked_ppo_bc_objective.h -- PpoBcMasked<Bc>, the objective of the masked
// PPO + cross-entropy entries (voxnav_masked_ppo_bc_loss.hip states the rule;
// voxnav_soft_ppo_bc_loss.hip uses it with BcSoft): PpoBc<Bc>
// (ppo_bc_objective.h) with the mask pointer, a Sample that carries the byte,
// and head_loss.h's kAllowed trait; the label's bits are masked_bc_objective.h's.
// Unit-local (an anonymous namespace): each unit instantiates its own kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "head_loss.h"
#include "masked_bc_objective.h"
#include "ppo_bc_objective.h"

namespace {

template <class Bc>
struct PpoBcMasked : PpoBc<Bc> {
    using Base = PpoBc<Bc>;
    static constexpr bool kAllowed = true;
    const uint8_t *mask;        // [rows] bit j: action j allowed
    struct Sample : Base::Sample {
        unsigned mask;
    };
    __device__ __forceinline__ Sample gather(const typename Base::Block &b, int64_t r, int A) const {
        Sample s;
        static_cast<typename Base::Sample &>(s) = Base::gather(b, r, A);
        s.mask = mask[r];
        return s;
    }
    __device__ __forceinline__ unsigned allowed(const Sample &s, int A) const {
        const unsigned taken = (unsigned)s.p.act < (unsigned)A ? 1u << s.p.act : 0u;
        return allowed_set(s.mask, taken | label_bits(s.b, A), A);
    }
};

}  // namespace
