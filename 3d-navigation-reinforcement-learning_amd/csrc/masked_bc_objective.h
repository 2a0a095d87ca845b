// masked_bc_objective.h -- what the masked cross-entropy objectives share
// (voxnav_masked_bc_loss.hip, voxnav_masked_ppo_bc_loss.hip; head_loss.h: the
// kAllowed trait): the label's bits of a sample, which always count as allowed,
// and BcMasked<Bc>, BcLabel or BcSet (bc_objective.h) plus the mask byte.
// Unit-local (an anonymous namespace): each unit instantiates its own kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bc_objective.h"
#include "head_loss.h"

namespace {

// L_i: the label's bits below A where the sample is labelled, else 0
__device__ __forceinline__ unsigned label_bits(const BcLabel::Sample &s, int A) {
    return (s.has && (unsigned)s.lab < (unsigned)A) ? 1u << s.lab : 0u;
}
__device__ __forceinline__ unsigned label_bits(const BcSet::Sample &s, int) { return s.has ? s.S : 0u; }

// S_i from the mask byte and the bits that always count (the label's, the taken action's); empty: full
__device__ __forceinline__ unsigned allowed_set(unsigned mask, unsigned always, int A) {
    const unsigned full = (1u << A) - 1u;
    const unsigned S = (mask & full) | always;
    return S ? S : full;
}

// vn_bc_loss_masked (Bc = BcLabel) / vn_bc_loss_set_masked (BcSet): S_i = (mask_i & full) | L_i
template <class Bc>
struct BcMasked : Bc {
    static constexpr bool kAllowed = true;
    const uint8_t *mask;        // [rows] bit j: action j allowed
    struct Sample : Bc::Sample {
        unsigned mask;
    };
    __device__ __forceinline__ Sample gather(const typename Bc::Block &b, int64_t r, int A) const {
        Sample s;
        static_cast<typename Bc::Sample &>(s) = Bc::gather(b, r, A);
        s.mask = mask[r];
        return s;
    }
    __device__ __forceinline__ unsigned allowed(const Sample &s, int A) const {
        return allowed_set(s.mask, label_bits(static_cast<const typename Bc::Sample &>(s), A), A);
    }
};

}  // namespace
