// voxnav_masked_loss.hip -- vn_ppo_loss with invalid-action masking (Huang &
// Ontanon 2020; sb3_contrib MaskablePPO.train: evaluate_actions with
// action_masks): the PPO minibatch loss of voxnav_ppo_loss.hip with the
// softmax of every sample restricted to its allowed actions.  With
//   S_i = (mask_i & (2^A - 1)) | (1 << a_i)   (the taken action always counts
//         as allowed; an empty set as full)
//   lp_ij = z_ij - logsumexp_{k in S_i} z_ik        (j in S_i)
//   p_ij  = exp(lp_ij)                              (j in S_i), 0 otherwise
//   H_i   = -sum_{j in S_i} p_ij lp_ij
//   dz_ij = g_lp_i ([j = a_i] - p_ij) + (ent_coef / n) p_ij (lp_ij + H_i)
//                                                   (j in S_i), exactly 0 otherwise
// and everything else -- the ratio, the clip, the advantage normalisation, the
// value term, stats [6], the workspaces and the three launches -- that file's.
// A masked action takes no part in the max, the log-sum-exp or the entropy and
// contributes selected zeros (no 0 * -inf), so a saturated head whose largest
// logit is masked stays finite.
//
// The objective is PpoClip (ppo_objective.h) plus the sample's allowed set,
// which head_loss.h's kernel takes as the compile-time trait kAllowed: the
// masked forward and backward are instantiated in this unit only.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "head_loss.h"
#include "ppo_objective.h"
#include "vn_common.h"

namespace {

struct PpoClipMasked : PpoClip {
    static constexpr bool kAllowed = true;
    const uint8_t *mask;        // [rows] bit j: action j allowed
    struct Sample : PpoClip::Sample {
        unsigned mask;
    };
    __device__ __forceinline__ Sample gather(const Block &b, int64_t r, int A) const {
        Sample s;
        static_cast<PpoClip::Sample &>(s) = PpoClip::gather(b, r, A);
        s.mask = mask[r];
        return s;
    }
    __device__ __forceinline__ unsigned allowed(const Sample &s, int A) const {
        const unsigned full = (1u << A) - 1u;
        const unsigned S = (s.mask & full) | ((unsigned)s.act < (unsigned)A ? 1u << s.act : 0u);
        return S ? S : full;
    }
};

}  // namespace

extern "C" {

int vn_ppo_loss_masked_part_floats(int32_t M, int32_t F, int32_t A, int64_t *n_part, int64_t *n_spart) {
    return head_loss::part_floats(M, F, A, PpoClipMasked::kStats, 2 * kAdvBlocks /* the advantage sums */, n_part,
                                  n_spart);
}

int vn_ppo_loss_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                       const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                       const float *advantages, const float *old_log_prob, const float *returns, const uint8_t *mask,
                       int32_t M, int32_t F, int32_t A, float clip_range, float ent_coef, float vf_coef,
                       int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                       double *adv_sums, float *part, double *spart, void *stream) {
    if (const int e = head_loss::check_args(!hp || !hv || !wa || !ba || !wv || !bv || !actions || !advantages ||
                                                !old_log_prob || !returns || !mask || !dhp || !dhv || !grad_heads ||
                                                !stats || !adv_sums || !part || !spart,
                                            M, F, A, ldh))
        return e;
    const hipStream_t s = (hipStream_t)stream;
    if (normalize_advantage)
        hipLaunchKernelGGL(adv_sum_kernel, dim3(kAdvBlocks), dim3(256), 0, s, advantages, src, M, adv_sums);
    const head_loss::HeadArgs g{hp,  hv,  ldh,  wa,    ba, wv, bv, src, returns,
                                dhp, dhv, part, spart, M,  F,  A,  ent_coef, vf_coef};
    PpoClipMasked obj;
    static_cast<PpoClip &>(obj) = PpoClip{actions, advantages, old_log_prob, adv_sums, normalize_advantage, clip_range};
    obj.mask = mask;
    head_loss::launch(g, obj, grad_heads, stats, s);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // extern "C"
