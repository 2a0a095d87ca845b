// voxnav_masked_ppo_bc_loss.hip -- vn_ppo_bc_loss / vn_ppo_bc_loss_set with
// invalid-action masking (masked kickstart): kickstarted PPO's minibatch loss
// of voxnav_ppo_bc_loss.hip with the softmax of every sample restricted to its
// allowed actions, the taken action and the label's among them.
//
// The rule (include/voxnav.h states it once; this is the same text).  With
// full = 2^A - 1 and L_i the label's bits where sample i is labelled (its
// weight nonzero or absent; label form: bit lab_i when 0 <= lab_i < A; set
// form: set_i & full, labelled only when that is non-empty), else 0:
//   S_i   = (mask_i & full) | (1 << a_i) | L_i      (an empty S_i counts as full)
//   lp_ij = z_ij - logsumexp_{k in S_i} z_ik        (j in S_i)
//   p_ij  = exp(lp_ij)                              (j in S_i), 0 otherwise
//   H_i   = -sum_{j in S_i} p_ij lp_ij
//   q_i   = one-hot at the label, or the softmax of z_i restricted to set_i & full
//   dz_ij = g_lp,i ([j = a_i] - p_ij) + bc_coef (w_i / max(n,1)) (p_ij - q_ij)
//           + (ent_coef / M) p_ij (lp_ij + H_i)     (j in S_i), exactly 0 otherwise
// formed as (ppo term + bc term) + entropy term.  This is vn_ppo_loss_masked's
// rule extended by the label: the ratio and the cross-entropy never read a
// log-probability outside the support; the argmax behind the accuracy runs
// over S_i.  Everything else -- n, bc_coef on the gradient scale, the value
// term, stats [9], the workspaces (vn_ppo_bc_loss_part_floats), the launches
// (adv_sum_kernel, bc_count_kernel, loss, reduce) and the refusals, plus a
// NULL mask -- is the unmasked entry's.  With every S_i full the outputs are
// its bits; with bc_coef = 0 and the labels inside the masks dhp, dhv,
// grad_heads and stats[0..5] are vn_ppo_loss_masked's; with zero advantages
// (not normalised), bc_coef = 1 and the taken actions inside the masks the
// gradients are vn_bc_loss_masked's (vn_bc_loss_set_masked's).
//
// The objective is PpoBcMasked<Bc> (masked_ppo_bc_objective.h): PpoBc<Bc>
// (ppo_bc_objective.h) with the mask pointer, a Sample that carries the byte,
// and head_loss.h's kAllowed trait; the label's bits are masked_bc_objective.h's.
//
// HBM per sample: vn_ppo_bc_loss's + 1 B (the mask).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "bc_objective.h"
#include "head_loss.h"
#include "masked_bc_objective.h"
#include "masked_ppo_bc_objective.h"
#include "ppo_bc_objective.h"
#include "ppo_objective.h"
#include "vn_common.h"

using vn_detail::fail;

namespace {

// vn_ppo_bc_loss_masked (Bc = BcLabel, int32 labels) and vn_ppo_bc_loss_set_masked (BcSet, uint8 label sets)
template <class Bc, class Label>
int ppo_bc_masked_launch(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                         const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                         const float *advantages, const float *old_log_prob, const float *returns,
                         const Label *labels, const uint8_t *weight, const uint8_t *mask, int32_t M, int32_t F,
                         int32_t A, float clip_range, float ent_coef, float vf_coef, float bc_coef,
                         int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                         double *adv_sums, float *part, double *spart, void *stream) {
    constexpr bool SET = std::is_same<Bc, BcSet>::value;
    if (const int e = head_loss::check_args(!hp || !hv || !wa || !ba || !wv || !bv || !actions || !advantages ||
                                                !old_log_prob || !returns || !labels || !mask || !dhp || !dhv ||
                                                !grad_heads || !stats || !adv_sums || !part || !spart,
                                            M, F, A, ldh))
        return e;
    if (!(std::isfinite(bc_coef) && bc_coef >= 0.0f))
        return fail(VN_ERR_INVALID, "bc_coef %g: finite and >= 0", (double)bc_coef);
    const hipStream_t s = (hipStream_t)stream;
    if (normalize_advantage)
        hipLaunchKernelGGL(adv_sum_kernel, dim3(kAdvBlocks), dim3(256), 0, s, advantages, src, M, adv_sums);
    PpoBcMasked<Bc> obj{};
    obj.ppo = PpoClip{actions, advantages, old_log_prob, adv_sums, normalize_advantage, clip_range};
    obj.bc.lab = labels;
    obj.bc.wgt = weight;
    obj.mask = mask;
    // the labelled counts sit behind the blocks' sums in spart, as in voxnav_ppo_bc_loss.hip; the
    // count does not depend on the masks
    int64_t *cnt = reinterpret_cast<int64_t *>(spart + head_loss::blocks(M) * PpoBc<Bc>::kStats);
    obj.bc.cnt = cnt;
    obj.bc.counted = (SET || weight) ? 1 : 0;
    obj.bc_coef = bc_coef;
    if (obj.bc.counted)
        hipLaunchKernelGGL(bc_count_kernel<SET>, dim3(kCntBlocks), dim3(256), 0, s,
                           reinterpret_cast<const uint8_t *>(labels), weight, src, M, (1u << A) - 1u, cnt);
    const head_loss::HeadArgs g{hp,  hv,  ldh,  wa,    ba, wv, bv, src, returns,
                                dhp, dhv, part, spart, M,  F,  A,  ent_coef, vf_coef};
    head_loss::launch(g, obj, grad_heads, stats, s);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace

extern "C" {

int vn_ppo_bc_loss_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                          const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                          const float *advantages, const float *old_log_prob, const float *returns,
                          const int32_t *labels, const uint8_t *weight, const uint8_t *mask, int32_t M, int32_t F,
                          int32_t A, float clip_range, float ent_coef, float vf_coef, float bc_coef,
                          int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                          double *adv_sums, float *part, double *spart, void *stream) {
    return ppo_bc_masked_launch<BcLabel>(hp, hv, ldh, wa, ba, wv, bv, src, actions, advantages, old_log_prob, returns,
                                         labels, weight, mask, M, F, A, clip_range, ent_coef, vf_coef, bc_coef,
                                         normalize_advantage, dhp, dhv, grad_heads, stats, adv_sums, part, spart,
                                         stream);
}

int vn_ppo_bc_loss_set_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                              const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                              const float *advantages, const float *old_log_prob, const float *returns,
                              const uint8_t *label_set, const uint8_t *weight, const uint8_t *mask, int32_t M,
                              int32_t F, int32_t A, float clip_range, float ent_coef, float vf_coef, float bc_coef,
                              int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                              double *adv_sums, float *part, double *spart, void *stream) {
    return ppo_bc_masked_launch<BcSet>(hp, hv, ldh, wa, ba, wv, bv, src, actions, advantages, old_log_prob, returns,
                                       label_set, weight, mask, M, F, A, clip_range, ent_coef, vf_coef, bc_coef,
                                       normalize_advantage, dhp, dhv, grad_heads, stats, adv_sums, part, spart,
                                       stream);
}

}  // extern "C"
