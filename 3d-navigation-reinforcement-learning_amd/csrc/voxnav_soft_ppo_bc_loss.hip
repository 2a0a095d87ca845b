// voxnav_soft_ppo_bc_loss.hip -- kickstarted PPO's minibatch loss (f32) with
// the distance-weighted target: vn_ppo_bc_loss (voxnav_ppo_bc_loss.hip) with
// vn_bc_loss_soft's KL(q || pi) (voxnav_soft_bc_loss.hip states the target) in
// the cross-entropy's place (vn_ppo_bc_loss_soft), and the same with
// invalid-action masking (vn_ppo_bc_loss_soft_masked).
//
// The loss (include/voxnav.h states it once; this is the same text): the
// formulas of vn_ppo_bc_loss with q_i the distance-weighted target, ce_i = kl_i
// and n the count of samples with a positive distance and a nonzero weight.
// The objectives are PpoBc<BcSoft> (ppo_bc_objective.h, soft_bc_objective.h)
// and PpoBcMasked<BcSoft> (masked_ppo_bc_objective.h), whose softmax runs over
//   S_i = (mask_i & full) | (1 << a_i) | L_i,  L_i = P_i where labelled
// (an empty S_i counts as full): the identities of the composition hold as they
// do for the label and set forms -- bc_coef = 0 gives vn_ppo_loss's
// (vn_ppo_loss_masked's) values, zero advantages (not normalised) with
// bc_coef = 1 the gradients of vn_bc_loss_soft (vn_bc_loss_soft_masked), every
// S_i full the unmasked entry's bits.
//
// Launches: (1) adv_sum_kernel when normalize_advantage; (2)
// bc_soft_count_kernel, always; (3) head_loss_kernel<Q, AM, PpoBc<BcSoft>>;
// (4) the reduce kernel.  Plain stores, fixed orders: two calls on the same
// inputs give the same bits.  Workspaces: vn_ppo_bc_loss_part_floats.
//
// HBM per sample: vn_ppo_bc_loss_set's + 4 A B (the distance row) - 1 B (no set).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bc_objective.h"
#include "head_loss.h"
#include "masked_bc_objective.h"
#include "masked_ppo_bc_objective.h"
#include "ppo_bc_objective.h"
#include "ppo_objective.h"
#include "soft_bc_objective.h"
#include "vn_common.h"

using vn_detail::fail;

namespace {

// vn_ppo_bc_loss_soft (Obj = PpoBc<BcSoft>; mask unused) and vn_ppo_bc_loss_soft_masked (PpoBcMasked<BcSoft>)
template <class Obj>
int ppo_bc_soft_launch(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                       const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                       const float *advantages, const float *old_log_prob, const float *returns,
                       const int32_t *dists, int64_t ldd, const uint8_t *weight, const uint8_t *mask, bool masked,
                       int32_t M, int32_t F, int32_t A, float clip_range, float ent_coef, float vf_coef,
                       float bc_coef, float tau, int32_t normalize_advantage, float *dhp, float *dhv,
                       float *grad_heads, double *stats, double *adv_sums, float *part, double *spart, void *stream,
                       Obj obj) {
    if (const int e = head_loss::check_args(!hp || !hv || !wa || !ba || !wv || !bv || !actions || !advantages ||
                                                !old_log_prob || !returns || !dists || (masked && !mask) || !dhp ||
                                                !dhv || !grad_heads || !stats || !adv_sums || !part || !spart,
                                            M, F, A, ldh))
        return e;
    if (!(std::isfinite(bc_coef) && bc_coef >= 0.0f))
        return fail(VN_ERR_INVALID, "bc_coef %g: finite and >= 0", (double)bc_coef);
    if (const int e = check_soft_args(ldd, A, tau)) return e;
    const hipStream_t s = (hipStream_t)stream;
    if (normalize_advantage)
        hipLaunchKernelGGL(adv_sum_kernel, dim3(kAdvBlocks), dim3(256), 0, s, advantages, src, M, adv_sums);
    obj.ppo = PpoClip{actions, advantages, old_log_prob, adv_sums, normalize_advantage, clip_range};
    obj.bc.dists = dists;
    obj.bc.ldd = ldd;
    obj.bc.tau = tau;
    obj.bc.wgt = weight;
    // the labelled counts sit behind the blocks' sums in spart, as in voxnav_ppo_bc_loss.hip
    int64_t *cnt = reinterpret_cast<int64_t *>(spart + head_loss::blocks(M) * PpoBc<BcSoft>::kStats);
    obj.bc.cnt = cnt;
    obj.bc.counted = 1;
    obj.bc_coef = bc_coef;
    hipLaunchKernelGGL(bc_soft_count_kernel, dim3(kCntBlocks), dim3(256), 0, s, dists, ldd, weight, src, M, A, cnt);
    const head_loss::HeadArgs g{hp,  hv,  ldh,  wa,    ba, wv, bv, src, returns,
                                dhp, dhv, part, spart, M,  F,  A,  ent_coef, vf_coef};
    head_loss::launch(g, obj, grad_heads, stats, s);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace

extern "C" {

int vn_ppo_bc_loss_soft(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                        const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                        const float *advantages, const float *old_log_prob, const float *returns,
                        const int32_t *dists, int64_t ldd, const uint8_t *weight, int32_t M, int32_t F, int32_t A,
                        float clip_range, float ent_coef, float vf_coef, float bc_coef, float tau,
                        int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                        double *adv_sums, float *part, double *spart, void *stream) {
    return ppo_bc_soft_launch(hp, hv, ldh, wa, ba, wv, bv, src, actions, advantages, old_log_prob, returns, dists,
                              ldd, weight, nullptr, false, M, F, A, clip_range, ent_coef, vf_coef, bc_coef, tau,
                              normalize_advantage, dhp, dhv, grad_heads, stats, adv_sums, part, spart, stream,
                              PpoBc<BcSoft>{});
}

int vn_ppo_bc_loss_soft_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                               const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                               const float *advantages, const float *old_log_prob, const float *returns,
                               const int32_t *dists, int64_t ldd, const uint8_t *weight, const uint8_t *mask,
                               int32_t M, int32_t F, int32_t A, float clip_range, float ent_coef, float vf_coef,
                               float bc_coef, float tau, int32_t normalize_advantage, float *dhp, float *dhv,
                               float *grad_heads, double *stats, double *adv_sums, float *part, double *spart,
                               void *stream) {
    PpoBcMasked<BcSoft> obj{};
    obj.mask = mask;
    return ppo_bc_soft_launch(hp, hv, ldh, wa, ba, wv, bv, src, actions, advantages, old_log_prob, returns, dists,
                              ldd, weight, mask, true, M, F, A, clip_range, ent_coef, vf_coef, bc_coef, tau,
                              normalize_advantage, dhp, dhv, grad_heads, stats, adv_sums, part, spart, stream, obj);
}

}  // extern "C"
