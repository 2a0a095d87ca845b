// voxnav_ppo_bc_loss.hip -- kickstarted PPO's minibatch loss (f32): the PPO
// loss of vn_ppo_loss with the cross-entropy to the planner's labels of
// vn_bc_loss / vn_bc_loss_set added under a coefficient, and the gradient of
// the sum down to the MLP latents, in one pass over the samples (Schmitt et
// al., "Kickstarting Deep Reinforcement Learning", 2018).
//
// The loss (include/voxnav.h states it once; this is the same text).  lp, p, H
// and v are head_loss.h's; A_i, r_i and g_lp,i those of vn_ppo_loss (the
// optionally normalised advantage, the ratio, the surrogate's gradient scale);
// w_i, n and q_i those of vn_bc_loss / vn_bc_loss_set (q_i one-hot at the
// label, or the softmax of z restricted to S_i = set_i & (2^A - 1); n the
// labelled count, with sets only samples with S_i != 0):
//   loss  = -mean(min(A r, A clamp(r, 1-c, 1+c))) - ent_coef mean(H)
//           + vf_coef mean((ret - v)^2) + bc_coef (1/max(n,1)) sum_i w_i ce_i
//   dz_ij = g_lp,i (d_j,a_i - p_ij) + bc_coef (w_i / max(n,1)) (p_ij - q_ij)
//           + (ent_coef / M) p_ij (lp_ij + H_i)
//   dv_i  = 2 vf_coef (v_i - ret_i) / M
// dz is formed as (ppo term + bc term) + entropy term.  With bc_coef = 0 or no
// labelled sample the bc term is a zero and every output equals vn_ppo_loss's;
// with zero advantages (not normalised) and bc_coef = 1 the ppo term is a zero
// and the gradients equal vn_bc_loss's.  n = 0: the cross-entropy, its
// gradient and the accuracy are exactly 0.
//
// The objective PpoBc<Bc> (ppo_bc_objective.h) is composed of PpoClip
// (ppo_objective.h) and BcLabel or BcSet (bc_objective.h): their members run as
// they are, on their own parts of the block and sample records (the masked
// forms, voxnav_masked_ppo_bc_loss.hip, compose it too).  f64 sums per block
// [7]: PPO's five (surrogate, squared value error, entropy, kl, clipped), the
// cross-entropy, the correct argmax.
//
// Launches: (1) adv_sum_kernel when normalize_advantage; (2) bc_count_kernel
// with weights or sets (each loss block folds the 64 pairs, then the 64 counts,
// in order); (3) head_loss_kernel<Q, AM, PpoBc<Bc>>; (4) the reduce kernel.
// Plain stores, fixed orders: two calls on the same inputs give the same bits.
//
// HBM per sample: vn_ppo_loss's + 5 B (label 4 B or set 1 B, weight 1 B).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "bc_objective.h"
#include "head_loss.h"
#include "ppo_bc_objective.h"
#include "ppo_objective.h"
#include "vn_common.h"

using vn_detail::fail;

namespace {

// vn_ppo_bc_loss (Bc = BcLabel, int32 labels) and vn_ppo_bc_loss_set (BcSet, uint8 label sets)
template <class Bc, class Label>
int ppo_bc_launch(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                  const float *bv, const int64_t *src, const int32_t *actions, const float *advantages,
                  const float *old_log_prob, const float *returns, const Label *labels, const uint8_t *weight,
                  int32_t M, int32_t F, int32_t A, float clip_range, float ent_coef, float vf_coef, float bc_coef,
                  int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                  double *adv_sums, float *part, double *spart, void *stream) {
    constexpr bool SET = std::is_same<Bc, BcSet>::value;
    if (const int e = head_loss::check_args(!hp || !hv || !wa || !ba || !wv || !bv || !actions || !advantages ||
                                                !old_log_prob || !returns || !labels || !dhp || !dhv ||
                                                !grad_heads || !stats || !adv_sums || !part || !spart,
                                            M, F, A, ldh))
        return e;
    if (!(std::isfinite(bc_coef) && bc_coef >= 0.0f))
        return fail(VN_ERR_INVALID, "bc_coef %g: finite and >= 0", (double)bc_coef);
    const hipStream_t s = (hipStream_t)stream;
    if (normalize_advantage)
        hipLaunchKernelGGL(adv_sum_kernel, dim3(kAdvBlocks), dim3(256), 0, s, advantages, src, M, adv_sums);
    PpoBc<Bc> obj{};
    obj.ppo = PpoClip{actions, advantages, old_log_prob, adv_sums, normalize_advantage, clip_range};
    obj.bc.lab = labels;
    obj.bc.wgt = weight;
    // the labelled counts sit behind the blocks' sums in spart (8-byte words both)
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

int vn_ppo_bc_loss_part_floats(int32_t M, int32_t F, int32_t A, int64_t *n_part, int64_t *n_spart) {
    return head_loss::part_floats(M, F, A, PpoBc<BcLabel>::kStats, kCntBlocks /* the labelled counts (int64 words) */,
                                  n_part, n_spart);
}

int vn_ppo_bc_loss(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                   const float *bv, const int64_t *src, const int32_t *actions, const float *advantages,
                   const float *old_log_prob, const float *returns, const int32_t *labels, const uint8_t *weight,
                   int32_t M, int32_t F, int32_t A, float clip_range, float ent_coef, float vf_coef, float bc_coef,
                   int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                   double *adv_sums, float *part, double *spart, void *stream) {
    return ppo_bc_launch<BcLabel>(hp, hv, ldh, wa, ba, wv, bv, src, actions, advantages, old_log_prob, returns, labels,
                                  weight, M, F, A, clip_range, ent_coef, vf_coef, bc_coef, normalize_advantage, dhp,
                                  dhv, grad_heads, stats, adv_sums, part, spart, stream);
}

int vn_ppo_bc_loss_set(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                       const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                       const float *advantages, const float *old_log_prob, const float *returns,
                       const uint8_t *label_set, const uint8_t *weight, int32_t M, int32_t F, int32_t A,
                       float clip_range, float ent_coef, float vf_coef, float bc_coef, int32_t normalize_advantage,
                       float *dhp, float *dhv, float *grad_heads, double *stats, double *adv_sums, float *part,
                       double *spart, void *stream) {
    return ppo_bc_launch<BcSet>(hp, hv, ldh, wa, ba, wv, bv, src, actions, advantages, old_log_prob, returns,
                                label_set, weight, M, F, A, clip_range, ent_coef, vf_coef, bc_coef,
                                normalize_advantage, dhp, dhv, grad_heads, stats, adv_sums, part, spart, stream);
}

}  // extern "C"
