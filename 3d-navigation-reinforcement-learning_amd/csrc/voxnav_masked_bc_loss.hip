// voxnav_masked_bc_loss.hip -- vn_bc_loss / vn_bc_loss_set with invalid-action
// masking (masked DAgger): the behaviour-cloning minibatch loss of
// voxnav_bc_loss.hip with the softmax of every sample restricted to its allowed
// actions, the label's among them.
//
// The rule (include/voxnav.h states it once; this is the same text).  With
// full = 2^A - 1 and L_i the label's bits where sample i is labelled (its
// weight nonzero or absent; label form: bit lab_i when 0 <= lab_i < A; set
// form: set_i & full, labelled only when that is non-empty), else 0:
//   S_i   = (mask_i & full) | L_i          (an empty S_i counts as full)
//   lp_ij = z_ij - logsumexp_{k in S_i} z_ik        (j in S_i)
//   p_ij  = exp(lp_ij)                              (j in S_i), 0 otherwise
//   H_i   = -sum_{j in S_i} p_ij lp_ij
//   q_i   = one-hot at the label, or the softmax of z_i restricted to set_i & full
//   dz_ij = (w_i / max(n,1)) (p_ij - q_ij) + (ent_coef / M) p_ij (lp_ij + H_i)
//                                                   (j in S_i), exactly 0 otherwise
// The label lies in S_i, so the cross-entropy never reads a log-probability
// outside the support; the argmax behind the accuracy runs over S_i.
// Everything else -- n, the value term, stats [6], the workspaces
// (vn_bc_loss_part_floats), the launches (bc_count_kernel, loss, reduce) and
// the refusals, plus a NULL mask -- is the unmasked entry's.  With every S_i
// full the outputs are its bits.
//
// The objectives are BcMasked<BcLabel> / BcMasked<BcSet>
// (masked_bc_objective.h): BcLabel / BcSet (bc_objective.h) with the mask
// pointer, a Sample that carries the byte, and head_loss.h's kAllowed trait.
// The masked forward and backward are instantiated in this unit (and in
// voxnav_masked_loss.hip, voxnav_masked_ppo_bc_loss.hip) only.
//
// HBM per sample: vn_bc_loss's + 1 B (the mask).

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "bc_objective.h"
#include "head_loss.h"
#include "masked_bc_objective.h"
#include "vn_common.h"

namespace {

// vn_bc_loss_masked (Bc = BcLabel, int32 labels) and vn_bc_loss_set_masked (BcSet, uint8 label sets)
template <class Bc, class Label>
int bc_masked_launch(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                     const float *bv, const int64_t *src, const Label *labels, const uint8_t *weight,
                     const uint8_t *mask, const float *returns, int32_t M, int32_t F, int32_t A, float ent_coef,
                     float vf_coef, float *dhp, float *dhv, float *grad_heads, double *stats, float *part,
                     double *spart, void *stream) {
    constexpr bool SET = std::is_same<Bc, BcSet>::value;
    if (const int e = head_loss::check_args(!hp || !hv || !wa || !ba || !wv || !bv || !labels || !mask || !returns ||
                                                !dhp || !dhv || !grad_heads || !stats || !part || !spart,
                                            M, F, A, ldh))
        return e;
    const hipStream_t s = (hipStream_t)stream;
    BcMasked<Bc> obj{};
    obj.lab = labels;
    obj.wgt = weight;
    obj.mask = mask;
    // the labelled counts sit behind the blocks' sums in spart, as in voxnav_bc_loss.hip; the
    // count does not depend on the masks
    int64_t *cnt = reinterpret_cast<int64_t *>(spart + head_loss::blocks(M) * Bc::kStats);
    obj.cnt = cnt;
    obj.counted = (SET || weight) ? 1 : 0;
    if (obj.counted)
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

int vn_bc_loss_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                      const float *wv, const float *bv, const int64_t *src, const int32_t *labels,
                      const uint8_t *weight, const uint8_t *mask, const float *returns, int32_t M, int32_t F,
                      int32_t A, float ent_coef, float vf_coef, float *dhp, float *dhv, float *grad_heads,
                      double *stats, float *part, double *spart, void *stream) {
    return bc_masked_launch<BcLabel>(hp, hv, ldh, wa, ba, wv, bv, src, labels, weight, mask, returns, M, F, A,
                                     ent_coef, vf_coef, dhp, dhv, grad_heads, stats, part, spart, stream);
}

int vn_bc_loss_set_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                          const float *wv, const float *bv, const int64_t *src, const uint8_t *label_set,
                          const uint8_t *weight, const uint8_t *mask, const float *returns, int32_t M, int32_t F,
                          int32_t A, float ent_coef, float vf_coef, float *dhp, float *dhv, float *grad_heads,
                          double *stats, float *part, double *spart, void *stream) {
    return bc_masked_launch<BcSet>(hp, hv, ldh, wa, ba, wv, bv, src, label_set, weight, mask, returns, M, F, A,
                                   ent_coef, vf_coef, dhp, dhv, grad_heads, stats, part, spart, stream);
}

}  // extern "C"
