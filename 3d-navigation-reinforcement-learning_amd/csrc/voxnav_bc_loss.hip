// voxnav_bc_loss.hip -- the DAgger warm start's kernels (f32): the
// behaviour-cloning minibatch loss with its gradient down to the MLP latents
// (vn_bc_loss, the counterpart of vn_ppo_loss in voxnav_ppo_loss.hip; and
// vn_bc_loss_set, the same on sets of labels), and the
// per-step choice between the planner's action and the policy's own
// (vn_dagger_mix).
//
// The loss (include/voxnav.h states it once; this is the same text):
//   z = h_pi Wa^T + ba,  lp = log_softmax(z),  p = exp(lp),  H = -sum_j p_j lp_j
//   v = h_vf wv + bv,    n = sum_i w_i  (w_i in {0,1};  n = M without weights)
//   loss = (1/max(n,1)) sum_i w_i (-lp_i[a*_i]) - ent_coef (1/M) sum_i H_i
//          + vf_coef (1/M) sum_i (ret_i - v_i)^2
//   dz_ij = (w_i / max(n,1)) (p_ij - [j = a*_i]) + (ent_coef / M) p_ij (lp_ij + H_i)
//   dv_i  = 2 vf_coef (v_i - ret_i) / M
//   dh_pi = dz Wa, dh_vf = dv wv, dWa = dz^T h_pi, dba = sum dz, dwv, dbv
//
// Launches: (1) with weights only, 64 blocks: the labelled count of the
// minibatch, an exact integer sum (each loss block folds the 64 counts, in
// order; the count never leaves the device); (2) the samples,
// head_loss_kernel<Q, AM, BcLabel>; (3) the partials summed in a fixed order,
// head_loss_reduce_kernel<BcLabel>, so two calls on the same inputs give the
// same bits.  head_loss.h has the kernels' tiling and their LDS layout;
// bc_objective.h has what is BC's: the labelled count and the two
// cross-entropy objectives (voxnav_ppo_bc_loss.hip composes them too).
//
// vn_bc_loss_set is the same call with a set of equally good actions per
// sample (a uint8 bit set) in place of the label:
//   S = set & (2^A - 1);  labelled iff S != 0 and w != 0
//   ce = logsumexp_j z_j - logsumexp_{j in S} z_j,  q = softmax of z restricted to S
//   dz_ij = (w_i / max(n,1)) (p_ij - q_ij) + the entropy term above
// through the objective BcSet; its labelled count depends on the sets, so
// launch (1) always runs.
//
// HBM per sample: the two latent rows read (2 F 4 B) and their gradient rows
// written (2 F 4 B) + 9 B of gathered buffer scalars (label, weight, return)
// + the 8 B row index.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "bc_objective.h"
#include "head_loss.h"
#include "vn_common.h"

using vn_detail::fail;
using vn_detail::philox_word0;

namespace {

// ---- DAgger's executed action (Ross et al. 2011: the expert's with
// probability beta, else the learner's own) ----
// One thread per agent; the draw is the sampler's Philox word under another
// key, so it does not depend on how the agents are sharded.  executed may be
// the policy array itself: each thread reads its element before it writes it.
__global__ __launch_bounds__(256) void dagger_mix_kernel(const int32_t *policy, const int32_t *__restrict__ expert,
                                                         const int32_t *__restrict__ dist, int N, uint32_t thr,
                                                         uint64_t seed, uint64_t t, uint64_t gid_base,
                                                         int32_t *executed, uint8_t *__restrict__ took,
                                                         uint8_t *__restrict__ weight) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint32_t u24 = philox_word0(seed, gid_base + (uint64_t)i, t | (1ull << 63)) >> 8;
    const bool lab = dist[i] != -1;
    const bool tk = lab && u24 < thr;
    const int32_t a = tk ? expert[i] : policy[i];
    executed[i] = a;
    took[i] = tk ? 1 : 0;
    weight[i] = lab ? 1 : 0;
}

// vn_bc_loss (Obj = BcLabel, int32 labels) and vn_bc_loss_set (BcSet, uint8 label sets)
template <class Obj, class Label>
int bc_launch(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
              const float *bv, const int64_t *src, const Label *labels, const uint8_t *weight, const float *returns,
              int32_t M, int32_t F, int32_t A, float ent_coef, float vf_coef, float *dhp, float *dhv,
              float *grad_heads, double *stats, float *part, double *spart, void *stream) {
    constexpr bool SET = std::is_same<Obj, BcSet>::value;
    if (const int e = head_loss::check_args(!hp || !hv || !wa || !ba || !wv || !bv || !labels || !returns || !dhp ||
                                                !dhv || !grad_heads || !stats || !part || !spart,
                                            M, F, A, ldh))
        return e;
    const hipStream_t s = (hipStream_t)stream;
    Obj obj{};
    obj.lab = labels;
    obj.wgt = weight;
    // the labelled counts sit behind the blocks' sums in spart (8-byte words both); a set may be
    // empty, so the labelled count of the set form depends on the sets: always counted
    int64_t *cnt = reinterpret_cast<int64_t *>(spart + head_loss::blocks(M) * Obj::kStats);
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

int vn_bc_loss_part_floats(int32_t M, int32_t F, int32_t A, int64_t *n_part, int64_t *n_spart) {
    return head_loss::part_floats(M, F, A, BcCommon::kStats, kCntBlocks /* the labelled counts (int64 words) */,
                                  n_part, n_spart);
}

int vn_bc_loss(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
               const float *bv, const int64_t *src, const int32_t *labels, const uint8_t *weight,
               const float *returns, int32_t M, int32_t F, int32_t A, float ent_coef, float vf_coef, float *dhp,
               float *dhv, float *grad_heads, double *stats, float *part, double *spart, void *stream) {
    return bc_launch<BcLabel>(hp, hv, ldh, wa, ba, wv, bv, src, labels, weight, returns, M, F, A, ent_coef, vf_coef,
                              dhp, dhv, grad_heads, stats, part, spart, stream);
}

int vn_bc_loss_set(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                   const float *bv, const int64_t *src, const uint8_t *label_set, const uint8_t *weight,
                   const float *returns, int32_t M, int32_t F, int32_t A, float ent_coef, float vf_coef, float *dhp,
                   float *dhv, float *grad_heads, double *stats, float *part, double *spart, void *stream) {
    return bc_launch<BcSet>(hp, hv, ldh, wa, ba, wv, bv, src, label_set, weight, returns, M, F, A, ent_coef, vf_coef,
                            dhp, dhv, grad_heads, stats, part, spart, stream);
}

int vn_dagger_mix(const int32_t *policy, const int32_t *expert, const int32_t *dist, int32_t N, double beta,
                  uint64_t mix_seed, uint64_t t_global, int64_t agent_id_base, int32_t *executed, uint8_t *took_expert,
                  uint8_t *label_weight, void *stream) {
    if (!policy || !expert || !dist || !executed || !took_expert || !label_weight)
        return fail(VN_ERR_INVALID, "NULL argument");
    if (N < 1) return fail(VN_ERR_INVALID, "bad size N=%d", N);
    if (!(beta >= 0.0 && beta <= 1.0)) return fail(VN_ERR_INVALID, "beta %g outside [0, 1]", beta);
    const uint32_t thr = (uint32_t)std::floor(beta * 16777216.0);   // 0 .. 2^24; u24 < 2^24 always
    hipLaunchKernelGGL(dagger_mix_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, policy,
                       expert, dist, N, thr, mix_seed, t_global, (uint64_t)agent_id_base, executed, took_expert,
                       label_weight);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // extern "C"
