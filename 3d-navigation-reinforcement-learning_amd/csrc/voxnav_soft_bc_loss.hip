// voxnav_soft_bc_loss.hip -- the distance-weighted DAgger warm start's kernels
// (f32): vn_bc_loss / vn_bc_loss_set (voxnav_bc_loss.hip) with the planner's
// distance through every first action in place of the label
// (vn_bc_loss_soft), the same with invalid-action masking
// (vn_bc_loss_soft_masked), and vn_dagger_mix with the policy's own sample
// executed wherever it is among the shortest actions (vn_dagger_mix_best).
//
// The target (include/voxnav.h states it once; this is the same text).  Sample
// i has distances d_ik = dists[r ldd + k], k < A (vn_plan_frontier_dists:
// positive = path length through first action k, -1 unreached, -2 not
// passable), r its row through src; tau is finite and > 0:
//   P_i      = {k < A : d_ik > 0};  labelled iff P_i is not empty and w_i != 0
//   d*_i     = min over P_i,  delta_ik = d_ik - d*_i
//   w_ik     = 1 where delta_ik = 0, else expf(-delta_ik / tau)   (k in P_i), 0 outside P_i
//   q_ik     = w_ik / sum_k w_ik
//   kl_i     = sum_{k in P_i} q_ik (ln q_ik - lp_ik),  ln q_ik = -delta_ik / tau - ln sum_k w_ik,
//              a term whose q_ik is 0 being 0
//   loss     = (1/max(n,1)) sum_{i labelled} kl_i + the entropy and value terms of vn_bc_loss
//   dz_ij    = (w_i / max(n,1)) (p_ij - q_ij) + the entropy term of vn_bc_loss
//   accuracy : the argmax (lowest index on ties) has delta = 0
// KL(q || pi) has the cross-entropy's gradient and a floor of 0 at every tau;
// with a singleton P_i it is vn_bc_loss's cross-entropy.  tau -> 0+ gives the
// uniform distribution on the shortest actions (delta / tau overflows, w = 0),
// a large tau the uniform distribution on P_i (every w = 1): no tau gives a
// NaN or an inf.
//
// The masked form runs the softmax over S_i = (mask_i & full) | L_i with
// L_i = P_i where the sample is labelled (BcMasked<BcSoft>,
// masked_bc_objective.h): every action the target gives mass to is allowed, so
// the KL never reads a log-probability outside the support, and dz is exactly
// 0 outside S_i.  With every S_i full the outputs are the unmasked entry's bits.
//
// Launches, as vn_bc_loss_set's: (1) bc_soft_count_kernel, 64 blocks (n
// depends on the distances, so it always runs); (2) head_loss_kernel<Q, AM,
// BcSoft>; (3) the reduce kernel.  Plain stores, fixed orders: two calls on the
// same inputs give the same bits.  Workspaces: vn_bc_loss_part_floats.
//
// HBM per sample: vn_bc_loss_set's + 4 A B (the distance row) - 1 B (no set).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bc_objective.h"
#include "head_loss.h"
#include "masked_bc_objective.h"
#include "soft_bc_objective.h"
#include "vn_common.h"

using vn_detail::fail;
using vn_detail::philox_word0;

namespace {

// vn_dagger_mix's draw; the planner's action is executed only where the
// policy's own sample is not among the shortest actions.  One thread per
// agent; executed may be the policy array itself: each thread reads its
// element before it writes it.
__global__ __launch_bounds__(256) void dagger_mix_best_kernel(const int32_t *policy,
                                                              const int32_t *__restrict__ expert,
                                                              const int32_t *__restrict__ dist,
                                                              const uint8_t *__restrict__ best, int N, uint32_t thr,
                                                              uint64_t seed, uint64_t t, uint64_t gid_base,
                                                              int32_t *executed, uint8_t *__restrict__ took,
                                                              uint8_t *__restrict__ weight,
                                                              uint8_t *__restrict__ own_best) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint32_t u24 = philox_word0(seed, gid_base + (uint64_t)i, t | (1ull << 63)) >> 8;
    const bool lab = dist[i] != -1;
    const int32_t pa = policy[i];
    const bool own = lab && (uint32_t)pa < 8u && (((uint32_t)best[i] >> pa) & 1u) != 0u;
    const bool tk = lab && u24 < thr && !own;
    executed[i] = tk ? expert[i] : pa;
    took[i] = tk ? 1 : 0;
    weight[i] = lab ? 1 : 0;
    own_best[i] = own ? 1 : 0;
}

// vn_bc_loss_soft (Obj = BcSoft; mask unused) and vn_bc_loss_soft_masked (BcMasked<BcSoft>)
template <class Obj>
int bc_soft_launch(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                   const float *bv, const int64_t *src, const int32_t *dists, int64_t ldd, const uint8_t *weight,
                   const uint8_t *mask, bool masked, const float *returns, int32_t M, int32_t F, int32_t A, float tau,
                   float ent_coef, float vf_coef, float *dhp, float *dhv, float *grad_heads, double *stats,
                   float *part, double *spart, void *stream, Obj obj) {
    if (const int e = head_loss::check_args(!hp || !hv || !wa || !ba || !wv || !bv || !dists || (masked && !mask) ||
                                                !returns || !dhp || !dhv || !grad_heads || !stats || !part || !spart,
                                            M, F, A, ldh))
        return e;
    if (const int e = check_soft_args(ldd, A, tau)) return e;
    const hipStream_t s = (hipStream_t)stream;
    obj.dists = dists;
    obj.ldd = ldd;
    obj.tau = tau;
    obj.wgt = weight;
    // the labelled counts sit behind the blocks' sums in spart, as in voxnav_bc_loss.hip; the
    // count depends on the distances (not on the masks): always counted
    int64_t *cnt = reinterpret_cast<int64_t *>(spart + head_loss::blocks(M) * BcSoft::kStats);
    obj.cnt = cnt;
    obj.counted = 1;
    hipLaunchKernelGGL(bc_soft_count_kernel, dim3(kCntBlocks), dim3(256), 0, s, dists, ldd, weight, src, M, A, cnt);
    const head_loss::HeadArgs g{hp,  hv,  ldh,  wa,    ba, wv, bv, src, returns,
                                dhp, dhv, part, spart, M,  F,  A,  ent_coef, vf_coef};
    head_loss::launch(g, obj, grad_heads, stats, s);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace

extern "C" {

int vn_bc_loss_soft(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                    const float *bv, const int64_t *src, const int32_t *dists, int64_t ldd, const uint8_t *weight,
                    const float *returns, int32_t M, int32_t F, int32_t A, float tau, float ent_coef, float vf_coef,
                    float *dhp, float *dhv, float *grad_heads, double *stats, float *part, double *spart,
                    void *stream) {
    return bc_soft_launch(hp, hv, ldh, wa, ba, wv, bv, src, dists, ldd, weight, nullptr, false, returns, M, F, A, tau,
                          ent_coef, vf_coef, dhp, dhv, grad_heads, stats, part, spart, stream, BcSoft{});
}

int vn_bc_loss_soft_masked(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                           const float *wv, const float *bv, const int64_t *src, const int32_t *dists, int64_t ldd,
                           const uint8_t *weight, const uint8_t *mask, const float *returns, int32_t M, int32_t F,
                           int32_t A, float tau, float ent_coef, float vf_coef, float *dhp, float *dhv,
                           float *grad_heads, double *stats, float *part, double *spart, void *stream) {
    BcMasked<BcSoft> obj{};
    obj.mask = mask;
    return bc_soft_launch(hp, hv, ldh, wa, ba, wv, bv, src, dists, ldd, weight, mask, true, returns, M, F, A, tau,
                          ent_coef, vf_coef, dhp, dhv, grad_heads, stats, part, spart, stream, obj);
}

int vn_dagger_mix_best(const int32_t *policy, const int32_t *expert, const int32_t *dist, const uint8_t *best,
                       int32_t N, double beta, uint64_t mix_seed, uint64_t t_global, int64_t agent_id_base,
                       int32_t *executed, uint8_t *took_expert, uint8_t *label_weight, uint8_t *own_best,
                       void *stream) {
    if (!policy || !expert || !dist || !best || !executed || !took_expert || !label_weight || !own_best)
        return fail(VN_ERR_INVALID, "NULL argument");
    if (N < 1) return fail(VN_ERR_INVALID, "bad size N=%d", N);
    if (!(beta >= 0.0 && beta <= 1.0)) return fail(VN_ERR_INVALID, "beta %g outside [0, 1]", beta);
    const uint32_t thr = (uint32_t)std::floor(beta * 16777216.0);   // 0 .. 2^24; u24 < 2^24 always
    hipLaunchKernelGGL(dagger_mix_best_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       policy, expert, dist, best, N, thr, mix_seed, t_global, (uint64_t)agent_id_base, executed,
                       took_expert, label_weight, own_best);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // extern "C"
