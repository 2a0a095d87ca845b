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
// same bits.  head_loss.h has the kernels' tiling and their LDS layout; this
// unit has what is BC's: the labelled count and the two cross-entropy
// objectives.
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

#include "head_loss.h"
#include "vn_common.h"

using vn_detail::fail;
using vn_detail::philox_word0;

namespace {

constexpr int kCntBlocks = 64; // blocks of the labelled count

// per-block counts of the minibatch's labelled samples (kCntBlocks blocks, a
// contiguous range each): integers, so their sum is exact in any order.  SET
// (label sets): a sample counts when its set has a bit below A and its weight,
// if any, is nonzero; else when its weight (given) is nonzero.
template <bool SET>
__global__ __launch_bounds__(256) void bc_count_kernel(const uint8_t *__restrict__ set,
                                                       const uint8_t *__restrict__ wgt,
                                                       const int64_t *__restrict__ src, int M, uint32_t amask,
                                                       int64_t *__restrict__ cnt) {
    __shared__ int s[256];
    const int t = threadIdx.x;
    const int per = (M + kCntBlocks - 1) / kCntBlocks;
    const int i0 = blockIdx.x * per, i1 = min(M, i0 + per);
    int c = 0;
    for (int i = i0 + t; i < i1; i += 256) {
        const int64_t r = src ? src[i] : i;
        if constexpr (SET) c += ((set[r] & amask) != 0u && (wgt == nullptr || wgt[r] != 0)) ? 1 : 0;
        else c += wgt[r] != 0 ? 1 : 0;
    }
    s[t] = c;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) s[t] += s[t + h];
        __syncthreads();
    }
    if (t == 0) cnt[blockIdx.x] = s[0];
}

// What the two cross-entropy objectives share (head_loss.h: what an objective
// supplies).  f64 sums per block: cross-entropy, squared value error, entropy,
// correct argmax.
struct BcCommon {
    static constexpr int kStats = 4;
    const uint8_t *wgt;         // 1 = labelled (NULL: all)
    const int64_t *cnt;         // [kCntBlocks] labelled counts (read when counted)
    int counted;                // launch (1) ran: weights, or label sets
    struct Block {
        float inv_l;            // 1 / max(n, 1) with n the labelled count
    };

    // the labelled count n of the minibatch (M when nothing was counted)
    __device__ __forceinline__ int64_t labelled(int M) const {
        if (!counted) return M;
        int64_t n = 0;
        for (int b = 0; b < kCntBlocks; ++b) n += cnt[b];
        return n;
    }
    // (every thread folds the same 64 integers; the loads are uniform over the block)
    __device__ __forceinline__ Block begin(int M) const {
        const int64_t n_lab = labelled(M);
        return {1.0f / (float)(n_lab > 0 ? n_lab : 1)};
    }
    // stats [6] = cross-entropy, value loss, entropy loss, loss, accuracy, labelled share
    __device__ __forceinline__ void finish(const double *v, int M, float ent_coef, float vf_coef,
                                           double *stats) const {
        const int64_t nl = labelled(M);
        const double n = M, dl = (double)(nl > 0 ? nl : 1);
        const double ce = v[0] / dl, vl = v[1] / n, el = -v[2] / n;
        stats[0] = ce;
        stats[1] = vl;
        stats[2] = el;
        stats[3] = ce + (double)ent_coef * el + (double)vf_coef * vl;
        stats[4] = v[3] / dl;
        stats[5] = (double)nl / n;
    }
};

// vn_bc_loss: one expert action per sample
struct BcLabel : BcCommon {
    const int32_t *lab;
    struct Sample {
        int lab;
        bool has;
        float lp, gce;          // policy(): the label's log-probability, the cross-entropy's gradient scale
    };
    __device__ __forceinline__ Sample gather(const Block &, int64_t r, int) const {
        Sample s;
        s.lab = lab[r];
        s.has = wgt ? wgt[r] != 0 : true;
        return s;
    }
    template <int AM>
    __device__ __forceinline__ void policy(const Block &b, Sample &s, const head_loss::Forward<AM> &f, bool ok, float,
                                           float) const {
        s.lp = 0.0f;
#pragma unroll
        for (int a = 0; a < AM; ++a) s.lp = a == s.lab ? f.lpa[a] : s.lp;
        s.gce = (s.has && ok) ? b.inv_l : 0.0f;
    }
    template <int AM>
    __device__ __forceinline__ float dz(const Sample &s, const head_loss::Forward<AM> &f, int a) const {
        return s.gce * (f.p[a] - (a == s.lab ? 1.0f : 0.0f));
    }
    template <int AM>
    __device__ __forceinline__ void stats(const Sample &s, const head_loss::Forward<AM> &f, double *st) const {
        st[0] += s.has ? (double)(-s.lp) : 0.0;
        st[3] += (s.has && f.amax == s.lab) ? 1.0 : 0.0;
    }
};

// vn_bc_loss_set: a set of equally good actions per sample (a uint8 bit set);
// the target of the cross-entropy is the softmax restricted to the set, and a
// sample with an empty set is unlabelled
struct BcSet : BcCommon {
    const uint8_t *lab;         // the label sets
    struct Sample {
        uint32_t S;             // the label set, bits below A
        bool has;
        float lp, gce;          // policy(): the whole set's log-probability, the gradient scale
        float q[head_loss::kMaxA];   // policy(): the target distribution
    };
    __device__ __forceinline__ Sample gather(const Block &, int64_t r, int A) const {
        Sample s;
        s.S = (uint32_t)lab[r] & ((1u << A) - 1u);
        s.has = wgt ? wgt[r] != 0 : true;
        s.has = s.has && s.S != 0u;
        return s;
    }
    template <int AM>
    __device__ __forceinline__ void policy(const Block &b, Sample &s, const head_loss::Forward<AM> &f, bool ok, float,
                                           float) const {
        const uint32_t S = s.S;
        // logsumexp over S around S's own maximum: a set far below the top logit keeps its digits
        float zs = -INFINITY, ses = 0.0f;
#pragma unroll
        for (int a = 0; a < AM; ++a) zs = ((S >> a) & 1u) ? fmaxf(zs, f.z[a]) : zs;
#pragma unroll
        for (int a = 0; a < AM; ++a) {
            s.q[a] = ((S >> a) & 1u) ? expf(f.z[a] - zs) : 0.0f;
            ses += s.q[a];
        }
        const float inv_s = S != 0u ? 1.0f / ses : 0.0f;
#pragma unroll
        for (int a = 0; a < AM; ++a) s.q[a] *= inv_s;
        s.lp = S != 0u ? (zs + logf(ses)) - (f.zmax + f.lse) : 0.0f;
        s.gce = (s.has && ok) ? b.inv_l : 0.0f;
    }
    template <int AM>
    __device__ __forceinline__ float dz(const Sample &s, const head_loss::Forward<AM> &f, int a) const {
        return s.gce * (f.p[a] - s.q[a]);
    }
    template <int AM>
    __device__ __forceinline__ void stats(const Sample &s, const head_loss::Forward<AM> &f, double *st) const {
        st[0] += s.has ? (double)(-s.lp) : 0.0;
        st[3] += (s.has && ((s.S >> f.amax) & 1u) != 0u) ? 1.0 : 0.0;
    }
};

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
