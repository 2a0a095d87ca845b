// voxnav_ppo_loss.hip -- the PPO learner's per-minibatch kernels around the
// matrix products (f32, the reference's dtype): the loss and its gradient down
// to the MLP latents in three launches, the gradient norm of the clip, the Adam
// step, and the feed-forward minibatch gather (each below its own header).
//
// Restates, per minibatch, what sb3 RecurrentPPO.train / PPO.train run after
// the MLP extractor (train/Grid_Train.py:228 -> model.learn; SURVEY.md App.
// D.3/D.4): the heads (action_net Linear -> Categorical, value_net Linear),
// the advantage normalisation, the clipped surrogate, the value MSE and the
// entropy bonus, and -- instead of autograd -- their gradient written
// directly:
//   z = h_pi Wa^T + ba,  lp_all = log_softmax(z),  v = h_vf wv + bv
//   H = -sum p lp_all,   ratio = exp(lp_all[a] - old_lp)
//   loss = -mean(min(A r, A clamp(r, 1-c, 1+c))) - ent_coef mean(H)
//          + vf_coef mean((ret - v)^2)
//   dz_j = g_lp (d_ja - p_j) + (ent_coef / n) p_j (lp_j + H)
//   g_lp = -(1/n) A r (m1 + m2 [1-c <= r <= 1+c])      (torch's min / clamp
//          backward: the smaller branch, a tie split in halves)
//   dv   = vf_coef 2 (v - ret) / n
//   dh_pi = dz Wa, dh_vf = dv wv, dWa = dz^T h_pi, dba = sum dz, dwv, dbv
// with A = (adv - mean) / (std + 1e-8) over the minibatch (unbiased std).
//
// Launches: (1) 64 blocks: f64 sums of the minibatch's advantages and their
// squares (each loss block folds the 64 pairs, in order, into mean / std);
// (2) the samples, head_loss_kernel<Q, AM, PpoClip>; (3) the partials summed
// in a fixed order, head_loss_reduce_kernel<PpoClip> (results do not depend on
// scheduling).  head_loss.h has the kernels' tiling and their LDS layout;
// ppo_objective.h has what is PPO's: the advantage sums and the
// clipped-surrogate objective (voxnav_ppo_bc_loss.hip composes it too).
//
// HBM per sample: the two latent rows read (2 F 4 B) and their gradient rows
// written (2 F 4 B) + 16 B of gathered buffer scalars + the 8 B row index.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "head_loss.h"
#include "ppo_objective.h"
#include "vn_common.h"

using vn_detail::fail;

namespace {

// ---- gradient clipping (torch.nn.utils.clip_grad_norm_, sb3 max_grad_norm) ----
// The total 2-norm over every parameter gradient (f64 sums: per-block
// partials over all tensors, then one block in a fixed order) and the
// divisor the fused Adam step applies to the gradients (its grad_scale):
// max(1, (norm + 1e-6) / max_norm) = 1 / clip_grad_norm_'s clamped coefficient.
constexpr int kMaxGradTensors = 64;
constexpr int kNormBlocks = 256;

struct GradList {
    const float *p[kMaxGradTensors];
    int64_t n[kMaxGradTensors];
    int count;
};

__global__ __launch_bounds__(256) void grad_sq_kernel(GradList gl, double *__restrict__ part) {
    __shared__ double sr[256];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int k = 0; k < gl.count; ++k) {
        const float *g = gl.p[k];
        const int64_t n = gl.n[k];
        const int64_t n4 = ((((uintptr_t)g) & 15) == 0) ? n / 4 : 0;
        for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < n4; i += (int64_t)gridDim.x * 256) {
            const float4 v = reinterpret_cast<const float4 *>(g)[i];
            acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
        for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + t; i < n; i += (int64_t)gridDim.x * 256)
            acc += (double)g[i] * g[i];
    }
    sr[t] = acc;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) sr[t] += sr[t + h];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = sr[0];
}

__global__ __launch_bounds__(256) void grad_norm_kernel(const double *__restrict__ part, float max_norm,
                                                        float *__restrict__ norm, float *__restrict__ scale) {
    __shared__ double sr[256];
    const int t = threadIdx.x;
    sr[t] = part[t];
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) sr[t] += sr[t + h];
        __syncthreads();
    }
    if (t == 0) {
        const float nv = (float)sqrt(sr[0]);
        norm[0] = nv;
        scale[0] = fmaxf(1.0f, (nv + 1e-6f) / max_norm);
    }
}

// ---- Adam step (torch.optim.Adam, the update sb3's policy optimizer runs) ----
// One launch over every parameter (pointers by value): with the clip divisor
// s (vn_grad_norm; 1 when NULL) and the step's bias corrections from the host,
// per element, in torch's fused-Adam order:
//   g = grad / s;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g
//   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// The gradients are read, not rewritten (the learner drops them after the step).
// A gated step (skip and the step counters both given) counts on the device:
// adam_count_kernel advances the counters first, only when the step is
// applied, and adam_kernel takes the step number from counter 0 -- when steps
// were skipped before, the host's number runs ahead of it, and the bias
// corrections are then formed here from the applied count.
struct AdamList {
    float *p[kMaxGradTensors];
    const float *g[kMaxGradTensors];
    float *m[kMaxGradTensors];
    float *v[kMaxGradTensors];
    float *step[kMaxGradTensors];   // torch's per-parameter step counters (device f32 scalars)
    int64_t n[kMaxGradTensors];
    int count;
};

__global__ __launch_bounds__(64) void adam_count_kernel(AdamList al, const int32_t *__restrict__ skip) {
    if (skip[0] != 0) return;
    const int k = threadIdx.x;
    if (k < al.count && al.step[k]) al.step[k][0] += 1.0f;
}

__global__ __launch_bounds__(256) void adam_kernel(AdamList al, const float *__restrict__ scale,
                                                   const int32_t *__restrict__ skip, float lr, float b1, float b2,
                                                   float eps, float bc1, float bc2_sqrt, float step_value,
                                                   int device_count) {
    if (skip && skip[0] != 0) return;   // gradients from a failed launch: leave every tensor as it was
    const bool div = scale != nullptr;
    const float s = scale ? scale[0] : 1.0f;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (device_count) {
        // counter 0 was advanced by adam_count_kernel and is only read in this launch
        const float t = al.step[0][0];
        if (t != step_value) {
            bc1 = (float)(1.0 - pow((double)b1, (double)t));
            bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, (double)t));
        }
    } else if (gid < al.count && al.step[gid]) {
        al.step[gid][0] = step_value;
    }
    const float step_size = lr / bc1;
    auto upd = [&](float &pp, float g, float &mm, float &vv) {
        if (div) g = g / s;
        mm = b1 * mm + (1.0f - b1) * g;
        vv = b2 * vv + (1.0f - b2) * g * g;
        const float denom = sqrtf(vv) / bc2_sqrt + eps;
        pp = pp - step_size * (mm / denom);
    };
    for (int k = 0; k < al.count; ++k) {
        const int64_t n = al.n[k];
        float *P = al.p[k], *M = al.m[k], *V = al.v[k];
        const float *G = al.g[k];
        const bool vec = ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)M) | ((uintptr_t)V)) & 15) == 0;
        const int64_t n4 = vec ? n / 4 : 0;
        for (int64_t i = gid; i < n4; i += stride) {
            float4 pp = reinterpret_cast<float4 *>(P)[i], mm = reinterpret_cast<float4 *>(M)[i],
                   vv = reinterpret_cast<float4 *>(V)[i];
            const float4 gg = reinterpret_cast<const float4 *>(G)[i];
            upd(pp.x, gg.x, mm.x, vv.x);
            upd(pp.y, gg.y, mm.y, vv.y);
            upd(pp.z, gg.z, mm.z, vv.z);
            upd(pp.w, gg.w, mm.w, vv.w);
            reinterpret_cast<float4 *>(P)[i] = pp;
            reinterpret_cast<float4 *>(M)[i] = mm;
            reinterpret_cast<float4 *>(V)[i] = vv;
        }
        for (int64_t i = 4 * n4 + gid; i < n; i += stride) upd(P[i], G[i], M[i], V[i]);
    }
}

// ---- minibatch gather (PPO.train: rollout_buffer.get(batch_size) on the
// swap_and_flatten'ed, env-major buffer) ----
// sample i of the minibatch is env-major flat id idx[i] = env * T + t; its row
// in the collector's [T, N]-major buffers is t * N + env.  One block per 16
// samples: the rows (src) and the observation rows copied, 16 B per lane.
__global__ __launch_bounds__(256) void minibatch_rows_kernel(const int64_t *__restrict__ idx, int M, int T, int N,
                                                             const float *__restrict__ obs, int D,
                                                             float *__restrict__ out, int64_t *__restrict__ src) {
    const int lane = threadIdx.x & 15, s = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (s >= M) return;
    const int64_t id = idx[s];
    const int64_t env = id / T, t = id - env * T;
    const int64_t r = t * N + env;
    if (lane == 0) src[s] = r;
    const float4 *in = reinterpret_cast<const float4 *>(obs + r * D);
    float4 *o = reinterpret_cast<float4 *>(out + (int64_t)s * D);
    for (int c = lane; c < D / 4; c += 16) o[c] = in[c];
}
}  // namespace

extern "C" {

int vn_ppo_loss_part_floats(int32_t M, int32_t F, int32_t A, int64_t *n_part, int64_t *n_spart) {
    return head_loss::part_floats(M, F, A, PpoClip::kStats, 2 * kAdvBlocks /* the advantage sums */, n_part, n_spart);
}

int vn_ppo_loss(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                const float *bv, const int64_t *src, const int32_t *actions, const float *advantages,
                const float *old_log_prob, const float *returns, int32_t M, int32_t F, int32_t A, float clip_range,
                float ent_coef, float vf_coef, int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads,
                double *stats, double *adv_sums, float *part, double *spart, void *stream) {
    if (const int e = head_loss::check_args(!hp || !hv || !wa || !ba || !wv || !bv || !actions || !advantages ||
                                                !old_log_prob || !returns || !dhp || !dhv || !grad_heads || !stats ||
                                                !adv_sums || !part || !spart,
                                            M, F, A, ldh))
        return e;
    const hipStream_t s = (hipStream_t)stream;
    if (normalize_advantage)
        hipLaunchKernelGGL(adv_sum_kernel, dim3(kAdvBlocks), dim3(256), 0, s, advantages, src, M, adv_sums);
    const head_loss::HeadArgs g{hp,  hv,  ldh,  wa,    ba, wv, bv, src, returns,
                                dhp, dhv, part, spart, M,  F,  A,  ent_coef, vf_coef};
    const PpoClip obj{actions, advantages, old_log_prob, adv_sums, normalize_advantage, clip_range};
    head_loss::launch(g, obj, grad_heads, stats, s);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int vn_grad_norm(const float *const *grads, const int64_t *sizes, int32_t count, float max_norm, float *norm,
                 float *scale, double *work, void *stream) {
    if (!grads || !sizes || !norm || !scale || !work) return fail(VN_ERR_INVALID, "NULL argument");
    if (count < 1 || count > kMaxGradTensors)
        return fail(VN_ERR_INVALID, "gradient count %d outside 1..%d", count, kMaxGradTensors);
    if (!(max_norm > 0.0f)) return fail(VN_ERR_INVALID, "max_norm must be > 0");
    GradList gl{};
    gl.count = count;
    for (int k = 0; k < count; ++k) {
        if (!grads[k] || sizes[k] < 0) return fail(VN_ERR_INVALID, "gradient %d: NULL or negative size", k);
        gl.p[k] = grads[k];
        gl.n[k] = sizes[k];
    }
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(grad_sq_kernel, dim3(kNormBlocks), dim3(256), 0, s, gl, work);
    hipLaunchKernelGGL(grad_norm_kernel, dim3(1), dim3(256), 0, s, work, max_norm, norm, scale);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int vn_adam_step(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                 float *const *steps, const int64_t *sizes, int32_t count, const float *clip_scale,
                 const int32_t *skip, float lr, float beta1, float beta2, float eps, int64_t step, void *stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !sizes) return fail(VN_ERR_INVALID, "NULL argument");
    if (count < 1 || count > kMaxGradTensors)
        return fail(VN_ERR_INVALID, "parameter count %d outside 1..%d", count, kMaxGradTensors);
    if (step < 1) return fail(VN_ERR_INVALID, "step must be >= 1");
    AdamList al{};
    al.count = count;
    int64_t total = 0;
    for (int k = 0; k < count; ++k) {
        if (!params[k] || !grads[k] || !exp_avg[k] || !exp_avg_sq[k] || sizes[k] < 0)
            return fail(VN_ERR_INVALID, "parameter %d: NULL or negative size", k);
        al.p[k] = params[k];
        al.g[k] = grads[k];
        al.m[k] = exp_avg[k];
        al.v[k] = exp_avg_sq[k];
        al.step[k] = steps ? steps[k] : nullptr;
        al.n[k] = sizes[k];
        total += sizes[k];
    }
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    int blocks = (int)((total / 4 + 255) / 256);
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    // gated with counters: the step number is the device's (every counter given, as the launch reads counter 0)
    int device_count = skip && steps ? 1 : 0;
    for (int k = 0; device_count && k < count; ++k)
        if (!al.step[k]) device_count = 0;
    if (device_count)
        hipLaunchKernelGGL(adam_count_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, al, skip);
    hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, al, clip_scale, skip, lr, beta1,
                       beta2, eps, (float)bc1, (float)sqrt(bc2), (float)step, device_count);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int vn_minibatch_rows(const int64_t *idx, int32_t M, int32_t T, int32_t N, const float *obs, int32_t D, float *out,
                      int64_t *src, void *stream) {
    if (!idx || !obs || !out || !src) return fail(VN_ERR_INVALID, "NULL argument");
    if (M < 1 || T < 1 || N < 1 || D < 4 || D % 4) return fail(VN_ERR_INVALID, "bad sizes M=%d T=%d N=%d D=%d", M, T, N, D);
    if ((((uintptr_t)obs) | ((uintptr_t)out)) & 15) return fail(VN_ERR_INVALID, "obs / out must be 16-B aligned");
    hipLaunchKernelGGL(minibatch_rows_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, (hipStream_t)stream, idx,
                       M, T, N, obs, D, out, src);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // extern "C"
