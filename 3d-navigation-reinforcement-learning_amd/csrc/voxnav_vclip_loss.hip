// voxnav_vclip_loss.hip -- vn_ppo_loss / vn_ppo_loss_masked with the value
// update clipped (sb3 PPO.train / RecurrentPPO.train with clip_range_vf):
// with old_i the value the rollout stored for the sample, c = clip_range_vf and
//   lo_i = old_i - c,  hi_i = old_i + c            (formed in f32)
//   v'_i = min(max(v_i, lo_i), hi_i)
//   value loss = (1/M) sum_i (ret_i - v'_i)^2
//   dv_i = 2 vf_coef (v'_i - ret_i) / M  where lo_i <= v_i <= hi_i, exactly 0 elsewhere
// (the bounds inclusive, as torch.clamp's backward).  In exact arithmetic this
// is sb3's old + clamp(v - old, -c, c); this form is taken because inside the
// range v' is v bit for bit, so c = +inf gives the unclipped entry's outputs.
// Everything else -- the policy term, the masked softmax, stats [6], the
// workspaces and the launches -- is voxnav_ppo_loss.hip's / voxnav_masked_loss.hip's.
//
// The objectives are PpoClip (ppo_objective.h) and its masked form with the
// sample's old value added, which head_loss.h's kernel takes as the
// compile-time trait kValueClip: the clipped value term is instantiated in
// this unit only.  HBM per sample: 4 B more than the unclipped entry's.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "head_loss.h"
#include "ppo_objective.h"
#include "vn_common.h"

namespace {

// PpoClip with each sample's allowed set (voxnav_masked_loss.hip states the rule)
struct PpoClipAllowed : PpoClip {
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

// Base with the value term clipped round the sample's old value
template <class Base>
struct ValueClipped : Base {
    static constexpr bool kValueClip = true;
    const float *old_v;         // [rows] the rollout's values
    float cvf;                  // clip_range_vf
    struct Sample : Base::Sample {
        float old;
    };
    __device__ __forceinline__ Sample gather(const typename Base::Block &b, int64_t r, int A) const {
        Sample s;
        static_cast<typename Base::Sample &>(s) = Base::gather(b, r, A);
        s.old = old_v[r];
        return s;
    }
    // comparisons, not fmin / fmax: inside the range the result is v itself
    __device__ __forceinline__ head_loss::ClippedValue value_clip(const Sample &s, float v) const {
        const float lo = s.old - cvf, hi = s.old + cvf;
        return {v < lo ? lo : (v > hi ? hi : v), lo <= v && v <= hi};
    }
};

int check_vclip(const float *old_values, float clip_range_vf) {
    if (!old_values) return vn_detail::fail(VN_ERR_INVALID, "NULL argument");
    if (!(clip_range_vf > 0.0f))   // also NaN
        return vn_detail::fail(VN_ERR_INVALID, "clip_range_vf must be > 0 (+inf: no clip)");
    return VN_OK;
}

}  // namespace

extern "C" {

int vn_ppo_loss_vclip(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                      const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                      const float *advantages, const float *old_log_prob, const float *returns,
                      const float *old_values, int32_t M, int32_t F, int32_t A, float clip_range, float clip_range_vf,
                      float ent_coef, float vf_coef, int32_t normalize_advantage, float *dhp, float *dhv,
                      float *grad_heads, double *stats, double *adv_sums, float *part, double *spart, void *stream) {
    if (const int e = head_loss::check_args(!hp || !hv || !wa || !ba || !wv || !bv || !actions || !advantages ||
                                                !old_log_prob || !returns || !dhp || !dhv || !grad_heads || !stats ||
                                                !adv_sums || !part || !spart,
                                            M, F, A, ldh))
        return e;
    if (const int e = check_vclip(old_values, clip_range_vf)) return e;
    const hipStream_t s = (hipStream_t)stream;
    if (normalize_advantage)
        hipLaunchKernelGGL(adv_sum_kernel, dim3(kAdvBlocks), dim3(256), 0, s, advantages, src, M, adv_sums);
    const head_loss::HeadArgs g{hp,  hv,  ldh,  wa,    ba, wv, bv, src, returns,
                                dhp, dhv, part, spart, M,  F,  A,  ent_coef, vf_coef};
    ValueClipped<PpoClip> obj;
    static_cast<PpoClip &>(obj) = PpoClip{actions, advantages, old_log_prob, adv_sums, normalize_advantage, clip_range};
    obj.old_v = old_values;
    obj.cvf = clip_range_vf;
    head_loss::launch(g, obj, grad_heads, stats, s);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

int vn_ppo_loss_masked_vclip(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba,
                             const float *wv, const float *bv, const int64_t *src, const int32_t *actions,
                             const float *advantages, const float *old_log_prob, const float *returns,
                             const uint8_t *mask, const float *old_values, int32_t M, int32_t F, int32_t A,
                             float clip_range, float clip_range_vf, float ent_coef, float vf_coef,
                             int32_t normalize_advantage, float *dhp, float *dhv, float *grad_heads, double *stats,
                             double *adv_sums, float *part, double *spart, void *stream) {
    if (const int e = head_loss::check_args(!hp || !hv || !wa || !ba || !wv || !bv || !actions || !advantages ||
                                                !old_log_prob || !returns || !mask || !dhp || !dhv || !grad_heads ||
                                                !stats || !adv_sums || !part || !spart,
                                            M, F, A, ldh))
        return e;
    if (const int e = check_vclip(old_values, clip_range_vf)) return e;
    const hipStream_t s = (hipStream_t)stream;
    if (normalize_advantage)
        hipLaunchKernelGGL(adv_sum_kernel, dim3(kAdvBlocks), dim3(256), 0, s, advantages, src, M, adv_sums);
    const head_loss::HeadArgs g{hp,  hv,  ldh,  wa,    ba, wv, bv, src, returns,
                                dhp, dhv, part, spart, M,  F,  A,  ent_coef, vf_coef};
    ValueClipped<PpoClipAllowed> obj;
    static_cast<PpoClip &>(obj) = PpoClip{actions, advantages, old_log_prob, adv_sums, normalize_advantage, clip_range};
    obj.mask = mask;
    obj.old_v = old_values;
    obj.cvf = clip_range_vf;
    head_loss::launch(g, obj, grad_heads, stats, s);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // extern "C"
