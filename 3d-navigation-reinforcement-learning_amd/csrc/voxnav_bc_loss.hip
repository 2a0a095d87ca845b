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
// order; the count never leaves the device); (2) the samples, laid out as
// ppo_loss_kernel: one wave per kSPW samples, 16 lanes per sample across the
// latent features (a float4 each), the head dot products reduced over the 16
// lanes by xor butterflies, the action weights in LDS, per-block partials of
// the head gradients (f32) and of the logged sums (f64); (3) the partials
// summed in a fixed order, so two calls on the same inputs give the same bits.
//
// vn_bc_loss_set is the same call with a set of equally good actions per
// sample (a uint8 bit set) in place of the label:
//   S = set & (2^A - 1);  labelled iff S != 0 and w != 0
//   ce = logsumexp_j z_j - logsumexp_{j in S} z_j,  q = softmax of z restricted to S
//   dz_ij = (w_i / max(n,1)) (p_ij - q_ij) + the entropy term above
// through bc_loss_kernel<.., SET = true>; its labelled count depends on the
// sets, so launch (1) always runs (bc_count_set_kernel).
//
// All LDS is in the dynamic region and every carve offset is a multiple of
// 16 B: the float4 reads of the action weights and the float4 stores of the
// per-wave head-gradient rows stay on their natural alignment.
//
// HBM per sample: the two latent rows read (2 F 4 B) and their gradient rows
// written (2 F 4 B) + 9 B of gathered buffer scalars (label, weight, return)
// + the 8 B row index.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "vn_common.h"

using vn_detail::fail;
using vn_detail::philox_word0;

namespace {

constexpr int kSPW = 32;       // samples per wave
constexpr int kWaves = 4;      // waves per block
constexpr int kMaxA = 8;       // actions
constexpr int kCntBlocks = 64; // blocks of the labelled count
constexpr int kStats = 4;      // per-block f64 sums: cross-entropy, squared value error, entropy, correct argmax

struct BcArgs {
    const float *hp, *hv;       // latents [M][F] (row stride ldh)
    int64_t ldh;
    const float *wa, *ba, *wv, *bv;   // action_net [A][F], [A]; value_net [F], [1]
    const int64_t *src;         // [M] rows of the buffers (NULL: identity)
    const int32_t *lab;         // expert actions
    const uint8_t *wgt;         // 1 = labelled (NULL: all)
    const float *ret;
    const int64_t *cnt;         // [kCntBlocks] labelled counts (read with wgt only)
    float *dhp, *dhv;           // [M][F] contiguous
    float *part;                // [blocks][PG]
    double *spart;              // [blocks][kStats]
    int M, F, A;
    float ent_coef, vf_coef;
};

// per-block counts of the minibatch's labelled samples (kCntBlocks blocks, a
// contiguous range each): integers, so their sum is exact in any order
__global__ __launch_bounds__(256) void bc_count_kernel(const uint8_t *__restrict__ wgt, const int64_t *__restrict__ src,
                                                       int M, int64_t *__restrict__ cnt) {
    __shared__ int s[256];
    const int t = threadIdx.x;
    const int per = (M + kCntBlocks - 1) / kCntBlocks;
    const int i0 = blockIdx.x * per, i1 = min(M, i0 + per);
    int c = 0;
    for (int i = i0 + t; i < i1; i += 256) c += wgt[src ? src[i] : i] != 0 ? 1 : 0;
    s[t] = c;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) s[t] += s[t + h];
        __syncthreads();
    }
    if (t == 0) cnt[blockIdx.x] = s[0];
}

// the same for label sets: a sample counts when its set has a bit below A (and its weight, if any, is nonzero)
__global__ __launch_bounds__(256) void bc_count_set_kernel(const uint8_t *__restrict__ set,
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
        c += ((set[r] & amask) != 0u && (wgt == nullptr || wgt[r] != 0)) ? 1 : 0;
    }
    s[t] = c;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) s[t] += s[t + h];
        __syncthreads();
    }
    if (t == 0) cnt[blockIdx.x] = s[0];
}

// the labelled count n of the minibatch (M without weights)
__device__ __forceinline__ int64_t labelled(const int64_t *cnt, bool weighted, int M) {
    if (!weighted) return M;
    int64_t n = 0;
    for (int b = 0; b < kCntBlocks; ++b) n += cnt[b];
    return n;
}

// LDS row of the head gradients: d Wa [A][F], d wv [F], d ba [A], d bv -- the
// two float4-stored parts first, so both start on 16 B; grad_heads' order is
// d Wa, d ba, d wv, d bv (head_slot maps an output index to its LDS slot)
__device__ __forceinline__ int head_slot(int i, int A, int F) {
    const int AF = A * F;
    if (i < AF) return i;
    if (i < AF + A) return AF + F + (i - AF);
    if (i < AF + A + F) return AF + (i - AF - A);
    return AF + F + A;
}

// Q = F / 64: lane l of a 16-lane group holds latent features
// 64 q + 4 (l & 15) .. +3 (q < Q) -- one float4 per q, 256 B contiguous per
// group; the wave's 4 groups take 4 samples at once.  AM: A rounded up to
// even (the per-action registers); the action weights are read from LDS.
//
// SET (vn_bc_loss_set): g.lab points at the samples' label sets, one uint8
// each, instead of int32 labels (BcArgs and with it vn_bc_loss' kernels stay
// as they were); the target of the cross-entropy is the softmax restricted to
// the set, and a sample with an empty set is unlabelled.
template <int Q, int AM, bool SET>
__global__ __launch_bounds__(256) void bc_loss_kernel(BcArgs g) {
    // action weights [AM][F], then the waves' head-gradient rows [kWaves][PGP],
    // then the waves' f64 sums [kWaves][kStats]
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int grp = lane >> 4, gl = lane & 15;
    const int F = g.F, A = g.A, PG = A * F + A + F + 1, PGP = (PG + 3) & ~3;
    float *wsh = lds;
    float *red = lds + AM * F;
    double *sred = reinterpret_cast<double *>(red + kWaves * PGP);
    for (int i = threadIdx.x; i < AM * F; i += 256) wsh[i] = i < A * F ? g.wa[i] : 0.0f;
    auto wa = [&](int a, int q) { return *reinterpret_cast<const float4 *>(wsh + a * F + 64 * q + 4 * gl); };
    float4 wvv[Q];
    float ba[AM];
#pragma unroll
    for (int a = 0; a < AM; ++a) ba[a] = a < A ? g.ba[a] : 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) wvv[q] = *reinterpret_cast<const float4 *>(g.wv + 64 * q + 4 * gl);
    const float bv = g.bv[0];
    // 1 / max(n, 1) with n the labelled count (every thread folds the same 64
    // integers; the loads are uniform over the block)
    const int64_t n_lab = labelled(g.cnt, SET || g.wgt != nullptr, g.M);
    const float inv_l = 1.0f / (float)(n_lab > 0 ? n_lab : 1);
    const float inv_n = 1.0f / (float)g.M;
    __syncthreads();

    float4 gwa[AM][Q], gwv[Q];
    float gba[AM], gbv = 0.0f;
#pragma unroll
    for (int a = 0; a < AM; ++a) {
        gba[a] = 0.0f;
#pragma unroll
        for (int q = 0; q < Q; ++q) gwa[a][q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) gwv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    double st[kStats] = {0.0, 0.0, 0.0, 0.0};

    auto dot4 = [](float4 x, float4 y) { return x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w; };
    auto fma4 = [](float4 &acc, float s, float4 x) {
        acc.x += s * x.x;
        acc.y += s * x.y;
        acc.z += s * x.z;
        acc.w += s * x.w;
    };
    // sum over the 16 lanes of a group; every lane of the group ends with the same bits
    auto gsum = [](float v) {
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        return v;
    };

    const int s0 = (blockIdx.x * kWaves + wv) * kSPW;
    const int ns = max(0, min(kSPW, g.M - s0));
    for (int j0 = 0; j0 < ns; j0 += 4) {
        // a pass of 4 samples (one per group); a padding group re-reads the wave's first sample
        const int j = j0 + grp;
        const bool ok = j < ns;
        const int64_t row = (int64_t)(s0 + (ok ? j : 0));
        const int64_t r = g.src ? g.src[row] : row;
        float4 hp[Q], hv[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            hp[q] = *reinterpret_cast<const float4 *>(g.hp + row * g.ldh + 64 * q + 4 * gl);
            hv[q] = *reinterpret_cast<const float4 *>(g.hv + row * g.ldh + 64 * q + 4 * gl);
        }
        // keep the LDS weight reads inside the loop (hoisted, they would hold
        // A Q float4 registers for the whole kernel)
        asm volatile("" ::: "memory");
        int lab = 0;
        uint32_t S = 0u;                      // the label set, bits below A
        if constexpr (SET) S = (uint32_t)reinterpret_cast<const uint8_t *>(g.lab)[r] & ((1u << A) - 1u);
        else lab = g.lab[r];
        const float ret = g.ret[r];
        bool has = g.wgt ? g.wgt[r] != 0 : true;
        if constexpr (SET) has = has && S != 0u;
        float z[AM];
#pragma unroll
        for (int a = 0; a < AM; ++a) {
            float sacc = 0.0f;
#pragma unroll
            for (int q = 0; q < Q; ++q) sacc += dot4(hp[q], wa(a, q));
            z[a] = a < A ? gsum(sacc) + ba[a] : -INFINITY;
        }
        float sv = 0.0f;
#pragma unroll
        for (int q = 0; q < Q; ++q) sv += dot4(hv[q], wvv[q]);
        const float v = gsum(sv) + bv;
        // log_softmax, entropy, argmax with ties to the lowest index (uniform over the group)
        float zmax = z[0];
        int amax = 0;
#pragma unroll
        for (int a = 1; a < AM; ++a) {
            amax = z[a] > zmax ? a : amax;
            zmax = fmaxf(zmax, z[a]);
        }
        float se = 0.0f;
#pragma unroll
        for (int a = 0; a < AM; ++a) se += a < A ? expf(z[a] - zmax) : 0.0f;
        const float lse = logf(se);
        float lpa[AM], p[AM], ent = 0.0f;
#pragma unroll
        for (int a = 0; a < AM; ++a) {
            lpa[a] = z[a] - zmax - lse;
            p[a] = a < A ? expf(lpa[a]) : 0.0f;
            ent -= a < A ? p[a] * lpa[a] : 0.0f;
        }
        // lp: the log-probability of the label, or of the whole set; q: the target distribution
        float lp = 0.0f, q[SET ? AM : 1];
        bool hit = false;
        if constexpr (SET) {
            // logsumexp over S around S's own maximum: a set far below the top logit keeps its digits
            float zs = -INFINITY, ses = 0.0f;
#pragma unroll
            for (int a = 0; a < AM; ++a) zs = ((S >> a) & 1u) ? fmaxf(zs, z[a]) : zs;
#pragma unroll
            for (int a = 0; a < AM; ++a) {
                q[a] = ((S >> a) & 1u) ? expf(z[a] - zs) : 0.0f;
                ses += q[a];
            }
            const float inv_s = S != 0u ? 1.0f / ses : 0.0f;
#pragma unroll
            for (int a = 0; a < AM; ++a) q[a] *= inv_s;
            lp = S != 0u ? (zs + logf(ses)) - (zmax + lse) : 0.0f;
            hit = ((S >> amax) & 1u) != 0u;
        } else {
#pragma unroll
            for (int a = 0; a < AM; ++a) lp = a == lab ? lpa[a] : lp;
        }
        const float w = ok ? 1.0f : 0.0f;     // a padding pass contributes nothing
        const float gce = (has && ok) ? inv_l : 0.0f;
        const float gent = g.ent_coef * inv_n * w;
        const float dv = g.vf_coef * 2.0f * (v - ret) * inv_n * w;
        float4 dh[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) dh[q] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int a = 0; a < AM; ++a) {
            if (a >= A) break;
            float dz;
            if constexpr (SET) dz = gce * (p[a] - q[a]) + gent * p[a] * (lpa[a] + ent);
            else dz = gce * (p[a] - (a == lab ? 1.0f : 0.0f)) + gent * p[a] * (lpa[a] + ent);
            gba[a] += dz;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                fma4(dh[q], dz, wa(a, q));
                fma4(gwa[a][q], dz, hp[q]);
            }
        }
        gbv += dv;
        if (ok) {
            const int64_t orow = (int64_t)(s0 + j) * F;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                *reinterpret_cast<float4 *>(g.dhp + orow + 64 * q + 4 * gl) = dh[q];
                *reinterpret_cast<float4 *>(g.dhv + orow + 64 * q + 4 * gl) =
                    make_float4(dv * wvv[q].x, dv * wvv[q].y, dv * wvv[q].z, dv * wvv[q].w);
            }
            if (gl == 0) {
                st[0] += has ? (double)(-lp) : 0.0;
                st[1] += (double)((ret - v) * (ret - v));
                st[2] += (double)ent;
                if constexpr (SET) st[3] += (has && hit) ? 1.0 : 0.0;
                else st[3] += (has && amax == lab) ? 1.0 : 0.0;
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) fma4(gwv[q], dv, hv[q]);
    }
    // the 4 groups' sums (lanes l, l ^ 16, l ^ 32, l ^ 48), then the waves in order
    auto xsum = [](float v) {
        v += __shfl_xor(v, 16, 64);
        return v + __shfl_xor(v, 32, 64);
    };
    float *my = red + wv * PGP;
    const int AF = A * F;
#pragma unroll
    for (int a = 0; a < AM; ++a) {
        if (a >= A) break;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 t = make_float4(xsum(gwa[a][q].x), xsum(gwa[a][q].y), xsum(gwa[a][q].z), xsum(gwa[a][q].w));
            if (grp == 0) *reinterpret_cast<float4 *>(my + a * F + 64 * q + 4 * gl) = t;
        }
        // bias sums: every lane of a group holds its group's sum; one lane per group adds in
        const float b = gba[a];
        const float bs = __shfl(b, 0, 64) + __shfl(b, 16, 64) + __shfl(b, 32, 64) + __shfl(b, 48, 64);
        if (lane == 0) my[AF + F + a] = bs;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float4 t = make_float4(xsum(gwv[q].x), xsum(gwv[q].y), xsum(gwv[q].z), xsum(gwv[q].w));
        if (grp == 0) *reinterpret_cast<float4 *>(my + AF + 64 * q + 4 * gl) = t;
    }
    {
        const float bs = __shfl(gbv, 0, 64) + __shfl(gbv, 16, 64) + __shfl(gbv, 32, 64) + __shfl(gbv, 48, 64);
        if (lane == 0) my[AF + F + A] = bs;
    }
#pragma unroll
    for (int k = 0; k < kStats; ++k) {
        const double v0 = __shfl(st[k], 0, 64), v1 = __shfl(st[k], 16, 64), v2 = __shfl(st[k], 32, 64),
                     v3 = __shfl(st[k], 48, 64);
        if (lane == 0) sred[wv * kStats + k] = ((v0 + v1) + v2) + v3;
    }
    __syncthreads();
    float *out = g.part + (int64_t)blockIdx.x * PG;
    for (int i = threadIdx.x; i < PG; i += 256) {
        const int sl = head_slot(i, A, F);
        out[i] = ((red[sl] + red[PGP + sl]) + red[2 * PGP + sl]) + red[3 * PGP + sl];
    }
    if (threadIdx.x < kStats)
        g.spart[(int64_t)blockIdx.x * kStats + threadIdx.x] =
            ((sred[threadIdx.x] + sred[kStats + threadIdx.x]) + sred[2 * kStats + threadIdx.x]) +
            sred[3 * kStats + threadIdx.x];
}

// gout[i] = sum_b part[b][i] (blocks 0 .. nred-1, 64 outputs each, the 4 waves
// summing quarters of the block range in order); the last block sums the f64
// logged values and writes stats [6] = cross-entropy, value loss, entropy
// loss, loss, accuracy, labelled share.
__global__ __launch_bounds__(256) void bc_loss_reduce_kernel(const float *__restrict__ part,
                                                             const double *__restrict__ spart,
                                                             const int64_t *__restrict__ cnt, int weighted, int nb,
                                                             int PG, int M, float ent_coef, float vf_coef,
                                                             float *__restrict__ gout, double *__restrict__ stats) {
    const int t = threadIdx.x;
    if (blockIdx.x + 1 == gridDim.x) {
        __shared__ double sr[256];
        double v[kStats];
        for (int k = 0; k < kStats; ++k) {
            double s = 0.0;
            for (int b = t; b < nb; b += 256) s += spart[(int64_t)b * kStats + k];
            sr[t] = s;
            __syncthreads();
            for (int h = 128; h >= 1; h >>= 1) {
                if (t < h) sr[t] += sr[t + h];
                __syncthreads();
            }
            v[k] = sr[0];
            __syncthreads();
        }
        if (t == 0) {
            const int64_t nl = labelled(cnt, weighted != 0, M);
            const double n = M, dl = (double)(nl > 0 ? nl : 1);
            const double ce = v[0] / dl, vl = v[1] / n, el = -v[2] / n;
            stats[0] = ce;
            stats[1] = vl;
            stats[2] = el;
            stats[3] = ce + (double)ent_coef * el + (double)vf_coef * vl;
            stats[4] = v[3] / dl;
            stats[5] = (double)nl / n;
        }
        return;
    }
    __shared__ float q[4][64];
    const int o = t & 63, w = t >> 6;
    const int i = blockIdx.x * 64 + o;
    const int per_q = (nb + 3) / 4, b0 = w * per_q, b1 = min(nb, b0 + per_q);
    float s = 0.0f;
    if (i < PG) {
        int b = b0;
        for (; b + 8 <= b1; b += 8) {
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = part[(int64_t)(b + u) * PG + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += x[u];
        }
        for (; b < b1; ++b) s += part[(int64_t)b * PG + i];
    }
    q[w][o] = s;
    __syncthreads();
    if (w == 0 && i < PG) gout[i] = ((q[0][o] + q[1][o]) + q[2][o]) + q[3][o];
}

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
// vn_bc_loss (labels) and vn_bc_loss_set (label_set): exactly one of the two is given
int bc_launch(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
              const float *bv, const int64_t *src, const int32_t *labels, const uint8_t *label_set,
              const uint8_t *weight, const float *returns, int32_t M, int32_t F, int32_t A, float ent_coef,
              float vf_coef, float *dhp, float *dhv, float *grad_heads, double *stats, float *part, double *spart,
              void *stream) {
    const bool set = label_set != nullptr;
    if (!hp || !hv || !wa || !ba || !wv || !bv || (!labels && !label_set) || !returns || !dhp || !dhv || !grad_heads ||
        !stats || !part || !spart)
        return fail(VN_ERR_INVALID, "NULL argument");
    if (M < 1 || A < 1 || A > kMaxA) return fail(VN_ERR_INVALID, "bad sizes M=%d A=%d (A <= %d)", M, A, kMaxA);
    if (F < 64 || F > 256 || F % 64) return fail(VN_ERR_INVALID, "latent width F=%d: a multiple of 64 up to 256", F);
    if (ldh < F) return fail(VN_ERR_INVALID, "latent row stride %lld < F", (long long)ldh);
    const hipStream_t s = (hipStream_t)stream;
    const int nb = (M + kWaves * kSPW - 1) / (kWaves * kSPW);
    // the labelled counts sit behind the blocks' sums in spart (8-byte words both)
    int64_t *cnt = reinterpret_cast<int64_t *>(spart + (int64_t)nb * kStats);
    // (a set may be empty, so the labelled count of the set form depends on the sets: always counted)
    if (set)
        hipLaunchKernelGGL(bc_count_set_kernel, dim3(kCntBlocks), dim3(256), 0, s, label_set, weight, src, M,
                           (1u << A) - 1u, cnt);
    else if (weight)
        hipLaunchKernelGGL(bc_count_kernel, dim3(kCntBlocks), dim3(256), 0, s, weight, src, M, cnt);
    BcArgs g{};
    g.hp = hp; g.hv = hv; g.ldh = ldh; g.wa = wa; g.ba = ba; g.wv = wv; g.bv = bv;
    g.src = src; g.wgt = weight; g.ret = returns; g.cnt = cnt;
    g.lab = set ? reinterpret_cast<const int32_t *>(label_set) : labels;   // (bc_loss_kernel, SET)
    g.dhp = dhp; g.dhv = dhv; g.part = part; g.spart = spart;
    g.M = M; g.F = F; g.A = A; g.ent_coef = ent_coef; g.vf_coef = vf_coef;
    const int PG = A * F + A + F + 1;
    const int PGP = (PG + 3) & ~3;
    const int AM = (A + 1) / 2 * 2;
    const size_t lds = ((size_t)AM * F + (size_t)kWaves * PGP) * sizeof(float) + (size_t)kWaves * kStats * sizeof(double);
#define VN_BC_K(Q_, AM_)                                                                               \
    if (set) hipLaunchKernelGGL((bc_loss_kernel<Q_, AM_, true>), dim3(nb), dim3(256), lds, s, g);      \
    else hipLaunchKernelGGL((bc_loss_kernel<Q_, AM_, false>), dim3(nb), dim3(256), lds, s, g);         \
    break;
#define VN_BC_Q(Q_)                                                                                    \
    switch (AM) {                                                                                      \
        case 2: VN_BC_K(Q_, 2)                                                                         \
        case 4: VN_BC_K(Q_, 4)                                                                         \
        case 6: VN_BC_K(Q_, 6)                                                                         \
        default: VN_BC_K(Q_, 8)                                                                        \
    }
    switch (F / 64) {
        case 1: VN_BC_Q(1) break;
        case 2: VN_BC_Q(2) break;
        case 3: VN_BC_Q(3) break;
        default: VN_BC_Q(4) break;
    }
#undef VN_BC_Q
#undef VN_BC_K
    hipLaunchKernelGGL(bc_loss_reduce_kernel, dim3((unsigned)((PG + 63) / 64 + 1)), dim3(256), 0, s, part, spart, cnt,
                       (set || weight) ? 1 : 0, nb, PG, M, ent_coef, vf_coef, grad_heads, stats);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace

extern "C" {

int vn_bc_loss_part_floats(int32_t M, int32_t F, int32_t A, int64_t *n_part, int64_t *n_spart) {
    if (M < 1 || F < 1 || A < 1) return fail(VN_ERR_INVALID, "bad sizes M=%d F=%d A=%d", M, F, A);
    const int64_t nb = (M + kWaves * kSPW - 1) / (kWaves * kSPW);
    if (n_part) *n_part = nb * ((int64_t)A * F + A + F + 1);
    if (n_spart) *n_spart = nb * kStats + kCntBlocks;   // + the labelled counts (int64 words)
    return VN_OK;
}

int vn_bc_loss(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
               const float *bv, const int64_t *src, const int32_t *labels, const uint8_t *weight,
               const float *returns, int32_t M, int32_t F, int32_t A, float ent_coef, float vf_coef, float *dhp,
               float *dhv, float *grad_heads, double *stats, float *part, double *spart, void *stream) {
    return bc_launch(hp, hv, ldh, wa, ba, wv, bv, src, labels, nullptr, weight, returns, M, F, A, ent_coef, vf_coef,
                     dhp, dhv, grad_heads, stats, part, spart, stream);
}

int vn_bc_loss_set(const float *hp, const float *hv, int64_t ldh, const float *wa, const float *ba, const float *wv,
                   const float *bv, const int64_t *src, const uint8_t *label_set, const uint8_t *weight,
                   const float *returns, int32_t M, int32_t F, int32_t A, float ent_coef, float vf_coef, float *dhp,
                   float *dhv, float *grad_heads, double *stats, float *part, double *spart, void *stream) {
    return bc_launch(hp, hv, ldh, wa, ba, wv, bv, src, nullptr, label_set, weight, returns, M, F, A, ent_coef,
                     vf_coef, dhp, dhv, grad_heads, stats, part, spart, stream);
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
