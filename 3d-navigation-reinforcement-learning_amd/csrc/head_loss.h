// head_loss.h -- the fused "head loss" of the learner, once: the skeleton that
// vn_ppo_loss (voxnav_ppo_loss.hip), vn_bc_loss / vn_bc_loss_set
// (voxnav_bc_loss.hip), vn_ppo_bc_loss / vn_ppo_bc_loss_set
// (voxnav_ppo_bc_loss.hip), vn_ppo_loss_masked (voxnav_masked_loss.hip), the
// masked cross-entropy entries (voxnav_masked_bc_loss.hip,
// voxnav_masked_ppo_bc_loss.hip) and the value-clipped vn_ppo_loss[_masked]_vclip
// (voxnav_vclip_loss.hip) share; their file headers state the formulas.
// Common to them, with lp = log_softmax(z), p = exp(lp), H the entropy:
//   dz_j = (the objective's policy term)_j + (ent_coef / M) p_j (lp_j + H)
//   dv   = vf_coef 2 (v - ret) / M
//
// The skeleton owns the sample tiling (one wave per kSPW samples, 16 lanes per
// sample across the latent features, a float4 each; the wave's 4 groups take 4
// samples per pass), the head dot products (xor butterflies over the 16 lanes:
// every lane of a group ends with the same bits, so the per-sample scalar work
// runs redundantly without a broadcast), log-softmax, entropy and argmax, the
// value term, the gradient accumulation and stores, the group / wave / block
// fold into per-block partials (f32 head gradients, f64 logged sums: slot 1 the
// squared value error, slot 2 the entropy), and the reduce kernel that sums the
// partials in a fixed order.  An objective (a plain struct: PpoClip in
// ppo_objective.h, BcLabel / BcSet in bc_objective.h, PpoBc<> composed of them
// in ppo_bc_objective.h) supplies what differs:
//   kStats            f64 sums per block (slots 0, 3.. are the objective's)
//   begin(M)          block-uniform values, every thread (e.g. 1 / labelled) -> Obj::Block
//   gather(b, r, A)   the sample's own gathered inputs -> Obj::Sample
//   policy(b, s, f, ok, w, inv_n)   the sample's policy-gradient scale and friends
//   dz(s, f, a)       the policy term of dz_a
//   stats(s, f, st)   its logged sums
//   finish(v, M, ent_coef, vf_coef, stats)   sums -> stats[6] (reduce kernel)
// and, optionally, a compile-time trait: an objective that declares
//   static constexpr bool kAllowed = true;   allowed(s, A) -> bits of the sample's
//                     allowed actions, a non-empty subset of bits 0 .. A-1
// has the softmax, entropy and argmax run over that set only (PpoClipMasked in
// voxnav_masked_loss.hip, BcMasked<> in masked_bc_objective.h, PpoBcMasked<> in
// voxnav_masked_ppo_bc_loss.hip: lp_j = z_j - logsumexp_{k in S} z_k, p_j = 0 and
// dz_j exactly 0 outside S).  Without the trait the kernel is the unmasked one,
// instruction for instruction.  In the same way, an objective that declares
//   static constexpr bool kValueClip = true;   value_clip(s, v) -> ClippedValue
// has the value term run on the clipped value v' (ValueClipped<> in
// voxnav_vclip_loss.hip): the squared error is (ret - v')^2 and dv is the
// formula's on v' where the clip passes the gradient, exactly 0 elsewhere.
// Without it the value term is the one above.
//
// LDS (HeadLayout, all of it dynamic; used by the kernel's carve and by the
// launcher's byte count): action weights [AM][F], then the waves'
// head-gradient rows [kWaves][PGP], then the waves' f64 sums [kWaves][kStats].
// The rule: every carve offset and every float4-stored segment is a multiple
// of 16 B.  A row holds d Wa [A][F], d wv [F] (the two float4-stored parts
// first), d ba [A], d bv, padded to PGP = PG rounded up to 4; grad_heads' order
// is d Wa, d ba, d wv, d bv (slot() maps an output index to its row slot).
#pragma once

#include <cstdint>

namespace head_loss {

constexpr int kSPW = 32;       // samples per wave
constexpr int kWaves = 4;      // waves per block
constexpr int kMaxA = 8;       // actions

struct HeadLayout {
    int A, F, AM, PG, PGP, n_stats;
    // AM: A rounded up to even (the per-action registers; the kernel gives its template value)
    constexpr HeadLayout(int A_, int F_, int n_stats_, int AM_)
        : A(A_), F(F_), AM(AM_), PG(A_ * F_ + A_ + F_ + 1), PGP((A_ * F_ + A_ + F_ + 1 + 3) & ~3), n_stats(n_stats_) {}
    constexpr HeadLayout(int A_, int F_, int n_stats_) : HeadLayout(A_, F_, n_stats_, (A_ + 1) / 2 * 2) {}
    // carve offsets, bytes
    constexpr int weights() const { return 0; }
    constexpr int rows() const { return AM * F * 4; }
    constexpr int sums() const { return (AM * F + kWaves * PGP) * 4; }
    constexpr int bytes() const { return sums() + kWaves * n_stats * 8; }
    // segments of a row, floats
    constexpr int d_wa() const { return 0; }
    constexpr int d_wv() const { return A * F; }
    constexpr int d_ba() const { return A * F + F; }
    constexpr int d_bv() const { return A * F + F + A; }
    // grad_heads index -> row slot
    constexpr int slot(int i) const {
        const int AF = A * F;
        if (i < AF) return i;
        if (i < AF + A) return AF + F + (i - AF);
        if (i < AF + A + F) return AF + (i - AF - A);
        return AF + F + A;
    }
};

constexpr int64_t blocks(int M) { return ((int64_t)M + kWaves * kSPW - 1) / (kWaves * kSPW); }

}  // namespace head_loss

#ifdef __HIPCC__

#include <hip/hip_runtime.h>

#include <type_traits>

#include "vn_common.h"

namespace head_loss {

// the objective's kAllowed trait (false when it declares none)
template <class Obj, class = void>
struct has_allowed : std::false_type {};
template <class Obj>
struct has_allowed<Obj, std::void_t<decltype(Obj::kAllowed)>> : std::bool_constant<Obj::kAllowed> {};

// the objective's kValueClip trait (false when it declares none)
template <class Obj, class = void>
struct has_value_clip : std::false_type {};
template <class Obj>
struct has_value_clip<Obj, std::void_t<decltype(Obj::kValueClip)>> : std::bool_constant<Obj::kValueClip> {};

// value_clip's result: the value the loss sees, and whether v takes its gradient
struct ClippedValue {
    float v;
    bool pass;
};

struct HeadArgs {
    const float *hp, *hv;       // latents [M][F] (row stride ldh)
    int64_t ldh;
    const float *wa, *ba, *wv, *bv;   // action_net [A][F], [A]; value_net [F], [1]
    const int64_t *src;         // [M] rows of the buffers (NULL: identity)
    const float *ret;
    float *dhp, *dhv;           // [M][F] contiguous
    float *part;                // [blocks][PG]
    double *spart;              // [blocks][kStats]
    int M, F, A;
    float ent_coef, vf_coef;
};

// a sample's head forward, uniform over its 16-lane group
template <int AM>
struct Forward {
    float z[AM], lpa[AM], p[AM];
    float zmax, lse, ent;
    int amax;                   // argmax, ties to the lowest index
};

// Q = F / 64: lane l of a 16-lane group holds latent features
// 64 q + 4 (l & 15) .. +3 (q < Q) -- one float4 per q, 256 B contiguous per
// group.  The action weights are read from LDS.
template <int Q, int AM, class Obj>
__global__ __launch_bounds__(256) void head_loss_kernel(HeadArgs g, Obj obj) {
    constexpr int kStats = Obj::kStats;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int grp = lane >> 4, gl = lane & 15;
    const int F = g.F, A = g.A;
    const HeadLayout L(A, F, kStats, AM);
    const int PG = L.PG, PGP = L.PGP;
    float *wsh = lds + L.weights() / 4;
    float *red = lds + L.rows() / 4;
    double *sred = reinterpret_cast<double *>(lds + L.sums() / 4);
    for (int i = threadIdx.x; i < AM * F; i += 256) wsh[i] = i < A * F ? g.wa[i] : 0.0f;
    auto wa = [&](int a, int q) { return *reinterpret_cast<const float4 *>(wsh + a * F + 64 * q + 4 * gl); };
    float4 wvv[Q];
    float ba[AM];
#pragma unroll
    for (int a = 0; a < AM; ++a) ba[a] = a < A ? g.ba[a] : 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) wvv[q] = *reinterpret_cast<const float4 *>(g.wv + 64 * q + 4 * gl);
    const float bv = g.bv[0];
    const typename Obj::Block blk = obj.begin(g.M);
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
    double st[kStats];
#pragma unroll
    for (int k = 0; k < kStats; ++k) st[k] = 0.0;

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
        const float ret = g.ret[r];
        typename Obj::Sample s = obj.gather(blk, r, A);
        Forward<AM> f;
#pragma unroll
        for (int a = 0; a < AM; ++a) {
            float sacc = 0.0f;
#pragma unroll
            for (int q = 0; q < Q; ++q) sacc += dot4(hp[q], wa(a, q));
            f.z[a] = a < A ? gsum(sacc) + ba[a] : -INFINITY;
        }
        float sv = 0.0f;
#pragma unroll
        for (int q = 0; q < Q; ++q) sv += dot4(hv[q], wvv[q]);
        const float v = gsum(sv) + bv;
        // log_softmax, entropy, argmax (uniform over the group)
        unsigned allow = 0;
        if constexpr (has_allowed<Obj>::value) {
            // over the sample's allowed set only; an action outside it contributes
            // selected zeros (no 0 * -inf), as a >= A does
            allow = obj.allowed(s, A);
            f.zmax = -INFINITY;
            f.amax = 0;
            bool found = false;
#pragma unroll
            for (int a = 0; a < AM; ++a) {
                const bool in = (allow >> a) & 1u;
                f.amax = in && (!found || f.z[a] > f.zmax) ? a : f.amax;
                f.zmax = in ? fmaxf(f.zmax, f.z[a]) : f.zmax;
                found = found || in;
            }
            float se = 0.0f;
#pragma unroll
            for (int a = 0; a < AM; ++a) se += (allow >> a) & 1u ? expf(f.z[a] - f.zmax) : 0.0f;
            f.lse = logf(se);
            f.ent = 0.0f;
#pragma unroll
            for (int a = 0; a < AM; ++a) {
                const bool in = (allow >> a) & 1u;
                f.lpa[a] = in ? f.z[a] - f.zmax - f.lse : (a < A ? 0.0f : -INFINITY);
                f.p[a] = in ? expf(f.lpa[a]) : 0.0f;
                f.ent -= in ? f.p[a] * f.lpa[a] : 0.0f;
            }
        } else {
            f.zmax = f.z[0];
            f.amax = 0;
#pragma unroll
            for (int a = 1; a < AM; ++a) {
                f.amax = f.z[a] > f.zmax ? a : f.amax;
                f.zmax = fmaxf(f.zmax, f.z[a]);
            }
            float se = 0.0f;
#pragma unroll
            for (int a = 0; a < AM; ++a) se += a < A ? expf(f.z[a] - f.zmax) : 0.0f;
            f.lse = logf(se);
            f.ent = 0.0f;
#pragma unroll
            for (int a = 0; a < AM; ++a) {
                f.lpa[a] = f.z[a] - f.zmax - f.lse;
                f.p[a] = a < A ? expf(f.lpa[a]) : 0.0f;
                f.ent -= a < A ? f.p[a] * f.lpa[a] : 0.0f;
            }
        }
        const float w = ok ? 1.0f : 0.0f;     // a padding pass contributes nothing
        obj.policy(blk, s, f, ok, w, inv_n);
        const float gent = g.ent_coef * inv_n * w;
        float vl = v;                         // the value the loss sees
        float dv;
        if constexpr (has_value_clip<Obj>::value) {
            const ClippedValue cv = obj.value_clip(s, v);
            vl = cv.v;
            dv = cv.pass ? g.vf_coef * 2.0f * (vl - ret) * inv_n * w : 0.0f;
        } else {
            dv = g.vf_coef * 2.0f * (v - ret) * inv_n * w;
        }
        float4 dh[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) dh[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        // the backward reads the LDS weights again (kept from the forward, they
        // would hold A Q float4 registers across the softmax)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int a = 0; a < AM; ++a) {
            if (a >= A) break;
            float dz = obj.dz(s, f, a) + gent * f.p[a] * (f.lpa[a] + f.ent);
            if constexpr (has_allowed<Obj>::value) dz = (allow >> a) & 1u ? dz : 0.0f;
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
                st[1] += (double)((ret - vl) * (ret - vl));
                st[2] += (double)f.ent;
                obj.stats(s, f, st);
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
#pragma unroll
    for (int a = 0; a < AM; ++a) {
        if (a >= A) break;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 t = make_float4(xsum(gwa[a][q].x), xsum(gwa[a][q].y), xsum(gwa[a][q].z), xsum(gwa[a][q].w));
            if (grp == 0) *reinterpret_cast<float4 *>(my + L.d_wa() + a * F + 64 * q + 4 * gl) = t;
        }
        // bias sums: every lane of a group holds its group's sum; one lane per group adds in
        const float b = gba[a];
        const float bs = __shfl(b, 0, 64) + __shfl(b, 16, 64) + __shfl(b, 32, 64) + __shfl(b, 48, 64);
        if (lane == 0) my[L.d_ba() + a] = bs;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float4 t = make_float4(xsum(gwv[q].x), xsum(gwv[q].y), xsum(gwv[q].z), xsum(gwv[q].w));
        if (grp == 0) *reinterpret_cast<float4 *>(my + L.d_wv() + 64 * q + 4 * gl) = t;
    }
    {
        const float bs = __shfl(gbv, 0, 64) + __shfl(gbv, 16, 64) + __shfl(gbv, 32, 64) + __shfl(gbv, 48, 64);
        if (lane == 0) my[L.d_bv()] = bs;
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
        const int sl = L.slot(i);
        out[i] = ((red[sl] + red[PGP + sl]) + red[2 * PGP + sl]) + red[3 * PGP + sl];
    }
    if (threadIdx.x < kStats)
        g.spart[(int64_t)blockIdx.x * kStats + threadIdx.x] =
            ((sred[threadIdx.x] + sred[kStats + threadIdx.x]) + sred[2 * kStats + threadIdx.x]) +
            sred[3 * kStats + threadIdx.x];
}

// gout[i] = sum_b part[b][i] (blocks 0 .. nred-1, 64 outputs each, the 4 waves
// summing quarters of the block range in order); the last block sums the f64
// logged values and has the objective turn them into stats [6].
template <class Obj>
__global__ __launch_bounds__(256) void head_loss_reduce_kernel(const float *__restrict__ part,
                                                               const double *__restrict__ spart, Obj obj, int nb,
                                                               int PG, int M, float ent_coef, float vf_coef,
                                                               float *__restrict__ gout, double *__restrict__ stats) {
    constexpr int kStats = Obj::kStats;
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
        if (t == 0) obj.finish(v, M, ent_coef, vf_coef, stats);
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

// ---- host side ----
// the workspace sizes of vn_*_loss_part_floats: part floats, and spart words
// (8 B: the blocks' f64 sums + the objective's own `extra` words behind them)
inline int part_floats(int32_t M, int32_t F, int32_t A, int n_stats, int extra, int64_t *n_part, int64_t *n_spart) {
    if (M < 1 || F < 1 || A < 1) return vn_detail::fail(VN_ERR_INVALID, "bad sizes M=%d F=%d A=%d", M, F, A);
    const int64_t nb = blocks(M);
    if (n_part) *n_part = nb * HeadLayout(A, F, n_stats).PG;
    if (n_spart) *n_spart = nb * n_stats + extra;
    return VN_OK;
}

// any_null: one of the entry point's required pointers is NULL
inline int check_args(bool any_null, int32_t M, int32_t F, int32_t A, int64_t ldh) {
    if (any_null) return vn_detail::fail(VN_ERR_INVALID, "NULL argument");
    if (M < 1 || A < 1 || A > kMaxA)
        return vn_detail::fail(VN_ERR_INVALID, "bad sizes M=%d A=%d (A <= %d)", M, A, kMaxA);
    if (F < 64 || F > 256 || F % 64)
        return vn_detail::fail(VN_ERR_INVALID, "latent width F=%d: a multiple of 64 up to 256", F);
    if (ldh < F) return vn_detail::fail(VN_ERR_INVALID, "latent row stride %lld < F", (long long)ldh);
    return VN_OK;
}

template <int Q, class Obj>
void launch_q(const HeadArgs &g, const Obj &obj, const HeadLayout &L, hipStream_t s) {
    const dim3 nb((unsigned)blocks(g.M));
    switch (L.AM) {
        case 2: hipLaunchKernelGGL((head_loss_kernel<Q, 2, Obj>), nb, dim3(256), L.bytes(), s, g, obj); break;
        case 4: hipLaunchKernelGGL((head_loss_kernel<Q, 4, Obj>), nb, dim3(256), L.bytes(), s, g, obj); break;
        case 6: hipLaunchKernelGGL((head_loss_kernel<Q, 6, Obj>), nb, dim3(256), L.bytes(), s, g, obj); break;
        default: hipLaunchKernelGGL((head_loss_kernel<Q, 8, Obj>), nb, dim3(256), L.bytes(), s, g, obj); break;
    }
}

// the loss kernel's Q x AM instantiation for (F, A), then the reduce kernel (checked arguments)
template <class Obj>
void launch(const HeadArgs &g, const Obj &obj, float *grad_heads, double *stats, hipStream_t s) {
    const HeadLayout L(g.A, g.F, Obj::kStats);
    switch (g.F / 64) {
        case 1: launch_q<1>(g, obj, L, s); break;
        case 2: launch_q<2>(g, obj, L, s); break;
        case 3: launch_q<3>(g, obj, L, s); break;
        default: launch_q<4>(g, obj, L, s); break;
    }
    hipLaunchKernelGGL((head_loss_reduce_kernel<Obj>), dim3((unsigned)((L.PG + 63) / 64 + 1)), dim3(256), 0, s, g.part,
                       g.spart, obj, (int)blocks(g.M), L.PG, g.M, g.ent_coef, g.vf_coef, grad_heads, stats);
}

}  // namespace head_loss

#endif  // __HIPCC__
