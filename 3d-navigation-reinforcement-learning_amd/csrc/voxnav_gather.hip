// voxnav_gather.hip -- vn_copy_agents' kernel unit (vn_gather, env_params.h):
// agent i of one env becomes a layout-native copy of agent src_index[i] of a
// layout-compatible env (or of the same env).  What an agent consists of is
// the plan of env_plan.h (agent_parts), the one the whole-env snapshots are
// sized from: hot word, window record, next seed, belief block, goal,
// draw-ahead row, stood rows and nonzero-set mask -- not the episode record,
// which stays with the slot.  A bandwidth-bound copy: one block per
// destination agent, 16-byte accesses wherever a part's stride allows them,
// bounded loops, no LDS, no wait between blocks, no atomic but the rejection
// count.  The step kernels are not touched and not instantiated here.  No
// reference counterpart (the reference has one env per process).

#include "vn_common.h"
#include "env_params.h"
#include "env_plan.h"

namespace {

constexpr int GATHER_BLOCK = 256;

// one env's per-agent buffers (Params: hot with the window records behind it,
// stood with the masks behind it)
struct GatherSide {
    uint4 *hot, *wrec, *predraw;
    uint32_t *seed, *goal, *stood;
    int8_t *belief;
    uint2 *pnz;
    int N;
};

struct GatherArgs {
    GatherSide d, s;
    uint32_t wrec16, belief16, stood16;   // 16-byte pieces per agent of the window record, belief block, stood rows
    int same;                             // dst == src: a source that this call writes is refused
    const int32_t *src_index;
    const int64_t *seeds;
    int32_t *n_rejected;
};

GatherSide side_of(const Params &p, const AgentParts &ap) {
    GatherSide g;
    g.hot = p.hot;
    g.wrec = ap.wrec ? p.hot + p.N : nullptr;            // wrec_base (env_window.h)
    g.predraw = p.predraw;
    g.seed = p.next_seed;
    g.goal = p.goal;
    g.stood = ap.stood ? p.stood : nullptr;
    g.belief = p.belief;
    g.pnz = ap.stood ? p.pnz : nullptr;
    g.N = p.N;
    return g;
}

// R rows of GATHER_BLOCK 16-byte pieces from piece k on: this lane's R loads, then its R stores
template <int R>
__device__ __forceinline__ void copy_rows(uint4 *dst, const uint4 *src, uint32_t k) {
    static_assert(R == 1 || R == 2 || R == 4, "written out for 1, 2 and 4 rows");
    const uint4 v0 = src[k];
    uint4 v1 = v0, v2 = v0, v3 = v0;
    if (R >= 2) v1 = src[k + GATHER_BLOCK];
    if (R == 4) {
        v2 = src[k + 2 * GATHER_BLOCK];
        v3 = src[k + 3 * GATHER_BLOCK];
    }
    dst[k] = v0;
    if (R >= 2) dst[k + GATHER_BLOCK] = v1;
    if (R == 4) {
        dst[k + 2 * GATHER_BLOCK] = v2;
        dst[k + 3 * GATHER_BLOCK] = v3;
    }
}

// One block per destination agent.  Every exit before the copy is
// block-uniform: the decision reads src_index and seeds only.  With dst == src
// a block reads agent j only if no block writes j (the rule below), and writes
// agent i only, so the blocks need no order.
__global__ __launch_bounds__(GATHER_BLOCK) void gather_kernel(GatherArgs a) {
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (i >= a.d.N) return;
    const int j = a.src_index[i];
    if (j == -1) return;                                  // agent i keeps its state
    const int64_t sd = a.seeds != nullptr ? a.seeds[i] : -1;
    bool ok = j >= 0 && j < a.s.N && sd >= -1 && sd < ((int64_t)1 << 32);
    if (ok && a.same && j != i) {                         // in place: the source must be an agent this call leaves alone
        const int jj = a.src_index[j];
        ok = (jj == -1 || jj == j) && (a.seeds == nullptr || a.seeds[j] == -1);
    }
    if (!ok) {
        if (tid == 0 && a.n_rejected != nullptr) atomicAdd(a.n_rejected, 1);
        return;
    }
    if (a.same && j == i) {                               // a copy of itself: the seed override is all there is to do
        if (tid == 0 && sd >= 0) a.d.seed[i] = (uint32_t)sd;
        return;
    }
    const size_t si = (size_t)j, di = (size_t)i;

    // ---- the small parts: one 16-byte piece (or one word) per lane, loaded
    // before the belief block's loop and stored after it ----
    const uint32_t n_hot = 1u, n_wrec = n_hot + a.wrec16, n_pre = n_wrec + 1u, n_stood = n_pre + a.stood16;   // <= 42
    const uint4 *s16 = nullptr;
    uint4 *d16 = nullptr;
    const uint32_t t = (uint32_t)tid;
    if (t < n_hot) {
        s16 = a.s.hot + si;
        d16 = a.d.hot + di;
    } else if (t < n_wrec) {
        s16 = a.s.wrec + si * a.wrec16 + (t - n_hot);
        d16 = a.d.wrec + di * a.wrec16 + (t - n_hot);
    } else if (t < n_pre) {
        s16 = a.s.predraw + si;
        d16 = a.d.predraw + di;
    } else if (t < n_stood) {
        s16 = reinterpret_cast<const uint4 *>(a.s.stood + si * 32u) + (t - n_pre);
        d16 = reinterpret_cast<uint4 *>(a.d.stood + di * 32u) + (t - n_pre);
    }
    uint4 small = make_uint4(0u, 0u, 0u, 0u);
    if (s16 != nullptr) small = *s16;
    // words: lane 64 the seed, 65 the goal, 66 the nonzero-set mask (8 bytes)
    uint32_t word = 0u;
    uint2 mask = make_uint2(0u, 0u);
    if (tid == 64) word = sd >= 0 ? (uint32_t)sd : a.s.seed[si];
    if (tid == 65) word = a.s.goal[si];
    if (tid == 66 && a.s.pnz != nullptr) mask = a.s.pnz[si];

    // ---- the belief block: rows of GATHER_BLOCK 16-byte pieces.  The partial last row's load is issued first
    // and stored last; the full rows go four (then two, one) at a time, their loads before their stores ----
    const uint4 *sb = reinterpret_cast<const uint4 *>(a.s.belief) + si * a.belief16;
    uint4 *db = reinterpret_cast<uint4 *>(a.d.belief) + di * a.belief16;
    uint32_t full = a.belief16 / GATHER_BLOCK;
    const uint32_t kr = full * GATHER_BLOCK + t;
    const bool has_rest = kr < a.belief16;
    uint4 rest = make_uint4(0u, 0u, 0u, 0u);
    if (has_rest) rest = sb[kr];
    uint32_t k = t;
    for (; full >= 4u; full -= 4u, k += 4u * GATHER_BLOCK) copy_rows<4>(db, sb, k);
    if (full & 2u) {
        copy_rows<2>(db, sb, k);
        k += 2u * GATHER_BLOCK;
    }
    if (full & 1u) copy_rows<1>(db, sb, k);
    if (has_rest) db[kr] = rest;

    if (d16 != nullptr) *d16 = small;
    if (tid == 64) a.d.seed[di] = word;
    if (tid == 65) a.d.goal[di] = word;
    if (tid == 66 && a.d.pnz != nullptr) a.d.pnz[di] = mask;
}

}  // namespace

namespace vn_gather {

int copy_agents(const void *dst, const void *src, const void *parts, const int32_t *src_index, const int64_t *seeds,
                int32_t *n_rejected, hipStream_t s) {
    const Params &pd = *static_cast<const Params *>(dst);
    const Params &ps = *static_cast<const Params *>(src);
    const AgentParts &ap = *static_cast<const AgentParts *>(parts);
    // the 16-byte parts (agent_parts: hot 16, predraw 16; the others in pieces)
    if (ap.hot != 16u || ap.predraw != 16u || ap.seed != 4u || ap.goal != 4u || ap.wrec % 16u || ap.belief % 16u ||
        ap.stood % 16u || (ap.pnz != 0u && ap.pnz != 8u) || 2u + ap.wrec / 16u + ap.stood / 16u > 64u)
        return fail(VN_ERR_INVALID, "vn_copy_agents: the per-agent plan has a part this copy does not know");
    GatherArgs a;
    a.d = side_of(pd, ap);
    a.s = side_of(ps, ap);
    a.wrec16 = ap.wrec / 16u;
    a.belief16 = ap.belief / 16u;
    a.stood16 = ap.stood / 16u;
    a.same = pd.hot == ps.hot;
    a.src_index = src_index;
    a.seeds = seeds;
    a.n_rejected = n_rejected;
    if (n_rejected != nullptr) VN_HIP(hipMemsetAsync(n_rejected, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)pd.N), dim3(GATHER_BLOCK), 0, s, a);
    VN_HIP(hipGetLastError());
    return VN_OK;
}

}  // namespace vn_gather
