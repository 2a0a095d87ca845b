// kickstart_layout_check.cpp -- head_loss_layout_check.cpp's walk for the
// seven f64 sums of the kickstart objectives (csrc/voxnav_ppo_bc_loss.hip),
// built by tests/test_kickstart_layout_host.py with g++ and the sanitizers.  It
// walks every (A, F) the entry points take at 7 stats and checks the rule the
// kernel relies on: every carve offset and every
// float4-stored segment starts on 16 B, the f64 sums on 8 B, the regions do not
// overlap, slot() maps grad_heads' order one-to-one into a row, and the whole
// carve fits the 64 KB a block may ask for.
// It then walks a restatement of the spart workspace -- the blocks' seven
// sums, the 64 labelled-count words behind them, 8-byte words both -- in a heap
// block of the documented size.  The stat and count-block numbers are restated
// here (they live in HIP-only code), so of the product this part exercises
// head_loss::blocks() only: it shows that the documented layout is consistent,
// not that the launcher follows it.  The launcher's own layout is checked on
// the GPU, by the guard bands of tests/test_kickstart_loss_gpu.py.
// Prints one line per failure and "checked N layouts"; exit status 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "head_loss.h"

using head_loss::HeadLayout;
using head_loss::kWaves;

namespace {

int failures = 0;

void expect(bool ok, const HeadLayout &L, const char *what, long got) {
    if (ok) return;
    ++failures;
    std::printf("A=%d F=%d stats=%d: %s (%ld)\n", L.A, L.F, L.n_stats, what, got);
}

void check(int A, int F, int n_stats) {
    const HeadLayout L(A, F, n_stats);
    expect(L.AM >= A && L.AM % 2 == 0 && L.AM - A <= 1, L, "AM is A rounded up to even", L.AM);
    expect(L.PG == A * F + A + F + 1, L, "PG = A F + A + F + 1", L.PG);
    expect(L.PGP >= L.PG && L.PGP - L.PG < 4 && L.PGP % 4 == 0, L, "PGP is PG rounded up to 4", L.PGP);
    // the carve: weights [AM][F], rows [kWaves][PGP], sums [kWaves][n_stats] f64
    expect(L.weights() == 0, L, "weights offset", L.weights());
    expect(L.rows() % 16 == 0 && L.rows() >= L.weights() + L.AM * F * 4, L, "rows offset", L.rows());
    expect(L.sums() % 16 == 0 && L.sums() >= L.rows() + kWaves * L.PGP * 4, L, "sums offset", L.sums());
    expect(L.bytes() == L.sums() + kWaves * n_stats * 8, L, "total bytes", L.bytes());
    expect(L.bytes() <= 64 * 1024, L, "fits 64 KB", L.bytes());
    for (int wv = 0; wv < kWaves; ++wv) {
        const long row = L.rows() + 4L * wv * L.PGP;
        expect(row % 16 == 0, L, "a wave's row starts on 16 B", row);
        // the float4-stored segments: every d Wa row [F] and d wv
        for (int a = 0; a < A; ++a)
            expect((row + 4L * (L.d_wa() + a * F)) % 16 == 0, L, "a d Wa row starts on 16 B", a);
        expect((row + 4L * L.d_wv()) % 16 == 0, L, "d wv starts on 16 B", L.d_wv());
        expect((L.sums() + 8L * wv * n_stats) % 8 == 0, L, "a wave's f64 sums start on 8 B", wv);
    }
    // the row's segments tile [0, PG) in the order d Wa, d wv, d ba, d bv
    expect(L.d_wa() == 0 && L.d_wv() == A * F && L.d_ba() == L.d_wv() + F && L.d_bv() == L.d_ba() + A &&
               L.d_bv() + 1 == L.PG,
           L, "row segments", L.d_bv());
    // slot(): grad_heads' order d Wa, d ba, d wv, d bv -> the row, one-to-one
    std::vector<int> hits(L.PGP, 0);
    for (int i = 0; i < L.PG; ++i) {
        const int s = L.slot(i);
        if (s < 0 || s >= L.PG) {
            expect(false, L, "slot inside the row", s);
            continue;
        }
        ++hits[s];
        const int AF = A * F;
        const int want = i < AF ? L.d_wa() + i : i < AF + A ? L.d_ba() + (i - AF) : i < AF + A + F ? L.d_wv() + (i - AF - A) : L.d_bv();
        expect(s == want, L, "slot follows the segments", i);
    }
    for (int s = 0; s < L.PG; ++s) expect(hits[s] == 1, L, "slot is a bijection", s);
}

}  // namespace

constexpr int kStats = 7;      // PpoBc::kStats
constexpr int kCntBlocks = 64; // bc_objective.h

// as documented: the blocks write spart[b * 7 + k], the count kernel the int64
// words from spart + blocks * 7 on; the reduce kernel reads both back
void check_spart(int M) {
    static_assert(sizeof(double) == sizeof(int64_t), "8-byte words both");
    const int64_t nb = head_loss::blocks(M);
    const int64_t words = nb * kStats + kCntBlocks;     // part_floats' n_spart
    std::vector<double> spart((size_t)words, -1.0);
    int64_t *cnt = reinterpret_cast<int64_t *>(spart.data() + nb * kStats);
    for (int c = 0; c < kCntBlocks; ++c) cnt[c] = c;
    for (int64_t b = 0; b < nb; ++b)
        for (int k = 0; k < kStats; ++k) spart[(size_t)(b * kStats + k)] = (double)(b * kStats + k);
    bool ok = reinterpret_cast<uintptr_t>(cnt) % 8 == 0;
    for (int c = 0; c < kCntBlocks; ++c) ok = ok && cnt[c] == c;
    for (int64_t i = 0; i < nb * kStats; ++i) ok = ok && spart[(size_t)i] == (double)i;
    if (!ok) {
        ++failures;
        std::printf("M=%d: the sums and the count words overlap or are misaligned\n", M);
    }
}

int main() {
    int n = 0;
    for (int A = 1; A <= head_loss::kMaxA; ++A)
        for (int F = 64; F <= 256; F += 64, ++n) check(A, F, kStats);
    for (int M : {1, 128, 129, 257, 65536}) check_spart(M);
    // the launcher's block count
    if (head_loss::blocks(1) != 1 || head_loss::blocks(128) != 1 || head_loss::blocks(129) != 2) {
        ++failures;
        std::printf("blocks(): 128 samples per block\n");
    }
    std::printf("checked %d layouts\n", n);
    return failures ? 1 : 0;
}
