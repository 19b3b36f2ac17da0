// verify_wase_tree.cpp -- the two stack walks of csrc/wase_tree.h (what thread 0 of k_wase_piece_sums runs) against
// the recursive definition of numpy's pairwise sum, for EVERY piece length n = 1 .. 8192:
//   * the listed leaves tile [0, n) from left to right, each of 1 .. 128 elements, at most WASE_MAX_LEAVES of them;
//   * no write of either walk falls outside its WASE_TREE_STACK stack slots or the leaf arrays (checked before the write);
//   * leaf sums by numpy's leaf rule, added up by the combine walk, equal the recursive sum bit for bit, on data whose
//     magnitudes span six decades (so that another order of additions gives other bits).
// Prints "OK leaves <max> depth <max>" or the first failure.  Build: g++ -O1 -ffp-contract=off (float32 adds as written).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

// every array write of the walks is checked BEFORE it happens, and the largest index of each kind is kept
static int g_max_leaf = -1, g_max_slot = -1, g_n = 0;
#define WASE_TREE_SLOT(i, size)                                                                                   \
    do {                                                                                                          \
        if ((i) < 0 || (i) >= (size)) { std::printf("n=%d: index %d into an array of %d\n", g_n, (int)(i), (int)(size)); std::exit(1); } \
        int& mx_ = (size) == WASE_MAX_LEAVES ? g_max_leaf : g_max_slot;                                           \
        if ((i) > mx_) mx_ = (i);                                                                                 \
    } while (0)
#include "wase_tree.h"
static_assert(WASE_MAX_LEAVES != WASE_TREE_STACK, "the hook tells the two kinds of array apart by their size");

// numpy's pairwise sum, written the plain way: recursion, the eight accumulators spelled out
static float pairwise(const float* a, int n)
{
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        float r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i;
        for (i = 8; i < n - n % 8; i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise(a, n2) + pairwise(a + n2, n - n2);
}

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main()
{
    const int NMAX = 8192;
    std::mt19937 gen(12345);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::uniform_real_distribution<float> ud(-3.f, 3.f);
    std::vector<float> pool(2 * NMAX);
    for (float& v : pool) v = nd(gen) * std::pow(10.f, ud(gen));

    std::vector<int> loff(WASE_MAX_LEAVES), ln(WASE_MAX_LEAVES);
    std::vector<float> lsum(WASE_MAX_LEAVES);
    for (int n = 1; n <= NMAX; ++n) {
        const float* a = pool.data() + (n * 37) % NMAX;              // another window of the pool for every length
        g_n = n;
        const int nl = wase_tree_leaves(n, loff.data(), ln.data());
        if (nl < 1 || nl > WASE_MAX_LEAVES) { std::printf("n=%d: %d leaves\n", n, nl); return 1; }
        int at = 0;
        for (int l = 0; l < nl; ++l) {
            if (loff[l] != at || ln[l] < 1 || ln[l] > NP_PW_BLOCK) { std::printf("n=%d: leaf %d is [%d,+%d), expected to start at %d\n", n, l, loff[l], ln[l], at); return 1; }
            at += ln[l];
        }
        if (at != n) { std::printf("n=%d: leaves cover %d elements\n", n, at); return 1; }
        for (int l = 0; l < nl; ++l) lsum[l] = pairwise(a + loff[l], ln[l]);   // ln <= 128: the leaf rule alone
        const float got = wase_tree_combine(n, lsum.data());
        const float want = pairwise(a, n);
        if (bits(got) != bits(want)) { std::printf("n=%d: walk %.9g (%08x), recursion %.9g (%08x)\n", n, got, bits(got), want, bits(want)); return 1; }
    }
    std::printf("OK leaves %d depth %d\n", g_max_leaf + 1, g_max_slot + 1);
    return 0;
}
