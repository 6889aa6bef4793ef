// Host program of tests/test_segsort_hybrid_cpu.py: steps through the hybrid segment-sort schedule of gs_segsort_dev.h as ONE virtual
// thread (tid = 0, nthreads = 1 -- the groups of the schedule are separated by barriers and touch disjoint words inside a group, so a
// sequential sweep per group is the same computation) and compares with std::sort.  Prints "ok <cases>" and returns 0, or says what
// differs and returns 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define GS_SEGSORT_FN inline
#include "gs_segsort_dev.h"

static const int TAIL = 1000;                                    // somebody else's words behind the segment

template <int LGC, bool F64>
static int run_case(int n, int pattern, unsigned seed)
{
    constexpr int GMAX = 4, C = 1 << LGC;
    std::mt19937_64 rng(seed);
    std::vector<gs_u64> g((size_t)n + TAIL), tail(TAIL);
    // the items the scatter writes: key << 31 | slot, bit 62 set with 24-bit keys (F64); every slot once, in a shuffled order
    std::vector<unsigned> slot(n);
    for (int i = 0; i < n; ++i) slot[i] = (unsigned)i;
    std::shuffle(slot.begin(), slot.end(), rng);
    const unsigned kmask = F64 ? 0xffffffu : 0xffffffffu;
    const unsigned one = (unsigned)rng() & kmask;
    for (int i = 0; i < n; ++i) {
        unsigned key = pattern == 0 ? (unsigned)rng() : (pattern == 1 ? ((unsigned)(rng() % 16) << 9) : one);
        if (!F64 && pattern == 0 && i % 3 == 0) key |= 0x80000000u;
        g[i] = (F64 ? (1ull << 62) : 0ull) | ((gs_u64)(key & kmask) << 31) | (gs_u64)slot[i];
    }
    for (int i = 0; i < TAIL; ++i) g[(size_t)n + i] = tail[i] = (i % 3 == 0) ? 0ull : (i % 3 == 1 ? ~0ull : (gs_u64)rng());   // would move if touched
    std::vector<gs_u64> want(g.begin(), g.begin() + n);
    std::sort(want.begin(), want.end());
    std::vector<gs_u64> lds((size_t)gs_seg_phys<true>(C) + 1, 0x5a5a5a5a5a5a5a5aull);
    std::vector<gs_u64> out(n, 0ull);
    std::vector<int> times(n, 0);
    bool bad_index = false;
    gs_seg_hybrid<GMAX, LGC, 1, F64>(lds.data(), g.data(), n, 0, [] {}, [&](int i, gs_u64 w) {
        if (i < 0 || i >= n) { bad_index = true; return; }
        out[i] = w; ++times[i];
    });
    if (bad_index) { std::printf("LGC %d F64 %d n %d pattern %d: emit outside [0, n)\n", LGC, (int)F64, n, pattern); return 1; }
    for (int i = 0; i < n; ++i)
        if (times[i] != 1 || out[i] != want[i]) {
            std::printf("LGC %d F64 %d n %d pattern %d: index %d emitted %d times, %llx against %llx\n", LGC, (int)F64, n, pattern, i, times[i],
                        (unsigned long long)out[i], (unsigned long long)want[i]);
            return 1;
        }
    for (int i = 0; i < TAIL; ++i)
        if (g[(size_t)n + i] != tail[i]) { std::printf("LGC %d F64 %d n %d pattern %d: word %d behind n changed\n", LGC, (int)F64, n, pattern, i); return 1; }
    return 0;
}

int main()
{
    const int ns[] = { 1, 15, 17, 2049, 4095, 4096, 4097, 5000, 8191, 8192, 8193, 12288, 12289, 16384, 16385, 20000, 40000 };
    int cases = 0;
    unsigned seed = 1;
    for (int n : ns)
        for (int pattern = 0; pattern < 3; ++pattern) {
            if (run_case<12, true>(n, pattern, seed++) || run_case<12, false>(n, pattern, seed++) ||
                run_case<13, true>(n, pattern, seed++) || run_case<13, false>(n, pattern, seed++) ||
                run_case<6, false>(n, pattern, seed++))                  // (64-word chunks: many rounds, every group width of the wide stages)
                return 1;
            cases += 5;
        }
    std::printf("ok %d\n", cases);
    return 0;
}
