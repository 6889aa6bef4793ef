// gs_segsort_dev.h -- the sorting network of the binning's segment sort (gs_sort.hip): a bitonic sort of n 64-bit words held in one
// workgroup's LDS (or in its own range of a global buffer), plain C++ so that a host program can step through the same index arithmetic.
//
// Network: merge sizes k = 2, 4, .. P (P = the power of two >= n); every merge is ONE "flip" stage (i against i ^ (k - 1)) followed by
// half-cleaners of stride k/4 .. 1.  In this form EVERY comparator is ascending (the smaller word goes to the smaller index), so a word
// of +infinity at an index >= n never moves.  The cost is fixed by n alone -- all-equal keys take exactly the comparators of any other
// input.  Two ways to hold the padding (template GUARD):
//   GUARD = false  the buffer holds P words and the caller filled [n, P) with infinities: no index is ever checked;
//   GUARD = true   the buffer holds n words (a range of a global array, with somebody else's words behind it): a word behind n is
//                  neither loaded nor stored.
// Either way a virtual thread whose smallest index is >= n holds nothing but infinities and is skipped, so the work follows n, not P.
//
// A stage needs no barrier against the stages that pair the SAME words, so up to GMAX consecutive stages run on 2^GMAX words in
// registers between two barriers ("group"): the stride bits a .. a+G-1 of a group index the register, the bits below (lo) and above
// (hi) pick the virtual thread.  The flip leads a group: its partner also mirrors the bits below a, so the upper half of the registers
// is loaded from lo ^ (2^a - 1).  The merges up to 2^GMAX run in one go on 2^GMAX consecutive words.  GMAX = 4: 18 LDS round trips for
// 2 048 words instead of 66 stages.
#pragma once
#include <stdint.h>

#ifndef GS_SEGSORT_FN
#define GS_SEGSORT_FN __device__ __forceinline__
#endif

typedef unsigned long long gs_u64;

// LDS index of word i: one word of padding per 32 keeps the consecutive-words-per-lane access of the a = 0 groups off one bank
template <bool PAD>
GS_SEGSORT_FN int gs_seg_phys(int i) { return PAD ? i + (i >> 5) : i; }

// Compare-exchange.  F64: the words are bit patterns of positive, normal doubles (bit 63 clear, bit 62 set, bits 61..52 not all ones --
// the caller's composite of a 24-bit key guarantees it), whose order as doubles is their order as integers: v_min_f64 / v_max_f64
// return one operand unchanged, two instructions instead of a 64-bit compare and four selects.  +infinity is the padding word then.
template <bool F64>
GS_SEGSORT_FN gs_u64 gs_seg_inf() { return F64 ? 0x7ff0000000000000ull : ~0ull; }

template <bool F64>
GS_SEGSORT_FN void gs_seg_cx(gs_u64& a, gs_u64& b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (F64) {
        const double x = __builtin_bit_cast(double, a), y = __builtin_bit_cast(double, b);
        double lo, hi;
        asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(x), "v"(y));
        asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(x), "v"(y));
        a = __builtin_bit_cast(gs_u64, lo); b = __builtin_bit_cast(gs_u64, hi);
        return;
    }
#endif
    const gs_u64 lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo; b = hi;
}

// every merge k = 2 .. 2^F of 2^F consecutive words, in registers
template <int F, bool PAD, bool F64, bool GUARD>
GS_SEGSORT_FN void gs_seg_first(gs_u64* buf, int n, int P, int tid, int nthreads)
{
    constexpr int R = 1 << F;
    for (int v = tid; v < (P >> F); v += nthreads) {
        const int base = v << F;
        if (base >= n) break;
        gs_u64 e[R];
#pragma unroll
        for (int r = 0; r < R; ++r) e[r] = (!GUARD || base + r < n) ? buf[gs_seg_phys<PAD>(base + r)] : gs_seg_inf<F64>();
#pragma unroll
        for (int lgk = 1; lgk <= F; ++lgk) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r < (r ^ ((1 << lgk) - 1))) gs_seg_cx<F64>(e[r], e[r ^ ((1 << lgk) - 1)]);
#pragma unroll
            for (int s = lgk - 2; s >= 0; --s) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if ((r & (1 << s)) == 0) gs_seg_cx<F64>(e[r], e[r | (1 << s)]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) if (!GUARD || base + r < n) buf[gs_seg_phys<PAD>(base + r)] = e[r];
    }
}

// G consecutive stages (stride bits a + G - 1 .. a) on 2^G words per virtual thread; flip: the first of them is the flip of its merge
template <int G, bool PAD, bool F64, bool GUARD>
GS_SEGSORT_FN void gs_seg_group(gs_u64* buf, int n, int P, int a, bool flip, int tid, int nthreads)
{
    constexpr int R = 1 << G, H = R >> 1;
    const int jmask = (1 << a) - 1;
    for (int v = tid; v < (P >> G); v += nthreads) {
        const int base = ((v >> a) << (a + G)) | (v & jmask);
        if (base >= n) break;                                    // (the smallest index of v, ascending in v: nothing but infinities from here)
        const int base2 = flip ? (base ^ jmask) : base;
        gs_u64 e[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = (r >= H ? base2 : base) + (r << a);
            e[r] = (!GUARD || i < n) ? buf[gs_seg_phys<PAD>(i)] : gs_seg_inf<F64>();
        }
        if (flip) {
#pragma unroll
            for (int r = 0; r < H; ++r) gs_seg_cx<F64>(e[r], e[R - 1 - r]);
        } else {
#pragma unroll
            for (int r = 0; r < H; ++r) gs_seg_cx<F64>(e[r], e[r + H]);
        }
#pragma unroll
        for (int s = G - 2; s >= 0; --s) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if ((r & (1 << s)) == 0) gs_seg_cx<F64>(e[r], e[r | (1 << s)]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = (r >= H ? base2 : base) + (r << a);
            if (!GUARD || i < n) buf[gs_seg_phys<PAD>(i)] = e[r];
        }
    }
}

template <int GMAX, bool PAD, bool F64, bool GUARD>
GS_SEGSORT_FN void gs_seg_group_n(int g, gs_u64* buf, int n, int P, int a, bool flip, int tid, int nthreads)
{
    if (g == GMAX) gs_seg_group<GMAX, PAD, F64, GUARD>(buf, n, P, a, flip, tid, nthreads);
    else if constexpr (GMAX > 1) gs_seg_group_n<GMAX - 1, PAD, F64, GUARD>(g, buf, n, P, a, flip, tid, nthreads);
}

// Whole sort.  BARRIER separates the groups (a workgroup barrier on the device).  P: power of two, >= n and >= 2^GMAX.
#define GS_SEG_SORT_BODY(GMAX, PAD, F64, GUARD, buf, n, P, tid, nthreads, BARRIER)                           \
    do {                                                                                                     \
        gs_seg_first<GMAX, PAD, F64, GUARD>(buf, n, P, tid, nthreads);                                       \
        BARRIER;                                                                                             \
        for (int k_ = 2 << (GMAX), lgk_ = (GMAX) + 1; k_ <= (P); k_ <<= 1, ++lgk_) {                         \
            int rem_ = lgk_;                                                                                 \
            bool flip_ = true;                                                                               \
            while (rem_ > 0) {                                                                               \
                const int g_ = flip_ ? ((rem_ - 1) % (GMAX)) + 1 : (GMAX);                                   \
                gs_seg_group_n<GMAX, PAD, F64, GUARD>(g_, buf, n, P, rem_ - g_, flip_, tid, nthreads);       \
                BARRIER;                                                                                     \
                rem_ -= g_;                                                                                  \
                flip_ = false;                                                                               \
            }                                                                                                \
        }                                                                                                    \
    } while (0)

// Hybrid: the same network for a segment of ANY length n held in a global range g[0, n), by one workgroup of NT threads with an LDS
// buffer of one chunk, C = 2^LGC words (gs_seg_phys<true>(C) + 1 words of LDS).  P = the power of two >= n.
//   n <= C   load, pad to P, sort in LDS, emit.
//   n >  C   the merges k <= C stay inside the aligned chunks: every chunk that begins below n is loaded (indices >= n padded with
//            infinities), sorted in LDS, unguarded, and stored back.  A merge k = 2^lgk > C then runs its stages of stride bits
//            lgk-1 .. LGC as guarded register groups directly on g (the flip leads, up to GMAX stages per round trip), and its last
//            LGC stages (half-cleaners of stride C/2 .. 1, chunk-local again) per chunk in LDS: load, the groups, store.
//            The chunk pass of the last merge emits from LDS instead of storing back.
// The comparators are exactly those of GS_SEG_SORT_BODY for the same P, in the same stage order, so the result is the same word for
// word; a word behind n is neither loaded nor stored.  bar() separates the groups and the loads / stores of a chunk from them (a
// workgroup barrier on the device: every call sits in control flow that depends on n, LGC and GMAX alone).  emit(i, word) receives
// every sorted word once, i in [0, n).
template <int GMAX, int LGC, int NT, bool F64, class Barrier, class Emit>
GS_SEGSORT_FN void gs_seg_hybrid(gs_u64* lds, gs_u64* g, int n, int tid, Barrier bar, Emit emit)
{
    static_assert(LGC > GMAX, "a chunk holds more than one group");
    constexpr int C = 1 << LGC;
    if (n <= C) {
        int P = 1 << GMAX;
        while (P < n) P <<= 1;
        for (int i = tid; i < P; i += NT) lds[gs_seg_phys<true>(i)] = i < n ? g[i] : gs_seg_inf<F64>();
        bar();
        GS_SEG_SORT_BODY(GMAX, true, F64, false, lds, n, P, tid, NT, bar());
        for (int i = tid; i < n; i += NT) emit(i, lds[gs_seg_phys<true>(i)]);
        return;
    }
    int lgP = LGC + 1;
    while ((1ll << lgP) < (long long)n) ++lgP;
    // merges k <= C, chunk by chunk (a short last chunk takes the network of its own power of two: the merges above it meet nothing
    // but infinities in their upper halves and a sorted lower half, so none of their comparators would move a word)
    for (int cb = 0; cb < n; cb += C) {
        const int nl = n - cb < C ? n - cb : C;
        int Pl = 1 << GMAX;
        while (Pl < nl) Pl <<= 1;
        for (int i = tid; i < Pl; i += NT) lds[gs_seg_phys<true>(i)] = i < nl ? g[cb + i] : gs_seg_inf<F64>();
        bar();
        GS_SEG_SORT_BODY(GMAX, true, F64, false, lds, nl, Pl, tid, NT, bar());
        for (int i = tid; i < nl; i += NT) g[cb + i] = lds[gs_seg_phys<true>(i)];
        bar();
    }
    const int P = 1 << lgP;
    for (int lgk = LGC + 1; lgk <= lgP; ++lgk) {
        int rem = lgk;
        bool flip = true;
        while (rem > LGC) {                                      // global stages, stride bits rem-1 .. rem-gg
            const int gg = flip ? ((rem - LGC - 1) % GMAX) + 1 : GMAX;
            gs_seg_group_n<GMAX, false, F64, true>(gg, g, n, P, rem - gg, flip, tid, NT);
            bar();
            rem -= gg;
            flip = false;
        }
        const bool last = lgk == lgP;
        for (int cb = 0; cb < n; cb += C) {                      // stride bits LGC-1 .. 0
            const int nl = n - cb < C ? n - cb : C;
            for (int i = tid; i < C; i += NT) lds[gs_seg_phys<true>(i)] = i < nl ? g[cb + i] : gs_seg_inf<F64>();
            bar();
            for (int r = LGC; r > 0;) {
                const int gg = ((r - 1) % GMAX) + 1;
                gs_seg_group_n<GMAX, true, F64, false>(gg, lds, nl, C, r - gg, false, tid, NT);
                bar();
                r -= gg;
            }
            if (last) { for (int i = tid; i < nl; i += NT) emit(cb + i, lds[gs_seg_phys<true>(i)]); }
            else      { for (int i = tid; i < nl; i += NT) g[cb + i] = lds[gs_seg_phys<true>(i)]; }
            bar();
        }
    }
}
