// gs_sort.hip -- A2 + A3: tile binning and the stable (tile | depth) order of the intersections, hand-written for gfx950.
// Semantics: gsplat 1.4 `isect_tiles(sort=True)` as reached from rfstudio/model/gsplat.py:334 -- keys
// (tile_id << 32) | float_bits(depth), payload = packed Gaussian index, stable ascending radix sort, so that equal keys
// keep their emission order (= ascending packed index); that order fixes the composited order bit-exactly.
//
// Three entry points (no vendor sort library on any path):
//   gs_isect_bin_front : what the engine uses.  The front kernel has counted the intersections per tile, so every tile's segment of
//                   the output is known before anything is sorted: the intersections are scattered, in packed order, straight into
//                   their tile's segment, and one workgroup per tile sorts its segment on chip by (depth key, packed index) -- a
//                   bitonic network in LDS (gs_segsort_dev.h), no pass over the whole list.  See the block above the function.
//                   Without the per-tile counts (more than 8 192 tiles) it falls back to the radix machinery below.
//   gs_isect_sort : the upstream call shape -- sorts already emitted (isect_ids, flatten_ids) pairs, six 8-bit passes
//                   over the 32 + tile_bits significant key bits (kept for callers that hold emitted keys);
//   gs_isect_bin  : what rasterization() uses.  The 44-bit key of an intersection is (tile, depth of
//                   its Gaussian): the depth half is a property of the V Gaussians, not of the I = 2.1 V intersections,
//                   so it is sorted ONCE on the Gaussians (4 passes over 8-byte (depth, index) items, V-sized), the
//                   intersections are then EMITTED in depth order as 8-byte (tile, index) items, and two stable passes
//                   over the tile bits (6 + 6 for 2 500 tiles) finish the order: 2 I-sized passes of 8-byte items instead
//                   of 6 passes of 12-byte pairs, and the unsorted key array is never materialised.  Stability of every
//                   pass makes the result identical to the upstream order: by tile, then depth bits, then packed index.
//
// One radix pass = three kernels: per-block digit histogram -> exclusive scan of the [digit][block] table -> scatter.
// A block owns 4 096 consecutive items, a wave 1 024 of them (striped over its lanes: coalesced, and wave-major order =
// index order), and ranks them with ballots: for every item the lanes holding the same digit are found with one ballot
// per digit bit, the rank inside the wave is a popcount, and one lane per digit group advances the wave's running
// counter in LDS -- no sorting network, no atomics.
#include "gs_common.h"
#include "gs_segsort_dev.h"
#include "gs_ws.h"

#include <cstdlib>
#include <cstring>

#define RS_THREADS 256
#define RS_WAVES 4
#define RS_ITEMS 8                        // per thread.  16 until the end of round 4: alone the passes take the same time, inside the
                                          // step the 22 KB blocks find room beside the compositor's (39 KB blocks did not): 659 -> 669
                                          // views/s (4: 664, 12: 662)
#define RS_TILE (RS_THREADS * RS_ITEMS)   // 2048 items per block
#define RS_WCHUNK (64 * RS_ITEMS)         // 512 items per wave

typedef unsigned long long u64;

static int tile_bits(int tile_w, int tile_h)
{
    unsigned n = (unsigned)(tile_w * tile_h);       // floor(log2(n_tiles)) + 1, as upstream
    int b = 0;
    while (n > 1) { n >>= 1; ++b; }
    return b + 1;
}

// ---- item kinds ----------------------------------------------------------------------------------------------------
struct PairItem { u64 key; int32_t val; };                      // emitted (isect_id, flatten_id)
struct PairIn {
    const u64* keys; const int32_t* vals;
    __device__ __forceinline__ PairItem load(int64_t i) const { return PairItem{ keys[i], vals[i] }; }
};
struct PairOut {
    u64* keys; int32_t* vals;
    __device__ __forceinline__ void store(int64_t i, const PairItem& it) const { keys[i] = it.key; vals[i] = it.val; }
};
struct PairDigit {
    int shift; unsigned mask;
    __device__ __forceinline__ unsigned operator()(const PairItem& it) const { return (unsigned)(it.key >> shift) & mask; }
};

struct U2In {
    const uint2* p;
    __device__ __forceinline__ uint2 load(int64_t i) const { return p[i]; }
};
struct U2Out {
    uint2* p;
    __device__ __forceinline__ void store(int64_t i, const uint2& it) const { p[i] = it; }
};
struct DepthIn {                                                   // (depth bits, packed index) straight from the depth array
    const float* depths;
    __device__ __forceinline__ uint2 load(int64_t i) const { return make_uint2(__float_as_uint(depths[i]), (unsigned)i); }
};
struct XDigit {                                                    // digit of .x
    int shift; unsigned mask;
    __device__ __forceinline__ unsigned operator()(const uint2& it) const { return (it.x >> shift) & mask; }
};
struct FinalTiles {                                                // last tile pass without the 64-bit keys: (tile id, flatten id) as two int32 arrays
    int32_t* tile_ids; int32_t* flatten_ids;
    __device__ __forceinline__ void store(int64_t i, const uint2& it) const
    {
        flatten_ids[i] = (int32_t)it.y;
        tile_ids[i] = (int32_t)it.x;
    }
};
struct FinalOut {                                                  // last tile pass: the two sorted meta arrays
    u64* isect_ids; int32_t* flatten_ids; const float* depths;
    __device__ __forceinline__ void store(int64_t i, const uint2& it) const
    {
        flatten_ids[i] = (int32_t)it.y;
        isect_ids[i] = ((u64)it.x << 32) | (u64)__float_as_uint(depths[it.y]);
    }
};

// ---- pass kernels --------------------------------------------------------------------------------------------------
template <typename Item, typename In, typename Digit>
__global__ void __launch_bounds__(RS_THREADS)
radix_hist_kernel(GsCount nc, In in, Digit digit, int nbins, int nblocks, unsigned* __restrict__ table)
{
    const int64_t n = gs_count(nc);
    __shared__ unsigned hist[256];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RS_TILE;
#pragma unroll 4
    for (int k = 0; k < RS_ITEMS; ++k) {
        const int64_t i = base + (int64_t)k * RS_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&hist[digit(in.load(i))], 1u);
    }
    __syncthreads();
    if ((int)threadIdx.x < nbins) table[(size_t)threadIdx.x * nblocks + blockIdx.x] = hist[threadIdx.x];
}

// Offsets of a pass: table[d][b] (items of digit d in block b) -> exclusive prefix along b inside every digit row (one workgroup
// per digit, coalesced row) and the row totals; the scatter blocks scan the (<= 256) row totals themselves and add the two.  (A single workgroup scanning the whole 260 k-entry table was a 50 us latency chain per pass.)
__global__ void __launch_bounds__(256)
radix_rowscan_kernel(int nblocks, unsigned* __restrict__ table, unsigned* __restrict__ row_total)
{
    __shared__ unsigned wsum[4];
    unsigned* row = table + (size_t)blockIdx.x * nblocks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned carry = 0u;
    for (int i0 = 0; i0 < nblocks; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const unsigned v = i < nblocks ? row[i] : 0u;
        unsigned incl = v;
        incl = gs_wave_incl_scan(incl);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned before = 0u, all = 0u;
        for (int w = 0; w < 4; ++w) { if (w < wave) before += wsum[w]; all += wsum[w]; }
        if (i < nblocks) row[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) row_total[blockIdx.x] = carry;
}

// Scatter of one pass.  Ranks come from ballots (see the file header); the items are then staged through LDS in their
// block-local sorted order, so that the global stores of a digit run are contiguous (a wave writing 64 items of 64 different
// digits straight from registers is 64 partial-sector stores).
template <typename Item, typename In, typename Digit, typename Out, int NBITS>
__global__ void __launch_bounds__(RS_THREADS)
radix_scatter_kernel(GsCount nc, In in, Digit digit, int nblocks, const unsigned* __restrict__ table,
                     const unsigned* __restrict__ row_total, Out out)
{
    const int64_t n = gs_count(nc);
    constexpr int NB = 1 << NBITS;
    __shared__ unsigned cnt[RS_WAVES][NB];
    __shared__ unsigned dstart[NB];                              // start of digit d inside the block's sorted order
    __shared__ unsigned gbase[NB];                               // global position of that start
    __shared__ Item stage[RS_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < RS_WAVES * NB; i += RS_THREADS) (&cnt[0][0])[i] = 0u;
    __syncthreads();
    const int64_t bbase = (int64_t)blockIdx.x * RS_TILE;
    const int64_t wbase = bbase + (int64_t)wave * RS_WCHUNK;
    const int n_here = (n - bbase) < RS_TILE ? (int)((n - bbase) > 0 ? (n - bbase) : 0) : RS_TILE;
    const u64 lane_lt = (1ull << lane) - 1ull;
    Item item[RS_ITEMS];
    unsigned dig[RS_ITEMS];
    unsigned rank[RS_ITEMS];
#pragma unroll
    for (int k = 0; k < RS_ITEMS; ++k) {
        const int64_t i = wbase + (int64_t)k * 64 + lane;
        const bool valid = i < n;
        if (valid) item[k] = in.load(i);
        const unsigned d = valid ? digit(item[k]) : 0u;
        u64 m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < NBITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 bal = __ballot(bit);
            m &= bit ? bal : ~bal;
        }
        const unsigned old = cnt[wave][d];                       // running count of this wave for digit d (same for the group)
        __builtin_amdgcn_wave_barrier();
        const unsigned r = __popcll(m & lane_lt);
        if (valid && r == 0u) cnt[wave][d] = old + (unsigned)__popcll(m);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        dig[k] = d;
        rank[k] = old + r;
    }
    __syncthreads();
    // block-local start of every digit (exclusive scan of the digit totals by the first NB threads) and its global position
    {
        const int d = threadIdx.x;
        unsigned tot = 0u;
        if (d < NB) for (int w = 0; w < RS_WAVES; ++w) tot += cnt[w][d];
        unsigned incl = tot;
        incl = gs_wave_incl_scan(incl);
        __shared__ unsigned wtot[RS_WAVES];
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        unsigned before = 0u;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        if (d < NB) dstart[d] = before + incl - tot;
        // global start of digit d = exclusive prefix of the row totals (256 values: every block scans them itself, which
        // saves a kernel per pass) + this block's offset inside the row
        __syncthreads();
        const unsigned rt = d < NB ? row_total[d] : 0u;
        unsigned rincl = rt;
        rincl = gs_wave_incl_scan(rincl);
        if (lane == 63) wtot[wave] = rincl;
        __syncthreads();
        unsigned rbefore = 0u;
        for (int w = 0; w < wave; ++w) rbefore += wtot[w];
        if (d < NB) gbase[d] = rbefore + rincl - rt + table[(size_t)d * nblocks + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RS_ITEMS; ++k) {
        const int64_t i = wbase + (int64_t)k * 64 + lane;
        if (i < n) {
            const unsigned d = dig[k];
            unsigned off = dstart[d] + rank[k];
            for (int w = 0; w < wave; ++w) off += cnt[w][d];
            stage[off] = item[k];
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < RS_ITEMS; ++k) {
        const int p = k * RS_THREADS + (int)threadIdx.x;
        if (p < n_here) {
            const Item it = stage[p];
            const unsigned d = digit(it);
            out.store((int64_t)gbase[d] + (int64_t)(p - (int)dstart[d]), it);
        }
    }
}

template <typename Item, typename In, typename Digit, typename Out>
static int radix_pass(GsCount nc, In in, Digit digit, Out out, int nbits, unsigned* table, hipStream_t s)
{
    const int64_t n = nc.n;                                      // capacity: the grid and the table rows are sized by it
    const int nblocks = (int)((n + RS_TILE - 1) / RS_TILE);
    const int nbins = 1 << nbits;
    unsigned* row_total = table + (size_t)256 * nblocks;        // [256] + [256] behind the table
    hipLaunchKernelGGL((radix_hist_kernel<Item, In, Digit>), dim3(nblocks), dim3(RS_THREADS), 0, s, nc, in, digit, nbins, nblocks, table);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(radix_rowscan_kernel, dim3(nbins), dim3(256), 0, s, nblocks, table, row_total);
    GS_CHECK_LAUNCH();
    switch (nbits) {
#define RS_CASE(B) case B: hipLaunchKernelGGL((radix_scatter_kernel<Item, In, Digit, Out, B>), dim3(nblocks), dim3(RS_THREADS), 0, s, nc, in, digit, nblocks, table, row_total, out); break;
        RS_CASE(1) RS_CASE(2) RS_CASE(3) RS_CASE(4) RS_CASE(5) RS_CASE(6) RS_CASE(7) RS_CASE(8)
#undef RS_CASE
        default: gs_set_error("radix_pass: bad digit width %d", nbits); return GS_EINVAL;
    }
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// Workspaces (gs_ws.h): one function per layout gives the size (base == nullptr) and the pointers.  Every layout here ends in 256
// bytes that are no segment: nothing in this file addresses them, they stay because callers allocate and cache by these sizes.
static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }       // the tile-first path of gs_isect_bin_front still rounds by hand
static size_t table_words(int64_t n) { return (size_t)256 * (size_t)((n + RS_TILE - 1) / RS_TILE + 1) + 512; }   // [digit][block] + the row totals

// ---- gs_isect_sort: the upstream call shape ---------------------------------------------------------------------
struct SortWs { unsigned* table; u64* keys; int32_t* vals; size_t bytes; };
static SortWs sort_ws(void* base, int64_t n_isects)
{
    GsWs w(base, 256);
    SortWs r;
    r.table = w.take<unsigned>(table_words(n_isects));
    r.keys = w.take<u64>((size_t)n_isects);
    r.vals = w.take<int32_t>((size_t)n_isects);
    w.pad(256);
    r.bytes = w.bytes();
    return r;
}
extern "C" size_t gs_sort_ws_bytes(int64_t n_isects, int tile_w, int tile_h)
{
    if (n_isects <= 0) return 0;
    (void)tile_w; (void)tile_h;
    return sort_ws(nullptr, n_isects).bytes;
}

extern "C" int gs_isect_sort(int64_t n_isects, const int64_t* isect_ids, const int32_t* flatten_ids,
                             int64_t* isect_ids_sorted, int32_t* flatten_ids_sorted, int tile_w, int tile_h,
                             void* ws, size_t ws_bytes, void* stream)
{
    GS_CHECK_ARG(n_isects >= 0 && tile_w > 0 && tile_h > 0, "bad sizes");
    if (n_isects == 0) return GS_OK;
    GS_CHECK_ARG(ws != nullptr, "workspace must not be NULL");
    const SortWs w = sort_ws(ws, n_isects);
    if (ws_bytes < w.bytes) { gs_set_error("gs_isect_sort: workspace too small"); return GS_ENOSPC; }
    hipStream_t s = (hipStream_t)stream;
    const int end_bit = 32 + tile_bits(tile_w, tile_h);
    const int npass = (end_bit + 7) / 8;
    // ping-pong so that the LAST pass lands in the caller's output: pass parity decides where the first one goes
    const u64* src_k = (const u64*)isect_ids; const int32_t* src_v = flatten_ids;
    for (int pass = 0; pass < npass; ++pass) {
        const int shift = pass * 8;
        const int nbits = (end_bit - shift) < 8 ? (end_bit - shift) : 8;
        const bool to_out = ((npass - 1 - pass) % 2) == 0;
        u64* dk = to_out ? (u64*)isect_ids_sorted : w.keys;
        int32_t* dv = to_out ? flatten_ids_sorted : w.vals;
        const int rc = radix_pass<PairItem>(GsCount{ n_isects, nullptr }, PairIn{ src_k, src_v }, PairDigit{ shift, (1u << nbits) - 1u }, PairOut{ dk, dv }, nbits, w.table, s);
        if (rc != GS_OK) return rc;
        src_k = dk; src_v = dv;
    }
    return GS_OK;
}

// ---- gs_isect_bin: depth-major binning --------------------------------------------------------------------------
// emission in depth order.  tile_range_exact == gs_project.hip (same operation order: the counts come from there)
__device__ __forceinline__ void tile_range_sorted(float mx, float my, int radius, int tile_size, int tw, int th,
                                                  int& x0, int& y0, int& x1, int& y1)
{
#pragma clang fp contract(off)
    const float ts = (float)tile_size;
    const float tr = (float)radius / ts;
    const float tx = mx / ts, ty = my / ts;
    const float fx0 = floorf(tx - tr), fy0 = floorf(ty - tr);
    const float fx1 = ceilf(tx + tr), fy1 = ceilf(ty + tr);
    x0 = fx0 < 0.0f ? 0 : (fx0 > (float)tw ? tw : (int)fx0);
    y0 = fy0 < 0.0f ? 0 : (fy0 > (float)th ? th : (int)fy0);
    x1 = fx1 < 0.0f ? 0 : (fx1 > (float)tw ? tw : (int)fx1);
    y1 = fy1 < 0.0f ? 0 : (fy1 > (float)th ? th : (int)fy1);
}

#define EM_THREADS 256
#define EM_PER 4                             // ranks per thread (2 and 8 measured: DESIGN.md section 6)
#define EM_LOOK 4                            // x 64 predecessors per look-back round
#define EM_TILE (EM_THREADS * EM_PER)        // ranks per block

// tile rectangle of every visible Gaussian, packed (x0 | y0 << 16, x1 | y1 << 16): computed once in packed order (coalesced) so
// that the two depth-order kernels below gather ONE 8-byte word per Gaussian instead of means2d + radii + tiles_per_gauss
__global__ void __launch_bounds__(256)
tile_rect_kernel(GsCount vc, const float* __restrict__ means2d, const int32_t* __restrict__ radii, int tile_size, int tile_w, int tile_h,
                 uint2* __restrict__ rect)
{
    const int V = (int)gs_count(vc);
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float2 m = *reinterpret_cast<const float2*>(means2d + 2 * (size_t)v);
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    const int r = radii[v];
    if (r > 0) tile_range_sorted(m.x, m.y, r, tile_size, tile_w, tile_h, x0, y0, x1, y1);
    rect[v] = make_uint2((unsigned)x0 | ((unsigned)y0 << 16), (unsigned)x1 | ((unsigned)y1 << 16));
}
__device__ __forceinline__ unsigned rect_count(uint2 q)
{
    const int w = (int)(q.y & 0xffffu) - (int)(q.x & 0xffffu), h = (int)(q.y >> 16) - (int)(q.x >> 16);
    return (w > 0 && h > 0) ? (unsigned)(w * h) : 0u;
}

// scratch of the radix machinery (gs_isect_bin and the radix path of gs_isect_bin_front): the pass table, the (key, index) items of
// the depth order, the emission's look-back state, the (tile, index) items of the tile split; `rect` only where the rectangles are
// computed here, `tile_ids` only where the tile offsets are derived from the sorted ids
struct RadixWs { unsigned* table; uint2 *da, *db, *rect; unsigned* state; uint2 *ia, *ib; int32_t* tile_ids; int n_state_words; size_t bytes; };
static RadixWs radix_ws(void* base, size_t v, size_t n, bool rect, bool tile_ids)
{
    GsWs w(base, 256);
    RadixWs r;
    r.table = w.take<unsigned>(table_words((int64_t)(v > n ? v : n)));
    r.da = w.take<uint2>(v);
    r.db = w.take<uint2>(v);
    r.rect = rect ? w.take<uint2>(v) : nullptr;
    // ticket + error flag (16 bytes), then two u64 rows of one word per emission block + 1
    r.n_state_words = (int)(gs_align_up(16 + 2 * (size_t)(((int)v + EM_TILE - 1) / EM_TILE + 1) * sizeof(u64), 256) / 4);
    r.state = w.take<unsigned>((size_t)r.n_state_words);
    r.ia = w.take<uint2>(n);
    r.ib = w.take<uint2>(n);
    r.tile_ids = tile_ids ? w.take<int32_t>(n) : nullptr;
    w.pad(256);
    r.bytes = w.bytes();
    return r;
}

extern "C" size_t gs_isect_bin_ws_bytes(int V, int64_t n_isects, int tile_w, int tile_h)
{
    (void)tile_w; (void)tile_h;
    return radix_ws(nullptr, V > 0 ? (size_t)V : 1, n_isects > 0 ? (size_t)n_isects : 1, true, false).bytes;
}

// status word of the capacity protocol: {code, required n_isects}; written only on overflow (the caller zeroes it once)
__global__ void capacity_check_kernel(const long long* __restrict__ counts, long long v_cap, long long i_cap, long long* __restrict__ status)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long V = counts[0], I = counts[1];
    if (V > v_cap || I > i_cap) {
        status[0] = GS_ENOSPC;
        if (I > status[1]) status[1] = I;
        if (V > status[2]) status[2] = V;
    }
}

// ---- gs_isect_bin_front: binning of the engine's fused front ---------------------------------------------------------------------
// Same result as gs_isect_bin_tiles_cap + gs_isect_offsets_tiles_cap -- `flatten_ids` in (tile, depth bits, packed index) order and the
// per-tile offsets, bit for bit -- from what gs_front_fwd leaves behind: depth keys (24 bits wide when the engine knows the view's
// depth range, key = depth bits - key_base, checked by the front kernel), packed tile rectangles, and the intersections counted per TILE.
//
// Tile first (tile_counts given, <= BF_HIST_MAX tiles: the engine's path).  The counters fix every tile's segment of the output before
// anything is sorted, so no pass over the whole list is needed:
//   offsets  tile_offsets_scan_kernel   exclusive scan of the counters, clamped to the capacity; files the tiles by segment length;
//                                       clears the per-tile cursors; capacity check
//   scatter  bin_scatter_kernel         packed slots in order -> {key, slot} items into their tile's segment, any order inside it
//   sort     seg_sort_kernel,           one workgroup per tile sorts its segment by (key, slot) and writes the slots: up to 2 048 items
//            seg_sort_large_kernel      and up to 8 192 in LDS, longer ones chunk by chunk in LDS with the wide stages in place
// 4 launches, I * 8 bytes of scratch.  The items are written once and read once (about 27 MB each way for the bench view's 3.4 M
// intersections, next to 24 MB of keys and rectangles in and 14 MB of ids out); the radix path moved ~0.6 GB for the same list.  No
// kernel waits for another workgroup, every clear is a kernel, nothing is read back: capturable as it stands.
//
// Radix (no tile_counts, or more tiles than a block's LDS holds): key_bits / 8 V-sized depth passes, the emission in depth order with
// its in-launch chained scan, two or three stable passes over the tile bits that keep the tile ids, and the offsets from those.
// Round 6, built, bit-identical, measured and removed (`git show 3d98652:geosplatting_amd/csrc/gs_sort.hip`): every radix pass as ONE
// kernel -- ticketed blocks publish {flag | count} rows, offsets from a two-level look-back -- 9 launches instead of 18, 281 against
// 252 us per view alone, 640 against 649 views/s inside the step: the look-back cost more than the kernel boundaries it removed.
struct KeyIn {                                                     // (depth key, packed index) straight from the key array
    const unsigned* keys;
    __device__ __forceinline__ uint2 load(int64_t i) const { return make_uint2(keys[i], (unsigned)i); }
};
#define BF_HIST_MAX 8192                     // tiles whose counters fit a block's LDS (32 KB): the front kernel's histogram, the scatter's cursors

__global__ void __launch_bounds__(256)
bin_setup_kernel(unsigned* __restrict__ state, int n_state_words,
                 const long long* __restrict__ counts, long long v_cap, long long i_cap, long long* __restrict__ status)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int k = i; k < n_state_words; k += stride) state[k] = 0u;
    if (i == 0 && counts != nullptr && status != nullptr) {                        // capacity protocol, as capacity_check_kernel
        const long long V = counts[0], I = counts[1];
        if (V > v_cap || I > i_cap) {
            status[0] = GS_ENOSPC;
            if (I > status[1]) status[1] = I;
            if (V > status[2]) status[2] = V;
        }
    }
}

#define BF_VALID (1ull << 63)
#define BF_SPIN_LIMIT (1 << 22)

// thread r (depth rank) writes the (tile, index) items of its Gaussian at the exclusive prefix of the tile counts in depth order; the
// prefix across blocks is a decoupled look-back (blocks numbered by ticket, so a block only waits for blocks that already run)
__global__ void __launch_bounds__(EM_THREADS)
emit_chained_kernel(GsCount vc, const uint2* __restrict__ order, const uint2* __restrict__ rect, unsigned* __restrict__ ctrl,
                    u64* __restrict__ desc, int n_blocks, int tile_w, uint2* __restrict__ items, unsigned item_cap,
                    long long* __restrict__ status /* nullable: capacity protocol word */)
{
    const int V = (int)gs_count(vc);
    __shared__ unsigned ws[EM_THREADS / 64];
    __shared__ unsigned s_block;
    __shared__ unsigned long long s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_block = atomicAdd(ctrl, 1u);
    __syncthreads();
    const int block = (int)s_block;
    u64* agg = desc; u64* pre = desc + n_blocks;
    // blocked arrangement: thread t owns ranks base + t*EM_PER .. +EM_PER-1 (consecutive: the scan stays in index order)
    const int r0 = block * EM_TILE + (int)threadIdx.x * EM_PER;
    int v[EM_PER]; unsigned c[EM_PER]; uint2 q[EM_PER];
    unsigned mine = 0u;
#pragma unroll
    for (int k = 0; k < EM_PER; ++k) {
        const int r = r0 + k;
        v[k] = r < V ? (int)order[r].y : -1;
        q[k] = v[k] >= 0 ? rect[v[k]] : make_uint2(0u, 0u);
        c[k] = rect_count(q[k]);
        mine += c[k];
    }
    unsigned incl = mine;
    incl = gs_wave_incl_scan(incl);
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    unsigned before = 0u, total = 0u;
    for (int w = 0; w < EM_THREADS / 64; ++w) { if (w < wave) before += ws[w]; total += ws[w]; }
    if (wave == 0) {
        // look-back over EM_LOOK x 64 predecessors per round, nearest first: every lane has EM_LOOK descriptor pairs in flight and
        // keeps a private partial sum; ONE wave reduction at the end.  (All 1 920 blocks of a 2 M-Gaussian view are resident at once
        // and publish their aggregates together: nobody has a prefix yet, and block b walks all the way back -- b / 64 rounds of
        // dependent L2 round trips with a 64-bit wave sum each was most of this kernel's 84 us, round 6.)
        unsigned long long acc = 0ull;
        if (block > 0) {
            if (lane == 0) __hip_atomic_store(&agg[block], (u64)total | BF_VALID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int pos = block - 1;
            bool done = false;
            while (!done) {
                u64 pv[EM_LOOK], av[EM_LOOK];
#pragma unroll
                for (int j = 0; j < EM_LOOK; ++j) {
                    const int idx = pos - 64 * j - lane;
                    pv[j] = av[j] = 0ull;
                    if (idx >= 0) {
                        pv[j] = __hip_atomic_load(&pre[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        av[j] = __hip_atomic_load(&agg[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
#pragma unroll
                for (int j = 0; j < EM_LOOK; ++j) {
                    if (done) break;                         // (wave-uniform: the groups behind the first prefix are neither awaited nor summed)
                    const int idx = pos - 64 * j - lane;
                    bool isP = idx < 0;                      // (virtual predecessors before block 0: prefix 0)
                    u64 val = 0ull;
                    if (idx >= 0) {
                        int spins = 0;
                        for (;;) {
                            if (pv[j] & BF_VALID) { isP = true; val = pv[j]; break; }
                            if (av[j] & BF_VALID) { val = av[j]; break; }
                            if (++spins > BF_SPIN_LIMIT) { atomicExch(ctrl + 1, 1u); if (status) status[0] = GS_ENOSPC; break; }   // (reported as a truncated view)
                            __builtin_amdgcn_s_sleep(2);
                            pv[j] = __hip_atomic_load(&pre[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            av[j] = __hip_atomic_load(&agg[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                    const u64 pmask = __ballot(isP);
                    const int first = pmask ? __builtin_ctzll(pmask) : 64;
                    if (lane <= first) acc += val & ~BF_VALID;
                    if (pmask) done = true;
                }
                pos -= 64 * EM_LOOK;
            }
        }
        const unsigned long long base = gs_wave_sum_u64(acc);
        if (lane == 0) {
            __hip_atomic_store(&pre[block], (u64)(base + total) | BF_VALID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_base = base;
        }
    }
    __syncthreads();
    unsigned long long cur = s_base + before + incl - mine;
#pragma unroll
    for (int k = 0; k < EM_PER; ++k) {
        if (v[k] < 0 || c[k] == 0u) continue;
        const int x0 = (int)(q[k].x & 0xffffu), y0 = (int)(q[k].x >> 16), x1 = (int)(q[k].y & 0xffffu), y1 = (int)(q[k].y >> 16);
        for (int i = y0; i < y1; ++i)
            for (int j = x0; j < x1; ++j) {
                const unsigned t = (unsigned)(i * tile_w + j);
                if (cur < (unsigned long long)item_cap) items[cur] = make_uint2(t, (unsigned)v[k]);   // (capacity protocol: an overflowing view is reported, not written)
                ++cur;
            }
    }
}

// ---- tile-first binning (the engine's path up to BF_HIST_MAX tiles) ----------------------------------------------------------------
// Two classes of the segment sort, one launch each.  Small: a segment of up to SEG_CAP0 items is sorted in the LDS of one 128-thread
// workgroup (seven in ten of the bench scene's segments, in 16.9 KB, under the 22.5 KB RS_ITEMS was tuned to).  Large: every longer
// segment goes to one 512-thread workgroup with the LDS of one chunk of SEG_CHUNK items (66 KB: two of them, or one beside two
// compositor workgroups, share a CU -- no workgroup needs an empty CU); up to SEG_CHUNK items it is sorted there as in the small
// class, a longer one by the hybrid schedule of gs_segsort_dev.h -- the same network, its wide stages in place on the segment's range
// of the item buffer, the rest chunk by chunk in LDS.  The capacities are powers of two: the LDS then holds a whole padded network
// and no index of it is ever checked.  A thread holds 2^SEG_GMAX items.
#define SEG_CLASSES 2
#define SEG_CAP0 2048
#define SEG_LG_CHUNK 13                      // (the large class: 512 threads x 8 192 items; 256 x 4 096 measured: DESIGN.md section 6)
#define SEG_CHUNK (1 << SEG_LG_CHUNK)
#define SEG_GMAX 4                           // (8 items per thread: +7 % on the three sort launches, 32: +25 %, 164 VGPRs)
#define SEG_THREADS(cap) ((cap) >> SEG_GMAX)
#define SEG_BINS 64                          // half-octave length bins per class (lengths < 2^31: 62 used)
static size_t seg_lds_bytes(int cap) { return (size_t)(cap + (cap >> 5) + 1) * sizeof(u64); }

extern "C" int gs_isect_bin_front_classes(int* caps, int max)
{
    const int c[2] = { SEG_CAP0, SEG_CHUNK };                   // the lengths at which the path changes
    for (int i = 0; i < 2 && i < max; ++i) if (caps) caps[i] = c[i];
    return 2;
}

// Work lists of the segment sort, filled by the offsets scan: lists[c * n_tiles ..] = the non-empty tiles of class c, longest first to
// the half octave (struct BwdOrder of gs_raster.hip files the backward's tiles the same way), count[c] = how many.  The scan also does
// what bin_setup_kernel does for the radix path: it clears the scatter's per-tile cursors and checks the view against its capacity.
struct SegLists {
    unsigned* count; int32_t* lists;
    unsigned* cursor;                        // [n_tiles], cleared
    const long long* counts; long long v_cap, i_cap; long long* status;          // capacity protocol, as bin_setup_kernel
};

__device__ __forceinline__ int seg_class(unsigned len) { return len <= SEG_CAP0 ? 0 : 1; }
__device__ __forceinline__ int seg_bin(unsigned len)                 // len >= 1: 2 * floor(log2) + the next bit, reversed (longest first)
{
    const int l2 = 31 - __clz((int)len);
    const int half = l2 > 0 ? (int)((len >> (l2 - 1)) & 1u) : 0;
    return SEG_BINS - 1 - (2 * l2 + half);
}

// offsets[t] = min(exclusive prefix of the tile counts, n) by one workgroup: the tile offsets of a view.  (The clamp only ever acts
// on a view that overflowed its capacity: its list is truncated, the offsets then are not those of the truncated
// list -- memory-safe, wrong image, reported, as the capacity protocol says.)  With `sl` the same workgroup files every non-empty tile
// by the length of its (clamped) segment: the lengths of a class sum to <= n, which bounds the grid of that class on the host.  It
// walks every tile anyway, so it also clears the scatter's cursors, and its first thread does the capacity check.
__global__ void __launch_bounds__(1024)
tile_offsets_scan_kernel(int n_tiles, const unsigned* __restrict__ tile_counts, GsCount nc, int32_t* __restrict__ offsets, SegLists sl)
{
    __shared__ unsigned wsum[16];
    __shared__ unsigned s_bin[SEG_CLASSES * SEG_BINS];
    const unsigned n = (unsigned)gs_count(nc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (sl.count && threadIdx.x < SEG_CLASSES * SEG_BINS) s_bin[threadIdx.x] = 0u;
    if (sl.count && threadIdx.x == 0 && sl.counts != nullptr && sl.status != nullptr) {     // capacity protocol, as capacity_check_kernel
        const long long V = sl.counts[0], I = sl.counts[1];
        if (V > sl.v_cap || I > sl.i_cap) {
            sl.status[0] = GS_ENOSPC;
            if (I > sl.status[1]) sl.status[1] = I;
            if (V > sl.status[2]) sl.status[2] = V;
        }
    }
    __syncthreads();
    unsigned carry = 0u;
    for (int i0 = 0; i0 < n_tiles; i0 += 1024) {
        const int i = i0 + threadIdx.x;
        const unsigned v = i < n_tiles ? tile_counts[i] : 0u;
        unsigned incl = v;
        incl = gs_wave_incl_scan(incl);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned before = 0u, all = 0u;
        for (int w = 0; w < 16; ++w) { if (w < wave) before += wsum[w]; all += wsum[w]; }
        if (i < n_tiles) {
            const unsigned o = carry + before + incl - v;
            const unsigned beg = o < n ? o : n, end = o + v < n ? o + v : n;
            offsets[i] = (int32_t)beg;
            if (sl.count) sl.cursor[i] = 0u;
            if (sl.count && end > beg) atomicAdd(&s_bin[seg_class(end - beg) * SEG_BINS + seg_bin(end - beg)], 1u);
        }
        carry += all;
        __syncthreads();
    }
    if (!sl.count) return;
    // wave c scans the bins of class c (64 bins = one wave): start of every bin inside the class list, and the class total
    if (wave < SEG_CLASSES) {
        const unsigned v = s_bin[wave * SEG_BINS + lane];
        const unsigned incl = gs_wave_incl_scan(v);
        s_bin[wave * SEG_BINS + lane] = incl - v;
        if (lane == 63) sl.count[wave] = incl;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_tiles; i += 1024) {                      // (offsets[] of this workgroup's own stores: same thread, same index)
        const unsigned beg = (unsigned)offsets[i];
        unsigned end = n;
        if (i + 1 < n_tiles) end = (unsigned)__hip_atomic_load(&offsets[i + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (end > beg) {
            const int c = seg_class(end - beg);
            const unsigned pos = atomicAdd(&s_bin[c * SEG_BINS + seg_bin(end - beg)], 1u);
            sl.lists[(size_t)c * n_tiles + pos] = i;
        }
    }
}

#define SC_THREADS 512
#define SC_PER 8                             // packed slots per thread
#define SC_TILE (SC_THREADS * SC_PER)

// Scatter in slot order: a block owns SC_TILE consecutive packed slots, reads their keys and rectangles coalesced, counts its items per
// tile in LDS, reserves a range on every touched tile's cursor with ONE returning atomic, and ranks its items inside the range with LDS
// atomics -- the same LDS word first counts, then holds the next free position of the tile.  An item is the 64-bit composite the segment
// sort orders by: key << 31 | slot (slot < 2^31), with bit 62 set for 24-bit keys (item_bias: every item is then the bit pattern of a
// normal positive double, see gs_seg_cx).  The order inside a segment is arbitrary.  Nobody waits for anybody.
// The kernel's time follows the number of (block, touched tile) reservations, not the bytes: alone on the bench view 256 x 4 slots take
// 89 us, 256 x 8 81, 256 x 16 60, 512 x 8 50, 1024 x 8 46 (there too: scanning only the touched range of tile ids,
// and handing neighbouring chunks to one XCD, which both cost more than they saved).
__global__ void __launch_bounds__(SC_THREADS)
bin_scatter_kernel(GsCount vc, const unsigned* __restrict__ keys, const uint2* __restrict__ rects, unsigned key_mask, u64 item_bias, int tile_w, int tile_h,
                   const int32_t* __restrict__ offsets, unsigned* __restrict__ cursor, u64* __restrict__ items, unsigned item_cap)
{
    extern __shared__ unsigned s_pos[];                          // [n_tiles]
    const int V = (int)gs_count(vc);
    const int n_tiles = tile_w * tile_h;
    const int s0 = (int)blockIdx.x * SC_TILE + (int)threadIdx.x;
    if ((long long)blockIdx.x * SC_TILE >= V) return;
    for (int t = threadIdx.x; t < n_tiles; t += SC_THREADS) s_pos[t] = 0u;
    unsigned key[SC_PER]; uint2 q[SC_PER];
#pragma unroll
    for (int k = 0; k < SC_PER; ++k) {
        const int v = s0 + k * SC_THREADS;
        const int vv = v < V ? v : V - 1;                        // (a load under a branch would drain the loads in flight)
        key[k] = keys[vv];
        q[k] = rects[vv];
        if (v >= V) q[k] = make_uint2(0u, 0u);
    }
#pragma unroll
    for (int k = 0; k < SC_PER; ++k) {                           // rectangles clipped to the grid once: nothing below indexes outside s_pos
        int x1 = (int)(q[k].y & 0xffffu), y1 = (int)(q[k].y >> 16);
        x1 = x1 < tile_w ? x1 : tile_w; y1 = y1 < tile_h ? y1 : tile_h;
        q[k].y = (unsigned)x1 | ((unsigned)y1 << 16);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SC_PER; ++k) {
        const int x0 = (int)(q[k].x & 0xffffu), y0 = (int)(q[k].x >> 16), x1 = (int)(q[k].y & 0xffffu), y1 = (int)(q[k].y >> 16);
        for (int i = y0; i < y1; ++i)
            for (int j = x0; j < x1; ++j) atomicAdd(&s_pos[i * tile_w + j], 1u);
    }
    __syncthreads();
    for (int t0 = threadIdx.x; t0 < n_tiles; t0 += 4 * SC_THREADS) {       // four reservations in flight per thread
        unsigned c[4], o[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + u * SC_THREADS;
            c[u] = t < n_tiles ? s_pos[t] : 0u;
            o[u] = c[u] ? (unsigned)offsets[t] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = c[u] ? atomicAdd(&cursor[t0 + u * SC_THREADS], c[u]) : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) if (c[u]) s_pos[t0 + u * SC_THREADS] = o[u] + b[u];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SC_PER; ++k) {
        const int x0 = (int)(q[k].x & 0xffffu), y0 = (int)(q[k].x >> 16), x1 = (int)(q[k].y & 0xffffu), y1 = (int)(q[k].y >> 16);
        const u64 item = item_bias | ((u64)(key[k] & key_mask) << 31) | (u64)(unsigned)(s0 + k * SC_THREADS);
        for (int i = y0; i < y1; ++i)
            for (int j = x0; j < x1; ++j) {
                const unsigned pos = atomicAdd(&s_pos[i * tile_w + j], 1u);
                if (pos < item_cap) items[pos] = item;           // (capacity protocol: an overflowing view is reported, not written)
            }
    }
}

// Segment sort: workgroup b of a class sorts the segment of tile lists[b] by its items (key, then slot) -- the order of the stable radix sort,
// ties included, whatever order the scatter left -- and writes the slots.  The small class loads the segment once, pads it to its power
// of two and sorts it in LDS; the large class does the same up to one chunk and runs the hybrid schedule on a longer segment (its wide
// stages in place on the segment's own range of the item buffer: one CU, its stores and loads meet in that CU's cache, a workgroup
// barrier orders them).  A slot is clamped to the view's count: after an overflow the tail of the item buffer was never written, and
// the ids must stay valid rows for whoever gathers by them.
template <int THREADS, bool F64>
__global__ void __launch_bounds__(THREADS)
seg_sort_kernel(const int32_t* __restrict__ list, const unsigned* __restrict__ list_count, int n_tiles, const int32_t* __restrict__ offsets,
                GsCount ic, GsCount vc, u64* items, int32_t* __restrict__ flat)
{
    extern __shared__ u64 s_seg[];
    if (blockIdx.x >= *list_count) return;
    const int t = list[blockIdx.x];
    const int n_all = (int)gs_count(ic);
    const int beg = offsets[t], end = t + 1 < n_tiles ? offsets[t + 1] : n_all;
    const int n = end - beg;
    if (n <= 0) return;
    const long long V = gs_count(vc);
    const unsigned vmax = V > 0 ? (unsigned)(V - 1) : 0u;
    const int tid = threadIdx.x;
    int P = 1 << SEG_GMAX;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += THREADS) s_seg[gs_seg_phys<true>(i)] = i < n ? items[beg + i] : gs_seg_inf<F64>();
    __syncthreads();
    GS_SEG_SORT_BODY(SEG_GMAX, true, F64, false, s_seg, n, P, tid, THREADS, __syncthreads());
    for (int i = tid; i < n; i += THREADS) {
        const unsigned slot = (unsigned)s_seg[gs_seg_phys<true>(i)] & 0x7fffffffu;
        flat[beg + i] = (int32_t)(slot < vmax ? slot : vmax);
    }
}

template <int THREADS, int LG_CHUNK, bool F64>
__global__ void __launch_bounds__(THREADS)
seg_sort_large_kernel(const int32_t* __restrict__ list, const unsigned* __restrict__ list_count, int n_tiles, const int32_t* __restrict__ offsets,
                      GsCount ic, GsCount vc, u64* items, int32_t* __restrict__ flat)
{
    __shared__ u64 s_seg[(1 << LG_CHUNK) + (1 << (LG_CHUNK - 5)) + 1];          // (static: 66 KB need no per-launch opt-in on the host)
    if (blockIdx.x >= *list_count) return;
    const int t = list[blockIdx.x];
    const int n_all = (int)gs_count(ic);
    const int beg = offsets[t], end = t + 1 < n_tiles ? offsets[t + 1] : n_all;
    const int n = end - beg;                                     // (uniform across the workgroup: so is every barrier of the schedule)
    if (n <= 0) return;
    const long long V = gs_count(vc);
    const unsigned vmax = V > 0 ? (unsigned)(V - 1) : 0u;
    gs_seg_hybrid<SEG_GMAX, LG_CHUNK, THREADS, F64>(s_seg, items + beg, n, (int)threadIdx.x, [] { __syncthreads(); },
        [=](int i, u64 w) {
            const unsigned slot = (unsigned)w & 0x7fffffffu;
            flat[beg + i] = (int32_t)(slot < vmax ? slot : vmax);
        });
}

// offsets[t] = first sorted position whose tile id >= t (the > 8 192-tile path; same as isect_offsets_tiles_kernel of gs_project.hip)
__global__ void __launch_bounds__(256)
bin_offsets_tiles_kernel(GsCount nc, const int32_t* __restrict__ tiles, int n_tiles, int32_t* __restrict__ offsets)
{
    const int64_t n = gs_count(nc);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n == 0 && i == 0)
        for (int t = 0; t < n_tiles; ++t) offsets[t] = 0;
    if (i >= n) return;
    const int cur = tiles[i];
    if (i == 0) {
        for (int t = 0; t <= cur && t < n_tiles; ++t) offsets[t] = 0;
    } else {
        const int prev = tiles[i - 1];
        for (int t = prev + 1; t <= cur && t < n_tiles; ++t) offsets[t] = (int32_t)i;
    }
    if (i == n - 1)
        for (int t = cur + 1; t < n_tiles; ++t) offsets[t] = (int32_t)n;
}


// ---- the three steps of the radix machinery, as gs_isect_bin and the radix path of gs_isect_bin_front run them ---------------------
// 1. depth order of the Gaussians: npass stable 8-bit passes over (key, index) items, da -> db -> da ...; the first reads `first`
template <typename In>
static int depth_order(GsCount vc, In first, int npass, const RadixWs& w, hipStream_t s, const uint2** order)
{
    uint2* src = w.da; uint2* dst = w.db;
    int rc = radix_pass<uint2>(vc, first, XDigit{ 0, 255u }, U2Out{ src }, 8, w.table, s);
    for (int pass = 1; pass < npass && rc == GS_OK; ++pass) {
        rc = radix_pass<uint2>(vc, U2In{ src }, XDigit{ 8 * pass, 255u }, U2Out{ dst }, 8, w.table, s);
        uint2* t = src; src = dst; dst = t;
    }
    *order = src;
    return rc;
}

// 2. emission in depth order: the look-back state is cleared (the same launch checks the view against its capacity where `cap` names
//    the counts), then the positions come from a chained scan inside the launch
struct CapCheck { const long long* counts; long long v_cap, i_cap; long long* status; };
static int emit_in_depth_order(const RadixWs& w, GsCount vc, const uint2* order, const uint2* rect, int tile_w, int64_t n_isects,
                               const CapCheck& cap, hipStream_t s)
{
    const int eblocks = ((int)vc.n + EM_TILE - 1) / EM_TILE;
    hipLaunchKernelGGL(bin_setup_kernel, dim3(gs_cdiv(w.n_state_words, 256) < 64 ? gs_cdiv(w.n_state_words, 256) : 64), dim3(256), 0, s,
                       w.state, w.n_state_words, cap.counts, cap.v_cap, cap.i_cap, cap.status);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(emit_chained_kernel, dim3(eblocks), dim3(EM_THREADS), 0, s, vc, order, rect, w.state, (u64*)(w.state + 4),
                       eblocks + 1, tile_w, w.ia, (unsigned)n_isects, cap.status);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// 3. stable split by tile id: npass digits of `width` bits over the emitted (tile, index) items, ia -> ib -> ia ...; the last pass
//    writes through `final`
template <typename Final>
static int split_by_tile(GsCount ic, int n_tiles, const RadixWs& w, Final final, hipStream_t s)
{
    int tb = 0;
    while ((1 << tb) < n_tiles) ++tb;
    if (tb < 1) tb = 1;
    const int npass = (tb + 7) / 8, width = (tb + npass - 1) / npass;
    uint2* src = w.ia; uint2* dst = w.ib;
    for (int pass = 0; pass < npass; ++pass) {
        const int shift = pass * width;
        const int nbits = (tb - shift) < width ? (tb - shift) : width;
        const XDigit digit{ shift, (1u << nbits) - 1u };
        const int rc = pass == npass - 1 ? radix_pass<uint2>(ic, U2In{ src }, digit, final, nbits, w.table, s)
                                         : radix_pass<uint2>(ic, U2In{ src }, digit, U2Out{ dst }, nbits, w.table, s);
        if (rc != GS_OK) return rc;
        uint2* t = src; src = dst; dst = t;
    }
    return GS_OK;
}

// scratch of the two paths.  Tile first: the per-tile cursors + the class counters, the class lists, the items.
static size_t tf_state_words(int n_tiles) { return (size_t)n_tiles + SEG_CLASSES; }
static size_t tf_ws_bytes(int64_t n_isects, int n_tiles)
{
    return align256(tf_state_words(n_tiles) * 4) + align256((size_t)SEG_CLASSES * n_tiles * 4) + align256((size_t)n_isects * 8) + 256;
}

// What gs_isect_bin_front needs for these sizes when it is given tile_counts (it always needs that much; a caller that passes no
// tile_counts for a grid of <= BF_HIST_MAX tiles takes the radix path and is told if its scratch is too small for it).
extern "C" size_t gs_isect_bin_front_ws_bytes(int V, int64_t n_isects, int tile_w, int tile_h)
{
    const size_t v = V > 0 ? (size_t)V : 1, n = n_isects > 0 ? (size_t)n_isects : 1;
    const int64_t n_tiles = (int64_t)tile_w * tile_h;
    if (n_tiles > 0 && n_tiles <= BF_HIST_MAX) return tf_ws_bytes((int64_t)n, (int)n_tiles);
    return radix_ws(nullptr, v, n, false, true).bytes;
}

static int bin_front_tile_first(int V, const uint32_t* depth_keys, const uint32_t* tile_rects, const uint32_t* tile_counts,
                                const int64_t* counts_dev, int64_t n_isects, int key_bits, int tile_w, int tile_h, int32_t* flatten_ids_sorted,
                                int32_t* isect_offsets, void* ws, int64_t* status_dev, hipStream_t s)
{
    const int n_tiles = tile_w * tile_h;
    const GsCount vc{ (long long)V, (const long long*)counts_dev }, ic{ (long long)n_isects, counts_dev ? (const long long*)counts_dev + 1 : nullptr };
    char* p = (char*)ws;
    unsigned* cursor = (unsigned*)p;                                        // [n_tiles], then the class counters
    unsigned* class_count = cursor + n_tiles; p += align256(tf_state_words(n_tiles) * 4);
    int32_t* lists = (int32_t*)p; p += align256((size_t)SEG_CLASSES * n_tiles * 4);
    u64* items = (u64*)p;
    hipLaunchKernelGGL(tile_offsets_scan_kernel, dim3(1), dim3(1024), 0, s, n_tiles, (const unsigned*)tile_counts, ic, isect_offsets,
                       SegLists{ class_count, lists, cursor, (const long long*)counts_dev, (long long)V, (long long)n_isects, (long long*)status_dev });
    GS_CHECK_LAUNCH();
    const bool f64 = key_bits == 24;                                       // 24 + 31 bits under the bias bit: the double-precision compare-exchange
    hipLaunchKernelGGL(bin_scatter_kernel, dim3(gs_cdiv(V, SC_TILE)), dim3(SC_THREADS), (size_t)n_tiles * 4, s, vc,
                       (const unsigned*)depth_keys, (const uint2*)tile_rects, f64 ? 0xffffffu : 0xffffffffu, f64 ? (1ull << 62) : 0ull, tile_w, tile_h,
                       (const int32_t*)isect_offsets, cursor, items, (unsigned)n_isects);
    GS_CHECK_LAUNCH();
    // a class holds segments longer than the class below takes, and the (clamped) segments sum to <= n_isects: that bounds its grid
    const int caps[SEG_CLASSES] = { 0, SEG_CAP0 };
    for (int c = 0; c < SEG_CLASSES; ++c) {
        const int64_t most = n_isects / (caps[c] + 1);
        const int grid = (int)(most < n_tiles ? most : n_tiles);
        if (grid == 0) continue;
        const int32_t* list = lists + (size_t)c * n_tiles;
#define SEG_LAUNCH(KERNEL, T, LDS) hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(T), LDS, s, list, (const unsigned*)(class_count + c), n_tiles, \
                                                      (const int32_t*)isect_offsets, ic, vc, items, flatten_ids_sorted)
        if (c == 0) {
            if (f64) SEG_LAUNCH((seg_sort_kernel<SEG_THREADS(SEG_CAP0), true>), SEG_THREADS(SEG_CAP0), seg_lds_bytes(SEG_CAP0));
            else SEG_LAUNCH((seg_sort_kernel<SEG_THREADS(SEG_CAP0), false>), SEG_THREADS(SEG_CAP0), seg_lds_bytes(SEG_CAP0));
        } else {
            if (f64) SEG_LAUNCH((seg_sort_large_kernel<SEG_THREADS(SEG_CHUNK), SEG_LG_CHUNK, true>), SEG_THREADS(SEG_CHUNK), 0);
            else SEG_LAUNCH((seg_sort_large_kernel<SEG_THREADS(SEG_CHUNK), SEG_LG_CHUNK, false>), SEG_THREADS(SEG_CHUNK), 0);
        }
#undef SEG_LAUNCH
        GS_CHECK_LAUNCH();
    }
    return GS_OK;
}

extern "C" int gs_isect_bin_front(int V_cap, const uint32_t* depth_keys, const uint32_t* tile_rects, const uint32_t* tile_counts,
                                  const int64_t* counts_dev, int64_t n_isects_cap, int key_bits, int tile_w, int tile_h, int32_t* flatten_ids_sorted,
                                  int32_t* isect_offsets, void* ws, size_t ws_bytes, int64_t* status_dev, void* stream)
{
    const int V = V_cap;
    const int64_t n_isects = n_isects_cap;
    GS_CHECK_ARG(V >= 0 && n_isects >= 0 && tile_w > 0 && tile_h > 0 && (key_bits == 24 || key_bits == 32), "bad sizes or key width");
    GS_CHECK_ARG(n_isects < (1ll << 31), "n_isects must fit int32");
    GS_CHECK_ARG((int64_t)tile_w * tile_h < (1ll << 24) && tile_w < 65536 && tile_h < 65536, "tile grid too large");
    GS_CHECK_ARG(isect_offsets != nullptr && (counts_dev == nullptr || status_dev != nullptr), "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int n_tiles = tile_w * tile_h;
    if (V == 0 || n_isects == 0) { GS_CHECK_HIP(gs_zero_async(isect_offsets, sizeof(int32_t) * (size_t)n_tiles, s)); return GS_OK; }
    GS_CHECK_ARG(depth_keys != nullptr && tile_rects != nullptr && flatten_ids_sorted != nullptr && ws != nullptr, "null argument");
    if (tile_counts != nullptr && n_tiles <= BF_HIST_MAX) {
        if (ws_bytes < tf_ws_bytes(n_isects, n_tiles)) { gs_set_error("gs_isect_bin_front: workspace too small"); return GS_ENOSPC; }
        return bin_front_tile_first(V, depth_keys, tile_rects, tile_counts, counts_dev, n_isects, key_bits, tile_w, tile_h, flatten_ids_sorted,
                                    isect_offsets, ws, status_dev, s);
    }
    // radix path: the offsets come from the sorted tile ids
    const RadixWs w = radix_ws(ws, (size_t)V, (size_t)n_isects, false, true);
    if (ws_bytes < w.bytes) { gs_set_error("gs_isect_bin_front: workspace too small for the radix path (no tile_counts)"); return GS_ENOSPC; }
    const GsCount vc{ (long long)V, (const long long*)counts_dev }, ic{ (long long)n_isects, counts_dev ? (const long long*)counts_dev + 1 : nullptr };
    const uint2* order;
    int rc = depth_order(vc, KeyIn{ depth_keys }, key_bits / 8, w, s, &order);
    if (rc != GS_OK) return rc;
    rc = emit_in_depth_order(w, vc, order, (const uint2*)tile_rects, tile_w, n_isects,
                             CapCheck{ (const long long*)counts_dev, (long long)V_cap, (long long)n_isects_cap, (long long*)status_dev }, s);
    if (rc != GS_OK) return rc;
    rc = split_by_tile(ic, n_tiles, w, FinalTiles{ w.tile_ids, flatten_ids_sorted }, s);
    if (rc != GS_OK) return rc;
    hipLaunchKernelGGL(bin_offsets_tiles_kernel, dim3(gs_cdiv(n_isects, 256)), dim3(256), 0, s, ic, w.tile_ids, n_tiles, isect_offsets);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// ---- gs_isect_bin / _cap / _tiles_cap: the rasterization() call shape (emitted keys are never materialised) -----------------------
static int isect_bin_impl(int V, const float* means2d, const int32_t* radii, const float* depths, int64_t n_isects,
                          const long long* counts_dev, int tile_size, int tile_w, int tile_h, int64_t* isect_ids_sorted,
                          int32_t* flatten_ids_sorted, void* ws, size_t ws_bytes, void* stream, int32_t* tile_ids_sorted)
{
    const GsCount vc{ (long long)V, counts_dev }, ic{ (long long)n_isects, counts_dev ? counts_dev + 1 : nullptr };
    GS_CHECK_ARG(V >= 0 && n_isects >= 0 && tile_size > 0 && tile_w > 0 && tile_h > 0, "bad sizes");
    GS_CHECK_ARG(n_isects < (1ll << 31), "n_isects must fit int32");
    GS_CHECK_ARG((int64_t)tile_w * tile_h < (1ll << 24), "more than 2^24 tiles");
    if (V == 0 || n_isects == 0) return GS_OK;
    GS_CHECK_ARG(ws != nullptr, "workspace must not be NULL");
    const RadixWs w = radix_ws(ws, (size_t)V, (size_t)n_isects, true, false);
    if (ws_bytes < w.bytes) { gs_set_error("gs_isect_bin: workspace too small"); return GS_ENOSPC; }
    hipStream_t s = (hipStream_t)stream;
    const uint2* order;
    int rc = depth_order(vc, DepthIn{ depths }, 4, w, s, &order);
    if (rc != GS_OK) return rc;
    GS_CHECK_ARG(tile_w < 65536 && tile_h < 65536, "tile grid too large");
    hipLaunchKernelGGL(tile_rect_kernel, dim3(gs_cdiv(V, 256)), dim3(256), 0, s, vc, means2d, radii, tile_size, tile_w, tile_h, w.rect);
    GS_CHECK_LAUNCH();
    rc = emit_in_depth_order(w, vc, order, w.rect, tile_w, n_isects, CapCheck{ nullptr, 0ll, 0ll, nullptr }, s);
    if (rc != GS_OK) return rc;
    // the last tile pass writes the sorted meta arrays
    if (tile_ids_sorted != nullptr) return split_by_tile(ic, tile_w * tile_h, w, FinalTiles{ tile_ids_sorted, flatten_ids_sorted }, s);
    return split_by_tile(ic, tile_w * tile_h, w, FinalOut{ (u64*)isect_ids_sorted, flatten_ids_sorted, depths }, s);
}

extern "C" int gs_isect_bin(int V, const float* means2d, const int32_t* radii, const float* depths,
                            const int32_t* tiles_per_gauss, int64_t n_isects, int tile_size, int tile_w, int tile_h,
                            int64_t* isect_ids_sorted, int32_t* flatten_ids_sorted, void* ws, size_t ws_bytes, void* stream)
{
    (void)tiles_per_gauss;                                  // the counts are re-derived from the rectangles (same arithmetic as gs_project_fwd)
    return isect_bin_impl(V, means2d, radii, depths, n_isects, nullptr, tile_size, tile_w, tile_h, isect_ids_sorted, flatten_ids_sorted,
                          ws, ws_bytes, stream, nullptr);
}

extern "C" int gs_isect_bin_cap(int V_cap, const float* means2d, const int32_t* radii, const float* depths, const int64_t* counts_dev,
                                int64_t n_isects_cap, int tile_size, int tile_w, int tile_h, int64_t* isect_ids_sorted,
                                int32_t* flatten_ids_sorted, void* ws, size_t ws_bytes, int64_t* status_dev, void* stream)
{
    GS_CHECK_ARG(counts_dev != nullptr && status_dev != nullptr, "counts_dev / status_dev must not be NULL");
    hipLaunchKernelGGL(capacity_check_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const long long*)counts_dev, (long long)V_cap,
                       (long long)n_isects_cap, (long long*)status_dev);
    GS_CHECK_LAUNCH();
    return isect_bin_impl(V_cap, means2d, radii, depths, n_isects_cap, (const long long*)counts_dev, tile_size, tile_w, tile_h,
                          isect_ids_sorted, flatten_ids_sorted, ws, ws_bytes, stream, nullptr);
}

// The same without the 64-bit `isect_ids`: a caller that only composites (the step engine: `meta` is never returned) needs the sorted
// flatten ids and the tile offsets; the last pass then writes 8 bytes per intersection instead of 12 and does not gather the depths
// (gs_isect_offsets_tiles_cap takes the int32 tile ids).
extern "C" int gs_isect_bin_tiles_cap(int V_cap, const float* means2d, const int32_t* radii, const float* depths, const int64_t* counts_dev,
                                      int64_t n_isects_cap, int tile_size, int tile_w, int tile_h, int32_t* tile_ids_sorted,
                                      int32_t* flatten_ids_sorted, void* ws, size_t ws_bytes, int64_t* status_dev, void* stream)
{
    GS_CHECK_ARG(counts_dev != nullptr && status_dev != nullptr && tile_ids_sorted != nullptr, "counts_dev / status_dev / tile_ids_sorted must not be NULL");
    hipLaunchKernelGGL(capacity_check_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const long long*)counts_dev, (long long)V_cap,
                       (long long)n_isects_cap, (long long*)status_dev);
    GS_CHECK_LAUNCH();
    return isect_bin_impl(V_cap, means2d, radii, depths, n_isects_cap, (const long long*)counts_dev, tile_size, tile_w, tile_h,
                          nullptr, flatten_ids_sorted, ws, ws_bytes, stream, tile_ids_sorted);
}
