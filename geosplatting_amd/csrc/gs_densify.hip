// gs_densify.hip -- adaptive density control of the vanilla-3DGS trainer (rfstudio/graphics/_splats.py:82-184,
// rfstudio/model/gsplat.py:360-374, rfstudio/optim/optimizer.py:155-185) as three entry points:
//   gs_densify_stats : the per-view densification statistics (xys_grad_norm, vis_counts)
//   gs_densify_plan  : classify every Gaussian (keep / split / duplicate / cull), rank the classes, totals on the device
//   gs_densify_fill  : the row map, `indices`, and ONE gather launch over every parameter and Adam moment tensor
// The refinement is a memory move: 59 parameter floats + 118 moment floats per Gaussian.  Classification and ranks read 7 floats
// per Gaussian; the gather touches every attribute byte once on each side.  No LDS staging, no atomics, vector stores only.
#include "gs_common.h"
#include "gs_ws.h"

#define DN_BLOCK 256
#define DN_SCAN_THREADS 1024

#define DN_SELECTED 1u
#define DN_SPLIT 2u
#define DN_DUP 4u


// workspace: [ block counts / offsets u32[3 * nb] | class flags u8[N] | row map i32[N * max(S, 2)] ]
struct DnLayout { unsigned* blocks; unsigned char* flags; int* rowmap; size_t total; int nb; };
static inline DnLayout dn_layout(void* base, int64_t N, int num_splits)
{
    GsWs w(base, 256);
    DnLayout L;
    L.nb = gs_cdiv(N, DN_BLOCK);
    const int64_t per = num_splits > 2 ? num_splits : 2;           // a split row yields S rows, any other at most 2 (kept + copy)
    L.blocks = w.take<unsigned>((size_t)3 * (size_t)L.nb);
    L.flags = w.take<unsigned char>((size_t)N);
    L.rowmap = w.take<int>((size_t)N * (size_t)per);
    L.total = w.bytes();
    return L;
}

// ------------------------------------------------------------------------------------------------ statistics
static __global__ void __launch_bounds__(DN_BLOCK) densify_stats_kernel(int V, const long long* __restrict__ ids,
                                                                        const float2* __restrict__ v_means2d, long long N,
                                                                        float* __restrict__ xys_grad_norm, float* __restrict__ vis_counts)
{
    const int v = blockIdx.x * DN_BLOCK + threadIdx.x;
    if (v >= V) return;
    const long long id = ids[v];
    if (id < 0 || id >= N) return;
    const float2 g = v_means2d[v];
    // ids are unique within a call (packed, one camera): plain read-modify-write
    xys_grad_norm[id] += sqrtf(g.x * g.x + g.y * g.y);
    vis_counts[id] += 1.0f;
}

// ------------------------------------------------------------------------------------------------ classification
struct DnThresholds {
    float half_extent, grad_thresh, size_thresh, alpha_thresh, scale_thresh;
    int mode;
};

__device__ __forceinline__ unsigned dn_classify(long long i, const float* __restrict__ scales, const float* __restrict__ opacities,
                                                const float* __restrict__ xys_grad_norm, const float* __restrict__ vis_counts,
                                                const DnThresholds& t)
{
#pragma clang fp contract(off)
    const float s0 = expf(scales[3 * i + 0]), s1 = expf(scales[3 * i + 1]), s2 = expf(scales[3 * i + 2]);
    const float scale_max = fmaxf(s0, fmaxf(s1, s2));
    const float alpha = 1.0f / (1.0f + expf(-opacities[i]));
    bool cull = alpha < t.alpha_thresh;
    if (t.scale_thresh >= 0.0f) cull = cull || (scale_max > t.scale_thresh);
    bool split = false, dup = false;
    if (t.mode == 0) {
        const float avg = t.half_extent * (xys_grad_norm[i] / vis_counts[i]);     // the reference's order: the divide first
        const bool high = avg > t.grad_thresh;
        split = high && (scale_max > t.size_thresh);
        dup = high && (scale_max <= t.size_thresh);
    }
    const bool selected = !(cull || split);
    return (selected ? DN_SELECTED : 0u) | (split ? DN_SPLIT : 0u) | (dup ? DN_DUP : 0u);
}

// counts of one class over the 256 rows of a block; every thread of the block calls it
__device__ __forceinline__ unsigned dn_block_count(bool p, unsigned* lds)
{
    const unsigned long long b = __ballot(p);
    if (gs_lane_id() == 0) lds[threadIdx.x >> 6] = (unsigned)__popcll(b);
    __syncthreads();
    const unsigned total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return total;
}

static __global__ void __launch_bounds__(DN_BLOCK) densify_classify_kernel(long long N, const float* __restrict__ scales,
                                                                           const float* __restrict__ opacities,
                                                                           const float* __restrict__ xys_grad_norm,
                                                                           const float* __restrict__ vis_counts, DnThresholds t,
                                                                           unsigned char* __restrict__ flags, unsigned* __restrict__ blocks,
                                                                           int nb)
{
    __shared__ unsigned lds[4];
    const long long i = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    unsigned f = 0u;
    if (i < N) {
        f = dn_classify(i, scales, opacities, xys_grad_norm, vis_counts, t);
        flags[i] = (unsigned char)f;
    }
    const unsigned c_sel = dn_block_count((f & DN_SELECTED) != 0u, lds);
    const unsigned c_split = dn_block_count((f & DN_SPLIT) != 0u, lds);
    const unsigned c_dup = dn_block_count((f & DN_DUP) != 0u, lds);
    if (threadIdx.x == 0) {
        blocks[blockIdx.x] = c_sel;
        blocks[nb + blockIdx.x] = c_split;
        blocks[2 * nb + blockIdx.x] = c_dup;
    }
}

// One workgroup turns the three runs of block counts into exclusive offsets (in place) and writes the totals.
static __global__ void __launch_bounds__(DN_SCAN_THREADS) densify_scan_kernel(unsigned* __restrict__ blocks, int nb, int num_splits,
                                                                              long long* __restrict__ totals)
{
    __shared__ unsigned sums[DN_SCAN_THREADS];
    __shared__ unsigned run_total[3];
    const int t = threadIdx.x;
    const int chunk = (nb + DN_SCAN_THREADS - 1) / DN_SCAN_THREADS;
    const int lo = t * chunk, hi = min(lo + chunk, nb);
    for (int k = 0; k < 3; ++k) {
        unsigned* run = blocks + (size_t)k * nb;
        unsigned s = 0u;
        for (int j = lo; j < hi; ++j) s += run[j];
        sums[t] = s;
        __syncthreads();
        for (int d = 1; d < DN_SCAN_THREADS; d <<= 1) {                  // inclusive scan of the per-thread sums
            const unsigned add = t >= d ? sums[t - d] : 0u;
            __syncthreads();
            sums[t] += add;
            __syncthreads();
        }
        unsigned base = sums[t] - s;
        for (int j = lo; j < hi; ++j) {
            const unsigned c = run[j];
            run[j] = base;
            base += c;
        }
        if (t == DN_SCAN_THREADS - 1) run_total[k] = sums[t];
        __syncthreads();
    }
    if (t == 0) {
        const long long n_sel = run_total[0], n_split = run_total[1], n_dup = run_total[2];
        totals[0] = n_sel;
        totals[1] = n_split;
        totals[2] = n_dup;
        totals[3] = n_sel + (long long)num_splits * n_split + n_dup;
    }
}

// ------------------------------------------------------------------------------------------------ row map
// exclusive rank of this thread's predicate inside its block
__device__ __forceinline__ unsigned dn_block_rank(bool p, unsigned* lds)
{
    const unsigned long long b = __ballot(p);
    const int lane = gs_lane_id(), w = threadIdx.x >> 6;
    if (lane == 0) lds[w] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned r = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; ++k) r += lds[k];
    __syncthreads();
    return r;
}

static __global__ void __launch_bounds__(DN_BLOCK) densify_map_kernel(long long N, int num_splits, const unsigned char* __restrict__ flags,
                                                                      const unsigned* __restrict__ blocks, int nb, long long n_sel,
                                                                      long long n_split, long long N_out, int* __restrict__ rowmap,
                                                                      long long* __restrict__ indices)
{
    __shared__ unsigned lds[4];
    const long long i = (long long)blockIdx.x * DN_BLOCK + threadIdx.x;
    const unsigned f = i < N ? flags[i] : 0u;
    const long long r_sel = (long long)blocks[blockIdx.x] + dn_block_rank((f & DN_SELECTED) != 0u, lds);
    const long long r_split = (long long)blocks[nb + blockIdx.x] + dn_block_rank((f & DN_SPLIT) != 0u, lds);
    const long long r_dup = (long long)blocks[2 * nb + blockIdx.x] + dn_block_rank((f & DN_DUP) != 0u, lds);
    // every row is bounds-checked against the caller's N_out: totals that do not belong to this plan cannot write outside
    if ((f & DN_SELECTED) && r_sel < n_sel && r_sel < N_out) {
        rowmap[r_sel] = (int)i;
        indices[r_sel] = i;
    }
    if ((f & DN_SPLIT) && r_split < n_split) {
        for (int s = 0; s < num_splits; ++s) {                           // S-major: child s of every split row, then child s + 1
            const long long r = n_sel + (long long)s * n_split + r_split;
            if (r < N_out) {
                rowmap[r] = (int)i;
                indices[r] = -1;
            }
        }
    }
    if (f & DN_DUP) {
        const long long r = n_sel + (long long)num_splits * n_split + r_dup;
        if (r < N_out) {
            rowmap[r] = (int)i;
            indices[r] = -1;
        }
    }
}

// ------------------------------------------------------------------------------------------------ gather
struct DnTable {
    const float* src[GS_DENSIFY_MAX_TENSORS];
    float* dst[GS_DENSIFY_MAX_TENSORS];
    int floats_per_row[GS_DENSIFY_MAX_TENSORS];
    int kind[GS_DENSIFY_MAX_TENSORS];
    int wide_store[GS_DENSIFY_MAX_TENSORS];      // dst is 16-byte aligned
    int wide_load[GS_DENSIFY_MAX_TENSORS];       // src is 16-byte aligned and the row is a whole number of 16-byte pieces
};

struct DnRows {
    long long N;
    unsigned n_sel, n_split, n_children, N_out;  // n_children = S * n_split
    const int* rowmap;
    const float* quats;
    const float* scales;
    const float* randn;
};

// The three components of a child mean:  R(q / |q|) (exp(scales) o z) + mean  (what Splats.split computes, rfstudio/graphics/_splats.py:91-96),
// evaluated in fp64 and rounded once.  In fp32 a diagonal entry 1 - 2 (y^2 + z^2) / q.q that cancels to ~0 keeps an ABSOLUTE error of a
// few eps, which times a large offset exceeds any bound of the form eps * (|mean_i| + sum_j |R_ij| |o_j|) when the rest of the row is
// small (measured: 1.5 to 2.1 times the tests' 16 eps budget at 2 M rows); fp64 is a few hundred operations per CHILD ROW of a pass
// that moves 708 bytes per row.
__device__ __forceinline__ void dn_child_mean(const DnRows& R, unsigned src, unsigned child, const float* __restrict__ means, float (&out)[3])
{
    const double w = R.quats[4ull * src + 0], x = R.quats[4ull * src + 1], y = R.quats[4ull * src + 2], z = R.quats[4ull * src + 3];
    const double h = 2.0 / (w * w + x * x + y * y + z * z);          // I - (2 / q.q) [...] on the raw quaternion = the rotation of q / |q|
    const double o0 = exp((double)R.scales[3ull * src + 0]) * (double)R.randn[3ull * child + 0];
    const double o1 = exp((double)R.scales[3ull * src + 1]) * (double)R.randn[3ull * child + 1];
    const double o2 = exp((double)R.scales[3ull * src + 2]) * (double)R.randn[3ull * child + 2];
    out[0] = (float)((1.0 - h * (y * y + z * z)) * o0 + h * (x * y - w * z) * o1 + h * (x * z + w * y) * o2 + (double)means[3ull * src + 0]);
    out[1] = (float)(h * (x * y + w * z) * o0 + (1.0 - h * (x * x + z * z)) * o1 + h * (y * z - w * x) * o2 + (double)means[3ull * src + 1]);
    out[2] = (float)(h * (x * z - w * y) * o0 + h * (y * z + w * x) * o1 + (1.0 - h * (x * x + y * y)) * o2 + (double)means[3ull * src + 2]);
}

// per-thread memo of the last child row whose means were computed: a thread's four floats touch at most two rows
struct DnChildMemo {
    unsigned row;
    float m[3];
};

template <int KIND>
__device__ __forceinline__ float dn_element(const DnRows& R, const float* __restrict__ src, unsigned row, unsigned col, unsigned F,
                                            unsigned srow, DnChildMemo& memo)
{
    const bool child = row >= R.n_sel && row < R.n_sel + R.n_children;
    if (KIND == GS_DENSIFY_MOMENT) return row < R.n_sel ? src[(size_t)srow * F + col] : 0.0f;
    if (KIND == GS_DENSIFY_MEANS && child) {
        if (memo.row != row) {
            dn_child_mean(R, srow, row - R.n_sel, src, memo.m);
            memo.row = row;
        }
        return col == 0u ? memo.m[0] : (col == 1u ? memo.m[1] : memo.m[2]);
    }
    const float v = src[(size_t)srow * F + col];
    if (KIND == GS_DENSIFY_SCALES && child) return logf(expf(v) * 0.625f);         // 1 / 1.6
    return v;
}

__device__ __forceinline__ unsigned dn_source_row(const DnRows& R, unsigned row)
{
    const int s = R.rowmap[row];
    return (unsigned)(s < 0 ? 0 : ((long long)s < R.N ? s : (int)(R.N - 1)));      // (a row map the plan did not write cannot read outside)
}

// One tensor per blockIdx.y.  The output of a tensor is the flat array dst[N_out * F]; a thread owns four consecutive floats of it, so a
// wave stores 1 KiB contiguous per instruction whatever F is (the 45-float SH row is 180 B: rows straddle the 16-byte pieces).
template <int KIND, int FC>
__device__ __forceinline__ void dn_gather_body(const DnRows& R, const float* __restrict__ src, float* __restrict__ dst, unsigned Fdyn,
                                               bool wide_store, bool wide_load)
{
    const unsigned F = FC > 0 ? (unsigned)FC : Fdyn;
    const unsigned total = R.N_out * F;                                             // < 2^31 (checked on the host)
    const unsigned n_pieces = (total + 3u) / 4u;
    for (unsigned p = blockIdx.x * DN_BLOCK + threadIdx.x; p < n_pieces; p += gridDim.x * DN_BLOCK) {
        const unsigned e0 = 4u * p;
        unsigned row = e0 / F, col = e0 - row * F;
        unsigned srow = dn_source_row(R, row);
        float v[4];
        DnChildMemo memo;
        memo.row = 0xffffffffu;
        if ((KIND == GS_DENSIFY_COPY || KIND == GS_DENSIFY_MOMENT) && wide_load) {   // F % 4 == 0: the piece lies in one row
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (KIND == GS_DENSIFY_COPY || row < R.n_sel) q = *reinterpret_cast<const float4*>(src + (size_t)srow * F + col);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = (e0 + k < total) ? dn_element<KIND>(R, src, row, col, F, srow, memo) : 0.0f;
                if (++col == F) {
                    col = 0u;
                    ++row;
                    if (row < R.N_out) srow = dn_source_row(R, row);
                }
            }
        }
        if (wide_store && e0 + 4u <= total) {
            *reinterpret_cast<float4*>(dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < total) dst[e0 + k] = v[k];
        }
    }
}

static __global__ void __launch_bounds__(DN_BLOCK) densify_gather_kernel(DnTable T, DnRows R)
{
    const int t = blockIdx.y;
    const float* __restrict__ src = T.src[t];
    float* __restrict__ dst = T.dst[t];
    const unsigned F = (unsigned)T.floats_per_row[t];
    const bool ws = T.wide_store[t] != 0, wl = T.wide_load[t] != 0;
    switch (T.kind[t]) {                                                             // block-uniform
    case GS_DENSIFY_MEANS: dn_gather_body<GS_DENSIFY_MEANS, 3>(R, src, dst, 3u, ws, false); break;
    case GS_DENSIFY_SCALES: dn_gather_body<GS_DENSIFY_SCALES, 3>(R, src, dst, 3u, ws, false); break;
    case GS_DENSIFY_MOMENT:
        if (F == 45u) dn_gather_body<GS_DENSIFY_MOMENT, 45>(R, src, dst, F, ws, false);
        else if (F == 3u) dn_gather_body<GS_DENSIFY_MOMENT, 3>(R, src, dst, F, ws, false);
        else if (F == 4u) dn_gather_body<GS_DENSIFY_MOMENT, 4>(R, src, dst, F, ws, wl);
        else if (F == 1u) dn_gather_body<GS_DENSIFY_MOMENT, 1>(R, src, dst, F, ws, false);
        else dn_gather_body<GS_DENSIFY_MOMENT, 0>(R, src, dst, F, ws, wl);
        break;
    default:
        if (F == 45u) dn_gather_body<GS_DENSIFY_COPY, 45>(R, src, dst, F, ws, false);
        else if (F == 3u) dn_gather_body<GS_DENSIFY_COPY, 3>(R, src, dst, F, ws, false);
        else if (F == 4u) dn_gather_body<GS_DENSIFY_COPY, 4>(R, src, dst, F, ws, wl);
        else if (F == 1u) dn_gather_body<GS_DENSIFY_COPY, 1>(R, src, dst, F, ws, false);
        else dn_gather_body<GS_DENSIFY_COPY, 0>(R, src, dst, F, ws, wl);
        break;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" {

int gs_densify_stats(int V, const int64_t* gaussian_ids, const float* v_means2d, int64_t N, float* xys_grad_norm, float* vis_counts,
                     void* stream)
{
    GS_CHECK_ARG(V >= 0, "V must be >= 0");
    GS_CHECK_ARG(N >= 0, "N must be >= 0");
    if (V == 0 || N == 0) return GS_OK;
    GS_CHECK_ARG(gaussian_ids && v_means2d && xys_grad_norm && vis_counts, "null pointer");
    hipLaunchKernelGGL(densify_stats_kernel, dim3(gs_cdiv(V, DN_BLOCK)), dim3(DN_BLOCK), 0, (hipStream_t)stream, V,
                       (const long long*)gaussian_ids, (const float2*)v_means2d, (long long)N, xys_grad_norm, vis_counts);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

size_t gs_densify_ws_bytes(int64_t N, int num_splits)
{
    if (N <= 0 || N > GS_DENSIFY_MAX_N || num_splits < 0 || num_splits > GS_DENSIFY_MAX_SPLITS) return 0;
    return dn_layout(nullptr, N, num_splits).total;
}

int gs_densify_plan(int64_t N, const float* scales, const float* opacities, const float* xys_grad_norm, const float* vis_counts,
                    float half_extent, float grad_thresh, float size_thresh, float alpha_thresh, float scale_thresh, int num_splits,
                    int mode, void* ws, size_t ws_bytes, int64_t* totals, void* stream)
{
    GS_CHECK_ARG(N > 0 && N <= GS_DENSIFY_MAX_N, "N must be in [1, 2^27]");
    GS_CHECK_ARG(mode == GS_DENSIFY_MODE_DENSIFY || mode == GS_DENSIFY_MODE_CULL, "mode must be 0 (densify_and_cull) or 1 (cull)");
    GS_CHECK_ARG(num_splits >= 0 && num_splits <= GS_DENSIFY_MAX_SPLITS, "num_splits must be in [0, 8]");
    GS_CHECK_ARG(mode == GS_DENSIFY_MODE_CULL || num_splits >= 1, "num_splits must be >= 1 for densify_and_cull");
    const DnLayout L = dn_layout(ws, N, num_splits);
    if (!ws || ws_bytes < L.total) {
        gs_set_error("%s: workspace too small (%zu < %zu)", __func__, ws ? ws_bytes : (size_t)0, L.total);
        return ws ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(scales && opacities && totals, "null pointer");
    GS_CHECK_ARG(mode == GS_DENSIFY_MODE_CULL || (xys_grad_norm && vis_counts), "densify_and_cull needs xys_grad_norm and vis_counts");
    DnThresholds t{half_extent, grad_thresh, size_thresh, alpha_thresh, scale_thresh, mode};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(densify_classify_kernel, dim3(L.nb), dim3(DN_BLOCK), 0, s, (long long)N, scales, opacities, xys_grad_norm,
                       vis_counts, t, L.flags, L.blocks, L.nb);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(DN_SCAN_THREADS), 0, s, L.blocks, L.nb,
                       mode == GS_DENSIFY_MODE_CULL ? 0 : num_splits, (long long*)totals);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_densify_fill(int64_t N, int num_splits, void* ws, size_t ws_bytes, int64_t n_selected, int64_t n_split, int64_t n_dup,
                    const GsDensifyTensor* table, int n_tensors, const float* quats, const float* scales, const float* randn,
                    int64_t* indices, void* stream)
{
    GS_CHECK_ARG(N > 0 && N <= GS_DENSIFY_MAX_N, "N must be in [1, 2^27]");
    GS_CHECK_ARG(num_splits >= 0 && num_splits <= GS_DENSIFY_MAX_SPLITS, "num_splits must be in [0, 8]");
    GS_CHECK_ARG(n_selected >= 0 && n_split >= 0 && n_dup >= 0 && n_selected + n_split <= N && n_dup <= N, "totals out of range");
    GS_CHECK_ARG(n_tensors >= 0 && n_tensors <= GS_DENSIFY_MAX_TENSORS, "n_tensors must be in [0, 32]");
    GS_CHECK_ARG(n_tensors == 0 || table, "null table");
    const DnLayout L = dn_layout(ws, N, num_splits);
    if (!ws || ws_bytes < L.total) {
        gs_set_error("%s: workspace too small (%zu < %zu)", __func__, ws ? ws_bytes : (size_t)0, L.total);
        return ws ? GS_ENOSPC : GS_EINVAL;
    }
    const int64_t n_children = (int64_t)num_splits * n_split;
    const int64_t N_out = n_selected + n_children + n_dup;
    GS_CHECK_ARG(n_split == 0 || num_splits >= 1, "split rows need num_splits >= 1");
    GS_CHECK_ARG(N_out <= N * (int64_t)(num_splits > 2 ? num_splits : 2), "totals exceed the row map of the workspace");
    if (N_out == 0) return GS_OK;
    GS_CHECK_ARG(indices, "null indices");
    DnTable T;
    int64_t max_total = 0;
    for (int k = 0; k < GS_DENSIFY_MAX_TENSORS; ++k) {
        T.src[k] = nullptr; T.dst[k] = nullptr; T.floats_per_row[k] = 1; T.kind[k] = GS_DENSIFY_COPY; T.wide_store[k] = 0; T.wide_load[k] = 0;
    }
    bool need_child = false;
    for (int k = 0; k < n_tensors; ++k) {
        const GsDensifyTensor& e = table[k];
        GS_CHECK_ARG(e.src && e.dst, "null tensor in the table");
        GS_CHECK_ARG(e.floats_per_row >= 1, "floats_per_row must be >= 1");
        GS_CHECK_ARG(e.kind >= GS_DENSIFY_COPY && e.kind <= GS_DENSIFY_MOMENT, "unknown tensor kind");
        GS_CHECK_ARG((e.kind != GS_DENSIFY_MEANS && e.kind != GS_DENSIFY_SCALES) || e.floats_per_row == 3, "means / scales rows are 3 floats");
        const int64_t total = N_out * (int64_t)e.floats_per_row;
        GS_CHECK_ARG(total < ((int64_t)1 << 31) - 4, "N_out * floats_per_row must stay below 2^31");
        if (total > max_total) max_total = total;
        if (e.kind == GS_DENSIFY_MEANS) need_child = true;
        T.src[k] = e.src; T.dst[k] = e.dst; T.floats_per_row[k] = e.floats_per_row; T.kind[k] = e.kind;
        T.wide_store[k] = (((uintptr_t)e.dst) & 15) == 0;
        T.wide_load[k] = (((uintptr_t)e.src) & 15) == 0 && (e.floats_per_row % 4) == 0;
    }
    GS_CHECK_ARG(!(need_child && n_children > 0) || (quats && scales && randn), "child means need quats, scales and randn");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(densify_map_kernel, dim3(L.nb), dim3(DN_BLOCK), 0, s, (long long)N, num_splits, L.flags, L.blocks, L.nb,
                       (long long)n_selected, (long long)n_split, (long long)N_out, L.rowmap, (long long*)indices);
    GS_CHECK_LAUNCH();
    if (n_tensors == 0) return GS_OK;
    DnRows R{(long long)N, (unsigned)n_selected, (unsigned)n_split, (unsigned)n_children, (unsigned)N_out, L.rowmap, quats, scales, randn};
    const int64_t want = (max_total / 4 + DN_BLOCK) / DN_BLOCK;
    const int gx = (int)(want < 16384 ? want : 16384);                               // grid-stride above 16 Mi floats per tensor
    hipLaunchKernelGGL(densify_gather_kernel, dim3(gx, n_tensors), dim3(DN_BLOCK), 0, s, T, R);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

}  // extern "C"
