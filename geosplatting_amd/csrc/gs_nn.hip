// gs_nn.hip -- exact nearest-neighbour search of N query points in a set of M points (fp32 [.,3]) and the backward of the Chamfer
// pair: what the reference's geometry metrics get from its brute-force Chamfer kernel (rfstudio/loss/_chamfer) and from
// Points.k_nearest.  A from-scratch statement of the semantics in include/geosplat_hip.h: a uniform grid built on the device, a
// shell search that is exact to the bit, the k-nearest form of the same traversal, and the brute-force form of both.
//
// Build (six small launches + the radix passes of gs_sort.hip, nothing read back, no workgroup waits on another):
//   nn_init       resets the bounds
//   nn_bounds     bounds of the finite points (ordered-integer atomic min / max)
//   nn_layout     one thread: per-axis resolution and cell size into the grid header
//   nn_keys       key = cell of every point (finite points; the others get the code one past the last cell), payload = point index
//   gs_isect_sort stable ascending over the cell bits: equal cells keep ascending point index, i.e. the (cell << 32 | index) order
//   nn_gather     16-byte (x, y, z, index bits) records in sorted order
//   nn_cellstart  one thread per cell: first sorted position whose cell is >= this one, by binary search (no serial run over empty
//                 cells, whatever the distribution)
//
// Query: one thread per query.  Shell r is the cube of cells [home - r, home + r] clipped to the grid, minus the cube of shell
// r - 1; along z the cells of a column are adjacent in the sorted order, so a column is ONE run of records.  After shell r the search
// stops iff the (k-th) best d is STRICTLY below a lower bound on the fp32 d of every point outside the cube (nn_outside_bound), or the
// cube covers the grid.  Inside a shell a plane, a column or a cell is skipped when the same kind of bound for its own box is above
// the best d (nn_range_gap): a query far outside the box then reads the slab of cells that faces it, not the set.  The k best are
// a fixed-size sorted list with one kernel instantiation per k.  The brute-force form runs the SAME distance routine over every point
// through LDS tiles.
#include "gs_common.h"
#include "gs_ws.h"

#define NN_BLOCK 256
#define NN_MAX_POINTS ((int64_t)1 << 30)
#define NN_MAX_CELLS (1 << 21)
#define NN_MAX_K 8
#define NN_SORT_TILES 1                        // gs_isect_sort sorts 32 + tile_bits(1 x 1) = 33 key bits: every bit of a cell code
#define NN_TILE 1024                           // points per LDS tile of the brute-force form (16 KB)
#define NN_EMPTY 0x7fffffff                    // index of an unused slot: sorts behind every point among equal d

// ---- grid buffer ---------------------------------------------------------------------------------------------------------------
struct NnHeader {                              // the first 256 bytes of the grid buffer
    unsigned bounds[6];                        // ordered-integer min xyz, max xyz of the finite points
    float lo[3];                               // box minimum
    float inv_h[3];                            // cells per unit length: cell = clamp((int)((c - lo) * inv_h), 0, res - 1); 0 where res = 1
    int res[3];
    int ncells;                                // res[0] res[1] res[2] <= nn_max_cells(M)
    double h[3];                               // 1 / (double)inv_h: the cell size the bound uses
    double ext[3];                             // box maximum - box minimum in fp64
};
static int64_t nn_max_cells(int64_t M)
{
    const int64_t t = M / 4;
    return t < 1 ? 1 : (t > NN_MAX_CELLS ? NN_MAX_CELLS : t);
}
struct NnGrid { NnHeader* hdr; int* cell_start; float4* rec; size_t total; };
static NnGrid nn_grid_layout(int64_t M, const void* base)
{
    GsWs w((void*)base, 256);
    NnGrid G;
    G.hdr = (NnHeader*)w.take<char>(256);
    G.cell_start = w.take<int>((size_t)(nn_max_cells(M) + 1));           // cell_start[ncells + 1], sized for the most cells
    G.rec = w.take<float4>((size_t)M);
    G.total = w.bytes();
    return G;
}
struct NnWs { unsigned long long *keys, *skeys; int *vals, *svals; char* sort; size_t sort_bytes, total; };
static NnWs nn_ws_layout(int64_t M, void* base)
{
    GsWs w(base, 256);
    NnWs L;
    const size_t m = (size_t)M;
    L.keys = w.take<unsigned long long>(m);
    L.vals = w.take<int>(m);
    L.skeys = w.take<unsigned long long>(m);
    L.svals = w.take<int>(m);
    L.sort_bytes = gs_sort_ws_bytes(M, NN_SORT_TILES, NN_SORT_TILES);
    L.sort = w.take<char>(L.sort_bytes);
    L.total = w.bytes();
    return L;
}

// ---- small device helpers ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned nn_ord(float x)               // order-preserving map of the finite floats to unsigned
{
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float nn_unord(unsigned u)
{
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ bool nn_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool nn_finite3(float x, float y, float z) { return nn_finite(x) && nn_finite(y) && nn_finite(z); }

// THE distance: (dx dx + dy dy) + dz dz, every operation one fp32 round-to-nearest, no contraction
__device__ __forceinline__ float nn_dist(float qx, float qy, float qz, float px, float py, float pz)
{
#pragma clang fp contract(off)
    const float dx = qx - px;
    const float dy = qy - py;
    const float dz = qz - pz;
    const float xx = dx * dx;
    const float yy = dy * dy;
    const float zz = dz * dz;
    const float s = xx + yy;
    return s + zz;
}

// cell of a coordinate along one axis: monotone non-decreasing in c (a subtraction, a product by a non-negative number, a clamp and a
// truncation of a non-negative number are all monotone) -- the bound below rests on that and on nothing else
__device__ __forceinline__ int nn_cell1(float c, float lo, float inv_h, int res)
{
#pragma clang fp contract(off)
    const float u = c - lo;
    const float v = u * inv_h;
    return (int)fminf(fmaxf(v, 0.0f), (float)(res - 1));          // (fmaxf drops the NaN of inf * 0)
}

// the k smallest (d, index) pairs seen so far, ascending, in registers
template <int K>
struct NnTop {
    float d[K];
    int i[K];
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int j = 0; j < K; ++j) { d[j] = __builtin_inff(); i[j] = NN_EMPTY; }
    }
    __device__ __forceinline__ void insert(float nd, int ni)
    {
        if (!(nd < d[K - 1] || (nd == d[K - 1] && ni < i[K - 1]))) return;          // (a NaN d never enters)
        d[K - 1] = nd; i[K - 1] = ni;
#pragma unroll
        for (int j = K - 1; j > 0; --j) {
            const bool sw = d[j] < d[j - 1] || (d[j] == d[j - 1] && i[j] < i[j - 1]);
            const float td = sw ? d[j - 1] : d[j], ud = sw ? d[j] : d[j - 1];
            const int ti = sw ? i[j - 1] : i[j], ui = sw ? i[j] : i[j - 1];
            d[j] = td; i[j] = ti; d[j - 1] = ud; i[j - 1] = ui;
        }
    }
    __device__ __forceinline__ float kth() const { return d[K - 1]; }          // d of the K-th smallest
    __device__ __forceinline__ void store(long long q, float* __restrict__ dist, int* __restrict__ index) const
    {
#pragma unroll
        for (int j = 0; j < K; ++j) { dist[q * K + j] = d[j]; index[q * K + j] = (i[j] == NN_EMPTY) ? -1 : i[j]; }
    }
};

// ---- build kernels -------------------------------------------------------------------------------------------------------------
static __global__ void nn_init_kernel(NnHeader* __restrict__ hdr)
{
    if (threadIdx.x < 6) hdr->bounds[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
}

static __global__ void __launch_bounds__(NN_BLOCK) nn_bounds_kernel(long long M, const float* __restrict__ points, NnHeader* __restrict__ hdr)
{
    __shared__ unsigned sb[6];
    if (threadIdx.x < 6) sb[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
    __syncthreads();
    unsigned lo0 = 0xffffffffu, lo1 = 0xffffffffu, lo2 = 0xffffffffu, hi0 = 0u, hi1 = 0u, hi2 = 0u;
    for (long long i = (long long)blockIdx.x * NN_BLOCK + threadIdx.x; i < M; i += (long long)gridDim.x * NN_BLOCK) {
        const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
        if (!nn_finite3(x, y, z)) continue;
        lo0 = min(lo0, nn_ord(x)); hi0 = max(hi0, nn_ord(x));
        lo1 = min(lo1, nn_ord(y)); hi1 = max(hi1, nn_ord(y));
        lo2 = min(lo2, nn_ord(z)); hi2 = max(hi2, nn_ord(z));
    }
    atomicMin(&sb[0], lo0); atomicMin(&sb[1], lo1); atomicMin(&sb[2], lo2);
    atomicMax(&sb[3], hi0); atomicMax(&sb[4], hi1); atomicMax(&sb[5], hi2);
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&hdr->bounds[threadIdx.x], sb[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&hdr->bounds[threadIdx.x], sb[threadIdx.x]);
}

// Per-axis resolution: cubic cells of volume (box volume / max_cells) over the axes that have an extent, every other axis one cell;
// the largest resolution is halved until the product fits.  An axis whose extent or cells-per-length is not a finite positive
// fp32 number (a box wider than FLT_MAX, an extent in the denormals) gets one cell too: the search then scans along it.
static __global__ void nn_layout_kernel(int max_cells, NnHeader* __restrict__ hdr)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float ext[3];
    bool on[3];
    const bool any = hdr->bounds[0] <= hdr->bounds[3];
    int n_on = 0;
    double vol = 1.0;
    for (int a = 0; a < 3; ++a) {
        const float lo = any ? nn_unord(hdr->bounds[a]) : 0.0f, hi = any ? nn_unord(hdr->bounds[3 + a]) : 0.0f;
        hdr->lo[a] = lo;
        hdr->ext[a] = (double)hi - (double)lo;
        ext[a] = hi - lo;
        on[a] = any && ext[a] > 1e-30f && nn_finite(ext[a]);
        if (on[a]) { ++n_on; vol *= (double)ext[a]; }
    }
    int res[3] = { 1, 1, 1 };
    if (n_on > 0) {
        const double cell = pow(vol / (double)max_cells, 1.0 / (double)n_on);
        for (int a = 0; a < 3; ++a)
            if (on[a]) {
                const double r = floor((double)ext[a] / cell);
                res[a] = r < 1.0 ? 1 : (r > (double)max_cells ? max_cells : (int)r);
            }
        while ((long long)res[0] * res[1] * res[2] > (long long)max_cells) {
            const int a = (res[0] >= res[1] && res[0] >= res[2]) ? 0 : (res[1] >= res[2] ? 1 : 2);
            res[a] = (res[a] + 1) / 2;
        }
    }
    for (int a = 0; a < 3; ++a) {
        float inv_h = res[a] > 1 ? (float)res[a] / ext[a] : 0.0f;
        if (!nn_finite(inv_h) || !(inv_h > 0.0f)) { inv_h = 0.0f; res[a] = 1; }
        hdr->res[a] = res[a];
        hdr->inv_h[a] = inv_h;
        hdr->h[a] = inv_h > 0.0f ? 1.0 / (double)inv_h : 0.0;
    }
    hdr->ncells = res[0] * res[1] * res[2];
}

static __global__ void __launch_bounds__(NN_BLOCK) nn_keys_kernel(long long M, const float* __restrict__ points, const NnHeader* __restrict__ hdr,
                                                                  unsigned long long* __restrict__ keys, int* __restrict__ vals)
{
    const long long i = (long long)blockIdx.x * NN_BLOCK + threadIdx.x;
    if (i >= M) return;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    unsigned cell = (unsigned)hdr->ncells;                                            // a non-finite point: behind every cell
    if (nn_finite3(x, y, z)) {
        const int ix = nn_cell1(x, hdr->lo[0], hdr->inv_h[0], hdr->res[0]);
        const int iy = nn_cell1(y, hdr->lo[1], hdr->inv_h[1], hdr->res[1]);
        const int iz = nn_cell1(z, hdr->lo[2], hdr->inv_h[2], hdr->res[2]);
        cell = (unsigned)((ix * hdr->res[1] + iy) * hdr->res[2] + iz);
    }
    keys[i] = (unsigned long long)cell;
    vals[i] = (int)i;
}

static __global__ void __launch_bounds__(NN_BLOCK) nn_gather_kernel(long long M, const float* __restrict__ points, const int* __restrict__ svals,
                                                                    float4* __restrict__ rec)
{
    const long long i = (long long)blockIdx.x * NN_BLOCK + threadIdx.x;
    if (i >= M) return;
    int p = svals[i];
    p = p < 0 ? 0 : (p >= M ? (int)(M - 1) : p);
    rec[i] = make_float4(points[3 * (long long)p], points[3 * (long long)p + 1], points[3 * (long long)p + 2], __int_as_float(p));
}

// cell_start[c] = first sorted position whose cell code is >= c, for c in [0, ncells]: cell c holds records
// [cell_start[c], cell_start[c + 1]), and cell_start[ncells] is the number of finite points
static __global__ void __launch_bounds__(NN_BLOCK) nn_cellstart_kernel(long long M, const unsigned long long* __restrict__ skeys,
                                                                       const NnHeader* __restrict__ hdr, int* __restrict__ cell_start)
{
    const long long c = (long long)blockIdx.x * NN_BLOCK + threadIdx.x;
    if (c > hdr->ncells) return;
    long long lo = 0, hi = M;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (skeys[mid] < (unsigned long long)c) lo = mid + 1; else hi = mid;
    }
    cell_start[c] = (int)lo;
}

// ---- queries -------------------------------------------------------------------------------------------------------------------
// A lower bound on the fp32 d of every set point whose cell along this axis is below a0 or above a1, for a query coordinate q.
//   cell(c) >= k  =>  fl(fl(c - lo) inv_h) >= k  =>  c - lo >= k h (1 - 2^-23)      (two roundings, h = 1 / inv_h)
//   cell(c) <= k  =>  fl(fl(c - lo) inv_h) < k + 1  =>  c - lo < (k + 1) h (1 + 2^-22)
// so the point is at least gap = (face moved by 2^-21 relative towards the query) - q away along the axis, evaluated in fp64 with
// an absolute slack of 2^-50 of the magnitudes involved for fp64's own rounding.  d >= fl(fl(dx)^2) by monotonicity of rounding
// (the other squares are non-negative) and |fl(dx)| >= gap (1 - 2^-24), so gap^2 (1 - 2^-20), rounded to fp32, is a bound.
__device__ __forceinline__ double nn_axis_bound(double q, double lo, double h, int a0, int a1, int res)
{
    const double eps = 1.0 / 2097152.0, tiny = 1.0 / 1125899906842624.0;
    double b = __builtin_inf();
    if (a0 > 0) {                                               // points below: cell <= a0 - 1
        const double face = (double)a0 * h * (1.0 + eps);
        const double gap = (q - lo) - face - tiny * (fabs(q) + fabs(lo) + face);
        b = gap > 0.0 ? gap * gap : 0.0;
    }
    if (a1 < res - 1) {                                         // points above: cell >= a1 + 1
        const double face = (double)(a1 + 1) * h * (1.0 - eps);
        const double gap = face - (q - lo) - tiny * (fabs(q) + fabs(lo) + face);
        const double b1 = gap > 0.0 ? gap * gap : 0.0;
        b = b1 < b ? b1 : b;
    }
    return b;
}

// The same two facts give a lower bound on the distance along one axis to the points whose cell lies in [c0, c1]; the first cell
// starts at the box minimum and the last one ends at the box maximum (qrel = q - lo and ext = hi - lo, both in fp64).  Runs of cells
// whose bound is above the (k-th) best d are skipped: that only saves work, the answer does not depend on it.
__device__ __forceinline__ double nn_range_gap(double qrel, double slack, double h, double ext, int c0, int c1, int res)
{
    const double eps = 1.0 / 2097152.0;
    const double below = c0 > 0 ? (double)c0 * h * (1.0 - eps) : 0.0;
    const double above = c1 < res - 1 ? (double)(c1 + 1) * h * (1.0 + eps) : ext;
    const double g = fmax(below - qrel, qrel - above) - slack;
    return g > 0.0 ? g : 0.0;
}
// every fp32 d of a run is above `best` when the sum s of its squared gaps is: d >= s (1 - 6 2^-24) as long as no square underflows
// (s >= 1e-30 keeps clear of that), and a float d >= b has d >= fl(b)
__device__ __forceinline__ bool nn_skip(double s, float best)
{
    return s >= 1e-30 && (float)(s * (1.0 - 1.0 / 1048576.0)) > best;
}

template <int K>
__device__ __forceinline__ void nn_scan(const float4* __restrict__ rec, int s, int e, float qx, float qy, float qz, NnTop<K>& top)
{
    for (int j = s; j < e; ++j) {
        const float4 p = rec[j];
        top.insert(nn_dist(qx, qy, qz, p.x, p.y, p.z), __float_as_int(p.w));
    }
}

template <int K>
static __global__ void __launch_bounds__(NN_BLOCK) nn_grid_query_kernel(long long M, const NnHeader* __restrict__ hdr,
                                                                        const int* __restrict__ cell_start, const float4* __restrict__ rec,
                                                                        long long N, const float* __restrict__ queries,
                                                                        float* __restrict__ dist, int* __restrict__ index)
{
    const long long q = (long long)blockIdx.x * NN_BLOCK + threadIdx.x;
    if (q >= N) return;
    NnTop<K> top;
    top.init();
    const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
    if (!nn_finite3(qx, qy, qz)) { top.store(q, dist, index); return; }
    // a header that is not a grid of this set (never built, overwritten) gives a scan of one cell, not a fault
    int rx = hdr->res[0], ry = hdr->res[1], rz = hdr->res[2];
    const bool sane = rx >= 1 && ry >= 1 && rz >= 1 && (long long)rx * ry * rz == (long long)hdr->ncells && hdr->ncells <= NN_MAX_CELLS &&
                      (long long)hdr->ncells <= (M / 4 < 1 ? 1 : M / 4);
    if (!sane) { top.store(q, dist, index); return; }
    const int hx = nn_cell1(qx, hdr->lo[0], hdr->inv_h[0], rx), hy = nn_cell1(qy, hdr->lo[1], hdr->inv_h[1], ry),
              hz = nn_cell1(qz, hdr->lo[2], hdr->inv_h[2], rz);
    const int m32 = (int)M;
    const double tiny = 1.0 / 1125899906842624.0;
    const double hx_ = hdr->h[0], hy_ = hdr->h[1], hz_ = hdr->h[2], ex = hdr->ext[0], ey = hdr->ext[1], ez = hdr->ext[2];
    const double qrx = (double)qx - (double)hdr->lo[0], qry = (double)qy - (double)hdr->lo[1], qrz = (double)qz - (double)hdr->lo[2];
    const double slx = tiny * (fabs((double)qx) + fabs((double)hdr->lo[0]) + ex + (double)rx * hx_);
    const double sly = tiny * (fabs((double)qy) + fabs((double)hdr->lo[1]) + ey + (double)ry * hy_);
    const double slz = tiny * (fabs((double)qz) + fabs((double)hdr->lo[2]) + ez + (double)rz * hz_);
    for (int r = 0;; ++r) {
        const int x0 = max(hx - r, 0), x1 = min(hx + r, rx - 1), y0 = max(hy - r, 0), y1 = min(hy + r, ry - 1);
        const int z0 = max(hz - r, 0), z1 = min(hz + r, rz - 1);
        double gz = nn_range_gap(qrz, slz, hz_, ez, z0, z1, rz);
        const double gz2 = gz * gz;
        gz = hz - r >= 0 ? nn_range_gap(qrz, slz, hz_, ez, hz - r, hz - r, rz) : 0.0;
        const double gz2_lo = gz * gz;
        gz = hz + r <= rz - 1 ? nn_range_gap(qrz, slz, hz_, ez, hz + r, hz + r, rz) : 0.0;
        const double gz2_hi = gz * gz;
        for (int ix = x0; ix <= x1; ++ix) {
            const double gx = nn_range_gap(qrx, slx, hx_, ex, ix, ix, rx);
            const double gx2 = gx * gx;
            if (nn_skip(gx2, top.kth())) continue;
            for (int iy = y0; iy <= y1; ++iy) {
                const double gy = nn_range_gap(qry, sly, hy_, ey, iy, iy, ry);
                const double gxy2 = gx2 + gy * gy;
                const int col = (ix * ry + iy) * rz;
                const bool inner = r > 0 && abs(ix - hx) < r && abs(iy - hy) < r;      // a column of the cube already searched
                if (!inner) {
                    if (nn_skip(gxy2 + gz2, top.kth())) continue;
                    const int s = cell_start[col + z0], e = cell_start[col + z1 + 1];
                    nn_scan<K>(rec, max(s, 0), min(e, m32), qx, qy, qz, top);
                } else {
                    if (hz - r >= 0 && !nn_skip(gxy2 + gz2_lo, top.kth())) {
                        const int s = cell_start[col + hz - r], e = cell_start[col + hz - r + 1];
                        nn_scan<K>(rec, max(s, 0), min(e, m32), qx, qy, qz, top);
                    }
                    if (hz + r <= rz - 1 && !nn_skip(gxy2 + gz2_hi, top.kth())) {
                        const int s = cell_start[col + hz + r], e = cell_start[col + hz + r + 1];
                        nn_scan<K>(rec, max(s, 0), min(e, m32), qx, qy, qz, top);
                    }
                }
            }
        }
        if (x0 == 0 && x1 == rx - 1 && y0 == 0 && y1 == ry - 1 && z0 == 0 && z1 == rz - 1) break;      // the cube covers the grid
        const double bx = nn_axis_bound((double)qx, (double)hdr->lo[0], hdr->h[0], x0, x1, rx);
        const double by = nn_axis_bound((double)qy, (double)hdr->lo[1], hdr->h[1], y0, y1, ry);
        const double bz = nn_axis_bound((double)qz, (double)hdr->lo[2], hdr->h[2], z0, z1, rz);
        const double b = fmin(bx, fmin(by, bz)) * (1.0 - 1.0 / 1048576.0);
        if (top.kth() < (float)b) break;                          // strict: an equal d outside may carry a lower index
    }
    top.store(q, dist, index);
}

template <int K>
static __global__ void __launch_bounds__(NN_BLOCK) nn_brute_query_kernel(long long M, const float* __restrict__ points, long long N,
                                                                         const float* __restrict__ queries, float* __restrict__ dist,
                                                                         int* __restrict__ index)
{
    __shared__ float4 tile[NN_TILE];
    const long long q = (long long)blockIdx.x * NN_BLOCK + threadIdx.x;
    NnTop<K> top;
    top.init();
    float qx = __builtin_nanf(""), qy = qx, qz = qx;                // a query that is absent or non-finite meets only NaN distances
    if (q < N) {
        const float x = queries[3 * q], y = queries[3 * q + 1], z = queries[3 * q + 2];
        if (nn_finite3(x, y, z)) { qx = x; qy = y; qz = z; }
    }
    for (long long base = 0; base < M; base += NN_TILE) {
        const int n = (int)min((long long)NN_TILE, M - base);
        __syncthreads();
        for (int t = threadIdx.x; t < n; t += NN_BLOCK) {
            const long long p = base + t;
            float x = points[3 * p];
            const float y = points[3 * p + 1], z = points[3 * p + 2];
            if (!nn_finite3(x, y, z)) x = __builtin_nanf("");        // never returned: its d is NaN
            tile[t] = make_float4(x, y, z, __int_as_float((int)p));
        }
        __syncthreads();
        for (int t = 0; t < n; ++t) {
            const float4 p = tile[t];
            top.insert(nn_dist(qx, qy, qz, p.x, p.y, p.z), __float_as_int(p.w));
        }
    }
    if (q < N) top.store(q, dist, index);
}

// ---- Chamfer backward ----------------------------------------------------------------------------------------------------------
// own rows first (plain stores), the scattered halves in a second launch (atomics): no buffer needs zeroing by anybody
static __global__ void __launch_bounds__(NN_BLOCK) chamfer_bwd_own_kernel(long long Na, long long Nb, const float* __restrict__ a,
                                                                          const float* __restrict__ b, const int* __restrict__ idx,
                                                                          const float* __restrict__ grad, float* __restrict__ grad_a)
{
#pragma clang fp contract(off)
    const long long j = (long long)blockIdx.x * NN_BLOCK + threadIdx.x;
    if (j >= Na) return;
    const int i = idx[j];
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (i >= 0 && i < Nb) {
        const float g = 2.0f * grad[j];
        gx = g * (a[3 * j] - b[3 * (long long)i]);
        gy = g * (a[3 * j + 1] - b[3 * (long long)i + 1]);
        gz = g * (a[3 * j + 2] - b[3 * (long long)i + 2]);
    }
    grad_a[3 * j] = gx; grad_a[3 * j + 1] = gy; grad_a[3 * j + 2] = gz;
}
static __global__ void __launch_bounds__(NN_BLOCK) chamfer_bwd_scatter_kernel(long long Na, long long Nb, const float* __restrict__ a,
                                                                              const float* __restrict__ b, const int* __restrict__ idx,
                                                                              const float* __restrict__ grad, float* __restrict__ grad_b)
{
#pragma clang fp contract(off)
    const long long j = (long long)blockIdx.x * NN_BLOCK + threadIdx.x;
    if (j >= Na) return;
    const int i = idx[j];
    if (i < 0 || i >= Nb) return;
    const float g = 2.0f * grad[j];
    gs_atomic_add(&grad_b[3 * (long long)i], -(g * (a[3 * j] - b[3 * (long long)i])));
    gs_atomic_add(&grad_b[3 * (long long)i + 1], -(g * (a[3 * j + 1] - b[3 * (long long)i + 1])));
    gs_atomic_add(&grad_b[3 * (long long)i + 2], -(g * (a[3 * j + 2] - b[3 * (long long)i + 2])));
}

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t gs_nn_grid_bytes(int64_t M)
{
    if (M < 1 || M > NN_MAX_POINTS) return 0;
    return nn_grid_layout(M, nullptr).total;
}

extern "C" size_t gs_nn_ws_bytes(int64_t M)
{
    if (M < 1 || M > NN_MAX_POINTS) return 0;
    return nn_ws_layout(M, nullptr).total;
}

extern "C" int gs_nn_build(int64_t M, const float* points, void* grid, size_t grid_bytes, void* ws, size_t ws_bytes, void* stream)
{
    GS_CHECK_ARG(M >= 1, "empty set: M must be at least 1");
    GS_CHECK_ARG(M <= NN_MAX_POINTS, "too many points: at most 2^30");
    const NnGrid G = nn_grid_layout(M, grid);
    const NnWs L = nn_ws_layout(M, ws);
    GS_CHECK_ARG(grid_bytes >= G.total, "grid buffer too small");
    GS_CHECK_ARG(ws_bytes >= L.total, "workspace too small");
    GS_CHECK_ARG(points != nullptr, "points must not be NULL");
    GS_CHECK_ARG(grid != nullptr && ws != nullptr, "grid buffer and workspace must not be NULL");
    GS_CHECK_ARG(((uintptr_t)grid & 15) == 0 && ((uintptr_t)ws & 15) == 0, "grid buffer and workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int max_cells = (int)nn_max_cells(M);
    const int blocks = gs_cdiv(M, NN_BLOCK);
    hipLaunchKernelGGL(nn_init_kernel, dim3(1), dim3(64), 0, s, G.hdr);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_bounds_kernel, dim3(blocks < 512 ? blocks : 512), dim3(NN_BLOCK), 0, s, (long long)M, points, G.hdr);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_layout_kernel, dim3(1), dim3(64), 0, s, max_cells, G.hdr);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_keys_kernel, dim3(blocks), dim3(NN_BLOCK), 0, s, (long long)M, points, G.hdr, L.keys, L.vals);
    GS_CHECK_LAUNCH();
    const int rc = gs_isect_sort(M, (const int64_t*)L.keys, L.vals, (int64_t*)L.skeys, L.svals, NN_SORT_TILES, NN_SORT_TILES, L.sort,
                                 L.sort_bytes, stream);
    if (rc != GS_OK) return rc;
    hipLaunchKernelGGL(nn_gather_kernel, dim3(blocks), dim3(NN_BLOCK), 0, s, (long long)M, points, L.svals, G.rec);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(nn_cellstart_kernel, dim3(gs_cdiv(max_cells + 1, NN_BLOCK)), dim3(NN_BLOCK), 0, s, (long long)M, L.skeys, G.hdr, G.cell_start);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

template <int K>
static void nn_launch_query(int64_t M, const float* points, const void* grid, int64_t N, const float* queries, float* dist,
                            int32_t* index, hipStream_t s)
{
    const dim3 blocks(gs_cdiv(N, NN_BLOCK)), block(NN_BLOCK);
    if (grid != nullptr) {
        const NnGrid G = nn_grid_layout(M, grid);
        hipLaunchKernelGGL(nn_grid_query_kernel<K>, blocks, block, 0, s, (long long)M, (const NnHeader*)G.hdr, (const int*)G.cell_start,
                           (const float4*)G.rec, (long long)N, queries, dist, index);
    } else {
        hipLaunchKernelGGL(nn_brute_query_kernel<K>, blocks, block, 0, s, (long long)M, points, (long long)N, queries, dist, index);
    }
}

extern "C" int gs_nn_query(int64_t M, const float* points, const void* grid, int64_t N, const float* queries, int k, float* dist,
                           int32_t* index, void* stream)
{
    GS_CHECK_ARG(M >= 1, "empty set: M must be at least 1");
    GS_CHECK_ARG(M <= NN_MAX_POINTS, "too many points: at most 2^30");
    GS_CHECK_ARG(N >= 0, "negative N");
    GS_CHECK_ARG(k >= 1 && k <= NN_MAX_K, "k must be in [1, 8]");
    GS_CHECK_ARG(N <= NN_MAX_POINTS, "too many queries: at most 2^30");
    GS_CHECK_ARG(points != nullptr, "points must not be NULL");
    GS_CHECK_ARG(((uintptr_t)grid & 15) == 0, "grid buffer must be 16-byte aligned");
    if (N == 0) return GS_OK;
    GS_CHECK_ARG(queries != nullptr && dist != nullptr && index != nullptr, "queries and outputs must not be NULL");
    hipStream_t s = (hipStream_t)stream;
    switch (k) {                                  // one instantiation per k: every access to the k best is to a fixed register
    case 1: nn_launch_query<1>(M, points, grid, N, queries, dist, index, s); break;
    case 2: nn_launch_query<2>(M, points, grid, N, queries, dist, index, s); break;
    case 3: nn_launch_query<3>(M, points, grid, N, queries, dist, index, s); break;
    case 4: nn_launch_query<4>(M, points, grid, N, queries, dist, index, s); break;
    case 5: nn_launch_query<5>(M, points, grid, N, queries, dist, index, s); break;
    case 6: nn_launch_query<6>(M, points, grid, N, queries, dist, index, s); break;
    case 7: nn_launch_query<7>(M, points, grid, N, queries, dist, index, s); break;
    default: nn_launch_query<8>(M, points, grid, N, queries, dist, index, s); break;
    }
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_chamfer_bwd(int64_t N1, int64_t N2, const float* xyz1, const float* xyz2, const int32_t* idx1, const int32_t* idx2,
                              const float* grad1, const float* grad2, float* grad_xyz1, float* grad_xyz2, void* stream)
{
    GS_CHECK_ARG(N1 >= 1 && N2 >= 1, "empty set: N1 and N2 must be at least 1");
    GS_CHECK_ARG(N1 <= NN_MAX_POINTS && N2 <= NN_MAX_POINTS, "too many points: at most 2^30");
    GS_CHECK_ARG(xyz1 != nullptr && xyz2 != nullptr && idx1 != nullptr && idx2 != nullptr && grad1 != nullptr && grad2 != nullptr &&
                 grad_xyz1 != nullptr && grad_xyz2 != nullptr, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const dim3 b1(gs_cdiv(N1, NN_BLOCK)), b2(gs_cdiv(N2, NN_BLOCK)), block(NN_BLOCK);
    hipLaunchKernelGGL(chamfer_bwd_own_kernel, b1, block, 0, s, (long long)N1, (long long)N2, xyz1, xyz2, idx1, grad1, grad_xyz1);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(chamfer_bwd_own_kernel, b2, block, 0, s, (long long)N2, (long long)N1, xyz2, xyz1, idx2, grad2, grad_xyz2);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(chamfer_bwd_scatter_kernel, b1, block, 0, s, (long long)N1, (long long)N2, xyz1, xyz2, idx1, grad1, grad_xyz2);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(chamfer_bwd_scatter_kernel, b2, block, 0, s, (long long)N2, (long long)N1, xyz2, xyz1, idx2, grad2, grad_xyz1);
    GS_CHECK_LAUNCH();
    return GS_OK;
}
