// gs_tsdf.hip -- depth fusion into a dense TSDF volume and marching-cubes extraction: what the reference's MeshExport task does
// through TriangleMesh.from_depth_fusion (rfstudio/graphics/_mesh/_triangle_mesh.py:321-388, Open3D's ScalableTSDFVolume on the CPU).
//   gs_tsdf_integrate      : up to GS_TSDF_MAX_VIEWS depth maps per launch; one thread owns one voxel and keeps (tsdf, weight) in
//                            registers over the views, so the volume is read and written once per launch.  No atomics.
//   gs_tsdf_extract_count  : classify cubes and grid edges, block sums -> scan of the sums -> per-voxel vertex base; totals on the device
//   gs_tsdf_extract_fill   : vertices and faces, after the caller has read the totals and allocated
// Every scan step is its own launch; no workgroup waits on another.  The triangle table is csrc/gs_mc_table.h (generated).
#include "gs_common.h"
#include "gs_ws.h"
#include "gs_mc_table.h"

#define TS_BX 8
#define TS_BY 8
#define TS_BZ 4
#define TS_BLOCK 256
#define TS_SCAN_THREADS 1024

// ------------------------------------------------------------------------------------------------ integration
struct TsViews {
    GsTsdfView v[GS_TSDF_MAX_VIEWS];
    int n;
};

struct TsGrid {
    int R0, R1, R2;
    float ox, oy, oz, voxel_size;
};

// A workgroup owns the brick of TS_BX x TS_BY x TS_BZ voxels at blockIdx * (TS_BX, TS_BY, TS_BZ), i0 fastest: a wave is one 8 x 8
// slice, every row of it 64 contiguous bytes of the interleaved volume.
static __global__ void __launch_bounds__(TS_BLOCK) tsdf_integrate_kernel(TsGrid G, TsViews V, float sdf_trunc, float alpha_trunc,
                                                                         float depth_trunc, float2* __restrict__ volume)
{
    const int t = threadIdx.x;
    const int b0 = blockIdx.x * TS_BX, b1 = blockIdx.y * TS_BY, b2 = blockIdx.z * TS_BZ;
    const int i0 = b0 + (t & (TS_BX - 1)), i1 = b1 + ((t >> 3) & (TS_BY - 1)), i2 = b2 + (t >> 6);
    const bool live = i0 < G.R0 && i1 < G.R1 && i2 < G.R2;
    const size_t n = (size_t)i0 + (size_t)G.R0 * ((size_t)i1 + (size_t)G.R1 * (size_t)i2);
    const float px = G.ox + ((float)i0 + 0.5f) * G.voxel_size;
    const float py = G.oy + ((float)i1 + 0.5f) * G.voxel_size;
    const float pz = G.oz + ((float)i2 + 0.5f) * G.voxel_size;
    // bounding sphere of the brick's voxel centres (block-uniform): centre of the 8 x 8 x 4 lattice, half diagonal (3.5, 3.5, 1.5)
    const float bcx = G.ox + ((float)b0 + 0.5f * TS_BX) * G.voxel_size;
    const float bcy = G.oy + ((float)b1 + 0.5f * TS_BY) * G.voxel_size;
    const float bcz = G.oz + ((float)b2 + 0.5f * TS_BZ) * G.voxel_size;
    const float brad = 5.2f * G.voxel_size;                          // sqrt(3.5^2 + 3.5^2 + 1.5^2) = 5.17
    float2 cell = make_float2(0.0f, 0.0f);
    if (live) cell = volume[n];
    float tsdf = cell.x, w = cell.y;
    const float inv_trunc = 1.0f / sdf_trunc;
    for (int k = 0; k < V.n; ++k) {
        // camera rows and intrinsics: block-uniform addresses, read once per wave
        const float* __restrict__ M = V.v[k].viewmat;
        const float* __restrict__ Kc = V.v[k].K;
        const float r00 = M[0], r01 = M[1], r02 = M[2], t0 = M[3];
        const float r10 = M[4], r11 = M[5], r12 = M[6], t1 = M[7];
        const float r20 = M[8], r21 = M[9], r22 = M[10], t2 = M[11];
        const float fx = Kc[0], cx = Kc[2], fy = Kc[4], cy = Kc[5];
        const int W = V.v[k].W, H = V.v[k].H;
        {
            // Frustum test of the bounding sphere, conservative: the view is skipped only when every voxel centre of the brick is
            // certain to fail `z > 0` or the pixel range.  Rows of the rotation are unit, so distances carry over to camera space.
            const float sx = r00 * bcx + r01 * bcy + r02 * bcz + t0;
            const float sy = r10 * bcx + r11 * bcy + r12 * bcz + t1;
            const float sz = r20 * bcx + r21 * bcy + r22 * bcz + t2;
            const float rad = 1.05f * brad + 1e-5f * (fabsf(sx) + fabsf(sy) + fabsf(sz));
            bool miss = sz + rad <= 0.0f;
            // side planes through the eye, scaled by the focal length (> 0): fx x + cx z >= 0 is u >= 0, (W - cx) z - fx x >= 0 is
            // u <= W, likewise v.  The approximate square root (1 ulp) is covered by the 5 % on the radius.
            const float wx = (float)W - cx, hy = (float)H - cy;
            miss = miss || (fx * sx + cx * sz) < -rad * __builtin_amdgcn_sqrtf(fx * fx + cx * cx);
            miss = miss || (wx * sz - fx * sx) < -rad * __builtin_amdgcn_sqrtf(fx * fx + wx * wx);
            miss = miss || (fy * sy + cy * sz) < -rad * __builtin_amdgcn_sqrtf(fy * fy + cy * cy);
            miss = miss || (hy * sz - fy * sy) < -rad * __builtin_amdgcn_sqrtf(fy * fy + hy * hy);
            if (miss) continue;                                      // block-uniform
        }
        const float x = r00 * px + r01 * py + r02 * pz + t0;
        const float y = r10 * px + r11 * py + r12 * pz + t1;
        const float z = r20 * px + r21 * py + r22 * pz + t2;
        if (!(live && z > 0.0f)) continue;
        const float iz = __builtin_amdgcn_rcpf(z);                   // 1 ulp: 1e-4 px at |u| = 800, far inside what decides a texel
        const float u = fx * x * iz + cx, v = fy * y * iz + cy;
        if (!(u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H)) continue;          // (a NaN fails)
        int iu = (int)u, iv = (int)v;                                // floor: both are >= 0
        iu = iu < W ? iu : W - 1;                                    // (float)W may round up for W > 2^24: never index outside
        iv = iv < H ? iv : H - 1;
        const float2 da = reinterpret_cast<const float2*>(V.v[k].depth_alpha)[(size_t)iv * (size_t)W + (size_t)iu];
        const float d = da.x;
        if (!(da.y > alpha_trunc)) continue;
        if (!(d > 0.0f && d < depth_trunc)) continue;                // (a NaN depth fails)
        const float sdf = d - z;
        if (!(sdf > -sdf_trunc)) continue;
        const float val = fminf(1.0f, sdf * inv_trunc);
        tsdf = (tsdf * w + val) * __builtin_amdgcn_rcpf(w + 1.0f);
        w += 1.0f;
    }
    if (live) volume[n] = make_float2(tsdf, w);
}

// ------------------------------------------------------------------------------------------------ extraction

// workspace: [ vertex base u32[N] | cube info u16[N] | edge flags u8[N] | block sums / offsets u32[4 * nb] ]
//   cube info  : bits 0..7 the case (bit k: corner k inside), bit 8 valid; 0 for a voxel that is no cube's lower corner
//   edge flags : bit a: the edge from this voxel along axis a carries a vertex
//   block runs : vertices, triangles, valid cubes, surface cubes per 256 voxels; the scan turns them into exclusive offsets
struct TsLayout { unsigned* vbase; unsigned short* info; unsigned char* eflag; unsigned* blocks; size_t total; int nb; };
static inline TsLayout ts_layout(int64_t N, void* base)
{
    GsWs w(base, 16);
    TsLayout L;
    L.nb = gs_cdiv(N, TS_BLOCK);
    L.vbase = w.take<unsigned>((size_t)N);
    L.info = w.take<unsigned short>((size_t)N);
    L.eflag = w.take<unsigned char>((size_t)N);
    L.blocks = w.take<unsigned>((size_t)4 * (size_t)L.nb);
    L.total = w.bytes();
    return L;
}

struct TsDims {
    int R0, R1, R2;
    long long N;
};

__device__ __forceinline__ void ts_coords(const TsDims& D, long long n, int& i0, int& i1, int& i2)
{
    i0 = (int)(n % D.R0);
    const long long r = n / D.R0;
    i1 = (int)(r % D.R1);
    i2 = (int)(r / D.R1);
}

// sum over the 256 threads of a block; every thread calls it
__device__ __forceinline__ unsigned ts_block_sum(unsigned v, unsigned* lds)
{
    const unsigned s = gs_wave_sum_u32(v);
    if (gs_lane_id() == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    const unsigned total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return total;
}

// exclusive prefix of v over the 256 threads of a block; every thread calls it
__device__ __forceinline__ unsigned ts_block_excl(unsigned v, unsigned* lds)
{
    const unsigned incl = gs_wave_incl_scan(v);
    const int w = threadIdx.x >> 6;
    if (gs_lane_id() == 63) lds[w] = incl;
    __syncthreads();
    unsigned r = incl - v;
    for (int k = 0; k < w; ++k) r += lds[k];
    __syncthreads();
    return r;
}

static __global__ void __launch_bounds__(TS_BLOCK) tsdf_cubes_kernel(TsDims D, const float2* __restrict__ volume,
                                                                     unsigned short* __restrict__ info, unsigned* __restrict__ blocks,
                                                                     int nb)
{
    __shared__ unsigned lds[4];
    const long long n = (long long)blockIdx.x * TS_BLOCK + threadIdx.x;
    unsigned ntri = 0u, valid = 0u, surface = 0u;
    if (n < D.N) {
        int i0, i1, i2;
        ts_coords(D, n, i0, i1, i2);
        unsigned word = 0u;
        if (i0 + 1 < D.R0 && i1 + 1 < D.R1 && i2 + 1 < D.R2) {
            unsigned cs = 0u;
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const long long m = n + (k & 1) + (long long)D.R0 * (((k >> 1) & 1) + (long long)D.R1 * ((k >> 2) & 1));
                const float2 c = volume[m];
                ok = ok && (c.y > 0.0f);
                cs |= (c.x < 0.0f ? 1u : 0u) << k;
            }
            if (ok) {
                valid = 1u;
                ntri = GS_MC_NTRI[cs];
                surface = (cs != 0u && cs != 255u) ? 1u : 0u;
                word = cs | 0x100u;
            }
        }
        info[n] = (unsigned short)word;
    }
    const unsigned bt = ts_block_sum(ntri, lds), bv = ts_block_sum(valid, lds), bs = ts_block_sum(surface, lds);
    if (threadIdx.x == 0) {
        blocks[(size_t)nb + blockIdx.x] = bt;
        blocks[2 * (size_t)nb + blockIdx.x] = bv;
        blocks[3 * (size_t)nb + blockIdx.x] = bs;
    }
}

static __global__ void __launch_bounds__(TS_BLOCK) tsdf_edges_kernel(TsDims D, const float2* __restrict__ volume,
                                                                     const unsigned short* __restrict__ info,
                                                                     unsigned char* __restrict__ eflag, unsigned* __restrict__ blocks)
{
    __shared__ unsigned lds[4];
    const long long n = (long long)blockIdx.x * TS_BLOCK + threadIdx.x;
    unsigned flags = 0u;
    if (n < D.N) {
        int i[3];
        ts_coords(D, n, i[0], i[1], i[2]);
        const int R[3] = {D.R0, D.R1, D.R2};
        const long long stride[3] = {1, D.R0, (long long)D.R0 * D.R1};
        const bool in0 = volume[n].x < 0.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (i[a] + 1 >= R[a]) continue;
            const bool in1 = volume[n + stride[a]].x < 0.0f;
            if (in0 == in1) continue;
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            bool any = false;                                        // one of the (up to) four cubes around the edge is valid
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int jb = i[b] - (q & 1), jc = i[c] - (q >> 1);
                if (jb < 0 || jc < 0 || jb + 1 >= R[b] || jc + 1 >= R[c]) continue;
                any = any || ((info[n - (q & 1) * stride[b] - (q >> 1) * stride[c]] & 0x100u) != 0u);
            }
            if (any) flags |= 1u << a;
        }
        eflag[n] = (unsigned char)flags;
    }
    const unsigned bv = ts_block_sum((unsigned)__popc(flags), lds);
    if (threadIdx.x == 0) blocks[blockIdx.x] = bv;
}

// One workgroup turns the four runs of block sums into exclusive offsets (in place, modulo 2^32) and writes the 64-bit totals.
static __global__ void __launch_bounds__(TS_SCAN_THREADS) tsdf_scan_kernel(unsigned* __restrict__ blocks, int nb,
                                                                           long long* __restrict__ counts)
{
    __shared__ unsigned long long sums[TS_SCAN_THREADS];
    const int t = threadIdx.x;
    const int chunk = (nb + TS_SCAN_THREADS - 1) / TS_SCAN_THREADS;
    const long long lo = (long long)t * chunk;
    const long long hi = lo + chunk < nb ? lo + chunk : nb;
    for (int k = 0; k < 4; ++k) {
        unsigned* run = blocks + (size_t)k * nb;
        unsigned long long s = 0ull;
        for (long long j = lo; j < hi; ++j) s += run[j];
        sums[t] = s;
        __syncthreads();
        for (int d = 1; d < TS_SCAN_THREADS; d <<= 1) {              // inclusive scan of the per-thread sums
            const unsigned long long add = t >= d ? sums[t - d] : 0ull;
            __syncthreads();
            sums[t] += add;
            __syncthreads();
        }
        unsigned long long base = sums[t] - s;
        for (long long j = lo; j < hi; ++j) {
            const unsigned c = run[j];
            run[j] = (unsigned)base;
            base += c;
        }
        if (t == TS_SCAN_THREADS - 1) counts[k] = (long long)sums[t];
        __syncthreads();
    }
}

static __global__ void __launch_bounds__(TS_BLOCK) tsdf_vbase_kernel(long long N, const unsigned char* __restrict__ eflag,
                                                                     const unsigned* __restrict__ blocks, unsigned* __restrict__ vbase)
{
    __shared__ unsigned lds[4];
    const long long n = (long long)blockIdx.x * TS_BLOCK + threadIdx.x;
    const unsigned c = n < N ? (unsigned)__popc((unsigned)eflag[n]) : 0u;
    const unsigned r = blocks[blockIdx.x] + ts_block_excl(c, lds);
    if (n < N) vbase[n] = r;
}

struct TsOrigin {
    float o[3], voxel_size;
};

static __global__ void __launch_bounds__(TS_BLOCK) tsdf_vertices_kernel(TsDims D, TsOrigin O, const float2* __restrict__ volume,
                                                                        const unsigned char* __restrict__ eflag,
                                                                        const unsigned* __restrict__ vbase, long long n_vertices,
                                                                        float* __restrict__ vertices)
{
    const long long n = (long long)blockIdx.x * TS_BLOCK + threadIdx.x;
    if (n >= D.N) return;
    const unsigned flags = eflag[n];
    if (flags == 0u) return;
    int i[3];
    ts_coords(D, n, i[0], i[1], i[2]);
    const long long stride[3] = {1, D.R0, (long long)D.R0 * D.R1};
    float p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = O.o[a] + ((float)i[a] + 0.5f) * O.voxel_size;
    const float ta = volume[n].x;
    long long id = vbase[n];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(flags & (1u << a))) continue;
        const float tb = volume[n + stride[a]].x;
        const float s = ta / (ta - tb);
        if (id < n_vertices) {                                       // the totals are the caller's: never write outside what they size
            float* out = vertices + 3 * id;
            out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
            out[a] = p[a] + s * O.voxel_size;
        }
        ++id;
    }
}

static __global__ void __launch_bounds__(TS_BLOCK) tsdf_faces_kernel(TsDims D, const unsigned short* __restrict__ info,
                                                                     const unsigned char* __restrict__ eflag,
                                                                     const unsigned* __restrict__ vbase,
                                                                     const unsigned* __restrict__ blocks, int nb, long long n_triangles,
                                                                     long long* __restrict__ faces)
{
    __shared__ unsigned lds[4];
    const long long n = (long long)blockIdx.x * TS_BLOCK + threadIdx.x;
    unsigned word = 0u;
    if (n < D.N) word = info[n];
    const unsigned cs = word & 0xffu;
    const unsigned ntri = (word & 0x100u) ? (unsigned)GS_MC_NTRI[cs] : 0u;
    long long row = (long long)blocks[(size_t)nb + blockIdx.x] + ts_block_excl(ntri, lds);
    const long long stride1 = D.R0, stride2 = (long long)D.R0 * D.R1;
    for (unsigned k = 0; k < ntri; ++k, ++row) {
        if (row >= n_triangles) break;
        long long tri[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e = GS_MC_TRI[cs][3 * k + j];
            const int lo = GS_MC_EDGE_LO[e], a = e >> 2;
            const long long m = n + (lo & 1) + stride1 * ((lo >> 1) & 1) + stride2 * ((lo >> 2) & 1);    // inside the volume: a cube
            const unsigned f = eflag[m];
            tri[j] = (long long)vbase[m] + __popc(f & ((1u << a) - 1u));
        }
        faces[3 * row + 0] = tri[0];
        faces[3 * row + 1] = tri[1];
        faces[3 * row + 2] = tri[2];
    }
}

static bool ts_dims_ok(int R0, int R1, int R2)
{
    return R0 >= 1 && R1 >= 1 && R2 >= 1 && (int64_t)R0 * R1 * R2 < ((int64_t)1 << 31) && (int64_t)R0 * R1 < ((int64_t)1 << 31);
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" {

int gs_tsdf_integrate(int R0, int R1, int R2, float origin_x, float origin_y, float origin_z, float voxel_size, float sdf_trunc,
                      float alpha_trunc, float depth_trunc, int n_views, const GsTsdfView* views, float* volume, void* stream)
{
    GS_CHECK_ARG(ts_dims_ok(R0, R1, R2), "resolution must be >= 1 per axis with fewer than 2^31 voxels");
    GS_CHECK_ARG(voxel_size > 0.0f && sdf_trunc > 0.0f, "voxel_size and sdf_trunc must be > 0");
    GS_CHECK_ARG(n_views >= 0 && n_views <= GS_TSDF_MAX_VIEWS, "n_views must be in [0, 16]");
    if (n_views == 0) return GS_OK;
    GS_CHECK_ARG(views && volume, "null pointer");
    TsViews V;
    V.n = n_views;
    for (int k = 0; k < GS_TSDF_MAX_VIEWS; ++k) V.v[k] = views[k < n_views ? k : 0];
    for (int k = 0; k < n_views; ++k) {
        GS_CHECK_ARG(views[k].depth_alpha && views[k].viewmat && views[k].K, "null pointer in a view");
        GS_CHECK_ARG(views[k].W >= 1 && views[k].H >= 1 && (int64_t)views[k].W * views[k].H < ((int64_t)1 << 31), "bad image size");
    }
    const int g0 = gs_cdiv(R0, TS_BX), g1 = gs_cdiv(R1, TS_BY), g2 = gs_cdiv(R2, TS_BZ);
    GS_CHECK_ARG(g1 <= 65535 && g2 <= 65535, "resolution too large along axis 1 or 2");
    TsGrid G{R0, R1, R2, origin_x, origin_y, origin_z, voxel_size};
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(g0, g1, g2), dim3(TS_BLOCK), 0, (hipStream_t)stream, G, V, sdf_trunc, alpha_trunc,
                       depth_trunc, (float2*)volume);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

size_t gs_tsdf_extract_ws_bytes(int R0, int R1, int R2)
{
    if (!ts_dims_ok(R0, R1, R2)) return 0;
    return ts_layout((int64_t)R0 * R1 * R2, nullptr).total;
}

int gs_tsdf_extract_count(int R0, int R1, int R2, const float* volume, void* ws, size_t ws_bytes, int64_t* counts, void* stream)
{
    GS_CHECK_ARG(ts_dims_ok(R0, R1, R2), "resolution must be >= 1 per axis with fewer than 2^31 voxels");
    const int64_t N = (int64_t)R0 * R1 * R2;
    const TsLayout L = ts_layout(N, ws);
    if (!ws || ws_bytes < L.total) {
        gs_set_error("%s: workspace too small (%zu < %zu)", __func__, ws ? ws_bytes : (size_t)0, L.total);
        return ws ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(volume && counts, "null pointer");
    TsDims D{R0, R1, R2, (long long)N};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tsdf_cubes_kernel, dim3(L.nb), dim3(TS_BLOCK), 0, s, D, (const float2*)volume, L.info, L.blocks, L.nb);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsdf_edges_kernel, dim3(L.nb), dim3(TS_BLOCK), 0, s, D, (const float2*)volume, L.info, L.eflag, L.blocks);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(TS_SCAN_THREADS), 0, s, L.blocks, L.nb, (long long*)counts);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsdf_vbase_kernel, dim3(L.nb), dim3(TS_BLOCK), 0, s, (long long)N, L.eflag, L.blocks, L.vbase);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_tsdf_extract_fill(int R0, int R1, int R2, float origin_x, float origin_y, float origin_z, float voxel_size, const float* volume,
                         void* ws, size_t ws_bytes, int64_t n_vertices, int64_t n_triangles, float* vertices, int64_t* faces,
                         void* stream)
{
    GS_CHECK_ARG(ts_dims_ok(R0, R1, R2), "resolution must be >= 1 per axis with fewer than 2^31 voxels");
    GS_CHECK_ARG(n_vertices >= 0 && n_triangles >= 0, "totals out of range");
    GS_CHECK_ARG(n_vertices < ((int64_t)1 << 31) && n_triangles < ((int64_t)1 << 31), "more than 2^31 vertices or triangles");
    const int64_t N = (int64_t)R0 * R1 * R2;
    const TsLayout L = ts_layout(N, ws);
    if (!ws || ws_bytes < L.total) {
        gs_set_error("%s: workspace too small (%zu < %zu)", __func__, ws ? ws_bytes : (size_t)0, L.total);
        return ws ? GS_ENOSPC : GS_EINVAL;
    }
    if (n_vertices == 0 && n_triangles == 0) return GS_OK;
    GS_CHECK_ARG(volume, "null pointer");
    GS_CHECK_ARG((n_vertices == 0 || vertices) && (n_triangles == 0 || faces), "null output");
    TsDims D{R0, R1, R2, (long long)N};
    TsOrigin O{{origin_x, origin_y, origin_z}, voxel_size};
    hipStream_t s = (hipStream_t)stream;
    if (n_vertices > 0) {
        hipLaunchKernelGGL(tsdf_vertices_kernel, dim3(L.nb), dim3(TS_BLOCK), 0, s, D, O, (const float2*)volume, L.eflag, L.vbase,
                           (long long)n_vertices, vertices);
        GS_CHECK_LAUNCH();
    }
    if (n_triangles > 0) {
        hipLaunchKernelGGL(tsdf_faces_kernel, dim3(L.nb), dim3(TS_BLOCK), 0, s, D, L.info, L.eflag, L.vbase, L.blocks, L.nb,
                           (long long)n_triangles, (long long*)faces);
        GS_CHECK_LAUNCH();
    }
    return GS_OK;
}

}  // extern "C"
