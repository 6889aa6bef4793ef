// gs_meshraster.hip -- a differentiable triangle-mesh rasterizer for extracted meshes: what the reference gets from nvdiffrast's
// rasterize / interpolate in TriangleMesh.render and TriangleMesh.visible_faces (rfstudio/graphics/_mesh/_triangle_mesh.py:496-555)
// with the NormalShader / DepthShader (antialias = False).  A from-scratch statement of the semantics in include/geosplat_hip.h.
//   gs_meshraster_fwd      : visibility buffer, no tile binning.  fill keys -> pass 1 (one triangle per thread: set up, walk a small
//                            bounding box, 64-bit atomic min of (depth bits << 32 | face) per covered pixel behind a plain-load early-z;
//                            triangles over MR_SMALL_BOX px a side go to a compacted list) -> pass 2 (one wave per listed triangle,
//                            64 lanes striding over its box)
//   gs_meshraster_resolve  : one thread per pixel decodes the winner, recomputes b, one 16-byte store
//   gs_meshraster_bwd      : d(b0, b1, depth) -> d vc with the face ids fixed; fp32 atomics, nine per covered pixel
//   gs_mesh_interp_fwd/bwd : out = sum_i b_i attr[...]; d attr by fp32 atomics, d(b0, b1) per pixel
//   gs_meshclip_fwd/resolve/bwd : the same with near_clip (gs_meshclip_dev.h).  The kernels above are templates on CLIP; without it they
//                            are the code they were.  With it pass 1 also appends the faces that cross the near plane to a second
//                            compacted list, and one more launch (mr_cross_kernel, one wave per listed face) clips each face and
//                            walks its sub-triangles; resolve and backward evaluate a crossing face's values per face (mc_values).
// Every kernel is bounded: no workgroup waits on another.  Coverage is decided in 64-bit integers on 1/256 px coordinates, so a pixel
// on an edge shared by two triangles is covered exactly once (top-left rule) whatever the launch order.
#include "gs_common.h"
#include "gs_ws.h"
#include "gs_meshraster_dev.h"
#include "gs_meshclip_dev.h"

__device__ __forceinline__ void mr_emit(unsigned long long* __restrict__ keys, const MrCam& cam, const MrTri& T, int px, int py,
                                        unsigned fid, unsigned& n_frag, unsigned& n_atomic)
{
    float b0, b1, depth;
    mr_values(T, px, py, b0, b1, depth);
    if (!(depth > 0.0f && depth < 3.0e38f)) return;                                     // (a NaN fails)
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)fid;
    unsigned long long* slot = keys + (size_t)py * (size_t)cam.W + (size_t)px;
    ++n_frag;
    if (*slot <= key) return;                       // early-z on a plain load: a stale value only costs an atomic that changes nothing
    atomicMin(slot, key);
    ++n_atomic;
}

// CLIP (near_clip): the count of crossing faces sits next to the count of large triangles
template <bool CLIP>
static __global__ void __launch_bounds__(MR_BLOCK) mr_fill_kernel(unsigned long long* __restrict__ keys, size_t n_keys,
                                                                  unsigned* __restrict__ n_big)
{
    const size_t i = (size_t)blockIdx.x * MR_BLOCK + threadIdx.x;
    if (i == 0) *n_big = 0u;
    if (CLIP && i == 0) n_big[1] = 0u;
    // two keys per thread: one 16-byte store
    if (2 * i + 1 < n_keys) reinterpret_cast<ulonglong2*>(keys)[i] = make_ulonglong2(MR_EMPTY, MR_EMPTY);
    else if (2 * i < n_keys) keys[2 * i] = MR_EMPTY;
}

// stats (optional, device u64[4]): {fragments pass 1, atomics pass 1, fragments pass 2, atomics pass 2}
__device__ __forceinline__ void mr_commit_stats(unsigned long long* stats, int slot, unsigned n_frag, unsigned n_atomic)
{
    if (stats == nullptr) return;
    if (n_frag) atomicAdd(stats + slot, (unsigned long long)n_frag);
    if (n_atomic) atomicAdd(stats + slot + 1, (unsigned long long)n_atomic);
}

// CLIP: a face that fails mr_load because it crosses the near plane goes to the list `cross` (count n_big[1]) for mr_cross_kernel;
// every other face takes the same code as without CLIP.
template <bool CLIP>
static __global__ void __launch_bounds__(MR_BLOCK) mr_small_kernel(long long V, long long F, const float* __restrict__ vc,
                                                                   const int* __restrict__ faces, MrCam cam, int cull,
                                                                   unsigned long long* __restrict__ keys, unsigned* __restrict__ n_big,
                                                                   unsigned* __restrict__ big, unsigned* __restrict__ cross,
                                                                   unsigned long long* stats)
{
    const long long f = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
    if (f >= F) return;
    MrTri T;
    MrEdges E;
    float P[3][3];
    if (!mr_load(vc, faces, V, f, cam, T, P)) {
        if (CLIP) {
            float Pc[3][3];
            if (mc_crossing(vc, faces, V, f, cam, Pc)) {
                const unsigned slot = atomicAdd(n_big + 1, 1u);
                if (slot < (unsigned long long)F) cross[slot] = (unsigned)f;
            }
        }
        return;
    }
    if (!mr_edges(T, cam, E)) return;
    if (mr_culled(E, cull)) return;
    if (E.x1 < E.x0 || E.y1 < E.y0) return;
    if (E.x1 - E.x0 >= MR_SMALL_BOX || E.y1 - E.y0 >= MR_SMALL_BOX) {
        const unsigned slot = atomicAdd(n_big, 1u);
        if (slot < (unsigned long long)F) big[slot] = (unsigned)f;
        return;
    }
    unsigned n_frag = 0u, n_atomic = 0u;
    long long r0 = E.c[0], r1 = E.c[1], r2 = E.c[2];
    for (int py = E.y0; py <= E.y1; ++py) {
        long long e0 = r0, e1 = r1, e2 = r2;
        for (int px = E.x0; px <= E.x1; ++px) {
            if (((e0 + E.bias[0]) | (e1 + E.bias[1]) | (e2 + E.bias[2])) >= 0) mr_emit(keys, cam, T, px, py, (unsigned)f, n_frag, n_atomic);
            e0 += E.ax[0]; e1 += E.ax[1]; e2 += E.ax[2];
        }
        r0 += E.ay[0]; r1 += E.ay[1]; r2 += E.ay[2];
    }
    mr_commit_stats(stats, 0, n_frag, n_atomic);
}

// One wave per listed triangle (a grid-stride loop over the list: the count stays on the device), lanes stride over the box.
static __global__ void __launch_bounds__(MR_BLOCK) mr_big_kernel(long long V, long long F, const float* __restrict__ vc,
                                                                 const int* __restrict__ faces, MrCam cam,
                                                                 unsigned long long* __restrict__ keys,
                                                                 const unsigned* __restrict__ n_big, const unsigned* __restrict__ big,
                                                                 unsigned long long* stats)
{
    const unsigned total = *n_big;
    const unsigned count = total < (unsigned long long)F ? total : (unsigned)F;
    const unsigned n_waves = gridDim.x * (MR_BLOCK / GS_WAVE);
    const int lane = gs_lane_id();
    unsigned n_frag = 0u, n_atomic = 0u;
    for (unsigned w = blockIdx.x * (MR_BLOCK / GS_WAVE) + (threadIdx.x >> 6); w < count; w += n_waves) {
        const long long f = big[w];
        if (f >= F) continue;
        MrTri T;
        MrEdges E;
        float P[3][3];
        if (!mr_load(vc, faces, V, f, cam, T, P)) continue;      // (cannot fail: pass 1 listed it; wave-uniform either way)
        if (!mr_edges(T, cam, E)) continue;
        if (E.x1 < E.x0 || E.y1 < E.y0) continue;
        const int bw = E.x1 - E.x0 + 1, bh = E.y1 - E.y0 + 1;
        const int n = bw * bh;                                   // <= W H < 2^31
        for (int k = lane; k < n; k += GS_WAVE) {
            const int ry = k / bw, rx = k - ry * bw;
            const long long e0 = E.c[0] + E.ax[0] * rx + E.ay[0] * ry;
            const long long e1 = E.c[1] + E.ax[1] * rx + E.ay[1] * ry;
            const long long e2 = E.c[2] + E.ax[2] * rx + E.ay[2] * ry;
            if (((e0 + E.bias[0]) | (e1 + E.bias[1]) | (e2 + E.bias[2])) >= 0)
                mr_emit(keys, cam, T, E.x0 + rx, E.y0 + ry, (unsigned)f, n_frag, n_atomic);
        }
    }
    mr_commit_stats(stats, 2, n_frag, n_atomic);
}

// near_clip: one wave per crossing face.  Every lane clips the face (the same work in every lane: the polygon stays in registers),
// then the lanes stride over the box of each sub-triangle of the fan, set up by mr_edges like any triangle; the fragment carries the
// FACE's values (mc_values) and the face's id.
static __global__ void __launch_bounds__(MR_BLOCK) mr_cross_kernel(long long V, long long F, const float* __restrict__ vc,
                                                                   const int* __restrict__ faces, MrCam cam, int cull,
                                                                   unsigned long long* __restrict__ keys,
                                                                   const unsigned* __restrict__ n_cross,
                                                                   const unsigned* __restrict__ cross, unsigned long long* stats)
{
    const unsigned total = *n_cross;
    const unsigned count = total < (unsigned long long)F ? total : (unsigned)F;
    const unsigned n_waves = gridDim.x * (MR_BLOCK / GS_WAVE);
    const int lane = gs_lane_id();
    unsigned n_frag = 0u, n_atomic = 0u;
    for (unsigned w = blockIdx.x * (MR_BLOCK / GS_WAVE) + (threadIdx.x >> 6); w < count; w += n_waves) {
        const long long f = cross[w];
        if (f >= F) continue;
        float P[3][3];
        if (!mc_crossing(vc, faces, V, f, cam, P)) continue;     // (cannot fail: pass 1 listed it; wave-uniform either way)
        McPoly Q;
        mc_clip(P, cam, Q);
#pragma unroll 1
        for (int k = 1; k + 1 < Q.n; ++k) {
            MrTri T;
            MrEdges E;
            mc_subtri(Q, k, cam, T);
            if (!mr_edges(T, cam, E)) continue;
            if (mr_culled(E, cull)) continue;
            if (E.x1 < E.x0 || E.y1 < E.y0) continue;
            const int bw = E.x1 - E.x0 + 1, bh = E.y1 - E.y0 + 1;
            const int n = bw * bh;                               // <= W H < 2^31
            for (int i = lane; i < n; i += GS_WAVE) {
                const int ry = i / bw, rx = i - ry * bw;
                const long long e0 = E.c[0] + E.ax[0] * rx + E.ay[0] * ry;
                const long long e1 = E.c[1] + E.ax[1] * rx + E.ay[1] * ry;
                const long long e2 = E.c[2] + E.ax[2] * rx + E.ay[2] * ry;
                if (((e0 + E.bias[0]) | (e1 + E.bias[1]) | (e2 + E.bias[2])) < 0) continue;
                const int px = E.x0 + rx, py = E.y0 + ry;
                float b0, b1, depth;
                mc_values(P, cam, px, py, b0, b1, depth);
                if (!(depth > 0.0f && depth < 3.0e38f)) continue;                       // (a NaN fails)
                const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)f;
                unsigned long long* slot = keys + (size_t)py * (size_t)cam.W + (size_t)px;
                ++n_frag;
                if (*slot <= key) continue;
                atomicMin(slot, key);
                ++n_atomic;
            }
        }
    }
    mr_commit_stats(stats, 2, n_frag, n_atomic);
}

template <bool CLIP>
static __global__ void __launch_bounds__(MR_BLOCK) mr_resolve_kernel(long long V, long long F, const float* __restrict__ vc,
                                                                     const int* __restrict__ faces, MrCam cam,
                                                                     const unsigned long long* __restrict__ keys,
                                                                     float4* __restrict__ rast)
{
    const long long p = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
    if (p >= (long long)cam.H * cam.W) return;
    const unsigned long long key = keys[p];
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const long long f = (long long)(key & 0xffffffffull);
    if (key != MR_EMPTY && f < F) {
        MrTri T;
        float P[3][3];
        if (mr_load(vc, faces, V, f, cam, T, P)) {
            const int py = (int)(p / cam.W), px = (int)(p - (long long)py * cam.W);
            float b0, b1, depth;
            mr_values(T, px, py, b0, b1, depth);
            out = make_float4(b0, b1, __uint_as_float((unsigned)(key >> 32)), (float)(f + 1));      // the depth that won
        } else if (CLIP) {
            float Pc[3][3];
            if (mc_crossing(vc, faces, V, f, cam, Pc)) {
                const int py = (int)(p / cam.W), px = (int)(p - (long long)py * cam.W);
                float b0, b1, depth;
                mc_values(Pc, cam, px, py, b0, b1, depth);
                out = make_float4(b0, b1, __uint_as_float((unsigned)(key >> 32)), (float)(f + 1));
            }
        }
    }
    rast[p] = out;
}

// d(b0, b1, depth) -> d vc at fixed face ids.  With w_i = e_i iz_i, N = sum w, S = sum e:  b_i = w_i / N,  depth = S / N.
// near_clip, a pixel of a crossing face.  (b1, b2, depth)^T = -M P0 with M = (h, e1 x d, e1 x e2)^T / a the inverse of [e1 e2 -d]
// (mc_values).  Moving vertex m by delta moves the solution by -b_m M delta, so with R = ((g1 - g0) h - g0 (e1 x d) + gz n) / a the
// gradient of g0 b0 + g1 b1 + gz depth with respect to vertex m is -b_m R: all three original vertices, the ones behind the plane too.
__device__ __forceinline__ void mr_bwd_crossing(const float (&P)[3][3], const MrCam& cam, int px, int py, const float4& g,
                                                const int* __restrict__ tri, float* __restrict__ d_vc)
{
    McRay R;
    mc_ray(P, cam, px, py, R);
    float b0, b1, depth;
    mc_values(P, cam, px, py, b0, b1, depth);
    const float b[3] = {b0, b1, (1.0f - b0) - b1};
    const float c[3] = {R.e1[1] - R.dy * R.e1[2], R.dx * R.e1[2] - R.e1[0], R.dy * R.e1[0] - R.dx * R.e1[1]};         // e1 x d
    const float n[3] = {R.e1[1] * R.e2[2] - R.e1[2] * R.e2[1], R.e1[2] * R.e2[0] - R.e1[0] * R.e2[2],
                        R.e1[0] * R.e2[1] - R.e1[1] * R.e2[0]};
    const float ra = 1.0f / R.a;
    float Rv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) Rv[k] = ((g.y - g.x) * R.h[k] - g.x * c[k] + g.z * n[k]) * ra;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        float* dst = d_vc + 3 * (size_t)tri[m];
        gs_atomic_add(dst + 0, -b[m] * Rv[0]);
        gs_atomic_add(dst + 1, -b[m] * Rv[1]);
        gs_atomic_add(dst + 2, -b[m] * Rv[2]);
    }
}

template <bool CLIP>
static __global__ void __launch_bounds__(MR_BLOCK) mr_bwd_kernel(long long V, long long F, const float* __restrict__ vc,
                                                                 const int* __restrict__ faces, MrCam cam,
                                                                 const float4* __restrict__ rast, const float4* __restrict__ d_rast,
                                                                 float* __restrict__ d_vc)
{
    const long long p = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
    if (p >= (long long)cam.H * cam.W) return;
    const float4 r = rast[p];
    if (!(r.w >= 1.0f && r.w <= 16777216.0f)) return;
    const long long f = (long long)r.w - 1;
    if (f >= F) return;
    const float4 g = d_rast[p];
    if (g.x == 0.0f && g.y == 0.0f && g.z == 0.0f) return;
    MrTri T;
    float P[3][3];
    const int py = (int)(p / cam.W), px = (int)(p - (long long)py * cam.W);
    if (!mr_load(vc, faces, V, f, cam, T, P)) {
        if (CLIP) {
            float Pc[3][3];
            if (mc_crossing(vc, faces, V, f, cam, Pc)) mr_bwd_crossing(Pc, cam, px, py, g, faces + 3 * f, d_vc);
        }
        return;
    }
    const float pcx = (float)px + 0.5f, pcy = (float)py + 0.5f;
    float qx[3], qy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { qx[k] = T.xs[k] - pcx; qy[k] = T.ys[k] - pcy; }
    float e[3];
    e[0] = qx[1] * qy[2] - qy[1] * qx[2];
    e[1] = qx[2] * qy[0] - qy[2] * qx[0];
    e[2] = qx[0] * qy[1] - qy[0] * qx[1];
    const float S = (e[0] + e[1]) + e[2];
    const float N = (e[0] * T.iz[0] + e[1] * T.iz[1]) + e[2] * T.iz[2];
    const float rN = 1.0f / N;
    const float b0 = e[0] * T.iz[0] * rN, b1 = e[1] * T.iz[1] * rN, depth = S * rN;
    const float gN = -(g.x * b0 + g.y * b1 + g.z * depth) * rN;
    const float gb[3] = {g.x, g.y, 0.0f};
    float ge[3], giz[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ge[k] = (gb[k] * T.iz[k] + g.z) * rN + gN * T.iz[k];
        giz[k] = (gb[k] * rN + gN) * e[k];
    }
    // e_i = q_a x q_b with a = i + 1, b = i + 2:  d q_a = ge_i (q_b.y, -q_b.x),  d q_b = ge_i (-q_a.y, q_a.x)
    float gx[3] = {0.0f, 0.0f, 0.0f}, gy[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        gx[a] += ge[i] * qy[b];
        gy[a] -= ge[i] * qx[b];
        gx[b] -= ge[i] * qy[a];
        gy[b] += ge[i] * qx[a];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // xs = fx X / Z + cx, ys = fy Y / Z + cy, iz = 1 / Z
        const float iz = T.iz[k];
        const float dX = gx[k] * cam.fx * iz, dY = gy[k] * cam.fy * iz;
        const float dZ = -(dX * P[k][0] + dY * P[k][1] + giz[k] * iz) * iz;
        float* dst = d_vc + 3 * (size_t)faces[3 * f + k];                              // (mr_load checked the index)
        gs_atomic_add(dst + 0, dX);
        gs_atomic_add(dst + 1, dY);
        gs_atomic_add(dst + 2, dZ);
    }
}

// ------------------------------------------------------------------------------------------------ interpolate
// rows of the three attribute vectors of face f: per-vertex attributes go through the face's vertex indices, per-face-vertex
// attributes [F,3,C] are rows 3 f + i.  false: the pixel is empty or names something outside the tables.
__device__ __forceinline__ bool mi_rows(const float4& r, long long F, long long V, int per_face_vertex, const int* __restrict__ faces,
                                        long long (&row)[3])
{
    if (!(r.w >= 1.0f && r.w <= 16777216.0f)) return false;
    const long long f = (long long)r.w - 1;
    if (f >= F) return false;
    if (per_face_vertex) {
        row[0] = 3 * f; row[1] = 3 * f + 1; row[2] = 3 * f + 2;
        return true;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        row[k] = faces[3 * f + k];
        if (row[k] < 0 || row[k] >= V) return false;
    }
    return true;
}

static __global__ void __launch_bounds__(MR_BLOCK) mi_fwd_kernel(long long P, int C, long long F, long long V, int per_face_vertex,
                                                                 const float4* __restrict__ rast, const int* __restrict__ faces,
                                                                 const float* __restrict__ attr, float* __restrict__ out)
{
    const long long p = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
    if (p >= P) return;
    const float4 r = rast[p];
    long long row[3];
    float* o = out + (size_t)p * C;
    if (!mi_rows(r, F, V, per_face_vertex, faces, row)) {
        for (int c = 0; c < C; ++c) o[c] = 0.0f;
        return;
    }
    const float b0 = r.x, b1 = r.y, b2 = 1.0f - r.x - r.y;
    const float* a0 = attr + (size_t)row[0] * C;
    const float* a1 = attr + (size_t)row[1] * C;
    const float* a2 = attr + (size_t)row[2] * C;
    for (int c = 0; c < C; ++c) o[c] = b0 * a0[c] + b1 * a1[c] + b2 * a2[c];
}

static __global__ void __launch_bounds__(MR_BLOCK) mi_bwd_kernel(long long P, int C, long long F, long long V, int per_face_vertex,
                                                                 const float4* __restrict__ rast, const int* __restrict__ faces,
                                                                 const float* __restrict__ attr, const float* __restrict__ d_out,
                                                                 float* __restrict__ d_attr, float4* __restrict__ d_rast)
{
    const long long p = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
    if (p >= P) return;
    const float4 r = rast[p];
    long long row[3];
    float db0 = 0.0f, db1 = 0.0f;
    if (mi_rows(r, F, V, per_face_vertex, faces, row)) {
        const float b0 = r.x, b1 = r.y, b2 = 1.0f - r.x - r.y;
        const float* g = d_out + (size_t)p * C;
        const float* a0 = attr + (size_t)row[0] * C;
        const float* a1 = attr + (size_t)row[1] * C;
        const float* a2 = attr + (size_t)row[2] * C;
        float* d0 = d_attr + (size_t)row[0] * C;
        float* d1 = d_attr + (size_t)row[1] * C;
        float* d2 = d_attr + (size_t)row[2] * C;
        for (int c = 0; c < C; ++c) {
            const float gc = g[c];
            if (gc == 0.0f) continue;
            const float t2 = a2[c];
            db0 += gc * (a0[c] - t2);
            db1 += gc * (a1[c] - t2);
            gs_atomic_add(d0 + c, gc * b0);
            gs_atomic_add(d1 + c, gc * b1);
            gs_atomic_add(d2 + c, gc * b2);
        }
    }
    if (d_rast) d_rast[p] = make_float4(db0, db1, 0.0f, 0.0f);
}

// ------------------------------------------------------------------------------------------------ entry points
// workspace: [ keys u64[H W] | big-triangle count u32, crossing-face count u32 (16 bytes) | big-triangle list u32[F] ]
// and, with near_clip (gs_meshclip_*), [ ... | crossing-face list u32[F] ]
struct MrLayout { unsigned long long* keys; unsigned *n_big, *big, *cross; size_t total; };
static inline MrLayout mr_layout(const void* base, int64_t F, int H, int W, bool clip = false)
{
    GsWs w((void*)base, 16);
    MrLayout L;
    L.keys = w.take<unsigned long long>((size_t)H * (size_t)W);
    L.n_big = w.take<unsigned>(4);
    L.big = w.take<unsigned>((size_t)(F > 0 ? F : 1));
    L.cross = clip ? w.take<unsigned>((size_t)(F > 0 ? F : 1)) : nullptr;
    L.total = w.bytes();
    return L;
}
static bool mr_dims_ok(int64_t V, int64_t F, int H, int W)
{
    return V >= 0 && F >= 0 && V < ((int64_t)1 << 31) && F <= ((int64_t)1 << 24) && H >= 1 && W >= 1 &&
           (int64_t)H * W < ((int64_t)1 << 31);
}
static bool mr_cam_ok(float fx, float fy, float near) { return fx > 0.0f && fy > 0.0f && near > 0.0f; }

extern "C" {

size_t gs_meshraster_ws_bytes(int64_t F, int H, int W)
{
    if (!mr_dims_ok(0, F, H, W)) return 0;
    return mr_layout(nullptr, F, H, W).total;
}

int gs_meshraster_fwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                      float near, int cull, void* ws, size_t ws_bytes, uint64_t* stats, void* stream)
{
    GS_CHECK_ARG(mr_dims_ok(V, F, H, W), "need V < 2^31, F <= 2^24, H, W >= 1 and H W < 2^31");
    GS_CHECK_ARG(mr_cam_ok(fx, fy, near), "fx, fy and near must be > 0");
    GS_CHECK_ARG(cull == 0 || cull == 1, "cull must be 0 (none) or 1 (back)");
    const MrLayout L = mr_layout(ws, F, H, W);
    if (!ws || ws_bytes < L.total) {
        gs_set_error("%s: workspace too small (%zu < %zu)", __func__, ws ? ws_bytes : (size_t)0, L.total);
        return ws ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(F == 0 || (vc && faces), "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const size_t n_keys = (size_t)H * (size_t)W;
    hipLaunchKernelGGL(mr_fill_kernel<false>, dim3(gs_cdiv((int64_t)((n_keys + 1) / 2), MR_BLOCK)), dim3(MR_BLOCK), 0, s, L.keys, n_keys,
                       L.n_big);
    GS_CHECK_LAUNCH();
    if (F == 0) return GS_OK;
    MrCam cam{fx, fy, cx, cy, near, H, W};
    hipLaunchKernelGGL(mr_small_kernel<false>, dim3(gs_cdiv(F, MR_BLOCK)), dim3(MR_BLOCK), 0, s, (long long)V, (long long)F, vc, faces, cam,
                       cull, L.keys, L.n_big, L.big, (unsigned*)nullptr, (unsigned long long*)stats);
    GS_CHECK_LAUNCH();
    const int want = gs_cdiv(F, MR_BLOCK / GS_WAVE);
    hipLaunchKernelGGL(mr_big_kernel, dim3(want < MR_MAX_BIG_BLOCKS ? want : MR_MAX_BIG_BLOCKS), dim3(MR_BLOCK), 0, s, (long long)V,
                       (long long)F, vc, faces, cam, L.keys, L.n_big, L.big, (unsigned long long*)stats);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_meshraster_resolve(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H,
                          int W, float near, const void* ws, size_t ws_bytes, float* rast, void* stream)
{
    GS_CHECK_ARG(mr_dims_ok(V, F, H, W), "need V < 2^31, F <= 2^24, H, W >= 1 and H W < 2^31");
    GS_CHECK_ARG(mr_cam_ok(fx, fy, near), "fx, fy and near must be > 0");
    const MrLayout L = mr_layout(ws, F, H, W);
    if (!ws || ws_bytes < L.total) {
        gs_set_error("%s: workspace too small (%zu < %zu)", __func__, ws ? ws_bytes : (size_t)0, L.total);
        return ws ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(rast && (F == 0 || (vc && faces)), "null pointer");
    MrCam cam{fx, fy, cx, cy, near, H, W};
    hipLaunchKernelGGL(mr_resolve_kernel<false>, dim3(gs_cdiv((int64_t)H * W, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream,
                       (long long)V, (long long)F, vc, faces, cam, L.keys, (float4*)rast);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_meshraster_bwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                      float near, const float* rast, const float* d_rast, float* d_vc, void* stream)
{
    GS_CHECK_ARG(mr_dims_ok(V, F, H, W), "need V < 2^31, F <= 2^24, H, W >= 1 and H W < 2^31");
    GS_CHECK_ARG(mr_cam_ok(fx, fy, near), "fx, fy and near must be > 0");
    if (V == 0) return GS_OK;
    GS_CHECK_ARG(d_vc, "null pointer");
    GS_CHECK_HIP(gs_zero_async(d_vc, (size_t)V * 12, (hipStream_t)stream));
    if (F == 0) return GS_OK;
    GS_CHECK_ARG(vc && faces && rast && d_rast, "null pointer");
    MrCam cam{fx, fy, cx, cy, near, H, W};
    hipLaunchKernelGGL(mr_bwd_kernel<false>, dim3(gs_cdiv((int64_t)H * W, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, (long long)V,
                       (long long)F, vc, faces, cam, (const float4*)rast, (const float4*)d_rast, d_vc);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// ---- near_clip: the same three steps with crossing faces clipped (gs_meshclip_dev.h); every other face takes the code above
size_t gs_meshclip_ws_bytes(int64_t F, int H, int W)
{
    if (!mr_dims_ok(0, F, H, W)) return 0;
    return mr_layout(nullptr, F, H, W, true).total;
}

int gs_meshclip_fwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                    float near, int cull, void* ws, size_t ws_bytes, uint64_t* stats, void* stream)
{
    GS_CHECK_ARG(mr_dims_ok(V, F, H, W), "need V < 2^31, F <= 2^24, H, W >= 1 and H W < 2^31");
    GS_CHECK_ARG(mr_cam_ok(fx, fy, near), "fx, fy and near must be > 0");
    GS_CHECK_ARG(cull == 0 || cull == 1, "cull must be 0 (none) or 1 (back)");
    const MrLayout L = mr_layout(ws, F, H, W, true);
    if (!ws || ws_bytes < L.total) {
        gs_set_error("%s: workspace too small (%zu < %zu)", __func__, ws ? ws_bytes : (size_t)0, L.total);
        return ws ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(F == 0 || (vc && faces), "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const size_t n_keys = (size_t)H * (size_t)W;
    hipLaunchKernelGGL(mr_fill_kernel<true>, dim3(gs_cdiv((int64_t)((n_keys + 1) / 2), MR_BLOCK)), dim3(MR_BLOCK), 0, s, L.keys, n_keys,
                       L.n_big);
    GS_CHECK_LAUNCH();
    if (F == 0) return GS_OK;
    MrCam cam{fx, fy, cx, cy, near, H, W};
    hipLaunchKernelGGL(mr_small_kernel<true>, dim3(gs_cdiv(F, MR_BLOCK)), dim3(MR_BLOCK), 0, s, (long long)V, (long long)F, vc, faces, cam,
                       cull, L.keys, L.n_big, L.big, L.cross, (unsigned long long*)stats);
    GS_CHECK_LAUNCH();
    const int want = gs_cdiv(F, MR_BLOCK / GS_WAVE);
    const int blocks = want < MR_MAX_BIG_BLOCKS ? want : MR_MAX_BIG_BLOCKS;
    hipLaunchKernelGGL(mr_big_kernel, dim3(blocks), dim3(MR_BLOCK), 0, s, (long long)V, (long long)F, vc, faces, cam, L.keys, L.n_big, L.big,
                       (unsigned long long*)stats);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(mr_cross_kernel, dim3(blocks), dim3(MR_BLOCK), 0, s, (long long)V, (long long)F, vc, faces, cam, cull, L.keys,
                       L.n_big + 1, L.cross, (unsigned long long*)stats);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_meshclip_resolve(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H,
                        int W, float near, const void* ws, size_t ws_bytes, float* rast, void* stream)
{
    GS_CHECK_ARG(mr_dims_ok(V, F, H, W), "need V < 2^31, F <= 2^24, H, W >= 1 and H W < 2^31");
    GS_CHECK_ARG(mr_cam_ok(fx, fy, near), "fx, fy and near must be > 0");
    const MrLayout L = mr_layout(ws, F, H, W, true);
    if (!ws || ws_bytes < L.total) {
        gs_set_error("%s: workspace too small (%zu < %zu)", __func__, ws ? ws_bytes : (size_t)0, L.total);
        return ws ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(rast && (F == 0 || (vc && faces)), "null pointer");
    MrCam cam{fx, fy, cx, cy, near, H, W};
    hipLaunchKernelGGL(mr_resolve_kernel<true>, dim3(gs_cdiv((int64_t)H * W, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream,
                       (long long)V, (long long)F, vc, faces, cam, L.keys, (float4*)rast);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_meshclip_bwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                    float near, const float* rast, const float* d_rast, float* d_vc, void* stream)
{
    GS_CHECK_ARG(mr_dims_ok(V, F, H, W), "need V < 2^31, F <= 2^24, H, W >= 1 and H W < 2^31");
    GS_CHECK_ARG(mr_cam_ok(fx, fy, near), "fx, fy and near must be > 0");
    if (V == 0) return GS_OK;
    GS_CHECK_ARG(d_vc, "null pointer");
    GS_CHECK_HIP(gs_zero_async(d_vc, (size_t)V * 12, (hipStream_t)stream));
    if (F == 0) return GS_OK;
    GS_CHECK_ARG(vc && faces && rast && d_rast, "null pointer");
    MrCam cam{fx, fy, cx, cy, near, H, W};
    hipLaunchKernelGGL(mr_bwd_kernel<true>, dim3(gs_cdiv((int64_t)H * W, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, (long long)V,
                       (long long)F, vc, faces, cam, (const float4*)rast, (const float4*)d_rast, d_vc);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

static bool mi_args_ok(int64_t P, int C, int64_t F, int64_t V, int per_face_vertex)
{
    return P >= 0 && P < ((int64_t)1 << 31) && C >= 1 && C <= 4096 && F >= 0 && F <= ((int64_t)1 << 24) && V >= 0 &&
           V < ((int64_t)1 << 31) && (per_face_vertex == 0 || per_face_vertex == 1);
}

int gs_mesh_interp_fwd(int64_t P, int C, int64_t F, int64_t V, int per_face_vertex, const float* rast, const int32_t* faces,
                       const float* attr, float* out, void* stream)
{
    GS_CHECK_ARG(mi_args_ok(P, C, F, V, per_face_vertex), "need P < 2^31, 1 <= C <= 4096, F <= 2^24, V < 2^31, per_face_vertex 0 or 1");
    if (P == 0) return GS_OK;
    GS_CHECK_ARG(rast && out && (F == 0 || (faces && attr)), "null pointer");
    hipLaunchKernelGGL(mi_fwd_kernel, dim3(gs_cdiv(P, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, (long long)P, C, (long long)F,
                       (long long)V, per_face_vertex, (const float4*)rast, faces, attr, out);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_mesh_interp_bwd(int64_t P, int C, int64_t F, int64_t V, int per_face_vertex, const float* rast, const int32_t* faces,
                       const float* attr, const float* d_out, float* d_attr, float* d_rast, void* stream)
{
    GS_CHECK_ARG(mi_args_ok(P, C, F, V, per_face_vertex), "need P < 2^31, 1 <= C <= 4096, F <= 2^24, V < 2^31, per_face_vertex 0 or 1");
    const int64_t rows = per_face_vertex ? 3 * F : V;
    if (rows > 0) {
        GS_CHECK_ARG(d_attr, "null pointer");
        GS_CHECK_HIP(gs_zero_async(d_attr, (size_t)rows * (size_t)C * 4, (hipStream_t)stream));
    }
    if (P == 0) return GS_OK;
    GS_CHECK_ARG(rast && d_out && (F == 0 || (faces && attr)), "null pointer");
    hipLaunchKernelGGL(mi_bwd_kernel, dim3(gs_cdiv(P, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, (long long)P, C, (long long)F,
                       (long long)V, per_face_vertex, (const float4*)rast, faces, attr, d_out, d_attr, (float4*)d_rast);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

}  // extern "C"
