// gs_meshaa.hip -- silhouette antialiasing for the mesh rasterizer (gs_meshraster.hip): what the reference gets from nvdiffrast's
// `antialias` at the end of TriangleMesh.render (rfstudio/graphics/_mesh/_triangle_mesh.py:552-553).  A from-scratch statement of the
// semantics in include/geosplat_hip.h; faces are loaded, snapped and culled through gs_meshraster_dev.h, the rasterizer's own code.
//   gs_mesh_topology_build : for every half-edge (f, i) the other faces on its undirected edge.  A bounded open-addressing table of
//                            the 64-bit (min v, max v) keys; every slot heads a linked list of its half-edges.  Two launches, no waiting:
//                            a failed compare-and-swap moves on to the next slot, at most `slots` times.
//   gs_meshaa_fwd          : a gather, one thread per output pixel.  A pixel whose four neighbours carry its own face id copies its
//                            colour; another analyses its (at most four) pairs and writes `out` once.  No atomics.
//   gs_meshaa_bwd          : the same shape.  d color is gathered; the pixel that comes first in a pair issues its six vertex atomics.
//   gs_meshclip_aa_fwd/bwd : the same kernels with CLIP (near_clip): a face that crosses the near plane counts as a neighbour in the
//                            silhouette test (aa_crossing_side); as a foreground face it blends nothing.
// Every decision (foreground, exit edge, silhouette) is made in integers on the snapped positions, so it does not depend on launch
// order or on rounding; only the weight is fp32, from the unsnapped positions (the convention of mr_values).
#include "gs_meshraster_dev.h"
#include "gs_meshclip_dev.h"
#include "gs_ws.h"

#define AA_EMPTY 0xffffffffffffffffull

// ------------------------------------------------------------------------------------------------ edge topology
// [ keys u64[slots] | head i32[slots] | slot i32[3F] | next i32[3F] ],  slots = a power of two >= 6 F: at most half full
struct AaLayout {
    size_t slots, off_head, off_slot, off_next, total;
};
static inline AaLayout aa_layout(int64_t F)
{
    AaLayout L;
    L.slots = 16;
    while (L.slots < (size_t)(6 * F)) L.slots *= 2;
    L.off_head = L.slots * 8;
    L.off_slot = L.off_head + L.slots * 4;
    L.off_next = L.off_slot + (size_t)(3 * F) * 4;
    L.total = gs_align_up(L.off_next + (size_t)(3 * F) * 4, 16);
    return L;
}

struct AaTopo {
    const int* head;
    const int* slot;
    const int* next;
    long long slots, n_half;
};

static __global__ void __launch_bounds__(MR_BLOCK) aa_topo_fill_kernel(unsigned long long* __restrict__ keys, int* __restrict__ head,
                                                                       long long slots)
{
    const long long i = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
    if (i >= slots) return;
    keys[i] = AA_EMPTY;
    head[i] = -1;
}

static __global__ void __launch_bounds__(MR_BLOCK) aa_topo_insert_kernel(long long F, const int* __restrict__ faces,
                                                                         unsigned long long* __restrict__ keys, int* __restrict__ head,
                                                                         int* __restrict__ slot, int* __restrict__ next, long long slots)
{
    const long long h = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
    if (h >= 3 * F) return;
    const long long f = h / 3;
    const int i = (int)(h - 3 * f);
    // edge i runs between vertices i + 1 and i + 2.  The indices are labels here: nothing is read through them.
    const unsigned a = (unsigned)faces[3 * f + (i + 1) % 3], b = (unsigned)faces[3 * f + (i + 2) % 3];
    int found = -1;
    if (a != b) {                                                                         // (so a key is never AA_EMPTY)
        const unsigned long long key = ((unsigned long long)min(a, b) << 32) | (unsigned long long)max(a, b);
        unsigned long long x = key;                                                       // splitmix64 finaliser
        x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
        x ^= x >> 27; x *= 0x94d049bb133111ebull;
        x ^= x >> 31;
        long long s = (long long)(x & (unsigned long long)(slots - 1));
        for (long long n = 0; n < slots; ++n) {
            const unsigned long long prev = atomicCAS(keys + s, AA_EMPTY, key);
            if (prev == AA_EMPTY || prev == key) { found = (int)s; break; }
            s = (s + 1) & (slots - 1);
        }
    }
    slot[h] = found;
    next[h] = found >= 0 ? atomicExch(head + found, (int)h) : -1;
}

// ------------------------------------------------------------------------------------------------ a pair of pixels
struct AaCtx {
    long long V, F;
    const float* vc;
    const int* faces;
    MrCam cam;
    int cull;
    const float4* rast;
    AaTopo topo;
};

// what a blended pair does: `target` receives w (colour[other] - colour[target])
struct AaPair {
    long long target, other;            // pixel indices; target < 0: the weight is zero (d = 0.5), nothing to add
    float w;
    int code;                           // the decisions, for the debug output: 1 + exit edge + 4 (0 none, 1 first, 2 second pixel
                                        // receives) + 16 (the foreground pixel is the second)
    // backward: d w / d (camera-space position of the exit edge's two vertices), zero where d is clamped
    long long vert[2];
    float gX[2], gY[2], gZ[2];
};

__device__ __forceinline__ long long aa_face(float w, long long F)
{
    if (!(w >= 1.0f && w <= 16777216.0f)) return -1;
    const long long f = (long long)w - 1;
    return f < F ? f : -1;
}

__device__ __forceinline__ int aa_pick(const int (&A)[3], int k) { return k == 0 ? A[0] : (k == 1 ? A[1] : A[2]); }
__device__ __forceinline__ float aa_pick(const float (&A)[3], int k) { return k == 0 ? A[0] : (k == 1 ? A[1] : A[2]); }
__device__ __forceinline__ long long aa_pick(const long long (&A)[3], int k) { return k == 0 ? A[0] : (k == 1 ? A[1] : A[2]); }

// near_clip: does the crossing face f2 (gs_meshclip_dev.h) count as a neighbour on its half-edge i2, and on which side of the line
// through (x1, y1) with direction (dx, dy) does it lie?  It counts when at least one sub-triangle of its clipped polygon survives
// mr_edges and the cull, as in mr_cross_kernel.  The side is decided on the snapped position of the polygon vertex that follows the
// edge's second endpoint (f2's vertex i2 + 2): f2's opposite vertex when that is inside, else the cut towards it; every vertex of the
// polygon off the edge lies on that side in exact arithmetic.  false: not a neighbour (also when the guard band removed the endpoint).
__device__ __forceinline__ bool aa_crossing_side(const float* __restrict__ vc, const int* __restrict__ faces, long long V, long long f2,
                                                 int i2, const MrCam& cam, int cull, long long x1, long long y1, long long dx,
                                                 long long dy, long long& side2)
{
    float Pc[3][3];
    if (!mc_crossing(vc, faces, V, f2, cam, Pc)) return false;
    McPoly Q;
    mc_clip(Pc, cam, Q);
    bool kept = false;
#pragma unroll 1
    for (int k = 1; k + 1 < Q.n; ++k) {
        MrTri T;
        MrEdges E;
        mc_subtri(Q, k, cam, T);
        if (mr_edges(T, cam, E) && !mr_culled(E, cull)) kept = true;
    }
    if (!kept) return false;
    const int want = (i2 + 2) % 3;
    int m = -1;
#pragma unroll
    for (int j = 0; j < MC_MAX_VERTS; ++j)
        if (j < Q.n && Q.tag[j] == want) m = j;
    if (m < 0) return false;
    float x, y, z;
    mc_get(Q, m + 1 < Q.n ? m + 1 : 0, x, y, z);
    MrTri T;
    mc_project(x, y, z, cam, T, 0);
    const float sx = T.xs[0] * (float)MR_SNAP, sy = T.ys[0] * (float)MR_SNAP;
    if (!(fabsf(sx) <= MR_RANGE && fabsf(sy) <= MR_RANGE)) return false;
    side2 = dx * ((long long)__builtin_rintf(sy) - y1) - dy * ((long long)__builtin_rintf(sx) - x1);
    return true;
}

// The pair (p, q), q = p + (1, 0) (horizontal) or p + (0, 1), whose face-id channels differ.  false: the pair blends nothing.
// CLIP (near_clip): crossing faces count as neighbours (aa_crossing_side); a crossing foreground face fails mr_load and blends nothing.
template <bool CLIP>
__device__ __forceinline__ bool aa_pair(const AaCtx& K, long long p, long long q, int horizontal, AaPair& R)
{
    const float4 rp = K.rast[p], rq = K.rast[q];
    const long long fp = aa_face(rp.w, K.F), fq = aa_face(rq.w, K.F);
    if (fp < 0 && fq < 0) return false;
    // foreground: the pixel with a face and the smaller depth; the lower face id on equal depth
    bool first;
    if (fq < 0) first = true;
    else if (fp < 0) first = false;
    else if (rp.z < rq.z) first = true;
    else if (rq.z < rp.z) first = false;
    else first = fp < fq;
    const long long a = first ? p : q, b = first ? q : p, f = first ? fp : fq;
    const int ay = (int)(a / K.cam.W), ax = (int)(a - (long long)ay * K.cam.W);
    const int by = (int)(b / K.cam.W), bx = (int)(b - (long long)by * K.cam.W);

    MrTri T;
    MrEdges E;
    float P[3][3];
    int X[3], Y[3];
    if (!mr_load(K.vc, K.faces, K.V, f, K.cam, T, P)) return false;
    if (!mr_edges(T, K.cam, E, X, Y)) return false;
    if (mr_culled(E, K.cull)) return false;
    if (E.x1 < E.x0 || E.y1 < E.y0) return false;                                        // (the edge functions are not set up)

    // the exit edge: among the edges with a inside and b outside, the smallest Ea / (Ea - Eb), compared exactly; ties to the lower i
    int edge = -1;
    long long best_n = 0, best_d = 1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const long long ea = E.c[i] + E.ax[i] * (long long)(ax - E.x0) + E.ay[i] * (long long)(ay - E.y0);
        const long long eb = E.c[i] + E.ax[i] * (long long)(bx - E.x0) + E.ay[i] * (long long)(by - E.y0);
        if (!(ea + E.bias[i] >= 0 && eb + E.bias[i] < 0)) continue;
        const long long den = ea - eb;                                                   // > 0
        if (edge < 0 || (__int128)ea * (__int128)best_d < (__int128)best_n * (__int128)den) {
            edge = i; best_n = ea; best_d = den;
        }
    }
    if (edge < 0) return false;
    const int e1 = (edge + 1) % 3, e2 = (edge + 2) % 3;

    // silhouette: no other face that the rasterizer would keep has its opposite vertex strictly on the far side of the edge's line
    const long long x1 = aa_pick(X, e1), y1 = aa_pick(Y, e1);
    const long long dx = aa_pick(X, e2) - x1, dy = aa_pick(Y, e2) - y1;
    const long long side = dx * (aa_pick(Y, edge) - y1) - dy * (aa_pick(X, edge) - x1);  // +- the snapped area: never zero
    const long long h = 3 * f + edge;
    const int s = K.topo.slot[h];
    if (s >= 0 && s < K.topo.slots) {
        long long n = 0;
        for (int h2 = K.topo.head[s]; h2 >= 0 && h2 < K.topo.n_half && n < K.topo.n_half; h2 = K.topo.next[h2], ++n) {
            const long long f2 = h2 / 3;
            if (f2 == f) continue;
            const int i2 = h2 - 3 * (int)f2;
            MrTri T2;
            MrEdges E2;
            float P2[3][3];
            int X2[3], Y2[3];
            if (!mr_load(K.vc, K.faces, K.V, f2, K.cam, T2, P2)) {
                if (CLIP) {
                    long long side2;
                    if (aa_crossing_side(K.vc, K.faces, K.V, f2, i2, K.cam, K.cull, x1, y1, dx, dy, side2) &&
                        ((side > 0 && side2 < 0) || (side < 0 && side2 > 0))) return false;
                }
                continue;
            }
            if (!mr_edges(T2, K.cam, E2, X2, Y2)) continue;
            if (mr_culled(E2, K.cull)) continue;
            const long long side2 = dx * (aa_pick(Y2, i2) - y1) - dy * (aa_pick(X2, i2) - x1);
            if ((side > 0 && side2 < 0) || (side < 0 && side2 > 0)) return false;
        }
    }

    // the weight, from the unsnapped positions relative to a's centre: where the edge's line meets the pair's axis
    const float pcx = (float)ax + 0.5f, pcy = (float)ay + 0.5f;
    const float q1x = aa_pick(T.xs, e1) - pcx, q1y = aa_pick(T.ys, e1) - pcy;
    const float q2x = aa_pick(T.xs, e2) - pcx, q2y = aa_pick(T.ys, e2) - pcy;
    const float u1 = horizontal ? q1x : q1y, v1 = horizontal ? q1y : q1x;
    const float u2 = horizontal ? q2x : q2y, v2 = horizontal ? q2y : q2x;
    const float D = v2 - v1;
    const float xstar = (u1 * v2 - v1 * u2) / D;                                          // correctly rounded: 0.5 stays 0.5
    const float rD = 1.0f / D;
    const float sgn = first ? 1.0f : -1.0f;                                               // from a to b
    const float sd = sgn * xstar;
    R.code = 1 + edge + (first ? 0 : 16);
    R.target = -1;
    R.other = -1;
    R.w = 0.0f;
    R.vert[0] = R.vert[1] = 0;
    R.gX[0] = R.gX[1] = R.gY[0] = R.gY[1] = R.gZ[0] = R.gZ[1] = 0.0f;
    if (!(sd == sd)) return true;                                                         // 0 / 0: an edge along the axis, no weight
    const float d = fminf(fmaxf(sd, 0.0f), 1.0f);
    float dw_dd;
    if (d > 0.5f) { R.target = b; R.other = a; R.w = d - 0.5f; dw_dd = 1.0f; R.code += first ? 8 : 4; }
    else if (d < 0.5f) { R.target = a; R.other = b; R.w = 0.5f - d; dw_dd = -1.0f; R.code += first ? 4 : 8; }
    else return true;
    if (sd >= 0.0f && sd <= 1.0f) {
        const float g = dw_dd * sgn * rD;
        const float gu1 = g * v2, gu2 = -g * v1, gv1 = g * (xstar - u2), gv2 = g * (u1 - xstar);
        const float gx[2] = {horizontal ? gu1 : gv1, horizontal ? gu2 : gv2};
        const float gy[2] = {horizontal ? gv1 : gu1, horizontal ? gv2 : gu2};
        const int e[2] = {e1, e2};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            // xs = fx X / Z + cx, ys = fy Y / Z + cy
            const float iz = aa_pick(T.iz, e[k]);
            const float PX = e[k] == 0 ? P[0][0] : (e[k] == 1 ? P[1][0] : P[2][0]);
            const float PY = e[k] == 0 ? P[0][1] : (e[k] == 1 ? P[1][1] : P[2][1]);
            R.vert[k] = K.faces[3 * f + e[k]];                                            // (mr_load checked the index)
            R.gX[k] = gx[k] * K.cam.fx * iz;
            R.gY[k] = gy[k] * K.cam.fy * iz;
            R.gZ[k] = -(R.gX[k] * PX + R.gY[k] * PY) * iz;
        }
    }
    return true;
}

// A[k] = v with a run-time k on an array that stays in registers
template <typename T>
__device__ __forceinline__ void aa_set(T (&A)[4], int k, T v)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) A[j] = j == k ? v : A[j];
}

// the four pairs of pixel p in a fixed order: (p - 1, p), (p, p + 1), (p - W, p), (p, p + W); p owns the second and the fourth
__device__ __forceinline__ bool aa_pair_of(const AaCtx& K, long long p, int px, int py, int k, long long& first, long long& second)
{
    const int W = K.cam.W, H = K.cam.H;
    if (k == 0) { first = p - 1; second = p; return px > 0; }
    if (k == 1) { first = p; second = p + 1; return px + 1 < W; }
    if (k == 2) { first = p - W; second = p; return py > 0; }
    first = p; second = p + W;
    return py + 1 < H;
}

template <bool CLIP>
static __global__ void __launch_bounds__(MR_BLOCK) aa_fwd_kernel(AaCtx K, int C, const float* __restrict__ color, float* __restrict__ out,
                                                                 int* __restrict__ dbg)
{
    const long long p = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
    if (p >= (long long)K.cam.H * K.cam.W) return;
    const int py = (int)(p / K.cam.W), px = (int)(p - (long long)py * K.cam.W);
    const float me = K.rast[p].w;
    float wk[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    long long ok[4] = {p, p, p, p};
    int code[2] = {0, 0};
    bool any = false;
#pragma unroll 1                                                                          // one copy of the analysis, not four
    for (int k = 0; k < 4; ++k) {
        long long first, second;
        if (!aa_pair_of(K, p, px, py, k, first, second)) continue;
        if (K.rast[k & 1 ? second : first].w == me) continue;
        AaPair R;
        if (!aa_pair<CLIP>(K, first, second, k < 2, R)) continue;
        if (k == 1) code[0] = R.code;
        if (k == 3) code[1] = R.code;
        if (R.target == p) { aa_set(wk, k, R.w); aa_set(ok, k, R.other); any = true; }
    }
    if (dbg) { dbg[2 * p + 0] = code[0]; dbg[2 * p + 1] = code[1]; }
    const float* cp = color + (size_t)p * C;
    float* o = out + (size_t)p * C;
    if (!any) {
        for (int c = 0; c < C; ++c) o[c] = cp[c];
        return;
    }
    // explicit FMAs: left to contraction, the vectorised pairs of channels were fused and the odd last channel was not, so a channel's
    // bits depended on C and on its position in the image
    for (int c = 0; c < C; ++c) {
        const float mine = cp[c];
        float acc = mine;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = __builtin_fmaf(wk[k], color[(size_t)ok[k] * C + c] - mine, acc);
        o[c] = acc;
    }
}

template <bool CLIP>
static __global__ void __launch_bounds__(MR_BLOCK) aa_bwd_kernel(AaCtx K, int C, const float* __restrict__ color,
                                                                 const float* __restrict__ d_out, float* __restrict__ d_color,
                                                                 float* __restrict__ d_vc)
{
    const long long p = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
    if (p >= (long long)K.cam.H * K.cam.W) return;
    const int py = (int)(p / K.cam.W), px = (int)(p - (long long)py * K.cam.W);
    const float me = K.rast[p].w;
    // d color[p] = g[p] + sum over its pairs of  -w g[p] (p receives)  or  +w g[target] (p is the other colour of the blend)
    float wk[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    long long tk[4] = {p, p, p, p};
    bool any = false;
#pragma unroll 1                                                                          // one copy of the analysis, not four
    for (int k = 0; k < 4; ++k) {
        long long first, second;
        if (!aa_pair_of(K, p, px, py, k, first, second)) continue;
        if (K.rast[k & 1 ? second : first].w == me) continue;
        AaPair R;
        if (!aa_pair<CLIP>(K, first, second, k < 2, R)) continue;
        if (R.target < 0) continue;
        aa_set(wk, k, R.target == p ? -R.w : R.w);
        aa_set(tk, k, R.target);
        any = true;
        if ((k & 1) && d_vc) {                                                            // p owns the pair: its vertex gradients, once
            float dw = 0.0f;
            for (int c = 0; c < C; ++c)
                dw += d_out[(size_t)R.target * C + c] * (color[(size_t)R.other * C + c] - color[(size_t)R.target * C + c]);
            if (dw != 0.0f) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float* dst = d_vc + 3 * (size_t)R.vert[j];
                    gs_atomic_add(dst + 0, dw * R.gX[j]);
                    gs_atomic_add(dst + 1, dw * R.gY[j]);
                    gs_atomic_add(dst + 2, dw * R.gZ[j]);
                }
            }
        }
    }
    const float* g = d_out + (size_t)p * C;
    float* o = d_color + (size_t)p * C;
    if (!any) {
        for (int c = 0; c < C; ++c) o[c] = g[c];
        return;
    }
    for (int c = 0; c < C; ++c) {
        float acc = g[c];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = __builtin_fmaf(wk[k], d_out[(size_t)tk[k] * C + c], acc);
        o[c] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static bool aa_dims_ok(int64_t V, int64_t F, int H, int W, int C)
{
    return V >= 0 && F >= 0 && V < ((int64_t)1 << 31) && F <= ((int64_t)1 << 24) && H >= 1 && W >= 1 &&
           (int64_t)H * W < ((int64_t)1 << 31) && C >= 1 && C <= 4096;
}

static AaTopo aa_topo(const void* topo, const AaLayout& L, int64_t F)
{
    const char* base = (const char*)topo;
    return AaTopo{(const int*)(base + L.off_head), (const int*)(base + L.off_slot), (const int*)(base + L.off_next), (long long)L.slots,
                  (long long)(3 * F)};
}

extern "C" {

size_t gs_mesh_topology_bytes(int64_t F)
{
    if (F < 0 || F > ((int64_t)1 << 24)) return 0;
    return aa_layout(F).total;
}

int gs_mesh_topology_build(int64_t F, const int32_t* faces, void* topo, size_t topo_bytes, void* stream)
{
    GS_CHECK_ARG(F >= 0 && F <= ((int64_t)1 << 24), "need 0 <= F <= 2^24");
    const AaLayout L = aa_layout(F);
    if (!topo || topo_bytes < L.total) {
        gs_set_error("%s: topology buffer too small (%zu < %zu)", __func__, topo ? topo_bytes : (size_t)0, L.total);
        return topo ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(F == 0 || faces, "null pointer");
    char* base = (char*)topo;
    unsigned long long* keys = (unsigned long long*)base;
    int* head = (int*)(base + L.off_head);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(aa_topo_fill_kernel, dim3(gs_cdiv((int64_t)L.slots, MR_BLOCK)), dim3(MR_BLOCK), 0, s, keys, head, (long long)L.slots);
    GS_CHECK_LAUNCH();
    if (F == 0) return GS_OK;
    hipLaunchKernelGGL(aa_topo_insert_kernel, dim3(gs_cdiv(3 * F, MR_BLOCK)), dim3(MR_BLOCK), 0, s, (long long)F, faces, keys, head,
                       (int*)(base + L.off_slot), (int*)(base + L.off_next), (long long)L.slots);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_meshaa_fwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                  float near, int cull, const void* topo, size_t topo_bytes, int C, const float* rast, const float* color, float* out,
                  int32_t* dbg, void* stream)
{
    GS_CHECK_ARG(aa_dims_ok(V, F, H, W, C), "need V < 2^31, F <= 2^24, H, W >= 1, H W < 2^31 and 1 <= C <= 4096");
    GS_CHECK_ARG(fx > 0.0f && fy > 0.0f && near > 0.0f, "fx, fy and near must be > 0");
    GS_CHECK_ARG(cull == 0 || cull == 1, "cull must be 0 (none) or 1 (back)");
    const AaLayout L = aa_layout(F);
    if (!topo || topo_bytes < L.total) {
        gs_set_error("%s: topology buffer too small (%zu < %zu)", __func__, topo ? topo_bytes : (size_t)0, L.total);
        return topo ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(rast && color && out && (F == 0 || (vc && faces)), "null pointer");
    AaCtx K{(long long)V, (long long)F, vc, faces, MrCam{fx, fy, cx, cy, near, H, W}, cull, (const float4*)rast, aa_topo(topo, L, F)};
    hipLaunchKernelGGL(aa_fwd_kernel<false>, dim3(gs_cdiv((int64_t)H * W, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, K, C, color,
                       out, (int*)dbg);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_meshaa_bwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                  float near, int cull, const void* topo, size_t topo_bytes, int C, const float* rast, const float* color,
                  const float* d_out, float* d_color, float* d_vc, void* stream)
{
    GS_CHECK_ARG(aa_dims_ok(V, F, H, W, C), "need V < 2^31, F <= 2^24, H, W >= 1, H W < 2^31 and 1 <= C <= 4096");
    GS_CHECK_ARG(fx > 0.0f && fy > 0.0f && near > 0.0f, "fx, fy and near must be > 0");
    GS_CHECK_ARG(cull == 0 || cull == 1, "cull must be 0 (none) or 1 (back)");
    const AaLayout L = aa_layout(F);
    if (!topo || topo_bytes < L.total) {
        gs_set_error("%s: topology buffer too small (%zu < %zu)", __func__, topo ? topo_bytes : (size_t)0, L.total);
        return topo ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(rast && color && d_out && d_color && (F == 0 || (vc && faces)), "null pointer");
    if (d_vc && V > 0) GS_CHECK_HIP(gs_zero_async(d_vc, (size_t)V * 12, (hipStream_t)stream));
    AaCtx K{(long long)V, (long long)F, vc, faces, MrCam{fx, fy, cx, cy, near, H, W}, cull, (const float4*)rast, aa_topo(topo, L, F)};
    hipLaunchKernelGGL(aa_bwd_kernel<false>, dim3(gs_cdiv((int64_t)H * W, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, K, C, color,
                       d_out, d_color, d_vc);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// ---- near_clip: the same pass on a rast made by gs_meshclip_fwd / gs_meshclip_resolve
int gs_meshclip_aa_fwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                       float near, int cull, const void* topo, size_t topo_bytes, int C, const float* rast, const float* color,
                       float* out, int32_t* dbg, void* stream)
{
    GS_CHECK_ARG(aa_dims_ok(V, F, H, W, C), "need V < 2^31, F <= 2^24, H, W >= 1, H W < 2^31 and 1 <= C <= 4096");
    GS_CHECK_ARG(fx > 0.0f && fy > 0.0f && near > 0.0f, "fx, fy and near must be > 0");
    GS_CHECK_ARG(cull == 0 || cull == 1, "cull must be 0 (none) or 1 (back)");
    const AaLayout L = aa_layout(F);
    if (!topo || topo_bytes < L.total) {
        gs_set_error("%s: topology buffer too small (%zu < %zu)", __func__, topo ? topo_bytes : (size_t)0, L.total);
        return topo ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(rast && color && out && (F == 0 || (vc && faces)), "null pointer");
    AaCtx K{(long long)V, (long long)F, vc, faces, MrCam{fx, fy, cx, cy, near, H, W}, cull, (const float4*)rast, aa_topo(topo, L, F)};
    hipLaunchKernelGGL(aa_fwd_kernel<true>, dim3(gs_cdiv((int64_t)H * W, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, K, C, color,
                       out, (int*)dbg);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_meshclip_aa_bwd(int64_t V, int64_t F, const float* vc, const int32_t* faces, float fx, float fy, float cx, float cy, int H, int W,
                       float near, int cull, const void* topo, size_t topo_bytes, int C, const float* rast, const float* color,
                       const float* d_out, float* d_color, float* d_vc, void* stream)
{
    GS_CHECK_ARG(aa_dims_ok(V, F, H, W, C), "need V < 2^31, F <= 2^24, H, W >= 1, H W < 2^31 and 1 <= C <= 4096");
    GS_CHECK_ARG(fx > 0.0f && fy > 0.0f && near > 0.0f, "fx, fy and near must be > 0");
    GS_CHECK_ARG(cull == 0 || cull == 1, "cull must be 0 (none) or 1 (back)");
    const AaLayout L = aa_layout(F);
    if (!topo || topo_bytes < L.total) {
        gs_set_error("%s: topology buffer too small (%zu < %zu)", __func__, topo ? topo_bytes : (size_t)0, L.total);
        return topo ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(rast && color && d_out && d_color && (F == 0 || (vc && faces)), "null pointer");
    if (d_vc && V > 0) GS_CHECK_HIP(gs_zero_async(d_vc, (size_t)V * 12, (hipStream_t)stream));
    AaCtx K{(long long)V, (long long)F, vc, faces, MrCam{fx, fy, cx, cy, near, H, W}, cull, (const float4*)rast, aa_topo(topo, L, F)};
    hipLaunchKernelGGL(aa_bwd_kernel<true>, dim3(gs_cdiv((int64_t)H * W, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, K, C, color,
                       d_out, d_color, d_vc);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

}  // extern "C"
