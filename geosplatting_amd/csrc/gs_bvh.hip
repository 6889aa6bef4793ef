// gs_bvh.hip -- ray queries against a triangle mesh without ray-tracing hardware: what the reference's OptiX stages get from
// optix_build_bvh(ctx, vertices, indices, rebuild=1) and from the shadow test inside optix_env_shade
// (rfstudio/graphics/_mesh/_optix/c_src/envsampling/kernel.cu:101-118).  A from-scratch statement of the semantics in
// include/geosplat_hip.h: an LBVH built on the device, an any-hit and a closest-hit query, and the brute-force form of both.
//
// Build (five small launches + the radix passes of gs_sort.hip, nothing read back, no workgroup waits on another):
//   bvh_init     resets the scene bounds and the arrival counters
//   bvh_bounds   finite bounds of the vertices of the valid triangles (ordered-integer atomic min / max)
//   bvh_morton   30-bit Morton code of every centroid as a 64-bit key, payload = face index
//   gs_isect_sort  stable ascending: equal codes keep ascending face index, so the order -- and the tree -- is well defined
//   bvh_karras   internal node i of Karras 2012 ("Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees"):
//                range, split, children; ties between equal codes are broken by the sorted position as in the paper (section 4)
//   bvh_fit      one thread per leaf climbs towards the root; at every node the first arrival exits, the second merges.
// Nodes carry a left child and a SKIP link (the node that follows the node's subtree in depth-first order), so a traversal keeps one
// integer of state instead of a stack: a private stack indexed at run time would live in scratch memory.
//
// Queries: one thread per ray, the rays of one origin adjacent in a wave.  The triangle test is Woop, Benthin and Wald, "Watertight
// Ray/Triangle Intersection" (JCGT 2013), restated from the paper; the box test is padded so that it never culls a box holding a
// triangle which that test would accept (see ray_box).  The brute-force form runs the SAME device routine over every triangle.
#include "gs_bvh_dev.h"
#include "gs_ws.h"

#define BVH_BLOCK 256
#define BVH_MAX_FACES ((int64_t)1 << 30)       // node indices are int32: 2 F - 1 <= 2^31 - 1
#define BVH_INVALID_CODE (1ull << 30)          // sorts behind every 30-bit Morton code
#define BVH_SORT_TILES 1                       // gs_isect_sort sorts 32 + tile_bits(1 x 1) = 33 key bits: every bit of the codes above

// ---- workspace ---------------------------------------------------------------------------------------------------------------
struct BvhWs {
    unsigned* bounds; int *count, *parent, *right, *last, *rsplit, *vals, *svals; unsigned long long *keys, *skeys; char* sort;
    size_t sort_bytes, total;
};
static BvhWs bvh_ws_layout(int64_t F, void* base)
{
    GsWs w(base, 256);
    BvhWs L;
    const size_t f = (size_t)F;
    L.bounds = w.take<unsigned>(64);               // 6 ordered-integer bounds
    L.count = w.take<int>(f);                      // arrival counter per internal node
    L.parent = w.take<int>(2 * f - 1);
    L.right = w.take<int>(f);                      // right child per internal node
    L.last = w.take<int>(f);                       // last leaf of the range per internal node
    L.rsplit = w.take<int>(f);                     // right child of the internal node whose split is at leaf g
    L.keys = w.take<unsigned long long>(f);
    L.vals = w.take<int>(f);
    L.skeys = w.take<unsigned long long>(f);
    L.svals = w.take<int>(f);
    L.sort_bytes = gs_sort_ws_bytes(F, BVH_SORT_TILES, BVH_SORT_TILES);
    L.sort = w.take<char>(L.sort_bytes);
    L.total = w.bytes();
    return L;
}

// ---- small device helpers ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned bvh_ord(float x)             // order-preserving map of the finite floats to unsigned
{
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float bvh_unord(unsigned u)
{
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// ---- build kernels -------------------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(BVH_BLOCK) bvh_init_kernel(long long F, unsigned* __restrict__ bounds, int* __restrict__ count)
{
    const long long i = (long long)blockIdx.x * BVH_BLOCK + threadIdx.x;
    if (i < 6) bounds[i] = i < 3 ? 0xffffffffu : 0u;
    if (i < F) count[i] = 0;
}

static __global__ void __launch_bounds__(BVH_BLOCK) bvh_bounds_kernel(long long V, long long F, const float* __restrict__ vertices,
                                                                      const int* __restrict__ faces, unsigned* __restrict__ bounds)
{
    __shared__ unsigned sb[6];
    if (threadIdx.x < 6) sb[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
    __syncthreads();
    unsigned lo0 = 0xffffffffu, lo1 = 0xffffffffu, lo2 = 0xffffffffu, hi0 = 0u, hi1 = 0u, hi2 = 0u;
    for (long long f = (long long)blockIdx.x * BVH_BLOCK + threadIdx.x; f < F; f += (long long)gridDim.x * BVH_BLOCK) {
        BvhTri t;
        if (!bvh_load_tri(vertices, faces, V, f, t)) continue;
        lo0 = min(lo0, bvh_ord(fminf(t.ax, fminf(t.bx, t.cx)))); hi0 = max(hi0, bvh_ord(fmaxf(t.ax, fmaxf(t.bx, t.cx))));
        lo1 = min(lo1, bvh_ord(fminf(t.ay, fminf(t.by, t.cy)))); hi1 = max(hi1, bvh_ord(fmaxf(t.ay, fmaxf(t.by, t.cy))));
        lo2 = min(lo2, bvh_ord(fminf(t.az, fminf(t.bz, t.cz)))); hi2 = max(hi2, bvh_ord(fmaxf(t.az, fmaxf(t.bz, t.cz))));
    }
    atomicMin(&sb[0], lo0); atomicMin(&sb[1], lo1); atomicMin(&sb[2], lo2);
    atomicMax(&sb[3], hi0); atomicMax(&sb[4], hi1); atomicMax(&sb[5], hi2);
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&bounds[threadIdx.x], sb[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&bounds[threadIdx.x], sb[threadIdx.x]);
}

__device__ __forceinline__ unsigned bvh_spread10(unsigned v)      // 10 bits -> every third bit
{
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ unsigned bvh_quant(float c, unsigned lo_u, unsigned hi_u)
{
    if (lo_u > hi_u) return 0u;                                   // no valid triangle at all
    const float lo = bvh_unord(lo_u), hi = bvh_unord(hi_u);
    const float ext = hi - lo;
    if (!(ext > 0.0f) || !bvh_finite(ext)) return 0u;
    const float x = (c - lo) / ext * 1024.0f;
    return (unsigned)fminf(fmaxf(x, 0.0f), 1023.0f);
}

static __global__ void __launch_bounds__(BVH_BLOCK) bvh_morton_kernel(long long V, long long F, const float* __restrict__ vertices,
                                                                      const int* __restrict__ faces, const unsigned* __restrict__ bounds,
                                                                      unsigned long long* __restrict__ keys, int* __restrict__ vals)
{
    const long long f = (long long)blockIdx.x * BVH_BLOCK + threadIdx.x;
    if (f >= F) return;
    BvhTri t;
    unsigned long long code = BVH_INVALID_CODE;
    if (bvh_load_tri(vertices, faces, V, f, t)) {
        const float third = 1.0f / 3.0f;
        const unsigned qx = bvh_quant((t.ax + t.bx + t.cx) * third, bounds[0], bounds[3]);
        const unsigned qy = bvh_quant((t.ay + t.by + t.cy) * third, bounds[1], bounds[4]);
        const unsigned qz = bvh_quant((t.az + t.bz + t.cz) * third, bounds[2], bounds[5]);
        code = (unsigned long long)((bvh_spread10(qx) << 2) | (bvh_spread10(qy) << 1) | bvh_spread10(qz));
    }
    keys[f] = code;
    vals[f] = (int)f;
}

// length of the common prefix of the keys at sorted positions i and j, -1 when j is outside [0, F); equal keys are told apart by
// their position (Karras 2012, section 4), so the prefix of two different positions is always finite and the tree well defined
__device__ __forceinline__ int bvh_delta(const unsigned long long* __restrict__ keys, long long F, long long i, long long j)
{
    if (j < 0 || j >= F) return -1;
    const unsigned long long x = keys[i] ^ keys[j];
    if (x != 0ull) return __clzll((long long)x);
    return 64 + __clz((int)((unsigned)i ^ (unsigned)j));
}

static __global__ void __launch_bounds__(BVH_BLOCK) bvh_karras_kernel(long long F, const unsigned long long* __restrict__ keys,
                                                                      BvhNode* __restrict__ nodes, int* __restrict__ parent,
                                                                      int* __restrict__ right, int* __restrict__ last, int* __restrict__ rsplit)
{
    const long long i = (long long)blockIdx.x * BVH_BLOCK + threadIdx.x;
    if (i == 0) parent[0] = -1;
    if (i >= F - 1) return;
    const int d = bvh_delta(keys, F, i, i + 1) > bvh_delta(keys, F, i, i - 1) ? 1 : -1;
    const int dmin = bvh_delta(keys, F, i, i - d);
    long long lmax = 2;
    while (lmax < 2 * F && bvh_delta(keys, F, i, i + lmax * d) > dmin) lmax *= 2;              // (bounded: the prefix is -1 outside)
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (bvh_delta(keys, F, i, i + (l + t) * d) > dmin) l += t;
    const long long j = i + l * d;
    const int dnode = bvh_delta(keys, F, i, j);
    long long s = 0, t = l;
    do {                                                                                       // binary search for the split
        t = (t + 1) / 2;
        if (bvh_delta(keys, F, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const long long g = i + s * d + (d < 0 ? -1 : 0);                                          // split: left = [first, g], right = [g + 1, last]
    const long long first = i < j ? i : j, lst = i < j ? j : i;
    if (g < first || g >= lst) return;                                                         // (cannot happen; keeps every store below in range)
    const int L = (int)(first == g ? (F - 1) + g : g);
    const int R = (int)(lst == g + 1 ? (F - 1) + g + 1 : g + 1);
    nodes[i].left = L;
    right[i] = R;
    last[i] = (int)lst;
    rsplit[g] = R;                                                                             // every leaf gap g < F - 1 is the split of exactly one node
    parent[L] = (int)i;
    parent[R] = (int)i;
}

// Box fit.  Thread i stores leaf i, then climbs: at every parent an arrival counter decides -- the first arrival exits, the second
// reads its sibling's box, merges and goes on, so every internal node is written once, by a thread that has seen both children, and
// nobody waits.  Ordering: the counter is bumped with ONE acquire-release read-modify-write at agent scope
// (__hip_atomic_fetch_add(..., __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT)): its release half orders this thread's box stores in front of
// the counter for every other XCD (L2 write-back), its acquire half makes the first arrival's stores visible to the loads that follow
// (cache invalidate) -- no separate __threadfence() pair is needed.  The sibling's box is read through a plain (not restrict, not
// const) pointer so the loads stay behind the atomic.  min / max are order independent: two builds are bit-identical.
static __global__ void __launch_bounds__(BVH_BLOCK) bvh_fit_kernel(long long V, long long F, const float* __restrict__ vertices,
                                                                   const int* __restrict__ faces, const int* __restrict__ svals,
                                                                   const int* __restrict__ parent, const int* __restrict__ right,
                                                                   const int* __restrict__ last, const int* __restrict__ rsplit,
                                                                   int* count, BvhNode* nodes)
{
    const long long i = (long long)blockIdx.x * BVH_BLOCK + threadIdx.x;
    if (i >= F) return;
    if (i < F - 1) {
        const int l = last[i];
        nodes[i].skip = (l >= F - 1 || l < 0) ? -1 : rsplit[l];
    }
    int f = svals[i];
    if (f < 0 || f >= F) f = 0;                                                                // (cannot happen: the payloads are a permutation)
    BvhTri t;
    float lo0 = INFINITY, lo1 = INFINITY, lo2 = INFINITY, hi0 = -INFINITY, hi1 = -INFINITY, hi2 = -INFINITY;      // the empty box
    if (bvh_load_tri(vertices, faces, V, f, t)) {
        lo0 = fminf(t.ax, fminf(t.bx, t.cx)); hi0 = fmaxf(t.ax, fmaxf(t.bx, t.cx));
        lo1 = fminf(t.ay, fminf(t.by, t.cy)); hi1 = fmaxf(t.ay, fmaxf(t.by, t.cy));
        lo2 = fminf(t.az, fminf(t.bz, t.cz)); hi2 = fmaxf(t.az, fmaxf(t.bz, t.cz));
    }
    int cur = (int)(F - 1 + i);
    nodes[cur].lo[0] = lo0; nodes[cur].lo[1] = lo1; nodes[cur].lo[2] = lo2;
    nodes[cur].hi[0] = hi0; nodes[cur].hi[1] = hi1; nodes[cur].hi[2] = hi2;
    nodes[cur].left = f;
    nodes[cur].skip = i == F - 1 ? -1 : rsplit[i];
    for (long long step = 0; step < F; ++step) {                                               // a path to the root has fewer than F nodes
        const int p = parent[cur];
        if (p < 0 || p >= F - 1) return;
        if (__hip_atomic_fetch_add(&count[p], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
        const int lc = nodes[p].left;
        const int sib = lc == cur ? right[p] : lc;
        if (sib < 0 || sib >= 2 * F - 1) return;
        lo0 = fminf(lo0, nodes[sib].lo[0]); lo1 = fminf(lo1, nodes[sib].lo[1]); lo2 = fminf(lo2, nodes[sib].lo[2]);
        hi0 = fmaxf(hi0, nodes[sib].hi[0]); hi1 = fmaxf(hi1, nodes[sib].hi[1]); hi2 = fmaxf(hi2, nodes[sib].hi[2]);
        nodes[p].lo[0] = lo0; nodes[p].lo[1] = lo1; nodes[p].lo[2] = lo2;
        nodes[p].hi[0] = hi0; nodes[p].hi[1] = hi1; nodes[p].hi[2] = hi2;
        cur = p;
    }
}

// ---- rays (the device routines are in gs_bvh_dev.h) ------------------------------------------------------------------------------
__device__ __forceinline__ BvhRay bvh_fetch_ray(long long ray, int S, const float* __restrict__ origins, const float* __restrict__ dirs,
                                                int dirs_per_point)
{
    const long long p = ray / S;
    const long long d = dirs_per_point ? ray : ray - p * S;
    return bvh_make_ray(origins[3 * p], origins[3 * p + 1], origins[3 * p + 2], dirs[3 * d], dirs[3 * d + 1], dirs[3 * d + 2]);
}

// One query kernel for both forms and both queries.  ANY: stop at the first accepted triangle.  Otherwise keep the accepted hit with
// the smallest fp32 t, the lowest face index among equal t: the result is a minimum over (t, face) of ALL accepted triangles and does
// not depend on the order in which they are met; boxes are culled against thi = the best t, inclusively, so a tie is never culled.
// The BVH loop visits every node at most once (skip links only move forward in depth-first order), so 2 F - 1 iterations bound it:
// a corrupt node buffer ends in a miss, never in a hang; indices read from the buffer are range-checked before use.
template <bool ANY, bool BRUTE>
static __global__ void __launch_bounds__(BVH_BLOCK) bvh_query_kernel(long long V, long long F, const float* __restrict__ vertices,
                                                                     const int* __restrict__ faces, const BvhNode* __restrict__ nodes,
                                                                     long long n_rays, int S, const float* __restrict__ origins,
                                                                     const float* __restrict__ dirs, int dirs_per_point, float tmin, float tmax,
                                                                     unsigned char* __restrict__ occ, float* __restrict__ t_out,
                                                                     int* __restrict__ face_out, float* __restrict__ bary_out)
{
    const long long ray = (long long)blockIdx.x * BVH_BLOCK + threadIdx.x;
    if (ray >= n_rays) return;
    const BvhRay r = bvh_fetch_ray(ray, S, origins, dirs, dirs_per_point);
    float best_t = INFINITY, best_b1 = 0.0f, best_b2 = 0.0f;
    int best_f = -1;
    bool hit = false;
    if (r.valid) {
        if (ANY && !BRUTE) {
            hit = bvh_any_hit(r, V, F, vertices, faces, nodes, tmin, tmax);
        } else if (BRUTE) {
            for (long long f = 0; f < F; ++f) {
                BvhTri tr;
                float t, b1, b2;
                if (!bvh_load_tri(vertices, faces, V, f, tr) || !bvh_tri_test(r, tr, tmin, tmax, t, b1, b2)) continue;
                hit = true;
                if (ANY) break;
                if (t < best_t || (t == best_t && (int)f < best_f)) { best_t = t; best_f = (int)f; best_b1 = b1; best_b2 = b2; }
            }
        } else {
            const float absSz = fabsf(r.Sz);
            const long long n_nodes = 2 * F - 1;
            int node = 0;
            for (long long it = 0; it < n_nodes && node >= 0 && node < n_nodes; ++it) {
                const BvhNode n = nodes[node];
                const float thi = ANY ? tmax : fminf(tmax, best_t);
                if (!bvh_ray_box(r, absSz, n, tmin, thi)) { node = n.skip; continue; }
                if (node < F - 1) { node = n.left; continue; }
                node = n.skip;
                const int f = n.left;
                BvhTri tr;
                float t, b1, b2;
                if (f < 0 || f >= F || !bvh_load_tri(vertices, faces, V, f, tr) || !bvh_tri_test(r, tr, tmin, tmax, t, b1, b2)) continue;
                hit = true;
                if (ANY) break;
                if (t < best_t || (t == best_t && f < best_f)) { best_t = t; best_f = f; best_b1 = b1; best_b2 = b2; }
            }
        }
    }
    if (ANY) {
        occ[ray] = hit ? 1 : 0;
    } else {
        t_out[ray] = best_t;
        face_out[ray] = best_f;
        bary_out[2 * ray] = best_b1;
        bary_out[2 * ray + 1] = best_b2;
    }
}

// ---- C-ABI ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t gs_bvh_bytes(int64_t F)
{
    if (F < 1 || F > BVH_MAX_FACES) return 0;
    return (size_t)(2 * F - 1) * sizeof(BvhNode);
}

extern "C" size_t gs_bvh_ws_bytes(int64_t F)
{
    if (F < 1 || F > BVH_MAX_FACES) return 0;
    return bvh_ws_layout(F, nullptr).total;
}

extern "C" int gs_bvh_build(int64_t V, int64_t F, const float* vertices, const int32_t* faces, void* bvh, size_t bvh_bytes, void* ws,
                            size_t ws_bytes, void* stream)
{
    GS_CHECK_ARG(F >= 1, "empty mesh: F must be at least 1");
    GS_CHECK_ARG(F <= BVH_MAX_FACES, "too many faces: at most 2^30");
    GS_CHECK_ARG(V >= 1 && V <= 2147483647ll, "bad vertex count");
    GS_CHECK_ARG(bvh_bytes >= gs_bvh_bytes(F), "node buffer too small");
    const BvhWs L = bvh_ws_layout(F, ws);
    GS_CHECK_ARG(ws_bytes >= L.total, "workspace too small");
    GS_CHECK_ARG(vertices != nullptr && faces != nullptr, "vertices and faces must not be NULL");
    GS_CHECK_ARG(bvh != nullptr && ws != nullptr, "node buffer and workspace must not be NULL");
    GS_CHECK_ARG(((uintptr_t)bvh & 15) == 0 && ((uintptr_t)ws & 15) == 0, "node buffer and workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    BvhNode* nodes = (BvhNode*)bvh;
    const int blocks = gs_cdiv(F, BVH_BLOCK);
    hipLaunchKernelGGL(bvh_init_kernel, dim3(blocks), dim3(BVH_BLOCK), 0, s, (long long)F, L.bounds, L.count);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bvh_bounds_kernel, dim3(blocks < 512 ? blocks : 512), dim3(BVH_BLOCK), 0, s, (long long)V, (long long)F, vertices,
                       faces, L.bounds);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bvh_morton_kernel, dim3(blocks), dim3(BVH_BLOCK), 0, s, (long long)V, (long long)F, vertices, faces, L.bounds, L.keys, L.vals);
    GS_CHECK_LAUNCH();
    const int rc = gs_isect_sort(F, (const int64_t*)L.keys, L.vals, (int64_t*)L.skeys, L.svals, BVH_SORT_TILES, BVH_SORT_TILES, L.sort,
                                 L.sort_bytes, stream);
    if (rc != GS_OK) return rc;
    hipLaunchKernelGGL(bvh_karras_kernel, dim3(blocks), dim3(BVH_BLOCK), 0, s, (long long)F, L.skeys, nodes, L.parent, L.right, L.last, L.rsplit);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bvh_fit_kernel, dim3(blocks), dim3(BVH_BLOCK), 0, s, (long long)V, (long long)F, vertices, faces, L.svals, L.parent,
                       L.right, L.last, L.rsplit, L.count, nodes);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

static int bvh_check_query(const char* fn, int64_t V, int64_t F, const float* vertices, const int32_t* faces, int64_t P, int S,
                           const float* origins, const float* dirs, int dirs_per_point, const void* bvh)
{
    const char* msg = nullptr;
    if (F < 1) msg = "empty mesh: F must be at least 1";
    else if (F > BVH_MAX_FACES) msg = "too many faces: at most 2^30";
    else if (V < 1 || V > 2147483647ll) msg = "bad vertex count";
    else if (P < 0) msg = "negative P";
    else if (S < 0) msg = "negative S";
    else if (dirs_per_point != 0 && dirs_per_point != 1) msg = "dirs_per_point must be 0 or 1";
    else if ((S > 0 && P > 2147483647ll / S)) msg = "too many rays: P S must be below 2^31";
    else if (vertices == nullptr || faces == nullptr) msg = "vertices and faces must not be NULL";
    else if (P > 0 && S > 0 && (origins == nullptr || dirs == nullptr)) msg = "origins and dirs must not be NULL";
    else if (((uintptr_t)bvh & 15) != 0) msg = "node buffer must be 16-byte aligned";
    if (msg) { gs_set_error("%s: %s", fn, msg); return GS_EINVAL; }
    return GS_OK;
}

extern "C" int gs_ray_occluded(int64_t V, int64_t F, const float* vertices, const int32_t* faces, const void* bvh, int64_t P, int S,
                               const float* origins, const float* dirs, int dirs_per_point, float tmin, float tmax, uint8_t* out,
                               void* stream)
{
    const int rc = bvh_check_query(__func__, V, F, vertices, faces, P, S, origins, dirs, dirs_per_point, bvh);
    if (rc != GS_OK) return rc;
    const long long n = (long long)P * S;
    if (n == 0) return GS_OK;
    GS_CHECK_ARG(out != nullptr, "null output");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(gs_cdiv(n, BVH_BLOCK)), block(BVH_BLOCK);
    if (bvh != nullptr)
        hipLaunchKernelGGL((bvh_query_kernel<true, false>), grid, block, 0, s, (long long)V, (long long)F, vertices, faces, (const BvhNode*)bvh,
                           n, S, origins, dirs, dirs_per_point, tmin, tmax, out, (float*)nullptr, (int*)nullptr, (float*)nullptr);
    else
        hipLaunchKernelGGL((bvh_query_kernel<true, true>), grid, block, 0, s, (long long)V, (long long)F, vertices, faces, (const BvhNode*)nullptr,
                           n, S, origins, dirs, dirs_per_point, tmin, tmax, out, (float*)nullptr, (int*)nullptr, (float*)nullptr);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_ray_closest(int64_t V, int64_t F, const float* vertices, const int32_t* faces, const void* bvh, int64_t P, int S,
                              const float* origins, const float* dirs, int dirs_per_point, float tmin, float tmax, float* t, int32_t* face,
                              float* bary, void* stream)
{
    const int rc = bvh_check_query(__func__, V, F, vertices, faces, P, S, origins, dirs, dirs_per_point, bvh);
    if (rc != GS_OK) return rc;
    const long long n = (long long)P * S;
    if (n == 0) return GS_OK;
    GS_CHECK_ARG(t != nullptr && face != nullptr && bary != nullptr, "null output");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(gs_cdiv(n, BVH_BLOCK)), block(BVH_BLOCK);
    if (bvh != nullptr)
        hipLaunchKernelGGL((bvh_query_kernel<false, false>), grid, block, 0, s, (long long)V, (long long)F, vertices, faces, (const BvhNode*)bvh,
                           n, S, origins, dirs, dirs_per_point, tmin, tmax, (unsigned char*)nullptr, t, face, bary);
    else
        hipLaunchKernelGGL((bvh_query_kernel<false, true>), grid, block, 0, s, (long long)V, (long long)F, vertices, faces,
                           (const BvhNode*)nullptr, n, S, origins, dirs, dirs_per_point, tmin, tmax, (unsigned char*)nullptr, t, face, bary);
    GS_CHECK_LAUNCH();
    return GS_OK;
}
