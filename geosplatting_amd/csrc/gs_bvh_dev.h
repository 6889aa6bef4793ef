// gs_bvh_dev.h -- the device-side ray routines of csrc/gs_bvh.hip, shared with the kernels that trace rays inline
// (csrc/gs_envshade.hip): the node and triangle types, the ray set-up, the watertight triangle test, the padded box test and the
// stackless any-hit traversal.  include/geosplat_hip.h states the semantics; gs_bvh.hip builds the node buffer.
#pragma once
#include "gs_common.h"

#include <math.h>

// the node layout of include/geosplat_hip.h
struct alignas(16) BvhNode {
    float lo[3], hi[3];
    int left;      // internal: left child; leaf: face index
    int skip;      // next node in depth-first order once this subtree is done, -1 = end
};
static_assert(sizeof(BvhNode) == 32, "node layout is a contract");

__device__ __forceinline__ bool bvh_finite(float x) { return fabsf(x) <= 3.402823466e38f; }          // false for NaN and inf

struct BvhTri { float ax, ay, az, bx, by, bz, cx, cy, cz; };

// loads face f; false when an index is outside [0, V) or a coordinate is not finite: such a triangle is never hit and is in no box
__device__ __forceinline__ bool bvh_load_tri(const float* __restrict__ vertices, const int* __restrict__ faces, long long V, long long f,
                                             BvhTri& t)
{
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
    t.ax = vertices[3ll * i0]; t.ay = vertices[3ll * i0 + 1]; t.az = vertices[3ll * i0 + 2];
    t.bx = vertices[3ll * i1]; t.by = vertices[3ll * i1 + 1]; t.bz = vertices[3ll * i1 + 2];
    t.cx = vertices[3ll * i2]; t.cy = vertices[3ll * i2 + 1]; t.cz = vertices[3ll * i2 + 2];
    return bvh_finite(t.ax) && bvh_finite(t.ay) && bvh_finite(t.az) && bvh_finite(t.bx) && bvh_finite(t.by) && bvh_finite(t.bz) &&
           bvh_finite(t.cx) && bvh_finite(t.cy) && bvh_finite(t.cz);
}

struct BvhRay {
    float ox, oy, oz;                // origin
    float ix, iy, iz;                // 1 / direction (may be +-inf)
    float pkx, pky, pkz;             // origin in the permuted axes
    float Sx, Sy, Sz;                // shear and scale of the watertight test
    int kx, ky, kz;                  // permutation: kz = the dominant axis of the direction
    bool valid;
};

__device__ __forceinline__ float bvh_sel(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }   // no private array

__device__ __forceinline__ BvhRay bvh_make_ray(float ox, float oy, float oz, float dx, float dy, float dz)
{
#pragma clang fp contract(off)
    BvhRay r;
    r.ox = ox; r.oy = oy; r.oz = oz;
    r.valid = bvh_finite(ox) && bvh_finite(oy) && bvh_finite(oz) && bvh_finite(dx) && bvh_finite(dy) && bvh_finite(dz) &&
              (dx != 0.0f || dy != 0.0f || dz != 0.0f);
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    int kz = 0;
    if (ay > ax) kz = 1;
    if (az > fmaxf(ax, ay)) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1;
    int ky = kx == 2 ? 0 : kx + 1;
    const float dkz = bvh_sel(dx, dy, dz, kz);
    if (dkz < 0.0f) { const int s = kx; kx = ky; ky = s; }                                     // keeps the winding
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.Sx = bvh_sel(dx, dy, dz, kx) / dkz;
    r.Sy = bvh_sel(dx, dy, dz, ky) / dkz;
    r.Sz = 1.0f / dkz;
    r.pkx = bvh_sel(ox, oy, oz, kx); r.pky = bvh_sel(ox, oy, oz, ky); r.pkz = bvh_sel(ox, oy, oz, kz);
    r.ix = 1.0f / dx; r.iy = 1.0f / dy; r.iz = 1.0f / dz;
    return r;
}

// Watertight ray/triangle test (Woop, Benthin, Wald 2013), both sides, no culling.  Accepts iff the scaled edge functions U, V, W are
// all >= 0 or all <= 0, det = U + V + W != 0 and tmin < t < tmax with t = (U Az + V Bz + W Cz) / det as computed HERE in fp32.
// Contraction is off: an edge shared by two triangles gives the two of them the products (a b) and (c d) in the opposite order, and
// fl(a b) - fl(c d) is the exact negative of fl(c d) - fl(a b), which fma(a, b, -c d) and fma(c, d, -a b) are not -- the signs at a
// shared edge must agree for the mesh to be watertight.  An edge function that is exactly 0 is recomputed in fp64, where the products
// of fp32 values are exact and the sign of the difference is therefore the true one.  (b1, b2) weigh vertices 1 and 2.
__device__ __forceinline__ bool bvh_tri_test(const BvhRay& r, const BvhTri& tr, float tmin, float tmax, float& t_out, float& b1, float& b2)
{
#pragma clang fp contract(off)
    const float Akz = bvh_sel(tr.ax, tr.ay, tr.az, r.kz) - r.pkz, Bkz = bvh_sel(tr.bx, tr.by, tr.bz, r.kz) - r.pkz,
                Ckz = bvh_sel(tr.cx, tr.cy, tr.cz, r.kz) - r.pkz;
    const float Ax = (bvh_sel(tr.ax, tr.ay, tr.az, r.kx) - r.pkx) - r.Sx * Akz, Ay = (bvh_sel(tr.ax, tr.ay, tr.az, r.ky) - r.pky) - r.Sy * Akz;
    const float Bx = (bvh_sel(tr.bx, tr.by, tr.bz, r.kx) - r.pkx) - r.Sx * Bkz, By = (bvh_sel(tr.bx, tr.by, tr.bz, r.ky) - r.pky) - r.Sy * Bkz;
    const float Cx = (bvh_sel(tr.cx, tr.cy, tr.cz, r.kx) - r.pkx) - r.Sx * Ckz, Cy = (bvh_sel(tr.cx, tr.cy, tr.cz, r.ky) - r.pky) - r.Sy * Ckz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    bool neg = U < 0.0f || V < 0.0f || W < 0.0f, pos = U > 0.0f || V > 0.0f || W > 0.0f;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {
        const double Ud = (double)Cx * (double)By - (double)Cy * (double)Bx, Vd = (double)Ax * (double)Cy - (double)Ay * (double)Cx,
                     Wd = (double)Bx * (double)Ay - (double)By * (double)Ax;
        neg = Ud < 0.0 || Vd < 0.0 || Wd < 0.0;
        pos = Ud > 0.0 || Vd > 0.0 || Wd > 0.0;
        U = (float)Ud; V = (float)Vd; W = (float)Wd;
    }
    if (neg && pos) return false;
    const float det = U + V + W;
    if (!(det != 0.0f) || !bvh_finite(det)) return false;                                      // zero area or edge-on (and NaN)
    const float Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    const float T = (U * Az + V * Bz) + W * Cz;
    const float t = T / det;
    if (!(t > tmin && t < tmax)) return false;
    t_out = t;
    b1 = V / det;
    b2 = W / det;
    return true;
}

// Conservative slab test: true whenever the box holds a valid triangle that bvh_tri_test would accept with tlo < t < thi.
// Why the padding suffices.  Let M be the largest |coordinate - origin| over the box (so over every triangle in it).  The triangle
// test decides on sheared coordinates (v - o)[kx] - Sx (v - o)[kz] whose absolute error is at most 2^-24 M (the difference)
// + 2 * 2^-24 M (rounding of Sx with |Sx| <= 1, and of the product) + 2^-24 * 2 M (the last subtraction), under 2^-21 M; its sign
// decisions are exact for those rounded coordinates (monotone rounding of the two products; exact zero goes to fp64).  So an accepted
// triangle is crossed by the exact ray after its vertices moved by less than 2^-21 M in the two minor axes: the exact ray passes
// within 2^-21 M of the box, at a parameter that is a convex combination of the vertices' (v - o)[kz] / d[kz], while the t the kernel
// compares is that value up to a few 2^-24 M |Sz|.  The box is therefore widened by pad = 2^-18 M on every side -- eight times the
// bound, which also absorbs the rounding of the six differences and six products below -- and the interval by pad |Sz| at both ends.
// Special values: a direction component of +-0 has a reciprocal of +-inf; the slab then gives (-inf, +inf) when the origin is
// strictly inside the padded slab and (+inf, +inf) or (-inf, -inf) when outside -- correct.  0 * inf = NaN arises only when the
// origin lies exactly ON a padded face, at 2^-18 M from the box, eight times farther than any accepted triangle can be: fminf / fmaxf
// drop a NaN operand, and culling or keeping such a box are both right.  A box of zero thickness is padded like any other (M > 0
// unless the box is the origin itself, which holds only zero-area triangles); an origin inside gives tnear < 0 < tfar; the empty
// box (+inf, -inf) of non-finite triangles turns everything into NaN, every comparison is false, and it is culled.
__device__ __forceinline__ bool bvh_ray_box(const BvhRay& r, float absSz, const BvhNode& n, float tlo, float thi)
{
#pragma clang fp contract(off)
    float l0 = n.lo[0] - r.ox, l1 = n.lo[1] - r.oy, l2 = n.lo[2] - r.oz;
    float h0 = n.hi[0] - r.ox, h1 = n.hi[1] - r.oy, h2 = n.hi[2] - r.oz;
    const float M = fmaxf(fmaxf(fmaxf(fabsf(l0), fabsf(h0)), fmaxf(fabsf(l1), fabsf(h1))), fmaxf(fabsf(l2), fabsf(h2)));
    const float pad = M * 0x1p-18f;
    l0 -= pad; l1 -= pad; l2 -= pad; h0 += pad; h1 += pad; h2 += pad;
    const float a0 = l0 * r.ix, b0 = h0 * r.ix, a1 = l1 * r.iy, b1 = h1 * r.iy, a2 = l2 * r.iz, b2 = h2 * r.iz;
    const float et = pad * absSz;
    const float tn = fmaxf(fmaxf(fminf(a0, b0), fminf(a1, b1)), fmaxf(fminf(a2, b2), tlo - et));
    const float tf = fminf(fminf(fmaxf(a0, b0), fmaxf(a1, b1)), fminf(fmaxf(a2, b2), thi + et));
    return tn <= tf;
}

// Any-hit traversal of the node buffer for a VALID ray (r.valid): true at the first accepted triangle with tmin < t < tmax.  One integer
// of state (skip links), no stack.  The loop visits every node at most once (skip links only move forward in depth-first order), so
// 2 F - 1 iterations bound it: a corrupt node buffer ends in a miss, never in a hang; indices read from the buffer are range-checked
// before use.
__device__ __forceinline__ bool bvh_any_hit(const BvhRay& r, long long V, long long F, const float* __restrict__ vertices,
                                            const int* __restrict__ faces, const BvhNode* __restrict__ nodes, float tmin, float tmax)
{
    const float absSz = fabsf(r.Sz);
    const long long n_nodes = 2 * F - 1;
    int node = 0;
    for (long long it = 0; it < n_nodes && node >= 0 && node < n_nodes; ++it) {
        const BvhNode n = nodes[node];
        if (!bvh_ray_box(r, absSz, n, tmin, tmax)) { node = n.skip; continue; }
        if (node < F - 1) { node = n.left; continue; }
        node = n.skip;
        const int f = n.left;
        BvhTri tr;
        float t, b1, b2;
        if (f < 0 || f >= F || !bvh_load_tri(vertices, faces, V, f, tr) || !bvh_tri_test(r, tr, tmin, tmax, t, b1, b2)) continue;
        return true;
    }
    return false;
}
