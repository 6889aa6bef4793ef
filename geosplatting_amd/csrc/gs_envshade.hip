// gs_envshade.hip -- the Monte-Carlo environment shader of the reference's stage 2 on the ray routines of gs_bvh_dev.h: per point
// 2 n^2 samples (n^2 drawn from the lat-long light's CDF tables, n^2 from the BSDF), combined with the balance heuristic and each
// weighted by a shadow ray.  What optix_env_shade computes (rfstudio/graphics/_mesh/_optix: envsampling/kernel.cu, bsdf.h), written
// from the mathematics that include/geosplat_hip.h states; tests/envshade_ref.py restates the same in float64.
//
// Mapping.  A group of G lanes (G = 1, 16 or 64) owns one point: lane l of the group takes the iterations i = l, l + G, ... and
// enters the point's PCG stream 2 + 5 i draws in (the state is an LCG: a jump is one multiply-add by constants).  With G = 1 this is
// the reference's thread per point; with G > 1 the rays a wave traces together share an origin, and the table reads of a point are
// spread over its lanes.  Every lane of a block runs every iteration (a lane without work carries zeros), so the wave-wide
// operations of the backward pass see 64 active lanes.
// Sums.  Per point: each lane adds its iterations in order, the group is folded with a fixed xor butterfly, one lane stores -- no
// atomics, the same bits every run.  light_grad is the only sum across workgroups: after every sample the wave merges the adds that
// go to one texel (a few leader rounds: importance sampling sends most of a wave's light samples to a handful of bright texels),
// then one lane per merged texel and every lane left over issue their float atomics.
// The shadow ray is bvh_any_hit inline: one integer of state, no stack, no direction ever stored (except in the debug log).
#include "gs_bvh_dev.h"

#define ENV_BLOCK 256
#define ENV_PI 3.14159265358979323846f
#define ENV_ONE_BELOW 0.99999994f              // the largest float below 1
#define ENV_EPS 1e-4f                          // the clamp of every specular cosine
#define ENV_MIN_ROUGHNESS 0.08f
#define ENV_TMAX 1e16f
#define ENV_PCG_MUL 747796405u
#define ENV_PCG_INC 2891336453u

struct EnvArgs {
    long long P;
    const float *mask, *ro, *pos, *nrm, *view, *kd, *ks;
    int H, W, row_steps, col_steps;
    const float *light, *pdf, *rows, *cols;
    int T, n;
    const int* perms;
    unsigned seed, jump_mul, jump_inc;         // the LCG step over 5 G draws
    int bsdf;
    float shadow_scale;
    long long V, F;
    const float* vertices;
    const int* faces;
    const BvhNode* nodes;
    float *diff, *spec, *resi;                 // forward
    float *log_dirs, *log_pdf, *log_vis;       // forward, LOG only
    const float *d_diff, *d_spec;              // backward
    float *d_pos, *d_nrm, *d_kd, *d_ks, *d_light;
    int merge_rounds;
};

// ---- small vectors ---------------------------------------------------------------------------------------------------------------
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ V3 unit(V3 a)                                   // the zero vector stays zero
{
    const float l = sqrtf(dot(a, a));
    return l > 0.0f ? a * (1.0f / l) : v3(0.0f, 0.0f, 0.0f);
}
__device__ __forceinline__ V3 load3(const float* __restrict__ p, long long i) { return v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
__device__ __forceinline__ float luma(V3 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }

// Duff et al., "Building an Orthonormal Basis, Revisited" (JCGT 2017): no branch on the normal
__device__ __forceinline__ void env_basis(V3 n, V3& b1, V3& b2)
{
    const float sign = copysignf(1.0f, n.z);
    const float a = -1.0f / (sign + n.z);
    const float b = n.x * n.y * a;
    b1 = v3(1.0f + sign * n.x * n.x * a, sign * b, -sign * n.x);
    b2 = v3(b, sign + n.y * n.y * a, -n.y);
}

// ---- the random stream -----------------------------------------------------------------------------------------------------------
// PCG-RXS-M-XS output of an LCG state (www.pcg-random.org; the 32-bit hash of Jarzynski and Olano, JCGT 2020)
__device__ __forceinline__ unsigned env_pcg_out(unsigned s)
{
    const unsigned w = ((s >> ((s >> 28u) + 4u)) ^ s) * 277803737u;
    return (w >> 22u) ^ w;
}
__device__ __forceinline__ unsigned env_pcg_next(unsigned& s)
{
    const unsigned o = env_pcg_out(s);
    s = s * ENV_PCG_MUL + ENV_PCG_INC;
    return o;
}
__device__ __forceinline__ float env_uniform(unsigned& s) { return (float)(env_pcg_next(s) & 0xFFFFFFu) * 0x1p-24f; }   // exact
// the state after `steps` further draws (Brown, "Random Number Generation with Arbitrary Strides", 1994)
__host__ __device__ inline void env_lcg_jump(unsigned steps, unsigned& mul, unsigned& inc)
{
    unsigned cm = ENV_PCG_MUL, ci = ENV_PCG_INC;
    mul = 1u; inc = 0u;
    for (; steps > 0u; steps >>= 1) {
        if (steps & 1u) { mul *= cm; inc = inc * cm + ci; }
        ci = (cm + 1u) * ci;
        cm *= cm;
    }
}

// ---- the light -------------------------------------------------------------------------------------------------------------------
// One level of the inverse-CDF pick: a fixed number of bisection steps over cdf[0 .. size - 1], then the position inside the chosen
// cell from the remainder.  Plain fp32, no contraction: the comparisons and the index are reproducible bit for bit.
__device__ __forceinline__ int env_cdf_pick(const float* __restrict__ cdf, int size, int steps, float x, float& rem)
{
#pragma clang fp contract(off)
    x = fminf(x, ENV_ONE_BELOW);
    int lo = 0, hi = size - 1;
    for (int k = 0; k < steps; ++k) {
        const int mid = (lo + hi) >> 1;
        const float c = cdf[mid];
        lo = x >= c ? mid : lo;
        hi = x < c ? mid : hi;
    }
    float width, off;
    if (hi == 0) { width = cdf[0]; off = x; }
    else { const float below = cdf[hi - 1]; width = cdf[hi] - below; off = x - below; }
    rem = fminf(off / width, ENV_ONE_BELOW);
    return hi;
}

__device__ __forceinline__ int env_texel(float t, int size) { return (int)fminf(fmaxf(t * (float)size, 0.0f), (float)(size - 1)); }

// nearest texel of a direction and the solid-angle density of the light's pdf table there
__device__ __forceinline__ float env_light_pdf(const EnvArgs& a, V3 d, int& tx, int& ty)
{
    const float u = atan2f(d.x, -d.z) * (0.5f / ENV_PI) + 0.5f;
    const float v = acosf(fminf(fmaxf(d.y, -1.0f), 1.0f)) * (1.0f / ENV_PI);
    tx = env_texel(u, a.W);
    ty = env_texel(v, a.H);
    const float weight = (float)a.W * (float)a.H / (2.0f * ENV_PI * ENV_PI * fmaxf(sinf(v * ENV_PI), 1e-4f));
    return a.pdf[(long long)ty * a.W + tx] * weight;
}

__device__ __forceinline__ V3 env_light_sample(const EnvArgs& a, float sx, float sy)
{
    float rx, ry;
    const int y = env_cdf_pick(a.rows, a.H, a.row_steps, sy, ry);
    const int x = env_cdf_pick(a.cols + (long long)y * a.W, a.W, a.col_steps, sx, rx);
    const float u = ((float)x + rx) / (float)a.W, v = ((float)y + ry) / (float)a.H;
    float sp, cp, st, ct;
    sincosf((u * 2.0f - 1.0f) * ENV_PI, &sp, &cp);
    sincosf(v * ENV_PI, &st, &ct);
    return v3(st * sp, ct, -st * cp);
}

// ---- the point and its BSDF ------------------------------------------------------------------------------------------------------
struct EnvPoint {
    V3 ro, pos, n, kd, ks, wo;          // n as given (not normalised); wo = unit(view - pos)
    V3 fw, fu, fv;                      // frame of the normalised normal
    V3 wol, woln;                       // wo in the frame; the same normalised
    float alpha, pD, pS;                // roughness^2; lobe probabilities
    float wo_len;
};

__device__ __forceinline__ float env_pow5(float x) { const float x2 = x * x; return x2 * x2 * x; }
__device__ __forceinline__ float env_clampc(float c) { return fminf(fmaxf(c, ENV_EPS), 1.0f - ENV_EPS); }
__device__ __forceinline__ float env_ndf(float a2, float c)                 // GGX D with the denominator in the form d = (c a2 - c) c + 1
{
    const float d = (c * a2 - c) * c + 1.0f;
    return a2 / (d * d * ENV_PI);
}
__device__ __forceinline__ float env_g1(float a2, float c)                  // Smith G1, 0 at and below the horizon
{
    if (c <= 0.0f) return 0.0f;
    const float c2 = c * c;
    return 2.0f / (1.0f + sqrtf(1.0f + a2 * fmaxf(1.0f - c2, 0.0f) / c2));
}

__device__ __forceinline__ void env_point_setup(EnvPoint& q, V3 view)
{
    const V3 to_view = view - q.pos;
    q.wo_len = sqrtf(dot(to_view, to_view));
    q.wo = unit(to_view);
    q.fw = unit(q.n);
    env_basis(q.fw, q.fu, q.fv);
    q.wol = v3(dot(q.wo, q.fu), dot(q.wo, q.fv), dot(q.wo, q.fw));
    q.woln = unit(q.wol);
    q.alpha = q.ks.y * q.ks.y;
    const float metallic = q.ks.z;
    const V3 f0 = v3(0.04f, 0.04f, 0.04f) * (1.0f - metallic) + q.kd * metallic;
    const float wd = (1.0f - metallic) * luma(q.kd);
    float wsp = 0.0f;
    if (q.woln.z > 0.0f) {                                                  // Schlick albedo of the specular colour towards the viewer
        const float s = env_pow5(1.0f - env_clampc(q.woln.z));
        wsp = luma(f0 * (1.0f - s) + v3(s, s, s));
    }
    q.pD = (wd + wsp) > 0.0f ? wd / (wd + wsp) : 1.0f;
    q.pS = 1.0f - q.pD;
}

// pdf of the VNDF lobe for a pair of local directions, reflection Jacobian included
__device__ __forceinline__ float env_ggx_pdf(const EnvPoint& q, V3 wi)
{
    const V3 wil = v3(dot(wi, q.fu), dot(wi, q.fv), dot(wi, q.fw));
    if (!(q.wol.z > 0.0f && wil.z > 0.0f)) return 0.0f;
    const V3 m = unit(wil + q.wol);
    const float vh = dot(m, q.wol);
    const float a2 = q.alpha * q.alpha;
    float pdf = env_g1(a2, q.wol.z) * env_ndf(a2, m.z) * fmaxf(0.0f, vh) / q.wol.z;
    return pdf / (4.0f * vh);
}
__device__ __forceinline__ void env_mix(float& pdf, float other, float weight) { if (weight > 1e-6f) pdf += other * weight; }

// mixture pdf of a direction that the light produced
__device__ __forceinline__ float env_bsdf_pdf(const EnvPoint& q, V3 wi)
{
    const float nl = dot(q.n, wi), nv = dot(q.n, q.wo);
    if (fminf(nv, nl) < 1e-6f) return 1.0f;
    float pdf = 0.0f;
    if (q.pD > 0.0f) env_mix(pdf, fmaxf(nl, 0.0f) * (1.0f / ENV_PI), q.pD);
    if (q.pS > 0.0f) env_mix(pdf, env_ggx_pdf(q, wi), 1.0f - q.pD);
    return pdf;
}

// a direction from the mixture of the cosine lobe and the GGX lobe of visible normals (Heitz, JCGT 2018), and its mixture pdf
__device__ __forceinline__ V3 env_bsdf_sample(const EnvPoint& q, float u1, float u2, float u3, float& pdf)
{
    V3 wi;
    if (u3 < q.pD) {
        if (q.pD < 1e-4f) { pdf = 1.0f; return q.n; }
        float sp, cp;
        sincosf(2.0f * ENV_PI * u1, &sp, &cp);
        const float ct = sqrtf(u2), st = sqrtf(1.0f - u2);
        pdf = fmaxf(1e-6f, ct * (1.0f / ENV_PI));
        wi = unit(q.fu * (cp * st) + q.fv * (sp * st) + q.fw * ct);
        pdf *= q.pD;
        if (q.pS > 0.0f) env_mix(pdf, env_ggx_pdf(q, wi), 1.0f - q.pD);
        return wi;
    }
    const V3 o = q.woln;
    if (!(o.z > 0.0f)) { pdf = 0.0f; wi = v3(0.0f, 0.0f, 0.0f); }
    else {
        const float al = q.alpha, a2 = al * al;
        const V3 vh = unit(v3(al * o.x, al * o.y, o.z));                                        // viewer on the unit hemisphere
        const V3 t1 = vh.z < 0.9999f ? unit(v3(-vh.y, vh.x, 0.0f)) : v3(1.0f, 0.0f, 0.0f);
        const V3 t2 = cross(vh, t1);
        float sp, cp;
        sincosf(2.0f * ENV_PI * u2, &sp, &cp);
        const float r = sqrtf(u1);
        const float p1 = r * cp;
        const float s = 0.5f * (1.0f + vh.z);
        const float p2 = (1.0f - s) * sqrtf(1.0f - p1 * p1) + s * (r * sp);
        const V3 nh = t1 * p1 + t2 * p2 + vh * sqrtf(fmaxf(0.0f, 1.0f - p1 * p1 - p2 * p2));
        const V3 h = unit(v3(al * nh.x, al * nh.y, fmaxf(0.0f, nh.z)));                         // back on the ellipsoid: the half vector
        const float oh = dot(o, h);
        pdf = env_g1(a2, o.z) * env_ndf(a2, h.z) * fmaxf(0.0f, oh) / o.z;
        pdf /= 4.0f * oh;
        const V3 l = h * (2.0f * oh) - o;
        wi = unit(q.fu * l.x + q.fv * l.y + q.fw * l.z);
    }
    pdf *= 1.0f - q.pD;
    if (q.pD > 0.0f) env_mix(pdf, fmaxf(dot(q.n, wi), 0.0f) * (1.0f / ENV_PI), q.pD);
    return wi;
}

// intermediate values of the specular term that forward and backward share
struct EnvSpec {
    V3 h, col, F;
    float a2, nv, nl, vh, nh, D, G, s, lam_v, lam_l;
    bool front;
};
__device__ __forceinline__ float env_lambda(float a2, float c)
{
    const float cc = env_clampc(c), c2 = cc * cc;
    return 0.5f * (sqrtf(1.0f + a2 * ((1.0f - c2) / c2)) - 1.0f);
}
__device__ __forceinline__ V3 env_specular(const EnvPoint& q, V3 wi, EnvSpec& e)
{
    const float al = fminf(fmaxf(q.alpha, ENV_MIN_ROUGHNESS * ENV_MIN_ROUGHNESS), 1.0f);
    e.a2 = al * al;
    e.h = unit(q.wo + wi);
    e.nv = dot(q.wo, q.n); e.nl = dot(wi, q.n); e.vh = dot(q.wo, e.h); e.nh = dot(q.n, e.h);
    e.col = (v3(0.04f, 0.04f, 0.04f) * (1.0f - q.ks.z) + q.kd * q.ks.z) * (1.0f - q.ks.x);
    e.front = e.nv > ENV_EPS && e.nl > ENV_EPS;
    if (!e.front) return v3(0.0f, 0.0f, 0.0f);
    e.D = env_ndf(e.a2, env_clampc(e.nh));
    e.lam_v = env_lambda(e.a2, e.nv); e.lam_l = env_lambda(e.a2, e.nl);
    e.G = 1.0f / (1.0f + e.lam_v + e.lam_l);
    e.s = env_pow5(1.0f - env_clampc(e.vh));
    e.F = e.col * (1.0f - e.s) + v3(e.s, e.s, e.s);
    return e.F * (e.D * e.G * 0.25f / e.nv);
}

struct EnvGrads { V3 pos, nrm, kd, ks; };

__device__ __forceinline__ bool env_open(float c) { return c > ENV_EPS && c < 1.0f - ENV_EPS; }      // the clamp passes a gradient

// adds the gradient of g . specular (the sample's direction held constant) to the point's gradients
__device__ __forceinline__ void env_specular_bwd(const EnvPoint& q, V3 wi, const EnvSpec& e, V3 g, EnvGrads& acc)
{
    if (!e.front) return;
    const float k = 0.25f / e.nv;
    const float gF = g.x * e.F.x + g.y * e.F.y + g.z * e.F.z;
    const V3 dF = g * (e.D * e.G * k);
    const float dD = gF * e.G * k, dG = gF * e.D * k;
    float d_nv = -gF * e.D * e.G * k / e.nv, d_nl = 0.0f, d_vh = 0.0f, d_nh = 0.0f, d_a2 = 0.0f;
    // Fresnel: F = col (1 - s) + s,  s = (1 - vh)^5
    const V3 d_col = dF * (1.0f - e.s);
    const float d_s = dF.x * (1.0f - e.col.x) + dF.y * (1.0f - e.col.y) + dF.z * (1.0f - e.col.z);
    if (e.vh >= ENV_EPS && e.vh < 1.0f - ENV_EPS) { const float t = 1.0f - e.vh, t2 = t * t; d_vh += d_s * -5.0f * t2 * t2; }
    // masking: G = 1 / (1 + lambda(nv) + lambda(nl)),  lambda = (sqrt(1 + a2 tan^2) - 1) / 2
    const float d_lam = -dG * e.G * e.G;
    {
        const float cv = env_clampc(e.nv), cl = env_clampc(e.nl);
        const float tv = (1.0f - cv * cv) / (cv * cv), tl = (1.0f - cl * cl) / (cl * cl);
        const float rv = sqrtf(1.0f + e.a2 * tv), rl = sqrtf(1.0f + e.a2 * tl);
        d_a2 += d_lam * 0.25f * (tv / rv + tl / rl);
        if (env_open(e.nv)) d_nv += d_lam * -0.5f * e.a2 / (cv * cv * cv * rv);
        if (env_open(e.nl)) d_nl += d_lam * -0.5f * e.a2 / (cl * cl * cl * rl);
    }
    // distribution: D = a2 / (pi d^2),  d = (a2 - 1) c^2 + 1
    {
        const float c = env_clampc(e.nh), c2 = c * c;
        const float d = (c * e.a2 - c) * c + 1.0f;
        const float id3 = 1.0f / (ENV_PI * d * d * d);
        d_a2 += dD * (1.0f - (e.a2 + 1.0f) * c2) * id3;
        if (env_open(e.nh)) d_nh += dD * -4.0f * (e.a2 - 1.0f) * e.a2 * e.nh * id3;
    }
    // the four cosines
    acc.nrm = acc.nrm + e.h * d_nh + wi * d_nl + q.wo * d_nv;
    const V3 d_h = q.n * d_nh + q.wo * d_vh;
    V3 d_wo = e.h * d_vh + q.n * d_nv;
    {                                                                                            // h = unit(wo + wi)
        const V3 s = q.wo + wi;
        const float l = sqrtf(dot(s, s));
        if (l > 0.0f) d_wo = d_wo + (d_h - e.h * dot(e.h, d_h)) * (1.0f / l);
    }
    if (q.wo_len > 0.0f) acc.pos = acc.pos - (d_wo - q.wo * dot(q.wo, d_wo)) * (1.0f / q.wo_len);  // wo = unit(view - pos)
    // materials: col = (0.04 (1 - m) + kd m) (1 - ks.x);  a2 = clamp(ks.y^2)^2
    const float m = q.ks.z, keep = 1.0f - q.ks.x;
    acc.kd = acc.kd + d_col * (m * keep);
    const V3 base = v3(0.04f, 0.04f, 0.04f) * (1.0f - m) + q.kd * m;
    acc.ks.x -= d_col.x * base.x + d_col.y * base.y + d_col.z * base.z;
    acc.ks.z += (d_col.x * (q.kd.x - 0.04f) + d_col.y * (q.kd.y - 0.04f) + d_col.z * (q.kd.z - 0.04f)) * keep;
    if (q.alpha > ENV_MIN_ROUGHNESS * ENV_MIN_ROUGHNESS) acc.ks.y += d_a2 * 2.0f * q.alpha * 2.0f * q.ks.y;
}

// ---- light_grad: merge within the wave, then atomics ---------------------------------------------------------------------------------
// Every lane of the wave calls this (key < 0: nothing to add).  In each round the first lane that still holds an add names its
// texel, the lanes with the same texel are summed, and the leader issues the three atomics.  What is left after `rounds` goes out
// lane by lane.
__device__ __forceinline__ void env_light_scatter(float* __restrict__ d_light, int key, V3 g, int rounds)
{
    const int lane = gs_lane_id();
    for (int r = 0; r < rounds; ++r) {
        const unsigned long long open = __ballot(key >= 0);
        if (open == 0ull) break;
        const int leader = __ffsll((long long)open) - 1;
        const int k = __builtin_amdgcn_readlane(key, leader);
        const bool mine = key == k;
        if (__popcll(__ballot(mine)) == 1) {                                                     // nothing shares it: no reduction
            if (mine) { gs_atomic_add(d_light + 3ll * k, g.x); gs_atomic_add(d_light + 3ll * k + 1, g.y); gs_atomic_add(d_light + 3ll * k + 2, g.z); }
        } else {
            const float s0 = gs_wave_sum(mine ? g.x : 0.0f), s1 = gs_wave_sum(mine ? g.y : 0.0f), s2 = gs_wave_sum(mine ? g.z : 0.0f);
            if (lane == leader) { gs_atomic_add(d_light + 3ll * k, s0); gs_atomic_add(d_light + 3ll * k + 1, s1); gs_atomic_add(d_light + 3ll * k + 2, s2); }
        }
        if (mine) key = -1;
    }
    if (key >= 0) { gs_atomic_add(d_light + 3ll * key, g.x); gs_atomic_add(d_light + 3ll * key + 1, g.y); gs_atomic_add(d_light + 3ll * key + 2, g.z); }
}

template <int G>
__device__ __forceinline__ float env_group_sum(float v)                                          // fixed order: the same bits every run
{
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- the kernel --------------------------------------------------------------------------------------------------------------------
template <int G, bool BWD, bool LOG>
static __global__ void __launch_bounds__(ENV_BLOCK) envshade_kernel(const EnvArgs a)
{
    const int sub = (int)threadIdx.x & (G - 1);
    const long long p = ((long long)blockIdx.x * ENV_BLOCK + threadIdx.x) / G;
    const bool in_range = p < a.P;
    const long long pc = in_range ? p : 0;
    const bool live = in_range && a.mask[pc] > 0.0f;
    EnvPoint q;
    q.ro = load3(a.ro, pc); q.pos = load3(a.pos, pc); q.n = load3(a.nrm, pc); q.kd = load3(a.kd, pc); q.ks = load3(a.ks, pc);
    env_point_setup(q, v3(a.view[0], a.view[1], a.view[2]));
    V3 gd = v3(0.0f, 0.0f, 0.0f), gs = gd;
    if (BWD) { gd = load3(a.d_diff, pc); gs = load3(a.d_spec, pc); }

    const int nn = a.n * a.n;
    const float strata = 1.0f / (float)a.n, frac = 1.0f / (float)nn;
    unsigned state = env_pcg_out(a.seed) ^ env_pcg_out((unsigned)pc);
    const long long light_row = (long long)(env_pcg_next(state) % (unsigned)a.T) * nn;
    const long long bsdf_row = (long long)(env_pcg_next(state) % (unsigned)a.T) * nn;
    if (G > 1) {
        unsigned m, c;
        env_lcg_jump(5u * (unsigned)sub, m, c);
        state = state * m + c;
    }

    V3 diff = v3(0.0f, 0.0f, 0.0f), spec = diff;
    float resi_d = 0.0f, resi_s = 0.0f;
    EnvGrads acc;
    acc.pos = acc.nrm = acc.kd = acc.ks = v3(0.0f, 0.0f, 0.0f);

    const int iters = (nn + G - 1) / G;
    for (int it = 0; it < iters; ++it) {
        const int i = it * G + sub;
        const bool act = live && i < nn;
        const int ic = i < nn ? i : 0;
        unsigned s = state;
        const float r0 = env_uniform(s), r1 = env_uniform(s), r2 = env_uniform(s), r3 = env_uniform(s), r4 = env_uniform(s);
        state = G > 1 ? state * a.jump_mul + a.jump_inc : s;
        const int pl = a.perms[light_row + ic], pb = a.perms[bsdf_row + ic];
        float lx, ly, bx, by;
        {
#pragma clang fp contract(off)
            lx = ((float)(pl % a.n) + r0) * strata; ly = ((float)(pl / a.n) + r1) * strata;
            bx = ((float)(pb % a.n) + r2) * strata; by = ((float)(pb / a.n) + r3) * strata;
        }
        const V3 dir_l = env_light_sample(a, lx, ly);
        float pdf_b;
        const V3 dir_b = env_bsdf_sample(q, bx, by, r4, pdf_b);
#pragma unroll 1
        for (int k = 0; k < 2; ++k) {
            const V3 dir = k ? dir_b : dir_l;
            int tx, ty;
            const float pdf_l = env_light_pdf(a, dir, tx, ty);
            const float pdf_sum = pdf_l + (k ? pdf_b : env_bsdf_pdf(q, dir));
            const int texel = ty * a.W + tx;
            const V3 lc = load3(a.light, texel);
            const float w = frac / fmaxf(pdf_sum, 1e-4f);
            const float lam = fmaxf(dot(q.n, dir) * (1.0f / ENV_PI), 0.0f);
            EnvSpec e;
            e.front = false;
            V3 sp = v3(0.0f, 0.0f, 0.0f);
            if (a.bsdf == 0) sp = env_specular(q, dir, e);
            bool occluded = false;
            if (act) {
                const BvhRay ray = bvh_make_ray(q.ro.x, q.ro.y, q.ro.z, dir.x, dir.y, dir.z);
                if (ray.valid) occluded = bvh_any_hit(ray, a.V, a.F, a.vertices, a.faces, a.nodes, 0.0f, ENV_TMAX);
            }
            const float vis = occluded ? 0.0f : 1.0f;
            const float V = vis * a.shadow_scale + (1.0f - a.shadow_scale);
            const float c = act ? V * w : 0.0f;
            if (!BWD) {
                diff = diff + lc * (lam * c);
                spec = spec + v3(sp.x * lc.x, sp.y * lc.y, sp.z * lc.z) * c;
                const float shadow = act ? (1.0f - V) * w : 0.0f;
                resi_d += lam * shadow;
                resi_s += (sp.x + sp.y + sp.z) * (1.0f / 3.0f) * shadow;
                if (LOG && act) {
                    const long long slot = (p * nn + i) * 2 + k;
                    a.log_dirs[3 * slot] = dir.x; a.log_dirs[3 * slot + 1] = dir.y; a.log_dirs[3 * slot + 2] = dir.z;
                    a.log_pdf[slot] = pdf_sum;
                    a.log_vis[slot] = vis;
                }
            } else {
                const V3 gl = v3(gd.x * lam + gs.x * sp.x, gd.y * lam + gs.y * sp.y, gd.z * lam + gs.z * sp.z) * c;
                const bool adds = c != 0.0f && (gl.x != 0.0f || gl.y != 0.0f || gl.z != 0.0f);
                env_light_scatter(a.d_light, adds ? texel : -1, gl, a.merge_rounds);
                if (c != 0.0f) {
                    const float g_lam = (gd.x * lc.x + gd.y * lc.y + gd.z * lc.z) * c;
                    if (dot(q.n, dir) > 0.0f) acc.nrm = acc.nrm + dir * (g_lam * (1.0f / ENV_PI));
                    if (a.bsdf == 0) env_specular_bwd(q, dir, e, v3(gs.x * lc.x, gs.y * lc.y, gs.z * lc.z) * c, acc);
                }
            }
        }
    }

    if (!BWD) {
        const float o0 = env_group_sum<G>(diff.x), o1 = env_group_sum<G>(diff.y), o2 = env_group_sum<G>(diff.z);
        const float o3 = env_group_sum<G>(spec.x), o4 = env_group_sum<G>(spec.y), o5 = env_group_sum<G>(spec.z);
        const float o6 = env_group_sum<G>(resi_d), o7 = env_group_sum<G>(resi_s);
        if (in_range && sub == 0) {
            a.diff[3 * p] = o0; a.diff[3 * p + 1] = o1; a.diff[3 * p + 2] = o2;
            a.spec[3 * p] = o3; a.spec[3 * p + 1] = o4; a.spec[3 * p + 2] = o5;
            a.resi[2 * p] = o6; a.resi[2 * p + 1] = o7;
        }
    } else {
        const V3 gp = v3(env_group_sum<G>(acc.pos.x), env_group_sum<G>(acc.pos.y), env_group_sum<G>(acc.pos.z));
        const V3 gn = v3(env_group_sum<G>(acc.nrm.x), env_group_sum<G>(acc.nrm.y), env_group_sum<G>(acc.nrm.z));
        const V3 gk = v3(env_group_sum<G>(acc.kd.x), env_group_sum<G>(acc.kd.y), env_group_sum<G>(acc.kd.z));
        const V3 gr = v3(env_group_sum<G>(acc.ks.x), env_group_sum<G>(acc.ks.y), env_group_sum<G>(acc.ks.z));
        if (in_range && sub == 0) {
            a.d_pos[3 * p] = gp.x; a.d_pos[3 * p + 1] = gp.y; a.d_pos[3 * p + 2] = gp.z;
            a.d_nrm[3 * p] = gn.x; a.d_nrm[3 * p + 1] = gn.y; a.d_nrm[3 * p + 2] = gn.z;
            a.d_kd[3 * p] = gk.x; a.d_kd[3 * p + 1] = gk.y; a.d_kd[3 * p + 2] = gk.z;
            a.d_ks[3 * p] = gr.x; a.d_ks[3 * p + 1] = gr.y; a.d_ks[3 * p + 2] = gr.z;
        }
    }
}

// ---- C-ABI -------------------------------------------------------------------------------------------------------------------------
static int env_steps(int size)                                                                   // ceil(log2(size - 1)) + 1 bisection steps
{
    int c = 0;
    while ((1ll << c) < (long long)size - 1) ++c;
    return c + 1;
}

static const char* env_check(int64_t P, const float* mask, const float* ro, const float* pos, const float* nrm, const float* view,
                             const float* kd, const float* ks, int H, int W, const float* light, const float* pdf, const float* rows,
                             const float* cols, int T, int n, const int32_t* perms, int64_t rnd_seed, int bsdf, int64_t V, int64_t F,
                             const float* vertices, const int32_t* faces, const void* bvh, int lanes_per_point)
{
    if (P < 0) return "negative P";
    if (P > ((int64_t)1 << 31) - 1) return "too many points: P must be below 2^31";
    if (H < 2 || W < 2) return "the light needs H >= 2 and W >= 2";
    if ((int64_t)H * W > ((int64_t)1 << 30)) return "light too large: H W must be at most 2^30";
    if (T < 1) return "perms needs T >= 1 tables";
    if (n < 1) return "n_samples_x must be at least 1";
    if (n > 1024) return "n_samples_x must be at most 1024";
    if (rnd_seed < 0 || rnd_seed >= ((int64_t)1 << 31)) return "rnd_seed must be in [0, 2^31)";
    if (bsdf < 0 || bsdf > 2) return "BSDF must be 0 (pbr), 1 (diffuse) or 2 (white)";
    if (F < 1) return "empty mesh: F must be at least 1";
    if (F > ((int64_t)1 << 30)) return "too many faces: at most 2^30";
    if (V < 1 || V > 2147483647ll) return "bad vertex count";
    if (lanes_per_point != 0 && lanes_per_point != 1 && lanes_per_point != 16 && lanes_per_point != 64)
        return "lanes_per_point must be 0 (default), 1, 16 or 64";
    if (vertices == nullptr || faces == nullptr || bvh == nullptr) return "vertices, faces and the node buffer must not be NULL";
    if (((uintptr_t)bvh & 15) != 0) return "node buffer must be 16-byte aligned";
    if (light == nullptr || pdf == nullptr || rows == nullptr || cols == nullptr || perms == nullptr)
        return "light, pdf, rows, cols and perms must not be NULL";
    if (P > 0 && (mask == nullptr || ro == nullptr || pos == nullptr || nrm == nullptr || view == nullptr || kd == nullptr || ks == nullptr))
        return "null point input";
    return nullptr;
}

// the default arrangement: a whole wave per point once it has an iteration for every lane (the fastest form measured at n = 8 and 16,
// DESIGN.md section 0, "Monte-Carlo environment shader"); below that the group shrinks with n^2 so that lanes are not left without work
static int env_default_lanes(int n) { return n >= 8 ? 64 : (n >= 4 ? 16 : 1); }

template <bool BWD, bool LOG>
static void env_launch(const EnvArgs& a, int lanes, hipStream_t s)
{
    const dim3 block(ENV_BLOCK);
    if (lanes == 1) hipLaunchKernelGGL((envshade_kernel<1, BWD, LOG>), dim3(gs_cdiv(a.P, ENV_BLOCK)), block, 0, s, a);
    else if (lanes == 16) hipLaunchKernelGGL((envshade_kernel<16, BWD, LOG>), dim3(gs_cdiv(a.P, ENV_BLOCK / 16)), block, 0, s, a);
    else hipLaunchKernelGGL((envshade_kernel<64, BWD, LOG>), dim3(gs_cdiv(a.P, ENV_BLOCK / 64)), block, 0, s, a);
}

static EnvArgs env_args(int64_t P, const float* mask, const float* ro, const float* pos, const float* nrm, const float* view,
                        const float* kd, const float* ks, int H, int W, const float* light, const float* pdf, const float* rows,
                        const float* cols, int T, int n, const int32_t* perms, int64_t rnd_seed, int bsdf, float shadow_scale, int64_t V,
                        int64_t F, const float* vertices, const int32_t* faces, const void* bvh, int lanes)
{
    EnvArgs a = {};
    a.P = P; a.mask = mask; a.ro = ro; a.pos = pos; a.nrm = nrm; a.view = view; a.kd = kd; a.ks = ks;
    a.H = H; a.W = W; a.row_steps = env_steps(H); a.col_steps = env_steps(W);
    a.light = light; a.pdf = pdf; a.rows = rows; a.cols = cols;
    a.T = T; a.n = n; a.perms = perms; a.seed = (unsigned)rnd_seed;
    env_lcg_jump(5u * (unsigned)lanes, a.jump_mul, a.jump_inc);
    a.bsdf = bsdf; a.shadow_scale = shadow_scale;
    a.V = V; a.F = F; a.vertices = vertices; a.faces = faces; a.nodes = (const BvhNode*)bvh;
    return a;
}

extern "C" int gs_envshade_fwd(int64_t P, const float* mask, const float* ro, const float* gb_pos, const float* gb_normal,
                               const float* view_pos, const float* gb_kd, const float* gb_ks, int H, int W, const float* light,
                               const float* pdf, const float* rows, const float* cols, int T, int n_samples_x, const int32_t* perms,
                               int64_t rnd_seed, int bsdf, float shadow_scale, int64_t V, int64_t F, const float* vertices,
                               const int32_t* faces, const void* bvh, int lanes_per_point, float* diff, float* spec, float* resi,
                               float* log_dirs, float* log_pdf_sum, float* log_vis, void* stream)
{
    const char* msg = env_check(P, mask, ro, gb_pos, gb_normal, view_pos, gb_kd, gb_ks, H, W, light, pdf, rows, cols, T, n_samples_x, perms,
                                rnd_seed, bsdf, V, F, vertices, faces, bvh, lanes_per_point);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    if (P == 0) return GS_OK;
    GS_CHECK_ARG(diff != nullptr && spec != nullptr && resi != nullptr, "null output");
    const bool log = log_dirs != nullptr || log_pdf_sum != nullptr || log_vis != nullptr;
    GS_CHECK_ARG(!log || (log_dirs != nullptr && log_pdf_sum != nullptr && log_vis != nullptr), "the sample log needs all three buffers");
    GS_CHECK_ARG(!log || P <= (((int64_t)1 << 40) / ((int64_t)n_samples_x * n_samples_x)), "sample log too large");
    const int lanes = lanes_per_point ? lanes_per_point : env_default_lanes(n_samples_x);
    EnvArgs a = env_args(P, mask, ro, gb_pos, gb_normal, view_pos, gb_kd, gb_ks, H, W, light, pdf, rows, cols, T, n_samples_x, perms, rnd_seed,
                         bsdf, shadow_scale, V, F, vertices, faces, bvh, lanes);
    a.diff = diff; a.spec = spec; a.resi = resi;
    a.log_dirs = log_dirs; a.log_pdf = log_pdf_sum; a.log_vis = log_vis;
    if (log) env_launch<false, true>(a, lanes, (hipStream_t)stream);
    else env_launch<false, false>(a, lanes, (hipStream_t)stream);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_envshade_bwd(int64_t P, const float* mask, const float* ro, const float* gb_pos, const float* gb_normal,
                               const float* view_pos, const float* gb_kd, const float* gb_ks, int H, int W, const float* light,
                               const float* pdf, const float* rows, const float* cols, int T, int n_samples_x, const int32_t* perms,
                               int64_t rnd_seed, int bsdf, float shadow_scale, int64_t V, int64_t F, const float* vertices,
                               const int32_t* faces, const void* bvh, int lanes_per_point, int merge_rounds, const float* diff_grad,
                               const float* spec_grad, float* gb_pos_grad, float* gb_normal_grad, float* gb_kd_grad, float* gb_ks_grad,
                               float* light_grad, void* stream)
{
    const char* msg = env_check(P, mask, ro, gb_pos, gb_normal, view_pos, gb_kd, gb_ks, H, W, light, pdf, rows, cols, T, n_samples_x, perms,
                                rnd_seed, bsdf, V, F, vertices, faces, bvh, lanes_per_point);
    if (msg) { gs_set_error("%s: %s", __func__, msg); return GS_EINVAL; }
    GS_CHECK_ARG(merge_rounds >= -1 && merge_rounds <= 64, "merge_rounds must be -1 (default) or 0..64");
    if (P == 0) return GS_OK;
    GS_CHECK_ARG(diff_grad != nullptr && spec_grad != nullptr, "null output gradient");
    GS_CHECK_ARG(gb_pos_grad != nullptr && gb_normal_grad != nullptr && gb_kd_grad != nullptr && gb_ks_grad != nullptr && light_grad != nullptr,
                 "null gradient buffer");
    const int lanes = lanes_per_point ? lanes_per_point : env_default_lanes(n_samples_x);
    EnvArgs a = env_args(P, mask, ro, gb_pos, gb_normal, view_pos, gb_kd, gb_ks, H, W, light, pdf, rows, cols, T, n_samples_x, perms, rnd_seed,
                         bsdf, shadow_scale, V, F, vertices, faces, bvh, lanes);
    a.d_diff = diff_grad; a.d_spec = spec_grad;
    a.d_pos = gb_pos_grad; a.d_nrm = gb_normal_grad; a.d_kd = gb_kd_grad; a.d_ks = gb_ks_grad; a.d_light = light_grad;
    a.merge_rounds = merge_rounds < 0 ? 4 : merge_rounds;
    env_launch<true, false>(a, lanes, (hipStream_t)stream);
    GS_CHECK_LAUNCH();
    return GS_OK;
}
