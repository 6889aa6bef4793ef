/*
 * gs_oracle_shade.c -- CPU ORACLE (test infrastructure, NOT product code).
 *
 * Plain-C restatement of the per-Gaussian split-sum shading of the
 * GeoSplatting hot path (stages S1..S3 of SURVEY.md section 8a):
 *   S1  RenderableAttrs.splat arithmetic  rfstudio/model/geosplat.py:80-122
 *   S2  FG-LUT lookup (nvdiffrast dr.texture, 2-D, 'linear', 'clamp')
 *                                         rfstudio/model/geosplat.py:93-98
 *   S3  TextureSplitSum.sample            rfstudio/graphics/_mesh/_texture.py:571-613
 *       (dr.texture cube 'linear' on `base`, cube 'linear-mipmap-linear'
 *        on the specular pyramid with mip_level_bias = f(roughness))
 *
 * PARITY UNPINNED for the texture fetches: nvdiffrast is an un-vendored,
 * unpinned third-party dependency (README.md:36) and the reference holds no
 * golden vectors for it.  The S1 arithmetic and the roughness->mip map are
 * pinned against the importable reference Python (tests/golden/, generated
 * by scripts/make_golden.py).  Cube-map semantics restated here:
 *   - face order +x,-x,+y,-y,+z,-z with the (x,y) parameterisation of
 *     _cube_to_dir (rfstudio/graphics/_mesh/_texture.py:178-197) ==
 *     cube_to_dir (.../_splitsum/c_src/cubemap.cu:32-46); texel (ix,iy)
 *     centre at x = 2(ix+0.5)/R - 1;
 *   - bilinear footprint; a texel that falls over ONE face edge is taken
 *     from the adjacent face (re-projection of its centre, nearest texel);
 *     a texel over TWO edges (cube corner) does not exist: it takes the mean
 *     of the other three (the GL seamless-cube-map rule);
 *   - trilinear between floor(level) and floor(level)+1 with
 *     level = clamp(mip_level_bias, 0, L-1) (no uv derivatives are supplied
 *     by the reference, so the bias alone selects the level).
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "gs_oracle_ev.h"

#define GSO_API __attribute__((visibility("default")))

/* ---------------- 2-D bilinear, clamp (S2) ------------------------------- */
/* lut layout [H][W][C]; u -> width axis, v -> height axis. */
static void tex2d_linear_clamp(const float* lut, int W, int H, int C, float u, float v,
                               float* out, float* d_du, float* d_dv)
{
    float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    int cx = 0, cy = 0;
    if (x < 0.0f) { x = 0.0f; cx = 1; } else if (x > (float)(W - 1)) { x = (float)(W - 1); cx = 1; }
    if (y < 0.0f) { y = 0.0f; cy = 1; } else if (y > (float)(H - 1)) { y = (float)(H - 1); cy = 1; }
    int ix0 = (int)floorf(x), iy0 = (int)floorf(y);
    float fx = x - (float)ix0, fy = y - (float)iy0;
    int ix1 = ix0 + 1 < W ? ix0 + 1 : W - 1;
    int iy1 = iy0 + 1 < H ? iy0 + 1 : H - 1;
    for (int c = 0; c < C; ++c) {
        float t00 = lut[((size_t)iy0 * W + ix0) * C + c], t10 = lut[((size_t)iy0 * W + ix1) * C + c];
        float t01 = lut[((size_t)iy1 * W + ix0) * C + c], t11 = lut[((size_t)iy1 * W + ix1) * C + c];
        float top = t00 + fx * (t10 - t00);
        float bot = t01 + fx * (t11 - t01);
        out[c] = top + fy * (bot - top);
        if (d_du) d_du[c] = cx ? 0.0f : (float)W * ((t10 - t00) + fy * ((t11 - t01) - (t10 - t00)));
        if (d_dv) d_dv[c] = cy ? 0.0f : (float)H * (bot - top);
    }
}

/* ---------------- cube map (S3) ------------------------------------------ */
typedef struct {
    int face;
    int a, b, c;        /* component indices: x_ndc = sx*d[a]/|d[c]|, y_ndc = sy*d[b]/|d[c]| */
    float sx, sy;
} face_map;

static const face_map FACES[6] = {
    { 0, 2, 1, 0, -1.0f, -1.0f },   /* +x: (1,-y,-x) */
    { 1, 2, 1, 0,  1.0f, -1.0f },   /* -x: (-1,-y,x) */
    { 2, 0, 2, 1,  1.0f,  1.0f },   /* +y: (x,1,y)   */
    { 3, 0, 2, 1,  1.0f, -1.0f },   /* -y: (x,-1,-y) */
    { 4, 0, 1, 2,  1.0f, -1.0f },   /* +z: (x,-y,1)  */
    { 5, 0, 1, 2, -1.0f, -1.0f },   /* -z: (-x,-y,-1)*/
};

static int select_face(const float* d)
{
    float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    int f;
    float c;
    if (az > fmaxf(ax, ay)) { f = 4; c = d[2]; }
    else if (ay > ax)       { f = 2; c = d[1]; }
    else                    { f = 0; c = d[0]; }
    if (c < 0.0f) f += 1;
    return f;
}

static void face_point(int s, float x, float y, float* p)
{
    switch (s) {
    case 0: p[0] = 1.0f;  p[1] = -y;    p[2] = -x;    break;
    case 1: p[0] = -1.0f; p[1] = -y;    p[2] = x;     break;
    case 2: p[0] = x;     p[1] = 1.0f;  p[2] = y;     break;
    case 3: p[0] = x;     p[1] = -1.0f; p[2] = -y;    break;
    case 4: p[0] = x;     p[1] = -y;    p[2] = 1.0f;  break;
    default: p[0] = -x;   p[1] = -y;    p[2] = -1.0f; break;
    }
}

/* resolve texel (ix,iy) of face s (each may be one step outside [0,R-1]);
 * returns linear index face*R*R + y*R + x, or -1 for a cube corner. */
static int resolve_texel(int s, int ix, int iy, int R)
{
    int ox = (ix < 0 || ix >= R), oy = (iy < 0 || iy >= R);
    if (!ox && !oy) return (s * R + iy) * R + ix;
    if (ox && oy) return -1;
    float xn = 2.0f * (((float)ix + 0.5f) / (float)R) - 1.0f;
    float yn = 2.0f * (((float)iy + 0.5f) / (float)R) - 1.0f;
    float p[3];
    face_point(s, xn, yn, p);
    int s2 = select_face(p);
    const face_map* m = &FACES[s2];
    float inv = 1.0f / fabsf(p[m->c]);
    float x2 = m->sx * p[m->a] * inv, y2 = m->sy * p[m->b] * inv;
    float tx = (x2 + 1.0f) * 0.5f * (float)R - 0.5f, ty = (y2 + 1.0f) * 0.5f * (float)R - 0.5f;
    int jx = (int)floorf(tx + 0.5f), jy = (int)floorf(ty + 0.5f);
    if (jx < 0) jx = 0; if (jx > R - 1) jx = R - 1;
    if (jy < 0) jy = 0; if (jy > R - 1) jy = R - 1;
    return (s2 * R + jy) * R + jx;
}

typedef struct {
    int valid;           /* 0 -> zero direction: output 0, no grads */
    int idx[4];          /* texel linear indices (00,10,01,11); -1 = corner-missing */
    float w[4];          /* effective weights (missing weight redistributed) */
    float fx, fy;
    int face;
    float inv_c;         /* 1/|d[c]| */
    float xn, yn;        /* face coords in [-1,1] */
    int ix0, iy0;        /* texel of the footprint's first tap (may be -1: over the face edge) */
} cube_fp;

static void cube_footprint(const float* d, int R, cube_fp* fp)
{
    int s = select_face(d);
    const face_map* m = &FACES[s];
    float ac = fabsf(d[m->c]);
    fp->valid = (ac > 0.0f) && isfinite(ac);
    fp->face = s;
    if (!fp->valid) return;
    float inv = 1.0f / ac;
    float xn = m->sx * d[m->a] * inv, yn = m->sy * d[m->b] * inv;
    fp->inv_c = inv; fp->xn = xn; fp->yn = yn;
    float tx = (xn + 1.0f) * 0.5f * (float)R - 0.5f, ty = (yn + 1.0f) * 0.5f * (float)R - 0.5f;
    int ix0 = (int)floorf(tx), iy0 = (int)floorf(ty);
    float fx = tx - (float)ix0, fy = ty - (float)iy0;
    fp->fx = fx; fp->fy = fy; fp->ix0 = ix0; fp->iy0 = iy0;
    fp->idx[0] = resolve_texel(s, ix0, iy0, R);
    fp->idx[1] = resolve_texel(s, ix0 + 1, iy0, R);
    fp->idx[2] = resolve_texel(s, ix0, iy0 + 1, R);
    fp->idx[3] = resolve_texel(s, ix0 + 1, iy0 + 1, R);
    float w[4] = { (1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy };
    int miss = -1;
    for (int i = 0; i < 4; ++i) if (fp->idx[i] < 0) miss = i;
    for (int i = 0; i < 4; ++i) fp->w[i] = w[i];
    if (miss >= 0) {
        float wm = w[miss] / 3.0f;
        for (int i = 0; i < 4; ++i) fp->w[i] = (i == miss) ? 0.0f : w[i] + wm;
    }
}

/* bilinear cube fetch of 3 channels; optionally d out / d direction (3x3: dd[c*3+k]) */
static void cube_fetch(const float* tex, int R, const float* d, float* out, float* dd /*nullable [9]*/, cube_fp* fp_out)
{
    cube_fp fp;
    cube_footprint(d, R, &fp);
    if (fp_out) *fp_out = fp;
    if (!fp.valid) {
        out[0] = out[1] = out[2] = 0.0f;
        if (dd) memset(dd, 0, sizeof(float) * 9);
        return;
    }
    float t[4][3];
    int miss = -1;
    for (int i = 0; i < 4; ++i) {
        if (fp.idx[i] < 0) { miss = i; continue; }
        for (int c = 0; c < 3; ++c) t[i][c] = tex[(size_t)fp.idx[i] * 3 + c];
    }
    if (miss >= 0)
        for (int c = 0; c < 3; ++c) {
            float s = 0.0f;
            for (int i = 0; i < 4; ++i) if (i != miss) s += t[i][c];
            t[miss][c] = s / 3.0f;
        }
    const face_map* m = &FACES[fp.face];
    float sgn_c = d[m->c] < 0.0f ? -1.0f : 1.0f;
    for (int c = 0; c < 3; ++c) {
        float top = t[0][c] + fp.fx * (t[1][c] - t[0][c]);
        float bot = t[2][c] + fp.fx * (t[3][c] - t[2][c]);
        out[c] = top + fp.fy * (bot - top);
        if (dd) {
            float dtx = (t[1][c] - t[0][c]) + fp.fy * ((t[3][c] - t[2][c]) - (t[1][c] - t[0][c]));
            float dty = bot - top;
            float gx = dtx * 0.5f * (float)R, gy = dty * 0.5f * (float)R;   /* d/dxn, d/dyn */
            float g[3] = { 0.0f, 0.0f, 0.0f };
            g[m->a] += gx * m->sx * fp.inv_c;
            g[m->b] += gy * m->sy * fp.inv_c;
            g[m->c] += -(gx * fp.xn + gy * fp.yn) * fp.inv_c * sgn_c;
            dd[c * 3 + 0] = g[0]; dd[c * 3 + 1] = g[1]; dd[c * 3 + 2] = g[2];
        }
    }
}

static void cube_scatter(float* grad_tex, const cube_fp* fp, const float* g /*[3]*/, float scale)
{
    if (!fp->valid) return;
    for (int i = 0; i < 4; ++i) {
        if (fp->idx[i] < 0) continue;
        for (int c = 0; c < 3; ++c) {
            float v = g[c] * scale * fp->w[i];       /* (callers scatter inside an ordered region: one thread at a time) */
            grad_tex[(size_t)fp->idx[i] * 3 + c] += v;
        }
    }
}

/* roughness -> mip level (rfstudio/graphics/_mesh/_texture.py:584-594) */
static float mip_from_roughness(float r, float min_r, float max_r, int L, float* dmip_dr)
{
    float m, dm;
    if (r < max_r) {
        float t = (r - min_r) / (max_r - min_r);
        int inside = (t >= 0.0f && t <= 1.0f);
        t = fminf(fmaxf(t, 0.0f), 1.0f);
        m = t * (float)(L - 2);
        dm = inside ? (float)(L - 2) / (max_r - min_r) : 0.0f;
    } else {
        float t = (r - max_r) / (1.0f - max_r);
        int inside = (t >= 0.0f && t <= 1.0f);
        t = fminf(fmaxf(t, 0.0f), 1.0f);
        m = t + (float)(L - 2);
        dm = inside ? 1.0f / (1.0f - max_r) : 0.0f;
    }
    if (dmip_dr) *dmip_dr = dm;
    return m;
}

typedef struct {
    float out[3];
    float dd[9];         /* d out_c / d dir_k */
    float dmip[3];       /* d out_c / d level */
    cube_fp fp0, fp1;
    float f;             /* blend weight of level l1 */
    int l0, l1;          /* l1 = -1 when single level */
} mip_sample;

static void cube_mip_fetch(const float* const* levels, const int* res, int L, const float* d, float bias, mip_sample* s)
{
    float lam = fminf(fmaxf(bias, 0.0f), (float)(L - 1));
    int l0 = (int)floorf(lam);
    if (l0 >= L - 1) {
        s->l0 = L - 1; s->l1 = -1; s->f = 0.0f;
        cube_fetch(levels[L - 1], res[L - 1], d, s->out, s->dd, &s->fp0);
        s->dmip[0] = s->dmip[1] = s->dmip[2] = 0.0f;
        return;
    }
    float f = lam - (float)l0;
    float c0[3], c1[3], dd0[9], dd1[9];
    cube_fetch(levels[l0], res[l0], d, c0, dd0, &s->fp0);
    cube_fetch(levels[l0 + 1], res[l0 + 1], d, c1, dd1, &s->fp1);
    s->l0 = l0; s->l1 = l0 + 1; s->f = f;
    int clamped = (bias < 0.0f || bias > (float)(L - 1));
    for (int c = 0; c < 3; ++c) {
        s->out[c] = c0[c] + f * (c1[c] - c0[c]);
        s->dmip[c] = clamped ? 0.0f : (c1[c] - c0[c]);
        for (int k = 0; k < 3; ++k) s->dd[c * 3 + k] = dd0[c * 3 + k] + f * (dd1[c * 3 + k] - dd0[c * 3 + k]);
    }
}

/* ---------------- S1: per-Gaussian shading ------------------------------- */
typedef struct {
    float rough, metal, spec[3], diff[3];
    float wo[3], len; int wo_const;
    float d, ndv;
    float fg[2], dfg_du[2], dfg_dv[2];
    float refl[3];
    float mip, dmip_dr;
    mip_sample ls;
    float ld[3], ld_dd[9]; cube_fp ld_fp;
    float refl_c[3];   /* reflectance */
} shade_tmp;

static void shade_one(const float* mean, const float* normal, const float* kd, const float* ks, const float* cam_pos,
                      float min_roughness, float max_metallic, int mode,
                      const float* lut, int lut_res, const float* base, int base_res,
                      const float* const* levels, const int* res, int L, float env_min_r, float env_max_r,
                      float* color, shade_tmp* t)
{
    t->rough = ks[0] * (1.0f - min_roughness) + min_roughness;
    t->metal = ks[1] * max_metallic;
    for (int c = 0; c < 3; ++c) {
        t->spec[c] = (1.0f - t->metal) * 0.04f + kd[c] * t->metal;
        t->diff[c] = kd[c] * (1.0f - t->metal);
    }
    /* safe_normalize (rfstudio/graphics/math.py:119-125) */
    float v[3] = { cam_pos[0] - mean[0], cam_pos[1] - mean[1], cam_pos[2] - mean[2] };
    float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    t->len = len;
    if (len < 1e-6f) { t->wo[0] = 0.0f; t->wo[1] = 0.0f; t->wo[2] = 1.0f; t->wo_const = 1; }
    else { float l = fmaxf(len, 1e-6f); t->wo[0] = v[0] / l; t->wo[1] = v[1] / l; t->wo[2] = v[2] / l; t->wo_const = 0; }
    t->d = (normal[0] * t->wo[0] + normal[1] * t->wo[1]) + normal[2] * t->wo[2];
    t->ndv = fmaxf(t->d, 1e-6f);
    tex2d_linear_clamp(lut, lut_res, lut_res, 2, t->ndv, t->rough, t->fg, t->dfg_du, t->dfg_dv);
    for (int k = 0; k < 3; ++k) t->refl[k] = 2.0f * t->d * normal[k] - t->wo[k];
    t->mip = mip_from_roughness(t->rough, env_min_r, env_max_r, L, &t->dmip_dr);
    cube_mip_fetch(levels, res, L, t->refl, t->mip, &t->ls);
    cube_fetch(base, base_res, normal, t->ld, t->ld_dd, &t->ld_fp);
    for (int c = 0; c < 3; ++c) {
        t->refl_c[c] = t->spec[c] * t->fg[0] + t->fg[1];
        if (mode == 0)      color[c] = t->diff[c] + t->ls.out[c] * t->refl_c[c];   /* 'pbr'      geosplat.py:111-115 */
        else if (mode == 1) color[c] = t->ld[c] * t->diff[c];                      /* 'diffuse'  geosplat.py:116-117 */
        else                color[c] = t->ls.out[c] * t->refl_c[c];                /* 'specular' geosplat.py:118-119 */
    }
}

GSO_API void gso_shade_fwd(int N, const float* means, const float* normals, const float* kd, const float* ks,
                           const float* cam_pos, float min_roughness, float max_metallic, int mode,
                           const float* lut, int lut_res, const float* base, int base_res,
                           const float* const* levels, const int* res, int L, float env_min_r, float env_max_r,
                           float* colors)
{
#pragma omp parallel for schedule(static)
    for (int n = 0; n < N; ++n) {
        shade_tmp t;
        shade_one(means + 3 * (size_t)n, normals + 3 * (size_t)n, kd + 3 * (size_t)n, ks + 2 * (size_t)n, cam_pos,
                  min_roughness, max_metallic, mode, lut, lut_res, base, base_res, levels, res, L,
                  env_min_r, env_max_r, colors + 3 * (size_t)n, &t);
    }
}

/* ---------------- error budget of the backward (gso_shade_bwd_budget) ----- */
/* The statements of shade_one and of the chain rule below it once more in the running-error arithmetic of gs_oracle_ev.h:
 * every SELECTION (LUT cell and clamp flags, mip segment / inside / levels / clamped, face, the texels of a footprint, the
 * d and len thresholds) is taken from the fp32 evaluation `t`, everything smooth is re-evaluated as (value, error bound).
 * The constant 0.04f carries what it differs from 0.04 by, so that the budget also covers exact arithmetic (float64
 * autograd); every other input is exact.
 *
 * margins [N][GSO_SHADE_MARGINS][2] = (distance of a selecting quantity to its nearest decision boundary, forward
 * running-error bound of that quantity, both in the quantity's own units); an unused slot holds (inf, 0):
 *    0 len vs 1e-6             1 d vs 1e-6            2 LUT x vs cell edges / clamp ends     3 LUT y likewise
 *    4 roughness vs env_min_r, env_max_r, 1           5 mip level vs the integers (unclamped only)
 *    6, 7, 8    level l0: |major axis| - |largest other| (face), tx and ty vs the integers
 *    9, 10, 11  level l1 likewise                    12, 13, 14  diffuse base likewise
 * A texel element collects, per contribution, the contribution's own bound (b), its magnitude (a) and a count (n): the
 * budget is b + (n - 1) a, whatever order the n values are summed in. */
#define GSO_SHADE_MARGINS 15
typedef struct {
    double *b_means, *b_normals, *b_kd, *b_ks;
    double *b_base; double* const* b_levels;
    double *a_base; double** a_levels;
    int32_t *n_base; int32_t** n_levels;
    double *margins;
} shade_budget_out;

typedef struct { gso_ev out[3], dd[9], w[4]; double mg[6]; } ev_cube;

static inline double near_int(double x) { return fabs(x - floor(x + 0.5)); }

static void ev_cube_fetch(const float* tex, int R, const gso_ev* d, const cube_fp* fp, ev_cube* o)
{
    const gso_ev zero = ev_in(0.0), one = ev_in(1.0);
    for (int i = 0; i < 3; ++i) o->out[i] = zero;
    for (int i = 0; i < 9; ++i) o->dd[i] = zero;
    for (int i = 0; i < 4; ++i) o->w[i] = zero;
    for (int i = 0; i < 3; ++i) { o->mg[2 * i] = INFINITY; o->mg[2 * i + 1] = 0.0; }
    if (!fp->valid) return;
    const face_map* m = &FACES[fp->face];
    const double sgn = (fp->face & 1) ? -1.0 : 1.0;
    const gso_ev ac = ev_scale(d[m->c], sgn);
    const gso_ev inv = ev_div(one, ac);
    const gso_ev xn = ev_mul(ev_scale(d[m->a], m->sx), inv), yn = ev_mul(ev_scale(d[m->b], m->sy), inv);
    const gso_ev Rf = ev_in((double)R), half = ev_in(0.5);
    const gso_ev tx = ev_sub(ev_mul(ev_scale(ev_add(xn, one), 0.5), Rf), half);
    const gso_ev ty = ev_sub(ev_mul(ev_scale(ev_add(yn, one), 0.5), Rf), half);
    const gso_ev fx = ev_sub(tx, ev_in((double)fp->ix0)), fy = ev_sub(ty, ev_in((double)fp->iy0));
    {
        const double oa = fabs(d[m->a].v), ob = fabs(d[m->b].v);
        o->mg[0] = fabs(ac.v) - (oa > ob ? oa : ob);
        o->mg[1] = (ac.e + (d[m->a].e > d[m->b].e ? d[m->a].e : d[m->b].e)) * GSO_EPS;
        o->mg[2] = floor(tx.v) == (double)fp->ix0 ? near_int(tx.v) : 0.0; o->mg[3] = tx.e * GSO_EPS;
        o->mg[4] = floor(ty.v) == (double)fp->iy0 ? near_int(ty.v) : 0.0; o->mg[5] = ty.e * GSO_EPS;
    }
    gso_ev T[4][3];
    int miss = -1;
    for (int i = 0; i < 4; ++i) {
        if (fp->idx[i] < 0) { miss = i; continue; }
        for (int c = 0; c < 3; ++c) T[i][c] = ev_in((double)tex[(size_t)fp->idx[i] * 3 + c]);
    }
    if (miss >= 0)
        for (int c = 0; c < 3; ++c) {
            gso_ev s = zero;
            for (int i = 0; i < 4; ++i) if (i != miss) s = ev_add(s, T[i][c]);
            T[miss][c] = ev_div(s, ev_in(3.0));
        }
    for (int c = 0; c < 3; ++c) {
        const gso_ev d10 = ev_sub(T[1][c], T[0][c]), d32 = ev_sub(T[3][c], T[2][c]);
        const gso_ev top = ev_add(T[0][c], ev_mul(fx, d10)), bot = ev_add(T[2][c], ev_mul(fx, d32));
        const gso_ev dty = ev_sub(bot, top);
        o->out[c] = ev_add(top, ev_mul(fy, dty));
        const gso_ev dtx = ev_add(d10, ev_mul(fy, ev_sub(d32, d10)));
        const gso_ev gx = ev_mul(ev_scale(dtx, 0.5), Rf), gy = ev_mul(ev_scale(dty, 0.5), Rf);
        o->dd[c * 3 + m->a] = ev_mul(ev_scale(gx, m->sx), inv);
        o->dd[c * 3 + m->b] = ev_mul(ev_scale(gy, m->sy), inv);
        o->dd[c * 3 + m->c] = ev_scale(ev_mul(ev_add(ev_mul(gx, xn), ev_mul(gy, yn)), inv), -sgn);
    }
    const gso_ev omx = ev_sub(one, fx), omy = ev_sub(one, fy);
    gso_ev w[4] = { ev_mul(omx, omy), ev_mul(fx, omy), ev_mul(omx, fy), ev_mul(fx, fy) };
    if (miss >= 0) {
        const gso_ev wm = ev_div(w[miss], ev_in(3.0));
        for (int i = 0; i < 4; ++i) w[i] = (i == miss) ? zero : ev_add(w[i], wm);
    }
    for (int i = 0; i < 4; ++i) o->w[i] = w[i];
}

static void ev_scatter(double* b, double* a, int32_t* cnt, const cube_fp* fp, const ev_cube* e, const gso_ev* g, gso_ev scale)
{
    if (!fp->valid) return;
    for (int i = 0; i < 4; ++i) {
        if (fp->idx[i] < 0) continue;
        for (int c = 0; c < 3; ++c) {
            const gso_ev v = ev_mul(ev_mul(g[c], scale), e->w[i]);
            if (v.v == 0.0 && v.e == 0.0) continue;
            const size_t k = (size_t)fp->idx[i] * 3 + c;
            const double av = fabs(v.v);
#pragma omp atomic
            b[k] += v.e;
#pragma omp atomic
            a[k] += av;
#pragma omp atomic
            cnt[k] += 1;
        }
    }
}

/* bilinear LUT axis: the clamped coordinate as the fp32 path selected it, its cell, and the margin of that selection */
static gso_ev ev_lut_axis(gso_ev u, float u_f, int W, int* clamped, int* i0, int* i1, double* mg)
{
    gso_ev x = ev_sub(ev_mul(u, ev_in((double)W)), ev_in(0.5));
    float xf = u_f * (float)W - 0.5f;
    *clamped = 0;
    mg[1] = x.e * GSO_EPS;
    if (xf < 0.0f) { mg[0] = fabs(x.v); xf = 0.0f; x = ev_in(0.0); *clamped = 1; }
    else if (xf > (float)(W - 1)) { mg[0] = fabs(x.v - (double)(W - 1)); xf = (float)(W - 1); x = ev_in((double)(W - 1)); *clamped = 1; }
    else mg[0] = floor(x.v) == (double)floorf(xf) ? near_int(x.v) : 0.0;
    *i0 = (int)floorf(xf);
    *i1 = *i0 + 1 < W ? *i0 + 1 : W - 1;
    return ev_sub(x, ev_in((double)*i0));
}

static void shade_budget_gauss(int n, const float* mean, const float* normal, const float* kd, const float* ks, const float* cam_pos,
                               float min_roughness, float max_metallic, int mode, const float* lut, int lut_res,
                               const float* base, int base_res, const float* const* levels, const int* res, int L,
                               float env_min_r, float env_max_r, const float* g, const shade_tmp* t, shade_budget_out* B)
{
    const gso_ev zero = ev_in(0.0), one = ev_in(1.0);
    double mgs[GSO_SHADE_MARGINS][2];
    for (int i = 0; i < GSO_SHADE_MARGINS; ++i) { mgs[i][0] = INFINITY; mgs[i][1] = 0.0; }
    gso_ev nrm[3], kdv[3], gv[3];
    for (int k = 0; k < 3; ++k) { nrm[k] = ev_in(normal[k]); kdv[k] = ev_in(kd[k]); gv[k] = ev_in(g[k]); }
    /* ---- forward */
    const gso_ev minr = ev_in(min_roughness), maxm = ev_in(max_metallic);
    const gso_ev omr = ev_sub(one, minr);
    const gso_ev rough = ev_add(ev_mul(ev_in(ks[0]), omr), minr);
    const gso_ev metal = ev_mul(ev_in(ks[1]), maxm);
    const gso_ev omm = ev_sub(one, metal);
    const gso_ev c004 = ev_err((double)0.04f, 0.02);
    gso_ev spec[3], diff[3];
    for (int c = 0; c < 3; ++c) { spec[c] = ev_add(ev_mul(omm, c004), ev_mul(kdv[c], metal)); diff[c] = ev_mul(kdv[c], omm); }
    gso_ev v[3], wo[3];
    for (int k = 0; k < 3; ++k) v[k] = ev_sub(ev_in(cam_pos[k]), ev_in(mean[k]));
    const gso_ev len = ev_sqrt(ev_add(ev_add(ev_mul(v[0], v[0]), ev_mul(v[1], v[1])), ev_mul(v[2], v[2])));
    mgs[0][0] = fabs(len.v - (double)1e-6f); mgs[0][1] = len.e * GSO_EPS;
    if (t->wo_const) { wo[0] = zero; wo[1] = zero; wo[2] = one; }
    else for (int k = 0; k < 3; ++k) wo[k] = ev_div(v[k], len);
    const gso_ev d = ev_dot3(nrm[0], wo[0], nrm[1], wo[1], nrm[2], wo[2]);
    mgs[1][0] = fabs(d.v - (double)1e-6f); mgs[1][1] = d.e * GSO_EPS;
    const int live_ndv = t->d >= 1e-6f;
    const gso_ev ndv = live_ndv ? d : ev_in((double)1e-6f);
    int cx, cy, ix0, ix1, iy0, iy1;
    const gso_ev lfx = ev_lut_axis(ndv, t->ndv, lut_res, &cx, &ix0, &ix1, mgs[2]);
    const gso_ev lfy = ev_lut_axis(rough, t->rough, lut_res, &cy, &iy0, &iy1, mgs[3]);
    gso_ev fg[2], dfu[2], dfv[2];
    for (int c = 0; c < 2; ++c) {
        const int W = lut_res;
        const gso_ev t00 = ev_in(lut[((size_t)iy0 * W + ix0) * 2 + c]), t10 = ev_in(lut[((size_t)iy0 * W + ix1) * 2 + c]);
        const gso_ev t01 = ev_in(lut[((size_t)iy1 * W + ix0) * 2 + c]), t11 = ev_in(lut[((size_t)iy1 * W + ix1) * 2 + c]);
        const gso_ev d10 = ev_sub(t10, t00), d11 = ev_sub(t11, t01);
        const gso_ev top = ev_add(t00, ev_mul(lfx, d10)), bot = ev_add(t01, ev_mul(lfx, d11));
        const gso_ev bt = ev_sub(bot, top);
        fg[c] = ev_add(top, ev_mul(lfy, bt));
        dfu[c] = cx ? zero : ev_mul(ev_in((double)W), ev_add(d10, ev_mul(lfy, ev_sub(d11, d10))));
        dfv[c] = cy ? zero : ev_mul(ev_in((double)W), bt);
    }
    gso_ev refl[3];
    for (int k = 0; k < 3; ++k) refl[k] = ev_sub(ev_mul(ev_scale(d, 2.0), nrm[k]), wo[k]);
    gso_ev ls_out[3] = { zero, zero, zero }, ls_dd[9], ls_dmip[3] = { zero, zero, zero }, ld[3] = { zero, zero, zero }, ld_dd[9];
    for (int i = 0; i < 9; ++i) { ls_dd[i] = zero; ld_dd[i] = zero; }
    gso_ev dm = zero, f = zero;
    ev_cube e0, e1, eb;
    if (mode != 1) {
        const gso_ev emin = ev_in(env_min_r), emax = ev_in(env_max_r), Lm2 = ev_in((double)(L - 2));
        const float r = t->rough;
        {
            double m4 = fabs(rough.v - emin.v);
            if (fabs(rough.v - emax.v) < m4) m4 = fabs(rough.v - emax.v);
            if (fabs(rough.v - 1.0) < m4) m4 = fabs(rough.v - 1.0);
            mgs[4][0] = m4; mgs[4][1] = rough.e * GSO_EPS;
        }
        gso_ev m;
        int t_clamped;
        if (r < env_max_r) {
            const float tf = (r - env_min_r) / (env_max_r - env_min_r);
            const gso_ev den = ev_sub(emax, emin);
            gso_ev tt = ev_div(ev_sub(rough, emin), den);
            t_clamped = !(tf >= 0.0f && tf <= 1.0f);
            if (tf < 0.0f) tt = zero; else if (tf > 1.0f) tt = one;
            m = ev_mul(tt, Lm2);
            dm = t_clamped ? zero : ev_div(Lm2, den);
        } else {
            const float tf = (r - env_max_r) / (1.0f - env_max_r);
            const gso_ev den = ev_sub(one, emax);
            gso_ev tt = ev_div(ev_sub(rough, emax), den);
            t_clamped = !(tf >= 0.0f && tf <= 1.0f);
            if (tf < 0.0f) tt = zero; else if (tf > 1.0f) tt = one;
            m = ev_add(tt, Lm2);
            dm = t_clamped ? zero : ev_div(one, den);
        }
        const float bias = t->mip;
        const int lam_clamped = (bias < 0.0f || bias > (float)(L - 1));
        gso_ev lam = m;
        if (bias < 0.0f) lam = zero; else if (bias > (float)(L - 1)) lam = ev_in((double)(L - 1));
        if (!t_clamped && !lam_clamped && L > 1) { mgs[5][0] = near_int(m.v); mgs[5][1] = m.e * GSO_EPS; }
        ev_cube_fetch(levels[t->ls.l0], res[t->ls.l0], refl, &t->ls.fp0, &e0);
        for (int i = 0; i < 6; ++i) mgs[6 + i / 2][i & 1] = e0.mg[i];
        if (t->ls.l1 < 0) {
            for (int c = 0; c < 3; ++c) ls_out[c] = e0.out[c];
            for (int i = 0; i < 9; ++i) ls_dd[i] = e0.dd[i];
        } else {
            f = ev_sub(lam, ev_in((double)t->ls.l0));
            ev_cube_fetch(levels[t->ls.l1], res[t->ls.l1], refl, &t->ls.fp1, &e1);
            for (int i = 0; i < 6; ++i) mgs[9 + i / 2][i & 1] = e1.mg[i];
            for (int c = 0; c < 3; ++c) {
                const gso_ev dc = ev_sub(e1.out[c], e0.out[c]);
                ls_out[c] = ev_add(e0.out[c], ev_mul(f, dc));
                ls_dmip[c] = lam_clamped ? zero : dc;
            }
            for (int i = 0; i < 9; ++i) ls_dd[i] = ev_add(e0.dd[i], ev_mul(f, ev_sub(e1.dd[i], e0.dd[i])));
        }
    } else {
        ev_cube_fetch(base, base_res, nrm, &t->ld_fp, &eb);
        for (int i = 0; i < 6; ++i) mgs[12 + i / 2][i & 1] = eb.mg[i];
        for (int c = 0; c < 3; ++c) ld[c] = eb.out[c];
        for (int i = 0; i < 9; ++i) ld_dd[i] = eb.dd[i];
    }
    gso_ev refl_c[3];
    for (int c = 0; c < 3; ++c) refl_c[c] = ev_add(ev_mul(spec[c], fg[0]), fg[1]);
    /* ---- backward */
    gso_ev v_diff[3] = { zero, zero, zero }, v_ls[3] = { zero, zero, zero }, v_rf[3] = { zero, zero, zero }, v_ld[3] = { zero, zero, zero };
    for (int c = 0; c < 3; ++c) {
        if (mode == 0)      { v_diff[c] = gv[c]; v_ls[c] = ev_mul(gv[c], refl_c[c]); v_rf[c] = ev_mul(gv[c], ls_out[c]); }
        else if (mode == 1) { v_ld[c] = ev_mul(gv[c], diff[c]); v_diff[c] = ev_mul(gv[c], ld[c]); }
        else                { v_ls[c] = ev_mul(gv[c], refl_c[c]); v_rf[c] = ev_mul(gv[c], ls_out[c]); }
    }
    gso_ev v_A = zero, v_B = zero, v_metal = zero, o_kd[3];
    for (int c = 0; c < 3; ++c) {
        const gso_ev v_spec = ev_mul(v_rf[c], fg[0]);
        v_A = ev_add(v_A, ev_mul(v_rf[c], spec[c]));
        v_B = ev_add(v_B, v_rf[c]);
        o_kd[c] = ev_add(ev_mul(v_spec, metal), ev_mul(v_diff[c], omm));
        v_metal = ev_add(v_metal, ev_sub(ev_mul(v_spec, ev_sub(kdv[c], c004)), ev_mul(v_diff[c], kdv[c])));
    }
    const gso_ev v_ndv = ev_add(ev_mul(v_A, dfu[0]), ev_mul(v_B, dfu[1]));
    gso_ev v_rough = ev_add(ev_mul(v_A, dfv[0]), ev_mul(v_B, dfv[1]));
    gso_ev v_mip = zero, v_refl[3] = { zero, zero, zero }, v_n[3] = { zero, zero, zero };
    for (int c = 0; c < 3; ++c) {
        v_mip = ev_add(v_mip, ev_mul(v_ls[c], ls_dmip[c]));
        for (int k = 0; k < 3; ++k) {
            v_refl[k] = ev_add(v_refl[k], ev_mul(v_ls[c], ls_dd[c * 3 + k]));
            v_n[k] = ev_add(v_n[k], ev_mul(v_ld[c], ld_dd[c * 3 + k]));
        }
    }
    v_rough = ev_add(v_rough, ev_mul(v_mip, dm));
    const gso_ev o_ks0 = ev_mul(v_rough, omr), o_ks1 = ev_mul(v_metal, maxm);
    gso_ev v_d = ev_scale(ev_dot3(v_refl[0], nrm[0], v_refl[1], nrm[1], v_refl[2], nrm[2]), 2.0);
    gso_ev v_wo[3];
    for (int k = 0; k < 3; ++k) { v_n[k] = ev_add(v_n[k], ev_mul(ev_scale(d, 2.0), v_refl[k])); v_wo[k] = ev_scale(v_refl[k], -1.0); }
    if (live_ndv) v_d = ev_add(v_d, v_ndv);
    for (int k = 0; k < 3; ++k) { v_n[k] = ev_add(v_n[k], ev_mul(v_d, wo[k])); v_wo[k] = ev_add(v_wo[k], ev_mul(v_d, nrm[k])); }
    gso_ev o_mean[3] = { zero, zero, zero };
    if (!t->wo_const) {
        const gso_ev dot = ev_dot3(wo[0], v_wo[0], wo[1], v_wo[1], wo[2], v_wo[2]);
        for (int k = 0; k < 3; ++k) o_mean[k] = ev_scale(ev_div(ev_sub(v_wo[k], ev_mul(wo[k], dot)), len), -1.0);
    }
    const int dead = (g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f);
    for (int k = 0; k < 3; ++k) {
        B->b_means[3 * (size_t)n + k] = dead ? 0.0 : o_mean[k].e;
        B->b_normals[3 * (size_t)n + k] = dead ? 0.0 : v_n[k].e;
        B->b_kd[3 * (size_t)n + k] = dead ? 0.0 : o_kd[k].e;
    }
    B->b_ks[2 * (size_t)n] = dead ? 0.0 : o_ks0.e; B->b_ks[2 * (size_t)n + 1] = dead ? 0.0 : o_ks1.e;
    if (B->margins) memcpy(B->margins + (size_t)n * GSO_SHADE_MARGINS * 2, mgs, sizeof(mgs));
    if (dead) return;
    if (mode != 1) {
        const int l0 = t->ls.l0, l1 = t->ls.l1;
        if (l1 < 0) ev_scatter(B->b_levels[l0], B->a_levels[l0], B->n_levels[l0], &t->ls.fp0, &e0, v_ls, one);
        else {
            ev_scatter(B->b_levels[l0], B->a_levels[l0], B->n_levels[l0], &t->ls.fp0, &e0, v_ls, ev_sub(one, f));
            ev_scatter(B->b_levels[l1], B->a_levels[l1], B->n_levels[l1], &t->ls.fp1, &e1, v_ls, f);
        }
    } else {
        ev_scatter(B->b_base, B->a_base, B->n_base, &t->ld_fp, &eb, v_ld, one);
    }
}

/* v_base / v_levels[l] must be zero-initialised by the caller (accumulated into).  gso_shade_bwd (B == NULL) and
 * gso_shade_bwd_budget share this loop, so the gradients are the same bits. */
static void shade_bwd_run(int N, const float* means, const float* normals, const float* kd, const float* ks,
                           const float* cam_pos, float min_roughness, float max_metallic, int mode,
                           const float* lut, int lut_res, const float* base, int base_res,
                           const float* const* levels, const int* res, int L, float env_min_r, float env_max_r,
                           const float* v_colors,
                           float* v_means, float* v_normals, float* v_kd, float* v_ks,
                           float* v_base, float* const* v_levels, shade_budget_out* B)
{
    /* the texel sums are taken in Gaussian order (the ordered region below): the same bits in every run and from both entries */
#pragma omp parallel for ordered schedule(dynamic, 64)
    for (int n = 0; n < N; ++n) {
        const float* normal = normals + 3 * (size_t)n;
        const float* kdn = kd + 3 * (size_t)n;
        const float* g = v_colors + 3 * (size_t)n;
        shade_tmp t;
        float color[3];
        shade_one(means + 3 * (size_t)n, normal, kdn, ks + 2 * (size_t)n, cam_pos,
                  min_roughness, max_metallic, mode, lut, lut_res, base, base_res, levels, res, L,
                  env_min_r, env_max_r, color, &t);
        float v_diff[3] = { 0, 0, 0 }, v_ls[3] = { 0, 0, 0 }, v_rf[3] = { 0, 0, 0 }, v_ld[3] = { 0, 0, 0 };
        for (int c = 0; c < 3; ++c) {
            if (mode == 0)      { v_diff[c] = g[c]; v_ls[c] = g[c] * t.refl_c[c]; v_rf[c] = g[c] * t.ls.out[c]; }
            else if (mode == 1) { v_ld[c] = g[c] * t.diff[c]; v_diff[c] = g[c] * t.ld[c]; }
            else                { v_ls[c] = g[c] * t.refl_c[c]; v_rf[c] = g[c] * t.ls.out[c]; }
        }
        float v_A = 0.0f, v_B = 0.0f, v_metal = 0.0f;
        for (int c = 0; c < 3; ++c) {
            float v_spec = v_rf[c] * t.fg[0];
            v_A += v_rf[c] * t.spec[c];
            v_B += v_rf[c];
            v_kd[3 * (size_t)n + c] = v_spec * t.metal + v_diff[c] * (1.0f - t.metal);
            v_metal += v_spec * (kdn[c] - 0.04f) - v_diff[c] * kdn[c];
        }
        float v_ndv = v_A * t.dfg_du[0] + v_B * t.dfg_du[1];
        float v_rough = v_A * t.dfg_dv[0] + v_B * t.dfg_dv[1];
        float v_mip = 0.0f, v_refl[3] = { 0, 0, 0 }, v_n[3] = { 0, 0, 0 };
        for (int c = 0; c < 3; ++c) {
            v_mip += v_ls[c] * t.ls.dmip[c];
            for (int k = 0; k < 3; ++k) {
                v_refl[k] += v_ls[c] * t.ls.dd[c * 3 + k];
                v_n[k] += v_ld[c] * t.ld_dd[c * 3 + k];
            }
        }
        v_rough += v_mip * t.dmip_dr;
        v_ks[2 * (size_t)n + 0] = v_rough * (1.0f - min_roughness);
        v_ks[2 * (size_t)n + 1] = v_metal * max_metallic;
        /* refl = 2 d n - wo */
        float v_d = 2.0f * ((v_refl[0] * normal[0] + v_refl[1] * normal[1]) + v_refl[2] * normal[2]);
        float v_wo[3];
        for (int k = 0; k < 3; ++k) { v_n[k] += 2.0f * t.d * v_refl[k]; v_wo[k] = -v_refl[k]; }
        if (t.d >= 1e-6f) v_d += v_ndv;
        for (int k = 0; k < 3; ++k) { v_n[k] += v_d * t.wo[k]; v_wo[k] += v_d * normal[k]; }
        for (int k = 0; k < 3; ++k) v_normals[3 * (size_t)n + k] = v_n[k];
        if (t.wo_const) {
            for (int k = 0; k < 3; ++k) v_means[3 * (size_t)n + k] = 0.0f;
        } else {
            float dot = (t.wo[0] * v_wo[0] + t.wo[1] * v_wo[1]) + t.wo[2] * v_wo[2];
            float l = fmaxf(t.len, 1e-6f);
            for (int k = 0; k < 3; ++k) v_means[3 * (size_t)n + k] = -((v_wo[k] - t.wo[k] * dot) / l);
        }
        /* texel gradients */
#pragma omp ordered
        {
        if (mode != 1) {
            if (t.ls.l1 < 0) cube_scatter(v_levels[t.ls.l0], &t.ls.fp0, v_ls, 1.0f);
            else {
                cube_scatter(v_levels[t.ls.l0], &t.ls.fp0, v_ls, 1.0f - t.ls.f);
                cube_scatter(v_levels[t.ls.l1], &t.ls.fp1, v_ls, t.ls.f);
            }
        } else {
            cube_scatter(v_base, &t.ld_fp, v_ld, 1.0f);
        }
        }
        if (B) shade_budget_gauss(n, means + 3 * (size_t)n, normal, kdn, ks + 2 * (size_t)n, cam_pos, min_roughness, max_metallic, mode,
                                  lut, lut_res, base, base_res, levels, res, L, env_min_r, env_max_r, g, &t, B);
    }
}

GSO_API void gso_shade_bwd(int N, const float* means, const float* normals, const float* kd, const float* ks,
                           const float* cam_pos, float min_roughness, float max_metallic, int mode,
                           const float* lut, int lut_res, const float* base, int base_res,
                           const float* const* levels, const int* res, int L, float env_min_r, float env_max_r,
                           const float* v_colors,
                           float* v_means, float* v_normals, float* v_kd, float* v_ks,
                           float* v_base, float* const* v_levels)
{
    shade_bwd_run(N, means, normals, kd, ks, cam_pos, min_roughness, max_metallic, mode, lut, lut_res, base, base_res, levels, res, L,
                  env_min_r, env_max_r, v_colors, v_means, v_normals, v_kd, v_ks, v_base, v_levels, NULL);
}

/* S1..S3 backward with an error budget: the gradients of gso_shade_bwd, bit for bit, plus one float64 budget in units of
 * 2^-24 per output element (shade_budget_gauss) and, with margins != NULL, the selection margins of every Gaussian
 * [N][15][2].  v_base / v_levels[l] must be zero-initialised by the caller; b_base / b_levels[l] are overwritten.  A row
 * whose colour cotangent is all zero and a texel no footprint touches get gradient 0 and budget 0.  A check reads
 * |got - want| <= kappa * 2^-24 * budget element-wise, with no exceptions; it holds for implementations that make the
 * same selections, which the margins let a caller assert. */
GSO_API int gso_shade_margin_count(void) { return GSO_SHADE_MARGINS; }

GSO_API void gso_shade_bwd_budget(int N, const float* means, const float* normals, const float* kd, const float* ks,
                                  const float* cam_pos, float min_roughness, float max_metallic, int mode,
                                  const float* lut, int lut_res, const float* base, int base_res,
                                  const float* const* levels, const int* res, int L, float env_min_r, float env_max_r,
                                  const float* v_colors,
                                  float* v_means, float* v_normals, float* v_kd, float* v_ks,
                                  float* v_base, float* const* v_levels,
                                  double* b_means, double* b_normals, double* b_kd, double* b_ks,
                                  double* b_base, double* const* b_levels, double* margins,
                                  double* const* pool_abs, int32_t* const* pool_n)
{
    shade_budget_out B;
    double* a_levels[16]; int32_t* n_levels[16];
    const size_t nb = 18 * (size_t)base_res * base_res;
    B.b_means = b_means; B.b_normals = b_normals; B.b_kd = b_kd; B.b_ks = b_ks; B.b_base = b_base; B.b_levels = b_levels;
    B.margins = margins;
    memset(b_base, 0, nb * sizeof(double));
    B.a_base = (double*)calloc(nb, sizeof(double)); B.n_base = (int32_t*)calloc(nb, sizeof(int32_t));
    for (int l = 0; l < L && l < 16; ++l) {
        const size_t nl = 18 * (size_t)res[l] * res[l];
        memset(b_levels[l], 0, nl * sizeof(double));
        a_levels[l] = (double*)calloc(nl, sizeof(double)); n_levels[l] = (int32_t*)calloc(nl, sizeof(int32_t));
    }
    B.a_levels = a_levels; B.n_levels = n_levels;
    shade_bwd_run(N, means, normals, kd, ks, cam_pos, min_roughness, max_metallic, mode, lut, lut_res, base, base_res, levels, res, L,
                  env_min_r, env_max_r, v_colors, v_means, v_normals, v_kd, v_ks, v_base, v_levels, &B);
    /* pool_abs / pool_n (nullable) [L + 1] arrays, the base last: sum |contribution| and the number of contributions per texel
     * element, and b_* then hold the sum of the contributions' own bounds only -- for a caller that pools several calls into one
     * sum (budget = sum of the own bounds + (n_total - 1) * sum of the magnitudes) */
    if (pool_abs) { memcpy(pool_abs[L], B.a_base, nb * sizeof(double)); memcpy(pool_n[L], B.n_base, nb * sizeof(int32_t)); }
    else for (size_t i = 0; i < nb; ++i) if (B.n_base[i] > 1) b_base[i] += (double)(B.n_base[i] - 1) * B.a_base[i];
    free(B.a_base); free(B.n_base);
    for (int l = 0; l < L && l < 16; ++l) {
        const size_t nl = 18 * (size_t)res[l] * res[l];
        if (pool_abs) { memcpy(pool_abs[l], a_levels[l], nl * sizeof(double)); memcpy(pool_n[l], n_levels[l], nl * sizeof(int32_t)); free(a_levels[l]); free(n_levels[l]); continue; }
        for (size_t i = 0; i < nl; ++i) if (n_levels[l][i] > 1) b_levels[l][i] += (double)(n_levels[l][i] - 1) * a_levels[l][i];
        free(a_levels[l]); free(n_levels[l]);
    }
}

/* stand-alone texture entry points so that tests can probe S2/S3 directly */
GSO_API void gso_tex2d_linear_clamp(int n, const float* lut, int W, int H, int C, const float* uv, float* out,
                                    float* d_du, float* d_dv)
{
    for (int i = 0; i < n; ++i)
        tex2d_linear_clamp(lut, W, H, C, uv[2 * i], uv[2 * i + 1], out + (size_t)i * C,
                           d_du ? d_du + (size_t)i * C : NULL, d_dv ? d_dv + (size_t)i * C : NULL);
}
GSO_API void gso_cube_linear(int n, const float* tex, int R, const float* dirs, float* out, float* dd)
{
    for (int i = 0; i < n; ++i) cube_fetch(tex, R, dirs + 3 * (size_t)i, out + 3 * (size_t)i, dd ? dd + 9 * (size_t)i : NULL, NULL);
}
GSO_API void gso_cube_mip_linear(int n, const float* const* levels, const int* res, int L, const float* dirs,
                                 const float* bias, float* out, float* dd, float* dmip)
{
    for (int i = 0; i < n; ++i) {
        mip_sample s;
        cube_mip_fetch(levels, res, L, dirs + 3 * (size_t)i, bias[i], &s);
        for (int c = 0; c < 3; ++c) out[3 * (size_t)i + c] = s.out[c];
        if (dd) memcpy(dd + 9 * (size_t)i, s.dd, sizeof(float) * 9);
        if (dmip) memcpy(dmip + 3 * (size_t)i, s.dmip, sizeof(float) * 3);
    }
}
GSO_API float gso_mip_from_roughness(float r, float min_r, float max_r, int L)
{
    return mip_from_roughness(r, min_r, max_r, L, NULL);
}
