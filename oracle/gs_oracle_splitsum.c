/*
 * gs_oracle_splitsum.c -- CPU ORACLE (test infrastructure, NOT product code).
 *
 * Plain-C restatement of the split-sum environment-map prefilter (stage S5 of
 * SURVEY.md section 8a), i.e. of the reference's in-repo CUDA kernels
 *   rfstudio/graphics/_mesh/_splitsum/c_src/cubemap.cu:17-46   pixel_area, cube_to_dir
 *   rfstudio/graphics/_mesh/_splitsum/c_src/cubemap.cu:110-168 DiffuseCubemapFwd/BwdKernel
 *   rfstudio/graphics/_mesh/_splitsum/c_src/cubemap.cu:174-244 ndfGGX, SpecularBoundsKernel
 *   rfstudio/graphics/_mesh/_splitsum/c_src/cubemap.cu:246-350 SpecularCubemapFwd/BwdKernel
 * and of the mip chain _CubeMapMip (rfstudio/graphics/_mesh/_texture.py:199-226).
 * The reference's own sources are CUDA (__global__/atomicAdd) and cannot be
 * compiled with gcc; no golden vectors exist for them in the reference
 * (tests/graphics/test_splitsum.py only asserts isfinite) -> PARITY UNPINNED,
 * the restatement follows the cited lines statement by statement.
 *
 * Gradient accumulators are double (the CUDA kernels use fp32 atomics in
 * arbitrary order).
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define GSO_API __attribute__((visibility("default")))

static float pixel_area(int x, int y, int N)                      /* cubemap.cu:17-30 */
{
    if (N > 1) {
        int H = N / 2;
        x = abs(x - H);
        y = abs(y - H);
        float dx = atanf((float)(x + 1) / (float)H) - atanf((float)x / (float)H);
        float dy = atanf((float)(y + 1) / (float)H) - atanf((float)y / (float)H);
        return dx * dy;
    }
    return 1.0f;
}

static void safe_normalize3(float* v)                             /* vec3f.h:90-94 */
{
    float l = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (l > 0.0f) { v[0] /= l; v[1] /= l; v[2] /= l; }
    else { v[0] = v[1] = v[2] = 0.0f; }
}

static void cube_to_dir(int x, int y, int side, int N, float* d)  /* cubemap.cu:32-46 */
{
    float fx = 2.0f * (((float)x + 0.5f) / (float)N) - 1.0f;
    float fy = 2.0f * (((float)y + 0.5f) / (float)N) - 1.0f;
    switch (side) {
    case 0: d[0] = 1.0f;  d[1] = -fy;   d[2] = -fx;   break;
    case 1: d[0] = -1.0f; d[1] = -fy;   d[2] = fx;    break;
    case 2: d[0] = fx;    d[1] = 1.0f;  d[2] = fy;    break;
    case 3: d[0] = fx;    d[1] = -1.0f; d[2] = -fy;   break;
    case 4: d[0] = fx;    d[1] = -fy;   d[2] = 1.0f;  break;
    default: d[0] = -fx;  d[1] = -fy;   d[2] = -1.0f; break;
    }
    safe_normalize3(d);
}

static inline float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* ---------------- mip chain: 2x2 average (_texture.py:201-206) ----------- */
GSO_API void gso_cubemap_mip_fwd(int R, int C, const float* in /*[6,R,R,C]*/, float* out /*[6,R/2,R/2,C]*/)
{
    int H = R / 2;
    for (int s = 0; s < 6; ++s)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < H; ++x)
                for (int c = 0; c < C; ++c) {
                    const float* p = in + (((size_t)s * R + 2 * y) * R + 2 * x) * C + c;
                    /* F.avg_pool2d: sum of the window (row-major) * 1/4 */
                    float sum = ((p[0] + p[C]) + p[(size_t)R * C]) + p[(size_t)R * C + C];
                    out[(((size_t)s * H + y) * H + x) * C + c] = sum * 0.25f;
                }
}

/* ---------------- diffuse irradiance (cubemap.cu:110-168) ---------------- */
GSO_API void gso_diffuse_cubemap_fwd(int R, const float* cubemap /*[6,R,R,3]*/, float* out /*[6,R,R,3]*/)
{
#pragma omp parallel for schedule(static)
    for (int o = 0; o < 6 * R * R; ++o) {
        int pz = o / (R * R), py = (o / R) % R, px = o % R;
        float N[3]; cube_to_dir(px, py, pz, R, N);
        float col[3] = { 0, 0, 0 };
        for (int s = 0; s < 6; ++s)
            for (int y = 0; y < R; ++y)
                for (int x = 0; x < R; ++x) {
                    float L[3]; cube_to_dir(x, y, s, R, L);
                    float costheta = fminf(fmaxf(dot3(N, L), 0.0f), 0.999f);
                    float w = costheta * pixel_area(x, y, R) / 3.141592f;
                    const float* t = cubemap + (((size_t)s * R + y) * R + x) * 3;
                    col[0] += t[0] * w; col[1] += t[1] * w; col[2] += t[2] * w;
                }
        out[(size_t)o * 3] = col[0]; out[(size_t)o * 3 + 1] = col[1]; out[(size_t)o * 3 + 2] = col[2];
    }
}

GSO_API void gso_diffuse_cubemap_bwd(int R, const float* v_out /*[6,R,R,3]*/, float* v_cubemap /*[6,R,R,3]*/)
{
    size_t n = (size_t)6 * R * R;
    double* acc = (double*)calloc(n * 3, sizeof(double));
    /* adjoint: loop over INPUT texels so that no atomics are needed */
#pragma omp parallel for schedule(static)
    for (int i = 0; i < (int)n; ++i) {
        int s = i / (R * R), y = (i / R) % R, x = i % R;
        float L[3]; cube_to_dir(x, y, s, R, L);
        float pa = pixel_area(x, y, R);
        double a0 = 0, a1 = 0, a2 = 0;
        for (int o = 0; o < (int)n; ++o) {
            int pz = o / (R * R), py = (o / R) % R, px = o % R;
            float N[3]; cube_to_dir(px, py, pz, R, N);
            float costheta = fminf(fmaxf(dot3(N, L), 0.0f), 0.999f);
            float w = costheta * pa / 3.141592f;
            a0 += (double)(v_out[(size_t)o * 3] * w);
            a1 += (double)(v_out[(size_t)o * 3 + 1] * w);
            a2 += (double)(v_out[(size_t)o * 3 + 2] * w);
        }
        acc[(size_t)i * 3] = a0; acc[(size_t)i * 3 + 1] = a1; acc[(size_t)i * 3 + 2] = a2;
    }
    for (size_t i = 0; i < n * 3; ++i) v_cubemap[i] = (float)acc[i];
    free(acc);
}

/* ---------------- GGX specular prefilter (cubemap.cu:174-350) ------------ */
static inline float ndfGGX(float alphaSqr, float cosTheta)        /* cubemap.cu:174-179 */
{
    float c = fminf(fmaxf(cosTheta, 0.0f), 1.0f);
    float d = (c * alphaSqr - c) * c + 1.0f;
    /* M_PI is a double constant in the CUDA source: (d*d) is promoted and the quotient rounded once */
    return (float)((double)alphaSqr / ((double)(d * d) * M_PI));
}

/* bounds[6,R,R,24] stored as floats, like the reference (SpecularBoundsKernel, cubemap.cu:181-244) */
GSO_API void gso_specular_bounds(int R, float costheta_cutoff, float* bounds)
{
    const int TILE = 16;
#pragma omp parallel for schedule(dynamic, 64)
    for (int o = 0; o < 6 * R * R; ++o) {
        int pz = o / (R * R), py = (o / R) % R, px = o % R;
        float VNR[3]; cube_to_dir(px, py, pz, R, VNR);
        for (int s = 0; s < 6; ++s) {
            int min_x = R - 1, max_x = 0, min_y = R - 1, max_y = 0;
            for (int tx = 0; tx < (R + TILE - 1) / TILE; ++tx)
                for (int ty = 0; ty < (R + TILE - 1) / TILE; ++ty) {
                    int tsx = tx * TILE, tsy = ty * TILE;
                    int tex = (tx + 1) * TILE < R ? (tx + 1) * TILE : R;
                    int tey = (ty + 1) * TILE < R ? (ty + 1) * TILE : R;
                    float L0[3], L1[3], L2[3], L3[3];
                    cube_to_dir(tsx, tsy, s, R, L0); cube_to_dir(tex, tsy, s, R, L1);
                    cube_to_dir(tsx, tey, s, R, L2); cube_to_dir(tex, tey, s, R, L3);
                    float mn[3], mx[3];
                    for (int k = 0; k < 3; ++k) {
                        mn[k] = fminf(fminf(L0[k], L1[k]), fminf(L2[k], L3[k]));
                        mx[k] = fmaxf(fmaxf(L0[k], L1[k]), fmaxf(L2[k], L3[k]));
                    }
                    float maxdp = fmaxf(mn[0] * VNR[0], mx[0] * VNR[0]) + fmaxf(mn[1] * VNR[1], mx[1] * VNR[1])
                                + fmaxf(mn[2] * VNR[2], mx[2] * VNR[2]);
                    if (maxdp >= costheta_cutoff) {
                        for (int y = tsy; y < tey; ++y)
                            for (int x = tsx; x < tex; ++x) {
                                float L[3]; cube_to_dir(x, y, s, R, L);
                                if (dot3(L, VNR) >= costheta_cutoff) {
                                    if (x < min_x) min_x = x; if (x > max_x) max_x = x;
                                    if (y < min_y) min_y = y; if (y > max_y) max_y = y;
                                }
                            }
                    }
                }
            float* b = bounds + (size_t)o * 24 + s * 4;
            b[0] = (float)min_x; b[1] = (float)max_x; b[2] = (float)min_y; b[3] = (float)max_y;
        }
    }
}

/* out[6,R,R,4] = (sum rgb*w, sum w) exactly like SpecularCubemapFwdKernel */
GSO_API void gso_specular_cubemap_fwd(int R, const float* cubemap, const float* bounds, float roughness,
                                      float costheta_cutoff, float* out)
{
    float alpha = roughness * roughness;
    float alphaSqr = alpha * alpha;
#pragma omp parallel for schedule(dynamic, 64)
    for (int o = 0; o < 6 * R * R; ++o) {
        int pz = o / (R * R), py = (o / R) % R, px = o % R;
        float VNR[3]; cube_to_dir(px, py, pz, R, VNR);
        float wsum = 0.0f, col[3] = { 0, 0, 0 };
        for (int s = 0; s < 6; ++s) {
            const float* b = bounds + (size_t)o * 24 + s * 4;
            int xmin = (int)b[0], xmax = (int)b[1], ymin = (int)b[2], ymax = (int)b[3];
            if (xmin <= xmax)
                for (int y = ymin; y <= ymax; ++y)
                    for (int x = xmin; x <= xmax; ++x) {
                        float L[3]; cube_to_dir(x, y, s, R, L);
                        if (dot3(L, VNR) >= costheta_cutoff) {
                            float Hv[3] = { L[0] + VNR[0], L[1] + VNR[1], L[2] + VNR[2] };
                            safe_normalize3(Hv);
                            float wiDotN = fmaxf(dot3(L, VNR), 0.0f);
                            float VNRDotH = fmaxf(dot3(VNR, Hv), 0.0f);
                            float w = wiDotN * ndfGGX(alphaSqr, VNRDotH) * pixel_area(x, y, R) / 4.0f;
                            const float* t = cubemap + (((size_t)s * R + y) * R + x) * 3;
                            col[0] += t[0] * w; col[1] += t[1] * w; col[2] += t[2] * w;
                            wsum += w;
                        }
                    }
        }
        out[(size_t)o * 4] = col[0]; out[(size_t)o * 4 + 1] = col[1]; out[(size_t)o * 4 + 2] = col[2];
        out[(size_t)o * 4 + 3] = wsum;
    }
}

/* v_out[6,R,R,3] is the gradient w.r.t. the UN-normalised rgb sums (channels 0..2 of the forward output) */
GSO_API void gso_specular_cubemap_bwd(int R, const float* bounds, const float* v_out, float roughness,
                                      float costheta_cutoff, float* v_cubemap)
{
    float alpha = roughness * roughness;
    float alphaSqr = alpha * alpha;
    size_t n = (size_t)6 * R * R;
    double* acc = (double*)calloc(n * 3, sizeof(double));
#pragma omp parallel for schedule(dynamic, 64)
    for (int o = 0; o < (int)n; ++o) {
        int pz = o / (R * R), py = (o / R) % R, px = o % R;
        float VNR[3]; cube_to_dir(px, py, pz, R, VNR);
        const float* g = v_out + (size_t)o * 3;
        for (int s = 0; s < 6; ++s) {
            const float* b = bounds + (size_t)o * 24 + s * 4;
            int xmin = (int)b[0], xmax = (int)b[1], ymin = (int)b[2], ymax = (int)b[3];
            if (xmin <= xmax)
                for (int y = ymin; y <= ymax; ++y)
                    for (int x = xmin; x <= xmax; ++x) {
                        float L[3]; cube_to_dir(x, y, s, R, L);
                        if (dot3(L, VNR) >= costheta_cutoff) {
                            float Hv[3] = { L[0] + VNR[0], L[1] + VNR[1], L[2] + VNR[2] };
                            safe_normalize3(Hv);
                            float wiDotN = fmaxf(dot3(L, VNR), 0.0f);
                            float VNRDotH = fmaxf(dot3(VNR, Hv), 0.0f);
                            float w = wiDotN * ndfGGX(alphaSqr, VNRDotH) * pixel_area(x, y, R) / 4.0f;
                            double* a = acc + (((size_t)s * R + y) * R + x) * 3;
                            for (int c = 0; c < 3; ++c) {
                                double v = (double)(g[c] * w);
#pragma omp atomic
                                a[c] += v;
                            }
                        }
                    }
        }
    }
    for (size_t i = 0; i < n * 3; ++i) v_cubemap[i] = (float)acc[i];
    free(acc);
}

/* ---------------- subsets of output texels (full-size parity tests: R = 512 / 256 / 128) ----------------
 * The prefilter is independent per output texel, so a test can evaluate it on a random subset `sel[n_sel]` of the
 * 6*R*R texels (flat index (s*R + y)*R + x) in seconds.  Same statements as the full loops above; bounds / out /
 * v_out are COMPACT (row i belongs to texel sel[i]), v_cubemap is the full [6,R,R,3] gradient. */
static void bounds_of_texel(int R, float costheta_cutoff, int o, float* b24)
{
    const int TILE = 16;
    int pz = o / (R * R), py = (o / R) % R, px = o % R;
    float VNR[3]; cube_to_dir(px, py, pz, R, VNR);
    for (int s = 0; s < 6; ++s) {
        int min_x = R - 1, max_x = 0, min_y = R - 1, max_y = 0;
        for (int tx = 0; tx < (R + TILE - 1) / TILE; ++tx)
            for (int ty = 0; ty < (R + TILE - 1) / TILE; ++ty) {
                int tsx = tx * TILE, tsy = ty * TILE;
                int tex = (tx + 1) * TILE < R ? (tx + 1) * TILE : R;
                int tey = (ty + 1) * TILE < R ? (ty + 1) * TILE : R;
                float L0[3], L1[3], L2[3], L3[3];
                cube_to_dir(tsx, tsy, s, R, L0); cube_to_dir(tex, tsy, s, R, L1);
                cube_to_dir(tsx, tey, s, R, L2); cube_to_dir(tex, tey, s, R, L3);
                float mn[3], mx[3];
                for (int k = 0; k < 3; ++k) {
                    mn[k] = fminf(fminf(L0[k], L1[k]), fminf(L2[k], L3[k]));
                    mx[k] = fmaxf(fmaxf(L0[k], L1[k]), fmaxf(L2[k], L3[k]));
                }
                float maxdp = fmaxf(mn[0] * VNR[0], mx[0] * VNR[0]) + fmaxf(mn[1] * VNR[1], mx[1] * VNR[1])
                            + fmaxf(mn[2] * VNR[2], mx[2] * VNR[2]);
                if (maxdp >= costheta_cutoff) {
                    for (int y = tsy; y < tey; ++y)
                        for (int x = tsx; x < tex; ++x) {
                            float L[3]; cube_to_dir(x, y, s, R, L);
                            if (dot3(L, VNR) >= costheta_cutoff) {
                                if (x < min_x) min_x = x; if (x > max_x) max_x = x;
                                if (y < min_y) min_y = y; if (y > max_y) max_y = y;
                            }
                        }
                }
            }
        float* b = b24 + s * 4;
        b[0] = (float)min_x; b[1] = (float)max_x; b[2] = (float)min_y; b[3] = (float)max_y;
    }
}

GSO_API void gso_specular_bounds_subset(int R, float costheta_cutoff, int n_sel, const int* sel, float* bounds /*[n_sel,24]*/)
{
#pragma omp parallel for schedule(dynamic, 8)
    for (int i = 0; i < n_sel; ++i) bounds_of_texel(R, costheta_cutoff, sel[i], bounds + (size_t)i * 24);
}

GSO_API void gso_specular_cubemap_fwd_subset(int R, const float* cubemap, int n_sel, const int* sel, const float* bounds,
                                             float roughness, float costheta_cutoff, float* out /*[n_sel,4]*/)
{
    float alpha = roughness * roughness;
    float alphaSqr = alpha * alpha;
#pragma omp parallel for schedule(dynamic, 8)
    for (int i = 0; i < n_sel; ++i) {
        int o = sel[i];
        int pz = o / (R * R), py = (o / R) % R, px = o % R;
        float VNR[3]; cube_to_dir(px, py, pz, R, VNR);
        float wsum = 0.0f, col[3] = { 0, 0, 0 };
        for (int s = 0; s < 6; ++s) {
            const float* b = bounds + (size_t)i * 24 + s * 4;
            int xmin = (int)b[0], xmax = (int)b[1], ymin = (int)b[2], ymax = (int)b[3];
            if (xmin <= xmax)
                for (int y = ymin; y <= ymax; ++y)
                    for (int x = xmin; x <= xmax; ++x) {
                        float L[3]; cube_to_dir(x, y, s, R, L);
                        if (dot3(L, VNR) >= costheta_cutoff) {
                            float Hv[3] = { L[0] + VNR[0], L[1] + VNR[1], L[2] + VNR[2] };
                            safe_normalize3(Hv);
                            float wiDotN = fmaxf(dot3(L, VNR), 0.0f);
                            float VNRDotH = fmaxf(dot3(VNR, Hv), 0.0f);
                            float w = wiDotN * ndfGGX(alphaSqr, VNRDotH) * pixel_area(x, y, R) / 4.0f;
                            const float* t = cubemap + (((size_t)s * R + y) * R + x) * 3;
                            col[0] += t[0] * w; col[1] += t[1] * w; col[2] += t[2] * w;
                            wsum += w;
                        }
                    }
        }
        out[(size_t)i * 4] = col[0]; out[(size_t)i * 4 + 1] = col[1]; out[(size_t)i * 4 + 2] = col[2];
        out[(size_t)i * 4 + 3] = wsum;
    }
}

GSO_API void gso_specular_cubemap_bwd_subset(int R, int n_sel, const int* sel, const float* bounds, const float* v_out /*[n_sel,3]*/,
                                             float roughness, float costheta_cutoff, float* v_cubemap /*[6,R,R,3]*/)
{
    float alpha = roughness * roughness;
    float alphaSqr = alpha * alpha;
    size_t n = (size_t)6 * R * R;
    double* acc = (double*)calloc(n * 3, sizeof(double));
#pragma omp parallel for schedule(dynamic, 8)
    for (int i = 0; i < n_sel; ++i) {
        int o = sel[i];
        int pz = o / (R * R), py = (o / R) % R, px = o % R;
        float VNR[3]; cube_to_dir(px, py, pz, R, VNR);
        const float* g = v_out + (size_t)i * 3;
        for (int s = 0; s < 6; ++s) {
            const float* b = bounds + (size_t)i * 24 + s * 4;
            int xmin = (int)b[0], xmax = (int)b[1], ymin = (int)b[2], ymax = (int)b[3];
            if (xmin <= xmax)
                for (int y = ymin; y <= ymax; ++y)
                    for (int x = xmin; x <= xmax; ++x) {
                        float L[3]; cube_to_dir(x, y, s, R, L);
                        if (dot3(L, VNR) >= costheta_cutoff) {
                            float Hv[3] = { L[0] + VNR[0], L[1] + VNR[1], L[2] + VNR[2] };
                            safe_normalize3(Hv);
                            float wiDotN = fmaxf(dot3(L, VNR), 0.0f);
                            float VNRDotH = fmaxf(dot3(VNR, Hv), 0.0f);
                            float w = wiDotN * ndfGGX(alphaSqr, VNRDotH) * pixel_area(x, y, R) / 4.0f;
                            double* a = acc + (((size_t)s * R + y) * R + x) * 3;
                            for (int c = 0; c < 3; ++c) {
                                double v = (double)(g[c] * w);
#pragma omp atomic
                                a[c] += v;
                            }
                        }
                    }
        }
    }
    for (size_t i = 0; i < n * 3; ++i) v_cubemap[i] = (float)acc[i];
    free(acc);
}

/* ======================= float64 restatement with per-element error budgets =======================
 * The operators above once more in double, from directions and pixel areas computed in double, each with a budget per
 * output element in units of u = 2^-24: a correct float32 implementation (any summation order, any rounding of the same
 * formulas) lands within kappa * u * budget of the value.  Test infrastructure like the rest of this file.
 *
 * What stays float32: the roughness -> alpha^2 = (r*r)*(r*r) (a parameter both sides hold as the same float), the constant
 * 3.141592f of the diffuse weight, and the PAIR SET of the specular operator -- `dot3(L, V) >= cutoff` on the float
 * directions inside the float boxes of gso_specular_bounds, exactly as the loops above decide it.
 *
 * Per pair weight  w = max(L.V, 0) * a2 / (d^2 pi) * area / 4,   d = (c a2 - c) c + 1,   c = clamp(V.H, 0, 1):
 *   - c is a dot product of two normalised float vectors: absolute error ~1.5 u.  d = 1 - c^2 (1 - a2) moves by 2 c dc <= 3 u
 *     ABSOLUTE while d itself falls to a2 = roughness^4 (4.1e-5 at roughness 0.08): relative 3 / d, and D ~ 1 / d^2 doubles
 *     it: 6 / d.  This is the conditioning of the reference's formula in float32, not an implementation error.
 *   - area = (atan((x+1)/H) - atan(x/H)) * (same in y): each atanf value a carries ~2 u a (its argument's division and
 *     its own rounding), the difference dx keeps that absolute error: relative 2 (a1 + a0) / dx, ~2 R at the face edge.
 *   - the remaining roundings (L.V, the normalisation of H, a2 / (d d pi), * area, / 4, * texel): a constant, 8.
 *   k(o,i) = 8 + 6 / d + 2 (a1 + a0) / dx + 2 (b1 + b0) / dy.
 */
typedef struct { int R; double* dir; double* area; double* acond; float* dirf; } ss_tab;

static void ss_tab_make(int R, ss_tab* t)
{
    size_t n = (size_t)6 * R * R;
    t->R = R;
    t->dir = (double*)malloc(n * 3 * sizeof(double)); t->area = (double*)malloc(n * sizeof(double));
    t->acond = (double*)malloc(n * sizeof(double)); t->dirf = (float*)malloc(n * 3 * sizeof(float));
    for (int s = 0; s < 6; ++s)
        for (int y = 0; y < R; ++y)
            for (int x = 0; x < R; ++x) {
                size_t i = ((size_t)s * R + y) * R + x;
                cube_to_dir(x, y, s, R, t->dirf + i * 3);
                double fx = 2.0 * (((double)x + 0.5) / (double)R) - 1.0, fy = 2.0 * (((double)y + 0.5) / (double)R) - 1.0;
                double d[3];
                switch (s) {
                case 0: d[0] = 1.0;  d[1] = -fy;  d[2] = -fx;  break;
                case 1: d[0] = -1.0; d[1] = -fy;  d[2] = fx;   break;
                case 2: d[0] = fx;   d[1] = 1.0;  d[2] = fy;   break;
                case 3: d[0] = fx;   d[1] = -1.0; d[2] = -fy;  break;
                case 4: d[0] = fx;   d[1] = -fy;  d[2] = 1.0;  break;
                default: d[0] = -fx; d[1] = -fy;  d[2] = -1.0; break;
                }
                double l = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                t->dir[i * 3] = d[0] / l; t->dir[i * 3 + 1] = d[1] / l; t->dir[i * 3 + 2] = d[2] / l;
                if (R > 1) {
                    int H = R / 2, ax = abs(x - H), ay = abs(y - H);
                    double a1 = atan((double)(ax + 1) / H), a0 = atan((double)ax / H);
                    double b1 = atan((double)(ay + 1) / H), b0 = atan((double)ay / H);
                    t->area[i] = (a1 - a0) * (b1 - b0);
                    t->acond[i] = 2.0 * (a1 + a0) / (a1 - a0) + 2.0 * (b1 + b0) / (b1 - b0);
                } else { t->area[i] = 1.0; t->acond[i] = 0.0; }
            }
}

static void ss_tab_free(ss_tab* t) { free(t->dir); free(t->area); free(t->acond); free(t->dirf); }

static inline double dot3d(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* weight of the pair (output direction V, source texel i) in double, *k = its relative float32 error coefficient */
static inline double ss_pair(const ss_tab* t, const double* V, size_t i, double a2, double ldv, double* k)
{
    const double* L = t->dir + i * 3;
    double Hv[3] = { L[0] + V[0], L[1] + V[1], L[2] + V[2] };
    double hl = sqrt(dot3d(Hv, Hv));
    double c = hl > 0.0 ? dot3d(V, Hv) / hl : 0.0;
    c = fmin(fmax(c, 0.0), 1.0);
    double d = (c * a2 - c) * c + 1.0;
    *k = 8.0 + 6.0 / d + t->acond[i];
    return fmax(ldv, 0.0) * (a2 / (d * d * M_PI)) * t->area[i] / 4.0;
}

typedef struct { double w, k; int idx; int member; int doubt; } ss_pair_rec;
#define SS_DOUBT (4.0 / 16777216.0)   /* a pair is in doubt when its float64 cosine lies within 4 u of the cutoff */

/* the pairs of output o inside its float boxes: the members of the float32 set, plus the non-members in doubt */
static int ss_list(const ss_tab* t, const float* bounds, int o, double a2, float cutoff, ss_pair_rec* rec)
{
    int R = t->R, n = 0;
    const float* Vf = t->dirf + (size_t)o * 3;
    const double* V = t->dir + (size_t)o * 3;
    for (int s = 0; s < 6; ++s) {
        const float* b = bounds + (size_t)o * 24 + s * 4;
        int xmin = (int)b[0], xmax = (int)b[1], ymin = (int)b[2], ymax = (int)b[3];
        if (xmin > xmax) continue;
        for (int y = ymin; y <= ymax; ++y)
            for (int x = xmin; x <= xmax; ++x) {
                size_t i = ((size_t)s * R + y) * R + x;
                int member = dot3(t->dirf + i * 3, Vf) >= cutoff;
                double ldv = dot3d(t->dir + i * 3, V);
                int doubt = fabs(ldv - (double)cutoff) <= SS_DOUBT;
                if (!member && !doubt) continue;
                rec[n].w = ss_pair(t, V, i, a2, ldv, &rec[n].k);
                rec[n].idx = (int)i; rec[n].member = member; rec[n].doubt = doubt;
                ++n;
            }
    }
    return n;
}

static double ss_alpha_sqr(float roughness) { float a = roughness * roughness; return (double)(a * a); }

/* Specular forward, normalised: val[o,c] = sum_i w c_i / sum_i w over the float32 pair set; C channels (several maps stacked).
 * The result is a weighted mean: an error dw of one weight moves it by |dw| |c_i - val| / W, so
 *   bud = sum_i w k |c_i - val| / W  +  8 sum_i w |c_i| / W        (the second term: the two summations and the division)
 * A pair in doubt adds its whole effect, 2^24 w |c_i - val| / W' (W' = W without it for a member), so that both decisions are
 * admissible; doubt[o] = 1 for an output that owns such a pair.  An empty lobe is 0 / 0: val = NaN, bud = 0. */
GSO_API void gso_specular_cubemap_fwd_budget(int R, int C, const float* cubemap, const float* bounds, float roughness,
                                             float costheta_cutoff, double* val, double* bud, unsigned char* doubt)
{
    ss_tab t; ss_tab_make(R, &t);
    double a2 = ss_alpha_sqr(roughness);
    int n = 6 * R * R;
#pragma omp parallel
    {
        ss_pair_rec* rec = (ss_pair_rec*)malloc((size_t)n * sizeof(ss_pair_rec));
#pragma omp for schedule(dynamic, 16)
        for (int o = 0; o < n; ++o) {
            int m = ss_list(&t, bounds, o, a2, costheta_cutoff, rec);
            double W = 0.0;
            int dbt = 0;
            for (int p = 0; p < m; ++p) { if (rec[p].member) W += rec[p].w; dbt |= rec[p].doubt; }
            doubt[o] = (unsigned char)dbt;
            for (int c = 0; c < C; ++c) {
                double* v = val + (size_t)o * C + c; double* bb = bud + (size_t)o * C + c;
                if (!(W > 0.0)) { *v = NAN; *bb = 0.0; continue; }
                double acc = 0.0;
                for (int p = 0; p < m; ++p) if (rec[p].member) acc += rec[p].w * (double)cubemap[(size_t)rec[p].idx * C + c];
                double mean = acc / W, b1 = 0.0, b2 = 0.0, b3 = 0.0;
                for (int p = 0; p < m; ++p) {
                    double tx = (double)cubemap[(size_t)rec[p].idx * C + c], dev = fabs(tx - mean);
                    if (rec[p].member) { b1 += rec[p].w * rec[p].k * dev; b2 += rec[p].w * fabs(tx); }
                    if (rec[p].doubt) {
                        double Wd = rec[p].member ? (W - rec[p].w > 0.0 ? W - rec[p].w : W) : W;
                        b3 += rec[p].w * dev / Wd;
                    }
                }
                *v = mean; *bb = b1 / W + 8.0 * b2 / W + 16777216.0 * b3;
            }
        }
        free(rec);
    }
    ss_tab_free(&t);
}

/* Specular backward of the NORMALISED level: g[i,c] = sum_o w(o,i) v[o,c] / W_o (v = cotangent of the normalised level, as
 * as_splitsum_backward takes it).  Each term carries its weight's k, the error of W_o (the w-weighted mean of k over o's lobe)
 * and 8 for the division, the product and the summations:
 *   bud[i,c] = sum_o |v[o,c]| w / W_o (k(o,i) + mean_o(k) + 8)
 * A pair in doubt adds 2^24 |v| w / W_o to its source texel and, through W_o, 2^24 w_p / W_o relative to every other term of o.
 * An input no cotangent reaches has g = 0 and bud = 0.  Outputs with an empty lobe (W_o = 0) are skipped: 0 / 0 there.
 * doubt[i] = 1 for a gradient texel that is the source of such a pair (of an output with a non-zero cotangent). */
GSO_API void gso_specular_cubemap_bwd_budget(int R, int C, const float* bounds, const float* v, float roughness,
                                             float costheta_cutoff, double* g, double* bud, unsigned char* doubt)
{
    ss_tab t; ss_tab_make(R, &t);
    double a2 = ss_alpha_sqr(roughness);
    int n = 6 * R * R;
    size_t nc = (size_t)n * C;
    memset(g, 0, nc * sizeof(double)); memset(bud, 0, nc * sizeof(double)); memset(doubt, 0, (size_t)n);
#pragma omp parallel
    {
        ss_pair_rec* rec = (ss_pair_rec*)malloc((size_t)n * sizeof(ss_pair_rec));
        double* pg = (double*)calloc(nc * 2, sizeof(double));
        double* pb = pg + nc;
        unsigned char* pd = (unsigned char*)calloc((size_t)n, 1);
#pragma omp for schedule(dynamic, 16)
        for (int o = 0; o < n; ++o) {
            const float* vo = v + (size_t)o * C;
            int any = 0;
            for (int c = 0; c < C; ++c) any |= vo[c] != 0.0f;
            if (!any) continue;
            int m = ss_list(&t, bounds, o, a2, costheta_cutoff, rec);
            double W = 0.0, K = 0.0, D = 0.0;
            for (int p = 0; p < m; ++p) {
                if (rec[p].member) { W += rec[p].w; K += rec[p].w * rec[p].k; }
                if (rec[p].doubt) D += rec[p].w;
            }
            if (!(W > 0.0)) continue;
            K /= W; D /= W;
            for (int p = 0; p < m; ++p) {
                double share = rec[p].w / W;
                double rel = rec[p].k + K + 8.0 + 16777216.0 * (D + (rec[p].doubt ? 1.0 : 0.0));
                size_t at = (size_t)rec[p].idx * C;
                if (rec[p].doubt) pd[rec[p].idx] = 1;
                for (int c = 0; c < C; ++c) {
                    double term = (double)vo[c] * share;
                    if (rec[p].member) { pg[at + c] += term; pb[at + c] += fabs(term) * rel; }
                    else pb[at + c] += fabs(term) * 16777216.0;
                }
            }
        }
#pragma omp critical
        {
            for (size_t i = 0; i < nc; ++i) { g[i] += pg[i]; bud[i] += pb[i]; }
            for (int i = 0; i < n; ++i) doubt[i] |= pd[i];
        }
        free(rec); free(pg); free(pd);
    }
    ss_tab_free(&t);
}

/* Diffuse irradiance, forward (bwd = 0: val[o] = sum_i src_i w(o,i)) and its adjoint (bwd = 1: val[i] = sum_o src_o w(o,i)),
 * w(o,i) = clamp(N_o . L_i, 0, 0.999) area_i / 3.141592f.  The cosine of two normalised float directions carries ~6 u ABSOLUTE
 * (2 u relative per direction component, the products and the sums), which also covers both clamps (continuous); the area
 * carries its conditioning (acond above), the remaining products 4; a summation of n = 6 R^2 terms in blocks or as a tree
 * carries ~log2(n) + 5 = 16 at R = 16:
 *   bud[t] = sum_j |src_j| area / pi (6 + cos (4 + acond))  +  16 sum_j |src_j| w */
GSO_API void gso_diffuse_cubemap_budget(int R, int C, const float* src, int bwd, double* val, double* bud)
{
    ss_tab t; ss_tab_make(R, &t);
    int n = 6 * R * R;
    const double pi_f = (double)3.141592f;
#pragma omp parallel for schedule(static)
    for (int o = 0; o < n; ++o) {
        for (int c = 0; c < C; ++c) { val[(size_t)o * C + c] = 0.0; bud[(size_t)o * C + c] = 0.0; }
        for (int j = 0; j < n; ++j) {
            double cs = fmin(fmax(dot3d(t.dir + (size_t)o * 3, t.dir + (size_t)j * 3), 0.0), 0.999);
            int a = bwd ? o : j;
            double ap = t.area[a] / pi_f, w = cs * ap;
            double e = ap * (6.0 + cs * (4.0 + t.acond[a])) + 16.0 * w;
            for (int c = 0; c < C; ++c) {
                double x = (double)src[(size_t)j * C + c];
                val[(size_t)o * C + c] += x * w; bud[(size_t)o * C + c] += fabs(x) * e;
            }
        }
    }
    ss_tab_free(&t);
}

/* 2x2 average: three additions of float32 and an exact * 0.25: bud = 3 * 0.25 * sum |texel| */
GSO_API void gso_cubemap_mip_fwd_budget(int R, int C, const float* in, double* val, double* bud)
{
    int H = R / 2;
    for (int s = 0; s < 6; ++s)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < H; ++x)
                for (int c = 0; c < C; ++c) {
                    const float* p = in + (((size_t)s * R + 2 * y) * R + 2 * x) * C + c;
                    double q[4] = { p[0], p[C], p[(size_t)R * C], p[(size_t)R * C + C] };
                    size_t o = (((size_t)s * H + y) * H + x) * C + c;
                    val[o] = 0.25 * (q[0] + q[1] + q[2] + q[3]);
                    bud[o] = 0.75 * (fabs(q[0]) + fabs(q[1]) + fabs(q[2]) + fabs(q[3]));
                }
}

/* ---- _CubeMapMip.backward in double: the seam-aware bilinear lookup of 0.25 v at every fine texel's direction ---- */
static const int SS_FACE[6][3] = { {2, 1, 0}, {2, 1, 0}, {0, 2, 1}, {0, 2, 1}, {0, 1, 2}, {0, 1, 2} };   /* a, b, c */
static const double SS_SIGN[6][2] = { {-1, -1}, {1, -1}, {1, 1}, {1, -1}, {1, -1}, {-1, -1} };            /* sx, sy */

static void ss_face_point(int s, double x, double y, double* p)
{
    switch (s) {
    case 0: p[0] = 1.0;  p[1] = -y;   p[2] = -x;   break;
    case 1: p[0] = -1.0; p[1] = -y;   p[2] = x;    break;
    case 2: p[0] = x;    p[1] = 1.0;  p[2] = y;    break;
    case 3: p[0] = x;    p[1] = -1.0; p[2] = -y;   break;
    case 4: p[0] = x;    p[1] = -y;   p[2] = 1.0;  break;
    default: p[0] = -x;  p[1] = -y;   p[2] = -1.0; break;
    }
}

static int ss_select_face(const double* d)
{
    double ax = fabs(d[0]), ay = fabs(d[1]), az = fabs(d[2]), c;
    int f;
    if (az > fmax(ax, ay)) { f = 4; c = d[2]; } else if (ay > ax) { f = 2; c = d[1]; } else { f = 0; c = d[0]; }
    return c < 0.0 ? f + 1 : f;
}

/* texel (ix, iy) of face s, each at most one step outside the face: linear index, or -1 for a cube corner */
static int ss_resolve_texel(int s, int ix, int iy, int R)
{
    int ox = (ix < 0 || ix >= R), oy = (iy < 0 || iy >= R);
    if (!ox && !oy) return (s * R + iy) * R + ix;
    if (ox && oy) return -1;
    double p[3];
    ss_face_point(s, 2.0 * ((ix + 0.5) / R) - 1.0, 2.0 * ((iy + 0.5) / R) - 1.0, p);
    int s2 = ss_select_face(p);
    double inv = 1.0 / fabs(p[SS_FACE[s2][2]]);
    double x2 = SS_SIGN[s2][0] * p[SS_FACE[s2][0]] * inv, y2 = SS_SIGN[s2][1] * p[SS_FACE[s2][1]] * inv;
    int jx = (int)floor((x2 + 1.0) * 0.5 * R), jy = (int)floor((y2 + 1.0) * 0.5 * R);
    if (jx < 0) jx = 0; if (jx > R - 1) jx = R - 1;
    if (jy < 0) jy = 0; if (jy > R - 1) jy = R - 1;
    return (s2 * R + jy) * R + jx;
}

/* v [6,R,R,3] (double: a level's gradient with its budget b_in, nullable, in the same units) -> val, bud [6,2R,2R,3].
 * In exact arithmetic the fine texel x sits at the coarse coordinate x/2 - 1/4: fractions 3/4 and 1/4, never near a texel
 * boundary, so the float32 selections are the exact ones.  In float32 the coordinate (xn + 1) * 0.5 * R - 0.5 carries the
 * ~4 u of the normalised direction's ratio times R / 2 plus its own roundings: ~3 R u on each fraction, which moves the
 * result by at most 3 R u sum |tap| per axis; the interpolation itself adds ~8 u of the taps:
 *   bud = 0.25 (6 R + 8) sum_taps |v_tap|  +  0.25 sum_taps weight_tap b_in_tap        (a missing corner tap = the mean of the
 * other three, i.e. its weight shared among them) */
GSO_API void gso_cubemap_mip_bwd_budget(int R, const double* v, const double* b_in, double* val, double* bud)
{
    int F = 2 * R;
#pragma omp parallel for schedule(static)
    for (int i = 0; i < 6 * F * F; ++i) {
        int x = i % F, y = (i / F) % F, s = i / (F * F);
        double tx = 0.5 * x - 0.25, ty = 0.5 * y - 0.25;
        int ix0 = (int)floor(tx), iy0 = (int)floor(ty);
        double fx = tx - ix0, fy = ty - iy0;
        int idx[4] = { ss_resolve_texel(s, ix0, iy0, R), ss_resolve_texel(s, ix0 + 1, iy0, R),
                       ss_resolve_texel(s, ix0, iy0 + 1, R), ss_resolve_texel(s, ix0 + 1, iy0 + 1, R) };
        double w[4] = { (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy };
        for (int k = 0; k < 4; ++k)
            if (idx[k] < 0) { for (int j = 0; j < 4; ++j) if (j != k) w[j] += w[k] / 3.0; w[k] = 0.0; break; }
        for (int c = 0; c < 3; ++c) {
            double a = 0.0, ab = 0.0, bi = 0.0;
            for (int k = 0; k < 4; ++k) {
                if (idx[k] < 0) continue;
                double tv = v[(size_t)idx[k] * 3 + c];
                a += w[k] * tv; ab += fabs(tv);
                if (b_in) bi += w[k] * b_in[(size_t)idx[k] * 3 + c];
            }
            val[(size_t)i * 3 + c] = 0.25 * a;
            bud[(size_t)i * 3 + c] = 0.25 * ((6.0 * R + 8.0) * ab + bi);
        }
    }
}
