// gs_meshshade.hip -- per-pixel split-sum PBR shading of a mesh G-buffer, and the 2-D texture lookup behind it.
//   texture2d      dr.texture(tex[None], uv, filter_mode='linear', boundary_mode='wrap' | 'clamp'), no mip chain
//   Texture2D.sample   rfstudio/graphics/_mesh/_texture.py:168-175 (the lookup at u (1 - 1/Wt) + 0.5/Wt with 'wrap')
//   PBRShader.shade    rfstudio/graphics/shaders.py:44-105 on position / normal / uv maps, occlusion 'texture' | 'none'
// The semantics are stated in include/geosplat_hip.h.  The FG-LUT lookup, roughness -> mip level, the seam-aware cube fetches and
// their VJP, and the row-pair texel commit are the shading stage's own (gs_shade_dev.h, gs_cube.h).
//
// Forward: one thread per pixel, a gather.  Backward: recomputes the forward (no saved state), contracts the colour cotangent
// BEFORE each cube fetch (cube_fetch_vjp: 4 scalars per level instead of a 3x3 Jacobian) and writes d_position / d_normal / d_uv
// from registers.  What is left is contention: every covered pixel of a constant-material render adds into the same 3 + 3 floats of
// two 1x1 textures, and every pixel adds into the 16^2 base level.  So
//   * every array that fits the block's LDS budget (kd, ks, base, the small levels) is summed in LDS and flushed once per block
//     with one global atomic per non-zero float;
//   * a 1x1 texture is summed over the wave in registers first (one LDS add per wave and channel);
//   * the rest goes out through the row-pair commit: the two taps of a bilinear row are six contiguous floats, issued by six
//     adjacent lanes of one atomic instruction (neighbouring lanes are neighbouring pixels and mostly hit neighbouring texels).
#include "gs_common.h"
#include <stdlib.h>
#include <math.h>

// Contraction OFF for the whole file: texel / LUT-cell / level / face selection is discontinuous in the coordinates.
#pragma clang fp contract(off)
#include "gs_shade_dev.h"

#define GS_MS_BLOCK 512                       // backward block (2 waves per SIMD: 256 registers for the recomputed forward)
#define GS_MS_TEX_LDS_FLOATS 8192             // a 2-D texture of at most this many floats gets a private copy

struct Tex2Dev { const float* data; int W, H; };

#include "gs_tex2d_dev.h"          // Tex2Fp, tex2d_footprint, tex2d_eval, tex2d_weights (shared with gs_envmap.hip)

// ---------------------------------------------------------------------------------------------------- texture2d
template <int C>
__global__ void __launch_bounds__(256)
tex2d_fwd_kernel(long long P, Tex2Dev tex, int boundary, const float* __restrict__ uv, float* __restrict__ out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const float2 q = *reinterpret_cast<const float2*>(uv + 2 * p);
    Tex2Fp fp;
    tex2d_footprint(tex.W, tex.H, q.x, q.y, boundary, fp);
    float o[C], du[C], dv[C];
    tex2d_eval<C>(tex.data, fp, o, du, dv);
#pragma unroll
    for (int c = 0; c < C; ++c) out[p * C + c] = o[c];
}

// persistent blocks; a texture of at most GS_MS_TEX_LDS_FLOATS floats is summed in LDS and flushed once per block
template <int C>
__global__ void __launch_bounds__(256)
tex2d_bwd_kernel(long long P, Tex2Dev tex, int boundary, const float* __restrict__ uv, const float* __restrict__ d_out,
                 float* __restrict__ d_uv, float* __restrict__ d_tex, int lds_floats)
{
    extern __shared__ __attribute__((aligned(16))) float s_tex[];
    for (int i = threadIdx.x; i < lds_floats; i += blockDim.x) s_tex[i] = 0.0f;
    __syncthreads();
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
        const float2 q = *reinterpret_cast<const float2*>(uv + 2 * p);
        Tex2Fp fp;
        tex2d_footprint(tex.W, tex.H, q.x, q.y, boundary, fp);
        float o[C], du[C], dv[C], g[C], w[4];
        tex2d_eval<C>(tex.data, fp, o, du, dv);
        tex2d_weights(fp, w);
        float gu = 0.0f, gv = 0.0f;
        bool any = false;
#pragma unroll
        for (int c = 0; c < C; ++c) { g[c] = d_out[p * C + c]; gu += g[c] * du[c]; gv += g[c] * dv[c]; any = any || g[c] != 0.0f; }
        *reinterpret_cast<float2*>(d_uv + 2 * p) = make_float2(gu, gv);
        if (!fp.valid || !any) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float val = g[c] * w[i];
                if (lds_floats > 0) atomicAdd(s_tex + (size_t)fp.idx[i] * C + c, val);
                else gs_atomic_add(d_tex + (size_t)fp.idx[i] * C + c, val);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < lds_floats; i += blockDim.x) {
        const float v = s_tex[i];
        if (v != 0.0f) gs_atomic_add(d_tex + i, v);
    }
}

static int tex2d_check(const char* fn, int Ht, int Wt, int C, int boundary)
{
    if (C < 1 || C > 4) { gs_set_error("%s: C must be in 1..4", fn); return GS_EINVAL; }
    if (Ht < 1 || Wt < 1 || (long long)Ht * Wt > (1ll << 28)) { gs_set_error("%s: bad texture size", fn); return GS_EINVAL; }
    if (boundary != GS_TEX_WRAP && boundary != GS_TEX_CLAMP) { gs_set_error("%s: unknown boundary mode", fn); return GS_EINVAL; }
    return GS_OK;
}

extern "C" int gs_tex2d_fwd(int64_t P, int Ht, int Wt, int C, int boundary, const float* tex, const float* uv, float* out, void* stream)
{
    { const int rc = tex2d_check(__func__, Ht, Wt, C, boundary); if (rc != GS_OK) return rc; }
    GS_CHECK_ARG(P >= 0 && P < (1ll << 31), "bad P");
    if (P == 0) return GS_OK;
    GS_CHECK_ARG(tex != nullptr && uv != nullptr && out != nullptr, "null pointer");
    const Tex2Dev t = { tex, Wt, Ht };
    const dim3 grid(gs_cdiv(P, 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 1: hipLaunchKernelGGL(tex2d_fwd_kernel<1>, grid, block, 0, s, (long long)P, t, boundary, uv, out); break;
    case 2: hipLaunchKernelGGL(tex2d_fwd_kernel<2>, grid, block, 0, s, (long long)P, t, boundary, uv, out); break;
    case 3: hipLaunchKernelGGL(tex2d_fwd_kernel<3>, grid, block, 0, s, (long long)P, t, boundary, uv, out); break;
    default: hipLaunchKernelGGL(tex2d_fwd_kernel<4>, grid, block, 0, s, (long long)P, t, boundary, uv, out); break;
    }
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_tex2d_bwd(int64_t P, int Ht, int Wt, int C, int boundary, const float* tex, const float* uv, const float* d_out,
                            float* d_uv, float* d_tex, void* stream)
{
    { const int rc = tex2d_check(__func__, Ht, Wt, C, boundary); if (rc != GS_OK) return rc; }
    GS_CHECK_ARG(P >= 0 && P < (1ll << 31), "bad P");
    if (P == 0) return GS_OK;
    GS_CHECK_ARG(tex != nullptr && uv != nullptr && d_out != nullptr && d_uv != nullptr && d_tex != nullptr, "null pointer");
    const Tex2Dev t = { tex, Wt, Ht };
    const long long floats = (long long)Ht * Wt * C;
    const int lds_floats = floats <= GS_MS_TEX_LDS_FLOATS ? (int)floats : 0;
    const int want = gs_cdiv(P, 256);
    const dim3 grid(want < 2048 ? want : 2048), block(256);
    const size_t lds = (size_t)lds_floats * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 1: hipLaunchKernelGGL(tex2d_bwd_kernel<1>, grid, block, lds, s, (long long)P, t, boundary, uv, d_out, d_uv, d_tex, lds_floats); break;
    case 2: hipLaunchKernelGGL(tex2d_bwd_kernel<2>, grid, block, lds, s, (long long)P, t, boundary, uv, d_out, d_uv, d_tex, lds_floats); break;
    case 3: hipLaunchKernelGGL(tex2d_bwd_kernel<3>, grid, block, lds, s, (long long)P, t, boundary, uv, d_out, d_uv, d_tex, lds_floats); break;
    default: hipLaunchKernelGGL(tex2d_bwd_kernel<4>, grid, block, lds, s, (long long)P, t, boundary, uv, d_out, d_uv, d_tex, lds_floats); break;
    }
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------- PBR shading of a G-buffer
struct MsCfg { int occlusion; float min_visibility; int bend; };

// everything of a pixel before the environment lookups; the SELECTING expressions are shared by the forward and the backward
struct MsPre {
    Tex2Fp kd_fp, ks_fp;
    float kd[3], ks[3], kd_du[3], kd_dv[3], ks_du[3], ks_dv[3];
    float n[3], sgn;               // the normal after the bend, and the bend's sign
    float wo[3], len; bool wo_const;
    float d; bool ndv_pass;
    float spec[3], diff[3], fg[2], dfg_du[2], dfg_dv[2];
    float refl[3], mip, dmip_dr;
    float vis; bool vis_pass;
};

// Texture2D.sample's coordinates: u (1 - 1/Wt) + 0.5/Wt
__device__ __forceinline__ float ms_sample_scale(int n) { return 1.0f - 1.0f / (float)n; }
__device__ __forceinline__ float ms_sample_coord(float u, int n) { return u * ms_sample_scale(n) + 0.5f / (float)n; }

__device__ __forceinline__ bool ms_load_pixel(long long p, const float* __restrict__ rast, const float* __restrict__ position,
                                              const float* __restrict__ normal, const float* __restrict__ uv, float* pos, float* nrm, float* q)
{
    const bool covered = rast[4 * p + 3] > 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { pos[k] = position[3 * p + k]; nrm[k] = normal[3 * p + k]; }
    q[0] = uv[2 * p]; q[1] = uv[2 * p + 1];
    const bool finite = isfinite(pos[0]) && isfinite(pos[1]) && isfinite(pos[2]) && isfinite(nrm[0]) && isfinite(nrm[1]) &&
                        isfinite(nrm[2]) && isfinite(q[0]) && isfinite(q[1]);
    return covered && finite;
}

__device__ __forceinline__ void ms_pre(const float* pos, const float* nrm, const float* q, const Tex2Dev& kd, const Tex2Dev& ks,
                                       const float* cam, const EnvDev& env, const MsCfg& cfg, MsPre& t)
{
    tex2d_footprint(kd.W, kd.H, ms_sample_coord(q[0], kd.W), ms_sample_coord(q[1], kd.H), GS_TEX_WRAP, t.kd_fp);
    tex2d_footprint(ks.W, ks.H, ms_sample_coord(q[0], ks.W), ms_sample_coord(q[1], ks.H), GS_TEX_WRAP, t.ks_fp);
    tex2d_eval<3>(kd.data, t.kd_fp, t.kd, t.kd_du, t.kd_dv);
    tex2d_eval<3>(ks.data, t.ks_fp, t.ks, t.ks_du, t.ks_dv);
    const float rough = t.ks[1], metal = t.ks[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        t.spec[c] = (1.0f - metal) * 0.04f + t.kd[c] * metal;
        t.diff[c] = t.kd[c] * (1.0f - metal);
    }
    const float v[3] = { cam[0] - pos[0], cam[1] - pos[1], cam[2] - pos[2] };
    t.len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (t.len < 1e-6f) { t.wo[0] = 0.0f; t.wo[1] = 0.0f; t.wo[2] = 1.0f; t.wo_const = true; }
    else { const float l = fmaxf(t.len, 1e-6f); t.wo[0] = v[0] / l; t.wo[1] = v[1] / l; t.wo[2] = v[2] / l; t.wo_const = false; }
    float d = nrm[0] * t.wo[0] + nrm[1] * t.wo[1] + nrm[2] * t.wo[2];
    float ndv;
    t.sgn = 1.0f;
    if (cfg.bend) {
        if (!(d > 0.0f)) t.sgn = -1.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) t.n[k] = t.sgn * nrm[k];
        d = t.n[0] * t.wo[0] + t.n[1] * t.wo[1] + t.n[2] * t.wo[2];
        ndv = d; t.ndv_pass = true;
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) t.n[k] = nrm[k];
        ndv = fmaxf(d, 1e-4f); t.ndv_pass = d >= 1e-4f;
    }
    t.d = d;
    tex2d_linear_clamp2(env.lut, env.lut_res, env.lut_res, ndv, rough, t.fg, t.dfg_du, t.dfg_dv);
#pragma unroll
    for (int k = 0; k < 3; ++k) t.refl[k] = 2.0f * d * t.n[k] - t.wo[k];
    t.mip = mip_from_roughness(rough, env.min_r, env.max_r, env.L, t.dmip_dr);
    if (cfg.occlusion == GS_OCC_TEXTURE) {
        const float a = 1.0f - t.ks[0];
        t.vis = fmaxf(a, cfg.min_visibility); t.vis_pass = a >= cfg.min_visibility;
    } else { t.vis = 1.0f; t.vis_pass = false; }
}

// VM: 0 the two modes of MsCfg (GS_OCC_TEXTURE / GS_OCC_NONE, the code and the bits these kernels always had); GS_OCC_AO /
// GS_OCC_SCREEN: v = max(vis_map[p], min_visibility) scales the diffuse term alone / the whole colour.  vis_map carries no gradient.
template <int VM>
__global__ void __launch_bounds__(256)
meshshade_fwd_kernel(long long P, const float* __restrict__ rast, const float* __restrict__ position, const float* __restrict__ normal,
                     const float* __restrict__ uv, Tex2Dev kd, Tex2Dev ks, const float* __restrict__ cam_pos, EnvDev env, MsCfg cfg,
                     const float* __restrict__ vis_map, float* __restrict__ color)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    float pos[3], nrm[3], q[2], out[3] = { 0.0f, 0.0f, 0.0f };
    if (ms_load_pixel(p, rast, position, normal, uv, pos, nrm, q)) {
        const float cam[3] = { cam_pos[0], cam_pos[1], cam_pos[2] };
        MsPre t;
        ms_pre(pos, nrm, q, kd, ks, cam, env, cfg, t);
        float ld[3], dd[9];
        CubeFp fp;
        MipSample ls;
        cube_fetch<false>(env.base, env.base_res, t.n, ld, dd, fp);
        cube_mip_fetch<false>(env, t.refl, t.mip, ls);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (VM == 0) out[c] = (ld[c] * t.diff[c] + ls.out[c] * (t.spec[c] * t.fg[0] + t.fg[1])) * t.vis;
            else {
                const float v = fmaxf(vis_map[p], cfg.min_visibility);
                if (VM == GS_OCC_AO) out[c] = ld[c] * t.diff[c] * v + ls.out[c] * (t.spec[c] * t.fg[0] + t.fg[1]);
                else out[c] = (ld[c] * t.diff[c] + ls.out[c] * (t.spec[c] * t.fg[0] + t.fg[1])) * v;
            }
        }
    }
    color[3 * p] = out[0]; color[3 * p + 1] = out[1]; color[3 * p + 2] = out[2];
}

// the two 2-D textures' gradients, beside the environment's (EnvGradDev): pointers and float offsets of the private LDS copies, or -1
struct MsGradDev { float* kd; float* ks; int lds_kd, lds_ks; };

// texel gradients of one 3-channel 2-D texture; all 64 lanes of the wave call together (`act`: this lane has a contribution)
__device__ __forceinline__ void ms_tex_scatter(float* glob, float* s_grad, int lds_off, const Tex2Dev& tex, const Tex2Fp& fp,
                                               const float* v, bool act, float* stage)
{
    float w[4];
    tex2d_weights(fp, w);
    if (tex.W * tex.H == 1) {                                        // every tap is texel 0: sum over the wave in registers
        const float ws = (w[0] + w[1]) + (w[2] + w[3]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float sum = gs_wave_sum(act ? v[c] * ws : 0.0f);
            if (gs_lane_id() == 0 && sum != 0.0f) {
                if (lds_off >= 0) atomicAdd(s_grad + lds_off + c, sum); else gs_atomic_add(glob + c, sum);
            }
        }
    } else if (lds_off >= 0) {
        if (act) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float* p = s_grad + lds_off + (size_t)fp.idx[i] * 3;
                atomicAdd(p, v[0] * w[i]); atomicAdd(p + 1, v[1] * w[i]); atomicAdd(p + 2, v[2] * w[i]);
            }
        }
    } else {
#pragma unroll
        for (int row = 0; row < 2; ++row) {                          // t00 | t10, then t01 | t11: neighbours in memory unless wrapped
            float* pa = act ? glob + (size_t)fp.idx[2 * row] * 3 : nullptr;
            float* pb = act ? glob + (size_t)fp.idx[2 * row + 1] * 3 : nullptr;
            const float wa = act ? w[2 * row] : 0.0f, wb = act ? w[2 * row + 1] : 0.0f;
            const float val[6] = { v[0] * wa, v[1] * wa, v[2] * wa, v[0] * wb, v[1] * wb, v[2] * wb };
            wave_add6<false>(pa, pb, val, stage);
        }
    }
}

template <int VM>
__global__ void __launch_bounds__(GS_MS_BLOCK)
meshshade_bwd_kernel(long long P, const float* __restrict__ rast, const float* __restrict__ position, const float* __restrict__ normal,
                     const float* __restrict__ uv, Tex2Dev kd, Tex2Dev ks, const float* __restrict__ cam_pos, EnvDev env, MsCfg cfg,
                     const float* __restrict__ vis_map, const float* __restrict__ d_color, float* __restrict__ d_position, float* __restrict__ d_normal,
                     float* __restrict__ d_uv, MsGradDev mg, EnvGradDev eg)
{
    extern __shared__ __attribute__((aligned(16))) float s_grad[];
    for (int i = threadIdx.x; i < eg.lds_floats; i += blockDim.x) s_grad[i] = 0.0f;
    __syncthreads();
    float* const stage = s_grad + eg.stage_off + (threadIdx.x >> 6) * 640;
    const float cam[3] = { cam_pos[0], cam_pos[1], cam_pos[2] };
    const long long span = (long long)gridDim.x * blockDim.x;
    const int n_iter = (int)((P + span - 1) / span);                  // wave-uniform: every lane reaches the wave-wide commits
    for (int it = 0; it < n_iter; ++it) {
        const long long p = it * span + (long long)blockIdx.x * blockDim.x + threadIdx.x;
        bool act = false;
        MsPre t;
        t.kd_fp = Tex2Fp{}; t.ks_fp = Tex2Fp{};                    // (valid = false: the wave-wide commits see defined footprints on idle lanes)
        CubeFp fp_b{}, fp0{}, fp1{};
        float v_kd[3] = { 0, 0, 0 }, v_ks[3] = { 0, 0, 0 }, v_ld[3] = { 0, 0, 0 }, v_ls[3] = { 0, 0, 0 };
        int l0 = 0, l1 = -1;
        float f = 0.0f;
        if (p < P) {
            float pos[3], nrm[3], q[2];
            float o_pos[3] = { 0, 0, 0 }, o_n[3] = { 0, 0, 0 }, o_uv[2] = { 0, 0 };
            const bool shaded = ms_load_pixel(p, rast, position, normal, uv, pos, nrm, q);
            const float g[3] = { d_color[3 * p], d_color[3 * p + 1], d_color[3 * p + 2] };
            if (shaded && (g[0] != 0.0f || g[1] != 0.0f || g[2] != 0.0f)) {
                act = true;
                ms_pre(pos, nrm, q, kd, ks, cam, env, cfg, t);
                const MipSelect sel = mip_select(env.L, t.mip);                       // the forward's (cube_mip_fetch) selection
                l0 = sel.l0; l1 = sel.l1; f = sel.f;
                const bool clamped = sel.clamped;
                float refl_c[3];
                // GS_OCC_SCREEN: the map's visibility v, a constant of the backward pass, takes the place of t.vis (which is 1 without
                // GS_OCC_TEXTURE); the chain rule below stays the expression tree it always was, so a map of ones gives the bits of
                // GS_OCC_NONE.  (GS_OCC_AO runs instantiation 0 and meshshade_ao_fix_kernel after it.)
                if (VM == GS_OCC_SCREEN) t.vis = fmaxf(vis_map[p], cfg.min_visibility);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    refl_c[c] = t.spec[c] * t.fg[0] + t.fg[1];
                    const float gv = g[c] * t.vis;
                    v_ld[c] = gv * t.diff[c];
                    v_ls[c] = gv * refl_c[c];
                }
                float ld[3], s_b, vd_b[3], o0[3], s0, vd0[3], o1[3] = { 0, 0, 0 }, s1 = 0.0f, vd1[3] = { 0, 0, 0 };
                cube_fetch_vjp(env.base, env.base_res, t.n, v_ld, ld, s_b, vd_b, fp_b);
                cube_fetch_vjp(env.levels[l0], env.res[l0], t.refl, v_ls, o0, s0, vd0, fp0);
                if (l1 >= 0) cube_fetch_vjp(env.levels[l1], env.res[l1], t.refl, v_ls, o1, s1, vd1, fp1);
                {
#pragma clang fp contract(fast)
                    const float metal = t.ks[2];
                    float ls[3], v_refl[3], v_n[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        ls[c] = l1 >= 0 ? o0[c] + f * (o1[c] - o0[c]) : o0[c];
                        v_refl[c] = l1 >= 0 ? vd0[c] + f * (vd1[c] - vd0[c]) : vd0[c];
                        v_n[c] = vd_b[c];
                    }
                    const float v_mip = (clamped || l1 < 0) ? 0.0f : s1 - s0;
                    float v_A = 0.0f, v_B = 0.0f, v_metal = 0.0f, v_vis = 0.0f;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float gv = g[c] * t.vis;
                        const float v_diff = gv * ld[c], v_rf = gv * ls[c];
                        const float v_spec = v_rf * t.fg[0];
                        v_A += v_rf * t.spec[c];
                        v_B += v_rf;
                        v_kd[c] = v_spec * metal + v_diff * (1.0f - metal);
                        v_metal += v_spec * (t.kd[c] - 0.04f) - v_diff * t.kd[c];
                        v_vis += g[c] * (ld[c] * t.diff[c] + ls[c] * refl_c[c]);
                    }
                    const float v_ndv = v_A * t.dfg_du[0] + v_B * t.dfg_du[1];
                    const float v_rough = v_A * t.dfg_dv[0] + v_B * t.dfg_dv[1] + v_mip * t.dmip_dr;
                    v_ks[0] = t.vis_pass ? -v_vis : 0.0f; v_ks[1] = v_rough; v_ks[2] = v_metal;
                    float v_d = 2.0f * (v_refl[0] * t.n[0] + v_refl[1] * t.n[1] + v_refl[2] * t.n[2]);
                    float v_wo[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) { v_n[k] += 2.0f * t.d * v_refl[k]; v_wo[k] = -v_refl[k]; }
                    if (t.ndv_pass) v_d += v_ndv;
#pragma unroll
                    for (int k = 0; k < 3; ++k) { v_n[k] += v_d * t.wo[k]; v_wo[k] += v_d * t.n[k]; }
                    if (!t.wo_const) {
                        const float dot = t.wo[0] * v_wo[0] + t.wo[1] * v_wo[1] + t.wo[2] * v_wo[2];
                        const float l = fmaxf(t.len, 1e-6f);
#pragma unroll
                        for (int k = 0; k < 3; ++k) o_pos[k] = -((v_wo[k] - t.wo[k] * dot) / l);
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) o_n[k] = t.sgn * v_n[k];
                    float gu = 0.0f, gv2 = 0.0f, hu = 0.0f, hv = 0.0f;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        gu += v_kd[c] * t.kd_du[c]; gv2 += v_kd[c] * t.kd_dv[c];
                        hu += v_ks[c] * t.ks_du[c]; hv += v_ks[c] * t.ks_dv[c];
                    }
                    o_uv[0] = gu * ms_sample_scale(kd.W) + hu * ms_sample_scale(ks.W);
                    o_uv[1] = gv2 * ms_sample_scale(kd.H) + hv * ms_sample_scale(ks.H);
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { d_position[3 * p + k] = o_pos[k]; d_normal[3 * p + k] = o_n[k]; }
            d_uv[2 * p] = o_uv[0]; d_uv[2 * p + 1] = o_uv[1];
        }
        // ---- texel gradients (wave-wide: inactive lanes take part with nothing to add)
        ms_tex_scatter(mg.kd, s_grad, mg.lds_kd, kd, t.kd_fp, v_kd, act, stage);
        ms_tex_scatter(mg.ks, s_grad, mg.lds_ks, ks, t.ks_fp, v_ks, act, stage);
        const CommitDevice commit{};
        env_scatter_wave(eg, s_grad, stage, commit, true, act ? 0 : -1, fp_b, v_ld, 1.0f);
        env_scatter_wave(eg, s_grad, stage, commit, false, act ? l0 : -1, fp0, v_ls, l1 < 0 ? 1.0f : 1.0f - f);
        env_scatter_wave(eg, s_grad, stage, commit, false, act ? l1 : -1, fp1, v_ls, f);
    }
    // ---- flush the private copies: one global atomic per non-zero float and block
    __syncthreads();
    // (kd, ks: lds_flush_array, inline -- with the two calls the compiler contracts four more multiply-adds of the chain rule above, and
    // d_position / d_normal / d_uv no longer have the bits they had)
    if (mg.lds_kd >= 0) {
        const int cnt = 3 * kd.W * kd.H;
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) { const float v = s_grad[mg.lds_kd + i]; if (v != 0.0f) gs_atomic_add(mg.kd + i, v); }
    }
    if (mg.lds_ks >= 0) {
        const int cnt = 3 * ks.W * ks.H;
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) { const float v = s_grad[mg.lds_ks + i]; if (v != 0.0f) gs_atomic_add(mg.ks + i, v); }
    }
    env_lds_flush(s_grad, eg, env);
}

// GS_OCC_AO, backward.  colour_ao = colour_none + (v - 1) l_diff diff, so the gradient is that of GS_OCC_NONE -- instantiation 0 of the
// kernel above, the very code 'none' runs, launched first -- plus the gradient of the second term, added here: to the base texels and
// the normal through the diffuse lookup, to kd, to the metallic channel of ks, and to uv through the two texture lookups; nothing
// depends on the position.  A pixel with v = 1 adds nothing at all, so a map of ones leaves the bits of 'none'.  The skeleton
// (persistent blocks, private LDS copies, wave-wide commits, one flush) is meshshade_bwd_kernel's, with its launch configuration.
__global__ void __launch_bounds__(GS_MS_BLOCK)
meshshade_ao_fix_kernel(long long P, const float* __restrict__ rast, const float* __restrict__ position, const float* __restrict__ normal,
                        const float* __restrict__ uv, Tex2Dev kd, Tex2Dev ks, const float* __restrict__ cam_pos, EnvDev env, MsCfg cfg,
                        const float* __restrict__ vis_map, const float* __restrict__ d_color, float* __restrict__ d_normal,
                        float* __restrict__ d_uv, MsGradDev mg, EnvGradDev eg)
{
    extern __shared__ __attribute__((aligned(16))) float s_grad[];
    for (int i = threadIdx.x; i < eg.lds_floats; i += blockDim.x) s_grad[i] = 0.0f;
    __syncthreads();
    float* const stage = s_grad + eg.stage_off + (threadIdx.x >> 6) * 640;
    const float cam[3] = { cam_pos[0], cam_pos[1], cam_pos[2] };
    const long long span = (long long)gridDim.x * blockDim.x;
    const int n_iter = (int)((P + span - 1) / span);                  // wave-uniform: every lane reaches the wave-wide commits
    for (int it = 0; it < n_iter; ++it) {
        const long long p = it * span + (long long)blockIdx.x * blockDim.x + threadIdx.x;
        bool act = false;
        MsPre t;
        t.kd_fp = Tex2Fp{}; t.ks_fp = Tex2Fp{};
        CubeFp fp_b{};
        float v_kd[3] = { 0, 0, 0 }, v_ks[3] = { 0, 0, 0 }, v_ld[3] = { 0, 0, 0 };
        if (p < P) {
            float pos[3], nrm[3], q[2];
            const bool shaded = ms_load_pixel(p, rast, position, normal, uv, pos, nrm, q);
            const float g[3] = { d_color[3 * p], d_color[3 * p + 1], d_color[3 * p + 2] };
            const float s = fmaxf(vis_map[p], cfg.min_visibility) - 1.0f;
            if (shaded && s != 0.0f && (g[0] != 0.0f || g[1] != 0.0f || g[2] != 0.0f)) {
                act = true;
                ms_pre(pos, nrm, q, kd, ks, cam, env, cfg, t);
                float gs[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { gs[c] = g[c] * s; v_ld[c] = gs[c] * t.diff[c]; }
                float ld[3], s_b, vd_b[3];
                cube_fetch_vjp(env.base, env.base_res, t.n, v_ld, ld, s_b, vd_b, fp_b);
                const float metal = t.ks[2];
                float v_metal = 0.0f, gu = 0.0f, gv = 0.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v_diff = gs[c] * ld[c];
                    v_kd[c] = v_diff * (1.0f - metal);
                    v_metal -= v_diff * t.kd[c];
                    gu += v_kd[c] * t.kd_du[c]; gv += v_kd[c] * t.kd_dv[c];
                }
                v_ks[2] = v_metal;
#pragma unroll
                for (int k = 0; k < 3; ++k) d_normal[3 * p + k] += t.sgn * vd_b[k];
                d_uv[2 * p] += gu * ms_sample_scale(kd.W) + v_metal * t.ks_du[2] * ms_sample_scale(ks.W);
                d_uv[2 * p + 1] += gv * ms_sample_scale(kd.H) + v_metal * t.ks_dv[2] * ms_sample_scale(ks.H);
            }
        }
        ms_tex_scatter(mg.kd, s_grad, mg.lds_kd, kd, t.kd_fp, v_kd, act, stage);
        ms_tex_scatter(mg.ks, s_grad, mg.lds_ks, ks, t.ks_fp, v_ks, act, stage);
        const CommitDevice commit{};
        env_scatter_wave(eg, s_grad, stage, commit, true, act ? 0 : -1, fp_b, v_ld, 1.0f);
    }
    __syncthreads();
    if (mg.lds_kd >= 0) {
        const int cnt = 3 * kd.W * kd.H;
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) { const float v = s_grad[mg.lds_kd + i]; if (v != 0.0f) gs_atomic_add(mg.kd + i, v); }
    }
    if (mg.lds_ks >= 0) {
        const int cnt = 3 * ks.W * ks.H;
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) { const float v = s_grad[mg.lds_ks + i]; if (v != 0.0f) gs_atomic_add(mg.ks + i, v); }
    }
    env_lds_flush(s_grad, eg, env);
}

static int meshshade_check(const char* fn, int H, int W, int kd_h, int kd_w, int ks_h, int ks_w, int occlusion, bool with_map,
                           const GsEnv* env, EnvDev& e)
{
    if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) { gs_set_error("%s: bad image size", fn); return GS_EINVAL; }
    if (kd_h < 1 || kd_w < 1 || ks_h < 1 || ks_w < 1 || (long long)kd_h * kd_w > (1ll << 28) || (long long)ks_h * ks_w > (1ll << 28)) {
        gs_set_error("%s: bad texture size", fn); return GS_EINVAL;
    }
    const bool known = with_map ? (occlusion == GS_OCC_AO || occlusion == GS_OCC_SCREEN) : (occlusion == GS_OCC_TEXTURE || occlusion == GS_OCC_NONE);
    if (!known) { gs_set_error("%s: unknown occlusion mode", fn); return GS_EINVAL; }
    if (env_to_dev(env, e) != 0 || e.L < 2 || e.lut_res < 1 || e.base_res < 1) { gs_set_error("%s: bad GsEnv", fn); return GS_EINVAL; }
    return GS_OK;
}

// the body of gs_meshshade_fwd and gs_meshshade_vis_fwd (vis == NULL: the former)
static int meshshade_fwd_impl(const char* fn, int H, int W, const float* rast, const float* position, const float* normal, const float* uv,
                              int kd_h, int kd_w, const float* kd, int ks_h, int ks_w, const float* ks, const float* cam_pos,
                              const GsEnv* env, int occlusion, float min_visibility, int bend_back_normal, const float* vis, bool with_map,
                              float* color, void* stream)
{
    EnvDev e;
    { const int rc = meshshade_check(fn, H, W, kd_h, kd_w, ks_h, ks_w, occlusion, with_map, env, e); if (rc != GS_OK) return rc; }
    if (!(rast != nullptr && position != nullptr && normal != nullptr && uv != nullptr && kd != nullptr && ks != nullptr &&
          cam_pos != nullptr && color != nullptr && (!with_map || vis != nullptr))) {
        gs_set_error("%s: null pointer", fn); return GS_EINVAL;
    }
    const long long P = (long long)H * W;
    const Tex2Dev tkd = { kd, kd_w, kd_h }, tks = { ks, ks_w, ks_h };
    const MsCfg cfg = { occlusion, min_visibility, bend_back_normal ? 1 : 0 };
    const dim3 grid(gs_cdiv(P, 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (!with_map)
        hipLaunchKernelGGL(meshshade_fwd_kernel<0>, grid, block, 0, s, P, rast, position, normal, uv, tkd, tks, cam_pos, e, cfg,
                           (const float*)nullptr, color);
    else if (occlusion == GS_OCC_AO)
        hipLaunchKernelGGL(meshshade_fwd_kernel<GS_OCC_AO>, grid, block, 0, s, P, rast, position, normal, uv, tkd, tks, cam_pos, e, cfg, vis, color);
    else
        hipLaunchKernelGGL(meshshade_fwd_kernel<GS_OCC_SCREEN>, grid, block, 0, s, P, rast, position, normal, uv, tkd, tks, cam_pos, e, cfg, vis,
                           color);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_meshshade_fwd(int H, int W, const float* rast, const float* position, const float* normal, const float* uv,
                                int kd_h, int kd_w, const float* kd, int ks_h, int ks_w, const float* ks, const float* cam_pos,
                                const GsEnv* env, int occlusion, float min_visibility, int bend_back_normal, float* color, void* stream)
{
    return meshshade_fwd_impl(__func__, H, W, rast, position, normal, uv, kd_h, kd_w, kd, ks_h, ks_w, ks, cam_pos, env, occlusion,
                              min_visibility, bend_back_normal, nullptr, false, color, stream);
}

extern "C" int gs_meshshade_vis_fwd(int H, int W, const float* rast, const float* position, const float* normal, const float* uv,
                                    int kd_h, int kd_w, const float* kd, int ks_h, int ks_w, const float* ks, const float* cam_pos,
                                    const GsEnv* env, int occlusion, float min_visibility, int bend_back_normal, const float* vis,
                                    float* color, void* stream)
{
    return meshshade_fwd_impl(__func__, H, W, rast, position, normal, uv, kd_h, kd_w, kd, ks_h, ks_w, ks, cam_pos, env, occlusion,
                              min_visibility, bend_back_normal, vis, true, color, stream);
}

template <int VM>
static int meshshade_bwd_launch(int blocks, size_t lds_bytes, hipStream_t s, long long P, const float* rast, const float* position,
                                const float* normal, const float* uv, Tex2Dev tkd, Tex2Dev tks, const float* cam_pos, const EnvDev& e,
                                const MsCfg& cfg, const float* vis, const float* d_color, float* d_position, float* d_normal, float* d_uv,
                                const MsGradDev& mg, const EnvGradDev& eg)
{
    GS_CHECK_HIP(hipFuncSetAttribute((const void*)meshshade_bwd_kernel<VM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(meshshade_bwd_kernel<VM>, dim3(blocks), dim3(GS_MS_BLOCK), lds_bytes, s, P, rast, position, normal, uv, tkd, tks,
                       cam_pos, e, cfg, vis, d_color, d_position, d_normal, d_uv, mg, eg);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// the body of gs_meshshade_bwd and gs_meshshade_vis_bwd
static int meshshade_bwd_impl(const char* fn, int H, int W, const float* rast, const float* position, const float* normal, const float* uv,
                              int kd_h, int kd_w, const float* kd, int ks_h, int ks_w, const float* ks, const float* cam_pos,
                              const GsEnv* env, int occlusion, float min_visibility, int bend_back_normal, const float* vis, bool with_map,
                              const float* d_color, float* d_position, float* d_normal, float* d_uv, float* d_kd, float* d_ks,
                              const GsEnvGrad* env_grad, void* stream)
{
    EnvDev e;
    { const int rc = meshshade_check(fn, H, W, kd_h, kd_w, ks_h, ks_w, occlusion, with_map, env, e); if (rc != GS_OK) return rc; }
    if (!(rast != nullptr && position != nullptr && normal != nullptr && uv != nullptr && kd != nullptr && ks != nullptr &&
          cam_pos != nullptr && d_color != nullptr && d_position != nullptr && d_normal != nullptr && d_uv != nullptr &&
          d_kd != nullptr && d_ks != nullptr && env_grad != nullptr && env_grad->base != nullptr && (!with_map || vis != nullptr))) {
        gs_set_error("%s: null pointer", fn); return GS_EINVAL;
    }
    const long long P = (long long)H * W;
    EnvGradDev eg;
    { const int rc = env_grad_to_dev(fn, env_grad, e, GS_MODE_PBR, eg); if (rc != GS_OK) return rc; }
    eg.priv = nullptr; eg.priv_stride = 0; eg.priv_base = -1;
    for (int l = 0; l < GS_MAX_LEVELS; ++l) eg.priv_level[l] = -1;
    // LDS layout: the two textures, the base level, then the pyramid from its coarsest level up, while they fit
    MsGradDev mg = { d_kd, d_ks, -1, -1 };
    int used = 0;
    const long long kd_f = 3ll * kd_h * kd_w, ks_f = 3ll * ks_h * ks_w;
    if (kd_f <= GS_MS_TEX_LDS_FLOATS) { mg.lds_kd = used; used += (int)kd_f; }
    if (ks_f <= GS_MS_TEX_LDS_FLOATS) { mg.lds_ks = used; used += (int)ks_f; }
    const size_t lds_bytes = env_lds_stage(env_lds_place(e, true, true, used, eg), GS_MS_BLOCK, eg);
    // persistent blocks, one flush each: as many as are resident at once -- ONE per compute unit (512 threads at 256 registers are the
    // 2 waves per SIMD a CU holds, whatever the LDS use)
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        GS_CHECK_HIP(hipGetDevice(&dev));
        GS_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
        n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    const int max_blocks = n_cu;
    const int want = gs_cdiv(P, GS_MS_BLOCK);
    const int blocks = want < max_blocks ? want : max_blocks;
    const MsCfg cfg = { occlusion, min_visibility, bend_back_normal ? 1 : 0 };
    const Tex2Dev tkd = { kd, kd_w, kd_h }, tks = { ks, ks_w, ks_h };
    hipStream_t s = (hipStream_t)stream;
    if (!with_map)
        return meshshade_bwd_launch<0>(blocks, lds_bytes, s, P, rast, position, normal, uv, tkd, tks, cam_pos, e, cfg, nullptr, d_color,
                                       d_position, d_normal, d_uv, mg, eg);
    if (occlusion == GS_OCC_AO) {
        const int rc = meshshade_bwd_launch<0>(blocks, lds_bytes, s, P, rast, position, normal, uv, tkd, tks, cam_pos, e, cfg, nullptr, d_color,
                                               d_position, d_normal, d_uv, mg, eg);
        if (rc != GS_OK) return rc;
        GS_CHECK_HIP(hipFuncSetAttribute((const void*)meshshade_ao_fix_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        hipLaunchKernelGGL(meshshade_ao_fix_kernel, dim3(blocks), dim3(GS_MS_BLOCK), lds_bytes, s, P, rast, position, normal, uv, tkd, tks,
                           cam_pos, e, cfg, vis, d_color, d_normal, d_uv, mg, eg);
        GS_CHECK_LAUNCH();
        return GS_OK;
    }
    return meshshade_bwd_launch<GS_OCC_SCREEN>(blocks, lds_bytes, s, P, rast, position, normal, uv, tkd, tks, cam_pos, e, cfg, vis, d_color,
                                               d_position, d_normal, d_uv, mg, eg);
}

extern "C" int gs_meshshade_bwd(int H, int W, const float* rast, const float* position, const float* normal, const float* uv,
                                int kd_h, int kd_w, const float* kd, int ks_h, int ks_w, const float* ks, const float* cam_pos,
                                const GsEnv* env, int occlusion, float min_visibility, int bend_back_normal, const float* d_color,
                                float* d_position, float* d_normal, float* d_uv, float* d_kd, float* d_ks, const GsEnvGrad* env_grad,
                                void* stream)
{
    return meshshade_bwd_impl(__func__, H, W, rast, position, normal, uv, kd_h, kd_w, kd, ks_h, ks_w, ks, cam_pos, env, occlusion,
                              min_visibility, bend_back_normal, nullptr, false, d_color, d_position, d_normal, d_uv, d_kd, d_ks, env_grad,
                              stream);
}

extern "C" int gs_meshshade_vis_bwd(int H, int W, const float* rast, const float* position, const float* normal, const float* uv,
                                    int kd_h, int kd_w, const float* kd, int ks_h, int ks_w, const float* ks, const float* cam_pos,
                                    const GsEnv* env, int occlusion, float min_visibility, int bend_back_normal, const float* vis,
                                    const float* d_color, float* d_position, float* d_normal, float* d_uv, float* d_kd, float* d_ks,
                                    const GsEnvGrad* env_grad, void* stream)
{
    return meshshade_bwd_impl(__func__, H, W, rast, position, normal, uv, kd_h, kd_w, kd, ks_h, ks_w, ks, cam_pos, env, occlusion,
                              min_visibility, bend_back_normal, vis, true, d_color, d_position, d_normal, d_uv, d_kd, d_ks, env_grad,
                              stream);
}
