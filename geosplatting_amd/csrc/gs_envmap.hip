// gs_envmap.hip -- resampling between the two environment parameterisations, and the environment as a background.
//   cube -> lat-long    TextureCubeMap.as_latlng   rfstudio/graphics/_mesh/_texture.py:454-465 (and visualize, :439-452)
//   lat-long -> cube    TextureLatLng.as_cubemap   rfstudio/graphics/_mesh/_texture.py:359-377
//   cube sample VJP     TextureCubeMap.sample      rfstudio/graphics/_mesh/_texture.py:411-420 (the forward is gs_cube_sample_linear)
//   background          TextureCubeMap.render      rfstudio/graphics/_mesh/_texture.py:422-437
// The semantics are stated in include/geosplat_hip.h.  Every lookup is one of the project's two: the seam-aware cube footprint of
// gs_cube.h and the 2-D 'wrap' footprint of gs_tex2d_dev.h.  One thread per output texel / pixel / direction; the directions are
// computed in registers.  The forwards are gathers without atomics (two runs are bit-identical).  The backwards recompute the
// footprint and ADD into the texel gradient through the row-pair commit of gs_cube.h (six adjacent lanes issue the six contiguous
// floats of a bilinear row): cube_scatter_wave for the cube, wave_add6 for the lat-long map (plain per-tap atomics measured 1 049 us
// for 256 x 512 <- 512^2).
#include "gs_common.h"
#include <math.h>

// Contraction OFF for the whole file: face and texel selection is discontinuous in the coordinates.
#pragma clang fp contract(off)
#include "gs_cube.h"
#include "gs_tex2d_dev.h"
#include "gs_tone.h"

#define GS_ENV_BLOCK 256
#define GS_ENV_PI 3.14159265358979323846f

// torch.linspace(lo, hi, n)[k]
__device__ __forceinline__ float env_linspace(float lo, float hi, int n, int k)
{
    return n > 1 ? lo + ((hi - lo) / (float)(n - 1)) * (float)k : lo;
}

// d = T v  (T row-major [3,3] in device memory, or null)
__device__ __forceinline__ void env_transform(const float* __restrict__ T, const float* v, float* d)
{
    if (T == nullptr) { d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; return; }
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = (T[3 * r] * v[0] + T[3 * r + 1] * v[1]) + T[3 * r + 2] * v[2];
}

// direction of lat-long texel (i, j): theta = pi linspace(1/H, 1 - 1/H, H)[i], phi = pi linspace(-1 + 1/W, 1 - 1/W, W)[j]
__device__ __forceinline__ void latlng_texel_dir(int i, int j, int H, int W, const float* __restrict__ T, float* d)
{
    const float theta = GS_ENV_PI * env_linspace(1.0f / (float)H, 1.0f - 1.0f / (float)H, H, i);
    const float phi = GS_ENV_PI * env_linspace(-1.0f + 1.0f / (float)W, 1.0f - 1.0f / (float)W, W, j);
    float st, ct, sp, cp;
    sincosf(theta, &st, &ct);
    sincosf(phi, &sp, &cp);
    const float v[3] = { st * sp, ct, -(st * cp) };
    env_transform(T, v, d);
}

// lat-long lookup coordinates of cube texel (s, y, x)
__device__ __forceinline__ void cube_texel_uv(int s, int y, int x, int R, float& tu, float& tv)
{
    const float lo = -1.0f + 1.0f / (float)R, hi = 1.0f - 1.0f / (float)R;
    float v[3];
    face_point(s, env_linspace(lo, hi, R, x), env_linspace(lo, hi, R, y), v);
    const float l = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] /= l; v[1] /= l; v[2] /= l;
    tu = atan2f(v[0], -v[2]) / (2.0f * GS_ENV_PI) + 0.5f;
    tv = acosf(fminf(fmaxf(v[1], -1.0f), 1.0f)) / GS_ENV_PI;
}

__device__ __forceinline__ void env_store3(float* __restrict__ out, long long p, const float* o)
{
    float* q = out + 3 * p;
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
}

// ---------------------------------------------------------------------------------------------------- cube -> lat-long
__global__ void __launch_bounds__(GS_ENV_BLOCK)
env_cube_to_latlng_fwd_kernel(int R, int H, int W, const float* __restrict__ cube, const float* __restrict__ T, float* __restrict__ out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)H * W) return;
    float d[3], o[3];
    latlng_texel_dir((int)(p / W), (int)(p % W), H, W, T, d);
    CubeFp fp;
    cube_fetch<false>(cube, R, d, o, nullptr, fp);
    env_store3(out, p, o);
}

// every lane of every wave reaches the commit (a lane past the end passes valid == false)
__global__ void __launch_bounds__(GS_ENV_BLOCK)
env_cube_to_latlng_bwd_kernel(int R, int H, int W, const float* __restrict__ T, const float* __restrict__ d_out, float* __restrict__ d_cube)
{
    __shared__ __attribute__((aligned(16))) float s_stage[(GS_ENV_BLOCK / GS_WAVE) * 640];
    float* stage = s_stage + (threadIdx.x / GS_WAVE) * 640;
    const long long total = (long long)H * W;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = p < total;
    const long long q = valid ? p : 0;
    float d[3];
    latlng_texel_dir((int)(q / W), (int)(q % W), H, W, T, d);
    CubeFp fp;
    cube_footprint(d, R, fp);
    const float g[3] = { d_out[3 * q], d_out[3 * q + 1], d_out[3 * q + 2] };
    cube_scatter_wave<false>(d_cube, fp, g, 1.0f, valid, stage);
}

// ---------------------------------------------------------------------------------------------------- lat-long -> cube
__global__ void __launch_bounds__(GS_ENV_BLOCK)
env_latlng_to_cube_fwd_kernel(int H, int W, int R, const float* __restrict__ latlng, float* __restrict__ out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)6 * R * R) return;
    float tu, tv;
    cube_texel_uv((int)(p / ((long long)R * R)), (int)((p / R) % R), (int)(p % R), R, tu, tv);
    Tex2Fp fp;
    tex2d_footprint(W, H, tu, tv, GS_TEX_WRAP, fp);
    float o[3], du[3], dv[3];
    tex2d_eval<3>(latlng, fp, o, du, dv);
    env_store3(out, p, o);
}

// The two taps of a bilinear row are neighbours in memory (apart from the wrap column), and neighbouring lanes are neighbouring cube
// texels that mostly hit the same few lat-long texels: the row-pair commit of gs_cube.h (six adjacent lanes issue the six floats of a
// row) serves the 2-D map as it serves the cube faces.  Every lane of every wave reaches the commit.
__global__ void __launch_bounds__(GS_ENV_BLOCK)
env_latlng_to_cube_bwd_kernel(int H, int W, int R, const float* __restrict__ d_out, float* __restrict__ d_latlng)
{
    __shared__ __attribute__((aligned(16))) float s_stage[(GS_ENV_BLOCK / GS_WAVE) * 640];
    float* stage = s_stage + (threadIdx.x / GS_WAVE) * 640;
    const long long total = (long long)6 * R * R;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long q = p < total ? p : 0;
    float tu, tv;
    cube_texel_uv((int)(q / ((long long)R * R)), (int)((q / R) % R), (int)(q % R), R, tu, tv);
    Tex2Fp fp;
    tex2d_footprint(W, H, tu, tv, GS_TEX_WRAP, fp);
    const bool valid = p < total && fp.valid;
    float w[4];
    tex2d_weights(fp, w);
    const float g[3] = { d_out[3 * q], d_out[3 * q + 1], d_out[3 * q + 2] };
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        float* pa = valid ? d_latlng + (size_t)fp.idx[2 * row] * 3 : nullptr;
        float* pb = valid ? d_latlng + (size_t)fp.idx[2 * row + 1] * 3 : nullptr;
        const float wa = w[2 * row], wb = w[2 * row + 1];
        const float v[6] = { g[0] * wa, g[1] * wa, g[2] * wa, g[0] * wb, g[1] * wb, g[2] * wb };
        wave_add6<false>(pa, pb, v, stage);
    }
}

// ---------------------------------------------------------------------------------------------------- cube sample VJP
__global__ void __launch_bounds__(GS_ENV_BLOCK)
env_cube_sample_bwd_kernel(long long n, int R, const float* __restrict__ dirs, float scale, const float* __restrict__ d_out,
                           float* __restrict__ d_cube)
{
    __shared__ __attribute__((aligned(16))) float s_stage[(GS_ENV_BLOCK / GS_WAVE) * 640];
    float* stage = s_stage + (threadIdx.x / GS_WAVE) * 640;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = p < n;
    const long long q = valid ? p : 0;
    const float d[3] = { dirs[3 * q], dirs[3 * q + 1], dirs[3 * q + 2] };
    CubeFp fp;
    cube_footprint(d, R, fp);
    const float g[3] = { d_out[3 * q], d_out[3 * q + 1], d_out[3 * q + 2] };
    cube_scatter_wave<false>(d_cube, fp, g, scale, valid, stage);
}

// ---------------------------------------------------------------------------------------------------- background
struct EnvCam { float fx, fy, cx, cy; };

__global__ void __launch_bounds__(GS_ENV_BLOCK)
env_background_kernel(int R, int H, int W, const float* __restrict__ cube, EnvCam cam, const float* __restrict__ c2w,
                      const float* __restrict__ T, int srgb, float* __restrict__ out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)H * W) return;
    const int i = (int)(p / W), j = (int)(p % W);
    const float v[3] = { ((0.5f - cam.cx) + (float)j) / cam.fx, -(((0.5f - cam.cy) + (float)i) / cam.fy), -1.0f };
    float w[3], d[3], o[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = (c2w[4 * r] * v[0] + c2w[4 * r + 1] * v[1]) + c2w[4 * r + 2] * v[2];     // c2w is [3,4]
    env_transform(T, w, d);
    CubeFp fp;
    cube_fetch<false>(cube, R, d, o, nullptr, fp);
    if (srgb) { o[0] = tone_rgb2srgb(o[0]); o[1] = tone_rgb2srgb(o[1]); o[2] = tone_rgb2srgb(o[2]); }
    env_store3(out, p, o);
}

// ---------------------------------------------------------------------------------------------------- entry points
static int env_check(const char* fn, int R, int H, int W)
{
    if (R < 1 || R > GS_CUBE_EDGE_TABLE_MAX_R) { gs_set_error("%s: bad R (faces from 1 up to 4096^2: gs_cube.h)", fn); return GS_EINVAL; }
    if (H < 2 || W < 2 || (long long)H * W > (1ll << 28)) { gs_set_error("%s: H and W must be at least 2 (and H W at most 2^28)", fn); return GS_EINVAL; }
    return GS_OK;
}

extern "C" int gs_env_cube_to_latlng_fwd(int R, int H, int W, const float* cube, const float* transform, float* out, void* stream)
{
    { const int rc = env_check(__func__, R, H, W); if (rc != GS_OK) return rc; }
    GS_CHECK_ARG(cube != nullptr && out != nullptr, "null pointer");
    hipLaunchKernelGGL(env_cube_to_latlng_fwd_kernel, dim3(gs_cdiv((int64_t)H * W, GS_ENV_BLOCK)), dim3(GS_ENV_BLOCK), 0, (hipStream_t)stream,
                       R, H, W, cube, transform, out);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_env_cube_to_latlng_bwd(int R, int H, int W, const float* transform, const float* d_out, float* d_cube, void* stream)
{
    { const int rc = env_check(__func__, R, H, W); if (rc != GS_OK) return rc; }
    GS_CHECK_ARG(d_out != nullptr && d_cube != nullptr, "null pointer");
    hipLaunchKernelGGL(env_cube_to_latlng_bwd_kernel, dim3(gs_cdiv((int64_t)H * W, GS_ENV_BLOCK)), dim3(GS_ENV_BLOCK), 0, (hipStream_t)stream,
                       R, H, W, transform, d_out, d_cube);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_env_latlng_to_cube_fwd(int H, int W, int R, const float* latlng, float* out, void* stream)
{
    { const int rc = env_check(__func__, R, H, W); if (rc != GS_OK) return rc; }
    GS_CHECK_ARG(latlng != nullptr && out != nullptr, "null pointer");
    hipLaunchKernelGGL(env_latlng_to_cube_fwd_kernel, dim3(gs_cdiv((int64_t)6 * R * R, GS_ENV_BLOCK)), dim3(GS_ENV_BLOCK), 0,
                       (hipStream_t)stream, H, W, R, latlng, out);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_env_latlng_to_cube_bwd(int H, int W, int R, const float* d_out, float* d_latlng, void* stream)
{
    { const int rc = env_check(__func__, R, H, W); if (rc != GS_OK) return rc; }
    GS_CHECK_ARG(d_out != nullptr && d_latlng != nullptr, "null pointer");
    hipLaunchKernelGGL(env_latlng_to_cube_bwd_kernel, dim3(gs_cdiv((int64_t)6 * R * R, GS_ENV_BLOCK)), dim3(GS_ENV_BLOCK), 0,
                       (hipStream_t)stream, H, W, R, d_out, d_latlng);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_cube_sample_linear_bwd(int64_t n, int R, const float* dirs, float scale, const float* d_out, float* d_tex, void* stream)
{
    GS_CHECK_ARG(n >= 0 && n < (1ll << 31) && R >= 1 && R <= GS_CUBE_EDGE_TABLE_MAX_R, "bad sizes (faces up to 4096^2: gs_cube.h)");
    if (n == 0) return GS_OK;
    GS_CHECK_ARG(dirs != nullptr && d_out != nullptr && d_tex != nullptr, "null pointer");
    hipLaunchKernelGGL(env_cube_sample_bwd_kernel, dim3(gs_cdiv(n, GS_ENV_BLOCK)), dim3(GS_ENV_BLOCK), 0, (hipStream_t)stream,
                       (long long)n, R, dirs, scale, d_out, d_tex);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_env_background_fwd(int R, int H, int W, const float* cube, float fx, float fy, float cx, float cy, const float* c2w,
                                     const float* transform, int srgb, float* out, void* stream)
{
    GS_CHECK_ARG(R >= 1 && R <= GS_CUBE_EDGE_TABLE_MAX_R, "bad R (faces from 1 up to 4096^2: gs_cube.h)");
    GS_CHECK_ARG(H >= 1 && W >= 1 && (long long)H * W <= (1ll << 28), "bad image size");
    GS_CHECK_ARG(fx != 0.0f && fy != 0.0f && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy), "bad intrinsics");
    GS_CHECK_ARG(cube != nullptr && c2w != nullptr && out != nullptr, "null pointer");
    const EnvCam cam = { fx, fy, cx, cy };
    hipLaunchKernelGGL(env_background_kernel, dim3(gs_cdiv((int64_t)H * W, GS_ENV_BLOCK)), dim3(GS_ENV_BLOCK), 0, (hipStream_t)stream,
                       R, H, W, cube, cam, c2w, transform, srgb, out);
    GS_CHECK_LAUNCH();
    return GS_OK;
}
