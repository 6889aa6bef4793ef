// gs_surfel.hip -- 2D Gaussian splatting (surfels) for gfx950: the two stages the 3DGS path does not have.
//   S1  surfel projection: ray transform M = K [s0 Rc0 | s1 Rc1 | c], screen bounds, camera-facing normal, SH colours;
//       packed in ascending Gaussian order by a three-launch compaction (count, scan of the block totals, write) -- no look-back
//   S1' its exact backward (means2d through the bounds formula, the quaternion normalisation, the SH colours)
//   S5  ray-splat compositor: one tile per workgroup, front to back, Gaussians staged through LDS in batches
//   S6  its stored-state backward: back to front from (final T, last index, final D), alpha recomputed with the forward's expressions,
//       every per-Gaussian gradient reduced over the workgroup before one global atomic per value
// Binning, sort and tile offsets are gs_isect_bin / gs_isect_offsets on (means2d, radii, depths), unchanged.
// Semantics: gsplat 1.4 rasterization_2dgs(packed=True), one camera, as restated in tests/surfel_ref.py.  All arithmetic fp32.
#include "gs_common.h"
#include "gs_ws.h"
#include "gs_project_dev.h"
#include "gs_sh_dev.h"

// Contraction is off at file scope: every cull, radius, tile count, skip and sign below must come out the same in the forward and in
// the backward, and the helpers of gs_sh_dev.h that do not set a mode themselves (sh_campos) are compiled under this one.  The
// kernels whose results are only gradients turn it on for their own bodies.
#pragma clang fp contract(off)

#define SF_BLOCK 256
#define SF_WAVES (SF_BLOCK / 64)
#define SF_REC 20                    // floats per staged Gaussian: M[9], means2d[2], opacity, normal[3], colours[<= 4], pad
#define SF_MAX_RADIUS 16777216.0f    // radii are stored as int32

// ---------------------------------------------------------------------------------------------------
struct SurfelFwd {
    bool valid;
    int radius;
    float m2x, m2y, depth;
    float M[9];
    float nrm[3];
};

// The camera-space centre, the camera-space rotation and the side the normal is seen from.  The forward and the backward both call
// these with contraction off, so the backward flips the normal's gradient exactly when the forward flipped the normal.
__device__ __forceinline__ void surfel_cam_mean(const GsCam& c, const float* mean, float* mc)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
        mc[i] = ((c.R[i * 3 + 0] * mean[0] + c.R[i * 3 + 1] * mean[1]) + c.R[i * 3 + 2] * mean[2]) + c.t[i];
}

__device__ __forceinline__ void surfel_cam_rot(const GsCam& c, float qw, float qx, float qy, float qz, float* Rc)
{
#pragma clang fp contract(off)
    float Rq[9];
    quat_to_rotmat_exact(qw, qx, qy, qz, Rq);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Rc[i * 3 + j] = (c.R[i * 3 + 0] * Rq[0 * 3 + j] + c.R[i * 3 + 1] * Rq[1 * 3 + j]) + c.R[i * 3 + 2] * Rq[2 * 3 + j];
}

// -1 when the surfel's axis points away from the camera (n . c > 0) and the normal is negated, else +1
__device__ __forceinline__ float surfel_normal_sign(const float* Rc, const float* mc)
{
#pragma clang fp contract(off)
    return ((Rc[2] * mc[0] + Rc[5] * mc[1]) + Rc[8] * mc[2]) > 0.0f ? -1.0f : 1.0f;
}

// (contraction is off here, as in project_exact: the culls, radii and tile counts must not depend on how a caller is compiled)
__device__ __forceinline__ SurfelFwd surfel_project(const GsCam& c, const float* mean, const float* quat, float s0, float s1, float Wf,
                                                    float Hf, float near_plane, float far_plane, float radius_clip)
{
#pragma clang fp contract(off)
    SurfelFwd o;
    o.valid = false; o.radius = 0; o.m2x = o.m2y = o.depth = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.M[i] = 0.0f;
    o.nrm[0] = o.nrm[1] = o.nrm[2] = 0.0f;
    float mc[3], Rc[9];
    surfel_cam_mean(c, mean, mc);
    if (mc[2] < near_plane || mc[2] > far_plane) return o;
    surfel_cam_rot(c, quat[0], quat[1], quat[2], quat[3], Rc);
    float Hm[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) { Hm[i * 3 + 0] = s0 * Rc[i * 3 + 0]; Hm[i * 3 + 1] = s1 * Rc[i * 3 + 1]; Hm[i * 3 + 2] = mc[i]; }
    float* M0 = o.M; float* M1 = o.M + 3; float* M2 = o.M + 6;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        M0[j] = c.fx * Hm[0 * 3 + j] + c.cx * Hm[2 * 3 + j];
        M1[j] = c.fy * Hm[1 * 3 + j] + c.cy * Hm[2 * 3 + j];
        M2[j] = Hm[2 * 3 + j];
    }
    const float d = (M2[0] * M2[0] + M2[1] * M2[1]) - M2[2] * M2[2];
    if (d == 0.0f) return o;
    const float f = 1.0f / d;
    const float mx = f * ((M0[0] * M2[0] + M0[1] * M2[1]) - M0[2] * M2[2]);
    const float my = f * ((M1[0] * M2[0] + M1[1] * M2[1]) - M1[2] * M2[2]);
    const float ex = mx * mx - f * ((M0[0] * M0[0] + M0[1] * M0[1]) - M0[2] * M0[2]);
    const float ey = my * my - f * ((M1[0] * M1[0] + M1[1] * M1[1]) - M1[2] * M1[2]);
    float radius = ceilf(3.0f * sqrtf(fmaxf(1e-4f, fmaxf(ex, ey))));
    if (!(radius > radius_clip)) return o;
    radius = fminf(radius, SF_MAX_RADIUS);
    if (!(mx + radius > 0.0f) || !(mx - radius < Wf) || !(my + radius > 0.0f) || !(my - radius < Hf)) return o;
    const float sgn = surfel_normal_sign(Rc, mc);
    o.nrm[0] = sgn * Rc[2]; o.nrm[1] = sgn * Rc[5]; o.nrm[2] = sgn * Rc[8];
    o.valid = true;
    o.radius = (int)radius;
    o.m2x = mx; o.m2y = my; o.depth = mc[2];
    return o;
}

__device__ __forceinline__ SurfelFwd surfel_project_n(const GsCam& cam, int n, const float* __restrict__ means, const float* __restrict__ quats,
                                                      const float* __restrict__ scales, int W, int H, float near_plane, float far_plane,
                                                      float radius_clip)
{
    const float mean[3] = { means[3 * (size_t)n], means[3 * (size_t)n + 1], means[3 * (size_t)n + 2] };
    const float4 q = *reinterpret_cast<const float4*>(quats + 4 * (size_t)n);
    const float quat[4] = { q.x, q.y, q.z, q.w };
    return surfel_project(cam, mean, quat, scales[3 * (size_t)n], scales[3 * (size_t)n + 1], (float)W, (float)H, near_plane, far_plane,
                          radius_clip);
}

// S1 pass 1: tiles[n] = tile count of Gaussian n, -1 when culled; block totals of (visible, tiles)
__global__ void __launch_bounds__(SF_BLOCK)
surfel_count_kernel(int N, const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
                    const float* __restrict__ viewmat, const float* __restrict__ K, int W, int H, int tile_size, int tile_w, int tile_h,
                    float near_plane, float far_plane, float radius_clip, int32_t* __restrict__ tiles, int32_t* __restrict__ block_v,
                    long long* __restrict__ block_i)
{
    __shared__ unsigned s_v[SF_WAVES], s_i[SF_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x * SF_BLOCK + tid;
    int nt = -1;
    if (n < N) {
        const GsCam cam = load_cam(viewmat, K);
        const SurfelFwd p = surfel_project_n(cam, n, means, quats, scales, W, H, near_plane, far_plane, radius_clip);
        if (p.valid) {
            int x0, y0, x1, y1;
            tile_range_exact(p.m2x, p.m2y, p.radius, tile_size, tile_w, tile_h, x0, y0, x1, y1);
            nt = (x1 - x0) * (y1 - y0);
        }
        tiles[n] = nt;
    }
    const unsigned nv = (unsigned)__popcll(__ballot(nt >= 0));
    const unsigned ni = gs_wave_sum_u32(nt > 0 ? (unsigned)nt : 0u);       // (every lane of the block is here)
    if (lane == 0) { s_v[wave] = nv; s_i[wave] = ni; }
    __syncthreads();
    if (tid == 0) {
        unsigned v = 0; long long i = 0;
#pragma unroll
        for (int w = 0; w < SF_WAVES; ++w) { v += s_v[w]; i += (long long)s_i[w]; }
        block_v[blockIdx.x] = (int32_t)v;
        block_i[blockIdx.x] = i;
    }
}

// S1 pass 2 (one workgroup): block_v -> exclusive prefix in place, counts = {V, I}
__global__ void __launch_bounds__(SF_BLOCK)
surfel_scan_kernel(int n_blocks, int32_t* __restrict__ block_v, const long long* __restrict__ block_i, long long* __restrict__ counts)
{
    __shared__ long long s_v[SF_BLOCK], s_i[SF_BLOCK];
    const int tid = threadIdx.x;
    const int per = (n_blocks + SF_BLOCK - 1) / SF_BLOCK;
    const int lo = tid * per, hi = min(n_blocks, lo + per);
    long long v = 0, i = 0;
    for (int b = lo; b < hi; ++b) { v += block_v[b]; i += block_i[b]; }
    s_v[tid] = v; s_i[tid] = i;
    __syncthreads();
    if (tid == 0) {
        long long av = 0, ai = 0;
        for (int t = 0; t < SF_BLOCK; ++t) { const long long x = s_v[t]; s_v[t] = av; av += x; ai += s_i[t]; }
        counts[0] = av; counts[1] = ai;
    }
    __syncthreads();
    long long base = s_v[tid];
    for (int b = lo; b < hi; ++b) { const int x = block_v[b]; block_v[b] = (int32_t)base; base += x; }
}

// S1 pass 3: the packed rows
template <bool SH>
__global__ void __launch_bounds__(SF_BLOCK)
surfel_write_kernel(int N, const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
                    const float* __restrict__ opacities, const float* __restrict__ colors, int Dc, const float* __restrict__ sh_coeffs, int sh_K,
                    int sh_degree, int depth_channel, const float* __restrict__ viewmat, const float* __restrict__ K, int W, int H,
                    float near_plane, float far_plane, float radius_clip, const int32_t* __restrict__ tiles,
                    const int32_t* __restrict__ block_base, int32_t* __restrict__ gaussian_ids, int32_t* __restrict__ radii,
                    float* __restrict__ means2d, float* __restrict__ depths, float* __restrict__ ray_transforms, float* __restrict__ normals,
                    float* __restrict__ opacities_packed, float* __restrict__ colors_packed, int32_t* __restrict__ tiles_per_gauss)
{
    __shared__ int s_w[SF_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x * SF_BLOCK + tid;
    const int nt = n < N ? tiles[n] : -1;
    const bool valid = nt >= 0;
    const unsigned long long bal = __ballot(valid);
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < SF_WAVES; ++w) if (w < wave) before += s_w[w];
    if (!valid) return;
    const size_t slot = (size_t)block_base[blockIdx.x] + (size_t)before;
    const GsCam cam = load_cam(viewmat, K);
    const SurfelFwd p = surfel_project_n(cam, n, means, quats, scales, W, H, near_plane, far_plane, radius_clip);
    gaussian_ids[slot] = n;
    radii[slot] = p.radius;
    means2d[2 * slot] = p.m2x; means2d[2 * slot + 1] = p.m2y;
    depths[slot] = p.depth;
#pragma unroll
    for (int i = 0; i < 9; ++i) ray_transforms[9 * slot + i] = p.M[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) normals[3 * slot + i] = p.nrm[i];
    opacities_packed[slot] = opacities[n];
    tiles_per_gauss[slot] = nt;
    const int C = Dc + depth_channel;
    if constexpr (SH) {
        const float mean[3] = { means[3 * (size_t)n], means[3 * (size_t)n + 1], means[3 * (size_t)n + 2] };
        float rgb[3];
        sh_color(cam, mean, sh_coeffs + (size_t)n * sh_K * 3, sh_K, sh_degree, rgb);
        colors_packed[slot * C] = rgb[0]; colors_packed[slot * C + 1] = rgb[1]; colors_packed[slot * C + 2] = rgb[2];
    } else {
        for (int k = 0; k < Dc; ++k) colors_packed[slot * C + k] = colors[(size_t)n * Dc + k];
    }
    if (depth_channel) colors_packed[slot * C + Dc] = p.depth;
}

// projection workspace: the tile count of every Gaussian, then per block of SF_BLOCK the visible and the intersection counts
struct SurfelProjWs { int32_t* tiles; int32_t* block_v; long long* block_i; size_t bytes; };
static SurfelProjWs surfel_project_ws(void* base, int N)
{
    const size_t n = N > 0 ? (size_t)N : 1, nb = (n + SF_BLOCK - 1) / SF_BLOCK;
    GsWs w(base, 256);
    SurfelProjWs r;
    r.tiles = w.take<int32_t>(n);
    r.block_v = w.take<int32_t>(nb);
    r.block_i = w.tail<long long>(nb);
    r.bytes = w.bytes();
    return r;
}
extern "C" size_t gs_surfel_project_ws_bytes(int N) { return surfel_project_ws(nullptr, N).bytes; }

extern "C" int gs_surfel_project_fwd(int N, const float* means, const float* quats, const float* scales, const float* opacities,
                                     const float* colors, int Dc, const float* sh_coeffs, int sh_K, int sh_degree, int depth_channel,
                                     const float* viewmat, const float* K, int W, int H, int tile_size, float near_plane, float far_plane,
                                     float radius_clip, int32_t* gaussian_ids, int32_t* radii, float* means2d, float* depths,
                                     float* ray_transforms, float* normals, float* opacities_packed, float* colors_packed,
                                     int32_t* tiles_per_gauss, void* ws, size_t ws_bytes, int64_t* counts, void* stream)
{
    GS_CHECK_ARG(N >= 0 && W > 0 && H > 0 && tile_size > 0, "bad sizes");
    GS_CHECK_ARG(counts != nullptr && ws != nullptr, "counts/ws must not be NULL");
    GS_CHECK_ARG(depth_channel == 0 || depth_channel == 1, "depth_channel is 0 or 1");
    const bool sh = sh_degree >= 0;
    GS_CHECK_ARG(sh_degree >= -1 && sh_degree <= 3, "sh_degree in -1..3");
    GS_CHECK_ARG(!sh || (sh_coeffs != nullptr && colors == nullptr && Dc == 3 && sh_K >= (sh_degree + 1) * (sh_degree + 1)),
                 "SH colours need sh_coeffs [N, sh_K >= (degree+1)^2, 3], colors NULL and Dc == 3");
    GS_CHECK_ARG(sh || Dc == 0 || colors != nullptr, "colors is NULL");
    GS_CHECK_ARG(Dc >= 0 && Dc + depth_channel >= 1 && Dc + depth_channel <= 4, "1..4 composited channels");
    GS_CHECK_ARG(colors_packed != nullptr, "colors_packed is NULL");
    const SurfelProjWs w = surfel_project_ws(ws, N);
    if (ws_bytes < w.bytes) { gs_set_error("gs_surfel_project_fwd: workspace too small"); return GS_ENOSPC; }
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) { GS_CHECK_HIP(gs_zero_async(counts, 2 * sizeof(int64_t), s)); return GS_OK; }
    const int nb = (N + SF_BLOCK - 1) / SF_BLOCK;
    const int tile_w = (W + tile_size - 1) / tile_size, tile_h = (H + tile_size - 1) / tile_size;
    hipLaunchKernelGGL(surfel_count_kernel, dim3(nb), dim3(SF_BLOCK), 0, s, N, means, quats, scales, viewmat, K, W, H, tile_size, tile_w,
                       tile_h, near_plane, far_plane, radius_clip, w.tiles, w.block_v, w.block_i);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(surfel_scan_kernel, dim3(1), dim3(SF_BLOCK), 0, s, nb, w.block_v, w.block_i, (long long*)counts);
    GS_CHECK_LAUNCH();
    if (sh)
        hipLaunchKernelGGL(surfel_write_kernel<true>, dim3(nb), dim3(SF_BLOCK), 0, s, N, means, quats, scales, opacities, colors, Dc, sh_coeffs,
                           sh_K, sh_degree, depth_channel, viewmat, K, W, H, near_plane, far_plane, radius_clip, w.tiles, w.block_v, gaussian_ids,
                           radii, means2d, depths, ray_transforms, normals, opacities_packed, colors_packed, tiles_per_gauss);
    else
        hipLaunchKernelGGL(surfel_write_kernel<false>, dim3(nb), dim3(SF_BLOCK), 0, s, N, means, quats, scales, opacities, colors, Dc, sh_coeffs,
                           sh_K, sh_degree, depth_channel, viewmat, K, W, H, near_plane, far_plane, radius_clip, w.tiles, w.block_v, gaussian_ids,
                           radii, means2d, depths, ray_transforms, normals, opacities_packed, colors_packed, tiles_per_gauss);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// S1': one thread per visible Gaussian; the rows of the invisible ones are zeroed by the entry point.
template <bool SH>
__global__ void __launch_bounds__(SF_BLOCK)
surfel_project_bwd_kernel(int V, int Dc, const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
                          const float* __restrict__ sh_coeffs, int sh_K, int sh_degree, const float* __restrict__ viewmat,
                          const float* __restrict__ K, const int32_t* __restrict__ gaussian_ids, const float* __restrict__ v_ray_transforms,
                          const float* __restrict__ v_means2d, const float* __restrict__ v_depths, const float* __restrict__ v_normals,
                          const float* __restrict__ v_opacities, const float* __restrict__ v_colors, int stride, float* __restrict__ g_means,
                          float* __restrict__ g_quats, float* __restrict__ g_scales, float* __restrict__ g_opacities,
                          float* __restrict__ g_colors, float* __restrict__ g_sh)
{
#pragma clang fp contract(fast)
    const int v = blockIdx.x * SF_BLOCK + threadIdx.x;
    if (v >= V) return;
    const size_t n = (size_t)gaussian_ids[v], row = (size_t)v * stride;
    const GsCam cam = load_cam(viewmat, K);
    const float mean[3] = { means[3 * n], means[3 * n + 1], means[3 * n + 2] };
    const float4 q4 = *reinterpret_cast<const float4*>(quats + 4 * n);
    const float s0 = scales[3 * n], s1 = scales[3 * n + 1];
    // forward intermediates: the frame bit for bit as the forward had it
    float mc[3], Rc[9];
    surfel_cam_mean(cam, mean, mc);
    surfel_cam_rot(cam, q4.x, q4.y, q4.z, q4.w, Rc);
    float M0[3], M1[3], M2[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float h0 = j == 0 ? s0 * Rc[0] : j == 1 ? s1 * Rc[1] : mc[0];
        const float h1 = j == 0 ? s0 * Rc[3] : j == 1 ? s1 * Rc[4] : mc[1];
        const float h2 = j == 0 ? s0 * Rc[6] : j == 1 ? s1 * Rc[7] : mc[2];
        M0[j] = cam.fx * h0 + cam.cx * h2; M1[j] = cam.fy * h1 + cam.cy * h2; M2[j] = h2;
    }
    float vM0[3], vM1[3], vM2[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { vM0[j] = v_ray_transforms[row + j]; vM1[j] = v_ray_transforms[row + 3 + j]; vM2[j] = v_ray_transforms[row + 6 + j]; }
    {   // means2d = (sum test M0 M2, sum test M1 M2) / d,  d = sum test M2^2,  test = (1, 1, -1)
        const float vmx = v_means2d[row], vmy = v_means2d[row + 1];
        const float d = M2[0] * M2[0] + M2[1] * M2[1] - M2[2] * M2[2];
        const float f = 1.0f / d;
        const float mx = f * (M0[0] * M2[0] + M0[1] * M2[1] - M0[2] * M2[2]);
        const float my = f * (M1[0] * M2[0] + M1[1] * M2[1] - M1[2] * M2[2]);
        const float vd = -(vmx * mx + vmy * my) * f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float t = j == 2 ? -f : f;
            vM0[j] += vmx * t * M2[j];
            vM1[j] += vmy * t * M2[j];
            vM2[j] += t * (vmx * M0[j] + vmy * M1[j]) + 2.0f * vd * (j == 2 ? -M2[j] : M2[j]);
        }
    }
    // M = K Hm
    float vH[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        vH[0 * 3 + j] = cam.fx * vM0[j];
        vH[1 * 3 + j] = cam.fy * vM1[j];
        vH[2 * 3 + j] = cam.cx * vM0[j] + cam.cy * vM1[j] + vM2[j];
    }
    float v_mc[3] = { vH[2], vH[5], vH[8] };
    if (v_depths) v_mc[2] += v_depths[row];
    const float sgn = surfel_normal_sign(Rc, mc);
    float vRc[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        vRc[i * 3 + 0] = s0 * vH[i * 3 + 0];
        vRc[i * 3 + 1] = s1 * vH[i * 3 + 1];
        vRc[i * 3 + 2] = sgn * v_normals[row + i];
    }
    const float gs0 = vH[0] * Rc[0] + vH[3] * Rc[3] + vH[6] * Rc[6];
    const float gs1 = vH[1] * Rc[1] + vH[4] * Rc[4] + vH[7] * Rc[7];
    float v_mean[3], v_Rq[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) v_mean[i] = cam.R[0 * 3 + i] * v_mc[0] + cam.R[1 * 3 + i] * v_mc[1] + cam.R[2 * 3 + i] * v_mc[2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v_Rq[i * 3 + j] = cam.R[0 * 3 + i] * vRc[j] + cam.R[1 * 3 + i] * vRc[3 + j] + cam.R[2 * 3 + i] * vRc[6 + j];
    // rotation matrix of the normalised quaternion (project_bwd_one's chain)
    const float inv = 1.0f / sqrtf(q4.y * q4.y + q4.z * q4.z + q4.w * q4.w + q4.x * q4.x);
    const float w = q4.x * inv, xq = q4.y * inv, yq = q4.z * inv, zq = q4.w * inv;
#define VR(i, j) v_Rq[(i) * 3 + (j)]
    float vqn[4];
    vqn[0] = 2.0f * (xq * (VR(2, 1) - VR(1, 2)) + yq * (VR(0, 2) - VR(2, 0)) + zq * (VR(1, 0) - VR(0, 1)));
    vqn[1] = 2.0f * (-2.0f * xq * (VR(1, 1) + VR(2, 2)) + yq * (VR(1, 0) + VR(0, 1)) + zq * (VR(2, 0) + VR(0, 2)) + w * (VR(2, 1) - VR(1, 2)));
    vqn[2] = 2.0f * (xq * (VR(1, 0) + VR(0, 1)) - 2.0f * yq * (VR(0, 0) + VR(2, 2)) + zq * (VR(2, 1) + VR(1, 2)) + w * (VR(0, 2) - VR(2, 0)));
    vqn[3] = 2.0f * (xq * (VR(2, 0) + VR(0, 2)) + yq * (VR(2, 1) + VR(1, 2)) - 2.0f * zq * (VR(0, 0) + VR(1, 1)) + w * (VR(1, 0) - VR(0, 1)));
#undef VR
    const float qn[4] = { w, xq, yq, zq };
    const float dotp = vqn[0] * qn[0] + vqn[1] * qn[1] + vqn[2] * qn[2] + vqn[3] * qn[3];
    if constexpr (SH) {
        const float v_rgb[3] = { v_colors[row], v_colors[row + 1], v_colors[row + 2] };
        sh_color_bwd(cam, mean, sh_coeffs + n * sh_K * 3, sh_K, sh_degree, true, v_rgb, g_sh + n * sh_K * 3, v_mean);
    } else {
        for (int k = 0; k < Dc; ++k) g_colors[n * Dc + k] = v_colors[row + k];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) g_means[3 * n + i] = v_mean[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) g_quats[4 * n + k] = (vqn[k] - dotp * qn[k]) * inv;
    g_scales[3 * n] = gs0; g_scales[3 * n + 1] = gs1; g_scales[3 * n + 2] = 0.0f;
    g_opacities[n] = v_opacities[row];
}

extern "C" int gs_surfel_project_bwd(int N, int V, int Dc, const float* means, const float* quats, const float* scales,
                                     const float* sh_coeffs, int sh_K, int sh_degree, const float* viewmat, const float* K,
                                     const int32_t* gaussian_ids, const float* v_ray_transforms, const float* v_means2d,
                                     const float* v_depths, const float* v_normals, const float* v_opacities, const float* v_colors,
                                     int stride, float* g_means, float* g_quats, float* g_scales, float* g_opacities, float* g_colors,
                                     float* g_sh, void* stream)
{
    GS_CHECK_ARG(N >= 0 && V >= 0 && V <= N && stride >= 1, "bad sizes");
    const bool sh = sh_degree >= 0;
    GS_CHECK_ARG(sh_degree >= -1 && sh_degree <= 3, "sh_degree in -1..3");
    GS_CHECK_ARG(!sh || (sh_coeffs != nullptr && g_sh != nullptr && sh_K >= (sh_degree + 1) * (sh_degree + 1)), "SH colours need sh_coeffs and g_sh");
    GS_CHECK_ARG(sh || Dc == 0 || g_colors != nullptr, "g_colors is NULL");
    GS_CHECK_ARG(g_means && g_quats && g_scales && g_opacities, "gradient outputs must not be NULL");
    hipStream_t s = (hipStream_t)stream;
    GS_CHECK_HIP(gs_zero_async(g_means, (size_t)N * 3 * 4, s));
    GS_CHECK_HIP(gs_zero_async(g_quats, (size_t)N * 4 * 4, s));
    GS_CHECK_HIP(gs_zero_async(g_scales, (size_t)N * 3 * 4, s));
    GS_CHECK_HIP(gs_zero_async(g_opacities, (size_t)N * 4, s));
    if (sh) GS_CHECK_HIP(gs_zero_async(g_sh, (size_t)N * sh_K * 3 * 4, s));
    else if (Dc > 0) GS_CHECK_HIP(gs_zero_async(g_colors, (size_t)N * Dc * 4, s));
    if (V == 0) return GS_OK;
    GS_CHECK_ARG(v_ray_transforms && v_means2d && v_normals && v_opacities && (v_colors || (!sh && Dc == 0)), "incoming gradients must not be NULL");
    const int nb = (V + SF_BLOCK - 1) / SF_BLOCK;
    if (sh)
        hipLaunchKernelGGL(surfel_project_bwd_kernel<true>, dim3(nb), dim3(SF_BLOCK), 0, s, V, Dc, means, quats, scales, sh_coeffs, sh_K, sh_degree,
                           viewmat, K, gaussian_ids, v_ray_transforms, v_means2d, v_depths, v_normals, v_opacities, v_colors, stride, g_means,
                           g_quats, g_scales, g_opacities, g_colors, g_sh);
    else
        hipLaunchKernelGGL(surfel_project_bwd_kernel<false>, dim3(nb), dim3(SF_BLOCK), 0, s, V, Dc, means, quats, scales, sh_coeffs, sh_K, sh_degree,
                           viewmat, K, gaussian_ids, v_ray_transforms, v_means2d, v_depths, v_normals, v_opacities, v_colors, stride, g_means,
                           g_quats, g_scales, g_opacities, g_colors, g_sh);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// alpha of one surfel at one pixel centre; the forward and the backward both call this, so every skip decision agrees bit for bit.
struct SurfelHit {
    float alpha, G, sx, sy, rzz, dx, dy;
    float hu[3], hv[3];
    bool ray;        // w3 < w2: the ray-splat intersection decides, else the screen-space low-pass filter
    bool clamped;    // min(0.999, .) active
};

// a * b - c * d with the rounding error of c * d recovered (Kahan)
__device__ __forceinline__ float sf_diff_of_products(float a, float b, float c, float d)
{
#pragma clang fp contract(off)
    const float w = c * d;
    const float e = __builtin_fmaf(-c, d, w);
    const float f = __builtin_fmaf(a, b, -w);
    return f + e;
}

__device__ __forceinline__ bool surfel_hit(const float* __restrict__ r /* staged record */, float px, float py, SurfelHit& h)
{
#pragma clang fp contract(off)
    // both steps cancel for a surfel seen at a grazing angle or close to the camera: the products are kept exact in explicit FMAs
    // (the same instructions in the forward and in the backward, whatever the contraction mode of the caller)
#pragma unroll
    for (int j = 0; j < 3; ++j) { h.hu[j] = __builtin_fmaf(px, r[6 + j], -r[j]); h.hv[j] = __builtin_fmaf(py, r[6 + j], -r[3 + j]); }
    const float zx = sf_diff_of_products(h.hu[1], h.hv[2], h.hu[2], h.hv[1]);
    const float zy = sf_diff_of_products(h.hu[2], h.hv[0], h.hu[0], h.hv[2]);
    const float zz = sf_diff_of_products(h.hu[0], h.hv[1], h.hu[1], h.hv[0]);
    if (zz == 0.0f) return false;
    h.rzz = 1.0f / zz;
    h.sx = zx * h.rzz; h.sy = zy * h.rzz;
    const float w3 = h.sx * h.sx + h.sy * h.sy;
    h.dx = r[9] - px; h.dy = r[10] - py;
    const float w2 = 2.0f * (h.dx * h.dx + h.dy * h.dy);
    h.ray = w3 < w2;
    const float sigma = 0.5f * (h.ray ? w3 : w2);
    if (!(sigma >= 0.0f)) return false;
    h.G = gs_exp_neg(sigma);
    const float a = r[11] * h.G;
    h.clamped = a > 0.999f;
    h.alpha = h.clamped ? 0.999f : a;
    return h.alpha >= (1.0f / 255.0f);
}

__device__ __forceinline__ void surfel_stage(float* __restrict__ dst, int g, int C, const float* __restrict__ ray_transforms,
                                             const float* __restrict__ means2d, const float* __restrict__ opacities,
                                             const float* __restrict__ normals, const float* __restrict__ colors)
{
#pragma unroll
    for (int i = 0; i < 9; ++i) dst[i] = ray_transforms[9 * (size_t)g + i];
    dst[9] = means2d[2 * (size_t)g]; dst[10] = means2d[2 * (size_t)g + 1];
    dst[11] = opacities[g];
#pragma unroll
    for (int i = 0; i < 3; ++i) dst[12 + i] = normals[3 * (size_t)g + i];
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[15 + k] = k < C ? colors[(size_t)g * C + k] : 0.0f;
}

// S5.  blockDim = (tile_size, tile_size), one pixel per thread.
template <int C, bool DIST>
__global__ void __launch_bounds__(SF_BLOCK)
surfel_raster_fwd_kernel(int W, int H, int tile_w, int n_tiles, int n_isects, const int32_t* __restrict__ offsets,
                         const int32_t* __restrict__ flatten_ids, const float* __restrict__ ray_transforms, const float* __restrict__ means2d,
                         const float* __restrict__ opacities, const float* __restrict__ colors, const float* __restrict__ normals,
                         const float* __restrict__ background, int depth_channel, float* __restrict__ render, float* __restrict__ alphas,
                         float* __restrict__ render_normals, float* __restrict__ render_distort, float* __restrict__ render_median,
                         int32_t* __restrict__ last_ids, float* __restrict__ final_T, float* __restrict__ final_D)
{
    __shared__ float s_rec[SF_BLOCK * SF_REC];
    const int nthreads = blockDim.x * blockDim.y, tid = threadIdx.y * blockDim.x + threadIdx.x;
    const int tile = blockIdx.y * tile_w + blockIdx.x;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    const bool inside = x < W && y < H;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const int start = offsets[tile], end = tile == n_tiles - 1 ? n_isects : offsets[tile + 1];
    const int n_batches = (end - start + nthreads - 1) / nthreads;
    bool done = !inside;
    float T = 1.0f, acc[C], nrm[3] = { 0.f, 0.f, 0.f }, distort = 0.0f, Dsum = 0.0f, median = 0.0f;
#pragma unroll
    for (int k = 0; k < C; ++k) acc[k] = 0.0f;
    int last = -1;
    for (int b = 0; b < n_batches; ++b) {
        if (__syncthreads_count(done) == nthreads) break;
        const int base = start + b * nthreads;
        if (base + tid < end) surfel_stage(s_rec + tid * SF_REC, flatten_ids[base + tid], C, ray_transforms, means2d, opacities, normals, colors);
        __syncthreads();
        const int cnt = min(nthreads, end - base);
        for (int j = 0; j < cnt && !done; ++j) {
            const float* r = s_rec + j * SF_REC;
            SurfelHit h;
            if (!surfel_hit(r, px, py, h)) continue;
            const float Tn = T * (1.0f - h.alpha);
            if (Tn <= 1e-4f) { done = true; break; }
            const float vis = h.alpha * T;
#pragma unroll
            for (int k = 0; k < C; ++k) acc[k] += vis * r[15 + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) nrm[k] += vis * r[12 + k];
            if (depth_channel) {
                const float d = r[15 + C - 1];
                if constexpr (DIST) {
                    distort += 2.0f * (vis * d * (1.0f - T) - vis * Dsum);
                    Dsum += vis * d;
                }
                if (T > 0.5f) median = d;
            }
            last = base + j;
            T = Tn;
        }
    }
    if (!inside) return;
    const size_t pix = (size_t)y * W + x;
    if (background) {
        const int nc = C - depth_channel;
        for (int k = 0; k < nc && k < 3; ++k) acc[k] += T * background[k];
    }
#pragma unroll
    for (int k = 0; k < C; ++k) render[pix * C + k] = acc[k];
    alphas[pix] = 1.0f - T;
#pragma unroll
    for (int k = 0; k < 3; ++k) render_normals[pix * 3 + k] = nrm[k];
    if (render_distort) render_distort[pix] = distort;
    render_median[pix] = median;
    last_ids[pix] = last;
    final_T[pix] = T;
    if (final_D) final_D[pix] = Dsum;
}

// S6.  per-Gaussian record of the packed gradients: v_M[9], v_means2d[2], v_opacity, v_normal[3], v_colour[C]
template <int C, bool DIST>
__global__ void __launch_bounds__(SF_BLOCK)
surfel_raster_bwd_kernel(int W, int H, int tile_w, const int32_t* __restrict__ offsets, const int32_t* __restrict__ flatten_ids,
                         const float* __restrict__ ray_transforms, const float* __restrict__ means2d, const float* __restrict__ opacities,
                         const float* __restrict__ colors, const float* __restrict__ normals, const float* __restrict__ background,
                         int depth_channel, const int32_t* __restrict__ last_ids, const float* __restrict__ final_T,
                         const float* __restrict__ final_D, const float* __restrict__ v_render, const float* __restrict__ v_alphas,
                         const float* __restrict__ v_normals, const float* __restrict__ v_distort, float* __restrict__ v_packed)
{
#pragma clang fp contract(fast)
    constexpr int NV = 15 + C;
    __shared__ float s_rec[SF_BLOCK * SF_REC];
    __shared__ float s_acc[SF_BLOCK * SF_REC];
    __shared__ int s_id[SF_BLOCK];
    __shared__ int s_last;
    const int nthreads = blockDim.x * blockDim.y, tid = threadIdx.y * blockDim.x + threadIdx.x, lane = tid & 63;
    const int tile = blockIdx.y * tile_w + blockIdx.x;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    const bool inside = x < W && y < H;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const size_t pix = inside ? (size_t)y * W + x : 0;
    const int start = offsets[tile];
    const int my_last = inside ? last_ids[pix] : -1;
    if (tid == 0) s_last = -1;
#pragma unroll
    for (int i = 0; i < SF_REC; ++i) s_acc[tid * SF_REC + i] = 0.0f;
    __syncthreads();
    if (my_last >= 0) atomicMax(&s_last, my_last);
    __syncthreads();
    const int top = s_last;                                   // walk [start, top], back to front
    const int n_walk = top >= start ? top - start + 1 : 0;
    const int n_batches = (n_walk + nthreads - 1) / nthreads;

    float gC[C], gN[3] = { 0.f, 0.f, 0.f }, gA = 0.0f, gDist = 0.0f;
#pragma unroll
    for (int k = 0; k < C; ++k) gC[k] = 0.0f;
    float T = 1.0f, Tfin = 1.0f, Dk = 0.0f, Dtot = 0.0f;
    if (inside) {
#pragma unroll
        for (int k = 0; k < C; ++k) gC[k] = v_render[pix * C + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) gN[k] = v_normals[pix * 3 + k];
        gA = v_alphas[pix];
        T = Tfin = final_T[pix];
        if constexpr (DIST) { gDist = v_distort[pix]; Dk = Dtot = final_D[pix]; }
    }
    float tail = -gA;                                          // dL/dT_final: the background term minus the alpha term
    if (background) {
        const int nc = C - depth_channel;
        for (int k = 0; k < nc && k < 3; ++k) tail += gC[k] * background[k];
    }
    tail *= Tfin;
    float S = 0.0f;                                            // sum over the Gaussians behind of vis * dL/dvis
    for (int b = 0; b < n_batches; ++b) {
        const int hi = top - b * nthreads;                    // list index of staged entry 0; entry j is hi - j
        const int cnt = min(nthreads, hi - start + 1);
        __syncthreads();                                       // the commit of the batch before has read s_rec / s_id
        if (tid < cnt) {
            const int g = flatten_ids[hi - tid];
            s_id[tid] = g;
            surfel_stage(s_rec + tid * SF_REC, g, C, ray_transforms, means2d, opacities, normals, colors);
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float* r = s_rec + j * SF_REC;
            float val[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) val[i] = 0.0f;
            SurfelHit h;
            const bool hit = (hi - j <= my_last) && surfel_hit(r, px, py, h);
            if (hit) {
                const float ra = 1.0f / (1.0f - h.alpha);
                const float Tp = T * ra;                       // transmittance in front of this Gaussian
                const float vis = h.alpha * Tp;
                float f = gN[0] * r[12] + gN[1] * r[13] + gN[2] * r[14];
#pragma unroll
                for (int k = 0; k < C; ++k) f += gC[k] * r[15 + k];
#pragma unroll
                for (int k = 0; k < C; ++k) val[15 + k] = vis * gC[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) val[12 + k] = vis * gN[k];
                if constexpr (DIST) {
                    // distort = 2 sum_{j<k} vis_j vis_k (d_k - d_j); prefix sums from (T, D) here, suffix sums from the stored finals
                    const float d = r[15 + C - 1];
                    const float Wp = 1.0f - Tp, Dp = Dk - vis * d;
                    const float Wb = T - Tfin, Db = Dtot - Dk;     // weight and depth-weight of the Gaussians behind
                    f += gDist * 2.0f * ((d * Wp - Dp) + (Db - d * Wb));
                    val[15 + C - 1] += gDist * 2.0f * vis * (Wp - Wb);
                    Dk = Dp;
                }
                const float v_alpha = f * Tp - (S + tail) * ra;
                S += vis * f;
                T = Tp;
                if (!h.clamped) {
                    val[11] = h.G * v_alpha;
                    const float v_sigma = -h.alpha * v_alpha;
                    if (h.ray) {
                        const float vsx = v_sigma * h.sx, vsy = v_sigma * h.sy;
                        const float vz[3] = { vsx * h.rzz, vsy * h.rzz, -(vsx * h.sx + vsy * h.sy) * h.rzz };
                        const float vhu[3] = { h.hv[1] * vz[2] - h.hv[2] * vz[1], h.hv[2] * vz[0] - h.hv[0] * vz[2], h.hv[0] * vz[1] - h.hv[1] * vz[0] };
                        const float vhv[3] = { vz[1] * h.hu[2] - vz[2] * h.hu[1], vz[2] * h.hu[0] - vz[0] * h.hu[2], vz[0] * h.hu[1] - vz[1] * h.hu[0] };
#pragma unroll
                        for (int k = 0; k < 3; ++k) { val[k] = -vhu[k]; val[3 + k] = -vhv[k]; val[6 + k] = px * vhu[k] + py * vhv[k]; }
                    } else {
                        val[9] = v_sigma * 2.0f * h.dx; val[10] = v_sigma * 2.0f * h.dy;
                    }
                }
            }
            if (__ballot(hit) != 0ull) {                       // wave-uniform: every lane of the wave takes the reduction together
                float out[GsBfly<NV>::N4];
                GsBfly<NV>::reduce(val, out, lane);
                if (lane < 16) {
#pragma unroll
                    for (int q = 0; q < GsBfly<NV>::N4; ++q) {
                        const int idx = GsBfly<NV>::owned_index(lane, q);
                        if (idx < NV) atomicAdd(&s_acc[j * SF_REC + idx], out[q]);
                    }
                }
            }
        }
        __syncthreads();
        if (tid < cnt) {                                       // one global atomic per value and Gaussian of the tile
            float* dst = v_packed + (size_t)s_id[tid] * SF_REC;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const float a = s_acc[tid * SF_REC + i];
                if (a != 0.0f) gs_atomic_add(dst + i, a);
                s_acc[tid * SF_REC + i] = 0.0f;
            }
        }
    }
}

__global__ void __launch_bounds__(SF_BLOCK)
surfel_densify_kernel(int V, const float* __restrict__ depths, const float* __restrict__ v_packed, float* __restrict__ v_densify)
{
    const int v = blockIdx.x * SF_BLOCK + threadIdx.x;
    if (v >= V) return;
    const float d = depths[v];
    v_densify[2 * (size_t)v] = d * v_packed[(size_t)v * SF_REC + 2];
    v_densify[2 * (size_t)v + 1] = d * v_packed[(size_t)v * SF_REC + 5];
}

static int surfel_raster_args(int W, int H, int tile_size, int C, int depth_channel, int distloss, int64_t n_isects)
{
    GS_CHECK_ARG(W > 0 && H > 0, "bad image size");
    GS_CHECK_ARG(tile_size == 8 || tile_size == 16, "tile_size 8 or 16");
    GS_CHECK_ARG(C == 1 || C == 3 || C == 4, "1, 3 or 4 composited channels");
    GS_CHECK_ARG(depth_channel == 0 || depth_channel == 1, "depth_channel is 0 or 1");
    GS_CHECK_ARG(!distloss || depth_channel, "distloss needs the depth channel");
    GS_CHECK_ARG(n_isects >= 0 && n_isects < ((int64_t)1 << 31), "n_isects out of range");
    return GS_OK;
}

extern "C" int gs_surfel_grad_stride(void) { return SF_REC; }

// (<3, true> is built but can never be launched: surfel_raster_args and rasterization_2dgs both refuse distloss without the depth
// channel, and C == 3 is the mode without one.  The five launchable instantiations are the ones tests/test_gpu_surfel_budget.py runs.)
#define SF_DISPATCH(KERNEL, ...)                                                                        \
    do {                                                                                                \
        if (distloss) {                                                                                 \
            if (C == 1) hipLaunchKernelGGL((KERNEL<1, true>), grid, block, 0, s, __VA_ARGS__);          \
            else if (C == 3) hipLaunchKernelGGL((KERNEL<3, true>), grid, block, 0, s, __VA_ARGS__);     \
            else hipLaunchKernelGGL((KERNEL<4, true>), grid, block, 0, s, __VA_ARGS__);                 \
        } else {                                                                                        \
            if (C == 1) hipLaunchKernelGGL((KERNEL<1, false>), grid, block, 0, s, __VA_ARGS__);         \
            else if (C == 3) hipLaunchKernelGGL((KERNEL<3, false>), grid, block, 0, s, __VA_ARGS__);    \
            else hipLaunchKernelGGL((KERNEL<4, false>), grid, block, 0, s, __VA_ARGS__);                \
        }                                                                                               \
    } while (0)

extern "C" int gs_surfel_raster_fwd(int W, int H, int tile_size, int C, int depth_channel, int distloss, int V, const float* ray_transforms,
                                    const float* means2d, const float* opacities, const float* colors, const float* normals,
                                    const float* background, int64_t n_isects, const int32_t* offsets, const int32_t* flatten_ids,
                                    float* render, float* alphas, float* render_normals, float* render_distort, float* render_median,
                                    int32_t* last_ids, float* final_T, float* final_D, void* stream)
{
    const int rc = surfel_raster_args(W, H, tile_size, C, depth_channel, distloss, n_isects);
    if (rc != GS_OK) return rc;
    GS_CHECK_ARG(V >= 0 && render && alphas && render_normals && render_median && last_ids && final_T && offsets, "outputs must not be NULL");
    GS_CHECK_ARG(!distloss || (render_distort && final_D), "distloss needs render_distort and final_D");
    GS_CHECK_ARG(n_isects == 0 || (flatten_ids && ray_transforms && means2d && opacities && colors && normals), "inputs must not be NULL");
    hipStream_t s = (hipStream_t)stream;
    const int tile_w = (W + tile_size - 1) / tile_size, tile_h = (H + tile_size - 1) / tile_size;
    const dim3 grid(tile_w, tile_h), block(tile_size, tile_size);
    SF_DISPATCH(surfel_raster_fwd_kernel, W, H, tile_w, tile_w * tile_h, (int)n_isects, offsets, flatten_ids, ray_transforms, means2d, opacities,
                colors, normals, background, depth_channel, render, alphas, render_normals, render_distort, render_median, last_ids, final_T,
                final_D);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

extern "C" int gs_surfel_raster_bwd(int W, int H, int tile_size, int C, int depth_channel, int distloss, int V, const float* ray_transforms,
                                    const float* means2d, const float* opacities, const float* colors, const float* normals,
                                    const float* depths, const float* background, int64_t n_isects, const int32_t* offsets,
                                    const int32_t* flatten_ids, const int32_t* last_ids, const float* final_T, const float* final_D,
                                    const float* v_render, const float* v_alphas, const float* v_normals, const float* v_distort,
                                    float* v_packed, float* v_densify, void* stream)
{
    const int rc = surfel_raster_args(W, H, tile_size, C, depth_channel, distloss, n_isects);
    if (rc != GS_OK) return rc;
    GS_CHECK_ARG(V >= 0 && last_ids && final_T && offsets && v_render && v_alphas && v_normals, "inputs must not be NULL");
    GS_CHECK_ARG(!distloss || (v_distort && final_D), "distloss needs v_distort and final_D");
    GS_CHECK_ARG(V == 0 || (v_packed && v_densify && depths), "outputs must not be NULL");
    hipStream_t s = (hipStream_t)stream;
    if (V == 0) return GS_OK;
    GS_CHECK_HIP(gs_zero_async(v_packed, (size_t)V * SF_REC * sizeof(float), s));
    const int tile_w = (W + tile_size - 1) / tile_size, tile_h = (H + tile_size - 1) / tile_size;
    const dim3 grid(tile_w, tile_h), block(tile_size, tile_size);
    SF_DISPATCH(surfel_raster_bwd_kernel, W, H, tile_w, offsets, flatten_ids, ray_transforms, means2d, opacities, colors, normals, background,
                depth_channel, last_ids, final_T, final_D, v_render, v_alphas, v_normals, v_distort, v_packed);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(surfel_densify_kernel, dim3((V + SF_BLOCK - 1) / SF_BLOCK), dim3(SF_BLOCK), 0, s, V, depths, v_packed, v_densify);
    GS_CHECK_LAUNCH();
    return GS_OK;
}
