// gs_poisson.hip -- the hot paths of differentiable Poisson surface reconstruction (Shape-as-Points), the reference's
// rfstudio/graphics/_mesh/_dpsr/ops.py: oriented points -> periodic indicator grid by a spectral solve -> mesh.
//   gs_grid_splat               point_rasterize: periodic trilinear scatter of values[N,C] into grid[C,R0,R1,R2], bit-reproducible
//                               (64-bit fixed-point integer atomics, one power-of-two scale per call from max |v| on the device)
//   gs_grid_sample_fwd / _bwd   grid_interp, the adjoint gather, and the gather of the weight derivatives (no atomics)
//   gs_poisson_spectral_fwd/bwd one pass over S[3,R0,R1,R2/2+1]: Gaussian filter, -i omega_d, regularised Laplacian, zeroed DC
//   gs_grid_pack_volume         phi -> the interleaved (value, weight 1) volume gs_tsdf_extract_* triangulates
//   gs_grid_vertex_normals      normalise(grad phi) at vertices that lie on grid edges
// The FFTs are the caller's (hipFFT through torch.fft).  The weights come from csrc/gs_gridinterp_dev.h in all four directions.
#include "gs_gridinterp_dev.h"
#include "gs_ws.h"

#define PS_BLOCK 256

static bool ps_res_ok(int R0, int R1, int R2)
{
    return R0 >= 4 && R1 >= 4 && R2 >= 4 && (int64_t)R0 * R1 * R2 < ((int64_t)1 << 31);
}


// ------------------------------------------------------------------------------------------------ splat
// workspace: [ max |v| bits u32, padded to 16 bytes | C * R0 R1 R2 fixed-point accumulators i64 ]
constexpr size_t PS_HEAD = 16;

// max |v| over the rows that take part (bit patterns of non-negative floats order like unsigned integers; a NaN orders above inf)
static __global__ void __launch_bounds__(PS_BLOCK) ps_max_kernel(long long N, int C, GiRes G, const float* __restrict__ points,
                                                                 const float* __restrict__ values, unsigned* __restrict__ gmax_bits)
{
    __shared__ unsigned red[PS_BLOCK / 64];
    unsigned m = 0u;
    for (long long n = (long long)blockIdx.x * PS_BLOCK + threadIdx.x; n < N; n += (long long)gridDim.x * PS_BLOCK) {
        GiCell c;
        if (!gi_locate(points + 3 * n, G, c)) continue;
        for (int q = 0; q < C; ++q) m = max(m, (unsigned)__float_as_int(fabsf(values[n * C + q])));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PS_BLOCK / 64; ++w) m = max(m, red[w]);
        if (m != 0u) atomicMax(gmax_bits, m);
    }
}

// e such that N gmax 2^e < 2^62: no node sum can overflow (every weight is <= 1), and an addend 2^-14 of the largest one
// keeps 24 bits up to N = 2^24
__device__ __forceinline__ int ps_fx_exponent(long long N, float gmax)
{
    int ex;
    frexp((double)N * (double)gmax, &ex);                                           // value < 2^ex
    return 62 - ex;
}

template <int C>
static __global__ void __launch_bounds__(PS_BLOCK) ps_splat_kernel(long long N, GiRes G, long long cells, const float* __restrict__ points,
                                                                   const float* __restrict__ values,
                                                                   const unsigned* __restrict__ gmax_bits,
                                                                   unsigned long long* __restrict__ acc)
{
    const long long n = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (n >= N) return;
    const float gmax = __int_as_float((int)*gmax_bits);
    if (!(gmax > 0.0f) || !(gmax < 3.0e38f)) return;                                // all zero, or non-finite values: the convert pass decides
    GiCell c;
    if (!gi_locate(points + 3 * n, G, c)) return;
    const double up = ldexp(1.0, ps_fx_exponent(N, gmax));
    float w[3][2];
    gi_axis_weights(c, w);
    float v[C];
#pragma unroll
    for (int q = 0; q < C; ++q) v[q] = values[n * C + q];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float wk = gi_weight(w, k);
        const long long node = gi_node(c, G, k);                                    // < cells: lo and hi are in [0, R)
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const float t = wk * v[q];                                              // one fp32 rounding, then exact in double
            const long long fx = __double2ll_rn((double)t * up);
            if (fx != 0) atomicAdd(&acc[(long long)q * cells + node], (unsigned long long)fx);
        }
    }
}

static __global__ void __launch_bounds__(PS_BLOCK) ps_convert_kernel(long long N, long long total, const unsigned* __restrict__ gmax_bits,
                                                                     const long long* __restrict__ acc, float* __restrict__ grid)
{
    const float gmax = __int_as_float((int)*gmax_bits);
    const bool zero = gmax == 0.0f;
    const bool bad = !zero && (!(gmax > 0.0f) || !(gmax < 3.0e38f));                // a NaN or inf value in a row that takes part
    const double down = (zero || bad) ? 0.0 : ldexp(1.0, -ps_fx_exponent(N, gmax));
    for (long long i = (long long)blockIdx.x * PS_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * PS_BLOCK)
        grid[i] = bad ? __int_as_float(0x7fc00000) : (float)((double)acc[i] * down);
}

// ------------------------------------------------------------------------------------------------ sample
template <int C>
static __global__ void __launch_bounds__(PS_BLOCK) ps_sample_fwd_kernel(long long N, GiRes G, long long cells, const float* __restrict__ grid,
                                                                        const float* __restrict__ points, float* __restrict__ out)
{
    const long long n = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (n >= N) return;
    float r[C];
#pragma unroll
    for (int q = 0; q < C; ++q) r[q] = 0.0f;
    GiCell c;
    if (gi_locate(points + 3 * n, G, c)) {
        float w[3][2];
        gi_axis_weights(c, w);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float wk = gi_weight(w, k);
            const long long node = gi_node(c, G, k);
#pragma unroll
            for (int q = 0; q < C; ++q) r[q] = fmaf(wk, grid[(long long)q * cells + node], r[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < C; ++q) out[n * C + q] = r[q];
}

// g_points[n, a] = sum_c cot[n, c] * sum_k (d weight_k / d p_a) grid[c, node_k]
template <int C>
static __global__ void __launch_bounds__(PS_BLOCK) ps_sample_bwd_kernel(long long N, GiRes G, long long cells, const float* __restrict__ grid,
                                                                        const float* __restrict__ points, const float* __restrict__ cot,
                                                                        float* __restrict__ g_points)
{
    const long long n = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (n >= N) return;
    float g[3] = {0.0f, 0.0f, 0.0f};
    GiCell c;
    if (gi_locate(points + 3 * n, G, c)) {
        float w[3][2];
        gi_axis_weights(c, w);
        float v[C];
#pragma unroll
        for (int q = 0; q < C; ++q) v[q] = cot[n * C + q];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long node = gi_node(c, G, k);
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < C; ++q) s = fmaf(v[q], grid[(long long)q * cells + node], s);
#pragma unroll
            for (int a = 0; a < 3; ++a) g[a] = fmaf(gi_dweight(w, G, k, a), s, g[a]);
        }
    }
    g_points[3 * n + 0] = g[0];
    g_points[3 * n + 1] = g[1];
    g_points[3 * n + 2] = g[2];
}

// ------------------------------------------------------------------------------------------------ spectral step
struct PsSpec {
    int R0, R1, R2, H;                              // H = R2 / 2 + 1
    long long plane;                                // R0 R1 H: one component of S
    double sigma;
};

// integer frequency of index i: numpy's fftfreq (the Nyquist term of an even size is -R/2) and rfftfreq (+R/2)
__device__ __forceinline__ int ps_fftfreq(int i, int R) { return i <= (R - 1) / 2 ? i : i - R; }

// omega[3], the filter G and the denominator (the callers divide: IEEE division) of element m; false at DC
__device__ __forceinline__ bool ps_coeff(const PsSpec& P, long long m, float (&omega)[3], float& filt, float& denom)
{
#pragma clang fp contract(off)
    const int i2 = (int)(m % P.H);
    const long long r = m / P.H;
    const int i1 = (int)(r % P.R1), i0 = (int)(r / P.R1);
    const int k0 = ps_fftfreq(i0, P.R0), k1 = ps_fftfreq(i1, P.R1), k2 = i2;
    const float two_pi = 6.283185307179586f;
    omega[0] = (float)k0 * two_pi;
    omega[1] = (float)k1 * two_pi;
    omega[2] = (float)k2 * two_pi;
    const double kk = (double)k0 * k0 + (double)k1 * k1 + (double)k2 * k2;
    filt = (float)exp(-2.0 * P.sigma * P.sigma * kk);                               // float64, then cast: as the reference builds it
    const float lap = -((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2]);
    denom = lap + 1e-6f;
    return !(i0 == 0 && i1 == 0 && i2 == 0);
}

// Phi = sum_d (-i) (G S_d) omega_d / (-|omega|^2 + 1e-6),  Phi(0) = 0; operation order of DPSR.forward
static __global__ void __launch_bounds__(PS_BLOCK) ps_spectral_fwd_kernel(PsSpec P, const float2* __restrict__ S, float2* __restrict__ Phi)
{
#pragma clang fp contract(off)
    const long long m = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (m >= P.plane) return;
    float omega[3], filt, denom;
    const bool live = ps_coeff(P, m, omega, filt, denom);
    float re = 0.0f, im = 0.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float2 s = S[(long long)d * P.plane + m];
        const float nr = s.x * filt, ni = s.y * filt;
        re += ni * omega[d];                                                        // -i (nr + i ni) = ni - i nr
        im += -nr * omega[d];
    }
    Phi[m] = live ? make_float2(re / denom, im / denom) : make_float2(0.0f, 0.0f);
}

// the adjoint: g_S_d = conj(c_d) g_Phi with c_d = -i G omega_d / denom, i.e. (+i) (G omega_d) (g_Phi / denom)
static __global__ void __launch_bounds__(PS_BLOCK) ps_spectral_bwd_kernel(PsSpec P, const float2* __restrict__ gPhi, float2* __restrict__ gS)
{
#pragma clang fp contract(off)
    const long long m = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (m >= P.plane) return;
    float omega[3], filt, denom;
    const bool live = ps_coeff(P, m, omega, filt, denom);
    const float2 g = gPhi[m];
    const float tr = live ? g.x / denom : 0.0f, ti = live ? g.y / denom : 0.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float a = omega[d] * filt;
        gS[(long long)d * P.plane + m] = make_float2(-ti * a, tr * a);
    }
}

// ------------------------------------------------------------------------------------------------ mesh hand-off
static __global__ void __launch_bounds__(PS_BLOCK) ps_pack_kernel(long long total, const float* __restrict__ phi, float2* __restrict__ volume)
{
    for (long long i = (long long)blockIdx.x * PS_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * PS_BLOCK)
        volume[i] = make_float2(phi[i], 1.0f);
}

__device__ __forceinline__ int ps_wrap(int i, int R)
{
    i %= R;
    return i < 0 ? i + R : i;
}

// central-difference gradient of phi at node (i0, i1, i2), periodic, per unit of p = i / R: 0.5 R_a (phi[i + e_a] - phi[i - e_a])
__device__ __forceinline__ void ps_node_grad(const GiRes& G, const float* __restrict__ phi, const int (&i)[3], float (&g)[3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int p[3] = {i[0], i[1], i[2]}, q[3] = {i[0], i[1], i[2]};
        p[a] = ps_wrap(i[a] + 1, G.R[a]);
        q[a] = ps_wrap(i[a] - 1, G.R[a]);
        const float hi = phi[((long long)p[0] * G.R[1] + p[1]) * G.R[2] + p[2]];
        const float lo = phi[((long long)q[0] * G.R[1] + q[1]) * G.R[2] + q[2]];
        g[a] = (hi - lo) * (0.5f * (float)G.R[a]);
    }
}

// vertices in NODE units (vertex a = node index + fraction along at most one axis).  The gradient is interpolated linearly between
// the edge's two nodes; every index is wrapped, so no vertex can address outside phi.
static __global__ void __launch_bounds__(PS_BLOCK) ps_normals_kernel(long long V, GiRes G, const float* __restrict__ phi,
                                                                     const float* __restrict__ verts, float* __restrict__ normals)
{
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * PS_BLOCK + threadIdx.x;
    if (n >= V) return;
    float out[3] = {0.0f, 0.0f, 0.0f};
    const float x[3] = {verts[3 * n], verts[3 * n + 1], verts[3 * n + 2]};
    if (fabsf(x[0]) < 1.0e9f && fabsf(x[1]) < 1.0e9f && fabsf(x[2]) < 1.0e9f) {   // (a NaN fails) the float -> int below is in range
        int lo[3], axis = 0;
        float t = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float fl = floorf(x[a]);
            const float f = x[a] - fl;
            lo[a] = ps_wrap((int)fl, G.R[a]);
            if (f > t) { t = f; axis = a; }                                         // the edge's axis: the one fractional coordinate
        }
        int hi[3] = {lo[0], lo[1], lo[2]};
        hi[axis] = ps_wrap(lo[axis] + 1, G.R[axis]);
        float ga[3], gb[3];
        ps_node_grad(G, phi, lo, ga);
        ps_node_grad(G, phi, hi, gb);
        float g[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] = ga[a] + t * (gb[a] - ga[a]);
        const float m = fmaxf(fabsf(g[0]), fmaxf(fabsf(g[1]), fabsf(g[2])));
        if (m > 0.0f && m < 3.0e38f) {                                              // scaled first: no overflow or underflow in the norm
            const float s0 = g[0] / m, s1 = g[1] / m, s2 = g[2] / m;
            const float len = sqrtf((s0 * s0 + s1 * s1) + s2 * s2);
            out[0] = s0 / len; out[1] = s1 / len; out[2] = s2 / len;
        }
    }
    normals[3 * n + 0] = out[0];
    normals[3 * n + 1] = out[1];
    normals[3 * n + 2] = out[2];
}

static inline int ps_grid(long long items, int cap = 1 << 30)
{
    const long long b = (items + PS_BLOCK - 1) / PS_BLOCK;
    return (int)(b < 1 ? 1 : (b < cap ? b : cap));
}

template <int C>
static void ps_launch_splat(long long N, GiRes G, long long cells, const float* points, const float* values, const unsigned* gmax,
                            unsigned long long* acc, hipStream_t s)
{
    hipLaunchKernelGGL(ps_splat_kernel<C>, dim3(ps_grid(N)), dim3(PS_BLOCK), 0, s, N, G, cells, points, values, gmax, acc);
}
template <int C>
static void ps_launch_sample_fwd(long long N, GiRes G, long long cells, const float* grid, const float* points, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(ps_sample_fwd_kernel<C>, dim3(ps_grid(N)), dim3(PS_BLOCK), 0, s, N, G, cells, grid, points, out);
}
template <int C>
static void ps_launch_sample_bwd(long long N, GiRes G, long long cells, const float* grid, const float* points, const float* cot,
                                 float* g_points, hipStream_t s)
{
    hipLaunchKernelGGL(ps_sample_bwd_kernel<C>, dim3(ps_grid(N)), dim3(PS_BLOCK), 0, s, N, G, cells, grid, points, cot, g_points);
}

#define PS_DISPATCH_C(fn, ...)                      \
    switch (C) {                                    \
    case 1: fn<1>(__VA_ARGS__); break;              \
    case 2: fn<2>(__VA_ARGS__); break;              \
    case 3: fn<3>(__VA_ARGS__); break;              \
    default: fn<4>(__VA_ARGS__); break;             \
    }

// ------------------------------------------------------------------------------------------------ entry points
extern "C" {

size_t gs_grid_splat_ws_bytes(int C, int R0, int R1, int R2)
{
    if (!ps_res_ok(R0, R1, R2) || C < 1 || C > 4) return 0;
    return PS_HEAD + gs_align_up((size_t)C * (size_t)R0 * R1 * R2 * 8, 16);
}

int gs_grid_splat(int64_t N, int C, int R0, int R1, int R2, const float* points, const float* values, float* grid, void* ws,
                  size_t ws_bytes, void* stream)
{
    GS_CHECK_ARG(ps_res_ok(R0, R1, R2), "resolution must be >= 4 per axis with fewer than 2^31 nodes");
    GS_CHECK_ARG(C >= 1 && C <= 4, "C must be in [1, 4]");
    GS_CHECK_ARG(N >= 0 && N < ((int64_t)1 << 31), "N must be in [0, 2^31)");
    const size_t need = gs_grid_splat_ws_bytes(C, R0, R1, R2);
    if (!ws || ws_bytes < need) {
        gs_set_error("%s: workspace too small (%zu < %zu)", __func__, ws ? ws_bytes : (size_t)0, need);
        return ws ? GS_ENOSPC : GS_EINVAL;
    }
    GS_CHECK_ARG(grid && (N == 0 || (points && values)), "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long long cells = (long long)R0 * R1 * R2;
    GiRes G{{R0, R1, R2}};
    unsigned* gmax = (unsigned*)ws;
    unsigned long long* acc = (unsigned long long*)((char*)ws + PS_HEAD);
    GS_CHECK_HIP(gs_zero_async(ws, need, s));
    if (N > 0) {
        hipLaunchKernelGGL(ps_max_kernel, dim3(ps_grid(N, 2048)), dim3(PS_BLOCK), 0, s, (long long)N, C, G, points, values, gmax);
        GS_CHECK_LAUNCH();
        PS_DISPATCH_C(ps_launch_splat, (long long)N, G, cells, points, values, gmax, acc, s);
        GS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ps_convert_kernel, dim3(ps_grid(C * cells, 8192)), dim3(PS_BLOCK), 0, s, (long long)N, C * cells, gmax,
                       (const long long*)acc, grid);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_grid_sample_fwd(int64_t N, int C, int R0, int R1, int R2, const float* grid, const float* points, float* out, void* stream)
{
    GS_CHECK_ARG(ps_res_ok(R0, R1, R2), "resolution must be >= 4 per axis with fewer than 2^31 nodes");
    GS_CHECK_ARG(C >= 1 && C <= 4, "C must be in [1, 4]");
    GS_CHECK_ARG(N >= 0 && N < ((int64_t)1 << 31), "N must be in [0, 2^31)");
    if (N == 0) return GS_OK;
    GS_CHECK_ARG(grid && points && out, "null pointer");
    GiRes G{{R0, R1, R2}};
    PS_DISPATCH_C(ps_launch_sample_fwd, (long long)N, G, (long long)R0 * R1 * R2, grid, points, out, (hipStream_t)stream);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_grid_sample_bwd(int64_t N, int C, int R0, int R1, int R2, const float* grid, const float* points, const float* cot,
                       float* g_points, void* stream)
{
    GS_CHECK_ARG(ps_res_ok(R0, R1, R2), "resolution must be >= 4 per axis with fewer than 2^31 nodes");
    GS_CHECK_ARG(C >= 1 && C <= 4, "C must be in [1, 4]");
    GS_CHECK_ARG(N >= 0 && N < ((int64_t)1 << 31), "N must be in [0, 2^31)");
    if (N == 0) return GS_OK;
    GS_CHECK_ARG(grid && points && cot && g_points, "null pointer");
    GiRes G{{R0, R1, R2}};
    PS_DISPATCH_C(ps_launch_sample_bwd, (long long)N, G, (long long)R0 * R1 * R2, grid, points, cot, g_points, (hipStream_t)stream);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_poisson_spectral_fwd(int R0, int R1, int R2, double sigma, const float* S, float* Phi, void* stream)
{
    GS_CHECK_ARG(ps_res_ok(R0, R1, R2), "resolution must be >= 4 per axis with fewer than 2^31 nodes");
    GS_CHECK_ARG(sigma >= 0.0 && sigma < 1.0e6, "sigma must be finite and >= 0");
    GS_CHECK_ARG(S && Phi, "null pointer");
    const int H = R2 / 2 + 1;
    PsSpec P{R0, R1, R2, H, (long long)R0 * R1 * H, sigma};
    hipLaunchKernelGGL(ps_spectral_fwd_kernel, dim3(ps_grid(P.plane)), dim3(PS_BLOCK), 0, (hipStream_t)stream, P, (const float2*)S,
                       (float2*)Phi);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_poisson_spectral_bwd(int R0, int R1, int R2, double sigma, const float* g_Phi, float* g_S, void* stream)
{
    GS_CHECK_ARG(ps_res_ok(R0, R1, R2), "resolution must be >= 4 per axis with fewer than 2^31 nodes");
    GS_CHECK_ARG(sigma >= 0.0 && sigma < 1.0e6, "sigma must be finite and >= 0");
    GS_CHECK_ARG(g_Phi && g_S, "null pointer");
    const int H = R2 / 2 + 1;
    PsSpec P{R0, R1, R2, H, (long long)R0 * R1 * H, sigma};
    hipLaunchKernelGGL(ps_spectral_bwd_kernel, dim3(ps_grid(P.plane)), dim3(PS_BLOCK), 0, (hipStream_t)stream, P, (const float2*)g_Phi,
                       (float2*)g_S);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_grid_pack_volume(int R0, int R1, int R2, const float* phi, float* volume, void* stream)
{
    GS_CHECK_ARG(ps_res_ok(R0, R1, R2), "resolution must be >= 4 per axis with fewer than 2^31 nodes");
    GS_CHECK_ARG(phi && volume, "null pointer");
    const long long total = (long long)R0 * R1 * R2;
    hipLaunchKernelGGL(ps_pack_kernel, dim3(ps_grid(total, 8192)), dim3(PS_BLOCK), 0, (hipStream_t)stream, total, phi, (float2*)volume);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

int gs_grid_vertex_normals(int R0, int R1, int R2, const float* phi, int64_t V, const float* vertices, float* normals, void* stream)
{
    GS_CHECK_ARG(ps_res_ok(R0, R1, R2), "resolution must be >= 4 per axis with fewer than 2^31 nodes");
    GS_CHECK_ARG(V >= 0 && V < ((int64_t)1 << 31), "V must be in [0, 2^31)");
    if (V == 0) return GS_OK;
    GS_CHECK_ARG(phi && vertices && normals, "null pointer");
    GiRes G{{R0, R1, R2}};
    hipLaunchKernelGGL(ps_normals_kernel, dim3(ps_grid(V)), dim3(PS_BLOCK), 0, (hipStream_t)stream, (long long)V, G, phi, vertices, normals);
    GS_CHECK_LAUNCH();
    return GS_OK;
}

}  // extern "C"
