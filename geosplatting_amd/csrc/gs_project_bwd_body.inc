// gs_project_bwd_body.inc -- the statements of A7 for one input Gaussian, included INSIDE the body of every projection-backward kernel
// of gs_project.hip (textual for the same reason as gs_project_fwd_body.inc).  In scope: the kernel's parameters and
//   SH       -- the record's colour gradient (3 channels) goes through the SH evaluation of the forward into the whole coefficient
//               row g_sh_coeffs [N, sh_K, 3] and, for the direction, into v_means (v_colors is unused);
//   CLASSIC  -- the packed opacity was opacities[n] itself: v_opacity passes unscaled and the compensation has no gradient
//               (project_bwd_one with comp = 1 and opacity = 0 computes exactly that: g.op = v_op * 1, v_comp = 0).
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int V = (int)gs_count(vc);
    const int v = find_slot(gaussian_ids, V, N, n);
    float g_mean[3] = { 0, 0, 0 }, g_quat[4] = { 0, 0, 0, 0 }, g_scale[3] = { 0, 0, 0 }, g_op = 0.0f;
    if (v >= 0) {
        const GsCam cam = load_cam(viewmat, K);
        const float mean[3] = { means[3 * (size_t)n], means[3 * (size_t)n + 1], means[3 * (size_t)n + 2] };
        const float4 q4 = *reinterpret_cast<const float4*>(quats + 4 * (size_t)n);
        const float scale[3] = { scales[3 * (size_t)n], scales[3 * (size_t)n + 1], scales[3 * (size_t)n + 2] };
        const float* __restrict__ rec = v_packed + (size_t)v * rec_stride;   // {xy(2), conic(3), opacity, colors(D)}
        ProjGrad pg;
        project_bwd_one(cam, mean, q4, scale, CLASSIC ? 0.0f : opacities[n], (float)W, (float)H, eps2d, conics[3 * (size_t)v],
                        conics[3 * (size_t)v + 1], conics[3 * (size_t)v + 2], CLASSIC ? 1.0f : compensations[v], rec[0], rec[1], rec[2],
                        rec[3], rec[4], rec[5], v_depths ? v_depths[v] : 0.0f, pg);
#pragma unroll
        for (int k = 0; k < 3; ++k) { g_mean[k] = pg.mean[k]; g_scale[k] = pg.scale[k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) g_quat[k] = pg.quat[k];
        g_op = pg.op;
        if constexpr (SH) {
            const float v_rgb[3] = { rec[6], rec[7], rec[8] };
            sh_color_bwd(cam, mean, sh_coeffs + (size_t)n * sh_K * 3, sh_K, sh_degree, true, v_rgb,
                         g_sh_coeffs + (size_t)n * sh_K * 3, g_mean);
        }
    } else if constexpr (SH) {
        const GsCam cam = load_cam(viewmat, K);
        const float v_rgb[3] = { 0.f, 0.f, 0.f };
        sh_color_bwd(cam, nullptr, sh_coeffs + (size_t)n * sh_K * 3, sh_K, sh_degree, false, v_rgb, g_sh_coeffs + (size_t)n * sh_K * 3,
                     g_mean);
    }
    if (accumulate) {          // += into persistent gradient buffers (several views per step); culled Gaussians add nothing
        if (v >= 0) {
            v_means[3 * (size_t)n] += g_mean[0]; v_means[3 * (size_t)n + 1] += g_mean[1]; v_means[3 * (size_t)n + 2] += g_mean[2];
            float4 q = *reinterpret_cast<float4*>(v_quats + 4 * (size_t)n);
            q.x += g_quat[0]; q.y += g_quat[1]; q.z += g_quat[2]; q.w += g_quat[3];
            *reinterpret_cast<float4*>(v_quats + 4 * (size_t)n) = q;
            v_scales[3 * (size_t)n] += g_scale[0]; v_scales[3 * (size_t)n + 1] += g_scale[1]; v_scales[3 * (size_t)n + 2] += g_scale[2];
            v_opacities[n] += g_op;
        }
    } else {
        v_means[3 * (size_t)n] = g_mean[0]; v_means[3 * (size_t)n + 1] = g_mean[1]; v_means[3 * (size_t)n + 2] = g_mean[2];
        *reinterpret_cast<float4*>(v_quats + 4 * (size_t)n) = make_float4(g_quat[0], g_quat[1], g_quat[2], g_quat[3]);
        v_scales[3 * (size_t)n] = g_scale[0]; v_scales[3 * (size_t)n + 1] = g_scale[1]; v_scales[3 * (size_t)n + 2] = g_scale[2];
        v_opacities[n] = g_op;
    }
    if constexpr (!SH) {
        if (v_colors) {         // per-view quantity (feeds the shading backward): always a plain write
            for (int k = 0; k < D; ++k) v_colors[(size_t)n * D + k] = (v >= 0) ? v_packed[(size_t)v * rec_stride + 6 + k] : 0.0f;
        }
    }
