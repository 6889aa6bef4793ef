// gs_project_fwd_body.inc -- the statements of A1 + A1' (one workgroup = one chunk of the chained scan), included INSIDE the body of
// every projection-forward kernel of gs_project.hip; it is textual so that project_fwd_kernel compiles to exactly the ISA it had
// before the variants existed (an inlined template body reorders its instructions).  In scope: the kernel's parameters and
//   SH       -- the colour of a visible Gaussian is evaluated from its spherical-harmonics coefficients (sh_coeffs [N, sh_K, 3],
//               degree sh_degree; colors / D are then unused and 3 channels are written, see sh_color);
//   CLASSIC  -- gsplat's rasterize_mode='classic': the opacity is not multiplied by the anti-alias compensation.
    __shared__ int s_chunk;
    __shared__ int s_wv[GS_PROJ_WAVES];
    __shared__ int s_wi[GS_PROJ_WAVES];
    __shared__ long long s_base[2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_chunk = (int)atomicAdd(ctrl, 1u);
    __syncthreads();
    const int chunk = s_chunk;
    const int n = chunk * GS_PROJ_BLOCK + tid;

    u64* agg_v = desc;
    u64* agg_i = desc + n_chunks;
    u64* pre_v = desc + 2 * (size_t)n_chunks;
    u64* pre_i = desc + 3 * (size_t)n_chunks;

    GsCam cam = load_cam(viewmat, K);
    ProjFwd p;
    p.valid = false; p.radius = 0;
    int ntiles = 0;
    int tx0 = 0, ty0 = 0, tx1 = 0, ty1 = 0;
    if (n < N) {
        float mean[3] = { means[3 * (size_t)n], means[3 * (size_t)n + 1], means[3 * (size_t)n + 2] };
        float4 q = *reinterpret_cast<const float4*>(quats + 4 * (size_t)n);
        float quat[4] = { q.x, q.y, q.z, q.w };
        float scale[3] = { scales[3 * (size_t)n], scales[3 * (size_t)n + 1], scales[3 * (size_t)n + 2] };
        p = project_exact(cam, mean, quat, scale, (float)W, (float)H, eps2d, near_plane, far_plane, radius_clip);
        if (p.valid) {
            tile_range_exact(p.m2x, p.m2y, p.radius, tile_size, tile_w, tile_h, tx0, ty0, tx1, ty1);
            ntiles = (tx1 - tx0) * (ty1 - ty0);
        }
    }

    // ---- block-level scan of (valid, ntiles)
    const u64 bal = __ballot(p.valid);
    const int v_excl_wave = __popcll(bal & ((1ull << lane) - 1ull));
    int i_incl = ntiles;
    i_incl = gs_wave_incl_scan(i_incl);
    if (lane == 63) { s_wv[wave] = __popcll(bal); s_wi[wave] = i_incl; }
    __syncthreads();
    int v_before = 0, i_before = 0, aggV = 0, aggI = 0;
#pragma unroll
    for (int w = 0; w < GS_PROJ_WAVES; ++w) {
        if (w < wave) { v_before += s_wv[w]; i_before += s_wi[w]; }
        aggV += s_wv[w]; aggI += s_wi[w];
    }

    // ---- decoupled look-back across chunks (wave 0)
    if (wave == 0) {
        long long baseV = 0, baseI = 0;
        if (chunk > 0) {
            if (lane == 0) { desc_store(&agg_v[chunk], (u64)aggV); desc_store(&agg_i[chunk], (u64)aggI); }
            int pos = chunk - 1;
            for (;;) {
                const int idx = pos - lane;
                bool isP = idx < 0;           // virtual predecessors before chunk 0: prefix 0
                bool isA = false;
                u64 pv = 0, pi = 0, av = 0, ai = 0;
                if (idx >= 0) {
                    int spins = 0;
                    for (;;) {
                        pv = desc_load(&pre_v[idx]); pi = desc_load(&pre_i[idx]);
                        isP = (pv & pi & GS_VALID_BIT) != 0;
                        if (isP) break;
                        av = desc_load(&agg_v[idx]); ai = desc_load(&agg_i[idx]);
                        isA = (av & ai & GS_VALID_BIT) != 0;
                        if (isA) break;
                        if (++spins > GS_SPIN_LIMIT) { atomicExch(ctrl + 1, 1u); isA = true; av = ai = 0; break; }
                        __builtin_amdgcn_s_sleep(2);
                    }
                }
                const u64 pmask = __ballot(isP);
                const int first = pmask ? __builtin_ctzll(pmask) : 64;
                long long cv = 0, ci = 0;
                if (lane <= first) {
                    cv = (long long)((isP ? pv : av) & ~GS_VALID_BIT);
                    ci = (long long)((isP ? pi : ai) & ~GS_VALID_BIT);
                }
                baseV += wave_sum_i64(cv);
                baseI += wave_sum_i64(ci);
                if (pmask) break;
                pos -= 64;
            }
        }
        if (lane == 0) {
            desc_store(&pre_i[chunk], (u64)(baseI + aggI));
            desc_store(&pre_v[chunk], (u64)(baseV + aggV));
            s_base[0] = baseV; s_base[1] = baseI;
            if (chunk == n_chunks - 1) { counts[0] = baseV + aggV; counts[1] = baseI + aggI; }
        }
    }
    __syncthreads();
    const long long baseV = s_base[0], baseI = s_base[1];

    if (n < N) {
        const long long slot = baseV + v_before + v_excl_wave;
        if (packed_index) packed_index[n] = p.valid ? (int32_t)slot : -1;
        if (p.valid) {
            gaussian_ids[slot] = n;
            radii[slot] = p.radius;
            *reinterpret_cast<float2*>(means2d + 2 * slot) = make_float2(p.m2x, p.m2y);
            depths[slot] = p.depth;
            conics[3 * slot] = p.ca; conics[3 * slot + 1] = p.cb; conics[3 * slot + 2] = p.cc;
            compensations[slot] = p.comp;
            opacities_packed[slot] = CLASSIC ? opacities[n] : opacities[n] * p.comp;
            tiles_per_gauss[slot] = ntiles;
            cum_tiles[slot] = baseI + i_before + i_incl;
            if constexpr (SH) {                              // 3 channels evaluated here: colors_packed [N,3], and the record
                const float mean[3] = { means[3 * (size_t)n], means[3 * (size_t)n + 1], means[3 * (size_t)n + 2] };
                float rgb[3];
                sh_color(cam, mean, sh_coeffs + (size_t)n * sh_K * 3, sh_K, sh_degree, rgb);
                colors_packed[3 * slot] = rgb[0]; colors_packed[3 * slot + 1] = rgb[1]; colors_packed[3 * slot + 2] = rgb[2];
                if (vis) gs_write_vis_record(vis + 4 * slot, p.m2x, p.m2y, p.ca, p.cb, p.cc, CLASSIC ? opacities[n] : opacities[n] * p.comp,
                                             rgb[0], rgb[1], rgb[2]);
            } else {
                if (colors_packed) {
                    for (int k = 0; k < D; ++k) colors_packed[slot * D + k] = colors[(size_t)n * D + k];
                }
                if (vis) {                                   // the compositor's per-visible record, straight from the registers
                    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
                    if (colors && D <= 3) {
                        c0 = colors[(size_t)n * D];
                        if (D > 1) c1 = colors[(size_t)n * D + 1];
                        if (D > 2) c2 = colors[(size_t)n * D + 2];
                    }
                    gs_write_vis_record(vis + 4 * slot, p.m2x, p.m2y, p.ca, p.cb, p.cc, CLASSIC ? opacities[n] : opacities[n] * p.comp,
                                        c0, c1, c2);
                }
            }
        }
    }
