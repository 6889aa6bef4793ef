// gs_tone.h -- S4 tone mapping, per channel (rfstudio/model/geosplat.py:474-480: _tone_mapping_naive / _tone_mapping_aces; 'none' is the
// identity).  Shared by the stand-alone tone-map kernels (gs_shade.hip) and by the compositor kernels that apply it in their
// epilogue / prologue (gs_raster.hip: gs_raster_composite_tone*, gs_raster_bwd_tone*).  Contraction is OFF inside the functions so that
// every includer computes the same bits whatever its file-level setting is.
#pragma once
#include "gs_common.h"

__device__ __forceinline__ float tone_fwd(int mode, float rgb)
{
#pragma clang fp contract(off)
    if (mode == GS_TONE_NAIVE) {
        const float x = 1.0f - rgb, bx = 100.0f * x;
        const float sp = bx > 20.0f ? x : log1pf(expf(bx)) / 100.0f;
        return 1.0f - sp;
    }
    if (mode == GS_TONE_ACES) return (rgb * (2.51f * rgb + 0.03f)) / (rgb * (2.43f * rgb + 0.59f) + 0.14f);
    return rgb;
}
__device__ __forceinline__ float tone_grad(int mode, float rgb)
{
#pragma clang fp contract(off)
    if (mode == GS_TONE_NAIVE) {
        const float bx = 100.0f * (1.0f - rgb);
        return bx > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-bx));
    }
    if (mode == GS_TONE_ACES) {
        const float num = rgb * (2.51f * rgb + 0.03f), den = rgb * (2.43f * rgb + 0.59f) + 0.14f;
        return ((5.02f * rgb + 0.03f) * den - num * (4.86f * rgb + 0.59f)) / (den * den);
    }
    return 1.0f;
}

// rgb2srgb of PBRImages (rfstudio/graphics/_images.py:165-182): the same piecewise curve the photometric loss applies for its sRGB
// metric (gs_loss.hip: linear_to_srgb), here for the environment background (gs_envmap.hip).
__device__ __forceinline__ float tone_rgb2srgb(float c)
{
#pragma clang fp contract(off)
    return c <= 0.0031308f ? c * 12.92f : powf(fmaxf(c, 0.0031308f), 1.0f / 2.4f) * 1.055f - 0.055f;
}
