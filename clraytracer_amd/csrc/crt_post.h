// crt_post.h -- the per-pixel stages behind Trace, written once: PostProcess, the store and load through upstream's RGBA8 render target, the
// packed bytes, and the FXAA filter up to the value it chooses. Compiled into libcrt_hip.so (crt_kernels.h: the Trace kernel's epilogue,
// crt_postprocess_kernel, crt_fxaa_kernel, the pack kernels) and into libcrt_present.so (../present/crt_present.hip), which applies the same
// stages to any image on the device and therefore has to give the frame's bits. Needs crt_vec3.h only; no state, no exported name.
#pragma once
#include <math.h>
#include <stdint.h>
#include "crt_vec3.h"

// PostProcess (kernel_main.cl:342-359, MathAndSTL.cl:132-169): Saturation 1.2 -> Reinhard (white 0.8) + gamma 1.55 -> gamma 1.2
// -> Vignette; uv = p / resolution.
__device__ __forceinline__ v3 post_pixel(v3 rgb, int px, int py, int width, int height)
{
    const float uvx = (float)px / (float)width, uvy = (float)py / (float)height;
    const float P = sqrtf((rgb.x * rgb.x) * 0.299f + ((rgb.y * rgb.y) * 0.587f) + ((rgb.z * rgb.z) * 0.114f));
    const v3 Pv = mk3(P, P, P);
    rgb = add3(Pv, scale3(sub3(rgb, Pv), 1.2f));
    const v3 lw = mk3(0.2126f, 0.7152f, 0.0722f);
    const float max_white_l = 0.8f;
    const float l_old = dot3(rgb, lw);
    const float numerator = l_old * (1.0f + (l_old / (max_white_l * max_white_l)));
    const float l_new = numerator / (1.0f + l_old);
    const float l_in = dot3(rgb, lw);
    rgb = scale3(rgb, l_new / l_in);
    const float ig = 1.0f / 1.55f;
    rgb = mk3(powf(rgb.x, ig), powf(rgb.y, ig), powf(rgb.z, ig));
    const float oneDivGamma = 1.0f / 1.2f;
    rgb = mk3(powf(rgb.x, oneDivGamma), powf(rgb.y, oneDivGamma), powf(rgb.z, oneDivGamma));
    const float vx = uvx * (1.0f - uvy), vy = uvy * (1.0f - uvx);
    float vig = (vx * vy) * 15.0f;
    vig = powf(vig, 0.15f);
    return scale3(rgb, vig);
}
// Hazard H8: the store + load through upstream's RGBA8-UNORM render target (write_imagef / read_imagef):
// convert_uchar_sat_rte(x * 255) / 255 per channel (CRT_RENDER_UNORM8), and the byte itself.
__device__ __forceinline__ uint32_t unorm8(float x)
{
    const float v = x * 255.0f;
    if (!(v == v) || v <= 0.0f) return 0u;
    if (v >= 255.0f) return 255u;
    return (uint32_t)rintf(v);
}
__device__ __forceinline__ float quantize1(float x) { return (float)unorm8(x) / 255.0f; }
__device__ __forceinline__ v3 quantize3(v3 c) { return mk3(quantize1(c.x), quantize1(c.y), quantize1(c.z)); }
// the bytes of upstream's RGBA8 texture: an opaque pixel, or all four channels of a stored one
__device__ __forceinline__ uint32_t pack_rgba8(float4 p) { return unorm8(p.x) | (unorm8(p.y) << 8) | (unorm8(p.z) << 16) | (unorm8(p.w) << 24); }
__device__ __forceinline__ uint32_t pack_rgba8(v3 c) { return unorm8(c.x) | (unorm8(c.y) << 8) | (unorm8(c.z) << 16) | 0xFF000000u; }

// FXAA (kernel_main.cl:289-340) -- EXTENSION (CRT_RENDER_FXAA): upstream's function is dead code (call commented out at
// kernel_main.cl:349, no return, in-place neighbour reads); the semantics are the oracle's (orc_fxaa): result = the rgb it
// assigns last, neighbours from the unmodified frame `src`, reads clamped to the edge, uv = p / resolution, linear taps as
// OpenCL 1.2 8.2 defines CLK_FILTER_LINEAR. Same operations in the same order as the oracle: bit-identical.
// `src` is the image, a type of the caller's: fxaa_fetch(src, width, i, j) is the rgb of texel (i, j), 0 <= i < width, 0 <= j < height. The frame
// reads a float4 image (the overload below); libcrt_present.so declares overloads for whatever it staged.
__device__ __forceinline__ v3 fxaa_fetch(const float4* __restrict__ img, int width, int i, int j)
{
    const float4 p = img[(size_t)j * (size_t)width + (size_t)i];
    return mk3(p.x, p.y, p.z);
}
template <class Texels> __device__ __forceinline__ v3 fxaa_texel(Texels src, int width, int height, int i, int j)
{
    i = i < 0 ? 0 : (i > width - 1 ? width - 1 : i);
    j = j < 0 ? 0 : (j > height - 1 ? height - 1 : j);
    return fxaa_fetch(src, width, i, j);
}
template <class Texels> __device__ __forceinline__ v3 fxaa_linear(Texels src, int width, int height, float s, float t)
{
    const float u = s * (float)width - 0.5f, v = t * (float)height - 0.5f;
    const float fu = floorf(u), fv = floorf(v);
    const float a = u - fu, b = v - fv;
    const int i0 = (int)fu, j0 = (int)fv;
    const v3 t00 = fxaa_texel(src, width, height, i0, j0), t10 = fxaa_texel(src, width, height, i0 + 1, j0);
    const v3 t01 = fxaa_texel(src, width, height, i0, j0 + 1), t11 = fxaa_texel(src, width, height, i0 + 1, j0 + 1);
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    return add3(add3(add3(scale3(t00, w00), scale3(t10, w10)), scale3(t01, w01)), scale3(t11, w11));
}
// the filter at pixel (px, py) of the W x H image `src`, up to the value it chooses; the stages behind it are the caller's
template <class Texels> __device__ __forceinline__ v3 fxaa_pixel(Texels src, int W, int H, int px, int py)
{
    const float resx = (float)W, resy = (float)H;
    const float uvx = (float)px / resx, uvy = (float)py / resy;
    const v3 luma = mk3(0.299f, 0.587f, 0.114f);
    const v3 rgb = fxaa_texel(src, W, H, px, py);
    const float lumaNW = dot3(fxaa_texel(src, W, H, px - 1, py - 1), luma);
    const float lumaNE = dot3(fxaa_texel(src, W, H, px + 1, py - 1), luma);
    const float lumaSW = dot3(fxaa_texel(src, W, H, px - 1, py + 1), luma);
    const float lumaSE = dot3(fxaa_texel(src, W, H, px + 1, py + 1), luma);
    const float lumaM = dot3(rgb, luma);
    float dirx = -((lumaNW + lumaNE) - (lumaSW + lumaSE));
    float diry = ((lumaNW + lumaSW) - (lumaNE + lumaSE));
    const float lumaSum = ((lumaNW + lumaNE) + lumaSW) + lumaSE;
    const float dirReduce = fmaxf(lumaSum * (0.25f * (1.0f / 8.0f)), 1.0f / 128.0f);
    const float rcpDirMin = 1.0f / (fminf(fabsf(dirx), fabsf(diry)) + dirReduce);
    dirx = fminf(8.0f, fmaxf(-8.0f, dirx * rcpDirMin)) / resx;
    diry = fminf(8.0f, fmaxf(-8.0f, diry * rcpDirMin)) / resy;
    const v3 a0 = fxaa_linear(src, W, H, uvx + dirx * -0.166667f, uvy + diry * -0.166667f);
    const v3 a1 = fxaa_linear(src, W, H, uvx + dirx * 0.166667f, uvy + diry * 0.166667f);
    const v3 rgbA = scale3(add3(a0, a1), 0.5f);
    const v3 b0 = fxaa_linear(src, W, H, uvx + dirx * -0.5f, uvy + diry * -0.5f);
    const v3 b1 = fxaa_linear(src, W, H, uvx + dirx * 0.5f, uvy + diry * 0.5f);
    const v3 rgbB = add3(scale3(rgbA, 0.5f), scale3(add3(b0, b1), 0.25f));
    const float lumaB = dot3(rgbB, luma);
    const float lumaMin = fminf(lumaM, fminf(fminf(lumaNW, lumaNE), fminf(lumaSW, lumaSE)));
    const float lumaMax = fmaxf(lumaM, fmaxf(fmaxf(lumaNW, lumaNE), fmaxf(lumaSW, lumaSE)));
    return ((lumaB < lumaMin) || (lumaB > lumaMax)) ? rgbA : rgbB;
}
