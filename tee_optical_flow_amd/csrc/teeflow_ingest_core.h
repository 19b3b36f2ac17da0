// Frame ingest: a study's pixel data in the form its file stores -- RGB, one grey byte, or YBR_FULL -- to the uint8 RGB [N][H][W][3] that
// every frames-taking call reads, with the columns mirrored on request.  The pixel function and a lane's run of 4 pixels, in plain C++
// that compiles for the device (teeflow_ingest.hip.h: TFG_FN = __device__, TFG_FMA = __fmaf_rn) and for the host
// (tests/csrc/verify_ingest.cpp, under the address and undefined-behaviour sanitizers, with buffers of the exact size).
//
// What it replaces is the reference's host-side frame preparation (calculate_optical_flow.py:524-548): pydicom's
// convert_color_space(arr, 'YBR_FULL', 'RGB'), skimage's gray2rgb and np.flip(axis=2).  The YBR conversion is DICOM PS3.3 C.7.6.3.1.2's
// inverse, in float32, in ONE fixed order (frames.ybr_full_to_rgb is the numpy twin):
//     (y, cb, cr) = (Y, Cb - 128, Cr - 128);   t = y * m0;  t = fma(cb, m1, t);  t = fma(cr, m2, t);   out = clamp(floor(t + 0.5f), 0, 255)
// with m the float32 roundings of [[1, 1, 1], [0, -0.114 * 1.772 / 0.587, 1.772], [1.402, -0.299 * 1.402 / 0.587, 0]] (row = input,
// column = output channel).  Over all 2^24 triples this order equals np.matmul in float32 on an FMA host; multiply-add-add without
// fusion differs at 42 triples and a float64 evaluation at 8252, each by one count.
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifndef TFG_FN
#include <math.h>
#define TFG_FN inline
#define TFG_FMA(a, b, c) fmaf((a), (b), (c))
#endif

namespace tfg {
// the source forms (TF_FRAMES_* of include/teeflow.h)
enum : int { RGB = 0, GRAY = 1, YBR_FULL = 2 };
// An internal form, no TF_FRAMES_* value and refused by tf_hold_frames and tf_hold_frames_rle: Y, Cb, Cr as a JPEG stream holds them ->
// RGB with libjpeg's fixed-point tables (jdcolor.c, SCALEBITS 16), what a libjpeg-backed reader returns for such a stream.  With
// cb = Cb - 128, cr = Cr - 128, signed 32-bit and an arithmetic shift:
//     R = Y + ((91881 * cr + 32768) >> 16);   G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);   B = Y + ((116130 * cb + 32768) >> 16)
// each clamped to [0, 255] (tf_hold_frames_jpeg with TF_JPEG_COLOR_LIBJPEG; frames.ycc_to_rgb_libjpeg is the numpy twin).
enum : int { YBR_LIBJPEG = 3 };

// bytes per source pixel
TFG_FN int src_channels(int form) { return form == GRAY ? 1 : 3; }

TFG_FN uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
TFG_FN void ybr_libjpeg_pixel(uint8_t Y, uint8_t Cb, uint8_t Cr, uint8_t* rgb)
{
    const int y = Y, cb = (int)Cb - 128, cr = (int)Cr - 128;
    rgb[0] = clamp255(y + ((91881 * cr + 32768) >> 16));
    rgb[1] = clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    rgb[2] = clamp255(y + ((116130 * cb + 32768) >> 16));
}

constexpr float M_CB_G = (float)(-0.114 * 1.772 / 0.587), M_CB_B = (float)1.772;
constexpr float M_CR_R = (float)1.402, M_CR_G = (float)(-0.299 * 1.402 / 0.587);

TFG_FN uint8_t ybr_round(float t)
{
    const float r = __builtin_floorf(t + 0.5f);
    return (uint8_t)(int)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

// one YBR_FULL pixel -> RGB (every product by a 1 or 0 coefficient is kept: the chain is the same for the three channels)
TFG_FN void ybr_pixel(uint8_t Y, uint8_t Cb, uint8_t Cr, uint8_t* rgb)
{
    const float y = (float)Y, cb = (float)Cb - 128.f, cr = (float)Cr - 128.f;
    rgb[0] = ybr_round(TFG_FMA(cr, M_CR_R, TFG_FMA(cb, 0.f, y * 1.f)));
    rgb[1] = ybr_round(TFG_FMA(cr, M_CR_G, TFG_FMA(cb, M_CB_G, y * 1.f)));
    rgb[2] = ybr_round(TFG_FMA(cr, 0.f, TFG_FMA(cb, M_CB_B, y * 1.f)));
}

// source pixel s of form FORM -> its three output bytes
template <int FORM>
TFG_FN void pixel(const uint8_t* src, size_t s, uint8_t* rgb)
{
    if (FORM == GRAY) rgb[0] = rgb[1] = rgb[2] = src[s];
    else if (FORM == YBR_FULL) ybr_pixel(src[3 * s], src[3 * s + 1], src[3 * s + 2], rgb);
    else if (FORM == YBR_LIBJPEG) ybr_libjpeg_pixel(src[3 * s], src[3 * s + 1], src[3 * s + 2], rgb);
    else { rgb[0] = src[3 * s]; rgb[1] = src[3 * s + 1]; rgb[2] = src[3 * s + 2]; }
}

TFG_FN uint32_t load32(const uint8_t* p)       // p is dword-aligned
{
    uint32_t w;
    __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
    return w;
}
TFG_FN void store32(uint8_t* p, uint32_t w) { __builtin_memcpy(__builtin_assume_aligned(p, 4), &w, 4); }

// Lane `lane` of the ingest: output pixels [4 * lane, 4 * lane + 4) of the npx = N * H * W pixels seen as one flat array, i.e. the 12
// output bytes at the dword-aligned offset 12 * lane whatever W is (k_ov_compose's store shape) -- three dword stores.  Without FLIP
// the source run is as aligned as the output's (4 or 12 bytes at 4 * lane or 12 * lane): dword loads.  With FLIP output pixel (row, x)
// reads source pixel (row, W - 1 - x) of the same row -- rows are frames' rows back to back, so a run may cross a row's or a frame's
// end -- through byte loads.  The last lane's run may be short (npx % 4 pixels): byte loads and byte stores, nothing beyond 3 * npx.
// src and out are dword-aligned (device allocations; malloc'd buffers on the host).
// PLANAR (RGB and YBR_FULL; what the RLE decoder leaves, teeflow_rle.hip.h): the source is [N][3][hw] sample planes, hw = H * W bytes
// each, in place of [N][H][W][3] -- pixel q of frame f has its samples at (3 * f + c) * hw + q.  Where hw is a multiple of 4 a run
// without FLIP lies in one frame and every plane starts dword-aligned: three dword loads; otherwise byte loads.
template <int FORM, bool FLIP, bool PLANAR = false>
TFG_FN void ingest_lane(const uint8_t* src, size_t npx, int W, size_t lane, uint8_t* out, size_t hw = 0)
{
    static_assert(!PLANAR || FORM != GRAY, "one grey plane is the interleaved form already");
    const size_t p0 = lane * 4;
    if (p0 >= npx) return;
    const int n = npx - p0 < 4 ? (int)(npx - p0) : 4;
    uint8_t b[12];
    if (PLANAR) {
        uint8_t s[12];
        const size_t f0 = p0 / hw, q0 = p0 - f0 * hw;
        if (!FLIP && n == 4 && (hw & 3) == 0) {
            for (int c = 0; c < 3; ++c) {
                const uint32_t w = load32(src + (3 * f0 + (size_t)c) * hw + q0);
                for (int j = 0; j < 4; ++j) s[3 * j + c] = (uint8_t)(w >> (8 * j));
            }
        } else {
            size_t row = FLIP ? p0 / (size_t)W : 0;
            int x = FLIP ? (int)(p0 - row * (size_t)W) : 0;
            size_t f = f0, qo = q0;                                              // output pixel p0 + k is pixel qo of frame f
            for (int k = 0; k < n; ++k) {
                // (the mirrored pixel is in the output pixel's row: the same frame)
                const size_t q = FLIP ? row * (size_t)W + (size_t)(W - 1 - x) - f * hw : qo;
                for (int c = 0; c < 3; ++c) s[3 * k + c] = src[(3 * f + (size_t)c) * hw + q];
                if (FLIP && ++x == W) { x = 0; ++row; }
                if (++qo == hw) { qo = 0; ++f; }
            }
        }
        for (int k = 0; k < n; ++k) pixel<FORM>(s, (size_t)k, b + 3 * k);
    } else if (!FLIP && n == 4) {
        if (FORM == GRAY) {
            const uint32_t g = load32(src + p0);
            for (int k = 0; k < 4; ++k) b[3 * k] = b[3 * k + 1] = b[3 * k + 2] = (uint8_t)(g >> (8 * k));
        } else {
            uint8_t s[12];
            for (int d = 0; d < 3; ++d) {
                const uint32_t w = load32(src + 3 * p0 + 4 * d);
                for (int j = 0; j < 4; ++j) s[4 * d + j] = (uint8_t)(w >> (8 * j));
            }
            for (int k = 0; k < 4; ++k) pixel<FORM>(s, (size_t)k, b + 3 * k);
        }
    } else {
        size_t row = FLIP ? p0 / (size_t)W : 0;
        int x = FLIP ? (int)(p0 - row * (size_t)W) : 0;
        for (int k = 0; k < n; ++k) {
            pixel<FORM>(src, FLIP ? row * (size_t)W + (size_t)(W - 1 - x) : p0 + k, b + 3 * k);
            if (FLIP && ++x == W) { x = 0; ++row; }
        }
    }
    uint8_t* o = out + 3 * p0;
    if (n == 4)
        for (int d = 0; d < 3; ++d)
            store32(o + 4 * d, (uint32_t)b[4 * d] | ((uint32_t)b[4 * d + 1] << 8) | ((uint32_t)b[4 * d + 2] << 16) | ((uint32_t)b[4 * d + 3] << 24));
    else
        for (int i = 0; i < 3 * n; ++i) o[i] = b[i];
}
}  // namespace tfg
