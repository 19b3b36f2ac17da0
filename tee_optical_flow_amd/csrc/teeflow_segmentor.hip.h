// teeflow_segmentor.hip.h -- the frame glue around the SAM segmentor on the device (evaluate_1_slice of the reference,
// /root/reference/optical_flow/calculate_optical_flow.py:47-88; host restatement tee_optical_flow_amd/masks.py), exact:
//   k_seg_input     uint8 RGB frame -> PIL's Image.resize(BILINEAR) to out_h x out_w -> ToTensor + Normalize, planar float32 NCHW
//   k_seg_classmap  logits [N][C][h][w] -> argmax over C (torch's on the CPU) -> PIL's Image.resize(NEAREST) to H x W, uint8
// Integer arithmetic and table look-ups only: the tables are PIL's own (pil_resample_tables.h, built on the host in double), the float
// is read from a 3 x 256 table the caller made with the reference's torch expression.  No tolerance anywhere.
//
// k_seg_input is ONE kernel, not PIL's two passes with a uint8 image between them: every output pixel runs its vertical taps over
// horizontally resampled AND ROUNDED bytes, which is what the second pass reads from the intermediate image.  Upscaling (the usual
// case: 512^2 or 600 x 800 to 1024^2) that is 2 x 2 taps per channel; a lane makes four neighbouring x, whose taps mostly coincide
// and come from L1.  The pass is bound by its stores -- 12 bytes out per pixel against 3/4 byte in when 512^2 doubles -- so the
// recomputation costs nothing a second kernel and 3 MB more traffic per frame would not cost more of.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace seg {

constexpr int PREC = 22;                    // PIL's PRECISION_BITS for 8-bit images

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one axis of a bilinear resize: bounds [out][2] = (first source index, taps), coeff [out][ksize]
struct Axis { const int* __restrict__ bounds; const int* __restrict__ coeff; int ksize; };

// grid (ceil(out_h * ceil(out_w / 4) / 256), frames): thread = four consecutive output x of one row, all three planes.
// VEC: out_w % 4 == 0, so a row's quads are 16-byte aligned and each plane gets one float4 store; otherwise element stores, the row's
// last quad cut at out_w.  src: [frames][H][W][3], dst: [frames][3][out_h][out_w], lut: [3][256].
template <bool VEC>
__global__ __launch_bounds__(256) void k_seg_input(const uint8_t* __restrict__ src, int H, int W, int out_h, int out_w, Axis ax, Axis ay,
                                                   const float* __restrict__ lut, float* __restrict__ dst)
{
    __shared__ float slut[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) slut[i] = lut[i];
    __syncthreads();
    const int qpr = (out_w + 3) >> 2;                                   // quads per row
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)out_h * qpr) return;
    const int y = (int)(idx / qpr), x0 = (int)(idx % qpr) * 4;
    const size_t oplane = (size_t)out_h * out_w;
    const uint8_t* frame = src + (size_t)blockIdx.y * H * W * 3;
    float* o = dst + (size_t)blockIdx.y * 3 * oplane + (size_t)y * out_w + x0;
    const int ymin = ay.bounds[2 * y], ny = ay.bounds[2 * y + 1];
    const int* ky = ay.coeff + (size_t)y * ay.ksize;
    float r[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j < out_w ? x0 + j : out_w - 1;             // (a cut quad recomputes the row's last pixel; it is not stored)
        const int xmin = ax.bounds[2 * x], nx = ax.bounds[2 * x + 1];
        const int* kx = ax.coeff + (size_t)x * ax.ksize;
        int v0 = 1 << (PREC - 1), v1 = v0, v2 = v0;
        for (int ty = 0; ty < ny; ++ty) {
            const uint8_t* p = frame + ((size_t)(ymin + ty) * W + xmin) * 3;
            int h0 = 1 << (PREC - 1), h1 = h0, h2 = h0;
            for (int tx = 0; tx < nx; ++tx) {
                const int k = kx[tx];
                h0 += (int)p[3 * tx] * k; h1 += (int)p[3 * tx + 1] * k; h2 += (int)p[3 * tx + 2] * k;
            }
            const int k = ky[ty];                                       // the intermediate image's bytes, times the vertical tap
            v0 += clip8(h0 >> PREC) * k; v1 += clip8(h1 >> PREC) * k; v2 += clip8(h2 >> PREC) * k;
        }
        r[0][j] = slut[clip8(v0 >> PREC)];
        r[1][j] = slut[256 + clip8(v1 >> PREC)];
        r[2][j] = slut[512 + clip8(v2 >> PREC)];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (VEC) {
            *reinterpret_cast<float4*>(o + c * oplane) = make_float4(r[c][0], r[c][1], r[c][2], r[c][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < out_w) o[c * oplane + j] = r[c][j];
        }
    }
}

// grid (ceil(H * W / 256), frames): out[n][y][x] = argmax_c logits[n][c][iy[y]][ix[x]] -- the reference's argmax, uint8 cast and NEAREST
// resize in one gather (the resize only picks pixels, so it commutes with the argmax).  torch.argmax on the CPU: the lowest index of
// equal maxima, a NaN is the maximum and the first NaN stays.  C <= 256, so the index is its own uint8 cast.
__global__ __launch_bounds__(256) void k_seg_classmap(const float* __restrict__ logits, int C, int h, int w, int H, int W,
                                                      const int* __restrict__ iy, const int* __restrict__ ix, uint8_t* __restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)H * W) return;
    const int y = (int)(p / W), x = (int)(p % W);
    const size_t plane = (size_t)h * w;
    const float* l = logits + (size_t)blockIdx.y * C * plane + (size_t)iy[y] * w + ix[x];
    float best = l[0];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
        const float v = l[(size_t)c * plane];
        if (!(best != best) && (v != v || v > best)) { best = v; bi = c; }
    }
    out[(size_t)blockIdx.y * H * W + p] = (uint8_t)bi;
}

}  // namespace seg
