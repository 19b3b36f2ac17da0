// JPEG Lossless (SOF3, predictor 1) on the device: the kernels behind tf_jpegll_decode and tf_hold_frames_jpegll.  The decoder is
// teeflow_jpegll_core.h, the same text the host test runs under the sanitizers, on top of teeflow_jpeg_core.h; the host has parsed every
// frame's header into a tfj::Desc (read as the core says: an MCU is one sample of every component), so every grid is known before the
// first launch and nothing between the kernels waits for the host.
//   k_jpeg_marks      teeflow_jpeg.hip.h's, unchanged: the RSTn positions and the end of the entropy data, one wave64 per frame
//   k_jpegll_entropy  one wave64 per (frame, restart interval): Huffman decode into 16-bit differences, planar [component][H * W]
//   k_jpegll_col      one wave64 per (frame, component, restart interval): the running sum of column 0 over the interval's rows from
//                     128, in place -- the first entry of every row becomes the row's first sample
//   k_jpegll_rows     one wave64 per (frame, component, row): the running sum along the row, 64 samples a round by a __shfl_up scan
//                     with a carry between rounds, masked to 16 bits, range-checked, written as uint8
// The entropy wave is serial and wave-uniform, as k_jpeg_entropy is: the stream is read through the LDS stage of
// teeflow_wave_stage.hip.h and every table entry is made a scalar with readfirstlane; 64 differences of every component are gathered in
// LDS and leave as one coalesced store.  The reconstruction has no serial dependence between rows: with Px = Ra a row is a prefix sum
// of its own differences once its first sample is known, and the first samples are a prefix sum down column 0.
//
// Per-frame scratch (the host sizes it, teeflow_jpegll_host.hip.h): samples * H * W differences of 2 bytes and H RSTn positions (an
// interval is at least a row, so a frame has at most H of them); the samples, 1 byte each, go straight into the call's output.
//
// Safety (a malformed stream is an expected input): a frame whose status is set is touched by no kernel after the one that set it.  The
// stream is read only through the staged reader, whose safety argument is teeflow_wave_stage.hip.h's, at positions below the frame's
// length.  k_jpeg_marks writes position k only with k < nint - 1 < H.  k_jpegll_entropy writes difference s of component c only for
// sample s of its own interval, s < H * W, c < ncomp = samples (the host's parse_header refuses any other count); k_jpegll_col and
// k_jpegll_rows index by the descriptor, the grid and H, W alone, never by stream data: a difference is a value that is added, not a
// place.  Loop bounds: the entropy loop is the interval's samples, each symbol moves the reader on or fails (teeflow_jpeg_core.h).
//
// The build's assembly for gfx950: k_jpegll_entropy 61 VGPRs and 5024 bytes of LDS, k_jpegll_col 13 VGPRs, k_jpegll_rows 18; private
// segment 0 bytes and no scratch instruction in any of the three.
#pragma once
#include "teeflow_jpeg.hip.h"
#include "teeflow_jpegll_core.h"

namespace jpegll {
// the inclusive scan of x over the wave's lanes, modulo 2^32 (the callers mask to 16 bits)
__device__ inline uint32_t wave_scan(uint32_t x, int ln)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (ln >= o) x += y;
    }
    return x;
}
}  // namespace jpegll

// Block (k, fb): restart interval k of frame f0 + fb; a frame without DRI is one interval.  diff + fb * diff_stride gets the frame's
// differences modulo 2^16, component c's H * W at c * hw.  The first error sets status 3 and ends the wave; a wave of a frame whose
// status is already set returns at once.
__global__ __launch_bounds__(64) void k_jpegll_entropy(const uint8_t* __restrict__ blob, const unsigned long long* __restrict__ off,
                                                      const uint32_t* __restrict__ len, const tfj::Desc* __restrict__ desc, int f0, uint32_t ni_max,
                                                      const uint32_t* __restrict__ rst, const uint32_t* __restrict__ scan_end,
                                                      uint16_t* __restrict__ diff, size_t diff_stride, size_t hw, int* status)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[jpeg::STAGE];
    __shared__ tfj::Huff huff[4];
    __shared__ uint16_t blk[3][64];
    const int fb = (int)blockIdx.y, f = f0 + fb, ln = (int)threadIdx.x;
    const uint32_t k = blockIdx.x;
    const tfj::Desc& d = desc[f];
    if (jpeg::status_of(status, f) != 0 || k >= d.nint) return;
    if (ln < 4) tfj::huff_lengths(d.bits[ln], huff[ln]);
    for (int i = ln; i < 4 * 256; i += 64) huff[i >> 8].vals[i & 255] = d.vals[i >> 8][i & 255];
    __syncthreads();
    for (int i = ln; i < 4 * 256; i += 64) huff[i >> 8].look[i & 255] = tfj::huff_look(huff[i >> 8], i & 255);
    __syncthreads();
    jpeg::WaveIO io;
    jpeg::open_frame(io, stage, blob, off[f], len[f], ln);
    const uint32_t* list = rst + (size_t)f * ni_max;
    tfj::Bits b;
    b.acc = 0; b.cnt = 0; b.pad = 0;
    b.pos = k ? list[k - 1] + 2 : d.scan_off;
    b.end = k + 1 < d.nint ? list[k] : scan_end[f];
    const uint32_t s0 = d.ri ? k * d.ri : 0, s1 = d.ri && s0 + d.ri < d.nmcu ? s0 + d.ri : d.nmcu;
    const int nc = d.ncomp < 3 ? d.ncomp : 3;
    const tfj::Huff* const t0 = &huff[d.td[0] & 3];
    const tfj::Huff* const t1 = &huff[d.td[1] & 3];
    const tfj::Huff* const t2 = &huff[d.td[2] & 3];
    uint16_t* out = diff + (size_t)fb * diff_stride;
    int rc = tfj::OK;
    for (uint32_t base = s0; base < s1; base += 64) {
        const uint32_t n = s1 - base < 64 ? s1 - base : 64;
        for (uint32_t j = 0; j < n && rc == tfj::OK; ++j)
            for (int c = 0; c < nc; ++c) {
                const int v = tfl::decode_diff(io, b, c == 0 ? *t0 : (c == 1 ? *t1 : *t2));
                if (v < 0) { rc = tfj::BAD_DATA; break; }
                blk[c][j] = (uint16_t)v;
            }
        if (rc != tfj::OK) break;
        __syncthreads();
        if ((uint32_t)ln < n)
            for (int c = 0; c < nc; ++c) out[(size_t)c * hw + base + ln] = blk[c][ln];
        __syncthreads();
    }
    if (rc != tfj::OK && ln == 0) atomicMax(&status[f], rc);
}

// Block (k, c, fb): column 0 of component c over the rows of restart interval k of frame f0 + fb, 64 rows a round.
__global__ __launch_bounds__(64) void k_jpegll_col(const tfj::Desc* __restrict__ desc, int f0, uint16_t* __restrict__ diff, size_t diff_stride, size_t hw,
                                                  const int* status)
{
    const int fb = (int)blockIdx.z, f = f0 + fb, c = (int)blockIdx.y, ln = (int)threadIdx.x;
    const uint32_t k = blockIdx.x;
    const tfj::Desc& d = desc[f];
    if (jpeg::status_of(status, f) != 0 || k >= d.nint || c >= d.ncomp) return;
    uint32_t r0, r1;
    tfl::interval_rows(d, k, &r0, &r1);
    const size_t W = d.mcux;
    uint16_t* col = diff + (size_t)fb * diff_stride + (size_t)c * hw;
    uint32_t carry = 128;
    for (uint32_t base = r0; base < r1; base += 64) {
        const uint32_t r = base + (uint32_t)ln;
        const uint32_t x = carry + jpegll::wave_scan(r < r1 ? col[(size_t)r * W] : 0u, ln);
        if (r < r1) col[(size_t)r * W] = (uint16_t)x;
        carry = (uint32_t)__shfl((int)x, 63, 64) & 0xFFFFu;
    }
}

// Block (y, c, fb): row y of component c of frame f0 + fb.  out is the call's whole output, frame f0 + fb at its own place:
// interleaved [N][H][W][samples], or (planar) [N][samples][H * W], k_ingest_planar's layout.  A sample outside 0..255 sets status 3.
__global__ __launch_bounds__(64) void k_jpegll_rows(int f0, const uint16_t* __restrict__ diff, size_t diff_stride, int samples, int H, int W, int planar,
                                                   uint8_t* __restrict__ out, int* status)
{
    const int fb = (int)blockIdx.z, f = f0 + fb, c = (int)blockIdx.y, y = (int)blockIdx.x, ln = (int)threadIdx.x;
    if (y >= H || c >= samples || jpeg::status_of(status, f) != 0) return;
    const size_t hw = (size_t)H * W, row = (size_t)y * W;
    const uint16_t* in = diff + (size_t)fb * diff_stride + (size_t)c * hw + row;
    uint32_t carry = 0;
    bool bad = false;
    for (int base = 0; base < W; base += 64) {
        const int i = base + ln;
        const uint32_t x = (carry + jpegll::wave_scan(i < W ? in[i] : 0u, ln)) & 0xFFFFu;
        if (i < W) {
            bad |= x > 255;
            if (planar) out[((size_t)f * samples + c) * hw + row + i] = (uint8_t)x;
            else out[((size_t)f * hw + row + i) * samples + c] = (uint8_t)x;
        }
        carry = (uint32_t)__shfl((int)x, 63, 64);
    }
    if (bad) atomicMax(&status[f], (int)tfj::BAD_DATA);
}
