// JPEG Baseline on the device: the four kernels behind tf_jpeg_decode and tf_hold_frames_jpeg.  The decoder is teeflow_jpeg_core.h, the
// same text the host test runs under the sanitizers; the host has parsed every frame's header into a tfj::Desc, so every grid is known
// before the first launch and nothing between the kernels waits for the host.
//   k_jpeg_marks    one wave64 per frame: the RSTn positions and the end of the entropy data
//   k_jpeg_entropy  one wave64 per (frame, restart interval): Huffman decode into quantised coefficients, natural order, int16
//   k_jpeg_idct     one 8 x 8 block per lane: dequantise, islow IDCT, into the component planes at MCU-padded size
//   k_jpeg_finish   one pixel per lane: fancy upsampling, crop to H x W; interleaved [H][W][samples] or sample planes [samples][H * W]
// Where a stream is parsed a block is one wave and the parse is wave-uniform, as in k_inflate and k_rle_decode: the stream is read
// through the LDS stage of teeflow_wave_stage.hip.h and every table entry is made a scalar with readfirstlane.
//
// Per-frame scratch (the host sizes it, tf_jpeg host code): with PW, PH = W, H rounded up to 16 and plane = PW * PH, a frame has
// samples * plane coefficients, samples component planes of `plane` bytes and plane / 64 RSTn positions; every accepted sampling fits
// (an MCU row or column never passes PW or PH, and a frame has at most plane / 64 MCUs).
//
// Safety (a malformed stream is an expected input): a frame whose status is set is touched by no kernel after the one that set it.  The
// stream is read only through the staged reader, whose safety argument is teeflow_wave_stage.hip.h's, at positions below the frame's
// length.  k_jpeg_marks writes position k only with k < nint - 1 <= plane / 64; k_jpeg_entropy writes the 64 coefficients of block
// m * bpm + j only for MCU m < nmcu of its own interval; the other two kernels index by the descriptor alone, never by stream data.
// Loop bounds: the marks walk is the frame's length; a block's decode ends after at most 64 symbols, each of which moves the reader on
// or fails (teeflow_jpeg_core.h).
#pragma once
#define TFJ_FN __device__ inline
#define TFJ_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#include "teeflow_jpeg_core.h"
#include "teeflow_wave_stage.hip.h"

namespace jpeg {
constexpr uint32_t STAGE = 1024;            // bytes of a frame the LDS stage holds (tf_jpeg_stage_bytes tells the tests)

struct WaveIO : tfw::WaveStage<STAGE> {     // the frame is the stream
    __device__ uint8_t in_byte(uint32_t i)
    {
        const uint32_t at = i + skew;
        fill(at);
        return (uint8_t)__builtin_amdgcn_readfirstlane((int)stage[at % STAGE]);
    }
};

template <class IO>
__device__ void open_frame(IO& io, uint8_t* stage, const uint8_t* blob, unsigned long long o, uint32_t n, int lane)
{
    io.stage = stage;
    io.skew = (uint32_t)(o & 15); io.in = blob + (o - io.skew); io.in_len = n;
    io.ln = lane;
}

__device__ inline int status_of(const int* status, int f) { return __atomic_load_n(status + f, __ATOMIC_RELAXED); }
}  // namespace jpeg

// Block f: frame f.  A stage is looked at in 16 rounds of 64 consecutive bytes, lane i the pair that ends at byte 64 * round + i (the
// byte before a stage's first is carried over), so a ballot lists a round's marks in stream order.  rst + f * ni_max gets the
// positions, scan_end[f] the end; a wrong count or number sets status 3.
__global__ __launch_bounds__(64) void k_jpeg_marks(const uint8_t* __restrict__ blob, const unsigned long long* __restrict__ off,
                                                  const uint32_t* __restrict__ len, const tfj::Desc* __restrict__ desc, int n_frames,
                                                  uint32_t ni_max, uint32_t* __restrict__ rst, uint32_t* __restrict__ scan_end, int* status)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[jpeg::STAGE];
    const int f = (int)blockIdx.x, ln = (int)threadIdx.x;
    if (f >= n_frames || jpeg::status_of(status, f) != 0) return;
    const uint32_t n = len[f], nexp = desc[f].nint - 1;
    tfw::WaveStage<jpeg::STAGE> io;
    jpeg::open_frame(io, stage, blob, off[f], n, ln);
    uint32_t* list = rst + (size_t)f * ni_max;
    const uint32_t a0 = desc[f].scan_off + io.skew, a1 = n + io.skew;         // the pairs that end at q, a0 < q < a1
    uint32_t found = 0, end = n, carry = 0;
    bool bad = false, done = false;
    for (uint32_t base = a0 / jpeg::STAGE * jpeg::STAGE; base < a1 && !done; base += jpeg::STAGE) {
        io.fill(base);
        for (uint32_t r = 0; r < jpeg::STAGE / 64; ++r) {
            const uint32_t i = r * 64 + (uint32_t)ln, q = base + i;
            const uint32_t cur = stage[i], prev = i ? stage[i - 1] : carry;
            const bool pair = q > a0 && q < a1 && prev == 0xFF;
            const bool is_rst = pair && cur >= 0xD0 && cur <= 0xD7;
            const bool is_end = pair && !is_rst && cur != 0 && cur != 0xFF;
            const unsigned long long me = __ballot(is_end);
            unsigned long long mr = __ballot(is_rst);
            if (me) mr &= (me & (0ull - me)) - 1;                               // the RSTn before the first other marker
            if (mr) {
                const uint32_t idx = found + (uint32_t)__popcll(mr & ((1ull << ln) - 1));
                const bool mine = (mr >> ln) & 1, ok = idx < nexp && cur == 0xD0 + (idx & 7);
                if (mine && ok) list[idx] = q - 1 - io.skew;
                if (__ballot(mine && !ok)) bad = true;
                found += (uint32_t)__popcll(mr);
            }
            if (me) { end = base + r * 64 + (uint32_t)(__ffsll((long long)me) - 1) - 1 - io.skew; done = true; break; }
        }
        carry = stage[jpeg::STAGE - 1];
    }
    if (ln == 0) {
        scan_end[f] = end;
        if (bad || found != nexp) atomicMax(&status[f], (int)tfj::BAD_DATA);
    }
}

// Block (k, fb): restart interval k of frame f0 + fb; a frame without DRI is one interval.  coef + fb * coef_stride gets the frame's
// blocks in MCU order, 64 coefficients each.  The first error sets status 3 and ends the wave; a wave of a frame whose status is
// already set returns at once.
__global__ __launch_bounds__(64) void k_jpeg_entropy(const uint8_t* __restrict__ blob, const unsigned long long* __restrict__ off,
                                                    const uint32_t* __restrict__ len, const tfj::Desc* __restrict__ desc, int f0, uint32_t ni_max,
                                                    const uint32_t* __restrict__ rst, const uint32_t* __restrict__ scan_end,
                                                    int16_t* __restrict__ coef, size_t coef_stride, int* status)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[jpeg::STAGE];
    __shared__ tfj::Huff huff[4];
    __shared__ int16_t blk[64];
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
    const uint32_t m0 = d.ri ? k * d.ri : 0, m1 = d.ri && m0 + d.ri < d.nmcu ? m0 + d.ri : d.nmcu;
    int16_t* out = coef + (size_t)fb * coef_stride + (size_t)m0 * d.bpm * 64;
    int pred0 = 0, pred1 = 0, pred2 = 0, rc = tfj::OK;
    for (uint32_t m = m0; m < m1 && rc == tfj::OK; ++m)
        for (int j = 0; j < d.bpm; ++j) {
            int c, bx, by;
            tfj::mcu_block(d, j, &c, &bx, &by);
            blk[ln] = 0;
            __syncthreads();
            int pred = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
            rc = tfj::decode_block(io, b, huff[d.td[c]], huff[2 + d.ta[c]], &pred, [&](int at, int v) { blk[at] = (int16_t)v; });
            if (rc != tfj::OK) break;
            if (c == 0) pred0 = pred; else if (c == 1) pred1 = pred; else pred2 = pred;
            __syncthreads();
            out[ln] = blk[ln];
            out += 64;
        }
    if (rc != tfj::OK && ln == 0) atomicMax(&status[f], rc);
}

// Lane: block blockIdx.x * 64 + lane of frame f0 + fb, in the order k_jpeg_entropy stored them.  planes + (fb * samples + c) *
// plane_bytes is component c of the frame, comp_pitch bytes a row.  idct_block's workspace of 64 words and its zig-zag table stay out
// of memory: the loops unroll, the table folds into constant indices and the workspace lives in registers (the build's assembly for
// gfx950: 105 VGPRs, private segment 0 bytes, no scratch instruction in any of the four kernels).
__global__ __launch_bounds__(64) void k_jpeg_idct(const tfj::Desc* __restrict__ desc, int f0, const int16_t* __restrict__ coef, size_t coef_stride,
                                                 uint8_t* __restrict__ planes, size_t plane_bytes, int samples, const int* status)
{
    const int fb = (int)blockIdx.y, f = f0 + fb;
    const tfj::Desc& d = desc[f];
    const uint32_t bid = blockIdx.x * 64 + threadIdx.x;
    if (jpeg::status_of(status, f) != 0 || bid >= d.nmcu * d.bpm) return;
    const uint32_t m = bid / d.bpm;
    int c, bx, by;
    tfj::mcu_block(d, (int)(bid % d.bpm), &c, &bx, &by);
    const size_t pitch = (size_t)tfj::comp_pitch(d, c);
    const size_t x0 = ((size_t)(m % d.mcux) * d.h[c] + bx) * 8, y0 = ((size_t)(m / d.mcux) * d.v[c] + by) * 8;
    tfj::idct_block(coef + (size_t)fb * coef_stride + (size_t)bid * 64, d.q[d.tq[c]], planes + ((size_t)fb * samples + c) * plane_bytes + y0 * pitch + x0, pitch);
}

// Lane: pixel blockIdx.x * 256 + lane of frame f0 + fb.  out is the call's whole output, frame f0 + fb at its own place: interleaved
// [N][H][W][samples], or (planar) [N][samples][H * W], k_ingest_planar's layout.  A frame whose status is set is not written.
__global__ __launch_bounds__(256) void k_jpeg_finish(const tfj::Desc* __restrict__ desc, int f0, const uint8_t* __restrict__ planes, size_t plane_bytes,
                                                    int samples, int H, int W, int planar, uint8_t* __restrict__ out, const int* status)
{
    const int fb = (int)blockIdx.y, f = f0 + fb;
    const size_t hw = (size_t)H * W, px = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (px >= hw || jpeg::status_of(status, f) != 0) return;
    const tfj::Desc& d = desc[f];
    const int y = (int)(px / (size_t)W), x = (int)(px - (size_t)y * W);
    const uint8_t* fp = planes + (size_t)fb * samples * plane_bytes;
    for (int c = 0; c < samples; ++c) {
        const uint8_t s = tfj::frame_sample(d, fp, plane_bytes, H, W, c, x, y);
        if (planar) out[((size_t)f * samples + c) * hw + px] = s;
        else out[((size_t)f * hw + px) * samples + c] = s;
    }
}
