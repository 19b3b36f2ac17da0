// Inflate on the device: the gzip chunks of a study file, independent zlib streams, one wave64 per stream (k_inflate), and their
// assembly from chunk-major bytes into the row-major array (k_unchunk).  The decoder is teeflow_inflate_core.h, the same text the host
// test runs under the sanitizers; this header is its IO on a wave.
//
// A block is one wave.  Symbol decode is serial: every lane runs it with the same state, so the control flow is wave-uniform and
// table and window reads are broadcasts.  What is parallel is shared out by lane: the table fills, the LZ77 copy (lane i copies byte
// i, modulo the distance when the match overlaps itself), the staging of the input, and the flush of the window with its Adler-32.
// The 32 KiB window is a ring in LDS and the only place back-references read: no lane ever reads back what the wave stored to global
// memory.  Ring 32 KiB + input stage 1 KiB + tables 3.6 KiB = 37,440 B per block: four blocks per CU.
//
// Safety (a malformed stream is an expected input): the decoder asks for input byte i only with i < len, and the input is read
// through the staged reader, whose safety argument is teeflow_wave_stage.hip.h's; put / copy / stored refuse what would pass the
// slot's out_bytes before writing; flush writes [flushed, flushed + n) with flushed + n <= produced <= out_bytes.  Loop bounds:
// teeflow_inflate_core.h.
#pragma once
#define TFI_FN __device__ inline
#include "teeflow_inflate_core.h"
#include "teeflow_wave_stage.hip.h"

namespace inflate {
constexpr uint32_t RING = tfi::WINDOW, STAGE = 1024, FLUSH = 4096;

struct WaveIO : tfw::WaveStage<STAGE> {
    uint8_t* ring;                              // LDS
    uint8_t* out; uint32_t cap;                 // the stream's slot (16-byte aligned) and its size
    uint32_t n = 0, flushed = 0;                // bytes produced / written out
    uint32_t a = 1, b = 0;                      // Adler-32 of the flushed bytes

    __device__ int lane() const { return ln; }
    __device__ int lanes() const { return 64; }
    __device__ void sync() { __syncthreads(); }         // (a block is one wave: this orders the wave's LDS traffic)
    __device__ uint32_t produced() const { return n; }

    __device__ uint8_t in_byte(uint32_t i)
    {
        const uint32_t at = i + skew;
        fill(at);
        return stage[at % STAGE];
    }

    // n_ more bytes [flushed, flushed + n_) from the ring to the slot, and into the checksum.  flushed is a multiple of 16.
    __device__ void flush(uint32_t n_)
    {
        __syncthreads();
        uint32_t s1 = 0; unsigned long long s2 = 0;
        const uint32_t whole = n_ & ~15u;
        for (uint32_t c = (uint32_t)ln * 16; c < whole; c += 1024) {
            const uint4 v = *(const uint4*)(ring + ((flushed + c) & (RING - 1)));
            *(uint4*)(out + flushed + c) = v;
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint32_t t1 = 0, t2 = 0;                                          // sum d, sum j d over the 16 bytes
#pragma unroll
            for (int j = 0; j < 16; ++j) { const uint32_t d = (w[j >> 2] >> (8 * (j & 3))) & 255; t1 += d; t2 += (uint32_t)j * d; }
            s1 += t1; s2 += (unsigned long long)(n_ - c) * t1 - t2;
        }
        const uint32_t i = whole + (uint32_t)ln;
        if (i < n_) {
            const uint32_t d = ring[(flushed + i) & (RING - 1)];
            out[flushed + i] = (uint8_t)d;
            s1 += d; s2 += (unsigned long long)(n_ - i) * d;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { s1 += __shfl_xor(s1, m, 64); s2 += __shfl_xor(s2, m, 64); }
        b = (uint32_t)((b + (unsigned long long)n_ * a + s2) % 65521u);
        a = (a + s1) % 65521u;
        flushed += n_;
    }
    __device__ void advance(uint32_t k)
    {
        n += k;
        while (n - flushed >= FLUSH) flush(FLUSH);
    }

    __device__ bool put(uint8_t v)
    {
        if (n >= cap) return false;
        if (ln == 0) ring[n & (RING - 1)] = v;
        advance(1);
        return true;
    }
    __device__ int copy(uint32_t dist, uint32_t len)
    {
        if (dist > n) return tfi::BAD_DISTANCE;
        if (len > cap - n) return tfi::BAD_OUTPUT_SIZE;
        __syncthreads();
        const uint32_t from = n - dist;
        // (dist <= 32768 = RING: a source byte is never one this match has written, and a destination aliases only the source of the
        // same or an earlier lane, which was read by then)
        for (uint32_t k = (uint32_t)ln; k < len; k += 64) ring[(n + k) & (RING - 1)] = ring[(from + (k < dist ? k : k % dist)) & (RING - 1)];
        advance(len);
        return tfi::OK;
    }
    __device__ int stored(uint32_t pos, uint32_t cnt)
    {
        if (cnt > cap - n) return tfi::BAD_OUTPUT_SIZE;
        while (cnt) {
            const uint32_t at = pos + skew;
            uint32_t m = within(at);
            if (m > cnt) m = cnt;
            fill(at);                                                         // the stage holds [pos, pos + m)
            for (uint32_t k = (uint32_t)ln; k < m; k += 64) ring[(n + k) & (RING - 1)] = stage[(at + k) & (STAGE - 1)];
            advance(m);
            pos += m; cnt -= m;
        }
        return tfi::OK;
    }
    __device__ uint32_t finish()
    {
        if (n > flushed) flush(n - flushed);
        return b << 16 | a;
    }
};
}  // namespace inflate

// Stream s = blockIdx.x: len[s] bytes at blob + off[s] (blob 16-byte aligned) -> out + s * stride (stride a multiple of 16, >= out_bytes),
// status[s].  A raw stream (stored unfiltered in the file) is not decoded: its status says whether its length is out_bytes.
__global__ __launch_bounds__(64) void k_inflate(const uint8_t* __restrict__ blob, const unsigned long long* __restrict__ off,
                                                const uint32_t* __restrict__ len, const uint8_t* __restrict__ raw, int n, uint32_t out_bytes,
                                                size_t stride, uint8_t* __restrict__ out, int* __restrict__ status, uint32_t* __restrict__ produced)
{
    __shared__ __attribute__((aligned(16))) uint8_t ring[inflate::RING];
    __shared__ __attribute__((aligned(16))) uint8_t stage[inflate::STAGE];
    __shared__ tfi::Tables tables;
    const int s = blockIdx.x;
    if (s >= n) return;
    int rc;
    uint32_t made = 0;
    if (raw && raw[s]) rc = len[s] == out_bytes ? tfi::OK : tfi::BAD_OUTPUT_SIZE;
    else {
        inflate::WaveIO io;
        io.ring = ring; io.stage = stage;
        const unsigned long long o = off[s];
        io.skew = (uint32_t)(o & 15); io.in = blob + (o - io.skew); io.in_len = len[s];
        io.out = out + (size_t)s * stride; io.cap = out_bytes;
        io.ln = threadIdx.x;
        rc = tfi::inflate_zlib(io, tables, io.in_len, out_bytes);
        made = io.produced();
    }
    if (threadIdx.x == 0) { status[s] = rc; produced[s] = made; }
}

// Chunk c = blockIdx.x of a chunked dataset: its chunk[0] x .. x chunk[3] elements of T, row-major, at src(c), to their places in the
// row-major array dst of shape[0] x .. x shape[3]; the chunk's first element sits at coord[c][0..3].  What lies outside the array (an
// edge chunk's overhang) is dropped.  src(c): inflated + c * stride, or, raw[c], the file's own bytes blob + off[c].
struct UnchunkDims { long long shape[4], chunk[4]; };
template <typename T>
__global__ __launch_bounds__(256) void k_unchunk(const uint8_t* __restrict__ inflated, size_t stride, const uint8_t* __restrict__ blob,
                                                 const unsigned long long* __restrict__ off, const uint8_t* __restrict__ raw,
                                                 const long long* __restrict__ coord, const int* __restrict__ status, UnchunkDims d,
                                                 T* __restrict__ dst)
{
    const int c = blockIdx.x;
    if (status[c] != 0) return;
    const uint8_t* src = raw && raw[c] ? blob + off[c] : inflated + (size_t)c * stride;
    const long long c0 = coord[4 * c], c1 = coord[4 * c + 1], c2 = coord[4 * c + 2], c3 = coord[4 * c + 3];
    // (the host has checked: a chunk is at most 2^30 bytes, so its extents and element count fit 32 bits)
    const uint32_t k1 = (uint32_t)d.chunk[1], k2 = (uint32_t)d.chunk[2], k3 = (uint32_t)d.chunk[3];
    const uint32_t elems = (uint32_t)d.chunk[0] * k1 * k2 * k3;
    for (uint32_t e = blockIdx.y * blockDim.x + threadIdx.x; e < elems; e += gridDim.y * blockDim.x) {
        uint32_t r = e;
        const uint32_t i3 = r % k3; r /= k3;
        const uint32_t i2 = r % k2; r /= k2;
        const uint32_t i1 = r % k1;
        const uint32_t i0 = r / k1;
        const long long g0 = c0 + i0, g1 = c1 + i1, g2 = c2 + i2, g3 = c3 + i3;
        if (g0 >= d.shape[0] || g1 >= d.shape[1] || g2 >= d.shape[2] || g3 >= d.shape[3]) continue;
        T v;
        __builtin_memcpy(&v, src + (size_t)e * sizeof(T), sizeof(T));         // (a raw chunk's bytes sit at any offset of the file's)
        dst[((g0 * d.shape[1] + g1) * d.shape[2] + g2) * d.shape[3] + g3] = v;
    }
}
