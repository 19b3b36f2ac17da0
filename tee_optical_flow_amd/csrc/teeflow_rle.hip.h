// DICOM RLE Lossless on the device: k_rle_decode, one wave64 per (frame, segment), as k_inflate gives each stream one wave.  The decoder
// is teeflow_rle_core.h, the same text the host test runs under the sanitizers; this header is its IO on a wave.
//
// A block is one wave.  The parse is serial: every lane runs it with the same state.  The control byte (and a run's value byte) is read
// from the LDS stage at one address -- a broadcast -- and made a scalar with readfirstlane, so the hop from control byte to control
// byte is wave-uniform scalar control flow.  What is parallel is shared out by lane: the staging of the input (16 bytes a lane, STAGE =
// 1 KiB a refill) and the literal or run itself (lane i writes byte i; at most 128 bytes, so two lane rounds).  A plane is written
// front to back with contiguous byte stores into the planar scratch [N][samples][H * W]; no lane ever reads back what the wave stored,
// so the hop chain waits on no store.  Interleaving the planes is k_ingest_planar's (teeflow_ingest.hip.h).
//
// Safety (a malformed stream is an expected input): the header is read from the frame's own bytes, byte i only with i < len; the core
// asks for segment byte i only with i < the segment's length, and fill() stages whole 16-byte pieces only where they overlap the
// segment (the library's device copy of the blob starts 16-byte aligned and is padded past its end, so such a piece lies inside the
// copy whatever the caller's blob is); the core clips a literal or run to what the plane still lacks.  Loop bounds: teeflow_rle_core.h.
#pragma once
#define TFR_FN __device__ inline
#include "teeflow_rle_core.h"

namespace rle {
constexpr uint32_t STAGE = 1024;            // bytes of a segment the LDS stage holds (tf_rle_stage_bytes tells the tests)

struct WaveIO {
    uint8_t* stage;                             // LDS
    const uint8_t* in;                          // the segment's first byte less `skew`: 16-byte aligned
    uint32_t skew, in_len;
    uint8_t* out;                               // the segment's plane
    uint32_t unit = 0xFFFFFFFFu;                // which STAGE bytes of the input the stage holds
    int ln;

    // the stage holds the unit of byte `at` of `in` (the host has bounded a frame's length so that none of this wraps, rle_check).
    // A refill waits for its own load: loading the next unit a refill ahead into registers was tried, with a clipped and with an
    // unconditional load, and was slower both times (1.17 -> 1.43 ms on the 512 x 512 study of tools/rle_frames_bench.py).
    __device__ void fill(uint32_t at)
    {
        if (at / STAGE == unit) return;
        unit = at / STAGE;
        __syncthreads();                                                      // (a block is one wave: this orders the wave's LDS traffic)
        const uint32_t piece = unit * STAGE + (uint32_t)ln * 16;              // this lane's 16 bytes, from `in`
        uint4 v = make_uint4(0, 0, 0, 0);
        if (piece < skew + in_len) v = *(const uint4*)(in + piece);
        *(uint4*)(stage + ln * 16) = v;
        __syncthreads();
    }
    __device__ uint8_t in_byte(uint32_t i)
    {
        const uint32_t at = i + skew;
        fill(at);
        return (uint8_t)__builtin_amdgcn_readfirstlane((int)stage[at % STAGE]);
    }
    __device__ void literal(uint32_t pos, uint32_t made, uint32_t cnt)
    {
        while (cnt) {                                                         // piece by piece of what one stage holds
            const uint32_t at = pos + skew;
            uint32_t m = STAGE - at % STAGE;
            if (m > cnt) m = cnt;
            fill(at);                                                         // the stage holds [pos, pos + m)
            for (uint32_t k = (uint32_t)ln; k < m; k += 64) out[made + k] = stage[(at + k) % STAGE];
            pos += m; made += m; cnt -= m;
        }
    }
    __device__ void run(uint32_t made, uint8_t v, uint32_t cnt)
    {
        for (uint32_t k = (uint32_t)ln; k < cnt; k += 64) out[made + k] = v;
    }
};
}  // namespace rle

// Block b: segment b % samples of frame f = b / samples -- the len[f] bytes at blob + off[f] (blob 16-byte aligned and padded, above) --
// -> plane (f * samples + b % samples) of out, `plane` = H * W bytes each.  status[f], zero at the launch, gets the frame's status: the
// header's is the same in every wave of the frame, a short segment's comes from the wave that met it.
__global__ __launch_bounds__(64) void k_rle_decode(const uint8_t* __restrict__ blob, const unsigned long long* __restrict__ off,
                                                   const uint32_t* __restrict__ len, int n_frames, int samples, uint32_t plane,
                                                   uint8_t* __restrict__ out, int* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[rle::STAGE];
    const int f = (int)(blockIdx.x / (unsigned)samples), k = (int)(blockIdx.x % (unsigned)samples);
    if (f >= n_frames) return;
    const unsigned long long o = off[f];
    const uint32_t n = len[f];
    const uint8_t* frame = blob + o;
    auto byte = [&](uint32_t i) -> uint8_t { return frame[i]; };
    uint32_t s0 = 0, s1 = 0;
    int rc = tfr::frame_segment(byte, n, samples, k, &s0, &s1);
    if (rc == tfr::OK) {
        rle::WaveIO io;
        const unsigned long long so = o + s0;
        io.stage = stage;
        io.skew = (uint32_t)(so & 15); io.in = blob + (so - io.skew); io.in_len = s1 - s0;
        io.out = out + ((size_t)f * samples + k) * plane;
        io.ln = threadIdx.x;
        rc = tfr::decode_segment(io, s1 - s0, plane);
    }
    if (rc != tfr::OK && threadIdx.x == 0) atomicMax(&status[f], rc);
}
