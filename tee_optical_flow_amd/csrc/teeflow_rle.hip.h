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
// asks for segment byte i only with i < the segment's length, and the segment is read through the staged reader, whose safety
// argument is teeflow_wave_stage.hip.h's; the core clips a literal or run to what the plane still lacks.  Loop bounds:
// teeflow_rle_core.h.
#pragma once
#define TFR_FN __device__ inline
#include "teeflow_rle_core.h"
#include "teeflow_wave_stage.hip.h"

namespace rle {
constexpr uint32_t STAGE = 1024;            // bytes of a segment the LDS stage holds (tf_rle_stage_bytes tells the tests)

struct WaveIO : tfw::WaveStage<STAGE> {         // the segment is the stream
    uint8_t* out;                               // the segment's plane

    __device__ uint8_t in_byte(uint32_t i)
    {
        const uint32_t at = i + skew;
        fill(at);
        return (uint8_t)__builtin_amdgcn_readfirstlane((int)stage[at % STAGE]);
    }
    __device__ void literal(uint32_t pos, uint32_t made, uint32_t cnt)
    {
        while (cnt) {
            const uint32_t at = pos + skew;
            uint32_t m = within(at);
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
