// The staged reader of the one-wave-per-stream kernels (k_inflate, k_rle_decode): a wave64 reads its stream through an LDS stage of
// STAGE bytes, refilled 16 bytes a lane, and the decoders' byte reads are LDS reads at a wave-uniform address.  The other half of the
// format of teeflow_streams_core.h.
//
// Safety (a malformed stream is an expected input): the decoder asks for stream byte i only with i < in_len, and fill() loads a whole
// 16-byte piece only where the piece overlaps the stream, piece < skew + in_len.  The library's device copy of the blob starts
// 16-byte aligned, keeps the blob's alignment mod 16 and is padded past its end (tfs::PAD), so such a piece lies inside the copy
// whatever the caller's blob is; a piece that overlaps nothing is staged as zeros and never asked for.  in_len is bounded by the host
// so that skew + in_len does not wrap.
#pragma once

namespace tfw {
template <uint32_t STAGE>
struct WaveStage {
    static_assert(STAGE == 64 * 16, "a refill is one 16-byte piece a lane of a wave64");
    uint8_t* stage;                             // LDS, STAGE bytes, 16-byte aligned
    const uint8_t* in;                          // the stream's first byte less `skew`: 16-byte aligned
    uint32_t skew, in_len;
    uint32_t unit = 0xFFFFFFFFu;                // which STAGE bytes of `in` the stage holds
    int ln;

    // the stage holds the unit of byte `at` of `in` (at = i + skew for stream byte i).  A refill waits for its own load: loading the
    // next unit a refill ahead into registers was tried in k_rle_decode, with a clipped and with an unconditional load, and was slower
    // both times (1.17 -> 1.43 ms on the 512 x 512 study of tools/rle_frames_bench.py).
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
    // how many bytes from `at` on the unit of `at` holds: a copy of stream bytes goes piece by piece of what one stage holds, each
    // piece the lesser of this and what is left to copy
    __device__ uint32_t within(uint32_t at) const { return STAGE - at % STAGE; }
};
}  // namespace tfw
