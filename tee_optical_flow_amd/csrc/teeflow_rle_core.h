// DICOM RLE Lossless (transfer syntax 1.2.840.10008.1.2.5, PS3.5 Annex G), 8-bit samples: one frame's header and one segment's
// PackBits decode, in plain C++ that compiles for the device (teeflow_rle.hip.h: TFR_FN = __device__, the IO a wave64 with its input
// staged in LDS) and for the host (tests/csrc/verify_rle.cpp, under the address and undefined-behaviour sanitizers, with buffers of
// the exact size).  frames.rle_decode_frame is the numpy / Python twin.
//
// A frame: a 64-byte header -- a little-endian uint32 segment count, then fifteen little-endian uint32 offsets counted from the frame's
// first byte -- and the segments.  Segment k is the k-th sample plane, H * W bytes, PackBits-coded; it ends where the next one starts,
// the last one at the frame's end.  PackBits, a control byte c read as int8: 0..127 copy the next c + 1 bytes; -1..-127 write the next
// byte 1 - c times; -128 nothing.
//
// What the standard leaves to the decoder is pinned here, so that the first H * W bytes are what a decode-then-trim reader keeps:
//   * a segment's decode stops once H * W bytes are produced; what is left of the segment (the even-length pad byte, padding that does
//     not conform, trailing garbage) is ignored;
//   * runs and literals may cross row ends;
//   * a literal cut off by the segment's end contributes the bytes that exist; a run whose value byte is missing contributes nothing;
//   * a segment that ends with fewer than H * W bytes produced fails.
// Per-frame status: 0 ok; 1 bad header (frame shorter than 64 bytes, or segment count != samples); 2 bad offsets (a first offset other
// than 64 is allowed, but every offset must be >= 64, < the frame's length and strictly ascending); 3 a segment decoded short.
// Annex G is the specification.  What pydicom's handler makes of a malformed stream is NOT pinned: a valid stream has one decoding,
// an invalid one is refused or decoded by the rules above.
//
// Safety by construction: frame byte i is asked for only with i < len (segment byte i only with i < the segment's length); a
// literal or run is clipped to what the plane still lacks before the IO writes it; every loop iteration consumes at least one input byte.
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifndef TFR_FN
#define TFR_FN inline
#endif

namespace tfr {
enum : int { OK = 0, BAD_HEADER = 1, BAD_OFFSETS = 2, SHORT_SEGMENT = 3 };
constexpr uint32_t HEADER = 64;
constexpr int MAX_SEGMENTS = 15;

// byte(i): byte i of the frame, i < len
template <class BYTE>
TFR_FN uint32_t le32(BYTE& byte, uint32_t i)
{
    return (uint32_t)byte(i) | ((uint32_t)byte(i + 1) << 8) | ((uint32_t)byte(i + 2) << 16) | ((uint32_t)byte(i + 3) << 24);
}

// The header of a frame of len bytes that is to hold `samples` (1..15) segments: the frame's status (OK, BAD_HEADER, BAD_OFFSETS: the
// same whatever k), and, where it is OK, bytes [*start, *end) of the frame as segment k (0 <= k < samples).
template <class BYTE>
TFR_FN int frame_segment(BYTE& byte, uint32_t len, int samples, int k, uint32_t* start, uint32_t* end)
{
    if (len < HEADER || le32(byte, 0) != (uint32_t)samples) return BAD_HEADER;
    uint32_t prev = 0;
    *start = *end = len;
    for (int s = 0; s < samples; ++s) {
        const uint32_t o = le32(byte, 4 + 4 * (uint32_t)s);
        if (o < HEADER || o >= len || (s && o <= prev)) return BAD_OFFSETS;
        if (s == k) *start = o;
        if (s == k + 1) *end = o;
        prev = o;
    }
    return OK;
}

// One segment of n_in bytes -> its plane of `plane` = H * W bytes.  IO:
//   uint8_t in_byte(uint32_t i)                               segment byte i, i < n_in
//   void literal(uint32_t pos, uint32_t made, uint32_t cnt)   segment bytes [pos, pos + cnt) to plane bytes [made, made + cnt)
//   void run(uint32_t made, uint8_t v, uint32_t cnt)          v to plane bytes [made, made + cnt)
// with pos + cnt <= n_in and made + cnt <= plane; cnt may be 0.  -> OK or SHORT_SEGMENT.
template <class IO>
TFR_FN int decode_segment(IO& io, uint32_t n_in, uint32_t plane)
{
    uint32_t pos = 0, made = 0;
    while (made < plane && pos < n_in) {
        const int c = (int8_t)io.in_byte(pos++);
        if (c >= 0) {
            uint32_t cnt = (uint32_t)c + 1;
            if (cnt > n_in - pos) cnt = n_in - pos;              // cut off by the segment's end: the bytes that exist
            if (cnt > plane - made) cnt = plane - made;
            io.literal(pos, made, cnt);
            pos += cnt; made += cnt;
        } else if (c != -128) {
            if (pos >= n_in) break;                              // no value byte: nothing
            const uint8_t v = io.in_byte(pos++);
            uint32_t cnt = (uint32_t)(1 - c);
            if (cnt > plane - made) cnt = plane - made;
            io.run(made, v, cnt);
            made += cnt;
        }
    }
    return made == plane ? OK : SHORT_SEGMENT;
}
}  // namespace tfr
