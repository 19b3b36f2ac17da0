// A batch of byte streams on its way to the device: the one format that k_inflate (zlib streams) and k_rle_decode (RLE frames) read
// their input in, in plain C++ with no HIP, so that tests/csrc/verify_streams.cpp runs it under the sanitizers.  The upload and the
// verdict are teeflow_streams_host.hip.h's, the reader on the device is teeflow_wave_stage.hip.h's.
//
// The caller describes n streams as (blob, off[], len[]): stream i is the len[i] bytes at blob + off[i], anywhere in the blob, in any
// order, overlapping or not.  The format on the device:
//   * the span [lo, hi) of the blob that holds every stream is copied, nothing else, to byte `skew` = lo & 15 of a scratch buffer whose
//     first byte is 16-byte aligned: the copy keeps the blob's alignment mod 16, and a stream's offset in it is off - lo + skew;
//   * the buffer is PAD bytes longer than skew + (hi - lo), so every 16-byte aligned piece that overlaps a stream lies inside it;
//   * the per-stream table is columns end to end, each column n entries of one width, widest entries first so that every column is
//     aligned to its entry: the rewritten offsets (u64), the lengths (u32), and whatever else the kernel takes, zeroed.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>

namespace tfs {
constexpr size_t PIECE = 16, PAD = 2 * PIECE;
constexpr uint64_t OFF_LIMIT = ~0ull >> 1;                    // off + len stays below 2^63

struct Batch {
    const uint8_t* blob; const uint64_t* off; const uint32_t* len; int n;
    uint64_t lo = 0, hi = 0;                                  // [lo, hi) of the blob holds every stream (span)
    size_t skew() const { return (size_t)(lo & (PIECE - 1)); }
    size_t bytes() const { return (size_t)(hi - lo); }        // what is uploaded
    size_t device_bytes() const { return skew() + bytes() + PAD; }
};

// lo and hi of b (both 0 for an empty batch).  A stream of more than `cap` bytes, or one whose off + len passes OFF_LIMIT, is refused:
// false, and `msg` says which `noun` ("stream", "frame") and why.
inline bool span(Batch& b, uint32_t cap, const char* noun, char* msg, size_t msg_bytes)
{
    b.lo = b.n > 0 ? ~0ull : 0; b.hi = 0;
    for (int i = 0; i < b.n; ++i) {
        const uint64_t o = b.off[i]; const uint32_t l = b.len[i];
        if (l > cap) { snprintf(msg, msg_bytes, "%s %d has %u bytes, at most %u", noun, i, l, cap); return false; }
        if (o > OFF_LIMIT - l) { snprintf(msg, msg_bytes, "%s %d starts at byte %llu: off + len (%u) overflows", noun, i, (unsigned long long)o, l); return false; }
        b.lo = std::min(b.lo, o); b.hi = std::max(b.hi, o + l);
    }
    return true;
}

// The host side of the per-stream table.  at[c]: the first byte of column c; at[columns]: the table's size.
struct Table {
    std::vector<size_t> at; std::vector<uint8_t> bytes;
    uint8_t* col(int c) { return bytes.data() + at[c]; }
};

// widths: the bytes of one entry of each column.  Column col_off (8) gets each stream's offset in the device copy, column col_len (4)
// its length; every other column is zero.  b has been through span().
inline Table table(const Batch& b, std::initializer_list<size_t> widths, int col_off, int col_len)
{
    const size_t n = b.n > 0 ? (size_t)b.n : 0;
    Table t;
    size_t at = 0;
    for (size_t w : widths) { t.at.push_back(at); at += n * w; }
    t.at.push_back(at);
    t.bytes.assign(at, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t o = b.off[i] - b.lo + b.skew();
        memcpy(t.col(col_off) + i * 8, &o, 8);
    }
    if (n) memcpy(t.col(col_len), b.len, n * 4);
    return t;
}
}  // namespace tfs
