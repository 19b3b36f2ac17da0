// Inflate of one zlib stream (RFC 1950 wrapper, RFC 1951 body): the table construction, the symbol decode and the block loop, in plain
// C++ that compiles for the device (teeflow_inflate.hip.h: one wave64 per stream, TFI_FN = __device__) and for the host
// (tests/csrc/verify_inflate.cpp: one lane, under the address and undefined-behaviour sanitizers).  Written for this project from the
// two RFCs; which code-length sets are accepted follows what zlib accepts (stated at build_code).
//
// The decoder is written once over an IO policy, which owns the bytes: where the input comes from, where the output and its 32 KiB
// window live, how a match is copied and what the output's Adler-32 is.  Every lane of a wave runs the decoder with the same state
// (the control flow is wave-uniform); the IO says which lane it is, so that table fills are shared out and a table is written once.
//   uint8_t  in_byte(uint32_t i)                  input byte i, i < the stream's length (the decoder never asks for another)
//   bool     put(uint8_t b)                       one output byte; false: the slot is full
//   int      copy(uint32_t dist, uint32_t len)    a match: status (OK, BAD_DISTANCE, BAD_OUTPUT_SIZE)
//   int      stored(uint32_t pos, uint32_t n)     n input bytes from pos to the output: status (OK, BAD_OUTPUT_SIZE)
//   uint32_t produced()                           output bytes so far
//   uint32_t finish()                             everything is written out; the Adler-32 of the output
//   int lane(), lanes(); void sync()              this lane, the lanes that run the decoder together, a barrier among them
// Every loop here consumes at least one input bit or produces at least one output byte per iteration, and ends when the input is
// exhausted or the slot is full: a malformed stream neither hangs nor writes outside its slot.
#pragma once
#include <stdint.h>

#ifndef TFI_FN
#define TFI_FN inline
#endif

namespace tfi {
// a stream's status (tf_inflate's status[], include/teeflow.h)
enum : int { OK = 0, BAD_HEADER = 1, BAD_BLOCK_TYPE = 2, BAD_STORED_LEN = 3,
             BAD_CODE_LENGTHS = 4,    // ... or a code the lengths do not define
             BAD_DISTANCE = 5, TRUNCATED = 6, BAD_OUTPUT_SIZE = 7, BAD_CHECKSUM = 8 };

constexpr int LIT_BITS = 10, DIST_BITS = 8, CLEN_BITS = 7;      // index bits of the one-step tables; longer codes take the canonical walk
constexpr int N_LIT = 288, N_DIST = 32, N_CLEN = 19;
constexpr uint32_t WINDOW = 32768;
enum Kind { CLEN, LIT, DIST };

// One canonical Huffman code: how many codes each length has, the symbols in canonical order (length << 9 | symbol), the one-step
// table (the entry of a code of length <= bits at every index whose low bits are the reversed code; 0: none), and per length the
// first code and its place in `sorted`.
struct Tables {
    uint16_t lit_fast[1 << LIT_BITS];
    uint16_t dist_fast[1 << DIST_BITS];        // (the code-length code's table while a dynamic header is read)
    uint16_t lit_sorted[N_LIT], dist_sorted[N_DIST];
    uint16_t lit_count[16], dist_count[16];
    uint16_t first[16], base[16];              // build_code's scratch
    uint8_t lens[N_LIT + N_DIST];
};

struct Code { const uint16_t* count; const uint16_t* sorted; const uint16_t* fast; int bits; };

struct Bits {
    uint64_t buf = 0; uint32_t cnt = 0;        // cnt valid bits of buf, the next one lowest
    uint32_t pos = 0, len = 0;                 // the next input byte; the stream's length
};

template <class IO> TFI_FN void refill(IO& io, Bits& b)
{
    while (b.cnt <= 56 && b.pos < b.len) { b.buf |= (uint64_t)io.in_byte(b.pos) << b.cnt; ++b.pos; b.cnt += 8; }
}
TFI_FN void drop(Bits& b, uint32_t n) { b.buf >>= n; b.cnt -= n; }     // n <= cnt, n < 64

TFI_FN uint32_t reverse_bits(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}

// lens[0, n) -> the code.  As zlib: an over-subscribed set is refused; an incomplete one too, unless its only code has length 1 (the
// distance set of Z_RLE output) and it is not the code-length code; a set without any code is accepted and decodes nothing
// (Z_HUFFMAN_ONLY's distance set).  Called by every lane; the status is the same on all.
template <class IO> TFI_FN int build_code(IO& io, Tables& t, Kind kind, const uint8_t* lens, int n)
{
    uint16_t* count = kind == LIT ? t.lit_count : t.dist_count;
    uint16_t* sorted = kind == LIT ? t.lit_sorted : t.dist_sorted;
    uint16_t* fast = kind == LIT ? t.lit_fast : t.dist_fast;
    const int bits = kind == LIT ? LIT_BITS : kind == DIST ? DIST_BITS : CLEN_BITS;
    const int lane = io.lane(), nl = io.lanes();
    io.sync();                                                        // the lengths are written, the last user of the tables is done
    if (lane == 0) {
        for (int l = 0; l < 16; ++l) count[l] = 0;
        for (int s = 0; s < n; ++s) ++count[lens[s]];
        count[0] = 0;
        uint32_t code = 0, at = 0;
        for (int l = 1; l < 16; ++l) {
            code = (code + count[l - 1]) << 1;                         // (16 bits hold it: an over-subscribed set is refused below)
            t.first[l] = (uint16_t)code; t.base[l] = (uint16_t)at;
            at += count[l];
        }
        t.first[0] = t.base[0] = 0;
    }
    for (int i = lane; i < (1 << bits); i += nl) fast[i] = 0;
    io.sync();
    int left = 1, max = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)count[l];
        if (left < 0) return BAD_CODE_LENGTHS;                        // over-subscribed
        if (count[l]) max = l;
    }
    if (max == 0) return OK;                                          // no codes: nothing decodes
    if (left > 0 && (kind == CLEN || max != 1)) return BAD_CODE_LENGTHS;   // incomplete
    if (lane == 0) {                                                  // canonical order: by length, then by symbol
        for (int s = 0; s < n; ++s) {
            const int l = lens[s];
            if (l) { sorted[t.base[l]] = (uint16_t)(l << 9 | s); ++t.base[l]; }
        }
        for (int l = 1; l < 16; ++l) t.base[l] = (uint16_t)(t.base[l] - count[l]);
    }
    io.sync();
    int total = 0;
    for (int l = 1; l < 16; ++l) total += count[l];
    for (int i = lane; i < total; i += nl) {
        const uint16_t e = sorted[i];
        const int l = e >> 9;
        if (l > bits) continue;
        const uint32_t code = (uint32_t)t.first[l] + (uint32_t)(i - t.base[l]);
        for (uint32_t k = reverse_bits(code, l); k < (1u << bits); k += 1u << l) fast[k] = e;
    }
    io.sync();
    return OK;
}

// the next symbol of code c, or -status.  The caller has refilled: fewer than 15 valid bits means the input ends there.
TFI_FN int decode(Bits& b, const Code& c)
{
    const uint16_t e = c.fast[b.buf & ((1u << c.bits) - 1)];
    if (e) {
        const uint32_t l = e >> 9;
        if (l > b.cnt) return -TRUNCATED;
        drop(b, l);
        return e & 511;
    }
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        if (b.cnt < l) return -TRUNCATED;
        code |= (int)(b.buf >> (l - 1)) & 1;
        const int n = c.count[l];
        if (code - first < n) { drop(b, l); return c.sorted[index + (code - first)] & 511; }
        index += n; first = (first + n) << 1; code <<= 1;
    }
    return -BAD_CODE_LENGTHS;                                         // a code the lengths do not define
}

// the symbols of one fixed or dynamic block, up to its end-of-block
template <class IO> TFI_FN int inflate_codes(IO& io, const Tables& t, Bits& b)
{
    const Code lit{t.lit_count, t.lit_sorted, t.lit_fast, LIT_BITS}, dst{t.dist_count, t.dist_sorted, t.dist_fast, DIST_BITS};
    for (;;) {
        refill(io, b);                                                // >= 57 bits unless the input ends: a symbol takes at most 15 + 5 + 15 + 13
        int sym = decode(b, lit);
        if (sym < 0) return -sym;
        if (sym < 256) { if (!io.put((uint8_t)sym)) return BAD_OUTPUT_SIZE; continue; }
        if (sym == 256) return OK;
        if (sym > 285) return BAD_CODE_LENGTHS;
        uint32_t len, extra;
        if (sym < 265) { len = (uint32_t)sym - 254; extra = 0; }
        else if (sym == 285) { len = 258; extra = 0; }
        else { extra = ((uint32_t)sym - 261) >> 2; len = 3 + ((4 + (((uint32_t)sym - 261) & 3)) << extra); }
        if (b.cnt < extra) return TRUNCATED;
        len += (uint32_t)b.buf & ((1u << extra) - 1);
        drop(b, extra);
        sym = decode(b, dst);
        if (sym < 0) return -sym;
        if (sym > 29) return BAD_CODE_LENGTHS;
        uint32_t dist;
        if (sym < 4) { dist = (uint32_t)sym + 1; extra = 0; }
        else { extra = ((uint32_t)sym >> 1) - 1; dist = 1 + ((2 + ((uint32_t)sym & 1)) << extra); }
        if (b.cnt < extra) return TRUNCATED;
        dist += (uint32_t)b.buf & ((1u << extra) - 1);
        drop(b, extra);
        if (const int rc = io.copy(dist, len)) return rc;
    }
}

// lens[at] = v by one lane (the others read it after the next sync)
template <class IO> TFI_FN void set_len(IO& io, Tables& t, int at, int v) { if (io.lane() == 0) t.lens[at] = (uint8_t)v; }

template <class IO> TFI_FN int fixed_tables(IO& io, Tables& t)
{
    io.sync();
    for (int s = io.lane(); s < N_LIT + 32; s += io.lanes()) t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    if (const int rc = build_code(io, t, LIT, t.lens, N_LIT)) return rc;
    return build_code(io, t, DIST, t.lens + N_LIT, 32);
}

// the order in which a dynamic header gives the code-length code's lengths
TFI_FN int clen_order(int i)
{
    // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15, five bits each
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

template <class IO> TFI_FN int dynamic_tables(IO& io, Tables& t, Bits& b)
{
    refill(io, b);
    if (b.cnt < 14) return TRUNCATED;
    const int nlen = (int)(b.buf & 31) + 257, ndist = (int)((b.buf >> 5) & 31) + 1, nclen = (int)((b.buf >> 10) & 15) + 4;
    drop(b, 14);
    if (nlen > 286 || ndist > 30) return BAD_CODE_LENGTHS;
    io.sync();
    for (int s = io.lane(); s < N_CLEN; s += io.lanes()) t.lens[s] = 0;
    io.sync();
    for (int i = 0; i < nclen; ++i) {
        refill(io, b);
        if (b.cnt < 3) return TRUNCATED;
        set_len(io, t, clen_order(i), (int)(b.buf & 7));
        drop(b, 3);
    }
    if (const int rc = build_code(io, t, CLEN, t.lens, N_CLEN)) return rc;
    const Code cl{t.dist_count, t.dist_sorted, t.dist_fast, CLEN_BITS};
    int at = 0, prev = 0, have_256 = 0;
    while (at < nlen + ndist) {
        refill(io, b);
        const int sym = decode(b, cl);
        if (sym < 0) return -sym;
        int rep, v;
        if (sym < 16) { rep = 1; v = sym; }
        else {
            const uint32_t extra = sym == 16 ? 2 : sym == 17 ? 3 : 7;
            if (sym == 16 && at == 0) return BAD_CODE_LENGTHS;         // nothing to repeat
            if (b.cnt < extra) return TRUNCATED;
            rep = (sym == 18 ? 11 : 3) + (int)((uint32_t)b.buf & ((1u << extra) - 1));
            drop(b, extra);
            v = sym == 16 ? prev : 0;
        }
        if (at + rep > nlen + ndist) return BAD_CODE_LENGTHS;
        if (v && at <= 256 && at + rep > 256) have_256 = 1;
        for (int k = 0; k < rep; ++k) set_len(io, t, at + k, v);
        at += rep; prev = v;
    }
    if (!have_256) return BAD_CODE_LENGTHS;                           // no end-of-block code
    if (const int rc = build_code(io, t, LIT, t.lens, nlen)) return rc;
    return build_code(io, t, DIST, t.lens + nlen, ndist);
}

// One zlib stream of in_len bytes whose output must be `expect` bytes: the status.  What was decoded before a failure has gone to the
// IO (finish() is called on every way out).  Bytes after the trailer are not looked at.
template <class IO> TFI_FN int inflate_body(IO& io, Tables& t, Bits& b)
{
    refill(io, b);
    if (b.cnt < 16) return TRUNCATED;
    const uint32_t cmf = (uint32_t)b.buf & 255, flg = (uint32_t)(b.buf >> 8) & 255;
    drop(b, 16);
    if ((cmf * 256 + flg) % 31) return BAD_HEADER;                    // FCHECK
    if ((cmf & 15) != 8 || (cmf >> 4) > 7) return BAD_HEADER;          // CM, CINFO
    if (flg & 32) return BAD_HEADER;                                  // FDICT: there is no dictionary
    for (;;) {
        refill(io, b);
        if (b.cnt < 3) return TRUNCATED;
        const uint32_t last = (uint32_t)b.buf & 1, type = (uint32_t)(b.buf >> 1) & 3;
        drop(b, 3);
        if (type == 0) {
            drop(b, b.cnt & 7);
            refill(io, b);
            if (b.cnt < 32) return TRUNCATED;
            const uint32_t n = (uint32_t)b.buf & 0xFFFF, nn = (uint32_t)(b.buf >> 16) & 0xFFFF;
            if (n != (~nn & 0xFFFF)) return BAD_STORED_LEN;
            drop(b, 32);
            b.pos -= b.cnt >> 3;                                      // whole bytes the bit buffer had taken already go back
            b.buf = 0; b.cnt = 0;
            if (n > b.len - b.pos) return TRUNCATED;
            if (const int rc = io.stored(b.pos, n)) return rc;
            b.pos += n;
        } else if (type == 3) return BAD_BLOCK_TYPE;
        else {
            if (const int rc = type == 1 ? fixed_tables(io, t) : dynamic_tables(io, t, b)) return rc;
            if (const int rc = inflate_codes(io, t, b)) return rc;
        }
        if (last) return OK;
    }
}

template <class IO> TFI_FN int inflate_zlib(IO& io, Tables& t, uint32_t in_len, uint32_t expect)
{
    Bits b;
    b.len = in_len;
    int rc = inflate_body(io, t, b);
    const uint32_t adler = io.finish();
    if (rc) return rc;
    if (io.produced() != expect) return BAD_OUTPUT_SIZE;
    drop(b, b.cnt & 7);
    refill(io, b);
    if (b.cnt < 32) return TRUNCATED;
    const uint32_t v = (uint32_t)b.buf;                               // the trailer is big-endian
    const uint32_t want = (v & 255) << 24 | ((v >> 8) & 255) << 16 | ((v >> 16) & 255) << 8 | (v >> 24);
    return want == adler ? OK : BAD_CHECKSUM;
}

// The single-lane IO over plain buffers of exact sizes: the host's statement of the device's ring (teeflow_inflate.hip.h).
struct HostIO {
    const uint8_t* in; uint8_t* out; uint32_t cap, n = 0, a = 1, b = 0;
    HostIO(const uint8_t* in_, uint8_t* out_, uint32_t cap_) : in(in_), out(out_), cap(cap_) {}
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() {}
    uint8_t in_byte(uint32_t i) const { return in[i]; }
    uint32_t produced() const { return n; }
    void add(uint8_t v) { out[n++] = v; a += v; if (a >= 65521) a -= 65521; b += a; if (b >= 65521) b -= 65521; }
    bool put(uint8_t v) { if (n >= cap) return false; add(v); return true; }
    int copy(uint32_t dist, uint32_t len)
    {
        if (dist > n) return BAD_DISTANCE;
        if (len > cap - n) return BAD_OUTPUT_SIZE;
        const uint32_t from = n - dist;
        for (uint32_t k = 0; k < len; ++k) add(out[from + (k < dist ? k : k % dist)]);
        return OK;
    }
    int stored(uint32_t pos, uint32_t cnt)
    {
        if (cnt > cap - n) return BAD_OUTPUT_SIZE;
        for (uint32_t k = 0; k < cnt; ++k) add(in[pos + k]);
        return OK;
    }
    uint32_t finish() const { return b << 16 | a; }
};
}  // namespace tfi
