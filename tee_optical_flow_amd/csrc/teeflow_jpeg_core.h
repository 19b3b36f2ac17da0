// JPEG Baseline (ITU-T T.81 Process 1; DICOM transfer syntax 1.2.840.10008.1.2.4.50), 8-bit, in plain C++ that compiles for the device
// (teeflow_jpeg.hip.h: TFJ_FN = __device__) and for the host (the header parse of tf_jpeg_decode; tests/csrc/verify_jpeg.cpp under the
// address and undefined-behaviour sanitizers): the header parse, the Huffman table build, the bit reader, the block decode, the IDCT,
// the two chroma upsamplers.  The libjpeg colour function is teeflow_ingest_core.h's form YBR_LIBJPEG.  frames.jpeg_decode_frame is the
// numpy twin.
//
// The yardstick is libjpeg-turbo as Pillow drives it (slow-integer IDCT, fancy upsampling), which this arithmetic equals on every valid
// stream; the arithmetic is fixed here, signed 32-bit throughout, computed on uint32_t so that no stream reaches undefined behaviour.
// What libjpeg or pydicom make of a MALFORMED stream is NOT pinned: libjpeg repairs and warns where this decoder gives a status.
//
// Accepted: SOF0, precision 8; one component, or three with sampling (1x1 | 2x1 | 2x2, 1x1, 1x1); one scan that holds every component
// in the frame's order with Ss = 0, Se = 63, Ah = Al = 0; 8-bit quantisation tables 0..3; DC and AC Huffman tables 0..1; DRI with
// RSTn; every other segment (APPn, COM, ...) is skipped.  A frame is a full interchange stream from SOI on; EOI is not required.
//
// Status of a frame -- the first finding of the walk over the marker segments in stream order, then of the entropy data:
//   1 BAD_HEADER   no SOI; a byte that is no marker where one is due; the frame ends before SOS (EOI included); a segment length below 2
//                  or past the frame; SOF0 twice, shorter than its components, of a size other than H x W or with components other
//                  than `samples`; a table id above 3; a DHT of more than 256 codes or of lengths that are no prefix code; a DQT or
//                  DHT cut short; a DRI whose length is not 4; an SOS before SOF0, of a wrong length, or naming a table nobody defined
//   2 NOT_DECODED  SOF1..SOF15 other than DHT, DAC, DNL, DHP, EXP; precision other than 8; SOF0 of 0 lines (DNL); a 16-bit quantisation
//                  table; a Huffman table 2 or 3; any other sampling; a scan that is not the one described above
//   3 BAD_DATA     a bit pattern that is no code; a DC category above 15; an AC symbol (r, 0) with r in 1..14; a coefficient index
//                  past 63 (a ZRL included); a DC value outside int16; the data of a restart interval ends before its last MCU; a
//                  missing, extra or wrongly numbered RSTn
// In a segment the checks run in the order of parse_header's text.  Bytes left after an interval's last MCU are ignored.
//
// The entropy data runs from the scan header's end to the first marker that is no RSTn (or the frame's end); a pair FF 00 is the data
// byte FF, an FF before an FF is fill.  A restart interval is `ri` MCUs; interval k's data ends at RSTm, m = k mod 8, and the DC
// predictors start at 0 in every interval.  find_marks is the serial form of k_jpeg_marks.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#ifndef TFJ_FN
#define TFJ_FN inline
#endif
#ifndef TFJ_UNIFORM                           // a table entry read by every lane of a wave at one address: the device makes it a scalar
#define TFJ_UNIFORM(x) (x)
#endif

namespace tfj {
enum : int { OK = 0, BAD_HEADER = 1, NOT_DECODED = 2, BAD_DATA = 3 };

// What the host's header parse leaves for the kernels: one per frame, fixed size.  Table set t of bits / vals: DC 0, DC 1, AC 0, AC 1.
struct Desc {
    uint32_t scan_off, ri, nmcu, nint;        // the entropy data's first byte; the restart interval in MCUs (0: none); MCUs; intervals
    uint16_t mcux, mcuy;                      // MCUs a row, MCU rows
    uint8_t ncomp, hmax, vmax, bpm;           // components; the first component's sampling; blocks an MCU
    uint8_t h[4], v[4], tq[4], td[4], ta[4];  // per component (a lone component: h = v = 1, its MCU is one block)
    uint32_t reserved;
    uint8_t q[4][64];                         // zig-zag order
    uint8_t bits[4][16];
    uint8_t vals[4][256];
};
static_assert(sizeof(Desc) == 1392 && sizeof(Desc) % 16 == 0, "the descriptor is a column of the per-frame table");

// the MCU-padded size of component c, and its true downsampled size
TFJ_FN int comp_pitch(const Desc& d, int c) { return d.mcux * d.h[c] * 8; }
TFJ_FN int comp_rows(const Desc& d, int c) { return d.mcuy * d.v[c] * 8; }
TFJ_FN int down_size(int n, int s, int smax) { return (n * s + smax - 1) / smax; }

TFJ_FN int zigzag(int k)                      // zig-zag position -> natural position
{
    const uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k];
}

// The marker segments of frame [0, len) up to the scan header -> d.  byte(i) is asked only with i < len.  Host only.
template <class Byte>
inline int parse_header(Byte&& byte, uint32_t len, int H, int W, int samples, Desc* d)
{
    memset(d, 0, sizeof *d);
    bool have_q[4] = {}, have_h[4] = {}, sof = false;
    int cid[4] = {};
    if (len < 2 || byte(0) != 0xFF || byte(1) != 0xD8) return BAD_HEADER;
    uint32_t p = 2;
    for (;;) {
        if (p >= len || byte(p) != 0xFF) return BAD_HEADER;
        while (p < len && byte(p) == 0xFF) ++p;                               // (fill)
        if (p >= len) return BAD_HEADER;
        const int m = byte(p++);
        if (m == 0x00 || m == 0xD9) return BAD_HEADER;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;                  // stand-alone markers
        if (len - p < 2) return BAD_HEADER;
        const uint32_t L = (uint32_t)byte(p) << 8 | byte(p + 1);
        if (L < 2 || L > len - p) return BAD_HEADER;
        const uint32_t s = p + 2, e = p + L;                                  // the segment's parameters
        p = e;
        if ((m >= 0xC1 && m <= 0xCF && m != 0xC4) || m == 0xDC || m == 0xDE || m == 0xDF) return NOT_DECODED;
        if (m == 0xC0) {
            if (sof || L < 8) return BAD_HEADER;
            const int P = byte(s), Y = byte(s + 1) << 8 | byte(s + 2), X = byte(s + 3) << 8 | byte(s + 4), Nf = byte(s + 5);
            if (P != 8) return NOT_DECODED;
            if (L != 8u + 3u * Nf) return BAD_HEADER;
            if (Y == 0) return NOT_DECODED;
            if (Y != H || X != W || Nf != samples || Nf > 3) return BAD_HEADER;
            for (int c = 0; c < Nf; ++c) {
                cid[c] = byte(s + 6 + 3 * c);
                const int hv = byte(s + 7 + 3 * c), tq = byte(s + 8 + 3 * c);
                if (tq > 3) return BAD_HEADER;
                d->h[c] = (uint8_t)(hv >> 4); d->v[c] = (uint8_t)(hv & 15); d->tq[c] = (uint8_t)tq;
            }
            if (Nf == 1) d->h[0] = d->v[0] = 1;
            else {
                const int s0 = d->h[0] << 4 | d->v[0];
                if (d->h[1] != 1 || d->v[1] != 1 || d->h[2] != 1 || d->v[2] != 1 || (s0 != 0x11 && s0 != 0x21 && s0 != 0x22)) return NOT_DECODED;
            }
            d->ncomp = (uint8_t)Nf; d->hmax = d->h[0]; d->vmax = d->v[0];
            d->mcux = (uint16_t)((W + 8 * d->hmax - 1) / (8 * d->hmax)); d->mcuy = (uint16_t)((H + 8 * d->vmax - 1) / (8 * d->vmax));
            d->nmcu = (uint32_t)d->mcux * d->mcuy;
            for (int c = 0; c < Nf; ++c) d->bpm = (uint8_t)(d->bpm + d->h[c] * d->v[c]);
            sof = true;
        } else if (m == 0xDB) {
            for (uint32_t q = s; q < e; q += 65) {
                const int pq = byte(q) >> 4, tq = byte(q) & 15;
                if (tq > 3 || pq > 1) return BAD_HEADER;
                if (pq) return NOT_DECODED;
                if (e - q < 65) return BAD_HEADER;
                for (int k = 0; k < 64; ++k) d->q[tq][k] = byte(q + 1 + k);
                have_q[tq] = true;
            }
        } else if (m == 0xC4) {
            for (uint32_t q = s; q < e;) {
                const int tc = byte(q) >> 4, th = byte(q) & 15;
                if (tc > 1 || th > 3) return BAD_HEADER;
                if (th > 1) return NOT_DECODED;
                if (e - q < 17) return BAD_HEADER;
                uint32_t n = 0, code = 0;
                for (int l = 1; l <= 16; ++l) {
                    const uint32_t b = byte(q + l);
                    n += b; code += b;
                    if (code > (1u << l)) return BAD_HEADER;
                    code <<= 1;
                }
                if (n > 256 || e - q - 17 < n) return BAD_HEADER;
                const int t = tc * 2 + th;
                memset(d->vals[t], 0, 256);
                for (int l = 0; l < 16; ++l) d->bits[t][l] = byte(q + 1 + l);
                for (uint32_t k = 0; k < n; ++k) d->vals[t][k] = byte(q + 17 + k);
                have_h[t] = true;
                q += 17 + n;
            }
        } else if (m == 0xDD) {
            if (L != 4) return BAD_HEADER;
            d->ri = (uint32_t)byte(s) << 8 | byte(s + 1);
        } else if (m == 0xDA) {
            if (!sof || L < 3) return BAD_HEADER;
            const int Ns = byte(s);
            if (L != 6u + 2u * Ns) return BAD_HEADER;
            if (Ns != d->ncomp) return NOT_DECODED;
            for (int c = 0; c < Ns; ++c) {
                const int cs = byte(s + 1 + 2 * c), t = byte(s + 2 + 2 * c);
                if (cs != cid[c]) return NOT_DECODED;
                if ((t >> 4) > 3 || (t & 15) > 3) return BAD_HEADER;
                if ((t >> 4) > 1 || (t & 15) > 1) return NOT_DECODED;
                d->td[c] = (uint8_t)(t >> 4); d->ta[c] = (uint8_t)(t & 15);
            }
            if (byte(s + 1 + 2 * Ns) != 0 || byte(s + 2 + 2 * Ns) != 63 || byte(s + 3 + 2 * Ns) != 0) return NOT_DECODED;
            for (int c = 0; c < Ns; ++c)
                if (!have_q[d->tq[c]] || !have_h[d->td[c]] || !have_h[2 + d->ta[c]]) return BAD_HEADER;
            d->scan_off = e;
            d->nint = d->ri ? (d->nmcu + d->ri - 1) / d->ri : 1;
            return OK;
        }
    }
}

// The entropy data's marks, serially: rst[k] (k < d.nint - 1) gets the position of the FF of RSTk, *scan_end the position of the
// first other marker's FF, or len.  byte(i) is asked only with i < len.
template <class Byte>
TFJ_FN int find_marks(Byte&& byte, uint32_t len, const Desc& d, uint32_t* rst, uint32_t* scan_end)
{
    uint32_t found = 0;
    int rc = OK;
    *scan_end = len;
    for (uint32_t p = d.scan_off; p + 1 < len; ++p) {
        if (byte(p) != 0xFF) continue;
        const uint32_t n = byte(p + 1);
        if (n == 0 || n == 0xFF) continue;                                   // (the pair at p + 1 is looked at in its turn)
        if (n < 0xD0 || n > 0xD7) { *scan_end = p; break; }
        if (found + 1 < d.nint && n == 0xD0 + (found & 7)) rst[found] = p;
        else rc = BAD_DATA;
        ++found;
    }
    return found + 1 == d.nint ? rc : (int)BAD_DATA;
}

// ---- Huffman tables (T.81 Annex C) and decoding (F.2.2) ---------------------------------------------------------------------------------
struct Huff {
    int32_t maxcode[17];                      // [l], l = 1..16: the largest code of l bits, -1 where there is none
    int32_t valoff[17];                       // code c of l bits is vals[valoff[l] + c]
    uint16_t look[256];                       // by the next 8 bits: length << 8 | value of a code of up to 8 bits, 0 for a longer one
    uint8_t vals[256];
};

TFJ_FN void huff_lengths(const uint8_t* bits, Huff& t)
{
    int32_t code = 0, k = 0;
    t.maxcode[0] = -1; t.valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int32_t n = bits[l - 1];
        t.valoff[l] = k - code;
        k += n; code += n;
        t.maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
}

// look[x].  A code not found at the lengths below l is at least the first code of l bits (the codes are canonical), so the index is
// one of the table's values.
TFJ_FN uint16_t huff_look(const Huff& t, int x)
{
    for (int l = 1; l <= 8; ++l) {
        const int32_t c = x >> (8 - l);
        if (c <= t.maxcode[l]) return (uint16_t)(l << 8 | t.vals[(t.valoff[l] + c) & 255]);
    }
    return 0;
}

TFJ_FN void huff_build(const uint8_t* bits, const uint8_t* vals, Huff& t)
{
    huff_lengths(bits, t);
    for (int i = 0; i < 256; ++i) t.vals[i] = vals[i];
    for (int x = 0; x < 256; ++x) t.look[x] = huff_look(t, x);
}

// The bit reader over the data bytes [pos, end) of a restart interval.  IO: uint8_t in_byte(uint32_t i), asked only with pos <= i < end.
// Behind the data's end the reader feeds zero bits and counts them in `pad`: a decode that has used one of them (cnt < pad) has failed.
struct Bits { uint32_t acc, pos, end; int cnt, pad; };

template <class IO> TFJ_FN void refill(IO& io, Bits& b)                       // -> cnt >= 25
{
    while (b.cnt <= 24) {
        uint32_t v = 0;
        bool real = false;
        while (b.pos < b.end) {                                               // (pos moves on in every round)
            const uint32_t c = io.in_byte(b.pos);
            if (c != 0xFF) { v = c; ++b.pos; real = true; break; }
            if (b.pos + 1 >= b.end) { b.pos = b.end; break; }
            const uint32_t n = io.in_byte(b.pos + 1);
            if (n == 0) { v = 0xFF; b.pos += 2; real = true; break; }
            if (n == 0xFF) { ++b.pos; continue; }
            b.pos = b.end;                                                    // (a marker: the interval's bounds leave none inside it)
        }
        if (!real) b.pad += 8;
        if (b.pad > 64) b.pad = 64;
        b.acc = b.acc << 8 | v; b.cnt += 8;
    }
}

template <class IO> TFJ_FN int decode(IO& io, Bits& b, const Huff& t)         // -> the symbol, or -1: no code
{
    refill(io, b);
    const uint32_t e = (uint32_t)TFJ_UNIFORM((int)t.look[(b.acc >> (b.cnt - 8)) & 0xFF]);
    if (e) { b.cnt -= (int)(e >> 8); return (int)(e & 0xFF); }
    for (int l = 9; l <= 16; ++l) {
        const int32_t c = (int32_t)((b.acc >> (b.cnt - l)) & ((1u << l) - 1));
        if (c <= TFJ_UNIFORM(t.maxcode[l])) { b.cnt -= l; return TFJ_UNIFORM((int)t.vals[(TFJ_UNIFORM(t.valoff[l]) + c) & 255]); }
    }
    return -1;
}

// decode for lanes that each read a stream of their own: the same steps with every table entry read per lane (TFJ_UNIFORM would hand
// all lanes the first lane's entry)
template <class IO> TFJ_FN int decode_any(IO& io, Bits& b, const Huff& t)
{
    refill(io, b);
    const uint32_t e = t.look[(b.acc >> (b.cnt - 8)) & 0xFF];
    if (e) { b.cnt -= (int)(e >> 8); return (int)(e & 0xFF); }
    for (int l = 9; l <= 16; ++l) {
        const int32_t c = (int32_t)((b.acc >> (b.cnt - l)) & ((1u << l) - 1));
        if (c <= t.maxcode[l]) { b.cnt -= l; return (int)t.vals[(t.valoff[l] + c) & 255]; }
    }
    return -1;
}

template <class IO> TFJ_FN int receive_extend(IO& io, Bits& b, int s)        // 1 <= s <= 15
{
    refill(io, b);
    b.cnt -= s;
    const int r = (int)((b.acc >> b.cnt) & ((1u << s) - 1));
    return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

// One block: put(n, v) is called for every non-zero quantised coefficient, n its natural position, v in int16; *pred is the
// component's DC predictor.
template <class IO, class Put>
TFJ_FN int decode_block(IO& io, Bits& b, const Huff& dc, const Huff& ac, int* pred, Put&& put)
{
    const int s = decode(io, b, dc);
    if (s < 0 || s > 15) return BAD_DATA;
    if (s) *pred += receive_extend(io, b, s);
    if (b.cnt < b.pad || *pred < -32768 || *pred > 32767) return BAD_DATA;
    if (*pred) put(0, *pred);
    for (int k = 1; k < 64;) {
        const int rs = decode(io, b, ac);
        if (rs < 0) return BAD_DATA;
        const int r = rs >> 4, n = rs & 15;
        if (n == 0) {
            if (r == 0) break;
            if (r != 15) return BAD_DATA;
            k += 16;
            if (k > 64) return BAD_DATA;
            continue;
        }
        k += r;
        if (k > 63) return BAD_DATA;
        put(zigzag(k), receive_extend(io, b, n));
        ++k;
        if (b.cnt < b.pad) return BAD_DATA;
    }
    return b.cnt < b.pad ? (int)BAD_DATA : (int)OK;
}

// block j of an MCU -> its component and the block's place (bx, by) in the component's h x v blocks of the MCU
TFJ_FN void mcu_block(const Desc& d, int j, int* c, int* bx, int* by)
{
    int cc = 0;
    while (cc + 1 < d.ncomp && j >= d.h[cc] * d.v[cc]) { j -= d.h[cc] * d.v[cc]; ++cc; }
    *c = cc; *bx = j % d.h[cc]; *by = j / d.h[cc];
}

// ---- dequantisation and libjpeg's jidctint "islow" IDCT, CONST_BITS 13, PASS1_BITS 2 ---------------------------------------------------
TFJ_FN void idct_1d(const uint32_t* x, uint32_t* o)
{
    uint32_t z1 = (x[2] + x[6]) * 4433u;
    const uint32_t t2 = z1 - x[6] * 15137u, t3 = z1 + x[2] * 6270u;
    const uint32_t t0 = (x[0] + x[4]) << 13, t1 = (x[0] - x[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
    z1 = a0 + a3;
    uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995; z3 = z3 * (uint32_t)-16069 + z5; z4 = z4 * (uint32_t)-3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    o[0] = t10 + a3; o[1] = t11 + a2; o[2] = t12 + a1; o[3] = t13 + a0;
    o[4] = t13 - a0; o[5] = t12 - a1; o[6] = t11 - a2; o[7] = t10 - a3;
}
TFJ_FN uint32_t descale(uint32_t v, int n) { return (uint32_t)((int32_t)(v + (1u << (n - 1))) >> n); }

// coef: 64 quantised coefficients in natural order; q: the table in zig-zag order; out: 8 rows of 8 samples, `pitch` bytes apart
TFJ_FN void idct_block(const int16_t* coef, const uint8_t* q, uint8_t* out, size_t pitch)
{
    uint32_t ws[64], x[8], o[8];
    for (int k = 0; k < 64; ++k) { const int n = zigzag(k); ws[n] = (uint32_t)(int32_t)coef[n] * q[k]; }
    for (int c = 0; c < 8; ++c) {
        for (int i = 0; i < 8; ++i) x[i] = ws[8 * i + c];
        idct_1d(x, o);
        for (int i = 0; i < 8; ++i) ws[8 * i + c] = descale(o[i], 11);
    }
    for (int r = 0; r < 8; ++r) {
        idct_1d(ws + 8 * r, o);
        for (int i = 0; i < 8; ++i) {
            const int32_t v = (int32_t)descale(o[i], 18) + 128;
            out[(size_t)r * pitch + i] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    }
}

// ---- libjpeg's fancy upsampling.  s: a component's plane, `pitch` bytes a row, of wd x hd true samples (down_size); (x, y): the
// output sample.  Neighbours are true samples, never MCU padding. ------------------------------------------------------------------------
TFJ_FN uint8_t up_h2v1(const uint8_t* s, size_t pitch, int wd, int x, int y)
{
    const uint8_t* r = s + (size_t)y * pitch;
    const int i = x >> 1;
    if (x & 1) return (uint8_t)(i + 1 < wd ? (3 * r[i] + r[i + 1] + 2) >> 2 : r[i]);
    return (uint8_t)(i > 0 ? (3 * r[i] + r[i - 1] + 1) >> 2 : r[i]);
}
TFJ_FN uint8_t up_h2v2(const uint8_t* s, size_t pitch, int wd, int hd, int x, int y)
{
    const int yy = y >> 1;
    int yn = (y & 1) ? yy + 1 : yy - 1;
    yn = yn < 0 ? 0 : (yn > hd - 1 ? hd - 1 : yn);
    const uint8_t* r0 = s + (size_t)yy * pitch;
    const uint8_t* r1 = s + (size_t)yn * pitch;
    const int i = x >> 1, t = 3 * r0[i] + r1[i];
    if (wd == 1) return (uint8_t)((4 * t + 8) >> 4);
    if (x & 1) return (uint8_t)(i + 1 < wd ? (3 * t + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4 : (4 * t + 7) >> 4);
    return (uint8_t)(i > 0 ? (3 * t + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4 : (4 * t + 8) >> 4);
}

// sample (x, y) of component c of a frame of H x W, from the frame's component planes (plane c at planes + c * plane_bytes)
TFJ_FN uint8_t frame_sample(const Desc& d, const uint8_t* planes, size_t plane_bytes, int H, int W, int c, int x, int y)
{
    const uint8_t* s = planes + (size_t)c * plane_bytes;
    const size_t pitch = (size_t)comp_pitch(d, c);
    if (d.h[c] == d.hmax && d.v[c] == d.vmax) return s[(size_t)y * pitch + x];
    if (d.vmax == 1) return up_h2v1(s, pitch, down_size(W, 1, 2), x, y);
    return up_h2v2(s, pitch, down_size(W, 1, 2), down_size(H, 1, 2), x, y);
}
}  // namespace tfj
