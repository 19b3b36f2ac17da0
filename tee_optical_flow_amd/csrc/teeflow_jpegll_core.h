// JPEG Lossless (ITU-T T.81 Process 14, frame marker SOF3; DICOM transfer syntaxes 1.2.840.10008.1.2.4.70 "first-order prediction",
// SV1, and its parent 1.2.840.10008.1.2.4.57), 8-bit, in plain C++ that compiles for the device (teeflow_jpegll.hip.h: TFJ_FN =
// __device__) and for the host (the header parse of tf_jpegll_decode; tests/csrc/verify_jpegll.cpp under the address and
// undefined-behaviour sanitizers).  It stands on teeflow_jpeg_core.h: the descriptor, find_marks, the Huffman tables, the bit reader,
// decode and receive_extend are that header's, unchanged.  frames.jpegll_decode_frame is the numpy twin.
//
// The Huffman-coded value of a lossless scan is the prediction DIFFERENCE, which does not depend on reconstructed samples, so the decode
// splits in two: decode_diffs (serial, one restart interval at a time) emits differences only, and with selection value 1 (Px = Ra)
// the reconstruction is prefix sums modulo 2^16 -- restore_col down the first column of an interval, then restore_row along every
// row, each row on its own.  A valid stream has exactly one decoding, the encoded array.  What libjpeg or pydicom make of a MALFORMED
// stream is NOT pinned: they mask a sample to its precision where this decoder gives a status.
//
// Accepted: SOF3, precision 8; one component, or three, each sampled 1 x 1 (a lone component's sampling is not looked at); one scan that
// holds every component in the frame's order with Ss (the predictor) = 1, Se = 0, Ah = 0, Al (the point transform) = 0; Huffman tables
// of class 0 with ids 0..3, each component its own if it likes; DRI with RSTn, the interval a positive multiple of W (T.81 B.2.4.4;
// 0: none); every other segment (APPn, COM, DQT, ...) is skipped.  A frame is a full interchange stream from SOI on; EOI is not required.
//
// The descriptor is tfj::Desc read for a scan whose MCU is one sample of every component: mcux = W, mcuy = H, nmcu = H * W, ri in
// samples, bpm = ncomp, td[c] the table of component c, bits / vals [t] table t; h, v, tq, ta and q are not used.
//
// Rules (T.81 Annex H): category SSSS = 0 is the difference 0, 1..15 go through receive_extend, 16 is 32768 with no further bits.  The
// first sample of the scan and of every restart interval is predicted by 128 (2^(P-1)), the rest of the first line of the scan and of
// every interval by Ra (the sample to the left), the first sample of any other line by Rb (the sample above), everything else by Ra.
// Sums are kept modulo 2^16 in full: categories 9..16 decode by the rule, and the range check on the reconstructed sample judges.
//
// Status of a frame (tfj's numbering) -- the first finding of the walk over the marker segments in stream order, then of the data:
//   1 BAD_HEADER   teeflow_jpeg_core.h's header findings (no SOI, no marker where one is due, the frame ends before SOS, a segment
//                  length below 2 or past the frame, a DHT that is cut short, has more than 256 codes or is no prefix code, a DRI whose
//                  length is not 4, an SOS before the frame header or of a wrong length); SOF3 twice, shorter than its components, of
//                  a size other than H x W or with components other than `samples`; a DHT of class 1 (or above) or of an id above 3;
//                  a DRI interval that is no multiple of W; a scan naming a table nobody defined
//   2 NOT_DECODED  any frame marker other than SOF3 (SOF0 included; C8 too), DAC, DNL, DHP, EXP; precision other than 8; SOF3 of 0 lines;
//                  a sampling other than 1 x 1 on three components; Ss other than 1 (0 and 2..7 included); Se, Ah or Al other than 0; a
//                  scan that does not hold every component in order
//   3 BAD_DATA     a bit pattern that is no code; a category above 16; the data of a restart interval ends before its last sample; a
//                  missing, extra or wrongly numbered RSTn; a reconstructed sample outside 0..255
// In a segment the checks run in the order of parse_header's text.  Bytes left after an interval's last sample are ignored.
#pragma once
#include "teeflow_jpeg_core.h"

namespace tfl {
using tfj::OK; using tfj::BAD_HEADER; using tfj::NOT_DECODED; using tfj::BAD_DATA;

// The marker segments of frame [0, len) up to the scan header -> d.  byte(i) is asked only with i < len.  Host only.
template <class Byte>
inline int parse_header(Byte&& byte, uint32_t len, int H, int W, int samples, tfj::Desc* d)
{
    memset(d, 0, sizeof *d);
    bool have_h[4] = {}, sof = false;
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
        if ((m >= 0xC0 && m <= 0xCF && m != 0xC3 && m != 0xC4) || m == 0xDC || m == 0xDE || m == 0xDF) return NOT_DECODED;
        if (m == 0xC3) {
            if (sof || L < 8) return BAD_HEADER;
            const int P = byte(s), Y = byte(s + 1) << 8 | byte(s + 2), X = byte(s + 3) << 8 | byte(s + 4), Nf = byte(s + 5);
            if (P != 8) return NOT_DECODED;
            if (L != 8u + 3u * Nf) return BAD_HEADER;
            if (Y == 0) return NOT_DECODED;
            if (Y != H || X != W || Nf != samples || Nf > 3) return BAD_HEADER;
            for (int c = 0; c < Nf; ++c) {
                cid[c] = byte(s + 6 + 3 * c);
                if (Nf > 1 && byte(s + 7 + 3 * c) != 0x11) return NOT_DECODED;
                d->h[c] = d->v[c] = 1;
            }
            d->ncomp = d->bpm = (uint8_t)Nf; d->hmax = d->vmax = 1;
            d->mcux = (uint16_t)W; d->mcuy = (uint16_t)H;
            d->nmcu = (uint32_t)W * (uint32_t)H;
            sof = true;
        } else if (m == 0xC4) {
            for (uint32_t q = s; q < e;) {
                const int tc = byte(q) >> 4, th = byte(q) & 15;
                if (tc != 0 || th > 3) return BAD_HEADER;
                if (e - q < 17) return BAD_HEADER;
                uint32_t n = 0, code = 0;
                for (int l = 1; l <= 16; ++l) {
                    const uint32_t b = byte(q + l);
                    n += b; code += b;
                    if (code > (1u << l)) return BAD_HEADER;
                    code <<= 1;
                }
                if (n > 256 || e - q - 17 < n) return BAD_HEADER;
                memset(d->vals[th], 0, 256);
                for (int l = 0; l < 16; ++l) d->bits[th][l] = byte(q + 1 + l);
                for (uint32_t k = 0; k < n; ++k) d->vals[th][k] = byte(q + 17 + k);
                have_h[th] = true;
                q += 17 + n;
            }
        } else if (m == 0xDD) {
            if (L != 4) return BAD_HEADER;
            d->ri = (uint32_t)byte(s) << 8 | byte(s + 1);
            if (d->ri % (uint32_t)W) return BAD_HEADER;
        } else if (m == 0xDA) {
            if (!sof || L < 3) return BAD_HEADER;
            const int Ns = byte(s);
            if (L != 6u + 2u * Ns) return BAD_HEADER;
            if (Ns != d->ncomp) return NOT_DECODED;
            for (int c = 0; c < Ns; ++c) {
                const int cs = byte(s + 1 + 2 * c), t = byte(s + 2 + 2 * c);
                if (cs != cid[c]) return NOT_DECODED;
                if ((t >> 4) > 3) return BAD_HEADER;
                d->td[c] = (uint8_t)(t >> 4);
            }
            if (byte(s + 1 + 2 * Ns) != 1 || byte(s + 2 + 2 * Ns) != 0 || byte(s + 3 + 2 * Ns) != 0) return NOT_DECODED;
            for (int c = 0; c < Ns; ++c)
                if (!have_h[d->td[c]]) return BAD_HEADER;
            d->scan_off = e;
            d->nint = d->ri ? (d->nmcu + d->ri - 1) / d->ri : 1;
            return OK;
        }
    }
}

// the rows [*r0, *r1) of restart interval k (k < d.nint): whole rows, the interval being a multiple of W
TFJ_FN void interval_rows(const tfj::Desc& d, uint32_t k, uint32_t* r0, uint32_t* r1)
{
    const uint32_t rows = d.ri ? d.ri / d.mcux : d.mcuy;
    *r0 = k * rows;
    *r1 = *r0 + rows < d.mcuy ? *r0 + rows : d.mcuy;
}

// One difference of a component whose table is t -> 0..65535 (the difference modulo 2^16), or -1: no code, a category above 16, or the
// interval's data has ended.
template <class IO> TFJ_FN int decode_diff(IO& io, tfj::Bits& b, const tfj::Huff& t)
{
    const int s = tfj::decode(io, b, t);
    if (s < 0 || s > 16) return -1;
    const int v = s == 0 ? 0 : (s == 16 ? 32768 : tfj::receive_extend(io, b, s));
    return b.cnt < b.pad ? -1 : (v & 0xFFFF);
}

// ---- the reconstruction: prefix sums modulo 2^16.  col: the first column's differences of one interval's rows in place, `pitch`
// entries apart; row: one row's W entries in place, the first being the sample restore_col left.  These are the serial forms of
// k_jpegll_col and k_jpegll_rows. ----------------------------------------------------------------------------------------------------------
TFJ_FN void restore_col(uint16_t* col, size_t pitch, uint32_t rows)
{
    uint32_t x = 128;
    for (uint32_t r = 0; r < rows; ++r) { x = (x + col[(size_t)r * pitch]) & 0xFFFF; col[(size_t)r * pitch] = (uint16_t)x; }
}
// -> false: a sample outside 0..255 (the row's other samples are still written, modulo 256)
TFJ_FN bool restore_row(const uint16_t* diff, uint32_t W, uint8_t* out, size_t step)
{
    uint32_t x = 0;
    bool ok = true;
    for (uint32_t i = 0; i < W; ++i) {
        x = (x + diff[i]) & 0xFFFF;
        if (x > 255) ok = false;
        out[(size_t)i * step] = (uint8_t)x;
    }
    return ok;
}
}  // namespace tfl
