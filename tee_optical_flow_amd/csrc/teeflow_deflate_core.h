// Deflate of one buffer into the zlib stream that zlib 1.2.11 writes for it at level 9 (memLevel 8, 15 window bits, default strategy,
// all input in one call, Z_FINISH), byte for byte, in plain C++ that compiles for the device (teeflow_deflate.hip.h, TFD_FN =
// __device__) and for the host (tests/csrc/verify_deflate.cpp, under the address and undefined-behaviour sanitizers).  Written for
// this project from RFC 1950 / 1951 and from what zlib's deflate_slow, longest_match and trees.c are documented to do; zlib itself is
// the judge (tests/deflate_cases.py).
//
// The work is cut where it stops being parallel:
//   links(in, n, head, pred)        pred[p]: the distance from p back to the nearest earlier position with the same hash of three
//                                   bytes (0: none within reach).  zlib inserts every position up to n - 3 into its hash chains as it
//                                   passes it, whatever the parse does, so the chains are a function of the data alone.
//   search(in, n, pred, p, e)       longest_match at p, without the parse: e[0] is the nearest longest candidate among the first 1024
//                                   of p's chain, e[1] among the first 4096.  The parse reaches longest_match with a previous length
//                                   that a candidate must beat and that, from 32 on, quarters the chain; those two pairs answer both.
//                                   One independent task per position: the device's hot path.
//   deflate(in, n, tab, ...)        the serial rest, per stream: deflate_slow's lazy parse over the table, a block every 16,383
//                                   symbols, zlib's Huffman trees (heap order, depth tie-break, length-limit repair), the choice of a
//                                   stored, fixed or dynamic block, the bits, the header 78 DA and the Adler-32.
// Positions count from the start of the stream; zlib's window slide is followed only for the two things it decides: whether a block's
// first byte is still in the window (a stored block needs it), and that the position that becomes the window's first is "none" as a
// chain's head from then on (deflate(), nil_head).
//
// Bounds: links and search read in[0, n), pred[0, n); deflate reads tab[0, 2n) and writes syms[0, SYM_BUF), and out only through
// Bits::byte, which refuses what would pass `cap` (status OUTPUT_FULL; nothing is written from then on).  Every loop consumes input,
// walks a chain link (at most 4096 per search) or produces output.
#pragma once
#include <stdint.h>

#ifndef TFD_FN
#define TFD_FN inline
#endif

namespace tfd {
// a stream's status (tf_deflate's status[], include/teeflow.h)
enum : int { OK = 0, OUTPUT_FULL = 1,      // the stream does not fit its slot of bound(n) bytes (zlib's never exceeds it)
             STORED_TOO_LONG = 2 };        // a stored block of more than 65,535 bytes was chosen (zlib cannot write one either)

constexpr uint32_t MIN_MATCH = 3, MAX_MATCH = 258, WSIZE = 32768, MIN_LOOKAHEAD = MAX_MATCH + MIN_MATCH + 1;
constexpr uint32_t MAX_DIST = WSIZE - MIN_LOOKAHEAD;              // 32506
constexpr uint32_t HASH_SIZE = 32768, TOO_FAR = 4096;
constexpr uint32_t CHAIN = 4096, CHAIN_GOOD = 1024, GOOD_MATCH = 32, MAX_LAZY = 258;       // level 9 (nice length 258 = MAX_MATCH)
constexpr uint32_t SYM_BUF = 16384;                               // memLevel 8: a block is flushed at SYM_BUF - 1 symbols
constexpr uint32_t MAX_BYTES = 1u << 30;                          // of one stream's input
constexpr int L_CODES = 286, D_CODES = 30, BL_CODES = 19, HEAP_SIZE = 2 * L_CODES + 1, END_BLOCK = 256;

// compressBound(n) (constexpr: the device's kernels and their host code both call it)
constexpr uint32_t bound(uint32_t n) { return n + (n >> 12) + (n >> 14) + (n >> 25) + 13; }

TFD_FN uint32_t hash3(const uint8_t* b) { return (((uint32_t)b[0] << 10) ^ ((uint32_t)b[1] << 5) ^ b[2]) & (HASH_SIZE - 1); }

struct Entry { uint16_t len, dist; };          // a match of len bytes, dist back; len 0: no candidate

// head: HASH_SIZE words of scratch (any content).  pred[0, n).  Position 0 is zlib's NIL and never a candidate; a link longer than
// MAX_DIST is never followed (the search admits the chain's head up to MAX_DIST back and later links nearer than that), so both are 0.
TFD_FN void links(const uint8_t* in, uint32_t n, uint32_t* head, uint16_t* pred)
{
    for (uint32_t i = 0; i < HASH_SIZE; ++i) head[i] = 0;
    for (uint32_t p = 0; p < n; ++p) {
        uint32_t d = 0;
        if (n - p >= MIN_MATCH) {
            const uint32_t h = hash3(in + p), q = head[h];
            if (q != 0 && p - q <= MAX_DIST) d = p - q;
            head[h] = p;
        }
        pred[p] = (uint16_t)d;
    }
}

// how many bytes at a and b agree, up to lim (a < b, b + lim <= n)
TFD_FN uint32_t agree(const uint8_t* in, uint32_t a, uint32_t b, uint32_t lim)
{
    uint32_t k = 0;
    for (; k + 8 <= lim; k += 8) {                               // eight bytes at a time (both machines are little-endian)
        uint64_t x, y;
        __builtin_memcpy(&x, in + a + k, 8); __builtin_memcpy(&y, in + b + k, 8);
        if (x != y) return k + ((uint32_t)__builtin_ctzll(x ^ y) >> 3);
    }
    while (k < lim && in[a + k] == in[b + k]) ++k;
    return k;
}

TFD_FN void search(const uint8_t* in, uint32_t n, const uint16_t* pred, uint32_t p, Entry* e)
{
    e[0] = e[1] = Entry{0, 0};
    const uint32_t lim = n - p < MAX_MATCH ? n - p : MAX_MATCH;
    uint32_t d = pred[p], best = 0, best_dist = 0;
    if (!d) return;
    uint32_t cand = p - d;
    bool past_good = false;
    for (uint32_t k = 0; k < CHAIN; ++k) {
        if (k == CHAIN_GOOD) { e[0] = Entry{(uint16_t)best, (uint16_t)best_dist}; past_good = true; }
        if (in[cand + best] == in[p + best]) {                   // (best < lim) only then can the candidate be longer
            const uint32_t len = agree(in, cand, p, lim);
            if (len > best) { best = len; best_dist = p - cand; }
        }
        if (best >= lim) break;                                  // nothing later is longer
        d = pred[cand];
        if (!d) break;
        cand -= d;
        if (p - cand >= MAX_DIST) break;                         // a link is followed only while it lands above strstart - MAX_DIST
    }
    e[1] = Entry{(uint16_t)best, (uint16_t)best_dist};
    if (!past_good) e[0] = e[1];
}

// ---- the bits ---------------------------------------------------------------------------------------------------------------------------
struct Bits {
    uint8_t* out; uint32_t cap, pos = 0; uint64_t buf = 0; uint32_t cnt = 0; int status = OK;
};
TFD_FN void byte(Bits& w, uint32_t v)
{
    if (w.status) return;
    if (w.pos >= w.cap) { w.status = OUTPUT_FULL; return; }
    w.out[w.pos++] = (uint8_t)v;
}
TFD_FN void send(Bits& w, uint32_t v, uint32_t n)                 // n <= 16 bits of v, the lowest first
{
    w.buf |= (uint64_t)v << w.cnt; w.cnt += n;
    while (w.cnt >= 8) { byte(w, (uint32_t)w.buf & 255); w.buf >>= 8; w.cnt -= 8; }
}
TFD_FN void windup(Bits& w) { if (w.cnt) { byte(w, (uint32_t)w.buf & 255); w.buf = 0; w.cnt = 0; } }

// ---- the trees (zlib's trees.c) ------------------------------------------------------------------------------------------------------
enum Kind { LIT, DIST, BL };
struct Tree { uint16_t* freq; uint16_t* code; uint8_t* len; int kind, elems, max_length, max_code; };

struct Work {
    uint16_t lfreq[HEAP_SIZE], dfreq[2 * D_CODES + 1], bfreq[2 * BL_CODES + 1];
    uint16_t lcode[L_CODES], dcode[D_CODES], bcode[BL_CODES];
    uint8_t llen[HEAP_SIZE], dlen[2 * D_CODES + 1], blen[2 * BL_CODES + 1];
    uint16_t dad[HEAP_SIZE], bl_count[16];
    int16_t heap[HEAP_SIZE];
    uint8_t depth[HEAP_SIZE];
    uint32_t opt_len, static_len, nsym;
};

TFD_FN int extra_lbits(int code) { return code < 8 || code == 28 ? 0 : (code - 4) >> 2; }
TFD_FN int extra_dbits(int code) { return code < 4 ? 0 : (code >> 1) - 1; }
TFD_FN int extra_bits(int kind, int n)
{
    if (kind == LIT) return n > END_BLOCK ? extra_lbits(n - END_BLOCK - 1) : 0;
    if (kind == DIST) return extra_dbits(n);
    return n == 16 ? 2 : n == 17 ? 3 : n == 18 ? 7 : 0;
}
TFD_FN int static_len_of(int kind, int n) { return kind == DIST ? 5 : n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : 8; }
TFD_FN int bl_order(int i)
{
    constexpr uint8_t order[BL_CODES] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}
// length - 3 -> its code (0..28); distance - 1 -> its code (0..29)
TFD_FN int length_code(uint32_t lc)
{
    if (lc < 8) return (int)lc;
    if (lc == 255) return 28;
    int msb = 3;
    while ((lc >> (msb + 1)) != 0) ++msb;
    const int extra = msb - 2;
    return 4 * extra + 4 + (int)((lc >> extra) & 3);
}
TFD_FN int dist_code(uint32_t d)
{
    if (d < 4) return (int)d;
    int msb = 2;
    while ((d >> (msb + 1)) != 0) ++msb;
    return 2 * msb + (int)((d >> (msb - 1)) & 1);
}
TFD_FN uint32_t reverse(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}

TFD_FN bool smaller(const Tree& t, const Work& w, int n, int m)
{
    return t.freq[n] < t.freq[m] || (t.freq[n] == t.freq[m] && w.depth[n] <= w.depth[m]);
}
TFD_FN void down_heap(const Tree& t, Work& w, int heap_len, int k)
{
    const int v = w.heap[k];
    int j = k << 1;
    while (j <= heap_len) {
        if (j < heap_len && smaller(t, w, w.heap[j + 1], w.heap[j])) ++j;
        if (smaller(t, w, v, w.heap[j])) break;
        w.heap[k] = w.heap[j]; k = j; j <<= 1;
    }
    w.heap[k] = (int16_t)v;
}

// the code lengths of a tree from its frequencies, limited to max_length as zlib repairs them, and opt_len / static_len
TFD_FN void gen_bitlen(Tree& t, Work& w, int heap_max)
{
    for (int b = 0; b < 16; ++b) w.bl_count[b] = 0;
    int overflow = 0, h;
    t.len[w.heap[heap_max]] = 0;                                 // the root
    for (h = heap_max + 1; h < HEAP_SIZE; ++h) {
        const int n = w.heap[h];
        int bits = t.len[w.dad[n]] + 1;
        if (bits > t.max_length) { bits = t.max_length; ++overflow; }
        t.len[n] = (uint8_t)bits;
        if (n > t.max_code) continue;                            // not a leaf
        ++w.bl_count[bits];
        const uint32_t x = (uint32_t)extra_bits(t.kind, n), f = t.freq[n];
        w.opt_len += f * ((uint32_t)bits + x);
        if (t.kind != BL) w.static_len += f * ((uint32_t)static_len_of(t.kind, n) + x);
    }
    if (overflow == 0) return;
    do {
        int bits = t.max_length - 1;
        while (w.bl_count[bits] == 0) --bits;
        --w.bl_count[bits];
        w.bl_count[bits + 1] = (uint16_t)(w.bl_count[bits + 1] + 2);
        --w.bl_count[t.max_length];
        overflow -= 2;
    } while (overflow > 0);
    for (int bits = t.max_length; bits != 0; --bits) {
        int n = w.bl_count[bits];
        while (n != 0 && h > heap_max) {                         // (h > heap_max always holds: the lengths' counts sum to the leaves)
            const int m = w.heap[--h];
            if (m > t.max_code) continue;
            if (t.len[m] != bits) {
                w.opt_len += ((uint32_t)bits - (uint32_t)t.len[m]) * (uint32_t)t.freq[m];
                t.len[m] = (uint8_t)bits;
            }
            --n;
        }
    }
}

TFD_FN void build_tree(Tree& t, Work& w)
{
    int heap_len = 0, heap_max = HEAP_SIZE, max_code = -1;
    for (int n = 0; n < t.elems; ++n) {
        if (t.freq[n] != 0) { w.heap[++heap_len] = (int16_t)(max_code = n); w.depth[n] = 0; }
        else t.len[n] = 0;
    }
    while (heap_len < 2) {                                       // at least two codes, so that the tree has a root
        const int node = w.heap[++heap_len] = (int16_t)(max_code < 2 ? ++max_code : 0);
        t.freq[node] = 1; w.depth[node] = 0; --w.opt_len;
        if (t.kind != BL) w.static_len -= (uint32_t)static_len_of(t.kind, node);
    }
    t.max_code = max_code;
    for (int n = heap_len / 2; n >= 1; --n) down_heap(t, w, heap_len, n);
    int node = t.elems;
    do {
        const int n = w.heap[1];
        w.heap[1] = w.heap[heap_len--];
        down_heap(t, w, heap_len, 1);
        const int m = w.heap[1];
        w.heap[--heap_max] = (int16_t)n; w.heap[--heap_max] = (int16_t)m;
        t.freq[node] = (uint16_t)(t.freq[n] + t.freq[m]);
        w.depth[node] = (uint8_t)((w.depth[n] >= w.depth[m] ? w.depth[n] : w.depth[m]) + 1);
        w.dad[n] = w.dad[m] = (uint16_t)node;
        w.heap[1] = (int16_t)node++;
        down_heap(t, w, heap_len, 1);
    } while (heap_len >= 2);
    w.heap[--heap_max] = w.heap[1];
    gen_bitlen(t, w, heap_max);
    uint32_t next[16], code = 0;                                 // the codes: canonical, stored reversed
    next[0] = 0;
    for (int b = 1; b < 16; ++b) next[b] = code = (code + w.bl_count[b - 1]) << 1;
    for (int n = 0; n <= max_code; ++n) {
        const int l = t.len[n];
        if (l) t.code[n] = (uint16_t)reverse(next[l]++, l);
    }
}

// the run-length coding of a tree's code lengths: counted into the code-length tree's frequencies (w = null) or sent
TFD_FN void code_lengths(const Tree& t, Work& wk, Bits* w)
{
    int prevlen = -1, nextlen = t.len[0], count = 0, max_count = 7, min_count = 4;
    if (nextlen == 0) { max_count = 138; min_count = 3; }
    auto put = [&](int sym) { if (w) send(*w, wk.bcode[sym], wk.blen[sym]); else ++wk.bfreq[sym]; };
    for (int n = 0; n <= t.max_code; ++n) {
        const int curlen = nextlen;
        nextlen = n + 1 > t.max_code ? 0xFFFF : t.len[n + 1];
        if (++count < max_count && curlen == nextlen) continue;
        if (count < min_count) { do put(curlen); while (--count != 0); }
        else if (curlen != 0) {
            if (curlen != prevlen) { put(curlen); --count; }
            put(16); if (w) send(*w, (uint32_t)count - 3, 2);
        } else if (count <= 10) { put(17); if (w) send(*w, (uint32_t)count - 3, 3); }
        else { put(18); if (w) send(*w, (uint32_t)count - 11, 7); }
        count = 0; prevlen = curlen;
        if (nextlen == 0) { max_count = 138; min_count = 3; }
        else if (curlen == nextlen) { max_count = 6; min_count = 3; }
        else { max_count = 7; min_count = 4; }
    }
}

TFD_FN void init_block(Work& w)
{
    for (int i = 0; i < HEAP_SIZE; ++i) w.lfreq[i] = 0;
    for (int i = 0; i < 2 * D_CODES + 1; ++i) w.dfreq[i] = 0;
    for (int i = 0; i < 2 * BL_CODES + 1; ++i) w.bfreq[i] = 0;
    w.lfreq[END_BLOCK] = 1;
    w.opt_len = w.static_len = 0; w.nsym = 0;
}

// one symbol (dist 0: the literal lc; else a match of lc + 3 bytes, dist back) into the block; true: the block is full
TFD_FN bool tally(Work& w, uint32_t* syms, uint32_t dist, uint32_t lc)
{
    syms[w.nsym++] = dist << 16 | lc;
    if (dist == 0) ++w.lfreq[lc];
    else { ++w.lfreq[length_code(lc) + END_BLOCK + 1]; ++w.dfreq[dist_code(dist - 1)]; }
    return w.nsym == SYM_BUF - 1;
}

TFD_FN void send_symbols(Bits& b, const uint32_t* syms, uint32_t nsym, const uint16_t* lcode, const uint8_t* llen, const uint16_t* dcode, const uint8_t* dlen,
                         bool fixed)
{
    auto lit = [&](int s) { if (fixed) send(b, reverse((uint32_t)(s < 144 ? 0x30 + s : s < 256 ? 0x190 + s - 144 : s < 280 ? s - 256 : 0xC0 + s - 280), static_len_of(LIT, s)), (uint32_t)static_len_of(LIT, s));
                            else send(b, lcode[s], llen[s]); };
    for (uint32_t i = 0; i < nsym; ++i) {
        const uint32_t dist = syms[i] >> 16, lc = syms[i] & 0xFFFF;
        if (dist == 0) { lit((int)lc); continue; }
        const int lcd = length_code(lc), lx = extra_lbits(lcd);
        lit(lcd + END_BLOCK + 1);
        if (lx) send(b, lc & ((1u << lx) - 1), (uint32_t)lx);   // (a length code's base is a multiple of its extra bits' range)
        const uint32_t d = dist - 1;
        const int dc = dist_code(d), dx = extra_dbits(dc);
        if (fixed) send(b, reverse((uint32_t)dc, 5), 5); else send(b, dcode[dc], dlen[dc]);
        if (dx) send(b, d & ((1u << dx) - 1), (uint32_t)dx);
    }
    lit(END_BLOCK);
}

// the block's symbols out: stored (its bytes in[from, from + stored_len), if `can_store`), fixed or dynamic, as zlib chooses
TFD_FN void flush_block(Work& w, Bits& b, const uint32_t* syms, const uint8_t* in, uint32_t from, uint32_t stored_len, bool can_store, bool last)
{
    Tree lt{w.lfreq, w.lcode, w.llen, LIT, L_CODES, 15, 0}, dt{w.dfreq, w.dcode, w.dlen, DIST, D_CODES, 15, 0}, bt{w.bfreq, w.bcode, w.blen, BL, BL_CODES, 7, 0};
    build_tree(lt, w);
    build_tree(dt, w);
    code_lengths(lt, w, nullptr);
    code_lengths(dt, w, nullptr);
    build_tree(bt, w);
    int max_blindex = BL_CODES - 1;
    for (; max_blindex >= 3; --max_blindex) if (w.blen[bl_order(max_blindex)] != 0) break;
    w.opt_len += 3 * ((uint32_t)max_blindex + 1) + 5 + 5 + 4;
    uint32_t opt_lenb = (w.opt_len + 3 + 7) >> 3;
    const uint32_t static_lenb = (w.static_len + 3 + 7) >> 3;
    if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
    if (stored_len + 4 <= opt_lenb && can_store) {
        if (stored_len > 0xFFFF) { if (!b.status) b.status = STORED_TOO_LONG; }
        else {
            send(b, last ? 1 : 0, 3);
            windup(b);
            byte(b, stored_len & 255); byte(b, stored_len >> 8); byte(b, ~stored_len & 255); byte(b, (~stored_len >> 8) & 255);
            for (uint32_t k = 0; k < stored_len; ++k) byte(b, in[from + k]);
        }
    } else if (static_lenb == opt_lenb) {
        send(b, 2 + (last ? 1 : 0), 3);
        send_symbols(b, syms, w.nsym, nullptr, nullptr, nullptr, nullptr, true);
    } else {
        send(b, 4 + (last ? 1 : 0), 3);
        send(b, (uint32_t)lt.max_code + 1 - 257, 5); send(b, (uint32_t)dt.max_code, 5); send(b, (uint32_t)max_blindex + 1 - 4, 4);
        for (int r = 0; r <= max_blindex; ++r) send(b, w.blen[bl_order(r)], 3);
        code_lengths(lt, w, &b);
        code_lengths(dt, w, &b);
        send_symbols(b, syms, w.nsym, w.lcode, w.llen, w.dcode, w.dlen, false);
    }
    init_block(w);
    if (last) windup(b);
}

// in[0, n) -> its zlib stream in out[0, *out_len), *out_len <= cap: the status.  tab: search()'s two entries of every position.
// syms: SYM_BUF words of scratch.  (On the device one lane runs this.)
TFD_FN int deflate(const uint8_t* in, uint32_t n, const Entry* tab, uint32_t* syms, Work& w, uint8_t* out, uint32_t cap, uint32_t* out_len)
{
    Bits b;
    b.out = out; b.cap = cap;
    byte(b, 0x78); byte(b, 0xDA);
    init_block(w);
    uint32_t p = 0, match_length = MIN_MATCH - 1, match_dist = 0, base = 0, filled = n < 2 * WSIZE ? n : 2 * WSIZE;
    uint32_t block_start = 0;                                    // (absolute, like every position here; zlib's is block_start - base)
    bool match_available = false;
    for (;;) {
        if (filled - p < MIN_LOOKAHEAD) {                        // zlib's fill_window: the slide, then as much input as the window takes
            if (p - base >= WSIZE + MAX_DIST) base += WSIZE;
            filled = n - base < 2 * WSIZE ? n : base + 2 * WSIZE;
            if (filled == p) break;
        }
        const uint32_t prev_length = match_length, prev_dist = match_dist;
        match_length = MIN_MATCH - 1;
        if (n - p >= MIN_MATCH && prev_length < MAX_LAZY) {
            const Entry e = tab[2 * (size_t)p + (prev_length >= GOOD_MATCH ? 0 : 1)];
            // The position a slide made the window's first is zlib's NIL from then on.  It is at least MAX_DIST back when the window
            // slides and p only grows, so it can be a candidate only as the chain's head, at exactly MAX_DIST, in the very step that
            // slid -- which happens where the input ends within MIN_LOOKAHEAD behind p.  A later link must be nearer than MAX_DIST, so
            // that head is then the only candidate and zlib does not search at all.
            const bool nil_head = base > 0 && p - base == MAX_DIST && e.dist == MAX_DIST;
            if (e.len > prev_length && !(e.len == MIN_MATCH && e.dist > TOO_FAR) && !nil_head) { match_length = e.len; match_dist = e.dist; }
        }
        if (prev_length >= MIN_MATCH && match_length <= prev_length) {
            const bool full = tally(w, syms, prev_dist, prev_length - MIN_MATCH);
            p += prev_length - 1;
            match_available = false; match_length = MIN_MATCH - 1;
            if (full) { flush_block(w, b, syms, in, block_start, p - block_start, block_start >= base, false); block_start = p; }
        } else if (match_available) {
            if (tally(w, syms, 0, in[p - 1])) { flush_block(w, b, syms, in, block_start, p - block_start, block_start >= base, false); block_start = p; }
            ++p;
        } else { match_available = true; ++p; }
    }
    if (match_available) (void)tally(w, syms, 0, in[p - 1]);
    flush_block(w, b, syms, in, block_start, p - block_start, block_start >= base, true);
    uint32_t s1 = 1, s2 = 0;                                     // Adler-32
    for (uint32_t at = 0; at < n;) {
        const uint32_t stop = n - at < 5552 ? n : at + 5552;      // as many bytes as the sums take before they must be reduced
        for (; at < stop; ++at) { s1 += in[at]; s2 += s1; }
        s1 %= 65521u; s2 %= 65521u;
    }
    byte(b, s2 >> 8); byte(b, s2 & 255); byte(b, s1 >> 8); byte(b, s1 & 255);
    *out_len = b.pos;
    return b.status;
}
}  // namespace tfd
