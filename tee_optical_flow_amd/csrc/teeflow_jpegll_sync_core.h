// Decoding one restart interval's Huffman data from many places at once, in plain C++ that compiles for the device
// (teeflow_jpegll.hip.h) and for the host (tests/csrc/verify_jpegll_sync.cpp under the address and undefined-behaviour sanitizers).
// Huffman streams self-synchronise (Klein and Wiseman; Weissenberger and Schmidt for the GPU form): the interval's bytes [pos, end)
// are cut into pieces of SEG bytes, every piece is decoded from a guessed start, and then every piece is handed the exit of the piece
// before it, round after round, until a round changes nothing.
//
// State.  A symbol boundary is the CANONICAL position of the next unconsumed data bit: (p, k), p the frame offset of the first stream
// byte of the data byte that holds the bit -- never the 00 of a pair FF 00, never a fill FF, `end` when no data byte is left -- and k
// its bit in that byte, 0 the most significant.  Two readers that stand at the same bit compare equal whatever they have prefetched,
// because the position is carried beside the bit reader and moved on by the bits a symbol used, not derived from the reader.  A
// `phase` (which symbol function comes next; for the lossless scan the component) is part of the state only where the caller says the
// symbol functions differ (nphase > 1).  A state is one uint32_t, (p << 3 | k) << 2 | phase, so a frame must be shorter than MAX_LEN;
// FAILED (phase 3 is never a phase) is the exit of a piece whose decode found no code, a bad symbol or the data's end.
//
// Why the fixed point is the serial decode.  run_piece is a pure function of (entry state, stream): the reader it builds at (p, k) sees
// the bits the serial reader sees from that bit on, zero bits behind `end` included, and a symbol fails exactly where the serial
// decoder's fails (a used pad bit: cnt < pad).  Piece 0 starts from the interval's true start.  When a round has changed no piece,
// every piece's entry is the exit its predecessor decoded from its own entry; by induction from piece 0 every entry is the serial
// decoder's state at that point, and the symbols that START in a piece (p below the piece's end) are the serial decoder's, each in
// exactly one piece.  A wrong guess -- the 00 of a pair, the middle of a symbol -- is merely a wrong entry: it is decoded as data and
// replaced when the truth arrives.  Periodic data need not synchronise at all (the truth then moves one block of pieces a round: inside
// a block of BLOCK piece slots the caller hands exits on between barriers), so the caller caps the rounds and decodes what has not
// converged serially.
//
// Safety: every stream byte is asked through IO with pos <= i < end (the bit reader's contract, teeflow_jpeg_core.h; next_data and
// step check p < end and p + 1 < end before they ask).  Loops: next_data moves p on in every turn and ends at `end`; run_piece's loop
// decodes one symbol a turn, a symbol uses at least one bit or fails, and a position never moves back, so a piece of SEG bytes ends
// after at most 8 * SEG symbols.
#pragma once
#include "teeflow_jpegll_core.h"

namespace tfsync {
constexpr uint32_t SEG = 32;                  // bytes a piece; a symbol is at most 31 bits, so every piece holds a symbol start
constexpr uint32_t BLOCK = 256;                // piece slots a thread block: inside it exits are handed on between barriers, within one round
constexpr uint32_t FAILED = 0xFFFFFFFFu;
constexpr uint32_t IDLE = 0xFFFFFFFFu;        // a piece slot that no interval owns
constexpr uint32_t MAX_LEN = 1u << 27;        // a state holds a byte offset in 27 bits

TFJ_FN uint32_t make_state(uint32_t p, uint32_t k, uint32_t phase) { return ((p << 3 | k) << 2) | phase; }
TFJ_FN uint32_t state_byte(uint32_t s) { return s >> 5; }
TFJ_FN uint32_t state_bit(uint32_t s) { return (s >> 2) & 7; }
TFJ_FN uint32_t state_phase(uint32_t s) { return s & 3; }

// the pieces of the interval [pos, end): at least one, so that an interval without data has a piece that finds that out
TFJ_FN uint32_t piece_count(uint32_t pos, uint32_t end) { return end > pos ? (end - pos + SEG - 1) / SEG : 1; }
// The first slot of interval k's pieces among its frame's slots: intervals are two bytes or more apart, so the slots of interval
// k + 1 start behind those of interval k, and all of them lie below slot_count().
TFJ_FN uint32_t first_slot(uint32_t scan_off, uint32_t pos, uint32_t k) { return (pos - scan_off) / SEG + k; }
// (host only, as same_tables below: the host sizes the slots and marks the frames)
inline uint32_t slot_count(uint32_t len, uint32_t scan_off, uint32_t nint) { return (len - scan_off) / SEG + nint + 1; }

// the first data byte at or behind p, as the bit reader's refill finds it: a pair FF 00 is the data byte FF, an FF before an FF is
// fill, an FF before anything else (or at the very end) ends the data
template <class IO> TFJ_FN uint32_t next_data(IO& io, uint32_t p, uint32_t end)
{
    while (p < end) {
        if (io.in_byte(p) != 0xFF) return p;
        if (p + 1 >= end) return end;
        const uint32_t n = io.in_byte(p + 1);
        if (n == 0) return p;
        if (n != 0xFF) return end;
        ++p;
    }
    return end;
}

// the data byte behind the one that starts at p (p < end)
template <class IO> TFJ_FN uint32_t step(IO& io, uint32_t p, uint32_t end)
{
    p += io.in_byte(p) == 0xFF ? 2u : 1u;
    return p < end ? next_data(io, p, end) : end;
}

// where piece i of the interval [pos, end) starts decoding before anybody knows better: piece 0 at the truth, every other at its first bit
template <class IO> TFJ_FN uint32_t guess(IO& io, uint32_t pos, uint32_t end, uint32_t i)
{
    const uint32_t p = pos + i * SEG;
    return make_state(p < end ? next_data(io, p, end) : end, 0, 0);
}

struct Exit { uint32_t state, count; };       // where the decode stood when it left the piece (or FAILED); the symbols that started in it

// Decode from `entry` the symbols that start below byte `stop` (the piece's end, <= end), at most `limit` of them.
// sym(io, bits, phase, &used) -> the symbol's value (>= 0; `used` gets the bits it took, >= 1) or -1; put(n, phase, value) takes the
// n-th symbol of this call.  nphase: 1 where the symbol function does not depend on the phase (the phase then stays 0).
template <class IO, class Sym, class Put>
TFJ_FN Exit run_piece(IO& io, uint32_t entry, uint32_t stop, uint32_t end, uint32_t nphase, const Sym& sym, uint32_t limit, Put&& put)
{
    Exit x{entry, 0};
    if (entry == FAILED) return x;
    uint32_t p = state_byte(entry), k = state_bit(entry), ph = state_phase(entry);
    if (p >= stop) return x;
    tfj::Bits b;
    b.acc = 0; b.cnt = 0; b.pad = 0; b.pos = p; b.end = end;
    if (k) { tfj::refill(io, b); b.cnt -= (int)k; }
    while (p < stop && x.count < limit) {
        int used = 0;
        const int v = sym(io, b, ph, &used);
        if (v < 0 || used < 1) { x.state = FAILED; return x; }
        put(x.count, ph, v);
        ++x.count;
        ph = ph + 1 < nphase ? ph + 1 : 0;
        for (k += (uint32_t)used; k >= 8 && p < end; k -= 8) p = step(io, p, end);
        if (p >= end) { p = end; k = 0; }
    }
    x.state = make_state(p, k, ph);
    return x;
}

// The lossless scan's symbol: one difference of component `phase` (teeflow_jpegll_core.h's decode_diff with the lane-divergent table
// reads and the bits counted).  After refill the reader holds 25 bits or more and a code takes 16 at the most, so decode_any fetches
// nothing and the code's length is the difference of cnt; the extra bits are the category.
struct DiffSym {
    const tfj::Huff* t0; const tfj::Huff* t1; const tfj::Huff* t2;   // by phase (selected, not indexed: the struct stays in registers)
    template <class IO> TFJ_FN int operator()(IO& io, tfj::Bits& b, uint32_t phase, int* used) const
    {
        tfj::refill(io, b);
        const int c0 = b.cnt;
        const int s = tfj::decode_any(io, b, phase == 0 ? *t0 : (phase == 1 ? *t1 : *t2));
        if (s < 0 || s > 16) return -1;
        *used = c0 - b.cnt + (s < 16 ? s : 0);
        const int v = s == 0 ? 0 : (s == 16 ? 32768 : tfj::receive_extend(io, b, s));
        return b.cnt < b.pad ? -1 : (v & 0xFFFF);
    }
};

// every component names the same code (compared by bits and vals, not by id): the phase is then no part of the state
inline bool same_tables(const tfj::Desc& d)
{
    for (int c = 1; c < d.ncomp && c < 3; ++c) {
        if (d.td[c] == d.td[0]) continue;
        for (int i = 0; i < 16; ++i) if (d.bits[d.td[c] & 3][i] != d.bits[d.td[0] & 3][i]) return false;
        for (int i = 0; i < 256; ++i) if (d.vals[d.td[c] & 3][i] != d.vals[d.td[0] & 3][i]) return false;
    }
    return true;
}
}  // namespace tfsync
