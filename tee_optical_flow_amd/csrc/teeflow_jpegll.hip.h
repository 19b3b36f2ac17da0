// JPEG Lossless (SOF3, predictor 1) on the device: the kernels behind tf_jpegll_decode and tf_hold_frames_jpegll.  The decoder is
// teeflow_jpegll_core.h, the same text the host test runs under the sanitizers, on top of teeflow_jpeg_core.h; the host has parsed every
// frame's header into a tfj::Desc (read as the core says: an MCU is one sample of every component), so every grid is known before the
// first launch and nothing between the kernels waits for the host.
//   k_jpeg_marks      teeflow_jpeg.hip.h's, unchanged: the RSTn positions and the end of the entropy data, one wave64 per frame
//   k_jpegll_entropy  one wave64 per (frame, restart interval): Huffman decode into 16-bit differences, planar [component][H * W]
//   k_jpegll_spec, k_jpegll_sync, k_jpegll_scan, k_jpegll_emit, k_jpegll_entropy_rest
//                     the split entropy decode, one lane per 32-byte piece of an interval: the same differences into the same scratch
//                     where an interval is long enough to pay for it (described where they stand, below)
//   k_jpegll_col      one wave64 per (frame, component, restart interval): the running sum of column 0 over the interval's rows from
//                     128, in place -- the first entry of every row becomes the row's first sample
//   k_jpegll_rows     one wave64 per (frame, component, row): the running sum along the row, 64 samples a round by a __shfl_up scan
//                     with a carry between rounds, masked to 16 bits, range-checked, written as uint8
// The entropy wave is serial and wave-uniform, as k_jpeg_entropy is: the stream is read through the LDS stage of
// teeflow_wave_stage.hip.h and every table entry is made a scalar with readfirstlane; 64 differences of every component are gathered in
// LDS and leave as one coalesced store.  The reconstruction has no serial dependence between rows: with Px = Ra a row is a prefix sum
// of its own differences once its first sample is known, and the first samples are a prefix sum down column 0.
//
// Per-frame scratch (the host sizes it, teeflow_jpegll_host.hip.h): samples * H * W differences of 2 bytes and H RSTn positions (an
// interval is at least a row, so a frame has at most H of them); the samples, 1 byte each, go straight into the call's output.
//
// Safety (a malformed stream is an expected input): a frame whose status is set is touched by no kernel after the one that set it.  The
// stream is read only through the staged reader, whose safety argument is teeflow_wave_stage.hip.h's, at positions below the frame's
// length.  k_jpeg_marks writes position k only with k < nint - 1 < H.  k_jpegll_entropy writes difference s of component c only for
// sample s of its own interval, s < H * W, c < ncomp = samples (the host's parse_header refuses any other count); k_jpegll_col and
// k_jpegll_rows index by the descriptor, the grid and H, W alone, never by stream data: a difference is a value that is added, not a
// place.  Loop bounds: the entropy loop is the interval's samples, each symbol moves the reader on or fails (teeflow_jpeg_core.h).
//
// The build's assembly for gfx950: k_jpegll_entropy 61 VGPRs and 5024 bytes of LDS, k_jpegll_col 13 VGPRs, k_jpegll_rows 18; private
// segment 0 bytes and no scratch instruction in any of the three.
#pragma once
#include "teeflow_jpeg.hip.h"
#include "teeflow_jpegll_core.h"
#include "teeflow_jpegll_sync_core.h"

namespace jpegll {
// the inclusive scan of x over the wave's lanes, modulo 2^32 (the callers mask to 16 bits)
__device__ inline uint32_t wave_scan(uint32_t x, int ln)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (ln >= o) x += y;
    }
    return x;
}
}  // namespace jpegll

// Block (k, fb): restart interval k of frame f0 + fb; a frame without DRI is one interval.  diff + fb * diff_stride gets the frame's
// differences modulo 2^16, component c's H * W at c * hw.  The first error sets status 3 and ends the wave; a wave of a frame whose
// status is already set returns at once.
__global__ __launch_bounds__(64) void k_jpegll_entropy(const uint8_t* __restrict__ blob, const unsigned long long* __restrict__ off,
                                                      const uint32_t* __restrict__ len, const tfj::Desc* __restrict__ desc, int f0, uint32_t ni_max,
                                                      const uint32_t* __restrict__ rst, const uint32_t* __restrict__ scan_end,
                                                      uint16_t* __restrict__ diff, size_t diff_stride, size_t hw, int* status)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[jpeg::STAGE];
    __shared__ tfj::Huff huff[4];
    __shared__ uint16_t blk[3][64];
    const int fb = (int)blockIdx.y, f = f0 + fb, ln = (int)threadIdx.x;
    const uint32_t k = blockIdx.x;
    const tfj::Desc& d = desc[f];
    if (jpeg::status_of(status, f) != 0 || k >= d.nint) return;
    if (ln < 4) tfj::huff_lengths(d.bits[ln], huff[ln]);
    for (int i = ln; i < 4 * 256; i += 64) huff[i >> 8].vals[i & 255] = d.vals[i >> 8][i & 255];
    __syncthreads();
    for (int i = ln; i < 4 * 256; i += 64) huff[i >> 8].look[i & 255] = tfj::huff_look(huff[i >> 8], i & 255);
    __syncthreads();
    jpeg::WaveIO io;
    jpeg::open_frame(io, stage, blob, off[f], len[f], ln);
    const uint32_t* list = rst + (size_t)f * ni_max;
    tfj::Bits b;
    b.acc = 0; b.cnt = 0; b.pad = 0;
    b.pos = k ? list[k - 1] + 2 : d.scan_off;
    b.end = k + 1 < d.nint ? list[k] : scan_end[f];
    const uint32_t s0 = d.ri ? k * d.ri : 0, s1 = d.ri && s0 + d.ri < d.nmcu ? s0 + d.ri : d.nmcu;
    const int nc = d.ncomp < 3 ? d.ncomp : 3;
    const tfj::Huff* const t0 = &huff[d.td[0] & 3];
    const tfj::Huff* const t1 = &huff[d.td[1] & 3];
    const tfj::Huff* const t2 = &huff[d.td[2] & 3];
    uint16_t* out = diff + (size_t)fb * diff_stride;
    int rc = tfj::OK;
    for (uint32_t base = s0; base < s1; base += 64) {
        const uint32_t n = s1 - base < 64 ? s1 - base : 64;
        for (uint32_t j = 0; j < n && rc == tfj::OK; ++j)
            for (int c = 0; c < nc; ++c) {
                const int v = tfl::decode_diff(io, b, c == 0 ? *t0 : (c == 1 ? *t1 : *t2));
                if (v < 0) { rc = tfj::BAD_DATA; break; }
                blk[c][j] = (uint16_t)v;
            }
        if (rc != tfj::OK) break;
        __syncthreads();
        if ((uint32_t)ln < n)
            for (int c = 0; c < nc; ++c) out[(size_t)c * hw + base + ln] = blk[c][ln];
        __syncthreads();
    }
    if (rc != tfj::OK && ln == 0) atomicMax(&status[f], rc);
}

// k_jpegll_entropy for a batch that holds split frames (below): conv [frames of the batch][ni_max] marks the intervals the split decode
// has served, and their waves return at once; every other interval -- of a frame the host kept on the serial path, or one that did not
// converge -- is decoded as k_jpegll_entropy decodes it.  The text is k_jpegll_entropy's with that one condition more, kept as a copy
// so that the serial kernel's code object stays exactly what it was.
__global__ __launch_bounds__(64) void k_jpegll_entropy_rest(const uint8_t* __restrict__ blob, const unsigned long long* __restrict__ off,
                                                           const uint32_t* __restrict__ len, const tfj::Desc* __restrict__ desc, int f0, uint32_t ni_max,
                                                           const uint32_t* __restrict__ rst, const uint32_t* __restrict__ scan_end,
                                                           uint16_t* __restrict__ diff, size_t diff_stride, size_t hw, int* status,
                                                           const uint32_t* __restrict__ conv)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[jpeg::STAGE];
    __shared__ tfj::Huff huff[4];
    __shared__ uint16_t blk[3][64];
    const int fb = (int)blockIdx.y, f = f0 + fb, ln = (int)threadIdx.x;
    const uint32_t k = blockIdx.x;
    const tfj::Desc& d = desc[f];
    if (jpeg::status_of(status, f) != 0 || k >= d.nint || conv[(size_t)fb * ni_max + k] != 0) return;
    if (ln < 4) tfj::huff_lengths(d.bits[ln], huff[ln]);
    for (int i = ln; i < 4 * 256; i += 64) huff[i >> 8].vals[i & 255] = d.vals[i >> 8][i & 255];
    __syncthreads();
    for (int i = ln; i < 4 * 256; i += 64) huff[i >> 8].look[i & 255] = tfj::huff_look(huff[i >> 8], i & 255);
    __syncthreads();
    jpeg::WaveIO io;
    jpeg::open_frame(io, stage, blob, off[f], len[f], ln);
    const uint32_t* list = rst + (size_t)f * ni_max;
    tfj::Bits b;
    b.acc = 0; b.cnt = 0; b.pad = 0;
    b.pos = k ? list[k - 1] + 2 : d.scan_off;
    b.end = k + 1 < d.nint ? list[k] : scan_end[f];
    const uint32_t s0 = d.ri ? k * d.ri : 0, s1 = d.ri && s0 + d.ri < d.nmcu ? s0 + d.ri : d.nmcu;
    const int nc = d.ncomp < 3 ? d.ncomp : 3;
    const tfj::Huff* const t0 = &huff[d.td[0] & 3];
    const tfj::Huff* const t1 = &huff[d.td[1] & 3];
    const tfj::Huff* const t2 = &huff[d.td[2] & 3];
    uint16_t* out = diff + (size_t)fb * diff_stride;
    int rc = tfj::OK;
    for (uint32_t base = s0; base < s1; base += 64) {
        const uint32_t n = s1 - base < 64 ? s1 - base : 64;
        for (uint32_t j = 0; j < n && rc == tfj::OK; ++j)
            for (int c = 0; c < nc; ++c) {
                const int v = tfl::decode_diff(io, b, c == 0 ? *t0 : (c == 1 ? *t1 : *t2));
                if (v < 0) { rc = tfj::BAD_DATA; break; }
                blk[c][j] = (uint16_t)v;
            }
        if (rc != tfj::OK) break;
        __syncthreads();
        if ((uint32_t)ln < n)
            for (int c = 0; c < nc; ++c) out[(size_t)c * hw + base + ln] = blk[c][ln];
        __syncthreads();
    }
    if (rc != tfj::OK && ln == 0) atomicMax(&status[f], rc);
}

// ---- the split entropy decode (teeflow_jpegll_sync_core.h): one lane per piece of tfsync::SEG bytes, lane-divergent ---------------------------
// A frame the host sent down this path (desc.reserved bit 0; bit 1: the components' tables differ, so the phase is part of a state) has
// `pmax` piece slots in each of the per-piece arrays -- owner (the interval, or IDLE), entry, two exit arrays, cnt -- and ni_max
// entries in the per-interval arrays lastchg (the last round that changed a piece; 0: the speculation, -1: one piece) and conv (0: not
// served here, the serial kernel decodes it; 1: served; 2: served, and its data ends before its last sample).  Slot g of a frame is
// piece g - first_slot(k) of the one interval k whose pieces cover g; a grid is (slots / 256, frames of the batch).
//   k_jpegll_spec   every piece decoded from its guess (piece 0 of an interval from the truth): owner, entry, exit, cnt, lastchg
//   k_jpegll_sync   one round: a piece whose predecessor's exit differs from its entry decodes again from it.  Across blocks a round
//                   reads only the exits the launch before wrote (two arrays); inside a block exits are handed on through LDS in
//                   Jacobi turns between barriers until a turn changes nothing (at most 256: piece j of a block is final after
//                   turn j), so what a round computes does not depend on scheduling.  No block waits for another.
//   k_jpegll_scan   one wave64 per (frame, interval): converged (lastchg < rounds) or not; where converged, the exclusive prefix
//                   sum of cnt in place -- a piece's first symbol index -- and the verdict on the total
//   k_jpegll_emit   every piece of a converged interval decoded once more from its now-true entry: symbol q is the difference of
//                   sample s0 + q / ncomp, component q % ncomp, written only for q below the interval's symbols
// Safety: the stream is read through LaneIO by the core alone, every index below the interval's end, which is clamped to the frame's
// length.  A slot index is g < pmax on top of the frame's pmax slots; an interval index is k < nint <= ni_max.  k_jpegll_scan refuses
// an interval whose pieces would pass pmax (the host sizes pmax so that none does).  k_jpegll_emit writes difference (c, s) only
// with s0 <= s < s1 <= H * W of its own interval: run_piece hands out at most nsym - q0 symbols.  Loops: the interval search halves
// its range; a decode is teeflow_jpegll_sync_core.h's; the turns of k_jpegll_sync are counted to 256; the rounds are the host's.
// A block leaves before a barrier only on conditions every one of its threads sees alike (the status through LDS).
//
// The build's assembly for gfx950: k_jpegll_spec 30 VGPRs and 3620 bytes of LDS, k_jpegll_sync 31 and 5928, k_jpegll_scan 18 and none,
// k_jpegll_emit 28 and 3620, k_jpegll_entropy_rest 61 and 5024; private segment 0 bytes and no scratch instruction in any of the five.
namespace jpegll {
struct LaneIO {
    const uint8_t* p;
    __device__ uint8_t in_byte(uint32_t i) const { return p[i]; }
};

// the frame's tables into LDS by a block of nt threads (the two loops of k_jpegll_entropy)
__device__ inline void load_tables(const tfj::Desc& d, tfj::Huff* huff, int tid, int nt)
{
    if (tid < 4) tfj::huff_lengths(d.bits[tid], huff[tid]);
    for (int i = tid; i < 4 * 256; i += nt) huff[i >> 8].vals[i & 255] = d.vals[i >> 8][i & 255];
    __syncthreads();
    for (int i = tid; i < 4 * 256; i += nt) huff[i >> 8].look[i & 255] = tfj::huff_look(huff[i >> 8], i & 255);
    __syncthreads();
}

// the frame's status as every thread of the block sees it alike (another block may set it meanwhile)
__device__ inline int block_status(const int* status, int f)
{
    __shared__ int st;
    if (threadIdx.x == 0) st = jpeg::status_of(status, f);
    __syncthreads();
    return st;
}

struct Piece { uint32_t pos, end, base, n; };     // interval k's data bytes [pos, end), its first slot and its pieces

__device__ inline Piece interval_pieces(const tfj::Desc& d, const uint32_t* list, uint32_t scan_end, uint32_t len, uint32_t k)
{
    Piece pc;
    pc.pos = k ? list[k - 1] + 2 : d.scan_off;
    pc.end = k + 1 < d.nint ? list[k] : scan_end;
    if (pc.end > len) pc.end = len;
    if (pc.pos > pc.end) pc.pos = pc.end;
    pc.base = pc.pos >= d.scan_off ? tfsync::first_slot(d.scan_off, pc.pos, k) : 0xFFFFFFFFu - 0x10000u;
    pc.n = tfsync::piece_count(pc.pos, pc.end);
    return pc;
}

__device__ inline uint32_t piece_stop(const Piece& pc, uint32_t i)
{
    return pc.end - pc.pos > (i + 1) * tfsync::SEG ? pc.pos + (i + 1) * tfsync::SEG : pc.end;
}
}  // namespace jpegll

#define JPEGLL_SPLIT_ARGS                                                                                                                          \
    const uint8_t *__restrict__ blob, const unsigned long long *__restrict__ off, const uint32_t *__restrict__ len, const tfj::Desc *__restrict__ desc, \
        int f0, uint32_t ni_max, const uint32_t *__restrict__ rst, const uint32_t *__restrict__ scan_end, uint32_t pmax

__global__ __launch_bounds__(256) void k_jpegll_spec(JPEGLL_SPLIT_ARGS, uint32_t* __restrict__ owner, uint32_t* __restrict__ entry, uint32_t* __restrict__ exit0,
                                                    uint32_t* __restrict__ cnt, int* __restrict__ lastchg, const int* status)
{
    __shared__ tfj::Huff huff[4];
    const int fb = (int)blockIdx.y, f = f0 + fb, tid = (int)threadIdx.x;
    const tfj::Desc& d = desc[f];
    if (!(d.reserved & 1) || jpegll::block_status(status, f) != 0) return;
    jpegll::load_tables(d, huff, tid, 256);
    const uint32_t g = blockIdx.x * 256 + (uint32_t)tid;
    if (g >= pmax) return;
    const size_t slot = (size_t)fb * pmax + g;
    const uint32_t* list = rst + (size_t)f * ni_max;
    uint32_t lo = 0, hi = d.nint - 1;                                       // the last interval whose first slot is not behind g
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1, p = list[mid - 1] + 2;
        if (p >= d.scan_off && tfsync::first_slot(d.scan_off, p, mid) <= g) lo = mid; else hi = mid - 1;
    }
    const jpegll::Piece pc = jpegll::interval_pieces(d, list, scan_end[f], len[f], lo);
    const uint32_t i = g - pc.base;
    if (g < pc.base || i >= pc.n) { owner[slot] = tfsync::IDLE; return; }
    jpegll::LaneIO io{blob + off[f]};
    const tfsync::DiffSym sym{&huff[d.td[0] & 3], &huff[d.td[1] & 3], &huff[d.td[2] & 3]};
    const uint32_t e = tfsync::guess(io, pc.pos, pc.end, i);
    const tfsync::Exit x = tfsync::run_piece(io, e, jpegll::piece_stop(pc, i), pc.end, (d.reserved & 2) ? d.ncomp : 1u, sym, 0xFFFFFFFFu, [](uint32_t, uint32_t, int) {});
    owner[slot] = lo; entry[slot] = e; exit0[slot] = x.state; cnt[slot] = x.count;
    if (i == 0) lastchg[(size_t)fb * ni_max + lo] = pc.n > 1 ? 0 : -1;
}

__global__ __launch_bounds__(256) void k_jpegll_sync(JPEGLL_SPLIT_ARGS, const uint32_t* __restrict__ owner, uint32_t* __restrict__ entry,
                                                    const uint32_t* __restrict__ exit_prev, uint32_t* __restrict__ exit_cur, uint32_t* __restrict__ cnt,
                                                    int* __restrict__ lastchg, int round, const int* status)
{
    __shared__ tfj::Huff huff[4];
    __shared__ uint32_t ex[2][256];
    const int fb = (int)blockIdx.y, f = f0 + fb, tid = (int)threadIdx.x;
    const tfj::Desc& d = desc[f];
    if (!(d.reserved & 1) || jpegll::block_status(status, f) != 0) return;
    jpegll::load_tables(d, huff, tid, 256);
    const uint32_t g = blockIdx.x * 256 + (uint32_t)tid;
    const size_t slot = (size_t)fb * pmax + g;
    const uint32_t k = g < pmax ? owner[slot] : tfsync::IDLE;
    const bool live = k != tfsync::IDLE && k < d.nint;
    jpegll::Piece pc = {};
    if (live) pc = jpegll::interval_pieces(d, rst + (size_t)f * ni_max, scan_end[f], len[f], k);
    const uint32_t i = g - pc.base;
    const bool follows = live && i > 0 && i < pc.n;                         // a piece with a predecessor, which is slot g - 1
    uint32_t en = live ? entry[slot] : 0, c = live ? cnt[slot] : 0, mine = live ? exit_prev[slot] : tfsync::FAILED;
    const uint32_t edge = follows && tid == 0 ? exit_prev[slot - 1] : 0;    // across the block's edge: what the launch before wrote
    jpegll::LaneIO io{blob + off[f]};
    const tfsync::DiffSym sym{&huff[d.td[0] & 3], &huff[d.td[1] & 3], &huff[d.td[2] & 3]};
    const uint32_t stop = jpegll::piece_stop(pc, i), nphase = (d.reserved & 2) ? d.ncomp : 1u;
    bool touched = false;
    int cur = 0;
    ex[0][tid] = mine;
    __syncthreads();
    for (int turn = 0; turn < 256; ++turn) {
        bool moved = false;
        if (follows) {
            const uint32_t pred = tid == 0 ? edge : ex[cur][tid - 1];
            if (pred != en) {
                en = pred;
                const tfsync::Exit x = tfsync::run_piece(io, en, stop, pc.end, nphase, sym, 0xFFFFFFFFu, [](uint32_t, uint32_t, int) {});
                mine = x.state; c = x.count;
                moved = touched = true;
            }
        }
        ex[cur ^ 1][tid] = mine;
        if (!__syncthreads_or(moved ? 1 : 0)) break;
        cur ^= 1;
    }
    if (live) {
        exit_cur[slot] = mine;
        if (touched) { entry[slot] = en; cnt[slot] = c; atomicMax(&lastchg[(size_t)fb * ni_max + k], round); }
    }
}

// Block (k, fb).  ctr[0] counts the intervals of split frames that did not converge.
__global__ __launch_bounds__(64) void k_jpegll_scan(const uint32_t* __restrict__ len, const tfj::Desc* __restrict__ desc, int f0, uint32_t ni_max,
                                                   const uint32_t* __restrict__ rst, const uint32_t* __restrict__ scan_end, uint32_t pmax,
                                                   uint32_t* __restrict__ cnt, const int* __restrict__ lastchg, uint32_t* __restrict__ conv, int rounds,
                                                   unsigned int* ctr, const int* status)
{
    const int fb = (int)blockIdx.y, f = f0 + fb, ln = (int)threadIdx.x;
    const uint32_t k = blockIdx.x;
    const tfj::Desc& d = desc[f];
    if (jpeg::status_of(status, f) != 0 || k >= d.nint) return;             // (no kernel sets a status between k_jpeg_marks and k_jpegll_emit)
    const size_t iv = (size_t)fb * ni_max + k;
    if (!(d.reserved & 1)) { if (ln == 0) conv[iv] = 0; return; }
    const jpegll::Piece pc = jpegll::interval_pieces(d, rst + (size_t)f * ni_max, scan_end[f], len[f], k);
    if (lastchg[iv] >= rounds || pc.base > pmax || pc.n > pmax - pc.base) {
        if (ln == 0) { conv[iv] = 0; atomicAdd(&ctr[0], 1u); }
        return;
    }
    uint32_t* mine = cnt + (size_t)fb * pmax + pc.base;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < pc.n; b0 += 256) {                            // four pieces a lane
        const uint32_t j = b0 + 4u * (uint32_t)ln;
        uint32_t v[4], s = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) { v[t] = j + t < pc.n ? mine[j + t] : 0u; s += v[t]; }
        const uint32_t incl = jpegll::wave_scan(s, ln);
        uint32_t x = carry + incl - s;
#pragma unroll
        for (int t = 0; t < 4; ++t) { if (j + t < pc.n) mine[j + t] = x; x += v[t]; }
        carry += (uint32_t)__shfl((int)incl, 63, 64);
    }
    const uint32_t s0 = d.ri ? k * d.ri : 0, s1 = d.ri && s0 + d.ri < d.nmcu ? s0 + d.ri : d.nmcu;
    if (ln == 0) conv[iv] = carry < (s1 - s0) * (uint32_t)d.ncomp ? 2u : 1u;
}

__global__ __launch_bounds__(256) void k_jpegll_emit(JPEGLL_SPLIT_ARGS, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ entry,
                                                    const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ conv, uint16_t* __restrict__ diff,
                                                    size_t diff_stride, size_t hw, int* status)
{
    __shared__ tfj::Huff huff[4];
    const int fb = (int)blockIdx.y, f = f0 + fb, tid = (int)threadIdx.x;
    const tfj::Desc& d = desc[f];
    if (!(d.reserved & 1) || jpegll::block_status(status, f) != 0) return;
    jpegll::load_tables(d, huff, tid, 256);
    const uint32_t g = blockIdx.x * 256 + (uint32_t)tid;
    if (g >= pmax) return;
    const size_t slot = (size_t)fb * pmax + g;
    const uint32_t k = owner[slot];
    if (k == tfsync::IDLE || k >= d.nint) return;
    const uint32_t cv = conv[(size_t)fb * ni_max + k];
    if (cv == 0) return;
    const jpegll::Piece pc = jpegll::interval_pieces(d, rst + (size_t)f * ni_max, scan_end[f], len[f], k);
    const uint32_t i = g - pc.base;
    if (cv == 2) { if (i == 0) atomicMax(&status[f], (int)tfj::BAD_DATA); return; }
    const uint32_t s0 = d.ri ? k * d.ri : 0, s1 = d.ri && s0 + d.ri < d.nmcu ? s0 + d.ri : d.nmcu;
    const uint32_t nc = d.ncomp < 3 ? d.ncomp : 3, nsym = (s1 - s0) * nc, q0 = cnt[slot];
    if (i >= pc.n || q0 >= nsym) return;
    jpegll::LaneIO io{blob + off[f]};
    const tfsync::DiffSym sym{&huff[d.td[0] & 3], &huff[d.td[1] & 3], &huff[d.td[2] & 3]};
    uint16_t* out = diff + (size_t)fb * diff_stride;
    uint32_t s = s0 + q0 / nc, c = q0 % nc;
    tfsync::run_piece(io, entry[slot], jpegll::piece_stop(pc, i), pc.end, (d.reserved & 2) ? d.ncomp : 1u, sym, nsym - q0, [&](uint32_t, uint32_t, int v) {
        out[(size_t)c * hw + s] = (uint16_t)v;
        if (++c == nc) { c = 0; ++s; }
    });
}

// Block (k, c, fb): column 0 of component c over the rows of restart interval k of frame f0 + fb, 64 rows a round.
__global__ __launch_bounds__(64) void k_jpegll_col(const tfj::Desc* __restrict__ desc, int f0, uint16_t* __restrict__ diff, size_t diff_stride, size_t hw,
                                                  const int* status)
{
    const int fb = (int)blockIdx.z, f = f0 + fb, c = (int)blockIdx.y, ln = (int)threadIdx.x;
    const uint32_t k = blockIdx.x;
    const tfj::Desc& d = desc[f];
    if (jpeg::status_of(status, f) != 0 || k >= d.nint || c >= d.ncomp) return;
    uint32_t r0, r1;
    tfl::interval_rows(d, k, &r0, &r1);
    const size_t W = d.mcux;
    uint16_t* col = diff + (size_t)fb * diff_stride + (size_t)c * hw;
    uint32_t carry = 128;
    for (uint32_t base = r0; base < r1; base += 64) {
        const uint32_t r = base + (uint32_t)ln;
        const uint32_t x = carry + jpegll::wave_scan(r < r1 ? col[(size_t)r * W] : 0u, ln);
        if (r < r1) col[(size_t)r * W] = (uint16_t)x;
        carry = (uint32_t)__shfl((int)x, 63, 64) & 0xFFFFu;
    }
}

// Block (y, c, fb): row y of component c of frame f0 + fb.  out is the call's whole output, frame f0 + fb at its own place:
// interleaved [N][H][W][samples], or (planar) [N][samples][H * W], k_ingest_planar's layout.  A sample outside 0..255 sets status 3.
__global__ __launch_bounds__(64) void k_jpegll_rows(int f0, const uint16_t* __restrict__ diff, size_t diff_stride, int samples, int H, int W, int planar,
                                                   uint8_t* __restrict__ out, int* status)
{
    const int fb = (int)blockIdx.z, f = f0 + fb, c = (int)blockIdx.y, y = (int)blockIdx.x, ln = (int)threadIdx.x;
    if (y >= H || c >= samples || jpeg::status_of(status, f) != 0) return;
    const size_t hw = (size_t)H * W, row = (size_t)y * W;
    const uint16_t* in = diff + (size_t)fb * diff_stride + (size_t)c * hw + row;
    uint32_t carry = 0;
    bool bad = false;
    for (int base = 0; base < W; base += 64) {
        const int i = base + ln;
        const uint32_t x = (carry + jpegll::wave_scan(i < W ? in[i] : 0u, ln)) & 0xFFFFu;
        if (i < W) {
            bad |= x > 255;
            if (planar) out[((size_t)f * samples + c) * hw + row + i] = (uint8_t)x;
            else out[((size_t)f * hw + row + i) * samples + c] = (uint8_t)x;
        }
        carry = (uint32_t)__shfl((int)x, 63, 64);
    }
    if (bad) atomicMax(&status[f], (int)tfj::BAD_DATA);
}
