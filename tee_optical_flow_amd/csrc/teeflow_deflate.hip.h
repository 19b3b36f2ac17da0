// Deflate on the device: the chunks of a study's datasets, each into the zlib stream that zlib writes for it at level 9, byte for byte
// (what `write_direct_chunk` of a gzip-9 dataset takes).  The compressor is teeflow_deflate_core.h, the same text the host test runs
// under the sanitizers; this header is how its three parts are spread over the device, a batch of equal-sized chunks at a time:
//   k_chunk            (array sources) gathers a row-major array of up to 4 dimensions into full chunks, zero-padded at the array's
//                      edge, as HDF5 stores them: the inverse of k_unchunk
//   k_deflate_links    one wave per chunk: the hash-chain links, 64 positions a step.  A lane's predecessor is the nearest lower lane
//                      of the step with its hash, or else the head the earlier steps left; the highest lane of each hash writes the
//                      head.  Heads are read and written with agent-scope atomics, so a step reads what the step before wrote.
//   k_deflate_search   one thread per position of every chunk: tfd::search, the hot path (up to 4096 candidates each)
//   k_deflate_emit     one thread per chunk: tfd::deflate, the parse, the trees and the bits, into the chunk's slot of compressBound bytes
//   k_deflate_offsets  exclusive prefix sum of the streams' lengths, continued from the batches before (one block)
//   k_deflate_pack     the slots' streams end to end into the call's blob
// Scratch per chunk of n bytes: n for the chunk itself, 2 n links, 8 n for the two match tables, 128 KiB of heads, 64 KiB of symbols
// and compressBound(n) for the slot, about 12 n + 192 KiB.  A call works through its chunks in batches whose scratch stays under
// DEFLATE_SCRATCH_CAP = 256 MiB (teeflow_deflate_host.hip.h); a chunk has at most 16 MiB, so one always fits.
//
// Bounds: every kernel indexes a chunk's buffers by c < the batch's chunks and p < n only; the core's own bounds are stated there.
#pragma once
#define TFD_FN __device__ inline
#include "teeflow_deflate_core.h"

// Chunk c = blockIdx.x of the batch, whose first element sits at coord[c][0..3] of the row-major array src of shape[0] x .. x
// shape[3] elements of T: its chunk[0] x .. x chunk[3] elements, row-major, to dst + c * chunk_bytes; 0 outside the array.
template <typename T>
__global__ __launch_bounds__(256) void k_chunk(const T* __restrict__ src, const long long* __restrict__ coord, UnchunkDims d, size_t chunk_bytes,
                                               uint8_t* __restrict__ dst)
{
    const int c = blockIdx.x;
    const long long c0 = coord[4 * c], c1 = coord[4 * c + 1], c2 = coord[4 * c + 2], c3 = coord[4 * c + 3];
    const uint32_t k1 = (uint32_t)d.chunk[1], k2 = (uint32_t)d.chunk[2], k3 = (uint32_t)d.chunk[3];
    const uint32_t elems = (uint32_t)d.chunk[0] * k1 * k2 * k3;            // (the host has checked: a chunk is at most 16 MiB)
    T* out = (T*)(dst + (size_t)c * chunk_bytes);
    for (uint32_t e = blockIdx.y * blockDim.x + threadIdx.x; e < elems; e += gridDim.y * blockDim.x) {
        uint32_t r = e;
        const uint32_t i3 = r % k3; r /= k3;
        const uint32_t i2 = r % k2; r /= k2;
        const uint32_t i1 = r % k1;
        const uint32_t i0 = r / k1;
        const long long g0 = c0 + i0, g1 = c1 + i1, g2 = c2 + i2, g3 = c3 + i3;
        T v = 0;
        if (g0 < d.shape[0] && g1 < d.shape[1] && g2 < d.shape[2] && g3 < d.shape[3]) v = src[((g0 * d.shape[1] + g1) * d.shape[2] + g2) * d.shape[3] + g3];
        out[e] = v;
    }
}

// chunk c = blockIdx.x: in + c * n -> pred + c * n; head + c * HASH_SIZE is its scratch
__global__ __launch_bounds__(64) void k_deflate_links(const uint8_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ head, uint16_t* __restrict__ pred)
{
    const size_t c = blockIdx.x;
    const uint8_t* src = in + c * n;
    uint32_t* hd = head + c * tfd::HASH_SIZE;
    uint16_t* pr = pred + c * n;
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < tfd::HASH_SIZE; i += 64) __hip_atomic_store(hd + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t p = base + lane;
        const bool ins = p < n && n - p >= tfd::MIN_MATCH;                  // zlib inserts no position whose three bytes pass the end
        const uint32_t h = ins ? tfd::hash3(src + p) : tfd::HASH_SIZE + lane;   // (a value no other lane has)
        uint32_t q = ins ? __hip_atomic_load(hd + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        bool later = false;
        for (uint32_t j = 0; j < 64; ++j) {
            const uint32_t hj = __shfl(h, (int)j, 64);
            if (hj == h) { if (j < lane) q = base + j; else if (j > lane) later = true; }
        }
        if (p < n) pr[p] = (uint16_t)(ins && q != 0 && p - q <= tfd::MAX_DIST ? p - q : 0);
        if (ins && !later) __hip_atomic_store(hd + h, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();                                                  // the heads written are what the next step's lanes read
        __syncthreads();
    }
}

// position p = blockIdx.x * 256 + threadIdx.x of chunk c = blockIdx.y -> its two entries
__global__ __launch_bounds__(256) void k_deflate_search(const uint8_t* __restrict__ in, uint32_t n, const uint16_t* __restrict__ pred, tfd::Entry* __restrict__ tab)
{
    const size_t c = blockIdx.y;
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    tfd::Entry e[2];
    tfd::search(in + c * n, n, pred + c * n, p, e);
    tab[2 * (c * n + p)] = e[0];
    tab[2 * (c * n + p) + 1] = e[1];
}

// chunk c = blockIdx.x -> its stream in slot + c * stride (stride >= cap = compressBound(n)), len[c], status[c]
__global__ __launch_bounds__(1) void k_deflate_emit(const uint8_t* __restrict__ in, uint32_t n, const tfd::Entry* __restrict__ tab, uint32_t* __restrict__ syms,
                                                     uint8_t* __restrict__ slot, size_t stride, uint32_t cap, uint32_t* __restrict__ len, int* __restrict__ status)
{
    __shared__ tfd::Work work;                                           // (a block is one thread: the parse and the bits are serial)
    const size_t c = blockIdx.x;
    uint32_t made = 0;
    const int rc = tfd::deflate(in + c * n, n, tab + 2 * c * n, syms + c * tfd::SYM_BUF, work, slot + c * stride, cap, &made);
    len[c] = made; status[c] = rc;
}

// off[i] = *total + len[0] + .. + len[i - 1] for the batch's m streams; *total moves behind the last
__global__ __launch_bounds__(256) void k_deflate_offsets(const uint32_t* __restrict__ len, int m, unsigned long long* __restrict__ off, unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long part[256];
    const int t = threadIdx.x, per = (m + 255) / 256, lo = t * per < m ? t * per : m, hi = lo + per < m ? lo + per : m;
    unsigned long long s = 0;
    for (int i = lo; i < hi; ++i) s += len[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        unsigned long long at = *total;
        for (int k = 0; k < 256; ++k) { const unsigned long long v = part[k]; part[k] = at; at += v; }
        *total = at;
    }
    __syncthreads();
    unsigned long long at = part[t];
    for (int i = lo; i < hi; ++i) { off[i] = at; at += len[i]; }
}

// stream c = blockIdx.x of the batch: slot + c * stride [0, len[c]) -> blob + off[c]; nothing at or behind blob_cap
__global__ __launch_bounds__(256) void k_deflate_pack(const uint8_t* __restrict__ slot, size_t stride, const uint32_t* __restrict__ len,
                                                      const unsigned long long* __restrict__ off, uint8_t* __restrict__ blob, unsigned long long blob_cap)
{
    const size_t c = blockIdx.x;
    const uint32_t n = len[c];
    const unsigned long long o = off[c];
    if (n > stride || o > blob_cap || n > blob_cap - o) return;
    for (uint32_t i = blockIdx.y * 256 + threadIdx.x; i < n; i += gridDim.y * 256) blob[o + i] = slot[c * stride + i];
}
