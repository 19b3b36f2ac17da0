// The host side of deflate on the device (kernels: teeflow_deflate.hip.h): tf_deflate, tf_deflate_array, tf_held_deflate.  Included by
// teeflow.hip after teeflow_inflate_host.hip.h.  One function, deflate_run, serves the three: its source is packed chunks in host
// memory, a row-major array in host memory, or a held array read where it is (Src).  The scratch lives in the handle's PRE_DF_* slots;
// a call works through its chunks in batches so that PRE_DF_WORK stays under DEFLATE_SCRATCH_CAP.

namespace {
constexpr uint32_t DEFLATE_MAX_CHUNK = 16u << 20;             // bytes of one chunk
constexpr size_t DEFLATE_SCRATCH_CAP = (size_t)256 << 20;     // of PRE_DF_WORK (one chunk's scratch, about 12 n + 192 KiB, always fits)

const char* deflate_status_text(int s) { return s == 0 ? "ok" : s == 1 ? "the stream passed compressBound" : s == 2 ? "a stored block of more than 65,535 bytes" : "unknown status"; }

struct DeflateJob {
    Src src; bool array = false;                              // packed chunks, or a row-major array of `shape` cut into `chunk`
    int ndim = 0; long long shape[4] = {1, 1, 1, 1}, chunk[4] = {1, 1, 1, 1}; int elem_bytes = 1;
    int n = 0; uint32_t chunk_bytes = 0; size_t array_bytes = 0;
    uint8_t* blob = nullptr; uint64_t blob_cap = 0; uint64_t* off = nullptr; uint32_t* len = nullptr; int64_t* coord = nullptr; int* status = nullptr;
};

uint64_t deflate_blob_bytes(int n, uint32_t chunk_bytes) { return (uint64_t)n * tfd::bound(chunk_bytes); }

// the outputs of every form, before any GPU work (the job's n and chunk_bytes are set)
int deflate_check_out(tf_handle* h, const char* who, const DeflateJob& j)
{
    if (j.n < 0) return fail(h, TF_ERR_INVALID_ARG, "%s: n = %d chunks", who, j.n);
    if (j.chunk_bytes > DEFLATE_MAX_CHUNK) return fail(h, TF_ERR_INVALID_ARG, "%s: a chunk of %u bytes, at most %u", who, j.chunk_bytes, DEFLATE_MAX_CHUNK);
    if (j.n && (!j.blob || !j.off || !j.len || !j.status || (j.array && !j.coord))) return fail(h, TF_ERR_INVALID_ARG, "%s: null blob, off, len, coord or status", who);
    if (j.blob_cap < deflate_blob_bytes(j.n, j.chunk_bytes))
        return fail(h, TF_ERR_INVALID_ARG, "%s: blob_cap %llu is less than the %d x %u bytes the streams may take", who, (unsigned long long)j.blob_cap, j.n,
                    tfd::bound(j.chunk_bytes));
    return TF_OK;
}

// an array's shape and chunk shape -> the job's n, chunk_bytes and array_bytes; `n` is what the caller sized its outputs for
int deflate_check_array(tf_handle* h, const char* who, DeflateJob& j, int ndim, const int64_t* shape, const int64_t* chunk, int elem_bytes, int n)
{
    if (ndim < 1 || ndim > 4) return fail(h, TF_ERR_INVALID_ARG, "%s: %d dimensions, need 1 to 4", who, ndim);
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return fail(h, TF_ERR_INVALID_ARG, "%s: %d-byte elements, need 1, 2 or 4", who, elem_bytes);
    if (!shape || !chunk) return fail(h, TF_ERR_INVALID_ARG, "%s: null shape or chunk", who);
    double total = elem_bytes, cb = elem_bytes, count = 1;
    for (int d = 0; d < ndim; ++d) {
        if (shape[d] < 1 || shape[d] > std::numeric_limits<int>::max() || chunk[d] < 1 || chunk[d] > std::numeric_limits<int>::max())
            return fail(h, TF_ERR_INVALID_ARG, "%s: dimension %d has shape %lld in chunks of %lld", who, d, (long long)shape[d], (long long)chunk[d]);
        j.shape[d] = shape[d]; j.chunk[d] = chunk[d];
        total *= (double)shape[d]; cb *= (double)chunk[d]; count *= (double)((shape[d] + chunk[d] - 1) / chunk[d]);
    }
    if (cb > DEFLATE_MAX_CHUNK) return fail(h, TF_ERR_INVALID_ARG, "%s: a chunk of %.0f bytes, at most %u", who, cb, DEFLATE_MAX_CHUNK);
    if (total > 64.0 * (1ull << 30)) return fail(h, TF_ERR_INVALID_ARG, "%s: an array of %.0f bytes", who, total);
    if (count != (double)n) return fail(h, TF_ERR_INVALID_ARG, "%s: n = %d, the array has %.0f chunks", who, n, count);
    j.array = true; j.ndim = ndim; j.elem_bytes = elem_bytes; j.n = n; j.chunk_bytes = (uint32_t)cb; j.array_bytes = (size_t)total;
    return TF_OK;
}

int deflate_run(tf_handle* h, const char* who, const DeflateJob& j)
{
    if (!j.n) return TF_OK;
    HIPC(h, hipSetDevice(h->dev));
    const size_t n = (size_t)j.n, cb = j.chunk_bytes, cap = tfd::bound(j.chunk_bytes), stride = (cap + 15) & ~(size_t)15;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t per = 11 * cb + tfd::HASH_SIZE * 4 + tfd::SYM_BUF * 4 + stride;
    const size_t P = std::max<size_t>(1, std::min<size_t>({(DEFLATE_SCRATCH_CAP - 6 * 256) / per, n, 65535}));
    const size_t o_pred = up(P * cb), o_tab = o_pred + up(P * cb * 2), o_head = o_tab + up(P * cb * 8), o_syms = o_head + P * tfd::HASH_SIZE * 4,
                 o_slot = o_syms + P * tfd::SYM_BUF * 4, work_bytes = o_slot + P * stride;
    // the table: coord [n][4] i64 | off [n] u64 | total u64 | len [n] u32 | status [n] i32
    const size_t t_off = n * 32, t_total = t_off + n * 8, t_len = t_total + 8, t_st = t_len + n * 4, tb = t_st + n * 4;
    std::vector<uint8_t> table(tb, 0);
    if (j.array) {                                            // the chunks in row-major order of the chunk grid (h5py's order of writing)
        long long at[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < n; ++i) {
            memcpy(table.data() + i * 32, at, 32);
            for (int d = 0; d < j.ndim; ++d) j.coord[i * j.ndim + d] = at[d];
            for (int d = j.ndim - 1; d >= 0; --d) { at[d] += j.chunk[d]; if (at[d] < j.shape[d]) break; at[d] = 0; }
        }
    }
    Pre pre(h);
    auto* work = pre.get<uint8_t>(tf_handle::PRE_DF_WORK, work_bytes);
    auto* dtab = pre.get<uint8_t>(tf_handle::PRE_DF_TABLE, tb);
    auto* dblob = pre.get<uint8_t>(tf_handle::PRE_DF_BLOB, std::max<size_t>(n * cap, 16));
    auto* dsrc = j.array && j.src.host ? pre.get<uint8_t>(tf_handle::PRE_DF_SRC, j.array_bytes) : nullptr;
    if (pre.rc) return pre.rc;
    const uint8_t* array = nullptr;
    if (j.array) if (int rc = src_to_device(h, j.src, 0, j.array_bytes, dsrc, &array)) return rc;
    HIPC(h, hipMemcpyAsync(dtab, table.data(), tb, hipMemcpyHostToDevice, h->stream));
    uint8_t* din = work;
    auto* dpred = (uint16_t*)(work + o_pred); auto* dmatch = (tfd::Entry*)(work + o_tab); auto* dhead = (uint32_t*)(work + o_head);
    auto* dsyms = (uint32_t*)(work + o_syms); uint8_t* dslot = work + o_slot;
    auto* dcoord = (const long long*)dtab; auto* doff = (unsigned long long*)(dtab + t_off); auto* dtotal = (unsigned long long*)(dtab + t_total);
    auto* dlen = (uint32_t*)(dtab + t_len); auto* dstat = (int*)(dtab + t_st);
    UnchunkDims dims;
    for (int d = 0; d < 4; ++d) { dims.shape[d] = j.shape[d]; dims.chunk[d] = j.chunk[d]; }
    for (size_t c0 = 0; c0 < n; c0 += P) {
        const unsigned m = (unsigned)std::min(P, n - c0);
        ++h->deflate_batches;
        HIPC(h, hipEventRecord(h->ev[3], h->stream));
        if (j.array) {
            const size_t elems = cb / (size_t)j.elem_bytes;
            const dim3 grid(m, (unsigned)std::min<size_t>((elems + 2047) / 2048, 64));
#define TF_CHUNK(T) hipLaunchKernelGGL(k_chunk<T>, grid, dim3(256), 0, h->stream, (const T*)array, dcoord + 4 * c0, dims, cb, din)
            if (j.elem_bytes == 1) TF_CHUNK(uint8_t); else if (j.elem_bytes == 2) TF_CHUNK(uint16_t); else TF_CHUNK(uint32_t);
#undef TF_CHUNK
            HIPC(h, hipGetLastError());
        } else if (cb) {
            HIPC(h, hipMemcpyAsync(din, (const uint8_t*)j.src.host + c0 * cb, m * cb, hipMemcpyHostToDevice, h->stream));
            h->tail_upload_bytes += (long long)(m * cb);
        }
        HIPC(h, hipEventRecord(h->ev[0], h->stream));
        if (cb) {
            hipLaunchKernelGGL(k_deflate_links, dim3(m), dim3(64), 0, h->stream, (const uint8_t*)din, (uint32_t)cb, dhead, dpred);
            hipLaunchKernelGGL(k_deflate_search, dim3((unsigned)((cb + 255) / 256), m), dim3(256), 0, h->stream, (const uint8_t*)din, (uint32_t)cb,
                               (const uint16_t*)dpred, dmatch);
            HIPC(h, hipGetLastError());
        }
        HIPC(h, hipEventRecord(h->ev[1], h->stream));
        hipLaunchKernelGGL(k_deflate_emit, dim3(m), dim3(1), 0, h->stream, (const uint8_t*)din, (uint32_t)cb, (const tfd::Entry*)dmatch, dsyms, dslot, stride,
                           (uint32_t)cap, dlen + c0, dstat + c0);
        hipLaunchKernelGGL(k_deflate_offsets, dim3(1), dim3(256), 0, h->stream, (const uint32_t*)(dlen + c0), (int)m, doff + c0, dtotal);
        hipLaunchKernelGGL(k_deflate_pack, dim3(m, (unsigned)std::min<size_t>((cap + 4095) / 4096, 32)), dim3(256), 0, h->stream, (const uint8_t*)dslot, stride,
                           (const uint32_t*)(dlen + c0), (const unsigned long long*)(doff + c0), dblob, (unsigned long long)(n * cap));
        HIPC(h, hipGetLastError());
        HIPC(h, hipEventRecord(h->ev[2], h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));             // the next batch writes the same scratch and records the same events
        if (j.array) (void)dev_time(h, 3, 0, tf_handle::DT_CHUNK, true);
        (void)dev_time(h, 0, 1, tf_handle::DT_DEFLATE_MATCH, true);
        (void)dev_time(h, 1, 2, tf_handle::DT_DEFLATE_EMIT, true);
    }
    HIPC(h, hipMemcpyAsync(table.data() + t_off, dtab + t_off, tb - t_off, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    unsigned long long total = 0;
    memcpy(&total, table.data() + t_total, 8);
    memcpy(j.off, table.data() + t_off, n * 8); memcpy(j.len, table.data() + t_len, n * 4); memcpy(j.status, table.data() + t_st, n * 4);
    if (total > n * cap) return fail(h, TF_ERR_HIP, "%s: the streams take %llu bytes, more than their slots", who, total);
    if (total) HIPC(h, hipMemcpyAsync(j.blob, dblob, total, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < j.n; ++i)
        if (j.status[i]) return fail(h, TF_ERR_UNSUPPORTED, "%s: chunk %d did not deflate: status %d (%s)", who, i, j.status[i], deflate_status_text(j.status[i]));
    return TF_OK;
}
}  // namespace

TF_API int tf_deflate(tf_handle* h, const uint8_t* chunks, int n, uint32_t chunk_bytes, uint8_t* blob, uint64_t blob_cap, uint64_t* off, uint32_t* len, int* status)
{
    if (!h) return TF_ERR_INVALID_ARG;
    DeflateJob j;
    j.src = Src::on_host(chunks); j.n = n; j.chunk_bytes = chunk_bytes;
    j.blob = blob; j.blob_cap = blob_cap; j.off = off; j.len = len; j.status = status;
    if (n > 0 && chunk_bytes && !chunks) return fail(h, TF_ERR_INVALID_ARG, "tf_deflate: null chunks");
    if (int rc = deflate_check_out(h, "tf_deflate", j)) return rc;
    return finish_host_call(h, deflate_run(h, "tf_deflate", j));
}

TF_API int tf_deflate_array(tf_handle* h, const void* array, int ndim, const int64_t* shape, const int64_t* chunk, int elem_bytes, int n, uint8_t* blob,
                            uint64_t blob_cap, uint64_t* off, uint32_t* len, int64_t* coord, int* status)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const char* who = "tf_deflate_array";
    if (!array) return fail(h, TF_ERR_INVALID_ARG, "%s: null array", who);
    DeflateJob j;
    if (int rc = deflate_check_array(h, who, j, ndim, shape, chunk, elem_bytes, n)) return rc;
    j.src = Src::on_host(array);
    j.blob = blob; j.blob_cap = blob_cap; j.off = off; j.len = len; j.coord = coord; j.status = status;
    if (int rc = deflate_check_out(h, who, j)) return rc;
    return finish_host_call(h, deflate_run(h, who, j));
}

TF_API int tf_held_deflate(tf_handle* h, int what, int slot, const int64_t* chunk, int n, uint8_t* blob, uint64_t blob_cap, uint64_t* off, uint32_t* len,
                           int64_t* coord, int* status)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const char* who = "tf_held_deflate";
    if (int rc = held_study(h, who)) return rc;
    const tf_handle::Held& k = h->held;
    int64_t shape[4] = {k.N, k.H, k.W, 2};
    int ndim = 4, elem_bytes = 2;
    const void* p = k.flow;
    if (what == TF_HELD_ECHO) {
        if (!k.echo) return fail(h, TF_ERR_INVALID_ARG, "%s: the held study has no echo", who);
        shape[0] = k.n_echo; ndim = 3; p = k.echo;
    } else if (what == TF_HELD_MASK) {
        const tf_handle::Held::Mask* m = nullptr;
        if (int rc = held_mask(h, who, slot, 1, &m)) return rc;
        shape[0] = m->n_frames; shape[3] = m->C; elem_bytes = 1; p = m->p;
    } else if (what != TF_HELD_FLOW) return fail(h, TF_ERR_INVALID_ARG, "%s: what = %d is none of flow (0), echo (1), mask (2)", who, what);
    DeflateJob j;
    if (int rc = deflate_check_array(h, who, j, ndim, shape, chunk, elem_bytes, n)) return rc;
    j.src = Src::on_device(p);
    j.blob = blob; j.blob_cap = blob_cap; j.off = off; j.len = len; j.coord = coord; j.status = status;
    if (int rc = deflate_check_out(h, who, j)) return rc;
    return finish_host_call(h, deflate_run(h, who, j));
}
