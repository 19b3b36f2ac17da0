// The host side of inflate on the device (kernels: teeflow_inflate.hip.h): tf_inflate, and a study held from the chunks of its file,
// tf_hold_study_chunks / tf_hold_mask_chunks.  Included by teeflow.hip after teeflow_streams_host.hip.h (the batch of streams: check, upload, verdict),
// teeflow_held.hip.h and teeflow_study_host.hip.h.  The compressed bytes, the per-stream
// table and the inflated chunk-major bytes live in the handle's PRE_INF_* slots; a held array is inflated and assembled into a fresh
// buffer and takes the held one's place only when every chunk of the call has decoded, so a failed call changes nothing.

namespace {
constexpr uint32_t INFLATE_MAX_BYTES = 1u << 30;              // of one stream and of its output

const char* inflate_status_text(int s)
{
    static const char* const text[] = {"ok", "bad header", "bad block type", "bad stored length", "bad code lengths", "distance before the start of the output",
                                       "input truncated", "output longer or shorter than expected", "checksum mismatch"};
    return s >= 0 && s <= 8 ? text[s] : "unknown status";
}

struct InflateJob {
    tfs::Batch in; const uint8_t* raw; uint32_t out_bytes;    // the streams (checked: inflate_check), which of them are stored raw, every slot's size
};

// before any GPU work
int inflate_check(tf_handle* h, const char* who, InflateJob& j)
{
    if (j.in.n < 0) return fail(h, TF_ERR_INVALID_ARG, "%s: n = %d streams", who, j.in.n);
    if (j.out_bytes > INFLATE_MAX_BYTES) return fail(h, TF_ERR_INVALID_ARG, "%s: %u output bytes per stream, at most %u", who, j.out_bytes, INFLATE_MAX_BYTES);
    return streams_check(h, who, j.in, INFLATE_MAX_BYTES, "stream");
}

// what a launched inflate left on the device (valid once the handle's stream has run it)
struct Inflated {
    const uint8_t* bytes = nullptr; size_t stride = 0;        // stream i's output: bytes + i * stride
    const uint8_t* blob = nullptr;                            // the uploaded span, and per stream:
    const unsigned long long* off = nullptr; const uint8_t* raw = nullptr; const long long* coord = nullptr;
    int* status = nullptr; uint32_t* produced = nullptr;
    tfs::Table table;                                         // the host side of the per-stream table: lives until the stream is waited for
};

// The streams of j (n >= 1) onto the device and k_inflate behind them on the handle's stream, between ev[0] and ev[1]; not waited
// for.  coord4: host [n][4] chunk coordinates that go up with the table, or null.
int inflate_launch(tf_handle* h, const InflateJob& j, const long long* coord4, Inflated* r)
{
    const size_t n = (size_t)j.in.n;
    r->stride = ((size_t)j.out_bytes + 15) & ~(size_t)15;
    enum { COORD, OFF, LEN, STATUS, PRODUCED, RAW };          // coord [n][4] i64 | off [n] u64 | len [n] u32 | status [n] i32 | produced [n] u32 | raw [n] u8
    r->table = tfs::table(j.in, {32, 8, 4, 4, 4, 1}, OFF, LEN);
    if (coord4) memcpy(r->table.col(COORD), coord4, n * 32);
    if (j.raw) for (size_t i = 0; i < n; ++i) r->table.col(RAW)[i] = j.raw[i] ? 1 : 0;
    Pre pre(h);
    auto* dout = pre.get<uint8_t>(tf_handle::PRE_INF_OUT, std::max<size_t>(n * r->stride, 16));
    if (pre.rc) return pre.rc;
    uint8_t* dtab = nullptr;
    if (int rc = streams_upload(h, j.in, r->table, tf_handle::PRE_INF_BLOB, tf_handle::PRE_INF_TABLE, &tf_handle::tail_upload_bytes, &r->blob, &dtab)) return rc;
    const auto& at = r->table.at;
    r->bytes = dout;
    r->coord = (const long long*)(dtab + at[COORD]); r->off = (const unsigned long long*)(dtab + at[OFF]);
    r->status = (int*)(dtab + at[STATUS]); r->produced = (uint32_t*)(dtab + at[PRODUCED]); r->raw = dtab + at[RAW];
    HIPC(h, hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(k_inflate, dim3((unsigned)n), dim3(64), 0, h->stream, r->blob, r->off, (const uint32_t*)(dtab + at[LEN]), r->raw,
                       j.in.n, j.out_bytes, r->stride, dout, r->status, r->produced);
    HIPC(h, hipGetLastError());
    HIPC(h, hipEventRecord(h->ev[1], h->stream));
    return TF_OK;
}

size_t chunk_elems(const tf_chunked& c)
{
    size_t e = 1;
    for (int d = 0; d < c.ndim; ++d) e *= (size_t)c.chunk[d];
    return e;
}

// a chunked dataset's description, before any GPU work: `ndim` dimensions of elem_bytes-byte elements
int chunks_check(tf_handle* h, const char* who, const char* what, const tf_chunked* c, int ndim, int elem_bytes, InflateJob* j)
{
    if (!c) return fail(h, TF_ERR_INVALID_ARG, "%s: null %s description", who, what);
    if (c->ndim != ndim) return fail(h, TF_ERR_INVALID_ARG, "%s: %s has %d dimensions, need %d", who, what, c->ndim, ndim);
    if (c->elem_bytes != elem_bytes) return fail(h, TF_ERR_INVALID_ARG, "%s: %s has %d-byte elements, need %d", who, what, c->elem_bytes, elem_bytes);
    double total = elem_bytes, cb = elem_bytes;
    for (int d = 0; d < ndim; ++d) {
        if (c->shape[d] < 1 || c->shape[d] > std::numeric_limits<int>::max() || c->chunk[d] < 1 || c->chunk[d] > std::numeric_limits<int>::max())
            return fail(h, TF_ERR_INVALID_ARG, "%s: %s: dimension %d has shape %lld in chunks of %lld", who, what, d, (long long)c->shape[d], (long long)c->chunk[d]);
        total *= (double)c->shape[d]; cb *= (double)c->chunk[d];
    }
    if (cb > INFLATE_MAX_BYTES) return fail(h, TF_ERR_INVALID_ARG, "%s: %s: a chunk of %.0f bytes, at most %u", who, what, cb, INFLATE_MAX_BYTES);
    if (total > 64.0 * (1ull << 30)) return fail(h, TF_ERR_INVALID_ARG, "%s: %s: %.0f bytes", who, what, total);
    if ((double)c->chunk_bytes != cb) return fail(h, TF_ERR_INVALID_ARG, "%s: %s: chunk_bytes %u is not the chunk's %.0f bytes", who, what, c->chunk_bytes, cb);
    if (c->n && !c->coord) return fail(h, TF_ERR_INVALID_ARG, "%s: %s: null coord", who, what);
    *j = InflateJob{{c->blob, c->off, c->len, c->n}, c->raw, c->chunk_bytes};
    if (int rc = inflate_check(h, who, *j)) return rc;
    for (int i = 0; i < c->n; ++i)
        for (int d = 0; d < ndim; ++d) {
            const long long at = c->coord[(size_t)i * ndim + d];
            if (at < 0 || at >= c->shape[d]) return fail(h, TF_ERR_INVALID_ARG, "%s: %s: chunk %d starts at %lld of dimension %d, outside [0, %lld)", who, what, i, at, d, (long long)c->shape[d]);
        }
    return TF_OK;
}

// The checked dataset c -> the row-major array dst (device, dst_bytes): zero where the file wrote no chunk.  Waits for the stream;
// a chunk that does not decode fails the call (dst is then the caller's to drop).
int chunks_to_device(tf_handle* h, const char* who, const char* what, const tf_chunked& c, const InflateJob& j, void* dst, size_t dst_bytes)
{
    HIPC(h, hipMemsetAsync(dst, 0, dst_bytes, h->stream));
    if (!c.n) { HIPC(h, hipStreamSynchronize(h->stream)); return TF_OK; }
    std::vector<long long> coord4((size_t)c.n * 4, 0);
    for (int i = 0; i < c.n; ++i)
        for (int d = 0; d < c.ndim; ++d) coord4[(size_t)i * 4 + d] = c.coord[(size_t)i * c.ndim + d];
    Inflated r;
    if (int rc = inflate_launch(h, j, coord4.data(), &r)) return rc;
    UnchunkDims dims;
    for (int d = 0; d < 4; ++d) { dims.shape[d] = d < c.ndim ? c.shape[d] : 1; dims.chunk[d] = d < c.ndim ? c.chunk[d] : 1; }
    const size_t elems = chunk_elems(c);
    const dim3 grid((unsigned)c.n, (unsigned)std::min<size_t>((elems + 2047) / 2048, 64));
#define TF_UNCHUNK(T) hipLaunchKernelGGL(k_unchunk<T>, grid, dim3(256), 0, h->stream, r.bytes, r.stride, r.blob, r.off, r.raw, r.coord, (const int*)r.status, dims, (T*)dst)
    if (c.elem_bytes == 1) TF_UNCHUNK(uint8_t); else if (c.elem_bytes == 2) TF_UNCHUNK(uint16_t); else TF_UNCHUNK(uint32_t);
#undef TF_UNCHUNK
    HIPC(h, hipGetLastError());
    HIPC(h, hipEventRecord(h->ev[2], h->stream));
    std::vector<int> status((size_t)c.n);
    HIPC(h, hipMemcpyAsync(status.data(), r.status, status.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    (void)dev_time(h, 0, 1, tf_handle::DT_INFLATE, true);   // (the stream has been waited for; a counter alone depends on the read-back)
    (void)dev_time(h, 1, 2, tf_handle::DT_UNCHUNK, true);
    return streams_verdict(h, who, what, "inflate", inflate_status_text, status.data(), c.n);
}
}  // namespace

TF_API int tf_inflate(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, const uint8_t* raw, int n, uint32_t out_bytes,
                      uint8_t* out_host, int* status)
{
    if (!h) return TF_ERR_INVALID_ARG;
    InflateJob j{{blob, off, len, n}, raw, out_bytes};
    if (int rc = inflate_check(h, "tf_inflate", j)) return rc;
    if (n && (!status || (out_bytes && !out_host))) return fail(h, TF_ERR_INVALID_ARG, "tf_inflate: null out_host or status");
    if (!n) return TF_OK;
    auto run = [&]() -> int {
        HIPC(h, hipSetDevice(h->dev));
        Inflated r;
        if (int rc = inflate_launch(h, j, nullptr, &r)) return rc;
        std::vector<uint32_t> produced((size_t)n);
        HIPC(h, hipMemcpyAsync(status, r.status, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipMemcpyAsync(produced.data(), r.produced, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        (void)dev_time(h, 0, 1, tf_handle::DT_INFLATE, true);
        // a slot gets what its stream produced and nothing else: all of them in one copy when every stream filled its slot
        bool full = out_bytes > 0;
        for (int i = 0; i < n && full; ++i) full = produced[i] == out_bytes && !(raw && raw[i]);
        if (full) HIPC(h, hipMemcpy2DAsync(out_host, out_bytes, r.bytes, r.stride, out_bytes, (size_t)n, hipMemcpyDeviceToHost, h->stream));
        else
            for (int i = 0; i < n; ++i) {
                uint8_t* slot = out_host + (size_t)i * out_bytes;
                if (raw && raw[i]) { if (status[i] == 0 && out_bytes) memcpy(slot, blob + off[i], out_bytes); }
                else if (produced[i]) HIPC(h, hipMemcpyAsync(slot, r.bytes + (size_t)i * r.stride, produced[i], hipMemcpyDeviceToHost, h->stream));
            }
        HIPC(h, hipStreamSynchronize(h->stream));
        return streams_verdict(h, "tf_inflate", "stream", "inflate", inflate_status_text, status, n);
    };
    return finish_host_call(h, run());
}

TF_API int tf_hold_study_chunks(tf_handle* h, const tf_chunked* flow, const tf_chunked* echo)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const char* who = "tf_hold_study_chunks";
    InflateJob jf, je;
    if (int rc = chunks_check(h, who, "flow", flow, 4, 2, &jf)) return rc;
    if (flow->shape[3] != 2) return fail(h, TF_ERR_INVALID_ARG, "%s: flow's last dimension is %lld, need 2", who, (long long)flow->shape[3]);
    if (echo) {
        if (int rc = chunks_check(h, who, "echo", echo, 3, 2, &je)) return rc;
        if (echo->shape[1] != flow->shape[1] || echo->shape[2] != flow->shape[2])
            return fail(h, TF_ERR_INVALID_ARG, "%s: echo frames are %lld x %lld, flow frames %lld x %lld", who, (long long)echo->shape[1], (long long)echo->shape[2],
                        (long long)flow->shape[1], (long long)flow->shape[2]);
    }
    const int N = (int)flow->shape[0], H = (int)flow->shape[1], W = (int)flow->shape[2], n_echo = echo ? (int)echo->shape[0] : 0;
    uint16_t* dflow = nullptr; uint16_t* decho = nullptr;
    auto run = [&]() -> int {
        HIPC(h, hipSetDevice(h->dev));
        const size_t HW = (size_t)H * W, fb = (size_t)N * HW * 2 * sizeof(uint16_t), eb = (size_t)n_echo * HW * sizeof(uint16_t);
        HIPC(h, hipMalloc(&dflow, fb));
        if (echo) HIPC(h, hipMalloc(&decho, eb));
        if (int rc = chunks_to_device(h, who, "flow chunk", *flow, jf, dflow, fb)) return rc;
        if (echo) if (int rc = chunks_to_device(h, who, "echo chunk", *echo, je, decho, eb)) return rc;
        tf_handle::Held& k = h->held;                        // every chunk decoded, the stream is drained: the new study takes the place
        k.release();
        k.flow = dflow; k.echo = decho; k.N = N; k.H = H; k.W = W; k.n_echo = n_echo;
        ++k.gen;
        dflow = decho = nullptr;
        return TF_OK;
    };
    const int rc = finish_host_call(h, run());
    (void)hipFree(dflow); (void)hipFree(decho);              // (a failed call's; null after a good one)
    return rc;
}

TF_API int tf_hold_mask_chunks(tf_handle* h, int slot, const tf_chunked* mask)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const char* who = "tf_hold_mask_chunks";
    if (int rc = held_study(h, who)) return rc;
    if (slot < 0 || slot >= TF_HELD_SLOTS) return fail(h, TF_ERR_INVALID_ARG, "%s: mask slot %d is out of range [0, %d)", who, slot, TF_HELD_SLOTS);
    InflateJob j;
    if (int rc = chunks_check(h, who, "mask", mask, 4, 1, &j)) return rc;
    if (mask->shape[1] != h->held.H || mask->shape[2] != h->held.W || (mask->shape[3] != 1 && mask->shape[3] != 2))
        return fail(h, TF_ERR_INVALID_ARG, "%s: the mask is [%lld][%lld][%lld][%lld], need [n][%d][%d][1 or 2] (the held study's frames)", who, (long long)mask->shape[0],
                    (long long)mask->shape[1], (long long)mask->shape[2], (long long)mask->shape[3], h->held.H, h->held.W);
    uint8_t* p = nullptr;
    auto run = [&]() -> int {
        HIPC(h, hipSetDevice(h->dev));
        const size_t bytes = (size_t)mask->shape[0] * h->held.H * h->held.W * (size_t)mask->shape[3];
        HIPC(h, hipMalloc(&p, bytes));
        if (int rc = chunks_to_device(h, who, "mask chunk", *mask, j, p, bytes)) return rc;
        tf_handle::Held::Mask& m = h->held.mask[slot];
        (void)hipFree(m.p);                                   // (the tail calls are host-synchronous: nothing reads the old mask)
        m.p = p; m.n_frames = (int)mask->shape[0]; m.C = (int)mask->shape[3];
        p = nullptr;
        return TF_OK;
    };
    const int rc = finish_host_call(h, run());
    (void)hipFree(p);
    return rc;
}
