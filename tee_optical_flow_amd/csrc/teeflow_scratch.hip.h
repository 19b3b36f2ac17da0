// What every call of the study tail shares: the handle's PRE_* scratch slots (grown on demand, never shrunk, freed with the handle,
// so a call neither allocates nor frees once a study's sizes have been seen), the chunk walk, and Src, a call's input on the host or
// on the device.  Relies on teeflow_engine.hip.h (tf_handle, HIPC, fail).

namespace {
int pre_grow(tf_handle* h, int which, size_t bytes, void** out)
{
    tf_handle::GrowBuf& b = h->pre[which];
    if (b.cap < bytes) {
        if (b.p) { HIPC(h, hipStreamSynchronize(h->stream)); (void)hipFree(b.p); }
        b.p = nullptr; b.cap = 0;
        HIPC(h, hipMalloc(&b.p, bytes));
        b.cap = bytes;
    }
    *out = b.p;
    return TF_OK;
}

// typed access to the slots; latches the first error (get() gives nullptr from then on), to be checked once after the last get()
struct Pre {
    tf_handle* h;
    int rc = TF_OK;
    explicit Pre(tf_handle* h_) : h(h_) {}
    template <typename T>
    T* get(int which, size_t count)
    {
        void* p = nullptr;
        if (rc == TF_OK) rc = pre_grow(h, which, count * sizeof(T), &p);
        return (T*)p;
    }
};

// a failed call leaves nothing of it running: its destinations are host memory the caller may free at once
// (a call refused for its null handle passes through)
int finish_host_call(tf_handle* h, int rc)
{
    if (rc != TF_OK && h) {
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        (void)hipGetLastError();
    }
    return rc;
}

// A study goes through the chunked calls in chunks of as many frames as fit in `budget` bytes of per-chunk scratch: at most N (and
// `cap`, where a chunk's planes are a grid dimension), at least 1.  The walk is the same everywhere:
//     for (int f0 = 0; f0 < N; f0 += nf) { const int n = std::min(nf, N - f0); ... frames [f0, f0 + n) ... }
constexpr size_t MASK_CHUNK_BYTES = (size_t)512 << 20;

int chunk_frames(size_t bytes_per_frame, int N, size_t cap = 65535, size_t budget = MASK_CHUNK_BYTES)
{
    const size_t nf = std::min({budget / bytes_per_frame, (size_t)N, cap});
    return nf < 1 ? 1 : (int)nf;
}

// the start values of `pairs` (min, max) key pairs; the caller keeps them alive until the stream has run their upload
std::vector<u64> minmax_seed(size_t pairs)
{
    std::vector<u64> init(pairs * 2);
    for (size_t i = 0; i < pairs; ++i) { init[2 * i] = ~0ull; init[2 * i + 1] = 0ull; }
    return init;
}

// Where a tail call finds its flow, its mask or its echo: host memory, which the call uploads into its scratch, or device memory
// that already holds it (a held study's buffers, teeflow_held.hip.h), which the call's kernels read where it is.
struct Src {
    const void* host = nullptr; const void* dev = nullptr;
    static Src on_host(const void* p) { return {p, nullptr}; }
    static Src on_device(const void* p) { return {nullptr, p}; }
};

// bytes [off, off + bytes) of src, on the device: *out is the resident bytes themselves, or `scratch` behind their upload on the
// handle's stream, counted in `uploaded` (a call's frames count in frames_upload_bytes)
int src_to_device(tf_handle* h, const Src& src, size_t off, size_t bytes, void* scratch, const uint8_t** out,
                  long long tf_handle::*uploaded = &tf_handle::tail_upload_bytes)
{
    if (src.dev) { *out = (const uint8_t*)src.dev + off; return TF_OK; }
    HIPC(h, hipMemcpyAsync(scratch, (const uint8_t*)src.host + off, bytes, hipMemcpyHostToDevice, h->stream));
    h->*uploaded += (long long)bytes;
    *out = (const uint8_t*)scratch;
    return TF_OK;
}
}  // namespace
