// A batch of byte streams between the C ABI and a one-wave-per-stream kernel: the check before any GPU work, the upload in the format
// of teeflow_streams_core.h, and the verdict on the statuses the kernel left.  Shared by inflate (teeflow_inflate_host.hip.h) and RLE
// (teeflow_frames_host.hip.h), which pass what differs -- nouns, caps, slots, counters, status texts -- and keep their own argument
// checks and kernel launches.  Relies on teeflow_scratch.hip.h.
#include "teeflow_streams_core.h"

namespace {
// before any GPU work: the three pointers, every stream's length against `cap`, and the span
int streams_check(tf_handle* h, const char* who, tfs::Batch& b, uint32_t cap, const char* noun)
{
    if (b.n && (!b.blob || !b.off || !b.len)) return fail(h, TF_ERR_INVALID_ARG, "%s: null blob, off or len", who);
    char msg[160];
    return tfs::span(b, cap, noun, msg, sizeof msg) ? TF_OK : fail(h, TF_ERR_INVALID_ARG, "%s: %s", who, msg);
}

// The span of b and the table t onto the device, into the two PRE_* slots the caller names, behind what is queued on the handle's
// stream; not waited for, so t lives until the stream has been.  The span's bytes are counted in `uploaded`.
int streams_upload(tf_handle* h, const tfs::Batch& b, const tfs::Table& t, int slot_blob, int slot_table, long long tf_handle::*uploaded,
                   const uint8_t** dblob, uint8_t** dtab)
{
    Pre pre(h);
    auto* blob = pre.get<uint8_t>(slot_blob, b.device_bytes());
    auto* tab = pre.get<uint8_t>(slot_table, t.bytes.size());
    if (pre.rc) return pre.rc;
    if (b.bytes()) HIPC(h, hipMemcpyAsync(blob + b.skew(), b.blob + b.lo, b.bytes(), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(tab, t.bytes.data(), t.bytes.size(), hipMemcpyHostToDevice, h->stream));
    h->*uploaded += (long long)b.bytes();
    *dblob = blob; *dtab = tab;
    return TF_OK;
}

// the first stream with a status -> the call's failure: "<who>: <noun> i did not <verb>: status s (<text>); k of n failed"
int streams_verdict(tf_handle* h, const char* who, const char* noun, const char* verb, const char* (*text)(int), const int* status, int n)
{
    const int bad = n - (int)std::count(status, status + n, 0);
    if (!bad) return TF_OK;
    const int i = (int)(std::find_if(status, status + n, [](int s) { return s != 0; }) - status);
    return fail(h, TF_ERR_INVALID_ARG, "%s: %s %d did not %s: status %d (%s); %d of %d failed", who, noun, i, verb, status[i], text(status[i]), bad, n);
}
}  // namespace
