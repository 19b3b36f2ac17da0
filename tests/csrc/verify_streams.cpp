// The stream-batch arithmetic (tee_optical_flow_amd/csrc/teeflow_streams_core.h) on the host: the span walk and the table builder that
// inflate and RLE share, built with -fsanitize=address,undefined by tests/test_streams_cpu.py.  off[] and len[] live in heap buffers
// of exactly their size; the blob is never read by this arithmetic, so its offsets may be anywhere below 2^63.
//   verify_streams
// Exit status 0 and "<n> checks ok": every lo, hi, rewritten offset and column is the expected one.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "teeflow_streams_core.h"

static long g_checks = 0;
#define MUST(ok)                                                                                  \
    do {                                                                                          \
        ++g_checks;                                                                               \
        if (!(ok)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #ok); exit(1); }          \
    } while (0)

static const uint8_t BLOB[1] = {0};
static const std::initializer_list<size_t> INFLATE_COLS = {32, 8, 4, 4, 4, 1}, RLE_COLS = {8, 4, 4};   // coord | off | len | status | produced | raw; off | len | status

// a batch that owns its off[] and len[] (exact-size heap buffers), and what span() made of it
struct Spanned {
    std::vector<uint64_t> off; std::vector<uint32_t> len;
    tfs::Batch b; bool ok; char msg[160];
    Spanned(std::vector<uint64_t> off_, std::vector<uint32_t> len_, uint32_t cap, const char* noun)
        : off(std::move(off_)), len(std::move(len_)), b{BLOB, off.data(), len.data(), (int)off.size()}
    {
        msg[0] = 0;
        ok = tfs::span(b, cap, noun, msg, sizeof msg);
    }
    Spanned(const Spanned&) = delete;
};

// the table of a spanned batch in one layout: every column inside the table, aligned to its entry, end to end; the offsets rewritten,
// the lengths copied, everything else zero
static void check_table(const tfs::Batch& b, const std::initializer_list<size_t>& widths, int col_off, int col_len)
{
    tfs::Table t = tfs::table(b, widths, col_off, col_len);
    const size_t n = (size_t)b.n, cols = widths.size();
    MUST(t.at.size() == cols + 1 && t.at[0] == 0 && t.at[cols] == t.bytes.size());
    size_t c = 0, total = 0;
    for (size_t w : widths) {
        MUST(t.at[c] == total && t.at[c] % w == 0 && t.at[c] + n * w == t.at[c + 1] && t.at[c + 1] <= t.bytes.size());
        total += n * w; ++c;
    }
    MUST(total == t.bytes.size());
    const size_t skew = (size_t)(b.lo & 15);
    MUST(b.skew() == skew && b.bytes() == (size_t)(b.hi - b.lo) && b.device_bytes() == skew + b.bytes() + 32);
    for (size_t i = 0; i < n; ++i) {
        uint64_t o; uint32_t l;
        memcpy(&o, t.col(col_off) + i * 8, 8); memcpy(&l, t.col(col_len) + i * 4, 4);
        MUST(o == b.off[i] - b.lo + skew && l == b.len[i]);
        MUST((o & 15) == (b.off[i] & 15));                                  // the device copy keeps the blob's alignment mod 16
        // every 16-byte aligned piece that overlaps the stream lies inside the padded copy
        MUST(o >= skew && ((o + l + 15) & ~(uint64_t)15) <= b.device_bytes());
    }
    c = 0;
    for (size_t w : widths) {
        if ((int)c != col_off && (int)c != col_len)
            for (size_t k = 0; k < n * w; ++k) MUST(t.col((int)c)[k] == 0);
        ++c;
    }
}

static void check_both_layouts(const tfs::Batch& b)
{
    check_table(b, INFLATE_COLS, 1, 2);
    check_table(b, RLE_COLS, 0, 1);
}

int main()
{
    const uint32_t CAP = 1u << 30;
    // empty batches: null arrays are never read, the span is [0, 0), the tables are empty
    for (int n : {0, -1}) {
        tfs::Batch e{nullptr, nullptr, nullptr, n};
        char msg[160];
        MUST(tfs::span(e, CAP, "stream", msg, sizeof msg) && e.lo == 0 && e.hi == 0 && e.bytes() == 0 && e.device_bytes() == 32);
        tfs::Table t = tfs::table(e, INFLATE_COLS, 1, 2);
        MUST(t.bytes.empty() && t.at.size() == 7);
        for (size_t a : t.at) MUST(a == 0);
        t = tfs::table(e, RLE_COLS, 0, 1);
        MUST(t.bytes.empty() && t.at.size() == 4);
    }
    // one stream at every lo & 15, near the blob's start and far inside it; a stream of no bytes
    for (uint64_t base : {(uint64_t)0, (uint64_t)4096, (uint64_t)1 << 40})
        for (uint64_t g = 0; g < 16; ++g)
            for (uint32_t len : {0u, 1u, 15u, 16u, 17u, 1000u}) {
                Spanned s({base + g}, {len}, CAP, "stream");
                MUST(s.ok && s.b.lo == base + g && s.b.hi == base + g + len && s.b.skew() == g);
                check_both_layouts(s.b);
            }
    // several streams behind g junk bytes: out of order, overlapping, touching, one of no bytes; lo is the least offset, hi the
    // greatest end, whichever streams have them
    for (uint64_t g = 0; g < 16; ++g) {
        const uint64_t rel[6] = {700, 0, 259, 259, 300, 1400};
        Spanned s({g + rel[0], g + rel[1], g + rel[2], g + rel[3], g + rel[4], g + rel[5]}, {300, 259, 41, 0, 1100, 3}, CAP, "frame");
        MUST(s.ok && s.b.lo == g && s.b.hi == g + 1403 && s.b.bytes() == 1403 && s.b.skew() == g);
        check_both_layouts(s.b);
        tfs::Table t = tfs::table(s.b, RLE_COLS, 0, 1);
        for (int i = 0; i < 6; ++i) { uint64_t o; memcpy(&o, t.col(0) + i * 8, 8); MUST(o == rel[i] + g); }   // off - lo + skew, lo = skew = g
    }
    // off + len at the 63-bit limit, and one past it
    for (uint32_t len : {0u, 1u, 77u, CAP}) {
        const uint64_t at = tfs::OFF_LIMIT - len;
        Spanned fits({16, at}, {4, len}, CAP, "stream");
        MUST(fits.ok && fits.b.lo == 16 && fits.b.hi == tfs::OFF_LIMIT);
        check_both_layouts(fits.b);
        Spanned past({16, at + 1}, {4, len}, CAP, "stream");
        MUST(!past.ok && strstr(past.msg, "stream 1 starts") && strstr(past.msg, "overflows"));
        Spanned frame({16, at + 1}, {4, len}, CAP, "frame");
        MUST(!frame.ok && strstr(frame.msg, "frame 1") && strstr(frame.msg, "overflows"));
    }
    for (uint64_t far : {(uint64_t)1 << 63, ~(uint64_t)0}) MUST(!Spanned({0, far}, {4, 0}, CAP, "stream").ok);
    // a length at the cap, and one past it (both callers' caps)
    for (uint32_t cap : {CAP, 0xFFFFF000u, 0u}) {
        const uint32_t small = cap ? 1 : 0;
        Spanned fits({5, 9}, {small, cap}, cap, "stream");
        MUST(fits.ok && fits.b.lo == 5 && fits.b.hi == 9 + (uint64_t)cap);
        check_both_layouts(fits.b);
        Spanned past({5, 9}, {small, cap + 1}, cap, "stream");
        MUST(!past.ok && strstr(past.msg, "stream 1 has") && strstr(past.msg, "at most"));
    }
    printf("%ld checks ok\n", g_checks);
    return 0;
}
