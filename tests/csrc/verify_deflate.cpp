// The deflate core (tee_optical_flow_amd/csrc/teeflow_deflate_core.h) on the host, for tests/test_deflate_cpu.py: built with the
// address and undefined-behaviour sanitizers, it compresses every input of a corpus file with buffers allocated at their exact sizes
// (the input, the links, the two match tables, the symbols, and a slot of compressBound(n) bytes), so that a read or a write one byte
// outside any of them is a sanitizer report.
//   verify_deflate <corpus> <result>
// corpus: u32 count, then per input u32 n and the n bytes.  result: per input i32 status, u32 length, u32 clean (1: the slot still
// holds 0xEE behind the stream) and the stream's bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "teeflow_deflate_core.h"

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <class T> static T* exact(size_t count) { return count ? (T*)malloc(count * sizeof(T)) : nullptr; }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s corpus result\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    uint32_t count = 0;
    if (!read_exact(in, &count, 4)) return 2;
    tfd::Work* w = new tfd::Work;
    uint32_t* head = exact<uint32_t>(tfd::HASH_SIZE);
    uint32_t* syms = exact<uint32_t>(tfd::SYM_BUF);
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t n = 0;
        if (!read_exact(in, &n, 4) || n > tfd::MAX_BYTES) return 2;
        const uint32_t cap = tfd::bound(n);
        uint8_t* src = exact<uint8_t>(n);                               // (an empty input has no buffer: none of its bytes may be read)
        uint16_t* pred = exact<uint16_t>(n);
        tfd::Entry* tab = exact<tfd::Entry>(2 * (size_t)n);
        uint8_t* dst = exact<uint8_t>(cap);
        if ((n && (!src || !pred || !tab)) || !dst || !read_exact(in, src, n)) return 2;
        memset(dst, 0xEE, cap);
        memset(w, 0xA5, sizeof *w);                                    // nothing of one stream's state serves the next
        memset(head, 0xA5, tfd::HASH_SIZE * sizeof *head);
        memset(syms, 0xA5, tfd::SYM_BUF * sizeof *syms);
        tfd::links(src, n, head, pred);
        for (uint32_t p = 0; p < n; ++p) tfd::search(src, n, pred, p, tab + 2 * (size_t)p);
        uint32_t len = 0;
        const int32_t status = tfd::deflate(src, n, tab, syms, *w, dst, cap, &len);
        uint32_t clean = len <= cap;
        for (uint32_t k = len; k < cap && clean; ++k) clean = dst[k] == 0xEE;
        fwrite(&status, 4, 1, out); fwrite(&len, 4, 1, out); fwrite(&clean, 4, 1, out);
        if (len && len <= cap) fwrite(dst, 1, len, out);
        free(src); free(pred); free(tab); free(dst);
    }
    delete w; free(head); free(syms);
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
