// The inflate core (tee_optical_flow_amd/csrc/teeflow_inflate_core.h) on one lane, for tests/test_inflate_cpu.py: built with the
// address and undefined-behaviour sanitizers, it decodes every stream of a corpus file into buffers allocated at their exact sizes
// and writes what it got, so that a read or a write one byte outside either buffer is a sanitizer report.
//   verify_inflate <corpus> <result>
// corpus: u32 n, then per stream u32 in_len, u32 out_bytes and the in_len bytes.  result: per stream i32 status, u32 produced and
// the out_bytes bytes of its output buffer (0xEE where nothing was written).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "teeflow_inflate_core.h"

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s corpus result\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    uint32_t n = 0;
    if (!read_exact(in, &n, 4)) return 2;
    tfi::Tables* t = new tfi::Tables;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t head[2];
        if (!read_exact(in, head, 8)) return 2;
        uint8_t* src = (uint8_t*)malloc(head[0] ? head[0] : 1);        // exact sizes: the sanitizer guards both ends
        uint8_t* dst = (uint8_t*)malloc(head[1] ? head[1] : 1);
        if (!src || !dst || !read_exact(in, src, head[0])) return 2;
        if (head[0] == 0) { free(src); src = nullptr; }               // no byte of an empty stream may be read
        memset(dst, 0xEE, head[1] ? head[1] : 1);
        memset(t, 0xA5, sizeof *t);                                   // nothing of a stream's tables serves the next
        tfi::HostIO io(src, dst, head[1]);
        const int32_t status = tfi::inflate_zlib(io, *t, head[0], head[1]);
        const uint32_t produced = io.produced();
        fwrite(&status, 4, 1, out); fwrite(&produced, 4, 1, out);
        if (head[1]) fwrite(dst, 1, head[1], out);
        free(src); free(dst);
    }
    delete t;
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
