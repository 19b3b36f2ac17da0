// The JPEG Lossless core (tee_optical_flow_amd/csrc/teeflow_jpegll_core.h, on top of teeflow_jpeg_core.h) on the host, over the corpus
// of tests/jpegll_cases.py, every stream in a heap buffer of exactly its length, every restart interval's data in one of exactly its
// length, and the differences, the component planes and the output in buffers of exactly their size: built with
// -fsanitize=address,undefined by tests/test_jpegll_cpu.py, so that a read or write of one byte outside them ends the program.
//   verify_jpegll <corpus.bin>
// corpus.bin: uint32 count, then per case uint32 H, W, samples, len, status, the stream's len bytes and -- status 0 -- the
// H * W * samples bytes [H][W][samples] it decodes to.  Exit status 0: every status and every output is the expected one.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "teeflow_jpegll_core.h"

static void must(bool ok, const char* what) { if (!ok) { fprintf(stderr, "the core broke its contract: %s\n", what); abort(); } }

// a restart interval's data bytes [pos, end) of the frame in a buffer of their own
struct HostIO {
    const uint8_t* data; uint32_t pos, end;
    uint8_t in_byte(uint32_t i) { must(i >= pos && i < end, "in_byte outside the interval"); return data[i - pos]; }
};

// one frame as the kernels take it -> its status; out [H][W][samples] is written only for status 0
static int decode_frame(const uint8_t* frame, uint32_t len, int H, int W, int samples, uint8_t* out)
{
    tfj::Desc d;
    auto byte = [&](uint32_t i) -> uint8_t { must(i < len, "a byte past the frame"); return frame[i]; };
    int rc = tfl::parse_header(byte, len, H, W, samples, &d);
    if (rc) return rc;
    must(d.nint >= 1 && d.nint <= (uint32_t)H && d.scan_off <= len && d.ncomp == samples && d.nmcu == (uint32_t)H * (uint32_t)W && d.mcux == W && d.mcuy == H,
         "the descriptor");
    std::vector<uint32_t> rst(d.nint - 1);                                 // (exactly the positions k_jpeg_marks may write)
    uint32_t scan_end = 0;
    rc = tfj::find_marks(byte, len, d, rst.data(), &scan_end);
    if (rc) return rc;
    tfj::Huff huff[4];
    for (int t = 0; t < 4; ++t) tfj::huff_build(d.bits[t], d.vals[t], huff[t]);
    const size_t hw = (size_t)H * W;
    uint16_t* diff = (uint16_t*)malloc(hw * samples * sizeof(uint16_t));   // planar [component][H * W], exactly
    for (uint32_t k = 0; k < d.nint; ++k) {
        tfj::Bits b;
        b.acc = 0; b.cnt = 0; b.pad = 0;
        b.pos = k ? rst[k - 1] + 2 : d.scan_off;
        b.end = k + 1 < d.nint ? rst[k] : scan_end;
        must(b.pos <= b.end && b.end <= len, "an interval's bounds");
        uint8_t* data = (uint8_t*)malloc(b.end - b.pos);
        memcpy(data, frame + b.pos, b.end - b.pos);
        HostIO io{data, b.pos, b.end};
        const uint32_t s0 = d.ri ? k * d.ri : 0, s1 = d.ri && s0 + d.ri < d.nmcu ? s0 + d.ri : d.nmcu;
        uint32_t r0, r1;
        tfl::interval_rows(d, k, &r0, &r1);
        must(s0 == r0 * (uint32_t)W && s1 == r1 * (uint32_t)W && r1 <= (uint32_t)H, "an interval is whole rows");
        for (uint32_t s = s0; s < s1 && rc == tfj::OK; ++s)
            for (int c = 0; c < samples; ++c) {
                const int v = tfl::decode_diff(io, b, huff[d.td[c]]);
                if (v < 0) { rc = tfj::BAD_DATA; break; }
                must(v <= 0xFFFF, "a difference's value");
                diff[(size_t)c * hw + s] = (uint16_t)v;
            }
        free(data);
        if (rc) { free(diff); return rc; }
    }
    // the reconstruction, plane by plane from a copy of exactly the plane's size, row by row into a row of exactly W bytes
    bool ok = true;
    for (int c = 0; c < samples; ++c) {
        uint16_t* plane = (uint16_t*)malloc(hw * sizeof(uint16_t));
        memcpy(plane, diff + (size_t)c * hw, hw * sizeof(uint16_t));
        for (uint32_t k = 0; k < d.nint; ++k) {
            uint32_t r0, r1;
            tfl::interval_rows(d, k, &r0, &r1);
            tfl::restore_col(plane + (size_t)r0 * W, (size_t)W, r1 - r0);
        }
        uint8_t* row = (uint8_t*)malloc((size_t)W);
        for (int y = 0; y < H; ++y) {
            ok &= tfl::restore_row(plane + (size_t)y * W, (uint32_t)W, row, 1);
            for (int x = 0; x < W; ++x) out[((size_t)y * W + x) * samples + c] = row[x];
        }
        free(row); free(plane);
    }
    free(diff);
    return ok ? (int)tfj::OK : (int)tfj::BAD_DATA;
}

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: verify_jpegll corpus.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint32_t count = 0;
    if (!f || !read_exact(f, &count, 4)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int bad = 0;
    for (uint32_t c = 0; c < count; ++c) {
        uint32_t hd[5];
        if (!read_exact(f, hd, sizeof hd)) { fprintf(stderr, "case %u: truncated corpus\n", c); return 2; }
        const uint32_t H = hd[0], W = hd[1], samples = hd[2], len = hd[3], want_status = hd[4];
        const size_t out_bytes = (size_t)H * W * samples;
        uint8_t* frame = (uint8_t*)malloc(len);                            // (a frame of no bytes: no byte of it may be read)
        uint8_t* want = (uint8_t*)malloc(out_bytes);
        uint8_t* got = (uint8_t*)malloc(out_bytes);
        if (!read_exact(f, frame, len) || (want_status == 0 && !read_exact(f, want, out_bytes))) { fprintf(stderr, "case %u: truncated corpus\n", c); return 2; }
        const int status = decode_frame(frame, len, (int)H, (int)W, (int)samples, got);
        if (status != (int)want_status) { fprintf(stderr, "case %u: status %d, expected %u\n", c, status, want_status); ++bad; }
        else if (status == 0 && memcmp(got, want, out_bytes) != 0) { fprintf(stderr, "case %u: output differs\n", c); ++bad; }
        free(frame); free(want); free(got);
    }
    fclose(f);
    if (bad) { fprintf(stderr, "%d of %u cases failed\n", bad, count); return 1; }
    printf("%u cases ok\n", count);
    return 0;
}
