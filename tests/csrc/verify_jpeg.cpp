// The JPEG Baseline core (tee_optical_flow_amd/csrc/teeflow_jpeg_core.h) and the libjpeg colour form of teeflow_ingest_core.h on the
// host, over the corpus of tests/jpeg_cases.py, every stream in a heap buffer of exactly its length, every restart interval's data in
// one of exactly its length, and the coefficients, component planes and output in buffers of exactly their size: built with
// -fsanitize=address,undefined by tests/test_jpeg_cpu.py, so that a read or write of one byte outside them ends the program.
//   verify_jpeg <corpus.bin>
// corpus.bin: uint32 count, then per case uint32 H, W, samples, len, status, the stream's len bytes and -- status 0 -- the
// H * W * samples bytes [H][W][samples] it decodes to.  Exit status 0: every status and every output is the expected one.
//   verify_jpeg color <in.bin> <out.bin> <n>: n pixels of Y, Cb, Cr -> RGB by tfg::ybr_libjpeg_pixel
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "teeflow_jpeg_core.h"
#include "teeflow_ingest_core.h"

static void must(bool ok, const char* what) { if (!ok) { fprintf(stderr, "the core broke its contract: %s\n", what); abort(); } }

// a restart interval's data bytes [pos, end) of the frame in a buffer of their own
struct HostIO {
    const uint8_t* data; uint32_t pos, end;
    uint8_t in_byte(uint32_t i) { must(i >= pos && i < end, "in_byte outside the interval"); return data[i - pos]; }
};

// one frame as the four kernels take it -> its status; out [H][W][samples] is written only for status 0
static int decode_frame(const uint8_t* frame, uint32_t len, int H, int W, int samples, uint8_t* out)
{
    tfj::Desc d;
    auto byte = [&](uint32_t i) -> uint8_t { must(i < len, "a byte past the frame"); return frame[i]; };
    int rc = tfj::parse_header(byte, len, H, W, samples, &d);
    if (rc) return rc;
    must(d.nint >= 1 && d.nint <= d.nmcu && d.scan_off <= len, "the descriptor");
    std::vector<uint32_t> rst(d.nint - 1);                                 // (exactly the positions k_jpeg_marks may write)
    uint32_t scan_end = 0;
    rc = tfj::find_marks(byte, len, d, rst.data(), &scan_end);
    if (rc) return rc;
    tfj::Huff huff[4];
    for (int t = 0; t < 4; ++t) tfj::huff_build(d.bits[t], d.vals[t], huff[t]);
    std::vector<int16_t> coef((size_t)d.nmcu * d.bpm * 64, 0);
    for (uint32_t k = 0; k < d.nint; ++k) {
        tfj::Bits b;
        b.acc = 0; b.cnt = 0; b.pad = 0;
        b.pos = k ? rst[k - 1] + 2 : d.scan_off;
        b.end = k + 1 < d.nint ? rst[k] : scan_end;
        must(b.pos <= b.end && b.end <= len, "an interval's bounds");
        uint8_t* data = (uint8_t*)malloc(b.end - b.pos);
        memcpy(data, frame + b.pos, b.end - b.pos);
        HostIO io{data, b.pos, b.end};
        const uint32_t m0 = d.ri ? k * d.ri : 0, m1 = d.ri && m0 + d.ri < d.nmcu ? m0 + d.ri : d.nmcu;
        int pred[3] = {0, 0, 0};
        for (uint32_t m = m0; m < m1 && rc == tfj::OK; ++m)
            for (int j = 0; j < d.bpm && rc == tfj::OK; ++j) {
                int c, bx, by;
                tfj::mcu_block(d, j, &c, &bx, &by);
                int16_t* blk = coef.data() + ((size_t)m * d.bpm + j) * 64;
                rc = tfj::decode_block(io, b, huff[d.td[c]], huff[2 + d.ta[c]], &pred[c], [&](int at, int v) {
                    must(at >= 0 && at < 64 && v >= -32768 && v <= 32767, "a coefficient's place or value");
                    blk[at] = (int16_t)v;
                });
            }
        free(data);
        if (rc) return rc;
    }
    // the component planes, each of exactly its MCU-padded size, end to end
    size_t at[4] = {0, 0, 0, 0}, total = 0;
    for (int c = 0; c < d.ncomp; ++c) {
        at[c] = total;
        total += (size_t)tfj::comp_pitch(d, c) * tfj::comp_rows(d, c);
    }
    uint8_t* planes = (uint8_t*)malloc(total);
    for (uint32_t bid = 0; bid < d.nmcu * d.bpm; ++bid) {
        int c, bx, by;
        tfj::mcu_block(d, (int)(bid % d.bpm), &c, &bx, &by);
        const uint32_t m = bid / d.bpm;
        const size_t pitch = (size_t)tfj::comp_pitch(d, c);
        const size_t x0 = ((size_t)(m % d.mcux) * d.h[c] + bx) * 8, y0 = ((size_t)(m / d.mcux) * d.v[c] + by) * 8;
        tfj::idct_block(coef.data() + (size_t)bid * 64, d.q[d.tq[c]], planes + at[c] + y0 * pitch + x0, pitch);
    }
    // component by component from a copy of exactly the component's size
    for (int c = 0; c < d.ncomp; ++c) {
        const size_t n = (size_t)tfj::comp_pitch(d, c) * tfj::comp_rows(d, c);
        uint8_t* one = (uint8_t*)malloc(n);
        memcpy(one, planes + at[c], n);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                out[((size_t)y * W + x) * samples + c] = tfj::frame_sample(d, one, 0, H, W, c, x, y);   // (stride 0: `one` is plane c)
        free(one);
    }
    free(planes);
    return tfj::OK;
}

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int color_main(char** argv)
{
    const size_t n = (size_t)atol(argv[4]);
    std::vector<uint8_t> in(3 * n), out(3 * n);
    FILE* f = fopen(argv[2], "rb");
    if (!f || !read_exact(f, in.data(), 3 * n)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    fclose(f);
    for (size_t i = 0; i < n; ++i) tfg::pixel<tfg::YBR_LIBJPEG>(in.data(), i, out.data() + 3 * i);
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 1, 3 * n, f) != 3 * n || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 5 && strcmp(argv[1], "color") == 0) return color_main(argv);
    if (argc != 2) { fprintf(stderr, "usage: verify_jpeg corpus.bin | verify_jpeg color in out n\n"); return 2; }
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
