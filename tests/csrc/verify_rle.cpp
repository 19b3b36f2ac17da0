// The RLE Lossless core (tee_optical_flow_amd/csrc/teeflow_rle_core.h) and the planar ingest (teeflow_ingest_core.h) on the host, over the
// corpus of tests/rle_cases.py, every frame in a heap buffer of exactly its length and every output in one of exactly its size: built
// with -fsanitize=address,undefined by tests/test_rle_cpu.py, so that a read or write of one byte outside them ends the program.
//   verify_rle <corpus.bin>
// corpus.bin: uint32 count, then per case uint32 H, W, samples, len, status, the frame's len bytes and -- status 0 -- the
// H * W * samples bytes [H][W][samples] it decodes to.  Exit status 0: every status and every output is the expected one.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "teeflow_rle_core.h"
#include "teeflow_ingest_core.h"

// the core's IO on plain memory: segment [seg, seg + n_in) -> plane [out, out + plane); what the core may ask for is asserted, and
// the sanitizers see every byte it touches
struct HostIO {
    const uint8_t* seg; uint32_t n_in; uint8_t* out; uint32_t plane;
    static void must(bool ok, const char* what) { if (!ok) { fprintf(stderr, "the core broke its contract: %s\n", what); abort(); } }
    uint8_t in_byte(uint32_t i) { must(i < n_in, "in_byte past the segment"); return seg[i]; }
    void literal(uint32_t pos, uint32_t made, uint32_t cnt)
    {
        must(pos <= n_in && cnt <= n_in - pos && made <= plane && cnt <= plane - made, "literal outside the segment or the plane");
        for (uint32_t k = 0; k < cnt; ++k) out[made + k] = seg[pos + k];
    }
    void run(uint32_t made, uint8_t v, uint32_t cnt)
    {
        must(made <= plane && cnt <= plane - made, "run outside the plane");
        for (uint32_t k = 0; k < cnt; ++k) out[made + k] = v;
    }
};

// one frame as k_rle_decode's waves take it: segment by segment into [samples][plane], the frame's status the largest of theirs
static int decode_frame(const uint8_t* frame, uint32_t len, int samples, uint32_t plane, uint8_t* planes)
{
    int status = 0;
    auto byte = [&](uint32_t i) -> uint8_t { HostIO::must(i < len, "header byte past the frame"); return frame[i]; };
    for (int k = 0; k < samples; ++k) {
        uint32_t s0 = 0, s1 = 0;
        int rc = tfr::frame_segment(byte, len, samples, k, &s0, &s1);
        if (rc == tfr::OK) {
            HostIO::must(s0 >= 64 && s0 < s1 && s1 <= len, "segment bounds");
            uint8_t* seg = (uint8_t*)malloc(s1 - s0);          // (its own exact buffer: a read past the segment's end is caught even inside the frame)
            memcpy(seg, frame + s0, s1 - s0);
            HostIO io{seg, s1 - s0, planes + (size_t)k * plane, plane};
            rc = tfr::decode_segment(io, s1 - s0, plane);
            free(seg);
        }
        if (rc > status) status = rc;
    }
    return status;
}

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

template <int FORM, bool FLIP>
static void run_planar(const uint8_t* src, size_t npx, int W, size_t hw, uint8_t* out)
{
    const size_t lanes = (npx + 3) / 4, grid = (lanes + 255) / 256 * 256;
    for (size_t lane = 0; lane < grid; ++lane) tfg::ingest_lane<FORM, FLIP, true>(src, npx, W, lane, out, hw);
}

// verify_rle planar <in.bin> <out.bin> <form 0|2> <flip 0|1> <N> <H> <W>: sample planes [N][3][H * W] -> uint8 RGB [N][H][W][3]
static int planar_main(char** argv)
{
    const int form = atoi(argv[4]), flip = atoi(argv[5]), N = atoi(argv[6]), H = atoi(argv[7]), W = atoi(argv[8]);
    if ((form != tfg::RGB && form != tfg::YBR_FULL) || N < 1 || H < 1 || W < 1) { fprintf(stderr, "bad arguments\n"); return 2; }
    const size_t hw = (size_t)H * W, npx = (size_t)N * hw, bytes = npx * 3;
    uint8_t* src = (uint8_t*)malloc(bytes);
    uint8_t* out = (uint8_t*)malloc(bytes);
    FILE* f = fopen(argv[2], "rb");
    if (!src || !out || !f || !read_exact(f, src, bytes)) { fprintf(stderr, "cannot read %zu bytes of %s\n", bytes, argv[2]); return 2; }
    fclose(f);
    if (form == tfg::YBR_FULL) flip ? run_planar<tfg::YBR_FULL, true>(src, npx, W, hw, out) : run_planar<tfg::YBR_FULL, false>(src, npx, W, hw, out);
    else flip ? run_planar<tfg::RGB, true>(src, npx, W, hw, out) : run_planar<tfg::RGB, false>(src, npx, W, hw, out);
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out, 1, bytes, f) != bytes || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    free(src);
    free(out);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 9 && strcmp(argv[1], "planar") == 0) return planar_main(argv);
    if (argc != 2) { fprintf(stderr, "usage: verify_rle corpus.bin | verify_rle planar in out form flip N H W\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint32_t count = 0;
    if (!f || !read_exact(f, &count, 4)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int bad = 0;
    for (uint32_t c = 0; c < count; ++c) {
        uint32_t hd[5];
        if (!read_exact(f, hd, sizeof hd)) { fprintf(stderr, "case %u: truncated corpus\n", c); return 2; }
        const uint32_t H = hd[0], W = hd[1], samples = hd[2], len = hd[3], want_status = hd[4];
        const size_t plane = (size_t)H * W, out_bytes = plane * samples;
        uint8_t* frame = (uint8_t*)malloc(len ? len : 1);
        uint8_t* want = (uint8_t*)malloc(out_bytes);
        uint8_t* planes = (uint8_t*)malloc(out_bytes);
        uint8_t* got = (uint8_t*)malloc(out_bytes);
        if (len == 0) { free(frame); frame = (uint8_t*)malloc(0); }   // (a frame of no bytes: no byte of it may be read)
        if (!read_exact(f, frame, len) || (want_status == 0 && !read_exact(f, want, out_bytes))) { fprintf(stderr, "case %u: truncated corpus\n", c); return 2; }
        const int status = decode_frame(frame, len, (int)samples, (uint32_t)plane, planes);
        if (status != (int)want_status) { fprintf(stderr, "case %u: status %d, expected %u\n", c, status, want_status); ++bad; }
        else if (status == 0) {
            if (samples == 1) memcpy(got, planes, out_bytes);
            else {                                               // the interleave, lane by lane as k_ingest_planar runs it, idle lanes included
                const size_t lanes = (plane + 3) / 4, grid = (lanes + 255) / 256 * 256;
                for (size_t lane = 0; lane < grid; ++lane) tfg::ingest_lane<tfg::RGB, false, true>(planes, plane, (int)W, lane, got, plane);
            }
            if (memcmp(got, want, out_bytes) != 0) { fprintf(stderr, "case %u: output differs\n", c); ++bad; }
        }
        free(frame); free(want); free(planes); free(got);
    }
    fclose(f);
    if (bad) { fprintf(stderr, "%d of %u cases failed\n", bad, count); return 1; }
    printf("%u cases ok\n", count);
    return 0;
}
