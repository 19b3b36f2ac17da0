// The frame ingest's core (tee_optical_flow_amd/csrc/teeflow_ingest_core.h) on the host, lane by lane as k_ingest runs it, with source
// and output buffers of exactly the study's size: built with -fsanitize=address,undefined by tests/test_frames_cpu.py, so that a lane
// that reads or writes one byte outside them, or a misaligned dword access, ends the program.
//   verify_ingest <in.bin> <out.bin> <form 0|1|2> <flip 0|1> <N> <H> <W>
// in.bin: the source bytes as stored ([N][H][W] or [N][H][W][3]); out.bin: uint8 RGB [N][H][W][3].
#include <stdio.h>
#include <stdlib.h>
#include "teeflow_ingest_core.h"

template <int FORM, bool FLIP>
static void run(const uint8_t* src, size_t npx, int W, uint8_t* out)
{
    const size_t lanes = (npx + 3) / 4, grid = (lanes + 255) / 256 * 256;   // the launch's lanes, the idle ones of its last block included
    for (size_t lane = 0; lane < grid; ++lane) tfg::ingest_lane<FORM, FLIP>(src, npx, W, lane, out);
}

int main(int argc, char** argv)
{
    if (argc != 8) { fprintf(stderr, "usage: verify_ingest in out form flip N H W\n"); return 2; }
    const int form = atoi(argv[3]), flip = atoi(argv[4]), N = atoi(argv[5]), H = atoi(argv[6]), W = atoi(argv[7]);
    if (form < 0 || form > 2 || N < 1 || H < 1 || W < 1) { fprintf(stderr, "bad arguments\n"); return 2; }
    const size_t npx = (size_t)N * H * W, in_bytes = npx * tfg::src_channels(form), out_bytes = npx * 3;
    uint8_t* src = (uint8_t*)malloc(in_bytes);
    uint8_t* out = (uint8_t*)malloc(out_bytes);
    if (!src || !out) { fprintf(stderr, "out of memory\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(src, 1, in_bytes, f) != in_bytes) { fprintf(stderr, "cannot read %zu bytes of %s\n", in_bytes, argv[1]); return 2; }
    fclose(f);
    if (form == tfg::GRAY) flip ? run<tfg::GRAY, true>(src, npx, W, out) : run<tfg::GRAY, false>(src, npx, W, out);
    else if (form == tfg::YBR_FULL) flip ? run<tfg::YBR_FULL, true>(src, npx, W, out) : run<tfg::YBR_FULL, false>(src, npx, W, out);
    else flip ? run<tfg::RGB, true>(src, npx, W, out) : run<tfg::RGB, false>(src, npx, W, out);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out, 1, out_bytes, f) != out_bytes || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    free(src);
    free(out);
    return 0;
}
