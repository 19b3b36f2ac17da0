// Prints the tables of tee_optical_flow_amd/csrc/pil_resample_tables.h for the size pairs on its command line, for
// tests/test_segmentor_glue_cpu.py to compare with the Python twins (tee_optical_flow_amd/masks.py).  Arguments, any number of:
//   b IN OUT   ->  "bilinear IN OUT KSIZE", then per output index one line "xmin n k[0] .. k[KSIZE-1]"
//   n IN OUT   ->  "nearest IN OUT", then one line of OUT source indices
// Exits 2 on a malformed command line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "pil_resample_tables.h"

int main(int argc, char** argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) return 2;
    for (int a = 1; a + 2 < argc; a += 3) {
        const int in = std::atoi(argv[a + 1]), out = std::atoi(argv[a + 2]);
        if (in < 1 || out < 1) return 2;
        if (!std::strcmp(argv[a], "b")) {
            int ksize = 0;
            std::vector<int> bounds, coeff;
            pil_bilinear_tables(in, out, ksize, bounds, coeff);
            if (ksize != pil_bilinear_ksize(in, out)) return 3;
            std::printf("bilinear %d %d %d\n", in, out, ksize);
            for (int xx = 0; xx < out; ++xx) {
                std::printf("%d %d", bounds[(size_t)xx * 2], bounds[(size_t)xx * 2 + 1]);
                for (int t = 0; t < ksize; ++t) std::printf(" %d", coeff[(size_t)xx * ksize + t]);
                std::printf("\n");
            }
        } else if (!std::strcmp(argv[a], "n")) {
            std::vector<int> idx;
            pil_nearest_table(in, out, idx);
            std::printf("nearest %d %d\n", in, out);
            for (int x = 0; x < out; ++x) std::printf(x ? " %d" : "%d", idx[(size_t)x]);
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
