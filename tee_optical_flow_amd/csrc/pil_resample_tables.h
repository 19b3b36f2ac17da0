// pil_resample_tables.h -- the tables PIL's Image.resize works from, in plain C++ (no HIP): what the segmentor glue's kernels
// (teeflow_segmentor.hip.h) gather with.  Double arithmetic in PIL's own order, so the tables -- and with integer kernels the
// results -- are PIL's bit for bit.  Shared between the library and tests/csrc/verify_resample_tables.cpp, which prints them for
// the Python twins (tee_optical_flow_amd/masks.py: pil_bilinear_coeffs, pil_nearest_index) to be compared with.
//
// resize(size, BILINEAR) on a uint8 image is two passes, horizontal then vertical, with a uint8 image between them.  Per axis, for
// `in` samples to `out` samples, output xx is  clip((2^21 + sum_t pixel[xmin + t] * k[t]) >> 22, 0, 255)  over n taps, with
//   scale = in / out, fs = max(scale, 1), support = fs, ksize = (int)ceil(support) * 2 + 1 (the row length of the coefficient table)
//   center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0), n = min((int)(center + support + 0.5), in) - xmin
//   w[t] = max(0, 1 - |(t + xmin - center + 0.5) / fs|), normalised by their sum in tap order, k[t] = (int)(0.5 + w[t] * 2^22)
// A pass with in == out has the single coefficient 2^22: it changes nothing, PIL skips it, running it is exact.
// resize(size, NEAREST): a = in / out, xo = a * 0.5, and for each output index in turn source (int)xo, then xo += a -- a running
// double sum, not a product.
#ifndef TEEFLOW_PIL_RESAMPLE_TABLES_H
#define TEEFLOW_PIL_RESAMPLE_TABLES_H

#include <cmath>
#include <vector>

constexpr int PIL_PRECISION_BITS = 32 - 8 - 2;

inline int pil_bilinear_ksize(int in, int out)
{
    const double scale = (double)in / out;
    const double support = scale < 1.0 ? 1.0 : scale;
    return (int)std::ceil(support) * 2 + 1;
}

// bounds: [out][2] = (first source index, taps); coeff: [out][ksize] fixed-point coefficients, zero behind a row's taps
inline void pil_bilinear_tables(int in, int out, int& ksize, std::vector<int>& bounds, std::vector<int>& coeff)
{
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs;
    ksize = (int)std::ceil(support) * 2 + 1;
    bounds.assign((size_t)out * 2, 0);
    coeff.assign((size_t)out * ksize, 0);
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            double a = (x + xmin - center + 0.5) / fs;
            if (a < 0.0) a = -a;
            w[x] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[x];
        }
        for (int x = 0; x < n; ++x) {
            if (ww != 0.0) w[x] /= ww;
            coeff[(size_t)xx * ksize + x] = (int)(0.5 + w[x] * (double)(1 << PIL_PRECISION_BITS));
        }
        bounds[(size_t)xx * 2] = xmin;
        bounds[(size_t)xx * 2 + 1] = n;
    }
}

// idx: [out] source index of each output index, clamped to in - 1 (it never exceeded that in the checks; a gather stays in bounds)
inline void pil_nearest_table(int in, int out, std::vector<int>& idx)
{
    idx.assign((size_t)out, 0);
    const double a = (double)in / out;
    double xo = a * 0.5;
    for (int x = 0; x < out; ++x) {
        int s = (int)xo;
        if (s > in - 1) s = in - 1;
        idx[(size_t)x] = s;
        xo += a;
    }
}

#endif
