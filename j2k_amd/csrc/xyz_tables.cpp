// xyz_tables.cpp -- see xyz_tables.h.  Everything is computed in double and rounded to binary32 once.
#include "xyz_tables.h"

#include <cmath>

namespace j2k_hip {

bool xyz_tables_valid(uint32_t source, uint32_t src_depth, uint32_t dst_depth)
{
    return source >= 1 && source <= kXyzSources && src_depth >= 1 && src_depth <= 16 && dst_depth >= 1 && dst_depth <= 16;
}

static double eotf(uint32_t source, double x)
{
    if (source == 1) return x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4); // IEC 61966-2-1
    if (source == 2) return std::pow(x, 2.4);                                               // BT.1886 without black lift
    return x;
}

std::vector<float> xyz_lin_table(uint32_t source, uint32_t src_depth)
{
    const uint32_t n = 1u << src_depth;
    const double top = (double)(n - 1);
    std::vector<float> lin(n);
    for (uint32_t v = 0; v < n; ++v) lin[v] = (float)eotf(source, (double)v / top);
    return lin;
}

std::vector<float> xyz_thr_table(uint32_t dst_depth)
{
    const uint32_t top = (1u << dst_depth) - 1;
    std::vector<float> thr(top);
    for (uint32_t c = 1; c <= top; ++c) thr[c - 1] = (float)std::pow(((double)c - 0.5) / (double)top, 2.6);
    return thr;
}

void xyz_matrix(float M[9])
{
    static const double m[9] = {0.4124564, 0.3575761, 0.1804375, 0.2126729, 0.7151522, 0.0721750, 0.0193339, 0.1191920, 0.9503041};
    const double k = 48.0 / 52.37;
    for (int i = 0; i < 9; ++i) M[i] = (float)(m[i] * k);
}

bool xyz_inverse_valid(uint32_t target, uint32_t comp_depth, uint32_t dst_depth)
{
    return xyz_tables_valid(target, comp_depth, dst_depth); // (the same three codings, the same depths)
}

std::vector<float> xyz_delin_table(uint32_t comp_depth)
{
    const uint32_t n = 1u << comp_depth;
    const double top = (double)(n - 1);
    std::vector<float> dl(n);
    for (uint32_t c = 0; c < n; ++c) dl[c] = (float)std::pow((double)c / top, 2.6);
    return dl;
}

std::vector<float> xyz_othr_table(uint32_t target, uint32_t dst_depth)
{
    const uint32_t top = (1u << dst_depth) - 1;
    std::vector<float> othr(top);
    for (uint32_t k = 1; k <= top; ++k) othr[k - 1] = (float)eotf(target, ((double)k - 0.5) / (double)top);
    return othr;
}

void xyz_inverse_matrix(float N[9])
{
    static const double n[9] = {3.2404542, -1.5371385, -0.4985314, -0.9692660, 1.8760108, 0.0415560, 0.0556434, -0.2040259, 1.0572252};
    const double k = 52.37 / 48.0;
    for (int i = 0; i < 9; ++i) N[i] = (float)(n[i] * k);
}

uint32_t xyz_code(const float *thr, uint32_t n, float x)
{
    uint32_t lo = 0, hi = n; // thr[i] <= x for i < lo, thr[i] > x for i >= hi
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (thr[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

} // namespace j2k_hip
