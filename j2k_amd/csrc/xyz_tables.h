// xyz_tables.h -- the tables of the cinema colour front end (j2k_hip_params.rgb_to_xyz; include/j2k_hip.h has the definition):
// source code -> linear light, the R G B -> X Y Z matrix scaled to 48 / 52.37, and the thresholds that decide the X'Y'Z' code.
// Host only, no HIP: the encoder uploads what these functions make, j2k_hip_xyz_tables hands out the same values, and the
// file is also built and run on its own (tests/native/xyz_sanitize.cpp).
#pragma once

#include <cstdint>
#include <vector>

namespace j2k_hip {

constexpr uint32_t kXyzSources = 3; // 1 sRGB, 2 Rec.709 primaries under a 2.4 power, 3 Rec.709 primaries in linear light

// Are these arguments ones that tables exist for?  source 1..3, depths 1..16.
bool xyz_tables_valid(uint32_t source, uint32_t src_depth, uint32_t dst_depth);
// lin[v] = (float)EOTF_source((double)v / (2^d - 1)), v = 0 .. 2^d - 1
std::vector<float> xyz_lin_table(uint32_t source, uint32_t src_depth);
// thr[c - 1] = (float)pow(((double)c - 0.5) / top, 2.6), c = 1 .. top = 2^depth - 1: strictly increasing
std::vector<float> xyz_thr_table(uint32_t dst_depth);
// M[3 * i + j] = (float)(m_ij * (48.0 / 52.37)), m = sRGB -> XYZ (D65), row i = X, Y, Z
void xyz_matrix(float M[9]);
// The code of a linear value: how many thresholds are <= x (0 .. n).  The definition the kernel's search has to equal.
uint32_t xyz_code(const float *thr, uint32_t n, float x);

// The way back, for the decode's RGBA output stage (j2k_hip_decode_set_xyz_to_rgb; include/j2k_hip.h has the definition):
// X'Y'Z' code -> linear light, the X Y Z -> R G B matrix scaled to 52.37 / 48, and the thresholds that decide the R'G'B' code of
// target 1..3 (the codings of `source` above).  j2k_hip_xyz_inverse_tables hands out the same values.
// target 1..3, depths 1..16
bool xyz_inverse_valid(uint32_t target, uint32_t comp_depth, uint32_t dst_depth);
// dl[c] = (float)pow((double)c / (2^P - 1), 2.6), c = 0 .. 2^P - 1
std::vector<float> xyz_delin_table(uint32_t comp_depth);
// othr[k - 1] = (float)EOTF_target(((double)k - 0.5) / top), k = 1 .. top = 2^depth - 1: strictly increasing
std::vector<float> xyz_othr_table(uint32_t target, uint32_t dst_depth);
// N[3 * i + j] = (float)(n_ij * (52.37 / 48.0)), n = XYZ -> linear Rec.709 (D65), row i = R, G, B
void xyz_inverse_matrix(float N[9]);

} // namespace j2k_hip
