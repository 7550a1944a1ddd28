// denoise.h — the arithmetic of the edge-avoiding a-trous denoiser,
// shared by the device path (denoise.hip) and its host twin (denoise_host.cpp). Plain C++
// when no HIP compiler is present, __host__ __device__ under hipcc; both are built with
// -ffp-contract=off, so every expression rounds once per operation on either side and the
// two give the same bits. The project's own rule (Dammertz, Sewtz, Hanika, Lensch, HPG
// 2010), not a restatement of the reference.
//
// A canvas is Render's: [H][W][4] float64, R G B alpha. One iteration reads C_i and the
// guides and writes C_{i+1}; nothing is updated in place.
#pragma once
#include <stdint.h>

#include "../../include/izpi_host.h"
#include "gomath.h"

namespace dn {

// The constants of iteration i, formed on the host and handed to the kernel as doubles.
struct Iter {
  int64_t step;       // 1 << i
  double kc, kn, ka;  // 1 / (sigma_colour / 2^i)^2, 1 / sigma_normal^2, 1 / sigma_albedo^2
};
inline Iter iteration(const izpi_denoise_params& p, uint32_t i) {
  Iter it;
  it.step = (int64_t)1 << i;
  const double s = gm::ldexp(1.0, -(int)i);
  it.kc = 1.0 / ((p.sigma_colour * s) * (p.sigma_colour * s));
  it.kn = 1.0 / (p.sigma_normal * p.sigma_normal);
  it.ka = 1.0 / (p.sigma_albedo * p.sigma_albedo);
  return it;
}

inline izpi_denoise_params defaults() {
  izpi_denoise_params p;
  p.iterations = IZPI_DENOISE_DEFAULT_ITERATIONS;
  p.flags = 0;
  p.sigma_colour = IZPI_DENOISE_DEFAULT_SIGMA_COLOUR;
  p.sigma_normal = IZPI_DENOISE_DEFAULT_SIGMA_NORMAL;
  p.sigma_albedo = IZPI_DENOISE_DEFAULT_SIGMA_ALBEDO;
  return p;
}

// Do [a, a + bytes) and [b, b + bytes) share a byte?
inline bool overlap(const void* a, const void* b, uint64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? y - x < bytes : x - y < bytes;
}

// The argument checks of all three entries: the message of the first one that fails, or null.
inline const char* check_args(const double* colour, const double* normal, const double* albedo, const double* out,
                              uint32_t width, uint32_t height, const izpi_denoise_params& p) {
  if (!colour || !out) return "denoise: colour and out must be given";
  if (width == 0 || height == 0) return "denoise: width and height must be at least 1";
  if ((uint64_t)width * height > (1ull << 40)) return "denoise: more than 2^40 pixels";
  const uint64_t bytes = (uint64_t)width * height * 4 * sizeof(double);
  if (overlap(out, colour, bytes) || (normal && overlap(out, normal, bytes)) || (albedo && overlap(out, albedo, bytes)))
    return "denoise: out may not overlap an input canvas";
  if (p.iterations > IZPI_DENOISE_MAX_ITERATIONS) return "denoise: at most 8 iterations";
  if (p.flags != 0) return "denoise: flags must be 0";
  if (!(p.sigma_colour > 0) || !(p.sigma_normal > 0) || !(p.sigma_albedo > 0))
    return "denoise: every sigma must be greater than 0 (+Inf drops its term)";
  return nullptr;
}

IZPI_HD bool finite(double x) { return ((gm::bits(x) >> 52) & 0x7FFull) != 0x7FFull; }
// A pixel takes part when something was written there (alpha) and its colour is a number.
IZPI_HD bool live(const double* px) { return px[3] != 0 && finite(px[0]) && finite(px[1]) && finite(px[2]); }
IZPI_HD double dist2(const double* a, const double* b) {
  const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// The B3-spline row h = {1/16, 1/4, 3/8, 1/4, 1/16} at offset d = -2..2 (no table: nothing
// is indexed at run time on the device).
IZPI_HD double b3(int d) { return d == 0 ? 3.0 / 8.0 : ((d == 1 || d == -1) ? 1.0 / 4.0 : 1.0 / 16.0); }

// One pixel of one iteration: C, Nm, A are the whole canvases (guides as they are, their
// alpha ignored), o the pixel's four doubles in the output canvas.
template <bool HAS_N, bool HAS_A>
IZPI_HD void pixel(const double* C, const double* Nm, const double* A, int64_t W, int64_t H, int64_t x, int64_t y,
                   const Iter& it, double* o) {
  const int64_t at = (y * W + x) * 4;
  const double c[4] = {C[at], C[at + 1], C[at + 2], C[at + 3]};
  o[3] = c[3];
  if (!live(c)) {
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    return;
  }
  double n[3] = {0, 0, 0}, a[3] = {0, 0, 0};
  if (HAS_N) { n[0] = Nm[at]; n[1] = Nm[at + 1]; n[2] = Nm[at + 2]; }
  if (HAS_A) { a[0] = A[at]; a[1] = A[at + 1]; a[2] = A[at + 2]; }
  double sw = 0.0, sc[3] = {0.0, 0.0, 0.0};
  for (int dy = -2; dy <= 2; dy++) {
    const int64_t qy = y + it.step * dy;
    if (qy < 0 || qy >= H) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int64_t qx = x + it.step * dx;
      if (qx < 0 || qx >= W) continue;
      const int64_t q = (qy * W + qx) * 4;
      const double cq[4] = {C[q], C[q + 1], C[q + 2], C[q + 3]};
      if (!live(cq)) continue;
      double e = dist2(c, cq) * it.kc;
      if (HAS_N) e = e + dist2(n, Nm + q) * it.kn;
      if (HAS_A) e = e + dist2(a, A + q) * it.ka;
      if (!(e >= 0)) continue;  // NaN: a NaN in a guide, or Inf * 0
      const double w = (b3(dy) * b3(dx)) * gm::exp(-e);
      sw += w;
      sc[0] += w * cq[0];
      sc[1] += w * cq[1];
      sc[2] += w * cq[2];
    }
  }
  if (sw > 0) {
    o[0] = sc[0] / sw; o[1] = sc[1] / sw; o[2] = sc[2] / sw;
  } else {
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
  }
}

}  // namespace dn
