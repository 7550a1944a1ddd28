// denoise_var.h — the arithmetic of the variance-guided a-trous denoiser (DESIGN.md section
// 3.8a), shared by the device path (denoise_var.hip) and its host twin (denoise_var_host.cpp)
// in the way denoise.h is: plain C++ or __host__ __device__, -ffp-contract=off, one rounding
// per operation on either side, the same bits. The project's own rule: the spatial filter of
// SVGF (Schied et al., HPG 2017, section 4.4) without its temporal part, over the per-pixel
// standard errors a noise session measures (section 3.9).
//
// Beside the canvas C ([H][W][4] float64) runs a variance plane V ([H][W] float64): V_0 is the
// squared length of the pixel's standard errors, and every iteration carries it along with
// the squared weights, so the colour term narrows by itself as the image gets smoother.
// One iteration reads C_i, V_i and the guides and writes C_{i+1}, V_{i+1}.
#pragma once
#include <stdint.h>

#include "denoise.h"

namespace dnv {

// The constants of an iteration: all but `step` are the same in every one (sigma_colour is
// not halved; the variance shrinks instead).
struct Iter {
  int64_t step;   // 1 << i
  double s2;      // sigma_colour * sigma_colour
  double floor;   // variance_floor
  double kn, ka;  // dn::Iter's
};
inline Iter iteration(const izpi_denoise_params& p, double variance_floor, uint32_t i) {
  const dn::Iter d = dn::iteration(p, 0);
  Iter it;
  it.step = (int64_t)1 << i;
  it.s2 = p.sigma_colour * p.sigma_colour;
  it.floor = variance_floor;
  it.kn = d.kn;
  it.ka = d.ka;
  return it;
}

inline izpi_denoise_params defaults() {
  izpi_denoise_params p = dn::defaults();
  p.sigma_colour = IZPI_DENOISE_VAR_DEFAULT_SIGMA_COLOUR;
  return p;
}

// Do [a, a + na) and [b, b + nb) share a byte?
inline bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? y - x < na : x - y < nb;
}

// The argument checks of all three entries: dn::check_args' over what the two filters share,
// then the standard errors, the variance output and the floor.
inline const char* check_args(const double* colour, const double* se, const double* normal, const double* albedo,
                              const double* out, const double* var_out, uint32_t width, uint32_t height,
                              const izpi_denoise_params& p, double variance_floor) {
  if (const char* bad = dn::check_args(colour, normal, albedo, out, width, height, p)) return bad;
  if (!se) return "denoise: the standard errors must be given";
  const uint64_t plane = (uint64_t)width * height * sizeof(double), bytes = 4 * plane;
  if (overlap(out, bytes, se, bytes)) return "denoise: out may not overlap an input canvas";
  if (var_out) {
    if (overlap(var_out, plane, out, bytes)) return "denoise: out may not overlap the variance output";
    if (overlap(var_out, plane, colour, bytes) || overlap(var_out, plane, se, bytes) ||
        (normal && overlap(var_out, plane, normal, bytes)) || (albedo && overlap(var_out, plane, albedo, bytes)))
      return "denoise: the variance output may not overlap an input canvas";
  }
  if (!(variance_floor > 0) || !dn::finite(variance_floor)) return "denoise: variance_floor must be finite and greater than 0";
  return nullptr;
}

// V_0 of a pixel from its standard errors (se_0, se_1, se_2, alpha ignored).
IZPI_HD double variance0(const double* s) { return (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]; }
// A pixel takes part when dn::live holds and its variance is a number that can be one.
IZPI_HD bool live(const double* px, double v) { return dn::live(px) && v >= 0 && dn::finite(v); }
// The 3-tap row {1/4, 1/2, 1/4} at offset d = -1..1.
IZPI_HD double k3(int d) { return d == 0 ? 1.0 / 2.0 : 1.0 / 4.0; }

// One pixel of one iteration: C, V, Nm, A are the whole canvases and the plane, o the pixel's
// four doubles in the output canvas, the return value V_{i+1} of the pixel.
template <bool HAS_N, bool HAS_A>
IZPI_HD double pixel(const double* C, const double* V, const double* Nm, const double* A, int64_t W, int64_t H, int64_t x,
                     int64_t y, const Iter& it, double* o) {
  const int64_t p = y * W + x, at = p * 4;
  const double c[4] = {C[at], C[at + 1], C[at + 2], C[at + 3]};
  const double v = V[p];
  o[3] = c[3];
  if (!live(c, v)) {
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    return v;
  }
  // the variance the colour term is measured in: V_i through a 3 x 3 kernel at unit spacing
  double gs = 0.0, gk = 0.0;
  for (int dy = -1; dy <= 1; dy++) {
    const int64_t qy = y + dy;
    if (qy < 0 || qy >= H) continue;
    for (int dx = -1; dx <= 1; dx++) {
      const int64_t qx = x + dx;
      if (qx < 0 || qx >= W) continue;
      const int64_t q = qy * W + qx;
      const double vq = V[q];
      if (!live(C + q * 4, vq)) continue;
      const double k = k3(dy) * k3(dx);
      gs += k * vq;
      gk += k;
    }
  }
  const double g = gs / gk;  // (the centre is live: gk >= 1/4)
  const double kc = 1.0 / (it.s2 * (g + it.floor));
  double n[3] = {0, 0, 0}, a[3] = {0, 0, 0};
  if (HAS_N) { n[0] = Nm[at]; n[1] = Nm[at + 1]; n[2] = Nm[at + 2]; }
  if (HAS_A) { a[0] = A[at]; a[1] = A[at + 1]; a[2] = A[at + 2]; }
  double sw = 0.0, sv = 0.0, sc[3] = {0.0, 0.0, 0.0};
  for (int dy = -2; dy <= 2; dy++) {
    const int64_t qy = y + it.step * dy;
    if (qy < 0 || qy >= H) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int64_t qx = x + it.step * dx;
      if (qx < 0 || qx >= W) continue;
      const int64_t qp = qy * W + qx, q = qp * 4;
      const double cq[4] = {C[q], C[q + 1], C[q + 2], C[q + 3]};
      const double vq = V[qp];
      if (!live(cq, vq)) continue;
      double e = dn::dist2(c, cq) * kc;
      if (HAS_N) e = e + dn::dist2(n, Nm + q) * it.kn;
      if (HAS_A) e = e + dn::dist2(a, A + q) * it.ka;
      if (!(e >= 0)) continue;  // NaN: a NaN in a guide, or Inf * 0
      const double w = (dn::b3(dy) * dn::b3(dx)) * gm::exp(-e);
      sw += w;
      sc[0] += w * cq[0];
      sc[1] += w * cq[1];
      sc[2] += w * cq[2];
      sv += (w * w) * vq;
    }
  }
  if (sw > 0) {
    o[0] = sc[0] / sw; o[1] = sc[1] / sw; o[2] = sc[2] / sw;
    return sv / (sw * sw);
  }
  o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
  return v;
}

}  // namespace dnv
