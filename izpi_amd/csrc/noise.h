// noise.h — the arithmetic of a progressive session's noise estimate (DESIGN.md section 3.9,
// deviation A25), shared by the device path (noise.hip, and the fold in k_accumulate's
// moments instance, wavefront.hip) and the host twin (noise_host.cpp). Plain C++ when no HIP
// compiler is present, __host__ __device__ under hipcc; both are built with
// -ffp-contract=off, so every expression rounds once per operation on either side and the
// two give the same bits. The project's own rule: the reference has no such estimate.
//
// Per pixel the session keeps the sums s_c of its samples (what it always kept) and, with
// IZPI_PROG_NOISE, their second moments m2_c = m2_c + x_c * x_c, folded in sample order.
#pragma once
#include <stdint.h>

#include "../../include/izpi_host.h"
#include "gomath.h"

namespace nz {

constexpr uint32_t BLOCK = 256;  // pixels per block of sum_error's tree (k_noise_stats' block)

inline izpi_noise_params defaults() {
  izpi_noise_params p;
  p.threshold = IZPI_NOISE_DEFAULT_THRESHOLD;
  p.floor = IZPI_NOISE_DEFAULT_FLOOR;
  p.tolerated = IZPI_NOISE_DEFAULT_TOLERATED;
  p.min_spp = IZPI_NOISE_DEFAULT_MIN_SPP;
  p.flags = 0;
  return p;
}

IZPI_HD bool finite(double x) { return ((gm::bits(x) >> 52) & 0x7FFull) != 0x7FFull; }

// The parameter checks of every entry: the message of the first one that fails, or null.
inline const char* check_params(const izpi_noise_params& p) {
  if (!finite(p.threshold) || !(p.threshold > 0)) return "noise: threshold must be finite and greater than 0";
  if (!finite(p.floor) || !(p.floor > 0)) return "noise: floor must be finite and greater than 0";
  if (!(p.tolerated >= 0 && p.tolerated <= 1)) return "noise: tolerated must lie in [0, 1]";
  if (p.flags != 0) return "noise: flags must be 0";
  return nullptr;
}

// One sample into a pixel's second moments (the sums keep their own additions).
IZPI_HD void fold(double x0, double x1, double x2, double& q0, double& q1, double& q2) {
  q0 = q0 + x0 * x0; q1 = q1 + x1 * x1; q2 = q2 + x2 * x2;
}

// The standard error of the mean of one channel after n >= 2 samples.
IZPI_HD double std_error(double s, double m2, uint32_t n) {
  double v = (m2 - (s * s) / (double)n) / (double)(n - 1);
  if (!(v > 0)) v = 0;  // rounding below zero, and NaN
  return gm::sqrt(v / (double)n);
}

// One pixel after n >= 2 samples: se[3], the relative error e, and whether the pixel is
// non-finite (a sum, a moment or e is not a number). `spectral`: the canvas rule of the mean
// (sum * (1 / n), render/spectral.go:98-99; else col / n, rgb.go:38).
IZPI_HD bool pixel(const double s[3], const double m2[3], uint32_t n, bool spectral, double floor, double se[3], double* e) {
  double mean[3];
  if (!spectral) {
    mean[0] = s[0] / (double)n; mean[1] = s[1] / (double)n; mean[2] = s[2] / (double)n;
  } else {
    const double inv = 1.0 / (double)n;
    mean[0] = s[0] * inv; mean[1] = s[1] * inv; mean[2] = s[2] * inv;
  }
  se[0] = std_error(s[0], m2[0], n); se[1] = std_error(s[1], m2[1], n); se[2] = std_error(s[2], m2[2], n);
  *e = ((se[0] + se[1]) + se[2]) / (((gm::abs(mean[0]) + gm::abs(mean[1])) + gm::abs(mean[2])) + floor);
  return finite(s[0]) && finite(s[1]) && finite(s[2]) && finite(m2[0]) && finite(m2[1]) && finite(m2[2]) && finite(*e);
}

// Adaptive sampling (deviation A26): evaluated at n = done, an active
// pixel goes on taking samples iff it is counted (sample row y >= 1), finite and its e is above
// the threshold. Every other pixel retires for good with the samples it has: the uncounted
// never reach a canvas, and a non-finite pixel can never converge.
IZPI_HD bool stays_active(bool counted, bool fin, double e, double threshold) { return counted && fin && e > threshold; }

// The stop rule over the frame's integers (order-free, so every share plan decides alike).
inline uint32_t converged(uint64_t pixels, uint64_t nonfinite, uint64_t above, uint32_t done, const izpi_noise_params& p) {
  return done >= p.min_spp && (double)above <= p.tolerated * (double)(pixels - nonfinite) ? 1u : 0u;
}

}  // namespace nz
