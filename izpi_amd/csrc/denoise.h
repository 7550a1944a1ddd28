// denoise.h — the arithmetic of the two a-trous denoisers, shared by the device path
// (denoise.hip) and its host twin (denoise_host.cpp): the fixed-sigma filter (DESIGN.md
// section 3.8; Dammertz, Sewtz, Hanika, Lensch, HPG 2010) and the variance-guided one
// (section 3.8a; the spatial filter of SVGF, Schied et al., HPG 2017, section 4.4, without
// its temporal part, over the per-pixel standard errors a noise session measures, section
// 3.9). Plain C++ when no HIP compiler is present, __host__ __device__ under hipcc; both are
// built with -ffp-contract=off, so every expression rounds once per operation on either side
// and the two give the same bits. The project's own rule, not a restatement of the reference.
//
// The two filters are one pixel rule, pixel(), instantiated by the type of its constants:
// dn::Iter for the fixed filter, dnv::Iter for the variance-guided one (`var` below).
//
// A canvas is Render's: [H][W][4] float64, R G B alpha. One iteration reads C_i and the
// guides and writes C_{i+1}; nothing is updated in place. The variance-guided filter runs a
// variance plane V ([H][W] float64) beside the canvas: V_0 is the squared length of the
// pixel's standard errors, and every iteration carries it along with the squared weights
// (it reads V_i and writes V_{i+1}), so the colour term narrows by itself as the image gets
// smoother.
//
// Albedo demodulation (IZPI_DENOISE_DEMODULATE; section 3.8b, deviation A29) is an option of
// both: demodulate() forms D_0 = C / m (and V_0 from S / m) ahead of iteration 0, the
// iterations above run on it unchanged, and remodulate() multiplies m back after the last.
// They are two passes of their own and pixel() knows nothing of them.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/izpi_host.h"
#include "gomath.h"

// The constants of iteration i, formed on the host and handed to the kernel as doubles.
namespace dn {
struct Iter {
  static constexpr bool kVar = false;
  int64_t step;       // 1 << i
  double kc, kn, ka;  // 1 / (sigma_colour / 2^i)^2, 1 / sigma_normal^2, 1 / sigma_albedo^2
};
}  // namespace dn
namespace dnv {
// All but `step` are the same in every iteration (sigma_colour is not halved; the variance
// shrinks instead).
struct Iter {
  static constexpr bool kVar = true;
  int64_t step;   // 1 << i
  double s2;      // sigma_colour * sigma_colour
  double floor;   // variance_floor
  double kn, ka;  // dn::Iter's
};
}  // namespace dnv

namespace dn {

template <bool VAR>
inline std::conditional_t<VAR, dnv::Iter, Iter> iteration(const izpi_denoise_params& p, double variance_floor, uint32_t i) {
  std::conditional_t<VAR, dnv::Iter, Iter> it;
  it.step = (int64_t)1 << i;
  if constexpr (VAR) {
    it.s2 = p.sigma_colour * p.sigma_colour;
    it.floor = variance_floor;
  } else {
    const double s = gm::ldexp(1.0, -(int)i);
    it.kc = 1.0 / ((p.sigma_colour * s) * (p.sigma_colour * s));
  }
  it.kn = 1.0 / (p.sigma_normal * p.sigma_normal);
  it.ka = 1.0 / (p.sigma_albedo * p.sigma_albedo);
  return it;
}

inline izpi_denoise_params defaults(bool var) {
  izpi_denoise_params p;
  p.iterations = IZPI_DENOISE_DEFAULT_ITERATIONS;
  p.flags = 0;
  p.sigma_colour = var ? IZPI_DENOISE_VAR_DEFAULT_SIGMA_COLOUR : IZPI_DENOISE_DEFAULT_SIGMA_COLOUR;
  p.sigma_normal = IZPI_DENOISE_DEFAULT_SIGMA_NORMAL;
  p.sigma_albedo = IZPI_DENOISE_DEFAULT_SIGMA_ALBEDO;
  return p;
}

// Do [a, a + na) and [b, b + nb) share a byte?
inline bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? y - x < na : x - y < nb;
}

IZPI_HD bool finite(double x) { return ((gm::bits(x) >> 52) & 0x7FFull) != 0x7FFull; }

// The argument checks of all six entries: the message of the first one that fails, or null.
// What the two filters share first, then (var) the standard errors, the variance output and
// the floor.
inline const char* check_args(bool var, const double* colour, const double* se, const double* normal, const double* albedo,
                              const double* out, const double* var_out, uint32_t width, uint32_t height,
                              const izpi_denoise_params& p, double variance_floor) {
  if (!colour || !out) return "denoise: colour and out must be given";
  if (width == 0 || height == 0) return "denoise: width and height must be at least 1";
  if ((uint64_t)width * height > (1ull << 40)) return "denoise: more than 2^40 pixels";
  const uint64_t plane = (uint64_t)width * height * sizeof(double), bytes = 4 * plane;
  if (overlap(out, bytes, colour, bytes) || (normal && overlap(out, bytes, normal, bytes)) ||
      (albedo && overlap(out, bytes, albedo, bytes)))
    return "denoise: out may not overlap an input canvas";
  if (p.iterations > IZPI_DENOISE_MAX_ITERATIONS) return "denoise: at most 8 iterations";
  if (p.flags != 0 && p.flags != IZPI_DENOISE_DEMODULATE) return "denoise: flags must be 0";
  if (p.flags && !albedo) return "denoise: demodulation needs the albedo canvas";
  if (!(p.sigma_colour > 0) || !(p.sigma_normal > 0) || !(p.sigma_albedo > 0))
    return "denoise: every sigma must be greater than 0 (+Inf drops its term)";
  if (!var) return nullptr;
  if (!se) return "denoise: the standard errors must be given";
  if (overlap(out, bytes, se, bytes)) return "denoise: out may not overlap an input canvas";
  if (var_out) {
    if (overlap(var_out, plane, out, bytes)) return "denoise: out may not overlap the variance output";
    if (overlap(var_out, plane, colour, bytes) || overlap(var_out, plane, se, bytes) ||
        (normal && overlap(var_out, plane, normal, bytes)) || (albedo && overlap(var_out, plane, albedo, bytes)))
      return "denoise: the variance output may not overlap an input canvas";
  }
  if (!(variance_floor > 0) || !finite(variance_floor)) return "denoise: variance_floor must be finite and greater than 0";
  return nullptr;
}

// f(std::bool_constant<HAS_N>, std::bool_constant<HAS_A>) for the guides that are given: the
// one place that picks among the four instances of a kernel or a host pass.
template <class F>
inline void with_guides(const double* normal, const double* albedo, F&& f) {
  if (normal && albedo) f(std::true_type{}, std::true_type{});
  else if (normal) f(std::true_type{}, std::false_type{});
  else if (albedo) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}

// V_0 of a pixel from its standard errors (se_0, se_1, se_2, alpha ignored).
IZPI_HD double variance0(const double* s) { return (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]; }
// A pixel takes part when something was written there (alpha) and its colour is a number,
// and (VAR) when its variance is a number that can be one.
template <bool VAR>
IZPI_HD bool live(const double* px, double v) {
  const bool colour = px[3] != 0 && finite(px[0]) && finite(px[1]) && finite(px[2]);
  if constexpr (VAR) return colour && v >= 0 && finite(v);
  return colour;
}
IZPI_HD double dist2(const double* a, const double* b) {
  const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// ---- albedo demodulation (IZPI_DENOISE_DEMODULATE)
// Do this call's iterations run on the demodulated canvas? (With no iteration the flag changes
// nothing: C is copied and V_0 is the colour's.)
inline bool demodulates(const izpi_denoise_params& p) { return (p.flags & IZPI_DENOISE_DEMODULATE) && p.iterations > 0; }
// m_k of an albedo channel: the albedo when it is a number above the floor, else the floor (a
// power of two, so a black, negative, NaN or Inf albedo divides and multiplies back exactly).
IZPI_HD double modulus(double a) { return finite(a) && a > IZPI_DENOISE_ALBEDO_FLOOR ? a : IZPI_DENOISE_ALBEDO_FLOOR; }
// D_0 of a pixel into d (four doubles) from its colour c, standard errors s (VAR; else not
// read: pass null) and albedo a: c / m when c is live, c as it is otherwise; alpha copied. The
// return value is (VAR) V_0, variance0 of s / m.
template <bool VAR>
IZPI_HD double demodulate(const double* c, const double* s, const double* a, double* d) {
  const double m[3] = {modulus(a[0]), modulus(a[1]), modulus(a[2])};
  const bool alive = live<false>(c, 0.0);
  for (int k = 0; k < 3; k++) d[k] = alive ? c[k] / m[k] : c[k];
  d[3] = c[3];
  if constexpr (VAR) {
    const double q[3] = {s[0] / m[0], s[1] / m[1], s[2] / m[2]};
    return variance0(q);
  }
  return 0.0;
}
// The pixel f of the last iteration's canvas back into colour, in place: f * m with the
// centre's alpha when the pixel was live in iteration 0 (D_0 live, which a quotient that
// overflowed is not, and (VAR) V_0 a number that can be a variance), else the input c, all
// four doubles. The predicate is formed again from c, s and a, which no entry changes.
template <bool VAR>
IZPI_HD void remodulate(const double* c, const double* s, const double* a, double* f) {
  double d[4];
  const double v = demodulate<VAR>(c, s, a, d);
  if (live<VAR>(d, v)) {
    for (int k = 0; k < 3; k++) f[k] = f[k] * modulus(a[k]);
    f[3] = c[3];
  } else {
    for (int k = 0; k < 4; k++) f[k] = c[k];
  }
}

// The B3-spline row h = {1/16, 1/4, 3/8, 1/4, 1/16} at offset d = -2..2 (no table: nothing
// is indexed at run time on the device), and the 3-tap row {1/4, 1/2, 1/4} at d = -1..1.
IZPI_HD double b3(int d) { return d == 0 ? 3.0 / 8.0 : ((d == 1 || d == -1) ? 1.0 / 4.0 : 1.0 / 16.0); }
IZPI_HD double k3(int d) { return d == 0 ? 1.0 / 2.0 : 1.0 / 4.0; }

// One pixel of one iteration: C, Nm, A are the whole canvases (guides as they are, their
// alpha ignored), o the pixel's four doubles in the output canvas. With a dnv::Iter, V is the
// variance plane and the return value V_{i+1} of the pixel; with a dn::Iter, V is not read
// (pass null) and the return value means nothing.
template <bool HAS_N, bool HAS_A, class IT>
IZPI_HD double pixel(const double* C, const double* V, const double* Nm, const double* A, int64_t W, int64_t H, int64_t x,
                     int64_t y, const IT& it, double* o) {
  constexpr bool VAR = IT::kVar;
  const int64_t p = y * W + x, at = p * 4;
  const double c[4] = {C[at], C[at + 1], C[at + 2], C[at + 3]};
  double v = 0.0;
  if constexpr (VAR) v = V[p];
  o[3] = c[3];
  if (!live<VAR>(c, v)) {
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    return v;
  }
  double kc;
  if constexpr (VAR) {
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
        if (!live<VAR>(C + q * 4, vq)) continue;
        const double k = k3(dy) * k3(dx);
        gs += k * vq;
        gk += k;
      }
    }
    const double g = gs / gk;  // (the centre is live: gk >= 1/4)
    kc = 1.0 / (it.s2 * (g + it.floor));
  } else {
    kc = it.kc;
  }
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
      double vq = 0.0;
      if constexpr (VAR) vq = V[qp];
      if (!live<VAR>(cq, vq)) continue;
      double e = dist2(c, cq) * kc;
      if (HAS_N) e = e + dist2(n, Nm + q) * it.kn;
      if (HAS_A) e = e + dist2(a, A + q) * it.ka;
      if (!(e >= 0)) continue;  // NaN: a NaN in a guide, or Inf * 0
      const double w = (b3(dy) * b3(dx)) * gm::exp(-e);
      sw += w;
      sc[0] += w * cq[0];
      sc[1] += w * cq[1];
      sc[2] += w * cq[2];
      if constexpr (VAR) sv += (w * w) * vq;
    }
  }
  if (sw > 0) {
    o[0] = sc[0] / sw; o[1] = sc[1] / sw; o[2] = sc[2] / sw;
    if constexpr (VAR) v = sv / (sw * sw);
    return v;
  }
  o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
  return v;
}

}  // namespace dn
