// denoise_host.cpp — izpi_host_denoise and izpi_host_denoise_var: the two a-trous denoisers
// on the host, the plain sequential form of the arithmetic in denoise.h (DESIGN.md sections
// 3.8, 3.8a and, for IZPI_DENOISE_DEMODULATE, 3.8b). It is the twin the device path (denoise.hip) is tested against. No HIP
// here: a host compiler builds it alone.
#include <stdint.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "denoise.h"

namespace izpi_internal {
void set_host_error(const std::string& s);
}

namespace {

template <bool HAS_N, bool HAS_A, class IT>
void pass(const double* C, const double* V, const double* Nm, const double* A, int64_t W, int64_t H, const IT& it, double* out,
          double* vout) {
  for (int64_t y = 0; y < H; y++)
    for (int64_t x = 0; x < W; x++) {
      const double v = dn::pixel<HAS_N, HAS_A>(C, V, Nm, A, W, H, x, y, it, out + (y * W + x) * 4);
      if constexpr (IT::kVar) vout[y * W + x] = v;
    }
}

template <bool VAR>
int filter(const double* colour, const double* se, const double* normal, const double* albedo, double* out, double* var_out,
           uint32_t width, uint32_t height, const izpi_denoise_params* params, double variance_floor) {
  const izpi_denoise_params p = params ? *params : dn::defaults(VAR);
  if (const char* bad = dn::check_args(VAR, colour, se, normal, albedo, out, var_out, width, height, p, variance_floor)) {
    izpi_internal::set_host_error(bad);
    return IZPI_ERR_INVALID;
  }
  try {
    const size_t pixels = (size_t)width * height, doubles = pixels * 4;
    // (VAR) two variance planes: iteration i reads plane i % 2 and writes the other
    std::vector<double> planes[2];
    if (VAR) {
      planes[0].resize(pixels);
      planes[1].resize(p.iterations ? pixels : 0);
    }
    // (IZPI_DENOISE_DEMODULATE) D_0, and V_0 of the demodulated standard errors with it
    const bool demod = dn::demodulates(p);
    std::vector<double> d0(demod ? doubles : 0);
    for (size_t q = 0; q < pixels && (VAR || demod); q++) {
      double v;
      if (demod) v = dn::demodulate<VAR>(colour + q * 4, VAR ? se + q * 4 : nullptr, albedo + q * 4, d0.data() + q * 4);
      else v = dn::variance0(se + q * 4);
      if (VAR) planes[0][q] = v;
    }
    if (p.iterations == 0) memcpy(out, colour, doubles * sizeof(double));
    // ping-pong between `out` and one scratch canvas so that the last iteration lands in `out`
    std::vector<double> scratch(p.iterations > 1 ? doubles : 0);
    const double* src = demod ? d0.data() : colour;
    for (uint32_t i = 0; i < p.iterations; i++) {
      double* dst = (p.iterations - 1 - i) % 2 == 0 ? out : scratch.data();
      const double* v = planes[i % 2].data();
      double* vdst = planes[(i + 1) % 2].data();
      const auto it = dn::iteration<VAR>(p, variance_floor, i);
      dn::with_guides(normal, albedo, [&](auto n, auto a) {
        pass<decltype(n)::value, decltype(a)::value>(src, v, normal, albedo, width, height, it, dst, vdst);
      });
      src = dst;
    }
    for (size_t q = 0; q < pixels && demod; q++)
      dn::remodulate<VAR>(colour + q * 4, VAR ? se + q * 4 : nullptr, albedo + q * 4, out + q * 4);
    if (VAR && var_out) memcpy(var_out, planes[p.iterations % 2].data(), pixels * sizeof(double));
    return IZPI_OK;
  } catch (const std::bad_alloc&) {
    izpi_internal::set_host_error("out of host memory");
    return IZPI_ERR_INVALID;
  }
}

}  // namespace

extern "C" int izpi_host_denoise(const double* colour, const double* normal, const double* albedo, double* out,
                                 uint32_t width, uint32_t height, const izpi_denoise_params* params) {
  return filter<false>(colour, nullptr, normal, albedo, out, nullptr, width, height, params, 0.0);
}

extern "C" int izpi_host_denoise_var(const double* colour, const double* stderr_host, const double* normal,
                                     const double* albedo, double* out, double* var_out, uint32_t width, uint32_t height,
                                     const izpi_denoise_params* params, double variance_floor) {
  return filter<true>(colour, stderr_host, normal, albedo, out, var_out, width, height, params, variance_floor);
}
