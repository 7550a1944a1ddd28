// denoise_host.cpp — izpi_host_denoise: the edge-avoiding a-trous denoiser on the host, the
// plain sequential form of the arithmetic in denoise.h. It is the
// twin the device path (denoise.hip) is tested against. No HIP here: a host compiler builds
// it alone.
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

template <bool HAS_N, bool HAS_A>
void pass(const double* C, const double* Nm, const double* A, int64_t W, int64_t H, const dn::Iter& it, double* out) {
  for (int64_t y = 0; y < H; y++)
    for (int64_t x = 0; x < W; x++) dn::pixel<HAS_N, HAS_A>(C, Nm, A, W, H, x, y, it, out + (y * W + x) * 4);
}

}  // namespace

extern "C" int izpi_host_denoise(const double* colour, const double* normal, const double* albedo, double* out,
                                 uint32_t width, uint32_t height, const izpi_denoise_params* params) {
  const izpi_denoise_params p = params ? *params : dn::defaults();
  if (const char* bad = dn::check_args(colour, normal, albedo, out, width, height, p)) {
    izpi_internal::set_host_error(bad);
    return IZPI_ERR_INVALID;
  }
  try {
    const size_t doubles = (size_t)width * height * 4;
    if (p.iterations == 0) {
      memcpy(out, colour, doubles * sizeof(double));
      return IZPI_OK;
    }
    // ping-pong between `out` and one scratch canvas so that the last iteration lands in `out`
    std::vector<double> scratch(p.iterations > 1 ? doubles : 0);
    const double* src = colour;
    for (uint32_t i = 0; i < p.iterations; i++) {
      double* dst = (p.iterations - 1 - i) % 2 == 0 ? out : scratch.data();
      const dn::Iter it = dn::iteration(p, i);
      if (normal && albedo) pass<true, true>(src, normal, albedo, width, height, it, dst);
      else if (normal) pass<true, false>(src, normal, albedo, width, height, it, dst);
      else if (albedo) pass<false, true>(src, normal, albedo, width, height, it, dst);
      else pass<false, false>(src, normal, albedo, width, height, it, dst);
      src = dst;
    }
    return IZPI_OK;
  } catch (const std::bad_alloc&) {
    izpi_internal::set_host_error("out of host memory");
    return IZPI_ERR_INVALID;
  }
}
