// noise_host.cpp — izpi_host_noise: a progressive session's noise estimate on the host, the
// plain sequential form of the arithmetic in noise.h. It is the twin
// the device path (noise.hip) is tested against. No HIP here: a host compiler builds it alone.
#include <stdint.h>

#include <string>

#include "noise.h"

namespace izpi_internal {
void set_host_error(const std::string& s);
}

extern "C" int izpi_host_noise(const double* sums, const double* moment2, const uint8_t* counted, uint32_t num_pixels,
                               uint32_t done, uint32_t sampler, const izpi_noise_params* params, double* se_out,
                               izpi_noise_stats* out) {
  const izpi_noise_params p = params ? *params : nz::defaults();
  const char* bad = nz::check_params(p);
  if (!bad && (!sums || !moment2)) bad = "noise: sums and moment2 must be given";
  if (!bad && done < 2) bad = "noise: needs at least 2 samples";
  if (!bad && (sampler < IZPI_SAMPLER_NORMAL || sampler > IZPI_SAMPLER_SPECTRAL)) bad = "noise: unknown sampler";
  if (bad) {
    izpi_internal::set_host_error(bad);
    return IZPI_ERR_INVALID;
  }
  const bool spectral = sampler == IZPI_SAMPLER_SPECTRAL;
  izpi_noise_stats st{};
  st.done = done;
  for (uint64_t b0 = 0; b0 < num_pixels; b0 += nz::BLOCK) {
    double v[nz::BLOCK];
    for (uint32_t i = 0; i < nz::BLOCK; i++) {
      v[i] = 0.0;
      const uint64_t px = b0 + i;
      if (px >= num_pixels) continue;
      double se[3], e;
      const bool fin = nz::pixel(sums + 3 * px, moment2 + 3 * px, done, spectral, p.floor, se, &e);
      if (se_out) {
        double* o = se_out + 4 * px;
        o[0] = se[0]; o[1] = se[1]; o[2] = se[2]; o[3] = 1.0;
      }
      if (counted && !counted[px]) continue;
      st.pixels++;
      if (!fin) {
        st.nonfinite++;
        continue;
      }
      if (e > p.threshold) st.above++;
      if (e > st.max_error) st.max_error = e;
      v[i] = e;
    }
    for (uint32_t stride = nz::BLOCK / 2; stride; stride >>= 1)
      for (uint32_t i = 0; i < stride; i++) v[i] = v[i] + v[i + stride];
    st.sum_error = st.sum_error + v[0];
  }
  st.converged = nz::converged(st.pixels, st.nonfinite, st.above, done, p);
  if (out) *out = st;
  return IZPI_OK;
}

// izpi_host_adapt: one evaluation of the adaptive rule, the twin of
// k_adapt_select (adapt.hip) and of the integers the host adds up after it.
extern "C" int izpi_host_adapt(const double* sums, const double* moment2, const uint8_t* counted, const uint32_t* samples,
                               uint8_t* active, uint32_t num_pixels, uint32_t done, uint32_t sampler,
                               const izpi_noise_params* params, double* e_out, izpi_adapt_stats* out) {
  const izpi_noise_params p = params ? *params : nz::defaults();
  const char* bad = nz::check_params(p);
  if (!bad && (!sums || !moment2)) bad = "adapt: sums and moment2 must be given";
  if (!bad && (!samples || !active)) bad = "adapt: samples and active must be given";
  if (!bad && done < 2) bad = "adapt: needs at least 2 samples";
  if (!bad && (sampler != IZPI_SAMPLER_COLOUR && sampler != IZPI_SAMPLER_SPECTRAL)) bad = "adapt: the Colour or the Spectral sampler";
  if (bad) {
    izpi_internal::set_host_error(bad);
    return IZPI_ERR_INVALID;
  }
  const bool spectral = sampler == IZPI_SAMPLER_SPECTRAL;
  izpi_adapt_stats st{};
  st.done = done;
  for (uint64_t px = 0; px < num_pixels; px++) {
    const bool is_counted = !counted || counted[px];
    const uint32_t n = active[px] ? done : samples[px];
    double se[3], e = 0.0;
    const bool fin = n >= 2 ? nz::pixel(sums + 3 * px, moment2 + 3 * px, n, spectral, p.floor, se, &e) : true;
    if (e_out) e_out[px] = e;
    if (is_counted) {
      st.pixels++;
      if (!fin) st.nonfinite++;
    }
    st.samples += n;
    if (!active[px]) continue;
    if (nz::stays_active(is_counted, fin, e, p.threshold)) {
      st.active++;
    } else {
      active[px] = 0;
      st.retired++;
    }
  }
  st.converged = nz::converged(st.pixels, st.nonfinite, st.active, done, p);
  if (out) *out = st;
  return IZPI_OK;
}
