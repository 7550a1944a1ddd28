// resolve.hip — k_resolve: a snapshot of a progressive session's running sums
// (izpi_gpu_progressive_snapshot, include/izpi_gpu.h). What k_accumulate's last chunk does to
// the sums of a one-shot render (shade.h), without consuming them: divide by the samples done
// and write the pixel, packed or into the canvas. A translation unit of its own, so the
// shading units compile what they compiled before.
#include "izpi_runtime.h"

// One thread per pixel in packed order: 24 B of sums in, 32 B out; HBM-streaming. The sums
// are read only.
//  IZPI_SNAP_CANVAS:  the sampler's mean of the sums (pixel_mean, pixel_map.h) after the
//    pixel's samples (an adaptive session after its first retirement: its own count); alpha 1.0.
//  IZPI_SNAP_DISPLAY: the pixel display.DisplayTile shows (rgb.go:43-51, spectral.go:38-46):
//    B, G, R, 1.0; for Spectral XYZToACEScg of (X, Y, Z) * exposure (rgb_image.go:13-22), each
//    row (m0 * x + m1 * y) + m2 * z in that order.
//  IZPI_SNAP_SAMPLES (an adaptive session): (n, n, n, 1.0), n the pixel's sample count.
__global__ void __launch_bounds__(256) k_resolve(const ResolveParams rp) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  const SessionView& v = rp.view;
  if (p >= v.map.num_pixels) return;
  const double c0 = v.running[3 * (size_t)p], c1 = v.running[3 * (size_t)p + 1], c2 = v.running[3 * (size_t)p + 2];
  const uint32_t n = v.n(p);
  double r0, r1, r2;
  if (rp.form == IZPI_SNAP_SAMPLES) {  // the sample-count map
    r0 = r1 = r2 = (double)n;
  } else {
    r0 = pixel_mean(v.sampler, c0, n); r1 = pixel_mean(v.sampler, c1, n); r2 = pixel_mean(v.sampler, c2, n);
  }
  if (rp.form == IZPI_SNAP_DISPLAY) {
    if (v.sampler == IZPI_SAMPLER_SPECTRAL) {
      const double X = r0 * rp.exposure, Y = r1 * rp.exposure, Z = r2 * rp.exposure;
      r0 = 1.6410234 * X + -0.3248033 * Y + -0.2364247 * Z;
      r1 = -0.6636629 * X + 1.6153316 * Y + 0.0167563 * Z;
      r2 = 0.0117219 * X + -0.0082845 * Y + 0.9883949 * Z;
    }
    const double t = r0;  // R, G, B -> B, G, R
    r0 = r2; r2 = t;
  }
  store_pixel(v.map, p, rp.out, r0, r1, r2);
}

void launch_resolve(hipStream_t st, const ResolveParams& rp) {
  hipLaunchKernelGGL(k_resolve, dim3((rp.view.map.num_pixels + 255) / 256), dim3(256), 0, st, rp);
}
