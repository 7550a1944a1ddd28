// resolve.hip — k_resolve: a snapshot of a progressive session's running sums
// (izpi_gpu_progressive_snapshot, include/izpi_gpu.h). What k_accumulate's last chunk does to
// the sums of a one-shot render (shade.h), without consuming them: divide by the samples done
// and write the pixel, packed or into the canvas. A translation unit of its own, so the
// shading units compile what they compiled before.
#include "izpi_runtime.h"

// One thread per pixel in packed order: 24 B of sums in, 32 B out; HBM-streaming. The sums
// are read only.
//  IZPI_SNAP_CANVAS:  Colour (and the preview samplers, which render under rgb.go's loop)
//    col / numSamples (rgb.go:38); Spectral sum * (1 / numSamples) (render/spectral.go:98-99);
//    alpha 1.0.
//  IZPI_SNAP_DISPLAY: the pixel display.DisplayTile shows (rgb.go:43-51, spectral.go:38-46):
//    B, G, R, 1.0; for Spectral XYZToACEScg of (X, Y, Z) * exposure (rgb_image.go:13-22), each
//    row (m0 * x + m1 * y) + m2 * z in that order.
//  IZPI_SNAP_SAMPLES (an adaptive session): (n, n, n, 1.0), n the pixel's sample count.
__global__ void __launch_bounds__(256) k_resolve(const ResolveParams rp) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= rp.num_pixels) return;
  const double c0 = rp.running[3 * (size_t)p], c1 = rp.running[3 * (size_t)p + 1], c2 = rp.running[3 * (size_t)p + 2];
  // (an adaptive session after its first retirement: the pixel's own sample count)
  const uint32_t n = rp.counts ? rp.counts[p] : rp.done;
  double r0, r1, r2;
  if (rp.form == IZPI_SNAP_SAMPLES) {  // the sample-count map
    r0 = r1 = r2 = (double)n;
  } else if (rp.sampler != IZPI_SAMPLER_SPECTRAL) {  // vec3.ScalarDiv(col, numSamples)
    r0 = c0 / (double)n; r1 = c1 / (double)n; r2 = c2 / (double)n;
  } else {  // sum * (1/numSamples)
    const double inv = 1.0 / (double)n;
    r0 = c0 * inv; r1 = c1 * inv; r2 = c2 * inv;
  }
  if (rp.form == IZPI_SNAP_DISPLAY) {
    if (rp.sampler == IZPI_SAMPLER_SPECTRAL) {
      const double X = r0 * rp.exposure, Y = r1 * rp.exposure, Z = r2 * rp.exposure;
      r0 = 1.6410234 * X + -0.3248033 * Y + -0.2364247 * Z;
      r1 = -0.6636629 * X + 1.6153316 * Y + 0.0167563 * Z;
      r2 = 0.0117219 * X + -0.0082845 * Y + 0.9883949 * Z;
    }
    const double t = r0;  // R, G, B -> B, G, R
    r0 = r2; r2 = t;
  }
  double* o;
  if (rp.out_layout == IZPI_OUT_PACKED) {
    o = rp.out + (size_t)p * 4;
  } else {  // k_accumulate's rule: canvas.Set(x, ny - y), row ny is dropped (A9)
    const uint32_t tile_px = rp.tile_w * rp.tile_h;
    const uint32_t tile = p / tile_px, in_tile = p % tile_px;
    const uint32_t x = rp.tiles[4 * tile] + in_tile % rp.tile_w;
    const uint32_t y = rp.tiles[4 * tile + 1] + in_tile / rp.tile_w;
    const uint32_t row = rp.height - y;
    if (row >= rp.height) return;
    o = rp.out + ((size_t)row * rp.width + x) * 4;
  }
  o[0] = r0; o[1] = r1; o[2] = r2; o[3] = 1.0;  // (a caller's device buffer: 8-B aligned is all it need be)
}

void launch_resolve(hipStream_t st, const ResolveParams& rp) {
  hipLaunchKernelGGL(k_resolve, dim3((rp.num_pixels + 255) / 256), dim3(256), 0, st, rp);
}
