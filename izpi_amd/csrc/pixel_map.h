// pixel_map.h — where the pixels of a request lie and how their sums become a mean: the one
// home of the packed-pixel rule, of the canvas slot and of the choice between col / n and
// sum * (1 / n). Every kernel that walks a request's pixels in packed order (k_accumulate,
// k_resolve, the noise and adapt kernels, k_unpack) and the host's assembly of the shares
// (izpi_host_assemble_shares) read them here; start_path and camera_path call tile_pixel. Plain
// C++ when no HIP compiler is present, __host__ __device__ under hipcc, as noise.h and gomath.h;
// the units are built with -ffp-contract=off, so pixel_mean rounds alike on both sides.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/izpi_host.h"

#if defined(__HIP__)
#define IZPI_PM __host__ __device__ __forceinline__
#else
#define IZPI_PM inline
#endif

// The packed order (IZPI_OUT_PACKED): tile after tile of `tiles` ([n][4], of which a tile's
// x0 and y0 are read), the rows of each tile, tile_w x tile_h pixels per tile. Packed pixel p
// is sample (x, y) of the frame. An adaptive session's active list, (x, y, pixel, 0) per entry,
// is such a list of 1 x 1 tiles.
IZPI_PM void tile_pixel(const uint32_t* tiles, uint32_t tile_w, uint32_t tile_h, uint32_t p, uint32_t* x, uint32_t* y) {
  const uint32_t tile_px = tile_w * tile_h;
  const uint32_t tile = p / tile_px, in_tile = p % tile_px;
  *x = tiles[4 * tile] + in_tile % tile_w;
  *y = tiles[4 * tile + 1] + in_tile / tile_w;
}

// The pixels of one request and where each goes in its output.
struct PixelMap {
  uint32_t num_pixels, width, height, tile_w, tile_h;
  uint32_t out_layout;  // IZPI_OUT_*
  const uint32_t* tiles;
  IZPI_PM void xy(uint32_t p, uint32_t* x, uint32_t* y) const { tile_pixel(tiles, tile_w, tile_h, p, x, y); }
  // Pixel p's four doubles in `out`: packed, entry p; a canvas, canvas.Set(x, ny - y)
  // (rgb.go:41): column x of row H - y. Sample row y = 0 would be row ny, which the canvas does
  // not have (deviation A9): null.
  IZPI_PM double* slot(uint32_t p, double* out) const {
    if (out_layout == IZPI_OUT_PACKED) return out + (size_t)p * 4;
    uint32_t x, y;
    xy(p, &x, &y);
    const uint32_t row = height - y;
    return row < height ? out + ((size_t)row * width + x) * 4 : nullptr;
  }
};

// (r0, r1, r2, 1.0) into pixel p's slot, if it has one (a caller's buffer: 8-B aligned is all it need be).
IZPI_PM void store_pixel(const PixelMap& map, uint32_t p, double* out, double r0, double r1, double r2) {
  double* o = map.slot(p, out);
  if (!o) return;
  o[0] = r0; o[1] = r1; o[2] = r2; o[3] = 1.0;
}

// The samplers whose mean is sum * (1 / numSamples): Spectral alone (render/spectral.go:98-99).
// Colour, and the preview samplers, which render under rgb.go's loop, take
// vec3.ScalarDiv(col, numSamples) (rgb.go:38). The two differ in the last bit.
IZPI_PM bool mean_by_reciprocal(uint32_t sampler) { return sampler == IZPI_SAMPLER_SPECTRAL; }
// One channel's mean after n samples, as that sampler's canvas holds it.
IZPI_PM double pixel_mean(uint32_t sampler, double c, uint32_t n) {
  return mean_by_reciprocal(sampler) ? c * (1.0 / (double)n) : c / (double)n;
}

// A progressive session's sums as the per-pixel kernels read them (resolve.hip, noise.hip,
// adapt.hip): the session's pixels, the samples `done`, its sampler, the running sums and, with
// IZPI_PROG_NOISE, the second moments ([num_pixels][3] each, read only). counts: an adaptive
// session after its first retirement keeps n_p per pixel; else null,
// and every pixel has `done` samples.
struct SessionView {
  PixelMap map;
  uint32_t done, sampler;
  const double* running;
  const double* moments;
  const uint32_t* counts;
  IZPI_PM uint32_t n(uint32_t p) const { return counts ? counts[p] : done; }
  // Pixel p's sums and moments (48 B).
  IZPI_PM void load(uint32_t p, double s[3], double m2[3]) const {
    for (int c = 0; c < 3; c++) {
      s[c] = running[3 * (size_t)p + c];
      m2[c] = moments[3 * (size_t)p + c];
    }
  }
};
