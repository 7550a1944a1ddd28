// denoise_check.cpp — a stand-alone program over izpi_host_denoise (izpi_amd/csrc/
// denoise_host.cpp; host_scene.cpp and scene_pack.cpp hold the host error string), built by
// tests/test_denoise.py with -fsanitize=address,undefined: every canvas is a heap block of
// exactly its size, so a tap or a store one pixel outside the image ends the program.
// It runs the sizes of the parity cases with every guide set and iteration count, dead,
// NaN and Inf pixels, a 64 x 64 image at 8 iterations (reach 256, four times the image),
// and the argument checks. Prints one "case <name> ..." line per group and "ok".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "../include/izpi_host.h"

namespace {

int failures = 0;
#define EXPECT(cond, what)                                            \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED %s: %s (line %d)\n", what, #cond, __LINE__);     \
      failures++;                                                     \
    }                                                                 \
  } while (0)

struct Lcg {
  uint32_t s;
  double next() {
    s = 1664525u * s + 1013904223u;
    return s / 4294967296.0;
  }
};

struct Frames {
  uint32_t w, h;
  std::vector<double> colour, normal, albedo;
};

// noise over a two-region guide, row 0 dead, one NaN and one Inf pixel where there is room
Frames make(uint32_t w, uint32_t h, uint32_t seed, bool specials) {
  Frames f{w, h, std::vector<double>((size_t)w * h * 4), std::vector<double>((size_t)w * h * 4),
           std::vector<double>((size_t)w * h * 4)};
  Lcg g{seed};
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++) {
      const size_t at = ((size_t)y * w + x) * 4;
      const bool left = 2 * x + y < w + h / 2;
      for (int k = 0; k < 3; k++) {
        f.colour[at + k] = (left ? 0.7 : 0.2) + 0.3 * (g.next() - 0.5);
        f.normal[at + k] = (left ? (k == 0) : (k == 1)) + 0.02 * (g.next() - 0.5);
        f.albedo[at + k] = (left ? 0.8 : 0.1 + 0.4 * k) + 0.01 * (g.next() - 0.5);
      }
      f.colour[at + 3] = f.albedo[at + 3] = 1.0;
    }
  if (specials && h > 1) {
    for (uint32_t x = 0; x < w; x++)
      for (int k = 0; k < 4; k++) f.colour[(size_t)x * 4 + k] = 0.0;  // row 0: never written
    if (w > 4 && h > 4) {
      f.colour[((size_t)(h / 2) * w + w / 3) * 4 + 1] = std::numeric_limits<double>::quiet_NaN();
      f.colour[((size_t)(h / 3) * w + w / 2) * 4 + 2] = std::numeric_limits<double>::infinity();
      f.normal[((size_t)(h - 1) * w + 1) * 4] = std::numeric_limits<double>::quiet_NaN();
    }
  }
  return f;
}

bool live(const double* p) { return p[3] != 0 && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

void run_size(uint32_t w, uint32_t h, const std::vector<uint32_t>& iterations, const char* name) {
  int calls = 0;
  for (int specials = 0; specials < 2; specials++) {
    const Frames f = make(w, h, 7u + w * 131u + h, specials != 0);
    for (uint32_t n : iterations)
      for (int guides = 0; guides < 3; guides++) {  // both, normal only, none
        const double* nm = guides < 2 ? f.normal.data() : nullptr;
        const double* al = guides < 1 ? f.albedo.data() : nullptr;
        std::vector<double> out(f.colour.size(), -5.0);
        const izpi_denoise_params p = {n, 0, 1.0, 0.5, 0.5};
        const int rc = izpi_host_denoise(f.colour.data(), nm, al, out.data(), w, h, &p);
        calls++;
        EXPECT(rc == IZPI_OK, name);
        for (size_t i = 0; i < (size_t)w * h; i++) {
          const double* c = &f.colour[4 * i];
          const double* o = &out[4 * i];
          EXPECT(memcmp(&o[3], &c[3], sizeof(double)) == 0, name);  // alpha is the centre's
          if (!live(c) || n == 0) EXPECT(memcmp(o, c, 4 * sizeof(double)) == 0, name);  // copied through
          else EXPECT(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]), name);  // nothing leaked in
        }
      }
  }
  printf("case %s %d calls\n", name, calls);
}

void expect_invalid(const double* c, double* out, uint32_t w, uint32_t h, const izpi_denoise_params* p, const char* what) {
  const int rc = izpi_host_denoise(c, nullptr, nullptr, out, w, h, p);
  EXPECT(rc == IZPI_ERR_INVALID, what);
  EXPECT(strncmp(izpi_host_last_error(), "denoise: ", 9) == 0, what);
}

void run_arguments() {
  std::vector<double> c(4 * 4 * 4, 1.0), out(4 * 4 * 4, 7.0);
  const izpi_denoise_params ok = {5, 0, 1.0, 0.5, 0.5};
  izpi_denoise_params p = ok;
  expect_invalid(c.data(), c.data(), 4, 4, &ok, "alias");
  expect_invalid(c.data(), c.data() + 4, 3, 4, &ok, "overlap");
  p = ok; p.iterations = 9;
  expect_invalid(c.data(), out.data(), 4, 4, &p, "nine iterations");
  p = ok; p.sigma_colour = 0.0;
  expect_invalid(c.data(), out.data(), 4, 4, &p, "sigma 0");
  p = ok; p.sigma_albedo = std::numeric_limits<double>::quiet_NaN();
  expect_invalid(c.data(), out.data(), 4, 4, &p, "sigma NaN");
  p = ok; p.sigma_normal = -2.0;
  expect_invalid(c.data(), out.data(), 4, 4, &p, "sigma < 0");
  p = ok; p.flags = 2;
  expect_invalid(c.data(), out.data(), 4, 4, &p, "flags");
  expect_invalid(c.data(), out.data(), 0, 4, &ok, "zero width");
  expect_invalid(c.data(), out.data(), 4, 0, &ok, "zero height");
  expect_invalid(nullptr, out.data(), 4, 4, &ok, "no colour");
  expect_invalid(c.data(), nullptr, 4, 4, &ok, "no out");
  for (double v : out) EXPECT(v == 7.0, "a refused call writes nothing");
  const double inf = std::numeric_limits<double>::infinity();
  p = {8, 0, inf, inf, inf};
  EXPECT(izpi_host_denoise(c.data(), nullptr, nullptr, out.data(), 4, 4, &p) == IZPI_OK, "the limits are allowed");
  EXPECT(izpi_host_denoise(c.data(), nullptr, nullptr, out.data(), 4, 4, nullptr) == IZPI_OK, "NULL params");
  for (double v : out) EXPECT(v == 1.0, "a constant image stays constant");
  printf("case arguments\n");
}

}  // namespace

int main() {
  const std::vector<uint32_t> all = {0, 1, 5, 8};
  run_size(40, 30, all, "40x30");
  run_size(1, 1, all, "1x1");
  run_size(1, 7, all, "1x7");
  run_size(37, 19, all, "37x19");
  run_size(64, 64, {8}, "64x64");
  run_arguments();
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
