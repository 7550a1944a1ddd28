// denoise_var_check.cpp — a stand-alone program over izpi_host_denoise_var (izpi_amd/csrc/
// denoise_host.cpp; host_scene.cpp and scene_pack.cpp hold the host error string), built
// by tests/test_denoise_var.py with -fsanitize=address,undefined: every canvas and plane is a
// heap block of exactly its size, so a tap or a store one pixel outside the image ends the
// program. It runs the sizes of the parity cases with every guide set and iteration count,
// with and without a variance output; dead, NaN and Inf pixels, NaN, Inf and zero standard
// errors; a 64 x 64 image at 8 iterations (reach 256, four times the image); two hand cases;
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

const double kFloor = IZPI_DENOISE_VAR_DEFAULT_FLOOR;

struct Lcg {
  uint32_t s;
  double next() {
    s = 1664525u * s + 1013904223u;
    return s / 4294967296.0;
  }
};

struct Frames {
  uint32_t w, h;
  std::vector<double> colour, se, normal, albedo;
};

// noise over a two-region guide with standard errors around 0.1; with `specials` row 0 dead,
// one NaN and one Inf colour pixel, a NaN guide texel, and NaN, Inf and zero standard errors
Frames make(uint32_t w, uint32_t h, uint32_t seed, bool specials) {
  const size_t n = (size_t)w * h * 4;
  Frames f{w, h, std::vector<double>(n), std::vector<double>(n), std::vector<double>(n), std::vector<double>(n)};
  Lcg g{seed};
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++) {
      const size_t at = ((size_t)y * w + x) * 4;
      const bool left = 2 * x + y < w + h / 2;
      for (int k = 0; k < 3; k++) {
        f.colour[at + k] = (left ? 0.7 : 0.2) + 0.3 * (g.next() - 0.5);
        f.se[at + k] = 0.05 + 0.1 * g.next();
        f.normal[at + k] = (left ? (k == 0) : (k == 1)) + 0.02 * (g.next() - 0.5);
        f.albedo[at + k] = (left ? 0.8 : 0.1 + 0.4 * k) + 0.01 * (g.next() - 0.5);
      }
      f.colour[at + 3] = f.se[at + 3] = f.albedo[at + 3] = 1.0;
    }
  if (specials && h > 1) {
    for (uint32_t x = 0; x < w; x++)
      for (int k = 0; k < 4; k++) f.colour[(size_t)x * 4 + k] = f.se[(size_t)x * 4 + k] = 0.0;  // row 0: never written
    if (w > 4 && h > 4) {
      const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
      f.colour[((size_t)(h / 2) * w + w / 3) * 4 + 1] = nan;
      f.colour[((size_t)(h / 3) * w + w / 2) * 4 + 2] = inf;
      f.normal[((size_t)(h - 1) * w + 1) * 4] = nan;
      f.se[((size_t)(h / 2) * w + w / 3 + 2) * 4] = nan;
      f.se[((size_t)(h / 3) * w + w / 2 + 2) * 4 + 1] = inf;
      for (uint32_t x = 0; x < 3; x++)
        for (int k = 0; k < 3; k++) f.se[((size_t)(h - 2) * w + x) * 4 + k] = 0.0;
    }
  }
  return f;
}

double v0_of(const double* s) { return (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]; }
bool live(const double* p, double v) {
  return p[3] != 0 && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && v >= 0 && isfinite(v);
}

void run_size(uint32_t w, uint32_t h, const std::vector<uint32_t>& iterations, const char* name) {
  int calls = 0;
  for (int specials = 0; specials < 2; specials++) {
    const Frames f = make(w, h, 7u + w * 131u + h, specials != 0);
    for (uint32_t n : iterations)
      for (int guides = 0; guides < 3; guides++)      // both, normal only, none
        for (int plane = 0; plane < 2; plane++) {     // with and without a variance output
          const double* nm = guides < 2 ? f.normal.data() : nullptr;
          const double* al = guides < 1 ? f.albedo.data() : nullptr;
          std::vector<double> out(f.colour.size(), -5.0), var(plane ? (size_t)w * h : 0, -5.0);
          const izpi_denoise_params p = {n, 0, 2.0, 0.5, 0.5};
          const int rc = izpi_host_denoise_var(f.colour.data(), f.se.data(), nm, al, out.data(), plane ? var.data() : nullptr,
                                               w, h, &p, kFloor);
          calls++;
          EXPECT(rc == IZPI_OK, name);
          for (size_t i = 0; i < (size_t)w * h; i++) {
            const double* c = &f.colour[4 * i];
            const double* o = &out[4 * i];
            const double v0 = v0_of(&f.se[4 * i]);
            EXPECT(memcmp(&o[3], &c[3], sizeof(double)) == 0, name);  // alpha is the centre's
            if (!live(c, v0) || n == 0) {
              EXPECT(memcmp(o, c, 4 * sizeof(double)) == 0, name);  // copied through
              if (plane) EXPECT(memcmp(&var[i], &v0, sizeof(double)) == 0, name);  // ... with its V
            } else {
              EXPECT(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]), name);  // nothing leaked in
              if (plane) EXPECT(isfinite(var[i]) && var[i] >= 0, name);
            }
          }
        }
  }
  printf("case %s %d calls\n", name, calls);
}

void run_hand() {
  // a constant frame keeps its colour, and its variance falls by (sum h^2)^2 = (35/128)^2
  const uint32_t w = 9, h = 9;
  std::vector<double> c((size_t)w * h * 4, 0.5), s((size_t)w * h * 4, 0.1), out(c.size()), var((size_t)w * h);
  for (size_t i = 0; i < (size_t)w * h; i++) c[4 * i + 3] = s[4 * i + 3] = 1.0;
  const izpi_denoise_params one = {1, 0, 2.0, 0.5, 0.5};
  EXPECT(izpi_host_denoise_var(c.data(), s.data(), nullptr, nullptr, out.data(), var.data(), w, h, &one, kFloor) == IZPI_OK, "hand");
  EXPECT(memcmp(out.data(), c.data(), c.size() * sizeof(double)) == 0, "hand: the colour stays");
  const double v0 = v0_of(s.data()), want = v0 * (35.0 / 128.0) * (35.0 / 128.0);
  EXPECT(fabs(var[4 * w + 4] - want) <= 1e-12 * want, "hand: the B3 gain");
  // zero iterations: a copy and V_0
  const izpi_denoise_params none = {0, 0, 2.0, 0.5, 0.5};
  std::fill(out.begin(), out.end(), -1.0);
  EXPECT(izpi_host_denoise_var(c.data(), s.data(), nullptr, nullptr, out.data(), var.data(), w, h, &none, kFloor) == IZPI_OK, "hand");
  EXPECT(memcmp(out.data(), c.data(), c.size() * sizeof(double)) == 0, "hand: 0 iterations copy");
  for (double v : var) EXPECT(memcmp(&v, &v0, sizeof(double)) == 0, "hand: 0 iterations hand out V_0");
  printf("case hand\n");
}

void expect_invalid(const double* c, const double* s, double* out, double* var, uint32_t w, uint32_t h,
                    const izpi_denoise_params* p, double floor, const char* what) {
  const int rc = izpi_host_denoise_var(c, s, nullptr, nullptr, out, var, w, h, p, floor);
  EXPECT(rc == IZPI_ERR_INVALID, what);
  EXPECT(strncmp(izpi_host_last_error(), "denoise: ", 9) == 0, what);
}

void run_arguments() {
  std::vector<double> c(4 * 4 * 4, 1.0), s(4 * 4 * 4, 0.1), out(4 * 4 * 4, 7.0), var(4 * 4, 7.0);
  const izpi_denoise_params ok = {5, 0, 2.0, 0.5, 0.5};
  izpi_denoise_params p = ok;
  expect_invalid(c.data(), s.data(), c.data(), var.data(), 4, 4, &ok, kFloor, "alias");
  expect_invalid(c.data(), s.data(), c.data() + 4, var.data(), 3, 4, &ok, kFloor, "overlap");
  expect_invalid(c.data(), s.data(), s.data(), var.data(), 4, 4, &ok, kFloor, "out is the standard errors");
  expect_invalid(c.data(), s.data(), out.data(), out.data() + 8, 4, 4, &ok, kFloor, "the plane inside out");
  expect_invalid(c.data(), s.data(), out.data(), s.data() + 48, 4, 4, &ok, kFloor, "the plane inside the standard errors");
  expect_invalid(c.data(), nullptr, out.data(), var.data(), 4, 4, &ok, kFloor, "no standard errors");
  p = ok; p.iterations = 9;
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 4, 4, &p, kFloor, "nine iterations");
  p = ok; p.sigma_colour = 0.0;
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 4, 4, &p, kFloor, "sigma 0");
  p = ok; p.sigma_albedo = std::numeric_limits<double>::quiet_NaN();
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 4, 4, &p, kFloor, "sigma NaN");
  p = ok; p.sigma_normal = -2.0;
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 4, 4, &p, kFloor, "sigma < 0");
  p = ok; p.flags = 2;
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 4, 4, &p, kFloor, "flags");
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 0, 4, &ok, kFloor, "zero width");
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 4, 0, &ok, kFloor, "zero height");
  expect_invalid(nullptr, s.data(), out.data(), var.data(), 4, 4, &ok, kFloor, "no colour");
  expect_invalid(c.data(), s.data(), nullptr, var.data(), 4, 4, &ok, kFloor, "no out");
  const double inf = std::numeric_limits<double>::infinity();
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 4, 4, &ok, 0.0, "floor 0");
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 4, 4, &ok, -1.0, "floor < 0");
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 4, 4, &ok, inf, "floor Inf");
  expect_invalid(c.data(), s.data(), out.data(), var.data(), 4, 4, &ok, std::numeric_limits<double>::quiet_NaN(), "floor NaN");
  for (double v : out) EXPECT(v == 7.0, "a refused call writes nothing");
  for (double v : var) EXPECT(v == 7.0, "a refused call writes nothing");
  p = {8, 0, inf, inf, inf};
  EXPECT(izpi_host_denoise_var(c.data(), s.data(), nullptr, nullptr, out.data(), var.data(), 4, 4, &p, kFloor) == IZPI_OK,
         "the limits are allowed");
  EXPECT(izpi_host_denoise_var(c.data(), s.data(), nullptr, nullptr, out.data(), nullptr, 4, 4, nullptr, kFloor) == IZPI_OK,
         "NULL params, no plane");
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
  run_hand();
  run_arguments();
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
