// denoise_demod_check.cpp — a stand-alone program over izpi_host_denoise and
// izpi_host_denoise_var with IZPI_DENOISE_DEMODULATE (izpi_amd/csrc/denoise_host.cpp;
// host_scene.cpp and scene_pack.cpp hold the host error string), built by
// tests/test_denoise_demod.py with -fsanitize=address,undefined: every canvas and plane is a
// heap block of exactly its size, so a divide, a tap or a multiply one pixel outside the image
// ends the program. It runs the sizes of the parity cases with and without the Normal guide at
// every iteration count, with and without a variance output, over frames whose albedo holds
// zeros, values below the floor, a negative, a NaN and an Inf texel and whose colour and
// standard errors hold a dead row, NaN and overflowing pixels; two hand cases; and every error
// return. Prints one "case <name> ..." line per group and "ok".
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
const double kNan = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

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
  size_t at(uint32_t x, uint32_t y) const { return ((size_t)y * w + x) * 4; }
};

// noise over a two-region guide, the albedo in (0.05, 1); with `specials` the texels and pixels
// the header names
Frames make(uint32_t w, uint32_t h, uint32_t seed, bool specials) {
  const size_t n = (size_t)w * h * 4;
  Frames f{w, h, std::vector<double>(n), std::vector<double>(n), std::vector<double>(n), std::vector<double>(n)};
  Lcg g{seed};
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++) {
      const size_t at = f.at(x, y);
      const bool left = 2 * x + y < w + h / 2;
      for (int k = 0; k < 3; k++) {
        f.colour[at + k] = (left ? 0.7 : 0.2) + 0.3 * (g.next() - 0.5);
        f.se[at + k] = 0.05 + 0.1 * g.next();
        f.normal[at + k] = (left ? (k == 0) : (k == 1)) + 0.02 * (g.next() - 0.5);
        f.albedo[at + k] = left ? 0.5 + 0.5 * g.next() : 0.05 + 0.45 * g.next();
      }
      f.colour[at + 3] = f.se[at + 3] = f.albedo[at + 3] = 1.0;
    }
  if (specials && h > 1)
    for (uint32_t x = 0; x < w; x++)
      for (int k = 0; k < 4; k++) f.colour[f.at(x, 0) + k] = f.se[f.at(x, 0) + k] = f.albedo[f.at(x, 0) + k] = 0.0;
  if (specials && w >= 8 && h >= 8) {
    for (uint32_t y = 2; y < 5; y++)
      for (uint32_t x = 1; x < 4; x++)
        for (int k = 0; k < 3; k++) f.albedo[f.at(x, y) + k] = 0.0;
    for (uint32_t y = 5; y < 7; y++)
      for (uint32_t x = 2; x < 6; x++)
        for (int k = 0; k < 3; k++) f.albedo[f.at(x, y) + k] = 1.0 / 4096.0;
    f.albedo[f.at(w / 3, h / 2 + 2)] = -0.25;
    f.albedo[f.at(w / 3 + 2, h / 2 + 2) + 1] = kNan;
    f.albedo[f.at(w / 3 + 1, h / 2 + 3) + 2] = kInf;
    f.colour[f.at(w / 3, h / 2) + 1] = kNan;
    f.colour[f.at(2, 3)] = 1e308;  // over a 0 texel: the quotient overflows
    f.se[f.at(w / 3 + 1, h / 2 - 2) + 2] = kNan;
  }
  return f;
}

double modulus(double a) { return isfinite(a) && a > IZPI_DENOISE_ALBEDO_FLOOR ? a : IZPI_DENOISE_ALBEDO_FLOOR; }
bool live(const double* p) { return p[3] != 0 && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// was the pixel live in iteration 0? (var: with its V_0)
bool live0(const Frames& f, size_t at, bool var) {
  const double* c = &f.colour[at];
  if (!live(c)) return false;
  double v = 0.0;
  for (int k = 0; k < 3; k++) {
    const double m = modulus(f.albedo[at + k]);
    if (!isfinite(c[k] / m)) return false;
    const double s = f.se[at + k] / m;
    v += s * s;
  }
  return !var || (v >= 0 && isfinite(v));
}

void run_size(uint32_t w, uint32_t h, const std::vector<uint32_t>& iterations, const char* name) {
  int calls = 0;
  for (int specials = 0; specials < 2; specials++) {
    const Frames f = make(w, h, 11u + w * 131u + h, specials != 0);
    for (uint32_t n : iterations)
      for (int guides = 0; guides < 2; guides++)  // with and without the Normal guide
        for (int mode = 0; mode < 3; mode++) {    // the fixed filter; the variance one without and with a plane
          const double* nm = guides == 0 ? f.normal.data() : nullptr;
          const bool var = mode > 0, plane = mode == 2;
          std::vector<double> out(f.colour.size(), -5.0), v(plane ? (size_t)w * h : 0, -5.0);
          const izpi_denoise_params p = {n, IZPI_DENOISE_DEMODULATE, var ? 2.0 : 1.0, 0.5, 0.5};
          const int rc = var ? izpi_host_denoise_var(f.colour.data(), f.se.data(), nm, f.albedo.data(), out.data(),
                                                     plane ? v.data() : nullptr, w, h, &p, kFloor)
                             : izpi_host_denoise(f.colour.data(), nm, f.albedo.data(), out.data(), w, h, &p);
          calls++;
          EXPECT(rc == IZPI_OK, name);
          for (size_t i = 0; i < (size_t)w * h; i++) {
            const double* c = &f.colour[4 * i];
            const double* o = &out[4 * i];
            EXPECT(memcmp(&o[3], &c[3], sizeof(double)) == 0, name);  // alpha is the centre's
            if (n == 0 || !live0(f, 4 * i, var)) {
              EXPECT(memcmp(o, c, 4 * sizeof(double)) == 0, name);  // the input, bit for bit
            } else {
              EXPECT(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]), name);  // nothing leaked in
              if (plane) EXPECT(isfinite(v[i]) && v[i] >= 0, name);
            }
          }
        }
  }
  printf("case %s %d calls\n", name, calls);
}

void run_hand() {
  // a texture under constant light comes back: C = A * L, so D_0 is L and the filter has nothing to do
  const uint32_t w = 9, h = 9;
  const size_t n = (size_t)w * h * 4;
  std::vector<double> c(n), s(n), a(n), out(n), var((size_t)w * h);
  for (uint32_t i = 0; i < w * h; i++) {
    for (int k = 0; k < 3; k++) {
      a[4 * i + k] = 0.3 + 0.2 * (i % 2) + 0.1 * k;
      c[4 * i + k] = a[4 * i + k] * 0.75;
      s[4 * i + k] = a[4 * i + k] * 0.05;
    }
    a[4 * i + 3] = c[4 * i + 3] = s[4 * i + 3] = 1.0;
  }
  const izpi_denoise_params five = {5, IZPI_DENOISE_DEMODULATE, 1.0, 0.5, 0.5};
  EXPECT(izpi_host_denoise(c.data(), nullptr, a.data(), out.data(), w, h, &five) == IZPI_OK, "hand");
  for (size_t i = 0; i < n; i++) EXPECT(fabs(out[i] - c[i]) <= 1e-12 * c[i], "hand: the texture stays");
  EXPECT(izpi_host_denoise_var(c.data(), s.data(), nullptr, a.data(), out.data(), var.data(), w, h, &five, kFloor) == IZPI_OK, "hand");
  for (size_t i = 0; i < n; i++) EXPECT(fabs(out[i] - c[i]) <= 1e-12 * c[i], "hand: the texture stays (variance)");
  // zero iterations: a copy and the colour's V_0, flag or not
  const izpi_denoise_params none = {0, IZPI_DENOISE_DEMODULATE, 1.0, 0.5, 0.5};
  std::fill(out.begin(), out.end(), -1.0);
  EXPECT(izpi_host_denoise_var(c.data(), s.data(), nullptr, a.data(), out.data(), var.data(), w, h, &none, kFloor) == IZPI_OK, "hand");
  EXPECT(memcmp(out.data(), c.data(), n * sizeof(double)) == 0, "hand: 0 iterations copy");
  for (uint32_t i = 0; i < w * h; i++) {
    const double* q = &s[4 * i];
    const double v0 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    EXPECT(memcmp(&var[i], &v0, sizeof(double)) == 0, "hand: 0 iterations hand out the colour's V_0");
  }
  printf("case hand\n");
}

void expect_invalid(int rc, const char* message, const char* what) {
  EXPECT(rc == IZPI_ERR_INVALID, what);
  EXPECT(strcmp(izpi_host_last_error(), message) == 0, what);
}

void run_arguments() {
  std::vector<double> c(4 * 4 * 4, 1.0), s(4 * 4 * 4, 0.1), a(4 * 4 * 4, 0.5), out(4 * 4 * 4, 7.0), var(4 * 4, 7.0);
  const izpi_denoise_params ok = {5, IZPI_DENOISE_DEMODULATE, 2.0, 0.5, 0.5};
  izpi_denoise_params p = ok;
  const char* flags = "denoise: flags must be 0";
  const char* needs = "denoise: demodulation needs the albedo canvas";
  const char* over = "denoise: out may not overlap an input canvas";
  for (uint32_t word : {1u, 2u, 3u, 5u, 6u, 8u, 12u, 0x80000004u}) {
    p.flags = word;
    expect_invalid(izpi_host_denoise(c.data(), nullptr, a.data(), out.data(), 4, 4, &p), flags, "flags");
    expect_invalid(izpi_host_denoise_var(c.data(), s.data(), nullptr, a.data(), out.data(), var.data(), 4, 4, &p, kFloor), flags,
                   "flags (variance)");
  }
  expect_invalid(izpi_host_denoise(c.data(), a.data(), nullptr, out.data(), 4, 4, &ok), needs, "no albedo");
  expect_invalid(izpi_host_denoise_var(c.data(), s.data(), a.data(), nullptr, out.data(), var.data(), 4, 4, &ok, kFloor), needs,
                 "no albedo (variance)");
  p = ok; p.iterations = 0;  // (the rule holds with no iteration to run)
  expect_invalid(izpi_host_denoise(c.data(), nullptr, nullptr, out.data(), 4, 4, &p), needs, "no albedo, 0 iterations");
  expect_invalid(izpi_host_denoise(c.data(), nullptr, a.data(), a.data(), 4, 4, &ok), over, "out is the albedo");
  expect_invalid(izpi_host_denoise_var(c.data(), s.data(), nullptr, a.data(), out.data(), a.data() + 16, 4, 4, &ok, kFloor),
                 "denoise: the variance output may not overlap an input canvas", "the plane inside the albedo");
  p = ok; p.iterations = 9;
  expect_invalid(izpi_host_denoise(c.data(), nullptr, a.data(), out.data(), 4, 4, &p), "denoise: at most 8 iterations", "nine iterations");
  p = ok; p.sigma_albedo = 0.0;
  expect_invalid(izpi_host_denoise(c.data(), nullptr, a.data(), out.data(), 4, 4, &p),
                 "denoise: every sigma must be greater than 0 (+Inf drops its term)", "sigma 0");
  expect_invalid(izpi_host_denoise_var(c.data(), nullptr, nullptr, a.data(), out.data(), var.data(), 4, 4, &ok, kFloor),
                 "denoise: the standard errors must be given", "no standard errors");
  expect_invalid(izpi_host_denoise_var(c.data(), s.data(), nullptr, a.data(), out.data(), var.data(), 4, 4, &ok, 0.0),
                 "denoise: variance_floor must be finite and greater than 0", "floor 0");
  expect_invalid(izpi_host_denoise(c.data(), nullptr, a.data(), out.data(), 0, 4, &ok), "denoise: width and height must be at least 1",
                 "zero width");
  expect_invalid(izpi_host_denoise(nullptr, nullptr, a.data(), out.data(), 4, 4, &ok), "denoise: colour and out must be given", "no colour");
  for (double v : out) EXPECT(v == 7.0, "a refused call writes nothing");
  for (double v : var) EXPECT(v == 7.0, "a refused call writes nothing");
  p = {8, IZPI_DENOISE_DEMODULATE, kInf, kInf, kInf};
  EXPECT(izpi_host_denoise(c.data(), nullptr, a.data(), out.data(), 4, 4, &p) == IZPI_OK, "the limits are allowed");
  EXPECT(izpi_host_denoise_var(c.data(), s.data(), nullptr, a.data(), out.data(), nullptr, 4, 4, &p, kFloor) == IZPI_OK,
         "the limits are allowed (variance, no plane)");
  for (double v : out) EXPECT(fabs(v - 1.0) <= 1e-14, "a constant image stays constant");
  EXPECT(izpi_host_denoise(c.data(), nullptr, nullptr, out.data(), 4, 4, nullptr) == IZPI_OK, "NULL params: no flag, no albedo needed");
  printf("case arguments\n");
}

}  // namespace

int main() {
  const std::vector<uint32_t> all = {0, 1, 5, 8};
  run_size(40, 30, all, "40x30");
  run_size(1, 1, all, "1x1");
  run_size(1, 7, all, "1x7");
  run_size(37, 19, all, "37x19");
  run_hand();
  run_arguments();
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
