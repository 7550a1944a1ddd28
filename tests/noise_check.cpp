// noise_check.cpp — a stand-alone program over izpi_host_noise (izpi_amd/csrc/noise_host.cpp;
// host_scene.cpp and scene_pack.cpp hold the host error string), built by tests/test_noise.py
// with -fsanitize=address,undefined: every array is a heap block of exactly its size, so a
// read or a store one pixel outside ends the program. It runs the pixel counts around the
// 256-pixel blocks of sum_error's tree, with and without a mask and an se output, the hand
// cases, non-finite pixels, and the argument checks. Prints one "case <name> ..." line per
// group and "ok".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
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

struct Pixels {
  std::vector<double> sums, m2;
  std::vector<uint8_t> counted;
};

// n pixels of `done` samples each, folded in sample order; every seventh pixel black
Pixels make(uint32_t n, uint32_t done, uint32_t seed) {
  Pixels px{std::vector<double>((size_t)n * 3), std::vector<double>((size_t)n * 3), std::vector<uint8_t>(n)};
  Lcg g{seed};
  for (uint32_t p = 0; p < n; p++) {
    px.counted[p] = p % 5 != 0;
    for (uint32_t s = 0; s < done; s++)
      for (int c = 0; c < 3; c++) {
        const double x = p % 7 == 0 ? 0.0 : g.next() * (1 + c);
        px.sums[3 * (size_t)p + c] += x;
        px.m2[3 * (size_t)p + c] += x * x;
      }
  }
  return px;
}

void sizes() {
  const uint32_t ns[] = {1, 255, 256, 257, 1200};
  for (uint32_t n : ns) {
    const Pixels px = make(n, 5, 17 + n);
    for (int masked = 0; masked < 2; masked++)
      for (int with_se = 0; with_se < 2; with_se++) {
        std::vector<double> se(with_se ? (size_t)n * 4 : 0);
        izpi_noise_stats st;
        memset(&st, 0xAB, sizeof(st));
        const int rc = izpi_host_noise(px.sums.data(), px.m2.data(), masked ? px.counted.data() : nullptr, n, 5,
                                       IZPI_SAMPLER_COLOUR, nullptr, with_se ? se.data() : nullptr, &st);
        EXPECT(rc == IZPI_OK, "sizes");
        uint64_t want = 0;
        for (uint32_t p = 0; p < n; p++) want += masked ? px.counted[p] : 1;
        EXPECT(st.pixels == want && st.nonfinite == 0 && st.above <= st.pixels && st.done == 5, "sizes");
        EXPECT(st.sum_error >= 0 && st.max_error >= 0 && st.sum_error <= st.max_error * (double)st.pixels, "sizes");
        EXPECT(st.device_ms == 0, "sizes");
        for (size_t k = 0; k < se.size(); k++) EXPECT(k % 4 == 3 ? se[k] == 1.0 : se[k] >= 0, "sizes");
      }
    printf("case %u pixels\n", n);
  }
}

void hand() {
  izpi_noise_params p = {0.25, 0.01, 0.05, 2, 0};
  izpi_noise_stats st;
  double se[4];
  {  // four samples of 0.5
    const double s[3] = {2.0, 2.0, 2.0}, m[3] = {1.0, 1.0, 1.0};
    EXPECT(izpi_host_noise(s, m, nullptr, 1, 4, IZPI_SAMPLER_COLOUR, &p, se, &st) == IZPI_OK, "hand");
    EXPECT(se[0] == 0 && se[1] == 0 && se[2] == 0 && se[3] == 1.0 && st.max_error == 0 && st.sum_error == 0 && st.converged == 1, "hand");
  }
  {  // samples 0, 1, 0, 1: v = 1/3
    const double s[3] = {2.0, 2.0, 2.0}, m[3] = {2.0, 2.0, 2.0};
    EXPECT(izpi_host_noise(s, m, nullptr, 1, 4, IZPI_SAMPLER_SPECTRAL, &p, se, &st) == IZPI_OK, "hand");
    const double v = (2.0 - 4.0 / 4.0) / 3.0;
    EXPECT(se[0] == sqrt(v / 4.0) && st.above == 1 && st.converged == 0, "hand");
  }
  {  // NaN sum, Inf moment, an overflowing s * s
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double s[9] = {nan, 1, 1, 1, 1, 1, 2.4e154, 1, 1}, m[9] = {1, 1, 1, 1, inf, 1, 1.44e308, 1, 1};
    double se3[12];
    EXPECT(izpi_host_noise(s, m, nullptr, 3, 4, IZPI_SAMPLER_COLOUR, &p, se3, &st) == IZPI_OK, "hand");
    EXPECT(st.pixels == 3 && st.nonfinite == 2 && se3[0] == 0 && isinf(se3[5]) && se3[8] == 0, "hand");
  }
  printf("case hand\n");
}

void arguments() {
  const double s[3] = {1, 1, 1}, m[3] = {1, 1, 1};
  izpi_noise_stats st;
  memset(&st, 0, sizeof(st));
  const izpi_noise_params good = {0.25, 0.01, 0.05, 8, 0};
  izpi_noise_params bad[8] = {good, good, good, good, good, good, good, good};
  bad[0].threshold = 0; bad[1].threshold = std::numeric_limits<double>::infinity();
  bad[2].floor = -1; bad[3].floor = std::numeric_limits<double>::quiet_NaN();
  bad[4].tolerated = -0.1; bad[5].tolerated = 1.5; bad[6].tolerated = std::numeric_limits<double>::quiet_NaN();
  bad[7].flags = 1;
  for (const izpi_noise_params& b : bad) {
    EXPECT(izpi_host_noise(s, m, nullptr, 1, 4, IZPI_SAMPLER_COLOUR, &b, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
    EXPECT(strncmp(izpi_host_last_error(), "noise: ", 7) == 0, "arguments");
  }
  EXPECT(izpi_host_noise(nullptr, m, nullptr, 1, 4, IZPI_SAMPLER_COLOUR, &good, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
  EXPECT(izpi_host_noise(s, nullptr, nullptr, 1, 4, IZPI_SAMPLER_COLOUR, &good, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
  EXPECT(izpi_host_noise(s, m, nullptr, 1, 1, IZPI_SAMPLER_COLOUR, &good, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
  EXPECT(izpi_host_noise(s, m, nullptr, 1, 4, 0, &good, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
  EXPECT(st.pixels == 0, "arguments");  // nothing was written
  EXPECT(izpi_host_noise(s, m, nullptr, 0, 4, IZPI_SAMPLER_COLOUR, &good, nullptr, &st) == IZPI_OK && st.pixels == 0, "arguments");
  EXPECT(izpi_host_noise(s, m, nullptr, 1, 4, IZPI_SAMPLER_COLOUR, nullptr, nullptr, nullptr) == IZPI_OK, "arguments");
  printf("case arguments\n");
}

}  // namespace

int main() {
  sizes();
  hand();
  arguments();
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
