// adapt_check.cpp — a stand-alone program over izpi_host_adapt (izpi_amd/csrc/noise_host.cpp;
// host_scene.cpp and scene_pack.cpp hold the host error string), built by tests/test_adapt.py
// with -fsanitize=address,undefined: every array is a heap block of exactly its size, so a
// read or a store one pixel outside ends the program. It runs sessions of two evaluations over
// several pixel counts, with and without a mask and an e output, and the argument checks.
// Prints one "case <name>" line per group and "ok".
#include <stdint.h>
#include <stdio.h>

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

void sessions() {
  const uint32_t ns[] = {1, 63, 64, 257, 1200};
  for (uint32_t n : ns) {
    for (int masked = 0; masked < 2; masked++) {
      std::vector<double> sums((size_t)n * 3), m2((size_t)n * 3), e(n);
      std::vector<uint8_t> counted(n), active(n, 1);
      std::vector<uint32_t> samples(n, 0);
      Lcg g{n};
      uint64_t was_active = n, rendered = 0;
      for (uint32_t done = 4; done <= 8; done += 4) {  // two steps of 4 samples over the active pixels
        for (uint32_t p = 0; p < n; p++) {
          counted[p] = p % 5 != 0;
          if (!active[p]) continue;
          samples[p] += 4;
          rendered += 4;
          for (uint32_t s = 0; s < 4; s++)
            for (int c = 0; c < 3; c++) {
              const double x = p % 7 == 0 ? 0.25 : p % 11 == 0 ? std::numeric_limits<double>::quiet_NaN() : g.next() * (1 + c);
              sums[3 * (size_t)p + c] += x;
              m2[3 * (size_t)p + c] += x * x;
            }
        }
        izpi_adapt_stats st;
        const izpi_noise_params p = {0.25, 0.01, 0.5, 4, 0};
        const int rc = izpi_host_adapt(sums.data(), m2.data(), masked ? counted.data() : nullptr, samples.data(), active.data(), n,
                                       done, IZPI_SAMPLER_COLOUR, &p, done == 4 ? e.data() : nullptr, &st);
        EXPECT(rc == IZPI_OK, "sessions");
        uint64_t now = 0;
        for (uint32_t q = 0; q < n; q++) now += active[q] != 0;
        EXPECT(st.active == now && st.retired == was_active - now && st.samples == rendered && st.done == done, "sessions");
        EXPECT(st.active + st.nonfinite <= st.pixels || !masked, "sessions");
        for (uint32_t q = 0; q < n; q++)  // constant, NaN and uncounted pixels never stay
          EXPECT(!(active[q] && (q % 7 == 0 || q % 11 == 0 || (masked && !counted[q]))), "sessions");
        was_active = now;
      }
    }
    printf("case %u pixels\n", n);
  }
}

void arguments() {
  double s[3] = {2, 2, 2}, m[3] = {2, 2, 2};
  uint32_t n4 = 4;
  uint8_t act = 1;
  izpi_adapt_stats st = {};
  const izpi_noise_params good = {0.25, 0.01, 0.05, 8, 0};
  izpi_noise_params bad = good;
  bad.threshold = 0;
  EXPECT(izpi_host_adapt(s, m, nullptr, &n4, &act, 1, 4, IZPI_SAMPLER_COLOUR, &bad, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
  EXPECT(izpi_host_adapt(nullptr, m, nullptr, &n4, &act, 1, 4, IZPI_SAMPLER_COLOUR, &good, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
  EXPECT(izpi_host_adapt(s, m, nullptr, nullptr, &act, 1, 4, IZPI_SAMPLER_COLOUR, &good, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
  EXPECT(izpi_host_adapt(s, m, nullptr, &n4, nullptr, 1, 4, IZPI_SAMPLER_COLOUR, &good, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
  EXPECT(izpi_host_adapt(s, m, nullptr, &n4, &act, 1, 1, IZPI_SAMPLER_COLOUR, &good, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
  EXPECT(izpi_host_adapt(s, m, nullptr, &n4, &act, 1, 4, IZPI_SAMPLER_NORMAL, &good, nullptr, &st) == IZPI_ERR_INVALID, "arguments");
  EXPECT(st.pixels == 0 && act == 1, "arguments");
  EXPECT(izpi_host_adapt(s, m, nullptr, &n4, &act, 0, 4, IZPI_SAMPLER_COLOUR, &good, nullptr, &st) == IZPI_OK && st.pixels == 0, "arguments");
  EXPECT(izpi_host_adapt(s, m, nullptr, &n4, &act, 1, 4, IZPI_SAMPLER_SPECTRAL, nullptr, nullptr, nullptr) == IZPI_OK, "arguments");
  printf("case arguments\n");
}

}  // namespace

int main() {
  sessions();
  arguments();
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
