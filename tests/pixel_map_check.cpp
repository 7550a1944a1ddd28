// pixel_map_check.cpp — a stand-alone program over izpi_amd/csrc/pixel_map.h, the header the
// per-pixel kernels and the host's share assembly read the packed-pixel rule from, compiled here
// as plain C++ (host_scene.cpp supplies izpi_host_tiles). tests/test_pixel_map.py builds it with
// -fsanitize=address,undefined: every output is a heap block of exactly its size, so a slot one
// pixel outside ends the program. The map is compared against a brute-force enumeration (tile
// after tile, row after row) in both layouts; pixel_mean against the two expressions, at a
// (c, n) where they differ in the last bit. Prints one "case <name> ..." line per case and "ok".
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../izpi_amd/csrc/pixel_map.h"

namespace {

int failures = 0;
#define EXPECT(cond, what)                                            \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED %s: %s (line %d)\n", what, #cond, __LINE__);     \
      failures++;                                                     \
    }                                                                 \
  } while (0)

uint64_t bits(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof(u));
  return u;
}

// The map of `tiles` ([n][4], tw x th each) on a W x H frame against the enumeration, in both
// layouts; row0: whether the list is meant to hold pixels of sample row 0.
void check_map(const char* name, uint32_t W, uint32_t H, const std::vector<uint32_t>& tiles, uint32_t tw, uint32_t th, bool row0) {
  const uint32_t nt = (uint32_t)(tiles.size() / 4), np = nt * tw * th;
  std::vector<uint32_t> ex, ey;  // brute force: tile after tile, row after row
  for (uint32_t t = 0; t < nt; t++)
    for (uint32_t r = 0; r < th; r++)
      for (uint32_t c = 0; c < tw; c++) {
        ex.push_back(tiles[4 * t] + c);
        ey.push_back(tiles[4 * t + 1] + r);
      }
  EXPECT(ex.size() == np, name);
  uint32_t in_row0 = 0;
  for (uint32_t p = 0; p < np; p++) in_row0 += ey[p] == 0;
  EXPECT((in_row0 > 0) == row0, name);
  for (uint32_t layout : {(uint32_t)IZPI_OUT_CANVAS, (uint32_t)IZPI_OUT_PACKED}) {
    const PixelMap map{np, W, H, tw, th, layout, tiles.data()};
    const size_t doubles = layout == IZPI_OUT_PACKED ? (size_t)np * 4 : (size_t)W * H * 4;
    std::vector<double> out(doubles, -7.0);
    std::vector<uint8_t> taken(doubles / 4, 0);
    uint32_t without = 0;
    for (uint32_t p = 0; p < np; p++) {
      uint32_t x = ~0u, y = ~0u, fx = ~0u, fy = ~0u;
      map.xy(p, &x, &y);
      tile_pixel(tiles.data(), tw, th, p, &fx, &fy);
      EXPECT(x == ex[p] && y == ey[p] && fx == ex[p] && fy == ey[p], name);
      double* o = map.slot(p, out.data());
      const bool expect_slot = layout == IZPI_OUT_PACKED || ey[p] != 0;  // sample row 0 has no canvas row (A9)
      EXPECT((o != nullptr) == expect_slot, name);
      store_pixel(map, p, out.data(), p + 0.25, p + 0.5, p + 0.75);  // (ASan: a slot outside the block ends the program)
      if (!o) { without++; continue; }
      const ptrdiff_t at = o - out.data();
      EXPECT(at >= 0 && (size_t)at + 4 <= doubles && at % 4 == 0, name);
      if (at < 0 || (size_t)at + 4 > doubles) continue;
      const size_t want = layout == IZPI_OUT_PACKED ? (size_t)p * 4 : ((size_t)(H - ey[p]) * W + ex[p]) * 4;
      EXPECT((size_t)at == want, name);
      EXPECT(!taken[at / 4], name);  // slots are distinct
      taken[at / 4] = 1;
      EXPECT(o[0] == p + 0.25 && o[1] == p + 0.5 && o[2] == p + 0.75 && o[3] == 1.0, name);
    }
    EXPECT(without == (layout == IZPI_OUT_PACKED ? 0u : in_row0), name);  // exactly the pixels of sample row 0
    size_t written = 0;
    for (size_t k = 0; k < doubles / 4; k++) {
      written += taken[k];
      if (!taken[k]) EXPECT(out[4 * k] == -7.0 && out[4 * k + 1] == -7.0 && out[4 * k + 2] == -7.0 && out[4 * k + 3] == -7.0, name);
    }
    EXPECT(written == np - without, name);
  }
  printf("case %s: %u pixels, %u in sample row 0\n", name, np, in_row0);
}

void maps() {
  const uint32_t W = 40, H = 30;
  std::vector<uint32_t> all(4 * 64);
  const uint32_t nt = izpi_host_tiles(W, H, all.data(), 64);
  EXPECT(nt > 1 && nt <= 64, "frame");
  all.resize(4 * (size_t)nt);
  const uint32_t tw = all[2] - all[0] + 1, th = all[3] - all[1] + 1;
  EXPECT(nt * tw * th == W * H, "frame");
  check_map("frame", W, H, all, tw, th, true);
  // two subsets of the frame's tiles, in the list's order: with and without sample row 0
  std::vector<uint32_t> with0, without0;
  for (uint32_t t = 0; t < nt; t++) {
    std::vector<uint32_t>& to = all[4 * t + 1] == 0 ? with0 : without0;
    if (to.size() < 4 * 3) to.insert(to.end(), all.begin() + 4 * t, all.begin() + 4 * t + 4);
  }
  with0.insert(with0.end(), without0.begin(), without0.begin() + 4);  // (mixed: a tile off row 0 after those on it)
  check_map("subset_row0", W, H, with0, tw, th, true);
  check_map("subset_no_row0", W, H, without0, tw, th, false);
  // the adaptive table's form, (x, y, pixel, 0) per entry: every third pixel of the frame's packed order
  for (int with_row0 = 0; with_row0 < 2; with_row0++) {
    std::vector<uint32_t> list;
    for (uint32_t p = 0; p < W * H; p += 3) {
      uint32_t x, y;
      tile_pixel(all.data(), tw, th, p, &x, &y);
      if (y == 0 && !with_row0) continue;
      const uint32_t e[4] = {x, y, p, 0u};
      list.insert(list.end(), e, e + 4);
    }
    check_map(with_row0 ? "list_1x1_row0" : "list_1x1_no_row0", W, H, list, 1, 1, with_row0 != 0);
  }
}

void means() {
  const uint32_t dividing[] = {IZPI_SAMPLER_NORMAL, IZPI_SAMPLER_COLOUR, IZPI_SAMPLER_WIREFRAME, IZPI_SAMPLER_ALBEDO};
  uint32_t s = 12345u, differing = 0, tried = 0;
  double dc = 0;
  uint32_t dn = 0;
  for (uint32_t n = 1; n <= 64; n++)
    for (int k = 0; k < 16; k++) {
      s = 1664525u * s + 1013904223u;
      const double c = (s / 4294967296.0) * 40.0;
      const double quotient = c / (double)n, product = c * (1.0 / (double)n);
      for (uint32_t sampler : dividing) EXPECT(bits(pixel_mean(sampler, c, n)) == bits(quotient), "mean");
      EXPECT(bits(pixel_mean(IZPI_SAMPLER_SPECTRAL, c, n)) == bits(product), "mean");
      EXPECT(mean_by_reciprocal(IZPI_SAMPLER_SPECTRAL) && !mean_by_reciprocal(IZPI_SAMPLER_COLOUR), "mean");
      tried++;
      if (bits(quotient) != bits(product)) {
        if (!differing) { dc = c; dn = n; }
        differing++;
      }
    }
  // not vacuous: a (c, n) where the two expressions differ in the last bit, and the samplers with them
  EXPECT(differing > 0, "mean");
  if (differing) {
    const double a = pixel_mean(IZPI_SAMPLER_COLOUR, dc, dn), b = pixel_mean(IZPI_SAMPLER_SPECTRAL, dc, dn);
    EXPECT(bits(a) != bits(b), "mean");
    EXPECT(bits(a) + 1 == bits(b) || bits(b) + 1 == bits(a), "mean");
    EXPECT(bits(pixel_mean(IZPI_SAMPLER_ALBEDO, dc, dn)) == bits(a), "mean");
  }
  printf("case mean: %u of %u (c, n) differ, the first at c=%.17g n=%u\n", differing, tried, dc, dn);
}

void view() {
  const std::vector<double> running = {1, 2, 3, 4, 5, 6}, moments = {7, 8, 9, 10, 11, 12};
  const std::vector<uint32_t> counts = {5, 9};
  SessionView v{};
  v.done = 16; v.running = running.data(); v.moments = moments.data();
  EXPECT(v.n(0) == 16 && v.n(1) == 16, "view");
  v.counts = counts.data();
  EXPECT(v.n(0) == 5 && v.n(1) == 9, "view");
  double sum[3], m2[3];
  v.load(1, sum, m2);
  EXPECT(sum[0] == 4 && sum[1] == 5 && sum[2] == 6 && m2[0] == 10 && m2[1] == 11 && m2[2] == 12, "view");
  printf("case view\n");
}

}  // namespace

int main() {
  maps();
  means();
  view();
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
