// displace_host.cpp — izpi_host_displace: the DISPLACE geometry operator on the host, the
// plain sequential restatement of displacement.ApplyDisplacementMap
// (displacement/displacement.go:143-280) from the arithmetic in displace.h. It is the twin
// the device path (displace.hip) is tested against, and what izpi_scene_to_input uses when
// no device was handed over. No HIP here: a host compiler builds it alone.
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <new>
#include <string>
#include <vector>

#include "displace.h"

namespace izpi_internal {
void set_host_error(const std::string& s);
}

namespace {

// Work-list bytes one call may hold (both lists of a level): a request beyond it is refused,
// not attempted.
constexpr uint64_t kHostMaxBytes = 8ull << 30;

// applyTessellation + applyDisplacement over `in` as one mesh: level-synchronous, outputs
// level-major, within a level the parents' order times child 0..3. Appends to `out` when
// it is given; counts[src] is always advanced.
int run_mesh(std::vector<izpi_tri_in> in, const dsp::Map& m, double dmin, double dmax, std::vector<izpi_tri_in>* out,
             uint64_t* total, uint64_t* counts, std::string& err) {
  const double max_du = dsp::max_delta(m.w), max_dv = dsp::max_delta(m.h);
  std::vector<izpi_tri_in> next;
  for (int level = 1; !in.empty(); level++) {
    if (level > IZPI_DISPLACE_MAX_LEVELS) {
      err = dsp::cap_message();
      return IZPI_ERR_UNSUPPORTED;
    }
    if ((uint64_t)in.size() * 4 * sizeof(izpi_tri_in) > kHostMaxBytes) {
      err = "displace: the next level's work list could need more than 8 GiB on the host";
      return IZPI_ERR_UNSUPPORTED;
    }
    next.clear();
    for (const izpi_tri_in& parent : in) {
      dsp::Six s;
      dsp::six_points(parent, s);
      double d[6];
      const uint32_t done = dsp::done_mask(s, m, max_du, max_dv, dmin, dmax, d);
      for (int c = 0; c < 4; c++) {
        izpi_tri_in child;
        dsp::make_child(s, c, parent, child);
        if ((done >> c) & 1u) {
          if (counts) counts[parent.pad]++;
          (*total)++;
          if (out) {
            izpi_tri_in o;
            dsp::displace(child, d[dsp::child_point(c, 0)], d[dsp::child_point(c, 1)], d[dsp::child_point(c, 2)], dmin,
                          dmax, o);
            out->push_back(o);
          }
        } else {
          next.push_back(child);
        }
      }
    }
    in.swap(next);
  }
  return IZPI_OK;
}

}  // namespace

extern "C" int izpi_host_displace(const izpi_tri_in* tris, uint64_t n, const double* rgba, uint32_t width,
                                  uint32_t height, double dmin, double dmax, uint32_t order, izpi_tri_in* out,
                                  uint64_t cap, uint64_t* n_out, uint64_t* counts, double* ms) {
  if (n_out) *n_out = 0;
  if (ms) *ms = 0.0;
  if (const char* bad = dsp::check_args(tris, n, rgba, width, height, order, n_out)) {
    izpi_internal::set_host_error(bad);
    return IZPI_ERR_INVALID;
  }
  try {
    const auto t0 = std::chrono::steady_clock::now();
    const dsp::Map m{rgba + 2, width, height, 4};
    if (counts) memset(counts, 0, n * sizeof(uint64_t));
    std::vector<izpi_tri_in> result;
    std::vector<izpi_tri_in>* sink = out ? &result : nullptr;
    std::string err;
    uint64_t total = 0;
    std::vector<izpi_tri_in> work;
    int rc = IZPI_OK;
    if (order == IZPI_DISPLACE_MESH) {
      work.assign(tris, tris + n);
      for (uint64_t i = 0; i < n; i++) { work[i].pad = (uint32_t)i; }
      rc = run_mesh(std::move(work), m, dmin, dmax, sink, &total, counts, err);
    } else {
      for (uint64_t i = 0; i < n && rc == IZPI_OK; i++) {
        work.assign(1, tris[i]);
        work[0].pad = (uint32_t)i;
        rc = run_mesh(work, m, dmin, dmax, sink, &total, counts, err);
      }
    }
    if (rc) {
      izpi_internal::set_host_error(err);
      return rc;
    }
    *n_out = total;
    if (out) {
      if (total > cap) {
        izpi_internal::set_host_error("displace: the output holds " + std::to_string(cap) + " triangles, " +
                                      std::to_string(total) + " are needed");
        return IZPI_ERR_INVALID;
      }
      if (total) memcpy(out, result.data(), total * sizeof(izpi_tri_in));
    }
    if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return IZPI_OK;
  } catch (const std::bad_alloc&) {
    izpi_internal::set_host_error("out of host memory");
    return IZPI_ERR_INVALID;
  }
}
