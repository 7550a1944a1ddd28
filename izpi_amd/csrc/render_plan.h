// render_plan.h — the workspace of one render call, decided from plain numbers: chunking,
// slot count, record tiers, overflow pool, which per-entry arrays exist, every render
// buffer's bytes and the layout of the state allocation. Plain C++ (no HIP,
// no izpi_ctx): the driver in izpi_gpu.hip reads the free memory, allocates what the plan
// says and turns its offsets into pointers, so a host compiler can build and check the
// arithmetic on its own (tests/render_plan_check.cpp).
#pragma once
#include <stdint.h>

#include "../../include/izpi_gpu.h"

namespace izpi_internal {

// The sizes of the device records the plan counts, pinned against the real types where those
// are declared (izpi_runtime.h).
namespace plan_size {
constexpr uint64_t RAY = 48;        // RayOD
constexpr uint64_t PATH_HOT = 16;   // PathHot
constexpr uint64_t PATH_COLD = 48;  // PathCold
constexpr uint64_t HIT = 16;        // a hit record: (t, primitive); with (u, v) two of them
constexpr uint32_t SMP_D = 3;       // doubles per per-sample result
constexpr uint32_t POOL_SHARDS = 256;
constexpr uint32_t REC_COLOUR = 5, REC_COMPACT = 3, REC_SPECTRAL = 3;  // RecLayout<...>::D
}  // namespace plan_size

// Everything the decision reads, and nothing else.
struct PlanInput {
  uint32_t num_pixels;    // of the request's tiles
  uint32_t size_spp;      // the samples sized for: the request's, or a session's step_spp
  uint32_t sampler;       // IZPI_SAMPLER_*
  uint32_t accumulation;  // IZPI_ACC_*   (the preview samplers ignore it and max_depth, the
  uint32_t max_depth;     //               record tuning and pool_grow: their caller passes 0)
  uint32_t slots, chunk_units, rec_dense, pool_div;  // izpi_render_tuning's sizing fields
  uint32_t pool_grow;     // overflow pool doublings earned by frames that parked
  bool tri_only, no_pathlen, any_uv;  // of the scene
  bool const_basic;       // basic_materials && const_albedo: Colour's compact records
  uint64_t avail;         // bytes this context may use; 0: the free-memory reading failed
};
// Equal apart from `avail`: the cached plan serves, without reading the free memory.
bool same_request(const PlanInput& a, const PlanInput& b);

// One side of the wavefront state: byte offsets into the state allocation, ABSENT for an
// array this render does not have. Every array holds `slots` entries and starts 256-B aligned.
struct SideLayout {
  static constexpr uint64_t ABSENT = ~0ull;
  uint64_t ray, kind, time, path, blk, cold, hit, thr, tminmax;
};

struct WorkspacePlan {
  uint32_t chunk;        // samples per chunk, balanced over the chunks of size_spp
  uint32_t slots;        // paths in flight (entries per side)
  uint32_t rec_dense, rec_pool;  // record levels per slot / per overflow block (forward, preview: max_depth / 0, no records)
  uint32_t pool_div, pool_blocks, pool_shift;
  uint32_t D;            // doubles per record
  bool compact;          // Colour's MATSET_CONST records
  uint32_t thr_planes;   // IZPI_ACC_FORWARD: throughput planes per entry
  uint32_t sides;        // 2, or 1 for the preview samplers (no path arrays)
  bool time, blk, cold, uv, tminmax;  // the per-entry arrays beyond ray, kind, hit (and path)
  uint64_t samples_bytes, recs_bytes, pool_bytes, ring_bytes, running_bytes, state_bytes;
  SideLayout side[2];
};

// The path samplers (Colour, Spectral) and the preview samplers (Normal, Albedo, WireFrame):
// the same budget and chunk rule; a preview plan has one side of state without path arrays,
// records or pool, plus tminmax for WireFrame.
WorkspacePlan plan_workspace(const PlanInput& in);

// The plan of a context's last render and what it was decided for: a request of the same
// shape reuses it, so frames of one renderer never re-size (sizing from the free HBM of each
// frame made C4 reallocate its 148 GB every frame, 2 s each). An allocation failure and a
// scene upload clear `valid`.
struct PlanCache {
  bool valid = false;
  PlanInput in{};
  WorkspacePlan plan{};
  const WorkspacePlan* find(const PlanInput& q) const { return valid && same_request(q, in) ? &plan : nullptr; }
  void store(const PlanInput& q, const WorkspacePlan& p) { valid = true; in = q; plan = p; }
};

}  // namespace izpi_internal
