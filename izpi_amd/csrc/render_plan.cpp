// render_plan.cpp — plan_workspace (render_plan.h): plain integer arithmetic, no HIP.
#include "render_plan.h"

#include <algorithm>

namespace izpi_internal {

namespace {
using namespace plan_size;

// The sides of the state, `slots` entries per array, in one allocation: fills side[] (when
// given) from the plan's flags and returns the bytes.
uint64_t lay_out(const WorkspacePlan& p, uint32_t slots, SideLayout* side) {
  uint64_t off = 0;
  auto take = [&](bool present, uint64_t entry_bytes) {
    if (!present) return SideLayout::ABSENT;
    const uint64_t at = off;
    off += (slots * entry_bytes + 255) & ~255ull;
    return at;
  };
  for (uint32_t k = 0; k < p.sides; k++) {
    SideLayout s;
    s.ray = take(true, RAY);
    s.kind = take(true, sizeof(uint32_t));
    s.time = take(p.time, sizeof(double));
    s.path = take(p.sides == 2, PATH_HOT);
    s.blk = take(p.blk, sizeof(uint32_t));
    s.cold = take(p.cold, PATH_COLD);
    // with (u, v): one 32-B record per entry, (t, prim) then (u, v), so a finished ray's
    // two stores land in one line (two separate arrays made C4 / C5 trace 6-7% slower)
    s.hit = take(true, HIT * (p.uv ? 2 : 1));
    s.thr = take(p.thr_planes != 0, p.thr_planes * sizeof(double));
    s.tminmax = take(p.tminmax, HIT);
    if (side) side[k] = s;
  }
  return off;
}
}  // namespace

bool same_request(const PlanInput& a, const PlanInput& b) {
  return a.num_pixels == b.num_pixels && a.size_spp == b.size_spp && a.sampler == b.sampler &&
         a.accumulation == b.accumulation && a.max_depth == b.max_depth && a.slots == b.slots &&
         a.chunk_units == b.chunk_units && a.rec_dense == b.rec_dense && a.pool_div == b.pool_div &&
         a.pool_grow == b.pool_grow && a.tri_only == b.tri_only && a.no_pathlen == b.no_pathlen && a.any_uv == b.any_uv &&
         a.const_basic == b.const_basic;
}

// Sizing against the HBM this context may use (`avail`: what is free plus the render buffers
// it holds and would release, shared evenly by the contexts of one process on this device).
WorkspacePlan plan_workspace(const PlanInput& in) {
  WorkspacePlan p{};
  const bool spectral = in.sampler == IZPI_SAMPLER_SPECTRAL;
  const bool path = spectral || in.sampler == IZPI_SAMPLER_COLOUR;  // else: Normal, Albedo, WireFrame
  const bool fwd = path && in.accumulation == IZPI_ACC_FORWARD;
  // The render workspace stays within 15/32 of the HBM (~135 GB of 288, under the ~137 GB
  // C3 takes at its slot cap): per-sample results within 1/8, the wavefront state in the
  // rest. At 17/32 C4 took 153 GB, and a fresh process allocating it right after processes
  // of ~131-137 GB waited 0.4-3.9 s for the driver to clear VRAM (first frame up to 6.6x
  // steady); at 113 GB it allocated in 2 ms and its steady frame was 0.7% slower.
  // Per-sample results wait in HBM ([units][3] doubles) until k_accumulate folds them in
  // sample order. One chunk per request when it fits in 1/8 of the HBM (C3: 12.9 GB of
  // 288 GB), so the wavefront drains once per frame instead of once per chunk (C4 at 1024
  // spp: 2 chunks, C5 at 4096 spp: 12; a chunk's drain costs a few ms).
  uint64_t max_units = std::max<uint64_t>(64ull << 20, (in.avail / 8) / (SMP_D * sizeof(double)));
  if (in.chunk_units) max_units = in.chunk_units;
  // the chunks of a request are balanced: as many as the limit needs, equal in size (C4 at
  // 1024 spp: 2 chunks of 512 instead of 774 + 250, 13 GB less to allocate, same drains)
  p.chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(in.size_spp, max_units / in.num_pixels));
  const uint32_t nchunks = (in.size_spp + p.chunk - 1) / p.chunk;
  p.chunk = (in.size_spp + nchunks - 1) / nchunks;
  p.sides = path ? 2 : 1;
  p.time = !in.tri_only;  // only sphere tests read the ray time
  // a hit's (u, v) array: read by (u, v)-reading textures and, for spheres, the root (A16)
  p.uv = !in.tri_only || in.any_uv;
  p.tminmax = in.sampler == IZPI_SAMPLER_WIREFRAME;  // its second traversal's (tMin, tMax)
  uint64_t per_slot, per_block = 0;
  if (path) {
    // Unwinding records: the first rec_dense levels per slot, deeper levels in overflow
    // blocks (ShadeParams::rec_pool). Colour records are 40 B (24 B compact), spectral 24 B.
    p.compact = !fwd && !spectral && in.const_basic;
    p.D = spectral ? REC_SPECTRAL : p.compact ? REC_COMPACT : REC_COLOUR;
    const uint32_t max_depth = std::max(1u, in.max_depth);
    // Spectral glass paths run deep (C5: 12 rays per sample): with 16 dense levels the first
    // frame parked 15% of its shading items on an empty overflow pool; 32 levels park none
    // (C5 256 spp first frame 8854 -> 8130 ms; 92 GB of workspace, less than a pool twice the
    // size would take).
    p.rec_dense = spectral ? 32u : 8u;
    if (in.rec_dense) p.rec_dense = in.rec_dense;
    p.rec_dense = std::min(p.rec_dense, max_depth);
    if (fwd) p.rec_dense = max_depth;  // (no records at all: recs_bytes and the pool below)
    p.rec_pool = max_depth - p.rec_dense;
    p.blk = p.rec_pool != 0;
    // IZPI_ACC_FORWARD: the throughput per entry instead of the records (3 planes Colour, 1 Spectral)
    p.thr_planes = fwd ? (spectral ? 1u : 3u) : 0u;
    // PathCold (wavelength, dielectric point) is read only by the spectral sampler and glass
    p.cold = spectral || !in.no_pathlen;
    const uint64_t rec_bytes_slot = fwd ? 0 : (uint64_t)p.rec_dense * p.D * sizeof(double);
    // (the blk word is counted whether or not a pool exists)
    per_slot = 2 * (RAY + sizeof(uint32_t) + (p.time ? sizeof(double) : 0) + PATH_HOT + sizeof(uint32_t) +
                    (p.cold ? PATH_COLD : 0) + HIT * (p.uv ? 2 : 1) + p.thr_planes * sizeof(double)) +
               rec_bytes_slot;
    // Overflow blocks per slot. Lambert/light scenes: 1 per 16 slots (C3: ~3% of the paths
    // in flight are deeper than 8). Scenes with glass or the spectral sampler run deep
    // chains through glass: 1 per 4 slots (C5 at 1 per 16 parked 29% of its
    // shading items, 574 -> 502 ms per 16-spp frame with no parks at 1 per 4). A frame that
    // still parks more than 1/64 of its rays doubles the pool for the renderer's next frame.
    // Metal / PBR scenes without glass stay at 1 per 16: C4's paths (1.85 rays per sample)
    // park none, and 1 per 4 allocated 56 GB of pool there (a second of a first frame on
    // boxes whose driver clears memory as it maps it).
    p.pool_div = p.cold ? 4u : 16u;
    p.pool_div = std::max(1u, p.pool_div >> std::min(in.pool_grow, 4u));
    if (in.pool_div) p.pool_div = in.pool_div;
    per_block = (uint64_t)p.rec_pool * p.D * sizeof(double) + sizeof(uint32_t);
    // The overflow pool rounds up to a power of two per ring, up to twice slots / pool_div
    // blocks: counted at that worst case (C4 at 256M slots otherwise took 271 GB of the 288).
    per_slot += 2 * per_block / p.pool_div + 1;
    p.recs_bytes = rec_bytes_slot;  // (times slots, below)
  } else {
    per_slot = lay_out(p, 1024, nullptr) / 1024 + 1;
  }
  // Paths in flight per wavefront pass. Larger = fewer k_trace/k_shade launches and
  // a smaller share of launch tails.
  // C3 per frame (round 2, tiered records): 40M slots 349 ms, 100M 334, 160M 326, 250M 320
  // (fewer passes and pass tails; the first frame, fresh allocations included, is faster
  // too: 371 ms at 40M, 349 ms at 250M); C5 at 64 spp 120M slots: -6%; C4 100M: -3%.
  // The wavefront state takes the rest of the workspace budget: C3 keeps its 256M slots
  // (135 GB); C5 at 128 spp ran 1.4% faster at 64M slots than at 118M (less state, better
  // cache and TLB reach in k_shade), so the smaller budget costs the deep-path scenes nothing.
  uint64_t slot_cap = 256ull << 20;
  if (in.slots) slot_cap = std::max<uint64_t>(1024, in.slots);
  p.samples_bytes = (uint64_t)in.num_pixels * p.chunk * SMP_D * sizeof(double);
  const uint64_t budget = in.avail / 32 * 15;
  if (in.avail > 0)
    slot_cap = std::min<uint64_t>(slot_cap, std::max<uint64_t>(1024, (budget > p.samples_bytes ? budget - p.samples_bytes : 0) / per_slot));
  p.slots = (uint32_t)std::min<uint64_t>((uint64_t)in.num_pixels * p.chunk, slot_cap);
  if (p.rec_pool) {  // POOL_SHARDS rings of a power of two each, at least 16 blocks per ring
    p.pool_blocks = POOL_SHARDS * 16;
    while (p.pool_blocks < p.slots / p.pool_div && p.pool_blocks < (1u << 30)) p.pool_blocks <<= 1;
    while ((POOL_SHARDS << p.pool_shift) < p.pool_blocks) p.pool_shift++;
  }
  p.recs_bytes *= p.slots;
  p.pool_bytes = (uint64_t)p.pool_blocks * p.rec_pool * p.D * sizeof(double);
  p.ring_bytes = (uint64_t)p.pool_blocks * sizeof(uint32_t);
  p.running_bytes = (uint64_t)in.num_pixels * 3 * sizeof(double);
  p.state_bytes = lay_out(p, p.slots, p.side);
  return p;
}

}  // namespace izpi_internal
