// render_plan_check.cpp — plan_workspace (izpi_amd/csrc/render_plan.cpp) on the sizes that
// matter (C3-C5 frames on a 288 GB device, budget-bound slots, several chunks, the floors)
// and on the small frames the GPU tests render, as a stand-alone program
// (tests/test_render_plan.py builds it under AddressSanitizer and UBSan). One line per case:
//   name|the inputs the test's properties need|the plan|the layout of the state allocation
// (key=value ...; -1: the array is absent),
// then `cache|...`: which changes of a request the plan cache takes for a new request.
#include <inttypes.h>
#include <stdio.h>

#include "../izpi_amd/csrc/render_plan.h"

using namespace izpi_internal;

namespace {

constexpr uint64_t GB288 = 288ull << 30;
constexpr uint32_t MP = 1024 * 1024;
constexpr uint32_t COL = IZPI_SAMPLER_COLOUR, SPE = IZPI_SAMPLER_SPECTRAL, NOR = IZPI_SAMPLER_NORMAL, ALB = IZPI_SAMPLER_ALBEDO,
                   WIR = IZPI_SAMPLER_WIREFRAME, REC = IZPI_ACC_RECURSIVE, FWD = IZPI_ACC_FORWARD;

struct Case {
  const char* name;
  PlanInput in;
};
// {pixels, size_spp, sampler, accumulation, max_depth, slots, chunk_units, rec_dense, pool_div, pool_grow,
//  tri_only, no_pathlen, any_uv, const_basic, avail}
const Case CASES[] = {
    // CASES-BEGIN
    // a Lambert / triangle-only scene without (u, v) textures (C3), 1024 x 1024
    {"colour_fwd_512", {MP, 512, COL, FWD, 50, 0, 0, 0, 0, 0, true, true, false, true, GB288}},
    {"colour_rec_compact_512", {MP, 512, COL, REC, 50, 0, 0, 0, 0, 0, true, true, false, true, GB288}},
    // glass + spheres + (u, v) textures (C5)
    {"spectral_rec_256", {MP, 256, SPE, REC, 50, 0, 0, 0, 0, 0, false, false, true, false, GB288}},
    {"spectral_fwd_4096", {MP, 4096, SPE, FWD, 50, 0, 0, 0, 0, 0, false, false, true, false, GB288}},
    {"spectral_rec_64_grow2", {MP, 64, SPE, REC, 50, 0, 0, 0, 0, 2, false, false, true, false, GB288}},
    // the budget below the per-sample results: the 1024-slot floor binds
    {"colour_fwd_512_avail_1g", {MP, 512, COL, FWD, 50, 0, 0, 0, 0, 0, true, true, false, true, 1ull << 30}},
    // the GPU tests' 40 x 30 frames
    {"small_rec_avail0", {1200, 5, COL, REC, 50, 0, 0, 0, 0, 0, true, true, false, true, 0}},
    {"small_fwd_slots2000_chunk3600", {1200, 5, COL, FWD, 50, 2000, 3600, 0, 0, 0, true, true, false, true, 0}},
    {"small_rec_dense1_div100000", {1200, 8, COL, REC, 50, 0, 0, 1, 100000, 0, true, true, false, true, 0}},
    {"small_rec_depth5", {1200, 4, COL, REC, 5, 0, 0, 0, 0, 0, true, true, false, true, 0}},
    // Colour's 40-B records (textured albedo), metal / PBR with spheres (C4)
    {"colour_rec_full_1024", {MP, 1024, COL, REC, 50, 0, 0, 0, 0, 0, false, true, true, false, GB288}},
    {"colour_fwd_textured_tri", {MP, 256, COL, FWD, 50, 0, 0, 0, 0, 0, true, true, true, false, GB288}},
    {"colour_rec_glass_tri", {MP, 128, COL, REC, 50, 0, 0, 0, 0, 0, true, false, false, false, GB288}},
    {"colour_rec_grow7", {MP, 128, COL, REC, 50, 0, 0, 0, 0, 7, true, true, false, true, GB288}},
    {"colour_rec_depth0", {1200, 2, COL, REC, 0, 0, 0, 0, 0, 0, true, true, false, true, GB288}},
    {"spectral_rec_dense64", {1200, 4, SPE, REC, 50, 0, 0, 64, 0, 0, true, true, false, false, GB288}},
    {"small_slots300", {1200, 5, COL, FWD, 50, 300, 0, 0, 0, 0, true, true, false, true, GB288}},
    {"tiny_slots300", {100, 4, COL, FWD, 50, 300, 0, 0, 0, 0, true, true, false, true, GB288}},
    {"colour_rec_one_sample_chunks", {MP, 3, COL, REC, 50, 0, MP + 5, 0, 0, 0, true, true, false, true, 1ull << 28}},
    // the preview samplers
    {"normal_512", {MP, 512, NOR, 0, 0, 0, 0, 0, 0, 0, true, true, false, true, GB288}},
    {"albedo_spheres_uv_1024", {MP, 1024, ALB, 0, 0, 0, 0, 0, 0, 0, false, false, true, false, GB288}},
    {"albedo_tri_uv_256", {MP, 256, ALB, 0, 0, 0, 0, 0, 0, 0, true, true, true, false, GB288}},
    {"wireframe_512", {MP, 512, WIR, 0, 0, 0, 0, 0, 0, 0, true, true, false, true, GB288}},
    {"wireframe_spheres_uv_4096", {MP, 4096, WIR, 0, 0, 0, 0, 0, 0, 0, false, false, true, false, GB288}},
    {"normal_512_avail_1g", {MP, 512, NOR, 0, 0, 0, 0, 0, 0, 0, true, true, false, true, 1ull << 30}},
    {"wireframe_spheres_avail_8g", {MP, 64, WIR, 0, 0, 0, 0, 0, 0, 0, false, true, false, true, 8ull << 30}},
    {"small_wireframe_chunk3600_slots1024", {1200, 5, WIR, 0, 0, 1024, 3600, 0, 0, 0, true, true, false, true, GB288}},
    {"small_wireframe_avail0", {1200, 5, WIR, 0, 0, 0, 0, 0, 0, 0, true, true, false, true, 0}},
    {"small_normal_slots300", {1200, 3, NOR, 0, 0, 300, 0, 0, 0, 0, true, true, false, true, GB288}},
    {"tiny_albedo_slots300", {100, 1, ALB, 0, 0, 300, 0, 0, 0, 0, true, true, false, true, GB288}},
    // CASES-END
};

void print_side(int k, const SideLayout& s) {
  const struct { const char* n; uint64_t v; } f[] = {{"ray", s.ray}, {"kind", s.kind}, {"time", s.time}, {"path", s.path},
                                                      {"blk", s.blk}, {"cold", s.cold}, {"hit", s.hit}, {"thr", s.thr},
                                                      {"tminmax", s.tminmax}};
  for (const auto& a : f) printf(" s%d.%s=%" PRId64, k, a.n, a.v == SideLayout::ABSENT ? (int64_t)-1 : (int64_t)a.v);
}

void print_plan(const char* name, const PlanInput& in, const WorkspacePlan& p) {
  printf("%s|pixels=%u size_spp=%u avail=%" PRIu64 "|chunk=%u slots=%u rec_dense=%u rec_pool=%u pool_div=%u pool_blocks=%u pool_shift=%u D=%u compact=%d thr_planes=%u "
         "sides=%u time=%d blk=%d cold=%d uv=%d tminmax=%d samples=%" PRIu64 " recs=%" PRIu64 " pool=%" PRIu64 " ring=%" PRIu64
         " running=%" PRIu64 " state=%" PRIu64,
         name, in.num_pixels, in.size_spp, in.avail, p.chunk, p.slots, p.rec_dense, p.rec_pool, p.pool_div, p.pool_blocks, p.pool_shift, p.D, (int)p.compact,
         p.thr_planes, p.sides, (int)p.time, (int)p.blk, (int)p.cold, (int)p.uv, (int)p.tminmax, p.samples_bytes, p.recs_bytes,
         p.pool_bytes, p.ring_bytes, p.running_bytes, p.state_bytes);
  printf("|");
  for (uint32_t k = 0; k < p.sides; k++) print_side((int)k, p.side[k]);
  printf("\n");
}

}  // namespace

int main() {
  for (const Case& c : CASES) print_plan(c.name, c.in, plan_workspace(c.in));
  // the cache: a plan made for `a` serves a request that differs in `avail` alone
  const PlanInput a = CASES[1].in;
  PlanCache cache;
  const bool empty_misses = cache.find(a) == nullptr;
  cache.store(a, plan_workspace(a));
  PlanInput avail = a, grow = a, acc = a, slots = a, chunk = a, dense = a, div = a, spp = a, px = a, depth = a, sampler = a;
  avail.avail = 1ull << 30; grow.pool_grow = 1; acc.accumulation = FWD; slots.slots = 4096; chunk.chunk_units = 1u << 20;
  dense.rec_dense = 4; div.pool_div = 8; spp.size_spp = 64; px.num_pixels = 1200; depth.max_depth = 10; sampler.sampler = SPE;
  const WorkspacePlan* hit = cache.find(avail);
  const bool reused = hit && hit->slots == plan_workspace(a).slots && hit->slots != plan_workspace(avail).slots;
  printf("cache|empty_misses=%d same=%d avail=%d pool_grow=%d accumulation=%d slots=%d chunk_units=%d rec_dense=%d pool_div=%d "
         "size_spp=%d num_pixels=%d max_depth=%d sampler=%d",
         (int)empty_misses, (int)(cache.find(a) != nullptr), (int)reused, (int)(cache.find(grow) != nullptr),
         (int)(cache.find(acc) != nullptr), (int)(cache.find(slots) != nullptr), (int)(cache.find(chunk) != nullptr),
         (int)(cache.find(dense) != nullptr), (int)(cache.find(div) != nullptr), (int)(cache.find(spp) != nullptr),
         (int)(cache.find(px) != nullptr), (int)(cache.find(depth) != nullptr), (int)(cache.find(sampler) != nullptr));
  cache.valid = false;  // (an allocation failure, a scene upload)
  printf(" invalidated=%d\n", (int)(cache.find(a) != nullptr));
  return 0;
}
