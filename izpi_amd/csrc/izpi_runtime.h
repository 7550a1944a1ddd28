// izpi_runtime.h — the host side of libizpi_gpu.so that its HIP translation units share: the
// context, the parameter blocks of the smaller kernels (each embeds pixel_map.h's PixelMap, and
// those of a session's kernels its SessionView), and what the units call across each other:
//   izpi_gpu.hip    the context, scene upload, the buffers, the one-context render call
//                   (render_plan.cpp: its workspace plan, plain C++);
//   session.hip     progressive sessions on one context, their noise estimate and stop rule;
//   multi.hip       the share plan, device groups in one process (and their sessions), RCCL ranks;
//   components.hip  post-processing and the component entries the tests call;
//   trace.hip, wavefront.hip, preview.hip, resolve.hip, noise.hip, adapt.hip, denoise.hip,
//   checkpoint.hip: the kernels a render, a filter or a session's checkpoint runs, each with
//   its launch code.
// The shade_*.hip units need none of this (izpi_kern.h). Not part of the ABI.
#pragma once
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/izpi_host.h"
#include "../../include/izpi_gpu_debug.h"
#include "izpi_kern.h"
#include "izpi_req.h"
#include "pixel_map.h"
#include "checkpoint.h"
#include "render_plan.h"

namespace izpi_bvh {  // bvh_build.hip
int build(hipStream_t st, const double* h_boxes, uint32_t n, uint32_t leaf_max, uint32_t method,
          std::vector<izpi_bvh4_node>& nodes, std::vector<uint32_t>& order, float* ms, std::string& err);
}

// ================================================================ host side (shared)
constexpr uint32_t CPART_BLOCKS_PER_CU = 16;  // counter rows per CU / 4: above any resident 256-thread grid
// The per-pixel kernels read where a request's pixels lie and, for a session, its sums from two
// blocks they all embed (pixel_map.h): PixelMap, the pixels of a request in packed order and
// their output slots, and SessionView, a session's map with its samples done, sampler, running
// sums, second moments and per-pixel counts (session.hip builds it in one place).
// Per-pixel sequential sum of the chunk's samples (render/rgb.go:36 col += ...,
// render/spectral.go:164-166 sum += ...), in sample order; finalize on the last chunk
// (pixel_mean of the request's sampler, store_pixel). An adaptive session's step over its
// active list: map.num_pixels is the list's entries.
struct AccumParams {
  PixelMap map;
  uint32_t chunk_spp, spp, sampler, last;
  uint32_t raw_spectral;  // the samples are (radiance, lambda, pdf): weigh each (spectral_weigh) before summing
  const double* samples;  // [num_pixels][chunk_spp][3]
  double* running;        // [num_pixels][3]
  double* out;
};
// The samples one run of the chunk loops renders (run_wavefront, run_preview). A one-shot render:
// [0, req->spp), and the chunk that ends it divides and scatters (AccumParams::last). A step
// of a progressive session: [begin, end) with keep set: every chunk is folded into the running
// sums with last = 0, and k_resolve reads them.
struct SampleRange {
  uint32_t begin, end;
  bool keep;
};
// k_resolve (resolve.hip): a snapshot of the running sums after view.n(p) samples, in the
// layout of k_accumulate's last chunk.
struct ResolveParams {
  SessionView view;
  uint32_t form;    // IZPI_SNAP_*
  double exposure;  // IZPI_SNAP_DISPLAY of the Spectral sampler
  double* out;
};
void launch_resolve(hipStream_t st, const ResolveParams& rp);
// k_noise_resolve and k_noise_stats (noise.hip): the noise estimate of a session begun with
// IZPI_PROG_NOISE, from its sums and second moments after view.n(p) >= 2 samples (noise.h;
// DESIGN.md section 3.9).
struct NoiseParams {
  SessionView view;
  double threshold, floor;  // k_noise_stats
  double* out;            // k_noise_resolve: (se_0, se_1, se_2, 1.0) per pixel, in k_resolve's layout
  double* block_sums;     // k_noise_stats: v[0] of each 256-pixel block, [ceil(num_pixels / 256)]
  unsigned long long* block_counts;  // k_noise_stats: each block's pixels, nonfinite, above and the bits of its largest e, [blocks][4]
};
void launch_noise_resolve(hipStream_t st, const NoiseParams& np);
void launch_noise_stats(hipStream_t st, const NoiseParams& np);
// k_adapt_select, k_adapt_scan and k_adapt_scatter (adapt.hip): izpi_gpu_progressive_adapt of a
// session begun with IZPI_PROG_ADAPTIVE (noise.h). The rule is evaluated
// at view.done, whatever view.counts holds; the arrays it writes are the context's d_adapt (AdaptBufs).
struct AdaptParams {
  SessionView view;
  uint32_t blocks;  // ceil(view.map.num_pixels / 256)
  double threshold, floor;
  uint32_t* counts;       // [num_pixels]: n_p, the samples in pixel p's sums
  uint8_t* state;         // [num_pixels]: 0 active, 1 retired, 2 retired as a counted non-finite pixel
  uint32_t* table;        // [num_pixels][4]: the active list in packed order, (x, y, pixel, 0) per entry: the 1 x 1 tiles of a step
  uint32_t* block_keep;   // [blocks]: k_adapt_select: each block's survivors; k_adapt_scan: the survivors before the block
  uint32_t* block_stat;   // [blocks][2]: each block's counted and (counted) non-finite pixels
  uint32_t* totals;       // [4]: active, counted, non-finite, 0
};
void launch_adapt(hipStream_t st, const AdaptParams& ap);
// ... and a resumed session's active list from the state bytes a checkpoint stored: k_adapt_select_state
// counts where k_adapt_select evaluates the rule (retirement is final, and the thresholds of the
// earlier adapt calls are not stored), then k_adapt_scan and k_adapt_scatter as they are.
void launch_adapt_restore(hipStream_t st, const AdaptParams& ap);
// k_ckpt_gather, k_ckpt_scatter and k_ckpt_claimed (checkpoint.hip): a
// session's state between the packed order of its tiles and the frame-order planes of a
// checkpoint in the context's staging buffer (d_ckpt: CkptBufs).
struct CkptParams {
  PixelMap map;
  ck::Packed packed;
  ck::Planes planes;
  uint32_t* block_counts;  // k_ckpt_scatter: [ceil(num_pixels / 256)] pixels without a record; k_ckpt_claimed: [ceil(W * H / 256)] claimed records
};
void launch_ckpt_gather(hipStream_t st, const CkptParams& cp);
void launch_ckpt_scatter(hipStream_t st, const CkptParams& cp);
void launch_ckpt_claimed(hipStream_t st, const CkptParams& cp);
// d_ckpt for a W x H frame and a session of `pixels` pixels: the blob's planes as they lie behind
// its header (one copy moves them), the claimed marks, the blocks' counts.
struct CkptBufs {
  size_t planes, claimed, block_counts, bytes;
  CkptBufs(const ck::Layout& l, size_t pixels) {
    auto up = [](size_t v) { return (v + 15) / 16 * 16; };
    planes = 0;
    claimed = up(l.bytes - sizeof(ck::Header));
    block_counts = claimed + up(l.n);
    bytes = block_counts + up(((std::max<size_t>(pixels, l.n) + 255) / 256) * 4);
  }
};
// d_adapt of `pixels` pixels: the five arrays above at 16-B aligned offsets.
struct AdaptBufs {
  size_t counts, state, table, block_keep, block_stat, totals, bytes;
  explicit AdaptBufs(size_t pixels) {
    auto up = [](size_t v) { return (v + 15) / 16 * 16; };
    const size_t blocks = (pixels + 255) / 256;
    table = 0;
    counts = table + pixels * 16;
    block_keep = counts + up(pixels * 4);
    block_stat = block_keep + up(blocks * 4);
    totals = block_stat + up(blocks * 8);
    state = totals + 16;
    bytes = state + up(pixels);
  }
};
// ================================================================ host side
// The record sizes the workspace planner counts with (render_plan.h), against the real types.
static_assert(sizeof(RayOD) == izpi_internal::plan_size::RAY && sizeof(PathHot) == izpi_internal::plan_size::PATH_HOT &&
                  sizeof(PathCold) == izpi_internal::plan_size::PATH_COLD && sizeof(double2) == izpi_internal::plan_size::HIT,
              "render_plan.h: entry records");
static_assert(SMP_D == izpi_internal::plan_size::SMP_D && POOL_SHARDS == izpi_internal::plan_size::POOL_SHARDS,
              "render_plan.h: per-sample results, pool rings");
static_assert(RecLayout<IZPI_SAMPLER_COLOUR, MATSET_FULL>::D == izpi_internal::plan_size::REC_COLOUR &&
                  RecLayout<IZPI_SAMPLER_COLOUR, MATSET_CONST>::D == izpi_internal::plan_size::REC_COMPACT &&
                  RecLayout<IZPI_SAMPLER_SPECTRAL, MATSET_FULL>::D == izpi_internal::plan_size::REC_SPECTRAL,
              "render_plan.h: record strides");
// Scratch device buffers of one ABI call, freed when it returns (on every path).
struct DevBufs {
  std::vector<void*> p;
  template <typename T>
  hipError_t alloc(T** out, size_t count) {
    *out = nullptr;
    const hipError_t e = hipMalloc((void**)out, count * sizeof(T));
    if (e == hipSuccess) p.push_back(*out);
    return e;
  }
  ~DevBufs() {
    for (void* q : p) (void)hipFree(q);
  }
};

struct izpi_ctx {
  int device = 0;
  std::string err;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  int num_cus = 0;
  // scene
  bool have_scene = false;
  uint32_t num_textures = 0;     // of the uploaded scene (izpi_gpu_gomath texture lookups)
  uint32_t num_materials = 0;    // of the uploaded scene
  uint32_t num_spd = 0;          // tabulated SPD entries of the uploaded scene
  // The workspace plan of the last render per sampler family, [0] Colour / Spectral, [1] the
  // preview samplers (render_plan.h): a Colour frame and a preview frame alternating on one
  // context do not evict each other's.
  izpi_internal::PlanCache plans[2];
  const GTriVerts* d_triverts = nullptr;  // [num_prims], leaf order: the triangles' v1, v2 (WireFrame's edge test); a scene allocation
  DevScene sc{};
  uint32_t stack_needed = 0;
  uint32_t num_prims = 0;
  std::vector<void*> scene_allocs;
  size_t scene_bytes = 0;
  // render workspace (grown on demand)
  double* d_samples = nullptr; size_t samples_cap = 0;
  double* d_recs = nullptr; size_t recs_cap = 0;
  double* d_pool = nullptr; size_t pool_cap = 0;       // overflow unwinding records
  uint32_t* d_ring = nullptr; size_t ring_cap = 0;     // free ring of overflow blocks
  unsigned long long* d_pool_ctr = nullptr;            // ring counters, [POOL_SHARDS][POOL_CTR_STRIDE]
  double* d_running = nullptr; size_t running_cap = 0;
  double* d_out = nullptr; size_t out_cap = 0;
  uint32_t* d_tiles = nullptr; size_t tiles_cap = 0;
  uint32_t* d_utiles = nullptr; size_t utiles_cap = 0;  // tile lists of k_unpack (multi-GPU root)
  double* d_bg = nullptr; size_t bg_cap = 0;
  uint32_t* d_misc = nullptr;              // words k * MISC_STRIDE (misc()): 0 unit head, 1 error, 2 trace cursor, 3..4 queue counts, 6..7 park flags
  unsigned long long* d_counters = nullptr;
  unsigned long long* d_cpart = nullptr; size_t cpart_cap = 0;  // per-wave counter rows of a render (count_add)
  unsigned long long* d_finq = nullptr; size_t finq_cap = 0;  // k_shade blocks' deferred unwinding jobs (fin_flush)
  char* d_state = nullptr; size_t state_cap = 0;      // the sides of the wavefront state (WorkspacePlan::side)
  int32_t* d_spill = nullptr; size_t spill_cap = 0;  // traversal-stack spill area of k_trace2
  double* d_post = nullptr; size_t post_cap = 0;      // spectral post-processing output
  double* d_share = nullptr; size_t share_cap = 0;    // multi-GPU: this device's packed tiles
  double* d_gather = nullptr; size_t gather_cap = 0;  // multi-GPU root: every device's packed tiles
  double* d_denoise = nullptr; size_t denoise_cap = 0;  // the two denoisers' scratch canvas (denoise.hip; it only grows)
  double* d_dnvar = nullptr; size_t dnvar_cap = 0;  // izpi_gpu_denoise_var_device's two variance planes (denoise.hip; it only grows)
  double* d_demod = nullptr; size_t demod_cap = 0;  // IZPI_DENOISE_DEMODULATE's demodulated canvas D_0 (denoise.hip; it only grows)
  // a session begun with IZPI_PROG_NOISE (noise.hip; both only grow, and no workspace plan counts them):
  double* d_moments = nullptr; size_t moments_cap = 0;  // the samples' second moments, [num_pixels][3]
  double* d_noisepart = nullptr; size_t noisepart_cap = 0;  // k_noise_stats' block partials: [blocks] sums, then [blocks][4] counts
  // a session begun with IZPI_PROG_ADAPTIVE (adapt.hip; AdaptBufs; as above, it only grows and no plan counts it):
  char* d_adapt = nullptr; size_t adapt_cap = 0;  // the per-pixel sample counts, the retirements, the active list
  // a session's checkpoint or resume (checkpoint.hip; CkptBufs): allocated by the first of either, it only grows
  char* d_ckpt = nullptr; size_t ckpt_cap = 0;
  uint32_t* h_count = nullptr;                        // pinned readback of d_misc (unit head, queue lengths; same stride) + scratch
  hipEvent_t ev3 = nullptr;
  hipEvent_t evb[3 * IZPI_PASS_BATCH] = {};
  // RCCL communicator of a multi-process render (izpi_gpu_comm_init), or null
  ncclComm_t comm = nullptr;
  // izpi_gpu_debug_fault 3: the pinned word a stalled stream waits on (null when none)
  volatile uint32_t* stall_word = nullptr;
  uint32_t* stall_host = nullptr;  // its allocation (coherent pinned host memory)
  uint32_t comm_rank = 0, comm_size = 1;
  int32_t* d_status = nullptr;   // agreement word of izpi_gpu_render_rank ([0] in, [1] max over ranks)
  int fault_inject = 0;          // izpi_gpu_debug_fault: 1 fail before rendering, 2 fail the render
  izpi_render_stats last{};
  bool mat_ok_rgb = false, mat_ok_spectral = false;
  bool basic_materials = false;  // only Lambertian + DiffuseLight: use the MATSET_BASIC shader
  uint32_t matset = 0;           // MS_* bits of the scene's material kinds
  bool const_albedo = false;     // ... and every albedo / emit texture a constant RGB: MATSET_CONST (Colour)
  bool any_uv = false;           // a material reads the hit's (u, v) (image textures)
  // The scene's shading instances, [Spectral][forward] (shade_instance, resolved at upload: what
  // is prepared is what renders); null where the scene lacks the sampler's textures.
  const ShadeKernels* kernels[2][2] = {};
  uint32_t pool_grow = 0;        // overflow pool doublings earned by frames that parked (render_impl)
  uint32_t dev_share = 1;        // contexts of this process on this device (izpi_gpu_multi_open): they split its HBM
  // Progress of the running render (izpi_gpu_progress, read from other threads): samples
  // whose paths have finished, as of the host's last queue poll, and the request's samples.
  std::atomic<uint64_t> prog_done{0}, prog_total{0};
  // The progressive session of this context (izpi_gpu_progressive_*), when open: the
  // library's copy of the request (req.spp is the cap N; its arrays are the vectors here),
  // the samples done, and the statistics summed over the steps.
  struct Session {
    bool open = false;
    bool broken = false;  // a step failed: the sums are not those of `done` samples
    izpi_render_req req{};
    izpi_render_tuning tuning{};
    std::vector<uint32_t> tiles;  // the request's own list (may be empty: the whole frame)
    std::vector<double> bg_wl, bg_val;
    uint32_t step_spp = 0, done = 0;
    bool noise = false;  // IZPI_PROG_NOISE: the steps fold the second moments into d_moments
    // IZPI_PROG_ADAPTIVE: `active` pixels still take samples, each with n_p == done;
    // `listed` once a pixel has retired: the steps run over the active list and the snapshots
    // read the per-pixel counts. samples = the sum of n_p over the session's pixels.
    bool adaptive = false, listed = false;
    uint32_t active = 0;
    uint64_t samples = 0;
    // filled by render_body: the tiles rendered, their extent and pixels
    std::vector<uint32_t> run_tiles;
    uint32_t tile_w = 0, tile_h = 0, num_pixels = 0;
    izpi_render_stats cum{};
  } session;
};

// The words of d_misc lie MISC_STRIDE words (256 B) apart: the unit head and the queue
// counts take one returning atomic each per shading block-iteration (~11M per C3 frame),
// and atomics on one line are served one at a time (a single word saturates near 88 per
// microsecond, MI355X_MICROARCH.md "dequeue").
inline uint32_t* misc(izpi_ctx* ctx, int k) { return ctx->d_misc + (size_t)k * MISC_STRIDE; }

template <typename K>
inline int resident_blocks(izpi_ctx* ctx, K kernel, int* blocks, int threads = 256, size_t dyn_lds = 0) {
  int per_cu = 0;
  if (dyn_lds) HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, dyn_lds));
  if (per_cu < 1) per_cu = 1;
  *blocks = per_cu * ctx->num_cus;
  return IZPI_OK;
}

// Traversal kernel selection: k_trace2 with a 16-entry LDS stack ring and global spill,
// 5 waves/SIMD. Instances: DIST (leaf tests spread over the wave; off only when primitive
// indices do not fit the 26-bit LDS packing, or IZPI_TUNE_NO_DIST) x TRI (sphere code
// compiled out for triangle-only scenes; IZPI_TUNE_GENERAL_TRACE forces the general one).
// izpi_render_tuning: prim_weight (default 32) weighs primitive steps against node steps
// (x/16); trace_chunk queue entries per dequeue; refill_min idle lanes per refill. All
// settings give identical results and counters.
constexpr int TRACE_RING = 16, TRACE_WPE = 5;
struct Tracer {
  bool p2 = true;    // DIST
  bool tri = false;  // TRI
  bool lds_bvh = false;  // LB
  bool ray_lds = false;  // RL
  bool qnodes = false;   // Q
  bool a32 = false;      // A32 (the BVH-in-LDS instances read no record from global memory: compiled without)
  bool leaf3 = false;    // L3 (the distributed-leaf instances)
  // queue entries per dequeue and idle lanes per refill, measured on C3: chunk 128 / refill
  // 16 -> 211 ms of k_trace2 per frame, 512 / 24 -> 201, 1024 -> 207, 2048 -> 216, 64 -> 303
  uint32_t prim_w = 32, tchunk = 512, refill_min = 24;
  int blocks = 0;
  size_t spill_bytes = 0;  // the per-thread traversal-stack spill area this launch needs
};

// (the request's tuning across ABI versions: tuning_of, izpi_req.h)
const izpi_render_tuning kDefaultTuning{};

// trace.hip: pick the k_trace2 instance and its grid (no allocation: the caller grows d_spill
// to t->spill_bytes; need_uv: the caller reads the hits' (u, v), WaveParams::hit_uv), and
// launch it for one pass.
int make_tracer(izpi_ctx* ctx, const izpi_render_tuning& tu, bool need_uv, Tracer* t);
void launch_trace(izpi_ctx* ctx, const DevScene& sc, const Tracer& t, const WaveParams& wp, hipStream_t st, int32_t* spill);
int trace_ring(const Tracer& t);  // entries of the instance's LDS stack ring (deeper stacks spill)
// What a run of the chunk loops (run_wavefront, run_preview) is given: the pixels of the request's
// tiles, the samples per pixel and chunk, the overflow record blocks (the path samplers), the
// sample range; and what it reports: the device times of its passes and their number.
// An adaptive session's step over its active list (SampleRange::keep): num_pixels entries of
// `list` (AdaptParams::table), k_accumulate's scatter instance with `counts`; its progress
// starts at samples_before samples. A null list: every other run.
struct RunInput {
  uint32_t num_pixels, chunk, pool_blocks; SampleRange range;
  const uint32_t* list = nullptr; uint32_t* counts = nullptr; uint64_t samples_before = 0;
};
struct RunTimes { float trace_ms = 0, shade_ms = 0, tail_ms = 0; uint32_t launches = 0; };
// wavefront.hip: the shading instance a scene runs, the smallest that holds its material kinds
// (matset: its MS_* bits; const_basic: Lambertian + DiffuseLight with constant albedos, whose
// recursive Colour renders write compact records); every chunk of the request through the
// wavefront passes with the kernels of k; the code of those kernels (and of k_accumulate)
// loaded ahead of the first frame (izpi_gpu_upload_scene); k_accumulate's launch.
const ShadeKernels* shade_instance(uint32_t matset, bool const_basic, uint32_t sampler, bool fwd);
int run_wavefront(izpi_ctx* ctx, const izpi_render_req* req, const DevScene& sc, const Tracer& tr, const ShadeKernels& k,
                  ShadeParams& sp, WaveParams& wp, AccumParams& ap, const RunInput& in, RunTimes* out);
int prepare_wavefront(izpi_ctx* ctx, const ShadeKernels& k);
int prepare_accumulate(izpi_ctx* ctx);
void launch_accumulate(hipStream_t st, const AccumParams& ap, double* moments = nullptr);
// ... and of its scatter instance: entry j of `list` adds its samples to pixel list[4 * j + 2]'s
// sums and moments and ap.chunk_spp to its count (ap.num_pixels entries; never the last chunk).
void launch_accumulate_list(hipStream_t st, const AccumParams& ap, double* moments, const uint32_t* list, uint32_t* counts);
// The moments k_accumulate folds besides the sums: those of a noise session's steps, else none
// (the present instance runs).
inline double* session_moments(const izpi_ctx* ctx, const SampleRange& r) {
  return r.keep && ctx->session.noise ? ctx->d_moments : nullptr;
}
// preview.hip: the Normal, Albedo and WireFrame samplers (sampler/normal.go, albedo.go,
// wireframe.go): one primary ray per sample, no path state. The request's units run in
// batches of `slots`: k_preview_start writes the batch's camera rays into `buf` (start_path),
// k_trace2 traces them in place, k_preview writes each sample's result; WireFrame re-enqueues
// every hit with tMax = t + 2^-52 in buf.tminmax and traces and tests the batch once more
// (HitableSlice.HitEdge's two traversals). k_accumulate folds each chunk as for Colour.
struct PreviewParams {
  WaveBuf buf;            // one side of state: ray, kind, time, hit (+ (u, v)); no path state
  double2* tminmax;       // WireFrame: (tMin, tMax) of the second traversal, per entry; else null
  const GTriVerts* verts; // izpi_ctx::d_triverts
  double ink[3];          // WireFrame: the edge colour (the paper is ShadeParams::background)
  uint32_t slots;         // entries of buf
};
int run_preview(izpi_ctx* ctx, const izpi_render_req* req, const DevScene& sc, const Tracer& tr, ShadeParams& sp,
                const PreviewParams& pp, AccumParams& ap, const RunInput& in, RunTimes* out);
// preview.hip: load the code of the preview kernels (izpi_gpu_upload_scene)
int prepare_preview(izpi_ctx* ctx);
inline bool preview_sampler(uint32_t s) {
  return s == IZPI_SAMPLER_NORMAL || s == IZPI_SAMPLER_ALBEDO || s == IZPI_SAMPLER_WIREFRAME;
}
// Diagnostics (IZPI_TUNE_PASS_LOG): host milliseconds on a process-wide steady clock.
inline double diag_clock_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ================================================================ across the runtime's units
namespace izpi_internal { struct PackedScene; }  // scene_pack.h
// (hidden: the library exports none of these)
#pragma GCC visibility push(hidden)
namespace izpi_internal {

// ---- izpi_gpu.hip: buffers, tiles, scene upload in its two steps, the render call
int grow(izpi_ctx* ctx, void** p, size_t* cap, size_t bytes);
uint32_t validate_tiles(const izpi_render_req* req, const uint32_t* tiles, uint32_t n, uint32_t* tw, uint32_t* th);
int request_tiles(izpi_ctx* ctx, const izpi_render_req* req, std::vector<uint32_t>& tiles);
int begin_upload(izpi_ctx* ctx, const izpi_scene_desc* d);
int upload_packed(izpi_ctx* ctx, const izpi_scene_desc* d, const PackedScene& ps);
// How a render call is driven: the samples it renders, the samples its workspace is sized
// for (the request's, or a progressive session's step_spp: the sums then stay in d_running),
// and whether it stops once the workspace is allocated (izpi_gpu_prepare, a session's begin).
// list: an adaptive session's step over the `list_count` entries of its device-built active
// list instead of the request's tiles (AdaptParams::table; counts: the pixels' sample counts;
// samples_before: what the session has rendered). The workspace is the one planned for all pixels.
struct RenderCall {
  SampleRange range;
  uint32_t size_spp;
  bool prepare_only;
  const uint32_t* list = nullptr;
  uint32_t* counts = nullptr;
  uint32_t list_count = 0;
  uint64_t samples_before = 0;
};
inline RenderCall one_shot(const izpi_render_req* req, bool prepare_only = false) {
  const uint32_t spp = req ? req->spp : 0;
  return RenderCall{SampleRange{0, spp, false}, spp, prepare_only};
}
int render_body(izpi_ctx* ctx, const izpi_render_req* req, const RenderCall& call, double* out_dev);
int render_impl(izpi_ctx* ctx, const izpi_render_req* req, const RenderCall& call, double* out_dev);
// A progressive session owns the context's running sums, counters and progress: the calls
// that would overwrite them are refused while it is open.
inline bool session_open(izpi_ctx* ctx) {
  if (!ctx->session.open) return false;
  ctx->err = "a progressive session is open";
  return true;
}
// A host caller's output through d_out: grown to `bytes` and filled from the caller's buffer
// (untouched pixels keep their values); after the device call, back to it, synchronised.
int output_from_host(izpi_ctx* ctx, const double* out_host, size_t bytes);
int output_to_host(izpi_ctx* ctx, double* out_host, size_t bytes);

// ---- components.hip: Render's post-processing of a whole-frame canvas on the context's stream
int apply_post(izpi_ctx* ctx, const izpi_render_req* req, double* canvas_dev);

// ---- session.hip: a context's progressive session (izpi_gpu_progressive_*)
int session_copy_request(izpi_ctx::Session& ss, const izpi_render_req* req, std::string& err);
void session_drop(izpi_ctx* ctx);
int session_begin(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp, uint32_t flags);
int session_step(izpi_ctx* ctx, uint32_t spp, izpi_render_stats* stats);
int session_noise(izpi_ctx* ctx, const izpi_noise_params* params, izpi_noise_stats* out);
int session_adapt(izpi_ctx* ctx, const izpi_noise_params* params, izpi_adapt_stats* out);
int session_snapshot(izpi_ctx* ctx, uint32_t form, double* out_dev);
// The session's checkpoint into out_host (cap bytes), and a session begun from one. share: a
// device of a group installs its own share's pixels: records of other shares may be left over
// (the group checks the frame's pixel set), and the counters are the blob's or (zero_counters) zero.
int session_checkpoint_bytes(izpi_ctx* ctx, uint64_t* bytes);
int session_checkpoint(izpi_ctx* ctx, uint64_t scene_tag, void* out_host, uint64_t cap);
int session_resume(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp, uint64_t scene_tag, const void* blob,
                   uint64_t bytes, bool share = false, bool zero_counters = false);
// The checks a context's session and a group's share (each true / false with the message in err).
bool session_lacks_noise(const izpi_ctx::Session& ss, std::string& err, uint32_t need = 2);
bool noise_params_ok(const izpi_noise_params* params, izpi_noise_params& p, std::string& err);
bool snapshot_form_ok(uint32_t form, uint32_t done, std::string& err);
bool session_lacks_adaptive(const izpi_ctx::Session& ss, std::string& err);
// converge on an adaptive session: step(step_spp), then adapt once done >= max(2, min_spp), until
// the frame rule holds or the cap is reached. A step that leaves done where it was found no
// active pixel (an earlier adapt retired them all, at any done >= 2): nothing is left to render,
// and the loop ends there (*idle), whatever min_spp is.
template <class Step, class Adapt, class Done>
int adapt_loop(const izpi_noise_params& p, uint32_t cap, Step step, Adapt adapt, Done done, izpi_adapt_stats* out, bool* idle) {
  izpi_adapt_stats last{};
  int rc = IZPI_OK;
  *idle = false;
  while (!rc && done() < cap) {
    const uint32_t before = done();
    if ((rc = step())) break;
    if (done() == before) { *idle = true; break; }
    if (done() < std::max(2u, p.min_spp)) continue;
    if ((rc = adapt(p, &last))) break;
    if (last.converged) break;
  }
  if (out) *out = last;
  return rc;
}
// converge: step(step_spp), then the statistic once done >= max(2, min_spp), until the frame is
// converged or the cap is reached. `step` and `noise` are the session's own (one context or
// the devices of a group); done() reads its samples; p is checked (noise_params_ok).
template <class Step, class Noise, class Done>
int converge_loop(const izpi_noise_params& p, uint32_t cap, Step step, Noise noise, Done done, izpi_noise_stats* out) {
  izpi_noise_stats last{};
  int rc = IZPI_OK;
  while (!rc && done() < cap) {
    if ((rc = step())) break;
    if (done() < std::max(2u, p.min_spp)) continue;
    if ((rc = noise(p, &last))) break;
    if (last.converged) break;
  }
  if (out) *out = last;
  return rc;
}

// ---- multi.hip: izpi_gpu_prepare on a rank of a communicator: the workspace of its share
int prepare_rank_share(izpi_ctx* ctx, const izpi_render_req* req);
}  // namespace izpi_internal
#pragma GCC visibility pop
