// izpi_gpu.hip — the one-context core of the C ABI (include/izpi_gpu.h): contexts, scene upload,
// the device buffers and the render call (its workspace is planned in render_plan.cpp).
// Progressive sessions are in session.hip, multi-GPU in multi.hip, post-processing and the
// component entries in components.hip (izpi_runtime.h); the kernels of the hot path are in
// trace.hip and shade.hip (izpi_kern.h).
#include "izpi_runtime.h"
#include "scene_pack.h"

#include <array>

using namespace izpi_internal;

// End of frame: counters[k] += the sum of column k of the per-wave rows (count_add).
__global__ void __launch_bounds__(256) k_cpart_reduce(const unsigned long long* cpart, uint32_t rows,
                                                      unsigned long long* counters) {
  __shared__ unsigned long long red[256];
  unsigned long long v = 0;
  for (uint32_t r = threadIdx.x; r < rows; r += 256) v += cpart[(size_t)r * CNT_N + blockIdx.x];
  red[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) counters[blockIdx.x] += red[0];
}

namespace izpi_internal {
int grow(izpi_ctx* ctx, void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return IZPI_OK;
  if (*p) HIP_TRY(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  HIP_TRY(hipMalloc(p, bytes));
  *cap = bytes;
  return IZPI_OK;
}

uint32_t validate_tiles(const izpi_render_req* req, const uint32_t* tiles, uint32_t n, uint32_t* tw, uint32_t* th) {
  if (n == 0) return 0;
  *tw = tiles[2] - tiles[0] + 1;
  *th = tiles[3] - tiles[1] + 1;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t* t = tiles + 4 * i;
    if (t[2] < t[0] || t[3] < t[1] || t[2] >= req->width || t[3] >= req->height) return 0;
    if (t[2] - t[0] + 1 != *tw || t[3] - t[1] + 1 != *th) return 0;
  }
  return n;
}

// The request's tiles: its own list, or the whole frame in common.Tiles steps and
// grid.WalkGrid's spiral order (tiles.go:6-24, renderer.go:172-188).
int request_tiles(izpi_ctx* ctx, const izpi_render_req* req, std::vector<uint32_t>& tiles) {
  if (req->num_tiles) {
    if (!req->tiles) { ctx->err = "num_tiles without tiles"; return IZPI_ERR_INVALID; }
    tiles.assign(req->tiles, req->tiles + 4 * (size_t)req->num_tiles);
    return IZPI_OK;
  }
  tiles.resize(4 * ((size_t)req->width * req->height / 16 + 16));
  const uint32_t nt = izpi_host_tiles(req->width, req->height, tiles.data(), (uint32_t)(tiles.size() / 4));
  if (nt == 0) { ctx->err = "image size not divisible by any common.Tiles step"; return IZPI_ERR_INVALID; }
  tiles.resize(4 * (size_t)nt);
  return IZPI_OK;
}

// A host caller's output through d_out (izpi_gpu_render, izpi_gpu_progressive_snapshot).
int output_from_host(izpi_ctx* ctx, const double* out_host, size_t bytes) {
  const int rc = grow(ctx, (void**)&ctx->d_out, &ctx->out_cap, bytes);
  if (rc) return rc;
  // start from the caller's buffer so untouched pixels keep their values
  HIP_TRY(hipMemcpyAsync(ctx->d_out, out_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  return IZPI_OK;
}
int output_to_host(izpi_ctx* ctx, double* out_host, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(out_host, ctx->d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return IZPI_OK;
}
}  // namespace izpi_internal

namespace {

template <typename T>
int dev_upload(izpi_ctx* ctx, const T* host, size_t count, T** out) {
  *out = nullptr;
  if (count == 0) return IZPI_OK;
  HIP_TRY(hipMalloc((void**)out, count * sizeof(T)));
  ctx->scene_allocs.push_back(*out);
  ctx->scene_bytes += count * sizeof(T);
  if (host) HIP_TRY(hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice));
  return IZPI_OK;
}
#define UP(ptr, n, dst)                                   \
  do {                                                    \
    int rc_ = dev_upload(ctx, ptr, (size_t)(n), dst);     \
    if (rc_) return rc_;                                  \
  } while (0)

// Every device buffer `grow` manages. The first RENDER_BUFS are the ones a render sizes per
// frame and may release to re-size (not the output, share, gather and post-processing
// buffers, which it never frees), in the order of izpi_gpu_debug_realloc's mask bits.
struct CtxBuf {
  void** p;
  size_t* cap;
};
constexpr size_t RENDER_BUFS = 7, CTX_BUFS = 23;
std::array<CtxBuf, CTX_BUFS> ctx_buffers(izpi_ctx* c) {
#define IZPI_BUF(name) CtxBuf{(void**)&c->d_##name, &c->name##_cap}
  return {IZPI_BUF(samples), IZPI_BUF(recs), IZPI_BUF(pool), IZPI_BUF(ring), IZPI_BUF(running), IZPI_BUF(state),
          IZPI_BUF(spill), IZPI_BUF(out), IZPI_BUF(tiles), IZPI_BUF(utiles), IZPI_BUF(bg), IZPI_BUF(post),
          IZPI_BUF(share), IZPI_BUF(gather), IZPI_BUF(cpart), IZPI_BUF(finq), IZPI_BUF(denoise),
          IZPI_BUF(moments), IZPI_BUF(noisepart), IZPI_BUF(adapt), IZPI_BUF(dnvar), IZPI_BUF(ckpt),
          IZPI_BUF(demod)};
#undef IZPI_BUF
}
uint64_t buffer_bytes(izpi_ctx* ctx, size_t n) {
  uint64_t sum = 0;
  const auto bufs = ctx_buffers(ctx);
  for (size_t i = 0; i < n; i++) sum += *bufs[i].cap;
  return sum;
}
// Device bytes of the render workspace, and of the buffers a render may release to re-size.
uint64_t workspace_bytes(izpi_ctx* ctx) { return buffer_bytes(ctx, CTX_BUFS); }
uint64_t render_buffer_bytes(izpi_ctx* ctx) { return buffer_bytes(ctx, RENDER_BUFS); }

// Make each of the first RENDER_BUFS buffers at least its `bytes`: if any must grow, free them
// all first, then allocate each at exactly its size.
int grow_render_buffers(izpi_ctx* ctx, const CtxBuf* b, const size_t* bytes, bool* fresh) {
  const size_t n = RENDER_BUFS;
  for (size_t i = 0; i < n; i++)  // a buffer this render does not use (the records of IZPI_ACC_FORWARD)
    if (bytes[i] == 0 && *b[i].p) {
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      HIP_TRY(hipFree(*b[i].p));
      *b[i].p = nullptr;
      *b[i].cap = 0;
    }
  bool must = false;
  for (size_t i = 0; i < n; i++) must = must || *b[i].cap < bytes[i];
  *fresh = must;
  if (!must) return IZPI_OK;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; i++) {
    if (*b[i].p) HIP_TRY(hipFree(*b[i].p));
    *b[i].p = nullptr;
    *b[i].cap = 0;
  }
  for (size_t i = 0; i < n; i++) {
    if (bytes[i] == 0) continue;
    const hipError_t e = hipMalloc(b[i].p, bytes[i]);
    if (e != hipSuccess) {
      *b[i].p = nullptr;
      ctx->err = "render workspace: hipMalloc of " + std::to_string(bytes[i]) + " bytes: " + hipGetErrorString(e);
      return IZPI_ERR_HIP;
    }
    *b[i].cap = bytes[i];
  }
  return IZPI_OK;
}

// One side of the wavefront state at its place in izpi_ctx::d_state.
WaveBuf bind_side(char* base, const WorkspacePlan& plan, const SideLayout& s) {
  auto at = [base](uint64_t off) { return off == SideLayout::ABSENT ? nullptr : base + off; };
  WaveBuf w{};
  w.ray = (RayOD*)at(s.ray);
  w.kind = (uint32_t*)at(s.kind);
  w.time = (double*)at(s.time);
  w.path = (PathHot*)at(s.path);
  w.blk = (uint32_t*)at(s.blk);
  w.cold = (PathCold*)at(s.cold);
  w.hs = plan.uv ? 2u : 1u;  // (t, prim) and (u, v) interleaved
  w.hit = (double2*)at(s.hit);
  w.huv = plan.uv ? w.hit + 1 : nullptr;
  w.thr = (double*)at(s.thr);
  w.tplane = plan.slots;
  return w;
}

void free_scene(izpi_ctx* ctx) {
  for (void* p : ctx->scene_allocs) (void)hipFree(p);
  ctx->scene_allocs.clear();
  ctx->scene_bytes = 0;
  ctx->have_scene = false;
}

// A step of a progressive session finds the workspace its begin allocated: were a buffer to
// be re-allocated (`moved`), the running sums would go with it.
int session_keeps_sums(izpi_ctx* ctx, const RenderCall& call, bool moved) {
  if (!call.range.keep || call.prepare_only || !moved) return IZPI_OK;
  ctx->err = "progressive step: the session's workspace no longer fits (its sums would be lost)";
  return IZPI_ERR_INVALID;
}

// counter rows: one per wave of the largest grid (run_wavefront and run_preview check the grids against it)
uint32_t cpart_rows(const izpi_ctx* ctx) { return ctx->num_cus * CPART_BLOCKS_PER_CU * 4u; }

// ---- render_body's steps, shared by the path samplers and the preview samplers
// 1. The request against the ABI and the scene; what the later steps need of it.
struct RequestShape {
  std::vector<uint32_t> tiles;
  uint32_t tw = 0, th = 0, num_pixels = 0;
  bool fwd = false;      // IZPI_ACC_FORWARD (never with a preview sampler: they ignore the accumulation, as max_depth)
  bool preview = false;  // Normal, Albedo, WireFrame
};
int check_request(izpi_ctx* ctx, const izpi_render_req* req, RequestShape* rs) {
  if (ctx->fault_inject == 2) { ctx->err = "injected render fault (izpi_gpu_debug_fault)"; return IZPI_ERR_DEVICE; }
  if (!ctx->have_scene) { ctx->err = "render before izpi_gpu_upload_scene"; return IZPI_ERR_NO_SCENE; }
  if (!req || req->width == 0 || req->height == 0 || req->spp == 0) { ctx->err = "invalid render request"; return IZPI_ERR_INVALID; }
  if (req->abi_version > IZPI_ABI_VERSION) { ctx->err = "render request from a newer ABI"; return IZPI_ERR_INVALID; }
  rs->preview = preview_sampler(req->sampler);
  if (req->sampler != IZPI_SAMPLER_COLOUR && req->sampler != IZPI_SAMPLER_SPECTRAL && !rs->preview) { ctx->err = "unsupported sampler"; return IZPI_ERR_UNSUPPORTED; }
  // (a request of ABI 1 or 2 ends at `tuning`: accumulation is not read)
  const uint32_t acc = rs->preview ? (uint32_t)IZPI_ACC_RECURSIVE : req->abi_version >= 3 ? req->accumulation : (uint32_t)IZPI_ACC_RECURSIVE;
  if (acc != IZPI_ACC_RECURSIVE && acc != IZPI_ACC_FORWARD) { ctx->err = "unknown accumulation mode"; return IZPI_ERR_INVALID; }
  rs->fwd = acc == IZPI_ACC_FORWARD;
  if (req->post != IZPI_POST_NONE &&
      ((req->post & ~(uint32_t)(IZPI_POST_SPECTRAL | IZPI_POST_GAMMA_CLAMP)) || req->out_layout != IZPI_OUT_CANVAS ||
       req->num_tiles != 0)) {
    ctx->err = "post-processing needs a whole-frame IZPI_OUT_CANVAS request";
    return IZPI_ERR_INVALID;
  }
  if (rs->preview && (req->post & IZPI_POST_SPECTRAL)) {
    ctx->err = "IZPI_POST_SPECTRAL needs the Spectral sampler's XYZ canvas";
    return IZPI_ERR_INVALID;
  }
  // Normal and WireFrame read no material texture but the normal maps; Albedo reads Colour's
  if (req->sampler == IZPI_SAMPLER_COLOUR || req->sampler == IZPI_SAMPLER_ALBEDO ? !ctx->mat_ok_rgb
      : req->sampler == IZPI_SAMPLER_SPECTRAL                                     ? !ctx->mat_ok_spectral
                                                                                  : false) {
    ctx->err = "a material lacks the textures this sampler reads";
    return IZPI_ERR_INVALID;
  }
  if (!rs->preview && ctx->sc.num_lights == 0) { ctx->err = "scene has no lights (HitableSlice.PDFValue divides by zero)"; return IZPI_ERR_INVALID; }
  const int rc = request_tiles(ctx, req, rs->tiles);
  if (rc) return rc;
  const uint32_t ntiles = validate_tiles(req, rs->tiles.data(), (uint32_t)(rs->tiles.size() / 4), &rs->tw, &rs->th);
  if (ntiles == 0) { ctx->err = "tiles must be non-empty, in bounds and equal-sized"; return IZPI_ERR_INVALID; }
  const uint64_t num_pixels64 = (uint64_t)ntiles * rs->tw * rs->th;
  if (num_pixels64 > (1ull << 30)) { ctx->err = "too many pixels in one request"; return IZPI_ERR_INVALID; }
  rs->num_pixels = (uint32_t)num_pixels64;
  ctx->prog_total.store(num_pixels64 * req->spp, std::memory_order_relaxed);
  if (ctx->stack_needed > 64) { ctx->err = "BVH deeper than the 64-entry traversal stack (bvh4.go:71)"; return IZPI_ERR_UNSUPPORTED; }
  return IZPI_OK;
}

// 2. What plan_workspace reads of this call (render_plan.h), but for `avail`. The preview
// samplers' plans do not depend on the fields they ignore.
PlanInput plan_input(const izpi_ctx* ctx, const izpi_render_req* req, const RequestShape& rs, const izpi_render_tuning& tu,
                     uint32_t size_spp) {
  PlanInput in{};
  in.num_pixels = rs.num_pixels; in.size_spp = size_spp; in.sampler = req->sampler;
  in.slots = tu.slots; in.chunk_units = tu.chunk_units;
  in.tri_only = ctx->sc.tri_only; in.any_uv = ctx->any_uv;
  if (!rs.preview) {
    in.accumulation = rs.fwd ? IZPI_ACC_FORWARD : IZPI_ACC_RECURSIVE; in.max_depth = req->max_depth;
    in.rec_dense = tu.rec_dense; in.pool_div = tu.pool_div; in.pool_grow = ctx->pool_grow;
    in.no_pathlen = ctx->sc.no_pathlen; in.const_basic = ctx->basic_materials && ctx->const_albedo;
  }
  return in;
}
// The HBM this context may use: what is free plus the render buffers it holds and would
// release (a later frame reuses them, so every frame of a renderer sizes alike), shared
// evenly by the contexts of one process on this device. 0: the reading failed.
uint64_t available_bytes(izpi_ctx* ctx) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b == 0) return 0;
  return ((uint64_t)free_b + render_buffer_bytes(ctx)) / std::max(1u, ctx->dev_share);
}

// ... and its buffers. The path samplers: when a render buffer must grow, all are released
// before any is allocated, so a frame never holds an old buffer next to a new one (the plan
// counted every one of them as available). The preview samplers stay within the buffers a
// Colour render of this context may already hold: they only grow. A failed allocation drops
// the family's cached plan.
int allocate(izpi_ctx* ctx, const izpi_render_req* req, const RequestShape& rs, const WorkspacePlan& plan, const Tracer& tr,
             const RenderCall& call) {
  const auto bufs = ctx_buffers(ctx);
  const size_t bytes[RENDER_BUFS] = {plan.samples_bytes, plan.recs_bytes, plan.pool_bytes, plan.ring_bytes,
                                     plan.running_bytes, plan.state_bytes, tr.spill_bytes};
  int rc = IZPI_OK;
  if (rs.preview) {
    if ((rc = session_keeps_sums(ctx, call, ctx->running_cap < plan.running_bytes))) return rc;
    for (size_t k = 0; k < RENDER_BUFS && !rc; k++) rc = grow(ctx, bufs[k].p, bufs[k].cap, bytes[k]);
  } else {
    bool fresh = false;
    rc = grow_render_buffers(ctx, bufs.data(), bytes, &fresh);
    if (!rc && (rc = session_keeps_sums(ctx, call, fresh))) return rc;
  }
  if (!rc) rc = grow(ctx, (void**)&ctx->d_tiles, &ctx->tiles_cap, rs.tiles.size() * sizeof(uint32_t));
  if (!rc && !rs.preview) {  // (the preview samplers read no background SPD)
    if (req->num_bg_spd && (!req->bg_spd_wavelengths || !req->bg_spd_values)) { ctx->err = "num_bg_spd without the SPD arrays"; return IZPI_ERR_INVALID; }
    rc = grow(ctx, (void**)&ctx->d_bg, &ctx->bg_cap, (2 * (size_t)req->num_bg_spd + 1) * sizeof(double));
  }
  if (!rc) rc = grow(ctx, (void**)&ctx->d_cpart, &ctx->cpart_cap, (size_t)cpart_rows(ctx) * CNT_N * sizeof(unsigned long long));
  // deferred unwinding jobs: one queue per k_shade block (run_wavefront checks its grid against it)
  if (!rc && !rs.preview && !rs.fwd) rc = grow(ctx, (void**)&ctx->d_finq, &ctx->finq_cap, (size_t)ctx->num_cus * CPART_BLOCKS_PER_CU * FINQ_WORDS * FINQ_CAP * sizeof(unsigned long long));
  if (rc) ctx->plans[rs.preview].valid = false;
  return rc;
}

// 3. prepare_only (izpi_gpu_prepare, a session's begin): the device's first work on the fresh
// workspace (its first submission after a large allocation waited ~7 ms, and the kernels'
// first touch of its pages) happens here, in the renderer's setup, not in its first frame.
int touch_workspace(izpi_ctx* ctx, const WorkspacePlan& plan, const RenderCall& call, double alloc_ms) {
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemsetAsync(ctx->d_state, 0, plan.state_bytes, st));
  HIP_TRY(hipMemsetAsync(ctx->d_samples, 0, plan.samples_bytes, st));
  if (plan.recs_bytes) HIP_TRY(hipMemsetAsync(ctx->d_recs, 0, plan.recs_bytes, st));
  if (call.range.keep) {  // izpi_gpu_progressive_begin: the session's sums and counters start at zero
    HIP_TRY(hipMemsetAsync(ctx->d_running, 0, plan.running_bytes, st));
    HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, CNT_N * sizeof(unsigned long long), st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  ctx->last = izpi_render_stats{};
  ctx->last.workspace_bytes = workspace_bytes(ctx);
  ctx->last.slots = plan.slots; ctx->last.chunk_spp = plan.chunk; ctx->last.alloc_ms = alloc_ms;
  return IZPI_OK;
}

// 4. Begin frame: the tiles and the background SPD (nbg entries) to the device, the sums and
// counters zeroed (a session's run on from step to step).
int begin_frame(izpi_ctx* ctx, const izpi_render_req* req, const RequestShape& rs, const WorkspacePlan& plan, const RenderCall& call,
                size_t nbg) {
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemcpyAsync(ctx->d_tiles, rs.tiles.data(), rs.tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (nbg) {
    HIP_TRY(hipMemcpyAsync(ctx->d_bg, req->bg_spd_wavelengths, nbg * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->d_bg + nbg, req->bg_spd_values, nbg * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (!call.range.keep) {
    HIP_TRY(hipMemsetAsync(ctx->d_running, 0, plan.running_bytes, st));
    HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, CNT_N * sizeof(unsigned long long), st));
  }
  HIP_TRY(hipMemsetAsync(ctx->d_cpart, 0, (size_t)cpart_rows(ctx) * CNT_N * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(ctx->d_misc, 0, 8 * MISC_STRIDE * sizeof(uint32_t), st));
  return IZPI_OK;
}

// 5. The kernels' parameters. What every sampler's kernels read of ShadeParams ...
ShadeParams shade_params(izpi_ctx* ctx, const izpi_render_req* req, const RequestShape& rs, const WorkspacePlan& plan) {
  ShadeParams sp{};
  sp.width = req->width; sp.height = req->height; sp.tile_w = rs.tw; sp.tile_h = rs.th; sp.slots = plan.slots;
  // (the preview samplers ignore the request's; start_path completes a sample of max_depth 0 at once)
  sp.max_depth = rs.preview ? 1 : req->max_depth;
  sp.tiles = ctx->d_tiles; sp.seed = req->seed; sp.out = ctx->d_samples;
  sp.background[0] = req->background[0]; sp.background[1] = req->background[1]; sp.background[2] = req->background[2];
  sp.counters = ctx->d_counters; sp.cpart = ctx->d_cpart; sp.error = misc(ctx, 1);
  return sp;
}
// ... and what the path samplers' read besides: the background SPD, the records and their
// overflow pool, the scene's table sizes.
void path_shade_params(izpi_ctx* ctx, const izpi_render_req* req, const DevScene& sc, const RequestShape& rs,
                       const WorkspacePlan& plan, size_t nbg, ShadeParams& sp) {
  sp.num_bg_spd = (uint32_t)nbg;
  sp.bg_sorted = nbg >= 2;
  for (size_t i = 1; i < nbg; i++)
    if (!(req->bg_spd_wavelengths[i - 1] <= req->bg_spd_wavelengths[i])) sp.bg_sorted = 0;
  sp.bg_wl = ctx->d_bg; sp.bg_val = ctx->d_bg + nbg;
  sp.rec_dense = plan.rec_dense; sp.rec_pool = plan.rec_pool; sp.pool_shift = plan.pool_shift;
  sp.recs = rs.fwd ? nullptr : ctx->d_recs; sp.mat_const = sc.mat_const; sp.head = misc(ctx, 0);
  sp.num_mc = ctx->num_materials; sp.num_tex = ctx->num_textures; sp.num_spd = ctx->num_spd;
  sp.pool = plan.rec_pool ? ctx->d_pool : nullptr; sp.pool_ring = plan.rec_pool ? ctx->d_ring : nullptr;
  sp.pool_ctr = plan.rec_pool ? ctx->d_pool_ctr : nullptr;
  sp.finq = ctx->d_finq;
}
// Which of the scene's tables this render's k_shade / k_tail blocks copy into LDS
// (sp.staged, sp.prims_staged), and the LDS arena that takes (sc.lds_bytes).
void stage_tables(const izpi_ctx* ctx, const izpi_render_req* req, const izpi_render_tuning& tu, const RequestShape& rs,
                  const WorkspacePlan& plan, size_t nbg, DevScene& sc, ShadeParams& sp) {
  sp.staged = ctx->num_materials <= MC_LDS && ctx->num_materials <= MAT_LDS && sc.num_lights <= LT_LDS &&
              ctx->num_textures <= TEX_LDS && ctx->num_spd <= SPD_LDS && nbg <= BG_LDS;
  sp.prims_staged = sc.num_prims <= PR_LDS && !(tu.flags & IZPI_TUNE_NO_PRIM_LDS);
  if (sp.staged && (req->sampler == IZPI_SAMPLER_SPECTRAL || ctx->num_spd)) sp.staged = 2;  // + the Spectral tables
  // A forward Colour render of a Lambert / light scene (C1, C2) that could run k_shade's staged
  // form but for its primitives in LDS (the output stage lies behind the Colour tables, where
  // they would) leaves them in global memory: its hits read their 32-B GShade only, and C2's
  // shading at 256 spp measured 35.0-35.3 ms with the primitives in LDS, 34.3-34.4 without and
  // 30.3-30.4 without them in the staged form (run_wavefront; profiles/r7b/ab_stage_c2.jsonl).
  if (rs.fwd && req->sampler == IZPI_SAMPLER_COLOUR && ctx->matset == 0 && sp.staged == 1 && !plan.rec_pool && !plan.time &&
      !plan.cold && !(tu.flags & IZPI_TUNE_NO_SHADE_STAGE))
    sp.prims_staged = 0;
  // k_shade / k_tail's LDS arena: the prefix of lds_off's layout that this render stages
  sc.lds_bytes = sp.prims_staged ? lds_off::END : sp.staged == 2 ? lds_off::SPECTRAL_END : sp.staged ? lds_off::COLOUR_END : 0;
  if (tu.flags & IZPI_TUNE_PASS_LOG)  // diagnostics: which tables this render's k_shade / k_tail blocks copy into LDS
    fprintf(stderr, "IZPI_SHADE_TABLES tables=%u prims=%u lds_bytes=%u\n", sp.staged, sp.prims_staged, sc.lds_bytes);
}
WaveParams wave_params(izpi_ctx* ctx, const WorkspacePlan& plan, const ShadeParams& sp) {
  WaveParams wp{};
  wp.in = bind_side(ctx->d_state, plan, plan.side[0]); wp.out = bind_side(ctx->d_state, plan, plan.side[1]);
  wp.trace_next = misc(ctx, 2); wp.slots = plan.slots;
  // kind words other than plain main rays: path-length rays, parked entries
  wp.read_kind = !ctx->sc.no_pathlen ? 1u : 0u;  // parked entries: wp.in_park, per pass
  wp.hit_uv = plan.uv ? 1u : 0u;
  wp.pool_ctr = sp.pool_ctr;
  wp.cpart = ctx->d_cpart;
  return wp;
}
PreviewParams preview_params(izpi_ctx* ctx, const izpi_render_req* req, const WorkspacePlan& plan) {
  PreviewParams pp{};
  pp.buf = bind_side(ctx->d_state, plan, plan.side[0]);
  pp.tminmax = plan.tminmax ? (double2*)(ctx->d_state + plan.side[0].tminmax) : nullptr;
  pp.slots = plan.slots;
  pp.verts = ctx->d_triverts;
  if (req->abi_version >= 4)  // (a request of ABI 3 ends before `ink`: black)
    for (int k = 0; k < 3; k++) pp.ink[k] = req->ink[k];
  return pp;
}
AccumParams accum_params(izpi_ctx* ctx, const izpi_render_req* req, const RequestShape& rs, double* out_dev) {
  AccumParams ap{};
  ap.map = PixelMap{rs.num_pixels, req->width, req->height, rs.tw, rs.th, req->out_layout, ctx->d_tiles};
  ap.spp = req->spp; ap.sampler = req->sampler;
  ap.samples = ctx->d_samples; ap.running = ctx->d_running; ap.out = out_dev;
  return ap;
}

// 6. The device's error word (k_trace2 can set bit 1 alone; k_shade and k_tail the others).
int guard_status(izpi_ctx* ctx, uint32_t guard) {
  if (!guard) return IZPI_OK;
  ctx->err = guard & 1u   ? "device guard: traversal stack overflow"
             : guard & 2u ? "device guard: unknown material kind"
                            : "device guard: no overflow record block in k_tail";
  return IZPI_ERR_DEVICE;
}
}  // namespace

namespace izpi_internal {
// One render on one context, or (call.prepare_only) the allocation of its workspace: the
// steps above in turn, for every sampler.
int render_body(izpi_ctx* ctx, const izpi_render_req* req, const RenderCall& call, double* out_dev) {
  const auto t_body0 = std::chrono::steady_clock::now();
  auto host_ms = [&t_body0]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_body0).count(); };
  RequestShape rs;
  int rc = check_request(ctx, req, &rs);
  if (rc) return rc;
  const SampleRange& sr = call.range;
  const uint32_t num_pixels = rs.num_pixels;
  if (sr.keep) {
    izpi_ctx::Session& ss = ctx->session;
    ss.run_tiles = rs.tiles; ss.tile_w = rs.tw; ss.tile_h = rs.th; ss.num_pixels = num_pixels;
  }
  const izpi_render_tuning& tu = tuning_of(req);
  const bool pass_log = (tu.flags & IZPI_TUNE_PASS_LOG) != 0;
  // this render's view of the scene: the traversal shortcuts the tuning switches off
  DevScene sc = ctx->sc;
  if (tu.flags & IZPI_TUNE_NO_LEAF_SHORTCUT) sc.leaf_shortcut = 0;
  if (tu.flags & IZPI_TUNE_SCALAR_SLAB) sc.nan_free_bounds = 0;
  Tracer tr;
  const double t_tiles = host_ms();
  if ((rc = make_tracer(ctx, tu, !ctx->sc.tri_only || ctx->any_uv, &tr))) return rc;
  if (pass_log)  // diagnostics: the k_trace2 instance this render runs
    fprintf(stderr, "IZPI_TRACE_INSTANCE dist=%d tri=%d lds_bvh=%d ray_lds=%d q=%d\nIZPI_TRACE_ADDR a32=%d ring=%d\nIZPI_TRACE_LEAVES leaf_max=%u leaf3=%d tmin_fixed=%d\n", (int)tr.p2, (int)tr.tri,
            (int)tr.lds_bvh, (int)tr.ray_lds, (int)tr.qnodes, (int)(tr.a32 && !tr.lds_bvh), trace_ring(tr), ctx->sc.leaf_max, (int)tr.leaf3, (int)(ctx->sc.no_pathlen != 0));
  const double t_tracer = host_ms();
  // Plan: the family's cached plan when the request has its shape, else from the free memory.
  PlanCache& cache = ctx->plans[rs.preview];
  PlanInput in = plan_input(ctx, req, rs, tu, call.size_spp);
  const bool reuse = cache.find(in) != nullptr;
  if (!reuse) in.avail = available_bytes(ctx);
  const double t_meminfo = host_ms();
  if (!reuse) cache.store(in, plan_workspace(in));
  const WorkspacePlan& plan = cache.plan;
  const double t_sized = host_ms();
  const auto t_alloc0 = std::chrono::steady_clock::now();
  if ((rc = allocate(ctx, req, rs, plan, tr, call))) return rc;
  const double alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_alloc0).count();
  if (call.prepare_only) return touch_workspace(ctx, plan, call, alloc_ms);
  hipStream_t st = ctx->stream;
  if (pass_log) HIP_TRY(hipEventRecord(ctx->evb[0], st));
  const size_t nbg = rs.preview ? 0 : req->num_bg_spd;  // (the preview samplers read no background SPD)
  if ((rc = begin_frame(ctx, req, rs, plan, call, nbg))) return rc;
  ShadeParams sp = shade_params(ctx, req, rs, plan);
  AccumParams ap = accum_params(ctx, req, rs, out_dev);
  // An adaptive session's step over its active list: the list's entries are the step's tiles,
  // one pixel each, and its pixels (entry j's samples lie where pixel j's would: the workspace
  // planned for all pixels holds them).
  const uint32_t run_pixels = call.list ? call.list_count : num_pixels;
  if (call.list) {
    sp.tile_w = sp.tile_h = 1; sp.tiles = call.list;
    ap.map.num_pixels = run_pixels;
  }
  if (!rs.preview) {
    path_shade_params(ctx, req, sc, rs, plan, nbg, sp);
    stage_tables(ctx, req, tu, rs, plan, nbg, sc, sp);
  }

  const RunInput run{run_pixels, plan.chunk, plan.pool_blocks, sr, call.list, call.counts, call.samples_before};
  RunTimes times;
  float total_ms = 0;
  const double t_launch = host_ms();
  HIP_TRY(hipEventRecord(ctx->ev0, st));
  if (pass_log) {  // diagnostics: the GPU time of the setup copies before ev0
    HIP_TRY(hipEventSynchronize(ctx->ev0));
    float prep = 0;
    HIP_TRY(hipEventElapsedTime(&prep, ctx->evb[0], ctx->ev0));
    fprintf(stderr, "IZPI_T ev0_synced %.3f prep_gpu_ms %.3f body_start %.3f\n", diag_clock_ms(), prep,
            diag_clock_ms() - host_ms());
  }
  if (rs.preview) {
    const PreviewParams pp = preview_params(ctx, req, plan);
    rc = run_preview(ctx, req, sc, tr, sp, pp, ap, run, &times);
  } else {
    WaveParams wp = wave_params(ctx, plan, sp);
    // the instance izpi_gpu_upload_scene resolved and prepared (check_request: the scene has the sampler's textures)
    const ShadeKernels* k = ctx->kernels[req->sampler == IZPI_SAMPLER_SPECTRAL][rs.fwd];
    if (!k || (!rs.fwd && k->rec_doubles != plan.D)) {  // (the planner derives the record stride on its own)
      ctx->err = "the shading instance and the workspace plan disagree on the record stride";
      return IZPI_ERR_INVALID;
    }
    rc = run_wavefront(ctx, req, sc, tr, *k, sp, wp, ap, run, &times);
  }
  if (rc) return rc;
  // End frame: the per-wave counter rows summed, the request's post-processing, then the
  // counters and the error word back to the host.
  hipLaunchKernelGGL(k_cpart_reduce, dim3(CNT_N), dim3(256), 0, st, ctx->d_cpart, cpart_rows(ctx), ctx->d_counters);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ev1, st));
  if (!sr.keep && (rc = apply_post(ctx, req, out_dev))) return rc;
  const double t_issued = host_ms();
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  if (pass_log)  // diagnostics: where the call's host time goes
    fprintf(stderr, "IZPI_HOST tiles %.3f tracer %.3f meminfo %.3f sized %.3f allocated %.3f launched %.3f issued %.3f done %.3f ms\n",
            t_tiles, t_tracer, t_meminfo, t_sized, t_sized + alloc_ms, t_launch, t_issued, host_ms());
  HIP_TRY(hipEventElapsedTime(&total_ms, ctx->ev0, ctx->ev1));
  unsigned long long cnt[CNT_N];
  uint32_t guard = 0;
  HIP_TRY(hipMemcpy(cnt, ctx->d_counters, sizeof(cnt), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&guard, misc(ctx, 1), sizeof(guard), hipMemcpyDeviceToHost));
  // (the preview samplers run no light tests, no k_tail and park nothing: those counters stay zero)
  izpi_render_stats& s = ctx->last;
  memset(&s, 0, sizeof(s));
  s.rays = cnt[CNT_RAYS]; s.node_visits = cnt[CNT_NODES]; s.tri_tests = cnt[CNT_TRI]; s.sph_tests = cnt[CNT_SPH];
  s.light_tri_tests = cnt[CNT_LTRI]; s.light_sph_tests = cnt[CNT_LSPH];
  s.samples = call.list ? call.samples_before + (uint64_t)run_pixels * (sr.end - sr.begin) : (uint64_t)num_pixels * sr.end;
  s.kernel_ms = times.trace_ms; s.shade_ms = times.shade_ms; s.total_ms = total_ms; s.launches = times.launches; s.tail_ms = times.tail_ms;
  s.node_steps = cnt[CNT_NSTEP]; s.prim_steps = cnt[CNT_PSTEP]; s.leaf_shortcuts = cnt[CNT_SHORT];
  s.tail_node_visits = cnt[CNT_TAIL_NODES]; s.tail_tri_tests = cnt[CNT_TAIL_TRI]; s.tail_sph_tests = cnt[CNT_TAIL_SPH];
  s.parks = cnt[CNT_PARK];
  s.workspace_bytes = workspace_bytes(ctx);
  s.scene_bytes = ctx->scene_bytes;
  s.slots = plan.slots; s.rec_dense = rs.fwd ? 0 : plan.rec_dense; s.pool_blocks = plan.pool_blocks; s.chunk_spp = plan.chunk;
  s.alloc_ms = alloc_ms;
  // (not within a session: a larger pool would re-allocate the workspace, the sums with it)
  if (!sr.keep && plan.rec_pool && s.parks * 64 > s.rays && plan.pool_blocks < plan.slots) ctx->pool_grow++;
#ifdef IZPI_SHADE_CLOCKS
  fprintf(stderr, "IZPI_SHADE_CLOCKS item %llu refill %llu push %llu mat %llu finish %llu mix %llu lpdf %llu entry %llu tex %llu "
          "res_barrier1 %llu res_atomics %llu res_barrier2 %llu (wave cycles; res_atomics: thread 0 only)\n",
          cnt[CNT_SCLK_ITEM], cnt[CNT_SCLK_REFILL], cnt[CNT_SCLK_PUSH], cnt[CNT_SCLK_MAT], cnt[CNT_SCLK_FIN],
          cnt[CNT_SCLK_MIX], cnt[CNT_SCLK_LPDF], cnt[CNT_SCLK_ENTRY], cnt[CNT_SCLK_TEX], cnt[CNT_SCLK_RB1],
          cnt[CNT_SCLK_RATOM], cnt[CNT_SCLK_RB2]);
#endif
#ifdef IZPI_SHADOW
  fprintf(stderr, "IZPI_SHADOW spill_stores %llu spill_loads %llu (entries)\n", cnt[CNT_CLK_REFILL], cnt[CNT_CLK_NODE]);
#endif
#ifdef IZPI_TRACE_ICOUNT
  fprintf(stderr, "IZPI_TRACE_ICOUNT {\"iterations\": %llu, \"due\": %llu, \"dequeue\": %llu, \"refill\": %llu, \"prim\": %llu, \"node_fast\": %llu, "
          "\"node_twin\": %llu, \"spill\": %llu, \"readback\": %llu, \"spilled\": %llu, \"pop\": %llu, \"finish\": %llu, \"waves\": %llu}\n",
          cnt[CNT_IC_ITER], cnt[CNT_IC_DUE], cnt[CNT_IC_DEQUEUE], cnt[CNT_IC_REFILL], cnt[CNT_PSTEP], cnt[CNT_NSTEP] - cnt[CNT_IC_TWIN], cnt[CNT_IC_TWIN],
          cnt[CNT_IC_SPILL], cnt[CNT_IC_READBACK], cnt[CNT_IC_SPILLED], cnt[CNT_IC_POP], cnt[CNT_IC_FINISH], cnt[CNT_IC_WAVES]);
#endif
#ifdef IZPI_TRACE_CLOCKS
  fprintf(stderr, "IZPI_TRACE_CLOCKS refill %llu node %llu prim %llu advance %llu (wave cycles)\n", cnt[CNT_CLK_REFILL],
          cnt[CNT_CLK_NODE], cnt[CNT_CLK_PRIM], cnt[CNT_CLK_ADV]);
#endif
  return guard_status(ctx, guard);
}

// One render on one context. The progress counters (izpi_gpu_progress) start at 0/0 before
// any check and read done == total on every return, failed calls included.
int render_impl(izpi_ctx* ctx, const izpi_render_req* req, const RenderCall& call, double* out_dev) {
  if (session_open(ctx)) return IZPI_ERR_INVALID;  // (before the progress counters: they are the session's)
  ctx->prog_done.store(0, std::memory_order_relaxed);
  ctx->prog_total.store(0, std::memory_order_relaxed);
  const int rc = render_body(ctx, req, call, out_dev);
  ctx->prog_done.store(ctx->prog_total.load(std::memory_order_relaxed), std::memory_order_relaxed);
  return rc;
}

static_assert(sizeof(Double4) == sizeof(double4), "PackedScene::mat_const uploads as DevScene::mat_const");

// izpi_gpu_upload_scene's first steps: the context is idle on its device and holds no scene.
int begin_upload(izpi_ctx* ctx, const izpi_scene_desc* d) {
  if (!ctx || !d) return IZPI_ERR_INVALID;
  // the scene descriptor is laid out alike in ABI 1 and 2
  if (d->abi_version < 1 || d->abi_version > IZPI_ABI_VERSION) { ctx->err = "ABI version mismatch"; return IZPI_ERR_INVALID; }
  if (session_open(ctx)) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  free_scene(ctx);
  return IZPI_OK;
}

// ... and its last: ps = pack_scene(d) becomes ctx's scene (after begin_upload). The
// materials, the SPD tables and the camera go to the device as the descriptor has them.
int upload_packed(izpi_ctx* ctx, const izpi_scene_desc* d, const PackedScene& ps) {
  DevScene& sc = ctx->sc;
  memset(&sc, 0, sizeof(sc));
  GInner* di; GInnerQ* dq; GLeaf* dl; GPrim* dp; GShade* dsh; GTriVerts* dtv; GTriTex* dtt; GLight* dlt;
  izpi_material* dm; Double4* dmc; MatTex* dmt; izpi_texture* dtx;
  double *dtex, *dswl, *dsv;
  {  // the node block: inner, innerq and leaves in one allocation (trace_layout), so that k_trace2
     // reaches a node step's records from one base. scene_allocs holds the block's base alone
     // (= di: `inner` is never empty); dq and dl point into the block and are never freed on
     // their own. (UP with no host array only allocates: the three parts are copied below.)
    const TraceLayout tl = trace_layout(ps.inner.size(), ps.innerq.size(), ps.leaves.size());
    char* nb;
    UP((const char*)nullptr, tl.alloc_bytes, &nb);
    di = reinterpret_cast<GInner*>(nb);
    dq = ps.innerq.empty() ? nullptr : reinterpret_cast<GInnerQ*>(nb + tl.innerq_at);
    dl = reinterpret_cast<GLeaf*>(nb + tl.leaves_at);
    HIP_TRY(hipMemcpy(di, ps.inner.data(), ps.inner.size() * sizeof(GInner), hipMemcpyHostToDevice));
    if (dq) HIP_TRY(hipMemcpy(dq, ps.innerq.data(), ps.innerq.size() * sizeof(GInnerQ), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dl, ps.leaves.data(), ps.leaves.size() * sizeof(GLeaf), hipMemcpyHostToDevice));
  }
  UP(ps.prims.data(), ps.prims.size(), &dp);
  UP(ps.shade.data(), ps.shade.size(), &dsh);
  UP(ps.triverts.data(), ps.triverts.size(), &dtv);
  UP(ps.tritex.data(), ps.tritex.size(), &dtt);
  UP(ps.lights.data(), ps.lights.size(), &dlt);
  UP(d->materials, d->num_materials, &dm);
  UP(ps.mat_const.data(), ps.mat_const.size(), &dmc);
  UP(ps.mat_tex.data(), ps.mat_tex.size(), &dmt);
  UP(ps.textures.data(), ps.textures.size(), &dtx);
  UP(ps.texels.data(), ps.texels.size(), &dtex);
  UP(d->spd_wavelengths, d->num_spd, &dswl);
  UP(d->spd_values, d->num_spd, &dsv);
#ifdef IZPI_SHADOW
  {
    GInner* si; GLeaf* sl; GPrim* sp;
    UP(ps.inner.data(), ps.inner.size(), &si);
    UP(ps.leaves.data(), ps.leaves.size(), &sl);
    UP(ps.prims.data(), ps.prims.size(), &sp);
    sc.sh_inner = si; sc.sh_leaves = sl; sc.sh_prims = sp;
  }
#endif
  sc.inner = di; sc.innerq = dq; sc.leaves = dl; sc.prims = dp; sc.shade = dsh; sc.tritex = dtt; sc.lights = dlt;
  sc.materials = dm; sc.mat_const = (const double4*)dmc; sc.mat_tex = dmt; sc.textures = dtx; sc.texels = dtex;
  sc.spd_wl = dswl; sc.spd_val = dsv;
  sc.root = ps.root; sc.num_inner = ps.num_inner; sc.num_prims = d->num_prims; sc.num_lights = d->num_lights;
  sc.quantized = ps.quantized; sc.leaf_shortcut = ps.leaf_shortcut; sc.nan_free_bounds = ps.nan_free_bounds;
  sc.ordered_bounds = ps.ordered_bounds;
  sc.tri_only = ps.tri_only; sc.time_free = ps.time_free; sc.no_pathlen = ps.no_pathlen; sc.leaf_max = ps.leaf_max;
  sc.addr32 = trace_addr32(ps.inner.size(), ps.innerq.size(), ps.leaves.size(), ps.prims.size());
  sc.cam = d->camera;
  ctx->d_triverts = dtv;
  ctx->mat_ok_rgb = ps.mat_ok_rgb; ctx->mat_ok_spectral = ps.mat_ok_spectral;
  ctx->basic_materials = ps.basic_materials; ctx->matset = ps.matset;
  ctx->const_albedo = ps.const_albedo; ctx->any_uv = ps.any_uv;
  ctx->pool_grow = 0;
  ctx->stack_needed = ps.stack_needed;
  ctx->num_prims = d->num_prims;
  ctx->num_textures = d->num_textures;
  ctx->num_materials = d->num_materials;
  ctx->num_spd = d->num_spd;
  ctx->have_scene = true;
  ctx->plans[0].valid = ctx->plans[1].valid = false;  // per-slot sizes depend on the scene
  // Load the code of the kernels this scene's renders run now, as part of the scene setup
  // (izpi's Render timer starts after it, renderer.go:170): a first occupancy query loads a
  // kernel's code object, 14 ms of a fresh renderer's first frame otherwise.
  Tracer tr;
  int rc = make_tracer(ctx, kDefaultTuning, !ctx->sc.tri_only || ctx->any_uv, &tr);
  const bool const_basic = ctx->basic_materials && ctx->const_albedo;
  for (int s = 0; s < 2; s++)    // Colour, Spectral
    for (int f = 1; f >= 0; f--) {  // forward, recursive
      const uint32_t sampler = s ? IZPI_SAMPLER_SPECTRAL : IZPI_SAMPLER_COLOUR;
      const ShadeKernels*& k = ctx->kernels[s][f];
      k = (s ? ctx->mat_ok_spectral : ctx->mat_ok_rgb) ? shade_instance(ctx->matset, const_basic, sampler, f != 0) : nullptr;
      if (!rc && k) rc = prepare_wavefront(ctx, *k);
    }
  if (!rc) rc = prepare_preview(ctx);
  return rc;
}
}  // namespace izpi_internal

extern "C" {

int izpi_gpu_open(int device, izpi_ctx** out) {
  if (!out) return IZPI_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0 || device < 0 || device >= n) return IZPI_ERR_HIP;
  if (hipSetDevice(device) != hipSuccess) return IZPI_ERR_HIP;
  izpi_ctx* ctx = new izpi_ctx();
  ctx->device = device;
  hipDeviceProp_t prop;
  bool ok = hipGetDeviceProperties(&prop, device) == hipSuccess;
  ctx->num_cus = ok ? prop.multiProcessorCount : 0;
  ok = ok && hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess &&
       hipEventCreate(&ctx->ev0) == hipSuccess && hipEventCreate(&ctx->ev1) == hipSuccess &&
       hipEventCreate(&ctx->ev2) == hipSuccess && hipEventCreate(&ctx->ev3) == hipSuccess &&
       hipHostMalloc((void**)&ctx->h_count, 9 * MISC_STRIDE * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess &&
       hipMalloc((void**)&ctx->d_misc, 8 * MISC_STRIDE * sizeof(uint32_t)) == hipSuccess &&
       hipMalloc((void**)&ctx->d_pool_ctr, POOL_SHARDS * POOL_CTR_STRIDE * sizeof(unsigned long long)) == hipSuccess &&
       hipMalloc((void**)&ctx->d_counters, CNT_N * sizeof(unsigned long long)) == hipSuccess;
  for (int i = 0; ok && i < 3 * IZPI_PASS_BATCH; i++) ok = hipEventCreate(&ctx->evb[i]) == hipSuccess;
  if (!ok) {
    izpi_gpu_close(ctx);
    return IZPI_ERR_HIP;
  }
  *out = ctx;
  return IZPI_OK;
}

int izpi_gpu_close(izpi_ctx* ctx) {
  if (!ctx) return IZPI_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
  free_scene(ctx);
  for (const CtxBuf& b : ctx_buffers(ctx)) if (*b.p) (void)hipFree(*b.p);
  void* fixed[] = {ctx->d_pool_ctr, ctx->d_misc, ctx->d_counters, ctx->d_status};
  for (void* p : fixed) if (p) (void)hipFree(p);
  if (ctx->h_count) (void)hipHostFree(ctx->h_count);
  if (ctx->stall_host) (void)hipHostFree(ctx->stall_host);
  for (int i = 0; i < 3 * IZPI_PASS_BATCH; i++) if (ctx->evb[i]) (void)hipEventDestroy(ctx->evb[i]);
  hipEvent_t evs[] = {ctx->ev0, ctx->ev1, ctx->ev2, ctx->ev3};
  for (hipEvent_t ev : evs) if (ev) (void)hipEventDestroy(ev);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return IZPI_OK;
}

const char* izpi_gpu_last_error(izpi_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int izpi_gpu_upload_scene(izpi_ctx* ctx, const izpi_scene_desc* d) {
  int rc = begin_upload(ctx, d);
  if (rc) return rc;
  PackedScene ps;
  rc = pack_scene(d, &ps, &ctx->err);
  return rc ? rc : upload_packed(ctx, d, ps);
}

uint64_t izpi_gpu_output_bytes(const izpi_render_req* req) {
  if (!req) return 0;
  if (req->out_layout == IZPI_OUT_PACKED && req->num_tiles) {
    uint64_t px = 0;
    for (uint32_t i = 0; i < req->num_tiles; i++) {
      const uint32_t* t = req->tiles + 4 * i;
      px += (uint64_t)(t[2] - t[0] + 1) * (t[3] - t[1] + 1);
    }
    return px * 4 * sizeof(double);
  }
  return (uint64_t)req->width * req->height * 4 * sizeof(double);
}

int izpi_gpu_render_device(izpi_ctx* ctx, const izpi_render_req* req, double* out_dev, izpi_render_stats* stats) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (!out_dev) { ctx->err = "null output"; return IZPI_ERR_INVALID; }
  HIP_TRY(hipSetDevice(ctx->device));
  int rc = render_impl(ctx, req, one_shot(req), out_dev);
  if (stats) *stats = ctx->last;
  return rc;
}

int izpi_gpu_render(izpi_ctx* ctx, const izpi_render_req* req, double* out_host, izpi_render_stats* stats) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (!out_host || !req) { ctx->err = "null argument"; return IZPI_ERR_INVALID; }
  if (session_open(ctx)) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t bytes = izpi_gpu_output_bytes(req);
  int rc = output_from_host(ctx, out_host, bytes);
  if (rc) return rc;
  rc = render_impl(ctx, req, one_shot(req), ctx->d_out);
  if (stats) *stats = ctx->last;
  return rc ? rc : output_to_host(ctx, out_host, bytes);
}

int izpi_gpu_prepare(izpi_ctx* ctx, const izpi_render_req* req) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (!req) { ctx->err = "null argument"; return IZPI_ERR_INVALID; }
  if (session_open(ctx)) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->comm && ctx->comm_size > 1) return prepare_rank_share(ctx, req);
  return render_impl(ctx, req, one_shot(req, true), nullptr);
}

int izpi_gpu_progress(izpi_ctx* ctx, uint64_t* samples_done, uint64_t* samples_total) {
  if (!ctx || !samples_done || !samples_total) return IZPI_ERR_INVALID;
  // total first: a render starting between the two loads shows 0 of its own total at worst
  *samples_total = ctx->prog_total.load(std::memory_order_relaxed);
  *samples_done = std::min(ctx->prog_done.load(std::memory_order_relaxed), *samples_total);
  return IZPI_OK;
}

int izpi_gpu_debug_realloc(izpi_ctx* ctx, uint32_t mask) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (session_open(ctx)) return IZPI_ERR_INVALID;  // (the fresh buffers are not copies: the sums would be lost)
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const auto bufs = ctx_buffers(ctx);
  for (size_t k = 0; k < RENDER_BUFS; k++) {
    if (!(mask >> k & 1u) || !*bufs[k].p || !*bufs[k].cap) continue;
    void* fresh = nullptr;  // allocated while the old buffer is still held: other pages
    HIP_TRY(hipMalloc(&fresh, *bufs[k].cap));
    HIP_TRY(hipFree(*bufs[k].p));
    *bufs[k].p = fresh;
  }
  return IZPI_OK;
}

int izpi_gpu_debug_fault(izpi_ctx* ctx, int where) {
  if (!ctx || where < 0 || where > 4) return IZPI_ERR_INVALID;
  ctx->fault_inject = where;
  return IZPI_OK;
}

}  // extern "C"

