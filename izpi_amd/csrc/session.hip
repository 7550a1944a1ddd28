// session.hip — progressive sessions on one context (izpi_gpu_progressive_*): the samples of a
// request in resumable steps, snapshots of the running sums, the noise estimate and its stop
// rule, adaptive sampling by that estimate (noise.h). A device group's session (multi.hip) is
// one of these per device.
#include "izpi_runtime.h"
#include "noise.h"

namespace izpi_internal {
// The library's own copy of a session's request and of the arrays it points to.
int session_copy_request(izpi_ctx::Session& ss, const izpi_render_req* req, std::string& err) {
  ss = izpi_ctx::Session{};
  ss.req = request_copy(req);
  ss.tuning = tuning_of(req);
  ss.req.tuning = req->tuning ? &ss.tuning : nullptr;
  if (ss.req.num_tiles) {
    if (!ss.req.tiles) { err = "num_tiles without tiles"; return IZPI_ERR_INVALID; }
    ss.tiles.assign(ss.req.tiles, ss.req.tiles + 4 * (size_t)ss.req.num_tiles);
    ss.req.tiles = ss.tiles.data();
  }
  if (ss.req.num_bg_spd) {
    if (!ss.req.bg_spd_wavelengths || !ss.req.bg_spd_values) { err = "num_bg_spd without the SPD arrays"; return IZPI_ERR_INVALID; }
    ss.bg_wl.assign(ss.req.bg_spd_wavelengths, ss.req.bg_spd_wavelengths + ss.req.num_bg_spd);
    ss.bg_val.assign(ss.req.bg_spd_values, ss.req.bg_spd_values + ss.req.num_bg_spd);
    ss.req.bg_spd_wavelengths = ss.bg_wl.data();
    ss.req.bg_spd_values = ss.bg_val.data();
  }
  return IZPI_OK;
}

void session_drop(izpi_ctx* ctx) {
  ctx->session = izpi_ctx::Session{};
  ctx->prog_done.store(0, std::memory_order_relaxed);
  ctx->prog_total.store(0, std::memory_order_relaxed);
}

static int session_zero_moments(izpi_ctx* ctx) {
  izpi_ctx::Session& ss = ctx->session;
  const size_t bytes = (size_t)ss.num_pixels * 3 * sizeof(double);
  const int rc = grow(ctx, (void**)&ctx->d_moments, &ctx->moments_cap, bytes);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(ctx->d_moments, 0, bytes, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ss.noise = true;
  return IZPI_OK;
}

// The arrays of d_adapt (AdaptBufs) for the session's pixels.
static AdaptParams adapt_arrays(izpi_ctx* ctx) {
  const izpi_ctx::Session& ss = ctx->session;
  const AdaptBufs ab(ss.num_pixels);
  AdaptParams a{};
  a.blocks = (ss.num_pixels + 255) / 256;
  a.table = (uint32_t*)(ctx->d_adapt + ab.table); a.counts = (uint32_t*)(ctx->d_adapt + ab.counts);
  a.block_keep = (uint32_t*)(ctx->d_adapt + ab.block_keep); a.block_stat = (uint32_t*)(ctx->d_adapt + ab.block_stat);
  a.totals = (uint32_t*)(ctx->d_adapt + ab.totals); a.state = (uint8_t*)(ctx->d_adapt + ab.state);
  return a;
}
// The session's sums as its per-pixel kernels read them (SessionView, pixel_map.h), over the
// tiles session_tiles puts in d_tiles. The per-pixel counts are an adaptive session's once a
// pixel has retired; until then every pixel has `done` samples, and the plain forms run.
static SessionView session_view(izpi_ctx* ctx) {
  const izpi_ctx::Session& ss = ctx->session;
  SessionView v{};
  v.map = PixelMap{ss.num_pixels, ss.req.width, ss.req.height, ss.tile_w, ss.tile_h, ss.req.out_layout, ctx->d_tiles};
  v.done = ss.done; v.sampler = ss.req.sampler;
  v.running = ctx->d_running; v.moments = ctx->d_moments;
  v.counts = ss.listed ? adapt_arrays(ctx).counts : nullptr;
  return v;
}
// IZPI_PROG_ADAPTIVE: every pixel active with no sample, in a buffer of its own.
static int session_zero_adapt(izpi_ctx* ctx) {
  izpi_ctx::Session& ss = ctx->session;
  const AdaptBufs ab(ss.num_pixels);
  const int rc = grow(ctx, (void**)&ctx->d_adapt, &ctx->adapt_cap, ab.bytes);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(ctx->d_adapt, 0, ab.bytes, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ss.adaptive = true; ss.listed = false; ss.active = ss.num_pixels; ss.samples = 0;
  return IZPI_OK;
}

// begin: render_body's own checks, plan and allocation for a request of step_spp samples
// (its prepare_only form, which for a session also zeroes the sums and the counters).
// With IZPI_PROG_NOISE the samples' second moments start at zero in a buffer of their own
// (24 B per pixel; it only grows, and no workspace plan counts it).
int session_begin(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp, uint32_t flags) {
  if (ctx->session.open) { ctx->err = "a progressive session is already open"; return IZPI_ERR_INVALID; }
  if (!req || step_spp == 0) { ctx->err = "progressive_begin: a request and step_spp >= 1"; return IZPI_ERR_INVALID; }
  if (flags & ~(uint32_t)(IZPI_PROG_NOISE | IZPI_PROG_ADAPTIVE)) { ctx->err = "progressive_begin: unknown flags"; return IZPI_ERR_INVALID; }
  if ((flags & IZPI_PROG_ADAPTIVE) && !(flags & IZPI_PROG_NOISE)) { ctx->err = "progressive_begin: IZPI_PROG_ADAPTIVE needs IZPI_PROG_NOISE"; return IZPI_ERR_INVALID; }
  if ((flags & IZPI_PROG_ADAPTIVE) && preview_sampler(req->sampler)) { ctx->err = "progressive_begin: IZPI_PROG_ADAPTIVE with a preview sampler"; return IZPI_ERR_INVALID; }
  izpi_ctx::Session& ss = ctx->session;
  int rc = session_copy_request(ss, req, ctx->err);
  if (!rc) {
    ss.step_spp = std::min(step_spp, std::max(1u, ss.req.spp));
    rc = render_body(ctx, &ss.req, RenderCall{SampleRange{0, 0, true}, ss.step_spp, true}, nullptr);
  }
  if (!rc && (flags & IZPI_PROG_NOISE)) rc = session_zero_moments(ctx);
  if (!rc && (flags & IZPI_PROG_ADAPTIVE)) rc = session_zero_adapt(ctx);
  if (rc) {
    const std::string why = ctx->err;
    session_drop(ctx);
    ctx->err = why;
    return rc;
  }
  ss.cum = izpi_render_stats{};
  ss.open = true;
  ctx->prog_done.store(0, std::memory_order_relaxed);
  ctx->prog_total.store((uint64_t)ss.num_pixels * ss.req.spp, std::memory_order_relaxed);
  return IZPI_OK;
}

static int session_usable(izpi_ctx* ctx) {
  if (!ctx->session.open) { ctx->err = "no progressive session is open"; return IZPI_ERR_INVALID; }
  if (ctx->session.broken) { ctx->err = "the session's last step failed: end it"; return IZPI_ERR_INVALID; }
  return IZPI_OK;
}

// step: samples [done, done + n) through render_body's chunk loops, never finalised. The
// device counters run on from step to step; times and launches are summed here. An adaptive
// session after its first retirement: the same over its active list (render_body), and with no
// active pixel nothing.
int session_step(izpi_ctx* ctx, uint32_t spp, izpi_render_stats* stats) {
  int rc = session_usable(ctx);
  if (rc) return rc;
  izpi_ctx::Session& ss = ctx->session;
  uint32_t n = std::min(spp ? spp : ss.step_spp, ss.req.spp - ss.done);
  if (ss.listed && ss.active == 0) n = 0;
  if (n) {
    RenderCall call{SampleRange{ss.done, ss.done + n, true}, ss.step_spp, false};
    if (ss.listed) {
      const AdaptParams a = adapt_arrays(ctx);
      call.list = a.table; call.counts = a.counts; call.list_count = ss.active; call.samples_before = ss.samples;
    }
    rc = render_body(ctx, &ss.req, call, nullptr);
    if (rc) {  // a chunk may or may not be in the sums
      ss.broken = true;
      return rc;
    }
    ss.done += n;
    ss.samples += (uint64_t)n * (ss.adaptive ? ss.active : ss.num_pixels);
    izpi_render_stats s = ctx->last;
    s.kernel_ms += ss.cum.kernel_ms; s.shade_ms += ss.cum.shade_ms; s.tail_ms += ss.cum.tail_ms;
    s.total_ms += ss.cum.total_ms; s.alloc_ms += ss.cum.alloc_ms; s.launches += ss.cum.launches;
    ss.cum = s;
    ctx->last = s;
    ctx->prog_done.store(ss.samples, std::memory_order_relaxed);
  }
  if (stats) *stats = ss.cum;
  return IZPI_OK;
}

// The session's tiles on the device (izpi_gpu_unpack_tiles may have used d_tiles since the last step).
static int session_tiles(izpi_ctx* ctx) {
  const izpi_ctx::Session& ss = ctx->session;
  const int rc = grow(ctx, (void**)&ctx->d_tiles, &ctx->tiles_cap, ss.run_tiles.size() * sizeof(uint32_t));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->d_tiles, ss.run_tiles.data(), ss.run_tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  return IZPI_OK;
}

// The noise estimate needs a session begun with IZPI_PROG_NOISE and two samples (n - 1 divides;
// need = 0: a converge, which steps before it estimates). True, with the message, when it lacks one.
bool session_lacks_noise(const izpi_ctx::Session& ss, std::string& err, uint32_t need) {
  if (!ss.noise) { err = "noise: the session was begun without IZPI_PROG_NOISE"; return true; }
  if (ss.done < need) { err = "noise: needs at least 2 samples"; return true; }
  return false;
}
// The caller's parameters, or the defaults for a null pointer, checked (nz::check_params).
bool noise_params_ok(const izpi_noise_params* params, izpi_noise_params& p, std::string& err) {
  p = params ? *params : nz::defaults();
  const char* bad = nz::check_params(p);
  if (bad) err = bad;
  return !bad;
}
// A snapshot's form is known, and the session has a sample to show.
bool snapshot_form_ok(uint32_t form, uint32_t done, std::string& err) {
  if (form != IZPI_SNAP_CANVAS && form != IZPI_SNAP_DISPLAY && form != IZPI_SNAP_NOISE && form != IZPI_SNAP_SAMPLES) { err = "unknown snapshot form"; return false; }
  if (done == 0) { err = "snapshot before the session's first sample"; return false; }
  return true;
}
// adapt, and the IZPI_SNAP_SAMPLES snapshot, need a session begun with IZPI_PROG_ADAPTIVE.
bool session_lacks_adaptive(const izpi_ctx::Session& ss, std::string& err) {
  if (!ss.adaptive) err = "adapt: the session was begun without IZPI_PROG_ADAPTIVE";
  return !ss.adaptive;
}

// noise: k_noise_stats over the sums and moments; the block sums are added here, in block order.
int session_noise(izpi_ctx* ctx, const izpi_noise_params* params, izpi_noise_stats* out) {
  int rc = session_usable(ctx);
  if (rc) return rc;
  izpi_noise_params p;
  const izpi_ctx::Session& ss = ctx->session;
  if (!noise_params_ok(params, p, ctx->err) || session_lacks_noise(ss, ctx->err)) return IZPI_ERR_INVALID;
  hipStream_t st = ctx->stream;
  if ((rc = session_tiles(ctx))) return rc;
  const size_t blocks = ((size_t)ss.num_pixels + nz::BLOCK - 1) / nz::BLOCK;
  if ((rc = grow(ctx, (void**)&ctx->d_noisepart, &ctx->noisepart_cap, 5 * blocks * sizeof(double)))) return rc;
  NoiseParams np{};
  np.view = session_view(ctx);
  np.threshold = p.threshold; np.floor = p.floor;
  np.block_sums = ctx->d_noisepart;
  np.block_counts = (unsigned long long*)(ctx->d_noisepart + blocks);
  HIP_TRY(hipEventRecord(ctx->ev0, st));
  launch_noise_stats(st, np);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ev1, st));
  std::vector<double> part(5 * blocks);
  HIP_TRY(hipMemcpyAsync(part.data(), ctx->d_noisepart, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  izpi_noise_stats s{};
  unsigned long long max_bits = 0;
  for (size_t b = 0; b < blocks; b++) {  // (every block writes its partials: nothing to zero)
    unsigned long long cnt[4];
    memcpy(cnt, part.data() + blocks + 4 * b, sizeof(cnt));
    s.pixels += cnt[0]; s.nonfinite += cnt[1]; s.above += cnt[2];
    max_bits = std::max(max_bits, cnt[3]);
    s.sum_error = s.sum_error + part[b];
  }
  s.max_error = gm::from_bits(max_bits);
  s.device_ms = ms;
  s.done = ss.done;
  s.converged = nz::converged(s.pixels, s.nonfinite, s.above, s.done, p);
  if (out) *out = s;
  return IZPI_OK;
}

// adapt: adapt.hip's three launches over the session's pixels; the frame's integers come back
// in one small copy. From the first retirement on the steps run over the list it leaves.
int session_adapt(izpi_ctx* ctx, const izpi_noise_params* params, izpi_adapt_stats* out) {
  int rc = session_usable(ctx);
  if (rc) return rc;
  izpi_noise_params p;
  izpi_ctx::Session& ss = ctx->session;
  if (!noise_params_ok(params, p, ctx->err) || session_lacks_adaptive(ss, ctx->err)) return IZPI_ERR_INVALID;
  if (ss.done < 2) { ctx->err = "adapt: needs at least 2 samples"; return IZPI_ERR_INVALID; }
  hipStream_t st = ctx->stream;
  if ((rc = session_tiles(ctx))) return rc;
  AdaptParams a = adapt_arrays(ctx);
  a.view = session_view(ctx);
  a.threshold = p.threshold; a.floor = p.floor;
  HIP_TRY(hipEventRecord(ctx->ev0, st));
  launch_adapt(st, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ev1, st));
  uint32_t totals[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  if (totals[0] > ss.active) { ctx->err = "adapt: the active list grew"; ss.broken = true; return IZPI_ERR_DEVICE; }
  izpi_adapt_stats s{};
  s.pixels = totals[1]; s.nonfinite = totals[2]; s.active = totals[0]; s.retired = ss.active - totals[0];
  ss.active = totals[0];
  if (ss.active < ss.num_pixels) ss.listed = true;
  s.samples = ss.samples; s.device_ms = ms; s.done = ss.done;
  s.converged = nz::converged(s.pixels, s.nonfinite, s.active, s.done, p);
  if (out) *out = s;
  return IZPI_OK;
}

// snapshot: k_resolve of the sums into device memory, then (IZPI_SNAP_CANVAS) the request's post.
int session_snapshot(izpi_ctx* ctx, uint32_t form, double* out_dev) {
  int rc = session_usable(ctx);
  if (rc) return rc;
  const izpi_ctx::Session& ss = ctx->session;
  if (!snapshot_form_ok(form, ss.done, ctx->err)) return IZPI_ERR_INVALID;
  if (form == IZPI_SNAP_NOISE && session_lacks_noise(ss, ctx->err)) return IZPI_ERR_INVALID;
  if (form == IZPI_SNAP_SAMPLES && session_lacks_adaptive(ss, ctx->err)) return IZPI_ERR_INVALID;
  if (!out_dev) { ctx->err = "null output"; return IZPI_ERR_INVALID; }
  hipStream_t st = ctx->stream;
  if ((rc = session_tiles(ctx))) return rc;
  if (form == IZPI_SNAP_NOISE) {  // k_noise_resolve: the standard errors, where k_resolve writes the pixels; no post
    NoiseParams np{};
    np.view = session_view(ctx);
    np.floor = IZPI_NOISE_DEFAULT_FLOOR;  // (of e, which the snapshot does not show)
    np.out = out_dev;
    launch_noise_resolve(st, np);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return IZPI_OK;
  }
  ResolveParams rp{};
  rp.view = session_view(ctx);
  rp.form = form; rp.exposure = ss.req.exposure; rp.out = out_dev;
  launch_resolve(st, rp);
  HIP_TRY(hipGetLastError());
  if (form == IZPI_SNAP_CANVAS && (rc = apply_post(ctx, &ss.req, out_dev))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return IZPI_OK;
}

// ---- checkpoint and resume
static uint32_t session_flags(const izpi_ctx::Session& ss) {
  return (ss.noise ? (uint32_t)IZPI_PROG_NOISE : 0u) | (ss.adaptive ? (uint32_t)IZPI_PROG_ADAPTIVE : 0u);
}

// The staging buffer for the session's frame (grown on the first checkpoint or resume of its
// size, never by a session that does neither), the session's tiles on the device, and the
// kernels' view of both.
static int ckpt_params(izpi_ctx* ctx, const ck::Layout& l, CkptParams* cp) {
  const izpi_ctx::Session& ss = ctx->session;
  const CkptBufs cb(l, ss.num_pixels);
  int rc = grow(ctx, (void**)&ctx->d_ckpt, &ctx->ckpt_cap, cb.bytes);
  if (!rc) rc = session_tiles(ctx);
  if (rc) return rc;
  cp->map = session_view(ctx).map;
  cp->planes = ck::planes_at(ctx->d_ckpt + cb.planes, sizeof(ck::Header), l, (uint8_t*)(ctx->d_ckpt + cb.claimed));
  cp->block_counts = (uint32_t*)(ctx->d_ckpt + cb.block_counts);
  return IZPI_OK;
}

// The sum of the first `blocks` words of cp.block_counts, on the host (integers: no order matters).
static int ckpt_block_total(izpi_ctx* ctx, const CkptParams& cp, size_t blocks, uint64_t* total) {
  std::vector<uint32_t> part(blocks);
  HIP_TRY(hipMemcpyAsync(part.data(), cp.block_counts, blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *total = 0;
  for (uint32_t v : part) *total += v;
  return IZPI_OK;
}

int session_checkpoint_bytes(izpi_ctx* ctx, uint64_t* bytes) {
  if (!ctx->session.open) { ctx->err = "no progressive session is open"; return IZPI_ERR_INVALID; }
  if (!bytes) { ctx->err = "null output"; return IZPI_ERR_INVALID; }
  *bytes = ck::Layout(ctx->session.req.width, ctx->session.req.height, session_flags(ctx->session)).bytes;
  return IZPI_OK;
}

// checkpoint: the planes are zeroed with every record absent, k_ckpt_gather writes the session's
// pixels, and one copy moves them behind the header in the caller's memory; the header is
// written last, with the checksum of what lies behind it. Nothing of the session is written.
int session_checkpoint(izpi_ctx* ctx, uint64_t scene_tag, void* out_host, uint64_t cap) {
  int rc = session_usable(ctx);
  if (rc) return rc;
  const izpi_ctx::Session& ss = ctx->session;
  if (!out_host) { ctx->err = "null output"; return IZPI_ERR_INVALID; }
  if (ss.done == 0) { ctx->err = "checkpoint: before the session's first sample (done == 0)"; return IZPI_ERR_INVALID; }
  const uint32_t flags = session_flags(ss);
  const ck::Layout l(ss.req.width, ss.req.height, flags);
  if (cap < l.bytes) {
    ctx->err = "checkpoint: the output holds " + std::to_string(cap) + " bytes, the blob takes " + std::to_string(l.bytes);
    return IZPI_ERR_INVALID;
  }
  CkptParams cp{};
  if ((rc = ckpt_params(ctx, l, &cp))) return rc;
  hipStream_t st = ctx->stream;
  const size_t plane_bytes = l.bytes - sizeof(ck::Header);
  HIP_TRY(hipMemsetAsync(ctx->d_ckpt, 0, plane_bytes, st));
  HIP_TRY(hipMemsetAsync(cp.planes.state, ck::NOT_IN_SESSION, l.n, st));
  const AdaptParams a = ss.listed ? adapt_arrays(ctx) : AdaptParams{};
  cp.packed = ck::Packed{ctx->d_running, ss.noise ? ctx->d_moments : nullptr, a.counts, a.state, ss.done};
  launch_ckpt_gather(st, cp);
  HIP_TRY(hipGetLastError());
  char* out = (char*)out_host;
  unsigned long long cnt[CNT_N];
  HIP_TRY(hipMemcpyAsync(out + sizeof(ck::Header), ctx->d_ckpt, plane_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(cnt, ctx->d_counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ck::Header h = checkpoint_header(ss.req, flags, scene_tag);
  h.listed = ss.listed ? 1u : 0u;
  const uint8_t* state = (const uint8_t*)(out + l.state);
  for (uint64_t i = 0; i < l.n; i++) h.pixels += state[i] != ck::NOT_IN_SESSION;
  h.done = ss.done; h.samples = ss.samples; h.active = ss.adaptive ? ss.active : 0;
  h.cnt_n = CNT_N;
  for (uint32_t k = 0; k < ck::CARRIED_COUNTERS; k++) h.counters[k] = cnt[k];  // (the diagnostics stay 0: checkpoint.h)
  memcpy(out, &h, sizeof h);
  h.checksum = checkpoint_checksum(out, l.bytes);
  memcpy(out, &h, sizeof h);
  return IZPI_OK;
}

// resume: the blob's own validation (checkpoint_check: no device work before it holds), begin
// with the blob's flags, then the planes to the staging buffer and k_ckpt_scatter into the
// session's arrays. The pixel sets are equal when no session pixel lacks a record and the
// distinct records claimed (marked by the scatter, counted by k_ckpt_claimed) are as many as the
// blob holds. An adaptive session's list is rebuilt from the stored state bytes.
int session_resume(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp, uint64_t scene_tag, const void* blob,
                   uint64_t bytes, bool share, bool zero_counters) {
  if (ctx->session.open) { ctx->err = "a progressive session is already open"; return IZPI_ERR_INVALID; }
  char msg[160];
  if (const char* bad = checkpoint_check(blob, bytes, req, scene_tag, msg, sizeof msg)) { ctx->err = bad; return IZPI_ERR_INVALID; }
  ck::Header h;
  memcpy(&h, blob, sizeof h);
  if (h.cnt_n != CNT_N) {
    ctx->err = "checkpoint: it holds " + std::to_string(h.cnt_n) + " device counters, this library " + std::to_string((uint32_t)CNT_N);
    return IZPI_ERR_INVALID;
  }
  int rc = session_begin(ctx, req, step_spp, h.flags);
  if (rc) return rc;
  izpi_ctx::Session& ss = ctx->session;
  auto fail = [&](int status, const std::string& why) {
    session_drop(ctx);
    ctx->err = why;
    return status;
  };
  const ck::Layout l(h.width, h.height, h.flags);
  CkptParams cp{};
  if ((rc = ckpt_params(ctx, l, &cp))) return fail(rc, ctx->err);
  hipStream_t st = ctx->stream;
  const size_t plane_bytes = l.bytes - sizeof(ck::Header);
  const CkptBufs cb(l, ss.num_pixels);
  const AdaptParams arrays = ss.adaptive ? adapt_arrays(ctx) : AdaptParams{};
  cp.packed = ck::Packed{ctx->d_running, ss.noise ? ctx->d_moments : nullptr, arrays.counts, arrays.state, h.done};
  uint64_t absent = 0, claimed = 0;
  auto install = [&]() -> int {
    HIP_TRY(hipMemcpyAsync(ctx->d_ckpt, (const char*)blob + sizeof(ck::Header), plane_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(ctx->d_ckpt + cb.claimed, 0, l.n, st));
    launch_ckpt_scatter(st, cp);
    HIP_TRY(hipGetLastError());
    int r = ckpt_block_total(ctx, cp, ((size_t)ss.num_pixels + 255) / 256, &absent);
    if (r || absent || share) return r;
    launch_ckpt_claimed(st, cp);
    HIP_TRY(hipGetLastError());
    return ckpt_block_total(ctx, cp, (size_t)((l.n + 255) / 256), &claimed);
  };
  if ((rc = install())) return fail(rc, ctx->err);
  if (absent)
    return fail(IZPI_ERR_INVALID, "checkpoint: " + std::to_string(absent) + " pixels of the request have no record in it (the pixel sets differ)");
  if (!share && claimed != h.pixels)
    return fail(IZPI_ERR_INVALID, "checkpoint: " + std::to_string(h.pixels - claimed) + " of its records belong to no pixel of the request (the pixel sets differ)");
  // the integers: Σ n_p over the session's pixels, from the blob's own counts
  uint64_t samples = (uint64_t)h.done * ss.num_pixels;
  uint32_t active = 0;
  if (ss.adaptive) {
    const char* counts = (const char*)blob + l.counts;
    samples = 0;
    for (uint32_t p = 0; p < ss.num_pixels; p++) {
      uint32_t x, y, n;
      tile_pixel(ss.run_tiles.data(), ss.tile_w, ss.tile_h, p, &x, &y);
      memcpy(&n, counts + 4 * ((size_t)y * h.width + x), sizeof n);
      samples += n;
    }
    AdaptParams a = arrays;
    a.view = session_view(ctx);
    auto rebuild = [&]() -> int {
      launch_adapt_restore(st, a);
      HIP_TRY(hipGetLastError());
      uint32_t totals[4] = {0, 0, 0, 0};
      HIP_TRY(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      active = totals[0];
      return IZPI_OK;
    };
    if ((rc = rebuild())) return fail(rc, ctx->err);
    if (!share && active != h.active) return fail(IZPI_ERR_INVALID, "checkpoint: its state bytes and its active count disagree");
  }
  if (!zero_counters) {
    auto counters = [&]() -> int {
      HIP_TRY(hipMemcpyAsync(ctx->d_counters, h.counters, CNT_N * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));
      return IZPI_OK;
    };
    if ((rc = counters())) return fail(rc, ctx->err);
  }
  ss.done = h.done; ss.samples = samples;
  if (ss.adaptive) { ss.active = active; ss.listed = active < ss.num_pixels; }
  ctx->prog_done.store(samples, std::memory_order_relaxed);
  return IZPI_OK;
}

}  // namespace izpi_internal

using namespace izpi_internal;

extern "C" {

int izpi_gpu_progressive_begin_ex(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp, uint32_t flags) {
  if (!ctx) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  return session_begin(ctx, req, step_spp, flags);
}

int izpi_gpu_progressive_begin(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp) {
  return izpi_gpu_progressive_begin_ex(ctx, req, step_spp, 0);
}

int izpi_gpu_progressive_noise(izpi_ctx* ctx, const izpi_noise_params* p, izpi_noise_stats* out) {
  if (!ctx) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  return session_noise(ctx, p, out);
}

int izpi_gpu_progressive_adapt(izpi_ctx* ctx, const izpi_noise_params* p, izpi_adapt_stats* out) {
  if (!ctx) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  return session_adapt(ctx, p, out);
}

int izpi_gpu_progressive_converge(izpi_ctx* ctx, const izpi_noise_params* p, izpi_render_stats* stats, izpi_noise_stats* noise) {
  if (!ctx) return IZPI_ERR_INVALID;
  int rc = session_usable(ctx);
  if (rc) return rc;
  izpi_noise_params q;
  if (!noise_params_ok(p, q, ctx->err) || session_lacks_noise(ctx->session, ctx->err, 0)) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->session.adaptive) {  // adapt decides; the statistic after the last one is the caller's
    izpi_adapt_stats last{};
    bool idle = false;  // no active pixel is left: the statistic of the frame as it stands
    rc = adapt_loop(q, ctx->session.req.spp, [&]() { return session_step(ctx, 0, nullptr); },
                    [&](const izpi_noise_params& np, izpi_adapt_stats* as) { return session_adapt(ctx, &np, as); },
                    [&]() { return ctx->session.done; }, &last, &idle);
    izpi_noise_stats ns{};
    if (!rc && (last.done || idle)) rc = session_noise(ctx, &q, &ns);
    if (noise) *noise = ns;
  } else {
    rc = converge_loop(q, ctx->session.req.spp, [&]() { return session_step(ctx, 0, nullptr); },
                       [&](const izpi_noise_params& np, izpi_noise_stats* ns) { return session_noise(ctx, &np, ns); },
                       [&]() { return ctx->session.done; }, noise);
  }
  if (stats) *stats = ctx->session.cum;
  return rc;
}

int izpi_gpu_progressive_step(izpi_ctx* ctx, uint32_t spp, izpi_render_stats* stats) {
  if (!ctx) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  return session_step(ctx, spp, stats);
}

int izpi_gpu_progressive_snapshot_device(izpi_ctx* ctx, uint32_t form, double* out_dev) {
  if (!ctx) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  return session_snapshot(ctx, form, out_dev);
}

int izpi_gpu_progressive_snapshot(izpi_ctx* ctx, uint32_t form, double* out_host) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (!out_host) { ctx->err = "null output"; return IZPI_ERR_INVALID; }
  int rc = session_usable(ctx);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t bytes = izpi_gpu_output_bytes(&ctx->session.req);
  if ((rc = output_from_host(ctx, out_host, bytes))) return rc;
  if ((rc = session_snapshot(ctx, form, ctx->d_out))) return rc;
  return output_to_host(ctx, out_host, bytes);
}

int izpi_gpu_progressive_checkpoint_bytes(izpi_ctx* ctx, uint64_t* bytes) {
  if (!ctx) return IZPI_ERR_INVALID;
  return session_checkpoint_bytes(ctx, bytes);
}

int izpi_gpu_progressive_checkpoint(izpi_ctx* ctx, uint64_t scene_tag, void* out_host, uint64_t cap) {
  if (!ctx) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  return session_checkpoint(ctx, scene_tag, out_host, cap);
}

int izpi_gpu_progressive_resume(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp, uint64_t scene_tag,
                                const void* blob, uint64_t bytes) {
  if (!ctx) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  if (!req || step_spp == 0) { ctx->err = "progressive_resume: a request and step_spp >= 1"; return IZPI_ERR_INVALID; }
  return session_resume(ctx, req, step_spp, scene_tag, blob, bytes);
}

int izpi_gpu_progressive_end(izpi_ctx* ctx) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (!ctx->session.open) { ctx->err = "no progressive session is open"; return IZPI_ERR_INVALID; }
  session_drop(ctx);
  return IZPI_OK;
}

}  // extern "C"
