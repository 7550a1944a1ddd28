// multi.hip — one frame over several GPUs: the share plan (Shares), the devices of one process
// (izpi_multi: a host thread per device, peer copies to the root) with their progressive
// session, and one process per GPU over RCCL (izpi_gpu_render_rank). Each device renders its
// share through the one-context calls of izpi_gpu.hip and session.hip.
#include "izpi_runtime.h"
#include "noise.h"
#include "scene_pack.h"

#include <functional>

using namespace izpi_internal;

// Packed pixel p of the tiles (IZPI_OUT_PACKED) into its slot of the W x H canvas (PixelMap::slot,
// pixel_map.h; sample row y = 0 has none), as izpi_host_assemble_shares does on the host.
__global__ void k_unpack(const uint32_t* tiles, uint32_t num_pixels, uint32_t tile_w, uint32_t tile_h, uint32_t width,
                         uint32_t height, const double* packed, double* canvas) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= num_pixels) return;
  const PixelMap map{num_pixels, width, height, tile_w, tile_h, IZPI_OUT_CANVAS, tiles};
  if (double* o = map.slot(p, canvas)) {
    const double* s = packed + (size_t)p * 4;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
  }
}

namespace {
// ------------------------------------------------------------------ multi-GPU
// The frame is split into G shares: its tiles (common.Tiles' spiral order) become the units
// of izpi_host_share_units (quarter tiles, where they can be cut) and unit u goes to share
// u % G (izpi_host_share_tiles), so the costly centre tiles spread over all devices. Share
// r is rendered packed (IZPI_OUT_PACKED) into d_share, padded to the largest share's size
// (izpi_host_share_block) so that one gather moves equal blocks; the root scatters share
// r's units from block r into the canvas (k_unpack; on the host izpi_host_assemble_shares).
struct Shares {
  std::vector<uint32_t> all;  // the units the frame is dealt in, [n][4]
  uint32_t n = 1;             // shares
  uint32_t tw = 0, th = 0;    // a unit's extent
  size_t block = 0;           // doubles per (padded) share
  std::vector<uint32_t> mine(uint32_t r) const {
    std::vector<uint32_t> t(all.size());
    t.resize(4 * (size_t)izpi_host_share_tiles(all.data(), (uint32_t)(all.size() / 4), r, n, t.data()));
    return t;
  }
};

size_t share_block(size_t ntiles, uint32_t tw, uint32_t th, uint32_t n) { return ((ntiles + n - 1) / n) * (size_t)tw * th * 4; }

int make_shares(izpi_ctx* ctx, const izpi_render_req* req, uint32_t n, Shares& sh) {
  if (!req || req->width == 0 || req->height == 0) { ctx->err = "invalid render request"; return IZPI_ERR_INVALID; }
  if (req->out_layout != IZPI_OUT_CANVAS) { ctx->err = "multi-GPU renders produce a canvas (IZPI_OUT_CANVAS)"; return IZPI_ERR_INVALID; }
  std::vector<uint32_t> tiles;
  int rc = request_tiles(ctx, req, tiles);
  if (rc) return rc;
  sh.all.resize(4 * tiles.size());
  sh.all.resize(4 * (size_t)izpi_host_share_units(tiles.data(), (uint32_t)(tiles.size() / 4), n, sh.all.data()));
  // (the units cover exactly the tiles' pixels: they are valid where the request's tiles are)
  if (!validate_tiles(req, sh.all.data(), (uint32_t)(sh.all.size() / 4), &sh.tw, &sh.th)) {
    ctx->err = "tiles must be non-empty, in bounds and equal-sized";
    return IZPI_ERR_INVALID;
  }
  sh.n = n;
  sh.block = share_block(sh.all.size() / 4, sh.tw, sh.th, n);
  return IZPI_OK;
}

// The buffers of a share on this context: its block and, on the root, the gather buffer of
// every share's block and (canvas_bytes != 0) the canvas in d_out.
int share_buffers(izpi_ctx* ctx, const Shares& sh, bool root, size_t canvas_bytes = 0) {
  int rc = grow(ctx, (void**)&ctx->d_share, &ctx->share_cap, sh.block * sizeof(double));
  if (!rc && root) rc = grow(ctx, (void**)&ctx->d_gather, &ctx->gather_cap, (size_t)sh.n * sh.block * sizeof(double));
  if (!rc && root && canvas_bytes) rc = grow(ctx, (void**)&ctx->d_out, &ctx->out_cap, canvas_bytes);
  return rc;
}

// The request of one share of `base` (the library's own full copy of a request): the share's
// units `mine`, packed and un-posted (the root posts the assembled frame).
izpi_render_req share_request(const izpi_render_req& base, const std::vector<uint32_t>& mine) {
  izpi_render_req q = base;
  q.num_tiles = (uint32_t)(mine.size() / 4);
  q.tiles = mine.data();
  q.out_layout = IZPI_OUT_PACKED;
  q.post = IZPI_POST_NONE;
  return q;
}

// Render share r of the frame into ctx->d_share (share_buffers; stats in ctx->last), or
// with prepare_only allocate the workspace that render needs.
int render_share(izpi_ctx* ctx, const izpi_render_req* req, const Shares& sh, uint32_t r, bool prepare_only = false) {
  const std::vector<uint32_t> mine = sh.mine(r);
  memset(&ctx->last, 0, sizeof(ctx->last));
  if (mine.empty()) return IZPI_OK;  // more shares than units: an empty block joins the gather
  const izpi_render_req q = share_request(request_copy(req), mine);  // (the caller's may be an older ABI's prefix)
  return render_impl(ctx, &q, one_shot(&q, prepare_only), prepare_only ? nullptr : ctx->d_share);
}

// Root: scatter every share's packed tiles from d_gather into the canvas (row H - y,
// rgb.go:41), then Render's post-processing of the assembled frame.
int assemble(izpi_ctx* ctx, const izpi_render_req* req, const Shares& sh, double* canvas_dev) {
  izpi_ctx* root = ctx;  // (HIP_TRY reports into ctx)
  hipStream_t st = root->stream;
  for (uint32_t r = 0; r < sh.n; r++) {
    const std::vector<uint32_t> t = sh.mine(r);
    if (t.empty()) continue;
    int rc = grow(root, (void**)&root->d_utiles, &root->utiles_cap, sh.all.size() * sizeof(uint32_t));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(root->d_utiles, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    const uint32_t np = (uint32_t)(t.size() / 4) * sh.tw * sh.th;
    hipLaunchKernelGGL(k_unpack, dim3((np + 255) / 256), dim3(256), 0, st, root->d_utiles, np, sh.tw, sh.th, req->width,
                       req->height, root->d_gather + (size_t)r * sh.block, canvas_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // d_utiles is reused by the next share
  }
  int rc = apply_post(root, req, canvas_dev);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return IZPI_OK;
}

}  // namespace

// One context per device of a single-process multi-GPU render (izpi_gpu_multi_*).
struct izpi_multi {
  std::vector<izpi_ctx*> ctx;
  std::string err;
  // the progressive session over the devices (izpi_gpu_multi_progressive_*): the request (and
  // step_spp, done), and the share plan its devices' sessions were opened with
  bool prog_open = false;
  izpi_ctx::Session session;
  Shares shares;
};

namespace {
// The frame's shares over m's devices, with the root's (device 0's) buffers; the root's
// device is left current.
int multi_shares(izpi_multi* m, const izpi_render_req* req, Shares& sh) {
  izpi_ctx* root = m->ctx[0];
  int rc = make_shares(root, req, (uint32_t)m->ctx.size(), sh);
  if (!rc && hipSetDevice(root->device) != hipSuccess) { root->err = "hipSetDevice"; rc = IZPI_ERR_HIP; }
  if (!rc) rc = share_buffers(root, sh, true, (size_t)req->width * req->height * 4 * sizeof(double));
  if (rc) m->err = root->err;
  return rc;
}

// One host thread per device: fn(i, context i) with that device current. The first
// failure in device order is the call's, reported in m->err.
template <class F>
int on_every_device(izpi_multi* m, F fn) {
  const uint32_t G = (uint32_t)m->ctx.size();
  std::vector<int> rcs(G, IZPI_OK);
  std::vector<std::thread> th;
  for (uint32_t i = 0; i < G; i++) {
    th.emplace_back([&, i]() {
      izpi_ctx* c = m->ctx[i];
      if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice"; rcs[i] = IZPI_ERR_HIP; return; }
      rcs[i] = fn(i, c);
    });
  }
  for (std::thread& t : th) t.join();
  for (uint32_t i = 0; i < G; i++)
    if (rcs[i]) { m->err = "device " + std::to_string(i) + ": " + m->ctx[i]->err; return rcs[i]; }
  return IZPI_OK;
}

// The guards of the group's entry points: a group with devices (a null one has no err to write) ...
bool multi_valid(const izpi_multi* m) { return m && !m->ctx.empty(); }
// ... and one with a progressive session open.
bool multi_in_session(izpi_multi* m) {
  if (multi_valid(m) && !m->prog_open) m->err = "no progressive session is open";
  return multi_valid(m) && m->prog_open;
}

bool multi_session_open(izpi_multi* m) {
  if (!m->prog_open) return false;
  m->err = "a progressive session is open";
  return true;
}

// The group's whole-frame round trip (multi_shares has sized the root's buffers). The root's
// canvas starts from the caller's (pixels of no tile keep their values) or zeroed; share(i, c)
// leaves device i's packed block in c->d_share, which goes into block i of the root's gather
// buffer (a peer copy over xGMI; a plain device copy for the root); the root assembles the
// frame with req's width, height and post, and the canvas goes back to the caller.
int multi_frame(izpi_multi* m, const izpi_render_req* req, const Shares& sh, double* out_host,
                const std::function<int(uint32_t, izpi_ctx*)>& share) {
  izpi_ctx* root = m->ctx[0];
  const size_t canvas_bytes = (size_t)req->width * req->height * 4 * sizeof(double);
  if (hipSetDevice(root->device) != hipSuccess) { m->err = "hipSetDevice"; return IZPI_ERR_HIP; }
  if (out_host) {
    if (hipMemcpy(root->d_out, out_host, canvas_bytes, hipMemcpyHostToDevice) != hipSuccess) { m->err = "hipMemcpy"; return IZPI_ERR_HIP; }
  } else if (hipMemset(root->d_out, 0, canvas_bytes) != hipSuccess) {
    m->err = "hipMemset";
    return IZPI_ERR_HIP;
  }
  int rc = on_every_device(m, [&](uint32_t i, izpi_ctx* c) {
    const int r = share(i, c);
    if (r) return r;
    hipError_t e = hipMemcpyPeerAsync(root->d_gather + (size_t)i * sh.block, root->device, c->d_share, c->device,
                                      sh.block * sizeof(double), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("gather copy: ") + hipGetErrorString(e); return (int)IZPI_ERR_HIP; }
    return (int)IZPI_OK;
  });
  if (rc) return rc;
  if (hipSetDevice(root->device) != hipSuccess) { m->err = "hipSetDevice"; return IZPI_ERR_HIP; }
  if ((rc = assemble(root, req, sh, root->d_out))) { m->err = root->err; return rc; }
  if (out_host && hipMemcpy(out_host, root->d_out, canvas_bytes, hipMemcpyDeviceToHost) != hipSuccess) {
    m->err = "hipMemcpy";
    return IZPI_ERR_HIP;
  }
  return IZPI_OK;
}

}  // namespace

namespace izpi_internal {
int prepare_rank_share(izpi_ctx* ctx, const izpi_render_req* req) {
  Shares sh;
  int rc = make_shares(ctx, req, ctx->comm_size, sh);
  if (!rc) rc = share_buffers(ctx, sh, ctx->comm_rank == 0);
  return rc ? rc : render_share(ctx, req, sh, ctx->comm_rank, true);
}
}  // namespace izpi_internal

extern "C" {

int izpi_gpu_unpack_tiles(izpi_ctx* ctx, const izpi_render_req* req, const double* packed_dev, double* canvas_dev) {
  if (!ctx || !req || !packed_dev || !canvas_dev || !req->num_tiles) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  uint32_t tw, th;
  if (!validate_tiles(req, req->tiles, req->num_tiles, &tw, &th)) { ctx->err = "bad tiles"; return IZPI_ERR_INVALID; }
  int rc = grow(ctx, (void**)&ctx->d_tiles, &ctx->tiles_cap, 4 * (size_t)req->num_tiles * sizeof(uint32_t));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->d_tiles, req->tiles, 4 * (size_t)req->num_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  const uint32_t np = req->num_tiles * tw * th;
  hipLaunchKernelGGL(k_unpack, dim3((np + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_tiles, np, tw, th, req->width,
                     req->height, packed_dev, canvas_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return IZPI_OK;
}

// ------------------------------------------------- multi-GPU, one process
int izpi_gpu_multi_open(const int* devices, uint32_t num_devices, izpi_multi** out) {
  if (!out) return IZPI_ERR_INVALID;
  *out = nullptr;
  if (!devices || num_devices == 0) return IZPI_ERR_INVALID;
  izpi_multi* m = new izpi_multi();
  for (uint32_t i = 0; i < num_devices; i++) {
    izpi_ctx* c = nullptr;
    const int rc = izpi_gpu_open(devices[i], &c);
    if (rc) {
      izpi_gpu_multi_close(m);
      return rc;
    }
    m->ctx.push_back(c);
  }
  // contexts on one device split its HBM when they size their workspaces
  for (izpi_ctx* c : m->ctx) {
    c->dev_share = 0;
    for (izpi_ctx* o : m->ctx) c->dev_share += o->device == c->device ? 1u : 0u;
  }
  // device 0 receives every share: let it read/write peers directly over xGMI
  for (uint32_t i = 1; i < num_devices; i++) {
    if (devices[i] == devices[0]) continue;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, devices[i], devices[0]) == hipSuccess && can) {
      (void)hipSetDevice(devices[i]);
      (void)hipDeviceEnablePeerAccess(devices[0], 0);  // "already enabled" is fine
      (void)hipGetLastError();
    }
  }
  *out = m;
  return IZPI_OK;
}

int izpi_gpu_multi_close(izpi_multi* m) {
  if (!m) return IZPI_OK;
  for (izpi_ctx* c : m->ctx) izpi_gpu_close(c);
  delete m;
  return IZPI_OK;
}

const char* izpi_gpu_multi_last_error(izpi_multi* m) { return m ? m->err.c_str() : "null context"; }

uint32_t izpi_gpu_multi_size(izpi_multi* m) { return m ? (uint32_t)m->ctx.size() : 0u; }

izpi_ctx* izpi_gpu_multi_context(izpi_multi* m, uint32_t i) { return (m && i < m->ctx.size()) ? m->ctx[i] : nullptr; }

int izpi_gpu_multi_upload_scene(izpi_multi* m, const izpi_scene_desc* scene) {
  if (!m) return IZPI_ERR_INVALID;
  if (multi_session_open(m)) return IZPI_ERR_INVALID;
  PackedScene ps;  // packed once (after the first context's checks); replicated per GPU
  for (size_t i = 0; i < m->ctx.size(); i++) {
    izpi_ctx* c = m->ctx[i];
    int rc = begin_upload(c, scene);
    if (!rc && i == 0) rc = pack_scene(scene, &ps, &c->err);
    if (!rc) rc = upload_packed(c, scene, ps);
    if (rc) {
      m->err = "device " + std::to_string(i) + ": " + c->err;
      return rc;
    }
  }
  return IZPI_OK;
}

int izpi_gpu_multi_render(izpi_multi* m, const izpi_render_req* req, double* out_host, izpi_render_stats* stats) {
  if (!multi_valid(m) || multi_session_open(m)) return IZPI_ERR_INVALID;
  Shares sh;
  int rc = multi_shares(m, req, sh);
  if (rc) return rc;
  if (req->post != IZPI_POST_NONE && req->num_tiles != 0) {
    m->err = "post-processing needs a whole-frame request";
    return IZPI_ERR_INVALID;
  }
  // every device renders its share
  rc = multi_frame(m, req, sh, out_host, [&](uint32_t i, izpi_ctx* c) {
    const int r = share_buffers(c, sh, false);
    return r ? r : render_share(c, req, sh, i);
  });
  for (size_t i = 0; stats && i < m->ctx.size(); i++) stats[i] = m->ctx[i]->last;
  return rc;
}

int izpi_gpu_multi_prepare(izpi_multi* m, const izpi_render_req* req) {
  if (!multi_valid(m)) return IZPI_ERR_INVALID;
  if (!req) { m->err = "null argument"; return IZPI_ERR_INVALID; }
  if (multi_session_open(m)) return IZPI_ERR_INVALID;
  Shares sh;
  const int rc = multi_shares(m, req, sh);
  if (rc) return rc;
  // the devices' workspaces, as izpi_gpu_multi_render renders them
  return on_every_device(m, [&](uint32_t i, izpi_ctx* c) {
    const int r = share_buffers(c, sh, false);
    return r ? r : render_share(c, req, sh, i, true);
  });
}

// A progressive session over the devices: izpi_gpu_multi_render's share plan, one session per
// device over its share's units (packed; a device without units has none).
int izpi_gpu_multi_progressive_begin(izpi_multi* m, const izpi_render_req* req, uint32_t step_spp) {
  return izpi_gpu_multi_progressive_begin_ex(m, req, step_spp, 0);
}

int izpi_gpu_multi_progressive_begin_ex(izpi_multi* m, const izpi_render_req* req, uint32_t step_spp, uint32_t flags) {
  if (!multi_valid(m)) return IZPI_ERR_INVALID;
  if (m->prog_open) { m->err = "a progressive session is already open"; return IZPI_ERR_INVALID; }
  if (!req || step_spp == 0) { m->err = "progressive_begin: a request and step_spp >= 1"; return IZPI_ERR_INVALID; }
  if (flags & ~(uint32_t)(IZPI_PROG_NOISE | IZPI_PROG_ADAPTIVE)) { m->err = "progressive_begin: unknown flags"; return IZPI_ERR_INVALID; }
  if ((flags & IZPI_PROG_ADAPTIVE) && !(flags & IZPI_PROG_NOISE)) { m->err = "progressive_begin: IZPI_PROG_ADAPTIVE needs IZPI_PROG_NOISE"; return IZPI_ERR_INVALID; }
  if ((flags & IZPI_PROG_ADAPTIVE) && preview_sampler(req->sampler)) { m->err = "progressive_begin: IZPI_PROG_ADAPTIVE with a preview sampler"; return IZPI_ERR_INVALID; }
  for (izpi_ctx* c : m->ctx)
    if (c->session.open) { m->err = "a context of this group has a progressive session of its own"; return IZPI_ERR_INVALID; }
  int rc = session_copy_request(m->session, req, m->err);
  if (rc) return rc;
  izpi_ctx::Session& ms = m->session;
  if (ms.req.spp == 0) { m->err = "invalid render request"; return IZPI_ERR_INVALID; }
  if (ms.req.post != IZPI_POST_NONE && ms.req.num_tiles != 0) {
    m->err = "post-processing needs a whole-frame request";
    return IZPI_ERR_INVALID;
  }
  ms.step_spp = std::min(step_spp, ms.req.spp);
  Shares sh;
  if ((rc = multi_shares(m, &ms.req, sh))) return rc;
  rc = on_every_device(m, [&](uint32_t i, izpi_ctx* c) {
    const int r = share_buffers(c, sh, false);
    if (r) return r;
    const std::vector<uint32_t> mine = sh.mine(i);
    if (mine.empty()) return (int)IZPI_OK;  // more shares than units
    const izpi_render_req q = share_request(ms.req, mine);
    return session_begin(c, &q, ms.step_spp, flags);
  });
  if (rc) {
    for (izpi_ctx* c : m->ctx) session_drop(c);
    return rc;
  }
  ms.noise = (flags & IZPI_PROG_NOISE) != 0;
  ms.adaptive = (flags & IZPI_PROG_ADAPTIVE) != 0;  // (ms.listed: an adapt has run, and ms.active is the devices' sum)
  m->shares = sh;
  m->prog_open = true;
  return IZPI_OK;
}

int izpi_gpu_multi_progressive_step(izpi_multi* m, uint32_t spp, izpi_render_stats* stats) {
  if (!multi_in_session(m)) return IZPI_ERR_INVALID;
  izpi_ctx::Session& ms = m->session;
  uint32_t n = std::min(spp ? spp : ms.step_spp, ms.req.spp - ms.done);
  if (ms.listed && ms.active == 0) n = 0;  // an adaptive session with no active pixel on any device
  // (A device whose own share has retired renders nothing and keeps its session's done where it
  // was: a device session's done may lag ms.done. Nothing reads it there: its snapshots and
  // statistic use the per-pixel counts, and its adapt finds no active pixel to evaluate.)
  int rc = IZPI_OK;
  if (n) rc = on_every_device(m, [&](uint32_t, izpi_ctx* c) { return c->session.open ? session_step(c, n, nullptr) : (int)IZPI_OK; });
  for (size_t i = 0; stats && i < m->ctx.size(); i++) stats[i] = m->ctx[i]->session.cum;
  if (rc) return rc;
  ms.done += n;
  return IZPI_OK;
}

int izpi_gpu_multi_progressive_snapshot(izpi_multi* m, uint32_t form, double* out_host) {
  if (!multi_in_session(m)) return IZPI_ERR_INVALID;
  const izpi_ctx::Session& ms = m->session;
  if (!snapshot_form_ok(form, ms.done, m->err)) return IZPI_ERR_INVALID;
  if (form == IZPI_SNAP_NOISE && session_lacks_noise(ms, m->err)) return IZPI_ERR_INVALID;
  if (form == IZPI_SNAP_SAMPLES && session_lacks_adaptive(ms, m->err)) return IZPI_ERR_INVALID;
  izpi_render_req q = ms.req;
  if (form != IZPI_SNAP_CANVAS) q.post = IZPI_POST_NONE;  // the display pixels and the standard errors are not post-processed
  // every device with a share resolves its sums into its packed block
  return multi_frame(m, &q, m->shares, out_host, [&](uint32_t, izpi_ctx* c) {
    return c->session.open ? session_snapshot(c, form, c->d_share) : (int)IZPI_OK;
  });
}

// The devices' statistics in one: the integers added, the largest maximum, sum_error added in
// device order (its last bits depend on the share plan), the slowest device's time.
int izpi_gpu_multi_progressive_noise(izpi_multi* m, const izpi_noise_params* p, izpi_noise_stats* out) {
  if (!multi_in_session(m)) return IZPI_ERR_INVALID;
  izpi_noise_params q;
  if (!noise_params_ok(p, q, m->err) || session_lacks_noise(m->session, m->err)) return IZPI_ERR_INVALID;
  std::vector<izpi_noise_stats> part(m->ctx.size());
  const int rc = on_every_device(m, [&](uint32_t i, izpi_ctx* c) { return c->session.open ? session_noise(c, &q, &part[i]) : (int)IZPI_OK; });
  if (rc) return rc;
  izpi_noise_stats s{};
  for (const izpi_noise_stats& d : part) {
    s.pixels += d.pixels; s.nonfinite += d.nonfinite; s.above += d.above;
    s.max_error = std::max(s.max_error, d.max_error);
    s.sum_error = s.sum_error + d.sum_error;
    s.device_ms = std::max(s.device_ms, d.device_ms);
  }
  s.done = m->session.done;
  s.converged = nz::converged(s.pixels, s.nonfinite, s.above, s.done, q);
  if (out) *out = s;
  return IZPI_OK;
}

// Every device adapts its own share (the rule is per pixel); the integers are added, the
// slowest device's time is the call's, and the frame rule reads the sums.
int izpi_gpu_multi_progressive_adapt(izpi_multi* m, const izpi_noise_params* p, izpi_adapt_stats* out) {
  if (!multi_in_session(m)) return IZPI_ERR_INVALID;
  izpi_noise_params q;
  izpi_ctx::Session& ms = m->session;
  if (!noise_params_ok(p, q, m->err) || session_lacks_adaptive(ms, m->err)) return IZPI_ERR_INVALID;
  if (ms.done < 2) { m->err = "adapt: needs at least 2 samples"; return IZPI_ERR_INVALID; }
  std::vector<izpi_adapt_stats> part(m->ctx.size());
  const int rc = on_every_device(m, [&](uint32_t i, izpi_ctx* c) { return c->session.open ? session_adapt(c, &q, &part[i]) : (int)IZPI_OK; });
  if (rc) return rc;
  izpi_adapt_stats s{};
  for (const izpi_adapt_stats& d : part) {
    s.pixels += d.pixels; s.nonfinite += d.nonfinite; s.active += d.active; s.retired += d.retired; s.samples += d.samples;
    s.device_ms = std::max(s.device_ms, d.device_ms);
  }
  ms.listed = true; ms.active = (uint32_t)s.active;
  s.done = ms.done;
  s.converged = nz::converged(s.pixels, s.nonfinite, s.active, s.done, q);
  if (out) *out = s;
  return IZPI_OK;
}

int izpi_gpu_multi_progressive_converge(izpi_multi* m, const izpi_noise_params* p, izpi_render_stats* stats, izpi_noise_stats* noise) {
  if (!multi_in_session(m)) return IZPI_ERR_INVALID;
  izpi_noise_params q;
  if (!noise_params_ok(p, q, m->err) || session_lacks_noise(m->session, m->err, 0)) return IZPI_ERR_INVALID;
  if (m->session.adaptive) {
    izpi_adapt_stats last{};
    bool idle = false;
    int rc = adapt_loop(q, m->session.req.spp, [&]() { return izpi_gpu_multi_progressive_step(m, 0, stats); },
                        [&](const izpi_noise_params& np, izpi_adapt_stats* as) { return izpi_gpu_multi_progressive_adapt(m, &np, as); },
                        [&]() { return m->session.done; }, &last, &idle);
    izpi_noise_stats ns{};
    if (!rc && (last.done || idle)) rc = izpi_gpu_multi_progressive_noise(m, &q, &ns);
    if (noise) *noise = ns;
    return rc;
  }
  return converge_loop(q, m->session.req.spp, [&]() { return izpi_gpu_multi_progressive_step(m, 0, stats); },
                       [&](const izpi_noise_params& np, izpi_noise_stats* ns) { return izpi_gpu_multi_progressive_noise(m, &np, ns); },
                       [&]() { return m->session.done; }, noise);
}

// ---- checkpoint and resume of the group's session
int izpi_gpu_multi_progressive_checkpoint_bytes(izpi_multi* m, uint64_t* bytes) {
  if (!multi_in_session(m)) return IZPI_ERR_INVALID;
  if (!bytes) { m->err = "null output"; return IZPI_ERR_INVALID; }
  const izpi_ctx::Session& ms = m->session;
  *bytes = ck::Layout(ms.req.width, ms.req.height, (ms.noise ? (uint32_t)IZPI_PROG_NOISE : 0u) | (ms.adaptive ? (uint32_t)IZPI_PROG_ADAPTIVE : 0u)).bytes;
  return IZPI_OK;
}

// One blob for the frame: every device exports its share's blob (the frame's planes with its own
// pixels present), and the host copies each present record into the caller's. The shares are
// disjoint but for pixels of overlapping tiles, whose records are equal. The header's integers
// and counters are the devices' sums, done is the group's.
int izpi_gpu_multi_progressive_checkpoint(izpi_multi* m, uint64_t scene_tag, void* out_host, uint64_t cap) {
  if (!multi_in_session(m)) return IZPI_ERR_INVALID;
  const izpi_ctx::Session& ms = m->session;
  if (!out_host) { m->err = "null output"; return IZPI_ERR_INVALID; }
  if (ms.done == 0) { m->err = "checkpoint: before the session's first sample (done == 0)"; return IZPI_ERR_INVALID; }
  const uint32_t flags = (ms.noise ? (uint32_t)IZPI_PROG_NOISE : 0u) | (ms.adaptive ? (uint32_t)IZPI_PROG_ADAPTIVE : 0u);
  const ck::Layout l(ms.req.width, ms.req.height, flags);
  if (cap < l.bytes) {
    m->err = "checkpoint: the output holds " + std::to_string(cap) + " bytes, the blob takes " + std::to_string(l.bytes);
    return IZPI_ERR_INVALID;
  }
  std::vector<std::vector<char>> part(m->ctx.size());
  for (size_t i = 0; i < part.size(); i++)
    if (m->ctx[i]->session.open) part[i].resize(l.bytes);
  const int rc = on_every_device(m, [&](uint32_t i, izpi_ctx* c) {
    return c->session.open ? session_checkpoint(c, scene_tag, part[i].data(), l.bytes) : (int)IZPI_OK;
  });
  if (rc) return rc;
  char* out = (char*)out_host;
  memset(out, 0, l.bytes);
  const ck::Planes f = ck::planes_at(out, 0, l);
  memset(f.state, ck::NOT_IN_SESSION, l.n);
  ck::Header h = checkpoint_header(ms.req, flags, scene_tag);
  h.cnt_n = CNT_N;
  for (std::vector<char>& b : part) {
    if (b.empty()) continue;
    ck::Header d;
    memcpy(&d, b.data(), sizeof d);
    h.listed |= d.listed; h.samples += d.samples; h.active += d.active;
    for (uint32_t k = 0; k < CNT_N; k++) h.counters[k] += d.counters[k];
    const ck::Planes s = ck::planes_at(b.data(), 0, l);
    for (uint64_t i = 0; i < l.n; i++) {
      if (s.state[i] == ck::NOT_IN_SESSION) continue;
      f.state[i] = s.state[i];
      memcpy(f.sums + 3 * i, s.sums + 3 * i, 24);
      if (f.moments) memcpy(f.moments + 3 * i, s.moments + 3 * i, 24);
      if (f.counts) f.counts[i] = s.counts[i];
    }
  }
  for (uint64_t i = 0; i < l.n; i++) h.pixels += f.state[i] != ck::NOT_IN_SESSION;
  h.done = ms.done;
  memcpy(out, &h, sizeof h);
  h.checksum = checkpoint_checksum(out, l.bytes);
  memcpy(out, &h, sizeof h);
  return IZPI_OK;
}

// begin_ex's checks and share plan with the blob's flags; every device resumes the pixels of its
// own share (session_resume's share form: it refuses a pixel without a record), and the first
// device with a share takes the stored counters, so that the devices' sums run on. Whether a
// record belongs to no pixel of the frame is checked here, on the host, over the units: the
// devices' marks would have to be merged first.
int izpi_gpu_multi_progressive_resume(izpi_multi* m, const izpi_render_req* req, uint32_t step_spp, uint64_t scene_tag,
                                      const void* blob, uint64_t bytes) {
  if (!multi_valid(m)) return IZPI_ERR_INVALID;
  if (m->prog_open) { m->err = "a progressive session is already open"; return IZPI_ERR_INVALID; }
  if (!req || step_spp == 0) { m->err = "progressive_resume: a request and step_spp >= 1"; return IZPI_ERR_INVALID; }
  for (izpi_ctx* c : m->ctx)
    if (c->session.open) { m->err = "a context of this group has a progressive session of its own"; return IZPI_ERR_INVALID; }
  char msg[160];
  if (const char* bad = checkpoint_check(blob, bytes, req, scene_tag, msg, sizeof msg)) { m->err = bad; return IZPI_ERR_INVALID; }
  ck::Header h;
  memcpy(&h, blob, sizeof h);
  int rc = session_copy_request(m->session, req, m->err);
  if (rc) return rc;
  izpi_ctx::Session& ms = m->session;
  auto fail = [&](int status) {
    for (izpi_ctx* c : m->ctx) session_drop(c);
    ms = izpi_ctx::Session{};
    return status;
  };
  if (ms.req.post != IZPI_POST_NONE && ms.req.num_tiles != 0) {
    m->err = "post-processing needs a whole-frame request";
    return fail(IZPI_ERR_INVALID);
  }
  ms.step_spp = std::min(step_spp, ms.req.spp);
  Shares sh;
  if ((rc = multi_shares(m, &ms.req, sh))) return fail(rc);
  const ck::Layout l(h.width, h.height, h.flags);
  {
    std::vector<uint8_t> mine(l.n, 0);
    for (size_t u = 0; u < sh.all.size() / 4; u++)
      for (uint32_t y = sh.all[4 * u + 1]; y <= sh.all[4 * u + 3]; y++)
        for (uint32_t x = sh.all[4 * u]; x <= sh.all[4 * u + 2]; x++) mine[(size_t)y * h.width + x] = 1;
    const uint8_t* state = (const uint8_t*)blob + l.state;
    uint64_t absent = 0, unclaimed = 0;
    for (uint64_t i = 0; i < l.n; i++) {
      absent += mine[i] && state[i] == ck::NOT_IN_SESSION;
      unclaimed += !mine[i] && state[i] != ck::NOT_IN_SESSION;
    }
    if (absent || unclaimed) {
      m->err = absent ? "checkpoint: " + std::to_string(absent) + " pixels of the request have no record in it (the pixel sets differ)"
                      : "checkpoint: " + std::to_string(unclaimed) + " of its records belong to no pixel of the request (the pixel sets differ)";
      return fail(IZPI_ERR_INVALID);
    }
  }
  uint32_t first = (uint32_t)m->ctx.size();
  for (uint32_t i = 0; i < m->ctx.size() && first == m->ctx.size(); i++)
    if (!sh.mine(i).empty()) first = i;
  rc = on_every_device(m, [&](uint32_t i, izpi_ctx* c) {
    const int r = share_buffers(c, sh, false);
    if (r) return r;
    const std::vector<uint32_t> mine = sh.mine(i);
    if (mine.empty()) return (int)IZPI_OK;
    const izpi_render_req q = share_request(ms.req, mine);
    return session_resume(c, &q, ms.step_spp, scene_tag, blob, bytes, true, i != first);
  });
  if (rc) return fail(rc);
  ms.noise = (h.flags & IZPI_PROG_NOISE) != 0;
  ms.adaptive = (h.flags & IZPI_PROG_ADAPTIVE) != 0;
  ms.listed = h.listed != 0; ms.active = (uint32_t)h.active;
  ms.done = h.done;
  m->shares = sh;
  m->prog_open = true;
  return IZPI_OK;
}

int izpi_gpu_multi_progressive_end(izpi_multi* m) {
  if (!multi_in_session(m)) return IZPI_ERR_INVALID;
  for (izpi_ctx* c : m->ctx) session_drop(c);
  m->session = izpi_ctx::Session{};
  m->prog_open = false;
  return IZPI_OK;
}

// ------------------------------------------ multi-GPU, one process per GPU
int izpi_gpu_comm_id(uint8_t* id) {
  if (!id) return IZPI_ERR_INVALID;
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return IZPI_ERR_HIP;
  memcpy(id, u.internal, IZPI_COMM_ID_BYTES);
  return IZPI_OK;
}

int izpi_gpu_comm_init(izpi_ctx* ctx, uint32_t nranks, uint32_t rank, const uint8_t* id) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (!id || nranks == 0 || rank >= nranks) { ctx->err = "comm_init: bad arguments"; return IZPI_ERR_INVALID; }
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->comm) { (void)ncclCommDestroy(ctx->comm); ctx->comm = nullptr; }
  // the status word of izpi_gpu_render_rank's agreement steps, allocated here so that a
  // render never fails to reach them for want of it
  if (!ctx->d_status) HIP_TRY(hipMalloc((void**)&ctx->d_status, 2 * sizeof(int32_t)));
  ncclUniqueId u;
  memcpy(u.internal, id, IZPI_COMM_ID_BYTES);
  const ncclResult_t r = ncclCommInitRank(&ctx->comm, (int)nranks, u, (int)rank);
  if (r != ncclSuccess) {
    ctx->comm = nullptr;
    ctx->err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r);
    return IZPI_ERR_HIP;
  }
  ctx->comm_rank = rank;
  ctx->comm_size = nranks;
  return IZPI_OK;
}

}  // extern "C"

namespace {
// Agreement step of a multi-rank render: every rank contributes (status << 16 | rank) and
// all receive the maximum, i.e. the worst status and the highest rank that had it
// (ncclAllReduce(max), rccl.h). Returns non-zero only if the collective itself failed.
// Device-side stall of the fault-injection hook (izpi_gpu_debug_fault 3): one thread spins
// until the host sets *release (a coherent pinned word), as a stream stuck in a collective
// on a dead peer does; bounded (about 7 s of clock) so that the grid always drains.
__global__ void k_stall(const volatile uint32_t* release) {
  const uint64_t t0 = __builtin_readcyclecounter();
  while (__atomic_load_n(release, __ATOMIC_RELAXED) == 0u && __builtin_readcyclecounter() - t0 < (1ull << 34))
    __builtin_amdgcn_s_sleep(100);
}

// Wait for this context's stream (a collective step) as a rank that may outlive its peers:
// poll the stream and the communicator's asynchronous error; an RCCL error, a HIP error of
// this rank's stream or a wait past the deadline aborts the communicator and returns
// IZPI_ERR_PEER (render/remote.go:40-55 logs a failed remote tile and carries on; here the
// call returns instead of hanging). After a local HIP error this rank cannot join the
// remaining collectives, and peers blocked in them would never return: aborting the
// communicator ends their waits too (they see the async error), and the communicator is
// gone on this rank (izpi_gpu_comm_init makes a new one).
int wait_peers(izpi_ctx* ctx, uint32_t timeout_ms, const char* step) {
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t naps = 0;
  for (;;) {
    hipError_t q = hipStreamQuery(ctx->stream);
    if (ctx->fault_inject == 4 && q != hipErrorNotReady) q = hipErrorLaunchFailure;  // test hook: a failed stream
    if (q == hipSuccess) return IZPI_OK;
    ncclResult_t ae = ncclSuccess;
    const ncclResult_t qr = q == hipErrorNotReady ? ncclCommGetAsyncError(ctx->comm, &ae) : ncclSuccess;
    const bool failed = qr != ncclSuccess || (ae != ncclSuccess && ae != ncclInProgress);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (q != hipErrorNotReady || failed || (timeout_ms && ms > timeout_ms)) {
      ctx->err = std::string(step) +
                 (q != hipErrorNotReady ? ": this rank's stream failed: " + std::string(hipGetErrorString(q))
                  : failed ? ": RCCL reported " + std::string(ncclGetErrorString(qr != ncclSuccess ? qr : ae))
                           : ": no answer from the other ranks within " + std::to_string(timeout_ms) + " ms") +
                 "; communicator aborted";
      // test hook: let the stall drain first (ncclCommAbort waits for the operations it
      // aborts, which sit behind it on the stream)
      if (ctx->stall_word) { *ctx->stall_word = 1u; ctx->stall_word = nullptr; }
      (void)ncclCommAbort(ctx->comm);
      ctx->comm = nullptr;
      (void)hipStreamSynchronize(ctx->stream);
      return IZPI_ERR_PEER;
    }
    // sub-millisecond polls at first (a collective normally completes in microseconds),
    // then 1 ms naps for a gather that waits on the slowest rank's render
    std::this_thread::sleep_for(std::chrono::microseconds(naps++ < 200 ? 20 : 1000));
  }
}

// Agree on the worst status over all ranks. The collective is issued whatever failed
// locally before it (a failed staging copy only makes this rank's word stale), so that no
// rank is left waiting in it; a local HIP error is reported after the collective.
int agree_status(izpi_ctx* ctx, int local, uint32_t timeout_ms, int* worst_status, uint32_t* worst_rank) {
  const int32_t word = (int32_t)((uint32_t)std::min(local, 0x7FFF) << 16 | (ctx->comm_rank & 0xFFFFu));
  int32_t* h = (int32_t*)ctx->h_count + 8 * MISC_STRIDE;  // pinned scratch
  h[0] = word;
  h[1] = word;  // this rank's own word, should the collective's copy-back fail
  const hipError_t e1 = hipMemcpyAsync(ctx->d_status, h, sizeof(word), hipMemcpyHostToDevice, ctx->stream);
  const ncclResult_t r = ncclAllReduce(ctx->d_status, ctx->d_status + 1, 1, ncclInt32, ncclMax, ctx->comm, ctx->stream);
  if (r != ncclSuccess) {
    ctx->err = std::string("ncclAllReduce: ") + ncclGetErrorString(r) + "; communicator aborted";
    (void)ncclCommAbort(ctx->comm);
    ctx->comm = nullptr;
    return IZPI_ERR_PEER;
  }
  const hipError_t e2 = hipMemcpyAsync(h + 1, ctx->d_status + 1, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
  const int rc = wait_peers(ctx, timeout_ms, "status agreement");
  if (rc) return rc;
  if (e1 != hipSuccess || e2 != hipSuccess) {
    ctx->err = std::string("status agreement: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2);
    return IZPI_ERR_HIP;
  }
  const int32_t out = h[1];
  *worst_status = (int)((uint32_t)out >> 16);
  *worst_rank = (uint32_t)out & 0xFFFFu;
  return IZPI_OK;
}

// A rank whose own step succeeded returns IZPI_ERR_PEER when another rank's failed.
int peer_failure(izpi_ctx* ctx, int worst, uint32_t worst_rank, const char* when) {
  ctx->err = "rank " + std::to_string(worst_rank) + " failed " + when + " (status " + std::to_string(worst) + ")";
  return IZPI_ERR_PEER;
}
}  // namespace

extern "C" {

// Every rank runs the same sequence of collectives whatever fails locally, so no rank is
// left waiting in one (render/remote.go:40-55 logs a failed remote tile; here every rank
// learns the worst status):
//   1. local checks and buffers (share block; gather buffer on rank 0), then agree: if any
//      rank failed, all return before rendering;
//   2. render the share (a failed share posts a zeroed block), ncclGather to rank 0, agree
//      again: if any rank failed, all return it and rank 0 does not assemble;
//   3. rank 0 assembles and post-processes (a failure there is rank 0's alone).
int izpi_gpu_render_rank(izpi_ctx* ctx, const izpi_render_req* req, double* out_dev, izpi_render_stats* stats) {
  if (!ctx) return IZPI_ERR_INVALID;
  // without a communicator no collective can run: every rank in this state returns here
  if (!ctx->comm || !ctx->d_status) { ctx->err = "render_rank before izpi_gpu_comm_init"; return IZPI_ERR_INVALID; }
  if (session_open(ctx)) return IZPI_ERR_INVALID;  // (the caller's error on every rank alike: no collective has started)
  memset(&ctx->last, 0, sizeof(ctx->last));
  ctx->prog_done.store(0, std::memory_order_relaxed);  // (no stale count while the ranks agree)
  ctx->prog_total.store(0, std::memory_order_relaxed);
  if (stats) *stats = ctx->last;
  const uint32_t timeout_ms = tuning_of(req).peer_timeout_ms;
  // ---- 1 (local failures, HIP ones included, are recorded and agreed on, not returned early)
  Shares sh;
  int prc = IZPI_OK;
  const hipError_t de = hipSetDevice(ctx->device);
  if (de != hipSuccess) { ctx->err = std::string("hipSetDevice: ") + hipGetErrorString(de); prc = IZPI_ERR_HIP; }
  else if (ctx->comm_rank == 0 && !out_dev) { ctx->err = "rank 0 needs an output canvas"; prc = IZPI_ERR_INVALID; }
  else if (req && req->post != IZPI_POST_NONE && req->num_tiles != 0) { ctx->err = "post-processing needs a whole-frame request"; prc = IZPI_ERR_INVALID; }
  if (!prc) prc = make_shares(ctx, req, ctx->comm_size, sh);
  if (!prc) prc = share_buffers(ctx, sh, ctx->comm_rank == 0);
  if (prc == IZPI_OK && ctx->fault_inject == 1) { ctx->err = "injected fault before rendering"; prc = IZPI_ERR_DEVICE; }
  const std::string local_err = ctx->err;
  int worst = 0;
  uint32_t wr = 0;
  int rc = agree_status(ctx, prc, timeout_ms, &worst, &wr);
  if (rc) return rc;
  if (prc) { ctx->err = local_err; return prc; }
  if (worst) return peer_failure(ctx, worst, wr, "before rendering");
  // ---- 2 (a failed share posts a zeroed block: the gather runs on every rank)
  int rrc = render_share(ctx, req, sh, ctx->comm_rank);
  if (stats) *stats = ctx->last;
  if (rrc) (void)hipMemsetAsync(ctx->d_share, 0, sh.block * sizeof(double), ctx->stream);
  if (ctx->fault_inject == 3) {  // test hook: this rank's stream stalls as on a dead peer
    // the release word is fine-grained (coherent) host memory: the spinning kernel sees
    // the host's store while it runs
    if (!ctx->stall_host && hipHostMalloc((void**)&ctx->stall_host, 64, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
      ctx->stall_host = nullptr;
    if (ctx->stall_host) {
      ctx->stall_word = ctx->stall_host;
      *ctx->stall_word = 0u;
      hipLaunchKernelGGL(k_stall, dim3(1), dim3(1), 0, ctx->stream, (const volatile uint32_t*)ctx->stall_word);
    }
  }
  // ncclGather (rccl.h:745): block r of the root's buffer = rank r's packed share
  const ncclResult_t r = ncclGather(ctx->d_share, ctx->comm_rank == 0 ? ctx->d_gather : nullptr, sh.block, ncclFloat64, 0,
                                    ctx->comm, ctx->stream);
  if (r != ncclSuccess) {  // the peers may already wait in the gather: abort rather than leave them there
    ctx->err = std::string("ncclGather: ") + ncclGetErrorString(r) + "; communicator aborted";
    if (ctx->stall_word) { *ctx->stall_word = 1u; ctx->stall_word = nullptr; }
    (void)ncclCommAbort(ctx->comm);
    ctx->comm = nullptr;
    (void)hipStreamSynchronize(ctx->stream);
    return IZPI_ERR_PEER;
  }
  if ((rc = wait_peers(ctx, timeout_ms, "share gather"))) return rc;
  const std::string share_err = ctx->err;
  if ((rc = agree_status(ctx, rrc, timeout_ms, &worst, &wr))) return rc;
  if (rrc) { ctx->err = share_err; return rrc; }
  if (worst) return peer_failure(ctx, worst, wr, "while rendering its share");
  // ---- 3
  if (ctx->comm_rank == 0 && (rc = assemble(ctx, req, sh, out_dev))) return rc;
  return IZPI_OK;
}

uint64_t izpi_host_share_block(uint32_t num_tiles, uint32_t tile_w, uint32_t tile_h, uint32_t num_shares) {
  return num_shares ? share_block(num_tiles, tile_w, tile_h, num_shares) : 0;
}

int izpi_host_assemble_shares(uint32_t width, uint32_t height, const uint32_t* tiles, uint32_t num_tiles,
                              uint32_t num_shares, const double* gathered, double* canvas) {
  if (!tiles || !gathered || !canvas || num_tiles == 0 || num_shares == 0 || width == 0 || height == 0) return IZPI_ERR_INVALID;
  izpi_render_req req{};
  req.width = width; req.height = height;
  uint32_t tw = 0, th = 0;
  if (!validate_tiles(&req, tiles, num_tiles, &tw, &th)) return IZPI_ERR_INVALID;
  const size_t block = share_block(num_tiles, tw, th, num_shares);
  std::vector<uint32_t> mine(4 * (size_t)num_tiles);
  for (uint32_t r = 0; r < num_shares; r++) {
    const uint32_t nt = izpi_host_share_tiles(tiles, num_tiles, r, num_shares, mine.data());
    const double* packed = gathered + (size_t)r * block;
    const PixelMap map{nt * tw * th, width, height, tw, th, IZPI_OUT_CANVAS, mine.data()};
    for (uint32_t p = 0; p < map.num_pixels; p++)
      if (double* o = map.slot(p, canvas)) memcpy(o, packed + (size_t)p * 4, 4 * sizeof(double));
  }
  return IZPI_OK;
}

int izpi_gpu_multi_progress(izpi_multi* m, uint64_t* samples_done, uint64_t* samples_total) {
  if (!m || !samples_done || !samples_total) return IZPI_ERR_INVALID;
  *samples_done = 0; *samples_total = 0;
  for (izpi_ctx* c : m->ctx) {
    uint64_t d = 0, t = 0;
    izpi_gpu_progress(c, &d, &t);
    *samples_done += d; *samples_total += t;
  }
  return IZPI_OK;
}

}  // extern "C"
