// izpi_gpu.hip — the C ABI of the MI355X path-tracing inner loop for izpi (include/izpi_gpu.h):
// contexts, scene upload, the render call (its workspace is planned in render_plan.cpp), multi-GPU
// (threads and RCCL ranks), post-processing and the component entries. The kernels of the
// hot path are in trace.hip and shade.hip (izpi_kern.h).
#include "izpi_kern.h"
#include "noise.h"
#include "scene_pack.h"

#include <array>

using izpi_internal::Double4;
using izpi_internal::pack_scene;
using izpi_internal::PackedScene;
using izpi_internal::trace_addr32;
using izpi_internal::trace_layout;
using izpi_internal::TraceLayout;
using izpi_internal::PlanCache;
using izpi_internal::PlanInput;
using izpi_internal::SideLayout;
using izpi_internal::WorkspacePlan;

// FireflyRejection (firefly_rejection.go:12-113) fused with XYZToRGB (rgb_image.go:28-67).
// FireflyRejection reads only the ORIGINAL Y plane (it copies it first, :33-39) and
// scales the pixel's own X, Y, Z, so pixels are independent: one thread per pixel, the
// 18x18 Y halo of a 16x16 tile staged in LDS. The scaled XYZ then goes through the
// exposure multiply and the ACEScg matrix in XYZToRGB's operation order.
__global__ void __launch_bounds__(256) k_spectral_post(const double* in, double* out, uint32_t W, uint32_t H,
                                                       double exposure) {
  __shared__ double ys[18][18];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
  for (int i = threadIdx.x; i < 18 * 18; i += 256) {
    const int hx = x0 + (i % 18) - 1, hy = y0 + (i / 18) - 1;
    ys[i / 18][i % 18] = (hx >= 0 && hx < (int)W && hy >= 0 && hy < (int)H) ? in[((size_t)hy * W + hx) * 4 + 1] : 0.0;
  }
  __syncthreads();
  const int x = x0 + tx, y = y0 + ty;
  if (x >= (int)W || y >= (int)H) return;
  const size_t pi = ((size_t)y * W + x) * 4;
  const double2 xy = *reinterpret_cast<const double2*>(in + pi), za = *reinterpret_cast<const double2*>(in + pi + 2);
  double X = xy.x, Y = xy.y, Z = za.x;
  const double cur = ys[ty + 1][tx + 1];
  if (cur > 0) {  // `currentY <= 0` skips (NaN does not)
    double nb[8];
    int nn = 0;
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        if (dx == 0 && dy == 0) continue;
        const int nx = x + dx, ny = y + dy;
        if (nx >= 0 && nx < (int)W && ny >= 0 && ny < (int)H) {
          const double v = ys[ty + 1 + dy][tx + 1 + dx];
          if (v > 0) nb[nn++] = v;
        }
      }
    if (nn >= 3) {
      double sum = 0.0;
      for (int i = 0; i < nn; i++) sum += nb[i];
      const double mean = sum / (double)nn;
      double vs = 0.0;
      for (int i = 0; i < nn; i++) { const double d = nb[i] - mean; vs += d * d; }
      const double stddev = gm::sqrt(vs / (double)nn);
      const double threshold = mean + 2.5 * stddev;
      if (cur > threshold && threshold > 0) {
        const double ratio = threshold / cur;
        X *= ratio; Y *= ratio; Z *= ratio;
      }
    }
  }
  X *= exposure; Y *= exposure; Z *= exposure;
  double2 rg, ba;
  rg.x = 1.6410234 * X + -0.3248033 * Y + -0.2364247 * Z;
  rg.y = -0.6636629 * X + 1.6153316 * Y + 0.0167563 * Z;
  ba.x = 0.0117219 * X + -0.0082845 * Y + 0.9883949 * Z;
  ba.y = za.y;  // alpha unchanged
  *reinterpret_cast<double2*>(out + pi) = rg;
  *reinterpret_cast<double2*>(out + pi + 2) = ba;
}

// postprocess.Pipeline (pipeline.go:20-31) of Gamma (gamma.go:24-41: R,G,B = math.Sqrt)
// and Clamp (clamp.go:27-51: v < max ? v : max, so NaN -> max) filters, applied in list
// order to each pixel; alpha unchanged. The reference walks x <= Max.X, y <= Max.Y: the
// extra row/column reads zero and its Set is dropped, so only in-bounds pixels change.
// HBM-streaming, 32 B in + 32 B out per pixel.
struct PostFilters {
  uint32_t n;
  uint32_t kind[IZPI_MAX_FILTERS];
  double param[IZPI_MAX_FILTERS];
};

__global__ void __launch_bounds__(256) k_postprocess(double* canvas, uint64_t num_pixels, const PostFilters pf) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num_pixels) return;
  double2* p = reinterpret_cast<double2*>(canvas + i * 4);
  double2 rg = p[0], ba = p[1];
  double c[3] = {rg.x, rg.y, ba.x};
  for (uint32_t f = 0; f < pf.n; f++) {
    if (pf.kind[f] == IZPI_FILTER_GAMMA) {
      for (int k = 0; k < 3; k++) c[k] = gm::sqrt(c[k]);
    } else {
      const double mx = pf.param[f];
      for (int k = 0; k < 3; k++) c[k] = c[k] < mx ? c[k] : mx;
    }
  }
  p[0] = make_double2(c[0], c[1]);
  p[1] = make_double2(c[2], ba.y);
}

// Packed pixel p (IZPI_OUT_PACKED: tile after tile, the rows of each tile) -> its canvas
// column x and row H - y (rgb.go:41); false for sample row y = 0, which has no canvas row.
// k_unpack and izpi_host_assemble_shares share this rule.
__host__ __device__ inline bool packed_target(const uint32_t* tiles, uint32_t p, uint32_t tile_w, uint32_t tile_h,
                                              uint32_t height, uint32_t* x, uint32_t* row) {
  const uint32_t tile_px = tile_w * tile_h;
  const uint32_t tile = p / tile_px, in_tile = p % tile_px;
  *x = tiles[4 * tile] + in_tile % tile_w;
  *row = height - (tiles[4 * tile + 1] + in_tile / tile_w);
  return *row < height;
}
__global__ void k_unpack(const uint32_t* tiles, uint32_t num_pixels, uint32_t tile_w, uint32_t tile_h, uint32_t width,
                         uint32_t height, const double* packed, double* canvas) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= num_pixels) return;
  uint32_t x, row;
  if (packed_target(tiles, p, tile_w, tile_h, height, &x, &row)) {
    const double* s = packed + (size_t)p * 4;
    double* o = canvas + ((size_t)row * width + x) * 4;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
  }
}

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

// ------------------------------------------------------- component kernels
// izpi_gpu_trace: rays [n][8] -> queue entries with explicit (tMin, tMax)
__global__ void k_trace_setup(const double* rays, uint32_t n, RayOD* ray, uint32_t* kind, double2* tminmax, uint32_t* qn) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *qn = n;
  if (i >= n) return;
  const double* r = rays + (size_t)i * 8;
  RayOD h;
  for (int k = 0; k < 3; k++) { h.o[k] = r[k]; h.d[k] = r[3 + k]; }
  ray[i] = h;
  kind[i] = RAY_PATHLEN;  // not a Sampler call
  tminmax[i] = make_double2(r[6], r[7]);
}
__global__ void k_trace_records(const DevScene sc, const RayOD* rr, const double2* hit, uint32_t n, izpi_hit* out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  izpi_hit h;
  memset(&h, 0, sizeof(h));
  h.prim_ref = 0xFFFFFFFFu;
  HitOut c;
  const double2* rec = hit + 2 * (size_t)i;  // (t, prim), (u, v)
  c.t = rec[0].x; c.prim = hit_prim(rec[0]); c.u = rec[1].x; c.v = rec[1].y; c.pad = 0;
  if (c.prim >= 0) {
    const RayOD R = rr[i];
    HitRec hr;
    const GShade gs = sc.shade[c.prim];
    hit_record(sc, c, rec + 1, gs, mk(R.o[0], R.o[1], R.o[2]), mk(R.d[0], R.d[1], R.d[2]), 0.0, true, hr);
    const GPrim& p = sc.prims[c.prim];
    h.hit = 1; h.t = hr.t; h.u = hr.u; h.v = hr.v;
    h.p[0] = hr.p.x; h.p[1] = hr.p.y; h.p[2] = hr.p.z;
    h.normal[0] = hr.n.x; h.normal[1] = hr.n.y; h.normal[2] = hr.n.z;
    h.prim_ref = IZPI_PRIM_REF(p.kind, p.index);
  }
  out[i] = h;
}

__global__ void k_aabb4(const float* boxes, const float* rays, uint32_t n, uint8_t* masks) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* b = boxes + (size_t)i * 24;
  const float* r = rays + (size_t)i * 7;
  uint8_t m = 0;
  for (int k = 0; k < 4; k++)
    if (slab(b[k], b[4 + k], b[8 + k], b[12 + k], b[16 + k], b[20 + k], r[0], r[1], r[2], r[3], r[4], r[5], r[6])) m |= (uint8_t)(1 << k);
  masks[i] = m;
}

__global__ void k_gomath(const DevScene sc, int op, const double* x, const double* y, uint32_t n, double* out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (op == 14) {  // path_length(hit point x[i], exit point y[i]): 3 doubles each
    out[i] = path_length(mk(x[3 * i], x[3 * i + 1], x[3 * i + 2]), mk(y[3 * i], y[3 * i + 1], y[3 * i + 2]));
    return;
  }
  double a = x[i], b = y ? y[i] : 0.0, r;
  switch (op) {
    case 0: r = gm::sin(a); break;
    case 1: r = gm::cos(a); break;
    case 2: r = gm::tan(a); break;
    case 3: r = gm::exp(a); break;
    case 4: r = gm::log(a); break;
    case 5: r = gm::pow(a, b); break;
    case 6: r = gm::atan2(a, b); break;
    case 7: r = gm::asin(a); break;
    case 8: r = gm::sqrt(a); break;
    case 9: r = a / b; break;
    case 10: r = gm::atan(a); break;
    case 11: case 12: { double sv, cv; gm::sincos_nonneg(a, &sv, &cv); r = op == 11 ? sv : cv; break; }
    case 13: r = sdiv(mk(a, 0.0, 0.0), b).x; break;  // sdiv's shared reciprocal (= a / b)
    case 32: case 33: { double l, pdf; sample_wavelength(a, l, pdf); r = op == 32 ? l : pdf; break; }
    case 34: case 35: case 36: { double cx, cy, cz; cie_values(a, cx, cy, cz); r = op == 34 ? cx : op == 35 ? cy : cz; break; }
    case 37: r = tex_spectral(sc, (int32_t)b, a); break;
    default: r = gm::nan();
  }
  out[i] = r;
}

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

int grow(izpi_ctx* ctx, void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return IZPI_OK;
  if (*p) HIP_TRY(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  HIP_TRY(hipMalloc(p, bytes));
  *cap = bytes;
  return IZPI_OK;
}

// Every device buffer `grow` manages. The first RENDER_BUFS are the ones a render sizes per
// frame and may release to re-size (not the output, share, gather and post-processing
// buffers, which it never frees), in the order of izpi_gpu_debug_realloc's mask bits.
struct CtxBuf {
  void** p;
  size_t* cap;
};
constexpr size_t RENDER_BUFS = 7, CTX_BUFS = 19;
std::array<CtxBuf, CTX_BUFS> ctx_buffers(izpi_ctx* c) {
#define IZPI_BUF(name) CtxBuf{(void**)&c->d_##name, &c->name##_cap}
  return {IZPI_BUF(samples), IZPI_BUF(recs), IZPI_BUF(pool), IZPI_BUF(ring), IZPI_BUF(running), IZPI_BUF(state),
          IZPI_BUF(spill), IZPI_BUF(out), IZPI_BUF(tiles), IZPI_BUF(utiles), IZPI_BUF(bg), IZPI_BUF(post),
          IZPI_BUF(share), IZPI_BUF(gather), IZPI_BUF(cpart), IZPI_BUF(finq), IZPI_BUF(denoise),
          IZPI_BUF(moments), IZPI_BUF(noisepart)};
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

// Render's post-processing of a whole-frame canvas on the context's stream: the Spectral
// sampler's FireflyRejection + XYZToRGB (renderer.go:215-219), then the leader's "png"
// pipeline, Gamma and Clamp(1.0) (leader.go:179-182).
int apply_post(izpi_ctx* ctx, const izpi_render_req* req, double* canvas_dev) {
  hipStream_t st = ctx->stream;
  int rc;
  if (req->post & IZPI_POST_SPECTRAL) {
    if ((rc = grow(ctx, (void**)&ctx->d_post, &ctx->post_cap, (size_t)req->width * req->height * 4 * sizeof(double)))) return rc;
    dim3 g((req->width + 15) / 16, (req->height + 15) / 16);
    hipLaunchKernelGGL(k_spectral_post, g, dim3(256), 0, st, canvas_dev, ctx->d_post, req->width, req->height, req->exposure);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(canvas_dev, ctx->d_post, (size_t)req->width * req->height * 4 * sizeof(double),
                           hipMemcpyDeviceToDevice, st));
  }
  if (req->post & IZPI_POST_GAMMA_CLAMP) {
    PostFilters pf;
    memset(&pf, 0, sizeof pf);
    pf.n = 2; pf.kind[0] = IZPI_FILTER_GAMMA; pf.kind[1] = IZPI_FILTER_CLAMP; pf.param[1] = 1.0;
    const uint64_t np = (uint64_t)req->width * req->height;
    hipLaunchKernelGGL(k_postprocess, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, canvas_dev, np, pf);
    HIP_TRY(hipGetLastError());
  }
  return IZPI_OK;
}

// How a render call is driven: the samples it renders, the samples its workspace is sized
// for (the request's, or a progressive session's step_spp: the sums then stay in d_running),
// and whether it stops once the workspace is allocated (izpi_gpu_prepare, a session's begin).
struct RenderCall {
  SampleRange range;
  uint32_t size_spp;
  bool prepare_only;
};
RenderCall one_shot(const izpi_render_req* req, bool prepare_only = false) {
  const uint32_t spp = req ? req->spp : 0;
  return RenderCall{SampleRange{0, spp, false}, spp, prepare_only};
}

// A progressive session owns the context's running sums, counters and progress: the calls
// that would overwrite them are refused while it is open.
bool session_open(izpi_ctx* ctx) {
  if (!ctx->session.open) return false;
  ctx->err = "a progressive session is open";
  return true;
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
  ap.num_pixels = rs.num_pixels; ap.spp = req->spp; ap.width = req->width; ap.height = req->height;
  ap.tile_w = rs.tw; ap.tile_h = rs.th; ap.out_layout = req->out_layout;
  ap.sampler = rs.preview ? (uint32_t)IZPI_SAMPLER_COLOUR : req->sampler;  // (the preview samplers: col / numSamples, rgb.go:38)
  ap.tiles = ctx->d_tiles; ap.samples = ctx->d_samples; ap.running = ctx->d_running; ap.out = out_dev;
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
  if (!rs.preview) {
    path_shade_params(ctx, req, sc, rs, plan, nbg, sp);
    stage_tables(ctx, req, tu, rs, plan, nbg, sc, sp);
  }

  const RunInput run{num_pixels, plan.chunk, plan.pool_blocks, sr};
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
  s.samples = (uint64_t)num_pixels * sr.end;
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

// Render share r of the frame into ctx->d_share (share_buffers; stats in ctx->last), or
// with prepare_only allocate the workspace that render needs.
int render_share(izpi_ctx* ctx, const izpi_render_req* req, const Shares& sh, uint32_t r, bool prepare_only = false) {
  const std::vector<uint32_t> mine = sh.mine(r);
  memset(&ctx->last, 0, sizeof(ctx->last));
  if (mine.empty()) return IZPI_OK;  // more shares than units: an empty block joins the gather
  izpi_render_req q = request_copy(req);
  q.num_tiles = (uint32_t)(mine.size() / 4);
  q.tiles = mine.data();
  q.out_layout = IZPI_OUT_PACKED;
  q.post = IZPI_POST_NONE;
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

// ------------------------------------------------------- progressive sessions
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

int session_zero_moments(izpi_ctx* ctx) {
  izpi_ctx::Session& ss = ctx->session;
  const size_t bytes = (size_t)ss.num_pixels * 3 * sizeof(double);
  const int rc = grow(ctx, (void**)&ctx->d_moments, &ctx->moments_cap, bytes);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(ctx->d_moments, 0, bytes, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ss.noise = true;
  return IZPI_OK;
}

// begin: render_body's own checks, plan and allocation for a request of step_spp samples
// (its prepare_only form, which for a session also zeroes the sums and the counters).
// With IZPI_PROG_NOISE the samples' second moments start at zero in a buffer of their own
// (24 B per pixel; it only grows, and no workspace plan counts it).
int session_begin(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp, uint32_t flags = 0) {
  if (ctx->session.open) { ctx->err = "a progressive session is already open"; return IZPI_ERR_INVALID; }
  if (!req || step_spp == 0) { ctx->err = "progressive_begin: a request and step_spp >= 1"; return IZPI_ERR_INVALID; }
  if (flags & ~(uint32_t)IZPI_PROG_NOISE) { ctx->err = "progressive_begin: unknown flags"; return IZPI_ERR_INVALID; }
  izpi_ctx::Session& ss = ctx->session;
  int rc = session_copy_request(ss, req, ctx->err);
  if (!rc) {
    ss.step_spp = std::min(step_spp, std::max(1u, ss.req.spp));
    rc = render_body(ctx, &ss.req, RenderCall{SampleRange{0, 0, true}, ss.step_spp, true}, nullptr);
  }
  if (!rc && (flags & IZPI_PROG_NOISE)) rc = session_zero_moments(ctx);
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

int session_usable(izpi_ctx* ctx) {
  if (!ctx->session.open) { ctx->err = "no progressive session is open"; return IZPI_ERR_INVALID; }
  if (ctx->session.broken) { ctx->err = "the session's last step failed: end it"; return IZPI_ERR_INVALID; }
  return IZPI_OK;
}

// step: samples [done, done + n) through render_body's chunk loops, never finalised. The
// device counters run on from step to step; times and launches are summed here.
int session_step(izpi_ctx* ctx, uint32_t spp, izpi_render_stats* stats) {
  int rc = session_usable(ctx);
  if (rc) return rc;
  izpi_ctx::Session& ss = ctx->session;
  const uint32_t n = std::min(spp ? spp : ss.step_spp, ss.req.spp - ss.done);
  if (n) {
    rc = render_body(ctx, &ss.req, RenderCall{SampleRange{ss.done, ss.done + n, true}, ss.step_spp, false}, nullptr);
    if (rc) {  // a chunk may or may not be in the sums
      ss.broken = true;
      return rc;
    }
    ss.done += n;
    izpi_render_stats s = ctx->last;
    s.kernel_ms += ss.cum.kernel_ms; s.shade_ms += ss.cum.shade_ms; s.tail_ms += ss.cum.tail_ms;
    s.total_ms += ss.cum.total_ms; s.alloc_ms += ss.cum.alloc_ms; s.launches += ss.cum.launches;
    ss.cum = s;
    ctx->last = s;
    ctx->prog_done.store((uint64_t)ss.num_pixels * ss.done, std::memory_order_relaxed);
  }
  if (stats) *stats = ss.cum;
  return IZPI_OK;
}

// The session's tiles on the device (izpi_gpu_unpack_tiles may have used d_tiles since the last step).
int session_tiles(izpi_ctx* ctx) {
  const izpi_ctx::Session& ss = ctx->session;
  const int rc = grow(ctx, (void**)&ctx->d_tiles, &ctx->tiles_cap, ss.run_tiles.size() * sizeof(uint32_t));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->d_tiles, ss.run_tiles.data(), ss.run_tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  return IZPI_OK;
}

// The noise estimate needs a session begun with IZPI_PROG_NOISE and two samples (n - 1 divides).
int session_has_noise(izpi_ctx* ctx) {
  if (!ctx->session.noise) { ctx->err = "noise: the session was begun without IZPI_PROG_NOISE"; return IZPI_ERR_INVALID; }
  if (ctx->session.done < 2) { ctx->err = "noise: needs at least 2 samples"; return IZPI_ERR_INVALID; }
  return IZPI_OK;
}
NoiseParams noise_params(izpi_ctx* ctx) {
  const izpi_ctx::Session& ss = ctx->session;
  NoiseParams np{};
  np.num_pixels = ss.num_pixels; np.done = ss.done; np.width = ss.req.width; np.height = ss.req.height;
  np.tile_w = ss.tile_w; np.tile_h = ss.tile_h; np.sampler = ss.req.sampler; np.out_layout = ss.req.out_layout;
  np.threshold = IZPI_NOISE_DEFAULT_THRESHOLD; np.floor = IZPI_NOISE_DEFAULT_FLOOR;
  np.tiles = ctx->d_tiles; np.running = ctx->d_running; np.moments = ctx->d_moments;
  return np;
}

// noise: k_noise_stats over the sums and moments; the block sums are added here, in block order.
int session_noise(izpi_ctx* ctx, const izpi_noise_params* params, izpi_noise_stats* out) {
  int rc = session_usable(ctx);
  if (rc) return rc;
  const izpi_noise_params p = params ? *params : nz::defaults();
  if (const char* bad = nz::check_params(p)) { ctx->err = bad; return IZPI_ERR_INVALID; }
  if ((rc = session_has_noise(ctx))) return rc;
  const izpi_ctx::Session& ss = ctx->session;
  hipStream_t st = ctx->stream;
  if ((rc = session_tiles(ctx))) return rc;
  const size_t blocks = ((size_t)ss.num_pixels + nz::BLOCK - 1) / nz::BLOCK;
  if ((rc = grow(ctx, (void**)&ctx->d_noisepart, &ctx->noisepart_cap, 5 * blocks * sizeof(double)))) return rc;
  NoiseParams np = noise_params(ctx);
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

// converge: step(step_spp), then the statistic once done >= max(2, min_spp), until the frame is
// converged or the cap is reached. `step` and `noise` are the session's own (one context or
// the devices of a group); done() reads its samples.
template <class Step, class Noise, class Done>
int converge_loop(const izpi_noise_params* params, uint32_t cap, Step step, Noise noise, Done done, izpi_noise_stats* out) {
  const izpi_noise_params p = params ? *params : nz::defaults();
  izpi_noise_stats last{};
  int rc = IZPI_OK;
  while (!rc && done() < cap) {
    if ((rc = step())) break;
    if (done() < std::max(2u, p.min_spp)) continue;
    if ((rc = noise(&p, &last))) break;
    if (last.converged) break;
  }
  if (out) *out = last;
  return rc;
}

// snapshot: k_resolve of the sums into device memory, then (IZPI_SNAP_CANVAS) the request's post.
int session_snapshot(izpi_ctx* ctx, uint32_t form, double* out_dev) {
  int rc = session_usable(ctx);
  if (rc) return rc;
  const izpi_ctx::Session& ss = ctx->session;
  if (form != IZPI_SNAP_CANVAS && form != IZPI_SNAP_DISPLAY && form != IZPI_SNAP_NOISE) { ctx->err = "unknown snapshot form"; return IZPI_ERR_INVALID; }
  if (ss.done == 0) { ctx->err = "snapshot before the session's first sample"; return IZPI_ERR_INVALID; }
  if (form == IZPI_SNAP_NOISE && (rc = session_has_noise(ctx))) return rc;
  if (!out_dev) { ctx->err = "null output"; return IZPI_ERR_INVALID; }
  hipStream_t st = ctx->stream;
  if ((rc = session_tiles(ctx))) return rc;
  if (form == IZPI_SNAP_NOISE) {  // k_noise_resolve: the standard errors, where k_resolve writes the pixels; no post
    NoiseParams np = noise_params(ctx);
    np.out = out_dev;
    launch_noise_resolve(st, np);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return IZPI_OK;
  }
  ResolveParams rp{};
  rp.num_pixels = ss.num_pixels; rp.done = ss.done; rp.width = ss.req.width; rp.height = ss.req.height;
  rp.tile_w = ss.tile_w; rp.tile_h = ss.tile_h; rp.sampler = ss.req.sampler; rp.out_layout = ss.req.out_layout;
  rp.form = form; rp.exposure = ss.req.exposure;
  rp.tiles = ctx->d_tiles; rp.running = ctx->d_running; rp.out = out_dev;
  launch_resolve(st, rp);
  HIP_TRY(hipGetLastError());
  if (form == IZPI_SNAP_CANVAS && (rc = apply_post(ctx, &ss.req, out_dev))) return rc;
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

// (true, with the message, when the group's session cannot give a noise estimate)
bool multi_lacks_noise(izpi_multi* m) {
  if (!m->session.noise) { m->err = "noise: the session was begun without IZPI_PROG_NOISE"; return true; }
  if (m->session.done < 2) { m->err = "noise: needs at least 2 samples"; return true; }
  return false;
}

bool multi_session_open(izpi_multi* m) {
  if (!m->prog_open) return false;
  m->err = "a progressive session is open";
  return true;
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
    UP((const char*)nullptr, tl.bytes, &nb);
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
}  // namespace

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
  int rc = grow(ctx, (void**)&ctx->d_out, &ctx->out_cap, bytes);
  if (rc) return rc;
  // start from the caller's buffer so untouched pixels keep their values
  HIP_TRY(hipMemcpyAsync(ctx->d_out, out_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = render_impl(ctx, req, one_shot(req), ctx->d_out);
  if (stats) *stats = ctx->last;
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out_host, ctx->d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return IZPI_OK;
}

int izpi_gpu_prepare(izpi_ctx* ctx, const izpi_render_req* req) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (!req) { ctx->err = "null argument"; return IZPI_ERR_INVALID; }
  if (session_open(ctx)) return IZPI_ERR_INVALID;
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->comm && ctx->comm_size > 1) {  // izpi_gpu_render_rank's share of the frame on this rank
    Shares sh;
    int rc = make_shares(ctx, req, ctx->comm_size, sh);
    if (!rc) rc = share_buffers(ctx, sh, ctx->comm_rank == 0);
    return rc ? rc : render_share(ctx, req, sh, ctx->comm_rank, true);
  }
  return render_impl(ctx, req, one_shot(req, true), nullptr);
}

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

int izpi_gpu_progressive_converge(izpi_ctx* ctx, const izpi_noise_params* p, izpi_render_stats* stats, izpi_noise_stats* noise) {
  if (!ctx) return IZPI_ERR_INVALID;
  int rc = session_usable(ctx);
  if (rc) return rc;
  const izpi_noise_params q = p ? *p : nz::defaults();
  if (const char* bad = nz::check_params(q)) { ctx->err = bad; return IZPI_ERR_INVALID; }
  if (!ctx->session.noise) { ctx->err = "noise: the session was begun without IZPI_PROG_NOISE"; return IZPI_ERR_INVALID; }
  HIP_TRY(hipSetDevice(ctx->device));
  rc = converge_loop(&q, ctx->session.req.spp, [&]() { return session_step(ctx, 0, nullptr); },
                     [&](const izpi_noise_params* np, izpi_noise_stats* ns) { return session_noise(ctx, np, ns); },
                     [&]() { return ctx->session.done; }, noise);
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
  if ((rc = grow(ctx, (void**)&ctx->d_out, &ctx->out_cap, bytes))) return rc;
  // start from the caller's buffer so untouched pixels keep their values, as izpi_gpu_render
  HIP_TRY(hipMemcpyAsync(ctx->d_out, out_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = session_snapshot(ctx, form, ctx->d_out))) return rc;
  HIP_TRY(hipMemcpyAsync(out_host, ctx->d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return IZPI_OK;
}

int izpi_gpu_progressive_end(izpi_ctx* ctx) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (!ctx->session.open) { ctx->err = "no progressive session is open"; return IZPI_ERR_INVALID; }
  session_drop(ctx);
  return IZPI_OK;
}

int izpi_gpu_spectral_post(izpi_ctx* ctx, const double* xyz_dev, double* rgba_dev, uint32_t width, uint32_t height,
                           double exposure) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (!xyz_dev || !rgba_dev || xyz_dev == rgba_dev || width == 0 || height == 0) {
    ctx->err = "spectral_post: bad arguments (buffers must be distinct device canvases)";
    return IZPI_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  dim3 g((width + 15) / 16, (height + 15) / 16);
  hipLaunchKernelGGL(k_spectral_post, g, dim3(256), 0, ctx->stream, xyz_dev, rgba_dev, width, height, exposure);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return IZPI_OK;
}

int izpi_gpu_build_bvh4(izpi_ctx* ctx, const double* boxes, uint32_t n, uint32_t leaf_max, uint32_t method,
                        izpi_bvh4_node* nodes, uint32_t max_nodes, uint32_t* num_nodes, uint32_t* order, double* build_ms) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (num_nodes) *num_nodes = 0;
  if ((n && (!boxes || !nodes || !order)) || !num_nodes || (uint64_t)max_nodes < 2ull * n) {
    ctx->err = "build_bvh4: bad arguments (nodes needs 2n entries)";
    return IZPI_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  std::vector<izpi_bvh4_node> out;
  std::vector<uint32_t> ord;
  float ms = 0;
  const int rc = izpi_bvh::build(ctx->stream, boxes, n, leaf_max, method, out, ord, &ms, ctx->err);
  if (rc) return rc;
  if (!out.empty()) memcpy(nodes, out.data(), out.size() * sizeof(izpi_bvh4_node));
  if (!ord.empty()) memcpy(order, ord.data(), ord.size() * sizeof(uint32_t));
  *num_nodes = (uint32_t)out.size();
  if (build_ms) *build_ms = ms;
  return IZPI_OK;
}

}  // extern "C"
namespace izpi_displace {  // displace.hip
int run(hipStream_t st, const izpi_tri_in* tris, uint64_t n, const double* rgba, uint32_t width, uint32_t height,
        double dmin, double dmax, uint32_t order, izpi_tri_in* out, uint64_t cap, uint64_t* n_out, uint64_t* counts,
        double* ms, std::string& err);
const char* check(const izpi_tri_in* tris, uint64_t n, const double* rgba, uint32_t width, uint32_t height,
                  uint32_t order, const uint64_t* n_out);
}
extern "C" {

int izpi_gpu_displace(izpi_ctx* ctx, const izpi_tri_in* tris, uint64_t n, const double* rgba, uint32_t width,
                      uint32_t height, double dmin, double dmax, uint32_t order, izpi_tri_in* out, uint64_t cap,
                      uint64_t* n_out, uint64_t* counts, double* ms) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (n_out) *n_out = 0;
  if (const char* bad = izpi_displace::check(tris, n, rgba, width, height, order, n_out)) {
    ctx->err = bad;
    return IZPI_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  return izpi_displace::run(ctx->stream, tris, n, rgba, width, height, dmin, dmax, order, out, cap, n_out, counts, ms,
                            ctx->err);
}

int izpi_gpu_postprocess(izpi_ctx* ctx, double* canvas_dev, uint32_t width, uint32_t height, const uint32_t* filters,
                         const double* params, uint32_t num_filters) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (!canvas_dev || num_filters > IZPI_MAX_FILTERS || (num_filters && (!filters || !params))) {
    ctx->err = "postprocess: bad arguments";
    return IZPI_ERR_INVALID;
  }
  PostFilters pf;
  memset(&pf, 0, sizeof pf);
  pf.n = num_filters;
  for (uint32_t i = 0; i < num_filters; i++) {
    if (filters[i] != IZPI_FILTER_GAMMA && filters[i] != IZPI_FILTER_CLAMP) {
      ctx->err = "postprocess: unknown filter (colour grading needs a .cube LUT reader, not on this path)";
      return IZPI_ERR_UNSUPPORTED;
    }
    pf.kind[i] = filters[i];
    pf.param[i] = params[i];
  }
  const uint64_t np = (uint64_t)width * height;
  if (np == 0 || num_filters == 0) return IZPI_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_postprocess, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, canvas_dev, np, pf);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return IZPI_OK;
}

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

int izpi_gpu_trace(izpi_ctx* ctx, const double* rays, uint32_t n, izpi_hit* out) {
  if (!ctx || !rays || !out) return IZPI_ERR_INVALID;
  if (!ctx->have_scene) { ctx->err = "no scene"; return IZPI_ERR_NO_SCENE; }
  if (session_open(ctx)) return IZPI_ERR_INVALID;  // (it zeroes the counters a session keeps)
  if (n == 0) return IZPI_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  DevBufs tmp;  // freed on every return
  double* dr; izpi_hit* dh; RayOD* rr; uint32_t* kk; double2* tm; double2* hh;
  HIP_TRY(tmp.alloc(&dr, (size_t)n * 8));
  HIP_TRY(tmp.alloc(&dh, n));
  HIP_TRY(tmp.alloc(&rr, n));
  HIP_TRY(tmp.alloc(&kk, n));
  HIP_TRY(tmp.alloc(&tm, n));
  HIP_TRY(tmp.alloc(&hh, 2 * (size_t)n));  // (t, prim) and (u, v) interleaved
  HIP_TRY(hipMemcpy(dr, rays, (size_t)n * 8 * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(ctx->d_misc, 0, 8 * MISC_STRIDE * sizeof(uint32_t), ctx->stream));
  HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, CNT_N * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_trace_setup, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, dr, n, rr, kk, tm, misc(ctx, 3));
  WaveParams wp{};
  wp.in.ray = rr; wp.in.kind = kk; wp.in.tminmax = tm; wp.in.hit = hh; wp.in.huv = hh + 1; wp.in.hs = 2;
  wp.in_count = misc(ctx, 3); wp.trace_next = misc(ctx, 2); wp.slots = n; wp.read_kind = 1; wp.hit_uv = 1;
  Tracer tr;
  int rc = make_tracer(ctx, kDefaultTuning, true, &tr);
  if (rc) return rc;
  if ((rc = grow(ctx, (void**)&ctx->d_spill, &ctx->spill_cap, tr.spill_bytes))) return rc;
  launch_trace(ctx, ctx->sc, tr, wp, ctx->stream, ctx->d_spill);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_trace_records, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->sc, rr, hh, n, dh);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(out, dh, (size_t)n * sizeof(izpi_hit), hipMemcpyDeviceToHost));
  return IZPI_OK;
}

int izpi_gpu_ray_aabb4(izpi_ctx* ctx, const float* boxes, const float* rays, uint32_t n, uint8_t* masks) {
  if (!ctx || !boxes || !rays || !masks) return IZPI_ERR_INVALID;
  if (n == 0) return IZPI_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  DevBufs tmp;  // freed on every return
  float *db, *dr; uint8_t* dm;
  HIP_TRY(tmp.alloc(&db, (size_t)n * 24));
  HIP_TRY(tmp.alloc(&dr, (size_t)n * 7));
  HIP_TRY(tmp.alloc(&dm, n));
  HIP_TRY(hipMemcpy(db, boxes, (size_t)n * 24 * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dr, rays, (size_t)n * 7 * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_aabb4, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, db, dr, n, dm);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(masks, dm, n, hipMemcpyDeviceToHost));
  return IZPI_OK;
}

int izpi_gpu_gomath(izpi_ctx* ctx, int op, const double* x, const double* y, uint32_t n, double* out) {
  if (!ctx || !x || !out) return IZPI_ERR_INVALID;
  if (n == 0) return IZPI_OK;
  if (op == 37) {  // texture lookups: a scene, and texture numbers in range
    if (!ctx->have_scene) { ctx->err = "texture lookup before izpi_gpu_upload_scene"; return IZPI_ERR_NO_SCENE; }
    if (!y) { ctx->err = "texture lookup without texture numbers"; return IZPI_ERR_INVALID; }
    for (uint32_t i = 0; i < n; i++)
      if (!(y[i] >= 0 && y[i] < (double)ctx->num_textures)) { ctx->err = "texture number out of range"; return IZPI_ERR_INVALID; }
  }
  if (op == 14 && !y) { ctx->err = "path length without exit points"; return IZPI_ERR_INVALID; }
  const size_t nin = op == 14 ? 3 * (size_t)n : n;  // op 14 reads 3-vectors
  HIP_TRY(hipSetDevice(ctx->device));
  DevBufs tmp;  // freed on every return
  double *dx, *dy = nullptr, *dout;
  HIP_TRY(tmp.alloc(&dx, nin));
  HIP_TRY(tmp.alloc(&dout, n));
  HIP_TRY(hipMemcpy(dx, x, nin * sizeof(double), hipMemcpyHostToDevice));
  if (y) {
    HIP_TRY(tmp.alloc(&dy, nin));
    HIP_TRY(hipMemcpy(dy, y, nin * sizeof(double), hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(k_gomath, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->sc, op, dx, dy, n, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(out, dout, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
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
  if (!m || m->ctx.empty()) return IZPI_ERR_INVALID;
  if (multi_session_open(m)) return IZPI_ERR_INVALID;
  izpi_ctx* root = m->ctx[0];
  Shares sh;
  int rc = multi_shares(m, req, sh);
  if (rc) return rc;
  if (req->post != IZPI_POST_NONE && req->num_tiles != 0) {
    m->err = "post-processing needs a whole-frame request";
    return IZPI_ERR_INVALID;
  }
  const size_t canvas_bytes = (size_t)req->width * req->height * 4 * sizeof(double);
  // the caller's canvas is the starting point (pixels of no tile keep their values)
  if (out_host) {
    if (hipMemcpy(root->d_out, out_host, canvas_bytes, hipMemcpyHostToDevice) != hipSuccess) { m->err = "hipMemcpy"; return IZPI_ERR_HIP; }
  } else if (hipMemset(root->d_out, 0, canvas_bytes) != hipSuccess) {
    m->err = "hipMemset";
    return IZPI_ERR_HIP;
  }
  // every device renders its share, then copies it into block i of the root's gather
  // buffer (peer copy over xGMI; a plain device copy for the root)
  rc = on_every_device(m, [&](uint32_t i, izpi_ctx* c) {
    int r = share_buffers(c, sh, false);
    if (!r) r = render_share(c, req, sh, i);
    if (r) return r;
    hipError_t e = hipMemcpyPeerAsync(root->d_gather + (size_t)i * sh.block, root->device, c->d_share, c->device,
                                      sh.block * sizeof(double), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("gather copy: ") + hipGetErrorString(e); return (int)IZPI_ERR_HIP; }
    return (int)IZPI_OK;
  });
  for (size_t i = 0; stats && i < m->ctx.size(); i++) stats[i] = m->ctx[i]->last;
  if (rc) return rc;
  if (hipSetDevice(root->device) != hipSuccess) { m->err = "hipSetDevice"; return IZPI_ERR_HIP; }
  if ((rc = assemble(root, req, sh, root->d_out))) { m->err = root->err; return rc; }
  if (out_host && hipMemcpy(out_host, root->d_out, canvas_bytes, hipMemcpyDeviceToHost) != hipSuccess) {
    m->err = "hipMemcpy";
    return IZPI_ERR_HIP;
  }
  return IZPI_OK;
}

int izpi_gpu_multi_prepare(izpi_multi* m, const izpi_render_req* req) {
  if (!m || m->ctx.empty()) return IZPI_ERR_INVALID;
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
  if (!m || m->ctx.empty()) return IZPI_ERR_INVALID;
  if (m->prog_open) { m->err = "a progressive session is already open"; return IZPI_ERR_INVALID; }
  if (!req || step_spp == 0) { m->err = "progressive_begin: a request and step_spp >= 1"; return IZPI_ERR_INVALID; }
  if (flags & ~(uint32_t)IZPI_PROG_NOISE) { m->err = "progressive_begin: unknown flags"; return IZPI_ERR_INVALID; }
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
    izpi_render_req q = ms.req;
    q.num_tiles = (uint32_t)(mine.size() / 4);
    q.tiles = mine.data();
    q.out_layout = IZPI_OUT_PACKED;
    q.post = IZPI_POST_NONE;
    return session_begin(c, &q, ms.step_spp, flags);
  });
  if (rc) {
    for (izpi_ctx* c : m->ctx) session_drop(c);
    return rc;
  }
  ms.noise = (flags & IZPI_PROG_NOISE) != 0;
  m->shares = sh;
  m->prog_open = true;
  return IZPI_OK;
}

int izpi_gpu_multi_progressive_step(izpi_multi* m, uint32_t spp, izpi_render_stats* stats) {
  if (!m || m->ctx.empty()) return IZPI_ERR_INVALID;
  if (!m->prog_open) { m->err = "no progressive session is open"; return IZPI_ERR_INVALID; }
  izpi_ctx::Session& ms = m->session;
  const uint32_t n = std::min(spp ? spp : ms.step_spp, ms.req.spp - ms.done);
  int rc = IZPI_OK;
  if (n) rc = on_every_device(m, [&](uint32_t, izpi_ctx* c) { return c->session.open ? session_step(c, n, nullptr) : (int)IZPI_OK; });
  for (size_t i = 0; stats && i < m->ctx.size(); i++) stats[i] = m->ctx[i]->session.cum;
  if (rc) return rc;
  ms.done += n;
  return IZPI_OK;
}

int izpi_gpu_multi_progressive_snapshot(izpi_multi* m, uint32_t form, double* out_host) {
  if (!m || m->ctx.empty()) return IZPI_ERR_INVALID;
  if (!m->prog_open) { m->err = "no progressive session is open"; return IZPI_ERR_INVALID; }
  const izpi_ctx::Session& ms = m->session;
  if (form != IZPI_SNAP_CANVAS && form != IZPI_SNAP_DISPLAY && form != IZPI_SNAP_NOISE) { m->err = "unknown snapshot form"; return IZPI_ERR_INVALID; }
  if (ms.done == 0) { m->err = "snapshot before the session's first sample"; return IZPI_ERR_INVALID; }
  if (form == IZPI_SNAP_NOISE && multi_lacks_noise(m)) return IZPI_ERR_INVALID;
  izpi_ctx* root = m->ctx[0];
  const Shares& sh = m->shares;
  const size_t canvas_bytes = (size_t)ms.req.width * ms.req.height * 4 * sizeof(double);
  if (hipSetDevice(root->device) != hipSuccess) { m->err = "hipSetDevice"; return IZPI_ERR_HIP; }
  // the caller's canvas is the starting point, as in izpi_gpu_multi_render
  if (out_host) {
    if (hipMemcpy(root->d_out, out_host, canvas_bytes, hipMemcpyHostToDevice) != hipSuccess) { m->err = "hipMemcpy"; return IZPI_ERR_HIP; }
  } else if (hipMemset(root->d_out, 0, canvas_bytes) != hipSuccess) {
    m->err = "hipMemset";
    return IZPI_ERR_HIP;
  }
  // every device resolves its sums into its packed share, then copies it into its block of
  // the root's gather buffer
  int rc = on_every_device(m, [&](uint32_t i, izpi_ctx* c) {
    if (!c->session.open) return (int)IZPI_OK;
    const int r = session_snapshot(c, form, c->d_share);
    if (r) return r;
    hipError_t e = hipMemcpyPeerAsync(root->d_gather + (size_t)i * sh.block, root->device, c->d_share, c->device,
                                      sh.block * sizeof(double), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("gather copy: ") + hipGetErrorString(e); return (int)IZPI_ERR_HIP; }
    return (int)IZPI_OK;
  });
  if (rc) return rc;
  if (hipSetDevice(root->device) != hipSuccess) { m->err = "hipSetDevice"; return IZPI_ERR_HIP; }
  izpi_render_req q = ms.req;
  if (form != IZPI_SNAP_CANVAS) q.post = IZPI_POST_NONE;  // the display pixels and the standard errors are not post-processed
  if ((rc = assemble(root, &q, sh, root->d_out))) { m->err = root->err; return rc; }
  if (out_host && hipMemcpy(out_host, root->d_out, canvas_bytes, hipMemcpyDeviceToHost) != hipSuccess) {
    m->err = "hipMemcpy";
    return IZPI_ERR_HIP;
  }
  return IZPI_OK;
}

// The devices' statistics in one: the integers added, the largest maximum, sum_error added in
// device order (its last bits depend on the share plan), the slowest device's time.
int izpi_gpu_multi_progressive_noise(izpi_multi* m, const izpi_noise_params* p, izpi_noise_stats* out) {
  if (!m || m->ctx.empty()) return IZPI_ERR_INVALID;
  if (!m->prog_open) { m->err = "no progressive session is open"; return IZPI_ERR_INVALID; }
  const izpi_noise_params q = p ? *p : nz::defaults();
  if (const char* bad = nz::check_params(q)) { m->err = bad; return IZPI_ERR_INVALID; }
  if (multi_lacks_noise(m)) return IZPI_ERR_INVALID;
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

int izpi_gpu_multi_progressive_converge(izpi_multi* m, const izpi_noise_params* p, izpi_render_stats* stats, izpi_noise_stats* noise) {
  if (!m || m->ctx.empty()) return IZPI_ERR_INVALID;
  if (!m->prog_open) { m->err = "no progressive session is open"; return IZPI_ERR_INVALID; }
  const izpi_noise_params q = p ? *p : nz::defaults();
  if (const char* bad = nz::check_params(q)) { m->err = bad; return IZPI_ERR_INVALID; }
  if (!m->session.noise) { m->err = "noise: the session was begun without IZPI_PROG_NOISE"; return IZPI_ERR_INVALID; }
  return converge_loop(&q, m->session.req.spp, [&]() { return izpi_gpu_multi_progressive_step(m, 0, stats); },
                       [&](const izpi_noise_params* np, izpi_noise_stats* ns) { return izpi_gpu_multi_progressive_noise(m, np, ns); },
                       [&]() { return m->session.done; }, noise);
}

int izpi_gpu_multi_progressive_end(izpi_multi* m) {
  if (!m) return IZPI_ERR_INVALID;
  if (!m->prog_open) { m->err = "no progressive session is open"; return IZPI_ERR_INVALID; }
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
    for (uint32_t p = 0; p < nt * tw * th; p++) {
      uint32_t x, row;
      if (packed_target(mine.data(), p, tw, th, height, &x, &row))
        memcpy(canvas + ((size_t)row * width + x) * 4, packed + (size_t)p * 4, 4 * sizeof(double));
    }
  }
  return IZPI_OK;
}

int izpi_gpu_progress(izpi_ctx* ctx, uint64_t* samples_done, uint64_t* samples_total) {
  if (!ctx || !samples_done || !samples_total) return IZPI_ERR_INVALID;
  // total first: a render starting between the two loads shows 0 of its own total at worst
  *samples_total = ctx->prog_total.load(std::memory_order_relaxed);
  *samples_done = std::min(ctx->prog_done.load(std::memory_order_relaxed), *samples_total);
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

