// components.hip — the entries around the render call: Render's post-processing (its kernels and
// apply_post), the component kernels the tests call (izpi_gpu_trace, izpi_gpu_ray_aabb4,
// izpi_gpu_gomath), and the ABI entries of the BVH builder and the DISPLACE operator.
#include "izpi_runtime.h"

using namespace izpi_internal;

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

// k_trace2's global-memory box test on n (node, ray) pairs, a lane each, in whole waves: the
// near-index rule, the planes selected by it and slab4_sorted for a wave of fast rays, the twin on
// those same planes for a wave that holds any other ray (as the node step chooses).
__global__ void k_debug_slab4(const float* boxes, const float* rays, uint32_t n, uint8_t* masks) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t j = i < n ? i : n - 1;  // (n > 0; the lanes past n repeat the last pair)
  const float* b = boxes + (size_t)j * 24;
  const float* r = rays + (size_t)j * 7;
  const float ox = r[0], oy = r[1], oz = r[2], ix = r[3], iy = r[4], iz = r[5], tm = r[6];
  // (the upload facts nan_free_bounds and ordered_bounds, here of the pair's own box)
  bool box_ok = true;
  for (int k = 0; k < 4; k++) box_ok = box_ok && b[k] <= b[12 + k] && b[4 + k] <= b[16 + k] && b[8 + k] <= b[20 + k];
  const bool fast = box_ok && ray_fast_ok(ox, oy, oz, ix, iy, iz);
  const uint32_t nx = slab_near_index(0, ix, fast), ny = slab_near_index(1, iy, fast), nz = slab_near_index(2, iz, fast);
  auto plane = [&](uint32_t k) { return make_float4(b[4 * k], b[4 * k + 1], b[4 * k + 2], b[4 * k + 3]); };
  const float4 p0 = plane(nx), p1 = plane(ny), p2 = plane(nz);
  const float4 p3 = plane(slab_far_index(0, nx)), p4 = plane(slab_far_index(1, ny)), p5 = plane(slab_far_index(2, nz));
  uint64_t hit[4];
  if (__builtin_amdgcn_ballot_w64(!fast) == 0) {
    slab4_sorted(p0, p1, p2, p3, p4, p5, ox, oy, oz, ix, iy, iz, tm, hit);
  } else {
    const float a0[4] = {p0.x, p0.y, p0.z, p0.w}, a1[4] = {p1.x, p1.y, p1.z, p1.w}, a2[4] = {p2.x, p2.y, p2.z, p2.w},
                a3[4] = {p3.x, p3.y, p3.z, p3.w}, a4[4] = {p4.x, p4.y, p4.z, p4.w}, a5[4] = {p5.x, p5.y, p5.z, p5.w};
#pragma unroll
    for (int k = 0; k < 4; k++)
      hit[k] = __builtin_amdgcn_ballot_w64(slab(a0[k], a1[k], a2[k], a3[k], a4[k], a5[k], ox, oy, oz, ix, iy, iz, tm));
  }
  const uint32_t lane = threadIdx.x & 63;
  uint8_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) m |= (uint8_t)(((hit[k] >> lane) & 1u) << k);
  if (i < n) masks[i] = m;
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

namespace izpi_internal {
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
}  // namespace izpi_internal

extern "C" {

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

int izpi_gpu_debug_slab4(izpi_ctx* ctx, const float* boxes, const float* rays, uint32_t n, uint8_t* masks) {
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
  hipLaunchKernelGGL(k_debug_slab4, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, db, dr, n, dm);
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

}  // extern "C"
