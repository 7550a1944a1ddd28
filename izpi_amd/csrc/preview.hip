// preview.hip — the Normal, Albedo and WireFrame samplers (sampler/normal.go:28-34,
// albedo.go:30-36, wireframe.go:34-40) under render/rgb.go:27-41's pixel loop: k_preview_start,
// k_preview and the batch loop that drives them with k_trace2 (run_preview, izpi_runtime.h). A
// translation unit of its own, so the four shade_*.hip units compile what they compiled before.
#include "izpi_runtime.h"

namespace {

// What k_preview does with a traced batch.
enum { PV_NORMAL = 0, PV_ALBEDO = 1, PV_WIRE_FIRST = 2, PV_WIRE_EDGE = 3 };

// The camera rays of units [base, base + n) into entries [0, n) (entry j IS unit base + j: no
// path state is stored). start_path's arithmetic and streams: a preview frame looks through
// the primary rays of a Colour frame of the same seed.
__global__ void __launch_bounds__(256) k_preview_start(const DevScene sc, const ShadeParams sp, const WaveBuf out,
                                                       uint32_t base, uint32_t n, uint32_t* count, uint32_t* cursor) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0) { *count = n; *cursor = 0; }  // k_trace2's queue length and dequeue cursor
  if (j >= n) return;
  PathSt P;
  RayRec R;
  // (sp.max_depth is 1: the preview samplers ignore the request's, and a camera ray always starts)
  if (start_path<IZPI_SAMPLER_COLOUR, true>(sc, sp, base + j, P, R)) store_camera_entry(out, j, R);
  else dead_entry(out, j);
}

// segment.Belongs (segment/segment.go:13-30)
IZPI_DEV bool segment_belongs(V3 a, V3 b, V3 c) {
  const V3 ab = sub(b, a), ac = sub(c, a);
  if (length(cross(unit(ab), unit(ac))) >= .005) return false;
  const double kac = dot(ab, ac), kab = dot(ab, ab);
  if (kac < 0 || kac > kab) return false;
  return true;
}

// Entry j of the traced batch (unit base + j): the sampler's value of its hit into the
// per-sample results (DeNAN as rgb.go:36), or, PV_WIRE_FIRST, the entry's second traversal.
template <int MODE>
__global__ void __launch_bounds__(256) k_preview(const DevScene sc, const ShadeParams sp, const PreviewParams pp,
                                                 uint32_t base, uint32_t n, uint32_t* cursor) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0) *cursor = 0;  // (PV_WIRE_FIRST: the second traversal dequeues from 0 again)
  if (j >= n) return;
  const WaveBuf& b = pp.buf;
  if (MODE == PV_WIRE_EDGE && (sld(b.kind + j) & RAY_DEAD)) return;  // first-pass miss: paper, written then
  const double2 hit = sld(b.hit + (size_t)j * b.hs);
  HitOut c;
  c.t = hit.x; c.prim = hit_prim(hit); c.u = 0; c.v = 0; c.pad = 0;
  const V3 paper = mk(sp.background[0], sp.background[1], sp.background[2]);
  V3 col = mk(0.0, 0.0, 0.0);
  if (MODE == PV_WIRE_FIRST) {
    if (c.prim >= 0) {
      // HitableSlice.HitEdge: obj.HitEdge(r, tMin, closestSoFar + epsilon), epsilon =
      // Nextafter(1, 2) - 1 (hitable_slice.go:54,66); not a Sampler call (RAY_PATHLEN)
      sst(pp.tminmax + j, make_double2(0.001, c.t + 2.220446049250313e-16));
      sst(b.kind + j, (uint32_t)RAY_PATHLEN);
      return;
    }
    dead_entry(b, j);
    col = paper;
  } else if (c.prim >= 0) {
    const RayOD r = sld(b.ray + j);
    const V3 o = mk(r.o[0], r.o[1], r.o[2]), d = mk(r.d[0], r.d[1], r.d[2]);
    const double time = b.time ? sld(b.time + j) : 0.0;
    const GShade gs = sc.shade[c.prim];
    if (MODE == PV_WIRE_EDGE) {
      const V3 p = add(o, smul(d, c.t));  // rec.P()
      const GPrim& pr = sc.prims[c.prim];
      bool edge = false;
      if (IZPI_PRIM_KIND(gs.ref) == IZPI_PRIM_TRIANGLE) {  // Triangle.HitEdge (triangle.go:282-302)
        const V3 v0 = ld3(pr.a), v1 = ld3(pp.verts[c.prim].v1), v2 = ld3(pp.verts[c.prim].v2);
        edge = segment_belongs(v0, v1, p) || segment_belongs(v1, v2, p) || segment_belongs(v2, v0, p);
      } else {  // Sphere.HitEdge (sphere.go:97-113); math.Acos(x) = Pi/2 - Asin(x)
        double pa[9];
        for (int k = 0; k < 9; k++) pa[k] = pr.a[k];
        const V3 a = sub(p, o), bb = sub(p, sph_center(pa, time));
        const double theta = 1.5707963267948966 - gm::asin(dot(a, bb) / (length(a) * length(bb)));
        edge = gm::abs(theta) <= 1.6707963267948966;  // math.Pi/2.0 + 0.1
      }
      col = edge ? mk(pp.ink[0], pp.ink[1], pp.ink[2]) : paper;
    } else {
      HitRec h;
      hit_record(sc, c, b.huv ? b.huv + (size_t)j * b.hs : nullptr, gs, o, d, time, (gs_cflags(gs) & 2u) != 0, h);
      if (MODE == PV_NORMAL) {
        col = h.n;  // rec.Normal(), raw
      } else {  // Material.Albedo(rec.U(), rec.V(), rec.P())
        const uint32_t kind = gs_kind(gs);
        if (kind == IZPI_MAT_DIELECTRIC) {
          col = mk(1.0, 1.0, 1.0);
        } else if (kind == IZPI_MAT_METAL) {
          col = ld3(sc.materials[h.mat].rgb);
        } else {  // Lambertian, PBR, Isotropic: albedo.Value; DiffuseLight: emit.Value
          col = tex_rgb(sc, sc.materials[h.mat].albedo_tex, h.u, h.v);
        }
      }
    }
  } else if (MODE == PV_WIRE_EDGE) {
    col = paper;  // the second traversal lost the hit (a sphere at t + epsilon == t)
  }
  col = denan(col);
  double* out = sample_out(sp, base + j);
  sst(out, col.x); sst(out + 1, col.y); sst(out + 2, col.z);
}

template <int MODE>
void launch_preview(hipStream_t st, const DevScene& sc, const ShadeParams& sp, const PreviewParams& pp, uint32_t base,
                    uint32_t n, uint32_t* cursor) {
  hipLaunchKernelGGL(k_preview<MODE>, dim3((n + 255) / 256), dim3(256), 0, st, sc, sp, pp, base, n, cursor);
}

}  // namespace

int run_preview(izpi_ctx* ctx, const izpi_render_req* req, const DevScene& sc, const Tracer& tr, ShadeParams& sp,
                const PreviewParams& pp, AccumParams& ap, const RunInput& in, RunTimes* out) {
  hipStream_t st = ctx->stream;
  const uint32_t num_pixels = in.num_pixels, chunk = in.chunk;
  const SampleRange& sr = in.range;
  if ((uint32_t)tr.blocks * 4 > ctx->num_cus * CPART_BLOCKS_PER_CU * 4) {
    ctx->err = "grid larger than the counter rows";
    return IZPI_ERR_INVALID;
  }
  const bool wire = req->sampler == IZPI_SAMPLER_WIREFRAME;
  uint32_t* count = misc(ctx, 3);
  uint32_t* cursor = misc(ctx, 2);
  WaveParams wp{};
  wp.in = pp.buf;
  wp.in_count = count; wp.trace_next = cursor; wp.slots = pp.slots;
  wp.hit_uv = pp.buf.huv ? 1u : 0u;
  wp.cpart = ctx->d_cpart;
  for (uint32_t s0 = sr.begin; s0 < sr.end; s0 += chunk) {
    const uint32_t cs = std::min(chunk, sr.end - s0);
    sp.chunk_spp = cs; sp.s0 = s0; sp.total_units = num_pixels * cs;
    for (uint32_t base = 0; base < sp.total_units; base += pp.slots) {
      const uint32_t n = std::min(pp.slots, sp.total_units - base);
      hipLaunchKernelGGL(k_preview_start, dim3((n + 255) / 256), dim3(256), 0, st, sc, sp, pp.buf, base, n, count, cursor);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(ctx->evb[0], st));
      wp.in.tminmax = nullptr; wp.read_kind = 0;  // camera rays: RAY_MAIN, 0.001 .. MaxFloat64
      launch_trace(ctx, sc, tr, wp, st, ctx->d_spill);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(ctx->evb[1], st));
      if (req->sampler == IZPI_SAMPLER_NORMAL) launch_preview<PV_NORMAL>(st, sc, sp, pp, base, n, cursor);
      else if (req->sampler == IZPI_SAMPLER_ALBEDO) launch_preview<PV_ALBEDO>(st, sc, sp, pp, base, n, cursor);
      else launch_preview<PV_WIRE_FIRST>(st, sc, sp, pp, base, n, cursor);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(ctx->evb[2], st));
      if (wire) {  // the second traversal, each entry up to its own tMax
        wp.in.tminmax = pp.tminmax; wp.read_kind = 1;
        launch_trace(ctx, sc, tr, wp, st, ctx->d_spill);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ctx->evb[3], st));
        launch_preview<PV_WIRE_EDGE>(st, sc, sp, pp, base, n, cursor);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ctx->evb[4], st));
      }
      HIP_TRY(hipStreamSynchronize(st));
      for (int k = 0; k < (wire ? 4 : 2); k++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->evb[k], ctx->evb[k + 1]));
        ((k & 1) ? out->shade_ms : out->trace_ms) += ms;
      }
      out->launches += wire ? 2u : 1u;
      ctx->prog_done.store((uint64_t)s0 * num_pixels + base + n, std::memory_order_relaxed);
    }
    ap.chunk_spp = cs;
    ap.raw_spectral = 0;
    ap.last = (!sr.keep && s0 + cs >= sr.end) ? 1u : 0u;
    launch_accumulate(st, ap, session_moments(ctx, sr));
    HIP_TRY(hipGetLastError());
  }
  return IZPI_OK;
}

int prepare_preview(izpi_ctx* ctx) {
  int blocks = 0, rc;
  if ((rc = resident_blocks(ctx, k_preview_start, &blocks))) return rc;
  if ((rc = resident_blocks(ctx, k_preview<PV_NORMAL>, &blocks))) return rc;
  if ((rc = resident_blocks(ctx, k_preview<PV_ALBEDO>, &blocks))) return rc;
  if ((rc = resident_blocks(ctx, k_preview<PV_WIRE_FIRST>, &blocks))) return rc;
  if ((rc = resident_blocks(ctx, k_preview<PV_WIRE_EDGE>, &blocks))) return rc;
  return prepare_accumulate(ctx);
}
