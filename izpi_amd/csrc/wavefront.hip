// wavefront.hip — the host side of the wavefront scheme, once for every shading instance: which
// instance a scene runs (shade_instance), the pass loop that drives its kernels with k_trace2
// (run_wavefront) and the code-load step ahead of the first frame (prepare_wavefront), all over
// a table of kernel pointers (ShadeKernels, filled by the shade_*.hip units); and the small
// kernels of the loop that depend on no instance: the forward refill's plans, the overflow
// pool's rings, the ordered per-pixel sums (k_accumulate, which the preview samplers share).
#include "izpi_runtime.h"
#include "noise.h"

#include <type_traits>

// Forward mode's refill (k_shade<..., FWD = true>): after a shading pass, the entries its
// finished paths freed take the next units, as one run of camera rays appended behind the
// continuing paths. k_refill_plan (one thread) reads the pass's continuing entries and the
// unit head and hands out min(free entries, units left); k_refill (shade.h) starts unit
// head + j in entry continuing + j (a start whose sample completes without a ray, spectral
// pdf 0, leaves a dead entry, which the next pass drops). Starting the paths in k_shade, in
// the lanes whose path had finished, ran the start's code on a few lanes of each wave: 1-7%
// slower frames (C3 238.3 vs 236.1 ms, C4 at 256 spp 138.4 vs 131.1 ms, C5 at 256 spp
// 4507 vs 4180 ms; profiles/r6l).
// The new entries start on a multiple of REFILL_ALIGN entries, the gap before them dead:
// an unaligned start split a line of every state array between two k_refill blocks at each
// 256-entry boundary (C3 235.4 -> 233.3 ms per frame aligned, the same at 16 or 64;
// `profiles/r6t/`). Starting 4 or 8 units per thread and iteration with their tile loads
// issued together measured the same as one (`profiles/r6s/`).
constexpr uint32_t REFILL_ALIGN = 64;
// Forward mode's first fill of a chunk: entry j takes unit j, a camera entry (k_refill)
static __global__ void k_plan_first(uint32_t* out_count, uint32_t* plan, uint32_t fill) {
  plan[0] = 0; plan[1] = 0; plan[2] = fill; plan[3] = 0;
  *out_count = fill;
}
static __global__ void k_refill_plan(const ShadeParams sp, uint32_t* out_count, uint32_t* plan) {
  const uint32_t nc = *out_count, h = *sp.head;
  // the new entries start on a REFILL_ALIGN boundary; the gap holds dead entries
  const uint32_t base = min((nc + (REFILL_ALIGN - 1)) / REFILL_ALIGN * REFILL_ALIGN, sp.slots);
  const uint32_t room = sp.slots - base;
  const uint32_t m = h < sp.total_units ? min(room, sp.total_units - h) : 0u;
  plan[0] = m ? base : nc; plan[1] = h; plan[2] = m; plan[3] = nc;
  *out_count = m ? base + m : nc;
  *sp.head = h + m;
}

// Publish the frees of the last shading pass (k_trace2 does it at its start; k_tail and
// the host's pool checks need it on their own).
static __global__ void k_pool_publish(unsigned long long* ctr) { pool_publish(ctr); }
// Every ring holds all of its blocks at the start of a render.
static __global__ void k_pool_init(uint32_t* ring, uint32_t n, uint32_t per_ring, unsigned long long* ctr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) ring[i] = i;
  if (i < POOL_SHARDS) {
    unsigned long long* c = ctr + (size_t)i * POOL_CTR_STRIDE;
    c[0] = 0; c[1] = per_ring; c[2] = per_ring;
  }
}

// k_accumulate in its three instances, chosen by the parameter type: P = AccumParams is the
// kernel every render runs; P = AccumMoments (AccumParams and one more pointer: AccumParams
// itself stays as it is) is the moments instance of a session begun with IZPI_PROG_NOISE, which
// also folds each sample's squares into `moments` ([num_pixels][3], DESIGN.md section 3.9:
// nz::fold) in the same pass over the same bytes. The sums' additions are the same in both.
// P = AccumScatter (AccumMoments, the active list and the counts) is the instance of an adaptive
// session's steps after its first retirement: thread p is entry p of
// the list, whose samples lie where pixel p's would, and adds them to the sums and moments of
// pixel list[4 * p + 2] and chunk_spp to its count. It is never the last chunk.
struct AccumMoments : AccumParams {
  double* moments;
};
struct AccumScatter : AccumMoments {
  const uint32_t* list;  // [num_pixels][4]: (x, y, pixel, 0)
  uint32_t* counts;
};
template <class P>
static __global__ void __launch_bounds__(256) k_accumulate(const P ap) {
  constexpr bool M2 = !std::is_same<P, AccumParams>::value;
  constexpr bool LIST = std::is_same<P, AccumScatter>::value;
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= ap.map.num_pixels) return;
  size_t at = p;  // the pixel whose sums this thread holds
  if constexpr (LIST) at = ap.list[4 * (size_t)p + 2];
  double c0 = ap.running[3 * at], c1 = ap.running[3 * at + 1], c2 = ap.running[3 * at + 2];
  double q0 = 0, q1 = 0, q2 = 0;
  if constexpr (M2) { q0 = ap.moments[3 * at]; q1 = ap.moments[3 * at + 1]; q2 = ap.moments[3 * at + 2]; }
  const double* s = ap.samples + (size_t)p * ap.chunk_spp * SMP_D;
  uint32_t k = 0;
  // one sample into the sums (rgb.go:36 col += ..., render/spectral.go:92-96 sum += ...);
  // a raw forward Spectral sample is weighed first
  auto add = [&](double a, double b, double c) {
    if (ap.raw_spectral) {
      double x, y, z;
      spectral_weigh(a, b, c, x, y, z);
      c0 = c0 + x; c1 = c1 + y; c2 = c2 + z;
      if constexpr (M2) nz::fold(x, y, z, q0, q1, q2);
    } else {
      c0 = c0 + a; c1 = c1 + b; c2 = c2 + c;
      if constexpr (M2) nz::fold(a, b, c, q0, q1, q2);
    }
  };
  if ( (ap.chunk_spp & 3u) == 0 && blockIdx.x * 256 + 256 <= ap.map.num_pixels) {
    // Staged through LDS, 4 samples (96 B) of each of the wave's 64 pixels at a time: the
    // wave's lanes load the 64 runs as consecutive 16-B pieces (a load instruction covers
    // ~11 neighbouring runs instead of one piece of 64 runs 12 KB apart), then each lane
    // adds its own pixel's 4 samples from LDS in sample order (rgb.go:36).
    __shared__ double2 st[4][64 * 6];
    double2* w = st[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t p0 = p - lane;  // the wave's first pixel
    const size_t run = (size_t)ap.chunk_spp * 3 / 2;  // double2 per pixel
    const double2* s2 = reinterpret_cast<const double2*>(ap.samples) + (size_t)p0 * run;
    for (; k < ap.chunk_spp; k += 4) {
      double2 v[6];
#pragma unroll
      for (int i = 0; i < 6; i++) {
        const uint32_t q = lane + 64 * i, j = q / 6, c = q % 6;
        v[i] = sld(s2 + (size_t)j * run + (k >> 1) * 3 + c);
      }
#pragma unroll
      for (int i = 0; i < 6; i++) w[lane + 64 * i] = v[i];
      __builtin_amdgcn_wave_barrier();
      const double2 a = w[6 * lane], b = w[6 * lane + 1], c = w[6 * lane + 2];
      const double2 d = w[6 * lane + 3], e = w[6 * lane + 4], f = w[6 * lane + 5];
      __builtin_amdgcn_wave_barrier();
      add(a.x, a.y, b.x);  // sample k
      add(b.y, c.x, c.y);  // sample k + 1
      add(d.x, d.y, e.x);  // sample k + 2
      add(e.y, f.x, f.y);  // sample k + 3
    }
  }
  if ((ap.chunk_spp & 1u) == 0 && k == 0) {
    // two samples (48 B, 16-B aligned for an even chunk_spp) per three 16-B loads: the
    // lanes' runs lie chunk_spp * 24 B apart, so every load instruction touches 64 lines
    // and the instruction count, not the bytes, bounds this loop
    const double2* s2 = reinterpret_cast<const double2*>(s);
    for (; k + 1 < ap.chunk_spp; k += 2) {  // sample order, as rgb.go:36
      const double2 a = s2[3 * (k >> 1)], b = s2[3 * (k >> 1) + 1], c = s2[3 * (k >> 1) + 2];
      add(a.x, a.y, b.x);  // sample k
      add(b.y, c.x, c.y);  // sample k + 1
    }
  }
  for (; k < ap.chunk_spp; k++) add(s[3 * k], s[3 * k + 1], s[3 * k + 2]);  // sample order, as rgb.go:36
  if (LIST || !ap.last) {
    ap.running[3 * at] = c0; ap.running[3 * at + 1] = c1; ap.running[3 * at + 2] = c2;
    if constexpr (M2) { ap.moments[3 * at] = q0; ap.moments[3 * at + 1] = q1; ap.moments[3 * at + 2] = q2; }
    if constexpr (LIST) ap.counts[at] = ap.counts[at] + ap.chunk_spp;
    return;
  }
  // the last chunk: the request's mean into the pixel's slot (pixel_map.h)
  store_pixel(ap.map, p, ap.out, pixel_mean(ap.sampler, c0, ap.spp), pixel_mean(ap.sampler, c1, ap.spp),
              pixel_mean(ap.sampler, c2, ap.spp));
}

void launch_accumulate(hipStream_t st, const AccumParams& ap, double* moments) {
  const dim3 grid((ap.map.num_pixels + 255) / 256);
  if (moments) {
    AccumMoments am;
    static_cast<AccumParams&>(am) = ap;
    am.moments = moments;
    hipLaunchKernelGGL(k_accumulate<AccumMoments>, grid, dim3(256), 0, st, am);
  } else {
    hipLaunchKernelGGL(k_accumulate<AccumParams>, grid, dim3(256), 0, st, ap);
  }
}
void launch_accumulate_list(hipStream_t st, const AccumParams& ap, double* moments, const uint32_t* list, uint32_t* counts) {
  AccumScatter as;
  static_cast<AccumParams&>(as) = ap;
  as.moments = moments; as.list = list; as.counts = counts;
  hipLaunchKernelGGL(k_accumulate<AccumScatter>, dim3((ap.map.num_pixels + 255) / 256), dim3(256), 0, st, as);
}
int prepare_accumulate(izpi_ctx* ctx) {
  int blocks = 0;
  return resident_blocks(ctx, k_accumulate<AccumParams>, &blocks);
}

// The instance rule: the smallest material set that holds the scene's material kinds; the
// compact records of MATSET_CONST are the recursion's (the forward form has none).
const ShadeKernels* shade_instance(uint32_t matset, bool const_basic, uint32_t sampler, bool fwd) {
  int set = matset == 0 ? MATSET_BASIC : (matset & ~(uint32_t)MATSET_SURF) == 0 ? MATSET_SURF : MATSET_FULL;
  if (sampler == IZPI_SAMPLER_COLOUR) {
    if (const_basic && !fwd) set = MATSET_CONST;
    return fwd ? shade_kernels<IZPI_SAMPLER_COLOUR, true>(set) : shade_kernels<IZPI_SAMPLER_COLOUR, false>(set);
  }
  return fwd ? shade_kernels<IZPI_SAMPLER_SPECTRAL, true>(set) : shade_kernels<IZPI_SAMPLER_SPECTRAL, false>(set);
}

// Load the kernel code this scene's renders of k's (sampler, accumulation) run, ahead of the
// first frame: the first occupancy query of a kernel loads its code object, ~14 ms that a fresh
// renderer's first frame paid (tools/first_frame_host.py). Called by izpi_gpu_upload_scene.
// (k_accumulate's query loads this unit's code, the other small kernels of the loop with it.)
int prepare_wavefront(izpi_ctx* ctx, const ShadeKernels& k) {
  int blocks = 0, rc;
  if ((rc = resident_blocks(ctx, k.shade, &blocks, (int)SHADE_THREADS))) return rc;
  if ((rc = resident_blocks(ctx, k.tail32, &blocks))) return rc;
  if ((rc = resident_blocks(ctx, k.tail64, &blocks))) return rc;
  if (k.shade_staged && (rc = resident_blocks(ctx, k.shade_staged, &blocks, (int)SHADE_THREADS))) return rc;
  if (k.start && (rc = resident_blocks(ctx, k.start, &blocks))) return rc;
  if (k.refill && (rc = resident_blocks(ctx, k.refill, &blocks))) return rc;
  return prepare_accumulate(ctx);
}

// One chunk loop of the wavefront scheme: k_start (the recursion) or k_refill (forward) fills
// the slots, then k_trace2 / k_shade alternate until no slot has a ray left (the last few
// paths run to their end in k_tail); k_accumulate folds the chunk's per-sample radiance into
// the pixels in sample order.
int run_wavefront(izpi_ctx* ctx, const izpi_render_req* req, const DevScene& sc, const Tracer& tr, const ShadeKernels& k,
                  ShadeParams& sp, WaveParams& wp, AccumParams& ap, const RunInput& in, RunTimes* out) {
  hipStream_t st = ctx->stream;
  const izpi_render_tuning& tu = tuning_of(req);
  const uint32_t num_pixels = in.num_pixels, chunk = in.chunk, pool_blocks = in.pool_blocks;
  const SampleRange& sr = in.range;
  // the samples finished before sample s of this run (an adaptive session's list: of its session)
  auto finished_before = [&](uint32_t s) {
    return in.list ? in.samples_before + (uint64_t)(s - sr.begin) * num_pixels : (uint64_t)s * num_pixels;
  };
  int shade_res = 0;
  const size_t dyn = sc.lds_bytes;  // the staged tables' LDS arena (render_body)
  int rc = resident_blocks(ctx, k.shade, &shade_res, (int)SHADE_THREADS, dyn);
  if (rc) return rc;
  // The staged form (k_shade<..., STAGE>): a forward Colour render without overflow blocks
  // whose arena holds the Colour tables alone (no Spectral tables, no primitives in LDS: the
  // stage lies behind them), whose entries are the arrays stage_flush writes, and whose
  // blocks stay as many per CU with the stage's LDS as without.
  bool stage = false;
  const char* form = "plain (no staged instance)";
  if (k.shade_staged) {
    if (tu.flags & IZPI_TUNE_NO_SHADE_STAGE) form = "plain (IZPI_TUNE_NO_SHADE_STAGE)";
    else if (sp.rec_pool || sc.lds_bytes != lds_off::COLOUR_END) form = "plain (LDS arena)";
    else if (wp.out.time || wp.out.blk || wp.out.cold || !wp.out.thr) form = "plain (entry arrays)";
    else {
      int stage_res = 0;
      if ((rc = resident_blocks(ctx, k.shade_staged, &stage_res, (int)SHADE_THREADS, dyn + lds_off::STG_BYTES))) return rc;
      stage = stage_res == shade_res;
      form = stage ? "staged" : "plain (occupancy)";
    }
  }
  // tail kernel: used once every unit has started and at most `tail_max` paths remain
  const bool tail_deep = ctx->stack_needed > 32;
  const auto tail = tail_deep ? k.tail64 : k.tail32;
  if (tu.flags & IZPI_TUNE_PASS_LOG) {
    fprintf(stderr, "IZPI_SHADE_INSTANCE %s tail=%d\n", k.name, tail_deep ? 64 : 32);
    fprintf(stderr, "IZPI_SHADE_FORM %s\n", form);
  }
  int tail_res = 0;
  if ((rc = resident_blocks(ctx, tail, &tail_res, 256, dyn))) return rc;
  if ((uint32_t)std::max({tr.blocks * 4, shade_res * (int)SHADE_WAVES, tail_res * 4}) > ctx->num_cus * CPART_BLOCKS_PER_CU * 4 ||
      (uint32_t)shade_res > ctx->num_cus * CPART_BLOCKS_PER_CU) {
    ctx->err = "grid larger than the counter rows or the unwinding queues";
    return IZPI_ERR_INVALID;
  }
  if (tail_deep && (size_t)tail_res * 256 * (64 - TAIL_LDS_STACK) * sizeof(int32_t) > ctx->spill_cap) {
    ctx->err = "k_tail's stack spill does not fit k_trace2's spill area";
    return IZPI_ERR_INVALID;
  }
  int refill_res = 0;
  if (k.fwd && (rc = resident_blocks(ctx, k.refill, &refill_res, 256, 0))) return rc;
  uint64_t tail_max = (uint64_t)tail_res * 256;
  if (tu.tail_paths) tail_max = tu.tail_paths;
  if (tu.flags & IZPI_TUNE_NO_TAIL) tail_max = 0;
  // k_tail's allocations cannot park: every tail path must find a published block
  if (sp.rec_pool) tail_max = std::min<uint64_t>(tail_max, pool_blocks);
  const WaveBuf q[2] = {wp.in, wp.out};  // the two sides of the state; entry counts in d_misc[3..4]
  uint32_t* qn[2] = {misc(ctx, 3), misc(ctx, 4)};
  if (sp.rec_pool)
    hipLaunchKernelGGL(k_pool_init, dim3((pool_blocks + 255) / 256), dim3(256), 0, st, sp.pool_ring, pool_blocks,
                       pool_blocks / POOL_SHARDS, sp.pool_ctr);
  HIP_TRY(hipGetLastError());
  for (uint32_t s0 = sr.begin; s0 < sr.end; s0 += chunk) {
    const uint32_t cs = std::min(chunk, sr.end - s0);
    sp.chunk_spp = cs; sp.s0 = s0; sp.total_units = num_pixels * cs;
    const uint32_t fill = std::min<uint32_t>(sp.slots, sp.total_units);
    HIP_TRY(hipMemsetD32Async(misc(ctx, 0), (int)fill, 1, st));  // unit head: k_start gives slot i unit i
    HIP_TRY(hipMemsetAsync(misc(ctx, 2), 0, 3 * MISC_STRIDE * sizeof(uint32_t), st));  // dequeue cursor, queue counts
    HIP_TRY(hipMemsetAsync(misc(ctx, 6), 0, 2 * MISC_STRIDE * sizeof(uint32_t), st));  // park flags of the two sides
    wp.out = q[0]; wp.out_count = qn[0];
    if (k.fwd) {  // camera entries j = unit j (the unit head starts at `fill` above)
      hipLaunchKernelGGL(k_plan_first, dim3(1), dim3(1), 0, st, wp.out_count, misc(ctx, 5), fill);
      hipLaunchKernelGGL(k.refill, dim3(refill_res), dim3(256), 0, st, sc, sp, wp, (const uint32_t*)misc(ctx, 5));
    } else {
      hipLaunchKernelGGL(k.start, dim3((fill + 255) / 256), dim3(256), 0, st, sc, sp, wp);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_count, qn[0], sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tu.flags & IZPI_TUNE_PASS_LOG) fprintf(stderr, "IZPI_T start_synced %.3f\n", diag_clock_ms());
    uint32_t n = ctx->h_count[0];
    int cur = 0;
    // Launch passes in batches without a host round-trip per pass: both kernels read
    // their queue length from device memory and exit at once when it is zero, so the
    // host only polls the queue length once per batch (overshoot costs a few empty
    // launches of ~5 us).
    // Once every unit has started, the queue only shrinks: poll after every pass, so that
    // k_tail takes over as soon as few enough paths remain instead of up to 8 passes later
    // (each of those last passes costs ~0.3-1 ms of mostly idle machine).
    const bool pass_log = (tu.flags & IZPI_TUNE_PASS_LOG) != 0;  // diagnostics: per-pass times on stderr
    int B = pass_log ? 1 : IZPI_PASS_BATCH;  // (the log reads every pass's queue length)
    while (n > 0) {
      for (int b = 0; b < B; b++) {
        wp.in = q[cur]; wp.in_count = qn[cur];
        wp.out = q[1 - cur]; wp.out_count = qn[1 - cur];
        wp.in_park = misc(ctx, 6 + cur); wp.out_park = misc(ctx, 6 + (1 - cur));
        wp.cam = k.fwd ? misc(ctx, 5) : nullptr;  // (k_refill_plan's plan of the pass before: `in`'s camera entries)
        // (k_trace2 zeroes out_count and out_park, k_shade the dequeue cursor for the next pass)
        HIP_TRY(hipEventRecord(ctx->evb[3 * b], st));
        launch_trace(ctx, sc, tr, wp, st, ctx->d_spill);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ctx->evb[3 * b + 1], st));
        if (stage) hipLaunchKernelGGL(k.shade_staged, dim3(shade_res), dim3(SHADE_THREADS), dyn + lds_off::STG_BYTES, st, sc, sp, wp);
        else hipLaunchKernelGGL(k.shade, dim3(shade_res), dim3(SHADE_THREADS), dyn, st, sc, sp, wp);
        HIP_TRY(hipGetLastError());
        if (k.fwd) {
          hipLaunchKernelGGL(k_refill_plan, dim3(1), dim3(1), 0, st, sp, wp.out_count, misc(ctx, 5));
          hipLaunchKernelGGL(k.refill, dim3(refill_res), dim3(256), 0, st, sc, sp, wp, (const uint32_t*)misc(ctx, 5));
          HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(ctx->evb[3 * b + 2], st));
        cur = 1 - cur;
      }
      HIP_TRY(hipMemcpyAsync(ctx->h_count, ctx->d_misc, 8 * MISC_STRIDE * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (int b = 0; b < B; b++) {
        float t_ms = 0, s_ms = 0;
        HIP_TRY(hipEventElapsedTime(&t_ms, ctx->evb[3 * b], ctx->evb[3 * b + 1]));
        HIP_TRY(hipEventElapsedTime(&s_ms, ctx->evb[3 * b + 1], ctx->evb[3 * b + 2]));
        out->trace_ms += t_ms;
        out->shade_ms += s_ms;
        if (pass_log) fprintf(stderr, "IZPI_PASS %u trace %.3f shade %.3f\n", out->launches, t_ms, s_ms);
        out->launches++;
      }
      const uint32_t head = ctx->h_count[0];
      n = ctx->h_count[(3 + cur) * MISC_STRIDE];
      {  // units handed out minus the entries still queued: samples finished (a lower bound)
        const uint64_t started = std::min<uint64_t>(head, sp.total_units);
        ctx->prog_done.store(finished_before(s0) + (started > n ? started - n : 0), std::memory_order_relaxed);
      }
      if (pass_log) fprintf(stderr, "IZPI_BATCH queue %u head %u\n", n, head);
      if (head >= sp.total_units) B = 1;
      // every unit has started: finish the remaining paths in one k_tail launch
      if (n > 0 && n <= tail_max && head >= sp.total_units) {
        wp.in = q[cur]; wp.in_count = qn[cur];
        HIP_TRY(hipEventRecord(ctx->ev2, st));
        if (sp.rec_pool) hipLaunchKernelGGL(k_pool_publish, dim3(1), dim3(256), 0, st, sp.pool_ctr);
        // (the deep instance spills stack entries past 32 into k_trace2's spill area, which
        // holds 64 entries for each of k_trace2's threads, more than k_tail has)
        hipLaunchKernelGGL(tail, dim3(tail_res), dim3(256), dyn, st, sc, sp, wp, ctx->d_spill);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ctx->ev3, st));
        HIP_TRY(hipEventSynchronize(ctx->ev3));
        float t_ms = 0;
        HIP_TRY(hipEventElapsedTime(&t_ms, ctx->ev2, ctx->ev3));
        out->tail_ms += t_ms;
        n = 0;
      }
    }
    ap.chunk_spp = cs;
    ap.raw_spectral = k.fwd && k.sampler == IZPI_SAMPLER_SPECTRAL ? 1u : 0u;
    ap.last = (!sr.keep && s0 + cs >= sr.end) ? 1u : 0u;
    ctx->prog_done.store(finished_before(s0 + cs), std::memory_order_relaxed);
    if (in.list) launch_accumulate_list(st, ap, session_moments(ctx, sr), in.list, in.counts);
    else launch_accumulate(st, ap, session_moments(ctx, sr));
    HIP_TRY(hipGetLastError());
  }
  return IZPI_OK;
}
