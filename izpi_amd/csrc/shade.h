// shade.h — the sampler, materials and pdfs of one bounce (k_shade), the first fill (k_start),
// the wavefront's tail (k_tail) and forward mode's refill (k_refill): device code, and the
// tables that hand its instances to the pass loop (shade_kernels; the loop: wavefront.hip).
// Compiled by the shade_*.hip translation units, one per (sampler, accumulation): each
// instantiates shade_kernels for its pair, so the four sets of kernel instances compile in
// parallel.
#pragma once
#include "izpi_kern.h"

// First fill of the queue (first pass of a chunk): record slot j takes unit j (the host
// starts the unit head at min(slots, units), so no atomic is needed: one counter word
// serialises ~88 atomics/us), then further units from the head while its path needs no
// tracing; the path goes to entry j of `out`.
template <int SAMPLER, bool FWD>
__global__ void __launch_bounds__(256) k_start(const DevScene sc, const ShadeParams sp_in, const WaveParams wp) {
  ShadeParams sp = sp_in;
  sp.staged = 0;  // k_start stages no tables: its path starts read them from global memory
  sp.prims_staged = 0;
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  bool want = j < sp.slots;
  bool push = false;
  bool first = true;
  PathSt P;
  RayRec R;
  P.rslot = j;
  // a wave keeps grabbing while any of its lanes still lacks a traceable path
  for (;;) {
    uint32_t unit;
    if (first) {
      unit = (want && j < sp.total_units) ? j : 0xFFFFFFFFu;
      first = false;
    } else {
      unit = grab_unit(sp, want);
    }
    if (__ballot(want) == 0) break;
    if (want) {
      if (unit == 0xFFFFFFFFu) {
        want = false;
      } else if (start_path<SAMPLER, FWD>(sc, sp, unit, P, R)) {
        want = false;
        push = true;
      }
    }
  }
  // Entry j of the first queue belongs to record slot j (no queue atomic: one per block on
  // one counter word made this kernel 1.9 ms per C3 frame); a slot whose samples all
  // completed without a ray (spectral pdf 0, the units ran out) leaves a dead entry, which
  // the first shading pass drops.
  const uint32_t fill = min(sp.slots, sp.total_units);
  if (j < fill) {
    if (push) store_entry<SAMPLER, FWD>(wp.out, j, P, R);
    else dead_entry(wp.out, j);
  }
  if (j == 0) *wp.out_count = fill;
}

#ifdef IZPI_SHADE_CLOCKS
// Timing builds only: wave cycles per section of shade_item, accumulated in LDS by the
// first active lane of the wave that runs the section (so divergent sections count the
// wave's time once), added to the CNT_SCLK_* counters at the end of the kernel.
enum { SCLK_MAT = 0, SCLK_FIN, SCLK_MIX, SCLK_LPDF, SCLK_ENTRY, SCLK_TEX, SCLK_RB1, SCLK_RATOM, SCLK_RB2, SCLK_N };
IZPI_DEV unsigned long long* sclk_lds() {
  __shared__ unsigned long long c[16][SCLK_N];
  return &c[(threadIdx.x >> 6) & 15][0];
}
IZPI_DEV void sclk_add(int sec, uint64_t dt) {
  const uint64_t act = __ballot(1);
  if ((threadIdx.x & 63) == (uint32_t)(__ffsll((long long)act) - 1)) sclk_lds()[sec] += dt;
}
IZPI_DEV void sclk_flush(unsigned long long* counters) {
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < SCLK_N; k++) atomicAdd(counters + CNT_SCLK_MAT + k, sclk_lds()[k]);
}
IZPI_DEV void sclk_zero() {
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < SCLK_N; k++) sclk_lds()[k] = 0;
  __syncthreads();
}
#define SCLK_T(v) const uint64_t v = __builtin_readcyclecounter()
#define SCLK_ADD(sec, t0) sclk_add(sec, __builtin_readcyclecounter() - (t0))
// wait for every outstanding vector memory access (vmcnt(0); expcnt, lgkmcnt left alone):
// separates a section's memory wait from the work after it
#define SCLK_VMWAIT() __builtin_amdgcn_s_waitcnt(0x0F70)
#else
#define SCLK_VMWAIT() (void)0
#define SCLK_T(v) (void)0
#define SCLK_ADD(sec, t0) (void)0
#endif

// One block-wide reservation phase for a shading iteration (ONE pair of barriers, two
// atomics by one thread): `unit_want` lanes get consecutive work units from the unit
// head (the units past total_units are not granted); lanes with `put` and granted
// `unit_want` lanes get consecutive output entries, `put` lanes first. q_rank: the
// lane's rank among the block's `queue` lanes (deferred unwinding jobs), q_total: their number. A granted lane
// whose new path cannot trace (start_path false) leaves a RAY_DEAD entry behind.
// QSEP: `queue` lanes are a subset of the `unit_want` lanes with a ballot of their own;
// otherwise they are the `unit_want` lanes.
template <bool QSEP>
IZPI_DEV void block_reserve2(const ShadeParams& sp, uint32_t* out_count, bool put, bool unit_want, uint32_t& unit,
                             uint32_t& pos, uint32_t& parity, bool& exhausted, bool queue, uint32_t& q_rank, uint32_t& q_total) {
  __shared__ uint32_t s_p[2][SHADE_WAVES], s_u[2][SHADE_WAVES], s_q[2][SHADE_WAVES];
  __shared__ uint32_t s_pbase[2], s_ubase[2], s_granted[2], s_nput[2], s_nent[2];
  const uint32_t b = parity;
  parity ^= 1u;
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t lt = (1ull << lane) - 1;
  const uint64_t mp = __ballot(put), mu = __ballot(unit_want), mq = QSEP ? __ballot(queue) : 0ull;
  if (lane == 0) { s_p[b][w] = (uint32_t)__popcll(mp); s_u[b][w] = (uint32_t)__popcll(mu); if (QSEP) s_q[b][w] = (uint32_t)__popcll(mq); }
  SCLK_T(rb0);
  __syncthreads();
  SCLK_ADD(SCLK_RB1, rb0);
  SCLK_T(rb1);
  // both atomics in flight together: entries are reserved for every unit_want lane
  // until this block has seen the unit head run out (`exhausted`, thread 0's register);
  // a lane reserved an entry but denied a unit leaves a dead entry (at most one
  // iteration per block, in the frame's last passes)
  uint32_t np = 0, nu = 0, u0 = 0, pb = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t k = 0; k < SHADE_WAVES; k++) { np += s_p[b][k]; nu += s_u[b][k]; }
    if (exhausted) nu = 0;
    u0 = nu ? atomicAdd(sp.head, nu) : sp.total_units;
    pb = np + nu ? atomicAdd(out_count, np + nu) : 0u;
  }
  if (threadIdx.x == 0) {
    const uint32_t ne = np + nu;
    // (an iteration without finished paths asks for nothing and learns nothing: it must
    // not mark the block exhausted, or the block's later finished paths lose their slots)
    if (nu && u0 + nu >= sp.total_units) exhausted = true;
    s_pbase[b] = pb;
    s_ubase[b] = u0;
    s_granted[b] = u0 >= sp.total_units ? 0u : min(nu, sp.total_units - u0);
    s_nput[b] = np;
    s_nent[b] = ne;
    SCLK_VMWAIT();
    SCLK_ADD(SCLK_RATOM, rb1);
  }
  __syncthreads();
  SCLK_ADD(SCLK_RB2, rb1);
  uint32_t ur = (uint32_t)__popcll(mu & lt), pr = (uint32_t)__popcll(mp & lt);
  for (uint32_t i = 0; i < w; i++) { ur += s_u[b][i]; pr += s_p[b][i]; }
  if constexpr (QSEP) {
    q_rank = (uint32_t)__popcll(mq & lt);
    q_total = 0;
#pragma unroll
    for (uint32_t k = 0; k < SHADE_WAVES; k++) {
      q_rank += k < w ? s_q[b][k] : 0u;
      q_total += s_q[b][k];
    }
  } else {
    q_rank = ur;
    q_total = 0;
#pragma unroll
    for (uint32_t k = 0; k < SHADE_WAVES; k++) q_total += s_u[b][k];
  }
  const bool has_entry = unit_want && s_nput[b] + ur < s_nent[b];
  const bool granted = unit_want && ur < s_granted[b];
  unit = granted ? s_ubase[b] + ur : 0xFFFFFFFFu;
  pos = put ? s_pbase[b] + pr : (has_entry ? s_pbase[b] + s_nput[b] + ur : 0xFFFFFFFFu);
}

// ---- the forward Colour k_shade's staged form (k_shade<..., STAGE = true>)
// One word serves ~88 returning atomics per microsecond chip-wide, and block_reserve2's one
// per block-iteration on *out_count (5.75 M per C3 frame) had become the floor of forward
// shading. Which entries a block gets does not change the image, so every other iteration
// (phase 0) keeps its continuing entries in LDS, ranked within the block (stage_put: one
// barrier, no atomic), and the next one (phase 1) reserves for both with one atomic
// (block_reserve_fwd) and copies the staged entries out in front of its own (stage_flush).
// The stage is lds_off::STG_*: planes that mirror the arrays store_entry writes for a
// forward Colour render without ray times, overflow blocks or cold records.
typedef double stg_d2 __attribute__((ext_vector_type(2)));
typedef uint32_t stg_u4 __attribute__((ext_vector_type(4)));
#define IZPI_LDS3 __attribute__((address_space(3)))
IZPI_DEV IZPI_LDS3 stg_d2* stg_ray() { return (IZPI_LDS3 stg_d2*)(lds_arena() + lds_off::STG_RAY); }
IZPI_DEV IZPI_LDS3 double* stg_thr() { return (IZPI_LDS3 double*)(lds_arena() + lds_off::STG_THR); }
IZPI_DEV IZPI_LDS3 stg_u4* stg_path() { return (IZPI_LDS3 stg_u4*)(lds_arena() + lds_off::STG_PATH); }
IZPI_DEV IZPI_LDS3 uint32_t* stg_kind() { return (IZPI_LDS3 uint32_t*)(lds_arena() + lds_off::STG_KIND); }
// Phase 0: the `put` lanes' entries go to the stage at their block-local rank; returns their
// number (the same in every thread). The block's next use of s_n is two iterations on, behind
// the barriers of block_reserve_fwd.
IZPI_DEV uint32_t stage_put(bool put, const PathSt& P, const RayRec& R) {
  __shared__ uint32_t s_n[SHADE_WAVES];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t mp = __ballot(put);
  if (lane == 0) s_n[w] = (uint32_t)__popcll(mp);
  SCLK_T(rb0);
  __syncthreads();
  SCLK_ADD(SCLK_RB1, rb0);
  uint32_t r = (uint32_t)__popcll(mp & ((1ull << lane) - 1)), n = 0;
#pragma unroll
  for (uint32_t k = 0; k < SHADE_WAVES; k++) {
    r += k < w ? s_n[k] : 0u;
    n += s_n[k];
  }
  if (put) {
    stg_ray()[r] = stg_d2{R.o[0], R.o[1]};
    stg_ray()[SHADE_THREADS + r] = stg_d2{R.o[2], R.d[0]};
    stg_ray()[2 * SHADE_THREADS + r] = stg_d2{R.d[1], R.d[2]};
    stg_thr()[r] = P.thr[0];
    stg_thr()[SHADE_THREADS + r] = P.thr[1];
    stg_thr()[2 * SHADE_THREADS + r] = P.thr[2];
    stg_path()[r] = stg_u4{P.rng, P.depth | P.zf << 16, P.unit, P.rslot};
    stg_kind()[r] = R.kind;
  }
  return n;
}
// Phase 1's reservation (block_reserve2 without units): `staged` + the block's `put` lanes
// entries of *out_count in one atomic, none when that is nothing. `base` is the first of
// them, `rank` the lane's rank among the `put` lanes. Two calls are always a stage_put
// (a barrier) apart, so one set of LDS words serves.
IZPI_DEV void block_reserve_fwd(uint32_t* out_count, bool put, uint32_t staged, uint32_t& base, uint32_t& rank) {
  __shared__ uint32_t s_p[SHADE_WAVES], s_base;
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t mp = __ballot(put);
  if (lane == 0) s_p[w] = (uint32_t)__popcll(mp);
  SCLK_T(rb0);
  __syncthreads();
  SCLK_ADD(SCLK_RB1, rb0);
  SCLK_T(rb1);
  if (threadIdx.x == 0) {
    uint32_t ne = staged;
#pragma unroll
    for (uint32_t k = 0; k < SHADE_WAVES; k++) ne += s_p[k];
    s_base = ne ? atomicAdd(out_count, ne) : 0u;
    SCLK_VMWAIT();
    SCLK_ADD(SCLK_RATOM, rb1);
  }
  __syncthreads();
  SCLK_ADD(SCLK_RB2, rb1);
  rank = (uint32_t)__popcll(mp & ((1ull << lane) - 1));
  for (uint32_t k = 0; k < w; k++) rank += s_p[k];
  base = s_base;
}
// Thread t < n copies staged entry t to entry base + t of `out` (after block_reserve_fwd's
// second barrier): consecutive positions, 16 B or 8 B per lane and array.
IZPI_DEV void stage_flush(const WaveBuf& out, uint32_t base, uint32_t n) {
  const uint32_t t = threadIdx.x;
  if (t >= n) return;
  const uint32_t pos = base + t;
  const stg_d2 r0 = stg_ray()[t], r1 = stg_ray()[SHADE_THREADS + t], r2 = stg_ray()[2 * SHADE_THREADS + t];
  const double t0 = stg_thr()[t], t1 = stg_thr()[SHADE_THREADS + t], t2 = stg_thr()[2 * SHADE_THREADS + t];
  const stg_u4 ph = stg_path()[t];
  const uint32_t kind = stg_kind()[t];
  sst(out.thr + pos, t0);
  sst(out.thr + out.tplane + pos, t1);
  sst(out.thr + 2 * (size_t)out.tplane + pos, t2);
  double2* r = reinterpret_cast<double2*>(out.ray + pos);
  sst(r, make_double2(r0.x, r0.y));
  sst(r + 1, make_double2(r1.x, r1.y));
  sst(r + 2, make_double2(r2.x, r2.y));
  sst(out.kind + pos, kind);
  sst(out.path + pos, PathHot{ph.x, ph.y, ph.z, ph.w});
}

// A lane whose path finished got `unit` and entry `pos` (block_reserve2): start the
// unit's path in the finished path's record slot and store it; when its sample completes
// without a ray, take further units one at a time (rare), and leave a dead entry when
// none traces.
template <int SAMPLER, bool FWD>
IZPI_DEV void refill_one(const DevScene& sc, const ShadeParams& sp, const WaveBuf& out, uint32_t unit, uint32_t pos,
                         PathSt& P) {
  RayRec R;
  for (;;) {
    if (start_path<SAMPLER, FWD>(sc, sp, unit, P, R)) {
      store_entry<SAMPLER, FWD>(out, pos, P, R);
      return;
    }
    unit = atomicAdd(sp.head, 1u);
    if (unit >= sp.total_units) {
      dead_entry(out, pos);
      return;
    }
  }
}




// One shading pass of `slot` (its ray was traced): Colour.Sample / SampleSpectral
// one bounce deep (colour.go:33-65, sampler/spectral.go:47-80). Sets `push` when the path
// has a ray to trace next and `done` when its sample finished.
// Entry i of `in`: P is its path state (load_path), with blk set to the path's overflow
// block when it needs one (P.depth >= rec_dense); `kind` its kind word. On return, P and
// R hold the continuing path and its next ray (`push`), or `done` is set and `fblk` is
// the block to free. DEFER: a finished path is not unwound here (`queued`; Colour: only
// one whose unwinding reads records, finish_reads); R.o holds its terminal radiance
// (Spectral: R.o[0]) for the caller's queue (fin_queue), and the caller frees its block
// after the unwinding. (Spectral queues every finished path: the test cost the Spectral
// instances up to 24 more spilled VGPRs, C5 shade 320 -> 352 ms.)
template <int SAMPLER, int MATSET, bool DEFER, bool FWD>
IZPI_DEV void shade_item(const DevScene& sc, const ShadeParams& sp, const WaveBuf& in, uint32_t i, uint32_t kind,
                         const EntryIn& E, PathSt& P, RayRec& R, bool& push, bool& done, uint32_t& fblk, uint32_t& c_lt,
                         uint32_t& c_ls, bool& queued) {
  const bool COLOUR = SAMPLER == IZPI_SAMPLER_COLOUR;
  const bool st = sp.staged != 0;  // the scene's small tables are in this block's LDS
  SCLK_T(sc0);
  SCLK_VMWAIT();
  SCLK_ADD(SCLK_ENTRY, sc0);
  for (int k = 0; k < 3; k++) { R.o[k] = E.ray.o[k]; R.d[k] = E.ray.d[k]; }
  R.kind = kind;
  R.time = E.time;  // NewRay(hr.P, dir, r.Time()): the next ray keeps the time
  HitOut H;
  H.t = E.hit.x; H.prim = (int32_t)__double2loint(E.hit.y); H.pad = 0; H.u = 0; H.v = 0;  // (u, v) read on demand
  Lcg rng;
  rng.s = P.rng;
  const V3 ro = mk(R.o[0], R.o[1], R.o[2]), rd = mk(R.d[0], R.d[1], R.d[2]);
  V3 L = mk(0, 0, 0);
  bool terminal = false;
  bool spec = false, have_pdf = false, zero_spdf = false;
  V3 att = mk(0, 0, 0), next_o = mk(0, 0, 0), next_d = mk(0, 0, 0);
  V3 hit_n = mk(0, 0, 0);
  uint32_t rec_mat = 0;
  Onb cos_onb;
  if (ms_has(MATSET, MS_DIEL) && kind_of(R.kind) == RAY_PATHLEN) {
    // calculatePathLength result (dielectric.go:135-152) -> finish the glass bounce
    const PathCold& pc = in.cold[i];
    const V3 hp = mk(pc.pend[0], pc.pend[1], pc.pend[2]);
    const double len = H.prim >= 0 ? path_length(hp, add(ro, smul(rd, H.t))) : 10.0;  // no exit: dielectric.go:152
    const uint32_t mat_id = R.kind >> KIND_MAT_SHIFT;  // dielectric material stashed by the glass bounce
    const izpi_material gm_ = mat_rec(sc, st, mat_id);
    if (COLOUR) att = mk(gm::exp(-gm_.rgb[0] * len), gm::exp(-gm_.rgb[1] * len), gm::exp(-gm_.rgb[2] * len));
    else att.x = gm_.absorb_tex >= 0 ? gm::exp(-tex_spectral(sc, gm_.absorb_tex, P.lambda, 0.0, 0.0, st) * len) : 1.0;
    spec = true;
    next_o = hp;
    next_d = rd;
  } else if (H.prim < 0) {
    L = COLOUR ? mk(sp.background[0], sp.background[1], sp.background[2])
               : mk(bg_value(sp, P.lambda), 0, 0);
    terminal = true;
  } else {
    const bool pst = sp.prims_staged != 0;
    const GShade gs = gshade_of(sc, pst, H.prim);
    HitRec h;
    hit_record(sc, H, in.huv ? in.huv + (size_t)i * in.hs : nullptr, gs, ro, rd, R.time, (gs_cflags(gs) & 2u) != 0, h, st, ms_has(MATSET, MS_PBR), pst);
    hit_n = h.n;
    rec_mat = h.mat;
    next_o = h.p;
    // the shade record carries the material kind and, for a constant RGB texture, its
    // value: the common Lambert/light hit reads no material or texture record
    const izpi_material m = mat_rec(sc, st, h.mat);
    const bool cconst = COLOUR && (gs_cflags(gs) & 1u) != 0;
    V3 cval = mk(0, 0, 0);
    if (cconst) { const double4 c4 = mat_const_of(sp, h.mat); cval = mk(c4.x, c4.y, c4.z); }
    switch (gs_kind(gs)) {
      case IZPI_MAT_DIFFUSE_LIGHT: {  // no scatter: return emitted (diffuselight.go:49-63)
        if (dot(h.n, rd) < 0.0) {
          if (cconst) L = cval;
          else if (COLOUR) L = tex_rgb(sc, m.albedo_tex, h.u, h.v, st);
          else L.x = tex_spectral(sc, m.spectral_tex, P.lambda, h.u, h.v, st);
        }
        terminal = true;
        break;
      }
      case IZPI_MAT_LAMBERT: {  // lambertian.go:44-70: 2 draws for a ray the sampler discards (A6)
        rng.next();
        rng.next();
        cos_onb.build(h.n);
        if (cconst) att = cval;
        else if (COLOUR) att = tex_rgb(sc, m.albedo_tex, h.u, h.v, st);
        else att.x = tex_spectral(sc, m.spectral_tex, P.lambda, h.u, h.v, st);
        have_pdf = true;
        break;
      }
      case IZPI_MAT_ISOTROPIC: {  // isotropic.go:32-60: a randomInUnitSphere ray the sampler discards,
        // Cosine(N) as the material pdf of the mixture, ScatteringPDF 0; Spectral: the albedo's red
        if constexpr (!ms_has(MATSET, MS_ISO)) { atomicOr(sp.error, 2u); terminal = true; break; }
        (void)random_in_unit_sphere(rng);
        cos_onb.build(h.n);
        const V3 a = tex_rgb(sc, m.albedo_tex, h.u, h.v, st);
        if (COLOUR) att = a; else att.x = a.x;
        have_pdf = true;
        zero_spdf = true;
        break;
      }
      case IZPI_MAT_DIELECTRIC: {  // dielectric.go:156-207
        if constexpr (!ms_has(MATSET, MS_DIEL)) { atomicOr(sp.error, 2u); terminal = true; break; }
        const double ri = COLOUR ? m.ref_idx : tex_spectral(sc, m.spectral_tex, P.lambda, 0.0, 0.0, st);
        bool reflected;
        next_d = dielectric_scatter(rd, h.n, ri, rng, reflected);
        const bool beer_rgb = COLOUR && (m.flags & IZPI_MATF_BEER_LAMBERT) && !(m.rgb[0] == 0 && m.rgb[1] == 0 && m.rgb[2] == 0);
        if (!reflected && (!COLOUR || beer_rgb)) {
          // the extra World.Hit of calculatePathLength: trace it, finish next pass
          P.pend[0] = h.p.x; P.pend[1] = h.p.y; P.pend[2] = h.p.z;
          P.rng = rng.s;
          const V3 po = add(h.p, smul(next_d, 0.001));
          R.o[0] = po.x; R.o[1] = po.y; R.o[2] = po.z;
          R.d[0] = next_d.x; R.d[1] = next_d.y; R.d[2] = next_d.z;
          R.kind = RAY_PATHLEN | (h.mat << KIND_MAT_SHIFT);
          push = true;
          break;
        }
        att = mk(1.0, 1.0, 1.0);
        spec = true;
        break;
      }
      case IZPI_MAT_METAL: {  // metal.go:34-41 (RGB only: SpectralScatter is nonSpectral)
        if constexpr (!ms_has(MATSET, MS_METAL)) { atomicOr(sp.error, 2u); terminal = true; break; }
        if (!COLOUR) { terminal = true; break; }
        V3 reflected = reflect(unit(rd), h.n);
        next_d = add(reflected, smul(random_in_unit_sphere(rng), m.fuzz));
        att = mk(m.rgb[0], m.rgb[1], m.rgb[2]);
        spec = true;
        break;
      }
      case IZPI_MAT_PBR: {  // pbr.go:59-155 / 158-263
        if constexpr (!ms_has(MATSET, MS_PBR)) { atomicOr(sp.error, 2u); terminal = true; break; }
        // the four texture slots (LDS, or one 64-B record); every lookup below is issued
        // before the first of them is used
        SCLK_T(sct);
        const TexSlot s_alb = mat_slot(sc, st, h.mat, 0), s_nrm = mat_slot(sc, st, h.mat, 1),
                      s_rgh = mat_slot(sc, st, h.mat, 2), s_met = mat_slot(sc, st, h.mat, 3);
        // one texel index for the images of the normal map's size (C4: all four)
        const uint32_t w0 = s_nrm.w, h0 = s_nrm.hf & 0x3FFFFFFFu;
        const uint64_t k0 = (s_nrm.hf >> 30) <= TEXF_GRAY ? image_index(w0, h0, h.u, h.v) : 0;
        double alb_s = 0;
        if (COLOUR) att = slot_rgb_k(sc, s_alb, h.u, h.v, st, w0, h0, k0);
        else if (m.spectral_tex >= 0) alb_s = tex_spectral(sc, m.spectral_tex, P.lambda, h.u, h.v, st);
        else { V3 c = slot_rgb_k(sc, s_alb, h.u, h.v, st, w0, h0, k0); alb_s = 0.299 * c.x + 0.587 * c.y + 0.114 * c.z; }
        V3 rough = slot_set(s_rgh) ? slot_rgb_k(sc, s_rgh, h.u, h.v, st, w0, h0, k0) : mk(0.5, 0.5, 0.5);
        V3 metal = slot_set(s_met) ? slot_rgb_k(sc, s_met, h.u, h.v, st, w0, h0, k0) : mk(0.0, 0.0, 0.0);
        const bool has_nmap = slot_set(s_nrm);
        const V3 nuv = has_nmap ? slot_rgb_k(sc, s_nrm, h.u, h.v, st, w0, h0, k0) : mk(0, 0, 0);  // one texel for both uses
        SCLK_VMWAIT();
        SCLK_ADD(SCLK_TEX, sct);
        if (has_nmap && IZPI_PRIM_KIND(gs.ref) == IZPI_PRIM_TRIANGLE) {
          h.n = nmap_tbn(sc, H.prim, h.n, nuv, pst);  // the hit record's normal (triangle.go:250-264)
          hit_n = h.n;
        }
        V3 normal = h.n;
        if (has_nmap) {
          V3 tn = mk(2.0 * nuv.x - 1.0, 2.0 * nuv.y - 1.0, nuv.z);
          V3 nn0 = h.n;
          V3 t = cross(nn0, mk(0, 1, 0));
          if (dot(t, t) < 0.001) t = cross(nn0, mk(1, 0, 0));
          t = sdiv(t, length(t));
          V3 b = cross(nn0, t);
          b = sdiv(b, length(b));
          V3 nn = mk(t.x * tn.x + b.x * tn.y + nn0.x * tn.z, t.y * tn.x + b.y * tn.y + nn0.y * tn.z,
                     t.z * tn.x + b.z * tn.y + nn0.z * tn.z);
          normal = sdiv(nn, length(nn));
        }
        double rv = (rough.x + rough.y + rough.z) / 3.0;
        double mv = (metal.x + metal.y + metal.z) / 3.0;
        cos_onb.build(normal);  // the scatter's ONB and the sampler's Cosine(normal) pdf: one build (onb.go:38-67)
        const Onb& uvw = cos_onb;
        const V3 urd = unit(rd);  // (one evaluation for both uses)
        V3 reflected = reflect(urd, normal);
        double cosTheta = gm::abs(dot(urd, normal));
        double fresnel = 0.04 + (1.0 - 0.04) * gm::pow(1.0 - cosTheta, 5.0);
        fresnel = fresnel + (mv * 0.5);
        double sprob = fresnel * (1.0 - rv);
        if (rng.next() < sprob) {
          double rf = gm::max(0.01, rv * 0.3);
          V3 rdir = random_in_unit_sphere(rng);
          next_d = unit(add(reflected, smul(rdir, rf)));
          spec = true;
        } else {
          next_d = unit(uvw.local(random_cosine_direction(rng)));
          spec = false;
          have_pdf = true;  // the sampler ignores this ray and samples the mixture pdf
        }
        if (!COLOUR) att.x = spec ? alb_s * 1.5 : alb_s;
        break;
      }
      default: {
        atomicOr(sp.error, 2u);
        terminal = true;
      }
    }
  }
  SCLK_ADD(SCLK_MAT, sc0);
  if (!push) {
    if (terminal) {
      SCLK_T(sc1);
      if constexpr (FWD) finish_fwd<SAMPLER>(sp, P, L);
      else if constexpr (DEFER && !COLOUR) { R.o[0] = L.x; R.o[1] = L.y; R.o[2] = L.z; }
      else if (DEFER && finish_reads<SAMPLER, MATSET>(P, L)) { R.o[0] = L.x; R.o[1] = L.y; R.o[2] = L.z; queued = true; }
      else finish<SAMPLER, MATSET>(sp, P, L);
      SCLK_ADD(SCLK_FIN, sc1);
      done = true;
      fblk = P.blk;
    } else {
      SCLK_T(sc2);
      if (have_pdf) {
        // Mixture(Hitable(lights, P), Cosine(N)) (colour.go:48-51, mixture.go:17-33)
        V3 dir;
        if (rng.next() < 0.5) dir = lights_random(sc, st, next_o, rng);
        else dir = cos_onb.local(random_cosine_direction(rng));
        // (evaluated in an order that frees the ONB, normal and attenuation before
        // the light-pdf loop; every value is computed exactly as in the reference)
        const V3 ud = unit(dir);
        const double cosv = dot(ud, cos_onb.w);
        const double cos_pdf = cosv > 0 ? cosv / 3.141592653589793 : 0;
        double sc_cos = dot(hit_n, ud);  // ScatteringPDF with the hit normal
        if (sc_cos < 0) sc_cos = 0;
        const double spdf = zero_spdf ? 0.0 : sc_cos / 3.141592653589793;  // Isotropic.ScatteringPDF is 0
        if constexpr (FWD) {  // T * att now (frees T and att during the light-pdf loop), * (s / p) after it
          P.thr[0] = P.thr[0] * att.x;
          if (COLOUR) { P.thr[1] = P.thr[1] * att.y; P.thr[2] = P.thr[2] * att.z; }
        } else {
          rec_store<SAMPLER, MATSET>(sp, P.rslot, P.blk, P.depth, false, att, spdf, rec_mat);
        }
        SCLK_T(sc3);
        const double pdf_val = 0.5 * lights_pdf(sc, st, next_o, dir, c_lt, c_ls) + 0.5 * cos_pdf;
        SCLK_ADD(SCLK_LPDF, sc3);
        if constexpr (FWD) {
          const double w = spdf / pdf_val;
          P.thr[0] = P.thr[0] * w;
          if (COLOUR) { P.thr[1] = P.thr[1] * w; P.thr[2] = P.thr[2] * w; }
        } else {
          sst(rec_ptr<SAMPLER, MATSET>(sp, P.rslot, P.blk, P.depth) + RecLayout<SAMPLER, MATSET>::P, pdf_val);
          if constexpr (ms_spec(MATSET) || SAMPLER == IZPI_SAMPLER_SPECTRAL) rec_zero_track<SAMPLER>(P.zf, false, att, spdf, pdf_val);
        }
        next_d = dir;
      } else if constexpr (FWD) {
        P.thr[0] = P.thr[0] * att.x;
        if (COLOUR) { P.thr[1] = P.thr[1] * att.y; P.thr[2] = P.thr[2] * att.z; }
      } else {
        rec_store<SAMPLER, MATSET>(sp, P.rslot, P.blk, P.depth, true, att, 0, rec_mat);
        rec_zero_track<SAMPLER>(P.zf, true, att, 0.0, 0.0);
      }
      SCLK_ADD(SCLK_MIX, sc2);
      P.depth++;
      P.rng = rng.s;
      if (P.depth >= sp.max_depth) {
        const V3 Lt = terminal_max_depth(sp, P, COLOUR);
        if constexpr (FWD) finish_fwd<SAMPLER>(sp, P, Lt);
        else if constexpr (DEFER && !COLOUR) { R.o[0] = Lt.x; R.o[1] = Lt.y; R.o[2] = Lt.z; }
        else if (DEFER && finish_reads<SAMPLER, MATSET>(P, Lt)) { R.o[0] = Lt.x; R.o[1] = Lt.y; R.o[2] = Lt.z; queued = true; }
        else finish<SAMPLER, MATSET>(sp, P, Lt);
        done = true;
        fblk = P.blk;
      } else {
        R.o[0] = next_o.x; R.o[1] = next_o.y; R.o[2] = next_o.z;
        R.d[0] = next_d.x; R.d[1] = next_d.y; R.d[2] = next_d.z;
        R.kind = RAY_MAIN;
        push = true;
      }
    }
  }
}

// ---- overflow record blocks
// POOL_SHARDS rings of free block ids. A ring holds its own blocks only: block b belongs
// to ring b >> pool_shift, and a freed block goes back to its ring, so no ring ever holds
// more than its 1 << pool_shift entries. Each ring is a FIFO between an allocation head
// and a free tail (64-bit counters, index = counter & (ring size - 1)). Allocations take
// from the head but only below the PUBLISHED tail, which k_trace2 advances once per pass
// (kernel boundaries order the frees' ring writes before the next pass's reads). A wave
// allocates from its own ring; an allocation that finds no published block there parks
// its slot for one pass (PARK_BIT). Paths that hold a block never wait, so parked slots
// always get one back.
IZPI_DEV unsigned long long* pool_ring_ctr(const ShadeParams& sp, uint32_t r) {
  return sp.pool_ctr + (size_t)r * POOL_CTR_STRIDE;
}
// Wave-aggregated allocation for the lanes with `need`: returns 1 + block, or 0 (`need`
// lanes with 0 are parked).
IZPI_DEV uint32_t pool_alloc(const ShadeParams& sp, bool need) {
  const uint64_t m = __ballot(need);
  if (m == 0) return 0;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t ring = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (POOL_SHARDS - 1);
  unsigned long long* c = pool_ring_ctr(sp, ring);
  const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1;
  unsigned long long base = 0, pub = 0;
  if (lane == leader) {
    base = atomicAdd(c, (unsigned long long)__popcll(m));
    pub = __atomic_load_n(c + 2, __ATOMIC_RELAXED);
  }
  base = __shfl(base, (int)leader);
  pub = __shfl(pub, (int)leader);
  const unsigned long long idx = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1));
  const uint32_t size_mask = (1u << sp.pool_shift) - 1u;
  return (need && idx < pub) ? sp.pool_ring[((size_t)ring << sp.pool_shift) + (idx & size_mask)] + 1u : 0u;
}
// Return a lane's block (1 + block, 0 = none) to its ring.
IZPI_DEV void pool_free_one(const ShadeParams& sp, uint32_t fblk) {
  const uint32_t b = fblk - 1u, ring = b >> sp.pool_shift, size_mask = (1u << sp.pool_shift) - 1u;
  const unsigned long long pos = atomicAdd(pool_ring_ctr(sp, ring) + 1, 1ull);
  sp.pool_ring[((size_t)ring << sp.pool_shift) + (pos & size_mask)] = b;
}
// Single-lane allocation that tries every ring (k_tail: cannot park), or 0.
IZPI_DEV uint32_t pool_alloc_any(const ShadeParams& sp, uint32_t first) {
  const uint32_t size_mask = (1u << sp.pool_shift) - 1u;
  for (uint32_t k = 0; k < POOL_SHARDS; k++) {
    const uint32_t ring = (first + k) & (POOL_SHARDS - 1);
    unsigned long long* c = pool_ring_ctr(sp, ring);
    if (__atomic_load_n(c, __ATOMIC_RELAXED) >= __atomic_load_n(c + 2, __ATOMIC_RELAXED)) continue;  // exhausted
    const unsigned long long idx = atomicAdd(c, 1ull);
    if (idx < __atomic_load_n(c + 2, __ATOMIC_RELAXED)) return sp.pool_ring[((size_t)ring << sp.pool_shift) + (idx & size_mask)] + 1u;
  }
  return 0u;
}

// Deferred unwinding. A path that ends in a shading pass is unwound (finish) from its
// records, depth - 1 down to 0; done in the finishing lane itself, a wave waits for its
// deepest finishing lane while its other lanes idle (C5: finish took 48% of k_shade's
// wave cycles with a few lanes of a wave finishing per iteration). Instead the finishing
// lane queues a job in its block's queue, and the block unwinds the queued jobs with every
// lane busy once FINQ_FLUSH are queued (and at the end of the launch). The records stay
// put until then: the slot's next path writes its first record in the NEXT pass, after
// its first ray is traced, and the finished path's overflow block is freed by fin_flush.
// A job: unit | rslot << 32, blk | (depth | zf << 16) << 32, then the terminal radiance
// (Colour) or L.x, lambda, lpdf (Spectral), word-major (word k of job j at k * FINQ_CAP + j).
template <int SAMPLER>
IZPI_DEV void fin_queue(unsigned long long* q, uint32_t j, const PathSt& P, const RayRec& R) {
  const bool colour = SAMPLER == IZPI_SAMPLER_COLOUR;
  q[j] = P.unit | (unsigned long long)P.rslot << 32;
  q[FINQ_CAP + j] = P.blk | (unsigned long long)(P.depth | P.zf << 16) << 32;
  q[2 * FINQ_CAP + j] = (unsigned long long)__double_as_longlong(R.o[0]);
  q[3 * FINQ_CAP + j] = (unsigned long long)__double_as_longlong(colour ? R.o[1] : P.lambda);
  q[4 * FINQ_CAP + j] = (unsigned long long)__double_as_longlong(colour ? R.o[2] : P.lpdf);
}
template <int SAMPLER, int MATSET>
IZPI_DEV void fin_flush(const ShadeParams& sp, const unsigned long long* q, uint32_t n) {
  const bool colour = SAMPLER == IZPI_SAMPLER_COLOUR;
  for (uint32_t j = threadIdx.x; j < n; j += SHADE_THREADS) {
    PathSt P;
    const unsigned long long w0 = q[j], w1 = q[FINQ_CAP + j];
    P.unit = (uint32_t)w0; P.rslot = (uint32_t)(w0 >> 32);
    P.blk = (uint32_t)w1; P.depth = (uint32_t)(w1 >> 32) & 0xFFFFu; P.zf = (uint32_t)(w1 >> 48);
    const double a = __longlong_as_double((long long)q[2 * FINQ_CAP + j]);
    const double b = __longlong_as_double((long long)q[3 * FINQ_CAP + j]);
    const double c = __longlong_as_double((long long)q[4 * FINQ_CAP + j]);
    P.lambda = colour ? 0.0 : b; P.lpdf = colour ? 0.0 : c;
    finish<SAMPLER, MATSET>(sp, P, colour ? mk(a, b, c) : mk(a, 0.0, 0.0));
    if (sp.rec_pool && P.blk) pool_free_one(sp, P.blk);
  }
}
// Which k_shade instances defer: 1 = the Spectral ones and the Colour ones with specular
// materials (C5 at 32 spp: shading 377 -> 320 ms; C4, queueing only the unwindings that
// read records: 464.7 -> 453.7 ms), not C1-C3's Lambert-only instances (C3 +3.4% even
// with only the record-reading unwindings queued: they are short, and the queue costs
// stores), 2 = all, 0 = none. Handing each wave's lanes jobs of similar depth (a counting
// sort of a flush's jobs by depth) measured slower: C5 338 ms, C4 +1.4%.

// One shading pass over the slots traced in the previous k_trace.
// k_shade's register budget: 3 waves per SIMD (168 VGPRs). MATSET_BASIC colour at 4 waves spilled
// 47 VGPRs and measured 1% slower; the spectral / MATSET_FULL instances ran C5 7% faster at 3
// waves than at 2 despite ~100 B/lane of spill. The forward instances (153-168 VGPRs, no
// spill) at 4 waves spill 24-71 VGPRs: C2 +1.5%, C3 +0.3%, C4 +2.7%, C5 (256 spp) +23%
// (profiles/r6m).
constexpr int SHADE_WPE = 3;
// Forward mode: a finished path frees its entry and starts nothing; k_refill starts the new
// units after the pass (see there). The recursion's new paths take over the finished
// paths' record slots, here.
// STAGE: the staged form of the forward Colour instances (stage_put), chosen per render by
// run_wavefront; its output stage lies behind the Colour tables in the LDS arena. MATSET_BASIC
// and MATSET_SURF have one (165 and 168 VGPRs, no spill); MATSET_FULL's spilled 18 VGPRs
// and is not compiled (its dielectric scenes carry cold records, which the stage lacks).
constexpr bool shade_can_stage(int sampler, int matset, bool fwd) {
  return fwd && sampler == IZPI_SAMPLER_COLOUR && matset != MATSET_FULL;
}
template <int SAMPLER, int MATSET, bool FWD, bool STAGE = false>
__global__ void __launch_bounds__(SHADE_THREADS) __attribute__((amdgpu_waves_per_eu(SHADE_WPE)))
k_shade(const DevScene sc, const ShadeParams sp, const WaveParams wp) {
  static_assert(!STAGE || shade_can_stage(SAMPLER, MATSET, FWD), "no staged form of this instance");
  constexpr bool DREF = FWD;
  shade_stage(sc, sp);
  uint32_t parity = 0;  // block_reserve2 LDS buffer set
  uint32_t st_phase = 0, st_n = 0;  // (STAGE) 1: the stage holds the st_n entries of the iteration before
  const uint32_t n = *wp.in_count;
  // (forward mode) `in`'s camera entries: their path state is computed, not loaded
  const uint32_t cam_b = FWD && wp.cam ? wp.cam[0] : 0u, cam_u = FWD && wp.cam ? wp.cam[1] : 0u,
                 cam_m = FWD && wp.cam ? wp.cam[2] : 0u;
  // this pass's k_trace2 is done with its dequeue cursor: reset it for the next pass's
  if (blockIdx.x == 0 && threadIdx.x == 0) *wp.trace_next = 0;
  bool exhausted = false;  // (thread 0) this block has seen the unit head run out
  uint32_t c_lt = 0, c_ls = 0, c_park = 0;
  const uint32_t stride = gridDim.x * SHADE_THREADS;
  constexpr bool DEFER = !FWD && (SAMPLER == IZPI_SAMPLER_SPECTRAL || ms_spec(MATSET));
  constexpr bool COLOUR_DEFER = DEFER && SAMPLER == IZPI_SAMPLER_COLOUR;  // a subset of the finished paths is queued
  unsigned long long* fq = sp.finq + (size_t)blockIdx.x * FINQ_WORDS * FINQ_CAP;
  uint32_t fq_n = 0;  // jobs in this block's queue (the same in every thread)
#ifdef IZPI_SHADE_CLOCKS
  uint64_t k_item = 0, k_ref = 0, k_push = 0;
  sclk_zero();
#endif
  // Block-uniform trip count: the unit and queue reservations are block-wide.
  for (uint32_t base = blockIdx.x * SHADE_THREADS; base < n; base += stride) {
    const uint32_t i = base + threadIdx.x;
    const bool valid = i < n;
    bool push = false;      // the path has a ray to trace next (P, R)
    bool done = false;      // its sample finished: start a new unit in its record slot
    bool parked = false;
    uint32_t fblk = 0;
#ifdef IZPI_SHADE_CLOCKS
    uint64_t t0 = __builtin_readcyclecounter();
#endif
    PathSt P;
    RayRec R;
    P.rslot = 0; P.blk = 0; P.depth = 0; P.zf = 0;
    uint32_t kind = RAY_DEAD;
    EntryIn E;
    if (valid) {
      // the kind word, path state, ray and hit record in one round of loads (a dead entry's
      // path and hit are read too, and ignored): waiting for the kind word first, then the
      // path, then the ray put three memory round trips in front of every item
      kind = sld(wp.in.kind + i) & ~(uint32_t)RAY_PARKED;  // a parked entry retries its pass
      if (FWD && i - cam_b < cam_m) camera_path<SAMPLER>(sp, cam_u + (i - cam_b), P);
      else load_path<SAMPLER, FWD>(wp.in, i, P);
      load_entry(wp.in, i, E);
    }
    const bool live = valid && !(kind & RAY_DEAD);
    if (sp.rec_pool) {  // a path at depth >= rec_dense writes its records to an overflow block
      const bool need = live && P.depth >= sp.rec_dense && P.blk == 0;
      const uint32_t b = pool_alloc(sp, need);
      P.blk = need ? b : P.blk;
      parked = need && b == 0;
      c_park += parked ? 1u : 0u;
    }
    bool queued = false;    // (DEFER) its unwinding waits in the block's queue
    if (live && !parked) shade_item<SAMPLER, MATSET, DEFER, FWD>(sc, sp, wp.in, i, kind, E, P, R, push, done, fblk, c_lt, c_ls, queued);
    if (SAMPLER == IZPI_SAMPLER_SPECTRAL) queued = DEFER && done;  // (every finished path)
    // a queued path's overflow block is freed after its unwinding (fin_flush)
    if ((COLOUR_DEFER ? !queued : !DEFER) && sp.rec_pool && fblk) pool_free_one(sp, fblk);
#ifdef IZPI_SHADE_CLOCKS
    uint64_t t1 = __builtin_readcyclecounter();
    k_item += t1 - t0;
    t0 = t1;
#endif
    // one reservation phase: output entries for continuing and parked paths, new units
    // (and their entries) for finished ones
    uint32_t unit = 0xFFFFFFFFu, pos = 0xFFFFFFFFu, frank = 0, ftotal = 0;
    if constexpr (STAGE) {  // (no pool: nothing parks; no unit or unwinding job is taken here)
      if (st_phase == 0) {  // block-uniform
        st_n = stage_put(push, P, R);
      } else {
        uint32_t rbase, rank;
        block_reserve_fwd(wp.out_count, push, st_n, rbase, rank);
        if (push) store_entry<SAMPLER, FWD>(wp.out, rbase + st_n + rank, P, R);
        stage_flush(wp.out, rbase, st_n);
      }
      st_phase ^= 1u;
    } else {
      block_reserve2<COLOUR_DEFER>(sp, wp.out_count, push || parked, done && !DREF, unit, pos, parity, exhausted, queued, frank,
                                   ftotal);
      if (queued) fin_queue<SAMPLER>(fq, fq_n + frank, P, R);  // (before refill_one reuses P)
      fq_n += ftotal;
      if (push) store_entry<SAMPLER, FWD>(wp.out, pos, P, R);
      if (parked) copy_entry(wp.in, i, wp.out, pos);
    }
#ifdef IZPI_SHADE_CLOCKS
    t1 = __builtin_readcyclecounter();
    k_push += t1 - t0;
    t0 = t1;
#endif
    if constexpr (!DREF) {
      if (unit != 0xFFFFFFFFu) refill_one<SAMPLER, FWD>(sc, sp, wp.out, unit, pos, P);
      else if (done && pos != 0xFFFFFFFFu) dead_entry(wp.out, pos);  // entry reserved, the units ran out
    }
#ifdef IZPI_SHADE_CLOCKS
    t1 = __builtin_readcyclecounter();
    k_ref += t1 - t0;
#endif
    if (DEFER && fq_n >= FINQ_FLUSH) {  // (block-uniform; the next iteration's jobs wait for its reservation's barriers)
      __syncthreads();
      fin_flush<SAMPLER, MATSET>(sp, fq, fq_n);
      fq_n = 0;
    }
  }
  if (DEFER && fq_n) {
    __syncthreads();
    fin_flush<SAMPLER, MATSET>(sp, fq, fq_n);
  }
  if constexpr (STAGE) {
    if (st_phase) {  // an odd trip count: the last iteration's entries are still staged
      uint32_t rbase, rank;
      block_reserve_fwd(wp.out_count, false, st_n, rbase, rank);
      stage_flush(wp.out, rbase, st_n);
    }
  }
  const uint32_t lane = threadIdx.x & 63;
#ifdef IZPI_SHADE_CLOCKS
  if (lane == 0) {
    atomicAdd(sp.counters + CNT_SCLK_ITEM, (unsigned long long)k_item);
    atomicAdd(sp.counters + CNT_SCLK_REFILL, (unsigned long long)k_ref);
    atomicAdd(sp.counters + CNT_SCLK_PUSH, (unsigned long long)k_push);
  }
  sclk_flush(sp.counters);
#endif
  if (c_park && wp.out_park) *wp.out_park = 1u;  // the next k_trace2 must read kind words
  unsigned long long vals[3] = {c_lt, c_ls, c_park};
  const int idx[3] = {CNT_LTRI, CNT_LSPH, CNT_PARK};
  for (int k = 0; k < 3; k++) {
    unsigned long long s = vals[k];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (lane == 0) count_add(sp.cpart, sp.counters, idx[k], s);
  }
}

// Forward mode's refill: after a shading pass, the entries its finished paths freed take the next
// units: unit plan[1] + j starts in entry plan[0] + j (the plan: k_refill_plan, wavefront.hip).
template <int SAMPLER>
__global__ void __launch_bounds__(256) k_refill(const DevScene sc, const ShadeParams sp_in, const WaveParams wp, const uint32_t* plan) {
  ShadeParams sp = sp_in;
  sp.staged = 0;  // (no tables staged, as k_start)
  sp.prims_staged = 0;
  const uint32_t nc = plan[0], u0 = plan[1], m = plan[2], gap0 = plan[3];
  if (blockIdx.x == 0 && gap0 + threadIdx.x < nc) dead_entry(wp.out, gap0 + threadIdx.x);  // (the gap: < 256 entries)
  for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
    PathSt P;
    RayRec R;
    P.rslot = 0;  // (forward mode: no records)
    if (start_path<SAMPLER, true>(sc, sp, u0 + j, P, R)) store_camera_entry(wp.out, nc + j, R);  // (camera_path)
    else dead_entry(wp.out, nc + j);
  }
}

// The wavefront's tail. Once every work unit has started and few paths remain, the
// pass-synchronous loop pays, per pass, the latency of that pass's longest traversal.
// k_tail instead runs each remaining path to its end in one lane: trace, shade, trace...
// (no refill: the unit head is exhausted), so the passes of different paths overlap.
// Same per-ray code paths, results and counters as k_trace + k_shade.
template <int SAMPLER, int MATSET, int STACK, bool FWD>
__global__ void __launch_bounds__(256) k_tail(const DevScene sc, const ShadeParams sp, const WaveParams wp, int32_t* spill) {
  shade_stage(sc, sp);
  __shared__ int32_t lds_stack[std::min(STACK, TAIL_LDS_STACK) * 256];
  int32_t* stk = lds_stack + threadIdx.x;
  const uint32_t gstride = gridDim.x * 256;
  int32_t* gsp = spill + blockIdx.x * 256 + threadIdx.x;
  const uint32_t n = *wp.in_count;
  const uint32_t cam_b = FWD && wp.cam ? wp.cam[0] : 0u, cam_u = FWD && wp.cam ? wp.cam[1] : 0u,
                 cam_m = FWD && wp.cam ? wp.cam[2] : 0u;
  uint32_t c_rays = 0, c_nodes = 0, c_tri = 0, c_sph = 0, c_lt = 0, c_ls = 0;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    // entry i runs to its end in this lane; its next ray goes back to entry i
    if (wp.in.kind[i] & RAY_DEAD) continue;
    bool traced = (wp.in.kind[i] & RAY_PARKED) != 0;  // a parked entry's ray is already traced
    bool cam = FWD && i - cam_b < cam_m;  // (forward mode) a camera entry's path state is computed once
    for (;;) {
      if (!traced) trace_one<STACK>(sc, wp.in, i, stk, gsp, gstride, c_rays, c_nodes, c_tri, c_sph, sp.error);
      traced = false;
      PathSt P;
      RayRec R;
      if (cam) camera_path<SAMPLER>(sp, cam_u + (i - cam_b), P);
      else load_path<SAMPLER, FWD>(wp.in, i, P);
      cam = false;  // (its next state is stored below)
      const uint32_t kind = wp.in.kind[i] & ~(uint32_t)RAY_PARKED;
      if (sp.rec_pool && P.depth >= sp.rec_dense && P.blk == 0) {
        // The host launches k_tail with at most pool blocks paths, all of the free
        // blocks published, so this cannot fail (guarded anyway: no spin on a bug).
        P.blk = pool_alloc_any(sp, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
        if (P.blk == 0) { atomicOr(sp.error, 4u); break; }
      }
      bool push = false, done = false;
      uint32_t fblk = 0;
      EntryIn E;
      load_entry(wp.in, i, E);
      bool queued = false;  // (k_tail unwinds in place)
      shade_item<SAMPLER, MATSET, false, FWD>(sc, sp, wp.in, i, kind, E, P, R, push, done, fblk, c_lt, c_ls, queued);
      if (fblk) pool_free_one(sp, fblk);
      if (!push) break;
      store_entry<SAMPLER, FWD>(wp.in, i, P, R);
    }
  }
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long vals[9] = {c_rays, c_nodes, c_tri, c_sph, c_lt, c_ls, c_nodes, c_tri, c_sph};
  const int idx[9] = {CNT_RAYS, CNT_NODES, CNT_TRI, CNT_SPH, CNT_LTRI, CNT_LSPH, CNT_TAIL_NODES, CNT_TAIL_TRI, CNT_TAIL_SPH};
#pragma unroll
  for (int k = 0; k < 9; k++) {
    unsigned long long v = vals[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) count_add(sp.cpart, sp.counters, idx[k], v);
  }
}

// The kernels of the instance (SAMPLER, MATSET, FWD) as a table for the pass loop (wavefront.hip).
template <int SAMPLER, int MATSET, bool FWD>
ShadeKernels make_kernels(const char* set_name) {
  ShadeKernels k{};
  k.shade = k_shade<SAMPLER, MATSET, FWD>;
  if constexpr (shade_can_stage(SAMPLER, MATSET, FWD)) k.shade_staged = k_shade<SAMPLER, MATSET, FWD, true>;
  k.tail32 = k_tail<SAMPLER, MATSET, 32, FWD>; k.tail64 = k_tail<SAMPLER, MATSET, 64, FWD>;
  if constexpr (FWD) k.refill = k_refill<SAMPLER>;  // (forward renders start through k_refill: no k_start)
  else k.start = k_start<SAMPLER, FWD>;
  k.sampler = SAMPLER; k.fwd = FWD; k.matset = MATSET; k.rec_doubles = RecLayout<SAMPLER, MATSET>::D;
  snprintf(k.name, sizeof(k.name), "%s/%s/%s", SAMPLER == IZPI_SAMPLER_COLOUR ? "colour" : "spectral", FWD ? "fwd" : "rec", set_name);
  return k;
}
// The instances of (SAMPLER, FWD), by material set (izpi_kern.h: shade_kernels). The compact
// records of MATSET_CONST are the recursion's; the forward form has none.
template <int SAMPLER, bool FWD>
const ShadeKernels* shade_kernels(int matset) {
  static const ShadeKernels basic = make_kernels<SAMPLER, MATSET_BASIC, FWD>("BASIC"),
                            surf = make_kernels<SAMPLER, MATSET_SURF, FWD>("SURF"),
                            full = make_kernels<SAMPLER, MATSET_FULL, FWD>("FULL");
  if constexpr (SAMPLER == IZPI_SAMPLER_COLOUR && !FWD) {
    static const ShadeKernels compact = make_kernels<SAMPLER, MATSET_CONST, FWD>("CONST");
    if (matset == MATSET_CONST) return &compact;
  }
  return matset == MATSET_BASIC ? &basic : matset == MATSET_SURF ? &surf : matset == MATSET_FULL ? &full : nullptr;
}
