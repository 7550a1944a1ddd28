// izpi_dev.h — device-side data layouts and per-lane primitives of the gfx950
// path-tracing inner loop. Included by every kernel source through izpi_kern.h. The scene's
// records, which the host packer shares, are in scene_records.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/izpi_gpu.h"
#include "gomath.h"
#include "scene_records.h"
#include "slab_rule.h"

#define IZPI_DEV __device__ __forceinline__

namespace izd {

// The scene as the kernels read it (izpi_gpu_upload_scene). The small tables k_shade / k_tail
// stage per block in LDS are laid out by izpi_kern.h's lds_off (compile-time offsets; a
// render sizes the arena to the prefix it stages, lds_bytes).
struct DevScene {
  const GInner* inner;
  const GInnerQ* innerq;        // the same nodes quantised (DevScene::quantized), else null
  const GLeaf* leaves;
  const GPrim* prims;
  const GShade* shade;          // [num_prims], leaf order
  const GTriTex* tritex;        // [num_prims], leaf order: triangle UVs and tangent frame (textured scenes only, else null)
  const GLight* lights;
  const izpi_material* materials;
  const izpi_texture* textures;
  const double4* mat_const;     // per material: its constant RGB albedo / emit texture value (GShade cflags bit0)
  const MatTex* mat_tex;        // per material: its RGB texture slots
  const double* texels;
  const double* spd_wl;
  const double* spd_val;
  int32_t root;                 // encoded ref of BVH4.Nodes[0]; -1 when empty
  uint32_t num_lights;
  uint32_t nan_free_bounds;     // no NaN in any inner-node bound: slab4_fast allowed
  uint32_t leaf_shortcut;       // every leaf's slot-0 box equals its parent slot's box
  uint32_t tri_only;            // no spheres: leaf tests may be spread over the wave
  uint32_t no_pathlen;          // no dielectric material: every traced ray is a sampler ray (RAY_MAIN)
  uint32_t num_inner;           // GInner records
  uint32_t num_prims;           // GPrim records (and GLeaf slots, indexed by first primitive)
  izpi_camera cam;
  uint32_t lds_bytes;           // per render (render_body): k_shade / k_tail's dynamic LDS arena (lds_off)
  uint32_t time_free;           // no sphere moves: traversal needs no ray times (upload)
  uint32_t quantized;           // IZPI_SCENE_QUANTIZED_BVH: `inner` holds the decoded boxes of `innerq`
  uint32_t addr32;              // inner, innerq and leaves are one block under 4 GiB, as are prims (trace_addr32):
                                // k_trace2 addresses their records by 32-bit byte offsets (fills the struct's tail padding)
  uint32_t leaf_max;            // the largest primitive count of a leaf, 0 for an empty scene (make_tracer: at most 3, as
                                // the GPU builder's trees have, picks the primitive step sized for three)
  uint32_t ordered_bounds;      // mn <= mx on every axis of every valid slot and leaf box: with nan_free_bounds,
                                // k_trace2 picks a fast ray's near and far planes by its sign (slab4_sorted; fills the tail padding)
#ifdef IZPI_SHADOW
  // measurement builds only (byte breakdown): copies of the traversal arrays that
  // k_trace2 reads beside the real ones, so a class's bytes past L2 show as extra FETCH_SIZE
  const GInner* sh_inner;
  const GLeaf* sh_leaves;
  const GPrim* sh_prims;
#endif
};

struct RenderParams {
  uint32_t width, height, spp, max_depth;
  uint32_t chunk_spp;       // samples per pixel in this launch
  uint32_t s0;              // first sample index of this launch
  uint32_t num_pixels;      // pixels in the request
  uint32_t tile_w, tile_h;  // all tiles equal-sized
  uint32_t total_units;     // num_pixels * chunk_spp
  uint32_t lanes;           // gridDim.x * blockDim.x
  uint32_t num_bg_spd;
  const uint32_t* tiles;    // [n][4]
  const double* bg_wl;
  const double* bg_val;
  double background[3];
  uint64_t seed;
  double* out;              // [total_units][3] per-sample result
  double* recs;             // [max_depth][6][lanes] unwinding records
  uint32_t* head;           // work queue head
  unsigned long long* counters;  // 6 counters
  uint32_t* error;          // device-side guard flag
};

// ---------------------------------------------------------------- RNG
// fastrandom.LCG (fastrandom.go:41-47): state = (a*state + c) mod 2^32 — with a
// 64-bit seed the first step already reduces mod 2^32, so a uint32 state is exact.
struct Lcg {
  uint32_t s;
  IZPI_DEV double next() {
    s = 1664525u * s + 1013904223u;
    return (double)s / 4294967296.0;
  }
};
IZPI_DEV uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
#define IZPI_CAMERA_STREAM_SALT 0xD6E8FEB86659FD93ull

// Go int(float64) on amd64 (CVTTSD2SQ): NaN / out of range -> INT64_MIN.
IZPI_DEV int64_t go_int(double x) {
  if (x != x || x >= 9223372036854775808.0 || x < -9223372036854775808.0) return INT64_MIN;
  return (int64_t)x;
}

// ------------------------------------------------------------- vec3
struct V3 { double x, y, z; };
IZPI_DEV V3 mk(double x, double y, double z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
IZPI_DEV V3 ld3(const double* p) { return mk(p[0], p[1], p[2]); }
IZPI_DEV V3 add(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
IZPI_DEV V3 sub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
IZPI_DEV V3 mul(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
IZPI_DEV V3 smul(V3 a, double t) { return mk(a.x * t, a.y * t, a.z * t); }
// a / t per component, correctly rounded as `/`. gfx950's f64 division is v_div_scale (x2),
// v_rcp, a Newton refinement of the reciprocal that depends on the divisor only, then
// mul, fma, v_div_fmas, v_div_fixup per dividend. When no operand needs v_div_scale's
// rescaling (divisor and dividends within 2^+-300, dividends also +-0: v_div_fixup
// alone settles a zero dividend), that is the same sequence with the scales the
// identity, so one refined reciprocal serves the three dividends: 18 instructions
// instead of 36, bit for bit the three divisions (test_sdiv_shared_reciprocal_bitwise).
IZPI_DEV bool sdiv_plain(double x) {  // exponent within 2^+-300
  return ((uint32_t)(__double2hiint(x) >> 20) & 0x7FFu) - (1023u - 300u) <= 600u;
}
IZPI_DEV V3 sdiv(V3 a, double t) {
  // (bitwise: one test, no branches)
  const int px = (int)sdiv_plain(a.x) | (int)(a.x == 0.0), py = (int)sdiv_plain(a.y) | (int)(a.y == 0.0),
            pz = (int)sdiv_plain(a.z) | (int)(a.z == 0.0);
  const bool plain = ((int)sdiv_plain(t) & px & py & pz) != 0;
  if (plain) {
    double r = __builtin_amdgcn_rcp(t);
    double e = __builtin_fma(-t, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-t, r, 1.0);
    r = __builtin_fma(r, e, r);
    auto q1 = [&](double n) {
      const double q = n * r;
      const double res = __builtin_fma(-t, q, n);
      return __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(res, r, q, false), t, n);
    };
    return mk(q1(a.x), q1(a.y), q1(a.z));
  }
  return mk(a.x / t, a.y / t, a.z / t);
}
IZPI_DEV double dot(V3 a, V3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }
IZPI_DEV V3 cross(V3 a, V3 b) { return mk((a.y * b.z) - (a.z * b.y), -((a.x * b.z) - (a.z * b.x)), (a.x * b.y) - (a.y * b.x)); }
IZPI_DEV double sqlen(V3 a) { return (a.x * a.x) + (a.y * a.y) + (a.z * a.z); }
IZPI_DEV double length(V3 a) { return gm::sqrt(sqlen(a)); }
IZPI_DEV V3 unit(V3 a) { return sdiv(a, length(a)); }
IZPI_DEV V3 lerp(V3 a, V3 b, double t) {
  return mk((1 - t) * a.x + t * b.x, (1 - t) * a.y + t * b.y, (1 - t) * a.z + t * b.z);
}
IZPI_DEV bool bad(double x) { return x != x || gm::is_inf(x, 0); }
IZPI_DEV V3 denan(V3 v) { return mk(bad(v.x) ? 0.0 : v.x, bad(v.y) ? 0.0 : v.y, bad(v.z) ? 0.0 : v.z); }

// onb.go:38-67
struct Onb {
  V3 u, v, w;
  IZPI_DEV void build(V3 n) {
    w = unit(n);
    V3 a = gm::abs(w.x) > 0.9 ? mk(0, 1, 0) : mk(1, 0, 0);
    v = unit(cross(w, a));
    u = cross(w, v);
  }
  IZPI_DEV V3 local(V3 a) const { return add(add(smul(u, a.x), smul(v, a.y)), smul(w, a.z)); }
};

// vec3.go:119-138
IZPI_DEV V3 random_cosine_direction(Lcg& r) {
  double r1 = r.next();
  double r2 = r.next();
  double z = gm::sqrt(1 - r2);
  double phi = 6.283185307179586 * r1;   // 2*math.Pi folded by the Go compiler
  double sp, cp;
  gm::sincos_nonneg(phi, &sp, &cp);      // = gm::sin(phi), gm::cos(phi): phi in [0, 2 Pi)
  double x = cp * 2 * gm::sqrt(r2);
  double y = sp * 2 * gm::sqrt(r2);
  return mk(x, y, z);
}
IZPI_DEV V3 random_to_sphere(double radius, double dist2, Lcg& r) {
  double r1 = r.next();
  double r2 = r.next();
  double z = 1 + r2 * (gm::sqrt(1 - radius * radius / dist2) - 1);
  double phi = 6.283185307179586 * r1;
  double sp, cp;
  gm::sincos_nonneg(phi, &sp, &cp);
  double x = cp * gm::sqrt(1 - z * z);
  double y = sp * gm::sqrt(1 - z * z);
  return mk(x, y, z);
}
// material.go:10-18
IZPI_DEV V3 random_in_unit_sphere(Lcg& r) {
  for (;;) {
    double x = r.next(), y = r.next(), z = r.next();
    V3 p = sub(smul(mk(x, y, z), 2.0), mk(1.0, 1.0, 1.0));
    if (sqlen(p) < 1.0) return p;
  }
}

// --------------------------------------------------- RayAABB4 (bvh4_simd_generic.go)
// The scalar twin `slab`, ray_fast_ok and the per-slot sorted rule are in slab_rule.h.

// RayAABB4 over the 4 slots of an inner node, NaN-free fast form. When the ray's f32
// origin is finite and its f32 inverse direction is finite and non-zero on every axis,
// and the node bounds hold no NaN (checked once at upload), no t value can be NaN, so
// the scalar twin's swap / max32 / min32 reduce to IEEE min/max (they can differ only in
// the sign of a zero, which no comparison below sees): the mask is bit-identical.
// The subtract and multiply run as packed f32 pairs (children 0-1 and 2-3), min3/max3
// fold the three axes.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// The result is four wave masks (bit l of h[i]: lane l hits slot i; inactive lanes 0), not a
// bit field per lane: each compare already leaves a lane mask, its ballot is that mask, and the
// caller combines masks on the scalar unit. (The ballot of a conjunction is built the long way,
// through a 0 / 1 register and a second compare: hence one ballot per compare.)
IZPI_DEV void slab4_fast(float4 mnx, float4 mny, float4 mnz, float4 mxx, float4 mxy, float4 mxz, float ox, float oy,
                         float oz, float ix, float iy, float iz, float tmax, uint64_t (&h)[4]) {
  const f32x2 o_x = {ox, ox}, o_y = {oy, oy}, o_z = {oz, oz};
  const f32x2 i_x = {ix, ix}, i_y = {iy, iy}, i_z = {iz, iz};
  const f32x2 a0x = (f32x2{mnx.x, mnx.y} - o_x) * i_x, a1x = (f32x2{mnx.z, mnx.w} - o_x) * i_x;
  const f32x2 b0x = (f32x2{mxx.x, mxx.y} - o_x) * i_x, b1x = (f32x2{mxx.z, mxx.w} - o_x) * i_x;
  const f32x2 a0y = (f32x2{mny.x, mny.y} - o_y) * i_y, a1y = (f32x2{mny.z, mny.w} - o_y) * i_y;
  const f32x2 b0y = (f32x2{mxy.x, mxy.y} - o_y) * i_y, b1y = (f32x2{mxy.z, mxy.w} - o_y) * i_y;
  const f32x2 a0z = (f32x2{mnz.x, mnz.y} - o_z) * i_z, a1z = (f32x2{mnz.z, mnz.w} - o_z) * i_z;
  const f32x2 b0z = (f32x2{mxz.x, mxz.y} - o_z) * i_z, b1z = (f32x2{mxz.z, mxz.w} - o_z) * i_z;
  const float t0x[4] = {a0x.x, a0x.y, a1x.x, a1x.y}, t1x[4] = {b0x.x, b0x.y, b1x.x, b1x.y};
  const float t0y[4] = {a0y.x, a0y.y, a1y.x, a1y.y}, t1y[4] = {b0y.x, b0y.y, b1y.x, b1y.y};
  const float t0z[4] = {a0z.x, a0z.y, a1z.x, a1z.y}, t1z[4] = {b0z.x, b0z.y, b1z.x, b1z.y};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(t0x[i], t1x[i]), __builtin_fminf(t0y[i], t1y[i])),
                                     __builtin_fminf(t0z[i], t1z[i]));
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(t0x[i], t1x[i]), __builtin_fmaxf(t0y[i], t1y[i])),
                                     __builtin_fmaxf(t0z[i], t1z[i]));
    h[i] = __builtin_amdgcn_ballot_w64(tn <= tf) & __builtin_amdgcn_ballot_w64(tf >= 0.0f) & __builtin_amdgcn_ballot_w64(tn <= tmax);
  }
}
// The same test for the planes already chosen by the ray's sign (slab_rule.h: near / far hold, per
// slot, the near and far plane of each axis): no sort of the two products. Exact for a fast ray
// (ray_fast_ok) on NaN-free bounds with mn <= mx (DevScene::ordered_bounds). The three compares are
// slab_sorted_hit's, each with a ballot of its own, as in slab4_fast.
IZPI_DEV void slab4_sorted(float4 nrx, float4 nry, float4 nrz, float4 frx, float4 fry, float4 frz, float ox, float oy,
                           float oz, float ix, float iy, float iz, float tmax, uint64_t (&h)[4]) {
  const f32x2 o_x = {ox, ox}, o_y = {oy, oy}, o_z = {oz, oz};
  const f32x2 i_x = {ix, ix}, i_y = {iy, iy}, i_z = {iz, iz};
  const f32x2 a0x = (f32x2{nrx.x, nrx.y} - o_x) * i_x, a1x = (f32x2{nrx.z, nrx.w} - o_x) * i_x;
  const f32x2 b0x = (f32x2{frx.x, frx.y} - o_x) * i_x, b1x = (f32x2{frx.z, frx.w} - o_x) * i_x;
  const f32x2 a0y = (f32x2{nry.x, nry.y} - o_y) * i_y, a1y = (f32x2{nry.z, nry.w} - o_y) * i_y;
  const f32x2 b0y = (f32x2{fry.x, fry.y} - o_y) * i_y, b1y = (f32x2{fry.z, fry.w} - o_y) * i_y;
  const f32x2 a0z = (f32x2{nrz.x, nrz.y} - o_z) * i_z, a1z = (f32x2{nrz.z, nrz.w} - o_z) * i_z;
  const f32x2 b0z = (f32x2{frz.x, frz.y} - o_z) * i_z, b1z = (f32x2{frz.z, frz.w} - o_z) * i_z;
  const float nx[4] = {a0x.x, a0x.y, a1x.x, a1x.y}, fx[4] = {b0x.x, b0x.y, b1x.x, b1x.y};
  const float ny[4] = {a0y.x, a0y.y, a1y.x, a1y.y}, fy[4] = {b0y.x, b0y.y, b1y.x, b1y.y};
  const float nz[4] = {a0z.x, a0z.y, a1z.x, a1z.y}, fz[4] = {b0z.x, b0z.y, b1z.x, b1z.y};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float tn = slab_sorted_near(nx[i], ny[i], nz[i]), tf = slab_sorted_far(fx[i], fy[i], fz[i]);
    h[i] = __builtin_amdgcn_ballot_w64(tn <= tf) & __builtin_amdgcn_ballot_w64(tf >= 0.0f) & __builtin_amdgcn_ballot_w64(tn <= tmax);
  }
}

// ----------------------------------------------------- primitive tests
// Möller–Trumbore acceptance of Triangle.Hit (triangle.go:193-221).
IZPI_DEV bool tri_intersect(const double* a, V3 o, V3 d, double tmin, double tmax, double& t, double& u, double& v) {
  const double eps = 1e-8;
  V3 v0 = mk(a[0], a[1], a[2]), e1 = mk(a[3], a[4], a[5]), e2 = mk(a[6], a[7], a[8]);
  V3 h = cross(d, e2);
  double aa = dot(e1, h);
  if (gm::abs(aa) < eps) return false;
  double f = 1.0 / aa;
  V3 s = sub(o, v0);
  u = f * dot(s, h);
  if (u < -eps || u > 1.0 + eps) return false;
  V3 q = cross(s, e1);
  v = f * dot(d, q);
  if (v < -eps || u + v > 1.0 + eps) return false;
  t = f * dot(e2, q);
  if (t < tmin || t > tmax) return false;
  return true;
}
// The same test without the final `t > tMax` rejection: that last comparison is the
// only one that depends on tMax, so tests of one leaf can run in parallel and be
// accepted afterwards in primitive order against the running tMax (bit-identical).
// It has no early returns: every product is computed and the four rejections are combined at
// the end. A lane that passes runs tri_intersect's operations on the same operands, and a lane
// that fails returns false whatever its later values are (a zero determinant only makes them
// infinite or NaN). In a wave of up to 64 tests some lane passes each rejection nearly always,
// so an early return skips nothing; but each one is a divergent branch, and the compiler sinks
// the loads of v0 behind the first, a second dependent round trip to memory in every step.
IZPI_DEV bool tri_intersect_no_tmax(const double* a, V3 o, V3 d, double tmin, double& t, double& u, double& v) {
  const double eps = 1e-8;
  V3 v0 = mk(a[0], a[1], a[2]), e1 = mk(a[3], a[4], a[5]), e2 = mk(a[6], a[7], a[8]);
  V3 h = cross(d, e2);
  double aa = dot(e1, h);
  double f = 1.0 / aa;
  V3 s = sub(o, v0);
  u = f * dot(s, h);
  V3 q = cross(s, e1);
  v = f * dot(d, q);
  t = f * dot(e2, q);
  const bool r0 = gm::abs(aa) < eps, r1 = (u < -eps) | (u > 1.0 + eps), r2 = (v < -eps) | (u + v > 1.0 + eps), r3 = t < tmin;
  return !(r0 | r1 | r2 | r3);
}
// Sphere.center (sphere.go:495-497)
IZPI_DEV V3 sph_center(const double* a, double time) {
  V3 c0 = mk(a[0], a[1], a[2]), c1 = mk(a[3], a[4], a[5]);
  return add(c0, smul(sub(c1, c0), ((time - a[7]) / (a[8] - a[7]))));
}
// Sphere.Hit acceptance (sphere.go:63-95): root 0 or 1; strict bounds.
IZPI_DEV bool sph_intersect_at(V3 center, double radius, V3 o, V3 d, double tmin, double tmax, double& t, int& root) {
  V3 oc = sub(o, center);
  double aa = dot(d, d);
  double b = dot(oc, d);
  double c = dot(oc, oc) - (radius * radius);
  double disc = (b * b) - (aa * c);
  if (disc > 0) {
    double temp = (-b - gm::sqrt(b * b - aa * c)) / aa;
    if (temp < tmax && temp > tmin) { t = temp; root = 0; return true; }
    temp = (-b + gm::sqrt(b * b - aa * c)) / aa;
    if (temp < tmax && temp > tmin) { t = temp; root = 1; return true; }
  }
  return false;
}
// The two candidate roots of sph_intersect_at, computed without tMax/tMin (the acceptance
// `temp < tMax && temp > tMin`, root 0 first, is applied by the caller).
IZPI_DEV bool sph_roots(V3 center, double radius, V3 o, V3 d, double& t0, double& t1) {
  V3 oc = sub(o, center);
  double aa = dot(d, d);
  double b = dot(oc, d);
  double c = dot(oc, oc) - (radius * radius);
  double disc = (b * b) - (aa * c);
  if (!(disc > 0)) return false;
  t0 = (-b - gm::sqrt(b * b - aa * c)) / aa;
  t1 = (-b + gm::sqrt(b * b - aa * c)) / aa;
  return true;
}
IZPI_DEV bool sph_intersect(const double* a, V3 o, V3 d, double time, double tmin, double tmax, double& t, int& root) {
  return sph_intersect_at(sph_center(a, time), a[6], o, d, tmin, tmax, t, root);
}

}  // namespace izd
