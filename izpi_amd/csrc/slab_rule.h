// slab_rule.h — RayAABB4 (bvh4_simd_generic.go) per slot: the scalar twin `slab`, and the sorted
// rule k_trace2's global-memory node step runs for a `fast` ray, which picks each axis's near and
// far plane by the sign of the ray's inverse direction instead of sorting the two products. One
// source for the kernels (izpi_dev.h) and the host (tests/slab_rule_check.cpp). Plain C++ when no
// HIP compiler is present, __host__ __device__ under hipcc, as pixel_map.h; the units are built
// with -ffp-contract=off.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define IZPI_SR __host__ __device__ __forceinline__
#else
#define IZPI_SR inline
#endif

namespace izd {

// Comparisons written as the scalar twin's select form: never fminf/fmaxf (A14).
IZPI_SR float max32(float a, float b) { return a > b ? a : b; }
IZPI_SR float min32(float a, float b) { return a < b ? a : b; }
IZPI_SR bool slab(float mnx, float mny, float mnz, float mxx, float mxy, float mxz, float ox, float oy, float oz,
                  float ix, float iy, float iz, float tmax) {
  float t0x = (mnx - ox) * ix, t1x = (mxx - ox) * ix;
  if (t0x > t1x) { float t = t0x; t0x = t1x; t1x = t; }
  float t0y = (mny - oy) * iy, t1y = (mxy - oy) * iy;
  if (t0y > t1y) { float t = t0y; t0y = t1y; t1y = t; }
  float t0z = (mnz - oz) * iz, t1z = (mxz - oz) * iz;
  if (t0z > t1z) { float t = t0z; t0z = t1z; t1z = t; }
  float tn = max32(max32(t0x, t0y), t0z);
  float tf = min32(min32(t1x, t1y), t1z);
  return tn <= tf && tf >= 0 && tn <= tmax;
}

// The f32 ray for which no t value of a NaN-free box can be NaN: finite origin, finite and
// non-zero inverse direction.
IZPI_SR bool ray_fast_ok(float ox, float oy, float oz, float ix, float iy, float iz) {
  const float inf = __builtin_huge_valf();
  return __builtin_fabsf(ox) < inf && __builtin_fabsf(oy) < inf && __builtin_fabsf(oz) < inf &&
         __builtin_fabsf(ix) < inf && __builtin_fabsf(iy) < inf && __builtin_fabsf(iz) < inf &&
         ix != 0.0f && iy != 0.0f && iz != 0.0f;
}

// The six bounds of a box in GInner's order: mnx 0, mny 1, mnz 2, mxx 3, mxy 4, mxz 5. A fast
// ray's near plane on `axis` is the box's maximum when it travels down the axis; every other
// ray keeps the canonical order (its planes then reach `slab` as mn and mx). The far plane is the
// other one of the pair.
IZPI_SR uint32_t slab_near_index(uint32_t axis, float inv, bool fast) { return axis + ((fast && inv < 0.0f) ? 3u : 0u); }
IZPI_SR uint32_t slab_far_index(uint32_t axis, uint32_t near) { return 3u + 2u * axis - near; }

// The sorted rule on the six products (plane - o) * inv of a fast ray and a box with mn <= mx on
// every axis. Rounded subtraction and multiplication by a value of fixed sign are monotone, so the
// near plane's product is the smaller of the axis's two: what `slab` has after its swap, up to
// the sign of a zero, which no comparison sees. No product is NaN, so the twin's max32 / min32
// are IEEE max / min; the three compares are the twin's own (tmax may be anything).
IZPI_SR float slab_sorted_near(float nx, float ny, float nz) { return __builtin_fmaxf(__builtin_fmaxf(nx, ny), nz); }
IZPI_SR float slab_sorted_far(float fx, float fy, float fz) { return __builtin_fminf(__builtin_fminf(fx, fy), fz); }
IZPI_SR bool slab_sorted_hit(float nx, float ny, float nz, float fx, float fy, float fz, float tmax) {
  const float tn = slab_sorted_near(nx, ny, nz), tf = slab_sorted_far(fx, fy, fz);
  return tn <= tf && tf >= 0 && tn <= tmax;
}
// b: the box's six bounds in GInner's order.
IZPI_SR bool slab_sorted(const float* b, uint32_t nx, uint32_t ny, uint32_t nz, float ox, float oy, float oz, float ix,
                         float iy, float iz, float tmax) {
  return slab_sorted_hit((b[nx] - ox) * ix, (b[ny] - oy) * iy, (b[nz] - oz) * iz, (b[slab_far_index(0, nx)] - ox) * ix,
                         (b[slab_far_index(1, ny)] - oy) * iy, (b[slab_far_index(2, nz)] - oz) * iz, tmax);
}

}  // namespace izd
