// displace.h — the arithmetic of the DISPLACE geometry operator, shared by the device path
// (displace.hip) and its host twin (displace_host.cpp). Plain C++ when no HIP compiler is
// present, __host__ __device__ under hipcc; both are built with -ffp-contract=off, so every
// expression rounds as Go's does on amd64 (no FMA).
//
//   tessellate            displacement/displacement.go:36-101
//   isTessellatedEnough   displacement/displacement.go:103-141
//   applyDisplacement     displacement/displacement.go:219-280 (vec3.go:18-35,105-111; mat3.go:19-40)
//   ImageTxt.Value        texture/image.go:73-101 (float64 NRGBA branch)
//
// A work item is an izpi_tri_in whose `pad` carries the index of its source triangle; the
// finished triangle is written with pad = 0.
#pragma once
#include <stdint.h>

#include "../../include/izpi_host.h"
#include "gomath.h"

namespace dsp {

// The blue channel of a float64 NRGBA map: texel (i, j) is z[(j * w + i) * stride].
// stride = 4 on the caller's interleaved texels, 1 on a packed copy of the channel.
struct Map {
  const double* z;
  uint32_t w, h, stride;
};

// ApplyDisplacementMap's constants (displacement.go:174-181)
IZPI_HD double max_delta(uint32_t res) { return 4.0 / (double)((int64_t)res - 1); }
#define IZPI_DSP_THRESHOLD 2.0

// Go's int(float64) on amd64 (CVTTSD2SQ): NaN and out-of-range values give INT64_MIN.
IZPI_HD int64_t go_int(double x) {
  if (x != x || x >= 9223372036854775808.0 || x < -9223372036854775808.0) return INT64_MIN;
  return (int64_t)x;
}

// ImageTxt.Value(u, v).Z: nearest texel with the reference's own clamping.
IZPI_HD uint64_t texel(const Map& m, double u, double v) {
  int64_t i = go_int(u * (double)m.w);
  int64_t j = go_int((1.0 - v) * ((double)m.h - 0.001));
  if (i < 0) i = 0;
  if (j < 0) j = 0;
  if (i > (int64_t)m.w - 1) i = (int64_t)m.w - 1;
  if (j > (int64_t)m.h - 1) j = (int64_t)m.h - 1;
  return ((uint64_t)j * m.w + (uint64_t)i) * m.stride;
}
IZPI_HD double sample(const Map& m, double u, double v) { return m.z[texel(m, u, v)]; }

// The six points the four children of a parent share: its vertices 0 1 2 and the edge
// midpoints a (01), b (12), c (20). p[k] = x y z u v.
struct Six {
  double p[6][5];
};
IZPI_HD void six_points(const izpi_tri_in& t, Six& s) {
  const double* vs[3] = {t.v0, t.v1, t.v2};
  for (int k = 0; k < 3; k++) {
    for (int a = 0; a < 3; a++) s.p[k][a] = vs[k][a];
    s.p[k][3] = t.uv[2 * k];
    s.p[k][4] = t.uv[2 * k + 1];
  }
  for (int k = 0; k < 3; k++) {
    const int n = (k + 1) % 3;
    for (int a = 0; a < 5; a++) s.p[3 + k][a] = (s.p[k][a] + s.p[n][a]) / 2.0;
  }
}
// tessellate's children, in its order, as indices into Six (0 1 2 a=3 b=4 c=5).
IZPI_HD int child_point(int child, int vertex) {
  // {0,a,c} {a,b,c} {a,1,b} {c,b,2}, 4 bits per entry
  const uint32_t tbl[4] = {0x530u, 0x543u, 0x413u, 0x245u};
  return (int)((tbl[child] >> (4 * vertex)) & 15u);
}
IZPI_HD void make_child(const Six& s, int child, const izpi_tri_in& parent, izpi_tri_in& o) {
  double* vs[3] = {o.v0, o.v1, o.v2};
  for (int k = 0; k < 3; k++) {
    const double* p = s.p[child_point(child, k)];
    for (int a = 0; a < 3; a++) vs[k][a] = p[a];
    o.uv[2 * k] = p[3];
    o.uv[2 * k + 1] = p[4];
  }
  o.material = parent.material;
  o.pad = parent.pad;
}

// The UV half of isTessellatedEnough for child `child`.
IZPI_HD bool uv_enough(const Six& s, int child, double max_du, double max_dv) {
  const double* p0 = s.p[child_point(child, 0)];
  const double* p1 = s.p[child_point(child, 1)];
  const double* p2 = s.p[child_point(child, 2)];
  return gm::abs(p1[3] - p0[3]) <= max_du && gm::abs(p2[3] - p1[3]) <= max_du && gm::abs(p0[3] - p2[3]) <= max_du &&
         gm::abs(p1[4] - p0[4]) <= max_dv && gm::abs(p2[4] - p1[4]) <= max_dv && gm::abs(p0[4] - p2[4]) <= max_dv;
}
// The displacement half: d0 d1 d2 are the map's values at the child's vertices.
IZPI_HD bool variation_enough(double d0, double d1, double d2, double dmin, double dmax) {
  const double lo = gm::min(d0, gm::min(d1, d2));
  const double hi = gm::max(d0, gm::max(d1, d2));
  const double variation = hi - lo;
  const double range = gm::abs(dmax - dmin);
  return variation * range <= IZPI_DSP_THRESHOLD;
}

// The children of `parent` that are tessellated enough, as a 4-bit mask. The map is read
// only when some child passes the UV test; d[] receives the six shared values then.
IZPI_HD uint32_t done_mask(const Six& s, const Map& m, double max_du, double max_dv, double dmin, double dmax,
                           double d[6]) {
  uint32_t uvok = 0;
  for (int c = 0; c < 4; c++) uvok |= uv_enough(s, c, max_du, max_dv) ? (1u << c) : 0u;
  if (!uvok) return 0;
  uint64_t at[6];
  for (int k = 0; k < 6; k++) at[k] = texel(m, s.p[k][3], s.p[k][4]);
  for (int k = 0; k < 6; k++) d[k] = m.z[at[k]];
  uint32_t done = 0;
  for (int c = 0; c < 4; c++)
    if ((uvok >> c) & 1u)
      done |= variation_enough(d[child_point(c, 0)], d[child_point(c, 1)], d[child_point(c, 2)], dmin, dmax) ? (1u << c)
                                                                                                            : 0u;
  return done;
}

struct Vec {
  double x, y, z;
};
IZPI_HD Vec unit(Vec v) {
  const double l = gm::sqrt((v.x * v.x) + (v.y * v.y) + (v.z * v.z));
  Vec r;
  r.x = v.x / l;
  r.y = v.y / l;
  r.z = v.z / l;
  return r;
}

// applyDisplacement on one finished triangle; z0 z1 z2 are the map's values at its vertices.
// All three terms of MatrixVectorMul stay: with NaN tangents, NaN * 0 reaches the vertex.
IZPI_HD void displace(const izpi_tri_in& t, double z0, double z1, double z2, double dmin, double dmax, izpi_tri_in& o) {
  Vec e1, e2;
  e1.x = t.v1[0] - t.v0[0]; e1.y = t.v1[1] - t.v0[1]; e1.z = t.v1[2] - t.v0[2];
  e2.x = t.v2[0] - t.v0[0]; e2.y = t.v2[1] - t.v0[1]; e2.z = t.v2[2] - t.v0[2];
  Vec n;
  n.x = (e1.y * e2.z) - (e1.z * e2.y);
  n.y = -((e1.x * e2.z) - (e1.z * e2.x));
  n.z = (e1.x * e2.y) - (e1.y * e2.x);
  n = unit(n);
  const double du1 = t.uv[2] - t.uv[0], du2 = t.uv[4] - t.uv[0];
  const double dv1 = t.uv[3] - t.uv[1], dv2 = t.uv[5] - t.uv[1];
  const double f = 1.0 / (du1 * dv2 - du2 * dv1);
  Vec tg, bt;
  tg.x = f * (dv2 * e1.x - dv1 * e2.x);
  tg.y = f * (dv2 * e1.y - dv1 * e2.y);
  tg.z = f * (dv2 * e1.z - dv1 * e2.z);
  tg = unit(tg);
  bt.x = f * (-du2 * e1.x + du1 * e2.x);
  bt.y = f * (-du2 * e1.y + du1 * e2.y);
  bt.z = f * (-du2 * e1.z + du1 * e2.z);
  bt = unit(bt);
  const double zs[3] = {z0, z1, z2};
  const double* vin[3] = {t.v0, t.v1, t.v2};
  double* vout[3] = {o.v0, o.v1, o.v2};
  for (int k = 0; k < 3; k++) {
    const double x = 0.0, y = 0.0;
    const double z = dmin + ((dmax - dmin) * zs[k]);
    vout[k][0] = vin[k][0] + (tg.x * x + bt.x * y + n.x * z);
    vout[k][1] = vin[k][1] + (tg.y * x + bt.y * y + n.y * z);
    vout[k][2] = vin[k][2] + (tg.z * x + bt.z * y + n.z * z);
  }
  for (int k = 0; k < 6; k++) o.uv[k] = t.uv[k];
  o.material = t.material;
  o.pad = 0;
}

// What both entries refuse, in the same words (nullptr = fine).
inline const char* check_args(const izpi_tri_in* tris, uint64_t n, const double* rgba, uint32_t width, uint32_t height,
                              uint32_t order, const uint64_t* n_out) {
  if (!n_out || (!tris && n) || !rgba) return "displace: null argument";
  if (width < 1 || height < 1) return "displace: a displacement map needs width and height of at least 1";
  if (order != IZPI_DISPLACE_PER_TRIANGLE && order != IZPI_DISPLACE_MESH) return "displace: unknown output order";
  if (n > 0xFFFFFFFFull) return "displace: too many source triangles";
  return nullptr;
}
#define IZPI_DSP_STR2(x) #x
#define IZPI_DSP_STR(x) IZPI_DSP_STR2(x)
inline const char* cap_message() {
  return "displace: triangles are still subdividing after IZPI_DISPLACE_MAX_LEVELS (" IZPI_DSP_STR(
      IZPI_DISPLACE_MAX_LEVELS) ") levels: the map steps by more than 2/|max-min| between neighbouring texels";
}

}  // namespace dsp
