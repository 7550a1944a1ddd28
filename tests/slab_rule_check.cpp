// slab_rule_check.cpp — a stand-alone program over izpi_amd/csrc/slab_rule.h, the header
// k_trace2's global-memory node step takes its box test from, compiled here as plain C++ with
// -ffp-contract=off (tests/test_slab_rule.py builds it with -fsanitize=address,undefined;
// host_scene.cpp and scene_pack.cpp supply the test trees and pack_scene). It checks that
//   - the sorted rule (near and far planes by the ray's sign, no sort of the products) equals the
//     scalar twin `slab` for every fast ray, on random pairs in each of the 8 sign octants and on
//     pairs drawn from pools of special values;
//   - `slab` on the planes swapped by the ray's sign equals `slab` on the planes in order (a fast
//     lane in a wave that runs the twin);
//   - a sealed box (mn = +inf, mx = -inf, what an uploader could give an empty slot: DESIGN 3.6)
//     misses under the sorted rule;
//   - PackedScene::ordered_bounds is 1 for the built trees and 0 after one valid slot or one leaf
//     box is inverted, while an inverted empty slot leaves it 1;
//   - the 16-B load at the last leaf record's mx[2] ends inside the node block's allocation.
// Prints one "case <name> ..." line per case and "ok".
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/izpi_host.h"
#include "../izpi_amd/csrc/scene_pack.h"
#include "../izpi_amd/csrc/slab_rule.h"

using namespace izd;
using izpi_internal::pack_scene;
using izpi_internal::PackedScene;
using izpi_internal::trace_layout;
using izpi_internal::TraceLayout;

namespace {

int failures = 0;
#define EXPECT(cond, what)                                            \
  do {                                                                \
    if (!(cond)) {                                                    \
      if (failures < 20) printf("FAILED %s: %s (line %d)\n", what, #cond, __LINE__); \
      failures++;                                                     \
    }                                                                 \
  } while (0)

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) / 9007199254740992.0; }
  float range(float lo, float hi) { return lo + (float)(uni() * ((double)hi - (double)lo)); }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct Pair {
  float b[6];  // mnx, mny, mnz, mxx, mxy, mxz
  float o[3], inv[3], tmax;
};

struct Tally { uint64_t pairs = 0, fast = 0, hits = 0; };

// One pair through the three rules. need_fast: the case is meant to hold fast rays only.
void check_pair(const Pair& p, const char* name, bool need_fast, Tally* t) {
  const bool fast = ray_fast_ok(p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2]);
  t->pairs++;
  if (need_fast) EXPECT(fast, name);
  const bool twin = slab(p.b[0], p.b[1], p.b[2], p.b[3], p.b[4], p.b[5], p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmax);
  const uint32_t nx = slab_near_index(0, p.inv[0], fast), ny = slab_near_index(1, p.inv[1], fast), nz = slab_near_index(2, p.inv[2], fast);
  const uint32_t fx = slab_far_index(0, nx), fy = slab_far_index(1, ny), fz = slab_far_index(2, nz);
  EXPECT((nx == 0 || nx == 3) && (ny == 1 || ny == 4) && (nz == 2 || nz == 5) && nx + fx == 3 && ny + fy == 5 && nz + fz == 7, name);
  if (!fast) {  // canonical order: the loads and the twin's operands are the unsorted ones
    EXPECT(nx == 0 && ny == 1 && nz == 2, name);
    return;
  }
  t->fast++;
  t->hits += twin;
  EXPECT((nx == 3) == (p.inv[0] < 0) && (ny == 4) == (p.inv[1] < 0) && (nz == 5) == (p.inv[2] < 0), name);
  const bool sorted = slab_sorted(p.b, nx, ny, nz, p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmax);
  EXPECT(sorted == twin, name);
  const bool swapped = slab(p.b[nx], p.b[ny], p.b[nz], p.b[fx], p.b[fy], p.b[fz], p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmax);
  EXPECT(swapped == twin, name);
  // the sealed box: no fast ray of either sign enters it
  float e[6] = {p.b[0], p.b[1], p.b[2], p.b[3], p.b[4], p.b[5]};
  for (int a = 0; a < 3; a++) {
    const float mn = e[a], mx = e[3 + a];
    e[a] = INFINITY; e[3 + a] = -INFINITY;
    EXPECT(!slab_sorted(e, nx, ny, nz, p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmax), name);
    e[a] = mn; e[3 + a] = mx;
  }
  const float sealed[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  EXPECT(!slab_sorted(sealed, nx, ny, nz, p.o[0], p.o[1], p.o[2], p.inv[0], p.inv[1], p.inv[2], p.tmax), name);
}

float pick_tmax(Rng& r) {
  switch (r.below(7)) {
    case 6: return r.below(2) ? -1.0f : NAN;  // (explicit bounds may hold anything: the compares are the twin's)
    case 0: return INFINITY;
    case 1: return 0.0f;
    case 2: return 1e-30f;
    case 3: return 1e-42f;  // subnormal
    case 4: return r.range(0.0f, 50.0f);
    default: return r.range(0.0f, 1000.0f);
  }
}

// Random boxes around random origins, directions of one sign octant.
void random_octant(int oct, uint32_t n, Tally* t) {
  char name[32];
  snprintf(name, sizeof name, "octant%d", oct);
  Rng r{0x1234u + (uint64_t)oct};
  for (uint32_t k = 0; k < n; k++) {
    Pair p;
    float dir[3];
    for (int a = 0; a < 3; a++) {
      const float c = r.range(-100.0f, 100.0f), h = r.below(8) == 0 ? 0.0f : r.range(0.0f, 40.0f);
      p.b[a] = c - h; p.b[3 + a] = c + h;
      if (p.b[a] > p.b[3 + a]) p.b[3 + a] = p.b[a];
      p.o[a] = r.below(6) == 0 ? (r.below(2) ? p.b[a] : p.b[3 + a]) : r.range(-150.0f, 150.0f);  // some origins on a plane
      float d = r.range(1e-4f, 1.0f);
      if (r.below(16) == 0) d = 1e-30f;  // a nearly axis-parallel ray: products overflow
      if ((oct >> a) & 1) d = -d;
      p.inv[a] = (float)(1.0 / (double)d);
      dir[a] = d;
    }
    if (k % 2) {  // every other ray passes through a point of its box (from in front of it, or from inside)
      const float back = r.range(-20.0f, 200.0f);
      for (int a = 0; a < 3; a++) p.o[a] = r.range(p.b[a], p.b[3 + a]) - back * dir[a];
    }
    p.tmax = pick_tmax(r);
    check_pair(p, name, true, t);
  }
}

// Pairs drawn from pools of special values: flat boxes, origins on a plane (t = +-0), boxes behind
// the ray, bounds and products that overflow, subnormal products, infinite boxes; inverse
// directions that are huge, tiny, zero, infinite or NaN among them (those rays are not fast).
void special_pairs(int oct, uint32_t n, Tally* t) {
  static const float bound[] = {-INFINITY, -3.4028234663852886e38f, -1e30f, -7.5f, -1.0f, -1e-40f, -0.0f, 0.0f, 1e-40f,
                                1e-20f, 1.0f, 2.0f, 7.5f, 1e30f, 3.4028234663852886e38f, INFINITY};
  static const float org[] = {-3.0e38f, -1e30f, -7.5f, -1.0f, -1e-40f, -0.0f, 0.0f, 1e-40f, 1e-20f, 1.0f, 2.0f, 7.5f, 1e30f, 3.0e38f};
  static const float invm[] = {1e-42f, 1e-38f, 1e-30f, 1e-5f, 0.5f, 1.0f, 3.0f, 1e5f, 1e30f, 3.4028234663852886e38f};
  static const float tmaxs[] = {0.0f, 1e-45f, 1e-30f, 1.0f, 1e30f, INFINITY, -1.0f, NAN};
  const uint32_t nb = sizeof bound / sizeof *bound, no = sizeof org / sizeof *org, ni = sizeof invm / sizeof *invm;
  char name[32];
  snprintf(name, sizeof name, "special%d", oct);
  Rng r{0x9876u + (uint64_t)oct};
  for (uint32_t k = 0; k < n; k++) {
    Pair p;
    for (int a = 0; a < 3; a++) {
      uint32_t i = r.below(nb), j = r.below(nb);
      if (r.below(4) == 0) j = i;  // flat
      if (i > j) { const uint32_t s = i; i = j; j = s; }  // (the pool ascends: mn <= mx)
      p.b[a] = bound[i]; p.b[3 + a] = bound[j];
      p.o[a] = r.below(3) == 0 && fabsf(p.b[a]) < INFINITY ? p.b[a] : (r.below(4) == 0 && fabsf(p.b[3 + a]) < INFINITY ? p.b[3 + a] : org[r.below(no)]);
      float v = invm[r.below(ni)];
      if ((oct >> a) & 1) v = -v;
      p.inv[a] = v;
    }
    p.tmax = tmaxs[r.below(sizeof tmaxs / sizeof *tmaxs)];
    check_pair(p, name, true, t);
  }
  // rays that are not fast keep the canonical planes
  static const float bad_inv[] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN};
  for (uint32_t k = 0; k < 200; k++) {
    Pair p;
    for (int a = 0; a < 3; a++) { p.b[a] = -1.0f; p.b[3 + a] = 1.0f; p.o[a] = org[r.below(no)]; p.inv[a] = ((oct >> a) & 1) ? -1.0f : 1.0f; }
    p.tmax = 10.0f;
    if (k % 2) p.inv[r.below(3)] = bad_inv[r.below(5)];
    else p.o[r.below(3)] = r.below(2) ? INFINITY : NAN;
    Tally none;
    check_pair(p, name, false, &none);
    EXPECT(none.fast == 0, name);
  }
}

// A row of n quads (2 n triangles) under Lambertian and DiffuseLight materials.
izpi_host_scene* build(int quads) {
  std::vector<izpi_tri_in> tris(2 * (size_t)quads);
  for (int i = 0; i < 2 * quads; i++) {
    izpi_tri_in& t = tris[i];
    memset(&t, 0, sizeof t);
    const double x = i / 2;
    const double q[4][3] = {{x, 0, 0.1 * (i % 5)}, {x + 1, 0.1 * i, 0}, {x + 1, 0.2, 1}, {x, 0.3, 1}};
    static const int corners[2][3] = {{0, 1, 2}, {0, 2, 3}};
    const int* c = corners[i & 1];
    memcpy(t.v0, q[c[0]], 24); memcpy(t.v1, q[c[1]], 24); memcpy(t.v2, q[c[2]], 24);
    t.material = (uint32_t)(i % 2);
  }
  izpi_material mats[2];
  memset(mats, 0, sizeof mats);
  for (int i = 0; i < 2; i++) {
    mats[i].kind = i ? IZPI_MAT_DIFFUSE_LIGHT : IZPI_MAT_LAMBERT;
    mats[i].albedo_tex = 0; mats[i].spectral_tex = -1;
    mats[i].normal_tex = mats[i].roughness_tex = mats[i].metalness_tex = mats[i].absorb_tex = -1;
    mats[i].ref_idx = 1.5;
  }
  izpi_texture tex;
  memset(&tex, 0, sizeof tex);
  tex.kind = IZPI_TEX_CONSTANT; tex.value[0] = 0.5; tex.value[1] = 0.25; tex.value[2] = 0.125;
  izpi_scene_input in;
  memset(&in, 0, sizeof in);
  in.num_tris = (uint32_t)tris.size(); in.tris = tris.data();
  in.num_materials = 2; in.materials = mats;
  in.num_textures = 1; in.textures = &tex;
  const double from[3] = {3, 5, 8}, at[3] = {3, 0, 0.5}, up[3] = {0, 1, 0};
  memcpy(in.camera.look_from, from, 24); memcpy(in.camera.look_at, at, 24); memcpy(in.camera.vup, up, 24);
  in.camera.vfov = 40; in.camera.aspect = 1; in.camera.focus_dist = 1; in.camera.time0 = 0; in.camera.time1 = 1;
  in.camera.exposure = 1;
  in.bvh_seed = 7;
  izpi_host_scene* s = nullptr;
  if (izpi_host_build_scene(&in, &s)) { fprintf(stderr, "build: %s\n", izpi_host_last_error()); return nullptr; }
  return s;
}

// ordered_bounds of the tree with `nodes` in place of the descriptor's, or -1.
int ordered_of(const izpi_scene_desc& base, const std::vector<izpi_bvh4_node>& nodes, PackedScene* ps) {
  izpi_scene_desc d = base;
  d.nodes = nodes.data();
  std::string err;
  const int rc = pack_scene(&d, ps, &err);
  if (rc) { printf("pack_scene: %d %s\n", rc, err.c_str()); return -1; }
  return (int)ps->ordered_bounds;
}

void swap_bounds(izpi_bvh4_node& n, int slot, int axis) {
  float* mn = axis == 0 ? n.min_x : axis == 1 ? n.min_y : n.min_z;
  float* mx = axis == 0 ? n.max_x : axis == 1 ? n.max_y : n.max_z;
  const float t = mn[slot]; mn[slot] = mx[slot]; mx[slot] = t;
}

// The 16-B loads of a leaf lane start at each of the record's six floats: the one at mx[2] of
// the block's last record must end inside the allocation (and does not inside the records).
void check_alloc(const char* name, uint64_t n_inner, uint64_t n_innerq, uint64_t n_leaves) {
  const TraceLayout tl = trace_layout(n_inner, n_innerq, n_leaves);
  const uint64_t last = tl.leaves_at + (n_leaves - 1) * sizeof(GLeaf);
  const uint64_t end = last + offsetof(GLeaf, mx) + 2 * sizeof(float) + 16;  // slab_far_index / near index 5, shift 2
  EXPECT(offsetof(GLeaf, mn) == 0 && offsetof(GLeaf, mx) == 12, name);
  EXPECT(end == last + (5u << 2) + 16, name);
  EXPECT(end > tl.bytes && end <= tl.alloc_bytes, name);
  EXPECT(tl.alloc_bytes == tl.bytes + izpi_internal::TRACE_TAIL_PAD, name);
  // an inner node's sixth piece ends inside its record
  EXPECT((5u << 4) + 16 <= offsetof(GInner, child), name);
  printf("case alloc_%s: records %llu B, last load ends at %llu, allocation %llu B\n", name, (unsigned long long)tl.bytes,
         (unsigned long long)end, (unsigned long long)tl.alloc_bytes);
}

void check_trees() {
  for (int quads : {1, 6, 40}) {
    izpi_host_scene* hs = build(quads);
    if (!hs) { failures++; return; }
    const izpi_scene_desc& d = *izpi_host_scene_desc(hs);
    const std::vector<izpi_bvh4_node> nodes(d.nodes, d.nodes + d.num_nodes);
    PackedScene ps;
    EXPECT(ordered_of(d, nodes, &ps) == 1, "ordered_built");
    EXPECT(ps.nan_free_bounds == 1, "ordered_built");
    char an[32];
    snprintf(an, sizeof an, "tree%d", quads);
    check_alloc(an, ps.inner.size(), ps.innerq.size(), ps.leaves.size());
    int valid_inner = 0, leaf_boxes = 0, empties = 0;
    for (uint32_t k = 0; k < d.num_nodes; k++) {
      const izpi_bvh4_node& n = nodes[k];
      if (n.prim_count[0] > 0) {  // a leaf node: slot 0 is its box
        for (int a = 0; a < 3; a++) {
          std::vector<izpi_bvh4_node> m(nodes);
          if ((a == 0 ? m[k].min_x[0] == m[k].max_x[0] : a == 1 ? m[k].min_y[0] == m[k].max_y[0] : m[k].min_z[0] == m[k].max_z[0])) continue;
          swap_bounds(m[k], 0, a);
          PackedScene q;
          EXPECT(ordered_of(d, m, &q) == 0, "ordered_leaf_inverted");
          EXPECT(q.nan_free_bounds == 1, "ordered_leaf_inverted");
          leaf_boxes++;
        }
        continue;
      }
      for (int i = 0; i < 4; i++) {
        std::vector<izpi_bvh4_node> m(nodes);
        if (n.child[i] == -1) {  // an inverted empty slot is read by no result
          m[k].min_x[i] = 1.0f; m[k].max_x[i] = -1.0f; m[k].min_y[i] = INFINITY; m[k].max_y[i] = -INFINITY;
          PackedScene q;
          EXPECT(ordered_of(d, m, &q) == 1, "ordered_empty_inverted");
          empties++;
          continue;
        }
        const int a = (int)((k + (uint32_t)i) % 3);
        if ((a == 0 ? n.min_x[i] == n.max_x[i] : a == 1 ? n.min_y[i] == n.max_y[i] : n.min_z[i] == n.max_z[i])) continue;
        swap_bounds(m[k], i, a);
        PackedScene q;
        EXPECT(ordered_of(d, m, &q) == 0, "ordered_slot_inverted");
        valid_inner++;
      }
    }
    printf("case trees_%d: %u nodes, %d valid slots, %d leaf boxes and %d empty slots inverted in turn\n", quads, d.num_nodes,
           valid_inner, leaf_boxes, empties);
    if (quads == 40) EXPECT(valid_inner > 0 && leaf_boxes > 0 && empties > 0, "trees_cover");
    if (quads == 1) EXPECT(leaf_boxes > 0, "trees_cover");
    izpi_host_scene_free(hs);
  }
}

}  // namespace

int main() {
  for (int oct = 0; oct < 8; oct++) {
    Tally t;
    random_octant(oct, 120000, &t);
    EXPECT(t.fast == t.pairs && t.pairs >= 100000 && t.hits > t.pairs / 10 && t.hits < t.pairs - t.pairs / 10, "octant_cover");
    printf("case octant%d: %llu pairs, %llu fast, %llu hit\n", oct, (unsigned long long)t.pairs, (unsigned long long)t.fast,
           (unsigned long long)t.hits);
    Tally s;
    special_pairs(oct, 100000, &s);
    EXPECT(s.fast == s.pairs && s.hits > 0 && s.hits < s.pairs, "special_cover");
    printf("case special%d: %llu pairs, %llu fast, %llu hit\n", oct, (unsigned long long)s.pairs, (unsigned long long)s.fast,
           (unsigned long long)s.hits);
  }
  check_trees();
  check_alloc("c3_like", 190000, 0, 820000);
  check_alloc("quantised", 1000, 1000, 4000);
  check_alloc("one_leaf", 1, 0, 1);
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
