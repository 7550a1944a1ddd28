// scene_facts_check.cpp — the two scene facts k_trace2's primitive step is specialised on, as
// pack_scene (izpi_amd/csrc/scene_pack.cpp) records them: PackedScene::leaf_max, the largest
// primitive count of a leaf, and PackedScene::no_pathlen, no dielectric in the material table.
// Small scenes from izpi_host_build_scene with hand-made trees attached
// (izpi_host_scene_set_bvh), as a stand-alone program (tests/test_scene_facts.py builds it under
// AddressSanitizer and UBSan). One line per case:
//   name|status|leaf_max=N walked=N no_pathlen=B
// walked: the largest prim_count of the descriptor's leaf nodes, counted here.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/izpi_host.h"
#include "../izpi_amd/csrc/scene_pack.h"

using izpi_internal::pack_scene;
using izpi_internal::PackedScene;

namespace {

izpi_material material(uint32_t kind, int32_t albedo) {
  izpi_material m;
  memset(&m, 0, sizeof m);
  m.kind = kind; m.albedo_tex = albedo; m.spectral_tex = -1;
  m.normal_tex = m.roughness_tex = m.metalness_tex = m.absorb_tex = -1;
  m.ref_idx = 1.5;
  return m;
}

// n triangles in a row over Lambertian + DiffuseLight, with a dielectric in the material table
// as well (glass) that `glass_used` triangles use.
izpi_host_scene* build(int n, bool glass, int glass_used) {
  std::vector<izpi_tri_in> tris((size_t)n);
  for (int i = 0; i < n; i++) {
    izpi_tri_in& t = tris[(size_t)i];
    memset(&t, 0, sizeof t);
    const double x = i;
    const double a[3] = {x, 0, 0}, b[3] = {x + 1, 0.1 * i, 0}, c[3] = {x + 0.5, 1, 0.25};
    memcpy(t.v0, a, 24); memcpy(t.v1, b, 24); memcpy(t.v2, c, 24);
    t.material = i < glass_used ? 2u : (uint32_t)(i & 1);
  }
  std::vector<izpi_material> mats = {material(IZPI_MAT_LAMBERT, 0), material(IZPI_MAT_DIFFUSE_LIGHT, 0)};
  if (glass) mats.push_back(material(IZPI_MAT_DIELECTRIC, -1));
  izpi_texture tex;
  memset(&tex, 0, sizeof tex);
  tex.kind = IZPI_TEX_CONSTANT; tex.value[0] = 0.5; tex.value[1] = 0.25; tex.value[2] = 0.125;
  izpi_scene_input in;
  memset(&in, 0, sizeof in);
  in.num_tris = (uint32_t)n; in.tris = tris.data();
  in.num_materials = (uint32_t)mats.size(); in.materials = mats.data();
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

izpi_bvh4_node empty_node() {
  izpi_bvh4_node n;
  memset(&n, 0, sizeof n);
  for (int i = 0; i < 4; i++) {
    n.min_x[i] = n.min_y[i] = n.min_z[i] = -100.0f;
    n.max_x[i] = n.max_y[i] = n.max_z[i] = 100.0f;
    n.child[i] = -1;
  }
  return n;
}

// A root whose slots are leaves of the given sizes in primitive order; a single size: the root
// itself is that leaf.
std::vector<izpi_bvh4_node> tree(const std::vector<int>& sizes) {
  std::vector<izpi_bvh4_node> nodes;
  if (sizes.size() == 1) {
    izpi_bvh4_node leaf = empty_node();
    leaf.child[0] = 0; leaf.prim_count[0] = sizes[0];
    nodes.push_back(leaf);
    return nodes;
  }
  izpi_bvh4_node root = empty_node();
  int start = 0;
  for (size_t i = 0; i < sizes.size(); i++) {
    root.child[i] = (int32_t)(1 + i);
    izpi_bvh4_node leaf = empty_node();
    leaf.child[0] = start; leaf.prim_count[0] = sizes[i];
    start += sizes[i];
    nodes.push_back(leaf);
  }
  nodes.insert(nodes.begin(), root);
  return nodes;
}

int failures = 0;

void report(const char* name, izpi_host_scene* s) {
  const izpi_scene_desc* d = izpi_host_scene_desc(s);
  uint32_t walked = 0;
  for (uint32_t k = 0; k < d->num_nodes; k++)
    if (d->nodes[k].prim_count[0] > 0 && (uint32_t)d->nodes[k].prim_count[0] > walked) walked = (uint32_t)d->nodes[k].prim_count[0];
  PackedScene ps;
  std::string err;
  const int rc = pack_scene(d, &ps, &err);
  if (rc) fprintf(stderr, "%s: %s\n", name, err.c_str());
  printf("%s|%d|leaf_max=%u walked=%u no_pathlen=%u\n", name, rc, ps.leaf_max, walked, ps.no_pathlen);
}

// n triangles under the tree `sizes` (which must add up to n)
void tree_case(const char* name, const std::vector<int>& sizes, bool glass = false, int glass_used = 0) {
  int n = 0;
  for (int c : sizes) n += c;
  izpi_host_scene* s = build(n, glass, glass_used);
  if (!s) { failures++; return; }
  const std::vector<izpi_bvh4_node> nodes = tree(sizes);
  std::vector<uint32_t> order((size_t)n);
  for (int i = 0; i < n; i++) order[(size_t)i] = (uint32_t)i;
  if (izpi_host_scene_set_bvh(s, nodes.data(), (uint32_t)nodes.size(), order.data())) {
    fprintf(stderr, "%s: set_bvh: %s\n", name, izpi_host_last_error());
    failures++;
  } else {
    report(name, s);
  }
  izpi_host_scene_free(s);
}

}  // namespace

int main() {
  tree_case("root_leaf_1", {1});
  tree_case("root_leaf_2", {2});
  tree_case("root_leaf_3", {3});
  tree_case("root_leaf_4", {4});
  tree_case("root_leaf_7", {7});
  tree_case("leaves_3_1", {3, 1});
  tree_case("leaves_1_4_2", {1, 4, 2});
  tree_case("leaves_3_3_3_3", {3, 3, 3, 3});
  tree_case("leaves_2_1_2_4", {2, 1, 2, 4});
  tree_case("glass_in_table_unused", {3, 1}, true, 0);
  tree_case("glass_used", {2, 2}, true, 1);
  {  // the host builder's own tree
    izpi_host_scene* s = build(12, false, 0);
    if (s) { report("host_built_12", s); izpi_host_scene_free(s); } else failures++;
  }
  return failures ? 1 : 0;
}
