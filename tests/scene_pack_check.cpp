// scene_pack_check.cpp — pack_scene (izpi_amd/csrc/scene_pack.cpp) on small scenes built by
// izpi_host_build_scene and on mutated copies of their descriptors, as a stand-alone
// program (tests/test_scene_pack.py builds it under AddressSanitizer and UBSan: every array
// of a descriptor copy is a heap block of exactly its size). One line per case:
//   name|status|error text|key=value ...
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "../include/izpi_host.h"
#include "../izpi_amd/csrc/scene_pack.h"

using namespace izd;
using izpi_internal::pack_scene;
using izpi_internal::PackedScene;

namespace {

// A descriptor with arrays of its own, to mutate.
struct Desc {
  izpi_scene_desc d;
  std::vector<izpi_bvh4_node> nodes;
  std::vector<uint32_t> prim_ref, tri_mat, sph_mat, light_ref;
  std::vector<double> v0, v1, v2, e1, e2, nrm, tg, bt, uv, area, c0, c1, st, rad, texels, wl, val;
  std::vector<izpi_material> mats;
  std::vector<izpi_texture> texs;
  explicit Desc(const izpi_scene_desc& s) : d(s) {
    const size_t nt = s.num_tris, ns = s.num_spheres;
    nodes.assign(s.nodes, s.nodes + s.num_nodes);
    prim_ref.assign(s.prim_ref, s.prim_ref + s.num_prims);
    tri_mat.assign(s.tri_mat, s.tri_mat + nt);
    light_ref.assign(s.light_ref, s.light_ref + s.num_lights);
    v0.assign(s.tri_v0, s.tri_v0 + 3 * nt); v1.assign(s.tri_v1, s.tri_v1 + 3 * nt); v2.assign(s.tri_v2, s.tri_v2 + 3 * nt);
    e1.assign(s.tri_e1, s.tri_e1 + 3 * nt); e2.assign(s.tri_e2, s.tri_e2 + 3 * nt); nrm.assign(s.tri_normal, s.tri_normal + 3 * nt);
    tg.assign(s.tri_tangent, s.tri_tangent + 3 * nt); bt.assign(s.tri_bitangent, s.tri_bitangent + 3 * nt);
    uv.assign(s.tri_uv, s.tri_uv + 6 * nt); area.assign(s.tri_area, s.tri_area + nt);
    if (ns) {
      sph_mat.assign(s.sph_mat, s.sph_mat + ns);
      c0.assign(s.sph_center0, s.sph_center0 + 3 * ns); c1.assign(s.sph_center1, s.sph_center1 + 3 * ns);
      st.assign(s.sph_time, s.sph_time + 2 * ns); rad.assign(s.sph_radius, s.sph_radius + ns);
    }
    mats.assign(s.materials, s.materials + s.num_materials);
    texs.assign(s.textures, s.textures + s.num_textures);
    if (s.num_texels) texels.assign(s.texels, s.texels + s.num_texels);
    if (s.num_spd) { wl.assign(s.spd_wavelengths, s.spd_wavelengths + s.num_spd); val.assign(s.spd_values, s.spd_values + s.num_spd); }
    fix();
  }
  // the descriptor's pointers and counts from the arrays (after a copy or a resize)
  void fix() {
    d.nodes = nodes.data(); d.num_nodes = (uint32_t)nodes.size();
    d.prim_ref = prim_ref.data(); d.num_prims = (uint32_t)prim_ref.size();
    d.tri_mat = tri_mat.data(); d.num_tris = (uint32_t)tri_mat.size();
    d.sph_mat = sph_mat.data(); d.num_spheres = (uint32_t)sph_mat.size();
    d.light_ref = light_ref.data(); d.num_lights = (uint32_t)light_ref.size();
    d.tri_v0 = v0.data(); d.tri_v1 = v1.data(); d.tri_v2 = v2.data(); d.tri_e1 = e1.data(); d.tri_e2 = e2.data();
    d.tri_normal = nrm.data(); d.tri_tangent = tg.data(); d.tri_bitangent = bt.data(); d.tri_uv = uv.data(); d.tri_area = area.data();
    d.sph_center0 = c0.data(); d.sph_center1 = c1.data(); d.sph_time = st.data(); d.sph_radius = rad.data();
    d.materials = mats.data(); d.num_materials = (uint32_t)mats.size();
    d.textures = texs.data(); d.num_textures = (uint32_t)texs.size();
    d.texels = texels.data(); d.num_texels = texels.size();
    d.spd_wavelengths = wl.data(); d.spd_values = val.data(); d.num_spd = (uint32_t)wl.size();
  }
};

izpi_material material(uint32_t kind, int32_t albedo = -1, int32_t spectral = -1) {
  izpi_material m;
  memset(&m, 0, sizeof m);
  m.kind = kind; m.albedo_tex = albedo; m.spectral_tex = spectral;
  m.normal_tex = m.roughness_tex = m.metalness_tex = m.absorb_tex = -1;
  m.ref_idx = 1.5; m.fuzz = 0.1; m.rgb[0] = 0.8; m.rgb[1] = 0.7; m.rgb[2] = 0.6;
  return m;
}
izpi_texture texture(uint32_t kind) {
  izpi_texture t;
  memset(&t, 0, sizeof t);
  t.kind = kind;
  t.pad0 = 77;  // the packer sets it
  return t;
}

// Materials and textures of the full scene (indices used by the cases below).
enum { M_LAMBERT, M_LIGHT, M_GLASS, M_METAL, M_ISO, M_PBR, M_LAMBERT_IMG, NUM_MATS };
enum { T_CONST, T_GRAY, T_RGBA, T_SPD_UNIFORM, T_SPD_SORTED, T_SPD_UNSORTED, T_GAUSS, T_SPEC_IMG, NUM_TEXS };
const double kWl[] = {400, 450, 500, 550, 600, /* sorted */ 400, 410, 500, 700, /* unsorted */ 500, 400, 600};

// 12 triangles (6 quads in a row), with 2 spheres and every material kind (full) or
// Lambertian + DiffuseLight over one constant texture only (basic).
izpi_host_scene* build(bool full) {
  std::vector<izpi_tri_in> tris(12);
  for (int i = 0; i < 12; i++) {
    izpi_tri_in& t = tris[i];
    memset(&t, 0, sizeof t);
    const double x = i / 2;
    const double q[4][3] = {{x, 0, 0}, {x + 1, 0.1 * i, 0}, {x + 1, 0.2, 1}, {x, 0.3, 1}};
    static const int corners[2][3] = {{0, 1, 2}, {0, 2, 3}};
    const int* c = corners[i & 1];
    memcpy(t.v0, q[c[0]], 24); memcpy(t.v1, q[c[1]], 24); memcpy(t.v2, q[c[2]], 24);
    const double uv[6] = {0.1, 0.2, 0.9, 0.15 + 0.01 * i, 0.5, 0.8};
    memcpy(t.uv, uv, 48);
    t.material = full ? (uint32_t)(i % NUM_MATS) : (uint32_t)(i % 2);
  }
  std::vector<izpi_sphere_in> sph(2);
  for (int i = 0; i < 2; i++) {
    memset(&sph[i], 0, sizeof sph[i]);
    sph[i].center[0] = 1.5 + 3 * i; sph[i].center[1] = 2; sph[i].center[2] = 0.5;
    sph[i].radius = 0.5 + 0.25 * i;
    sph[i].material = i ? M_GLASS : M_LIGHT;
  }
  std::vector<izpi_material> mats;
  std::vector<izpi_texture> texs;
  std::vector<double> texels, val;
  if (full) {
    mats = {material(IZPI_MAT_LAMBERT, T_CONST, T_SPD_UNIFORM), material(IZPI_MAT_DIFFUSE_LIGHT, T_CONST, T_GAUSS),
            material(IZPI_MAT_DIELECTRIC, -1, T_SPD_SORTED), material(IZPI_MAT_METAL), material(IZPI_MAT_ISOTROPIC, T_CONST),
            material(IZPI_MAT_PBR, T_RGBA, T_SPEC_IMG), material(IZPI_MAT_LAMBERT, T_RGBA, T_SPD_UNIFORM)};
    mats[M_GLASS].absorb_tex = T_SPD_UNSORTED;
    mats[M_PBR].roughness_tex = T_GRAY; mats[M_PBR].metalness_tex = T_CONST;
    texs = {texture(IZPI_TEX_CONSTANT), texture(IZPI_TEX_IMAGE), texture(IZPI_TEX_IMAGE), texture(IZPI_TEX_SPECTRAL_TABULATED),
            texture(IZPI_TEX_SPECTRAL_TABULATED), texture(IZPI_TEX_SPECTRAL_TABULATED), texture(IZPI_TEX_SPECTRAL_GAUSSIAN),
            texture(IZPI_TEX_SPECTRAL_IMAGE)};
    texs[T_CONST].value[0] = 0.7; texs[T_CONST].value[1] = 0.6; texs[T_CONST].value[2] = 0.5;
    texs[T_GRAY].width = 3; texs[T_GRAY].height = 1; texs[T_GRAY].texel_offset = 0;  // 3 texels: an odd run before the RGBA one
    texs[T_RGBA].width = 2; texs[T_RGBA].height = 2; texs[T_RGBA].texel_offset = 12;
    texs[T_SPEC_IMG].width = 2; texs[T_SPEC_IMG].height = 2; texs[T_SPEC_IMG].texel_offset = 12;
    texs[T_SPD_UNIFORM].spd_offset = 0; texs[T_SPD_UNIFORM].spd_count = 5;
    texs[T_SPD_SORTED].spd_offset = 5; texs[T_SPD_SORTED].spd_count = 4;
    texs[T_SPD_UNSORTED].spd_offset = 9; texs[T_SPD_UNSORTED].spd_count = 3;
    texs[T_GAUSS].peak = 1; texs[T_GAUSS].center = 550; texs[T_GAUSS].width_nm = 50;
    for (int k = 0; k < 3; k++) { const double g = 0.25 * (k + 1); texels.insert(texels.end(), {g, g, g, 1.0 - g}); }
    for (int k = 0; k < 16; k++) texels.push_back(0.05 * (k + 1));
    for (size_t k = 0; k < sizeof kWl / sizeof *kWl; k++) val.push_back(0.1 + 0.05 * k);
  } else {
    mats = {material(IZPI_MAT_LAMBERT, 0), material(IZPI_MAT_DIFFUSE_LIGHT, 0)};
    texs = {texture(IZPI_TEX_CONSTANT)};
    texs[0].value[0] = 0.5; texs[0].value[1] = 0.25; texs[0].value[2] = 0.125;
  }
  izpi_scene_input in;
  memset(&in, 0, sizeof in);
  in.num_tris = 12; in.tris = tris.data();
  if (full) { in.num_spheres = 2; in.spheres = sph.data(); }
  in.num_materials = (uint32_t)mats.size(); in.materials = mats.data();
  in.num_textures = (uint32_t)texs.size(); in.textures = texs.data();
  in.num_texels = texels.size(); in.texels = texels.data();
  in.num_spd = (uint32_t)val.size(); in.spd_wavelengths = kWl; in.spd_values = val.data();
  const double from[3] = {3, 5, 8}, at[3] = {3, 0, 0.5}, up[3] = {0, 1, 0};
  memcpy(in.camera.look_from, from, 24); memcpy(in.camera.look_at, at, 24); memcpy(in.camera.vup, up, 24);
  in.camera.vfov = 40; in.camera.aspect = 1; in.camera.focus_dist = 1; in.camera.time0 = 0; in.camera.time1 = 1;
  in.camera.exposure = 1;
  in.bvh_seed = 7;
  izpi_host_scene* s = nullptr;
  if (izpi_host_build_scene(&in, &s)) { fprintf(stderr, "build: %s\n", izpi_host_last_error()); return nullptr; }
  return s;
}

bool same(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }
bool is_image(const izpi_scene_desc& d, int32_t t) {
  return t >= 0 && (d.textures[t].kind == IZPI_TEX_IMAGE || d.textures[t].kind == IZPI_TEX_SPECTRAL_IMAGE);
}

// What a valid descriptor's PackedScene must hold, field by field against the descriptor.
std::string structure(const izpi_scene_desc& d, const PackedScene& ps) {
  bool refs = true, leaves = true, contains = true, rows = true, mk = true, lights = true, tex = true, slots = true;
  std::vector<int32_t> inner_of(d.num_nodes, -1);
  uint32_t n_inner = 0;
  for (uint32_t k = 0; k < d.num_nodes; k++)
    if (d.nodes[k].prim_count[0] <= 0) inner_of[k] = (int32_t)n_inner++;
  refs = refs && ps.num_inner == n_inner && ps.inner.size() == (n_inner ? n_inner : 1) && ps.leaves.size() == (d.num_prims ? d.num_prims : 1);
  refs = refs && ps.innerq.size() == (ps.quantized ? n_inner : 0);
  const izpi_bvh4_node& r0 = d.nodes[0];
  refs = refs && ps.root == (inner_of[0] >= 0 ? inner_of[0] : make_leaf_ref(r0.child[0], r0.prim_count[0]));
  for (uint32_t k = 0; k < d.num_nodes; k++) {
    const izpi_bvh4_node& n = d.nodes[k];
    if (inner_of[k] < 0) {
      if (k == 0) {  // a root leaf has no parent slot
        const GLeaf& L = ps.leaves[(size_t)n.child[0]];
        leaves = leaves && L.start == n.child[0] && L.count == n.prim_count[0];
      }
      continue;
    }
    const GInner& g = ps.inner[(size_t)inner_of[k]];
    if (!ps.quantized) refs = refs && same(g.mnx, n.min_x, 96);
    for (int i = 0; i < 4; i++) {
      const int32_t c = n.child[i];
      refs = refs && g.pad[i] == 0;
      if (ps.quantized) refs = refs && ps.innerq[(size_t)inner_of[k]].child[i] == g.child[i];
      if (c == -1) { refs = refs && g.child[i] == -1; continue; }
      const float ex[6] = {n.min_x[i], n.min_y[i], n.min_z[i], n.max_x[i], n.max_y[i], n.max_z[i]};
      const float de[6] = {g.mnx[i], g.mny[i], g.mnz[i], g.mxx[i], g.mxy[i], g.mxz[i]};
      for (int a = 0; a < 3; a++) contains = contains && de[a] <= ex[a] && de[3 + a] >= ex[3 + a];
      if (ps.quantized) {  // `inner` holds what the kernels decode from `innerq`
        const GInnerQ& q = ps.innerq[(size_t)inner_of[k]];
        for (int a = 0; a < 3; a++) {
          const float s = ldexpf(1.0f, (int)((q.ex >> (8 * a)) & 255u) - 127);
          contains = contains && de[a] == qdecode(q.org[a], (q.q[a] >> (8 * i)) & 255u, s) &&
                     de[3 + a] == qdecode(q.org[a], (q.q[3 + a] >> (8 * i)) & 255u, s);
        }
      }
      const izpi_bvh4_node& cn = d.nodes[(size_t)c];
      if (inner_of[(size_t)c] >= 0) { refs = refs && g.child[i] == inner_of[(size_t)c]; continue; }
      refs = refs && ref_is_leaf(g.child[i]) && leaf_start(g.child[i]) == cn.child[0] && leaf_count(g.child[i]) == cn.prim_count[0];
      // the leaf's record: at its first primitive, with its node's slot-0 box (exact) or
      // its decoded parent slot (quantised)
      const GLeaf& L = ps.leaves[(size_t)cn.child[0]];
      const float lb[6] = {cn.min_x[0], cn.min_y[0], cn.min_z[0], cn.max_x[0], cn.max_y[0], cn.max_z[0]};
      leaves = leaves && L.start == cn.child[0] && L.count == cn.prim_count[0] && same(L.mn, ps.quantized ? de : lb, 24);
    }
  }
  // rows k of prims, shade, triverts, tritex describe prim_ref[k]
  rows = rows && ps.prims.size() == d.num_prims && ps.shade.size() == d.num_prims && ps.triverts.size() == d.num_prims &&
         ps.tritex.size() == d.num_prims;
  const GTriVerts zero_verts{};
  const GTriTex zero_tex{};
  for (uint32_t k = 0; rows && k < d.num_prims; k++) {
    const uint32_t r = d.prim_ref[k], kind = IZPI_PRIM_KIND(r);
    const size_t idx = IZPI_PRIM_INDEX(r);
    const GPrim& p = ps.prims[k];
    const GShade& gs = ps.shade[k];
    rows = rows && p.kind == kind && p.index == idx && gs.ref == r;
    uint32_t mat;
    if (kind == IZPI_PRIM_TRIANGLE) {
      mat = d.tri_mat[idx];
      rows = rows && same(p.a, d.tri_v0 + 3 * idx, 24) && same(p.a + 3, d.tri_e1 + 3 * idx, 24) && same(p.a + 6, d.tri_e2 + 3 * idx, 24) &&
             same(gs.n, d.tri_normal + 3 * idx, 24) && same(ps.triverts[k].v1, d.tri_v1 + 3 * idx, 24) &&
             same(ps.triverts[k].v2, d.tri_v2 + 3 * idx, 24) && same(ps.tritex[k].uv, d.tri_uv + 6 * idx, 48) &&
             same(ps.tritex[k].tg, d.tri_tangent + 3 * idx, 24) && same(ps.tritex[k].bt, d.tri_bitangent + 3 * idx, 24);
    } else {
      mat = d.sph_mat[idx];
      const double tail[3] = {d.sph_radius[idx], d.sph_time[2 * idx], d.sph_time[2 * idx + 1]};
      const double none[3] = {0, 0, 0};
      rows = rows && same(p.a, d.sph_center0 + 3 * idx, 24) && same(p.a + 3, d.sph_center1 + 3 * idx, 24) && same(p.a + 6, tail, 24) &&
             same(gs.n, none, 24) && same(&ps.triverts[k], &zero_verts, sizeof zero_verts) && same(&ps.tritex[k], &zero_tex, sizeof zero_tex);
    }
    // gs.mk = material index, kind and cflags (bit0: a constant albedo in mat_const; bit1: a texture reads (u, v))
    const izpi_material& m = d.materials[mat];
    const bool diffuse = m.kind == IZPI_MAT_LAMBERT || m.kind == IZPI_MAT_DIFFUSE_LIGHT;
    const bool has_const = diffuse && m.albedo_tex >= 0 && d.textures[m.albedo_tex].kind == IZPI_TEX_CONSTANT;
    const bool reads_uv = is_image(d, m.albedo_tex) || is_image(d, m.spectral_tex) || is_image(d, m.normal_tex) ||
                          is_image(d, m.roughness_tex) || is_image(d, m.metalness_tex) || is_image(d, m.absorb_tex);
    mk = mk && gs_mat(gs) == mat && gs_kind(gs) == m.kind && gs_cflags(gs) == ((has_const ? 1u : 0u) | (reads_uv ? 2u : 0u));
    const double black[4] = {0, 0, 0, 0};
    mk = mk && ps.mat_const.size() == d.num_materials && same(&ps.mat_const[mat], has_const ? d.textures[m.albedo_tex].value : black, 24) &&
         ps.mat_const[mat].w == 0;
  }
  lights = lights && ps.lights.size() == d.num_lights;
  for (uint32_t i = 0; lights && i < d.num_lights; i++) {
    const uint32_t r = d.light_ref[i], kind = IZPI_PRIM_KIND(r);
    const size_t idx = IZPI_PRIM_INDEX(r);
    const GLight& L = ps.lights[i];
    lights = lights && L.kind == kind && L.index == idx;
    if (kind == IZPI_PRIM_TRIANGLE) {
      lights = lights && same(L.v0, d.tri_v0 + 3 * idx, 24) && same(L.v1, d.tri_v1 + 3 * idx, 24) && same(L.v2, d.tri_v2 + 3 * idx, 24) &&
               same(L.e1, d.tri_e1 + 3 * idx, 24) && same(L.e2, d.tri_e2 + 3 * idx, 24) && same(L.n, d.tri_normal + 3 * idx, 24) &&
               L.area == d.tri_area[idx];
    } else {
      const double t0 = d.sph_time[2 * idx], t1 = d.sph_time[2 * idx + 1];
      lights = lights && same(L.c0, d.sph_center0 + 3 * idx, 24) && same(L.c1, d.sph_center1 + 3 * idx, 24) &&
               L.radius == d.sph_radius[idx] && L.t0 == t0 && L.t1 == t1;
      const double f = (0.0 - t0) / (t1 - t0);  // Sphere.center(0) in the device's operation order
      for (int q = 0; q < 3; q++) lights = lights && L.cz[q] == L.c0[q] + (L.c1[q] - L.c0[q]) * f;
    }
  }
  // textures: pad0 0 = scan, 1 = sorted SPD, 2 = sorted and near-uniform SPD (value[0] = wl[0], value[1] = 1 / step);
  // an IMAGE's pad0 is its storage form. Every image has its own run of texels, 32-B aligned.
  tex = tex && ps.textures.size() == d.num_textures && !ps.texels.empty();
  size_t next = 0;
  for (uint32_t i = 0; tex && i < d.num_textures; i++) {
    const izpi_texture& s = d.textures[i];
    const izpi_texture& t = ps.textures[i];
    tex = tex && t.kind == s.kind && t.width == s.width && t.height == s.height;
    if (s.kind == IZPI_TEX_SPECTRAL_TABULATED && s.spd_count >= 2) {
      const double* wl = d.spd_wavelengths + s.spd_offset;
      bool sorted = true, uniform = true;
      for (uint32_t j = 1; j < s.spd_count; j++) sorted = sorted && wl[j - 1] <= wl[j];
      const double step = (wl[s.spd_count - 1] - wl[0]) / (s.spd_count - 1);
      for (uint32_t j = 0; j < s.spd_count; j++) uniform = uniform && fabs(wl[j] - (wl[0] + j * step)) <= 0.5 * step;
      tex = tex && t.pad0 == (sorted ? (uniform ? 2u : 1u) : 0u);
      if (t.pad0 == 2) tex = tex && t.value[0] == wl[0] && t.value[1] == (double)(s.spd_count - 1) / (wl[s.spd_count - 1] - wl[0]);
    } else if (s.kind == IZPI_TEX_IMAGE || s.kind == IZPI_TEX_SPECTRAL_IMAGE) {
      const double* src = d.texels + s.texel_offset;
      const size_t np = (size_t)s.width * s.height;
      bool gray = s.kind == IZPI_TEX_IMAGE;
      for (size_t k = 0; k < np; k++) gray = gray && same(src + 4 * k, src + 4 * k + 1, 8) && same(src + 4 * k, src + 4 * k + 2, 8);
      next = (next + 3) & ~(size_t)3;
      tex = tex && t.texel_offset == next && t.pad0 == (s.kind == IZPI_TEX_IMAGE && gray ? (uint32_t)TEXF_GRAY : (uint32_t)TEXF_RGBA) &&
            next + (gray ? np : 4 * np) <= ps.texels.size();
      for (size_t k = 0; tex && k < np; k++)
        tex = gray ? same(&ps.texels[next + k], src + 4 * k, 8) : same(&ps.texels[next + 4 * k], src + 4 * k, 32);
      next += gray ? np : 4 * np;
    } else {
      tex = tex && t.pad0 == 0 && same(t.value, s.value, 24);
    }
  }
  tex = tex && ps.texels.size() == (next ? next : 1);
  // the materials' slots: albedo, normal, roughness, metalness
  slots = slots && ps.mat_tex.size() == d.num_materials;
  for (uint32_t i = 0; slots && i < d.num_materials; i++) {
    const izpi_material& m = d.materials[i];
    const int32_t ids[4] = {m.albedo_tex, m.normal_tex, m.roughness_tex, m.metalness_tex};
    for (int k = 0; k < 4; k++) {
      const TexSlot& sl = ps.mat_tex[i].s[k];
      if (ids[k] < 0) slots = slots && sl.off == 0 && sl.w == 0 && sl.hf == (uint32_t)TEXF_NONE << 30;
      else if (d.textures[ids[k]].kind == IZPI_TEX_IMAGE) {
        const izpi_texture& t = ps.textures[ids[k]];
        slots = slots && sl.off == t.texel_offset && sl.w == t.width && sl.hf == (t.height | t.pad0 << 30);
      } else slots = slots && sl.off == (uint64_t)ids[k] && sl.w == 0 && sl.hf == (uint32_t)TEXF_OTHER << 30;
    }
  }
  char buf[256];
  snprintf(buf, sizeof buf, "refs=%d leaves=%d contains=%d rows=%d mk=%d lights=%d tex=%d slots=%d", refs, leaves, contains, rows, mk,
           lights, tex, slots);
  return buf;
}

void run(const char* name, const Desc& base, const std::function<void(Desc&)>& mutate, const izpi_host_scene* host = nullptr) {
  Desc c(base);
  c.fix();
  if (mutate) mutate(c);
  PackedScene ps;
  std::string err;
  const int rc = pack_scene(&c.d, &ps, &err);
  printf("%s|%d|%s|", name, rc, err.c_str());
  if (rc == IZPI_OK) {
    printf("quantized=%u leaf_shortcut=%u nan_free_bounds=%u time_free=%u no_pathlen=%u tri_only=%u mat_ok_rgb=%d mat_ok_spectral=%d "
           "basic_materials=%d matset=%u const_albedo=%d any_uv=%d gray_at=%llu rgba_at=%llu texels=%zu",
           ps.quantized, ps.leaf_shortcut, ps.nan_free_bounds, ps.time_free, ps.no_pathlen, ps.tri_only, ps.mat_ok_rgb, ps.mat_ok_spectral,
           ps.basic_materials, ps.matset, ps.const_albedo, ps.any_uv,
           ps.textures.size() > T_RGBA ? (unsigned long long)ps.textures[T_GRAY].texel_offset : 0ull,
           ps.textures.size() > T_RGBA ? (unsigned long long)ps.textures[T_RGBA].texel_offset : 0ull, ps.texels.size());
    if (host) printf(" stack=%d %s", ps.stack_needed == izpi_host_scene_stack_bound(host), structure(c.d, ps).c_str());
  }
  printf("\n");
}

}  // namespace

int main() {
  izpi_host_scene* hfull = build(true);
  izpi_host_scene* hbasic = build(false);
  if (!hfull || !hbasic) return 2;
  const Desc full(*izpi_host_scene_desc(hfull)), basic(*izpi_host_scene_desc(hbasic));
  uint32_t leaf = 0, tri_lambert = 0, tri_pbr = 0;  // a leaf node (the root is an inner node); triangles by material
  while (full.nodes[leaf].prim_count[0] <= 0) leaf++;
  while (full.tri_mat[tri_lambert] != M_LAMBERT) tri_lambert++;
  while (full.tri_mat[tri_pbr] != M_PBR) tri_pbr++;
  const uint32_t nt = full.d.num_tris, ns = full.d.num_spheres;

  // ---- valid scenes
  run("full", full, nullptr, hfull);
  run("full_quantized", full, [](Desc& c) { c.d.flags = IZPI_SCENE_QUANTIZED_BVH; }, hfull);
  run("basic", basic, nullptr, hbasic);
  run("basic_quantized", basic, [](Desc& c) { c.d.flags = IZPI_SCENE_QUANTIZED_BVH; }, hbasic);
  run("moving_sphere", full, [](Desc& c) { c.c1[3] += 1.0; }, hfull);
  run("camera_before_sphere", full, [](Desc& c) { c.d.camera.time0 = -1.0; }, hfull);
  run("nan_bound", full, [](Desc& c) { c.nodes[0].min_x[0] = NAN; });
  run("leaf_box_changed", full, [&](Desc& c) { c.nodes[leaf].max_x[0] = nextafterf(c.nodes[leaf].max_x[0], INFINITY); });
  run("leaf_box_changed_quantized", full, [&](Desc& c) {
    c.d.flags = IZPI_SCENE_QUANTIZED_BVH;
    c.nodes[leaf].max_x[0] = nextafterf(c.nodes[leaf].max_x[0], INFINITY);
  });
  run("no_rgb_albedo", full, [](Desc& c) { c.mats[M_LAMBERT].albedo_tex = -1; }, hfull);
  run("no_spectral_albedo", full, [](Desc& c) { c.mats[M_LAMBERT].spectral_tex = -1; }, hfull);

  // ---- every error return
  run("leaf_second_slot", full, [&](Desc& c) { c.nodes[leaf].child[1] = 0; });
  run("leaf_range", full, [&](Desc& c) { c.nodes[leaf].child[0] = (int32_t)c.d.num_prims; });
  run("leaf_count_8", full, [&](Desc& c) { c.nodes[leaf].child[0] = 0; c.nodes[leaf].prim_count[0] = 8; });
  run("inner_prim_slot", full, [](Desc& c) { c.nodes[0].prim_count[1] = 1; });
  run("child_index", full, [](Desc& c) { c.nodes[0].child[0] = (int32_t)c.d.num_nodes; });
  run("not_preorder", full, [](Desc& c) { c.nodes[0].child[0] = 0; });
  run("triangle_ref", full, [&](Desc& c) { for (uint32_t& r : c.prim_ref) if (IZPI_PRIM_KIND(r) == IZPI_PRIM_TRIANGLE) { r = IZPI_PRIM_REF(IZPI_PRIM_TRIANGLE, nt); break; } });
  run("sphere_ref", full, [&](Desc& c) { for (uint32_t& r : c.prim_ref) if (IZPI_PRIM_KIND(r) == IZPI_PRIM_SPHERE) { r = IZPI_PRIM_REF(IZPI_PRIM_SPHERE, ns); break; } });
  run("light_triangle_ref", full, [&](Desc& c) { c.light_ref[0] = IZPI_PRIM_REF(IZPI_PRIM_TRIANGLE, nt); });
  run("light_sphere_ref", full, [&](Desc& c) { c.light_ref[0] = IZPI_PRIM_REF(IZPI_PRIM_SPHERE, ns); });
  run("normal_mapped_light", full, [&](Desc& c) {
    c.mats[M_PBR].normal_tex = T_CONST;
    c.light_ref.push_back(IZPI_PRIM_REF(IZPI_PRIM_TRIANGLE, tri_pbr));
    c.fix();
  });
  run("texture_index", full, [](Desc& c) { c.mats[M_LAMBERT].albedo_tex = (int32_t)c.d.num_textures; });
  run("spectral_image_in_rgb_slot", full, [](Desc& c) { c.mats[M_PBR].roughness_tex = T_SPEC_IMG; });
  run("spectral_image_on_metal", full, [](Desc& c) { c.mats[M_METAL].spectral_tex = T_SPEC_IMG; });
  run("material_kind", full, [](Desc& c) { c.mats[M_METAL].kind = 99; });
  run("material_index_bvh", full, [&](Desc& c) { c.tri_mat[tri_lambert] = c.d.num_materials; });
  run("material_index_light", full, [&](Desc& c) {  // a light triangle the BVH does not reference
    for (std::vector<double>* v : {&c.v0, &c.v1, &c.v2, &c.e1, &c.e2, &c.nrm, &c.tg, &c.bt}) v->insert(v->end(), {0.0, 1.0, 0.0});
    c.uv.insert(c.uv.end(), {0.0, 0.0, 1.0, 0.0, 0.0, 1.0});
    c.area.push_back(0.5);
    c.tri_mat.push_back(c.d.num_materials + 5);
    c.light_ref.push_back(IZPI_PRIM_REF(IZPI_PRIM_TRIANGLE, nt));
    c.fix();
  });
  run("normal_map_without_tangents", full, [](Desc& c) { c.mats[M_PBR].normal_tex = T_CONST; c.d.tri_tangent = nullptr; });
  run("image_range", full, [](Desc& c) { c.texs[T_RGBA].texel_offset = c.d.num_texels; });
  run("spd_range", full, [](Desc& c) { c.texs[T_SPD_UNIFORM].spd_count = c.d.num_spd + 1; });
  izpi_host_scene_free(hfull);
  izpi_host_scene_free(hbasic);
  return 0;
}
