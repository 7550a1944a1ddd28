// scene_pack.cpp — the host half of izpi_gpu_upload_scene (scene_pack.h): every check of
// the caller's descriptor and every record of DESIGN.md §2.1, in one step per purpose.
// Every index is checked before it is used, and nothing here knows of a device.
#include "scene_pack.h"

#include <string.h>
#include <algorithm>
#include <cmath>

namespace izpi_internal {

using namespace izd;

bool stack_bound(const izpi_bvh4_node* nodes, size_t n, uint32_t* bound) {
  std::vector<uint32_t> best(n, 0);
  for (size_t k = n; k-- > 0;) {
    const izpi_bvh4_node& nd = nodes[k];
    if (nd.prim_count[0] > 0) continue;  // a leaf pushes nothing
    uint32_t valid = 0, deepest = 0;
    for (int i = 0; i < 4; i++) {
      if (nd.child[i] < 0) continue;
      valid++;
      if ((uint32_t)nd.child[i] <= k) return false;
      deepest = std::max(deepest, best[(size_t)nd.child[i]]);
    }
    best[k] = (valid ? valid - 1 : 0) + deepest;
  }
  *bound = n ? best[0] : 0;
  return true;
}

namespace {

int fail(std::string* err, int rc, const char* what) {
  *err = what;
  return rc;
}

// ---- BVH4: split the reference nodes into inner nodes and leaf records. ref[k] is node
// k's encoded ref (child ref encoding, scene_records.h).
int split_bvh(const izpi_scene_desc* d, PackedScene* out, std::vector<int32_t>& ref, std::string* err) {
  ref.assign(d->num_nodes, 0);
  uint32_t n_inner = 0;
  for (uint32_t k = 0; k < d->num_nodes; k++) {
    const izpi_bvh4_node& n = d->nodes[k];
    if (n.prim_count[0] > 0) {
      for (int i = 1; i < 4; i++)
        if (n.child[i] != -1) return fail(err, IZPI_ERR_INVALID, "leaf node with more than one slot");
      const int32_t st = n.child[0], cnt = n.prim_count[0];
      if (st < 0 || (uint64_t)st + (uint64_t)cnt > d->num_prims) return fail(err, IZPI_ERR_INVALID, "leaf primitive range out of bounds");
      if (cnt > 7 || st >= (1 << 27)) return fail(err, IZPI_ERR_UNSUPPORTED, "leaf too large for the leaf-ref encoding");
      ref[k] = make_leaf_ref(st, cnt);
      out->leaf_max = std::max(out->leaf_max, (uint32_t)cnt);
    } else {
      for (int i = 0; i < 4; i++)
        if (n.prim_count[i] != 0) return fail(err, IZPI_ERR_INVALID, "inner node with a primitive slot");
      ref[k] = (int32_t)n_inner++;
    }
  }
  out->num_inner = n_inner;
  out->root = d->num_nodes ? ref[0] : -1;
  out->inner.assign(std::max<uint32_t>(1, n_inner), GInner{});
  out->leaves.assign(std::max<uint32_t>(1, d->num_prims), GLeaf{});
  out->leaf_shortcut = 1;
  for (uint32_t k = 0; k < d->num_nodes; k++) {
    const izpi_bvh4_node& n = d->nodes[k];
    if (ref[k] <= -2) {
      GLeaf& L = out->leaves[(size_t)leaf_start(ref[k])];
      L.mn[0] = n.min_x[0]; L.mn[1] = n.min_y[0]; L.mn[2] = n.min_z[0];
      L.mx[0] = n.max_x[0]; L.mx[1] = n.max_y[0]; L.mx[2] = n.max_z[0];
      L.start = n.child[0]; L.count = n.prim_count[0];
    } else {
      GInner& g = out->inner[(size_t)ref[k]];
      memcpy(g.mnx, n.min_x, 16); memcpy(g.mny, n.min_y, 16); memcpy(g.mnz, n.min_z, 16);
      memcpy(g.mxx, n.max_x, 16); memcpy(g.mxy, n.max_y, 16); memcpy(g.mxz, n.max_z, 16);
      for (int i = 0; i < 4; i++) {
        int32_t c = n.child[i];
        if (c != -1 && (c < 0 || (uint32_t)c >= d->num_nodes)) return fail(err, IZPI_ERR_INVALID, "child index out of bounds");
        g.child[i] = c == -1 ? -1 : ref[(size_t)c];
        g.pad[i] = 0;
        if (c >= 0 && ref[(size_t)c] <= -2) {
          // a leaf's re-test (A10) may be skipped only if its slot-0 box is bit-identical
          // to this slot's box (flattenBVH4 converts the same node.box twice, bvh4.go:745-781)
          const izpi_bvh4_node& lnode = d->nodes[(size_t)c];
          const float pb[6] = {n.min_x[i], n.min_y[i], n.min_z[i], n.max_x[i], n.max_y[i], n.max_z[i]};
          const float lb[6] = {lnode.min_x[0], lnode.min_y[0], lnode.min_z[0], lnode.max_x[0], lnode.max_y[0], lnode.max_z[0]};
          if (memcmp(pb, lb, sizeof(pb)) != 0) out->leaf_shortcut = 0;
        }
      }
    }
  }
  return IZPI_OK;
}

// Quantise inner node g's child boxes (IZPI_SCENE_QUANTIZED_BVH) into q and replace g's
// valid slot boxes by the decoded ones. Per axis: the origin is the minimum over the valid
// children's mins, the scale 2^e the smallest for which every child's bounds, rounded
// outwards to the grid, fit a byte; each rounded bound is then checked in the kernels' own
// f32 decode (qdecode) and moved one step outwards while it would not contain the exact
// bound. False when a valid bound is not finite or no exponent fits (the scene then keeps
// its exact boxes).
bool quantize_node(GInner& g, GInnerQ& q) {
  memset(&q, 0, sizeof(q));
  float* mn[3] = {g.mnx, g.mny, g.mnz};
  float* mx[3] = {g.mxx, g.mxy, g.mxz};
  for (int i = 0; i < 4; i++) q.child[i] = g.child[i];
  for (int a = 0; a < 3; a++) {
    float lo = 0.0f, hi = 0.0f;
    bool any = false;
    for (int i = 0; i < 4; i++) {
      if (g.child[i] == -1) continue;
      if (!std::isfinite(mn[a][i]) || !std::isfinite(mx[a][i])) return false;
      lo = any ? std::min(lo, mn[a][i]) : mn[a][i];
      hi = any ? std::max(hi, mx[a][i]) : mx[a][i];
      any = true;
    }
    const double ext = (double)hi - (double)lo;
    int e = -126;
    if (ext > 0) e = std::max(-126, (int)std::ceil(std::log2(ext / 255.0)));
    uint32_t qlo[4] = {0, 0, 0, 0}, qhi[4] = {0, 0, 0, 0};
    for (;; e++) {
      if (e > 127) return false;
      const float sc = std::ldexp(1.0f, e);
      bool ok = true;
      for (int i = 0; i < 4 && ok; i++) {
        if (g.child[i] == -1) continue;
        double fl = std::floor(((double)mn[a][i] - (double)lo) / (double)sc);
        int ql = (int)std::min(255.0, std::max(0.0, fl));
        while (ql > 0 && qdecode(lo, (uint32_t)ql, sc) > mn[a][i]) ql--;  // qdecode(lo, 0) == lo <= every min
        double fh = std::ceil(((double)mx[a][i] - (double)lo) / (double)sc);
        int qh = (int)std::max((double)ql, std::min(256.0, fh));
        while (qh <= 255 && qdecode(lo, (uint32_t)qh, sc) < mx[a][i]) qh++;
        if (qh > 255) ok = false;
        qlo[i] = (uint32_t)ql; qhi[i] = (uint32_t)qh;
      }
      if (ok) break;
    }
    const float sc = std::ldexp(1.0f, e);
    q.org[a] = lo;
    q.ex |= (uint32_t)(e + 127) << (8 * a);
    for (int i = 0; i < 4; i++) {
      q.q[a] |= qlo[i] << (8 * i);
      q.q[3 + a] |= qhi[i] << (8 * i);
      if (g.child[i] == -1) continue;
      mn[a][i] = qdecode(lo, qlo[i], sc);
      mx[a][i] = qdecode(lo, qhi[i], sc);
    }
  }
  return true;
}

// ---- quantised child boxes (IZPI_SCENE_QUANTIZED_BVH, ABI 3): `inner` and the leaf
// records take the decoded boxes, which every traversal instance then tests (the 64-B
// nodes and the 128-B ones describe the same tree); a leaf's re-test box is its decoded
// parent slot, so its shortcut holds
void quantize_bvh(const izpi_scene_desc* d, PackedScene* out) {
  const uint32_t n_inner = out->num_inner;
  out->quantized = 0;
  if (!(d->abi_version >= 3 && (d->flags & IZPI_SCENE_QUANTIZED_BVH) && n_inner > 0)) return;
  std::vector<GInner> dec(out->inner);
  out->innerq.resize(n_inner);
  bool quantized = true;
  for (uint32_t k = 0; k < n_inner && quantized; k++) quantized = quantize_node(dec[k], out->innerq[k]);
  if (!quantized) {
    out->innerq.clear();
    return;
  }
  out->inner.swap(dec);
  for (uint32_t k = 0; k < n_inner; k++) {
    const GInner& g = out->inner[k];
    for (int i = 0; i < 4; i++) {
      if (!ref_is_leaf(g.child[i])) continue;
      GLeaf& L = out->leaves[(size_t)leaf_start(g.child[i])];
      L.mn[0] = g.mnx[i]; L.mn[1] = g.mny[i]; L.mn[2] = g.mnz[i];
      L.mx[0] = g.mxx[i]; L.mx[1] = g.mxy[i]; L.mx[2] = g.mxz[i];
    }
  }
  out->leaf_shortcut = 1;
  out->quantized = 1;
}

// ---- primitives in leaf order: the intersection record, the shading record (gs.mk holds
// the bare material index until finish_shade), the triangles' v1, v2 (Triangle.HitEdge's
// sides: the WireFrame sampler) and, when the descriptor has them, the triangles' UVs and
// tangent frames (shading reads them for image textures and normal maps; izpi_gpu_trace's
// hit records carry the UVs)
int pack_prims(const izpi_scene_desc* d, PackedScene* out, std::string* err) {
  const uint32_t nt = d->num_tris, ns = d->num_spheres;
  const bool tex = d->num_prims && (d->tri_uv || d->tri_tangent || d->tri_bitangent);
  out->prims.assign(d->num_prims, GPrim{});
  out->shade.assign(d->num_prims, GShade{});
  out->triverts.assign(std::max<uint32_t>(1, d->num_prims), GTriVerts{});
  out->tritex.assign(tex ? d->num_prims : 0, GTriTex{});
  for (uint32_t k = 0; k < d->num_prims; k++) {
    const uint32_t r = d->prim_ref[k], kind = IZPI_PRIM_KIND(r);
    const size_t idx = IZPI_PRIM_INDEX(r);
    GPrim& g = out->prims[k];
    g.kind = kind; g.index = (uint32_t)idx;
    GShade& gs = out->shade[k];
    gs.ref = r;
    if (kind == IZPI_PRIM_TRIANGLE) {
      if (idx >= nt) return fail(err, IZPI_ERR_INVALID, "triangle ref out of range");
      memcpy(gs.n, d->tri_normal + 3 * idx, 24);
      gs.mk = d->tri_mat[idx];
      memcpy(g.a, d->tri_v0 + 3 * idx, 24); memcpy(g.a + 3, d->tri_e1 + 3 * idx, 24);
      memcpy(g.a + 6, d->tri_e2 + 3 * idx, 24);
      memcpy(out->triverts[k].v1, d->tri_v1 + 3 * idx, 24);
      memcpy(out->triverts[k].v2, d->tri_v2 + 3 * idx, 24);
      if (tex && d->tri_uv) memcpy(out->tritex[k].uv, d->tri_uv + 6 * idx, 48);
      if (tex && d->tri_tangent) memcpy(out->tritex[k].tg, d->tri_tangent + 3 * idx, 24);
      if (tex && d->tri_bitangent) memcpy(out->tritex[k].bt, d->tri_bitangent + 3 * idx, 24);
    } else {
      if (idx >= ns) return fail(err, IZPI_ERR_INVALID, "sphere ref out of range");
      gs.mk = d->sph_mat[idx];
      memcpy(g.a, d->sph_center0 + 3 * idx, 24); memcpy(g.a + 3, d->sph_center1 + 3 * idx, 24);
      g.a[6] = d->sph_radius[idx]; g.a[7] = d->sph_time[2 * idx]; g.a[8] = d->sph_time[2 * idx + 1];
    }
  }
  return IZPI_OK;
}

// ---- lights (transport order; a light need not be a primitive of the BVH)
int pack_lights(const izpi_scene_desc* d, PackedScene* out, std::string* err) {
  out->lights.assign(d->num_lights, GLight{});
  for (uint32_t i = 0; i < d->num_lights; i++) {
    GLight& L = out->lights[i];
    const uint32_t r = d->light_ref[i], kind = IZPI_PRIM_KIND(r);
    const size_t idx = IZPI_PRIM_INDEX(r);
    L.kind = kind; L.index = (uint32_t)idx;
    if (kind == IZPI_PRIM_TRIANGLE) {
      if (idx >= d->num_tris) return fail(err, IZPI_ERR_INVALID, "light triangle out of range");
      if (d->tri_mat[idx] >= d->num_materials) return fail(err, IZPI_ERR_INVALID, "material index out of range");
      const izpi_material& m = d->materials[d->tri_mat[idx]];
      if (m.kind == IZPI_MAT_PBR && m.normal_tex >= 0) return fail(err, IZPI_ERR_UNSUPPORTED, "normal-mapped light");
      memcpy(L.v0, d->tri_v0 + 3 * idx, 24); memcpy(L.v1, d->tri_v1 + 3 * idx, 24);
      memcpy(L.v2, d->tri_v2 + 3 * idx, 24); memcpy(L.e1, d->tri_e1 + 3 * idx, 24);
      memcpy(L.e2, d->tri_e2 + 3 * idx, 24); memcpy(L.n, d->tri_normal + 3 * idx, 24);
      L.area = d->tri_area[idx];
    } else {
      if (idx >= d->num_spheres) return fail(err, IZPI_ERR_INVALID, "light sphere out of range");
      memcpy(L.c0, d->sph_center0 + 3 * idx, 24); memcpy(L.c1, d->sph_center1 + 3 * idx, 24);
      L.radius = d->sph_radius[idx]; L.t0 = d->sph_time[2 * idx]; L.t1 = d->sph_time[2 * idx + 1];
      // Sphere.center(0) (sphere.go:125-127) with the device's operation order:
      // c0 + (c1 - c0) * ((0 - t0) / (t1 - t0)), computed once here
      const double k = (0.0 - L.t0) / (L.t1 - L.t0);
      for (int q = 0; q < 3; q++) L.cz[q] = L.c0[q] + (L.c1[q] - L.c0[q]) * k;
    }
  }
  return IZPI_OK;
}

// ---- material classification. mflags[i]: bit0 a texture of material i reads (u,v); bit1
// usable by the Colour sampler; bit2 usable by the Spectral sampler (the reference would
// dereference a nil texture otherwise).
int classify_materials(const izpi_scene_desc* d, PackedScene* out, std::vector<uint32_t>& mflags, std::string* err) {
  mflags.assign(d->num_materials, 0);
  out->mat_ok_rgb = out->mat_ok_spectral = true;
  out->basic_materials = true;
  out->matset = 0;
  out->any_uv = false;
  out->no_pathlen = 1;
  for (uint32_t i = 0; i < d->num_materials; i++) {
    const izpi_material& m = d->materials[i];
    const int32_t ids[] = {m.albedo_tex, m.spectral_tex, m.normal_tex, m.roughness_tex, m.metalness_tex, m.absorb_tex};
    for (int32_t t : ids) {
      if (t < -1 || t >= (int32_t)d->num_textures) return fail(err, IZPI_ERR_INVALID, "texture index out of range");
      if (t >= 0 && (d->textures[t].kind == IZPI_TEX_IMAGE || d->textures[t].kind == IZPI_TEX_SPECTRAL_IMAGE)) mflags[i] |= 1u;
    }
    // a SpectralImage is made for PBR albedos (transport.go:486-497) and reads the hit's
    // (u, v): Lambert / DiffuseLight / PBR spectral textures only
    for (int32_t t : {m.normal_tex, m.roughness_tex, m.metalness_tex, m.absorb_tex, m.albedo_tex})
      if (t >= 0 && d->textures[t].kind == IZPI_TEX_SPECTRAL_IMAGE) return fail(err, IZPI_ERR_INVALID, "SpectralImage outside a spectral albedo");
    if (m.spectral_tex >= 0 && d->textures[m.spectral_tex].kind == IZPI_TEX_SPECTRAL_IMAGE && m.kind != IZPI_MAT_LAMBERT &&
        m.kind != IZPI_MAT_DIFFUSE_LIGHT && m.kind != IZPI_MAT_PBR)
      return fail(err, IZPI_ERR_INVALID, "SpectralImage outside a spectral albedo");
    auto is_rgb = [&](int32_t t) { return t >= 0 && (d->textures[t].kind == IZPI_TEX_CONSTANT || d->textures[t].kind == IZPI_TEX_IMAGE); };
    auto is_spec = [&](int32_t t) {
      return t >= 0 && (d->textures[t].kind == IZPI_TEX_SPECTRAL_GAUSSIAN || d->textures[t].kind == IZPI_TEX_SPECTRAL_TABULATED ||
                        d->textures[t].kind == IZPI_TEX_SPECTRAL_IMAGE);
    };
    auto opt_rgb = [&](int32_t t) { return t == -1 || is_rgb(t); };
    bool rgb = false, spec = false;
    switch (m.kind) {
      case IZPI_MAT_LAMBERT: case IZPI_MAT_DIFFUSE_LIGHT: rgb = is_rgb(m.albedo_tex); spec = is_spec(m.spectral_tex); break;
      case IZPI_MAT_DIELECTRIC: rgb = true; spec = is_spec(m.spectral_tex) && (m.absorb_tex == -1 || is_spec(m.absorb_tex)); break;
      case IZPI_MAT_METAL: rgb = spec = true; break;
      case IZPI_MAT_ISOTROPIC: rgb = spec = is_rgb(m.albedo_tex); break;  // SpectralScatter reads the RGB albedo's X
      case IZPI_MAT_PBR: {
        bool aux = opt_rgb(m.normal_tex) && opt_rgb(m.roughness_tex) && opt_rgb(m.metalness_tex);
        rgb = aux && is_rgb(m.albedo_tex);
        spec = aux && (is_spec(m.spectral_tex) || is_rgb(m.albedo_tex));
        break;
      }
      default: return fail(err, IZPI_ERR_INVALID, "unknown material kind");
    }
    if (m.kind != IZPI_MAT_LAMBERT && m.kind != IZPI_MAT_DIFFUSE_LIGHT) out->basic_materials = false;
    if (m.kind == IZPI_MAT_DIELECTRIC) out->no_pathlen = 0;  // else every traced ray is a sampler ray
    out->matset |= m.kind == IZPI_MAT_DIELECTRIC ? MS_DIEL : m.kind == IZPI_MAT_METAL ? MS_METAL
                 : m.kind == IZPI_MAT_PBR ? MS_PBR : m.kind == IZPI_MAT_ISOTROPIC ? MS_ISO : 0u;
    if (mflags[i] & 1u) out->any_uv = true;
    if (rgb) mflags[i] |= 2u; else out->mat_ok_rgb = false;
    if (spec) mflags[i] |= 4u; else out->mat_ok_spectral = false;
  }
  return IZPI_OK;
}

// ---- material essentials in the per-primitive shade records: mat_const, and gs.mk from
// the bare material index to index << 8 | kind << 2 | cflags (every kind is below 64:
// classify_materials)
int finish_shade(const izpi_scene_desc* d, PackedScene* out, const std::vector<uint32_t>& mflags, std::string* err) {
  if (d->num_materials >= (1u << 24)) return fail(err, IZPI_ERR_INVALID, "too many materials");
  out->mat_const.assign(std::max<uint32_t>(1, d->num_materials), Double4{0, 0, 0, 0});
  std::vector<uint32_t> mcflags(d->num_materials, 0);
  out->const_albedo = true;
  for (uint32_t i = 0; i < d->num_materials; i++) {
    const izpi_material& m = d->materials[i];
    const bool diffuse = m.kind == IZPI_MAT_LAMBERT || m.kind == IZPI_MAT_DIFFUSE_LIGHT;
    mcflags[i] = (mflags[i] & 1u) ? 2u : 0u;
    if (diffuse && m.albedo_tex >= 0 && d->textures[m.albedo_tex].kind == IZPI_TEX_CONSTANT) {
      const double* v = d->textures[m.albedo_tex].value;
      out->mat_const[i] = Double4{v[0], v[1], v[2], 0.0};
      mcflags[i] |= 1u;
    } else if (diffuse) {
      out->const_albedo = false;
    }
  }
  for (GShade& gs : out->shade) {
    const uint32_t mat = gs.mk;
    if (mat >= d->num_materials) return fail(err, IZPI_ERR_INVALID, "material index out of range");
    gs.mk = mat << 8 | d->materials[mat].kind << 2 | mcflags[mat];
  }
  for (uint32_t i = 0; i < d->num_materials; i++)
    if (d->materials[i].kind == IZPI_MAT_PBR && d->materials[i].normal_tex >= 0 && d->num_tris && (!d->tri_tangent || !d->tri_bitangent))
      return fail(err, IZPI_ERR_INVALID, "a PBR normal map needs the triangles' tangents and bitangents");
  return IZPI_OK;
}

// ---- textures in their device form, the texels repacked, and the materials' slots
int pack_textures(const izpi_scene_desc* d, PackedScene* out, std::string* err) {
  for (uint32_t i = 0; i < d->num_textures; i++) {
    const izpi_texture& t = d->textures[i];
    if (t.kind != IZPI_TEX_IMAGE && t.kind != IZPI_TEX_SPECTRAL_IMAGE) continue;
    if (t.width == 0 || t.height == 0 || t.texel_offset + 4ull * t.width * t.height > d->num_texels || !d->texels)
      return fail(err, IZPI_ERR_INVALID, "image texture outside the texel array");
  }
  // pad0 = 1 marks a tabulated SPD with non-decreasing wavelengths, which tex_spectral
  // searches by bisection; pad0 = 2 one whose wavelengths are also near-uniform (entry j
  // within half a step of wl[0] + j * step), whose interval tex_spectral guesses from lambda
  // with value[0] = wl[0] and value[1] = 1 / step
  std::vector<izpi_texture>& texs = out->textures;
  texs.assign(d->textures, d->textures + d->num_textures);
  for (izpi_texture& t : texs) {
    t.pad0 = 0;
    if (t.kind != IZPI_TEX_SPECTRAL_TABULATED || t.spd_count < 2) continue;  // n = 1: the scan returns 0.0
    if ((uint64_t)t.spd_offset + t.spd_count > d->num_spd) return fail(err, IZPI_ERR_INVALID, "SPD range out of bounds");
    const double* wl = d->spd_wavelengths + t.spd_offset;
    const uint32_t n = t.spd_count;
    bool sorted = true;
    for (uint32_t i = 1; i < n; i++)
      if (!(wl[i - 1] <= wl[i])) sorted = false;
    t.pad0 = sorted ? 1u : 0u;
    const double span = wl[n - 1] - wl[0];
    if (!sorted || !(span > 0) || !std::isfinite(span)) continue;
    const double scale = (double)(n - 1) / span;
    bool uniform = std::isfinite(scale);
    for (uint32_t i = 0; i < n && uniform; i++)
      if (!(std::fabs((wl[i] - wl[0]) * scale - (double)i) <= 0.5)) uniform = false;
    if (uniform) { t.pad0 = 2; t.value[0] = wl[0]; t.value[1] = scale; }
  }
  // texels in their device storage form (TexSlot): every image texture gets its own run,
  // RGBA runs 32-B aligned; a texture whose R, G and B are bit-identical in every texel is
  // stored as one double per texel
  std::vector<double>& texels = out->texels;
  texels.clear();
  std::vector<uint32_t> tex_fmt(d->num_textures, TEXF_OTHER);
  for (uint32_t i = 0; i < d->num_textures; i++) {
    izpi_texture& t = texs[i];
    if (t.kind != IZPI_TEX_IMAGE && t.kind != IZPI_TEX_SPECTRAL_IMAGE) continue;
    const double* src = d->texels + t.texel_offset;
    const uint64_t np = (uint64_t)t.width * t.height;
    bool gray = t.kind == IZPI_TEX_IMAGE;
    for (uint64_t k = 0; k < np && gray; k++)
      gray = memcmp(src + 4 * k, src + 4 * k + 1, 8) == 0 && memcmp(src + 4 * k, src + 4 * k + 2, 8) == 0;
    texels.resize((texels.size() + 3) & ~(size_t)3);
    t.texel_offset = texels.size();
    if (gray) {
      for (uint64_t k = 0; k < np; k++) texels.push_back(src[4 * k]);
    } else {
      texels.insert(texels.end(), src, src + 4 * np);
    }
    if (t.kind == IZPI_TEX_IMAGE) t.pad0 = tex_fmt[i] = gray ? TEXF_GRAY : TEXF_RGBA;
  }
  if (texels.empty()) texels.push_back(0.0);
  // the materials' texture slots (albedo, normal, roughness, metalness)
  out->mat_tex.assign(std::max<uint32_t>(1, d->num_materials), MatTex{});
  for (uint32_t i = 0; i < d->num_materials; i++) {
    const izpi_material& m = d->materials[i];
    const int32_t ids[4] = {m.albedo_tex, m.normal_tex, m.roughness_tex, m.metalness_tex};
    for (int k = 0; k < 4; k++) {
      TexSlot& sl = out->mat_tex[i].s[k];
      const int32_t id = ids[k];
      if (id < 0) { sl.off = 0; sl.w = 0; sl.hf = (uint32_t)TEXF_NONE << 30; continue; }
      const izpi_texture& t = texs[id];
      if (tex_fmt[id] <= TEXF_GRAY && t.height < (1u << 30)) {
        sl.off = t.texel_offset; sl.w = t.width; sl.hf = t.height | tex_fmt[id] << 30;
      } else {
        sl.off = (uint64_t)id; sl.w = 0; sl.hf = (uint32_t)TEXF_OTHER << 30;
      }
    }
  }
  return IZPI_OK;
}

// ---- the scene's flags that come from its geometry
void scene_flags(const izpi_scene_desc* d, PackedScene* out) {
  out->tri_only = d->num_spheres == 0 ? 1u : 0u;
  // time_free: no sphere moves, so Sphere.center(time) == center(time0) for every ray time
  // (c1 == c0 finite: (c1 - c0) * x = +0 for the x >= 0 every camera time gives)
  bool tf = true;
  const double tmin_cam = std::min(d->camera.time0, d->camera.time1);
  if (!std::isfinite(d->camera.time0) || !std::isfinite(d->camera.time1)) tf = false;
  for (uint32_t i = 0; tf && i < d->num_spheres; i++) {
    const double* c0 = d->sph_center0 + 3 * (size_t)i;
    const double* c1 = d->sph_center1 + 3 * (size_t)i;
    const double t0 = d->sph_time[2 * (size_t)i], t1 = d->sph_time[2 * (size_t)i + 1];
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(c0[k]) || memcmp(c0 + k, c1 + k, sizeof(double)) != 0) tf = false;
    if (!std::isfinite(t0) || !std::isfinite(t1) || !(t1 > t0) || !(tmin_cam >= t0)) tf = false;
  }
  out->time_free = tf ? 1u : 0u;
  out->nan_free_bounds = 1;
  for (const GInner& g : out->inner) {
    const float* f = g.mnx;  // the 24 bounds are contiguous
    for (int i = 0; i < 24; i++) if (f[i] != f[i]) out->nan_free_bounds = 0;
  }
  for (const GLeaf& L : out->leaves)  // leaf re-tests run through the same 4-slot test
    for (int i = 0; i < 3; i++) if (L.mn[i] != L.mn[i] || L.mx[i] != L.mx[i]) out->nan_free_bounds = 0;
  // ordered_bounds: mn <= mx on every axis of every valid slot and of every leaf box (an empty
  // slot's box is read by no sorted test's result: k_trace2 masks it by its child)
  out->ordered_bounds = 1;
  for (const GInner& g : out->inner)
    for (int i = 0; i < 4; i++)
      if (g.child[i] != -1 && !(g.mnx[i] <= g.mxx[i] && g.mny[i] <= g.mxy[i] && g.mnz[i] <= g.mxz[i])) out->ordered_bounds = 0;
  for (const GLeaf& L : out->leaves)
    for (int i = 0; i < 3; i++) if (!(L.mn[i] <= L.mx[i])) out->ordered_bounds = 0;
}

}  // namespace

int pack_scene(const izpi_scene_desc* d, PackedScene* out, std::string* err) {
  *out = PackedScene();
  std::vector<int32_t> ref;
  std::vector<uint32_t> mflags;
  int rc = split_bvh(d, out, ref, err);
  if (!rc) quantize_bvh(d, out);
  if (!rc) rc = pack_prims(d, out, err);
  if (!rc) rc = pack_lights(d, out, err);
  if (!rc) rc = classify_materials(d, out, mflags, err);
  if (!rc) rc = finish_shade(d, out, mflags, err);
  if (!rc) rc = pack_textures(d, out, err);
  if (rc) return rc;
  scene_flags(d, out);
  if (!stack_bound(d->nodes, d->num_nodes, &out->stack_needed)) return fail(err, IZPI_ERR_INVALID, "BVH4 nodes not in pre-order");
  return IZPI_OK;
}

}  // namespace izpi_internal
