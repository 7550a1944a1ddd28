// scene_records.h — the records of the uploaded scene, as the host packs
// them (scene_pack.cpp) and the kernels read them (izpi_dev.h). Plain C++ (no HIP), so a host
// compiler can build and check the packer on its own (tests/scene_pack_check.cpp).
//
// HBM layout:
//   GInner  128 B  inner BVH4 nodes: SoA f32 bounds of 4 children + encoded child refs.
//                  (== hitable.BVH4Node, bvh4.go:23-39, with PrimitiveCount — always 0 in
//                  inner nodes — replaced by nothing; leaf children become leaf refs).
//   GLeaf   32 B   one per reference leaf node, indexed by its first primitive: its slot-0
//                  bounds + primitive range.
//                  A reference leaf node carries only slot 0 (bvh4.go:736-760), so the
//                  re-test on visit (quirk A10) needs 32 B instead of a 128 B node load.
//   GPrim   80 B   primitives in BVH leaf order: triangle v0,e1,e2 (the 72 B Hit reads,
//                  triangle.go:198-218) or sphere c0,c1,r,t0,t1; + kind/index.
//   shading data (normals, UVs, materials) stays in transport order and is read once per
//   closest hit, after traversal (deferred hit record).
#pragma once
#include <stdint.h>
#include "../../include/izpi_gpu.h"

#ifdef __HIPCC__
#define IZPI_REC_HD __host__ __device__
#else
#define IZPI_REC_HD
#endif

namespace izd {

// child ref encoding inside GInner / the traversal stack
//   r >= 0 : inner node index;   r == -1 : empty slot;   r <= -2 : leaf (below)
//   leaf refs carry the leaf's primitive range: r = -(1 + (start << 3 | count)), count 1..4
//   (bvh4.go:638-642 makes leaves of <= 4 primitives)
IZPI_REC_HD inline bool ref_is_leaf(int32_t r) { return r <= -2; }
IZPI_REC_HD inline int32_t leaf_start(int32_t r) { return (-r - 1) >> 3; }
IZPI_REC_HD inline int32_t leaf_count(int32_t r) { return (-r - 1) & 7; }
IZPI_REC_HD inline int32_t make_leaf_ref(int32_t start, int32_t count) { return -(1 + ((start << 3) | count)); }

struct alignas(16) GInner {
  float mnx[4], mny[4], mnz[4], mxx[4], mxy[4], mxz[4];
  int32_t child[4];
  int32_t pad[4];
};
static_assert(sizeof(GInner) == 128, "GInner is 128 B");
// An inner node with its child boxes quantised (IZPI_SCENE_QUANTIZED_BVH), 64 B: two per
// 128-B line, four 16-B loads per visit instead of seven. Bound b of child i on axis a is
// org[a] + q * 2^(e[a] - 127), q = byte i of the bound's word: the product is exact (q < 256,
// a normal power of two), so a fused multiply-add decodes it bit for bit as the upload's
// `org + (float)q * s` does (qdecode). Child refs as in GInner.
struct alignas(64) GInnerQ {
  float org[3];
  uint32_t ex;        // biased exponents: x bits 0-7, y 8-15, z 16-23
  uint32_t q[6];      // mnx, mny, mnz, mxx, mxy, mxz: byte i = child i
  int32_t child[4];
  uint32_t pad[2];
};
static_assert(sizeof(GInnerQ) == 64, "GInnerQ is 64 B");
// The upload's decoding of one quantised bound (host), which the kernels' fmaf reproduces.
IZPI_REC_HD inline float qdecode(float org, uint32_t q, float s) {
  const float p = (float)q * s;  // exact
  return org + p;
}
struct alignas(16) GLeaf {
  float mn[3], mx[3];
  int32_t start, count;
};
static_assert(sizeof(GLeaf) == 32, "GLeaf is 32 B");
struct alignas(16) GPrim {
  double a[9];      // tri: v0[3] e1[3] e2[3];  sphere: c0[3] c1[3] radius t0 t1
  uint32_t kind;    // IZPI_PRIM_*
  uint32_t index;   // transport-order index (shading data, lights)
};
static_assert(sizeof(GPrim) == 80, "GPrim is 80 B");
// Shading record of a primitive, in BVH leaf order next to GPrim: everything the
// deferred hit record needs, in 32 B (half a 64-B line: one sector per closest hit). The
// material's constant RGB albedo / emit value, when it has one, is in DevScene::mat_const.
struct alignas(32) GShade {
  double n[3];      // triangle: unit(e1 x e2) (triangle.go:100); sphere: unused
  uint32_t ref;     // IZPI_PRIM_REF(kind, transport index)
  uint32_t mk;      // material index << 8 | material kind << 2 | cflags
                    // (cflags bit0: mat_const holds the albedo; bit1: a texture of the material reads the hit (u,v))
};
static_assert(sizeof(GShade) == 32, "GShade is 32 B");
IZPI_REC_HD inline uint32_t gs_mat(const GShade& g) { return g.mk >> 8; }
IZPI_REC_HD inline uint32_t gs_kind(const GShade& g) { return (g.mk >> 2) & 63u; }
IZPI_REC_HD inline uint32_t gs_cflags(const GShade& g) { return g.mk & 3u; }
// Texture-space data of a triangle, in BVH leaf order next to GShade (a hit's primitive
// indexes it directly, so it loads in parallel with GShade instead of after it): the
// vertex UVs (triangle.go:61-134) and the tangent / bitangent of the normal map's TBN
// (triangle.go:250-264). Uploaded only for scenes with image textures or normal maps.
struct alignas(16) GTriTex {
  double uv[6];     // u0, v0, u1, v1, u2, v2
  double tg[3], bt[3];
};
static_assert(sizeof(GTriTex) == 96, "GTriTex is 96 B");
// A triangle's second and third vertex as uploaded, in BVH leaf order (GPrim holds v0 and the
// edges): Triangle.HitEdge tests the hit point against the sides v0v1, v1v2, v2v0
// (triangle.go:282-302), and v0 + e1 is not bit for bit v1. Read by the WireFrame sampler only.
struct alignas(16) GTriVerts {
  double v1[3], v2[3];
};
static_assert(sizeof(GTriVerts) == 48, "GTriVerts is 48 B");
// Light record (Scene.Lights entry, transport order): everything PDFValue/Random read.
struct alignas(16) GLight {
  double v0[3], v1[3], v2[3], e1[3], e2[3], n[3];  // triangle
  double area;
  double c0[3], c1[3], radius, t0, t1;             // sphere
  double cz[3];                                    // sphere: center(0), the PDFValue ray's time
  uint32_t kind, index;
};
static_assert(sizeof(GLight) == 256, "GLight is 256 B");

// An image texture's texels in their device storage form (pack_scene repacks
// each IMAGE texture): RGBA = 4 doubles per texel as uploaded, GRAY = 1 double per texel
// for a texture whose every texel has R, G and B bit-identical (a roughness or metalness
// map): the lookup returns the same three values from an 8-B read instead of a 32-B one.
enum { TEXF_RGBA = 0, TEXF_GRAY = 1, TEXF_OTHER = 2, TEXF_NONE = 3 };
// One texture slot of a material (DevScene::mat_tex), resolved at upload so that a hit
// reads its material's textures with one dependent load less (material -> texels instead
// of material -> texture record -> texels): off = first texel (doubles into
// DevScene::texels), w, hf = height | format << 30. TEXF_OTHER: a non-image texture, off =
// its index into DevScene::textures; TEXF_NONE: no texture (-1).
struct alignas(16) TexSlot {
  uint64_t off;
  uint32_t w, hf;
};
static_assert(sizeof(TexSlot) == 16, "TexSlot is 16 B");
// Slots 0..3: albedo, normal map, roughness, metalness (the PBR set, pbr.go:20-56).
struct alignas(64) MatTex {
  TexSlot s[4];
};
static_assert(sizeof(MatTex) == 64, "MatTex is 64 B");

// The material kinds a scene holds beyond Lambertian + DiffuseLight, as feature bits: the
// packer sets them (PackedScene::matset) and the shading instances are compiled per set
// (MATSET_*, izpi_kern.h). MS_CONST marks the constant-albedo instance, not a kind.
enum { MS_DIEL = 1, MS_METAL = 2, MS_PBR = 4, MS_ISO = 8, MS_CONST = 16 };

}  // namespace izd
