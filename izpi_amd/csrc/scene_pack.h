// scene_pack.h — izpi_scene_desc -> the arrays and flags izpi_gpu_upload_scene copies to the
// device. Plain C++ (no HIP, no izpi_ctx): the whole of the upload's validation, repacking
// and material classification, so a host compiler can build and check it on its own
// (tests/scene_pack_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "scene_records.h"

namespace izpi_internal {

struct Double4 { double x, y, z, w; };  // a device double4's four doubles

// One scene in its device form. The arrays the device reads as the caller gave them
// (materials, the SPD tables, the camera) are not copied here: the uploader takes them from
// the descriptor.
struct PackedScene {
  std::vector<izd::GInner> inner;        // >= 1 record: k_trace2's leaf lanes read a dummy inner node
  std::vector<izd::GInnerQ> innerq;      // `inner` quantised (then `inner` holds the decoded boxes), else empty
  std::vector<izd::GLeaf> leaves;        // >= 1, indexed by first primitive
  std::vector<izd::GPrim> prims;         // leaf order, as shade
  std::vector<izd::GShade> shade;
  std::vector<izd::GTriVerts> triverts;  // >= 1, leaf order: the triangles' v1, v2 (the WireFrame sampler)
  std::vector<izd::GTriTex> tritex;      // leaf order, or empty: the descriptor has no UVs and no tangent frames
  std::vector<izd::GLight> lights;
  std::vector<Double4> mat_const;        // >= 1, per material: its constant RGB albedo / emit value (GShade cflags bit0)
  std::vector<izd::MatTex> mat_tex;      // >= 1, per material: its RGB texture slots
  std::vector<izpi_texture> textures;    // the caller's, with pad0, value[0..1] and texel_offset in their device form
  std::vector<double> texels;            // >= 1, every image texture's own run (TexSlot)
  // DevScene's scalars
  int32_t root = -1;
  uint32_t num_inner = 0, leaf_shortcut = 1, quantized = 0, nan_free_bounds = 1, ordered_bounds = 1, time_free = 1, no_pathlen = 1, tri_only = 1;
  uint32_t stack_needed = 0;             // stack_bound of the tree
  uint32_t leaf_max = 0;                 // the largest primitive count of a leaf (0: no leaf)
  // what the materials allow and need: the kernel instances a render picks
  bool mat_ok_rgb = true, mat_ok_spectral = true;  // every material has the textures the Colour / Spectral sampler reads
  bool basic_materials = true;           // only Lambertian + DiffuseLight
  uint32_t matset = 0;                   // MS_* bits of the material kinds
  bool const_albedo = true;              // every Lambertian / DiffuseLight albedo is a constant RGB
  bool any_uv = false;                   // a material reads the hit's (u, v) (image textures)
};

// Validate and pack *d. IZPI_OK, or the status with its text in *err; *out is then unspecified.
int pack_scene(const izpi_scene_desc* d, PackedScene* out, std::string* err);

// The node block of an uploaded scene: the inner nodes at its start, then their quantised form
// (if any), then the leaf records, in one device allocation (byte offsets; counts of records).
// alloc_bytes: the allocation, TRACE_TAIL_PAD past the records: a leaf lane of k_trace2 loads 16 B at each
// of its box's six floats (GLeaf::mn, mx), so the load at the last record's mx[2] ends 4 B past it.
constexpr uint64_t TRACE_TAIL_PAD = 16;
struct TraceLayout { uint64_t innerq_at, leaves_at, bytes, alloc_bytes; };
inline TraceLayout trace_layout(uint64_t n_inner, uint64_t n_innerq, uint64_t n_leaves) {
  TraceLayout t;
  t.innerq_at = n_inner * sizeof(izd::GInner);
  t.leaves_at = t.innerq_at + n_innerq * sizeof(izd::GInnerQ);
  t.bytes = t.leaves_at + n_leaves * sizeof(izd::GLeaf);
  t.alloc_bytes = t.bytes + TRACE_TAIL_PAD;
  return t;
}
// DevScene::addr32: every record of the node block starts below 4 GiB from the block's base, and
// every primitive record below 4 GiB from the first, so k_trace2 may address them with unsigned
// 32-bit byte offsets (a load's immediate offset within a record is added 64 bits wide).
inline bool trace_addr32(uint64_t n_inner, uint64_t n_innerq, uint64_t n_leaves, uint64_t n_prims) {
  const uint64_t lim = 1ull << 32;
  return trace_layout(n_inner, n_innerq, n_leaves).bytes <= lim && n_prims * sizeof(izd::GPrim) <= lim;
}

// Upper bound on the traversal stack (bvh4.go:71-73): along any root-to-leaf path a node
// pushes at most (valid children - 1) entries that stay below its subtree. One backward
// pass, so children must follow their parents (pre-order does): false when a child's index
// is not larger than its parent's. Child indices are below n.
bool stack_bound(const izpi_bvh4_node* nodes, size_t n, uint32_t* bound);

}  // namespace izpi_internal
