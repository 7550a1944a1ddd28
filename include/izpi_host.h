/* izpi_host.h — host-side scene producer (C++), standing in for the Go host's
 * transport.ToScene (transport/transport.go:53-92, 551-680) + camera.New
 * (camera/camera.go:28-58) + hitable.NewBVH4 (hitable/bvh4.go:517-855).
 *
 * Input is the protobuf-level scene (transport.proto): vertices, UVs, materials,
 * textures, spheres, camera. Output is the flattened izpi_scene_desc consumed by
 * izpi_gpu_upload_scene. In the production Go integration this step stays in Go
 * (the Go side already owns BVH4.Nodes); here it lets the C++/Python harness
 * build the same arrays without a Go toolchain.
 */
#ifndef IZPI_HOST_H
#define IZPI_HOST_H
#include <stdint.h>
#include "izpi_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* transport.proto Triangle: vertices/uv are proto floats widened to float64. */
typedef struct izpi_tri_in {
  double v0[3], v1[3], v2[3];
  double uv[6];          /* u0,v0,u1,v1,u2,v2 */
  uint32_t material;
  uint32_t pad;
} izpi_tri_in;

/* transport.proto Sphere: NewSphere(c, c, 0, 1, r, mat) (transport.go:679) */
typedef struct izpi_sphere_in {
  double center[3];
  double radius;
  uint32_t material;
  uint32_t pad;
} izpi_sphere_in;

/* transport.proto Camera */
typedef struct izpi_camera_in {
  double look_from[3], look_at[3], vup[3];
  double vfov, aspect, aperture, focus_dist, time0, time1, exposure;
} izpi_camera_in;

typedef struct izpi_scene_input {
  uint32_t num_tris, num_spheres, num_materials, num_textures;
  uint32_t num_spd;
  uint32_t pad0;
  uint64_t num_texels;
  const izpi_tri_in* tris;       /* embedded + streamed triangles, transport order */
  const izpi_sphere_in* spheres;
  const izpi_material* materials;
  const izpi_texture* textures;
  const double* texels;
  const double* spd_wavelengths;
  const double* spd_values;
  izpi_camera_in camera;
  double aspect_override;        /* leader: W/H (transport.go aspectOverride), 0 = camera.aspect */
  uint64_t bvh_seed;             /* seed of the BVH split-axis LCG (bvh4.go:520) */
} izpi_scene_input;

typedef struct izpi_host_scene izpi_host_scene;

/* Build; on failure returns non-zero and *out = NULL. */
int izpi_host_build_scene(const izpi_scene_input* in, izpi_host_scene** out);
/* flags: IZPI_HOST_SKIP_BVH leaves the BVH out (num_nodes = 0, primitives in transport
 * order) for another builder, e.g. izpi_gpu_build_bvh4, to attach with
 * izpi_host_scene_set_bvh. */
#define IZPI_HOST_SKIP_BVH 1u
int izpi_host_build_scene_ex(const izpi_scene_input* in, uint32_t flags, izpi_host_scene** out);
/* The f64 primitive boxes the BVH is built over ([num_tris + num_spheres][6]: min xyz,
 * max xyz; triangles first, transport order): Triangle.BoundingBox with its relative
 * epsilon (triangle.go:100-113), Sphere.BoundingBox (sphere.go). */
int izpi_host_scene_prim_boxes(const izpi_host_scene* s, double* boxes);
/* Attach a BVH4 built elsewhere: nodes in BVH4Node format with children after their
 * parents, order[k] = primitive (triangles then spheres) at leaf position k. */
int izpi_host_scene_set_bvh(izpi_host_scene* s, const izpi_bvh4_node* nodes, uint32_t num_nodes, const uint32_t* order);
/* Set the descriptor's IZPI_SCENE_* flags (izpi_scene_desc.flags), e.g. IZPI_SCENE_QUANTIZED_BVH
 * for a GPU-built tree. */
int izpi_host_scene_set_flags(izpi_host_scene* s, uint32_t flags);
const izpi_scene_desc* izpi_host_scene_desc(const izpi_host_scene* s);
/* Max stack depth the traversal of this BVH can reach (host-computed bound). */
uint32_t izpi_host_scene_stack_bound(const izpi_host_scene* s);
double izpi_host_scene_build_ms(const izpi_host_scene* s);
void izpi_host_scene_free(izpi_host_scene* s);
const char* izpi_host_last_error(void);

/* Tile grid of common.Tiles (common/tiles.go:6-24) + grid.WalkGrid spiral order
 * (grid/grid.go:27-130): writes up to max_tiles entries of x0,y0,x1,y1; returns count. */
uint32_t izpi_host_tiles(uint32_t width, uint32_t height, uint32_t* tiles, uint32_t max_tiles);

/* How izpi_gpu_multi_render / izpi_gpu_render_rank split a frame over num_shares devices,
 * step by step (the device path is exactly these five):
 *   1. izpi_host_share_units: the frame's tiles -> the units that are dealt;
 *   2. izpi_host_share_tiles: the units of share r (unit % num_shares == r);
 *   3. izpi_host_share_block: the padded size of every share's packed block;
 *   4. each share is rendered packed (IZPI_OUT_PACKED) into its block;
 *   5. izpi_host_assemble_shares (on the device: k_unpack) scatters the gathered blocks
 *      into the canvas.
 * Steps 2, 3 and 5 take the unit list of step 1 as their `tiles`. */

/* The units a frame's tiles are dealt in when it is split into num_shares shares: with
 * num_shares > 1 and tiles that are equal-sized, even in both extents and at least
 * 16 x 16, every tile becomes its four quarters (in the tile's order, then rows j, then
 * columns i); otherwise the list is copied unchanged. `out` holds [4 * num_tiles][4];
 * returns the number of units. */
uint32_t izpi_host_share_units(const uint32_t* tiles, uint32_t num_tiles, uint32_t num_shares, uint32_t* out);

/* One share of a list of units (izpi_host_share_units; any tile list deals the same way):
 * copies units t with t % num_shares == share, in order, into `out`; returns how many.
 * The largest share has ceil(num_tiles / num_shares) of them. */
uint32_t izpi_host_share_tiles(const uint32_t* tiles, uint32_t num_tiles, uint32_t share, uint32_t num_shares,
                               uint32_t* out);

/* Primitives per leaf for izpi_gpu_build_bvh4 on this scene: 3, or 2 when spheres are at
 * least a quarter of the primitives (a sphere test costs more than a node visit; C5 at
 * 32 spp: -2.9% per frame with 2). The Python host, the C replay and the Go shim all use it. */
uint32_t izpi_host_bvh_leaf_max(const izpi_scene_desc* desc);

/* Doubles per padded share block of a packed multi-GPU gather, over the units
 * (izpi_host_share_units: num_tiles of them, tile_w x tile_h each): ceil(num_tiles /
 * num_shares) * tile_w * tile_h * 4 (every share's block has this size). */
uint64_t izpi_host_share_block(uint32_t num_tiles, uint32_t tile_w, uint32_t tile_h, uint32_t num_shares);

/* What the root of izpi_gpu_multi_render / izpi_gpu_render_rank does after the gather,
 * on the host, with `tiles` the units those deal (izpi_host_share_units): block r of
 * `gathered` (izpi_host_share_block doubles each) holds share r's units
 * (izpi_host_share_tiles) packed (IZPI_OUT_PACKED); every pixel is scattered to canvas
 * row height - y (render/rgb.go:41; sample row y = 0 has no canvas row). The same index
 * rule as the device's k_unpack. Replaces the framebuffer assembly of renderer.go:172-211
 * (workers write their tiles into the shared canvas). Units must be equal-sized and in
 * bounds. */
int izpi_host_assemble_shares(uint32_t width, uint32_t height, const uint32_t* tiles, uint32_t num_tiles,
                              uint32_t num_shares, const double* gathered, double* canvas);

/* The Go-math routines of izpi_amd/csrc/gomath.h evaluated on the host (same op
 * codes as izpi_gpu_gomath); used by the parity tests. */
double izpi_host_gomath(int op, double x, double y);

/* ======================================================================
 * The DISPLACE geometry operator: displacement.ApplyDisplacementMap
 * (displacement/displacement.go:143-280) over `n` triangles and a float64 NRGBA map
 * (row 0 = top; its blue channel is the height, read as ImageTxt.Value reads it,
 * texture/image.go:73-101). Every triangle is tessellated at least once, adaptively and
 * level by level, and each finished triangle is displaced along its own normal by
 * dmin + (dmax - dmin) * z. The result is izpi_tri_in again: the displaced vertices, the
 * child's UVs and the source's material.
 *
 * order: IZPI_DISPLACE_PER_TRIANGLE = one ApplyDisplacementMap per source triangle, as the
 * scene path calls it (transport.go:641): outputs are source-major; IZPI_DISPLACE_MESH =
 * one call over the whole mesh (wavefront.go:347): outputs are level-major across the
 * mesh. In both, a level's outputs follow the parents' order times child 0..3.
 *
 * One deviation: where the reference would subdivide without end (a map that steps by more
 * than 2/|dmax-dmin| between two neighbouring texels), a source triangle that still has
 * work after IZPI_DISPLACE_MAX_LEVELS levels fails the whole call with
 * IZPI_ERR_UNSUPPORTED.
 *
 * out == NULL counts only. *n_out receives the number of output triangles; when out holds
 * fewer (cap), the call returns IZPI_ERR_INVALID with *n_out set. counts (may be NULL)
 * receives the outputs per source triangle, [n]. *ms (may be NULL): the device time
 * between upload and copy back (izpi_gpu_displace), the wall time (izpi_host_displace).
 * The device entry keeps its buffers for the call only and refuses, without trying, a
 * request whose work lists could exceed half of the free device memory. The host entry is
 * the sequential twin, bit for bit; its error is izpi_host_last_error's.
 * ====================================================================== */
#define IZPI_DISPLACE_PER_TRIANGLE 0u
#define IZPI_DISPLACE_MESH 1u
#define IZPI_DISPLACE_MAX_LEVELS 16
int izpi_gpu_displace(izpi_ctx* ctx, const izpi_tri_in* tris, uint64_t n, const double* rgba, uint32_t width,
                      uint32_t height, double dmin, double dmax, uint32_t order, izpi_tri_in* out, uint64_t cap,
                      uint64_t* n_out, uint64_t* counts, double* ms);
int izpi_host_displace(const izpi_tri_in* tris, uint64_t n, const double* rgba, uint32_t width, uint32_t height,
                       double dmin, double dmax, uint32_t order, izpi_tri_in* out, uint64_t cap, uint64_t* n_out,
                       uint64_t* counts, double* ms);

/* The host twin of izpi_gpu_denoise (izpi_gpu.h: the rule and the arguments are the same):
 * the sequential restatement from the same arithmetic (izpi_amd/csrc/denoise.h), bit for
 * bit what the device writes, IZPI_DENOISE_DEMODULATE included (the demodulated canvas is
 * a temporary). All pointers host; its error is izpi_host_last_error's. */
int izpi_host_denoise(const double* colour, const double* normal, const double* albedo, double* out, uint32_t width,
                      uint32_t height, const izpi_denoise_params* p);

/* The host twin of izpi_gpu_denoise_var (izpi_gpu.h: the rule and the arguments are the same;
 * the arithmetic is izpi_amd/csrc/denoise.h's), bit for bit what the device writes.
 * stderr_host: the [H][W][4] canvas of standard errors (IZPI_SNAP_NOISE's form); var_out
 * ([H][W], may be NULL): the variance of the filtered canvas (with IZPI_DENOISE_DEMODULATE:
 * of the filtered demodulated canvas, the space the filter ran in). All pointers host; its
 * error is izpi_host_last_error's. */
int izpi_host_denoise_var(const double* colour, const double* stderr_host, const double* normal, const double* albedo,
                          double* out, double* var_out, uint32_t width, uint32_t height, const izpi_denoise_params* p,
                          double variance_floor);

/* The host twin of izpi_gpu_progressive_noise and of the IZPI_SNAP_NOISE snapshot (izpi_gpu.h:
 * the rule is stated there; the arithmetic is izpi_amd/csrc/noise.h's, bit for bit what the
 * device gives): sums and moment2 are [num_pixels][3], the per-pixel sums and second moments
 * after `done` >= 2 samples, in packed order; counted[p] != 0 marks the pixels the statistic
 * counts (NULL: all); sampler (IZPI_SAMPLER_*) picks the mean's rule; p == NULL: the
 * defaults. se_out ([num_pixels][4], may be NULL) receives (se_0, se_1, se_2, 1.0) of every
 * pixel, counted or not; out (may be NULL) the statistic, device_ms 0. Its error is
 * izpi_host_last_error's. */
int izpi_host_noise(const double* sums, const double* moment2, const uint8_t* counted, uint32_t num_pixels, uint32_t done,
                    uint32_t sampler, const izpi_noise_params* p, double* se_out, izpi_noise_stats* out);

/* The host twin of izpi_gpu_progressive_adapt (izpi_gpu.h states the rule; noise.h's arithmetic):
 * one evaluation over a session's pixels in packed order. sums, moment2: [num_pixels][3];
 * counted[p] != 0 marks the counted pixels (NULL: all); samples[p]: n_p (read only: an active
 * pixel has n_p == done, a retired one what it retired with); active[p] != 0 on entry marks the
 * active pixels, and on return those that stay active; done >= 2. An active pixel is evaluated
 * at n = done, a retired one (for nonfinite) at its n_p >= 2. e_out ([num_pixels], may be NULL)
 * receives that e. stats (may be NULL): as izpi_gpu_progressive_adapt fills them, device_ms 0.
 * Its error is izpi_host_last_error's. */
int izpi_host_adapt(const double* sums, const double* moment2, const uint8_t* counted, const uint32_t* samples,
                    uint8_t* active, uint32_t num_pixels, uint32_t done, uint32_t sampler, const izpi_noise_params* p,
                    double* e_out, izpi_adapt_stats* stats);

/* ======================================================================
 * The checkpoint of a progressive session on the host (izpi_gpu.h states the format and the
 * rule). None of these needs a GPU; their error is
 * izpi_host_last_error's.
 *
 *  _field   one scalar of a blob's header (IZPI_CKPT_*; the doubles as their bits, counter k
 *           as IZPI_CKPT_COUNTER + k, the planes' offsets from the blob's start, 0 for a plane
 *           the session lacks). Checks the header only: a truncated blob still tells its size.
 *  _check   the validation izpi_gpu_progressive_resume runs before it touches the device: the
 *           blob is whole (size, magic, version, checksum), holds a sample, every deciding
 *           field of `req` and the scene tag equal its own, and req->spp >= done.
 *  _pack    k_ckpt_gather's twin: a session's state in the packed order of `tiles` (sums and
 *           moment2 [num_pixels][3], samples and state [num_pixels]; moment2 is read with
 *           IZPI_PROG_NOISE; samples and state come together and may be NULL: every pixel
 *           active with `done` samples) into the frame-order planes, the blob's bytes after
 *           its header. A pixel of no tile: state 255, zeros. *bytes (may be NULL) receives
 *           their size; planes == NULL asks for that alone.
 *  _unpack  k_ckpt_scatter's twin: the planes into the packed order of `tiles` (the outputs a
 *           session with `flags` has are required). *absent: the pixels of `tiles` without a
 *           record, which are left untouched; *unclaimed: the records no pixel took.
 *  izpi_host_scene_tag  a 64-bit digest (the blob's word-wise FNV-1a) over every array of the
 *           descriptor, its counts and flags, and the camera: what a caller passes as the
 *           checkpoint's scene tag. The library hashes nothing at upload.
 * ====================================================================== */
enum {
  IZPI_CKPT_VERSION = 0, IZPI_CKPT_HEADER_BYTES, IZPI_CKPT_BLOB_BYTES, IZPI_CKPT_CHECKSUM, IZPI_CKPT_FLAGS,
  IZPI_CKPT_LISTED, IZPI_CKPT_WIDTH, IZPI_CKPT_HEIGHT, IZPI_CKPT_SAMPLER, IZPI_CKPT_ACCUMULATION, IZPI_CKPT_MAX_DEPTH,
  IZPI_CKPT_NUM_BG_SPD, IZPI_CKPT_SEED, IZPI_CKPT_BG_DIGEST, IZPI_CKPT_PIXELS, IZPI_CKPT_SCENE_TAG, IZPI_CKPT_DONE,
  IZPI_CKPT_SPP, IZPI_CKPT_SAMPLES, IZPI_CKPT_ACTIVE, IZPI_CKPT_NUM_COUNTERS, IZPI_CKPT_STATE_OFFSET,
  IZPI_CKPT_SUMS_OFFSET, IZPI_CKPT_MOMENTS_OFFSET, IZPI_CKPT_COUNTS_OFFSET,
  IZPI_CKPT_BACKGROUND = 32, /* + 0..2 */
  IZPI_CKPT_INK = 36,        /* + 0..2 */
  IZPI_CKPT_COUNTER = 64     /* + k, k < IZPI_CKPT_NUM_COUNTERS */
};
int izpi_host_checkpoint_field(const void* blob, uint64_t bytes, uint32_t which, uint64_t* out);
int izpi_host_checkpoint_check(const void* blob, uint64_t bytes, const izpi_render_req* req, uint64_t scene_tag);
int izpi_host_checkpoint_pack(uint32_t width, uint32_t height, const uint32_t* tiles, uint32_t num_tiles, uint32_t flags,
                              uint32_t done, const double* sums, const double* moment2, const uint32_t* samples,
                              const uint8_t* state, void* planes, uint64_t cap, uint64_t* bytes);
int izpi_host_checkpoint_unpack(uint32_t width, uint32_t height, const uint32_t* tiles, uint32_t num_tiles, uint32_t flags,
                                const void* planes, uint64_t bytes, double* sums, double* moment2, uint32_t* samples,
                                uint8_t* state, uint64_t* absent, uint64_t* unclaimed);
int izpi_host_scene_tag(const izpi_scene_desc* desc, uint64_t* out);

/* sizeof() of the boundary structs: 0 izpi_bvh4_node 1 izpi_texture 2 izpi_material
 * 3 izpi_camera 4 izpi_scene_desc 5 izpi_render_req 6 izpi_render_stats 7 izpi_hit
 * 8 izpi_tri_in 9 izpi_sphere_in 10 izpi_camera_in 11 izpi_scene_input 12 izpi_proto_info
 * 13 izpi_obj_info 14 izpi_obj_group 15 izpi_obj_material 16 izpi_render_tuning
 * 17 izpi_denoise_params 18 izpi_noise_params 19 izpi_noise_stats 20 izpi_adapt_stats
 * (0 = unknown). */
uint32_t izpi_abi_struct_size(int which);

/* ======================================================================
 * Scene ingestion — for hosts without Go.
 * In the Go integration these steps stay in Go (prototext/proto + transport).
 * ====================================================================== */

/* transport.Scene, parsed from the text (.pbtxt, prototext.Unmarshal, leader.go:64-71)
 * or binary (.izpi, proto.Unmarshal, leader.go:56-63) encoding of transport.proto.
 * Text format follows prototext: unknown fields, a repeated singular field and two
 * members of one oneof are errors. Binary: unknown fields are skipped. */
typedef struct izpi_proto_scene izpi_proto_scene;

enum { IZPI_COLOUR_RGB = 1, IZPI_COLOUR_SPECTRAL = 2 }; /* transport.proto ColourRepresentation */

typedef struct izpi_proto_info {
  uint32_t colour_representation; /* IZPI_COLOUR_*, 0 = unspecified */
  uint32_t stream_triangles;
  uint64_t total_triangles;
  uint32_t num_triangles;          /* Scene.objects.triangles (embedded) */
  uint32_t num_streamed_triangles; /* added with izpi_scene_add_triangles */
  uint32_t num_spheres, num_materials, num_image_textures, num_displacement_maps;
  uint32_t num_background;         /* spectral_background entries */
  uint32_t pad;
  const char* name;
  const char* version;
  const char* warnings;            /* e.g. unknown light source -> CIE A (transport.go:474-478) */
} izpi_proto_info;

int izpi_scene_parse_text(const char* text, uint64_t len, izpi_proto_scene** out);
int izpi_scene_parse_binary(const void* buf, uint64_t len, izpi_proto_scene** out);
/* The parsed scene as transport.Scene wire bytes, as proto.Marshal writes them (fields in
 * number order, repeated scalars packed, proto3 zero scalars omitted): the .izpi form of
 * a .pbtxt. Writes min(cap, size) bytes to buf (may be NULL with cap 0) and the size to
 * *len. Streamed triangles (izpi_scene_add_triangles) are not part of the message. */
int izpi_scene_serialize(const izpi_proto_scene* s, void* buf, uint64_t cap, uint64_t* len);
int izpi_scene_info(const izpi_proto_scene* s, izpi_proto_info* out);
/* Filenames of Scene.image_textures, which the host decodes (leader.go:84-98)... */
const char* izpi_scene_image_file(const izpi_proto_scene* s, uint32_t i);
/* ...and hands over as float64 NRGBA texels, row 0 = top (texture.ImageTxt). */
int izpi_scene_set_image(izpi_proto_scene* s, const char* filename, uint32_t width, uint32_t height, const double* rgba);
/* Filenames of Scene.displacement_maps, which the host decodes (leader.go:100-109)... */
const char* izpi_scene_displacement_file(const izpi_proto_scene* s, uint32_t i);
/* ...and hands over as float64 NRGBA texels, row 0 = top; maps are keyed by filename.
 * Width and height are at least 1. */
int izpi_scene_set_displacement_map(izpi_proto_scene* s, const char* filename, uint32_t width, uint32_t height,
                                    const double* rgba);
/* Where izpi_scene_to_input runs triangles with `operator: DISPLACE`: on ctx's device
 * (izpi_gpu_displace), or with NULL, the default, on the host (izpi_host_displace). Both
 * give the same triangles. The context must outlive the conversions that use it. */
int izpi_scene_set_displacer(izpi_proto_scene* s, izpi_ctx* ctx);
/* Streamed triangles (transport.go:574-583, e.g. from izpi_obj_group_to_triangles);
 * `material` of each izpi_tri_in is ignored, the name is resolved at conversion. */
int izpi_scene_add_triangles(izpi_proto_scene* s, const izpi_tri_in* tris, uint64_t n, const char* material_name);
/* Scene.spectral_background; returns its length, copies up to max entries. */
uint32_t izpi_scene_background(const izpi_proto_scene* s, double* wavelengths, double* values, uint32_t max);
/* transport.ToScene (transport.go:53-92) up to the BVH build: materials (registered by
 * Material.name), textures, light-source library, camera, embedded then streamed
 * triangles, spheres. An embedded triangle with `operator: DISPLACE` is replaced, in its
 * place, by what displacement.ApplyDisplacementMap returns for it (transport.go:634-646);
 * its map must be declared in Scene.displacement_maps and handed over, else
 * IZPI_ERR_INVALID "displacement map <name> not found". *out stays valid until the next
 * call or izpi_scene_free; pass it to izpi_host_build_scene. */
int izpi_scene_to_input(izpi_proto_scene* s, double aspect_override, uint64_t bvh_seed, const izpi_scene_input** out);
/* name of material i of the last izpi_scene_to_input */
const char* izpi_scene_material_name(const izpi_proto_scene* s, uint32_t i);
void izpi_scene_free(izpi_proto_scene* s);

/* lightsources.GetLightSource (lightsources.go:472-475): copies the 75 values at the CIE
 * wavelengths (blackbody entries computed as spectral.NewBlackbodySPD); returns 75, or
 * 0 if the name is unknown. izpi_light_source_name(i) enumerates the library. */
uint32_t izpi_light_source(const char* name, double* values);
const char* izpi_light_source_name(uint32_t i);

/* Wavefront OBJ (wavefront.go:107-625). */
typedef struct izpi_obj izpi_obj;
#define IZPI_OBJ_IGNORE_NORMALS 1u   /* ParseOption IGNORE_NORMALS */
#define IZPI_OBJ_IGNORE_MATERIALS 2u /* IGNORE_MATERIALS: mtllib lines are skipped */
#define IZPI_OBJ_IGNORE_TEXTURES 4u  /* IGNORE_TEXTURES */
#define IZPI_OBJ_FACE_POLYGON 1u     /* ObjFaceType OBJ_FACE_TYPE_POLYGON */

typedef struct izpi_obj_info {
  uint32_t has_normals, has_uv, ignore_materials, ignore_normals, ignore_textures;
  uint32_t num_groups, num_materials, pad;
  uint64_t num_vertices, num_normals, num_uvs;
  double centre[3];
  const char* object_name;
} izpi_obj_info;

typedef struct izpi_obj_group {
  const char* name;
  const char* material;
  uint32_t face_type;
  uint32_t is_null;                /* the trailing nil group of a file without faces */
  uint64_t num_faces;
  uint64_t num_face_vertices;
} izpi_obj_group;

typedef struct izpi_obj_material { /* wavefront.Material; Kd/Ka/Ks up to 3 values */
  const char* name;
  double kd[3], ka[3], ks[3];
  uint32_t num_kd, num_ka, num_ks, pad;
  double ns, ni, d;
  int64_t sharpness, illum;
} izpi_obj_material;

/* NewObjFromReader: mtllib files are read from container_dir (wavefront.go:193-204). */
int izpi_obj_parse(const char* text, uint64_t len, const char* container_dir, uint32_t options, izpi_obj** out);
int izpi_obj_info_get(const izpi_obj* o, izpi_obj_info* out);
int izpi_obj_copy_vertices(const izpi_obj* o, double* v, double* vn, double* vt);
int izpi_obj_group_get(const izpi_obj* o, uint32_t g, izpi_obj_group* out);
/* per face its vertex count; per face vertex (VIdx, VtIdx, VnIdx) as in the file (1-based) */
int izpi_obj_copy_faces(const izpi_obj* o, uint32_t g, uint32_t* face_sizes, int64_t* indices);
/* materials in name order */
int izpi_obj_material_get(const izpi_obj* o, uint32_t i, izpi_obj_material* out);
void izpi_obj_translate(izpi_obj* o, double x, double y, double z);
void izpi_obj_scale(izpi_obj* o, double x, double y, double z);
void izpi_obj_rotate(izpi_obj* o, double alpha, double beta, double gamma);
/* GroupToTransportTrianglesWithMaterial (wavefront.go:240-312); out = NULL: count only */
int izpi_obj_group_to_triangles(const izpi_obj* o, uint32_t g, uint32_t without_uvs, izpi_tri_in* out, uint64_t max,
                                uint64_t* n);
void izpi_obj_free(izpi_obj* o);

#ifdef __cplusplus
}
#endif
#endif
