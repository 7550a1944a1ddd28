// checkpoint_host.cpp — the host side of a session's checkpoint: reading
// and validating a blob, the host twins of the two reorder kernels (checkpoint.hip) from the same
// per-pixel rule (checkpoint.h), and the scene tag. No HIP here: a host compiler builds it alone.
#include <stdio.h>

#include <string>
#include <vector>

#include "checkpoint.h"
#include "izpi_req.h"

namespace izpi_internal {
void set_host_error(const std::string& s);

static uint64_t hash_doubles(uint64_t h, const double* v, uint64_t n) { return v && n ? ck::hash_words(h, v, n * 8) : h; }

ck::Header checkpoint_header(const izpi_render_req& req, uint32_t flags, uint64_t scene_tag) {
  ck::Header h;
  memset(&h, 0, sizeof h);
  h.magic = ck::MAGIC; h.version = ck::VERSION; h.header_bytes = sizeof h;
  h.blob_bytes = ck::Layout(req.width, req.height, flags).bytes;
  h.flags = flags;
  h.width = req.width; h.height = req.height; h.sampler = req.sampler; h.accumulation = req.accumulation;
  h.max_depth = req.max_depth; h.num_bg_spd = req.num_bg_spd; h.seed = req.seed;
  for (int k = 0; k < 3; k++) { h.background[k] = req.background[k]; h.ink[k] = req.ink[k]; }
  h.bg_digest = hash_doubles(hash_doubles(ck::HASH_BASIS, req.bg_spd_wavelengths, req.num_bg_spd), req.bg_spd_values, req.num_bg_spd);
  h.scene_tag = scene_tag;
  h.spp = req.spp;
  return h;
}

uint64_t checkpoint_checksum(const void* blob, uint64_t bytes) {
  return ck::hash_words(ck::HASH_BASIS, (const char*)blob + ck::CHECKSUM_FROM, bytes - ck::CHECKSUM_FROM);
}

// The header alone: present in full, of this format, and of the size its planes take.
static const char* header_check(const void* blob, uint64_t bytes, ck::Header* h) {
  if (!blob) return "checkpoint: null blob";
  if (bytes < sizeof(ck::Header)) return "checkpoint: truncated within the header";
  memcpy(h, blob, sizeof *h);
  if (h->magic != ck::MAGIC) return "checkpoint: bad magic";
  if (h->version != ck::VERSION) return "checkpoint: unknown format version";
  if (h->header_bytes != sizeof(ck::Header)) return "checkpoint: unknown header size";
  if (h->flags & ~(uint32_t)(IZPI_PROG_NOISE | IZPI_PROG_ADAPTIVE) || ((h->flags & IZPI_PROG_ADAPTIVE) && !(h->flags & IZPI_PROG_NOISE)))
    return "checkpoint: unknown session flags";
  if (h->width == 0 || h->height == 0 || (uint64_t)h->width * h->height > (1ull << 30)) return "checkpoint: bad frame size";
  if (h->blob_bytes != ck::Layout(h->width, h->height, h->flags).bytes) return "checkpoint: its size does not match its planes";
  if (h->cnt_n > ck::MAX_COUNTERS) return "checkpoint: too many counters";
  return nullptr;
}

const char* checkpoint_check(const void* blob, uint64_t bytes, const izpi_render_req* req, uint64_t scene_tag, char* msg,
                             size_t cap) {
  ck::Header h;
  if (const char* bad = header_check(blob, bytes, &h)) return bad;
  if (bytes < h.blob_bytes) {
    snprintf(msg, cap, "checkpoint: truncated: %llu of %llu bytes", (unsigned long long)bytes, (unsigned long long)h.blob_bytes);
    return msg;
  }
  if (bytes != h.blob_bytes) return "checkpoint: bytes past the blob's end";
  if (checkpoint_checksum(blob, bytes) != h.checksum) return "checkpoint: checksum mismatch";
  if (h.done == 0) return "checkpoint: no sample in it (done == 0)";
  if (!req) return "checkpoint: null request";
  const izpi_render_req q = request_copy(req);
  if (q.num_bg_spd && (!q.bg_spd_wavelengths || !q.bg_spd_values)) return "num_bg_spd without the SPD arrays";
  const ck::Header want = checkpoint_header(q, h.flags, scene_tag);
  const char* field = nullptr;
  if (h.width != want.width) field = "width";
  else if (h.height != want.height) field = "height";
  else if (h.sampler != want.sampler) field = "sampler";
  else if (h.accumulation != want.accumulation) field = "accumulation";
  else if (h.max_depth != want.max_depth) field = "max_depth";
  else if (h.seed != want.seed) field = "seed";
  else if (memcmp(h.background, want.background, sizeof h.background)) field = "background";
  else if (memcmp(h.ink, want.ink, sizeof h.ink)) field = "ink";
  else if (h.num_bg_spd != want.num_bg_spd || h.bg_digest != want.bg_digest) field = "bg_spd";
  if (field) {
    snprintf(msg, cap, "checkpoint: the request's %s differs from the checkpoint's", field);
    return msg;
  }
  if (h.scene_tag != scene_tag) return "checkpoint: the scene tag differs (another scene)";
  if (q.spp < h.done) {
    snprintf(msg, cap, "checkpoint: spp %u is below the %u samples done", q.spp, h.done);
    return msg;
  }
  return nullptr;
}

// The tiles of a pack / unpack call: non-empty, in bounds, equal-sized (validate_tiles' rule).
static bool tiles_ok(uint32_t width, uint32_t height, const uint32_t* tiles, uint32_t n, uint32_t* tw, uint32_t* th) {
  if (!tiles || n == 0 || width == 0 || height == 0) return false;
  *tw = tiles[2] - tiles[0] + 1;
  *th = tiles[3] - tiles[1] + 1;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t* t = tiles + 4 * (size_t)i;
    if (t[2] < t[0] || t[3] < t[1] || t[2] >= width || t[3] >= height) return false;
    if (t[2] - t[0] + 1 != *tw || t[3] - t[1] + 1 != *th) return false;
  }
  return (uint64_t)n * *tw * *th <= (1ull << 30);
}
}  // namespace izpi_internal

using namespace izpi_internal;

static int refuse(const std::string& why) {
  set_host_error(why);
  return IZPI_ERR_INVALID;
}

extern "C" {

int izpi_host_checkpoint_field(const void* blob, uint64_t bytes, uint32_t which, uint64_t* out) {
  ck::Header h;
  if (const char* bad = header_check(blob, bytes, &h)) return refuse(bad);
  if (!out) return refuse("checkpoint_field: null output");
  auto bits = [](double d) { uint64_t u; memcpy(&u, &d, 8); return u; };
  const ck::Layout l(h.width, h.height, h.flags);
  switch (which) {
    case IZPI_CKPT_VERSION: *out = h.version; break;
    case IZPI_CKPT_HEADER_BYTES: *out = h.header_bytes; break;
    case IZPI_CKPT_BLOB_BYTES: *out = h.blob_bytes; break;
    case IZPI_CKPT_CHECKSUM: *out = h.checksum; break;
    case IZPI_CKPT_FLAGS: *out = h.flags; break;
    case IZPI_CKPT_LISTED: *out = h.listed; break;
    case IZPI_CKPT_WIDTH: *out = h.width; break;
    case IZPI_CKPT_HEIGHT: *out = h.height; break;
    case IZPI_CKPT_SAMPLER: *out = h.sampler; break;
    case IZPI_CKPT_ACCUMULATION: *out = h.accumulation; break;
    case IZPI_CKPT_MAX_DEPTH: *out = h.max_depth; break;
    case IZPI_CKPT_NUM_BG_SPD: *out = h.num_bg_spd; break;
    case IZPI_CKPT_SEED: *out = h.seed; break;
    case IZPI_CKPT_BG_DIGEST: *out = h.bg_digest; break;
    case IZPI_CKPT_PIXELS: *out = h.pixels; break;
    case IZPI_CKPT_SCENE_TAG: *out = h.scene_tag; break;
    case IZPI_CKPT_DONE: *out = h.done; break;
    case IZPI_CKPT_SPP: *out = h.spp; break;
    case IZPI_CKPT_SAMPLES: *out = h.samples; break;
    case IZPI_CKPT_ACTIVE: *out = h.active; break;
    case IZPI_CKPT_NUM_COUNTERS: *out = h.cnt_n; break;
    case IZPI_CKPT_STATE_OFFSET: *out = l.state; break;
    case IZPI_CKPT_SUMS_OFFSET: *out = l.sums; break;
    case IZPI_CKPT_MOMENTS_OFFSET: *out = l.moments; break;
    case IZPI_CKPT_COUNTS_OFFSET: *out = l.counts; break;
    default:
      if (which >= IZPI_CKPT_BACKGROUND && which < IZPI_CKPT_BACKGROUND + 3) *out = bits(h.background[which - IZPI_CKPT_BACKGROUND]);
      else if (which >= IZPI_CKPT_INK && which < IZPI_CKPT_INK + 3) *out = bits(h.ink[which - IZPI_CKPT_INK]);
      else if (which >= IZPI_CKPT_COUNTER && which < IZPI_CKPT_COUNTER + h.cnt_n) *out = h.counters[which - IZPI_CKPT_COUNTER];
      else return refuse("checkpoint_field: unknown field");
  }
  return IZPI_OK;
}

int izpi_host_checkpoint_check(const void* blob, uint64_t bytes, const izpi_render_req* req, uint64_t scene_tag) {
  char msg[160];
  const char* bad = checkpoint_check(blob, bytes, req, scene_tag, msg, sizeof msg);
  return bad ? refuse(bad) : IZPI_OK;
}

int izpi_host_checkpoint_pack(uint32_t width, uint32_t height, const uint32_t* tiles, uint32_t num_tiles, uint32_t flags,
                              uint32_t done, const double* sums, const double* moment2, const uint32_t* samples,
                              const uint8_t* state, void* planes, uint64_t cap, uint64_t* bytes) {
  uint32_t tw = 0, th = 0;
  if (!tiles_ok(width, height, tiles, num_tiles, &tw, &th)) return refuse("checkpoint_pack: tiles must be non-empty, in bounds and equal-sized");
  if (flags & ~(uint32_t)(IZPI_PROG_NOISE | IZPI_PROG_ADAPTIVE)) return refuse("checkpoint_pack: unknown flags");
  const ck::Layout l(width, height, flags);
  const uint64_t need = l.bytes - sizeof(ck::Header);
  if (bytes) *bytes = need;
  if (!planes) return IZPI_OK;  // (the size alone)
  if (cap < need) return refuse("checkpoint_pack: the output holds fewer bytes than the planes take");
  if (!sums || ((flags & IZPI_PROG_NOISE) && !moment2)) return refuse("checkpoint_pack: the sums (and with IZPI_PROG_NOISE the moments) must be given");
  if ((samples == nullptr) != (state == nullptr)) return refuse("checkpoint_pack: samples and state come together");
  // every record absent, then the session's pixels in packed order
  memset(planes, 0, need);
  const ck::Planes f = ck::planes_at(planes, sizeof(ck::Header), l);
  memset(f.state, ck::NOT_IN_SESSION, l.n);
  const PixelMap map{num_tiles * tw * th, width, height, tw, th, IZPI_OUT_PACKED, tiles};
  const ck::Packed s{const_cast<double*>(sums), const_cast<double*>(moment2), const_cast<uint32_t*>(samples),
                     const_cast<uint8_t*>(state), done};
  for (uint32_t p = 0; p < map.num_pixels; p++) ck::gather_pixel(map, p, s, f);
  return IZPI_OK;
}

int izpi_host_checkpoint_unpack(uint32_t width, uint32_t height, const uint32_t* tiles, uint32_t num_tiles, uint32_t flags,
                                const void* planes, uint64_t bytes, double* sums, double* moment2, uint32_t* samples,
                                uint8_t* state, uint64_t* absent, uint64_t* unclaimed) {
  uint32_t tw = 0, th = 0;
  if (!tiles_ok(width, height, tiles, num_tiles, &tw, &th)) return refuse("checkpoint_unpack: tiles must be non-empty, in bounds and equal-sized");
  if (flags & ~(uint32_t)(IZPI_PROG_NOISE | IZPI_PROG_ADAPTIVE)) return refuse("checkpoint_unpack: unknown flags");
  const ck::Layout l(width, height, flags);
  if (!planes || bytes != l.bytes - sizeof(ck::Header)) return refuse("checkpoint_unpack: the planes have another size");
  if (!sums || ((flags & IZPI_PROG_NOISE) && !moment2) || ((flags & IZPI_PROG_ADAPTIVE) && (!samples || !state)))
    return refuse("checkpoint_unpack: an output array is missing");
  std::vector<uint8_t> claimed(l.n, 0);
  const ck::Planes f = ck::planes_at(const_cast<void*>(planes), sizeof(ck::Header), l, claimed.data());
  const PixelMap map{num_tiles * tw * th, width, height, tw, th, IZPI_OUT_PACKED, tiles};
  const ck::Packed s{sums, moment2, samples, state, 0};
  uint64_t none = 0, left = 0;
  for (uint32_t p = 0; p < map.num_pixels; p++) none += ck::scatter_pixel(map, p, s, f) ? 0 : 1;
  for (uint64_t i = 0; i < l.n; i++) left += f.state[i] != ck::NOT_IN_SESSION && !claimed[i];
  if (absent) *absent = none;
  if (unclaimed) *unclaimed = left;
  return IZPI_OK;
}

int izpi_host_scene_tag(const izpi_scene_desc* d, uint64_t* out) {
  if (!d || !out) return refuse("scene_tag: null argument");
  uint64_t h = ck::HASH_BASIS;
  const uint64_t counts[] = {d->num_nodes, d->num_prims, d->num_tris, d->num_spheres, d->num_lights, d->num_materials,
                             d->num_textures, d->num_spd, d->flags, d->num_texels};
  h = ck::hash_words(h, counts, sizeof counts);
  auto add = [&h](const void* p, uint64_t bytes) {  // (each array with its length: no two layouts share a stream)
    h = ck::hash_u64(h, p ? bytes : 0);
    if (p && bytes) h = ck::hash_words(h, p, bytes);
  };
  const uint64_t nt = d->num_tris, ns = d->num_spheres;
  add(d->nodes, (uint64_t)d->num_nodes * sizeof(izpi_bvh4_node));
  add(d->prim_ref, (uint64_t)d->num_prims * 4);
  const double* tri3[] = {d->tri_v0, d->tri_v1, d->tri_v2, d->tri_e1, d->tri_e2, d->tri_normal, d->tri_tangent, d->tri_bitangent};
  for (const double* a : tri3) add(a, nt * 24);
  add(d->tri_uv, nt * 48); add(d->tri_area, nt * 8); add(d->tri_mat, nt * 4);
  add(d->sph_center0, ns * 24); add(d->sph_center1, ns * 24); add(d->sph_time, ns * 16); add(d->sph_radius, ns * 8);
  add(d->sph_mat, ns * 4);
  add(d->light_ref, (uint64_t)d->num_lights * 4);
  add(d->materials, (uint64_t)d->num_materials * sizeof(izpi_material));
  add(d->textures, (uint64_t)d->num_textures * sizeof(izpi_texture));
  add(d->texels, d->num_texels * 8);
  add(d->spd_wavelengths, (uint64_t)d->num_spd * 8); add(d->spd_values, (uint64_t)d->num_spd * 8);
  add(&d->camera, sizeof d->camera);
  *out = h;
  return IZPI_OK;
}

}  // extern "C"
