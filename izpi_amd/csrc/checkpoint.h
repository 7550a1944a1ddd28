// checkpoint.h — the checkpoint of a progressive session (deviation A28):
// the blob's header and plane layout, its checksum, and the per-pixel rule that moves a session's
// state between the packed order of its tiles and the frame order of the blob. The device kernels
// (checkpoint.hip) and the host twins (checkpoint_host.cpp) read the rule here, as noise.h is read
// by noise.hip and noise_host.cpp. Plain C++ when no HIP compiler is present.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#endif

#include "pixel_map.h"

namespace ck {

constexpr uint64_t MAGIC = 0x54504B4349505A49ull;  // "IZPICKPT" as the file's first eight bytes
constexpr uint32_t VERSION = 1;
constexpr uint32_t MAX_COUNTERS = 32;  // slots of Header::counters (the device has CNT_N of them, recorded in cnt_n)
// The counters a checkpoint carries: the six reference quantities (rays, node visits, triangle,
// sphere and the two light tests), which are a function of the samples rendered. The others are
// diagnostics of how the hardware happened to schedule the waves (wave-level step counts, the
// tail's share, parks): two runs of one session differ in them, so they are stored as 0 and count
// from the resume on, and the blob stays a function of the session's state alone.
constexpr uint32_t CARRIED_COUNTERS = 6;
// A pixel's state byte in the blob. The first three are AdaptParams::state's.
constexpr uint8_t ACTIVE = 0, RETIRED = 1, RETIRED_NONFINITE = 2, NOT_IN_SESSION = 255;

// The blob's first bytes, little-endian, every field at its natural alignment (no padding but
// `pad`, which is 0). `checksum` covers the bytes from `flags` to the blob's end.
struct Header {
  uint64_t magic;
  uint32_t version, header_bytes;
  uint64_t blob_bytes;
  uint64_t checksum;
  // ---- everything below is checksummed
  uint32_t flags, listed;  // IZPI_PROG_*; a pixel has retired
  uint32_t width, height, sampler, accumulation, max_depth, num_bg_spd;  // the request fields that decide a sample ...
  uint64_t seed;
  double background[3], ink[3];
  uint64_t bg_digest;  // ... and hash_words over the background SPD's wavelengths, then its values
  uint64_t pixels;     // present records: the session's distinct pixels
  uint64_t scene_tag;
  uint32_t done, spp;  // samples per active pixel; the cap at export (informational)
  uint64_t samples;    // the sum of n_p over the session's pixels (tile by tile)
  uint64_t active;     // an adaptive session's active pixels (else 0)
  uint32_t cnt_n, pad;
  uint64_t counters[MAX_COUNTERS];  // the device counters, [cnt_n] slots: the first CARRIED_COUNTERS hold values, the rest 0
};
static_assert(sizeof(Header) == 432, "the checkpoint header is 432 bytes");
constexpr uint64_t CHECKSUM_FROM = 32;  // offsetof(Header, flags)

// FNV-1a (offset basis 0xcbf29ce484222325, prime 0x100000001b3) taken over little-endian 64-bit
// words instead of bytes: h = (h ^ word) * prime. A tail of fewer than eight bytes is padded
// with zeros. The blob's planes are padded to eight bytes, so its checksum meets no tail.
constexpr uint64_t HASH_BASIS = 0xcbf29ce484222325ull, HASH_PRIME = 0x100000001b3ull;
inline uint64_t hash_words(uint64_t h, const void* data, uint64_t bytes) {
  const unsigned char* b = (const unsigned char*)data;
  uint64_t i = 0;
  for (; i + 8 <= bytes; i += 8) {
    uint64_t w;
    memcpy(&w, b + i, 8);
    h = (h ^ w) * HASH_PRIME;
  }
  if (i < bytes) {
    uint64_t w = 0;
    memcpy(&w, b + i, bytes - i);
    h = (h ^ w) * HASH_PRIME;
  }
  return h;
}
inline uint64_t hash_u64(uint64_t h, uint64_t w) { return (h ^ w) * HASH_PRIME; }

// Where the planes lie, as offsets from the blob's start: W * H entries each in sample-coordinate
// row-major order (y * W + x), the state bytes and the counts padded to eight bytes.
struct Layout {
  uint64_t n, state, sums, moments, counts, bytes;  // moments / counts: 0 when the session has none
  Layout(uint32_t width, uint32_t height, uint32_t flags) {
    auto up = [](uint64_t v) { return (v + 7) / 8 * 8; };
    n = (uint64_t)width * height;
    state = sizeof(Header);
    sums = state + up(n);
    uint64_t end = sums + n * 24;
    moments = counts = 0;
    if (flags & IZPI_PROG_NOISE) { moments = end; end += n * 24; }
    if (flags & IZPI_PROG_ADAPTIVE) { counts = end; end += up(n * 4); }
    bytes = end;
  }
};

// The planes in frame order. moments / counts are null when the session has none; claimed (a
// resume's marks, one byte per record, may be null) is not part of the blob.
struct Planes {
  uint8_t* state;
  double* sums;
  double* moments;
  uint32_t* counts;
  uint8_t* claimed;
};
// `base` is the blob's byte `from` (0: the blob itself; sizeof(Header): its planes alone).
inline Planes planes_at(void* base, uint64_t from, const Layout& l, uint8_t* claimed = nullptr) {
  char* b = (char*)base;
  return Planes{(uint8_t*)(b + (l.state - from)), (double*)(b + (l.sums - from)),
                l.moments ? (double*)(b + (l.moments - from)) : nullptr,
                l.counts ? (uint32_t*)(b + (l.counts - from)) : nullptr, claimed};
}

// A session's state in the packed order of its tiles. state / counts: an adaptive session's once
// a pixel has retired, else null: every pixel is active with `done` samples.
struct Packed {
  double* running;
  double* moments;
  uint32_t* counts;
  uint8_t* state;
  uint32_t done;
};

// Packed pixel p's record into the frame-order planes.
IZPI_PM void gather_pixel(const PixelMap& map, uint32_t p, const Packed& s, const Planes& f) {
  uint32_t x, y;
  map.xy(p, &x, &y);
  const size_t i = (size_t)y * map.width + x;
  f.state[i] = s.state ? s.state[p] : ACTIVE;
  for (int c = 0; c < 3; c++) f.sums[3 * i + c] = s.running[3 * (size_t)p + c];
  if (f.moments)
    for (int c = 0; c < 3; c++) f.moments[3 * i + c] = s.moments[3 * (size_t)p + c];
  if (f.counts) f.counts[i] = s.counts ? s.counts[p] : s.done;
}

// The reverse: packed pixel p takes its record, which is marked as claimed. False, and nothing
// written, when the blob holds none for it. (A pixel of two tiles writes equal marks twice.)
IZPI_PM bool scatter_pixel(const PixelMap& map, uint32_t p, const Packed& s, const Planes& f) {
  uint32_t x, y;
  map.xy(p, &x, &y);
  const size_t i = (size_t)y * map.width + x;
  const uint8_t st = f.state[i];
  if (st == NOT_IN_SESSION) return false;
  if (s.state) s.state[p] = st;
  for (int c = 0; c < 3; c++) s.running[3 * (size_t)p + c] = f.sums[3 * i + c];
  if (f.moments)
    for (int c = 0; c < 3; c++) s.moments[3 * (size_t)p + c] = f.moments[3 * i + c];
  if (f.counts && s.counts) s.counts[p] = f.counts[i];
  if (f.claimed) f.claimed[i] = 1;
  return true;
}

}  // namespace ck

// checkpoint_host.cpp, for the library's own units: the header of a session's blob from its
// request (the counters, pixels, samples, active, done and the checksum are the caller's to
// fill), the blob's checksum, and the validation of izpi_host_checkpoint_check with the message
// returned (null: the blob is this request's).
namespace izpi_internal {
ck::Header checkpoint_header(const izpi_render_req& req, uint32_t flags, uint64_t scene_tag);
uint64_t checkpoint_checksum(const void* blob, uint64_t bytes);
const char* checkpoint_check(const void* blob, uint64_t bytes, const izpi_render_req* req, uint64_t scene_tag,
                             char* msg, size_t msg_cap);
}  // namespace izpi_internal
