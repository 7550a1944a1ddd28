// checkpoint_check.cpp — the host side of a session's checkpoint (izpi_amd/csrc/checkpoint_host.cpp)
// as a stand-alone program: tests/test_checkpoint.py builds it with the host sources only under
// AddressSanitizer and UBSan. Every array is a heap block of exactly its size, and the blobs are
// built here by hand from the format's description. One "pass <case>" line per case, then "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/izpi_host.h"
#include "../izpi_amd/csrc/checkpoint.h"

namespace {

int failures = 0;
void expect(bool ok, const std::string& name) {
  printf("%s %s\n", ok ? "pass" : "FAIL", name.c_str());
  if (!ok) failures++;
}

struct State {
  std::vector<double> sums, m2;
  std::vector<uint32_t> samples;
  std::vector<uint8_t> state;
};

// A session over `tiles`: values that depend on the pixel (x, y) alone, so that a pixel of two tiles agrees with itself.
State make_state(uint32_t W, const std::vector<uint32_t>& tiles, uint32_t tw, uint32_t th, uint32_t done) {
  State s;
  const uint32_t n = (uint32_t)(tiles.size() / 4) * tw * th;
  for (uint32_t p = 0; p < n; p++) {
    uint32_t x, y;
    tile_pixel(tiles.data(), tw, th, p, &x, &y);
    const uint32_t i = y * W + x;
    for (int c = 0; c < 3; c++) { s.sums.push_back(i + 0.25 * c); s.m2.push_back(2.0 * i + c); }
    const uint8_t st = (uint8_t)(i % 3);
    s.state.push_back(st);
    s.samples.push_back(st ? 2 + i % 5 : done);
  }
  return s;
}

std::vector<char> pack(uint32_t W, uint32_t H, const std::vector<uint32_t>& tiles, uint32_t flags, uint32_t done, const State& s,
                       bool listed) {
  uint64_t need = 0;
  if (izpi_host_checkpoint_pack(W, H, tiles.data(), (uint32_t)(tiles.size() / 4), flags, done, nullptr, nullptr, nullptr, nullptr,
                                nullptr, 0, &need))
    return {};
  std::vector<char> planes(need);
  if (izpi_host_checkpoint_pack(W, H, tiles.data(), (uint32_t)(tiles.size() / 4), flags, done, s.sums.data(),
                                (flags & IZPI_PROG_NOISE) ? s.m2.data() : nullptr, listed ? s.samples.data() : nullptr,
                                listed ? s.state.data() : nullptr, planes.data(), planes.size(), nullptr))
    return {};
  return planes;
}

void round_trip(const char* name, uint32_t W, uint32_t H, const std::vector<uint32_t>& tiles, uint32_t flags) {
  const uint32_t tw = tiles[2] - tiles[0] + 1, th = tiles[3] - tiles[1] + 1, nt = (uint32_t)(tiles.size() / 4), n = nt * tw * th;
  const bool adaptive = (flags & IZPI_PROG_ADAPTIVE) != 0;
  const State s = make_state(W, tiles, tw, th, 9);
  const std::vector<char> planes = pack(W, H, tiles, flags, 9, s, adaptive);
  bool ok = planes.size() == ck::Layout(W, H, flags).bytes - sizeof(ck::Header);
  State o;
  o.sums.assign(3 * (size_t)n, -1.0);
  if (flags & IZPI_PROG_NOISE) o.m2.assign(3 * (size_t)n, -1.0);
  if (adaptive) { o.samples.assign(n, 77); o.state.assign(n, 77); }
  uint64_t absent = 9, unclaimed = 9;
  ok = ok && izpi_host_checkpoint_unpack(W, H, tiles.data(), nt, flags, planes.data(), planes.size(), o.sums.data(),
                                         o.m2.empty() ? nullptr : o.m2.data(), adaptive ? o.samples.data() : nullptr,
                                         adaptive ? o.state.data() : nullptr, &absent, &unclaimed) == IZPI_OK;
  ok = ok && absent == 0 && unclaimed == 0 && o.sums == s.sums;
  if (flags & IZPI_PROG_NOISE) ok = ok && o.m2 == s.m2;
  if (adaptive) ok = ok && o.samples == s.samples && o.state == s.state;
  ok = ok && pack(W, H, tiles, flags, 9, o, adaptive) == planes;  // pack -> unpack -> pack
  expect(ok, std::string("round_trip ") + name + " flags " + std::to_string(flags));
}

// A whole blob: the header by hand, the planes of a 16 x 8 frame's two 8 x 8 tiles behind it.
std::vector<char> make_blob(const izpi_render_req& req, uint32_t flags, uint64_t tag, uint32_t done) {
  const std::vector<uint32_t> tiles = {0, 0, 7, 7, 8, 0, 15, 7};
  const State s = make_state(req.width, tiles, 8, 8, done);
  const std::vector<char> planes = pack(req.width, req.height, tiles, flags, done, s, (flags & IZPI_PROG_ADAPTIVE) != 0);
  ck::Header h;
  memset(&h, 0, sizeof h);
  h.magic = ck::MAGIC; h.version = ck::VERSION; h.header_bytes = sizeof h; h.blob_bytes = sizeof h + planes.size();
  h.flags = flags; h.listed = 1; h.width = req.width; h.height = req.height; h.sampler = req.sampler;
  h.accumulation = req.accumulation; h.max_depth = req.max_depth; h.num_bg_spd = req.num_bg_spd; h.seed = req.seed;
  memcpy(h.background, req.background, sizeof h.background);
  memcpy(h.ink, req.ink, sizeof h.ink);
  h.bg_digest = ck::hash_words(ck::hash_words(ck::HASH_BASIS, req.bg_spd_wavelengths, 8 * (uint64_t)req.num_bg_spd),
                               req.bg_spd_values, 8 * (uint64_t)req.num_bg_spd);
  h.pixels = 128; h.scene_tag = tag; h.done = done; h.spp = req.spp; h.samples = 1000; h.active = 40; h.cnt_n = 29;
  for (uint32_t k = 0; k < h.cnt_n; k++) h.counters[k] = 1000 + k;
  std::vector<char> blob(sizeof h + planes.size());
  memcpy(blob.data() + sizeof h, planes.data(), planes.size());
  memcpy(blob.data(), &h, sizeof h);
  h.checksum = ck::hash_words(ck::HASH_BASIS, blob.data() + ck::CHECKSUM_FROM, blob.size() - ck::CHECKSUM_FROM);
  memcpy(blob.data(), &h, sizeof h);
  return blob;
}

// check on a heap copy of exactly `bytes` bytes: status and message.
bool refused(const std::vector<char>& blob, size_t bytes, const izpi_render_req& req, uint64_t tag, const char* message) {
  char* copy = (char*)malloc(bytes ? bytes : 1);
  memcpy(copy, blob.data(), bytes);
  const int rc = izpi_host_checkpoint_check(copy, bytes, &req, tag);
  free(copy);
  if (!message) return rc == IZPI_OK;
  return rc == IZPI_ERR_INVALID && strstr(izpi_host_last_error(), message) != nullptr;
}

}  // namespace

int main() {
  const uint32_t kinds[] = {0, IZPI_PROG_NOISE, IZPI_PROG_NOISE | IZPI_PROG_ADAPTIVE};
  for (uint32_t flags : kinds) {
    round_trip("two 16 x 16 tiles", 40, 32, {16, 16, 31, 31, 0, 0, 15, 15}, flags);
    round_trip("overlapping tiles", 40, 30, {3, 2, 12, 9, 8, 5, 17, 12}, flags);
    round_trip("1 x 1", 1, 1, {0, 0, 0, 0}, flags);
    round_trip("1 x 7", 1, 7, {0, 0, 0, 6}, flags);
    round_trip("the last pixel of a 5 x 3 frame", 5, 3, {4, 2, 4, 2}, flags);
  }
  {  // a pixel without a record, a record without a pixel, and bad arguments
    const std::vector<uint32_t> tiles = {0, 0, 3, 3}, other = {1, 0, 4, 3};
    const State s = make_state(8, tiles, 4, 4, 5);
    const std::vector<char> planes = pack(8, 4, tiles, 0, 5, s, false);
    std::vector<double> sums(48, 0.0);
    uint64_t absent = 0, unclaimed = 0;
    const int rc = izpi_host_checkpoint_unpack(8, 4, other.data(), 1, 0, planes.data(), planes.size(), sums.data(), nullptr, nullptr,
                                               nullptr, &absent, &unclaimed);
    expect(rc == IZPI_OK && absent == 4 && unclaimed == 4, "pixel sets that differ by a column");
    expect(izpi_host_checkpoint_unpack(8, 4, other.data(), 1, 0, planes.data(), planes.size() - 8, sums.data(), nullptr, nullptr,
                                       nullptr, &absent, &unclaimed) == IZPI_ERR_INVALID, "planes of another size");
    const std::vector<uint32_t> outside = {5, 0, 8, 3};
    expect(izpi_host_checkpoint_pack(8, 4, outside.data(), 1, 0, 5, s.sums.data(), nullptr, nullptr, nullptr, nullptr, 0, nullptr) ==
               IZPI_ERR_INVALID, "a tile out of bounds");
    std::vector<char> small(planes.size() - 1);
    expect(izpi_host_checkpoint_pack(8, 4, tiles.data(), 1, 0, 5, s.sums.data(), nullptr, nullptr, nullptr, small.data(), small.size(),
                                     nullptr) == IZPI_ERR_INVALID, "an output one byte short");
  }
  {  // the header's reader and the validation
    std::vector<double> wl = {400, 550, 700}, val = {0.5, 1.0, 0.25};
    izpi_render_req req;
    memset(&req, 0, sizeof req);
    req.abi_version = IZPI_ABI_VERSION;
    req.width = 16; req.height = 8; req.spp = 32; req.max_depth = 9; req.sampler = IZPI_SAMPLER_SPECTRAL;
    req.accumulation = IZPI_ACC_FORWARD; req.seed = 99; req.background[1] = 0.5; req.ink[2] = 0.25;
    req.num_bg_spd = 3; req.bg_spd_wavelengths = wl.data(); req.bg_spd_values = val.data();
    const uint64_t tag = 0x1234567890ABCDEFull;
    const std::vector<char> blob = make_blob(req, IZPI_PROG_NOISE | IZPI_PROG_ADAPTIVE, tag, 12);
    expect(refused(blob, blob.size(), req, tag, nullptr), "the blob is this request's");
    uint64_t v = 0;
    bool ok = izpi_host_checkpoint_field(blob.data(), blob.size(), IZPI_CKPT_DONE, &v) == IZPI_OK && v == 12;
    ok = ok && izpi_host_checkpoint_field(blob.data(), blob.size(), IZPI_CKPT_COUNTER + 28, &v) == IZPI_OK && v == 1028;
    ok = ok && izpi_host_checkpoint_field(blob.data(), blob.size(), IZPI_CKPT_COUNTER + 29, &v) == IZPI_ERR_INVALID;
    ok = ok && izpi_host_checkpoint_field(blob.data(), sizeof(ck::Header), IZPI_CKPT_BLOB_BYTES, &v) == IZPI_OK && v == blob.size();
    ok = ok && izpi_host_checkpoint_field(blob.data(), blob.size(), IZPI_CKPT_COUNTS_OFFSET, &v) == IZPI_OK &&
         v == sizeof(ck::Header) + 128 + 2 * 24 * 128;
    expect(ok, "fields");
    expect(refused(blob, 0, req, tag, "truncated within the header"), "no bytes");
    expect(refused(blob, sizeof(ck::Header) - 1, req, tag, "truncated within the header"), "truncated in the header");
    expect(refused(blob, sizeof(ck::Header), req, tag, "truncated: 432 of"), "the header alone");
    expect(refused(blob, blob.size() - 1, req, tag, "truncated: "), "truncated in the last plane");
    std::vector<char> bad = blob;
    bad[sizeof(ck::Header) + 130] ^= 4;
    expect(refused(bad, bad.size(), req, tag, "checksum mismatch"), "one flipped payload byte");
    bad = blob;
    bad[0] = 'i';
    expect(refused(bad, bad.size(), req, tag, "bad magic"), "bad magic");
    expect(refused(blob, blob.size(), req, tag ^ 1, "scene tag"), "another scene tag");
    izpi_render_req q = req;
    q.spp = 11;
    expect(refused(blob, blob.size(), q, tag, "spp 11 is below the 12 samples done"), "spp below done");
    q = req; q.seed = 98;
    expect(refused(blob, blob.size(), q, tag, "request's seed differs"), "seed");
    q = req; q.max_depth = 10;
    expect(refused(blob, blob.size(), q, tag, "request's max_depth differs"), "max_depth");
    q = req; q.background[1] = 0.75;
    expect(refused(blob, blob.size(), q, tag, "request's background differs"), "background");
    std::vector<double> val2 = val;
    val2[2] = 0.5;
    q = req; q.bg_spd_values = val2.data();
    expect(refused(blob, blob.size(), q, tag, "request's bg_spd differs"), "one SPD value");
    q = req; q.spp = 12; q.out_layout = IZPI_OUT_PACKED; q.exposure = 4.0;
    expect(refused(blob, blob.size(), q, tag, nullptr), "spp, layout and exposure may differ");
    // a request of ABI 3 ends before `ink`: a heap block of exactly its size is read no further
    const size_t abi3 = offsetof(izpi_render_req, ink);
    izpi_render_req* old = (izpi_render_req*)malloc(abi3);
    memcpy(old, &req, abi3);
    old->abi_version = 3;
    char* copy = (char*)malloc(blob.size());
    memcpy(copy, blob.data(), blob.size());
    const int rc = izpi_host_checkpoint_check(copy, blob.size(), old, tag);
    expect(rc == IZPI_ERR_INVALID && strstr(izpi_host_last_error(), "request's ink differs"), "an ABI 3 request's ink is black");
    free(copy);
    free(old);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
