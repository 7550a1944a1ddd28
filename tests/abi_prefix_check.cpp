// Requests and tunings of older ABIs, allocated on the heap at exactly the size their
// caller's struct had, through request_copy and tuning_of (izpi_req.h). Built with
// -fsanitize=address,undefined by tests/test_abi.py: a read past the caller's object ends
// the program. Prints one line of copied fields per case.
#include <cstdio>
#include <cstdlib>

#include "../izpi_amd/csrc/izpi_req.h"

namespace {
constexpr size_t kOldReq = offsetof(izpi_render_req, accumulation);  // ABI 1 and 2 end at `tuning`
constexpr size_t kOldTuning = offsetof(izpi_render_tuning, tail_paths) + sizeof(uint64_t);  // ABI 1

// A request whose heap block holds `bytes` of the struct and nothing after them.
izpi_render_req* heap_request(size_t bytes, uint32_t abi, const izpi_render_tuning* tuning) {
  izpi_render_req full;
  memset(&full, 0, sizeof full);
  full.width = 64; full.height = 48; full.spp = 7; full.max_depth = 50;
  full.sampler = IZPI_SAMPLER_SPECTRAL;
  full.seed = 12345; full.post = IZPI_POST_SPECTRAL; full.exposure = 1.5;
  full.abi_version = abi;
  full.tuning = tuning;
  full.accumulation = IZPI_ACC_FORWARD;  // (only a full-sized block holds it)
  void* p = malloc(bytes);
  memcpy(p, &full, bytes);
  return static_cast<izpi_render_req*>(p);
}

izpi_render_tuning* heap_tuning(size_t bytes) {
  izpi_render_tuning full;
  memset(&full, 0, sizeof full);
  full.slots = 300; full.flags = IZPI_TUNE_NO_TAIL; full.tail_paths = 99;
  full.peer_timeout_ms = 4000;  // (only a full-sized block holds it)
  void* p = malloc(bytes);
  memcpy(p, &full, bytes);
  return static_cast<izpi_render_tuning*>(p);
}

void check(const char* what, size_t req_bytes, uint32_t abi, size_t tuning_bytes) {
  izpi_render_tuning* tu = tuning_bytes ? heap_tuning(tuning_bytes) : nullptr;
  izpi_render_req* req = heap_request(req_bytes, abi, tu);
  const izpi_render_req q = request_copy(req);
  const izpi_render_tuning t = tuning_of(req);
  printf("%s abi=%u width=%u height=%u spp=%u sampler=%u seed=%llu post=%u exposure=%g accumulation=%u pad_req=%u "
         "tuning=%d slots=%u flags=%u tail_paths=%llu peer_timeout_ms=%u\n",
         what, q.abi_version, q.width, q.height, q.spp, q.sampler, (unsigned long long)q.seed, q.post, q.exposure,
         q.accumulation, q.pad_req, q.tuning == tu, t.slots, t.flags, (unsigned long long)t.tail_paths, t.peer_timeout_ms);
  free(req);
  free(tu);
}
}  // namespace

int main() {
  check("abi0", kOldReq, 0, kOldTuning);
  check("abi0_no_tuning", kOldReq, 0, 0);
  check("abi2", kOldReq, 2, sizeof(izpi_render_tuning));
  check("abi3", sizeof(izpi_render_req), 3, sizeof(izpi_render_tuning));
  return 0;
}
