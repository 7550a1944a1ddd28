// trace_addr32_check.cpp — trace_layout / trace_addr32 (izpi_amd/csrc/scene_pack.h) on fabricated
// record counts around the 4-GiB limit, as a stand-alone host program: nothing is allocated.
// One line per case: name inner innerq leaves prims -> innerq_at leaves_at bytes addr32
#include <stdint.h>
#include <stdio.h>

#include "../izpi_amd/csrc/scene_pack.h"

using izpi_internal::trace_addr32;
using izpi_internal::trace_layout;
using izpi_internal::TraceLayout;

static void run(const char* name, uint64_t inner, uint64_t innerq, uint64_t leaves, uint64_t prims) {
  const TraceLayout t = trace_layout(inner, innerq, leaves);
  printf("%s %llu %llu %llu %llu -> %llu %llu %llu %d\n", name, (unsigned long long)inner, (unsigned long long)innerq,
         (unsigned long long)leaves, (unsigned long long)prims, (unsigned long long)t.innerq_at, (unsigned long long)t.leaves_at,
         (unsigned long long)t.bytes, (int)trace_addr32(inner, innerq, leaves, prims));
}

int main() {
  const uint64_t G4 = 1ull << 32;
  run("empty", 1, 0, 1, 0);
  run("c3_like", 190000, 0, 820000, 820000);
  // the node block: 128-B inner nodes, 64-B quantised nodes, 32-B leaf records
  run("inner_at_limit", G4 / 128, 0, 0, 1);
  run("inner_over", G4 / 128, 0, 1, 1);
  run("leaves_at_limit", 1, 0, (G4 - 128) / 32, 1);
  run("leaves_over", 1, 0, (G4 - 128) / 32 + 1, 1);
  run("quantised_at_limit", 1000, 1000, (G4 - 192000) / 32, 1);
  run("quantised_over", 1000, 1000, (G4 - 192000) / 32 + 1, 1);
  // the primitive records: 80 B, so 4 GiB is no whole number of them
  run("prims_under", 1, 0, 1, G4 / 80);
  run("prims_over", 1, 0, 1, G4 / 80 + 1);
  run("far_over", 1ull << 40, 0, 1ull << 40, 1ull << 40);
  return 0;
}
