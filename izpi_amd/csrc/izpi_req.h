// izpi_req.h — reading a caller's izpi_render_req and its tuning across ABI versions.
// Plain C++ (no HIP), so a host compiler can build and check it on its own
// (tests/abi_prefix_check.cpp).
#pragma once
#include <cstddef>
#include <cstring>

#include "../../include/izpi_gpu.h"

// The request's tuning. ABI 1's izpi_render_tuning ended at tail_paths (an ABI-1 request,
// abi_version 0, has its tuning pointer at the same place): its fields are read and the
// later ones keep their defaults.
inline izpi_render_tuning tuning_of(const izpi_render_req* req) {
  izpi_render_tuning t{};
  if (!req || !req->tuning) return t;
  if (req->abi_version >= 2) return *req->tuning;
  memcpy(&t, req->tuning, offsetof(izpi_render_tuning, tail_paths) + sizeof(t.tail_paths));
  return t;
}

// The library's own copy of the caller's request (req != NULL). A request of ABI 1 or 2
// (abi_version below 3) ends at `tuning`: only that prefix is the caller's to read, and
// the later fields are zero (accumulation = IZPI_ACC_RECURSIVE). A request of ABI 3 ends at
// `pad_req`: it is read up to `ink`, which stays zero (black).
inline izpi_render_req request_copy(const izpi_render_req* req) {
  izpi_render_req q;
  memset(&q, 0, sizeof q);
  memcpy(&q, req, req->abi_version < 3    ? offsetof(izpi_render_req, accumulation)
                  : req->abi_version == 3 ? offsetof(izpi_render_req, ink)
                                          : sizeof q);
  return q;
}
