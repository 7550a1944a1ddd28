// displace.hip — the DISPLACE geometry operator on the device: adaptive tessellation and
// displacement of triangles by a float64 NRGBA map (displacement.ApplyDisplacementMap,
// displacement/displacement.go:143-280), the stage between a scene file and the GPU-built
// BVH4 (bvh_build.hip). The arithmetic is displace.h's, shared with the host twin
// (displace_host.cpp), so both give the same bits.
//
// The reference appends one triangle at a time; here a level is three steps over the work
// list (one izpi_tri_in per item, its source index in `pad`):
//   k_dsp_flag     one thread per parent: the 3 midpoints, the 6 texels its four children
//                  share, the mask of finished children; packs (finished, continuing)
//                  counts into one 64-bit word
//   exclusive scan rocPRIM, over the packed counts: both ranks at once
//   k_dsp_scatter  recomputes the children; a continuing child goes to its rank in the
//                  next level's list, a finished one is displaced on the spot (its texels
//                  are in registers) and written to its rank in the level's output
// The host reads one 8-byte total per level (at most IZPI_DISPLACE_MAX_LEVELS), so every
// buffer is sized exactly before the scatter writes it.
//
// Output order never depends on the order atomics arrive in: the mesh order is the levels'
// outputs one after another, each in scan order (parents' order times child 0..3), and the
// per-triangle order is a stable radix sort of that by source index. The only atomics are
// the integer adds of the per-source counts.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "displace.h"

static_assert(sizeof(izpi_tri_in) == 128, "a work item is one 128-B line");

namespace izpi_displace {

namespace {

#define DSP_TRY(expr)                                                       \
  do {                                                                      \
    hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess) {                                                 \
      err = std::string(#expr) + ": " + hipGetErrorString(e_);              \
      return IZPI_ERR_HIP;                                                  \
    }                                                                       \
  } while (0)

constexpr int kBlock = 256;
constexpr uint32_t kMaxBlocks = 1u << 20;  // grid-stride beyond that

struct Params {
  dsp::Map map;
  double max_du, max_dv, dmin, dmax;
};

// A record moves as eight 16-B accesses, so that a line is read and written whole.
__device__ __forceinline__ izpi_tri_in load_rec(const izpi_tri_in* p) {
  const double2* s = reinterpret_cast<const double2*>(p);
  double2 q[8];
#pragma unroll
  for (int k = 0; k < 8; k++) q[k] = s[k];
  izpi_tri_in t;
  __builtin_memcpy(&t, q, sizeof t);
  return t;
}
__device__ __forceinline__ void store_rec(izpi_tri_in* p, const izpi_tri_in& t) {
  double2 q[8];
  __builtin_memcpy(q, &t, sizeof t);
  double2* d = reinterpret_cast<double2*>(p);
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = q[k];
}

__global__ __launch_bounds__(kBlock) void k_dsp_flag(const izpi_tri_in* in, uint64_t n, Params p, uint8_t* mask,
                                                     uint64_t* packed) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const izpi_tri_in t = load_rec(in + i);
    dsp::Six s;
    dsp::six_points(t, s);
    double d[6];
    const uint32_t done = dsp::done_mask(s, p.map, p.max_du, p.max_dv, p.dmin, p.dmax, d);
    const uint32_t nd = (uint32_t)__builtin_popcount(done);
    mask[i] = (uint8_t)done;
    packed[i] = (uint64_t)nd | ((uint64_t)(4u - nd) << 32);
  }
}

// scan[i]: finished children before parent i in the low word, continuing ones in the high.
// fin == nullptr: count only (the sources of the finished children are still written).
__global__ __launch_bounds__(kBlock) void k_dsp_scatter(const izpi_tri_in* in, uint64_t n, Params p, const uint8_t* mask,
                                                        const uint64_t* scan, izpi_tri_in* next, izpi_tri_in* fin,
                                                        uint32_t* fin_src) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const izpi_tri_in t = load_rec(in + i);
    const uint32_t done = mask[i];
    const uint64_t base = scan[i];
    uint64_t at_done = base & 0xFFFFFFFFull, at_next = base >> 32;
    dsp::Six s;
    dsp::six_points(t, s);
    double d[6] = {0, 0, 0, 0, 0, 0};
    if (done && fin) {
      uint64_t at[6];
#pragma unroll
      for (int k = 0; k < 6; k++) at[k] = dsp::texel(p.map, s.p[k][3], s.p[k][4]);
#pragma unroll
      for (int k = 0; k < 6; k++) d[k] = p.map.z[at[k]];
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
      izpi_tri_in child;
      dsp::make_child(s, c, t, child);
      if ((done >> c) & 1u) {
        fin_src[at_done] = t.pad;
        if (fin) {
          izpi_tri_in o;
          dsp::displace(child, d[dsp::child_point(c, 0)], d[dsp::child_point(c, 1)], d[dsp::child_point(c, 2)], p.dmin,
                        p.dmax, o);
          store_rec(fin + at_done, o);
        }
        at_done++;
      } else {
        store_rec(next + at_next, child);
        at_next++;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_dsp_prepare(izpi_tri_in* in, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    in[i].pad = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_dsp_count(const uint32_t* src, uint64_t n, unsigned long long* counts) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    atomicAdd(&counts[src[i]], 1ull);
}

__global__ __launch_bounds__(kBlock) void k_dsp_iota(uint32_t* v, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    v[i] = (uint32_t)i;
}

// The levels' outputs, one after another in mesh order.
struct Chunks {
  const izpi_tri_in* p[IZPI_DISPLACE_MAX_LEVELS];
  uint64_t start[IZPI_DISPLACE_MAX_LEVELS + 1];
  int n;
};

// out[k] = the triangle at mesh position pos[k]
__global__ __launch_bounds__(kBlock) void k_dsp_gather(Chunks ch, const uint32_t* pos, uint64_t n, izpi_tri_in* out) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t m = pos[i];
    const izpi_tri_in* base = ch.p[0];
    uint64_t first = 0;
#pragma unroll  // constant indices: the table stays in scalar registers
    for (int l = 1; l < IZPI_DISPLACE_MAX_LEVELS; l++)
      if (l < ch.n && m >= ch.start[l]) {
        base = ch.p[l];
        first = ch.start[l];
      }
    store_rec(out + i, load_rec(base + (m - first)));
  }
}

dim3 grid_for(uint64_t n) { return dim3((unsigned)std::min<uint64_t>(kMaxBlocks, std::max<uint64_t>(1, (n + kBlock - 1) / kBlock))); }

// Device memory of one call, against the call's budget.
struct Arena {
  uint64_t budget = 0, held = 0;
  std::vector<void*> all;
  ~Arena() { for (void* p : all) if (p) (void)hipFree(p); }
  bool fits(uint64_t bytes) const { return bytes <= budget && held <= budget - bytes; }
  template <typename T>
  hipError_t alloc(T** out, uint64_t count) {
    const uint64_t bytes = std::max<uint64_t>(1, count) * sizeof(T);
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    all.push_back(p);
    sizes.push_back(bytes);
    held += bytes;
    *out = (T*)p;
    return hipSuccess;
  }
  void release(void* p) {
    for (size_t i = 0; i < all.size(); i++)
      if (all[i] == p && p) {
        (void)hipFree(p);
        held -= sizes[i];
        all[i] = nullptr;
      }
  }
  std::vector<uint64_t> sizes;
};

std::string mib(uint64_t b) { return std::to_string((b + (1u << 20) - 1) >> 20) + " MiB"; }

}  // namespace

const char* check(const izpi_tri_in* tris, uint64_t n, const double* rgba, uint32_t width, uint32_t height,
                  uint32_t order, const uint64_t* n_out) {
  return dsp::check_args(tris, n, rgba, width, height, order, n_out);
}

// See izpi_gpu_displace (include/izpi_host.h). Arguments are already checked (check).
int run(hipStream_t st, const izpi_tri_in* tris, uint64_t n, const double* rgba, uint32_t width, uint32_t height,
        double dmin, double dmax, uint32_t order, izpi_tri_in* out, uint64_t cap, uint64_t* n_out, uint64_t* counts,
        double* ms, std::string& err) {
  *n_out = 0;
  if (ms) *ms = 0.0;
  if (counts && n) memset(counts, 0, n * sizeof(uint64_t));
  if (n == 0) return IZPI_OK;
  size_t free_b = 0, total_b = 0;
  DSP_TRY(hipMemGetInfo(&free_b, &total_b));
  Arena mem;
  mem.budget = free_b / 2;  // the call's share of the free device memory
  auto refuse = [&](uint64_t need) {
    err = "displace: the work lists could need " + mib(need) + " more device memory; the call holds " + mib(mem.held) +
          " of its share of " + mib(mem.budget) + " (half of the free memory)";
    return IZPI_ERR_UNSUPPORTED;
  };
  // the map's blue channel, packed: a quarter of the bytes, and neighbours share lines
  const uint64_t texels = (uint64_t)width * height;
  if (!mem.fits(texels * 8 + n * (sizeof(izpi_tri_in) + 8))) return refuse(texels * 8 + n * (sizeof(izpi_tri_in) + 8));
  std::vector<double> blue(texels);
  for (uint64_t i = 0; i < texels; i++) blue[i] = rgba[4 * i + 2];
  double* d_map = nullptr;
  izpi_tri_in* d_in = nullptr;
  unsigned long long* d_counts = nullptr;
  DSP_TRY(mem.alloc(&d_map, texels));
  DSP_TRY(mem.alloc(&d_in, n));
  DSP_TRY(mem.alloc(&d_counts, n));
  struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } ev;
  DSP_TRY(hipEventCreate(&ev.a));
  DSP_TRY(hipEventCreate(&ev.b));
  const hipEvent_t e0 = ev.a, e1 = ev.b;
  DSP_TRY(hipMemcpyAsync(d_map, blue.data(), texels * 8, hipMemcpyHostToDevice, st));
  DSP_TRY(hipMemcpyAsync(d_in, tris, n * sizeof(izpi_tri_in), hipMemcpyHostToDevice, st));
  DSP_TRY(hipEventRecord(e0, st));
  DSP_TRY(hipMemsetAsync(d_counts, 0, n * 8, st));
  hipLaunchKernelGGL(k_dsp_prepare, grid_for(n), dim3(kBlock), 0, st, d_in, n);
  DSP_TRY(hipGetLastError());

  Params p;
  p.map = dsp::Map{d_map, width, height, 1};
  p.max_du = dsp::max_delta(width);
  p.max_dv = dsp::max_delta(height);
  p.dmin = dmin;
  p.dmax = dmax;

  Chunks ch;
  memset(&ch, 0, sizeof ch);
  std::vector<uint32_t*> src_chunks;
  uint64_t n_in = n, total = 0;
  for (int level = 1; n_in > 0; level++) {
    if (level > IZPI_DISPLACE_MAX_LEVELS) {
      DSP_TRY(hipStreamSynchronize(st));
      err = dsp::cap_message();
      return IZPI_ERR_UNSUPPORTED;
    }
    // the worst case of this level, all 4 n_in children, must fit before anything is launched
    // (and keeps every count below 2^32, so the packed halves cannot carry)
    const uint64_t worst = n_in * (1 + 16 + 32) + 4 * n_in * (sizeof(izpi_tri_in) + 4);
    if (4 * n_in + total >= 0xFFFFFFFFull || !mem.fits(worst)) return refuse(worst);
    uint8_t* d_mask = nullptr;
    uint64_t *d_packed = nullptr, *d_scan = nullptr;
    uint8_t* d_temp = nullptr;
    DSP_TRY(mem.alloc(&d_mask, n_in));
    DSP_TRY(mem.alloc(&d_packed, n_in + 1));
    DSP_TRY(mem.alloc(&d_scan, n_in + 1));
    DSP_TRY(hipMemsetAsync(d_packed + n_in, 0, 8, st));
    hipLaunchKernelGGL(k_dsp_flag, grid_for(n_in), dim3(kBlock), 0, st, d_in, n_in, p, d_mask, d_packed);
    DSP_TRY(hipGetLastError());
    size_t temp_bytes = 0;
    DSP_TRY(rocprim::exclusive_scan(nullptr, temp_bytes, d_packed, d_scan, (uint64_t)0, (size_t)(n_in + 1),
                                    rocprim::plus<uint64_t>(), st));
    DSP_TRY(mem.alloc(&d_temp, temp_bytes));
    DSP_TRY(rocprim::exclusive_scan(d_temp, temp_bytes, d_packed, d_scan, (uint64_t)0, (size_t)(n_in + 1),
                                    rocprim::plus<uint64_t>(), st));
    uint64_t totals = 0;
    DSP_TRY(hipMemcpyAsync(&totals, d_scan + n_in, 8, hipMemcpyDeviceToHost, st));
    DSP_TRY(hipStreamSynchronize(st));
    const uint64_t n_done = totals & 0xFFFFFFFFull, n_next = totals >> 32;
    if (n_done + n_next != 4 * n_in) { err = "displace: the level's counts do not add up"; return IZPI_ERR_DEVICE; }
    izpi_tri_in *d_next = nullptr, *d_fin = nullptr;
    uint32_t* d_src = nullptr;
    DSP_TRY(mem.alloc(&d_next, n_next));
    if (out) DSP_TRY(mem.alloc(&d_fin, n_done));
    DSP_TRY(mem.alloc(&d_src, n_done));
    hipLaunchKernelGGL(k_dsp_scatter, grid_for(n_in), dim3(kBlock), 0, st, d_in, n_in, p, d_mask, d_scan, d_next, d_fin,
                       d_src);
    DSP_TRY(hipGetLastError());
    if (n_done) {
      hipLaunchKernelGGL(k_dsp_count, grid_for(n_done), dim3(kBlock), 0, st, d_src, n_done, d_counts);
      DSP_TRY(hipGetLastError());
    }
    DSP_TRY(hipStreamSynchronize(st));
    mem.release(d_in);
    mem.release(d_mask);
    mem.release(d_packed);
    mem.release(d_scan);
    mem.release(d_temp);
    ch.p[ch.n] = d_fin;
    ch.start[ch.n] = total;
    ch.n++;
    ch.start[ch.n] = total + n_done;
    src_chunks.push_back(d_src);
    total += n_done;
    d_in = d_next;
    n_in = n_next;
  }
  mem.release(d_in);

  *n_out = total;
  const bool too_small = out && total > cap;
  izpi_tri_in* d_sorted = nullptr;
  if (out && !too_small && order == IZPI_DISPLACE_PER_TRIANGLE && total) {
    // stable sort of the mesh positions by source index, then one gather
    const uint64_t need = total * (4 * 4 + sizeof(izpi_tri_in));
    if (!mem.fits(need)) return refuse(need);
    uint32_t *keys = nullptr, *keys_s = nullptr, *pos = nullptr, *pos_s = nullptr;
    uint8_t* d_temp = nullptr;
    DSP_TRY(mem.alloc(&keys, total));
    DSP_TRY(mem.alloc(&keys_s, total));
    DSP_TRY(mem.alloc(&pos, total));
    DSP_TRY(mem.alloc(&pos_s, total));
    DSP_TRY(mem.alloc(&d_sorted, total));
    for (int l = 0; l < ch.n; l++) {
      const uint64_t c = ch.start[l + 1] - ch.start[l];
      if (c) DSP_TRY(hipMemcpyAsync(keys + ch.start[l], src_chunks[l], c * 4, hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(k_dsp_iota, grid_for(total), dim3(kBlock), 0, st, pos, total);
    DSP_TRY(hipGetLastError());
    unsigned bits = 1;
    while (bits < 32 && (n - 1) >> bits) bits++;
    size_t temp_bytes = 0;
    DSP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys, keys_s, pos, pos_s, (size_t)total, 0, bits, st));
    DSP_TRY(mem.alloc(&d_temp, temp_bytes));
    DSP_TRY(rocprim::radix_sort_pairs(d_temp, temp_bytes, keys, keys_s, pos, pos_s, (size_t)total, 0, bits, st));
    hipLaunchKernelGGL(k_dsp_gather, grid_for(total), dim3(kBlock), 0, st, ch, pos_s, total, d_sorted);
    DSP_TRY(hipGetLastError());
  }
  DSP_TRY(hipEventRecord(e1, st));
  if (counts) DSP_TRY(hipMemcpyAsync(counts, d_counts, n * 8, hipMemcpyDeviceToHost, st));
  if (out && !too_small && total) {
    if (d_sorted) {
      DSP_TRY(hipMemcpyAsync(out, d_sorted, total * sizeof(izpi_tri_in), hipMemcpyDeviceToHost, st));
    } else {
      for (int l = 0; l < ch.n; l++) {
        const uint64_t c = ch.start[l + 1] - ch.start[l];
        if (c) DSP_TRY(hipMemcpyAsync(out + ch.start[l], ch.p[l], c * sizeof(izpi_tri_in), hipMemcpyDeviceToHost, st));
      }
    }
  }
  DSP_TRY(hipStreamSynchronize(st));
  float f = 0;
  DSP_TRY(hipEventElapsedTime(&f, e0, e1));
  if (ms) *ms = f;
  if (too_small) {
    err = "displace: the output holds " + std::to_string(cap) + " triangles, " + std::to_string(total) + " are needed";
    return IZPI_ERR_INVALID;
  }
  return IZPI_OK;
}

}  // namespace izpi_displace
