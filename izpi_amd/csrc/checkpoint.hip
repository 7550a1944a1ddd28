// checkpoint.hip — a progressive session's checkpoint on the device (DESIGN.md section 3.11,
// deviation A28): the two reorder kernels between the packed order of a session's tiles and the
// frame-order planes of the blob, and the count of the records a resume claimed. The per-pixel
// rule is checkpoint.h's, which the host twins (checkpoint_host.cpp) read too. A translation
// unit of its own, so the other units compile what they compiled before.
#include "izpi_runtime.h"

static_assert(CNT_N <= ck::MAX_COUNTERS, "checkpoint.h: the header holds every device counter");
static_assert(CNT_RAYS == 0 && CNT_LSPH + 1 == ck::CARRIED_COUNTERS, "checkpoint.h: the reference counters lead the device's");

namespace {
constexpr uint32_t BLOCK = 256, WAVES = BLOCK / 64;

// The block's sum of the waves' ballot counts into counts[blockIdx.x]. Every thread of the block calls it.
__device__ __forceinline__ void block_count(bool flag, uint32_t* counts) {
  __shared__ uint32_t part[WAVES];
  const uint32_t t = threadIdx.x;
  const uint32_t n = __popcll(__ballot(flag));
  if ((t & 63u) == 0) part[t >> 6] = n;
  __syncthreads();
  if (t == 0) {
    uint32_t v = part[0];
    for (uint32_t w = 1; w < WAVES; w++) v += part[w];
    counts[blockIdx.x] = v;
  }
}
}  // namespace

// One thread per session pixel p in packed order: its state byte, sums, moments and count into
// the frame-order planes at y * W + x (PixelMap::xy). A packed tile row is contiguous on both
// sides. p < num_pixels and x < W, y < H (the tiles are validated): every index is in bounds.
__global__ void __launch_bounds__(BLOCK) k_ckpt_gather(const CkptParams c) {
  const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
  if (p < c.map.num_pixels) ck::gather_pixel(c.map, p, c.packed, c.planes);
}

// The reverse: pixel p takes its record and marks it claimed. A pixel whose record is absent
// (state 255) takes nothing and is counted, per block and in integers; the host adds the blocks
// and refuses on a non-zero total. No thread leaves before the barrier.
__global__ void __launch_bounds__(BLOCK) k_ckpt_scatter(const CkptParams c) {
  const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
  const bool absent = p < c.map.num_pixels && !ck::scatter_pixel(c.map, p, c.packed, c.planes);
  block_count(absent, c.block_counts);
}

// One thread per record of the frame: the records k_ckpt_scatter marked, counted per block. A
// pixel of two tiles marked its record twice and counts once: the total is the session's distinct
// pixels, which the host compares with the header's.
__global__ void __launch_bounds__(BLOCK) k_ckpt_claimed(const CkptParams c) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool claimed = i < (size_t)c.map.width * c.map.height && c.planes.claimed[i] != 0;
  block_count(claimed, c.block_counts);
}

void launch_ckpt_gather(hipStream_t st, const CkptParams& cp) {
  hipLaunchKernelGGL(k_ckpt_gather, dim3((cp.map.num_pixels + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, cp);
}
void launch_ckpt_scatter(hipStream_t st, const CkptParams& cp) {
  hipLaunchKernelGGL(k_ckpt_scatter, dim3((cp.map.num_pixels + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, cp);
}
void launch_ckpt_claimed(hipStream_t st, const CkptParams& cp) {
  const size_t n = (size_t)cp.map.width * cp.map.height;
  hipLaunchKernelGGL(k_ckpt_claimed, dim3((uint32_t)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, cp);
}
