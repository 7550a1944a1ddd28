// adapt.hip — adaptive sampling of a progressive session on the device (DESIGN.md section 3.10,
// deviation A26): izpi_gpu_progressive_adapt's three launches. k_adapt_select evaluates the rule
// of noise.h (nz::pixel at n = done, nz::stays_active) for every active pixel and retires the
// others; k_adapt_scan turns the blocks' survivor counts into offsets; k_adapt_scatter writes the
// survivors, in packed order, as the table of 1 x 1 tiles that the next steps trace and shade
// instead of the request's tiles (start_path and camera_path read a tile's x and y and nothing
// else of it, so the hot kernels run the list as they are). No atomic decides a position: the
// list, and with it every unit's result slot, is the same on every run. The fold of a list's
// samples is k_accumulate's scatter instance (wavefront.hip). A translation unit of its own, so
// the other units compile what they compiled before.
#include "izpi_runtime.h"
#include "noise.h"

namespace {

constexpr uint32_t BLOCK = 256, WAVES = BLOCK / 64;

}  // namespace

// One thread per session pixel in packed order. An active pixel (state 0) is evaluated at
// n = done, which is its own count: retirement is final, so every active pixel has taken every
// sample. It stays active iff it is counted (sample row y >= 1), finite and e > threshold; else
// its state becomes 1, or 2 for a counted non-finite pixel, which the later calls still report.
// Every evaluated pixel's count is written (until the first retirement the steps do not keep
// it). Each wave counts by ballot; the block's three figures go out through LDS, as
// k_noise_stats' do. No thread leaves before the barrier.
__global__ void __launch_bounds__(BLOCK) k_adapt_select(const AdaptParams a) {
  __shared__ uint32_t part[WAVES][3];
  const uint32_t t = threadIdx.x;
  const uint32_t p = blockIdx.x * BLOCK + t;
  bool keep = false, counted = false, bad = false;
  const SessionView& v = a.view;
  if (p < v.map.num_pixels) {
    uint32_t x, y;
    v.map.xy(p, &x, &y);
    counted = y >= 1;
    const uint8_t s = a.state[p];
    if (s == 0) {
      double sum[3], m2[3], se[3], e;
      v.load(p, sum, m2);
      const bool fin = nz::pixel(sum, m2, v.done, mean_by_reciprocal(v.sampler), a.floor, se, &e);
      keep = nz::stays_active(counted, fin, e, a.threshold);
      bad = counted && !fin;
      if (!keep) a.state[p] = bad ? 2 : 1;
      a.counts[p] = v.done;
    } else {
      bad = s == 2;
    }
  }
  const uint32_t n_keep = __popcll(__ballot(keep)), n_counted = __popcll(__ballot(counted)), n_bad = __popcll(__ballot(bad));
  if ((t & 63u) == 0) {
    uint32_t* w = part[t >> 6];
    w[0] = n_keep; w[1] = n_counted; w[2] = n_bad;
  }
  __syncthreads();
  if (t < 3) {
    uint32_t v = part[0][t];
    for (uint32_t w = 1; w < WAVES; w++) v += part[w][t];
    if (t == 0) a.block_keep[blockIdx.x] = v;
    else a.block_stat[2 * (size_t)blockIdx.x + (t - 1)] = v;
  }
}

// One block. Thread t owns the blocks [t * per, (t + 1) * per): it adds their three figures, the
// 256 partial sums are scanned in LDS, and it then replaces each of its blocks' survivor counts
// by the survivors before that block. The frame's totals (integers: no order matters) go to
// `totals`, which the host reads.
__global__ void __launch_bounds__(BLOCK) k_adapt_scan(const AdaptParams a) {
  __shared__ uint32_t acc[BLOCK][3];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (a.blocks + BLOCK - 1) / BLOCK;
  const uint32_t b0 = min(t * per, a.blocks), b1 = min(b0 + per, a.blocks);
  uint32_t mine[3] = {0, 0, 0};
  for (uint32_t b = b0; b < b1; b++) {
    mine[0] += a.block_keep[b]; mine[1] += a.block_stat[2 * (size_t)b]; mine[2] += a.block_stat[2 * (size_t)b + 1];
  }
  for (int k = 0; k < 3; k++) acc[t][k] = mine[k];
  __syncthreads();
  for (uint32_t off = 1; off < BLOCK; off <<= 1) {  // inclusive scan of the threads' sums
    uint32_t add[3] = {0, 0, 0};
    if (t >= off)
      for (int k = 0; k < 3; k++) add[k] = acc[t - off][k];
    __syncthreads();
    for (int k = 0; k < 3; k++) acc[t][k] += add[k];
    __syncthreads();
  }
  uint32_t before = acc[t][0] - mine[0];
  for (uint32_t b = b0; b < b1; b++) {
    const uint32_t n = a.block_keep[b];
    a.block_keep[b] = before;
    before += n;
  }
  if (t == BLOCK - 1) {
    a.totals[0] = acc[t][0]; a.totals[1] = acc[t][1]; a.totals[2] = acc[t][2]; a.totals[3] = 0;
  }
}

// One thread per session pixel in packed order: a survivor's place is the survivors before its
// block (k_adapt_scan), before its wave in the block (LDS) and before its lane in the wave (the
// ballot's lower bits); its entry is (x, y, pixel, 0). The places are below the number of
// survivors, which is at most num_pixels, the table's entries.
__global__ void __launch_bounds__(BLOCK) k_adapt_scatter(const AdaptParams a) {
  __shared__ uint32_t wave_n[WAVES];
  const uint32_t t = threadIdx.x;
  const uint32_t p = blockIdx.x * BLOCK + t;
  const bool keep = p < a.view.map.num_pixels && a.state[p] == 0;
  const unsigned long long m = __ballot(keep);
  const uint32_t lane = t & 63u, wave = t >> 6;
  if (lane == 0) wave_n[wave] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  uint32_t pos = a.block_keep[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (uint32_t w = 0; w < wave; w++) pos += wave_n[w];
  uint32_t x, y;
  a.view.map.xy(p, &x, &y);
  *reinterpret_cast<uint4*>(a.table + 4 * (size_t)pos) = make_uint4(x, y, p, 0u);
}

// k_adapt_select for a session resumed from a checkpoint: the state bytes
// are the stored ones, and no rule is evaluated (retirement is final, and the thresholds of the
// earlier calls are not stored). It writes no state and no count; the blocks' three figures are
// k_adapt_select's, so k_adapt_scan and k_adapt_scatter build the list an adapt would have left.
__global__ void __launch_bounds__(BLOCK) k_adapt_select_state(const AdaptParams a) {
  __shared__ uint32_t part[WAVES][3];
  const uint32_t t = threadIdx.x;
  const uint32_t p = blockIdx.x * BLOCK + t;
  bool keep = false, counted = false, bad = false;
  if (p < a.view.map.num_pixels) {
    uint32_t x, y;
    a.view.map.xy(p, &x, &y);
    counted = y >= 1;
    const uint8_t s = a.state[p];
    keep = s == 0;
    bad = s == 2;
  }
  const uint32_t n_keep = __popcll(__ballot(keep)), n_counted = __popcll(__ballot(counted)), n_bad = __popcll(__ballot(bad));
  if ((t & 63u) == 0) {
    uint32_t* w = part[t >> 6];
    w[0] = n_keep; w[1] = n_counted; w[2] = n_bad;
  }
  __syncthreads();
  if (t < 3) {
    uint32_t v = part[0][t];
    for (uint32_t w = 1; w < WAVES; w++) v += part[w][t];
    if (t == 0) a.block_keep[blockIdx.x] = v;
    else a.block_stat[2 * (size_t)blockIdx.x + (t - 1)] = v;
  }
}

void launch_adapt_restore(hipStream_t st, const AdaptParams& ap) {
  hipLaunchKernelGGL(k_adapt_select_state, dim3(ap.blocks), dim3(BLOCK), 0, st, ap);
  hipLaunchKernelGGL(k_adapt_scan, dim3(1), dim3(BLOCK), 0, st, ap);
  hipLaunchKernelGGL(k_adapt_scatter, dim3(ap.blocks), dim3(BLOCK), 0, st, ap);
}

void launch_adapt(hipStream_t st, const AdaptParams& ap) {
  hipLaunchKernelGGL(k_adapt_select, dim3(ap.blocks), dim3(BLOCK), 0, st, ap);
  hipLaunchKernelGGL(k_adapt_scan, dim3(1), dim3(BLOCK), 0, st, ap);
  hipLaunchKernelGGL(k_adapt_scatter, dim3(ap.blocks), dim3(BLOCK), 0, st, ap);
}
