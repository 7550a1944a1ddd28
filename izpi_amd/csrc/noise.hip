// noise.hip — the noise estimate of a progressive session on the device (DESIGN.md section
// 3.9): k_noise_resolve, the IZPI_SNAP_NOISE snapshot, and k_noise_stats, the frame statistic
// behind izpi_gpu_progressive_noise (include/izpi_gpu.h). The arithmetic is noise.h's, shared
// with the host twin (noise_host.cpp), so both give the same bits. The second moments both
// read are folded by k_accumulate's moments instance (wavefront.hip). A translation unit of
// its own, so the other units compile what they compiled before.
#include "izpi_runtime.h"
#include "noise.h"

// One thread per pixel in packed order: 48 B of sums and moments in, 32 B out; HBM-streaming.
// Writes (se_0, se_1, se_2, 1.0) where k_resolve writes the pixel.
__global__ void __launch_bounds__(256) k_noise_resolve(const NoiseParams np) {
  const SessionView& v = np.view;
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= v.map.num_pixels) return;
  double s[3], m2[3], se[3], e;
  v.load(p, s, m2);
  nz::pixel(s, m2, v.n(p), mean_by_reciprocal(v.sampler), np.floor, se, &e);
  store_pixel(v.map, p, np.out, se[0], se[1], se[2]);
}

// The frame statistic: one thread per pixel in packed order, blocks of nz::BLOCK = 256 = four
// waves. Every wave counts its counted, non-finite and above-threshold pixels by ballot and
// takes the maximum of its finite e on the bit pattern (non-negative doubles order as their
// bits); the four waves' figures meet in LDS and go out as the block's partials, which the
// host adds (one atomic per wave on four shared words measured 0.44 ms per 1024 x 1024
// evaluation, 27 times the kernel's bytes' worth: profiles/r13a/). sum_error's tree
// (izpi_gpu.h) is taken literally: strides 128 and 64 across the four waves through LDS,
// strides 32 ... 1 within the first wave by __shfl_down, and v[0] goes to block_sums, which the
// host adds in block order. No thread leaves before the barriers.
__global__ void __launch_bounds__(nz::BLOCK) k_noise_stats(const NoiseParams np) {
  __shared__ double v[nz::BLOCK];
  __shared__ unsigned long long part[nz::BLOCK / 64][4];
  const uint32_t t = threadIdx.x;
  const uint32_t p = blockIdx.x * nz::BLOCK + t;
  bool counted = false, fin = false;
  double e = 0.0;
  const SessionView& sv = np.view;
  if (p < sv.map.num_pixels) {
    uint32_t x, y;
    sv.map.xy(p, &x, &y);
    counted = y >= 1;
    double s[3], m2[3], se[3];
    sv.load(p, s, m2);
    fin = nz::pixel(s, m2, sv.n(p), mean_by_reciprocal(sv.sampler), np.floor, se, &e);
  }
  const bool good = counted && fin;
  const double mine = good ? e : 0.0;
  const unsigned long long n_counted = __popcll(__ballot(counted));
  const unsigned long long n_bad = __popcll(__ballot(counted && !fin));
  const unsigned long long n_above = __popcll(__ballot(good && e > np.threshold));
  // the wave's largest e (every term is >= +0.0)
  double mx = mine;
  for (int off = 32; off; off >>= 1) {
    const double o = __shfl_down(mx, off);
    mx = o > mx ? o : mx;
  }
  if ((t & 63u) == 0) {
    unsigned long long* w = part[t >> 6];
    w[0] = n_counted; w[1] = n_bad; w[2] = n_above; w[3] = gm::bits(mx);
  }
  v[t] = mine;
  __syncthreads();
  if (t < 4) {  // the block's pixels, nonfinite, above (sums) and the bits of its largest e (maximum)
    unsigned long long a = part[0][t];
    for (uint32_t w = 1; w < nz::BLOCK / 64; w++) a = t < 3 ? a + part[w][t] : (part[w][t] > a ? part[w][t] : a);
    np.block_counts[4 * (size_t)blockIdx.x + t] = a;
  }
  if (t < 128) v[t] = v[t] + v[t + 128];
  __syncthreads();
  if (t < 64) {
    double a = v[t] + v[t + 64];
    for (int stride = 32; stride; stride >>= 1) a = a + __shfl_down(a, stride);
    if (t == 0) np.block_sums[blockIdx.x] = a;
  }
}

void launch_noise_resolve(hipStream_t st, const NoiseParams& np) {
  hipLaunchKernelGGL(k_noise_resolve, dim3((np.view.map.num_pixels + 255) / 256), dim3(256), 0, st, np);
}
void launch_noise_stats(hipStream_t st, const NoiseParams& np) {
  hipLaunchKernelGGL(k_noise_stats, dim3((np.view.map.num_pixels + nz::BLOCK - 1) / nz::BLOCK), dim3(nz::BLOCK), 0, st, np);
}
