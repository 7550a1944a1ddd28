// denoise.hip — the edge-avoiding a-trous denoiser on the device:
// k_denoise and the izpi_gpu_denoise entries (include/izpi_gpu.h). The arithmetic is
// denoise.h's, shared with the host twin (denoise_host.cpp), so both give the same bits.
//
// One launch per iteration, one thread per pixel, 32 x 8 blocks: a wave covers two rows of
// 32 pixels, each row 1 KiB of contiguous canvas. An iteration reads C_i and the guides
// directly (the taps of steps 1 and 2 come out of L1 / L2, those of the wider steps out of
// the Infinity Cache, which holds the four canvases of a 1024 x 1024 frame) and writes
// C_{i+1}; iterations ping-pong between the caller's output and one scratch canvas the
// context keeps, so that the last one lands in the output.
#include "izpi_runtime.h"

#include "denoise.h"

namespace {

constexpr int kBlockX = 32, kBlockY = 8;
constexpr unsigned kMaxGridX = 1u << 16, kMaxGridY = 1u << 15;  // strides beyond that

template <bool HAS_N, bool HAS_A>
__global__ __launch_bounds__(kBlockX * kBlockY) void k_denoise(const double* C, const double* Nm, const double* A,
                                                                double* out, uint32_t width, uint32_t height,
                                                                dn::Iter it) {
  const int64_t W = width, H = height;
  for (int64_t y = (int64_t)blockIdx.y * kBlockY + threadIdx.y; y < H; y += (int64_t)gridDim.y * kBlockY)
    for (int64_t x = (int64_t)blockIdx.x * kBlockX + threadIdx.x; x < W; x += (int64_t)gridDim.x * kBlockX) {
      double o[4];
      dn::pixel<HAS_N, HAS_A>(C, Nm, A, W, H, x, y, it, o);
      double2* d = reinterpret_cast<double2*>(out + (y * W + x) * 4);  // a pixel is 32 B, 32-B aligned
      d[0] = make_double2(o[0], o[1]);
      d[1] = make_double2(o[2], o[3]);
    }
}

// The scratch canvas only grows: a smaller frame after a larger one reuses it.
int grow_scratch(izpi_ctx* ctx, size_t bytes) {
  if (ctx->denoise_cap >= bytes) return IZPI_OK;
  if (ctx->d_denoise) HIP_TRY(hipFree(ctx->d_denoise));
  ctx->d_denoise = nullptr;
  ctx->denoise_cap = 0;
  HIP_TRY(hipMalloc((void**)&ctx->d_denoise, bytes));
  ctx->denoise_cap = bytes;
  return IZPI_OK;
}

void launch(hipStream_t st, const double* src, const double* nm, const double* al, double* dst, uint32_t w, uint32_t h,
            const dn::Iter& it) {
  const dim3 block(kBlockX, kBlockY);
  const dim3 grid(std::min<unsigned>(kMaxGridX, (w + kBlockX - 1) / kBlockX),
                  std::min<unsigned>(kMaxGridY, (h + kBlockY - 1) / kBlockY));
  if (nm && al) hipLaunchKernelGGL((k_denoise<true, true>), grid, block, 0, st, src, nm, al, dst, w, h, it);
  else if (nm) hipLaunchKernelGGL((k_denoise<true, false>), grid, block, 0, st, src, nm, al, dst, w, h, it);
  else if (al) hipLaunchKernelGGL((k_denoise<false, true>), grid, block, 0, st, src, nm, al, dst, w, h, it);
  else hipLaunchKernelGGL((k_denoise<false, false>), grid, block, 0, st, src, nm, al, dst, w, h, it);
}

}  // namespace

extern "C" {

int izpi_gpu_denoise_device(izpi_ctx* ctx, const double* colour_dev, const double* normal_dev, const double* albedo_dev,
                            double* out_dev, uint32_t width, uint32_t height, const izpi_denoise_params* params,
                            double* device_ms) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (device_ms) *device_ms = 0.0;
  const izpi_denoise_params p = params ? *params : dn::defaults();
  if (const char* bad = dn::check_args(colour_dev, normal_dev, albedo_dev, out_dev, width, height, p)) {
    ctx->err = bad;
    return IZPI_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)width * height * 4 * sizeof(double);
  if (p.iterations > 1) {
    const int rc = grow_scratch(ctx, bytes);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  if (p.iterations == 0) HIP_TRY(hipMemcpyAsync(out_dev, colour_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  const double* src = colour_dev;
  for (uint32_t i = 0; i < p.iterations; i++) {
    double* dst = (p.iterations - 1 - i) % 2 == 0 ? out_dev : ctx->d_denoise;
    launch(ctx->stream, src, normal_dev, albedo_dev, dst, width, height, dn::iteration(p, i));
    HIP_TRY(hipGetLastError());
    src = dst;
  }
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  if (device_ms) *device_ms = ms;
  return IZPI_OK;
}

int izpi_gpu_denoise(izpi_ctx* ctx, const double* colour, const double* normal, const double* albedo, double* out,
                     uint32_t width, uint32_t height, const izpi_denoise_params* params, double* device_ms) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (device_ms) *device_ms = 0.0;
  const izpi_denoise_params p = params ? *params : dn::defaults();
  if (const char* bad = dn::check_args(colour, normal, albedo, out, width, height, p)) {
    ctx->err = bad;
    return IZPI_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t doubles = (size_t)width * height * 4, bytes = doubles * sizeof(double);
  DevBufs tmp;  // freed on every return
  double *d_colour, *d_normal = nullptr, *d_albedo = nullptr, *d_out;
  HIP_TRY(tmp.alloc(&d_colour, doubles));
  HIP_TRY(tmp.alloc(&d_out, doubles));
  HIP_TRY(hipMemcpy(d_colour, colour, bytes, hipMemcpyHostToDevice));
  if (normal) {
    HIP_TRY(tmp.alloc(&d_normal, doubles));
    HIP_TRY(hipMemcpy(d_normal, normal, bytes, hipMemcpyHostToDevice));
  }
  if (albedo) {
    HIP_TRY(tmp.alloc(&d_albedo, doubles));
    HIP_TRY(hipMemcpy(d_albedo, albedo, bytes, hipMemcpyHostToDevice));
  }
  const int rc = izpi_gpu_denoise_device(ctx, d_colour, d_normal, d_albedo, d_out, width, height, &p, device_ms);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost));
  return IZPI_OK;
}

}  // extern "C"
