// denoise_var.hip — the variance-guided a-trous denoiser on the device (DESIGN.md section
// 3.8a): k_dnv_init, k_dnv and the izpi_gpu_denoise_var entries (include/izpi_gpu.h). The
// arithmetic is denoise_var.h's, shared with the host twin (denoise_var_host.cpp), so both
// give the same bits.
//
// The launch form is k_denoise's (denoise.hip): one launch per iteration, one thread per
// pixel, 32 x 8 blocks, grid-stride beyond the grid limits. An iteration reads C_i, V_i and
// the guides and writes C_{i+1} (two 16-byte stores per pixel) and V_{i+1} (one 8-byte store,
// a wave's 32 pixels of a row contiguous). The colour ping-pongs between the caller's output
// and the context's scratch canvas, which it shares with izpi_gpu_denoise_device (every entry
// returns after its stream has finished, so the two never hold it at once); the variance
// between the two planes of d_dnvar, the last one landing in the caller's plane when given.
#include "izpi_runtime.h"

#include "denoise_var.h"

namespace {

constexpr int kBlockX = 32, kBlockY = 8;
constexpr unsigned kMaxGridX = 1u << 16, kMaxGridY = 1u << 15;  // strides beyond that

__global__ __launch_bounds__(kBlockX * kBlockY) void k_dnv_init(const double* S, double* V, uint64_t pixels) {
  for (uint64_t p = (uint64_t)blockIdx.x * (kBlockX * kBlockY) + threadIdx.x; p < pixels;
       p += (uint64_t)gridDim.x * (kBlockX * kBlockY))
    V[p] = dnv::variance0(S + p * 4);
}

template <bool HAS_N, bool HAS_A>
__global__ __launch_bounds__(kBlockX * kBlockY) void k_dnv(const double* C, const double* V, const double* Nm, const double* A,
                                                           double* out, double* vout, uint32_t width, uint32_t height,
                                                           dnv::Iter it) {
  const int64_t W = width, H = height;
  for (int64_t y = (int64_t)blockIdx.y * kBlockY + threadIdx.y; y < H; y += (int64_t)gridDim.y * kBlockY)
    for (int64_t x = (int64_t)blockIdx.x * kBlockX + threadIdx.x; x < W; x += (int64_t)gridDim.x * kBlockX) {
      double o[4];
      const double v = dnv::pixel<HAS_N, HAS_A>(C, V, Nm, A, W, H, x, y, it, o);
      double2* d = reinterpret_cast<double2*>(out + (y * W + x) * 4);
      d[0] = make_double2(o[0], o[1]);
      d[1] = make_double2(o[2], o[3]);
      vout[y * W + x] = v;
    }
}

void launch(hipStream_t st, const double* src, const double* v, const double* nm, const double* al, double* dst, double* vdst,
            uint32_t w, uint32_t h, const dnv::Iter& it) {
  const dim3 block(kBlockX, kBlockY);
  const dim3 grid(std::min<unsigned>(kMaxGridX, (w + kBlockX - 1) / kBlockX),
                  std::min<unsigned>(kMaxGridY, (h + kBlockY - 1) / kBlockY));
  if (nm && al) hipLaunchKernelGGL((k_dnv<true, true>), grid, block, 0, st, src, v, nm, al, dst, vdst, w, h, it);
  else if (nm) hipLaunchKernelGGL((k_dnv<true, false>), grid, block, 0, st, src, v, nm, al, dst, vdst, w, h, it);
  else if (al) hipLaunchKernelGGL((k_dnv<false, true>), grid, block, 0, st, src, v, nm, al, dst, vdst, w, h, it);
  else hipLaunchKernelGGL((k_dnv<false, false>), grid, block, 0, st, src, v, nm, al, dst, vdst, w, h, it);
}

}  // namespace

extern "C" {

int izpi_gpu_denoise_var_device(izpi_ctx* ctx, const double* colour_dev, const double* stderr_dev, const double* normal_dev,
                                const double* albedo_dev, double* out_dev, double* var_out_dev, uint32_t width,
                                uint32_t height, const izpi_denoise_params* params, double variance_floor,
                                double* device_ms) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (device_ms) *device_ms = 0.0;
  const izpi_denoise_params p = params ? *params : dnv::defaults();
  if (const char* bad = dnv::check_args(colour_dev, stderr_dev, normal_dev, albedo_dev, out_dev, var_out_dev, width, height,
                                        p, variance_floor)) {
    ctx->err = bad;
    return IZPI_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t pixels = (size_t)width * height, bytes = pixels * 4 * sizeof(double);
  if (p.iterations > 1) {
    const int rc = izpi_internal::grow(ctx, (void**)&ctx->d_denoise, &ctx->denoise_cap, bytes);
    if (rc) return rc;
  }
  if (p.iterations > 0) {
    const int rc = izpi_internal::grow(ctx, (void**)&ctx->d_dnvar, &ctx->dnvar_cap, 2 * pixels * sizeof(double));
    if (rc) return rc;
  }
  double* const planes[2] = {ctx->d_dnvar, ctx->d_dnvar ? ctx->d_dnvar + pixels : nullptr};
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  // V_0: into plane 0, or with no iteration to come straight into the caller's plane
  double* const v0 = p.iterations ? planes[0] : var_out_dev;
  if (v0) {
    const unsigned blocks = (unsigned)std::min<uint64_t>(1u << 20, (pixels + kBlockX * kBlockY - 1) / (kBlockX * kBlockY));
    hipLaunchKernelGGL(k_dnv_init, dim3(blocks), dim3(kBlockX * kBlockY), 0, ctx->stream, stderr_dev, v0, (uint64_t)pixels);
    HIP_TRY(hipGetLastError());
  }
  if (p.iterations == 0) HIP_TRY(hipMemcpyAsync(out_dev, colour_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  const double* src = colour_dev;
  for (uint32_t i = 0; i < p.iterations; i++) {
    const bool last = i + 1 == p.iterations;
    double* dst = (p.iterations - 1 - i) % 2 == 0 ? out_dev : ctx->d_denoise;
    double* vdst = last && var_out_dev ? var_out_dev : planes[(i + 1) % 2];
    launch(ctx->stream, src, planes[i % 2], normal_dev, albedo_dev, dst, vdst, width, height,
           dnv::iteration(p, variance_floor, i));
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

int izpi_gpu_denoise_var(izpi_ctx* ctx, const double* colour, const double* stderr_host, const double* normal,
                         const double* albedo, double* out, double* var_out, uint32_t width, uint32_t height,
                         const izpi_denoise_params* params, double variance_floor, double* device_ms) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (device_ms) *device_ms = 0.0;
  const izpi_denoise_params p = params ? *params : dnv::defaults();
  if (const char* bad = dnv::check_args(colour, stderr_host, normal, albedo, out, var_out, width, height, p, variance_floor)) {
    ctx->err = bad;
    return IZPI_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t pixels = (size_t)width * height, doubles = pixels * 4, bytes = doubles * sizeof(double);
  DevBufs tmp;  // freed on every return
  double *d_colour, *d_se, *d_normal = nullptr, *d_albedo = nullptr, *d_out, *d_var = nullptr;
  HIP_TRY(tmp.alloc(&d_colour, doubles));
  HIP_TRY(tmp.alloc(&d_se, doubles));
  HIP_TRY(tmp.alloc(&d_out, doubles));
  HIP_TRY(hipMemcpy(d_colour, colour, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_se, stderr_host, bytes, hipMemcpyHostToDevice));
  if (normal) {
    HIP_TRY(tmp.alloc(&d_normal, doubles));
    HIP_TRY(hipMemcpy(d_normal, normal, bytes, hipMemcpyHostToDevice));
  }
  if (albedo) {
    HIP_TRY(tmp.alloc(&d_albedo, doubles));
    HIP_TRY(hipMemcpy(d_albedo, albedo, bytes, hipMemcpyHostToDevice));
  }
  if (var_out) HIP_TRY(tmp.alloc(&d_var, pixels));
  const int rc = izpi_gpu_denoise_var_device(ctx, d_colour, d_se, d_normal, d_albedo, d_out, d_var, width, height, &p,
                                             variance_floor, device_ms);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost));
  if (var_out) HIP_TRY(hipMemcpy(var_out, d_var, pixels * sizeof(double), hipMemcpyDeviceToHost));
  return IZPI_OK;
}

}  // extern "C"
