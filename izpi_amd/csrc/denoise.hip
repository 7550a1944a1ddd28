// denoise.hip — the two a-trous denoisers on the device: the fixed-sigma filter (DESIGN.md
// section 3.8: k_denoise, the izpi_gpu_denoise entries) and the variance-guided one (section
// 3.8a: k_dnv_init, k_dnv, the izpi_gpu_denoise_var entries; include/izpi_gpu.h), and for
// both albedo demodulation (section 3.8b: k_demodulate, k_remodulate). The
// arithmetic is denoise.h's, shared with the host twin (denoise_host.cpp), so both give the
// same bits; the launch, the driver and the staging below are each written once for both.
//
// One launch per iteration, one thread per pixel, 32 x 8 blocks: a wave covers two rows of
// 32 pixels, each row 1 KiB of contiguous canvas. An iteration reads C_i and the guides
// directly (the taps of steps 1 and 2 come out of L1 / L2, those of the wider steps out of
// the Infinity Cache, which holds the four canvases of a 1024 x 1024 frame) and writes
// C_{i+1} (two 16-byte stores per pixel); the variance-guided one also reads V_i and writes
// V_{i+1} (one 8-byte store, a wave's 32 pixels of a row contiguous). The colour ping-pongs
// between the caller's output and one scratch canvas the context keeps, so that the last
// iteration lands in the output (every entry returns after its stream has finished, so the
// two filters never hold the scratch at once); the variance between the two planes of
// d_dnvar, the last one landing in the caller's plane when given.
#include "izpi_runtime.h"

#include "denoise.h"

namespace {

constexpr int kBlockX = 32, kBlockY = 8;
constexpr unsigned kMaxGridX = 1u << 16, kMaxGridY = 1u << 15;  // strides beyond that

__global__ __launch_bounds__(kBlockX * kBlockY) void k_dnv_init(const double* S, double* V, uint64_t pixels) {
  for (uint64_t p = (uint64_t)blockIdx.x * (kBlockX * kBlockY) + threadIdx.x; p < pixels;
       p += (uint64_t)gridDim.x * (kBlockX * kBlockY))
    V[p] = dn::variance0(S + p * 4);
}

// IZPI_DENOISE_DEMODULATE (section 3.8b): D_0 = C / m into the context's d_demod ahead of
// iteration 0, with VAR also V_0 from S / m (so that mode launches no k_dnv_init), and after
// the last iteration the albedo back in place on the output. k_dnv_init's launch shape; the
// inputs are read as pixel() reads them (plain doubles: they carry no alignment rule), the
// two canvases written in two 16-byte stores per pixel. Each pass moves a few canvases once.
__device__ inline void load_px(const double* at, double* px) {
  for (int k = 0; k < 4; k++) px[k] = at[k];
}
__device__ inline void store_px(double* at, const double* px) {
  double2* d = reinterpret_cast<double2*>(at);  // a pixel is 32 B, 32-B aligned
  d[0] = make_double2(px[0], px[1]);
  d[1] = make_double2(px[2], px[3]);
}

template <bool VAR>
__global__ __launch_bounds__(kBlockX * kBlockY) void k_demodulate(const double* C, const double* S, const double* A, double* D,
                                                                   double* V, uint64_t pixels) {
  for (uint64_t p = (uint64_t)blockIdx.x * (kBlockX * kBlockY) + threadIdx.x; p < pixels;
       p += (uint64_t)gridDim.x * (kBlockX * kBlockY)) {
    double c[4], s[4] = {0, 0, 0, 0}, a[4], d[4];
    load_px(C + p * 4, c);
    load_px(A + p * 4, a);
    if constexpr (VAR) load_px(S + p * 4, s);
    const double v = dn::demodulate<VAR>(c, s, a, d);
    store_px(D + p * 4, d);
    if constexpr (VAR) V[p] = v;
  }
}

template <bool VAR>
__global__ __launch_bounds__(kBlockX * kBlockY) void k_remodulate(const double* C, const double* S, const double* A, double* out,
                                                                   uint64_t pixels) {
  for (uint64_t p = (uint64_t)blockIdx.x * (kBlockX * kBlockY) + threadIdx.x; p < pixels;
       p += (uint64_t)gridDim.x * (kBlockX * kBlockY)) {
    double c[4], s[4] = {0, 0, 0, 0}, a[4], f[4];
    load_px(C + p * 4, c);
    load_px(A + p * 4, a);
    if constexpr (VAR) load_px(S + p * 4, s);
    load_px(out + p * 4, f);
    dn::remodulate<VAR>(c, s, a, f);
    store_px(out + p * 4, f);
  }
}

// The two kernels state their sweep themselves, k_dnv's being k_denoise's plus the variance
// store: a shared __device__ function between pixel() and the kernels gives the optimiser one
// more round over the tap loops, and the guide-less instances then come out peeled and
// unrolled differently (k_dnv<false, false> at 232 VGPRs for 124).
template <bool HAS_N, bool HAS_A>
__global__ __launch_bounds__(kBlockX * kBlockY) void k_denoise(const double* C, const double* Nm, const double* A,
                                                                double* out, uint32_t width, uint32_t height,
                                                                dn::Iter it) {
  const int64_t W = width, H = height;
  for (int64_t y = (int64_t)blockIdx.y * kBlockY + threadIdx.y; y < H; y += (int64_t)gridDim.y * kBlockY)
    for (int64_t x = (int64_t)blockIdx.x * kBlockX + threadIdx.x; x < W; x += (int64_t)gridDim.x * kBlockX) {
      double o[4];
      dn::pixel<HAS_N, HAS_A>(C, nullptr, Nm, A, W, H, x, y, it, o);
      double2* d = reinterpret_cast<double2*>(out + (y * W + x) * 4);  // a pixel is 32 B, 32-B aligned
      d[0] = make_double2(o[0], o[1]);
      d[1] = make_double2(o[2], o[3]);
    }
}

template <bool HAS_N, bool HAS_A>
__global__ __launch_bounds__(kBlockX * kBlockY) void k_dnv(const double* C, const double* V, const double* Nm, const double* A,
                                                           double* out, double* vout, uint32_t width, uint32_t height,
                                                           dnv::Iter it) {
  const int64_t W = width, H = height;
  for (int64_t y = (int64_t)blockIdx.y * kBlockY + threadIdx.y; y < H; y += (int64_t)gridDim.y * kBlockY)
    for (int64_t x = (int64_t)blockIdx.x * kBlockX + threadIdx.x; x < W; x += (int64_t)gridDim.x * kBlockX) {
      double o[4];
      const double v = dn::pixel<HAS_N, HAS_A>(C, V, Nm, A, W, H, x, y, it, o);
      double2* d = reinterpret_cast<double2*>(out + (y * W + x) * 4);
      d[0] = make_double2(o[0], o[1]);
      d[1] = make_double2(o[2], o[3]);
      vout[y * W + x] = v;
    }
}

template <class IT>
void launch(hipStream_t st, const double* src, const double* v, const double* nm, const double* al, double* dst, double* vdst,
            uint32_t w, uint32_t h, const IT& it) {
  const dim3 block(kBlockX, kBlockY);
  const dim3 grid(std::min<unsigned>(kMaxGridX, (w + kBlockX - 1) / kBlockX),
                  std::min<unsigned>(kMaxGridY, (h + kBlockY - 1) / kBlockY));
  dn::with_guides(nm, al, [&](auto n, auto a) {
    constexpr bool N = decltype(n)::value, A = decltype(a)::value;
    if constexpr (IT::kVar) hipLaunchKernelGGL((k_dnv<N, A>), grid, block, 0, st, src, v, nm, al, dst, vdst, w, h, it);
    else hipLaunchKernelGGL((k_denoise<N, A>), grid, block, 0, st, src, nm, al, dst, w, h, it);
  });
}

// The *_device entries. The scratch canvas is there only when iterations > 1, the planes only
// when iterations > 0 and D_0's canvas only for a demodulating call; all three only grow: a
// smaller frame after a larger one reuses them.
template <bool VAR>
int filter_device(izpi_ctx* ctx, const double* colour_dev, const double* stderr_dev, const double* normal_dev,
                  const double* albedo_dev, double* out_dev, double* var_out_dev, uint32_t width, uint32_t height,
                  const izpi_denoise_params* params, double variance_floor, double* device_ms) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (device_ms) *device_ms = 0.0;
  const izpi_denoise_params p = params ? *params : dn::defaults(VAR);
  if (const char* bad = dn::check_args(VAR, colour_dev, stderr_dev, normal_dev, albedo_dev, out_dev, var_out_dev, width,
                                       height, p, variance_floor)) {
    ctx->err = bad;
    return IZPI_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t pixels = (size_t)width * height, bytes = pixels * 4 * sizeof(double);
  if (p.iterations > 1) {
    const int rc = izpi_internal::grow(ctx, (void**)&ctx->d_denoise, &ctx->denoise_cap, bytes);
    if (rc) return rc;
  }
  if (VAR && p.iterations > 0) {
    const int rc = izpi_internal::grow(ctx, (void**)&ctx->d_dnvar, &ctx->dnvar_cap, 2 * pixels * sizeof(double));
    if (rc) return rc;
  }
  const bool demod = dn::demodulates(p);
  if (demod) {
    const int rc = izpi_internal::grow(ctx, (void**)&ctx->d_demod, &ctx->demod_cap, bytes);
    if (rc) return rc;
  }
  double* const planes[2] = {VAR ? ctx->d_dnvar : nullptr, VAR && ctx->d_dnvar ? ctx->d_dnvar + pixels : nullptr};
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  const dim3 per_pixel((unsigned)std::min<uint64_t>(1u << 20, (pixels + kBlockX * kBlockY - 1) / (kBlockX * kBlockY)));
  // V_0: into plane 0, or with no iteration to come straight into the caller's plane
  double* const v0 = !VAR ? nullptr : p.iterations ? planes[0] : var_out_dev;
  if (demod) {  // D_0, and V_0 with it
    hipLaunchKernelGGL(k_demodulate<VAR>, per_pixel, dim3(kBlockX * kBlockY), 0, ctx->stream, colour_dev, stderr_dev,
                       albedo_dev, ctx->d_demod, v0, (uint64_t)pixels);
    HIP_TRY(hipGetLastError());
  } else if (v0) {
    hipLaunchKernelGGL(k_dnv_init, per_pixel, dim3(kBlockX * kBlockY), 0, ctx->stream, stderr_dev, v0, (uint64_t)pixels);
    HIP_TRY(hipGetLastError());
  }
  if (p.iterations == 0) HIP_TRY(hipMemcpyAsync(out_dev, colour_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  const double* src = demod ? ctx->d_demod : colour_dev;
  for (uint32_t i = 0; i < p.iterations; i++) {
    const bool last = i + 1 == p.iterations;
    double* dst = (p.iterations - 1 - i) % 2 == 0 ? out_dev : ctx->d_denoise;
    double* vdst = last && var_out_dev ? var_out_dev : planes[(i + 1) % 2];
    launch(ctx->stream, src, planes[i % 2], normal_dev, albedo_dev, dst, vdst, width, height,
           dn::iteration<VAR>(p, variance_floor, i));
    HIP_TRY(hipGetLastError());
    src = dst;
  }
  if (demod) {  // the last iteration landed in out_dev
    hipLaunchKernelGGL(k_remodulate<VAR>, per_pixel, dim3(kBlockX * kBlockY), 0, ctx->stream, colour_dev, stderr_dev,
                       albedo_dev, out_dev, (uint64_t)pixels);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  if (device_ms) *device_ms = ms;
  return IZPI_OK;
}

// The host-pointer entries: device copies of what is given, the device entry, `out` and the
// plane (when asked for) back.
template <bool VAR>
int filter_staged(izpi_ctx* ctx, const double* colour, const double* stderr_host, const double* normal, const double* albedo,
                  double* out, double* var_out, uint32_t width, uint32_t height, const izpi_denoise_params* params,
                  double variance_floor, double* device_ms) {
  if (!ctx) return IZPI_ERR_INVALID;
  if (device_ms) *device_ms = 0.0;
  const izpi_denoise_params p = params ? *params : dn::defaults(VAR);
  if (const char* bad = dn::check_args(VAR, colour, stderr_host, normal, albedo, out, var_out, width, height, p, variance_floor)) {
    ctx->err = bad;
    return IZPI_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t pixels = (size_t)width * height, doubles = pixels * 4, bytes = doubles * sizeof(double);
  DevBufs tmp;  // freed on every return
  double* d_in[4] = {nullptr, nullptr, nullptr, nullptr};
  const double* const in[4] = {colour, stderr_host, normal, albedo};
  for (int k = 0; k < 4; k++)
    if (in[k]) {
      HIP_TRY(tmp.alloc(&d_in[k], doubles));
      HIP_TRY(hipMemcpy(d_in[k], in[k], bytes, hipMemcpyHostToDevice));
    }
  double *d_out, *d_var = nullptr;
  HIP_TRY(tmp.alloc(&d_out, doubles));
  if (var_out) HIP_TRY(tmp.alloc(&d_var, pixels));
  const int rc = filter_device<VAR>(ctx, d_in[0], d_in[1], d_in[2], d_in[3], d_out, d_var, width, height, &p, variance_floor,
                                    device_ms);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost));
  if (var_out) HIP_TRY(hipMemcpy(var_out, d_var, pixels * sizeof(double), hipMemcpyDeviceToHost));
  return IZPI_OK;
}

}  // namespace

extern "C" {

int izpi_gpu_denoise_device(izpi_ctx* ctx, const double* colour_dev, const double* normal_dev, const double* albedo_dev,
                            double* out_dev, uint32_t width, uint32_t height, const izpi_denoise_params* params,
                            double* device_ms) {
  return filter_device<false>(ctx, colour_dev, nullptr, normal_dev, albedo_dev, out_dev, nullptr, width, height, params, 0.0,
                              device_ms);
}

int izpi_gpu_denoise(izpi_ctx* ctx, const double* colour, const double* normal, const double* albedo, double* out,
                     uint32_t width, uint32_t height, const izpi_denoise_params* params, double* device_ms) {
  return filter_staged<false>(ctx, colour, nullptr, normal, albedo, out, nullptr, width, height, params, 0.0, device_ms);
}

int izpi_gpu_denoise_var_device(izpi_ctx* ctx, const double* colour_dev, const double* stderr_dev, const double* normal_dev,
                                const double* albedo_dev, double* out_dev, double* var_out_dev, uint32_t width,
                                uint32_t height, const izpi_denoise_params* params, double variance_floor,
                                double* device_ms) {
  return filter_device<true>(ctx, colour_dev, stderr_dev, normal_dev, albedo_dev, out_dev, var_out_dev, width, height,
                                params, variance_floor, device_ms);
}

int izpi_gpu_denoise_var(izpi_ctx* ctx, const double* colour, const double* stderr_host, const double* normal,
                         const double* albedo, double* out, double* var_out, uint32_t width, uint32_t height,
                         const izpi_denoise_params* params, double variance_floor, double* device_ms) {
  return filter_staged<true>(ctx, colour, stderr_host, normal, albedo, out, var_out, width, height, params, variance_floor,
                                device_ms);
}

}  // extern "C"
