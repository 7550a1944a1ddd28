/* izpi_gpu.h — C ABI of the MI355X path-tracing inner loop for izpi.
 *
 * Drop-in boundary: a Go `GPURenderer` implementing
 * render.Renderer (internal/render/renderer.go:26-28) flattens the scene once and
 * calls izpi_gpu_render per frame (or per tile batch), replacing
 *   render.New(...).Render(ctx)      leader/leader.go:136-158, renderer.go:73-222
 * and, per tile, the per-pixel loops
 *   renderRectRGB                     render/rgb.go:12-57
 *   renderRectSpectral / RenderPixelSpectral  render/spectral.go:14-106
 * The per-sample Sampler interface (sampler.go:30-33) is deliberately NOT the
 * boundary: cgo costs ~35 ns per call (hitable/bvh4_simd_arm64.go:14).
 *
 * Ownership: host arrays passed to izpi_gpu_upload_scene are read during the call
 * only; the library owns all device buffers inside the opaque context. Output
 * buffers are caller-allocated. Calls on one context are serialised by the caller;
 * one context per GPU. No C++ exception or abort() crosses this ABI: every entry
 * point returns an IZPI_* status and izpi_gpu_last_error() explains failures.
 */
#ifndef IZPI_GPU_H
#define IZPI_GPU_H
#include <stddef.h>
#include <stdint.h>
#include "izpi_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct izpi_ctx izpi_ctx;

/* Flattened scene, as the Go host holds it after transport.ToScene
 * (transport/transport.go:53-92) and hitable.NewBVH4 (hitable/bvh4.go:517-593).
 * Every per-triangle array is [num_tris][3] doubles unless noted. */
typedef struct izpi_scene_desc {
  uint32_t abi_version;      /* IZPI_ABI_VERSION */
  uint32_t num_nodes;        /* len(BVH4.Nodes) */
  uint32_t num_prims;        /* len(BVH4.Primitives) */
  uint32_t num_tris, num_spheres, num_lights, num_materials, num_textures;
  uint32_t num_spd;          /* entries in spd_wavelengths / spd_values */
  uint32_t flags;            /* IZPI_SCENE_* (ABI 3; was padding, 0 in ABI 1 and 2 descriptors) */
  uint64_t num_texels;       /* doubles in texels[] */
  const izpi_bvh4_node* nodes;  /* BVH4.Nodes, root = 0 (bvh4.go:42-47) */
  const uint32_t* prim_ref;     /* BVH4.Primitives (leaf order, bvh4.go:585-590) as IZPI_PRIM_REF */
  /* hitable.Triangle fields (triangle.go:20-52) */
  const double* tri_v0;
  const double* tri_v1;
  const double* tri_v2;
  const double* tri_e1;        /* edge1 = v1 - v0 */
  const double* tri_e2;        /* edge2 = v2 - v0 */
  const double* tri_normal;    /* unit(edge1 x edge2) */
  const double* tri_tangent;   /* normal-mapping frame */
  const double* tri_bitangent;
  const double* tri_uv;        /* [num_tris][6]: u0,v0,u1,v1,u2,v2 */
  const double* tri_area;      /* [num_tris] */
  const uint32_t* tri_mat;     /* [num_tris] material index */
  /* hitable.Sphere fields (sphere.go:20-27) */
  const double* sph_center0;   /* [num_spheres][3] */
  const double* sph_center1;   /* [num_spheres][3] */
  const double* sph_time;      /* [num_spheres][2]: time0, time1 */
  const double* sph_radius;    /* [num_spheres] */
  const uint32_t* sph_mat;     /* [num_spheres] */
  /* Scene.Lights = every hitable whose material IsEmitter() (transport.go:67-72) */
  const uint32_t* light_ref;   /* [num_lights] IZPI_PRIM_REF, transport order */
  const izpi_material* materials;
  const izpi_texture* textures;
  const double* texels;        /* image textures, float64 NRGBA */
  const double* spd_wavelengths;
  const double* spd_values;
  izpi_camera camera;
} izpi_scene_desc;

/* izpi_scene_desc.flags */
enum {
  /* Store the inner nodes' child boxes quantised to 8 bits per bound against a per-node f32
   * origin and power-of-two scale (64-B nodes instead of 128 B). Every decoded box contains
   * the node's own f32 box (rounded outwards; checked at upload in the kernels' own f32
   * arithmetic), so the traversal visits every node the exact boxes do, and maybe more: the
   * closest hit can differ only where two primitives are hit at the same t (A11) or a box
   * is culled at tMax by float rounding. The traversal is that of the BVH whose slot boxes
   * are the decoded ones (the oracle restates it, oracle_quantize_bvh4).
   * Ignored (the scene traverses its exact boxes) when a bound is not finite. */
  IZPI_SCENE_QUANTIZED_BVH = 1
};

/* render.New's sampler types (sampler.go:13-20). Colour and Spectral trace paths. The other
 * three are the preview samplers (render/rgb.go:27-41 around sampler/normal.go, albedo.go,
 * wireframe.go): one primary ray per sample, the Colour sampler's own (same seed, same
 * streams), max_depth and accumulation ignored, IZPI_POST_SPECTRAL refused:
 *  NORMAL:    the closest hit's normal as Hit leaves it (normal-mapped, a sphere's flipped
 *             towards the ray; components may be negative); a miss is (0, 0, 0).
 *  ALBEDO:    Material.Albedo at the closest hit: the albedo texture (Lambertian, PBR,
 *             Isotropic), the emit texture (DiffuseLight), Metal's albedo, (1, 1, 1) for a
 *             Dielectric; a miss is (0, 0, 0). Needs the RGB textures the Colour sampler needs.
 *  WIREFRAME: req->ink where HitableSlice.HitEdge (hitable_slice.go:48-70) reports an edge,
 *             else req->background (the paper). HitEdge traverses twice, the second time up
 *             to tMax = t + 2^-52, which is t itself from t = 4 upwards: a sphere hit that far
 *             away then fails `temp < tMax` and the sample is paper. Both traversals run and
 *             both count in node_visits / tri_tests / sph_tests.
 * stats.rays == stats.samples for the three (numRays counts Sample calls). */
enum {
  IZPI_SAMPLER_NORMAL = 1,
  IZPI_SAMPLER_COLOUR = 2,
  IZPI_SAMPLER_WIREFRAME = 3,
  IZPI_SAMPLER_ALBEDO = 4,
  IZPI_SAMPLER_SPECTRAL = 5
};
enum {
  IZPI_OUT_CANVAS = 0, /* W*H*4 float64 NRGBA canvas; pixel (x,y) lands in row H-y (rgb.go:41) */
  IZPI_OUT_PACKED = 1  /* tiles packed in request order, each (x1-x0+1)*(y1-y0+1)*4,
                          row-major by sample row y then x; the row-H-y rule is applied
                          by izpi_gpu_unpack_tiles */
};

/* Launch tuning of one render call. Every setting gives a bit-identical canvas and
 * identical counters; they trade memory and scheduling only. Zero fields take the
 * defaults, and a NULL izpi_render_req.tuning means all defaults. The library reads
 * no environment variables: an inherited variable cannot change a production render. */
typedef struct izpi_render_tuning {
  uint32_t slots;        /* cap on paths in flight; 0 = 256M, within 15/32 of the HBM this context may use */
  uint32_t chunk_units;  /* per-sample results held at once (pixels x spp of a chunk); 0 = 1/8 of that HBM */
  uint32_t rec_dense;    /* unwinding levels per record slot; 0 = 8 (Colour), 32 (Spectral) */
  uint32_t pool_div;     /* record slots per overflow block; 0 = 16 (Colour scenes without glass), 4 (others) */
  uint32_t trace_chunk;  /* queue entries per k_trace2 dequeue; 0 = 512 */
  uint32_t refill_min;   /* idle lanes before a k_trace2 refill (1..64); 0 = 24 (40 with the BVH in LDS) */
  uint32_t prim_weight;  /* k_trace2 primitive-step weight against node steps, x/16; 0 = 32 (24 with the BVH in LDS) */
  uint32_t flags;        /* IZPI_TUNE_* */
  uint64_t tail_paths;   /* k_tail takes over at <= this many paths; 0 = the resident lanes */
  /* izpi_gpu_render_rank: longest wait for the other ranks in one collective step, in ms
   * (the gather waits for the slowest rank's render: set it above a frame's time); past it,
   * or when RCCL reports an asynchronous error, the communicator is aborted and the call
   * returns IZPI_ERR_PEER. 0 = wait without a deadline (the async-error poll still runs). */
  uint32_t peer_timeout_ms;
  uint32_t pad_tuning;
} izpi_render_tuning;
enum {
  IZPI_TUNE_NO_DIST = 1,          /* k_trace2 runs each leaf's tests in its own lane */
  IZPI_TUNE_GENERAL_TRACE = 2,    /* the sphere-capable k_trace2 instance on triangle-only scenes */
  IZPI_TUNE_NO_LEAF_SHORTCUT = 4, /* re-test every leaf box (A10) instead of inferring it */
  IZPI_TUNE_SCALAR_SLAB = 8,      /* the scalar twin of RayAABB4 for every ray */
  IZPI_TUNE_NO_TAIL = 16,         /* no k_tail: wavefront passes to the end */
  IZPI_TUNE_PASS_LOG = 32,        /* diagnostics: per-pass device times on stderr */
  IZPI_TUNE_NO_LDS_BVH = 64,      /* small scenes: traverse from global memory, not the per-block LDS copy */
  IZPI_TUNE_NO_RAY_LDS = 128,     /* triangle-only scenes without (u, v) reads: primitive tests re-read the ray from global memory */
  IZPI_TUNE_NO_PRIM_LDS = 256,    /* small scenes: shading reads the primitives' records from global memory, not the per-block LDS copy */
  IZPI_TUNE_NO_PLACE_PICK = 512,  /* ignored since ABI 3 (the record arrays' page pick of ABI 2 is gone) */
  IZPI_TUNE_NO_QNODES = 1024,     /* a quantised scene (IZPI_SCENE_QUANTIZED_BVH): k_trace2 reads the decoded 128-B nodes
                                     instead of the 64-B quantised ones (the same boxes) */
  IZPI_TUNE_NO_SHADE_STAGE = 2048,/* forward Colour renders: k_shade reserves its output entries every block-iteration
                                     instead of every other one with the first's entries staged in LDS */
  IZPI_TUNE_WIDE_ADDR = 4096,     /* k_trace2 forms the 64-bit record addresses of a scene whose arrays pass 4 GiB,
                                     not 32-bit offsets from a scalar base */
  IZPI_TUNE_LEAF4 = 8192          /* k_trace2's distributed primitive step sized for leaves of four primitives on a
                                     scene whose leaves hold at most three */
};

typedef struct izpi_render_req {
  uint32_t width, height;     /* canvas size = Renderer sizeX, sizeY */
  uint32_t spp;               /* numSamples */
  uint32_t max_depth;         /* maxDepth (main.go:25 default 50) */
  uint32_t sampler;           /* IZPI_SAMPLER_* */
  uint32_t out_layout;        /* IZPI_OUT_* */
  uint32_t num_tiles;         /* 0 = whole frame in common.Tiles steps */
  uint32_t num_bg_spd;        /* entries of the spectral background SPD (0 = black) */
  const uint32_t* tiles;      /* [num_tiles][4] = x0,y0,x1,y1 inclusive (workUnit, renderer.go:56-70) */
  const double* bg_spd_wavelengths; /* spectral background (Spectral.background) */
  const double* bg_spd_values;
  double background[3];       /* Colour background (leader.go:140: black); the WireFrame sampler's paper */
  uint64_t seed;              /* master seed of the per-sample LCG streams */
  uint32_t post;              /* IZPI_POST_*: post-processing of a whole-frame IZPI_OUT_CANVAS render */
  uint32_t abi_version;       /* IZPI_ABI_VERSION (4); 0 = a request laid out by ABI 1 (this field was padding):
                                 its tuning, when set, is read as ABI 1's izpi_render_tuning, which ended at
                                 tail_paths; the later fields keep their defaults. A request of ABI 1 or 2
                                 ends at `tuning`: it renders IZPI_ACC_RECURSIVE. A request of ABI 3 ends
                                 at `pad_req`: its ink is black */
  double exposure;            /* XYZToRGB exposure (Scene.Exposure = camera exposure) */
  const izpi_render_tuning* tuning; /* NULL = defaults */
  uint32_t accumulation;      /* IZPI_ACC_* (ABI 3) */
  uint32_t pad_req;
  double ink[3];              /* IZPI_SAMPLER_WIREFRAME: the edge colour (render.New's ink); the paper is
                                 `background` (ABI 4) */
} izpi_render_req;

/* How a path's radiance is summed (izpi_render_req.accumulation). Both trace the same
 * rays with the same random draws, so every counter is the same.
 *  IZPI_ACC_RECURSIVE: the recursion of Colour.Sample / SampleSpectral (colour.go:44-57,
 *    sampler/spectral.go:60-72) unwound from the deepest bounce, in its operation order:
 *    bit-identical to the CPU restatement. The default.
 *  IZPI_ACC_FORWARD: the path's throughput is carried forward, T = (T * att) * (s / p) per
 *    non-specular bounce and T *= att per specular one, and the sample is T * (terminal
 *    radiance). Only the rounding differs (a few ulp per bounce; pixel RMSE < 1e-6, the
 *    north star's contract); NaN and Inf land where the recursion puts them (DESIGN.md
 *    section 3.2). No per-bounce records: a smaller, faster workspace. */
enum { IZPI_ACC_RECURSIVE = 0, IZPI_ACC_FORWARD = 1 };

/* Post-processing applied by Render for the Spectral sampler (renderer.go:215-219):
 * spectral.FireflyRejection (firefly_rejection.go:12-113) then spectral.XYZToRGB
 * (rgb_image.go:28-67, ACEScg matrix :13-17) with req->exposure. */
enum { IZPI_POST_NONE = 0, IZPI_POST_SPECTRAL = 1,
       /* bit 2: the leader's "png" output pipeline, Gamma then Clamp(1.0) (leader.go:179-182),
        * after the spectral post when both are set */
       IZPI_POST_GAMMA_CLAMP = 2 };

/* postprocess.Filter kinds for izpi_gpu_postprocess (postprocess/api.go:10-14) */
enum { IZPI_FILTER_GAMMA = 1, /* gamma.go:24-41, R,G,B = math.Sqrt; param unused */
       IZPI_FILTER_CLAMP = 2  /* clamp.go:27-51, v < max ? v : max; param = max */ };
#define IZPI_MAX_FILTERS 8

/* Per-render counters. The traversal is bit-identical to the CPU restatement, so
 * these equal the oracle's counts exactly (used for algorithmic bytes, §8(d)). */
typedef struct izpi_render_stats {
  uint64_t rays;          /* Sampler calls past the depth check == numRays (colour.go:38) */
  uint64_t node_visits;   /* BVH4 node loads (bvh4.go:91), incl. dielectric path-length traversals */
  uint64_t tri_tests;     /* Triangle.Hit calls inside traversal (bvh4.go:127) */
  uint64_t sph_tests;     /* Sphere.Hit calls inside traversal */
  uint64_t light_tri_tests; /* Triangle.PDFValue intersection tests (hitable_slice.go:98-105) */
  uint64_t light_sph_tests; /* Sphere.PDFValue intersection tests */
  uint64_t samples;       /* pixel samples evaluated */
  double kernel_ms;       /* device time of the traversal kernel (k_trace), HIP events on the library stream */
  double shade_ms;        /* device time of the shading kernel (k_shade) */
  double total_ms;        /* device time of the whole render call (kernels + accumulation) */
  uint32_t launches;      /* k_trace launches (wavefront iterations) in the call */
  uint32_t pad;
  /* traversal-kernel work breakdown (diagnostics, not reference quantities): wave-level
   * loop iterations that ran a node step / a primitive step, and leaf visits taken by a
   * shortcut (no node load). */
  uint64_t node_steps, prim_steps, leaf_shortcuts;
  /* device time of k_tail, which traces AND shades the last paths once every work unit
   * has started (not included in kernel_ms / shade_ms) */
  double tail_ms;
  /* the part of node_visits / tri_tests / sph_tests done inside k_tail */
  uint64_t tail_node_visits, tail_tri_tests, tail_sph_tests;
  /* shading passes deferred one pass for want of an overflow record block (diagnostic) */
  uint64_t parks;
  /* device memory of the context after the call: render workspace and uploaded scene */
  uint64_t workspace_bytes, scene_bytes;
  /* wavefront configuration of the call: paths in flight, unwinding records per path kept
   * in the dense array, overflow record blocks, samples per pixel per chunk */
  uint32_t slots, rec_dense, pool_blocks, chunk_spp;
  /* host wall time of the call's workspace allocations (a fresh context's first frame pays
   * for its HBM here; 0 when every buffer was already large enough) */
  double alloc_ms;
} izpi_render_stats;

/* Hit record returned by izpi_gpu_trace: BVH4.Hit (bvh4.go:49-164) followed by
 * the closest primitive's record (triangle.go:193-265 / sphere.go:63-95). */
typedef struct izpi_hit {
  double t, u, v;
  double p[3];
  double normal[3];
  uint32_t prim_ref;  /* IZPI_PRIM_REF of the closest primitive, 0xFFFFFFFF on miss */
  uint32_t hit;       /* 0/1 */
} izpi_hit;

/* Open a context on HIP device `device` (>=0). */
int izpi_gpu_open(int device, izpi_ctx** out);
int izpi_gpu_close(izpi_ctx* ctx);
const char* izpi_gpu_last_error(izpi_ctx* ctx);

/* Copy a flattened scene to the device (repacking to the GPU layouts of DESIGN.md). */
int izpi_gpu_upload_scene(izpi_ctx* ctx, const izpi_scene_desc* scene);

/* Render into a caller-owned HOST buffer: W*H*4 doubles for IZPI_OUT_CANVAS.
 * Pixels outside the requested tiles are left untouched (the caller zero-fills,
 * like floatimage.NewFloat64NRGBA). This is the Renderer.Render drop-in. */
int izpi_gpu_render(izpi_ctx* ctx, const izpi_render_req* req, double* out_host, izpi_render_stats* stats);

/* Size and allocate the render workspace of requests shaped like `req` (and run the device's
 * first work on it), so that the first frame renders only: the setup render.New does when it
 * allocates the canvas (renderer.go:73-104), ahead of the Render izpi times
 * (renderer.go:170,213). With a communicator (izpi_gpu_comm_init, nranks > 1) this rank's share
 * of izpi_gpu_render_rank is prepared. Optional: a render sizes its own workspace otherwise. */
int izpi_gpu_prepare(izpi_ctx* ctx, const izpi_render_req* req);

/* Same, but `out_dev` is a DEVICE pointer (e.g. a framebuffer owned by the caller
 * on this context's device). Used by multi-GPU runs that gather over RCCL. */
int izpi_gpu_render_device(izpi_ctx* ctx, const izpi_render_req* req, double* out_dev, izpi_render_stats* stats);

/* Scatter packed tiles (IZPI_OUT_PACKED, device memory) into a W*H*4 canvas
 * (device memory) applying the row = H - y rule of rgb.go:41 / spectral.go:36. */
int izpi_gpu_unpack_tiles(izpi_ctx* ctx, const izpi_render_req* req, const double* packed_dev, double* canvas_dev);

/* FireflyRejection + XYZToRGB of a W*H*4 float64 CIE-XYZ canvas (device memory) into
 * `rgba_dev` (device memory, may not alias `xyz_dev`): the multi-GPU path runs it on
 * rank 0 after the gather. */
int izpi_gpu_spectral_post(izpi_ctx* ctx, const double* xyz_dev, double* rgba_dev, uint32_t width, uint32_t height,
                           double exposure);

/* postprocess.Pipeline.Apply (pipeline.go:20-31) on a W*H*4 float64 canvas in device
 * memory, in place: filters[i] (IZPI_FILTER_*) with params[i], in list order. */
int izpi_gpu_postprocess(izpi_ctx* ctx, double* canvas_dev, uint32_t width, uint32_t height, const uint32_t* filters,
                         const double* params, uint32_t num_filters);

/* ---- Denoising a low-sample frame ---------------------------
 * An edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) over
 * a W*H*4 float64 canvas in Render's layout, with the Normal and Albedo frames of the same
 * view as edge-stopping guides (they share the Colour frame's primary rays, DESIGN 3.3a, so
 * they line up with it pixel for pixel). The project's own rule, not the reference's.
 *
 * Iteration i = 0..iterations-1 is a 5 x 5 B3-spline kernel with taps `1 << i` pixels apart;
 * a tap weighs h * exp(-(dc / (sigma_colour / 2^i)^2 + dn / sigma_normal^2 + da /
 * sigma_albedo^2)) with dc, dn, da the squared RGB distances to the centre in the three
 * frames. Pixels with alpha 0 (row 0, pixels outside the tiles) or a non-finite colour are
 * neither read as taps nor changed. Alpha is the centre's. iterations is 0..8 (0 copies);
 * every sigma is > 0 and may be +Inf (its term drops out); flags is 0 or
 * IZPI_DENOISE_DEMODULATE (below; it needs the albedo canvas). Anything else is
 * IZPI_ERR_INVALID. p == NULL: the defaults below. normal / albedo may be NULL: the term is
 * left out. out may not overlap an input; width and height are at least 1.
 *
 *  _denoise_device  all four canvases in device memory. Keeps one scratch canvas with the
 *                   context (it only grows) and ping-pongs so that the last iteration
 *                   lands in out_dev; returns after the stream has finished. *device_ms
 *                   (may be NULL): HIP-event time over the iterations. Needs no scene, and
 *                   touches none of a progressive session's workspace, so it is allowed
 *                   while one is open: a viewer denoises _snapshot_device output this way.
 *  _denoise         the same over host memory: upload, _denoise_device, download.
 *  izpi_host_denoise (izpi_host.h) is the twin on the host, bit for bit.
 * Multi-GPU callers run it on izpi_gpu_multi_context(m, 0) over the gathered canvas. */
typedef struct izpi_denoise_params {
  uint32_t iterations;
  uint32_t flags; /* 0 or IZPI_DENOISE_DEMODULATE */
  double sigma_colour, sigma_normal, sigma_albedo;
} izpi_denoise_params;
/* Albedo demodulation, an option of both filters: with this flag the
 * filter runs on irradiance, colour / albedo, and the albedo is multiplied back afterwards, so
 * texture detail is not smoothed. The albedo canvas is then required (it also stays the
 * edge-stopping guide under sigma_albedo) and should come from at least as many samples as the
 * frame. Channel k of a pixel is divided by m_k = its albedo when that is finite and greater
 * than IZPI_DENOISE_ALBEDO_FLOOR (2^-10), by the floor otherwise (the albedo's alpha is
 * ignored); the standard errors of the variance-guided filter are divided likewise, and V_0 is
 * the squared length of the quotients. A pixel whose colour is not live is not divided. After
 * the last iteration a pixel that was live in iteration 0 (its quotient live; its V_0 finite
 * and >= 0) is multiplied by m_k; every other pixel of `out` is the input's four doubles, bit
 * for bit. var_out is the variance of the filtered demodulated canvas, in the filter's own
 * space: a scalar plane cannot be multiplied back per channel. iterations == 0 means what it
 * means without the flag. Any other flag bit is refused. */
#define IZPI_DENOISE_DEMODULATE 4u
#define IZPI_DENOISE_ALBEDO_FLOOR 0.0009765625 /* 2^-10: dividing and multiplying by it is exact */
#define IZPI_DENOISE_MAX_ITERATIONS 8
#define IZPI_DENOISE_DEFAULT_ITERATIONS 5 /* sigma defaults 1.0, 0.5, 0.5: see DESIGN 3.8 */
#define IZPI_DENOISE_DEFAULT_SIGMA_COLOUR 1.0
#define IZPI_DENOISE_DEFAULT_SIGMA_NORMAL 0.5
#define IZPI_DENOISE_DEFAULT_SIGMA_ALBEDO 0.5
int izpi_gpu_denoise_device(izpi_ctx* ctx, const double* colour_dev, const double* normal_dev, const double* albedo_dev,
                            double* out_dev, uint32_t width, uint32_t height, const izpi_denoise_params* p,
                            double* device_ms);
int izpi_gpu_denoise(izpi_ctx* ctx, const double* colour, const double* normal, const double* albedo, double* out,
                     uint32_t width, uint32_t height, const izpi_denoise_params* p, double* device_ms);

/* ---- Variance-guided denoising of a noise session's frame ----
 * A second filter beside the one above, for frames that carry a measured error: the spatial
 * filter of SVGF (Schied et al., HPG 2017, section 4.4) without its temporal part. It takes,
 * with the canvas and the guides, the canvas of standard errors an IZPI_SNAP_NOISE snapshot
 * writes (se_0, se_1, se_2, 1.0; the alpha is ignored), and measures every colour
 * difference in the pixel's own variance, so that a pixel with many samples is left nearly
 * alone and one with few is smoothed: what a progressive or an adaptive session (whose
 * pixels carry different sample counts by design) needs. The project's own rule.
 *
 * V_0[p] = (se_0^2 + se_1^2) + se_2^2, a [H][W] float64 plane. A pixel is live when the
 * filter above takes it (alpha != 0, finite colour) and its V is finite and >= 0; others
 * are neither read as taps nor changed (their V is copied). Iteration i, taps `1 << i`
 * apart, of a live pixel: g = V_i through a 3 x 3 kernel {1/4, 1/2, 1/4}^2 at unit spacing
 * over the live pixels, kc = 1 / (sigma_colour^2 * (g + variance_floor)); then the 25 taps
 * of the filter above with e = dc * kc + dn / sigma_normal^2 + da / sigma_albedo^2 and
 * w = h * exp(-e); C_{i+1} = sum(w C_i) / sum(w), V_{i+1} = sum(w^2 V_i) / sum(w)^2.
 * sigma_colour is not halved per iteration: the variance shrinks instead. iterations == 0
 * copies the canvas and hands out V_0.
 *
 * p: an izpi_denoise_params under the rules above; p == NULL means 5 iterations, sigma_colour
 * IZPI_DENOISE_VAR_DEFAULT_SIGMA_COLOUR, sigma_normal and sigma_albedo 0.5. variance_floor
 * is finite and > 0 (IZPI_DENOISE_VAR_DEFAULT_FLOOR: the chosen default; it keeps a pixel
 * whose samples happened to agree from freezing). stderr_dev is required; out may overlap
 * neither an input nor var_out. var_out ([H][W] float64, may be NULL) receives the variance
 * of the filtered canvas (with IZPI_DENOISE_DEMODULATE: of the filtered demodulated canvas).
 *
 *  _denoise_var_device  all canvases and the plane in device memory. The colour ping-pong
 *                       shares the scratch canvas of _denoise_device; two variance planes
 *                       live in one more buffer of the context that only grows. Like
 *                       _denoise_device it needs no scene, returns after the stream has
 *                       finished and is allowed while a progressive session is open.
 *  _denoise_var         the same over host memory.
 *  izpi_host_denoise_var (izpi_host.h) is the twin on the host, bit for bit.
 * Multi-GPU callers run it on izpi_gpu_multi_context(m, 0) over gathered snapshots. */
#define IZPI_DENOISE_VAR_DEFAULT_SIGMA_COLOUR 1.5 /* and the floor: chosen on a grid, DESIGN 3.8a */
#define IZPI_DENOISE_VAR_DEFAULT_FLOOR 1e-4
int izpi_gpu_denoise_var_device(izpi_ctx* ctx, const double* colour_dev, const double* stderr_dev, const double* normal_dev,
                                const double* albedo_dev, double* out_dev, double* var_out_dev, uint32_t width,
                                uint32_t height, const izpi_denoise_params* p, double variance_floor, double* device_ms);
int izpi_gpu_denoise_var(izpi_ctx* ctx, const double* colour, const double* stderr_host, const double* normal,
                         const double* albedo, double* out, double* var_out, uint32_t width, uint32_t height,
                         const izpi_denoise_params* p, double variance_floor, double* device_ms);

/* GPU BVH4 builder: Morton codes and a radix sort, then a binary
 * tree (method: IZPI_BVH_PLOC clustering or IZPI_BVH_LBVH radix tree), collapsed to
 * 4-wide nodes with collectChildren's rule (or, with IZPI_BVH_SAH, the collapse of least
 * surface-area cost) and <= leaf_max (1..4) primitives per leaf, written in the reference's BVH4Node
 * format (conservative f32 bounds, separate leaf nodes), breadth-first with the root at
 * 0. boxes: [n][6] f64 host array (izpi_host_scene_prim_boxes). nodes: host array of at
 * least 2n entries; order[k] (n entries) = input index of leaf position k. The topology
 * differs from hitable.NewBVH4's, so images match the reference tree's except for
 * equal-t tie-breaks and f32 culling at tMax. */
enum { IZPI_BVH_LBVH = 0, /* Karras radix tree over the Morton order */
       IZPI_BVH_PLOC = 1, /* locally-ordered clustering (Meister & Bittner 2018) over the Morton order */
       /* flag (PLOC only): collapse to 4-wide nodes by the surface-area cost model's
        * dynamic programme instead of collectChildren's rule; leaves still hold <= leaf_max */
       IZPI_BVH_SAH = 0x100 };
int izpi_gpu_build_bvh4(izpi_ctx* ctx, const double* boxes, uint32_t n, uint32_t leaf_max, uint32_t method,
                        izpi_bvh4_node* nodes, uint32_t max_nodes, uint32_t* num_nodes, uint32_t* order, double* build_ms);

/* ---- Multi-GPU (SURVEY.md §8(b),(e)) ---------------------------------------------
 * Render fans out over the GPUs of the node in ONE call, as RendererImpl.Render fans
 * out over its workers (render/renderer.go:123-147): one host thread and stream per
 * device instead of one goroutine per core. The frame's tiles (common.Tiles in
 * grid.WalkGrid's spiral order, or req->tiles) become the units of izpi_host_share_units
 * (quarter tiles, where they can be cut), dealt unit % G == i (izpi_host.h lists the
 * steps); device i renders its share packed; the shares are gathered to device 0 (peer copies over xGMI), which
 * scatters them into the W*H*4 canvas (row H - y, rgb.go:41) and applies req->post.
 * Per pixel-sample RNG streams make the canvas bit-identical for every G. A device may
 * appear twice in `devices` (two contexts on one GPU). */
typedef struct izpi_multi izpi_multi;
int izpi_gpu_multi_open(const int* devices, uint32_t num_devices, izpi_multi** out);
int izpi_gpu_multi_close(izpi_multi* m);
const char* izpi_gpu_multi_last_error(izpi_multi* m);
uint32_t izpi_gpu_multi_size(izpi_multi* m);
/* context of device i (e.g. for izpi_gpu_build_bvh4), owned by `m` */
izpi_ctx* izpi_gpu_multi_context(izpi_multi* m, uint32_t i);
/* the scene is replicated on every device */
int izpi_gpu_multi_upload_scene(izpi_multi* m, const izpi_scene_desc* scene);
/* izpi_gpu_prepare for every device's share of `req` */
int izpi_gpu_multi_prepare(izpi_multi* m, const izpi_render_req* req);
/* out_host: the caller's W*H*4 canvas (read first: pixels of no tile keep their values),
 * or NULL to leave the canvas in device 0's memory (timing). stats: [num_devices] or NULL. */
int izpi_gpu_multi_render(izpi_multi* m, const izpi_render_req* req, double* out_host, izpi_render_stats* stats);

/* One process per GPU (torchrun / MPI style launchers): the library's own RCCL
 * communicator. Rank 0 makes the id with izpi_gpu_comm_id and the launcher broadcasts
 * it; every rank calls izpi_gpu_comm_init on its context. */
#define IZPI_COMM_ID_BYTES 128 /* == NCCL_UNIQUE_ID_BYTES */
int izpi_gpu_comm_id(uint8_t* id /* [IZPI_COMM_ID_BYTES] */);
int izpi_gpu_comm_init(izpi_ctx* ctx, uint32_t nranks, uint32_t rank, const uint8_t* id /* [IZPI_COMM_ID_BYTES] */);
/* Collective: every rank passes the same whole-frame request. Rank r renders the tiles
 * t % nranks == r, ncclGather moves the packed shares to rank 0, which writes the canvas
 * into out_dev (device memory on its GPU; ignored on other ranks) and applies req->post.
 * stats: this rank's share. Every rank runs the same collectives whatever fails locally
 * (its own HIP errors included), and two ncclAllReduce(max) agreement steps (after the
 * buffers, after the gather) give every rank the worst status: a rank's own failure returns
 * its status, a failure of another rank IZPI_ERR_PEER (last_error names the rank).
 * A rank that dies or hangs instead of failing: each collective step is waited on by
 * polling the stream and ncclCommGetAsyncError; an asynchronous RCCL error, or a wait past
 * tuning->peer_timeout_ms, aborts the communicator (ncclCommAbort) and returns
 * IZPI_ERR_PEER. The context then has no communicator: izpi_gpu_comm_init makes a new one. */
int izpi_gpu_render_rank(izpi_ctx* ctx, const izpi_render_req* req, double* out_dev, izpi_render_stats* stats);

/* Progress of the render running on ctx (izpi_gpu_render, _render_device, _render_rank),
 * callable from another thread while it runs (RendererImpl.Render's per-tile progress
 * bar, renderer.go:119-121, rgb.go:54-56): samples (pixels x spp) whose paths have
 * finished, as of the library's last queue poll (every <= 8 wavefront passes, a lower
 * bound), and the request's samples. After the call returns, done == total (both 0 when
 * the request failed its checks), whether or not it succeeded. The multi
 * form sums the contexts of `m` (their shares of one frame). */
int izpi_gpu_progress(izpi_ctx* ctx, uint64_t* samples_done, uint64_t* samples_total);
int izpi_gpu_multi_progress(izpi_multi* m, uint64_t* samples_done, uint64_t* samples_total);

/* ---- Progressive rendering ---------------------------------------------------------
 * render.New's previewChan and a cancellable ctx (render/rgb.go:18-52, spectral.go:20-52),
 * in the form a wavefront renderer has them: the frame's samples are rendered in steps, the
 * per-pixel sums stay on the device, and a snapshot normalised by the samples done so far
 * can be taken after any step. Sample s of a pixel draws from its own stream whatever the
 * request's spp, and the sums are folded in sample order, so a session that has rendered k
 * samples in ANY split of steps snapshots exactly the canvas izpi_gpu_render writes at
 * spp = k, bit for bit, with the same counters.
 *
 *  begin     req->spp is the session's cap N; every other field means what it means to
 *            izpi_gpu_render and is checked as there. The workspace is sized and allocated
 *            as a request of step_spp samples (>= 1, clipped to N) would size it; the sums
 *            and counters start at zero. `req` and what it points to are copied. A context
 *            holds one session: a second begin is IZPI_ERR_INVALID.
 *  step      renders samples [done, done + min(spp, N - done)); spp == 0 means step_spp. A
 *            step of more than step_spp samples runs in pieces of at most step_spp. At
 *            done == N a no-op. stats (may be NULL) are cumulative since begin: the counters
 *            equal a one-shot render's at spp = done; times and launches are the steps' sums.
 *  snapshot  resolves the sums, without changing them, into a caller-owned buffer of
 *            izpi_gpu_output_bytes(req): host memory (read first, as izpi_gpu_render reads
 *            it: pixels outside the tiles keep their values) or, _device, device memory.
 *            IZPI_SNAP_CANVAS is what izpi_gpu_render writes at spp = done, req->post
 *            included. IZPI_SNAP_DISPLAY holds the pixels of display.DisplayTile
 *            (render/rgb.go:43-51, spectral.go:38-46): B, G, R, 1.0, for the Spectral
 *            sampler XYZToACEScg of the exposed X, Y, Z (rgb_image.go:13-22), without
 *            FireflyRejection and without req->post; same layout. IZPI_ERR_INVALID before
 *            the first sample.
 *  end       closes the session (the cancellation point: a caller whose ctx is cancelled
 *            stops stepping and ends). The workspace stays with the context.
 * While a session is open izpi_gpu_render, _render_device, _render_rank, _prepare,
 * _upload_scene, _trace and _debug_realloc return IZPI_ERR_INVALID and leave it intact;
 * izpi_gpu_close ends it; izpi_gpu_progress reports (pixels * done + the running step's
 * progress, pixels * N). */
enum { IZPI_SNAP_CANVAS = 0, IZPI_SNAP_DISPLAY = 1 };
int izpi_gpu_progressive_begin(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp);
int izpi_gpu_progressive_step(izpi_ctx* ctx, uint32_t spp, izpi_render_stats* stats);
int izpi_gpu_progressive_snapshot(izpi_ctx* ctx, uint32_t form, double* out_host);
int izpi_gpu_progressive_snapshot_device(izpi_ctx* ctx, uint32_t form, double* out_dev);
int izpi_gpu_progressive_end(izpi_ctx* ctx);
/* The same over the devices of `m`, with izpi_gpu_multi_render's share plan: every device
 * holds a session over its share's units (packed), steps run on the per-device threads, and a
 * snapshot gathers the resolved shares to device 0, which scatters them into the canvas and
 * applies req->post (IZPI_SNAP_CANVAS). out_host: the caller's W*H*4 canvas, read first.
 * stats: [num_devices] or NULL. izpi_gpu_multi_render, _multi_prepare and _multi_upload_scene
 * return IZPI_ERR_INVALID while the session is open. */
int izpi_gpu_multi_progressive_begin(izpi_multi* m, const izpi_render_req* req, uint32_t step_spp);
int izpi_gpu_multi_progressive_step(izpi_multi* m, uint32_t spp, izpi_render_stats* stats);
int izpi_gpu_multi_progressive_snapshot(izpi_multi* m, uint32_t form, double* out_host);
int izpi_gpu_multi_progressive_end(izpi_multi* m);

/* ---- The noise estimate of a progressive session (deviation A25) ----
 * How noisy is the frame, where, and may the caller stop? The project's own rule: the
 * reference has no such estimate, and no entry above computes it unasked. A session begun
 * with IZPI_PROG_NOISE keeps, next to each pixel's sums s_c, the second moments of its
 * samples, m2_c = m2_c + x_c * x_c, folded by the pass that folds the sums, in sample order
 * (24 B per pixel, a buffer of the context's own that only grows). x is what is added to the
 * sums: for a forward Spectral render the weighed X, Y, Z. The sums keep their additions: the
 * CANVAS and DISPLAY snapshots and the counters are those of a session without the flag.
 *
 * Per pixel after n = done >= 2 samples (no fused multiply-add anywhere):
 *   mean_c = the canvas rule: s_c / n (Colour, the preview samplers), s_c * (1 / n) (Spectral)
 *   v_c    = (m2_c - (s_c * s_c) / n) / (n - 1);  !(v_c > 0) -> 0
 *   se_c   = sqrt(v_c / n)                        (the standard error of the mean)
 *   e      = ((se_0 + se_1) + se_2) / (((|mean_0| + |mean_1|) + |mean_2|) + floor)
 * A pixel is non-finite when a sum, a moment or e is not finite. A pixel is counted when its
 * sample row y >= 1 (row 0 lands on canvas row H and is dropped: it must not hold a render
 * open). Over the counted pixels, in packed order p (tile after tile, by y then x):
 *   pixels, nonfinite, above (finite pixels with e > threshold), max_error (largest finite e),
 *   sum_error: each block of 256 consecutive p fills v[0..255] with e (+0.0 for a pixel that
 *   is not counted, not finite, or past the end), adds v[i] = v[i] + v[i + stride] for i <
 *   stride, stride = 128, 64, ..., 1, and the blocks' v[0] are added in block order.
 * The integers and the maximum depend on no order; sum_error on the blocking only. The multi
 * form adds the devices' integers, takes the maximum of their maxima and adds their
 * sum_error in device order: sum_error (and nothing else) depends on the share plan in its
 * last bits. converged = done >= min_spp && (double)above <= tolerated * (double)(pixels -
 * nonfinite).
 *
 * The defaults are placeholders from one look at a 40 x 40 Cornell box (forward accumulation,
 * seed 12345: median e 0.47 at 4 spp, 0.18 at 32). A handful of samples UNDERESTIMATES the
 * variance wherever most of them are black (the share of pixels above 0.25 rises from 0.59 at
 * 2 spp to 0.82 at 4 before it falls): min_spp keeps a frame from "converging" on such an
 * estimate, so do not set it to 2 without a reason.
 *
 *  begin_ex   _begin with flags: IZPI_PROG_NOISE, with or without IZPI_PROG_ADAPTIVE (below), or 0
 *             (any other bit, the flag value 2 among them: IZPI_ERR_INVALID).
 *             _begin is _begin_ex(..., 0).
 *  snapshot   IZPI_SNAP_NOISE (every snapshot entry): (se_0, se_1, se_2, 1.0) per pixel in the
 *             session's layout, by IZPI_SNAP_CANVAS's row and tile rule, without req->post;
 *             Spectral values are in XYZ, the sums' space; a non-finite pixel holds what the
 *             arithmetic gives. IZPI_ERR_INVALID without the flag or with done < 2.
 *  noise      the frame statistic (p == NULL: the defaults). threshold and floor finite and
 *             > 0, tolerated in [0, 1], flags 0, a session with the flag and done >= 2: else
 *             IZPI_ERR_INVALID. device_ms: HIP-event time of the statistic's kernel (the
 *             multi form: the largest of the devices').
 *  converge   repeats step(step_spp) then, once done >= max(2, min_spp), noise, until the
 *             frame is converged or done == N. The decision reads above, pixels and
 *             nonfinite only: a multi-GPU session stops at the same done as one GPU. stats /
 *             noise (either may be NULL) are the last step's and the last evaluation's
 *             (noise->done == 0: none was made). stats of the multi form: [num_devices].
 * All of them need an open session. izpi_host_noise (izpi_host.h) is the twin on the host. */
enum { IZPI_PROG_NOISE = 1 };  /* izpi_gpu_progressive_begin_ex's flags */
enum { IZPI_SNAP_NOISE = 2 };  /* with IZPI_SNAP_CANVAS, IZPI_SNAP_DISPLAY */
typedef struct izpi_noise_params {
  double threshold, floor, tolerated;
  uint32_t min_spp;
  uint32_t flags; /* 0 */
} izpi_noise_params;
#define IZPI_NOISE_DEFAULT_THRESHOLD 0.25 /* placeholders: see above */
#define IZPI_NOISE_DEFAULT_FLOOR 0.01
#define IZPI_NOISE_DEFAULT_TOLERATED 0.05
#define IZPI_NOISE_DEFAULT_MIN_SPP 8
typedef struct izpi_noise_stats {
  uint64_t pixels, nonfinite, above;
  double max_error, sum_error, device_ms;
  uint32_t done, converged;
} izpi_noise_stats;
int izpi_gpu_progressive_begin_ex(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp, uint32_t flags);
int izpi_gpu_progressive_noise(izpi_ctx* ctx, const izpi_noise_params* p, izpi_noise_stats* out);
int izpi_gpu_progressive_converge(izpi_ctx* ctx, const izpi_noise_params* p, izpi_render_stats* stats,
                                  izpi_noise_stats* noise);
int izpi_gpu_multi_progressive_begin_ex(izpi_multi* m, const izpi_render_req* req, uint32_t step_spp, uint32_t flags);
int izpi_gpu_multi_progressive_noise(izpi_multi* m, const izpi_noise_params* p, izpi_noise_stats* out);
int izpi_gpu_multi_progressive_converge(izpi_multi* m, const izpi_noise_params* p, izpi_render_stats* stats,
                                        izpi_noise_stats* noise);

/* ---- Adaptive sampling of a progressive session (deviation A26) ----
 * A session begun with IZPI_PROG_NOISE | IZPI_PROG_ADAPTIVE stops sampling the pixels whose
 * noise estimate has fallen to the threshold. The project's own rule, like the estimate: no
 * entry above computes it unasked. Sample s of pixel (x, y) draws from its own stream, and sums
 * and moments fold in sample order, so a pixel's value after n samples depends on that pixel and
 * n alone: EVERY PIXEL OF AN ADAPTIVE FRAME IS, BIT FOR BIT, THE PIXEL OF A PLAIN RENDER AT THAT
 * PIXEL'S OWN SAMPLE COUNT n_p, and the counts follow the rule below.
 *
 * The session keeps n_p (uint32) per pixel and an active set; every pixel starts active with
 * n_p = 0 (a buffer of the context's own that only grows; no workspace plan counts it).
 *   step    renders samples [done, done + k') of the ACTIVE pixels only, k' = min(k, N - done),
 *           folds them in sample order and adds k' to their n_p. Retirement is final, so every
 *           active pixel has n_p == done. With no active pixel a step renders nothing and
 *           leaves done as it is.
 *   adapt   (done >= 2, else IZPI_ERR_INVALID; p == NULL: the defaults, checked as _noise checks
 *           them) evaluates every active pixel by the rule above at n = done. The pixel STAYS
 *           ACTIVE iff it is counted (sample row y >= 1), finite and e > threshold; every other
 *           pixel retires for good with n_p = done. Uncounted pixels never reach a canvas and
 *           non-finite ones can never converge: both retire at the first evaluation. tolerated
 *           and min_spp do not bear on a retirement. out (may be NULL): pixels and nonfinite as
 *           _noise counts them, active after this call, retired by this call, samples = the sum
 *           of n_p over the session's pixels, device_ms of the call's kernels, done, and
 *           converged = done >= min_spp && (double)active <= tolerated * (double)(pixels -
 *           nonfinite).
 *   converge  on an adaptive session: step(step_spp), then adapt once done >= max(2, min_spp),
 *           until adapt reports converged or done == N. Integers only: every share plan stops
 *           alike. A session in which no pixel is active (an earlier adapt, legal from done >= 2
 *           whatever min_spp is, retired them all) has nothing left to render: converge returns
 *           at once with done as it is. noise (may be NULL) is _noise's statistic of the frame
 *           as the call leaves it, when the call made an adapt or found no active pixel (else
 *           noise->done == 0); its converged is _noise's, so 0 while done < min_spp.
 *   snapshot, noise  use n_p wherever they used done (the mean, the standard errors, e). A
 *           retired pixel's sums no longer change, so noise's above equals adapt's active.
 *           IZPI_SNAP_SAMPLES writes (n_p, n_p, n_p, 1.0) as doubles by IZPI_SNAP_CANVAS's row and
 *           tile rule, without req->post: the sample-count map. IZPI_ERR_INVALID on a session
 *           that is not adaptive.
 * The counters are additive per sample: they equal the sum, over the steps, of a plain render
 * of exactly the samples each step rendered. stats->samples is the sum of n_p, and
 * izpi_gpu_progress reports it against pixels * N. Until the first retirement (adapt never
 * called, or nothing retired yet) the session runs the plain session's kernels: its sums,
 * moments, counters and CANVAS / DISPLAY / NOISE snapshots are those of a session begun with
 * IZPI_PROG_NOISE alone, bit for bit.
 * IZPI_PROG_ADAPTIVE without IZPI_PROG_NOISE, or with a preview sampler (one ray per sample: not
 * worth adapting), is IZPI_ERR_INVALID. The multi form: every device adapts its own share (the
 * rule is per pixel, so the image and the map are one device's); the integers are added and
 * device_ms is the largest. izpi_host_adapt (izpi_host.h) is the twin on the host. */
enum { IZPI_PROG_ADAPTIVE = 4 };  /* with IZPI_PROG_NOISE; the flag value 2 stays unknown: callers were promised that the flag words 2 and 3 are refused */
enum { IZPI_SNAP_SAMPLES = 3 };   /* with IZPI_SNAP_CANVAS, IZPI_SNAP_DISPLAY, IZPI_SNAP_NOISE */
typedef struct izpi_adapt_stats {
  uint64_t pixels, nonfinite, active, retired, samples;
  double device_ms;
  uint32_t done, converged;
} izpi_adapt_stats;
int izpi_gpu_progressive_adapt(izpi_ctx* ctx, const izpi_noise_params* p, izpi_adapt_stats* out);
int izpi_gpu_multi_progressive_adapt(izpi_multi* m, const izpi_noise_params* p, izpi_adapt_stats* out);

/* ---- Checkpoint and resume of a progressive session (deviation A28) ----
 * A session's state lives in device memory of one process. A checkpoint is that state as one
 * self-describing byte blob in host memory, which the caller stores wherever they like. Sample
 * s of pixel (x, y) draws from its own stream, sums and moments fold in sample order, and a
 * session's result depends neither on how its steps were cut nor on the share plan, so: A SESSION
 * THAT IS EXPORTED, ENDED AND RESUMED IS, BIT FOR BIT, THE UNINTERRUPTED SESSION, in another
 * process, on another context or over another number of devices: canvas, standard errors,
 * sample-count map, adapt's integers and the reference counters. The project's own addition.
 *
 * The blob, little-endian: a 432-byte header, then per-pixel planes of width * height entries in
 * sample-coordinate row-major order (y * W + x: sample rows, not canvas rows; no tile list and
 * no share plan shows in it): a state byte (0 active, 1 retired, 2 retired as a counted
 * non-finite pixel, 255 not in this session), the sums (3 doubles), with IZPI_PROG_NOISE the
 * second moments (3 doubles), with IZPI_PROG_ADAPTIVE n_p (uint32); the byte and the uint32
 * planes are padded to 8 bytes. A pixel that is not in the session holds zeros. The header
 * (izpi_host_checkpoint_field reads it): magic "IZPICKPT", version, its size, the blob's size,
 * a checksum of everything after it (FNV-1a over 64-bit words), the session flags and whether a
 * pixel has retired, the request fields that decide a sample (width, height, sampler,
 * accumulation, max_depth, seed, background, ink, the background SPD's length and digest), the
 * session's distinct pixels, the caller's 64-bit scene tag (izpi_host_scene_tag), done, the sum
 * of n_p, the active pixels, the cap at export, and the device counters: the six reference
 * counters (rays, node_visits, tri_tests, sph_tests, light_tri_tests, light_sph_tests) with their
 * values, the diagnostic ones (node_steps, prim_steps, leaf_shortcuts, the tail's share, parks)
 * as 0: those depend on how the hardware scheduled the waves, differ between two runs of one
 * session, and count from the resume on. No time and no pointer: the blob is a function of the
 * session's state alone, and two exports of one state give the same bytes.
 *
 *  checkpoint_bytes  the blob's size for the open session.
 *  checkpoint        writes the blob into out_host (cap bytes). Legal on an open session that is
 *                    not broken and has done >= 1; the session stays as it was.
 *  resume            _begin_ex's checks, plan and allocation with the flags taken from the blob,
 *                    then the state, the integers and the counters are installed: progress and
 *                    counters run on from the stored values, the times start at zero, and a
 *                    further checkpoint gives the same bytes. These may differ from the exporting
 *                    session's: spp (the new cap, >= done), step_spp, out_layout, post, exposure,
 *                    tuning, and the tile list's order and shape; the SET of pixels must be equal.
 * Refused with IZPI_ERR_INVALID and a message naming what failed, no session left open and the
 * context usable: a short or truncated blob, a bad magic or version, a checksum mismatch, a
 * deciding field that differs, the scene tag, spp < done, a session pixel without a record or a
 * record no session pixel claims, a session already open, cap too small, a broken session,
 * done == 0.
 * The multi forms: a group exports one blob for the frame, byte for byte the one a single
 * context exports at that state (the counters and the integers are the devices' sums); on resume
 * every device installs the pixels of its own share and the first device with a share takes the
 * stored counters, so that the devices' sums run on. */
int izpi_gpu_progressive_checkpoint_bytes(izpi_ctx* ctx, uint64_t* bytes);
int izpi_gpu_progressive_checkpoint(izpi_ctx* ctx, uint64_t scene_tag, void* out_host, uint64_t cap);
int izpi_gpu_progressive_resume(izpi_ctx* ctx, const izpi_render_req* req, uint32_t step_spp, uint64_t scene_tag,
                                const void* blob, uint64_t bytes);
int izpi_gpu_multi_progressive_checkpoint_bytes(izpi_multi* m, uint64_t* bytes);
int izpi_gpu_multi_progressive_checkpoint(izpi_multi* m, uint64_t scene_tag, void* out_host, uint64_t cap);
int izpi_gpu_multi_progressive_resume(izpi_multi* m, const izpi_render_req* req, uint32_t step_spp, uint64_t scene_tag,
                                      const void* blob, uint64_t bytes);

/* Bytes of device output izpi_gpu_render_device writes for `req`. */
uint64_t izpi_gpu_output_bytes(const izpi_render_req* req);

/* Component entry points (parity tests of the path's pieces). All arrays host. */
/* Closest hit through World (HitableSlice{BVH4}); rays are [n][8]: o[3], d[3], tmin, tmax. */
int izpi_gpu_trace(izpi_ctx* ctx, const double* rays, uint32_t n, izpi_hit* out);
/* RayAABB4 masks (bvh4_simd_generic.go:10-52): boxes [n][24] f32 (SoA as BVH4Node),
 * rays [n][7] f32: org[3], invdir[3], tmax. */
int izpi_gpu_ray_aabb4(izpi_ctx* ctx, const float* boxes, const float* rays, uint32_t n, uint8_t* masks);
/* Go-math on device, op codes in izpi_amd/csrc/gomath.h order: 0 sin 1 cos 2 tan 3 exp
 * 4 log 5 pow(x,y) 6 atan2(x,y) 7 asin 8 sqrt 9 div(x,y) 10 atan, 11/12 sin/cos from one
 * shared reduction (x >= 0), 13 the shared-reciprocal vector division (= x / y); 14
 * calculatePathLength's clamped |exit - p| (dielectric.go:141-150) with x the hit points
 * and y the exit points as [n][3]; spectral helpers:
 * 32/33 SampleWavelength(x) lambda/pdf (spectral.go:184-224), 34/35/36 GetCIEValues(x)
 * x/y/z (spectral.go:227-253); 37 SpectralConstant.Value(x) of the uploaded scene's texture
 * number y (spectral_constant.go:65-106, needs a scene). */
int izpi_gpu_gomath(izpi_ctx* ctx, int op, const double* x, const double* y, uint32_t n, double* out);

#ifdef __cplusplus
}
#endif
#endif
