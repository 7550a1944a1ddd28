// izpi_render.cpp — a C++ host for the MI355X path: what `izpi --role standalone`
// (cmd/izpi/main.go, leader/leader.go:37-230) does for one frame, through the C ABI
// only (include/izpi_gpu.h, include/izpi_host.h). No Python, no Go.
//
//   izpi-render --scene cornell.pbtxt [--obj mesh.obj --obj-material White] [--x 1024 --y 1024]
//               [--samples 512] [--depth 50] [--bvh gpu|reference] [--quantized] [--png-pipeline]
//               [--accumulation forward|recursive] [--out image.pfm] [--raw canvas.f64]
//               [--device 0 | --gpus N] [--seed 12345]
//               [--sampler colour|normal|wireframe|albedo|spectral] [--ink r,g,b]
//               [--progressive STEP [--snapshots PREFIX]]
//               [--denoise [N] [--denoise-sigma c,n,a] [--denoise-demodulate]]
//               [--progressive STEP --noise-threshold T [--noise-tolerated F] [--noise-floor L]
//                [--min-samples K] [--noise-out se.pfm] [--adaptive [--samples-out n.pfm]]
//                [--denoise-variance [N] [--denoise-sigma c,n,a] [--variance-floor F] [--variance-out v.pfm]
//                 [--denoise-demodulate]]]
//               [--progressive STEP [--stop-after K] [--checkpoint FILE] [--resume FILE]]
//
// --checkpoint FILE (with --progressive STEP) writes the session's checkpoint (DESIGN.md section
// 3.11, izpi_gpu_progressive_checkpoint) when the run ends, through a temporary file and a rename;
// --stop-after K ends the run after K steps, which is how a job with a time limit renders a part
// of a frame; --resume FILE continues the session FILE holds under this command's scene, size,
// sampler and seed (--samples, the cap, and STEP may be new). The three need --progressive, and
// --noise-threshold / --adaptive must be given as the interrupted run had them. One
//   IZPI_CHECKPOINT read|wrote file= bytes= done=
// line is printed per file. The files a resumed run writes are, byte for byte, those of the
// run that was never interrupted.
//
// --denoise [N] (--sampler colour or spectral) filters the frame with N iterations (default
// IZPI_DENOISE_DEFAULT_ITERATIONS) of the edge-avoiding a-trous denoiser (izpi_gpu_denoise,
// DESIGN.md section 3.8): the frame, a Normal frame and, for the Colour sampler, an Albedo
// frame (the guides at 4 samples) are rendered to host memory and filtered on the device;
// --out / --raw get the filtered canvas. --denoise-sigma sets sigma_colour, sigma_normal
// and sigma_albedo (defaults 1, 0.5, 0.5).
//
// --denoise-demodulate (with --denoise on the Colour sampler, or with --denoise-variance) sets
// IZPI_DENOISE_DEMODULATE: the filter runs on colour / albedo and the
// albedo is multiplied back, which keeps texture detail. The guide frames are then rendered at
// --samples instead of 4: the dividing albedo must come from at least the frame's samples.
// The --denoise message and the IZPI_DENOISE_VAR line then say `demodulated`, and
// --variance-out is the variance of the demodulated canvas.
//
// --progressive STEP renders the frame in steps of STEP samples per pixel (a progressive
// session, izpi_gpu_progressive_*) and --snapshots PREFIX writes PREFIX_<done>.pfm after each
// step; --out / --raw get the last snapshot, byte for byte the files the same command writes
// without --progressive.
//
// --noise-threshold T (with --progressive STEP) stops by the noise estimate's rule (DESIGN.md
// section 3.9, izpi_gpu_progressive_noise): after each step from max(2, --min-samples) samples
// on, the frame statistic is evaluated and printed on stderr as one
//   IZPI_NOISE done= pixels= above= nonfinite= max= mean=
// line, and the render ends when at most --noise-tolerated (a share, default 0.05) of the
// finite pixels have a relative error above T, or at --samples. --out / --raw get the frame
// at the samples spent, byte for byte the file of a render at --samples done; --noise-out
// gets the per-pixel standard errors (IZPI_SNAP_NOISE) as a PFM. --min-samples (default 8)
// guards against the underestimated variance of the first few samples.
//
// --adaptive (with --progressive STEP --noise-threshold T; --sampler colour or spectral) stops
// sampling the pixels whose own relative error is at most T (DESIGN.md section 3.10,
// izpi_gpu_progressive_adapt): each evaluation prints one
//   IZPI_ADAPT done= pixels= active= retired= nonfinite= samples=
// line instead, and the render ends when at most --noise-tolerated of the finite pixels are
// still active. Every pixel of --out is that pixel of a render at its own sample count;
// --samples-out gets the counts (IZPI_SNAP_SAMPLES) as a PFM.
//
// --denoise-variance [N] (with --progressive STEP --noise-threshold T, with or without --adaptive;
// --sampler colour) filters the frame the session ends with by its own noise estimate, with N
// iterations (default 5) of the variance-guided a-trous denoiser (izpi_gpu_denoise_var, DESIGN.md
// section 3.8a): the Normal and Albedo guides (4 samples) are rendered before the session opens,
// the IZPI_SNAP_CANVAS and IZPI_SNAP_NOISE snapshots are filtered on the device, and one
//   IZPI_DENOISE_VAR iterations= sigma_colour= floor= ms=
// line is printed. --out / --raw get the filtered canvas, --variance-out its variance plane as a
// PFM (the value in all three channels). --denoise-sigma is this filter's too (defaults
// IZPI_DENOISE_VAR_DEFAULT_SIGMA_COLOUR, 0.5, 0.5); --variance-floor defaults to
// IZPI_DENOISE_VAR_DEFAULT_FLOOR. A Spectral frame is filtered in XYZ ahead of its
// post-processing, which needs device canvases: through the library, not this tool.
//
// Defaults are the Go shim's: the GPU-built tree and the forward accumulation
// (IZPI_ACC_FORWARD; --accumulation recursive is bit-identical to the CPU oracle).
// --quantized uploads the tree with 64-B quantised nodes (IZPI_SCENE_QUANTIZED_BVH).
//
// The scene file is read as leader.go:54-75 does (.pbtxt text, .izpi binary); a SPECTRAL
// scene renders with the spectral sampler and Render's post-processing (leader.go:77-81,
// renderer.go:215-219); --sampler picks another of render.New's five (sampler.go:22-28;
// wireframe draws edges in --ink, default black, on a black paper). --obj streams a Wavefront mesh into the scene with the
// transforms of scenes/spectral.go:644-646. The canvas is written as a PFM (float32 RGB,
// bottom row first) and/or the raw W*H*4 float64 canvas.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/izpi_gpu.h"
#include "../../include/izpi_host.h"

namespace {

bool read_file(const std::string& path, std::vector<char>& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

[[noreturn]] void die(const std::string& m) {
  fprintf(stderr, "izpi-render: %s\n", m.c_str());
  exit(1);
}

std::string dir_of(const std::string& p) {
  const size_t k = p.find_last_of('/');
  return k == std::string::npos ? "." : p.substr(0, k);
}

// -(60 * math.Pi / 180) as Go evaluates the constant expression: pi/3 rounded once
constexpr double kMinus60Deg = -0x1.0c152382d7366p+0;  // == -ingest.go_radians(60) (test_ingest.py)

// PFM: "PF", W H, -1 (little endian), rows bottom to top
void write_pfm(const std::string& path, const std::vector<double>& canvas, uint32_t W, uint32_t H) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) die("cannot write " + path);
  fprintf(f, "PF\n%u %u\n-1.0\n", W, H);
  std::vector<float> row(3 * (size_t)W);
  for (uint32_t y = H; y-- > 0;) {
    for (uint32_t x = 0; x < W; x++)
      for (int c = 0; c < 3; c++) row[3 * x + c] = (float)canvas[((size_t)y * W + x) * 4 + c];
    fwrite(row.data(), sizeof(float), row.size(), f);
  }
  fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  std::string scene_path, obj_path, obj_material = "White", out_pfm, out_raw, bvh = "gpu", acc = "forward", sampler_name, snap_prefix;
  uint32_t progressive = 0;
  bool denoise = false;
  izpi_denoise_params dparams = {IZPI_DENOISE_DEFAULT_ITERATIONS, 0, IZPI_DENOISE_DEFAULT_SIGMA_COLOUR,
                                 IZPI_DENOISE_DEFAULT_SIGMA_NORMAL, IZPI_DENOISE_DEFAULT_SIGMA_ALBEDO};
  bool dvar = false, sigma_given = false, demodulate = false;
  uint32_t dvar_iterations = IZPI_DENOISE_DEFAULT_ITERATIONS;
  double variance_floor = IZPI_DENOISE_VAR_DEFAULT_FLOOR;
  std::string variance_out;
  bool noise = false;
  izpi_noise_params nparams = {IZPI_NOISE_DEFAULT_THRESHOLD, IZPI_NOISE_DEFAULT_FLOOR, IZPI_NOISE_DEFAULT_TOLERATED,
                               IZPI_NOISE_DEFAULT_MIN_SPP, 0};
  std::string noise_out, samples_out;
  bool adaptive = false;
  double ink[3] = {0.0, 0.0, 0.0};
  std::string ckpt_out, ckpt_in;
  uint32_t stop_after = 0;
  bool quantized = false;
  uint32_t W = 1024, H = 1024, spp = 16, depth = 50, device = 0, gpus = 1;
  uint64_t seed = 12345;
  bool png = false;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto val = [&]() -> std::string { if (i + 1 >= argc) die("missing value for " + a); return argv[++i]; };
    if (a == "--scene") scene_path = val();
    else if (a == "--obj") obj_path = val();
    else if (a == "--obj-material") obj_material = val();
    else if (a == "--x") W = (uint32_t)atoi(val().c_str());
    else if (a == "--y") H = (uint32_t)atoi(val().c_str());
    else if (a == "--samples") spp = (uint32_t)atoi(val().c_str());
    else if (a == "--depth") depth = (uint32_t)atoi(val().c_str());
    else if (a == "--bvh") bvh = val();
    else if (a == "--quantized") quantized = true;
    else if (a == "--accumulation") acc = val();
    else if (a == "--png-pipeline") png = true;
    else if (a == "--out") out_pfm = val();
    else if (a == "--raw") out_raw = val();
    else if (a == "--device") device = (uint32_t)atoi(val().c_str());
    else if (a == "--gpus") gpus = (uint32_t)atoi(val().c_str());
    else if (a == "--seed") seed = strtoull(val().c_str(), nullptr, 10);
    else if (a == "--sampler") sampler_name = val();
    else if (a == "--progressive") { progressive = (uint32_t)atoi(val().c_str()); if (!progressive) die("--progressive takes a step of at least 1 sample"); }
    else if (a == "--snapshots") snap_prefix = val();
    else if (a == "--denoise") {
      denoise = true;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') dparams.iterations = (uint32_t)atoi(argv[++i]);
    }
    else if (a == "--denoise-sigma") {
      if (sscanf(val().c_str(), "%lf,%lf,%lf", &dparams.sigma_colour, &dparams.sigma_normal, &dparams.sigma_albedo) != 3)
        die("--denoise-sigma takes colour,normal,albedo");
      sigma_given = true;
    }
    else if (a == "--denoise-variance") {
      dvar = true;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') dvar_iterations = (uint32_t)atoi(argv[++i]);
    }
    else if (a == "--denoise-demodulate") demodulate = true;
    else if (a == "--variance-floor") variance_floor = atof(val().c_str());
    else if (a == "--variance-out") variance_out = val();
    else if (a == "--noise-threshold") { noise = true; nparams.threshold = atof(val().c_str()); }
    else if (a == "--noise-tolerated") nparams.tolerated = atof(val().c_str());
    else if (a == "--noise-floor") nparams.floor = atof(val().c_str());
    else if (a == "--min-samples") nparams.min_spp = (uint32_t)atoi(val().c_str());
    else if (a == "--noise-out") noise_out = val();
    else if (a == "--adaptive") adaptive = true;
    else if (a == "--samples-out") samples_out = val();
    else if (a == "--checkpoint") ckpt_out = val();
    else if (a == "--resume") ckpt_in = val();
    else if (a == "--stop-after") { stop_after = (uint32_t)atoi(val().c_str()); if (!stop_after) die("--stop-after takes at least 1 step"); }
    else if (a == "--ink") { if (sscanf(val().c_str(), "%lf,%lf,%lf", &ink[0], &ink[1], &ink[2]) != 3) die("--ink takes r,g,b"); }
    else die("unknown option " + a);
  }
  if (scene_path.empty()) die("--scene is required");
  if (bvh != "gpu" && bvh != "reference") die("--bvh must be gpu or reference");
  if (acc != "forward" && acc != "recursive") die("--accumulation must be forward or recursive");
  if (!snap_prefix.empty() && !progressive) die("--snapshots needs --progressive");
  if (noise && !progressive) die("--noise-threshold needs --progressive");
  if (!ckpt_out.empty() && !progressive) die("--checkpoint needs --progressive");
  if (!ckpt_in.empty() && !progressive) die("--resume needs --progressive");
  if (stop_after && !progressive) die("--stop-after needs --progressive");
  if (!noise_out.empty() && !noise) die("--noise-out needs --noise-threshold");
  if (adaptive && !noise) die("--adaptive needs --progressive and --noise-threshold");
  if (!samples_out.empty() && !adaptive) die("--samples-out needs --adaptive");
  if (dvar && !noise) die("--denoise-variance needs --progressive and --noise-threshold");
  if (dvar && denoise) die("--denoise-variance and --denoise are two filters: name one");
  if (!variance_out.empty() && !dvar) die("--variance-out needs --denoise-variance");
  if (demodulate && !denoise && !dvar) die("--denoise-demodulate needs --denoise or --denoise-variance");
  if (demodulate) dparams.flags |= IZPI_DENOISE_DEMODULATE;
  if (dvar) {
    dparams.iterations = dvar_iterations;
    if (!sigma_given) dparams.sigma_colour = IZPI_DENOISE_VAR_DEFAULT_SIGMA_COLOUR;
  }
  // ---- scene file (leader.go:54-75)
  std::vector<char> text;
  if (!read_file(scene_path, text)) die("cannot read " + scene_path);
  izpi_proto_scene* ps = nullptr;
  const std::string ext = scene_path.size() > 5 ? scene_path.substr(scene_path.size() - 5) : "";
  int rc;
  if (ext == "pbtxt") rc = izpi_scene_parse_text(text.data(), text.size(), &ps);
  else if (ext == ".izpi") rc = izpi_scene_parse_binary(text.data(), text.size(), &ps);
  else die("Unknown scene file extension: " + scene_path);
  if (rc) die(izpi_host_last_error());
  izpi_proto_info info;
  izpi_scene_info(ps, &info);
  if (info.num_image_textures) die("image textures need a host-side decoder (not part of this tool)");
  // ---- optional streamed mesh (scenes/spectral.go:639-657)
  if (!obj_path.empty()) {
    std::vector<char> obj;
    if (!read_file(obj_path, obj)) die("cannot read " + obj_path);
    izpi_obj* mesh = nullptr;
    if (izpi_obj_parse(obj.data(), obj.size(), dir_of(obj_path).c_str(), 0, &mesh)) die(izpi_host_last_error());
    izpi_obj_scale(mesh, 90.0, 90.0, 90.0);
    izpi_obj_rotate(mesh, 0.0, kMinus60Deg, 0.0);
    izpi_obj_translate(mesh, 50.0, 25.1, 60.0);
    izpi_obj_info oi;
    izpi_obj_info_get(mesh, &oi);
    for (uint32_t g = 0; g < oi.num_groups; g++) {
      uint64_t n = 0;
      if (izpi_obj_group_to_triangles(mesh, g, 1, nullptr, 0, &n)) die(izpi_host_last_error());
      std::vector<izpi_tri_in> tris(n);
      if (n && izpi_obj_group_to_triangles(mesh, g, 1, tris.data(), n, &n)) die(izpi_host_last_error());
      if (n && izpi_scene_add_triangles(ps, tris.data(), n, obj_material.c_str())) die(izpi_host_last_error());
    }
    izpi_obj_free(mesh);
  }
  // the sampler: the scene file's colour representation (leader.go:77-81) unless --sampler names one (sampler.go:22-28)
  uint32_t sampler = info.colour_representation == IZPI_COLOUR_SPECTRAL ? IZPI_SAMPLER_SPECTRAL : IZPI_SAMPLER_COLOUR;
  if (sampler_name == "colour") sampler = IZPI_SAMPLER_COLOUR;
  else if (sampler_name == "normal") sampler = IZPI_SAMPLER_NORMAL;
  else if (sampler_name == "wireframe") sampler = IZPI_SAMPLER_WIREFRAME;
  else if (sampler_name == "albedo") sampler = IZPI_SAMPLER_ALBEDO;
  else if (sampler_name == "spectral") sampler = IZPI_SAMPLER_SPECTRAL;
  else if (!sampler_name.empty()) die("--sampler must be colour, normal, wireframe, albedo or spectral");
  else sampler_name = sampler == IZPI_SAMPLER_SPECTRAL ? "spectral" : "colour";
  const bool spectral = sampler == IZPI_SAMPLER_SPECTRAL;
  if (denoise && sampler != IZPI_SAMPLER_COLOUR && !spectral) die("--denoise needs --sampler colour or spectral");
  if (denoise && demodulate && spectral) die("--denoise-demodulate needs --sampler colour: a spectral frame has no albedo guide");
  if (denoise && progressive) die("--denoise filters a whole frame: not with --progressive");
  if (denoise && png) die("--denoise filters linear values: not with --png-pipeline");
  if (adaptive && sampler != IZPI_SAMPLER_COLOUR && !spectral) die("--adaptive needs --sampler colour or spectral");
  if (dvar && sampler != IZPI_SAMPLER_COLOUR) die("--denoise-variance needs --sampler colour");
  if (dvar && png) die("--denoise-variance filters linear values: not with --png-pipeline");
  // ---- transport.ToScene, BVH, upload
  auto t0 = std::chrono::steady_clock::now();
  const izpi_scene_input* in = nullptr;
  if (izpi_scene_to_input(ps, (double)W / H, 12345, &in)) die(izpi_host_last_error());
  izpi_host_scene* host = nullptr;
  if (izpi_host_build_scene_ex(in, bvh == "gpu" ? IZPI_HOST_SKIP_BVH : 0u, &host)) die(izpi_host_last_error());
  // --gpus N: one Render fans out over GPUs 0..N-1 (izpi_gpu_multi_*, renderer.go:123-147)
  izpi_ctx* ctx = nullptr;
  izpi_multi* multi = nullptr;
  if (gpus > 1) {
    std::vector<int> devs(gpus);
    for (uint32_t i = 0; i < gpus; i++) devs[i] = (int)i;
    if (izpi_gpu_multi_open(devs.data(), gpus, &multi)) die("izpi_gpu_multi_open failed (fewer GPUs?)");
    ctx = izpi_gpu_multi_context(multi, 0);
  } else if (izpi_gpu_open((int)device, &ctx)) {
    die("izpi_gpu_open failed (no HIP device?)");
  }
  const izpi_scene_desc* desc = izpi_host_scene_desc(host);
  if (bvh == "gpu") {
    const uint32_t n = desc->num_tris + desc->num_spheres;
    std::vector<double> boxes(6 * (size_t)n);
    std::vector<izpi_bvh4_node> nodes(2 * (size_t)n + 1);
    std::vector<uint32_t> order(n + 1);
    uint32_t num_nodes = 0;
    double ms = 0;
    if (n) {
      izpi_host_scene_prim_boxes(host, boxes.data());
      if (izpi_gpu_build_bvh4(ctx, boxes.data(), n, izpi_host_bvh_leaf_max(desc), IZPI_BVH_PLOC | IZPI_BVH_SAH, nodes.data(), (uint32_t)nodes.size(), &num_nodes,
                              order.data(), &ms))
        die(izpi_gpu_last_error(ctx));
      if (izpi_host_scene_set_bvh(host, nodes.data(), num_nodes, order.data())) die(izpi_host_last_error());
      if (quantized && izpi_host_scene_set_flags(host, IZPI_SCENE_QUANTIZED_BVH)) die(izpi_host_last_error());
    }
    fprintf(stderr, "izpi-render: GPU BVH4 of %u primitives, %u nodes, %.1f ms\n", n, num_nodes, ms);
  }
  if (multi ? izpi_gpu_multi_upload_scene(multi, izpi_host_scene_desc(host)) : izpi_gpu_upload_scene(ctx, izpi_host_scene_desc(host)))
    die(multi ? izpi_gpu_multi_last_error(multi) : izpi_gpu_last_error(ctx));
  const double setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  // ---- Render (renderer.go:108-222)
  izpi_render_req req;
  memset(&req, 0, sizeof req);
  req.abi_version = IZPI_ABI_VERSION;
  req.width = W; req.height = H; req.spp = spp; req.max_depth = depth;
  req.sampler = sampler;
  for (int k = 0; k < 3; k++) req.ink[k] = ink[k];
  req.out_layout = IZPI_OUT_CANVAS;
  req.seed = seed;
  req.exposure = izpi_host_scene_desc(host)->camera.exposure;
  req.post = (spectral ? IZPI_POST_SPECTRAL : IZPI_POST_NONE) | (png ? IZPI_POST_GAMMA_CLAMP : 0u);
  req.accumulation = acc == "forward" ? IZPI_ACC_FORWARD : IZPI_ACC_RECURSIVE;
  std::vector<double> canvas((size_t)W * H * 4);
  std::vector<izpi_render_stats> stv(gpus > 1 ? gpus : 1);
  uint32_t spent = spp;  // samples per pixel in the canvas (fewer when the noise rule stopped the render)
  uint64_t rendered = 0;  // --adaptive: the samples rendered, the sum of the pixels' own counts
  auto t1 = std::chrono::steady_clock::now();
  // The Normal or Albedo guide of a filter: it shares the frame's primary rays (same seed, same streams).
  auto guide = [&](uint32_t which, std::vector<double>& into) {
    std::vector<izpi_render_stats> gst(stv.size());
    izpi_render_req g = req;
    g.post = IZPI_POST_NONE;
    g.spp = demodulate ? spp : 4;  // render_denoised's aov_spp
    g.sampler = which;
    into.resize(canvas.size());
    if (multi ? izpi_gpu_multi_render(multi, &g, into.data(), gst.data()) : izpi_gpu_render(ctx, &g, into.data(), gst.data()))
      die(multi ? izpi_gpu_multi_last_error(multi) : izpi_gpu_last_error(ctx));
  };
  // --denoise-variance: renders are refused while a session is open, so the guides come first.
  // dv_se: the standard errors of the frame the session ends with.
  std::vector<double> dv_normal, dv_albedo, dv_se;
  if (dvar) {
    guide(IZPI_SAMPLER_NORMAL, dv_normal);
    guide(IZPI_SAMPLER_ALBEDO, dv_albedo);
  }
  if (progressive) {
    // the frame in steps; a snapshot after each (the last one is the frame)
    auto ok = [&](int r) { if (r) die(multi ? izpi_gpu_multi_last_error(multi) : izpi_gpu_last_error(ctx)); };
    const uint32_t flags = (noise ? (uint32_t)IZPI_PROG_NOISE : 0u) | (adaptive ? (uint32_t)IZPI_PROG_ADAPTIVE : 0u);
    uint64_t scene_tag = 0;
    if (izpi_host_scene_tag(izpi_host_scene_desc(host), &scene_tag)) die(izpi_host_last_error());
    uint32_t done0 = 0;
    if (!ckpt_in.empty()) {  // continue the session the file holds
      std::vector<char> blob;
      if (!read_file(ckpt_in, blob)) die("cannot read " + ckpt_in);
      uint64_t bflags = 0, bdone = 0;
      if (izpi_host_checkpoint_field(blob.data(), blob.size(), IZPI_CKPT_FLAGS, &bflags) ||
          izpi_host_checkpoint_field(blob.data(), blob.size(), IZPI_CKPT_DONE, &bdone))
        die(izpi_host_last_error());
      if (bflags != flags) die("--resume: the checkpoint's session was begun with other --noise-threshold / --adaptive options");
      ok(multi ? izpi_gpu_multi_progressive_resume(multi, &req, progressive, scene_tag, blob.data(), blob.size())
               : izpi_gpu_progressive_resume(ctx, &req, progressive, scene_tag, blob.data(), blob.size()));
      done0 = (uint32_t)bdone;
      fprintf(stderr, "IZPI_CHECKPOINT read file=%s bytes=%llu done=%u\n", ckpt_in.c_str(), (unsigned long long)blob.size(), done0);
    } else {
      ok(multi ? izpi_gpu_multi_progressive_begin_ex(multi, &req, progressive, flags) : izpi_gpu_progressive_begin_ex(ctx, &req, progressive, flags));
    }
    bool stop = false;
    uint32_t steps = 0, last_done = done0;
    for (uint32_t done = done0; done < spp && !stop;) {
      ok(multi ? izpi_gpu_multi_progressive_step(multi, 0, stv.data()) : izpi_gpu_progressive_step(ctx, 0, stv.data()));
      done = done + progressive < spp ? done + progressive : spp;
      last_done = done;
      const bool interrupted = stop_after && ++steps >= stop_after;  // --stop-after: the run ends here, the frame as it stands
      if (adaptive && done >= (nparams.min_spp > 2 ? nparams.min_spp : 2u)) {  // ... and its rule on an adaptive session
        izpi_adapt_stats as;
        ok(multi ? izpi_gpu_multi_progressive_adapt(multi, &nparams, &as) : izpi_gpu_progressive_adapt(ctx, &nparams, &as));
        fprintf(stderr, "IZPI_ADAPT done=%u pixels=%llu active=%llu retired=%llu nonfinite=%llu samples=%llu\n", as.done,
                (unsigned long long)as.pixels, (unsigned long long)as.active, (unsigned long long)as.retired,
                (unsigned long long)as.nonfinite, (unsigned long long)as.samples);
        stop = as.converged != 0;
        rendered = as.samples;
      } else if (noise && done >= (nparams.min_spp > 2 ? nparams.min_spp : 2u)) {  // izpi_gpu_progressive_converge's rule, an evaluation at a time
        izpi_noise_stats ns;
        ok(multi ? izpi_gpu_multi_progressive_noise(multi, &nparams, &ns) : izpi_gpu_progressive_noise(ctx, &nparams, &ns));
        const uint64_t fin = ns.pixels - ns.nonfinite;
        fprintf(stderr, "IZPI_NOISE done=%u pixels=%llu above=%llu nonfinite=%llu max=%.6g mean=%.6g\n", ns.done,
                (unsigned long long)ns.pixels, (unsigned long long)ns.above, (unsigned long long)ns.nonfinite, ns.max_error,
                fin ? ns.sum_error / (double)fin : 0.0);
        stop = ns.converged != 0;
      }
      if (stop || done == spp || interrupted) {
        spent = done;
        if (!noise_out.empty() && done >= 2) {
          std::vector<double> se((size_t)W * H * 4);
          ok(multi ? izpi_gpu_multi_progressive_snapshot(multi, IZPI_SNAP_NOISE, se.data())
                   : izpi_gpu_progressive_snapshot(ctx, IZPI_SNAP_NOISE, se.data()));
          write_pfm(noise_out, se, W, H);
        }
        if (dvar) {
          if (done < 2) die("--denoise-variance needs a frame of at least 2 samples");
          dv_se.resize(canvas.size());
          ok(multi ? izpi_gpu_multi_progressive_snapshot(multi, IZPI_SNAP_NOISE, dv_se.data())
                   : izpi_gpu_progressive_snapshot(ctx, IZPI_SNAP_NOISE, dv_se.data()));
        }
        if (!samples_out.empty()) {  // the sample-count map
          std::vector<double> map((size_t)W * H * 4);
          ok(multi ? izpi_gpu_multi_progressive_snapshot(multi, IZPI_SNAP_SAMPLES, map.data())
                   : izpi_gpu_progressive_snapshot(ctx, IZPI_SNAP_SAMPLES, map.data()));
          write_pfm(samples_out, map, W, H);
        }
      }
      if (snap_prefix.empty() && done < spp && !stop && !interrupted) continue;
      ok(multi ? izpi_gpu_multi_progressive_snapshot(multi, IZPI_SNAP_CANVAS, canvas.data())
               : izpi_gpu_progressive_snapshot(ctx, IZPI_SNAP_CANVAS, canvas.data()));
      if (!snap_prefix.empty()) write_pfm(snap_prefix + "_" + std::to_string(done) + ".pfm", canvas, W, H);
      if (interrupted) break;
    }
    if (!ckpt_out.empty()) {  // the session as the run leaves it, through a temporary file and a rename
      uint64_t n = 0;
      ok(multi ? izpi_gpu_multi_progressive_checkpoint_bytes(multi, &n) : izpi_gpu_progressive_checkpoint_bytes(ctx, &n));
      std::vector<char> blob(n);
      ok(multi ? izpi_gpu_multi_progressive_checkpoint(multi, scene_tag, blob.data(), n) : izpi_gpu_progressive_checkpoint(ctx, scene_tag, blob.data(), n));
      const std::string tmp = ckpt_out + ".tmp";
      FILE* f = fopen(tmp.c_str(), "wb");
      if (!f || fwrite(blob.data(), 1, blob.size(), f) != blob.size() || fclose(f) != 0 || rename(tmp.c_str(), ckpt_out.c_str()) != 0)
        die("cannot write " + ckpt_out);
      fprintf(stderr, "IZPI_CHECKPOINT wrote file=%s bytes=%llu done=%u\n", ckpt_out.c_str(), (unsigned long long)n, last_done);
    }
    ok(multi ? izpi_gpu_multi_progressive_end(multi) : izpi_gpu_progressive_end(ctx));
  } else if (multi) {
    if (izpi_gpu_multi_render(multi, &req, canvas.data(), stv.data())) die(izpi_gpu_multi_last_error(multi));
  } else if (izpi_gpu_render(ctx, &req, canvas.data(), stv.data())) {
    die(izpi_gpu_last_error(ctx));
  }
  if (dvar) {  // (after a multi-GPU gather: on device 0's context, over the gathered snapshots)
    std::vector<double> filtered(canvas.size()), plane((size_t)W * H);
    double ms = 0;
    if (izpi_gpu_denoise_var(ctx, canvas.data(), dv_se.data(), dv_normal.data(), dv_albedo.data(), filtered.data(),
                             plane.data(), W, H, &dparams, variance_floor, &ms))
      die(izpi_gpu_last_error(ctx));
    canvas.swap(filtered);
    fprintf(stderr, "IZPI_DENOISE_VAR iterations=%u sigma_colour=%.6g floor=%.6g ms=%.3f%s\n", dparams.iterations,
            dparams.sigma_colour, variance_floor, ms, demodulate ? " demodulated" : "");
    if (!variance_out.empty()) {
      std::vector<double> v4(canvas.size());
      for (size_t q = 0; q < plane.size(); q++) v4[4 * q] = v4[4 * q + 1] = v4[4 * q + 2] = plane[q];
      write_pfm(variance_out, v4, W, H);
    }
  }
  if (denoise) {
    // the guides, then the filter
    std::vector<double> normal, albedo, filtered(canvas.size());
    guide(IZPI_SAMPLER_NORMAL, normal);
    if (!spectral) guide(IZPI_SAMPLER_ALBEDO, albedo);
    double ms = 0;
    if (izpi_gpu_denoise(ctx, canvas.data(), normal.data(), spectral ? nullptr : albedo.data(), filtered.data(), W, H,
                         &dparams, &ms))
      die(izpi_gpu_last_error(ctx));
    canvas.swap(filtered);
    fprintf(stderr, "izpi-render: denoised%s, %u iterations, %.3f ms on the device\n", demodulate ? " (demodulated)" : "",
            dparams.iterations, ms);
  }
  izpi_render_stats st = stv[0];
  for (size_t i = 1; i < stv.size(); i++) { st.rays += stv[i].rays; st.node_visits += stv[i].node_visits; }
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  printf("{\"scene\": \"%s\", \"width\": %u, \"height\": %u, \"spp\": %u, \"bvh\": \"%s\", \"quantized\": %d, \"accumulation\": \"%s\", \"sampler\": \"%s\", \"gpus\": %u, "
         "\"setup_s\": %.3f, \"render_s\": %.4f, \"msamples_per_s\": %.2f, \"rays\": %llu, \"node_visits\": %llu}\n",
         scene_path.c_str(), W, H, spent, bvh.c_str(), bvh == "gpu" && quantized ? 1 : 0, acc.c_str(), sampler_name.c_str(), gpus > 1 ? gpus : 1u, setup_s, secs,
         (rendered ? (double)rendered : (double)W * H * spent) / secs / 1e6, (unsigned long long)st.rays, (unsigned long long)st.node_visits);
  // ---- outputs
  if (!out_raw.empty()) {
    FILE* f = fopen(out_raw.c_str(), "wb");
    if (!f || fwrite(canvas.data(), sizeof(double), canvas.size(), f) != canvas.size()) die("cannot write " + out_raw);
    fclose(f);
  }
  if (!out_pfm.empty()) write_pfm(out_pfm, canvas, W, H);
  if (multi) izpi_gpu_multi_close(multi);
  else izpi_gpu_close(ctx);
  izpi_host_scene_free(host);
  izpi_scene_free(ps);
  return 0;
}
