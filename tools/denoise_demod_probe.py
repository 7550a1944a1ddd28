#!/usr/bin/env python3
"""Time albedo demodulation on both denoisers.

C3 (the Cornell box with the dragon) at 1024 x 1024 on the GPU-built tree, one process and one
context: the Normal and Albedo guides at the session's cap (a demodulating guide wants the
frame's samples), then a noise session of --steps steps of --step-spp samples, whose CANVAS and
NOISE snapshots go into device canvases. Then izpi_gpu_denoise_device and
izpi_gpu_denoise_var_device, each at its defaults with and without IZPI_DENOISE_DEMODULATE,
alternate: one warm-up call and --runs timed calls each (HIP-event time over the launches of a
call, k_demodulate and k_remodulate included). The figure to read is each flagged median over
its unflagged twin's of this one run: times of different boxes, or of different processes, do
not compare. Nothing is judged: the two added passes have no predecessor.

    python tools/denoise_demod_probe.py --out profiles/<round>/denoise_demod_probe.json
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from izpi_amd import _native as N  # noqa: E402
from izpi_amd import configs  # noqa: E402
from izpi_amd.renderer import GPURenderer, denoise_var_device  # noqa: E402


def spread(values):
    v = sorted(values)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4), "runs": len(v)}


def frames(a):
    """(renderer, {name: device canvas}): the guides, then the session's two snapshots."""
    import torch
    cfg = configs.configs()[a.config]
    cap = a.steps * a.step_spp
    r = GPURenderer(cfg.build(), a.size, a.size, cap, max_depth=cfg.max_depth, sampler=N.SAMPLER_COLOUR,
                    device=a.device, bvh="gpu", accumulation=N.ACC_FORWARD)
    dev = torch.device("cuda", a.device)
    shape = (a.size, a.size, 4)
    t = {name: torch.zeros(shape, dtype=torch.float64, device=dev) for name in ("colour", "stderr", "out")}
    t["variance"] = torch.zeros(shape[:2], dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    t["normal"], t["albedo"] = r.render_guides(cap)
    with r.progressive(a.step_spp, noise=True) as s:
        for _ in range(a.steps):
            s.step()
        s.snapshot_device(t["colour"].data_ptr(), N.SNAP_CANVAS)
        s.snapshot_device(t["stderr"].data_ptr(), N.SNAP_NOISE)
    return r, t


def fixed(r, t, flag):
    return r.denoise_device(t["colour"].data_ptr(), t["normal"].data_ptr(), t["albedo"].data_ptr(), t["out"].data_ptr(),
                            N.denoise_params(demodulate=flag))


def guided(r, t, flag):
    return denoise_var_device(r.ctx, t["colour"].data_ptr(), t["stderr"].data_ptr(), t["normal"].data_ptr(),
                              t["albedo"].data_ptr(), t["out"].data_ptr(), t["variance"].data_ptr(), r.width, r.height,
                              N.denoise_var_params(demodulate=flag))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--step-spp", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("denoise_demod_probe: no HIP device (this measurement needs the GPU)")
    r, t = frames(a)
    calls = [("denoise_device", fixed, False), ("denoise_device_demodulated", fixed, True),
             ("denoise_var_device", guided, False), ("denoise_var_device_demodulated", guided, True)]
    times = {name: [] for name, _, _ in calls}
    outputs = {}
    for run in range(a.runs + 1):  # (the first round is the warm-up)
        for name, call, flag in calls:
            ms = call(r, t, flag)
            if run:
                times[name].append(ms)
            else:
                outputs[name] = t["out"].cpu().numpy()
    colour = t["colour"].cpu().numpy()
    live = colour[..., 3] != 0
    for name, out in outputs.items():
        if not (out[..., 3] == colour[..., 3]).all() or not (out[live] == out[live]).all() or (out[live] == colour[live]).all():
            raise SystemExit("denoise_demod_probe: %s's output is not a filtered copy of the frame" % name)
    for plain in ("denoise_device", "denoise_var_device"):
        if (outputs[plain] == outputs[plain + "_demodulated"]).all():
            raise SystemExit("denoise_demod_probe: the flag changed nothing in %s" % plain)
    r.close()

    res = {"config": a.config, "width": a.size, "height": a.size, "session": "%d x %d spp" % (a.steps, a.step_spp),
           "guide_spp": a.steps * a.step_spp, "live_pixels": int(live.sum()), "iterations": N.DENOISE_DEFAULT_ITERATIONS}
    for name in times:
        res[name + "_ms"] = spread(times[name])
    for plain in ("denoise_device", "denoise_var_device"):
        res[plain + "_flagged_over_unflagged"] = round(res[plain + "_demodulated_ms"]["median"] / res[plain + "_ms"]["median"], 4)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
