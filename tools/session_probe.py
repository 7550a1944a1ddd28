"""One adaptive progressive session and one one-shot render on C3 (1024 x 1024, the GPU-built
tree, forward accumulation), as one JSON line: the SHA-256 of every snapshot form (CANVAS and
NOISE before the first adapt, all four after two), the integers of both adapt() calls, the
figures of noise() (floats in hex), and the hash of a 16-spp render. Two commits that compute
the same print the same line (profiles/r17a/session_*.json); under

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/session_probe.py

it is the workload that reaches k_resolve in every form, k_noise_resolve, k_noise_stats, the
three adapt kernels and all three instances of k_accumulate in one short run.
"""
import hashlib, json, sys
sys.path.insert(0, ".")
from izpi_amd import configs
from izpi_amd import _native as N
from izpi_amd.renderer import GPURenderer

cfg = configs.configs()["C3"]
r = GPURenderer(cfg.build(), cfg.width, cfg.height, 64, max_depth=cfg.max_depth, sampler=cfg.sampler, device=0,
                bvh="gpu", accumulation=N.ACC_FORWARD)
sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
out = {"sampler": int(cfg.sampler)}
INTS = ("pixels", "nonfinite", "active", "retired", "samples", "done", "converged")
with r.progressive(16, total=64, noise=True, adaptive=True) as s:
    s.step(); s.step()
    out["plain_canvas_32"] = sha(s.snapshot(N.SNAP_CANVAS))
    out["plain_noise_32"] = sha(s.snapshot(N.SNAP_NOISE))
    a = s.adapt(threshold=0.25)
    out["adapt_32"] = {k: int(a[k]) for k in INTS}
    s.step()
    a = s.adapt(threshold=0.25)
    out["adapt_48"] = {k: int(a[k]) for k in INTS}
    s.step()
    for form, name in ((N.SNAP_CANVAS, "canvas"), (N.SNAP_DISPLAY, "display"), (N.SNAP_NOISE, "noise"), (N.SNAP_SAMPLES, "samples")):
        out["snap_" + name] = sha(s.snapshot(form))
    n = s.noise(threshold=0.25)
    out["noise"] = {k: (float(n[k]).hex() if isinstance(n[k], float) else int(n[k])) for k in n if k != "device_ms"}
out["one_shot_16"] = sha(r.render(spp=16))
r.close()
print(json.dumps(out, sort_keys=True))
