"""What a checkpoint of a progressive session costs, in ONE process: C3
(1024 x 1024, the GPU-built tree, forward accumulation) as an adaptive noise session of 8 steps
of 64 samples with adapt at threshold 0.25 after every step. One warm-up round and then --rounds
rounds; in each, after step --at (default 4) and its adapt:

    export   ProgressiveSession.checkpoint(): host wall time (staging memsets, k_ckpt_gather, the
             copy of the planes to the host, the header and its checksum);
    end, then a plain begin + end of the same shape (wall), as the yardstick a resume contains;
    resume   progressive(..., resume=blob): wall time (the blob's checksum, begin, the copy to the
             device, k_ckpt_scatter, k_ckpt_claimed, the list's rebuild);
    the session then runs to its end.

The yardstick is one 64-sample step of the same session: the library's HIP-event device time
(izpi_render_stats.total_ms) of the step before the export. A plain session (no checkpoint, no
flag) of the same steps is timed beside it per round: it allocates and launches what it did
before this feature, and its device time is the figure tools/noise_probe.py's "plain" row gives.
Written to <out>/checkpoint_c3.json (default profiles/<name>/).

    python tools/checkpoint_probe.py --name r22a

The kernels' own device times come from a run of their own under the profiler, which this tool
only shortens (one round, no warm-up):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/checkpoint_probe.py --name r22a --rounds 1 --warmup 0 --out DIR
"""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, ".")
import izpi_amd
from izpi_amd import configs
from izpi_amd import _native as N
from izpi_amd.renderer import GPURenderer

ap = argparse.ArgumentParser()
ap.add_argument("--name", required=True, help="profiles/<name>/checkpoint_c3.json")
ap.add_argument("--out", default=None, help="directory to write into instead of profiles/<name>")
ap.add_argument("--config", default="C3")
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--step-spp", type=int, default=64)
ap.add_argument("--at", type=int, default=4, help="export after this step")
ap.add_argument("--threshold", type=float, default=0.25)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--no-plain", action="store_true", help="leave the plain session out")
a = ap.parse_args()
cfg = configs.configs()[a.config]
total = a.steps * a.step_spp
r = GPURenderer(cfg.build(), cfg.width, cfg.height, total, max_depth=cfg.max_depth, sampler=cfg.sampler, device=0,
                bvh="gpu", accumulation=N.ACC_FORWARD)
rule = dict(threshold=a.threshold, min_spp=2)


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


rows, plain = [], []
for rnd in range(a.warmup + a.rounds):
    row = {}
    s = r.progressive(a.step_spp, noise=True, adaptive=True)
    before = 0.0
    for k in range(a.at):
        before = s.stats["total_ms"] if s.stats else 0.0
        s.step()
        s.adapt(**rule)
    row["step_device_ms"] = s.stats["total_ms"] - before  # the step before the export
    row["active_at_export"] = s.active
    t0 = time.perf_counter()
    blob = s.checkpoint()
    row["export_wall_ms"] = ms(t0)
    t0 = time.perf_counter()
    again = s.checkpoint()
    row["export_again_wall_ms"] = ms(t0)  # the staging buffer exists by now
    assert again == blob
    s.close()
    t0 = time.perf_counter()
    b = r.progressive(a.step_spp, noise=True, adaptive=True)
    row["begin_wall_ms"] = ms(t0)
    b.close()
    t0 = time.perf_counter()
    s = r.progressive(a.step_spp, resume=blob)
    row["resume_wall_ms"] = ms(t0)
    assert s.checkpoint() == blob
    while s.done < s.total and s.active:
        s.step()
        s.adapt(**rule)
    row["done"], row["active_at_end"], row["blob_bytes"] = s.done, s.active, len(blob)
    s.close()
    if not a.no_plain:
        with r.progressive(a.step_spp) as p:
            while p.done < p.total:
                p.step()
            row["plain_session_device_ms"] = p.stats["total_ms"]
            row["workspace_bytes_plain"] = p.stats["workspace_bytes"]
    print(json.dumps(row), flush=True)
    if rnd >= a.warmup:
        rows.append(row)
r.close()
med = lambda k: statistics.median(x[k] for x in rows) if rows and k in rows[0] else None
info = izpi_amd.checkpoint_info(blob)
out = {"config": a.config, "steps": a.steps, "step_spp": a.step_spp, "at": a.at, "threshold": a.threshold, "rounds": rows,
       "blob_bytes": len(blob), "pixels": info["pixels"],
       "median": {k: med(k) for k in ("step_device_ms", "export_wall_ms", "export_again_wall_ms", "begin_wall_ms",
                                      "resume_wall_ms", "plain_session_device_ms")}}
m = out["median"]
if m["step_device_ms"]:
    out["export_share_of_a_step"] = m["export_again_wall_ms"] / m["step_device_ms"]
    out["resume_less_begin_share_of_a_step"] = (m["resume_wall_ms"] - m["begin_wall_ms"]) / m["step_device_ms"]
d = Path(a.out) if a.out else Path("profiles") / a.name
d.mkdir(parents=True, exist_ok=True)
(d / "checkpoint_c3.json").write_text(json.dumps(out, indent=1) + "\n")
print("IZPI_CHECKPOINT_PROBE", json.dumps({k: v for k, v in out.items() if k != "rounds"}))
