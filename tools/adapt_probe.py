"""What adaptive sampling saves, and what it costs, in ONE process and
alternating (settings compared in one process share its shading-time mode):
C3 (1024 x 1024, the GPU-built tree, forward accumulation) with a cap of --cap samples, for
every (--step-spp, --threshold) pair converge's loop, an evaluation at a time, on

    a uniform IZPI_PROG_NOISE session | an IZPI_PROG_ADAPTIVE session

one warm-up round and then --rounds rounds, each running the two in that order. Reported per
form: the median and the spread of the wall time and of the library's HIP-event device time
summed over the steps (the evaluations' own device_ms next to it), the samples rendered, the
final above / active, and per step the pixels it rendered and its device time: the tail of an
adaptive session is a handful of passes per step at the pass floor, and these
figures are what a later change to the step length would start from.

Gate (b), "no retirement, no cost": a session begun adaptive in which adapt is never called
against a plain noise session, --gate-steps steps of --gate-spp samples, alternating likewise;
the difference is to stay within the plain session's own spread.

Written to <out>/adapt_probe.json (default profiles/<name>/).

    python tools/adapt_probe.py --name r14a

The kernels' own times (k_adapt_select, k_adapt_scan, k_adapt_scatter, the scatter instance of
k_accumulate, k_trace2, k_shade) come from a run of their own under the profiler, which this
tool only shortens:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/adapt_probe.py --name r14a --rounds 1 --warmup 0 \\
        --step-spp 16 --threshold 0.25 --no-gate --out DIR
"""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, ".")
from izpi_amd import configs
from izpi_amd import _native as N
from izpi_amd.renderer import GPURenderer

ap = argparse.ArgumentParser()
ap.add_argument("--name", required=True, help="profiles/<name>/adapt_probe.json")
ap.add_argument("--out", default=None, help="directory to write into instead of profiles/<name>")
ap.add_argument("--config", default="C3")
ap.add_argument("--cap", type=int, default=512)
ap.add_argument("--step-spp", type=int, nargs="+", default=[16, 64])
ap.add_argument("--threshold", type=float, nargs="+", default=[N.NOISE_DEFAULT_THRESHOLD, 0.1])
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--gate-steps", type=int, default=8)
ap.add_argument("--gate-spp", type=int, default=64)
ap.add_argument("--no-gate", action="store_true")
a = ap.parse_args()
cfg = configs.configs()[a.config]
r = GPURenderer(cfg.build(), cfg.width, cfg.height, a.cap, max_depth=cfg.max_depth, sampler=cfg.sampler, device=0,
                bvh="gpu", accumulation=N.ACC_FORWARD)


def median_spread(rows, key):
    v = [row[key] for row in rows]
    return {"median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)}


def converge(step_spp, threshold, adaptive):
    """converge's loop (izpi_gpu.h), an evaluation at a time, with each step's figures."""
    p = N.noise_params(threshold=threshold)
    first = max(2, p.min_spp)
    steps, eval_ms = [], 0.0
    t0 = time.perf_counter()
    with r.progressive(step_spp, noise=True, adaptive=adaptive) as s:
        pixels, before, final = cfg.width * cfg.height, 0.0, None
        while s.done < s.total:
            rendering = pixels if s.active is None else s.active
            s.step()
            steps.append({"done": s.done, "rendered_pixels": rendering, "device_ms": round(s.stats["total_ms"] - before, 3),
                          "launches": s.stats["launches"]})
            before = s.stats["total_ms"]
            if s.done < first:
                continue
            final = s.adapt(p) if adaptive else s.noise(p)
            eval_ms += final["device_ms"]
            steps[-1]["active" if adaptive else "above"] = final["active" if adaptive else "above"]
            if final["converged"]:
                break
        st = s.stats
        out = {"device_ms": round(st["total_ms"], 3), "evaluations_device_ms": round(eval_ms, 3), "trace_ms": round(st["kernel_ms"], 3),
               "shade_ms": round(st["shade_ms"], 3), "samples": st["samples"], "rays": st["rays"], "done": s.done,
               "final": None if final is None else {k: final[k] for k in ("pixels", "nonfinite", "active" if adaptive else "above",
                                                                           "converged")},
               "steps": steps}
    out["wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    return out


def gate_session(adaptive):
    t0 = time.perf_counter()
    with r.progressive(a.gate_spp, total=a.gate_steps * a.gate_spp, noise=True, adaptive=adaptive) as s:
        while s.done < s.total:
            s.step()
        st = s.stats
    return {"device_ms": round(st["total_ms"], 3), "wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "rays": st["rays"]}


cases = []
for step_spp in a.step_spp:
    for threshold in a.threshold:
        runs = {"uniform": [], "adaptive": []}
        for rnd in range(a.warmup + a.rounds):
            for name in ("uniform", "adaptive"):
                got = converge(step_spp, threshold, name == "adaptive")
                if rnd >= a.warmup:
                    runs[name].append(got)
                print("probe: step %d threshold %g round %d %s %.1f ms device, %d samples" %
                      (step_spp, threshold, rnd, name, got["device_ms"], got["samples"]), file=sys.stderr, flush=True)
        case = {"step_spp": step_spp, "threshold": threshold}
        for name, rows in runs.items():
            assert len({row["samples"] for row in rows}) == 1  # the same session every round
            case[name] = {"device_ms": median_spread(rows, "device_ms"), "wall_ms": median_spread(rows, "wall_ms"),
                          "evaluations_device_ms": median_spread(rows, "evaluations_device_ms"),
                          "trace_ms": median_spread(rows, "trace_ms"), "shade_ms": median_spread(rows, "shade_ms"),
                          "samples": rows[0]["samples"], "rays": rows[0]["rays"], "done": rows[0]["done"], "final": rows[0]["final"],
                          "steps": rows[len(rows) // 2]["steps"]}
        cases.append(case)

gate = None
if not a.no_gate:
    rows = {"plain": [], "adaptive_never_adapted": []}
    for rnd in range(a.warmup + a.rounds):
        for name in rows:
            got = gate_session(name != "plain")
            if rnd >= a.warmup:
                rows[name].append(got)
    assert len({row["rays"] for v in rows.values() for row in v}) == 1  # no retirement changes no ray
    gate = {"steps": a.gate_steps, "step_spp": a.gate_spp, "runs": rows,
            "device_ms": {k: median_spread(v, "device_ms") for k, v in rows.items()}}
    gate["difference_ms"] = round(gate["device_ms"]["adaptive_never_adapted"]["median"] - gate["device_ms"]["plain"]["median"], 3)
    gate["within_plain_spread"] = abs(gate["difference_ms"]) <= gate["device_ms"]["plain"]["spread"]
r.close()

out = {"config": cfg.name, "width": cfg.width, "height": cfg.height, "cap": a.cap, "bvh": "gpu", "accumulation": "forward",
       "rounds": a.rounds, "cases": cases, "gate_b": gate}
path = Path(a.out) if a.out else Path("profiles") / a.name
path.mkdir(parents=True, exist_ok=True)
(path / "adapt_probe.json").write_text(json.dumps(out, indent=1) + "\n")
print(json.dumps({"cases": [{"step_spp": c["step_spp"], "threshold": c["threshold"],
                             **{n: {"device_ms": c[n]["device_ms"], "wall_ms": c[n]["wall_ms"], "samples": c[n]["samples"],
                                    "done": c[n]["done"], "final": c[n]["final"]} for n in ("uniform", "adaptive")}} for c in cases],
                  "gate_b": None if gate is None else {k: gate[k] for k in ("device_ms", "difference_ms", "within_plain_spread")}}))
