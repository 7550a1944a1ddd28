#!/usr/bin/env python3
"""Time the DISPLACE operator on a mesh of a size users render.

Input: a grid plane of about half a million source triangles (uv = position) over a
1025 x 1025 smooth height map. Measured, each several times after a warm-up:
  * izpi_gpu_displace: device time of the call (HIP events) and wall time with the copy back,
    in mesh order and in per-triangle order;
  * izpi_host_displace, the sequential twin, on one thread of the same box;
  * izpi_gpu_build_bvh4 over the displaced triangles.
The device result is compared with the host twin's byte for byte before any time is reported.

    python tools/displace_probe.py [--quads 500] [--map 1025] [--range 8] [--runs 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from izpi_amd import _native as N  # noqa: E402
from izpi_amd import ingest  # noqa: E402
from izpi_amd.renderer import build_bvh4, gpu_leaf_max  # noqa: E402
from izpi_amd.scene import TRI_DTYPE, HostScene, Scene  # noqa: E402


def smooth_map(res):
    y, x = np.mgrid[0:res, 0:res].astype(np.float64)
    rgba = np.zeros((res, res, 4))
    rgba[..., 0], rgba[..., 1], rgba[..., 3] = 0.1, 0.9, 1.0
    rgba[..., 2] = 0.5 + 0.25 * np.sin(0.37 * x) + 0.25 * np.cos(0.23 * y + 0.11 * x)
    return rgba


def grid_plane(quads):
    """2 * quads^2 triangles over the unit square of the XZ plane, uv = position."""
    j, i = np.mgrid[0:quads, 0:quads]
    x0, x1 = (i / quads).ravel(), ((i + 1) / quads).ravel()
    z0, z1 = (j / quads).ravel(), ((j + 1) / quads).ravel()
    t = np.zeros((quads * quads, 2), TRI_DTYPE)
    zero = np.zeros_like(x0)
    for k, (a, b, c) in enumerate((((x0, z0), (x1, z0), (x1, z1)), ((x0, z0), (x1, z1), (x0, z1)))):
        for name, (x, z) in (("v0", a), ("v1", b), ("v2", c)):
            t[name][:, k] = np.stack([x, zero, z], axis=1)
        t["uv"][:, k] = np.stack([a[0], a[1], b[0], b[1], c[0], c[1]], axis=1)
    return t.reshape(-1)


def spread(values):
    v = sorted(values)
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1], "runs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--map", type=int, default=1025)
    ap.add_argument("--range", type=float, default=8.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    tris, rgba = grid_plane(a.quads), smooth_map(a.map)
    L = N.lib()
    ctx = C.c_void_p()
    if L.izpi_gpu_open(a.device, C.byref(ctx)) != 0:
        raise SystemExit("displace_probe: izpi_gpu_open failed (this measurement needs the GPU)")

    res = {"source_triangles": len(tris), "map": [a.map, a.map], "dmin": -a.range, "dmax": a.range}
    _, counts = ingest.displace(tris, rgba, -a.range, a.range, N.DISPLACE_MESH, count_only=True)
    total = int(counts.sum())
    res["output_triangles"] = total
    res["outputs_per_source"] = {"min": int(counts.min()), "max": int(counts.max())}
    # a source that went k levels deep yields at most 4^k triangles
    res["levels"] = int(np.ceil(np.log(counts.max()) / np.log(4.0)))

    def call(fn, order, out, *head):
        """One call into a preallocated output: (wall ms, the entry's own ms)."""
        n, ms = C.c_uint64(), C.c_double()
        got = np.zeros(len(tris), np.uint64)
        t0 = time.perf_counter()
        rc = fn(*head, tris.ctypes.data, len(tris), rgba.ctypes.data_as(N.c_double_p), a.map, a.map, -a.range, a.range,
                order, out.ctypes.data, len(out), C.byref(n), got.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ms))
        wall = (time.perf_counter() - t0) * 1e3
        if rc != 0 or n.value != total or got.tolist() != counts.tolist():
            raise SystemExit("displace_probe: call failed (status %d)" % rc)
        return wall, ms.value

    want = {}
    for name, order in (("mesh", N.DISPLACE_MESH), ("per_triangle", N.DISPLACE_PER_TRIANGLE)):
        want[name] = np.zeros(total, TRI_DTYPE)
        host_ms = [call(L.izpi_host_displace, order, want[name])[0] for _ in range(max(2, a.runs // 2))]
        res["host_twin_%s_wall_ms" % name] = spread(host_ms)
        out = np.zeros(total, TRI_DTYPE)
        dev_ms, wall_ms = [], []
        for run in range(a.runs + 1):
            wall, ms = call(L.izpi_gpu_displace, order, out, ctx)
            if run == 0:  # the warm-up, and the check
                if out.tobytes() != want[name].tobytes():
                    raise SystemExit("displace_probe: device result differs from the host twin (%s)" % name)
                continue
            dev_ms.append(ms)
            wall_ms.append(wall)
        res["gpu_%s" % name] = {"device_ms": spread(dev_ms), "wall_ms_with_upload_and_copy_back": spread(wall_ms)}
    want = want["per_triangle"]

    s = Scene("displaced plane")
    s.lambert(s.constant((0.5, 0.5, 0.5)))
    s.set_camera((0.5, -12, 0.5), (0.5, 0, 0.5), (0, 0, 1), 8, 1, 0, 10, 0, 1, 1)
    s.tris = want
    host = HostScene(s, skip_bvh=True)
    boxes = host.prim_boxes()
    bvh_ms = []
    for run in range(a.runs + 1):
        nodes, order, ms = build_bvh4(ctx, boxes, gpu_leaf_max(host.desc))
        if run:
            bvh_ms.append(ms)
    res["gpu_bvh4_build_ms"] = spread(bvh_ms)
    res["bvh4_nodes"] = len(nodes)
    host.close()
    L.izpi_gpu_close(ctx)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
