"""Adaptive sampling of a progressive session, restated in numpy on top
of tests/noise_ref.py: the oracle's one-sample canvases, folded per pixel in sample order for as
long as the pixel is active, and the rule (noise_ref.pixel_rule at n = done; a pixel stays
active iff it is counted, finite and e > threshold) applied after the steps the caller names.

The expected counters are the oracle's: every sample s of a step is one oracle render with
spp = 1 and seed ^ (s << 32) (noise_ref.sample_canvases' rule) over that step's active pixels
as a list of 1 x 1 tiles (the session's own tiles until the first retirement), and the counters
are added up. The oracle takes such a list as it takes any other.

Arrays are in the session's packed order (tile after tile, by sample row y then x) unless
they are canvases (H, W, ...), pixel (x, y) in row H - y; sample row 0 reaches no canvas.
"""
import ctypes as C

import numpy as np

from izpi_amd import _native as N
from izpi_amd.renderer import common_tiles
from oracle import oracle as O
from tests import noise_ref as NR

COUNTERS = ("rays", "node_visits", "tri_tests", "sph_tests", "light_tri_tests", "light_sph_tests", "samples")


def rule_at(s, m2, n, sampler, floor):
    """pixel_rule with a sample count per pixel (every n >= 2): (se (P, 3), e (P,), finite (P,))."""
    n = np.asarray(n)
    se, e, fin = np.zeros(s.shape), np.zeros(len(s)), np.ones(len(s), bool)
    for v in np.unique(n):
        m = n == v
        se[m], e[m], fin[m] = NR.pixel_rule(s[m], m2[m], int(v), sampler, floor)
    return se, e, fin


def mean_at(s, n, sampler):
    """The canvas rule with a sample count per pixel."""
    nn = np.asarray(n, np.float64)[:, None]
    with np.errstate(all="ignore"):
        if sampler == N.SAMPLER_SPECTRAL:
            return s * (np.float64(1.0) / nn)
        return s / nn


def to_canvas(values, x, y, H, W, counted):
    """Packed (P, 3) values as an (H, W, 4) snapshot into a zeroed buffer (alpha 1.0)."""
    out = np.zeros((H, W, 4))
    out[H - y[counted], x[counted], :3] = values[counted]
    out[H - y[counted], x[counted], 3] = 1.0
    return out


def simulate(which, acc, steps, rule, size=None, tiles=None, evaluate=None, counters=True, seed=12345):
    """An adaptive session over tests.test_forward_accumulation.scene_case(which): `steps` are
    the samples asked of each step; evaluate(done) says whether adapt follows the step (None:
    after every step with done >= 2). rule: threshold, floor, tolerated, min_spp.
    Returns (one dict per step, W, H, sampler). A step's dict: done; n (P,) the n_p; n_map (H, W);
    active (P,) after the step's adapt; adapt (its integers, or None without one); canvas, noise,
    samples_snap (H, W, 4): the three snapshots; stat: noise()'s statistic; samples: the sum of
    n_p; counters: cumulative (when asked for); rendered: the pixels the step rendered; sums, m2,
    counted, e: the packed sums, moments, counted mask and e (at each pixel's n_p) after the step."""
    from tests.test_forward_accumulation import scene_case
    scene, W, H, _, sampler = scene_case(which)
    if size is not None:
        W, H = size
    cap = sum(steps)
    canvases = NR.case_canvases(which, acc, cap, size, seed)[0]
    session_tiles = np.asarray(common_tiles(W, H) if tiles is None else tiles, np.uint32).reshape(-1, 4)
    x, y = NR.packed_xy(session_tiles)
    P = len(x)
    counted = y >= 1
    row = np.where(counted, H - y, 0)
    s, m2 = np.zeros((P, 3)), np.zeros((P, 3))
    n = np.zeros(P, np.int64)
    active = np.ones(P, bool)
    bad = np.zeros(P, bool)  # counted pixels that retired non-finite
    retired_any = False
    total = dict.fromkeys(COUNTERS, 0)
    o = O.OracleScene(scene, aspect_override=W / H) if counters else None
    done, out = 0, []
    for k in steps:
        k = min(k, cap - done) if active.any() else 0
        rendered = int(active.sum()) if k else 0
        for smp in range(done, done + k):
            xs = canvases[smp][row, x, :3]
            with np.errstate(all="ignore"):
                s[active] = s[active] + xs[active]
                m2[active] = m2[active] + xs[active] * xs[active]
            if counters:
                req = N.RenderReq(width=W, height=H, spp=1, max_depth=50, sampler=sampler, seed=seed ^ (smp << 32),
                                  abi_version=N.IZPI_ABI_VERSION, accumulation=acc)
                if retired_any:
                    keep = np.ascontiguousarray(np.stack([x[active], y[active], x[active], y[active]], 1), np.uint32)
                elif tiles is not None:
                    keep = np.ascontiguousarray(session_tiles)
                else:
                    keep = None
                if keep is not None:
                    req.num_tiles = len(keep)
                    req.tiles = keep.ctypes.data_as(C.POINTER(C.c_uint32))
                st = o.render(req, threads=8)[1]
                for c in COUNTERS:
                    total[c] += st[c]
        n[active] += k
        done += k
        adapt = None
        if done >= 2 and (evaluate(done) if evaluate else True):
            _, e, fin = NR.pixel_rule(s, m2, done, sampler, rule["floor"])
            stay = active & counted & fin & (e > rule["threshold"])
            bad |= active & counted & ~fin
            adapt = {"pixels": int(counted.sum()), "nonfinite": int(bad.sum()), "active": int(stay.sum()),
                     "retired": int(active.sum() - stay.sum()), "samples": int(n.sum()), "done": done}
            adapt["converged"] = int(done >= rule["min_spp"] and
                                     float(adapt["active"]) <= rule["tolerated"] * float(adapt["pixels"] - adapt["nonfinite"]))
            active = stay
            retired_any = retired_any or not active.all()
        step = {"done": done, "n": n.copy(), "active": active.copy(), "adapt": adapt, "samples": int(n.sum()),
                "counters": dict(total), "rendered": rendered, "sums": s.copy(), "m2": m2.copy(), "counted": counted}
        nm = np.zeros((H, W), np.int64)
        nm[row[counted], x[counted]] = n[counted]
        step["n_map"] = nm
        step["canvas"] = to_canvas(mean_at(s, np.maximum(n, 1), sampler), x, y, H, W, counted)
        step["samples_snap"] = to_canvas(np.repeat(n[:, None], 3, 1).astype(np.float64), x, y, H, W, counted)
        if done >= 2:
            se, e, fin = rule_at(s, m2, n, sampler, rule["floor"])
            step["e"] = e
            step["noise"] = to_canvas(se, x, y, H, W, counted)
            step["stat"] = NR.frame_stat(e, fin, counted, done, rule["threshold"], rule["tolerated"], rule["min_spp"])
        out.append(step)
    if o:
        o.close()
    return out, W, H, sampler


def packed_rows(snap, tiles, H):
    """A canvas-layout snapshot as the packed output of a session over `tiles` (none in sample row 0)."""
    return np.concatenate([snap[H - y, x0:x1 + 1] for x0, y0, x1, y1 in np.asarray(tiles).tolist() for y in range(y0, y1 + 1)])
