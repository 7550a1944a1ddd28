"""The noise estimate of a progressive session, restated in numpy.

Per-sample canvases come from the CPU oracle: oracle_render keys sample s of pixel pix with
seed ^ (s << 32 | pix), so a one-sample render with seed ^ (s << 32) is exactly sample s of
the original request (a forward Spectral one: the weighed X, Y, Z). Sums and second moments
are folded from them in sample order, one IEEE operation at a time (numpy's elementwise
float64 arithmetic fuses nothing and its sqrt is correctly rounded); then the per-pixel rule
and the frame statistic are written out, sum_error's tree included.

Everything here works on canvases (H, W, ...) in Render's layout, pixel (x, y) in row H - y;
sample row y = 0 never reaches a canvas (A9), which is also why it is not counted.
"""
import ctypes as C
import functools

import numpy as np

from izpi_amd import _native as N
from izpi_amd.renderer import common_tiles
from oracle import oracle as O

BLOCK = 256


# ------------------------------------------------------------------ samples
def sample_canvases(scene, W, H, n, sampler, acc, seed=12345, tiles=None, threads=8):
    """[n] canvases (H, W, 4): canvas s holds sample s of every pixel of the request."""
    o = O.OracleScene(scene, aspect_override=W / H)
    out = []
    for s in range(n):
        req = N.RenderReq(width=W, height=H, spp=1, max_depth=50, sampler=sampler, seed=seed ^ (s << 32),
                          abi_version=N.IZPI_ABI_VERSION, accumulation=acc)
        keep = None
        if tiles is not None:
            keep = np.ascontiguousarray(tiles, np.uint32).reshape(-1, 4)
            req.num_tiles = len(keep)
            req.tiles = keep.ctypes.data_as(C.POINTER(C.c_uint32))
        canvas, _ = o.render(req, threads=threads)
        out.append(canvas.reshape(H, W, 4).copy())
    o.close()
    return out


def fold(canvases, n):
    """(sums, moment2), each (H, W, 3), of the first n sample canvases, in sample order."""
    s = np.zeros(canvases[0].shape[:2] + (3,))
    m2 = np.zeros_like(s)
    with np.errstate(all="ignore"):
        for c in canvases[:n]:
            x = c[..., :3]
            s = s + x
            m2 = m2 + x * x
    return s, m2


def mean_of(s, n, sampler):
    """The canvas rule: col / n (rgb.go:38), or sum * (1 / n) for Spectral (render/spectral.go:98-99)."""
    with np.errstate(all="ignore"):
        if sampler == N.SAMPLER_SPECTRAL:
            return s * (np.float64(1.0) / np.float64(n))
        return s / np.float64(n)


# ------------------------------------------------------------------ the rule
def pixel_rule(s, m2, n, sampler, floor):
    """Arrays (..., 3) of sums and moments after n >= 2 samples -> (se (..., 3), e (...), finite (...))."""
    assert n >= 2
    s, m2 = np.asarray(s, np.float64), np.asarray(m2, np.float64)
    nn, n1 = np.float64(n), np.float64(n - 1)
    with np.errstate(all="ignore"):
        mean = mean_of(s, n, sampler)
        v = (m2 - (s * s) / nn) / n1
        v = np.where(v > 0, v, 0.0)  # !(v > 0) -> 0: rounding below zero, and NaN
        se = np.sqrt(v / nn)
        a = np.abs(mean)
        e = ((se[..., 0] + se[..., 1]) + se[..., 2]) / (((a[..., 0] + a[..., 1]) + a[..., 2]) + np.float64(floor))
    finite = np.isfinite(s).all(axis=-1) & np.isfinite(m2).all(axis=-1) & np.isfinite(e)
    return se, e, finite


def tree_sum(e):
    """sum_error of the packed values e (already +0.0 where a pixel does not take part)."""
    e = np.asarray(e, np.float64)
    blocks = (len(e) + BLOCK - 1) // BLOCK
    v = np.zeros((blocks, BLOCK))
    v.reshape(-1)[:len(e)] = e
    stride = BLOCK // 2
    while stride:
        v[:, :stride] = v[:, :stride] + v[:, stride:2 * stride]
        stride //= 2
    total = np.float64(0.0)
    for b in range(blocks):
        total = total + v[b, 0]
    return float(total)


def frame_stat(e, finite, counted, done, threshold, tolerated, min_spp):
    """The statistic over packed arrays (one entry per pixel of the packed order)."""
    e, finite, counted = np.asarray(e, np.float64), np.asarray(finite, bool), np.asarray(counted, bool)
    good = counted & finite
    pixels, nonfinite = int(counted.sum()), int((counted & ~finite).sum())
    above = int((good & (e > threshold)).sum())
    st = {"pixels": pixels, "nonfinite": nonfinite, "above": above,
          "max_error": float(e[good].max()) if good.any() else 0.0,
          "sum_error": tree_sum(np.where(good, e, 0.0)), "done": int(done)}
    st["converged"] = int(done >= min_spp and float(above) <= tolerated * float(pixels - nonfinite))
    return st


def packed_xy(tiles):
    """(x, y) of every pixel in packed order: tile after tile, each by sample row y then x."""
    xs, ys = [], []
    for x0, y0, x1, y1 in np.asarray(tiles, np.int64).reshape(-1, 4):
        yy, xx = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        xs.append(xx.reshape(-1))
        ys.append(yy.reshape(-1))
    return np.concatenate(xs), np.concatenate(ys)


def reference(canvases, n, W, H, sampler, tiles=None, threshold=0.25, floor=0.01, tolerated=0.05, min_spp=8):
    """(NOISE snapshot (H, W, 4), statistic) after the first n sample canvases. tiles: the
    session's (None: the whole frame in common.Tiles order). Pixels outside the tiles, and
    canvas row 0, stay zero, as in a snapshot into a zeroed buffer."""
    s, m2 = fold(canvases, n)
    se, e, finite = pixel_rule(s, m2, n, sampler, floor)
    x, y = packed_xy(common_tiles(W, H) if tiles is None else tiles)
    counted = y >= 1
    row = np.where(counted, H - y, 0)  # (row 0 is read for the uncounted, and masked out)
    stat = frame_stat(e[row, x], finite[row, x], counted, n, threshold, tolerated, min_spp)
    snap = np.zeros((H, W, 4))
    snap[row[counted], x[counted], :3] = se[row[counted], x[counted]]
    snap[row[counted], x[counted], 3] = 1.0
    return snap, stat


def packed_sums(canvases, n, W, H, tiles=None):
    """(sums (P, 3), moment2 (P, 3), counted (P,)) in packed order, for the host twin; the
    uncounted pixels (sample row 0, which no canvas holds) carry zeros."""
    s, m2 = fold(canvases, n)
    x, y = packed_xy(common_tiles(W, H) if tiles is None else tiles)
    counted = y >= 1
    row = np.where(counted, H - y, 0)
    ps, pm = s[row, x].copy(), m2[row, x].copy()
    ps[~counted] = 0.0
    pm[~counted] = 0.0
    return ps, pm, counted


# ------------------------------------------------------------------ shared cases
@functools.lru_cache(maxsize=None)
def case_canvases(which, acc, n, size=None, seed=12345):
    """The sample canvases of tests/test_forward_accumulation.scene_case(which), computed once
    per process and shared (read only). size: (W, H) instead of the case's own."""
    from tests.test_forward_accumulation import scene_case
    scene, W, H, _, sampler = scene_case(which)
    if size is not None:
        W, H = size
    return tuple(sample_canvases(scene, W, H, n, sampler, acc, seed)), W, H, sampler
