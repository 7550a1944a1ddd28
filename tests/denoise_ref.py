"""TEST INFRASTRUCTURE — the edge-avoiding a-trous denoiser restated
in plain Python, independent of izpi_amd/csrc/denoise.h: float loops in the stated order
(Python floats are IEEE doubles and nothing here contracts to an FMA), with exp through
izpi_host_gomath (gomath.h's exp, op 3). Also the seeded inputs the denoiser's tests share."""
import math

import numpy as np

from izpi_amd import _native as N

H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def _exp(x):
    return N.lib().izpi_host_gomath(3, x, 0.0)


def _live(px):
    return px[3] != 0 and math.isfinite(px[0]) and math.isfinite(px[1]) and math.isfinite(px[2])


def _dist2(a, b):
    d0, d1, d2 = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (d0 * d0 + d1 * d1) + d2 * d2


def iteration(C, Nm, A, W, Hh, step, kc, kn, ka):
    """One iteration over lists of rows of 4-float lists; returns the new canvas (same form)."""
    out = []
    for y in range(Hh):
        row = []
        for x in range(W):
            p = C[y][x]
            if not _live(p):
                row.append(list(p))
                continue
            sw, sc = 0.0, [0.0, 0.0, 0.0]
            for dy in range(-2, 3):
                qy = y + step * dy
                if qy < 0 or qy >= Hh:
                    continue
                for dx in range(-2, 3):
                    qx = x + step * dx
                    if qx < 0 or qx >= W:
                        continue
                    q = C[qy][qx]
                    if not _live(q):
                        continue
                    e = _dist2(p, q) * kc
                    if Nm is not None:
                        e = e + _dist2(Nm[y][x], Nm[qy][qx]) * kn
                    if A is not None:
                        e = e + _dist2(A[y][x], A[qy][qx]) * ka
                    if not e >= 0:
                        continue
                    w = (H5[dy + 2] * H5[dx + 2]) * _exp(-e)
                    sw += w
                    for k in range(3):
                        sc[k] += w * q[k]
            if sw > 0:
                row.append([sc[0] / sw, sc[1] / sw, sc[2] / sw, p[3]])
            else:
                row.append(list(p))
        out.append(row)
    return out


def denoise(colour, normal=None, albedo=None, iterations=N.DENOISE_DEFAULT_ITERATIONS,
            sigma_colour=N.DENOISE_DEFAULT_SIGMA_COLOUR, sigma_normal=N.DENOISE_DEFAULT_SIGMA_NORMAL,
            sigma_albedo=N.DENOISE_DEFAULT_SIGMA_ALBEDO):
    """(H, W, 4) float64 arrays in, the denoised (H, W, 4) array out."""
    Hh, W = colour.shape[:2]
    C = colour.tolist()
    Nm = None if normal is None else normal.tolist()
    A = None if albedo is None else albedo.tolist()
    kn = 1.0 / (sigma_normal * sigma_normal)
    ka = 1.0 / (sigma_albedo * sigma_albedo)
    for i in range(iterations):
        s = math.ldexp(1.0, -i)
        kc = 1.0 / ((sigma_colour * s) * (sigma_colour * s))
        C = iteration(C, Nm, A, W, Hh, 1 << i, kc, kn, ka)
    return np.array(C, np.float64).reshape(Hh, W, 4)


# ------------------------------------------------------------------ shared seeded inputs
def seeded(width, height, seed=1, variant="plain"):
    """(colour, normal, albedo): noise over a two-region guide (the regions meet on a slanted
    line, so neither border is special). Every pixel is written (alpha 1) unless the variant
    says otherwise:
      dead_row0    row 0 is what Render leaves there: zeros, alpha 0
      nan_pixel    one colour pixel has a NaN channel
      inf_pixel    one colour pixel has a +Inf channel
      nan_guide    one normal and one albedo texel hold a NaN"""
    rng = np.random.default_rng(seed * 1000003 + width * 1009 + height)
    yy, xx = np.mgrid[0:height, 0:width]
    left = (2 * xx + yy) < (width + height // 2)
    colour = np.ones((height, width, 4))
    colour[..., :3] = np.where(left[..., None], 0.7, 0.2) + rng.normal(0.0, 0.15, (height, width, 3))
    normal = np.zeros((height, width, 4))
    normal[..., :3] = np.where(left[..., None], (1.0, 0.0, 0.0), (0.0, 0.6, 0.8)) + rng.normal(0.0, 0.02, (height, width, 3))
    albedo = np.ones((height, width, 4))
    albedo[..., :3] = np.where(left[..., None], (0.8, 0.8, 0.8), (0.9, 0.1, 0.1)) + rng.normal(0.0, 0.01, (height, width, 3))
    cy, cx = height // 2, width // 3
    if variant == "dead_row0":
        colour[0] = 0.0
        normal[0] = 0.0
        albedo[0] = 0.0
    elif variant == "nan_pixel":
        colour[cy, cx, 1] = float("nan")
    elif variant == "inf_pixel":
        colour[cy, cx, 2] = float("inf")
    elif variant == "nan_guide":
        normal[cy, cx, 0] = float("nan")
        albedo[min(cy + 1, height - 1), cx, 2] = float("nan")
    elif variant != "plain":
        raise ValueError(variant)
    return colour, normal, albedo


SIZES = [(40, 30), (1, 1), (1, 7), (37, 19)]  # width, height
VARIANTS = ["plain", "dead_row0", "nan_pixel", "inf_pixel", "nan_guide"]
ITERATIONS = [0, 1, 5, 8]
GUIDES = ["both", "normal", "none"]


def cases():
    """The (width, height, variant, iterations, guides) cases the twin, the sanitizer program's
    Python side and the device are all checked on: every size at 5 iterations with both
    guides, and on 40 x 30 every variant, every iteration count and every guide set."""
    out = []
    for w, h in SIZES:
        out.append((w, h, "plain", 5, "both"))
    for v in VARIANTS[1:]:
        out.append((40, 30, v, 5, "both"))
    for n in ITERATIONS:
        if n != 5:
            out.append((40, 30, "dead_row0", n, "both"))
    for g in GUIDES[1:]:
        out.append((40, 30, "nan_guide", 5, g))
        out.append((37, 19, "plain", 1, g))
    return out


def case_id(c):
    return "%dx%d-%s-n%d-%s" % c


def pick_guides(normal, albedo, guides):
    return {"both": (normal, albedo), "normal": (normal, None), "none": (None, None)}[guides]


_REFERENCE = {}


def reference(case):
    """The restatement's result for a case, computed once per process (treat as read-only)."""
    if case not in _REFERENCE:
        w, h, variant, n, guides = case
        c, nm, al = seeded(w, h, variant=variant)
        nm, al = pick_guides(nm, al, guides)
        _REFERENCE[case] = denoise(c, nm, al, iterations=n)
    return _REFERENCE[case]
