"""TEST INFRASTRUCTURE — albedo demodulation restated in plain Python
around the two restated filters (tests/denoise_ref.py and tests/denoise_var_ref.py, by import):
the divide, the liveness predicate and the multiply are Python floats (IEEE doubles, one
rounding per operation), independent of izpi_amd/csrc/denoise.h. Also the seeded inputs and the
cases the demodulation tests share."""
import math

import numpy as np

from izpi_amd import _native as N
from tests import denoise_ref as DR
from tests import denoise_var_ref as VR

FLOOR = 2.0 ** -10


def modulus(a):
    return a if math.isfinite(a) and a > FLOOR else FLOOR


def demodulate(colour, stderr, albedo):
    """Lists of rows: (D_0, the demodulated standard errors or None, the moduli). A pixel whose
    colour is not live keeps its colour; the standard errors are divided everywhere."""
    D, Sd, M = [], [], []
    for y, row in enumerate(colour):
        drow, srow, mrow = [], [], []
        for x, c in enumerate(row):
            m = [modulus(albedo[y][x][k]) for k in range(3)]
            drow.append([c[k] / m[k] for k in range(3)] + [c[3]] if DR._live(c) else list(c))
            if stderr is not None:
                s = stderr[y][x]
                srow.append([s[k] / m[k] for k in range(3)] + [s[3]])
            mrow.append(m)
        D.append(drow)
        Sd.append(srow)
        M.append(mrow)
    return D, (Sd if stderr is not None else None), M


def remodulate(colour, D, V0, M, F):
    """The filtered demodulated canvas F (an array) back into colour: F * m where D_0 was live
    (and V_0, when there is one, finite and >= 0), the input's four doubles elsewhere."""
    out = np.array(colour, np.float64)
    for y, row in enumerate(D):
        for x, d in enumerate(row):
            live = DR._live(d) if V0 is None else VR._live(d, V0[y][x])
            if live:
                for k in range(3):
                    out[y, x, k] = float(F[y, x, k]) * M[y][x][k]
    return out


def denoise(colour, normal, albedo, iterations=N.DENOISE_DEFAULT_ITERATIONS, **sigmas):
    """The fixed-sigma filter with IZPI_DENOISE_DEMODULATE: arrays in, the canvas out."""
    if iterations == 0:
        return DR.denoise(colour, normal, albedo, iterations=0, **sigmas)
    C = colour.tolist()
    D, _, M = demodulate(C, None, albedo.tolist())
    F = DR.denoise(np.array(D, np.float64).reshape(colour.shape), normal, albedo, iterations=iterations, **sigmas)
    return remodulate(C, D, None, M, F)


def denoise_var(colour, stderr, normal, albedo, iterations=N.DENOISE_DEFAULT_ITERATIONS, **kw):
    """The variance-guided filter with the flag: (canvas, variance of the demodulated canvas)."""
    if iterations == 0:
        return VR.denoise_var(colour, stderr, normal, albedo, iterations=0, **kw)
    C = colour.tolist()
    D, Sd, M = demodulate(C, stderr.tolist(), albedo.tolist())
    F, var = VR.denoise_var(np.array(D, np.float64).reshape(colour.shape), np.array(Sd, np.float64).reshape(colour.shape),
                            normal, albedo, iterations=iterations, **kw)
    return remodulate(C, D, VR.variance0(Sd), M, F), var


# ------------------------------------------------------------------ shared seeded inputs
def seeded(width, height, seed=1):
    """(colour, stderr, normal, albedo): denoise_var_ref.seeded's colour, standard errors and
    normals under an albedo seeded in (0.05, 1), two regions as the normals'. Where they fit
    (height > 1; the rest from 8 x 8 on) the frames also hold
      albedo   a block of 0, a block at 2^-12, one negative, one NaN and one +Inf texel
      colour   a dead row 0, a NaN pixel, and one pixel at 1e308 over a texel of the 0 block
               (its quotient overflows, so the pixel comes back as the input)
      stderr   a NaN channel."""
    colour, S, normal, _ = VR.seeded(width, height, seed)
    rng = np.random.default_rng(seed * 6151 + width * 53 + height)
    yy, xx = np.mgrid[0:height, 0:width]
    left = (2 * xx + yy) < (width + height // 2)
    albedo = np.ones((height, width, 4))
    albedo[..., :3] = np.where(left[..., None], rng.uniform(0.5, 1.0, (height, width, 3)),
                               rng.uniform(0.05, 0.5, (height, width, 3)))
    if height > 1:
        colour[0] = 0.0
        S[0] = 0.0
        albedo[0] = 0.0
    if width >= 8 and height >= 8:
        cy, cx = height // 2, width // 3
        albedo[2:5, 1:4, :3] = 0.0
        albedo[5:7, 2:6, :3] = 2.0 ** -12
        albedo[cy + 2, cx, 0] = -0.25
        albedo[cy + 2, cx + 2, 1] = float("nan")
        albedo[cy + 3, cx + 1, 2] = float("inf")
        colour[cy, cx, 1] = float("nan")
        colour[3, 2, 0] = 1e308
        S[cy - 2, cx + 1, 2] = float("nan")
    return colour, S, normal, albedo


SIZES = [(40, 30), (37, 19), (1, 1), (1, 7)]  # width, height
GUIDES = ["both", "albedo"]  # with and without the Normal guide


def cases():
    """(width, height, iterations, guides): every size at 5 iterations with both guides, 40 x 30
    at every other iteration count, and two sizes without the Normal guide."""
    out = [(w, h, 5, "both") for w, h in SIZES]
    out += [(40, 30, n, "both") for n in (0, 1, 8)]
    out += [(40, 30, 5, "albedo"), (37, 19, 1, "albedo")]
    return out


def case_id(c):
    return "%dx%d-n%d-%s" % c


def pick_guides(normal, albedo, guides):
    return (normal if guides == "both" else None), albedo


_REFERENCE = {}


def reference(case, var):
    """The restatement's result for a case, computed once per process (treat as read-only): the
    canvas of the fixed filter, or with `var` (canvas, variance) of the variance-guided one."""
    key = (case, bool(var))
    if key not in _REFERENCE:
        w, h, n, guides = case
        c, S, nm, al = seeded(w, h)
        nm, al = pick_guides(nm, al, guides)
        _REFERENCE[key] = denoise_var(c, S, nm, al, iterations=n) if var else denoise(c, nm, al, iterations=n)
    return _REFERENCE[key]
