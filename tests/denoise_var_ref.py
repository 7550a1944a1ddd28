"""TEST INFRASTRUCTURE — the variance-guided a-trous denoiser restated
in plain Python, independent of izpi_amd/csrc/denoise.h: float loops in the stated order
(Python floats are IEEE doubles and nothing here contracts to an FMA), with exp through
izpi_host_gomath (gomath.h's exp, op 3), as tests/denoise_ref.py does for the filter of
section 3.8. Also the seeded standard errors and the cases the filter's tests share."""
import math

import numpy as np

from izpi_amd import _native as N
from tests import denoise_ref as DR

K3 = (1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0)
H5 = DR.H5


def _live(px, v):
    return DR._live(px) and v >= 0 and math.isfinite(v)


def variance0(S):
    """V_0 (rows of floats) of a canvas of standard errors (rows of 4-float lists)."""
    return [[(s[0] * s[0] + s[1] * s[1]) + s[2] * s[2] for s in row] for row in S]


def iteration(C, V, Nm, A, W, Hh, step, s2, floor, kn, ka):
    """One iteration over lists of rows; returns the new canvas and the new plane."""
    out, vout = [], []
    for y in range(Hh):
        row, vrow = [], []
        for x in range(W):
            p, v = C[y][x], V[y][x]
            if not _live(p, v):
                row.append(list(p))
                vrow.append(v)
                continue
            gs, gk = 0.0, 0.0
            for dy in range(-1, 2):
                qy = y + dy
                if qy < 0 or qy >= Hh:
                    continue
                for dx in range(-1, 2):
                    qx = x + dx
                    if qx < 0 or qx >= W:
                        continue
                    if not _live(C[qy][qx], V[qy][qx]):
                        continue
                    k = K3[dy + 1] * K3[dx + 1]
                    gs += k * V[qy][qx]
                    gk += k
            g = gs / gk
            d = s2 * (g + floor)
            kc = 1.0 / d if d != 0 else math.inf  # (d == 0: an underflowed s2; C's 1 / 0 is +Inf)
            sw, sv, sc = 0.0, 0.0, [0.0, 0.0, 0.0]
            for dy in range(-2, 3):
                qy = y + step * dy
                if qy < 0 or qy >= Hh:
                    continue
                for dx in range(-2, 3):
                    qx = x + step * dx
                    if qx < 0 or qx >= W:
                        continue
                    q, vq = C[qy][qx], V[qy][qx]
                    if not _live(q, vq):
                        continue
                    e = DR._dist2(p, q) * kc
                    if Nm is not None:
                        e = e + DR._dist2(Nm[y][x], Nm[qy][qx]) * kn
                    if A is not None:
                        e = e + DR._dist2(A[y][x], A[qy][qx]) * ka
                    if not e >= 0:
                        continue
                    w = (H5[dy + 2] * H5[dx + 2]) * DR._exp(-e)
                    sw += w
                    for k in range(3):
                        sc[k] += w * q[k]
                    sv += (w * w) * vq
            if sw > 0:
                row.append([sc[0] / sw, sc[1] / sw, sc[2] / sw, p[3]])
                vrow.append(_div(sv, sw * sw))
            else:
                row.append(list(p))
                vrow.append(v)
        out.append(row)
        vout.append(vrow)
    return out, vout


def _div(a, b):
    """IEEE a / b for a >= 0, b >= 0 (Python raises where C gives Inf or NaN)."""
    if b != 0:
        return a / b
    return math.nan if a == 0 or a != a else math.inf


def denoise_var(colour, stderr, normal=None, albedo=None, iterations=N.DENOISE_DEFAULT_ITERATIONS,
                sigma_colour=N.DENOISE_VAR_DEFAULT_SIGMA_COLOUR, sigma_normal=N.DENOISE_DEFAULT_SIGMA_NORMAL,
                sigma_albedo=N.DENOISE_DEFAULT_SIGMA_ALBEDO, variance_floor=N.DENOISE_VAR_DEFAULT_FLOOR):
    """(H, W, 4) float64 arrays in; the filtered (H, W, 4) canvas and its (H, W) variance out."""
    Hh, W = colour.shape[:2]
    C = colour.tolist()
    V = variance0(stderr.tolist())
    Nm = None if normal is None else normal.tolist()
    A = None if albedo is None else albedo.tolist()
    s2 = sigma_colour * sigma_colour
    kn = 1.0 / (sigma_normal * sigma_normal)
    ka = 1.0 / (sigma_albedo * sigma_albedo)
    for i in range(iterations):
        C, V = iteration(C, V, Nm, A, W, Hh, 1 << i, s2, variance_floor, kn, ka)
    return np.array(C, np.float64).reshape(Hh, W, 4), np.array(V, np.float64).reshape(Hh, W)


# ------------------------------------------------------------------ shared seeded inputs
S_VARIANTS = ["nan_stderr", "inf_stderr", "zero_stderr"]


def seeded(width, height, seed=1, variant="plain"):
    """(colour, stderr, normal, albedo): denoise_ref.seeded's frames (its variants included) and
    a seeded non-negative canvas of standard errors around the colour noise's 0.15, alpha 1.0
    wherever the colour's is (a NOISE snapshot's form). The variants of the standard errors:
      nan_stderr   one pixel's has a NaN channel
      inf_stderr   one pixel's has a +Inf channel (V_0 = +Inf)
      zero_stderr  a block of pixels has standard errors 0 (V_0 = 0)"""
    colour, normal, albedo = DR.seeded(width, height, seed, "plain" if variant in S_VARIANTS else variant)
    rng = np.random.default_rng(seed * 7919 + width * 31 + height)
    S = np.zeros((height, width, 4))
    S[..., :3] = np.abs(rng.normal(0.15, 0.05, (height, width, 3)))
    S[..., 3] = 1.0
    S[colour[..., 3] == 0] = 0.0
    cy, cx = height // 2, width // 3
    if variant == "nan_stderr":
        S[cy, cx, 0] = float("nan")
    elif variant == "inf_stderr":
        S[cy, cx, 2] = float("inf")
    elif variant == "zero_stderr":
        S[cy:cy + 5, cx:cx + 6, :3] = 0.0
    return colour, S, normal, albedo


def cases():
    """denoise_ref.cases() and, on 40 x 30 at 5 iterations with both guides, the variants of
    the standard errors; one of them also unguided, where the colour term stands alone."""
    out = list(DR.cases())
    for v in S_VARIANTS:
        out.append((40, 30, v, 5, "both"))
    out.append((40, 30, "zero_stderr", 5, "none"))
    return out


case_id = DR.case_id

_REFERENCE = {}


def reference(case):
    """The restatement's (canvas, variance) for a case, computed once per process (read only)."""
    if case not in _REFERENCE:
        w, h, variant, n, guides = case
        c, S, nm, al = seeded(w, h, variant=variant)
        nm, al = DR.pick_guides(nm, al, guides)
        _REFERENCE[case] = denoise_var(c, S, nm, al, iterations=n)
    return _REFERENCE[case]
