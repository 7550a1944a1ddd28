"""An independent Python restatement of izpi's displacement operator, for the tests.

Restates displacement/displacement.go:36-280 (tessellate, isTessellatedEnough,
applyTessellation, applyDisplacement, ApplyDisplacementMap) and ImageTxt.Value
(texture/image.go:73-101, the float64 NRGBA branch) on Python floats, which are IEEE
doubles: every expression keeps the reference's operand order and rounds once per
operation, as Go does on amd64. It never calls the library.

A triangle is a tuple (v0, v1, v2, (u0, u1, u2), (v0, v1, v2), material) with vertices as
3-tuples. A map is a list of rows (row 0 = top) of (r, g, b, a) tuples, or anything
indexable as m[y][x][c].
"""
import math

MAX_LEVELS = 16          # the product's one deviation (IZPI_DISPLACE_MAX_LEVELS)
INT64_MIN = -(1 << 63)


class LevelCap(Exception):
    """A source triangle still had work after MAX_LEVELS levels."""


def go_int(x):
    """int(float64) on amd64: NaN and out-of-range values give the smallest int64."""
    if x != x or x >= 9223372036854775808.0 or x < -9223372036854775808.0:
        return INT64_MIN
    return int(x)


def go_min(x, y):
    """math.Min: -Inf, then NaN, then signed zeros."""
    if x == -math.inf or y == -math.inf:
        return -math.inf
    if x != x or y != y:
        return math.nan
    if x == 0 and x == y:
        return x if math.copysign(1.0, x) < 0 else y
    return x if x < y else y


def go_max(x, y):
    if x == math.inf or y == math.inf:
        return math.inf
    if x != x or y != y:
        return math.nan
    if x == 0 and x == y:
        return y if math.copysign(1.0, x) < 0 else x
    return x if x > y else y


def go_div(a, b):
    """float64 division with IEEE results for a zero divisor."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def go_sqrt(x):
    if x != x or x < 0:
        return math.nan
    return math.sqrt(x)


class ImageTxt:
    """texture.ImageTxt over float64 NRGBA texels."""

    def __init__(self, texels):
        self.data = texels
        self.size_y = len(texels)
        self.size_x = len(texels[0])

    def value(self, u, v):
        i = go_int(u * float(self.size_x))
        j = go_int((1 - v) * (float(self.size_y) - 0.001))
        if i < 0:
            i = 0
        if j < 0:
            j = 0
        if i > self.size_x - 1:
            i = self.size_x - 1
        if j > self.size_y - 1:
            j = self.size_y - 1
        p = self.data[j][i]
        return (float(p[0]), float(p[1]), float(p[2]))


class Constant:
    """texture.Constant, which displacement_test.go uses for its flat maps."""

    def __init__(self, value):
        self._v = tuple(float(x) for x in value)

    def value(self, u, v):
        return self._v


def _mid(a, b):
    return tuple((x + y) / 2.0 for x, y in zip(a, b))


def tessellate(t):
    v0, v1, v2, us, vs, mat = t
    a, b, c = _mid(v0, v1), _mid(v1, v2), _mid(v2, v0)
    ua, va = (us[0] + us[1]) / 2.0, (vs[0] + vs[1]) / 2.0
    ub, vb = (us[1] + us[2]) / 2.0, (vs[1] + vs[2]) / 2.0
    uc, vc = (us[2] + us[0]) / 2.0, (vs[2] + vs[0]) / 2.0
    return [
        (v0, a, c, (us[0], ua, uc), (vs[0], va, vc), mat),
        (a, b, c, (ua, ub, uc), (va, vb, vc), mat),
        (a, v1, b, (ua, us[1], ub), (va, vs[1], vb), mat),
        (c, b, v2, (uc, ub, us[2]), (vc, vb, vs[2]), mat),
    ]


def displacement_variation(t, tex):
    us, vs = t[3], t[4]
    d0 = tex.value(us[0], vs[0])[2]
    d1 = tex.value(us[1], vs[1])[2]
    d2 = tex.value(us[2], vs[2])[2]
    return go_max(d0, go_max(d1, d2)) - go_min(d0, go_min(d1, d2))


def is_tessellated_enough(t, max_du, max_dv, tex, dmin, dmax, threshold):
    us, vs = t[3], t[4]
    uv_ok = (abs(us[1] - us[0]) <= max_du and abs(us[2] - us[1]) <= max_du and abs(us[0] - us[2]) <= max_du and
             abs(vs[1] - vs[0]) <= max_dv and abs(vs[2] - vs[1]) <= max_dv and abs(vs[0] - vs[2]) <= max_dv)
    if not uv_ok:
        return False
    return displacement_variation(t, tex) * abs(dmax - dmin) <= threshold


def apply_tessellation(tris, max_du, max_dv, tex, dmin, dmax, threshold, max_levels=MAX_LEVELS):
    out, work, level = [], list(tris), 0
    while work:
        level += 1
        if max_levels is not None and level > max_levels:
            raise LevelCap("still subdividing after %d levels" % max_levels)
        nxt = []
        for t in work:
            for child in tessellate(t):
                (out if is_tessellated_enough(child, max_du, max_dv, tex, dmin, dmax, threshold) else nxt).append(child)
        work = nxt
    return out


def _unit(v):
    l = go_sqrt((v[0] * v[0]) + (v[1] * v[1]) + (v[2] * v[2]))
    return (go_div(v[0], l), go_div(v[1], l), go_div(v[2], l))


def apply_displacement(tris, tex, dmin, dmax):
    out = []
    for v0, v1, v2, us, vs, mat in tris:
        e1 = (v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2])
        e2 = (v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2])
        normal = _unit(((e1[1] * e2[2]) - (e1[2] * e2[1]), -((e1[0] * e2[2]) - (e1[2] * e2[0])),
                        (e1[0] * e2[1]) - (e1[1] * e2[0])))
        du1, du2 = us[1] - us[0], us[2] - us[0]
        dv1, dv2 = vs[1] - vs[0], vs[2] - vs[0]
        f = go_div(1.0, du1 * dv2 - du2 * dv1)
        tangent = _unit(tuple(f * (dv2 * e1[k] - dv1 * e2[k]) for k in range(3)))
        bitangent = _unit(tuple(f * (-du2 * e1[k] + du1 * e2[k]) for k in range(3)))
        new = []
        for vert, u, v in ((v0, us[0], vs[0]), (v1, us[1], vs[1]), (v2, us[2], vs[2])):
            x, y = 0.0, 0.0
            z = dmin + ((dmax - dmin) * tex.value(u, v)[2])
            d = tuple(tangent[k] * x + bitangent[k] * y + normal[k] * z for k in range(3))  # MatrixVectorMul(tbn, .)
            new.append((vert[0] + d[0], vert[1] + d[1], vert[2] + d[2]))
        out.append((new[0], new[1], new[2], us, vs, mat))
    return out


def apply_displacement_map(tris, texels, dmin, dmax, max_levels=MAX_LEVELS):
    """displacement.ApplyDisplacementMap over `tris` as one mesh (level-major output)."""
    tex = ImageTxt(texels)
    max_du = go_div(4.0, float(tex.size_x - 1))
    max_dv = go_div(4.0, float(tex.size_y - 1))
    done = apply_tessellation(tris, max_du, max_dv, tex, dmin, dmax, 2.0, max_levels)
    return apply_displacement(done, tex, dmin, dmax)


def per_triangle(tris, texels, dmin, dmax, max_levels=MAX_LEVELS):
    """The scene path (transport.go:641): one ApplyDisplacementMap per source triangle.
    Returns (triangles, source-major; outputs per source)."""
    out, counts = [], []
    for t in tris:
        r = apply_displacement_map([t], texels, dmin, dmax, max_levels)
        out += r
        counts.append(len(r))
    return out, counts


def mesh(tris, texels, dmin, dmax, max_levels=MAX_LEVELS):
    """One ApplyDisplacementMap over the mesh (wavefront.go:347); the per-source counts come
    from tagging each source's material slot with its index."""
    tagged = [(t[0], t[1], t[2], t[3], t[4], (k, t[5])) for k, t in enumerate(tris)]
    r = apply_displacement_map(tagged, texels, dmin, dmax, max_levels)
    counts = [0] * len(tris)
    for t in r:
        counts[t[5][0]] += 1
    return [(t[0], t[1], t[2], t[3], t[4], t[5][1]) for t in r], counts
