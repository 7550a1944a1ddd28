"""Inputs and comparisons shared by the displacement tests (CPU and GPU): the maps, the
source triangles, the scene file, and the bitwise comparison with its NaN rule."""
import functools

import numpy as np

from izpi_amd.scene import TRI_DTYPE
from tests import displace_ref as DR


def smooth_map(width, height):
    """z[y][x] = 0.5 + 0.25 sin(0.37 x) + 0.25 cos(0.23 y + 0.11 x) in the blue channel;
    R = 0.1 and G = 0.9, so that reading another channel shows."""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    rgba = np.zeros((height, width, 4))
    rgba[..., 0], rgba[..., 1], rgba[..., 3] = 0.1, 0.9, 1.0
    rgba[..., 2] = 0.5 + 0.25 * np.sin(0.37 * x) + 0.25 * np.cos(0.23 * y + 0.11 * x)
    return rgba


def flat_map(width, height, z=0.5):
    rgba = np.zeros((height, width, 4))
    rgba[..., 2], rgba[..., 3] = z, 1.0
    return rgba


def step_map():
    """9 x 9, Z = 0 in columns 0..4 and 1 in columns 5..8: the level-cap case."""
    rgba = flat_map(9, 9, 0.0)
    rgba[:, 5:, 2] = 1.0
    return rgba


def tris(rows, material=0):
    """TRI_DTYPE from rows of (v0, v1, v2, (u0, v0), (u1, v1), (u2, v2))."""
    t = np.zeros(len(rows), TRI_DTYPE)
    for k, (a, b, c, uv0, uv1, uv2) in enumerate(rows):
        t[k]["v0"], t[k]["v1"], t[k]["v2"] = a, b, c
        t[k]["uv"] = (*uv0, *uv1, *uv2)
    t["material"] = material
    return t


# the source of displacement_test.go
T = [((-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0), (1, 0), (0.5, 1))]
# a quad in the XZ plane, uv = (x, z)
QUAD = [((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0), (1, 0), (1, 1)),
        ((0, 0, 0), (1, 0, 1), (0, 0, 1), (0, 0), (1, 1), (0, 1))]
# three equal u: f = 1 / 0, NaN tangents, and NaN * 0 reaches every vertex
EQUAL_U = [((0, 0, 0), (1, 0, 0), (0, 1, 0), (0.5, 0), (0.5, 1), (0.5, 0.5))]


def grid_plane(quads):
    """quads x quads quads over the unit square of the XZ plane, uv = position."""
    rows = []
    for j in range(quads):
        for i in range(quads):
            x0, x1, z0, z1 = i / quads, (i + 1) / quads, j / quads, (j + 1) / quads
            rows.append(((x0, 0, z0), (x1, 0, z0), (x1, 0, z1), (x0, z0), (x1, z0), (x1, z1)))
            rows.append(((x0, 0, z0), (x1, 0, z1), (x0, 0, z1), (x0, z0), (x1, z1), (x0, z1)))
    return rows


# name -> (source rows, map, dmin, dmax): the cases of the issue's test 2
CASES = {
    "smooth_T": (T, lambda: smooth_map(33, 17), -8.0, 8.0),
    "smooth_quad": (QUAD, lambda: smooth_map(33, 33), -4.0, 4.0),
    "equal_u": (EQUAL_U, lambda: smooth_map(33, 17), -8.0, 8.0),
    "flat_9x9": (T, lambda: flat_map(9, 9), 0.0, 1.0),
    "flat_13x5": (T, lambda: flat_map(13, 5), 0.0, 1.0),
    "flat_5x13": (T, lambda: flat_map(5, 13), 0.0, 1.0),
}
FLAT_COUNTS = {"flat_9x9": 4, "flat_13x5": 16, "flat_5x13": 16}


def to_ref(t):
    """TRI_DTYPE rows -> the restatement's tuples."""
    out = []
    for r in t:
        uv = [float(x) for x in r["uv"]]
        out.append((tuple(map(float, r["v0"])), tuple(map(float, r["v1"])), tuple(map(float, r["v2"])),
                    (uv[0], uv[2], uv[4]), (uv[1], uv[3], uv[5]), int(r["material"])))
    return out


def from_ref(ref):
    t = np.zeros(len(ref), TRI_DTYPE)
    for k, (a, b, c, us, vs, mat) in enumerate(ref):
        t[k]["v0"], t[k]["v1"], t[k]["v2"] = a, b, c
        t[k]["uv"] = (us[0], vs[0], us[1], vs[1], us[2], vs[2])
        t[k]["material"] = mat
    return t


@functools.lru_cache(maxsize=None)
def reference(name, order):
    """The restatement's answer for CASES[name]: (TRI_DTYPE triangles, counts). Computed once."""
    rows, make_map, dmin, dmax = CASES[name]
    texels = make_map().tolist()
    fn = DR.per_triangle if order == "per_triangle" else DR.mesh
    out, counts = fn(to_ref(tris(rows, material=3)), texels, dmin, dmax)
    return from_ref(out), counts


def assert_same_triangles(got, want):
    """Bitwise on vertices, UVs, material and pad; a NaN vertex component must be NaN at the
    same place in both (its sign and payload are not compared)."""
    assert len(got) == len(want), (len(got), len(want))
    for f in ("v0", "v1", "v2"):
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        na, nb = np.isnan(a), np.isnan(b)
        assert (na == nb).all(), (f, np.argwhere(na != nb)[:5].tolist())
        bad = (a.view(np.uint64) != b.view(np.uint64)) & ~na
        assert not bad.any(), (f, np.argwhere(bad)[:5].tolist(), a[bad][:3], b[bad][:3])
    a, b = np.ascontiguousarray(got["uv"]), np.ascontiguousarray(want["uv"])
    assert (a.view(np.uint64) == b.view(np.uint64)).all(), np.argwhere(a.view(np.uint64) != b.view(np.uint64))[:5].tolist()
    assert (got["material"] == want["material"]).all()
    assert (got["pad"] == 0).all()


# The ingestion scene of the issue's test 4: one Lambert material, one declared map, two
# DISPLACE triangles (the quad) with a plain triangle between them, one sphere.
MAP_FILE = "waves.exr"


def _tri_text(row, displace):
    a, b, c, uv0, uv1, uv2 = row
    s = "    triangles {\n"
    for name, v in (("vertex0", a), ("vertex1", b), ("vertex2", c)):
        s += "      %s { x: %r y: %r z: %r }\n" % (name, float(v[0]), float(v[1]), float(v[2]))
    for name, v in (("uv0", uv0), ("uv1", uv1), ("uv2", uv2)):
        s += "      %s { u: %r v: %r }\n" % (name, float(v[0]), float(v[1]))
    s += '      material_name: "ground"\n'
    if displace:
        s += displace
    return s + "    }\n"


PLAIN = ((0, -0.5, 0), (1, -0.5, 0), (0, -0.5, 1), (0, 0), (1, 0), (0, 1))
# For the frames: the CPU oracle needs a light to sample, so the rendered variant of the
# scene (light=True) adds a DIFFUSE_LIGHT material and one emitting triangle at the end.
LAMP = ((-6, -14, -6), (7, -14, -6), (-6, -14, 7), (0, 0), (1, 0), (0, 1))


def scene_text(map_name=MAP_FILE, declare=True, dmin=-4.0, dmax=4.0, light=False):
    op = '      operator: DISPLACE\n      displace { min: %r max: %r displacement_map: "%s" }\n' % (dmin, dmax, map_name)
    s = 'name: "displaced quad"\ncolour_representation: RGB\n'
    s += ("camera { lookfrom { x: 0.5 y: -12 z: 0.5 } lookat { x: 0.5 y: 0 z: 0.5 } vup { z: 1 } vfov: 8 aspect: 1 "
          "focusdist: 10 time1: 1 exposure: 1 }\n")
    s += ('materials { key: "ground" value { name: "ground" type: LAMBERT lambert { albedo { constant { value '
          "{ x: 0.5 y: 0.6 z: 0.7 } } } } } }\n")
    if light:
        s += ('materials { key: "lamp" value { name: "lamp" type: DIFFUSE_LIGHT diffuselight { emit { constant { value '
              "{ x: 4 y: 4 z: 4 } } } } } }\n")
    if declare:
        s += 'displacement_maps { key: "waves" value { filename: "%s" } }\n' % MAP_FILE
    s += "objects {\n"
    s += _tri_text(QUAD[0], op) + _tri_text(PLAIN, None) + _tri_text(QUAD[1], op)
    if light:
        s += _tri_text(LAMP, None).replace('"ground"', '"lamp"')
    s += '    spheres { center { x: 0.5 y: -6 z: 0.5 } radius: 0.125 material_name: "ground" }\n'
    return s + "}\n"


def restated_scene(light=False):
    """scene_text()'s scene built programmatically, its DISPLACE triangles replaced by the
    restatement's answer: what the ingestion must produce, without going through it."""
    from izpi_amd.scene import Scene
    s = Scene("displaced quad")
    s.lambert(s.constant((0.5, 0.6, 0.7)))
    s.set_camera((0.5, -12, 0.5), (0.5, 0, 0.5), (0, 0, 1), 8, 1, 0, 10, 0, 1, 1)
    want, counts = reference("smooth_quad", "per_triangle")
    want = want.copy()
    want["material"] = 0
    s.tris = np.concatenate([want[:counts[0]], tris([PLAIN]), want[counts[0]:]])
    if light:
        s.tris = np.concatenate([s.tris, tris([LAMP], material=s.diffuse_light(s.constant((4, 4, 4))))])
    s.add_sphere((0.5, -6, 0.5), 0.125, 0)
    return s


def input_tris(si):
    """The triangles of an izpi_scene_input as a TRI_DTYPE copy."""
    import ctypes as C
    n = si.struct.num_tris
    buf = C.string_at(si.struct.tris, n * TRI_DTYPE.itemsize) if n else b""
    return np.frombuffer(buf, TRI_DTYPE).copy()
