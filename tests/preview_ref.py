"""TEST INFRASTRUCTURE — the Normal, Albedo and WireFrame samplers restated in Python, on what
the CPU oracle already exports (OracleScene.camera / trace, oracle.gomath, oracle.lbvh4).

    render/rgb.go:27-41        the pixel loop: jitter, GetRay, DeNAN, sum, / numSamples, row H - y
    camera/camera.go:61-89     GetRay, in the operation order of the device's start_path
    fastrandom.go:41-47        the LCG; the per-sample streams of DESIGN section 4 A1
    sampler/normal.go:28-34, albedo.go:30-36, wireframe.go:34-40
    hitable_slice.go:48-70     HitEdge: a second traversal up to tMax = t + 2^-52
    triangle.go:282-302, segment/segment.go:13-30, sphere.go:97-113   the edge tests
    texture/image.go:73-101    ImageTxt.Value

Every vector operation is written out per component in the reference's own order (vec3.Dot
is ((x + y) + z)); Python floats are IEEE doubles and nothing here contracts to an FMA.
The oracle traces at ray time 0, so scenes checked with this keep their spheres static.
"""
import math

import numpy as np

from izpi_amd import _native as N
from izpi_amd.renderer import gpu_leaf_max
from izpi_amd.scene import HostScene
from oracle import oracle as O

MASK64 = (1 << 64) - 1
CAMERA_STREAM_SALT = 0xD6E8FEB86659FD93  # the camera stream of a sample
MAX_FLOAT64 = 1.7976931348623157e308
EPSILON = 2.0 ** -52  # math.Nextafter(1, 2) - 1 (hitable_slice.go:54)
EDGE_ANGLE = 1.6707963267948966  # math.Pi/2.0 + 0.1, folded exactly by the Go compiler and rounded once
HALF_PI = 1.5707963267948966  # math.Pi / 2 (math.Acos(x) = Pi/2 - Asin(x))
HIT_DTYPE = np.dtype([("t", "<f8"), ("u", "<f8"), ("v", "<f8"), ("p", "<f8", 3), ("normal", "<f8", 3),
                      ("prim_ref", "<u4"), ("hit", "<u4")])
SAMPLER_MAP = {"colour": 2, "normal": 1, "wireframe": 3, "albedo": 4, "spectral": 5}  # sampler.go:13-28


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


class Lcg:
    """fastrandom.LCG (fastrandom.go:41-47): state = (a * state + c) mod 2^32."""

    def __init__(self, seed):
        self.state = seed

    def float64(self):
        self.state = (1664525 * self.state + 1013904223) % 4294967296
        return self.state / 4294967296.0


def lcg(seed, n):
    """The first n values and states of the stream, as oracle.lcg returns them."""
    g, vals, states = Lcg(seed), [], []
    for _ in range(n):
        vals.append(g.float64())
        states.append(g.state)
    return vals, states


# ------------------------------------------------------------------ vec3, per component
def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def smul(a, t):
    return (a[0] * t, a[1] * t, a[2] * t)


def dot(a, b):
    return (a[0] * b[0]) + (a[1] * b[1]) + (a[2] * b[2])


def cross(a, b):
    return ((a[1] * b[2]) - (a[2] * b[1]), -((a[0] * b[2]) - (a[2] * b[0])), (a[0] * b[1]) - (a[1] * b[0]))


def length(a):
    return math.sqrt((a[0] * a[0]) + (a[1] * a[1]) + (a[2] * a[2]))


def fdiv(x, y):
    """Go's float64 division: x / 0 is +-Inf or NaN, never a panic."""
    if y == 0.0:
        if x == 0.0 or x != x:
            return math.nan
        return math.copysign(math.inf, x) * math.copysign(1.0, y)
    return x / y


def unit(a):
    k = length(a)
    return (fdiv(a[0], k), fdiv(a[1], k), fdiv(a[2], k))


def denan(c):
    """render.DeNAN (rgb.go:36): NaN and +-Inf components become 0."""
    return tuple(0.0 if (x != x or math.isinf(x)) else x for x in c)


# ------------------------------------------------------------------ the edge tests
def belongs(a, b, c):
    """segment.Belongs (segment/segment.go:13-30)."""
    ab, ac = sub(b, a), sub(c, a)
    k = length(cross(unit(ab), unit(ac)))
    if k >= .005:  # (NaN, when c == a, is not)
        return False
    kac, kab = dot(ab, ac), dot(ab, ab)
    if kac < 0 or kac > kab:
        return False
    return True


def triangle_edge(v0, v1, v2, p):
    """Triangle.HitEdge's flag (triangle.go:289-299)."""
    return belongs(v0, v1, p) or belongs(v1, v2, p) or belongs(v2, v0, p)


def sphere_edge(origin, center, p):
    """Sphere.HitEdge's flag (sphere.go:103-110), math.Asin from the oracle's Go math."""
    a, b = sub(p, origin), sub(p, center)
    theta = HALF_PI - O.gomath(7, fdiv(dot(a, b), length(a) * length(b)))
    return abs(theta) <= EDGE_ANGLE


def second_pass_tmax(t):
    """HitableSlice.HitEdge's tMax of the second traversal (hitable_slice.go:66)."""
    return t + EPSILON


def sphere_root_accepted(t, tmax, tmin=0.001):
    """Sphere.Hit's strict acceptance of a root (sphere.go:73,83)."""
    return t < tmax and t > tmin


# ------------------------------------------------------------------ textures and materials
def go_int(x):
    """int(float64) on amd64: NaN and out-of-range give the minimum int64."""
    if x != x or x >= 9223372036854775808.0 or x < -9223372036854775808.0:
        return -(1 << 63)
    return int(x)


def image_value(texels, tex, u, v):
    """ImageTxt.Value (texture/image.go:73-101) on float64 NRGBA texels."""
    w, h = tex.width, tex.height
    i = go_int(u * float(w))
    j = go_int((1 - v) * (float(h) - 0.001))
    i = 0 if i < 0 else i
    j = 0 if j < 0 else j
    i = w - 1 if i > w - 1 else i
    j = h - 1 if j > h - 1 else j
    k = tex.texel_offset + (j * w + i) * 4
    return (float(texels[k]), float(texels[k + 1]), float(texels[k + 2]))


def texture_value(scene, texels, tex_id, u, v):
    tex = scene.textures[tex_id]
    if tex.kind == N.TEX_IMAGE:
        return image_value(texels, tex, u, v)
    assert tex.kind == N.TEX_CONSTANT
    return tuple(tex.value)


def material_albedo(scene, texels, mat_id, u, v):
    """Material.Albedo(u, v, p) of the five materials (material/*.go)."""
    m = scene.materials[mat_id]
    if m.kind == N.MAT_DIELECTRIC:
        return (1.0, 1.0, 1.0)
    if m.kind == N.MAT_METAL:
        return tuple(m.rgb)
    assert m.kind in (N.MAT_LAMBERT, N.MAT_PBR, N.MAT_DIFFUSE_LIGHT, N.MAT_ISOTROPIC)
    return texture_value(scene, texels, m.albedo_tex, u, v)


def has_rgb_textures(scene):
    """Whether every material has the RGB textures Material.Albedo reads (the Colour sampler's need)."""
    for m in scene.materials:
        if m.kind in (N.MAT_LAMBERT, N.MAT_PBR, N.MAT_DIFFUSE_LIGHT, N.MAT_ISOTROPIC):
            if m.albedo_tex < 0 or scene.textures[m.albedo_tex].kind not in (N.TEX_CONSTANT, N.TEX_IMAGE):
                return False
    return True


# ------------------------------------------------------------------ primary rays
def primary_ray(cam, x, y, s, width, height, seed):
    """rgb.go:33-35 and Camera.GetRay (camera.go:61-89) for sample s of pixel (x, y): the
    jitter from the sample's stream, the lens disc and the time from its camera stream."""
    key = (s << 32) | ((y * width + x) & 0xFFFFFFFF)
    rng = Lcg(splitmix64(seed ^ key) & 0xFFFFFFFF)
    lens = Lcg(splitmix64(seed ^ key ^ CAMERA_STREAM_SALT) & 0xFFFFFFFF)
    u = (float(x) + rng.float64()) / float(width)
    v = (float(y) + rng.float64()) / float(height)
    while True:  # randomInUnitDisc
        rx, ry = lens.float64(), lens.float64()
        px, py, pz = rx * 2.0 - 1.0, ry * 2.0 - 1.0, 0.0 * 2.0 - 0.0
        if (px * px) + (py * py) + (pz * pz) < 1.0:
            break
    rdx, rdy = px * cam.lens_radius, py * cam.lens_radius
    offset = add(smul(tuple(cam.u), rdx), smul(tuple(cam.v), rdy))
    time = cam.time0 + lens.float64() * (cam.time1 - cam.time0)
    origin = tuple(cam.origin)
    ro = add(origin, offset)
    rd = sub(sub(add(add(tuple(cam.lower_left), smul(tuple(cam.horizontal), u)), smul(tuple(cam.vertical), v)), origin), offset)
    return ro, rd, time


def unit_scene():
    """A unit-scale scene for the WireFrame quirks: the camera at the origin looks down -z with
    |direction| about 1, so t is about the distance. A static sphere 2 away (hit near t = 1.5,
    where t + epsilon > t: its silhouette ring draws ink), a second one 8.5 away (hit near
    t = 8, where t + epsilon == t: Sphere.Hit's strict `temp < tMax` loses it and it comes out
    paper), and a Metal and a Dielectric triangle behind them at z = -12."""
    from izpi_amd.scene import Scene
    s = Scene("preview_unit")
    s.add_sphere((-0.4, 0.0, -2.0), 0.5, s.lambert(albedo=s.constant((0.6, 0.5, 0.4))))
    s.add_sphere((1.2, 0.3, -8.5), 0.5, s.diffuse_light(emit=s.constant((4.0, 3.0, 2.0))))
    s.add_triangles([(-6, -5, -12)], [(0.5, -5, -12)], [(-6, 5, -12)], s.metal((0.8, 0.7, 0.6), 0.1))
    s.add_triangles([(0.5, -5, -12)], [(6, -5, -12)], [(6, 5, -12)], s.dielectric(ref_idx=1.5))
    s.set_camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40, 4.0 / 3.0, 0, 1, 0, 1, 1.0)
    return s


def hits_array(hits):
    return np.frombuffer(bytes(hits), HIT_DTYPE).copy()


class PreviewRef:
    """The three samplers over one frame of `scene` on the GPU-built tree (as the tests'
    renderers use it): primary rays and first hits are computed once and shared."""

    def __init__(self, scene, width, height, spp, seed=12345, bvh="gpu"):
        self.scene, self.W, self.H, self.spp, self.seed = scene, width, height, spp, seed
        self.oracle = O.OracleScene(scene, aspect_override=width / height)
        if bvh == "gpu":
            host = HostScene(scene, aspect_override=width / height, skip_bvh=True)
            nodes, order = O.lbvh4(self.oracle.prim_boxes(), gpu_leaf_max(host.desc), N.BVH_PLOC_SAH)
            host.close()
            self.oracle.set_bvh(nodes, order)
        self.texels = np.concatenate(scene.texels) if scene.texels else np.zeros(0)
        cam = self.oracle.camera()
        n = width * height * spp
        self.rays = np.zeros((n, 8))
        self.times = np.zeros(n)
        k = 0
        for y in range(height):
            for x in range(width):
                for s in range(spp):
                    ro, rd, t = primary_ray(cam, x, y, s, width, height, seed)
                    self.rays[k, 0:3], self.rays[k, 3:6], self.times[k] = ro, rd, t
                    k += 1
        self.rays[:, 6], self.rays[:, 7] = 0.001, MAX_FLOAT64
        self.first = hits_array(self.oracle.trace(self.rays))

    def close(self):
        self.oracle.close()

    def _material_of(self, prim_ref):
        idx = int(prim_ref) & 0x7FFFFFFF
        if int(prim_ref) >> 31 == N.PRIM_TRIANGLE:
            return int(self.scene.tris["material"][idx])
        return int(self.scene.spheres["material"][idx])

    def canvas(self, samples):
        """rgb.go:36-41: DeNAN per sample, summed in sample order, / numSamples, alpha 1, row H - y."""
        out = np.zeros((self.H, self.W, 4))
        k = 0
        for y in range(self.H):
            for x in range(self.W):
                c = (0.0, 0.0, 0.0)
                for _ in range(self.spp):
                    c = add(c, denan(samples[k]))
                    k += 1
                if 0 <= self.H - y < self.H:
                    out[self.H - y, x] = (c[0] / float(self.spp), c[1] / float(self.spp), c[2] / float(self.spp), 1.0)
        return out

    def normal_samples(self):
        return [tuple(h["normal"]) if h["hit"] else (0.0, 0.0, 0.0) for h in self.first]

    def albedo_samples(self):
        return [material_albedo(self.scene, self.texels, self._material_of(h["prim_ref"]), float(h["u"]), float(h["v"]))
                if h["hit"] else (0.0, 0.0, 0.0) for h in self.first]

    def wireframe_samples(self, paper, ink):
        """Also returns, per sample, what happened: 'miss', 'lost' (the second traversal found
        nothing), 'tri' / 'sph' with or without '+edge'."""
        paper, ink = tuple(float(c) for c in paper), tuple(float(c) for c in ink)
        idx = np.nonzero(self.first["hit"])[0]
        rays2 = self.rays[idx].copy()
        rays2[:, 7] = [second_pass_tmax(float(t)) for t in self.first["t"][idx]]
        second = hits_array(self.oracle.trace(rays2)) if len(idx) else np.zeros(0, HIT_DTYPE)
        out, what = [paper] * len(self.first), ["miss"] * len(self.first)
        for k, h in zip(idx, second):
            if not h["hit"]:
                what[k] = "lost"
                continue
            ref, p = int(h["prim_ref"]), tuple(float(c) for c in h["p"])
            i = ref & 0x7FFFFFFF
            if ref >> 31 == N.PRIM_TRIANGLE:
                t = self.scene.tris[i]
                edge = triangle_edge(tuple(map(float, t["v0"])), tuple(map(float, t["v1"])), tuple(map(float, t["v2"])), p)
                what[k] = "tri"
            else:
                edge = sphere_edge(tuple(map(float, self.rays[k, 0:3])), tuple(map(float, self.scene.spheres[i]["center"])), p)
                what[k] = "sph"
            if edge:
                out[k] = ink
                what[k] += "+edge"
        return out, what

    def render(self, sampler, paper=(0.0, 0.0, 0.0), ink=(0.0, 0.0, 0.0)):
        if sampler == N.SAMPLER_NORMAL:
            return self.canvas(self.normal_samples())
        if sampler == N.SAMPLER_ALBEDO:
            return self.canvas(self.albedo_samples())
        assert sampler == N.SAMPLER_WIREFRAME
        return self.canvas(self.wireframe_samples(paper, ink)[0])
