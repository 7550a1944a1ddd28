"""Scenes at the renderer's LDS size limits, shared by the CPU and GPU tests of the table
paths (test_table_cases.py, test_gpu_table_paths.py).

render_body copies the scene's small tables into every k_shade / k_tail block's LDS only
when all of them fit (izpi_kern.h: 64 materials, 64 textures, 64 lights, 384 SPD entries, 128
background entries), its primitives' records when there are at most 64, and make_tracer
traverses the tree from LDS when num_inner * 128 + num_prims * 112 <= 4096. Every case here
is the Cornell box of configs.py changed so that ONE of these counts sits exactly at its limit
or one past it; `expect` says what the render's IZPI_SHADE_TABLES / IZPI_TRACE_INSTANCE lines
must then report.

build(name) returns the case; build(name, bite=True) the same case with only its
highest-index entry changed (the last material's colour, the last texture's texels or value,
the last light's position, the last spectrum's values, the last background entry, the last
primitive), which must change the oracle's image: otherwise no path reads that entry.
"""
import collections
import functools
import math

import numpy as np

from izpi_amd import _native as N
from izpi_amd import configs
from izpi_amd.scene import Scene

# the limits of izpi_kern.h / trace.hip that the cases sit at
TABLE_LIMIT = 64     # MAT_LDS, MT_LDS, MC_LDS, LT_LDS, TEX_LDS, PR_LDS
SPD_LIMIT = 384      # SPD_LDS
BG_LIMIT = 128       # BG_LDS
BVH_LDS_BYTES = 4096
INNER_BYTES, PRIM_BYTES = 128, 112  # GInner; GLeaf + GPrim

SPP, MAX_DEPTH, SEED = 4, 50, 12345

# scene, sampler, bg: the render's inputs (bg = (wavelengths, values) or None).
# expect: tables / prims of IZPI_SHADE_TABLES (prims_forward where IZPI_ACC_FORWARD differs),
#         tri / lds_bvh / ray_lds of IZPI_TRACE_INSTANCE.
# counts: the descriptor's intended num_materials, num_textures, num_lights, num_spd,
#         num_prims and the background's length.
# frame: (W, H). past: the case lies past a table limit (so has a biting twin).
Case = collections.namedtuple("Case", "scene sampler bg expect counts frame past")

NODE_DTYPE = np.dtype([("mn", "<f4", (3, 4)), ("mx", "<f4", (3, 4)), ("child", "<i4", 4), ("pc", "<i4", 4)])

# the box's triangles in configs.add_box's order
BACK_WALL, FLOOR, CEILING, LIGHT = (0, 1), (2, 3), (4, 5), (6, 7)


def bvh_lds_bytes(host):
    """What make_tracer compares with BVH_LDS_BYTES, from a HostScene's node array: an inner
    node is one whose first slot holds no primitives (scene_pack.cpp: split_bvh)."""
    nd = np.frombuffer(host.nodes().tobytes(), NODE_DTYPE)
    return int((nd["pc"][:, 0] == 0).sum()) * INNER_BYTES + int(host.desc.num_prims) * PRIM_BYTES


def wall_cells(n):
    """n rectangles (a0, a1, b0, b1) tiling the unit square in about sqrt(n) rows, the one
    nearest the square's centre last."""
    rows = max(1, int(round(math.sqrt(n))))
    base, extra = divmod(n, rows)
    cells = []
    for r in range(rows):
        cols = base + (1 if r < extra else 0)
        for c in range(cols):
            cells.append((c / cols, (c + 1) / cols, r / rows, (r + 1) / rows))
    cells.sort(key=lambda q: -((q[0] + q[1] - 1) ** 2 + (q[2] + q[3] - 1) ** 2))
    return cells


def add_back_quad(s, cell, mat):
    """A quad of the back wall (z = 100) with the box's winding, uv spanning the quad."""
    x0, x1, y0, y1 = (100.0 * c for c in cell)
    s.add_triangles([(x1, y0, 100)], [(x0, y0, 100)], [(x1, y1, 100)], mat, uv=[[0, 0, 1, 0, 0, 1]])
    s.add_triangles([(x1, y1, 100)], [(x0, y0, 100)], [(x0, y1, 100)], mat, uv=[[0, 1, 1, 0, 1, 1]])


def add_floor_quad(s, cell, mat):
    x0, x1, z0, z1 = (100.0 * c for c in cell)
    s.add_triangles([(x0, 0, z0)], [(x0, 0, z1)], [(x1, 0, z1)], mat, uv=[[0, 0, 0, 1, 1, 1]])
    s.add_triangles([(x0, 0, z0)], [(x1, 0, z1)], [(x1, 0, z0)], mat, uv=[[0, 0, 1, 1, 1, 0]])


def box_without(s, mats, *walls):
    """configs.add_box less the triangles of `walls` (index pairs above)."""
    configs.add_box(s, mats)
    s.tris = np.delete(s.tris, [i for w in walls for i in w])


def spectral_box_materials(s, light=None):
    """The box's four materials for the Spectral sampler from Gaussians (no SPD entries);
    `light`: the light's spectral texture (default a broad Gaussian)."""
    return {"White": s.lambert(spectral=s.spectral_gaussian(0.73, 550, 400)),
            "Green": s.lambert(spectral=s.spectral_gaussian(0.9, 540, 40)),
            "Red": s.lambert(spectral=s.spectral_gaussian(0.9, 640, 40)),
            "light": s.diffuse_light(spectral=s.spectral_gaussian(15.0, 560, 150) if light is None else light)}


def counts_of(s, bg=None):
    """The table sizes of a Scene as built (the descriptor must report the same)."""
    emit = {i for i, m in enumerate(s.materials) if m.kind in (N.MAT_DIFFUSE_LIGHT, N.MAT_DIELECTRIC)}
    lights = sum(int(m) in emit for m in s.tris["material"]) + sum(int(m) in emit for m in s.spheres["material"])
    return {"num_materials": len(s.materials), "num_textures": len(s.textures), "num_lights": lights,
            "num_spd": len(s.spd_wl), "num_prims": len(s.tris) + len(s.spheres), "num_bg": 0 if bg is None else len(bg[0])}


def expectation(tables, prims, tri, lds_bvh, ray_lds, prims_forward=None):
    e = {"tables": tables, "prims": prims, "tri": tri, "lds_bvh": lds_bvh, "ray_lds": ray_lds}
    if prims_forward is not None:
        e["prims_forward"] = prims_forward
    return e


# ------------------------------------------------------------------ materials 64 / 65
def materials_case(total, bite=False):
    """Floor and back wall as `total - 4` quads, each with a Lambert material of its own
    colour; the last material lies on the back wall's centre quad. The first three quads take
    the constants of the box's White, Green and Red (textures 0..2), so the textures stay
    under their own limit."""
    s = Scene("materials_%d" % total)
    mats = configs.rgb_box_materials(s)
    box_without(s, mats, BACK_WALL, FLOOR)
    n = total - len(s.materials)
    nf = n // 2
    cells = [(add_floor_quad, c) for c in wall_cells(nf)] + [(add_back_quad, c) for c in wall_cells(n - nf)]
    for i, (add, cell) in enumerate(cells):
        rgb = [0.2 + 0.6 * ((i * k) % n) / n for k in (37, 11, 23)]
        if bite and i == n - 1:
            rgb = [0.95, 0.05, 0.5]
        add(s, cell, s.lambert(albedo=i if i < 3 else s.constant(rgb)))
    configs.cornell_camera(s, 1.0)
    past = total > TABLE_LIMIT
    # more than 64 primitives; a Lambert scene: the compact Colour instances
    return Case(s, N.SAMPLER_COLOUR, None, expectation(0 if past else 1, 0, 1, 0, 1), counts_of(s), (48, 48), past)


# ------------------------------------------------------------------- textures 64 / 65
def _image(seed, w, h, lo, hi, gray=False):
    rng = np.random.default_rng(seed)
    a = np.ones((h, w, 4))
    a[..., :3] = rng.uniform(lo, hi, (h, w, 1 if gray else 3))
    return a


def _normal_map(seed, w, h):
    rng = np.random.default_rng(seed)
    a = np.ones((h, w, 4))
    a[..., :2] = rng.uniform(0.3, 0.7, (h, w, 2))
    a[..., 2] = 0.9
    return a


def textures_case(total, spectral, bite=False):
    """The back wall as PBR quads whose slots point at textures of their own: constants,
    RGBA images and images whose R = G = B (stored as one double per texel); in the Spectral
    twin every albedo is an image with its SpectralImage. The last texture belongs to the
    centre quad: a constant albedo (Colour), the SpectralImage of its albedo (Spectral)."""
    s = Scene("textures_%s%d" % ("spectral_" if spectral else "", total))
    mats = spectral_box_materials(s) if spectral else configs.rgb_box_materials(s)
    box_without(s, mats, BACK_WALL)
    per = 5 if spectral else 4
    full, rest = divmod(total - len(s.textures), per)
    quads = []
    if rest:  # the remainder: a material with fewer slots, made first
        kw = {}
        for slot, make in zip(("albedo", "roughness", "metalness", "normal"),
                              (lambda: s.constant((0.6, 0.5, 0.3)), lambda: s.image(_image(900, 3, 2, 0.3, 0.7, gray=True)),
                               lambda: s.constant((0.2, 0.2, 0.2)), lambda: s.constant((0.5, 0.5, 1.0)))):
            if len(kw) < rest:
                kw[slot] = make()
        quads.append(s.pbr(**kw))
    for k in range(full):
        last = k == full - 1
        normal = s.image(_normal_map(100 + k, 4, 4)) if k % 2 == 0 else s.constant((0.5, 0.5, 1.0))
        rough = (s.constant((0.4, 0.4, 0.4)) if k % 3 == 0 else s.image(_image(200 + k, 3, 5, 0.2, 0.8, gray=True)) if k % 3 == 1
                 else s.image(_image(200 + k, 2, 3, 0.2, 0.8)))
        metal = s.image(_image(300 + k, 2, 2, 0.0, 0.6, gray=True)) if k % 2 else s.constant((0.1, 0.1, 0.1))
        if spectral:
            texels = _image(400 + k, 5, 3, 0.2, 0.9)
            if bite and last:
                texels[..., :3] = 1.0 - texels[..., :3]
            albedo = s.image(texels)
            quads.append(s.pbr(albedo, normal=normal, roughness=rough, metalness=metal, spectral=s.spectral_image(albedo)))
        else:
            if last:
                albedo = s.constant((0.1, 0.2, 0.9) if bite else (0.8, 0.6, 0.2))
            else:
                albedo = s.image(_image(400 + k, 5, 3, 0.2, 0.9)) if k % 2 else s.constant((0.3 + 0.04 * k, 0.5, 0.7 - 0.04 * k))
            quads.append(s.pbr(albedo, normal=normal, roughness=rough, metalness=metal))
    for cell, mat in zip(wall_cells(len(quads)), quads):
        add_back_quad(s, cell, mat)
    configs.cornell_camera(s, 1.0)
    past = total > TABLE_LIMIT
    return Case(s, N.SAMPLER_SPECTRAL if spectral else N.SAMPLER_COLOUR, None,
                expectation(0 if past else 2 if spectral else 1, 1, 1, 0, 0), counts_of(s), (48, 48), past)


# --------------------------------------------------------------------- lights 64 / 65
def light_triangles(n):
    """The ceiling light (33..66 x 33..66 at y = 99) cut into n triangles of the box's
    winding: n // 2 quads, the last triangle halved when n is odd."""
    out = []
    for a0, a1, b0, b1 in wall_cells(n // 2):
        x0, x1, z0, z1 = 33 + 33 * a0, 33 + 33 * a1, 33 + 33 * b0, 33 + 33 * b1
        out.append(((x0, 99, z0), (x1, 99, z0), (x1, 99, z1)))
        out.append(((x0, 99, z0), (x1, 99, z1), (x0, 99, z1)))
    if n % 2:
        a, b, c = out.pop()
        m = tuple((p + q) / 2 for p, q in zip(a, b))
        out += [(a, m, c), (m, b, c)]
    return out


def lights_case(num_tris, mixed, bite=False):
    """The ceiling light as num_tris emissive triangles; `mixed`: also two glass spheres and
    one emissive sphere, which follow the triangles in light_ref order (the emissive one last)."""
    s = Scene("lights_%d%s" % (num_tris, "_mixed" if mixed else ""))
    mats = configs.rgb_box_materials(s)
    box_without(s, mats, LIGHT)
    tris = light_triangles(num_tris)
    if bite and not mixed:
        tris[-1] = tuple((x, y - 6, z) for x, y, z in tris[-1])
    for a, b, c in tris:
        s.add_triangles([a], [b], [c], mats["light"])
    if mixed:
        glass = s.dielectric(ref_idx=1.5)
        s.add_sphere((28, 14, 40), 14, glass)
        s.add_sphere((72, 12, 60), 12, glass)
        s.add_sphere((55, 60, 55) if bite else (50, 60, 55), 6, mats["light"])
    configs.cornell_camera(s, 1.0)
    c = counts_of(s)
    past = c["num_lights"] > TABLE_LIMIT
    return Case(s, N.SAMPLER_COLOUR, None, expectation(0 if past else 1, 0, 0 if mixed else 1, 0, 0 if mixed else 1), c, (32, 32), past)


# --------------------------------------------------------------- SPD entries 384 / 385+
def _spectrum(n, kind, phase):
    """n (wavelength, value) entries over 380..750 nm: 'uniform' steps (the guessed
    interval), 'irregular' but sorted (the bisection), 'unsorted' (the scan)."""
    t = np.linspace(0.0, 1.0, n)
    if kind != "uniform":
        t = t ** 1.7
    wl = 380.0 + 370.0 * t
    val = 0.45 + 0.35 * np.sin(phase + wl / 41.0)
    if kind == "unsorted":
        wl[[n // 3, n // 3 + 1]] = wl[[n // 3 + 1, n // 3]]
    return wl.tolist(), val.tolist()


def spd_case(over, colour, bite=False):
    """Six tabulated spectra: the light (75 entries), the glass sphere's refractive index (20)
    and absorption (38), the Green and Red walls', and stored last the White walls', whose
    offset is 323 of 384 entries at the limit and 385 past it. `colour`: RGB albedos as well,
    for the Colour sampler, which reads none of the spectra."""
    s = Scene("spd_%s%s" % ("over" if over else "384", "_colour" if colour else ""))
    tabs = configs.spectral_tables()
    rgb = (lambda v: s.constant(v)) if colour else (lambda v: -1)
    light = s.diffuse_light(emit=rgb((15.0, 15.0, 15.0)),
                            spectral=s.spectral_spd(tabs["cie_wavelengths"], tabs["light_sources"]["cie_f1_daylight_fluorescent"]))
    refidx = s.spectral_tabulated(np.linspace(380, 750, 20).tolist(), np.linspace(1.52, 1.42, 20).tolist())
    glass = s.dielectric(ref_idx=1.5, spectral_refidx=refidx, spectral_absorb=s.spectral_neutral(0.01))
    ng, nr, nw = (140, 112, 61) if over else (100, 90, 61)
    green = s.lambert(albedo=rgb((0.0, 0.73, 0.0)), spectral=s.spectral_tabulated(*_spectrum(ng, "uniform", 0.3)))
    red = s.lambert(albedo=rgb((0.73, 0.0, 0.0)), spectral=s.spectral_tabulated(*_spectrum(nr, "unsorted", 2.1)))
    wl, val = _spectrum(nw, "irregular", 1.2)
    if bite and not colour:
        val = [0.5 * v for v in val]
    white = s.lambert(albedo=rgb((0.2, 0.3, 0.9) if bite and colour else (0.73, 0.73, 0.73)), spectral=s.spectral_tabulated(wl, val))
    assert s.textures[s.materials[white].spectral_tex].spd_offset == (385 if over else 323)
    configs.add_box(s, {"White": white, "Green": green, "Red": red, "light": light})
    s.add_sphere((50, 22, 50), 18, glass)
    configs.cornell_camera(s, 1.0)
    c = counts_of(s)
    past = c["num_spd"] > SPD_LIMIT
    return Case(s, N.SAMPLER_COLOUR if colour else N.SAMPLER_SPECTRAL, None, expectation(0 if past else 2, 1, 0, 1, 1), c, (32, 32), past)


# --------------------------------------------------------- background SPD 128 / 129
def background_case(n, inverted, bite=False):
    """The box without its back wall under the Spectral sampler, with a background SPD of n
    entries over 400..600 nm (every wavelength from 600 nm up reads the last entry);
    `inverted`: two neighbouring wavelengths exchanged, so the lookups scan."""
    s = Scene("background_%d%s" % (n, "_inverted" if inverted else ""))
    tabs = configs.spectral_tables()
    mats = spectral_box_materials(s, light=s.spectral_spd(tabs["cie_wavelengths"], tabs["light_sources"]["cie_f1_daylight_fluorescent"]))
    box_without(s, mats, BACK_WALL)
    configs.cornell_camera(s, 1.0)
    wl = np.linspace(400.0, 600.0, n)
    val = 0.3 + 0.2 * np.sin(wl / 17.0)
    if inverted:
        wl[[n // 2, n // 2 + 1]] = wl[[n // 2 + 1, n // 2]]
    if bite:
        val[-1] *= 3.0
    bg = (wl, val)
    past = n > BG_LIMIT
    return Case(s, N.SAMPLER_SPECTRAL, bg, expectation(0 if past else 2, 1, 1, 1, 1), counts_of(s, bg), (32, 32), past)


# ------------------------------------------------------------------ primitives 64 / 65
def prims_case(total, bite=False):
    """The box plus total - 12 spheres (Lambert and metal): four rows of 13 small ones on the
    floor and, for 65, a larger one above them, which is the last primitive."""
    s = Scene("prims_%d" % total)
    mats = configs.rgb_box_materials(s)
    configs.add_box(s, mats)
    metal = s.metal((0.8, 0.8, 0.9), 0.05)
    pick = [mats["White"], mats["Green"], metal, mats["Red"]]
    n = total - len(s.tris)
    for i in range(min(n, 52)):
        s.add_sphere((8 + 7 * (i % 13), 3, 20 + 20 * (i // 13)), 3, pick[i % 4])
    if n > 52:
        s.add_sphere((50, 30, 50), 12 if bite else 8, metal)
    configs.cornell_camera(s, 1.0)
    past = total > TABLE_LIMIT
    return Case(s, N.SAMPLER_COLOUR, None, expectation(1, 0 if past else 1, 0, 0, 0), counts_of(s), (32, 32), past)


# ------------------------------------------------------------------------ BVH in LDS
# Triangle counts on either side of make_tracer's 4096 bytes with the reference builder's
# tree (seed 12345), and the bytes they give; test_table_cases.py recomputes both from
# HostScene's node array and checks that neighbouring counts have no closer pair.
#        name: (extra triangles, sphere, num_inner * 128 + num_prims * 112)
BVH = {"bvh_tri_under": (18, False, 4000), "bvh_tri_over": (19, False, 4112),
       "bvh_sphere_under": (17, True, 4000), "bvh_sphere_over": (18, True, 4112)}


def bvh_scene(extra, sphere):
    """The box, `extra` small upright triangles on its floor and, with `sphere`, one sphere
    (the general k_trace2 instances instead of the triangle-only ones)."""
    s = Scene("bvh_%d%s" % (extra, "_sphere" if sphere else ""))
    mats = configs.rgb_box_materials(s)
    configs.add_box(s, mats)
    pick = [mats["Red"], mats["White"], mats["Green"]]
    for i in range(extra):
        x, z = 8.0 + 3.5 * i, 30.0 + 9.0 * (i % 5)
        s.add_triangles([(x, 0.5, z)], [(x + 3, 0.5, z)], [(x + 1.5, 14, z + 1)], pick[i % 3])
    if sphere:
        s.add_sphere((50, 40, 60), 12, mats["White"])
    configs.cornell_camera(s, 1.0)
    return s


def bvh_case(name):
    extra, sphere, nbytes = BVH[name]
    s = bvh_scene(extra, sphere)
    lds = int(nbytes <= BVH_LDS_BYTES)
    # the triangle-only scene is what the forward Colour k_shade's staged form takes the
    # primitives' LDS copy from (render_body); a traversal from global memory keeps its rays in
    # LDS only in the triangle-only instance
    return Case(s, N.SAMPLER_COLOUR, None, expectation(1, 1, 0 if sphere else 1, lds, 1 if lds or not sphere else 0,
                                                       prims_forward=None if sphere else 0), counts_of(s), (32, 32), False)


CASES = {
    "materials_64": lambda bite: materials_case(64, bite),
    "materials_65": lambda bite: materials_case(65, bite),
    "textures_64": lambda bite: textures_case(64, False, bite),
    "textures_65": lambda bite: textures_case(65, False, bite),
    "textures_spectral_64": lambda bite: textures_case(64, True, bite),
    "textures_spectral_65": lambda bite: textures_case(65, True, bite),
    "lights_64": lambda bite: lights_case(64, False, bite),
    "lights_65": lambda bite: lights_case(65, False, bite),
    "lights_mixed_65": lambda bite: lights_case(62, True, bite),
    "spd_384": lambda bite: spd_case(False, False, bite),
    "spd_over": lambda bite: spd_case(True, False, bite),           # also: at most 64 primitives, tables=0 prims=1
    "spd_over_colour": lambda bite: spd_case(True, True, bite),
    "background_128": lambda bite: background_case(128, False, bite),
    "background_128_inverted": lambda bite: background_case(128, True, bite),
    "background_129": lambda bite: background_case(129, False, bite),
    "background_129_inverted": lambda bite: background_case(129, True, bite),
    "prims_64": lambda bite: prims_case(64, bite),
    "prims_65": lambda bite: prims_case(65, bite),
    "bvh_tri_under": lambda bite: bvh_case("bvh_tri_under"),
    "bvh_tri_over": lambda bite: bvh_case("bvh_tri_over"),
    "bvh_sphere_under": lambda bite: bvh_case("bvh_sphere_under"),
    "bvh_sphere_over": lambda bite: bvh_case("bvh_sphere_over"),
}

# the descriptor counts each case is built for (None: not what the case is about)
INTENDED = {
    "materials_64": {"num_materials": 64}, "materials_65": {"num_materials": 65},
    "textures_64": {"num_textures": 64}, "textures_65": {"num_textures": 65},
    "textures_spectral_64": {"num_textures": 64}, "textures_spectral_65": {"num_textures": 65},
    "lights_64": {"num_lights": 64}, "lights_65": {"num_lights": 65}, "lights_mixed_65": {"num_lights": 65},
    "spd_384": {"num_spd": 384, "num_prims": 13}, "spd_over": {"num_spd": 446, "num_prims": 13},
    "spd_over_colour": {"num_spd": 446, "num_prims": 13},
    "background_128": {"num_bg": 128}, "background_128_inverted": {"num_bg": 128},
    "background_129": {"num_bg": 129}, "background_129_inverted": {"num_bg": 129},
    "prims_64": {"num_prims": 64}, "prims_65": {"num_prims": 65},
    "bvh_tri_under": {"num_prims": 30}, "bvh_tri_over": {"num_prims": 31},
    "bvh_sphere_under": {"num_prims": 30}, "bvh_sphere_over": {"num_prims": 31},
}


@functools.lru_cache(maxsize=None)
def build(name, bite=False):
    return CASES[name](bite)


def past_the_limit():
    return [n for n in CASES if build(n).past]


def log_line(err, prefix):
    """The one line of a render's pass log (stderr under IZPI_TUNE_PASS_LOG) that starts with
    `prefix`, as {field: int}: IZPI_SHADE_TABLES tables= prims= lds_bytes=, IZPI_TRACE_INSTANCE
    dist= tri= lds_bvh= ray_lds= q=."""
    lines = [l for l in err.splitlines() if l.startswith(prefix + " ")]
    assert len(lines) == 1, (prefix, lines)
    return {k: int(v) for k, v in (f.split("=") for f in lines[0].split()[1:])}


_REFS = {}


def oracle_ref(name, acc=N.ACC_RECURSIVE, bite=False):
    """The oracle's canvas (H, W, 4) and counters of a case, computed once per (case,
    accumulation, bite) and shared; callers leave the canvas unchanged."""
    key = (name, int(acc), bool(bite))
    if key not in _REFS:
        import ctypes as C

        from oracle import oracle as O
        case = build(name, bite)
        W, H = case.frame
        o = O.OracleScene(case.scene, aspect_override=W / H)
        req = N.RenderReq(width=W, height=H, spp=SPP, max_depth=MAX_DEPTH, sampler=case.sampler, seed=SEED,
                          abi_version=N.IZPI_ABI_VERSION, accumulation=acc)
        if case.bg is not None:
            wl, val = (np.ascontiguousarray(x, np.float64) for x in case.bg)
            req.num_bg_spd = len(wl)
            req.bg_spd_wavelengths = wl.ctypes.data_as(C.POINTER(C.c_double))
            req.bg_spd_values = val.ctypes.data_as(C.POINTER(C.c_double))
        canvas, stats = o.render(req, threads=16)
        o.close()
        canvas = canvas.reshape(H, W, 4)
        canvas.setflags(write=False)
        _REFS[key] = (canvas, stats)
    return _REFS[key]
