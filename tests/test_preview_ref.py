"""The checker of the preview samplers (tests/preview_ref.py) pinned on its own, without a
GPU: its LCG against the oracle's, segment.Belongs and the sphere rule on hand cases, the
epsilon quirk of HitableSlice.HitEdge's second traversal, and the sampler names and values
the front ends take (sampler.go:13-28)."""
import json
import math
from pathlib import Path

import izpi_amd
from izpi_amd import _native as N
from oracle import oracle as O
from tests import preview_ref as PR

KATS = json.loads((Path(__file__).parent / "golden" / "reference_kats.json").read_text())


def test_python_lcg_is_the_oracles():
    for seed in (12345, 0, 0xFFFFFFFF, PR.splitmix64(12345) & 0xFFFFFFFF):
        vals, states = O.lcg(seed, 64)
        pv, ps = PR.lcg(seed, 64)
        assert pv == list(vals) and ps == [int(s) for s in states]
    vals, states = PR.lcg(12345, 4)
    assert states == KATS["lcg_seed_12345"]["states"] and vals == KATS["lcg_seed_12345"]["values"]


def test_belongs_hand_cases():
    a, b = (0.0, 0.0, 0.0), (2.0, 0.0, 0.0)
    assert PR.belongs(a, b, (1.0, 0.0, 0.0))          # the midpoint of the side
    assert PR.belongs(a, b, a) and PR.belongs(a, b, b)  # a vertex (unit(0) is NaN, and NaN >= .005 is false)
    assert not PR.belongs(a, b, (1.0, 0.01, 0.0))     # 1% off the side: |sin| = 0.01 >= .005
    assert PR.belongs(a, b, (1.0, 0.004, 0.0))        # within the allowed angle
    assert not PR.belongs(a, b, (2.5, 0.0, 0.0))      # colinear, beyond the segment's end
    assert not PR.belongs(a, b, (-0.5, 0.0, 0.0))     # colinear, before its start
    tri = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    assert PR.triangle_edge(*tri, (0.5, 0.5, 0.0)) and not PR.triangle_edge(*tri, (0.25, 0.25, 0.0))


def test_sphere_edge_rule():
    origin, center = (0.0, 0.0, 0.0), (0.0, 0.0, -2.0)
    # the pole facing the ray: a and b are opposed, theta = Pi, not an edge
    assert not PR.sphere_edge(origin, center, (0.0, 0.0, -1.5))
    # a grazing hit: the tangent point, where a is perpendicular to b (theta = Pi/2)
    r, d = 0.5, 2.0
    z = -(d - r * r / d)
    x = r * math.sqrt(1.0 - (r / d) ** 2)
    assert PR.sphere_edge(origin, center, (x, 0.0, z))
    # 0.1 rad is the ring's width: 0.2 rad in from the tangent point is no edge any more
    ang = math.acos(r / d) - 0.2
    assert not PR.sphere_edge(origin, center, (r * math.sin(ang), 0.0, -d + r * math.cos(ang)))
    assert PR.EDGE_ANGLE == float.fromhex("0x1.abb94edddc6b2p+0") and PR.HALF_PI == math.pi / 2


def test_epsilon_quirk_of_the_second_traversal():
    assert PR.EPSILON == math.nextafter(1.0, 2.0) - 1.0
    for t, kept in ((1.5, True), (3.999, True), (4.0, False), (8.0, False)):
        tmax = PR.second_pass_tmax(t)
        assert (tmax > t) == kept
        assert PR.sphere_root_accepted(t, tmax) == kept  # Sphere.Hit: temp < tMax, strictly
    # (a triangle survives either way: Triangle.Hit rejects only t > tMax)


def test_sampler_names_and_values():
    assert izpi_amd.SAMPLERS == PR.SAMPLER_MAP == {"colour": 2, "normal": 1, "wireframe": 3, "albedo": 4, "spectral": 5}
    assert (N.SAMPLER_NORMAL, N.SAMPLER_COLOUR, N.SAMPLER_WIREFRAME, N.SAMPLER_ALBEDO, N.SAMPLER_SPECTRAL) == (1, 2, 3, 4, 5)
    assert N.IZPI_ABI_VERSION == 4 and tuple(N.RenderReq().ink) == (0.0, 0.0, 0.0)


def test_unit_scene_reference_has_the_quirks():
    """The hand-built scene does what it was built for, on the reference alone: ink from the
    near sphere's ring, and second traversals that lose the far sphere."""
    ref = PR.PreviewRef(PR.unit_scene(), 40, 30, 3)
    _, what = ref.wireframe_samples((0.1, 0.2, 0.3), (1.0, 0.5, 0.25))
    near = [k for k, w in enumerate(what) if w == "sph+edge"]
    lost = [k for k, w in enumerate(what) if w == "lost"]
    assert near and all(ref.first["t"][k] < 4.0 for k in near)
    assert lost and all(ref.first["t"][k] >= 4.0 and (int(ref.first["prim_ref"][k]) >> 31) == N.PRIM_SPHERE for k in lost)
    ref.close()
