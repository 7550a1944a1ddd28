"""The scenes of tests/table_cases.py are what they claim to be, established on the CPU:
* the host scene's descriptor has exactly the intended table sizes, and the mixed lights
  case a sphere at light index 64;
* the expected IZPI_SHADE_TABLES / IZPI_TRACE_INSTANCE values follow from those sizes by
  render_body's and make_tracer's rules, restated here;
* the BVH cases lie on either side of 4096 bytes, one triangle apart;
* every past-the-limit case bites: changing only its highest-index entry changes the
  oracle's image, so a path reads that entry and a wrong lookup on the GPU would show;
* the oracle renders every case quickly.
"""
import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd.scene import HostScene
from tests import table_cases as T

NAMES = list(T.CASES)


@pytest.fixture(scope="module")
def hosts():
    made = {}

    def get(name):
        if name not in made:
            case = T.build(name)
            made[name] = HostScene(case.scene, aspect_override=case.frame[0] / case.frame[1])
        return made[name]
    yield get
    for h in made.values():
        h.close()


@pytest.mark.parametrize("name", NAMES)
def test_descriptor_has_the_intended_counts(hosts, name):
    case, d = T.build(name), hosts(name).desc
    got = {"num_materials": d.num_materials, "num_textures": d.num_textures, "num_lights": d.num_lights,
           "num_spd": d.num_spd, "num_prims": d.num_prims, "num_bg": 0 if case.bg is None else len(case.bg[0])}
    assert got == case.counts
    for k, v in T.INTENDED[name].items():
        assert got[k] == v, (k, got[k], v)
    if case.bg is not None:
        assert len(case.bg[0]) == len(case.bg[1])
        inversions = int((np.diff(case.bg[0]) < 0).sum())
        assert inversions == (1 if name.endswith("inverted") else 0)
    # one limit per case: every other table stays under its own
    over = [k for k, lim in (("num_materials", T.TABLE_LIMIT), ("num_textures", T.TABLE_LIMIT), ("num_lights", T.TABLE_LIMIT),
                             ("num_spd", T.SPD_LIMIT), ("num_bg", T.BG_LIMIT)) if got[k] > lim]
    assert over == ([k for k in T.INTENDED[name] if k != "num_prims"] if case.past and not name.startswith("prims") else [])


def test_mixed_lights_have_a_sphere_past_the_limit(hosts):
    refs = hosts("lights_mixed_65").light_refs()
    kinds = [int(r) >> 31 for r in refs]  # IZPI_PRIM_REF: the kind in the top bit
    assert len(refs) == 65 and kinds[:62] == [N.PRIM_TRIANGLE] * 62 and kinds[62:] == [N.PRIM_SPHERE] * 3
    # the emissive sphere (the scene's last) is light 64; the glass ones 62 and 63
    case = T.build("lights_mixed_65")
    assert (int(refs[64]) & 0x7FFFFFFF) == len(case.scene.spheres) - 1
    assert case.scene.materials[int(case.scene.spheres["material"][-1])].kind == N.MAT_DIFFUSE_LIGHT


@pytest.mark.parametrize("name", NAMES)
def test_expected_paths_follow_from_the_counts(hosts, name):
    """render_body's and make_tracer's rules on the descriptor's sizes give the case's
    expected line values (the GPU test then reads them from the library itself)."""
    case, host = T.build(name), hosts(name)
    c, e = case.counts, case.expect
    fits = (c["num_materials"] <= T.TABLE_LIMIT and c["num_textures"] <= T.TABLE_LIMIT and c["num_lights"] <= T.TABLE_LIMIT
            and c["num_spd"] <= T.SPD_LIMIT and c["num_bg"] <= T.BG_LIMIT)
    spectral_tables = case.sampler == N.SAMPLER_SPECTRAL or c["num_spd"] > 0
    assert e["tables"] == (0 if not fits else 2 if spectral_tables else 1)
    assert e["prims"] == int(c["num_prims"] <= T.TABLE_LIMIT)
    assert case.past == (not fits or name == "prims_65")
    tri = int(len(case.scene.spheres) == 0)
    lds = int(T.bvh_lds_bytes(host) <= T.BVH_LDS_BYTES)
    assert (e["tri"], e["lds_bvh"]) == (tri, lds)
    reads_uv = any(t.kind in (N.TEX_IMAGE, N.TEX_SPECTRAL_IMAGE) for t in case.scene.textures)
    assert e["ray_lds"] == int(bool(lds or (tri and not reads_uv)))  # (no sphere of these scenes moves)
    # forward Colour k_shade's staged form takes the primitives' place in LDS in Lambert /
    # light scenes of triangles whose Colour tables are staged
    lambert_only = all(m.kind in (N.MAT_LAMBERT, N.MAT_DIFFUSE_LIGHT) for m in case.scene.materials)
    gives_up = case.sampler == N.SAMPLER_COLOUR and lambert_only and tri and e["tables"] == 1
    assert e.get("prims_forward", e["prims"]) == (0 if gives_up else e["prims"])


def test_bvh_cases_straddle_the_limit_one_triangle_apart(hosts):
    for kind in ("tri", "sphere"):
        (ku, su, bu), (ko, so, bo) = T.BVH["bvh_%s_under" % kind], T.BVH["bvh_%s_over" % kind]
        assert su == so and ko == ku + 1
        assert T.bvh_lds_bytes(hosts("bvh_%s_under" % kind)) == bu <= T.BVH_LDS_BYTES
        assert T.bvh_lds_bytes(hosts("bvh_%s_over" % kind)) == bo > T.BVH_LDS_BYTES
        assert bo - bu <= T.PRIM_BYTES + T.INNER_BYTES  # one primitive and at most one inner node more


@pytest.mark.parametrize("name", NAMES)
def test_oracle_renders_the_case_quickly(name):
    img, stats = T.oracle_ref(name)
    assert np.isfinite(img).all() and (img[..., :3] > 0).any()
    assert stats["seconds"] < 2.0, stats["seconds"]
    if name == "lights_mixed_65":
        assert stats["light_sph_tests"] > 0


@pytest.mark.parametrize("name", T.past_the_limit())
def test_case_bites(name):
    """Only the highest-index entry differs between the case and its biting twin (the sizes
    are the same), and the oracle's image differs: some path reads that entry."""
    a, b = T.build(name), T.build(name, bite=True)
    assert a.counts == b.counts and a.expect == b.expect
    img, _ = T.oracle_ref(name)
    bit, _ = T.oracle_ref(name, bite=True)
    changed = int((img.view(np.uint64) != bit.view(np.uint64)).any(axis=-1).sum())
    assert changed >= 8, "only %d pixels read the last entry" % changed
