"""The DISPLACE geometry operator on the CPU: the Python restatement (tests/displace_ref.py)
against the reference's known answers, izpi_host_displace against the restatement bit for
bit, the level cap, and scene ingestion of DISPLACE triangles. No GPU."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import ingest
from tests import displace_cases as DC
from tests import displace_ref as DR

KATS = json.loads((Path(__file__).resolve().parent / "golden" / "displacement_kats.json").read_text())
ORDERS = {"per_triangle": N.DISPLACE_PER_TRIANGLE, "mesh": N.DISPLACE_MESH}


def _kat_tri(d, material=None):
    return (tuple(map(float, d["vertex0"])), tuple(map(float, d["vertex1"])), tuple(map(float, d["vertex2"])),
            tuple(map(float, d["u"])), tuple(map(float, d["v"])), material)


# ---------------------------------------------------------------- 1. the restatement
def test_restatement_tessellate_known_answer():
    for case in KATS["tessellate"]:
        assert DR.tessellate(_kat_tri(case["input"])) == [_kat_tri(w) for w in case["want"]], case["name"]


def test_restatement_apply_tessellation_known_counts():
    kat = KATS["apply_tessellation"]
    tex = DR.Constant((0.0, 0.0, kat["flat_z"]))
    for case in kat["cases"]:
        got = DR.apply_tessellation([_kat_tri(kat["input"])], 1.0 / (case["res_u"] - 1), 1.0 / (case["res_v"] - 1), tex,
                                    kat["min"], kat["max"], kat["threshold"])
        assert len(got) == case["want_triangles"], case["name"]


def test_restatement_apply_displacement_known_answers():
    for case in KATS["apply_displacement"]:
        got = DR.apply_displacement([_kat_tri(case["input"])], DR.Constant(case["texture"]), case["min"], case["max"])
        assert got == [_kat_tri(case["want"])], case["name"]


@pytest.mark.parametrize("name", sorted(DC.FLAT_COUNTS))
def test_flat_maps_reach_the_known_counts_through_the_public_entry(name):
    """ApplyDisplacementMap uses 4/(res-1) where the reference's test used 1/(res-1): the
    same three counts are reached on 9x9, 13x5 and 5x13 flat maps."""
    rows, make_map, dmin, dmax = DC.CASES[name]
    want, counts = DC.reference(name, "per_triangle")
    assert len(want) == counts[0] == DC.FLAT_COUNTS[name]
    out, got_counts = ingest.displace(DC.tris(rows), make_map(), dmin, dmax)
    assert len(out) == DC.FLAT_COUNTS[name] and got_counts.tolist() == [DC.FLAT_COUNTS[name]]


# ------------------------------------------------- 2. the host twin == the restatement
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_host_twin_equals_the_restatement_bitwise(name, order):
    rows, make_map, dmin, dmax = DC.CASES[name]
    want, want_counts = DC.reference(name, order)
    got, counts = ingest.displace(DC.tris(rows, material=3), make_map(), dmin, dmax, ORDERS[order])
    print(name, order, "triangles", len(got), "counts", counts.tolist())
    DC.assert_same_triangles(got, want)
    assert counts.tolist() == want_counts
    only, counts = ingest.displace(DC.tris(rows, material=3), make_map(), dmin, dmax, ORDERS[order], count_only=True)
    assert len(only) == 0 and counts.tolist() == want_counts


def test_cases_cover_what_they_are_meant_to():
    """The smooth T finishes triangles at several levels; the quad's two orders differ; the
    equal-u triangle gives NaN vertices."""
    t, _ = DC.reference("smooth_T", "per_triangle")
    assert len(t) > 100
    uv = t["uv"]
    area = np.abs((uv[:, 2] - uv[:, 0]) * (uv[:, 5] - uv[:, 1]) - (uv[:, 4] - uv[:, 0]) * (uv[:, 3] - uv[:, 1]))
    assert len(np.unique(np.round(np.log2(area)))) >= 3   # a level divides the UV area by 4: several depths
    a, ca = DC.reference("smooth_quad", "per_triangle")
    b, cb = DC.reference("smooth_quad", "mesh")
    assert ca == cb and len(a) == len(b) == sum(ca) and min(ca) > 0
    assert a.tobytes() != b.tobytes() and sorted(a.tobytes()[i:i + 128] for i in range(0, a.nbytes, 128)) == \
        sorted(b.tobytes()[i:i + 128] for i in range(0, b.nbytes, 128))
    n, _ = DC.reference("equal_u", "per_triangle")
    assert len(n) > 0 and np.isnan(n["v0"]).all() and np.isnan(n["v2"]).all()


def test_cap_too_small_reports_the_needed_count():
    rows, make_map, dmin, dmax = DC.CASES["smooth_quad"]
    t, rgba = DC.tris(rows), make_map()
    want, _ = DC.reference("smooth_quad", "mesh")
    out = np.zeros(5, DC.TRI_DTYPE)
    n = C.c_uint64()
    rc = N.lib().izpi_host_displace(t.ctypes.data, len(t), rgba.ctypes.data_as(N.c_double_p), 33, 33, dmin, dmax,
                                    N.DISPLACE_MESH, out.ctypes.data, len(out), C.byref(n), None, None)
    assert rc == N.IZPI_ERR_INVALID and n.value == len(want)
    assert not out["v0"].any()
    rc = N.lib().izpi_host_displace(t.ctypes.data, len(t), rgba.ctypes.data_as(N.c_double_p), 0, 33, dmin, dmax,
                                    N.DISPLACE_MESH, None, 0, C.byref(n), None, None)
    assert rc == N.IZPI_ERR_INVALID and b"width and height" in N.lib().izpi_host_last_error()
    rc = N.lib().izpi_host_displace(t.ctypes.data, len(t), rgba.ctypes.data_as(N.c_double_p), 33, 33, dmin, dmax, 7,
                                    None, 0, C.byref(n), None, None)
    assert rc == N.IZPI_ERR_INVALID and b"order" in N.lib().izpi_host_last_error()


# ------------------------------------------------------------------- 3. the level cap
def test_level_cap():
    """A step of 1 between neighbouring texels with |max - min| = 3 never passes the
    variation test (1 * 3 > 2): the reference would subdivide until UVs collide. Here the
    call fails after IZPI_DISPLACE_MAX_LEVELS levels; with max 2 the step passes (1 * 2 <= 2)."""
    t, rgba = DC.tris(DC.T), DC.step_map()
    with pytest.raises(RuntimeError, match=r"status %d.*IZPI_DISPLACE_MAX_LEVELS \(16\)" % N.IZPI_ERR_UNSUPPORTED):
        ingest.displace(t, rgba, 0.0, 3.0)
    with pytest.raises(RuntimeError, match="IZPI_DISPLACE_MAX_LEVELS"):
        ingest.displace(t, rgba, 0.0, 3.0, N.DISPLACE_MESH)
    with pytest.raises(DR.LevelCap):  # the restatement agrees (a cap of 8 keeps it quick)
        DR.per_triangle(DC.to_ref(t), rgba.tolist(), 0.0, 3.0, max_levels=8)
    out, counts = ingest.displace(t, rgba, 0.0, 2.0)
    want, want_counts = DR.per_triangle(DC.to_ref(t), rgba.tolist(), 0.0, 2.0)
    assert len(out) == 4 and counts.tolist() == want_counts == [4]
    DC.assert_same_triangles(out, DC.from_ref(want))


# -------------------------------------------------------------------- 4. ingestion
def _scene(**kw):
    s = ingest.ProtoScene(DC.scene_text(**kw).encode())
    return s


def test_ingestion_runs_displace_triangles_in_place():
    s = _scene()
    assert s.info()["num_displacement_maps"] == 1 and s.displacement_files() == [DC.MAP_FILE]
    rgba = DC.smooth_map(33, 33)
    s.set_displacement_map(DC.MAP_FILE, rgba)
    si = s.to_input()
    got = DC.input_tris(si)
    want, counts = DC.reference("smooth_quad", "per_triangle")
    want = want.copy()
    want["material"] = 0
    print("ingested", len(got), "triangles; per DISPLACE source", counts)
    assert len(got) == counts[0] + 1 + counts[1] and si.struct.num_spheres == 1
    DC.assert_same_triangles(got[:counts[0]], want[:counts[0]])
    plain = DC.tris([DC.PLAIN])
    DC.assert_same_triangles(got[counts[0]:counts[0] + 1], plain)
    DC.assert_same_triangles(got[counts[0] + 1:], want[counts[0]:])
    assert si.struct.num_materials == 1 and s.material_names() == ["ground"]


def test_ingested_scene_renders_as_the_restated_scene():
    """The CPU oracle's image of the ingested .pbtxt == its image of the same scene built
    programmatically from the restatement's triangles (reference BVH), bit for bit."""
    from oracle import oracle as O
    s = _scene(light=True)
    s.set_displacement_map(DC.MAP_FILE, DC.smooth_map(33, 33))
    req = N.RenderReq(width=32, height=32, spp=2, max_depth=50, sampler=N.SAMPLER_COLOUR, seed=12345)
    req.background[:] = (0.7, 0.8, 1.0)
    ia, sa = O.OracleScene(s, aspect_override=1.0).render(req, threads=4)
    ib, sb = O.OracleScene(DC.restated_scene(light=True), aspect_override=1.0).render(req, threads=4)
    assert ia.tobytes() == ib.tobytes() and sa["rays"] == sb["rays"]
    assert (ia.reshape(-1, 4)[:, :3] != req.background[:]).any(axis=1).mean() > 0.3  # the surface is in view


def test_ingestion_map_errors():
    s = _scene()
    with pytest.raises(RuntimeError, match="triangle DISPLACE operator: displacement map %s not found" % DC.MAP_FILE):
        s.to_input()  # declared, not handed over
    s = _scene(map_name="other.exr")
    s.set_displacement_map("other.exr", DC.smooth_map(33, 33))
    with pytest.raises(RuntimeError, match="triangle DISPLACE operator: displacement map other.exr not found"):
        s.to_input()  # handed over, not declared
    s = _scene(declare=False)
    assert s.displacement_files() == []
    s.set_displacement_map(DC.MAP_FILE, DC.smooth_map(33, 33))
    with pytest.raises(RuntimeError, match="displacement map %s not found" % DC.MAP_FILE):
        s.to_input()
    s = _scene()
    with pytest.raises(RuntimeError, match="width and height"):
        s.set_displacement_map(DC.MAP_FILE, np.zeros((0, 4, 4)))


def test_ingestion_level_cap_error_reaches_the_caller():
    s = _scene(dmin=0.0, dmax=3.0)
    s.set_displacement_map(DC.MAP_FILE, DC.step_map())
    with pytest.raises(RuntimeError, match=r"status %d.*DISPLACE.*IZPI_DISPLACE_MAX_LEVELS" % N.IZPI_ERR_UNSUPPORTED):
        s.to_input()


def test_wire_round_trip_keeps_the_displace_fields():
    s = _scene()
    wire = s.to_wire()
    b = ingest.ProtoScene(wire, binary=True)
    assert b.to_wire() == wire
    assert b.displacement_files() == [DC.MAP_FILE] and b.info()["num_displacement_maps"] == 1
    rgba = DC.smooth_map(33, 33)
    s.set_displacement_map(DC.MAP_FILE, rgba)
    b.set_displacement_map(DC.MAP_FILE, rgba)
    assert DC.input_tris(b.to_input()).tobytes() == DC.input_tris(s.to_input()).tobytes()
