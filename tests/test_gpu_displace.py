"""The DISPLACE geometry operator on the GPU (izpi_gpu_displace, izpi_amd/csrc/displace.hip):
bitwise against the Python restatement and the host twin, in both output orders; the level
cap; and a displaced scene end to end (ingestion on the device, GPU-built BVH4, frame)
against the CPU oracle and the preview reference."""
import ctypes as C

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import configs, ingest
from izpi_amd.renderer import GPURenderer
from oracle import oracle as O
from tests import displace_cases as DC
from tests import preview_ref as PR
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

ORDERS = {"per_triangle": N.DISPLACE_PER_TRIANGLE, "mesh": N.DISPLACE_MESH}
PAPER, INK = (0.7, 0.8, 1.0), (1.0, 0.5, 0.25)


@pytest.fixture(scope="module")
def ctx(gpu):
    h = C.c_void_p()
    assert N.lib().izpi_gpu_open(gpu, C.byref(h)) == 0
    yield h
    N.lib().izpi_gpu_close(h)


# -------------------------------------------------- 5. the device == the restatement
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_device_equals_the_restatement_bitwise(ctx, name, order):
    rows, make_map, dmin, dmax = DC.CASES[name]
    want, want_counts = DC.reference(name, order)
    timing = {}
    got, counts = ingest.displace(DC.tris(rows, material=3), make_map(), dmin, dmax, ORDERS[order], ctx=ctx, timing=timing)
    print(name, order, "triangles", len(got), "device ms", timing["ms"])
    DC.assert_same_triangles(got, want)
    assert counts.tolist() == want_counts
    assert timing["ms"] > 0
    only, counts = ingest.displace(DC.tris(rows, material=3), make_map(), dmin, dmax, ORDERS[order], ctx=ctx,
                                   count_only=True)
    assert len(only) == 0 and counts.tolist() == want_counts


# ------------------------------------------------ 6. blocks, scan tiles, uneven counts
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("res", [33, 129])
def test_grid_plane_equals_the_host_twin(ctx, res, order):
    """1152 source triangles (a 24 x 24-quad plane, uv = position: more than one block and
    scan tile from level 1 on) over the smooth map at +-8.

    On the 33 x 33 map a quad is smaller than a texel and the diagonal of every child runs
    along the map's gentler diagonal, so every source finishes at level 1 with 4 triangles
    (4608 in all). The 129 x 129 map is there for the uneven counts: 4 to 52 per source,
    31641 in all on the host twin, sources finishing at levels 1 to 3 side by side."""
    t, rgba = DC.tris(DC.grid_plane(24), material=2), DC.smooth_map(res, res)
    assert len(t) == 1152
    want, want_counts = ingest.displace(t, rgba, -8.0, 8.0, ORDERS[order])
    print(res, order, "host twin:", len(want), "triangles, per source", int(want_counts.min()), "..",
          int(want_counts.max()))
    assert len(want) < 200000
    if res == 129:
        assert want_counts.min() == 4 and want_counts.max() > 16 and len(np.unique(want_counts)) > 3
    got, counts = ingest.displace(t, rgba, -8.0, 8.0, ORDERS[order], ctx=ctx)
    DC.assert_same_triangles(got, want)
    assert got.tobytes() == want.tobytes()  # no NaN here: equal to the byte
    assert counts.tolist() == want_counts.tolist()


def test_cap_too_small_reports_the_needed_count(ctx):
    rows, make_map, dmin, dmax = DC.CASES["smooth_quad"]
    t, rgba = DC.tris(rows), make_map()
    want, _ = DC.reference("smooth_quad", "mesh")
    out = np.zeros(5, DC.TRI_DTYPE)
    n = C.c_uint64()
    rc = N.lib().izpi_gpu_displace(ctx, t.ctypes.data, len(t), rgba.ctypes.data_as(N.c_double_p), 33, 33, dmin, dmax,
                                   N.DISPLACE_MESH, out.ctypes.data, len(out), C.byref(n), None, None)
    assert rc == N.IZPI_ERR_INVALID and n.value == len(want)
    assert not out["v0"].any()


# ------------------------------------------------------------------ 7. the level cap
def test_level_cap_matches_the_host_twin_and_the_context_still_renders(gpu):
    L = N.lib()
    t, rgba = DC.tris(DC.T), DC.step_map()
    r = GPURenderer(configs.cornell_rgb(), 8, 8, 1)
    n = C.c_uint64()
    args = (t.ctypes.data, len(t), rgba.ctypes.data_as(N.c_double_p), 9, 9, 0.0, 3.0, N.DISPLACE_PER_TRIANGLE, None, 0,
            C.byref(n), None, None)
    host_rc = L.izpi_host_displace(*args)
    host_msg = L.izpi_host_last_error().decode()
    gpu_rc = L.izpi_gpu_displace(r.ctx, *args)
    gpu_msg = L.izpi_gpu_last_error(r.ctx).decode()
    assert gpu_rc == host_rc == N.IZPI_ERR_UNSUPPORTED
    assert gpu_msg == host_msg and "IZPI_DISPLACE_MAX_LEVELS (16)" in gpu_msg
    out, counts = ingest.displace(t, rgba, 0.0, 2.0, ctx=r.ctx)
    assert len(out) == 4 and counts.tolist() == [4]
    img = r.render()
    assert r.stats["samples"] == 64 and np.isfinite(img).all()
    r.close()


# --------------------------------------------------------------------- 8. end to end
def _ingested(displacer=None, light=False):
    s = ingest.ProtoScene(DC.scene_text(light=light).encode())
    s.set_displacement_map(DC.MAP_FILE, DC.smooth_map(33, 33))
    if displacer is not None:
        s.set_displacer(displacer)
    return s


def test_ingestion_on_the_device_equals_the_host_path(ctx):
    host = DC.input_tris(_ingested().to_input())
    s = ingest.ProtoScene(DC.scene_text().encode())
    s.set_displacement_map(DC.MAP_FILE, DC.smooth_map(33, 33))
    dev = DC.input_tris(s.to_input(displacer=ctx))
    assert dev.tobytes() == host.tobytes()
    assert DC.input_tris(s.to_input()).tobytes() == host.tobytes()  # and back on the host


def test_displaced_scene_colour_frame_equals_the_oracle(ctx):
    """File -> displaced mesh (device) -> GPU-built BVH4 -> frame, against the CPU oracle over
    the scene built from the restatement's triangles, on the same tree."""
    W = H = 32
    r = GPURenderer(_ingested(ctx, light=True), W, H, 4, background=PAPER, bvh="gpu")
    img = r.render()
    o = O.OracleScene(DC.restated_scene(light=True), aspect_override=1.0)
    o.set_bvh(r.bvh_nodes(), r.host._bvh_keep[1])
    req = N.RenderReq(width=W, height=H, spp=4, max_depth=50, sampler=N.SAMPLER_COLOUR, seed=12345)
    req.background[:] = PAPER
    ref, ostats = o.render(req, threads=16)
    assert_parity(img, ref.reshape(H, W, 4), r.stats, ostats)
    assert (img.reshape(-1, 4)[:, :3] != PAPER).any(axis=1).mean() > 0.3  # the surface is in view
    r.close()


def test_displaced_scene_normal_frame_equals_the_preview_reference(ctx):
    W = H = 32
    want = PR.PreviewRef(DC.restated_scene(light=True), W, H, 4).render(N.SAMPLER_NORMAL, PAPER, INK)
    r = GPURenderer(_ingested(ctx, light=True), W, H, 4, sampler=N.SAMPLER_NORMAL, background=PAPER, ink=INK, bvh="gpu")
    img = r.render()
    assert r.stats["rays"] == r.stats["samples"] == W * H * 4
    assert img.tobytes() == want.tobytes(), "max |diff| %g" % np.nanmax(np.abs(img - want))
    r.close()
