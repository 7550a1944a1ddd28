"""The device on the branches only tests/parity_edge_cases.py reaches: texel indices clamped
from every side and from int() overflow (image_rgb, image_index + image_at, tex_spectral_image
behind go_int), SpectralImage's grey and bright rules at their limits, RGB absorption vectors
with zero components and computeBeerLambert against them, spectral glass without an absorption
texture, and as components the table ends of SampleWavelength / GetCIEValues, a spectral image's
bucket search outside 380..750 nm and for NaN, and rays in a triangle's plane.

Every render case: the canvas equals the oracle's bit for bit and the counters are equal
(assert_parity), in both accumulations, with the scene's tables, primitives and tree staged in
LDS and with IZPI_TUNE_NO_PRIM_LDS | IZPI_TUNE_NO_LDS_BVH (the pass log must say so); the
texel-clamp cases also on a GPU-built tree, against the oracle traversing that tree.
tests/test_parity_edge_cases.py shows on the CPU that each case takes its branches.
"""
import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd.renderer import GPURenderer
from oracle import oracle as O
from tests import parity_edge_cases as E
from tests.table_cases import log_line
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

ACCS = {"recursive": N.ACC_RECURSIVE, "forward": N.ACC_FORWARD}
FORMS = {"lds": 0, "global": N.TUNE_NO_PRIM_LDS | N.TUNE_NO_LDS_BVH}
RENDERS = [c for c in E.CASES if c.component is None]


def _params():
    out = []
    for c in RENDERS:
        for tree in ["reference"] + (["gpu"] if c.clamp else []):
            out += [(c.name, tree, acc, form) for acc in ACCS for form in FORMS]
    return out


_RENDERER, _REFS = {}, {}


def renderer_of(name, tree):
    """One renderer per (case, tree), kept while consecutive tests use it (accumulation and
    tuning change between its frames)."""
    if (name, tree) not in _RENDERER:
        for r in _RENDERER.values():
            r.close()
        _RENDERER.clear()
        c = E.BY_NAME[name]
        _RENDERER[name, tree] = GPURenderer(c.build(), c.size[0], c.size[1], c.spp, sampler=c.sampler, bvh=tree)
    return _RENDERER[name, tree]


def oracle_ref(name, tree, acc, r):
    """The oracle's canvas and counters, once per (case, tree, accumulation); on the GPU-built
    tree of renderer r the oracle traverses that tree."""
    key = (name, tree, acc)
    if key not in _REFS:
        c = E.BY_NAME[name]
        W, H = c.size
        o = O.OracleScene(c.build(), aspect_override=W / H)
        if tree == "gpu":
            o.set_bvh(r.bvh_nodes(), r.host._bvh_keep[1])
        req = N.RenderReq(width=W, height=H, spp=c.spp, max_depth=50, sampler=c.sampler, seed=12345,
                          abi_version=N.IZPI_ABI_VERSION, accumulation=ACCS[acc])
        canvas, stats = o.render(req, threads=16)
        o.close()
        canvas = canvas.reshape(H, W, 4)
        canvas.setflags(write=False)
        _REFS[key] = (canvas, stats)
    return _REFS[key]


@pytest.fixture(scope="module", autouse=True)
def close_renderers():
    yield
    for r in _RENDERER.values():
        r.close()
    _RENDERER.clear()
    _REFS.clear()


@pytest.mark.parametrize("name,tree,acc,form", _params(), ids=lambda v: v)
def test_edge_case_bitwise(gpu, capfd, name, tree, acc, form):
    r = renderer_of(name, tree)
    r.accumulation = ACCS[acc]
    r.tuning = N.tuning(flags=FORMS[form] | N.TUNE_PASS_LOG)
    capfd.readouterr()
    img = r.render()
    err = capfd.readouterr().err
    tables, trace = log_line(err, "IZPI_SHADE_TABLES"), log_line(err, "IZPI_TRACE_INSTANCE")
    print("%s %s %s %s: IZPI_SHADE_TABLES %s IZPI_TRACE_INSTANCE %s" % (name, tree, acc, form, tables, trace))
    assert tables["tables"] >= 1, tables  # materials, textures and slots in LDS in both forms
    if form == "global":
        assert tables["prims"] == 0 and trace["lds_bvh"] == 0, (tables, trace)
    elif tree == "reference":
        assert trace["lds_bvh"] == 1, trace
    ref, ostats = oracle_ref(name, tree, acc, r)
    assert_parity(img, ref, r.stats, ostats)
    assert not np.isnan(img).any() and float(img[..., :3].max()) > 0


@pytest.mark.parametrize("name", [c.name for c in E.CASES if c.component is not None])
def test_edge_component_bitwise(gpu, name):
    comp = E.BY_NAME[name].component
    want = comp.oracle(O)
    r = GPURenderer(comp.scene(), 8, 8, 1, sampler=E.BY_NAME[name].sampler)
    got = comp.device(r)
    r.close()
    assert got.shape == want.shape
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))[:8].tolist()
