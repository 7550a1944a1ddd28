"""k_shade / k_tail with the scene's tables in global memory, and at the sizes that fill their
LDS copies to the last entry: the scenes of tests/table_cases.py, each at or one past one
limit (64 materials, textures, lights or primitives, 384 SPD entries, 128 background entries,
4096 bytes of BVH).

Every render runs under IZPI_TUNE_PASS_LOG and must
* report the IZPI_SHADE_TABLES / IZPI_TRACE_INSTANCE values its case expects (tables=0 past
  a table limit, 1 or 2 at it), so that a scene which stays under a limit, or a limit that
  moves, fails here instead of passing on the other path;
* equal the CPU oracle, which knows no staging: the image bit for bit and the counters
  (assert_parity), in both accumulations; past a limit also without k_tail, and for one
  Spectral case with the overflow record pool.
"""
import pytest

from izpi_amd import _native as N
from izpi_amd.renderer import GPURenderer
from tests import table_cases as T
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

ACCS = {"forward": N.ACC_FORWARD, "recursive": N.ACC_RECURSIVE}
TUNES = {"default": {}, "no_tail": {"flags": N.TUNE_NO_TAIL}, "record_pool": {"rec_dense": 1, "pool_div": 100000}}


def _params():
    out = []
    for name in T.CASES:
        tunes = ["default"] + (["no_tail"] if T.build(name).past else [])
        out += [(name, acc, tune) for tune in tunes for acc in ACCS]
        if name == "spd_over":  # the record pool holds the recursion's unwinding records (the forward form has none)
            out.append((name, "recursive", "record_pool"))
    return out


_RENDERER = {}


def renderer_of(name):
    """One renderer per case, kept while consecutive tests use the same case (accumulation
    and tuning change between its frames)."""
    if name not in _RENDERER:
        for r in _RENDERER.values():
            r.close()
        _RENDERER.clear()
        case = T.build(name)
        _RENDERER[name] = GPURenderer(case.scene, case.frame[0], case.frame[1], T.SPP, max_depth=T.MAX_DEPTH, sampler=case.sampler,
                                      spectral_background=case.bg, seed=T.SEED)
    return _RENDERER[name]


@pytest.fixture(scope="module", autouse=True)
def close_renderers():
    yield
    for r in _RENDERER.values():
        r.close()
    _RENDERER.clear()


@pytest.mark.parametrize("name,acc,tune", _params(), ids=lambda v: v)
def test_table_paths_bitwise(gpu, capfd, name, acc, tune):
    case = T.build(name)
    r = renderer_of(name)
    r.accumulation = ACCS[acc]
    kw = dict(TUNES[tune])
    r.tuning = N.tuning(**dict(kw, flags=kw.get("flags", 0) | N.TUNE_PASS_LOG))
    capfd.readouterr()
    img = r.render()
    err = capfd.readouterr().err
    tables, trace = T.log_line(err, "IZPI_SHADE_TABLES"), T.log_line(err, "IZPI_TRACE_INSTANCE")
    print("%s %s %s: IZPI_SHADE_TABLES %s IZPI_TRACE_INSTANCE %s" % (name, acc, tune, tables, trace))
    e = case.expect
    prims = e.get("prims_forward", e["prims"]) if acc == "forward" else e["prims"]
    assert (tables["tables"], tables["prims"]) == (e["tables"], prims), (tables, e)
    assert (tables["lds_bytes"] > 0) == bool(e["tables"] or prims), tables
    assert trace == {"dist": 1, "tri": e["tri"], "lds_bvh": e["lds_bvh"], "ray_lds": e["ray_lds"], "q": 0}, (trace, e)
    ref, ostats = T.oracle_ref(name, ACCS[acc])
    assert_parity(img, ref, r.stats, ostats)
    if name == "lights_mixed_65":
        assert r.stats["light_sph_tests"] > 0
    if tune == "record_pool":
        assert r.stats["pool_blocks"] > 0, r.stats  # records past the first level live in overflow blocks
