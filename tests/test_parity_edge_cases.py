"""Every case of tests/parity_edge_cases.py reaches the oracle branches it exists for: each
case is replayed alone, in a process of its own, against the oracle built with branch counters
(tools/oracle_coverage.py), and every edge it declares must have been taken at least MIN_REACH
times, so that no case rests on one lucky sample. No GPU: the device side of the same cases is
tests/test_gpu_parity_edges.py.

The edges are named by their place in the unoptimised build (condition K's fall-through or
jumping edge); test_edge_names_mean_what_they_say pins parity_edge_cases.EDGES' reading of
them on suite scenes that can take one side only.
"""
import importlib.util
import shutil
from pathlib import Path

import pytest

from tests import parity_edge_cases as E

_spec = importlib.util.spec_from_file_location("oracle_coverage", Path(__file__).resolve().parents[1] / "tools" / "oracle_coverage.py")
OC = importlib.util.module_from_spec(_spec)  # (tools/ is a directory of scripts, not a package)
_spec.loader.exec_module(OC)

# suite scenes that take one side of the tagged branches only: every UV inside its image; clear
# RGB glass; a spectral image without a grey texel; spectral glass with an absorption texture
ONE_SIDED = {
    "materials/textured_lambert": {
        0: [("tex-i-low", "clamped"), ("tex-j-low", "clamped"), ("tex-i-high", "clamped"), ("tex-j-high", "clamped"),
            ("go-int-range", "nan"), ("go-int-range", "too-big"), ("go-int-range", "too-small")],
        1: [("tex-i-low", "kept"), ("tex-j-low", "kept"), ("tex-i-high", "kept"), ("tex-j-high", "kept"),
            ("go-int-range", "number"), ("go-int-range", "below-2^63"), ("go-int-range", "in-range")]},
    "materials/rgb_glass_0": {
        0: [("diel-abs-zero", "x-set"), ("diel-abs-zero", "y-set"), ("diel-abs-zero", "z-set"), ("diel-beer", "beer-on")],
        1: [("diel-abs-zero", "x-zero"), ("diel-abs-zero", "y-zero"), ("diel-abs-zero", "z-zero"), ("diel-beer", "beer-off")]},
    "materials/rgb_glass_1": {
        0: [("diel-abs-zero", "y-set"), ("diel-abs-zero", "z-set"), ("diel-beer", "clear")],  # (0.12, 0.05, 0.02) and clear glass
        1: [("diel-abs-zero", "x-set"), ("diel-abs-zero", "x-zero"), ("diel-beer", "beer-on"), ("diel-beer", "absorbs"),
            ("diel-beer", "refracted"), ("diel-beer", "reflected")]},
    "materials/spectral_pbr_image": {
        0: [("grey-rule", "grey"), ("grey-rule", "rule-on"), ("stex-i-low", "clamped"), ("stex-j-high", "clamped"),
            ("stex-lambda-low", "below-380"), ("stex-lambda-high", "above-750"), ("stex-lambda-scan", "ran-out")],
        1: [("grey-rule", "rg-far"), ("grey-rule", "rule-off"), ("stex-i-low", "kept"), ("stex-j-high", "kept"),
            ("stex-lambda-low", "from-380"), ("stex-lambda-high", "to-750"), ("stex-lambda-scan", "next-bucket")]},
    "render/spectral_glass": {0: [("sdiel-abs-tex", "none")], 1: [("sdiel-abs-tex", "texture")]},
}


@pytest.fixture(scope="module")
def reached(tmp_path_factory):
    """{case: {edge: count}} of every edge case and ONE_SIDED scene, each replayed alone: the
    child processes run side by side, one counter directory each."""
    OC.build_instrumented()
    root = tmp_path_factory.mktemp("oracle_coverage")
    names = ["edges/" + c.name for c in E.CASES] + list(ONE_SIDED)
    procs = {n: OC.replay([n], root / n.replace("/", "_"), threads=2, wait=False) for n in names}
    out = {}
    for n, p in procs.items():
        assert p.wait() == 0, n
        out[n] = OC.edge_counts(OC.branches_of(root / n.replace("/", "_")))
    shutil.rmtree(root, ignore_errors=True)
    return out


def test_every_tag_is_known():
    """The oracle's tags and parity_edge_cases.EDGES name the same branches."""
    assert set(OC.tags()) == set(E.EDGES)


@pytest.mark.parametrize("scene", list(ONE_SIDED))
def test_edge_names_mean_what_they_say(reached, scene):
    got = reached[scene]
    for tag, meaning in ONE_SIDED[scene][0]:
        assert got[E.edge(tag, meaning)] == 0, (tag, meaning, got[E.edge(tag, meaning)])
    for tag, meaning in ONE_SIDED[scene][1]:
        assert got[E.edge(tag, meaning)] > 0, (tag, meaning)


def test_edges_cover_every_condition(reached):
    """EDGES names both edges of every condition gcov reports on a tagged line, once each."""
    some = next(iter(reached.values()))
    for tag, names in E.EDGES.items():
        want = sorted(k.split(":")[1] for k in some if k.startswith(tag + ":"))
        assert sorted(names.values()) == want, (tag, want)


@pytest.mark.parametrize("case", E.CASES, ids=[c.name for c in E.CASES])
def test_case_reaches_its_edges(reached, case):
    got = reached["edges/" + case.name]
    assert case.reaches
    short = {e: got.get(e) for e in case.reaches if not got.get(e, 0) >= E.MIN_REACH}
    assert not short, short


def test_cases_take_every_tagged_edge():
    """Together the cases declare every edge of every tagged branch: after them no tagged
    branch is left one-sided."""
    declared = {e for c in E.CASES for e in c.reaches}
    missing = [E.edge(t, m) for t, names in E.EDGES.items() for m in names if E.edge(t, m) not in declared]
    assert not missing, missing
