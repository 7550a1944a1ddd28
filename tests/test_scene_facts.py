"""The two scene facts k_trace2's primitive step is specialised on, as pack_scene records them
(izpi_amd/csrc/scene_pack.cpp): the largest leaf (PackedScene::leaf_max, DevScene::leaf_max) and
whether any traced ray can be a path-length ray (no_pathlen). Checked without a GPU by a
stand-alone program under AddressSanitizer and UBSan, on small scenes with hand-made trees."""
import subprocess
from pathlib import Path

import pytest

from izpi_amd import _native as N

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"

# case -> (largest leaf, no_pathlen)
WANT = {
    "root_leaf_1": (1, 1), "root_leaf_2": (2, 1), "root_leaf_3": (3, 1), "root_leaf_4": (4, 1), "root_leaf_7": (7, 1),
    "leaves_3_1": (3, 1), "leaves_1_4_2": (4, 1), "leaves_3_3_3_3": (3, 1), "leaves_2_1_2_4": (4, 1),
    # a dielectric in the material table counts whether a primitive uses it or not (the flag is the table's)
    "glass_in_table_unused": (3, 0), "glass_used": (2, 0),
    "host_built_12": (None, 1),  # the host builder's tree: whatever its largest leaf is
}


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = tmp_path_factory.mktemp("scene_facts") / "scene_facts_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(ROOT / "tests" / "scene_facts_check.cpp"), str(CSRC / "scene_pack.cpp"),
                    str(CSRC / "host_scene.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-3000:]  # a sanitizer report ends the program
    out = {}
    for line in run.stdout.splitlines():
        name, rc, fields = line.split("|")
        out[name] = (int(rc), {k: int(v) for k, v in (f.split("=") for f in fields.split())})
    return out


def test_every_case_ran(rows):
    assert sorted(rows) == sorted(WANT)


@pytest.mark.parametrize("name", sorted(WANT))
def test_leaf_max_and_no_pathlen(rows, name):
    rc, f = rows[name]
    leaf_max, no_pathlen = WANT[name]
    assert rc == N.IZPI_OK
    assert f["leaf_max"] == f["walked"] and 1 <= f["leaf_max"] <= 7
    if leaf_max is not None:
        assert f["leaf_max"] == leaf_max
    assert f["no_pathlen"] == no_pathlen


def test_both_sides_of_the_three_primitive_bound():
    """The cases hold leaves on both sides of the bound the tracer tests (leaf_max <= 3)."""
    sizes = {v[0] for v in WANT.values() if v[0] is not None}
    assert {3, 4} <= sizes and min(sizes) < 3 and max(sizes) > 4
