"""slab_rule.h (izpi_amd/csrc), the one home of RayAABB4's per-slot rules: the scalar twin and the
sorted rule k_trace2's global-memory node step runs (near and far planes picked by the ray's sign,
no sort of the two products), without a GPU: the stand-alone program tests/slab_rule_check.cpp, built by
the host compiler under AddressSanitizer and UBSan with -ffp-contract=off and run as a child
process. It also checks the upload fact ordered_bounds on pack_scene's output and that a leaf
lane's last 16-B load ends inside the node block's allocation."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"


def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "slab_rule_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "slab_rule_check.cpp"),
                    str(CSRC / "host_scene.cpp"), str(CSRC / "scene_pack.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])  # a sanitizer report ends the program
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok", lines[-5:]
    ran = {ln.split()[1].rstrip(":") for ln in lines if ln.startswith("case ")}
    want = {"octant%d" % i for i in range(8)} | {"special%d" % i for i in range(8)} | {"trees_1", "trees_6", "trees_40"}
    want |= {"alloc_tree1", "alloc_tree6", "alloc_tree40", "alloc_c3_like", "alloc_quantised", "alloc_one_leaf"}
    assert ran == want, ran ^ want
    for ln in lines:
        m = re.match(r"case (octant|special)\d: (\d+) pairs, (\d+) fast, (\d+) hit", ln)
        if m:  # at least 10^5 pairs per octant, every ray fast, hits and misses both present
            pairs, fast, hit = (int(m.group(k)) for k in (2, 3, 4))
            assert pairs >= 100000 and fast == pairs and 0 < hit < pairs, ln


def test_the_rule_is_written_once():
    """The scalar twin and the fast-ray predicate have one definition site, a header the host
    compiler builds; the kernels' sorted test takes tn and tf from the header's functions."""
    sources = {p.name: p.read_text() for p in CSRC.iterdir() if p.suffix in (".h", ".hip", ".cpp")}
    assert [n for n, s in sources.items() if re.search(r"\bbool slab\(", s)] == ["slab_rule.h"]
    assert [n for n, s in sources.items() if re.search(r"\bbool ray_fast_ok\(", s)] == ["slab_rule.h"]
    assert "#include <hip" not in sources["slab_rule.h"]
    assert "slab_sorted_near(" in sources["izpi_dev.h"] and "slab_near_index(" in sources["trace.hip"]
