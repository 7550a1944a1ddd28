"""pixel_map.h (izpi_amd/csrc), the one home of the packed-pixel rule, the canvas slot and the
samplers' mean, without a GPU: the stand-alone program tests/pixel_map_check.cpp, built by the
host compiler under AddressSanitizer and UBSan and run as a child process, and the places that
once restated the rule."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"


def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "pixel_map_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "pixel_map_check.cpp"),
                    str(CSRC / "host_scene.cpp"), str(CSRC / "scene_pack.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])  # a sanitizer report ends the program
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok", lines[-5:]
    ran = {ln.split()[1].rstrip(":") for ln in lines if ln.startswith("case ")}
    assert ran == {"frame", "subset_row0", "subset_no_row0", "list_1x1_row0", "list_1x1_no_row0", "mean", "view"}, ran
    frame = next(ln for ln in lines if ln.startswith("case frame:"))
    assert frame == "case frame: 1200 pixels, 40 in sample row 0", frame
    differ = re.match(r"case mean: (\d+) of (\d+) \(c, n\) differ", next(ln for ln in lines if ln.startswith("case mean:")))
    assert differ and 0 < int(differ.group(1)) < int(differ.group(2)), lines


def test_the_rule_is_written_once():
    """The index arithmetic has one definition site, and the copies it replaced are gone."""
    sources = {p.name: p.read_text() for p in CSRC.iterdir() if p.suffix in (".h", ".hip", ".cpp")}
    assert [n for n, s in sources.items() if "tile_px" in s] == ["pixel_map.h"]
    for gone in ("packed_target", "pixel_xy", "noise_params(", "session_counts", "load_pixel", "pixel_n("):
        assert not [n for n, s in sources.items() if gone in s], gone
    assert "IZPI_SAMPLER_COLOUR : req->sampler" not in sources["izpi_gpu.hip"]  # accum_params carries the request's sampler
    assert "#include <hip" not in sources["pixel_map.h"]
