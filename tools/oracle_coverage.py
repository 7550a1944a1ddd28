#!/usr/bin/env python3
"""Which branches of the CPU oracle's hot path do the parity tests' scenes execute?

The GPU suite compares the device with oracle/izpi_oracle.cpp bit for bit, which checks the
branches the compared scenes take and no others. This tool measures them on the CPU (no GPU
is used): it builds the oracle with `--coverage -fprofile-update=atomic -O0` into
oracle/_build/coverage/ (liboracle.so is never replaced), replays the oracle side of the
suite's render, trace and component cases against that library in a child Python process
(the counters are written when it exits), runs `gcov -b` and prints every hot-path branch
that was not taken in both directions, with its source line and its `// [edge: NAME]` tag.

    python tools/oracle_coverage.py                  # the suite without tests/parity_edge_cases.py, then with it
    python tools/oracle_coverage.py --set suite      # one table
    python tools/oracle_coverage.py --list           # the replayed cases
    python tools/oracle_coverage.py --case NAME ...  # these cases alone

The hot path: textures, spectra, materials, primitives, traversal, lights and samplers
(HOT_SECTIONS); scene construction (COLD_FUNCTIONS) and the builder restatements are left out.
profiles/r23a/oracle_branch_coverage.md is this tool's output on the commit that added it.
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

ORACLE_DIR = ROOT / "oracle"
SOURCE = ORACLE_DIR / "izpi_oracle.cpp"
COV_DIR = ORACLE_DIR / "_build" / "coverage"
COV_LIB = COV_DIR / "liboracle_cov.so"
# the oracle's own flags (oracle/Makefile) with -O0 and the counters; no exception edges, which
# gcov would list as branches of every call
CXXFLAGS = ["-O0", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-fno-exceptions",
            "--coverage", "-fprofile-update=atomic"]

# [first line matching, line matching the end): the hot path
HOT_SECTIONS = [(r"^// Go's int\(float64\)", r"^// -+ fastrandom\.go"),
                (r"^// -+ onb\.go", r"^// --- Go sort\.Slice"),
                (r"^struct HitableSlice ", r"^// -+ camera\.go"),
                (r"^  Vec3 randomInUnitDisc", r"^\}  // namespace orc")]
# functions inside those sections that run once per scene: from the matching line to the
# closing brace at the same indentation
COLD_FUNCTIONS = [r"^  void Build\(int w, int h", r"^  static Triangle\* NewWithUV", r"^  AABB BoundingBox\(\) const override \{$",
                  r"^static float conservativeFloat32M"]
TAG_RE = re.compile(r"// \[edge: ([a-z0-9-]+)\]")
# threads of one oracle render in the child (the counters are atomic: a few threads per child
# and several children side by side are faster than many threads on the same counters)
THREADS = int(os.environ.get("ORACLE_COVERAGE_THREADS", "16"))


# ------------------------------------------------------------------ the instrumented build
def build_instrumented():
    """oracle/_build/coverage/liboracle_cov.so, rebuilt when a source is newer."""
    deps = [SOURCE, ORACLE_DIR / "go_math_ref.h", ORACLE_DIR / "cie_tables_ref.h"] + sorted((ROOT / "include").glob("*.h"))
    if COV_LIB.exists() and all(d.stat().st_mtime <= COV_LIB.stat().st_mtime for d in deps):
        return COV_LIB
    COV_DIR.mkdir(parents=True, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    obj = COV_DIR / "izpi_oracle.o"
    subprocess.run([cxx] + CXXFLAGS + ["-c", "-o", str(obj), str(SOURCE)], check=True, cwd=COV_DIR)
    tmp = COV_DIR / ("liboracle_cov.so.tmp%d" % os.getpid())
    subprocess.run([cxx, "-shared", "-pthread", "--coverage", "-o", str(tmp), str(obj)], check=True, cwd=COV_DIR)
    os.replace(tmp, COV_LIB)
    return COV_LIB


# ----------------------------------------------------------------------- the replayed cases
def _render(O, scene, W, H, spp, sampler, acc=None, max_depth=50, bg=None):
    import numpy as np
    from izpi_amd import _native as N
    o = O.OracleScene(scene, aspect_override=W / H)
    kw = dict(width=W, height=H, spp=spp, max_depth=max_depth, sampler=sampler, seed=12345)
    if acc is not None:
        kw.update(abi_version=N.IZPI_ABI_VERSION, accumulation=acc)
    req = N.RenderReq(**kw)
    if bg is not None:
        wl, val = (np.ascontiguousarray(x, np.float64) for x in bg)
        req.num_bg_spd = len(wl)
        req.bg_spd_wavelengths, req.bg_spd_values = O.dptr(wl), O.dptr(val)
    o.render(req, threads=THREADS)
    o.close()


def _trace(O, scene, rays):
    o = O.OracleScene(scene, aspect_override=1.0)
    o.trace(rays)
    o.close()


def _axis_rays():
    """test_gpu_parity.test_axis_aligned_rays_trace_bitwise's ray set."""
    import numpy as np
    rng = np.random.default_rng(7)
    rays = []
    for i in range(4096):
        org = rng.uniform(-10, 110, 3)
        if i % 3 == 0:
            org = np.round(org)
        d = np.zeros(3)
        d[i % 3] = 1.0 if (i // 3) % 2 else -1.0
        if i % 5 == 0:
            d[(i + 1) % 3] = rng.uniform(-1, 1)
        rays.append(list(org) + list(d) + [0.001, 1e300])
    return np.ascontiguousarray(rays, np.float64)


def _spectral_components(O):
    """test_gpu_parity.test_spectral_sampling_device_bitwise's inputs through SampleWavelength and
    GetCIEValues, and test_spectral_tabulated_lookup_device_bitwise's first table."""
    import numpy as np
    from izpi_amd import configs
    rng = np.random.default_rng(11)
    tabs = configs.spectral_tables()
    wl = np.asarray(tabs["cie_wavelengths"], np.float64)
    cum = np.cumsum(np.asarray(tabs["cie_y"], np.float64)) / float(tabs["cie_y_integral"])
    rand = np.concatenate([rng.random(20000), [0.0, 0.5, np.nextafter(1.0, 0.0)], cum, np.nextafter(cum, 0), np.nextafter(cum, 2)])
    rand = rand.clip(0, np.nextafter(1.0, 0.0))
    lams = np.concatenate([rng.uniform(370, 790, 20000), wl, np.nextafter(wl, 0), np.nextafter(wl, 1e4), [379.0, 380.0, 780.0, 800.0]])
    a, b, o3 = C.c_double(), C.c_double(), (C.c_double * 3)()
    L = O.lib()
    for v in rand:
        L.oracle_sample_wavelength(float(v), C.byref(a), C.byref(b))
    for v in lams:
        L.oracle_cie_values(float(v), o3)
    vl = np.ascontiguousarray(np.random.default_rng(3).random(len(wl)))
    for v in np.concatenate([wl, rng.uniform(375, 785, 2000), [300.0, 900.0]]):
        L.oracle_spd_tabulated_value(O.dptr(wl), O.dptr(vl), len(wl), float(v))


def _table_lookup_scene(table):
    """test_gpu_parity.test_spectral_table_lookups_bitwise's scene and background SPD."""
    import numpy as np
    from izpi_amd import configs
    from izpi_amd.scene import Scene
    tabs = configs.spectral_tables()
    wl = list(tabs["cie_wavelengths"])
    light = list(tabs["light_sources"]["cie_f1_daylight_fluorescent"])
    if table == "duplicates":
        wl_l = wl[:10] + [wl[10]] * 3 + wl[13:]
        ref = ([380, 500, 500, 500, 620, 750], [1.55, 1.5, 1.52, 1.49, 1.47, 1.45])
        bg = (np.array([380.0, 450, 450, 600, 780]), np.array([0.1, 0.2, 0.3, 0.05, 0.4]))
    elif table == "unsorted":
        wl_l = wl[:20] + [wl[25], wl[21], wl[22], wl[23], wl[24], wl[20]] + wl[26:]
        ref = ([380, 620, 500, 560, 750], [1.55, 1.47, 1.5, 1.48, 1.45])
        bg = (np.array([380.0, 600, 450, 780]), np.array([0.1, 0.2, 0.3, 0.4]))
    else:
        wl_l, ref, bg = wl, ([550], [1.5]), (np.array([550.0]), np.array([0.25]))
    s = Scene("spd_tables")
    mats = {"Green": s.lambert(spectral=s.spectral_gaussian(0.9, 540, 40)),
            "Red": s.lambert(spectral=s.spectral_tabulated([400, 600, 600, 700], [0.1, 0.8, 0.6, 0.9])),
            "White": s.lambert(spectral=s.spectral_neutral(0.73)),
            "light": s.diffuse_light(spectral=s.spectral_spd(wl_l, light))}
    glass = s.dielectric(spectral_refidx=s.spectral_tabulated(*ref), spectral_absorb=s.spectral_neutral(0.01))
    configs.add_box(s, mats)
    s.add_sphere((50, 30, 50), 15, glass)
    s.set_camera((50, 50, -120), (50, 50, 50), (0, 1, 0), 35, 1.0, 0, 10, 0, 1, 1.0)
    return s, bg


def _zero_sign_scene(albedo):
    """test_gpu_parity_materials.test_zero_radiance_unwinding_signs_bitwise's scene; albedo None:
    the spectral one's."""
    from izpi_amd import configs
    from izpi_amd.scene import Scene
    if albedo is not None:
        s = Scene("zero_signs")
        configs.add_box(s, configs.rgb_box_materials(s))
        s.add_sphere((35, 20, 45), 18, s.metal(albedo, 0.05))
        s.add_sphere((70, 15, 30), 12, s.metal((0.8, -0.3, 0.6), 0.0))
        s.add_sphere((55, 60, 40), 10, s.dielectric(ref_idx=1.5))
    else:
        tabs = configs.spectral_tables()
        s = Scene("spectral_zero_signs")
        mats = {"Green": s.lambert(spectral=s.spectral_gaussian(0.9, 540, 40)),
                "Red": s.lambert(spectral=s.spectral_gaussian(0.9, 640, 40)),
                "light": s.diffuse_light(spectral=s.spectral_spd(tabs["cie_wavelengths"],
                                                                 tabs["light_sources"]["cie_f1_daylight_fluorescent"])),
                "White": s.pbr(s.constant((0.7, 0.7, 0.7)), spectral=s.spectral_gaussian(-0.8, 560, 80))}
        configs.add_box(s, mats)
        s.add_sphere((35, 20, 45), 18, s.pbr(s.constant((0.2, 0.5, 0.3)), spectral=s.spectral_gaussian(-0.5, 500, 50)))
        s.add_sphere((70, 15, 30), 12, s.dielectric(spectral_refidx=s.spectral_tabulated(configs._REFIDX_WL, configs._REFIDX_V)))
    configs.cornell_camera(s, 1.0)
    return s


def suite_cases():
    """name -> f(O): the oracle side of the suite's render, trace and component cases, at the
    tests' own sizes."""
    import numpy as np

    from izpi_amd import _native as N
    from izpi_amd import configs
    from tests import table_cases as T
    from tests import test_gpu_parity_materials as M
    from tests import test_gpu_shade_instances as SI
    from tests.test_gpu_parity import random_rays
    from tests.test_oracle_kats import tbn_kat_scene
    COL, SPE = N.SAMPLER_COLOUR, N.SAMPLER_SPECTRAL
    cases = {}

    def render(name, build, W, H, spp, sampler, **kw):
        cases[name] = lambda O: _render(O, build(), W, H, spp, sampler, **kw)

    c1 = configs.configs()["C1"]
    render("render/c1", c1.build, c1.width, c1.height, c1.spp, c1.sampler)
    render("render/dragon", lambda: configs.cornell_dragon(1.0, n=60), 64, 64, 8, COL)
    render("render/spectral_glass", configs.cornell_glass_spectral, 48, 48, 8, SPE)
    render("render/pbr", lambda: configs.cornell_pbr(1.5, res=64), 60, 40, 8, COL)
    for md in (0, 1, 3):
        render("render/max_depth_%d" % md, configs.cornell_rgb, 40, 40, 4, COL, max_depth=md)
    for coloured in (False, True):
        render("materials/rgb_glass_%d" % coloured, lambda c=coloured: M.rgb_glass_box(c), 48, 48, 8, COL)
    for alb in (True, False, "image"):
        render("materials/spectral_pbr_%s" % alb, lambda a=alb: M.spectral_pbr_box(a), 48, 48, 8, SPE)
    render("materials/textured_lambert", M.textured_lambert_box, 48, 48, 8, COL)
    render("materials/isotropic_colour", lambda: M.isotropic_box(False), 48, 48, 8, COL)
    render("materials/isotropic_spectral", lambda: M.isotropic_box(True), 48, 48, 8, SPE)
    render("materials/pbr_storage", M.pbr_storage_box, 48, 48, 8, COL)

    def thin_lens(scene):
        scene.set_camera((50, 50, -140), (50, 50, 0), (0, 1, 0), 40, 1.0, 4.0, 190.0, 0.25, 0.75)
        return scene
    render("materials/thin_lens_colour", lambda: thin_lens(configs.cornell_dragon(1.0, n=30)), 40, 40, 6, COL)
    render("materials/thin_lens_spectral", lambda: thin_lens(configs.cornell_glass_spectral()), 40, 40, 6, SPE)
    for k, alb in enumerate([(-0.5, 0.7, -0.0), (0.9, float("inf"), 0.4), (-0.0, -0.0, -0.0)]):
        render("materials/zero_signs_%d" % k, lambda a=alb: _zero_sign_scene(a), 48, 48, 8, COL)  # (the test: 16 spp)
    render("materials/zero_signs_spectral", lambda: _zero_sign_scene(None), 48, 48, 8, SPE)
    for table in ("duplicates", "unsorted", "single"):
        cases["render/spd_tables_" + table] = lambda O, t=table: _render(O, _table_lookup_scene(t)[0], 40, 40, 8, SPE,
                                                                         bg=_table_lookup_scene(t)[1])
    for name, build in SI.SCENES.items():
        s, a = name.split("/")[:2]
        render("instances/" + name, build, SI.W, SI.H, SI.SPP, SI.SAMPLERS[s], acc=SI.ACCS[a], max_depth=SI.MAX_DEPTH)
    for name in T.CASES:
        cases["tables/" + name] = lambda O, n=name: T.oracle_ref(n)
    trace_scenes = {"box": configs.cornell_rgb, "dragon": lambda: configs.cornell_dragon(1.0, n=40),
                    "glass": configs.cornell_glass_spectral, "pbr": configs.cornell_pbr}
    for which, build in trace_scenes.items():
        cases["trace/random_" + which] = lambda O, b=build: _trace(O, b(), random_rays(20000))
    cases["trace/axis_aligned"] = lambda O: _trace(O, configs.cornell_dragon(1.0, n=40), _axis_rays())

    def tbn(O):
        s, rays = tbn_kat_scene()
        r8 = np.zeros((len(rays), 8))
        r8[:, :6], r8[:, 6], r8[:, 7] = rays, 0.001, np.finfo(np.float64).max
        _trace(O, s, r8)
    cases["trace/tbn_kats"] = tbn
    cases["component/spectral"] = _spectral_components
    return cases


def edge_cases():
    from tests import parity_edge_cases as E
    cases = {}
    for c in E.CASES:
        if c.component is not None:
            cases["edges/" + c.name] = c.component.oracle
        else:
            cases["edges/" + c.name] = lambda O, c=c: _render(O, c.build(), c.size[0], c.size[1], c.spp, c.sampler)
    return cases


def all_cases():
    cases = suite_cases()
    cases.update(edge_cases())
    return cases


def _child(names):
    from oracle import oracle as O
    O.use_library(COV_LIB)
    cases = all_cases()
    for n in names:
        cases[n](O)


def replay(names, run_dir, threads=None, wait=True):
    """Run the cases `names` in one child process; its counters land in run_dir/ when it exits.
    wait=False: the started process (several may run side by side, one run_dir each)."""
    run_dir = Path(run_dir)
    if run_dir.exists():
        shutil.rmtree(run_dir)
    run_dir.mkdir(parents=True)
    build_instrumented()
    env = dict(os.environ, GCOV_PREFIX=str(run_dir), GCOV_PREFIX_STRIP="99")
    if threads:
        env["ORACLE_COVERAGE_THREADS"] = str(threads)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child"] + list(names)
    if not wait:
        return subprocess.Popen(cmd, env=env, cwd=ROOT)
    subprocess.run(cmd, check=True, env=env, cwd=ROOT)
    return run_dir


# -------------------------------------------------------------------------- reading gcov
def branches_of(run_dir):
    """{line: [(count, falls_through)]} of izpi_oracle.cpp from the counters in run_dir."""
    run_dir = Path(run_dir)
    shutil.copy(COV_DIR / "izpi_oracle.gcno", run_dir / "izpi_oracle.gcno")
    out = subprocess.run(["gcov", "-b", "-c", "--json-format", "--stdout", "izpi_oracle.gcda"], check=True, cwd=run_dir,
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    res = {}
    for f in json.loads(out)["files"]:
        if Path(f["file"]).name != SOURCE.name:
            continue
        for ln in f["lines"]:
            br = [(b["count"], b["fallthrough"]) for b in ln["branches"] if not b["throw"]]
            if br:
                old = res.get(ln["line_number"])  # (a line listed once per function instance)
                res[ln["line_number"]] = br if old is None else [(a[0] + b[0], a[1]) for a, b in zip(old, br)]
    return res


def source_lines():
    return SOURCE.read_text().split("\n")


def tags(src=None):
    """{tag: line number} of the oracle's `// [edge: NAME]` comments."""
    out = {}
    for i, l in enumerate(src or source_lines(), 1):
        m = TAG_RE.search(l)
        if m:
            assert m.group(1) not in out, m.group(1)
            out[m.group(1)] = i
    return out


def hot_lines(src=None):
    src = src or source_lines()

    def find(rx, start=0):
        for i in range(start, len(src)):
            if re.search(rx, src[i]):
                return i
        raise KeyError(rx)
    hot = set()
    for a, b in HOT_SECTIONS:
        i = find(a)
        hot.update(range(i + 1, find(b, i) + 1))
    for rx in COLD_FUNCTIONS:
        i = 0
        while True:
            try:
                i = find(rx, i)
            except KeyError:
                break
            ind = len(src[i]) - len(src[i].lstrip())
            j = i if src[i].rstrip().endswith("}") and src[i].count("{") == src[i].count("}") else find("^" + " " * ind + r"\}", i + 1)
            hot.difference_update(range(i + 1, j + 2))
            i = j + 1
    return hot


def edge_counts(br):
    """{"TAG:cK+": count, "TAG:cK-": count} over the tagged lines: condition K's fall-through
    and jumping edge (two gcov branches per condition, in source order)."""
    out = {}
    for tag, line in tags().items():
        b = br.get(line, [])
        assert len(b) % 2 == 0, (tag, b)
        for k in range(len(b) // 2):
            pair = b[2 * k:2 * k + 2]
            assert pair[0][1] != pair[1][1], (tag, pair)
            for cnt, ft in pair:
                out["%s:c%d%s" % (tag, k, "+" if ft else "-")] = cnt
    return out


def one_sided(br):
    """Rows (line, tag, per-condition (falls through, jumps) counts, text) of the hot-path lines
    with a branch that was not taken in both directions."""
    src = source_lines()
    hot = hot_lines(src)
    by_line = {v: k for k, v in tags(src).items()}
    unreachable = {i for i, l in enumerate(src, 1) if "[edge-unreachable:" in l}
    rows = []
    for line in sorted(br):
        b = br[line]
        if line not in hot or all(c > 0 for c, _ in b):
            continue
        conds = []
        for k in range(0, len(b) - 1, 2):
            ft = sum(c for c, f in b[k:k + 2] if f)
            conds.append((ft, sum(c for c, f in b[k:k + 2] if not f)))
        text = re.sub(r"\s*// \[edge.*", "", src[line - 1]).strip()
        rows.append((line, by_line.get(line, "(dead)" if line in unreachable else ""), conds, text))
    return rows


def print_table(rows, out=sys.stdout):
    print("| line | tag | falls through / jumps, per condition | source |", file=out)
    print("|---|---|---|---|", file=out)
    for line, tag, conds, text in rows:
        text = text if len(text) <= 90 else text[:87] + "..."
        print("| %d | %s | %s | `%s` |" % (line, tag, " ; ".join("%d / %d" % c for c in conds), text.replace("|", "\\|")), file=out)


def measure(names, label):
    t = time.time()
    run = replay(names, COV_DIR / ("run_" + label))
    br = branches_of(run)
    rows = one_sided(br)
    hot = hot_lines()
    total = sum(len(b) for l, b in br.items() if l in hot)
    taken = sum(1 for l, b in br.items() if l in hot for c, _ in b if c > 0)
    print("\n## %s: %d cases, %d of %d hot-path branch outcomes taken, %d lines one-sided, %.0f s\n" %
          (label, len(names), taken, total, len(rows), time.time() - t))
    print_table(rows)
    tagged = set(tags().values())
    left = [r for r in rows if r[0] in tagged]
    print("\ntagged lines not taken both ways: %s" % (", ".join("%s (%d)" % (r[1], r[0]) for r in left) or "none"))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--set", choices=["suite", "all", "both"], default="both")
    ap.add_argument("--case", nargs="+", help="replay these cases alone")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--child", nargs="*", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return _child(a.child)
    if a.list:
        print("\n".join(all_cases()))
        return
    if a.case:
        measure(a.case, "cases")
        return
    if a.set in ("suite", "both"):
        measure(list(suite_cases()), "suite")
    if a.set in ("all", "both"):
        measure(list(all_cases()), "suite_and_edge_cases")


if __name__ == "__main__":
    main()
