"""plan_workspace (izpi_amd/csrc/render_plan.cpp): the host-only half of the render call's
setup, checked without a GPU in a stand-alone program under AddressSanitizer and UBSan.

The expected rows are not the planner's own: they were made by transcribing the sizing
arithmetic the render call had before the planner existed (commit 06db42c: render_body's
sizing block, preview_body's, carve_state and carve_preview) into a throwaway program with
`avail` as a parameter, run on the cases of tests/render_plan_check.cpp. The C3 rows agree
with DESIGN.md §2.2 (268M entries, 12.9 GB of results, 51 GB of compact records, 16.8M blocks)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"

PLANS = {
    "colour_fwd_512":
        "chunk=512 slots=268435456 rec_dense=50 rec_pool=0 pool_div=16 pool_blocks=0 pool_shift=0 D=5 compact=0 thr_planes=3 sides=2 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=12884901888 recs=0 pool=0 ring=0 running=25165824 state=57982058496",
    "colour_rec_compact_512":
        "chunk=512 slots=266808574 rec_dense=8 rec_pool=42 pool_div=16 pool_blocks=16777216 pool_shift=16 D=3 compact=1 thr_planes=0 sides=2 time=0 blk=1 cold=0 uv=0 tminmax=0 samples=12884901888 recs=51227246208 pool=16911433728 ring=67108864 running=25165824 state=46958309376",
    "spectral_rec_256":
        "chunk=256 slots=105977578 rec_dense=32 rec_pool=18 pool_div=4 pool_blocks=33554432 pool_shift=17 D=3 compact=0 thr_planes=0 sides=2 time=1 blk=1 cold=1 uv=1 tminmax=0 samples=6442450944 recs=81390779904 pool=14495514624 ring=134217728 running=25165824 state=33912826368",
    "spectral_fwd_4096":
        "chunk=1366 slots=268435456 rec_dense=50 rec_pool=0 pool_div=4 pool_blocks=0 pool_shift=0 D=3 compact=0 thr_planes=1 sides=2 time=1 blk=0 cold=1 uv=1 tminmax=0 samples=34376515584 recs=0 pool=0 ring=0 running=25165824 state=88046829568",
    "spectral_rec_64_grow2":
        "chunk=64 slots=67108864 rec_dense=32 rec_pool=18 pool_div=1 pool_blocks=67108864 pool_shift=18 D=3 compact=0 thr_planes=0 sides=2 time=1 blk=1 cold=1 uv=1 tminmax=0 samples=1610612736 recs=51539607552 pool=28991029248 ring=268435456 running=25165824 state=21474836480",
    "colour_fwd_512_avail_1g":
        "chunk=64 slots=1024 rec_dense=50 rec_pool=0 pool_div=16 pool_blocks=0 pool_shift=0 D=5 compact=0 thr_planes=3 sides=2 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=1610612736 recs=0 pool=0 ring=0 running=25165824 state=221184",
    "small_rec_avail0":
        "chunk=5 slots=6000 rec_dense=8 rec_pool=42 pool_div=16 pool_blocks=4096 pool_shift=4 D=3 compact=1 thr_planes=0 sides=2 time=0 blk=1 cold=0 uv=0 tminmax=0 samples=144000 recs=1152000 pool=4128768 ring=16384 running=28800 state=1056256",
    "small_fwd_slots2000_chunk3600":
        "chunk=3 slots=2000 rec_dense=50 rec_pool=0 pool_div=16 pool_blocks=0 pool_shift=0 D=5 compact=0 thr_planes=3 sides=2 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=86400 recs=0 pool=0 ring=0 running=28800 state=432640",
    "small_rec_dense1_div100000":
        "chunk=8 slots=9600 rec_dense=1 rec_pool=49 pool_div=100000 pool_blocks=4096 pool_shift=4 D=3 compact=1 thr_planes=0 sides=2 time=0 blk=1 cold=0 uv=0 tminmax=0 samples=230400 recs=230400 pool=4816896 ring=16384 running=28800 state=1689600",
    "small_rec_depth5":
        "chunk=4 slots=4800 rec_dense=5 rec_pool=0 pool_div=16 pool_blocks=0 pool_shift=0 D=3 compact=1 thr_planes=0 sides=2 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=115200 recs=576000 pool=0 ring=0 running=28800 state=806400",
    "colour_rec_full_1024":
        "chunk=1024 slots=157861380 rec_dense=8 rec_pool=42 pool_div=16 pool_blocks=16777216 pool_shift=16 D=5 compact=0 thr_planes=0 sides=2 time=1 blk=1 cold=0 uv=1 tminmax=0 samples=25769803776 recs=50515641600 pool=28185722880 ring=67108864 running=25165824 state=35360951296",
    "colour_fwd_textured_tri":
        "chunk=256 slots=268435456 rec_dense=50 rec_pool=0 pool_div=16 pool_blocks=0 pool_shift=0 D=5 compact=0 thr_planes=3 sides=2 time=0 blk=0 cold=0 uv=1 tminmax=0 samples=6442450944 recs=0 pool=0 ring=0 running=25165824 state=66571993088",
    "colour_rec_glass_tri":
        "chunk=128 slots=98769282 rec_dense=8 rec_pool=42 pool_div=4 pool_blocks=33554432 pool_shift=17 D=5 compact=0 thr_planes=0 sides=2 time=0 blk=1 cold=1 uv=0 tminmax=0 samples=3221225472 recs=31606170240 pool=56371445760 ring=134217728 running=25165824 state=26865247232",
    "colour_rec_grow7":
        "chunk=128 slots=59228550 rec_dense=8 rec_pool=42 pool_div=1 pool_blocks=67108864 pool_shift=18 D=3 compact=1 thr_planes=0 sides=2 time=0 blk=1 cold=0 uv=0 tminmax=0 samples=3221225472 recs=11371881600 pool=67645734912 ring=268435456 running=25165824 state=10424226816",
    "colour_rec_depth0":
        "chunk=2 slots=2400 rec_dense=1 rec_pool=0 pool_div=16 pool_blocks=0 pool_shift=0 D=3 compact=1 thr_planes=0 sides=2 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=57600 recs=57600 pool=0 ring=0 running=28800 state=403456",
    "spectral_rec_dense64":
        "chunk=4 slots=4800 rec_dense=50 rec_pool=0 pool_div=4 pool_blocks=0 pool_shift=0 D=3 compact=0 thr_planes=0 sides=2 time=0 blk=0 cold=1 uv=0 tminmax=0 samples=115200 recs=5760000 pool=0 ring=0 running=28800 state=1267200",
    "small_slots300":
        "chunk=5 slots=1024 rec_dense=50 rec_pool=0 pool_div=16 pool_blocks=0 pool_shift=0 D=5 compact=0 thr_planes=3 sides=2 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=144000 recs=0 pool=0 ring=0 running=28800 state=221184",
    "tiny_slots300":
        "chunk=4 slots=400 rec_dense=50 rec_pool=0 pool_div=16 pool_blocks=0 pool_shift=0 D=5 compact=0 thr_planes=3 sides=2 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=9600 recs=0 pool=0 ring=0 running=2400 state=87040",
    "colour_rec_one_sample_chunks":
        "chunk=1 slots=203360 rec_dense=8 rec_pool=42 pool_div=16 pool_blocks=16384 pool_shift=6 D=3 compact=1 thr_planes=0 sides=2 time=0 blk=1 cold=0 uv=0 tminmax=0 samples=25165824 recs=39045120 pool=16515072 ring=65536 running=25165824 state=35791872",
    "normal_512":
        "chunk=512 slots=268435456 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=12884901888 recs=0 pool=0 ring=0 running=25165824 state=18253611008",
    "albedo_spheres_uv_1024":
        "chunk=1024 slots=268435456 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=1 blk=0 cold=0 uv=1 tminmax=0 samples=25769803776 recs=0 pool=0 ring=0 running=25165824 state=24696061952",
    "albedo_tri_uv_256":
        "chunk=256 slots=268435456 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=0 blk=0 cold=0 uv=1 tminmax=0 samples=6442450944 recs=0 pool=0 ring=0 running=25165824 state=22548578304",
    "wireframe_512":
        "chunk=512 slots=268435456 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=0 blk=0 cold=0 uv=0 tminmax=1 samples=12884901888 recs=0 pool=0 ring=0 running=25165824 state=22548578304",
    "wireframe_spheres_uv_4096":
        "chunk=1366 slots=268435456 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=1 blk=0 cold=0 uv=1 tminmax=1 samples=34376515584 recs=0 pool=0 ring=0 running=25165824 state=28991029248",
    "normal_512_avail_1g":
        "chunk=64 slots=1024 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=1610612736 recs=0 pool=0 ring=0 running=25165824 state=69632",
    "wireframe_spheres_avail_8g":
        "chunk=64 slots=22164395 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=1 blk=0 cold=0 uv=1 tminmax=1 samples=1610612736 recs=0 pool=0 ring=0 running=25165824 state=2393755392",
    "small_wireframe_chunk3600_slots1024":  # tests/test_gpu_preview.py::test_spp_1_and_chunked_spp_5
        "chunk=3 slots=1024 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=0 blk=0 cold=0 uv=0 tminmax=1 samples=86400 recs=0 pool=0 ring=0 running=28800 state=86016",
    "small_wireframe_avail0":
        "chunk=5 slots=6000 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=0 blk=0 cold=0 uv=0 tminmax=1 samples=144000 recs=0 pool=0 ring=0 running=28800 state=504064",
    "small_normal_slots300":
        "chunk=3 slots=1024 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=86400 recs=0 pool=0 ring=0 running=28800 state=69632",
    "tiny_albedo_slots300":
        "chunk=1 slots=100 rec_dense=0 rec_pool=0 pool_div=0 pool_blocks=0 pool_shift=0 D=0 compact=0 thr_planes=0 sides=1 time=0 blk=0 cold=0 uv=0 tminmax=0 samples=2400 recs=0 pool=0 ring=0 running=2400 state=7168",
}
# the state allocation's layout: every array's offset per side (-1: the render has no such array)
LAYOUTS = {
    "spectral_rec_256":
        "s0.ray=0 s0.kind=5086923776 s0.time=5510834176 s0.path=6358654976 s0.blk=8054296320 s0.cold=8478206720 s0.hit=13565130496 s0.thr=-1 s0.tminmax=-1 s1.ray=16956413184 s1.kind=22043336960 s1.time=22467247360 s1.path=23315068160 s1.blk=25010709504 s1.cold=25434619904 s1.hit=30521543680 s1.thr=-1 s1.tminmax=-1",
    "small_fwd_slots2000_chunk3600":
        "s0.ray=0 s0.kind=96000 s0.time=-1 s0.path=104192 s0.blk=-1 s0.cold=-1 s0.hit=136192 s0.thr=168192 s0.tminmax=-1 s1.ray=216320 s1.kind=312320 s1.time=-1 s1.path=320512 s1.blk=-1 s1.cold=-1 s1.hit=352512 s1.thr=384512 s1.tminmax=-1",
    "wireframe_spheres_uv_4096":
        "s0.ray=0 s0.kind=12884901888 s0.time=13958643712 s0.path=-1 s0.blk=-1 s0.cold=-1 s0.hit=16106127360 s0.thr=-1 s0.tminmax=24696061952",
    "small_wireframe_chunk3600_slots1024":
        "s0.ray=0 s0.kind=49152 s0.time=-1 s0.path=-1 s0.blk=-1 s0.cold=-1 s0.hit=53248 s0.thr=-1 s0.tminmax=69632",
}
# The plan cache (PlanCache::find): an empty or invalidated cache serves nothing; equal inputs,
# and inputs that differ in `avail` alone, reuse the stored plan; any other field makes a new one.
CACHE = dict(empty_misses=1, same=1, avail=1, pool_grow=0, accumulation=0, slots=0, chunk_units=0, rec_dense=0, pool_div=0,
             size_spp=0, num_pixels=0, max_depth=0, sampler=0, invalidated=0)
# Rows whose plan may exceed the 15/32 budget because a floor binds: the budget is below the
# per-sample results of one 64M-unit chunk, and the entries stay at 1024.
FLOOR_BOUND = {"colour_fwd_512_avail_1g", "normal_512_avail_1g"}
# bytes per entry of each array (RayOD, kind word, time, PathHot, blk word, PathCold, hit record, throughput plane, tminmax)
ENTRY = dict(ray=48, kind=4, time=8, path=16, blk=4, cold=48, tminmax=16)


def fields(text):
    return {k: int(v) for k, v in (f.split("=") for f in text.split())}


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = tmp_path_factory.mktemp("render_plan") / "render_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ROOT / "tests" / "render_plan_check.cpp"), str(CSRC / "render_plan.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-3000:]  # a sanitizer report ends the program
    return {line.split("|")[0]: line.split("|")[1:] for line in run.stdout.splitlines()}


def test_every_case_ran(rows):
    assert sorted(rows) == sorted([*PLANS, "cache"])


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_is_the_earlier_arithmetics(rows, name):
    assert rows[name][1] == PLANS[name]


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_layout_is_the_earlier_carve(rows, name):
    assert rows[name][2].strip() == LAYOUTS[name]


def test_cache_rule(rows):
    assert fields(rows["cache"][0]) == CACHE


def test_every_flag_takes_both_values():
    plans = [fields(p) for p in PLANS.values()]
    for k in ("compact", "time", "blk", "cold", "uv", "tminmax"):
        assert {p[k] for p in plans} == {0, 1}, k
    assert {p["sides"] for p in plans} == {1, 2}
    assert {p["thr_planes"] for p in plans} == {0, 1, 3}
    assert {p["D"] for p in plans} == {0, 3, 5}
    assert {p["pool_div"] for p in plans} >= {1, 4, 16, 100000}  # the defaults, pool_grow's shifts, the tuning's
    assert {p["rec_dense"] for p in plans} >= {0, 1, 5, 8, 32, 50}  # preview, tuning, max_depth, Colour, Spectral, forward
    assert any(p["pool_blocks"] == 4096 for p in plans) and any(p["pool_blocks"] > 4096 for p in plans)
    assert any(p["slots"] == 268435456 for p in plans)  # the 256M cap
    budget_bound = [p for p in plans if 1024 < p["slots"] < 268435456 and p["samples"] > 10 ** 9]
    assert any(p["sides"] == 2 for p in budget_bound) and any(p["sides"] == 1 for p in budget_bound)


def test_budget(rows):
    """Per-sample results, records, overflow pool (as allocated: its power-of-two rounding
    included), ring and state lie within 15/32 of `avail`. The running sums (24 B per pixel) and
    the tracer's spill area are outside the rule, as they always were."""
    bound = set()
    for name in PLANS:
        i, p = fields(rows[name][0]), fields(rows[name][1])
        if i["avail"] == 0:
            continue
        used = p["samples"] + p["recs"] + p["pool"] + p["ring"] + p["state"]
        if used > i["avail"] // 32 * 15:
            bound.add(name)
            assert p["slots"] == 1024
    assert bound == FLOOR_BOUND


def test_chunks_cover_the_samples_and_are_balanced(rows):
    for name in PLANS:
        i, p = fields(rows[name][0]), fields(rows[name][1])
        n = -(-i["size_spp"] // p["chunk"])
        assert n * p["chunk"] >= i["size_spp"] > (n - 1) * p["chunk"], name
        assert p["chunk"] == -(-i["size_spp"] // n), name  # no chunk count n leaves smaller chunks


def test_layout_arrays_are_aligned_disjoint_and_fill_the_state(rows):
    for name in PLANS:
        p, lay = fields(rows[name][1]), fields(rows[name][2])
        size = dict(ENTRY, hit=32 if p["uv"] else 16, thr=8 * p["thr_planes"])
        present = dict(ray=1, kind=1, hit=1, time=p["time"], path=p["sides"] == 2, blk=p["blk"], cold=p["cold"],
                       thr=p["thr_planes"] != 0, tminmax=p["tminmax"])
        assert len(lay) == 9 * p["sides"], name
        spans = []
        for key, off in lay.items():
            arr = key.split(".")[1]
            assert (off >= 0) == bool(present[arr]), (name, key)
            if off >= 0:
                assert off % 256 == 0, (name, key)
                spans.append((off, off + p["slots"] * size[arr]))
        spans.sort()
        for (_, end), (start, _) in zip(spans, spans[1:]):
            assert end <= start < end + 256, name  # disjoint, and no gap beyond the alignment
        assert spans[0][0] == 0 and spans[-1][1] <= p["state"] < spans[-1][1] + 256, name
