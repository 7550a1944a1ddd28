"""Adaptive sampling of a progressive session on the GPU (IZPI_PROG_ADAPTIVE,
izpi_gpu_progressive_adapt, IZPI_SNAP_SAMPLES).

The reference is tests/adapt_ref.py: the oracle's one-sample renders folded in numpy for as long
as a pixel is active, and the oracle's counters of each step's active pixels as 1 x 1 tiles.
Snapshots, integers and counters are compared bit for bit; the only GPU-against-GPU comparisons
are the ones the feature's contract names (a plain session, a single context, render(spp = n)).
"""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from izpi_amd import _native as N
from izpi_amd import build, configs
from izpi_amd.renderer import GPURenderer, MultiGPURenderer
from tests import adapt_ref as AR
from tests.test_forward_accumulation import scene_case

pytestmark = pytest.mark.gpu

ACCS = [N.ACC_RECURSIVE, N.ACC_FORWARD]
RULE = dict(threshold=0.25, floor=0.01, tolerated=0.05, min_spp=4)
INTS = ("pixels", "nonfinite", "active", "retired", "samples", "done", "converged")


def same_bits(got, want):
    """Bit-identical arrays (a NaN matches a NaN)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape
    bad = np.argwhere((got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want)))
    assert len(bad) == 0, "not bit-identical: %d values differ, first %s" % (len(bad), bad[:5].tolist())


@functools.lru_cache(maxsize=None)
def reference(which, acc, steps, threshold, size=None, first=2, counters=True):
    """adapt_ref.simulate, once per process (read only). first: adapt follows a step once done >= first."""
    return AR.simulate(which, acc, list(steps), dict(RULE, threshold=threshold), size=size, counters=counters,
                       evaluate=lambda done: done >= first)


def renderer(which, acc, size=None, spp=None, **kw):
    scene, W, H, n, sampler = scene_case(which)
    if size is not None:
        W, H = size
    return GPURenderer(scene, W, H, n if spp is None else spp, sampler=sampler, accumulation=acc, **kw)


def check_step(s, st, rule, counters=True):
    """Session s after a step (and its adapt) against the reference's record of that step."""
    assert s.done == st["done"]
    same_bits(s.snapshot(), st["canvas"])
    same_bits(s.snapshot(N.SNAP_SAMPLES), st["samples_snap"])
    if st["done"] >= 2:
        same_bits(s.snapshot(N.SNAP_NOISE), st["noise"])
        got = s.noise(**rule)
        for k, v in st["stat"].items():
            if k == "sum_error":  # (its blocks add in the same order: the session's packed order)
                assert np.float64(got[k]).tobytes() == np.float64(v).tobytes(), (k, got[k], v)
            else:
                assert got[k] == v, (k, got[k], v)
        if st["adapt"] is not None:
            assert got["above"] == st["adapt"]["active"]
    if counters:
        got = {k: s.stats[k] for k in AR.COUNTERS}
        assert got == st["counters"], (st["done"], got, st["counters"])
        assert got["samples"] == st["samples"]


def run_session(r, ref, steps, rule, first=2, counters=True, **kw):
    """Step by step with adapt from done >= first on, every step checked; returns the adapt integers."""
    seen = []
    with r.progressive(max(steps[0], 1), total=sum(steps), noise=True, adaptive=True, **kw) as s:
        for k, st in zip(steps, ref):
            s.step(k)
            if s.done >= first:
                got = s.adapt(**rule)
                print("done", s.done, {k: got[k] for k in INTS})
                assert {k: got[k] for k in INTS} == st["adapt"], (got, st["adapt"])
                assert got["device_ms"] >= 0
                seen.append(got)
            check_step(s, st, rule, counters)
            d, t = r.progress()
            assert (d, t) == (st["samples"], len(st["n"]) * sum(steps))
    return seen


# ---- 1. staggered retirement
@pytest.mark.parametrize("acc", ACCS)
@pytest.mark.parametrize("threshold", [0.25, 0.5])
def test_staggered_retirement(gpu, acc, threshold):
    """cornell 40 x 30, steps of 4 up to 32, adapt after every step: lists longer than 256 entries
    (full blocks: the LDS-staged fold through the index), shorter ones (the partial-block fold),
    most of them no multiple of 64; at threshold 0.5 the last lists are shorter than one wave."""
    steps = (4,) * 8
    ref, W, H, sampler = reference("cornell", acc, steps, threshold, (40, 30))
    counts = [st["adapt"]["active"] for st in ref]
    if acc == N.ACC_FORWARD:  # (the issue's figures, from the CPU oracle)
        assert counts == ([716, 614, 502, 384, 285, 221, 184, 159] if threshold == 0.25 else counts[:6] + [52, 44])
    # conditions on the reference's own map: the test cannot pass vacuously
    assert len(set(ref[-1]["n"].tolist())) >= 3 and max(counts) > 256
    if threshold == 0.5:
        assert min(counts) < 64
    else:
        assert len(set(ref[-1]["n"].tolist())) == 8 and min(counts) < 256 and any(c % 64 for c in counts)
        assert int((ref[-1]["n"] == 32).sum()) == counts[-2]  # the pixels that took the last step
    r = renderer("cornell", acc, (W, H))
    run_session(r, ref, steps, dict(RULE, threshold=threshold))
    r.close()


# ---- 2. odd chunks
@pytest.mark.parametrize("acc", ACCS)
def test_odd_chunks(gpu, acc):
    """step_spp 3, steps of 3, 3, 2, 5: chunks of 3, 3, 2 and 3 + 2 samples at s0 = 0, 3, 6, 8, 11;
    the first evaluation at done = 6 (max(2, min_spp) = 4), so the list steps start at s0 = 6."""
    steps = (3, 3, 2, 5)
    ref, W, H, sampler = reference("cornell", acc, steps, 0.25, (40, 30), 4)
    assert ref[0]["adapt"] is None and ref[0]["rendered"] == ref[1]["rendered"] == 1200
    if acc == N.ACC_FORWARD:
        assert ref[1]["adapt"]["active"] == 702
    assert 256 < ref[3]["rendered"] < 1200
    r = renderer("cornell", acc, (W, H))
    run_session(r, ref, steps, RULE, first=4)
    r.close()


# ---- 3. Spectral, forward: raw samples weighed by the fold, through the index
@pytest.mark.parametrize("threshold", [0.25, 0.5])
def test_spectral_forward(gpu, threshold):
    steps = (4,) * 4
    ref, W, H, sampler = reference("glass_spectral", N.ACC_FORWARD, steps, threshold)
    if threshold == 0.25:
        assert [st["adapt"]["active"] for st in ref] == [493, 485, 471, 464]
    assert len(set(ref[-1]["n"].tolist())) >= 3
    r = renderer("glass_spectral", N.ACC_FORWARD)
    run_session(r, ref, steps, dict(RULE, threshold=threshold))
    r.close()


def test_nonfinite_pixels_retire(gpu):
    """special_spectral: the pixels that are not finite at an evaluation retire there, and
    `nonfinite` is the reference's at every call (it counts the retired ones too)."""
    steps = (4,) * 4
    ref, W, H, sampler = reference("special_spectral", N.ACC_FORWARD, steps, 0.25)
    assert ref[0]["adapt"]["nonfinite"] > 0
    r = renderer("special_spectral", N.ACC_FORWARD)
    seen = run_session(r, ref, steps, RULE)
    assert [a["nonfinite"] for a in seen] == [st["adapt"]["nonfinite"] for st in ref]
    r.close()


# ---- 4. edges
def test_everything_retires(gpu):
    """Threshold 1e9: no pixel is above it, so all retire at the first adapt; further steps leave
    done and the snapshots as they are, and converge returns converged."""
    acc = N.ACC_FORWARD
    rule = dict(RULE, threshold=1e9)
    ref, W, H, sampler = reference("cornell", acc, (4,), 1e9, (40, 30))
    r = renderer("cornell", acc, (W, H), spp=32)
    with r.progressive(4, noise=True, adaptive=True) as s:
        s.step()
        got = s.adapt(**rule)
        assert (got["active"], got["retired"], got["samples"], got["converged"]) == (0, W * H, 4 * W * H, 1)
        check_step(s, ref[0], rule)
        before = (s.snapshot().tobytes(), s.snapshot(N.SNAP_SAMPLES).tobytes(), dict(s.stats))
        for _ in range(2):
            s.step()
            assert s.done == 4
        stat = s.converge(**rule)
        assert s.done == 4 and stat["converged"] == 1 and stat["above"] == 0
        after = (s.snapshot().tobytes(), s.snapshot(N.SNAP_SAMPLES).tobytes())
        assert after == before[:2]
        assert {k: s.stats[k] for k in AR.COUNTERS} == {k: before[2][k] for k in AR.COUNTERS}
        assert r.progress() == (4 * W * H, 32 * W * H)
    with r.progressive(4, noise=True, adaptive=True) as s:  # converge alone: one step, one adapt
        stat = s.converge(**rule)
        assert s.done == 4 and stat["done"] == 4 and stat["converged"] == 1 and s.active == 0
    r.close()


@pytest.mark.parametrize("contexts", [1, 2])
def test_converge_returns_when_everything_retired_below_min_spp(gpu, contexts):
    """adapt is legal from done = 2 and reads no min_spp: at done = 4 it retires everything
    (threshold 1e9); converge with min_spp = 8 then finds no active pixel, renders nothing and
    returns with done = 4, the frame as it was and noise()'s statistic of it (not converged by
    its own rule: done < min_spp). One context and a group of two."""
    acc = N.ACC_FORWARD
    rule = dict(RULE, threshold=1e9, min_spp=8)
    ref, W, H, sampler = reference("cornell", acc, (4,), 1e9, (40, 30))
    scene = scene_case("cornell")[0]
    if contexts == 1:
        r = GPURenderer(scene, W, H, 32, sampler=sampler, accumulation=acc)
    else:
        r = MultiGPURenderer(scene, W, H, 32, [0] * contexts, sampler=sampler, bvh="reference", accumulation=acc)
    with r.progressive(4, noise=True, adaptive=True) as s:
        s.step()
        got = s.adapt(**rule)
        assert (got["active"], got["retired"], got["done"], got["converged"]) == (0, W * H, 4, 0)
        before = s.snapshot().tobytes()
        stat = s.converge(**rule)
        assert s.done == 4 and s.active == 0
        assert (stat["done"], stat["above"], stat["pixels"], stat["converged"]) == (4, 0, W * (H - 1), 0)
        same_bits(s.snapshot(), ref[0]["canvas"])
        assert s.snapshot().tobytes() == before
        same_bits(s.snapshot(N.SNAP_SAMPLES), ref[0]["samples_snap"])
        assert r.progress() == (4 * W * H, 32 * W * H)
        stat = s.converge(**dict(rule, min_spp=4))  # ... and by its rule once min_spp allows
        assert s.done == 4 and stat["converged"] == 1
    r.close()


@pytest.mark.parametrize("acc", ACCS)
def test_without_adapt_it_is_a_plain_noise_session(gpu, acc):
    which = "glass_spectral"
    r = renderer(which, acc)
    seen = {}
    for adaptive in (False, True):
        with r.progressive(3, noise=True, adaptive=adaptive) as s:
            for _ in range(3):
                s.step()
                seen[adaptive, s.done] = (s.snapshot().tobytes(), s.snapshot(N.SNAP_DISPLAY).tobytes(),
                                          s.snapshot(N.SNAP_NOISE).tobytes() if s.done >= 2 else b"",
                                          {k: s.stats[k] for k in AR.COUNTERS},
                                          {k: v for k, v in s.noise(**RULE).items() if k != "device_ms"})
                if adaptive:
                    assert (s.snapshot(N.SNAP_SAMPLES)[1:, :, :3] == s.done).all()
    for done in (3, 6, 8):
        assert seen[True, done] == seen[False, done]
    r.close()


def test_rules(gpu):
    acc = N.ACC_FORWARD
    L = N.lib()
    W, H = 40, 30
    r = renderer("cornell", acc, (W, H))
    out = np.zeros((H, W, 4))
    ptr = out.ctypes.data_as(C.c_void_p)
    st, good = N.AdaptStats(), N.noise_params(**RULE)
    req = r.request()
    assert L.izpi_gpu_progressive_begin_ex(r.ctx, C.byref(req), 4, N.PROG_ADAPTIVE) == N.IZPI_ERR_INVALID
    assert b"IZPI_PROG_NOISE" in L.izpi_gpu_last_error(r.ctx)
    for flags in (2, 3):  # the flag value 2 is no flag: refused as before the adaptive flag existed
        assert L.izpi_gpu_progressive_begin_ex(r.ctx, C.byref(req), 4, flags) == N.IZPI_ERR_INVALID
        assert L.izpi_gpu_last_error(r.ctx) == b"progressive_begin: unknown flags"
    assert L.izpi_gpu_progressive_begin_ex(r.ctx, C.byref(req), 4, 8 | N.PROG_NOISE | N.PROG_ADAPTIVE) == N.IZPI_ERR_INVALID
    assert L.izpi_gpu_progressive_adapt(r.ctx, C.byref(good), C.byref(st)) == N.IZPI_ERR_INVALID  # no session
    with r.progressive(4, noise=True) as s:  # a plain noise session
        s.step(4)
        assert L.izpi_gpu_progressive_snapshot(r.ctx, N.SNAP_SAMPLES, ptr) == N.IZPI_ERR_INVALID
        assert b"IZPI_PROG_ADAPTIVE" in L.izpi_gpu_last_error(r.ctx)
        assert L.izpi_gpu_progressive_adapt(r.ctx, C.byref(good), C.byref(st)) == N.IZPI_ERR_INVALID
        assert s.snapshot().any() and not out.any() and st.pixels == 0  # the session is intact
    ref = reference("cornell", acc, (4,) * 8, 0.25, (W, H))[0]
    s = r.progressive(4, total=32, noise=True, adaptive=True)
    for done in (0, 1):
        if done:
            s.step(1)
        assert L.izpi_gpu_progressive_adapt(r.ctx, C.byref(good), C.byref(st)) == N.IZPI_ERR_INVALID
        assert b"at least 2 samples" in L.izpi_gpu_last_error(r.ctx)
    for field, value in (("threshold", 0.0), ("floor", float("nan")), ("tolerated", 1.5), ("flags", 1)):
        bad = N.noise_params(**RULE)
        setattr(bad, field, value)
        assert L.izpi_gpu_progressive_adapt(r.ctx, C.byref(bad), C.byref(st)) == N.IZPI_ERR_INVALID, field
        assert L.izpi_gpu_last_error(r.ctx).startswith(b"noise: ")
    assert st.pixels == 0
    s.step(3)  # ... and left the session intact: it goes on as the reference does
    assert {k: v for k, v in s.adapt(**RULE).items() if k in INTS} == ref[0]["adapt"]
    check_step(s, ref[0], RULE)
    s.step()
    s.adapt(**RULE)
    check_step(s, ref[1], RULE)
    s.close()
    p = GPURenderer(configs.cornell_rgb(), 32, 32, 4, sampler=N.SAMPLER_NORMAL, bvh="gpu")  # a preview sampler
    preq = p.request()
    assert L.izpi_gpu_progressive_begin_ex(p.ctx, C.byref(preq), 2, N.PROG_NOISE | N.PROG_ADAPTIVE) == N.IZPI_ERR_INVALID
    assert b"preview sampler" in L.izpi_gpu_last_error(p.ctx)
    with p.progressive(2, noise=True) as ps:  # the context is intact
        ps.step()
        assert ps.snapshot().any()
    p.close()
    r.close()


# ---- 5. tiles and the packed layout
def test_tiles_packed(gpu):
    """Two 16 x 16 tiles packed (none in sample row 0), steps of 4 up to 16."""
    acc = N.ACC_RECURSIVE
    steps = (4,) * 4
    tiles = np.array(((0, 1, 15, 16), (16, 16, 31, 31)), np.uint32)
    scene, W, H, _, sampler = scene_case("cornell")
    ref = AR.simulate("cornell", acc, list(steps), RULE, tiles=tiles)[0]
    counts = [st["adapt"]["active"] for st in ref]
    assert len(set(ref[-1]["n"].tolist())) >= 3 and 0 < counts[-1] < counts[0] < 512
    r = renderer("cornell", acc)
    with r.progressive(4, total=16, tiles=tiles, layout=N.OUT_PACKED, noise=True, adaptive=True) as s:
        for st in ref:
            s.step()
            got = s.adapt(**RULE)
            assert {k: got[k] for k in INTS} == st["adapt"]
            for form, key in ((N.SNAP_CANVAS, "canvas"), (N.SNAP_SAMPLES, "samples_snap"), (N.SNAP_NOISE, "noise")):
                snap = s.snapshot(form)
                assert snap.shape == (2 * 16 * 16 * 4,)
                same_bits(snap.reshape(-1, 4), AR.packed_rows(st[key], tiles, H))
            assert {k: s.stats[k] for k in AR.COUNTERS} == st["counters"]
            assert s.noise(**RULE)["above"] == st["adapt"]["active"]
    r.close()


# ---- 6. multi-GPU
@pytest.mark.parametrize("contexts", [2, 3])
def test_multi(gpu, contexts):
    """CANVAS and SAMPLES snapshots and adapt's integers are one context's (and the reference's);
    converge stops at the same done."""
    acc, steps = N.ACC_FORWARD, (4,) * 8
    ref, W, H, sampler = reference("cornell", acc, steps, 0.25, (40, 30))
    scene = scene_case("cornell")[0]
    one = GPURenderer(scene, W, H, 32, sampler=sampler, accumulation=acc)
    m = MultiGPURenderer(scene, W, H, 32, [0] * contexts, sampler=sampler, bvh="reference", accumulation=acc)
    with one.progressive(4, noise=True, adaptive=True) as a, m.progressive(4, noise=True, adaptive=True) as b:
        for st in ref[:3]:
            a.step()
            b.step()
            ga, gb = a.adapt(**RULE), b.adapt(**RULE)
            assert {k: gb[k] for k in INTS} == {k: ga[k] for k in INTS} == st["adapt"]
            for form, key in ((N.SNAP_CANVAS, "canvas"), (N.SNAP_SAMPLES, "samples_snap"), (N.SNAP_NOISE, "noise")):
                snap = b.snapshot(form)
                assert snap.tobytes() == a.snapshot(form).tobytes()
                same_bits(snap, st[key])
            assert b.noise(**RULE)["above"] == st["adapt"]["active"]
            assert sum(d["samples"] for d in b.stats) == st["samples"]
    rule = dict(RULE, tolerated=0.5)  # the reference's first count at or below half of the finite pixels
    stop = next(st["done"] for st in ref if st["adapt"]["active"] <= 0.5 * (st["adapt"]["pixels"] - st["adapt"]["nonfinite"]))
    assert 4 < stop < 32
    with one.progressive(4, noise=True, adaptive=True) as a, m.progressive(4, noise=True, adaptive=True) as b:
        sa, sb = a.converge(**rule), b.converge(**rule)
        assert a.done == b.done == stop and sa["converged"] == sb["converged"] == 1 and sa["above"] == sb["above"]
        assert b.snapshot().tobytes() == a.snapshot().tobytes()
        assert b.snapshot(N.SNAP_SAMPLES).tobytes() == a.snapshot(N.SNAP_SAMPLES).tobytes()
    one.close()
    m.close()


# ---- 7. render_adaptive and the command-line tool
def test_render_adaptive_pixels_are_plain_renders(gpu):
    """Every pixel of render_adaptive's image is that pixel of render(spp = n_p), bit for bit,
    checked against a GPU render at each distinct n_p of the returned map (at most 8)."""
    acc = N.ACC_FORWARD
    W, H = 40, 30
    ref = reference("cornell", acc, (4,) * 8, 0.25, (W, H), 4)[0]
    r = renderer("cornell", acc, (W, H), spp=32)
    img, stats, n_map = r.render_adaptive(0.25, step_spp=4, floor=0.01, tolerated=0.05, min_spp=4)
    assert n_map.shape == (H, W) and np.array_equal(n_map, ref[-1]["n_map"])
    assert stats["done"] == 32 and stats["above"] == ref[-1]["adapt"]["active"]
    distinct = sorted(set(n_map[1:].reshape(-1).astype(int).tolist()))
    assert 3 <= len(distinct) <= 8
    for n in distinct:
        plain = r.render(spp=n)
        m = n_map == n
        m[0] = False  # (canvas row 0 is no pixel's)
        assert img[m].tobytes() == plain[m].tobytes(), n
    assert not img[0].any() and not n_map[0].any()
    r.close()


def test_cli_writes_the_same_map(gpu, tmp_path):
    """izpi-render --adaptive --samples-out on the RGB box: the map and the image are
    render_adaptive's for the same scene, tree and rule; one IZPI_ADAPT line per evaluation."""
    box = tmp_path / "box.pbtxt"
    box.write_text(configs.cornell_rgb_pbtxt(1.0))
    out, smp = tmp_path / "out.pfm", tmp_path / "n.pfm"
    run = subprocess.run([str(build.CLI), "--scene", str(box), "--x", "40", "--y", "40", "--samples", "32", "--progressive", "4",
                          "--noise-threshold", "0.25", "--noise-tolerated", "0.05", "--min-samples", "4", "--adaptive",
                          "--out", str(out), "--samples-out", str(smp)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    fields = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in run.stderr.splitlines() if ln.startswith("IZPI_ADAPT ")]
    assert all(sorted(f) == ["active", "done", "nonfinite", "pixels", "retired", "samples"] for f in fields), run.stderr
    r = GPURenderer(configs.cornell_rgb(), 40, 40, 32, bvh="gpu", accumulation=N.ACC_FORWARD)
    img, stats, n_map = r.render_adaptive(0.25, step_spp=4, floor=0.01, tolerated=0.05, min_spp=4)
    r.close()
    assert [int(f["done"]) for f in fields] == list(range(4, stats["done"] + 1, 4))
    assert int(fields[-1]["active"]) == stats["above"] and int(fields[-1]["samples"]) == int(n_map.sum()) + 40 * 4
    head = b"PF\n40 40\n-1.0\n"
    for path, want in ((smp, np.repeat(n_map[..., None], 3, 2)), (out, img[..., :3])):
        data = path.read_bytes()
        assert data.startswith(head)
        pixels = np.frombuffer(data[len(head):], "<f4").reshape(40, 40, 3)[::-1]  # bottom row first
        assert np.array_equal(pixels, want.astype(np.float32))
    assert len(set(n_map[1:].reshape(-1).tolist())) >= 3
