"""Checkpoint and resume of progressive sessions on the GPU (izpi_gpu_progressive_checkpoint /
_resume and the multi forms): a session that is exported, ended and resumed is,
bit for bit, the uninterrupted session, on the same context, on another one, in another process
and over another number of contexts.

The expected values are the uninterrupted session's, from the references that already state it:
the CPU oracle's canvas and counters, tests/noise_ref.py and tests/adapt_ref.py. GPU is compared
with GPU only where the contract names it (render(spp = n), an uninterrupted session, a blob
exported twice)."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import izpi_amd
from izpi_amd import _native as N
from izpi_amd import build, checkpoint, configs
from izpi_amd.renderer import GPURenderer, MultiGPURenderer
from tests import adapt_ref as AR
from tests import checkpoint_ref as CR
from tests import noise_ref as NR
from tests.test_forward_accumulation import scene_case
from tests.test_gpu_adapt import INTS, RULE, check_step, reference, same_bits
from tests.test_gpu_forward import assert_bitwise, oracle_both
from tests.test_gpu_noise import RULE as NOISE_RULE
from tests.test_gpu_noise import check_session

pytestmark = pytest.mark.gpu

ACCS = [N.ACC_RECURSIVE, N.ACC_FORWARD]
SIZE = (40, 30)  # 1200 pixels: 18.75 waves, the last one partial
STEPS = (4,) * 8  # test_gpu_adapt's staggered retirement: lists of 716, 614, 502, 384, 285, 221, 184, 159 (forward)
REFERENCE_COUNTERS = 6  # rays, node_visits, tri_tests, sph_tests, light_tri_tests, light_sph_tests lead the device counters


def renderer(which, acc, size=None, spp=None, contexts=1, **kw):
    scene, W, H, n, sampler = scene_case(which)
    if size is not None:
        W, H = size
    if contexts > 1:
        return MultiGPURenderer(scene, W, H, n if spp is None else spp, [0] * contexts, sampler=sampler, bvh="reference",
                                accumulation=acc, **kw)
    return GPURenderer(scene, W, H, n if spp is None else spp, sampler=sampler, accumulation=acc, **kw)


def through_a_checkpoint(s, r, step_spp, **kw):
    """Export s, end it, resume on renderer r: the new session, whose own export gives the same
    bytes (under a new cap: but for the header's informational spp)."""
    blob = s.checkpoint()
    assert s.checkpoint() == blob  # two exports of one state
    before = (s.done, s.active, s.adaptive)
    s.close()
    s2 = r.progressive(step_spp, resume=blob, **kw)
    assert (s2.done, s2.active, s2.adaptive) == before
    same_blob(s2.checkpoint(), CR.reseal(blob, spp=s2.total))
    return s2, blob


def summed(stats, keys=AR.COUNTERS):
    """The counters of a session's stats: one context's, or a group's devices added."""
    if isinstance(stats, dict):
        return {k: stats[k] for k in keys}
    return {k: sum(d[k] for d in stats) for k in keys}


def differing(a, b):
    """Where two blobs differ: header fields by name, then whether the planes do."""
    ha, hb = CR.parse(a), CR.parse(b)
    out = [k for k in ha if k != "counters" and ha[k] != hb[k]]
    out += ["counter %d" % k for k in range(CR.MAX_COUNTERS) if ha["counters"][k] != hb["counters"][k]]
    if a[CR.HEADER_BYTES:] != b[CR.HEADER_BYTES:]:
        out.append("planes")
    return out


def same_blob(a, b):
    """Two blobs are byte-equal; where they are not, the message names the header fields."""
    assert a == b, differing(a, b)


# ---- 1. plain and noise sessions
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("acc", ACCS)
def test_interrupted_session_is_the_uninterrupted_one(gpu, acc, noise):
    """cornell 40 x 30, steps 3, 3 | 2, 5 on one context: the canvas and the reference counters at
    13 samples are the oracle's and render(spp = 13)'s; a noise session's standard errors and
    statistic are noise_ref's after every further step."""
    scene, _, _, _, sampler = scene_case("cornell")
    W, H = SIZE
    r = renderer("cornell", acc, SIZE)
    s = r.progressive(3, total=13, noise=noise)
    s.step(3)
    s.step(3)
    s, blob = through_a_checkpoint(s, r, 3, total=13)
    info = izpi_amd.checkpoint_info(blob)
    assert (info["done"], info["pixels"], info["samples"], info["noise"], info["adaptive"]) == (6, W * H, 6 * W * H, noise, False)
    assert r.progress() == (6 * W * H, 13 * W * H)
    canvases = NR.case_canvases("cornell", acc, 13, SIZE)[0] if noise else None
    for n in (2, 5):
        s.step(n)
        if noise:
            check_session(s, canvases, W, H, sampler)
    assert s.done == 13
    ref, ref_stats = oracle_both(scene, W, H, 13, sampler)[acc]
    got = s.snapshot()
    assert_bitwise(got, ref, s.stats, ref_stats)
    s.close()
    assert r.render(spp=13).tobytes() == got.tobytes()
    r.close()


# ---- 2. adaptive sessions
@functools.lru_cache(maxsize=None)
def adaptive_blobs(acc):
    """One uninterrupted adaptive session (cornell 40 x 30, threshold 0.25, adapt after every step)
    on a context of its own, exported after every step's adapt: {done: blob}, and before the
    first adapt (no pixel retired yet) as done 0."""
    ref, W, H, sampler = reference("cornell", acc, STEPS, 0.25, SIZE)
    r = renderer("cornell", acc, SIZE)
    blobs = {}
    with r.progressive(4, total=sum(STEPS), noise=True, adaptive=True) as s:
        for k, st in zip(STEPS, ref):
            s.step(k)
            if s.done == 4:
                blobs[0] = s.checkpoint()
            s.adapt(**RULE)
            blobs[s.done] = s.checkpoint()
    r.close()
    return blobs


def check_group_step(s, st):
    """check_step for a group: the three snapshots and the statistic's integers and maximum
    (sum_error's last bits depend on the share plan)."""
    assert s.done == st["done"]
    same_bits(s.snapshot(), st["canvas"])
    same_bits(s.snapshot(N.SNAP_SAMPLES), st["samples_snap"])
    same_bits(s.snapshot(N.SNAP_NOISE), st["noise"])
    got = s.noise(**RULE)
    for k in ("pixels", "nonfinite", "above", "max_error", "done", "converged"):
        assert got[k] == st["stat"][k], (k, got[k], st["stat"][k])
    assert st["adapt"] is None or got["above"] == st["adapt"]["active"]


def continue_adaptive(s, ref, first, group=False):
    """Steps first.. of STEPS on session s (step first - 1's adapt has run), every step checked:
    adapt's integers, the snapshots, the statistic and the reference counters."""
    for k, st in list(zip(STEPS, ref))[first:]:
        s.step(k)
        got = s.adapt(**RULE)
        assert {k: got[k] for k in INTS} == st["adapt"], (got, st["adapt"])
        if group:
            check_group_step(s, st)
        else:
            check_step(s, st, RULE, counters=False)
        assert summed(s.stats) == st["counters"], (st["done"], summed(s.stats), st["counters"])


@pytest.mark.parametrize("acc", ACCS)
def test_adaptive_session(gpu, acc):
    ref, W, H, sampler = reference("cornell", acc, STEPS, 0.25, SIZE)
    counts = [st["adapt"]["active"] for st in ref]
    assert max(counts) > 256 and any(c % 64 for c in counts)  # (test_gpu_adapt's lists)
    blobs = adaptive_blobs(acc)
    r = renderer("cornell", acc, SIZE)
    # exported before any retirement: state 0 and n_p = done everywhere, the plain steps' kernels go on
    info = izpi_amd.checkpoint_info(blobs[0])
    assert (info["listed"], info["active"], info["done"], info["samples"]) == (0, W * H, 4, 4 * W * H)
    planes = checkpoint.unpack(W, H, [[0, 0, W - 1, H - 1]], info["flags"], blobs[0][CR.HEADER_BYTES:])
    assert not planes[3].any() and (planes[2] == 4).all() and planes[4:] == (0, 0)
    with r.progressive(4, total=sum(STEPS), resume=blobs[0]) as s:
        assert (s.done, s.active, s.adaptive) == (4, W * H, True) and s.checkpoint() == blobs[0]
        got = s.adapt(**RULE)
        assert {k: got[k] for k in INTS} == ref[0]["adapt"]
        check_step(s, ref[0], RULE, counters=False)  # (stats come with a step; continue_adaptive checks the counters)
        same_blob(s.checkpoint(), blobs[4])
    # exported after staggered retirements (three adapts), then every further step
    info = izpi_amd.checkpoint_info(blobs[12])
    assert (info["listed"], info["active"], info["samples"]) == (1, counts[2], ref[2]["samples"])
    state = checkpoint.unpack(W, H, [[0, 0, W - 1, H - 1]], info["flags"], blobs[12][CR.HEADER_BYTES:])[3]
    assert int((state == 0).sum()) == counts[2] and int((state == 1).sum()) == W * H - counts[2]
    with r.progressive(4, total=sum(STEPS), resume=blobs[12]) as s:
        assert (s.done, s.active) == (12, counts[2]) and s.checkpoint() == blobs[12]
        assert r.progress() == (ref[2]["samples"], W * H * sum(STEPS))
        check_step(s, ref[2], RULE, counters=False)  # the snapshots and noise().above == active, before any step
        continue_adaptive(s, ref, 3)
        same_blob(s.checkpoint(), blobs[32])  # the uninterrupted session's at the end
    r.close()


def test_everything_retired(gpu):
    """Threshold 1e9: all retire at the first adapt; the resumed session's steps change nothing
    and converge returns converged."""
    acc, rule = N.ACC_FORWARD, dict(RULE, threshold=1e9)
    ref, W, H, sampler = reference("cornell", acc, (4,), 1e9, SIZE)
    r = renderer("cornell", acc, SIZE, spp=32)
    s = r.progressive(4, noise=True, adaptive=True)
    s.step()
    assert s.adapt(**rule)["active"] == 0
    s, blob = through_a_checkpoint(s, r, 4)
    assert s.active == 0 and izpi_amd.checkpoint_info(blob)["active"] == 0
    check_step(s, ref[0], rule, counters=False)
    before = (s.snapshot().tobytes(), s.snapshot(N.SNAP_SAMPLES).tobytes())
    for _ in range(2):
        s.step()
        assert s.done == 4
    stat = s.converge(**rule)
    assert s.done == 4 and stat["converged"] == 1 and stat["above"] == 0
    assert (s.snapshot().tobytes(), s.snapshot(N.SNAP_SAMPLES).tobytes()) == before
    assert s.checkpoint() == blob and r.progress() == (4 * W * H, 32 * W * H)
    s.close()
    r.close()


@pytest.mark.parametrize("which", ["glass_spectral", "special_spectral"])
def test_spectral_forward(gpu, which):
    """32 x 32 forward Spectral: a noise session exported after one of three steps, an adaptive
    one after the first of four steps and its adapt. special_spectral's 668 counted non-finite
    pixels (adapt_ref's count at that adapt) keep state 2 across the checkpoint."""
    acc, steps = N.ACC_FORWARD, (4,) * 4
    canvases, W, H, sampler = NR.case_canvases(which, acc, 8)
    r = renderer(which, acc)
    s = r.progressive(3, noise=True)  # the noise session, steps 3 | 3, 2
    s.step()
    s, _ = through_a_checkpoint(s, r, 3)
    for _ in range(2):
        s.step()
        stat = check_session(s, canvases, W, H, sampler)
    assert s.done == 8 and (which != "special_spectral" or stat["nonfinite"] > 0)
    s.close()
    ref, W, H, sampler = reference(which, acc, steps, 0.25)
    s = r.progressive(4, total=16, noise=True, adaptive=True)
    s.step(steps[0])
    s.adapt(**RULE)
    s, blob = through_a_checkpoint(s, r, 4, total=16)
    info = izpi_amd.checkpoint_info(blob)
    state = checkpoint.unpack(W, H, [[0, 0, W - 1, H - 1]], info["flags"], blob[CR.HEADER_BYTES:])[3]
    nonfinite = ref[0]["adapt"]["nonfinite"]
    print(which, "state 2:", int((state == 2).sum()), "reference nonfinite:", nonfinite)
    assert int((state == 2).sum()) == nonfinite and (which != "special_spectral" or nonfinite == 668)
    for k, st in list(zip(steps, ref))[1:]:
        s.step(k)
        got = s.adapt(**RULE)
        assert {k: got[k] for k in INTS} == st["adapt"], (got, st["adapt"])
        check_step(s, st, RULE)
    s.close()
    r.close()


# ---- 3. tiles, layouts, caps
def test_packed_tiles_resumed_in_the_other_order_on_a_canvas(gpu):
    """Two packed 16 x 16 tiles, steps 2 | 2; resumed with the tiles in the other order and
    IZPI_OUT_CANVAS: the canvas of an uninterrupted session of that shape, noise_ref's errors."""
    acc = N.ACC_RECURSIVE
    canvases, W, H, sampler = NR.case_canvases("cornell", acc, 8)
    tiles = np.array(((0, 1, 15, 16), (16, 16, 31, 31)), np.uint32)
    r = renderer("cornell", acc)
    with r.progressive(2, total=4, tiles=tiles[::-1], noise=True) as s:  # the uninterrupted one
        s.step(4)
        want = s.snapshot()
    s = r.progressive(2, total=4, tiles=tiles, layout=N.OUT_PACKED, noise=True)
    s.step()
    s, blob = through_a_checkpoint(s, r, 2, total=4, tiles=tiles[::-1])
    assert izpi_amd.checkpoint_info(blob)["pixels"] == 512
    s.step()
    assert s.done == 4 and s.snapshot().tobytes() == want.tobytes()
    snap, stat = NR.reference(canvases, 4, W, H, sampler, tiles[::-1], **NOISE_RULE)
    same_bits(s.snapshot(N.SNAP_NOISE), snap)
    got = s.noise(**NOISE_RULE)
    assert {k: got[k] for k in ("pixels", "nonfinite", "above", "max_error")} == {k: stat[k] for k in ("pixels", "nonfinite", "above", "max_error")}
    s.close()
    r.close()


def test_a_higher_cap_and_another_step(gpu):
    """Cap 8 in steps of 3 up to 6; resumed with cap 16 and steps of 5 and continued past the
    old cap: one long session, which is render(spp = 16)."""
    acc = N.ACC_FORWARD
    r = renderer("cornell", acc, SIZE)
    s = r.progressive(3, total=8)
    s.step()
    s.step()
    s, blob = through_a_checkpoint(s, r, 5, total=16)
    assert (izpi_amd.checkpoint_info(blob)["spp"], s.total, s.step_spp) == (8, 16, 5)
    while s.done < 16:
        s.step()
    got, stats = s.snapshot(), summed(s.stats)
    s.close()
    assert r.render(spp=16).tobytes() == got.tobytes() and summed(r.stats) == stats
    with pytest.raises(RuntimeError, match="spp 5 is below the 6 samples done"):
        r.progressive(3, total=5, resume=blob)
    r.close()


# ---- 4. other contexts, other share plans
def test_across_contexts(gpu):
    """Export, close the context, open a new one, upload the scene, resume."""
    acc = N.ACC_FORWARD
    ref, W, H, sampler = reference("cornell", acc, STEPS, 0.25, SIZE)
    blobs = adaptive_blobs(acc)  # (their context is closed)
    r = renderer("cornell", acc, SIZE)
    with r.progressive(4, total=sum(STEPS), resume=blobs[20]) as s:
        assert s.checkpoint() == blobs[20]
        continue_adaptive(s, ref, 5)
    r.close()


@pytest.mark.parametrize("contexts", [2, 3])
def test_one_context_to_a_group(gpu, contexts):
    """Exported from one context after three adapts, resumed over 2 and 3 contexts of the one GPU."""
    acc = N.ACC_FORWARD
    ref, W, H, sampler = reference("cornell", acc, STEPS, 0.25, SIZE)
    blobs = adaptive_blobs(acc)
    g = renderer("cornell", acc, SIZE, contexts=contexts)
    with g.progressive(4, total=sum(STEPS), resume=blobs[12]) as s:
        assert (s.done, s.active) == (12, ref[2]["adapt"]["active"])
        same_blob(s.checkpoint(), blobs[12])
        continue_adaptive(s, ref, 3, group=True)
        same_blob(s.checkpoint(), blobs[32])  # the group's blob is the one context's at that state
    g.close()


def test_a_group_to_one_context(gpu):
    """A group of 3 runs the session from the start and exports after five adapts: the one
    context's blob at that state, byte for byte; one context continues it."""
    acc = N.ACC_FORWARD
    ref, W, H, sampler = reference("cornell", acc, STEPS, 0.25, SIZE)
    blobs = adaptive_blobs(acc)
    g = renderer("cornell", acc, SIZE, contexts=3)
    with g.progressive(4, total=sum(STEPS), noise=True, adaptive=True) as s:
        for k in STEPS[:5]:
            s.step(k)
            s.adapt(**RULE)
        blob = s.checkpoint()
    g.close()
    same_blob(blob, blobs[20])
    assert CR.parse(blob)["counters"][:REFERENCE_COUNTERS] == tuple(ref[4]["counters"][k] for k in AR.COUNTERS[:REFERENCE_COUNTERS])
    assert not any(CR.parse(blob)["counters"][REFERENCE_COUNTERS:])  # the diagnostics are not carried
    r = renderer("cornell", acc, SIZE)
    with r.progressive(4, total=sum(STEPS), resume=blob) as s:
        continue_adaptive(s, ref, 5)
    r.close()


# ---- 5. refusals on the device
def test_refusals_leave_no_session_and_a_usable_context(gpu):
    acc = N.ACC_FORWARD
    W, H = SIZE
    L = N.lib()
    r = renderer("cornell", acc, SIZE)
    frame = r.render(spp=2).tobytes()
    cells = np.array([[x, y, x, y] for y in range(3, 7) for x in range(5, 13)], np.uint32)  # 32 pixels as 1 x 1 tiles

    def refused(message, **kw):
        """A resume that must fail with `message`; then no session is open and the next frame is bit-exact."""
        seed = r.seed
        r.seed += kw.pop("seed_offset", 0)
        with pytest.raises(RuntimeError, match=message):
            r.progressive(2, total=8, **kw)
        r.seed = seed
        assert L.izpi_gpu_progressive_end(r.ctx) == N.IZPI_ERR_INVALID
        assert L.izpi_gpu_last_error(r.ctx) == b"no progressive session is open"
        assert r.render(spp=2).tobytes() == frame

    s = r.progressive(2, total=8, noise=True)
    n = C.c_uint64()
    s._call("checkpoint_bytes", C.byref(n))
    buf = C.create_string_buffer(n.value)
    with pytest.raises(RuntimeError, match=r"done == 0"):  # export before the first sample
        s.checkpoint()
    s.step()
    with pytest.raises(RuntimeError, match="the output holds %d bytes, the blob takes %d" % (n.value - 1, n.value)):
        s._call("checkpoint", r.scene_tag, buf, n.value - 1)  # cap one byte short
    blob = s.checkpoint()  # (the session is as it was)
    with pytest.raises(RuntimeError, match="a progressive session is already open"):
        r.progressive(2, total=8, resume=blob)
    assert s.checkpoint() == blob
    s.close()
    tag = r.scene_tag
    r._scene_tag = tag ^ 1
    refused("the scene tag differs", resume=blob)
    r._scene_tag = tag
    refused("the request's seed differs", resume=blob, seed_offset=1)
    refused("truncated: %d of %d bytes" % (len(blob) - 8, len(blob)), resume=blob[:-8])
    refused("checksum mismatch", resume=blob[:-8] + bytes(8 * [0x55]))
    with r.progressive(2, total=8, tiles=cells) as s:
        s.step()
        part = s.checkpoint()
    assert izpi_amd.checkpoint_info(part)["pixels"] == 32
    more = np.vstack([cells, [[13, 6, 13, 6]]])
    refused("1 pixels of the request have no record", tiles=more, resume=part)
    refused("1 of its records belong to no pixel of the request", tiles=cells[:-1], resume=part)
    refused("1 of its records belong to no pixel of the request", tiles=np.vstack([cells[:-1], cells[:1]]), resume=part)  # 32 entries, 31 pixels
    with r.progressive(2, total=8, tiles=cells[::-1], resume=part) as s:  # the same set in another order
        assert s.checkpoint() == part
    r.close()
    g = renderer("cornell", acc, SIZE, contexts=2)  # the group's own check of the pixel set
    for t, message in ((more, "1 pixels of the request have no record"), (cells[:-1], "1 of its records belong to no pixel")):
        with pytest.raises(RuntimeError, match=message):
            g.progressive(2, total=8, tiles=t, resume=part)
        assert L.izpi_gpu_multi_progressive_end(g.m) == N.IZPI_ERR_INVALID
    assert g.render().tobytes() == renderer_frame(acc)
    g.close()


@functools.lru_cache(maxsize=None)
def renderer_frame(acc):
    r = renderer("cornell", acc, SIZE)
    out = r.render().tobytes()
    r.close()
    return out


# ---- 6. izpi-render in child processes
@pytest.mark.parametrize("adaptive", [False, True])
def test_cli_resumes_in_another_process(gpu, tmp_path, adaptive):
    """--progressive 4 --stop-after 3 --checkpoint a, then --resume a: the files of the run that
    was never interrupted, byte for byte. Each child has its own time limit; a failed one ends the chain."""
    box = tmp_path / "box.pbtxt"
    box.write_text(configs.cornell_rgb_pbtxt(1.0))
    common = [str(build.CLI), "--scene", str(box), "--x", "40", "--y", "40", "--samples", "24", "--progressive", "4"]
    if adaptive:
        common += ["--noise-threshold", "0.25", "--noise-tolerated", "0.0", "--min-samples", "4", "--adaptive"]

    def run(tag, extra):
        outs = ["--out", str(tmp_path / (tag + ".pfm"))] + (["--samples-out", str(tmp_path / (tag + "_n.pfm"))] if adaptive else [])
        p = subprocess.run(common + outs + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        return [ln for ln in p.stderr.splitlines() if ln.startswith("IZPI_CHECKPOINT ")]

    ckpt = tmp_path / "a.ckpt"
    assert run("whole", []) == []
    lines = run("part", ["--stop-after", "3", "--checkpoint", str(ckpt)])
    assert len(lines) == 1 and lines[0].startswith("IZPI_CHECKPOINT wrote file=%s bytes=%d done=12" % (ckpt, ckpt.stat().st_size))
    info = izpi_amd.checkpoint_info(ckpt)
    assert (info["done"], info["adaptive"], info["spp"]) == (12, adaptive, 24)
    lines = run("rest", ["--resume", str(ckpt)])
    assert len(lines) == 1 and lines[0].startswith("IZPI_CHECKPOINT read file=%s bytes=%d done=12" % (ckpt, ckpt.stat().st_size))
    names = ["%s.pfm", "%s_n.pfm"] if adaptive else ["%s.pfm"]
    for name in names:
        whole, part, rest = [(tmp_path / (name % t)).read_bytes() for t in ("whole", "part", "rest")]
        assert rest == whole and part != whole
