"""The checkpoint of a progressive session without a GPU: the host twins of the
reorder kernels and the blob's reader against tests/checkpoint_ref.py (numpy and struct, from the
format's description), every refusal that needs no device with its message, the scene tag, the
entries' declarations, a stand-alone program under AddressSanitizer and UBSan, and the
command-line tool's argument rules."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import izpi_amd
from izpi_amd import _native as N
from izpi_amd import build, checkpoint, configs
from izpi_amd.renderer import common_tiles, make_request
from izpi_amd.scene import HostScene
from tests import checkpoint_ref as CR
from tests.noise_ref import packed_xy
from tests.test_abi import declared_functions

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"
FLAGS = {"plain": 0, "noise": N.PROG_NOISE, "adaptive": N.PROG_NOISE | N.PROG_ADAPTIVE}
TILESETS = {
    "frame_40x30": (40, 30, None),  # the whole frame in common.Tiles order
    "two_16x16": (40, 32, [[16, 16, 31, 31], [0, 0, 15, 15]]),
    "overlapping": (40, 30, [[3, 2, 12, 9], [8, 5, 17, 12]]),
    "1x1": (1, 1, [[0, 0, 0, 0]]),
    "1x7": (1, 7, [[0, 0, 0, 6]]),
}


def tiles_of(name):
    W, H, tiles = TILESETS[name]
    return W, H, np.asarray(common_tiles(W, H) if tiles is None else tiles, np.uint32)


def session_state(W, tiles, kind, seed=0):
    """Random packed state of a session over `tiles`; a pixel of two tiles has one state."""
    rng = np.random.default_rng(seed)
    x, y = packed_xy(tiles)
    key = y * W + x
    per_pixel = lambda a: a[key]  # (drawn per frame entry, so that duplicates agree)
    n = int(key.max()) + 1
    sums = per_pixel(rng.random((n, 3)) * 8)
    m2 = per_pixel(rng.random((n, 3)) * 64) if kind != "plain" else None
    samples = state = None
    if kind == "adaptive":
        state = per_pixel(rng.integers(0, 3, n).astype(np.uint8))
        samples = per_pixel(rng.integers(2, 12, n).astype(np.uint32))
        samples = np.where(state == 0, 12, samples).astype(np.uint32)
    return sums, m2, samples, state


@pytest.mark.parametrize("kind", list(FLAGS))
@pytest.mark.parametrize("tileset", list(TILESETS))
def test_pack_and_unpack_match_the_reference(tileset, kind):
    W, H, tiles = tiles_of(tileset)
    flags = FLAGS[kind]
    sums, m2, samples, state = session_state(W, tiles, kind)
    want = CR.pack(W, H, tiles, flags, 12, sums, m2, samples, state)
    got = checkpoint.pack(W, H, tiles, flags, 12, sums, m2, samples, state)
    assert len(got) == CR.layout(W, H, flags)["bytes"] - CR.HEADER_BYTES
    assert got == want
    out, ref = checkpoint.unpack(W, H, tiles, flags, got), CR.unpack(W, H, tiles, flags, want)
    assert out[4:] == ref[4:] == (0, 0)
    for a, b, orig in zip(out[:4], ref[:4], (sums, m2, samples, state)):
        assert (a is None) == (b is None) == (orig is None)
        if a is not None:
            assert a.tobytes() == b.tobytes() == np.ascontiguousarray(orig).tobytes()
    # pack -> unpack -> pack is the identity
    assert checkpoint.pack(W, H, tiles, flags, 12, *out[:4]) == got


def test_adaptive_session_before_any_retirement_packs_done():
    W, H, tiles = tiles_of("two_16x16")
    flags = FLAGS["adaptive"]
    sums, m2, _, _ = session_state(W, tiles, "noise")
    got = checkpoint.pack(W, H, tiles, flags, 7, sums, m2)
    assert got == CR.pack(W, H, tiles, flags, 7, sums, m2)
    _, _, samples, state, _, _ = checkpoint.unpack(W, H, tiles, flags, got)
    assert (samples == 7).all() and not state.any()


def test_unpack_counts_the_pixels_without_a_record_and_the_records_without_a_pixel():
    W, H, tiles = tiles_of("two_16x16")
    sums = session_state(W, tiles, "plain")[0]
    planes = checkpoint.pack(W, H, tiles, 0, 3, sums)
    ones = lambda t: np.array([[x, y, x, y] for x, y in zip(*packed_xy(t))], np.uint32)  # (a list's tiles are equal-sized)
    for req_tiles, want in ((np.vstack([ones(tiles), [[32, 0, 32, 0]]]), (1, 0)), (ones(tiles)[:-1], (0, 1)),
                            (ones(tiles)[::-1], (0, 0))):
        got = checkpoint.unpack(W, H, req_tiles, 0, planes)
        assert got[4:] == want == CR.unpack(W, H, req_tiles, 0, planes)[4:]


# ---------------------------------------------------------------- the header
def small_blob(kind="adaptive", **kw):
    W, H, tiles = tiles_of("two_16x16")
    flags = FLAGS[kind]
    sums, m2, samples, state = session_state(W, tiles, kind)
    planes = CR.pack(W, H, tiles, flags, 12, sums, m2, samples, state)
    args = dict(listed=1, sampler=N.SAMPLER_SPECTRAL, accumulation=N.ACC_FORWARD, max_depth=17, seed=(1 << 63) + 5,
                background=(0.25, 0.5, 1.0), ink=(0.125, 0.0, 2.0), bg_spd=(np.array([400.0, 500.0, 700.0]), np.array([1.0, 0.5, 0.25])),
                scene_tag=0xDEADBEEF12345678, spp=64, samples=9999, active=77, counters=tuple(range(100, 129)))
    args.update(kw)
    return CR.build(planes, W, H, flags, 12, **args), (W, H, tiles, args)


def request_for(W, H, tiles, args, **kw):
    a = dict(args, **kw)
    return make_request(W, H, a["spp"], a["max_depth"], a["sampler"], a["background"], a["seed"], 1.0,
                        tuple(np.ascontiguousarray(v, np.float64) for v in a["bg_spd"]), tiles, N.OUT_PACKED,
                        accumulation=a["accumulation"], ink=a["ink"])


def test_a_blob_built_by_the_reference_parses_field_by_field():
    blob, (W, H, tiles, args) = small_blob()
    info = izpi_amd.checkpoint_info(blob)
    want = CR.parse(blob)
    for name in N.CKPT_FIELDS:
        if name.endswith("_offset"):
            assert info[name] == CR.layout(W, H, want["flags"])[name[:-7]]
        else:
            assert info[name] == want[name], name
    assert info["background"] == want["background"] == (0.25, 0.5, 1.0) and info["ink"] == want["ink"]
    assert tuple(info["counters"]) == want["counters"][:29] == tuple(range(100, 129))
    assert info["noise"] and info["adaptive"] and info["pixels"] == 512 and info["blob_bytes"] == len(blob)
    assert want["checksum"] == CR.hash_words(blob[CR.CHECKSUM_FROM:])
    checkpoint.check(blob, request_for(W, H, tiles, args), args["scene_tag"])  # ... and is this request's


def refusal(blob, req, tag):
    L = N.lib()
    rc = L.izpi_host_checkpoint_check(blob, len(blob), C.byref(req), tag)
    return rc, L.izpi_host_last_error().decode()


@pytest.mark.parametrize("field,value", [("width", 41), ("height", 33), ("sampler", N.SAMPLER_COLOUR),
                                         ("accumulation", N.ACC_RECURSIVE), ("max_depth", 18), ("seed", 6),
                                         ("background", (0.25, 0.5, 1.5)), ("ink", (0.125, -0.0, 2.0)),
                                         ("bg_spd", (np.array([400.0, 500.0, 700.0]), np.array([1.0, 0.5, 0.5]))),
                                         ("bg_spd", (np.array([400.0, 500.0]), np.array([1.0, 0.5]))),
                                         ("bg_spd", (np.zeros(0), np.zeros(0)))])
def test_each_deciding_field_alone_is_refused_by_name(field, value):
    blob, (W, H, tiles, args) = small_blob()
    W2, H2 = (value if field == "width" else W), (value if field == "height" else H)
    rc, msg = refusal(blob, request_for(W2, H2, tiles, args, **({} if field in ("width", "height") else {field: value})),
                      args["scene_tag"])
    assert rc == N.IZPI_ERR_INVALID and msg == "checkpoint: the request's %s differs from the checkpoint's" % field, msg


def test_fields_that_do_not_decide_a_sample_may_differ():
    blob, (W, H, tiles, args) = small_blob()
    req = request_for(W, H, tiles[::-1], args, spp=12)  # the other tile order, the cap at done
    req.out_layout, req.post, req.exposure = N.OUT_CANVAS, N.POST_GAMMA_CLAMP, 3.0
    rc, msg = refusal(blob, req, args["scene_tag"])
    assert rc == 0, msg


def test_the_other_refusals_that_need_no_device():
    blob, (W, H, tiles, args) = small_blob()
    req, tag = request_for(W, H, tiles, args), args["scene_tag"]
    cases = [
        (blob[:100], req, tag, "checkpoint: truncated within the header"),
        (blob[:CR.HEADER_BYTES + 1000], req, tag, "checkpoint: truncated: 1432 of %d bytes" % len(blob)),
        (blob[:-1], req, tag, "checkpoint: truncated: %d of %d bytes" % (len(blob) - 1, len(blob))),
        (blob + b"\0", req, tag, "checkpoint: bytes past the blob's end"),
        (b"X" + blob[1:], req, tag, "checkpoint: bad magic"),
        (blob[:8] + b"\2" + blob[9:], req, tag, "checkpoint: unknown format version"),
        (blob[:700] + bytes([blob[700] ^ 1]) + blob[701:], req, tag, "checkpoint: checksum mismatch"),
        (blob[:40] + bytes([blob[40] ^ 1]) + blob[41:], req, tag, "checkpoint: its size does not match its planes"),  # width, unsealed
        (blob[:60] + bytes([blob[60] ^ 1]) + blob[61:], req, tag, "checkpoint: checksum mismatch"),  # num_bg_spd, unsealed
        (blob, req, tag + 1, "checkpoint: the scene tag differs (another scene)"),
        (blob, request_for(W, H, tiles, args, spp=11), tag, "checkpoint: spp 11 is below the 12 samples done"),
        (CR.reseal(blob, done=0), req, tag, "checkpoint: no sample in it (done == 0)"),
        (CR.reseal(blob, flags=N.PROG_ADAPTIVE), req, tag, "checkpoint: unknown session flags"),
    ]
    for b, r, t, want in cases:
        rc, msg = refusal(b, r, t)
        assert (rc, msg) == (N.IZPI_ERR_INVALID, want), (want, rc, msg)
    with pytest.raises(RuntimeError, match="bad magic"):
        izpi_amd.checkpoint_info(b"\0" * 500)


# ---------------------------------------------------------------- the scene tag
def tag_after(scene, change=None, **kw):
    h = HostScene(scene, **kw)
    if change:
        change(h.desc)
    tag = checkpoint.scene_tag(h.desc)
    h.close()
    return tag


def test_scene_tag():
    pbr, glass = configs.cornell_pbr(1.5, res=8), configs.cornell_glass_spectral()
    base = tag_after(pbr)
    assert base == tag_after(configs.cornell_pbr(1.5, res=8)) and base != tag_after(glass)  # two builds of one scene

    def bump(array, k=0):
        def change(d):
            a = getattr(d, array)
            a[k] = a[k] + 1.0
        return change

    def node(d):
        d.nodes[0].min_x[0] -= 1.0

    def camera(d):
        d.camera.origin[1] += 0.5

    def material(d):
        d.materials[1].fuzz += 0.25

    seen = {base}
    for change in (bump("tri_v1", 4), bump("texels", 9), material, camera, node):
        t = tag_after(pbr, change)
        assert t not in seen, change
        seen.add(t)
    gbase = tag_after(glass)
    assert tag_after(glass, bump("spd_values", 3)) != gbase and tag_after(glass, bump("spd_wavelengths", 1)) != gbase


# ---------------------------------------------------------------- the entries
ENTRIES = ["checkpoint_bytes", "checkpoint", "resume"]
HOST = ["izpi_host_checkpoint_field", "izpi_host_checkpoint_check", "izpi_host_checkpoint_pack",
        "izpi_host_checkpoint_unpack", "izpi_host_scene_tag"]


def test_entry_points_are_declared_exported_and_listed():
    L = N.lib()
    decl = declared_functions()
    for name in ["izpi_gpu_progressive_" + e for e in ENTRIES] + ["izpi_gpu_multi_progressive_" + e for e in ENTRIES] + HOST:
        assert name in decl and name in N.EXPORTS and hasattr(L, name), name
    assert L.izpi_abi_struct_size(21) == 0 and N.IZPI_ABI_VERSION == 4  # no struct joined the numbered ones


def test_null_context_and_null_arguments_are_invalid():
    L = N.lib()
    blob, (W, H, tiles, args) = small_blob()
    req, n = request_for(W, H, tiles, args), C.c_uint64()
    buf = C.create_string_buffer(len(blob))
    for pre in ("izpi_gpu_progressive_", "izpi_gpu_multi_progressive_"):
        assert getattr(L, pre + "checkpoint_bytes")(None, C.byref(n)) == N.IZPI_ERR_INVALID
        assert getattr(L, pre + "checkpoint")(None, 1, buf, len(blob)) == N.IZPI_ERR_INVALID
        assert getattr(L, pre + "resume")(None, C.byref(req), 4, args["scene_tag"], blob, len(blob)) == N.IZPI_ERR_INVALID
    assert L.izpi_host_checkpoint_field(None, 0, 0, C.byref(n)) == N.IZPI_ERR_INVALID
    assert L.izpi_host_checkpoint_field(blob, len(blob), 9999, C.byref(n)) == N.IZPI_ERR_INVALID
    assert L.izpi_host_checkpoint_check(blob, len(blob), None, 0) == N.IZPI_ERR_INVALID
    assert L.izpi_host_scene_tag(None, C.byref(n)) == N.IZPI_ERR_INVALID


def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "checkpoint_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "checkpoint_check.cpp"),
                    str(CSRC / "checkpoint_host.cpp"), str(CSRC / "host_scene.cpp"), str(CSRC / "scene_pack.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])  # a sanitizer report ends the program
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok" and len(lines) > 10, lines[-5:]
    assert not [ln for ln in lines[:-1] if not ln.startswith("pass ")], lines


# ---------------------------------------------------------------- izpi-render
@pytest.mark.parametrize("args,message", [
    (["--checkpoint", "a.ckpt"], "--checkpoint needs --progressive"),
    (["--resume", "a.ckpt"], "--resume needs --progressive"),
    (["--stop-after", "2"], "--stop-after needs --progressive"),
    (["--progressive", "4", "--stop-after", "0"], "--stop-after takes at least 1 step"),
    (["--progressive", "4", "--checkpoint"], "missing value for --checkpoint"),
])
def test_command_line_argument_rules(args, message):
    build.build_cli(verbose=False)
    run = subprocess.run([str(build.CLI), "--scene", "none.pbtxt"] + args, capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and run.stderr.strip() == "izpi-render: " + message, run.stderr
