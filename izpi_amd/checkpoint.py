"""A progressive session's checkpoint on the host (include/izpi_host.h): reading
a blob's header, the validation a resume runs, the host twins of the two reorder kernels, and
the scene tag. None of it needs a GPU. The blob itself comes from
``ProgressiveSession.checkpoint()`` and goes back in through ``progressive(..., resume=blob)``."""
import ctypes as C
import os

import numpy as np

from . import _native as N


def _host(name, *args):
    L = N.lib()
    rc = getattr(L, "izpi_host_" + name)(*args)
    if rc != 0:
        raise RuntimeError("izpi_host_%s failed (status %d): %s" % (name, rc, L.izpi_host_last_error().decode()))


def _void(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load(blob_or_path):
    """A checkpoint as bytes: the blob itself, or the contents of the file it names."""
    if isinstance(blob_or_path, (bytes, bytearray, memoryview)):
        return bytes(blob_or_path)
    with open(os.fspath(blob_or_path), "rb") as f:
        return f.read()


def save(blob, path):
    """Write `blob` to `path` through a temporary file beside it and a rename: a reader finds
    the old checkpoint or the new one, never a part of either."""
    path = os.fspath(path)
    tmp = "%s.tmp%d" % (path, os.getpid())
    with open(tmp, "wb") as f:
        f.write(blob)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def _field(blob, which):
    out = C.c_uint64()
    _host("checkpoint_field", blob, len(blob), which, C.byref(out))
    return out.value


def checkpoint_info(blob):
    """The header of a checkpoint (bytes or a path) as a dict: izpi_host_checkpoint_field's
    scalars by name (N.CKPT_FIELDS), `background` and `ink` as tuples of floats, `counters` as a
    list, and `noise` / `adaptive` from the flags. Raises on a blob that is no checkpoint."""
    blob = load(blob)
    info = {name: _field(blob, k) for k, name in enumerate(N.CKPT_FIELDS)}
    as_float = lambda base: tuple(float(np.array(_field(blob, base + k), np.uint64).view(np.float64)) for k in range(3))
    info["background"], info["ink"] = as_float(N.CKPT_BACKGROUND), as_float(N.CKPT_INK)
    info["counters"] = [_field(blob, N.CKPT_COUNTER + k) for k in range(info["num_counters"])]
    info["noise"] = bool(info["flags"] & N.PROG_NOISE)
    info["adaptive"] = bool(info["flags"] & N.PROG_ADAPTIVE)
    return info


def check(blob, req, scene_tag):
    """izpi_host_checkpoint_check: raises with the refusal's message unless `blob` can resume
    under the request `req` (an N.RenderReq) and `scene_tag`."""
    _host("checkpoint_check", blob, len(blob), C.byref(req), int(scene_tag))


def scene_tag(desc):
    """izpi_host_scene_tag of an izpi_scene_desc (HostScene.desc)."""
    out = C.c_uint64()
    _host("scene_tag", C.byref(desc), C.byref(out))
    return out.value


def _tiles(tiles):
    t = np.ascontiguousarray(tiles, np.uint32).reshape(-1, 4)
    return t, t.ctypes.data_as(N.c_uint32_p), len(t)


def pack(width, height, tiles, flags, done, sums, moment2=None, samples=None, state=None):
    """izpi_host_checkpoint_pack: a session's state in the packed order of `tiles` ((n, 3) sums
    and moments, (n,) uint32 samples and uint8 state, or None for both: every pixel active with
    `done` samples) as the frame-order planes of a blob (its bytes after the header)."""
    t, tp, nt = _tiles(tiles)
    sums = np.ascontiguousarray(sums, np.float64)
    moment2 = None if moment2 is None else np.ascontiguousarray(moment2, np.float64)
    samples = None if samples is None else np.ascontiguousarray(samples, np.uint32)
    state = None if state is None else np.ascontiguousarray(state, np.uint8)
    need = C.c_uint64()
    _host("checkpoint_pack", width, height, tp, nt, flags, done, None, None, None, None, None, 0, C.byref(need))
    out = np.zeros(need.value, np.uint8)
    _host("checkpoint_pack", width, height, tp, nt, flags, done, _void(sums), _void(moment2), _void(samples),
          _void(state), _void(out), out.size, None)
    return out.tobytes()


def unpack(width, height, tiles, flags, planes):
    """izpi_host_checkpoint_unpack: the frame-order planes into the packed order of `tiles`.
    Returns (sums, moment2 or None, samples or None, state or None, absent, unclaimed)."""
    t, tp, nt = _tiles(tiles)
    n = int(nt * (t[0, 2] - t[0, 0] + 1) * (t[0, 3] - t[0, 1] + 1)) if nt else 0
    sums = np.zeros((n, 3), np.float64)
    moment2 = np.zeros((n, 3), np.float64) if flags & N.PROG_NOISE else None
    samples = np.zeros(n, np.uint32) if flags & N.PROG_ADAPTIVE else None
    state = np.zeros(n, np.uint8) if flags & N.PROG_ADAPTIVE else None
    absent, unclaimed = C.c_uint64(), C.c_uint64()
    _host("checkpoint_unpack", width, height, tp, nt, flags, planes, len(planes), _void(sums), _void(moment2),
          _void(samples), _void(state), C.byref(absent), C.byref(unclaimed))
    return sums, moment2, samples, state, absent.value, unclaimed.value
