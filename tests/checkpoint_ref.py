"""The checkpoint of a progressive session, restated in numpy and the
struct module from the format's description alone: the 432-byte header, the word-wise FNV-1a
checksum, the frame-order planes, and pack / unpack between the packed order of a tile list and
those planes. Nothing here calls the C++.

Packed arrays are in the session's order (tile after tile, by sample row y then x); a plane
entry is y * W + x (sample rows, not canvas rows)."""
import struct

import numpy as np

from tests.noise_ref import packed_xy

MAGIC = b"IZPICKPT"
VERSION = 1
HEADER_BYTES = 432
MAX_COUNTERS = 32
CHECKSUM_FROM = 32
PROG_NOISE, PROG_ADAPTIVE = 1, 4
NOT_IN_SESSION = 255
MASK = (1 << 64) - 1
BASIS, PRIME = 0xcbf29ce484222325, 0x100000001b3

# name, struct format; in the header's order
FIELDS = [("magic", "8s"), ("version", "I"), ("header_bytes", "I"), ("blob_bytes", "Q"), ("checksum", "Q"),
          ("flags", "I"), ("listed", "I"), ("width", "I"), ("height", "I"), ("sampler", "I"), ("accumulation", "I"),
          ("max_depth", "I"), ("num_bg_spd", "I"), ("seed", "Q"), ("background", "3d"), ("ink", "3d"),
          ("bg_digest", "Q"), ("pixels", "Q"), ("scene_tag", "Q"), ("done", "I"), ("spp", "I"), ("samples", "Q"),
          ("active", "Q"), ("num_counters", "I"), ("pad", "I"), ("counters", "%dQ" % MAX_COUNTERS)]
HEADER = struct.Struct("<" + "".join(f for _, f in FIELDS))
assert HEADER.size == HEADER_BYTES


def hash_words(data, h=BASIS):
    """FNV-1a over little-endian 64-bit words; a tail shorter than a word is padded with zeros."""
    data = bytes(data)
    data += b"\0" * (-len(data) % 8)
    for (w,) in struct.iter_unpack("<Q", data):
        h = ((h ^ w) * PRIME) & MASK
    return h


def bg_digest(wavelengths, values):
    h = BASIS
    for a in (wavelengths, values):
        a = np.ascontiguousarray(a, np.float64)
        if a.size:
            h = hash_words(a.tobytes(), h)
    return h


def up8(n):
    return (n + 7) // 8 * 8


def layout(width, height, flags):
    """Offsets of the planes from the blob's start (0: a plane the session lacks) and the blob's size."""
    n = width * height
    off = {"state": HEADER_BYTES, "moments": 0, "counts": 0}
    off["sums"] = off["state"] + up8(n)
    end = off["sums"] + 24 * n
    if flags & PROG_NOISE:
        off["moments"], end = end, end + 24 * n
    if flags & PROG_ADAPTIVE:
        off["counts"], end = end, end + up8(4 * n)
    off["bytes"] = end
    return off


def pack(width, height, tiles, flags, done, sums, moment2=None, samples=None, state=None):
    """The planes (the blob's bytes after its header) of a session over `tiles`."""
    x, y = packed_xy(tiles)
    i = y * width + x
    n = width * height
    st = np.full(up8(n), 0, np.uint8)
    st[:n] = NOT_IN_SESSION
    st[i] = 0 if state is None else np.asarray(state, np.uint8)
    s = np.zeros((n, 3))
    s[i] = sums
    out = [st.tobytes(), s.tobytes()]
    if flags & PROG_NOISE:
        m = np.zeros((n, 3))
        m[i] = moment2
        out.append(m.tobytes())
    if flags & PROG_ADAPTIVE:
        c = np.zeros(up8(4 * n) // 4, np.uint32)
        c[i] = done if samples is None else np.asarray(samples, np.uint32)
        out.append(c.tobytes())
    return b"".join(out)


def unpack(width, height, tiles, flags, planes):
    """(sums, moment2, samples, state, absent, unclaimed) in the packed order of `tiles`; pixels
    without a record keep zeros."""
    off = layout(width, height, flags)
    n = width * height
    at = lambda name, dtype, count: np.frombuffer(planes, dtype, count, off[name] - HEADER_BYTES)
    st = at("state", np.uint8, n)
    x, y = packed_xy(tiles)
    i = y * width + x
    have = st[i] != NOT_IN_SESSION
    take = lambda a, shape, dtype: np.where(have.reshape((-1,) + (1,) * (len(shape) - 1)), a[i], np.zeros(1, dtype))
    sums = take(at("sums", np.float64, 3 * n).reshape(n, 3), (0, 3), np.float64)
    moment2 = take(at("moments", np.float64, 3 * n).reshape(n, 3), (0, 3), np.float64) if flags & PROG_NOISE else None
    samples = state = None
    if flags & PROG_ADAPTIVE:
        samples = take(at("counts", np.uint32, n), (0,), np.uint32).astype(np.uint32)
        state = take(st, (0,), np.uint8).astype(np.uint8)
    claimed = np.zeros(n, bool)
    claimed[i[have]] = True
    return sums, moment2, samples, state, int((~have).sum()), int(((st != NOT_IN_SESSION) & ~claimed).sum())


def build(planes, width, height, flags, done, *, listed=0, sampler=2, accumulation=0, max_depth=50, seed=12345,
          background=(0.0, 0.0, 0.0), ink=(0.0, 0.0, 0.0), bg_spd=((), ()), scene_tag=0, spp=None, samples=0, active=0,
          counters=()):
    """A whole blob around `planes`: the header with its sizes, the count of present records and
    the checksum."""
    n = width * height
    st = np.frombuffer(planes, np.uint8, n)
    fields = {"magic": MAGIC, "version": VERSION, "header_bytes": HEADER_BYTES, "blob_bytes": HEADER_BYTES + len(planes),
              "checksum": 0, "flags": flags, "listed": listed, "width": width, "height": height, "sampler": sampler,
              "accumulation": accumulation, "max_depth": max_depth, "num_bg_spd": len(bg_spd[0]), "seed": seed,
              "background": tuple(background), "ink": tuple(ink), "bg_digest": bg_digest(*bg_spd),
              "pixels": int((st != NOT_IN_SESSION).sum()), "scene_tag": scene_tag, "done": done,
              "spp": done if spp is None else spp, "samples": samples, "active": active, "num_counters": len(counters),
              "pad": 0, "counters": tuple(counters) + (0,) * (MAX_COUNTERS - len(counters))}
    assert fields["blob_bytes"] == layout(width, height, flags)["bytes"]
    return reseal(header_bytes(fields) + planes)


def header_bytes(fields):
    flat = []
    for name, fmt in FIELDS:
        v = fields[name]
        flat.extend(v if isinstance(v, tuple) else [v])
    return HEADER.pack(*flat)


def parse(blob):
    """The header's fields by name (tuples for background, ink and the counters)."""
    vals = list(HEADER.unpack_from(blob))
    out = {}
    for name, fmt in FIELDS:
        k = int(fmt[:-1]) if fmt[:-1] and fmt[-1] != "s" else 1
        out[name] = vals.pop(0) if k == 1 else tuple(vals.pop(0) for _ in range(k))
    return out


def reseal(blob, **changes):
    """`blob` with header fields changed and the checksum taken anew."""
    fields = parse(blob)
    fields.update(changes)
    body = header_bytes(dict(fields, checksum=0)) + blob[HEADER_BYTES:]
    fields["checksum"] = hash_words(body[CHECKSUM_FROM:])
    return header_bytes(fields) + blob[HEADER_BYTES:]
