"""The share plan on CPU: izpi_host_share_units (the units a frame's tiles are dealt in)
against an independent numpy restatement, and izpi_host_share_tiles' deal of those units.
The device deals with the same functions (make_shares in multi.hip); the GPU tests tie
each device's sample count to this plan."""
import numpy as np
import pytest

from izpi_amd import sharding
from izpi_amd.renderer import common_tiles


def split_tiles(tl, k=2):
    """Every tile cut k x k: the tile's order, then rows j, then columns i."""
    out = []
    for x0, y0, x1, y1 in np.asarray(tl).reshape(-1, 4):
        w, h = (x1 - x0 + 1) // k, (y1 - y0 + 1) // k
        for j in range(k):
            for i in range(k):
                out.append((x0 + i * w, y0 + j * h, x0 + i * w + w - 1, y0 + j * h + h - 1))
    return np.asarray(out, np.uint32)


def expected_units(tiles, world):
    t = np.asarray(tiles, np.int64)
    w, h = t[:, 2] - t[:, 0] + 1, t[:, 3] - t[:, 1] + 1
    cut = world > 1 and np.all(w == w[0]) and np.all(h == h[0]) and w[0] % 2 == 0 and h[0] % 2 == 0 and w[0] >= 16 and h[0] >= 16
    return split_tiles(tiles) if cut else np.asarray(tiles, np.uint32)


def coverage(tiles, W, H):
    n = np.zeros((H, W), np.int64)
    for x0, y0, x1, y1 in np.asarray(tiles, np.int64):
        n[y0:y1 + 1, x0:x1 + 1] += 1
    return n


# frame -> (tiles, tile extent, units when cut)
FRAMES = {(64, 64): (4, 32, 16), (96, 96): (9, 32, 36), (1024, 1024): (1024, 32, 4096),
          (50, 50): (4, 25, 4),    # odd tiles: no cut
          (56, 56): (49, 8, 49)}   # tiles below 16 x 16: no cut


@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("world", [1, 2, 3, 7, 8])
def test_share_units_and_their_deal(frame, world):
    W, H = frame
    ntiles, extent, nunits = FRAMES[frame]
    tiles = common_tiles(W, H)
    assert len(tiles) == ntiles and tiles[0, 2] - tiles[0, 0] + 1 == extent
    units = sharding.share_units(tiles, world)
    assert len(units) == (nunits if world > 1 else ntiles)
    assert units.tobytes() == expected_units(tiles, world).tobytes()  # the rule, order included
    if len(units) != ntiles:  # cut: unit 4 t + 2 j + i is quarter (j, i) of tile t
        half = extent // 2
        assert np.all(units[:, 2] - units[:, 0] + 1 == half) and np.all(units[:, 3] - units[:, 1] + 1 == half)
        for k in range(4):
            assert np.array_equal(units[k::4, 0], tiles[:, 0] + (k % 2) * half)
            assert np.array_equal(units[k::4, 1], tiles[:, 1] + (k // 2) * half)
    assert np.all(coverage(units, W, H) == 1)  # every pixel of the frame in exactly one unit
    parts = [sharding.shard_tiles(units, r, world) for r in range(world)]
    for r, p in enumerate(parts):
        assert np.array_equal(p, units[r::world])
    total = np.zeros((H, W), np.int64)
    for p in parts:
        total += coverage(p, W, H) if len(p) else 0
    assert np.all(total == 1)  # disjoint, and they cover the frame
    assert max(len(p) for p in parts) == -(-len(units) // world)
    assert sharding.packed_len(units, world) == -(-len(units) // world) * sharding.tile_pixels(units[:1]) * 4


def test_share_units_leaves_unequal_tiles_alone():
    tiles = np.array([[0, 0, 31, 31], [32, 0, 47, 31]], np.uint32)
    assert sharding.share_units(tiles, 4).tobytes() == tiles.tobytes()


def test_three_shares_of_64x64_differ_from_whole_tiles():
    """The counts the GPU test's per-device assertion expects: 16 units of 16 x 16 over three
    shares are 6 / 5 / 5 units (1536 / 1280 / 1280 pixels), where whole tiles give 2048 /
    1024 / 1024."""
    tiles = common_tiles(64, 64)
    units = sharding.share_units(tiles, 3)
    assert [sharding.tile_pixels(sharding.shard_tiles(units, r, 3)) for r in range(3)] == [1536, 1280, 1280]
    assert [sharding.tile_pixels(sharding.shard_tiles(tiles, r, 3)) for r in range(3)] == [2048, 1024, 1024]
