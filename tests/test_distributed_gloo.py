"""Multi-rank path on CPU (gloo, world_size 2, 3 and 8): the library's own share plan,
the one izpi_gpu_render_rank runs — the units the frame is dealt in
(izpi_host_share_units), their deal (izpi_host_share_tiles), the padded block size
(izpi_host_share_block) and root assembly (izpi_host_assemble_shares, the host twin of
the device's k_unpack step) — with the blocks moved by a gloo gather and fed by oracle
renders of each rank's units. The assembled canvas must be bit-identical to a single-rank
render: per pixel-sample RNG streams make the image partition-independent (SURVEY.md
§8(e)); a Python restatement of the unpack rule cross-checks the library's."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

SPP = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_render(tiles, W, H):
    import ctypes as C
    from izpi_amd import _native as N
    from izpi_amd import configs
    from oracle import oracle as O
    o = O.OracleScene(configs.cornell_rgb(1.0), aspect_override=1.0)
    req = N.RenderReq(width=W, height=H, spp=SPP, max_depth=50, sampler=N.SAMPLER_COLOUR, seed=12345)
    t = np.ascontiguousarray(tiles, np.uint32)
    req.num_tiles = len(t)
    req.tiles = t.ctypes.data_as(C.POINTER(C.c_uint32))
    canvas, _ = o.render(req, threads=2)
    return canvas.reshape(H, W, 4)


def _worker(rank, world, port, outdir, W, H):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist
    from izpi_amd import sharding
    from oracle import oracle as O
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    all_tiles = sharding.share_units(O.tiles(W, H), world)  # (named as before: the units from here on)
    mine = sharding.shard_tiles(all_tiles, rank, world)
    packed = np.zeros(sharding.packed_len(all_tiles, world))
    if len(mine):
        part = sharding.pack_from_canvas(_oracle_render(mine, W, H), mine, H)
        packed[:part.size] = part
    got = sharding.gather_packed(torch.from_numpy(packed), rank, world)
    if rank == 0:
        blocks = np.concatenate([g.numpy() for g in got])
        canvas = sharding.assemble(all_tiles, world, blocks, W, H)
        check = np.zeros((H, W, 4))
        for r in range(world):
            rt = sharding.shard_tiles(all_tiles, r, world)
            if len(rt):
                sharding.unpack_into(check, rt, got[r].numpy()[:sharding.tile_pixels(rt) * 4], W, H)
        assert canvas.tobytes() == check.tobytes()
        np.save(os.path.join(outdir, "canvas_%d.npy" % world), canvas)
    dist.barrier()
    dist.destroy_process_group()


def _check_world(tmp_path, world, size, share_lens):
    from izpi_amd import sharding
    from oracle import oracle as O
    W = H = size
    units = sharding.share_units(O.tiles(W, H), world)
    assert sorted({len(sharding.shard_tiles(units, r, world)) for r in range(world)}) == share_lens
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), W, H), nprocs=world, join=True)
    got = np.load(tmp_path / ("canvas_%d.npy" % world))
    full = _oracle_render(O.tiles(W, H), W, H)
    assert got.tobytes() == full.tobytes()
    assert np.all(full[0] == 0) and np.all(full[1:, :, 3] == 1.0)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_sharded_gather_is_partition_independent(tmp_path, world):
    """64 x 64: 16 units of 16 x 16 in shares of 8, of 6 and 5, and of 2."""
    _check_world(tmp_path, world, 64, {2: [8], 3: [5, 6], 8: [2]}[world])


@pytest.mark.parametrize("size,share_lens", [(96, [4, 5]), (50, [0, 1])])
def test_sharded_gather_padded_and_empty_shares(tmp_path, size, share_lens):
    """Eight ranks. 96 x 96: 36 units in shares of 5 and 4, so the blocks are padded.
    50 x 50: 4 uncut tiles, so four ranks post empty (zero) blocks."""
    _check_world(tmp_path, 8, size, share_lens)
