"""The progressive-rendering entry points (include/izpi_gpu.h: izpi_gpu_progressive_*,
izpi_gpu_multi_progressive_*) without a GPU: exported, listed in the ctypes mirror, and a
NULL context or handle is IZPI_ERR_INVALID, not a crash."""
import ctypes as C

import numpy as np

from izpi_amd import _native as N
from tests.test_abi import declared_functions

SINGLE = ["izpi_gpu_progressive_begin", "izpi_gpu_progressive_step", "izpi_gpu_progressive_snapshot",
          "izpi_gpu_progressive_snapshot_device", "izpi_gpu_progressive_end"]
MULTI = ["izpi_gpu_multi_progressive_begin", "izpi_gpu_multi_progressive_step", "izpi_gpu_multi_progressive_snapshot",
         "izpi_gpu_multi_progressive_end"]


def test_entry_points_are_declared_exported_and_listed():
    L = N.lib()
    decl = declared_functions()
    for name in SINGLE + MULTI:
        assert name in decl, name
        assert hasattr(L, name), name
        assert name in N.EXPORTS, name
    assert (N.SNAP_CANVAS, N.SNAP_DISPLAY) == (0, 1)


def test_null_context_is_invalid():
    L = N.lib()
    req = N.RenderReq(width=8, height=8, spp=2, sampler=N.SAMPLER_COLOUR, abi_version=N.IZPI_ABI_VERSION)
    st = N.RenderStats()
    out = np.zeros(8 * 8 * 4)
    ptr = out.ctypes.data_as(C.c_void_p)
    for pre in ("izpi_gpu_progressive_", "izpi_gpu_multi_progressive_"):
        assert getattr(L, pre + "begin")(None, C.byref(req), 1) == N.IZPI_ERR_INVALID
        assert getattr(L, pre + "step")(None, 1, C.byref(st)) == N.IZPI_ERR_INVALID
        assert getattr(L, pre + "step")(None, 0, None) == N.IZPI_ERR_INVALID
        for form in (N.SNAP_CANVAS, N.SNAP_DISPLAY):
            assert getattr(L, pre + "snapshot")(None, form, ptr) == N.IZPI_ERR_INVALID
        assert getattr(L, pre + "end")(None) == N.IZPI_ERR_INVALID
    assert L.izpi_gpu_progressive_snapshot_device(None, N.SNAP_CANVAS, None) == N.IZPI_ERR_INVALID
    assert not out.any()
