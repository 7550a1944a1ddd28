"""izpi_amd — MI355X-native path-tracing inner loop for izpi (flynn-nrg/izpi).

Product pieces: izpi_amd/csrc (gfx950 HIP kernels + the C ABI of include/izpi_gpu.h,
C++ host scene producer of include/izpi_host.h), and this thin Python host mirror
(scene description, GPURenderer = render.Renderer drop-in, multi-GPU sharding).
"""
from . import _native  # noqa: F401
from .checkpoint import checkpoint_info  # noqa: F401  (a session's checkpoint as a dict; needs no GPU)

# sampler.go:22-28 (samplerMap): the names izpi's --sampler takes and render.New's SamplerType
# values, which are the IZPI_SAMPLER_* of include/izpi_gpu.h
SAMPLERS = {"colour": _native.SAMPLER_COLOUR, "normal": _native.SAMPLER_NORMAL,
            "wireframe": _native.SAMPLER_WIREFRAME, "albedo": _native.SAMPLER_ALBEDO,
            "spectral": _native.SAMPLER_SPECTRAL}

__all__ = ["_native", "scene", "configs", "renderer", "build", "checkpoint", "checkpoint_info", "SAMPLERS"]
