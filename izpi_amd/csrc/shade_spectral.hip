// shade_spectral.hip — the shading kernels of the Spectral sampler, recursive (IZPI_ACC_RECURSIVE) accumulation (shade.h).
#include "shade.h"

template const ShadeKernels* shade_kernels<IZPI_SAMPLER_SPECTRAL, false>(int);
