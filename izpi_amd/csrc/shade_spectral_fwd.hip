// shade_spectral_fwd.hip — the shading kernels of the Spectral sampler, forward (IZPI_ACC_FORWARD) accumulation (shade.h).
#include "shade.h"

template const ShadeKernels* shade_kernels<IZPI_SAMPLER_SPECTRAL, true>(int);
