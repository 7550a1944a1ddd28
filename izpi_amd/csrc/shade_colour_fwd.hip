// shade_colour_fwd.hip — the shading kernels of the Colour sampler, forward (IZPI_ACC_FORWARD) accumulation (shade.h).
#include "shade.h"

template const ShadeKernels* shade_kernels<IZPI_SAMPLER_COLOUR, true>(int);
