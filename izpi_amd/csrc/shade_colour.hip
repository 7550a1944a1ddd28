// shade_colour.hip — the shading kernels of the Colour sampler, recursive (IZPI_ACC_RECURSIVE) accumulation (shade.h).
#include "shade.h"

template const ShadeKernels* shade_kernels<IZPI_SAMPLER_COLOUR, false>(int);
