// Stand-in of this repository for CUDA's header of the same name (TEST INFRASTRUCTURE): see cuda_runtime.h.
#pragma once
#include "cuda_runtime.h"
