// Stand-in of this repository for CUDA's header of the same name (TEST INFRASTRUCTURE): the graphics-interop calls of the
// reference's window code only have to compile; none of them is ever called by oracle/ref_probe.cpp.
#pragma once
#include "cuda_runtime.h"
struct cudaGraphicsResource;
enum { cudaGraphicsMapFlagsNone = 0 };
inline cudaError_t cudaGLSetGLDevice(int) { return cudaSuccess; }
inline cudaError_t cudaGraphicsGLRegisterBuffer(cudaGraphicsResource**, unsigned, unsigned) { return cudaSuccess; }
inline cudaError_t cudaGraphicsUnregisterResource(cudaGraphicsResource*) { return cudaSuccess; }
inline cudaError_t cudaGraphicsMapResources(int, cudaGraphicsResource**, void*) { return cudaSuccess; }
inline cudaError_t cudaGraphicsUnmapResources(int, cudaGraphicsResource**, void*) { return cudaSuccess; }
inline cudaError_t cudaGraphicsResourceGetMappedPointer(void** p, size_t* n, cudaGraphicsResource*) { *p = nullptr; *n = 0; return cudaSuccess; }
