// cuda_runtime.h — this repository's own stand-in for the CUDA runtime header (TEST INFRASTRUCTURE), so that the reference's
// sources compile with g++ and run on the CPU (oracle/build.py build_ref -> oracle/_ref/libref_probe.so).
//   * __device__, __host__, __global__ are defined away: every function of the reference is an ordinary C++ function;
//   * dim3, uchar3, uchar4, uint3; threadIdx, blockIdx, blockDim, gridDim are globals that REF_LAUNCH sets;
//   * cudaMalloc / cudaMemcpy / cudaFree act on host memory, the event calls on a steady clock;
//   * REF_LAUNCH(kernel, grid, block, args...) replaces kernel<<<grid, block>>>(args...): it calls the kernel once per thread of
//     the grid. Blocks run in parallel under OpenMP (the index variables are thread-local); the reference's kernels neither
//     synchronise nor share memory between threads, so the order does not matter;
//   * clock64() returns ref_clock_seed, which the driver sets: the reference seeds cuRAND with the clock (CudaTracer.cu:28).
#pragma once
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdlib.h>

// The reference defines M_PI itself, as a float literal, where the platform's <cmath> has not (RenderStructs.h:9-11): that is the
// case it was written for. <cmath> is complete by now, so no later #include brings the double one back.
#undef M_PI
using std::abs;   // abs(float) must be the float overload, as in CUDA (CudaTracer.cu:273-276, 508)

#define __device__
#define __host__
#define __global__

struct uchar3 { unsigned char x, y, z; };
struct uchar4 { unsigned char x, y, z, w; };
struct uint3 { unsigned int x, y, z; };
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

inline thread_local uint3 threadIdx = {0, 0, 0};
inline thread_local uint3 blockIdx = {0, 0, 0};
inline dim3 blockDim;
inline dim3 gridDim;

template <class Body>
inline void ref_launch(dim3 grid, dim3 block, Body body) {
    gridDim = grid;
    blockDim = block;
    const long blocks = (long)grid.x * grid.y * grid.z;
#pragma omp parallel for schedule(dynamic, 16)
    for (long b = 0; b < blocks; ++b) {
        blockIdx.x = (unsigned)(b % grid.x);
        blockIdx.y = (unsigned)((b / grid.x) % grid.y);
        blockIdx.z = (unsigned)(b / ((long)grid.x * grid.y));
        for (unsigned tz = 0; tz < block.z; ++tz)
            for (unsigned ty = 0; ty < block.y; ++ty)
                for (unsigned tx = 0; tx < block.x; ++tx) {
                    threadIdx.x = tx;
                    threadIdx.y = ty;
                    threadIdx.z = tz;
                    body();
                }
    }
}
#define REF_LAUNCH(kernel, grid, block, ...) ref_launch(dim3(grid), dim3(block), [&]() { kernel(__VA_ARGS__); })

inline unsigned long long ref_clock_seed = 0;
inline long long clock64() { return (long long)ref_clock_seed; }

typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
inline const char* cudaGetErrorString(cudaError_t) { return "host stand-in"; }
inline cudaError_t cudaMalloc(void** p, size_t n) { *p = std::calloc(n ? n : 1, 1); return *p ? cudaSuccess : 2; }
template <class T> inline cudaError_t cudaMalloc(T** p, size_t n) { return cudaMalloc((void**)p, n); }
inline cudaError_t cudaMemcpy(void* dst, const void* src, size_t n, cudaMemcpyKind) { if (n) std::memcpy(dst, src, n); return cudaSuccess; }
inline cudaError_t cudaFree(void* p) { std::free(p); return cudaSuccess; }

struct cudaDeviceProp { int major, minor; };
inline cudaError_t cudaChooseDevice(int* dev, const cudaDeviceProp*) { *dev = 0; return cudaSuccess; }

typedef std::chrono::steady_clock::time_point* cudaEvent_t;
inline cudaError_t cudaEventCreate(cudaEvent_t* e) { *e = new std::chrono::steady_clock::time_point(); return cudaSuccess; }
inline cudaError_t cudaEventDestroy(cudaEvent_t e) { delete e; return cudaSuccess; }
inline cudaError_t cudaEventRecord(cudaEvent_t e) { *e = std::chrono::steady_clock::now(); return cudaSuccess; }
inline cudaError_t cudaEventSynchronize(cudaEvent_t) { return cudaSuccess; }
inline cudaError_t cudaEventElapsedTime(float* ms, cudaEvent_t a, cudaEvent_t b) {
    *ms = std::chrono::duration<float, std::milli>(*b - *a).count();
    return cudaSuccess;
}
