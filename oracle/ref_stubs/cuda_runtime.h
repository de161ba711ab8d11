/*
 * cuda_runtime.h -- TEST INFRASTRUCTURE: a host stand-in for the part of the CUDA runtime API that a single-threaded
 * g++ build of a CUDA translation unit needs (oracle/Makefile target _ref/realtime_harness).  It describes the CUDA
 * API; it holds nothing of any program that uses it.  Function-space qualifiers are empty, the vector types are plain
 * structs, and the built-in index variables are ordinary globals that the caller sets before it calls a __global__
 * function as a host function: one "thread" at a time.
 */
#ifndef RT_STUB_CUDA_RUNTIME_H
#define RT_STUB_CUDA_RUNTIME_H

#include <math.h>
#include <stddef.h>

#define __device__
#define __host__
#define __global__
#define __inline__ inline

struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct int4 { int x, y, z, w; };
struct uint3 { unsigned int x, y, z; };
struct uchar4 { unsigned char x, y, z, w; };
struct dim3 { unsigned int x = 1, y = 1, z = 1; };

static inline float2 make_float2(float x, float y) { return float2{x, y}; }
static inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
static inline int2 make_int2(int x, int y) { return int2{x, y}; }
static inline int3 make_int3(int x, int y, int z) { return int3{x, y, z}; }
static inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
static inline uint3 make_uint3(unsigned int x, unsigned int y, unsigned int z) { return uint3{x, y, z}; }
static inline uchar4 make_uchar4(unsigned char x, unsigned char y, unsigned char z, unsigned char w) { return uchar4{x, y, z, w}; }

/* threadIdx and friends: set by the host code that plays the launch */
inline uint3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0};
inline dim3 blockDim, gridDim;

/* the min / max overload set of CUDA's math headers, mixed float / double included: the floating forms are fmin / fmax
 * (a NaN operand loses), the mixed forms promote to double */
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
static inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
static inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }
static inline float min(float a, float b) { return fminf(a, b); }
static inline float max(float a, float b) { return fmaxf(a, b); }
static inline double min(double a, double b) { return fmin(a, b); }
static inline double max(double a, double b) { return fmax(a, b); }
static inline double min(float a, double b) { return fmin((double)a, b); }
static inline double min(double a, float b) { return fmin(a, (double)b); }
static inline double max(float a, double b) { return fmax((double)a, b); }
static inline double max(double a, float b) { return fmax(a, (double)b); }
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }

typedef int cudaError_t;
enum { cudaSuccess = 0 };
static inline const char *cudaGetErrorString(cudaError_t) { return "stand-in"; }

#endif
