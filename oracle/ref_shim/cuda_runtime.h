// Host stand-in for <cuda_runtime.h>, used only to compile the reference's own source files for
// the CPU (oracle/ref_wrap.cpp, `make -C oracle ref`).  TEST INFRASTRUCTURE ONLY.
//
// It supplies the CUDA vocabulary the reference's hot path uses and nothing else.  Wherever a host
// compiler would silently pick something other than what nvcc compiles for the device, the choice
// is pinned here and the reason written next to it.
#pragma once

// Every standard header the reference's files use, here and up front: some arrive only through
// MSVC's transitive includes in the original build (memcpy, std::numeric_limits in BVH.cpp), and all
// of them must be seen before the math macros at the end of this file are defined.
#include <algorithm>
#include <cassert>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#define __host__
#define __device__
#define __global__

// Material::sample reads its texture only under `#if __CUDA_ARCH__` (Material.inl:26-35): without
// this the host build would shade every textured object with its plain base colour.  Defined for
// every translation unit alike, so the inline function has one body.
#define __CUDA_ARCH__ 520

// CUDA's float4 is 16-byte aligned: sizeof(Hittable) is 96, not 92 (checked in ref_wrap.cpp).
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(4) uchar4 { unsigned char x, y, z, w; };
struct uint3 { unsigned int x, y, z; };
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

// One "thread" runs at a time per host thread; ref_wrap.cpp sets these before each kernel call.
inline thread_local uint3 threadIdx = { 0, 0, 0 };
inline thread_local uint3 blockIdx = { 0, 0, 0 };
inline thread_local dim3 blockDim(1, 1, 1);

// A texture object is a pointer to liboracle.so's texture record (or_texture in pt_oracle.c).
typedef unsigned long long cudaTextureObject_t;
struct ptref_texture { uint32_t width, height; const float *texels; };

// The three third-party pieces the reference's source does not contain come from liboracle.so:
// CUDA's libm, the bilinear sampler (below) and cuRAND XORWOW (curand_kernel.h).
extern "C" {
float pm_sinf(float);
float pm_cosf(float);
float pm_acosf(float);
float pm_atan2f(float, float);
float pm_powf(float, float);
void or_tex2d(const ptref_texture *, float, float, float *);
}

template <class T> T tex2D(cudaTextureObject_t, float, float);
template <> inline float4 tex2D<float4>(cudaTextureObject_t t, float u, float v)
{
    float4 r;
    or_tex2d(reinterpret_cast<const ptref_texture *>(static_cast<uintptr_t>(t)), u, v, &r.x);
    return r;
}

namespace ptref_shim {
// True while a kernel runs (ref_wrap.cpp).  sinf and cosf are called from device code
// (MonteCarlo.h) and from host code alike (worldTransform in Hittable.cpp, Camera::rotate): the
// device calls are CUDA's libm, the host calls stay the C library's, as in the original program.
inline thread_local bool in_kernel = false;
inline float sinf_(float x) { return in_kernel ? pm_sinf(x) : ::sinf(x); }
inline float cosf_(float x) { return in_kernel ? pm_cosf(x) : ::cosf(x); }
// acosf, atan2f (Hittable.inl hitSphere/hitCylinder) run on the device only.
inline float acosf_(float x) { return pm_acosf(x); }
inline float atan2f_(float y, float x) { return pm_atan2f(y, x); }
inline float powf_(float x, float y) { return pm_powf(x, y); }
// nvcc resolves the unsuffixed abs, acos, atan2 and pow on float arguments to the float forms
// (trace.cu:123-124,150, Material.inl:31-33, tonemap.cu:21-23).  g++ sees only ::abs(int) and the
// double forms of the rest in the global namespace, so abs(dot(..)) would truncate to an integer and
// the others would round differently.  Float arguments go to the float forms; any other argument
// type fails to compile rather than convert.
inline float abs_(float x) { return ::fabsf(x); }
inline float acos_(float x) { return pm_acosf(x); }
inline float atan2_(float y, float x) { return pm_atan2f(y, x); }
inline float pow_(float x, float y) { return pm_powf(x, y); }
template <class T> T abs_(T) = delete;
template <class T> T acos_(T) = delete;
template <class T, class U> T atan2_(T, U) = delete;
template <class T, class U> T pow_(T, U) = delete;
}  // namespace ptref_shim

#define sinf(x) ptref_shim::sinf_(x)
#define cosf(x) ptref_shim::cosf_(x)
#define acosf(x) ptref_shim::acosf_(x)
#define atan2f(y, x) ptref_shim::atan2f_(y, x)
#define powf(x, y) ptref_shim::powf_(x, y)
#define abs(x) ptref_shim::abs_(x)
#define acos(x) ptref_shim::acos_(x)
#define atan2(y, x) ptref_shim::atan2_(y, x)
#define pow(x, y) ptref_shim::pow_(x, y)
