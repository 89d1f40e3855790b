// Issue cost of packed against plain FP32 vector instructions on one SIMD.
//
// Six instruction streams, each timed per wave with s_memtime around an unrolled loop:
//   mul, add         64 independent v_mul_f32 / v_add_f32 per iteration (16 accumulators in turn)
//   pk_mul, pk_add   the same with v_pk_mul_f32 / v_pk_add_f32 on 16 register pairs
//   dep_pk           16 pairs, each a packed multiply and the packed add that reads its result, written with
//                    the kernel's vector type so that the compiler places the wait states the pair needs
//   dep_scalar       the same 32 products and sums as plain multiplies and adds
// at 1, 2 and 6 resident waves per SIMD: workgroups of four waves (one per SIMD), a full grid of
// CUs x waves-per-SIMD of them, the residency held down by the dynamic LDS of a workgroup.
// Prints one JSON line: per occupancy and stream the median over the waves of cycles per instruction
// (dep streams: per multiply-add pair of one element pair, i.e. per 2 packed or 4 plain instructions).
//
//   pk_issue_probe [iterations]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        const hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "pk_issue_probe: %s: %s\n", #call, hipGetErrorString(e_));                \
            exit(1);                                                                                  \
        }                                                                                             \
    } while (0)

typedef float f2v __attribute__((ext_vector_type(2)));

enum { S_MUL = 0, S_ADD, S_PK_MUL, S_PK_ADD, S_DEP_PK, S_DEP_SCALAR, kStreams };
static const char* const kNames[kStreams] = {"mul", "add", "pk_mul", "pk_add", "dep_pk", "dep_scalar"};
constexpr int kAcc = 16;       // accumulators (registers or register pairs) a stream cycles through
constexpr int kRounds = 4;     // passes over the accumulators per loop iteration

#define PLAIN(op, a, c) asm volatile(op " %0, %0, %1" : "+v"(a) : "v"(c))

template <int STREAM>
__global__ void __launch_bounds__(256) stream_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                     uint32_t* __restrict__ cycles, int iters)
{
    extern __shared__ float lds[];
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    // factors that keep every accumulator finite and normal over the whole run (1 and 0 from memory)
    // every operand in vector registers, as in the trace kernel
    float one = in[0], zero = in[1];
    asm volatile("" : "+v"(one), "+v"(zero));
    float ax[kAcc], ay[kAcc];
    f2v a[kAcc];
#pragma unroll
    for (int k = 0; k < kAcc; ++k) {
        ax[k] = in[2 + k];
        ay[k] = in[2 + kAcc + k];
        asm volatile("" : "+v"(ax[k]), "+v"(ay[k]));
        a[k] = (f2v){ax[k], ay[k]};
    }
    f2v one2 = {one, one}, zero2 = {zero, zero};
    asm volatile("" : "+v"(one2), "+v"(zero2));
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);                 // nothing of the set-up moves behind the stamp
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
#pragma unroll
            for (int k = 0; k < kAcc; ++k) {
                if (STREAM == S_MUL) PLAIN("v_mul_f32", ax[k], one);
                if (STREAM == S_ADD) PLAIN("v_add_f32", ax[k], zero);
                if (STREAM == S_PK_MUL) PLAIN("v_pk_mul_f32", a[k], one2);
                if (STREAM == S_PK_ADD) PLAIN("v_pk_add_f32", a[k], zero2);
                if (STREAM == S_DEP_PK) {
                    a[k] = a[k] * one2 + zero2;
                    __builtin_amdgcn_sched_barrier(0);     // the add stays right behind its multiply
                }
                if (STREAM == S_DEP_SCALAR) {
                    ax[k] = ax[k] * one + zero;
                    ay[k] = ay[k] * one + zero;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    const uint64_t t1 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < kAcc; ++k) s += (a[k].x + a[k].y) + (ax[k] + ay[k]);
    out[tid] = s;
    if ((threadIdx.x & 63u) == 0u) cycles[tid >> 6] = (uint32_t)(t1 - t0);
}

typedef void (*Kernel)(const float*, float*, uint32_t*, int);

int main(int argc, char** argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 256;
    if (iters < 1 || iters > 65536) {
        fprintf(stderr, "pk_issue_probe: iterations must be in 1 .. 65536\n");
        return 1;
    }
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    static const Kernel kernels[kStreams] = {stream_kernel<S_MUL>,    stream_kernel<S_ADD>,    stream_kernel<S_PK_MUL>,
                                             stream_kernel<S_PK_ADD>, stream_kernel<S_DEP_PK>, stream_kernel<S_DEP_SCALAR>};
    // a CU of gfx950 has 160 KB of LDS: one workgroup of 96 KB fits, two of 64 KB, six of 24 KB
    const int occs[3] = {1, 2, 6};
    const size_t ldsOf[3] = {96u << 10, 64u << 10, 24u << 10};
    const int maxWaves = cus * 6 * 4;
    std::vector<float> hin(2 + 2 * kAcc, 1.0f);
    hin[1] = 0.0f;
    for (int k = 0; k < 2 * kAcc; ++k) hin[2 + k] = 1.0f + 0.03125f * (float)k;
    float *din, *dout;
    uint32_t* dcyc;
    CHECK(hipMalloc(&din, hin.size() * sizeof(float)));
    CHECK(hipMalloc(&dout, (size_t)maxWaves * 64 * sizeof(float)));
    CHECK(hipMalloc(&dcyc, (size_t)maxWaves * sizeof(uint32_t)));
    CHECK(hipMemcpy(din, hin.data(), hin.size() * sizeof(float), hipMemcpyHostToDevice));
    std::vector<uint32_t> hcyc(maxWaves);
    printf("{\"tool\": \"pk_issue_probe\", \"device\": \"%s\", \"cus\": %d, \"iterations\": %d, "
           "\"unit\": \"median over waves of s_memtime cycles per instruction (dep_*: per multiply-add of one "
           "element pair = 2 packed or 4 plain instructions)\"",
           prop.gcnArchName, cus, iters);
    for (int oi = 0; oi < 3; ++oi) {
        const int occ = occs[oi];
        const size_t lds = ldsOf[oi];
        const int blocks = cus * occ, waves = blocks * 4;
        printf(", \"waves_per_simd_%d\": {\"lds_bytes_per_workgroup\": %zu", occ, lds);
        for (int s = 0; s < kStreams; ++s) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[s]),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                (void)hipGetLastError();                 // this much LDS is not to be had: no figure, not a guess
                printf(", \"%s\": null", kNames[s]);
                continue;
            }
            const double perIter = (double)kAcc * kRounds;
            for (int rep = 0; rep < 2; ++rep) {      // the first launch warms the instruction cache
                hipLaunchKernelGGL(kernels[s], dim3(blocks), dim3(256), lds, 0, din, dout, dcyc, iters);
                CHECK(hipGetLastError());
                CHECK(hipDeviceSynchronize());
            }
            CHECK(hipMemcpy(hcyc.data(), dcyc, (size_t)waves * sizeof(uint32_t), hipMemcpyDeviceToHost));
            std::sort(hcyc.begin(), hcyc.begin() + waves);
            printf(", \"%s\": %.3f", kNames[s], (double)hcyc[waves / 2] / ((double)iters * perIter));
        }
        printf("}");
    }
    printf("}\n");
    CHECK(hipFree(din));
    CHECK(hipFree(dout));
    CHECK(hipFree(dcyc));
    return 0;
}
