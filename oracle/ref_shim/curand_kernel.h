// Host stand-in for <curand_kernel.h>: cuRAND's XORWOW generator as liboracle.so restates it
// (or_xorwow_* in pt_oracle.c, checked against cuRAND's documented outputs in tests/test_oracle.py).
#pragma once
#include "cuda_runtime.h"

struct curandState { unsigned int d, v[5]; };   // the 24 bytes of the state that XORWOW uses

extern "C" {
void or_xorwow_init(unsigned long long seed, curandState *s);
float or_xorwow_uniform(curandState *s);
}

inline void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long offset,
                        curandState *s)
{
    assert(subsequence == 0 && offset == 0);   // all initRandState.cu asks for
    or_xorwow_init(seed, s);
}

inline float curand_uniform(curandState *s) { return or_xorwow_uniform(s); }
