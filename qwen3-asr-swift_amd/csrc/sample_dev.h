// sample_dev.h -- the two device helpers the sampler kernels of tts_talker.hip and llm_cosyvoice.hip share (1024-thread workgroups).
#pragma once
#include "common.h"

namespace qasr {

// an unsigned key that orders like the float it was made of
__device__ __forceinline__ unsigned sample_order_key(float v) {
    const unsigned u = __float_as_uint(v + 0.0f);                             // -0 -> +0: the host compares values
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// first maximum of the workgroup's (value, index) pairs; every thread passes its own best with the lowest index among equals
__device__ __forceinline__ int sample_block_argmax(float v, int i, float* r_v, int* r_i) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    __syncthreads();
    if ((tid & 63) == 0) { r_v[tid >> 6] = v; r_i[tid >> 6] = i; }
    __syncthreads();
    float bv = r_v[0];
    int bi = r_i[0];
    for (int w = 1; w < 16; ++w)
        if (r_v[w] > bv || (r_v[w] == bv && r_i[w] < bi)) { bv = r_v[w]; bi = r_i[w]; }
    return bi;
}

}  // namespace qasr
