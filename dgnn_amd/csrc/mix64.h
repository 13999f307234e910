// The splitmix64 finaliser, modulo 2^64: the one hash of the package's counter-based draws (sampler.hip's neighbour selection and
// dgnn_amd/sampler.py, mesh_common.h's mm_hash, scansub.hip's thinning order).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
