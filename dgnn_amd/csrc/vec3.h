// The fp64 3-vector of the mesh, scene and triangulation kernels.  Every helper states its operation order: with -ffp-contract=off each
// product, sum and difference rounds on its own, and the numpy models of the tests repeat these expressions operation for operation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgnn_exact {

struct V3 { double x, y, z; };

template <typename I>          // the index in the caller's own width: widening it here keeps each caller's address arithmetic as it was
__device__ __forceinline__ V3 load_v3(const double* __restrict__ v, I i) { return V3{v[3 * (int64_t)i], v[3 * (int64_t)i + 1], v[3 * (int64_t)i + 2]}; }
__device__ __forceinline__ V3 sub(const V3& a, const V3& b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(const V3& a, const V3& b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double get(const V3& a, int k) { return k == 0 ? a.x : (k == 1 ? a.y : a.z); }

}  // namespace dgnn_exact
