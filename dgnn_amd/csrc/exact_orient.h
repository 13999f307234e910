// Exact sign of the 3D orientation det[b - a, c - a, p - a] on fp64 coordinates (meshtopo.hip).
//
//   filter  the fp64 determinant in the operation order of meshmetrics.hip's orient(), accepted when |det| > (7 + 56 eps) eps * permanent
//           + 2^-700 (eps = 2^-53: the static bound of the classic adaptive orientation predicate for this expression, the permanent being
//           the same expression with every product and difference replaced by its magnitude; the absolute term covers products that
//           underflow, which the relative bound does not).
//   exact   otherwise: det = D(b, c, p) - D(a, c, p) + D(a, b, p) - D(a, b, c) with D the 3x3 determinant of raw coordinates, 24 signed triple
//           products x y z, each split exactly into four doubles by TwoProduct (fma); the 96 doubles are summed into a non-overlapping
//           expansion by Grow-Expansion (TwoSum, zero components dropped), whose largest component carries the sign.
//   range   exact when every coordinate is 0 or has a magnitude in [2^-300, 2^300]: every non-zero triple product then lies in
//           [2^-900, 2^900], so no TwoProduct underflows and no partial sum overflows.  The caller checks the range (orient_coord_ok).
// Needs -ffp-contract=off (the Makefile's flags): TwoSum and the filter's error bound assume every + and * rounds on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "vec3.h"

namespace dgnn_exact {

// 0 or a magnitude in [1 / lim, lim], lim a power of two (NaN and the infinities fail it)
__device__ __forceinline__ bool coord_in_range(double x, double lim) {
    const double m = fabs(x);
    return m == 0.0 || (m >= 1.0 / lim && m <= lim);
}
__device__ __forceinline__ bool orient_coord_ok(double x) { return coord_in_range(x, 0x1p300); }
__device__ __forceinline__ bool orient_coords_ok(const V3& a) { return orient_coord_ok(a.x) && orient_coord_ok(a.y) && orient_coord_ok(a.z); }

// one coordinate for the orientation predicate: fine, not finite, or finite and out of range; the callers map it onto their status bits
enum CoordClass { COORD_FINE = 0, COORD_NONFINITE, COORD_RANGE };
__device__ __forceinline__ bool coord_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }
__device__ __forceinline__ CoordClass coord_class(double x) {
    return !coord_finite(x) ? COORD_NONFINITE : (orient_coord_ok(x) ? COORD_FINE : COORD_RANGE);
}

__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bv = s - a, av = s - bv;
    e = (a - av) + (b - bv);
}

__device__ __forceinline__ void two_prod(double a, double b, double& p, double& e) {
    p = a * b;
    e = fma(a, b, -p);
}

// e[0, n): non-overlapping, increasing magnitude, no zeros  ->  the same for e + b; returns the new length (<= n + 1)
__device__ __forceinline__ int grow_expansion(double* e, int n, double b) {
    double q = b;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        double s, h;
        two_sum(q, e[i], s, h);
        q = s;
        if (h != 0.0) e[m++] = h;
    }
    if (q != 0.0 || m == 0) e[m++] = q;
    return m;
}

// adds sign * x * y * z exactly (four doubles)
__device__ __forceinline__ int add_triple(double* e, int n, double sign, double x, double y, double z) {
    double p, pe, p1, e1, p2, e2;
    two_prod(x, y, p, pe);
    two_prod(p, z, p1, e1);
    two_prod(pe, z, p2, e2);
    n = grow_expansion(e, n, sign * e2);
    n = grow_expansion(e, n, sign * p2);
    n = grow_expansion(e, n, sign * e1);
    return grow_expansion(e, n, sign * p1);
}

// adds sign * det[r; s; t] (rows of raw coordinates)
__device__ __forceinline__ int add_det3(double* e, int n, double sign, const V3& r, const V3& s, const V3& t) {
    n = add_triple(e, n, sign, r.x, s.y, t.z);
    n = add_triple(e, n, -sign, r.x, s.z, t.y);
    n = add_triple(e, n, -sign, r.y, s.x, t.z);
    n = add_triple(e, n, sign, r.y, s.z, t.x);
    n = add_triple(e, n, sign, r.z, s.x, t.y);
    return add_triple(e, n, -sign, r.z, s.y, t.x);
}

// the exact stage alone: -1, 0, +1
__device__ __noinline__ int orient_sign_exact(V3 a, V3 b, V3 c, V3 p) {
    double e[97];
    int n = 0;
    n = add_det3(e, n, 1.0, b, c, p);
    n = add_det3(e, n, -1.0, a, c, p);
    n = add_det3(e, n, 1.0, a, b, p);
    n = add_det3(e, n, -1.0, a, b, c);
    const double top = e[n - 1];
    return top > 0.0 ? 1 : (top < 0.0 ? -1 : 0);
}

// sign of det[b - a, c - a, p - a]; *exact_used = 1 when the filter could not decide (NULL: not reported)
__device__ __forceinline__ int orient_sign(const V3& a, const V3& b, const V3& c, const V3& p, int* exact_used = nullptr) {
    const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
    const double vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
    const double wx = p.x - a.x, wy = p.y - a.y, wz = p.z - a.z;
    const double m0 = vy * wz, m1 = vz * wy, m2 = vx * wz, m3 = vz * wx, m4 = vx * wy, m5 = vy * wx;
    const double det = ux * (m0 - m1) - uy * (m2 - m3) + uz * (m4 - m5);
    const double perm = fabs(ux) * (fabs(m0) + fabs(m1)) + fabs(uy) * (fabs(m2) + fabs(m3)) + fabs(uz) * (fabs(m4) + fabs(m5));
    const double bound = (7.0 + 56.0 * 0x1p-53) * 0x1p-53 * perm + 0x1p-700;
    if (det > bound) return 1;
    if (-det > bound) return -1;
    if (exact_used) *exact_used = 1;
    return orient_sign_exact(a, b, c, p);
}

}  // namespace dgnn_exact
