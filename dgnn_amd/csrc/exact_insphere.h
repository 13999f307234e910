// Exact sign of the 3D in-sphere test on fp64 coordinates (delaunay.hip), beside exact_orient.h and in its style.
//
//   insphere_sign(a, b, c, d, e) = +1 when e lies strictly inside the sphere through a, b, c, d, 0 when it lies on it, -1 outside, for ANY
//   non-flat a..d: with L the 5x5 determinant of the rows [x y z x^2+y^2+z^2 1] of a, b, c, d, e the result is -sign(L) * orient_sign(a, b, c, d)
//   (orient_sign of exact_orient.h; a positively oriented a..d has e inside exactly when L < 0).  Flat a..d give 0: four coplanar points
//   have no sphere.
//
//   filter  L = det of the four rows [p - e, |p - e|^2], p = a..d, in fp64 in the operation order of the classic adaptive in-sphere predicate:
//           the six 2x2 minors of the xy differences, the four 3x3 minors abc, bcd, cda, dab, the four lifts, then
//           (dlift * abc - clift * dab) + (blift * cda - alift * bcd).  The sign is accepted when |L| > (16 + 224 eps) eps * permanent + 2^-600,
//           eps = 2^-53.  The relative term is the static bound of that predicate for this expression: the 12 differences carry (1 + eps) each,
//           a lift (three squares, two sums) 2 more roundings on top of the 2 of its differences, a 3x3 minor 5 roundings on top of 3 levels of
//           differences and products; walking the expression tree gives at most 16 roundings on any path from a coordinate to L, hence
//           (1 + eps)^16 - 1 <= (16 + 224 eps) eps times the same expression with every product and sum replaced by its magnitude (the
//           permanent).  The absolute term covers products that underflow, which the relative bound does not: an underflowing product is off
//           by at most 2^-1074, it is multiplied by at most three further differences (each below 2^151 in the range below), so it moves L by
//           less than 2^-621; fewer than 2^7 products feed L, together less than 2^-614 < 2^-600.
//   exact   otherwise, out of line, on the RAW coordinates: L = sum over the 120 assignments of the five rows to the columns (x, y, z, w, 1)
//           and the three squares of w of sign * x_i y_j z_k c_l c_l: 360 products of five coordinates.  Every coordinate is an integer of 53
//           bits times a power of two, so a product is an integer of at most 265 bits times 2^E; it is formed in 32-bit digits and added at
//           its exponent into a fixed-point accumulator of 58 limbs of 64 bits (464 bytes), 32 bits of weight per limb, so that carries wait
//           until the end (lazy carries: a limb takes less than 2^43 in magnitude from 360 products).  One carry pass then leaves the sign in
//           the highest non-zero limb.  No rounding happens anywhere.
//   range   exact when every coordinate is 0 or has a magnitude in [2^-150, 2^150]: a coordinate is then m * 2^e with m odd and below
//           2^53 and e in [-202, 150], a product of five lies on the grid 2^-1010 and below 2^755, the sum of 360 below 2^764: 1774 bits from the grid up, inside the
//           accumulator's 58 * 32 = 1856.  In the filter no intermediate overflows (|L| < 2^770).  The caller checks the range
//           (insphere_coord_ok); exact_orient.h's range [2^-300, 2^300] contains this one.
// Needs -ffp-contract=off (the Makefile's flags), as exact_orient.h does.
#pragma once
#include "exact_orient.h"

namespace dgnn_exact {

__device__ __forceinline__ bool insphere_coord_ok(double x) { return coord_in_range(x, 0x1p150); }

constexpr int IS_LIMBS = 58;        // 64-bit limbs of the accumulator, 32 bits of weight each
constexpr int IS_BASE = -1010;      // exponent of limb 0's lowest bit

struct IsMant {   // value = (neg ? -1 : 1) * (hi * 2^32 + lo) * 2^e; lo == hi == 0 for 0.0
    uint32_t lo, hi;
    int32_t e, neg;
};

__device__ __forceinline__ IsMant is_split(double x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    const uint64_t frac = u & 0x000fffffffffffffull;
    const int ef = (int)((u >> 52) & 0x7ff);
    IsMant m;
    m.neg = (int32_t)(u >> 63);
    if (ef == 0) {   // 0.0 (subnormals are outside the range)
        m.lo = m.hi = 0;
        m.e = 0;
        return m;
    }
    uint64_t full = frac | 0x0010000000000000ull;
    const int tz = __builtin_ctzll(full);   // trailing zeros go to the exponent: small integers and powers of two become one short digit
    full >>= tz;
    m.lo = (uint32_t)full;
    m.hi = (uint32_t)(full >> 32);
    m.e = ef - 1075 + tz;
    return m;
}

// acc += sign * f0 f1 f2 f3 f4, exactly
__device__ __forceinline__ void is_add_product(int64_t* acc, int sign, const IsMant& f0, const IsMant& f1, const IsMant& f2, const IsMant& f3,
                                               const IsMant& f4) {
    const IsMant* f[5] = {&f0, &f1, &f2, &f3, &f4};
    if (!((f0.lo | f0.hi) && (f1.lo | f1.hi) && (f2.lo | f2.hi) && (f3.lo | f3.hi) && (f4.lo | f4.hi))) return;
    uint32_t d[12];
    for (int i = 0; i < 12; ++i) d[i] = 0;
    d[0] = f0.lo;
    d[1] = f0.hi;
    int len = f0.hi ? 2 : 1, e = f0.e, neg = f0.neg;
#pragma unroll 1
    for (int t = 1; t < 5; ++t) {
        uint32_t r[12];
        for (int i = 0; i < 12; ++i) r[i] = 0;
        const uint64_t lo = f[t]->lo, hi = f[t]->hi;
        if (hi == 0) {   // a one-digit factor
            uint64_t carry = 0;
            for (int i = 0; i < len; ++i) {
                const uint64_t v = (uint64_t)d[i] * lo + carry;
                r[i] = (uint32_t)v;
                carry = v >> 32;
            }
            r[len] = (uint32_t)carry;
            len += 1;
        } else {
            for (int i = 0; i < len; ++i) {   // r[i + 2] is still 0 here: the step before ended at r[i + 1]
                uint64_t v = (uint64_t)d[i] * lo + r[i];
                r[i] = (uint32_t)v;
                v = (uint64_t)d[i] * hi + r[i + 1] + (v >> 32);
                r[i + 1] = (uint32_t)v;
                r[i + 2] = (uint32_t)(v >> 32);
            }
            len += 2;
        }
        for (int i = 0; i < 12; ++i) d[i] = r[i];
        e += f[t]->e;
        neg ^= f[t]->neg;
    }
    const int shift = e - IS_BASE;          // >= 0 in the range
    const int q = shift >> 5, s = shift & 31;
    const int64_t sg = (neg ? -sign : sign);
    for (int i = 0; i < len; ++i) {         // a non-zero digit i starts below bit 755 - IS_BASE = 1765 of the accumulator: q + i <= 55
        if (d[i] == 0) continue;
        const uint64_t v = (uint64_t)d[i] << s;
        acc[q + i] += sg * (int64_t)(v & 0xffffffffull);
        acc[q + i + 1] += sg * (int64_t)(v >> 32);
    }
}

// the exact stage alone: sign of L (-1, 0, +1)
__device__ __noinline__ int insphere_det_sign_exact(V3 a, V3 b, V3 c, V3 d, V3 e) {
    int64_t acc[IS_LIMBS];
    for (int i = 0; i < IS_LIMBS; ++i) acc[i] = 0;
    IsMant m[5][3];
    const V3 p[5] = {a, b, c, d, e};
    for (int i = 0; i < 5; ++i) {
        m[i][0] = is_split(p[i].x);
        m[i][1] = is_split(p[i].y);
        m[i][2] = is_split(p[i].z);
    }
#pragma unroll 1
    for (int code = 0; code < 625; ++code) {   // rows (i, j, k, l) of the columns x, y, z, w; the fifth row takes the 1
        const int i = code / 125, j = (code / 25) % 5, k = (code / 5) % 5, l = code % 5;
        if (i == j || i == k || i == l || j == k || j == l || k == l) continue;
        const int r = 10 - i - j - k - l;
        const int perm[5] = {i, j, k, l, r};
        int inv = 0;
        for (int x = 0; x < 5; ++x)
            for (int y = x + 1; y < 5; ++y) inv += perm[x] > perm[y];
        const int sign = (inv & 1) ? -1 : 1;
#pragma unroll 1
        for (int w = 0; w < 3; ++w) is_add_product(acc, sign, m[i][0], m[j][1], m[k][2], m[l][w], m[l][w]);
    }
    for (int i = 0; i + 1 < IS_LIMBS; ++i) {   // the one carry pass: limbs below the top end in [0, 2^32)
        const int64_t carry = acc[i] >> 32;
        acc[i] -= carry * 4294967296ll;
        acc[i + 1] += carry;
    }
    if (acc[IS_LIMBS - 1] < 0) return -1;
    for (int i = IS_LIMBS - 1; i >= 0; --i)
        if (acc[i] != 0) return 1;
    return 0;
}

// sign of L; *exact_used = 1 when the filter could not decide (NULL: not reported)
__device__ __forceinline__ int insphere_det_sign(const V3& a, const V3& b, const V3& c, const V3& d, const V3& e, int* exact_used = nullptr) {
    const double aex = a.x - e.x, aey = a.y - e.y, aez = a.z - e.z;
    const double bex = b.x - e.x, bey = b.y - e.y, bez = b.z - e.z;
    const double cex = c.x - e.x, cey = c.y - e.y, cez = c.z - e.z;
    const double dex = d.x - e.x, dey = d.y - e.y, dez = d.z - e.z;
    const double aexbey = aex * bey, bexaey = bex * aey, ab = aexbey - bexaey;
    const double bexcey = bex * cey, cexbey = cex * bey, bc = bexcey - cexbey;
    const double cexdey = cex * dey, dexcey = dex * cey, cd = cexdey - dexcey;
    const double dexaey = dex * aey, aexdey = aex * dey, da = dexaey - aexdey;
    const double aexcey = aex * cey, cexaey = cex * aey, ac = aexcey - cexaey;
    const double bexdey = bex * dey, dexbey = dex * bey, bd = bexdey - dexbey;
    const double abc = aez * bc - bez * ac + cez * ab;
    const double bcd = bez * cd - cez * bd + dez * bc;
    const double cda = cez * da + dez * ac + aez * cd;
    const double dab = dez * ab + aez * bd + bez * da;
    const double alift = aex * aex + aey * aey + aez * aez;
    const double blift = bex * bex + bey * bey + bez * bez;
    const double clift = cex * cex + cey * cey + cez * cez;
    const double dlift = dex * dex + dey * dey + dez * dez;
    const double det = (dlift * abc - clift * dab) + (blift * cda - alift * bcd);
    const double faez = fabs(aez), fbez = fabs(bez), fcez = fabs(cez), fdez = fabs(dez);
    const double pab = fabs(aexbey) + fabs(bexaey), pbc = fabs(bexcey) + fabs(cexbey), pcd = fabs(cexdey) + fabs(dexcey);
    const double pda = fabs(dexaey) + fabs(aexdey), pac = fabs(aexcey) + fabs(cexaey), pbd = fabs(bexdey) + fabs(dexbey);
    const double perm = ((pcd * fbez + pbd * fcez + pbc * fdez) * alift + (pda * fcez + pac * fdez + pcd * faez) * blift) +
                        ((pab * fdez + pbd * faez + pda * fbez) * clift + (pbc * faez + pac * fbez + pab * fcez) * dlift);
    const double bound = (16.0 + 224.0 * 0x1p-53) * 0x1p-53 * perm + 0x1p-600;
    if (det > bound) return 1;
    if (-det > bound) return -1;
    if (exact_used) *exact_used = 1;
    return insphere_det_sign_exact(a, b, c, d, e);
}

// e against the sphere of a positively oriented a..d (orient_sign(a, b, c, d) > 0, which the caller guarantees): +1 inside, 0 on, -1 outside
__device__ __forceinline__ int insphere_pos(const V3& a, const V3& b, const V3& c, const V3& d, const V3& e, int* exact_used = nullptr) {
    return -insphere_det_sign(a, b, c, d, e, exact_used);
}

// any a..d; 0 for flat a..d
__device__ __forceinline__ int insphere_sign(const V3& a, const V3& b, const V3& c, const V3& d, const V3& e, int* exact_used = nullptr,
                                             int* orient_exact_used = nullptr) {
    const int o = orient_sign(a, b, c, d, orient_exact_used);
    if (o == 0) return 0;
    return -o * insphere_det_sign(a, b, c, d, e, exact_used);
}

}  // namespace dgnn_exact
