// The facet / circumsphere arithmetic of DESIGN §23, written once for its two users: cutterms.hip recomputes a cell's sphere on every facet
// row that needs it, facetgeom.hip (§32) computes every sphere once (k_cell_spheres) and loads the 32-byte record per facet side.  Both
// forms feed the same sphere_cosine, and (o, R) are fp64 values either way -- p0 + c is rounded to fp64 whether it goes to a register or to
// memory (-ffp-contract=off) -- so the two give the same bits.  The operation order is the one include/dgnn_hip.h states.
#pragma once
#include <math.h>

#include "vec3.h"

namespace dgnn_exact {

// the circumsphere of the cell (p0, p1, p2, p3): the centre o = p0 + c, the radius R = sqrt(c . c), and det (0: a flat cell, whose c is
// a division by zero: R is then inf or NaN, never finite)
struct Sphere { V3 o; double R, det; };
__device__ __forceinline__ Sphere cell_sphere(const V3& p0, const V3& p1, const V3& p2, const V3& p3) {
    const V3 u = sub(p1, p0), vv = sub(p2, p0), w = sub(p3, p0);
    const V3 vw = cross(vv, w), wu = cross(w, u), uv = cross(u, vv);
    const double det = dot(u, vw), u2 = dot(u, u), v2 = dot(vv, vv), w2 = dot(w, w), d2 = 2.0 * det;
    const V3 c{((u2 * vw.x + v2 * wu.x) + w2 * uv.x) / d2, ((u2 * vw.y + v2 * wu.y) + w2 * uv.y) / d2, ((u2 * vw.z + v2 * wu.z) + w2 * uv.z) / d2};
    return Sphere{V3{p0.x + c.x, p0.y + c.y, p0.z + c.z}, sqrt(dot(c, c)), det};
}

// the facet (a, b, c) as stored: n = (b - a) X (c - a), nn = |n| (the area is 0.5 * nn)
struct FacetPlane { V3 a, n; double nn; };
__device__ __forceinline__ FacetPlane facet_plane(const V3& a, const V3& b, const V3& c) {
    const V3 n = cross(sub(b, a), sub(c, a));
    return FacetPlane{a, n, sqrt(dot(n, n))};
}

// cos phi of the facet seen from the cell with the circumsphere (o, R) and the opposite vertex d: the circumcentre's signed distance to the
// facet's plane over the circumradius, positive on the cell's own side.  0 and *neutral += 1 for a degenerate side: nn == 0, sd == 0 or one
// of R, h, r not finite (a flat cell, det == 0, is among these: its R is not finite).
__device__ __forceinline__ double sphere_cosine(const V3& o, double R, const FacetPlane& p, const V3& d, int* neutral) {
    const double sd = dot(p.n, sub(d, p.a));
    const double hn = dot(p.n, sub(o, p.a));
    const double h = (sd > 0 ? hn : -hn) / p.nn;
    const double r = h / R;
    if (p.nn == 0 || sd == 0 || !isfinite(R) || !isfinite(h) || !isfinite(r)) {
        *neutral += 1;
        return 0;
    }
    return r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
}

}  // namespace dgnn_exact
