// rt_locate.hpp — the per-lane bodies of rt_locate.hip's kernels (k_locate_points, k_locate_grid, k_sample).  Plain arithmetic
// around rt_device.hpp's find_element: they also compile for the host, where tests/host_locate.hip runs them against the CPU
// checker without a GPU (test infrastructure; the library itself never locates on the host).
#pragma once
#include "rt_device.hpp"

namespace rt {

// find_element(mesh, p) followed, where that fails, by find_element(mesh, p, k) (src/track.jl:122,139; src/mesh.jl:103-146) for a
// point the caller hands in: the 1-based cell id, or -1.  A non-finite coordinate is -1 BEFORE any index is formed — the reference
// never sees such a point (a track's start lies on the bounding box), and bucket_of's floor(...) -> int conversion is undefined
// for NaN on the host build.  The guard stands here and not in find_element: the march calls that with points it has made itself,
// and its instructions stay what they are.  Finite points far outside go through the procedure as they are (bucket_of clamps).
template <bool WIDEK>
RT_HD __forceinline__ int32_t locate_point(const DGeo &g, double x, double y, int k) {
    if (!(isfin(x) && isfin(y))) return -1;
    Tri tri;
    const int32_t c = find_element<WIDEK>(g, x, y, k, tri);
    return c < 0 ? -1 : c + 1;
}

// Coordinate i of a raster axis: one multiply and one add in binary64, two roundings (the unit is compiled with
// -ffp-contract=off) — numpy's x0 + i*dx gives the same bits.
RT_HD __forceinline__ double grid_coord(double x0, double dx, int32_t i) {
    const double s = (double)i * dx;
    return x0 + s;
}

// What k_sample reads of a solver: φ [n_rows][G]; the cells' source regions (null: a row per cell); the linear source's flux
// moments φ⃗ [n_rows][G][2], C⁻¹ [n_rows][4] (xx, xy, yy, -) and centroids [n_rows][2] (null: the scalar flux alone).
struct DSample {
    const double *phi;
    const int32_t *region;
    const double *mom, *cinv, *cen;
    int32_t n_mesh, G, g0, ng;
    double fill;
};

// The flux of group g0 + j at (x, y) in the 1-based cell `cell`; `fill` for a cell outside 1 .. n_mesh (-1: not located).  Linear
// source: φ + ∇φ·(r − centroid) with ∇φ = C⁻¹ φ⃗ formed as rt_solver_fetch_moments forms it, every product and sum rounded on
// its own, left to right.
RT_HD __forceinline__ double sample_value(const DSample &a, int32_t cell, double x, double y, int32_t j) {
    if (cell < 1 || cell > a.n_mesh) return a.fill;
    const int64_t r = a.region ? a.region[cell - 1] : cell - 1;
    const int64_t e = r * a.G + a.g0 + j;
    double v = a.phi[e];
    if (a.mom) {
        const double mx = a.mom[2 * e], my = a.mom[2 * e + 1];
        const double cxx = a.cinv[4 * r], cxy = a.cinv[4 * r + 1], cyy = a.cinv[4 * r + 2];
        const double gx = cxx * mx + cxy * my, gy = cxy * mx + cyy * my;
        const double dx = x - a.cen[2 * r], dy = y - a.cen[2 * r + 1];
        v = (v + gx * dx) + gy * dy;
    }
    return v;
}

}  // namespace rt
