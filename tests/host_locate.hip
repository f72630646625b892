// host_locate.hip — TEST INFRASTRUCTURE.  Runs the bodies of the locate and sample kernels on the host.
//
// What a lane of k_locate_points, k_locate_grid and k_sample does (csrc/rt_locate.hpp: locate_point around rt_device.hpp's
// find_element, grid_coord, sample_value) is plain FP64 arithmetic that compiles for the host as well.  This file builds the mesh
// view the kernels read (csrc/rt_mesh_prep.hpp, as rt_mesh_create does) and loops over the points where the kernels have one lane
// each, so that the locate's parity with the CPU checker at ties and outside the mesh, and its rule for non-finite points, are
// tested without a GPU (tests/test_locate_cpu.py) and under the sanitizers (tests/sanitize/locate_san.hip).  It is not part of the
// product: the library never locates on the host, and the GPU tests go through the C ABI on the real kernels.
//
// Build: hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -fno-fast-math -fPIC -shared (tests/hostlocate.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../raytracing.jl_amd/csrc/rt_locate.hpp"
#include "../raytracing.jl_amd/csrc/rt_mesh_prep.hpp"

namespace {

// The generic step's mesh view over host memory (ids as at the C ABI: cell_nodes and node_cells_data 1-based, ptrs 0-based).
struct HostGeo {
    std::vector<int32_t> cn, ncd;
    std::vector<rt::FanEntry> fan;
    rtprep::Prep P;
    rt::DGeo g{};
    HostGeo(const double *x, const double *y, int32_t n_nodes, const int32_t *cell_nodes, int32_t n_cells, const int32_t *ncp,
            const int32_t *ncd1, const double *bb)
        : cn(3 * (size_t)n_cells), ncd((size_t)std::max(ncp[n_nodes], 1)), fan((size_t)std::max(ncp[n_nodes], 1)) {
        for (size_t i = 0; i < cn.size(); ++i) cn[i] = cell_nodes[i] - 1;
        for (int32_t i = 0; i < ncp[n_nodes]; ++i) ncd[i] = ncd1[i] - 1;
        P = rtprep::prepare(x, y, n_nodes, cn.data(), n_cells, bb);
        for (int32_t i = 0; i < ncp[n_nodes]; ++i) {
            const int32_t c = ncd[i];
            rt::FanEntry &e = fan[i];
            e.x1 = x[cn[3 * c]]; e.y1 = y[cn[3 * c]]; e.x2 = x[cn[3 * c + 1]]; e.y2 = y[cn[3 * c + 1]]; e.x3 = x[cn[3 * c + 2]]; e.y3 = y[cn[3 * c + 2]];
            e.cell = c;
            for (int q = 0; q < 3; ++q) e.adj[q] = P.adjr[(size_t)3 * c + q];
        }
        g.x = rt::as_global(x); g.y = rt::as_global(y); g.cn = rt::as_global((const int32_t *)cn.data());
        g.ncp = rt::as_global(ncp); g.ncd = rt::as_global((const int32_t *)ncd.data());
        g.gstart = rt::as_global((const int32_t *)P.gstart.data()); g.gnode = rt::as_global((const int32_t *)P.gnode.data());
        g.c3start = rt::as_global((const int32_t *)P.c3start.data()); g.c3node = rt::as_global((const int32_t *)P.c3node.data());
        g.c3x = rt::as_global((const double *)P.c3x.data()); g.c3y = rt::as_global((const double *)P.c3y.data());
        g.fan = rt::as_global((const rt::FanEntry *)fan.data());
        g.gx0 = bb[0]; g.gy0 = bb[1]; g.gh = P.gh; g.ginv = P.ginv; g.gnx = P.gnx; g.gny = P.gny; g.n_nodes = n_nodes;
    }
};

}  // namespace

extern "C" {

// k_locate_points, lane by lane: cell[i] = the 1-based cell of (px[i], py[i]) or -1.  Returns -1 for k < 0 (rt_locate_points refuses it).
int32_t hostlocate_points(const double *x, const double *y, int32_t n_nodes, const int32_t *cell_nodes, int32_t n_cells, const int32_t *ncp,
                          const int32_t *ncd1, const double *bb, int64_t n, const double *px, const double *py, int32_t k, int32_t *cell) {
    if (k < 0) return -1;
    HostGeo H(x, y, n_nodes, cell_nodes, n_cells, ncp, ncd1, bb);
    for (int64_t i = 0; i < n; ++i)
        cell[i] = k > rt::kMaxK ? rt::locate_point<true>(H.g, px[i], py[i], k) : rt::locate_point<false>(H.g, px[i], py[i], k);
    return 0;
}

// k_locate_grid, lane by lane: cell [ny][nx] and (either may be NULL) the coordinates the lanes formed, gx [nx] and gy [ny].
int32_t hostlocate_grid(const double *x, const double *y, int32_t n_nodes, const int32_t *cell_nodes, int32_t n_cells, const int32_t *ncp,
                        const int32_t *ncd1, const double *bb, double x0, double y0, double dx, double dy, int32_t nx, int32_t ny, int32_t k,
                        int32_t *cell, double *gx, double *gy) {
    if (k < 0 || nx < 0 || ny < 0) return -1;
    HostGeo H(x, y, n_nodes, cell_nodes, n_cells, ncp, ncd1, bb);
    const int64_t n = (int64_t)nx * ny;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t row = (int32_t)(i / nx), col = (int32_t)(i - (int64_t)row * nx);
        const double qx = rt::grid_coord(x0, dx, col), qy = rt::grid_coord(y0, dy, row);
        if (gx) gx[col] = qx;
        if (gy) gy[row] = qy;
        cell[i] = k > rt::kMaxK ? rt::locate_point<true>(H.g, qx, qy, k) : rt::locate_point<false>(H.g, qx, qy, k);
    }
    return 0;
}

// k_sample, lane by lane: out [n][ng].  region, and mom / cinv / cen (all three or none), may be NULL.
void hostlocate_sample(const double *phi, const int32_t *region, const double *mom, const double *cinv, const double *cen, int32_t n_mesh,
                       int32_t G, int32_t g0, int32_t ng, double fill, int64_t n, const int32_t *cell, const double *px, const double *py, double *out) {
    rt::DSample a{};
    a.phi = phi; a.region = region; a.mom = mom; a.cinv = cinv; a.cen = cen;
    a.n_mesh = n_mesh; a.G = G; a.g0 = g0; a.ng = ng; a.fill = fill;
    for (int64_t i = 0; i < n * ng; ++i) {
        const int64_t p = i / ng;
        out[i] = rt::sample_value(a, cell[p], px[p], py[p], (int32_t)(i - p * ng));
    }
}

}  // extern "C"
