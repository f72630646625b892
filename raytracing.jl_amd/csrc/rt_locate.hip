// rt_locate.hip — batched point location and flux sampling: "which cell holds this point?" and "what is the flux there?" asked
// from outside, for points, for a raster, and of a solver's device-resident φ.
//   k_locate_points   one lane per point: find_element(mesh, p) then find_element(mesh, p, k) (src/track.jl:122,139), 1-based id or -1
//   k_locate_grid     the same for the points (x0 + i·dx, y0 + j·dy) of an nx × ny raster, row-major with j outer; no points uploaded
//   k_sample          out[n][ng]: φ of the located cells (through the source-region table; + ∇φ·(r − centroid) with the linear source)
// Each locate is a chain of dependent loads (the nearest node's 3x3 block three candidates per trip, then the node's cell fan): the
// kernels are bound by latency, and what a launch can give them is waves in flight and neighbouring points in neighbouring lanes.
// A wave's lanes are 64 consecutive points: a raster's are neighbours along x by construction; scattered points are located in
// the caller's order (no host-side bucket sort: no measurement asked for one — DESIGN.md §8 "Point location and flux sampling").
// Nothing here is launched by an existing call, and find_element is rt_device.hpp's as the march uses it; the rule for
// non-finite points stands in rt_locate.hpp's locate_point, outside it.
#include "rt_solver_state.hpp"
#include "rt_locate.hpp"

namespace rt {

constexpr int kLocateBlock = 256;

template <bool WIDEK>
__global__ void __launch_bounds__(kLocateBlock) k_locate_points(const RT_K DGeo *geo, int64_t n, const double *x, const double *y, int32_t k,
                                                                int32_t *cell) {
    const int64_t i = (int64_t)blockIdx.x * kLocateBlock + threadIdx.x;
    if (i >= n) return;
    const DGeo g = load_geo(geo);
    cell[i] = locate_point<WIDEK>(g, x[i], y[i], k);
}

template <bool WIDEK>
__global__ void __launch_bounds__(kLocateBlock) k_locate_grid(const RT_K DGeo *geo, double x0, double y0, double dx, double dy, int32_t nx,
                                                              int64_t n, int32_t k, int32_t *cell) {
    const int64_t i = (int64_t)blockIdx.x * kLocateBlock + threadIdx.x;
    if (i >= n) return;
    const DGeo g = load_geo(geo);
    const int32_t row = (int32_t)(i / nx), col = (int32_t)(i - (int64_t)row * nx);
    cell[i] = locate_point<WIDEK>(g, grid_coord(x0, dx, col), grid_coord(y0, dy, row), k);
}

// one lane per value: lane i holds group g0 + i % ng of point i / ng (out is [n][ng]: the stores of a wave are contiguous)
__global__ void __launch_bounds__(kLocateBlock) k_sample(DSample a, int64_t n_values, const int32_t *cell, const double *x, const double *y,
                                                         double *out) {
    const int64_t i = (int64_t)blockIdx.x * kLocateBlock + threadIdx.x;
    if (i >= n_values) return;
    const int64_t p = i / a.ng;
    out[i] = sample_value(a, cell[p], x[p], y[p], (int32_t)(i - p * a.ng));
}

}  // namespace rt

namespace {

constexpr int64_t kLocateMax = 0x7fffffff;  // points per call: the grid is ⌈n / 256⌉ workgroups

unsigned locate_blocks(int64_t n) { return (unsigned)((n + rt::kLocateBlock - 1) / rt::kLocateBlock); }

// what every locate entry point checks; `n` = 0 is a success that launches nothing (the caller returns before the pointers are read)
int locate_enter(const char *who, rt_mesh *mesh, int64_t n, int32_t k, const void *cell) {
    if (!mesh) { set_error("%s: null mesh", who); return RT_ERR_INVALID; }
    if (k < 0) {  // knn(kdtree, x, k, ...) rejects a negative k (src/mesh.jl:123); any k >= 0 is honoured
        set_error("%s: k = %d: the number of neighbouring nodes to search must not be negative", who, k);
        return RT_ERR_INVALID;
    }
    if (n < 0 || n > kLocateMax) { set_error("%s: bad arguments (%lld points, need 0 .. %lld)", who, (long long)n, (long long)kLocateMax); return RT_ERR_INVALID; }
    if (n > 0 && !cell) { set_error("%s: null output array", who); return RT_ERR_INVALID; }
    return RT_SUCCESS;
}

int grid_points(const char *who, int32_t nx, int32_t ny, int64_t *n) {
    if (nx < 0 || ny < 0 || (int64_t)nx * ny > kLocateMax) {
        set_error("%s: bad arguments (a raster of %d x %d points, need nx, ny >= 0 and nx * ny <= %lld)", who, nx, ny, (long long)kLocateMax);
        return RT_ERR_INVALID;
    }
    *n = (int64_t)nx * ny;
    return RT_SUCCESS;
}

int queue_locate_points(rt_mesh *m, int64_t n, const double *d_x, const double *d_y, int32_t k, int32_t *d_cell) {
    if (k > rt::kMaxK) hipLaunchKernelGGL(rt::k_locate_points<true>, dim3(locate_blocks(n)), dim3(rt::kLocateBlock), 0, m->stream, m->d.geo, n, d_x, d_y, k, d_cell);
    else hipLaunchKernelGGL(rt::k_locate_points<false>, dim3(locate_blocks(n)), dim3(rt::kLocateBlock), 0, m->stream, m->d.geo, n, d_x, d_y, k, d_cell);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

int queue_locate_grid(rt_mesh *m, double x0, double y0, double dx, double dy, int32_t nx, int64_t n, int32_t k, int32_t *d_cell) {
    if (k > rt::kMaxK) hipLaunchKernelGGL(rt::k_locate_grid<true>, dim3(locate_blocks(n)), dim3(rt::kLocateBlock), 0, m->stream, m->d.geo, x0, y0, dx, dy, nx, n, k, d_cell);
    else hipLaunchKernelGGL(rt::k_locate_grid<false>, dim3(locate_blocks(n)), dim3(rt::kLocateBlock), 0, m->stream, m->d.geo, x0, y0, dx, dy, nx, n, k, d_cell);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

// the solver holds a flux: after a completed run, and in an open one between a fold and the next sweep (a transient: from its begin)
int sample_enter(const char *who, rt_solver *S, int64_t n, int32_t g0, int32_t ng, const void *cell, const void *x, const void *y, const void *out) {
    if (!S) { set_error("%s: null solver", who); return RT_ERR_INVALID; }
    if (n < 0 || g0 < 0 || ng < 0 || (int64_t)g0 + ng > S->G || n * std::max<int64_t>(ng, 1) > kLocateMax) {
        set_error("%s: bad arguments (%lld points, groups %d .. %d + %d of %d; need n >= 0, a group range inside the solver's and n * ng <= %lld)", who,
                  (long long)n, g0, g0, ng, S->G, (long long)kLocateMax);
        return RT_ERR_INVALID;
    }
    const bool held = S->ran.done || (S->run.open && !S->run.swept && (S->run.it > 0 || S->tr.open));
    if (!held) {
        set_error("%s: the solver holds no flux (valid after a completed run, and between rt_solver_step_fold and the next rt_solver_step_sweep)", who);
        return RT_ERR_INVALID;
    }
    if (n > 0 && ng > 0 && (!cell || !x || !y || !out)) { set_error("%s: null array", who); return RT_ERR_INVALID; }
    return RT_SUCCESS;
}

int queue_sample(rt_solver *S, int64_t n, const int32_t *d_cell, const double *d_x, const double *d_y, int32_t g0, int32_t ng, double fill, double *d_out) {
    const bool linear = (S->run.open ? S->run.mode : S->ran.mode) == SweepMode::Linear;
    rt::DSample a{};
    a.phi = S->phi.p; a.region = S->sr.on ? S->sr.map.p : nullptr;
    a.mom = linear ? S->ls.mom.p : nullptr; a.cinv = linear ? S->ls.cinv.p : nullptr; a.cen = linear ? S->ls.cen.p : nullptr;
    a.n_mesh = S->n_mesh; a.G = S->G; a.g0 = g0; a.ng = ng; a.fill = fill;
    const int64_t nv = n * ng;
    hipLaunchKernelGGL(rt::k_sample, dim3(locate_blocks(nv)), dim3(rt::kLocateBlock), 0, S->t->mesh->stream, a, nv, d_cell, d_x, d_y, d_out);
    RT_HIP(hipGetLastError());
    return RT_SUCCESS;
}

}  // namespace

extern "C" {

int32_t rt_locate_points_device(rt_mesh *mesh, int64_t n, const double *d_x, const double *d_y, int32_t k, int32_t *d_cell) {
    const char *who = "rt_locate_points_device";
    if (int rc = locate_enter(who, mesh, n, k, d_cell)) return rc;
    if (n == 0) return RT_SUCCESS;
    if (!d_x || !d_y) { set_error("%s: null coordinate array", who); return RT_ERR_INVALID; }
    RT_HIP(hipSetDevice(mesh->device));
    return queue_locate_points(mesh, n, d_x, d_y, k, d_cell);
}

int32_t rt_locate_points(rt_mesh *mesh, int64_t n, const double *x, const double *y, int32_t k, int32_t *cell) {
    const char *who = "rt_locate_points";
    if (int rc = locate_enter(who, mesh, n, k, cell)) return rc;
    if (n == 0) return RT_SUCCESS;
    if (!x || !y) { set_error("%s: null coordinate array", who); return RT_ERR_INVALID; }
    RT_HIP(hipSetDevice(mesh->device));
    hipStream_t s = mesh->stream;
    DevBuf<double> dx, dy;
    DevBuf<int32_t> dc;
    if (int rc = rtx::upload(dx, x, (size_t)n, s)) return rc;
    if (int rc = rtx::upload(dy, y, (size_t)n, s)) return rc;
    RT_HIP(dc.reserve((size_t)n));
    if (int rc = queue_locate_points(mesh, n, dx.p, dy.p, k, dc.p)) return rc;
    RT_HIP(hipMemcpyAsync(cell, dc.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    return RT_SUCCESS;
}

int32_t rt_locate_grid_device(rt_mesh *mesh, double x0, double y0, double dx, double dy, int32_t nx, int32_t ny, int32_t k, int32_t *d_cell) {
    const char *who = "rt_locate_grid_device";
    int64_t n = 0;
    if (int rc = grid_points(who, nx, ny, &n)) return rc;
    if (int rc = locate_enter(who, mesh, n, k, d_cell)) return rc;
    if (n == 0) return RT_SUCCESS;
    RT_HIP(hipSetDevice(mesh->device));
    return queue_locate_grid(mesh, x0, y0, dx, dy, nx, n, k, d_cell);
}

int32_t rt_locate_grid(rt_mesh *mesh, double x0, double y0, double dx, double dy, int32_t nx, int32_t ny, int32_t k, int32_t *cell) {
    const char *who = "rt_locate_grid";
    int64_t n = 0;
    if (int rc = grid_points(who, nx, ny, &n)) return rc;
    if (int rc = locate_enter(who, mesh, n, k, cell)) return rc;
    if (n == 0) return RT_SUCCESS;
    RT_HIP(hipSetDevice(mesh->device));
    hipStream_t s = mesh->stream;
    DevBuf<int32_t> dc;
    RT_HIP(dc.reserve((size_t)n));
    if (int rc = queue_locate_grid(mesh, x0, y0, dx, dy, nx, n, k, dc.p)) return rc;
    RT_HIP(hipMemcpyAsync(cell, dc.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    return RT_SUCCESS;
}

int32_t rt_solver_sample(rt_solver *solver, int64_t n, const int32_t *d_cell, const double *d_x, const double *d_y, int32_t g0, int32_t ng, double fill,
                         double *d_out) {
    if (int rc = sample_enter("rt_solver_sample", solver, n, g0, ng, d_cell, d_x, d_y, d_out)) return rc;
    if (n == 0 || ng == 0) return RT_SUCCESS;
    RT_HIP(hipSetDevice(solver->t->mesh->device));
    return queue_sample(solver, n, d_cell, d_x, d_y, g0, ng, fill, d_out);
}

int32_t rt_solver_sample_host(rt_solver *solver, int64_t n, const int32_t *cell, const double *x, const double *y, int32_t g0, int32_t ng, double fill,
                              double *out) {
    if (int rc = sample_enter("rt_solver_sample_host", solver, n, g0, ng, cell, x, y, out)) return rc;
    if (n == 0 || ng == 0) return RT_SUCCESS;
    RT_HIP(hipSetDevice(solver->t->mesh->device));
    hipStream_t s = solver->t->mesh->stream;
    DevBuf<double> dx, dy, dout;
    DevBuf<int32_t> dc;
    if (int rc = rtx::upload(dx, x, (size_t)n, s)) return rc;
    if (int rc = rtx::upload(dy, y, (size_t)n, s)) return rc;
    if (int rc = rtx::upload(dc, cell, (size_t)n, s)) return rc;
    RT_HIP(dout.reserve((size_t)(n * ng)));
    if (int rc = queue_sample(solver, n, dc.p, dx.p, dy.p, g0, ng, fill, dout.p)) return rc;
    RT_HIP(hipMemcpyAsync(out, dout.p, (size_t)(n * ng) * sizeof(double), hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    return RT_SUCCESS;
}

}  // extern "C"
