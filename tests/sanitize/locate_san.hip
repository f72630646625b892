// locate_san.hip — the bodies of the locate and sample kernels (csrc/rt_locate.hpp through tests/host_locate.hip) on the host under
// AddressSanitizer + UndefinedBehaviorSanitizer: GPU sanitizers are not available on the pool, so the code is sanitized where it
// can run.  One mesh (a 7 x 5 structured grid of right triangles, made here), its point set — every node, every cell's centroid,
// every edge's midpoint, seeded random points in the box inflated by 10 %, points far outside (±1e300) and non-finite ones — for
// k on both sides of kMaxK, against the checker (oracle/rt_oracle.c, same flags); the raster kernel's body over the same mesh; the
// sampler's body on arrays with cells outside 1 .. n_cells.  TEST INFRASTRUCTURE; a program of its own, not run by run.sh:
//   hipcc --cuda-host-only -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1 -ffp-contract=off \
//         -std=c++17 -Wno-unused-function -x hip -c tests/sanitize/locate_san.hip -o tests/build/sanitize/locate_san.o
//   /opt/rocm/lib/llvm/bin/clang <same -f flags> -c oracle/rt_oracle.c -o tests/build/sanitize/rt_oracle_clang.o
//   /opt/rocm/lib/llvm/bin/clang++ <same -f flags> -o tests/build/sanitize/locate_san tests/build/sanitize/locate_san.o tests/build/sanitize/rt_oracle_clang.o -lm
//   ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 tests/build/sanitize/locate_san
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>

#include "../host_locate.hip"

extern "C" {
void *orc_mesh_create(const double *x, const double *y, int32_t n_nodes, const int32_t *cell_nodes, int32_t n_cells,
                      const int32_t *nc_ptrs, const int32_t *nc_data, const double *bb);
void orc_mesh_destroy(void *mv);
int32_t orc_find_element(void *mv, double x, double y, int32_t k);
}

int main() {
    // the mesh: (nx + 1) x (ny + 1) nodes, every square cut along one diagonal (alternating), ids 1-based, ascending per cell
    const int nx = 7, ny = 5;
    const double x0 = -0.35, y0 = 0.2, hx = 0.15, hy = 0.11;
    std::vector<double> x, y;
    for (int j = 0; j <= ny; ++j)
        for (int i = 0; i <= nx; ++i) { x.push_back(x0 + i * hx); y.push_back(y0 + j * hy); }
    std::vector<int32_t> cells;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const int32_t a = j * (nx + 1) + i + 1, b = a + 1, c = a + nx + 1, d = a + nx + 2;
            if ((i + j) % 2) { for (int32_t v : {a, b, d, a, c, d}) cells.push_back(v); }
            else { for (int32_t v : {a, b, c, b, c, d}) cells.push_back(v); }
        }
    const int32_t nn = (int32_t)x.size(), nc = (int32_t)cells.size() / 3;
    std::vector<int32_t> ptrs(nn + 1, 0), data(cells.size());
    for (int32_t v : cells) ++ptrs[v];
    for (int32_t i = 0; i < nn; ++i) ptrs[i + 1] += ptrs[i];
    {
        std::vector<int32_t> at(ptrs.begin(), ptrs.end() - 1);
        for (int32_t c = 0; c < nc; ++c)
            for (int q = 0; q < 3; ++q) data[at[cells[3 * c + q] - 1]++] = c + 1;  // (cells ascending per node)
    }
    const double bb[4] = {x0, y0, x0 + nx * hx, y0 + ny * hy};
    // the points
    std::vector<double> px(x), py(y);
    for (int32_t c = 0; c < nc; ++c) {
        const int32_t *v = &cells[3 * c];
        px.push_back((x[v[0] - 1] + x[v[1] - 1] + x[v[2] - 1]) / 3.0); py.push_back((y[v[0] - 1] + y[v[1] - 1] + y[v[2] - 1]) / 3.0);
        for (int q = 0; q < 3; ++q) {
            const int32_t p = v[q] - 1, r = v[(q + 1) % 3] - 1;
            px.push_back(0.5 * (x[p] + x[r])); py.push_back(0.5 * (y[p] + y[r]));
        }
    }
    std::mt19937_64 rng(17);
    std::uniform_real_distribution<double> ux(bb[0] - 0.1 * (bb[2] - bb[0]), bb[2] + 0.1 * (bb[2] - bb[0])), uy(bb[1] - 0.1 * (bb[3] - bb[1]), bb[3] + 0.1 * (bb[3] - bb[1]));
    for (int i = 0; i < 300; ++i) { px.push_back(ux(rng)); py.push_back(uy(rng)); }
    for (const double v : {1e300, -1e300}) { px.push_back(v); py.push_back(0.4); px.push_back(0.1); py.push_back(v); px.push_back(v); py.push_back(-v); }
    const size_t n_finite = px.size();
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (const double v : {nan, inf, -inf}) { px.push_back(v); py.push_back(0.4); px.push_back(0.1); py.push_back(v); px.push_back(v); py.push_back(v); }
    const int64_t n = (int64_t)px.size();

    void *orc = orc_mesh_create(x.data(), y.data(), nn, cells.data(), nc, ptrs.data(), data.data(), bb);
    int bad = 0;
    long long located = 0, missed = 0;
    std::vector<int32_t> got(n);
    for (const int k : {0, 1, 2, 5, 8, 9, 20}) {
        if (hostlocate_points(x.data(), y.data(), nn, cells.data(), nc, ptrs.data(), data.data(), bb, n, px.data(), py.data(), k, got.data())) ++bad;
        for (int64_t i = 0; i < n; ++i) {
            int32_t want = -1;
            if ((size_t)i < n_finite) {
                want = orc_find_element(orc, px[i], py[i], 2);
                if (want < 0) want = orc_find_element(orc, px[i], py[i], k);
            }
            if (got[i] != want) { ++bad; printf("MISMATCH k=%d point %lld (%.17g, %.17g): %d, checker %d\n", k, (long long)i, px[i], py[i], got[i], want); }
            (got[i] > 0 ? located : missed) += 1;
        }
    }
    if (hostlocate_points(x.data(), y.data(), nn, cells.data(), nc, ptrs.data(), data.data(), bb, n, px.data(), py.data(), -1, got.data()) != -1) ++bad;
    // the raster's body: 23 x 19 reaching outside; the lanes' coordinates against x0 + i*dx formed here, the cells against the points' form
    const int gnx = 23, gny = 19;
    const double gx0 = bb[0] - 0.03, gy0 = bb[1] - 0.02, gdx = (bb[2] - bb[0] + 0.07) / gnx, gdy = (bb[3] - bb[1] + 0.05) / gny;
    std::vector<int32_t> gcell((size_t)gnx * gny), pcell((size_t)gnx * gny);
    std::vector<double> gx(gnx), gy(gny), qx, qy;
    if (hostlocate_grid(x.data(), y.data(), nn, cells.data(), nc, ptrs.data(), data.data(), bb, gx0, gy0, gdx, gdy, gnx, gny, 9, gcell.data(), gx.data(), gy.data())) ++bad;
    for (int j = 0; j < gny; ++j)
        for (int i = 0; i < gnx; ++i) {
            volatile double sx = (double)i * gdx, sy = (double)j * gdy;  // (two roundings each, whatever the flags)
            qx.push_back(gx0 + sx); qy.push_back(gy0 + sy);
            if (gx[i] != qx.back() || gy[j] != qy.back()) { ++bad; printf("RASTER COORDINATE (%d, %d)\n", i, j); }
        }
    hostlocate_points(x.data(), y.data(), nn, cells.data(), nc, ptrs.data(), data.data(), bb, (int64_t)gnx * gny, qx.data(), qy.data(), 9, pcell.data());
    if (gcell != pcell) { ++bad; printf("RASTER CELLS differ from the points' form\n"); }
    orc_mesh_destroy(orc);
    // the sampler's body: cells -1, 0 and nc + 1 among valid ones, with the region table and with the linear source's arrays
    const int G = 3;
    std::vector<double> phi((size_t)nc * G), mom((size_t)nc * G * 2), cinv((size_t)nc * 4), cen((size_t)nc * 2), out((size_t)n * G);
    std::vector<int32_t> region(nc), scell(n);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    for (auto &v : phi) v = 1.0 + u01(rng);
    for (auto &v : mom) v = u01(rng) - 0.5;
    for (auto &v : cinv) v = 1.0 + u01(rng);
    for (auto &v : cen) v = u01(rng);
    for (int32_t c = 0; c < nc; ++c) region[c] = c % 5;
    for (int64_t i = 0; i < n; ++i) scell[i] = (int32_t)(i % (nc + 3)) - 1;  // -1 .. nc + 1
    long long filled = 0;
    for (int mode = 0; mode < 3; ++mode) {
        hostlocate_sample(phi.data(), mode == 1 ? region.data() : nullptr, mode == 2 ? mom.data() : nullptr, mode == 2 ? cinv.data() : nullptr,
                          mode == 2 ? cen.data() : nullptr, nc, G, 1, 2, -5.0, n, scell.data(), px.data(), py.data(), out.data());
        for (int64_t i = 0; i < n; ++i) {
            const bool in = scell[i] >= 1 && scell[i] <= nc;
            if (!in) { ++filled; if (out[2 * i] != -5.0 || out[2 * i + 1] != -5.0) { ++bad; printf("SAMPLE fill, mode %d point %lld\n", mode, (long long)i); } }
            else if (mode < 2 && out[2 * i] != phi[(size_t)(mode ? region[scell[i] - 1] : scell[i] - 1) * G + 1]) { ++bad; printf("SAMPLE value, mode %d point %lld\n", mode, (long long)i); }
        }
    }
    printf("locate_san: %d nodes, %d cells, %lld points x 7 k (%lld located, %lld not), raster %d x %d, %lld sampled values filled; host build == checker: %s\n",
           nn, nc, (long long)n, located, missed, gnx, gny, filled, bad ? "MISMATCH" : "yes");
    return bad ? 1 : 0;
}
