// krylov_host.cpp — TEST INFRASTRUCTURE: a stand-alone driver of csrc/rt_krylov_host.hpp (the Givens-rotated Hessenberg least-squares
// problem of the solver's restarted GMRES), built by tests/test_solver_krylov_cpu.py with the host sanitizers and run as a child.
// Input (stdin): m, the number of columns n <= m, β, then column k = 0 .. n − 1 as its k + 2 entries h[0 .. k + 1].
// Output: one line "res" with the residual norm after every column, one line "y" with the solution, one line "full" with what
// append returns for a column beyond m.
#include <cstdio>
#include <vector>

#include "../raytracing.jl_amd/csrc/rt_krylov_host.hpp"

int main() {
    int m = 0, n = 0;
    double beta = 0.0;
    if (std::scanf("%d %d %lf", &m, &n, &beta) != 3 || m < 0 || n < 0 || n > m) return 2;
    rtkry::Hessenberg H;
    H.reset(m, beta);
    std::vector<double> col((size_t)m + 2, 0.0), res;
    for (int k = 0; k < n; ++k) {
        for (int i = 0; i <= k + 1; ++i)
            if (std::scanf("%lf", &col[(size_t)i]) != 1) return 2;
        res.push_back(H.append(col.data()));
    }
    if (H.columns() != n) return 3;
    std::vector<double> y((size_t)n + 1, 0.0);
    H.solve(y.data());
    std::printf("res");
    for (double r : res) std::printf(" %.17g", r);
    std::printf("\ny");
    for (int i = 0; i < n; ++i) std::printf(" %.17g", y[(size_t)i]);
    // a column too many is refused and changes nothing
    rtkry::Hessenberg F;
    F.reset(1, 1.0);
    const double one[2] = {1.0, 0.5};
    F.append(one);
    std::printf("\nfull %.17g %d\n", F.append(one), F.columns());
    return 0;
}
