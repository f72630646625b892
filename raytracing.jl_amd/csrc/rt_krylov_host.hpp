// rt_krylov_host.hpp — the small least-squares problem of rt_solver's restarted GMRES, on the host: min_y ‖β e₁ − H y‖ for the
// (k + 1) x k upper Hessenberg H that grows by one column per Krylov vector.  Givens rotations keep H triangular as it grows, so the
// residual norm of the GMRES iterate is known after every column without solving for y.  Host-only, no HIP types: the cycle driver
// in rt_solver.hip includes it (through rt_solver_state.hpp), and tests/krylov_host.cpp drives it alone.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace rtkry {

class Hessenberg {
public:
    // a system of at most m columns with the right-hand side β e₁
    void reset(int m, double beta) {
        m_ = m < 0 ? 0 : m; k_ = 0;
        R_.assign((size_t)m_ * (size_t)(m_ + 1), 0.0);
        c_.assign((size_t)m_, 1.0); s_.assign((size_t)m_, 0.0);
        g_.assign((size_t)m_ + 1, 0.0);
        g_[0] = beta;
    }
    int columns() const { return k_; }
    // Column k = columns(): h[0 .. k + 1] (h[k + 1] the subdiagonal entry, 0 at a breakdown).  Returns the residual norm
    // min_y ‖β e₁ − H y‖ over the k + 1 columns so far; -1 when the system is full.
    double append(const double *h) {
        if (k_ >= m_) return -1.0;
        const int k = k_;
        double *r = R_.data() + (size_t)k * (size_t)(m_ + 1);
        for (int i = 0; i <= k + 1; ++i) r[i] = h[i];
        for (int i = 0; i < k; ++i) {  // the rotations of the columns before
            const double a = r[i], b = r[i + 1];
            r[i] = c_[(size_t)i] * a + s_[(size_t)i] * b;
            r[i + 1] = -s_[(size_t)i] * a + c_[(size_t)i] * b;
        }
        const double a = r[k], b = r[k + 1], d = std::hypot(a, b);
        const double c = d > 0.0 ? a / d : 1.0, s = d > 0.0 ? b / d : 0.0;  // (a zero column: no rotation, a zero pivot that solve skips)
        c_[(size_t)k] = c; s_[(size_t)k] = s;
        r[k] = d; r[k + 1] = 0.0;
        const double gk = g_[(size_t)k];
        g_[(size_t)k] = c * gk;
        g_[(size_t)k + 1] = -s * gk;
        ++k_;
        return std::fabs(g_[(size_t)k_]);
    }
    // y [columns()] by back-substitution; a zero pivot (a zero column) takes y = 0 there
    void solve(double *y) const {
        for (int i = k_ - 1; i >= 0; --i) {
            double v = g_[(size_t)i];
            for (int j = i + 1; j < k_; ++j) v -= R_[(size_t)j * (size_t)(m_ + 1) + (size_t)i] * y[j];
            const double p = R_[(size_t)i * (size_t)(m_ + 1) + (size_t)i];
            y[i] = p != 0.0 ? v / p : 0.0;
        }
    }

private:
    int m_ = 0, k_ = 0;
    std::vector<double> R_, c_, s_, g_;  // R column-major with stride m + 1; the rotations; the rotated right-hand side
};

}  // namespace rtkry
