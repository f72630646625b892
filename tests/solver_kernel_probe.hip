// solver_kernel_probe.hip — TEST INFRASTRUCTURE.  Calls the Krylov vector kernels (csrc/rt_krylov.hip) through their own launchers
// with a DKrylov whose `blocks` the caller chooses, and k_cmfd_solve (csrc/rt_cmfd.hip) alone on coarse data the caller writes, so
// that tests/test_gpu_krylov_kernels.py and tests/test_gpu_cmfd_solve_paths.py reach the loops and exits no whole solver run
// gets to.  The kernels are the product's own text: the two files are included below, nothing is typed again; the only host
// symbols they need from the library are rthost::set_error and its message, supplied here.  Not part of the product: nothing in
// raytracing.jl_amd/ builds or loads this file.
//
// Every entry point takes host arrays, synchronises, and returns the first HIP status that is not hipSuccess (0: all succeeded), or
// kProbeRefused − the launcher's (negative) code when a launcher refused (its message: probe_last_error).  Arrays marked in/out are uploaded
// first and fetched afterwards with their canaries: the pad of a row and ONE element past every array the kernels write.
//
// Build: the library's Makefile FLAGS for gfx950, -shared (tests/solverprobe.py).
#include "../raytracing.jl_amd/csrc/rt_krylov.hip"
#include "../raytracing.jl_amd/csrc/rt_cmfd.hip"

namespace rthost {
thread_local std::string g_last_error;
void set_error(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}
}  // namespace rthost

namespace {

constexpr int kProbeRefused = 100000;

// device arrays of one call: every allocation is released when the call returns, whatever its status
struct Arena {
    std::vector<void *> ptrs;
    hipError_t st = hipSuccess;
    ~Arena() { for (void *p : ptrs) (void)hipFree(p); }
    // n elements (at least one is allocated), uploaded from `src` when it is given, else zeroed
    template <typename T>
    T *get(size_t n, const T *src) {
        if (st != hipSuccess) return nullptr;
        void *p = nullptr;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        st = hipMalloc(&p, bytes);
        if (st != hipSuccess) return nullptr;
        ptrs.push_back(p);
        st = (src && n) ? hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) : hipMemset(p, 0, bytes);
        return static_cast<T *>(p);
    }
    template <typename T>
    void fetch(T *dst, const T *src, size_t n) {
        if (st == hipSuccess && dst && n) st = hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost);
    }
    void sync() {
        if (st == hipSuccess) st = hipGetLastError();
        if (st == hipSuccess) st = hipDeviceSynchronize();
    }
};

bool kry_shape_ok(int64_t nphi, int64_t N, int64_t Ns, int32_t m, int32_t blocks) {
    return N >= 1 && N <= ((int64_t)1 << 22) && nphi >= 0 && nphi <= N && Ns == ((N + 1) & ~(int64_t)1) && m >= 0 && m <= 128 &&
           blocks >= 1 && blocks <= rt::kKryMaxBlocks;
}

// the scratch every launcher may touch, sized as rt_solver sizes it
void kry_scratch(Arena &A, rt::DKrylov &k) {
    k.part = A.get<double>((size_t)k.blocks * rt::kKryStride, nullptr);
    k.npart = A.get<double>((size_t)k.blocks, nullptr);
    k.coef = A.get<double>(rt::kKryStride, nullptr);
}

}  // namespace

extern "C" {

const char *probe_last_error() { return rthost::g_last_error.c_str(); }
int probe_kry_max_blocks() { return rt::kKryMaxBlocks; }
int probe_kry_stride() { return rt::kKryStride; }
int probe_refused() { return kProbeRefused; }

// out [Ns + 1] in/out; npart [blocks]; norm [1] (null: no reduction is queued).  phi [nphi], psi [N − nphi], ref [N].
int probe_kry_residual(int neg, const double *phi, const double *psi, int64_t nphi, int64_t N, const double *ref, int32_t blocks,
                       double *out, double *npart, double *norm) {
    const int64_t Ns = (N + 1) & ~(int64_t)1;
    if (!kry_shape_ok(nphi, N, Ns, 0, blocks) || !ref || !out || !npart) return (int)hipErrorInvalidValue;
    Arena A;
    rt::DKrylov k{};
    k.nphi = nphi; k.N = N; k.Ns = Ns; k.m = 0; k.blocks = blocks;
    kry_scratch(A, k);
    k.phi = A.get<double>((size_t)nphi, phi);
    k.psi = A.get<double>((size_t)(N - nphi), psi);
    double *d_ref = A.get<double>((size_t)N, ref);
    double *d_out = A.get<double>((size_t)Ns + 1, out);
    double *d_norm = A.get<double>(1, nullptr);
    if (A.st != hipSuccess) return (int)A.st;
    const int rc = rtx::launch_kry_residual(k, neg != 0, d_ref, d_out, norm ? d_norm : nullptr, 0);
    A.sync();
    if (rc != RT_SUCCESS) return kProbeRefused - rc;
    A.fetch(out, d_out, (size_t)Ns + 1);
    A.fetch(npart, k.npart, (size_t)blocks);
    A.fetch(norm, d_norm, 1);
    return (int)A.st;
}

// basis [(m + 1)·Ns + 1] in/out (row `slot` is orthogonalised against the rows 0 .. nvec − 1); hcol [nvec + 1] in/out;
// coef [nvec], part [blocks][kKryStride], npart [blocks]: what the second pass and the last update left.
int probe_kry_orthogonalise(double *basis, int64_t Ns, int64_t N, int32_t m, int32_t slot, int32_t nvec, int32_t blocks, double *hcol,
                            double *coef, double *part, double *npart) {
    if (!kry_shape_ok(0, N, Ns, m, blocks) || !basis || !hcol || !coef || !part || !npart) return (int)hipErrorInvalidValue;
    Arena A;
    rt::DKrylov k{};
    k.nphi = 0; k.N = N; k.Ns = Ns; k.m = m; k.blocks = blocks;
    kry_scratch(A, k);
    k.basis = A.get<double>((size_t)(m + 1) * Ns + 1, basis);
    const size_t nh = (size_t)std::clamp(nvec, 0, 64) + 1;
    double *d_h = A.get<double>(nh, hcol);
    if (A.st != hipSuccess) return (int)A.st;
    const int rc = rtx::launch_kry_orthogonalise(k, slot, nvec, d_h, 0);
    A.sync();
    if (rc != RT_SUCCESS) return kProbeRefused - rc;
    A.fetch(basis, k.basis, (size_t)(m + 1) * Ns + 1);
    A.fetch(hcol, d_h, nh);
    A.fetch(coef, k.coef, (size_t)nvec);
    A.fetch(part, k.part, (size_t)blocks * rt::kKryStride);
    A.fetch(npart, k.npart, (size_t)blocks);
    return (int)A.st;
}

// row [Ns + 1], phi [nphi + 1], psi [N − nphi + 1]: all in/out.  The row is slot `slot` of a basis of m + 1 rows of which only
// this one exists (slot = m = 0 for a plain call; anything else is for the launcher's refusal).
int probe_kry_scale_store(double *row, double div, int64_t nphi, int64_t N, int32_t m, int32_t slot, int32_t blocks, double *phi, double *psi) {
    const int64_t Ns = (N + 1) & ~(int64_t)1;
    if (!kry_shape_ok(nphi, N, Ns, m, blocks) || !row || !phi || !psi) return (int)hipErrorInvalidValue;
    Arena A;
    rt::DKrylov k{};
    k.nphi = nphi; k.N = N; k.Ns = Ns; k.m = m; k.blocks = blocks;
    kry_scratch(A, k);
    double *d_row = A.get<double>((size_t)Ns + 1, row);
    k.basis = d_row - (slot >= 0 && slot <= m ? (int64_t)slot * Ns : 0);  // (a refused slot is never dereferenced)
    k.phi = A.get<double>((size_t)nphi + 1, phi);
    k.psi = A.get<double>((size_t)(N - nphi) + 1, psi);
    double *d_div = A.get<double>(1, &div);
    if (A.st != hipSuccess) return (int)A.st;
    const int rc = rtx::launch_kry_scale_store(k, slot, d_div, 0);
    A.sync();
    if (rc != RT_SUCCESS) return kProbeRefused - rc;
    A.fetch(row, d_row, (size_t)Ns + 1);
    A.fetch(phi, k.phi, (size_t)nphi + 1);
    A.fetch(psi, k.psi, (size_t)(N - nphi) + 1);
    return (int)A.st;
}

// x0 [Ns], basis [(m + 1)·Ns], y [nvec]; phi [nphi + 1], psi [N − nphi + 1] in/out.
int probe_kry_combine(const double *x0, const double *basis, int64_t Ns, int64_t nphi, int64_t N, int32_t m, int32_t nvec, const double *y,
                      int32_t blocks, double *phi, double *psi) {
    if (!kry_shape_ok(nphi, N, Ns, m, blocks) || !x0 || !basis || !phi || !psi || (nvec > 0 && !y)) return (int)hipErrorInvalidValue;
    Arena A;
    rt::DKrylov k{};
    k.nphi = nphi; k.N = N; k.Ns = Ns; k.m = m; k.blocks = blocks;
    kry_scratch(A, k);
    k.x0 = A.get<double>((size_t)Ns, x0);
    k.basis = A.get<double>((size_t)(m + 1) * Ns, basis);
    k.phi = A.get<double>((size_t)nphi + 1, phi);
    k.psi = A.get<double>((size_t)(N - nphi) + 1, psi);
    if (A.st == hipSuccess && nvec > 0 && nvec <= rt::kKryStride) A.st = hipMemcpy(k.coef, y, (size_t)nvec * sizeof(double), hipMemcpyHostToDevice);
    if (A.st != hipSuccess) return (int)A.st;
    const int rc = rtx::launch_kry_combine(k, nvec, 0);
    A.sync();
    if (rc != RT_SUCCESS) return kProbeRefused - rc;
    A.fetch(phi, k.phi, (size_t)nphi + 1);
    A.fetch(psi, k.psi, (size_t)(N - nphi) + 1);
    return (int)A.st;
}

// coarse [R][NV] (NV = 4G + 2G² + 1, the layout of k_cmfd_restrict), J [(R + 1)][(R + 1)][G], coupling [R][R][G] or null.  One
// restriction item per region: part = coarse, reg_first = 0 .. R.  resident_override: 0 keeps the factors in global memory even
// where they would fit the LDS; anything else leaves the choice to cmfd_solve_lds.  fac [R][G], k [1]; info [3] in/out.
// resident_out (or null): where the factors were.
int probe_cmfd_solve(int32_t R, int32_t G, const double *coarse, const double *J, const double *coupling, int32_t eigen, double k0,
                     int32_t max_iter, double tol, double theta, int32_t resident_override, double *fac, double *k, int32_t *info,
                     int32_t *resident_out) {
    if (R < 1 || R > 512 || G < 1 || G > 16 || max_iter < 0 || !coarse || !J || !fac || !k || !info) return (int)hipErrorInvalidValue;
    bool resident = false;
    const size_t smem = rtx::cmfd_solve_lds(R, G, &resident);
    if (!smem) return (int)hipErrorInvalidValue;
    if (resident_override == 0) resident = false;
    if (resident_out) *resident_out = resident ? 1 : 0;
    const size_t NV = 4 * (size_t)G + 2 * (size_t)G * G + 1, Rp = (size_t)R + 1;
    std::vector<int32_t> first(Rp);
    std::iota(first.begin(), first.end(), 0);
    Arena A;
    rt::DCmfd c{};
    c.R = R; c.G = G; c.eigen = eigen ? 1 : 0; c.max_iter = max_iter; c.resident = resident ? 1 : 0;
    c.theta = theta; c.tol = tol;
    c.part = A.get<double>((size_t)R * NV, coarse);
    c.reg_first = A.get<int32_t>(Rp, first.data());
    c.coarse = A.get<double>((size_t)R * NV, nullptr);
    c.lu = A.get<double>((size_t)G * R * R, nullptr);
    c.fac = A.get<double>((size_t)R * G, nullptr);
    c.out = A.get<double>(1, nullptr);
    c.info = A.get<int32_t>(3, info);
    c.J = A.get<double>(Rp * Rp * G, J);
    c.coupling = coupling ? A.get<double>((size_t)R * R * G, coupling) : nullptr;
    const double scal[4] = {k0, 0.0, 0.0, 0.0};
    c.scal = A.get<double>(4, scal);
    if (A.st != hipSuccess) return (int)A.st;
    if (smem > 48 * 1024) A.st = hipFuncSetAttribute((const void *)rt::k_cmfd_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (A.st != hipSuccess) return (int)A.st;
    hipLaunchKernelGGL(rt::k_cmfd_solve, dim3(1), dim3(rt::kCmfdBlock), smem, 0, c);
    A.sync();
    A.fetch(fac, (const double *)c.fac, (size_t)R * G);
    A.fetch(k, (const double *)c.out, 1);
    A.fetch(info, (const int32_t *)c.info, 3);
    return (int)A.st;
}

}  // extern "C"
