"""The six Krylov vector kernels of rt_krylov.hip through their own launchers (tests/solver_kernel_probe.hip), with `blocks` chosen so
that the loops no solver run of the suite reaches are taken: a second, third and fourth round of the grid-stride loops, a second
round of k_kry_reduce's lanes over the blocks (66 blocks), the φ | ψ_in seam inside a pair, the zero pad of an odd N in the middle of
the grid.  Reference: numpy longdouble on the same arrays.

Bounds (u = 2⁻⁵³).  A sum of n terms, in any order, products rounded: (n + 4) u Σ|terms| (the bound of tests/sweep_f32_replay.py);
a norm gets its square root's rounding on top.  w − Σ_j h_j v_j and x₀ + Σ_j y_j v_j per element: (2 nvec + 2) u (|w| + Σ_j |h_j v_j|),
with or without contraction.  k_kry_residual and k_kry_scale_store are one IEEE operation per element: bits.
launch_kry_orthogonalise queues both Gram–Schmidt passes.  Against the longdouble classical Gram–Schmidt applied twice (c1, w₁, c2, w₂):
    hcol_i  within the dot bound of each pass added, d1_i + d2_i + 2 u |hcol_i| (its own addition), d1_i = (n + 4) u Σ |v_i| |w|,
            d2_i = (n + 4) u Σ |v_i| |w₁|;  the first pass alone within d1 through hcol − coef
    the row within the update's bound for both passes, with the DEVICE's coefficients c1' = hcol − coef and c2' = coef: the device forms
            (w − Σ_j c1'_j v_j) − Σ_j c2'_j v_j, each pass within (nvec + 1) u (1 + O(u)) of its |terms|, the second on a w₁ that is at
            most |w| + Σ_j |c1'_j v_j| (1 + O(u)); so |row − (w − Σ_j (c1'_j + c2'_j) v_j)| <= (4 nvec + 2) u (|w| + Σ_j (|c1'_j| + |c2'_j|) |v_j|)
            + Σ_j 2 u |hcol_j| |v_j|, the last for c1' recovered from the rounded sum hcol
The second pass works on the device's w₁ and the reference's on the exact one; bounds that carry the first pass's rounding into the
second (e1, d2', e2 in the test) are asserted as well, as extra checks beside the ones above, not in their place.  On small-integer
vectors, where no operation rounds, every coefficient and every element of the row is compared to the bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
SHAPES = [(26, 14, 1), (2000, 999, 2), (2001, 1000, 3), (16640 + 257, 5001, 66), (700, 0, 2), (700, 700, 2)]
NVEC_FULL = [1, 3, 4, 5, 8, 9, 17, 64]
# the kernels that go by pairs take 256 PAIRS per workgroup and round: with 66 workgroups only N > 2 · 65 · 256 gives the last two
# something to add, and k_kry_reduce's second round of lanes something other than zeros (16644 pairs: 4 in workgroup 65)
PAIRS66 = (2 * 65 * 256 + 7, 0, 66)
ORTHO = ([(SHAPES[1], nv) for nv in NVEC_FULL] + [(s, nv) for s in (SHAPES[0], SHAPES[2], SHAPES[3], SHAPES[5]) for nv in (5, 9)]
         + [(PAIRS66, 5)])
COMBINE = [(SHAPES[1], nv) for nv in [0] + NVEC_FULL] + [(s, nv) for s in (SHAPES[0], SHAPES[2], SHAPES[3], SHAPES[4], SHAPES[5]) for nv in (5, 9)]
_ids = lambda cases: ["N%d-nphi%d-b%d-nvec%d" % (s + (nv,)) for s, nv in cases]
_worst = {}


@pytest.fixture(scope="module")
def probe():
    import solverprobe

    yield solverprobe
    for name in sorted(_worst):
        print("largest fraction of its bound, %s: %.3g" % (name, _worst[name]))


def mixed(rng, shape):
    """Mixed signs, magnitudes 1e-3 .. 1e3."""
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)


def note(name, dev, bound):
    """Asserts dev <= bound elementwise; keeps the largest fraction per name (printed when the module's tests are done)."""
    dev, bound = np.atleast_1d(np.asarray(dev, LD)), np.atleast_1d(np.asarray(bound, LD))
    assert np.all(np.isfinite(dev)), name
    frac = float(np.max(np.where(bound > 0, dev / np.where(bound > 0, bound, 1), np.where(dev > 0, np.inf, 0.0))))
    _worst[name] = max(_worst.get(name, 0.0), frac)
    print("%s: largest fraction of the bound %.3g" % (name, frac))
    assert frac <= 1.0, (name, frac)


def block_of(n, blocks):
    """The workgroup that takes index (or pair) i of n in the grid-stride loops."""
    return (np.arange(n) // 256) % blocks


def rows(rng, nrows, N, integer=False):
    """[nrows, Ns] with a zero pad, flat with one canary element behind."""
    import solverprobe

    Ns = solverprobe.stride(N)
    b = np.zeros((nrows, Ns))
    b[:, :N] = rng.integers(-2, 3, (nrows, N)).astype(np.float64) if integer else mixed(rng, (nrows, N))
    return np.concatenate([b.ravel(), [solverprobe.CANARY]]), Ns


# ---- k_kry_residual, k_kry_reduce (mode 2) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("neg", [False, True])
@pytest.mark.parametrize("N,nphi,blocks", SHAPES)
def test_residual_bits_partials_norm_and_canaries(probe, N, nphi, blocks, neg):
    rng = np.random.default_rng(N + nphi)
    x, ref = mixed(rng, N), mixed(rng, N)
    Ns = probe.stride(N)
    outs = []
    for _ in range(2):
        out = np.full(Ns + 1, probe.CANARY)
        npart, norm = probe.kry_residual(neg, x[:nphi], x[nphi:], ref, blocks, out)
        outs.append((out, npart, norm))
    out, npart, norm = outs[0]
    d = ref - x if neg else x - ref
    assert np.array_equal(out[:N], d) and np.all(out[N:] == probe.CANARY)
    t = d.astype(LD) ** 2
    blk = block_of(N, blocks)
    for b in range(blocks):
        tb = t[blk == b]
        note("residual npart", abs(LD(npart[b]) - tb.sum()), (len(tb) + 4) * U * tb.sum())
    note("residual norm", abs(LD(norm) ** 2 - t.sum()), (N + 4) * U * t.sum() + 2.5 * U * t.sum())
    assert all(np.array_equal(a, b) for a, b in zip(outs[0][:2], outs[1][:2])) and outs[0][2] == outs[1][2]
    npart2, none = probe.kry_residual(neg, x[:nphi], x[nphi:], ref, blocks, np.full(Ns + 1, probe.CANARY), with_norm=False)
    assert none is None and np.array_equal(npart2, npart)


# ---- k_kry_scale_store ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nphi,blocks", SHAPES)
def test_scale_store_bits_and_canaries(probe, N, nphi, blocks):
    rng = np.random.default_rng(7 * N + nphi)
    Ns = probe.stride(N)
    w, div = mixed(rng, N), 0.037
    row = np.concatenate([w, np.full(Ns + 1 - N, probe.CANARY)])
    phi, psi = np.full(nphi + 1, probe.CANARY), np.full(N - nphi + 1, probe.CANARY)
    probe.kry_scale_store(row, div, nphi, N, blocks, phi, psi)
    v = w / div
    assert np.array_equal(row[:N], v) and np.all(row[N:] == probe.CANARY)
    assert np.array_equal(phi[:nphi], v[:nphi]) and phi[nphi] == probe.CANARY
    assert np.array_equal(psi[:N - nphi], v[nphi:]) and psi[N - nphi] == probe.CANARY


# ---- k_kry_dots, k_kry_reduce (modes 0, 1, 2), k_kry_update ----------------------------------------------------------------------------
def ortho_ref(B, slot, nvec):
    """Classical Gram–Schmidt twice in longdouble: c1, w1, c2, w2 of row `slot` of B [rows, Ns] against the rows below nvec."""
    V, w = B[:nvec].astype(LD), B[slot].astype(LD)
    c1 = V @ w
    w1 = w - (c1[:, None] * V).sum(0)
    c2 = V @ w1
    w2 = w1 - (c2[:, None] * V).sum(0)
    return V, w, c1, w1, c2, w2


def run_ortho(probe, N, blocks, nvec, integer, seed):
    rng = np.random.default_rng(seed)
    flat, Ns = rows(rng, nvec + 1, N, integer)
    before = flat.copy()
    res = probe.kry_orthogonalise(flat, N, nvec, nvec, blocks)
    B0, B1 = before[:-1].reshape(nvec + 1, Ns), flat[:-1].reshape(nvec + 1, Ns)
    assert flat[-1] == probe.CANARY and np.array_equal(B1[:nvec], B0[:nvec])
    assert np.all(B1[:, N:] == 0.0) and not np.any(np.signbit(B1[:, N:]))  # the pad is still exactly 0
    # the same call again: the same bits
    again = before.copy()
    res2 = probe.kry_orthogonalise(again, N, nvec, nvec, blocks)
    assert np.array_equal(again, flat) and all(np.array_equal(res[k], res2[k]) for k in ("hcol", "coef", "npart"))
    assert np.array_equal(res["part"][:, :nvec], res2["part"][:, :nvec])
    return B0, B1, res


@pytest.mark.parametrize("shape,nvec", ORTHO, ids=_ids(ORTHO))
def test_orthogonalise_against_longdouble(probe, shape, nvec):
    N, _, blocks = shape
    B0, B1, res = run_ortho(probe, N, blocks, nvec, False, 11 * N + nvec)
    V, w, c1, w1, c2, w2 = ortho_ref(B0, nvec, nvec)
    aV, n = np.abs(V), N
    d1 = (n + 4) * U * (aV * np.abs(w)).sum(1)
    e1 = (2 * nvec + 2) * U * (np.abs(w) + (np.abs(c1)[:, None] * aV).sum(0)) + (d1[:, None] * aV).sum(0)
    d2 = (n + 4) * U * (aV * (np.abs(w1) + e1)).sum(1) + (aV * e1).sum(1)
    e2 = (2 * nvec + 2) * U * (np.abs(w1) + e1 + ((np.abs(c2) + d2)[:, None] * aV).sum(0)) + e1 + (d2[:, None] * aV).sum(0)
    hcol, coef = res["hcol"].astype(LD), res["coef"].astype(LD)
    note("dots, pass 1 (hcol - coef)", np.abs((hcol[:nvec] - coef) - c1), d1 + 2 * U * np.abs(hcol[:nvec]))
    # the bounds the file's header states: hcol within the dot bound of each pass added, the row within the update's bound
    d2_plain = (n + 4) * U * (aV * np.abs(w1)).sum(1)
    note("hcol (dot bound of each pass added)", np.abs(hcol[:nvec] - (c1 + c2)), d1 + d2_plain + 2 * U * np.abs(hcol[:nvec]))
    c1d, c2d = hcol[:nvec] - coef, coef
    row_ref = w - ((c1d + c2d)[:, None] * V).sum(0)
    note("update (row, the device's coefficients)", np.abs(B1[nvec].astype(LD) - row_ref),
         (4 * nvec + 2) * U * (np.abs(w) + ((np.abs(c1d) + np.abs(c2d))[:, None] * aV).sum(0)) + 2 * U * (np.abs(hcol[:nvec])[:, None] * aV).sum(0))
    # extra: against the exact second pass, the first pass's rounding carried along
    note("extra: dots, pass 2 (coef), propagated", np.abs(coef - c2), d2)
    note("extra: hcol, propagated", np.abs(hcol[:nvec] - (c1 + c2)), d1 + d2 + 2 * U * np.abs(hcol[:nvec]))
    note("extra: row against w2, propagated", np.abs(B1[nvec].astype(LD) - w2), e2)
    # k_kry_reduce on the partials the device left (pass 2): the blocks in any order
    part = res["part"][:, :nvec].astype(LD)
    note("reduce of the dots' partials", np.abs(coef - part.sum(0)), (blocks + 4) * U * np.abs(part).sum(0))
    # the norm of the row the device wrote: per block, and reduced (mode 2)
    t = (B1[nvec].astype(LD) ** 2).reshape(-1, 2).sum(1)  # per pair
    blk = block_of(len(t), blocks)
    for b in range(blocks):
        tb = t[blk == b]
        note("update npart", abs(LD(res["npart"][b]) - tb.sum()), (2 * len(tb) + 4) * U * tb.sum())
    note("norm of the row", abs(hcol[nvec] ** 2 - t.sum()), (N + 4) * U * t.sum() + 2.5 * U * t.sum())


@pytest.mark.parametrize("shape,nvec", ORTHO, ids=_ids(ORTHO))
def test_orthogonalise_on_integers_to_the_bit(probe, shape, nvec):
    """Entries in −2 .. 2: every product, sum and difference of both passes is an integer below 2⁵³ (N <= 33287 with nvec <= 9, N = 2000 with nvec <= 64:
    |c1| <= 4 N, |w₁| <= 2 + 8 N nvec, |c2| <= 2 N |w₁|, |w₂| <= |w₁| + 2 nvec |c2| < 2⁵³), so nothing rounds whatever the order."""
    N, _, blocks = shape
    B0, B1, res = run_ortho(probe, N, blocks, nvec, True, 13 * N + nvec)
    V, w, c1, w1, c2, w2 = ortho_ref(B0, nvec, nvec)
    assert float(np.abs(w2).max()) < 2.0 ** 53 and float(np.abs(c2).max()) < 2.0 ** 53
    assert np.array_equal(res["coef"].astype(LD), c2) and np.array_equal(res["hcol"][:nvec].astype(LD), c1 + c2)
    assert np.array_equal(B1[nvec].astype(LD), w2)
    part = res["part"][:, :nvec].astype(LD)
    assert np.array_equal(part.sum(0), c2)
    blk = block_of(B0.shape[1] // 2, blocks)
    pairs = (V * w1).reshape(nvec, -1, 2).sum(2)
    for b in range(blocks):
        assert np.array_equal(part[b], pairs[:, blk == b].sum(1)), b


# ---- k_kry_combine -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nvec", COMBINE, ids=_ids(COMBINE))
def test_combine_against_longdouble(probe, shape, nvec):
    N, nphi, blocks = shape
    rng = np.random.default_rng(17 * N + nvec)
    m = max(nvec, 1)
    flat, Ns = rows(rng, m + 1, N)
    B = flat[:-1].reshape(m + 1, Ns)
    x0 = np.concatenate([mixed(rng, N), np.zeros(Ns - N)])
    y = mixed(rng, nvec)
    outs = []
    for _ in range(2):
        phi, psi = np.full(nphi + 1, probe.CANARY), np.full(N - nphi + 1, probe.CANARY)
        probe.kry_combine(x0, B, nphi, N, nvec, y, blocks, phi, psi)
        outs.append(np.concatenate([phi, psi]))
        assert phi[nphi] == probe.CANARY and psi[N - nphi] == probe.CANARY
    assert np.array_equal(outs[0], outs[1])
    got = np.concatenate([phi[:nphi], psi[:N - nphi]]).astype(LD)
    terms = y.astype(LD)[:, None] * B[:nvec, :N].astype(LD)
    if nvec == 0:
        assert np.array_equal(got, x0[:N].astype(LD))
    note("combine", np.abs(got - (x0[:N].astype(LD) + terms.sum(0))), (2 * nvec + 2) * U * (np.abs(x0[:N]) + np.abs(terms).sum(0)))


# ---- every `blocks`, the refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [1, 2, 3, 7, 8, 65, 1024])
def test_integers_to_the_bit_for_every_blocks(probe, blocks):
    """N = 2001, nvec = 9 with 1 .. kKryMaxBlocks workgroups (eight rounds down to workgroups with nothing to do): the same exact
    coefficients and row."""
    B0, B1, res = run_ortho(probe, 2001, blocks, 9, True, 99)
    V, w, c1, w1, c2, w2 = ortho_ref(B0, 9, 9)
    assert np.array_equal(res["hcol"][:9].astype(LD), c1 + c2) and np.array_equal(B1[9].astype(LD), w2)
    assert blocks <= probe.max_blocks()


def test_launchers_refuse_and_name_the_row(probe):
    rng = np.random.default_rng(5)
    N = 26
    flat, Ns = rows(rng, 67, N)  # m = 66
    keep = flat.copy()
    for slot, nvec in ((0, 1), (67, 1), (3, 0), (3, 4), (66, 65)):
        with pytest.raises(probe.Refused, match="row %d against %d rows of a basis of 67" % (slot, nvec)):
            probe.kry_orthogonalise(flat, N, slot, nvec, 1)
    assert np.array_equal(flat, keep)
    B = flat[:5 * Ns].reshape(5, Ns)  # m = 4
    phi, psi = np.full(15, probe.CANARY), np.full(N - 14 + 1, probe.CANARY)
    for nvec in (5, -1):
        with pytest.raises(probe.Refused, match="%d rows of a basis of 5" % nvec):
            probe.kry_combine(np.zeros(Ns), B, 14, N, nvec, np.ones(5), 1, phi, psi)
    row = np.zeros(Ns + 1)
    with pytest.raises(probe.Refused, match="row 2 of a basis of 2"):
        probe.kry_scale_store(row, 1.0, 14, N, 1, phi, psi, m=1, slot=2)
    assert np.all(phi == probe.CANARY) and np.all(psi == probe.CANARY)

