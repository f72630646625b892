"""tests/sweep_f32_replay.py without a GPU: (1) the replay is the same definition as the numpy twin moc_ref_f32.sweep_f32 — within this
file's own E_ref (the twin's deviation from the FP64 sweep_fast on the same problem: the two differ in F alone, the correctly rounded
factor against the host build of rt_device.hpp's, at most 4·2⁻²⁴ apart); (2) records of ℓ = 0 — what a lane beyond its track's end
evaluates — leave ψ's bits and add nothing to a tally; (3) hand-made single-record tracks with ψ_in = −0.0, a subnormal ψ_in and ψ = r
exactly: Δ and the ψ kept have the bits the definition gives; (4) the tally's sum, Σ|terms| and N against a plain loop.

Measured: E_ref φ 7.8e-8, ψ_out 1.1e-7 of the largest value; the replay 1.9e-8 and 6.5e-8 from the twin."""
import numpy as np
import pytest

import f32_cases
import hostf32
import moc_ref_f32
import sweep_f32_replay as rp
import sweep_ref

F32 = np.float32


def _bits32(a):
    return np.asarray(a, np.float64).astype(F32).view(np.uint32)


def _dev(a, b):
    return float(np.abs(a - b).max()) / float(np.abs(b).max())


@pytest.fixture(scope="module")
def square(rt, oracle_run):
    tg, rec, _ = f32_cases.problem(rt, oracle_run, "square")
    G = 5
    rng = np.random.default_rng(31)
    nc, n = tg.mesh.num_cells, tg.n_total_tracks
    args = (rec["offsets"], rec["ell"], rec["element"], rng.uniform(0.05, 3.0, (nc, G)), rng.uniform(0.0, 2.0, (nc, G)),
            rng.uniform(0.5, 1.5, n), rng.uniform(0.0, 1.5, (2, n, G)))
    off, ell, el, st, q, w, psi_in = args
    return args, rp.replay(off, ell, el, st, rp.quotient(st, q), w, psi_in)


def test_replay_is_the_twins_definition(square):
    args, R = square
    nc = args[3].shape[0]
    phi64, out64 = sweep_ref.sweep_fast(*args)
    phi32, out32 = moc_ref_f32.sweep_f32(*args)
    e_phi, e_psi = _dev(phi32, phi64), _dev(out32, out64)
    total, mag, count = R.tally(nc)
    d_phi, d_psi = _dev(total.astype(np.float64), phi32), _dev(R.psi_out, out32)
    print("E_ref phi %.2e psi_out %.2e; replay against sweep_f32: phi %.2e psi_out %.2e" % (e_phi, e_psi, d_phi, d_psi))
    assert 0 < e_phi < 1e-4 and 0 < e_psi < 1e-4
    assert d_phi <= e_phi and d_psi <= e_psi
    assert np.array_equal(R.psi_out, R.psi_out.astype(F32).astype(np.float64))  # binary32 values
    assert count.sum() == 2 * len(args[1]) and R.terms.shape == (2 * len(args[1]), 5)


def test_tally_sum_magnitude_and_count(square):
    args, R = square
    nc = args[3].shape[0]
    total, mag, count = R.tally(nc)
    for cell in (0, 17, nc - 1):
        own = R.terms[R.cells == cell].astype(rp.LD)
        assert count[cell] == len(own) > 0
        slack = len(own) * rp.LD(2.0) ** -63 * np.abs(own).sum(0)  # (two longdouble sums in different orders)
        assert (np.abs(total[cell] - own.sum(0)) <= slack).all() and (np.abs(mag[cell] - np.abs(own).sum(0)) <= slack).all()
        assert (slack * 2 ** 8 < rp.tally_bound(mag, count)[cell]).all()  # (far inside the bound's "+ 4")
    b = rp.tally_bound(mag, count)
    assert b.shape == total.shape and (b > 0).all() and (b < 1e-12 * mag).all()
    # a cell that no record visits: sum 0, bound 0
    t2, m2, c2 = rp.Replay(R.psi_out, R.cells, R.terms).tally(nc + 3)
    assert not t2[nc:].any() and not c2[nc:].any() and not rp.tally_bound(m2, c2)[nc:].any()


def test_rows_of_zero_length_leave_psi_and_the_tallies(square):
    """Every track gets two records of ℓ = 0 in front and three behind (cell 1, the cell an idle lane reads): ψ_out keeps every bit in
    both directions, and the added terms are zeros."""
    args, R = square
    off, ell, el, st, q, w, psi_in = args
    n = len(off) - 1
    ell2, el2, off2 = [], [], [0]
    for u in range(n):
        a, b = off[u], off[u + 1]
        ell2 += [0.0, 0.0] + list(ell[a:b]) + [0.0, 0.0, 0.0]
        el2 += [1, 1] + list(el[a:b]) + [1, 1, 1]
        off2.append(len(ell2))
    R2 = rp.replay(np.array(off2), np.array(ell2), np.array(el2), st, rp.quotient(st, q), w, psi_in)
    assert np.array_equal(R2.psi_out.view(np.uint64), R.psi_out.view(np.uint64))
    # the same non-zero terms (in another order: the steps shifted), and 2 · 5 · n rows of zeros more
    assert np.array_equal(np.sort(R2.terms[R2.terms != 0]), np.sort(R.terms[R.terms != 0]))
    assert len(R2.terms) == len(R.terms) + 2 * 5 * n and (R2.terms == 0).sum() == (R.terms == 0).sum() + 2 * 5 * n * 5
    m1, m2 = R.tally(st.shape[0])[1], R2.tally(st.shape[0])[1]
    assert (np.abs(m1 - m2) <= 1e-17 * m1).all()


def test_edge_values_have_the_definitions_bits():
    """Five tracks of one record each, one component, weight 1 (a term is then (double)Δ): ψ_in = −0.0 with r = 0 and with r > 0, the
    smallest subnormal and a larger one with r = 0, and ψ = r exactly."""
    sub, sub2 = float(np.finfo(F32).smallest_subnormal), 3e-39
    r_eq = float(F32(0.7))
    psi0 = np.array([-0.0, -0.0, sub, sub2, r_eq])
    st = np.array([[0.5], [2.0], [1.0]])
    qs = np.array([[0.0], [1.25], [r_eq]])
    el = np.array([1, 2, 1, 1, 3])
    ell = np.array([0.3, 0.4, 0.5, 0.25, 0.2])
    R = rp.replay(np.arange(6), ell, el, st, qs, np.ones(5), np.stack([psi0, psi0])[:, :, None])
    assert np.array_equal(R.psi_out[0].view(np.uint64), R.psi_out[1].view(np.uint64))  # (one record: both directions alike)
    tau = st.astype(F32)[el - 1, 0] * ell.astype(F32)
    F = hostf32.one_minus_exp_neg(tau).astype(np.float64)
    assert (F > 0).all() and (F < 1).all()
    delta = R.terms[:5, 0]
    out = R.psi_out[0, :, 0]
    # −0 with r = 0: ψ − r = −0, Δ = −0·F = −0, ψ ← −0 − (−0) = +0
    assert delta[0] == 0 and np.signbit(delta[0]) and out[0] == 0 and not np.signbit(out[0])
    # −0 with r > 0: Δ = −r·F rounded once, ψ ← −0 − Δ = −Δ
    d1 = F32(-1.25 * F[1])  # (24 x 24 bits: exact in binary64, rounded once here)
    assert _bits32(delta[1]) == d1.view(np.uint32) and _bits32(out[1]) == F32(-d1).view(np.uint32)
    # subnormals with r = 0: Δ = ψ·F rounded once into the subnormal range, ψ ← ψ − Δ exactly (both multiples of 2⁻¹⁴⁹)
    for k, s in ((2, sub), (3, sub2)):
        p = float(F32(s))
        dk = F32(p * F[k])
        assert _bits32(delta[k]) == dk.view(np.uint32) and out[k] == p - float(dk) and 0 <= out[k] <= p
    assert delta[2] in (0.0, sub) and out[3] > 0 and delta[3] > 0  # (nothing was flushed to zero)
    # ψ = r: Δ = +0, ψ keeps its bits, the term is +0
    assert delta[4] == 0 and not np.signbit(delta[4]) and _bits32(out[4]) == F32(0.7).view(np.uint32)
