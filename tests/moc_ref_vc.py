"""Numpy twin of the solver's volume correction (rt_solver_set_volume_correction): A_e, L[e][a], f, ℓ' and V' from the definitions of
include/rt_segmentize.h ("Volume correction") over a set of records — the ORACLE's in the tests.  `correct` hands ℓ' and V' to a built
`moc_ref.Twin` (its records' ℓ and its `vol`, which every twin built around it — moc_ref_bc.BoundaryTwin, moc_ref_iface.IfaceTwin,
moc_ref_cmfd.CmfdTwin, the P1 sweep of moc_ref_p1 — reads where they lie): the twins are driven, not copied.  The checker of
tests/test_solver_volume_correction_cpu.py and tests/test_gpu_solver_volume_correction.py."""
import numpy as np

MODES = ("angle", "cell")


def cell_areas(mesh):
    """A_e = ½ |(x1 − x0)(y2 − y0) − (x2 − x0)(y1 − y0)| from the mesh's node coordinates, in that order."""
    cn = np.asarray(mesh.cell_nodes, np.int64) - 1
    x, y = np.asarray(mesh.x, np.float64)[cn], np.asarray(mesh.y, np.float64)[cn]
    return 0.5 * np.abs((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]))


def tracked_lengths(rec, azim_idx, n_cells, n_azim_2):
    """L[e][a] = Σ_{u: azim[u] = a} Σ_{rec of u in e} ℓ, [n_cells, n_azim_2] (column a − 1)."""
    cnt = np.diff(np.asarray(rec["offsets"], np.int64))
    a_rec = np.repeat(np.asarray(azim_idx, np.int64) - 1, cnt)
    e = np.asarray(rec["element"], np.int64) - 1
    return np.bincount(e * n_azim_2 + a_rec, weights=np.asarray(rec["ell"], np.float64), minlength=n_cells * n_azim_2).reshape(n_cells, n_azim_2)


def tables(mesh, rec, azim_idx, delta_s, alpha, mode):
    """dict: area [nc], L, f [nc, N2], ell (ℓ' per record), vol (V' [nc]), vol_track (Σ_a w_a L), f_min, f_max and the counts
    unseen_pairs, zero_area_cells, zero_volume_cells."""
    if mode not in MODES:
        raise ValueError('mode must be "angle" or "cell"')
    delta_s, alpha = np.asarray(delta_s, np.float64), np.asarray(alpha, np.float64)
    N2 = len(delta_s)
    A = cell_areas(mesh)
    nc = len(A)
    L = tracked_lengths(rec, azim_idx, nc, N2)
    w = 2.0 * alpha * delta_s
    V = np.zeros(nc)
    for a in range(N2):  # (a ascending, as one thread per cell sums it)
        V = V + w[a] * L[:, a]
    f = np.ones((nc, N2))
    live = A > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == "angle":
            seen = (L > 0) & live[:, None]
            f[seen] = (A[:, None] / (delta_s[None, :] * L))[seen]
        else:
            ok = live & (V > 0)
            f[ok] = (A / V)[ok, None]
    Vc = np.zeros(nc)
    for a in range(N2):
        Vc = Vc + w[a] * (f[:, a] * L[:, a])
    cnt = np.diff(np.asarray(rec["offsets"], np.int64))
    a_rec = np.repeat(np.asarray(azim_idx, np.int64) - 1, cnt)
    e = np.asarray(rec["element"], np.int64) - 1
    ell = np.asarray(rec["ell"], np.float64) * f[e, a_rec]  # (one multiplication)
    return dict(area=A, L=L, f=f, ell=ell, vol=Vc, vol_track=V, f_min=float(f.min()) if f.size else 1.0, f_max=float(f.max()) if f.size else 1.0,
                unseen_pairs=int((~(L > 0)).sum()), zero_area_cells=int((~live).sum()), zero_volume_cells=int((~(V > 0)).sum()))


def correct(twin, tg, alpha, mode):
    """ℓ' into the records of a built moc_ref.Twin (a copy of the dict: the caller's records stay) and V' into its `vol`, in place.
    Returns the tables.  The linear source is refused, as the library refuses it."""
    if twin.linear:
        raise ValueError("the volume correction together with the linear source is not supported")
    aq = tg.azimuthal_quadrature
    t = tables(tg.mesh, twin.rec, tg.azim_idx, aq.delta_s, alpha, mode)
    twin.rec = dict(twin.rec, ell=t["ell"])
    twin.vol[...] = t["vol"]
    return t
