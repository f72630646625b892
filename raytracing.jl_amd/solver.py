"""MOC transport solver on the device: power-iteration ``k_eff`` and fixed-source source iteration over the
records of the last ``segmentize`` — what the tracks and segments exist to feed (the reference's README:
"computes quantities used to solve the transport equation").

The iteration runs in ``librt_segmentize.so`` (``rt_solver_*``, ``csrc/rt_solver.hip``; the options' setters in ``csrc/rt_solver_set.hip``) around ``rt_sweep``:
per iteration a source-update kernel, one sweep over G x P components (energy groups x polar angles),
a fold kernel and a fixed-order reduction; only k, the residual and |Δk|/k come back to the host.
The definitions (azimuthal and polar weights, volumes, fold, source, residual, normalisation) are stated
in ``include/rt_segmentize.h``.  With ``CrossSections(..., sigma_s1=...)`` scattering is linearly anisotropic (P1): the
sweep's source depends on the direction of travel, first angular moments are tallied and ``SolverResult.current`` is the
net current.  With ``sigma_s2`` (and ``sigma_s3``) on top scattering is P2 (P3): the sweep carries the azimuthal Fourier functions of
its track up to that order, and ``SolverResult.angular_moments`` holds every moment φ_lm with l + m even (``rt_solver_set_scatter_pn``).
With ``scheme="linear"`` the source of a cell is linear in space (LS-MOC: a coarser mesh resolves the same flux
gradient); ``SolverResult.flux_moments``, ``flux_gradient`` and ``centroids`` describe the flux inside the cells.
With ``adjoint=True`` the same iteration runs on the transposed problem (``rt_solver_set_adjoint``) and returns the adjoint flux φ†;
``perturbation_reactivity`` and ``kinetics_parameters`` weigh cross-section changes and kinetics data with it
(``rt_solver_bilinear``).
With ``boundary=SolverBoundary(...)`` the four sides of the domain carry albedos β (ψ_in = β ψ_out + ψ_inc behind every track end
on that side, whatever ``trace`` linked there) and, in fixed-source runs, an isotropic incoming flux ψ_inc; the result then
carries the partial currents per side and group and the neutron balance (``rt_solver_set_boundary``).
With ``regions=...`` (an int per cell, or ``"material"``) every sweep also tallies the partial currents between the cell regions
(``rt_solver_set_regions``): ``SolverResult.region_current`` and the balance of every region, ``region_balance``.
With ``volume_correction="angle"`` (or ``"cell"``) the chord lengths the sweeps read are renormalised so that every cell's tracked
area equals its exact area (``rt_solver_set_volume_correction``); ``SolverResult.volumes`` are then the corrected ones.
With ``source_regions=...`` (an int per cell, or ``"material"``) every flat-source region is a set of cells and the sweeps read rows
merged per region (``rt_solver_set_source_regions``): ``phi``, ``volumes``, ``current`` and ``source`` are then per source region, and
``SolverResult.to_cells`` spreads such an array over the mesh's cells.
With ``cmfd=True`` (or a ``Cmfd``) on top of ``regions=...`` every iteration also solves the partial-current coarse-mesh balance
over the regions and prolongs its solution onto φ, k and the boundary fluxes (``rt_solver_set_cmfd``): the same answer in fewer
iterations; ``diffusion_coupling`` builds an optional coupling D̂ from the mesh.
``solve_transient`` continues an eigenvalue result in time (``rt_solver_transient_*``): implicit Euler with ``Kinetics`` data (1/v, delayed
fractions, decay constants and spectra), every step a fixed-source problem started from the previous step's flux, cross sections
changed between steps by ``events``; the result carries the relative power ``production`` over ``times``.
With ``krylov=True`` (or a ``Krylov``) ``solve_fixed_source`` and ``solve_transient`` take restarted-GMRES cycles in place of plain
iterations (``rt_solver_set_krylov``): the iteration is an affine map on (φ, ψ_in), every Krylov vector costs one unchanged sweep and
counts as an iteration, and a scattering ratio (or a transient's 1 − β) near one no longer sets the number of sweeps;
``SolverResult.krylov`` and ``TransientResult.krylov_vectors`` say what the cycles did.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi
from .trackgenerator import SIDE_NAMES, TrackGenerator, track_end_sides

__all__ = ["CrossSections", "PolarQuadrature", "SolverBoundary", "SolverResult", "Cmfd", "diffusion_coupling", "exact_azimuthal_weights", "azimuthal_weights",
           "solve_eigenvalue", "solve_fixed_source", "perturbation_reactivity", "kinetics_parameters", "neutron_balance", "region_balance",
           "Kinetics", "TransientResult", "solve_transient", "Krylov"]


class CrossSections:
    """Macroscopic cross sections of M materials in G groups: ``sigma_t``, ``nu_sigma_f``, ``chi`` [M, G] and
    ``sigma_s`` [M, G, G] with ``sigma_s[m, g', g]`` the transfer from group g' to g (isotropic scattering).
    One material may be given without its leading axis.  ``sigma_s1`` [M, G, G] (optional): the l = 1 Legendre moment of the
    same transfer, Σs(g'→g, μ0) = (1/4π) [Σs0 + 3 Σs1 μ0] — linearly anisotropic scattering; entries may be negative but
    must be finite with |Σs1| <= Σs0.  ``sigma_s2``, ``sigma_s3`` [M, G, G] (optional): the l = 2 and l = 3 moments of
    Σs(g'→g, μ0) = (1/4π) Σ_l (2l+1) Σs_l P_l(μ0), validated like ``sigma_s1``; ``sigma_s3`` needs ``sigma_s2``, and both need
    ``sigma_s1``.  ``scatter_order``: the highest l given (0 .. 3); ``sigma_sl``: the moments from l = 1 stacked.
    A material with ``sigma_t`` = 0 in every group is *void* ("Void" in ``include/rt_segmentize.h``): it must have no ``sigma_s``,
    ``sigma_s1`` and ``nu_sigma_f`` (its ``chi`` is ignored), and a material with ``sigma_t`` = 0 in some groups only is refused, both
    with the messages of ``rt_solver_create``.  ``void_materials``: one bool per material."""

    def __init__(self, sigma_t, sigma_s, nu_sigma_f, chi, sigma_s1=None, sigma_s2=None, sigma_s3=None):
        st = np.asarray(sigma_t, np.float64)
        st = st.reshape(1, -1) if st.ndim <= 1 else st
        if st.ndim != 2:
            raise ValueError("sigma_t must have shape [M, G]")
        M, G = st.shape
        ss = np.asarray(sigma_s, np.float64)
        if ss.size == M * G * G:
            ss = ss.reshape(M, G, G)
        nf = np.asarray(nu_sigma_f, np.float64)
        ch = np.asarray(chi, np.float64)
        nf = nf.reshape(M, G) if nf.size == M * G else nf
        ch = ch.reshape(M, G) if ch.size == M * G else ch
        if ss.shape != (M, G, G):
            raise ValueError(f"sigma_s must have shape [M, G, G] = {(M, G, G)}, got {np.shape(sigma_s)}")
        if nf.shape != (M, G) or ch.shape != (M, G):
            raise ValueError(f"nu_sigma_f and chi must have shape [M, G] = {(M, G)}")
        self.sigma_t, self.sigma_s, self.nu_sigma_f, self.chi = (np.ascontiguousarray(a) for a in (st, ss, nf, ch))
        for m in np.flatnonzero((st == 0).any(1)):
            m = int(m)
            if (st[m] != 0).any():
                g0, g1 = int(np.flatnonzero(st[m] == 0)[0]), int(np.flatnonzero(st[m] != 0)[0])
                raise ValueError(f"material {m} has sigma_t[{m}][{g0}] = 0 but sigma_t[{m}][{g1}] = {st[m, g1]:g} "
                                 "(a void material has Σt = 0 in every group)")
            for name, a, what in (("sigma_s", ss[m], "scatters"), ("nu_sigma_f", nf[m], "fissions")):
                if (a != 0).any():
                    idx = tuple(int(i) for i in np.argwhere(a != 0)[0])
                    raise ValueError(f"material {m} is void (sigma_t[{m}][g] = 0 in every group) but {name}[{m}]" + "".join(f"[{i}]" for i in idx)
                                     + f" = {a[idx]:g} (a void material {what} nothing)")
        if sigma_s2 is not None and sigma_s1 is None:
            raise ValueError("sigma_s2 needs sigma_s1 (the Legendre moments are given without gaps)")
        if sigma_s3 is not None and sigma_s2 is None:
            raise ValueError("sigma_s3 needs sigma_s2 (the Legendre moments are given without gaps)")
        self.sigma_s1 = self.sigma_s2 = self.sigma_s3 = None
        for name, given in (("sigma_s1", sigma_s1), ("sigma_s2", sigma_s2), ("sigma_s3", sigma_s3)):
            if given is None:
                continue
            sl = np.asarray(given, np.float64)
            if sl.size == M * G * G and sl.ndim <= 3:
                sl = sl.reshape(M, G, G)
            if sl.shape != (M, G, G):
                raise ValueError(f"{name} must have shape [M, G, G] = {(M, G, G)}, got {np.shape(given)}")
            for m in np.flatnonzero(self.void_materials):
                if (sl[m] != 0).any():
                    a, b = (int(i) for i in np.argwhere(sl[m] != 0)[0])
                    raise ValueError(f"material {int(m)} is void (sigma_t[{int(m)}][g] = 0 in every group) but {name}[{int(m)}][{a}][{b}] = {sl[m, a, b]:g} "
                                     "(a void material scatters nothing)")
            if not np.all(np.isfinite(sl)) or not np.all(np.abs(sl) <= self.sigma_s):
                raise ValueError(f"every {name} must be finite with |{name}| <= sigma_s")
            setattr(self, name, np.ascontiguousarray(sl))

    @property
    def void_materials(self) -> np.ndarray:
        """[M] bool: the materials with Σt = 0 in every group."""
        return (self.sigma_t == 0).all(1)

    @property
    def scatter_order(self) -> int:
        return 3 if self.sigma_s3 is not None else 2 if self.sigma_s2 is not None else 1 if self.sigma_s1 is not None else 0

    @property
    def sigma_sl(self):
        L = self.scatter_order
        return np.stack([self.sigma_s1, self.sigma_s2, self.sigma_s3][:L]) if L else None

    @property
    def n_materials(self) -> int:
        return int(self.sigma_t.shape[0])

    @property
    def n_groups(self) -> int:
        return int(self.sigma_t.shape[1])


# Tabuchi-Yamamoto optimal polar sets (sin θ_p, ω_p) for 1-3 angles per half space
_TY = {
    1: ((0.798184,), (1.0,)),
    2: ((0.363900, 0.899900), (0.212854, 0.787146)),
    3: ((0.166648, 0.537707, 0.932954), (0.046233, 0.283619, 0.670148)),
}


class PolarQuadrature:
    """Polar angles of one half space: ``sin_theta`` and ``weights`` [P] with Σ weights = 1.  ``spec``:
    ``"TY1"``, ``"TY2"``, ``"TY3"`` (Tabuchi-Yamamoto), ``"GL<n>"`` (Gauss-Legendre on μ = cos θ in (0, 1)),
    ``"none"`` (P = 1, sin θ = 1, ω = 1: the plain 2-D sweep), or a pair of arrays (sin θ, ω)."""

    def __init__(self, spec="TY3"):
        if isinstance(spec, PolarQuadrature):
            sin_t, w = spec.sin_theta, spec.weights
        elif isinstance(spec, str):
            s = spec.strip().upper()
            if s == "NONE":
                sin_t, w = [1.0], [1.0]
            elif s.startswith("TY") and s[2:].isdigit() and int(s[2:]) in _TY:
                sin_t, w = _TY[int(s[2:])]
            elif s.startswith("GL") and s[2:].isdigit() and int(s[2:]) >= 1:
                x, wx = np.polynomial.legendre.leggauss(2 * int(s[2:]))
                pos = x > 0  # the nodes of (0, 1): half of the symmetric set on (-1, 1)
                mu, wmu = x[pos], wx[pos]
                sin_t, w = np.sqrt(1.0 - mu * mu), wmu / wmu.sum()
            else:
                raise ValueError(f"unknown polar quadrature {spec!r} (TY1-TY3, GL<n>, none, or (sin_theta, weights))")
        else:
            sin_t, w = spec
        self.sin_theta = np.ascontiguousarray(sin_t, np.float64).reshape(-1)
        self.weights = np.ascontiguousarray(w, np.float64).reshape(-1)
        if self.sin_theta.shape != self.weights.shape or not len(self.weights):
            raise ValueError("sin_theta and weights must be non-empty and of equal length")
        if np.any(self.sin_theta <= 0) or np.any(self.sin_theta > 1) or np.any(self.weights <= 0):
            raise ValueError("need 0 < sin θ <= 1 and ω > 0")
        if abs(float(self.weights.sum()) - 1.0) > 1e-12:
            raise ValueError(f"polar weights sum to {float(self.weights.sum())!r}, not 1")

    @property
    def n_polar(self) -> int:
        return len(self.weights)


def exact_azimuthal_weights(aq) -> np.ndarray:
    """α_a [n_azim/2] with Σ α = 1/2: within the first quadrant (angles φ_1 < ... < φ_n), b_0 = 0,
    b_i = (φ_i + φ_{i+1}) / 2, b_n = π/2 and α_i = (b_i − b_{i−1}) / 2π, mirrored to the supplementary index.
    Equal to the reference's ω_a (``init_weights!``) except at the first angle of each quadrant."""
    n4, n2 = aq.n_azim_4, aq.n_azim_2
    ph = np.asarray(aq.phis[:n4], np.float64)
    if np.any(np.isnan(ph)):
        raise ValueError("the azimuthal angles are not set: call trace first")
    b = np.empty(n4 + 1)
    b[0], b[n4] = 0.0, math.pi / 2
    b[1:n4] = 0.5 * (ph[:-1] + ph[1:])
    a = np.empty(n2)
    a[:n4] = np.diff(b) / (2 * math.pi)
    a[n2 - n4:] = a[:n4][::-1]  # supplementary index N2 − i + 1
    return a


def azimuthal_weights(tg: TrackGenerator, spec="exact") -> np.ndarray:
    """``"exact"`` (``exact_azimuthal_weights``), ``"equal"`` (α = 1 / n_azim), or an explicit array (positive, sum 1/2)."""
    aq = tg.azimuthal_quadrature
    if isinstance(spec, str):
        if spec == "exact":
            return exact_azimuthal_weights(aq)
        if spec == "equal":
            return np.full(aq.n_azim_2, 1.0 / (2 * aq.n_azim_2))
        raise ValueError(f"unknown azimuthal weights {spec!r} (exact, equal or an array)")
    a = np.ascontiguousarray(spec, np.float64).reshape(-1)
    if a.shape != (aq.n_azim_2,) or np.any(a <= 0) or abs(float(a.sum()) - 0.5) > 1e-12:
        raise ValueError("azimuthal weights must be n_azim/2 positive numbers that sum to 1/2")
    return a


class SolverBoundary:
    """Albedos and an incoming flux on the four sides of the domain (ids and names as ``track_end_sides``: 0 left, 1 right,
    2 bottom, 3 top).  ``albedo``: a scalar (all sides, all groups), a dict side name -> scalar or [G] (sides not named: 1,
    reflective), or an array [4, G]; every β in [0, 1].  ``incoming``: the isotropic angular flux ψ_inc that enters through a side,
    given the same ways (sides not named: 0), None: none; fixed-source runs only."""

    def __init__(self, albedo=1.0, incoming=None):
        self.albedo, self.incoming = albedo, incoming

    @staticmethod
    def _expand(v, G, default, what):
        if isinstance(v, dict):
            unknown = sorted(set(v) - set(SIDE_NAMES))
            if unknown:
                raise ValueError(f"unknown sides {unknown} in {what} (left, right, bottom, top)")
            a = np.full((4, G), float(default))
            for i, name in enumerate(SIDE_NAMES):
                if name in v:
                    a[i] = np.broadcast_to(np.asarray(v[name], np.float64), (G,))
            return a
        a = np.asarray(v, np.float64)
        if a.ndim == 0:
            return np.full((4, G), float(a))
        if a.shape != (4, G):
            raise ValueError(f"{what} must be a scalar, a dict by side name or an array [4, G] = {(4, G)}, got {a.shape}")
        return np.ascontiguousarray(a)

    def arrays(self, G: int):
        """``(albedo, incoming)`` as [4, G] arrays (``incoming`` None when none was given)."""
        be = self._expand(self.albedo, G, 1.0, "albedo")
        if not np.all(np.isfinite(be)) or np.any(be < 0) or np.any(be > 1):
            raise ValueError("every albedo must be finite and in [0, 1]")
        inc = None if self.incoming is None else self._expand(self.incoming, G, 0.0, "incoming")
        if inc is not None and (not np.all(np.isfinite(inc)) or np.any(inc < 0)):
            raise ValueError("every incoming flux must be finite and >= 0")
        return be, inc


def neutron_balance(xs, cell_material, phi, volumes, k_eff, source, current_out, current_in, adjoint=False) -> dict:
    """The balance of ``include/rt_segmentize.h`` per group, from a run's last φ and last sweep's currents: ``gain`` [G] =
    Σ_e V_e (χ_g F_e / k + Σ_g'≠g Σs[g'→g] φ_g' + S_g) (production / k, in-scatter, external source), ``removal`` [G] =
    Σ_e V_e (Σt_g − Σs[g→g]) φ_g, ``leakage`` [G] = Σ_s (J⁺ − J⁻) and ``defect`` = gain − removal − leakage, of the size of the
    iteration error.  ``adjoint``: with the transposed data, as the run used them."""
    mat = np.asarray(cell_material, np.int64)
    V = np.asarray(volumes, np.float64)[:, None]
    st, ss, nf, ch = xs.sigma_t[mat], xs.sigma_s[mat], xs.nu_sigma_f[mat], xs.chi[mat]
    if adjoint:
        fissile = nf.sum(1, keepdims=True) > 0
        ss, nf, ch = ss.transpose(0, 2, 1), np.where(fissile, ch, 0.0), nf
    G = st.shape[1]
    diag = ss[:, np.arange(G), np.arange(G)]
    k = 1.0 if k_eff is None else float(k_eff)
    prod = (nf * phi).sum(1, keepdims=True)
    gain = ch * prod / k + np.einsum("eh,ehg->eg", phi, ss) - diag * phi
    if source is not None:
        gain = gain + np.asarray(source, np.float64)
    gain, removal = (V * gain).sum(0), (V * (st - diag) * phi).sum(0)
    leakage = (np.asarray(current_out) - np.asarray(current_in)).sum(0)
    return dict(gain=gain, removal=removal, leakage=leakage, defect=gain - removal - leakage)


def region_balance(xs, cell_material, cell_region, phi, volumes, k_eff, source, region_current, adjoint=False) -> dict:
    """``neutron_balance`` per region, from a run's last φ and the last sweep's ``region_current`` J [R + 1, R + 1, G]: for region a
    the cells with ``cell_region == a``, J⁺ = J[a → b] and J⁻ = J[b → a] over b ≠ a (b = R: outside the track, i.e. the domain's
    boundary).  Returns ``gain``, ``removal``, ``leakage`` (net outflow), ``net_inflow`` = −leakage and ``defect`` =
    gain − removal − leakage, each [R, G]; the defect is of the size of the iteration error."""
    J = np.asarray(region_current, np.float64)
    R = J.shape[0] - 1
    reg = np.asarray(cell_region, np.int64)
    mat = np.asarray(cell_material, np.int64)
    phi, V = np.asarray(phi, np.float64), np.asarray(volumes, np.float64)
    src = None if source is None else np.asarray(source, np.float64)
    rows = []
    for a in range(R):
        m = reg == a
        others = np.arange(R + 1) != a
        rows.append(neutron_balance(xs, mat[m], phi[m], V[m], k_eff, None if src is None else src[m], J[a, others], J[others, a], adjoint=adjoint))
    out = {key: np.stack([r[key] for r in rows]) for key in ("gain", "removal", "leakage", "defect")}
    out["net_inflow"] = -out["leakage"]
    return out


@dataclass
class Cmfd:
    """The coarse-mesh (pCMFD) acceleration of ``include/rt_segmentize.h`` over ``regions=``: ``coupling`` D̂ [R, R, G], symmetric
    and >= 0 (None: 0; ``diffusion_coupling`` builds one), ``relax`` θ in (0, 1], and the coarse power iteration's ``max_iter`` and
    ``tol``."""
    coupling: Optional[np.ndarray] = None
    relax: float = 1.0
    max_iter: int = 200
    tol: float = 1e-10

    def check(self, n_regions: int, n_groups: int):
        """Raises ``ValueError`` for what ``rt_solver_set_cmfd`` would refuse in these fields."""
        if not (0.0 < float(self.relax) <= 1.0):
            raise ValueError("Cmfd.relax must lie in (0, 1]")
        if int(self.max_iter) < 0 or not (float(self.tol) >= 0.0) or not math.isfinite(float(self.tol)):
            raise ValueError("Cmfd.max_iter must be >= 0 and Cmfd.tol finite and >= 0")
        if self.coupling is not None:
            co = np.asarray(self.coupling, np.float64)
            if co.shape != (n_regions, n_regions, n_groups):
                raise ValueError(f"Cmfd.coupling must have shape [R, R, G] = {(n_regions, n_regions, n_groups)}, got {co.shape}")
            if not np.all(np.isfinite(co)) or np.any(co < 0):
                raise ValueError("every Cmfd.coupling entry must be finite and >= 0")
            if not np.array_equal(co, co.transpose(1, 0, 2)):
                raise ValueError("Cmfd.coupling must be symmetric in its two regions")


@dataclass
class Krylov:
    """Restarted GMRES of ``include/rt_segmentize.h`` ("Krylov") for fixed-source runs and transient steps: at most ``m`` Krylov
    vectors per cycle (1 .. 64; the basis holds (m + 1) vectors of n_cells·G + 2·n_tracks·G·P doubles on the device) and the
    relative GMRES residual ``tol_lin`` at which a cycle stops early."""
    m: int = 20
    tol_lin: float = 1e-2

    def check(self):
        if not (1 <= int(self.m) <= 64):
            raise ValueError("Krylov.m must lie in 1 .. 64")
        if not (0.0 <= float(self.tol_lin) < 1.0):
            raise ValueError("Krylov.tol_lin must lie in [0, 1)")


def _as_krylov(krylov):
    if krylov is None or krylov is False:
        return None
    if krylov is True:
        return Krylov()
    if isinstance(krylov, Krylov):
        krylov.check()
        return krylov
    raise TypeError("krylov must be True, False, None or a Krylov")


def _as_cmfd(cmfd):
    if cmfd is None or cmfd is False:
        return None
    if cmfd is True:
        return Cmfd()
    if isinstance(cmfd, Cmfd):
        return cmfd
    raise TypeError("cmfd must be True, False, None or a Cmfd")


def diffusion_coupling(tg, cell_region, xs, cell_material) -> np.ndarray:
    """A diffusion-like coupling D̂ [R, R, G] for ``Cmfd(coupling=...)``, on the host from the mesh: A_ab the summed length of the mesh
    edges between cells of regions a and b, d_ab the distance of the volume-weighted (cell areas) region centroids, D_a the
    volume-weighted 1 / (3 Σt) of the region, and D̂_ab = A_ab · 2 D_a D_b / ((D_a + D_b) d_ab); 0 for regions that share no edge
    and on the diagonal.  It only shapes the coarse iteration (a preconditioner): the converged answer does not depend on it."""
    mesh = tg.mesh
    cn = np.asarray(mesh.cell_nodes, np.int64) - 1
    nc = cn.shape[0]
    reg = np.asarray(cell_region, np.int64)
    mat = np.asarray(_cell_material(tg, cell_material), np.int64)
    if reg.shape != (nc,) or mat.shape != (nc,):
        raise ValueError("cell_region and cell_material must have one entry per cell")
    if reg.size and reg.min() < 0:
        raise ValueError("region ids must be >= 0")
    R, G = int(reg.max(initial=-1)) + 1, xs.n_groups
    x, y = mesh.x[cn], mesh.y[cn]
    area = 0.5 * np.abs((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]))
    Va = np.bincount(reg, weights=area, minlength=R)
    Vs = np.where(Va > 0, Va, 1.0)
    cen = np.stack([np.bincount(reg, weights=area * x.mean(1), minlength=R) / Vs, np.bincount(reg, weights=area * y.mean(1), minlength=R) / Vs], 1)
    D = np.stack([np.bincount(reg, weights=area / (3.0 * xs.sigma_t[mat, g]), minlength=R) / Vs for g in range(G)], 1)  # [R, G]
    # every edge (sorted node pair) with the cells on its two sides
    ed = np.sort(np.concatenate([cn[:, [0, 1]], cn[:, [1, 2]], cn[:, [2, 0]]]), axis=1)
    owner = np.tile(np.arange(nc), 3)
    order = np.lexsort((ed[:, 1], ed[:, 0]))
    ed, owner = ed[order], owner[order]
    same = (ed[1:] == ed[:-1]).all(1)
    c0, c1, e2 = owner[:-1][same], owner[1:][same], ed[:-1][same]
    length = np.hypot(mesh.x[e2[:, 0]] - mesh.x[e2[:, 1]], mesh.y[e2[:, 0]] - mesh.y[e2[:, 1]])
    cross = reg[c0] != reg[c1]
    A = np.zeros((R, R))
    np.add.at(A, (reg[c0][cross], reg[c1][cross]), length[cross])
    A = A + A.T
    out = np.zeros((R, R, G))
    a, b = np.nonzero(A > 0)
    dab = np.hypot(cen[a, 0] - cen[b, 0], cen[a, 1] - cen[b, 1])
    ok = dab > 0
    a, b, dab = a[ok], b[ok], dab[ok]
    out[a, b] = A[a, b, None] * 2.0 * D[a] * D[b] / ((D[a] + D[b]) * dab[:, None])
    return 0.5 * (out + out.transpose(1, 0, 2))  # (the two orders of a pair differ by rounding: exactly symmetric)


@dataclass
class SolverResult:
    k_eff: Optional[float]        # None in fixed-source mode
    phi: np.ndarray               # [n_cells, G]; eigenvalue mode: scaled to Σ_e V_e Σ_g νΣf φ = 1
    volumes: np.ndarray           # [n_cells], with the solver's azimuthal weights
    iterations: int
    converged: bool
    k_history: np.ndarray         # k after every iteration
    ms_per_iteration: float       # HIP-event time of the iterations / iterations
    residual: float
    solver: object = None         # the device solver (rt_solver handle), for a further run
    current: Optional[np.ndarray] = None  # net current (Jx, Jy) [n_cells, G, 2] with sigma_s1; None when isotropic
    flux_moments: Optional[np.ndarray] = None   # scheme="linear": (φx, φy) [n_cells, G, 2], the moments of φ about the centroid
    flux_gradient: Optional[np.ndarray] = None  # ... C⁻¹ φ⃗ [n_cells, G, 2]: φ(r) ≈ phi + flux_gradient·(r − centroid)
    centroids: Optional[np.ndarray] = None      # ... track-based cell centroids [n_cells, 2]; all three None when flat
    adjoint: bool = False         # True: phi (current, flux_moments, ...) are the adjoint quantities of include/rt_segmentize.h
    current_out: Optional[np.ndarray] = None    # boundary=...: the last sweep's partial currents J⁺ [4, G] out through every side
    current_in: Optional[np.ndarray] = None     # ... J⁻ [4, G], in through every side (left, right, bottom, top)
    leakage: Optional[np.ndarray] = None        # ... J⁺ − J⁻ [4, G]
    balance: Optional[dict] = None              # ... neutron_balance: gain, removal, leakage, defect [G]; all four None without
    reproducible: bool = False    # True: the run used the fixed-order sweep tallies (rt_solver_set_reproducible): its bits repeat
    precision: str = "double"     # "single": the run swept the angular flux in binary32 (rt_solver_set_precision); sums, fold, k in FP64
    region_current: Optional[np.ndarray] = None  # regions=...: the last sweep's partial currents J [R + 1, R + 1, G], J[a, b] from a to b (R: outside)
    region_balance: Optional[dict] = None        # ... region_balance: gain, removal, leakage, net_inflow, defect [R, G]; both None without
    cmfd: Optional[dict] = None   # cmfd=...: the last coarse step's factors [R, G], its iterations, skipped_regions, skipped_steps
    volume_correction: Optional[str] = None       # "angle" / "cell": chord lengths renormalised to the cells' areas; `volumes` are then V'
    cell_area: Optional[np.ndarray] = None        # ... the cells' exact areas A_e [n_cells]
    volume_factor: Optional[np.ndarray] = None    # ... f [n_cells, n_azim_2]
    volume_correction_info: Optional[dict] = None  # ... unseen_pairs, zero_area_cells, zero_volume_cells, f_min, f_max; all None without
    source_region: Optional[np.ndarray] = None     # source_regions=...: the cells' regions [mesh cells]; phi, volumes, current are then [n_src, ...]
    source_region_info: Optional[dict] = None      # ... n_src, rows / largest count / chunks before and after the merge; both None without
    xs: Optional["CrossSections"] = None           # the cross sections of the run (what ``solve_transient`` starts from)
    krylov: Optional[dict] = None                  # krylov=...: cycles, vectors, sweeps, the last cycle's vectors / breakdown / resnorm; None without
    angular_moments: Optional[np.ndarray] = None   # sigma_s2 (sigma_s3): φ_lm [n_cells, G, NM], NM = 6 (10), slot 0 is phi; None below order 2
    moment_lm: Optional[np.ndarray] = None         # ... the (l, m) of every slot [NM, 2]
    void_cells: Optional[np.ndarray] = None        # [n_cells] bool: the cells of a void material (Σt = 0); there phi is the track-length flux

    def to_cells(self, a):
        """An array per source region (``phi``, ``volumes``, ``current``) spread over the mesh's cells: ``a[source_region]``; ``a``
        itself without source regions."""
        return np.asarray(a) if self.source_region is None else np.asarray(a)[self.source_region]

    def sample(self, points, groups=None, fill=float("nan")):
        """The flux at ``points`` [n, 2], from the φ the run's solver holds on the device (``DeviceSolver.sample``): ``(cells,
        values [n, ng])`` — the cells' 1-based ids (-1: outside, ``fill`` there), φ of the cell or of its source region, with
        ``scheme="linear"`` phi + flux_gradient·(r − centroid)."""
        return self.solver.sample(points, groups, fill)

    def sample_grid(self, x0, y0, dx, dy, nx, ny, groups=None, fill=float("nan")):
        """``sample`` on the raster (x0 + i·dx, y0 + j·dy): ``(cells [ny, nx], values [ny, nx, ng])`` — a flux map."""
        return self.solver.sample_grid(x0, y0, dx, dy, nx, ny, groups, fill)


def _cell_material(tg, cell_material):
    if isinstance(cell_material, dict):
        reg = getattr(tg.mesh.model, "cell_region", None)
        if reg is None:
            raise ValueError("cell_material given by region name, but the mesh has no cell regions")
        missing = sorted(set(np.unique(reg)) - set(cell_material))
        if missing:
            raise ValueError(f"no material for regions {missing}")
        return np.asarray([cell_material[r] for r in reg], np.int32)
    cm = np.asarray(cell_material)
    if cm.ndim == 0:
        return np.full(tg.mesh.num_cells, int(cm), np.int32)
    return np.ascontiguousarray(cm, np.int32)


def _cell_regions(cm, regions):
    """``regions`` as an int32 array per cell: ``"material"`` is ``cell_material``."""
    if isinstance(regions, str):
        if regions != "material":
            raise ValueError(f'unknown regions {regions!r} ("material" or an int array per cell)')
        return np.ascontiguousarray(cm, np.int32)
    reg = np.asarray(regions)
    if reg.shape != np.shape(cm) or not np.issubdtype(reg.dtype, np.integer):
        raise ValueError("regions must be an int array with one entry per cell")
    if reg.size and (reg.min() < 0 or reg.max() >= 127):
        raise ValueError("region ids must lie in 0 .. 126 (at most 127 regions)")
    return np.ascontiguousarray(reg, np.int32)


def _source_regions(cm, source_regions):
    """``source_regions`` as (int32 array per cell, n_src): ``"material"`` is ``cell_material``'s distinct values, numbered in
    ascending order.  A region whose cells carry different materials raises ``ValueError``."""
    if isinstance(source_regions, str):
        if source_regions != "material":
            raise ValueError(f'unknown source_regions {source_regions!r} ("material" or an int array per cell)')
        sr = np.unique(cm, return_inverse=True)[1].reshape(-1)
    else:
        sr = np.asarray(source_regions)
        if sr.shape != np.shape(cm) or not np.issubdtype(sr.dtype, np.integer):
            raise ValueError("source_regions must be an int array with one entry per cell")
    sr = np.ascontiguousarray(sr, np.int32)
    if sr.size == 0 or sr.min() < 0:
        raise ValueError("source region ids must be >= 0, one per cell")
    n_src = int(sr.max()) + 1
    lo = np.full(n_src, np.iinfo(np.int64).max); hi = np.full(n_src, -1)
    np.minimum.at(lo, sr, cm); np.maximum.at(hi, sr, cm)
    if (hi < 0).any():
        raise ValueError(f"source region {int(np.flatnonzero(hi < 0)[0])} has no cell (the ids must be 0 .. n_src - 1 without gaps)")
    if (lo != hi).any():
        raise ValueError(f"source region {int(np.flatnonzero(lo != hi)[0])} mixes materials: every cell of a region must carry the same one")
    return sr, n_src


def _device_tracks(tg, device):
    """The tracks' device handle after ``segmentize`` (run here with ``fetch=False`` if it has not run), links set."""
    from .segmentize import segmentize

    dt = getattr(tg, "device_tracks", None)
    if dt is None or getattr(dt, "_h", None) is None or dt.total is None:
        segmentize(tg, fetch=False, device=device)
        dt = tg.device_tracks
    dt.sweep_set_links(tg)
    return dt


def _volume_correction(tg, volume_correction):
    """The mode of a solve: None is what the TrackGenerator says (``volume_correction=True`` there: "angle"), False is off."""
    if volume_correction is None:
        return "angle" if getattr(tg, "volume_correction", False) else None
    if volume_correction is False:
        return None
    if volume_correction is True:
        return "angle"
    if volume_correction not in ("angle", "cell"):
        raise ValueError('volume_correction must be None, "angle" or "cell"')
    return volume_correction


def _solve(tg, xs, cell_material, mode, source, polar, azim_weights, tol_k, tol_flux, max_iter, device, scheme="flat", adjoint=False,
           boundary=None, reproducible=False, precision="double", regions=None, cmfd=None, volume_correction=None, source_regions=None,
           krylov=None):
    acc = _as_cmfd(cmfd)
    kry = _as_krylov(krylov)
    vc = _volume_correction(tg, volume_correction)
    if source_regions is not None:
        for on, what in ((scheme == "linear", 'scheme="linear" (centroids and the C matrices are per cell)'),
                         (reproducible, "reproducible=True (the tally index is per original row slot)"),
                         (regions is not None or acc is not None, "regions= / cmfd= (the coarse-mesh prolongation reads the compact records' cells)"),
                         (vc is not None, "volume_correction (its factors are per cell)")):
            if on:
                raise ValueError(f"source_regions together with {what} is not supported")
    if vc is not None and scheme == "linear":
        raise ValueError('volume_correction together with scheme="linear" is not supported (scaled chords would move the linear '
                         "source's midpoints off the track)")
    if vc is not None and reproducible:
        raise ValueError("volume_correction together with reproducible=True is not supported (the tracked lengths are an atomic sum)")
    if acc is not None and regions is None:
        raise ValueError("cmfd needs regions= (its coarse cells)")
    if isinstance(xs, CrossSections) and xs.void_materials.any():  # (what rt_solver's setters refuse on a solver that holds a void material)
        for on, what in ((scheme == "linear", 'scheme="linear" (the linear source)'),
                         (xs.scatter_order >= 2, "sigma_s2 / sigma_s3 (P2 / P3 scattering)"),
                         (precision == "single", 'precision="single" (the single-precision sweep)'),
                         (reproducible, "reproducible=True (the reproducible tallies)"),
                         (regions is not None or acc is not None, "regions= / cmfd= (region currents, the coarse-mesh acceleration)"),
                         (source_regions is not None, "source_regions= (source regions)"),
                         (vc is not None, "volume_correction (the volume correction)"),
                         (kry is not None, "krylov= (restarted GMRES)")):
            if on:
                raise ValueError(f"solve: void materials (sigma_t = 0: material {int(np.flatnonzero(xs.void_materials)[0])}) together with {what} "
                                 "are not supported")
    if precision not in _capi.PRECISIONS:
        raise ValueError('precision must be "double" or "single"')
    if not isinstance(xs, CrossSections):
        raise TypeError("xs must be a CrossSections")
    if scheme not in ("flat", "linear"):
        raise ValueError(f"unknown scheme {scheme!r} (flat or linear)")
    linear = scheme == "linear"
    if linear and xs.sigma_s1 is not None:
        raise ValueError('scheme="linear" together with sigma_s1 (P1 scattering) is not supported')
    if boundary is not None and not isinstance(boundary, SolverBoundary):
        raise TypeError("boundary must be a SolverBoundary")
    if boundary is not None:
        boundary.arrays(xs.n_groups)  # (raises on a bad albedo or incoming flux before anything is built)
    pq = PolarQuadrature(polar)
    alpha = azimuthal_weights(tg, azim_weights)
    dt = _device_tracks(tg, device)
    cm = _cell_material(tg, cell_material)
    reg = None if regions is None else _cell_regions(cm, regions)
    sr, cm_r = None, cm  # (cm_r: the material of every flat-source region — of every cell without source regions)
    if source_regions is not None:
        sr, n_src = _source_regions(cm, source_regions)
        cm_r = np.zeros(n_src, cm.dtype)
        cm_r[sr] = cm
        if source is not None and (np.ndim(source) == 0 or np.shape(source) == (xs.n_groups,)):
            source = np.broadcast_to(source, (n_src, xs.n_groups))
        if source is not None and np.shape(source) != (n_src, xs.n_groups):
            raise ValueError("source must have shape [n_src, G] with source_regions")
    if acc is not None:
        acc.check(int(reg.max(initial=-1)) + 1, xs.n_groups)
    sv = _capi.DeviceSolver(dt, cm, xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi,
                            pq.sin_theta, pq.weights, alpha)
    if sr is not None:  # (first: the source below is per region; refused by the library on a shard's track set)
        sv.set_source_regions(sr, n_src)
    if source is not None:
        sv.set_source(source)
    if xs.scatter_order >= 2:  # (refused by the library, in a message that names both, together with what it does not run with)
        sv.set_scatter_pn(xs.scatter_order, xs.sigma_sl)
    elif xs.sigma_s1 is not None:
        sv.set_scatter_p1(xs.sigma_s1)
    if linear:
        sv.set_linear_source(True)
    if adjoint:
        sv.set_adjoint(True)
    if boundary is not None:
        sv.set_boundary(boundary, track_end_sides(tg))
    if reg is not None:  # (refused by the library together with reproducible=True or precision="single")
        sv.set_regions(reg)
    if acc is not None:  # (refused by the library together with an incoming boundary flux)
        sv.set_cmfd(True, acc.coupling, acc.relax, acc.max_iter, acc.tol)
    if reproducible:  # (last: the delta buffer is sized for the mode set above)
        sv.set_reproducible(True)
    if precision != "double":  # (refused by the library together with sigma_s1, scheme="linear" or reproducible=True)
        sv.set_precision(precision)
    if vc is not None:  # (refused by the library on a shard's track set)
        sv.set_volume_correction(vc)
    if kry is not None:  # (last: refused by the library, in a message that names both, together with what it does not run with)
        sv.set_krylov(kry.m, kry.tol_lin)
    r = sv.run(mode, int(max_iter), float(tol_k), float(tol_flux))
    f = sv.fetch(r["iterations"])
    mom = sv.fetch_moments() if linear else dict(flux_moments=None, flux_gradient=None)
    centroids = sv.fetch_geometry()["centroids"] if linear else None
    current = sv.fetch_current() if xs.sigma_s1 is not None else None
    it = r["iterations"]
    bnd = dict(current_out=None, current_in=None, leakage=None, balance=None)
    if boundary is not None:
        bnd.update(sv.fetch_boundary())
        bnd["leakage"] = bnd["current_out"] - bnd["current_in"]
        eigen = mode == _capi.DeviceSolver.EIGENVALUE
        bnd["balance"] = neutron_balance(xs, cm_r, f["phi"], f["volumes"], r["k_eff"] if eigen else None, None if eigen else source,
                                         bnd["current_out"], bnd["current_in"], adjoint=adjoint)
    if reg is not None:
        eigen = mode == _capi.DeviceSolver.EIGENVALUE
        bnd["region_current"] = sv.fetch_regions()
        bnd["region_balance"] = region_balance(xs, cm, reg, f["phi"], f["volumes"], r["k_eff"] if eigen else None, None if eigen else source,
                                               bnd["region_current"], adjoint=adjoint)
    if acc is not None and it > 0:
        bnd["cmfd"] = sv.fetch_cmfd()
    if vc is not None:
        v = sv.fetch_volume_correction()
        bnd.update(volume_correction=vc, cell_area=v.pop("area"), volume_factor=v.pop("factor"), volume_correction_info=v)
    if sr is not None:
        bnd.update(source_region=sr, source_region_info=sv.source_region_info())
    if kry is not None:
        bnd["krylov"] = sv.krylov_info()
    if xs.scatter_order >= 2:
        bnd.update(sv.fetch_angular_moments())
    return SolverResult(k_eff=r["k_eff"] if mode == _capi.DeviceSolver.EIGENVALUE else None, phi=f["phi"], volumes=f["volumes"],
                        iterations=it, converged=r["converged"], k_history=f["k_history"],
                        ms_per_iteration=r["device_ms"] / it if it else 0.0, residual=r["residual"], solver=sv, current=current,
                        flux_moments=mom["flux_moments"], flux_gradient=mom["flux_gradient"], centroids=centroids, adjoint=bool(adjoint),
                        reproducible=bool(reproducible), precision=precision, xs=xs, void_cells=xs.void_materials[np.asarray(cm_r, np.int64)], **bnd)


def solve_eigenvalue(tg: TrackGenerator, xs: CrossSections, cell_material, polar="TY3", azim_weights="exact",
                     tol_k=1e-8, tol_flux=1e-7, max_iter=1000, device: int = 0, scheme: str = "flat", adjoint: bool = False,
                     boundary: Optional["SolverBoundary"] = None, reproducible: bool = False, precision: str = "double",
                     regions=None, cmfd=None, volume_correction=None, source_regions=None) -> SolverResult:
    """Power iteration for k_eff on the device.  ``cell_material``: material index per cell [n_cells] (or one index for all,
    or a dict region name -> index over ``tg.mesh.model.cell_region``).  ``polar``: a ``PolarQuadrature`` spec;
    ``azim_weights``: "exact", "equal" or an array.  Uses ``tg.device_tracks`` when ``segmentize(tg, fetch=False)`` has run,
    else segmentizes first; the boundary conditions are the ones ``trace`` linked.  ``scheme``: "flat" (a constant source per cell)
    or "linear" (a source linear in space per cell; not together with ``sigma_s1``).  ``adjoint=True``: the adjoint problem — the
    same k_eff, ``phi`` the adjoint flux φ† scaled to Σ_e V_e Σ_g χ_g φ† = 1 over the fissile cells (``current``: that of the
    transposed problem, J† = −J*; ``flux_moments``: those of φ†).  ``boundary``: a ``SolverBoundary`` (albedos per side and group;
    the result then carries ``current_out``, ``current_in``, ``leakage`` and ``balance``); None: what ``trace`` linked, nothing
    tallied.  ``reproducible=True``: the sweep tallies in a fixed order instead of FP64 atomics (``rt_solver_set_reproducible``) — a
    repeated run returns the same bits in every field, at the price of a delta buffer on the device and a slower sweep.
    ``precision="single"``: the sweep carries the angular flux in binary32 (``rt_solver_set_precision``; every sum, the fold, k and
    the residual stay FP64) — k then differs from the FP64 run's in about the seventh digit; not together with ``sigma_s1``,
    ``scheme="linear"`` or ``reproducible=True`` (``RtError``).  ``regions``: an int array per cell (ids 0 .. R − 1, R <= 127) or
    ``"material"`` (``cell_material``): every sweep tallies the partial currents between the regions (``rt_solver_set_regions``) and
    the result carries ``region_current`` [R + 1, R + 1, G] and ``region_balance``; not together with ``reproducible=True`` or
    ``precision="single"`` (``RtError``).  ``cmfd``: True or a ``Cmfd`` — the partial-current coarse-mesh acceleration over the
    regions (``rt_solver_set_cmfd``; needs ``regions``): the same converged k and φ in fewer iterations; the result carries the last
    coarse step under ``cmfd``.  ``volume_correction``: ``"angle"`` or ``"cell"`` — the chord lengths the sweeps read are renormalised
    so that every cell's tracked area equals its exact area, per azimuthal angle or with one factor per cell
    (``rt_solver_set_volume_correction``); ``volumes`` are then the corrected V' and the result carries ``cell_area``,
    ``volume_factor`` and ``volume_correction_info``; None: what ``tg.volume_correction`` says (True there: ``"angle"``), False: off.
    Not together with ``scheme="linear"`` or ``reproducible=True`` (``ValueError``).  ``source_regions``: an int array per cell or
    ``"material"`` — every flat-source region a set of cells of one material, the sweeps over rows merged per region
    (``rt_solver_set_source_regions``); ``cell_material`` stays per mesh cell (a mixed region: ``ValueError``), ``phi``, ``volumes``
    and ``current`` are per source region, the result carries ``source_region`` and ``source_region_info``, and
    ``result.to_cells(a)`` spreads an array over the cells.  Not together with ``scheme="linear"``, ``reproducible=True``,
    ``regions`` / ``cmfd`` or ``volume_correction`` (``ValueError``)."""
    return _solve(tg, xs, cell_material, _capi.DeviceSolver.EIGENVALUE, None, polar, azim_weights, tol_k, tol_flux, max_iter, device, scheme,
                  adjoint, boundary, reproducible, precision, regions, cmfd, volume_correction, source_regions)


def solve_fixed_source(tg: TrackGenerator, xs: CrossSections, cell_material, source, polar="TY3", azim_weights="exact",
                       tol_k=1e-8, tol_flux=1e-7, max_iter=1000, device: int = 0, scheme: str = "flat", adjoint: bool = False,
                       boundary: Optional["SolverBoundary"] = None, reproducible: bool = False, precision: str = "double",
                       regions=None, cmfd=None, volume_correction=None, source_regions=None, krylov=None) -> SolverResult:
    """Source iteration with the external volumetric source ``source`` [n_cells, G] (k ≡ 1; fission multiplies).  Stops when
    the relative L2 change of φ is below ``tol_flux``.  Arguments as ``solve_eigenvalue``; with ``adjoint=True`` ``source`` is the
    adjoint source S† (for instance a detector cross section) and ``phi`` the importance φ†: Σ V S† φ = Σ V S φ†.  ``boundary``: a
    ``SolverBoundary``, here also with an incoming flux per side and group (``source`` may then be zero: a run driven from the
    boundary).  ``reproducible``, ``precision``, ``regions``, ``cmfd``, ``volume_correction``, ``source_regions``: as for ``solve_eigenvalue``
    (``cmfd`` not together with an incoming flux; with ``source_regions`` the ``source`` is [n_src, G]).  ``krylov``: True or a
    ``Krylov`` — restarted GMRES cycles in place of plain iterations (``rt_solver_set_krylov``): the same fixed point in fewer sweeps
    where the scattering ratio is near one; ``iterations`` and ``max_iter`` count sweeps, Krylov vectors included, and the result
    carries ``krylov``.  Not together with ``sigma_s1``, ``scheme="linear"``, ``precision="single"``, ``reproducible=True``, ``regions``
    / ``cmfd``, ``source_regions``, ``volume_correction`` or an incoming boundary flux (``RtError``)."""
    q = np.asarray(source, np.float64)
    G = xs.n_groups
    if (q.ndim == 0 or q.shape == (G,)) and source_regions is None:  # (with source_regions: _solve broadcasts over its n_src)
        q = np.broadcast_to(q, (tg.mesh.num_cells, G))
    return _solve(tg, xs, cell_material, _capi.DeviceSolver.FIXED_SOURCE, q, polar, azim_weights, tol_k, tol_flux, max_iter, device, scheme,
                  adjoint, boundary, reproducible, precision, regions, cmfd, volume_correction, source_regions, krylov)


# ---- adjoint-weighted integrals ------------------------------------------------------------------------------------------------
def _bilinear(forward, adjoint, A, cell_material, void_materials=None):
    """B_f = Σ_e V_e Σ_g Σ_g' φ†[e, g] A[f, m(e), g', g] φ[e, g'] for A [n_forms, M, G, G]: on the device (``rt_solver_bilinear``)
    when the two results carry their device solvers; for host results (``solver`` None: the numpy twins of the tests) by
    ``numpy.einsum`` with ``cell_material`` [n_cells], which they do not carry.  Void cells (``void_materials`` [M] bool for host
    results; the device knows its own) have zero weight: they take part in no reaction."""
    sa, sf = getattr(adjoint, "solver", None), getattr(forward, "solver", None)
    if sa is not None and sf is not None:
        return np.asarray(sa.bilinear(sf, A))
    if sa is not None or sf is not None:
        raise ValueError("one result carries a device solver and the other does not")
    if cell_material is None:
        raise ValueError("host results carry no materials: cell_material [n_cells] is needed")
    mat = np.asarray(cell_material, np.int64)
    V = np.asarray(forward.volumes, np.float64)
    live = V > 0
    if void_materials is not None:
        live = live & ~np.asarray(void_materials, bool)[mat]
    return np.einsum("e,eg,fehg,eh->f", V[live], np.asarray(adjoint.phi)[live], np.asarray(A)[:, mat[live]], np.asarray(forward.phi)[live])


def _fission_form(xs):
    """F[m, g', g] = χ_g νΣf_g'."""
    return xs.nu_sigma_f[:, :, None] * xs.chi[:, None, :]


def _check_pair(forward, adjoint):
    if getattr(forward, "source_region", None) is not None or getattr(adjoint, "source_region", None) is not None:
        raise ValueError("the adjoint-weighted integrals are per mesh cell: results of a run with source_regions= are not supported")
    if getattr(forward, "adjoint", False) or not getattr(adjoint, "adjoint", True):
        raise ValueError("forward must be a forward result and adjoint an adjoint one (solve_eigenvalue(..., adjoint=True))")
    if forward.k_eff is None:
        raise ValueError("forward must be an eigenvalue result")


def perturbation_reactivity(forward, adjoint, xs: CrossSections, xs_perturbed: CrossSections, cell_material=None) -> dict:
    """First-order estimate of the reactivity change Δρ = ρ' − ρ (ρ = 1 − 1/k) when ``xs`` becomes ``xs_perturbed`` (same materials
    and groups), from the forward and the adjoint eigenvalue results of the unperturbed problem:

        Δρ = ((1/k) B(ΔF) − B(ΔΣt) + B(ΔS)) / B(F),    B(A) = Σ_e V_e Σ_g Σ_g' φ†_{e,g} A[m(e)][g'→g] φ_{e,g'}

    with F = χ ⊗ νΣf, ΔF the difference of the two outer products, ΔS = ΔΣs0 and ΔΣt on the diagonal.  The S and F terms
    (changes of Σs0, νΣf and χ) are exact to first order for a flat source with isotropic scattering: the error is O(Δ²).  The ΔΣt
    term uses the scalar fluxes only — the isotropic-angular-flux approximation, exact in an infinite medium and approximate where
    the angular flux is anisotropic.  With ``sigma_s1`` or ``scheme="linear"`` the whole estimate is of that approximate kind (the
    first moments and the flux moments carry weight that the scalar integrals do not see; a change of ``sigma_s1`` is ignored).
    ``cell_material`` [n_cells]: only for host results without a device solver.  Returns ``delta_rho`` and the four integrals
    ``B_F``, ``B_dF``, ``B_dS``, ``B_dT``."""
    _check_pair(forward, adjoint)
    if xs_perturbed.sigma_t.shape != xs.sigma_t.shape:
        raise ValueError("xs and xs_perturbed must have the same materials and groups")
    M, G = xs.sigma_t.shape
    F = _fission_form(xs)
    dT = np.zeros((M, G, G))
    dT[:, np.arange(G), np.arange(G)] = xs_perturbed.sigma_t - xs.sigma_t
    A = np.stack([F, _fission_form(xs_perturbed) - F, xs_perturbed.sigma_s - xs.sigma_s, dT])
    bF, bdF, bdS, bdT = (float(b) for b in _bilinear(forward, adjoint, A, cell_material, xs.void_materials))
    return dict(delta_rho=(bdF / forward.k_eff - bdT + bdS) / bF, B_F=bF, B_dF=bdF, B_dS=bdS, B_dT=bdT)


def kinetics_parameters(forward, adjoint, xs: CrossSections, inv_velocity, beta, chi_delayed, cell_material=None) -> dict:
    """Adjoint-weighted kinetics parameters from the forward and the adjoint eigenvalue results: the generation time
    ``Lambda`` = B(diag 1/v) / B(F) and ``beta_eff`` [D] with β_eff,d = B(χ_d ⊗ β_d νΣf) / B(F), F = χ ⊗ νΣf and B as in
    ``perturbation_reactivity``.  ``inv_velocity`` [G] or [M, G]; ``beta`` [M, D] (delayed fractions per material and family);
    ``chi_delayed`` [M, D, G] (delayed spectra).  Returns ``Lambda``, ``beta_eff`` and ``B_F``."""
    _check_pair(forward, adjoint)
    M, G = xs.sigma_t.shape
    iv = np.asarray(inv_velocity, np.float64)
    iv = np.broadcast_to(iv, (M, G)) if iv.shape == (G,) else iv
    be = np.asarray(beta, np.float64)
    be = be.reshape(1, -1) if be.ndim == 1 and M == 1 else be
    if iv.shape != (M, G) or be.ndim != 2 or be.shape[0] != M:
        raise ValueError("inv_velocity must have shape [G] or [M, G] and beta [M, D]")
    D = be.shape[1]
    cd = np.asarray(chi_delayed, np.float64)
    cd = cd.reshape(M, D, G) if cd.size == M * D * G else cd
    if cd.shape != (M, D, G):
        raise ValueError(f"chi_delayed must have shape [M, D, G] = {(M, D, G)}")
    V = np.zeros((M, G, G))
    V[:, np.arange(G), np.arange(G)] = iv
    Ad = (be[:, :, None] * xs.nu_sigma_f[:, None, :])[:, :, :, None] * cd[:, :, None, :]  # [M, D, g', g]
    A = np.concatenate([np.stack([_fission_form(xs), V]), Ad.transpose(1, 0, 2, 3)])
    b = _bilinear(forward, adjoint, A, cell_material, xs.void_materials)
    return dict(Lambda=float(b[1] / b[0]), beta_eff=np.asarray(b[2:] / b[0]), B_F=float(b[0]))


# ---- transients -----------------------------------------------------------------------------------------------------------------
class Kinetics:
    """Kinetics data of a transient, in the conventions of ``kinetics_parameters`` plus the decay constants: ``inv_velocity`` [G] or
    [M, G] (1/v, > 0), ``beta`` [M, D] (delayed fractions per material and family; [D] for one material), ``decay`` [D] (λ_d, > 0),
    ``chi_delayed`` [M, D, G] (delayed spectra; any array of M·D·G values).  ``arrays(xs)`` returns them shaped for ``xs`` and checks
    the prompt spectrum χ − Σ_d β_d χd_d >= −1e-14 in every material and group."""

    def __init__(self, inv_velocity, beta, decay, chi_delayed):
        self.inv_velocity = np.asarray(inv_velocity, np.float64)
        self.beta = np.asarray(beta, np.float64)
        self.decay = np.ascontiguousarray(decay, np.float64).reshape(-1)
        self.chi_delayed = np.asarray(chi_delayed, np.float64)
        D = len(self.decay)
        if D < 1 or not np.all(np.isfinite(self.decay)) or np.any(self.decay <= 0):
            raise ValueError("decay must hold at least one decay constant, every one finite and > 0")
        if self.beta.ndim not in (1, 2) or self.beta.shape[-1] != D:
            raise ValueError(f"beta must have shape [M, D] with D = {D} families (the length of decay), got {self.beta.shape}")
        if not np.all(np.isfinite(self.beta)) or np.any(self.beta < 0):
            raise ValueError("every beta must be finite and >= 0")
        if not np.all(np.isfinite(self.inv_velocity)) or np.any(self.inv_velocity <= 0) or self.inv_velocity.ndim not in (1, 2):
            raise ValueError("inv_velocity must have shape [G] or [M, G], every entry finite and > 0")
        if not np.all(np.isfinite(self.chi_delayed)) or np.any(self.chi_delayed < 0):
            raise ValueError("every chi_delayed must be finite and >= 0")

    @property
    def n_families(self) -> int:
        return len(self.decay)

    def arrays(self, xs: "CrossSections"):
        """``(inv_velocity [M, G], beta [M, D], decay [D], chi_delayed [M, D, G])`` for ``xs``; ``ValueError`` for a shape that
        does not fit or a negative prompt spectrum."""
        M, G = xs.sigma_t.shape
        D = self.n_families
        iv = np.broadcast_to(self.inv_velocity, (M, G)) if self.inv_velocity.shape == (G,) else self.inv_velocity
        be = self.beta.reshape(1, -1) if self.beta.ndim == 1 and M == 1 else self.beta
        if iv.shape != (M, G) or be.shape != (M, D):
            raise ValueError(f"inv_velocity must have shape [G] or [M, G] = {(M, G)} and beta [M, D] = {(M, D)}")
        cd = self.chi_delayed.reshape(M, D, G) if self.chi_delayed.size == M * D * G else self.chi_delayed
        if cd.shape != (M, D, G):
            raise ValueError(f"chi_delayed must have shape [M, D, G] = {(M, D, G)}")
        iv, be, cd = (np.ascontiguousarray(a, np.float64) for a in (iv, be, cd))
        self.check_prompt(xs, be, cd)
        return iv, be, self.decay, cd

    @staticmethod
    def check_prompt(xs, beta, chi_delayed):
        prompt = xs.chi - np.einsum("md,mdg->mg", beta, chi_delayed)
        if np.any(prompt < -1e-14):
            m, g = (int(i) for i in np.argwhere(prompt < -1e-14)[0])
            raise ValueError(f"the prompt spectrum chi - sum_d beta_d chi_delayed_d of material {m}, group {g} is {prompt[m, g]:g} "
                             "(must be >= 0: the delayed part exceeds chi there)")


@dataclass
class TransientResult:
    times: np.ndarray             # [n_steps + 1], times[0] = 0
    production: np.ndarray        # [n_steps + 1]: F(φ(t)) = Σ_e V_e Σ_g νΣf φ, the relative power; production[0] = 1
    inner_iterations: np.ndarray  # [n_steps]: inner iterations of every step
    residual: np.ndarray          # [n_steps]: the last inner iteration's flux residual
    converged: np.ndarray         # [n_steps] bool: the step's residual got below tol within max_inner iterations
    phi: np.ndarray               # [n_cells, G] at the last time
    precursors: np.ndarray        # [n_cells, D] at the last time
    settle_iterations: int        # iterations the boundary fluxes took to settle before the first step
    settle_residual: float
    k_eff: float                  # k0: the eigenvalue the transient is normalised with
    ms_per_step: np.ndarray       # [n_steps]: HIP-event time of every step
    phi_history: Optional[np.ndarray] = None  # keep_flux=True: [n_steps + 1, n_cells, G]
    krylov_vectors: Optional[np.ndarray] = None  # krylov=...: [n_steps], the Krylov vectors among every step's inner iterations; None without


def solve_transient(result: SolverResult, kinetics: Kinetics, dt, n_steps: int, events=(), tol=1e-8, max_inner=200, settle_tol=1e-9,
                    settle_max_iter=500, keep_flux=False, krylov=None) -> TransientResult:
    """Continues the eigenvalue ``result`` (``solve_eigenvalue``; its device solver does the work) in time: ``n_steps`` implicit-Euler
    steps of ``dt`` (a float, or a sequence of ``n_steps`` values) with the delayed-neutron data ``kinetics``.  ``events``: a sequence of
    ``(step_index, CrossSections)`` — the cross sections (same materials and groups) that hold from that step on, applied before it.
    Every step iterates until the flux residual < ``tol`` or ``max_inner`` iterations; before the first one the boundary fluxes settle
    (``settle_tol``, ``settle_max_iter``).  The scheme and what it does not run with: "Transient" in ``include/rt_segmentize.h``.
    A step that stops at ``max_inner`` is not an error: ``TransientResult.converged`` says which steps met ``tol`` (near critical, a
    step after a reactivity change can take thousands of unaccelerated iterations).  A cell that no track crosses (``volumes == 0``)
    enters no sum and iterates on its own — in a fissile material without bound over many steps — so ``phi``, ``phi_history`` and
    ``precursors`` may hold inf there: mask with ``result.volumes > 0``.  ``krylov``: True or a ``Krylov`` — every step's inner
    iterations are restarted-GMRES cycles (``rt_solver_set_krylov``; ``inner_iterations`` and ``max_inner`` count sweeps, Krylov vectors
    included, ``krylov_vectors`` how many of them were); None: plain iterations, whatever an earlier call left set.
    ``ValueError`` for an adjoint result, a fixed-source result, a host result without a device solver, a result without its cross
    sections, data that does not fit."""
    if not isinstance(kinetics, Kinetics):
        raise TypeError("kinetics must be a Kinetics")
    if getattr(result, "adjoint", False):
        raise ValueError("result is an adjoint result (adjoint=True): a transient starts from a forward eigenvalue result")
    if result.k_eff is None:
        raise ValueError("result is a fixed-source result: a transient starts from an eigenvalue result (solve_eigenvalue)")
    n_steps = int(n_steps)
    dts = np.full(n_steps, float(dt)) if np.ndim(dt) == 0 else np.asarray(dt, np.float64).reshape(-1)
    if n_steps < 0 or dts.shape != (n_steps,) or not np.all(np.isfinite(dts)) or np.any(dts <= 0):
        raise ValueError("dt must be a positive float or a sequence of n_steps positive floats")
    xs = getattr(result, "xs", None)
    ev = {}
    for step, x in events:
        if not isinstance(x, CrossSections) or not (0 <= int(step) < max(n_steps, 1)):
            raise ValueError("events must be (step_index in 0 .. n_steps - 1, CrossSections) pairs")
        if xs is not None and x.sigma_t.shape != xs.sigma_t.shape:
            raise ValueError("the CrossSections of an event must have the materials and groups of the result's")
        ev[int(step)] = x
    if (xs is not None and xs.void_materials.any()) or any(x.void_materials.any() for x in ev.values()):
        raise ValueError("solve_transient: void materials (sigma_t = 0) together with a transient are not supported")
    if xs is not None:
        arrays = kinetics.arrays(xs)
        for x in ev.values():
            kinetics.check_prompt(x, arrays[1], arrays[3])
    sv = getattr(result, "solver", None)
    if sv is None:
        raise ValueError("result carries no device solver (a host twin's result): solve_transient runs on the device")
    if xs is None:
        raise ValueError("result carries no cross sections (result.xs is None: it was not made by solve_eigenvalue of this version): "
                         "set result.xs to the CrossSections of its run")
    if getattr(result, "source_region", None) is not None:
        raise ValueError("source_regions together with a transient is not supported")
    kry = _as_krylov(krylov)
    if kry is not None:
        sv.set_krylov(kry.m, kry.tol_lin)
    elif hasattr(_capi.lib(), "rt_solver_fetch_krylov") and sv.krylov_info()["m"]:  # (an earlier call's: a solver without it takes no new call)
        sv.set_krylov(0)
    r0 = sv.transient_begin(*arrays, settle_max_iter=settle_max_iter, settle_tol=settle_tol)
    times, prod, inner, res, ms, conv, kv = [0.0], [1.0], [], [], [], [], []
    hist = [np.array(result.phi, np.float64)] if keep_flux else None
    try:
        for n in range(n_steps):
            if n in ev:
                x = ev[n]
                sv.transient_set_xs(x.sigma_t, x.sigma_s, x.nu_sigma_f, x.chi)
            r = sv.transient_step(dts[n], max_inner, tol)
            times.append(times[-1] + float(dts[n])); prod.append(r["production"]); inner.append(r["iterations"]); res.append(r["residual"])
            ms.append(r["device_ms"]); conv.append(r["converged"])
            if kry is not None:
                kv.append(sv.krylov_info()["vectors"])
            if keep_flux:
                hist.append(sv.transient_fetch()["phi"])
        f = sv.transient_fetch()
    finally:
        if getattr(sv, "_h", None):
            try:
                sv.transient_end()
            except _capi.RtError:
                pass  # (a failed step has ended the transient already)
    return TransientResult(times=np.asarray(times), production=np.asarray(prod), inner_iterations=np.asarray(inner, np.int64),
                           residual=np.asarray(res), converged=np.asarray(conv, bool), phi=f["phi"], precursors=f["precursors"], settle_iterations=r0["iterations"],
                           settle_residual=r0["residual"], k_eff=r0["k_eff"], ms_per_step=np.asarray(ms),
                           phi_history=np.stack(hist) if keep_flux else None,
                           krylov_vectors=np.diff(np.asarray([0] + kv, np.int64)) if kry is not None else None)
