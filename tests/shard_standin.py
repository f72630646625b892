"""The step solver distributed.ShardedSolver drives, without a GPU: `ShardTwin`, a moc_ref.Twin over the oracle's records of ONE uid
range (`shard_records`, the per-track arrays cut to it, the plan's links restricted to it), seen the way the driver sees
_capi.DeviceSolver — `pointers()` and `ls_geometry_pointer()` hand out the twin's own arrays as torch tensors (zero-copy: what the
driver's collectives write is what the next step reads), the fetches return what `ShardedSolver.run` packs.  It computes what
rt_solver computes on a shard — partial volumes, partial tallies, the hand-over of fluxes inside the shard, the partial sums of the
linear source's geometry — by the twin's formulas and holds none of its own; everything that crosses ranks is the driver's."""
import numpy as np
import torch

import moc_ref


def shard_records(rec, lo, hi):
    """The records of uids [lo, hi) as a record dict of their own (offsets from 0)."""
    s0, s1 = int(rec["offsets"][lo]), int(rec["offsets"][hi])
    out = {k: np.asarray(rec[k])[s0:s1] for k in ("ell", "element", "px", "py", "qx", "qy")}
    out["offsets"] = np.asarray(rec["offsets"][lo:hi + 1]) - s0
    return out


class ShardTwin(moc_ref.Twin):
    """xs: a CrossSections (with sigma_s1: P1 scattering); linear: with the linear source's geometry calls."""

    def __init__(self, rec, lo, hi, local_links, azim_idx, delta_s, alpha, xs, mat, sin_polar, polar_weight, cos_phi=None, sin_phi=None,
                 linear=False):
        links = tuple(local_links[k] for k in ("next_fwd", "next_bwd", "dir_fwd", "dir_bwd", "bc_fwd", "bc_bwd"))
        cut = lambda x: None if x is None else np.asarray(x)[lo:hi]
        super().__init__(shard_records(rec, lo, hi), links, azim_idx[lo:hi], delta_s, alpha, xs.sigma_t, xs.sigma_s, xs.nu_sigma_f, xs.chi, mat,
                         sin_polar, polar_weight, sigma_s1=getattr(xs, "sigma_s1", None), linear=linear, cos_phi=cut(cos_phi),
                         sin_phi=cut(sin_phi))

    def pointers(self):
        """As rt_solver_pointers: `tally1` only with first moments, for the linear source only while a run is open."""
        t, has1 = torch.from_numpy, self.p1 or (self.linear and self.state is not None)
        return dict(volumes=t(self.vol), tally=t(self.T), tally1=t(self.T1) if has1 else None, psi_out=t(self.psi_out), psi_in=t(self.psi_in))

    def ls_geometry_pointer(self):
        acc, n = super().ls_geometry_pointer()
        return (None if acc is None else torch.from_numpy(acc), n)

    def fetch(self, iterations):
        return dict(phi=self.phi, volumes=self.vol.copy(), k_history=np.asarray(self.hist[:iterations]))

    def fetch_current(self):
        return self.mom

    def fetch_moments(self):
        return dict(flux_moments=self.mom, flux_gradient=self.gradient())

    def fetch_geometry(self):
        if not self.ls:
            raise moc_ref.StageError("fetch_geometry: the linear source is not on")
        return dict(centroids=self.cen, cmat=self.cmat, n_degenerate=int(self.deg.sum()))
