#!/usr/bin/env python3
"""Which of rt_solver's run options refuse each other, recorded from the library as it stands: for every ordered pair (A, B) of the
settable options (and "shard": the handle's links with one next uid 0) whether B's setter refuses after A and, where it does not,
whether rt_solver_begin refuses an eigenvalue and a fixed-source run; for every A what rt_solver_transient_begin says after a
completed eigenvalue run.  The problem is the 288-cell square of tests/test_gpu_solver_pn.py, G = 2, one material, one shared
handle.  tests/test_gpu_solver_option_matrix.py replays walk() against tests/golden/solver_option_refusals.json.  Needs a GPU.
usage: python tools/option_refusals.py OUT.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

EIG, FIX = 0, 1
# name -> the words that name the option in a message, whichever side it is on
WORDS = {
    "p1": "first-moment scattering", "pn": "P2", "linear": "linear source", "single": "single-precision sweep",
    "reproducible": "reproducible tallies", "regions": "region currents", "cmfd": "coarse-mesh acceleration",
    "source_regions": "source regions", "volume_correction": "volume correction", "krylov": "restarted GMRES", "adjoint": "adjoint mode",
    "incoming": "incoming flux", "shard": "shard", "transient": "transient",
}
OPTIONS = [o for o in WORDS if o != "transient"]


class Problem:
    """The square, its cross sections and one device handle; switch(sv, name) sets option `name` on a DeviceSolver of it."""

    def __init__(self, rt):
        from test_gpu_solver_shapes import _handle, _tg_model
        from test_solver_p1_cpu import square_model
        from test_solver_pn_cpu import with_moments

        self.rt = rt
        self.tg = tg = _tg_model(rt, square_model(rt), 8, 0.05, "mixed")
        self.xs = with_moments(rt, rt.CrossSections([[0.6, 1.0]], [[[0.30, 0.10], [0.0, 0.70]]], [[0.002, 0.05]], [[1.0, 0.0]]), 3, 2)
        self.cm = np.zeros(tg.mesh.num_cells, np.int64)
        self.dt = _handle(rt, tg)
        self.end_side = rt.track_end_sides(tg)
        self.shard_links = dict(next_fwd=np.array(tg.next_fwd_uid).copy(), next_bwd=tg.next_bwd_uid, dir_fwd=tg.dir_next_fwd,
                                dir_bwd=tg.dir_next_bwd, bc_fwd=tg.bc_fwd, bc_bwd=tg.bc_bwd)
        self.shard_links["next_fwd"][3] = 0

    def solver(self):
        from test_gpu_solver_shapes import _solver

        return _solver(self.rt, self.tg, self.dt, self.xs, self.cm)

    def restore(self):
        self.dt.sweep_set_links(self.tg)

    def switch(self, sv, name):
        nc, xs = self.tg.mesh.num_cells, self.xs
        if name == "p1":
            sv.set_scatter_p1(xs.sigma_s1)
        elif name == "pn":
            sv.set_scatter_pn(2, xs.sigma_sl)
        elif name == "linear":
            sv.set_linear_source(True)
        elif name == "single":
            sv.set_precision("single")
        elif name == "reproducible":
            sv.set_reproducible(True)
        elif name == "regions":
            sv.set_regions(np.zeros(sv.n_cells, np.int32))  # (per source region where those are set)
        elif name == "cmfd":
            sv.set_regions(np.zeros(sv.n_cells, np.int32))  # (per source region where those are set)
            sv.set_cmfd(True)
        elif name == "source_regions":
            sv.set_source_regions(np.zeros(nc, np.int32), 1)
        elif name == "volume_correction":
            sv.set_volume_correction("angle")
        elif name == "krylov":
            sv.set_krylov(4, 1e-2)
        elif name == "adjoint":
            sv.set_adjoint(True)
        elif name == "incoming":
            inc = np.zeros((4, sv.G))
            inc[0, 0] = 1.0
            sv.set_boundary(end_side=self.end_side, albedo=np.ones((4, sv.G)), incoming=inc)
        elif name == "shard":
            self.dt.sweep_set_links(self.shard_links)
        else:
            raise KeyError(name)


def _outcome(f):
    """None where f() went through, the library's message where it refused."""
    from raytracing_jl_amd import _capi

    try:
        f()
    except _capi.RtError as e:
        return str(e)
    return None


def _begin(sv, mode):
    def f():
        if mode == FIX:
            sv.set_source(np.ones((sv.n_cells, sv.G)))
        sv.begin(mode)
        sv.end()
    return _outcome(f)


def _transient_begin(sv):
    def f():
        sv.transient_begin(np.ones((1, sv.G)), np.array([[0.006]]), np.array([0.08]), np.array([[[1.0, 0.0]]]), settle_max_iter=2)
        sv.transient_end()
    return _outcome(f)


def walk(p, a):
    """What the library does with option `a` set first: "alone" (the two begins with nothing else), "transient" (the eigenvalue run
    and rt_solver_transient_begin after it) and, per second option b, "setter" (b's refusal, None: accepted), then either "begin"
    (the eigenvalue and the fixed-source begin's refusals) or "run_after_refusal" (a 2-iteration eigenvalue run's)."""
    out = {"alone": None, "transient": None, "then": {}}
    for b in [None, "transient"] + [o for o in OPTIONS if o != a]:
        sv = p.solver()
        try:
            first = _outcome(lambda: p.switch(sv, a))
            assert first is None, (a, first)
            if b is None:
                out["alone"] = {"begin": [_begin(sv, EIG), _begin(sv, FIX)]}
            elif b == "transient":
                run = _outcome(lambda: sv.run(EIG, 2, 0.0, 0.0))
                if run is not None:  # (no eigenvalue run with a set: the run first, on a solver without it, then a)
                    sv.close()
                    p.restore()
                    sv = p.solver()
                    sv.run(EIG, 2, 0.0, 0.0)
                    p.switch(sv, a)
                out["transient"] = {"run": run, "transient_begin": _transient_begin(sv)}
            else:
                rec = {"setter": _outcome(lambda: p.switch(sv, b))}
                if rec["setter"] is None:
                    rec["begin"] = [_begin(sv, EIG), _begin(sv, FIX)]
                else:
                    rec["run_after_refusal"] = _outcome(lambda: sv.run(EIG, 2, 0.0, 0.0))
                out["then"][b] = rec
        finally:
            p.restore()
            sv.close()
    return out


def main():
    import raytracing_jl_amd as rt

    p = Problem(rt)
    rec = {a: walk(p, a) for a in OPTIONS}
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, ensure_ascii=False, sort_keys=True)
        f.write("\n")
    n = sum(len(v["then"]) for v in rec.values())
    print("%d options, %d ordered pairs, %d setter refusals -> %s" % (len(rec), n, sum(r["setter"] is not None for v in rec.values() for r in v["then"].values()), sys.argv[1]))


if __name__ == "__main__":
    main()
