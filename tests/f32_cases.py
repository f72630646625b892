"""The problems and the bounds the single-precision tests share (tests/test_solver_f32_cpu.py, tests/test_gpu_solver_f32.py): every
case is run on the CPU by the FP64 twin (moc_ref.Twin) and by the binary32 twin (moc_ref_f32.TwinF32) for N iterations; the deviations
between the two — k, φ of the median φ, J⁺ / J⁻ of the largest J — pooled over the cases (their largest values) are E_ref, and a device
run in single precision must lie within 4 · E_ref of either twin (the issue's reasoning: per segment the twin commits about 2.5 ulp
— τ, F at 0.5, subtract, multiply, subtract — and the device at most about 6 with F at 4: 2.4x, rounded up).  E_ref never comes from
the device."""
import numpy as np

import moc_ref
import moc_ref_bc
import moc_ref_f32
from conftest import make_grid_model
from test_gpu_solver import _bcs, _cell_material_array, _materials, _traced, _xs
from test_gpu_solver_shapes import _bands
from test_solver_adjoint_cpu import adjoint_xs
from test_solver_p1_cpu import square_model

N = 12
EIG, FIX = 0, 1
BETA4 = np.array([[0.3, 0.9, 0.5], [1.0, 1.0, 1.0], [0.6, 0.6, 0.6], [0.0, 0.0, 0.0]])  # per side and group
# case -> (problem, G, polar, mode): 316 tracks with 9 components (passes 4 + 4 + 1), 60 tracks with one, 7 groups x TY3 on the pincell
CASES = {"square-eig": ("square", 3, "TY3", "eig"), "square-fix": ("square", 3, "TY3", "fix"), "square-adjoint": ("square", 3, "TY3", "adjoint"),
         "square-albedo": ("square_vacuum", 3, "TY3", "albedo"), "tiny-eig": ("tiny", 1, "TY1", "eig"), "tiny-fix": ("tiny", 1, "TY1", "fix"),
         "pin-eig": ("pin", 7, "TY3", "eig")}

_PROBLEMS, _RUNS = {}, {}


def problem(rt, oracle_run, name):
    """(TrackGenerator, the oracle's records, material per cell)."""
    if name not in _PROBLEMS:
        vac = _bcs(rt, "vacuum")
        if name == "square":
            tg = _traced(rt.TrackGenerator(square_model(rt), 8, 0.05, bcs=_bcs(rt, "mixed")), rt)
        elif name == "square_vacuum":
            tg = _traced(rt.TrackGenerator(square_model(rt), 8, 0.05, bcs=vac), rt)
        elif name == "tiny":
            tg = _traced(rt.TrackGenerator(make_grid_model(rt, 2, 2, hx=1.0, hy=1.0, flip=True), 4, 0.1, bcs=vac), rt)
        else:
            tg = _traced(rt.TrackGenerator(rt.DiscreteModelFromFile(rt.data_path("pincell.json")), 8, 0.05, bcs=_bcs(rt, "mixed")), rt)
        cm = _cell_material_array(tg, _materials(tg)) if name == "pin" else np.asarray(_bands(tg), np.int64)
        _PROBLEMS[name] = (tg, oracle_run(tg), cm)
        if name in ("square", "square_vacuum"):
            assert tg.mesh.num_cells == 288 and tg.n_total_tracks == 316
        if name == "tiny":
            assert tg.n_total_tracks == 60
    return _PROBLEMS[name]


def source(cm, G):
    return np.where(cm[:, None] == cm.max(), 1.0, 0.0) * np.linspace(1.0, 0.5, G)[None, :]


def case_xs(rt, case):
    _, G, _, mode = CASES[case]
    return _xs(rt, G, 70 + G)


def twin(rt, oracle_run, case, single):
    """The step twin of a case, built and not run (a BoundaryTwin around it for the albedo case)."""
    name, G, polar, mode = CASES[case]
    tg, rec, cm = problem(rt, oracle_run, name)
    xs = case_xs(rt, case)
    tw = moc_ref_f32.make_twin(rt, tg, rec, adjoint_xs(rt, xs) if mode == "adjoint" else xs, cm, polar, single=single)
    if mode == "albedo":
        tw = moc_ref_bc.BoundaryTwin(tw, rt.track_end_sides(tg), BETA4[:, :G])
    return tw


def twin_run(rt, oracle_run, case, single):
    """N iterations of the case's twin (cached): moc_ref.Twin.result, with current_out / current_in for the albedo case."""
    key = (case, bool(single))
    if key not in _RUNS:
        name, G, _, mode = CASES[case]
        _, _, cm = problem(rt, oracle_run, name)
        tw = twin(rt, oracle_run, case, single)
        fix = mode == "fix"
        _RUNS[key] = moc_ref.run(tw, "fixed" if fix else "eigenvalue", source(cm, G) if fix else None, N, 0.0, 0.0)
    return _RUNS[key]


def deviations(r, ref):
    """dict k, phi (of the median φ) and — where both carry the currents — J (of the largest J) of a result against a twin's."""
    med = float(np.median(np.abs(ref["phi"])))
    d = dict(k=float(np.abs(np.asarray(r["k_history"]) / ref["k_history"] - 1.0).max()), phi=float(np.abs(r["phi"] - ref["phi"]).max()) / med)
    if "current_out" in ref and "current_out" in r:
        top = max(float(np.abs(ref["current_out"]).max()), float(np.abs(ref["current_in"]).max()))
        d["J"] = max(float(np.abs(r["current_out"] - ref["current_out"]).max()), float(np.abs(r["current_in"] - ref["current_in"]).max())) / top
    return d


def e_ref(rt, oracle_run, cases=tuple(CASES)):
    """E_ref: the largest deviation of TwinF32 from Twin over `cases`, per quantity; and the per-case figures."""
    per = {c: deviations(twin_run(rt, oracle_run, c, True), twin_run(rt, oracle_run, c, False)) for c in cases}
    pooled = {q: max(d.get(q, 0.0) for d in per.values()) for q in ("k", "phi", "J")}
    return pooled, per
