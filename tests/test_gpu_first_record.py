"""Every track's first record (GPU only): the one generic step each lane of k_march takes before its cheap steps — locate from
scratch (nearest node, incident cells, and the k-nearest fallback when the nearest node's cells do not hold the point), three
edge intersections, entry into the walk / cheap state — at the smallest batches that reach each of its branches.  Records,
counts, status and volumes are the checker's (oracle/oracle.py), bit for bit where the suite compares bits (volumes: 1e-10);
whole tracks with cheap steps ("split" 0: the kernel of the headline configuration), the default plan (batches this small
march in pieces: the SPLIT instantiations share the locate) and both again with "topo" 0, the march without cheap steps."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("px", "py", "qx", "qy", "ell")
OPTION_SETS = (dict(split=0), dict(), dict(split=0, topo=0), dict(topo=0))


def _tracks(rt, model, px, py, phi):
    """Hand-made tracks from p on the boundary at angle ϕ to the opposite boundary, with the fields trace! fills
    (src/trackgenerator.jl:179-273); the quadrature's weights are those of a 4-angle trace of the same box."""
    from raytracing_jl_amd.trackgenerator import _general_form

    tg = rt.TrackGenerator(model, 4, 0.5)  # (the cases' meshes fill the unit square)
    rt.trace(tg)
    x0, y0, x1, y1 = tg.mesh.bb
    px, py, phi = (np.asarray(v, dtype=np.float64) for v in (px, py, phi))
    cs, sn = np.cos(phi), np.sin(phi)
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.where(cs > 0, (x1 - px) / cs, np.where(cs < 0, (x0 - px) / cs, np.inf))
        ty = (y1 - py) / sn
    t = np.minimum(tx, ty)
    qx, qy = px + t * cs, py + t * sn
    qx = np.where(tx <= ty, np.where(cs > 0, x1, x0), np.clip(qx, x0, x1))
    qy = np.where(tx <= ty, np.clip(qy, y0, y1), y1)
    A, B, C = _general_form(px, py, qx, qy)
    n = len(px)
    return SimpleNamespace(mesh=tg.mesh, px=px, py=py, phi=phi, cos_phi=cs, sin_phi=sn, A=A, B=B, C=C,
                           ell=np.hypot(px - qx, py - qy), azim_idx=np.ones(n, np.int32), tiny_step=tg.tiny_step,
                           azimuthal_quadrature=tg.azimuthal_quadrature, n_total_tracks=n)


def _head(tg, n):
    """The first n tracks of a traced generator."""
    assert n <= tg.n_total_tracks
    f = lambda a: np.ascontiguousarray(a[:n])
    return SimpleNamespace(mesh=tg.mesh, px=f(tg.px), py=f(tg.py), phi=f(tg.phi), cos_phi=f(tg.cos_phi), sin_phi=f(tg.sin_phi),
                           A=f(tg.A), B=f(tg.B), C=f(tg.C), ell=f(tg.ell), azim_idx=f(tg.azim_idx), tiny_step=tg.tiny_step,
                           azimuthal_quadrature=tg.azimuthal_quadrature, n_total_tracks=n)


def _corner_cutters(rt):
    """Tracks across the four corners of a jittered lattice, ε from the corner on both sides: ε of a few tiny_step — the whole
    track lies in the boundary band, it ends inside the start band —, ε inside the corner cell — its first record is its
    only one —, and larger ones."""
    import meshgen

    model = meshgen.lattice_model(rt, 7, 6, 6)
    px, py, phi = [], [], []
    for eps in (1.5e-9, 6e-9, 3e-8, 1e-6, 1e-4, 1e-2, 0.08, 0.3):
        px += [eps, 1.0 - eps, 0.0, 1.0]
        py += [0.0, 0.0, 1.0 - eps, 1.0 - eps]
        phi += [0.75 * math.pi, 0.25 * math.pi, 0.25 * math.pi, 0.75 * math.pi]
    return _tracks(rt, model, px, py, phi)


def _near_boundary_nodes(rt):
    """Start points within 1e-4 … 1e-9 edge lengths of a boundary node, on either side of it and on it, at five angles."""
    import meshgen

    model = meshgen.lattice_model(rt, 11, 5, 5)
    h = 1.0 / 5
    px, py, phi = [], [], []
    for j in range(1, 5):
        for d in (0.0, 1e-4, -1e-4, 1e-6, -1e-6, 1e-9, -1e-9):
            for a in (0.2, 0.35, 0.45, 0.65, 0.8):
                px.append(j * h + d * h); py.append(0.0); phi.append(a * math.pi)
    return _tracks(rt, model, px, py, phi)


def _vertex_touch(rt):
    """Right-triangle grid, tracks from boundary nodes along the diagonals and at atan 2 and atan 1/2: the first step runs along
    an edge or through a vertex (n_int ∈ {1, 3}, parallel edges)."""
    from conftest import make_grid_model

    model = make_grid_model(rt, 4, 4, hx=0.25, hy=0.25, flip=True)
    px, py, phi = [], [], []
    for j in range(0, 4):
        for a in (math.atan2(1, 1), math.atan2(2, 1), math.atan2(1, 2), math.pi - math.atan2(1, 1), math.pi - math.atan2(2, 1)):
            px.append(j * 0.25 if a < 0.5 * math.pi else (j + 1) * 0.25); py.append(0.0); phi.append(a)
    return _tracks(rt, model, px, py, phi)


def _traced(rt, model, n_azim, delta):
    tg = rt.TrackGenerator(model, n_azim, delta)
    rt.trace(tg)
    return tg


def _obtuse_boundary(rt):
    """Four boundary nodes per side and 150 random interior ones: long obtuse cells on the boundary, inside which a start point's
    nearest node is no vertex of its cell — the k-nearest fallback of find_element decides the first record."""
    import meshgen

    return _traced(rt, meshgen.random_model(rt, 5, 150, nb=4), 8, 0.01)


def _lattice(rt):
    import meshgen

    return _traced(rt, meshgen.lattice_model(rt, 3, 9, 9), 8, 0.01)


CASES = {
    "corner_cutters": _corner_cutters,
    "near_boundary_nodes": _near_boundary_nodes,
    "vertex_touch": _vertex_touch,
    "obtuse_boundary": _obtuse_boundary,
    "partial_wave_65": lambda rt: _head(_lattice(rt), 65),
    "partial_wave_63": lambda rt: _head(_lattice(rt), 63),
    "pieces_300": lambda rt: _head(_lattice(rt), 300),
}

_REF = {}


def _case(rt, orc, name):
    """The case's tracks and the checker's result, computed once per session and left unchanged."""
    if name not in _REF:
        tg = CASES[name](rt)
        om = orc.OracleMesh.from_mesh(tg.mesh, omp=True)
        r = om.segmentize(tg.px, tg.py, tg.phi, tg.A, tg.B, tg.C, tg.ell, cos_phi=tg.cos_phi, sin_phi=tg.sin_phi,
                          tiny_step=tg.tiny_step, iter_cap=4000000, n_threads=0)
        aq = tg.azimuthal_quadrature
        r["volumes"] = om.fill_volumes(r["offsets"], tg.azim_idx, aq.delta_s, aq.n_azim_2)
        _REF[name] = (tg, r)
    return _REF[name]


def _needs_fallback(tg, ref):
    """Tracks whose first record lies in a cell that has the start point's nearest node not among its vertices."""
    xy = np.column_stack((tg.mesh.x, tg.mesh.y))
    cells = np.asarray(tg.mesh.cell_nodes)
    cnt = np.diff(ref["offsets"])
    has = np.flatnonzero(cnt > 0)
    sx, sy = tg.px[has] + 3 * tg.tiny_step * tg.cos_phi[has], tg.py[has] + 3 * tg.tiny_step * tg.sin_phi[has]
    nn = np.argmin((sx[:, None] - xy[None, :, 0]) ** 2 + (sy[:, None] - xy[None, :, 1]) ** 2, axis=1) + 1
    first = ref["element"][ref["offsets"][has]] - 1
    return int(np.count_nonzero(~np.any(cells[first] == nn[:, None], axis=1)))


def _run(rt, tg, opts):
    from raytracing_jl_amd import _capi

    dm = _capi.DeviceMesh(tg.mesh, 0)
    for k, v in opts.items():
        dm.set_option(k, v)
    dt = _capi.DeviceTracks(dm, tg.px, tg.py, tg.phi, tg.cos_phi, tg.sin_phi, tg.A, tg.B, tg.C, tg.ell, tg.azim_idx)
    aq = tg.azimuthal_quadrature
    total = dt.segmentize(tg.tiny_step, 5, rt.RTOL_DEFAULT, aq.delta_s, aq.n_azim_2)
    off, st = dt.fetch_offsets()
    seg = dt.fetch_segments()
    vol = dt.fetch_volumes()
    dt.close(); dm.close()
    return total, off, st, seg, vol


def test_cases_reach_their_branches(rt, orc):
    """What the cases are for, read off the checker's results (no device work): tracks without a record, tracks with one
    record, first locates that need the fallback, batches of one wave and a lane more or less, fewer than 160 waves."""
    tg, ref = _case(rt, orc, "corner_cutters")
    cnt = np.diff(ref["offsets"])
    assert np.count_nonzero(cnt == 0) >= 4 and np.count_nonzero(cnt == 1) >= 4 and cnt.max() > 2, cnt
    tg, ref = _case(rt, orc, "obtuse_boundary")
    assert _needs_fallback(tg, ref) >= 3
    tg, ref = _case(rt, orc, "vertex_touch")
    assert np.count_nonzero(ref["status"]) < tg.n_total_tracks  # (the reference fails some of these tracks: compared as they are)
    assert _case(rt, orc, "partial_wave_65")[0].n_total_tracks == 65 and _case(rt, orc, "partial_wave_63")[0].n_total_tracks == 63
    assert 64 < _case(rt, orc, "pieces_300")[0].n_total_tracks < 160 * 64


@pytest.mark.parametrize("name", list(CASES))
def test_first_record_matches_the_checker(rt, orc, name):
    tg, ref = _case(rt, orc, name)
    runs = {}
    for opts in OPTION_SETS:
        total, off, st, seg, vol = runs[tuple(opts.items())] = _run(rt, tg, opts)
        assert total == ref["total"], opts
        assert np.array_equal(st, ref["status"]), ("per-track status differs", opts)
        assert np.array_equal(off, ref["offsets"]), ("segment counts differ", opts)
        assert np.array_equal(seg["element"], ref["element"]), ("element ids differ", opts)
        for k in FIELDS:
            assert np.array_equal(seg[k], ref[k]), (k, opts)
        assert np.allclose(vol, ref["volumes"], rtol=1e-10, atol=1e-300), opts
    # the default options against the march without cheap steps, directly
    for a, b in (((), (("topo", 0),)), ((("split", 0),), (("split", 0), ("topo", 0)))):
        ra, rb = runs[a], runs[b]
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
        for k in FIELDS + ("element",):
            assert np.array_equal(ra[3][k], rb[3][k]), k
        assert np.allclose(ra[4], rb[4], rtol=1e-10, atol=1e-300)
    cnt = np.diff(ref["offsets"])
    print(f"{name}: {tg.n_total_tracks} tracks, {int(ref['total'])} records, {int(np.count_nonzero(cnt == 0))} tracks without a record, "
          f"{int(np.count_nonzero(cnt == 1))} with one, {int(np.count_nonzero(ref['status']))} failed by the reference")
