"""CPU side of the collision-detector tests on synthesised geometry: the reference (tests/detector_ref.py) against what is already pinned, the host
build of the device geometry (stark_amd/csrc/contact_geom.hpp through tests/host_elem/host_elem.cpp) against the exact predicates on the
atlases, and the conditions the builders of tests/detector_cases.py promise to the GPU tests (tests/test_gpu_detector_synth.py)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import contact as oc  # noqa: E402
from oracle import evaluator as ev  # noqa: E402
from contact_util import state_from_fixture  # noqa: E402
import detector_cases as dc  # noqa: E402
import detector_ref as dr  # noqa: E402
from test_gpu_contact import _oracle_lists  # noqa: E402  (oracle detect() -> rows of mistark_tmcd.h, the mapping the device lists are compared with)


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_geom_"), "host_elem.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host_elem", "host_elem.cpp"), "-o", out], check=True)
    return ctypes.CDLL(out)


@pytest.mark.parametrize("name", ["contactmix_t0", "contactrods_t0"])
def test_reference_equals_the_pinned_oracle_on_recorded_scenes(name):
    """detector_ref.proximity against oracle.contact.detect, which tests/test_oracle_contact.py ties to the reference's tables: the same six lists
    (nothing undecidable in these scenes may hide a difference: the undecidable pairs are removed from both sides and counted)."""
    prob, man, z = ev.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    st, _ = state_from_fixture(prob, man)
    scene = oc.scene_from_fixture(man, z)
    dt = float(np.asarray(st["dt"]).ravel()[0])
    X = [np.ascontiguousarray(x, dtype=np.float64) for x in oc.mesh_vertices(scene, st, dt)]
    enl = 2.0 * oc.max_thickness(scene)
    sc = dr.Scene([(x, m.tris, m.edges) for m, x in zip(scene.meshes, X)])
    for a, b in scene.disabled:
        sc.blacklist(a, b)
    ref = dr.proximity(sc, enl)
    want, _ = _oracle_lists(oc.detect(scene, X, enl))
    assert ref.n_hits > 10
    n_und = 0
    for l, lname in enumerate(dr.LISTS):
        w = np.array(want[lname], dtype=np.int64).reshape(-1, dr.COLS[l])
        und = ref.und_pt if lname.startswith("pt_") else ref.und_ee
        keep, _ = dr.without(w, dr.row_keys(w, lname), und)
        n_und += len(w) - len(keep)
        keep, _ = dr.sorted_rows(keep)
        assert keep.shape == ref.rows[lname].shape and (keep == ref.rows[lname]).all(), lname
    print("%s: %d hits, %d oracle rows left out as undecidable" % (name, ref.n_hits, n_und))
    assert n_und <= dr.undecidable_cap(ref.n_hits)


def _host_pt(lib, rows):
    inp = np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(-1, 12))
    ty, d2 = np.zeros(len(inp), dtype=np.int32), np.zeros(len(inp))
    lib.host_geom_point_triangle(ctypes.c_void_p(inp.ctypes.data), len(inp), ctypes.c_void_p(ty.ctypes.data), ctypes.c_void_p(d2.ctypes.data))
    return ty, d2


def _host_ee(lib, rows):
    inp = np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(-1, 12))
    ty, d2 = np.zeros(len(inp), dtype=np.int32), np.zeros(len(inp))
    lib.host_geom_edge_edge(ctypes.c_void_p(inp.ctypes.data), len(inp), ctypes.c_void_p(ty.ctypes.data), ctypes.c_void_p(d2.ctypes.data))
    return ty, d2


def test_host_build_of_the_device_geometry_decides_the_point_triangle_atlas_exactly(host_lib):
    """every (query point, triangle) pair of atlas a.: contact_geom.hpp compiled for the host gives the type of the rational predicate and its d^2
    (correctly rounded where it is no double); all seven types and the ties along == 0, along == 1, across == 0, d^2 == enl^2 occur."""
    scene, info = dc.pt_atlas()
    Q = scene.meshes[info["query_mesh"]][0]
    rows, want_ty, want_d2, ties = [], [], [], set()
    for g in range(12):
        T = scene.meshes[g][0]
        for q in Q:
            ty, d2, _ = dr.point_triangle_exact(q, T[0], T[1], T[2], ties=ties)
            rows.append(np.concatenate([q, T[0], T[1], T[2]]))
            want_ty.append(ty)
            want_d2.append(float(d2))
    ty, d2 = _host_pt(host_lib, rows)
    assert (ty == np.array(want_ty)).all()
    assert (d2 == np.array(want_d2)).all()
    assert set(want_ty) == set(range(7))
    assert {"along==0", "along==1", "across==0"} <= ties
    ref = dr.proximity(scene, info["enl"], exact_inputs=True)
    present = set(sum((dr.pt_key(ref.rows[n]) for n in dr.LISTS[:3]), []))
    qm = info["query_mesh"]
    assert all((qm, i, g, 0) not in present for i, g in info["tie_absent"]) and all((qm, i, g, 0) in present for i, g in info["tie_present"])
    assert all(len(ref.rows[n]) > 0 for n in dr.LISTS[:3])
    # every closest vertex / edge of the lists occurs: the seven types, seen through the rows
    assert {tuple(r[4:7]).index(r[7]) for r in ref.rows["pt_point_point"].tolist()} == {0, 1, 2}
    assert {tuple(r[4:7]).index(r[7]) for r in ref.rows["pt_point_edge"].tolist()} == {0, 1, 2}


def test_host_build_of_the_device_geometry_decides_the_edge_edge_atlas_exactly(host_lib):
    """every edge pair of atlas b. that the parallel cutoff lets through: type and d^2 as above; all nine types and the eight named ties occur,
    in both role orders; exactly parallel pairs exist and reach no list."""
    scene, info = dc.ee_atlas()
    g = scene.flat()
    rows, want_ty, want_d2, ties, n_parallel = [], [], [], set(), 0
    ne = len(g["E"])
    for a in range(ne):
        for b in range(a + 1, ne):
            if g["em"][a] == g["em"][b] and g["em"][a] != 1:
                continue   # (pairs inside the two grids of second edges are left to the list comparison)
            pair_ties = set()
            ty, d2, _ = dr.edge_edge_exact(g["E"][a, 0], g["E"][a, 1], g["E"][b, 0], g["E"][b, 1], ties=pair_ties)
            if ty is None:
                n_parallel += 1
                continue
            ties |= {(t, bool(g["em"][a] < 1 or g["em"][b] < 1)) for t in pair_ties}
            rows.append(np.concatenate([g["E"][a, 0], g["E"][a, 1], g["E"][b, 0], g["E"][b, 1]]))
            want_ty.append(ty)
            want_d2.append(float(d2))
    ty, d2 = _host_ee(host_lib, rows)
    assert (ty == np.array(want_ty)).all()
    assert (d2 == np.array(want_d2)).all()
    assert n_parallel > 10
    ref = dr.proximity(scene, info["enl"], exact_inputs=True)
    # the types that reach a list (within enl), by role order: the first edge's mesh is 1, second edges live in meshes 0 (registered before) and 2
    names = ("sN==0", "sN==D", "tN==0", "tN==tD", "-d==0", "-d==a", "-d+b==0", "-d+b==a")
    assert {t for t, _ in ties} >= set(names), set(names) - {t for t, _ in ties}
    for order in (True, False):
        assert {t for t, o in ties if o == order} >= set(names), (order, set(names) - {t for t, o in ties if o == order})
    listed = set()
    for a, b, t in _listed_types(scene, ref):
        listed.add((t, a[0] < 1 or b[0] < 1))
    for order in (True, False):
        assert {t for t, o in listed if o == order} == set(range(9)), order
    keys = set(sum((dr.ee_key(ref.rows[n], n) for n in dr.LISTS[3:]), []))
    assert info["tie_absent"][0] + info["tie_absent"][1] not in keys and info["tie_present"][0] + info["tie_present"][1] in keys
    assert info["shared"][0] + info["shared"][1] not in keys


def _listed_types(scene, ref):
    """(edge a, edge b, type) of every listed edge pair, recomputed exactly (a = the lower global edge)"""
    X = scene.X()
    for n in dr.LISTS[3:]:
        for k in dr.ee_key(ref.rows[n], n):
            a, b = (k[0], k[1]), (k[2], k[3])
            ea, eb = scene.meshes[a[0]][2][a[1]], scene.meshes[b[0]][2][b[1]]
            ty, _, _ = dr.edge_edge_exact(X[a[0]][ea[0]], X[a[0]][ea[1]], X[b[0]][eb[0]], X[b[0]][eb[1]])
            yield a, b, ty


def test_host_build_of_the_device_geometry_decides_the_intersection_atlas_exactly(host_lib):
    scene, info = dc.et_atlas()
    g = scene.flat()
    rows, want = [], []
    for e in range(len(g["E"])):
        for t in range(len(g["T"])):
            hit, _, _ = dr.edge_triangle_exact(g["E"][e, 0], g["E"][e, 1], g["T"][t, 0], g["T"][t, 1], g["T"][t, 2])
            rows.append(np.concatenate([g["E"][e, 0], g["E"][e, 1], g["T"][t, 0], g["T"][t, 1], g["T"][t, 2]]))
            want.append(int(hit))
    inp = np.ascontiguousarray(np.array(rows))
    hit = np.zeros(len(inp), dtype=np.int32)
    host_lib.host_geom_edge_triangle(ctypes.c_void_p(inp.ctypes.data), len(inp), ctypes.c_void_p(hit.ctypes.data))
    assert (hit == np.array(want)).all()
    ref, und = dr.intersections(scene, exact_inputs=True)
    n = info["n_probes"]
    expect = {(1, k, 0, k // n) for k, lab in enumerate(info["labels"]) if lab not in ("short", "outside", "coplanar")}
    assert set(dr.et_key(ref)) == expect          # (the own-mesh edge at a shared vertex and the blacklisted mesh are absent)
    ref0, _ = dr.intersections(dc.et_atlas(signed_zeros=True)[0], exact_inputs=True)
    assert (ref0 == ref).all()


def test_cutoff_pairs_lie_on_either_side():
    for sc, kept in dc.ee_cutoff_scenes():
        ref = dr.proximity(sc, dc.ATLAS_ENL, exact_inputs=True)
        assert ref.n_hits == (1 if kept else 0)


def restatement_error(scene, ref):
    """largest |d_numpy - d_exact| over ALL of the reference's hits, in units of 2^-53 L (L = the pair's largest coordinate difference): the float64
    restatement of oracle/contact.py against the exact value, same inputs"""
    X = scene.X()
    worst = 0.0
    for n in dr.LISTS:
        rows = ref.rows[n]
        if len(rows) == 0:
            continue

        def pos(mesh_col, vert_col):
            return np.array([X[m][v] for m, v in zip(rows[:, mesh_col].tolist(), rows[:, vert_col].tolist())])

        if n.startswith("pt_"):
            _, d2 = oc.point_triangle_sq_distance(pos(0, 1), pos(2, 4), pos(2, 5), pos(2, 6))
        else:
            j = 4 if n == "ee_edge_edge" else 5
            first = [pos(0, 2), pos(0, 3)]
            second = [pos(j, j + 2), pos(j, j + 3)]
            # the restatement wants the lower global edge as edge a (rows list the edges by role)
            swap = (rows[:, 0] > rows[:, j]) | ((rows[:, 0] == rows[:, j]) & (rows[:, 1] > rows[:, j + 1]))
            a0, a1 = np.where(swap[:, None], second[0], first[0]), np.where(swap[:, None], second[1], first[1])
            b0, b1 = np.where(swap[:, None], first[0], second[0]), np.where(swap[:, None], first[1], second[1])
            _, d2 = oc.edge_edge_sq_distance(a0, a1, b0, b1)
        worst = max(worst, float((np.abs(np.sqrt(d2) - ref.dist[n]) / (2.0 ** -53 * ref.span[n])).max()))
    return worst


def test_random_scenes_keep_the_builders_promises():
    """counts, strip lengths, the undecidable cap of every random case of d., and the distance-tolerance measurement: the float64 restatement
    stays within 32 * 2^-53 * L of the exact distance (printed; measured over every hit: 1.6 x 2^-53 L on d.1, 5.2 on d.1 pushed, 1.1 on d.5, 2.4 on d.6; no undecidable pair in any case)."""
    scene, normal = dc.two_grids()
    nv, nt, ne = scene.counts()
    assert (nv, nt, ne) == (1152, 2116, 3266) and all(c % 256 for c in (nv, nt, ne))
    ref = dr.proximity(scene, dc.ENL)
    assert ref.n_hits > 2000 and len(ref.und_pt) + len(ref.und_ee) <= dr.undecidable_cap(ref.n_hits)
    assert all(len(ref.rows[n]) > 0 for n in dr.LISTS)
    hits, und = dr.intersections(scene)
    assert len(hits) == 0 and len(und) == 0
    worst = restatement_error(scene, ref)
    print("d.1: %d hits, %d undecidable, float64 restatement error %.2f x 2^-53 L" % (ref.n_hits, len(ref.und_pt) + len(ref.und_ee), worst))
    assert worst <= dr.DIST_ROUNDINGS
    scene.meshes[1][0][:] -= 0.72 * dc.ENL * normal
    ref2 = dr.proximity(scene, dc.ENL)
    hits, und = dr.intersections(scene)
    print("d.1 pushed: %d hits, %d undecidable, %d intersections, %d undecidable" % (ref2.n_hits, len(ref2.und_pt) + len(ref2.und_ee), len(hits), len(und)))
    assert len(hits) > 100 and len(und) <= dr.undecidable_cap(len(hits))
    assert len(ref2.und_pt) + len(ref2.und_ee) <= dr.undecidable_cap(ref2.n_hits)
    worst = restatement_error(scene, ref2)
    print("d.1 pushed: float64 restatement error %.2f x 2^-53 L" % worst)
    assert worst <= dr.DIST_ROUNDINGS
    # d.5
    far, _ = dc.two_grids(n=12, shift=(1000.0, -2000.0, 500.0))
    ref = dr.proximity(far, dc.ENL)
    worst = restatement_error(far, ref)
    print("d.5: %d hits, %d undecidable, float64 restatement error %.2f x 2^-53 L" % (ref.n_hits, len(ref.und_pt) + len(ref.und_ee), worst))
    assert ref.n_hits > 500 and len(ref.und_pt) + len(ref.und_ee) <= dr.undecidable_cap(ref.n_hits)
    # d.6
    sc = dc.stacked_patches()
    ref = dr.proximity(sc, dc.ENL)
    n_pairs = 40 * 39 // 2
    n_black = sum(1 for a, b in sc.disabled if a < b)
    assert abs(n_black - n_pairs / 3) < 0.2 * n_pairs / 3 and any(a == b for a, b in sc.disabled)
    assert ref.n_hits > 1000 and len(ref.und_pt) + len(ref.und_ee) <= dr.undecidable_cap(ref.n_hits)
    worst = restatement_error(sc, ref)
    print("d.6: %d hits, float64 restatement error %.2f x 2^-53 L" % (ref.n_hits, worst))
    assert worst <= dr.DIST_ROUNDINGS
    free = dr.Scene(sc.meshes)
    free.disabled = set(sc.disabled)
    assert dr.proximity(free, dc.ENL).n_hits > ref.n_hits      # the range blacklists remove pairs that exist


def test_lattice_grids_hold_massive_ties():
    sc, enl = dc.lattice_grids()
    assert sc.counts() == (1152, 2116, 3266)
    ref = dr.proximity(sc, enl, exact_inputs=True)
    assert ref.n_hits > 2000
    lo = np.concatenate([m[0] for m in sc.meshes])
    assert len(np.unique(lo[:, 0])) == 24   # whole columns of boxes share one lower bound
    dc.lattice_push(sc)
    hits, _ = dr.intersections(sc, exact_inputs=True)
    assert len(hits) > 100


@pytest.mark.parametrize("n", dc.STRIP_LENGTHS)
def test_strips_are_one_range_of_n_pairs(n):
    assert dc.STRIP_LENGTHS == (511, 512, 513, 1543)
    sc = dc.strip_points(n)
    ref = dr.proximity(sc, dc.ENL)
    assert ref.n_hits == n and not ref.und_pt                      # the brute force is n pairs, all hits
    for k in (1, 2):   # the spread in the two other axes stays below enl
        allv = np.concatenate([m[0][:, k] for m in sc.meshes])
        assert allv.max() - allv.min() < dc.ENL
    sc = dc.strip_edges(n)
    ref = dr.proximity(sc, dc.ENL)
    assert ref.n_hits == n and not ref.und_ee
    for k in (1, 2):
        allv = np.concatenate([m[0][:, k] for m in sc.meshes])
        assert allv.max() - allv.min() < dc.ENL
    sc = dc.strip_triangles(n)
    hits, und = dr.intersections(sc)
    assert len(hits) == n and not und
    T = sc.meshes[1][0].reshape(n, 3, 3)
    assert (T[:, :, 1].min(axis=1) == T[0, :, 1].min()).all()      # one first band for all triangles


def test_rods():
    for kind in ("skew", "axis"):
        sc = dc.rods(kind)
        assert sc.counts() == (802, 0, 800)
        ref = dr.proximity(sc, dc.ENL)
        assert not ref.und_ee
        X = np.concatenate(sc.X())
        if kind == "axis":
            assert ref.n_hits == 0 and np.ptp(X[:, 1]) == 0 and np.ptp(X[:, 2]) == 0
            assert 64 * (802 + 800) > (802 + 800) * 3 // 2 + 4096    # every box in every band outgrows the band list's first capacity
            assert len(dr.broad_phase(sc, dc.ENL)[1]) > 800
        else:
            assert 0 < ref.n_hits < 100
