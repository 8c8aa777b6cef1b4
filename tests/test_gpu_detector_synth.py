"""The standalone collision detector (include/mistark_tmcd.h through capi.CollisionDetector: the sweep kernels of the engine's contact update)
on synthesised geometry and exact ties, against tests/detector_ref.py: exact rational predicates and brute force over all pairs.

Common to every test (detector_ref.check_proximity / check_intersections / check_broad_phase): row sets equal apart from the undecidable
pairs, no duplicate rows, no pair in two lists, counts equal the list lengths, distances within 32 * 2^-53 * L of the exact distance (L = the
largest coordinate difference among the pair's vertices; the float64 numpy restatement measured against the exact value on the same inputs,
tests/test_detector_ref_cpu.py, over every hit: 1.6 x 2^-53 L on scene d.1, 5.2 once its grids are pushed through each other, 1.1 far from
the origin, 2.4 on the stacked patches, so the bound of 32 roundings stands and no measured value replaces it). UNDECIDABLE CAP: at most 0.1 % of the reference's hits in a case and never more than 5
(detector_ref.undecidable_cap), asserted here and for the reference alone in the CPU module; the atlases and the lattice grids run with
exact inputs, where nothing is undecidable and every tie is a decision to reproduce.

Sweep paths the cases reach are listed in DESIGN.md ("Detector tests on synthesised geometry")."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detector_cases as dc  # noqa: E402
import detector_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu


def detector(scene):
    from stark_amd import capi
    return scene.register(capi.CollisionDetector())


def capped(ref):
    n = len(ref.und_pt) + len(ref.und_ee)
    assert n <= dr.undecidable_cap(ref.n_hits), (n, ref.n_hits)


_GRIDS = {}


def grids_reference():
    """scene d.1 at its first positions: (proximity lists, broad-phase listing) of the reference, computed once for the tests that share it"""
    if not _GRIDS:
        scene, _ = dc.two_grids()
        _GRIDS["ref"] = (dr.proximity(scene, dc.ENL), dr.broad_phase(scene, dc.ENL))
    return _GRIDS["ref"]


def check_all(cd, scene, enl, exact_inputs=False, broad=True, intersections=True, known=None):
    """proximity, broad-phase listing and intersections of the detector at the scene's current positions against the reference"""
    ref = known[0] if known else dr.proximity(scene, enl, exact_inputs=exact_inputs)
    capped(ref)
    worst = dr.check_proximity(cd.run_proximity(enl), ref)
    hits = None
    if broad:
        dr.check_broad_phase(cd.run_broad_phase(enl), known[1] if known else dr.broad_phase(scene, enl))
    if intersections:
        hits, und = dr.intersections(scene, exact_inputs=exact_inputs)
        assert len(und) <= dr.undecidable_cap(len(hits))
        dr.check_intersections(cd.run_intersection(), hits, und)
    return ref, hits, worst


def test_point_triangle_atlas_on_exact_ties():
    """a. One triangle in all six vertex orders and mirrored (12 meshes) against a vertex-only mesh of query points on the 2^-8 lattice: above the
    interior, the edges, exactly on across == 0, along == 0, along == 1, above the vertices, in the plane inside and outside, at distance exactly
    enl (absent: d2 < enl2 is strict) and one lattice step closer (present). Every product is exact in double: nothing is undecidable."""
    scene, info = dc.pt_atlas()
    cd = detector(scene)
    got = cd.run_proximity(info["enl"])
    ref = dr.proximity(scene, info["enl"], exact_inputs=True)
    dr.check_proximity(got, ref)
    present = set(sum((dr.pt_key(got[n][0]) for n in dr.LISTS[:3]), []))
    qm = info["query_mesh"]
    assert all((qm, i, g, 0) not in present for i, g in info["tie_absent"])
    assert all((qm, i, g, 0) in present for i, g in info["tie_present"])
    # all seven types: every closest vertex, every closest edge, and the face
    assert {tuple(r[4:7]).index(r[7]) for r in got["pt_point_point"][0].tolist()} == {0, 1, 2}
    assert {tuple(r[4:7]).index(r[7]) for r in got["pt_point_edge"][0].tolist()} == {0, 1, 2}
    assert len(got["pt_point_triangle"][0]) > 0
    assert all(len(got[n][0]) == 0 for n in dr.LISTS[3:])
    assert len(cd.run_intersection()) == 0     # (no edges)
    cd.close()


def test_edge_edge_atlas_on_exact_ties():
    """b. The lattice edge pairs of detector_cases.ee_atlas: all nine types, the ties sN == 0, sN == D, tN == 0, tN == tD, -d == 0, -d == a,
    -d + b == 0, -d + b == a in both role orders (tests/test_detector_ref_cpu.py asserts that they occur), distance exactly enl (absent) and
    one step inside (present), exactly parallel edges (in no list), edges of one mesh sharing a vertex (never a pair)."""
    scene, info = dc.ee_atlas()
    cd = detector(scene)
    got = cd.run_proximity(info["enl"])
    ref = dr.proximity(scene, info["enl"], exact_inputs=True)
    dr.check_proximity(got, ref)
    keys = set(sum((dr.ee_key(got[n][0], n) for n in dr.LISTS[3:]), []))
    assert info["tie_absent"][0] + info["tie_absent"][1] not in keys and info["tie_present"][0] + info["tie_present"][1] in keys
    assert info["shared"][0] + info["shared"][1] not in keys
    assert all(len(got[n][0]) > 0 for n in dr.LISTS[3:]) and all(len(got[n][0]) == 0 for n in dr.LISTS[:3])
    dr.check_broad_phase(cd.run_broad_phase(info["enl"]), dr.broad_phase(scene, info["enl"]))
    cd.close()


def test_edge_edge_parallel_cutoff():
    """b. |u x v|^2 = 2^-100 <= 1e-30: the pair reaches no list; 2^-98: it is in exactly one (which one is not asserted)."""
    for scene, kept in dc.ee_cutoff_scenes():
        cd = detector(scene)
        got = cd.run_proximity(dc.ATLAS_ENL)
        assert sum(len(got[n][0]) for n in dr.LISTS) == (1 if kept else 0)
        assert len(cd.run_broad_phase(dc.ATLAS_ENL)[1]) == 1      # (a candidate either way: the cutoff belongs to the narrow phase)
        cd.close()


@pytest.mark.parametrize("signed_zeros", [False, True])
def test_intersection_atlas(signed_zeros):
    """c. run_intersection as the FIRST call on a fresh detector; the whole 9-column row set against the reference: edges through the interior, through
    a triangle edge (u == 0, v == 0, u + v == 1), through a vertex, ending in the triangle (t == 0, t == 1), one lattice step short, coplanar
    (crossing or not: det == 0, absent), sharing a vertex with a triangle of their own mesh (absent), of a blacklisted mesh (absent). Second
    variant: the probing edges' zero coordinates are -0.0, the triangles' +0.0 (the box sort key orders signed zeros, comparisons do not)."""
    scene, info = dc.et_atlas(signed_zeros=signed_zeros)
    cd = detector(scene)
    got = cd.run_intersection()
    ref, und = dr.intersections(scene, exact_inputs=True)
    dr.check_intersections(got, ref, set())
    n = info["n_probes"]
    expect = {(1, k, 0, k // n) for k, lab in enumerate(info["labels"]) if lab not in ("short", "outside", "coplanar")}
    assert set(dr.et_key(got)) == expect
    # and the proximity lists of the same scene behind it
    dr.check_proximity(cd.run_proximity(dc.ATLAS_ENL), dr.proximity(scene, dc.ATLAS_ENL, exact_inputs=True))
    dr.check_intersections(cd.run_intersection(), ref, set())
    cd.close()


def test_two_jittered_grids_general_position():
    """d.1 Two jittered 24 x 24 grids 0.7 enl apart, rotated off the axes, coordinates of both signs; 1152 points, 2116 triangles, 3266 edges (no
    multiple of 256). Proximity, broad-phase listing (bit-exact against oracle.contact.broad_phase) and intersections (none); then one grid is
    pushed through the other IN PLACE: positions are read again, intersections appear."""
    scene, normal = dc.two_grids()
    assert scene.counts() == (1152, 2116, 3266)
    cd = detector(scene)
    ref, hits, worst = check_all(cd, scene, dc.ENL, known=grids_reference())
    assert ref.n_hits > 2000 and len(hits) == 0
    scene.meshes[1][0][:] -= 0.72 * dc.ENL * normal
    ref2, hits2, worst2 = check_all(cd, scene, dc.ENL)
    assert len(hits2) > 100 and ref2.n_hits != ref.n_hits
    print("distance error %.2f / %.2f x 2^-53 L" % (worst, worst2))
    cd.close()


def test_lattice_grids_massive_ties():
    """d.2 The same grids axis-aligned on the 2^-8 lattice, no jitter: whole columns of boxes share one lower bound on every axis (the [lo, hi] /
    (lo, hi] split of the sweep: a slip loses pairs or reports them twice), and the closest-feature decisions sit on ties throughout."""
    scene, enl = dc.lattice_grids()
    cd = detector(scene)
    hits, _ = dr.intersections(scene, exact_inputs=True)
    dr.check_intersections(cd.run_intersection(), hits, set())
    ref, _, _ = check_all(cd, scene, enl, exact_inputs=True, intersections=False)
    assert ref.n_hits > 2000
    # second state, in place: the second grid zigzags through the first one's plane, crossing it exactly over its vertices and edges
    dc.lattice_push(scene)
    hits, _ = dr.intersections(scene, exact_inputs=True)
    assert len(hits) > 100
    dr.check_intersections(cd.run_intersection(), hits, set())
    check_all(cd, scene, enl, exact_inputs=True, intersections=False)
    cd.close()


@pytest.mark.parametrize("n", dc.STRIP_LENGTHS)
def test_long_ranges(n):
    """d.3 One primitive over a strip of n others that is ONE range of its sweep entry, n = SWEEP_SPLIT - 1, SWEEP_SPLIT, SWEEP_SPLIT + 1,
    3 SWEEP_SPLIT + 7: a triangle over n points, an edge over n skew edges, an edge through n triangles (intersection sweep). n pairs each."""
    sc = dc.strip_points(n)
    cd = detector(sc)
    ref, _, _ = check_all(cd, sc, dc.ENL, intersections=False)
    assert ref.n_hits == n
    cd.close()
    sc = dc.strip_edges(n)
    cd = detector(sc)
    ref, _, _ = check_all(cd, sc, dc.ENL, intersections=False)
    assert ref.n_hits == n
    cd.close()
    sc = dc.strip_triangles(n)
    cd = detector(sc)
    hits, und = dr.intersections(sc)
    assert len(hits) == n and not und
    dr.check_intersections(cd.run_intersection(), hits, und)
    cd.close()


@pytest.mark.parametrize("kind", ["skew", "axis"])
def test_rods_flat_scene_and_band_list_growth(kind):
    """d.4 Two straight rods of 400 edges, edges only. "skew": on two skew lines 0.5 enl apart. "axis": every vertex on one line parallel to x: the
    band axis has extent 0 (clamped to 1e-12), every box lies in all 64 bands and the band list outgrows its first capacity; collinear edges are
    parallel, so the lists are empty while the broad-phase listing is not."""
    sc = dc.rods(kind)
    cd = detector(sc)
    ref, _, _ = check_all(cd, sc, dc.ENL, intersections=False)
    assert (ref.n_hits == 0) == (kind == "axis")
    assert len(cd.run_intersection()) == 0
    cd.close()


def test_single_vertex_only_mesh():
    """d.4 One mesh without triangles and edges: empty lists, no error."""
    sc = dr.Scene([(np.array([[0.0, 0.0, 0.0], [1e-4, 0.0, 0.0], [0.0, 2e-4, 0.0]]), np.zeros((0, 3)), np.zeros((0, 2)))])
    cd = detector(sc)
    got = cd.run_proximity(dc.ENL)
    assert all(got[n][0].shape == (0, dr.COLS[l]) for l, n in enumerate(dr.LISTS))
    assert len(cd.run_intersection()) == 0
    assert all(len(r) == 0 for r in cd.run_broad_phase(dc.ENL))
    cd.close()


def test_far_from_the_origin():
    """d.5 Scene d.1 at quarter size translated by (1000, -2000, 500): a float ulp there is 6e-5 to 1.2e-4 against enl = 1e-3, the boxes are coarse but
    rounded outwards: no pair of the brute force may be missing and the row sets are still equal; the listing equals oracle.contact.broad_phase."""
    scene, _ = dc.two_grids(n=12, shift=(1000.0, -2000.0, 500.0))
    cd = detector(scene)
    ref, hits, _ = check_all(cd, scene, dc.ENL)
    assert ref.n_hits > 500
    cd.close()


def test_many_meshes_and_blacklists():
    """d.6 40 stacked patches 0.6 enl apart, a third of the mesh pairs and some self pairs blacklisted, one point-triangle and one edge-edge range."""
    sc = dc.stacked_patches()
    cd = detector(sc)
    ref, _, _ = check_all(cd, sc, dc.ENL)
    assert ref.n_hits > 1000
    cd.close()


def test_other_states():
    """d.7 enlargement 0 (empty lists, no error); one family switched off (exactly its three lists empty, the others as the reference has them); a
    repeated run at unchanged positions (identical lists: the one comparison of the detector with itself); and one vertex moved by ONE ULP
    across the d == enl tie of atlas a.: the answer changes, the fingerprint cache must not serve the old lists. (That move leaves the lattice,
    but the decision stays exact: with the normal (0, 0, +-1/2) the distance is h^2 / |n|^2 = dz^2 up to powers of two, and dz^2 = enl^2 -
    2.5 * 2^-56 rounds to a double below enl^2 = 25 / 256, whose neighbours are 2^-56 apart.)"""
    scene, _ = dc.two_grids()
    cd = detector(scene)
    got = cd.run_proximity(0.0)
    assert all(len(got[n][0]) == 0 for n in dr.LISTS)
    ref, broad = grids_reference()
    capped(ref)
    first = cd.run_proximity(dc.ENL)
    dr.check_proximity(first, ref)
    again = cd.run_proximity(dc.ENL)
    for n in dr.LISTS:
        assert (first[n][0] == again[n][0]).all() and (first[n][1] == again[n][1]).all(), n
    for pt, ee in ((False, True), (True, False)):
        cd.activate(point_triangle=pt, edge_edge=ee)
        got = cd.run_proximity(dc.ENL)
        dr.check_proximity(got, dr.only(ref, point_triangle=pt, edge_edge=ee))
        assert all((len(got[n][0]) == 0) == (n.startswith("pt_") != pt) for n in dr.LISTS)
        dr.check_broad_phase(cd.run_broad_phase(dc.ENL), (broad[0] if pt else broad[0][:0], broad[1] if ee else broad[1][:0]))
    cd.close()
    scene, info = dc.pt_atlas()
    cd = detector(scene)
    enl = info["enl"]
    qm = info["query_mesh"]
    i = info["tie_absent"][0][0]
    Q = scene.meshes[qm][0]
    assert Q[i, 2] == enl
    before = cd.run_proximity(enl)
    dr.check_proximity(before, dr.proximity(scene, enl, exact_inputs=True))
    assert (qm, i, 0, 0) not in set(sum((dr.pt_key(before[n][0]) for n in dr.LISTS[:3]), []))
    Q[i, 2] = np.nextafter(Q[i, 2], 0.0)
    after = cd.run_proximity(enl)
    dr.check_proximity(after, dr.proximity(scene, enl, exact_inputs=True))
    assert (qm, i, 0, 0) in dr.pt_key(after["pt_point_triangle"][0])
    cd.close()
