"""Synthesised inputs of the collision-detector tests (tests/test_gpu_detector_synth.py on the device, tests/test_detector_ref_cpu.py for the
builders' own conditions): the atlases on exact ties and the scenes that walk the sweep's paths. Plain numpy; every builder is deterministic."""
from fractions import Fraction

import numpy as np

import detector_ref as dr

STEP = 2.0 ** -8            # the lattice of the atlases: coordinates are integer multiples of STEP with magnitude <= 4
ATLAS_ENL = 80 * STEP       # 0.3125: enl^2 = 25 / 256 is a double, and 48^2 + 64^2 = 80^2 gives lattice points at distance exactly enl
SWEEP_SPLIT = 512           # contact.hip: ranges longer than this are cut into tasks
ENL = 1e-3                  # enlargement of the random scenes
STRIP_LENGTHS = (SWEEP_SPLIT - 1, SWEEP_SPLIT, SWEEP_SPLIT + 1, 3 * SWEEP_SPLIT + 7)


def on_lattice(x):
    x = np.asarray(x, dtype=np.float64)
    return bool((np.abs(x) <= 4).all() and (x / STEP == np.round(x / STEP)).all())


def is_double(fr):
    return Fraction(float(fr)) == fr


# ---- a. point-triangle atlas ------------------------------------------------------------------------------------------------------------------
def pt_atlas():
    """-> (scene, info). Meshes 0..11: the triangle A=(0,0,0) B=(1,0,0) C=(0,1/2,0) in all six vertex orders, then its mirror image (x -> -x)
    in all six; mesh 12: the query points (vertices only). info: `tie_absent` / `tie_present` = (query index, mesh) pairs at distance exactly
    enl / one lattice step closer."""
    A, B, C = np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.5, 0.0])
    h = np.array([0.0, 0.0, 32 * STEP])
    q = []
    tri = (A, B, C)
    for k in range(3):
        e0, e1 = tri[k], tri[(k + 1) % 3]
        b0 = e1 - e0
        m = np.array([b0[1], -b0[0], 0.0])        # in the plane, pointing away from the triangle (A, B, C is counter-clockwise seen from +z)
        q += [e0 + b0 / 2 + m / 8 + h,              # above the edge's half plane, outside
              e0 + b0 / 2 + m / 4,                  # in the plane, outside
              e0 + b0 / 4 + h,                      # across == 0: straight above the edge
              e0 + b0 / 4,                          # on the edge itself (d = 0)
              e0 + m / 8 + h, e0 + m / 8,           # along == 0
              e1 + m / 8 + h, e1 + m / 8,           # along == 1
              e0 - b0 / 8 + h,                      # beyond the edge's start, across == 0
              e0 + h, e0 - h]                       # above and below the vertex
    q += [np.array([0.25, 0.125, 0.0]) + h, np.array([0.25, 0.125, 0.0]) - h, np.array([0.25, 0.125, 0.0])]   # above / below / in the interior (d = 0)
    n_plain = len(q)
    # distance exactly enl, and one lattice step closer: above the interior, beside edge AB (3-4-5), beyond vertex A (3-4-5)
    ties = [(np.array([0.25, 0.125, 80 * STEP]), np.array([0.25, 0.125, 79 * STEP])),
            (np.array([0.5, -48 * STEP, 64 * STEP]), np.array([0.5, -47 * STEP, 64 * STEP])),
            (np.array([-48 * STEP, 0.0, 64 * STEP]), np.array([-47 * STEP, 0.0, 64 * STEP])),
            (np.array([-48 * STEP, 0.0, -64 * STEP]), np.array([-48 * STEP, 0.0, -63 * STEP]))]
    for far, close in ties:
        q += [far, close]
    Q = np.array(q)
    Q = np.concatenate([Q, Q * np.array([-1.0, 1.0, 1.0])])   # the mirror image's queries
    orders = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]
    meshes = []
    for mirror in (1.0, -1.0):
        for o in orders:
            X = np.array([tri[o[0]], tri[o[1]], tri[o[2]]]) * np.array([mirror, 1.0, 1.0])
            meshes.append((X, [[0, 1, 2]], np.zeros((0, 2), dtype=np.int64)))
    meshes.append((Q, np.zeros((0, 3), dtype=np.int64), np.zeros((0, 2), dtype=np.int64)))
    scene = dr.Scene(meshes)
    assert all(on_lattice(m[0]) for m in scene.meshes)
    nq = len(q)
    info = dict(tie_absent=[], tie_present=[], query_mesh=12, enl=ATLAS_ENL)
    enl2 = Fraction(ATLAS_ENL) ** 2
    assert is_double(enl2) and float(enl2) == ATLAS_ENL * ATLAS_ENL
    for half, first_mesh in ((0, 0), (1, 6)):
        for t in range(len(ties)):
            for g in range(first_mesh, first_mesh + 6):
                i_far, i_close = half * nq + n_plain + 2 * t, half * nq + n_plain + 2 * t + 1
                T = scene.meshes[g][0]
                _, d2, _ = dr.point_triangle_exact(Q[i_far], T[0], T[1], T[2])
                assert d2 == enl2 and is_double(d2), (t, g, d2)       # exactly on the tie, in rationals, and a double
                _, d2c, _ = dr.point_triangle_exact(Q[i_close], T[0], T[1], T[2])
                assert d2c < enl2
                info["tie_absent"].append((i_far, g))
                info["tie_present"].append((i_close, g))
    return scene, info


# ---- b. edge-edge atlas ------------------------------------------------------------------------------------------------------------------------
def ee_atlas():
    """-> (scene, info). Mesh 1: the edge a0=(0,0,0) -> a1=(1,0,0), a second edge from a1 (shares a vertex) and the reversed edge on vertices of its
    own; meshes 0 and 2: second edges of four directions on a grid of start points around it at height 1/8 (even ones registered BEFORE the
    first edge's mesh, odd ones after it: both role orders), among them exactly parallel ones; mesh 2 also holds the crossing edges at height
    exactly enl and one step below."""
    dirs = [np.array([0.0, 0.5, 0.0]), np.array([0.5, 0.5, 0.0]), np.array([-0.5, 0.5, 0.0]), np.array([0.0, 0.5, 0.125]), np.array([0.5, 0.0, 0.0])]
    xs = [-0.125, 0.0, 0.125, 0.5, 0.875, 1.0, 1.125]
    ys = [-0.75, -0.5, -0.25, 0.0, 0.125]
    seconds = []
    for v in dirs:
        for x in xs:
            for y in ys:
                b0 = np.array([x, y, 0.125])
                seconds.append((b0, b0 + v))
    even, odd = seconds[0::2], seconds[1::2]
    tie_far = (np.array([0.5, -0.25, 80 * STEP]), np.array([0.5, 0.25, 80 * STEP]))
    tie_close = (np.array([0.25, -0.25, 79 * STEP]), np.array([0.25, 0.25, 79 * STEP]))
    odd = odd + [tie_far, tie_close]

    def edge_mesh(pairs):
        X = np.array([p for pr in pairs for p in pr])
        return (X, np.zeros((0, 3), dtype=np.int64), np.arange(2 * len(pairs)).reshape(-1, 2))

    first = (np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0.25, 0.0], [1.0, 0, 0], [0.0, 0, 0]]), np.zeros((0, 3), dtype=np.int64), [[0, 1], [1, 2], [3, 4]])
    scene = dr.Scene([edge_mesh(even), first, edge_mesh(odd)])
    assert all(on_lattice(m[0]) for m in scene.meshes)
    enl2 = Fraction(ATLAS_ENL) ** 2
    a0, a1 = scene.meshes[1][0][0], scene.meshes[1][0][1]
    ty, d2, _ = dr.edge_edge_exact(a0, a1, tie_far[0], tie_far[1])
    assert ty == dr.EA_EB and d2 == enl2 and is_double(d2)
    ty, d2, _ = dr.edge_edge_exact(a0, a1, tie_close[0], tie_close[1])
    assert ty == dr.EA_EB and d2 < enl2
    n_odd = len(odd)
    info = dict(enl=ATLAS_ENL, tie_absent=((1, 0), (2, n_odd - 2)), tie_present=((1, 0), (2, n_odd - 1)), shared=((1, 0), (1, 1)))
    return scene, info


def ee_cutoff_scenes():
    """two detectors' worth of short near-parallel edge pairs: |u x v|^2 = 2^-100 (<= 1e-30: dropped) and 2^-98 (kept); every feature distance is
    2^-10, far below enl. -> [(scene, kept)]"""
    out = []
    for ybit, kept in ((-40, False), (-39, True)):
        e = 2.0 ** -10
        A = np.array([[0.0, 0.0, 0.0], [e, 0.0, 0.0]])
        B = np.array([[0.0, 0.0, e], [e, 2.0 ** ybit, e]])
        sc = dr.Scene([(A, np.zeros((0, 3)), [[0, 1]]), (B, np.zeros((0, 3)), [[0, 1]])])
        c2 = dr.edge_cross2_exact(A[0], A[1], B[0], B[1])
        assert c2 == Fraction(2) ** (-100 if not kept else -98)
        assert (c2 > dr.EE_CUTOFF) == kept
        out.append((sc, kept))
    return out


# ---- c. intersection atlas --------------------------------------------------------------------------------------------------------------------
def et_atlas(signed_zeros=False):
    """-> (scene, info). Mesh 0: the triangle (0,0,0) (1,0,0) (0,1,0), a second one with the opposite vertex order two units along x, and an edge of
    the mesh's own from a triangle vertex straight up (shares the vertex: never a pair); mesh 1: the probing edges, the same set over either
    triangle; mesh 2: one edge through the first triangle's interior, blacklisted against mesh 0. `signed_zeros`: every zero coordinate of
    mesh 1 is -0.0 (the triangle's stay +0.0)."""
    s = STEP
    probes = [((0.25, 0.25, -0.5), (0.25, 0.25, 0.5), "interior"),
              ((0.0, 0.25, -0.5), (0.0, 0.25, 0.5), "edge"), ((0.25, 0.0, -0.5), (0.25, 0.0, 0.5), "edge"), ((0.5, 0.5, -0.5), (0.5, 0.5, 0.5), "edge"),
              ((0.0, 0.0, -0.5), (0.0, 0.0, 0.5), "vertex"), ((1.0, 0.0, -0.5), (1.0, 0.0, 0.5), "vertex"), ((0.0, 1.0, -0.5), (0.0, 1.0, 0.5), "vertex"),
              ((0.25, 0.25, 0.0), (0.25, 0.25, 1.0), "t==0"), ((0.25, 0.25, -1.0), (0.25, 0.25, 0.0), "t==1"),
              ((0.25, 0.25, -1.0), (0.25, 0.25, -s), "short"), ((0.25, 0.25, s), (0.25, 0.25, 1.0), "short"),
              ((-0.25, 0.25, 0.0), (0.5, 0.25, 0.0), "coplanar"), ((0.125, 0.125, 0.0), (0.25, 0.25, 0.0), "coplanar"), ((1.25, 1.25, 0.0), (1.5, 1.25, 0.0), "coplanar"),
              ((0.5 + s, 0.5, -0.5), (0.5 + s, 0.5, 0.5), "outside"), ((-s, 0.25, -0.5), (-s, 0.25, 0.5), "outside"),
              ((0.0, 0.0, -0.5), (0.5, 0.5, 0.5), "oblique")]
    T = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 1.0, 0], [2.0, 1.0, 0.0], [3.0, 0, 0], [2.0, 0, 0], [0.0, 0.0, 0.5]])
    tris = [[0, 1, 2], [3, 4, 5]]
    own_edges = [[0, 6]]
    P = []
    for off in (0.0, 2.0):
        for q1, q2, _ in probes:
            P += [np.array(q1) + [off, 0, 0], np.array(q2) + [off, 0, 0]]
    P = np.array(P)
    if signed_zeros:
        P = np.where(P == 0.0, -0.0, P)
        assert np.signbit(P[P == 0.0]).all() and not np.signbit(T[T == 0.0]).any()
    Bk = np.array([[0.25, 0.5, -0.5], [0.25, 0.5, 0.5]])
    scene = dr.Scene([(T, tris, own_edges), (P, np.zeros((0, 3)), np.arange(len(P)).reshape(-1, 2)), (Bk, np.zeros((0, 3)), [[0, 1]])])
    scene.blacklist(0, 2)
    assert all(on_lattice(m[0]) for m in scene.meshes)
    labels = [lab for _ in (0, 1) for _, _, lab in probes]
    for k, lab in enumerate(labels):
        tv = T[tris[k // len(probes)]]
        hit, _, det = dr.edge_triangle_exact(P[2 * k], P[2 * k + 1], tv[0], tv[1], tv[2])
        if lab == "coplanar":
            assert det == 0 and not hit
        elif lab in ("short", "outside"):
            assert not hit
        elif lab != "oblique":   # the tie cases
            n, d = abs(det.numerator), det.denominator
            assert n & (n - 1) == 0 and d & (d - 1) == 0, det     # det is +- a power of two: 1 / det is exact
            assert hit, (k, lab)
    return scene, dict(labels=labels, n_probes=len(probes))


# ---- d. sweep structure ------------------------------------------------------------------------------------------------------------------------
def grid(n, h, origin, jitter=None):
    """n x n vertices, spacing h in x and y from `origin`; triangles (two per cell), the unique edges; jitter: [n*n, 3] offsets"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    X = np.stack([origin[0] + h * i.ravel(), origin[1] + h * j.ravel(), np.full(n * n, origin[2])], axis=1).astype(np.float64)
    if jitter is not None:
        X = X + jitter
    v = lambda a, b: a * n + b
    tris = []
    for a in range(n - 1):
        for b in range(n - 1):
            tris += [[v(a, b), v(a + 1, b), v(a + 1, b + 1)], [v(a, b), v(a + 1, b + 1), v(a, b + 1)]]
    tris = np.array(tris, dtype=np.int64)
    e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1)
    edges = np.unique(e, axis=0)
    return X, tris, edges


ROT = None


def rotation():
    """a fixed rotation about (1, 2, 3) by 0.7 rad: no axis stays an axis"""
    global ROT
    if ROT is None:
        k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        ROT = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    return ROT


def two_grids(n=24, seed=11, shift=(0.0, 0.0, 0.0)):
    """d.1 / d.5: two jittered n x n grids 0.7 enl apart, rotated by rotation() about the scene's centre (coordinates of both signs), then
    translated by `shift`. -> (scene, normal): moving mesh 1 by -t * normal pushes it through mesh 0."""
    rng = np.random.default_rng(seed)
    h = 3.0 * ENL
    o = -0.5 * (n - 1) * h
    meshes = []
    for k in range(2):
        jit = rng.uniform(-1.0, 1.0, size=(n * n, 3)) * np.array([0.15 * h, 0.15 * h, 0.08 * ENL])
        X, t, e = grid(n, h, (o + 0.31 * h * k, o + 0.17 * h * k, (k - 0.5) * 0.7 * ENL), jit)
        meshes.append((np.ascontiguousarray(X @ rotation().T + np.asarray(shift)), t, e))
    return dr.Scene(meshes), rotation()[:, 2].copy()


def lattice_grids(n=24):
    """d.2: the two grids axis-aligned on the 2^-8 lattice, no jitter: spacing 16 steps, 7 steps apart, enl = 10 steps"""
    o = -8 * (n - 1) * STEP
    meshes = [grid(n, 16 * STEP, (o, o, 0.0)), grid(n, 16 * STEP, (o, o, 7 * STEP))]
    sc = dr.Scene(meshes)
    assert all(on_lattice(m[0]) for m in sc.meshes)
    return sc, 10 * STEP


def lattice_push(scene, n=24):
    """d.2, second state, in place: the second grid becomes a zigzag through the first one's plane (vertices 4 steps above / below it by the parity
    of their grid position) and moves half a cell along x. Its axis-parallel edges then cross the plane z = 0 exactly over vertices and edges of
    the first grid (u == 0, v == 0, u + v == 1 ties), with det = -(dir . n) = +-8 steps x 256 steps^2: a power of two, so 1 / det is exact."""
    X = scene.meshes[1][0]
    parity = ((np.arange(n)[:, None] + np.arange(n)[None, :]) % 2).ravel()
    X[:, 2] = np.where(parity == 0, 4.0, -4.0) * STEP
    X[:, 0] += 8 * STEP
    assert on_lattice(X)


def strip_points(n, seed=5):
    """d.3: one long thin triangle (mesh 0) over a straight strip of n points (mesh 1) spaced along x, all within enl of it; the spread in y and z
    stays below enl, so every box lies in every band and the triangle's range is the whole strip"""
    rng = np.random.default_rng(seed + n)
    dx = 0.25 * ENL
    T = np.array([[-2 * ENL, -0.3 * ENL, 0.0], [n * dx + 2 * ENL, -0.3 * ENL, 0.013 * ENL], [0.5 * n * dx, 0.3 * ENL, -0.011 * ENL]])
    P = np.stack([dx * np.arange(n) + rng.uniform(-0.3, 0.3, n) * dx, rng.uniform(-0.1, 0.1, n) * ENL, (0.5 + rng.uniform(-0.2, 0.2, n)) * ENL], axis=1)
    return dr.Scene([(T, [[0, 1, 2]], np.zeros((0, 2))), (P, np.zeros((0, 3)), np.zeros((0, 2)))])


def strip_edges(n, seed=6):
    """d.3: one long edge (mesh 0) over a strip of n short skew edges (mesh 1, no pairs inside it)"""
    rng = np.random.default_rng(seed + n)
    dx = 0.25 * ENL
    A = np.array([[-2 * ENL, 0.01 * ENL, 0.0], [n * dx + 2 * ENL, -0.02 * ENL, 0.017 * ENL]])
    x = dx * np.arange(n) + rng.uniform(-0.3, 0.3, n) * dx
    z = (0.5 + rng.uniform(-0.2, 0.2, n)) * ENL
    B0 = np.stack([x, -0.2 * ENL + rng.uniform(-0.05, 0.05, n) * ENL, z], axis=1)
    B1 = np.stack([x + rng.uniform(-0.1, 0.1, n) * dx, 0.2 * ENL + rng.uniform(-0.05, 0.05, n) * ENL, z + rng.uniform(-0.1, 0.1, n) * ENL], axis=1)
    X = np.stack([B0, B1], axis=1).reshape(-1, 3)
    sc = dr.Scene([(A, np.zeros((0, 3)), [[0, 1]]), (X, np.zeros((0, 3)), np.arange(2 * n).reshape(-1, 2))])
    sc.blacklist(1, 1)
    return sc


def strip_triangles(n, seed=7):
    """d.3, intersection sweep: one long edge (mesh 0) through a strip of n small triangles (mesh 1) that all span the same y interval, so they
    share their first band and the edge meets all of them in one range"""
    rng = np.random.default_rng(seed + n)
    dx = 0.25 * ENL
    A = np.array([[-2 * ENL, 0.01 * ENL, 0.003 * ENL], [n * dx + 2 * ENL, -0.02 * ENL, -0.004 * ENL]])
    x = dx * np.arange(n)
    w = 0.3 * ENL
    V0 = np.stack([x + rng.uniform(-0.1, 0.1, n) * dx, np.full(n, -w), -0.4 * ENL + rng.uniform(-0.1, 0.1, n) * ENL], axis=1)
    V1 = np.stack([x + rng.uniform(-0.1, 0.1, n) * dx, np.full(n, -w), 0.4 * ENL + rng.uniform(-0.1, 0.1, n) * ENL], axis=1)
    V2 = np.stack([x + rng.uniform(-0.1, 0.1, n) * dx, np.full(n, w), rng.uniform(-0.1, 0.1, n) * ENL], axis=1)
    X = np.stack([V0, V1, V2], axis=1).reshape(-1, 3)
    return dr.Scene([(A, np.zeros((0, 3)), [[0, 1]]), (X, np.arange(3 * n).reshape(-1, 3), np.zeros((0, 2)))])


def rods(kind, n=400):
    """d.4: two straight rods of n edges each, edges only. "skew": on two skew lines that cross at distance 0.5 enl. "axis": every vertex of the
    scene on ONE line parallel to x (the second rod continues the first with an overlap): the band axis has extent 0, its 1e-12 clamp applies and
    every box falls into all 64 bands (1600 boxes x 64 entries: the band list outgrows n + n / 2 + 4096)."""
    L = 0.5 * ENL
    s = (np.arange(n + 1) - 0.5 * n + 0.37) * L
    if kind == "skew":
        d0 = np.array([1.0, 0.3, 0.2]) / np.linalg.norm([1.0, 0.3, 0.2])
        d1 = np.array([0.4, -1.0, 0.1]) / np.linalg.norm([0.4, -1.0, 0.1])
        nrm = np.cross(d0, d1) / np.linalg.norm(np.cross(d0, d1))
        X0 = s[:, None] * d0[None, :]
        X1 = (s + 0.21 * L)[:, None] * d1[None, :] + 0.5 * ENL * nrm[None, :]
    else:
        X0 = np.stack([s, np.full(n + 1, 0.25), np.full(n + 1, -0.125)], axis=1)
        X1 = np.stack([s + 0.3 * n * L + 0.4 * L, np.full(n + 1, 0.25), np.full(n + 1, -0.125)], axis=1)
    e = np.stack([np.arange(n), np.arange(n) + 1], axis=1)
    return dr.Scene([(np.ascontiguousarray(X0), np.zeros((0, 3)), e), (np.ascontiguousarray(X1), np.zeros((0, 3)), e)])


def stacked_patches(n_mesh=40, seed=3):
    """d.6: n_mesh jittered 2 x 2-cell patches stacked 0.6 enl apart; mesh blacklists on a fixed pseudo-random third of the mesh pairs and on some
    self pairs, one point-triangle and one edge-edge range blacklist"""
    rng = np.random.default_rng(seed)
    h = 1.2 * ENL
    meshes = []
    for k in range(n_mesh):
        jit = rng.uniform(-1.0, 1.0, size=(9, 3)) * np.array([0.1 * h, 0.1 * h, 0.05 * ENL])
        meshes.append(grid(3, h, (-h + 0.07 * h * (k % 5), -h - 0.05 * h * (k % 3), 0.6 * ENL * k), jit))
    sc = dr.Scene(meshes)
    for a in range(n_mesh):
        for b in range(a + 1, n_mesh):
            if rng.integers(0, 3) == 0:
                sc.blacklist(a, b)
    for a in range(0, n_mesh, 7):
        sc.blacklist(a, a)
    free = [(a, a + 1) for a in range(n_mesh - 1) if (a, a + 1) not in sc.disabled]
    (a, b), (c, d) = free[0], free[-1]
    sc.bl_pt.append((a, (2, 7), b, (1, 6)))     # points 2..6 of mesh a never pair with triangles 1..5 of mesh b
    sc.bl_ee.append((c, (3, 12), d, (0, 9)))    # edges 3..11 of mesh c (the lower ones) with edges 0..8 of mesh d
    return sc
