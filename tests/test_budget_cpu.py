"""Budget readout without a GPU: the numpy restatement of tests/budget_ref.py against closed forms of rigid motion, and the arithmetic header
stark_amd/csrc/budget.hpp compiled with g++ (tests/host_budget/host_budget.cpp, test-only) against the restatement.

Tolerances are multiples of 2^-53 * S_abs, S_abs = sum |terms| of the slot: (n + 8) for a sum of n items against math.fsum of the same terms (any
summation order), 64 for the fixed number of operations of one body; where BOTH sides are rounded sums of n terms built by different formulas, twice
(n + 8) for the two sums times 4 for the handful of roundings inside a term."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import budget_ref as br  # noqa: E402
from oracle import contact as oc  # noqa: E402
from oracle import evaluator as ev  # noqa: E402

U = br.U


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_budget_"), "host_budget.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host_budget", "host_budget.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p = ctypes.c_void_p
    lib.host_budget_points.argtypes = [p, p, ctypes.c_int, ctypes.c_int, p, p]
    lib.host_budget_bodies.argtypes = [p, p, p, p, p, p, ctypes.c_int, ctypes.c_double, p, p, p]
    lib.host_budget_R1.argtypes = [p, p, ctypes.c_double, p]
    return lib


def _lattice(n, size, centre, masses):
    ax = [(np.arange(n[k]) + 0.5) / n[k] * size[k] - 0.5 * size[k] for k in range(3)]
    x = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return x + centre, masses(len(x))


def _inertia_of_points(m, r):
    return (m[:, None, None] * ((r * r).sum(axis=1)[:, None, None] * np.eye(3) - r[:, :, None] * r[:, None, :])).sum(axis=0)


def test_rigid_motion_of_a_lattice():
    """Point masses moving as v = v_c + w x (x - c), c their centre of mass: p = M v_c, L = c x p + I w, T = 0.5 M v_c^2 + 0.5 w.I w."""
    rng = np.random.default_rng(5)
    x, m = _lattice((5, 4, 3), (0.5, 0.4, 0.3), np.array([0.3, -0.2, 1.1]), lambda k: 0.5 + rng.random(k))
    M = m.sum()
    c = (m[:, None] * x).sum(axis=0) / M
    v_c, w = np.array([0.7, -0.4, 0.25]), np.array([1.5, -2.0, 0.8])
    v = v_c + np.cross(w, x - c)
    gravity = np.array([0.0, 0.0, -9.81])
    rec, mag = br.point_records(m, x, v, np.zeros(len(m), dtype=int), 1, np.zeros(3), gravity)
    rec, mag = rec[0], mag[0]
    I = _inertia_of_points(m, x - c)
    want = np.r_[M, M * c, M * v_c, np.cross(c, M * v_c) + I @ w, 0.5 * M * v_c @ v_c + 0.5 * w @ I @ w, -M * gravity @ c, len(m)]
    tol = 8.0 * (len(m) + 8) * U * mag
    print("lattice: worst |difference| / bound %.3g" % float((np.abs(rec - want) / tol).max()))
    assert (np.abs(rec - want) <= tol).all()
    # about another point: L' = L - a x p
    a = np.array([0.2, 0.1, -0.3])
    rec_a, mag_a = br.point_records(m, x, v, np.zeros(len(m), dtype=int), 1, a, gravity)
    assert (np.abs(rec_a[0, 7:10] - (want[7:10] - np.cross(a, M * v_c))) <= 8.0 * (len(m) + 8) * U * mag_a[0, 7:10]).all()


def test_solid_box_through_the_rigid_body_path():
    """One body with inertia_tensor_box's tensor, rotated by a non-trivial q1, against matrix algebra — and against a midpoint lattice of n^3 equal
    point masses filling the same box and moving with it, whose inertia is exactly (1 - 1/n^2) times the solid's."""
    mass, size = 2.5, (0.3, 0.2, 0.1)
    J = br.inertia_tensor_box(mass, size)
    q1 = br.quat_advance(np.array([0.8, 0.2, -0.4, 0.4]) / np.linalg.norm([0.8, 0.2, -0.4, 0.4]), np.array([3.0, -2.0, 1.0]), 0.05)
    R = br.quat_to_R(q1)
    assert abs(np.trace(R) - 3.0) > 0.5 and np.abs(R @ R.T - np.eye(3)).max() < 1e-15
    t = np.array([0.4, -0.1, 0.9])
    v, w = np.array([0.3, 0.2, -0.5]), np.array([2.0, 1.0, -3.0])
    about, gravity = np.array([0.1, 0.2, 0.3]), np.array([0.0, 0.0, -9.81])
    rec, mag = br.body_record(mass, t, R, v, w, J, about, gravity)
    J1 = R @ J @ R.T
    want = np.r_[mass, mass * t, mass * v, np.cross(t - about, mass * v) + J1 @ w, 0.5 * mass * v @ v + 0.5 * w @ J1 @ w, -mass * gravity @ t, 1.0]
    assert (np.abs(rec - want) <= 64 * U * mag).all()
    n = 6
    xl, m = _lattice((n, n, n), size, np.zeros(3), lambda k: np.full(k, mass / k))
    x = xl @ R.T + t
    vp = v + np.cross(w, x - t)
    rec_l, mag_l = br.point_records(m, x, vp, np.zeros(len(m), dtype=int), 1, about, gravity)
    rec_s, mag_s = br.body_record(mass, t, R, v, w, (1.0 - 1.0 / n ** 2) * J, about, gravity)
    tol = 8.0 * (len(m) + 8) * U * np.maximum(mag_l[0], mag_s)
    assert (np.abs(rec_l[0, :12] - rec_s[:12]) <= tol[:12]).all()
    assert rec_l[0, 12] == n ** 3 and rec_s[12] == 1.0


def _inertia_inputs(volume, density, x0, v1, dt, gravity, group, rng=None):
    """[n, 23] gathered inputs of EnergyLumpedInertia in binding order (the entries the budget does not read hold NaN)."""
    n = len(volume)
    inp = np.full((n, 23), np.nan)
    inp[:, 0:3], inp[:, 3:6] = v1, x0
    inp[:, 15], inp[:, 16], inp[:, 19] = volume, np.asarray(density)[group], dt
    inp[:, 20:23] = gravity
    return np.ascontiguousarray(inp)


def dyadic_items(rng, n, n_groups):
    """The exact family: volumes integer / 8, density 1, x0 and v1 integer / 64 with |integer| < 32, dt = 1 / 8, gravity (0, 0, -8)."""
    volume = rng.integers(1, 32, n) / 8.0
    x0 = rng.integers(-31, 32, (n, 3)) / 64.0
    v1 = rng.integers(-31, 32, (n, 3)) / 64.0
    return volume, np.ones(n_groups), x0, v1, 0.125, np.array([0.0, 0.0, -8.0])


def test_host_build_points_against_restatement(host_lib):
    rng = np.random.default_rng(11)
    n, ng = 700, 3
    group = rng.integers(0, ng, n).astype(np.int32)
    about = np.array([0.25, -0.5, 0.125])
    # random
    volume, density = 0.1 + rng.random(n), 500.0 + 1000.0 * rng.random(ng)
    x0, v1, dt, gravity = 1.0 + rng.random((n, 3)), rng.standard_normal((n, 3)), 0.01, np.array([0.3, -0.2, -9.81])
    rec = np.full((ng, 13), np.nan)
    assert host_lib.host_budget_points(_inertia_inputs(volume, density, x0, v1, dt, gravity, group).ctypes.data, group.ctypes.data, n, ng, about.ctypes.data, rec.ctypes.data) == 0
    want, mag = br.inertia_records(volume, density, x0, v1, dt, group, ng, about, gravity)
    cnt = np.bincount(group, minlength=ng)[:, None]
    print("random points: worst |difference| / bound %.3g" % float((np.abs(rec - want) / ((cnt + 8) * U * mag)).max()))
    assert (np.abs(rec - want) <= (cnt + 8) * U * mag).all()
    # dyadic: every operation exact, so the records are the restatement's bit for bit
    volume, density, x0, v1, dt, gravity = dyadic_items(rng, n, ng)
    br.assert_exact_family(volume, density, x0, v1, dt, group, ng, about, gravity)
    assert host_lib.host_budget_points(_inertia_inputs(volume, density, x0, v1, dt, gravity, group).ctypes.data, group.ctypes.data, n, ng, about.ctypes.data, rec.ctypes.data) == 0
    want, _ = br.inertia_records(volume, density, x0, v1, dt, group, ng, about, gravity)
    assert (rec == want).all()


def _host_bodies(lib, t0, q0, v1, w1, mass, J, dt, about, gravity):
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (t0, q0, v1, w1, mass, J, about, gravity)]
    rec = np.full((len(mass), 13), np.nan)
    assert lib.host_budget_bodies(*[a.ctypes.data for a in arrs[:6]], len(mass), dt, arrs[6].ctypes.data, arrs[7].ctypes.data, rec.ctypes.data) == 0
    return rec


def test_host_build_bodies_against_restatement(host_lib):
    rng = np.random.default_rng(12)
    n = 40
    q0 = rng.standard_normal((n, 4))
    q0 /= np.linalg.norm(q0, axis=1)[:, None]
    t0, v1, w1 = rng.standard_normal((n, 3)), rng.standard_normal((n, 3)), 3.0 * rng.standard_normal((n, 3))
    mass = 0.5 + rng.random(n)
    J = np.array([br.inertia_tensor_box(m, 0.1 + rng.random(3)) for m in mass]).reshape(n, 9)
    about, gravity, dt = np.array([0.25, -0.5, 0.125]), np.array([0.3, -0.2, -9.81]), 0.01
    rec = _host_bodies(host_lib, t0, q0, v1, w1, mass, J, dt, about, gravity)
    want, mag = br.rigid_records(t0, q0, v1, w1, mass, J, dt, about, gravity)
    print("random bodies: worst |difference| / bound %.3g" % float((np.abs(rec - want) / (64 * U * mag)).max()))
    assert (np.abs(rec - want) <= 64 * U * mag).all()
    # dyadic and not rotating (q0 the identity, w1 = 0: R = I exactly): bit for bit
    t0, v1 = rng.integers(-31, 32, (n, 3)) / 64.0, rng.integers(-31, 32, (n, 3)) / 64.0
    q0 = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    mass = rng.integers(1, 32, n) / 8.0
    rec = _host_bodies(host_lib, t0, q0, v1, np.zeros((n, 3)), mass, J, 0.125, about, np.array([0.0, 0.0, -8.0]))
    want, _ = br.rigid_records(t0, q0, v1, np.zeros((n, 3)), mass, J, 0.125, about, np.array([0.0, 0.0, -8.0]))
    assert (rec == want).all()


def test_quaternion_advance_against_the_oracle_on_rbchain(host_lib):
    """The shared update (energies.hpp rb_R1) and the restatement against the oracle's rigid-body transformation at the rbchain fixture's states."""
    prob, man, z = ev.load_fixture(os.path.join(ROOT, "tests", "golden", "rbchain.npz"))
    (q0,) = [a for a in prob.arrays if a.ndim == 2 and a.shape[1] == 4]
    w1 = np.asarray(prob.arrays[prob.dof_arrays[max(prob.dof_arrays)]]).reshape(-1, 3)
    assert len(q0) == len(w1) == 9 and np.abs(w1).max() > 0.0
    for dt in (prob.dt, 10.0 * prob.dt):
        for b in range(len(q0)):
            R_or = oc.quat_to_R(oc.quat_time_integration(q0[b], w1[b], dt))
            R_ref = br.quat_to_R(br.quat_advance(q0[b], w1[b], dt))
            R = np.full(9, np.nan)
            qb, wb = np.ascontiguousarray(q0[b]), np.ascontiguousarray(w1[b])
            assert host_lib.host_budget_R1(qb.ctypes.data, wb.ctypes.data, dt, R.ctypes.data) == 0
            # entries of a rotation are sums of a handful of products of unit-quaternion components: 16 roundings of magnitude <= 2
            assert np.abs(R.reshape(3, 3) - R_or).max() <= 32 * U
            assert np.abs(R_ref - R_or).max() <= 32 * U
