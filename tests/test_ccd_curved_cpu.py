"""The curved rigid-body CCD without a GPU: the deviation bound the padded query rests on, the padded additive CCD, the whole restated query
(tests/ccd_curved_ref.py) against the true curved motion, the scene that tells the curved query from the linear one, and the arithmetic header
stark_amd/csrc/ccd_pad.hpp compiled with g++ (tests/host_ccd_pad/host_ccd_pad.cpp, test-only) against the restatement."""
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ccd_curved_ref as CR
import ccd_ref as R
from test_ccd_cpu import CASES, _random_crossings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_ccd_pad", "host_ccd_pad.cpp")
U = 2.0 ** -53
ETA = 0.9


def _random_motion(rng):
    """(t0, q0, v, w, dv, dw, dt, x_loc, tau) with phi tau = dt |dw| tau log-uniform over [1e-4, 12] (beyond pi: the 2 r cap takes over)"""
    q0 = rng.normal(size=4)
    q0 /= np.linalg.norm(q0)
    dt = rng.uniform(0.005, 0.1)
    tau = float(rng.choice([1.0, 0.5, 0.25]))
    a = 10.0 ** rng.uniform(-4.0, math.log10(12.0))
    dw = rng.normal(size=3)
    dw *= a / (tau * dt) / np.linalg.norm(dw)
    w = rng.normal(size=3) * rng.uniform(0.0, 30.0)
    x_loc = rng.normal(size=3) * rng.uniform(0.01, 2.0)
    return rng.normal(size=3), q0, rng.normal(size=3), w, rng.normal(size=3) * 3.0, dw, dt, x_loc, tau


# ---- 1. the bound ------------------------------------------------------------------------------------------------------------------------------
def test_vectorised_path_is_the_scalar_update():
    rng = np.random.default_rng(1)
    for _ in range(20):
        t0, q0, v, w, dv, dw, dt, x_loc, tau = _random_motion(rng)
        ts = np.array([0.0, 0.3 * tau, tau])
        P = CR.rigid_path(t0, q0, v, w, dv, dw, dt, x_loc, ts)
        for t, p in zip(ts, P):
            want = CR.rigid_point(t0, q0, v + t * dv, w + t * dw, dt, x_loc)
            assert np.abs(p - want).max() <= 64 * U * (np.linalg.norm(x_loc) + np.abs(want).max())


def test_deviation_from_the_chord_is_within_the_bound():
    """| p(t) - chord over [0, tau] | <= delta(tau) = min((7/16) r (phi tau)^2, 2 r) on 2400 random motions sampled at 401 points each; halving tau
    quarters delta exactly where the cap is inactive. Slack: the roundings of the sampled positions, 64 * 2^-53 of their magnitude."""
    rng = np.random.default_rng(2)
    worst, n_cap, n_beyond_pi = 0.0, 0, 0
    u = np.linspace(0.0, 1.0, 401)
    for _ in range(2400):
        t0, q0, v, w, dv, dw, dt, x_loc, tau = _random_motion(rng)
        phi, r = CR.pad_phi(dt, dw), float(np.linalg.norm(x_loc))
        delta = CR.pad_vertex(x_loc, phi, tau)
        P = CR.rigid_path(t0, q0, v, w, dv, dw, dt, x_loc, u * tau)
        chord = P[0][None, :] + u[:, None] * (P[-1] - P[0])[None, :]
        dev = float(np.linalg.norm(P - chord, axis=1).max())
        assert dev <= delta + 64 * U * (r + np.abs(P).max()), (dev, delta, phi, tau, r)
        capped = delta == 2.0 * math.sqrt(x_loc[0] ** 2 + x_loc[1] ** 2 + x_loc[2] ** 2)
        n_cap += capped
        n_beyond_pi += phi * tau > math.pi
        if not capped:
            assert CR.pad_vertex(x_loc, phi, 0.5 * tau) == 0.25 * delta
            if phi * tau > 1e-2:   # (below, the deviation itself is lost in the roundings of positions of size r)
                worst = max(worst, dev / delta)
    print("worst sampled deviation / bound: %.4f (cap active in %d motions, phi tau > pi in %d)" % (worst, n_cap, n_beyond_pi))
    assert n_cap > 50 and n_beyond_pi > 100 and 0.2 < worst <= 1.0
    assert CR.pad_delta(0.7, 0.0, 1.0) == 0.0 and CR.pad_delta(0.0, 3.0, 1.0) == 0.0 and math.copysign(1.0, CR.pad_delta(0.7, 0.0, 1.0)) == 1.0


# ---- 2. the padded ACCD ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_padded_accd_without_pad_is_accd(case):
    name, ee, xa, xb, t_star = case
    xa, xb = np.asarray(xa, float), np.asarray(xb, float)
    want = R.accd(ee, xa, xb, ETA)
    got = CR.accd_padded(ee, xa, xb, 0.0, ETA)
    assert {k: got[k] for k in want} == want and not got["bound"]
    if want["status"] == "hit":
        assert CR.last_step_padded(ee, xa, xb, 0.0, ETA, want["toi"]) == R.last_step(ee, xa, xb, ETA, want["toi"])


def test_padded_accd_never_passes_the_thickened_contact():
    """Straight-line pairs thickened by their pad: for every sampled t up to the reported toi the distance stays above the pad, at the toi of a hit
    it keeps (1 - eta) of the padded gap, and a pad that leaves no gap reports 0."""
    rng = np.random.default_rng(8)
    n_hit = n_zero = n_bound = 0
    for k, (ee, xa, xb, t_star) in enumerate(_random_crossings(rng, 240)):
        d0 = R.distance(ee, [tuple(p) for p in xa])
        pad = d0 * [0.0, 0.05, 0.45, 0.55, 0.9, 1.0, 1.7][k % 7]
        r = CR.accd_padded(ee, xa, xb, pad, ETA)
        assert r["status"] != "touching"
        if pad >= d0:
            assert r["status"] == "zero_gap" and r["toi"] == 0.0 and r["bound"]
            n_zero += 1
            continue
        assert r["status"] in ("hit", "capped"), r    # (the unpadded pair crosses at t_star, so the thickened one is reached before)
        assert 0.0 < r["toi"] <= t_star
        assert r["bound"] == (pad > 0.5 * d0)
        n_bound += r["bound"]
        ts = np.linspace(0.0, r["toi"], 400)
        d = np.array([R.distance(ee, [tuple(p) for p in xa + t * (xb - xa)]) for t in ts])
        assert (d - pad > 0.0).all(), (k, float((d - pad).min()))
        if r["status"] == "hit":
            n_hit += 1
            assert d[-1] - pad >= (1.0 - ETA) * (d0 - pad) * (1 - 1e-9)
    print("hits %d, no gap %d, pad-bound %d" % (n_hit, n_zero, n_bound))
    assert n_hit > 150 and n_zero > 60 and n_bound > 60


# ---- 3. the whole query against the true motion ----------------------------------------------------------------------------------------------
def _random_scene(rng):
    """a rigid triangle (spinning, about to turn by phi = dt |dw| in [0.01, 6] more along the direction) next to a moving deformable triangle"""
    tri = dict(verts=[0, 1, 2], tris=[[0, 1, 2]], edges=[[0, 1], [1, 2], [2, 0]])
    q0 = rng.normal(size=4)
    q0 /= np.linalg.norm(q0)
    t0, dt = rng.normal(size=3) * 0.1, 0.05
    x0 = t0 + rng.normal(size=3) * 0.35 + rng.normal(size=(3, 3)) * 0.15
    sc = CR.Scene([dict(kind="rb", body=0, **tri), dict(kind="d", **tri)], x0, rng.normal(size=(3, 3)), rng.normal(size=(3, 3)) * 0.3, [t0], [q0], [rng.normal(size=3)],
                  [rng.normal(size=3) * rng.uniform(0.0, 10.0)], dt)
    dw = rng.normal(size=3)
    dw *= 10.0 ** rng.uniform(-2.0, 0.8) / dt / np.linalg.norm(dw)
    return sc, rng.normal(size=(3, 3)) * rng.uniform(0.0, 4.0), rng.normal(size=(1, 3)) * rng.uniform(0.0, 6.0), dw[None, :]


def check_against_true_motion(sc, dv1, dv, dw, res, eta, samples):
    """For `samples` values of t in [0, max_step] and every pair, by brute force: the true classified distance is > 0, and at max_step it is
    >= (1 - eta) (d(0) - pad) - 1e-12, pad the pair's pad of the last round. (Proved: the first for every pair, the second for the pair that
    limits the step; asserted for all.) Returns the smallest distance seen."""
    pairs = sc.all_pairs()
    D = CR.true_distances(sc, dv1, dv, dw, np.linspace(0.0, res["max_step"], samples), pairs)
    assert (D[0] > 0.0).all()
    assert (D > 0.0).all(), float(D.min())
    for j, (ee, v) in enumerate(pairs):
        pad = CR.pair_pad(ee, res["pad_v"][v])
        assert D[-1, j] >= (1.0 - eta) * (D[0, j] - pad) - 1e-12, (j, D[-1, j], D[0, j], pad)
    return float(D.min())


def test_restated_query_keeps_the_true_motion_apart():
    rng = np.random.default_rng(3)
    scenes = [_random_scene(rng) for _ in range(40)]
    results = [CR.max_step_curved(sc, dv1, dv, dw, ETA, 4) for sc, dv1, dv, dw in scenes]
    rounds = [r["rounds"] for r in results]
    limited = [k for k, r in enumerate(results) if 0.0 < r["max_step"] < 1.0]
    print("rounds histogram", np.bincount(rounds, minlength=5).tolist(), "limited", len(limited), "no step", sum(r["max_step"] == 0.0 for r in results))
    assert len(limited) >= 8 and max(rounds) == 4 and any(results[k]["rounds"] > 1 for k in limited)
    dense = limited[:4] + [k for k in limited if results[k]["rounds"] > 1][:2]
    for k, ((sc, dv1, dv, dw), res) in enumerate(zip(scenes, results)):
        check_against_true_motion(sc, dv1, dv, dw, res, ETA, 2001 if k in dense else 101)
        assert res["tau"] == 0.5 ** (res["rounds"] - 1) and res["max_step"] == res["tau"] * res["query"]["toi"]
        if res["rounds"] < 4:
            assert res["pad_bound_pairs"] == 0
    # without a change of the angular velocity the curved query is the linear one
    for sc, dv1, dv, dw in scenes[:10]:
        a, b = CR.max_step_linear(sc, dv1, dv, 0.0 * dw, ETA), CR.max_step_curved(sc, dv1, dv, 0.0 * dw, ETA, 4)
        assert (a["max_step"], a["n_candidates"], 1, 0.0) == (b["max_step"], b["n_candidates"], b["rounds"], b["max_pad"])


# ---- 4. the discriminating scene ---------------------------------------------------------------------------------------------------------------
def blade_crossing_time(phi):
    """fraction of the direction at which the blade's axis lies in the triangle's plane: the body has turned by 2 atan(t phi / 2), the plane sits at
    half of the full angle 2 atan(phi / 2). The blade's leading edge touches the triangle just before."""
    return math.tan(0.5 * math.atan(0.5 * phi)) / (0.5 * phi)


def test_blade_scene_tells_curved_from_linear():
    phi = 1.2
    sc, dv1, dv, dw = CR.blade_scene(phi)
    assert abs(CR.pad_phi(sc.dt, dw[0]) - phi) <= 4 * U * phi
    t_cross = blade_crossing_time(phi)
    ts = np.linspace(0.0, 1.0, 2001)
    D = CR.true_distances(sc, dv1, dv, dw, ts).min(axis=1)
    k = int(np.argmax(D < 2e-4))
    t_touch = ts[k]   # a sample at which the blade is within 0.2 mm of the triangle: no later than the first touch is far
    assert D[k] < 2e-4 and 0.9 * t_cross < t_touch <= t_cross, (t_touch, t_cross)
    # the chord of the tip passes inside of the triangle (nearest the axis at its middle) while the blade itself reaches through it
    lin = CR.max_step_linear(sc, dv1, dv, dw, ETA)
    mid = 0.5 * (lin["xa"][0] + lin["xb"][0])
    assert 0.02 < 0.46 - np.linalg.norm(mid) < 0.04
    print("blade: first touch of the true motion at t = %.4f (axis in the plane at %.4f); linear max_step %.6f, " % (t_touch, t_cross, lin["max_step"]), end="")
    assert lin["max_step"] > t_cross    # the documented limitation: the linear query lets the line search pass the contact
    cur = CR.max_step_curved(sc, dv1, dv, dw, ETA, 4)
    print("curved max_step %.6f in %d rounds (tau %.3g, largest pad %.4g)" % (cur["max_step"], cur["rounds"], cur["tau"], cur["max_pad"]))
    assert 0.0 < cur["max_step"] < t_touch
    check_against_true_motion(sc, dv1, dv, dw, cur, ETA, 2001)


# ---- 5., 6. the header the device compiles ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_ccd_pad_"), "host_ccd_pad.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p = ctypes.c_void_p
    lib.host_ccd_pad.argtypes = [p, p, p, p, ctypes.c_int, p]
    lib.host_ccd_true_point.argtypes = [p, p, p, p, p, p, ctypes.c_double, p, ctypes.c_double, p]
    return lib


def test_host_build_of_the_pad_against_restatement(host_lib):
    rng = np.random.default_rng(4)
    n = 3000
    ms = [_random_motion(rng) for _ in range(n)]
    x_loc, dw = np.ascontiguousarray([m[7] for m in ms]), np.ascontiguousarray([m[5] for m in ms])
    dt, tau = np.ascontiguousarray([m[6] for m in ms]), np.ascontiguousarray([m[8] for m in ms])
    dw[::7] = 0.0
    pad = np.full(n, np.nan)
    assert host_lib.host_ccd_pad(x_loc.ctypes.data, dw.ctypes.data, dt.ctypes.data, tau.ctypes.data, n, pad.ctypes.data) == 0
    want = np.array([CR.pad_vertex(x_loc[i], CR.pad_phi(dt[i], dw[i]), tau[i]) for i in range(n)])
    assert (np.abs(pad - want) <= 8 * U * want).all()    # (a handful of roundings; a compiler may fuse a product into a sum)
    assert (pad[::7] == 0.0).all() and not np.signbit(pad[::7]).any()
    # the true point of the header's own rb_R1 against the restatement's
    for m in ms[:50]:
        t0, q0, v, w, dv, dw1, dt1, xl, tau1 = (np.ascontiguousarray(a, dtype=np.float64) if not np.isscalar(a) else a for a in m)
        out = np.full(3, np.nan)
        assert host_lib.host_ccd_true_point(t0.ctypes.data, q0.ctypes.data, v.ctypes.data, w.ctypes.data, dv.ctypes.data, dw1.ctypes.data, float(dt1), xl.ctypes.data,
                                            float(tau1), out.ctypes.data) == 0
        want = CR.rigid_point(t0, q0, v + tau1 * dv, w + tau1 * dw1, dt1, xl)
        assert np.abs(out - want).max() <= 64 * U * (np.linalg.norm(xl) + np.abs(want).max())


def test_sanitizer_run_of_the_header():
    """The same file as a stand-alone program (its own main, no Python in the process, no preload) under AddressSanitizer and UBSan."""
    exe = os.path.join(tempfile.mkdtemp(prefix="mistark_host_ccd_pad_"), "host_ccd_pad_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOST_CCD_PAD_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "motions 400 bad 0" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


def test_curved_ccd_symbols_declared():
    decl = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("mistark_contact.h", "mistark_tmcd.h", "mistark_sim.h")}
    assert re.search(r"int mistark_contact_max_step_ex\(mistark_ctx\* ctx, double dt, double conservative_rescaling, int rigid_mode, int max_rounds, const double\* du, "
                     r"mistark_ccd_result\* out\);", decl["mistark_contact.h"])
    assert re.search(r"int mistark_cd_run_ccd_padded\(mistark_cd\* cd, const double\* const\* x1, const double\* const\* pad, double conservative_rescaling, double\* toi, "
                     r"int32_t\* n_candidates,\s+int32_t\* n_pad_bound\);", decl["mistark_tmcd.h"])
    assert "mistark_sim_set_contact_ccd_rigid(" in decl["mistark_sim.h"] and "mistark_sim_get_ccd_rigid_info(" in decl["mistark_sim.h"]
