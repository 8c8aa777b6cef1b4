"""The CCD restatement (tests/ccd_ref.py) on trajectories with closed-form crossing times, and the CCD entry points in the headers."""
import os
import re

import numpy as np
import pytest

import ccd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETA = 0.9

TRI = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])


def _pt(p0, p1, tri0=TRI, tri1=TRI):
    return np.vstack([p0, tri0]), np.vstack([p1, tri1])


# (name, edge-edge?, start [4 x 3], end [4 x 3], exact first crossing time or None)
CASES = [
    ("pt_interior", False, *_pt([0.0, -0.2, 1.0], [0.0, -0.2, -1.0]), 0.5),
    ("pt_edge", False, *_pt([0.0, -1.0, 1.0], [0.0, -1.0, -1.0]), 0.5),
    ("pt_vertex", False, *_pt([1.0, -1.0, 1.0], [1.0, -1.0, -3.0]), 0.25),
    ("pt_triangle_moves", False, *_pt([0.1, 0.0, 0.2], [0.1, 0.0, 0.2], TRI, TRI + [0.0, 0.0, 0.8]), 0.25),
    ("pt_both_move", False, *_pt([0.0, -0.5, 0.3], [0.0, -0.5, -0.3], TRI, TRI + [0.0, 0.0, 0.6]), 0.25),
    ("ee_perpendicular", True, np.array([[-1.0, 0.0, 0.5], [1.0, 0.0, 0.5], [0.0, -1.0, 0.0], [0.0, 1.0, 0.0]]),
     np.array([[-1.0, 0.0, -0.5], [1.0, 0.0, -0.5], [0.0, -1.0, 0.0], [0.0, 1.0, 0.0]]), 0.5),
    ("ee_parallel_overlapping", True, np.array([[-1.0, 0.0, 0.3], [1.0, 0.0, 0.3], [-0.5, 0.0, 0.0], [1.5, 0.0, 0.0]]),
     np.array([[-1.0, 0.0, -0.3], [1.0, 0.0, -0.3], [-0.5, 0.0, 0.0], [1.5, 0.0, 0.0]]), 0.5),
    ("ee_parallel_both_move", True, np.array([[0.0, 0.2, 0.0], [1.0, 0.2, 0.0], [0.5, -0.2, 0.0], [1.5, -0.2, 0.0]]),
     np.array([[0.0, -0.2, 0.0], [1.0, -0.2, 0.0], [0.5, 0.2, 0.0], [1.5, 0.2, 0.0]]), 0.5),
    ("pt_graze_miss", False, *_pt([0.0, -1.5, 1.0], [0.0, -1.5, -1.0]), None),
    ("pt_stops_short", False, *_pt([0.0, 0.0, 1.0], [0.0, 0.0, 0.2]), None),
    ("ee_graze_miss", True, np.array([[-1.0, 0.0, 0.5], [1.0, 0.0, 0.5], [0.0, 0.4, 0.0], [0.0, 1.0, 0.0]]),
     np.array([[-1.0, 0.0, -0.5], [1.0, 0.0, -0.5], [0.0, 0.4, 0.0], [0.0, 1.0, 0.0]]), None),
    ("ee_parallel_miss", True, np.array([[-1.0, 0.0, 0.3], [1.0, 0.0, 0.3], [1.2, 0.0, 0.0], [2.0, 0.0, 0.0]]),
     np.array([[-1.0, 0.0, -0.3], [1.0, 0.0, -0.3], [1.2, 0.0, 0.0], [2.0, 0.0, 0.0]]), None),
]


def _d_at(ee, xa, xb, t):
    return R.distance(ee, [tuple(p) for p in xa + t * (xb - xa)])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_accd_constructed(case):
    name, ee, xa, xb, t_star = case
    xa, xb = np.asarray(xa, float), np.asarray(xb, float)
    r = R.accd(ee, xa, xb, ETA)
    if t_star is None:
        assert r["status"] in ("none", "filtered"), r
        return
    assert r["status"] == "hit", r
    assert 0.0 < r["toi"] <= r["t_stop"] <= t_star, (r, t_star)
    assert _d_at(ee, xa, xb, r["t_stop"]) < (1.0 - ETA) * r["d0"] * (1 + 1e-9), r
    assert r["toi"] > 0.5 * t_star   # (and it gets near: eta = 0.9 leaves a tenth of the gap)


def _random_crossings(rng, n):
    """Point-triangle and edge-edge pairs with known first crossing times: a static primitive, the other one translated through it, everything
    under a common random motion (the relative motion, hence the crossing time, is unchanged)."""
    out = []
    for k in range(n):
        ee = k % 2 == 1
        t_star = rng.uniform(0.05, 0.95)
        common = rng.normal(size=3) * rng.uniform(0.0, 0.5)
        if not ee:
            tri = rng.normal(size=(3, 3))
            w = rng.dirichlet([1.0, 1.0, 1.0]) * 0.9 + 0.1 / 3
            hit = w @ tri
            vel = rng.normal(size=3)
            vel *= rng.uniform(0.2, 2.0) / np.linalg.norm(vel)
            p0 = hit - t_star * vel
            xa = np.vstack([p0, tri])
            xb = np.vstack([p0 + vel, tri])
        else:
            eb = rng.normal(size=(2, 3))
            ea_dir = rng.normal(size=3)
            s, u = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9)
            hit = eb[0] + s * (eb[1] - eb[0])
            L = rng.uniform(0.3, 2.0)
            ea = np.vstack([hit - u * L * ea_dir / np.linalg.norm(ea_dir), hit + (1 - u) * L * ea_dir / np.linalg.norm(ea_dir)])
            vel = rng.normal(size=3)
            vel *= rng.uniform(0.2, 2.0) / np.linalg.norm(vel)
            xa = np.vstack([ea - t_star * vel, eb])
            xb = np.vstack([ea + (1 - t_star) * vel, eb])
        xb = xb + common
        out.append((ee, xa, xb, t_star))
    return out


def test_accd_random_never_passes_the_crossing():
    rng = np.random.default_rng(7)
    hits = 0
    for ee, xa, xb, t_star in _random_crossings(rng, 400):
        r = R.accd(ee, xa, xb, ETA)
        if r["status"] == "touching":
            continue
        assert r["status"] in ("hit", "capped"), r
        assert r["toi"] <= t_star, (r, t_star)
        if r["status"] == "hit":
            hits += 1
            assert r["t_stop"] <= t_star
            assert _d_at(ee, xa, xb, r["t_stop"]) < (1.0 - ETA) * r["d0"] * (1 + 1e-9)
    assert hits > 350


def test_candidates_exclusions():
    # one triangle mesh (2 triangles sharing an edge) falling onto a point: own-triangle points and edges sharing a vertex never pair
    xa = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.3, 0.3, 0.0]])
    xb = xa.copy()
    xb[:4, 2] -= 2.0
    tris = np.array([[0, 1, 2], [1, 3, 2]])
    edges = np.array([[0, 1], [1, 2], [2, 0], [1, 3], [3, 2]])
    pt, ee = R.candidates(xa, xb, tris, edges)
    assert sorted(map(tuple, pt.tolist())) == [(0, 1), (3, 0), (4, 0), (4, 1)]
    assert len(ee) == 0   # (the square's opposite edges sweep apart boxes; adjacent ones share a vertex)
    toi, n = R.max_step(xa, xb, tris, edges)
    assert n == 4 and 0.4 < toi <= 0.5


def test_ccd_symbols_declared():
    decl = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("mistark_contact.h", "mistark_tmcd.h", "mistark_sim.h")}
    assert re.search(r"int mistark_contact_max_step\(mistark_ctx\* ctx, double dt, double conservative_rescaling, double\* max_step, int64_t\* n_candidates\);",
                     decl["mistark_contact.h"])
    assert re.search(r"int mistark_cd_run_ccd\(mistark_cd\* cd, const double\* const\* x1, double conservative_rescaling, double\* toi, int32_t\* n_candidates\);",
                     decl["mistark_tmcd.h"])
    assert "mistark_sim_set_contact_ccd(" in decl["mistark_sim.h"] and "mistark_sim_get_ccd_info(" in decl["mistark_sim.h"]
