"""CPU: the synthesised contact and friction states of tests/contact_cases.py are proved here, before any kernel is blamed
(tests/test_gpu_contact_synth.py).

 * every labelled state is what it says, measured from its rounded float64 inputs in float64 and in mpmath alike: d / dhat, x / eps_x and u / epsu
   within 1e-9 of the target, the branch taken the same in both, at least 1e-7 away from a threshold, the closest feature the one the potential's
   distance assumes (oracle.contact.point_triangle_type / edge_edge_type), `beyond` with E < 0, the sliding and sticking arms as labelled;
 * the float64 oracle equals `exact` within tests/contact_tolerances.json, and that table is a fresh measurement;
 * all 35 potentials of oracle.energies._CONTACT have cases, with bindings and SymX op arrays from a golden;
 * rows that repeat a state repeat its inputs bit for bit, in both layouts; `shared` has block rows with 257 incident rows;
 * the oracle's Hessian is symmetric, and `exact`'s gradient and Hessian match first and second central differences of the mpmath energy, taken
   in mpmath, along random directions.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_cases as cc  # noqa: E402
from oracle import contact as oc  # noqa: E402
from oracle import energies as en  # noqa: E402

LAYOUTS = ["isolated", "shared"]
mpf = cc.mpf


def _both(name, st):
    return cc.measure(name, st, "mp"), cc.measure(name, st, "float")


def _close(measured, target, tol=1e-9):
    return abs(float(measured) / target - 1.0) <= tol


def test_all_35_potentials_have_cases_with_bindings_and_ops_from_a_golden():
    assert len(cc.NAMES) == 35 and set(cc.NAMES) == set(en._CONTACT)
    assert sum(cc.parse(n)["fam"] == "friction" for n in cc.NAMES) == 14 and sum(cc.parse(n)["fam"] == "ee" for n in cc.NAMES) == 10
    for name in cc.NAMES:
        L = cc.layout(name)
        assert L["golden"] in cc.GOLDENS and {"ops", "opsc"} <= set(L["ops"]) and len(L["ops"]["ops"]) == len(L["ops"]["opsc"]) > 0
        S = cc.bound_schema(name)                                        # (asserts stride, DoF set and column use binding by binding)
        assert sum(s for _, _, _, s, _, _ in S) == L["n_inputs"]
        P = cc.parse(name)
        want = (cc.FRICTION_STATES if P["fam"] == "friction" else cc.BARRIER_STATES + (cc.MOLL_STATES if P["fam"] == "ee" else []))
        rigid = "rb" in (P["A"], P["B"])
        # `spin` needs a rigid side, `corner` a barycentric weight vector: nothing else is left out
        assert cc.labels(name) == [l for l in want if (l != "spin" or rigid) and (l != "corner" or cc.NBARY[P["kind"]])]
        assert len(cc.labels(name)) <= 12


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", [n for n in cc.NAMES if cc.parse(n)["fam"] != "friction"])
def test_barrier_states_are_what_they_say(name, layout):
    P = cc.parse(name)
    for label, st in cc.states(name, layout):
        m, f = _both(name, st)
        target = cc.D_TARGET.get(label, 0.6)
        # float64 loses digits of its own in the point-line distance |ap|^2 - (ap . ab)^2 / |ab|^2 close to the line: 2^-52 |ap|^2 / d^2 per
        # operation (what `near` is for); the state itself is within 1e-9, as the mpmath measurement of the same inputs shows
        lever = 0.0
        if (P["fam"] == "pt" and P["kind"] in ("pe", "ep")) or (P["fam"] == "ee" and P["kind"] in ("pe", "ep")):
            lever = 16 * 2.0 ** -52 * max(cc.DT, 0.6 * 0.13, 0.6 * 0.08) ** 2 / float(m["d"]) ** 2
        assert _close(m["d"] / m["dhat"], target) and _close(f["d"] / f["dhat"], target, max(1e-9, lever)), (label, float(m["d"] / m["dhat"]), f["d"] / f["dhat"])
        E = cc.energy(name, [mpf(c) for c in cc.flat(name, st)])[0]
        assert (E < 0) == (label == "beyond") and E != 0
        if P["fam"] == "ee":
            rm, rf = m["x"] / m["eps_x"], f["x"] / f["eps_x"]
            assert m["mollified"] == f["mollified"] == (label in ("moll_half", "moll_in", "moll_par")), label
            assert abs(float(rm) - 1.0) >= 1e-7 and abs(rf - 1.0) >= 1e-7
            if label in cc.X_TARGET:
                assert _close(rm, cc.X_TARGET[label]) and _close(rf, cc.X_TARGET[label]), (label, float(rm))
            else:
                assert rm > 10
            ea, eb = f["edges"]
            ty = oc.edge_edge_type(*(np.array(p) for p in (ea[0], ea[1], eb[0], eb[1])))
            assert int(ty) == {"pp": oc.EA1_EB0, "pe": oc.EA1_EB, "ee": oc.EA_EB, "ep": oc.EA_EB0}[P["kind"]], (label, int(ty))
            # rest edges of a deformable side are not the current ones: eps_x is no function of the state
            for side, e in ((0, ea), (1, eb)):
                if ("soft", side, 0) in st:
                    rest = np.linalg.norm(np.asarray(st[("soft", side, 0)]["X"]) - np.asarray(st[("soft", side, 1)]["X"]))
                    assert abs(rest / np.linalg.norm(np.array(e[1]) - np.array(e[0])) - 1.0) > 0.1
        else:
            p, prim = np.array(f["point"]), [np.array(q) for q in f["prim"]]
            if len(prim) == 3:
                assert int(oc.point_triangle_type(p, *prim)) == oc.P_T, label
            elif len(prim) == 2:
                s = np.dot(p - prim[0], prim[1] - prim[0]) / np.dot(prim[1] - prim[0], prim[1] - prim[0])
                assert 0.05 < s < 0.95, label
        for side in (0, 1):
            if ("body", side) in st:
                b = st[("body", side)]
                turn = np.linalg.norm(b["bw1"]) * cc.DT
                assert abs(turn - (cc.SPIN if (label == "spin" or layout == "shared") else cc.CALM)) < 1e-12
                assert abs(b["q0"][0]) < 0.999 and abs(np.linalg.norm(b["q0"]) - 1.0) < 1e-12      # a non-identity q0
                ax = b["bw1"] / np.linalg.norm(b["bw1"])
                assert np.abs(ax).max() < 0.999                                                  # a skew axis
                for e, v in st.items():                                                          # x_loc off the axis
                    if e[0] == "rv" and e[1] == side:
                        assert np.linalg.norm(np.cross(ax, v["xloc"])) > 1e-5
        if label == "far" and layout == "isolated":
            pos = np.array(f["edges"][0][0] if P["fam"] == "ee" else f["point"])
            assert np.abs(pos - np.array(cc.FAR)).max() < 5.0
        if label == "aniso" and P["fam"] == "ee":
            la, lb = (np.linalg.norm(np.array(e[1]) - np.array(e[0])) for e in f["edges"])
            assert abs(la / 1e-3 - 1) < 1e-6 and abs(lb / 10.0 - 1) < 1e-6


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", [n for n in cc.NAMES if cc.parse(n)["fam"] == "friction"])
def test_friction_states_are_what_they_say(name, layout):
    seen = set()
    for label, st in cc.states(name, layout):
        m, f = _both(name, st)
        rm, rf = m["u"] / m["epsu"], f["u"] / f["epsu"]
        assert m["stick"] == f["stick"] and abs(float(rm) - 1.0) >= 1e-7 and abs(rf - 1.0) >= 1e-7
        assert m["stick"] == (label in ("stick", "edge_in", "rest", "corner")), label     # slide, fast, edge_out (and spin): the sliding arm
        row = st[("row",)]
        T = np.asarray(row["T"]).reshape(2, 3)
        assert np.abs(T @ T.T - np.eye(2)).max() < 1e-14 and np.abs(T).max() < 0.999 and row["mu"] * row["fn"] > 0
        seen.add((row["mu"], row["fn"]))
        u0 = float(np.hypot(*cc.U_OFF))
        if label == "rest" and layout == "isolated":
            for e, v in st.items():
                if e[0] == "soft":
                    assert (np.asarray(v["v1"]) == 0).all()
                if e[0] == "body":
                    assert (v["bv1"] == 0).all() and (v["bw1"] == 0).all()
            assert f["u"] == u0
        elif label == "rest":
            assert abs(float(m["u"]) / u0 - 1.0) < 1e-5
        else:
            assert _close(rm, cc.U_TARGET[label]) and _close(rf, cc.U_TARGET[label]), (label, float(rm))
        if label == "corner":
            assert (np.asarray(row["bary%d" % cc.NBARY[cc.parse(name)["kind"]]]) == 0).sum() == 1
        for side in (0, 1):
            if ("body", side) in st and not (label == "rest" and layout == "isolated"):
                turn = np.linalg.norm(st[("body", side)]["bw1"]) * cc.DT
                assert abs(turn - (cc.SPIN if (label == "spin" or layout == "shared") else cc.CALM)) < 1e-12
    assert len(seen) == len(cc.labels(name))                                              # mu and fn differ from row to row


_FRESH = {}


def _fresh():
    if not _FRESH:
        _FRESH.update(cc.measure_tolerances())
    return _FRESH


def test_committed_tolerances_are_a_fresh_measurement():
    with open(cc.TOLERANCES) as f:
        committed = json.load(f)
    assert committed == json.loads(json.dumps(_fresh())), "tests/contact_tolerances.json is stale: regenerate it with contact_cases.write_tolerances()"
    kinds = {cc.kind_of(n) for n in cc.NAMES}
    assert kinds == {"pt_soft", "pt_rigid", "ee_soft", "ee_rigid", "friction_soft", "friction_rigid"}
    assert set(committed) == {"%s/%s/%s" % (lay, l, cc.kind_of(n)) for lay in LAYOUTS for n in cc.NAMES for l in cc.labels(n)}


@pytest.mark.parametrize("name", cc.NAMES)
def test_the_oracle_equals_exact_within_the_table_and_is_symmetric(name):
    with open(cc.TOLERANCES) as f:
        tab = json.load(f)
    for lay in LAYOUTS:
        t = cc.Table(name, lay, len(cc.labels(name)))
        ex = t.exact_rows()
        E, g, H, rows = cc.oracle_rows(t)
        assert (rows == t.block_rows()).all()
        assert np.abs(H - np.transpose(H, (0, 2, 1))).max() <= 4 * 2.0 ** -52 * np.abs(H).max()
        for o in (cc.oracle_rows(t), cc.oracle_alt(t)):
            err = cc.row_errors(*o[:3], ex)
            for i, l in enumerate(t.labels):
                for q, e in err.items():
                    assert e[i] <= tab["%s/%s/%s" % (lay, l, cc.kind_of(name))][q], (lay, l, q, e[i])
        b = cc.bounds(t)
        assert all((b[q] >= cc.FLOOR * t.scales()[q]).all() and (b[q] > 0).all() for q in b)


@pytest.mark.parametrize("name", cc.NAMES)
def test_exact_matches_central_differences_taken_in_mpmath(name):
    d, n = cc.in_dof(name)
    for lay in LAYOUTS:
        for i, (label, st) in enumerate(cc.states(name, lay)):
            E0, g, H = cc.exact(name, lay, i)
            x = cc.flat(name, st)
            rng = np.random.default_rng(i)
            with cc.MP.workdps(80):
                for _ in range(2):
                    v = rng.uniform(-1.0, 1.0, n)
                    h = mpf("1e-18")
                    xp = [mpf(c) + h * mpf(float(v[d[k]])) if d[k] >= 0 else mpf(c) for k, c in enumerate(x)]
                    xm = [mpf(c) - h * mpf(float(v[d[k]])) if d[k] >= 0 else mpf(c) for k, c in enumerate(x)]
                    Ep, Em, Ec = cc.exact_energy_mp(name, xp), cc.exact_energy_mp(name, xm), cc.exact_energy_mp(name, [mpf(c) for c in x])
                    d1, d2 = float((Ep - Em) / (2 * h)), float((Ep - 2 * Ec + Em) / (h * h))
                    assert abs(float(Ec) - E0) <= 2.0 ** -52 * abs(E0)
                    assert abs(d1 - g @ v) <= 1e-12 * np.abs(g * v).sum(), (lay, label, d1, g @ v)
                    assert abs(d2 - v @ H @ v) <= 1e-12 * np.abs(H * np.outer(v, v)).sum(), (lay, label, d2, v @ H @ v)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_repeated_rows_repeat_their_inputs_bit_for_bit(name, layout):
    t = cc.Table(name, layout)
    assert t.n_rows == cc.NE == 257
    G = t.gathered()
    n = len(t.labels)
    assert (t.state_of_row == np.arange(cc.NE) % n).all()
    assert (G.view(np.int64) == G[t.state_of_row].view(np.int64)).all()
    for i, (_, st) in enumerate(t.t["states"]):
        assert (G[i].view(np.int64) == np.array(cc.flat(name, st)).view(np.int64)).all()
    rows = t.block_rows()
    counts = np.bincount(rows.reshape(-1), minlength=t.prob.ndofs // 3)
    P = cc.parse(name)
    if layout == "shared":       # one block row per common deformable vertex, two (v1, w1) per common body: each with (at least) 257 incident rows
        want = (1 if "d" in (P["A"], P["B"]) else 0) + 2 * ((P["A"] == "rb") + (P["B"] == "rb"))
        assert (counts >= cc.NE).sum() == want and want >= 1
    else:
        assert counts.max() <= 4 and len(np.unique(rows)) * 1 >= cc.NE     # rows share nothing (an `ee` point and its edge's end are one vertex)
        for r in (0, 100, 256):
            others = np.delete(rows, r, axis=0)
            assert not np.isin(rows[r], others).any()
    if layout == "isolated":
        for k in cc.SMALL:
            ts = cc.Table(name, layout, k)
            assert (ts.gathered().view(np.int64) == G[:k].view(np.int64)).all()


def test_all_tables_in_one_problem_hold_the_same_rows():
    prob, tables = cc.merged_tables("shared", 12)
    assert len(prob.potentials) == 35
    for t in tables:
        one = cc.Table(t.name, "shared", 12)
        assert (t.gathered().view(np.int64) == one.gathered().view(np.int64)).all()
    assert set(cc.custom_ops(tables)) >= {"p%d_ops" % i for i in range(35)}
