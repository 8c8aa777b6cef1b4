"""GPU (-m gpu): user-defined potentials op by op — the device interpreter (k_eval_custom / run_program) and the hipRTC kernels of the emitter
(stark_amd/csrc/custom.hip) on the synthesised programs of tests/custom_cases.py, against `exact(case)`: the same op sequence evaluated per element
in mpmath at 50 digits on second-order Taylor numbers (tests/test_custom_cases_cpu.py proves the cases and the float64 oracle against it on the CPU).

Every case: f, f', f'' of every op of symx::ExprType in and near the edge of its domain, branches whose condition differs between the lanes of a
wavefront (no else, values defined in both arms, Symbol inside an arm, nesting to 3, 31 and 32 = CUSTOM_MAX_DEPTH, conditions +0.0 / -0.0 / a
negative denormal / NaN), register reuse across arms, 256 live temporaries, 600 ops, 16 random programs, strides 1 2 3 9 12, a broadcast binding,
96 inputs on triangles, Zero / One / Print, and a condition program whose inactive elements would evaluate to NaN. Each on 257 elements of a chain
(shared nodes: the gradient scatter accumulates; 257 * 21 lanes cross block boundaries inside an element) and on one element.

Bounds: 8 x the float64 oracle's own error against `exact` for the case's family (tests/custom_tolerances.json, nothing else), floor 8 * 2^-52,
relative to the largest magnitude of the quantity over the case. The factor covers device libm results a few ulp from the host's and FMA
contraction; it is a margin over the reference's rounding, not derived from what the kernels return.

Not compared: POWF at x <= 0 (the device's exp(y ln x) is NaN, and the reference cannot differentiate PowF: no derivative to compare with). LN and
LOG10 of q <= 0 (-inf with zero derivatives) are asserted on the host build of the emitted program (tests/test_custom_cases_cpu.py).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in cc.BASE]
_RESULTS = {}     # (case name, custom_rtc) -> what _run returned: shared by the interpreter-against-emitter test


def _run(case, rtc):
    from stark_amd import capi
    from stark_amd.engine import Engine

    eng = Engine(0)
    x = case.x.copy()
    eng.add_dof_set("x", x)
    a_x = eng.L.mistark_dof_array(eng.h, 0, 3)
    ids = [eng.array(a, a.shape[1]) for a in case.arrays]
    bind = [(a_x if isinstance(a, str) else ids[a], s, c) for a, s, c in case.bindings]
    pid = eng.potential_custom(case.name, case.conn, bind, case.ops, case.consts, case.n_inputs, case.cond_ops, case.cond_consts)
    eng.set_option("custom_rtc", rtc)
    E_h, g_h = eng.eval(capi.EVAL_P_G_H)
    H, rows = eng.element_hessians(pid, case.n_elem)
    Ee = eng.element_energies(pid, case.n_elem)
    E_p, _ = eng.eval(capi.EVAL_P)
    E_g, g_g = eng.eval(capi.EVAL_P_G)
    counters = (eng.counter("rtc_launches"), eng.counter("rtc_builds"))
    eng.close()
    return {"E": (E_p, E_g, E_h), "Ee": Ee, "g": (g_g.copy(), g_h.copy()), "H": H.copy(), "rows": rows.copy(), "counters": counters}


def _check(case, rtc, r):
    ex = cc.exact(case)
    bound = cc.bounds(case, ex)
    assert (r["counters"][0] > 0) == bool(rtc) and r["counters"][1] == rtc, r["counters"]   # the intended path ran: emitted launches of one build, or none
    assert (r["rows"] == case.conn[:, case.dof_cols]).all()
    figures = {"energy": max(abs(E - ex.E) for E in r["E"]), "gradient": max(float(np.abs(g - ex.grad).max()) for g in r["g"]), "hessian": float(np.abs(r["H"] - ex.H).max())}
    print(case.name, "rtc" if rtc else "interpreter", {k: "%.3g of %.3g" % (figures[k], bound[k]) for k in figures})
    assert all(np.isfinite(E) for E in r["E"]) and all(np.isfinite(g).all() for g in r["g"]) and np.isfinite(r["H"]).all()
    for k in figures:
        assert figures[k] <= bound[k], (k, figures[k], bound[k])
    assert (r["H"] == np.transpose(r["H"], (0, 2, 1))).all()                   # symmetric to the bit
    assert np.abs(r["Ee"] - ex.Ee).max() <= bound["energy"]                    # per element too: a wrong arm must not hide in the total
    assert (r["H"][~ex.active] == 0).all() and (r["Ee"][~ex.active] == 0).all()   # an inactive element: zeros, never NaN
    touched = np.zeros(case.x.shape[0], dtype=bool)
    touched[case.conn[ex.active][:, case.dof_cols].reshape(-1)] = True
    for g in r["g"]:
        assert (g.reshape(-1, 3)[~touched] == 0).all()                         # ... and contributes exactly 0.0 to the gradient


@pytest.mark.parametrize("rtc", [0, 1], ids=["interpreter", "rtc"])
@pytest.mark.parametrize("name", NAMES)
def test_custom_potential_equals_the_exact_reference(name, rtc, tmp_path, monkeypatch):
    monkeypatch.setenv("MISTARK_RTC_CACHE", str(tmp_path))   # a build per case, not a stale cache hit (the one-element twin then loads the same code object)
    for case in (cc.CASES[name], cc.CASES[name + ".1"]):
        r = _run(case, rtc)
        _RESULTS[(case.name, rtc)] = r
        _check(case, rtc, r)


@pytest.mark.parametrize("name", NAMES)
def test_interpreter_and_emitted_kernels_agree(name, tmp_path, monkeypatch):
    """Not bit for bit: the compiler may contract the straight-line code differently (tests/test_gpu_custom_rtc.py says so too). Each is within its
    bound of `exact`, so the two are within twice the bound of each other; the tighter single bound is what is asserted."""
    monkeypatch.setenv("MISTARK_RTC_CACHE", str(tmp_path))
    case = cc.CASES[name]
    res = [_RESULTS[(name, rtc)] if (name, rtc) in _RESULTS else _run(case, rtc) for rtc in (0, 1)]
    ex = cc.exact(case)
    bound = cc.bounds(case, ex)
    dE = max(abs(a - b) for a, b in zip(res[0]["E"], res[1]["E"]))
    dH = float(np.abs(res[0]["H"] - res[1]["H"]).max())
    print(name, "energy %.3g of %.3g, hessian %.3g of %.3g" % (dE, bound["energy"], dH, bound["hessian"]))
    assert dE <= bound["energy"] and dH <= bound["hessian"]
