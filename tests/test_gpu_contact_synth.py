"""GPU (-m gpu): the 21 barrier and 14 friction potentials on the synthesised branch states of tests/contact_cases.py, against `exact`: the potential
restated on second-order Taylor numbers over mpmath at 40 digits (tests/test_contact_cases_cpu.py proves the states, the float64 oracle and the
tolerance table against it on the CPU).

States (per potential, one row each, then repeated cyclically to 257 rows: the one-lane-per-contact kernel crosses its 256-lane block): the gap at
0.6, 1e-3, 1 - 1e-6 and 1.5 of dhat, translated by kilometres, primitives of 1e-3 m against 10 m, rigid sides turning by 1.2 rad in the step; the
edge-edge mollifier at 0.5, 1 -+ 1e-6 and 1e-6 of eps_x; friction sticking, sliding, at 1 -+ 1e-6 of epsu, at rest, at 1e4 epsu, with a zero
barycentric weight. Layouts: `isolated` (every row its own vertices and bodies), `shared` (one body per rigid side and one deformable vertex for
the whole table: block rows with 257 incident rows, summed by k_grad_gather_long), and the first 1 and 7 rows of `isolated`.

Variants, and the kernel each reaches:
  closed          contact_closed_min_lanes = 0: k_eval_contact_closed<En, false / true> (contact_closed.hpp), k_eval_p / k_eval_p_multi for EVAL_P
  generic         generic_contact, no_multi_eval_pgh, no_multi_eval_p: k_eval_pgh<En, false / true>, k_eval_p
  generic_shared  generic_contact, all 35 tables in one engine, routed to the dynamic part: the one launch of k_eval_pgh_multi (counter multi_pgh_launches)
  interpreter     potential_custom with the golden's SymX op arrays, custom_rtc = 0: k_eval_custom / run_program (custom.hip)

Bounds: 8 x the float64 oracle's own error against `exact` for the row's (layout, state, kind) — tests/contact_tolerances.json, nothing else — floor
8 * 2^-52, relative to the row's largest exact entry of the quantity. A gradient entry that several rows add to is allowed the sum of their bounds.
`generic_shared` is held to the bits of `generic`: both run eval_pgh_body<En, true>, the same per-lane arithmetic, and sum nothing across lanes in
what is compared (element energies and Hessians).
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ["isolated", "shared"]
VARIANTS = ["closed", "generic", "interpreter"]
_TABLES, _RESULTS, _MERGED = {}, {}, {}


def table(name, layout, n_rows=cc.NE):
    key = (name, layout, n_rows)
    if key not in _TABLES:
        _TABLES[key] = cc.Table(name, layout, n_rows)
    return _TABLES[key]


def _evaluate(prob, tables, variant):
    """one engine over `prob`; per table what the device returned"""
    from gpu_util import engine_from_problem
    from stark_amd import capi

    eng = engine_from_problem(prob, None, custom_ops=cc.custom_ops(tables) if variant == "interpreter" else None)
    assert eng.ndofs == prob.ndofs
    if variant == "closed":
        eng.set_option("contact_closed_min_lanes", 0)
    elif variant == "generic":
        for o in ("generic_contact", "no_multi_eval_pgh", "no_multi_eval_p"):
            eng.set_option(o, 1)
    elif variant == "generic_shared":
        eng.set_option("generic_contact", 1)
        for pid in eng.pot_ids.values():
            eng.set_dynamic(pid, True)
    else:
        eng.set_option("custom_rtc", 0)
    E_h, g_h = eng.eval(capi.EVAL_P_G_H)
    out = []
    for t in tables:
        pid = eng.pot_ids[t.t["index"]]
        H, rows = eng.element_hessians(pid, t.n_rows)
        out.append({"H": H.copy(), "rows": rows.copy(), "Ee": eng.element_energies(pid, t.n_rows).copy()})
    E_p, _ = eng.eval(capi.EVAL_P)
    E_g, g_g = eng.eval(capi.EVAL_P_G)
    multi, rtc = eng.counter("multi_pgh_launches"), eng.counter("rtc_launches")
    eng.close()
    assert rtc == 0                                                      # no emitted kernel in any variant
    assert (multi > 0) == (variant == "generic_shared"), (variant, multi)   # the shared launch ran where it is under test, and nowhere else
    for r in out:
        r.update(E=(E_p, E_g, E_h), g=(g_g.copy(), g_h.copy()))
    return out


def run(name, layout, variant, n_rows=cc.NE):
    key = (name, layout, variant, n_rows)
    if key not in _RESULTS:
        t = table(name, layout, n_rows)
        _RESULTS[key] = _evaluate(t.prob, [t], variant)[0]
    return _RESULTS[key]


def run_merged(layout):
    if layout not in _MERGED:
        prob, tables = cc.merged_tables(layout)
        _MERGED[layout] = (tables, _evaluate(prob, tables, "generic_shared"))
    return _MERGED[layout]


def check_against_exact(t, r, variant, with_totals=True):
    Ee, ge, He = t.exact_rows()
    b = cc.bounds(t)
    rows = t.block_rows()
    assert (r["rows"] == rows).all()
    assert np.isfinite(r["Ee"]).all() and np.isfinite(r["H"]).all() and all(np.isfinite(g).all() for g in r["g"])
    fE = np.abs(r["Ee"] - Ee) / b["energy"]
    fH = np.abs(r["H"] - He).max(axis=(1, 2)) / b["hessian"]
    fS = np.abs(r["H"] - np.transpose(r["H"], (0, 2, 1))).max(axis=(1, 2)) / (2.0 * b["hessian"])
    # the gradient: scatter-add of the exact element gradients; an entry is allowed the sum of the bounds of the rows that add to it
    idx = (3 * rows[:, :, None] + np.arange(3)[None, None, :]).reshape(t.n_rows, -1)
    g_ref, g_tol = np.zeros(t.prob.ndofs), np.zeros(t.prob.ndofs)
    np.add.at(g_ref, idx.reshape(-1), ge.reshape(-1))
    np.add.at(g_tol, idx.reshape(-1), np.repeat(b["gradient"], idx.shape[1]))
    touched = g_tol > 0
    fG = np.zeros(t.prob.ndofs)
    for g in r["g"]:                                                      # EVAL_P_G and EVAL_P_G_H, each against exact
        fG[touched] = np.maximum(fG[touched], np.abs(g - g_ref)[touched] / g_tol[touched])
    worst = lambda f: "%s %.3g" % (t.labels[t.state_of_row[int(np.argmax(f))]], float(f.max()))
    row_of = np.zeros(t.prob.ndofs, dtype=np.int64)
    row_of[idx.reshape(-1)] = np.repeat(np.arange(t.n_rows), idx.shape[1])
    print("%s %s %s rows=%d |.-exact| of bound: energy %s, hessian %s, gradient %s %.3g, asymmetry %s" % (
        t.name, t.layout, variant, t.n_rows, worst(fE), worst(fH), t.labels[t.state_of_row[row_of[int(np.argmax(fG))]]], float(fG.max()), worst(fS)))
    assert fE.max() <= 1.0 and fH.max() <= 1.0 and fG.max() <= 1.0
    if variant == "closed":
        assert fS.max() <= 1.0
    assert (r["g"][0][~touched] == 0).all() and (r["g"][1][~touched] == 0).all()
    if with_totals:
        total, allowed = math.fsum(Ee.tolist()), float(b["energy"].sum())
        for E in r["E"]:                                                  # EVAL_P, EVAL_P_G, EVAL_P_G_H
            assert abs(E - total) <= allowed, (E, total, allowed)
    # position independence: a repeated row has the bits of its first occurrence
    first = t.state_of_row
    assert (r["Ee"].view(np.int64) == r["Ee"][first].view(np.int64)).all()
    assert (r["H"].view(np.int64) == r["H"][first].view(np.int64)).all()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_contact_kernel_equals_the_exact_reference(name, layout, variant):
    t = table(name, layout)
    r = run(name, layout, variant)
    check_against_exact(t, r, variant)
    if layout == "isolated":      # the tables of 1 and 7 rows: the bits of the same rows in the table of 257
        for n in cc.SMALL:
            ts, rs = table(name, layout, n), run(name, layout, variant, n)
            check_against_exact(ts, rs, variant)
            assert (rs["Ee"].view(np.int64) == r["Ee"][:n].view(np.int64)).all() and (rs["H"].view(np.int64) == r["H"][:n].view(np.int64)).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_shared_launch_equals_the_exact_reference_and_the_generic_kernel(name, layout):
    tables, results = run_merged(layout)
    i = cc.NAMES.index(name)
    t, r = tables[i], results[i]
    # (the totals and the gradient are the sums over all 35 tables there; the gradient is compared for the table's own rows only where no other
    # table adds to them, which is every row: the tables share arrays, not vertices)
    Ee, ge, He = t.exact_rows()
    b = cc.bounds(t)
    rows = t.block_rows()
    assert (r["rows"] == rows).all()
    fE, fH = np.abs(r["Ee"] - Ee) / b["energy"], np.abs(r["H"] - He).max(axis=(1, 2)) / b["hessian"]
    idx = (3 * rows[:, :, None] + np.arange(3)[None, None, :]).reshape(t.n_rows, -1)
    g_ref, g_tol = np.zeros(t.prob.ndofs), np.zeros(t.prob.ndofs)
    np.add.at(g_ref, idx.reshape(-1), ge.reshape(-1))
    np.add.at(g_tol, idx.reshape(-1), np.repeat(b["gradient"], idx.shape[1]))
    own = g_tol > 0
    fG = np.maximum(np.abs(r["g"][0] - g_ref)[own], np.abs(r["g"][1] - g_ref)[own]) / g_tol[own]
    print("%s %s generic_shared |.-exact| of bound: energy %.3g, hessian %.3g, gradient %.3g" % (name, layout, fE.max(), fH.max(), fG.max()))
    assert fE.max() <= 1.0 and fH.max() <= 1.0 and fG.max() <= 1.0
    if i == 0:
        total = math.fsum(x for tt in tables for x in tt.exact_rows()[0].tolist())
        allowed = sum(float(cc.bounds(tt)["energy"].sum()) for tt in tables)
        for E in r["E"]:
            assert abs(E - total) <= allowed, (E, total, allowed)
    one = run(name, layout, "generic")
    assert (r["Ee"].view(np.int64) == one["Ee"].view(np.int64)).all() and (r["H"].view(np.int64) == one["H"].view(np.int64)).all()


@pytest.mark.parametrize("name", cc.NAMES)
def test_closed_form_equals_the_generic_kernel_on_the_well_conditioned_states(name):
    """contact_closed.hpp's claim (1e-11 of the largest entry), on `mid` and on both friction arms; the ill-conditioned states are held to `exact` alone."""
    t = table(name, "isolated")
    a, b = run(name, "isolated", "closed"), run(name, "isolated", "generic")
    for i, l in enumerate(t.labels):
        if l in ("mid", "stick", "slide"):
            dH = np.abs(a["H"][i] - b["H"][i]).max() / np.abs(b["H"][i]).max()
            dE = abs(a["Ee"][i] - b["Ee"][i]) / abs(b["Ee"][i])
            print(name, l, "closed - generic: energy %.3g, hessian %.3g of the largest entry" % (dE, dH))
            assert dH < 1e-11 and dE < 1e-11


@pytest.mark.parametrize("variant", VARIANTS + ["generic_shared"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_eval_p_g_and_eval_p_g_h_give_the_same_gradient_bits(name, layout, variant):
    """Two defects of reproducibility showed here first (contact kernel tests), each with gradients well inside their bound of `exact`:
      * generic / generic_shared, the potentials with a point-line or line-line distance (pt_pe, pt_ep, ee_pe, ee_ep, ee_ee): EVAL_P_G ran
        k_eval_pgh<En, false>, another instantiation of eval_pgh_body than EVAL_P_G_H's; the two differed in up to 1303 of 3084 entries, by up to
        7.0e4 ulp of the entry on `near` / `beyond` (where |ap|^2 - (ap . ab)^2 / |ab|^2 cancels), at most 0.014 of the entry's bound. EVAL_P_G now
        runs k_eval_pgh<En, true> without a Hessian pool for these tables.
      * interpreter, `shared`: a user-defined potential added its node gradients with atomics in arrival order, so a row with 257 incident rows
        differed by up to 7 ulp even between two EVAL_P_G calls. Its kernels now write to the gradient pool, summed in list order."""
    if variant == "generic_shared":
        tables, results = run_merged(layout)
        i = cc.NAMES.index(name)
        t, r = tables[i], results[i]
    else:
        t, r = table(name, layout), run(name, layout, variant)
    own = np.zeros(t.prob.ndofs, dtype=bool)
    own[(3 * t.block_rows()[:, :, None] + np.arange(3)[None, None, :]).reshape(-1)] = True
    a, b = r["g"][0][own], r["g"][1][own]
    d = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        ulp = np.where(d > 0, d / np.spacing(np.maximum(np.abs(a), np.abs(b))), 0.0)
    print("%s %s %s EVAL_P_G - EVAL_P_G_H: %d of %d entries differ, by up to %.1f ulp" % (name, layout, variant, int((d > 0).sum()), int(own.sum()), float(ulp.max())))
    assert (a.view(np.int64) == b.view(np.int64)).all()
