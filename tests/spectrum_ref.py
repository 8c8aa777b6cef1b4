"""Reference of the Hessian spectrum report (include/mistark.h "Hessian spectrum report"; record layout: stark_amd/csrc/spectrum_report.hpp), in numpy:
a float64 restatement of the record function (the same pair schedule, stop rule, guard and sweep limit, IEEE division and square root), the bound every
test compares against, and the numpy folds of the nodal and potential stages. Shared by tests/test_spectrum_cpu.py and tests/test_gpu_spectrum.py.

Tolerance (the convention of psd_cases.py): per family of psd_cases.FAMILIES and NB = 1..8
      rounding = 8 x the restatement's largest sorted-eigenvalue error against psd_cases.exact(...).lam, relative to ||H||_F, floor 8 * 2^-52 * 3 NB
in tests/spectrum_tolerances.json, written by write_tolerances() from measure_tolerances() and from nothing else, measured on the CPU. The factor 8 is the
project's margin for device op order and fma contraction. Per element
      b = ||H_in - H_exact||_F + SQRT_OFF_TOL ||H||_F + rounding ||H||_F
bounds every sorted eigenvalue (Weyl: the first term for the input, the second for the stop rule, the third for the rotations' rounding); the count of
eigenvalues below eps lies between #(lam < eps - b) and #(lam < eps + b), and |deficit - exact| <= sqrt(n) b (the deficit is 1-Lipschitz in the vector
of eigenvalues).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psd_cases as pc  # noqa: E402

TOLERANCES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "spectrum_tolerances.json")
SPEC_REC, SPEC_NODAL, SPEC_POT = 10, 5, 10
APQ_GUARD = 1e-300
F_PROJECTED, F_NON_FINITE, F_NOT_CONVERGED = 1, 2, 4


def fro(M):
    return np.sqrt((M * M).sum(axis=(1, 2)))


def sort_by_rank(lam):
    """ascending, ties in index order (a stable sort is rank counting with ties broken by index; -0.0 == +0.0 keep their order)"""
    idx = np.argsort(lam, axis=1, kind="stable")
    return np.take_along_axis(lam, idx, axis=1)


def finish(lam, eps, fro2, trace, sweeps, off, converged, finite):
    """records [ne, 10] from eigenvalues in index order"""
    ne, n = lam.shape
    rec = np.zeros((ne, SPEC_REC))
    below = lam < eps
    rec[:, 0] = lam.min(axis=1)
    rec[:, 1] = lam.max(axis=1)
    rec[:, 2] = below.sum(axis=1)
    rec[:, 3] = (lam < 0.0).sum(axis=1)
    d2 = np.zeros(ne)
    for k in range(n):                                   # (index order, as the header)
        d2 = d2 + np.where(below[:, k], (eps - lam[:, k]) ** 2, 0.0)
    rec[:, 4] = np.sqrt(d2)
    rec[:, 5] = np.sqrt(fro2)
    rec[:, 6] = trace
    rec[:, 7] = sweeps
    rec[:, 8] = np.sqrt(off)
    rec[:, 9] = np.where(below.any(axis=1), 1.0, 0.0) + np.where(converged, 0.0, 4.0)
    rec[~finite] = 0.0
    rec[~finite, 9] = 2.0
    return rec


def restatement(H, eps=pc.EPS):
    """(records [ne, 10], sorted spectrum [ne, n], final matrices [ne, n, n]) of float64 matrices [ne, n, n]: spectrum_record<n> in numpy"""
    H = np.asarray(H, dtype=np.float64)
    ne, n, _ = H.shape
    m = (n + 1) & ~1
    finite = np.isfinite(H).all(axis=(1, 2))
    A = np.where(finite[:, None, None], H, 0.0).copy()
    with np.errstate(all="ignore"):
        fro2 = np.zeros(ne)
        trace = np.zeros(ne)
        for c in range(n):                               # column by column, columns in order
            s = np.zeros(ne)
            for i in range(n):
                s = s + H[:, i, c] * H[:, i, c]
            fro2 = fro2 + s
            trace = trace + H[:, c, c]

        def off2(A):
            t = np.zeros(ne)
            for c in range(n):
                s = np.zeros(ne)
                for i in range(n):
                    if i != c:
                        s = s + A[:, i, c] * A[:, i, c]
                t = t + s
            return t

        active = finite.copy()
        converged = np.zeros(ne, dtype=bool)
        sweeps = np.zeros(ne, dtype=int)
        off_stop = np.zeros(ne)
        for sweep in range(pc.MAX_SWEEPS + 1):
            off = off2(A)
            off_stop[active] = off[active]
            done = active & (off <= pc.JACOBI_OFF_TOL * fro2)
            converged |= done
            active &= ~done
            if sweep == pc.MAX_SWEEPS:
                active[:] = False
            if not active.any():
                break
            sweeps[active] += 1
            for r in range(m - 1):
                for p, q in sorted(pc.round_pairs(n, r)):
                    apq = A[:, p, q]
                    rot = active & (np.abs(apq) > APQ_GUARD)
                    if not rot.any():
                        continue
                    theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                    t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    cs = np.where(rot, 1.0 / np.sqrt(t * t + 1.0), 1.0)
                    sn = np.where(rot, t * cs, 0.0)
                    x, y = A[:, :, p].copy(), A[:, :, q].copy()
                    A[:, :, p] = np.where(rot[:, None], cs[:, None] * x - sn[:, None] * y, x)
                    A[:, :, q] = np.where(rot[:, None], sn[:, None] * x + cs[:, None] * y, y)
                    x, y = A[:, p, :].copy(), A[:, q, :].copy()
                    A[:, p, :] = np.where(rot[:, None], cs[:, None] * x - sn[:, None] * y, x)
                    A[:, q, :] = np.where(rot[:, None], sn[:, None] * x + cs[:, None] * y, y)
        lam = np.einsum("eii->ei", A).copy()
        rec = finish(lam, eps, fro2, trace, sweeps, off_stop, converged, finite)
    spec = sort_by_rank(lam)
    spec[~finite] = 0.0
    return rec, spec, A


# ======================================================================================================================================
# tolerances and the bound
# ======================================================================================================================================
def floor(nb):
    return 8.0 * 2.0 ** -52 * 3 * nb


def restatement_error(family, nb):
    """the restatement's largest sorted-eigenvalue error against the exact spectrum over the family's elements, relative to ||H||_F"""
    ex = pc.exact(family, nb)
    _, spec, _ = restatement(ex.H, pc.EPS)
    err = np.abs(spec - np.sort(ex.lam, axis=1)).max(axis=1)
    return float(pc._rel(err, ex.fro).max())


def measure_tolerances():
    """family -> NB -> rounding"""
    return {fam: {str(nb): max(8.0 * restatement_error(fam, nb), floor(nb)) for nb in pc.NBS} for fam in pc.FAMILIES}


def write_tolerances(path=TOLERANCES):
    """Regenerates tests/spectrum_tolerances.json:  python -c "import spectrum_ref as s; s.write_tolerances()"  from tests/ (repository root on PYTHONPATH)."""
    with open(path, "w") as f:
        json.dump(measure_tolerances(), f, indent=1, sort_keys=True)
        f.write("\n")


_TABLE = {}


def _table():
    if not _TABLE:
        with open(TOLERANCES) as f:
            _TABLE.update(json.load(f))
    return _TABLE


def rounding(family, nb):
    return _table()[family][str(nb)]


def rounding_largest(nb):
    """the largest entry of that NB: for Hessians of no synthesised family (the built-in potentials)"""
    return max(t[str(nb)] for t in _table().values())


def bound(rnd, fro_, h_in_err):
    """per element: ||H_in - H_exact||_F + (SQRT_OFF_TOL + rounding) ||H||_F"""
    return np.asarray(h_in_err) + (pc.SQRT_OFF_TOL + rnd) * np.asarray(fro_)


def exact_figures(lam, eps=pc.EPS):
    """(sorted eigenvalues, deficit) of exact eigenvalues [ne, n]"""
    s = np.sort(lam, axis=1)
    return s, np.sqrt((np.where(s < eps, eps - s, 0.0) ** 2).sum(axis=1))


def check_records(tag, rec, spec, lam_exact, b, eps=pc.EPS, show=print):
    """the derived checks of one potential's records against exact eigenvalues [ne, n] and the per-element bound b [ne]; prints each figure first"""
    ne, n = lam_exact.shape
    s, deficit = exact_figures(lam_exact, eps)
    flags = rec[:, 9].astype(int)
    err = np.abs(spec - s).max(axis=1)
    k = int(np.argmax(err - b))
    show("%s |lambda - exact| %.3g of %.3g; sweeps <= %d; sqrt(off) <= %.3g" % (tag, err[k], b[k], int(rec[:, 7].max()), rec[:, 8].max()))
    assert (flags & (F_NON_FINITE | F_NOT_CONVERGED) == 0).all(), tag
    assert (err <= b).all(), (tag, k, err[k], b[k])
    assert (np.diff(spec, axis=1) >= 0).all(), tag
    assert (rec[:, 0] == spec[:, 0]).all() and (rec[:, 1] == spec[:, -1]).all(), tag
    lo_cnt, hi_cnt = (s < (eps - b)[:, None]).sum(axis=1), (s < (eps + b)[:, None]).sum(axis=1)
    assert ((rec[:, 2] >= lo_cnt) & (rec[:, 2] <= hi_cnt)).all(), tag
    lo_neg, hi_neg = (s < -b[:, None]).sum(axis=1), (s < b[:, None]).sum(axis=1)
    assert ((rec[:, 3] >= lo_neg) & (rec[:, 3] <= hi_neg)).all(), tag
    assert (rec[:, 2] == (spec < eps).sum(axis=1)).all() and (rec[:, 3] == (spec < 0.0).sum(axis=1)).all(), tag
    derr = np.abs(rec[:, 4] - deficit)
    db = np.sqrt(n) * b + (n + 2) * 2.0 ** -52 * deficit     # (+ the sum's own rounding: n squares and additions and one root, in two orders)
    k = int(np.argmax(derr - db))
    show("%s |deficit - exact| %.3g of %.3g" % (tag, derr[k], db[k]))
    assert (derr <= db).all(), (tag, k, derr[k])
    assert ((flags & F_PROJECTED) == (rec[:, 2] > 0)).all(), tag
    assert (rec[:, 7] <= pc.MAX_SWEEPS).all() and (rec[:, 8] <= pc.SQRT_OFF_TOL * rec[:, 5] * (1 + 4 * 2.0 ** -52)).all(), tag


# ======================================================================================================================================
# numpy folds of the nodal and potential stages
# ======================================================================================================================================
def nodal_fold(nbr, pots):
    """pots: list of (potential id, records [ne, 10], block rows [ne, NB]) in list order. Returns (out [nbr, 5], abs sums [nbr]) — field 3 is a sum."""
    out = np.zeros((nbr, SPEC_NODAL))
    out[:, 4] = -1.0
    mn = np.full(nbr, np.inf)
    asum = np.zeros(nbr)
    nb_max = max(r.shape[1] for _, _, r in pots)
    # contribution order of a row: potential by potential, block by block, element by element (g = g_off + block * n_elem + element)
    for pid, rec, rows in pots:
        flags = rec[:, 9].astype(int)
        for b in range(rows.shape[1]):
            for e in range(len(rec)):
                r = rows[e, b]
                out[r, 0] += 1
                out[r, 1] += flags[e] & 1
                out[r, 3] += rec[e, 4] ** 2
                asum[r] += rec[e, 4] ** 2
                if not (flags[e] & 2) and rec[e, 0] < mn[r]:
                    mn[r] = rec[e, 0]
                    out[r, 4] = pid
    del nb_max
    out[:, 2] = np.where(np.isfinite(mn), mn, 0.0)
    return out, asum


def potential_fold(rec):
    """(record [10], sum of deficit^2) of one potential's element records"""
    o = np.zeros(SPEC_POT)
    o[6] = o[9] = -1.0
    if len(rec) == 0:
        return o, 0.0
    flags = rec[:, 9].astype(int)
    fin = (flags & 2) == 0
    o[0] = len(rec)
    o[1] = (flags & 1).sum()
    o[2] = (fin & (rec[:, 0] < 0.0)).sum()
    o[3] = (~fin).sum()
    o[4] = ((flags & 4) != 0).sum()
    if fin.any():
        lo = np.where(fin, rec[:, 0], np.inf)
        o[5] = lo.min()
        o[6] = int(np.argmax(lo == lo.min()))
        o[7] = np.where(fin, rec[:, 1], -np.inf).max()
    d2 = float((rec[:, 4] ** 2).sum())
    o[8] = np.sqrt(d2)
    if (~fin).any():
        o[9] = int(np.argmax(~fin))
    return o, d2
