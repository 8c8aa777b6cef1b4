"""Synthesised element Hessians with KNOWN spectra for the PSD projection (stark_amd/csrc/project.hip), and their exact projections — shared by
tests/test_psd_cases_cpu.py (the cases and references are proved there, no device) and tests/test_gpu_psd_synth.py (the kernels against them).

Pure numpy + mpmath. Two user potentials, written as op sequences for the device interpreter (custom_rtc = 0) with custom_cases.Prog:

  SynthSpectral<NB>:  E = 1/2 sum_k lambda_k (q_k . u)^2      u = the element's 3 NB DoFs, lambda = 3 NB per-element inputs,
                      Q = [q_k] = H1 H2, two Householder reflections y = u - 2 v (v . u) / (v . v) of small integer vectors written into the
                      program: the element Hessian is Q diag(lambda) Q^T whatever the state, its spectrum is lambda without any eigen-solver.
  SynthDiag<NB>:      E = 1/2 sum_i d_i u_i^2 + oa u_0 u_1 + ob u_1 u_2      d, oa, ob per-element inputs. With oa = ob = 0 the Hessian is
                      diag(d) to the bit (d_i * 1 + 0); oa, ob place single off-diagonal entries (the guards of the rotation).

Every element owns its own NB nodes, so any subset of elements is selected by activating its nodes, and lists of any exact length exist.

Spectrum families (FAMILIES; eps = 1e-10; all values small dyadic numbers except the ones made of eps itself). In every family whose own
spectrum has an eigenvalue below eps the ODD elements carry an all-positive variant, so changed and unchanged elements alternate inside a wavefront:
  positive, mixed, one_negative, rank_one_negative (the rest exactly 0), zero, repeated (triples (2, 2, 2 | -1, -1, -1 | ...); NB = 1: (2, 2, -1)),
  range (2^39 .. -2^13 .. 2^-10: fifteen decades; -2^13 is what 1e3 bounds of a matrix of norm 2^39 leave room for), near_eps (3 eps / -eps beside 1/64 and 1/512),
  s2_big (oa = 1e-290 (d_1 - d_0): theta^2 overflows, the `s2 < 1e300` branch), tiny_off (oa = 1e-305, below the `fabs(apq) > 1e-300` guard) — both
  with ob = O(1) on half of the elements so that sweeps do run —, at_eps (entries exactly eps: NOT clamped, nothing counts as changed),
  below_eps (nextafter(eps, 0): clamped), zeros_denormal (+0.0, -0.0, -5e-324).

Exact reference: `exact(family, nb)` = H_exact = Q diag(lambda) Q^T and its projection Q diag(f(lambda)) Q^T in mpmath at 40 digits, rounded once to
float64; f is the reference's rule (project_to_PD.cpp:22-27): lambda < eps ? (mirroring ? -lambda : eps) : lambda. An element without an
eigenvalue below eps is returned untouched. `project_readback` does the same for a float64 matrix read back from the device, through mpmath.eigsy.

The bound (tests/test_gpu_psd_synth.py states the argument): per element
      ||H_in - H_exact||_F  +  sqrt(JACOBI_OFF_TOL) ||H||_F  +  rounding ||H||_F,
rounding = 8 x the error of `restatement` (a float64 numpy restatement of the kernels' Jacobi: same pair schedule, same stop rule, 30 sweeps)
against the exact projection, per family and NB, relative to ||H||_F, floor 8 * 2^-52 * 3 NB — tests/psd_tolerances.json, written by
write_tolerances() from measure_tolerances() and from nothing else.

Decision margin (asserted by margins_hold): for every element of the spectral families and of s2_big / tiny_off either some exact eigenvalue is
<= eps - 1e3 bound or all are >= eps + 1e3 bound, so changed / unchanged is never a matter of rounding. (Demanding that distance of EVERY
eigenvalue is not possible for the spectra themselves: the exact zeros of rank_one_negative sit 1e-10 from eps beside an eigenvalue of order 1,
2^-10 of `range` sits beside 2^39. What the count needs is the element's decision, and that is what is asserted. near_eps keeps its large
eigenvalues at 1/64 and 1/512 for this reason: 3 eps and -eps are 2e-10 from eps, and 1e3 bounds of a matrix of norm 1/64 are 1.5e-10; they are
still 1.5e8 times the eigenvalues they sit beside.)
"""
from __future__ import annotations

import json
import os
import re
import sys
from dataclasses import dataclass

import mpmath
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_cases as cc  # noqa: E402

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stark_amd", "csrc")
TOLERANCES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "psd_tolerances.json")

MP = mpmath.mp.clone()
MP.dps = 40

EPS = 1e-10
MARGIN = 1e3


# thresholds of the engine, read from its sources' text (as linsys_cases._constants does): a moved threshold moves the cases with it
def _constant(fname, name, pattern=r"([0-9][0-9.eE+-]*)"):
    with open(os.path.join(_CSRC, fname)) as f:
        text = f.read()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*%s\s*;" % (name, pattern), text)
    assert m, "%s: no constexpr %s" % (fname, name)
    return m.group(1)


SHORT_LIST = int(_constant("project.hip", "SHORT_LIST"))
PROJ_BATCH = int(_constant("project.hip", "PROJ_BATCH"))
MARK_BATCH = int(_constant("project.hip", "MARK_BATCH"))
JACOBI_OFF_TOL = float(_constant("kernels_common.hpp", "JACOBI_OFF_TOL"))
SQRT_OFF_TOL = float(np.sqrt(JACOBI_OFF_TOL))
with open(os.path.join(_CSRC, "project.hip")) as _f:           # ProjWaveShared: W = m = even(3 NB), EPW = 64 / W — epw() below restates exactly this line
    assert re.search(r"n = 3 \* NB, m = \(n \+ 1\) & ~1, W = m, EPW = 64 / W;", _f.read()), "project.hip: the elements-per-wavefront rule moved"
MAX_SWEEPS = 30
NBS = list(range(1, 9))


def epw(nb):
    """elements per wavefront of the register-resident kernel: 64 / even(3 NB)"""
    return 64 // ((3 * nb + 1) & ~1)


def n_elem_default(nb):
    return 4 * epw(nb) + 1


SPECTRAL = ["positive", "mixed", "one_negative", "rank_one_negative", "zero", "repeated", "range", "near_eps"]
DIAG = ["s2_big", "tiny_off", "at_eps", "below_eps", "zeros_denormal"]
FAMILIES = SPECTRAL + DIAG
MARGIN_FAMILIES = SPECTRAL + ["s2_big", "tiny_off"]
EPS_BELOW = float(np.nextafter(EPS, 0.0))
DENORMAL = -5e-324


# ======================================================================================================================================
# spectra
# ======================================================================================================================================
def _pos(n):
    return (np.arange(n) + 2) / 4.0               # 0.5, 0.75, ...: distinct


def _scale(e):
    return 2.0 ** (e % 3 - 1)


def spectrum(family, nb, ne):
    """lambda [ne, 3 nb] of a spectral family"""
    n = 3 * nb
    k = np.arange(n)
    lam = np.zeros((ne, n))
    for e in range(ne):
        odd = e % 2 == 1
        pos = np.roll(_pos(n), e) * _scale(e)
        if family == "positive":
            l = pos
        elif family == "mixed":
            l = pos if odd else pos * np.where(k % 2 == 0, -1.0, 1.0)
        elif family == "one_negative":
            l = pos.copy()
            if not odd:
                l[e % n] = -1.25 * _scale(e)
        elif family == "rank_one_negative":
            l = pos
            if not odd:
                l = np.zeros(n)
                l[e % n] = -(1 + e % 4) / 2.0
        elif family == "zero":
            l = pos if odd else np.zeros(n)
        elif family == "repeated":
            base = np.array([2.0, 2.0, -1.0]) if n == 3 else np.array([2.0, -1.0, 0.5, 3.0])[(k // 3) % 4]
            l = np.roll(base, e) * _scale(e)
            if odd:
                l = np.abs(l)
        elif family == "range":
            if odd:
                l = np.concatenate([[2.0 ** 39, 2.0 ** 13], 2.0 ** (36 - np.arange(n - 2))])
            else:
                l = np.concatenate([[2.0 ** 39, -2.0 ** 13, 2.0 ** -10], 2.0 ** (36 - 2 * np.arange(n - 3))])
            l = np.roll(l, e)
        elif family == "near_eps":
            l = np.full(n, 3 * EPS)
            l[0] = 1.0 / 64
            l[3::3] = 1.0 / 512
            l[1] = 3 * EPS if odd else -EPS
            l = np.roll(l, e)
        else:
            raise KeyError(family)
        lam[e] = l
    return lam


def diag_inputs(family, nb, ne):
    """(d [ne, 3 nb], o [ne, 2]) of a SynthDiag family"""
    n = 3 * nb
    d = np.zeros((ne, n))
    o = np.zeros((ne, 2))
    for e in range(ne):
        odd = e % 2 == 1
        pos = np.roll(_pos(n), e) * _scale(e)
        de = pos.copy()
        if family in ("s2_big", "tiny_off"):
            if not odd:
                de[n - 1] = -0.75 * _scale(e)
            o[e, 0] = 1e-290 * (de[1] - de[0]) if family == "s2_big" else (1e-305 if e % 4 < 2 else -1e-305)
            o[e, 1] = 0.375 * _scale(e) if e % 4 < 2 else 0.0
        elif family == "at_eps":
            if e % 3 == 0:
                de[:] = EPS
            de[e % n] = EPS
        elif family == "below_eps":
            if e % 4 == 0:
                de[:] = EPS
            de[e % n] = EPS if odd else EPS_BELOW
        elif family == "zeros_denormal":
            if not odd:
                de[:3] = [0.0, -0.0, DENORMAL]
                de = np.roll(de, e)
        else:
            raise KeyError(family)
        d[e] = de
    return d, o


# ======================================================================================================================================
# the programs
# ======================================================================================================================================
def householder_vectors(n):
    """two small integer vectors, dense, not parallel"""
    i = np.arange(n)
    return 1 + i % 3, np.where(i % 2 == 0, 1, -1) * (1 + (i * i + 1) % 4)


def spectral_program(nb):
    """inputs: u 0 .. n-1 (DoFs), lambda n .. 2n-1"""
    n = 3 * nb
    p = cc.Prog(2 * n)
    y = list(range(n))
    for v in householder_vectors(n):
        cst = {int(c): p.const(float(c)) for c in sorted(set(np.abs(v).tolist())) if c != 1}
        term = lambda i: y[i] if abs(v[i]) == 1 else p.mul(cst[abs(int(v[i]))], y[i])
        dot = None
        for i in range(n):
            t = term(i)
            dot = t if dot is None else (p.add(dot, t) if v[i] > 0 else p.sub(dot, t))
        if v[0] < 0:                                   # (the first term entered with a plus sign)
            raise AssertionError("first component must be positive")
        s = p.mul(dot, p.const(2.0 / float((v * v).sum())))
        ynew = []
        for i in range(n):
            vs = s if abs(v[i]) == 1 else p.mul(cst[abs(int(v[i]))], s)
            ynew.append(p.sub(y[i], vs) if v[i] > 0 else p.add(y[i], vs))
        y = ynew
    e = None
    for k in range(n):
        t = p.mul(n + k, p.mul(y[k], y[k]))
        e = t if e is None else p.add(e, t)
    p.out(p.mul(p.const(0.5), e))
    return p.arrays()


def diag_program(nb):
    """inputs: u 0 .. n-1 (DoFs), d n .. 2n-1, oa 2n, ob 2n+1. d_i multiplies (1/2 u_i^2), whose second derivative is exactly 1."""
    n = 3 * nb
    p = cc.Prog(2 * n + 2)
    half = p.const(0.5)
    e = None
    for i in range(n):
        t = p.mul(n + i, p.mul(half, p.mul(i, i)))
        e = t if e is None else p.add(e, t)
    e = p.add(e, p.mul(2 * n, p.mul(0, 1)))
    e = p.add(e, p.mul(2 * n + 1, p.mul(1, 2)))
    p.out(e)
    return p.arrays()


_CASES = {}


def make_case(family, nb, ne=None, reverse=False):
    """custom_cases.Case of the family on ne elements (default 4 EPW + 1); reverse: the same elements registered in reversed order"""
    ne = n_elem_default(nb) if ne is None else ne
    key = (family, nb, ne, reverse)
    if key in _CASES:
        return _CASES[key]
    n = 3 * nb
    rng = np.random.default_rng(1000 * nb + FAMILIES.index(family))
    x = rng.uniform(-0.8, 0.8, (ne * nb, 3))
    order = np.arange(ne)[::-1] if reverse else np.arange(ne)
    conn = np.stack([order * nb + k for k in range(nb)] + [order], axis=1).astype(np.int32)
    bind = [("x", 3, k) for k in range(nb)]
    if family in SPECTRAL:
        arrays = [np.ascontiguousarray(spectrum(family, nb, ne))]
        bind = bind + [(0, n, nb)]
        ops, cst = spectral_program(nb)
    else:
        d, o = diag_inputs(family, nb, ne)
        arrays = [np.ascontiguousarray(d), np.ascontiguousarray(o)]
        bind = bind + [(0, n, nb), (1, 2, nb)]
        ops, cst = diag_program(nb)
    c = cc.Case("psd_%s_%d%s" % (family, nb, "_rev" if reverse else ""), family, nb, x, np.ascontiguousarray(conn), bind, arrays, ops, cst, compile_cpu=False)
    assert c.n_inputs <= cc.MAX_IN
    _CASES[key] = c
    return c


# ======================================================================================================================================
# exact references
# ======================================================================================================================================
def f_rule(l, eps, mirroring):
    return (-l if mirroring else type(l)(eps)) if l < eps else l


def _mp_eye(n):
    return np.array([[MP.mpf(1 if i == j else 0) for j in range(n)] for i in range(n)], dtype=object)


def q_exact(n):
    """(Z, D): Q = H1 H2 = Z / D with the INTEGER matrix Z = prod((v . v) I - 2 v v^T) and D = prod(v . v), as object arrays of mpf. Z Z^T = D^2 I holds
    exactly (integers of a few digits), so the projection of a multiple of the identity has exact zeros off the diagonal."""
    Z = _mp_eye(n)
    D = MP.mpf(1)
    for v in householder_vectors(n):
        vm = np.array([MP.mpf(int(c)) for c in v], dtype=object)
        vv = MP.mpf(int((v * v).sum()))
        Z = Z @ (_mp_eye(n) * vv - np.outer(vm, vm) * MP.mpf(2))
        D = D * vv
    return Z, D


def _sandwich(ZD, lm):
    """Q diag(lm) Q^T"""
    Z, D = ZD
    return ((Z * lm) @ Z.T) / (D * D)


def _to_float(M):
    return np.array([[float(v) for v in row] for row in M])


@dataclass
class Exact:
    H: np.ndarray          # [ne, n, n]: H_exact rounded once to float64
    P: dict                # mirroring (0, 1) -> [ne, n, n]: the exact projection rounded once (H where the element is unchanged)
    lam: np.ndarray        # [ne, n]: the exact eigenvalues (rounded)
    changed: np.ndarray    # [ne] bool: an exact eigenvalue below eps
    fro: np.ndarray        # [ne]: ||H_exact||_F


_EXACT = {}


def _eig_block(B, eps):
    """(eigenvalues, {mirroring: projected}) of a small exact matrix through mpmath.eigsy at 40 digits"""
    k = B.shape[0]
    with mpmath.workdps(MP.dps):
        E, V = MP.eigsy(MP.matrix(B.tolist()))
    E = [E[i] for i in range(k)]
    Vn = np.array([[V[i, j] for j in range(k)] for i in range(k)], dtype=object)
    P = {}
    for mir in (0, 1):
        fl = np.array([f_rule(l, MP.mpf(eps), mir) for l in E], dtype=object)
        P[mir] = (Vn * fl) @ Vn.T
    return E, P


def exact(family, nb, ne=None, eps=EPS) -> Exact:
    ne = n_elem_default(nb) if ne is None else ne
    key = (family, nb, ne, eps)
    if key in _EXACT:
        return _EXACT[key]
    n = 3 * nb
    H = np.zeros((ne, n, n))
    P = {0: np.zeros((ne, n, n)), 1: np.zeros((ne, n, n))}
    lam = np.zeros((ne, n))
    if family in SPECTRAL:
        Q = q_exact(n)
        lf = spectrum(family, nb, ne)
        for e in range(ne):
            lm = np.array([MP.mpf(float(v)) for v in lf[e]], dtype=object)
            H[e] = _to_float(_sandwich(Q, lm))
            lam[e] = lf[e]
            for mir in (0, 1):
                fl = np.array([f_rule(l, MP.mpf(eps), mir) for l in lm], dtype=object)
                P[mir][e] = _to_float(_sandwich(Q, fl)) if (lf[e] < eps).any() else H[e]
    else:
        d, o = diag_inputs(family, nb, ne)
        for e in range(ne):
            H[e] = np.diag(d[e])
            H[e, 0, 1] = H[e, 1, 0] = o[e, 0]
            H[e, 1, 2] = H[e, 2, 1] = o[e, 1]
            if (o[e] != 0).any():       # the coupled leading 3 x 3 block by mpmath.eigsy, the rest is diagonal
                B = np.array([[MP.mpf(float(v)) for v in row] for row in H[e, :3, :3]], dtype=object)
                E3, P3 = _eig_block(B, eps)
                lam[e] = np.concatenate([[float(v) for v in E3], d[e, 3:]])
            else:
                lam[e] = d[e]
            for mir in (0, 1):
                if not (lam[e] < eps).any():
                    P[mir][e] = H[e]
                    continue
                P[mir][e] = np.diag([f_rule(float(v), eps, mir) for v in d[e]])
                if (o[e] != 0).any():
                    P[mir][e][:3, :3] = _to_float(P3[mir])
    res = Exact(H, P, lam, (lam < eps).any(axis=1), np.sqrt((H * H).sum(axis=(1, 2))))
    _EXACT[key] = res
    return res


def project_readback(H, eps=EPS, mirroring=0):
    """(projected [ne, n, n], changed [ne]) of float64 matrices read back from the device, through mpmath.eigsy at 40 digits. The matrix is taken
    as stored (symmetric to the bit is asserted by the caller); an element without an eigenvalue below eps is returned untouched. mirroring = None:
    both rules from one decomposition, as {0: ..., 1: ...}."""
    H = np.asarray(H, dtype=np.float64)
    out = {0: H.copy(), 1: H.copy()}
    changed = np.zeros(len(H), dtype=bool)
    for e in range(len(H)):
        B = np.array([[MP.mpf(float(v)) for v in row] for row in H[e]], dtype=object)
        E, P = _eig_block(B, eps)
        if any(l < eps for l in E):
            changed[e] = True
            for mir in (0, 1):
                if mirroring is None or mir == int(bool(mirroring)):
                    out[mir][e] = _to_float(P[mir])
    return (out if mirroring is None else out[int(bool(mirroring))]), changed


# ======================================================================================================================================
# the float64 restatement of the kernels' Jacobi
# ======================================================================================================================================
def round_pairs(n, r):
    """the disjoint pairs (p < q < n) of round r of the round-robin schedule of m = even(n) players (k_project_eig; rr_partner)"""
    m = (n + 1) & ~1
    out = []
    for k in range(m // 2):
        p, q = (m - 1, r) if k == 0 else ((r + k) % (m - 1), (r - k + (m - 1)) % (m - 1))
        p, q = min(p, q), max(p, q)
        if q < n:
            out.append((p, q))
    return out


def restatement(H, eps=EPS):
    """({mirroring: projected}, changed, sweeps [ne], converged [ne]): cyclic-by-round Jacobi in float64 with IEEE division and square root, the kernels' pair
    schedule, stop rule off <= JACOBI_OFF_TOL * fro and clamping; at most 30 sweeps."""
    H = np.asarray(H, dtype=np.float64)
    ne, n, _ = H.shape
    m = (n + 1) & ~1
    A = H.copy()
    V = np.broadcast_to(np.eye(n), (ne, n, n)).copy()
    offmask = ~np.eye(n, dtype=bool)

    def off(A):
        return ((A * A) * offmask).sum(axis=(1, 2))

    fro = (A * A).sum(axis=(1, 2))
    active = np.ones(ne, dtype=bool)
    sweeps = np.zeros(ne, dtype=int)
    with np.errstate(all="ignore"):
        for _ in range(MAX_SWEEPS):
            active &= ~(off(A) <= JACOBI_OFF_TOL * fro)
            if not active.any():
                break
            sweeps[active] += 1
            for r in range(m - 1):
                J = np.broadcast_to(np.eye(n), (ne, n, n)).copy()
                for p, q in round_pairs(n, r):
                    apq = A[:, p, q]
                    rot = active & (np.abs(apq) > 1e-300)
                    theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                    t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    cs = 1.0 / np.sqrt(t * t + 1.0)
                    sn = t * cs
                    # new[p] = cs old[p] - sn old[q];  new[q] = sn old[p] + cs old[q]
                    J[rot, p, p] = cs[rot]
                    J[rot, q, q] = cs[rot]
                    J[rot, q, p] = -sn[rot]
                    J[rot, p, q] = sn[rot]
                A = np.transpose(J, (0, 2, 1)) @ A @ J
                V = V @ J
        converged = off(A) <= JACOBI_OFF_TOL * fro
    l = np.einsum("eii->ei", A)
    bad = l < eps
    changed = bad.any(axis=1)
    P = {}
    for mir in (0, 1):
        l2 = np.where(bad, -l if mir else eps, l)
        P[mir] = H.copy()
        P[mir][changed] = np.einsum("eik,ek,ejk->eij", V, l2, V)[changed]
    return P, changed, sweeps, converged


# ======================================================================================================================================
# tolerances and the bound
# ======================================================================================================================================
def _rel(err, fro):
    return np.where(fro > 0, err / np.where(fro > 0, fro, 1.0), np.where(err == 0, 0.0, np.inf))


def restatement_error(family, nb):
    """the restatement's largest error against the exact projection over the family's elements and both rules, relative to ||H||_F"""
    return restatement_figures(family, nb)[0]


def restatement_figures(family, nb):
    """(error, changed, sweeps, converged, P) of one run of the restatement on the family's H_exact"""
    ex = exact(family, nb)
    P, changed, sweeps, converged = restatement(ex.H, EPS)
    worst = 0.0
    for mir in (0, 1):
        err = np.sqrt(((P[mir] - ex.P[mir]) ** 2).sum(axis=(1, 2)))
        worst = max(worst, float(_rel(err, ex.fro).max()))
    return worst, changed, sweeps, converged, P


def measure_tolerances():
    """family -> NB -> restatement_error"""
    return {fam: {str(nb): restatement_error(fam, nb) for nb in NBS} for fam in FAMILIES}


def write_tolerances(path=TOLERANCES):
    """Regenerates tests/psd_tolerances.json:  python -c "import psd_cases as c; c.write_tolerances()"  from tests/ (repository root on PYTHONPATH)."""
    with open(path, "w") as f:
        json.dump(measure_tolerances(), f, indent=1, sort_keys=True)
        f.write("\n")


_TABLE = {}


def rounding_tolerance(family, nb):
    """8 x the recorded restatement error, floor 8 * 2^-52 * 3 NB (relative to ||H||_F)"""
    if not _TABLE:
        with open(TOLERANCES) as f:
            _TABLE.update(json.load(f))
    return max(8.0 * _TABLE[family][str(nb)], 8.0 * 2.0 ** -52 * 3 * nb)


def bound(family, nb, fro, h_in_err):
    """per element: ||H_in - H_exact||_F + (sqrt(JACOBI_OFF_TOL) + rounding) ||H||_F"""
    return np.asarray(h_in_err) + (SQRT_OFF_TOL + rounding_tolerance(family, nb)) * np.asarray(fro)


def margins_hold(family, nb):
    """(ok [ne], figures): every element's decision is MARGIN bounds away from rounding. H_in's error is taken at its CPU limit 8 * 2^-52 ||H||."""
    ex = exact(family, nb)
    b = bound(family, nb, ex.fro, 8.0 * 2.0 ** -52 * ex.fro)
    lo = ex.lam.min(axis=1)
    ok = np.where(ex.changed, lo <= EPS - MARGIN * b, lo >= EPS + MARGIN * b)
    return ok, (lo, b)
