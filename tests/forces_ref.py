"""Reference of the force readout (include/mistark.h "force readout"), from the numpy oracle: per potential the element gradients of
oracle.evaluator.evaluate_potential, negated, scaled and scattered by their block rows; elements switched off by their condition are zero.

`reference(path)` evaluates a stage fixture once per process; the tests share the result and leave it unchanged."""
import functools

import numpy as np

from oracle import evaluator as ev

ELEMENT_TOL = {"EnergyDiscreteShells": 1e-8}  # ill-conditioned acos near 1, see tests/test_oracle_golden.py


def rel(a, b):
    """_rel of tests/test_gpu_parity.py"""
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def block_rows_all(prob, pot):
    """Block rows [n_elem, nb] of EVERY element of a potential (ElementOutput.block_rows lists the active ones only)."""
    order = ev.dof_layout(pot)
    return np.stack([prob.dof_offsets[pot.bindings[bi].dof_set] // 3 + pot.conn[:, pot.bindings[bi].conn] for bi in order], axis=1).astype(np.int64)


def potential_forces(prob, pot, scale):
    """None for an empty table, else dict(f [n_elem, nb, 3] with zeros for inactive elements, rows [n_elem, nb], active [n_elem],
    g_active [n_active, 3 nb] = the oracle's own gradients, rows_active = the oracle's own block rows)."""
    o = ev.evaluate_potential(prob, pot)
    if o is None:
        return None
    n_elem = pot.conn.shape[0]
    nb = o.block_rows.shape[1]
    f = np.zeros((n_elem, nb, 3))
    f[o.active] = -scale * o.g.reshape(-1, nb, 3)
    return dict(f=f, rows=block_rows_all(prob, pot), active=o.active, g_active=o.g, rows_active=o.block_rows, term_scale=term_scale(prob, pot, o))


def term_scale(prob, pot, o):
    """Magnitude of the terms an element gradient of this potential is the sum of. Several fixtures hold a state at rest (a trajectory's first
    step): the strain, bending and constraint gradients there are exact zeros mathematically, the reference's values are what the cancellation
    of its terms leaves (1e-18 beside terms of 1e-2), and an error relative to THAT measures nothing: no two evaluation orders agree on
    it. The terms: a relative change eps of an input x moves the gradient by |H| |x| eps; the DoFs are velocities, x1 = x0 + dt v1, so a
    position counts |x| / dt. Hence max|H| * max|3-vector inputs| / dt, with the oracle's own element Hessians."""
    if o.H.size == 0:
        return 0.0
    x = [np.abs(prob.arrays[b.array]).max() for b in pot.bindings if b.conn >= 0 and b.stride == 3 and prob.arrays[b.array].size]
    return float(np.abs(o.H).max() * (max(x) if x else 1.0) / prob.dt)


def cancelled(r, name):
    """The reference gradient of this potential is rounding noise: below the element tolerance of its own terms."""
    g = r["g_active"]
    return bool(g.size and np.abs(g).max() < ELEMENT_TOL.get(name, 1e-11) * r["term_scale"])


def rel_to_scale(a, b, scale, tol):
    """rel() — except where the reference has cancelled to rounding noise, max|b| < tol * (the magnitude of its terms): a value that lies below
    the tolerance of its own terms is no denominator, and the error is taken relative to the terms instead."""
    bmax = np.abs(b).max()
    return np.abs(a - b).max() / max(bmax if bmax >= tol * scale else scale, 1e-300)


def scatter(ndofs, rows, f):
    """Nodal vector [ndofs] of element forces f [n, nb, 3] at block rows [n, nb], and per scalar row the sum of |contributions|."""
    out, mag = np.zeros(ndofs), np.zeros(ndofs)
    idx = (3 * np.asarray(rows)[:, :, None] + np.arange(3)[None, None, :]).reshape(-1)
    np.add.at(out, idx, np.asarray(f).reshape(-1))
    np.add.at(mag, idx, np.abs(np.asarray(f)).reshape(-1))
    return out, mag


@functools.lru_cache(maxsize=None)
def reference(path, scale=None):
    """(prob, man, z, scale, per-potential dicts by potential index, nodal sum over all potentials, its magnitudes). scale: 1 / dt of the fixture."""
    prob, man, z = ev.load_fixture(path)
    s = (1.0 / prob.dt) if scale is None else scale
    per = {}
    total, mag = np.zeros(prob.ndofs), np.zeros(prob.ndofs)
    for pi, pot in enumerate(prob.potentials):
        r = potential_forces(prob, pot, s)
        if r is None:
            continue
        per[pi] = r
        n, m = scatter(prob.ndofs, r["rows"], r["f"])
        total += n
        mag += m
    total.setflags(write=False)
    mag.setflags(write=False)
    return prob, man, z, s, per, total, mag


def gradient_tolerance(man):
    """The tolerance tests/test_oracle_golden.py holds the oracle's gradient to on every stage fixture."""
    return max([1e-11] + [ELEMENT_TOL.get(p["name"], 0) for p in man["potentials"] if p["n_elem"] > 0])
