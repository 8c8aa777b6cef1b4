"""Synthesised user-defined potentials (SymX op sequences) and their exact derivatives — shared by tests/test_custom_cases_cpu.py (the cases and
the float64 oracle are proved here, the emitted program is run on the host) and tests/test_gpu_custom_synth.py (the device interpreter and the
hipRTC kernels of stark_amd/csrc/custom.hip against the same numbers).

 * `Prog` is a tiny expression builder that hands out value indices and writes the rows {type, dst, a, b, cond} of include/mistark.h
   mistark_potential_custom.
 * `exact(case)` evaluates an op sequence per element in mpmath at 50 digits on truncated second-order Taylor numbers (value, gradient, the
   full n x n Hessian as sparse maps) — not the device's (i, j) hyper-dual pairs and not oracle.ad's dense arrays: an independent formulation.
   A branch takes the arm chosen by `value > 0`, a condition program gates the element the same way, an inactive element is not evaluated.
 * `CASES` / `BASE` are the named cases of the families a-g of the module's sections; every case of 257 elements has a one-element twin
   (`<name>.1`: the same program and arrays, one element of the chain), and the twin is what `single(case)` returns.
 * `measure_tolerances()` / `write_tolerances()` regenerate tests/custom_tolerances.json: per family the float64 oracle's own error against
   `exact`, relative to the largest magnitude of the quantity over the case. The GPU test's bounds are 8 x these numbers (floor 8 * 2^-52).

POWF at x <= 0 is not part of any case: the device's value exp(y ln x) is NaN there and the reference has no derivative of PowF to compare
with (user potentials).
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field

import mpmath
import numpy as np

# symx::ExprType as include/mistark.h lists them
ZERO, ONE, BRANCH, CONST, SYMBOL, ADD, SUB, MUL, RECIP, POWN, POWF, SQRT, LN, LOG10, EXP, SIN, COS, TAN, ASIN, ACOS, ATAN, PRINT = 0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22
UNARY = {"RECIP": RECIP, "SQRT": SQRT, "LN": LN, "LOG10": LOG10, "EXP": EXP, "SIN": SIN, "COS": COS, "TAN": TAN, "ASIN": ASIN, "ACOS": ACOS, "ATAN": ATAN}
MAX_REGS, MAX_IN, MAX_DEPTH = 256, 96, 32     # CUSTOM_MAX_REGS, CUSTOM_MAX_IN, CUSTOM_MAX_DEPTH of stark_amd/csrc/custom.hip
NE = 257                                      # 257 * 21 lanes cross the 256-thread blocks in the middle of an element; no multiple of 64
TOLERANCES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "custom_tolerances.json")
FLOOR = 8.0 * 2.0 ** -52

MP = mpmath.mp.clone()
MP.dps = 50


# ======================================================================================================================================
# the builder
# ======================================================================================================================================
class Prog:
    def __init__(self, n_in):
        self.n_in = n_in
        self.rows, self.cst = [], []
        self.next = n_in
        self.depth = 0

    def new(self):
        self.next += 1
        return self.next - 1

    def _op(self, t, a=-1, b=-1, c=0.0, dst=None):
        dst = self.new() if dst is None else dst
        self.rows.append((t, dst, a, b, -1))
        self.cst.append(float(c))
        return dst

    def zero(self, dst=None): return self._op(ZERO, dst=dst)
    def one(self, dst=None): return self._op(ONE, dst=dst)
    def const(self, c, dst=None): return self._op(CONST, c=c, dst=dst)
    def add(self, a, b, dst=None): return self._op(ADD, a, b, dst=dst)
    def sub(self, a, b, dst=None): return self._op(SUB, a, b, dst=dst)
    def mul(self, a, b, dst=None): return self._op(MUL, a, b, dst=dst)
    def un(self, t, a, dst=None): return self._op(t, a, dst=dst)
    def pown(self, a, n, dst=None): return self._op(POWN, a, int(n), dst=dst)
    def powf(self, a, b, dst=None): return self._op(POWF, a, b, dst=dst)

    def if_(self, cond):
        self.rows.append((BRANCH, -1, 0, -1, cond))
        self.cst.append(0.0)
        self.depth += 1

    def else_(self):
        self.rows.append((BRANCH, -1, 1, -1, -1))
        self.cst.append(0.0)

    def endif(self):
        self.rows.append((BRANCH, -1, -1, -1, -2))
        self.cst.append(0.0)
        self.depth -= 1

    def out(self, a):
        self.rows.append((SYMBOL, 0, a, -1, -1))
        self.cst.append(0.0)

    # small compounds
    def dot3(self, a, b):
        s = self.mul(a, b)
        for d in (1, 2):
            s = self.add(s, self.mul(a + d, b + d))
        return s

    def dist2(self, a, b):
        s = None
        for d in range(3):
            t = self.sub(a + d, b + d)
            t = self.mul(t, t)
            s = t if s is None else self.add(s, t)
        return s

    def arrays(self):
        return np.array(self.rows, dtype=np.int32).reshape(-1, 5), np.array(self.cst, dtype=np.float64)


@dataclass
class Case:
    name: str
    family: str
    nb: int
    x: np.ndarray                 # [n_nodes, 3]: the one DoF set
    conn: np.ndarray              # int32 [n_elem, n_cols]
    bindings: list                # (array, stride, conn column): array "x" = the DoF set, otherwise an index into `arrays`; column -1 = broadcast
    arrays: list                  # float64 [n_items, stride]
    ops: np.ndarray
    consts: np.ndarray
    cond_ops: np.ndarray | None = None
    cond_consts: np.ndarray | None = None
    compile_cpu: bool = True      # compiled with hipRTC / run on the host in the CPU suite (the one-op families: one case per op)
    notes: dict = field(default_factory=dict)

    @property
    def n_elem(self):
        return self.conn.shape[0]

    @property
    def strides(self):
        return np.array([s for _, s, _ in self.bindings], dtype=np.int32)

    @property
    def n_inputs(self):
        return int(self.strides.sum())

    @property
    def in_dof(self):
        d = -np.ones(self.n_inputs, dtype=np.int32)
        o = blk = 0
        for a, s, _ in self.bindings:
            if isinstance(a, str):
                d[o:o + 3] = 3 * blk + np.arange(3)
                blk += 1
            o += s
        return d

    @property
    def dof_cols(self):
        return [c for a, _, c in self.bindings if isinstance(a, str)]

    def gathered(self):
        """[n_elem, n_inputs]: what the kernels gather per element."""
        cols = []
        for a, s, c in self.bindings:
            data = self.x if isinstance(a, str) else self.arrays[a]
            data = data.reshape(-1, s)
            cols.append(data[self.conn[:, c]] if c >= 0 else np.broadcast_to(data[0], (self.n_elem, s)))
        return np.ascontiguousarray(np.concatenate(cols, axis=1))


def single(case: Case, e=None) -> Case:
    e = case.n_elem // 2 if e is None else e
    return Case(case.name + ".1", case.family, case.nb, case.x, np.ascontiguousarray(case.conn[e:e + 1]), case.bindings, case.arrays, case.ops, case.consts, case.cond_ops,
                case.cond_consts, False, dict(case.notes))


# ======================================================================================================================================
# the exact reference: second-order Taylor numbers over mpmath, sparse in the DoFs
# ======================================================================================================================================
class T2:
    __slots__ = ("v", "g", "h")

    def __init__(self, v, g=None, h=None):
        self.v, self.g, self.h = v, g or {}, h or {}


def _lin(ca, A, cb, B):
    r = {k: ca * v for k, v in A.items()}
    for k, v in B.items():
        r[k] = r[k] + cb * v if k in r else cb * v
    return r


def _outer(r, A, B, c=None):
    """r[(i, j)] += c * (A_i B_j + A_j B_i) for i <= j (c = None: 1)"""
    for i, ai in A.items():
        for j, bj in B.items():
            p = ai * bj if c is None else c * ai * bj
            if i == j:
                p = p + p
                k = (i, i)
            else:
                k = (i, j) if i < j else (j, i)
            r[k] = r[k] + p if k in r else p


def t_add(a, b, sign=1):
    return T2(a.v + sign * b.v, _lin(1, a.g, sign, b.g), _lin(1, a.h, sign, b.h))


def t_mul(a, b):
    h = _lin(b.v, a.h, a.v, b.h)
    if a.g and b.g:
        _outer(h, a.g, b.g)
    return T2(a.v * b.v, _lin(b.v, a.g, a.v, b.g), h)


def t_chain(x, f, df, ddf):
    h = {k: df * v for k, v in x.h.items()}
    if x.g and ddf != 0:
        half = {k: v / 2 for k, v in x.g.items()}
        _outer(h, half, x.g, ddf)
    return T2(f, {k: df * v for k, v in x.g.items()}, h)


def t_unary(t, x, n=0):
    m, v = MP, x.v
    if t == RECIP:
        r = 1 / v
        return t_chain(x, r, -r * r, 2 * r * r * r)
    if t == SQRT:
        s = m.sqrt(v)
        return t_chain(x, s, 1 / (2 * s), -1 / (4 * s * v))
    if t in (LN, LOG10):
        if not v > 0:
            return T2(m.mpf("-inf"))                       # custom_math.hpp cop_ln: -inf, no derivatives
        k = 1 if t == LN else 1 / m.log(10)
        return t_chain(x, k * m.log(v), k / v, -k / (v * v))
    if t == EXP:
        e = m.exp(v)
        return t_chain(x, e, e, e)
    if t == SIN:
        return t_chain(x, m.sin(v), m.cos(v), -m.sin(v))
    if t == COS:
        return t_chain(x, m.cos(v), -m.sin(v), -m.cos(v))
    if t == TAN:
        tn = m.tan(v)
        return t_chain(x, tn, 1 + tn * tn, 2 * tn * (1 + tn * tn))
    if t in (ASIN, ACOS):
        s = 1 / m.sqrt(1 - v * v)
        return t_chain(x, m.asin(v), s, v * s ** 3) if t == ASIN else t_chain(x, m.acos(v), -s, -v * s ** 3)
    if t == ATAN:
        d = 1 / (1 + v * v)
        return t_chain(x, m.atan(v), d, -2 * v * d * d)
    if t == POWN:
        if n == 0:
            return T2(m.mpf(1))
        return t_chain(x, v ** n, n * v ** (n - 1), n * (n - 1) * v ** (n - 2))
    raise ValueError(t)


def run_exact(ops, consts, inp, in_dof, with_derivatives=True):
    """One element: inp = list of mpf. Returns the T2 bound to output 0."""
    n_in = len(inp)
    val = {}

    def get(i):
        if i < n_in:
            d = in_dof[i]
            return T2(inp[i], {int(d): MP.mpf(1)} if (d >= 0 and with_derivatives) else None)
        return val[i]

    out = T2(MP.mpf(0))
    stack = []                  # (parent active, taken)
    active = True
    for (t, dst, a, b, cond), c in zip(ops, consts):
        if t == BRANCH:
            if cond == -2:
                active = stack.pop()[0]
            elif a == 0:
                tk = False
                if active:
                    cv = get(cond).v
                    tk = bool(cv > 0)
                    # a computed condition must not sit where float64 and exact arithmetic could disagree about its sign
                    assert cond < n_in or cv == 0 or abs(cv) > 1e-6, "condition value %s too close to zero" % cv
                stack.append((active, tk))
                active = tk
            else:
                active = stack[-1][0] and not stack[-1][1]
            continue
        if not active:
            continue
        if t == SYMBOL:
            out = get(a)
        elif t == ZERO or t == PRINT:
            val[dst] = T2(MP.mpf(0))
        elif t == ONE:
            val[dst] = T2(MP.mpf(1))
        elif t == CONST:
            val[dst] = T2(MP.mpf(c))
        elif t == ADD:
            val[dst] = t_add(get(a), get(b))
        elif t == SUB:
            val[dst] = t_add(get(a), get(b), -1)
        elif t == MUL:
            val[dst] = t_mul(get(a), get(b))
        elif t == POWF:
            x, y = get(a), get(b)
            assert x.v > 0, "POWF at x <= 0 is not compared"
            val[dst] = t_unary(EXP, t_mul(y, t_unary(LN, x)))
        elif t == POWN:
            val[dst] = t_unary(POWN, get(a), b)
        else:
            val[dst] = t_unary(t, get(a))
    return out


@dataclass
class Exact:
    E: float
    grad: np.ndarray        # [3 * n_nodes], assembled
    H: np.ndarray           # [n_elem, n, n] (zeros where inactive)
    Ee: np.ndarray          # [n_elem]
    ge: np.ndarray          # [n_elem, n]
    active: np.ndarray      # [n_elem] bool
    scale: dict             # largest magnitude of {"energy": element energies, "gradient": assembled gradient, "hessian": element Hessians}


_EXACT = {}


def exact(case: Case) -> Exact:
    if case.name in _EXACT:
        return _EXACT[case.name]
    ops, cst = case.ops.tolist(), case.consts.tolist()
    inp = case.gathered()
    in_dof = case.in_dof.tolist()
    n = 3 * case.nb
    ne = case.n_elem
    H = np.zeros((ne, n, n))
    ge = np.zeros((ne, n))
    Ee = np.zeros(ne)
    active = np.ones(ne, dtype=bool)
    E = MP.mpf(0)
    grad = [MP.mpf(0)] * case.x.size
    nodes = case.conn[:, case.dof_cols]
    for e in range(ne):
        x = [MP.mpf(float(v)) for v in inp[e]]
        if case.cond_ops is not None:
            active[e] = bool(run_exact(case.cond_ops.tolist(), case.cond_consts.tolist(), x, in_dof, False).v > 0)
            if not active[e]:
                continue
        r = run_exact(ops, cst, x, in_dof)
        E += r.v
        Ee[e] = float(r.v)
        for i, v in r.g.items():
            ge[e, i] = float(v)
            grad[3 * int(nodes[e, i // 3]) + i % 3] += v
        for (i, j), v in r.h.items():
            H[e, i, j] = H[e, j, i] = float(v)
    g = np.array([float(v) for v in grad])
    scale = {"energy": float(np.abs(Ee).max()), "gradient": float(np.abs(g).max()), "hessian": float(np.abs(H).max())}
    res = Exact(float(E), g, H, Ee, ge, active, scale)
    if case.family == "random":   # the generator's promise: nothing of a random program leaves 1e-6 .. 1e6
        for k, s in scale.items():
            assert 1e-6 <= s <= 1e6, (case.name, k, s)
    _EXACT[case.name] = res
    return res


# ======================================================================================================================================
# the float64 oracle on a case, and the tolerance table
# ======================================================================================================================================
def oracle_problem(case: Case):
    from oracle import evaluator as ev

    arrays = [case.x] + list(case.arrays)
    bs = [ev.Binding(0 if isinstance(a, str) else a + 1, s, c, 0 if isinstance(a, str) else -1) for a, s, c in case.bindings]
    pot = ev.PotentialDesc(case.name, case.conn, bs, case.cond_ops is not None)
    return ev.Problem(dt=0.0, ndofs=case.x.size, dof_offsets=[0], dof_sizes=[case.x.size], arrays=arrays, potentials=[pot], dof_arrays={0: 0}), pot


def oracle(case: Case):
    """(E, assembled gradient, element Hessians [n_elem, n, n] with zeros where inactive, active) from oracle.symx_ops in float64."""
    from oracle import symx_ops

    prob, pot = oracle_problem(case)
    o = symx_ops.evaluate(prob, pot, case.ops, case.consts, case.cond_ops, case.cond_consts)
    n = 3 * case.nb
    g = np.zeros(case.x.size)
    for k in range(case.nb):
        np.add.at(g.reshape(-1, 3), o.block_rows[:, k], o.g[:, 3 * k:3 * k + 3])
    H = np.zeros((case.n_elem, n, n))
    H[o.active] = o.H
    return float(o.E.sum()), g, H, o.active


def errors(E, g, H, ex: Exact):
    """max |. - exact| / scale per quantity"""
    d = {"energy": abs(E - ex.E), "gradient": float(np.abs(np.asarray(g).reshape(-1) - ex.grad).max()), "hessian": float(np.abs(H - ex.H).max())}
    # (a quantity that is exactly zero over the whole case, such as an element whose only Symbol op sits in the arm it does not take, has to come out as zero)
    return {k: v / ex.scale[k] if ex.scale[k] > 0 else (0.0 if v == 0 else float("inf")) for k, v in d.items()}


def measure_tolerances(cases=None):
    """family -> quantity -> the largest error of the float64 oracle against `exact` over the family's cases, relative to the case's scale"""
    tab = {}
    for c in (CASES.values() if cases is None else cases):
        if c.notes.get("untoleranced"):
            continue
        e = errors(*oracle(c)[:3], exact(c))
        t = tab.setdefault(c.family, {"energy": 0.0, "gradient": 0.0, "hessian": 0.0})
        for k in t:
            t[k] = max(t[k], e[k])
    return tab


def write_tolerances(path=TOLERANCES):
    """Regenerates tests/custom_tolerances.json:  python -c "import custom_cases as c; c.write_tolerances()"  from tests/ (repository root on PYTHONPATH)."""
    with open(path, "w") as f:
        json.dump(measure_tolerances(), f, indent=1, sort_keys=True)
        f.write("\n")


def bounds(case: Case, ex: Exact):
    """The absolute bounds of a device (or host-compiled) result against `exact`: 8 x the oracle's own error for the family, floor 8 * 2^-52, times the scale."""
    with open(TOLERANCES) as f:
        t = json.load(f)[case.family]
    return {k: max(8.0 * t[k], FLOOR) * ex.scale[k] for k in t}


# ======================================================================================================================================
# the cases
# ======================================================================================================================================
def _chain(seed, nb, ne=NE, span=0.8):
    """ne elements over a chain of nodes: element e joins nodes e .. e + nb - 1 (neighbours share nodes), last column = the element's own index"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-span, span, (ne + nb - 1, 3))
    conn = np.stack([np.arange(ne) + k for k in range(nb)] + [np.arange(ne)], axis=1).astype(np.int32)
    return rng, x, conn


def _edge_q(p, k):
    """q = k0 + k1 (xa . xb) + k2 |xa - xb|^2 on inputs xa = 0..2, xb = 3..5, k = k..k+2;  s = 1.5 + xa_z xb_x"""
    q = p.add(p.add(k, p.mul(k + 1, p.dot3(0, 3))), p.mul(k + 2, p.dist2(0, 3)))
    s = p.add(p.const(1.5), p.mul(2, 3))
    return q, s


def _edge_k(rng, x, lo, hi):
    """per-element constants such that q lies in [lo, hi] (drawn 1 % inside the interval; the margin is asserted on the float64 q)"""
    ne = x.shape[0] - 1
    xa, xb = x[:-1], x[1:]
    k = rng.uniform(0.05, 0.3, (ne, 3)) * rng.choice([-1.0, 1.0], (ne, 3))
    w = hi - lo
    target = rng.uniform(lo + 0.01 * w, hi - 0.01 * w, ne)
    dot, d2 = (xa * xb).sum(1), ((xa - xb) ** 2).sum(1)
    k[:, 0] = target - k[:, 1] * dot - k[:, 2] * d2
    q = k[:, 0] + k[:, 1] * dot + k[:, 2] * d2
    assert (q >= lo).all() and (q <= hi).all(), (lo, hi, q.min(), q.max())
    return np.ascontiguousarray(k), q


EDGE_BIND = [("x", 3, 0), ("x", 3, 1), (0, 3, 2)]


def _one_op(name, family, seed, build, ranges, compile_cpu):
    """E = U(q) s with q in the union of `ranges` (alternating over the elements)"""
    rng, x, conn = _chain(seed, 2)
    k = np.zeros((NE, 3))
    for r, (lo, hi) in enumerate(ranges):
        kr, _ = _edge_k(rng, x, lo, hi)
        k[r::len(ranges)] = kr[r::len(ranges)]
    p = Prog(9)
    q, s = _edge_q(p, 6)
    p.out(p.mul(build(p, q), s))
    ops, cst = p.arrays()
    return Case(name, family, 2, x, conn, EDGE_BIND, [k], ops, cst, compile_cpu=compile_cpu)


# domains with the stated margins: |q| <= 0.9 (ASIN, ACOS), q >= 0.1 (SQRT, LN, LOG10, RECIP), |q| <= 1.2 (TAN)
UNARY_DOMAIN = {"RECIP": [(0.1, 2.0)], "SQRT": [(0.1, 2.0)], "LN": [(0.1, 2.0)], "LOG10": [(0.1, 2.0)], "EXP": [(-2.0, 2.0)], "SIN": [(-3.0, 3.0)], "COS": [(-3.0, 3.0)],
                "TAN": [(-1.2, 1.2)], "ASIN": [(-0.9, 0.9)], "ACOS": [(-0.9, 0.9)], "ATAN": [(-3.0, 3.0)]}
# near the edge where the derivative grows: |q| up to 0.999, q down to 1e-3
UNARY_EDGE = {"ASIN": [(0.99, 0.999), (-0.999, -0.99)], "ACOS": [(0.99, 0.999), (-0.999, -0.99)], "SQRT": [(1e-3, 1e-2)], "LN": [(1e-3, 1e-2)], "RECIP": [(1e-3, 1e-2)]}
POWN_N = [0, 1, 2, 3, 5, -1, -2, -3]


def _family_a():
    out = []
    for i, (nm, t) in enumerate(UNARY.items()):
        out.append(_one_op("op_" + nm.lower(), "one_op", 100 + i, lambda p, q, t=t: p.un(t, q), UNARY_DOMAIN[nm], True))
        if nm in UNARY_EDGE:
            out.append(_one_op("op_%s_edge" % nm.lower(), "one_op_edge", 150 + i, lambda p, q, t=t: p.un(t, q), UNARY_EDGE[nm], False))
    for i, n in enumerate(POWN_N):
        tag = ("m%d" % -n) if n < 0 else str(n)
        out.append(_one_op("op_pown_" + tag, "one_op", 200 + i, lambda p, q, n=n: p.pown(q, n), [(0.5, 2.0)], True))
        out.append(_one_op("op_pown_%s_negbase" % tag, "one_op", 250 + i, lambda p, q, n=n: p.pown(q, n), [(-2.0, -0.5)], False))
    return out


def _family_b():
    out = []
    for i, y in enumerate([0.5, 2.0, -1.5, 0.0, 1.0]):
        out.append(_one_op("powf_const_%g" % y, "powf", 300 + i, lambda p, q, y=y: p.powf(q, p.const(y)), [(0.3, 2.5)], i == 0))
    # the exponent as a bound non-DoF input (a fourth per-element constant), and depending on DoFs
    for name, seed, dof in (("powf_bound_exponent", 310, False), ("powf_dof_exponent", 311, True)):
        rng, x, conn = _chain(seed, 2)
        k, _ = _edge_k(rng, x, 0.3, 2.5)
        k = np.ascontiguousarray(np.concatenate([k, rng.uniform(-2.0, 2.0, (NE, 1))], axis=1))
        p = Prog(10)
        q, s = _edge_q(p, 6)
        y = p.add(p.const(0.5), p.mul(1, 5)) if dof else 9
        p.out(p.mul(p.powf(q, y), s))
        ops, cst = p.arrays()
        out.append(Case(name, "powf", 2, x, conn, [("x", 3, 0), ("x", 3, 1), (0, 4, 2)], [k], ops, cst))
    return out


def _branch_case(name, seed, body, special=None):
    """inputs: xa 0..2, xb 3..5, p 6..8 (per element; |p| in [0.2, 1], signs drawn per element: neighbouring lanes take different arms).
    body(P, u, w) writes the program; u = xa . xb, w = |xa - xb|^2 are defined before any branch."""
    rng, x, conn = _chain(seed, 2)
    prm = rng.uniform(0.2, 1.0, (NE, 3)) * rng.choice([-1.0, 1.0], (NE, 3))
    if special is not None:
        prm[:, 0] = np.resize(np.array(special), NE)
    p = Prog(9)
    u, w = p.dot3(0, 3), p.dist2(0, 3)
    body(p, u, w)
    assert p.depth == 0
    ops, cst = p.arrays()
    return Case(name, "branch", 2, x, conn, EDGE_BIND, [np.ascontiguousarray(prm)], ops, cst)


def _family_c():
    def if_no_else(p, u, w):
        v = p.mul(u, w)
        p.if_(6)
        p.add(p.un(SIN, u), w, dst=v)
        p.endif()
        p.out(p.mul(v, p.add(p.const(1.5), p.mul(2, 3))))

    def if_else_same_value(p, u, w):
        v = p.new()
        p.if_(6)
        p.un(SIN, u, dst=v)
        p.else_()
        p.mul(p.un(COS, w), u, dst=v)
        p.endif()
        p.out(p.add(p.mul(v, v), v))

    def symbol_in_arms(p, u, w):
        p.if_(6)
        p.out(p.mul(u, w))
        p.else_()
        t = p.add(u, w)
        p.out(p.mul(t, t))
        p.endif()

    def symbol_in_if_only(p, u, w):
        p.if_(6)
        p.out(p.mul(p.un(EXP, u), w))
        p.endif()

    def nest3(p, u, w):
        v = p.new()
        p.if_(6)
        p.if_(7)
        p.mul(u, u, dst=v)
        p.else_()
        p.if_(8)                       # an if inside an else
        p.un(SIN, w, dst=v)
        p.else_()
        p.mul(p.un(COS, u), w, dst=v)
        p.endif()
        p.endif()
        p.else_()
        p.if_(7)
        t = p.add(u, w)
        p.if_(8)
        p.mul(t, t, dst=v)
        p.else_()
        p.un(ATAN, t, dst=v)
        p.endif()
        p.else_()
        p.sub(u, w, dst=v)
        p.endif()
        p.endif()
        p.out(p.mul(v, p.add(p.const(1.5), p.mul(2, 3))))

    def deep(depth):
        def body(p, u, w):
            v = p.mul(u, w)
            one = p.one()
            for _ in range(depth - 1):   # trivially true
                p.if_(one)
            p.if_(6)                     # the data-dependent one, innermost
            p.un(SIN, u, dst=v)
            p.else_()
            p.mul(v, w, dst=v)
            p.endif()
            for _ in range(depth - 1):
                p.endif()
            p.out(p.add(v, w))
        return body

    def reuse_across_arms(p, u, w):
        a = p.mul(u, w)                  # defined before the if, read for the last time inside the if arm
        v = p.new()
        p.if_(6)
        b = p.mul(a, a)
        p.add(b, u, dst=v)
        p.else_()
        c = p.mul(w, w)                  # new definitions in the else arm (may take a's register)
        d = p.add(c, u)
        p.mul(d, c, dst=v)
        p.endif()
        e = p.mul(v, w)                  # ... and after endif
        p.out(p.add(e, v))

    def reuse_else_reads(p, u, w):
        a = p.un(SIN, u)                 # read only in the else arm: alive across the whole if arm
        v = p.new()
        p.if_(6)
        b = p.mul(u, w)
        c = p.add(b, w)
        p.mul(c, b, dst=v)
        p.else_()
        p.mul(a, w, dst=v)
        p.endif()
        p.out(p.mul(v, u))

    def last_read_defines_next(p, u, w):
        t1 = p.mul(u, w)
        t2 = p.mul(t1, t1)               # t1 is read for the last time (twice) by the op that defines t2
        t3 = p.add(t2, u)
        t4 = p.mul(t3, t2)               # both operands die here
        t5 = p.un(SIN, t4)
        t6 = p.sub(t5, w)
        t7 = p.mul(t6, t6)
        p.out(p.add(t7, u))

    nan = float("nan")
    return [_branch_case("branch_if_no_else", 400, if_no_else), _branch_case("branch_if_else_same_value", 401, if_else_same_value),
            _branch_case("branch_symbol_in_arms", 402, symbol_in_arms), _branch_case("branch_symbol_in_if_only", 403, symbol_in_if_only),
            _branch_case("branch_nest3", 404, nest3), _branch_case("branch_depth31", 405, deep(MAX_DEPTH - 1)), _branch_case("branch_depth32", 406, deep(MAX_DEPTH)),
            # +0.0, -0.0, a negative denormal and NaN are not taken (the rule is > 0); 0.25 beside them so that the lanes of a wavefront diverge
            _branch_case("branch_special_conditions", 407, if_else_same_value, special=[0.0, -0.0, -5e-324, nan, 0.25]),
            _branch_case("branch_reuse_across_arms", 408, reuse_across_arms), _branch_case("branch_reuse_else_reads", 409, reuse_else_reads),
            _branch_case("branch_last_read_defines_next", 410, last_read_defines_next)]


NODE_BIND = [("x", 3, 0), (0, 3, 1)]


def pressure_program(K):
    """K temporaries defined first, then all read: inputs x 0..2, p 3..5. The sum runs in place in the first temporary, so exactly K are live."""
    p = Prog(6)
    t = []
    for i in range(K):
        if i % 8 == 0:
            t.append(p.mul(i // 8 % 3, (i // 8 + 1) % 3))      # x_i x_j
        elif i % 8 == 4:
            t.append(p.mul(3 + i % 3, (i // 8) % 3))            # p x
        else:
            t.append(p.mul(3 + i % 3, 3 + (i + 1) % 3))         # p p
    for i in range(1, K):
        p.add(t[0], t[i], dst=t[0])
    p.out(t[0])
    return p.arrays()


def _family_d():
    out = []
    rng, x, conn = _chain(500, 1)
    prm = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (NE, 3)))
    ops, cst = pressure_program(MAX_REGS)
    out.append(Case("regs_256_live", "regs", 1, x, conn, NODE_BIND, [prm], ops, cst))
    # 600 ops, a handful of registers: a recurrence on constants with a DoF-dependent step every tenth op
    p = Prog(6)
    v = p.mul(0, 1)
    c = p.mul(3, 4)
    while len(p.rows) < 597:
        k = len(p.rows)
        if k % 10 == 0:                  # v <- t / (1 + t^2), t = v + x_k c: bounded whatever c does
            t = p.add(v, p.mul(k // 10 % 3, c))
            v = p.mul(t, p.un(RECIP, p.add(p.one(), p.mul(t, t))))
        else:                            # (arithmetic only: 600 ops of inlined device libm would compile for minutes)
            c = p.add(c, 3 + k % 3) if k % 3 == 0 else p.mul(c, 3 + k % 3)
    p.out(p.mul(v, p.add(c, 2)))
    ops, cst = p.arrays()
    assert 600 <= len(ops) <= 606
    out.append(Case("regs_chain_600", "regs", 1, x, conn, NODE_BIND, [prm], ops, cst))
    return out


def _random_case(seed):
    rng, x, conn = _chain(600 + seed, 2)
    n_par = int(rng.integers(2, 4))
    prm = np.ascontiguousarray(rng.uniform(0.2, 1.0, (NE, n_par)) * rng.choice([-1.0, 1.0], (NE, n_par)))
    n_in = 6 + n_par
    p = Prog(n_in)
    case0 = Case("tmp", "random", 2, x, conn, [("x", 3, 0), ("x", 3, 1), (0, n_par, 2)], [prm], None, None)
    vals = {i: col for i, col in enumerate(case0.gathered().T)}     # float64 values of every value index, per element (growth / domain control)
    n_target = int(rng.integers(48, 108))
    n_branches = int(rng.integers(0, 4))

    def ev(t, a=None, b=None, c=0.0):
        with np.errstate(all="ignore"):
            A, B = vals.get(a), vals.get(b)
            return {ZERO: lambda: np.zeros(NE), ONE: lambda: np.ones(NE), PRINT: lambda: np.zeros(NE), CONST: lambda: np.full(NE, c), ADD: lambda: A + B, SUB: lambda: A - B,
                    MUL: lambda: A * B, RECIP: lambda: 1 / A, SQRT: lambda: np.sqrt(A), LN: lambda: np.log(A), LOG10: lambda: np.log10(A), EXP: lambda: np.exp(A),
                    SIN: lambda: np.sin(A), COS: lambda: np.cos(A), TAN: lambda: np.tan(A), ASIN: lambda: np.arcsin(A), ACOS: lambda: np.arccos(A), ATAN: lambda: np.arctan(A),
                    POWN: lambda: A ** b, POWF: lambda: A ** B}[t]()

    def emit(t, a=-1, b=-1, c=0.0, dst=None):
        r = ev(t, a, b, c)
        d = p._op(t, a, b, c, dst)
        vals[d] = r
        return d

    def tame(v):          # keep magnitudes near 1: scale down what grew
        m = float(np.abs(vals[v]).max())
        assert np.isfinite(m), "random program left the domain"
        return emit(MUL, v, emit(CONST, c=1.0 / m)) if m > 2.0 else v

    def one_plus_sq(v):   # 1 + v^2 >= 1: legal for SQRT, LN, LOG10, RECIP, negative powers, POWF
        return emit(ADD, emit(ONE), emit(MUL, v, v))

    def unit(v):          # 0.9 v / sqrt(1 + v^2): inside (-0.9, 0.9) for ASIN, ACOS, TAN
        return emit(MUL, emit(CONST, c=0.9), emit(MUL, v, emit(RECIP, emit(SQRT, one_plus_sq(v)))))

    def step(pool):
        pick = lambda: pool[int(rng.integers(max(0, len(pool) - 12), len(pool)))] if rng.random() < 0.7 else pool[int(rng.integers(0, len(pool)))]
        kind = int(rng.integers(0, 20))
        a, b = pick(), pick()
        if kind < 3: r = emit(ADD, a, b)
        elif kind < 5: r = emit(SUB, a, b)
        elif kind < 9: r = emit(MUL, a, b)
        elif kind == 9: r = emit([SIN, COS, ATAN][int(rng.integers(0, 3))], a)
        elif kind == 10: r = emit(EXP, a)
        elif kind == 11: r = emit([SQRT, LN, LOG10, RECIP][int(rng.integers(0, 4))], one_plus_sq(a))
        elif kind == 12: r = emit([ASIN, ACOS, TAN][int(rng.integers(0, 3))], unit(a))
        elif kind == 13: r = emit(POWN, a, int(rng.choice([0, 1, 2, 3, 5])))
        elif kind == 14: r = emit(POWN, one_plus_sq(a), int(rng.choice([-1, -2, -3])))
        elif kind == 15: r = emit(POWF, one_plus_sq(a), b)
        elif kind == 16:
            z = int(rng.integers(0, 3))
            r = emit(ADD, a, emit(ZERO) if z == 0 else (emit(ONE) if z == 1 else emit(PRINT, b)))
        elif kind == 17: r = emit(MUL, a, emit(CONST, c=float(rng.uniform(-1.5, 1.5))))
        else: r = emit(MUL, emit(SIN, a), b)
        return tame(r)

    def block(pool, n_ops, depth):
        """ops appended to the pool; may open a balanced branch whose merged value joins the pool"""
        nonlocal n_branches
        start = len(p.rows)
        while len(p.rows) - start < n_ops:
            if n_branches > 0 and depth < 3 and rng.random() < 0.08:
                n_branches -= 1
                cands = [v for v in pool[-6:] if v >= n_in and float(np.abs(vals[v]).min()) > 1e-3 and (vals[v] > 0).any() and (vals[v] < 0).any()]
                cond = cands[-1] if cands and rng.random() < 0.5 else 6 + int(rng.integers(0, n_par))
                taken = vals[cond] > 0
                m = step(pool)                             # the merged value: defined before, redefined in the arm(s)
                before = vals[m].copy()
                has_else = rng.random() < 0.6
                p.if_(cond)
                inner = list(pool)
                block(inner, int(rng.integers(2, 8)), depth + 1)
                r_if = vals[emit(MUL, inner[-1], pool[-1], dst=m)].copy()
                r_else = before
                if has_else:
                    p.else_()
                    vals[m] = before
                    inner = list(pool)
                    block(inner, int(rng.integers(2, 8)), depth + 1)
                    r_else = vals[emit(SUB, inner[-1], pool[0], dst=m)].copy()
                p.endif()
                vals[m] = np.where(taken, r_if, r_else)
                pool.append(tame(m))
            else:
                pool.append(step(pool))

    pool = list(range(n_in))
    block(pool, n_target - 8, 0)
    e = emit(ADD, pool[-1], pool[-2])
    for v in pool[-5:-2]:
        e = emit(ADD, e, v)
    e = emit(MUL, e, emit(ADD, emit(CONST, c=1.5), emit(MUL, 2, 3)))
    p.out(e)
    ops, cst = p.arrays()
    assert 40 <= len(ops) <= 120, (seed, len(ops))
    return Case("random_%02d" % seed, "random", 2, x, conn, case0.bindings, [prm], ops, cst)


def _family_f():
    out = []
    # strides 1, 2, 3, 9, 12; per element (column 2), per node (columns 0, 1) and broadcast (-1) side by side
    rng, x, conn = _chain(700, 2)
    arr = [rng.uniform(-1, 1, (NE, 1)), rng.uniform(-1, 1, (NE + 1, 2)), rng.uniform(-1, 1, (1, 3)), rng.uniform(-1, 1, (NE, 9)), rng.uniform(-1, 1, (NE + 1, 12))]
    arr = [np.ascontiguousarray(a) for a in arr]
    bind = [("x", 3, 0), ("x", 3, 1), (0, 1, 2), (1, 2, 0), (2, 3, -1), (3, 9, 2), (4, 12, 1)]
    o1, o2, o3, o9, o12 = 6, 7, 9, 12, 21
    p = Prog(33)
    u, w = p.dot3(0, 3), p.dist2(0, 3)
    e = p.mul(p.un(SIN, u), o1)
    e = p.add(e, p.mul(o2 + 1, w))
    e = p.add(e, p.mul(o3 + 2, p.mul(u, u)))
    e = p.add(e, p.mul(o9 + 8, p.mul(w, u)))
    e = p.add(e, p.mul(o12 + 11, p.mul(0, 4)))
    e = p.add(e, p.mul(p.mul(o12, o9), p.mul(o2, p.mul(o3, 5))))
    p.out(e)
    ops, cst = p.arrays()
    out.append(Case("inputs_strides_and_broadcast", "inputs", 2, x, conn, bind, arr, ops, cst))
    # exactly 96 inputs on triangles (NB = 3: 45 lanes per element): 9 DoFs + seven arrays of stride 12 + one of stride 3
    rng, x, conn = _chain(701, 3)
    arr = [np.ascontiguousarray(rng.uniform(-1, 1, (NE, 12))) for _ in range(7)] + [np.ascontiguousarray(rng.uniform(-1, 1, (1, 3)))]
    bind = [("x", 3, 0), ("x", 3, 1), ("x", 3, 2)] + [(i, 12, 3) for i in range(7)] + [(7, 3, -1)]
    ops, cst = full_inputs_program(MAX_IN)
    out.append(Case("inputs_96", "inputs", 3, x, conn, bind, arr, ops, cst))
    # ZERO / ONE / PRINT (Print's value is 0)
    rng, x, conn = _chain(702, 2)
    p = Prog(9)
    u, w = p.dot3(0, 3), p.dist2(0, 3)
    e = p.add(p.mul(u, p.one()), p.zero())
    e = p.add(e, p.un(PRINT, u))
    e = p.mul(e, p.add(w, p.mul(p.un(PRINT, w), 6)))
    p.out(p.add(e, p.mul(p.one(), 7)))
    ops, cst = p.arrays()
    out.append(Case("inputs_zero_one_print", "inputs", 2, x, conn, EDGE_BIND, [np.ascontiguousarray(rng.uniform(-1, 1, (NE, 3)))], ops, cst))
    return out


def full_inputs_program(n_in):
    """reads every input of a triangle potential with n_in inputs (9 DoFs first): E = sum_k in[k] * (a product of DoFs) + |xa - xb|^2 (xb . xc)"""
    p = Prog(n_in)
    e = p.mul(p.dist2(0, 3), p.dot3(3, 6))
    for k in range(9, n_in):
        e = p.add(e, p.mul(k, p.mul(k % 9, (k + 4) % 9)) if k % 6 == 0 else p.mul(k, k % 9))
    p.out(e)
    return p.arrays()


def _family_g():
    """A condition program: c |xa - xb|^2 is > 0 on about half of the elements, exactly 0.0 on some, < 0 on the rest. The energy of an inactive
    element is NaN / inf (0 * ln c, sqrt c at c <= 0): evaluated there, it shows in every total."""
    rng, x, conn = _chain(800, 2)
    prm = rng.uniform(0.2, 1.0, (NE, 3))
    kind = rng.choice([1.0, 0.0, -1.0], NE, p=[0.5, 0.15, 0.35])
    prm[:, 0] *= kind
    prm[NE // 2, 0] = 0.7                         # (the one-element twin is an active element; its neighbours are not)
    prm[NE // 2 - 1, 0], prm[NE // 2 + 1, 0] = 0.0, -0.4
    assert (prm[:, 0] > 0).sum() > NE // 3 and (prm[:, 0] == 0).sum() > 10 and (prm[:, 0] < 0).sum() > NE // 5
    p = Prog(9)
    u, w = p.dot3(0, 3), p.dist2(0, 3)
    e = p.mul(p.un(SIN, u), p.add(p.const(1.5), p.mul(2, 3)))
    e = p.add(e, p.mul(p.un(SQRT, 6), w))
    e = p.add(e, p.mul(p.un(LN, 6), p.zero()))
    p.out(e)
    ops, cst = p.arrays()
    c = Prog(9)
    c.out(c.mul(6, c.dist2(0, 3)))
    cops, ccst = c.arrays()
    return [Case("condition_half_active", "condition", 2, x, conn, EDGE_BIND, [np.ascontiguousarray(prm)], ops, cst, cops, ccst)]


def _build():
    base = _family_a() + _family_b() + _family_c() + _family_d() + [_random_case(s) for s in range(16)] + _family_f() + _family_g()
    cases = {}
    for c in base:
        cases[c.name] = c
        cases[c.name + ".1"] = single(c)
    return base, cases


BASE, CASES = _build()
