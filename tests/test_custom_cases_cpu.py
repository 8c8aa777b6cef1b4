"""CPU: the synthesised user potentials of tests/custom_cases.py are proved here, before any kernel is blamed (tests/test_gpu_custom_synth.py).

 * a. for every case the float64 oracle (oracle.symx_ops, every op of symx::ExprType) agrees with the 50-digit Taylor reference `exact(case)`;
      its error per family is what tests/custom_tolerances.json records (custom_cases.write_tolerances regenerates it), and the table is the only
      source of the bounds the host-compiled and the GPU comparisons use;
 * b. registration through mistark_custom_emit, no device: every case emits, the branch / register / random / input / condition families and one
      case per op compile with hipRTC for gfx950, 257 live temporaries and 97 inputs are refused, and so is every malformed if / else / endif
      sequence, with the potential's name and the op index in the message, in the energy and in the condition program;
 * c. the emitted prog_energy / prog_condition themselves, cut out of that source and compiled with g++ (tests/host_custom/host_custom.cpp),
      against `exact` under the same bounds as on the GPU: a wrong register or a wrong line of the emitter changes a number here. (The host
      compiler and libm differ from the device's: this is not a substitute for the GPU run.) LN / LOG10 of q <= 0 is asserted here as
      custom_math.hpp defines it: -inf with zero derivatives.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_cases as cc  # noqa: E402

ALL = list(cc.CASES)
COMPILED = [c.name for c in cc.BASE if c.compile_cpu]
CAP = 1 << 22


def _emit(name, strides, in_dof, ops, cst, n_in, nb, compile_it=False, cops=None, ccst=None):
    from stark_amd import capi

    L = capi.lib()
    L.mistark_custom_emit.restype = C.c_int64
    L.mistark_custom_emit.argtypes = [C.c_char_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_char_p, C.c_int64]
    strides = np.ascontiguousarray(strides, dtype=np.int32)
    in_dof = np.ascontiguousarray(in_dof, dtype=np.int32)
    ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 5)
    cst = np.ascontiguousarray(cst, dtype=np.float64)
    nco = 0 if cops is None else len(cops)
    if nco:
        cops = np.ascontiguousarray(cops, dtype=np.int32).reshape(-1, 5)
        ccst = np.ascontiguousarray(ccst, dtype=np.float64)
    out = C.create_string_buffer(CAP)
    r = L.mistark_custom_emit(name.encode(), strides.ctypes.data, len(strides), in_dof.ctypes.data, ops.ctypes.data, cst.ctypes.data, len(ops), n_in,
                              cops.ctypes.data if nco else None, ccst.ctypes.data if nco else None, nco, nb, 1 if compile_it else 0, out, CAP)
    return r, out.value.decode()


def _emit_case(case, compile_it=False):
    return _emit(case.name, case.strides, case.in_dof, case.ops, case.consts, case.n_inputs, case.nb, compile_it, case.cond_ops, case.cond_consts)


# ---- a. the cases and the oracle ---------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_what_it_promises():
    fam = {}
    for c in cc.BASE:
        fam.setdefault(c.family, []).append(c)
        assert c.n_elem == cc.NE and cc.CASES[c.name + ".1"].n_elem == 1
    assert set(fam) == {"one_op", "one_op_edge", "powf", "branch", "regs", "random", "inputs", "condition"}
    assert len(fam["random"]) == 16 and all(40 <= len(c.ops) <= 120 for c in fam["random"])
    used = set()
    for c in cc.BASE:
        used |= set(c.ops[:, 0].tolist())
    assert used == set(range(0, 23)) - {3}                                       # every op type
    assert {c.nb for c in cc.BASE} == {1, 2, 3}
    assert sum(((c.ops[:, 0] == cc.BRANCH) & (c.ops[:, 4] >= 0)).sum() > 0 for c in fam["random"]) >= 8
    # condition values of the special case: +0.0, -0.0, a negative denormal, NaN
    p0 = cc.CASES["branch_special_conditions"].arrays[0][:5, 0]
    assert p0[0] == 0 and not np.signbit(p0[0]) and p0[1] == 0 and np.signbit(p0[1]) and -1e-300 < p0[2] < 0 and np.isnan(p0[3]) and p0[4] > 0


def test_the_oracle_knows_every_op_and_refuses_only_what_is_none():
    from oracle import symx_ops

    for t in (3, 23, -1):
        with pytest.raises(NotImplementedError):
            symx_ops.run(np.array([[t, 1, 0, 0, -1]]), np.zeros(1), [np.ones(2)], 2)


@pytest.fixture(scope="module")
def table():
    with open(cc.TOLERANCES) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ALL)
def test_oracle_agrees_with_the_exact_reference(name, table):
    case = cc.CASES[name]
    ex = cc.exact(case)
    E, g, H, active = cc.oracle(case)
    assert (active == ex.active).all()
    assert np.isfinite(ex.E) and np.isfinite(ex.grad).all() and np.isfinite(ex.H).all()
    err = cc.errors(E, g, H, ex)
    print(name, case.family, err)
    for k, v in err.items():
        # float64 throughout: the worst conditioning among the cases is the 1 / q^3 of RECIP's second derivative at q = 1e-3 against a q that
        # carries the rounding of a cancelling sum, a few 1e4 eps relative to the case's largest entry
        assert v <= 1e-11, (k, v)
        # ... and the committed table is this measurement (numpy's vectorised libm may differ by an ulp between hosts: a factor 2, and the floor)
        assert v <= max(2.0 * table[case.family][k], cc.FLOOR / 8), (k, v, table[case.family][k])


def test_margins_hold_on_the_exact_arguments():
    """The generator asserts the domain margins on the float64 q; here the same on the 50-digit q of every one-op case."""
    for c in cc.BASE:
        if c.family not in ("one_op", "one_op_edge") or "pown" in c.name:
            continue
        op = c.name.split("_")[1].upper()
        lo = min(r[0] for r in (cc.UNARY_EDGE if c.family == "one_op_edge" else cc.UNARY_DOMAIN)[op])
        hi = max(r[1] for r in (cc.UNARY_EDGE if c.family == "one_op_edge" else cc.UNARY_DOMAIN)[op])
        k = int(np.flatnonzero(c.ops[:, 0] == cc.UNARY[op])[0])
        sub = np.vstack([c.ops[:k], [[cc.SYMBOL, 0, c.ops[k, 2], -1, -1]]])
        for e in range(c.n_elem):
            q = cc.run_exact(sub.tolist(), c.consts[:k + 1].tolist(), [cc.MP.mpf(float(v)) for v in c.gathered()[e]], c.in_dof.tolist(), False).v
            assert lo <= q <= hi, (c.name, e, q)


# ---- b. registration ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in cc.BASE])
def test_every_case_emits(name):
    case = cc.CASES[name]
    n, src = _emit_case(case)
    assert n > 0, src
    assert "prog_energy" in src and ("prog_condition" in src) == (case.cond_ops is not None)
    n_if = int(((case.ops[:, 0] == cc.BRANCH) & (case.ops[:, 4] != -2) & (case.ops[:, 2] == 0)).sum())
    body = src[src.index("HDual prog_energy"):]
    body = body[:body.index("return out;")]
    assert body.count(".v > 0.0) {") == n_if and body.count("{") == body.count("}") + 1


@pytest.mark.parametrize("name", COMPILED)
def test_cases_compile_with_hiprtc(name, tmp_path, monkeypatch):
    monkeypatch.setenv("MISTARK_RTC_CACHE", str(tmp_path))   # (a build, not a cache hit)
    size, msg = _emit_case(cc.CASES[name], True)
    assert size > 4096, msg[:2000]


def _refused(ops, cst, n_in=6, strides=(3, 3), in_dof=(0, 1, 2, -1, -1, -1), nb=1, cond=None, name="Bad"):
    r, msg = _emit(name, strides, in_dof, ops, cst, n_in, nb, False, *(cond or (None, None)))
    assert r < 0, "accepted"
    return msg


def test_257_live_temporaries_and_97_inputs_are_refused():
    ops, cst = cc.pressure_program(cc.MAX_REGS)
    r, src = _emit("K256", (3, 3), (0, 1, 2, -1, -1, -1), ops, cst, 6, 1)
    assert r > 0 and "HDual r255;" in src and "HDual r256;" not in src
    ops, cst = cc.pressure_program(cc.MAX_REGS + 1)
    msg = _refused(ops, cst, name="K257")
    assert "K257" in msg and "needs 257 live temporaries" in msg and "has 256" in msg
    dof9 = list(range(9))
    ops, cst = cc.full_inputs_program(cc.MAX_IN)
    r, _ = _emit("In96", [3, 3, 3] + [12] * 7 + [3], dof9 + [-1] * 87, ops, cst, 96, 3)
    assert r > 0
    ops, cst = cc.full_inputs_program(cc.MAX_IN + 1)
    msg = _refused(ops, cst, 97, [3, 3, 3] + [12] * 7 + [3, 1], dof9 + [-1] * 88, 3, name="In97")
    assert "In97" in msg and "more than 96 inputs" in msg


def _marker_programs():
    """name -> (rows, index of the op the message has to name, a word of the message)"""
    IF, ELSE, ENDIF = (cc.BRANCH, -1, 0, -1, 3), (cc.BRANCH, -1, 1, -1, -1), (cc.BRANCH, -1, -1, -1, -2)
    body, sym = (cc.MUL, 6, 0, 1, -1), (cc.SYMBOL, 0, 6, -1, -1)
    deep = [body] + [IF] * (cc.MAX_DEPTH + 1) + [ENDIF] * (cc.MAX_DEPTH + 1) + [sym]
    return {"else_without_if": ([body, ELSE, sym], 1, "else without an open if"), "endif_without_if": ([body, ENDIF, sym], 1, "endif without an open if"),
            "endif_after_balanced": ([body, IF, ENDIF, ENDIF, sym], 3, "endif without an open if"), "second_else": ([body, IF, ELSE, body, ELSE, ENDIF, sym], 4, "second else"),
            "if_left_open": ([body, IF, sym], 2, "still open"), "else_left_open": ([body, IF, ELSE, sym], 3, "still open"),
            "too_deep": (deep, cc.MAX_DEPTH + 1, "deeper than %d" % cc.MAX_DEPTH)}


@pytest.mark.parametrize("where", ["energy", "condition"])
@pytest.mark.parametrize("form", list(_marker_programs()))
def test_malformed_branch_markers_are_refused_with_name_and_op_index(form, where):
    rows, k, word = _marker_programs()[form]
    ops, cst = np.array(rows, dtype=np.int32), np.zeros(len(rows))
    good = np.array([(cc.MUL, 6, 0, 1, -1), (cc.SYMBOL, 0, 6, -1, -1)], dtype=np.int32)
    if where == "energy":
        msg = _refused(ops, cst, name="Marker")
    else:
        msg = _refused(good, np.zeros(2), cond=(ops, cst), name="Marker")
    assert "custom potential 'Marker" in msg and ("op %d " % k) in msg and word in msg, msg
    assert ("condition" in msg) == (where == "condition")


def test_the_depth_limit_is_the_first_refused_depth():
    """CUSTOM_MAX_DEPTH = 32 nested branches work (branch_depth32 runs on the GPU against `exact`), 33 is refused."""
    one = (cc.ONE, 6, -1, -1, -1)
    for depth, ok in ((cc.MAX_DEPTH - 1, True), (cc.MAX_DEPTH, True), (cc.MAX_DEPTH + 1, False)):
        rows = [one] + [(cc.BRANCH, -1, 0, -1, 6)] * depth + [(cc.SYMBOL, 0, 0, -1, -1)] + [(cc.BRANCH, -1, -1, -1, -2)] * depth
        r, msg = _emit("Deep", (3, 3), (0, 1, 2, -1, -1, -1), np.array(rows, dtype=np.int32), np.zeros(len(rows)), 6, 1)
        assert (r > 0) == ok, (depth, msg[:300])
    assert max(int(np.cumsum(np.where(c.ops[:, 0] != cc.BRANCH, 0, np.where(c.ops[:, 4] == -2, -1, np.where(c.ops[:, 2] == 0, 1, 0)))).max())
               for c in cc.BASE) == cc.MAX_DEPTH


# ---- c. the emitted program on the host --------------------------------------------------------------------------------------------------
def _host_eval(case, tmp_path):
    n, src = _emit_case(case)
    assert n > 0, src
    a, b = src.index("__device__ __forceinline__ HDual prog_energy"), src.index('extern "C" __global__')
    inc = tmp_path / "prog.inc"
    inc.write_text(src[a:b])
    so = tmp_path / "host_custom.so"
    cmd = ["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-D__device__=", "-D__forceinline__=inline", '-DHOST_CUSTOM_PROG="%s"' % inc, "-DHOST_CUSTOM_NIN=%d" % case.n_inputs,
           "-DHOST_CUSTOM_NB=%d" % case.nb] + (["-DHOST_CUSTOM_COND"] if case.cond_ops is not None else []) + [os.path.join(ROOT, "tests", "host_custom", "host_custom.cpp"), "-o", str(so)]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(str(so))
    lib.host_custom_eval.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    inp = case.gathered()
    ne, nn = case.n_elem, 3 * case.nb
    E, g, H, act = np.zeros(ne), np.zeros((ne, nn)), np.zeros((ne, nn, nn)), np.zeros(ne, dtype=np.int32)
    with np.errstate(all="ignore"):
        assert lib.host_custom_eval(inp.ctypes.data, ne, E.ctypes.data, g.ctypes.data, H.ctypes.data, act.ctypes.data) == 0
    return E, g, H, act.astype(bool)


@pytest.mark.parametrize("name", COMPILED)
def test_emitted_program_on_the_host_equals_the_exact_reference(name, tmp_path):
    case = cc.CASES[name]
    ex = cc.exact(case)
    E, ge, H, active = _host_eval(case, tmp_path)
    assert (active == ex.active).all()
    assert (E[~active] == 0).all() and (ge[~active] == 0).all() and (H[~active] == 0).all()
    g = np.zeros_like(ex.grad).reshape(-1, 3)
    nodes = case.conn[:, case.dof_cols]
    for k in range(case.nb):
        np.add.at(g, nodes[:, k], ge[:, 3 * k:3 * k + 3])
    err = cc.errors(float(E.sum()), g, H, ex)
    bound = cc.bounds(case, ex)
    print(name, {k: (err[k] * ex.scale[k], bound[k]) for k in err})
    for k in err:
        assert err[k] * ex.scale[k] <= bound[k] if ex.scale[k] > 0 else err[k] == 0, (k, err[k], bound[k] / max(ex.scale[k], 1e-300))
    # per element too (a wrong register in one arm must not hide in a total)
    assert np.abs(E - ex.Ee).max() <= bound["energy"] and np.abs(ge - ex.ge).max() <= bound["gradient"]
    assert (H == np.transpose(H, (0, 2, 1))).all()


@pytest.mark.parametrize("op", [cc.LN, cc.LOG10])
def test_ln_and_log10_of_a_nonpositive_value_are_minus_infinity_with_zero_derivatives(op, tmp_path):
    base = cc.CASES["op_ln"]
    p = cc.Prog(9)
    w = p.dist2(0, 3)
    q = p.mul(p.const(-1.0), p.mul(w, 6))          # -(k0 |xa - xb|^2): < 0 where k0 > 0, > 0 where k0 < 0, and 0 * ... = -0.0 where k0 = 0
    p.out(p.un(op, q))
    ops, cst = p.arrays()
    k = base.arrays[0].copy()
    k[:, 0] = np.resize(np.array([0.5, -0.5, 0.0]), len(k))
    case = cc.Case("ln_nonpositive", "one_op", 2, base.x, base.conn[:30], base.bindings, [k], ops, cst)
    E, g, H, _ = _host_eval(case, tmp_path)
    neg = np.resize(np.array([True, False, True]), 30)
    assert (E[neg] == -np.inf).all() and (g[neg] == 0).all() and (H[neg] == 0).all()
    assert np.isfinite(E[~neg]).all() and (np.abs(g[~neg]).max(axis=1) > 0).all()
