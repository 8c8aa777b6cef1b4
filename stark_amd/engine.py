"""Thin object wrapper over the C ABI: mirrors the reference's registration calls
(symx::GlobalPotential::add_dof / add_potential, symx/src/solver/GlobalPotential.h:37-70) one to one."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


class EngineError(RuntimeError):
    pass


class Engine:
    def __init__(self, device: int = 0):
        self.L = capi.lib()
        h = C.c_void_p()
        rc = self.L.mistark_create(device, C.byref(h))
        if rc != 0:
            raise EngineError("mistark_create failed (%d): no MI355X visible / HIP runtime error; the hot path has no CPU fallback" % rc)
        self.h = h
        self._keep = []          # host buffers must outlive the context (caller-owned memory contract)
        self._array_ids = {}
        self.potential_ids = {}

    def close(self):
        if self.h:
            self.L.mistark_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise EngineError(self.L.mistark_last_error(self.h).decode())
        return rc

    # ---- registration ------------------------------------------------------------------------------------------------
    def add_dof_set(self, label: str, arr: np.ndarray) -> int:
        assert arr.dtype == np.float64 and arr.flags.c_contiguous
        self._keep.append(arr)
        return self._ck(self.L.mistark_add_dof_set(self.h, label.encode(), arr.ctypes.data, arr.size))

    def array(self, arr: np.ndarray, stride: int | None = None) -> int:
        assert arr.dtype == np.float64 and arr.flags.c_contiguous
        if stride is None:
            stride = 1 if arr.ndim == 1 else arr.shape[-1]
        n_items = arr.size // stride
        self._keep.append(arr)
        return self._ck(self.L.mistark_array(self.h, arr.ctypes.data, n_items, stride))

    def potential(self, name: str, conn: np.ndarray, bindings) -> int:
        """bindings: list of (array_id, stride, conn_col) in the reference's mws.make_* order."""
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        if conn.ndim != 2:
            raise ValueError("conn must be [n_elem, stride]")
        b = (capi.Binding * len(bindings))(*[capi.Binding(a, s, c) for a, s, c in bindings])
        pid = self._ck(self.L.mistark_potential(self.h, name.encode(), conn.ctypes.data if conn.size else None, conn.shape[0], conn.shape[1], b, len(bindings)))
        self.potential_ids[name] = pid
        return pid

    def potential_custom(self, name: str, conn: np.ndarray, bindings, ops, constants, n_inputs: int, cond_ops=None, cond_constants=None) -> int:
        """A potential given as SymX's op sequence (rows {type, dst, a, b, cond} + one constant per op), interpreted on the device."""
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        b = (capi.Binding * len(bindings))(*[capi.Binding(a, s, c) for a, s, c in bindings])
        ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 5)
        cst = np.ascontiguousarray(constants, dtype=np.float64)
        nco = 0
        cops = ccst = None
        if cond_ops is not None and len(cond_ops):
            cops = np.ascontiguousarray(cond_ops, dtype=np.int32).reshape(-1, 5)
            ccst = np.ascontiguousarray(cond_constants, dtype=np.float64)
            nco = len(cops)
        self.L.mistark_potential_custom.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(capi.Binding), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        pid = self._ck(self.L.mistark_potential_custom(self.h, name.encode(), conn.ctypes.data if conn.size else None, conn.shape[0], conn.shape[1], b, len(bindings),
                                                       ops.ctypes.data, cst.ctypes.data, len(ops), int(n_inputs), cops.ctypes.data if nco else None,
                                                       ccst.ctypes.data if nco else None, nco))
        self.potential_ids[name] = pid
        return pid

    def potential_custom_set_summation(self, pid: int, first_input: int, data: np.ndarray):
        """Summation loop of a custom potential (MappedWorkspace::add_for_each): inputs [first_input, first_input + data.shape[1]) take the rows
        of `data` one after the other; energy, gradient and Hessian are summed over the rows."""
        d = np.ascontiguousarray(data, dtype=np.float64).reshape(len(data), -1)
        self.L.mistark_potential_custom_set_summation.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        self._ck(self.L.mistark_potential_custom_set_summation(self.h, pid, int(first_input), d.shape[1], d.shape[0], d.ctypes.data))

    def potential_id(self, name: str) -> int:
        pid = self.L.mistark_find_potential(self.h, name.encode())
        if pid < 0:
            raise KeyError(name)
        return pid

    def set_dynamic(self, pid: int, dynamic: bool = True):
        """Routes the potential's Hessian blocks to the dynamic (contact) part of the split matrix."""
        self._ck(self.L.mistark_potential_set_dynamic(self.h, pid, int(dynamic)))

    def update_connectivity(self, pid: int, conn: np.ndarray):
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        self._ck(self.L.mistark_potential_update_connectivity(self.h, pid, conn.ctypes.data if conn.size else None, conn.shape[0]))

    # ---- multi-GPU sharding ------------------------------------------------------------------------------------------------
    def dist_init_local(self, group, rank: int):
        self._ck(self.L.mistark_dist_init_local(self.h, group, rank))

    def dist_init_ipc(self, comm):
        """comm: a connected capi.IpcComm (one process per rank; include/mistark.h "IPC windows")."""
        self._comm = comm  # (must outlive the engine)
        self._ck(self.L.mistark_dist_init_ipc(self.h, comm.h))

    def dist_info(self):
        out = (C.c_int64 * 8)()
        self._ck(self.L.mistark_dist_info(self.h, out, 8))
        return list(out)

    def dist_row_owner(self) -> np.ndarray:
        o = np.zeros(self.ndofs // 3, dtype=np.int32)
        self._ck(self.L.mistark_dist_get_row_owner(self.h, o.ctypes.data))
        return o

    def dist_set_row_owner(self, owner):
        o = np.ascontiguousarray(owner, dtype=np.int32)
        self._ck(self.L.mistark_dist_set_row_owner(self.h, o.ctypes.data, len(o)))

    def dist_init_rccl(self, rank: int, world: int, unique_id: bytes):
        buf = C.create_string_buffer(unique_id, 128)
        self._ck(self.L.mistark_dist_init_rccl(self.h, rank, world, buf))

    # ---- device contact detector (include/mistark_contact.h) ----------------------------------------------------------------
    def contact_init(self, **array_ids):
        """array_ids: engine array ids by role (capi.CONTACT_ROLES); absent roles are -1."""
        a = capi.ContactArrays(*[int(array_ids.get(r, -1)) for r in capi.CONTACT_ROLES])
        self._ck(self.L.mistark_contact_init(self.h, C.byref(a)))

    def contact_add_mesh(self, kind: str, idx_in_ps: int, verts, tris, edges) -> int:
        v = np.ascontiguousarray(verts, dtype=np.int32)
        t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        return self._ck(self.L.mistark_contact_add_mesh(self.h, 0 if kind == "d" else 1, idx_in_ps, v.ctypes.data, len(v), t.ctypes.data if t.size else None, len(t),
                                                        e.ctypes.data if e.size else None, len(e)))

    def contact_set_friction(self, a, b, mu):
        self._ck(self.L.mistark_contact_set_friction(self.h, a, b, mu))

    def contact_disable_collision(self, a, b):
        self._ck(self.L.mistark_contact_disable_collision(self.h, a, b))

    def contact_set_broad_phase(self, brute_force: bool):
        self._ck(self.L.mistark_contact_set_broad_phase(self.h, int(brute_force)))

    def contact_update(self, dt) -> int:
        n = C.c_int64()
        self._ck(self.L.mistark_contact_update(self.h, dt, C.byref(n)))
        return n.value

    def contact_update_friction(self) -> int:
        n = C.c_int64()
        self._ck(self.L.mistark_contact_update_friction(self.h, C.byref(n)))
        return n.value

    def contact_count_intersections(self, dt) -> int:
        n = C.c_int64()
        self._ck(self.L.mistark_contact_count_intersections(self.h, dt, C.byref(n)))
        return n.value

    def contact_max_step(self, dt, conservative_rescaling=0.9):
        """mistark_contact_max_step: (max_step, n_candidates) of the current Newton direction (inside a max_allowed_step callback)."""
        t, n = C.c_double(), C.c_int64()
        self._ck(self.L.mistark_contact_max_step(self.h, dt, conservative_rescaling, C.byref(t), C.byref(n)))
        return t.value, n.value

    CCD_RIGID_MODES = ("linear", "curved")

    def contact_max_step_ex(self, dt, conservative_rescaling=0.9, rigid_mode="linear", max_rounds=4, du=None) -> dict:
        """mistark_contact_max_step_ex: the CCD query with rigid bodies on their chords ("linear") or on their true curved paths ("curved"), along the
        current Newton direction (du None) or a given one (ndofs doubles). Returns max_step, n_candidates, rounds, tau, pad_bound_pairs, max_pad."""
        if rigid_mode not in self.CCD_RIGID_MODES:
            raise ValueError("contact_max_step_ex: rigid_mode must be one of %s, not %r" % (self.CCD_RIGID_MODES, rigid_mode))
        ptr = None
        if du is not None:
            du = np.ascontiguousarray(du, dtype=np.float64)
            if du.size != self.ndofs:
                raise ValueError("contact_max_step_ex: du has %d entries, the engine %d DoFs" % (du.size, self.ndofs))
            ptr = du.ctypes.data
        r = capi.CcdResult()
        self._ck(self.L.mistark_contact_max_step_ex(self.h, dt, conservative_rescaling, self.CCD_RIGID_MODES.index(rigid_mode), int(max_rounds), ptr, C.byref(r)))
        return dict(max_step=r.max_step, n_candidates=r.n_candidates, rounds=r.rounds, tau=r.tau, pad_bound_pairs=r.pad_bound_pairs, max_pad=r.max_pad)

    def contact_table(self, name: str) -> np.ndarray:
        n, st = C.c_int32(), C.c_int32()
        self._ck(self.L.mistark_contact_get_table(self.h, name.encode(), None, C.byref(n), C.byref(st)))
        out = np.zeros((n.value, st.value), dtype=np.int32)
        if n.value:
            self._ck(self.L.mistark_contact_get_table(self.h, name.encode(), out.ctypes.data, C.byref(n), C.byref(st)))
        return out

    def contact_friction_data(self, name: str, n_rows: int) -> dict:
        nb = C.c_int32()
        self._ck(self.L.mistark_contact_get_friction_data(self.h, name.encode(), None, None, None, None, C.byref(nb)))
        T = np.zeros((n_rows, 6)); mu = np.zeros(n_rows); fn = np.zeros(n_rows); bary = np.zeros((n_rows, max(nb.value, 1)))
        self._ck(self.L.mistark_contact_get_friction_data(self.h, name.encode(), T.ctypes.data, mu.ctypes.data, fn.ctypes.data, bary.ctypes.data if nb.value else None, C.byref(nb)))
        out = dict(T=T, mu=mu, fn=fn)
        if nb.value:
            out["bary"] = bary
        return out

    # ---- contact report (include/mistark_contact.h "contact report") ------------------------------------------------------
    def contact_report(self) -> dict:
        """Rows of the installed barrier tables at the current DoFs, in table order: dict(ints [n, 8], doubles [n, 16], bounds [22] (table t owns rows
        bounds[t]:bounds[t + 1]) and the named columns table, source, type, group_a, group_b, prim_a, prim_b, flags, d, dhat, point_a, point_b,
        normal, mollifier, fn, E, params). No search runs; bit-reproducible."""
        n = C.c_int64()
        self._ck(self.L.mistark_contact_report(self.h, None, None, C.byref(n)))
        ri = np.zeros((n.value, 8), dtype=np.int32)
        rd = np.zeros((n.value, 16))
        if n.value:
            self._ck(self.L.mistark_contact_report(self.h, ri.ctypes.data, rd.ctypes.data, C.byref(n)))
        return contact_rows_dict(ri, rd)

    def contact_vertex_report(self) -> dict:
        """Per collision vertex: dict(records [n, 5], gap, count, force, area, pressure, group, source_index)."""
        n = C.c_int64()
        self._ck(self.L.mistark_contact_vertex_report(self.h, None, None, None, C.byref(n)))
        out = np.zeros((n.value, 5))
        group, src = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        if n.value:
            self._ck(self.L.mistark_contact_vertex_report(self.h, out.ctypes.data, group.ctypes.data, src.ctypes.data, C.byref(n)))
        return contact_vertices_dict(out, group, src)

    def contact_pair_report(self) -> np.ndarray:
        """records [n_groups, n_groups, 8], entries ga <= gb filled: rows, smallest d, dhat, sum fn, sum fn n (on the lower group), sum E."""
        g = C.c_int32()
        self._ck(self.L.mistark_contact_pair_report(self.h, None, C.byref(g)))
        out = np.zeros((g.value, g.value, 8))
        if g.value:
            self._ck(self.L.mistark_contact_pair_report(self.h, out.ctypes.data, C.byref(g)))
        return out

    # ---- friction report (include/mistark_contact.h "friction report") ----------------------------------------------------
    def friction_report(self) -> dict:
        """Rows of the installed friction tables at the velocities of the current DoFs, in table order: dict(ints [n, 8], doubles [n, 24], bounds [15]
        (table 21 + t owns rows bounds[t]:bounds[t + 1]) and the named columns table, row, kind, group_a, group_b, body_a, body_b, flags, mu, fn, epsu,
        u, slip, slip_speed, v, ft, ft_norm, mobilised, dissipation, E, param_a, weights_b). No search runs; bit-reproducible."""
        n = C.c_int64()
        self._ck(self.L.mistark_contact_friction_report(self.h, None, None, C.byref(n)))
        ri = np.zeros((n.value, 8), dtype=np.int32)
        rd = np.zeros((n.value, 24))
        if n.value:
            self._ck(self.L.mistark_contact_friction_report(self.h, ri.ctypes.data, rd.ctypes.data, C.byref(n)))
        return friction_rows_dict(ri, rd)

    def friction_vertex_report(self) -> dict:
        """Per collision vertex: dict(records [n, 8], count, sliding, force [n, 3], slip_speed, area, traction, group, source_index)."""
        n = C.c_int64()
        self._ck(self.L.mistark_contact_friction_vertex_report(self.h, None, None, None, C.byref(n)))
        out = np.zeros((n.value, 8))
        group, src = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        if n.value:
            self._ck(self.L.mistark_contact_friction_vertex_report(self.h, out.ctypes.data, group.ctypes.data, src.ctypes.data, C.byref(n)))
        return friction_vertices_dict(out, group, src)

    def friction_pair_report(self) -> np.ndarray:
        """records [n_groups, n_groups, 12], entries ga <= gb filled: rows, sliding rows, sum fn, sum mu fn, sum ft (on the lower group), sum |ft|, sum
        dissipation, sum E, largest slip speed, sum |ft| / sum mu fn."""
        g = C.c_int32()
        self._ck(self.L.mistark_contact_friction_pair_report(self.h, None, C.byref(g)))
        out = np.zeros((g.value, g.value, 12))
        if g.value:
            self._ck(self.L.mistark_contact_friction_pair_report(self.h, out.ctypes.data, C.byref(g)))
        return out

    def contact_vertices(self) -> np.ndarray:
        n = C.c_int64()
        self._ck(self.L.mistark_contact_get_vertices(self.h, None, C.byref(n)))
        x = np.zeros((n.value, 3))
        self._ck(self.L.mistark_contact_get_vertices(self.h, x.ctypes.data, C.byref(n)))
        return x

    def upload(self, array: int = -1):
        self._ck(self.L.mistark_upload(self.h, array))

    def download(self, array: int = -1):
        self._ck(self.L.mistark_download(self.h, array))

    def axpby(self, dst, a, x, b=0.0, y=-1):
        self._ck(self.L.mistark_array_axpby(self.h, dst, a, x, b, y))

    def fill(self, dst, v):
        self._ck(self.L.mistark_array_fill(self.h, dst, v))

    # ---- DoFs ------------------------------------------------------------------------------------------------------------
    @property
    def ndofs(self) -> int:
        return int(self.L.mistark_ndofs(self.h))

    def get_dofs(self) -> np.ndarray:
        u = np.zeros(self.ndofs)
        self._ck(self.L.mistark_get_dofs(self.h, u.ctypes.data))
        return u

    def set_dofs(self, u: np.ndarray):
        u = np.ascontiguousarray(u, dtype=np.float64)
        assert u.size == self.ndofs
        self._ck(self.L.mistark_set_dofs(self.h, u.ctypes.data))

    def dofs_to_host(self):
        self._ck(self.L.mistark_dofs_to_host_arrays(self.h))

    def dofs_from_host(self):
        self._ck(self.L.mistark_dofs_from_host_arrays(self.h))

    # ---- stages ------------------------------------------------------------------------------------------------------------
    def eval(self, mode=capi.EVAL_P_G_H, want_grad=True):
        E = C.c_double()
        g = np.zeros(self.ndofs) if (want_grad and mode != capi.EVAL_P) else None
        self._ck(self.L.mistark_eval(self.h, mode, C.byref(E), g.ctypes.data if g is not None else None))
        return E.value, g

    def element_hessians(self, pot: int, n_elem: int):
        nb = C.c_int32()
        self._ck(self.L.mistark_get_element_hessians(self.h, pot, None, None, C.byref(nb)))
        n = 3 * nb.value
        H = np.zeros((n_elem, n, n))
        rows = np.zeros((n_elem, nb.value), dtype=np.int32)
        self._ck(self.L.mistark_get_element_hessians(self.h, pot, H.ctypes.data, rows.ctypes.data, C.byref(nb)))
        return H, rows

    def element_energies(self, pot: int, n_elem: int):
        E = np.zeros(n_elem)
        self._ck(self.L.mistark_get_element_energies(self.h, pot, E.ctypes.data))
        return E

    # ---- force readout (include/mistark.h "force readout") ------------------------------------------------------------------
    def element_forces(self, pot: int, scale: float = 1.0):
        """(forces [n_elem, NB, 3], block_rows [n_elem, NB]) of one potential at the current DoFs: -scale * dE_e/du per node of every
        element (zeros for elements whose condition is off)."""
        ne, nb = C.c_int64(), C.c_int32()
        self._ck(self.L.mistark_potential_element_forces(self.h, pot, float(scale), None, None, C.byref(ne), C.byref(nb)))
        f = np.zeros((ne.value, nb.value, 3))
        rows = np.zeros((ne.value, nb.value), dtype=np.int32)
        if ne.value:
            self._ck(self.L.mistark_potential_element_forces(self.h, pot, float(scale), f.ctypes.data, rows.ctypes.data, C.byref(ne), C.byref(nb)))
        return f, rows

    @staticmethod
    def _pot_list(pots):
        ids = np.ascontiguousarray([] if pots is None else pots, dtype=np.int32).reshape(-1)
        return ids, (ids.ctypes.data if ids.size else None)

    def forces(self, pots=None, scale: float = 1.0) -> np.ndarray:
        """f[ndofs] = -scale * sum over the listed potential ids of dE/du (None or empty: all potentials); bit-reproducible."""
        ids, ptr = self._pot_list(pots)
        f = np.zeros(self.ndofs)
        self._ck(self.L.mistark_forces(self.h, ptr, ids.size, float(scale), f.ctypes.data))
        return f

    def forces_resultant(self, pots, scale, rows, positions=None, about=(0.0, 0.0, 0.0)) -> np.ndarray:
        """out[6]: the sum of the same forces over the block rows `rows` (list order) and, with `positions` (one per listed row), of their
        moments (positions - about) x f; zeros for the moment otherwise."""
        ids, ptr = self._pot_list(pots)
        r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        pos = None if positions is None else np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        if pos is not None and len(pos) != len(r):
            raise ValueError("one position per listed row")
        ab = np.ascontiguousarray(about, dtype=np.float64).reshape(3)
        out = np.zeros(6)
        self._ck(self.L.mistark_forces_resultant(self.h, ptr, ids.size, float(scale), r.ctypes.data if r.size else None, r.size,
                                                 pos.ctypes.data if pos is not None and pos.size else None, ab.ctypes.data, out.ctypes.data))
        return out

    # ---- stress readout (include/mistark.h "stress readout") ----------------------------------------------------------------
    def element_stress(self, pot: int):
        """(records [n_elem, 16], kind) of one strain potential at the current DoFs; kind 0 tet, 1 triangle, 2 segment. Record layout: mistark.h."""
        ne, kind = C.c_int64(), C.c_int32()
        self._ck(self.L.mistark_potential_element_stress(self.h, pot, None, C.byref(ne), C.byref(kind)))
        rec = np.zeros((ne.value, 16))
        if ne.value:
            self._ck(self.L.mistark_potential_element_stress(self.h, pot, rec.ctypes.data, C.byref(ne), C.byref(kind)))
        return rec, kind.value

    def nodal_stress(self, pots) -> np.ndarray:
        """out[block rows, 10]: rest-measure-weighted averages of record fields 0..8 over the listed potentials (one kind), then the weight sum."""
        ids, ptr = self._pot_list(pots)
        out = np.zeros((self.ndofs // 3, 10))
        self._ck(self.L.mistark_nodal_stress(self.h, ptr, ids.size, out.ctypes.data))
        return out

    # ---- budget readout (include/mistark.h "budget readout") ----------------------------------------------------------------
    def energies(self, pots=None) -> np.ndarray:
        """The energy of each listed potential id at the current DoFs (None or empty: of every potential, in id order); bit-reproducible."""
        ids, ptr = self._pot_list(pots)
        n = ids.size if ids.size else len(self.describe_potentials())
        out = np.zeros(n)
        self._ck(self.L.mistark_energies(self.h, ptr, ids.size, out.ctypes.data if n else None))
        return out

    def describe_potentials(self):
        import json
        n = self.L.mistark_describe(self.h, None, 0)
        buf = C.create_string_buffer(int(n))
        self.L.mistark_describe(self.h, buf, n)
        return json.loads(buf.value.decode())["potentials"]

    def inertia_budget(self, pot: int, n_groups: int, about=(0.0, 0.0, 0.0)) -> np.ndarray:
        """records [n_groups, 13] of an EnergyLumpedInertia potential: mass, first moment, momentum, angular momentum about `about`, kinetic and
        gravitational energy, item count per group (connectivity column 2)."""
        ab = np.ascontiguousarray(about, dtype=np.float64).reshape(3)
        out = np.zeros((int(n_groups), 13))
        self._ck(self.L.mistark_inertia_budget(self.h, int(pot), ab.ctypes.data, int(n_groups), out.ctypes.data if out.size else None))
        return out

    def rigid_budget(self, t0, q0, v1, w1, mass, J_loc, n_bodies: int, about=(0.0, 0.0, 0.0)) -> np.ndarray:
        """records [n_bodies, 13] of the rigid bodies whose state arrays have the given ids (J_loc: 9 doubles per body, row-major, body frame)."""
        ab = np.ascontiguousarray(about, dtype=np.float64).reshape(3)
        out = np.zeros((int(n_bodies), 13))
        self._ck(self.L.mistark_rigid_budget(self.h, int(t0), int(q0), int(v1), int(w1), int(mass), int(J_loc), int(n_bodies), ab.ctypes.data,
                                             out.ctypes.data if out.size else None))
        return out

    # ---- constraint report (include/mistark.h "constraint report") ---------------------------------------------------------
    def constraint_report(self, pot: int, tolerance=None, n_groups=None) -> dict:
        """The row records of a penalty-constraint potential (prescribed positions, attachments, rigid-body constraints) at the current DoFs, columns
        named (constraint_rows_dict). tolerance: one per group, flags rows beyond it; n_groups defaults to its length."""
        tol = None if tolerance is None else np.ascontiguousarray(tolerance, dtype=np.float64).reshape(-1)
        ng = int(n_groups) if n_groups is not None else (0 if tol is None else tol.size)
        if tol is not None and tol.size < ng:
            raise ValueError("constraint_report: %d tolerances for %d groups" % (tol.size, ng))
        tp = tol.ctypes.data if tol is not None and tol.size else None
        n, kind = C.c_int64(), C.c_int32()
        self._ck(self.L.mistark_potential_constraint_report(self.h, int(pot), tp, ng, None, None, None, C.byref(n), C.byref(kind)))
        rec, aux, ids = np.zeros((n.value, 16)), np.zeros((n.value, 2)), np.zeros((n.value, 4), dtype=np.int32)
        if n.value:
            self._ck(self.L.mistark_potential_constraint_report(self.h, int(pot), tp, ng, rec.ctypes.data, aux.ctypes.data, ids.ctypes.data, C.byref(n), C.byref(kind)))
        return constraint_rows_dict(rec, aux, ids, kind.value)

    def constraint_group_report(self, pot: int, n_groups: int, tolerance=None, about=(0.0, 0.0, 0.0)) -> np.ndarray:
        """records [n_groups, 12] of a penalty-constraint potential: rows, active rows, rows beyond tolerance, largest |violation|, position in the
        group's list of the first row attaining it (-1: none), resultant, moment about `about`, energy."""
        tol = None if tolerance is None else np.ascontiguousarray(tolerance, dtype=np.float64).reshape(-1)
        if tol is not None and tol.size < int(n_groups):
            raise ValueError("constraint_group_report: %d tolerances for %d groups" % (tol.size, int(n_groups)))
        ab = np.ascontiguousarray(about, dtype=np.float64).reshape(3)
        out = np.zeros((int(n_groups), 12))
        self._ck(self.L.mistark_constraint_group_report(self.h, int(pot), tol.ctypes.data if tol is not None and tol.size else None, int(n_groups), ab.ctypes.data,
                                                        out.ctypes.data if out.size else None))
        return out

    # ---- rigid-body wrench report (include/mistark.h "rigid-body wrench report") -------------------------------------------
    def rigid_wrench_rows(self, pid: int, v1, w1, t0, q0, n_bodies: int):
        """(records [n_elem, 2, 12], ids [n_elem, 4]) of one potential: per element and body slot F, tau_com, arm, couple along F, |F|, |tau_com|; ids:
        body of slot 0 and 1 (-1: none), number of rigid blocks, flags. v1, w1, t0, q0: array ids of the bodies' state."""
        n = C.c_int64()
        args = (int(pid), int(v1), int(w1), int(t0), int(q0), int(n_bodies))
        self._ck(self.L.mistark_potential_rigid_wrench(self.h, *args, None, None, C.byref(n)))
        rec, ids = np.zeros((n.value, 2, 12)), np.zeros((n.value, 4), dtype=np.int32)
        if n.value:
            self._ck(self.L.mistark_potential_rigid_wrench(self.h, *args, rec.ctypes.data, ids.ctypes.data, C.byref(n)))
        return rec, ids

    def rigid_wrench(self, families, v1, w1, t0, q0, n_bodies: int, about=(0.0, 0.0, 0.0)):
        """(records [n_families, n_bodies, 16], counts [n_families, n_bodies]) for families of potential ids (a list of lists; an empty list: every
        potential, the unbalanced wrench): F, tau_com, torque about `about`, -dE/dw1 / dt, t1, |a|; counts: active elements touching the body."""
        fams = [np.ascontiguousarray([] if f is None else f, dtype=np.int32).reshape(-1) for f in families]
        start = np.zeros(len(fams) + 1, dtype=np.int32)
        start[1:] = np.cumsum([f.size for f in fams])
        flat = np.ascontiguousarray(np.concatenate(fams) if fams else [], dtype=np.int32)
        ab = np.ascontiguousarray(about, dtype=np.float64).reshape(3)
        out = np.zeros((len(fams), int(n_bodies), 16))
        cnt = np.zeros((len(fams), int(n_bodies)), dtype=np.int32)
        self._ck(self.L.mistark_rigid_wrench(self.h, flat.ctypes.data if flat.size else None, start.ctypes.data, len(fams), int(v1), int(w1), int(t0), int(q0),
                                             int(n_bodies), ab.ctypes.data, out.ctypes.data if out.size else None, cnt.ctypes.data if cnt.size else None))
        return out, cnt

    # ---- bending report (include/mistark.h "bending report") ---------------------------------------------------------------
    @staticmethod
    def _thresholds(threshold, n_groups, who):
        thr = None if threshold is None else np.ascontiguousarray(threshold, dtype=np.float64).reshape(-1)
        ng = int(n_groups) if n_groups is not None else (0 if thr is None else thr.size)
        if thr is not None and thr.size < ng:
            raise ValueError("%s: %d thresholds for %d groups" % (who, thr.size, ng))
        return thr, ng, (thr.ctypes.data if thr is not None and thr.size else None)

    def bending_report(self, pot: int, threshold=None, n_groups=None) -> dict:
        """The row records of a cloth bending potential (EnergyDiscreteShells: kind 0, EnergyBendingFlat: kind 1) at the current DoFs, columns named
        (bending_rows_dict). threshold: one per group in rad, flags hinges whose |theta1 - rest| exceeds it; n_groups defaults to its length."""
        thr, ng, tp = self._thresholds(threshold, n_groups, "bending_report")
        n, kind = C.c_int64(), C.c_int32()
        self._ck(self.L.mistark_potential_bending_report(self.h, int(pot), tp, ng, None, C.byref(n), C.byref(kind)))
        rec = np.zeros((n.value, 16))
        if n.value:
            self._ck(self.L.mistark_potential_bending_report(self.h, int(pot), tp, ng, rec.ctypes.data, C.byref(n), C.byref(kind)))
        return bending_rows_dict(rec, kind.value)

    def nodal_bending(self, pots) -> np.ndarray:
        """out[block rows, 6] over the listed bending potentials (both kinds may be listed together): area-weighted mean kappa, mean kappa - kappa_rest,
        energy share, largest |theta1 - rest|, hinges ending at the node, weight sum."""
        ids, ptr = self._pot_list(pots)
        out = np.zeros((self.ndofs // 3, 6))
        self._ck(self.L.mistark_nodal_bending(self.h, ptr, ids.size, out.ctypes.data))
        return out

    def bending_group_report(self, pot: int, n_groups: int, threshold=None) -> np.ndarray:
        """records [n_groups, 10] of a cloth bending potential: hinges, degenerate, beyond threshold, largest |theta1 - rest|, position in the group's list
        of the first row attaining it (-1: none), elastic energy, damping energy, area, sum a (kappa - kappa_rest)^2, area-weighted mean |kappa - kappa_rest|."""
        thr, ng, tp = self._thresholds(threshold, n_groups, "bending_group_report")
        out = np.zeros((ng, 10))
        self._ck(self.L.mistark_bending_group_report(self.h, int(pot), tp, ng, out.ctypes.data if out.size else None))
        return out

    # ---- Hessian spectrum report (include/mistark.h "Hessian spectrum report") ------------------------------------------------
    def spectrum_report(self, pot: int, source: int = 0, eps: float = 1e-10, spectrum: bool = False) -> dict:
        """The element records of one potential's Hessian spectra, columns named (spectrum_rows_dict). source 0: the element Hessians as they stand
        after eval(P_G_H) / project(); 1: a fresh evaluation at the current DoFs beside eval(). spectrum=True adds the sorted eigenvalues [n_elem, 3 NB]."""
        n, nb = C.c_int64(), C.c_int32()
        self._ck(self.L.mistark_potential_spectrum_report(self.h, int(pot), int(source), float(eps), None, None, C.byref(n), C.byref(nb)))
        rec = np.zeros((n.value, 10))
        spec = np.zeros((n.value, 3 * nb.value)) if spectrum else None
        if n.value:
            self._ck(self.L.mistark_potential_spectrum_report(self.h, int(pot), int(source), float(eps), rec.ctypes.data, spec.ctypes.data if spectrum else None,
                                                               C.byref(n), C.byref(nb)))
        return spectrum_rows_dict(rec, nb.value, spec)

    def nodal_spectrum(self, pots, source: int = 0, eps: float = 1e-10) -> np.ndarray:
        """out[block rows, 5] over the listed potentials: elements touching the row, of them flagged (the projection would change them), smallest
        lambda_min among them, sum of deficit^2, potential id holding the smallest (-1: none)."""
        ids, ptr = self._pot_list(pots)
        out = np.zeros((self.ndofs // 3, 5))
        self._ck(self.L.mistark_nodal_spectrum(self.h, ptr, ids.size, int(source), float(eps), out.ctypes.data))
        return out

    def spectrum_potential_report(self, pots, source: int = 0, eps: float = 1e-10) -> np.ndarray:
        """records [len(pots), 10]: elements, flagged, with lambda_min < 0, non-finite, not converged, smallest lambda_min, first element attaining it
        (-1: none), largest lambda_max, sqrt(sum deficit^2), first non-finite element (-1: none)."""
        ids, ptr = self._pot_list(pots)
        out = np.zeros((ids.size, 10))
        self._ck(self.L.mistark_spectrum_potential_report(self.h, ptr, ids.size, int(source), float(eps), out.ctypes.data if out.size else None))
        return out

    # ---- linear-system report (include/mistark.h "linear-system report") -------------------------------------------------------
    def _linsys_start(self, start):
        """None: the built-in vector; "rhs": minus the gradient of the last evaluation; otherwise ndofs doubles in DoF order."""
        if start is None:
            return None, None
        if isinstance(start, str):
            if start != "rhs":
                raise ValueError("start is None, 'rhs' or an array")
            v = np.zeros(self.ndofs)
            self._ck(self.L.mistark_linsys_rhs(self.h, v.ctypes.data))
        else:
            v = np.ascontiguousarray(start, dtype=np.float64).reshape(-1)
            if v.size != self.ndofs:
                raise ValueError("start has %d entries, the system %d" % (v.size, self.ndofs))
        return v, v.ctypes.data

    def linsys_report(self, op: int = 1, m: int = 64, start=None) -> "LinsysReport":
        """Lanczos with full reorthogonalisation on the assembled matrix (op 0: A; 1: the block-Jacobi preconditioned matrix), m steps at the most:
        the summary record as named fields, ritz [k, 2] (theta ascending, rho) and tri [k, 2] (alpha_j, beta_j)."""
        v, ptr = self._linsys_start(start)
        mm = max(int(m), 1)
        out, ritz, tri, k = np.zeros(16), np.zeros((mm, 2)), np.zeros((mm, 2)), C.c_int32()
        self._ck(self.L.mistark_linsys_report(self.h, int(op), int(m), ptr, out.ctypes.data, ritz.ctypes.data, tri.ctypes.data, C.byref(k)))
        return LinsysReport(out, ritz[:k.value].copy(), tri[:k.value].copy())

    def linsys_modes(self, which=(0, -1), op: int = 1, m: int = 64, start=None, x: bool = True, nodal: bool = True) -> dict:
        """Ritz vectors of the same run: which[i] >= 0 the i-th smallest Ritz value, < 0 counted from the largest. dict(mode [n, 4]: theta, rho, measured
        residual, index; x [n, ndofs] with x^T D x = 1 (op 1) or |x| = 1 (op 0), DoF order; nodal [n, block rows, 4]: share, |x_r|, trace D_r, smallest
        squared pivot of D_r)."""
        v, ptr = self._linsys_start(start)
        w = np.ascontiguousarray(which, dtype=np.int32).reshape(-1)
        mode = np.zeros((w.size, 4))
        xs = np.zeros((w.size, self.ndofs)) if x else None
        nd = np.zeros((w.size, self.ndofs // 3, 4)) if nodal else None
        self._ck(self.L.mistark_linsys_modes(self.h, int(op), int(m), ptr, w.ctypes.data if w.size else None, w.size, xs.ctypes.data if x and xs.size else None,
                                             nd.ctypes.data if nodal and nd.size else None, mode.ctypes.data if mode.size else None))
        return dict(mode=mode, theta=mode[:, 0], rho=mode[:, 1], residual=mode[:, 2], index=mode[:, 3].astype(np.int64), x=xs, nodal=nd)

    def linsys_potential_shares(self, pots, which: int = 0, op: int = 1, m: int = 64, start=None) -> np.ndarray:
        """out[len(pots), 4] for one Ritz vector x: sum of q_e = x_e^T H_e x_e over the potential's element Hessians as they stand, sum |q_e|, elements
        that contribute, first element attaining the largest |q_e| (-1: none). Over all potentials column 0 adds up to theta."""
        v, ptr = self._linsys_start(start)
        ids, iptr = self._pot_list(pots)
        out = np.zeros((ids.size, 4))
        self._ck(self.L.mistark_linsys_potential_shares(self.h, int(op), int(m), ptr, int(which), iptr, ids.size, out.ctypes.data if out.size else None))
        return out

    def direct_llt(self, rhs):
        """x = A^-1 rhs by the device Cholesky (mistark_direct_llt_rhs); returns (x, success)."""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.zeros(self.ndofs)
        ok = C.c_int()
        self._ck(self.L.mistark_direct_llt_rhs(self.h, rhs.ctypes.data, x.ctypes.data, C.byref(ok)))
        return x, bool(ok.value)

    def project(self, eps=1e-10, mirroring=False, active_blocks=None):
        npj, nch = C.c_int64(), C.c_int64()
        ab = None
        if active_blocks is not None:
            ab = np.ascontiguousarray(active_blocks, dtype=np.uint8)
        self._ck(self.L.mistark_project(self.h, eps, int(mirroring), ab.ctypes.data if ab is not None else None, C.byref(npj), C.byref(nch)))
        return npj.value, nch.value

    def assemble(self):
        self._ck(self.L.mistark_assemble(self.h))

    def get_bsr(self, with_vals=True):
        nbr, nnzb = C.c_int64(), C.c_int64()
        self._ck(self.L.mistark_get_bsr(self.h, C.byref(nbr), C.byref(nnzb), None, None, None))
        row_ptr = np.zeros(nbr.value + 1, dtype=np.int64)
        cols = np.zeros(nnzb.value, dtype=np.int32)
        vals = np.zeros((nnzb.value, 3, 3), dtype=np.float32)
        self._ck(self.L.mistark_get_bsr(self.h, C.byref(nbr), C.byref(nnzb), row_ptr.ctypes.data, cols.ctypes.data, vals.ctypes.data if with_vals else None))
        return row_ptr, cols, vals

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        self._ck(self.L.mistark_spmv(self.h, x.ctypes.data, y.ctypes.data))
        return y

    def apply_preconditioner(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        z = np.zeros_like(x)
        self._ck(self.L.mistark_apply_preconditioner(self.h, x.ctypes.data, z.ctypes.data))
        return z

    def pcg(self, abs_tol, rel_tol=1e-4, max_iter=10000, stop_on_indef=True, rhs=None):
        info = capi.PcgInfo()
        x = np.zeros(self.ndofs)
        if rhs is None:
            self._ck(self.L.mistark_pcg(self.h, abs_tol, rel_tol, max_iter, int(stop_on_indef), x.ctypes.data, C.byref(info)))
        else:
            rhs = np.ascontiguousarray(rhs, dtype=np.float64)
            self._ck(self.L.mistark_pcg_rhs(self.h, rhs.ctypes.data, abs_tol, rel_tol, max_iter, int(stop_on_indef), x.ctypes.data, C.byref(info)))
        return x, info

    def default_newton_settings(self):
        s = capi.NewtonSettings()
        self.L.mistark_newton_default_settings(C.byref(s))
        return s

    def newton_solve(self, settings=None, callbacks=None):
        st = capi.NewtonStats()
        s = settings if settings is not None else self.default_newton_settings()
        rc = self._ck(self.L.mistark_newton_solve(self.h, C.byref(s), C.byref(callbacks) if callbacks is not None else None, C.byref(st)))
        return capi.SOLVER_RETURN[rc], st

    def newton_iteration_log(self):
        """Per-iteration records of the last newton_solve (capi.NewtonIteration)."""
        n = C.c_int32()
        self._ck(self.L.mistark_newton_iteration_log(self.h, None, 0, C.byref(n)))
        rec = (capi.NewtonIteration * max(n.value, 1))()
        self._ck(self.L.mistark_newton_iteration_log(self.h, rec, n.value, C.byref(n)))
        return list(rec)[:n.value]

    def counter(self, name: str) -> int:
        """mistark_get_counter: event counters of the context (tests assert that a feature under test actually ran)."""
        v = C.c_int64()
        self._ck(self.L.mistark_get_counter(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def set_option(self, name: str, value: int):
        self._ck(self.L.mistark_set_option(self.h, name.encode(), int(value)))

    def spmv_timing(self, reset=0):
        ms, n, b = C.c_double(), C.c_int64(), C.c_double()
        self._ck(self.L.mistark_spmv_timing(self.h, reset, C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value


def contact_rows_dict(ri, rd):
    """The row arrays of a contact report with their columns named (views)."""
    bounds = np.searchsorted(ri[:, 0], np.arange(22), side="left")
    return dict(ints=ri, doubles=rd, bounds=bounds, table=ri[:, 0], source=ri[:, 1], type=ri[:, 2], group_a=ri[:, 3], group_b=ri[:, 4], prim_a=ri[:, 5], prim_b=ri[:, 6],
                flags=ri[:, 7], d=rd[:, 0], dhat=rd[:, 1], point_a=rd[:, 2:5], point_b=rd[:, 5:8], normal=rd[:, 8:11], mollifier=rd[:, 11], fn=rd[:, 12], E=rd[:, 13],
                params=rd[:, 14:16])


CONSTRAINT_KINDS = ("EnergyPrescribedPositions", "rb_constraint_global_points", "rb_constraint_global_directions", "rb_constraint_points", "rb_constraint_point_on_axis",
                    "rb_constraint_distances", "rb_constraint_distance_limits", "rb_constraint_directions", "rb_constraint_angle_limits", "rb_constraint_damped_spring",
                    "rb_constraint_linear_velocity", "rb_constraint_angular_velocity", "EnergyAttachments_d_d_p_p", "EnergyAttachments_d_d_p_e", "EnergyAttachments_d_d_p_t",
                    "EnergyAttachments_d_d_e_e", "EnergyAttachments_rb_d")
CONSTRAINT_UNITS = ("m", "m", "deg", "m", "m", "m", "m", "deg", "deg", "m", "m/s", "deg/s", "m", "m", "m", "m", "m")


def constraint_rows_dict(rec, aux, ids, kind):
    """The row arrays of a constraint report with their columns named (views; flags as integers)."""
    flags = rec[:, 15].astype(np.int64)
    return dict(records=rec, aux=aux, ids=ids, kind=int(kind), name=CONSTRAINT_KINDS[kind] if 0 <= kind < 17 else None, unit=CONSTRAINT_UNITS[kind] if 0 <= kind < 17 else None,
                violation=rec[:, 0], reaction=rec[:, 1], force=rec[:, 2:5], torque=rec[:, 5:8], anchor_a=rec[:, 8:11], anchor_b=rec[:, 11:14], E=rec[:, 14], flags=flags,
                active=(flags & 1) != 0, beyond_tolerance=(flags & 2) != 0, out_of_range=(flags & 4) != 0, damper_velocity=aux[:, 0], damper_force=aux[:, 1],
                group=ids[:, 0], row_a=ids[:, 2], row_b=ids[:, 3])


BENDING_KINDS = ("EnergyDiscreteShells", "EnergyBendingFlat")


def bending_rows_dict(rec, kind):
    """The row array of a bending report with its columns named (views; flags and group as integers)."""
    flags = rec[:, 15].astype(np.int64)
    return dict(records=rec, kind=int(kind), name=BENDING_KINDS[kind] if 0 <= kind < 2 else None, theta=rec[:, 0], phi=rec[:, 1], rest_angle=rec[:, 2], rate=rec[:, 3],
                length=rec[:, 4], area=rec[:, 5], kappa=rec[:, 6], kappa_rest=rec[:, 7], moment=rec[:, 8], E_elastic=rec[:, 9], E_damping=rec[:, 10], normal=rec[:, 11:14],
                group=rec[:, 14].astype(np.int64), flags=flags, degenerate=(flags & 1) != 0, beyond_threshold=(flags & 2) != 0)


class LinsysReport:
    """The summary record of a linear-system report as named fields (record: the 16 doubles), with the Ritz list and the tridiagonal coefficients."""
    FIELDS = ("k", "flags", "theta_min", "rho_min", "theta_max", "rho_max", "condition", "t_norm", "beta_last", "n_negative", "n_converged", "n_diag_not_pd",
              "first_diag_not_pd", "min_pivot", "min_pivot_row", "n")
    INTEGERS = ("k", "flags", "n_negative", "n_converged", "n_diag_not_pd", "first_diag_not_pd", "min_pivot_row", "n")

    def __init__(self, record, ritz=None, tri=None):
        self.record = np.asarray(record, dtype=np.float64)
        self.ritz, self.tri = ritz, tri
        for i, f in enumerate(self.FIELDS):
            setattr(self, f, int(self.record[i]) if f in self.INTEGERS else float(self.record[i]))
        self.exhausted = bool(self.flags & 1)
        self.indefinite = bool(self.flags & 2)
        self.non_finite = bool(self.flags & 4)
        self.diag_not_pd = bool(self.flags & 8)

    def __repr__(self):
        return "LinsysReport(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f in self.FIELDS)


def spectrum_rows_dict(rec, nb, spectrum=None):
    """The element array of a spectrum report with its columns named (views; counts and flags as integers)."""
    flags = rec[:, 9].astype(np.int64)
    return dict(records=rec, nb=int(nb), lambda_min=rec[:, 0], lambda_max=rec[:, 1], n_below_eps=rec[:, 2].astype(np.int64), n_negative=rec[:, 3].astype(np.int64),
                deficit=rec[:, 4], frobenius=rec[:, 5], trace=rec[:, 6], sweeps=rec[:, 7].astype(np.int64), off=rec[:, 8], flags=flags, projected=(flags & 1) != 0,
                non_finite=(flags & 2) != 0, not_converged=(flags & 4) != 0, spectrum=spectrum)


def contact_vertices_dict(rec, group, source_index):
    """The vertex records of a contact report with their columns named (views; count as integers)."""
    return dict(records=rec, gap=rec[:, 0], count=rec[:, 1].astype(np.int64), force=rec[:, 2], area=rec[:, 3], pressure=rec[:, 4], group=group, source_index=source_index)


def friction_rows_dict(ri, rd):
    """The row arrays of a friction report with their columns named (views)."""
    bounds = np.searchsorted(ri[:, 0], 21 + np.arange(15), side="left")
    return dict(ints=ri, doubles=rd, bounds=bounds, table=ri[:, 0], row=ri[:, 1], kind=ri[:, 2], group_a=ri[:, 3], group_b=ri[:, 4], body_a=ri[:, 5], body_b=ri[:, 6],
                flags=ri[:, 7], mu=rd[:, 0], fn=rd[:, 1], epsu=rd[:, 2], u=rd[:, 3:5], slip=rd[:, 5], slip_speed=rd[:, 6], v=rd[:, 7:10], ft=rd[:, 10:13], ft_norm=rd[:, 13],
                mobilised=rd[:, 14], dissipation=rd[:, 15], E=rd[:, 16], param_a=rd[:, 17], weights_b=rd[:, 18:21])


def friction_vertices_dict(rec, group, source_index):
    """The vertex records of a friction report with their columns named (views; counts as integers)."""
    return dict(records=rec, count=rec[:, 0].astype(np.int64), sliding=rec[:, 1].astype(np.int64), force=rec[:, 2:5], slip_speed=rec[:, 5], area=rec[:, 6],
                traction=rec[:, 7], group=group, source_index=source_index)
