"""ctypes binding of the scene-level C facade (include/mistark_sim.h) over the C++ host mirror of stark::Simulation."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


class SimSettings(C.Structure):
    _fields_ = [("gravity", C.c_double * 3), ("max_time_step_size", C.c_double), ("use_adaptive_time_step", C.c_int32),
                ("time_step_size_success_multiplier", C.c_double), ("time_step_size_lower_bound", C.c_double), ("device", C.c_int32),
                ("mirror_state_to_host", C.c_int32), ("enable_output", C.c_int32), ("init_frictional_contact", C.c_int32), ("newton", capi.NewtonSettings),
                ("enable_frame_writes", C.c_int32), ("fps", C.c_int32), ("output_directory", C.c_char * 256), ("simulation_name", C.c_char * 64),
                ("allowed_execution_time", C.c_double), ("end_simulation_time", C.c_double), ("end_frame", C.c_int32)]


class VolumeParams(C.Structure):
    _fields_ = [("density", C.c_double), ("inertia_damping", C.c_double), ("quasistatic", C.c_int32), ("elasticity_only", C.c_int32), ("scale", C.c_double),
                ("youngs_modulus", C.c_double), ("poissons_ratio", C.c_double), ("strain_damping", C.c_double), ("strain_limit", C.c_double),
                ("strain_limit_stiffness", C.c_double)]


class SurfaceParams(C.Structure):
    _fields_ = [("density", C.c_double), ("inertia_damping", C.c_double), ("quasistatic", C.c_int32), ("elasticity_only", C.c_int32), ("scale", C.c_double),
                ("thickness", C.c_double), ("youngs_modulus", C.c_double), ("poissons_ratio", C.c_double), ("strain_damping", C.c_double),
                ("strain_limit", C.c_double), ("strain_limit_stiffness", C.c_double), ("inflation", C.c_double), ("bending_stiffness", C.c_double),
                ("bending_damping", C.c_double), ("flat_rest_angle", C.c_int32)]


class LineParams(C.Structure):
    _fields_ = [("density", C.c_double), ("inertia_damping", C.c_double), ("quasistatic", C.c_int32), ("elasticity_only", C.c_int32), ("scale", C.c_double),
                ("section_radius", C.c_double), ("youngs_modulus", C.c_double), ("strain_damping", C.c_double), ("strain_limit", C.c_double),
                ("strain_limit_stiffness", C.c_double)]


class ContactGlobalParams(C.Structure):
    _fields_ = [("default_contact_thickness", C.c_double), ("min_contact_stiffness", C.c_double), ("max_contact_stiffness", C.c_double),
                ("friction_stick_slide_threshold", C.c_double), ("collisions_enabled", C.c_int32), ("friction_enabled", C.c_int32),
                ("triangle_point_enabled", C.c_int32), ("edge_edge_enabled", C.c_int32), ("intersection_test_enabled", C.c_int32)]


class SimInfo(C.Structure):
    _fields_ = [("current_time", C.c_double), ("dt", C.c_double), ("current_time_step", C.c_int32), ("last_newton_result", C.c_int32), ("n_points", C.c_int64),
                ("ndofs", C.c_int64), ("total_newton_iterations", C.c_int64), ("total_cg_iterations", C.c_int64), ("total_linear_solves", C.c_int64),
                ("failed_steps", C.c_int64), ("total_newton_time", C.c_double), ("total_linear_solve_time", C.c_double), ("total_eval_pgh_time", C.c_double),
                ("total_eval_p_time", C.c_double), ("total_project_time", C.c_double), ("total_assembly_time", C.c_double), ("total_callback_time", C.c_double),
                ("total_step_time", C.c_double), ("total_evaluations", C.c_int64), ("last_stats", capi.NewtonStats)]


_bound = False


def _lib():
    global _bound
    L = capi.lib()
    if not _bound:
        p = C.c_void_p
        L.mistark_sim_default_settings.argtypes = [C.POINTER(SimSettings)]
        L.mistark_sim_default_settings.restype = None
        L.mistark_volume_params_soft_rubber.argtypes = [C.POINTER(VolumeParams)]
        L.mistark_volume_params_soft_rubber.restype = None
        L.mistark_surface_params_cotton_fabric.argtypes = [C.POINTER(SurfaceParams)]
        L.mistark_surface_params_cotton_fabric.restype = None
        L.mistark_sim_rb_fix_set_transformation.argtypes = [p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.mistark_sim_create.argtypes = [C.POINTER(SimSettings), C.POINTER(p)]
        L.mistark_sim_destroy.argtypes = [p]
        L.mistark_sim_destroy.restype = None
        L.mistark_sim_last_error.argtypes = [p]
        L.mistark_sim_last_error.restype = C.c_char_p
        L.mistark_sim_add_volume_grid.argtypes = [p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(VolumeParams)]
        L.mistark_sim_add_volume.argtypes = [p, C.c_char_p, p, C.c_int64, p, C.c_int64, C.POINTER(VolumeParams)]
        L.mistark_sim_add_surface_grid.argtypes = [p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(SurfaceParams)]
        L.mistark_sim_add_surface.argtypes = [p, C.c_char_p, p, C.c_int64, p, C.c_int64, C.POINTER(SurfaceParams)]
        L.mistark_sim_prescribe_inside_aabb.argtypes = [p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double]
        L.mistark_sim_prescribe_outside_aabb.argtypes = [p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double]
        L.mistark_sim_prescribe_points.argtypes = [p, C.c_int, p, C.c_int64, C.c_double, C.c_double]
        L.mistark_line_params_elastic_rubberband.argtypes = [C.POINTER(LineParams)]
        L.mistark_line_params_elastic_rubberband.restype = None
        L.mistark_sim_add_line.argtypes = [p, C.c_char_p, p, C.c_int64, p, C.c_int64, C.POINTER(LineParams)]
        L.mistark_sim_add_line_as_segments.argtypes = [p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.POINTER(LineParams)]
        L.mistark_sim_attach_point_point.argtypes = [p, C.c_int, C.c_int, p, p, C.c_int64, C.c_double, C.c_double]
        L.mistark_sim_attach_point_edge.argtypes = [p, C.c_int, C.c_int, p, p, p, C.c_int64, C.c_double, C.c_double]
        L.mistark_sim_attach_point_triangle.argtypes = [p, C.c_int, C.c_int, p, p, p, C.c_int64, C.c_double, C.c_double]
        L.mistark_sim_attach_edge_edge.argtypes = [p, C.c_int, C.c_int, p, p, p, p, C.c_int64, C.c_double, C.c_double]
        L.mistark_sim_attach_rigid_body.argtypes = [p, C.c_int, C.c_int, p, p, C.c_int64, C.c_double, C.c_double]
        L.mistark_sim_attach_by_distance.argtypes = [p, C.c_int, C.c_int, p, C.c_int64, p, C.c_int64, C.c_double, C.c_double, C.c_double, p]
        L.mistark_sim_attach_rigid_body_by_distance.argtypes = [p, C.c_int, C.c_int, p, C.c_int64, p, C.c_int64, p, C.c_int64, C.c_double, C.c_double, C.c_double]
        L.mistark_sim_attachment_stiffness.argtypes = [p, C.c_int, C.POINTER(C.c_double)]
        L.mistark_sim_run_one_step.argtypes = [p]
        L.mistark_sim_set_newton_settings.argtypes = [p, C.POINTER(capi.NewtonSettings)]
        L.mistark_sim_add_max_allowed_step.argtypes = [p, capi.DBLCB, C.c_void_p]
        L.mistark_sim_prepare.argtypes = [p]
        L.mistark_sim_begin_time_step.argtypes = [p]
        L.mistark_sim_before_energy_evaluation.argtypes = [p]
        L.mistark_sim_engine.argtypes = [p]
        L.mistark_sim_engine.restype = p
        L.mistark_sim_get_info.argtypes = [p, C.POINTER(SimInfo)]
        L.mistark_sim_get_points.argtypes = [p, C.c_int, p]
        L.mistark_sim_set_points.argtypes = [p, C.c_int, p]
        D = C.POINTER(C.c_double)
        L.mistark_sim_point_set_add_displacement.argtypes = [p, C.c_int, D]
        L.mistark_sim_point_set_add_rotation.argtypes = [p, C.c_int, C.c_double, D, D]
        L.mistark_sim_add_rigid_box.argtypes = [p, C.c_char_p, C.c_double, D]
        L.mistark_sim_rb_set_translation.argtypes = [p, C.c_int, D]
        L.mistark_sim_rb_add_translation.argtypes = [p, C.c_int, D]
        L.mistark_sim_rb_add_rotation.argtypes = [p, C.c_int, C.c_double, D, D]
        L.mistark_sim_rb_set_velocity.argtypes = [p, C.c_int, D, D]
        L.mistark_sim_rb_set_default_constraint_params.argtypes = [p, C.c_double, C.c_double, C.c_double]
        L.mistark_sim_rb_add_constraint.argtypes = [p, C.c_char_p, C.c_int, C.c_int, D, C.c_int]
        L.mistark_sim_rb_get_state.argtypes = [p, C.c_int, p, p, p, p]
        L.mistark_sim_rb_add.argtypes = [p, C.c_double, D]
        L.mistark_inertia_tensor_box.argtypes = [C.c_double, D, D]
        L.mistark_inertia_tensor_box.restype = None
        L.mistark_sim_rb_add_force_at_centroid.argtypes = [p, C.c_int, D]
        L.mistark_sim_rb_add_torque.argtypes = [p, C.c_int, D]
        L.mistark_sim_rb_constraint_count.argtypes = [p, C.c_char_p]
        L.mistark_sim_rb_constraint_measure.argtypes = [p, C.c_char_p, C.c_int, C.c_int, D, D]
        L.mistark_sim_run.argtypes = [p, C.c_double]
        L.mistark_contact_default_global_params.argtypes = [C.POINTER(ContactGlobalParams)]
        L.mistark_contact_default_global_params.restype = None
        L.mistark_sim_set_contact_global_params.argtypes = [p, C.POINTER(ContactGlobalParams)]
        L.mistark_sim_contact_group.argtypes = [p, C.c_int, C.c_int]
        L.mistark_sim_set_friction.argtypes = [p, C.c_int, C.c_int, C.c_double]
        L.mistark_sim_disable_collision.argtypes = [p, C.c_int, C.c_int]
        L.mistark_sim_set_dist_rccl.argtypes = [p, C.c_int, C.c_int, p]
        L.mistark_sim_set_dist_local.argtypes = [p, p, C.c_int, C.c_int]
        L.mistark_sim_set_dist_ipc.argtypes = [p, p, C.c_int, C.c_int]
        L.mistark_sim_get_contact_info.argtypes = [p, D, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.mistark_sim_set_contact_ccd.argtypes = [p, C.c_int, C.c_double]
        I64 = C.POINTER(C.c_int64)
        L.mistark_sim_get_ccd_info.argtypes = [p, I64, I64, I64, I64, I64, D]
        L.mistark_sim_set_contact_ccd_rigid.argtypes = [p, C.c_int, C.c_int]
        L.mistark_sim_get_ccd_rigid_info.argtypes = [p, C.POINTER(C.c_int), I64, I64, D]
        L.mistark_sim_record_forces.argtypes = [p, C.c_char_p]
        L.mistark_sim_get_forces.argtypes = [p, C.c_int, p, p]
        L.mistark_sim_record_stress.argtypes = [p, C.c_int]
        L.mistark_sim_get_stress.argtypes = [p, C.c_int, p, C.POINTER(C.c_int64)]
        L.mistark_sim_get_nodal_stress.argtypes = [p, C.c_int, p]
        L.mistark_sim_record_budget.argtypes = [p, C.c_int, D]
        I32 = C.POINTER(C.c_int32)
        L.mistark_sim_get_budget.argtypes = [p, I32, I32, I64, I64, D, p, p, p, p, p]
        L.mistark_sim_record_contacts.argtypes = [p, C.c_int]
        L.mistark_sim_get_contacts.argtypes = [p, I64, I64, I32, I64, D, p, p, p, p, p, p, p]
        L.mistark_sim_record_constraints.argtypes = [p, C.c_int, D]
        L.mistark_sim_get_constraints.argtypes = [p, C.c_int, I32, I64, I32, I32, D, p, p, p, p, p]
        L.mistark_sim_record_bending.argtypes = [p, C.c_int, C.c_double]
        L.mistark_sim_get_bending.argtypes = [p, C.c_int, I32, I64, I32, D, p, p]
        L.mistark_sim_get_nodal_bending.argtypes = [p, p]
        L.mistark_sim_record_spectrum.argtypes = [p, C.c_int, C.c_double]
        L.mistark_sim_get_spectrum.argtypes = [p, I32, I64, D, D, p, p]
        L.mistark_sim_get_nodal_spectrum.argtypes = [p, p]
        L.mistark_sim_get_spectrum_rows.argtypes = [p, C.c_char_p, I64, p, C.c_int64]
        L.mistark_sim_record_linsys.argtypes = [p, C.c_int, C.c_int, C.c_int]
        L.mistark_sim_get_linsys.argtypes = [p, I32, I32, D, p, p]
        L.mistark_sim_record_wrench.argtypes = [p, C.c_int, p]
        L.mistark_sim_wrench_sources.argtypes = [p, p, p, p]
        L.mistark_sim_get_wrench.argtypes = [p, I32, I32, I64, D, p, p, p]
        L.mistark_sim_record_friction.argtypes = [p, C.c_int]
        L.mistark_sim_get_friction.argtypes = [p, I64, I64, I32, I64, D, p, p, p, p, p, p, p]
        _bound = True
    return L


def default_settings() -> SimSettings:
    s = SimSettings()
    _lib().mistark_sim_default_settings(C.byref(s))
    return s


def soft_rubber() -> VolumeParams:
    p = VolumeParams()
    _lib().mistark_volume_params_soft_rubber(C.byref(p))
    return p


def cotton_fabric() -> SurfaceParams:
    p = SurfaceParams()
    _lib().mistark_surface_params_cotton_fabric(C.byref(p))
    return p


def elastic_rubberband() -> LineParams:
    p = LineParams()
    _lib().mistark_line_params_elastic_rubberband(C.byref(p))
    return p


def inertia_tensor_box(mass, size) -> np.ndarray:
    out = (C.c_double * 9)()
    _lib().mistark_inertia_tensor_box(float(mass), _d3(size), out)
    return np.array(out[:]).reshape(3, 3)


def generate_triangle_grid(center, dim, subdivisions):
    """stark::generate_triangle_grid: (vertices [n, 3], triangles [m, 3])."""
    L = _lib()
    L.mistark_generate_triangle_grid.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64)]
    nv, nt = C.c_int64(), C.c_int64()
    assert L.mistark_generate_triangle_grid(_d3(center), _d3(dim), _i3(subdivisions), None, C.byref(nv), None, C.byref(nt)) == 0
    V, T = np.zeros((nv.value, 3)), np.zeros((nt.value, 3), dtype=np.int32)
    assert L.mistark_generate_triangle_grid(_d3(center), _d3(dim), _i3(subdivisions), V.ctypes.data, C.byref(nv), T.ctypes.data, C.byref(nt)) == 0
    return V, T


def find_edges_from_triangles(triangles, n_vertices):
    """stark::find_edges_from_simplices for triangles: unique edges [k, 2] in the reference's order."""
    L = _lib()
    L.mistark_find_edges_from_triangles.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]
    T = np.ascontiguousarray(triangles, dtype=np.int32)
    ne = C.c_int64()
    assert L.mistark_find_edges_from_triangles(T.ctypes.data, len(T), n_vertices, None, C.byref(ne)) == 0
    E = np.zeros((ne.value, 2), dtype=np.int32)
    assert L.mistark_find_edges_from_triangles(T.ctypes.data, len(T), n_vertices, E.ctypes.data, C.byref(ne)) == 0
    return E


def contact_global_params() -> ContactGlobalParams:
    p = ContactGlobalParams()
    _lib().mistark_contact_default_global_params(C.byref(p))
    return p


def _d3(v):
    return (C.c_double * len(v))(*[float(x) for x in v])


def _i3(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


class SimError(RuntimeError):
    pass


class Simulation:
    """Mirror of stark::Simulation for the hot-path subset (deformables + presets)."""

    def __init__(self, settings: SimSettings | None = None):
        self.L = _lib()
        h = C.c_void_p()
        s = settings if settings is not None else default_settings()
        if self.L.mistark_sim_create(C.byref(s), C.byref(h)) != 0:
            raise SimError("mistark_sim_create failed")
        self.h = h

    def close(self):
        if self.h:
            self.L.mistark_sim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise SimError(self.L.mistark_sim_last_error(self.h).decode())
        return rc

    def add_volume_grid(self, label, center, dim, subdivisions, params: VolumeParams) -> int:
        return self._ck(self.L.mistark_sim_add_volume_grid(self.h, label.encode(), _d3(center), _d3(dim), _i3(subdivisions), C.byref(params)))

    def add_surface_grid(self, label, dim, subdivisions, params: SurfaceParams) -> int:
        return self._ck(self.L.mistark_sim_add_surface_grid(self.h, label.encode(), _d3(dim), _i3(subdivisions), C.byref(params)))

    def add_volume(self, label, vertices, tets, params: VolumeParams) -> int:
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        t = np.ascontiguousarray(tets, dtype=np.int32)
        return self._ck(self.L.mistark_sim_add_volume(self.h, label.encode(), v.ctypes.data, len(v), t.ctypes.data, len(t), C.byref(params)))

    def add_surface(self, label, vertices, triangles, params: SurfaceParams) -> int:
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        t = np.ascontiguousarray(triangles, dtype=np.int32)
        return self._ck(self.L.mistark_sim_add_surface(self.h, label.encode(), v.ctypes.data, len(v), t.ctypes.data, len(t), C.byref(params)))

    def add_line(self, label, vertices, segments, params: LineParams) -> int:
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        t = np.ascontiguousarray(segments, dtype=np.int32)
        return self._ck(self.L.mistark_sim_add_line(self.h, label.encode(), v.ctypes.data, len(v), t.ctypes.data, len(t), C.byref(params)))

    def add_line_as_segments(self, label, begin, end, n_segments, params: LineParams) -> int:
        return self._ck(self.L.mistark_sim_add_line_as_segments(self.h, label.encode(), _d3(begin), _d3(end), int(n_segments), C.byref(params)))

    def prescribe_points(self, point_set, points, stiffness, tolerance=0.0) -> int:
        pts = np.ascontiguousarray(points, dtype=np.int32)
        return self._ck(self.L.mistark_sim_prescribe_points(self.h, point_set, pts.ctypes.data, len(pts), stiffness, tolerance))

    # EnergyAttachments::add overloads; indices are local to their point set, tolerance <= 0 = none; return the handler index
    def attach_point_point(self, set_0, set_1, points_0, points_1, stiffness, tolerance=0.0) -> int:
        a, b = np.ascontiguousarray(points_0, dtype=np.int32), np.ascontiguousarray(points_1, dtype=np.int32)
        return self._ck(self.L.mistark_sim_attach_point_point(self.h, set_0, set_1, a.ctypes.data, b.ctypes.data, len(a), stiffness, tolerance))

    def attach_point_edge(self, set_0, set_1, points, edges, bary, stiffness, tolerance=0.0) -> int:
        a, e = np.ascontiguousarray(points, dtype=np.int32), np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        w = np.ascontiguousarray(bary, dtype=np.float64).reshape(-1, 2)
        return self._ck(self.L.mistark_sim_attach_point_edge(self.h, set_0, set_1, a.ctypes.data, e.ctypes.data, w.ctypes.data, len(a), stiffness, tolerance))

    def attach_point_triangle(self, set_0, set_1, points, triangles, bary, stiffness, tolerance=0.0) -> int:
        a, t = np.ascontiguousarray(points, dtype=np.int32), np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        w = np.ascontiguousarray(bary, dtype=np.float64).reshape(-1, 3)
        return self._ck(self.L.mistark_sim_attach_point_triangle(self.h, set_0, set_1, a.ctypes.data, t.ctypes.data, w.ctypes.data, len(a), stiffness, tolerance))

    def attach_edge_edge(self, set_0, set_1, edges_0, edges_1, bary_0, bary_1, stiffness, tolerance=0.0) -> int:
        e0, e1 = np.ascontiguousarray(edges_0, dtype=np.int32).reshape(-1, 2), np.ascontiguousarray(edges_1, dtype=np.int32).reshape(-1, 2)
        w0, w1 = np.ascontiguousarray(bary_0, dtype=np.float64).reshape(-1, 2), np.ascontiguousarray(bary_1, dtype=np.float64).reshape(-1, 2)
        return self._ck(self.L.mistark_sim_attach_edge_edge(self.h, set_0, set_1, e0.ctypes.data, e1.ctypes.data, w0.ctypes.data, w1.ctypes.data, len(e0), stiffness, tolerance))

    def attach_rigid_body(self, rb, point_set, points, stiffness, tolerance=0.0, rb_points_loc=None) -> int:
        a = np.ascontiguousarray(points, dtype=np.int32)
        loc = None if rb_points_loc is None else np.ascontiguousarray(rb_points_loc, dtype=np.float64).reshape(-1, 3)
        return self._ck(self.L.mistark_sim_attach_rigid_body(self.h, rb, point_set, None if loc is None else loc.ctypes.data, a.ctypes.data, len(a), stiffness, tolerance))

    def attach_by_distance(self, set_0, set_1, points, triangles, distance, stiffness, tolerance=0.0):
        """EnergyAttachments::add_by_distance: returns the (point-point, point-edge, point-triangle) handlers."""
        a = np.ascontiguousarray(points, dtype=np.int32)
        t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        out = (C.c_int32 * 3)()
        self._ck(self.L.mistark_sim_attach_by_distance(self.h, set_0, set_1, a.ctypes.data, len(a), t.ctypes.data, len(t), distance, stiffness, tolerance, out))
        return list(out)

    def attach_rigid_body_by_distance(self, rb, point_set, loc_vertices, triangles, points, distance, stiffness, tolerance=0.0) -> int:
        v = np.ascontiguousarray(loc_vertices, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        a = np.ascontiguousarray(points, dtype=np.int32)
        return self._ck(self.L.mistark_sim_attach_rigid_body_by_distance(self.h, rb, point_set, v.ctypes.data, len(v), t.ctypes.data, len(t), a.ctypes.data, len(a), distance, stiffness,
                                                                         tolerance))

    def attachment_stiffness(self, handler) -> float:
        k = C.c_double()
        self._ck(self.L.mistark_sim_attachment_stiffness(self.h, handler, C.byref(k)))
        return k.value

    def point_set_add_displacement(self, ps, d):
        self._ck(self.L.mistark_sim_point_set_add_displacement(self.h, ps, _d3(d)))

    def point_set_add_rotation(self, ps, angle_deg, axis, pivot=(0.0, 0.0, 0.0)):
        self._ck(self.L.mistark_sim_point_set_add_rotation(self.h, ps, angle_deg, _d3(axis), _d3(pivot)))

    # ---- rigid bodies ---------------------------------------------------------------------------------------------------
    def add_rigid_box(self, label, mass, size) -> int:
        size = (size, size, size) if np.isscalar(size) else size
        return self._count_rb(self._ck(self.L.mistark_sim_add_rigid_box(self.h, label.encode(), mass, _d3(size))))

    def _count_rb(self, idx):
        self._n_rb = max(getattr(self, "_n_rb", 0), idx + 1)  # (forces() sizes its rigid-body output by it)
        return idx

    def rb_add(self, mass, inertia_local) -> int:
        """RigidBodies::add(mass, inertia) without a collision mesh."""
        return self._count_rb(self._ck(self.L.mistark_sim_rb_add(self.h, float(mass), _d3(np.asarray(inertia_local, dtype=float).reshape(9)))))

    def rb_add_force_at_centroid(self, rb, f):
        self._ck(self.L.mistark_sim_rb_add_force_at_centroid(self.h, rb, _d3(f)))

    def rb_add_torque(self, rb, t):
        self._ck(self.L.mistark_sim_rb_add_torque(self.h, rb, _d3(t)))

    def rb_add_fix(self, rb):
        """RigidBodies::add_constraint_fix; returns the handler (anchor point, z lock, x lock) for rb_fix_set_transformation."""
        g, d = self.rb_constraint_count("global_point"), self.rb_constraint_count("global_direction")
        self.rb_add_constraint("fix", rb)
        return (g, d, d + 1)

    def rb_fix_set_transformation(self, fix, translation, angle_deg=0.0, axis=(0.0, 0.0, 1.0)):
        """RBCFixHandler::set_transformation(translation, angle_deg, axis) (rigidbody_constraints_ui.h:376-379)."""
        a = np.asarray(axis, dtype=np.float64)
        a = a / np.linalg.norm(a)
        th = np.deg2rad(angle_deg)
        K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        R = np.ascontiguousarray(np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K))
        t = np.ascontiguousarray(translation, dtype=np.float64)
        self._ck(self.L.mistark_sim_rb_fix_set_transformation(self.h, int(fix[0]), int(fix[1]), int(fix[2]), t.ctypes.data_as(C.POINTER(C.c_double)),
                                                              R.ctypes.data_as(C.POINTER(C.c_double))))

    def rb_constraint_count(self, base_type) -> int:
        return self._ck(self.L.mistark_sim_rb_constraint_count(self.h, base_type.encode()))

    def rb_constraint_measure(self, base_type, idx, which=0):
        """(violation, force or torque, tolerance) of a base constraint, as the reference's constraint handlers report them."""
        out = (C.c_double * 2)()
        tol = C.c_double()
        self._ck(self.L.mistark_sim_rb_constraint_measure(self.h, base_type.encode(), idx, which, out, C.byref(tol)))
        return out[0], out[1], tol.value

    def run(self, duration) -> bool:
        return self._ck(self.L.mistark_sim_run(self.h, float(duration))) == 1

    def rb_set_translation(self, rb, t):
        self._ck(self.L.mistark_sim_rb_set_translation(self.h, rb, _d3(t)))

    def rb_add_translation(self, rb, t):
        self._ck(self.L.mistark_sim_rb_add_translation(self.h, rb, _d3(t)))

    def rb_add_rotation(self, rb, angle_deg, axis, pivot=(0.0, 0.0, 0.0)):
        self._ck(self.L.mistark_sim_rb_add_rotation(self.h, rb, angle_deg, _d3(axis), _d3(pivot)))

    def rb_set_default_constraint_params(self, stiffness=0.0, tolerance_in_m=0.0, tolerance_in_deg=0.0):
        self._ck(self.L.mistark_sim_rb_set_default_constraint_params(self.h, stiffness, tolerance_in_m, tolerance_in_deg))

    def rb_add_constraint(self, kind, a, b=-1, *params):
        flat = []
        for x in params:
            flat.extend([float(x)] if np.isscalar(x) else [float(v) for v in x])
        return self._ck(self.L.mistark_sim_rb_add_constraint(self.h, kind.encode(), a, b, _d3(flat) if flat else None, len(flat)))

    def rb_state(self, rb):
        t, q, v, w = np.zeros(3), np.zeros(4), np.zeros(3), np.zeros(3)
        self._ck(self.L.mistark_sim_rb_get_state(self.h, rb, t.ctypes.data, q.ctypes.data, v.ctypes.data, w.ctypes.data))
        return t, q, v, w

    # ---- multi-GPU sharding ------------------------------------------------------------------------------------------------
    def set_dist_rccl(self, rank, world, unique_id: bytes):
        buf = C.create_string_buffer(unique_id, 128)
        self._ck(self.L.mistark_sim_set_dist_rccl(self.h, rank, world, buf))

    def set_dist_local(self, group, rank, world):
        self._ck(self.L.mistark_sim_set_dist_local(self.h, group, rank, world))

    def set_dist_ipc(self, comm, rank, world):
        """comm: a connected capi.IpcComm (IPC windows, one process per rank; include/mistark.h)."""
        self._comm = comm  # (must outlive the engine)
        self._ck(self.L.mistark_sim_set_dist_ipc(self.h, comm.h, rank, world))

    # ---- frictional contact ----------------------------------------------------------------------------------------------
    def set_contact_global_params(self, p: ContactGlobalParams):
        self._ck(self.L.mistark_sim_set_contact_global_params(self.h, C.byref(p)))

    def contact_group(self, kind, idx) -> int:
        return self._ck(self.L.mistark_sim_contact_group(self.h, 0 if kind == "d" else 1, idx))

    def set_friction(self, group_a, group_b, mu):
        self._ck(self.L.mistark_sim_set_friction(self.h, group_a, group_b, mu))

    def disable_collision(self, group_a, group_b):
        self._ck(self.L.mistark_sim_disable_collision(self.h, group_a, group_b))

    def contact_info(self):
        k, n, nf, nd = C.c_double(), C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(self.L.mistark_sim_get_contact_info(self.h, C.byref(k), C.byref(n), C.byref(nf), C.byref(nd)))
        return dict(contact_stiffness=k.value, n_contacts=n.value, n_friction_contacts=nf.value, n_detections=nd.value)

    def set_contact_ccd(self, enabled=True, conservative_rescaling=0.9):
        """Continuous collision detection: every line search is bounded so that no collision pair's distance falls below
        (1 - conservative_rescaling) of its start value along the step. Off (the default) registers nothing."""
        self._ck(self.L.mistark_sim_set_contact_ccd(self.h, 1 if enabled else 0, float(conservative_rescaling)))

    def ccd_info(self):
        q, lim, cand, sk, cap = (C.c_int64() for _ in range(5))
        t = C.c_double()
        self._ck(self.L.mistark_sim_get_ccd_info(self.h, C.byref(q), C.byref(lim), C.byref(cand), C.byref(sk), C.byref(cap), C.byref(t)))
        return dict(queries=q.value, limited=lim.value, last_candidates=cand.value, skipped_pairs=sk.value, capped_pairs=cap.value, seconds=t.value)

    CCD_RIGID_MODES = ("linear", "curved")

    def set_contact_ccd_rigid(self, mode="curved", max_rounds=4):
        """How rigid bodies move in the CCD query: "linear" (the default) on the chord between their end positions, "curved" on their true rotating
        paths (the chord padded by a proved deviation bound, halved up to max_rounds times while the pad limits the step). Kept across set_contact_ccd;
        no effect while CCD is off."""
        if mode not in self.CCD_RIGID_MODES:
            raise ValueError("set_contact_ccd_rigid: mode must be one of %s, not %r" % (self.CCD_RIGID_MODES, mode))
        self._ck(self.L.mistark_sim_set_contact_ccd_rigid(self.h, self.CCD_RIGID_MODES.index(mode), int(max_rounds)))

    def ccd_rigid_info(self):
        mode, r, pb, mp = C.c_int(), C.c_int64(), C.c_int64(), C.c_double()
        self._ck(self.L.mistark_sim_get_ccd_rigid_info(self.h, C.byref(mode), C.byref(r), C.byref(pb), C.byref(mp)))
        return dict(mode=self.CCD_RIGID_MODES[mode.value], rounds=r.value, pad_bound_pairs=pb.value, max_pad=mp.value)

    def prescribe_inside_aabb(self, point_set, center, dim, stiffness, tolerance=0.0) -> int:
        return self._ck(self.L.mistark_sim_prescribe_inside_aabb(self.h, point_set, _d3(center), _d3(dim), stiffness, tolerance))

    def prescribe_outside_aabb(self, point_set, center, dim, stiffness, tolerance=0.0) -> int:
        return self._ck(self.L.mistark_sim_prescribe_outside_aabb(self.h, point_set, _d3(center), _d3(dim), stiffness, tolerance))

    def set_newton_settings(self, s: capi.NewtonSettings):
        self._ck(self.L.mistark_sim_set_newton_settings(self.h, C.byref(s)))

    def add_max_allowed_step(self, fn):
        """fn() -> fraction of the Newton step the line search may take (symx::SolverCallbacks::add_max_allowed_step)."""
        from . import capi

        cb = capi.DBLCB(lambda _u: float(fn()))
        self._keep_cb = getattr(self, "_keep_cb", []) + [cb]
        self._ck(self.L.mistark_sim_add_max_allowed_step(self.h, cb, None))

    def run_one_step(self) -> bool:
        return self._ck(self.L.mistark_sim_run_one_step(self.h)) == 1

    def begin_time_step(self):
        self._ck(self.L.mistark_sim_begin_time_step(self.h))

    def before_energy_evaluation(self):
        self._ck(self.L.mistark_sim_before_energy_evaluation(self.h))

    def prepare(self):
        self._ck(self.L.mistark_sim_prepare(self.h))

    def info(self) -> SimInfo:
        i = SimInfo()
        self._ck(self.L.mistark_sim_get_info(self.h, C.byref(i)))
        return i

    def points(self, which="x0") -> np.ndarray:
        sel = {"X": 0, "x0": 1, "v0": 2, "v1": 3}[which]
        n = self.info().n_points
        out = np.zeros((n, 3))
        self._ck(self.L.mistark_sim_get_points(self.h, sel, out.ctypes.data))
        return out

    def set_points(self, which, arr):
        sel = {"x0": 1, "v0": 2}[which]
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        self._ck(self.L.mistark_sim_set_points(self.h, sel, arr.ctypes.data))

    # ---- force recording ---------------------------------------------------------------------------------------------------
    def record_forces(self, groups):
        """groups: a list of potential-name prefixes, one group per entry ("" = all potentials), or a comma-separated string; None switches
        recording off. Every accepted step then keeps, per group, the nodal forces (Newtons) of the state it converged at."""
        if groups is None:
            self._ck(self.L.mistark_sim_record_forces(self.h, None))
            return
        text = groups if isinstance(groups, str) else ",".join(groups)
        self._ck(self.L.mistark_sim_record_forces(self.h, text.encode()))

    def forces(self, group=0):
        """(points [n_points, 3], rigid bodies [n_rigid_bodies, 6] = force and torque) of group `group` at the last accepted step. The torque is the
        generalised force conjugate to w1 * dt (the physical torque to first order in |w1| * dt)."""
        pts = np.zeros((self.info().n_points, 3))
        rb = np.zeros((getattr(self, "_n_rb", 0), 6))
        self._ck(self.L.mistark_sim_get_forces(self.h, int(group), pts.ctypes.data if pts.size else None, rb.ctypes.data if rb.size else None))
        return pts, rb

    # ---- stress recording --------------------------------------------------------------------------------------------------
    def record_stress(self, on=True):
        """Every accepted step then keeps, per element kind, the stress records and nodal averages of the state it converged at (on the device)."""
        self._ck(self.L.mistark_sim_record_stress(self.h, int(bool(on))))

    def stress(self, kind=0):
        """(records [n_elem, 16], nodal [n_points, 10]) of kind 0 tet / 1 triangle / 2 segment at the last accepted step: the elements of that kind's
        potentials in potential order, then element order; layout in include/mistark.h "stress readout"."""
        n = C.c_int64()
        self._ck(self.L.mistark_sim_get_stress(self.h, int(kind), None, C.byref(n)))
        rec = np.zeros((n.value, 16))
        if n.value:
            self._ck(self.L.mistark_sim_get_stress(self.h, int(kind), rec.ctypes.data, C.byref(n)))
        nodal = np.zeros((self.info().n_points, 10))
        if nodal.size:
            self._ck(self.L.mistark_sim_get_nodal_stress(self.h, int(kind), nodal.ctypes.data))
        return rec, nodal

    # ---- budget recording --------------------------------------------------------------------------------------------------
    def record_budget(self, on=True, about=(0.0, 0.0, 0.0)):
        """Every accepted step then keeps the energy of every potential and the mass, momentum and energy record of every object (inertia group,
        rigid body) of the state it converged at, on the device; angular momentum about `about`."""
        ab = (C.c_double * 3)(*[float(v) for v in about])
        self._ck(self.L.mistark_sim_record_budget(self.h, int(bool(on)), ab))

    def budget(self):
        """The budget of the last accepted step: dict(potentials={registry name: energy}, objects=[dict(label, kind, mass, com, momentum,
        angular_momentum, kinetic, gravitational, count)], total=dict(the sums over the objects), time). kinetic + gravitational + the strain potentials'
        entries is a mechanical energy; EnergyLumpedInertia's own entry is the incremental potential."""
        npot, nobj, nb, lb, t = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_double()
        self._ck(self.L.mistark_sim_get_budget(self.h, C.byref(npot), C.byref(nobj), C.byref(nb), C.byref(lb), C.byref(t), None, None, None, None, None))
        names, labels = C.create_string_buffer(nb.value), C.create_string_buffer(lb.value)
        E = np.zeros(npot.value)
        kinds = np.zeros(nobj.value, dtype=np.int32)
        rec = np.zeros((nobj.value, 13))
        self._ck(self.L.mistark_sim_get_budget(self.h, C.byref(npot), C.byref(nobj), C.byref(nb), C.byref(lb), C.byref(t), names, E.ctypes.data if E.size else None, labels,
                                               kinds.ctypes.data if kinds.size else None, rec.ctypes.data if rec.size else None))
        potentials = {}
        for name, e in zip(names.value.decode().split("\n")[:-1], E):
            potentials[name] = potentials.get(name, 0.0) + float(e)
        objects = []
        for label, kind, r in zip(labels.value.decode().split("\n")[:-1], kinds, rec):
            with np.errstate(divide="ignore", invalid="ignore"):
                com = r[1:4] / r[0] if r[0] != 0.0 else np.full(3, np.nan)
            objects.append(dict(label=label, kind="rigid" if kind == 1 else "deformable", mass=float(r[0]), com=com, momentum=r[4:7].copy(),
                                angular_momentum=r[7:10].copy(), kinetic=float(r[10]), gravitational=float(r[11]), count=int(r[12])))
        total = dict(mass=sum(o["mass"] for o in objects), momentum=sum((o["momentum"] for o in objects), np.zeros(3)),
                     angular_momentum=sum((o["angular_momentum"] for o in objects), np.zeros(3)), kinetic=sum(o["kinetic"] for o in objects),
                     gravitational=sum(o["gravitational"] for o in objects))
        return dict(potentials=potentials, objects=objects, total=total, time=t.value)

    # ---- constraint recording ----------------------------------------------------------------------------------------------
    def record_constraints(self, on=True, about=(0.0, 0.0, 0.0)):
        """Every accepted step then keeps the constraint report of the state it converged at (row and group records of every registered prescribed-position,
        attachment and rigid-body constraint potential, with the tolerances the scene holds) on the device; group moments about `about`."""
        ab = (C.c_double * 3)(*[float(v) for v in about])
        self._ck(self.L.mistark_sim_record_constraints(self.h, int(bool(on)), ab))

    def constraints(self):
        """The constraint report of the last accepted step: dict(kinds={registry name: dict(rows=Engine.constraint_report()'s dict, groups [n_groups, 12],
        tolerance [n_groups] (inf where the scene holds none), unit)}, time); kinds without rows are left out. Raises while recording is off."""
        from .engine import CONSTRAINT_KINDS, CONSTRAINT_UNITS, constraint_rows_dict
        kinds, time = {}, 0.0
        ptr = lambda a: a.ctypes.data if a.size else None
        for kind, name in enumerate(CONSTRAINT_KINDS):
            pres, n, g, ht, t = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32(), C.c_double()
            self._ck(self.L.mistark_sim_get_constraints(self.h, kind, C.byref(pres), C.byref(n), C.byref(g), C.byref(ht), C.byref(t), None, None, None, None, None))
            time = t.value
            if not pres.value or n.value == 0:
                continue
            rec, aux, ids = np.zeros((n.value, 16)), np.zeros((n.value, 2)), np.zeros((n.value, 4), dtype=np.int32)
            groups, tol = np.zeros((g.value, 12)), np.zeros(g.value)
            self._ck(self.L.mistark_sim_get_constraints(self.h, kind, C.byref(pres), C.byref(n), C.byref(g), C.byref(ht), C.byref(t), ptr(rec), ptr(aux), ptr(ids), ptr(groups),
                                                        ptr(tol) if ht.value else None))
            kinds[name] = dict(rows=constraint_rows_dict(rec, aux, ids, kind), groups=groups, tolerance=tol if ht.value else np.full(g.value, np.inf), unit=CONSTRAINT_UNITS[kind])
        return dict(kinds=kinds, time=time)

    # ---- bending recording ---------------------------------------------------------------------------------------------------
    def record_bending(self, on=True, threshold_rad=0.0):
        """Every accepted step then keeps the bending report of the state it converged at (row, nodal and group records of the cloth bending potentials
        the scene registers) on the device; threshold_rad flags hinges whose |theta1 - rest| exceeds it (0: none)."""
        self._ck(self.L.mistark_sim_record_bending(self.h, int(bool(on)), float(threshold_rad)))

    def bending(self):
        """The bending report of the last accepted step: dict(kinds={registry name: dict(rows=Engine.bending_report()'s dict, groups [n_groups, 10])},
        nodal [n_points, 6] over both kinds, time); kinds the scene does not register are left out. Raises while recording is off."""
        from .engine import BENDING_KINDS, bending_rows_dict
        kinds, time = {}, 0.0
        ptr = lambda a: a.ctypes.data if a.size else None
        for kind, name in enumerate(BENDING_KINDS):
            pres, n, g, t = C.c_int32(), C.c_int64(), C.c_int32(), C.c_double()
            self._ck(self.L.mistark_sim_get_bending(self.h, kind, C.byref(pres), C.byref(n), C.byref(g), C.byref(t), None, None))
            time = t.value
            if not pres.value:
                continue
            rec, groups = np.zeros((n.value, 16)), np.zeros((g.value, 10))
            if rec.size or groups.size:
                self._ck(self.L.mistark_sim_get_bending(self.h, kind, C.byref(pres), C.byref(n), C.byref(g), C.byref(t), ptr(rec), ptr(groups)))
            kinds[name] = dict(rows=bending_rows_dict(rec, kind), groups=groups)
        nodal = np.zeros((self.info().n_points, 6))
        if nodal.size:
            self._ck(self.L.mistark_sim_get_nodal_bending(self.h, nodal.ctypes.data))
        return dict(kinds=kinds, nodal=nodal, time=time)

    # ---- spectrum recording ----------------------------------------------------------------------------------------------------
    def record_spectrum(self, enabled=True, eps=None):
        """Every accepted step then keeps the Hessian spectrum report of the state it converged at on the device: a fresh evaluation (source 1) over every
        built-in potential, with potential, nodal and element records. eps: the threshold of `l < eps`; None: the Newton settings' projection eps."""
        self._ck(self.L.mistark_sim_record_spectrum(self.h, int(bool(enabled)), -1.0 if eps is None else float(eps)))

    def spectrum(self):
        """The spectrum report of the last accepted step: dict(time, eps, names (registry names of the potentials, id order), potentials [n, 10] as
        Engine.spectrum_potential_report() gives them, nodal [n_points, 5] for the point set). Raises while recording is off."""
        n, nb, eps, t = C.c_int32(), C.c_int64(), C.c_double(), C.c_double()
        self._ck(self.L.mistark_sim_get_spectrum(self.h, C.byref(n), C.byref(nb), C.byref(eps), C.byref(t), None, None))
        pots = np.zeros((n.value, 10))
        buf = C.create_string_buffer(max(int(nb.value), 1))
        self._ck(self.L.mistark_sim_get_spectrum(self.h, C.byref(n), C.byref(nb), C.byref(eps), C.byref(t), pots.ctypes.data if pots.size else None, buf))
        nodal = np.zeros((self.info().n_points, 5))
        if nodal.size:
            self._ck(self.L.mistark_sim_get_nodal_spectrum(self.h, nodal.ctypes.data))
        return dict(time=t.value, eps=eps.value, names=buf.value.decode().split("\n")[:n.value], potentials=pots, nodal=nodal)

    def spectrum_rows(self, name):
        """The element records of one recorded potential (by registry name), fetched on demand: Engine.spectrum_report()'s dict without the spectrum."""
        from .engine import spectrum_rows_dict
        n = C.c_int64()
        self._ck(self.L.mistark_sim_get_spectrum_rows(self.h, name.encode(), C.byref(n), None, 0))
        rec = np.zeros((n.value, 10))
        if n.value:
            self._ck(self.L.mistark_sim_get_spectrum_rows(self.h, name.encode(), C.byref(n), rec.ctypes.data, n.value))
        return spectrum_rows_dict(rec, 0)

    # ---- linear-system recording ----------------------------------------------------------------------------------------------
    def record_linsys(self, enabled=True, op=1, m=64):
        """Every accepted step then keeps the linear-system report of the matrix as the step's last assembly left it (op 0: A; 1: the block-Jacobi
        preconditioned matrix; at most m Lanczos steps from the built-in start vector)."""
        self._ck(self.L.mistark_sim_record_linsys(self.h, int(bool(enabled)), int(op), int(m)))

    def linsys(self):
        """The linear-system report of the last accepted step: dict(time, op, m, report (engine.LinsysReport of the summary record), low_row / low_share and
        high_row / high_share: the block row with the largest share of the lowest and of the highest mode). Raises while recording is off."""
        from .engine import LinsysReport
        op, m, t = C.c_int32(), C.c_int32(), C.c_double()
        rec, rows = np.zeros(16), np.zeros(4)
        self._ck(self.L.mistark_sim_get_linsys(self.h, C.byref(op), C.byref(m), C.byref(t), rec.ctypes.data, rows.ctypes.data))
        return dict(time=t.value, op=op.value, m=m.value, report=LinsysReport(rec), record=rec, low_row=int(rows[0]), low_share=float(rows[1]), high_row=int(rows[2]),
                    high_share=float(rows[3]))

    # ---- wrench recording ------------------------------------------------------------------------------------------------------
    WRENCH_FAMILIES = ("inertia_linear", "inertia_angular", "constraints", "attachments", "contact", "friction", "all")

    def record_wrench(self, on=True, about=(0.0, 0.0, 0.0)):
        """Every accepted step then keeps the rigid-body wrench report of the state it converged at on the device: per body the force and torque of
        seven families of potentials (WRENCH_FAMILIES; "inertia_linear" holds gravity and applied forces, "all" is the unbalanced wrench)."""
        ab = np.ascontiguousarray(about, dtype=np.float64).reshape(3)
        self._ck(self.L.mistark_sim_record_wrench(self.h, int(bool(on)), ab.ctypes.data))

    def wrench_sources(self):
        """What a step records with, for direct calls of Engine.rigid_wrench on the simulation's engine: dict(v1, w1, t0, q0 (array ids), n_bodies,
        families={name: potential ids}); "all" is the empty list, and so is every family the scene has no potential of (a step records zeros for those,
        Engine.rigid_wrench reads an empty list as every potential)."""
        state, start = np.zeros(5, dtype=np.int32), np.zeros(8, dtype=np.int32)
        self._ck(self.L.mistark_sim_wrench_sources(self.h, state.ctypes.data, start.ctypes.data, None))
        flat = np.zeros(max(int(start[7]), 1), dtype=np.int32)
        self._ck(self.L.mistark_sim_wrench_sources(self.h, state.ctypes.data, start.ctypes.data, flat.ctypes.data))
        fams = {name: [int(x) for x in flat[start[k]:start[k + 1]]] for k, name in enumerate(self.WRENCH_FAMILIES)}
        return dict(v1=int(state[0]), w1=int(state[1]), t0=int(state[2]), q0=int(state[3]), n_bodies=int(state[4]), families=fams)

    def wrench(self):
        """The wrench report of the last accepted step: dict(families=WRENCH_FAMILIES, records [7, n_bodies, 16] and counts [7, n_bodies] as
        Engine.rigid_wrench() gives them, labels (one per body), time). Raises while recording is off."""
        nf, nb, lb, t = C.c_int32(), C.c_int32(), C.c_int64(), C.c_double()
        self._ck(self.L.mistark_sim_get_wrench(self.h, C.byref(nf), C.byref(nb), C.byref(lb), C.byref(t), None, None, None))
        rec, cnt = np.zeros((nf.value, nb.value, 16)), np.zeros((nf.value, nb.value), dtype=np.int32)
        buf = C.create_string_buffer(max(int(lb.value), 1))
        if nb.value:
            self._ck(self.L.mistark_sim_get_wrench(self.h, C.byref(nf), C.byref(nb), C.byref(lb), C.byref(t), rec.ctypes.data, cnt.ctypes.data, buf))
        labels = buf.value.decode().split("\n")[:nb.value]
        return dict(families=self.WRENCH_FAMILIES, records=rec, counts=cnt, labels=labels, time=t.value)

    # ---- contact recording -------------------------------------------------------------------------------------------------
    def record_contacts(self, on=True):
        """Every accepted step then keeps the contact report of the state it converged at (rows of the installed barrier tables, vertex records,
        group-pair records) on the device."""
        self._ck(self.L.mistark_sim_record_contacts(self.h, int(bool(on))))

    def contacts(self):
        """The contact report of the last accepted step: dict(rows=Engine.contact_report()'s dict, vertices=Engine.contact_vertex_report()'s dict,
        pairs [n_groups, n_groups, 8], labels [n_groups], time). Raises while recording is off."""
        from .engine import contact_rows_dict, contact_vertices_dict
        n, nv, lb, t, g = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double(), C.c_int32()
        self._ck(self.L.mistark_sim_get_contacts(self.h, C.byref(n), C.byref(nv), C.byref(g), C.byref(lb), C.byref(t), None, None, None, None, None, None, None))
        ri, rd = np.zeros((n.value, 8), dtype=np.int32), np.zeros((n.value, 16))
        vert, vg, vs = np.zeros((nv.value, 5)), np.zeros(nv.value, dtype=np.int32), np.zeros(nv.value, dtype=np.int32)
        pairs = np.zeros((g.value, g.value, 8))
        labels = C.create_string_buffer(max(lb.value, 1))
        ptr = lambda a: a.ctypes.data if a.size else None
        self._ck(self.L.mistark_sim_get_contacts(self.h, C.byref(n), C.byref(nv), C.byref(g), C.byref(lb), C.byref(t), ptr(ri), ptr(rd), ptr(vert), ptr(vg), ptr(vs), ptr(pairs),
                                                 labels))
        return dict(rows=contact_rows_dict(ri, rd), vertices=contact_vertices_dict(vert, vg, vs), pairs=pairs, labels=labels.value.decode().split("\n")[:-1], time=t.value)

    # ---- friction recording ------------------------------------------------------------------------------------------------
    def record_friction(self, on=True):
        """Every accepted step then keeps the friction report of the state it converged at (rows of the friction tables installed at the start of the step,
        vertex records, group-pair records) on the device."""
        self._ck(self.L.mistark_sim_record_friction(self.h, int(bool(on))))

    def friction(self):
        """The friction report of the last accepted step: dict(rows=Engine.friction_report()'s dict, vertices=Engine.friction_vertex_report()'s dict,
        pairs [n_groups, n_groups, 12], labels [n_groups], time). Raises while recording is off."""
        from .engine import friction_rows_dict, friction_vertices_dict
        n, nv, lb, t, g = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double(), C.c_int32()
        self._ck(self.L.mistark_sim_get_friction(self.h, C.byref(n), C.byref(nv), C.byref(g), C.byref(lb), C.byref(t), None, None, None, None, None, None, None))
        ri, rd = np.zeros((n.value, 8), dtype=np.int32), np.zeros((n.value, 24))
        vert, vg, vs = np.zeros((nv.value, 8)), np.zeros(nv.value, dtype=np.int32), np.zeros(nv.value, dtype=np.int32)
        pairs = np.zeros((g.value, g.value, 12))
        labels = C.create_string_buffer(max(lb.value, 1))
        ptr = lambda a: a.ctypes.data if a.size else None
        self._ck(self.L.mistark_sim_get_friction(self.h, C.byref(n), C.byref(nv), C.byref(g), C.byref(lb), C.byref(t), ptr(ri), ptr(rd), ptr(vert), ptr(vg), ptr(vs), ptr(pairs),
                                                 labels))
        return dict(rows=friction_rows_dict(ri, rd), vertices=friction_vertices_dict(vert, vg, vs), pairs=pairs, labels=labels.value.decode().split("\n")[:-1], time=t.value)

    def engine_handle(self):
        return C.c_void_p(self.L.mistark_sim_engine(self.h))

    def newton_iteration_log(self):
        """Per-iteration records (capi.NewtonIteration) of the last Newton solve of the last time step attempt."""
        from . import capi

        n = C.c_int32()
        if self.L.mistark_newton_iteration_log(self.engine_handle(), None, 0, C.byref(n)) < 0:
            raise SimError("newton_iteration_log failed")
        rec = (capi.NewtonIteration * max(n.value, 1))()
        if self.L.mistark_newton_iteration_log(self.engine_handle(), rec, n.value, C.byref(n)) < 0:
            raise SimError("newton_iteration_log failed")
        return list(rec)[:n.value]

    def spmv_timing(self, reset=0):
        ms, n, b = C.c_double(), C.c_int64(), C.c_double()
        rc = self.L.mistark_spmv_timing(self.engine_handle(), reset, C.byref(ms), C.byref(n), C.byref(b))
        if rc < 0:
            raise SimError("spmv_timing failed")
        return ms.value, n.value, b.value
