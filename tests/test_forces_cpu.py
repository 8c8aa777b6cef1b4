"""Force readout, the part that needs no GPU: the numpy reference the GPU tests compare against (tests/forces_ref.py) is proven against the
reference's own gradient, and a registration-only context refuses the three entry points."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forces_ref as fr  # noqa: E402
from fixture_list import stage_dumps  # noqa: E402

DUMPS = stage_dumps()


@pytest.mark.parametrize("path", DUMPS, ids=[os.path.basename(p)[:-4] for p in DUMPS])
def test_reference_sums_to_reference_gradient(path):
    """Summed over all potentials the reference forces are -scale * (the gradient the unmodified reference dumped), at the tolerance
    tests/test_oracle_golden.py holds the oracle's gradient to; inactive elements contribute exact zeros."""
    prob, man, z, scale, per, total, _ = fr.reference(path)
    assert fr.rel(total, -scale * z["grad"]) < fr.gradient_tolerance(man)
    for pi, r in per.items():
        assert (r["f"][~r["active"]] == 0.0).all()
        assert (r["rows"][r["active"]] == r["rows_active"]).all()
        assert r["f"].shape == (prob.potentials[pi].conn.shape[0], r["rows"].shape[1], 3)


def test_dry_context_refuses_every_entry_point():
    from stark_amd import capi

    L = capi.lib()
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        u = np.zeros(6)
        assert L.mistark_add_dof_set(h, b"u", u.ctypes.data, u.size) >= 0
        ne, nb = C.c_int64(), C.c_int32()
        f, out = np.zeros(6), np.zeros(6)
        rows = np.zeros(2, dtype=np.int32)
        about = np.zeros(3)
        calls = [
            lambda: L.mistark_potential_element_forces(h, 0, 1.0, None, None, C.byref(ne), C.byref(nb)),
            lambda: L.mistark_forces(h, None, 0, 1.0, f.ctypes.data),
            lambda: L.mistark_forces_resultant(h, None, 0, 1.0, rows.ctypes.data, 2, None, about.ctypes.data, out.ctypes.data),
        ]
        for call in calls:
            assert call() < 0
            msg = L.mistark_last_error(h).decode()
            assert msg and "registration-only" in msg, msg
    finally:
        L.mistark_destroy(h)
