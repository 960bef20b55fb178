"""What may be called after what on a device solver (IpmHold, lpopc_amd/csrc/rpm_ipm_hold.hpp; the table in DESIGN.md f-2), on a live
solver: the transitions no other test reaches.  tests/native/ipm_hold_test.cpp walks the whole table on the CPU; that a warm solve
after rpm_ipm_sensitivities is the warm solve without it is test_ipm_sensitivities.py's."""
import numpy as np
import pytest

import test_ipm_sensitivities as ts
from lpopc_amd.engine import RpmError


@pytest.mark.gpu
def test_call_order_on_a_live_solver(built):
    eng, ipm, XL, XU, x0, params = ts._quadrotor_batch(2)
    nt = ipm.info()["kkt_order"]

    def refused(text, fn):
        with pytest.raises(RpmError) as ei:
            fn()
        assert ei.value.code == 1 and text in str(ei.value), (text, str(ei.value))

    PASS = "valid only directly after rpm_ipm_debug_start"
    SEARCH = "valid only directly after rpm_ipm_debug_pass(stage 3)"
    UPDATE = "valid only directly after rpm_ipm_debug_line_search"
    SENS = "valid after a finished solve"
    MULT = "no solve has finished"

    def direction():
        """debug_start, debug_pass(3): a direction stands"""
        ipm.debug_start(x0, warm=False)
        out = ipm.debug_pass(3)
        assert (out["inst"]["status"] == 0).all()

    # a fresh solver holds nothing
    refused(PASS, lambda: ipm.debug_pass(1))
    refused(SEARCH, ipm.debug_line_search)
    refused(UPDATE, ipm.debug_update)
    refused(SENS, lambda: ipm.sensitivities(params))
    refused(MULT, ipm.bound_multipliers)

    # the sensitivities rewrite the matrix and the right-hand side: the state stays held, the direction does not survive
    direction()
    assert (ipm.sensitivities(params)["info"] < 2).all()
    refused(SEARCH, ipm.debug_line_search)
    refused(PASS, lambda: ipm.debug_pass(1))
    assert (ipm.sensitivities(params)["info"] < 2).all()
    refused(MULT, ipm.bound_multipliers)

    # their right-hand sides alone leave the direction alone
    direction()
    assert ipm.debug_sensitivity_rhs(params).shape == (2, len(params), nt)
    assert ipm.debug_storage().shape == (2, ipm.info()["storage_doubles"])      # read-only, like rpm_ipm_debug_slot: no state changes
    ipm.debug_line_search()

    # trial points are no state to take sensitivities at; one update per line search
    refused(SENS, lambda: ipm.sensitivities(params))
    refused(SENS, lambda: ipm.debug_sensitivity_rhs(params))
    refused(PASS, lambda: ipm.debug_pass(1))
    ipm.debug_line_search()                                     # (after itself)
    ipm.debug_update()
    refused(UPDATE, ipm.debug_update)
    refused(SEARCH, ipm.debug_line_search)
    refused(SENS, lambda: ipm.sensitivities(params))

    # the factor hook overwrites the matrix of a finished solve, not its bound multipliers
    sol = ipm.solve(x0)
    assert (sol["status"] == 0).all()
    z = ipm.bound_multipliers()
    assert (ipm.sensitivities(params)["info"] == 0).all()
    ipm.debug_solve_dense(np.tile(np.eye(nt), (2, 1, 1)), np.ones((2, nt)))
    refused(SENS, lambda: ipm.sensitivities(params))
    refused(PASS, lambda: ipm.debug_pass(1))
    z2 = ipm.bound_multipliers()
    assert np.array_equal(z[0], z2[0]) and np.array_equal(z[1], z2[1])

    # a start state's z is not a solve's
    ipm.debug_start(sol["x"], sol["lambda"], z)
    refused(MULT, ipm.bound_multipliers)
    refused(SEARCH, ipm.debug_line_search)
    ipm.close()
    eng.close()
