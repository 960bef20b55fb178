"""Python host side above the C ABI (include/rpm_hip.h): loads lpopc_amd/csrc/librpm_hip.so and
exposes the engine with the reference's TNLP method names (Core/LpopcIpopt.h:33-82).

There is no fallback of any kind: if the shared library is missing this module raises at
import of `lib()`, and every evaluation fails loudly when no HIP device is usable.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _abi
from .problem import LpopcException

_HERE = os.path.dirname(os.path.abspath(__file__))
# RPM_HIP_LIB lets profiling sessions load the -DRPM_DIAG timestamp-trace build; it is never a different backend
_SO = os.environ.get("RPM_HIP_LIB") or os.path.join(_HERE, "csrc", "librpm_hip.so")
_LIB = None

RPM_OK, RPM_E_INVALID, RPM_E_UNSUPPORTED, RPM_E_DEVICE, RPM_E_NONFINITE = 0, 1, 2, 3, 4

# every symbol include/rpm_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "rpm_create", "rpm_destroy", "rpm_last_error", "rpm_device_init", "rpm_get_nlp_info",
    "rpm_get_bounds_info", "rpm_get_starting_point", "rpm_eval_f", "rpm_eval_grad_f", "rpm_eval_g",
    "rpm_eval_jac_g", "rpm_eval_pair", "rpm_eval_h", "rpm_finalize_solution", "rpm_get_solution", "rpm_eval_g_dev",
    "rpm_eval_jac_g_dev", "rpm_eval_pair_dev", "rpm_eval_f_dev", "rpm_eval_grad_f_dev", "rpm_eval_h_dev", "rpm_debug_hess_tt", "rpm_debug_hess_structure", "rpm_debug_tile_slot",
    "rpm_synchronize", "rpm_set_option", "rpm_get_option", "rpm_set_instance_constants", "rpm_get_phase_sizes", "rpm_get_phase_tables",
    "rpm_shard_segments", "rpm_shard_pack_dev", "rpm_shard_unpack_dev", "rpm_shard_slot_len", "rpm_shard_pack_all_dev", "rpm_shard_unpack_all_dev", "rpm_nlp2op_control", "rpm_final_result_save",
    "rpm_solution_error", "rpm_ph_refine_mesh", "rpm_ph_refine_from_error",
    "rpm_solution_error_batch_sizes", "rpm_solution_error_batch_dev", "rpm_solution_error_batch", "rpm_sweep_solution_error",
    "rpm_carry_solution_batch_dev", "rpm_carry_solution_batch", "rpm_sweep_carry_solution",
    "rpm_carry_multipliers_batch_dev", "rpm_carry_multipliers_batch", "rpm_carry_multipliers_layout", "rpm_sweep_carry_multipliers",
    "rpm_ipm_solve_warm", "rpm_ipm_solve_warm_dev", "rpm_ipm_get_bound_multipliers", "rpm_ipm_get_bound_multipliers_dev",
    "rpm_ipm_debug_start", "rpm_sweep_solve_warm", "rpm_sweep_get_bound_multipliers",
    "rpm_shift_plan_batch_dev", "rpm_shift_plan_batch", "rpm_sweep_shift_plan",
    "rpm_sample_plan_batch_dev", "rpm_sample_plan_batch", "rpm_sweep_sample_plan",
    "rpm_rollout_batch_dev", "rpm_rollout_batch", "rpm_sweep_rollout",
    "rpm_ipm_set_initial_states_dev", "rpm_ipm_set_initial_states", "rpm_sweep_set_initial_states",
    "rpm_nlp2op_batch_layout", "rpm_nlp2op_batch_dev", "rpm_nlp2op_batch", "rpm_sweep_nlp2op",
    "rpm_hpliu_create", "rpm_hpliu_destroy", "rpm_hpliu_last_error", "rpm_hpliu_refine",
    "rpm_ipm_create", "rpm_ipm_destroy", "rpm_ipm_last_error", "rpm_ipm_set_option", "rpm_ipm_set_bounds", "rpm_ipm_set_all_bounds", "rpm_ipm_get_info",
    "rpm_group_create", "rpm_group_destroy", "rpm_group_last_error", "rpm_group_size", "rpm_group_engine", "rpm_group_device_init",
    "rpm_group_set_option", "rpm_group_eval_f", "rpm_group_eval_grad_f", "rpm_group_eval_g", "rpm_group_eval_jac_g", "rpm_group_eval_pair",
    "rpm_group_eval_h", "rpm_group_eval_pair_dev", "rpm_group_allgather_pair_dev",
    "rpm_sweep_create", "rpm_sweep_destroy", "rpm_sweep_last_error", "rpm_sweep_size", "rpm_sweep_engine", "rpm_sweep_solver", "rpm_sweep_share",
    "rpm_sweep_set_option", "rpm_sweep_set_bounds", "rpm_sweep_solve", "rpm_sweep_get_stats",
    "rpm_ipm_get_stats", "rpm_ipm_get_subproblems", "rpm_ipm_get_trace", "rpm_ipm_get_restorations", "rpm_ipm_get_kernel_times", "rpm_ipm_solve", "rpm_ipm_solve_dev", "rpm_ipm_get_permutation", "rpm_ipm_debug_solve", "rpm_ipm_debug_solve_dense", "rpm_ipm_debug_slot", "rpm_ipm_debug_storage",
    "rpm_ipm_debug_lbfgs_step", "rpm_ipm_debug_lbfgs_state", "rpm_ipm_debug_lbfgs_solve", "rpm_ipm_debug_pass",
    "rpm_ipm_debug_line_search", "rpm_ipm_debug_update",
    "rpm_ipm_initial_state_variables", "rpm_ipm_parameter_variables", "rpm_ipm_sensitivities_dev", "rpm_ipm_sensitivities", "rpm_ipm_apply_sensitivities_dev",
    "rpm_ipm_apply_sensitivities", "rpm_ipm_debug_sensitivity_rhs", "rpm_sweep_sensitivities",
    "rpm_ipm_constant_sensitivities_dev", "rpm_ipm_constant_sensitivities", "rpm_ipm_apply_constant_sensitivities_dev",
    "rpm_ipm_apply_constant_sensitivities", "rpm_ipm_debug_constant_sensitivity_rhs", "rpm_sweep_constant_sensitivities",
    "rpm_set_all_instance_constants",
]


def build(force=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", csrc] + (["-B"] if force else []) + ["librpm_hip.so"]
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return _SO


_LIBS = {}


def lib(path=None):
    """The native library (ctypes handle with its prototypes set): the package's librpm_hip.so, or — `path` — a library
    built from a user's functor header (lpopc_amd.userproblem).  One handle per path, loaded once."""
    global _LIB
    so = os.path.abspath(path) if path else _SO
    if so in _LIBS:
        return _LIBS[so]
    if not os.path.exists(so):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the engine has no CPU fallback)" % so)
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7.  Importing torch first makes the
    # loader resolve this library's libamdhip64.so.7 dependency to the copy torch already mapped; loading in
    # the other order leaves two runtimes in the process and torch then reports "No HIP GPUs are available".
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(so)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    L.rpm_create.argtypes = [C.POINTER(_abi.rpm_problem_desc), C.POINTER(vp)]
    L.rpm_destroy.argtypes = [vp]
    L.rpm_destroy.restype = None
    L.rpm_last_error.argtypes = [vp]
    L.rpm_last_error.restype = C.c_char_p
    L.rpm_device_init.argtypes = [vp, C.c_int]
    L.rpm_get_nlp_info.argtypes = [vp, ip, ip, ip, ip, ip]
    L.rpm_get_bounds_info.argtypes = [vp, C.c_int, dp, dp, C.c_int, dp, dp]
    L.rpm_get_starting_point.argtypes = [vp, C.c_int, C.c_int, dp, C.c_int, dp, dp, C.c_int, C.c_int, dp]
    L.rpm_eval_f.argtypes = [vp, C.c_int, dp, C.c_int, dp]
    L.rpm_eval_grad_f.argtypes = [vp, C.c_int, dp, C.c_int, dp]
    L.rpm_eval_g.argtypes = [vp, C.c_int, dp, C.c_int, C.c_int, dp]
    L.rpm_eval_jac_g.argtypes = [vp, C.c_int, dp, C.c_int, C.c_int, C.c_int, ip, ip, dp]
    L.rpm_eval_pair.argtypes = [vp, C.c_int, dp, C.c_int, dp, C.c_int, dp]
    L.rpm_eval_h.argtypes = [vp, C.c_int, dp, C.c_int, C.c_double, C.c_int, dp, C.c_int, C.c_int, ip, ip, dp]
    L.rpm_finalize_solution.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, C.c_int, dp, dp, C.c_double]
    L.rpm_get_solution.argtypes = [vp, C.c_int, dp, C.c_int, dp, dp]
    L.rpm_eval_g_dev.argtypes = [vp, vp, vp, vp]
    L.rpm_eval_jac_g_dev.argtypes = [vp, vp, vp, vp]
    L.rpm_eval_pair_dev.argtypes = [vp, vp, vp, vp, vp]
    L.rpm_eval_f_dev.argtypes = [vp, vp, vp, vp]
    L.rpm_eval_grad_f_dev.argtypes = [vp, vp, vp, vp]
    L.rpm_eval_h_dev.argtypes = [vp, vp, C.c_double, vp, vp, vp]
    L.rpm_debug_hess_tt.argtypes = [vp, dp, C.c_int, dp]
    L.rpm_debug_hess_structure.argtypes = [vp, ip, C.c_int, C.c_int, ip, ip, ip]
    L.rpm_debug_tile_slot.argtypes = [C.c_int] * 5
    L.rpm_synchronize.argtypes = [vp]
    L.rpm_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.rpm_set_instance_constants.argtypes = [vp, C.c_int, dp, C.c_int]
    L.rpm_set_all_instance_constants.argtypes = [vp, dp, C.c_int]
    L.rpm_get_option.argtypes = [vp, C.c_char_p, ip]
    L.rpm_get_phase_sizes.argtypes = [vp, C.c_int, ip, ip, ip]
    L.rpm_get_phase_tables.argtypes = [vp, C.c_int, dp, dp, ip, ip, dp, dp, ip, ip, dp]
    L.rpm_nlp2op_control.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp]
    L.rpm_final_result_save.argtypes = [vp, C.c_char_p]
    L.rpm_solution_error.argtypes = [vp, C.c_int, dp, dp, ip]
    L.rpm_ph_refine_mesh.argtypes = [vp, C.c_int, dp, C.c_double, C.c_int, C.c_int, C.c_int, dp, ip, ip, dp, ip]
    L.rpm_ph_refine_from_error.argtypes = [vp, C.c_int, dp, C.c_double, C.c_int, C.c_int, C.c_int, dp, ip, ip, dp, ip]
    L.rpm_solution_error_batch_sizes.argtypes = [vp, ip, C.POINTER(C.c_longlong)]
    L.rpm_solution_error_batch_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.rpm_solution_error_batch.argtypes = [vp, dp, ip, dp, dp, dp, ip]
    L.rpm_sweep_solution_error.argtypes = [vp, dp, ip, dp, dp, dp, ip]
    L.rpm_carry_solution_batch_dev.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rpm_carry_solution_batch.argtypes = [vp, vp, dp, dp, ip]
    L.rpm_sweep_carry_solution.argtypes = [vp, vp, dp, dp, ip]
    L.rpm_carry_multipliers_batch_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.rpm_carry_multipliers_batch.argtypes = [vp, vp, dp, dp, dp, ip]
    L.rpm_carry_multipliers_layout.argtypes = [vp, C.c_int, ip]
    L.rpm_sweep_carry_multipliers.argtypes = [vp, vp, dp, dp, dp, ip]
    L.rpm_shift_plan_batch_dev.argtypes = [vp] * 12
    L.rpm_shift_plan_batch.argtypes = [vp] + [dp] * 9 + [ip]
    L.rpm_sweep_shift_plan.argtypes = [vp] + [dp] * 9 + [ip]
    _abi.bind_rollout(L)
    L.rpm_ipm_set_initial_states_dev.argtypes = [vp, C.c_int, vp, vp]
    L.rpm_ipm_set_initial_states.argtypes = [vp, C.c_int, dp]
    L.rpm_sweep_set_initial_states.argtypes = [vp, C.c_int, dp]
    L.rpm_nlp2op_batch_layout.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.rpm_nlp2op_batch_dev.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rpm_nlp2op_batch.argtypes = [vp, dp, dp, dp, ip]
    L.rpm_sweep_nlp2op.argtypes = [vp, dp, dp, dp, ip]
    L.rpm_hpliu_create.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.POINTER(vp)]
    L.rpm_hpliu_destroy.argtypes = [vp]
    L.rpm_hpliu_destroy.restype = None
    L.rpm_hpliu_last_error.argtypes = [vp]
    L.rpm_hpliu_last_error.restype = C.c_char_p
    L.rpm_hpliu_refine.argtypes = [vp, vp, dp, dp, C.c_int, dp, ip, ip, ip, ip, ip]
    L.rpm_ipm_create.argtypes = [vp, C.POINTER(vp)]
    L.rpm_ipm_destroy.argtypes = [vp]
    L.rpm_ipm_destroy.restype = None
    L.rpm_ipm_last_error.argtypes = [vp]
    L.rpm_ipm_last_error.restype = C.c_char_p
    L.rpm_ipm_set_option.argtypes = [vp, C.c_char_p, C.c_double]
    L.rpm_ipm_set_bounds.argtypes = [vp, C.c_int, dp, dp]
    L.rpm_ipm_set_all_bounds.argtypes = [vp, dp, dp]
    L.rpm_ipm_get_info.argtypes = [vp, ip, ip, ip, ip, C.POINTER(C.c_longlong), ip]
    L.rpm_ipm_get_stats.argtypes = [vp, ip, ip, ip]
    L.rpm_ipm_get_subproblems.argtypes = [vp, C.c_int, ip, ip]
    L.rpm_ipm_get_trace.argtypes = [vp, C.c_int, C.c_int, dp, ip]
    L.rpm_ipm_get_restorations.argtypes = [vp, ip]
    L.rpm_ipm_get_kernel_times.argtypes = [vp, dp, dp]
    L.rpm_ipm_solve.argtypes = [vp, dp, dp, dp, ip, ip, dp]
    L.rpm_ipm_solve_dev.argtypes = [vp, vp, vp, dp, ip, ip, dp, vp]
    L.rpm_ipm_solve_warm.argtypes = [vp, dp, dp, dp, dp, dp, ip, ip, dp]
    L.rpm_ipm_solve_warm_dev.argtypes = [vp, vp, vp, vp, vp, dp, ip, ip, dp, vp]
    L.rpm_ipm_get_bound_multipliers.argtypes = [vp, dp, dp]
    L.rpm_ipm_get_bound_multipliers_dev.argtypes = [vp, vp, vp, vp]
    L.rpm_ipm_debug_start.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, dp, ip]
    _abi.bind_ipm_debug_pass(L)
    L.rpm_ipm_get_permutation.argtypes = [vp, ip, C.c_int]
    L.rpm_ipm_debug_solve.argtypes = [vp, dp, dp, dp, ip, ip]
    L.rpm_ipm_debug_solve_dense.argtypes = [vp, dp, dp, dp, ip, ip]
    L.rpm_ipm_debug_slot.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    L.rpm_ipm_debug_lbfgs_step.argtypes = [vp, C.c_int, dp, dp, dp, ip, ip]
    L.rpm_ipm_debug_lbfgs_state.argtypes = [vp, dp, dp, dp, dp]
    L.rpm_ipm_debug_lbfgs_solve.argtypes = [vp, C.c_int, ip, ip, dp, dp, dp]
    L.rpm_shard_segments.argtypes = [vp, C.c_int, C.c_int, C.POINTER(_abi.rpm_segment), ip, ip]
    L.rpm_shard_pack_dev.argtypes = [vp, C.c_int, vp, vp, vp]
    L.rpm_shard_unpack_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    L.rpm_shard_slot_len.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.rpm_shard_pack_all_dev.argtypes = [vp, vp, vp, vp, vp]
    L.rpm_shard_unpack_all_dev.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    L.rpm_group_create.argtypes = [C.POINTER(_abi.rpm_problem_desc), C.c_int, ip, C.POINTER(vp)]
    L.rpm_group_destroy.argtypes = [vp]
    L.rpm_group_destroy.restype = None
    L.rpm_group_last_error.argtypes = [vp]
    L.rpm_group_last_error.restype = C.c_char_p
    L.rpm_group_size.argtypes = [vp]
    L.rpm_group_engine.argtypes = [vp, C.c_int]
    L.rpm_group_engine.restype = vp
    L.rpm_group_device_init.argtypes = [vp]
    L.rpm_group_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.rpm_group_eval_f.argtypes = [vp, C.c_int, dp, C.c_int, dp]
    L.rpm_group_eval_grad_f.argtypes = [vp, C.c_int, dp, C.c_int, dp]
    L.rpm_group_eval_g.argtypes = [vp, C.c_int, dp, C.c_int, C.c_int, dp]
    L.rpm_group_eval_jac_g.argtypes = [vp, C.c_int, dp, C.c_int, C.c_int, C.c_int, ip, ip, dp]
    L.rpm_group_eval_pair.argtypes = [vp, C.c_int, dp, C.c_int, dp, C.c_int, dp]
    L.rpm_group_eval_h.argtypes = [vp, C.c_int, dp, C.c_int, C.c_double, C.c_int, dp, C.c_int, C.c_int, ip, ip, dp]
    L.rpm_group_eval_pair_dev.argtypes = [vp, C.c_int, vp, vp, vp]
    L.rpm_group_allgather_pair_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.rpm_sweep_create.argtypes = [vp, C.c_int, ip, C.POINTER(vp)]
    L.rpm_sweep_destroy.argtypes = [vp]
    L.rpm_sweep_destroy.restype = None
    L.rpm_sweep_last_error.argtypes = [vp]
    L.rpm_sweep_last_error.restype = C.c_char_p
    L.rpm_sweep_size.argtypes = [vp]
    L.rpm_sweep_engine.argtypes = [vp, C.c_int]
    L.rpm_sweep_engine.restype = vp
    L.rpm_sweep_solver.argtypes = [vp, C.c_int]
    L.rpm_sweep_solver.restype = vp
    L.rpm_sweep_share.argtypes = [vp, C.c_int, ip, ip]
    L.rpm_sweep_set_option.argtypes = [vp, C.c_char_p, C.c_double]
    L.rpm_sweep_set_bounds.argtypes = [vp, C.c_int, dp, dp]
    L.rpm_sweep_solve.argtypes = [vp, dp, dp, dp, ip, ip, dp]
    L.rpm_sweep_get_stats.argtypes = [vp, ip, ip, ip]
    L.rpm_sweep_solve_warm.argtypes = [vp, dp, dp, dp, dp, dp, ip, ip, dp]
    L.rpm_sweep_get_bound_multipliers.argtypes = [vp, dp, dp]
    L.rpm_ipm_initial_state_variables.argtypes = [vp, C.c_int, ip]
    L.rpm_ipm_parameter_variables.argtypes = [vp, C.c_int, ip]
    L.rpm_ipm_sensitivities_dev.argtypes = [vp, C.c_int, ip, vp, vp, dp, ip, vp]
    L.rpm_ipm_sensitivities.argtypes = [vp, C.c_int, ip, dp, dp, dp, ip]
    L.rpm_ipm_apply_sensitivities_dev.argtypes = [vp, C.c_int, ip] + [vp] * 8
    L.rpm_ipm_apply_sensitivities.argtypes = [vp, C.c_int, ip] + [dp] * 7
    L.rpm_ipm_debug_sensitivity_rhs.argtypes = [vp, C.c_int, ip, dp]
    L.rpm_sweep_sensitivities.argtypes = [vp, C.c_int, ip, dp, dp, dp, ip]
    L.rpm_ipm_constant_sensitivities_dev.argtypes = [vp, C.c_int, ip, vp, vp, dp, ip, vp]
    L.rpm_ipm_constant_sensitivities.argtypes = [vp, C.c_int, ip, dp, dp, dp, ip]
    L.rpm_ipm_apply_constant_sensitivities_dev.argtypes = [vp, C.c_int, ip] + [vp] * 8
    L.rpm_ipm_apply_constant_sensitivities.argtypes = [vp, C.c_int, ip] + [dp] * 7
    L.rpm_ipm_debug_constant_sensitivity_rhs.argtypes = [vp, C.c_int, ip, dp]
    L.rpm_sweep_constant_sensitivities.argtypes = [vp, C.c_int, ip, dp, dp, dp, ip]
    _LIBS[so] = L
    if so == _SO:
        _LIB = L
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class RpmError(LpopcException):
    def __init__(self, code, msg):
        super().__init__("rpm error %d: %s" % (code, msg))
        self.code = code


def _phase_shapes(L, handle, desc, n_phases, check):
    out = []
    for p in range(n_phases):
        N = C.c_int()
        check(L.rpm_get_phase_sizes(handle, p, C.byref(N), None, None))
        K = desc.phases[p].n_intervals
        out.append((K, N.value + K + 1, desc.phases[p].nx))
    return out


def _split_rel(flat, shapes):
    out, off = [], 0
    for _, rows, nx in shapes:
        blk = flat[..., off:off + rows * nx]
        out.append(blk.reshape(flat.shape[:-1] + (nx, rows)).swapaxes(-1, -2).copy())
        off += rows * nx
    return out


def _batch_estimate(fn, check, handle, x, B, sizes, shapes, mask, full):
    """Shared by NLPEngine.solution_error_batch and SweepGroup.solution_error: call, then cut the flat results per phase."""
    KT, RT = sizes
    mp = None
    if mask is not None:
        mk = np.ascontiguousarray(mask, dtype=np.int32).ravel()
        if mk.size != B:
            raise RpmError(RPM_E_INVALID, "mask has %d entries, expected %d" % (mk.size, B))
        mp = _ip(mk)
    iv, mx, flags = np.zeros((B, KT)), np.zeros(RT), np.zeros(B, dtype=np.int32)
    rel = np.zeros((B, RT)) if full else None
    check(fn(handle, _dp(x), mp, _dp(iv), _dp(mx), _dp(rel) if full else None, _ip(flags)))
    out = {"interval_error": [], "rel_err_max": _split_rel(mx, shapes), "nonfinite": flags}
    off = 0
    for K, _, _ in shapes:
        out["interval_error"].append(iv[:, off:off + K].copy())
        off += K
    if full:
        out["rel_err"] = _split_rel(rel, shapes)
    return out


EXTRACT_FIELDS = ("time", "state", "control", "costate", "pathmult", "hamiltonian", "mayer_cost", "lagrange_cost")


def _extract_layout(L, handle, n_phases, check):
    """rpm_nlp2op_batch_layout for every phase -> (offsets: n_phases x 8 in the order of EXTRACT_FIELDS, EB)."""
    offs, eb = np.zeros((n_phases, 8), dtype=np.int64), C.c_longlong()
    for p in range(n_phases):
        o = (C.c_longlong * 8)()
        check(L.rpm_nlp2op_batch_layout(handle, p, o, C.byref(eb)))
        offs[p] = list(o)
    return offs, eb.value


def _batch_extract(fn, check, handle, x, lam, B, m, layout):
    """Shared by NLPEngine.nlp2op_batch and SweepGroup.nlp2op: call, then cut every instance's block per phase and field."""
    offs, EB = layout
    lam = np.ascontiguousarray(lam, dtype=np.float64).ravel()
    if lam.size != B * m:
        raise RpmError(RPM_E_INVALID, "lambda has %d entries, expected %d" % (lam.size, B * m))
    out, flags = np.zeros((B, EB)), np.zeros(B, dtype=np.int32)
    check(fn(handle, _dp(x), _dp(lam), _dp(out), _ip(flags)))
    ends = np.append(offs.ravel()[1:], EB)             # a field ends where the next one starts
    phases = []
    for p in range(offs.shape[0]):
        d = {}
        for f, name in enumerate(EXTRACT_FIELDS):
            a = out[:, offs[p, f]:ends[p * 8 + f]]
            d[name] = a[:, 0].copy() if f >= 6 else a.copy()
        phases.append(d)
    return phases, flags


class NLPEngine:
    """One NLP (one mesh) on one GPU.  Method names and argument order follow LpopcIpopt
    (Core/LpopcIpopt.h:33-82); host arrays are numpy float64, device arrays are torch CUDA
    tensors (used only as HBM handles)."""

    def __init__(self, problem, options=None, n_instances=1, shard_mode=0, shard_rank=0, shard_world=1,
                 tile_nodes=0, device=None, role_loop=None, probe_hessian=True):
        """probe_hessian=False: an exact-Hessian engine is set up on the host only — the dependency probe, which needs the
        device, is left to the first eval_h_structure / eval_h, and nnz_h is None until then."""
        self._L = lib(getattr(problem.GetOpimalProblemFuns(), "library", None))
        self._desc, self._keep = _abi.lower(problem, options, n_instances, shard_mode, shard_rank, shard_world)
        h = C.c_void_p()
        rc = self._L.rpm_create(C.byref(self._desc), C.byref(h))
        if rc != RPM_OK:
            raise RpmError(rc, self._L.rpm_last_error(None).decode())
        self._h = h
        if tile_nodes:
            self.set_option("tile_nodes", tile_nodes)
        if role_loop is not None:
            self.set_option("role_loop", role_loop)
        # "pin_host" stays at the C ABI's default 0: this wrapper hands numpy arrays of any lifetime to the library, which
        # copies them through its own page-locked staging buffers.  A caller that reuses long-lived `out=` arrays (as
        # Ipopt does) may set_option("pin_host", 1) — then rpm_hip.h's lifetime contract for those arrays applies.
        n, m, nj, nh, st = (C.c_int() for _ in range(5))
        self._check(self._L.rpm_get_nlp_info(h, C.byref(n), C.byref(m), C.byref(nj), C.byref(nh) if probe_hessian else None, C.byref(st)))
        self.n, self.m, self.nnz_jac, self.nnz_h, self.index_style = n.value, m.value, nj.value, nh.value if probe_hessian else None, st.value
        self.n_instances = n_instances
        self.n_phases = problem.GetPhaseNum()
        if device is not None:
            self.device_init(device)

    def close(self):
        if getattr(self, "_h", None):
            self._L.rpm_destroy(self._h)          # also releases every page-locked registration
            self._h = None
        self._bufs = {}                           # only now: see _own

    def __del__(self):
        self.close()

    def _own(self, name, size):
        """A result array owned by this object for calls without `out=`.  With pin_host = 1 the library page-locks the
        host arrays it is handed and holds the registration until eviction or close() (rpm_hip.h: such arrays must stay
        mapped that long); a temporary numpy array would be freed while still registered.  So temporaries never reach the
        library: results are written into these buffers, which live until close(), and handed out as copies."""
        bufs = self.__dict__.setdefault("_bufs", {})
        b = bufs.get(name)
        if b is None or b.size != size:
            if b is not None:
                bufs.setdefault("_retired", []).append(b)    # still registered: keep it alive
            b = bufs[name] = np.zeros(size)
        return b

    def _check(self, rc):
        if rc != RPM_OK:
            raise RpmError(rc, self._L.rpm_last_error(self._h).decode())

    def last_error(self):
        """rpm_last_error: the reason of the last failed call, plus what the page-lock registry last refused this engine."""
        return self._L.rpm_last_error(self._h).decode()

    def device_init(self, device_id=0):
        self._check(self._L.rpm_device_init(self._h, int(device_id)))

    def set_option(self, key, value):
        self._check(self._L.rpm_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int()
        self._check(self._L.rpm_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def set_instance_constants(self, instance, consts):
        """Give one instance of a batched engine its own problem constants (parameter sweeps)."""
        c = np.ascontiguousarray(consts, dtype=np.float64)
        self._check(self._L.rpm_set_instance_constants(self._h, int(instance), _dp(c), int(c.size)))

    def set_all_instance_constants(self, consts):
        """Every instance's constants, (n_instances, nconst), in one upload: what set_instance_constants leaves instance by instance."""
        c = np.ascontiguousarray(consts, dtype=np.float64)
        if c.ndim != 2 or c.shape[0] != self.n_instances:
            raise RpmError(RPM_E_INVALID, "consts must be (n_instances, nconst)")
        self._check(self._L.rpm_set_all_instance_constants(self._h, _dp(c), int(c.shape[1])))

    # ---- TNLP surface, host buffers --------------------------------------------------------
    def get_nlp_info(self):
        return self.n, self.m, self.nnz_jac, self.nnz_h, self.index_style

    def get_bounds_info(self):
        xl, xu, gl, gu = np.zeros(self.n), np.zeros(self.n), np.zeros(self.m), np.zeros(self.m)
        self._check(self._L.rpm_get_bounds_info(self._h, self.n, _dp(xl), _dp(xu), self.m, _dp(gl), _dp(gu)))
        return xl, xu, gl, gu

    def get_starting_point(self):
        x = np.zeros(self.n)
        self._check(self._L.rpm_get_starting_point(self._h, self.n, 1, _dp(x), 0, None, None, self.m, 0, None))
        return x

    def _x(self, x):
        x0 = x
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        if x.size != self.n * self.n_instances:
            raise RpmError(RPM_E_INVALID, "x has %d entries, expected %d" % (x.size, self.n * self.n_instances))
        if not (isinstance(x0, np.ndarray) and np.shares_memory(x, x0)):     # a converted copy: a temporary (see _own)
            b = self._own("x", x.size)
            b[:] = x
            return b
        return x

    def eval_f(self, x, new_x=True):
        x = self._x(x)
        out = self._own("f", self.n_instances)
        self._check(self._L.rpm_eval_f(self._h, self.n, _dp(x), int(new_x), _dp(out)))
        return float(out[0]) if self.n_instances == 1 else out.copy()

    def eval_grad_f(self, x, new_x=True, out=None):
        x = self._x(x)
        res = self._own("grad", self.n * self.n_instances) if out is None else out
        self._check(self._L.rpm_eval_grad_f(self._h, self.n, _dp(x), int(new_x), _dp(res)))
        return res.copy() if out is None else out

    def eval_g(self, x, new_x=True, out=None):
        x = self._x(x)
        res = self._own("g", self.m * self.n_instances) if out is None else out
        self._check(self._L.rpm_eval_g(self._h, self.n, _dp(x), int(new_x), self.m, _dp(res)))
        return res.copy() if out is None else out

    def eval_jac_g_structure(self):
        i, j = np.zeros(self.nnz_jac, dtype=np.int32), np.zeros(self.nnz_jac, dtype=np.int32)
        self._check(self._L.rpm_eval_jac_g(self._h, self.n, None, 0, self.m, self.nnz_jac, _ip(i), _ip(j), None))
        return i, j

    def eval_jac_g(self, x, new_x=True, out=None):
        x = self._x(x)
        res = self._own("values", self.nnz_jac * self.n_instances) if out is None else out
        self._check(self._L.rpm_eval_jac_g(self._h, self.n, _dp(x), int(new_x), self.m, self.nnz_jac, None, None, _dp(res)))
        return res.copy() if out is None else out

    def eval_pair(self, x, g_out=None, values_out=None):
        """rpm_eval_pair: eval_g + eval_jac_g of one x in one call (host arrays) -> (g, values)."""
        x = self._x(x)
        g = self._own("g", self.m * self.n_instances) if g_out is None else g_out
        v = self._own("values", self.nnz_jac * self.n_instances) if values_out is None else values_out
        self._check(self._L.rpm_eval_pair(self._h, self.n, _dp(x), self.m, _dp(g), self.nnz_jac, _dp(v)))
        return (g.copy() if g_out is None else g_out), (v.copy() if values_out is None else values_out)

    def _probed(self):
        """nnz_h of an engine created with probe_hessian=False: asked for (the device probe runs) on first need."""
        if self.nnz_h is None:
            nh = C.c_int()
            self._check(self._L.rpm_get_nlp_info(self._h, None, None, None, C.byref(nh), None))
            self.nnz_h = nh.value
        return self.nnz_h

    def eval_h_structure(self):
        self._probed()
        i, j = np.zeros(self.nnz_h, dtype=np.int32), np.zeros(self.nnz_h, dtype=np.int32)
        self._check(self._L.rpm_eval_h(self._h, self.n, None, 0, 1.0, self.m, None, 0, self.nnz_h, _ip(i), _ip(j), None))
        return i, j

    def eval_h(self, x, obj_factor, lam, new_x=True, new_lambda=True):
        x = self._x(x)
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        out = np.zeros(self._probed() * self.n_instances)
        self._check(self._L.rpm_eval_h(self._h, self.n, _dp(x), int(new_x), float(obj_factor), self.m, _dp(lam),
                                       int(new_lambda), self.nnz_h, None, None, _dp(out)))
        return out

    def finalize_solution(self, status, x, lam, obj_value):
        x = self._x(x)
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        self._check(self._L.rpm_finalize_solution(self._h, int(status), self.n, _dp(x), None, None, self.m, None,
                                                  _dp(lam), float(obj_value)))

    def get_solution(self):
        x, lam, obj = np.zeros(self.n), np.zeros(self.m), C.c_double()
        self._check(self._L.rpm_get_solution(self._h, self.n, _dp(x), self.m, _dp(lam), C.byref(obj)))
        return x, lam, obj.value

    # ---- device-resident variants (torch CUDA tensors as HBM handles) -------------------------
    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    @staticmethod
    def _stream(stream):
        if stream is None:
            import torch
            return C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return C.c_void_p(stream)

    def eval_g_dev(self, d_x, d_g, stream=None):
        self._check(self._L.rpm_eval_g_dev(self._h, self._ptr(d_x), self._ptr(d_g), self._stream(stream)))

    def eval_jac_g_dev(self, d_x, d_values, stream=None):
        self._check(self._L.rpm_eval_jac_g_dev(self._h, self._ptr(d_x), self._ptr(d_values), self._stream(stream)))

    def eval_pair_dev(self, d_x, d_g, d_values, stream=None):
        self._check(self._L.rpm_eval_pair_dev(self._h, self._ptr(d_x), self._ptr(d_g), self._ptr(d_values),
                                              self._stream(stream)))

    def eval_f_dev(self, d_x, d_obj, stream=None):
        self._check(self._L.rpm_eval_f_dev(self._h, self._ptr(d_x), self._ptr(d_obj), self._stream(stream)))

    def eval_grad_f_dev(self, d_x, d_grad, stream=None):
        self._check(self._L.rpm_eval_grad_f_dev(self._h, self._ptr(d_x), self._ptr(d_grad), self._stream(stream)))

    def eval_h_dev(self, d_x, obj_factor, d_lambda, d_values, stream=None):
        self._check(self._L.rpm_eval_h_dev(self._h, self._ptr(d_x), float(obj_factor), self._ptr(d_lambda),
                                           self._ptr(d_values), self._stream(stream)))

    def debug_hess_structure(self, dep):
        """rpm_debug_hess_structure: (iRow, jCol) of the exact Hessian for a given dependency pattern (per phase (nx + nc) x
        (nx + nu) flags, column-major, concatenated), host only — no device is touched."""
        dep = np.ascontiguousarray(dep, dtype=np.int32).ravel()
        nnz = np.zeros(1, dtype=np.int32)
        self._check(self._L.rpm_debug_hess_structure(self._h, _ip(dep), int(dep.size), 0, None, None, _ip(nnz)))
        hi, hj = np.zeros(int(nnz[0]), dtype=np.int32), np.zeros(int(nnz[0]), dtype=np.int32)
        self._check(self._L.rpm_debug_hess_structure(self._h, _ip(dep), int(dep.size), int(nnz[0]), _ip(hi), _ip(hj), _ip(nnz)))
        return hi, hj

    def debug_hess_tt(self, tmp):
        """rpm_debug_hess_tt: rpm_hess_tt_kernel alone on per-node terms (n_instances, 3 * sum N) -> (n_instances, n_phases, 3)
        = the t0t0, tft0, tftf entries.  Per phase the rows are the terms of t0t0, tftf, tft0."""
        tmp = np.ascontiguousarray(tmp, dtype=np.float64)
        out = np.zeros((self.n_instances, self.n_phases, 3))
        self._check(self._L.rpm_debug_hess_tt(self._h, _dp(tmp), int(tmp.size // self.n_instances), _dp(out)))
        return out

    def synchronize(self):
        self._check(self._L.rpm_synchronize(self._h))

    # ---- solution extraction (Nlp2OpConverter) ----------------------------------------
    def nlp2op_control(self, phase, x=None, lam=None):
        d = self._desc.phases[phase]
        M = self.phase_tables(phase)["points"].size + 1
        out = dict(time=np.zeros(M), state=np.zeros(M * d.nx), control=np.zeros(M * max(d.nu, 1)),
                   costate=np.zeros(M * d.nx), pathmult=np.zeros(M * max(d.nc, 1)), hamiltonian=np.zeros(M))
        mc, lc = C.c_double(), C.c_double()
        xp = _dp(self._x(x)) if x is not None else None
        lp = _dp(np.ascontiguousarray(lam, dtype=np.float64)) if lam is not None else None
        self._check(self._L.rpm_nlp2op_control(self._h, phase, xp, lp, _dp(out["time"]), _dp(out["state"]),
                                               _dp(out["control"]), _dp(out["costate"]), _dp(out["pathmult"]),
                                               _dp(out["hamiltonian"]), C.cast(C.byref(mc), C.POINTER(C.c_double)),
                                               C.cast(C.byref(lc), C.POINTER(C.c_double))))
        out["control"] = out["control"][:M * d.nu]
        out["pathmult"] = out["pathmult"][:M * d.nc]
        out["mayer_cost"], out["lagrange_cost"] = mc.value, lc.value
        return out

    def final_result_save(self, directory):
        self._check(self._L.rpm_final_result_save(self._h, str(directory).encode()))

    # ---- mesh-error estimate and ph refinement ---------------------------------------
    def solution_error(self, phase, x=None):
        """SolutionErrorChecker::CheckSolutionDiffError -> relative_error, (N + K + 1) x nx."""
        rows = C.c_int()
        self._check(self._L.rpm_solution_error(self._h, phase, None, None, C.byref(rows)))
        nx = self._desc.phases[phase].nx
        rel = np.zeros(rows.value * nx)
        xp = _dp(self._x(x)) if x is not None else None
        self._check(self._L.rpm_solution_error(self._h, phase, xp, _dp(rel), C.byref(rows)))
        return rel.reshape((rows.value, nx), order="F")

    def _refine(self, fn, phase, arg, tol, nmin, nmax):
        K = self._desc.phases[phase].n_intervals
        nk, done, emax = C.c_int(), C.c_int(), np.zeros(K)
        self._check(fn(self._h, phase, arg, float(tol), int(nmin), int(nmax), 0, None, None, C.byref(nk), _dp(emax),
                       C.byref(done)))
        mesh, nodes = np.zeros(nk.value + 1), np.zeros(nk.value, dtype=np.int32)
        self._check(fn(self._h, phase, arg, float(tol), int(nmin), int(nmax), nk.value, _dp(mesh), _ip(nodes),
                       C.byref(nk), None, None))
        return bool(done.value), mesh, nodes, emax

    def ph_refine_mesh(self, phase, tol, nmin, nmax, x=None):
        """PhMeshRefineAlg::RefineMesh for one phase -> (no_more_refine, mesh_points, nodes_per_interval, emax)."""
        xp = _dp(self._x(x)) if x is not None else None
        return self._refine(self._L.rpm_ph_refine_mesh, phase, xp, tol, nmin, nmax)

    def ph_refine_from_error(self, phase, rel_err, tol, nmin, nmax):
        rel = np.asfortranarray(rel_err, dtype=np.float64).ravel(order="F").copy()
        return self._refine(self._L.rpm_ph_refine_from_error, phase, _dp(rel), tol, nmin, nmax)

    # ---- the estimate of a whole sweep: all phases, all instances (rpm_solution_error_batch*) -------------------------
    def solution_error_batch_sizes(self):
        """(KT, RT): sum of the phases' interval counts, doubles of one instance's relative-error block."""
        kt, rt = C.c_int(), C.c_longlong()
        self._check(self._L.rpm_solution_error_batch_sizes(self._h, C.byref(kt), C.byref(rt)))
        return kt.value, rt.value

    def _phase_shapes(self):
        """Per phase (K_p, rows_p, nx_p)."""
        return _phase_shapes(self._L, self._h, self._desc, self.n_phases, self._check)

    def solution_error_batch(self, x, mask=None, full=False):
        """The mesh-error estimate of every instance -> dict(interval_error: per phase B x K_p, rel_err_max: per phase
        rows_p x nx_p (maximum over the instances `mask` includes), nonfinite: B ints, and with full=True rel_err: per phase
        B x rows_p x nx_p)."""
        return _batch_estimate(self._L.rpm_solution_error_batch, self._check, self._h, self._x(x), self.n_instances,
                               self.solution_error_batch_sizes(), self._phase_shapes(), mask, full)

    def solution_error_batch_dev(self, d_x, d_mask=None, d_interval_error=None, d_rel_err_max=None, d_rel_err=None,
                                 d_nonfinite=None, stream=None):
        """Device-resident form on torch CUDA tensors (float64; mask / nonfinite int32); results as flat arrays in the
        library's layout (rpm_hip.h).  Asynchronous on `stream`."""
        self._check(self._L.rpm_solution_error_batch_dev(self._h, self._ptr(d_x), self._ptr(d_mask), self._ptr(d_interval_error),
                                                         self._ptr(d_rel_err_max), self._ptr(d_rel_err), self._ptr(d_nonfinite),
                                                         self._stream(stream)))

    def split_rel_err(self, flat):
        """One block of RT doubles (or B of them) -> list per phase of rows_p x nx_p (B x rows_p x nx_p) arrays."""
        return _split_rel(np.asarray(flat), self._phase_shapes())

    def ph_refine_sweep(self, x, tol, nmin, nmax, mask=None):
        """The next mesh of the sweep: per phase ph_refine_from_error on rel_err_max (the worst included instance decides)."""
        est = self.solution_error_batch(x, mask)
        return [self.ph_refine_from_error(p, est["rel_err_max"][p], tol, nmin, nmax) for p in range(self.n_phases)]

    # ---- the sweep's solutions carried onto another mesh (rpm_carry_solution_batch*) -----------------------------------
    def carry_solution_batch(self, to, x):
        """The solutions x (n_instances x n) of this engine splined onto the mesh of engine `to` (same problem, any mesh)
        -> (x_to: n_instances x to.n, the next solve's starting points; nonfinite: n_instances ints)."""
        if self._L is not to._L:
            raise RpmError(RPM_E_INVALID, "carry_solution_batch: the engines must come from one native library")
        x = self._x(x)
        out = self._own("carry", self.n_instances * to.n)
        flags = np.zeros(self.n_instances, dtype=np.int32)
        self._check(self._L.rpm_carry_solution_batch(self._h, to._h, _dp(x), _dp(out), _ip(flags)))
        return out.reshape(self.n_instances, to.n).copy(), flags

    def carry_solution_batch_dev(self, to, d_x, d_x_to, d_nonfinite=None, stream=None):
        """Device-resident form on torch CUDA tensors (float64; d_nonfinite int32).  Asynchronous on `stream`."""
        self._check(self._L.rpm_carry_solution_batch_dev(self._h, to._h, self._ptr(d_x), self._ptr(d_x_to), self._ptr(d_nonfinite),
                                                         self._stream(stream)))

    # ---- the sweep's constraint multipliers carried onto another mesh (rpm_carry_multipliers_batch*) ---------------------
    def carry_multipliers_layout(self):
        """The row map of the multiplier carry, host only: (n_phases + 1) x 4 — per phase the first defect row, the first path
        row, the first event row and one past its last row; the last line: the rows after the phases, [first] * 3 + [m]."""
        rows = np.zeros((self.n_phases + 1, 4), dtype=np.int32)
        for p in range(self.n_phases + 1):
            self._check(self._L.rpm_carry_multipliers_layout(self._h, p, _ip(rows[p])))
        return rows

    def carry_multipliers_batch(self, to, x, lam):
        """The multipliers lam (n_instances x m) of this engine's solutions x carried as costates / path-multiplier densities
        onto the mesh of engine `to` -> (lambda_to: n_instances x to.m, a warm solve's starting lambda; nonfinite)."""
        if self._L is not to._L:
            raise RpmError(RPM_E_INVALID, "carry_multipliers_batch: the engines must come from one native library")
        x = self._x(x)
        lam = np.ascontiguousarray(lam, dtype=np.float64).ravel()
        if lam.size != self.n_instances * self.m:
            raise RpmError(RPM_E_INVALID, "lambda has %d entries, expected %d" % (lam.size, self.n_instances * self.m))
        out = np.zeros((self.n_instances, to.m))
        flags = np.zeros(self.n_instances, dtype=np.int32)
        self._check(self._L.rpm_carry_multipliers_batch(self._h, to._h, _dp(x), _dp(lam), _dp(out), _ip(flags)))
        return out, flags

    def carry_multipliers_batch_dev(self, to, d_x, d_lambda, d_lambda_to, d_nonfinite=None, stream=None):
        """Device-resident form on torch CUDA tensors (float64; d_nonfinite int32).  Asynchronous on `stream`."""
        self._check(self._L.rpm_carry_multipliers_batch_dev(self._h, to._h, self._ptr(d_x), self._ptr(d_lambda), self._ptr(d_lambda_to),
                                                            self._ptr(d_nonfinite), self._stream(stream)))

    # ---- the receding-horizon shift of the sweep's plan and duals (rpm_shift_plan_batch*) -------------------------------
    def shift_plan_batch(self, dt, x, lam=None, z=None):
        """Every instance's plan moved on by its own dt (n_instances x n_phases) on this engine's mesh: x (n_instances x n),
        lam (n_instances x m) or None, z = (z_L, z_U) (n_instances x n each) or None -> dict(x, nonfinite, and lambda / z_L, z_U
        where they were given)."""
        return _shift_plan(self._L.rpm_shift_plan_batch, self._check, self._h, self.n_instances, self.n_phases, self.n, self.m,
                           dt, x, lam, z)

    def shift_plan_batch_dev(self, d_dt, d_x, d_x_out, d_lambda=None, d_lambda_out=None, d_z_L=None, d_z_U=None, d_z_L_out=None,
                             d_z_U_out=None, d_nonfinite=None, stream=None):
        """Device-resident form on torch CUDA tensors (float64; d_nonfinite int32).  Asynchronous on `stream`."""
        self._check(self._L.rpm_shift_plan_batch_dev(self._h, self._ptr(d_dt), self._ptr(d_x), self._ptr(d_x_out), self._ptr(d_lambda),
                                                     self._ptr(d_lambda_out), self._ptr(d_z_L), self._ptr(d_z_U), self._ptr(d_z_L_out),
                                                     self._ptr(d_z_U_out), self._ptr(d_nonfinite), self._stream(stream)))

    # ---- the plans at caller-given times and the plant under them (rpm_sample_plan_batch*, rpm_rollout_batch*) ------------
    def sample_plan_batch(self, phase, x, times):
        """One phase's plans x (n_instances x n) at times (n_instances x n_times, the problem's time unit; outside the horizon
        the end values are held) -> (samples: n_instances x (nx + nu) x n_times, states first; nonfinite: n_instances ints)."""
        return _sample_plan(self._L.rpm_sample_plan_batch, self._check, self._h, self._desc, self.n_instances, self.n, phase, x, times)

    def sample_plan_batch_dev(self, phase, d_x, n_times, d_times, d_out, d_nonfinite=None, stream=None):
        """Device-resident form on torch CUDA tensors (float64; d_nonfinite int32).  Asynchronous on `stream`."""
        self._check(self._L.rpm_sample_plan_batch_dev(self._h, int(phase), self._ptr(d_x), int(n_times), self._ptr(d_times),
                                                      self._ptr(d_out), self._ptr(d_nonfinite), self._stream(stream)))

    def rollout_batch(self, phase, x, dt, n_steps, hold=0, state0=None, t_start=None, traj=False):
        """Every instance's own dynamics integrated under its plan x (n_instances x n) over dt (n_instances) in n_steps classical
        Runge-Kutta steps, from state0 (n_instances x nx; None: the plan's first state values) at t_start (n_instances; None: the
        phase's first time).  hold=1: the control of t_start for the whole call.  Controls are not clipped to their bounds.
        -> dict(state: n_instances x nx, nonfinite: n_instances ints, and with traj=True traj: n_instances x (n_steps + 1) x nx)."""
        return _rollout(self._L.rpm_rollout_batch, self._check, self._h, self._desc, self.n_instances, self.n, phase, x, dt, n_steps,
                        hold, state0, t_start, traj)

    def rollout_batch_dev(self, phase, d_x, d_dt, n_steps, d_state_out, hold=0, d_state0=None, d_t_start=None, d_traj=None,
                          d_nonfinite=None, stream=None):
        """Device-resident form on torch CUDA tensors (float64; d_nonfinite int32); d_state_out may be d_state0 (in place).
        One launch, asynchronous on `stream`."""
        self._check(self._L.rpm_rollout_batch_dev(self._h, int(phase), self._ptr(d_x), self._ptr(d_t_start), self._ptr(d_dt),
                                                  int(n_steps), int(hold), self._ptr(d_state0), self._ptr(d_state_out),
                                                  self._ptr(d_traj), self._ptr(d_nonfinite), self._stream(stream)))

    # ---- the extraction of a whole sweep: all phases, all instances (rpm_nlp2op_batch*) ---------------------------------
    def nlp2op_batch_layout(self):
        """(offsets, EB): per phase the offsets of time, state, control, costate, pathmult, hamiltonian, mayer_cost and
        lagrange_cost inside one instance's block (n_phases x 8), and the block's length in doubles.  Host only."""
        return _extract_layout(self._L, self._h, self.n_phases, self._check)

    def nlp2op_batch(self, x, lam):
        """Nlp2OpControl of every instance: x (n_instances x n), lam (n_instances x m) -> (per phase a dict with the keys of
        nlp2op_control, every array with a leading instance axis and the two costs as n_instances-vectors; nonfinite:
        n_instances ints)."""
        return _batch_extract(self._L.rpm_nlp2op_batch, self._check, self._h, self._x(x), lam, self.n_instances, self.m,
                              self.nlp2op_batch_layout())

    def nlp2op_batch_dev(self, d_x, d_lambda, d_out, d_nonfinite=None, stream=None):
        """Device-resident form on torch CUDA tensors (float64; d_out n_instances x EB in the library's layout, d_nonfinite
        int32).  Asynchronous on `stream`."""
        self._check(self._L.rpm_nlp2op_batch_dev(self._h, self._ptr(d_x), self._ptr(d_lambda), self._ptr(d_out),
                                                 self._ptr(d_nonfinite), self._stream(stream)))

    # ---- tables and sharding ---------------------------------------------------------------
    def phase_tables(self, phase):
        N, dn, on = C.c_int(), C.c_int(), C.c_int()
        self._check(self._L.rpm_get_phase_sizes(self._h, phase, C.byref(N), C.byref(dn), C.byref(on)))
        N, dn, on = N.value, dn.value, on.value
        t = dict(points=np.zeros(N), weights=np.zeros(N), d_rows=np.zeros(dn, dtype=np.int32),
                 d_cols=np.zeros(dn, dtype=np.int32), d_vals=np.zeros(dn), diag_vals=np.zeros(N),
                 doff_rows=np.zeros(on, dtype=np.int32), doff_cols=np.zeros(on, dtype=np.int32),
                 doff_vals=np.zeros(on))
        self._check(self._L.rpm_get_phase_tables(self._h, phase, _dp(t["points"]), _dp(t["weights"]),
                                                 _ip(t["d_rows"]), _ip(t["d_cols"]), _dp(t["d_vals"]),
                                                 _dp(t["diag_vals"]), _ip(t["doff_rows"]), _ip(t["doff_cols"]),
                                                 _dp(t["doff_vals"])))
        return t

    def shard_segments(self, which, rank):
        ns, pl = C.c_int(0), C.c_int(0)
        self._check(self._L.rpm_shard_segments(self._h, which, rank, None, C.byref(ns), C.byref(pl)))
        segs = (_abi.rpm_segment * max(ns.value, 1))()
        self._check(self._L.rpm_shard_segments(self._h, which, rank, segs, C.byref(ns), C.byref(pl)))
        return [(segs[i].off, segs[i].len, segs[i].pos) for i in range(ns.value)], pl.value

    def shard_pack_dev(self, which, d_full, d_packed, stream=None):
        self._check(self._L.rpm_shard_pack_dev(self._h, which, self._ptr(d_full), self._ptr(d_packed),
                                               self._stream(stream)))

    def shard_unpack_dev(self, which, d_gathered, stride, d_full, stream=None):
        self._check(self._L.rpm_shard_unpack_dev(self._h, which, self._ptr(d_gathered), int(stride),
                                                 self._ptr(d_full), self._stream(stream)))


    def shard_slot_len(self):
        v = C.c_longlong()
        self._check(self._L.rpm_shard_slot_len(self._h, C.byref(v)))
        return v.value

    def shard_pack_all_dev(self, d_g, d_values, d_slot, stream=None):
        self._check(self._L.rpm_shard_pack_all_dev(self._h, self._ptr(d_g), self._ptr(d_values), self._ptr(d_slot),
                                                   self._stream(stream)))

    def shard_unpack_all_dev(self, d_gathered, d_g, d_values, skip_own=True, stream=None):
        self._check(self._L.rpm_shard_unpack_all_dev(self._h, self._ptr(d_gathered), self._ptr(d_g), self._ptr(d_values),
                                                     1 if skip_own else 0, self._stream(stream)))


def _shift_plan(fn, check, handle, B, P, n, m, dt, x, lam, z):
    """The host form of the shift for an engine or a sweep: arrays checked for size, results as a dict."""
    def arr(a, cols, name):
        return _sized(a, B, cols, name)
    dt, x = arr(dt, P, "dt"), arr(x, n, "x")
    out = {"x": np.zeros((B, n)), "nonfinite": np.zeros(B, dtype=np.int32)}
    args = [None] * 6
    if lam is not None:
        out["lambda"] = np.zeros((B, m))
        args[0], args[1] = _dp(arr(lam, m, "lambda")), _dp(out["lambda"])
    if z is not None:
        out["z_L"], out["z_U"] = np.zeros((B, n)), np.zeros((B, n))
        args[2:] = [_dp(arr(z[0], n, "z_L")), _dp(arr(z[1], n, "z_U")), _dp(out["z_L"]), _dp(out["z_U"])]
    check(fn(handle, _dp(dt), _dp(x), _dp(out["x"]), *args, _ip(out["nonfinite"])))
    return out


def _sized(a, B, cols, name):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    if a.size != B * cols:
        raise RpmError(RPM_E_INVALID, "%s has %d entries, expected %d" % (name, a.size, B * cols))
    return a


def _phase_dims(desc, phase):
    """(nx, nu) of a phase; (0, 0) for an index out of range, which the library then refuses with its own message"""
    phase = int(phase)
    return (desc.phases[phase].nx, desc.phases[phase].nu) if 0 <= phase < desc.n_phases else (0, 0)


def _sample_plan(fn, check, handle, desc, B, n, phase, x, times):
    """The host form of the sampler for an engine or a sweep: arrays checked for size, results shaped."""
    nx, nu = _phase_dims(desc, phase)
    x = _sized(x, B, n, "x")
    times = np.ascontiguousarray(times, dtype=np.float64).ravel()
    if times.size % B:
        raise RpmError(RPM_E_INVALID, "times has %d entries, expected a multiple of %d" % (times.size, B))
    n_times = times.size // B
    out = np.zeros((B, nx + nu, max(n_times, 1)))
    flags = np.zeros(B, dtype=np.int32)
    check(fn(handle, int(phase), _dp(x), n_times, _dp(times), _dp(out), _ip(flags)))
    return out, flags


def _rollout(fn, check, handle, desc, B, n, phase, x, dt, n_steps, hold, state0, t_start, traj):
    """The host form of the roll-out for an engine or a sweep: arrays checked for size, results as a dict."""
    nx, _ = _phase_dims(desc, phase)
    n_steps = int(n_steps)
    x, dt = _sized(x, B, n, "x"), _sized(dt, B, 1, "dt")
    s0 = None if state0 is None else _sized(state0, B, nx, "state0")
    ts = None if t_start is None else _sized(t_start, B, 1, "t_start")
    out = {"state": np.zeros((B, nx)), "nonfinite": np.zeros(B, dtype=np.int32)}
    if traj:
        out["traj"] = np.zeros((B, max(n_steps, 0) + 1, nx))
    check(fn(handle, int(phase), _dp(x), None if ts is None else _dp(ts), _dp(dt), n_steps, int(hold), None if s0 is None else _dp(s0),
             _dp(out["state"]), _dp(out["traj"]) if traj else None, _ip(out["nonfinite"])))
    return out


class HpLiuRefiner:
    """LiuHpMeshRefineAlg behind rpm_hpliu_* (Core/LpLiuHpMeshRefineAlg.cpp): one object per problem, it keeps the
    reference's mesh / solution histories across meshes."""

    def __init__(self, n_phases, tol, nmax, ratio_r):
        self._args = (int(n_phases), float(tol), int(nmax), float(ratio_r))
        self._L = None          # the native object is created by the library of the first engine it refines
        self._h = None
        self.P = int(n_phases)

    def _ensure(self, engine):
        if self._h is not None:
            if engine._L is not self._L:
                raise RpmError(RPM_E_INVALID, "HpLiuRefiner: engines of one refinement history must come from one native library")
            return
        self._L = engine._L
        self._h = C.c_void_p()
        rc = self._L.rpm_hpliu_create(*self._args, C.byref(self._h))
        if rc != RPM_OK:
            self._h = None
            raise RpmError(rc, "rpm_hpliu_create: invalid arguments")

    def close(self):
        if getattr(self, "_h", None):
            self._L.rpm_hpliu_destroy(self._h)
            self._h = None

    __del__ = close

    def refine(self, engine, x=None, rel_err=None, capacity=8192):
        """-> (no_more_refine, [(mesh_points, nodes_per_interval) per phase]).  rel_err: list of per-phase relative-error
        matrices to decide from (host only); default: estimate on the device."""
        self._ensure(engine)
        xp = _dp(engine._x(x)) if x is not None else None
        rp = None
        if rel_err is not None:
            flat = np.concatenate([np.asfortranarray(r, dtype=np.float64).ravel(order="F") for r in rel_err])
            rp = _dp(flat)
        mesh, nodes = np.zeros(capacity), np.zeros(capacity, dtype=np.int32)
        moff, noff, nk = (np.zeros(self.P, dtype=np.int32) for _ in range(3))
        done = C.c_int()
        rc = self._L.rpm_hpliu_refine(self._h, engine._h, xp, rp, capacity, _dp(mesh), _ip(nodes), _ip(moff), _ip(noff),
                                      _ip(nk), C.byref(done))
        if rc != RPM_OK:
            raise RpmError(rc, self._L.rpm_last_error(engine._h).decode())
        return bool(done.value), [(mesh[moff[p]:moff[p] + nk[p] + 1].copy(), nodes[noff[p]:noff[p] + nk[p]].copy())
                                  for p in range(self.P)]



class BatchedIPM:
    """rpm_ipm_* : the NLP solve (the reference's NLPSolver::SolveNlp -> Ipopt, Core/LpNLPSolver.cpp:13-53) for all of an
    engine's instances at once, iterates and KKT factors resident on the device.  The engine's hessian-approximation option
    decides what stands for the Hessian: "exact" lpopc's finite-difference Hessian (rpm_eval_h), "limited-memory" (lpopc's
    default) Ipopt's limited-memory BFGS."""

    STATUS = {0: "converged", 1: "converged to the acceptable level", 2: "iteration limit", 3: "line search and restoration phase failed",
              4: "inertia correction failed", 5: "NaN/Inf"}

    def __init__(self, engine, **options):
        self._L = engine._L
        self._e = engine
        self._h = C.c_void_p()
        rc = self._L.rpm_ipm_create(engine._h, C.byref(self._h))
        if rc != RPM_OK:
            raise RpmError(rc, self._L.rpm_last_error(engine._h).decode())
        for k, v in options.items():
            self.set_option(k, v)

    def close(self):
        if getattr(self, "_h", None):
            self._L.rpm_ipm_destroy(self._h)
            self._h = None

    __del__ = close

    def _chk(self, rc):
        if rc != RPM_OK:
            raise RpmError(rc, self._L.rpm_ipm_last_error(self._h).decode())

    def set_option(self, key, value):
        if key == "mu_strategy" and isinstance(value, str):       # Ipopt's spelling, as the restatement takes it
            value = {"monotone": 0, "adaptive": 1}[value]
        self._chk(self._L.rpm_ipm_set_option(self._h, key.encode(), float(value)))

    def set_bounds(self, instance, x_l, x_u):
        x_l, x_u = np.ascontiguousarray(x_l, dtype=np.float64), np.ascontiguousarray(x_u, dtype=np.float64)
        assert x_l.size == self._e.n and x_u.size == self._e.n
        self._chk(self._L.rpm_ipm_set_bounds(self._h, int(instance), _dp(x_l), _dp(x_u)))

    def set_all_bounds(self, x_l, x_u):
        """x_l, x_u: (n_instances, n)."""
        x_l, x_u = np.ascontiguousarray(x_l, dtype=np.float64), np.ascontiguousarray(x_u, dtype=np.float64)
        assert x_l.shape == x_u.shape == (self._e.n_instances, self._e.n)
        self._chk(self._L.rpm_ipm_set_all_bounds(self._h, _dp(x_l), _dp(x_u)))

    def set_initial_states(self, phase, state0):
        """The measured initial states of `phase`, (n_instances, nx): lower = upper = state0 at every instance's initial
        states, every other bound left alone."""
        s0 = np.ascontiguousarray(state0, dtype=np.float64)
        nx = self._e._desc.phases[int(phase)].nx if 0 <= int(phase) < self._e.n_phases else 0
        if nx and s0.size != self._e.n_instances * nx:
            raise RpmError(RPM_E_INVALID, "state0 has %d entries, expected %d" % (s0.size, self._e.n_instances * nx))
        self._chk(self._L.rpm_ipm_set_initial_states(self._h, int(phase), _dp(s0)))

    def set_initial_states_dev(self, phase, d_state0, stream=None):
        """Device-resident form on a torch CUDA tensor (float64, n_instances x nx): one small launch on `stream`."""
        self._chk(self._L.rpm_ipm_set_initial_states_dev(self._h, int(phase), C.c_void_p(d_state0.data_ptr()),
                                                         NLPEngine._stream(stream)))

    def info(self):
        a = [C.c_int() for _ in range(4)]
        st, ns = C.c_longlong(), C.c_int()
        self._chk(self._L.rpm_ipm_get_info(self._h, C.byref(a[0]), C.byref(a[1]), C.byref(a[2]), C.byref(a[3]), C.byref(st), C.byref(ns)))
        return {"kkt_order": a[0].value, "band_order": a[1].value, "half_bandwidth": a[2].value, "border": a[3].value,
                "storage_doubles": st.value, "n_slacks": ns.value}

    def subproblems(self):
        """Geometry of the factorisation's sub-problems: rows of (order, banded part, border, half bandwidth, column stride)."""
        n = C.c_int()
        self._chk(self._L.rpm_ipm_get_subproblems(self._h, 0, None, C.byref(n)))
        g = np.zeros((n.value, 5), dtype=np.int32)
        self._chk(self._L.rpm_ipm_get_subproblems(self._h, n.value, _ip(g), C.byref(n)))
        return g

    def factor_flops(self):
        """Floating-point operations of one LDL^T of one instance (multiply-adds counted as 2), from the sub-problems."""
        total = 0.0
        for nt, nb_, nbd, b, _ in self.subproblems():
            j = np.arange(nb_)
            r = np.minimum(b, nb_ - 1 - j) + nbd          # rows below the pivot of band column j
            total += float(np.sum(r * (r + 1.0))) + nbd ** 3 / 3.0
        return total

    def stats(self):
        a = [C.c_int() for _ in range(3)]
        self._chk(self._L.rpm_ipm_get_stats(self._h, C.byref(a[0]), C.byref(a[1]), C.byref(a[2])))
        return {"iterations": a[0].value, "factorizations": a[1].value, "trial_points": a[2].value}

    def trace(self, instance, capacity=4096):
        """Accepted steps of the last solve (option trace > 0): rows of f, theta, mu, alpha, alpha_z, delta_w, E_0, backtracks."""
        rec = np.zeros((capacity, 8))
        n = C.c_int()
        self._chk(self._L.rpm_ipm_get_trace(self._h, int(instance), capacity, _dp(rec), C.byref(n)))
        return rec[:n.value].copy()

    def kernel_times(self):
        """Device milliseconds of the last solve inside the factorisation / the substitution kernels (HIP events)."""
        f, s = C.c_double(), C.c_double()
        self._chk(self._L.rpm_ipm_get_kernel_times(self._h, C.byref(f), C.byref(s)))
        return {"factor_ms": f.value, "substitution_ms": s.value}

    def restorations(self):
        out = np.zeros(self._e.n_instances, dtype=np.int32)
        self._chk(self._L.rpm_ipm_get_restorations(self._h, _ip(out)))
        return out

    def permutation(self):
        nt = self.info()["kkt_order"]
        pos = np.zeros(nt, dtype=np.int32)
        self._chk(self._L.rpm_ipm_get_permutation(self._h, _ip(pos), nt))
        return pos

    def debug_solve(self, k_storage, rhs):
        B, nt = self._e.n_instances, self.info()["kkt_order"]
        k = np.ascontiguousarray(k_storage, dtype=np.float64)
        r = np.ascontiguousarray(rhs, dtype=np.float64)
        assert k.size == B * self.info()["storage_doubles"] and r.size == B * nt
        sol = np.zeros((B, nt))
        npos, nneg = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        self._chk(self._L.rpm_ipm_debug_solve(self._h, _dp(k), _dp(r), _dp(sol), _ip(npos), _ip(nneg)))
        return sol, npos, nneg

    def debug_solve_dense(self, k_dense, rhs):
        """Factor + solve dense symmetric matrices (B, Nt, Nt) in unknown order; -> (solutions, n_pos, n_neg)."""
        B, nt = self._e.n_instances, self.info()["kkt_order"]
        k = np.ascontiguousarray(k_dense, dtype=np.float64)
        r = np.ascontiguousarray(rhs, dtype=np.float64)
        assert k.shape == (B, nt, nt) and r.shape == (B, nt)
        sol = np.zeros((B, nt))
        npos, nneg = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        self._chk(self._L.rpm_ipm_debug_solve_dense(self._h, _dp(k), _dp(r), _dp(sol), _ip(npos), _ip(nneg)))
        return sol, npos, nneg

    def slot(self, ua, uc):
        off = C.c_longlong()
        self._chk(self._L.rpm_ipm_debug_slot(self._h, int(ua), int(uc), C.byref(off)))
        return off.value

    def debug_storage(self):
        """The KKT storage as it stands (rpm_ipm_debug_storage; read-only), (n_instances, storage_doubles): after debug_solve[_dense]
        or debug_pass(3) the factors — d on the diagonal, L below, L11^-1 below the diagonal of every 16 x 16 diagonal block."""
        k = np.zeros((self._e.n_instances, self.info()["storage_doubles"]))
        self._chk(self._L.rpm_ipm_debug_storage(self._h, _dp(k)))
        return k

    def debug_lbfgs_step(self, x, glag_new, glag_old, reset=False, mode=None, status=None):
        """One pass of the limited-memory update (rpm_ipm_debug_lbfgs_step): x, glag_new, glag_old (n_instances, n); mode, status
        per instance (None = 0).  The first call of a sequence resets."""
        B, n = self._e.n_instances, self._e.n
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (x, glag_new, glag_old)]
        assert all(v.shape == (B, n) for v in a)
        flags = [None if f is None else np.ascontiguousarray(f, dtype=np.int32) for f in (mode, status)]
        assert all(f is None or f.shape == (B,) for f in flags)
        self._chk(self._L.rpm_ipm_debug_lbfgs_step(self._h, int(bool(reset)), _dp(a[0]), _dp(a[1]), _dp(a[2]),
                                                   *[None if f is None else _ip(f) for f in flags]))

    def debug_lbfgs_state(self):
        """-> dict(record (B, 8): sigma, pairs held, consecutive skips, previous iterate valid, updates, skips, two decision words;
        M (B, 12, 12); S, Y (B, 6, n), oldest pair first)."""
        B, n = self._e.n_instances, self._e.n
        out = {"record": np.zeros((B, 8)), "M": np.zeros((B, 12, 12)), "S": np.zeros((B, 6, n)), "Y": np.zeros((B, 6, n))}
        self._chk(self._L.rpm_ipm_debug_lbfgs_state(self._h, _dp(out["record"]), _dp(out["M"]), _dp(out["S"]), _dp(out["Y"])))
        return out

    def debug_lbfgs_solve(self, rows, cols, vals, rhs):
        """(K0 - E M^-1 E') d = rhs with the memory as it stands: K0 as lower-triangle entries (rows >= cols, unknown order),
        vals (n_instances, nnz), rhs (n_instances, Nt) -> d (n_instances, Nt)."""
        B, nt = self._e.n_instances, self.info()["kkt_order"]
        rows, cols = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)
        v, r = np.ascontiguousarray(vals, dtype=np.float64), np.ascontiguousarray(rhs, dtype=np.float64)
        assert rows.shape == cols.shape == (v.shape[1],) and v.shape[0] == B and r.shape == (B, nt)
        sol = np.zeros((B, nt))
        self._chk(self._L.rpm_ipm_debug_lbfgs_solve(self._h, rows.size, _ip(rows), _ip(cols), _dp(v), _dp(r), _dp(sol)))
        return sol

    def solve(self, x0, lam0=None, z0=None):
        """x0: (n_instances, n) starting points -> dict(x, lambda, obj, status, iterations, kkt_error).  lam0 (n_instances, m):
        warm start in the primal and the dual (rpm_ipm_solve_warm); z0 = (z_L, z_U), (n_instances, n) each, or None: the bound
        multipliers from mu_init.  With z0 the dict also holds z_L and z_U."""
        B, n, m = self._e.n_instances, self._e.n, self._e.m
        x = np.array(x0, dtype=np.float64, order="C").reshape(B, n)
        obj, err = np.zeros(B), np.zeros(B)
        status, iters = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        if lam0 is None:
            if z0 is not None:
                raise RpmError(RPM_E_INVALID, "solve: z0 needs lam0")
            lam = np.zeros((B, max(m, 1)))[:, :m].copy()
            self._chk(self._L.rpm_ipm_solve(self._h, _dp(x), _dp(lam), _dp(obj), _ip(status), _ip(iters), _dp(err)))
            return {"x": x, "lambda": lam, "obj": obj, "status": status, "iterations": iters, "kkt_error": err}
        lam = np.array(lam0, dtype=np.float64, order="C").reshape(B, m)
        out = {"x": x, "lambda": lam, "obj": obj, "status": status, "iterations": iters, "kkt_error": err}
        zl = zu = None
        if z0 is not None:
            zl, zu = (np.array(z, dtype=np.float64, order="C").reshape(B, n) for z in z0)
            out["z_L"], out["z_U"] = zl, zu
        self._chk(self._L.rpm_ipm_solve_warm(self._h, _dp(x), _dp(lam), None if zl is None else _dp(zl), None if zu is None else _dp(zu),
                                             _dp(obj), _ip(status), _ip(iters), _dp(err)))
        return out

    def bound_multipliers(self):
        """(z_L, z_U), (n_instances, n) each: the multipliers of the variables' bounds after the last solve, unscaled."""
        B, n = self._e.n_instances, self._e.n
        zl, zu = np.zeros((B, n)), np.zeros((B, n))
        self._chk(self._L.rpm_ipm_get_bound_multipliers(self._h, _dp(zl), _dp(zu)))
        return zl, zu

    def bound_multipliers_dev(self, d_z_L, d_z_U, stream=None):
        self._chk(self._L.rpm_ipm_get_bound_multipliers_dev(self._h, C.c_void_p(d_z_L.data_ptr()), C.c_void_p(d_z_U.data_ptr()),
                                                            NLPEngine._stream(stream)))

    # ---- solution sensitivities to fixed variables (rpm_ipm_sensitivities, include/rpm_hip.h) --------------------------

    def initial_state_variables(self, phase):
        """The variables set_initial_states writes: x_state0 + j (N + 1), j < nx of `phase`."""
        if not 0 <= int(phase) < self._e.n_phases:
            raise RpmError(RPM_E_INVALID, "phase %d is out of range" % int(phase))
        out = np.zeros(self._e._desc.phases[int(phase)].nx, dtype=np.int32)
        self._chk(self._L.rpm_ipm_initial_state_variables(self._h, int(phase), _ip(out)))
        return out

    def parameter_variables(self, phase):
        """The static parameters of `phase`: x_t0 + 2 + j, j < nq.  Fixed in the plan (parameter_min == parameter_max) they are
        what sensitivities() differentiates with respect to."""
        if not 0 <= int(phase) < self._e.n_phases:
            raise RpmError(RPM_E_INVALID, "phase %d is out of range" % int(phase))
        out = np.zeros(self._e._desc.phases[int(phase)].nq, dtype=np.int32)
        self._chk(self._L.rpm_ipm_parameter_variables(self._h, int(phase), _ip(out)))
        return out

    @staticmethod
    def _var_index(var_index):
        return None if var_index is None else np.ascontiguousarray(var_index, dtype=np.int32).ravel()

    def sensitivities(self, var_index, want_lambda=True, _fn=None):
        """First-order sensitivities of the solution the solver holds to the fixed variables `var_index` (P of them):
        dict(dx (B, P, n), dlambda (B, P, m) or None, delta_w (B), info (B): 0 computed, 1 computed with a regularised matrix,
        2 left out (NaN blocks))."""
        B, n, m = self._e.n_instances, self._e.n, self._e.m
        vi = self._var_index(var_index)
        P = 0 if vi is None else vi.size
        out = {"dx": np.zeros((B, P, n)), "dlambda": np.zeros((B, P, m)) if want_lambda else None, "delta_w": np.zeros(B),
               "info": np.zeros(B, dtype=np.int32)}
        self._chk((_fn or self._L.rpm_ipm_sensitivities)(self._h, P, None if vi is None else _ip(vi), _dp(out["dx"]),
                                                         _dp(out["dlambda"]) if want_lambda else None, _dp(out["delta_w"]), _ip(out["info"])))
        return out

    def sensitivities_dev(self, var_index, d_dx, d_dlambda=None, stream=None, _fn=None):
        """The device-resident form on torch CUDA tensors (float64): d_dx (B, P, n), d_dlambda (B, P, m) or None, written when
        the call returns -> dict(delta_w, info)."""
        B = self._e.n_instances
        vi = self._var_index(var_index)
        out = {"delta_w": np.zeros(B), "info": np.zeros(B, dtype=np.int32)}
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk((_fn or self._L.rpm_ipm_sensitivities_dev)(self._h, 0 if vi is None else vi.size, None if vi is None else _ip(vi), ptr(d_dx),
                                                             ptr(d_dlambda), _dp(out["delta_w"]), _ip(out["info"]), NLPEngine._stream(stream)))
        return out

    def apply_sensitivities(self, var_index, dx, delta, x, dlambda=None, lam=None, _fn=None):
        """The predictor x + sum_k dx[:, k] delta[:, k] (and lambda likewise when dlambda and lam are given), nothing clipped:
        -> x_out (B, n), or (x_out, lambda_out)."""
        B, n, m = self._e.n_instances, self._e.n, self._e.m
        vi = self._var_index(var_index)
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        dx, delta, x, dlambda, lam = f(dx), f(delta), f(x), f(dlambda), f(lam)
        x_out = np.zeros((B, n))
        lam_out = np.zeros((B, m)) if dlambda is not None and lam is not None else None
        opt = lambda a: None if a is None else _dp(a)
        self._chk((_fn or self._L.rpm_ipm_apply_sensitivities)(self._h, 0 if vi is None else vi.size, None if vi is None else _ip(vi), opt(dx),
                                                               opt(dlambda), opt(delta), opt(x), _dp(x_out), opt(lam), opt(lam_out)))
        return x_out if lam_out is None else (x_out, lam_out)

    def apply_sensitivities_dev(self, var_index, d_dx, d_delta, d_x, d_x_out, d_dlambda=None, d_lambda=None, d_lambda_out=None, stream=None,
                                _fn=None):
        """One launch on `stream` (torch's current one by default) over torch CUDA tensors; capturable into a graph."""
        vi = self._var_index(var_index)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk((_fn or self._L.rpm_ipm_apply_sensitivities_dev)(self._h, 0 if vi is None else vi.size, None if vi is None else _ip(vi),
                                                                   ptr(d_dx), ptr(d_dlambda), ptr(d_delta), ptr(d_x), ptr(d_x_out), ptr(d_lambda),
                                                                   ptr(d_lambda_out), NLPEngine._stream(stream)))

    def debug_sensitivity_rhs(self, var_index, _fn=None):
        """Test hook: the right-hand sides of sensitivities() -> (B, P, kkt_order), unknown order (variables, slacks, multipliers)."""
        vi = self._var_index(var_index)
        P = 0 if vi is None else vi.size
        rhs = np.zeros((self._e.n_instances, P, self.info()["kkt_order"]))
        self._chk((_fn or self._L.rpm_ipm_debug_sensitivity_rhs)(self._h, P, None if vi is None else _ip(vi), _dp(rhs)))
        return rhs

    # ---- solution sensitivities to the instances' constants (rpm_ipm_constant_sensitivities, include/rpm_hip.h): the calls above
    # with a list of constants (indices into the functor's constants) in place of the list of fixed variables

    def constant_sensitivities(self, const_index, want_lambda=True):
        """First-order sensitivities of the solution the solver holds to the constants `const_index` of every instance (its own,
        set_instance_constants, or the shared ones): the dict of sensitivities(); dx is 0 on every fixed variable."""
        return self.sensitivities(const_index, want_lambda, _fn=self._L.rpm_ipm_constant_sensitivities)

    def constant_sensitivities_dev(self, const_index, d_dx, d_dlambda=None, stream=None):
        return self.sensitivities_dev(const_index, d_dx, d_dlambda, stream, _fn=self._L.rpm_ipm_constant_sensitivities_dev)

    def apply_constant_sensitivities(self, const_index, dx, delta, x, dlambda=None, lam=None):
        """The predictor for moves `delta` (B, P) of the listed constants."""
        return self.apply_sensitivities(const_index, dx, delta, x, dlambda, lam, _fn=self._L.rpm_ipm_apply_constant_sensitivities)

    def apply_constant_sensitivities_dev(self, const_index, d_dx, d_delta, d_x, d_x_out, d_dlambda=None, d_lambda=None, d_lambda_out=None,
                                         stream=None):
        self.apply_sensitivities_dev(const_index, d_dx, d_delta, d_x, d_x_out, d_dlambda, d_lambda, d_lambda_out, stream,
                                     _fn=self._L.rpm_ipm_apply_constant_sensitivities_dev)

    def debug_constant_sensitivity_rhs(self, const_index):
        """Test hook: the right-hand sides of constant_sensitivities() -> (B, P, kkt_order), unknown order."""
        return self.debug_sensitivity_rhs(const_index, _fn=self._L.rpm_ipm_debug_constant_sensitivity_rhs)

    def debug_start(self, x0, lam0=None, z0=None, warm=True):
        """The state the iteration loop starts from (rpm_ipm_debug_start; no step is taken): dict(v (B, nv): x then the slacks,
        zL, zU (B, nv), lambda (B, m), mu (B), status (B)).  warm=False: the cold start (lam0, z0 ignored)."""
        B, n, m = self._e.n_instances, self._e.n, self._e.m
        nv = n + self.info()["n_slacks"]
        x = np.array(x0, dtype=np.float64, order="C").reshape(B, n)
        lam = None if lam0 is None else np.array(lam0, dtype=np.float64, order="C").reshape(B, m)
        zl, zu = (None, None) if z0 is None else (np.array(z, dtype=np.float64, order="C").reshape(B, n) for z in z0)
        out = {"v": np.zeros((B, nv)), "zL": np.zeros((B, nv)), "zU": np.zeros((B, nv)), "lambda": np.zeros((B, m)), "mu": np.zeros(B),
               "status": np.zeros(B, dtype=np.int32)}
        opt = lambda a: None if a is None else _dp(a)
        self._chk(self._L.rpm_ipm_debug_start(self._h, int(bool(warm)), _dp(x), opt(lam), opt(zl), opt(zu), _dp(out["v"]), _dp(out["zL"]),
                                              _dp(out["zU"]), _dp(out["lambda"]), _dp(out["mu"]), _ip(out["status"])))
        return out

    def debug_pass(self, stage):
        """The loop's own next steps on the state debug_start has just made (rpm_ipm_debug_pass; valid only directly after
        debug_start).  stage 1: evaluation + residual pass; 2: + Hessian and KKT assembly; 3: + factorisation, substitution and the
        direction kernel.  -> dict of everything the hook returns, n_instances rows each: obj, grad, g, jac, c, glag, hess, K
        (the KKT storage), rhs (unknown order; after stage 3 the solution), dv, dlam, dzL, dzU, record (_abi.IPM_RECORD_FIELDS), and
        inst: the record as a dict of (n_instances,) arrays by field name."""
        B, n, m = self._e.n_instances, self._e.n, self._e.m
        info = self.info()
        nv = n + info["n_slacks"]
        width = {"obj": 1, "grad": n, "g": m, "jac": self._e.nnz_jac, "c": m, "glag": nv, "hess": self._e.nnz_h if self._e._desc.hessian_approximation in (1, 2) else 0,   # (limited-memory: none)
                 "K": info["storage_doubles"], "rhs": info["kkt_order"], "dv": nv,
                 "dlam": m, "dzL": nv, "dzU": nv, "record": _abi.RPM_IPM_RECORD_DOUBLES}
        out = {k: np.full((B, width[k]), np.nan) for k in _abi.IPM_PASS_OUTPUTS}
        self._chk(self._L.rpm_ipm_debug_pass(self._h, int(stage), *[_dp(out[k]) for k in _abi.IPM_PASS_OUTPUTS]))
        out["obj"] = out["obj"][:, 0]
        out["inst"] = {name: out["record"][:, k] for k, name in enumerate(_abi.IPM_RECORD_FIELDS)}
        return out

    def debug_line_search(self, rounds=1, filt=None):
        """Rounds of the line search on the direction debug_pass(3) has just left, or further rounds (rpm_ipm_debug_line_search;
        valid only directly after debug_pass(3) with an instance left running, or after itself).  filt: per instance a sequence of
        (theta, phi) pairs that replaces its filter before the first round.  -> dict, n_instances rows each: xt, objt, gt, ct,
        csoc, dv2, dlam2, dzL2, dzU2, soc_rhs (the correction's right-hand side, NaN where the last round ran none), rhs (its
        solution), record, inst (the record by field name), counts (line searches pending, corrections asked for)."""
        B, n, m = self._e.n_instances, self._e.n, self._e.m
        info = self.info()
        nv, nt = n + info["n_slacks"], info["kkt_order"]
        width = {"xt": n, "objt": 1, "gt": m, "ct": m, "csoc": m, "dv2": nv, "dlam2": m, "dzL2": nv, "dzU2": nv, "soc_rhs": nt, "rhs": nt,
                 "record": _abi.RPM_IPM_RECORD_DOUBLES}
        out = {k: np.full((B, width[k]), np.nan) for k in _abi.IPM_LINE_SEARCH_OUTPUTS}
        k, pairs, count = 0, None, None
        if filt is not None:
            assert len(filt) == B
            count = np.array([len(f) for f in filt], dtype=np.int32)
            k = int(count.max()) if B else 0
            pairs = np.zeros((B, max(k, 1), 2))
            for b, f in enumerate(filt):
                if len(f):
                    pairs[b, :len(f)] = np.asarray(f, dtype=np.float64).reshape(len(f), 2)
            pairs = np.ascontiguousarray(pairs[:, :k]) if k else None
        counts = np.zeros(2, dtype=np.int32)
        self._chk(self._L.rpm_ipm_debug_line_search(self._h, int(rounds), k, None if pairs is None else _dp(pairs),
                                                    None if count is None else _ip(count),
                                                    *[_dp(out[key]) for key in _abi.IPM_LINE_SEARCH_OUTPUTS], _ip(counts)))
        out["objt"] = out["objt"][:, 0]
        out["inst"] = {name: out["record"][:, i] for i, name in enumerate(_abi.IPM_RECORD_FIELDS)}
        out["counts"] = (int(counts[0]), int(counts[1]))
        return out

    def debug_update(self, n_filter=8):
        """IpmLoop::update on what debug_line_search has just left (rpm_ipm_debug_update; valid only directly after it).  -> dict,
        n_instances rows each: v, zL, zU, lambda, filter (n_filter pairs, inst["nfilt"] of them count), vR, dr2, pp, nn, zp, zn,
        lb_gold (limited-memory: grad_x L(x_old, lambda_new)), record, inst."""
        B, n, m = self._e.n_instances, self._e.n, self._e.m
        nv = n + self.info()["n_slacks"]
        width = {"v": nv, "zL": nv, "zU": nv, "lambda": m, "filter": 2 * int(n_filter), "vR": nv, "dr2": nv, "pp": m, "nn": m, "zp": m, "zn": m,
                 "lb_gold": n, "record": _abi.RPM_IPM_RECORD_DOUBLES}
        out = {k: np.full((B, width[k]), np.nan) for k in _abi.IPM_UPDATE_OUTPUTS}
        a = [_dp(out[k]) for k in _abi.IPM_UPDATE_OUTPUTS]
        self._chk(self._L.rpm_ipm_debug_update(self._h, *a[:4], int(n_filter), *a[4:]))
        out["filter"] = out["filter"].reshape(B, int(n_filter), 2)
        out["inst"] = {name: out["record"][:, i] for i, name in enumerate(_abi.IPM_RECORD_FIELDS)}
        return out

    def solve_dev(self, d_x, d_lambda=None, stream=None, d_z_L=None, d_z_U=None, warm=False):
        """d_x: torch CUDA tensor (n_instances, n), overwritten with the solutions; d_lambda: optional (n_instances, m).
        The solver waits for what is queued on `stream` (default: torch's current stream) before it touches the arrays.
        warm=True: rpm_ipm_solve_warm_dev — d_lambda (required) and d_z_L / d_z_U (n_instances, n; both or neither) are read as
        the starting duals and overwritten with the solution's."""
        B = self._e.n_instances
        obj, err = np.zeros(B), np.zeros(B)
        status, iters = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        if warm:
            self._chk(self._L.rpm_ipm_solve_warm_dev(self._h, ptr(d_x), ptr(d_lambda), ptr(d_z_L), ptr(d_z_U), _dp(obj), _ip(status),
                                                     _ip(iters), _dp(err), NLPEngine._stream(stream)))
        else:
            if d_z_L is not None or d_z_U is not None:
                raise RpmError(RPM_E_INVALID, "solve_dev: d_z_L / d_z_U need warm=True")
            self._chk(self._L.rpm_ipm_solve_dev(self._h, ptr(d_x), ptr(d_lambda), _dp(obj), _ip(status), _ip(iters), _dp(err),
                                                NLPEngine._stream(stream)))
        return {"obj": obj, "status": status, "iterations": iters, "kkt_error": err}
