"""ctypes binding of the C-ABI in include/mfgpu.h (test / bench harness plumbing).

The product is the shared library dealii-cuda_amd/lib/libmfgpu.so (hand-written HIP kernels
behind a C-ABI) and the C++ shim in dealii-cuda_amd/host/.  This module only loads that library;
it has NO fallback: if the library is missing or a call fails it raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MFGPU_LIB selects another build of the SAME sources (tools/stamps.py: lib/libmfgpu_diag.so)
LIB_PATH = os.environ.get("MFGPU_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libmfgpu.so")

F64, F32 = 0, 1
OK, EINVAL = 0, -1  # MFGPU_OK, MFGPU_EINVAL
EUNSUPPORTED = -4
MULTI_ADD, MULTI_LOOP, MULTI_FUSED = 1, 2, 4  # flags of Operator.vmult_multi
UNIFORM_J0, HANGING_NODES, COLORED_SCATTER, NO_SHARED_RECORDS = 1, 2, 1 << 8, 1 << 9
UPDATABLE_COEFFICIENTS = 1 << 10  # keep what update_coefficients (and Integrator.evaluate's gradients) read on the device
KERNEL_AUTO, KERNEL_PENCILS, KERNEL_PENCILS_X, KERNEL_PLANES, KERNEL_PLANES_2W = 0, 1, 2, 3, 4  # Desc.kernel


class MfgpuError(RuntimeError):
    pass


class Desc(C.Structure):
    """mirror of struct mfgpu_desc"""
    _fields_ = [
        ("dim", C.c_int32), ("degree", C.c_int32), ("number_type", C.c_int32), ("flags", C.c_uint32),
        ("n_dofs", C.c_uint32), ("n_cells", C.c_uint32),
        ("loc2glob", C.c_void_p), ("constraint_mask", C.c_void_p),
        ("JxW", C.c_void_p), ("inv_jac", C.c_void_p), ("coefficient", C.c_void_p),
        ("quadrature_points", C.c_void_p), ("shape_values", C.c_void_p), ("shape_gradients", C.c_void_p),
        ("constraint_weights", C.c_void_p), ("constrained_dofs", C.c_void_p),
        ("n_constrained", C.c_uint32), ("max_cells_per_batch", C.c_uint32), ("max_dofs_per_batch", C.c_uint32),
        ("kernel", C.c_uint32), ("cell_loop_segments", C.c_uint32), ("max_workgroups", C.c_uint32),
        ("mass_coefficient", C.c_void_p),
    ]


CG_NONE, CG_JACOBI, CG_CHEBYSHEV, CG_CALLBACK = 0, 1, 2, 3  # preconditioner of CG (MFGPU_CG_*)
CG_STATE_BYTES, CG_PARTIAL_BYTES = 128, 3 * 2048 * 8  # the fixed device blocks of a CG (mfgpu_cg_create)
BICGSTAB_STATE_BYTES, BICGSTAB_PARTIAL_BYTES = 128, 6 * 2048 * 8  # ... and of a BiCGStab (mfgpu_bicgstab_create)


class CGInfo(C.Structure):
    """mirror of struct mfgpu_cg_info; status: 0 running, 1 converged, 2 max iterations, 3 breakdown"""
    _fields_ = [("iterations", C.c_uint32), ("status", C.c_uint32), ("residual", C.c_double),
                ("initial_residual", C.c_double)]

    def as_tuple(self):
        return int(self.iterations), int(self.status), float(self.residual), float(self.initial_residual)


VCYCLE_COARSE_AUTO, VCYCLE_COARSE_DENSE, VCYCLE_COARSE_CG = 0, 1, 2  # VCycleDesc.coarse (MFGPU_VCYCLE_COARSE_*)
VCYCLE_DENSE_MAX = 2048
SPD_INVERSE_DEVICE_MAX = 512  # MFGPU_SPD_INVERSE_DEVICE_MAX
EIG_STATE_BYTES, EIG_PARTIAL_BYTES = 64, 2 * 2048 * 8  # the fixed blocks of mfgpu_eig_workspace_bytes


class EigResult(C.Structure):
    """mirror of struct mfgpu_eig_result, the head of the workspace of estimate_lambda_max_enqueue; status: 0 running,
    1 stopped by the 1 % rule, 2 n_steps used up, 3 a norm was not a positive finite number"""
    _fields_ = [("lambda_max", C.c_double), ("estimate", C.c_double), ("steps", C.c_uint32), ("status", C.c_uint32)]


class VCycleRefreshInfo(C.Structure):
    """mirror of struct mfgpu_vcycle_refresh_info"""
    _fields_ = [("coarse_status", C.c_uint32), ("eig_status_max", C.c_uint32), ("eig_steps_max", C.c_uint32),
                ("reserved", C.c_uint32)]


class VCycleLevelDesc(C.Structure):
    """mirror of struct mfgpu_vcycle_level_desc"""
    _fields_ = [("op", C.c_void_p), ("edges", C.c_void_p), ("from_coarser", C.c_void_p), ("to_mg", C.c_void_p),
                ("from_mg", C.c_void_p)]


class VCycleDesc(C.Structure):
    """mirror of struct mfgpu_vcycle_desc"""
    _fields_ = [("n_levels", C.c_uint32), ("levels", C.POINTER(VCycleLevelDesc)), ("active_type", C.c_int32),
                ("n_active", C.c_uint32), ("smoother_degree", C.c_uint32), ("smoothing_range", C.c_double),
                ("eig_iterations", C.c_uint32), ("lambda_max", C.POINTER(C.c_double)), ("coarse", C.c_uint32),
                ("coarse_tolerance", C.c_double), ("coarse_max_iterations", C.c_uint32)]


# terms of a QpOperator (MFGPU_QOP_*) and the flag of its vmult
QOP_DIFFUSION_SCALAR, QOP_DIFFUSION_TENSOR, QOP_CONVECTION, QOP_FLUX, QOP_REACTION = 1, 2, 4, 8, 16
QOP_TRANSPOSE = 1


class QopCoefficients(C.Structure):
    """mirror of struct mfgpu_qop_coefficients (device pointers)"""
    _fields_ = [("diffusion", C.c_void_p), ("convection", C.c_void_p), ("flux", C.c_void_p), ("reaction", C.c_void_p)]


# terms of a VectorQpOperator (MFGPU_VQOP_*)
VQOP_ISOTROPIC, VQOP_TENSOR4, VQOP_MASS = 1, 2, 4


class VqopCoefficients(C.Structure):
    """mirror of struct mfgpu_vqop_coefficients (device pointers)"""
    _fields_ = [("lam", C.c_void_p), ("mu", C.c_void_p), ("tensor", C.c_void_p), ("mass", C.c_void_p)]


# int fn(void *ctx, void *z_dev, const void *r_dev, void *stream)
CG_CALLBACK_TYPE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


# every symbol include/mfgpu.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "mfgpu_vmult_multi", "mfgpu_multi_width", "mfgpu_plan_multi_groups",
    "mfgpu_create", "mfgpu_vmult", "mfgpu_vmult_add", "mfgpu_n_dofs", "mfgpu_memory_consumption",
    "mfgpu_destroy", "mfgpu_last_error", "mfgpu_plan_stats", "mfgpu_kernel_name", "mfgpu_compute_inverse_diagonal", "mfgpu_set_constrained_values",
    "mfgpu_vec_sadd", "mfgpu_vec_equ", "mfgpu_vec_scale", "mfgpu_vec_divide", "mfgpu_vec_invert", "mfgpu_vec_mul",
    "mfgpu_vec_dot", "mfgpu_vec_l2_norm", "mfgpu_vec_add_and_dot", "mfgpu_vec_all_zero", "mfgpu_profile_enable", "mfgpu_profile_read", "mfgpu_profile_read_pass2",
    "mfgpu_plan_create", "mfgpu_plan_destroy", "mfgpu_plan_array_u32", "mfgpu_plan_lmap", "mfgpu_plan_bflags",
    "mfgpu_plan_shares_records", "mfgpu_record_stats",
    "mfgpu_vec_alloc", "mfgpu_vec_free", "mfgpu_vec_fill", "mfgpu_vec_from_host", "mfgpu_vec_to_host",
    "mfgpu_device_synchronize", "mfgpu_device_memory_info", "mfgpu_mesh_create_uniform", "mfgpu_mesh_create_adaptive", "mfgpu_mesh_create_ball", "mfgpu_mesh_create_from_leaves",
    "mfgpu_mesh_cell_levels", "mfgpu_mesh_destroy",
    "mfgpu_mesh_desc", "mfgpu_mesh_dof_coords", "mfgpu_mesh_interface_dofs",
    "mfgpu_dist_unique_id", "mfgpu_dist_create", "mfgpu_dist_connect_local", "mfgpu_dist_attach", "mfgpu_dist_schedule",
    "mfgpu_vmult_dist_begin", "mfgpu_vmult_dist_end", "mfgpu_vmult_dist", "mfgpu_dist_destroy",
    "mfgpu_transfer_create", "mfgpu_transfer_create_from_meshes", "mfgpu_transfer_prolongate",
    "mfgpu_transfer_restrict_and_add", "mfgpu_transfer_memory_consumption", "mfgpu_transfer_destroy",
    "mfgpu_mesh_transfer_patches", "mfgpu_suggest_renumbering", "mfgpu_mesh_renumber",
    "mfgpu_level_create", "mfgpu_level_operator", "mfgpu_level_vmult_interface_down", "mfgpu_level_vmult_interface_up",
    "mfgpu_level_destroy", "mfgpu_index_pairs_create", "mfgpu_vec_copy_pairs", "mfgpu_index_pairs_destroy",
    "mfgpu_mesh_create_adaptive_mg", "mfgpu_mg_hierarchy_create", "mfgpu_mg_n_levels", "mfgpu_mg_level_mesh",
    "mfgpu_mg_edge_dofs", "mfgpu_mg_copy_pairs", "mfgpu_mg_transfer_arrays", "mfgpu_mg_hierarchy_destroy",
    "mfgpu_integrator_create", "mfgpu_integrator_rhs", "mfgpu_integrator_l2_error", "mfgpu_integrator_error_points",
    "mfgpu_integrator_destroy",
    "mfgpu_vec_convert", "mfgpu_vec_copy_pairs_convert", "mfgpu_vec_chebyshev_start", "mfgpu_vec_chebyshev_update",
    "mfgpu_desc_size",
    "mfgpu_update_coefficients", "mfgpu_level_update_coefficients", "mfgpu_integrator_update_coefficients",
    "mfgpu_integrator_evaluate",
    "mfgpu_cg_create", "mfgpu_cg_set_callback", "mfgpu_cg_begin", "mfgpu_cg_iterate", "mfgpu_cg_status", "mfgpu_cg_solve",
    "mfgpu_cg_memory_consumption", "mfgpu_cg_destroy", "mfgpu_cg_chebyshev_scalars",
    "mfgpu_cg_begin_relative", "mfgpu_cg_set_vcycle", "mfgpu_transfer_prolongate_add", "mfgpu_vec_residual",
    "mfgpu_vcycle_create", "mfgpu_vcycle_apply", "mfgpu_vcycle_lambda_max", "mfgpu_vcycle_memory_consumption",
    "mfgpu_vcycle_destroy", "mfgpu_estimate_lambda_max", "mfgpu_spd_inverse",
    "mfgpu_vec_chebyshev_start_dev", "mfgpu_vec_chebyshev_update_dev", "mfgpu_cg_chebyshev_scalars_dev",
    "mfgpu_eig_workspace_bytes", "mfgpu_estimate_lambda_max_enqueue", "mfgpu_spd_inverse_workspace_bytes",
    "mfgpu_spd_inverse_enqueue", "mfgpu_vcycle_refresh", "mfgpu_vcycle_refresh_status", "mfgpu_estimate_lambda_max_steps",
    "mfgpu_transfer_create_p", "mfgpu_transfer_create_p_from_meshes", "mfgpu_transfer_p_prolongation_1d",
    "mfgpu_transfer_create_p_hn", "mfgpu_transfer_create_p_hn_from_meshes", "mfgpu_transfer_p_owner_list",
    "mfgpu_mesh_coarsen_leaves", "mfgpu_mesh_coarsening_map", "mfgpu_transfer_create_h_hn",
    "mfgpu_transfer_create_h_hn_from_meshes",
    "mfgpu_integrator_recovery_indicator", "mfgpu_mesh_refine_leaves",
    "mfgpu_mesh_adapt_leaves", "mfgpu_transfer_create_h_hn_interp", "mfgpu_transfer_create_h_hn_interp_from_meshes",
    "mfgpu_transfer_interpolate",
    "mfgpu_locate_points", "mfgpu_points_create", "mfgpu_points_create_in_cells", "mfgpu_points_cells",
    "mfgpu_points_n_not_found", "mfgpu_points_evaluate", "mfgpu_points_integrate", "mfgpu_points_memory_consumption",
    "mfgpu_points_destroy",
    "mfgpu_locator_create", "mfgpu_locator_locate", "mfgpu_locator_memory_consumption", "mfgpu_locator_destroy",
    "mfgpu_points_create_located",
    "mfgpu_debug_guard_begin", "mfgpu_debug_guard_end", "mfgpu_debug_guard_layout", "mfgpu_debug_guard_check",
    "mfgpu_debug_guard_selftest",
    "mfgpu_integrator_integrate", "mfgpu_qop_create", "mfgpu_qop_set_coefficients", "mfgpu_qop_vmult",
    "mfgpu_qop_compute_inverse_diagonal", "mfgpu_qop_memory_consumption", "mfgpu_qop_destroy",
    "mfgpu_bicgstab_create", "mfgpu_bicgstab_set_operator", "mfgpu_bicgstab_set_operator_handle",
    "mfgpu_bicgstab_set_operator_qop", "mfgpu_bicgstab_set_callback", "mfgpu_bicgstab_set_vcycle", "mfgpu_bicgstab_begin",
    "mfgpu_bicgstab_begin_relative", "mfgpu_bicgstab_iterate", "mfgpu_bicgstab_status", "mfgpu_bicgstab_solve",
    "mfgpu_bicgstab_memory_consumption", "mfgpu_bicgstab_destroy",
    "mfgpu_vqop_create", "mfgpu_vqop_set_coefficients", "mfgpu_vqop_vmult", "mfgpu_vqop_compute_inverse_diagonal",
    "mfgpu_vqop_set_constrained_values", "mfgpu_vqop_memory_consumption", "mfgpu_vqop_destroy",
    "mfgpu_bicgstab_set_operator_vqop",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MfgpuError(f"{LIB_PATH} not found: build it with __graft_entry__.build() "
                             "(make -C dealii-cuda_amd); there is no fallback path")
        L = C.CDLL(LIB_PATH)
        L.mfgpu_last_error.restype = C.c_char_p
        L.mfgpu_create.argtypes = [C.POINTER(Desc), C.POINTER(C.c_void_p)]
        L.mfgpu_desc_size.argtypes = []
        L.mfgpu_desc_size.restype = C.c_size_t
        L.mfgpu_vmult.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_vmult_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_n_dofs.argtypes = [C.c_void_p]
        L.mfgpu_n_dofs.restype = C.c_uint32
        L.mfgpu_memory_consumption.argtypes = [C.c_void_p]
        L.mfgpu_memory_consumption.restype = C.c_size_t
        L.mfgpu_destroy.argtypes = [C.c_void_p]
        L.mfgpu_destroy.restype = None
        L.mfgpu_plan_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.mfgpu_device_memory_info.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.mfgpu_kernel_name.argtypes = [C.c_void_p]
        L.mfgpu_kernel_name.restype = C.c_char_p
        L.mfgpu_compute_inverse_diagonal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_set_constrained_values.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
        vp, d, z, i = C.c_void_p, C.c_double, C.c_size_t, C.c_int
        L.mfgpu_vec_sadd.argtypes = [vp, d, d, vp, z, i, vp]
        L.mfgpu_vec_equ.argtypes = [vp, d, vp, z, i, vp]
        L.mfgpu_vec_scale.argtypes = [vp, vp, z, i, vp]
        L.mfgpu_vec_divide.argtypes = [vp, vp, z, i, vp]
        L.mfgpu_vec_invert.argtypes = [vp, z, i, vp]
        L.mfgpu_vec_mul.argtypes = [vp, d, z, i, vp]
        L.mfgpu_vec_dot.argtypes = [vp, vp, z, i, vp, C.POINTER(d)]
        L.mfgpu_vec_l2_norm.argtypes = [vp, z, i, vp, C.POINTER(d)]
        L.mfgpu_vec_add_and_dot.argtypes = [vp, d, vp, vp, z, i, vp, C.POINTER(d)]
        L.mfgpu_vec_all_zero.argtypes = [vp, z, i, vp, C.POINTER(i)]
        L.mfgpu_profile_enable.argtypes = [C.c_void_p, C.c_int]
        L.mfgpu_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.mfgpu_profile_read_pass2.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.mfgpu_plan_create.argtypes = [C.POINTER(Desc), C.POINTER(C.c_void_p)]
        L.mfgpu_plan_destroy.argtypes = [C.c_void_p]
        L.mfgpu_plan_destroy.restype = None
        L.mfgpu_plan_array_u32.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.mfgpu_plan_array_u32.restype = C.c_int64
        L.mfgpu_plan_lmap.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.mfgpu_plan_lmap.restype = C.c_int64
        L.mfgpu_plan_bflags.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.mfgpu_plan_bflags.restype = C.c_int64
        L.mfgpu_plan_shares_records.argtypes = [C.c_void_p]
        L.mfgpu_record_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.mfgpu_vec_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_int]
        L.mfgpu_vec_free.argtypes = [C.c_void_p]
        L.mfgpu_vec_fill.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_void_p]
        L.mfgpu_vec_from_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.mfgpu_vec_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.mfgpu_mesh_create_uniform.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_double, C.c_double,
                                                C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.mfgpu_mesh_create_adaptive.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.mfgpu_mesh_create_ball.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.mfgpu_mesh_create_from_leaves.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.mfgpu_mesh_cell_levels.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.mfgpu_mesh_cell_levels.restype = C.c_int64
        L.mfgpu_mesh_destroy.argtypes = [C.c_void_p]
        L.mfgpu_mesh_destroy.restype = None
        L.mfgpu_mesh_desc.argtypes = [C.c_void_p, C.POINTER(Desc)]
        L.mfgpu_mesh_dof_coords.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.mfgpu_mesh_dof_coords.restype = C.c_int64
        L.mfgpu_mesh_interface_dofs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.mfgpu_mesh_interface_dofs.restype = C.c_int64
        L.mfgpu_transfer_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
        L.mfgpu_transfer_create_from_meshes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.mfgpu_transfer_prolongate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_transfer_restrict_and_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_transfer_memory_consumption.argtypes = [C.c_void_p]
        L.mfgpu_transfer_memory_consumption.restype = C.c_size_t
        L.mfgpu_mesh_transfer_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_mesh_transfer_patches.restype = C.c_int64
        L.mfgpu_suggest_renumbering.argtypes = [C.POINTER(Desc), C.c_void_p]
        L.mfgpu_mesh_renumber.argtypes = [C.c_void_p, C.c_void_p]
        L.mfgpu_level_create.argtypes = [C.POINTER(Desc), C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mfgpu_level_operator.argtypes = [C.c_void_p]
        L.mfgpu_level_operator.restype = C.c_void_p
        L.mfgpu_level_vmult_interface_down.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_level_vmult_interface_up.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_mesh_create_adaptive_mg.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.mfgpu_mg_hierarchy_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.mfgpu_mg_n_levels.argtypes = [C.c_void_p]
        L.mfgpu_mg_level_mesh.argtypes = [C.c_void_p, C.c_int]
        L.mfgpu_mg_level_mesh.restype = C.c_void_p
        L.mfgpu_mg_edge_dofs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.mfgpu_mg_edge_dofs.restype = C.c_int64
        L.mfgpu_mg_copy_pairs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.mfgpu_mg_copy_pairs.restype = C.c_int64
        L.mfgpu_mg_transfer_arrays.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.mfgpu_mg_transfer_arrays.restype = C.c_int64
        L.mfgpu_mg_hierarchy_destroy.argtypes = [C.c_void_p]
        L.mfgpu_mg_hierarchy_destroy.restype = None
        L.mfgpu_index_pairs_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mfgpu_vec_copy_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mfgpu_index_pairs_destroy.argtypes = [C.c_void_p]
        L.mfgpu_index_pairs_destroy.restype = None
        L.mfgpu_level_destroy.argtypes = [C.c_void_p]
        L.mfgpu_level_destroy.restype = None
        L.mfgpu_transfer_destroy.argtypes = [C.c_void_p]
        L.mfgpu_transfer_destroy.restype = None
        L.mfgpu_integrator_create.argtypes = [C.POINTER(Desc), C.POINTER(C.c_void_p)]
        L.mfgpu_integrator_rhs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_integrator_l2_error.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_double)]
        L.mfgpu_integrator_error_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_integrator_destroy.argtypes = [C.c_void_p]
        L.mfgpu_integrator_destroy.restype = None
        L.mfgpu_vec_convert.argtypes = [vp, i, vp, i, z, vp]
        L.mfgpu_update_coefficients.argtypes = [vp, vp, vp, vp]
        L.mfgpu_level_update_coefficients.argtypes = [vp, vp, vp, vp]
        L.mfgpu_integrator_update_coefficients.argtypes = [vp, vp, vp, vp]
        L.mfgpu_integrator_evaluate.argtypes = [vp, vp, vp, vp, vp]
        L.mfgpu_vec_copy_pairs_convert.argtypes = [vp, vp, i, vp, i, vp]
        L.mfgpu_vec_chebyshev_start.argtypes = [vp, vp, vp, vp, vp, vp, d, i, z, i, vp]
        L.mfgpu_vec_chebyshev_update.argtypes = [vp, vp, vp, vp, vp, d, d, z, i, vp]
        L.mfgpu_vmult_multi.argtypes = [vp, vp, vp, C.c_uint32, z, C.c_uint32, vp]
        L.mfgpu_multi_width.argtypes = [vp]
        L.mfgpu_plan_multi_groups.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32),
                                              C.c_uint32]
        u32 = C.c_uint32
        L.mfgpu_cg_create.argtypes = [vp, i, vp, u32, d, d, C.POINTER(vp)]
        L.mfgpu_cg_set_callback.argtypes = [vp, CG_CALLBACK_TYPE, vp]
        L.mfgpu_cg_begin.argtypes = [vp, vp, vp, d, u32, vp]
        L.mfgpu_cg_iterate.argtypes = [vp, u32, vp]
        L.mfgpu_cg_status.argtypes = [vp, vp, C.POINTER(CGInfo)]
        L.mfgpu_cg_solve.argtypes = [vp, vp, vp, d, u32, u32, vp, C.POINTER(CGInfo)]
        L.mfgpu_cg_memory_consumption.argtypes = [vp]
        L.mfgpu_cg_memory_consumption.restype = C.c_size_t
        L.mfgpu_cg_destroy.argtypes = [vp]
        L.mfgpu_cg_destroy.restype = None
        L.mfgpu_cg_chebyshev_scalars.argtypes = [u32, d, d, C.POINTER(d)]
        L.mfgpu_cg_begin_relative.argtypes = [vp, vp, vp, d, u32, vp]
        L.mfgpu_cg_set_vcycle.argtypes = [vp, vp]
        L.mfgpu_bicgstab_create.argtypes = [C.c_size_t, i, i, vp, C.POINTER(vp)]
        L.mfgpu_bicgstab_set_operator.argtypes = [vp, CG_CALLBACK_TYPE, vp]
        L.mfgpu_bicgstab_set_operator_handle.argtypes = [vp, vp]
        L.mfgpu_bicgstab_set_operator_qop.argtypes = [vp, vp, u32]
        L.mfgpu_bicgstab_set_callback.argtypes = [vp, CG_CALLBACK_TYPE, vp]
        L.mfgpu_bicgstab_set_vcycle.argtypes = [vp, vp]
        L.mfgpu_bicgstab_begin.argtypes = [vp, vp, vp, d, u32, vp]
        L.mfgpu_bicgstab_begin_relative.argtypes = [vp, vp, vp, d, u32, vp]
        L.mfgpu_bicgstab_iterate.argtypes = [vp, u32, vp]
        L.mfgpu_bicgstab_status.argtypes = [vp, vp, C.POINTER(CGInfo)]
        L.mfgpu_bicgstab_solve.argtypes = [vp, vp, vp, d, u32, u32, vp, C.POINTER(CGInfo)]
        L.mfgpu_bicgstab_memory_consumption.argtypes = [vp]
        L.mfgpu_bicgstab_memory_consumption.restype = C.c_size_t
        L.mfgpu_bicgstab_destroy.argtypes = [vp]
        L.mfgpu_bicgstab_destroy.restype = None
        L.mfgpu_transfer_prolongate_add.argtypes = [vp, vp, vp, vp]
        L.mfgpu_vec_residual.argtypes = [vp, vp, vp, z, i, vp]
        L.mfgpu_vcycle_create.argtypes = [C.POINTER(VCycleDesc), C.POINTER(vp)]
        L.mfgpu_vcycle_apply.argtypes = [vp, vp, vp, vp]
        L.mfgpu_vcycle_lambda_max.argtypes = [vp, C.POINTER(d)]
        L.mfgpu_vcycle_memory_consumption.argtypes = [vp]
        L.mfgpu_vcycle_memory_consumption.restype = C.c_size_t
        L.mfgpu_vcycle_destroy.argtypes = [vp]
        L.mfgpu_vcycle_destroy.restype = None
        L.mfgpu_estimate_lambda_max.argtypes = [vp, vp, u32, C.POINTER(d)]
        L.mfgpu_spd_inverse.argtypes = [u32, vp, vp]
        L.mfgpu_vec_chebyshev_start_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, z, i, vp]
        L.mfgpu_vec_chebyshev_update_dev.argtypes = [vp, vp, vp, vp, vp, vp, z, i, vp]
        L.mfgpu_cg_chebyshev_scalars_dev.argtypes = [u32, vp, d, vp, vp]
        L.mfgpu_eig_workspace_bytes.argtypes = [u32, i]
        L.mfgpu_eig_workspace_bytes.restype = C.c_size_t
        L.mfgpu_estimate_lambda_max_enqueue.argtypes = [vp, vp, u32, u32, vp, vp]
        L.mfgpu_spd_inverse_workspace_bytes.argtypes = [u32]
        L.mfgpu_spd_inverse_workspace_bytes.restype = C.c_size_t
        L.mfgpu_spd_inverse_enqueue.argtypes = [u32, vp, u32, vp, u32, vp, vp, vp]
        L.mfgpu_vcycle_refresh.argtypes = [vp, u32, vp]
        L.mfgpu_estimate_lambda_max_steps.argtypes = [vp, vp, u32, C.POINTER(d), C.POINTER(u32)]
        L.mfgpu_vcycle_refresh_status.argtypes = [vp, vp, C.POINTER(VCycleRefreshInfo)]
        L.mfgpu_transfer_create_p.argtypes = [i, i, i, i, u32, vp, vp, u32, u32, vp, u32, vp, C.POINTER(vp)]
        L.mfgpu_transfer_create_p_from_meshes.argtypes = [vp, vp, C.POINTER(vp)]
        L.mfgpu_transfer_p_prolongation_1d.argtypes = [i, i, vp]
        L.mfgpu_transfer_create_p_hn.argtypes = [i, i, i, i, u32, vp, vp, u32, u32, vp, u32, vp, vp, vp, C.POINTER(vp)]
        L.mfgpu_transfer_create_p_hn_from_meshes.argtypes = [vp, vp, C.POINTER(vp)]
        L.mfgpu_transfer_p_owner_list.argtypes = [i, i, u32, vp, vp, u32, vp]
        L.mfgpu_mesh_coarsen_leaves.argtypes = [i, vp, u32, vp]
        L.mfgpu_mesh_coarsen_leaves.restype = C.c_int64
        L.mfgpu_mesh_coarsening_map.argtypes = [vp, vp, vp, vp]
        L.mfgpu_transfer_create_h_hn.argtypes = [i, i, i, u32, u32, vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp,
                                                 C.POINTER(vp)]
        L.mfgpu_transfer_create_h_hn_from_meshes.argtypes = [vp, vp, C.POINTER(vp)]
        L.mfgpu_integrator_recovery_indicator.argtypes = [vp, vp, vp, vp, vp]
        L.mfgpu_mesh_refine_leaves.argtypes = [i, vp, u32, vp, u32, vp, C.c_uint64]
        L.mfgpu_mesh_refine_leaves.restype = C.c_int64
        L.mfgpu_mesh_adapt_leaves.argtypes = [i, vp, u32, vp, vp, u32, vp, C.c_uint64, vp, C.POINTER(u32)]
        L.mfgpu_mesh_adapt_leaves.restype = C.c_int64
        L.mfgpu_transfer_create_h_hn_interp.argtypes = [i, i, i, u32, u32, vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp,
                                                        vp, C.POINTER(vp)]
        L.mfgpu_transfer_create_h_hn_interp_from_meshes.argtypes = [vp, vp, C.POINTER(vp)]
        L.mfgpu_transfer_interpolate.argtypes = [vp, vp, vp, vp]
        L.mfgpu_locate_points.argtypes = [C.POINTER(Desc), vp, u32, vp, vp, C.POINTER(u32)]
        L.mfgpu_points_create.argtypes = [vp, C.POINTER(Desc), vp, u32, C.POINTER(vp)]
        L.mfgpu_points_create_in_cells.argtypes = [vp, vp, vp, u32, C.POINTER(vp)]
        L.mfgpu_points_cells.argtypes = [vp, C.POINTER(vp)]
        L.mfgpu_points_cells.restype = C.c_int64
        L.mfgpu_points_n_not_found.argtypes = [vp]
        L.mfgpu_points_n_not_found.restype = u32
        L.mfgpu_points_evaluate.argtypes = [vp, vp, vp, vp, vp]
        L.mfgpu_points_integrate.argtypes = [vp, vp, vp, vp]
        L.mfgpu_points_memory_consumption.argtypes = [vp]
        L.mfgpu_points_memory_consumption.restype = C.c_size_t
        L.mfgpu_points_destroy.argtypes = [vp]
        L.mfgpu_points_destroy.restype = None
        L.mfgpu_locator_create.argtypes = [vp, C.POINTER(Desc), C.POINTER(vp)]
        L.mfgpu_locator_locate.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
        L.mfgpu_locator_memory_consumption.argtypes = [vp]
        L.mfgpu_locator_memory_consumption.restype = C.c_size_t
        L.mfgpu_locator_destroy.argtypes = [vp]
        L.mfgpu_locator_destroy.restype = None
        L.mfgpu_points_create_located.argtypes = [vp, vp, vp, u32, vp, C.POINTER(vp)]
        u64p = C.POINTER(C.c_uint64)
        L.mfgpu_debug_guard_begin.argtypes = [z]
        L.mfgpu_debug_guard_end.argtypes = []
        L.mfgpu_debug_guard_layout.argtypes = [z, z, C.POINTER(z), C.POINTER(z)]
        L.mfgpu_debug_guard_check.argtypes = [u64p, u64p, C.c_char_p, z]
        L.mfgpu_debug_guard_selftest.argtypes = [u64p, C.c_char_p, z, C.POINTER(i), C.POINTER(i)]
        L.mfgpu_integrator_integrate.argtypes = [vp, vp, vp, vp, vp]
        L.mfgpu_qop_create.argtypes = [vp, u32, C.POINTER(vp)]
        L.mfgpu_qop_set_coefficients.argtypes = [vp, C.POINTER(QopCoefficients), vp]
        L.mfgpu_qop_vmult.argtypes = [vp, vp, vp, u32, vp]
        L.mfgpu_qop_compute_inverse_diagonal.argtypes = [vp, vp, vp]
        L.mfgpu_qop_memory_consumption.argtypes = [vp]
        L.mfgpu_qop_memory_consumption.restype = C.c_size_t
        L.mfgpu_qop_destroy.argtypes = [vp]
        L.mfgpu_qop_destroy.restype = None
        L.mfgpu_vqop_create.argtypes = [vp, u32, vp, C.c_size_t, C.POINTER(vp)]
        L.mfgpu_vqop_set_coefficients.argtypes = [vp, C.POINTER(VqopCoefficients), vp]
        L.mfgpu_vqop_vmult.argtypes = [vp, vp, vp, vp]
        L.mfgpu_vqop_compute_inverse_diagonal.argtypes = [vp, vp, vp]
        L.mfgpu_vqop_set_constrained_values.argtypes = [vp, vp, C.c_double, vp]
        L.mfgpu_vqop_memory_consumption.argtypes = [vp]
        L.mfgpu_vqop_memory_consumption.restype = C.c_size_t
        L.mfgpu_vqop_destroy.argtypes = [vp]
        L.mfgpu_vqop_destroy.restype = None
        L.mfgpu_bicgstab_set_operator_vqop.argtypes = [vp, vp]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        err = MfgpuError(f"mfgpu error {rc}: {lib().mfgpu_last_error().decode()}")
        err.code = rc
        raise err


def np_dtype(number_type):
    return np.float64 if number_type == F64 else np.float32


def _view(ptr, count, dtype):
    if count <= 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=count)


class Mesh:
    """Host-side stand-in for Triangulation + DoFHandler + ConstraintMatrix (mfgpu_mesh_*)."""

    def __init__(self, handle, keep=None):
        self._h = handle
        self._keep = keep
        self.desc = Desc()
        _check(lib().mfgpu_mesh_desc(self._h, C.byref(self.desc)))

    @classmethod
    def uniform(cls, dim, degree, n_per_dir, lo=-1.0, hi=1.0, slab=(0, 0), number_type=F64):
        if np.isscalar(n_per_dir):
            n_per_dir = [int(n_per_dir)] * dim
        arr = (C.c_uint32 * 3)(*(list(n_per_dir) + [1] * (3 - len(n_per_dir))))
        h = C.c_void_p()
        _check(lib().mfgpu_mesh_create_uniform(dim, degree, arr, lo, hi, slab[0], slab[1], number_type, C.byref(h)))
        return cls(h)

    @classmethod
    def adaptive(cls, dim, degree, n_ref, number_type=F64):
        h = C.c_void_p()
        _check(lib().mfgpu_mesh_create_adaptive(dim, degree, n_ref, number_type, C.byref(h)))
        return cls(h)

    @classmethod
    def adaptive_mg(cls, dim, degree, n_ref, number_type=F64):
        """the ADAPTIVE_GRID recipe with 2:1 balance over vertices too (what the multigrid hierarchy needs)"""
        h = C.c_void_p()
        _check(lib().mfgpu_mesh_create_adaptive_mg(dim, degree, n_ref, number_type, C.byref(h)))
        return cls(h)

    @classmethod
    def ball(cls, dim, degree, n_ref, number_type=F64):
        h = C.c_void_p()
        _check(lib().mfgpu_mesh_create_ball(dim, degree, n_ref, number_type, C.byref(h)))
        return cls(h)

    @classmethod
    def from_leaves(cls, dim, degree, leaves, number_type=F64):
        lv = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 4)
        h = C.c_void_p()
        _check(lib().mfgpu_mesh_create_from_leaves(dim, degree, lv.ctypes.data, len(lv), number_type, C.byref(h)))
        return cls(h)

    @staticmethod
    def coarsen_leaves(dim, leaves):
        """one step of global coarsening of the leaves (level, cx, cy, cz) (mfgpu_mesh_coarsen_leaves): complete families
        become their parent unless that breaks one-irregularity; [n_coarse, 4]; host only"""
        lv = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 4)
        out = np.zeros((max(len(lv), 1), 4), dtype=np.uint32)
        n = lib().mfgpu_mesh_coarsen_leaves(dim, lv.ctypes.data if len(lv) else None, len(lv), out.ctypes.data)
        if n < 0:
            _check(int(n))
        return out[:n].copy()

    @staticmethod
    def refine_leaves(dim, leaves, flags, balance_vertices=False):
        """one refinement step of the leaves (level, cx, cy, cz) (mfgpu_mesh_refine_leaves): the flagged leaves and
        whatever one-irregularity forces become their children, in the parent's place; [n_fine, 4]; host only.  With
        balance_vertices the leaves must be one-irregular over vertices too (Mesh.adaptive_mg, results of this call
        with balance_vertices): the call balances what it splits, it does not repair an unbalanced input"""
        lv = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 4)
        fl = np.ascontiguousarray(np.asarray(flags) != 0, dtype=np.uint8).reshape(-1)
        if len(fl) != len(lv):
            raise MfgpuError("Mesh.refine_leaves: one flag per leaf")
        cap = max(len(lv), 1) * 2 ** dim  # no leaf splits twice
        out = np.zeros((cap, 4), dtype=np.uint32)
        n = lib().mfgpu_mesh_refine_leaves(dim, lv.ctypes.data if len(lv) else None, len(lv),
                                           fl.ctypes.data if len(fl) else None, int(bool(balance_vertices)),
                                           out.ctypes.data, cap)
        if n < 0:
            _check(int(n))
        return out[:n].copy()

    def refined(self, flags, degree=None, balance_vertices=False, number_type=None):
        """a new leaf mesh: this adaptive or from-leaves mesh with the flagged cells (one flag per cell, in cell order)
        refined by Mesh.refine_leaves, at `degree` and `number_type` (default: this mesh's).  Transfer.h_hn_from_meshes
        (self, result) and coarsening_map(self, result) apply to the pair when the degrees are equal."""
        leaves = self.cell_levels()
        if not len(leaves):
            raise MfgpuError("Mesh.refined: needs a leaf mesh (Mesh.adaptive, Mesh.adaptive_mg, Mesh.from_leaves)")
        dim = int(self.desc.dim)
        return Mesh.from_leaves(dim, int(self.desc.degree) if degree is None else int(degree),
                                Mesh.refine_leaves(dim, leaves, flags, balance_vertices),
                                number_type=int(self.desc.number_type) if number_type is None else number_type)

    @staticmethod
    def adapt_leaves(dim, leaves, refine, coarsen, balance_vertices=False):
        """one step of refinement and coarsening of the leaves (level, cx, cy, cz) (mfgpu_mesh_adapt_leaves): (new, mid),
        [n_new, 4] and [n_mid, 4].  Refinement wins; a family of siblings that all carry a coarsen flag becomes its parent
        unless that breaks one-irregularity; `mid` is the input with exactly those families replaced, the common
        coarsening of the input and `new`; host only"""
        lv = np.ascontiguousarray(leaves, dtype=np.uint32).reshape(-1, 4)
        rf = np.ascontiguousarray(np.asarray(refine) != 0, dtype=np.uint8).reshape(-1)
        cf = np.ascontiguousarray(np.asarray(coarsen) != 0, dtype=np.uint8).reshape(-1)
        if len(rf) != len(lv) or len(cf) != len(lv):
            raise MfgpuError("Mesh.adapt_leaves: one refine flag and one coarsen flag per leaf")
        cap = max(len(lv), 1) * 2 ** dim  # no leaf splits twice
        new, mid = np.zeros((cap, 4), dtype=np.uint32), np.zeros((max(len(lv), 1), 4), dtype=np.uint32)
        n_mid = C.c_uint32(0)
        n = lib().mfgpu_mesh_adapt_leaves(dim, lv.ctypes.data if len(lv) else None, len(lv),
                                          rf.ctypes.data if len(rf) else None, cf.ctypes.data if len(cf) else None,
                                          int(bool(balance_vertices)), new.ctypes.data, cap, mid.ctypes.data,
                                          C.byref(n_mid))
        if n < 0:
            _check(int(n))
        return new[:n].copy(), mid[:n_mid.value].copy()

    def adapted(self, refine, coarsen, degree=None, balance_vertices=False, number_type=None):
        """(new_mesh, mid_mesh): this adaptive or from-leaves mesh adapted by Mesh.adapt_leaves (one flag of each kind per
        cell, in cell order), at `degree` and `number_type` (default: this mesh's).  The h_hn creators and coarsening_map
        apply to (mid_mesh, self) and (mid_mesh, new_mesh) when the degrees are equal (carry_over)."""
        leaves = self.cell_levels()
        if not len(leaves):
            raise MfgpuError("Mesh.adapted: needs a leaf mesh (Mesh.adaptive, Mesh.adaptive_mg, Mesh.from_leaves)")
        dim = int(self.desc.dim)
        p = int(self.desc.degree) if degree is None else int(degree)
        nt = int(self.desc.number_type) if number_type is None else number_type
        new, mid = Mesh.adapt_leaves(dim, leaves, refine, coarsen, balance_vertices)
        return Mesh.from_leaves(dim, p, new, number_type=nt), Mesh.from_leaves(dim, p, mid, number_type=nt)

    @classmethod
    def coarsening_sequence(cls, mesh, degree=None, min_cells=None):
        """the meshes of global coarsening, coarse to fine (deal.II's create_geometric_coarsening_sequence): the leaves of
        `mesh` coarsened step by step while a step leaves at least min_cells (default 2^dim) cells, each a
        Mesh.from_leaves at `degree` (default: the mesh's) in the mesh's number type; the last one is `mesh` itself when
        `degree` is its own"""
        dim, p, nt = int(mesh.desc.dim), int(mesh.desc.degree), int(mesh.desc.number_type)
        degree = p if degree is None else int(degree)
        min_cells = 2 ** dim if min_cells is None else int(min_cells)
        leaves = mesh.cell_levels()
        if not len(leaves):
            raise MfgpuError("Mesh.coarsening_sequence: needs a leaf mesh (Mesh.adaptive, Mesh.adaptive_mg, Mesh.from_leaves)")
        out = [mesh if degree == p else cls.from_leaves(dim, degree, leaves, number_type=nt)]
        while len(leaves) > 1:
            leaves = cls.coarsen_leaves(dim, leaves)
            if len(leaves) < min_cells:
                break
            out.append(cls.from_leaves(dim, degree, leaves, number_type=nt))
        return out[::-1]

    def cell_levels(self):
        p = C.c_void_p()
        cnt = lib().mfgpu_mesh_cell_levels(self._h, C.byref(p))
        return _view(p.value, cnt, np.uint32).reshape(-1, 4).copy()

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(self, "_owner", None) is None:
            _lib.mfgpu_mesh_destroy(self._h)  # (_lib is None at interpreter shutdown)
            self._h = None

    # ---- numpy views of the description arrays (valid while the mesh lives)
    @property
    def n_dofs(self):
        return int(self.desc.n_dofs)

    @property
    def n_cells(self):
        return int(self.desc.n_cells)

    @property
    def nd(self):
        return (self.desc.degree + 1) ** self.desc.dim

    def arrays(self):
        d = self.desc
        dt = np_dtype(d.number_type)
        nd, nc, n = self.nd, d.n_cells, d.degree + 1
        out = dict(
            loc2glob=_view(d.loc2glob, nc * nd, np.uint32).reshape(nc, nd),
            JxW=_view(d.JxW, nc * nd, dt).reshape(nc, nd),
            inv_jac=(_view(d.inv_jac, nc, dt) if d.flags & UNIFORM_J0
                     else _view(d.inv_jac, nc * nd * d.dim * d.dim, dt).reshape(nc, nd, d.dim, d.dim)),
            quadrature_points=_view(d.quadrature_points, nc * nd * d.dim, dt).reshape(nc, nd, d.dim),
            shape_values=_view(d.shape_values, n * n, dt),
            shape_gradients=_view(d.shape_gradients, n * n, dt),
            constraint_weights=_view(d.constraint_weights, n * n, np.float64),
            constrained_dofs=_view(d.constrained_dofs, d.n_constrained, np.uint32),
            constraint_mask=_view(d.constraint_mask, nc, np.uint32) if d.constraint_mask else None,
        )
        return out

    def set_mass_coefficient(self, c):
        """desc.mass_coefficient = c [n_cells * (p+1)^dim] in the mesh's number type (None: no mass term); the array is
        kept alive by the mesh.  Objects created from self.desc afterwards carry the term."""
        if c is None:
            self._mass, self.desc.mass_coefficient = None, None
            return
        self._mass = np.ascontiguousarray(c, dtype=np_dtype(self.desc.number_type)).reshape(-1)
        assert self._mass.size == self.n_cells * self.nd
        self.desc.mass_coefficient = self._mass.ctypes.data

    def dof_coords(self):
        p = C.c_void_p()
        cnt = lib().mfgpu_mesh_dof_coords(self._h, C.byref(p))
        return _view(p.value, cnt, np.float64).reshape(-1, self.desc.dim)

    def suggest_renumbering(self):
        """new_index[old] = new, batch-major for the operator's plan (mfgpu_suggest_renumbering); host only"""
        out = np.zeros(self.n_dofs, dtype=np.uint32)
        _check(lib().mfgpu_suggest_renumbering(C.byref(self.desc), out.ctypes.data))
        return out

    def renumber(self, new_index):
        """DoFHandler::renumber_dofs on the stand-in mesh (in place).  self.desc is refilled from the mesh: set the
        tuning knobs (kernel, max_*_per_batch, ...) again afterwards."""
        ni = np.ascontiguousarray(new_index, dtype=np.uint32)
        assert ni.size == self.n_dofs
        _check(lib().mfgpu_mesh_renumber(self._h, ni.ctypes.data))
        _check(lib().mfgpu_mesh_desc(self._h, C.byref(self.desc)))

    def transfer_patches(self, fine: "Mesh"):
        """(coarse_cell_dofs, fine_patch_dofs) of the level pair (self, fine): host arrays, no GPU"""
        p, dim = self.desc.degree, self.desc.dim
        cd = np.zeros((self.n_cells, (p + 1) ** dim), dtype=np.uint32)
        fd = np.zeros((self.n_cells, (2 * p + 1) ** dim), dtype=np.uint32)
        rc = lib().mfgpu_mesh_transfer_patches(self._h, fine._h, cd.ctypes.data, fd.ctypes.data)
        if rc < 0:
            _check(int(rc))
        return cd, fd

    def interface_dofs(self, which):
        p = C.c_void_p()
        cnt = lib().mfgpu_mesh_interface_dofs(self._h, which, C.byref(p))
        return _view(p.value, cnt, np.uint32).copy()


def make_desc(dim, degree, n_dofs, loc2glob, JxW, inv_jac, coefficient, constrained,
              shape_values, shape_gradients, number_type=F64, constraint_mask=None,
              constraint_weights=None, quadrature_points=None, max_cells_per_batch=0, max_dofs_per_batch=0,
              colored=False, kernel=0, cell_loop_segments=0, max_workgroups=0, mass_coefficient=None):
    """Build a Desc from numpy arrays; returns (desc, keepalive list).  mass_coefficient: values of c at the quadrature
    points [n_cells * (p+1)^dim] for the mass term int c u v, or None (the Laplace operator)."""
    dt = np_dtype(number_type)
    keep = []

    def ptr(a, dtype):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    d = Desc()
    d.dim, d.degree, d.number_type = dim, degree, number_type
    l2g = np.ascontiguousarray(loc2glob, dtype=np.uint32)
    d.n_dofs = int(n_dofs)
    d.n_cells = l2g.size // ((degree + 1) ** dim)
    # one scalar J^-1 per cell (reference MATRIX_FREE_UNIFORM_MESH), or J^-1[dim][dim] per quadrature point
    uniform = np.asarray(inv_jac).size == d.n_cells
    assert uniform or np.asarray(inv_jac).size == l2g.size * dim * dim
    d.flags = ((UNIFORM_J0 if uniform else 0) | (HANGING_NODES if constraint_mask is not None else 0)
               | (COLORED_SCATTER if colored else 0))
    d.loc2glob = ptr(l2g, np.uint32)
    d.constraint_mask = ptr(constraint_mask, np.uint32)
    d.JxW = ptr(JxW, dt)
    d.inv_jac = ptr(inv_jac, dt)
    d.coefficient = ptr(coefficient, dt)
    d.quadrature_points = ptr(quadrature_points, dt)
    d.shape_values = ptr(shape_values, dt)
    d.shape_gradients = ptr(shape_gradients, dt)
    d.constraint_weights = ptr(constraint_weights, np.float64)
    c = np.ascontiguousarray(constrained, dtype=np.uint32)
    d.constrained_dofs = ptr(c, np.uint32)
    d.n_constrained = c.size
    d.max_cells_per_batch = max_cells_per_batch
    d.max_dofs_per_batch = max_dofs_per_batch
    d.kernel = kernel
    d.cell_loop_segments = cell_loop_segments
    d.max_workgroups = max_workgroups
    d.mass_coefficient = ptr(mass_coefficient, dt)
    return d, keep


class Plan:
    """Host-only plan (no GPU): mfgpu_plan_*"""

    def __init__(self, desc: Desc, keep=None):
        self._keep = keep
        self.nd = (desc.degree + 1) ** desc.dim
        h = C.c_void_p()
        _check(lib().mfgpu_plan_create(C.byref(desc), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_plan_destroy(self._h)
            self._h = None

    def _u32(self, what):
        p = C.c_void_p()
        cnt = lib().mfgpu_plan_array_u32(self._h, what, C.byref(p))
        if cnt < 0:
            _check(int(cnt))
        return _view(p.value, cnt, np.uint32).copy()

    batch_cell_off = property(lambda s: s._u32(0))
    batch_dof_off = property(lambda s: s._u32(1))
    color_batch_off = property(lambda s: s._u32(2))
    cell_order = property(lambda s: s._u32(3))
    bdofs = property(lambda s: s._u32(4) & np.uint32(0x7fffffff))       # global ids
    bdofs_constrained = property(lambda s: (s._u32(4) >> np.uint32(31)).astype(bool))
    orphans = property(lambda s: s._u32(5))
    batch_nint = property(lambda s: s._u32(6))
    halo_off = property(lambda s: s._u32(7))
    sdofs = property(lambda s: s._u32(8))
    s_off = property(lambda s: s._u32(9))
    s_idx = property(lambda s: s._u32(10))
    chunks = property(lambda s: s._u32(11).reshape(-1, 4))   # {sdofs position, count | k << 16, gstarts offset, offset in group}
    gstarts = property(lambda s: s._u32(12))
    # plane plans (apply_planes3): fixed-size per-batch records
    pr_dofs = property(lambda s: s._u32(13))   # dof lists, bit 31 = constrained
    pr_idx = property(lambda s: s._u32(14))    # index runs
    pr_hn = property(lambda s: s._u32(15))     # hanging-node records of the batches of masked cells
    pr_hn_slot = property(lambda s: s._u32(16))  # per plane batch: index of its record in pr_hn, or 0xffffffff
    # shared form of pr_dofs / pr_idx: every distinct record once + per plane batch {dof base, dof record, index record, 0}
    sh_dofs = property(lambda s: s._u32(17))   # entries relative to the batch's smallest dof id, bit 31 kept
    sh_idx = property(lambda s: s._u32(18))
    sh_batch = property(lambda s: s._u32(19).reshape(-1, 4))
    shares_records = property(lambda s: bool(lib().mfgpu_plan_shares_records(s._h) & 1))  # the form a handle would read
    # shared form of pass 2: records of the owner batches (layout: mfgpu_internal.h) + per batch {dof base, record offset}
    sh_p2rec = property(lambda s: s._u32(20))
    sh_p2tab = property(lambda s: s._u32(21).reshape(-1, 2))
    shares_pass2_records = property(lambda s: bool(lib().mfgpu_plan_shares_records(s._h) & 2))

    @property
    def lmap(self):
        p = C.c_void_p()
        cnt = lib().mfgpu_plan_lmap(self._h, C.byref(p))
        return _view(p.value, cnt, np.uint16).reshape(-1, self.nd).copy()

    @property
    def bflags(self):
        p = C.c_void_p()
        cnt = lib().mfgpu_plan_bflags(self._h, C.byref(p))
        return _view(p.value, cnt, np.uint8).copy()


class DeviceVector:
    """GpuVector<Number> pieces on the path (gpu_vec.h): owning device buffer."""

    def __init__(self, n, number_type=F64):
        self.n, self.number_type = int(n), number_type
        p = C.c_void_p()
        _check(lib().mfgpu_vec_alloc(C.byref(p), self.n, number_type))
        self.ptr = p.value

    @classmethod
    def view(cls, ptr, n, number_type=F64):
        """n elements at a device address somebody else owns (the vectors a CG callback is handed): never freed here"""
        v = cls.__new__(cls)
        v.n, v.number_type, v.ptr, v._borrowed = int(n), number_type, int(ptr), True
        return v

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None and not getattr(self, "_borrowed", False):
            _lib.mfgpu_vec_free(self.ptr)
            self.ptr = None

    def fill(self, value, stream=None):
        _check(lib().mfgpu_vec_fill(self.ptr, self.n, self.number_type, float(value), stream))

    def from_host(self, a):
        a = np.ascontiguousarray(a, dtype=np_dtype(self.number_type))
        assert a.size == self.n
        _check(lib().mfgpu_vec_from_host(self.ptr, a.ctypes.data, self.n, self.number_type))

    def to_host(self):
        a = np.empty(self.n, dtype=np_dtype(self.number_type))
        _check(lib().mfgpu_vec_to_host(a.ctypes.data, self.ptr, self.n, self.number_type))
        return a

    def swap(self, other):
        self.ptr, other.ptr = other.ptr, self.ptr
        self.n, other.n = other.n, self.n

    # ---- GpuVector BLAS-1 and reductions (gpu_vec.h:105-157), SURVEY.md 8(f) N2
    def _a(self, other=None):
        if other is not None:
            assert other.n == self.n and other.number_type == self.number_type
        return self.n, self.number_type

    def sadd(self, s, a, w, stream=None):      # this = s*this + a*w
        _check(lib().mfgpu_vec_sadd(self.ptr, float(s), float(a), w.ptr, *self._a(w), stream))

    def add(self, a, w, stream=None):          # this += a*w
        self.sadd(1.0, a, w, stream)

    def equ(self, a, w, stream=None):          # this = a*w
        _check(lib().mfgpu_vec_equ(self.ptr, float(a), w.ptr, *self._a(w), stream))

    def scale(self, w, stream=None):           # this[i] *= w[i]
        _check(lib().mfgpu_vec_scale(self.ptr, w.ptr, *self._a(w), stream))

    def divide(self, w, stream=None):          # operator/=
        _check(lib().mfgpu_vec_divide(self.ptr, w.ptr, *self._a(w), stream))

    def invert(self, stream=None):
        _check(lib().mfgpu_vec_invert(self.ptr, *self._a(), stream))

    def mul(self, a, stream=None):             # operator*=
        _check(lib().mfgpu_vec_mul(self.ptr, float(a), *self._a(), stream))

    def dot(self, w, stream=None):             # operator*
        r = C.c_double()
        _check(lib().mfgpu_vec_dot(self.ptr, w.ptr, *self._a(w), stream, C.byref(r)))
        return r.value

    def l2_norm(self, stream=None):
        r = C.c_double()
        _check(lib().mfgpu_vec_l2_norm(self.ptr, *self._a(), stream, C.byref(r)))
        return r.value

    def add_and_dot(self, a, x, w, stream=None):  # this += a*x; return this . w
        r = C.c_double()
        self._a(x)
        _check(lib().mfgpu_vec_add_and_dot(self.ptr, float(a), x.ptr, w.ptr, *self._a(w), stream, C.byref(r)))
        return r.value

    def all_zero(self, stream=None):
        r = C.c_int()
        _check(lib().mfgpu_vec_all_zero(self.ptr, *self._a(), stream, C.byref(r)))
        return bool(r.value)


class Operator:
    """LaplaceOperatorGpu surface over the C-ABI handle."""

    def __init__(self, desc: Desc, keep=None):
        self._keep = keep
        self.number_type = desc.number_type
        h = C.c_void_p()
        _check(lib().mfgpu_create(C.byref(desc), C.byref(h)))
        self._h = h

    def __del__(self):
        self.clear()

    def clear(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_destroy(self._h)
            self._h = None

    def n(self):
        return int(lib().mfgpu_n_dofs(self._h))

    m = n

    def vmult(self, dst, src, stream=None):
        _check(lib().mfgpu_vmult(self._h, _ptr(dst), _ptr(src), stream))

    def vmult_add(self, dst, src, stream=None):
        _check(lib().mfgpu_vmult_add(self._h, _ptr(dst), _ptr(src), stream))

    def vmult_multi(self, dst, src, n_vectors, stride=None, add=False, mode=None, stream=None):
        """mfgpu_vmult_multi: dst_k = A src_k (add: +=) for k < n_vectors; vector k starts at element k * stride of dst and
        src (default stride: n_dofs).  mode: None (the library's choice), MULTI_LOOP or MULTI_FUSED."""
        flags = (MULTI_ADD if add else 0) | (mode or 0)
        _check(lib().mfgpu_vmult_multi(self._h, _ptr(dst), _ptr(src), int(n_vectors),
                                       self.n() if stride is None else int(stride), flags, stream))

    def multi_width(self):
        """widest group of vectors one fused sweep serves (1: vmult_multi applies the vectors one by one)"""
        return int(lib().mfgpu_multi_width(self._h))

    def memory_consumption(self):
        return int(lib().mfgpu_memory_consumption(self._h))

    def plan_stats(self):
        s = (C.c_uint64 * 8)()
        _check(lib().mfgpu_plan_stats(self._h, s))
        keys = ["n_batches", "n_launches", "batch_dofs", "max_batch_dofs", "max_batch_cells", "n_orphans",
                "first_touch_or_shared_dofs", "rmw_adds_or_halo_slots"]
        out = dict(zip(keys, [int(v) for v in s]))
        r = (C.c_uint64 * 4)()
        _check(lib().mfgpu_record_stats(self._h, r))
        out.update(index_records="shared" if r[0] & 1 else "expanded",
                   pass2_records="shared" if r[0] & 2 else "expanded", distinct_dof_records=int(r[1]),
                   distinct_index_records=int(r[2]), index_record_bytes=int(r[3]))
        return out

    def kernel_name(self):
        return lib().mfgpu_kernel_name(self._h).decode()

    def compute_inverse_diagonal(self, inv_diag, stream=None):
        """LaplaceOperatorGpu::compute_diagonal + get_diagonal_inverse (laplace_operator_gpu.h:401-429)"""
        _check(lib().mfgpu_compute_inverse_diagonal(self._h, _ptr(inv_diag), stream))

    def set_constrained_values(self, vec, value, stream=None):
        """ConstraintHandlerGpu::set_constrained_values (constraint_handler_gpu.cu:126-137)"""
        _check(lib().mfgpu_set_constrained_values(self._h, _ptr(vec), float(value), stream))

    def update_coefficients(self, coef=None, mass=None, stream=None):
        """mfgpu_update_coefficients: new a and / or c from DEVICE arrays [n_cells * (p+1)^dim] (None: unchanged); the
        operator must have been created with UPDATABLE_COEFFICIENTS"""
        _check(lib().mfgpu_update_coefficients(self._h, _optr(coef), _optr(mass), stream))

    def profile_enable(self, on=True):
        _check(lib().mfgpu_profile_enable(self._h, int(on)))

    def profile_read(self):
        ms, nv = C.c_double(), C.c_uint64()
        _check(lib().mfgpu_profile_read(self._h, C.byref(ms), C.byref(nv)))
        return ms.value, int(nv.value)

    def profile_read_pass2(self):
        ms = C.c_double()
        _check(lib().mfgpu_profile_read_pass2(self._h, C.byref(ms)))
        return ms.value


def cg_chebyshev_scalars(degree, lambda_max, smoothing_range):
    """the 2 * degree - 1 scalars of the Chebyshev sweep (mfgpu_cg_chebyshev_scalars): f[0] = 1 / theta, then (f1, f2) per
    inner step; host only"""
    out = (C.c_double * max(2 * int(degree) - 1, 1))()
    _check(lib().mfgpu_cg_chebyshev_scalars(int(degree), float(lambda_max), float(smoothing_range), out))
    return np.array(out[:2 * int(degree) - 1], dtype=np.float64)


class CG:
    """Device-resident conjugate gradients on an Operator (mfgpu_cg_*): begin and iterate only enqueue work, status is the
    only blocking call.  preconditioner: CG_NONE, CG_JACOBI (inv_diag), CG_CHEBYSHEV (inv_diag, degree, lambda_max,
    smoothing_range) or CG_CALLBACK with callback(z, r, stream) -> 0 / None or an error code, where z and r are
    DeviceVector views of the solver's vectors and the callback enqueues z = M^-1 r on `stream`.  The operator, inv_diag, x
    and b must outlive the solve.  The methods return the raw code with check=False."""

    def __init__(self, op: "Operator", preconditioner=CG_NONE, inv_diag=None, degree=0, lambda_max=0.0,
                 smoothing_range=0.0, callback=None):
        self._op, self._inv_diag = op, inv_diag
        self._cb = self._cb_error = None
        self.n, self.number_type = op.n(), op.number_type
        h = C.c_void_p()
        _check(lib().mfgpu_cg_create(op._h, int(preconditioner), _optr(inv_diag), int(degree), float(lambda_max),
                                     float(smoothing_range), C.byref(h)))
        self._h = h
        if callback is not None:
            self.set_callback(callback)

    def set_callback(self, callback):
        def trampoline(_ctx, z, r, stream):
            try:
                rc = callback(DeviceVector.view(z, self.n, self.number_type),
                              DeviceVector.view(r, self.n, self.number_type), stream)
                return 0 if rc is None else int(rc)
            except Exception as e:  # no exception crosses the C-ABI: kept for _done
                self._cb_error = e
                return EINVAL

        cb = CG_CALLBACK_TYPE(trampoline)
        _check(lib().mfgpu_cg_set_callback(self._h, cb, None))
        self._cb = cb  # the library keeps the function pointer: keep the ctypes object alive

    def _done(self, rc, check):
        e, self._cb_error = self._cb_error, None
        if e is not None:
            raise e
        return _check(rc) if check else rc

    def destroy(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_cg_destroy(self._h)
            self._h = None

    __del__ = destroy

    def begin(self, x, b, tolerance, max_iterations, stream=None, check=True):
        return self._done(lib().mfgpu_cg_begin(self._h, _optr(x), _optr(b), float(tolerance), int(max_iterations), stream),
                          check)

    def begin_relative(self, x, b, relative_tolerance, max_iterations, stream=None, check=True):
        """begin with tolerance = relative_tolerance * |b|, formed on the device (mfgpu_cg_begin_relative)"""
        return self._done(lib().mfgpu_cg_begin_relative(self._h, _optr(x), _optr(b), float(relative_tolerance),
                                                        int(max_iterations), stream), check)

    def set_vcycle(self, vcycle: "VCycle", check=True):
        """the library's own callback of a CG_CALLBACK solver: z = vcycle.apply(r) without a trip through Python"""
        rc = lib().mfgpu_cg_set_vcycle(self._h, vcycle._h)
        if rc == 0:
            self._vcycle = vcycle  # borrowed by the library
        return _check(rc) if check else rc

    def iterate(self, n_iterations=1, stream=None, check=True):
        return self._done(lib().mfgpu_cg_iterate(self._h, int(n_iterations), stream), check)

    def status(self, stream=None):
        info = CGInfo()
        _check(lib().mfgpu_cg_status(self._h, stream, C.byref(info)))
        return info

    def solve(self, x, b, tolerance, max_iterations, check_every=10, stream=None):
        info = CGInfo()
        self._done(lib().mfgpu_cg_solve(self._h, _optr(x), _optr(b), float(tolerance), int(max_iterations),
                                        int(check_every), stream, C.byref(info)), True)
        return info

    def memory_consumption(self):
        return int(lib().mfgpu_cg_memory_consumption(self._h))


class Integrator:
    """Cell integrals of a Poisson solve (mfgpu_integrator_*): the load vector with the Dirichlet lift
    (poisson.cu:182-221) and the L2 error on QGauss(p+2) (VectorTools::integrate_difference, poisson.cu:277-292).
    Double only.  Vectors: DeviceVector or anything _ptr accepts; None = the built-in function / no lift."""

    def __init__(self, desc: Desc, keep=None):
        self._keep = keep
        self.dim, self.degree, self.n_cells = int(desc.dim), int(desc.degree), int(desc.n_cells)
        self.n_dofs = int(desc.n_dofs)
        h = C.c_void_p()
        _check(lib().mfgpu_integrator_create(C.byref(desc), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_integrator_destroy(self._h)
            self._h = None

    @property
    def n_error_points(self):
        """(p+2)^dim points per cell"""
        return (self.degree + 2) ** self.dim

    def rhs(self, dst, f=None, u_b=None, stream=None):
        """dst = int phi_i f - int grad phi_i . a grad u_b (- int c phi_i u_b with a mass term in the description);
        f: values at the quadrature points [n_cells * (p+1)^dim]"""
        _check(lib().mfgpu_integrator_rhs(self._h, _ptr(dst), None if f is None else _ptr(f),
                                          None if u_b is None else _ptr(u_b), stream))

    def l2_error(self, u, exact=None, per_cell=None, stream=None):
        """|u - exact|_L2; exact: values at the error points [n_cells * (p+2)^dim]; per_cell: squared cell errors"""
        r = C.c_double()
        _check(lib().mfgpu_integrator_l2_error(self._h, _ptr(u), None if exact is None else _ptr(exact),
                                               None if per_cell is None else _ptr(per_cell), stream, C.byref(r)))
        return r.value

    def update_coefficients(self, coef=None, mass=None, stream=None):
        """mfgpu_integrator_update_coefficients: a and c of the lift from device arrays (UPDATABLE_COEFFICIENTS)"""
        _check(lib().mfgpu_integrator_update_coefficients(self._h, _optr(coef), _optr(mass), stream))

    def evaluate(self, u, values=None, gradients=None, stream=None):
        """u at the quadrature points into `values` [n_cells * (p+1)^dim] and / or its real-space gradient into
        `gradients` [n_cells * (p+1)^dim * dim] (device arrays; gradients need UPDATABLE_COEFFICIENTS)"""
        _check(lib().mfgpu_integrator_evaluate(self._h, _ptr(u), _optr(values), _optr(gradients), stream))

    def recovery_indicator(self, u, per_cell=None, weight=None, stream=None):
        """eta_K^2 [n_cells] of the gradient-recovery indicator (mfgpu_integrator_recovery_indicator) into the device
        array `per_cell` (default: a new DeviceVector, which is returned); weight: [n_cells * (p+1)^dim] at the
        quadrature points or None for 1.  Needs UPDATABLE_COEFFICIENTS.  Asynchronous."""
        if per_cell is None:
            per_cell = DeviceVector(self.n_cells)
        _check(lib().mfgpu_integrator_recovery_indicator(self._h, _ptr(u), _optr(weight), _ptr(per_cell), stream))
        return per_cell

    def error_points(self):
        """the error points of every cell on the host, [n_cells, (p+2)^dim, dim]"""
        v = DeviceVector(self.n_cells * self.n_error_points * self.dim)
        _check(lib().mfgpu_integrator_error_points(self._h, v.ptr, None))
        return v.to_host().reshape(self.n_cells, self.n_error_points, self.dim)

    def integrate(self, dst, values=None, gradients=None, stream=None):
        """the transpose of evaluate: dst_i = sum_q JxW_q (phi_i v_q + grad phi_i . g_q), constrained rows 0; values
        [n_cells * (p+1)^dim], gradients [n_cells * (p+1)^dim * dim] real-space (need UPDATABLE_COEFFICIENTS)"""
        _check(lib().mfgpu_integrator_integrate(self._h, _ptr(dst), _optr(values), _optr(gradients), stream))


class QpOperator:
    """mfgpu_qop_*: (A u)_i = sum_q JxW_q [grad phi_i . (D grad u + gamma u) + phi_i (beta . grad u + c u)] with the
    coefficients given at the quadrature points (device arrays in the layout of Integrator.evaluate).  terms: QOP_* bits.
    Borrows the integrator, which it keeps alive."""

    def __init__(self, integrator: "Integrator", terms):
        self._it = integrator
        h = C.c_void_p()
        _check(lib().mfgpu_qop_create(integrator._h, int(terms), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_qop_destroy(self._h)
            self._h = None

    def set_coefficients(self, diffusion=None, convection=None, flux=None, reaction=None, stream=None):
        """folds the given real-space arrays; None keeps a term's last values"""
        c = QopCoefficients(_optr(diffusion), _optr(convection), _optr(flux), _optr(reaction))
        _check(lib().mfgpu_qop_set_coefficients(self._h, C.byref(c), stream))

    def vmult(self, dst, src, transpose=False, stream=None):
        _check(lib().mfgpu_qop_vmult(self._h, _ptr(dst), _ptr(src), QOP_TRANSPOSE if transpose else 0, stream))

    def inverse_diagonal(self, inv_diag, stream=None):
        _check(lib().mfgpu_qop_compute_inverse_diagonal(self._h, _ptr(inv_diag), stream))

    def memory_consumption(self):
        return int(lib().mfgpu_qop_memory_consumption(self._h))

    def n(self):
        return self._it.n_dofs

    m = n


class VectorQpOperator:
    """mfgpu_vqop_*: the elasticity operator on fields of dim components in blocks (u[a * n_dofs + i]),
    (A u)_(a,i) = sum_q JxW_q [sum_k d_k phi_i sigma_ak + phi_i rho u_a] with sigma = lam (div u) I + mu (grad u + grad u^T)
    (VQOP_ISOTROPIC) or sigma_ak = sum_bl C[a][k][b][l] d_l u_b (VQOP_TENSOR4), and VQOP_MASS for the rho term.
    constrained: ascending block indices in [0, dim * n_dofs) (None: the description's list in every component; a list
    of one's own must hold every dof of the description's list, the hanging dofs among them, in every component).
    Borrows the integrator, which it keeps alive."""

    def __init__(self, integrator: "Integrator", terms, constrained=None):
        self._it = integrator
        h = C.c_void_p()
        if constrained is None:
            ptr, cnt = None, 0
        else:
            c = np.asarray(constrained)
            if c.size and (c.min() < 0 or c.max() > 0xffffffff):
                raise MfgpuError("mfgpu error -1 (MFGPU_EINVAL): constrained index out of range")
            c = np.ascontiguousarray(c, dtype=np.uint32).reshape(-1)
            ptr, cnt = c.ctypes.data if c.size else np.zeros(1, np.uint32).ctypes.data, c.size
        _check(lib().mfgpu_vqop_create(integrator._h, int(terms), ptr, cnt, C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_vqop_destroy(self._h)
            self._h = None

    def set_coefficients(self, lam=None, mu=None, tensor=None, mass=None, stream=None):
        """folds the given real-space arrays; None keeps a term's last values; lam and mu go together"""
        c = VqopCoefficients(_optr(lam), _optr(mu), _optr(tensor), _optr(mass))
        _check(lib().mfgpu_vqop_set_coefficients(self._h, C.byref(c), stream))

    def vmult(self, dst, src, stream=None):
        _check(lib().mfgpu_vqop_vmult(self._h, _ptr(dst), _ptr(src), stream))

    def inverse_diagonal(self, inv_diag, stream=None):
        _check(lib().mfgpu_vqop_compute_inverse_diagonal(self._h, _ptr(inv_diag), stream))

    def set_constrained_values(self, vec, value, stream=None):
        _check(lib().mfgpu_vqop_set_constrained_values(self._h, _ptr(vec), float(value), stream))

    def memory_consumption(self):
        return int(lib().mfgpu_vqop_memory_consumption(self._h))

    def n(self):
        return self._it.dim * self._it.n_dofs

    m = n


class BiCGStab:
    """Device-resident BiCGStab (mfgpu_bicgstab_*) for the non-symmetric operators, in the shape of CG: begin and iterate
    only enqueue work, status is the only blocking call.  operator: an Operator, a QpOperator (transpose=True solves with
    A^T), a VectorQpOperator or a callable apply(dst, src, stream) -> 0 / None or an error code that enqueues dst = A src on `stream`, with
    dst and src DeviceVector views of the solver's vectors; a callable needs n (and number_type).  preconditioner:
    CG_NONE, CG_JACOBI (inv_diag) or CG_CALLBACK with callback(z, r, stream) as for CG, or set_vcycle.  The operator,
    inv_diag, x and b must outlive the solve.  The methods return the raw code with check=False."""

    def __init__(self, operator, preconditioner=CG_NONE, inv_diag=None, callback=None, transpose=False, n=None,
                 number_type=None):
        self._op, self._inv_diag = operator, inv_diag
        self._cb = self._apply = self._cb_error = None
        if isinstance(operator, (Operator, QpOperator, VectorQpOperator)):
            self.n = operator.n()
            self.number_type = operator.number_type if isinstance(operator, Operator) else F64
        elif callable(operator):
            if n is None:
                raise ValueError("BiCGStab on a callable needs n")
            self.n, self.number_type = int(n), F64 if number_type is None else number_type
        else:
            raise TypeError("BiCGStab: operator must be an Operator, a QpOperator or a callable")
        h = C.c_void_p()
        _check(lib().mfgpu_bicgstab_create(self.n, int(self.number_type), int(preconditioner), _optr(inv_diag), C.byref(h)))
        self._h = h
        if isinstance(operator, Operator):
            _check(lib().mfgpu_bicgstab_set_operator_handle(h, operator._h))
        elif isinstance(operator, QpOperator):
            _check(lib().mfgpu_bicgstab_set_operator_qop(h, operator._h, QOP_TRANSPOSE if transpose else 0))
        elif isinstance(operator, VectorQpOperator):
            _check(lib().mfgpu_bicgstab_set_operator_vqop(h, operator._h))
        else:
            self._apply = CG_CALLBACK_TYPE(self._trampoline(operator))
            _check(lib().mfgpu_bicgstab_set_operator(h, self._apply, None))
        if callback is not None:
            self.set_callback(callback)

    def _trampoline(self, f):
        def trampoline(_ctx, dst, src, stream):
            try:
                rc = f(DeviceVector.view(dst, self.n, self.number_type), DeviceVector.view(src, self.n, self.number_type),
                       stream)
                return 0 if rc is None else int(rc)
            except Exception as e:  # no exception crosses the C-ABI: kept for _done
                self._cb_error = e
                return EINVAL

        return trampoline

    def set_callback(self, callback):
        cb = CG_CALLBACK_TYPE(self._trampoline(callback))
        _check(lib().mfgpu_bicgstab_set_callback(self._h, cb, None))
        self._cb = cb  # the library keeps the function pointer: keep the ctypes object alive

    def set_vcycle(self, vcycle: "VCycle", check=True):
        """the library's own callback of a CG_CALLBACK solver: z = vcycle.apply(r) without a trip through Python"""
        rc = lib().mfgpu_bicgstab_set_vcycle(self._h, vcycle._h)
        if rc == 0:
            self._vcycle = vcycle  # borrowed by the library
        return _check(rc) if check else rc

    def _done(self, rc, check):
        e, self._cb_error = self._cb_error, None
        if e is not None:
            raise e
        return _check(rc) if check else rc

    def destroy(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_bicgstab_destroy(self._h)
            self._h = None

    __del__ = destroy

    def begin(self, x, b, tolerance, max_iterations, stream=None, check=True):
        return self._done(lib().mfgpu_bicgstab_begin(self._h, _optr(x), _optr(b), float(tolerance), int(max_iterations),
                                                     stream), check)

    def begin_relative(self, x, b, relative_tolerance, max_iterations, stream=None, check=True):
        """begin with tolerance = relative_tolerance * |b|, formed on the device (mfgpu_bicgstab_begin_relative)"""
        return self._done(lib().mfgpu_bicgstab_begin_relative(self._h, _optr(x), _optr(b), float(relative_tolerance),
                                                              int(max_iterations), stream), check)

    def iterate(self, n_iterations=1, stream=None, check=True):
        return self._done(lib().mfgpu_bicgstab_iterate(self._h, int(n_iterations), stream), check)

    def status(self, stream=None):
        info = CGInfo()
        _check(lib().mfgpu_bicgstab_status(self._h, stream, C.byref(info)))
        return info

    def solve(self, x, b, tolerance, max_iterations, check_every=10, stream=None, check=True):
        info = CGInfo()
        rc = self._done(lib().mfgpu_bicgstab_solve(self._h, _optr(x), _optr(b), float(tolerance), int(max_iterations),
                                                   int(check_every), stream, C.byref(info)), check)
        return info if check else rc

    def memory_consumption(self):
        return int(lib().mfgpu_bicgstab_memory_consumption(self._h))


POINT_NOT_FOUND = 0xffffffff  # MFGPU_POINT_NOT_FOUND


def locate_points(desc: Desc, x):
    """mfgpu_locate_points (host): (cell [n] uint32, xi [n, dim], n_not_found) of the points x [n, dim]; a point no cell
    holds has cell POINT_NOT_FOUND and xi 0"""
    dim = int(desc.dim)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, dim)
    cell, xi, missing = np.empty(len(x), np.uint32), np.empty((len(x), dim), np.float64), C.c_uint32()
    _check(lib().mfgpu_locate_points(C.byref(desc), x.ctypes.data, len(x), cell.ctypes.data, xi.ctypes.data,
                                     C.byref(missing)))
    return cell, xi, int(missing.value)


class Points:
    """A set of points in the cells of an integrator's mesh (mfgpu_points_*): the field and its gradient at them
    (evaluate) and the transpose of the value part, point sources (integrate).  Double only.  The integrator is kept
    alive by the object."""

    def __init__(self, integrator: "Integrator", desc: Desc = None, x=None, _in_cells=None, _located=None):
        self._it = integrator
        self.dim = integrator.dim
        h = C.c_void_p()
        if _located is not None:
            cell, xi, self.n, stream = _located
            _check(lib().mfgpu_points_create_located(integrator._h, _optr(cell), _optr(xi), self.n, stream, C.byref(h)))
        elif _in_cells is None:
            x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.dim)
            self.n = len(x)
            _check(lib().mfgpu_points_create(integrator._h, C.byref(desc), x.ctypes.data, self.n, C.byref(h)))
        else:
            cell, xi = _in_cells
            self.n = len(cell)
            _check(lib().mfgpu_points_create_in_cells(integrator._h, cell.ctypes.data, xi.ctypes.data, self.n, C.byref(h)))
        self._h = h

    @classmethod
    def in_cells(cls, integrator: "Integrator", cell, xi):
        """points given as (cell [n], xi [n, dim] in [0, 1]); POINT_NOT_FOUND is allowed as a cell"""
        cell = np.ascontiguousarray(cell, dtype=np.uint32).reshape(-1)
        xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(-1, integrator.dim)
        if len(xi) != len(cell):
            raise ValueError("cell and xi disagree on the number of points")
        return cls(integrator, _in_cells=(cell, xi))

    @classmethod
    def located(cls, integrator: "Integrator", cell, xi, n, stream=None):
        """points given as device buffers (cell [n] uint32, xi [n * dim]) as Locator.locate leaves them
        (mfgpu_points_create_located): synchronises `stream`, downloads both and builds the object of in_cells"""
        return cls(integrator, _located=(cell, xi, int(n), stream))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_points_destroy(self._h)
            self._h = None

    @property
    def cells(self):
        """the cell of every point, in the caller's order (a copy)"""
        p = C.c_void_p()
        n = lib().mfgpu_points_cells(self._h, C.byref(p))
        return _view(p.value, n, np.uint32).copy()

    @property
    def n_not_found(self):
        return int(lib().mfgpu_points_n_not_found(self._h))

    def evaluate(self, u, values=None, gradients=None, stream=None):
        """u_h at the points into `values` [n] and / or its real-space gradient into `gradients` [n * dim] (device
        arrays, caller's point order); points without a cell get 0"""
        _check(lib().mfgpu_points_evaluate(self._h, _ptr(u), _optr(values), _optr(gradients), stream))

    def integrate(self, rhs, weights=None, stream=None):
        """rhs [n_dofs] = sum_k weights_k phi_i(x_k) (weights None: all 1), distributed like a cell result"""
        _check(lib().mfgpu_points_integrate(self._h, _ptr(rhs), _optr(weights), stream))

    def memory_consumption(self):
        return int(lib().mfgpu_points_memory_consumption(self._h))


class Locator:
    """Point location on the device (mfgpu_locator_*): mfgpu_locate_points for points that move.  Created from an
    integrator and the description it was created from; the integrator is kept alive by the object.  Double only.

    The `cell`, `hint` and `n_not_found` buffers are 4-byte device memory holding uint32: allocate them as
    DeviceVector(n, F32) and read them back with `.to_host().view(np.uint32)` (cells_to_host does that); a torch int32
    tensor on the GPU is accepted as well."""

    def __init__(self, integrator: "Integrator", desc: Desc):
        self._it = integrator
        self.dim = integrator.dim
        h = C.c_void_p()
        _check(lib().mfgpu_locator_create(integrator._h, C.byref(desc), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_locator_destroy(self._h)
            self._h = None

    def locate(self, x, cell, xi, hint=None, n_not_found=None, stream=None, n=None):
        """the cell [n] (POINT_NOT_FOUND: none) and xi [n * dim] of the points x [n * dim], all device buffers; hint [n]
        (may be `cell` itself) names a cell to try first; n_not_found: one uint32, overwritten.  n defaults to the
        length of `cell`.  Asynchronous."""
        if n is None:
            n = cell.n if isinstance(cell, DeviceVector) else cell.numel()
        _check(lib().mfgpu_locator_locate(self._h, _optr(x), int(n), _optr(hint), _optr(cell), _optr(xi),
                                          _optr(n_not_found), stream))

    @staticmethod
    def cells_to_host(cell):
        """a DeviceVector(n, F32) that holds cells, on the host as uint32"""
        return cell.to_host().view(np.uint32)

    def memory_consumption(self):
        return int(lib().mfgpu_locator_memory_consumption(self._h))


class MgHierarchy:
    """Level hierarchy of an adaptive stand-in mesh (mfgpu_mg_*): level meshes, refinement-edge dofs, transfer arrays,
    copy_to_mg pairs.  Host only."""

    def __init__(self, mesh: "Mesh"):
        h = C.c_void_p()
        _check(lib().mfgpu_mg_hierarchy_create(mesh._h, C.byref(h)))
        self._h = h
        self.n_levels = int(lib().mfgpu_mg_n_levels(h))

    def level_mesh(self, level):
        m = Mesh.__new__(Mesh)
        m._owner = self  # borrowed: the level meshes belong to the hierarchy (Mesh.__del__ leaves them alone)
        m._h = C.c_void_p(lib().mfgpu_mg_level_mesh(self._h, level))
        m.desc = Desc()
        _check(lib().mfgpu_mesh_desc(m._h, C.byref(m.desc)))
        return m

    def edge_dofs(self, level):
        p = C.c_void_p()
        n = lib().mfgpu_mg_edge_dofs(self._h, level, C.byref(p))
        return _view(p.value, n, np.uint32).copy()

    def copy_pairs(self, level):
        a, b = C.c_void_p(), C.c_void_p()
        n = lib().mfgpu_mg_copy_pairs(self._h, level, C.byref(a), C.byref(b))
        return _view(a.value, n, np.uint32).copy(), _view(b.value, n, np.uint32).copy()

    def transfer_arrays(self, level, nd, nfd):
        a, b = C.c_void_p(), C.c_void_p()
        n = lib().mfgpu_mg_transfer_arrays(self._h, level, C.byref(a), C.byref(b))
        return _view(a.value, n * nd, np.uint32).reshape(n, nd).copy(), _view(b.value, n * nfd, np.uint32).reshape(n, nfd).copy()

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_mg_hierarchy_destroy(self._h)
            self._h = None


class Level:
    """Level operator with refinement edges + the interface matrices (mfgpu_level_*)."""

    def __init__(self, desc: Desc, edge_dofs, keep=None):
        self._keep = keep
        e = np.ascontiguousarray(edge_dofs, dtype=np.uint32)
        h = C.c_void_p()
        _check(lib().mfgpu_level_create(C.byref(desc), e.ctypes.data if e.size else None, e.size, C.byref(h)))
        self._h = h
        self.number_type = desc.number_type

    def vmult(self, dst, src, stream=None):
        _check(lib().mfgpu_vmult(lib().mfgpu_level_operator(self._h), _ptr(dst), _ptr(src), stream))

    def compute_inverse_diagonal(self, inv_diag, stream=None):
        _check(lib().mfgpu_compute_inverse_diagonal(lib().mfgpu_level_operator(self._h), _ptr(inv_diag), stream))

    def update_coefficients(self, coef=None, mass=None, stream=None):
        """mfgpu_level_update_coefficients: the level operator and the interface matrices (UPDATABLE_COEFFICIENTS)"""
        _check(lib().mfgpu_level_update_coefficients(self._h, _optr(coef), _optr(mass), stream))

    def vmult_interface_down(self, dst, src, stream=None):
        _check(lib().mfgpu_level_vmult_interface_down(self._h, _ptr(dst), _ptr(src), stream))

    def vmult_interface_up(self, dst, src, stream=None):
        _check(lib().mfgpu_level_vmult_interface_up(self._h, _ptr(dst), _ptr(src), stream))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_level_destroy(self._h)
            self._h = None


class Transfer:
    """A multigrid transfer (mfgpu_transfer_*) of one of three kinds: between two globally refined levels at one degree
    (from_arrays / from_meshes, MGTransferMatrixFreeGpu), between two degrees on one mesh (p_from_arrays / p_hn_from_arrays
    / p_from_meshes / p_hn_from_meshes: p-multigrid, with or without hanging nodes), and between two leaf meshes with
    hanging nodes at one degree (h_hn_from_arrays / h_hn_from_meshes: global coarsening); the calls are the same for all.
    The last kind made by h_hn_interp_from_arrays / h_hn_interp_from_meshes also interpolates from fine to coarse."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _arg(a, dtype):
        """(contiguous array or None, its address or None): None and an empty array are the library's null pointer"""
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=dtype)
        return a, a.ctypes.data if a.size else None

    @classmethod
    def _create(cls, creator, *args):
        h = C.c_void_p()
        _check(getattr(lib(), creator)(*args, C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, dim, degree, coarse_cell_dofs, fine_patch_dofs, n_coarse_dofs, n_fine_dofs, coarse_dirichlet,
                    number_type=F64, prolongation_1d=None):
        (cd, cdp), (fd, fdp) = cls._arg(coarse_cell_dofs, np.uint32), cls._arg(fine_patch_dofs, np.uint32)
        (di, dip), (_, p1p) = cls._arg(coarse_dirichlet, np.uint32), cls._arg(prolongation_1d, np.float64)
        n_cells = cd.size // ((degree + 1) ** dim)
        assert fd.size == n_cells * (2 * degree + 1) ** dim
        return cls._create("mfgpu_transfer_create", dim, degree, number_type, n_cells, cdp, fdp, n_coarse_dofs, n_fine_dofs,
                           dip, di.size, p1p)

    @classmethod
    def from_meshes(cls, coarse: "Mesh", fine: "Mesh"):
        return cls._create("mfgpu_transfer_create_from_meshes", coarse._h, fine._h)

    @classmethod
    def p_from_arrays(cls, dim, degree_coarse, degree_fine, coarse_cell_dofs, fine_cell_dofs, n_coarse_dofs, n_fine_dofs,
                      coarse_dirichlet, number_type=F64, prolongation_1d=None):
        """the p-multigrid transfer between FE_Q(degree_coarse) and FE_Q(degree_fine) on the same cells
        (mfgpu_transfer_create_p): the two descriptions' loc2glob, same cell order"""
        return cls.p_hn_from_arrays(dim, degree_coarse, degree_fine, coarse_cell_dofs, fine_cell_dofs, n_coarse_dofs,
                                    n_fine_dofs, coarse_dirichlet, number_type, prolongation_1d)

    @classmethod
    def p_from_meshes(cls, coarse: "Mesh", fine: "Mesh"):
        """mfgpu_transfer_create_p_from_meshes: two stand-in meshes of the same cells, the degree rises"""
        return cls._create("mfgpu_transfer_create_p_from_meshes", coarse._h, fine._h)

    @classmethod
    def p_hn_from_arrays(cls, dim, degree_coarse, degree_fine, coarse_cell_dofs, fine_cell_dofs, n_coarse_dofs, n_fine_dofs,
                         coarse_dirichlet, number_type=F64, prolongation_1d=None, constraint_mask=None,
                         coarse_constraint_weights=None):
        """p_from_arrays on cells with hanging nodes (mfgpu_transfer_create_p_hn): constraint_mask [n_cells] is the one of
        both descriptions (None: conforming), coarse_constraint_weights [(degree_coarse + 1)^2] the coarse description's
        constraint_weights (None: those of FE_Q(degree_coarse))"""
        (cd, cdp), (fd, fdp) = cls._arg(coarse_cell_dofs, np.uint32), cls._arg(fine_cell_dofs, np.uint32)
        (di, dip), (p1, p1p) = cls._arg(coarse_dirichlet, np.uint32), cls._arg(prolongation_1d, np.float64)
        (cm, cmp_), (w, wp) = cls._arg(constraint_mask, np.uint32), cls._arg(coarse_constraint_weights, np.float64)
        ncd, nfd = (max(int(degree_coarse), 0) + 1) ** dim, (max(int(degree_fine), 0) + 1) ** dim
        n_cells = cd.size // ncd
        if 1 <= degree_coarse < degree_fine <= 6:  # (any other pair is the library's MFGPU_EINVAL)
            assert cd.size == n_cells * ncd and fd.size == n_cells * nfd
            assert p1 is None or p1.size == (degree_coarse + 1) * (degree_fine + 1)
            assert cm is None or cm.size == n_cells
            assert w is None or w.size == (degree_coarse + 1) ** 2
        return cls._create("mfgpu_transfer_create_p_hn", dim, degree_coarse, degree_fine, number_type, n_cells, cdp, fdp,
                           n_coarse_dofs, n_fine_dofs, dip, di.size, p1p, cmp_, wp)

    @classmethod
    def p_hn_from_meshes(cls, coarse: "Mesh", fine: "Mesh"):
        """mfgpu_transfer_create_p_hn_from_meshes: what p_from_meshes accepts, and adaptive meshes or meshes from leaves
        of equal cells and masks"""
        return cls._create("mfgpu_transfer_create_p_hn_from_meshes", coarse._h, fine._h)

    @classmethod
    def h_hn_from_arrays(cls, dim, degree, coarse_cell_dofs, fine_cell_dofs, parent, child, n_coarse_dofs, n_fine_dofs,
                         coarse_dirichlet, number_type=F64, prolongation_1d=None, coarse_mask=None, fine_mask=None,
                         constraint_weights=None):
        """the global-coarsening h-transfer between two meshes with hanging nodes at one degree
        (mfgpu_transfer_create_h_hn): the two descriptions' loc2glob, per fine cell its coarse cell `parent` and `child`
        (0: the same cell, 1 + k: child k), the two descriptions' constraint masks (None: none)"""
        (cd, cdp), (fd, fdp) = cls._arg(coarse_cell_dofs, np.uint32), cls._arg(fine_cell_dofs, np.uint32)
        (pa, pap), (ch, chp) = cls._arg(parent, np.uint32), cls._arg(child, np.uint32)
        (di, dip), (p1, p1p) = cls._arg(coarse_dirichlet, np.uint32), cls._arg(prolongation_1d, np.float64)
        (cm, cmp_), (fm, fmp) = cls._arg(coarse_mask, np.uint32), cls._arg(fine_mask, np.uint32)
        w, wp = cls._arg(constraint_weights, np.float64)
        nd = (max(int(degree), 0) + 1) ** dim
        n_coarse, n_fine = cd.size // nd, fd.size // nd
        if 1 <= degree <= 6 and dim in (2, 3):  # (anything else is the library's MFGPU_EINVAL)
            assert cd.size == n_coarse * nd and fd.size == n_fine * nd and pa.size == n_fine and ch.size == n_fine
            assert p1 is None or p1.size == (2 * degree + 1) * (degree + 1)
            assert (cm is None or cm.size == n_coarse) and (fm is None or fm.size == n_fine)
            assert w is None or w.size == (degree + 1) ** 2
        return cls._create("mfgpu_transfer_create_h_hn", dim, degree, number_type, n_coarse, n_fine, cdp, fdp, pap, chp,
                           n_coarse_dofs, n_fine_dofs, dip, di.size, p1p, cmp_, fmp, wp)

    @classmethod
    def h_hn_from_meshes(cls, coarse: "Mesh", fine: "Mesh"):
        """mfgpu_transfer_create_h_hn_from_meshes: two leaf meshes of equal degree, the fine one's leaves those of the
        coarse one or their children (a mesh and a member of its Mesh.coarsening_sequence)"""
        return cls._create("mfgpu_transfer_create_h_hn_from_meshes", coarse._h, fine._h)

    @classmethod
    def h_hn_interp_from_arrays(cls, dim, degree, coarse_cell_dofs, fine_cell_dofs, parent, child, n_coarse_dofs,
                                n_fine_dofs, coarse_dirichlet, number_type=F64, prolongation_1d=None, coarse_mask=None,
                                fine_mask=None, constraint_weights=None, interpolation_1d=None):
        """h_hn_from_arrays plus the interpolation image (mfgpu_transfer_create_h_hn_interp): the same object, and
        interpolate works on it; interpolation_1d [(degree + 1)^2] replaces the default J1"""
        (cd, cdp), (fd, fdp) = cls._arg(coarse_cell_dofs, np.uint32), cls._arg(fine_cell_dofs, np.uint32)
        (pa, pap), (ch, chp) = cls._arg(parent, np.uint32), cls._arg(child, np.uint32)
        (di, dip), (p1, p1p) = cls._arg(coarse_dirichlet, np.uint32), cls._arg(prolongation_1d, np.float64)
        (cm, cmp_), (fm, fmp) = cls._arg(coarse_mask, np.uint32), cls._arg(fine_mask, np.uint32)
        (w, wp), (j1, j1p) = cls._arg(constraint_weights, np.float64), cls._arg(interpolation_1d, np.float64)
        nd = (max(int(degree), 0) + 1) ** dim
        n_coarse, n_fine = cd.size // nd, fd.size // nd
        if 1 <= degree <= 6 and dim in (2, 3):  # (anything else is the library's MFGPU_EINVAL)
            assert cd.size == n_coarse * nd and fd.size == n_fine * nd and pa.size == n_fine and ch.size == n_fine
            assert p1 is None or p1.size == (2 * degree + 1) * (degree + 1)
            assert (cm is None or cm.size == n_coarse) and (fm is None or fm.size == n_fine)
            assert w is None or w.size == (degree + 1) ** 2
            assert j1 is None or j1.size == (degree + 1) ** 2
        return cls._create("mfgpu_transfer_create_h_hn_interp", dim, degree, number_type, n_coarse, n_fine, cdp, fdp, pap,
                           chp, n_coarse_dofs, n_fine_dofs, dip, di.size, p1p, cmp_, fmp, wp, j1p)

    @classmethod
    def h_hn_interp_from_meshes(cls, coarse: "Mesh", fine: "Mesh"):
        """h_hn_from_meshes plus the interpolation image (mfgpu_transfer_create_h_hn_interp_from_meshes)"""
        return cls._create("mfgpu_transfer_create_h_hn_interp_from_meshes", coarse._h, fine._h)

    def interpolate(self, dst_coarse, src_fine, stream=None):
        """dst_coarse = the nodal interpolant of src_fine on the coarse mesh (mfgpu_transfer_interpolate); coarse
        Dirichlet dofs and dofs no coarse cell owns become 0.  Needs an object from an h_hn_interp creator"""
        _check(lib().mfgpu_transfer_interpolate(self._h, _ptr(dst_coarse), _ptr(src_fine), stream))

    def prolongate(self, dst_fine, src_coarse, stream=None):
        _check(lib().mfgpu_transfer_prolongate(self._h, _ptr(dst_fine), _ptr(src_coarse), stream))

    def prolongate_add(self, dst_fine, src_coarse, stream=None):
        """dst_fine += P src_coarse"""
        _check(lib().mfgpu_transfer_prolongate_add(self._h, _ptr(dst_fine), _ptr(src_coarse), stream))

    def restrict_and_add(self, dst_coarse, src_fine, stream=None):
        _check(lib().mfgpu_transfer_restrict_and_add(self._h, _ptr(dst_coarse), _ptr(src_fine), stream))

    def memory_consumption(self):
        return int(lib().mfgpu_transfer_memory_consumption(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_transfer_destroy(self._h)
            self._h = None


def p_prolongation_1d(degree_coarse, degree_fine):
    """the default 1D matrix of the p-transfer, [degree_fine + 1, degree_coarse + 1] (mfgpu_transfer_p_prolongation_1d);
    host only"""
    out = np.zeros((max(int(degree_fine), 0) + 1, max(int(degree_coarse), 0) + 1), dtype=np.float64)
    _check(lib().mfgpu_transfer_p_prolongation_1d(int(degree_coarse), int(degree_fine), out.ctypes.data))
    return out


def p_owner_list(dim, degree_fine, fine_cell_dofs, n_fine_dofs, constraint_mask=None):
    """the fine index list of a p-transfer as it is uploaded, [n_cells, (degree_fine + 1)^dim] with bit 31 on every entry
    but the owner's (mfgpu_transfer_p_owner_list); host only"""
    fd = np.ascontiguousarray(fine_cell_dofs, dtype=np.uint32)
    nfd = (max(int(degree_fine), 0) + 1) ** dim
    n_cells = fd.size // nfd
    cm = None if constraint_mask is None else np.ascontiguousarray(constraint_mask, dtype=np.uint32)
    assert fd.size == n_cells * nfd and (cm is None or cm.size == n_cells)
    out = np.zeros((n_cells, nfd), dtype=np.uint32)
    _check(lib().mfgpu_transfer_p_owner_list(dim, int(degree_fine), n_cells, fd.ctypes.data if fd.size else None,
                                             None if cm is None else cm.ctypes.data, n_fine_dofs, out.ctypes.data))
    return out


def coarsening_map(coarse: "Mesh", fine: "Mesh"):
    """(parent, child) [n_fine_cells] each of two leaf meshes (mfgpu_mesh_coarsening_map): the coarse cell of every fine
    cell and 0 (the same cell) or 1 + k (child k of it; bit d of k: the upper half in direction d); host only"""
    parent, child = np.zeros(fine.n_cells, dtype=np.uint32), np.zeros(fine.n_cells, dtype=np.uint32)
    _check(lib().mfgpu_mesh_coarsening_map(coarse._h, fine._h, parent.ctypes.data, child.ctypes.data))
    return parent, child


def mark_fixed_number(indicators, fraction):
    """flags [n] (uint8) of the ceil(fraction * n) largest indicators, ties broken by the lower cell index
    (GridRefinement::refine_and_coarsen_fixed_number without coarsening); host numpy"""
    eta = np.asarray(indicators, dtype=np.float64).reshape(-1)
    if not 0.0 <= fraction <= 1.0:
        raise MfgpuError("mark_fixed_number: fraction must lie in [0, 1]")
    k = min(len(eta), int(np.ceil(fraction * len(eta))))
    flags = np.zeros(len(eta), dtype=np.uint8)
    flags[np.argsort(-eta, kind="stable")[:k]] = 1
    return flags


def mark_refine_coarsen(indicators, refine_fraction, coarsen_fraction):
    """(refine, coarsen) flags [n] (uint8) each: the ceil(refine_fraction * n) largest and the floor(coarsen_fraction * n)
    smallest indicators, ties to the lower cell index; a cell that is marked for refinement is never marked for
    coarsening, so the two sets do not overlap (GridRefinement::refine_and_coarsen_fixed_number); host numpy"""
    eta = np.asarray(indicators, dtype=np.float64).reshape(-1)
    if not (0.0 <= refine_fraction <= 1.0 and 0.0 <= coarsen_fraction <= 1.0):
        raise MfgpuError("mark_refine_coarsen: the fractions must lie in [0, 1]")
    n = len(eta)
    refine = mark_fixed_number(eta, refine_fraction)
    coarsen = np.zeros(n, dtype=np.uint8)
    order = np.argsort(eta, kind="stable")
    order = order[refine[order] == 0]
    coarsen[order[:min(len(order), int(np.floor(coarsen_fraction * n)))]] = 1
    return refine, coarsen


def carry_over(old: "Mesh", mid: "Mesh", new: "Mesh", x_old, homogeneous=True, stream=None):
    """x_new, a DeviceVector on `new`: x_old (device, on `old`) interpolated to `mid` and prolongated to `new`, the three
    meshes those of Mesh.adapted at one degree.  Exact where the mesh did not change or was refined, the nodal interpolant
    where it was coarsened.  homogeneous: the dofs of `mid` on the boundary are carried as 0 (the homogeneous part of a
    solution; the lift is set again on the new mesh); otherwise every value is carried"""
    nt = int(new.desc.number_type)
    if homogeneous:
        down, up = Transfer.h_hn_interp_from_meshes(mid, old), Transfer.h_hn_from_meshes(mid, new)
    else:
        def make(creator, fine):
            dim, p = int(mid.desc.dim), int(mid.desc.degree)
            ma, fa = mid.arrays(), fine.arrays()
            parent, child = coarsening_map(mid, fine)
            return creator(dim, p, ma["loc2glob"], fa["loc2glob"], parent, child, mid.n_dofs, fine.n_dofs, [], nt,
                           coarse_mask=ma["constraint_mask"], fine_mask=fa["constraint_mask"])
        down, up = make(Transfer.h_hn_interp_from_arrays, old), make(Transfer.h_hn_from_arrays, new)
    x_mid, x_new = DeviceVector(mid.n_dofs, nt), DeviceVector(new.n_dofs, nt)
    down.interpolate(x_mid, x_old, stream)
    up.prolongate(x_new, x_mid, stream)
    synchronize()  # the two transfers and x_mid end here
    return x_new


def _ptr(v):
    if isinstance(v, DeviceVector):
        return v.ptr
    if hasattr(v, "data_ptr"):  # torch tensor on the GPU
        return v.data_ptr()
    return int(v)


def _optr(v):
    return None if v is None else _ptr(v)


class IndexPairs:
    """copy_to_mg / copy_from_mg index pairs on the device (mfgpu_index_pairs_*): dst[dst_idx[i]] = src[src_idx[i]]"""

    def __init__(self, dst_idx, src_idx):
        a = np.ascontiguousarray(dst_idx, dtype=np.uint32)
        b = np.ascontiguousarray(src_idx, dtype=np.uint32)
        assert a.size == b.size
        h = C.c_void_p()
        _check(lib().mfgpu_index_pairs_create(a.ctypes.data if a.size else None, b.ctypes.data if b.size else None,
                                              a.size, C.byref(h)))
        self._h = h

    def copy(self, dst, src, number_type=F64, stream=None):
        _check(lib().mfgpu_vec_copy_pairs(self._h, _ptr(dst), _ptr(src), number_type, stream))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_index_pairs_destroy(self._h)
            self._h = None


# ---- mixed-precision multigrid and the fused Chebyshev smoother (include/mfgpu.h).  Vectors: DeviceVector, a torch
# tensor on the GPU or a device address; the raw return code is given back so that tests can check MFGPU_EINVAL.
def vec_convert(dst, dst_type, src, src_type, n, stream=None, check=True):
    """dst[i] = (dst_type) src[i] for i < n"""
    rc = lib().mfgpu_vec_convert(_ptr(dst), dst_type, _ptr(src), src_type, n, stream)
    return _check(rc) if check else rc


def copy_pairs_convert(pairs: "IndexPairs", dst, dst_type, src, src_type, stream=None, check=True):
    """dst[dst_idx[i]] = (dst_type) src[src_idx[i]] over the pairs; other entries of dst untouched"""
    rc = lib().mfgpu_vec_copy_pairs_convert(pairs._h, _ptr(dst), dst_type, _ptr(src), src_type, stream)
    return _check(rc) if check else rc


def chebyshev_start(x, upd, r, b, t, dinv, f, zero_start, n, number_type, stream=None, check=True):
    """r = b - t (t None: r = b); upd = f dinv r; x = upd (zero_start) or x += upd"""
    rc = lib().mfgpu_vec_chebyshev_start(_ptr(x), _ptr(upd), _ptr(r), _ptr(b), None if t is None else _ptr(t),
                                         _ptr(dinv), float(f), 1 if zero_start else 0, n, number_type, stream)
    return _check(rc) if check else rc


def chebyshev_update(x, upd, r, t, dinv, f1, f2, n, number_type, stream=None, check=True):
    """r -= t; upd = f1 upd + f2 dinv r; x += upd"""
    rc = lib().mfgpu_vec_chebyshev_update(_ptr(x), _ptr(upd), _ptr(r), _ptr(t), _ptr(dinv), float(f1), float(f2), n,
                                          number_type, stream)
    return _check(rc) if check else rc


def chebyshev_start_dev(x, upd, r, b, t, dinv, f_dev, zero_start, n, number_type, stream=None, check=True):
    """chebyshev_start with f read from device memory: f_dev is a device address (or vector) of one double"""
    rc = lib().mfgpu_vec_chebyshev_start_dev(_ptr(x), _ptr(upd), _ptr(r), _ptr(b), None if t is None else _ptr(t),
                                             _ptr(dinv), _optr(f_dev), 1 if zero_start else 0, n, number_type, stream)
    return _check(rc) if check else rc


def chebyshev_update_dev(x, upd, r, t, dinv, f12_dev, n, number_type, stream=None, check=True):
    """chebyshev_update with (f1, f2) read from device memory: f12_dev is a device address (or vector) of two doubles"""
    rc = lib().mfgpu_vec_chebyshev_update_dev(_ptr(x), _ptr(upd), _ptr(r), _ptr(t), _ptr(dinv), _optr(f12_dev), n,
                                              number_type, stream)
    return _check(rc) if check else rc


def chebyshev_scalars_dev(degree, lambda_max_dev, smoothing_range, f_dev, stream=None, check=True):
    """cg_chebyshev_scalars on a lambda_max in device memory into f_dev [2 * degree - 1] doubles; one small launch"""
    rc = lib().mfgpu_cg_chebyshev_scalars_dev(int(degree), _optr(lambda_max_dev), float(smoothing_range), _optr(f_dev),
                                              stream)
    return _check(rc) if check else rc


def eig_workspace_bytes(n_dofs, number_type):
    """bytes of the workspace of estimate_lambda_max_enqueue (mfgpu_eig_workspace_bytes); host only"""
    return int(lib().mfgpu_eig_workspace_bytes(int(n_dofs), int(number_type)))


def estimate_lambda_max_enqueue(op, inv_diag, min_iterations, n_steps, workspace, stream=None, check=True):
    """the power iteration of estimate_lambda_max, enqueued: n_steps steps with the host's stopping rule as a freeze rule;
    the workspace (eig_workspace_bytes, a device vector or address) starts with an EigResult (eig_result reads it)"""
    rc = lib().mfgpu_estimate_lambda_max_enqueue(None if op is None else _op_handle(op), _optr(inv_diag),
                                                 int(min_iterations), int(n_steps), _optr(workspace), stream)
    return _check(rc) if check else rc


def eig_result(workspace):
    """the EigResult at the head of a workspace of estimate_lambda_max_enqueue (blocking copy)"""
    r = EigResult()
    _check(lib().mfgpu_vec_to_host(C.addressof(r), _ptr(workspace), C.sizeof(r) // 8, F64))  # 24 bytes
    return r


def spd_inverse_workspace_bytes(n):
    """bytes of the workspace of spd_inverse_enqueue (mfgpu_spd_inverse_workspace_bytes); host only"""
    return int(lib().mfgpu_spd_inverse_workspace_bytes(int(n)))


def spd_inverse_enqueue(n, a, lda, inv, ld, workspace, status, stream=None, check=True):
    """spd_inverse on the device: a [n rows of lda doubles, lower triangle read] -> inv [n rows of ld doubles, columns
    n .. ld - 1 zero]; status: device address of a uint32 that gets 0, or 1 for a matrix that is not positive definite
    (inv then keeps its contents).  All arguments are device vectors or addresses; only enqueues"""
    rc = lib().mfgpu_spd_inverse_enqueue(int(n), _optr(a), int(lda), _optr(inv), int(ld), _optr(workspace), _optr(status),
                                         stream)
    return _check(rc) if check else rc


def vec_residual(t, b, e, n, number_type, stream=None, check=True):
    """t = b - t (e None) or t = b - (t + e)"""
    rc = lib().mfgpu_vec_residual(_ptr(t), _ptr(b), _optr(e), n, number_type, stream)
    return _check(rc) if check else rc


def estimate_lambda_max(op, inv_diag, min_iterations=15, with_steps=False):
    """1.2 x the power-iteration estimate of the largest eigenvalue of D^-1 A (mfgpu_estimate_lambda_max); blocks.
    op: an Operator, a Level (its level matrix) or anything with the handle in _h.  with_steps: (estimate, steps taken)"""
    r, steps = C.c_double(), C.c_uint32()
    _check(lib().mfgpu_estimate_lambda_max_steps(_op_handle(op), _ptr(inv_diag), int(min_iterations), C.byref(r),
                                                 C.byref(steps)))
    return (r.value, int(steps.value)) if with_steps else r.value


def spd_inverse(a, check=True):
    """the inverse of a symmetric positive definite matrix by the library's Cholesky (mfgpu_spd_inverse; only the lower
    triangle of a is read); host only.  check=False: (code, inverse)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.ndim == 2 and a.shape[0] == a.shape[1]
    inv = np.empty_like(a)
    rc = lib().mfgpu_spd_inverse(a.shape[0], a.ctypes.data, inv.ctypes.data)
    if check:
        _check(rc)
        return inv
    return rc, inv


def _op_handle(op):
    """the mfgpu_handle of an Operator, of a Level (its level matrix) or a raw handle"""
    if isinstance(op, Level):
        return lib().mfgpu_level_operator(op._h)
    return getattr(op, "_h", op)


class VCycle:
    """The multigrid V-cycle as one object (mfgpu_vcycle_*): z = M^-1 r with Chebyshev smoothers and a device-resident
    coarse solve; apply only enqueues work.

    levels: coarse to fine, one dict per level with "op" (an Operator, or a Level: then its level matrix with the level as
    `edges` when has_edges is true), optional "transfer" (a Transfer from the coarser level; None on level 0), optional
    "to_mg" / "from_mg" (IndexPairs; on every level or on none).  The pieces are borrowed by the library and kept alive
    here.  options: smoother_degree, smoothing_range, eig_iterations, lambda_max (per level, or None = estimate),
    coarse (VCYCLE_COARSE_*), coarse_tolerance, coarse_max_iterations."""

    def __init__(self, levels, active_type, n_active, smoother_degree=0, smoothing_range=0.0, eig_iterations=0,
                 lambda_max=None, coarse=VCYCLE_COARSE_AUTO, coarse_tolerance=0.0, coarse_max_iterations=0, keep=None):
        self._keep = (levels, keep)
        self.n_levels, self.active_type, self.n_active = len(levels), int(active_type), int(n_active)
        ld = (VCycleLevelDesc * max(len(levels), 1))()
        for l, lev in enumerate(levels):
            op = lev.get("op")
            if isinstance(op, Level):
                ld[l].op = lib().mfgpu_level_operator(op._h)
                ld[l].edges = op._h if lev.get("has_edges", False) else None
            elif op is not None:
                ld[l].op = getattr(op, "_h", op)
                edges = lev.get("edges")
                ld[l].edges = None if edges is None else edges._h
            for key, field in (("transfer", "from_coarser"), ("to_mg", "to_mg"), ("from_mg", "from_mg")):
                piece = lev.get(key)
                setattr(ld[l], field, None if piece is None else piece._h)
        d = VCycleDesc()
        d.n_levels, d.levels = len(levels), ld
        d.active_type, d.n_active = int(active_type), int(n_active)
        d.smoother_degree, d.smoothing_range, d.eig_iterations = int(smoother_degree), float(smoothing_range), int(eig_iterations)
        lam = None
        if lambda_max is not None:
            lam = (C.c_double * len(levels))(*[float(x) for x in lambda_max])
            d.lambda_max = lam
        d.coarse, d.coarse_tolerance, d.coarse_max_iterations = int(coarse), float(coarse_tolerance), int(coarse_max_iterations)
        h = C.c_void_p()
        _check(lib().mfgpu_vcycle_create(C.byref(d), C.byref(h)))
        self._h = h

    @staticmethod
    def _flagged(desc, flags):
        """a copy of the description with `flags` added (UPDATABLE_COEFFICIENTS for levels that refresh() follows)"""
        d = Desc.from_buffer_copy(desc)
        d.flags |= int(flags)
        return d

    @staticmethod
    def hierarchy_levels(mesh: "Mesh", flags=0):
        """(levels, keep) of the constructor for the hierarchy of an adaptive stand-in mesh (Mesh.adaptive_mg): level
        operators with refinement edges, transfers over the refined parents and the copy pairs of mfgpu_mg_*, all in the
        mesh's number type; `flags` are added to every level's description"""
        dim, p, nt = int(mesh.desc.dim), int(mesh.desc.degree), int(mesh.desc.number_type)
        H = MgHierarchy(mesh)
        nd, nfd = (p + 1) ** dim, (2 * p + 1) ** dim
        meshes = [H.level_mesh(l) for l in range(H.n_levels)]
        levels = []
        for l, M in enumerate(meshes):
            E = H.edge_dofs(l)
            a, b = H.copy_pairs(l)
            tr = None
            if l > 0:
                cd, fd = H.transfer_arrays(l, nd, nfd)
                con = _view(meshes[l - 1].desc.constrained_dofs, meshes[l - 1].desc.n_constrained, np.uint32)
                tr = Transfer.from_arrays(dim, p, cd, fd, meshes[l - 1].n_dofs, M.n_dofs, con, nt)
            levels.append({"op": Level(VCycle._flagged(M.desc, flags), E, (M, H)), "has_edges": len(E) > 0, "n_dofs": M.n_dofs, "transfer": tr,
                           "to_mg": IndexPairs(b, a), "from_mg": IndexPairs(a, b)})
        return levels, (mesh, H, meshes)

    @classmethod
    def from_hierarchy(cls, mesh: "Mesh", level_type=F64, active_type=F64, flags=0, **options):
        """the local-smoothing V-cycle of an adaptive stand-in mesh (Mesh.adaptive_mg) built in level_type; the active
        vectors are of active_type with mesh.n_dofs entries (a float V-cycle under a double CG)"""
        if int(mesh.desc.number_type) != level_type:
            raise MfgpuError("VCycle.from_hierarchy: build the mesh in the level number type (Mesh.adaptive_mg(..., "
                             "number_type=level_type)); the active vectors may be of another type")
        levels, keep = cls.hierarchy_levels(mesh, flags)
        return cls(levels, active_type, mesh.n_dofs, keep=keep, **options)

    @classmethod
    def from_meshes(cls, meshes, active_type=None, flags=0, **options):
        """globally refined cubes or balls, coarse to fine (uniform meshes of n, 2n, 4n ... cells per direction or balls
        of successive n_ref): no edges, no pairs, the active vector is the finest level's"""
        nt = int(meshes[0].desc.number_type)
        levels = [{"op": Operator(cls._flagged(M.desc, flags), M), "n_dofs": M.n_dofs,
                   "transfer": Transfer.from_meshes(meshes[l - 1], M) if l else None} for l, M in enumerate(meshes)]
        return cls(levels, nt if active_type is None else active_type, meshes[-1].n_dofs, keep=list(meshes), **options)

    @staticmethod
    def level_mesh_levels(meshes, flags=0):
        """the `levels` of the constructor for any coarse-to-fine list of stand-in meshes: between two consecutive meshes
        the h-transfer when the degrees are equal (conforming cubes or balls, the finer one the global refinement), the
        p-transfer when the degree rises (then the cells must be the same; with hanging nodes -- adaptive meshes, meshes
        from leaves -- Transfer.p_hn_from_meshes); anything else raises"""
        levels = []
        for l, M in enumerate(meshes):
            tr = None
            if l:
                pc, pf = int(meshes[l - 1].desc.degree), int(M.desc.degree)
                if pc > pf:
                    raise MfgpuError(f"VCycle.level_mesh_levels: the degree falls from {pc} to {pf} between levels "
                                     f"{l - 1} and {l}")
                masked = bool(meshes[l - 1].desc.constraint_mask) or bool(M.desc.constraint_mask)
                leaf = len(meshes[l - 1].cell_levels()) > 0 or len(M.cell_levels()) > 0  # (cells_kind == -1)
                if pc == pf and (masked or leaf):
                    tr = Transfer.h_hn_from_meshes(meshes[l - 1], M)  # global coarsening: two leaf meshes
                elif pc == pf:
                    tr = Transfer.from_meshes(meshes[l - 1], M)
                else:  # (a leaf mesh without a hanging node has no mask, and p_from_meshes refuses leaf meshes)
                    tr = (Transfer.p_hn_from_meshes if masked or leaf else Transfer.p_from_meshes)(meshes[l - 1], M)
            levels.append({"op": Operator(VCycle._flagged(M.desc, flags), M), "n_dofs": M.n_dofs, "transfer": tr})
        return levels

    @classmethod
    def from_level_meshes(cls, meshes, active_type=None, flags=0, **options):
        """h- and p-multigrid over level_mesh_levels(meshes): no edges, no pairs, the active vector is the finest level's.
        h-levels at degree 1 followed by 1 -> 2 -> 4 on the finest mesh is the hybrid hierarchy of host/poisson_pmg.cc"""
        nt = int(meshes[0].desc.number_type)
        return cls(cls.level_mesh_levels(meshes, flags), nt if active_type is None else active_type, meshes[-1].n_dofs,
                   keep=list(meshes), **options)

    @classmethod
    def from_global_coarsening(cls, mesh: "Mesh", degrees=None, active_type=None, flags=0, min_cells=None, **options):
        """global-coarsening multigrid on ONE leaf mesh with hanging nodes (Mesh.adaptive, Mesh.from_leaves): from_level_meshes
        over Mesh.coarsening_sequence(mesh) at the lowest degree followed by `mesh`'s cells at the rising `degrees` (None: the
        mesh's degree throughout; the last one must be the mesh's).  Every level is a complete mesh: no edges, no pairs"""
        p = int(mesh.desc.degree)
        degrees = (p,) if degrees is None else tuple(int(d) for d in degrees)
        if degrees[-1] != p or any(a >= b for a, b in zip(degrees, degrees[1:])):
            raise MfgpuError(f"VCycle.from_global_coarsening: degrees {degrees} must rise and end at the mesh's degree {p}")
        dim, nt = int(mesh.desc.dim), int(mesh.desc.number_type)
        meshes = Mesh.coarsening_sequence(mesh, degrees[0], min_cells)
        leaves = mesh.cell_levels()
        meshes += [Mesh.from_leaves(dim, d, leaves, number_type=nt) for d in degrees[1:-1]]
        if len(degrees) > 1:
            meshes.append(mesh)
        return cls.from_level_meshes(meshes, active_type, flags, **options)

    def apply(self, z, r, stream=None, check=True):
        """z = M^-1 r on active vectors (enqueued on `stream`)"""
        rc = lib().mfgpu_vcycle_apply(self._h, _optr(z), _optr(r), stream)
        return _check(rc) if check else rc

    def refresh(self, eig_steps=0, stream=None, check=True):
        """mfgpu_vcycle_refresh: recompute the inverse diagonals, the eigenvalue estimates with the smoothers' scalars
        (where lambda_max was estimated at creation; eig_steps steps per level, 0 = as many as at creation) and the dense
        coarse inverse from what the level operators hold now.  Only enqueues on `stream`; the first call allocates"""
        rc = lib().mfgpu_vcycle_refresh(self._h, int(eig_steps), stream)
        return _check(rc) if check else rc

    def refresh_status(self, stream=None):
        """mfgpu_vcycle_refresh_status (blocking): the VCycleRefreshInfo of the last refresh; lambda_max() follows"""
        info = VCycleRefreshInfo()
        _check(lib().mfgpu_vcycle_refresh_status(self._h, stream, C.byref(info)))
        return info

    def lambda_max(self):
        out = (C.c_double * self.n_levels)()
        _check(lib().mfgpu_vcycle_lambda_max(self._h, out))
        return np.array(out[:], dtype=np.float64)

    def memory_consumption(self):
        return int(lib().mfgpu_vcycle_memory_consumption(self._h))

    def destroy(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mfgpu_vcycle_destroy(self._h)
            self._h = None

    __del__ = destroy


def multi_groups(n_vectors, widths):
    """how vmult_multi cuts n_vectors into groups for the given fused widths (descending); host only"""
    w = (C.c_uint32 * max(len(widths), 1))(*widths)
    out = (C.c_uint32 * max(int(n_vectors), 1))()
    n = lib().mfgpu_plan_multi_groups(int(n_vectors), w, len(widths), out, len(out))
    if n < 0:
        _check(n)
    return [int(out[i]) for i in range(n)]


def synchronize():
    _check(lib().mfgpu_device_synchronize())


def device_memory_info():
    """(free, total) bytes of the current device"""
    f, t = C.c_size_t(), C.c_size_t()
    _check(lib().mfgpu_device_memory_info(C.byref(f), C.byref(t)))
    return f.value, t.value


def guard_layout(n_bytes, guard_bytes):
    """(total bytes, payload offset) of a guard-mode allocation (mfgpu_debug_guard_layout; needs no device)"""
    total, off = C.c_size_t(), C.c_size_t()
    _check(lib().mfgpu_debug_guard_layout(int(n_bytes), int(guard_bytes), C.byref(total), C.byref(off)))
    return total.value, off.value


@contextlib.contextmanager
def guards(guard_bytes):
    """guard mode of the library's own device arrays (include/mfgpu.h) for the handles created inside the block"""
    _check(lib().mfgpu_debug_guard_begin(int(guard_bytes)))
    try:
        yield
    finally:
        _check(lib().mfgpu_debug_guard_end())


def guard_check_raw():
    """(n_live, n_damaged, report) of mfgpu_debug_guard_check"""
    live, damaged, report = C.c_uint64(), C.c_uint64(), C.create_string_buffer(2048)
    _check(lib().mfgpu_debug_guard_check(C.byref(live), C.byref(damaged), report, len(report)))
    return int(live.value), int(damaged.value), report.value.decode()


def guard_check():
    """the number of registered arrays; raises with the report when a guard is damaged"""
    live, damaged, report = guard_check_raw()
    if damaged:
        raise MfgpuError(f"{damaged} damaged guard(s) among {live} live arrays:\n{report}")
    return live


def guard_selftest():
    """(n_damaged, report, poisoned_ok, zeroed_ok) of mfgpu_debug_guard_selftest"""
    damaged, report, p_ok, z_ok = C.c_uint64(), C.create_string_buffer(2048), C.c_int(), C.c_int()
    _check(lib().mfgpu_debug_guard_selftest(C.byref(damaged), report, len(report), C.byref(p_ok), C.byref(z_ok)))
    return int(damaged.value), report.value.decode(), bool(p_ok.value), bool(z_ok.value)


def dist_unique_id() -> bytes:
    """rank 0: the 128-byte RCCL unique id every rank passes to Dist (mfgpu_dist_unique_id)"""
    buf = C.create_string_buffer(128)
    _check(lib().mfgpu_dist_unique_id(buf))
    return buf.raw


class Dist:
    """mfgpu_dist: exchange of a z-slab's interface planes with its two neighbours (include/mfgpu.h).
    unique_id = the bytes of dist_unique_id() (RCCL transport, collective over all ranks), or None (in-process
    transport: connect neighbours with connect_local)."""

    def __init__(self, mesh: "Mesh", rank: int, world: int, unique_id=None):
        lo = np.ascontiguousarray(mesh.interface_dofs(0), dtype=np.uint32)
        up = np.ascontiguousarray(mesh.interface_dofs(1), dtype=np.uint32)
        con = np.ascontiguousarray(mesh.arrays()["constrained_dofs"], dtype=np.uint32)
        self._keep = (lo, up, con)
        self.number_type = mesh.desc.number_type
        d = C.c_void_p()
        L = lib()
        L.mfgpu_dist_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                        C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        _check(L.mfgpu_dist_create(unique_id, rank, world, lo.ctypes.data if lo.size else None, lo.size,
                                   up.ctypes.data if up.size else None, up.size, con.ctypes.data if con.size else None,
                                   con.size, mesh.n_dofs, self.number_type, C.byref(d)))
        self._d = d
        for f in ("mfgpu_dist_connect_local", "mfgpu_dist_attach"):
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p]
        L.mfgpu_vmult_dist_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_vmult_dist.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_vmult_dist_end.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mfgpu_dist_destroy.argtypes = [C.c_void_p]

    def __del__(self):
        if getattr(self, "_d", None) and _lib is not None:
            _lib.mfgpu_dist_destroy(self._d)
            self._d = None

    def connect_local(self, upper: "Dist"):
        """in-process transport: `upper` is the slab above this one"""
        _check(lib().mfgpu_dist_connect_local(self._d, upper._d))

    def attach(self, op: "Operator"):
        _check(lib().mfgpu_dist_attach(self._d, op._h))

    def schedule(self):
        """(interface_first, r1_end, r2_begin, n_batches): mfgpu_dist_schedule"""
        info = (C.c_uint32 * 4)()
        lib().mfgpu_dist_schedule.argtypes = [C.c_void_p, C.c_void_p]
        _check(lib().mfgpu_dist_schedule(self._d, info))
        return bool(info[0]), int(info[1]), int(info[2]), int(info[3])

    def vmult_begin(self, op, dst, src, stream=None):
        _check(lib().mfgpu_vmult_dist_begin(op._h, self._d, _ptr(dst), _ptr(src), stream))

    def vmult_end(self, op, dst, stream=None):
        _check(lib().mfgpu_vmult_dist_end(op._h, self._d, _ptr(dst), stream))

    def vmult(self, op, dst, src, stream=None):
        _check(lib().mfgpu_vmult_dist(op._h, self._d, _ptr(dst), _ptr(src), stream))
