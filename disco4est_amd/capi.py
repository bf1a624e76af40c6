"""ctypes binding of libd4est_hip.so (include/d4est_hip.h).

Only plumbing lives here: argument marshalling and a ``Plan`` class whose methods
take torch CUDA tensors and pass their ``data_ptr()`` through the C-ABI.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libd4est_hip.so")

_c_int_p = ctypes.POINTER(ctypes.c_int)
_c_double_p = ctypes.POINTER(ctypes.c_double)
_vp = ctypes.c_void_p

# name -> (restype, argtypes); mirrors include/d4est_hip.h one to one
SIGNATURES = {
    "d4est_hip_version": (ctypes.c_char_p, []),
    "d4est_hip_device_count": (ctypes.c_int, []),
    "d4est_hip_table": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_double_p]),
    "d4est_hip_malloc": (_vp, [ctypes.c_size_t]),
    "d4est_hip_free": (None, [_vp]),
    "d4est_hip_memcpy_h2d": (None, [_vp, _vp, ctypes.c_size_t]),
    "d4est_hip_memcpy_d2h": (None, [_vp, _vp, ctypes.c_size_t]),
    "d4est_hip_memset": (None, [_vp, ctypes.c_int, ctypes.c_size_t]),
    "d4est_hip_device_synchronize": (None, []),
    "d4est_hip_plan_create": (_vp, [ctypes.c_int, _c_int_p, _c_int_p, _c_int_p, _c_int_p, ctypes.c_int]),
    "d4est_hip_plan_destroy": (None, [_vp]),
    "d4est_hip_plan_set_stream": (None, [_vp, _vp]),
    "d4est_hip_plan_set_tuning": (None, [_vp, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_plan_last_kernel": (ctypes.c_char_p, [_vp]),
    "d4est_hip_plan_face_path": (ctypes.c_char_p, [_vp]),
    "d4est_hip_plan_local_nodes": (ctypes.c_int, [_vp]),
    "d4est_hip_plan_local_nodes_quad": (ctypes.c_int, [_vp]),
    "d4est_hip_plan_stream_mode": (ctypes.c_int, [_vp]),
    "d4est_hip_plan_n_elements": (ctypes.c_int, [_vp]),
    "d4est_hip_plan_set_geometry": (None, [_vp, _vp, _vp, ctypes.c_int]),
    "d4est_hip_apply_stiffness_matrix": (None, [_vp, _vp, _vp]),
    "d4est_hip_apply_mass_matrix": (None, [_vp, _vp, _vp]),
    "d4est_hip_apply_galerkin_integral": (None, [_vp, _vp, _vp]),
    "d4est_hip_interpolate": (None, [_vp, _vp, _vp]),
    "d4est_hip_apply_weighted_mass_matrix": (None, [_vp, _vp, _vp, _vp]),
    "d4est_hip_apply_inverse_mass_matrix": (None, [_vp, _vp, _vp]),
    "d4est_hip_plan_face_nodes": (ctypes.c_int, [_vp]),
    "d4est_hip_apply_slicer": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_apply_lift": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_apply_dij": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_apply_dij_transpose": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_apply_mij": (None, [_vp, _vp, _vp]),
    "d4est_hip_apply_invmij": (None, [_vp, _vp, _vp]),
    "d4est_hip_compute_dudr": (None, [_vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_build_sides": (ctypes.c_int, [ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp,
                                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_topology_table": (ctypes.c_int, [ctypes.c_int, _vp]),
    "d4est_hip_plan_set_faces": (None, [_vp, _c_int_p, _c_int_p, _c_int_p, _c_int_p, _c_int_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, _c_int_p, _c_int_p]),
    "d4est_hip_plan_set_hanging": (None, [_vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_plan_set_geometry_numerical": (None, [_vp, _vp, ctypes.c_int]),
    "d4est_hip_plan_set_geometry_brick": (None, [_vp, _vp, ctypes.c_double, _vp]),
    "d4est_hip_plan_set_geometry_analytic": (None, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_double]),
    "d4est_hip_plan_set_mortar_geometry_analytic": (None, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double]),
    "d4est_hip_plan_compute_xyz_analytic": (None, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_double, _vp, _vp]),
    "d4est_hip_tree_map": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp]),
    "d4est_hip_plan_set_mortar_geometry_brick": (None, [_vp, _vp, ctypes.c_double, _vp]),
    "d4est_hip_tree_map_d2": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, _vp, _vp]),
    "d4est_hip_plan_set_hessian_brick": (None, [_vp, _vp, ctypes.c_double, _vp]),
    "d4est_hip_plan_set_hessian_analytic": (None, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_double]),
    "d4est_hip_plan_set_hessian_numerical": (None, [_vp, _vp, _vp, ctypes.c_int]),
    "d4est_hip_plan_hessian_info": (ctypes.c_int, [_vp]),
    "d4est_hip_plan_hessian_supported": (ctypes.c_int, [_vp]),
    "d4est_hip_hessian_trace": (None, [_vp, _vp, _vp]),
    "d4est_hip_estimator_bi_pointwise": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_plan_set_h_types": (None, [_vp, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_plan_compute_size_parameters_brick": (None, [_vp, _vp, _vp, ctypes.c_double, _vp]),
    "d4est_hip_plan_compute_size_parameters_analytic": (None, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double]),
    "d4est_hip_plan_compute_diameters": (None, [_vp, _vp]),
    "d4est_hip_plan_size_parameter": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp]),
    "d4est_hip_transfer_create": (_vp, [ctypes.c_int, _vp, _vp, _vp]),
    "d4est_hip_transfer_destroy": (None, [_vp]),
    "d4est_hip_transfer_set_stream": (None, [_vp, _vp]),
    "d4est_hip_transfer_coarse_nodes": (ctypes.c_longlong, [_vp]),
    "d4est_hip_transfer_fine_nodes": (ctypes.c_longlong, [_vp]),
    "d4est_hip_transfer_prolong": (None, [_vp, _vp, _vp]),
    "d4est_hip_transfer_prolong_add": (None, [_vp, _vp, _vp]),
    "d4est_hip_transfer_restrict": (None, [_vp, _vp, _vp]),
    "d4est_hip_transfer_project": (None, [_vp, _vp, _vp]),
    "d4est_hip_transfer_describe": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
    "d4est_hip_schwarz_create": (_vp, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "d4est_hip_schwarz_destroy": (None, [_vp]),
    "d4est_hip_schwarz_nodal_size": (ctypes.c_longlong, [_vp]),
    "d4est_hip_schwarz_restricted_nodal_size": (ctypes.c_longlong, [_vp]),
    "d4est_hip_schwarz_condensed_copies": (ctypes.c_int, [_vp]),
    "d4est_hip_schwarz_restrict_field": (None, [_vp, _vp, _vp]),
    "d4est_hip_schwarz_apply_over_subdomains": (None, [_vp, _vp, _vp]),
    "d4est_hip_schwarz_add_correction": (None, [_vp, _vp, _vp]),
    "d4est_hip_schwarz_iterate": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    "d4est_hip_schwarz_smooth": (None, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    "d4est_hip_schwarz_get_info": (None, [_vp, _vp, _vp]),
    "d4est_hip_schwarz_host_reads": (ctypes.c_longlong, [_vp]),
    "d4est_hip_schwarz_set_subdomain_solver": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_schwarz_subdomain_solver": (None, [_vp, _vp, _vp, _vp]),
    "d4est_hip_schwarz_set_element_exchange": (None, [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_schwarz_own_nodes": (ctypes.c_longlong, [_vp]),
    "d4est_hip_schwarz_exchange_first": (ctypes.c_longlong, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_schwarz_set_rccl_exchange": (_vp, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_schwarz_rccl_exchange_destroy": (None, [_vp]),
    "d4est_hip_schwarz_rccl_exchange_count": (ctypes.c_longlong, [_vp]),
    "d4est_hip_plan_set_sipg": (None, [_vp, ctypes.c_double, ctypes.c_int]),
    "d4est_hip_plan_set_mortar_geometry": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "d4est_hip_plan_set_estimator": (None, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]),
    "d4est_hip_estimator_bi": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_plan_estimator_info": (ctypes.c_int, [_vp, _vp, _vp]),
    "d4est_hip_plan_set_energy_norm": (None, [_vp, ctypes.c_int, ctypes.c_double]),
    "d4est_hip_plan_energy_norm_info": (ctypes.c_int, [_vp, _vp, _vp]),
    "d4est_hip_norms_error": (None, [_vp, _vp, _vp, _vp]),
    "d4est_hip_norm_l2_sqr": (None, [_vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_norm_linfty": (None, [_vp, _vp, _vp, _vp]),
    "d4est_hip_ip_energy_norm_sqr": (None, [_vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_masked_sum": (None, [_vp, _vp, _vp, _vp]),
    "d4est_hip_plan_bndry_nodes": (ctypes.c_int, [_vp]),
    "d4est_hip_plan_boundary_gather": (None, [_vp, _vp, _vp]),
    "d4est_hip_plan_set_dirichlet_values": (None, [_vp, _vp, ctypes.c_int]),
    "d4est_hip_plan_set_robin_values": (None, [_vp, _vp, _vp, ctypes.c_int]),
    "d4est_hip_plan_trace_size": (ctypes.c_longlong, [_vp]),
    "d4est_hip_plan_ghost_trace_size": (ctypes.c_longlong, [_vp]),
    "d4est_hip_compute_ghost_traces": (None, [_vp, _vp, _vp]),
    "d4est_hip_compute_face_traces": (None, [_vp, _vp, _vp]),
    "d4est_hip_apply_flux": (None, [_vp, _vp, _vp, _vp]),
    "d4est_hip_apply_aij": (None, [_vp, _vp, _vp, _vp]),
    "d4est_hip_build_rhs_with_strong_bc": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_build_rhs_with_strong_bc_host": (None, [_vp, _c_double_p, ctypes.c_int, _c_double_p]),
    "d4est_hip_plan_set_lhs_coefficient": (None, [_vp, _vp]),
    "d4est_hip_plan_lhs_coefficient_arrays": (ctypes.c_int, [_vp, _vp, _vp]),
    "d4est_hip_plan_matrix_nodes": (ctypes.c_longlong, [_vp]),
    "d4est_hip_compute_weighted_mass_blocks": (None, [_vp, _vp, _vp]),
    "d4est_hip_plan_set_lhs_element_blocks": (None, [_vp, _vp, _vp]),
    "d4est_hip_plan_set_lhs_galerkin_chain": (None, [_vp, ctypes.c_int, _vp, _vp]),
    "d4est_hip_transfer_fine_matrix_nodes": (ctypes.c_longlong, [_vp]),
    "d4est_hip_transfer_coarse_matrix_nodes": (ctypes.c_longlong, [_vp]),
    "d4est_hip_transfer_galerkin_blocks": (None, [_vp, _vp, _vp, ctypes.c_int]),
    "d4est_hip_plan_set_comm": (None, [_vp, _vp, _vp, _vp]),
    "d4est_hip_apply_lhs": (None, [_vp, _vp, _vp]),
    "d4est_hip_cheby_iterate": (None, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int]),
    "d4est_hip_cheby_update": (None, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp]),
    "d4est_hip_cg_eigs": (ctypes.c_double, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _c_double_p]),
    "d4est_hip_cg_solve": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, _c_double_p]),
    "d4est_hip_cg_solve_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, _c_double_p]),
    "d4est_hip_fcg_solve": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, _vp, _vp, _c_double_p]),
    "d4est_hip_plan_set_nonlinear_power": (None, [_vp, _vp, _vp, ctypes.c_int]),
    "d4est_hip_plan_set_nonlinear_abs_power": (None, [_vp, _vp, _vp, ctypes.c_double]),
    "d4est_hip_plan_nonlinear_exponent": (ctypes.c_int, [_vp, _vp]),
    "d4est_hip_apply_nonlinear_term": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_plan_nonlinear_fused": (ctypes.c_int, [_vp]),
    "d4est_hip_plan_linearise": (None, [_vp, _vp]),
    "d4est_hip_build_residual": (None, [_vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_newton_solve": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_double, ctypes.c_double, _vp, _vp, _vp, _vp, _c_double_p, _c_int_p]),
    "d4est_hip_multigrid_check": (ctypes.c_int, [ctypes.c_int, _vp, _vp]),
    "d4est_hip_multigrid_create": (_vp, [ctypes.c_int, _vp, _vp]),
    "d4est_hip_multigrid_destroy": (None, [_vp]),
    "d4est_hip_multigrid_set_stream": (None, [_vp, _vp]),
    "d4est_hip_multigrid_set_smoother_cheby": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                                              ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_multigrid_set_bottom_solver_cg": (None, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    "d4est_hip_multigrid_set_bottom_solver_cheby": (None, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int]),
    "d4est_hip_multigrid_ready": (ctypes.c_int, [_vp]),
    "d4est_hip_multigrid_vcycle": (None, [_vp, _vp, _vp, _vp, ctypes.c_int]),
    "d4est_hip_multigrid_vcycle_r2": (ctypes.c_double, [_vp]),
    "d4est_hip_multigrid_solve": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, _c_double_p]),
    "d4est_hip_multigrid_set_pc": (None, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    "d4est_hip_multigrid_pc_apply": (None, [_vp, _vp, _vp]),
    "d4est_hip_multigrid_get_info": (None, [_vp, _c_double_p, _c_int_p, _c_int_p]),
    "d4est_hip_multigrid_set_smoother_schwarz": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    "d4est_hip_multigrid_smooth_level": (None, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "d4est_hip_multigrid_set_bottom_solver_reuse_smoother": (None, [_vp]),
    "d4est_hip_pc_cheby_create": (_vp, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_pc_cheby_destroy": (None, [_vp]),
    "d4est_hip_pc_cheby_apply": (None, [_vp, _vp, _vp]),
    "d4est_hip_pc_cheby_eig": (ctypes.c_double, [_vp, _c_int_p]),
    "d4est_hip_pc_cheby_reset_eig": (None, [_vp]),
    "d4est_hip_pc_schwarz_create": (_vp, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    "d4est_hip_pc_schwarz_destroy": (None, [_vp]),
    "d4est_hip_pc_schwarz_apply": (None, [_vp, _vp, _vp]),
    "d4est_hip_copy_blocks": (None, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_plan_trace_offset": (ctypes.c_longlong, [_vp, ctypes.c_int]),
    "d4est_hip_plan_side_blocks": (ctypes.c_int, [_vp, ctypes.c_int]),
    "d4est_hip_reorient_face_order": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_face_reorder_code": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_plan_trace_offset_sub": (ctypes.c_longlong, [_vp, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_plan_ghost_trace_offset_sub": (ctypes.c_longlong, [_vp, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_plan_trace_block_len_sub": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_plan_ghost_trace_offset": (ctypes.c_longlong, [_vp, ctypes.c_int]),
    "d4est_hip_plan_trace_block_len": (ctypes.c_int, [_vp, ctypes.c_int]),
    "d4est_hip_vec_dot": (None, [_vp, ctypes.c_int, _vp, _vp, _vp]),
    "d4est_hip_comm_unique_id_bytes": (ctypes.c_int, []),
    "d4est_hip_comm_get_unique_id": (None, [_vp]),
    "d4est_hip_comm_create": (_vp, [_vp, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_comm_try_create": (_vp, [_vp, ctypes.c_int, ctypes.c_int]),
    "d4est_hip_comm_destroy": (None, [_vp]),
    "d4est_hip_comm_rank": (ctypes.c_int, [_vp]),
    "d4est_hip_comm_size": (ctypes.c_int, [_vp]),
    "d4est_hip_comm_nccl_count": (ctypes.c_int, [_vp]),
    "d4est_hip_plan_set_rccl_exchange": (_vp, [_vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_rccl_exchange_destroy": (None, [_vp]),
    "d4est_hip_rccl_exchange_count": (ctypes.c_longlong, [_vp]),
    "d4est_hip_rccl_exchange_send_doubles": (ctypes.c_longlong, [_vp]),
    "d4est_hip_rccl_exchange_recv_doubles": (ctypes.c_longlong, [_vp]),
    "d4est_hip_comm_sendrecv": (None, [_vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "d4est_hip_comm_allreduce_sum": (None, [_vp, _vp, _vp, ctypes.c_int]),
    "d4est_hip_apply_stiffness_matrix_host": (None, [_vp, _vp, _vp]),
    "d4est_hip_apply_aij_host": (None, [_vp, _vp, _vp]),
    "d4est_hip_apply_lhs_host": (None, [_vp, _vp, _vp]),
    "d4est_hip_cheby_iterate_host": (None, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int]),
    "d4est_hip_cg_eigs_host": (ctypes.c_double, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _c_double_p]),
    "d4est_hip_plan_set_jacobian": (None, [_vp, _vp, ctypes.c_int]),
    "d4est_hip_host_alloc": (_vp, [ctypes.c_size_t]),
    "d4est_hip_host_free": (None, [_vp]),
    "d4est_hip_memcpy_h2d_async": (None, [_vp, _vp, _vp, ctypes.c_size_t]),
    "d4est_hip_memcpy_d2h_async": (None, [_vp, _vp, _vp, ctypes.c_size_t]),
    "d4est_hip_plan_synchronize": (None, [_vp]),
    "d4est_hip_amr_create": (_vp, [ctypes.c_int, _vp, ctypes.c_int, ctypes.c_double]),
    "d4est_hip_amr_destroy": (None, [_vp]),
    "d4est_hip_amr_set_stream": (None, [_vp, _vp]),
    "d4est_hip_amr_n_elements": (ctypes.c_int, [_vp]),
    "d4est_hip_amr_local_nodes": (ctypes.c_longlong, [_vp]),
    "d4est_hip_amr_stats": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_amr_mark_smooth_pred": (None, [_vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "d4est_hip_amr_p_balance": (None, [_vp, _vp, ctypes.c_int]),
    "d4est_hip_amr_get_refinement_log": (None, [_vp, _vp]),
    "d4est_hip_amr_set_refinement_log": (None, [_vp, _vp]),
    "d4est_hip_amr_get_predictor": (None, [_vp, _vp]),
    "d4est_hip_amr_set_balance": (None, [_vp, ctypes.c_int, _vp]),
    "d4est_hip_amr_new_n_elements": (ctypes.c_int, [_vp]),
    "d4est_hip_amr_new_local_nodes": (ctypes.c_longlong, [_vp]),
    "d4est_hip_amr_get_new_degrees": (None, [_vp, _vp]),
    "d4est_hip_amr_interpolate_field": (None, [_vp, _vp, _vp]),
    "d4est_hip_amr_describe": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int]),
    "d4est_hip_amr_advance": (None, [_vp]),
    "d4est_hip_par_amr_set_comm": (None, [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "d4est_hip_par_amr_stats_global": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_par_amr_repartition": (ctypes.c_longlong, [_vp, _vp, _vp]),
    "d4est_hip_par_amr_repartition_field": (None, [_vp, _vp, _vp]),
    "d4est_hip_probe_create": (_vp, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_int]),
    "d4est_hip_probe_destroy": (None, [_vp]),
    "d4est_hip_probe_n_points": (ctypes.c_int, [_vp]),
    "d4est_hip_probe_info": (None, [_vp, _vp, _vp, _vp]),
    "d4est_hip_probe_element_info": (None, [_vp, _vp, _vp]),
    "d4est_hip_probe_eval": (None, [_vp, ctypes.c_int, _vp, ctypes.c_longlong, _vp]),
    "d4est_hip_probe_set_map": (None, [_vp, ctypes.c_int, _vp]),
    "d4est_hip_probe_eval_gradient": (None, [_vp, _vp, _vp, ctypes.c_int]),
    "d4est_hip_probe_xyz": (None, [_vp, _vp]),
    "d4est_hip_field_eval": (None, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_longlong, _vp]),
    "d4est_hip_plan_compute_xyz_brick": (None, [_vp, _vp, _vp, ctypes.c_double, _vp, _vp, _vp]),
    "d4est_hip_plan_set_puncture_term_brick": (None, [_vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_double, _vp]),
    "d4est_hip_plan_set_puncture_term_analytic": (None, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_double]),
    "d4est_hip_plan_set_puncture_term_xyz": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_plan_set_cds_term_brick": (None, [_vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_double, _vp]),
    "d4est_hip_plan_set_cds_term_analytic": (None, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_double]),
    "d4est_hip_plan_set_cds_term_xyz": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_plan_nonlinear_coefficients": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "d4est_hip_plan_set_okendon_term_brick": (None, [_vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_double, _vp]),
    "d4est_hip_plan_set_okendon_term_analytic": (None, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_double]),
    "d4est_hip_plan_set_okendon_term_xyz": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_plan_set_boyen_york_term_brick": (None, [_vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_double, _vp]),
    "d4est_hip_plan_set_boyen_york_term_analytic": (None, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_double]),
    "d4est_hip_plan_set_boyen_york_term_xyz": (None, [_vp, _vp, ctypes.c_int, _vp]),
    "d4est_hip_plan_build_load_by_id_brick": (None, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, ctypes.c_double, _vp, ctypes.c_int, _vp]),
    "d4est_hip_plan_build_load_by_id_analytic": (None, [_vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp,
                                                        ctypes.c_double, ctypes.c_int, _vp]),
    "d4est_hip_plan_build_load_by_id_xyz": (None, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp]),
    "d4est_hip_plan_compute_boundary_xyz_brick": (None, [_vp, _vp, _vp, ctypes.c_double, _vp, _vp]),
    "d4est_hip_plan_compute_boundary_xyz_analytic": (None, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_double, _vp]),
    "d4est_hip_plan_set_robin_by_id_brick": (None, [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_double, _vp]),
    "d4est_hip_plan_set_robin_by_id_analytic": (None, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_double]),
}

# problem fields and Robin callbacks by id (D4EST_HIP_FIELD_* / D4EST_HIP_ROBIN_*)
FIELD = {"PUNCTURE_K2": 0, "PUNCTURE_A": 1, "PUNCTURE_B": 2, "CDS_A": 3, "CDS_PSI": 4, "INV_R": 5, "OKENDON_U": 6, "BY_PSI": 7, "BY_A": 8,
         "LORENTZIAN_U": 9, "LORENTZIAN_RHS": 10, "LORENTZIAN_ROBIN": 11, "STAMM_U": 12, "STAMM_RHS": 13}
ROBIN_COEFF = {"INV_R": 0, "BRICK": 1, "LORENTZIAN": 2}
ROBIN_RHS = {"ZERO": 0, "INV_R": 1}
MAX_PUNCTURES = 10


def puncture_params(C, P, S, M, puncture_eps=1e-15):
    """the flat parameter vector of the puncture fields: {num_punctures, puncture_eps, then per puncture C[3], P[3], S[3], M}"""
    C, P, S = (np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in (C, P, S))
    M = np.asarray(M, dtype=np.float64).reshape(-1)
    n = M.size
    assert C.shape[0] == n and P.shape[0] == n and S.shape[0] == n and 1 <= n < MAX_PUNCTURES
    return np.concatenate([[float(n), float(puncture_eps)], np.concatenate([C, P, S, M[:, None]], axis=1).reshape(-1)])


def okendon_params(p):
    """the parameter vector of OKENDON_U and the Okendon term: {p}, 0 < p < 1"""
    assert 0.0 < float(p) < 1.0
    return np.array([float(p)])


def boyen_york_params(a, P):
    """the parameter vector of BY_PSI, BY_A and the Boyen-York term: {a, P}"""
    return np.array([float(a), float(P)])


def stamm_params(c2x, c2y, c2z):
    """the parameter vector of STAMM_U and STAMM_RHS: {c2x, c2y, c2z}"""
    return np.array([float(c2x), float(c2y), float(c2z)])


def _field_params(field_id, params):
    fid = FIELD[field_id] if isinstance(field_id, str) else int(field_id)
    assert 0 <= fid <= 13, "unknown field id"
    if fid == 5 or 9 <= fid <= 11:
        return fid, np.zeros(1), 0
    pr = np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
    if fid <= 2:
        assert pr.size >= 2 and pr[0] == int(pr[0]) and 1 <= pr[0] < MAX_PUNCTURES and pr.size == 2 + 10 * int(pr[0]), "puncture params"
    elif fid <= 4:
        assert pr.size == 8, "star params: cx, cy, cz, R, rho0, C0, alpha, beta"
    elif fid == 6:
        assert pr.size == 1 and 0.0 < pr[0] < 1.0, "Okendon params: p, 0 < p < 1"
    elif fid <= 8:
        assert pr.size == 2, "Boyen-York params: a, P"
    else:
        assert pr.size == 3, "Stamm params: c2x, c2y, c2z"
    return fid, pr, pr.size


def field_eval(field_id, params, xyz, out, stream=None):
    """out[i] = the problem field `field_id` (capi.FIELD name or id) at the points xyz = x[n] | y[n] | z[n]; float64 CUDA tensors.  One
    thread per point on `stream` (a torch stream or a raw handle; default: torch's current stream), no synchronisation"""
    import torch
    fid, pr, n_params = _field_params(field_id, params)
    n = out.numel()
    assert xyz.numel() == 3 * n
    if stream is None:
        stream = torch.cuda.current_stream(out.device)
    h = getattr(stream, "cuda_stream", stream)
    load_library().d4est_hip_field_eval(ctypes.c_void_p(int(h)), fid, pr.ctypes.data_as(_vp), n_params, _ptr(xyz), n, _ptr(out))

# [mesh_parameters] face_h_type / volume_h_type by the reference's names (d4est_mesh_face_h_t / d4est_mesh_volume_h_t) and the size
# parameter arrays (D4EST_HIP_SIZE_*)
FACE_H = {
    "FACE_H_EQ_J_DIV_SJ_QUAD": 0, "FACE_H_EQ_J_DIV_SJ_MIN_LOBATTO": 1, "FACE_H_EQ_J_DIV_SJ_MEAN_LOBATTO": 2,
    "FACE_H_EQ_J_DIV_SJ_MAX_LOBATTO": 3, "FACE_H_EQ_TREE_H": 4, "FACE_H_EQ_VOLUME_DIV_AREA": 5, "FACE_H_EQ_FACE_DIAM": 6,
    "FACE_H_EQ_TOTAL_VOLUME_DIV_TOTAL_AREA": 7,
}
VOL_H = {"VOL_H_EQ_DIAM": 0, "VOL_H_EQ_CUBE_APPROX": 1}
SIZE_PARAMETER = {"diam_volume": 0, "volume": 1, "area": 2, "diam_face": 3, "j_div_sj_min": 4, "j_div_sj_mean": 5, "j_div_sj_max": 6}

TABLE = {
    "lobatto_nodes": 0, "lobatto_weights": 1, "gauss_nodes": 2, "gauss_weights": 3,
    "dij": 4, "mij": 5, "invmij": 6, "lobatto_to_gauss": 7,
    "p_prolong": 8, "hp_prolong": 9, "p_restrict": 10, "hp_restrict": 11,
}

_lib = None


def load_library(path=None):
    """Load libd4est_hip.so and attach the signatures.  Fails loudly when absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # D4EST_HIP_LIBRARY: another build of the same library (kernel experiments: tools/build_variant.sh)
    p = path or os.environ.get("D4EST_HIP_LIBRARY") or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            "libd4est_hip.so not found at %s -- build it with `python -m disco4est_amd.build` "
            "(or __graft_entry__.build()); there is no CPU fallback" % p)
    # Load order matters in a process that also uses torch: torch ships its own HIP runtime under the same soname as /opt/rocm's.
    # Whichever is mapped first serves both; torch aborts on the system one, while this library runs on either.  So torch goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def table(name, deg_a, deg_b=0):
    """1-D operator table as a numpy array (host-side, no GPU needed)."""
    lib = load_library()
    tid = TABLE[name]
    n = lib.d4est_hip_table(tid, int(deg_a), int(deg_b), None)
    out = np.empty(n, dtype=np.float64)
    lib.d4est_hip_table(tid, int(deg_a), int(deg_b), out.ctypes.data_as(_c_double_p))
    return out


def tree_map(geom_type, params, tree, xi):
    """the library's analytic tree map evaluated on the HOST (d4est_hip_tree_map; no GPU needed): xi[n, 3] tree coordinates ->
    (status, x[n, 3], dxdxi[n, 3, 3]); status is the first non-zero return code (unknown type, rejected flag, tree out of range) or 0"""
    lib = load_library()
    pr = np.zeros(5)
    pv = np.asarray(params, dtype=np.float64).reshape(-1)
    pr[:pv.size] = pv
    xi = np.ascontiguousarray(np.asarray(xi, dtype=np.float64).reshape(-1, 3))
    X = np.full((xi.shape[0], 3), np.nan)
    D = np.full((xi.shape[0], 3, 3), np.nan)
    for k in range(xi.shape[0]):
        rc = lib.d4est_hip_tree_map(int(geom_type), pr.ctypes.data_as(_vp), int(tree), xi[k].ctypes.data_as(_vp),
                                    X[k].ctypes.data_as(_vp), D[k].ctypes.data_as(_vp))
        if rc:
            return rc, X, D
    return 0, X, D


def tree_map_d2(geom_type, params, tree, xi):
    """the second derivatives of the library's analytic tree map on the HOST (d4est_hip_tree_map_d2; no GPU needed): xi[n, 3] ->
    (status, d2[n, 3, 3, 3]) with d2[n, i, j, k] = d^2 x_i / d xi_j d xi_k; status as tree_map's"""
    lib = load_library()
    pr = np.zeros(5)
    pv = np.asarray(params, dtype=np.float64).reshape(-1)
    pr[:pv.size] = pv
    xi = np.ascontiguousarray(np.asarray(xi, dtype=np.float64).reshape(-1, 3))
    H = np.full((xi.shape[0], 3, 3, 3), np.nan)
    for k in range(xi.shape[0]):
        rc = lib.d4est_hip_tree_map_d2(int(geom_type), pr.ctypes.data_as(_vp), int(tree), xi[k].ctypes.data_as(_vp), H[k].ctypes.data_as(_vp))
        if rc:
            return rc, H
    return 0, H


def _ptr(t):
    """Device pointer of a contiguous float64 torch CUDA tensor."""
    import torch
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous(), \
        "expected a contiguous float64 CUDA tensor"
    return ctypes.c_void_p(t.data_ptr())


def _iarr(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_c_int_p)


class Plan:
    """Host mirror of a d4est mesh level: element arrays + geometric factors on the device.

    Argument meaning follows d4est_element_data_t (src/Mesh/d4est_element_data.h:13-48) and
    d4est_mesh_data_t (src/Mesh/d4est_mesh.h:123-169) of the reference.
    """

    def __init__(self, deg, deg_quad, nodal_stride, quad_stride, quad_type=0, stream=None):
        self.lib = load_library()
        self._keep = [_iarr(deg), _iarr(deg_quad), _iarr(nodal_stride), _iarr(quad_stride)]
        n = len(self._keep[0][0])
        self.handle = self.lib.d4est_hip_plan_create(n, self._keep[0][1], self._keep[1][1], self._keep[2][1],
                                                     self._keep[3][1], int(quad_type))
        self.n_elements = n
        self.torch_stream = None
        self.local_nodes = self.lib.d4est_hip_plan_local_nodes(self.handle)
        self.local_nodes_quad = self.lib.d4est_hip_plan_local_nodes_quad(self.handle)
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        """stream: a torch.cuda.Stream (its raw hipStream_t is passed through) or an int handle."""
        h = getattr(stream, "cuda_stream", stream)
        self.torch_stream = stream if hasattr(stream, "cuda_stream") else None   # parallel.attach makes it current around the exchange
        self._stream_handle = int(h)   # the raw hipStream_t, for calls outside the plan that must be ordered with it (field_eval)
        self.lib.d4est_hip_plan_set_stream(self.handle, ctypes.c_void_p(int(h)))

    def last_kernel(self):
        return self.lib.d4est_hip_plan_last_kernel(self.handle).decode()

    def face_path(self):
        """which face kernels the full operator runs on this plan: 'direct', 'direct+volume', 'two-phase' or 'hybrid...: direct+volume on C
        clean elements, two-phase on D' -- on a plan with ghost sides under set_tuning(14, 2): '... on C clean elements (G beside ghost
        sides), two-phase on D'."""
        return self.lib.d4est_hip_plan_face_path(self.handle).decode()

    def stream_mode(self):
        """1 when the large-plan kernels move once-touched data with the non-temporal hint (tuning key 12; automatic from 320 MB per apply)."""
        return self.lib.d4est_hip_plan_stream_mode(self.handle)

    def set_tuning(self, key, value):
        self.lib.d4est_hip_plan_set_tuning(self.handle, int(key), int(value))

    def set_geometry(self, J_quad, rst_xyz_quad):
        """J_quad[local_nodes_quad], rst_xyz_quad[9*local_nodes_quad] (reference SoA layout);
        numpy arrays (host) or torch CUDA tensors (device)."""
        if isinstance(J_quad, np.ndarray):
            J = np.ascontiguousarray(J_quad, dtype=np.float64)
            R = np.ascontiguousarray(rst_xyz_quad, dtype=np.float64).reshape(-1)
            assert J.size == self.local_nodes_quad and R.size == 9 * self.local_nodes_quad
            self.lib.d4est_hip_plan_set_geometry(self.handle, J.ctypes.data_as(_vp), R.ctypes.data_as(_vp), 0)
        else:
            assert J_quad.numel() == self.local_nodes_quad and rst_xyz_quad.numel() == 9 * self.local_nodes_quad
            self.lib.d4est_hip_plan_set_geometry(self.handle, _ptr(J_quad), _ptr(rst_xyz_quad), 1)

    def set_geometry_numerical(self, xyz_lobatto):
        """GEOM_COMPUTE_NUMERICAL volume factors from the nodal coordinates: xyz_lobatto = (x, y, z) arrays of local_nodes entries
        (numpy) or one torch CUDA tensor of 3*local_nodes entries"""
        if isinstance(xyz_lobatto, (list, tuple)) or isinstance(xyz_lobatto, np.ndarray):
            X = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in xyz_lobatto]))
            assert X.size == 3 * self.local_nodes
            self.lib.d4est_hip_plan_set_geometry_numerical(self.handle, X.ctypes.data_as(_vp), 0)
        else:
            assert xyz_lobatto.numel() == 3 * self.local_nodes
            self.lib.d4est_hip_plan_set_geometry_numerical(self.handle, _ptr(xyz_lobatto), 1)

    def apply_stiffness_matrix(self, u, Au):
        assert u.numel() == self.local_nodes and Au.numel() == self.local_nodes
        self.lib.d4est_hip_apply_stiffness_matrix(self.handle, _ptr(u), _ptr(Au))

    def apply_mass_matrix(self, u, Mu):
        assert u.numel() == self.local_nodes and Mu.numel() == self.local_nodes
        self.lib.d4est_hip_apply_mass_matrix(self.handle, _ptr(u), _ptr(Mu))

    def apply_galerkin_integral(self, f_quad, out):
        assert f_quad.numel() == self.local_nodes_quad and out.numel() == self.local_nodes
        self.lib.d4est_hip_apply_galerkin_integral(self.handle, _ptr(f_quad), _ptr(out))

    def interpolate(self, u, u_quad):
        assert u.numel() == self.local_nodes and u_quad.numel() == self.local_nodes_quad
        self.lib.d4est_hip_interpolate(self.handle, _ptr(u), _ptr(u_quad))

    def set_geometry_brick(self, elem_dq, root_len, extents, mortars=False):
        """device-generated factors of the reference's brick geometry (volume, or the mortars when mortars=True)"""
        dq = _iarr(elem_dq)
        ex = np.ascontiguousarray(extents, dtype=np.float64)
        fn = self.lib.d4est_hip_plan_set_mortar_geometry_brick if mortars else self.lib.d4est_hip_plan_set_geometry_brick
        fn(self.handle, dq[1], float(root_len), ex.ctypes.data_as(_vp))

    def set_geometry_analytic(self, geom_type, params, tree, q, dq, root_len, mortars=False, ghost=None):
        """factors of an analytic tree map generated on the device (geom_type 1 = cubed_sphere_7tree, params = (R0, R1,
        compactify_inner_shell); 2 = cubed_sphere, 3 = cubed_sphere_with_sphere_hole, 4 = cubed_sphere_with_cube_hole, params = (R0, R1,
        R2, compactify_outer_shell, compactify_inner_shell), e.g. forest.CubedSphere13Map(...).params); tree / q[n,3] / dq: where every element sits in the forest; mortars=True: the mortar factors
        (ghost = (tree, q, dq) of the ghost elements)"""
        pr = np.ascontiguousarray(params, dtype=np.float64)
        t, qq, d = _iarr(tree), _iarr(np.asarray(q).reshape(-1)), _iarr(dq)
        if not mortars:
            self.lib.d4est_hip_plan_set_geometry_analytic(self.handle, int(geom_type), pr.ctypes.data_as(_vp), t[1], qq[1], d[1], float(root_len))
            return
        gt, gq, gd = (_iarr(ghost[0]), _iarr(np.asarray(ghost[1]).reshape(-1)), _iarr(ghost[2])) if ghost is not None else \
            (_iarr(np.zeros(0)), _iarr(np.zeros(0)), _iarr(np.zeros(0)))
        self.lib.d4est_hip_plan_set_mortar_geometry_analytic(self.handle, int(geom_type), pr.ctypes.data_as(_vp), t[1], qq[1], d[1],
                                                             gt[1], gq[1], gd[1], float(root_len))

    def compute_xyz_analytic(self, geom_type, params, tree, q, dq, root_len, xyz_lobatto=None, xyz_quad=None):
        """node coordinates of an analytic tree map on the device: xyz_lobatto (3 * local_nodes, x | y | z at the Lobatto nodes) and /
        or xyz_quad (3 * local_nodes_quad, at the quadrature nodes); float64 CUDA tensors, either may be None.  Stream-ordered."""
        pr = np.zeros(5)
        pv = np.asarray(params, dtype=np.float64).reshape(-1)
        pr[:pv.size] = pv
        t, qq, d = _iarr(tree), _iarr(np.asarray(q).reshape(-1)), _iarr(dq)
        assert len(t[0]) == self.n_elements and len(d[0]) == self.n_elements and len(qq[0]) == 3 * self.n_elements
        assert xyz_lobatto is None or xyz_lobatto.numel() >= 3 * self.local_nodes
        assert xyz_quad is None or xyz_quad.numel() >= 3 * self.local_nodes_quad
        self.lib.d4est_hip_plan_compute_xyz_analytic(self.handle, int(geom_type), pr.ctypes.data_as(_vp), t[1], qq[1], d[1], float(root_len),
                                                     _ptr(xyz_lobatto) if xyz_lobatto is not None else None,
                                                     _ptr(xyz_quad) if xyz_quad is not None else None)

    # ---- element size parameters (csrc/d4est_hip_sizes.hip) ----
    def set_h_types(self, face_h_type=0, volume_h_type=0):
        """[mesh_parameters] face_h_type / volume_h_type: ids or the reference's names (capi.FACE_H / capi.VOL_H); before set_faces"""
        f = FACE_H[face_h_type] if isinstance(face_h_type, str) else int(face_h_type)
        v = VOL_H[volume_h_type] if isinstance(volume_h_type, str) else int(volume_h_type)
        self.lib.d4est_hip_plan_set_h_types(self.handle, f, v)

    def compute_size_parameters(self, brick=None, analytic=None):
        """d4est_mesh_init_element_size_parameters on the device, stream-ordered.  brick = (elem_dq, root_len, extents[, ghost_dq]) or
        analytic = (geom_type, params, tree, q, dq, root_len[, ghost]) with ghost = (tree, q, dq) of the ghost elements or None, as
        set_faces takes them; ghost elements need set_faces first.  The arrays: size_parameter(name)"""
        assert (brick is None) != (analytic is None), "one of brick / analytic"
        if brick is not None:
            dq = _iarr(brick[0])
            ex = np.ascontiguousarray(brick[2], dtype=np.float64)
            gdq = _iarr(brick[3]) if len(brick) > 3 and brick[3] is not None else None
            assert len(dq[0]) == self.n_elements
            self.lib.d4est_hip_plan_compute_size_parameters_brick(self.handle, dq[1], gdq[1] if gdq else None, float(brick[1]),
                                                                  ex.ctypes.data_as(_vp))
            return
        geom_type, params, tree, q, dq, root_len = analytic[:6]
        ghost = analytic[6] if len(analytic) > 6 else None
        pr = np.zeros(5)
        pv = np.asarray(params, dtype=np.float64).reshape(-1)
        pr[:pv.size] = pv
        t, qq, d = _iarr(tree), _iarr(np.asarray(q).reshape(-1)), _iarr(dq)
        assert len(t[0]) == self.n_elements and len(d[0]) == self.n_elements and len(qq[0]) == 3 * self.n_elements
        g = (_iarr(ghost[0]), _iarr(np.asarray(ghost[1]).reshape(-1)), _iarr(ghost[2])) if ghost is not None else None
        self.lib.d4est_hip_plan_compute_size_parameters_analytic(self.handle, int(geom_type), pr.ctypes.data_as(_vp), t[1], qq[1], d[1],
                                                                 g[0][1] if g else None, g[1][1] if g else None, g[2][1] if g else None,
                                                                 float(root_len))

    def compute_diameters(self, xyz):
        """diam_volume and diam_face of the local elements from their node coordinates alone: xyz = one float64 CUDA tensor of
        3 * local_nodes entries, x | y | z at the Lobatto nodes (any geometry).  Stream-ordered."""
        assert xyz.numel() == 3 * self.local_nodes
        self.lib.d4est_hip_plan_compute_diameters(self.handle, _ptr(xyz))

    def size_parameter(self, name, device=None):
        """the plan-owned array `name` (capi.SIZE_PARAMETER: diam_volume, volume: one per element; area, diam_face, j_div_sj_min / _mean /
        _max: six per element; ghost elements after the local ones) as a torch tensor VIEW of the plan's memory -- valid while the plan
        lives, overwritten by the next compute_* call; None when it has not been computed"""
        import torch
        ptr, cnt = ctypes.c_void_p(), ctypes.c_longlong()
        if not self.lib.d4est_hip_plan_size_parameter(self.handle, SIZE_PARAMETER[name] if isinstance(name, str) else int(name),
                                                      ctypes.byref(ptr), ctypes.byref(cnt)):
            return None
        n = int(cnt.value)
        dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        if n == 0:
            return torch.empty(0, dtype=torch.float64, device=dev)

        class _View:   # the CUDA array interface: torch.as_tensor wraps the memory without copying
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (int(ptr.value), False), "version": 2, "strides": None}

        t = torch.as_tensor(_View(), device=dev)
        t._d4est_hip_plan = self   # (the view keeps the plan object alive)
        return t

    def apply_weighted_mass_matrix(self, u, coeff_quad, out):
        assert u.numel() == self.local_nodes and out.numel() == self.local_nodes
        assert coeff_quad.numel() == self.local_nodes_quad
        self.lib.d4est_hip_apply_weighted_mass_matrix(self.handle, _ptr(u), _ptr(coeff_quad), _ptr(out))

    def apply_inverse_mass_matrix(self, x, out):
        assert x.numel() == self.local_nodes and out.numel() == self.local_nodes
        self.lib.d4est_hip_apply_inverse_mass_matrix(self.handle, _ptr(x), _ptr(out))

    def apply_mij(self, x, out):
        assert x.numel() == self.local_nodes and out.numel() == self.local_nodes
        self.lib.d4est_hip_apply_mij(self.handle, _ptr(x), _ptr(out))

    def apply_invmij(self, x, out):
        assert x.numel() == self.local_nodes and out.numel() == self.local_nodes
        self.lib.d4est_hip_apply_invmij(self.handle, _ptr(x), _ptr(out))

    def apply_slicer(self, x, face, out_face):
        assert x.numel() == self.local_nodes and out_face.numel() == self.lib.d4est_hip_plan_face_nodes(self.handle)
        self.lib.d4est_hip_apply_slicer(self.handle, _ptr(x), int(face), _ptr(out_face))

    def apply_lift(self, x_face, face, out):
        assert out.numel() == self.local_nodes and x_face.numel() == self.lib.d4est_hip_plan_face_nodes(self.handle)
        self.lib.d4est_hip_apply_lift(self.handle, _ptr(x_face), int(face), _ptr(out))

    def apply_dij(self, x, direction, out, transpose=False):
        assert x.numel() == self.local_nodes and out.numel() == self.local_nodes
        fn = self.lib.d4est_hip_apply_dij_transpose if transpose else self.lib.d4est_hip_apply_dij
        fn(self.handle, _ptr(x), int(direction), _ptr(out))

    def compute_dudr(self, u, d0, d1, d2):
        for t in (u, d0, d1, d2):
            assert t.numel() == self.local_nodes
        self.lib.d4est_hip_compute_dudr(self.handle, _ptr(u), _ptr(d0), _ptr(d1), _ptr(d2))

    # ---- faces
    def set_faces(self, sides, penalty_prefactor=10.0, penalty_fcn=0, brick=None, analytic=None):
        """sides: the dict of mesh.BrickMesh.build_sides() (reference-layout side list + mortar factors);
        brick = (elem_dq, root_len, extents): generate the mortar factors of the brick geometry on the device instead"""
        keep = [_iarr(sides[k]) for k in ("side_nbr", "side_nbr_face", "side_reorder", "side_mortar_stride", "side_bndry_stride",
                                         "ghost_deg", "ghost_deg_quad")]
        self._keep_sides = keep
        self.total_mortar_nodes = int(sides["total_mortar_nodes"])
        if "side_hang" in sides and np.any(np.asarray(sides["side_hang"]) != 0):
            hk = [_iarr(sides[k]) for k in ("side_hang", "side_sub", "side_nbr4", "side_orientation")]
            self._keep_hang = hk
            self.lib.d4est_hip_plan_set_hanging(self.handle, hk[0][1], hk[1][1], hk[2][1], hk[3][1])
        self.lib.d4est_hip_plan_set_faces(self.handle, keep[0][1], keep[1][1], keep[2][1], keep[3][1], keep[4][1],
                                          int(sides["total_mortar_nodes"]), int(sides["total_bndry_nodes"]),
                                          len(keep[5][0]), keep[5][1], keep[6][1])
        self.lib.d4est_hip_plan_set_sipg(self.handle, float(penalty_prefactor), int(penalty_fcn))
        if brick is not None:
            self.set_geometry_brick(brick[0], brick[1], brick[2], mortars=True)
        elif analytic is not None:      # (geom_type, params, tree, q, dq, root_len, ghost)
            self.set_geometry_analytic(*analytic[:6], mortars=True, ghost=analytic[6])
        else:
            arrs = [np.ascontiguousarray(sides[k], dtype=np.float64) for k in ("sj", "n", "drst_m", "drst_p", "hm", "hp")]
            self.lib.d4est_hip_plan_set_mortar_geometry(self.handle, *[a.ctypes.data_as(_vp) for a in arrs], 0)
        self.trace_size = self.lib.d4est_hip_plan_trace_size(self.handle)
        self.ghost_trace_size = self.lib.d4est_hip_plan_ghost_trace_size(self.handle)

    def set_estimator(self, gradu_fcn, u_fcn, u_dirichlet_fcn, penalty_prefactor):
        """request the a-posteriori error estimator (d4est_estimator_bi) with these penalty function ids (include/d4est_hip.h,
        D4EST_HIP_EST_*); before set_faces (whose mortar factors also form the estimator's)"""
        self.lib.d4est_hip_plan_set_estimator(self.handle, int(gradu_fcn), int(u_fcn), int(u_dirichlet_fcn), float(penalty_prefactor))

    # ---- the Laplacian at the quadrature nodes (csrc/d4est_hip_hessian.hip) ----
    def set_hessian_brick(self, elem_dq, root_len, extents):
        """Hessian-trace coefficients of the brick geometry (arguments as set_geometry_brick)"""
        dq = _iarr(elem_dq)
        ex = np.ascontiguousarray(extents, dtype=np.float64)
        assert len(dq[0]) == self.n_elements and ex.size == 6
        self.lib.d4est_hip_plan_set_hessian_brick(self.handle, dq[1], float(root_len), ex.ctypes.data_as(_vp))

    def set_hessian_analytic(self, geom_type, params, tree, q, dq, root_len):
        """Hessian-trace coefficients of an analytic tree map, HESSIAN_ANALYTICAL (arguments as set_geometry_analytic)"""
        pr = np.zeros(5)
        pv = np.asarray(params, dtype=np.float64).reshape(-1)
        pr[:pv.size] = pv
        t, qq, d = _iarr(tree), _iarr(np.asarray(q).reshape(-1)), _iarr(dq)
        assert len(t[0]) == self.n_elements and len(d[0]) == self.n_elements and len(qq[0]) == 3 * self.n_elements
        self.lib.d4est_hip_plan_set_hessian_analytic(self.handle, int(geom_type), pr.ctypes.data_as(_vp), t[1], qq[1], d[1], float(root_len))

    def set_hessian_numerical(self, xyz_lobatto, rst_xyz_quad=None):
        """Hessian-trace coefficients from the node coordinates, HESSIAN_NUMERICAL: xyz_lobatto = (x, y, z) numpy arrays or one CUDA
        tensor of 3 local_nodes; rst_xyz_quad (9 local_nodes_quad, reference SoA layout; the same kind of array) or None = dr/dx
        from the coordinates as set_geometry_numerical forms it"""
        if isinstance(xyz_lobatto, (list, tuple, np.ndarray)):
            X = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in xyz_lobatto]))
            R = None if rst_xyz_quad is None else np.ascontiguousarray(rst_xyz_quad, dtype=np.float64).reshape(-1)
            assert X.size == 3 * self.local_nodes and (R is None or R.size == 9 * self.local_nodes_quad)
            self.lib.d4est_hip_plan_set_hessian_numerical(self.handle, X.ctypes.data_as(_vp), R.ctypes.data_as(_vp) if R is not None else None, 0)
        else:
            assert xyz_lobatto.numel() == 3 * self.local_nodes and (rst_xyz_quad is None or rst_xyz_quad.numel() == 9 * self.local_nodes_quad)
            self.lib.d4est_hip_plan_set_hessian_numerical(self.handle, _ptr(xyz_lobatto),
                                                          _ptr(rst_xyz_quad) if rst_xyz_quad is not None else None, 1)

    def hessian_info(self):
        """0 none, 1 brick, 2 analytic, 3 numerical"""
        return self.lib.d4est_hip_plan_hessian_info(self.handle)

    def hessian_supported(self):
        """True when every (deg, deg_quad) bucket fits the LDS of the hessian_trace kernel (include/d4est_hip.h)"""
        return bool(self.lib.d4est_hip_plan_hessian_supported(self.handle))

    def hessian_trace(self, u, out):
        """out[local_nodes_quad] = the Laplacian of u[local_nodes] at the quadrature nodes (CUDA tensors; out is overwritten)"""
        assert u.numel() == self.local_nodes and out.numel() == self.local_nodes_quad
        self.lib.d4est_hip_hessian_trace(self.handle, _ptr(u), _ptr(out))

    def estimator_bi_pointwise(self, u, residual_quad, diam, eta2, terms=None, ghost_trace=None, g=None):
        """estimator_bi with the pointwise residual (d4est_estimator_bi_new_compute, use_pointwise_residual): residual_quad holds
        local_nodes_quad values at the quadrature nodes; everything else as estimator_bi"""
        self._estimator(self.lib.d4est_hip_estimator_bi_pointwise, self.local_nodes_quad, u, residual_quad, diam, eta2, terms, ghost_trace, g)

    def estimator_bi(self, u, residual, diam, eta2, terms=None, ghost_trace=None, g=None):
        """eta2[n_elements] (and terms[4 n_elements], term-major) of d4est_estimator_bi_compute.  u, residual: CUDA tensors of
        local_nodes doubles; eta2 / terms / ghost_trace: CUDA tensors; diam (n_elements) and g (Dirichlet data on the boundary Lobatto
        face nodes, set_dirichlet_values' layout; None = 0): numpy arrays or CUDA tensors; diam None: the plan's own diam_volume
        (compute_size_parameters / compute_diameters)"""
        self._estimator(self.lib.d4est_hip_estimator_bi, self.local_nodes, u, residual, diam, eta2, terms, ghost_trace, g)

    def _estimator(self, fn, n_residual, u, residual, diam, eta2, terms, ghost_trace, g):
        import torch
        assert u.numel() == self.local_nodes and residual.numel() == n_residual
        assert eta2.numel() == self.n_elements and (terms is None or terms.numel() == 4 * self.n_elements)
        dev = u.device

        def on_dev(a):
            if a is None or isinstance(a, torch.Tensor):
                return a
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)

        d_diam, d_g = on_dev(diam), on_dev(g)   # diam None: the plan's own diam_volume (compute_size_parameters / compute_diameters)
        assert d_diam is None or d_diam.numel() == self.n_elements
        if ghost_trace is not None:
            assert ghost_trace.numel() == self.ghost_trace_size
        fn(self.handle, _ptr(u), _ptr(ghost_trace) if ghost_trace is not None else None, _ptr(residual),
           _ptr(d_diam) if d_diam is not None else None, _ptr(d_g) if d_g is not None else None, _ptr(eta2),
           _ptr(terms) if terms is not None else None)
        if (diam is not None and not isinstance(diam, torch.Tensor)) or (g is not None and not isinstance(g, torch.Tensor)):
            torch.cuda.current_stream(dev).synchronize() if self.torch_stream is None else self.torch_stream.synchronize()
            self.lib.d4est_hip_device_synchronize()   # (the uploaded copies must outlive the launches)

    # ---- error norms (d4est_norms_save's columns; csrc/d4est_hip_norms.hip) ----
    def set_energy_norm(self, penalty_fcn, penalty_prefactor):
        """request the IP energy norm (d4est_ip_energy_norm_compute) with u_penalty_fcn = this SIPG penalty id (0..3, as set_faces') and
        this prefactor; before set_faces (whose mortar factors also form the norm's face factor)"""
        self.lib.d4est_hip_plan_set_energy_norm(self.handle, int(penalty_fcn), float(penalty_prefactor))

    def _skip_mask(self, skip, dev):
        """None, or the int32 CUDA tensor of a skip mask given as numpy / torch (1 = skip the element)"""
        import torch
        if skip is None:
            return None
        if isinstance(skip, torch.Tensor):
            d = skip.to(device=dev, dtype=torch.int32).contiguous()
        else:
            d = torch.from_numpy(np.ascontiguousarray(skip, dtype=np.int32)).to(dev)
        assert d.numel() == self.n_elements
        return d

    @staticmethod
    def _iptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def _sync_after_upload(self, uploaded, dev):
        import torch
        if uploaded:   # (the uploaded copy must outlive the launches)
            torch.cuda.current_stream(dev).synchronize() if self.torch_stream is None else self.torch_stream.synchronize()
            self.lib.d4est_hip_device_synchronize()

    def norms_error(self, u, u_compare, err):
        """err = |u - u_compare| at the Lobatto nodes (u_compare None: |u|); CUDA tensors of local_nodes doubles"""
        assert u.numel() == self.local_nodes and err.numel() == self.local_nodes
        assert u_compare is None or u_compare.numel() == self.local_nodes
        self.lib.d4est_hip_norms_error(self.handle, _ptr(u), _ptr(u_compare) if u_compare is not None else None, _ptr(err))

    def norm_l2_sqr(self, v, out, skip=None, l2_array=None):
        """out[0] = sum over the non-skipped elements of v_e^T M_e v_e; l2_array[n_elements] (optional) gets every element's value.
        v, out, l2_array: CUDA tensors; skip: numpy or torch mask, 1 = skip"""
        assert v.numel() == self.local_nodes and out.numel() >= 1 and (l2_array is None or l2_array.numel() == self.n_elements)
        d_skip = self._skip_mask(skip, v.device)
        self.lib.d4est_hip_norm_l2_sqr(self.handle, _ptr(v), self._iptr(d_skip), _ptr(l2_array) if l2_array is not None else None, _ptr(out))
        self._sync_after_upload(d_skip is not None and d_skip is not skip, v.device)

    def norm_linfty(self, v, out, skip=None):
        """out[0] = max(0, max_i v_i) over the nodes of the non-skipped elements (d4est_norms_fcn_Linfty)"""
        assert v.numel() == self.local_nodes and out.numel() >= 1
        d_skip = self._skip_mask(skip, v.device)
        self.lib.d4est_hip_norm_linfty(self.handle, _ptr(v), self._iptr(d_skip), _ptr(out))
        self._sync_after_upload(d_skip is not None and d_skip is not skip, v.device)

    def ip_energy_norm_sqr(self, v, sums, elem_terms=None, ghost_trace=None):
        """sums[4] = volume, boundary, interface terms and their total of d4est_ip_energy_norm_compute (squared, this rank's part);
        elem_terms[3 n_elements] (optional), term-major.  CUDA tensors; needs set_energy_norm before set_faces"""
        assert v.numel() == self.local_nodes and sums.numel() == 4 and (elem_terms is None or elem_terms.numel() == 3 * self.n_elements)
        if ghost_trace is not None:
            assert ghost_trace.numel() == self.ghost_trace_size
        self.lib.d4est_hip_ip_energy_norm_sqr(self.handle, _ptr(v), _ptr(ghost_trace) if ghost_trace is not None else None,
                                              _ptr(elem_terms) if elem_terms is not None else None, _ptr(sums))

    def masked_sum(self, elem, out, skip=None):
        """out[0] = fixed-order sum of elem[n_elements] over the non-skipped elements (with eta2: d4est_norms_fcn_energy_estimator)"""
        assert elem.numel() == self.n_elements and out.numel() >= 1
        d_skip = self._skip_mask(skip, elem.device)
        self.lib.d4est_hip_masked_sum(self.handle, _ptr(elem), self._iptr(d_skip), _ptr(out))
        self._sync_after_upload(d_skip is not None and d_skip is not skip, elem.device)

    def boundary_gather(self, vol, out):
        """out[bndry_nodes] = the volume field vol (local_nodes) on the Lobatto nodes of every boundary face, in the order
        set_dirichlet_values expects (e.g. one component of compute_xyz_analytic's xyz_lobatto at a time)"""
        assert vol.numel() == self.local_nodes and out.numel() == self.lib.d4est_hip_plan_bndry_nodes(self.handle)
        self.lib.d4est_hip_plan_boundary_gather(self.handle, _ptr(vol), _ptr(out))

    def set_dirichlet_values(self, g):
        if g is None:
            self.lib.d4est_hip_plan_set_dirichlet_values(self.handle, None, 0)
        elif not isinstance(g, np.ndarray) and hasattr(g, "data_ptr"):      # a float64 CUDA tensor
            assert g.numel() == self.lib.d4est_hip_plan_bndry_nodes(self.handle)
            self.lib.d4est_hip_plan_set_dirichlet_values(self.handle, _ptr(g), 1)
        else:
            g = np.ascontiguousarray(g, dtype=np.float64)
            self.lib.d4est_hip_plan_set_dirichlet_values(self.handle, g.ctypes.data_as(_vp), 0)

    def set_robin_values(self, coeff_quad, rhs_quad):
        """Robin data at the boundary sides' mortar quadrature nodes (indexed like sj); None switches back to Dirichlet"""
        if coeff_quad is None:
            self.lib.d4est_hip_plan_set_robin_values(self.handle, None, None, 0)
            return
        c = np.ascontiguousarray(coeff_quad, dtype=np.float64)
        r = np.ascontiguousarray(rhs_quad, dtype=np.float64)
        self.lib.d4est_hip_plan_set_robin_values(self.handle, c.ctypes.data_as(_vp), r.ctypes.data_as(_vp), 0)

    def compute_ghost_traces(self, u_ghost, ghost_trace):
        assert ghost_trace.numel() == self.ghost_trace_size
        self.lib.d4est_hip_compute_ghost_traces(self.handle, _ptr(u_ghost), _ptr(ghost_trace))

    def compute_face_traces(self, u, trace):
        assert u.numel() == self.local_nodes and trace.numel() == self.trace_size
        self.lib.d4est_hip_compute_face_traces(self.handle, _ptr(u), _ptr(trace))

    def apply_flux(self, trace, ghost_trace, Au):
        self.lib.d4est_hip_apply_flux(self.handle, _ptr(trace), _ptr(ghost_trace) if ghost_trace is not None else None, _ptr(Au))

    def apply_aij(self, u, Au, ghost_trace=None):
        assert u.numel() == self.local_nodes and Au.numel() == self.local_nodes
        self.lib.d4est_hip_apply_aij(self.handle, _ptr(u), _ptr(ghost_trace) if ghost_trace is not None else None, _ptr(Au))

    # ---- smoother loops
    EXCHANGE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
    ALLREDUCE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int)

    def set_comm(self, exchange=None, allreduce=None):
        """exchange(phase, trace_ptr, ghost_trace_ptr), allreduce(scalars_ptr, n): python callables (pointers are ints)"""
        def guarded(fn):
            # ctypes prints and DROPS an exception raised inside a callback; the C caller would carry on with a stale ghost trace
            # or un-reduced scalars.  A failed exchange aborts the process, like every other failure of the library (D4EST_HIP_ABORT).
            def call(*args):
                try:
                    fn(*args)
                except BaseException:
                    import os
                    import sys
                    import traceback
                    sys.stderr.write("[D4EST_HIP_ABORT] exception in a communication callback:\n")
                    traceback.print_exc()
                    sys.stderr.flush()
                    os.abort()
            return call

        self._cb_ex = self.EXCHANGE_FN(guarded(lambda ctx, ph, a, b: exchange(ph, a, b))) if exchange else None
        self._cb_ar = self.ALLREDUCE_FN(guarded(lambda ctx, p, n: allreduce(p, n))) if allreduce else None
        self.lib.d4est_hip_plan_set_comm(self.handle, ctypes.cast(self._cb_ex, ctypes.c_void_p) if self._cb_ex else None,
                                         ctypes.cast(self._cb_ar, ctypes.c_void_p) if self._cb_ar else None, None)

    def build_rhs_with_strong_bc(self, f, rhs, f_on_quad=False):
        """rhs = M f - A(0) with the boundary data currently set on the plan (d4est_laplacian_build_rhs_with_strong_bc)"""
        self.lib.d4est_hip_build_rhs_with_strong_bc(self.handle, _ptr(f), int(bool(f_on_quad)), _ptr(rhs))

    def set_lhs_coefficient(self, coeff_quad):
        """zeroth-order term of apply_lhs (+ V^T W J c V u): a float64 CUDA tensor of local_nodes_quad entries, or None for the pure
        Laplacian.  The VALUES ARE CAPTURED by this call (a plan-owned copy; the tensor is not read afterwards): call it again after
        every change of u0.  The tensor must be complete on the plan's stream (or the device synchronised) when this is called."""
        self._lhs_coeff = coeff_quad
        if coeff_quad is not None:
            assert coeff_quad.numel() == self.local_nodes_quad
        self.lib.d4est_hip_plan_set_lhs_coefficient(self.handle, _ptr(coeff_quad) if coeff_quad is not None else None)

    # ---- the multigrid matrix operator: the zeroth-order term on coarse levels (d4est_solver_multigrid_matrix_operator.c)
    def matrix_nodes(self):
        """d4est_mesh_get_local_matrix_nodes: sum of (deg+1)^6"""
        return self.lib.d4est_hip_plan_matrix_nodes(self.handle)

    def compute_weighted_mass_blocks(self, coeff_quad, blocks):
        """QUAD_COMPUTE_MATRIX for every element: blocks = V^T (W J coeff) V, dense, consecutive (coeff_quad None: the mass matrix)"""
        assert blocks.numel() == self.matrix_nodes()
        self.lib.d4est_hip_compute_weighted_mass_blocks(self.handle, _ptr(coeff_quad) if coeff_quad is not None else None, _ptr(blocks))

    def set_lhs_element_blocks(self, blocks, block_offset=None):
        """zeroth-order term of apply_lhs as dense element blocks (read at every apply: the tensor is kept alive here); block_offset:
        per-element offsets in doubles (a Schwarz subdomain plan: the mesh element's block) or None = consecutive"""
        self._lhs_blocks = blocks
        off = None
        if block_offset is not None:
            off = np.ascontiguousarray(block_offset, dtype=np.int64)
            assert off.size == self.n_elements
        self.lib.d4est_hip_plan_set_lhs_element_blocks(self.handle, _ptr(blocks) if blocks is not None else None,
                                                       off.ctypes.data_as(_vp) if off is not None else None)

    def set_lhs_galerkin_chain(self, transfers, fine_plan):
        """zeroth-order term as the Galerkin chain T_0^T .. T_k^T (V^T W J c V)_fine T_k .. T_0 (transfers[0] starts at this plan's
        level; fine_plan carries the coefficient); transfers = [] switches it off"""
        self._lhs_chain = (list(transfers), fine_plan)
        arr = (ctypes.c_void_p * max(len(transfers), 1))(*[t.handle for t in transfers])
        self.lib.d4est_hip_plan_set_lhs_galerkin_chain(self.handle, len(transfers), arr, fine_plan.handle if fine_plan is not None else None)

    def apply_lhs(self, u, Au):
        self.lib.d4est_hip_apply_lhs(self.handle, _ptr(u), _ptr(Au))

    def cheby_iterate(self, u, rhs, Au, r, iters, lmin, lmax, residual_at_end=1):
        self.lib.d4est_hip_cheby_iterate(self.handle, _ptr(u), _ptr(rhs), _ptr(Au), _ptr(r), int(iters), float(lmin), float(lmax),
                                         int(residual_at_end))

    def cg_eigs(self, u, rhs, Au, imax, use_new=1):
        hist = np.zeros(2 * imax)
        b = self.lib.d4est_hip_cg_eigs(self.handle, _ptr(u), _ptr(rhs), _ptr(Au), int(imax), int(use_new), hist.ctypes.data_as(_c_double_p))
        return b, hist

    # ---- Krylov solves (d4est_solver_cg_solve, d4est_solver_fcg_solve)
    PC_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)

    def cg_solve(self, u, rhs, Au, imax, atol, rtol):
        """CG on apply_lhs from u (advanced in place); returns (iterations, history delta_0 .. delta_iterations)"""
        for t in (u, rhs, Au):
            assert t.numel() == self.local_nodes
        hist = np.zeros(int(imax) + 1)
        it = self.lib.d4est_hip_cg_solve(self.handle, _ptr(u), _ptr(rhs), _ptr(Au), int(imax), float(atol), float(rtol),
                                         hist.ctypes.data_as(_c_double_p))
        return it, hist[:it + 1]

    def cg_solve_host(self, u_host, rhs_host, imax, atol, rtol):
        """the host-vector form: returns (u, Au, iterations, history)"""
        u = np.ascontiguousarray(u_host, dtype=np.float64).copy()
        rhs = np.ascontiguousarray(rhs_host, dtype=np.float64)
        assert u.size == self.local_nodes and rhs.size == self.local_nodes
        Au = np.empty_like(u)
        hist = np.zeros(int(imax) + 1)
        it = self.lib.d4est_hip_cg_solve_host(self.handle, u.ctypes.data_as(_vp), rhs.ctypes.data_as(_vp), Au.ctypes.data_as(_vp),
                                              int(imax), float(atol), float(rtol), hist.ctypes.data_as(_c_double_p))
        return u, Au, it, hist[:it + 1]

    def _pc_pair(self, pc):
        """(d4est_hip_pc_fn, ctx) of a preconditioner argument: None, an object with `pc_fn` / `pc_ctx`, or a Python callable"""
        if pc is None:
            return None, None
        if hasattr(pc, "pc_fn"):
            return ctypes.c_void_p(pc.pc_fn), ctypes.c_void_p(pc.pc_ctx)

        def call(_ctx, r, z):
            try:
                pc(r, z)
            except BaseException:   # (as set_comm: a dropped exception would leave z unwritten)
                import sys
                import traceback
                sys.stderr.write("[D4EST_HIP_ABORT] exception in a preconditioner callback:\n")
                traceback.print_exc()
                sys.stderr.flush()
                os.abort()
        cb = self.PC_FN(call)
        self._cb_pc = cb
        return ctypes.cast(cb, ctypes.c_void_p), None

    def fcg_solve(self, u, rhs, Au, imax, atol, rtol, pc=None):
        """FCG on apply_lhs from u (advanced in place); returns (iterations, history |r_k|).  pc: None (the identity), an object
        with `pc_fn` / `pc_ctx` (a C d4est_hip_pc_fn and its context, passed straight through: no Python in the loop), or a
        Python callable pc(r_ptr, z_ptr) that enqueues z = B r on the plan's stream"""
        for t in (u, rhs, Au):
            assert t.numel() == self.local_nodes
        hist = np.zeros(max(int(imax), 1))
        fn, ctx = self._pc_pair(pc)
        it = self.lib.d4est_hip_fcg_solve(self.handle, _ptr(u), _ptr(rhs), _ptr(Au), int(imax), float(atol), float(rtol), fn, ctx,
                                          hist.ctypes.data_as(_c_double_p))
        return it, hist[:it]

    # ---- nonlinear problems: the power term a (b + u)^k, its linearisation and the Newton loop (d4est_hip_nonlinear.hip)
    LINEARISE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p)

    def set_nonlinear_power(self, a_quad, b_quad, k):
        """registers f(x, u) = a (b + u)^k: float64 CUDA tensors of local_nodes_quad entries (b_quad None: b = 0; a_quad None: the term
        is off).  The VALUES ARE CAPTURED by this call, as by set_lhs_coefficient; |k| <= 16"""
        for t in (a_quad, b_quad):
            assert t is None or t.numel() == self.local_nodes_quad
        self.lib.d4est_hip_plan_set_nonlinear_power(self.handle, _ptr(a_quad) if a_quad is not None else None,
                                                    _ptr(b_quad) if b_quad is not None else None, int(k))

    def set_nonlinear_abs_power(self, a_quad, b_quad, s):
        """registers the real form f(x, u) = a |b + u|^s (Jacobian s a |b + u|^(s-1)), evaluated as a pow(t t, s/2), t = b + V u;
        tensors and capture as set_nonlinear_power.  Setting either form clears the other"""
        for t in (a_quad, b_quad):
            assert t is None or t.numel() == self.local_nodes_quad
        self.lib.d4est_hip_plan_set_nonlinear_abs_power(self.handle, _ptr(a_quad) if a_quad is not None else None,
                                                        _ptr(b_quad) if b_quad is not None else None, float(s))

    def nonlinear_exponent(self):
        """s of the real form that is set, or None (the integer form, or no term)"""
        s = ctypes.c_double(0.0)
        return s.value if self.lib.d4est_hip_plan_nonlinear_exponent(self.handle, ctypes.byref(s)) else None

    def apply_nonlinear_term(self, u, out, beta=0):
        """out = beta out + V^T W J a (b + V u)^k (beta 0 or 1), one kernel where nonlinear_fused() holds"""
        assert u.numel() == self.local_nodes and out.numel() == self.local_nodes
        self.lib.d4est_hip_apply_nonlinear_term(self.handle, _ptr(u), int(beta), _ptr(out))

    def nonlinear_fused(self):
        return bool(self.lib.d4est_hip_plan_nonlinear_fused(self.handle))

    def linearise(self, u0):
        """the zeroth-order coefficient of apply_lhs becomes c = k a (b + V u0)^(k-1): set_lhs_coefficient(c) in one kernel"""
        assert u0.numel() == self.local_nodes
        self._lhs_coeff = None
        self.lib.d4est_hip_plan_linearise(self.handle, _ptr(u0))

    def build_residual(self, u, out, rhs=None, ghost_trace=None):
        """out = A u + N(u) - rhs with the boundary data currently set on the plan"""
        assert u.numel() == self.local_nodes and out.numel() == self.local_nodes
        self.lib.d4est_hip_build_residual(self.handle, _ptr(u), _ptr(ghost_trace) if ghost_trace is not None else None,
                                          _ptr(rhs) if rhs is not None else None, _ptr(out))

    def newton_solve(self, u, rhs=None, g_lobatto=None, atol=1e-15, rtol=1e-10, imin=0, imax=10, krylov_imax=200, krylov_atol=1e-15,
                     krylov_rtol=1e-10, pc=None, on_linearise=None):
        """d4est_solver_newton_solve with FCG on u (advanced in place); g_lobatto: Dirichlet data as a float64 CUDA tensor or None; pc as
        in fcg_solve; on_linearise(u0_ptr): a Python callable run after every linearisation (refresh the preconditioner there).
        Returns (ierr, iterations, history |F| of iterations + 1 entries)"""
        assert u.numel() == self.local_nodes and (rhs is None or rhs.numel() == self.local_nodes)
        assert g_lobatto is None or g_lobatto.numel() == self.lib.d4est_hip_plan_bndry_nodes(self.handle)
        fn, ctx = self._pc_pair(pc)
        cb = None
        if on_linearise is not None:
            def call(_ctx, u0):
                try:
                    on_linearise(u0)
                except BaseException:   # (as set_comm: a dropped exception would leave the preconditioner stale)
                    import sys
                    import traceback
                    sys.stderr.write("[D4EST_HIP_ABORT] exception in a linearisation callback:\n")
                    traceback.print_exc()
                    sys.stderr.flush()
                    os.abort()
            self._cb_lin = self.LINEARISE_FN(call)
            cb = ctypes.cast(self._cb_lin, ctypes.c_void_p)
        hist = np.zeros(int(imax) + 1)
        its = ctypes.c_int(0)
        ierr = self.lib.d4est_hip_newton_solve(self.handle, _ptr(u), _ptr(rhs) if rhs is not None else None,
                                               _ptr(g_lobatto) if g_lobatto is not None else None, float(atol), float(rtol), int(imin),
                                               int(imax), int(krylov_imax), float(krylov_atol), float(krylov_rtol), fn, ctx, cb, None,
                                               hist.ctypes.data_as(_c_double_p), ctypes.byref(its))
        return ierr, its.value, hist[:its.value + 1]

    # ---- problem data on the device (csrc/d4est_hip_problem.hip)
    def _brick_source(self, brick):
        """brick = (elem_q[n, 3], elem_dq, root_len, extents) -> ctypes arguments (kept alive by the caller)"""
        q, dq = _iarr(np.asarray(brick[0]).reshape(-1)), _iarr(brick[1])
        ex = np.ascontiguousarray(brick[3], dtype=np.float64)
        assert len(q[0]) == 3 * self.n_elements and len(dq[0]) == self.n_elements and ex.size == 6
        return (q, dq, ex), (q[1], dq[1], float(brick[2]), ex.ctypes.data_as(_vp))

    def _analytic_source(self, analytic):
        """analytic = (geom_type, params, tree, q, dq, root_len) -> ctypes arguments"""
        geom_type, params, tree, q, dq, root_len = analytic[:6]
        pr = np.zeros(5)
        pv = np.asarray(params, dtype=np.float64).reshape(-1)
        pr[:pv.size] = pv
        t, qq, d = _iarr(tree), _iarr(np.asarray(q).reshape(-1)), _iarr(dq)
        assert len(t[0]) == self.n_elements and len(d[0]) == self.n_elements and len(qq[0]) == 3 * self.n_elements
        return (pr, t, qq, d), (int(geom_type), pr.ctypes.data_as(_vp), t[1], qq[1], d[1], float(root_len))

    def compute_xyz_brick(self, elem_q, elem_dq, root_len, extents, xyz_lobatto=None, xyz_quad=None):
        """node coordinates of the single-tree brick on the device, the layout of compute_xyz_analytic"""
        keep, args = self._brick_source((elem_q, elem_dq, root_len, extents))
        assert xyz_lobatto is None or xyz_lobatto.numel() >= 3 * self.local_nodes
        assert xyz_quad is None or xyz_quad.numel() >= 3 * self.local_nodes_quad
        self.lib.d4est_hip_plan_compute_xyz_brick(self.handle, *args, _ptr(xyz_lobatto) if xyz_lobatto is not None else None,
                                                  _ptr(xyz_quad) if xyz_quad is not None else None)

    def _set_term(self, name, field_id, params, brick, analytic, xyz):
        assert (brick is not None) + (analytic is not None) + (xyz is not None) == 1, "one of brick / analytic / xyz"
        _, pr, n_params = _field_params(field_id, params)
        pp = pr.ctypes.data_as(_vp)
        if brick is not None:
            keep, args = self._brick_source(brick)
            getattr(self.lib, "d4est_hip_plan_set_%s_term_brick" % name)(self.handle, pp, n_params, *args)
        elif analytic is not None:
            keep, args = self._analytic_source(analytic)
            getattr(self.lib, "d4est_hip_plan_set_%s_term_analytic" % name)(self.handle, pp, n_params, *args)
        else:
            assert xyz.numel() == 3 * self.local_nodes_quad
            getattr(self.lib, "d4est_hip_plan_set_%s_term_xyz" % name)(self.handle, pp, n_params, _ptr(xyz))

    def set_puncture_term(self, params, brick=None, analytic=None, xyz=None):
        """the puncture term a (b + u)^-7 (a = -K2/8, b = 1 + sum m/(2r); capi.puncture_params) set on the plan by one kernel from
        brick = (elem_q, elem_dq, root_len, extents), analytic = (geom_type, params, tree, q, dq, root_len) or xyz = the caller's
        x | y | z at the quadrature nodes (a CUDA tensor); afterwards the plan is as set_nonlinear_power(a, b, -7) leaves it"""
        self._set_term("puncture", "PUNCTURE_A", params, brick, analytic, xyz)

    def set_cds_term(self, params, brick=None, analytic=None, xyz=None):
        """the ConstantDensityStar term a u^5, a = -2 pi rho (params = cx, cy, cz, R, rho0, C0, alpha, beta); sources as
        set_puncture_term; afterwards the plan is as set_nonlinear_power(a, None, 5) leaves it"""
        self._set_term("cds", "CDS_A", params, brick, analytic, xyz)

    def set_okendon_term(self, params, brick=None, analytic=None, xyz=None):
        """the Okendon term |u|^p (capi.okendon_params): a = 1, b = 0, the real form with s = p; sources as set_puncture_term;
        afterwards the plan is as set_nonlinear_abs_power(a, None, p) leaves it"""
        self._set_term("okendon", "OKENDON_U", params, brick, analytic, xyz)

    def set_boyen_york_term(self, params, brick=None, analytic=None, xyz=None):
        """the Boyen-York term a u^-7, a = BY_A (capi.boyen_york_params); sources as set_puncture_term; afterwards the plan is as
        set_nonlinear_power(a, None, -7) leaves it"""
        self._set_term("boyen_york", "BY_A", params, brick, analytic, xyz)

    def build_load(self, field_id, params, out, beta=0, brick=None, analytic=None, xyz=None):
        """out = beta out + V^T W J f(x_quad), f a problem field (capi.FIELD name or id): the load vector of a linear problem in one
        kernel per degree bucket where apply_galerkin_integral has a one-kernel path; sources as set_puncture_term"""
        assert (brick is not None) + (analytic is not None) + (xyz is not None) == 1, "one of brick / analytic / xyz"
        assert out.numel() == self.local_nodes and beta in (0, 1)
        fid, pr, n_params = _field_params(field_id, params)
        pp = pr.ctypes.data_as(_vp)
        if brick is not None:
            keep, args = self._brick_source(brick)
            self.lib.d4est_hip_plan_build_load_by_id_brick(self.handle, fid, pp, n_params, *args, int(beta), _ptr(out))
        elif analytic is not None:
            keep, args = self._analytic_source(analytic)
            self.lib.d4est_hip_plan_build_load_by_id_analytic(self.handle, fid, pp, n_params, *args, int(beta), _ptr(out))
        else:
            assert xyz.numel() == 3 * self.local_nodes_quad
            self.lib.d4est_hip_plan_build_load_by_id_xyz(self.handle, fid, pp, n_params, _ptr(xyz), int(beta), _ptr(out))

    def nonlinear_coefficients(self, device=None):
        """(a, b, k) of the power term that is set: torch VIEWS of the plan-owned arrays (b None when b = 0), or None when the term is
        off; valid until the term changes or the plan is destroyed"""
        import torch
        pa, pb, k = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
        if not self.lib.d4est_hip_plan_nonlinear_coefficients(self.handle, ctypes.byref(pa), ctypes.byref(pb), ctypes.byref(k)):
            return None
        dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        return self._quad_view(pa, dev), self._quad_view(pb, dev), k.value

    def _quad_view(self, p, dev):
        """a torch VIEW of local_nodes_quad plan-owned doubles at the device pointer p (a ctypes.c_void_p; NULL: None)"""
        import torch
        n = self.local_nodes_quad
        if not p.value:
            return None
        if n == 0:
            return torch.empty(0, dtype=torch.float64, device=dev)

        class _View:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (int(p.value), False), "version": 2, "strides": None}

        t = torch.as_tensor(_View(), device=dev)
        t._d4est_hip_plan = self
        return t

    def lhs_coefficient_arrays(self, device=None):
        """(c, w J c) of the coefficient form that is set (set_lhs_coefficient / linearise): torch VIEWS of the plan-owned arrays, w J c
        None while it is not formed (the first apply that needs it forms it), or None when no coefficient form is set; the views follow
        every later set_lhs_coefficient / linearise on the plan's stream and are valid until the plan is destroyed"""
        import torch
        pc, pw = ctypes.c_void_p(), ctypes.c_void_p()
        if not self.lib.d4est_hip_plan_lhs_coefficient_arrays(self.handle, ctypes.byref(pc), ctypes.byref(pw)):
            return None
        dev = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        return self._quad_view(pc, dev), self._quad_view(pw, dev)

    def compute_boundary_xyz(self, xyz_mortar, brick=None, analytic=None):
        """x | y | z at the mortar quadrature nodes of every boundary side, indexed like sj (components total_mortar_nodes apart):
        xyz_mortar is a float64 CUDA tensor of 3 total_mortar_nodes; entries of other sides are left untouched.  Sources as
        set_puncture_term's brick / analytic; needs set_faces"""
        assert (brick is None) != (analytic is None), "one of brick / analytic"
        assert xyz_mortar.numel() == 3 * self.total_mortar_nodes
        if brick is not None:
            keep, args = self._brick_source(brick)
            self.lib.d4est_hip_plan_compute_boundary_xyz_brick(self.handle, *args, _ptr(xyz_mortar))
        else:
            keep, args = self._analytic_source(analytic)
            self.lib.d4est_hip_plan_compute_boundary_xyz_analytic(self.handle, *args, _ptr(xyz_mortar))

    def set_robin_by_id(self, coeff_id, rhs_id, brick=None, analytic=None):
        """Robin data from callback ids (capi.ROBIN_COEFF / capi.ROBIN_RHS names or ids) evaluated at the boundary mortar nodes on the
        device: the state set_robin_values leaves.  'BRICK' needs the brick source; set_robin_values(None, None) switches back"""
        assert (brick is None) != (analytic is None), "one of brick / analytic"
        c = ROBIN_COEFF[coeff_id] if isinstance(coeff_id, str) else int(coeff_id)
        r = ROBIN_RHS[rhs_id] if isinstance(rhs_id, str) else int(rhs_id)
        assert c in (0, 1, 2) and r in (0, 1), "unknown Robin id"
        assert not (c == 1 and brick is None), "ROBIN_COEFF_BRICK needs the brick source"
        if brick is not None:
            keep, args = self._brick_source(brick)
            self.lib.d4est_hip_plan_set_robin_by_id_brick(self.handle, c, r, *args)
        else:
            keep, args = self._analytic_source(analytic)
            self.lib.d4est_hip_plan_set_robin_by_id_analytic(self.handle, c, r, *args)

    def dirichlet_from_field(self, field_id, params, xyz_lobatto, out=None):
        """Dirichlet data of a problem field (e.g. 'CDS_PSI') in set_dirichlet_values' layout: the three Lobatto coordinate vectors of
        xyz_lobatto (x | y | z, 3 local_nodes) gathered to the boundary face nodes, then field_eval.  Returns the CUDA tensor"""
        import torch
        nb = self.lib.d4est_hip_plan_bndry_nodes(self.handle)
        assert xyz_lobatto.numel() == 3 * self.local_nodes
        bx = torch.empty(3 * nb, dtype=torch.float64, device=xyz_lobatto.device)
        for d in range(3):
            self.boundary_gather(xyz_lobatto[d * self.local_nodes:(d + 1) * self.local_nodes], bx[d * nb:(d + 1) * nb])
        if out is None:
            out = torch.empty(nb, dtype=torch.float64, device=xyz_lobatto.device)
        assert out.numel() == nb
        field_eval(field_id, params, bx, out, getattr(self, "_stream_handle", 0))   # the plan's own stream (0: the default stream)
        return out

    def copy_blocks(self, n_blocks, src, src_off, dst, dst_off, length):
        """src/dst: float64 CUDA tensors; src_off/dst_off: int64 CUDA tensors; length: int32 CUDA tensor"""
        self.lib.d4est_hip_copy_blocks(self.handle, int(n_blocks), _ptr(src), ctypes.c_void_p(src_off.data_ptr()), _ptr(dst),
                                       ctypes.c_void_p(dst_off.data_ptr()), ctypes.c_void_p(length.data_ptr()))

    def vec_dot(self, x, y, out):
        self.lib.d4est_hip_vec_dot(self.handle, int(x.numel()), _ptr(x), _ptr(y), _ptr(out))

    def apply_stiffness_matrix_host(self, u_host):
        u = np.ascontiguousarray(u_host, dtype=np.float64)
        assert u.size == self.local_nodes
        out = np.empty_like(u)
        self.lib.d4est_hip_apply_stiffness_matrix_host(self.handle, u.ctypes.data_as(_vp), out.ctypes.data_as(_vp))
        return out

    def destroy(self):
        if self.handle:
            self.lib.d4est_hip_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Transfer:
    """hp-multigrid inter-grid transfer (d4est_hip_transfer_*): items = coarse elements in traversal order,
    hrefine[k] 0 (1 <-> 1, p only) or 1 (8 children <-> parent), degH[k], degh[8k..8k+7]."""

    def __init__(self, hrefine, degH, degh, stream=None):
        self.lib = load_library()
        h, dH, dh = _iarr(hrefine), _iarr(degH), _iarr(degh)
        assert len(dh[0]) == 8 * len(h[0]) and len(dH[0]) == len(h[0])
        self.handle = self.lib.d4est_hip_transfer_create(len(h[0]), h[1], dH[1], dh[1])
        if stream is not None:
            self.lib.d4est_hip_transfer_set_stream(self.handle, ctypes.c_void_p(stream.cuda_stream))
        self.coarse_nodes = self.lib.d4est_hip_transfer_coarse_nodes(self.handle)
        self.fine_nodes = self.lib.d4est_hip_transfer_fine_nodes(self.handle)

    def prolong(self, x_coarse, x_fine):
        assert x_coarse.numel() == self.coarse_nodes and x_fine.numel() == self.fine_nodes
        self.lib.d4est_hip_transfer_prolong(self.handle, _ptr(x_coarse), _ptr(x_fine))

    def prolong_add(self, x_coarse, u_fine):
        """u_fine += P x_coarse in one kernel; bit-identical to prolong into a scratch vector followed by +="""
        assert x_coarse.numel() == self.coarse_nodes and u_fine.numel() == self.fine_nodes
        self.lib.d4est_hip_transfer_prolong_add(self.handle, _ptr(x_coarse), _ptr(u_fine))

    def restrict(self, x_fine, x_coarse):
        assert x_coarse.numel() == self.coarse_nodes and x_fine.numel() == self.fine_nodes
        self.lib.d4est_hip_transfer_restrict(self.handle, _ptr(x_fine), _ptr(x_coarse))

    def galerkin_blocks(self, fine_blocks, coarse_blocks, literal_window=False):
        """coarse block k = sum over the item's children of P^T M P (the multigrid matrix operator's restriction callback);
        literal_window: the reference's arithmetic to the letter on items with eight children (d4est_operators.c:651)"""
        assert fine_blocks.numel() == self.lib.d4est_hip_transfer_fine_matrix_nodes(self.handle)
        assert coarse_blocks.numel() == self.lib.d4est_hip_transfer_coarse_matrix_nodes(self.handle)
        self.lib.d4est_hip_transfer_galerkin_blocks(self.handle, _ptr(fine_blocks), _ptr(coarse_blocks), int(bool(literal_window)))

    def project(self, x_fine, x_coarse):
        """L2 projection onto the coarse space (apply_p_restrict / apply_hp_restrict per item)"""
        assert x_fine.numel() == self.fine_nodes and x_coarse.numel() == self.coarse_nodes
        self.lib.d4est_hip_transfer_project(self.handle, _ptr(x_fine), _ptr(x_coarse))

    def describe(self):
        """the work lists behind this transfer (d4est_hip_transfer_describe): {"prolong" | "restrict" | "galerkin": [(NH, dmax, nc, n, cg)]};
        NH = 0 is the generic list, "galerkin" is empty until a one-transfer chain with this transfer is set on a plan"""
        out = {}
        for which, name in enumerate(("prolong", "restrict", "galerkin")):
            n = self.lib.d4est_hip_transfer_describe(self.handle, which, None, 0)
            buf = ctypes.create_string_buffer(n + 1)
            self.lib.d4est_hip_transfer_describe(self.handle, which, buf, n + 1)
            out[name] = [tuple(int(v) for v in line.split()) for line in buf.value.decode().splitlines()]
        return out

    def destroy(self):
        if self.handle:
            self.lib.d4est_hip_transfer_destroy(self.handle)
            self.handle = None


class Amr:
    """One rank's hp-AMR bookkeeping on the device (d4est_hip_amr_*): degrees, the smooth_pred predictor, the refinement log, and the
    transfer of a field to the refined and balanced grid.  eta2 / stats / fields are float64 CUDA tensors; the logs are host int arrays."""

    def __init__(self, deg, max_degree, initial_pred, stream=None):
        self.lib = load_library()
        d = _iarr(deg)
        self.handle = self.lib.d4est_hip_amr_create(len(d[0]), d[1], int(max_degree), float(initial_pred))
        self.torch_stream = stream
        self.rank, self.world = 0, 1
        if stream is not None:
            self.lib.d4est_hip_amr_set_stream(self.handle, ctypes.c_void_p(stream.cuda_stream))

    @property
    def n_elements(self):
        return self.lib.d4est_hip_amr_n_elements(self.handle)

    @property
    def local_nodes(self):
        return self.lib.d4est_hip_amr_local_nodes(self.handle)

    def stats(self, eta2, percentile, stats):
        """stats (4 doubles on the device) <- total, mean, max, estimator_at_percentile"""
        assert eta2.numel() == self.n_elements and stats.numel() == 4
        self.lib.d4est_hip_amr_stats(self.handle, _ptr(eta2), int(percentile), _ptr(stats))

    def mark_smooth_pred(self, eta2, threshold, factor, gamma_h, gamma_p, gamma_n):
        """threshold: a one-entry device tensor, e.g. stats[1:2] (mean; factor = sigma) or stats[3:4] (percentile; factor = 1)"""
        assert eta2.numel() == self.n_elements and threshold.numel() == 1
        self.lib.d4est_hip_amr_mark_smooth_pred(self.handle, _ptr(eta2), _ptr(threshold), float(factor), float(gamma_h), float(gamma_p),
                                                float(gamma_n))

    def p_balance(self, p_balance, p_balance_if_diff):
        a = _iarr(p_balance)
        assert len(a[0]) == self.n_elements
        self.lib.d4est_hip_amr_p_balance(self.handle, a[1], int(p_balance_if_diff))

    def get_refinement_log(self):
        out = np.empty(self.n_elements, dtype=np.int32)
        self.lib.d4est_hip_amr_get_refinement_log(self.handle, out.ctypes.data_as(_c_int_p))
        return out

    def set_refinement_log(self, log):
        a = _iarr(log)
        assert len(a[0]) == self.n_elements
        self.lib.d4est_hip_amr_set_refinement_log(self.handle, a[1])

    def get_predictor(self):
        out = np.empty(self.n_elements, dtype=np.float64)
        self.lib.d4est_hip_amr_get_predictor(self.handle, out.ctypes.data_as(_c_double_p))
        return out

    def set_balance(self, balance_log):
        a = _iarr(balance_log)
        self.lib.d4est_hip_amr_set_balance(self.handle, len(a[0]), a[1])
        self.new_n_elements = self.lib.d4est_hip_amr_new_n_elements(self.handle)
        self.new_local_nodes = self.lib.d4est_hip_amr_new_local_nodes(self.handle)

    def new_degrees(self):
        out = np.empty(self.lib.d4est_hip_amr_new_n_elements(self.handle), dtype=np.int32)
        self.lib.d4est_hip_amr_get_new_degrees(self.handle, out.ctypes.data_as(_c_int_p))
        return out

    def interpolate_field(self, field_old, field_new):
        assert field_old.numel() == self.local_nodes and field_new.numel() == self.new_local_nodes
        self.lib.d4est_hip_amr_interpolate_field(self.handle, _ptr(field_old), _ptr(field_new))

    def describe(self):
        """the work lists of the field transfer: [(NH, dmax, nout, n)]; NH = 0 is the runtime-size kernel, (-1, 0, 0, n_aux) two-stage mode"""
        n = self.lib.d4est_hip_amr_describe(self.handle, None, 0)
        buf = ctypes.create_string_buffer(n + 1)
        self.lib.d4est_hip_amr_describe(self.handle, buf, n + 1)
        return [tuple(int(v) for v in line.split()) for line in buf.value.decode().splitlines()]

    def advance(self):
        self.lib.d4est_hip_amr_advance(self.handle)

    # ---- several ranks
    SENDRECV_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, _c_int_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong),
                                   ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong))

    def set_comm(self, rank, world, allreduce=None, sendrecv=None):
        """allreduce(scalars_ptr, n): in-place SUM over ranks of n device doubles; sendrecv(peers, send_ptr, send_first, recv_ptr,
        recv_first): one grouped point-to-point round (peers and the two first lists are python lists, pointers are ints).  An exception
        inside a hook aborts the process, as in Plan.set_comm."""
        def guarded(fn):
            def call(*args):
                try:
                    fn(*args)
                except BaseException:
                    import os
                    import sys
                    import traceback
                    sys.stderr.write("[D4EST_HIP_ABORT] exception in a communication callback:\n")
                    traceback.print_exc()
                    sys.stderr.flush()
                    os.abort()
            return call

        def sr(ctx, n, peers, send, sf, recv, rf):
            sendrecv([peers[i] for i in range(n)], send or 0, [sf[i] for i in range(n + 1)], recv or 0, [rf[i] for i in range(n + 1)])

        self._cb_ar = Plan.ALLREDUCE_FN(guarded(lambda ctx, p, n: allreduce(p, n))) if allreduce else None
        self._cb_sr = self.SENDRECV_FN(guarded(sr)) if sendrecv else None
        self.lib.d4est_hip_par_amr_set_comm(self.handle, int(rank), int(world), ctypes.cast(self._cb_ar, ctypes.c_void_p) if self._cb_ar else None,
                                        ctypes.cast(self._cb_sr, ctypes.c_void_p) if self._cb_sr else None, None)
        self.rank, self.world = int(rank), int(world)

    def stats_global(self, eta2, percentile, stats):
        """stats (4 doubles on the device) <- total, mean, max and estimator_at_percentile over ALL ranks (d4est_hip_par_amr_stats_global)"""
        assert eta2.numel() == self.n_elements and stats.numel() == 4
        self.lib.d4est_hip_par_amr_stats_global(self.handle, _ptr(eta2), int(percentile), _ptr(stats))

    def repartition(self, old_first, new_first):
        """moves degrees and predictor to the partition new_first (global_first_quadrant, world + 1 entries); returns the new local_nodes"""
        o = np.ascontiguousarray(old_first, dtype=np.int64)
        n = np.ascontiguousarray(new_first, dtype=np.int64)
        assert len(o) == self.world + 1 and len(n) == self.world + 1
        return self.lib.d4est_hip_par_amr_repartition(self.handle, o.ctypes.data_as(ctypes.c_void_p), n.ctypes.data_as(ctypes.c_void_p))

    def repartition_field(self, field_old, field_new):
        """one nodal field from the old partition to the new one (after repartition)"""
        assert field_new.numel() == self.local_nodes
        self.lib.d4est_hip_par_amr_repartition_field(self.handle, _ptr(field_old), _ptr(field_new))

    def destroy(self):
        if self.handle:
            self.lib.d4est_hip_amr_destroy(self.handle)
            self.handle = None


GEOM_BRICK = 0


class Probe:
    """Point probes on a plan (d4est_hip_probe_*): the points (tree[n], abc[n, 3] tree coordinates) are located once among the plan's
    elements -- cells = (elem_tree, elem_q[ne, 3], elem_dq) and root_len, what mesh.BrickMesh.cells() / forest.ForestMesh.cells() return --
    and then evaluated on the device: eval (values), eval_gradient (reference-space or physical gradient), xyz.  Fields and outputs are
    float64 CUDA tensors.  The probe must be destroyed before its plan."""

    def __init__(self, plan, tree, abc, cells, root_len):
        self.lib = load_library()
        self.plan = plan   # keeps the plan alive as long as the probe
        t = _iarr(np.asarray(tree).reshape(-1))
        a = np.ascontiguousarray(np.asarray(abc, dtype=np.float64).reshape(-1))
        self.n_points = len(t[0])
        assert a.size == 3 * self.n_points
        et, eq, ed = _iarr(cells[0]), _iarr(np.asarray(cells[1]).reshape(-1)), _iarr(cells[2])
        assert len(et[0]) == plan.n_elements and len(ed[0]) == plan.n_elements and len(eq[0]) == 3 * plan.n_elements
        self.handle = self.lib.d4est_hip_probe_create(plan.handle, self.n_points, t[1], a.ctypes.data_as(_vp), et[1], eq[1], ed[1],
                                                      float(root_len), 0)

    def info(self):
        """(err[n], elem[n], rst[n, 3]) as numpy arrays: err 0 found / 1 not on this plan, the local element id (-1), the element's rst (NaN)"""
        err = np.empty(self.n_points, dtype=np.int32)
        elem = np.empty(self.n_points, dtype=np.int32)
        rst = np.empty((self.n_points, 3), dtype=np.float64)
        self.lib.d4est_hip_probe_info(self.handle, err.ctypes.data_as(_vp), elem.ctypes.data_as(_vp), rst.ctypes.data_as(_vp))
        return err, elem, rst

    def element_info(self):
        """(nodal_stride[n], deg[n]) of the located elements (0 where err = 1)"""
        ns = np.empty(self.n_points, dtype=np.int32)
        deg = np.empty(self.n_points, dtype=np.int32)
        self.lib.d4est_hip_probe_element_info(self.handle, ns.ctypes.data_as(_vp), deg.ctypes.data_as(_vp))
        return ns, deg

    def eval(self, u, out, n_fields=1, field_stride=0):
        """out[f * n_points + p] = field f (at u[f * field_stride:]) at point p; NaN where err = 1.  Stream-ordered, no synchronisation."""
        assert out.numel() >= n_fields * self.n_points
        assert u.numel() >= (n_fields - 1) * field_stride + self.plan.local_nodes
        if self.n_points == 0 or n_fields == 0:
            return
        self.lib.d4est_hip_probe_eval(self.handle, int(n_fields), _ptr(u), int(field_stride), _ptr(out))

    def set_map(self, geom_type, params):
        """the map of the plan's geometry: capi.GEOM_BRICK with the six extents, or a sphere type with its params (forest maps: .params)"""
        pr = np.zeros(6)
        pv = np.asarray(params, dtype=np.float64).reshape(-1)
        pr[:pv.size] = pv
        self.lib.d4est_hip_probe_set_map(self.handle, int(geom_type), pr.ctypes.data_as(_vp))

    def eval_gradient(self, u, grad, physical=False):
        """grad[d * n_points + p]: the reference-space gradient, or with physical=True (after set_map) d/dx, d/dy, d/dz"""
        assert grad.numel() >= 3 * self.n_points and u.numel() >= self.plan.local_nodes
        if self.n_points == 0:
            return
        self.lib.d4est_hip_probe_eval_gradient(self.handle, _ptr(u), _ptr(grad), 1 if physical else 0)

    def xyz(self):
        """physical coordinates [n, 3] of the points through the map of set_map (NaN where err = 1)"""
        out = np.empty((self.n_points, 3), dtype=np.float64)
        self.lib.d4est_hip_probe_xyz(self.handle, out.ctypes.data_as(_vp))
        return out

    def destroy(self):
        if self.handle:
            self.lib.d4est_hip_probe_destroy(self.handle)
            self.handle = None


def multigrid_check(plans, transfers, n_levels=None):
    """d4est_hip_multigrid_check: 0, or 1 (fewer than two levels), 2 (a missing entry: None), 3 (a transfer's node counts do not match
    its two plans).  plans: coarsest first; transfers[l] connects plans[l] and plans[l + 1]."""
    lib = load_library()
    n = len(plans) if n_levels is None else int(n_levels)
    pa = (ctypes.c_void_p * max(len(plans), 1))(*[(p.handle if p is not None else None) for p in plans])
    ta = (ctypes.c_void_p * max(len(transfers), 1))(*[(t.handle if t is not None else None) for t in transfers])
    return lib.d4est_hip_multigrid_check(n, pa, ta)


class Multigrid:
    """The hp-multigrid V-cycle, solve and preconditioner on the device (d4est_hip_multigrid_*): plans[0] is the bottom (coarsest)
    level, plans[-1] the top (finest); transfers[l] connects plans[l] (coarse) and plans[l + 1] (fine).  Every plan carries its own
    operator (faces, zeroth-order term, hooks).  `pc_fn` / `pc_ctx` make the object a preconditioner of Plan.fcg_solve(pc=mg): the C
    function pointer and its context are passed straight through, no Python in the loop."""

    def __init__(self, plans, transfers):
        self.lib = load_library()
        self.handle = None
        self.plans, self.transfers = list(plans), list(transfers)   # kept alive: the object only borrows them
        code = multigrid_check(self.plans, self.transfers)
        if code != 0:            # (d4est_hip_multigrid_create would abort the process)
            raise ValueError("d4est_hip_multigrid_check returned %d" % code)
        pa = (ctypes.c_void_p * len(self.plans))(*[p.handle for p in self.plans])
        ta = (ctypes.c_void_p * len(self.transfers))(*[t.handle for t in self.transfers])
        self.handle = self.lib.d4est_hip_multigrid_create(len(self.plans), pa, ta)
        self.n_levels = len(self.plans)
        self.local_nodes = self.plans[-1].local_nodes
        self.pc_fn = ctypes.cast(self.lib.d4est_hip_multigrid_pc_apply, ctypes.c_void_p).value
        self.pc_ctx = self.handle

    def set_stream(self, stream):
        h = getattr(stream, "cuda_stream", stream)
        self.lib.d4est_hip_multigrid_set_stream(self.handle, ctypes.c_void_p(int(h)))

    def set_smoother_cheby(self, cheby_imax, cheby_eigs_cg_imax, cheby_eigs_lmax_lmin_ratio, cheby_eigs_max_multiplier=1.0,
                           cheby_eigs_reuse_fromdownvcycle=0, cheby_eigs_reuse_fromlastvcycle=0, cheby_use_new_cg_eigs=0,
                           cheby_use_zero_guess_for_eigs=0):
        """the [mg_smoother_cheby] keys; returns the C code (0 = accepted; 1 = zero guess without reuse_fromdownvcycle; 2 = bad counts)"""
        return self.lib.d4est_hip_multigrid_set_smoother_cheby(
            self.handle, int(cheby_imax), int(cheby_eigs_cg_imax), float(cheby_eigs_lmax_lmin_ratio), float(cheby_eigs_max_multiplier),
            int(cheby_eigs_reuse_fromdownvcycle), int(cheby_eigs_reuse_fromlastvcycle), int(cheby_use_new_cg_eigs),
            int(cheby_use_zero_guess_for_eigs))

    def set_smoother_schwarz(self, schwarz_list, iterations, subdomain_iter=None, subdomain_atol=None, subdomain_rtol=None):
        """the [mg_smoother_schwarz] smoother: schwarz_list[l] is the schwarz.Schwarz object of plans[l] (entry 0 may be None unless the
        reuse_smoother bottom solver is used).  The subdomain CG options are the Schwarz objects' own (they must agree, as in the
        reference where one input section serves every level) unless passed explicitly.  Returns the C code: 0 accepted; 1 a missing
        entry on a level >= 1; 2 node counts; 3 streams; 4 a plan with ghost sides; 5 options <= 0"""
        sl = list(schwarz_list)
        if len(sl) != self.n_levels:
            raise ValueError("set_smoother_schwarz: %d entries for %d levels" % (len(sl), self.n_levels))
        given = [z for z in sl if z is not None]
        opts = []
        for name, val in (("subdomain_iter", subdomain_iter), ("subdomain_atol", subdomain_atol), ("subdomain_rtol", subdomain_rtol)):
            if val is None:
                vals = {getattr(z, name) for z in given}
                if len(vals) > 1:
                    raise ValueError("set_smoother_schwarz: the Schwarz objects disagree on %s; pass it explicitly" % name)
                val = vals.pop() if vals else 0
            opts.append(val)
        self._schwarz = sl                                   # kept alive: the object only borrows the handles
        ha = (ctypes.c_void_p * self.n_levels)(*[(z.handle if z is not None else None) for z in sl])
        return self.lib.d4est_hip_multigrid_set_smoother_schwarz(self.handle, ha, int(iterations), int(opts[0]), float(opts[1]), float(opts[2]))

    def set_bottom_solver_reuse_smoother(self):
        """[mg_bottom_solver_reuse_smoother]: the bottom solve is the current smoother on level 0"""
        self.lib.d4est_hip_multigrid_set_bottom_solver_reuse_smoother(self.handle)

    def smooth_level(self, level, u, rhs, Au, r):
        """one call of the current smoother on `level`, as the V-cycle makes it: r = rhs - A u of the final iterate on exit"""
        n = self.plans[level].local_nodes
        for t in (u, rhs, Au, r):
            assert t.numel() == n
        self.lib.d4est_hip_multigrid_smooth_level(self.handle, int(level), _ptr(u), _ptr(rhs), _ptr(Au), _ptr(r))

    def set_bottom_solver_cg(self, bottom_imax, bottom_atol, bottom_rtol):
        self.lib.d4est_hip_multigrid_set_bottom_solver_cg(self.handle, int(bottom_imax), float(bottom_atol), float(bottom_rtol))

    def set_bottom_solver_cheby(self, cheby_imax, cheby_eigs_cg_imax, lmax_lmin_ratio, max_multiplier=1.0, use_new_cg_eigs=0):
        self.lib.d4est_hip_multigrid_set_bottom_solver_cheby(self.handle, int(cheby_imax), int(cheby_eigs_cg_imax), float(lmax_lmin_ratio),
                                                             float(max_multiplier), int(use_new_cg_eigs))

    def set_pc(self, vcycle_imax=1, vcycle_atol=0.0, vcycle_rtol=0.0):
        self.lib.d4est_hip_multigrid_set_pc(self.handle, int(vcycle_imax), float(vcycle_atol), float(vcycle_rtol))

    def ready(self):
        return self.lib.d4est_hip_multigrid_ready(self.handle)

    def _require_ready(self):
        if not self.ready():     # (the C entry would abort the process)
            raise RuntimeError("Multigrid: set a smoother and a bottom solver first")

    def vcycle(self, u, rhs, Au, vcycle_index=0):
        """one V-cycle on A u = rhs; returns vcycle_r2_local = |rhs - A u|^2 of the last smoother call"""
        self._require_ready()
        for t in (u, rhs, Au):
            assert t.numel() == self.local_nodes
        self.lib.d4est_hip_multigrid_vcycle(self.handle, _ptr(u), _ptr(rhs), _ptr(Au), int(vcycle_index))
        return self.lib.d4est_hip_multigrid_vcycle_r2(self.handle)

    def solve(self, u, rhs, Au, vcycle_imax, vcycle_atol, vcycle_rtol):
        """d4est_solver_multigrid_solve from u (advanced in place); returns (cycles, history r2_0 .. r2_cycles)"""
        self._require_ready()
        for t in (u, rhs, Au):
            assert t.numel() == self.local_nodes
        hist = np.zeros(int(vcycle_imax) + 1)
        n = self.lib.d4est_hip_multigrid_solve(self.handle, _ptr(u), _ptr(rhs), _ptr(Au), int(vcycle_imax), float(vcycle_atol),
                                               float(vcycle_rtol), hist.ctypes.data_as(_c_double_p))
        return n, hist[:n + 1]

    def pc_apply(self, r, z):
        """z = B r: the preconditioner as Plan.fcg_solve calls it through the C pointer"""
        self._require_ready()
        assert r.numel() == self.local_nodes and z.numel() == self.local_nodes
        self.lib.d4est_hip_multigrid_pc_apply(self.handle, _ptr(r), _ptr(z))

    def info(self):
        """(eigs per level after the multiplier, V-cycles of the last solve, bottom iterations of the last cycle)"""
        eigs = np.zeros(self.n_levels)
        vc, bi = ctypes.c_int(0), ctypes.c_int(0)
        self.lib.d4est_hip_multigrid_get_info(self.handle, eigs.ctypes.data_as(_c_double_p), ctypes.byref(vc), ctypes.byref(bi))
        return eigs, vc.value, bi.value

    def destroy(self):
        if self.handle:
            self.lib.d4est_hip_multigrid_destroy(self.handle)
            self.handle = None
            self.pc_ctx = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class PcCheby:
    """d4est_krylov_pc_cheby on the device (d4est_hip_pc_cheby_*), the [d4est_krylov_pc_cheby] keys.  Passed as `pc` to Plan.fcg_solve /
    Plan.newton_solve like a Multigrid: `pc_fn` / `pc_ctx` are the C function pointer and the object, no Python in the loop."""

    def __init__(self, plan, cheby_imax, cheby_eigs_cg_imax, cheby_eigs_lmax_lmin_ratio, cheby_eigs_max_multiplier=1.0, cheby_reuse_eig=0,
                 cheby_use_new_cg_eigs=0, cheby_use_zero_guess_for_eigs=0):
        self.lib = load_library()
        self.handle = None
        if int(cheby_imax) < 0 or int(cheby_eigs_cg_imax) < 1 or not float(cheby_eigs_lmax_lmin_ratio) > 0.0:   # (the C entry would abort)
            raise ValueError("PcCheby: cheby_imax < 0, cheby_eigs_cg_imax < 1 or a ratio that is not positive")
        self.plan = plan                                     # kept alive: the object only borrows it
        self.local_nodes = plan.local_nodes
        self.handle = self.lib.d4est_hip_pc_cheby_create(plan.handle, int(cheby_imax), int(cheby_eigs_cg_imax), float(cheby_eigs_lmax_lmin_ratio),
                                                         float(cheby_eigs_max_multiplier), int(cheby_reuse_eig), int(cheby_use_new_cg_eigs),
                                                         int(cheby_use_zero_guess_for_eigs))
        self.pc_fn = ctypes.cast(self.lib.d4est_hip_pc_cheby_apply, ctypes.c_void_p).value
        self.pc_ctx = self.handle

    def apply(self, r, z):
        """z = B r"""
        assert r.numel() == self.local_nodes and z.numel() == self.local_nodes
        self.lib.d4est_hip_pc_cheby_apply(self.handle, _ptr(r), _ptr(z))

    def eig(self):
        """(the bound held, after the multiplier; -1 = none, cg_eigs runs so far)"""
        runs = ctypes.c_int(0)
        e = self.lib.d4est_hip_pc_cheby_eig(self.handle, ctypes.byref(runs))
        return e, runs.value

    def reset_eig(self):
        self.lib.d4est_hip_pc_cheby_reset_eig(self.handle)

    def destroy(self):
        if self.handle:
            self.lib.d4est_hip_pc_cheby_destroy(self.handle)
            self.handle = None
            self.pc_ctx = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class PcSchwarz:
    """d4est_krylov_pc_schwarz on the device (d4est_hip_pc_schwarz_*): z = 0, then `iterations` times { residual = r - A z;
    schwarz_iterate(z, residual) }.  schwarz: a schwarz.Schwarz object of the mesh whose plan is mesh_plan; the subdomain CG options are
    the object's own unless passed.  Passed as `pc` to Plan.fcg_solve / Plan.newton_solve like a Multigrid."""

    def __init__(self, schwarz, mesh_plan, iterations=1, subdomain_iter=None, subdomain_atol=None, subdomain_rtol=None):
        self.lib = load_library()
        self.handle = None
        it = schwarz.subdomain_iter if subdomain_iter is None else subdomain_iter
        atol = schwarz.subdomain_atol if subdomain_atol is None else subdomain_atol
        rtol = schwarz.subdomain_rtol if subdomain_rtol is None else subdomain_rtol
        if mesh_plan.local_nodes != schwarz.local_nodes:      # (the C entry would abort)
            raise ValueError("PcSchwarz: the plan has %d nodes, the smoother's mesh %d" % (mesh_plan.local_nodes, schwarz.local_nodes))
        if int(iterations) < 0 or int(it) <= 0 or not float(atol) > 0 or not float(rtol) > 0:
            raise ValueError("PcSchwarz: some options are <= 0")
        self.schwarz, self.plan = schwarz, mesh_plan         # kept alive: the object only borrows them
        self.local_nodes = mesh_plan.local_nodes
        self.handle = self.lib.d4est_hip_pc_schwarz_create(schwarz.handle, mesh_plan.handle, int(iterations), int(it), float(atol), float(rtol))
        self.pc_fn = ctypes.cast(self.lib.d4est_hip_pc_schwarz_apply, ctypes.c_void_p).value
        self.pc_ctx = self.handle

    def apply(self, r, z):
        """z = B r"""
        assert r.numel() == self.local_nodes and z.numel() == self.local_nodes
        self.lib.d4est_hip_pc_schwarz_apply(self.handle, _ptr(r), _ptr(z))

    def destroy(self):
        if self.handle:
            self.lib.d4est_hip_pc_schwarz_destroy(self.handle)
            self.handle = None
            self.pc_ctx = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
