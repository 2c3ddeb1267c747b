"""ctypes binding of libfs_hip.so (include/fs_hip.h).  No PyTorch, no Taichi: numpy + ctypes only.

The library is REQUIRED: there is no CPU or eager fallback in the product path.  If the shared
object is missing (or was built for another ABI) importing a kernel entry point raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FS_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "libfs_hip.so")     # FS_LIB: A/B builds (tools/)
ABI_VERSION = 28

_lib = None

_c_int, _c_dbl, _c_vp, _c_sz = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
_P = ctypes.POINTER

# name -> argtypes (restype is int unless stated); mirrors include/fs_hip.h declaration by declaration
_ROWS = [_c_int, _c_int]
_PROTOS = {
    "fs_abi_version": [],
    "fs_device_count": [_P(_c_int)],
    "fs_tile_list_stats": [_c_vp, _P(_c_int), _P(_c_int)],
    "fs_create": [_P(_c_vp), _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int],
    "fs_destroy": [_c_vp],
    "fs_sync": [_c_vp],
    "fs_ctx_info": [_c_vp] + [_P(_c_int)] * 7,
    "fs_upload_mask": [_c_vp, _c_vp],
    "fs_upload_bc_const": [_c_vp, _c_vp],
    "fs_upload_bc_dye": [_c_vp, _c_vp],
    "fs_bc_radius": [_c_vp, _P(_c_int), _P(_c_int)],
    "fs_field_alloc": [_c_vp, _c_int, _P(_c_vp)],
    "fs_field_free": [_c_vp],
    "fs_field_fill": [_c_vp, _c_dbl],
    "fs_field_nchan": [_c_vp],
    "fs_field_upload": [_c_vp, _c_vp, _c_int, _c_int],
    "fs_field_download": [_c_vp, _c_vp, _c_int, _c_int],
    "fs_field_copy": [_c_vp, _c_vp],
    "fs_field_devptr": [_c_vp, _P(_c_vp), _P(_c_sz)],
    "fs_velocity_bc": [_c_vp, _c_vp] + _ROWS,
    "fs_velocity_bc_limit_ok": [_c_vp, _P(_c_int)],
    "fs_velocity_bc_limit": [_c_vp, _c_dbl, _c_vp, _c_int, _c_int, _c_int] + _ROWS,
    "fs_dye_bc_limit_ok": [_c_vp, _P(_c_int)],
    "fs_dye_bc_limit": [_c_vp, _c_dbl, _c_vp, _c_vp, _c_int, _c_int] + _ROWS,
    "fs_pressure_bc": [_c_vp, _c_vp] + _ROWS,
    "fs_dye_bc": [_c_vp, _c_vp] + _ROWS,
    "fs_mac_update": [_c_vp, _c_int, _c_dbl, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_mac_dye": [_c_vp, _c_int, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_cip_set_grad": [_c_vp, _c_dbl, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_cip_nonadv": [_c_vp, _c_dbl, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_cip_nonadv_dye": [_c_vp, _c_dbl, _c_dbl, _c_dbl, _c_vp, _c_vp] + _ROWS,
    "fs_cip_nonadv_grad": [_c_vp, _c_dbl] + [_c_vp] * 6 + _ROWS,
    "fs_cip_advect": [_c_vp, _c_dbl, _c_dbl] + [_c_vp] * 7 + _ROWS,
    "fs_cip_grad_advect": [_c_vp, _c_dbl, _c_dbl] + [_c_vp] * 7 + [_c_int] + _ROWS,
    "fs_cip_step_ok": [_c_vp, _P(_c_int)],
    "fs_cip_step_tiles": [_c_vp] + [_P(_c_int)] * 5,
    "fs_cip_step": [_c_vp, _c_dbl, _c_dbl, _c_dbl] + [_c_vp] * 8 + [_c_int] + _ROWS,
    "fs_cip_step_dye": [_c_vp, _c_dbl, _c_dbl, _c_dbl] + [_c_vp] * 8 + [_c_int, _c_int] + _ROWS,
    "fs_cip_grad_advect_dye": [_c_vp, _c_dbl, _c_dbl] + [_c_vp] * 8 + [_c_int, _c_int] + _ROWS,
    "fs_vort_calc": [_c_vp, _c_dbl, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_vort_add": [_c_vp, _c_dbl, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_vort_confine": [_c_vp, _c_dbl, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_jacobi_sweep": [_c_vp, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_rbsor_halfsweep": [_c_vp, _c_dbl, _c_dbl, _c_dbl, _c_int, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_rbsor_iteration": [_c_vp, _c_dbl, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_poisson_source": [_c_vp, _c_dbl, _c_dbl, _c_vp, _c_vp] + _ROWS,
    "fs_jacobi_sweep_src": [_c_vp, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_lazy_bc_ok": [_c_vp, _P(_c_int)],
    "fs_jacobi_sweep_lazy": [_c_vp, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_jacobi_pair_lazy": [_c_vp, _c_vp, _c_vp, _c_vp, _c_int] + _ROWS,
    "fs_jacobi_quad_ok": [_c_vp, _P(_c_int)],
    "fs_jacobi_quad_lazy": [_c_vp, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_jacobi_finish": [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_lazy_flags": [_c_vp, _c_vp, _c_int, _P(_c_int), _P(_c_int), _P(_c_int)],
    "fs_selftest_f64div": [_c_vp, _c_dbl, _P(_c_int)],
    "fs_rbsor_pair_ok": [_c_vp, _P(_c_int)],
    "fs_rbsor_pair": [_c_vp, _c_dbl, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int] + _ROWS,
    "fs_rbsor_halfsweep_src": [_c_vp, _c_dbl, _c_int, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_poisson_residual": [_c_vp, _c_dbl, _c_dbl, _c_vp, _c_vp, _P(_c_dbl), _P(_c_dbl)],
    "fs_flow_stats": [_c_vp, _c_dbl, _c_vp, _c_vp, _P(_c_int), _P(_c_dbl)],
    "fs_history_create": [_c_vp, _c_int, _P(_c_int), _c_int, _P(_c_int), _c_int, _c_int, _P(_c_vp)],
    "fs_history_record": [_c_vp, _c_vp, _c_dbl, _c_dbl, _c_vp, _c_vp],
    "fs_history_read": [_c_vp, _c_vp, _P(_c_dbl), _c_int, _P(_c_int), _P(ctypes.c_longlong), _P(_c_int)],
    "fs_history_free": [_c_vp, _c_vp],
    "fs_loads_create": [_c_vp, _c_int, _P(_c_int), _P(_c_dbl), _c_int, ctypes.c_longlong, ctypes.c_longlong, _P(_c_vp)],
    "fs_loads_record": [_c_vp, _c_vp, _c_dbl, _c_dbl, _c_dbl, _c_vp, _c_vp],
    "fs_loads_read": [_c_vp, _c_vp, _P(_c_dbl), _c_int, _P(_c_int), _P(ctypes.c_longlong), _P(ctypes.c_longlong), _P(_c_int)],
    "fs_loads_sums_read": [_c_vp, _c_vp, _P(_c_dbl)],
    "fs_loads_sums_write": [_c_vp, _c_vp, _P(_c_dbl), ctypes.c_longlong, ctypes.c_longlong],
    "fs_loads_reset": [_c_vp, _c_vp],
    "fs_loads_free": [_c_vp, _c_vp],
    "fs_mean_create": [_c_vp, ctypes.c_longlong, ctypes.c_longlong, _P(_c_vp)],
    "fs_mean_accumulate": [_c_vp, _c_vp, _c_dbl, _c_vp, _c_vp],
    "fs_mean_finalize": [_c_vp, _c_vp, _c_vp, _c_vp],
    "fs_mean_read": [_c_vp, _c_vp, _P(_c_dbl), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_mean_write": [_c_vp, _c_vp, _P(_c_dbl), ctypes.c_longlong, ctypes.c_longlong],
    "fs_mean_reset": [_c_vp, _c_vp],
    "fs_mean_free": [_c_vp, _c_vp],
    "fs_diag_rows": [_c_vp] + [_P(_c_int)] * 3,
    "fs_modes_create": [_c_vp, _c_int, _P(_c_dbl), ctypes.c_longlong, ctypes.c_longlong, _P(_c_vp)],
    "fs_modes_accumulate": [_c_vp, _c_vp, _c_dbl, _c_vp, _c_vp],
    "fs_modes_combine": [_c_vp, _c_vp, _P(_c_dbl), _c_vp, _c_vp],
    "fs_modes_read": [_c_vp, _c_vp, _P(_c_dbl), _P(_c_dbl), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_modes_write": [_c_vp, _c_vp, _P(_c_dbl), _P(_c_dbl), ctypes.c_longlong, ctypes.c_longlong],
    "fs_modes_reset": [_c_vp, _c_vp],
    "fs_modes_free": [_c_vp, _c_vp],
    "fs_modes_rows": [_c_vp, _c_int, _P(_c_int), _P(_c_int)],
    "fs_pod_create": [_c_vp, _c_int, ctypes.c_longlong, ctypes.c_longlong, _P(_c_vp)],
    "fs_pod_launch": [_c_vp, _c_vp, _c_dbl, _c_vp, _c_vp],
    "fs_pod_gram": [_c_vp, _c_vp, _P(_c_dbl), _c_int, _P(_c_int), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_pod_combine": [_c_vp, _c_vp, _P(_c_dbl), _c_vp, _c_vp],
    "fs_pod_read": [_c_vp, _c_vp, _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_pod_get": [_c_vp, _c_vp, _c_vp],
    "fs_pod_set": [_c_vp, _c_vp, _c_vp, ctypes.c_longlong, ctypes.c_longlong],
    "fs_pod_reset": [_c_vp, _c_vp],
    "fs_pod_free": [_c_vp, _c_vp],
    "fs_vortex_create": [_c_vp, _c_int, _c_dbl, _c_dbl, ctypes.c_longlong, ctypes.c_longlong, _c_int, _c_int, _c_int, _c_int, _P(_c_vp)],
    "fs_vortex_launch": [_c_vp, _c_vp, _c_dbl, _c_dbl, _c_vp],
    "fs_vortex_read": [_c_vp, _c_vp, _P(ctypes.c_longlong), _c_int, _P(_c_int), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_vortex_get_labels": [_c_vp, _c_vp, _P(ctypes.c_ubyte), _P(_c_int)],
    "fs_vortex_set": [_c_vp, _c_vp, ctypes.c_longlong],
    "fs_vortex_label": [_c_vp, _P(ctypes.c_ubyte), _P(_c_int)],
    "fs_vortex_criterion": [_c_vp, _c_int, _c_dbl, _c_dbl, _c_vp, _P(_c_dbl)],
    "fs_vortex_free": [_c_vp, _c_vp],
    "fs_dist_create": [_c_vp, _c_int, _c_vp, ctypes.c_longlong, ctypes.c_longlong, _P(_c_vp)],
    "fs_dist_launch": [_c_vp, _c_vp, _c_dbl, _c_dbl, _c_vp, _c_vp],
    "fs_dist_read": [_c_vp, _c_vp, _c_int, _P(ctypes.c_longlong), _P(ctypes.c_longlong), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_dist_get": [_c_vp, _c_vp, _P(ctypes.c_longlong)],
    "fs_dist_set": [_c_vp, _c_vp, _P(ctypes.c_longlong), ctypes.c_longlong, ctypes.c_longlong],
    "fs_dist_reset": [_c_vp, _c_vp],
    "fs_dist_free": [_c_vp, _c_vp],
    "fs_dist_select": [_c_vp, _c_int, _P(_c_int), _c_dbl, _c_dbl, _c_vp, _c_vp, _P(ctypes.c_longlong), _c_int, _P(_c_dbl), _P(ctypes.c_longlong),
                       _P(ctypes.c_longlong)],
    "fs_spec_create": [_c_vp, _P(_c_int)] + [_P(_c_dbl)] * 4 + [_c_dbl, _c_dbl, _c_int, ctypes.c_longlong, ctypes.c_longlong, _P(_c_vp)],
    "fs_spec_launch": [_c_vp, _c_vp, _c_dbl, _c_vp],
    "fs_spec_read": [_c_vp, _c_vp, _P(_c_dbl), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_spec_plane": [_c_vp, _c_vp, _P(_c_dbl)],
    "fs_spec_get": [_c_vp, _c_vp, _P(_c_dbl), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_spec_set": [_c_vp, _c_vp, _P(_c_dbl), ctypes.c_longlong, ctypes.c_longlong],
    "fs_spec_reset": [_c_vp, _c_vp],
    "fs_spec_free": [_c_vp, _c_vp],
    "fs_xspec_create": [_c_vp, _P(_c_int), _c_int, _c_int, _c_dbl] + [_P(_c_dbl)] * 4 + [_c_dbl, _c_dbl, _c_int, ctypes.c_longlong, ctypes.c_longlong, _P(_c_vp)],
    "fs_xspec_launch": [_c_vp, _c_vp, _c_dbl, _c_vp, _c_vp],
    "fs_xspec_read": [_c_vp, _c_vp, _P(_c_dbl), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_xspec_plane": [_c_vp, _c_vp, _P(_c_dbl)],
    "fs_xspec_get": [_c_vp, _c_vp, _P(_c_dbl), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_xspec_set": [_c_vp, _c_vp, _P(_c_dbl), ctypes.c_longlong, ctypes.c_longlong],
    "fs_xspec_reset": [_c_vp, _c_vp],
    "fs_xspec_free": [_c_vp, _c_vp],
    "fs_flux_create": [_c_vp, _P(_c_int), _c_int, _P(_c_int), _c_dbl, ctypes.c_longlong, ctypes.c_longlong, _P(_c_vp)],
    "fs_flux_launch": [_c_vp, _c_vp, _c_dbl, _c_vp],
    "fs_flux_read": [_c_vp, _c_vp, _P(_c_dbl), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_flux_filtered": [_c_vp, _c_vp, _c_int, _P(_c_dbl)],
    "fs_flux_get": [_c_vp, _c_vp, _P(_c_dbl), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_flux_set": [_c_vp, _c_vp, _P(_c_dbl), ctypes.c_longlong, ctypes.c_longlong],
    "fs_flux_reset": [_c_vp, _c_vp],
    "fs_flux_free": [_c_vp, _c_vp],
    "fs_budget_create": [_c_vp, _c_int, _c_int, _c_int, _c_int, _c_dbl, ctypes.c_longlong, ctypes.c_longlong, _P(_c_vp)],
    "fs_budget_launch": [_c_vp, _c_vp, _c_dbl, _c_vp, _c_vp],
    "fs_budget_read": [_c_vp, _c_vp, _P(_c_dbl), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_budget_get": [_c_vp, _c_vp, _P(_c_dbl), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_budget_set": [_c_vp, _c_vp, _P(_c_dbl), ctypes.c_longlong, ctypes.c_longlong],
    "fs_budget_reset": [_c_vp, _c_vp],
    "fs_budget_free": [_c_vp, _c_vp],
    "fs_flowmap_create": [_c_vp, _P(_c_int), _c_int, _P(_c_vp)],
    "fs_flowmap_advance": [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_int],
    "fs_flowmap_cauchy_green": [_c_vp, _c_vp],
    "fs_flowmap_get": [_c_vp, _c_vp, _P(_c_dbl), _P(_c_dbl), _P(_c_int), _P(_c_dbl)],
    "fs_flowmap_reset": [_c_vp, _c_vp],
    "fs_flowmap_free": [_c_vp, _c_vp],
    "fs_mg_create": [_c_vp, _c_int, _P(_c_int), _c_vp, _c_vp, _c_vp, ctypes.c_longlong, _c_int, _c_int, _P(_c_vp)],
    "fs_mg_cycle": [_c_vp, _c_vp, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp],
    "fs_mg_info": [_c_vp, _c_vp, _P(_c_int), _P(_c_int), _P(_c_int)],
    "fs_mg_set_direct": [_c_vp, _c_vp, _c_int, _P(_c_int), _c_vp, ctypes.c_longlong],
    "fs_mg_direct_info": [_c_vp, _c_vp, _P(_c_int), _P(_c_int)],
    "fs_mg_free": [_c_vp, _c_vp],
    "fs_tracer_create": [_c_vp, _c_int, _P(_c_dbl), _c_int, _c_int, _P(_c_vp)],
    "fs_tracer_advance": [_c_vp, _c_vp, _c_dbl, _c_dbl, _c_vp],
    "fs_tracer_read": [_c_vp, _c_vp, _P(_c_dbl), _P(_c_int), _P(ctypes.c_longlong)],
    "fs_tracer_write": [_c_vp, _c_vp, _P(_c_dbl), _P(_c_int), ctypes.c_longlong],
    "fs_tracer_draw": [_c_vp, _c_vp, _c_dbl, _c_dbl, _c_dbl, _c_vp],
    "fs_tracer_sort": [_c_vp, _c_vp],
    "fs_tracer_order": [_c_vp, _c_vp, _P(_c_int)],
    "fs_tracer_fields": [_c_vp, _c_vp, _P(_c_int), _P(ctypes.c_longlong)],
    "fs_tracer_free": [_c_vp, _c_vp],
    "fs_tracer_create_inertial": [_c_vp, _c_int, _P(_c_dbl), _P(_c_dbl), _P(_c_dbl), _c_dbl, _c_dbl, _c_int, _c_int, _c_int, _P(_c_vp)],
    "fs_tracer_read_vel": [_c_vp, _c_vp, _P(_c_dbl)],
    "fs_tracer_write_vel": [_c_vp, _c_vp, _P(_c_dbl)],
    "fs_tracer_deposits": [_c_vp, _c_vp, _P(_c_int)],
    "fs_tracer_deposits_write": [_c_vp, _c_vp, _P(_c_int)],
    "fs_tracer_accum_create": [_c_vp, _c_vp, ctypes.c_longlong, ctypes.c_longlong],
    "fs_tracer_accum_add": [_c_vp, _c_vp],
    "fs_tracer_accum_read": [_c_vp, _c_vp, _P(ctypes.c_longlong), _P(ctypes.c_longlong), _P(ctypes.c_longlong), _P(ctypes.c_longlong)],
    "fs_tracer_accum_write": [_c_vp, _c_vp, _P(ctypes.c_longlong), _P(ctypes.c_longlong), ctypes.c_longlong, ctypes.c_longlong],
    "fs_tracer_accum_reset": [_c_vp, _c_vp],
    "fs_tracer_accum_free": [_c_vp, _c_vp],
    "fs_limit_field": [_c_vp, _c_dbl, _c_vp] + _ROWS,
    "fs_clamp_field": [_c_vp, _c_dbl, _c_dbl, _c_vp] + _ROWS,
    "fs_cip_advect_dye_clamped": [_c_vp, _c_dbl, _c_dbl] + [_c_vp] * 7 + _ROWS,
    "fs_clamp_inflow": [_c_vp, _c_dbl, _c_dbl, _c_vp] + _ROWS,
    "fs_vis_norm": [_c_vp, _c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_vis_pressure": [_c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_vis_vorticity": [_c_vp, _c_dbl, _c_vp, _c_vp] + _ROWS,
    "fs_vis_dye": [_c_vp, _c_vp, _c_vp] + _ROWS,
    "fs_comm_available": [_P(_c_int)],
    "fs_comm_unique_id": [_c_vp],
    "fs_comm_init": [_c_vp, _c_int, _c_int, _c_vp],
    "fs_comm_destroy": [_c_vp],
    "fs_halo_exchange": [_c_vp, _c_vp, _c_int],
    "fs_halo_exchange_multi": [_c_vp, _P(_c_vp), _c_int, _c_int],
    "fs_halo_exchange_self": [_c_vp, _P(_c_vp), _c_int, _c_int],
    "fs_halo_exchange_begin": [_c_vp, _P(_c_vp), _c_int, _c_int],
    "fs_halo_exchange_begin_partial": [_c_vp, _P(_c_vp), _P(_c_int), _c_int, _c_int],
    "fs_halo_exchange_wait": [_c_vp],
    "fs_comm_set_overlap": [_c_vp, _c_int],
    "fs_halo_exchange_mark": [_c_vp],
    "fs_comm_loopback": [_c_vp, _c_int],
    "fs_allreduce_sum": [_c_vp, _P(_c_dbl), _c_int],
    "fs_graph_begin": [_c_vp],
    "fs_graph_end": [_c_vp, _P(_c_int)],
    "fs_graph_launch": [_c_vp, _c_int, _c_int],
    "fs_graph_free": [_c_vp, _c_int],
    "fs_tape_begin": [_c_vp, _c_int],
    "fs_tape_end": [_c_vp, _P(_c_int)],
    "fs_tape_length": [_c_vp, _c_int, _P(_c_int)],
    "fs_tape_replay": [_c_vp, _c_int, _c_int],
    "fs_tape_free": [_c_vp, _c_int],
    "fs_field_hot": [_c_vp, _P(_c_int)],
    "fs_box_rates": [_c_vp, _c_sz, _c_dbl, _P(_c_dbl), _P(_c_dbl)],
    "fs_box_valu_rate": [_c_vp, _c_dbl, _P(_c_dbl)],
    "fs_box_valu_pk_rate": [_c_vp, _c_dbl, _P(_c_dbl)],
    "fs_box_mixed_rate": [_c_vp, _c_sz, _c_dbl, _P(_c_dbl)],
    "fs_prof_enable": [_c_vp, _c_int],
    "fs_span_begin": [_c_vp],
    "fs_span_end": [_c_vp, _P(_c_dbl)],
    "fs_prof_reset": [_c_vp],
    "fs_prof_count": [_c_vp, _P(_c_int)],
    "fs_prof_get": [_c_vp, _c_int, ctypes.c_char_p, _c_int, _P(_c_int), _P(_c_dbl)],
    "fs_prof_kernels": [_c_vp, ctypes.c_char_p, ctypes.c_char_p, _c_int, _P(_c_int)],
}
EXPORTS = sorted(list(_PROTOS) + ["fs_last_error"])


class FsError(RuntimeError):
    """Raised for any non-zero status of a libfs_hip call (HIP / RCCL errors included)."""


def load():
    """Load libfs_hip.so (once) and attach prototypes.  Fails loudly when the extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FsError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C 2d-fluid-simulator_amd/csrc`.")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, argtypes in _PROTOS.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _c_int
    lib.fs_last_error.argtypes = []
    lib.fs_last_error.restype = ctypes.c_char_p
    if lib.fs_abi_version() != ABI_VERSION:
        raise FsError(f"libfs_hip ABI {lib.fs_abi_version()} != expected {ABI_VERSION}; rebuild the extension")
    _lib = lib
    return lib


def check(status):
    if status != 0:
        msg = load().fs_last_error()
        raise FsError(f"libfs_hip status {status}: {msg.decode() if msg else '?'}")


def call(name, *args):
    check(getattr(load(), name)(*args))
