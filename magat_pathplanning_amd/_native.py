"""ctypes binding of libmagat_hip.so (C ABI declared in include/magat_hip.h).

There is no CPU or torch fallback behind this module: if the shared library is missing or a
call returns an error code, a MagatNativeError is raised.
"""
import ctypes
import os
import threading

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MAGAT_LIB_PATH") or os.path.join(PKG, "lib", "libmagat_hip.so")   # override: A/B builds

MODE_KEYQUERY = 0
MODE_GAT_MODIFIED = 1
MODE_GAT_ORIGIN = 2
MODE_GNN = 3
MODE_SIMILARITY = 4
_MODE_IDS = {"KeyQuery": MODE_KEYQUERY, "GAT_modified": MODE_GAT_MODIFIED, "GAT_origin": MODE_GAT_ORIGIN,
             "GAT_Similarity": MODE_SIMILARITY}
TAGS = {0: "untagged", 1: "conv_first", 2: "layer1.conv1", 3: "layer1.conv2+ds", 4: "layer2.conv1",
        5: "layer2.conv2+ds", 6: "layer3.conv1", 7: "layer3.conv2+ds", 8: "head(avgpool+fc+linear)",
        9: "compressMLP", 10: "gat_maps_gemm", 11: "gat_graph", 12: "actionsMLP", 13: "head_mean",
        14: "gat_pack", 15: "gso_prepare", 16: "gat_prepare", 17: "range_guard", 18: "layer1.conv2+layer2 (fused)", 19: "gat_layer (one launch)", 20: "gso_to_csr", 21: "gat_cast", 22: "layer3 (fused, pooled)", 23: "layer1.conv2+layer2+layer3 (fused, pooled)", 24: "conv_wgrad", 25: "gnn_dense", 26: "sim_guided", 27: "sim_expert", 28: "sim_mapf", 29: "sim_mapf_lns", 30: "sim_mapf_audit", 31: "sim_mapf_cbs", 32: "sim_mapf_ecbs", 33: "head_loss", 35: "gso_edges"}
TAG_ACTIONS = 12
# magat_form_count ids (include/magat_hip.h MAGAT_FORM_*)
FORMS = {"head_longk": 0, "head_splitk": 1, "gat_pack": 2, "gat_persist": 3, "gat_hsplit": 4, "chain_persist": 5,
         "head_compress": 6, "guard_one": 7, "csr_fused": 8, "gat_mid": 9, "chain_lat": 10, "head_lat": 11, "guard_lat": 12, "stem_lat": 13, "actions_tail": 14, "gnn_dense": 15, "sim_guided": 16, "sim_expert": 17, "sim_mapf": 18, "sim_mapf_lns": 19, "sim_mapf_audit": 20, "sim_mapf_cbs": 21, "sim_mapf_ecbs": 22,
         "chain_tile16": 23, "sim_replay": 24, "gat_cos_train": 25, "gso_edges": 26}
TAG_GNN_DENSE = 25
TAG_SIM_GUIDED = 26
TAG_SIM_EXPERT = 27
TAG_SIM_MAPF = 28
TAG_SIM_MAPF_LNS = 29
TAG_SIM_MAPF_AUDIT = 30
TAG_SIM_MAPF_CBS = 31
TAG_SIM_MAPF_ECBS = 32
TAG_HEAD_LOSS = 33
TAG_GSO_EDGES = 35          # (34 is unassigned: csrc/magat_common.h)
GUIDE_LOCAL, GUIDE_GLOBAL, GUIDE_SEMI = 1, 2, 3      # include/magat_hip.h MAGAT_GUIDE_*

_lock = threading.Lock()
_lib = None


class MagatNativeError(RuntimeError):
    pass


class ConvGemmDesc(ctypes.Structure):
    _fields_ = [("inp", ctypes.c_void_p), ("in2", ctypes.c_void_p), ("wt", ctypes.c_void_p),
                ("bias", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("in_pix_stride", ctypes.c_int64), ("in2_pix_stride", ctypes.c_int64),
                ("out_pix_stride", ctypes.c_int64), ("M", ctypes.c_int),
                ("Cin", ctypes.c_int), ("lda", ctypes.c_int), ("Hin", ctypes.c_int), ("Win", ctypes.c_int),
                ("kH", ctypes.c_int), ("kW", ctypes.c_int), ("stride", ctypes.c_int), ("pad", ctypes.c_int),
                ("Hout", ctypes.c_int), ("Wout", ctypes.c_int),
                ("C2", ctypes.c_int), ("lda2", ctypes.c_int), ("W2", ctypes.c_int), ("stride2", ctypes.c_int),
                ("Cout", ctypes.c_int), ("ldc", ctypes.c_int), ("relu", ctypes.c_int), ("tag", ctypes.c_int),
                ("pool", ctypes.c_int), ("pool_w", ctypes.c_int),
                ("in_fmt", ctypes.c_int), ("out_fmt", ctypes.c_int),
                ("in_plane_stride", ctypes.c_int64), ("in2_plane_stride", ctypes.c_int64),
                ("out_plane_stride", ctypes.c_int64),
                ("in_tile_stride", ctypes.c_int64), ("in2_tile_stride", ctypes.c_int64),
                ("out_tile_stride", ctypes.c_int64),
                ("in_gl", ctypes.c_int), ("out_gl", ctypes.c_int), ("out_ntile_stride", ctypes.c_int64),
                ("wt_pix_stride", ctypes.c_int64), ("ldw", ctypes.c_int),
                ("range_flag", ctypes.c_void_p), ("run_if", ctypes.c_void_p),
                ("in_scale", ctypes.c_void_p), ("acc_scale", ctypes.c_void_p), ("absmax", ctypes.c_void_p),
                ("bf16_rows", ctypes.c_int),
                ("wt2", ctypes.c_void_p), ("bias2", ctypes.c_void_p), ("out2", ctypes.c_void_p), ("in_scale2", ctypes.c_void_p),
                ("Cout2", ctypes.c_int), ("ldc2", ctypes.c_int), ("relu2", ctypes.c_int),
                ("out2_bf16", ctypes.c_void_p), ("ldc2_bf16", ctypes.c_int), ("dilation", ctypes.c_int)]


class EncoderDesc(ctypes.Structure):
    _fields_ = [("variant", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("n_feat", ctypes.c_int), ("n_comp", ctypes.c_int), ("pack", ctypes.c_void_p),
                ("off", ctypes.c_int64 * 32), ("chain_off", ctypes.c_int64), ("chain3_off", ctypes.c_int64),
                ("head16_off", ctypes.c_int64), ("comp16_off", ctypes.c_int64), ("scaled_off", ctypes.c_int64),
                ("l1frag_off", ctypes.c_int64), ("form_agents", ctypes.c_int), ("comp_bf16", ctypes.c_void_p),
                ("headfrag_off", ctypes.c_int64), ("compfrag_off", ctypes.c_int64)]


class SimStepDesc(ctypes.Structure):
    """magat_sim_step_desc (include/magat_hip.h)."""
    _fields_ = [("logits", ctypes.c_void_p), ("actions_in", ctypes.c_void_p), ("map", ctypes.c_void_p),
                ("map_batched", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("B", ctypes.c_int32),
                ("N", ctypes.c_int32), ("policy", ctypes.c_int32), ("uniforms", ctypes.c_void_p), ("pos", ctypes.c_void_p),
                ("goal", ctypes.c_void_p), ("reach_goal", ctypes.c_void_p), ("first_move", ctypes.c_void_p),
                ("end_step", ctypes.c_void_p), ("currentstep", ctypes.c_int32), ("maxstep", ctypes.c_int32),
                ("actions_out", ctypes.c_void_p), ("moves_out", ctypes.c_void_p), ("flags_out", ctypes.c_void_p),
                ("done_out", ctypes.c_void_p), ("flowtime_out", ctypes.c_void_p), ("makespan_out", ctypes.c_void_p)]


class SimHistoryDesc(ctypes.Structure):
    """magat_sim_history_desc (include/magat_hip.h)."""
    _fields_ = [("row_case", ctypes.c_void_p), ("row_step", ctypes.c_void_p), ("pos_table", ctypes.c_void_p),
                ("cells", ctypes.c_void_p), ("lengths", ctypes.c_void_p), ("goal", ctypes.c_void_p),
                ("cases", ctypes.c_int32), ("T", ctypes.c_int32), ("Lcap", ctypes.c_int32)]


class SimPoolDesc(ctypes.Structure):
    """magat_sim_pool_desc (include/magat_hip.h)."""
    _fields_ = [("q_map", ctypes.c_void_p), ("q_start", ctypes.c_void_p), ("q_goal", ctypes.c_void_p),
                ("q_maxstep", ctypes.c_void_p), ("map_batched", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("C", ctypes.c_int32), ("B", ctypes.c_int32), ("N", ctypes.c_int32), ("first_step", ctypes.c_int32),
                ("record", ctypes.c_int32), ("traj_cells", ctypes.c_int32), ("radius_max_steps", ctypes.c_int32),
                ("comm_radius", ctypes.c_double), ("slot_case", ctypes.c_void_p), ("slot_step", ctypes.c_void_p),
                ("slot_maxstep", ctypes.c_void_p), ("over", ctypes.c_void_p), ("sticky", ctypes.c_void_p),
                ("map", ctypes.c_void_p), ("pos", ctypes.c_void_p), ("goal", ctypes.c_void_p), ("reach_goal", ctypes.c_void_p),
                ("first_move", ctypes.c_void_p), ("end_step", ctypes.c_void_p), ("done", ctypes.c_void_p),
                ("flowtime", ctypes.c_void_p), ("makespan", ctypes.c_void_p), ("radii", ctypes.c_void_p),
                ("agent_view", ctypes.c_void_p), ("agent_view_bytes", ctypes.c_int64), ("counters", ctypes.c_void_p),
                ("rows", ctypes.c_void_p), ("r_radius", ctypes.c_void_p), ("r_end_pos", ctypes.c_void_p),
                ("r_first_move", ctypes.c_void_p), ("r_end_step", ctypes.c_void_p), ("traj", ctypes.c_void_p),
                ("traj_len", ctypes.c_void_p)]


# columns of magat_sim_pool_desc.rows (include/magat_hip.h MAGAT_POOL_*)
POOL_COLUMNS = ("retired", "all_reach", "num_reach", "steps", "makespan", "flowtime", "predicted_collision", "flag_bits", "status")
POOL_STATUS_DISCONNECTED = 2

_I, _P, _Z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
_SIGNATURES = {
    "magat_abi_version": (ctypes.c_int, []),
    "magat_build_flavor": (ctypes.c_int, []),
    "magat_error_string": (ctypes.c_char_p, [_I]),
    "magat_set_option": (_I, [ctypes.c_char_p, _I]),
    "magat_get_option": (_I, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
    "magat_reset_option": (_I, [ctypes.c_char_p]),
    "magat_gat_dense_supported": (_I, [_I] * 3),
    "magat_gat_one_launch_supported": (_I, [_I] * 6),
    "magat_gat_packed_floats": (_Z, [_I] * 5),
    "magat_gat_pack_weights": (_I, [_P] * 5 + [_I] * 5 + [_P]),
    "magat_gat_workspace_bytes": (_Z, [_I] * 8),
    "magat_gat_forward_packed_f32": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _Z] + [_I] * 8 + [_P]),
    "magat_gat_forward_planned_f32": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _Z] + [_I] * 8 + [_P, _P]),
    "magat_gat_forward_tail_f32": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _Z] + [_I] * 8 + [_P, _P, _P]),
    "magat_gat_forward_dense_f32": (_I, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _Z] + [_I] * 8 + [_P]),
    "magat_gat_csr_workspace_bytes": (_Z, [_I, _I, ctypes.c_longlong] + [_I] * 6),
    "magat_gat_forward_csr_f32": (_I, [_P, _P, _P, ctypes.c_longlong, _P, _P, _P, _I, _P, _P, _Z] + [_I] * 8 + [_P]),
    "magat_gnn_forward_csr_f32": (_I, [_P, _P, _P, _P, ctypes.c_longlong, _P, _P, _P, _I, _P, _Z] + [_I] * 5 + [_P]),
    "magat_gnn_dense_supported": (_I, [_I] * 4),
    "magat_gnn_forward_dense_f32": (_I, [_P, _I, _P, _I, _P, _P, _P, _I] + [_I] * 7 + [_P]),
    "magat_gat_csr_bf16_workspace_bytes": (_Z, [_I, _I, ctypes.c_longlong] + [_I] * 6),
    "magat_gat_csc_workspace_bytes": (_Z, [_I, _I, ctypes.c_longlong] + [_I] * 7),
    "magat_gat_forward_csr_bf16": (_I, [_P, _P, _P, ctypes.c_longlong, _P, _P, _P, _I, _P, _P, _Z] + [_I] * 8 + [_P]),
    "magat_gat_train_forward_f32": (_I, [_P, _P, _P, ctypes.c_longlong] + [_P] * 10 + [_I] * 7 + [_P]),
    "magat_gat_train_backward_f32": (_I, [_P] * 10 + [ctypes.c_longlong] + [_P] * 3 + [_I] * 7 + [_P]),
    "magat_gat_train_forward_cos_f32": (_I, [_P, _P, _P, ctypes.c_longlong] + [_P] * 12 + [_I] * 4 + [_P]),
    "magat_gat_train_backward_cos_f32": (_I, [_P] * 11 + [ctypes.c_longlong] + [_P] * 3 + [_I] * 4 + [_P]),
    "magat_gso_csr_workspace_bytes": (_Z, [_I, _I]),
    "magat_gso_csr_build": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, ctypes.c_longlong, _P, _P, _Z, _I, _I, _P]),
    "magat_gso_csr_build_phase": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, ctypes.c_longlong, _P, _P, _Z, _I, _I, _I, _P]),
    "magat_gso_edges_workspace_bytes": (_Z, [_I, _I]),
    "magat_gso_edges_build": (_I, [_P, _P, ctypes.c_double, _I, _P, _P, _P, _P, _P, ctypes.c_longlong, _P, _P, _Z, _I, _I, _P]),
    "magat_gso_edge_values_workspace_bytes": (_Z, [_I, _I]),
    "magat_gso_edge_values": (_I, [_P, _P, _P, ctypes.c_longlong, _I, _I, _P, _P, _P, _Z, _I, _I, _P]),
    "magat_gat_forward_csc_f32": (_I, [_P] * 6 + [ctypes.c_longlong, _P, _P, _P, _I, _P, _P, _Z] + [_I] * 8 + [_P]),
    "magat_gat_forward_csc_bf16": (_I, [_P] * 6 + [ctypes.c_longlong, _P, _P, _P, _I, _P, _P, _Z] + [_I] * 8 + [_P]),
    "magat_gat_forward_csc_bf16_f32out": (_I, [_P] * 6 + [ctypes.c_longlong, _P, _P, _P, _I, _P, _P, _Z] + [_I] * 8 + [_P]),
    "magat_cast_rows": (_I, [_P, _P, _I, ctypes.c_longlong, _I, _I, _I, _P]),
    "magat_gso_row_degrees": (_I, [_P, _I, _I, _P, _I, _I, _P]),
    "magat_gso_fill_csr": (_I, [_P, _I, _I, _P, _P, _I, _I, _P]),
    "magat_gnn_backward_csr_f32": (_I, [_P, _P, _P, _P, ctypes.c_longlong, _P, _I, _I, _I, _I, _P]),
    "magat_sim_gso": (_I, [_P, ctypes.c_double, _I, _I, _P, _I, _P, _I, _I, _P]),
    "magat_sim_gso_radii": (_I, [_P, _P, _I, _I, _P, _I, _P, _I, _I, _P]),
    "magat_sim_connect_radius": (_I, [_P, ctypes.c_double, _P, _P, _I, _I, _I, _P]),
    "magat_sim_step": (_I, [ctypes.POINTER(SimStepDesc), _P]),
    "magat_sim_fov_states": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P]),
    "magat_sim_guided_states": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "magat_sim_move": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "magat_sim_guided_states_wide_workspace_bytes": (_Z, [_I] * 5),
    "magat_sim_guided_states_wide": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    "magat_sim_replayed_states": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _I, _I, ctypes.POINTER(SimHistoryDesc), _P]),
    "magat_sim_replayed_states_wide": (_I, [_P, _I, _I, _I, _P, _P, _P, _I, _I, _I, ctypes.POINTER(SimHistoryDesc), _P, _Z, _P]),
    "magat_sim_move_wide_workspace_bytes": (_Z, [_I] * 4),
    "magat_sim_move_wide": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P]),
    "magat_sim_step_wide": (_I, [ctypes.POINTER(SimStepDesc), _P, _Z, _P]),
    "magat_sim_pool_step": (_I, [ctypes.POINTER(SimStepDesc), _P, _P, _P, _P, _P, _P]),
    "magat_sim_pool_step_wide": (_I, [ctypes.POINTER(SimStepDesc), _P, _P, _P, _P, _P, _P, _Z, _P]),
    "magat_sim_pool_turn": (_I, [ctypes.POINTER(SimPoolDesc), _I, _P]),
    "magat_sim_pool_uniforms": (_I, [_P, _P, _P, ctypes.c_uint64, _I, _I, _P]),
    "magat_gso_prepare": (_I, [_P, _I, _Z, _I, _I, _P]),
    "magat_conv_gemm_f32": (_I, [ctypes.POINTER(ConvGemmDesc), _P]),
    "magat_conv_wgrad_workspace_floats": (_Z, [_I] * 7),
    "magat_conv_wgrad_f32": (_I, [_P, ctypes.c_longlong, _I, _P, ctypes.c_longlong, _I, _P, ctypes.POINTER(ctypes.c_int)] + [_I] * 12 + [_P]),
    "magat_bn_train_workspace_floats": (_Z, [ctypes.c_longlong, _I]),
    "magat_bn_train_forward_f32": (_I, [_P, _P, ctypes.c_longlong, _I, _P, _P, _P, _P, ctypes.c_float, ctypes.c_float, _I, _P, _P, _P, _P]),
    "magat_bn_train_backward_f32": (_I, [_P, _P, _P, _P, ctypes.c_longlong, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "magat_head_loss_workspace_floats": (_Z, [ctypes.c_longlong, _I]),
    "magat_head_loss_forward_f32": (_I, [_P, _I, _P, _P, _P, _I, ctypes.c_float, _P, _P, _P, _P, _P, ctypes.c_longlong, _I, _P]),
    "magat_head_loss_backward_f32": (_I, [_P, _P, _P, _I, _P, _P, _I, _P, _P, _P, ctypes.c_longlong, _I, _P]),
    "magat_action_loss_f32": (_I, [_P, _I, _P, _I, ctypes.c_float, _P, _P, _P, _P, ctypes.c_longlong, _P]),
    "magat_linear_f32": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "magat_linear_tagged_f32": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "magat_gat_set_debug_buffer": (_I, [_P]),
    "magat_profile_reserve": (_I, [_I]),
    "magat_profile_enable": (_I, [_I]),
    "magat_profile_collect": (_I, []),
    "magat_profile_read": (_I, [_I, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_double)]),
    "magat_profile_reset": (_I, []),
    "magat_mfma_sustained_f16": (_I, [ctypes.POINTER(ctypes.c_double), _P, _I, _P]),
    "magat_mfma_sustained_f16_ex": (_I, [ctypes.POINTER(ctypes.c_double)] * 3 + [_P, _I, _P]),
    "magat_form_count": (ctypes.c_longlong, [_I]),
    "magat_form_reset": (_I, []),
    "magat_sim_expert_schedule": (_I, [_P] * 8 + [_I] * 4 + [_P]),
    "magat_sim_expert_radius": (_I, [_P, _P, ctypes.c_double, _P, _P, _P, _I, _I, _I, _I, _P]),
    "magat_sim_expert_stats": (_I, [_P] * 9 + [_I] * 3 + [_P]),
    "magat_sim_expert_pick": (_I, [_P] * 17 + [_I] * 6 + [_P]),
    "magat_sim_mapf_workspace_bytes": (_Z, [_I, _I]),
    "magat_sim_mapf_plan": (_I, [_P, _I, _I, _I] + [_P] * 9 + [_Z, _I, _I, _I, _P]),
    "magat_sim_cases_generate": (_I, [_I, _P, _I, _I, _I, _I, _I, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64] + [_P] * 5 + [_I, _I, _P]),
    "magat_sim_mapf_wide_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "magat_sim_mapf_plan_wide": (_I, [_P, _I, _I, _I] + [_P] * 9 + [_Z, _I, _I, _I, _P]),
    "magat_sim_mapf_improve_workspace_bytes": (_Z, [_I, _I, _I]),
    "magat_sim_mapf_improve": (_I, [_P, _I, _I, _I] + [_P] * 9 + [_Z, _I, _I, _I, _I, _I, _P]),
    "magat_sim_mapf_improve_wide_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "magat_sim_mapf_improve_wide": (_I, [_P, _I, _I, _I] + [_P] * 9 + [_Z, _I, _I, _I, _I, _I, _P]),
    "magat_sim_mapf_audit_workspace_bytes": (_Z, [_I, _I, _I]),
    "magat_sim_mapf_audit": (_I, [_P, _I, _I, _I] + [_P] * 13 + [_Z, _I, _I, _I, _P]),
    "magat_sim_mapf_audit_wide_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "magat_sim_mapf_audit_wide": (_I, [_P, _I, _I, _I] + [_P] * 13 + [_Z, _I, _I, _I, _P]),
    "magat_sim_mapf_cbs_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "magat_sim_mapf_cbs": (_I, [_P, _I, _I, _I] + [_P] * 13 + [_Z, _I, _I, _I, _I, _P]),
    "magat_sim_mapf_ecbs_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "magat_sim_mapf_ecbs": (_I, [_P, _I, _I, _I] + [_P] * 13 + [_Z, _I, _I, _I, _I, _I, _I, _P]),
    "magat_sim_mapf_ecbs_wide_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I, _I]),
    "magat_sim_mapf_ecbs_wide": (_I, [_P, _I, _I, _I] + [_P] * 13 + [_Z, _I, _I, _I, _I, _I, _I, _P]),
    "magat_sim_cases_generate_wide": (_I, [_I, _P, _I, _I, _I, _I, _I, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64] + [_P] * 5 + [_I, _I, _P]),
    "magat_conv_first_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "magat_conv_first_tiled_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "magat_encoder_workspace_bytes": (_Z, [ctypes.POINTER(EncoderDesc), _I]),
    "magat_encoder_read_status": (_I, [_P, ctypes.POINTER(ctypes.c_int32), _P]),
    "magat_gat_read_status": (_I, [_P, ctypes.POINTER(ctypes.c_int32), _P]),
    "magat_encoder_forward_f32": (_I, [ctypes.POINTER(EncoderDesc), _P, _P, _I, _P, _I, _P, _Z, _I, _P]),
    "magat_encoder_stem_block_f32": (_I, [ctypes.POINTER(EncoderDesc), _P, _P, _P, _I, _I, _P, _P]),
    "magat_encoder_calibrate_f32": (_I, [ctypes.POINTER(EncoderDesc), _P, _P, _I, _P, _I, _P, _Z, _I, _P, _P]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def library_present():
    return os.path.exists(LIB_PATH)


def lib():
    """The loaded library (loaded once per process; fails loudly if it is not built)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise MagatNativeError(
                        "libmagat_hip.so is not built (%s). Run `python -m magat_pathplanning_amd.build_native` "
                        "(needs hipcc); there is no fallback path." % LIB_PATH)
                handle = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in _SIGNATURES.items():
                    fn = getattr(handle, name)
                    fn.restype, fn.argtypes = res, args
                if handle.magat_build_flavor() != 0 and os.environ.get("MAGAT_ALLOW_EXPERIMENT_BUILD", "0") != "1":
                    raise MagatNativeError(
                        "%s is an EXPERIMENT build (compiled with *_WHATIF_* timing switches: its results are wrong by "
                        "design).  Rebuild with `python -m magat_pathplanning_amd.build_native --force`; the timing probes "
                        "under tools/ set MAGAT_ALLOW_EXPERIMENT_BUILD=1." % LIB_PATH)
                _lib = handle
    return _lib


def set_option(name, value):
    """Library tunable (include/magat_hip.h "Options"); the environment variable MAGAT_<NAME> only seeds it at load."""
    check(lib().magat_set_option(name.encode(), int(value)), "magat_set_option(%s)" % name)


def get_option(name):
    v = ctypes.c_int(0)
    check(lib().magat_get_option(name.encode(), ctypes.byref(v)), "magat_get_option(%s)" % name)
    return v.value


def reset_option(name):
    check(lib().magat_reset_option(name.encode()), "magat_reset_option(%s)" % name)


def check(rc, what):
    if rc != 0:
        msg = lib().magat_error_string(rc)
        raise MagatNativeError("%s failed: %s (code %d)" % (what, msg.decode() if msg else "?", rc))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def current_stream(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def torch_composite_allowed():
    """The differentiable torch composites of the graph layers (same algebra as the pinned oracle) exist so that host-side
    tests can check state_dict / autograd semantics without a GPU.  They are NOT a product path: on CPU tensors they run
    only when MAGAT_ALLOW_TORCH_COMPOSITE=1 (tests/conftest.py sets it); otherwise the modules fail loudly."""
    return os.environ.get("MAGAT_ALLOW_TORCH_COMPOSITE", "0") == "1"


def require_device_or_composite(t, what):
    if not t.is_cuda and not torch_composite_allowed():
        raise MagatNativeError("%s: CPU tensors are not supported (no CPU fallback); the torch composite used by the host "
                               "tests needs MAGAT_ALLOW_TORCH_COMPOSITE=1" % what)
