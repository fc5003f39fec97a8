"""ctypes binding of libsdmi.so (include/sdmi.h).  No fallback: if the library is missing this raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SDMI_LIB_PATH') or os.path.join(_HERE, 'libsdmi.so')     # (override: same-box A/B of two builds)

c_f32p = C.c_void_p     # device pointers travel as integers (tensor.data_ptr())
c_ptr = C.c_void_p


class UNetCfg(C.Structure):
    _fields_ = [('in_channels', C.c_int32), ('out_channels', C.c_int32), ('model_channels', C.c_int32),
                ('num_res_blocks', C.c_int32), ('n_levels', C.c_int32), ('channel_mult', C.c_int32 * 8),
                ('n_attention_resolutions', C.c_int32), ('attention_resolutions', C.c_int32 * 8),
                ('num_heads', C.c_int32), ('transformer_depth', C.c_int32), ('context_dim', C.c_int32)]


class VaeCfg(C.Structure):
    _fields_ = [('ch', C.c_int32), ('out_ch', C.c_int32), ('n_levels', C.c_int32), ('ch_mult', C.c_int32 * 8),
                ('num_res_blocks', C.c_int32), ('in_channels', C.c_int32), ('z_channels', C.c_int32),
                ('embed_dim', C.c_int32)]


class UNetExt(C.Structure):
    _fields_ = [('attention_block', C.c_int32), ('resblock_updown', C.c_int32)]


class VaeExt(C.Structure):
    _fields_ = [('double_z', C.c_int32), ('mid_attn', C.c_int32), ('n_embed', C.c_int32)]


class ClipCfg(C.Structure):
    _fields_ = [('vocab_size', C.c_int32), ('hidden_size', C.c_int32), ('intermediate_size', C.c_int32),
                ('num_layers', C.c_int32), ('num_heads', C.c_int32), ('max_positions', C.c_int32)]


class BertCfg(C.Structure):
    _fields_ = [('vocab_size', C.c_int32), ('dim', C.c_int32), ('depth', C.c_int32), ('heads', C.c_int32),
                ('dim_head', C.c_int32), ('ff_inner', C.c_int32), ('max_seq_len', C.c_int32)]


class VitCfg(C.Structure):
    _fields_ = [('image_size', C.c_int32), ('patch_size', C.c_int32), ('hidden_size', C.c_int32), ('intermediate_size', C.c_int32),
                ('num_layers', C.c_int32), ('num_heads', C.c_int32), ('projection_dim', C.c_int32)]


class IGemmDesc(C.Structure):
    _fields_ = [('a0', c_ptr), ('a1', c_ptr), ('a2', c_ptr),
                ('c0', C.c_int32), ('c1', C.c_int32), ('c2', C.c_int32),
                ('lda0', C.c_int32), ('lda1', C.c_int32), ('lda2', C.c_int32),
                ('B', C.c_int32), ('Hin', C.c_int32), ('Win', C.c_int32), ('Hout', C.c_int32), ('Wout', C.c_int32),
                ('ksize', C.c_int32), ('stride', C.c_int32), ('up', C.c_int32),
                ('w', c_ptr), ('N', C.c_int32), ('mode', C.c_int32),
                ('bias', c_ptr), ('rowvec', c_ptr), ('ld_rowvec', C.c_int32),
                ('residual', c_ptr), ('ldr', C.c_int32),
                ('out_f32', c_ptr), ('out_f16', c_ptr), ('ldo', C.c_int32),
                ('seg_dst', c_ptr * 3), ('seg_kind', C.c_int32 * 3),
                ('heads', C.c_int32), ('dh', C.c_int32), ('ntok', C.c_int32), ('ntok_pad', C.c_int32),
                ('segC', C.c_int32), ('splitk', C.c_int32), ('splitk_ws', c_ptr), ('splitk_ws_floats', C.c_int64),
                ('tile', C.c_int32), ('dma', C.c_int32), ('asym_pad', C.c_int32),
                ('gn_n', C.c_int32), ('gn_acc', c_ptr * 2), ('gn_cpg', C.c_int32 * 2), ('gn_cbase', C.c_int32 * 2),
                ('splitk_cnt', c_ptr), ('splitk_cnt_ints', C.c_int32), ('split16', C.c_int32),
                ('f16_scale', c_ptr), ('lnp_out', c_ptr), ('lnf_part', c_ptr), ('lnf_npart', C.c_int32),
                ('lnf_eps', C.c_float), ('lnf_cs', c_ptr), ('lnf_d', c_ptr),
                ('pgn_gamma', c_ptr), ('pgn_beta', c_ptr), ('pgn_eps', C.c_float), ('pgn_silu', C.c_int32),
                ('pgn_out', c_ptr), ('pgn_keep_f32', C.c_int32), ('pgn_applied', C.POINTER(C.c_int32)),
                ('out_lo', c_ptr)]


SAMPLER_MAX_SLOTS = 8


class SamplerSlot(C.Structure):
    """sdmi_sampler_slot (include/sdmi.h): one latent of an sdmi_sampler_step_rows launch"""
    _fields_ = [('eps_u', c_ptr), ('eps_c', c_ptr), ('x', c_ptr), ('old0', c_ptr), ('old1', c_ptr), ('old2', c_ptr), ('noise', c_ptr),
                ('e_t_out', c_ptr), ('x_state_out', c_ptr), ('pred_x0', c_ptr), ('unet_dst0', c_ptr), ('unet_dst1', c_ptr),
                ('t_dst0', c_ptr), ('t_dst1', c_ptr), ('t_next', C.c_int64), ('cfg', C.c_int32), ('mode', C.c_int32),
                ('scale', C.c_float), ('a_t', C.c_float), ('a_prev', C.c_float), ('sigma', C.c_float), ('sqrt_1m_at', C.c_float),
                ('reserved', C.c_int32)]


class SamplerPlanSlot(C.Structure):
    """sdmi_sampler_plan_slot (include/sdmi.h): one latent of an sdmi_sampler_plan_rows launch"""
    _fields_ = [('eps_u', c_ptr), ('eps_c', c_ptr), ('x', c_ptr), ('old0', c_ptr), ('old1', c_ptr), ('old2', c_ptr), ('noise', c_ptr),
                ('x_base', c_ptr), ('m0', c_ptr), ('m1', c_ptr), ('m2', c_ptr), ('e_t_out', c_ptr), ('pred_x0', c_ptr), ('m_out', c_ptr),
                ('x_state_out', c_ptr), ('unet_dst0', c_ptr), ('unet_dst1', c_ptr), ('tf_dst0', c_ptr), ('tf_dst1', c_ptr),
                ('kind', C.c_int32), ('cfg', C.c_int32), ('mode', C.c_int32), ('form', C.c_int32), ('m_self', C.c_int32),
                ('data_prediction', C.c_int32), ('scale', C.c_float), ('t_next', C.c_float), ('a_t', C.c_float), ('a_prev', C.c_float),
                ('sigma', C.c_float), ('sqrt_1m_at', C.c_float), ('alpha_t', C.c_float), ('sigma_t', C.c_float), ('c9', C.c_float * 9),
                ('reserved', C.c_int32)]


_SIGS = {
    'sdmi_last_error': (C.c_char_p, []),
    'sdmi_abi_version': (C.c_int, []),
    'sdmi_unet_create': (C.c_int, [C.POINTER(UNetCfg), C.POINTER(c_ptr)]),
    'sdmi_unet_create_with_precision': (C.c_int, [C.POINTER(UNetCfg), C.c_int, C.POINTER(c_ptr)]),
    'sdmi_unet_precision': (C.c_int, [c_ptr]),
    'sdmi_unet_create_ext': (C.c_int, [C.POINTER(UNetCfg), C.POINTER(UNetExt), C.c_int, C.POINTER(c_ptr)]),
    'sdmi_unet_create_flags': (C.c_int, [C.POINTER(UNetCfg), C.POINTER(UNetExt), C.c_uint, C.c_int, C.POINTER(c_ptr)]),
    'sdmi_unet_destroy': (C.c_int, [c_ptr]),
    'sdmi_unet_num_weights': (C.c_int, [c_ptr]),
    'sdmi_unet_weight_info': (C.c_int, [c_ptr, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    'sdmi_unet_set_weight': (C.c_int, [c_ptr, C.c_char_p, c_ptr, C.POINTER(C.c_int64), C.c_int, c_ptr]),
    'sdmi_unet_finalize': (C.c_int, [c_ptr]),
    'sdmi_unet_packed_bytes': (C.c_int64, [c_ptr]),
    'sdmi_unet_export_packed': (C.c_int, [c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_unet_import_packed': (C.c_int, [c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_unet_workspace_bytes': (C.c_int64, [c_ptr, C.c_int, C.c_int, C.c_int, C.c_int]),
    'sdmi_unet_cache_context': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, c_ptr, C.c_int64, c_ptr]),
    'sdmi_unet_reserve_context': (C.c_int, [c_ptr, C.c_int, C.c_int]),
    'sdmi_unet_cache_timesteps': (C.c_int, [c_ptr, C.POINTER(C.c_int64), C.c_int, c_ptr]),
    'sdmi_unet_hint_timestep': (C.c_int, [c_ptr, C.c_int64]),
    'sdmi_unet_tape_stats': (C.c_int, [c_ptr, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'sdmi_unet_forward': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                    c_ptr, C.c_int64, c_ptr]),
    'sdmi_sampler_step': (C.c_int, [c_ptr, C.c_int, C.c_float, c_ptr, C.c_int, c_ptr, c_ptr, c_ptr, C.c_float,
                                    C.c_float, C.c_float, C.c_float, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_sampler_step_x0': (C.c_int, [c_ptr, C.c_int, C.c_float, c_ptr, C.c_int, c_ptr, c_ptr, c_ptr, C.c_float, C.c_float, c_ptr,
                                       c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_sampler_step_from_x0': (C.c_int, [c_ptr, c_ptr, C.c_float, C.c_float, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_sampler_step_rows': (C.c_int, [C.POINTER(SamplerSlot), C.c_int, C.c_int64, c_ptr]),
    'sdmi_sampler_plan_rows': (C.c_int, [C.POINTER(SamplerPlanSlot), C.c_int, C.c_int64, c_ptr]),
    'sdmi_ddpm_step': (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, c_ptr, c_ptr,
                                 c_ptr, c_ptr, C.c_float, C.c_float, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_dpm_solver_step': (C.c_int, [c_ptr, C.c_int, C.c_float, c_ptr, c_ptr, C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.c_float, C.c_int, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_dpm_model_value': (C.c_int, [c_ptr, C.c_int, C.c_float, c_ptr, C.c_int, C.c_float, C.c_float, c_ptr, C.c_int64, c_ptr,
                                       C.c_int64, c_ptr]),
    'sdmi_dpm_update': (C.c_int, [C.c_int, c_ptr, c_ptr, c_ptr, c_ptr, C.POINTER(C.c_float), c_ptr, C.c_int64, c_ptr]),
    'sdmi_dpm_threshold_scale': (C.c_int, [c_ptr, C.c_int, C.c_int64, C.c_float, c_ptr, c_ptr, c_ptr]),
    'sdmi_dpm_adaptive_error_ws_floats': (C.c_int64, [C.c_int, C.c_int64]),
    'sdmi_dpm_adaptive_error': (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_float, C.c_float, C.c_int, C.c_int64, c_ptr, C.c_int64, c_ptr, c_ptr]),
    'sdmi_vae_create': (C.c_int, [C.POINTER(VaeCfg), C.c_int, C.POINTER(c_ptr)]),
    'sdmi_vae_destroy': (C.c_int, [c_ptr]),
    'sdmi_vae_create_ext': (C.c_int, [C.POINTER(VaeCfg), C.POINTER(VaeExt), C.c_int, C.POINTER(c_ptr)]),
    'sdmi_vae_create_precision': (C.c_int, [C.POINTER(VaeCfg), C.POINTER(VaeExt), C.c_int, C.c_int, C.POINTER(c_ptr)]),
    'sdmi_vae_create_attn': (C.c_int, [C.POINTER(VaeCfg), C.POINTER(VaeExt), C.c_int, C.c_int, C.c_uint32, C.POINTER(c_ptr)]),
    'sdmi_vae_precision': (C.c_int, [c_ptr]),
    'sdmi_vae_decode_vq': (C.c_int, [c_ptr, c_ptr, C.c_float, C.c_int, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr, C.c_int64, c_ptr]),
    'sdmi_k_vq_quantize': (C.c_int, [c_ptr, C.c_float, c_ptr, c_ptr, C.c_int, C.c_int, c_ptr, c_ptr, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_patch_unfold': (C.c_int, [c_ptr, c_ptr, c_ptr] + [C.c_int] * 11 + [c_ptr]),
    'sdmi_k_patch_fold': (C.c_int, [c_ptr, c_ptr, c_ptr] + [C.c_int] * 11 + [c_ptr]),
    'sdmi_k_resample2': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_spatial_rescale': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr] + [C.c_int] * 6 + [c_ptr]),
    'sdmi_k_spatial_rescale_labels': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr] + [C.c_int] * 6 + [c_ptr]),
    'sdmi_vae_num_weights': (C.c_int, [c_ptr]),
    'sdmi_vae_weight_info': (C.c_int, [c_ptr, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    'sdmi_vae_set_weight': (C.c_int, [c_ptr, C.c_char_p, c_ptr, C.POINTER(C.c_int64), C.c_int, c_ptr]),
    'sdmi_vae_finalize': (C.c_int, [c_ptr]),
    'sdmi_vae_decode_workspace_bytes': (C.c_int64, [c_ptr, C.c_int, C.c_int, C.c_int]),
    'sdmi_vae_decode': (C.c_int, [c_ptr, c_ptr, C.c_float, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr, C.c_int64, c_ptr]),
    'sdmi_vae_encode_workspace_bytes': (C.c_int64, [c_ptr, C.c_int, C.c_int, C.c_int]),
    'sdmi_vae_encode': (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr, C.c_int64, c_ptr]),
    'sdmi_clip_create': (C.c_int, [C.POINTER(ClipCfg), C.POINTER(c_ptr)]),
    'sdmi_clip_create_precision': (C.c_int, [C.POINTER(ClipCfg), C.c_int, C.POINTER(c_ptr)]),
    'sdmi_clip_precision': (C.c_int, [c_ptr]),
    'sdmi_clip_destroy': (C.c_int, [c_ptr]),
    'sdmi_clip_num_weights': (C.c_int, [c_ptr]),
    'sdmi_clip_weight_info': (C.c_int, [c_ptr, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    'sdmi_clip_set_weight': (C.c_int, [c_ptr, C.c_char_p, c_ptr, C.POINTER(C.c_int64), C.c_int, c_ptr]),
    'sdmi_clip_finalize': (C.c_int, [c_ptr]),
    'sdmi_clip_workspace_bytes': (C.c_int64, [c_ptr, C.c_int, C.c_int]),
    'sdmi_clip_forward': (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, c_ptr, C.c_int64, c_ptr]),
    'sdmi_clip_create_projection': (C.c_int, [C.POINTER(ClipCfg), C.c_int, C.c_int, C.POINTER(c_ptr)]),
    'sdmi_clip_projection_dim': (C.c_int, [c_ptr]),
    'sdmi_clip_text_embeds_workspace_bytes': (C.c_int64, [c_ptr, C.c_int, C.c_int]),
    'sdmi_clip_text_embeds': (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr, C.c_int64, c_ptr]),
    'sdmi_bert_create': (C.c_int, [C.POINTER(BertCfg), C.POINTER(c_ptr)]),
    'sdmi_bert_create_precision': (C.c_int, [C.POINTER(BertCfg), C.c_int, C.POINTER(c_ptr)]),
    'sdmi_bert_precision': (C.c_int, [c_ptr]),
    'sdmi_bert_destroy': (C.c_int, [c_ptr]),
    'sdmi_bert_num_weights': (C.c_int, [c_ptr]),
    'sdmi_bert_weight_info': (C.c_int, [c_ptr, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    'sdmi_bert_set_weight': (C.c_int, [c_ptr, C.c_char_p, c_ptr, C.POINTER(C.c_int64), C.c_int, c_ptr]),
    'sdmi_bert_finalize': (C.c_int, [c_ptr]),
    'sdmi_bert_workspace_bytes': (C.c_int64, [c_ptr, C.c_int, C.c_int]),
    'sdmi_bert_forward': (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, c_ptr, C.c_int64, c_ptr]),
    'sdmi_vit_create': (C.c_int, [C.POINTER(VitCfg), C.POINTER(c_ptr)]),
    'sdmi_vit_destroy': (C.c_int, [c_ptr]),
    'sdmi_vit_num_weights': (C.c_int, [c_ptr]),
    'sdmi_vit_weight_info': (C.c_int, [c_ptr, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    'sdmi_vit_set_weight': (C.c_int, [c_ptr, C.c_char_p, c_ptr, C.POINTER(C.c_int64), C.c_int, c_ptr]),
    'sdmi_vit_finalize': (C.c_int, [c_ptr]),
    'sdmi_vit_workspace_bytes': (C.c_int64, [c_ptr, C.c_int]),
    'sdmi_vit_forward': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, c_ptr, C.c_int64, c_ptr]),
    'sdmi_k_vit_kpad': (C.c_int, [C.c_int]),
    'sdmi_k_vit_patchify': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_vit_embed': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_vit_preprocess': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_safety_head': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_fe_ksize': (C.c_int, [C.c_int, C.c_int]),
    'sdmi_fe_coeffs': (C.c_int, [C.c_int, C.c_int, c_ptr, c_ptr]),
    'sdmi_fe_output_size': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'sdmi_fe_workspace_bytes': (C.c_int64, [C.c_int] * 5),
    'sdmi_k_clip_feature_extract': (C.c_int, [c_ptr] + [C.c_int] * 7 + [c_ptr, c_ptr, C.c_int, c_ptr, c_ptr, C.c_int, C.POINTER(C.c_float),
                                              C.POINTER(C.c_float), c_ptr, C.c_int64, c_ptr, c_ptr, c_ptr]),
    'sdmi_knn_create': (C.c_int, [C.c_int, C.c_int64, C.POINTER(c_ptr)]),
    'sdmi_knn_destroy': (C.c_int, [c_ptr]),
    'sdmi_knn_set_rows': (C.c_int, [c_ptr, C.c_int64, C.c_int64, c_ptr, c_ptr]),
    'sdmi_knn_finalize': (C.c_int, [c_ptr, c_ptr]),
    'sdmi_knn_rows': (C.c_int64, [c_ptr]),
    'sdmi_knn_dim': (C.c_int, [c_ptr]),
    'sdmi_knn_workspace_bytes': (C.c_int64, [c_ptr, C.c_int, C.c_int]),
    'sdmi_knn_search': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_knn_condition': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_k_knn_inv_norm': (C.c_int, [c_ptr, C.c_int64, C.c_int, c_ptr, c_ptr]),
    'sdmi_k_knn_scan': (C.c_int, [c_ptr, c_ptr, C.c_int64, C.c_int, c_ptr, C.c_int, C.c_int, C.c_int64, c_ptr, c_ptr, c_ptr]),
    'sdmi_k_knn_merge': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr, c_ptr, c_ptr]),
    'sdmi_k_knn_stream_read': (C.c_int, [c_ptr, C.c_int64, c_ptr, c_ptr]),
    'sdmi_k_knn_gather': (C.c_int, [c_ptr, c_ptr, C.c_int64, C.c_int, c_ptr, C.c_int, C.c_int, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_has_experiments': (C.c_int, []),
    'sdmi_k_igemm': (C.c_int, [C.POINTER(IGemmDesc), c_ptr]),
    'sdmi_k_igemm_tail': (C.c_int, [C.POINTER(IGemmDesc), c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, c_ptr, C.c_int, c_ptr]),
    'sdmi_k_tail_split_range': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'sdmi_k_igemm_up_phase': (C.c_int, [C.POINTER(IGemmDesc), c_ptr]),
    'sdmi_k_up_phase_weights': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, c_ptr]),
    'sdmi_tune_lookup': (C.c_int, [C.c_int] * 9 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'sdmi_unet_skip_fold_plan': (C.c_int, [c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    'sdmi_k_ff_tail': (C.c_int, [C.POINTER(IGemmDesc), c_ptr, c_ptr, C.c_float, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    'sdmi_k_gn_conv3': (C.c_int, [C.POINTER(IGemmDesc), c_ptr, c_ptr, C.c_int, C.c_int, c_ptr, C.c_int64, c_ptr, c_ptr, C.c_float, c_ptr]),
    'sdmi_k_st_mid_ctx': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_float, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_float, c_ptr,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_st_tail': (C.c_int, [C.POINTER(IGemmDesc), c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_float, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    'sdmi_k_st_mid': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_float, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int, c_ptr]),
    'sdmi_k_st_head': (C.c_int, [c_ptr, c_ptr, C.c_int64, c_ptr, c_ptr, C.c_float, c_ptr, c_ptr, c_ptr, c_ptr, C.c_float, c_ptr, c_ptr, c_ptr,
                                 c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_attention_split16': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_float, c_ptr]),
    'sdmi_k_attention_split16_causal': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_float, c_ptr]),
    'sdmi_k_attention_causal': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                          c_ptr]),
    'sdmi_k_pointwise_nchw': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, c_ptr]),
    'sdmi_k_pointwise_nchw128': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, c_ptr]),
    'sdmi_k_softmax_rows': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_float, c_ptr]),
    'sdmi_k_gelu_erf': (C.c_int, [c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_k_quick_gelu': (C.c_int, [c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_k_quick_gelu_split': (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_k_gelu_erf_split': (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_k_attention': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_float, c_ptr]),
    'sdmi_attn_small_takes': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'sdmi_k_groupnorm': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr, c_ptr, C.c_float, C.c_int,
                                   c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_k_groupnorm_ws_floats': (C.c_int64, [C.c_int, C.c_int]),
    'sdmi_k_groupnorm_film': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr, c_ptr, C.c_float, C.c_int, c_ptr, C.c_int,
                                        c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_k_layernorm': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_float, c_ptr]),
    'sdmi_k_cast_f16': (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_int64, c_ptr]),
    'sdmi_k_split_heads': (C.c_int, [c_ptr, C.c_int, C.c_int, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     c_ptr]),
    'sdmi_k_geglu_split': (C.c_int, [c_ptr, C.c_int, C.c_int, c_ptr, c_ptr, c_ptr]),
    'sdmi_k_layernorm_split': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_float, c_ptr]),
    'sdmi_k_timestep_embedding': (C.c_int, [c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_small_linear': (C.c_int, [c_ptr, C.c_int, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, c_ptr]),
    'sdmi_k_conv_in': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_conv_out': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_pack_conv_weight': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_pack_conv_weight_src': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_conv_out32': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_conv_in64': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_conv_out128': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_pack_conv_out': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_pack_split3': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_pack_conv_split3': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_pack_geglu': (C.c_int, [c_ptr, c_ptr, c_ptr, c_ptr, C.c_int, C.c_int, c_ptr]),
    'sdmi_k_ln_fold_prep': (C.c_int, [c_ptr, C.c_int, C.c_int, C.c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    'sdmi_image_to_uint8': (C.c_int, [c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr]),
    'sdmi_range_check': (C.c_int, [C.c_int]),
    'sdmi_range_report': (C.c_int, [C.c_char_p, C.c_int]),
    'sdmi_tune_begin': (C.c_int, []),
    'sdmi_tune_round': (C.c_int, [C.c_int]),
    'sdmi_tune_end': (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    'sdmi_tune_dump': (C.c_int, [C.c_char_p, C.c_int]),
    'sdmi_profile_begin': (C.c_int, []),
    'sdmi_profile_end': (C.c_int, [C.c_char_p, C.c_int]),
    'sdmi_k_prefetch_lines': (C.c_int, [c_ptr, C.c_int64, c_ptr]),
    'sdmi_zero_page': (c_ptr, []),
}

_lib = None


class SdmiError(RuntimeError):
    pass


def load():
    """Load libsdmi.so (once).  Raises if it has not been built -- there is no CPU / PyTorch fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SdmiError(f'{LIB_PATH} not found: build it with `python stable-diffusion_amd/build.py` '
                            '(the MI355X path has no fallback implementation)')
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)      # AttributeError here = header / library mismatch
            fn.restype = res
            fn.argtypes = args
        if lib.sdmi_abi_version() != 17:
            raise SdmiError('libsdmi ABI version mismatch')
        _lib = lib
    return _lib


def exported_symbols():
    return sorted(_SIGS)


def check(rc):
    if rc != 0:
        raise SdmiError(load().sdmi_last_error().decode('utf-8', 'replace'))


def ptr(t):
    """tensor (or None) -> device pointer for ctypes"""
    return None if t is None else t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream
