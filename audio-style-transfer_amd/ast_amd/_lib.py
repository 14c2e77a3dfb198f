"""ctypes binding of libast_hip.so (include/ast_hip.h).

The product path has NO fallback: importing an op without the built library, or
calling one without a GPU, raises.  Build with `python __graft_entry__.py` (or
`make -C audio-style-transfer_amd/csrc`).
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AST_HIP_LIB") or os.path.join(_HERE, "libast_hip.so")   # AST_HIP_LIB: same-box A/B of two builds (tools/ab.sh)

F32, BF16 = 0, 1
MAX_TAPS = 9
IGEMM_ACCUMULATE, IGEMM_RELU, IGEMM_WS_ZEROED, IGEMM_STATS, IGEMM_BN_SUMS, IGEMM_BN_NO_RELU, IGEMM_PER_IMAGE = (1 << b for b in range(7))
IGEMM_SLOTS_SHIFT, IGEMM_DET = 8, 4096      # ast_igemm flags (include/ast_hip.h: AST_IGEMM_*)

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


class Gather(C.Structure):
    """ast_gather_t"""
    _fields_ = [(n, i32) for n in ("N", "Hs", "Ws", "Cs", "Hm", "Wm", "sh", "sw", "oh", "ow", "Hd", "Wd", "Cd",
                                   "dsh", "dsw", "doh", "dow", "ntaps", "wtaps")] + [("tap", i32 * MAX_TAPS)]


class WeightDesc(C.Structure):
    """ast_weight_desc_t"""
    _fields_ = [("w", vp), ("u", vp), ("v", vp), ("sigma", vp), ("scratch", vp), ("wf", vp), ("wb", vp)] + \
               [(n, i32) for n in ("Co", "Ci", "KK", "s_co", "s_ci", "Cop", "Cip", "power_iter")] + \
               [("dwp", vp), ("grad", vp), ("inner", vp), ("dwp_from_wb", i32), ("dwp_replicas", i32)]


class LinWg(C.Structure):
    """record of ast_linear_wgrad_batched"""
    _fields_ = [("dy", vp), ("x", vp), ("dW", vp), ("db", vp)] + [(n, i32) for n in ("M", "N", "K", "lddy", "ldw", "p0", "p1", "p2")]


_SIGS = {
    "ast_version": ([], i32),
    "ast_igemm": ([vp, vp, vp, vp, C.POINTER(Gather), i32, i32, vp, C.c_long, vp], i32),
    "ast_igemm_plan": ([C.POINTER(Gather), i32, C.POINTER(i32 * 5)], i32),
    "ast_pconv_variant": ([C.POINTER(Gather), i32, C.POINTER(i32 * 4)], i32),
    "ast_igemm_ws_floats": ([C.POINTER(Gather), i32], C.c_long),
    "ast_wgrad": ([vp, vp, vp, C.POINTER(Gather), i32, vp], i32),
    "ast_skinny_gemm": ([vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_skinny_gemm_ex": ([vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, f32, C.c_uint64, vp, vp], i32),
    "ast_bigk_gemm": ([vp, vp, vp, vp, i32, i32, i32, i32, vp], i32),
    "ast_bign_dgrad": ([vp, vp, vp, i32, i32, i32, i32, vp], i32),
    "ast_linear_wgrad": ([vp, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "ast_linear_wgrad_batched": ([vp, i32, i32, vp], i32),
    "ast_linear_wgrad_batched_host": ([vp, i32, i32, vp], i32),
    "ast_nchw_to_nhwc": ([vp, vp, i32, i32, i32, i32, i64, i64, i64, i32, i32, vp], i32),
    "ast_nhwc_to_nchw": ([vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_cast": ([vp, i32, vp, i32, i64, vp], i32),
    "ast_weights_prepare_t": ([vp, vp, i32, i32, i32, vp, i32, vp], i32),
    "ast_sn_scratch_floats": ([i32, i32], C.c_long),
    "ast_weight_grads_flush_t": ([vp, vp, i32, vp], i32),
    "ast_dropout_fwd": ([vp, vp, vp, i64, f32, C.c_uint64, vp, vp], i32),
    "ast_weight_grad_unpack": ([vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp], i32),
    "ast_chan_stats": ([vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "ast_norm_finalize": ([vp, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, f32, vp, vp, vp, vp, C.c_long, vp], i32),
    "ast_affine_act": ([vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "ast_bn_apply_fwd": ([vp, vp, vp, vp, i32, C.c_long, vp, vp, vp, vp, vp, vp, f32, vp, vp, f32, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_bn_apply_bwd": ([vp, vp, vp, vp, vp, vp, i32, C.c_long, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_norm_bwd_sums": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_norm_bwd_sums_pre": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp], i32),
    "ast_norm_bwd_apply_pre": ([vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp], i32),
    "ast_norm_bwd_finalize": ([vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    "ast_norm_bwd_finalize_n": ([vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_long, vp], i32),
    "ast_igemm_bn": ([vp, vp, vp, vp, C.POINTER(Gather), i32, i32, vp, C.c_long, vp, vp, vp, vp], i32),
    "ast_norm_bwd_apply": ([vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "ast_layernorm_fwd": ([vp, vp, vp, vp, vp, vp, i32, i32, f32, i32, vp], i32),
    "ast_layernorm_bwd": ([vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp], i32),
    "ast_add_drop_ln_fwd": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, C.c_uint64, vp, vp], i32),
    "ast_add_drop_ln_bwd": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp], i32),
    "ast_adaptive_pool_fwd": ([vp, vp, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_adaptive_pool_bwd": ([vp, vp, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_bilinear_fwd": ([vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_bilinear_bwd": ([vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_attn_fwd": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp], i32),
    "ast_attn_bwd": ([vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp], i32),
    "ast_rowmix": ([vp, vp, vp, i32, i32, i32, vp], i32),
    "ast_attn_fwd_p": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, f32, C.c_uint64, vp, vp], i32),
    "ast_attn_bwd_p": ([vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, f32, C.c_uint64, vp, vp], i32),
    "ast_add": ([vp, vp, vp, i64, i32, vp], i32),
    "ast_relu_bwd": ([vp, vp, vp, i64, i32, vp], i32),
    "ast_dropout_mask": ([vp, i64, f32, C.c_uint64, vp, vp], i32),
    "ast_mul": ([vp, vp, vp, i64, i32, vp], i32),
    "ast_recon_loss": ([vp, vp, i64, i32, i32, i32, i32, f32, f32, f32, f32, f32, vp, vp, vp], i32),
    "ast_recon_loss_total": ([vp, vp, i64, i32, i32, i32, i32, C.POINTER(f32), C.POINTER(f32), vp, vp, vp, vp], i32),
    "ast_infonce": ([vp, vp, i32, i32, f32, vp, vp, vp, vp], i32),
    "ast_margin": ([vp, i32, i32, f32, vp, vp, vp], i32),
    "ast_hsic": ([vp, vp, i32, i32, vp, vp, vp, vp, vp], i32),
    "ast_crosscov": ([vp, vp, i32, i32, vp, vp, vp, vp, vp], i32),
    "ast_istft": ([vp, i32, i32, vp, vp, vp], i32),
    "ast_bin_stats_acc": ([vp, vp, vp, i32, i32, i32, vp], i32),
    "ast_zscore": ([vp, vp, vp, vp, i32, i32, i32, f32, vp], i32),
    "ast_sections_overlap_avg": ([vp, vp, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_cross_entropy": ([vp, vp, i32, i32, vp, vp, vp], i32),
    "ast_softmax_entropy": ([vp, i32, i32, vp, vp, vp], i32),
    "ast_scale": ([vp, vp, f32, vp, i64, i32, vp], i32),
    "ast_colsum_acc": ([vp, i64, i32, i32, vp, i32, vp], i32),
    "ast_sumsq": ([vp, i64, vp, vp], i32),
    "ast_adam": ([vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, vp, vp, f32, vp], i32),
    "ast_adam_dev": ([vp, vp, vp, vp, i64, vp, f32, f32, f32, f32, vp, vp, vp], i32),
    "ast_set_values": ([vp, C.POINTER(f32), i32, vp], i32),
    "ast_weighted_sum": ([C.POINTER(vp), C.POINTER(i32), i32, vp, vp, vp], i32),
    "ast_weighted_sum_bwd": ([vp, C.POINTER(i32), i32, vp, vp, vp], i32),
    "ast_counter_incr": ([vp, vp], i32),
    "ast_stft_sections": ([vp, i32, i32, vp, vp, vp, i32, i32, i32, i32, vp], i32),
    "ast_cqt_octaves": ([vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, i32, i32, i32, vp], i32),
    "ast_cqt_sections": ([vp, i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "ast_resample_poly": ([vp, i32, i32, vp, i32, i32, i32, i32, vp, i32, f32, vp], i32),
    "ast_wgrad_rep": ([vp, vp, vp, C.POINTER(Gather), i32, i32, vp], i32),
    "ast_wgrad_slab": ([vp, vp, vp, C.POINTER(Gather), i32, i32, C.POINTER(i32), vp], i32),
    "ast_slab_sum": ([C.POINTER(vp), C.POINTER(i64), C.POINTER(i32), i32, vp], i32),
    "ast_wgrad_plan": ([C.POINTER(Gather), i32, i32, C.POINTER(i32 * 6)], i32),
    # deterministic forms (include/ast_hip.h)
    "ast_ordered_sum": ([vp, i64, i32, i32, vp, i32, vp], i32),
    "ast_igemm_ws_floats_det": ([C.POINTER(Gather), i32], C.c_long),
    "ast_sumsq_det": ([vp, i64, vp, vp, i32, vp], i32),
    "ast_colsum_acc_det": ([vp, i64, i32, i32, vp, i32, vp, i32, vp], i32),
    "ast_chan_stats_det": ([vp, vp, i32, i32, i32, i32, vp, i32, vp], i32),
    "ast_norm_bwd_sums_det": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp], i32),
    "ast_layernorm_bwd_det": ([vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp], i32),
    "ast_add_drop_ln_bwd_det": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp], i32),
    "ast_recon_loss_total_det": ([vp, vp, i64, i32, i32, i32, i32, C.POINTER(f32), C.POINTER(f32), vp, C.c_long, vp, vp, vp], i32),
    "ast_weight_grads_flush_det": ([vp, vp, i32, vp, C.c_long, vp], i32),
    "ast_bigk_gemm_det_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_bigk_gemm_det": ([vp, vp, vp, vp, i32, i32, i32, vp, C.c_long, vp], i32),
    "ast_bign_dgrad_det_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_bign_dgrad_det": ([vp, vp, vp, i32, i32, i32, i32, vp, C.c_long, vp], i32),
    # wide token path: 65 .. AST_WIDE_MAX_ROWS rows (include/ast_hip.h)
    "ast_skinny_gemm_wide": ([vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
    "ast_skinny_gemm_wide_ex": ([vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, f32, C.c_uint64, vp, vp], i32),
    "ast_linear_wgrad_wide": ([vp, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "ast_bigk_gemm_wide": ([vp, vp, vp, vp, i32, i32, i32, i32, vp], i32),
    "ast_bigk_gemm_wide_det_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_bigk_gemm_wide_det": ([vp, vp, vp, vp, i32, i32, i32, vp, C.c_long, vp], i32),
    "ast_bign_dgrad_wide": ([vp, vp, vp, i32, i32, i32, i32, vp], i32),
    "ast_bign_dgrad_wide_det_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_bign_dgrad_wide_det": ([vp, vp, vp, i32, i32, i32, i32, vp, C.c_long, vp], i32),
    "ast_tok_max_ops": ([], i32),
    "ast_tok_program": ([vp, i32, i32, i32, vp, vp, vp, vp], i32),
    # ragged inference batches: per-clip lengths read from the device (include/ast_hip.h)
    "ast_attn_fwd_len": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp], i32),
    # the same core in training: mask and dropout, forward and backward
    "ast_attn_fwd_len_p": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, f32, C.c_uint64, vp, vp], i32),
    "ast_attn_bwd_len_p": ([vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, f32, C.c_uint64, vp,
                            vp], i32),
    "ast_sections_overlap_avg_len": ([vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp], i32),
    "ast_istft_len": ([vp, i32, i32, vp, vp, vp, vp], i32),
    # ragged waveforms: per-clip sample counts read from the device (include/ast_hip.h)
    "ast_frontend_lengths": ([vp, i32, i32, i32, i32, vp, vp, vp], i32),
    "ast_frontend_lengths_host": ([i32, i32, i32, i32, C.POINTER(i32 * 4)], i32),
    "ast_stft_sections_len": ([vp, i32, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp], i32),
    "ast_decimate2_len": ([vp, i32, i32, vp, i32, i32, vp, i32, f32, vp, i32, i32, i32, i32, vp], i32),
    "ast_cqt_octaves_len": ([vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, i32, i32, i32, vp, i32, i32, i32, vp], i32),
    "ast_cqt_sections_len": ([vp, i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp], i32),
    # embedding_to_stft at inference: up to AST_BIGN_MAX_ROWS rows, per-clip section counts read from the device (include/ast_hip.h)
    "ast_bign_gemm_len": ([vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp], i32),
    # native-rate, stereo clips: load_audio's resample + channel mean per clip length read from the device (include/ast_hip.h)
    "ast_resample_poly_len": ([vp, i32, i32, i32, vp, i32, i32, i32, i32, vp, i32, f32, vp, vp, vp], i32),
    # spectrogram metrics of the evaluation scripts for a padded batch (include/ast_hip.h, ast_amd/metrics.py)
    "ast_spec_mse_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_spec_mse_len": ([vp, i32, vp, i32, i32, vp, vp, i32, vp, C.c_long, vp, vp], i32),
    "ast_band_energy_ws_floats": ([i32, i32], C.c_long),
    "ast_band_energy_len": ([vp, i32, i32, vp, i32, vp, C.c_long, vp, vp], i32),
    "ast_band_energy_run_frames": ([], i32),
    "ast_pearson_rows": ([vp, vp, i32, i32, vp, vp], i32),
    # MFCC and mfcc_distance for a padded batch (include/ast_hip.h, ast_amd/metrics.py)
    "ast_mel_table_words": ([], i32),
    "ast_mel_table": ([i32, vp], i32),
    "ast_mfcc_run_frames": ([], i32),
    "ast_mfcc_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_mfcc_len": ([vp, i32, i32, vp, i32, i32, i32, vp, vp, C.c_long, vp, vp], i32),
    "ast_mfcc_distance_ws_floats": ([i32, i32, i32, i32], C.c_long),
    "ast_mfcc_distance_len": ([vp, i32, vp, i32, i32, vp, vp, i32, i32, i32, vp, vp, C.c_long, vp, vp], i32),
    # onsets and self-similarity for a padded batch (include/ast_hip.h, ast_amd/metrics.py)
    "ast_onset_tile_frames": ([], i32),
    "ast_recurrence_chunk_frames": ([], i32),
    "ast_onset_strength_ws_floats": ([i32, i32], C.c_long),
    "ast_onset_strength_len": ([vp, i32, i32, vp, i32, vp, vp, C.c_long, vp, vp], i32),
    "ast_onset_detect_ws_floats": ([i32, i32], C.c_long),
    "ast_onset_detect_len": ([vp, i32, i32, vp, i32, vp, vp, C.c_long, vp, vp], i32),
    "ast_onset_accuracy_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_onset_accuracy_len": ([vp, i32, vp, i32, i32, vp, vp, i32, vp, vp, C.c_long, vp, vp], i32),
    "ast_recurrence_ws_floats": ([i32, i32], C.c_long),
    "ast_recurrence_len": ([vp, i32, i32, vp, i32, vp, vp, C.c_long, vp, vp, vp], i32),
    "ast_self_similarity_distance_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_self_similarity_distance_len": ([vp, i32, vp, i32, i32, vp, vp, i32, vp, vp, C.c_long, vp, vp], i32),
    # dataset screening for a padded batch (include/ast_hip.h, ast_amd/curation.py)
    "ast_frame_rms_tile_frames": ([], i32),
    "ast_mfcc_mean_chunk_frames": ([], i32),
    "ast_frame_rms_ws_floats": ([i32, i32], C.c_long),
    "ast_frame_rms_len": ([vp, i32, i32, vp, f32, i32, vp, C.c_long, vp, vp, vp, vp, vp, vp, vp], i32),
    "ast_window_sound_len": ([vp, i32, i32, vp, i32, f32, vp, vp, vp], i32),
    "ast_mfcc_mean_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_mfcc_mean_len": ([vp, i32, i32, vp, i32, i32, i32, vp, vp, C.c_long, vp, vp], i32),
    "ast_gain_rows_len": ([vp, i32, i32, vp, vp, C.c_double, vp, vp], i32),
    # chroma and pitch metrics for a padded batch (include/ast_hip.h, ast_amd/metrics.py)
    "ast_chroma_run_frames": ([], i32),
    "ast_pitch_band": ([i32, C.POINTER(i32), C.POINTER(i32)], i32),
    "ast_tuning_debug_words": ([], i32),
    "ast_tuning_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_tuning_len": ([vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, C.c_long, vp, vp, vp], i32),
    "ast_chroma_len": ([vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp], i32),
    "ast_chroma_distance_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_chroma_distance_len": ([vp, i32, vp, i32, i32, vp, vp, i32, vp, C.c_long, vp, vp], i32),
    "ast_chroma_similarity_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_chroma_similarity_len": ([vp, i32, vp, i32, i32, vp, vp, i32, vp, C.c_long, vp, vp], i32),
    "ast_pitch_mean_len": ([vp, i32, i32, vp, vp, i32, i32, vp, vp], i32),
    "ast_pitch_correlation_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_pitch_correlation_len": ([vp, i32, vp, i32, i32, vp, vp, i32, vp, C.c_long, vp, vp], i32),
    # per-clip reconstruction loss of a padded batch, section counts read from the device (include/ast_hip.h, ast_amd/losses.py)
    "ast_recon_loss_len_ws_floats": ([i32, i32, i32, i32], C.c_long),
    "ast_recon_loss_len": ([vp, vp, i64, i32, i32, i32, i32, vp, C.POINTER(f32), vp, C.c_long, vp, vp], i32),
    # training on a padded batch: the same loss with its gradient, and the backward of the length-masked output linear
    "ast_recon_loss_len_grad_ws_floats": ([i32, i32, i32, i32], C.c_long),
    "ast_recon_loss_len_grad": ([vp, vp, i64, i32, i32, i32, i32, vp, vp, C.POINTER(f32), vp, C.c_long, vp, vp, vp, vp], i32),
    "ast_bign_dgrad_len": ([vp, vp, vp, i32, i32, i32, i32, i32, vp, vp], i32),
    "ast_bign_dgrad_len_det_ws_floats": ([i32, i32, i32], C.c_long),
    "ast_bign_dgrad_len_det": ([vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, C.c_long, vp], i32),
    "ast_linear_wgrad_len": ([vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp], i32),
    # BatchNorm(+ReLU) and the decoder's two layout ops over the live images of a padded batch (include/ast_hip.h)
    "ast_chan_stats_len": ([vp, vp, i32, i32, i32, i32, i32, vp, vp], i32),
    "ast_norm_finalize_len": ([vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp], i32),
    "ast_affine_act_len": ([vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp], i32),
    "ast_norm_bwd_sums_len": ([vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp], i32),
    "ast_norm_bwd_finalize_len": ([vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    "ast_norm_bwd_apply_len": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp], i32),
    "ast_nchw_to_nhwc_len": ([vp, vp, i32, i32, i32, i32, i32, i64, i64, i64, i32, i32, vp, vp], i32),
    "ast_bilinear_fwd_len": ([vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp], i32),
    "ast_bilinear_bwd_len": ([vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp], i32),
    # 64-bit digest over the bytes of a list of device tensors (include/ast_hip.h, ast_amd/checkpoint.py)
    "ast_state_digest": ([C.POINTER(vp), C.POINTER(C.c_longlong), i32, vp, vp], i32),
}

EXPORTS = tuple(_SIGS) + ("ast_last_error",)

_lib = None


# ---- optional per-call profiling (bench.py's roofline.kernels[]): when PROFILE_CALLS is a list, every C-ABI call of the
# functions named in CALL_BYTES is bracketed by device events on the current stream and recorded as
# (name, algorithmic bytes, start event, end event).  Off (None) in normal operation: lib() returns the raw CDLL.
PROFILE_CALLS = None
NEXT_BYTES = None          # set by a caller whose byte count is not derivable from the arguments (weight pack / flush)


def _es(dtype_code):
    return 2 if dtype_code == BF16 else 4


CALL_BYTES = {
    # BatchNorm/InstanceNorm apply (+ReLU, + ResBlock add): read x (+ shortcut), write y
    "ast_affine_act": lambda a: a[7] * a[8] * a[9] * _es(a[11]) * (2 + (1 if a[3] else 0)),
    # norm backward apply: read dy, x (+ shortcut input), write dx (+ shortcut gradient)
    "ast_norm_bwd_apply_pre": lambda a: a[8] * a[9] * a[10] * _es(a[12]) * (3 + (2 if a[3] else 0)),
    "ast_norm_bwd_sums_pre": lambda a: a[5] * a[6] * a[7] * _es(a[9]) * (2 + (1 if a[3] else 0)),
    # the same two passes with the statistics finalize folded in (ast_bn_apply_fwd / _bwd)
    "ast_bn_apply_fwd": lambda a: a[18] * a[19] * a[20] * _es(a[23]) * (2 + (1 if a[1] else 0)),
    "ast_bn_apply_bwd": lambda a: a[22] * a[23] * a[24] * _es(a[27]) * (3 + (2 if a[2] else 0)),
    "ast_chan_stats": lambda a: a[2] * a[3] * a[4] * _es(a[5]),
    # compute_comprehensive_loss: read output and target, write the gradient (f32)
    "ast_recon_loss": lambda a: 3 * 4 * a[3] * a[4] * 2 * a[5] * a[6],
    "ast_recon_loss_total": lambda a: 3 * 4 * a[3] * a[4] * 2 * a[5] * a[6],
    # the per-clip values-only form: read output and target once (an upper bound for a ragged batch: padded sections are skipped)
    "ast_recon_loss_len": lambda a: 2 * 4 * a[3] * a[4] * 2 * a[5] * a[6],
    # the per-clip form with the gradient: read output and target, write the gradient (an upper bound for a ragged batch)
    "ast_recon_loss_len_grad": lambda a: 3 * 4 * a[3] * a[4] * 2 * a[5] * a[6],
    # backward of the length-masked output linear: the weight stream (N x K) plus dy; dW read and written plus dy and x
    "ast_bign_dgrad_len": lambda a: 4 * (a[4] * a[5] + a[3] * a[4] + a[3] * a[5]),
    "ast_bign_dgrad_len_det": lambda a: 4 * (a[4] * a[5] + a[3] * a[4] + a[3] * a[5]),
    "ast_linear_wgrad_len": lambda a: 4 * (2 * a[5] * a[6] + a[4] * (a[5] + a[6])),
    "ast_adam": lambda a: 7 * 4 * a[4],                    # read p, g, m, v; write p, m, v
    "ast_sumsq": lambda a: 4 * a[1],
    "ast_weights_prepare_t": None,                         # bytes from NEXT_BYTES (WeightBank)
    "ast_weight_grads_flush_t": None,
    "ast_nchw_to_nhwc": lambda a: a[2] * a[4] * a[5] * (a[3] * 4 + a[9] * _es(a[10])),
    "ast_bilinear_fwd": lambda a: a[0] and a[2] * (a[5] * a[6] * a[4] * _es(a[9]) + a[3] * a[7] * a[8] * 4),
}


class _ProfiledLib:
    def __init__(self, raw):
        self._raw = raw

    def __getattr__(self, name):
        fn = getattr(self._raw, name)
        if name not in CALL_BYTES:
            return fn

        def wrapped(*args):
            global NEXT_BYTES
            f = CALL_BYTES[name]
            nbytes = NEXT_BYTES if f is None else f(args)
            NEXT_BYTES = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            PROFILE_CALLS.append((name, float(nbytes or 0), e0, e1))
            return rc
        return wrapped


def lib():
    """The loaded library; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None and PROFILE_CALLS is not None:
        return _ProfiledLib(_lib)
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP library has not been built (run `python __graft_entry__.py` "
                "or `make -C audio-style-transfer_amd/csrc`). There is no CPU/PyTorch fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes, fn.restype = args, res
        L.ast_last_error.argtypes, L.ast_last_error.restype = [], C.c_char_p
        _lib = L
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        raise RuntimeError(f"libast_hip {what} failed ({rc}): {lib().ast_last_error().decode()}")


def dcode(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported activation dtype {dtype}")


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Refuses host tensors: the
    kernels would fault on them."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libast_hip needs device tensors (got a CPU tensor); there is no CPU path")
    return t.data_ptr()


def len_tensor(t, B, what, device=False, contiguous=False, training=False):
    """The one check of a per-clip count argument (lengths, key_len, n_sections, n_frames, n_samples): None passes through; anything
    but an int32 tensor of shape (B,) is a ValueError naming `what`.  The kernels read it as int32, so nothing else may reach them.
    device: it must be on the GPU as well (the entry points that never reach ptr() with it).  contiguous: return it contiguous.
    training: the caller's module is in training mode, where per-clip lengths do not exist; refused before the tensor is looked at."""
    if t is None:
        return None
    if training:
        raise ValueError("per-clip lengths are an inference feature: call .eval() first (training takes equal-length batches)")
    if not (torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == (B,) and (t.is_cuda or not device)):
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what} must be an int32 {'device ' if device else ''}tensor of shape ({B},), got {got}")
    return t.contiguous() if contiguous else t
