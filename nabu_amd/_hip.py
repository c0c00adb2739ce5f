"""ctypes binding of libnabu_hip.so (the C ABI declared in include/nabu_hip.h).

The product path has NO fallback: if the HIP library is missing or a tensor is
not on the GPU, the call raises.  PyTorch is used only to own device memory and
to name the HIP stream the kernels are enqueued on."""
import ctypes
import math
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NABU_HIP_LIB') or os.path.join(_HERE, 'libnabu_hip.so')   # (the override: A/B builds in experiments)

_c = ctypes
_vp, _i, _f, _sz, _ll = _c.c_void_p, _c.c_int, _c.c_float, _c.c_size_t, _c.c_longlong


class BlstmDesc(_c.Structure):
    _fields_ = [('size', _c.c_uint32), ('B', _c.c_int32), ('T', _c.c_int32), ('D', _c.c_int32),
                ('H', _c.c_int32), ('max_len', _c.c_int32), ('mode', _c.c_int32),
                ('gemm_precision', _c.c_int32), ('x_bound', _c.c_float), ('flags', _c.c_int32),
                ('recurrent_precision', _c.c_int32),
                # ABI version 3: packed companions (include/nabu_hip.h)
                ('out_stack', _c.c_int32), ('out_pk_rows', _c.c_void_p), ('out_pk_cols', _c.c_void_p),
                ('hT_pk', _c.c_void_p), ('x_pk_rows', _c.c_void_p), ('x_pk_cols', _c.c_void_p)]


class BlstmLnParams(_c.Structure):
    """nabu_blstm_ln_params: [fw, bw][input, transform, forget, output, state] pointers to [H] arrays"""
    _fields_ = [('size', _c.c_uint32), ('reserved', _c.c_uint32), ('gamma', (_c.c_void_p * 5) * 2),
                ('beta', (_c.c_void_p * 5) * 2), ('dgamma', (_c.c_void_p * 5) * 2), ('dbeta', (_c.c_void_p * 5) * 2)]


BLSTM_FWD_ONLY = 1
REC_PRECISIONS = {'default': 0, 'f32': 1}


class PkGemmDesc(_c.Structure):
    _fields_ = [('size', _c.c_uint32), ('planes', _c.c_int32), ('M', _c.c_int32), ('N', _c.c_int32),
                ('nkb', _c.c_int32), ('nbatch', _c.c_int32), ('A', _c.c_void_p * 2), ('B', _c.c_void_p * 2),
                ('a_rows_pad', _c.c_int32), ('b_rows_pad', _c.c_int32), ('a_planes', _c.c_int32),
                ('b_planes', _c.c_int32), ('C', _c.c_void_p * 2), ('C2', _c.c_void_p * 2),
                ('ldc', _c.c_int32), ('n_split', _c.c_int32), ('bias', _c.c_void_p), ('bias2', _c.c_void_p),
                ('alpha', _c.c_float), ('beta', _c.c_float), ('a_amax', _c.c_void_p * 2), ('b_amax', _c.c_void_p * 2), ('direct', _c.c_int32)]


class FeatDesc(_c.Structure):
    """nabu_feat_desc: build one with feat_desc(), which applies the reference's rounding to the frame sizes"""
    _fields_ = [('size', _c.c_uint32)] + [(n, _c.c_int32) for n in
                                          ('rate', 'frame_len', 'frame_step', 'nfft', 'nfilt', 'numcep', 'kind',
                                           'include_energy', 'dynamic', 'mvn', 'lowfreq', 'highfreq')] + \
               [('preemph', _c.c_float), ('ceplifter', _c.c_float), ('winlen', _c.c_double), ('winstep', _c.c_double)]


class BatchSeg(_c.Structure):
    """nabu_batch_seg: one tensor of a packed batch (nabu_batch_unpack)"""
    _fields_ = [('rows', _c.c_int32), ('width', _c.c_int32), ('max_len', _c.c_int32), ('reserved', _c.c_int32),
                ('len_off', _c.c_uint64), ('row_off', _c.c_uint64), ('data_off', _c.c_uint64),
                ('out', _c.c_void_p), ('out_len', _c.c_void_p)]


BATCH_MAX_SEGS = 8


class SpecAugDesc(_c.Structure):
    """nabu_specaug_desc (nabu_spec_augment_f32)"""
    _fields_ = [('size', _c.c_uint32)] + [(n, _c.c_int32) for n in
                                          ('B', 'T', 'D', 'feature_blocks', 'time_warp', 'time_masks', 'time_mask_width',
                                           'freq_masks', 'freq_mask_width')] + [('time_mask_ratio', _c.c_float)]


SPECAUG_MAX_MASKS = 8

FEAT_KINDS = {'fbank': 0, 'mfcc': 1}
FEAT_DYNAMIC = {'nodelta': 0, 'delta': 1, 'ddelta': 2}


def round_half_away(x):
    """Python 2's round() for x >= 0 (Python 3 rounds halves to even): 220.5 -> 221, 1102.5 -> 1103"""
    return int(math.floor(x + 0.5))


def feat_desc(rate, kind='fbank', winlen=0.025, winstep=0.01, nfft=512, nfilt=40, numcep=12, include_energy=True,
              dynamic='ddelta', mvn=True, lowfreq=0, highfreq=-1, preemph=0.97, ceplifter=22.0):
    return FeatDesc(_c.sizeof(FeatDesc), int(rate), round_half_away(float(winlen) * rate),
                    round_half_away(float(winstep) * rate), int(nfft), int(nfilt), int(numcep), FEAT_KINDS[kind],
                    int(bool(include_energy)), FEAT_DYNAMIC[dynamic], int(bool(mvn)), int(lowfreq), int(highfreq),
                    float(preemph), float(ceplifter), float(winlen), float(winstep))


# name -> (restype, argtypes); must list every symbol of include/nabu_hip.h
SIGNATURES = {
    'nabu_version': (_i, []),
    'nabu_last_error': (_c.c_char_p, []),
    'nabu_gemm_ws_bytes': (_sz, [_i, _i, _i]),
    'nabu_gemm_f32': (_i, [_i, _i, _i, _i, _i, _f, _vp, _i, _vp, _i, _f, _vp, _i, _vp, _i, _ll, _ll,
                           _vp, _sz, _vp]),
    'nabu_gemm_ex': (_i, [_i, _i, _i, _i, _i, _i, _f, _vp, _i, _vp, _i, _f, _vp, _i, _vp, _i, _ll, _ll,
                          _vp, _sz, _vp]),
    'nabu_gemm2_ws_bytes': (_sz, [_i, _i, _i, _i]),
    'nabu_gemm2_f32': (_i, [_i, _i, _i, _vp, _i, _vp, _i, _i, _vp, _i, _vp, _i, _f, _vp, _i, _vp, _vp, _sz, _vp]),
    'nabu_pk_rows_pad': (_i, [_i]),
    'nabu_pk_kblocks': (_i, [_i, _i]),
    'nabu_pk_bytes': (_sz, [_i, _i, _i]),
    'nabu_pk_pack': (_i, [_i, _i, _vp, _ll, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'nabu_pk_amax': (_i, [_vp, _ll, _i, _i, _vp, _vp, _vp]),
    'nabu_pk_amax_fill': (_i, [_vp, _i, _f, _vp]),
    'nabu_pk_pack_f16': (_i, [_i, _vp, _ll, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'nabu_gemm_pk_ws_bytes': (_sz, [_c.POINTER(PkGemmDesc)]),
    'nabu_gemm_pk': (_i, [_c.POINTER(PkGemmDesc), _vp, _sz, _vp]),
    'nabu_gemm_set_default_precision': (_i, [_i]),
    'nabu_gemm_get_default_precision': (_i, []),
    'nabu_colsum_ws_bytes': (_sz, [_i, _i]),
    'nabu_colsum_f32': (_i, [_i, _i, _vp, _i, _f, _vp, _vp, _sz, _vp]),
    'nabu_linear_bwd_ws_bytes': (_sz, [_i, _i, _i]),
    'nabu_linear_bwd_f32': (_i, [_i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    'nabu_blstm_reserve_bytes': (_sz, [_c.POINTER(BlstmDesc)]),
    'nabu_blstm_ws_bytes': (_sz, [_c.POINTER(BlstmDesc)]),
    'nabu_blstm_fwd': (_i, [_c.POINTER(BlstmDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_blstm_bwd': (_i, [_c.POINTER(BlstmDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                            _vp, _vp, _vp, _sz, _vp]),
    'nabu_blstm_bwd_data': (_i, [_c.POINTER(BlstmDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_blstm_bwd_weights': (_i, [_c.POINTER(BlstmDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_blstm_ln_reserve_bytes': (_sz, [_c.POINTER(BlstmDesc)]),
    'nabu_blstm_ln_ws_bytes': (_sz, [_c.POINTER(BlstmDesc)]),
    'nabu_blstm_ln_fwd': (_i, [_c.POINTER(BlstmDesc), _vp, _vp, _vp, _vp, _c.POINTER(BlstmLnParams), _vp, _vp, _vp, _sz, _vp]),
    'nabu_blstm_ln_bwd': (_i, [_c.POINTER(BlstmDesc), _vp, _vp, _vp, _vp, _c.POINTER(BlstmLnParams), _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp, _sz, _vp]),
    'nabu_blstm_ln_bwd_data': (_i, [_c.POINTER(BlstmDesc), _vp, _vp, _vp, _vp, _c.POINTER(BlstmLnParams), _vp, _vp, _vp, _vp,
                                    _vp, _sz, _vp]),
    'nabu_blstm_ln_bwd_weights': (_i, [_c.POINTER(BlstmDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_blstm_uses_persistent': (_i, [_c.POINTER(BlstmDesc)]),
    'nabu_blstm_pk_bytes': (_i, [_c.POINTER(BlstmDesc), _c.POINTER(_c.c_size_t)]),
    'nabu_blstm_emits_packed': (_i, [_c.POINTER(BlstmDesc)]),
    'nabu_blstm_set_profile_events': (_i, [_vp, _vp]),
    'nabu_persist_set_timeout_us': (_i, [_ll]),
    'nabu_blstm_set_phase_hook': (_i, [_vp, _vp]),
    'nabu_pad_time_f32': (_i, [_i, _i, _i, _i, _vp, _vp, _vp]),
    'nabu_unpad_time_f32': (_i, [_i, _i, _i, _i, _vp, _vp, _vp]),
    'nabu_ctc_ws_bytes': (_sz, [_i, _i, _i]),
    'nabu_ctc_loss_grad': (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_ctc_align_ws_bytes': (_sz, [_i, _i, _i]),
    'nabu_ctc_align': (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_transducer_ws_bytes': (_sz, [_i, _i, _i]),
    'nabu_transducer_loss_grad': (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_transducer_align_ws_bytes': (_sz, [_i, _i, _i]),
    'nabu_transducer_align_lds_bytes': (_sz, [_i, _i, _i]),
    'nabu_transducer_align': (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_transducer_greedy_step': (_i, [_i, _i, _i, _i, _i] + [_vp] * 9 + [_vp]),
    'nabu_transducer_beam_ws_bytes': (_sz, [_i, _i, _i, _i]),
    'nabu_transducer_beam_step': (_i, [_i] * 6 + [_vp] * 12 + [_vp, _sz, _vp]),
    'nabu_xent_loss_grad': (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp]),
    'nabu_xent_smooth_loss_grad': (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp]),
    'nabu_lstm_cell_fwd': (_i, [_i, _i, _i] + [_vp] * 10 + [_vp]),
    'nabu_lstm_cell_bwd': (_i, [_i, _i, _i] + [_vp] * 9 + [_vp]),
    'nabu_attn_fwd': (_i, [_vp, _i] + [_vp] * 14 + [_sz, _vp]),
    'nabu_attn_fwd_ws_bytes': (_sz, [_vp]),
    'nabu_attn_bwd': (_i, [_vp, _i] + [_vp] * 21 + [_sz, _vp]),
    'nabu_attn_bwd_slices': (_i, [_vp]),
    'nabu_attn_bwd_ws_bytes': (_sz, [_vp]),
    'nabu_sample_ids': (_i, [_i, _i, _vp, _f, _c.c_ulonglong, _c.c_ulonglong, _vp, _vp, _vp]),
    'nabu_speller_decoder_inputs': (_i, [_vp, _vp, _vp, _vp]),
    'nabu_speller_reserve_bytes': (_sz, [_vp]),
    'nabu_speller_ws_bytes': (_sz, [_vp]),
    'nabu_speller_uses_persistent': (_i, [_vp, _i]),
    'nabu_speller_fwd': (_i, [_vp] * 9 + [_sz, _vp]),
    'nabu_speller_bwd': (_i, [_vp] * 11 + [_sz, _vp]),
    'nabu_speller_multi_reserve_bytes': (_sz, [_vp]),
    'nabu_speller_multi_ws_bytes': (_sz, [_vp]),
    'nabu_speller_multi_uses_persistent': (_i, [_vp, _i]),
    'nabu_speller_multi_attn_slices': (_i, [_vp, _i]),
    'nabu_speller_multi_decoder_inputs': (_i, [_vp, _vp, _vp, _vp]),
    'nabu_speller_multi_beam_ws_bytes': (_sz, [_vp]),
    'nabu_speller_multi_beam_search': (_i, [_vp] * 10 + [_sz, _vp]),
    'nabu_speller_multi_fwd': (_i, [_vp] * 9 + [_sz, _vp]),
    'nabu_speller_multi_bwd': (_i, [_vp] * 11 + [_sz, _vp]),
    'nabu_mask_time_f32': (_i, [_i, _i, _i, _vp, _vp, _vp]),
    'nabu_swap01_f32': (_i, [_i, _i, _i, _vp, _vp, _vp]),
    'nabu_scatter_rows_f32': (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    'nabu_adam_clip_step': (_i, [_sz, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _vp]),
    'nabu_adam_clip_step_from': (_i, [_sz, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _vp]),
    'nabu_clip_f32': (_i, [_sz, _vp, _f, _vp]),
    'nabu_clip_accumulate_f32': (_i, [_sz, _vp, _vp, _vp, _f, _vp]),
    'nabu_adam_clip_step_acc': (_i, [_sz, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _f, _vp]),
    'nabu_grad_norm_ws_bytes': (_sz, [_sz]),
    'nabu_grad_norm_f32': (_i, [_sz, _vp, _vp, _f, _f, _vp, _vp, _sz, _vp]),
    'nabu_adam_scaled_step': (_i, [_sz, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _vp, _vp]),
    'nabu_dropout_f32': (_i, [_sz, _vp, _vp, _f, _c.c_ulonglong, _c.c_ulonglong, _vp]),
    'nabu_gaussian_noise_f32': (_i, [_sz, _vp, _vp, _f, _c.c_ulonglong, _c.c_ulonglong, _vp]),
    'nabu_weight_noise_f32': (_i, [_sz, _vp, _vp, _vp, _vp, _i, _f, _c.c_ulonglong, _c.c_ulonglong, _vp]),
    'nabu_spec_augment_f32': (_i, [_c.POINTER(SpecAugDesc), _vp, _vp, _vp, _vp, _c.c_ulonglong, _c.c_ulonglong, _vp]),
    'nabu_sum_f32': (_i, [_sz, _vp, _f, _vp, _vp]),
    'nabu_axpy_f32': (_i, [_sz, _f, _vp, _vp, _vp]),
    'nabu_ceil_div_i32': (_i, [_i, _vp, _i, _vp, _vp]),
    'nabu_batch_unpack': (_i, [_i, _vp, _vp, _sz, _vp]),
    'nabu_ctc_beam_ws_bytes': (_sz, [_i, _i, _i, _i]),
    'nabu_ctc_beam_search': (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_edit_distance': (_i, [_i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    'nabu_mwer_prepare': (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    'nabu_rows_tile_f32': (_i, [_i, _i, _i, _vp, _vp, _vp]),
    'nabu_rows_tile_bwd_f32': (_i, [_i, _i, _i, _vp, _vp, _vp]),
    'nabu_mwer_loss_grad': (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    'nabu_speller_beam_ws_bytes': (_sz, [_vp]),
    'nabu_speller_beam_search': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_beam_prune': (_i, [_i, _i, _i, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'nabu_beam_gather': (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'nabu_ctc_prefix_prepare': (_i, [_i, _i, _i, _i] + [_vp] * 6 + [_vp]),
    'nabu_ctc_prefix_score': (_i, [_i, _i, _i, _i] + [_vp] * 8 + [_vp]),
    'nabu_ctc_prefix_advance': (_i, [_i, _i, _i, _i] + [_vp] * 12 + [_vp]),
    'nabu_beam_prune_joint': (_i, [_i, _i, _i, _vp, _vp, _f, _f, _f] + [_vp] * 9 + [_vp]),
    'nabu_speller_beam_joint_ws_bytes': (_sz, [_vp]),
    'nabu_speller_beam_search_joint': (_i, [_vp] * 5 + [_f] + [_vp] * 6 + [_sz, _vp]),
    'nabu_speller_multi_beam_joint_ws_bytes': (_sz, [_vp]),
    'nabu_speller_multi_beam_search_joint': (_i, [_vp] * 5 + [_f] + [_vp] * 6 + [_sz, _vp]),
    'nabu_ctc_beam_lm_ws_bytes': (_sz, [_i, _i, _i, _i]),
    'nabu_ctc_beam_search_lm': (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    'nabu_beam_prune_lm': (_i, [_i, _i, _i, _vp, _vp, _f, _vp, _i, _f, _vp, _vp, _f, _f] + [_vp] * 9 + [_vp]),
    'nabu_speller_beam_ex_ws_bytes': (_sz, [_vp, _vp]),
    'nabu_speller_beam_search_ex': (_i, [_vp] * 11 + [_sz, _vp]),
    'nabu_speller_multi_beam_ex_ws_bytes': (_sz, [_vp, _vp]),
    'nabu_speller_multi_beam_search_ex': (_i, [_vp] * 11 + [_sz, _vp]),
    'nabu_sample_advance': (_i, [_i, _i, _vp, _c.c_ulonglong, _c.c_ulonglong, _i, _i] + [_vp] * 6 + [_vp]),
    'nabu_speller_sample_ws_bytes': (_sz, [_vp]),
    'nabu_speller_sample': (_i, [_vp] * 4 + [_c.c_ulonglong, _c.c_ulonglong] + [_vp] * 6 + [_sz, _vp]),
    'nabu_speller_multi_sample_ws_bytes': (_sz, [_vp]),
    'nabu_speller_multi_sample': (_i, [_vp] * 4 + [_c.c_ulonglong, _c.c_ulonglong] + [_vp] * 6 + [_sz, _vp]),
    'nabu_relu_f32': (_i, [_sz, _vp, _vp, _vp]),
    'nabu_relu_bwd_f32': (_i, [_sz, _vp, _vp, _vp, _vp]),
    'nabu_layer_norm_fwd': (_i, [_i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    'nabu_crc32c_host': (_c.c_uint32, [_c.c_char_p, _sz, _c.c_uint32]),
    'nabu_layer_norm_bwd': (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'nabu_splice_stack_f32': (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    'nabu_unstack_rows_f32': (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    'nabu_stack_rows_f32': (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    'nabu_rows_relu_ln_fwd': (_i, [_i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    'nabu_rows_relu_ln_bwd_parts': (_i, [_i]),
    'nabu_rows_relu_ln_bwd': (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'nabu_xent_wide_ws_bytes': (_sz, [_i, _i]),
    'nabu_xent_wide_loss_grad': (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _sz, _vp]),
    'nabu_xent_wide_smooth_loss_grad': (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    'nabu_log_softmax_prior_f32': (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'nabu_feat_dim': (_i, [_c.POINTER(FeatDesc)]),
    'nabu_feat_num_frames': (_i, [_c.POINTER(FeatDesc), _ll]),
    'nabu_feat_plan_host': (_i, [_c.POINTER(FeatDesc), _i, _vp, _vp, _vp]),
    'nabu_feat_ws_bytes': (_sz, [_c.POINTER(FeatDesc)]),
    'nabu_feat_tables_host': (_i, [_c.POINTER(FeatDesc), _vp, _sz]),
    'nabu_feat_compute': (_i, [_c.POINTER(FeatDesc), _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}

_lib = None
PHASE_HOOK_T = _c.CFUNCTYPE(None, _c.c_void_p)


class NabuHipError(RuntimeError):
    pass


def lib():
    """Load libnabu_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NabuHipError(
                'libnabu_hip.so is missing (%s): run `python -m nabu_amd.build` or '
                '__graft_entry__.build(); there is no CPU fallback' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if handle.nabu_version() != ABI_VERSION:
            raise NabuHipError('libnabu_hip.so reports ABI version %d, this binding is written against %d: rebuild '
                               '(python -m nabu_amd.build)' % (handle.nabu_version(), ABI_VERSION))
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().nabu_last_error().decode(errors='replace')
        raise NabuHipError('%s failed (%d): %s' % (what, code, msg))


def ptr(t):
    """Device pointer of a contiguous CUDA/HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise NabuHipError('tensor is not on the GPU (device=%s): the HIP path has no CPU fallback'
                           % t.device)
    if not t.is_contiguous():
        raise NabuHipError('tensor must be contiguous')
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Workspace(object):
    """Grow-only scratch buffers, one per (device, tag)."""
    _bufs = {}

    @classmethod
    def get(cls, nbytes, device, tag='ws'):
        key = (str(device), tag)
        buf = cls._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            # zero-filled: the first word of the 'blstm' workspace is the persistent
            # kernels' status word (0 = ok)
            buf = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            cls._bufs[key] = buf
        return buf


SPELLER_MAX_LAYERS = 4
GEMM_DEFAULT, GEMM_F32, GEMM_BF16, GEMM_BF16X3, GEMM_BF16X6 = 0, 1, 2, 3, 4
# NABU_ABI_VERSION of include/nabu_hip.h this binding was written against (lib() refuses another library)
ABI_VERSION = 4

GEMM_PRECISIONS = {'default': 0, 'f32': 1, 'bf16': 2, 'bf16x3': 3, 'bf16x6': 4, 'f16x3': 5}


class SpellerDesc(_c.Structure):
    _fields_ = [('size', _c.c_uint32)] + [(n, _c.c_int32) for n in
                                          ('B', 'Te', 'E', 'U', 'C', 'L', 'num_layers', 'kind', 'K', 'F', 'prob_fn')] + \
               [('keep_prob', _c.c_float), ('seed', _c.c_ulonglong), ('seed_offset', _c.c_ulonglong),
                ('sample_prob', _c.c_float), ('sample_seed', _c.c_ulonglong), ('sample_offset', _c.c_ulonglong)]


class BeamDesc(_c.Structure):
    _fields_ = [('size', _c.c_uint32)] + [(n, _c.c_int32) for n in
                                          ('B', 'Te', 'E', 'U', 'C', 'num_layers', 'kind', 'K', 'F', 'prob_fn',
                                           'beam_width', 'max_steps')] + \
               [('length_penalty', _c.c_float), ('temperature', _c.c_float)]


class BeamSearchOpts(_c.Structure):
    """nabu_beam_search_opts: the optional operands of nabu_speller[_multi]_beam_search_ex"""
    _fields_ = [('size', _c.c_uint32), ('ctc_logits', _c.c_void_p), ('ctc_weight', _c.c_float),
                ('lm_table', _c.c_void_p), ('lm_order', _c.c_int32), ('lm_weight', _c.c_float)]


LM_MAX_ENTRIES = 1 << 24        # entries of a label n-gram table the C side accepts (64 MiB)


class SpellerPtrs(_c.Structure):
    """nabu_speller_params / nabu_speller_grads (same layout, const or not)"""
    _fields_ = [(n, _c.c_void_p) for n in ('memory_kernel', 'query_kernel', 'attention_v', 'conv_kernel',
                                           'conv_proj', 'out_kernel', 'out_bias')] + \
               [('lstm_kernel', _c.c_void_p * SPELLER_MAX_LAYERS), ('lstm_bias', _c.c_void_p * SPELLER_MAX_LAYERS)]


SPELLER_MAX_MEMORIES = 4


class SpellerMultiDesc(_c.Structure):
    """nabu_speller_multi_desc: the Speller over M encoded inputs (Te, E per memory)"""
    _fields_ = [('size', _c.c_uint32)] + [(n, _c.c_int32) for n in ('M', 'B', 'U', 'C', 'L', 'num_layers')] + \
               [('Te', _c.c_int32 * SPELLER_MAX_MEMORIES), ('E', _c.c_int32 * SPELLER_MAX_MEMORIES)] + \
               [(n, _c.c_int32) for n in ('kind', 'K', 'F', 'prob_fn')] + \
               [('keep_prob', _c.c_float), ('seed', _c.c_ulonglong), ('seed_offset', _c.c_ulonglong),
                ('sample_prob', _c.c_float), ('sample_seed', _c.c_ulonglong), ('sample_offset', _c.c_ulonglong)]


class MultiBeamDesc(_c.Structure):
    _fields_ = [('size', _c.c_uint32)] + [(n, _c.c_int32) for n in ('M', 'B', 'U', 'C', 'num_layers')] + \
               [('Te', _c.c_int32 * SPELLER_MAX_MEMORIES), ('E', _c.c_int32 * SPELLER_MAX_MEMORIES)] + \
               [(n, _c.c_int32) for n in ('kind', 'K', 'F', 'prob_fn', 'beam_width', 'max_steps')] + \
               [('length_penalty', _c.c_float), ('temperature', _c.c_float)]


class SpellerMultiPtrs(_c.Structure):
    """nabu_speller_multi_params / nabu_speller_multi_grads (same layout, const or not)"""
    _fields_ = [(n, _c.c_void_p * SPELLER_MAX_MEMORIES) for n in ('memory_kernel', 'query_kernel', 'attention_v',
                                                                  'conv_kernel', 'conv_proj')] + \
               [('out_kernel', _c.c_void_p), ('out_bias', _c.c_void_p)] + \
               [('lstm_kernel', _c.c_void_p * SPELLER_MAX_LAYERS), ('lstm_bias', _c.c_void_p * SPELLER_MAX_LAYERS)]


class AttnDesc(_c.Structure):
    _fields_ = [('size', _c.c_uint32), ('B', _c.c_int32), ('Te', _c.c_int32), ('E', _c.c_int32),
                ('U', _c.c_int32), ('kind', _c.c_int32), ('K', _c.c_int32), ('F', _c.c_int32),
                ('prob_fn', _c.c_int32)]
