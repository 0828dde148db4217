"""ctypes binding of libbuzzdetect_hip.so — the declarations mirror include/buzzdetect_hip.h."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

from . import build as _build

ABI_VERSION = 5
EMBEDDER_BLOB_FLOATS = 3_217_344
EMBEDDING_SIZE = 1024
MEL_BANDS = 64
PATCH_FRAMES = 96
NUM_STAGES = 27
PROFILE_SLOTS = 29
MAX_CLASSES = 64

ERROR_NAMES = {-1: "BD_EINVAL", -2: "BD_ENODEVICE", -3: "BD_EHIP", -4: "BD_EWORKSPACE",
               -5: "BD_ERANGE", -6: "BD_EWEIGHTS"}


class BuzzdetectHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


class bd_weights(C.Structure):
    _fields_ = [
        ("embedder_blob", C.POINTER(C.c_float)),
        ("embedder_floats", C.c_int64),
        ("mel", C.POINTER(C.c_float)),
        ("head_kernel", C.POINTER(C.c_float)),
        ("head_bias", C.POINTER(C.c_float)),
        ("n_classes", C.c_int32),
    ]


# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_hip.h
PROTOTYPES = {
    "bd_abi_version": (C.c_int, []),
    "bd_last_error": (C.c_char_p, []),
    "bd_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(bd_weights)]),
    "bd_destroy": (C.c_int, [C.c_void_p]),
    "bd_set_group_windows": (C.c_int, [C.c_void_p, C.c_int32]),
    "bd_padded_length": (C.c_int64, [C.c_int64, C.c_int32]),
    "bd_num_frames": (C.c_int64, [C.c_int64, C.c_int32]),
    "bd_num_windows": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "bd_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "bd_resample_length": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "bd_resample_taps": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bd_set_resample_quality": (C.c_int, [C.c_void_p, C.c_int32]),
    "bd_format_rows": (C.c_int64, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_int64]),
    "bd_resample_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "bd_debug_fir_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "bd_resample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                              C.c_void_p]),
    "bd_resample_s16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p]),
    "bd_frontend": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_patches": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                           C.c_void_p, C.c_void_p]),
    "bd_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_batch_num_windows": (C.c_int64, [C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "bd_batch_workspace_bytes": (C.c_int64, [C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32]),
    "bd_predict_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_predict_chunks": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_calibrate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_get_scales": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "bd_set_activation_exponents": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "bd_stage_shape": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bd_stage_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                               C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_debug_pointwise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_void_p]),
    "bd_set_pointwise_variant": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "bd_set_pointwise_mode": (C.c_int, [C.c_void_p, C.c_int32]),
    "bd_range_flag": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p]),
    "bd_range_flag_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_set_fusion": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "bd_debug_pointwise_f16x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "bd_stager_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_int32]),
    "bd_stager_destroy": (C.c_int, [C.c_void_p]),
    "bd_stager_read": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "bd_stager_acquire": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]),
    "bd_stager_submit": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "bd_profile_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "bd_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]),
}

FLAC_ABI_VERSION = 1


class bd_flac_streaminfo(C.Structure):
    _fields_ = [("min_blocksize", C.c_int32), ("max_blocksize", C.c_int32), ("sample_rate", C.c_int32),
                ("channels", C.c_int32), ("bits_per_sample", C.c_int32), ("reserved", C.c_int32),
                ("total_samples", C.c_int64)]


class bd_flac_frame_header(C.Structure):
    _fields_ = [("number", C.c_int64), ("first_sample", C.c_int64), ("blocksize", C.c_int32), ("sample_rate", C.c_int32),
                ("channel_assignment", C.c_int32), ("channels", C.c_int32), ("bits_per_sample", C.c_int32),
                ("variable", C.c_int32), ("header_bytes", C.c_int32), ("reserved", C.c_int32)]


class bd_flac_status(C.Structure):
    _fields_ = [("samples", C.c_int64), ("stop_offset", C.c_int64), ("first_sample", C.c_int64), ("end_sample", C.c_int64),
                ("reason", C.c_int32), ("frames", C.c_int32)]


FLAC_STOP_NAMES = {0: "end", 1: "crc16", 2: "bad_subframe", 3: "lost_sync", 4: "truncated", 5: "overflow"}

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_flac.h
FLAC_PROTOTYPES = {
    "bd_flac_abi_version": (C.c_int, []),
    "bd_flac_crc8": (C.c_uint32, [C.c_void_p, C.c_int64]),
    "bd_flac_crc16": (C.c_uint32, [C.c_void_p, C.c_int64]),
    "bd_flac_parse_frame_header": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(bd_flac_streaminfo),
                                             C.POINTER(bd_flac_frame_header)]),
    "bd_flac_decode_host": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(bd_flac_streaminfo), C.c_int64, C.c_int64, C.c_void_p,
                                      C.POINTER(bd_flac_status)]),
    "bd_flac_workspace_bytes": (C.c_int64, [C.POINTER(bd_flac_streaminfo), C.c_int64, C.c_int64]),
    "bd_flac_decode": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(bd_flac_streaminfo), C.c_int64, C.c_int64, C.c_void_p,
                                 C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
}

PCM_ABI_VERSION = 1
PCM_MAX_COEFS = 32
PCM_LINEAR, PCM_FLOAT, PCM_ULAW, PCM_ALAW, PCM_IMA_ADPCM, PCM_MS_ADPCM = range(6)


class bd_pcm_format(C.Structure):
    _fields_ = [("codec", C.c_int32), ("channels", C.c_int32), ("bits", C.c_int32), ("big_endian", C.c_int32),
                ("is_signed", C.c_int32), ("block_align", C.c_int32), ("samples_per_block", C.c_int32), ("n_coefs", C.c_int32),
                ("coefs", C.c_int16 * (2 * PCM_MAX_COEFS))]


class bd_pcm_status(C.Structure):
    _fields_ = [("samples", C.c_int64), ("end_sample", C.c_int64), ("bad_block", C.c_int64), ("reason", C.c_int32),
                ("reserved", C.c_int32)]


PCM_STOP_NAMES = {0: "end", 1: "bad_header", 2: "truncated"}

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_pcm.h
PCM_PROTOTYPES = {
    "bd_pcm_abi_version": (C.c_int, []),
    "bd_pcm_decode_host": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(bd_pcm_format), C.c_int64, C.c_int64, C.c_void_p,
                                     C.POINTER(bd_pcm_status)]),
    "bd_pcm_workspace_bytes": (C.c_int64, [C.POINTER(bd_pcm_format), C.c_int64, C.c_int64]),
    "bd_pcm_decode": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(bd_pcm_format), C.c_int64, C.c_int64, C.c_void_p,
                                C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
}

HEAD_ABI_VERSION = 1
HEAD_MAX_LAYERS = 8
HEAD_MAX_WIDTH = 2048
HEAD_ACTIVATIONS = {"linear": 0, "relu": 1, "sigmoid": 2, "tanh": 3, "softmax": 4}


class bd_head_layer(C.Structure):
    _fields_ = [("kernel", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float)), ("n_in", C.c_int32), ("n_out", C.c_int32),
                ("activation", C.c_int32), ("reserved", C.c_int32)]


# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_head.h
HEAD_PROTOTYPES = {
    "bd_head_abi_version": (C.c_int, []),
    "bd_head_attach": (C.c_int, [C.c_void_p, C.POINTER(bd_head_layer), C.c_int32]),
    "bd_head_outputs": (C.c_int, [C.c_void_p]),
}

HEADSET_ABI_VERSION = 1
HEADSET_MAX_MEMBERS = 64
HEADSET_ROW = 2048                  # floats per window the hidden activations of one depth share (each width rounded up to 32)


class bd_headset_member(C.Structure):
    _fields_ = [("layers", C.POINTER(bd_head_layer)), ("n_layers", C.c_int32), ("reserved", C.c_int32)]


# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_headset.h
HEADSET_PROTOTYPES = {
    "bd_headset_abi_version": (C.c_int, []),
    "bd_headset_attach": (C.c_int, [C.c_void_p, C.POINTER(bd_headset_member), C.c_int32]),
    "bd_headset_members": (C.c_int, [C.c_void_p]),
    "bd_headset_outputs": (C.c_int, [C.c_void_p]),
    "bd_headset_columns": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}

ENSEMBLE_ABI_VERSION = 1
COMBINE_KINDS = {"none": 0, "mean": 1, "mean_probability": 2}
LINKS = {None: 0, "softmax": 1, "sigmoid": 2}


class bd_ensemble_output(C.Structure):
    _fields_ = [("first_member", C.c_int32), ("n_members", C.c_int32), ("combine", C.c_int32), ("link", C.c_int32)]


# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_ensemble.h
ENSEMBLE_PROTOTYPES = {
    "bd_ensemble_abi_version": (C.c_int, []),
    "bd_ensemble_attach": (C.c_int, [C.c_void_p, C.POINTER(bd_ensemble_output), C.c_int32]),
    "bd_ensemble_count": (C.c_int, [C.c_void_p]),
    "bd_ensemble_outputs": (C.c_int, [C.c_void_p]),
    "bd_ensemble_columns": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bd_ensemble_combine_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(bd_ensemble_output), C.c_int32,
                                           C.POINTER(C.c_int32), C.c_void_p, C.c_int32]),
}

ANYRATE_ABI_VERSION = 1

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_anyrate.h
ANYRATE_PROTOTYPES = {
    "bd_anyrate_abi_version": (C.c_int, []),
    "bd_anyrate_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "bd_resample_any": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p]),
    "bd_resample_any_s16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_void_p]),
    "bd_resample_any_host": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
}

TRAIN_ABI_VERSION = 2
TRAIN_SLICE_ROWS = 256
TRAIN_FUSED_MAX_WIDTH = 64
TRAIN_MAX_BATCH = 65536
TRAIN_LOSSES = {"categorical": 0, "binary": 1}
TRAIN_OPTIMIZERS = {"sgd": 0, "adam": 1}


class bd_train_optimizer(C.Structure):
    _fields_ = [("kind", C.c_int32), ("learning_rate", C.c_float), ("beta_1", C.c_float), ("beta_2", C.c_float),
                ("epsilon", C.c_float), ("reserved", C.c_int32)]


# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_train.h
TRAIN_PROTOTYPES = {
    "bd_train_abi_version": (C.c_int, []),
    "bd_trainer_create": (C.c_int, [C.c_int, C.POINTER(bd_head_layer), C.c_int32, C.c_int32, C.POINTER(bd_train_optimizer),
                                    C.c_int32, C.POINTER(C.c_void_p)]),
    "bd_trainer_destroy": (C.c_int, [C.c_void_p]),
    "bd_trainer_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_trainer_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_trainer_step_weighted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p]),
    "bd_trainer_loss_weighted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p]),
    "bd_trainer_set_weight_decay": (C.c_int, [C.c_void_p, C.c_float]),
    "bd_trainer_set_learning_rate": (C.c_int, [C.c_void_p, C.c_float]),
    "bd_trainer_snapshot": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bd_trainer_restore": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bd_trainer_gradients": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_trainer_read": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_trainer_logits": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_trainer_mean_loss": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_float)]),
    "bd_trainer_set_fusion": (C.c_int, [C.c_void_p, C.c_int32]),
    "bd_trainer_workspace_floats": (C.c_int64, [C.c_void_p]),
    "bd_trainer_workspace_fill": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bd_trainer_workspace_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
}

BANK_ABI_VERSION = 1
BANK_GROUP_COLUMNS = 64
BANK_MAX_MEMBERS = 4096
BANK_MAX_WORKSPACE_BYTES = 1 << 31

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_bank.h
BANK_PROTOTYPES = {
    "bd_bank_abi_version": (C.c_int, []),
    "bd_bank_create": (C.c_int, [C.c_int, C.POINTER(bd_head_layer), C.c_int32, C.c_int32, C.POINTER(bd_train_optimizer),
                                 C.c_int32, C.POINTER(C.c_void_p)]),
    "bd_bank_destroy": (C.c_int, [C.c_void_p]),
    "bd_bank_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                               C.c_void_p]),
    "bd_bank_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                               C.c_void_p, C.c_void_p]),
    "bd_bank_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_bank_set_learning_rate": (C.c_int, [C.c_void_p, C.c_int32, C.c_float]),
    "bd_bank_set_weight_decay": (C.c_int, [C.c_void_p, C.c_int32, C.c_float]),
    "bd_bank_set_frozen": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "bd_bank_snapshot": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_bank_restore": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_bank_read": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_bank_gradients": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_bank_mean_loss": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_bank_workspace_floats": (C.c_int64, [C.c_void_p]),
    "bd_bank_workspace_fill": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bd_bank_workspace_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
}

STACKBANK_ABI_VERSION = 1
STACKBANK_MAX_WORKSPACE_BYTES = 1 << 33

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_stackbank.h
STACKBANK_PROTOTYPES = {
    "bd_stackbank_abi_version": (C.c_int, []),
    "bd_stackbank_create": (C.c_int, [C.c_int, C.POINTER(bd_head_layer), C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(bd_train_optimizer), C.c_int32, C.POINTER(C.c_void_p)]),
    "bd_stackbank_destroy": (C.c_int, [C.c_void_p]),
    "bd_stackbank_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                    C.c_void_p]),
    "bd_stackbank_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                    C.c_void_p, C.c_void_p]),
    "bd_stackbank_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_stackbank_set_learning_rate": (C.c_int, [C.c_void_p, C.c_int32, C.c_float]),
    "bd_stackbank_set_weight_decay": (C.c_int, [C.c_void_p, C.c_int32, C.c_float]),
    "bd_stackbank_set_frozen": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "bd_stackbank_snapshot": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_stackbank_restore": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_stackbank_read": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_stackbank_gradients": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_stackbank_mean_loss": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_stackbank_workspace_floats": (C.c_int64, [C.c_void_p]),
    "bd_stackbank_workspace_fill": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bd_stackbank_workspace_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
}

MIX_ABI_VERSION = 1
MIX_SLICE = 4096
MIX_POWER_FLOOR = 1e-20
MIX_FLAG_SILENT_BACKGROUND = 1
MIX_MAX_CLIPS = 65536


class bd_mix_clip(C.Structure):
    _fields_ = [("ev_off", C.c_int64), ("nz_off", C.c_int64), ("out_off", C.c_int64), ("n", C.c_int32), ("ev_gain", C.c_float),
                ("ratio", C.c_float)]


# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_mix.h
MIX_PROTOTYPES = {
    "bd_mix_abi_version": (C.c_int, []),
    "bd_mix_workspace_bytes": (C.c_int64, [C.POINTER(bd_mix_clip), C.c_int32]),
    "bd_mix": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(bd_mix_clip), C.c_int32, C.c_void_p, C.c_int64,
                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_mix_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(bd_mix_clip), C.c_int32, C.c_void_p,
                              C.c_int64, C.c_void_p, C.c_void_p]),
}

SEARCH_ABI_VERSION = 1
SEARCH_DIM = 1024
SEARCH_MAX_QUERIES = 1024
SEARCH_MAX_K = 1024
SEARCH_MAX_WINDOWS = 1 << 20
SEARCH_NORM_FLOOR = 1e-30
SEARCH_METRICS = {"dot": 0, "cosine": 1}

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_search.h
SEARCH_PROTOTYPES = {
    "bd_search_abi_version": (C.c_int, []),
    "bd_search_packed_floats": (C.c_int64, [C.c_int32]),
    "bd_search_pack_queries": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_search_norms": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bd_search_norms_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_search_scores": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_int64, C.c_void_p]),
    "bd_search_update": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                   C.c_void_p]),
    "bd_search_update_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32]),
    "bd_search_decode_host": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
}

CLUSTER_ABI_VERSION = 1
CLUSTER_DIM = 1024
CLUSTER_MAX_CLUSTERS = 1024
CLUSTER_MAX_ROWS = 1 << 24
CLUSTER_CHUNK = 256
CLUSTER_STAT_SLICE = 256
CLUSTER_ORDER_SLICE = 1024
CLUSTER_METRICS = {"euclidean": 0, "cosine": 1}

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_cluster.h
CLUSTER_PROTOTYPES = {
    "bd_cluster_abi_version": (C.c_int, []),
    "bd_cluster_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "bd_cluster_assign": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "bd_cluster_order": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_cluster_order_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_cluster_centroids": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_cluster_centroids_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_cluster_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_cluster_stats_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
}

CALLS_ABI_VERSION = 1
CALLS_TILE = 1024
CALLS_MAX_WINDOWS = 1 << 20
CALLS_MAX_COLUMNS = 64
CALLS_MAX_BINS = 1 << 20
CALLS_EVENT_FIELDS = 5              # first, last, n_on, peak, kept


class bd_calls_rule(C.Structure):
    _fields_ = [("high", C.c_float), ("low", C.c_float), ("link", C.c_int32), ("min_extent", C.c_int32)]


# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_calls.h
CALLS_PROTOTYPES = {
    "bd_calls_abi_version": (C.c_int, []),
    "bd_calls_events": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_calls_events_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_calls_bins": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_calls_bins_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_void_p]),
}

EVAL_ABI_VERSION = 1
EVAL_BINS = 16384
EVAL_K_MIN = -8192
EVAL_PLANES = 3                     # negatives by kf, positives by kf, labelled rows by kr
EVAL_TAILS = 4                      # skipped, non-finite, below the range, above it
EVAL_SLICE = 32768
EVAL_MAX_WINDOWS = 1 << 24
EVAL_MAX_COLUMNS = 2048
EVAL_MAX_LABELS = 2048

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_eval.h
EVAL_PROTOTYPES = {
    "bd_eval_abi_version": (C.c_int, []),
    "bd_eval_state_bytes": (C.c_int64, [C.c_int32]),
    "bd_eval_accumulate": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_eval_accumulate_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
}

ROWS_ABI_VERSION = 1
ROWS_CODECS = {"f32": 0, "h": 1, "b": 2}
ROWS_SLICE = 256
ROWS_HEADER_BYTES = 16
ROWS_MAX_WINDOWS = 1 << 24
ROWS_BAD_EXPONENT = -(1 << 31)      # the record of a row that is not representable; it decodes to quiet NaN

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_rows.h
ROWS_PROTOTYPES = {
    "bd_rows_abi_version": (C.c_int, []),
    "bd_rows_record_bytes": (C.c_int64, [C.c_int32]),
    "bd_rows_encode": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_rows_decode": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_rows_encode_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_rows_decode_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_score_rows_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int64]),
    "bd_score_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
}

SUGGEST_ABI_VERSION = 1
SUGGEST_MAX_MEMBERS = 64
SUGGEST_MAX_WIDTH = 64
SUGGEST_MAX_POOL = 1024
SUGGEST_STRATEGIES = {"entropy": 0, "margin": 1, "bald": 2}

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_suggest.h
SUGGEST_PROTOTYPES = {
    "bd_suggest_abi_version": (C.c_int, []),
    "bd_suggest_acquire": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_suggest_acquire_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_int64]),
    "bd_suggest_pick": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "bd_suggest_pick_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
}

PITCH_ABI_VERSION = 1
PITCH_MAX_SELECTED = 1 << 20
PITCH_MAX_STEP = 1 << 24
PITCH_WINDOW = 15360
PITCH_FRAMES = 29
PITCH_FRAME = 1024
PITCH_INTEGRATION = 512
PITCH_MAX_LAG = 511


class bd_pitch_params(C.Structure):
    _fields_ = [("lag_lo", C.c_int32), ("lag_hi", C.c_int32), ("pick_ratio", C.c_float), ("clarity_min", C.c_float),
                ("min_voiced", C.c_int32), ("rate_hz", C.c_float)]


# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_pitch.h
PITCH_PROTOTYPES = {
    "bd_pitch_abi_version": (C.c_int, []),
    "bd_pitch_windows": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "bd_pitch_windows_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
}

HEALTH_ABI_VERSION = 1
HEALTH_S16 = 0
HEALTH_F32 = 1
HEALTH_MAX_CHANNELS = 8
HEALTH_SEGMENT = 4096
HEALTH_MAX_SEGMENTS = 1 << 24
HEALTH_MAX_RUN = 1 << 24
HEALTH_SUM_DEPTH = 24
HEALTH_FRAME = 1024
HEALTH_HOP = 512
HEALTH_BINS = 513
HEALTH_SEGMENT_FRAMES = 64
HEALTH_MAX_BANDS = 64
HEALTH_TABLE_FLOATS = 2048


class bd_health_level_params(C.Structure):
    _fields_ = [("clip_hi", C.c_float), ("clip_lo", C.c_float), ("clip_run", C.c_int32), ("flat_run", C.c_int32)]


class bd_health_record(C.Structure):
    _fields_ = [("n", C.c_int32), ("nonfinite", C.c_int32), ("peak", C.c_float), ("sum", C.c_float), ("sumsq", C.c_float),
                ("n_full", C.c_int32), ("clipped", C.c_int32), ("clip_runs", C.c_int32), ("flat", C.c_int32), ("flat_runs", C.c_int32)]


# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_health.h
HEALTH_PROTOTYPES = {
    "bd_health_abi_version": (C.c_int, []),
    "bd_health_check_cover": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_char_p]),
    "bd_health_levels_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "bd_health_levels": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_health_levels_host": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bd_health_tables": (C.c_int, [C.c_void_p]),
    "bd_health_spectrum": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "bd_health_spectrum_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
}

PCA_ABI_VERSION = 1
PCA_DIM = 1024
PCA_MAX_COMPONENTS = 64
PCA_MAX_ROWS = 1 << 18
PCA_SLICE = 1024
PCA_SUM_SLICE = 256
PCA_TILES = 528                     # 32 x 32 tiles of the Gram matrix's upper triangle, the diagonal included

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_pca.h
PCA_PROTOTYPES = {
    "bd_pca_abi_version": (C.c_int, []),
    "bd_pca_sums": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_pca_sums_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_pca_workspace_bytes": (C.c_int64, [C.c_int64]),
    "bd_pca_gram": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                              C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_pca_gram_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "bd_pca_project": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "bd_pca_project_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
}

KNN_ABI_VERSION = 1
KNN_DIM = 1024
KNN_MAX_K = 64
KNN_MAX_ROWS = 1 << 22
KNN_METRICS = {"dot": 0, "cosine": 1}

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_knn.h
KNN_PROTOTYPES = {
    "bd_knn_abi_version": (C.c_int, []),
    "bd_knn_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "bd_knn_update": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_knn_update_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                     C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    "bd_knn_decode_host": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
}

PROPAGATE_ABI_VERSION = 1
PROPAGATE_MAX_CLASSES = 64
PROPAGATE_MAX_POWER = 16
PROPAGATE_MAX_ROWS = 1 << 24
PROPAGATE_SLICE = 256

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_propagate.h
PROPAGATE_PROTOTYPES = {
    "bd_propagate_abi_version": (C.c_int, []),
    "bd_propagate_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_propagate_weights_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_propagate_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_propagate_step_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "bd_propagate_readout": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_propagate_readout_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

TSNE_ABI_VERSION = 1
TSNE_MAX_ROWS = 1 << 20
TSNE_MAX_K = 64
TSNE_SLICE = 2048
TSNE_ROWS_PER_BLOCK = 256
TSNE_BISECTIONS = 64

# name -> (restype, argtypes); one entry per prototype in include/buzzdetect_tsne.h
TSNE_PROTOTYPES = {
    "bd_tsne_abi_version": (C.c_int, []),
    "bd_tsne_workspace_bytes": (C.c_int64, [C.c_int64]),
    "bd_tsne_affinities": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_tsne_affinities_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "bd_tsne_attract": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bd_tsne_attract_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "bd_tsne_repulse": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_tsne_repulse_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "bd_tsne_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                 C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "bd_tsne_update_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                                      C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "bd_tsne_kl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_int64, C.c_void_p]),
    "bd_tsne_kl_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def library_path() -> str:
    return os.environ.get("BUZZDETECT_HIP_LIB", _build.LIB_PATH)


def load(build_if_missing: bool = True) -> C.CDLL:
    """Load the shared object (building it with hipcc first if it is not there).

    There is deliberately no fallback: if the library cannot be built or loaded this raises.
    """
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    external = "BUZZDETECT_HIP_LIB" in os.environ
    if not os.path.exists(path):
        if not build_if_missing or external:
            raise FileNotFoundError(f"{path} not found; run `python -m buzzdetect_amd.build`")
        _build.build()
    elif not external and _build.needs_build():
        # the in-tree library is older than its sources (it is git-ignored, so a checkout does not refresh it):
        # rebuild where hipcc exists, refuse to run stale kernels where it does not
        if not build_if_missing:
            raise RuntimeError(f"{path} is older than its sources; run `python -m buzzdetect_amd.build`")
        try:
            _build.build()
        except (RuntimeError, OSError, subprocess.CalledProcessError) as exc:
            raise RuntimeError(f"{path} is older than its sources and could not be rebuilt: {exc}") from exc
    lib = C.CDLL(path)
    for name, (res, args) in list(PROTOTYPES.items()) + list(FLAC_PROTOTYPES.items()) + list(PCM_PROTOTYPES.items()) \
            + list(HEAD_PROTOTYPES.items()) + list(HEADSET_PROTOTYPES.items()) + list(ENSEMBLE_PROTOTYPES.items()) + list(ANYRATE_PROTOTYPES.items()) + list(TRAIN_PROTOTYPES.items()) \
            + list(BANK_PROTOTYPES.items()) + list(STACKBANK_PROTOTYPES.items()) + list(MIX_PROTOTYPES.items()) \
            + list(SEARCH_PROTOTYPES.items()) + list(CLUSTER_PROTOTYPES.items()) + list(CALLS_PROTOTYPES.items()) \
            + list(EVAL_PROTOTYPES.items()) + list(ROWS_PROTOTYPES.items()) + list(SUGGEST_PROTOTYPES.items()) \
            + list(PITCH_PROTOTYPES.items()) + list(HEALTH_PROTOTYPES.items()) + list(PCA_PROTOTYPES.items()) \
            + list(KNN_PROTOTYPES.items()) + list(PROPAGATE_PROTOTYPES.items()) + list(TSNE_PROTOTYPES.items()):
        fn = getattr(lib, name)   # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.bd_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {lib.bd_abi_version()} != {ABI_VERSION}; rebuild")
    if lib.bd_flac_abi_version() != FLAC_ABI_VERSION:
        raise RuntimeError(f"{path}: FLAC ABI version {lib.bd_flac_abi_version()} != {FLAC_ABI_VERSION}; rebuild")
    if lib.bd_pcm_abi_version() != PCM_ABI_VERSION:
        raise RuntimeError(f"{path}: PCM ABI version {lib.bd_pcm_abi_version()} != {PCM_ABI_VERSION}; rebuild")
    if lib.bd_head_abi_version() != HEAD_ABI_VERSION:
        raise RuntimeError(f"{path}: head ABI version {lib.bd_head_abi_version()} != {HEAD_ABI_VERSION}; rebuild")
    if lib.bd_headset_abi_version() != HEADSET_ABI_VERSION:
        raise RuntimeError(f"{path}: head-set ABI version {lib.bd_headset_abi_version()} != {HEADSET_ABI_VERSION}; rebuild")
    if lib.bd_ensemble_abi_version() != ENSEMBLE_ABI_VERSION:
        raise RuntimeError(f"{path}: ensemble ABI version {lib.bd_ensemble_abi_version()} != {ENSEMBLE_ABI_VERSION}; rebuild")
    if lib.bd_anyrate_abi_version() != ANYRATE_ABI_VERSION:
        raise RuntimeError(f"{path}: any-ratio ABI version {lib.bd_anyrate_abi_version()} != {ANYRATE_ABI_VERSION}; rebuild")
    if lib.bd_train_abi_version() != TRAIN_ABI_VERSION:
        raise RuntimeError(f"{path}: trainer ABI version {lib.bd_train_abi_version()} != {TRAIN_ABI_VERSION}; rebuild")
    if lib.bd_bank_abi_version() != BANK_ABI_VERSION:
        raise RuntimeError(f"{path}: head-bank ABI version {lib.bd_bank_abi_version()} != {BANK_ABI_VERSION}; rebuild")
    if lib.bd_stackbank_abi_version() != STACKBANK_ABI_VERSION:
        raise RuntimeError(f"{path}: stack-bank ABI version {lib.bd_stackbank_abi_version()} != {STACKBANK_ABI_VERSION}; rebuild")
    if lib.bd_mix_abi_version() != MIX_ABI_VERSION:
        raise RuntimeError(f"{path}: mixer ABI version {lib.bd_mix_abi_version()} != {MIX_ABI_VERSION}; rebuild")
    if lib.bd_search_abi_version() != SEARCH_ABI_VERSION:
        raise RuntimeError(f"{path}: search ABI version {lib.bd_search_abi_version()} != {SEARCH_ABI_VERSION}; rebuild")
    if lib.bd_cluster_abi_version() != CLUSTER_ABI_VERSION:
        raise RuntimeError(f"{path}: cluster ABI version {lib.bd_cluster_abi_version()} != {CLUSTER_ABI_VERSION}; rebuild")
    if lib.bd_calls_abi_version() != CALLS_ABI_VERSION:
        raise RuntimeError(f"{path}: calls ABI version {lib.bd_calls_abi_version()} != {CALLS_ABI_VERSION}; rebuild")
    if lib.bd_eval_abi_version() != EVAL_ABI_VERSION:
        raise RuntimeError(f"{path}: eval ABI version {lib.bd_eval_abi_version()} != {EVAL_ABI_VERSION}; rebuild")
    if lib.bd_rows_abi_version() != ROWS_ABI_VERSION:
        raise RuntimeError(f"{path}: rows ABI version {lib.bd_rows_abi_version()} != {ROWS_ABI_VERSION}; rebuild")
    if lib.bd_suggest_abi_version() != SUGGEST_ABI_VERSION:
        raise RuntimeError(f"{path}: suggest ABI version {lib.bd_suggest_abi_version()} != {SUGGEST_ABI_VERSION}; rebuild")
    if lib.bd_pitch_abi_version() != PITCH_ABI_VERSION:
        raise RuntimeError(f"{path}: pitch ABI version {lib.bd_pitch_abi_version()} != {PITCH_ABI_VERSION}; rebuild")
    if lib.bd_health_abi_version() != HEALTH_ABI_VERSION:
        raise RuntimeError(f"{path}: health ABI version {lib.bd_health_abi_version()} != {HEALTH_ABI_VERSION}; rebuild")
    if lib.bd_pca_abi_version() != PCA_ABI_VERSION:
        raise RuntimeError(f"{path}: PCA ABI version {lib.bd_pca_abi_version()} != {PCA_ABI_VERSION}; rebuild")
    if lib.bd_knn_abi_version() != KNN_ABI_VERSION:
        raise RuntimeError(f"{path}: kNN ABI version {lib.bd_knn_abi_version()} != {KNN_ABI_VERSION}; rebuild")
    if lib.bd_propagate_abi_version() != PROPAGATE_ABI_VERSION:
        raise RuntimeError(f"{path}: propagation ABI version {lib.bd_propagate_abi_version()} != {PROPAGATE_ABI_VERSION}; rebuild")
    if lib.bd_tsne_abi_version() != TSNE_ABI_VERSION:
        raise RuntimeError(f"{path}: t-SNE ABI version {lib.bd_tsne_abi_version()} != {TSNE_ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int) -> int:
    if rc < 0:
        raise BuzzdetectHipError(int(rc), load().bd_last_error().decode(errors="replace"))
    return int(rc)
