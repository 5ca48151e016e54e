"""libpoporon_amd -- MI355X-native Reed-Solomon engine behind libpoporon's C API.

The product is the C-ABI shared library ``libpoporon_amd/libpoporon_amd.so``
(headers in ``include/``): the reference's ``poporon_*`` entry points
(include/poporon.h:67-99 of colopl/libpoporon) served by HIP kernels for
gfx950, plus the batch / device-pointer extension of ``include/poporon_amd.h``.

This module is the host-side mirror used by Python callers, the tests and
``bench.py``: a thin ctypes binding whose names, argument meaning and error
behaviour follow the reference API (``poporon_create``, ``poporon_encode``,
``poporon_decode``, erasure lists ...).  It never computes RS arithmetic
itself and it never falls back to a CPU path: if the shared library is
missing, importing the binding raises; if no GPU is usable, the codec calls
fail with the library's error message.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("POPORON_AMD_LIB") or os.path.join(HERE, "libpoporon_amd.so")  # override: experiments
INCLUDE_DIR = os.path.join(ROOT, "include")

POPORON_FEC_RS = 1
POPORON_FEC_LDPC = 2
POPORON_FEC_BCH = 3
POPORON_FEC_UNKNOWN = 255
# poporon_decode's *corrected_num after a device-side failure (include/poporon_amd.h)
DEVICE_ERROR = (1 << 64) - 1

_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)
_u32p = C.POINTER(C.c_uint32)
_vp = C.c_void_p

# name: (restype, argtypes)
_SIGS = {
    "poporon_rs_config_create": (_vp, [C.c_uint8, C.c_uint16, C.c_uint16, C.c_uint16, C.c_uint8, _vp, _vp]),
    "poporon_ldpc_config_create": (_vp, [C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_bool, C.c_bool, C.c_bool,
                                         C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_size_t, C.c_uint64]),
    "poporon_bch_config_create": (_vp, [C.c_uint8, C.c_uint16, C.c_uint8]),
    "poporon_config_rs_default": (_vp, []),
    "poporon_config_ldpc_default": (_vp, [C.c_size_t, C.c_int]),
    "poporon_config_ldpc_burst_resistant": (_vp, [C.c_size_t, C.c_int]),
    "poporon_config_bch_default": (_vp, []),
    "poporon_config_destroy": (None, [_vp]),
    "poporon_create": (_vp, [_vp]),
    "poporon_destroy": (None, [_vp]),
    "poporon_encode": (C.c_bool, [_vp, _vp, C.c_size_t, _vp]),
    "poporon_decode": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.POINTER(C.c_size_t)]),
    "poporon_get_fec_type": (C.c_int, [_vp]),
    "poporon_get_iterations_used": (C.c_uint32, [_vp]),
    "poporon_get_parity_size": (C.c_size_t, [_vp]),
    "poporon_get_info_size": (C.c_size_t, [_vp]),
    "poporon_version_id": (C.c_uint32, []),
    "poporon_buildtime": (C.c_uint32, []),
    "poporon_erasure_create": (_vp, [C.c_uint16, C.c_uint32]),
    "poporon_erasure_create_from_positions": (_vp, [C.c_uint16, _vp, C.c_uint32]),
    "poporon_erasure_add_position": (C.c_bool, [_vp, C.c_uint32]),
    "poporon_erasure_reset": (None, [_vp]),
    "poporon_erasure_destroy": (None, [_vp]),
    "poporon_gf_create": (_vp, [C.c_uint8, C.c_uint16]),
    "poporon_gf_destroy": (None, [_vp]),
    "poporon_gf_mod": (C.c_uint8, [_vp, C.c_uint16]),
    "poporon_rs_create": (_vp, [C.c_uint8, C.c_uint16, C.c_uint16, C.c_uint16, C.c_uint8]),
    "poporon_rs_destroy": (None, [_vp]),
    "poporon_amd_last_error": (C.c_char_p, []),
    "poporon_amd_device_count": (C.c_int, []),
    "poporon_amd_set_device": (C.c_bool, [_vp, C.c_int]),
    "poporon_amd_reserve": (C.c_bool, [_vp, C.c_size_t]),
    "poporon_amd_supported": (C.c_bool, [_vp]),
    "poporon_amd_timing": (C.c_bool, [_vp, C.c_int]),
    "poporon_amd_timing_read": (C.c_bool, [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "poporon_encode_batch_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp]),
    "poporon_decode_batch_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp,
                                               C.c_size_t, _vp, _vp, _vp, _vp]),
    "poporon_decode_batch_syndrome_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t,
                                                        C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp]),
    "poporon_check_batch_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp,
                                              _vp]),
    "poporon_encode_batch": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t]),
    "poporon_decode_batch": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp,
                                        C.c_size_t, _vp, _vp, _vp]),
    "poporon_encode_interleaved_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                     C.c_size_t, _vp]),
    "poporon_decode_interleaved_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                     C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
    "poporon_check_interleaved_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                    C.c_size_t, _vp, _vp]),
    "poporon_encode_interleaved": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                              C.c_size_t]),
    "poporon_decode_interleaved": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                              C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp]),
    "poporon_amd_reserve_interleaved": (C.c_bool, [_vp, C.c_size_t]),
    "poporon_amd_set_wire_form": (C.c_bool, [_vp, _vp, _vp, _vp, C.c_size_t]),
    "poporon_amd_set_wire_form_ccsds": (C.c_bool, [_vp, C.c_bool, C.c_bool]),
    "poporon_amd_get_wire_form": (C.c_bool, [_vp, _vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "poporon_decode_batch_report_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                      _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t,
                                                      _vp]),
    "poporon_decode_interleaved_report_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t,
                                                            C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp,
                                                            _vp, _vp, _vp, C.c_size_t, _vp]),
    "poporon_decode_batch_report": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp,
                                               C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t]),
    "poporon_amd_reserve_report": (C.c_bool, [_vp, C.c_size_t]),
    "poporon_amd_erasures_from_mask_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                                         _vp, C.c_size_t, _vp, _vp, _vp]),
    "poporon_amd_conv_span": (C.c_size_t, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    "poporon_amd_conv_tile": (C.c_size_t, [C.c_size_t, C.c_size_t, C.c_size_t]),
    "poporon_amd_conv_interleave_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                      C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp]),
    "poporon_amd_conv_deinterleave_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, C.c_size_t,
                                                        _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp]),
    "poporon_encode_conv_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                              C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp]),
    "poporon_decode_conv_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp,
                                              C.c_size_t, C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp,
                                              _vp]),
    "poporon_decode_conv_report_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, C.c_size_t,
                                                     _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp,
                                                     _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "poporon_check_conv_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                             _vp, _vp]),
    "poporon_amd_plane_tile": (C.c_size_t, [C.c_size_t]),
    "poporon_amd_reserve_planes": (C.c_bool, [_vp, C.c_size_t]),
    "poporon_encode_planes_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, _vp]),
    "poporon_decode_planes_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp,
                                                _vp]),
    "poporon_decode_planes_report_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp, _vp,
                                                       _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "poporon_check_planes_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp]),
    "poporon_encode_planes_strided_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t,
                                                        C.c_size_t, _vp]),
    "poporon_decode_planes_strided_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t,
                                                        C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
    "poporon_check_planes_strided_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t,
                                                       C.c_size_t, _vp, _vp]),
    "poporon_amd_soft_llr_row": (C.c_size_t, [_vp, C.c_size_t]),
    "poporon_amd_reserve_soft": (C.c_bool, [_vp, C.c_uint, C.c_size_t]),
    "poporon_decode_soft_batch_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t,
                                                    C.c_size_t, C.c_uint, _vp, _vp, _vp, _vp, _vp]),
    "poporon_amd_product_create": (_vp, [_vp, _vp]),
    "poporon_amd_product_destroy": (None, [_vp]),
    "poporon_amd_product_handle": (_vp, [_vp, C.c_int]),
    "poporon_amd_product_shape": (C.c_bool, [_vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t),
                                             C.POINTER(C.c_size_t)]),
    "poporon_amd_product_tile": (C.c_bool, [C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "poporon_amd_product_reserve": (C.c_bool, [_vp, C.c_size_t, C.c_size_t, C.c_size_t]),
    "poporon_encode_product_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                                 _vp]),
    "poporon_decode_product_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                                 C.c_int, C.c_size_t, C.c_int, _vp, _vp, _vp, _vp]),
    "poporon_check_product_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                                _vp, _vp, _vp, _vp]),
    "poporon_encode_product": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    "poporon_decode_product": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                          C.c_int, C.c_size_t, C.c_int, _vp, _vp, _vp]),
    "poporon_amd_cc_create": (_vp, [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint32, C.c_uint32, C.c_uint,
                                    C.c_uint]),
    "poporon_amd_cc_destroy": (None, [_vp]),
    "poporon_amd_cc_symbols": (C.c_size_t, [_vp, C.c_size_t]),
    "poporon_amd_cc_blocks": (C.c_size_t, [_vp, C.c_size_t]),
    "poporon_cc_encode_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _vp, C.c_size_t,
                                            _vp, _vp]),
    "poporon_cc_decode_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _vp,
                                            C.c_size_t, _vp, _vp]),
    "poporon_cc_decode_siso_device": (C.c_bool, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                                                 C.c_uint, _vp, C.c_size_t, _vp]),
    "poporon_rng_create": (_vp, [C.c_int, _vp, C.c_size_t]),
    "poporon_rng_destroy": (None, [_vp]),
    "poporon_rng_next": (C.c_bool, [_vp, _vp, C.c_size_t]),
    "poporon_amd_rng_fill_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp]),
    "poporon_syndrome_batch_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                 _vp, C.c_size_t, _vp, _vp]),
    "poporon_ldpc_encode_batch_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp]),
    "poporon_ldpc_decode_batch_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t,
                                                    _vp, _vp, _vp, C.c_size_t, _vp]),
    "poporon_ldpc_check_batch_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp, _vp]),
    "poporon_ldpc_encode_batch": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t]),
    "poporon_ldpc_decode_batch": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t,
                                             _vp, _vp, _vp, C.c_size_t]),
    "poporon_ldpc_check_batch": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp]),
    "poporon_amd_ldpc_graph": (C.c_bool, [_vp, _u32p, _u32p, _u32p, C.POINTER(_u32p), C.POINTER(_u32p),
                                          C.POINTER(_u32p), C.POINTER(_u32p)]),
    "poporon_amd_multi_create": (_vp, [_vp, _vp, C.c_size_t]),
    "poporon_amd_multi_destroy": (None, [_vp]),
    "poporon_amd_multi_device_count": (C.c_size_t, [_vp]),
    "poporon_amd_multi_handle": (_vp, [_vp, C.c_size_t]),
    "poporon_amd_multi_range": (C.c_bool, [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_size_t)]),
    "poporon_encode_batch_multi": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t]),
    "poporon_decode_batch_multi": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp,
                                              C.c_size_t, _vp, _vp, _vp]),
    "poporon_encode_batch_multi_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                     _vp]),
    "poporon_decode_batch_multi_device": (C.c_bool, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                     _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
}

# kernel ids for poporon_amd_timing_read (include/poporon_amd.h)
KERNEL_ENCODE, KERNEL_REMAINDER, KERNEL_CORRECT, KERNEL_CHECK = 0, 1, 2, 3
KERNEL_BM, KERNEL_CHIEN, KERNEL_FORNEY, KERNEL_LIST, KERNEL_APPLY, KERNEL_ERASURE, KERNEL_SINGLE = 4, 5, 6, 7, 8, 9, 10
KERNEL_WAVE = 11
KERNEL_LDPC_ENCODE, KERNEL_LDPC_DECODE, KERNEL_LDPC_CHECK = 12, 13, 14
KERNEL_ILV_GATHER, KERNEL_ILV_SCATTER = 15, 16
KERNEL_SNAPSHOT, KERNEL_REPORT, KERNEL_MASK_LISTS = 17, 18, 19
KERNEL_NAMES = {KERNEL_ENCODE: "rs_lfsr_k<false> (encode)", KERNEL_REMAINDER: "rs_lfsr_k<true> (remainder)",
                KERNEL_CORRECT: "rs_correct_k (BM/Chien/Forney)", KERNEL_BM: "rs_bm_k (BM/Omega)",
                KERNEL_CHIEN: "rs_chien_k (Chien)", KERNEL_FORNEY: "rs_forney_k (Forney)",
                KERNEL_APPLY: "rs_apply_k (apply)", KERNEL_LIST: "rs_wave_k (list)",
                KERNEL_ERASURE: "rs_era_bp_k (erasure)", KERNEL_SINGLE: "rs_dec1_k (one codeword)",
                KERNEL_WAVE: "rs_wave_k (small batch)"}
ILV_KERNEL_NAMES = {KERNEL_ILV_GATHER: "rs_ilv_gather_k (frames to rows)",
                    KERNEL_ILV_SCATTER: "rs_ilv_scatter_k (rows to frames)"}
REPORT_KERNEL_NAMES = {KERNEL_SNAPSHOT: "snapshot (device copy or rs_snapshot_k)", KERNEL_REPORT: "rs_report_k",
                       KERNEL_MASK_LISTS: "rs_mask_lists_k"}
KERNEL_CONV_GATHER, KERNEL_CONV_SCATTER = 20, 21
CONV_KERNEL_NAMES = {KERNEL_CONV_GATHER: "rs_conv_gather_k (stream to rows)",
                     KERNEL_CONV_SCATTER: "rs_conv_scatter_k (rows to stream)"}
KERNEL_PLANE_GATHER, KERNEL_PLANE_SCATTER = 22, 23
PLANE_KERNEL_NAMES = {KERNEL_PLANE_GATHER: "rs_plane_gather_k (planes to rows)",
                      KERNEL_PLANE_SCATTER: "rs_plane_scatter_k (rows to planes)"}
KERNEL_PROD_GATHER, KERNEL_PROD_SCATTER, KERNEL_PROD_LISTS = 24, 25, 26
PROD_KERNEL_NAMES = {KERNEL_PROD_GATHER: "rs_prod_gather_k (block to rows)",
                     KERNEL_PROD_SCATTER: "rs_prod_scatter_k (rows to block)",
                     KERNEL_PROD_LISTS: "rs_prod_lists_k / rs_prod_ok_k"}
KERNEL_SOFT_EXPAND, KERNEL_SOFT_SELECT = 27, 28
SOFT_KERNEL_NAMES = {KERNEL_SOFT_EXPAND: "rs_soft_expand_k (LLR rows to candidate rows)",
                     KERNEL_SOFT_SELECT: "rs_soft_select_k (scores and the winner's row)"}
LDPC_KERNEL_NAMES = {KERNEL_LDPC_ENCODE: "ldpc_encode_k", KERNEL_LDPC_DECODE: "ldpc_decode_k",
                     KERNEL_LDPC_CHECK: "ldpc_check_k"}

LDPC_RATE_1_3, LDPC_RATE_1_2, LDPC_RATE_2_3, LDPC_RATE_3_4, LDPC_RATE_4_5, LDPC_RATE_5_6 = range(6)
LDPC_RANDOM, LDPC_QC_RANDOM = 1, 2

_lib = None


def load_library(path: str = LIB_PATH):
    """Load the C-ABI library (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `make -C libpoporon_amd` (hipcc, gfx950)")
    # One HIP runtime per process: torch ships its own libamdhip64.so.7.  If
    # this library bound /opt/rocm's copy first, torch's HIP init would fail,
    # so let torch (when installed) load the runtime and share it.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def header_symbols(include_dir: str = INCLUDE_DIR):
    """Every function name declared in include/*.h and include/poporon/*.h."""
    names = []
    for sub in ("", "poporon"):
        d = os.path.join(include_dir, sub)
        for f in sorted(os.listdir(d)):
            if not f.endswith(".h"):
                continue
            text = open(os.path.join(d, f)).read()
            text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
            for m in re.finditer(r"\b(poporon_[a-z0-9_]+)\s*\(", text):
                if m.group(1) not in names:
                    names.append(m.group(1))
    return names


def conv_span(row_bytes: int, count: int, branches: int, cell: int) -> int:
    """poporon_amd_conv_span: bytes of stream that `count` codewords of row_bytes occupy behind a
    convolutional interleaver (count*row_bytes + (branches-1)*cell*branches); 0 on invalid arguments."""
    if min(row_bytes, count, branches, cell) < 0 or max(row_bytes, count, branches, cell) >= 1 << 64:
        return 0
    return int(load_library().poporon_amd_conv_span(row_bytes, count, branches, cell))


def conv_tile(row_bytes: int, branches: int, cell: int) -> int:
    """poporon_amd_conv_tile: codewords per workgroup of the convolutional layout kernels' LDS tile;
    0 where the window does not fit the LDS (the direct path)."""
    if min(row_bytes, branches, cell) < 0 or max(row_bytes, branches, cell) >= 1 << 64:
        return 0
    return int(load_library().poporon_amd_conv_tile(row_bytes, branches, cell))


def plane_tile(row_bytes: int) -> int:
    """poporon_amd_plane_tile: codewords per workgroup tile of the plane layout kernels; 0 for no row."""
    if row_bytes < 0 or row_bytes >= 1 << 64:
        return 0
    return int(load_library().poporon_amd_plane_tile(row_bytes))


def product_tile(codeword_bytes: int, codewords: int):
    """poporon_amd_product_tile: (whole blocks per workgroup tile, codewords of a block per tile) of the product
    layout kernels for blocks of `codewords` codewords of codeword_bytes; None for no such block."""
    if min(codeword_bytes, codewords) < 0 or max(codeword_bytes, codewords) >= 1 << 64:
        return None
    g, u = C.c_size_t(0), C.c_size_t(0)
    if not load_library().poporon_amd_product_tile(codeword_bytes, codewords, C.byref(g), C.byref(u)):
        return None
    return int(g.value), int(u.value)


def _plane_table(planes):
    """a host array of device pointers (ints; None or 0: NULL) for the plane calls"""
    return (C.c_void_p * len(planes))(*[p or None for p in planes])


def _lost_list(lost):
    lost = [] if lost is None else list(lost)
    return ((C.c_uint8 * len(lost))(*lost) if lost else None), len(lost)


def last_error() -> str:
    return load_library().poporon_amd_last_error().decode()


def device_count() -> int:
    return int(load_library().poporon_amd_device_count())


class PoporonError(RuntimeError):
    pass


def _buf(a):
    return a.ctypes.data_as(C.c_void_p)


def _u8(a, copy=False):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    return np.array(a, dtype=np.uint8, copy=True) if copy else np.ascontiguousarray(a, dtype=np.uint8)


def ccsds_dual_basis():
    """(to_code, to_wire) u8[256] each: CCSDS 131.0-B's conventional <-> dual-basis symbol maps,
    from the definition (numpy, independent of the library's own tables).  Field 0x187, alpha = 2,
    beta = alpha^117, Tr(a) = a + a^2 + ... + a^128: bit 7-i of to_wire[u] is Tr(u * beta^i)."""
    exp = np.zeros(255, np.int64)
    x = 1
    for i in range(255):
        exp[i] = x
        x <<= 1
        if x & 0x100:
            x ^= 0x187
    log = np.zeros(256, np.int64)
    log[exp] = np.arange(255)

    def mul(a, b):
        return np.where((a == 0) | (b == 0), 0, exp[(log[a] + log[b]) % 255])

    u = np.arange(256)
    to_wire = np.zeros(256, np.int64)
    for i in range(8):
        p = mul(u, np.full(256, exp[(117 * i) % 255]))
        tr = np.zeros(256, np.int64)
        for _ in range(8):
            tr ^= p
            p = mul(p, p)
        assert ((tr == 0) | (tr == 1)).all()
        to_wire |= tr << (7 - i)
    to_wire = to_wire.astype(np.uint8)
    to_code = np.zeros(256, np.uint8)
    to_code[to_wire] = u
    return to_code, to_wire


def ccsds_randomizer():
    """u8[255]: CCSDS 131.0-B's pseudo-randomizer, h(x) = x^8 + x^7 + x^5 + x^3 + 1 from the all-ones
    state, one period, bits packed MSB first."""
    s = [1] * 8
    bits = np.zeros(255 * 8, np.uint8)
    for n in range(bits.size):
        bits[n] = s[0]
        s = s[1:] + [s[0] ^ s[3] ^ s[5] ^ s[7]]
    return np.packbits(bits)


class Erasure:
    """poporon_erasure_t (include/poporon/erasure.h), reference src/erasure.c."""

    def __init__(self, num_roots: int = 32, initial_capacity: int = 0, positions=None):
        self.lib = load_library()
        if positions is not None:
            arr = np.ascontiguousarray(positions, dtype=np.uint32)
            self.h = self.lib.poporon_erasure_create_from_positions(num_roots, _buf(arr), arr.size)
        else:
            self.h = self.lib.poporon_erasure_create(num_roots, initial_capacity)
        if not self.h:
            raise PoporonError("poporon_erasure_create returned NULL")

    def add(self, position: int) -> bool:
        return bool(self.lib.poporon_erasure_add_position(self.h, int(position)))

    def reset(self):
        self.lib.poporon_erasure_reset(self.h)

    def set(self, positions):
        self.reset()
        for p in positions:
            self.add(p)

    def close(self):
        if getattr(self, "h", None):
            self.lib.poporon_erasure_destroy(self.h)
            self.h = None

    __del__ = close


class Poporon:
    """A poporon_t RS handle (poporon_rs_config_create + poporon_create).

    ``erasure`` (an :class:`Erasure`) and ``syndrome`` (32 log-form values) are
    borrowed and read live at every single-codeword decode, as in the reference.
    """

    def __init__(self, symbol_size=8, generator_polynomial=0x11D, first_consecutive_root=1, primitive_element=1,
                 num_roots=32, erasure: Erasure | None = None, syndrome=None, device: int | None = None):
        self.lib = load_library()
        self.erasure = erasure
        self._syn = None
        if syndrome is not None:
            self._syn = np.ascontiguousarray(syndrome, dtype=np.uint16)
        cfg = self.lib.poporon_rs_config_create(symbol_size, generator_polynomial, first_consecutive_root,
                                                primitive_element, num_roots, erasure.h if erasure else None,
                                                _buf(self._syn) if self._syn is not None else None)
        if not cfg:
            raise PoporonError("poporon_rs_config_create returned NULL")
        self.h = self.lib.poporon_create(cfg)
        self.lib.poporon_config_destroy(cfg)
        if not self.h:
            raise PoporonError(f"poporon_create returned NULL {last_error()}")
        self.num_roots = num_roots
        if device is not None:
            self._check(self.lib.poporon_amd_set_device(self.h, device), "poporon_amd_set_device")

    @classmethod
    def default(cls, **kw):
        """poporon_config_rs_default(): RS(255,223), 0x11D, fcr 1, prim 1."""
        return cls(8, 0x11D, 1, 1, 32, **kw)

    def close(self):
        if getattr(self, "h", None):
            self.lib.poporon_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, ok, what):
        if not ok:
            raise PoporonError(f"{what} failed: {last_error()}")

    # ---- getters ---------------------------------------------------------------
    @property
    def fec_type(self):
        return self.lib.poporon_get_fec_type(self.h)

    @property
    def parity_size(self):
        return self.lib.poporon_get_parity_size(self.h)

    @property
    def info_size(self):
        return self.lib.poporon_get_info_size(self.h)

    @property
    def supported(self):
        return bool(self.lib.poporon_amd_supported(self.h))

    # ---- single codeword (the reference's entry points) -------------------------
    def encode(self, data):
        """poporon_encode: returns the parity bytes (raises on failure)."""
        d = _u8(data)
        par = np.zeros(self.num_roots, np.uint8)
        self._check(self.lib.poporon_encode(self.h, _buf(d) if d.size else _buf(np.zeros(1, np.uint8)), d.size,
                                            _buf(par)), "poporon_encode")
        return par

    def decode(self, data, parity):
        """poporon_decode on copies: returns (ok, corrected_num, data', parity').

        A False result is a decode outcome (as in the reference), not an error,
        unless corrected_num == DEVICE_ERROR (a GPU failure; last_error() says which)."""
        d = _u8(data, copy=True)
        p = _u8(parity, copy=True)
        n = C.c_size_t(0)
        ok = self.lib.poporon_decode(self.h, _buf(d) if d.size else _buf(np.zeros(1, np.uint8)), d.size, _buf(p),
                                     C.byref(n))
        return bool(ok), int(n.value), d, p

    # ---- host batches ------------------------------------------------------------
    def encode_batch(self, data):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        count, size = data.shape
        par = np.zeros((count, self.num_roots), np.uint8)
        self._check(self.lib.poporon_encode_batch(self.h, _buf(data), size, _buf(par), self.num_roots, size, count),
                    "poporon_encode_batch")
        return par

    def decode_batch(self, data, parity, positions=None, counts=None):
        """Returns (ok u8[count], corrected u8[count], data', parity')."""
        d = np.array(data, dtype=np.uint8, copy=True, order="C")
        p = np.array(parity, dtype=np.uint8, copy=True, order="C")
        count, size = d.shape
        ok = np.zeros(count, np.uint8)
        cor = np.zeros(count, np.uint8)
        if positions is not None:
            pos = np.ascontiguousarray(positions, dtype=np.uint8)
            cnt = np.ascontiguousarray(counts, dtype=np.uint8)
            pargs = (_buf(pos), pos.shape[1], _buf(cnt))
        else:
            pargs = (None, 0, None)
        self._check(self.lib.poporon_decode_batch(self.h, _buf(d), size, _buf(p), p.shape[1], size, count, *pargs,
                                                  _buf(ok), _buf(cor)), "poporon_decode_batch")
        return ok, cor, d, p

    # ---- device batches (pointers + hipStream_t) ----------------------------------
    def encode_batch_device(self, d_data, data_stride, d_parity, parity_stride, size, count, stream=0):
        self._check(self.lib.poporon_encode_batch_device(self.h, d_data, data_stride, d_parity, parity_stride, size,
                                                         count, stream or None), "poporon_encode_batch_device")

    def decode_batch_device(self, d_data, data_stride, d_parity, parity_stride, size, count, d_ok, d_corrected=None,
                            d_positions=None, positions_stride=0, d_counts=None, stream=0):
        self._check(self.lib.poporon_decode_batch_device(self.h, d_data, data_stride, d_parity, parity_stride, size,
                                                         count, d_positions, positions_stride, d_counts, d_ok,
                                                         d_corrected, stream or None), "poporon_decode_batch_device")

    def decode_batch_syndrome_device(self, d_data, data_stride, d_parity, parity_stride, size, count, d_syndromes,
                                     syndrome_stride, d_ok, d_corrected=None, stream=0):
        """External-syndrome branch (src/decode.c:446-464) for a batch: d_syndromes holds num_roots
        u16 log-form syndromes per codeword, syndrome_stride elements apart."""
        self._check(self.lib.poporon_decode_batch_syndrome_device(self.h, d_data, data_stride, d_parity,
                                                                  parity_stride, size, count, d_syndromes,
                                                                  syndrome_stride, d_ok, d_corrected, stream or None),
                    "poporon_decode_batch_syndrome_device")

    def syndrome_batch_device(self, d_data, data_stride, d_parity, parity_stride, size, count, d_syndromes,
                              syndrome_stride, d_nonzero=None, stream=0):
        """calculate_syndrome_u8 for a batch: u16 log-form syndromes (+ nonzero flags)."""
        self._check(self.lib.poporon_syndrome_batch_device(self.h, d_data, data_stride, d_parity, parity_stride, size,
                                                           count, d_syndromes, syndrome_stride, d_nonzero,
                                                           stream or None), "poporon_syndrome_batch_device")

    def check_batch_device(self, d_data, data_stride, d_parity, parity_stride, size, count, d_dirty, stream=0):
        self._check(self.lib.poporon_check_batch_device(self.h, d_data, data_stride, d_parity, parity_stride, size,
                                                        count, d_dirty, stream or None), "poporon_check_batch_device")

    def reserve(self, max_count):
        self._check(self.lib.poporon_amd_reserve(self.h, max_count), "poporon_amd_reserve")

    # ---- symbol-interleaved frames (include/poporon_amd.h) --------------------------
    # frame f: message symbol j of codeword i at d_data + f*data_stride + j*depth + i, parity symbol p at
    # d_parity + f*parity_stride + p*depth + i; count frames; per-codeword arrays indexed by f*depth + i
    def encode_interleaved_device(self, d_data, data_stride, d_parity, parity_stride, size, depth, count, stream=0):
        self._check(self.lib.poporon_encode_interleaved_device(self.h, d_data, data_stride, d_parity, parity_stride,
                                                               size, depth, count, stream or None),
                    "poporon_encode_interleaved_device")

    def decode_interleaved_device(self, d_data, data_stride, d_parity, parity_stride, size, depth, count, d_ok,
                                  d_corrected=None, d_positions=None, positions_stride=0, d_counts=None, stream=0):
        self._check(self.lib.poporon_decode_interleaved_device(self.h, d_data, data_stride, d_parity, parity_stride,
                                                               size, depth, count, d_positions, positions_stride,
                                                               d_counts, d_ok, d_corrected, stream or None),
                    "poporon_decode_interleaved_device")

    def check_interleaved_device(self, d_data, data_stride, d_parity, parity_stride, size, depth, count, d_dirty,
                                 stream=0):
        self._check(self.lib.poporon_check_interleaved_device(self.h, d_data, data_stride, d_parity, parity_stride,
                                                              size, depth, count, d_dirty, stream or None),
                    "poporon_check_interleaved_device")

    def reserve_interleaved(self, max_codewords):
        self._check(self.lib.poporon_amd_reserve_interleaved(self.h, max_codewords),
                    "poporon_amd_reserve_interleaved")

    def encode_interleaved(self, frames, depth):
        """frames u8[count, size*depth] (message regions) -> parity regions u8[count, num_roots*depth]."""
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        count, width = fr.shape
        if depth < 1 or width % depth:
            raise PoporonError(f"frame width {width} is no multiple of depth {depth}")
        par = np.zeros((count, self.num_roots * depth), np.uint8)
        self._check(self.lib.poporon_encode_interleaved(self.h, _buf(fr), width, _buf(par), par.shape[1],
                                                        width // depth, depth, count), "poporon_encode_interleaved")
        return par

    def decode_interleaved(self, frames, parity, depth, positions=None, counts=None):
        """Returns (ok u8[count*depth], corrected u8[count*depth], frames', parity'); positions
        u8[count*depth, >= num_roots] and counts u8[count*depth] select the erasure decode."""
        d = np.array(frames, dtype=np.uint8, copy=True, order="C")
        p = np.array(parity, dtype=np.uint8, copy=True, order="C")
        count, width = d.shape
        if depth < 1 or width % depth:
            raise PoporonError(f"frame width {width} is no multiple of depth {depth}")
        ok = np.zeros(count * depth, np.uint8)
        cor = np.zeros(count * depth, np.uint8)
        if positions is not None:
            pos = np.ascontiguousarray(positions, dtype=np.uint8)
            cnt = np.ascontiguousarray(counts, dtype=np.uint8)
            pargs = (_buf(pos), pos.shape[1], _buf(cnt))
        else:
            pargs = (None, 0, None)
        self._check(self.lib.poporon_decode_interleaved(self.h, _buf(d), width, _buf(p), p.shape[1], width // depth,
                                                        depth, count, *pargs, _buf(ok), _buf(cor)),
                    "poporon_decode_interleaved")
        return ok, cor, d, p

    # ---- wire form of the interleaved calls (include/poporon_amd.h) -------------------
    def set_wire_form(self, to_code=None, to_wire=None, xor_seq=None):
        """Symbol map (u8[256] each, mutually inverse; both or neither) and receive-side XOR
        sequence (1 .. 65536 bytes) of the *_interleaved* calls; all None clears the form."""
        maps = [None if t is None else _u8(t) for t in (to_code, to_wire)]
        if any(t is not None and t.size != 256 for t in maps):
            raise PoporonError("a symbol map has 256 entries")
        seq = None if xor_seq is None else _u8(xor_seq).reshape(-1)
        self._check(self.lib.poporon_amd_set_wire_form(self.h, *(None if t is None else _buf(t) for t in maps),
                                                       None if seq is None else _buf(seq),
                                                       0 if seq is None else seq.size),
                    "poporon_amd_set_wire_form")

    def set_wire_form_ccsds(self, dual_basis=True, randomizer=True):
        """CCSDS 131.0-B: Berlekamp's dual-basis symbols and / or the 255-byte pseudo-randomizer."""
        self._check(self.lib.poporon_amd_set_wire_form_ccsds(self.h, bool(dual_basis), bool(randomizer)),
                    "poporon_amd_set_wire_form_ccsds")

    def wire_form(self):
        """(to_code u8[256], to_wire u8[256], xor_seq u8[n]) as last set, or None when no form is set."""
        tc, tw = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
        seq = np.zeros(65536, np.uint8)
        n = C.c_size_t(0)
        if not self.lib.poporon_amd_get_wire_form(self.h, _buf(tc), _buf(tw), _buf(seq), seq.size, C.byref(n)):
            return None
        return tc, tw, seq[:n.value].copy()

    # ---- decode reports and erasure lists from flag planes (include/poporon_amd.h) ---
    # the report of codeword c: d_err_num[c] changed bytes, their positions (0 .. size-1 message,
    # size .. parity) and before ^ after at d_err_pos / d_err_val + c*report_stride
    def decode_batch_report_device(self, d_data, data_stride, d_parity, parity_stride, size, count, d_ok,
                                   d_err_num, d_err_pos, d_err_val, report_stride, d_corrected=None,
                                   d_positions=None, positions_stride=0, d_counts=None, stream=0):
        self._check(self.lib.poporon_decode_batch_report_device(self.h, d_data, data_stride, d_parity, parity_stride,
                                                                size, count, d_positions, positions_stride, d_counts,
                                                                d_ok, d_corrected, d_err_num, d_err_pos, d_err_val,
                                                                report_stride, stream or None),
                    "poporon_decode_batch_report_device")

    def decode_interleaved_report_device(self, d_data, data_stride, d_parity, parity_stride, size, depth, count, d_ok,
                                         d_err_num, d_err_pos, d_err_val, report_stride, d_corrected=None,
                                         d_positions=None, positions_stride=0, d_counts=None, stream=0):
        self._check(self.lib.poporon_decode_interleaved_report_device(self.h, d_data, data_stride, d_parity,
                                                                      parity_stride, size, depth, count, d_positions,
                                                                      positions_stride, d_counts, d_ok, d_corrected,
                                                                      d_err_num, d_err_pos, d_err_val, report_stride,
                                                                      stream or None),
                    "poporon_decode_interleaved_report_device")

    def decode_batch_report(self, data, parity, positions=None, counts=None):
        """Returns (data', parity', ok u8[count], corrected u8[count], err_num u8[count],
        err_pos u8[count, num_roots], err_val u8[count, num_roots])."""
        d = np.array(data, dtype=np.uint8, copy=True, order="C")
        p = np.array(parity, dtype=np.uint8, copy=True, order="C")
        count, size = d.shape
        nr = self.num_roots
        ok, cor, num = (np.zeros(count, np.uint8) for _ in range(3))
        epos, eval_ = np.zeros((count, nr), np.uint8), np.zeros((count, nr), np.uint8)
        if positions is not None:
            pos = np.ascontiguousarray(positions, dtype=np.uint8)
            cnt = np.ascontiguousarray(counts, dtype=np.uint8)
            pargs = (_buf(pos), pos.shape[1], _buf(cnt))
        else:
            pargs = (None, 0, None)
        self._check(self.lib.poporon_decode_batch_report(self.h, _buf(d), size, _buf(p), p.shape[1], size, count,
                                                         *pargs, _buf(ok), _buf(cor), _buf(num), _buf(epos),
                                                         _buf(eval_), nr), "poporon_decode_batch_report")
        return d, p, ok, cor, num, epos, eval_

    def reserve_report(self, max_codewords):
        self._check(self.lib.poporon_amd_reserve_report(self.h, max_codewords), "poporon_amd_reserve_report")

    def erasures_from_mask_device(self, d_mask, mask_stride, size, depth, count, d_positions, positions_stride,
                                  d_counts, d_over=None, stream=0):
        """flag plane in the layout of the message regions (count frames) -> ascending erasure lists"""
        self._check(self.lib.poporon_amd_erasures_from_mask_device(self.h, d_mask, mask_stride, size, depth, count,
                                                                   d_positions, positions_stride, d_counts, d_over,
                                                                   stream or None),
                    "poporon_amd_erasures_from_mask_device")

    # ---- convolutional-interleaver streams (include/poporon_amd.h) --------------------
    # byte n = c*(size + num_roots) + s of the batch lies at d_stream + n + ((phase + n) % branches)*cell*branches;
    # d_stream is offset 0 of the batch's span of conv_span(size + num_roots, count, branches, cell) bytes
    def conv_interleave_device(self, d_data, data_stride, d_parity, parity_stride, size, count, branches, cell,
                               phase, d_stream, stream=0):
        self._check(self.lib.poporon_amd_conv_interleave_device(self.h, d_data, data_stride, d_parity, parity_stride,
                                                                size, count, branches, cell, phase, d_stream,
                                                                stream or None),
                    "poporon_amd_conv_interleave_device")

    def conv_deinterleave_device(self, d_stream, branches, cell, phase, d_data, data_stride, d_parity, parity_stride,
                                 size, count, stream=0):
        self._check(self.lib.poporon_amd_conv_deinterleave_device(self.h, d_stream, branches, cell, phase, d_data,
                                                                  data_stride, d_parity, parity_stride, size, count,
                                                                  stream or None),
                    "poporon_amd_conv_deinterleave_device")

    def encode_conv_device(self, d_data, data_stride, d_parity, parity_stride, size, count, branches, cell, phase,
                           d_stream, stream=0):
        self._check(self.lib.poporon_encode_conv_device(self.h, d_data, data_stride, d_parity, parity_stride, size,
                                                        count, branches, cell, phase, d_stream, stream or None),
                    "poporon_encode_conv_device")

    def decode_conv_device(self, d_stream, branches, cell, phase, d_data, data_stride, d_parity, parity_stride, size,
                           count, d_ok, d_corrected=None, d_positions=None, positions_stride=0, d_counts=None,
                           stream=0):
        self._check(self.lib.poporon_decode_conv_device(self.h, d_stream, branches, cell, phase, d_data, data_stride,
                                                        d_parity, parity_stride, size, count, d_positions,
                                                        positions_stride, d_counts, d_ok, d_corrected,
                                                        stream or None), "poporon_decode_conv_device")

    def decode_conv_report_device(self, d_stream, branches, cell, phase, d_data, data_stride, d_parity, parity_stride,
                                  size, count, d_ok, d_err_num, d_err_pos, d_err_val, report_stride,
                                  d_corrected=None, d_positions=None, positions_stride=0, d_counts=None, stream=0):
        self._check(self.lib.poporon_decode_conv_report_device(self.h, d_stream, branches, cell, phase, d_data,
                                                               data_stride, d_parity, parity_stride, size, count,
                                                               d_positions, positions_stride, d_counts, d_ok,
                                                               d_corrected, d_err_num, d_err_pos, d_err_val,
                                                               report_stride, stream or None),
                    "poporon_decode_conv_report_device")

    def check_conv_device(self, d_stream, branches, cell, phase, size, count, d_dirty, stream=0):
        self._check(self.lib.poporon_check_conv_device(self.h, d_stream, branches, cell, phase, size, count, d_dirty,
                                                       stream or None), "poporon_check_conv_device")

    # ---- plane layout: stripes across shards (include/poporon_amd.h) ------------------
    # planes: size + num_roots device pointers (None: NULL), symbol j of codeword c at planes[j] + c;
    # lost: ascending plane indices (host)
    def reserve_planes(self, max_codewords):
        self._check(self.lib.poporon_amd_reserve_planes(self.h, max_codewords), "poporon_amd_reserve_planes")

    def encode_planes_device(self, planes, size, count, stream=0):
        self._check(self.lib.poporon_encode_planes_device(self.h, _plane_table(planes), size, count, stream or None),
                    "poporon_encode_planes_device")

    def decode_planes_device(self, planes, size, count, d_ok, lost=None, d_corrected=None, d_dirty=None, stream=0):
        la, ln = _lost_list(lost)
        self._check(self.lib.poporon_decode_planes_device(self.h, _plane_table(planes), size, count, la, ln, d_ok,
                                                          d_corrected, d_dirty, stream or None),
                    "poporon_decode_planes_device")

    def decode_planes_report_device(self, planes, size, count, d_ok, d_err_num, d_err_pos, d_err_val, report_stride,
                                    lost=None, d_corrected=None, d_dirty=None, stream=0):
        la, ln = _lost_list(lost)
        self._check(self.lib.poporon_decode_planes_report_device(self.h, _plane_table(planes), size, count, la, ln,
                                                                 d_ok, d_corrected, d_dirty, d_err_num, d_err_pos,
                                                                 d_err_val, report_stride, stream or None),
                    "poporon_decode_planes_report_device")

    def check_planes_device(self, planes, size, count, d_dirty, stream=0):
        self._check(self.lib.poporon_check_planes_device(self.h, _plane_table(planes), size, count, d_dirty,
                                                         stream or None), "poporon_check_planes_device")

    def encode_planes_strided_device(self, d_data, data_plane_stride, d_parity, parity_plane_stride, size, count,
                                     stream=0):
        self._check(self.lib.poporon_encode_planes_strided_device(self.h, d_data, data_plane_stride, d_parity,
                                                                  parity_plane_stride, size, count, stream or None),
                    "poporon_encode_planes_strided_device")

    def decode_planes_strided_device(self, d_data, data_plane_stride, d_parity, parity_plane_stride, size, count,
                                     d_ok, lost=None, d_corrected=None, d_dirty=None, stream=0):
        la, ln = _lost_list(lost)
        self._check(self.lib.poporon_decode_planes_strided_device(self.h, d_data, data_plane_stride, d_parity,
                                                                  parity_plane_stride, size, count, la, ln, d_ok,
                                                                  d_corrected, d_dirty, stream or None),
                    "poporon_decode_planes_strided_device")

    def check_planes_strided_device(self, d_data, data_plane_stride, d_parity, parity_plane_stride, size, count,
                                    d_dirty, stream=0):
        self._check(self.lib.poporon_check_planes_strided_device(self.h, d_data, data_plane_stride, d_parity,
                                                                 parity_plane_stride, size, count, d_dirty,
                                                                 stream or None),
                    "poporon_check_planes_strided_device")

    # ---- soft-decision decode: Chase-2 over int8 bit LLRs (include/poporon_amd.h) ------
    # codeword c: soft_llr_row(size) int8 values at llr_ptr + c*llr_stride, bit j (MSB first) of symbol s
    # at s*symbol_size + j, negative = 1; the rows at data_ptr / par_ptr are outputs only
    def soft_llr_row(self, size):
        return int(self.lib.poporon_amd_soft_llr_row(self.h, size))

    def reserve_soft(self, flips, max_codewords):
        self._check(self.lib.poporon_amd_reserve_soft(self.h, flips, max_codewords), "poporon_amd_reserve_soft")

    def decode_soft_batch_device(self, llr_ptr, llr_stride, data_ptr, ds, par_ptr, ps, size, count, flips, ok_ptr,
                                 changed_ptr=0, pattern_ptr=0, score_ptr=0, stream=0):
        self._check(self.lib.poporon_decode_soft_batch_device(self.h, llr_ptr or None, llr_stride, data_ptr or None, ds,
                                                              par_ptr or None, ps, size, count, flips, ok_ptr or None,
                                                              changed_ptr or None, pattern_ptr or None,
                                                              score_ptr or None, stream or None),
                    "poporon_decode_soft_batch_device")

    # ---- in-library kernel timing (HIP events on the launch stream) ---------------
    def timing(self, enable: bool):
        self._check(self.lib.poporon_amd_timing(self.h, int(enable)), "poporon_amd_timing")

    def timing_read(self, kernel: int):
        ms = C.c_double(0)
        n = C.c_uint64(0)
        self._check(self.lib.poporon_amd_timing_read(self.h, kernel, C.byref(ms), C.byref(n)), "poporon_amd_timing_read")
        return ms.value, n.value


class Bch(Poporon):
    """A PPLN_FEC_BCH handle (poporon_bch_config_create + poporon_create): binary
    BCH over GF(2^m), messages and parity as big-endian byte images
    (src/encode.c:199-233, src/decode.c:542-590).  Same methods as
    :class:`Poporon`; ``parity_size``/``info_size`` are the byte-image sizes."""

    def __init__(self, symbol_size=4, generator_polynomial=0x13, correction_capability=3, device=None):
        self.lib = load_library()
        self.erasure = None
        self._syn = None
        cfg = self.lib.poporon_bch_config_create(symbol_size, generator_polynomial, correction_capability)
        if not cfg:
            raise PoporonError("poporon_bch_config_create returned NULL")
        self.h = self.lib.poporon_create(cfg)
        self.lib.poporon_config_destroy(cfg)
        if not self.h:
            raise PoporonError(f"poporon_create returned NULL {last_error()}")
        self.num_roots = int(self.lib.poporon_get_parity_size(self.h))  # parity bytes (array shapes)
        if device is not None:
            self._check(self.lib.poporon_amd_set_device(self.h, device), "poporon_amd_set_device")

    @classmethod
    def default(cls, **kw):
        """poporon_config_bch_default(): BCH(15, 5) over GF(16), 0x13, t = 3."""
        return cls(4, 0x13, 3, **kw)

    def decode(self, data, parity, corrected_init=0):
        """poporon_decode on copies: (ok, corrected_num, data').  As in the
        reference, corrected_num is left at corrected_init on failure."""
        d = _u8(data, copy=True)
        p = _u8(parity, copy=True)
        n = C.c_size_t(corrected_init)
        ok = self.lib.poporon_decode(self.h, _buf(d) if d.size else _buf(np.zeros(1, np.uint8)), d.size,
                                     _buf(p) if p.size else _buf(np.zeros(1, np.uint8)), C.byref(n))
        return bool(ok), int(n.value), d


class Ldpc(Poporon):
    """A PPLN_FEC_LDPC handle (poporon_ldpc_config_create + poporon_create), the
    reference's src/ldpc.c behind ldpc_encode / ldpc_decode (src/encode.c:147-197,
    src/decode.c:489-540).  The constructor takes poporon_ldpc_config_create's 13
    parameters; ``soft_llr`` (codeword_bits int8) is copied once and borrowed by
    the handle: :meth:`set_llr` rewrites it in place before a soft ``decode``.

    The two convenience constructors of the C API stay stubs; their argument
    lists are ``Ldpc(block, rate, LDPC_RANDOM, 3, True, True, True)`` (default)
    and ``Ldpc(block, rate, LDPC_RANDOM, 7, True, True, True)`` (burst resistant).
    """

    def __init__(self, block_size, rate, matrix_type=LDPC_RANDOM, column_weight=3, use_soft_decode=False,
                 use_outer_interleave=False, use_inner_interleave=False, interleave_depth=0, lifting_factor=0,
                 max_iterations=0, soft_llr=None, soft_llr_size=0, seed=0, device=None):
        self.lib = load_library()
        self.erasure = None
        self._syn = None
        self._llr = None if soft_llr is None else np.array(soft_llr, dtype=np.int8, copy=True, order="C")
        cfg = self.lib.poporon_ldpc_config_create(block_size, rate, matrix_type, column_weight, use_soft_decode,
                                                  use_outer_interleave, use_inner_interleave, interleave_depth,
                                                  lifting_factor, max_iterations,
                                                  _buf(self._llr) if self._llr is not None else None,
                                                  soft_llr_size or (self._llr.size if self._llr is not None else 0),
                                                  seed)
        if not cfg:
            raise PoporonError(f"poporon_ldpc_config_create returned NULL {last_error()}")
        self.h = self.lib.poporon_create(cfg)
        self.lib.poporon_config_destroy(cfg)
        if not self.h:
            raise PoporonError(f"poporon_create returned NULL {last_error()}")
        self.info_bytes = int(self.lib.poporon_get_info_size(self.h))
        self.parity_bytes = int(self.lib.poporon_get_parity_size(self.h))
        self.num_roots = self.parity_bytes  # parity bytes (array shapes of the base class)
        self.codeword_bytes = self.info_bytes + self.parity_bytes
        nb = C.c_uint32(0)
        self._check(self.lib.poporon_amd_ldpc_graph(self.h, None, C.byref(nb), None, None, None, None, None),
                    "poporon_amd_ldpc_graph")
        self.codeword_bits = int(nb.value)
        if device is not None:
            self._check(self.lib.poporon_amd_set_device(self.h, device), "poporon_amd_set_device")

    @property
    def iterations_used(self):
        return int(self.lib.poporon_get_iterations_used(self.h))

    def graph(self):
        """poporon_amd_ldpc_graph: dict of num_checks, num_bits, num_edges, row_ptr, col_idx,
        inner_forward, outer_forward (copies; the last two None when that interleaver is off)."""
        nc, nb, ne = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        rp, ci, inf, outf = _u32p(), _u32p(), _u32p(), _u32p()
        self._check(self.lib.poporon_amd_ldpc_graph(self.h, C.byref(nc), C.byref(nb), C.byref(ne), C.byref(rp),
                                                    C.byref(ci), C.byref(inf), C.byref(outf)),
                    "poporon_amd_ldpc_graph")
        arr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy() if p else None  # noqa: E731
        return dict(num_checks=nc.value, num_bits=nb.value, num_edges=ne.value, row_ptr=arr(rp, nc.value + 1),
                    col_idx=arr(ci, ne.value), inner_forward=arr(inf, nb.value),
                    outer_forward=arr(outf, self.info_bytes))

    def set_llr(self, llr):
        """Rewrite the borrowed soft_llr buffer (same size) for the next soft ``decode``."""
        self._llr[...] = np.asarray(llr, dtype=np.int8).reshape(self._llr.shape)

    # ---- single codeword ----------------------------------------------------------
    def encode(self, data):
        """poporon_encode: (data', parity); data' differs from data when an interleaver is on."""
        d = _u8(data, copy=True)
        par = np.zeros(max(self.parity_bytes, 1), np.uint8)
        self._check(self.lib.poporon_encode(self.h, _buf(d), d.size, _buf(par)), "poporon_encode")
        return d, par[:self.parity_bytes]

    def decode(self, data, parity, corrected_init=0):
        """poporon_decode on copies: (ok, corrected_num, data').  corrected_num is the
        iteration count on success and stays at corrected_init on failure."""
        d = _u8(data, copy=True)
        p = _u8(parity, copy=True)
        n = C.c_size_t(corrected_init)
        ok = self.lib.poporon_decode(self.h, _buf(d), d.size, _buf(p), C.byref(n))
        return bool(ok), int(n.value), d

    # ---- host batches ---------------------------------------------------------------
    def encode_batch(self, data):
        """(data', parity) of every row."""
        d = np.array(data, dtype=np.uint8, copy=True, order="C")
        count = d.shape[0]
        par = np.zeros((count, self.parity_bytes), np.uint8)
        self._check(self.lib.poporon_ldpc_encode_batch(self.h, _buf(d), d.shape[1], _buf(par), self.parity_bytes,
                                                       count), "poporon_ldpc_encode_batch")
        return d, par

    def decode_batch(self, data, parity, llr=None, want_hard=True):
        """(ok u8[count], iterations u32[count], data', hard u8[count, codeword_bytes] or None);
        ``llr`` (int8[count, codeword_bits]) selects the soft path."""
        d = np.array(data, dtype=np.uint8, copy=True, order="C")
        p = np.ascontiguousarray(parity, dtype=np.uint8)
        count = d.shape[0]
        ok = np.zeros(count, np.uint8)
        it = np.zeros(count, np.uint32)
        hard = np.zeros((count, self.codeword_bytes), np.uint8) if want_hard else None
        l = None if llr is None else np.ascontiguousarray(llr, dtype=np.int8)
        self._check(self.lib.poporon_ldpc_decode_batch(self.h, _buf(d), d.shape[1], _buf(p), p.shape[1],
                                                       _buf(l) if l is not None else None,
                                                       l.shape[1] if l is not None else 0, count, _buf(ok), _buf(it),
                                                       _buf(hard) if want_hard else None, self.codeword_bytes),
                    "poporon_ldpc_decode_batch")
        return ok, it, d, hard

    def check_batch(self, data, parity):
        d = np.ascontiguousarray(data, dtype=np.uint8)
        p = np.ascontiguousarray(parity, dtype=np.uint8)
        dirty = np.zeros(d.shape[0], np.uint8)
        self._check(self.lib.poporon_ldpc_check_batch(self.h, _buf(d), d.shape[1], _buf(p), p.shape[1], d.shape[0],
                                                      _buf(dirty)), "poporon_ldpc_check_batch")
        return dirty

    # ---- device batches (pointers + hipStream_t) ---------------------------------------
    def encode_batch_device(self, d_data, data_stride, d_parity, parity_stride, count, stream=0):
        self._check(self.lib.poporon_ldpc_encode_batch_device(self.h, d_data, data_stride, d_parity, parity_stride,
                                                              count, stream or None),
                    "poporon_ldpc_encode_batch_device")

    def decode_batch_device(self, d_data, data_stride, d_parity, parity_stride, count, d_ok, d_iterations=None,
                            d_hard=None, hard_stride=0, d_llr=None, llr_stride=0, stream=0):
        self._check(self.lib.poporon_ldpc_decode_batch_device(self.h, d_data, data_stride, d_parity, parity_stride,
                                                              d_llr, llr_stride, count, d_ok, d_iterations, d_hard,
                                                              hard_stride, stream or None),
                    "poporon_ldpc_decode_batch_device")

    def check_batch_device(self, d_data, data_stride, d_parity, parity_stride, count, d_dirty, stream=0):
        self._check(self.lib.poporon_ldpc_check_batch_device(self.h, d_data, data_stride, d_parity, parity_stride,
                                                             count, d_dirty, stream or None),
                    "poporon_ldpc_check_batch_device")


class Rng:
    """poporon_rng_t (include/poporon/rng.h): xoshiro128++ seeded by splitmix32,
    reference src/rng.c.  ``next`` fills host memory; ``fill_device`` writes
    the same stream into device memory (poporon_amd_rng_fill_device)."""

    def __init__(self, seed: int | bytes | None = 0, rng_type: int = 0):
        self.lib = load_library()
        if seed is None:
            self.h = self.lib.poporon_rng_create(rng_type, None, 0)
        else:
            b = seed if isinstance(seed, (bytes, bytearray)) else int(seed).to_bytes(4, "little")
            buf = np.frombuffer(bytes(b), dtype=np.uint8).copy()
            self.h = self.lib.poporon_rng_create(rng_type, _buf(buf), buf.size)
        if not self.h:
            raise PoporonError("poporon_rng_create returned NULL")

    def next(self, size: int) -> np.ndarray:
        out = np.zeros(max(size, 1), np.uint8)
        if not self.lib.poporon_rng_next(self.h, _buf(out), size):
            raise PoporonError("poporon_rng_next failed")
        return out[:size]

    def fill_device(self, d_dest, size, stream=0):
        if not self.lib.poporon_amd_rng_fill_device(self.h, d_dest, size, stream or None):
            raise PoporonError(f"poporon_amd_rng_fill_device failed: {last_error()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.poporon_rng_destroy(self.h)
            self.h = None

    __del__ = close


def shard_range(count: int, rank: int, world: int):
    """Contiguous codeword range [lo, hi) of `rank` out of `world`:
    the library's own partition (poporon_amd_multi_range), [count*r/W, count*(r+1)/W)."""
    first, n = C.c_size_t(0), C.c_size_t(0)
    if not load_library().poporon_amd_multi_range(count, world, rank, C.byref(first), C.byref(n)):
        raise PoporonError(f"poporon_amd_multi_range failed: {last_error()}")
    return int(first.value), int(first.value + n.value)


class Multi:
    """poporon_multi_t (include/poporon_amd.h): one RS handle per device, each
    codeword range on its own device; host batches run the devices concurrently."""

    def __init__(self, devices=None, symbol_size=8, generator_polynomial=0x11D, first_consecutive_root=1,
                 primitive_element=1, num_roots=32):
        self.lib = load_library()
        cfg = self.lib.poporon_rs_config_create(symbol_size, generator_polynomial, first_consecutive_root,
                                                primitive_element, num_roots, None, None)
        if not cfg:
            raise PoporonError("poporon_rs_config_create returned NULL")
        if devices is None:
            self.h = self.lib.poporon_amd_multi_create(cfg, None, 0)
        else:
            arr = (C.c_int * len(devices))(*devices)
            self.h = self.lib.poporon_amd_multi_create(cfg, arr, len(devices))
        self.lib.poporon_config_destroy(cfg)
        if not self.h:
            raise PoporonError(f"poporon_amd_multi_create failed: {last_error()}")
        self.num_roots = num_roots

    @property
    def devices(self):
        return int(self.lib.poporon_amd_multi_device_count(self.h))

    def _check(self, ok, what):
        if not ok:
            raise PoporonError(f"{what} failed: {last_error()}")

    def encode_batch(self, data):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        count, size = data.shape
        par = np.zeros((count, self.num_roots), np.uint8)
        self._check(self.lib.poporon_encode_batch_multi(self.h, _buf(data), size, _buf(par), self.num_roots, size,
                                                        count), "poporon_encode_batch_multi")
        return par

    def decode_batch(self, data, parity, positions=None, counts=None):
        d = np.array(data, dtype=np.uint8, copy=True, order="C")
        p = np.array(parity, dtype=np.uint8, copy=True, order="C")
        count, size = d.shape
        ok = np.zeros(count, np.uint8)
        cor = np.zeros(count, np.uint8)
        if positions is not None:
            pos = np.ascontiguousarray(positions, dtype=np.uint8)
            cnt = np.ascontiguousarray(counts, dtype=np.uint8)
            pargs = (_buf(pos), pos.shape[1], _buf(cnt))
        else:
            pargs = (None, 0, None)
        self._check(self.lib.poporon_decode_batch_multi(self.h, _buf(d), size, _buf(p), p.shape[1], size, count,
                                                        *pargs, _buf(ok), _buf(cor)), "poporon_decode_batch_multi")
        return ok, cor, d, p

    def encode_batch_device(self, d_data, data_stride, d_parity, parity_stride, size, count, streams=None):
        """d_data / d_parity / streams: one pointer per device (device i's range of rows)."""
        G = self.devices
        arr = lambda v: (C.c_void_p * G)(*v)  # noqa: E731
        self._check(self.lib.poporon_encode_batch_multi_device(self.h, arr(d_data), data_stride, arr(d_parity),
                                                               parity_stride, size, count,
                                                               arr(streams) if streams else None),
                    "poporon_encode_batch_multi_device")

    def decode_batch_device(self, d_data, data_stride, d_parity, parity_stride, size, count, d_ok, d_corrected=None,
                            streams=None, d_positions=None, positions_stride=0, d_counts=None):
        """d_positions / d_counts (erasure batches): one pointer per device, as d_data."""
        G = self.devices
        arr = lambda v: (C.c_void_p * G)(*v)  # noqa: E731
        self._check(self.lib.poporon_decode_batch_multi_device(self.h, arr(d_data), data_stride, arr(d_parity),
                                                               parity_stride, size, count,
                                                               arr(d_positions) if d_positions else None,
                                                               positions_stride,
                                                               arr(d_counts) if d_counts else None, arr(d_ok),
                                                               arr(d_corrected) if d_corrected else None,
                                                               arr(streams) if streams else None),
                    "poporon_decode_batch_multi_device")

    def close(self):
        if getattr(self, "h", None):
            self.lib.poporon_amd_multi_destroy(self.h)
            self.h = None

    __del__ = close


class _Borrowed(Poporon):
    """a handle another object owns: never destroyed from here"""

    def close(self):
        self.h = None

    __del__ = close


class Product:
    """poporon_product_t (include/poporon_amd.h): RS x RS product-code blocks, a row code and a column code
    over one field.  ``row`` / ``col``: (symbol_size, generator_polynomial, first_consecutive_root,
    primitive_element, num_roots).  Block b is n2 rows of n1 bytes, byte (i, j) at d_blocks + b*block_stride +
    i*row_pitch + j; count is in blocks."""

    def __init__(self, row, col, device: int | None = None):
        self.lib = load_library()
        cfgs = [self.lib.poporon_rs_config_create(*p, None, None) for p in (row, col)]
        try:
            if not all(cfgs):
                raise PoporonError("poporon_rs_config_create returned NULL")
            self.h = self.lib.poporon_amd_product_create(*cfgs)
        finally:
            for c in cfgs:
                if c:
                    self.lib.poporon_config_destroy(c)
        if not self.h:
            raise PoporonError(f"poporon_amd_product_create failed: {last_error()}")
        self.row_roots, self.col_roots = row[4], col[4]
        if device is not None:
            self._check(self.lib.poporon_amd_set_device(self.handle(0).h, device), "poporon_amd_set_device")

    def _check(self, ok, what):
        if not ok:
            raise PoporonError(f"{what} failed: {last_error()}")

    def handle(self, axis):
        """the axis's own handle (0: row code, 1: column code) as a Poporon that does not own it: timing()"""
        h = self.lib.poporon_amd_product_handle(self.h, axis)
        if not h:
            raise PoporonError("poporon_amd_product_handle: axis is neither 0 nor 1")
        p = _Borrowed.__new__(_Borrowed)
        p.lib, p.h, p.erasure, p._syn = self.lib, h, None, None
        p.num_roots = (self.row_roots, self.col_roots)[axis]
        p._owner = self
        return p

    def shape(self, row_size, col_size):
        n1, n2 = C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.poporon_amd_product_shape(self.h, row_size, col_size, C.byref(n1), C.byref(n2)),
                    "poporon_amd_product_shape")
        return int(n1.value), int(n2.value)

    def reserve(self, row_size, col_size, max_blocks):
        self._check(self.lib.poporon_amd_product_reserve(self.h, row_size, col_size, max_blocks),
                    "poporon_amd_product_reserve")

    def encode_device(self, d_blocks, row_pitch, block_stride, row_size, col_size, count, stream=0):
        self._check(self.lib.poporon_encode_product_device(self.h, d_blocks, row_pitch, block_stride, row_size,
                                                           col_size, count, stream or None),
                    "poporon_encode_product_device")

    def decode_device(self, d_blocks, row_pitch, block_stride, row_size, col_size, count, first_axis=0, passes=2,
                      couple=1, d_row_dirty=None, d_col_dirty=None, d_block_ok=None, stream=0):
        self._check(self.lib.poporon_decode_product_device(self.h, d_blocks, row_pitch, block_stride, row_size,
                                                           col_size, count, first_axis, passes, couple, d_row_dirty,
                                                           d_col_dirty, d_block_ok, stream or None),
                    "poporon_decode_product_device")

    def check_device(self, d_blocks, row_pitch, block_stride, row_size, col_size, count, d_row_dirty=None,
                     d_col_dirty=None, d_block_ok=None, stream=0):
        self._check(self.lib.poporon_check_product_device(self.h, d_blocks, row_pitch, block_stride, row_size,
                                                          col_size, count, d_row_dirty, d_col_dirty, d_block_ok,
                                                          stream or None), "poporon_check_product_device")

    def encode(self, messages):
        """host form on packed blocks: u8[count, k2, k1] messages -> u8[count, n2, n1] encoded blocks"""
        m = np.ascontiguousarray(messages, dtype=np.uint8)
        count, k2, k1 = m.shape
        n1, n2 = self.shape(k1, k2)
        out = np.zeros((count, n2, n1), np.uint8)
        out[:, :k2, :k1] = m
        self._check(self.lib.poporon_encode_product(self.h, _buf(out), n1, n1 * n2, k1, k2, count),
                    "poporon_encode_product")
        return out

    def decode(self, blocks, row_size, col_size, first_axis=0, passes=2, couple=1):
        """host form on packed blocks u8[count, n2, n1]: (blocks', row_dirty u8[count, n2], col_dirty u8[count, n1],
        block_ok u8[count])"""
        b = np.array(blocks, dtype=np.uint8, copy=True, order="C")
        count, n2, n1 = b.shape
        rd, cd, ok = np.zeros((count, n2), np.uint8), np.zeros((count, n1), np.uint8), np.zeros(count, np.uint8)
        self._check(self.lib.poporon_decode_product(self.h, _buf(b), n1, n1 * n2, row_size, col_size, count,
                                                    first_axis, passes, couple, _buf(rd), _buf(cd), _buf(ok)),
                    "poporon_decode_product")
        return b, rd, cd, ok

    def close(self):
        if getattr(self, "h", None):
            self.lib.poporon_amd_product_destroy(self.h)
            self.h = None

    __del__ = close


# ---- K = 7 convolutional code (include/poporon_amd.h) --------------------------------
# (g0, g1, invert)
CC_CODE_CCSDS = (0o171, 0o133, 2)
CC_CODE_DVB = (0o171, 0o133, 0)
# (period, keep0, keep1): bit k of a mask is phase k
CC_PUNCTURE_NONE = (1, 0b1, 0b1)
CC_PUNCTURE_DVB_2_3 = (2, 0b01, 0b11)
CC_PUNCTURE_DVB_3_4 = (3, 0b101, 0b011)
CC_PUNCTURE_DVB_5_6 = (5, 0b10101, 0b01011)
CC_PUNCTURE_DVB_7_8 = (7, 0b1010001, 0b0101111)
CC_DEFAULT_BLOCK, CC_DEFAULT_OVERLAP = 0, 0xFFFFFFFF  # the values that select the library defaults


def _dptr(a):
    """a device pointer: an int (None or 0: NULL) or a torch tensor"""
    if a is None:
        return None
    return (a.data_ptr() if hasattr(a, "data_ptr") else int(a)) or None


class Cc:
    """poporon_cc_t (include/poporon_amd.h): the K = 7, rate-1/2 convolutional code with puncturing.  ``code`` is
    (g0, g1, invert), ``puncture`` (period, keep0, keep1); ``block`` / ``overlap`` are the decoder's B and V.
    Buffers are device pointers (ints) or torch tensors; bits and symbols are packed MSB first, LLRs are int8."""

    def __init__(self, code=CC_CODE_DVB, puncture=CC_PUNCTURE_NONE, block=CC_DEFAULT_BLOCK,
                 overlap=CC_DEFAULT_OVERLAP):
        self.lib = load_library()
        self.h = self.lib.poporon_amd_cc_create(*code, *puncture, block, overlap)
        if not self.h:
            raise PoporonError(f"poporon_amd_cc_create failed: {last_error()}")

    def _check(self, ok, what):
        if not ok:
            raise PoporonError(f"{what} failed: {last_error()}")

    def symbols(self, nbits):
        return int(self.lib.poporon_amd_cc_symbols(self.h, nbits))

    def blocks(self, nbits):
        return int(self.lib.poporon_amd_cc_blocks(self.h, nbits))

    def encode(self, d_bits, bits_stride, nbits, count, d_symbols, symbols_stride, start_state=0, d_end_state=None,
               stream=0):
        self._check(self.lib.poporon_cc_encode_device(self.h, _dptr(d_bits), bits_stride, nbits, count, start_state,
                                                      _dptr(d_symbols), symbols_stride, _dptr(d_end_state),
                                                      stream or None), "poporon_cc_encode_device")

    def decode(self, d_llr, llr_stride, nbits, count, d_bits, bits_stride, start_state=-1, end_state=-1,
               d_metric=None, stream=0):
        self._check(self.lib.poporon_cc_decode_device(self.h, _dptr(d_llr), llr_stride, nbits, count, start_state,
                                                      end_state, _dptr(d_bits), bits_stride, _dptr(d_metric),
                                                      stream or None), "poporon_cc_decode_device")

    def decode_soft(self, d_llr, llr_stride, nbits, count, d_soft, soft_stride, start_state=-1, end_state=-1, shift=0,
                    stream=0):
        """max-log-MAP: one int8 per info bit (negative = 1), |D_1 - D_0| >> shift saturated at 127; with shift 0 and
        nbits a multiple of 8 a frame's row is an LLR row of Poporon.decode_soft_batch_device (m = 8)"""
        self._check(self.lib.poporon_cc_decode_siso_device(self.h, _dptr(d_llr), llr_stride, nbits, count, start_state,
                                                           end_state, shift, _dptr(d_soft), soft_stride,
                                                           stream or None), "poporon_cc_decode_siso_device")

    def close(self):
        if getattr(self, "h", None):
            self.lib.poporon_amd_cc_destroy(self.h)
            self.h = None

    __del__ = close
