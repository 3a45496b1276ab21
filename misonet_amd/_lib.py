"""ctypes binding of libmisonet_hip.so (C ABI: include/misonet.h).

There is no CPU fallback: if the shared library is missing or does not load, every compute entry point raises.
Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C misonet_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MISONET_LIB_PATH: another build of this same library, for A/B measurements of two builds on one box (tools/gpu_ab_lib.sh);
# normal use never sets it
LIB_PATH = os.environ.get("MISONET_LIB_PATH") or os.path.join(_HERE, "libmisonet_hip.so")

OK, EINVAL, ESTATE, EHIP, ENOMEM, ENAN = 0, -1, -2, -3, -4, -5


class MisonetError(RuntimeError):
    def __init__(self, code, detail):
        super().__init__(f"libmisonet_hip error {code}: {detail}")
        self.code = code


class Cfg(C.Structure):
    _fields_ = [("in_ch", C.c_int), ("out_ch", C.c_int), ("en_ch", C.c_int * 7), ("de_ch", C.c_int * 7),
                ("n_freq", C.c_int), ("tcn_norm", C.c_int)]       # tcn_norm: 0 IN, 1 gLN, 2 cLN, 3 BatchNorm1d (ABI 400)


class BfOpts(C.Structure):
    """misonet_bf_opts (ABI 510): kind 0 mvdr / 1 souden / 2 gev, noise 0 residual / 1 mix"""
    _fields_ = [("kind", C.c_int), ("noise", C.c_int), ("condition", C.c_double), ("trace_normalize", C.c_int),
                ("epsi", C.c_float), ("ban", C.c_int), ("ref_ch", C.c_int)]


class WpeOpts(C.Structure):
    """misonet_wpe_opts (ABI 520)"""
    _fields_ = [("taps", C.c_int), ("delay", C.c_int), ("iterations", C.c_int), ("diag_load", C.c_double),
                ("power_floor", C.c_double)]


class OwpeOpts(C.Structure):
    """misonet_owpe_opts (ABI 620)"""
    _fields_ = [("taps", C.c_int), ("delay", C.c_int), ("context", C.c_int), ("alpha", C.c_double),
                ("power_floor", C.c_double), ("init", C.c_double)]


class OivaOpts(C.Structure):
    """misonet_oiva_opts (ABI 630): model 0 gauss / 1 laplace"""
    _fields_ = [("model", C.c_int), ("ref_ch", C.c_int), ("alpha", C.c_double), ("floor", C.c_double), ("init", C.c_double)]


class ObfOpts(C.Structure):
    """misonet_obf_opts (ABI 640): noise 0 residual / 1 mix"""
    _fields_ = [("noise", C.c_int), ("ref_ch", C.c_int), ("alpha", C.c_double), ("mu", C.c_double), ("diag_load", C.c_double),
                ("epsi", C.c_double), ("init", C.c_double)]


class WpdOpts(C.Structure):
    """misonet_wpd_opts (ABI 530)"""
    _fields_ = [("taps", C.c_int), ("delay", C.c_int), ("diag_load", C.c_double), ("power_floor", C.c_double),
                ("ref_ch", C.c_int)]


class CacgmmOpts(C.Structure):
    """misonet_cacgmm_opts (ABI 560): prior 0 bin / 1 guided"""
    _fields_ = [("iterations", C.c_int), ("prior", C.c_int), ("diag_load", C.c_double), ("prior_floor", C.c_double)]


class JbfOpts(C.Structure):
    """misonet_jbf_opts (ABI 570): kind 0 lcmv / 1 mwf / 2 r1mwf, noise 0 residual / 1 mix, rtf 0 cw / 1 eig"""
    _fields_ = [("kind", C.c_int), ("noise", C.c_int), ("rtf", C.c_int), ("mu", C.c_double), ("diag_load", C.c_double),
                ("ref_ch", C.c_int)]


class DoaOpts(C.Structure):
    """misonet_doa_opts (ABI 610): kind 0 srp / 1 srp_phat / 2 music, block 0 = all frames, hop 0 = block, f_hi -1 = F - 1"""
    _fields_ = [("kind", C.c_int), ("num_src", C.c_int), ("block", C.c_int), ("hop", C.c_int), ("f_lo", C.c_int),
                ("f_hi", C.c_int), ("min_sep", C.c_double)]


class IvaOpts(C.Structure):
    """misonet_iva_opts (ABI 580): model 0 gauss / 1 laplace, channels 0 = the number of sources"""
    _fields_ = [("iterations", C.c_int), ("model", C.c_int), ("channels", C.c_int), ("ref_ch", C.c_int), ("floor", C.c_double)]


# name -> (restype, argtypes); every symbol declared in include/misonet.h
SIGNATURES = {
    "misonet_strerror": (C.c_char_p, [C.c_int]),
    "misonet_last_error": (C.c_char_p, []),
    "misonet_version": (C.c_int, []),
    "misonet_net_create": (C.c_int, [C.POINTER(Cfg), C.POINTER(C.c_void_p)]),
    "misonet_net_destroy": (C.c_int, [C.c_void_p]),
    "misonet_net_num_tensors": (C.c_int, [C.c_void_p]),
    "misonet_net_tensor_name": (C.c_char_p, [C.c_void_p, C.c_int]),
    "misonet_net_tensor_numel": (C.c_longlong, [C.c_void_p, C.c_int]),
    "misonet_net_set_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_longlong]),
    "misonet_net_commit": (C.c_int, [C.c_void_p]),
    "misonet_net_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "misonet_net_get_precision": (C.c_int, [C.c_void_p]),
    "misonet_net_keep_activations": (C.c_int, [C.c_void_p, C.c_int]),
    "misonet_net_buffer_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "misonet_net_conv_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "misonet_net_workspace_bytes": (C.c_longlong, [C.c_void_p, C.c_int, C.c_int]),
    "misonet_net_forward": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_net_check": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_net_tap_shape": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "misonet_net_tap": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "misonet_mvdr_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "misonet_mvdr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                               C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_mvdr_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_bf_opts_default": (C.c_int, [C.POINTER(BfOpts)]),
    "misonet_beamform_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.POINTER(BfOpts)]),
    "misonet_beamform": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(BfOpts), C.c_void_p,
                                   C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_beamform_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(BfOpts), C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "misonet_pipeline_set_beamformer": (C.c_int, [C.c_void_p, C.POINTER(BfOpts)]),
    "misonet_wpe_opts_default": (C.c_int, [C.POINTER(WpeOpts)]),
    "misonet_wpe_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WpeOpts)]),
    "misonet_wpe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WpeOpts), C.c_void_p,
                              C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_wpe_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(WpeOpts), C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "misonet_owpe_opts_default": (C.c_int, [C.POINTER(OwpeOpts)]),
    "misonet_owpe_state_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.POINTER(OwpeOpts)]),
    "misonet_owpe_lds_bytes": (C.c_int, [C.c_int, C.POINTER(OwpeOpts)]),
    "misonet_owpe_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(OwpeOpts), C.c_void_p]),
    "misonet_owpe": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OwpeOpts), C.c_void_p, C.c_void_p,
                               C.c_longlong, C.c_void_p]),
    "misonet_owpe_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(OwpeOpts), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_wpd_opts_default": (C.c_int, [C.POINTER(WpdOpts)]),
    "misonet_wpd_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.POINTER(WpdOpts)]),
    "misonet_wpd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WpdOpts), C.c_void_p,
                              C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_wpd_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(WpdOpts), C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "misonet_pipeline_set_wpd": (C.c_int, [C.c_void_p, C.POINTER(WpdOpts)]),
    "misonet_cacgmm_opts_default": (C.c_int, [C.POINTER(CacgmmOpts)]),
    "misonet_cacgmm_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "misonet_cacgmm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CacgmmOpts),
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_cacgmm_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "misonet_masks_from_estimates": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p]),
    "misonet_pipeline_set_refine": (C.c_int, [C.c_void_p, C.POINTER(CacgmmOpts)]),
    "misonet_jbf_opts_default": (C.c_int, [C.POINTER(JbfOpts)]),
    "misonet_beamform_joint_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(JbfOpts)]),
    "misonet_beamform_joint": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(JbfOpts),
                                         C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_beamform_joint_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(JbfOpts), C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_pipeline_set_joint": (C.c_int, [C.c_void_p, C.POINTER(JbfOpts)]),
    "misonet_iva_opts_default": (C.c_int, [C.POINTER(IvaOpts)]),
    "misonet_auxiva_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "misonet_auxiva_resident_frames": (C.c_int, [C.c_int]),
    "misonet_auxiva": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(IvaOpts), C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_auxiva_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_oiva_opts_default": (C.c_int, [C.POINTER(OivaOpts)]),
    "misonet_oiva_state_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "misonet_oiva_bins_per_pass": (C.c_int, [C.c_int]),
    "misonet_oiva_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(OivaOpts), C.c_void_p]),
    "misonet_oiva": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OivaOpts), C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_oiva_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "misonet_overiva_state_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "misonet_overiva_bins_per_pass": (C.c_int, [C.c_int, C.c_int]),
    "misonet_overiva_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OivaOpts), C.c_void_p]),
    "misonet_overiva": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OivaOpts), C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_overiva_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_obf_opts_default": (C.c_int, [C.POINTER(ObfOpts)]),
    "misonet_obf_state_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "misonet_obf_cells_per_block": (C.c_int, [C.c_int]),
    "misonet_obf_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ObfOpts), C.c_void_p]),
    "misonet_obf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ObfOpts), C.c_void_p,
                              C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_obf_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "misonet_pit_scratch_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "misonet_pit_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_longlong, C.c_void_p]),
    "misonet_css_scratch_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "misonet_css_align": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_css_stitch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_score_scratch_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_longlong]),
    "misonet_score_wave": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong,
                                     C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_score_spec": (C.c_int, [C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong,
                                     C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_bss_scratch_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int]),
    "misonet_bss_corr": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong,
                                   C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_bss_solve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_stoi_resampled_len": (C.c_longlong, [C.c_longlong, C.c_int]),
    "misonet_stoi_taps": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "misonet_stoi_scratch_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_longlong]),
    "misonet_stoi_resample": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p,
                                        C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong, C.c_longlong,
                                        C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "misonet_stoi_measure": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_resample_ratio": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "misonet_resampled_len": (C.c_longlong, [C.c_longlong, C.c_int, C.c_int]),
    "misonet_resample_taps": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int]),
    "misonet_resample_tile": (C.c_int, []),
    "misonet_resample": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_longlong,
                                   C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong,
                                   C.c_void_p]),
    "misonet_resample_stream_carry": (C.c_longlong, [C.c_longlong, C.c_longlong]),
    "misonet_resample_stream_state_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_longlong, C.c_longlong]),
    "misonet_resample_stream_outputs": (C.c_longlong, [C.c_longlong, C.c_longlong, C.c_int, C.c_longlong, C.c_longlong]),
    "misonet_resample_stream_tile": (C.c_int, []),
    "misonet_resample_stream_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p]),
    "misonet_resample_stream": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_int,
                                          C.c_longlong, C.c_longlong, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p, C.c_int,
                                          C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_room_tile": (C.c_int, []),
    "misonet_room_rir_len": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "misonet_room_mix_len": (C.c_longlong, [C.c_longlong, C.c_int]),
    "misonet_room_rir": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                   C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_room_mix": (C.c_int, [C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                   C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_doa_opts_default": (C.c_int, [C.POINTER(DoaOpts)]),
    "misonet_doa_tile": (C.c_int, []),
    "misonet_doa_bin_chunk": (C.c_int, []),
    "misonet_doa_blocks": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "misonet_doa_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DoaOpts)]),
    "misonet_doa": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_int, C.c_int, C.c_double, C.POINTER(DoaOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_doa_debug": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DoaOpts),
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_reverb_frames": (C.c_longlong, [C.c_longlong, C.c_int]),
    "misonet_reverb_scratch_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int]),
    "misonet_reverb_measure": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p,
                                         C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong, C.c_longlong,
                                         C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_srmr_frames": (C.c_longlong, [C.c_longlong, C.c_int]),
    "misonet_srmr_scratch_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_longlong, C.c_int]),
    "misonet_srmr_chunk": (C.c_int, []),
    "misonet_srmr_measure": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong,
                                       C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_pipeline_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                          C.POINTER(C.c_void_p)]),
    "misonet_pipeline_destroy": (C.c_int, [C.c_void_p]),
    "misonet_pipeline_workspace_bytes": (C.c_longlong, [C.c_void_p, C.c_int, C.c_int]),
    "misonet_pipeline_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_pipeline_run_wav": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_stft_frames": (C.c_int, [C.c_int]),
    "misonet_stft_workspace_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "misonet_stft": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_frontend_init": (C.c_int, []),
    "misonet_istft": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_stft_stream_state_bytes": (C.c_longlong, [C.c_int, C.c_int]),
    "misonet_stft_stream_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "misonet_stft_stream_frames": (C.c_longlong, [C.c_longlong, C.c_longlong, C.c_int]),
    "misonet_stft_stream": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_longlong, C.c_void_p]),
    "misonet_istft_stream_state_bytes": (C.c_longlong, [C.c_int]),
    "misonet_istft_stream_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "misonet_istft_stream_hops": (C.c_longlong, [C.c_longlong, C.c_longlong, C.c_int]),
    "misonet_istft_stream": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_longlong, C.c_void_p]),
    "misonet_pipeline_check": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "misonet_profile_begin": (C.c_int, [C.c_int]),
    "misonet_profile_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "misonet_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "misonet_event_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "misonet_event_elapsed_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "misonet_event_destroy": (C.c_int, [C.c_void_p]),
}

_lib = None


def lib():
    """The loaded library; raises ImportError (loudly) when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build the HIP extension first (make -C misonet_amd/csrc). "
                              "misonet_amd has no CPU fallback.")
        # torch first: it ships its own libamdhip64; loading this library BEFORE torch makes the process hold two HIP runtimes
        # (ours resolved against /opt/rocm), and the second one to initialise sees "no ROCm-capable device" (found by running
        # __graft_entry__.build() and smoke() in one process)
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code):
    if code != OK:
        L = lib()
        detail = L.misonet_last_error().decode() or L.misonet_strerror(code).decode()
        if code == ENAN:
            raise FloatingPointError(f"libmisonet_hip: {detail}")
        raise MisonetError(code, detail)


def stream_ptr(device=None):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
