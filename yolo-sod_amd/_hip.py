"""ctypes binding of the C ABI in ``include/yolosod_hip.h`` (``lib/libyolosod_hip.so``).

PyTorch is only plumbing here: it owns device memory (caching allocator) and the current HIP stream. Every
wrapper checks device / dtype / contiguity / shapes on the host before launching (a kernel never sees a shape it
was not written for) and raises ``RuntimeError`` with the library's message on failure. There is no CPU
fallback: calling an op on a CPU tensor, or without the built library, raises.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import torch

from .utils.metrics import IOU_THRESHOLDS

LIB_PATH = Path(__file__).resolve().parent / "lib" / "libyolosod_hip.so"

_c_float_p = ctypes.c_void_p
_vp = ctypes.c_void_p
_i = ctypes.c_int
_l = ctypes.c_long
_f = ctypes.c_float
_d = ctypes.c_double
_sz = ctypes.c_size_t

# name -> (restype, argtypes)
SIGNATURES = {
    "yolosod_abi_version": (_i, []),
    "yolosod_last_error": (ctypes.c_char_p, []),
    "yolosod_se_workspace": (_sz, [_i, _i, _i, _i]),
    "yolosod_se_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "yolosod_cbam_workspace": (_sz, [_i, _i, _i, _i]),
    "yolosod_cbam_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "yolosod_ca_workspace": (_sz, [_i, _i, _i, _i]),
    "yolosod_ca_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp,
                                _vp, _vp, _sz, _vp]),
    "yolosod_a2_workspace": (_sz, [_i, _i, _i, _i, _i]),
    "yolosod_a2_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _sz, _vp]),
    "yolosod_swin_workspace": (_sz, [_i, _i, _i, _i, _i, _i]),
    "yolosod_swin_workspace_v2": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "yolosod_swin_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _sz, _vp]),
    "yolosod_detect_decode": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "yolosod_detect_head": (_i, [_i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "yolosod_nms_workspace": (_sz, [_i, _i, _i, _i]),
    "yolosod_nms_workspace_v2": (_sz, [_i, _i, _i, _i, _i]),
    "yolosod_nms": (_i, [_vp, _i, _i, _i, _f, _d, _vp, _i, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yolosod_nms_merged": (_i, [_vp, _i, _i, _i, _f, _d, _vp, _i, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _sz,
                                _vp]),
    "yolosod_gemm_f32": (_i, [_vp, _l, _i, _vp, _l, _i, _i, _vp, _l, _i, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "yolosod_layernorm": (_i, [_vp, _vp, _l, _i, _vp, _vp, _f, _vp]),
    "yolosod_attention": (_i, [_vp, _vp, _l, _i, _i, _i, _vp]),
    "yolosod_bias_act": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _i, _i, _l, _i, _vp]),
    "yolosod_upsample2x": (_i, [_vp, _vp, _l, _i, _i, _i, _i, _i, _vp]),
    "yolosod_letterbox_ingest": (_i, [_vp, _i, _vp, _l, _i, _i, _i, _i, _vp]),
    "yolosod_letterbox_ingest_nv12": (_i, [_vp, _i, _vp, _l, _i, _i, _i, _i, _vp]),
    "yolosod_scale_boxes": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "yolosod_tile_merge": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _f, _vp]),
    "yolosod_tile_merge_tta": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _f, _i, _f, _f, _f, _vp]),
    "yolosod_match_predictions": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "yolosod_confusion_matrix": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _f, _f, _vp, _vp]),
    "yolosod_track_state_bytes": (_sz, [_i]),
    "yolosod_track_workspace": (_sz, [_i, _i, _i]),
    "yolosod_track_reset": (_i, [_vp, _i, _i, _vp, _i, _vp]),
    "yolosod_track_update": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yolosod_track_update_ex": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yolosod_debug_track_last": (_i, [_i]),
    "yolosod_tta_views": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "yolosod_tta_merge": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _i, _f, _i, _f, _f, _vp]),
    "yolosod_stem_workspace": (_sz, [_i, _i, _i, _i]),
    "yolosod_stem_conv": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _l, _vp, _vp, _sz, _vp]),
    "yolosod_conv1x1_thin_stats": (_i, [_vp, _l, _vp, _vp, _vp, _l, _i, _i, _i, _l, _i, _vp, _vp, _vp, _vp]),
    "yolosod_conv1x1_thin": (_i, [_vp, _l, _vp, _vp, _vp, _l, _vp, _l, _vp, _l, _i, _i, _i, _i, _l, _vp]),
    "yolosod_bias_act_dual": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _vp, _l, _i, _i, _i, _l, _i, _vp]),
    "yolosod_bias_act_capool": (_i, [_vp, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp, ctypes.c_long, _i, _i, _i, _i,
                                     _i, _vp, _vp]),
    "yolosod_ca_forward_pre": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp,
                                    _vp, _vp, ctypes.c_size_t, _vp]),
    "yolosod_bias_act_stats": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _i, _i, _l, _i, _i, _l, _vp, _vp, _vp]),
    "yolosod_plane_parts": (_i, [_l, ctypes.POINTER(ctypes.c_long)]),
    "yolosod_se_forward_pre": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "yolosod_cbam_forward_pre": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yolosod_conv1x1": (_i, [_vp, _l, _vp, _vp, _vp, _l, _vp, _l, _i, _i, _i, _l, _i, _vp]),
    "yolosod_conv3x3_prep_bytes": (_sz, [_i]),
    "yolosod_conv3x3_prepare": (_i, [_vp, _i, _vp, _sz, _vp]),
    "yolosod_conv3x3_silu": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "yolosod_conv1x1x2_prep_bytes": (_sz, [_i, _i]),
    "yolosod_conv1x1x2_prepare": (_i, [_vp, _i, _i, _vp, _sz, _vp]),
    "yolosod_conv1x1x2_silu": (_i, [_vp, _l, _vp, _l, _vp, _l, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "yolosod_conv1x1x2_silu_cat": (_i, [_vp, _l, _vp, _l, _i, _vp, _l, _vp, _l, _i, _i, _i, _i, _i, _vp, _vp, _sz,
                                        _i, _vp]),
    "yolosod_conv1x1x2_silu_stats": (_i, [_vp, _l, _vp, _l, _i, _i, _i, _i, _vp, _vp, _sz, _i, _i, _vp, _vp, _vp, _vp]),
    "yolosod_sppf_pool": (_i, [_vp, _l, _i, _i, _i, _i, _vp]),
    "yolosod_conv1x1_thin_cat": (_i, [_vp, _l, _vp, _l, _i, _vp, _vp, _vp, _l, _vp, _l, _i, _i, _i, _i, _l, _i, _vp]),
    "yolosod_conv3x3_prep_bytes_ex": (_sz, [_i, _i]),
    "yolosod_conv3x3_prepare_ex": (_i, [_vp, _i, _i, _vp, _sz, _vp]),
    "yolosod_conv3x3_silu_ex": (_i, [_vp, _vp, _l, _vp, _l, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "yolosod_conv3x3_silu_xs": (_i, [_vp, _l, _vp, _l, _vp, _l, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "yolosod_debug_set_swin_fused": (None, [_i]),
    "yolosod_debug_set_swin_x3": (_i, [_i]),
    "yolosod_debug_swin_route": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "yolosod_debug_swin_last_route": (_i, []),
    "yolosod_debug_set_head_x2": (_i, [_i]),
    "yolosod_debug_set_a2_x2": (_i, [_i]),
    "yolosod_debug_set_gemm_x2": (None, [_i]),
    "yolosod_debug_split_f16": (_i, [_vp, _vp, _vp, _l, _vp]),
    "yolosod_swin_prep_bytes": (_sz, [_i, _i, _i]),
    "yolosod_split_range_flag": (_i, [_i, _vp]),
    "yolosod_swin_prepare": (_i, [_i, _i, _i] + [_vp] * 15 + [_f, _vp, _sz, _vp]),
    "yolosod_swin_forward_prepared": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _f, _vp, _f, _i, _vp, _vp, _sz,
                                           _vp, _sz, _vp]),
    "yolosod_swin_prepared_workspace": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "yolosod_a2_prep_bytes": (_sz, [_i, _i, _i, _i]),
    "yolosod_a2_prepare": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yolosod_a2_forward_prepared": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp,
                                         _vp, _vp, _sz, _vp, _sz, _vp]),
    "yolosod_init": (_i, [_i]),
    "yolosod_debug_set_a2_fused": (_i, [_i]),
    "yolosod_debug_set_a2_pool_wide": (_i, [_i]),
    "yolosod_debug_set_conv3x3_form": (_i, [_i]),
    "yolosod_debug_conv3x3_form": (_i, [_i, _i, _i, _i]),
    "yolosod_debug_conv3x3_form_ex": (_i, [_i, _i, _i, _i, _i]),
    "yolosod_bottleneck3x3_silu_xs": (_i, [_vp, _l, _vp, _l, _vp, _l, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "yolosod_conv3x3_head_xs": (_i, [_vp, _l, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _i, _i, _f, _vp, _i, _i, _vp]),
    "yolosod_detect_head_prep_bytes": (_sz, [_i]),
    "yolosod_detect_head_prepare": (_i, [_vp, _i, _vp, _sz, _vp]),
    "yolosod_debug_conv3x3_head_fused": (_i, [_i, _i, _i]),
    "yolosod_debug_set_conv3x3_head_fuse": (_i, [_i]),
    "yolosod_debug_bottleneck3x3_fused": (_i, [_i, _i, _i]),
    "yolosod_debug_set_bottleneck3x3_fuse": (_i, [_i]),
    "yolosod_debug_set_conv1x1x2_form": (_i, [_i]),
    "yolosod_debug_conv1x1x2_form": (_i, [_i, _i, _i, _i]),
    "yolosod_debug_set_conv3x3s2_form": (_i, [_i]),
    "yolosod_debug_conv3x3s2_form": (_i, [_i, _i, _i, _i]),
    "yolosod_se_gate": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "yolosod_cbam_gates": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yolosod_conv3x3s2_prep_bytes": (_sz, [_i, _i]),
    "yolosod_conv3x3s2_prepare": (_i, [_vp, _i, _i, _vp, _sz, _vp]),
    "yolosod_conv3x3s2_silu": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yolosod_conv3x3s2_silu_out": (_i, [_vp, _vp, _l, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yolosod_debug_set_swin_tokln": (_i, [_i]),
    "yolosod_debug_set_a2_pool_px": (_i, [_i]),
    "yolosod_mamba_glu_workspace": (_sz, [_i, _i, _i, _i, _i, _i]),
    "yolosod_mamba_glu_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _sz, _vp]),
    # bf16 storage (the bf16 model config): activations / GEMM weights bf16, other parameters fp32
    "yolosod_se_forward_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "yolosod_cbam_forward_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "yolosod_ca_forward_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _sz, _vp]),
    "yolosod_bias_act_bf16": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _vp, _l, _i, _i, _i, _l, _i, _vp]),
    "yolosod_bias_act_stats_bf16": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _i, _i, _l, _i, _i, _l, _vp, _vp, _vp]),
    "yolosod_bias_act_capool_bf16": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _i, _i, _i, _i, _i, _vp, _vp]),
    "yolosod_swin_workspace_bf16": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "yolosod_swin_forward_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _sz, _vp]),
    "yolosod_a2_workspace_bf16": (_sz, [_i, _i, _i, _i, _i]),
    "yolosod_a2_forward_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp,
                                     _vp, _sz, _vp]),
    "yolosod_detect_head_bf16": (_i, [_i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp,
                                      _vp]),
    "yolosod_detect_head_levels": (_i, [_i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i,
                                        _i, _vp, _i, _vp]),
    "yolosod_gemm_bf16": (_i, [_vp, _l, _i, _vp, _l, _i, _i, _vp, _l, _i, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "yolosod_attention_bf16": (_i, [_vp, _vp, _l, _i, _i, _i, _vp]),
    "yolosod_debug_gemm_bf16_tile": (_i, [_i, _i, _i]),
    "yolosod_debug_gemm_bf16_last_tile": (_i, []),
    "yolosod_debug_gemm_bf16_launches": (_l, [_i]),
    "yolosod_debug_swin_bf16_route": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "yolosod_debug_swin_bf16_last_route": (_i, []),
    "yolosod_debug_attention_bf16_form": (_i, [_i, _i, _i]),
    "yolosod_debug_attention_bf16_last_form": (_i, []),
}

_LIB = None


def load_library() -> ctypes.CDLL:
    """Load (once) the in-tree HIP library; raises if it has not been built."""
    global _LIB
    if _LIB is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"yolosod_amd: HIP library {LIB_PATH} is missing - run __graft_entry__.build() "
                "(or python yolo-sod_amd/build.py). There is no CPU fallback.")
        path = os.environ.get("YOLOSOD_LIB_AB") or str(LIB_PATH)  # diagnostic A/B builds only
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            if path != str(LIB_PATH) and name.startswith("yolosod_debug_") and not hasattr(lib, name):
                continue  # an older A/B build may predate a test hook
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


OPS_LIB_PATH = LIB_PATH.parent / "yolosod_torch_ops.so"
_OPS = None


def ops():
    """torch.ops.yolosod (csrc/torch_ops.cpp over the C ABI): the op-registered form every hot-path wrapper below
    dispatches through (TORCH_CHECK errors, outputs and workspaces from the caching allocator on the current
    stream, Meta kernels for shape propagation). Raises if the extension has not been built - no fallback."""
    global _OPS
    if _OPS is None:
        load_library()  # the ops library links it (RUNPATH $ORIGIN); loaded first so both share one handle
        if not OPS_LIB_PATH.exists():
            raise RuntimeError(f"yolosod_amd: torch-op library {OPS_LIB_PATH} is missing - run "
                               "__graft_entry__.build() (or python yolo-sod_amd/build.py). There is no CPU fallback.")
        if not hasattr(torch.ops.yolosod, "se_fwd"):
            torch.ops.load_library(str(OPS_LIB_PATH))
        _OPS = torch.ops.yolosod
    return _OPS


class _OpTimer:
    """Records HIP events around every C-ABI launch sequence (on the launch stream) while active; with ``select``,
    only around the launches whose key it accepts (an event pair is a timestamped barrier on the stream: timing every
    launch of a step costs the step a few per cent)."""

    def __init__(self, select=None):
        self.records = []
        self.select = select

    def durations_ms(self):
        torch.cuda.synchronize()
        out = []
        for key, e0, e1 in self.records:
            out.append((key, e0.elapsed_time(e1)))
        return out


_TIMER: _OpTimer | None = None


class op_timer:
    """``with op_timer() as t: ...`` -> ``t.durations_ms()`` = [((op, shape, extra), ms), ...] per launch;
    ``op_timer(select)``: only the launches whose key ``select(key)`` accepts are timed."""

    def __init__(self, select=None):
        self.select = select

    def __enter__(self):
        global _TIMER
        self.t = _OpTimer(self.select)
        _TIMER = self.t
        return self.t

    def __exit__(self, *exc):
        global _TIMER
        _TIMER = None
        return False


_INIT_DEVS = set()


def _init_device(dev) -> None:
    """yolosod_init once per device: the library's device state (the split-range flag word) is allocated and zeroed
    before the first launch there, never lazily inside a stream capture."""
    idx = torch.device(dev).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _INIT_DEVS:
        _check(load_library().yolosod_init(int(idx)), "init")
        _INIT_DEVS.add(idx)


def _launch(key, dev, fn, *args):
    """Run one C-ABI launch sequence with ``dev`` (the operands' device) as the current HIP device; the stream
    argument inside ``args`` is that device's current stream (``_stream(dev)``). While an :class:`op_timer` is
    active, HIP events bracket the sequence on that stream."""
    _init_device(dev)
    with torch.cuda.device(dev):
        t = _TIMER
        if t is None or (t.select is not None and not t.select(key)):
            return fn(*args)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        t.records.append((key, e0, e1))
        return rc


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_library().yolosod_last_error().decode(errors="replace")
        raise RuntimeError(f"yolosod_amd.{what} failed (rc={rc}): {msg}")


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> int:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: HIP kernel requires a GPU tensor (got device {t.device}); no CPU fallback")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    return t.data_ptr()


def _p(t: torch.Tensor, name: str, numel: int | None = None, dtype=torch.float32) -> int:
    """Pointer of a (parameter) tensor after checking its element count (and, via ``_dev``, that it is a
    contiguous GPU tensor of ``dtype``: this only validates - callers pass prepared parameters, e.g. the modules'
    cached fp32 / bf16 copies)."""
    if numel is not None and t.numel() != numel:
        raise RuntimeError(f"{name}: expected {numel} elements, got {t.numel()}")
    return _dev(t, name, dtype)


_BF16 = torch.bfloat16


def _act_dtype(x: torch.Tensor) -> bool:
    """True for bf16 activations (the bf16 model config), False for fp32; anything else raises."""
    if x.dtype == torch.float32:
        return False
    if x.dtype == _BF16:
        return True
    raise RuntimeError(f"yolosod_amd: activations must be float32 or bfloat16, got {x.dtype}")


def _stream(dev) -> int:
    """The current stream of ``dev`` (the operands' device, not the current device: ADVICE r1)."""
    return torch.cuda.current_stream(dev).cuda_stream


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


# ---------------------------------------------------------------------------------------------------------------
# operator wrappers (parameters are passed as tensors already on the input's device)
# ---------------------------------------------------------------------------------------------------------------
class PlaneStats:
    """Per-plane partial sums (+ maxes) of a tensor, emitted by its producer's epilogue (bias_act(stats=...)) in
    the segmentation yolosod_plane_parts gives for its H*W; SE / CBAM consume them instead of re-reading it."""

    __slots__ = ("psum", "pmax", "parts", "shape")

    def __init__(self, psum, pmax, parts, shape):
        self.psum, self.pmax, self.parts, self.shape = psum, pmax, parts, tuple(shape)


_PARTS = {}


def plane_parts(HW: int):
    """(parts, seg) of the channel-attention statistics plan for planes of HW floats."""
    if HW not in _PARTS:
        seg = ctypes.c_long(0)
        parts = load_library().yolosod_plane_parts(int(HW), ctypes.byref(seg))
        _PARTS[HW] = (int(parts), int(seg.value))
    return _PARTS[HW]


def _pre_stats(x, need_max):
    st = getattr(x, "_ys_plane_stats", None)
    if st is None or st.shape != tuple(x.shape) or (need_max and st.pmax is None):
        return None
    return st


def _t(t, name):
    """A GPU tensor argument (device / dtype / shape checks are the op's TORCH_CHECKs)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: HIP kernel requires a GPU tensor (got device {t.device}); no CPU fallback")
    return t


def se_forward(x, fc1_w, fc1_b, fc2_w, fc2_b):
    """SE on fp32 or bf16 activations (parameters fp32) -> torch.ops.yolosod.se_fwd."""
    bf = _act_dtype(_t(x, "x"))
    hid = fc1_w.shape[0]
    pre = _pre_stats(x, False)  # plane sums that came with x from its producer's epilogue
    return _launch(("se", tuple(x.shape), hid) + ((2,) if bf else ()), x.device, ops().se_fwd, x, fc1_w, fc1_b,
                   fc2_w, fc2_b, None if pre is None else pre.psum)


def cbam_forward(x, fc0_w, fc2_w, sa_w):
    """CBAM on fp32 or bf16 activations (parameters fp32) -> torch.ops.yolosod.cbam_fwd."""
    bf = _act_dtype(_t(x, "x"))
    hid = fc0_w.shape[0]
    pre = _pre_stats(x, True)
    return _launch(("cbam", tuple(x.shape), hid) + ((2,) if bf else ()), x.device, ops().cbam_fwd, x, fc0_w, fc2_w,
                   sa_w, None if pre is None else pre.psum, None if pre is None else pre.pmax)


def se_gate(x, fc1_w, fc1_b, fc2_w, fc2_b):
    """The SE gate only (yolosod_se_gate): [B, C] fp32, for a consumer that applies x * gate itself (the fused
    stride-2 conv, conv3x3s2_silu). fp32 activations; x's producer statistics are used when they came with it."""
    lib = load_library()
    B, C, H, W = x.shape
    hid = int(fc1_w.shape[0])
    pre = _pre_stats(x, False)
    gate = torch.empty((B, C), dtype=torch.float32, device=x.device)
    ws = torch.empty(int(lib.yolosod_se_workspace(B, C, H, W)), dtype=torch.uint8, device=x.device)
    _check(_launch(("se_gate", tuple(x.shape), hid), x.device, lib.yolosod_se_gate, _dev(x, "x"), B, C, H, W,
                   _dev(fc1_w, "fc1_w"), _dev(fc1_b, "fc1_b"), _dev(fc2_w, "fc2_w"), _dev(fc2_b, "fc2_b"), hid,
                   None if pre is None else _dev(pre.psum, "psum"), gate.data_ptr(), ws.data_ptr(), ws.numel(),
                   _stream(x.device)), "se_gate")
    return gate


def cbam_gates(x, fc0_w, fc2_w, sa_w):
    """The CBAM gates only (yolosod_cbam_gates): (ca [B, C], sa [B, H, W]) fp32, for a consumer that applies
    (x * ca) * sa itself (conv3x3s2_silu). fp32 activations; x's producer statistics are used when they came with it."""
    lib = load_library()
    B, C, H, W = x.shape
    hid = int(fc0_w.shape[0])
    pre = _pre_stats(x, True)
    ca = torch.empty((B, C), dtype=torch.float32, device=x.device)
    sa = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    ws = torch.empty(int(lib.yolosod_cbam_workspace(B, C, H, W)), dtype=torch.uint8, device=x.device)
    _check(_launch(("cbam_gate", tuple(x.shape), hid), x.device, lib.yolosod_cbam_gates, _dev(x, "x"), B, C, H, W,
                   _dev(fc0_w, "fc0_w"), _dev(fc2_w, "fc2_w"), hid, _dev(sa_w, "sa_w"),
                   None if pre is None else _dev(pre.psum, "psum"), None if pre is None else _dev(pre.pmax, "pmax"),
                   ca.data_ptr(), sa.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x.device)), "cbam_gates")
    return ca, sa


def ca_forward(x, conv1_w, conv1_b, bn_w, bn_b, bn_mean, bn_var, bn_eps, convh_w, convh_b, convw_w, convw_b):
    """CA on fp32 or bf16 activations (parameters fp32) -> torch.ops.yolosod.ca_fwd."""
    bf = _act_dtype(_t(x, "x"))
    mip = conv1_w.shape[0]
    pre = getattr(x, "_ys_ca_pool", None)  # row / column means that came with x from its producer
    yin = pre[0] if pre is not None and pre[1] == tuple(x.shape) else None
    return _launch(("ca", tuple(x.shape), mip) + ((2,) if bf else ()), x.device, ops().ca_fwd, x, conv1_w, conv1_b,
                   bn_w, bn_b, bn_mean, bn_var, float(bn_eps), convh_w, convh_b, convw_w, convw_b, yin)


def a2_prep_bytes(C, num_heads, num_areas, W) -> int:
    """Size of the fused LN / QKV / attention kernel's prepared block (0: the shape does not take that kernel)."""
    return int(load_library().yolosod_a2_prep_bytes(int(C), int(num_heads), int(num_areas), int(W)))


def a2_prepare(x, num_areas, num_heads, proj_w, ln_w, ln_b, in_w, in_b):
    """The prepared block (proj and in_proj fp16 planes, uint8 tensor on x's device) for a2_forward(..., prep=...)."""
    return ops().a2_prep(x, int(num_areas), int(num_heads), proj_w, ln_w, ln_b, in_w, in_b)


def a2_forward(x, num_areas, num_heads, proj_w, proj_b, ln_w, ln_b, ln_eps, in_w, in_b, mo_w, mo_b, op_w, op_b,
               prep=None):
    """A2_Attn -> torch.ops.yolosod.a2_fwd. mo_w = mo_b = None: op_w / op_b are the pre-multiplied MHA-out x
    output-conv weights (A2_Attn._fused_out). bf16 activations: proj_w / in_w / op_w bf16 (pre-multiplied form
    only), biases and LN fp32. ``prep``: a callable returning the cached prepared block (a2_prepare) - used when the
    shape takes the fused LN / QKV / attention kernel (fp32)."""
    bf = _act_dtype(_t(x, "x"))
    B, C, H, W = x.shape
    if num_areas * W > 320:
        raise RuntimeError(f"A2_Attn: sequence length {num_areas * W} > 320 unsupported")
    if bf and (C // num_heads not in (32, 64, 128) or C % 64):
        raise RuntimeError(f"A2_Attn (bf16): C={C} with head dim {C // num_heads} unsupported")
    use_prep = prep is not None and not bf and mo_w is None and a2_prep_bytes(C, num_heads, num_areas, W) > 0

    def run():
        # the preparation (a launch on first use of a parameter version) runs inside _launch: after the device's
        # yolosod_init, under its device guard, and timed as part of this operator
        return ops().a2_fwd(x, int(num_areas), int(num_heads), proj_w, proj_b, ln_w, ln_b, float(ln_eps), in_w, in_b,
                            mo_w, mo_b, op_w, op_b, prep() if use_prep else None)

    return _launch(("a2", tuple(x.shape), (num_areas, num_heads)) + ((2,) if bf else ()), x.device, run)


def swin_forward(x, num_heads, window, dw_w, ln1_w, ln1_b, ln1_eps, in_w, in_b, out_w, out_b, ln2_w, ln2_b,
                 ln2_eps, m1_w, m1_b, m2_w, m2_b, pw_w, bn_w, bn_b, bn_mean, bn_var, bn_eps, prep=None):
    """SwinBlock -> torch.ops.yolosod.swin_fwd on fp32 or bf16 activations. bf16: the projection / MLP / pw weights
    (in_w, out_w, m1_w, m2_w, pw_w) are bf16, every other parameter fp32. ``prep``: a callable returning the cached
    prepared-parameter block (swin_prepare) - used when the shape takes the fp16-split kernels
    (torch.ops.yolosod.swin_fwd_prepared: the weight split is not redone per call)."""
    bf = _act_dtype(_t(x, "x"))
    B, C, H, W = x.shape
    hid = m1_w.shape[0]
    wh = H if (H <= window and W <= window) else min(window, H)
    ww = W if (H <= window and W <= window) else min(window, W)
    if wh * ww > 320:
        raise RuntimeError(f"SwinBlock: window of {wh}x{ww} tokens unsupported")
    if C % num_heads or (C // num_heads) not in ((32, 64, 128) if bf else (8, 16, 32, 64, 128)):
        raise RuntimeError(f"SwinBlock: head dim {C}/{num_heads} unsupported")
    key = ("swin", tuple(x.shape), (num_heads, window, hid)) + ((2,) if bf else ())
    if (prep is not None and not bf and wh == 7 and ww == 7 and C * H * W < (1 << 30)
            and swin_prep_bytes(C, num_heads, hid) > 0):
        # the weight split / folds were made once (``prep`` = swin_prepare of these parameters): one kernel launch;
        # prep() runs inside _launch (device initialised, timed with the operator), as in a2_forward
        return _launch(key, x.device, lambda: ops().swin_fwd_prepared(x, prep(), int(num_heads), int(window), dw_w,
                                                                      float(ln1_eps), out_b, float(ln2_eps), int(hid),
                                                                      m2_b))
    return _launch(key, x.device, ops().swin_fwd, x, int(num_heads), int(window), dw_w, ln1_w, ln1_b, float(ln1_eps),
                   in_w, in_b, out_w, out_b, ln2_w, ln2_b, float(ln2_eps), m1_w, m1_b, m2_w, m2_b, pw_w, bn_w, bn_b,
                   bn_mean, bn_var, float(bn_eps))


def split_range_flag(reset: bool = True, device=None) -> bool:
    """True if a fp16-split kernel on ``device`` (default: current) saw an operand beyond fp16's range since the last
    reset (the C-ABI's split-range guard); synchronises the device's current stream."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        rc = load_library().yolosod_split_range_flag(int(bool(reset)), _stream(dev))
    if rc < 0:
        _check(rc, "split_range_flag")
    return rc == 1


_split_convs_off = 0  # > 0 inside exact_fp32_matrix(): the fp16-split convolution kernels are bypassed


def split_convs_enabled() -> bool:
    """Whether the executor may route convolutions to the fp16-split conv kernels (conv3x3 / conv3x3s2 / conv1x1x2:
    Detect towers, the gate-fused SE / CBAM consumers, the neck); false inside exact_fp32_matrix(), where they run on
    MIOpen (+ the exact-fp32 epilogue / thin 1x1 kernels) instead."""
    return _split_convs_off == 0


class exact_fp32_matrix:
    """``with exact_fp32_matrix(): ...`` runs the fp32 model's matrix products on the exact fp32 MFMA kernels
    (Swin swin_fused / swin_wide, Detect head LDS kernel, A2 fp32 GEMMs) instead of the fp16 two-term splits, and its
    convolutions on MIOpen instead of the fp16-split conv kernels (split_convs_enabled) - the fallback when
    split_range_flag() reports an operand outside fp16's range."""

    _SWITCHES = ("yolosod_debug_set_swin_x3", "yolosod_debug_set_head_x2", "yolosod_debug_set_a2_x2")

    def __enter__(self):
        global _split_convs_off
        lib = load_library()
        # each switch returns its previous state, restored on exit (a user's YOLOSOD_*=0 or an outer setting stays)
        self._prev = [int(getattr(lib, f)(0)) for f in self._SWITCHES]
        _split_convs_off += 1
        return self

    def __exit__(self, *exc):
        global _split_convs_off
        lib = load_library()
        for f, v in zip(self._SWITCHES, self._prev):
            getattr(lib, f)(v)
        _split_convs_off -= 1
        return False


SWIN_ROUTES = ("decomposed", "split_fused", "exact_fused", "exact_wide")


def swin_route(B, C, num_heads, H, W, window, hid) -> str:
    """The route SwinBlock takes for this shape under the current switches (yolosod_debug_swin_route, host only): one
    of SWIN_ROUTES."""
    r = int(load_library().yolosod_debug_swin_route(int(B), int(C), int(num_heads), int(H), int(W), int(window),
                                                    int(hid)))
    if r < 0:
        raise RuntimeError(f"SwinBlock: shape {B}x{C}x{H}x{W} heads {num_heads} window {window} hidden {hid} unsupported")
    return SWIN_ROUTES[r]


def swin_last_route():
    """The route the last fp32 SwinBlock launch of this process took (yolosod_debug_swin_last_route; None: none yet)."""
    r = int(load_library().yolosod_debug_swin_last_route())
    return None if r < 0 else SWIN_ROUTES[r]


def swin_prep_bytes(C, num_heads, hid) -> int:
    """Size of the fp16-split Swin kernels' prepared-parameter block (0: no prepared path for this shape, or the
    split kernels are switched off - yolosod_debug_set_swin_x3 / YOLOSOD_SWIN_X3=0)."""
    return int(load_library().yolosod_swin_prep_bytes(int(C), int(num_heads), int(hid)))


def swin_prepare(x, num_heads, ln1_w, ln1_b, in_w, in_b, out_w, ln2_w, ln2_b, m1_w, m1_b, m2_w, pw_w, bn_w, bn_b,
                 bn_mean, bn_var, bn_eps):
    """The prepared-parameter block (uint8 tensor on x's device) for swin_forward(..., prep=...)."""
    return ops().swin_prep(x, int(num_heads), ln1_w, ln1_b, in_w, in_b, out_w, ln2_w, ln2_b, m1_w, m1_b, m2_w, pw_w,
                           bn_w, bn_b, bn_mean, bn_var, float(bn_eps))


def mamba_glu_forward(x, reduction, in_w, in_bn_w, in_bn_b, in_bn_m, in_bn_v, in_eps, pw1_w, dw_w, bn_w, bn_b, bn_m,
                      bn_v, bn_eps, pw2_w, out_w, out_bn_w, out_bn_b, out_bn_m, out_bn_v, out_eps):
    """MambaBlock GLU fallback (blocks_mamba.py:94-113,198-236): x [B,C,H,W] -> x + out_proj(up(GLU(pool(in_proj x))))."""
    lib = load_library()
    B, C, H, W = x.shape
    ch = in_w.shape[0]
    hd = 2 * ch
    r = int(reduction)
    if r < 1 or H // r < 1 or W // r < 1:
        raise RuntimeError(f"MambaBlock: seq_reduction {r} too large for {H}x{W}")
    if C % 32 or ch % 32:
        raise RuntimeError(f"MambaBlock: channels {C} / hidden {ch} must be multiples of 32 (MFMA GEMM K tiles)")
    y = torch.empty_like(x)
    ws = _workspace(lib.yolosod_mamba_glu_workspace(B, C, H, W, ch, r), x.device)
    _check(_launch(("mamba", tuple(x.shape), (ch, r)), x.device, lib.yolosod_mamba_glu_forward,
        _dev(x, "x"), _dev(y, "y"), B, C, H, W, ch, r, _p(in_w, "in_proj.0.weight", ch * C),
        _p(in_bn_w, "in_proj.1.weight", ch), _p(in_bn_b, "in_proj.1.bias", ch), _p(in_bn_m, "in_proj.1.running_mean", ch),
        _p(in_bn_v, "in_proj.1.running_var", ch), float(in_eps), _p(pw1_w, "fallback.pw1.weight", 2 * hd * ch),
        _p(dw_w, "fallback.dw.weight", hd * 9), _p(bn_w, "fallback.bn.weight", hd), _p(bn_b, "fallback.bn.bias", hd),
        _p(bn_m, "fallback.bn.running_mean", hd), _p(bn_v, "fallback.bn.running_var", hd), float(bn_eps),
        _p(pw2_w, "fallback.pw2.weight", ch * hd), _p(out_w, "out_proj.0.weight", C * ch),
        _p(out_bn_w, "out_proj.1.weight", C), _p(out_bn_b, "out_proj.1.bias", C),
        _p(out_bn_m, "out_proj.1.running_mean", C), _p(out_bn_v, "out_proj.1.running_var", C), float(out_eps),
        ws.data_ptr(), ws.numel(), _stream(x.device)), "mamba_glu_forward")
    return y


def detect_decode(maps, strides, nc, reg_max=16):
    """maps: list of [B, 4*reg_max+nc, Hi, Wi] fp32 -> y [B, 4+nc, A] (torch.ops.yolosod.detect_decode_fwd)."""
    no = 4 * reg_max + nc
    B = maps[0].shape[0]
    for i, m in enumerate(maps):
        _t(m, f"maps[{i}]")
        if m.dim() != 4 or m.shape[0] != B or m.shape[1] != no:
            raise RuntimeError(f"detect_decode: map {i} has shape {tuple(m.shape)}, expected [B,{no},H,W]")
    A = sum(m.shape[2] * m.shape[3] for m in maps)
    return _launch(("decode", (B, A), nc), maps[0].device, ops().detect_decode_fwd, list(maps),
                   [float(s) for s in strides], int(nc), int(reg_max))


def detect_head(box_feats, cls_feats, box_w, box_b, cls_w, cls_b, strides, nc, reg_max=16):
    """Fused last 1x1 convs of both Detect towers + decode (torch.ops.yolosod.detect_head_fwd). box_feats[i]
    [B, c2, Hi, Wi], cls_feats[i] [B, c3, Hi, Wi] contiguous fp32 or bf16 (all levels alike); box_w[i] [64, c2],
    cls_w[i] [nc, c3] and biases fp32 -> y [B, 4+nc, A] fp32 (the decode stays fp32 in the bf16 config)."""
    bf = _act_dtype(_t(box_feats[0], "box_feats[0]"))
    B, c2 = box_feats[0].shape[:2]
    c3 = cls_feats[0].shape[1]
    A = sum(t.shape[2] * t.shape[3] for t in box_feats)
    return _launch(("head", (B, A), (nc, c2, c3)) + ((2,) if bf else ()), box_feats[0].device, ops().detect_head_fwd,
                   list(box_feats), list(cls_feats), list(box_w), list(box_b), list(cls_w), list(cls_b),
                   [float(s) for s in strides], int(nc), int(reg_max))


def detect_head_into(y, l0, l1, box_feats, cls_feats, box_w, box_b, cls_w, cls_b, strides, nc, reg_max=16):
    """``detect_head`` for levels [l0, l1) only, into y [B, 4+nc, A] laid out for all levels (torch.ops.yolosod.
    detect_head_into): the executor decodes the levels whose towers are done while the last level's still run."""
    if any(not isinstance(t, torch.Tensor) for t in box_feats):
        return _detect_head_into_sized(y, l0, l1, box_feats, cls_feats, box_w, box_b, cls_w, cls_b, strides, nc, reg_max)
    bf = _act_dtype(_t(box_feats[0], "box_feats[0]"))
    B, c2 = box_feats[0].shape[:2]
    c3 = cls_feats[0].shape[1]
    A = sum(t.shape[2] * t.shape[3] for t in box_feats[l0:l1])  # the anchors this launch decodes (perf.op_cost)
    _launch(("head", (B, A), (nc, c2, c3)) + ((2,) if bf else ()), box_feats[0].device, ops().detect_head_into, y,
            int(l0), int(l1), list(box_feats), list(cls_feats), list(box_w), list(box_b), list(cls_w), list(cls_b),
            [float(s) for s in strides], int(nc), int(reg_max))
    return y


def _detect_head_into_sized(y, l0, l1, box_feats, cls_feats, box_w, box_b, cls_w, cls_b, strides, nc, reg_max):
    """detect_head_into when a level outside [l0, l1) has no tower features (a level whose tower convs decoded it
    themselves, conv3x3_head): its entry of box_feats is its map size (H, W) and its entry of cls_feats is ignored.
    fp32 features; straight on the C ABI (yolosod_detect_head_levels), since the registered op takes tensors only."""
    lib = load_library()
    nl = len(box_feats)
    if not (0 <= l0 < l1 <= nl) or any(not isinstance(box_feats[i], torch.Tensor) for i in range(l0, l1)):
        raise RuntimeError(f"detect_head_into: levels [{l0}, {l1}) need their tower features")
    f0 = box_feats[l0]
    B, c2 = f0.shape[:2]
    c3 = cls_feats[l0].shape[1]
    hs, ws, keep = [], [], []
    fb, fc, pw = ((ctypes.c_void_p * nl)() for _ in range(3))
    pb, cw, cb = ((ctypes.c_void_p * nl)() for _ in range(3))
    for i in range(nl):
        if isinstance(box_feats[i], torch.Tensor):
            hs.append(int(box_feats[i].shape[2]))
            ws.append(int(box_feats[i].shape[3]))
        else:
            hs.append(int(box_feats[i][0]))
            ws.append(int(box_feats[i][1]))
        if l0 <= i < l1:
            if tuple(box_feats[i].shape[:2]) != (B, c2) or tuple(cls_feats[i].shape) != (B, c3, hs[i], ws[i]):
                raise RuntimeError(f"detect_head_into: level {i} features {tuple(box_feats[i].shape)} / "
                                   f"{tuple(cls_feats[i].shape)} mismatch")
            ts = (box_feats[i], cls_feats[i], box_w[i], box_b[i], cls_w[i], cls_b[i])
            ne = (None, None, 64 * c2, 64, nc * c3, nc)
            for arr, t, n in zip((fb, fc, pw, pb, cw, cb), ts, ne):
                arr[i] = _p(t, f"detect_head_into: level {i}", n)
            keep.append(ts)
    A = sum(h * w for h, w in zip(hs, ws))
    if (y.dtype != torch.float32 or not y.is_contiguous() or tuple(y.shape) != (B, 4 + nc, A)
            or y.device != f0.device):
        raise RuntimeError(f"detect_head_into: y {tuple(y.shape)} is not a contiguous fp32 [{B}, {4 + nc}, {A}] tensor")
    Al = sum(hs[i] * ws[i] for i in range(l0, l1))  # the anchors this launch decodes (perf.op_cost)
    ih, iw = (ctypes.c_int * nl)(*hs), (ctypes.c_int * nl)(*ws)
    st = (ctypes.c_float * nl)(*[float(s) for s in strides])
    _check(_launch(("head", (B, Al), (nc, c2, c3)), f0.device, lib.yolosod_detect_head_levels, nl, int(l0), int(l1),
                   fb, fc, int(c2), int(c3), pw, pb, cw, cb, ih, iw, st, int(B), int(nc), int(reg_max), y.data_ptr(),
                   0, _stream(f0.device)), "detect_head_into")
    return y


def nms(pred, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, max_nms, max_wh, in_place):
    """Batched NMS on pred [B, 4+nc, A] (GPU; torch.ops.yolosod.nms_batched). Returns (out [B,max_det,6],
    counts [B] int32, index [B,max_det] int32). in_place: pred[:, :4] is rewritten to xyxy (the reference's
    non_max_suppression(in_place=True)); otherwise pred is left untouched (no copy is made)."""
    B, no, A = _t(pred, "prediction").shape
    cls = None
    if classes is not None:
        cls = torch.as_tensor(classes, dtype=torch.int32, device=pred.device).reshape(-1).contiguous()
    return _launch(("nms", (B, no - 4, A), int(multi_label)), pred.device, ops().nms_batched, pred, float(conf_thres),
                   float(iou_thres), cls, bool(agnostic), bool(multi_label), int(max_det), int(max_nms), float(max_wh),
                   bool(in_place))


NMS_MERGE_MAX_DET = 1024  # yolosod_nms_merged: the merge launch holds an image's kept rows in one grid row of 8-row groups


def nms_merged(pred, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, max_nms, max_wh, in_place,
               n_merged=None):
    """:func:`nms`, then every kept box replaced by the score-weighted mean of its cluster (merge-NMS, the definition
    in include/yolosod_hip.h; torch.ops.yolosod.nms_merged_batched). Returns (out, counts, index, n_merged
    [B, max_det] int32 = the clusters' sizes, 0 for padding rows). max_det 1..1024."""
    B, no, A = _t(pred, "prediction").shape
    if not 1 <= int(max_det) <= NMS_MERGE_MAX_DET:
        raise ValueError(f"nms_merged: max_det={max_det} unsupported with merging (1..{NMS_MERGE_MAX_DET})")
    cls = None
    if classes is not None:
        cls = torch.as_tensor(classes, dtype=torch.int32, device=pred.device).reshape(-1).contiguous()
    return _launch(("nms", (B, no - 4, A), int(multi_label)), pred.device, ops().nms_merged_batched, pred,
                   float(conf_thres), float(iou_thres), cls, bool(agnostic), bool(multi_label), int(max_det),
                   int(max_nms), float(max_wh), bool(in_place), n_merged)


def bias_act(y, bias, act, out=None, res=None, stats=None, out2=None, c2lo=0):
    """Backbone conv epilogue: out = act(y + bias[c]) (+ res). ``out`` may be a channel slice [B, C, H, W] of a
    larger contiguous concat buffer (batch stride > C*H*W); ``res`` likewise. In place when out is None.
    ``stats`` ("sum" / "summax"): also emit out's per-plane partial sums (+ maxes) for a following SE / CBAM,
    attached to the returned tensor as ``_ys_plane_stats`` (PlaneStats); "capool": the row / column means a
    following CA_Block pools, attached as ``_ys_ca_pool`` ([B, C, H + W], shape). y / out / res / out2 are fp32
    or bf16 (all alike; bias fp32); the statistics are fp32 of the stored values."""
    lib = load_library()
    bf = _act_dtype(y)
    dt = y.dtype
    B, C, H, W = y.shape
    HW = H * W
    if out is None:
        out = y
    if out2 is not None and stats is not None:  # statistics variants have no dual store: copy afterwards
        out = bias_act(y, bias, act, out=out, res=res, stats=stats)
        out2.copy_(out[:, c2lo:])
        return out

    def bstride(t, name):
        if t.device.type != "cuda" or t.dtype != dt:
            raise RuntimeError(f"bias_act: {name} must be a {dt} GPU tensor")
        if t.shape != y.shape or t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != HW:
            raise RuntimeError(f"bias_act: {name} must be [B,C,H,W] with contiguous channels (got {t.stride()})")
        return t.stride(0)

    yb = bstride(y, "y")
    ob = bstride(out, "out")
    rb = bstride(res, "res") if res is not None else 0
    rp = None if res is None else res.data_ptr()
    bp = _dev(bias, "bias")
    # op_timer key: extra = variant (+ "+res" with a shortcut input); bf16 launches carry the element size 2
    tail = (2,) if bf else ()
    rs = "" if res is None else "+res"

    def key(variant):
        return ("bias_act", tuple(y.shape), (variant + rs) if variant else (rs[1:] or None)) + tail

    if out2 is not None and stats is None:  # ``out2`` = packed copy of channels [c2lo, C) (next conv's input)
        if (out2.device.type != "cuda" or out2.dtype != dt or tuple(out2.shape) != (B, C - c2lo, H, W)
                or out2.stride(3) != 1 or out2.stride(2) != W or out2.stride(1) != HW):
            raise RuntimeError(f"bias_act: out2 must be a {dt} GPU tensor [B, C - c2lo, H, W] with contiguous channels")
        if bf:
            _check(_launch(key("dual"), y.device, lib.yolosod_bias_act_bf16, y.data_ptr(), yb,
                           out.data_ptr(), ob, bp, rp, rb, out2.data_ptr(), out2.stride(0), int(c2lo), B, C, HW,
                           int(act), _stream(y.device)), "bias_act_bf16")
        else:
            _check(_launch(key("dual"), y.device, lib.yolosod_bias_act_dual, y.data_ptr(), yb,
                           out.data_ptr(), ob, bp, rp, rb, out2.data_ptr(), out2.stride(0), int(c2lo), B, C, HW,
                           int(act), _stream(y.device)), "bias_act_dual")
        return out
    if stats == "capool":  # CA_Block input: pooled row / column means of out, [B, C, H + W]
        if W % 4 or W > 1024:
            stats = None
        else:
            yin = torch.empty((B, C, H + W), dtype=torch.float32, device=y.device)
            fn = lib.yolosod_bias_act_capool_bf16 if bf else lib.yolosod_bias_act_capool
            _check(_launch(key("capool"), y.device, fn, y.data_ptr(), yb, out.data_ptr(), ob,
                           bp, rp, rb, B, C, H, W, int(act), yin.data_ptr(), _stream(y.device)), "bias_act_capool")
            out._ys_ca_pool = (yin, tuple(out.shape))
            return out
    if stats is not None:
        parts, seg = plane_parts(HW)
        psum = torch.empty(B * C * parts, dtype=torch.float32, device=y.device)
        pmax = torch.empty_like(psum) if stats == "summax" else None
        fn = lib.yolosod_bias_act_stats_bf16 if bf else lib.yolosod_bias_act_stats
        _check(_launch(key(stats), y.device, fn, y.data_ptr(), yb, out.data_ptr(), ob, bp,
                       rp, rb, B, C, HW, int(act), parts, seg, psum.data_ptr(),
                       None if pmax is None else pmax.data_ptr(), _stream(y.device)), "bias_act_stats")
        out._ys_plane_stats = PlaneStats(psum, pmax, parts, out.shape)
        return out
    if bf:
        _check(_launch(key(None), y.device, lib.yolosod_bias_act_bf16, y.data_ptr(), yb,
                       out.data_ptr(), ob, bp, rp, rb, None, 0, 0, B, C, HW, int(act), _stream(y.device)),
               "bias_act_bf16")
        return out
    _check(_launch(key(None), y.device, lib.yolosod_bias_act, y.data_ptr(), yb, out.data_ptr(),
                   ob, bp, rp, rb, B, C, HW, int(act), _stream(y.device)), "bias_act")
    return out


STEM_TILE_ROWS = 8  # output rows per workgroup tile of csrc/stem.hip


def stem_ok(x, conv) -> bool:
    """Shapes the stem kernel takes (yolosod_stem_conv): a fused (bias-carrying) 3 -> Cout 3x3 / stride-2 / pad-1 conv
    on a contiguous fp32 GPU batch with even H, W and Wout % 4 == 0, Cout even and <= 64. Everything else (bf16, odd
    sizes, other Cin, CPU tensors, an un-fused Conv) keeps the MIOpen + epilogue path."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.device.type != "cuda" or x.dtype != torch.float32:
        return False
    B, Cin, H, W = x.shape
    if (conv.bias is None or Cin != 3 or conv.in_channels != 3 or conv.kernel_size != (3, 3) or conv.stride != (2, 2)
            or conv.padding != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1
            or conv.padding_mode != "zeros" or conv.weight.dtype != torch.float32 or conv.weight.device != x.device):
        return False
    Cout = conv.out_channels
    if Cout % 2 or Cout > 64 or B == 0 or H % 2 or W % 2 or (W // 2) % 4:
        return False
    if not x.is_contiguous() or x.data_ptr() % 16:
        return False
    parts, seg = plane_parts((H // 2) * (W // 2))
    return parts == 1 or STEM_TILE_ROWS * (W // 2) <= seg  # a tile meets at most two plan segments


def stem_conv(x, weight, bias):
    """out = SiLU(conv3x3 / stride 2 / pad 1 (x, weight) + bias) for x [B, 3, H, W] fp32 in one HIP pass (exact fp32
    FMAs, csrc/stem.hip), with the output's per-plane partial sums attached as ``_ys_plane_stats`` (PlaneStats) for
    the SE that follows, as ``bias_act(stats="sum")`` attaches them (torch.ops.yolosod.stem_fwd). Shapes: ``stem_ok``."""
    B, _, H, W = _t(x, "x").shape
    Cout = int(weight.shape[0])
    out, psum = _launch(("stem", tuple(x.shape), (Cout, "sum")), x.device, ops().stem_fwd, x, weight, bias)
    out._ys_plane_stats = PlaneStats(psum, None, plane_parts((H // 2) * (W // 2))[0], out.shape)
    return out


def upsample2x_into(x, out) -> bool:
    """Nearest 2x upsample of x [B, C, h, w] (contiguous, fp32 / bf16) into ``out`` [B, C, 2h, 2w], a channel slice
    of a Concat buffer (contiguous channels, any batch stride): the neck's ``nn.Upsample`` + ``Concat`` glue
    (tasks._predict_once_planned). Returns False, launching nothing, when the HIP kernel's shape / alignment
    conditions (w % 4 == 0, 16-byte aligned operands and strides) do not hold."""
    B, C, h, w = x.shape
    if (x.device.type != "cuda" or out.device != x.device or out.dtype != x.dtype or x.dtype not in (torch.float32, _BF16)
            or not x.is_contiguous() or tuple(out.shape) != (B, C, 2 * h, 2 * w) or out.stride(3) != 1
            or out.stride(2) != 2 * w or out.stride(1) != 4 * h * w):
        return False
    eb = x.element_size()
    if (w % 4 or x.data_ptr() % 16 or out.data_ptr() % 16 or (out.stride(0) * eb) % 16 or (4 * h * w * eb) % 16
            or B == 0):
        return False
    _check(_launch(("upsample2x", tuple(x.shape), None), x.device, load_library().yolosod_upsample2x, x.data_ptr(),
                   out.data_ptr(), out.stride(0), B, C, h, w, eb, _stream(x.device)), "upsample2x")
    return True


THIN1X1_COUT = (64, 128)
THIN1X1_CIN = (64, 96, 128, 192, 256)


def conv1x1_thin_ok(x, cout) -> bool:
    """Shapes the thin fused 1x1 conv kernel takes (yolosod_conv1x1_thin; a CatView: yolosod_conv1x1_thin_cat)."""
    if isinstance(x, CatView):  # any split; both parts fp32 on the GPU with contiguous images
        B, Cin, H, W = x.shape
        return (x.device.type == "cuda" and x.dtype == torch.float32 and cout in THIN1X1_COUT and Cin in THIN1X1_CIN
                and (H * W) % 64 == 0 and all(_imgs_contig(t) for t in x.parts) and (not x.up0 or W % 4 == 0))
    B, Cin, H, W = x.shape
    return (x.device.type == "cuda" and x.dtype == torch.float32 and cout in THIN1X1_COUT and Cin in THIN1X1_CIN
            and (H * W) % 64 == 0 and x.stride(3) == 1 and x.stride(2) == W and x.stride(1) == H * W
            and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0)


def conv1x1_thin(x, w, bias, out=None, res=None, out2=None, c2lo=0, stats=None):
    """SiLU(1x1 conv(x) + bias) (+ res) for Cout 64 / 128 and Cin <= 256 in one HIP kernel (weights in registers,
    x tiles in LDS, fp32 MFMA); ``x`` / ``out`` / ``res`` may be channel slices, ``out2`` = packed channels
    [c2lo, Cout)."""
    lib = load_library()
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    HW = H * W
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)

    def bstride(t, name, C):
        if t.device.type != "cuda" or t.dtype != torch.float32:
            raise RuntimeError(f"conv1x1_thin: {name} must be a float32 GPU tensor")
        if tuple(t.shape) != (B, C, H, W) or t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != HW:
            raise RuntimeError(f"conv1x1_thin: {name} must be [B,{C},H,W] with contiguous channels")
        return t.stride(0)

    if isinstance(x, CatView):  # a virtual concat: both parts read in place (no residual / statistics)
        if res is not None or stats is not None:
            raise RuntimeError("conv1x1_thin: a CatView input takes no res / stats")
        x0, x1 = x.parts
        k1 = int(x0.shape[1])
        ob = bstride(out, "out", Cout)
        o2 = bstride(out2, "out2", Cout - c2lo) if out2 is not None else 0
        if x.up0:  # part 0 is the quarter-size source of a nearest 2x upsample, addressed in place (CatView checked it)
            if not _imgs_contig(x0) or W % 4:
                raise RuntimeError("conv1x1_thin: an upsampled CatView part needs contiguous images and W % 4 == 0")
            xb0 = x0.stride(0)
        else:
            xb0 = bstride(x0, "x", k1)
        _check(_launch(("conv1x1_thin", tuple(x.shape), (Cout, False, out2 is not None, "cat")), x.device,
                       lib.yolosod_conv1x1_thin_cat, x0.data_ptr(), xb0, x1.data_ptr(),
                       bstride(x1, "x2", Cin - k1), k1, _dev(w.contiguous(), "weight"), _dev(bias, "bias"),
                       out.data_ptr(), ob, None if out2 is None else out2.data_ptr(), o2, int(c2lo), B, Cin, Cout, HW,
                       W if x.up0 else 0, _stream(x.device)), "conv1x1_thin_cat")
        return out
    xb = bstride(x, "x", Cin)
    ob = bstride(out, "out", Cout)
    rb = bstride(res, "res", Cout) if res is not None else 0
    o2 = bstride(out2, "out2", Cout - c2lo) if out2 is not None else 0
    if stats in ("sum", "summax") and res is None and out2 is None:
        # the same pass also yields the following SE / CBAM gate's plane statistics (PlaneStats on the output)
        parts, _ = plane_parts(HW)
        psum = torch.empty(B * Cout * parts, dtype=torch.float32, device=x.device)
        pmax = torch.empty_like(psum) if stats == "summax" else None
        tws = torch.empty(2 * B * Cout * (HW // 64), dtype=torch.float32, device=x.device)
        _check(_launch(("conv1x1_thin", tuple(x.shape), (Cout, stats)), x.device, lib.yolosod_conv1x1_thin_stats, x.data_ptr(), xb, _dev(w.contiguous(), "weight"), _dev(bias, "bias"),
                                              out.data_ptr(), ob, B, Cin, Cout, HW, parts, psum.data_ptr(),
                                              None if pmax is None else pmax.data_ptr(), tws.data_ptr(), _stream(x.device)),
               "conv1x1_thin_stats")
        out._ys_plane_stats = PlaneStats(psum, pmax, parts, out.shape)
        return out
    if stats is not None:
        raise RuntimeError(f"conv1x1_thin: stats={stats!r} needs res=None and out2=None")
    _check(_launch(("conv1x1_thin", tuple(x.shape), (Cout, res is not None, out2 is not None)), x.device, lib.yolosod_conv1x1_thin, x.data_ptr(), xb, _dev(w.contiguous(), "weight"), _dev(bias, "bias"),
                                    out.data_ptr(), ob, None if res is None else res.data_ptr(), rb,
                                    None if out2 is None else out2.data_ptr(), o2, int(c2lo), B, Cin, Cout, HW,
                                    _stream(x.device)), "conv1x1_thin")
    return out


def conv1x1(x, w, bias, act, out=None, res=None):
    """1x1 conv (stride 1, groups 1) + bias + act (+ res) as one fused GEMM; ``x``/``out``/``res`` may be
    channel slices of concat buffers (contiguous channels, any batch stride)."""
    lib = load_library()
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    HW = H * W
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)

    def bstride(t, name, C):
        if t.device.type != "cuda" or t.dtype != torch.float32:
            raise RuntimeError(f"conv1x1: {name} must be a float32 GPU tensor")
        if tuple(t.shape) != (B, C, H, W) or t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != HW:
            raise RuntimeError(f"conv1x1: {name} must be [B,{C},H,W] with contiguous channels")
        return t.stride(0)

    xb = bstride(x, "x", Cin)
    ob = bstride(out, "out", Cout)
    rb = bstride(res, "res", Cout) if res is not None else 0
    _check(_launch(("conv1x1", tuple(x.shape), Cout), x.device, lib.yolosod_conv1x1, x.data_ptr(), xb, _dev(w, "weight"), None if bias is None else _dev(bias, "bias"),
                               out.data_ptr(), ob, None if res is None else res.data_ptr(), rb, B, Cin, Cout, HW,
                               int(act), _stream(x.device)), "conv1x1")
    return out


def conv3x3_ok(x, conv) -> bool:
    """Shapes the fp16-split 3x3 conv kernel takes (yolosod_conv3x3_silu_xs): fp32 NCHW on a GPU with contiguous
    images (any batch stride: a channel slice), 3x3 / stride 1 / pad 1 / dilation 1 / groups 1, 32 or a multiple of
    64 (<= 512) outputs, Cin a multiple of 32."""
    return (x.device.type == "cuda" and x.dtype == torch.float32 and x.dim() == 4 and _imgs_contig(x)
            and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and x.shape[1] == conv.in_channels
            and int(load_library().yolosod_conv3x3_prep_bytes_ex(int(conv.in_channels), int(conv.out_channels))) > 0)


def _split_prepare(name, bytes_fn, prepare_fn, w):
    """Prepared block (uint8 tensor) of the conv weight ``w`` [Cout, Cin, ...] for the fp16-split conv kernel ``name``
    (csrc/split_conv.h); ``bytes_fn`` / ``prepare_fn``: the kernel's yolosod_*_prep_bytes / *_prepare entries."""
    cout, cin = int(w.shape[0]), int(w.shape[1])
    nbytes = int(bytes_fn(cin, cout))
    if nbytes == 0:
        raise RuntimeError(f"{name}: (Cin={cin}, Cout={cout}) unsupported")
    blk = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    wc = w.detach().float().contiguous()
    _check(_launch((f"{name}_prep", (cout, cin), None), w.device, prepare_fn, _dev(wc, "weight"), cin, cout,
                   blk.data_ptr(), nbytes, _stream(w.device)), f"{name}_prepare")
    return blk


def conv3x3_prepare(w):
    """Prepared block (fragment-major fp16 split planes of 64 W, uint8 tensor) of a [Cout, Cin, 3, 3] fp32 weight."""
    lib = load_library()
    return _split_prepare("conv3x3", lib.yolosod_conv3x3_prep_bytes_ex, lib.yolosod_conv3x3_prepare_ex, w)


def _img_view(t, shape, name):
    """t is a [B, C, H, W] fp32 view on the GPU whose images are contiguous (a channel slice of a concat buffer)."""
    B, C, H, W = shape
    if (tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or t.device.type != "cuda"
            or t.stride()[1:] != (H * W, W, 1) or t.data_ptr() % 16 or t.stride(0) % 4):
        raise RuntimeError(f"{name} {tuple(t.shape)} / {t.stride()} is not a [{B}, {C}, {H}, {W}] fp32 view with "
                           "contiguous 16-byte aligned images")


def conv3x3_silu(x, bias, prep, cout=64, out=None, res=None, op="conv3x3"):
    """SiLU(conv3x3(x) + bias) (+ res) on the fp16 two-term split MFMA (csrc/conv3x3.hip); ``prep`` is a callable
    returning the cached prepared block of the weights (conv3x3_prepare); ``out``: a [B, Cout, H, W] view with
    contiguous images (a concat slice) to write; ``res``: the residual added after the activation (same shape);
    ``op``: the op_timer key's name (the backbone's launches are recorded as "conv3x3_backbone")."""
    lib = load_library()
    B, Cin, H, W = x.shape
    if out is None:
        y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    else:
        _img_view(out, (B, cout, H, W), "conv3x3: out")
        y = out
    if res is not None:
        _img_view(res, (B, cout, H, W), "conv3x3: res")
    b = bias.detach().float().contiguous()

    def run():
        blk = prep()
        _img_view(x, (B, Cin, H, W), "conv3x3: x")
        return lib.yolosod_conv3x3_silu_xs(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0),
                                           None if res is None else res.data_ptr(),
                                           0 if res is None else res.stride(0), B, Cin, cout, H, W, _dev(b, "bias"),
                                           blk.data_ptr(), blk.numel(), _stream(x.device))

    _check(_launch((op, tuple(x.shape), cout if res is None else (cout, "res")), x.device, run), "conv3x3")
    return y


def conv3x3_head_fused(B, H, W) -> bool:
    """Whether a Detect level with [B, 64, H, W] tower maps runs its towers' last convs with the head's tail in their
    epilogue (yolosod_debug_conv3x3_head_fused: the shapes whose 64 -> 64 launch runs in 64-channel groups, or the
    route forced by yolosod_debug_set_conv3x3_head_fuse)."""
    return bool(load_library().yolosod_debug_conv3x3_head_fused(int(B), int(H), int(W)))


def detect_head_prepare(w, rows):
    """Prepared block (uint8 tensor) of a tower's last 1x1 conv weight ``w`` [rows, 64(, 1, 1)] for conv3x3_head."""
    lib = load_library()
    nbytes = int(lib.yolosod_detect_head_prep_bytes(int(rows)))
    wc = w.detach().float().reshape(w.shape[0], -1).contiguous()
    if nbytes == 0 or tuple(wc.shape) != (rows, 64):
        raise RuntimeError(f"detect_head_prepare: weight {tuple(w.shape)} unsupported ([64 | 1..16, 64])")
    blk = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _check(_launch(("head_prep", (rows, 64), None), w.device, lib.yolosod_detect_head_prepare, _dev(wc, "weight"),
                   int(rows), blk.data_ptr(), nbytes, _stream(w.device)), "detect_head_prepare")
    return blk


def conv3x3_head(x, bias, prep, head_prep, head_bias, mode, nc, stride, y, a_off):
    """A Detect tower's last 3x3 conv (64 -> 64) + its 1x1 conv + the decode in one launch (csrc/conv3x3.hip,
    conv3x3_head_kernel), bit-identical to conv3x3_silu followed by detect_head_into on that level: ``mode`` 1 writes
    the box rows 0 .. 3, 2 the class rows 4 .. 4 + nc - 1, of anchors [a_off, a_off + H W) of y [B, 4 + nc, A]. ``prep``
    / ``head_prep``: callables returning the cached prepared blocks (conv3x3_prepare / detect_head_prepare)."""
    lib = load_library()
    B, Cin, H, W = x.shape
    if Cin != 64:
        raise RuntimeError(f"conv3x3_head: {Cin} channels (64 only)")
    if (y.dtype != torch.float32 or y.device != x.device or not y.is_contiguous() or y.dim() != 3 or y.shape[0] != B
            or y.shape[1] != 4 + nc):
        raise RuntimeError(f"conv3x3_head: y {tuple(y.shape)} is not a contiguous fp32 [{B}, {4 + nc}, A] tensor")
    b = bias.detach().float().contiguous()
    hb = head_bias.detach().float().contiguous()
    if hb.numel() != (64 if mode == 1 else nc):
        raise RuntimeError(f"conv3x3_head: head bias of {hb.numel()} values")

    def run():
        blk, hblk = prep(), head_prep()
        _img_view(x, (B, 64, H, W), "conv3x3_head: x")
        return lib.yolosod_conv3x3_head_xs(x.data_ptr(), x.stride(0), B, H, W, _dev(b, "bias"), blk.data_ptr(),
                                           blk.numel(), hblk.data_ptr(), _dev(hb, "head bias"), int(mode), int(nc),
                                           float(stride), y.data_ptr(), int(y.shape[2]), int(a_off), _stream(x.device))

    _check(_launch(("conv3x3", tuple(x.shape), (64, "head", int(mode))), x.device, run), "conv3x3_head")
    return y


def bottleneck3x3_fused(B, H, W) -> bool:
    """Whether a [B, 32, H, W] Bottleneck is to run as one launch (yolosod_debug_bottleneck3x3_fused: large maps, or
    the form forced by yolosod_debug_set_bottleneck3x3_fuse)."""
    return bool(load_library().yolosod_debug_bottleneck3x3_fused(int(B), int(H), int(W)))


def bottleneck3x3_silu(x, bias1, prep1, bias2, prep2, out=None, res=None, op="bottleneck3x3"):
    """[res +] SiLU(conv3x3(SiLU(conv3x3(x) + bias1)) + bias2) for 32 -> 32 -> 32 channels as one launch
    (csrc/conv3x3.hip, bottleneck3x3_c32_kernel), bit-identical to conv3x3_silu twice; ``prep1`` / ``prep2``: callables
    returning the cached prepared blocks of the two weights; ``out`` / ``res`` / ``op`` as conv3x3_silu."""
    lib = load_library()
    B, C, H, W = x.shape
    if C != 32:
        raise RuntimeError(f"bottleneck3x3: {C} channels (32 only)")
    if out is None:
        y = torch.empty((B, 32, H, W), dtype=torch.float32, device=x.device)
    else:
        _img_view(out, (B, 32, H, W), "bottleneck3x3: out")
        y = out
    if res is not None:
        _img_view(res, (B, 32, H, W), "bottleneck3x3: res")
    b1 = bias1.detach().float().contiguous()
    b2 = bias2.detach().float().contiguous()

    def run():
        blk1, blk2 = prep1(), prep2()
        _img_view(x, (B, 32, H, W), "bottleneck3x3: x")
        return lib.yolosod_bottleneck3x3_silu_xs(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0),
                                                 None if res is None else res.data_ptr(),
                                                 0 if res is None else res.stride(0), B, H, W, _dev(b1, "bias1"),
                                                 blk1.data_ptr(), blk1.numel(), _dev(b2, "bias2"), blk2.data_ptr(),
                                                 blk2.numel(), _stream(x.device))

    _check(_launch((op, tuple(x.shape), 32 if res is None else (32, "res")), x.device, run), "bottleneck3x3")
    return y


class CatView:
    """A two-part channel concat left unmaterialised: [B, C0 + C1, H, W] as its parts. A neck Concat whose only reader
    is the next C2f's cv1 (a 1x1 conv) hands this over, and the 1x1 kernels read both parts in place
    (yolosod_conv1x1x2_silu_cat / yolosod_conv1x1_thin_cat) instead of a materialised concat (block.py:249-253,
    conv.py:336-340: the conv of a concat = the sum of the convs of its parts over their channel ranges).
    ``up0``: part 0 stands for the nearest 2x upsample of the tensor given ([B, C0, H/2, W/2]: the neck's nn.Upsample
    feeding the Concat, never written out): the 1x1 kernels address it at (y >> 1, x >> 1); ``materialize()``
    upsamples and concatenates, so every other reader sees the Concat's own output."""

    def __init__(self, parts, up0=False):
        a, b = parts
        sp = (2 * a.shape[2], 2 * a.shape[3]) if up0 else tuple(a.shape[2:])
        if a.shape[0] != b.shape[0] or sp != tuple(b.shape[2:]) or a.dtype != b.dtype or a.device != b.device:
            raise ValueError("CatView: parts must agree in batch, spatial size, dtype and device")
        self.parts = (a, b)
        self.up0 = bool(up0)
        self.shape = torch.Size((a.shape[0], a.shape[1] + b.shape[1], b.shape[2], b.shape[3]))
        self.device, self.dtype = a.device, a.dtype

    def dim(self):
        return 4

    def materialize(self):
        a, b = self.parts
        if self.up0:
            a = torch.nn.functional.interpolate(a, scale_factor=2, mode="nearest")
        return torch.cat((a, b), 1)


def sppf_pool(z, c):
    """SPPF's pooling pyramid in place (yolosod_sppf_pool): z [B, 4c, H, W] fp32 with contiguous images (any batch
    stride); channels [c, 4c) <- the one-, two- and three-fold 5x5 / stride-1 / pad-2 max pools of channels [0, c)."""
    B, C4, H, W = z.shape
    if (C4 != 4 * c or z.dtype != torch.float32 or z.device.type != "cuda"
            or z.stride()[1:] != (H * W, W, 1)):  # scalar accesses: no alignment needed
        raise RuntimeError("sppf_pool: z must be a [B, 4c, H, W] fp32 GPU tensor with contiguous images")
    lib = load_library()
    _check(_launch(("sppf_pool", (B, c, H, W), None), z.device, lib.yolosod_sppf_pool, z.data_ptr(), z.stride(0), B,
                   int(c), H, W, _stream(z.device)), "sppf_pool")
    return z


def _imgs_contig(t) -> bool:
    """[B, C, H, W] whose images are contiguous (any batch stride, e.g. a channel slice of a concat buffer)."""
    B, C, H, W = t.shape
    return t.stride()[1:] == (H * W, W, 1) and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


def conv1x1x2_ok(x, conv) -> bool:
    """Shapes the fp16-split 1x1 conv kernel takes (yolosod_conv1x1x2_silu): fp32 on a GPU with contiguous images,
    1x1 / stride 1 / groups 1, Cout a multiple of 128 (<= 1024), Cin a multiple of 32, H*W a multiple of 4."""
    if isinstance(x, CatView):  # both parts in place: the split on a 128-channel stage boundary
        if not (all(_imgs_contig(t) for t in x.parts) and x.parts[0].shape[1] % 128 == 0):
            return False
    elif not (x.dim() == 4 and _imgs_contig(x)):
        return False
    return (x.device.type == "cuda" and x.dtype == torch.float32
            and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1
            and x.shape[1] == conv.in_channels and (x.shape[2] * x.shape[3]) % 4 == 0
            and int(load_library().yolosod_conv1x1x2_prep_bytes(int(conv.in_channels), int(conv.out_channels))) > 0)


def conv1x1x2_prepare(w):
    """Prepared block (fragment-major fp16 split planes of 64 W, Cin padded to 128) of a [Cout, Cin(, 1, 1)] weight."""
    lib = load_library()
    return _split_prepare("conv1x1x2", lib.yolosod_conv1x1x2_prep_bytes, lib.yolosod_conv1x1x2_prepare,
                          w.reshape(int(w.shape[0]), int(w.shape[1])))


def conv1x1x2_silu(x, bias, prep, cout, out=None, out2=None, c2lo=0, op="conv1x1x2", stats=None):
    """SiLU(W x + bias) for a 1x1 conv on the fp16 two-term split MFMA (csrc/conv1x1x2.hip). ``x``, ``out`` may be
    channel slices of concat buffers (contiguous images); ``out2``: channels [c2lo, Cout) stored again (packed);
    ``op``: the op_timer key's name (the backbone's launches are recorded as "conv1x1x2_backbone").
    ``stats`` ("sum" / "summax"): the same launch emits the output's plane statistics for the SE / CBAM gate that
    follows (yolosod_conv1x1x2_silu_stats), attached as ``_ys_plane_stats`` (PlaneStats) the way bias_act(stats=...)
    attaches them; "capool": the plain launch - the CA_Block that follows pools the finished output itself. These
    launches are recorded as ("conv1x1x2_stats", x.shape, (cout, stats)) and take no out2 and no CatView."""
    lib = load_library()
    B, Cin, H, W = x.shape
    if stats is not None and (stats not in ("sum", "summax", "capool") or out2 is not None or isinstance(x, CatView)):
        raise RuntimeError(f"conv1x1x2: stats={stats!r} takes one input tensor, no out2")
    if out is None:
        y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    else:
        _img_view(out, (B, cout, H, W), "conv1x1x2: out")
        y = out
    if out2 is not None:
        _img_view(out2, (B, cout - c2lo, H, W), "conv1x1x2: out2")
    b = bias.detach().float().contiguous()
    if stats in ("sum", "summax"):
        HW = H * W
        parts, _ = plane_parts(HW)
        psum = torch.empty(B * cout * parts, dtype=torch.float32, device=x.device)
        pmax = torch.empty_like(psum) if stats == "summax" else None
        tws = torch.empty(2 * B * cout * ((HW + 63) // 64), dtype=torch.float32, device=x.device)

        def run_stats():
            blk = prep()
            return lib.yolosod_conv1x1x2_silu_stats(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), B, Cin, cout,
                                                    HW, _dev(b, "bias"), blk.data_ptr(), blk.numel(),
                                                    2 if stats == "summax" else 1, parts, psum.data_ptr(),
                                                    None if pmax is None else pmax.data_ptr(), tws.data_ptr(),
                                                    _stream(x.device))

        _check(_launch(("conv1x1x2_stats", tuple(x.shape), (cout, stats)), x.device, run_stats), "conv1x1x2_stats")
        y._ys_plane_stats = PlaneStats(psum, pmax, parts, y.shape)
        return y

    x0, x1 = x.parts if isinstance(x, CatView) else (x, None)

    def run():
        blk = prep()
        return lib.yolosod_conv1x1x2_silu_cat(x0.data_ptr(), x0.stride(0), None if x1 is None else x1.data_ptr(),
                                              0 if x1 is None else x1.stride(0), int(x0.shape[1]), y.data_ptr(),
                                              y.stride(0), None if out2 is None else out2.data_ptr(),
                                              0 if out2 is None else out2.stride(0), int(c2lo), B, Cin, cout, H * W,
                                              _dev(b, "bias"), blk.data_ptr(), blk.numel(),
                                              W if x1 is not None and x.up0 else 0, _stream(x.device))

    extra = (cout, out2 is not None) + (("cat",) if x1 is not None else ())
    if stats == "capool":
        op, extra = "conv1x1x2_stats", (cout, stats)
    _check(_launch((op, tuple(x.shape), extra), x.device, run), "conv1x1x2")
    return y


def conv3x3s2_ok(x, conv) -> bool:
    """Shapes the stride-2 fused-gate conv kernel takes (yolosod_conv3x3s2_silu): fp32 contiguous NCHW on a GPU,
    3x3 / stride 2 / pad 1 / dilation 1 / groups 1, 64 or a multiple of 128 (<= 512) outputs, Cin a multiple of 32,
    output width % 4 == 0."""
    return (x.device.type == "cuda" and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
            and conv.kernel_size == (3, 3) and conv.stride == (2, 2) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1
            and (conv.out_channels == 64 or (conv.out_channels % 128 == 0 and conv.out_channels <= 512))
            and conv.in_channels % 32 == 0 and x.shape[1] == conv.in_channels and ((x.shape[3] + 1) // 2) % 4 == 0
            and x.numel() * 4 < 2 ** 32
            and int(load_library().yolosod_conv3x3s2_prep_bytes(int(conv.in_channels), int(conv.out_channels))) > 0)


def conv3x3s2_prepare(w):
    """Prepared block (fragment-major fp16 split planes of 64 W, uint8 tensor) of a [Cout, Cin, 3, 3] fp32 weight."""
    lib = load_library()
    return _split_prepare("conv3x3s2", lib.yolosod_conv3x3s2_prep_bytes, lib.yolosod_conv3x3s2_prepare, w)


def conv3x3s2_silu(x, bias, prep, cout, gate_c=None, gate_p=None, key=None, out=None):
    """SiLU(conv3x3_stride2((x * gate_c) * gate_p) + bias) on the fp16 two-term split MFMA (csrc/conv3x3s2.hip):
    gate_c [B, Cin] (an SE / CBAM channel gate), gate_p [B, H, W] (CBAM's spatial gate), either may be None.
    ``prep``: a callable returning the cached prepared block (conv3x3s2_prepare); ``key``: the op_timer key (default
    ("conv3x3s2", shape, (Cout, gate_c given, gate_p given))); ``out``: a [B, Cout, Ho, Wo] fp32 view whose images are contiguous (e.g. a
    channel slice of a concat buffer) to write instead of a new tensor."""
    lib = load_library()
    B, Cin, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if out is None:
        y = torch.empty((B, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    else:
        y = out
        if (tuple(y.shape) != (B, cout, Ho, Wo) or y.dtype != torch.float32 or y.device != x.device
                or y.stride()[1:] != (Ho * Wo, Wo, 1) or y.data_ptr() % 16 or y.stride(0) % 4):
            raise RuntimeError(f"conv3x3s2: out {tuple(y.shape)} / {y.stride()} is not a [{B}, {cout}, {Ho}, {Wo}] "
                               "fp32 view with contiguous 16-byte aligned images")
    b = bias.detach().float().contiguous()
    gc = None if gate_c is None else gate_c.float().contiguous()
    gp = None if gate_p is None else gate_p.float().contiguous()
    if gc is not None and (tuple(gc.shape) != (B, Cin) or gc.data_ptr() % 16):
        raise RuntimeError(f"conv3x3s2: channel gate {tuple(gc.shape)} (16-byte aligned [{B}, {Cin}] expected)")
    if gp is not None and gp.numel() != B * H * W:
        raise RuntimeError(f"conv3x3s2: spatial gate of {gp.numel()} values ({B * H * W} expected)")

    def run():
        blk = prep()
        return lib.yolosod_conv3x3s2_silu_out(_dev(x, "x"), y.data_ptr(), y.stride(0), B, Cin, cout, H, W,
                                              _dev(b, "bias"), None if gc is None else _dev(gc, "gate_c"),
                                              None if gp is None else _dev(gp, "gate_p"), blk.data_ptr(), blk.numel(),
                                              _stream(x.device))

    if key is None:
        key = ("conv3x3s2", tuple(x.shape), (cout, gc is not None, gp is not None))
    _check(_launch(key, x.device, run), "conv3x3s2")
    return y


INGEST_MAX_DIM = 16384  # source / canvas extents of csrc/ingest.hip (32-bit arithmetic, 14-bit index fields)


def letterbox_ingest(images, out_shape, geoms, dtype=torch.float32, out=None, pad_value=114):
    """Raw frames -> the model's input tensor in one launch (yolosod_letterbox_ingest): ``images`` is a sequence of
    uint8 GPU tensors [h, w, 3] in BGR order (sizes may differ; a row-cropped / column-cropped view is fine: pixel
    stride 3, channel stride 1, any row pitch >= 3 w), ``geoms[i]`` = (new_h, new_w, top, left, ...) as
    ``LetterBox.geometry`` returns it, ``out_shape`` = (out_h, out_w) of the canvas. Returns [B, 3, out_h, out_w]
    RGB / 255 in ``dtype`` (float32 or bfloat16), border ``pad_value`` / 255. ``out``: write into this
    [B, 3, out_h, out_w] tensor instead (contiguous images, any batch stride that is a multiple of 4).

    The descriptor the kernel reads is built here from each tensor's own ``data_ptr()``, shape and strides only, and
    everything the kernel relies on is checked here: nothing is launched on a frame that fails."""
    lib = load_library()
    B = len(images)
    out_h, out_w = int(out_shape[0]), int(out_shape[1])
    if B < 1 or len(geoms) != B:
        raise RuntimeError(f"letterbox_ingest: {B} frames with {len(geoms)} geometries")
    if dtype not in (torch.float32, _BF16):
        raise RuntimeError(f"letterbox_ingest: output dtype must be float32 or bfloat16, got {dtype}")
    if out_w % 4 or not (0 < out_h <= INGEST_MAX_DIM and 0 < out_w <= INGEST_MAX_DIM):
        raise RuntimeError(f"letterbox_ingest: canvas {out_h}x{out_w} unsupported (width % 4 == 0, <= {INGEST_MAX_DIM})")
    rows = []
    dev = None
    for i, (t, g) in enumerate(zip(images, geoms)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"letterbox_ingest: frame {i}: expected a tensor")
        if t.dtype != torch.uint8:
            raise RuntimeError(f"letterbox_ingest: frame {i}: expected uint8, got {t.dtype}")
        if t.dim() != 3 or t.shape[2] != 3:
            raise RuntimeError(f"letterbox_ingest: frame {i}: expected [h, w, 3] (BGR), got {tuple(t.shape)}")
        h, w = int(t.shape[0]), int(t.shape[1])
        if not (0 < h <= INGEST_MAX_DIM and 0 < w <= INGEST_MAX_DIM):
            raise RuntimeError(f"letterbox_ingest: frame {i}: {h}x{w} outside 1..{INGEST_MAX_DIM}")
        if t.stride(2) != 1:
            raise RuntimeError(f"letterbox_ingest: frame {i}: channel stride {t.stride(2)} (1 expected)")
        if w > 1 and t.stride(1) != 3:
            raise RuntimeError(f"letterbox_ingest: frame {i}: pixel stride {t.stride(1)} (3 expected)")
        pitch = int(t.stride(0)) if h > 1 else 3 * w
        if pitch < 3 * w:
            raise RuntimeError(f"letterbox_ingest: frame {i}: row pitch {pitch} < 3 * {w}")
        if t.device.type != "cuda":
            raise RuntimeError(f"letterbox_ingest: frame {i}: HIP kernel requires a GPU tensor (got device "
                               f"{t.device}); no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"letterbox_ingest: frame {i} on {t.device}, frame 0 on {dev}")
        nh, nw, top, left = (int(v) for v in g[:4])
        if nh < 1 or nw < 1 or top < 0 or left < 0 or top + nh > out_h or left + nw > out_w:
            raise RuntimeError(f"letterbox_ingest: frame {i}: geometry {tuple(g)} leaves the {out_h}x{out_w} canvas")
        rows.append([t.data_ptr(), h, w, pitch, nh, nw, top, left])
    if out is None:
        out = torch.empty((B, 3, out_h, out_w), dtype=dtype, device=dev)
    elif (out.dtype != dtype or out.device != dev or tuple(out.shape) != (B, 3, out_h, out_w)
          or out.stride()[1:] != (out_h * out_w, out_w, 1) or out.stride(0) % 4 or out.stride(0) < 3 * out_h * out_w
          or out.data_ptr() % 16):
        raise RuntimeError(f"letterbox_ingest: out must be a {dtype} [{B}, 3, {out_h}, {out_w}] tensor on {dev} with "
                           "contiguous 16-byte aligned images and a batch stride that is a multiple of 4")
    desc = torch.tensor(rows, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    key = ("ingest", (B, 3, out_h, out_w), 2 if dtype == _BF16 else None)
    _check(_launch(key, dev, lib.yolosod_letterbox_ingest, desc.data_ptr(), B, out.data_ptr(), out.stride(0) if B > 1
                   else 3 * out_h * out_w, out_h, out_w, int(dtype == _BF16), int(pad_value), _stream(dev)),
           "letterbox_ingest")
    return out


def letterbox_ingest_nv12(frames, out_shape, geoms, dtype=torch.float32, out=None, pad_value=114):
    """NV12 frames -> the model's input tensor in one launch (yolosod_letterbox_ingest_nv12): ``frames`` is a sequence
    of :class:`~yolosod_amd.data.nv12.NV12Frame` on the GPU (sizes and matrices may differ; a crop at any origin with
    any extents is fine: element stride 1 in ``y``, pixel stride 2 and channel stride 1 in ``uv``, any row pitches).
    ``geoms``, ``out_shape``, ``dtype``, ``out`` and ``pad_value`` as :func:`letterbox_ingest`. The result is bit-equal
    to :func:`letterbox_ingest` on the frames converted to uint8 BGR by the integer definition in ``data/nv12.py``.

    The descriptor the kernel reads is built here from each tensor's own ``data_ptr()``, shape and strides only, and
    everything the kernel relies on is checked here: nothing is launched on a frame that fails."""
    from .data.nv12 import NV12_MATRICES, NV12Frame
    lib = load_library()
    B = len(frames)
    out_h, out_w = int(out_shape[0]), int(out_shape[1])
    if B < 1 or len(geoms) != B:
        raise RuntimeError(f"letterbox_ingest_nv12: {B} frames with {len(geoms)} geometries")
    if dtype not in (torch.float32, _BF16):
        raise RuntimeError(f"letterbox_ingest_nv12: output dtype must be float32 or bfloat16, got {dtype}")
    if out_w % 4 or not (0 < out_h <= INGEST_MAX_DIM and 0 < out_w <= INGEST_MAX_DIM):
        raise RuntimeError(f"letterbox_ingest_nv12: canvas {out_h}x{out_w} unsupported (width % 4 == 0, "
                           f"<= {INGEST_MAX_DIM})")
    rows = []
    dev = None
    for i, (f, g) in enumerate(zip(frames, geoms)):
        if not isinstance(f, NV12Frame):
            raise TypeError(f"letterbox_ingest_nv12: frame {i}: expected an NV12Frame, got {type(f).__name__}")
        y, uv = f.y, f.uv
        py, px = f.parity
        if y.dtype != torch.uint8 or uv.dtype != torch.uint8:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: expected uint8 planes, got {y.dtype} / {uv.dtype}")
        if y.dim() != 2 or uv.dim() != 3 or uv.shape[2] != 2:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: expected y [h, w] and uv [h/2, w/2, 2], got "
                               f"{tuple(y.shape)} / {tuple(uv.shape)}")
        h, w = int(y.shape[0]), int(y.shape[1])
        if not (0 < h <= INGEST_MAX_DIM and 0 < w <= INGEST_MAX_DIM):
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: {h}x{w} outside 1..{INGEST_MAX_DIM}")
        ch, cw = ((h - 1 + py) >> 1) + 1, ((w - 1 + px) >> 1) + 1  # chroma rows / pairs the view's pixels name
        if py not in (0, 1) or px not in (0, 1) or tuple(uv.shape[:2]) != (ch, cw):
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: uv {tuple(uv.shape)} is not the [{ch}, {cw}, 2] of a "
                               f"{h}x{w} view with origin parity ({py}, {px})")
        if f.matrix not in NV12_MATRICES:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: unknown matrix {f.matrix!r}")
        if w > 1 and y.stride(1) != 1:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: y element stride {y.stride(1)} (1 expected)")
        if uv.stride(2) != 1:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: uv channel stride {uv.stride(2)} (1 expected)")
        if cw > 1 and uv.stride(1) != 2:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: uv pixel stride {uv.stride(1)} (2 expected)")
        ypitch = int(y.stride(0)) if h > 1 else w
        uvpitch = int(uv.stride(0)) if ch > 1 else 2 * cw
        if ypitch < w:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: y row pitch {ypitch} < {w}")
        if uvpitch < 2 * cw:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: uv row pitch {uvpitch} < 2 * {cw}")
        if y.device.type != "cuda" or uv.device.type != "cuda":
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: HIP kernel requires GPU tensors (got devices "
                               f"{y.device} / {uv.device}); no CPU fallback")
        if uv.device != y.device:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: y on {y.device}, uv on {uv.device}")
        if dev is None:
            dev = y.device
        elif y.device != dev:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i} on {y.device}, frame 0 on {dev}")
        nh, nw, top, left = (int(v) for v in g[:4])
        if nh < 1 or nw < 1 or top < 0 or left < 0 or top + nh > out_h or left + nw > out_w:
            raise RuntimeError(f"letterbox_ingest_nv12: frame {i}: geometry {tuple(g)} leaves the {out_h}x{out_w} "
                               "canvas")
        rows.append([y.data_ptr(), uv.data_ptr(), h, w, ypitch, uvpitch, nh, nw, top, left, (py << 1) | px,
                     NV12_MATRICES.index(f.matrix)])
    if out is None:
        out = torch.empty((B, 3, out_h, out_w), dtype=dtype, device=dev)
    elif (out.dtype != dtype or out.device != dev or tuple(out.shape) != (B, 3, out_h, out_w)
          or out.stride()[1:] != (out_h * out_w, out_w, 1) or out.stride(0) % 4 or out.stride(0) < 3 * out_h * out_w
          or out.data_ptr() % 16):
        raise RuntimeError(f"letterbox_ingest_nv12: out must be a {dtype} [{B}, 3, {out_h}, {out_w}] tensor on {dev} "
                           "with contiguous 16-byte aligned images and a batch stride that is a multiple of 4")
    desc = torch.tensor(rows, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    key = ("ingest_nv12", (B, 3, out_h, out_w), 2 if dtype == _BF16 else None)
    _check(_launch(key, dev, lib.yolosod_letterbox_ingest_nv12, desc.data_ptr(), B, out.data_ptr(), out.stride(0)
                   if B > 1 else 3 * out_h * out_w, out_h, out_w, int(dtype == _BF16), int(pad_value), _stream(dev)),
           "letterbox_ingest_nv12")
    return out


def scale_boxes_padded(out, counts, geom):
    """The padded NMS rows back to each frame's own pixels, in place and without a host sync (yolosod_scale_boxes):
    ``out`` [B, D, 6] fp32, ``counts`` [B] int32, ``geom`` [B, 5] fp32 = (gain, pad_x, pad_y, w0, h0) per image.
    Rows below the image's count get ``utils.ops.scale_boxes``'s arithmetic; the padding rows stay as they are."""
    lib = load_library()
    if out.dim() != 3 or out.shape[2] != 6:
        raise RuntimeError(f"scale_boxes_padded: out must be [B, D, 6], got {tuple(out.shape)}")
    B, D = int(out.shape[0]), int(out.shape[1])
    if tuple(counts.shape) != (B,) or tuple(geom.shape) != (B, 5):
        raise RuntimeError(f"scale_boxes_padded: counts {tuple(counts.shape)} / geom {tuple(geom.shape)} do not match "
                           f"{B} images")
    _check(_launch(("scale_boxes", (B, D, 6), None), out.device, lib.yolosod_scale_boxes, _dev(out, "out"),
                   _dev(counts, "counts", torch.int32), B, D, _dev(geom, "geom"), _stream(out.device)),
           "scale_boxes")
    return out


TILE_MERGE_MAX_NC = 64  # csrc/tile_merge.hip


def tile_merge(y, rows, merged, A, cut_margin=None):
    """Tile outputs into per-frame prediction tensors in frame pixels, one launch (yolosod_tile_merge): ``y``
    [n, 4+nc, A] fp32 is the Detect output of one model call on n tiles (canvas pixels), ``merged`` [F, 4+nc, S*A] fp32
    the batch's NMS input; ``rows`` names the destination slots this call writes, one
    ``(src, frame, slot, gain, pad_x, pad_y, off_x, off_y, tile_w, tile_h, (left, right, top, bottom))`` each
    (``SlicePlan.merge_rows``): ``src`` a row of y, or -1 for an empty slot (zeros); gain / pad as ``scale_boxes``
    computes them for the tile on the canvas; ``off`` the tile's x0, y0; the last entry says which tile edges are
    interior to the frame. ``cut_margin``: scores of boxes that come within this many tile pixels of an interior edge
    are zeroed (None or negative: off). Returns ``merged``.

    The descriptor is built here and goes up as one pinned non-blocking copy; everything the kernel relies on is
    checked here first: nothing is launched on arguments that fail."""
    lib = load_library()
    for t, name in ((y, "y"), (merged, "merged")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"tile_merge: {name}: expected a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"tile_merge: {name}: HIP kernel requires a GPU tensor (got device {t.device}); "
                               "no CPU fallback")
        if t.dtype != torch.float32:
            raise RuntimeError(f"tile_merge: {name}: expected float32, got {t.dtype}")
        if t.dim() != 3:
            raise RuntimeError(f"tile_merge: {name}: expected 3 dimensions, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"tile_merge: {name}: expected a contiguous tensor")
    if merged.device != y.device:
        raise RuntimeError(f"tile_merge: y on {y.device}, merged on {merged.device}")
    n, no, A = int(y.shape[0]), int(y.shape[1]), int(A)
    nc = no - 4
    if A < 1 or int(y.shape[2]) != A:
        raise RuntimeError(f"tile_merge: y has {int(y.shape[2])} anchors, A = {A}")
    if n < 1 or not 1 <= nc <= TILE_MERGE_MAX_NC:
        raise RuntimeError(f"tile_merge: y {tuple(y.shape)} unsupported (n >= 1, 1..{TILE_MERGE_MAX_NC} classes)")
    F, SA = int(merged.shape[0]), int(merged.shape[2])
    if F < 1 or int(merged.shape[1]) != no or SA < A or SA % A:
        raise RuntimeError(f"tile_merge: merged {tuple(merged.shape)} is not [F, {no}, S * {A}]")
    S = SA // A
    if S * A * nc >= 1 << 32:
        raise RuntimeError(f"tile_merge: S * A * nc = {S} * {A} * {nc} >= 2^32")
    desc = _tile_merge_desc("tile_merge", rows, n, F, S)
    cm = -1.0 if cut_margin is None else float(cut_margin)
    if cm != cm:
        raise RuntimeError("tile_merge: cut_margin is NaN")
    dev = y.device
    d = torch.from_numpy(desc).pin_memory().to(dev, non_blocking=True)
    _check(_launch(("tile_merge", (n, no, A), (F, S)), dev, lib.yolosod_tile_merge, y.data_ptr(), n, nc, A,
                   d.data_ptr(), len(desc), merged.data_ptr(), F, S, cm, _stream(dev)), "tile_merge")
    return merged


def _tile_merge_desc(who, rows, n, F, S):
    """The int32 [rows, 16] descriptor of ``tile_merge`` / ``tile_merge_tta`` from ``SlicePlan.merge_rows``' tuples, on
    the host; refuses a row that names something outside y [n, ...] or merged [F, ., S * .], or a slot twice."""
    import numpy as np
    rows = list(rows)
    if not 1 <= len(rows) <= 65535:
        raise RuntimeError(f"{who}: {len(rows)} descriptor rows (1..65535)")
    desc = np.zeros((len(rows), 16), dtype=np.int32)
    fl = desc.view(np.float32)
    named = set()
    for i, r in enumerate(rows):
        if len(r) != 11 or len(r[10]) != 4:
            raise RuntimeError(f"{who}: row {i}: expected (src, frame, slot, gain, pad_x, pad_y, off_x, off_y, "
                               "tile_w, tile_h, (left, right, top, bottom))")
        src, frame, slot = int(r[0]), int(r[1]), int(r[2])
        if not -1 <= src < n:
            raise RuntimeError(f"{who}: row {i}: src {src} outside [-1, {n})")
        if not 0 <= frame < F:
            raise RuntimeError(f"{who}: row {i}: frame {frame} outside [0, {F})")
        if not 0 <= slot < S:
            raise RuntimeError(f"{who}: row {i}: slot {slot} outside [0, {S})")
        if (frame, slot) in named:
            raise RuntimeError(f"{who}: row {i}: slot {slot} of frame {frame} is named twice")
        named.add((frame, slot))
        gain = float(r[3])
        if src >= 0 and not (gain > 0.0 and gain < float("inf")):
            raise RuntimeError(f"{who}: row {i}: gain {gain}")
        desc[i, :3] = (src, frame, slot)
        desc[i, 3] = sum(1 << k for k in range(4) if r[10][k])
        fl[i, 4:11] = [float(v) for v in r[3:10]]
    return desc


def tile_merge_tta(y, rows, merged, A_tot, branch, canvas_hw, cut_margin=None):
    """One branch of one augmented model call on tiles straight into the per-frame prediction tensors, one launch
    (yolosod_tile_merge_tta): ``y`` [n, 4+nc, A_k] fp32 is the Detect output of view ``branch`` of n tiles, in that
    view's canvas pixels; ``merged`` [F, 4+nc, S*A_tot] fp32 the batch's NMS input in frame pixels. ``branch`` is a
    ``data.tta.TTABranch`` or its five terms ``(src_lo, n, dst, scale, flip)``: anchors [src_lo, src_lo + n) of y go
    to anchors [slot*A_tot + dst, + n) of every slot that ``rows`` names (``SlicePlan.merge_rows``, as ``tile_merge``
    takes them; a ``src = -1`` row: zeros). ``canvas_hw`` = (h, w) of the tiles' canvas, what a flip mirrors in.
    Per anchor ``tta_merge``'s arithmetic, then ``tile_merge``'s on its result: bit for bit ``tta_merge`` into a
    concatenated tensor followed by ``tile_merge`` of it with A = A_tot, without that tensor. The K launches of one
    model call write every element of the named slots exactly once. Returns ``merged``.

    The descriptor is built here and goes up as one pinned non-blocking copy; everything the kernel relies on is
    checked here first: nothing is launched on arguments that fail. No host sync."""
    lib = load_library()
    for t, name in ((y, "y"), (merged, "merged")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"tile_merge_tta: {name}: expected a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"tile_merge_tta: {name}: HIP kernel requires a GPU tensor (got device {t.device}); "
                               "no CPU fallback")
        if t.dtype != torch.float32:
            raise RuntimeError(f"tile_merge_tta: {name}: expected float32, got {t.dtype}")
        if t.dim() != 3:
            raise RuntimeError(f"tile_merge_tta: {name}: expected 3 dimensions, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"tile_merge_tta: {name}: expected a contiguous tensor")
    if merged.device != y.device:
        raise RuntimeError(f"tile_merge_tta: y on {y.device}, merged on {merged.device}")
    n, no, A = (int(v) for v in y.shape)
    nc, A_tot = no - 4, int(A_tot)
    if n < 1 or A < 1 or not 1 <= nc <= TILE_MERGE_MAX_NC:
        raise RuntimeError(f"tile_merge_tta: y {tuple(y.shape)} unsupported (n >= 1, 1..{TILE_MERGE_MAX_NC} classes)")
    if A * no >= 1 << 31:
        raise RuntimeError("tile_merge_tta: A * (4 + nc) >= 2^31")
    F, SA = int(merged.shape[0]), int(merged.shape[2])
    if A_tot < 1 or F < 1 or int(merged.shape[1]) != no or SA < A_tot or SA % A_tot:
        raise RuntimeError(f"tile_merge_tta: merged {tuple(merged.shape)} is not [F, {no}, S * {A_tot}]")
    S = SA // A_tot
    if S * A_tot * nc >= 1 << 32:
        raise RuntimeError(f"tile_merge_tta: S * A_tot * nc = {S} * {A_tot} * {nc} >= 2^32")
    if hasattr(branch, "src_lo"):
        if int(branch.A) != A:
            raise RuntimeError(f"tile_merge_tta: y has {A} anchors, the branch {int(branch.A)}")
        branch = (branch.src_lo, branch.n, branch.dst, branch.scale, branch.flip)
    if len(branch) != 5:
        raise RuntimeError("tile_merge_tta: branch: expected a TTABranch or (src_lo, n, dst, scale, flip)")
    src_lo, n_k, dst, scale, flip = int(branch[0]), int(branch[1]), int(branch[2]), float(branch[3]), branch[4]
    if n_k < 1 or src_lo < 0 or src_lo + n_k > A:
        raise RuntimeError(f"tile_merge_tta: source anchors [{src_lo}, {src_lo + n_k}) leave y's {A}")
    if dst < 0 or dst + n_k > A_tot:
        raise RuntimeError(f"tile_merge_tta: destination anchors [{dst}, {dst + n_k}) leave a slot's {A_tot}")
    if not (scale > 0.0 and scale < float("inf")):
        raise RuntimeError(f"tile_merge_tta: scale {scale} (finite and > 0 expected)")
    if flip not in TTA_FLIPS:
        raise RuntimeError(f"tile_merge_tta: flip {flip} (None, 2 or 3)")
    img_h, img_w = int(canvas_hw[0]), int(canvas_hw[1])
    desc = _tile_merge_desc("tile_merge_tta", rows, n, F, S)
    cm = -1.0 if cut_margin is None else float(cut_margin)
    if cm != cm:
        raise RuntimeError("tile_merge_tta: cut_margin is NaN")
    dev = y.device
    d = torch.from_numpy(desc).pin_memory().to(dev, non_blocking=True)
    _check(_launch(("tile_merge_tta", (n, no, n_k), (F, S, A_tot)), dev, lib.yolosod_tile_merge_tta, y.data_ptr(), n,
                   nc, A, src_lo, n_k, d.data_ptr(), len(desc), merged.data_ptr(), F, S, A_tot, dst, scale,
                   TTA_FLIPS[flip], float(img_w), float(img_h), cm, _stream(dev)), "tile_merge_tta")
    return merged


TTA_MAX_DIM = 16384  # extents of csrc/tta.hip
TTA_MAX_NC = 64
TTA_FLIPS = {None: 0, 0: 0, 2: 2, 3: 3}  # the reference's codes: 2 up-down, 3 left-right


def tta_views(x, views, outs=None, cache=None):
    """Every scaled / flipped view of a batch in one launch (torch.ops.yolosod.tta_views, yolosod_tta_views): ``x``
    [B, C, H, W] contiguous, float32 or bfloat16, on the GPU; ``views`` a sequence of ``(flip, sh, sw, ph, pw)``
    (``TTAPlan.views``): flip None / 2 (up-down) / 3 (left-right), the resized size and the padded size (pw % 4 == 0).
    Returns the list of views, [B, C, ph, pw] each in x's dtype: x flipped and resized (bilinear, csrc/tta.hip) at the
    top-left, 0.447 elsewhere. ``outs``: write into these tensors instead (contiguous, 16-byte aligned); otherwise all
    views are carved from one allocation. ``cache``: a dict that keeps the uploaded descriptor table per output
    addresses (the caching allocator hands a steady-state loop the same block: no upload then).

    The table the kernel reads is built here from the tensors' own ``data_ptr()`` and goes up as one pinned
    non-blocking copy; everything the kernel relies on is checked here first: nothing is launched on arguments that
    fail."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("tta_views: x: expected a tensor")
    if x.device.type != "cuda":
        raise RuntimeError(f"tta_views: x: HIP kernel requires GPU tensors (got device {x.device}); no CPU fallback")
    if x.dtype not in (torch.float32, _BF16):
        raise RuntimeError(f"tta_views: x must be float32 or bfloat16, got {x.dtype}")
    if x.dim() != 4:
        raise RuntimeError(f"tta_views: x: expected [B, C, H, W], got shape {tuple(x.shape)}")
    if not x.is_contiguous():
        raise RuntimeError("tta_views: x: expected a contiguous tensor")
    B, C, H, W = (int(v) for v in x.shape)
    if B < 1 or C < 1 or not (0 < H <= TTA_MAX_DIM and 0 < W <= TTA_MAX_DIM):
        raise RuntimeError(f"tta_views: x {tuple(x.shape)} unsupported (extents 1..{TTA_MAX_DIM})")
    views = list(views)
    V = len(views)
    if V < 1 or V * B * C > 65535:
        raise RuntimeError(f"tta_views: {V} views of {B} x {C} planes (1 <= views * B * C <= 65535)")
    geom = []
    for i, v in enumerate(views):
        if len(v) != 5 or v[0] not in TTA_FLIPS:
            raise RuntimeError(f"tta_views: view {i}: expected (flip None / 2 / 3, sh, sw, ph, pw), got {tuple(v)}")
        sh, sw, ph, pw = (int(k) for k in v[1:])
        if pw % 4:
            raise RuntimeError(f"tta_views: view {i}: padded width {pw} is no multiple of 4")
        if not (1 <= sh <= ph <= TTA_MAX_DIM and 1 <= sw <= pw <= TTA_MAX_DIM):
            raise RuntimeError(f"tta_views: view {i}: {sh}x{sw} in {ph}x{pw} unsupported (1 <= resized <= padded <= "
                               f"{TTA_MAX_DIM})")
        geom.append((TTA_FLIPS[v[0]], sh, sw, ph, pw))
    dev = x.device
    if outs is None:
        item = x.element_size()
        sizes = [(B * C * g[3] * g[4] * item + 15) // 16 * 16 for g in geom]
        buf = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
        outs, o = [], 0
        for g, n in zip(geom, sizes):
            outs.append(buf[o:o + B * C * g[3] * g[4] * item].view(x.dtype).view(B, C, g[3], g[4]))
            o += n
    else:
        outs = list(outs)
        if len(outs) != V:
            raise RuntimeError(f"tta_views: {len(outs)} outputs for {V} views")
        for i, (t, g) in enumerate(zip(outs, geom)):
            if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != x.dtype
                    or tuple(t.shape) != (B, C, g[3], g[4]) or not t.is_contiguous() or t.data_ptr() % 16):
                raise RuntimeError(f"tta_views: view {i}: out must be a contiguous 16-byte aligned {x.dtype} "
                                   f"[{B}, {C}, {g[3]}, {g[4]}] tensor on {dev}")
    key = (str(dev), tuple(t.data_ptr() for t in outs), tuple(geom))
    desc = None if cache is None else cache.get(key)
    if desc is None:
        rows = [[t.data_ptr(), *g, 0, 0] for t, g in zip(outs, geom)]
        desc = torch.tensor(rows, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        if cache is not None:
            if len(cache) >= 64:
                cache.clear()
            cache[key] = desc
    _launch(("tta_views", tuple(x.shape), tuple(geom)) + ((2,) if x.dtype == _BF16 else ()), dev, ops().tta_views, x,
            desc, outs, [k for g in geom for k in g])
    return outs


def tta_merge(y, cat, src_lo, n, dst, scale, flip, img_hw):
    """One branch of augmented inference into the concatenated prediction tensor, one launch
    (torch.ops.yolosod.tta_merge, yolosod_tta_merge; the reference's ``_descale_pred`` + ``_clip_augmented`` +
    ``torch.cat``): anchors [src_lo, src_lo + n) of ``y`` [B, 4+nc, A] fp32 (the head's output for the view) become
    anchors [dst, dst + n) of ``cat`` [B, 4+nc, A_tot] fp32: xywh / float32(scale), then x = img_w - x (flip 3) or
    y = img_h - y (flip 2); scores are copied. Nothing else of ``cat`` is touched. Returns ``cat``. Everything the
    kernel relies on is checked here first: nothing is launched on arguments that fail."""
    for t, name in ((y, "y"), (cat, "cat")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"tta_merge: {name}: expected a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"tta_merge: {name}: HIP kernel requires GPU tensors (got device {t.device}); "
                               "no CPU fallback")
        if t.dtype != torch.float32:
            raise RuntimeError(f"tta_merge: {name}: expected float32, got {t.dtype}")
        if t.dim() != 3:
            raise RuntimeError(f"tta_merge: {name}: expected 3 dimensions, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"tta_merge: {name}: expected a contiguous tensor")
    if cat.device != y.device:
        raise RuntimeError(f"tta_merge: y on {y.device}, cat on {cat.device}")
    B, no, A = (int(v) for v in y.shape)
    nc = no - 4
    if B < 1 or B > 65535 or A < 1 or not 1 <= nc <= TTA_MAX_NC:
        raise RuntimeError(f"tta_merge: y {tuple(y.shape)} unsupported (B 1..65535, 1..{TTA_MAX_NC} classes)")
    A_tot = int(cat.shape[2])
    if int(cat.shape[0]) != B or int(cat.shape[1]) != no:
        raise RuntimeError(f"tta_merge: cat {tuple(cat.shape)} is not [{B}, {no}, A_tot]")
    if max(A, A_tot) * no >= 1 << 31:
        raise RuntimeError(f"tta_merge: A * (4 + nc) >= 2^31")
    src_lo, n, dst = int(src_lo), int(n), int(dst)
    if n < 1 or src_lo < 0 or src_lo + n > A:
        raise RuntimeError(f"tta_merge: source anchors [{src_lo}, {src_lo + n}) leave y's {A}")
    if dst < 0 or dst + n > A_tot:
        raise RuntimeError(f"tta_merge: destination anchors [{dst}, {dst + n}) leave cat's {A_tot}")
    scale = float(scale)
    if not (scale > 0.0 and scale < float("inf")):
        raise RuntimeError(f"tta_merge: scale {scale} (finite and > 0 expected)")
    if flip not in TTA_FLIPS:
        raise RuntimeError(f"tta_merge: flip {flip} (None, 2 or 3)")
    img_h, img_w = int(img_hw[0]), int(img_hw[1])
    _launch(("tta_merge", (B, no, n), (A, A_tot)), y.device, ops().tta_merge, y, cat, src_lo, n, dst, scale,
            TTA_FLIPS[flip], img_h, img_w)
    return cat


EVAL_MATCH_LABEL_CHUNK = 256  # labels staged through LDS per pass (csrc/eval_match.hip ematch::CHUNK)
EVAL_MATCH_MAX_D = 1024       # detection rows per image (one lane each)
EVAL_MATCH_MAX_T = 16         # IoU thresholds (by value in the kernel arguments)


def match_predictions(out, counts, labels, label_off, iouv=IOU_THRESHOLDS):
    """The true-positive matrix of a batch of padded NMS rows against its labels, one launch and no host sync
    (yolosod_match_predictions, the reference's ``match_predictions`` over ``box_iou``): ``out`` [B, D, 6] fp32 and
    ``counts`` [B] int32 as ``non_max_suppression_padded`` / ``predict_padded`` return them, ``labels`` [L, 5] fp32 =
    (cls, x1, y1, x2, y2) of all images back to back in the boxes' own space, ``label_off`` [B + 1] int32 with image b
    owning labels [label_off[b], label_off[b + 1]) (``engine.validator.pack_labels`` builds both), ``iouv`` the T
    thresholds on the host (a CPU tensor, an array or a sequence; 1..16 finite values > 0). Returns tp, uint8
    [B, D, T] on ``out``'s device: rows >= counts[b] are 0.

    ``label_off`` is read on the device (reading it here would sync), so that it stays inside ``labels`` is the
    caller's word; everything else the kernel relies on is checked here first: nothing is launched on arguments that
    fail."""
    import numpy as np
    lib = load_library()
    for t, name, dtype, dim in ((out, "out", torch.float32, 3), (counts, "counts", torch.int32, 1),
                                (labels, "labels", torch.float32, 2), (label_off, "label_off", torch.int32, 1)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"match_predictions: {name}: expected a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"match_predictions: {name}: HIP kernel requires a GPU tensor (got device {t.device}); "
                               "no CPU fallback")
        if t.dtype != dtype:
            raise RuntimeError(f"match_predictions: {name}: expected {dtype}, got {t.dtype}")
        if t.dim() != dim:
            raise RuntimeError(f"match_predictions: {name}: expected {dim} dimensions, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"match_predictions: {name}: expected a contiguous tensor")
        if t.device != out.device:
            raise RuntimeError(f"match_predictions: out on {out.device}, {name} on {t.device}")
    B, D = int(out.shape[0]), int(out.shape[1])
    if B < 1 or not 1 <= D <= EVAL_MATCH_MAX_D or int(out.shape[2]) != 6:
        raise RuntimeError(f"match_predictions: out {tuple(out.shape)} unsupported ([B >= 1, 1..{EVAL_MATCH_MAX_D}, 6])")
    if tuple(counts.shape) != (B,) or tuple(label_off.shape) != (B + 1,):
        raise RuntimeError(f"match_predictions: counts {tuple(counts.shape)} / label_off {tuple(label_off.shape)} do "
                           f"not match {B} images ([{B}] and [{B + 1}] expected)")
    if int(labels.shape[1]) != 5:
        raise RuntimeError(f"match_predictions: labels {tuple(labels.shape)} is not [L, 5] (cls, x1, y1, x2, y2)")
    if isinstance(iouv, torch.Tensor):
        if iouv.device.type != "cpu":
            raise RuntimeError(f"match_predictions: iouv lives on the host (got device {iouv.device})")
        iouv = iouv.detach().numpy()
    thr = np.ascontiguousarray(np.asarray(iouv, dtype=np.float32).reshape(-1))
    T = int(thr.size)
    if not 1 <= T <= EVAL_MATCH_MAX_T:
        raise RuntimeError(f"match_predictions: {T} thresholds (1..{EVAL_MATCH_MAX_T})")
    if not (np.isfinite(thr).all() and (thr > 0).all()):
        raise RuntimeError(f"match_predictions: thresholds {thr.tolist()} (finite and > 0 expected)")
    dev = out.device
    tp = torch.empty((B, D, T), dtype=torch.uint8, device=dev)
    _check(_launch(("match_predictions", (B, D, T), int(labels.shape[0])), dev, lib.yolosod_match_predictions,
                   out.data_ptr(), counts.data_ptr(), B, D, labels.data_ptr() if labels.shape[0] else None,
                   label_off.data_ptr(), thr.ctypes.data, T, tp.data_ptr(), _stream(dev)), "match_predictions")
    return tp


EVAL_CONFUSION_LABEL_CHUNK = 256  # labels staged through LDS per pass (csrc/eval_confusion.hip econf::CHUNK)
EVAL_CONFUSION_MAX_D = 1024       # detection rows per image (one lane each)
EVAL_CONFUSION_MAX_NC = 100       # classes: the workgroup's LDS matrix is (MAX_NC + 1)^2 int32


def confusion_matrix(out, counts, labels, label_off, nc, conf=0.25, iou_thres=0.45):
    """The confusion matrices of a batch of padded NMS rows against its labels, one launch and no host sync
    (yolosod_confusion_matrix, the reference's ``ConfusionMatrix.process_batch`` over ``box_iou``): ``out``, ``counts``,
    ``labels`` and ``label_off`` as for :func:`match_predictions`, ``nc`` the number of classes (1..100), ``conf`` and
    ``iou_thres`` the two thresholds as the kernel compares them, in fp32 and strictly (finite and >= 0; the
    ``{None, 0.001} -> 0.25`` rule belongs to ``utils.metrics.ConfusionMatrix``). Returns cm, int32 [B, nc + 1, nc + 1]
    on ``out``'s device: per image, rows the predicted class, columns the true class, index ``nc`` the background.
    Rows and labels whose class is NaN or truncates outside [0, nc) are counted nowhere.

    ``label_off`` is read on the device, so that it stays inside ``labels`` is the caller's word; everything else the
    kernel relies on is checked here first: nothing is launched on arguments that fail."""
    import math
    lib = load_library()
    for t, name, dtype, dim in ((out, "out", torch.float32, 3), (counts, "counts", torch.int32, 1),
                                (labels, "labels", torch.float32, 2), (label_off, "label_off", torch.int32, 1)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"confusion_matrix: {name}: expected a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"confusion_matrix: {name}: HIP kernel requires a GPU tensor (got device {t.device}); "
                               "no CPU fallback")
        if t.dtype != dtype:
            raise RuntimeError(f"confusion_matrix: {name}: expected {dtype}, got {t.dtype}")
        if t.dim() != dim:
            raise RuntimeError(f"confusion_matrix: {name}: expected {dim} dimensions, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"confusion_matrix: {name}: expected a contiguous tensor")
        if t.device != out.device:
            raise RuntimeError(f"confusion_matrix: out on {out.device}, {name} on {t.device}")
    B, D = int(out.shape[0]), int(out.shape[1])
    if B < 1 or not 1 <= D <= EVAL_CONFUSION_MAX_D or int(out.shape[2]) != 6:
        raise RuntimeError(f"confusion_matrix: out {tuple(out.shape)} unsupported "
                           f"([B >= 1, 1..{EVAL_CONFUSION_MAX_D}, 6])")
    if tuple(counts.shape) != (B,) or tuple(label_off.shape) != (B + 1,):
        raise RuntimeError(f"confusion_matrix: counts {tuple(counts.shape)} / label_off {tuple(label_off.shape)} do "
                           f"not match {B} images ([{B}] and [{B + 1}] expected)")
    if int(labels.shape[1]) != 5:
        raise RuntimeError(f"confusion_matrix: labels {tuple(labels.shape)} is not [L, 5] (cls, x1, y1, x2, y2)")
    if isinstance(nc, bool) or not isinstance(nc, int) or not 1 <= nc <= EVAL_CONFUSION_MAX_NC:
        raise RuntimeError(f"confusion_matrix: nc {nc!r} unsupported (an int in 1..{EVAL_CONFUSION_MAX_NC})")
    conf, iou_thres = float(conf), float(iou_thres)
    for v, name in ((conf, "conf"), (iou_thres, "iou_thres")):
        if not (math.isfinite(v) and 0.0 <= v <= 3.4028234663852886e38):
            raise RuntimeError(f"confusion_matrix: {name} {v} (finite and >= 0 expected)")
    dev = out.device
    cm = torch.empty((B, nc + 1, nc + 1), dtype=torch.int32, device=dev)
    _check(_launch(("confusion_matrix", (B, D, nc), int(labels.shape[0])), dev, lib.yolosod_confusion_matrix,
                   out.data_ptr(), counts.data_ptr(), B, D, labels.data_ptr() if labels.shape[0] else None,
                   label_off.data_ptr(), nc, conf, iou_thres, cm.data_ptr(), _stream(dev)), "confusion_matrix")
    return cm


TRACK_MAX_T = 1024  # track slots per stream: a multiple of 64 in 64..1024 (csrc/track.hip trk::MAXN)
TRACK_MAX_D = 1024  # detection rows per stream and frame


def track_state_bytes(T: int) -> int:
    """Bytes of one stream's tracker state for ``T`` slots (yolosod_track_state_bytes)."""
    return int(load_library().yolosod_track_state_bytes(int(T)))


def _track_state_check(what, state, T):
    if not isinstance(state, torch.Tensor):
        raise TypeError(f"{what}: state: expected a tensor")
    if state.device.type != "cuda":
        raise RuntimeError(f"{what}: state: HIP kernel requires a GPU tensor (got device {state.device}); "
                           "no CPU fallback")
    if state.dtype != torch.uint8:
        raise RuntimeError(f"{what}: state: expected {torch.uint8}, got {state.dtype}")
    if state.dim() != 2:
        raise RuntimeError(f"{what}: state: expected 2 dimensions, got shape {tuple(state.shape)}")
    if not state.is_contiguous():
        raise RuntimeError(f"{what}: state: expected a contiguous tensor")
    if isinstance(T, bool) or not isinstance(T, int) or not 64 <= T <= TRACK_MAX_T or T % 64:
        raise RuntimeError(f"{what}: T {T!r} unsupported (a multiple of 64 in 64..{TRACK_MAX_T})")
    B = int(state.shape[0])
    if B < 1 or int(state.shape[1]) != track_state_bytes(T):
        raise RuntimeError(f"{what}: state {tuple(state.shape)} is not [B >= 1, {track_state_bytes(T)}] for T = {T}")
    return B


def track_reset(state, T, streams=None):
    """Zero the tracker state of the listed streams (``streams``: an int32 device tensor, or None for all) and start
    their ids at 1 (yolosod_track_reset); one launch, no host sync. ``state`` is uint8 [B, track_state_bytes(T)]."""
    lib = load_library()
    B = _track_state_check("track_reset", state, T)
    n, sp = 0, None
    if streams is not None:
        if not isinstance(streams, torch.Tensor):
            raise TypeError("track_reset: streams: expected a tensor")
        if streams.device != state.device:
            raise RuntimeError(f"track_reset: state on {state.device}, streams on {streams.device}")
        if streams.dtype != torch.int32:
            raise RuntimeError(f"track_reset: streams: expected {torch.int32}, got {streams.dtype}")
        if streams.dim() != 1 or not streams.is_contiguous() or int(streams.shape[0]) > B:
            raise RuntimeError(f"track_reset: streams {tuple(streams.shape)} is not a contiguous list of at most {B}")
        n, sp = int(streams.shape[0]), streams.data_ptr()
        if n == 0:
            return
    dev = state.device
    _check(_launch(("track_reset", (B, T), n), dev, lib.yolosod_track_reset, state.data_ptr(), B, T, sp, n,
                   _stream(dev)), "track_reset")


TRACK_MODELS = {"xyah": 0, "xywh": 1}  # the filter's model: ByteTrack, BoT-SORT (csrc/track.hip trk::XYAH / XYWH)


def track_update(state, T, out, counts, params, tracks=None, n_tracks=None, workspace=None, model="xyah", warps=None):
    """One ByteTrack update of every stream, one launch and no host sync (yolosod_track_update; the reference's
    ``BYTETracker.update`` per stream). With ``model="xywh"`` it is BoT-SORT's update
    (yolosod_track_update_ex): the XYWH filter and, if ``warps`` (fp64 [B, 2, 3] on the device, one
    camera-motion matrix per stream) is given, the warp of every pool and unconfirmed track before the first
    association; a stream whose warp has a non-finite entry skips it and counts it (``bad_warp``).

    ``state`` uint8 [B, track_state_bytes(T)] (reset once with :func:`track_reset`), ``out`` fp32 [B, D, 6] and
    ``counts`` int32 [B] the padded NMS rows of each stream's next frame, ``params`` a host sequence of 8 floats
    (``utils.bytetrack.params_vector``). Returns (tracks fp32 [B, T, 8] = x1, y1, x2, y2, track_id, score, cls, idx,
    ascending track_id, zero padded; n_tracks int32 [B]) on ``out``'s device; ``tracks`` / ``n_tracks`` /
    ``workspace`` may be passed in to be reused.

    Everything the kernel relies on is checked here first: nothing is launched on arguments that fail."""
    import math

    import numpy as np
    lib = load_library()
    B = _track_state_check("track_update", state, T)
    if model not in TRACK_MODELS:
        raise RuntimeError(f"track_update: model {model!r} unknown ({sorted(TRACK_MODELS)})")
    if warps is not None and model != "xywh":
        raise RuntimeError("track_update: warps with model 'xyah' (ByteTrack has no camera-motion step)")
    checked = [(out, "out", torch.float32, 3), (counts, "counts", torch.int32, 1)]
    if warps is not None:
        checked.append((warps, "warps", torch.float64, 3))
    for t, name, dtype, dim in checked:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"track_update: {name}: expected a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"track_update: {name}: HIP kernel requires a GPU tensor (got device {t.device}); "
                               "no CPU fallback")
        if t.dtype != dtype:
            raise RuntimeError(f"track_update: {name}: expected {dtype}, got {t.dtype}")
        if t.dim() != dim:
            raise RuntimeError(f"track_update: {name}: expected {dim} dimensions, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"track_update: {name}: expected a contiguous tensor")
        if t.device != state.device:
            raise RuntimeError(f"track_update: state on {state.device}, {name} on {t.device}")
    D = int(out.shape[1])
    if int(out.shape[0]) != B or not 1 <= D <= TRACK_MAX_D or int(out.shape[2]) != 6:
        raise RuntimeError(f"track_update: out {tuple(out.shape)} unsupported ([{B}, 1..{TRACK_MAX_D}, 6] for "
                           f"{B} streams)")
    if tuple(counts.shape) != (B,):
        raise RuntimeError(f"track_update: counts {tuple(counts.shape)} does not match {B} streams ([{B}] expected)")
    if warps is not None and tuple(warps.shape) != (B, 2, 3):
        raise RuntimeError(f"track_update: warps {tuple(warps.shape)} does not match {B} streams ([{B}, 2, 3] expected)")
    prm = np.ascontiguousarray(params, dtype=np.float32)
    if prm.shape != (8,) or not all(math.isfinite(float(v)) and float(v) >= 0.0 for v in prm):
        raise RuntimeError(f"track_update: params {prm!r} (8 finite values >= 0 expected)")
    dev = state.device
    if tracks is None:
        tracks = torch.empty((B, T, 8), dtype=torch.float32, device=dev)
    if n_tracks is None:
        n_tracks = torch.empty((B,), dtype=torch.int32, device=dev)
    need = int(lib.yolosod_track_workspace(B, T, D))
    if workspace is None:
        workspace = _workspace(need, dev)
    for t, name, dtype, shape in ((tracks, "tracks", torch.float32, (B, T, 8)),
                                  (n_tracks, "n_tracks", torch.int32, (B,)),
                                  (workspace, "workspace", torch.uint8, None)):
        if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or not t.is_contiguous()
                or (shape is not None and tuple(t.shape) != shape)):
            raise RuntimeError(f"track_update: {name}: expected a contiguous {dtype} tensor"
                               + (f" {list(shape)}" if shape else "") + f" on {dev}")
    if workspace.numel() < need:
        raise RuntimeError(f"track_update: workspace of {workspace.numel()} bytes, {need} needed")
    if model == "xyah":
        _check(_launch(("track_update", (B, T, D), 0), dev, lib.yolosod_track_update, state.data_ptr(), B, T,
                       out.data_ptr(), counts.data_ptr(), D, prm.ctypes.data, tracks.data_ptr(), n_tracks.data_ptr(),
                       workspace.data_ptr(), workspace.numel(), _stream(dev)), "track_update")
    else:
        _check(_launch(("track_update", (B, T, D), 1 + (warps is not None)), dev, lib.yolosod_track_update_ex,
                       state.data_ptr(), B, T, out.data_ptr(), counts.data_ptr(), D, prm.ctypes.data,
                       TRACK_MODELS[model], None if warps is None else warps.data_ptr(), tracks.data_ptr(),
                       n_tracks.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(dev)), "track_update")
    return tracks, n_tracks


def track_last_launch() -> dict:
    """Host-side facts of the last :func:`track_update` launch of this thread (yolosod_debug_track_last): T, D, B, the
    workspace layout (1: boxes and the [T, D] fp32 cost matrix per stream), lanes per workgroup, workspace bytes per
    stream; all 0 before the first launch. ``model`` (0 XYAH, 1 XYWH) and ``warps`` (0 / 1: whether warps were given)
    of that launch are :func:`track_last_model`'s: this dict keeps its six keys."""
    lib = load_library()
    return {k: int(lib.yolosod_debug_track_last(i))
            for i, k in enumerate(("T", "D", "B", "layout", "lanes", "workspace_per_stream"))}


def track_last_model() -> dict:
    """``model`` (0 XYAH, 1 XYWH) and ``warps`` (0 / 1) of this thread's last track_update launch
    (yolosod_debug_track_last indices 6 and 7)."""
    lib = load_library()
    return dict(model=int(lib.yolosod_debug_track_last(6)), warps=int(lib.yolosod_debug_track_last(7)))


def track_state_fetch(state, T) -> list:
    """Debug fetch (a host sync): the tracker state parsed per stream into numpy arrays - ``frame``, ``next_id``,
    ``overflow``, ``bad_warp`` and per slot ``state`` (0 free, 1 Tracked, 2 Lost, 3 Removed but listed as lost), ``flags`` (1
    activated, 2 the id was removed once), ``tid``, ``start``, ``last``, ``idx``, ``score``, ``cls``, ``mean`` [T, 8]
    and ``cov`` [T, 8, 8] (fp64) - plus ``raw``, the stream's bytes."""
    import numpy as np
    B = _track_state_check("track_state_fetch", state, T)
    raw = state.cpu().numpy()
    res = []
    for b in range(B):
        r = np.ascontiguousarray(raw[b])
        hdr = r[:64].view(np.int32)
        o = 64
        mean = r[o:o + 64 * T].view(np.float64).reshape(8, T).T.copy()
        o += 64 * T
        cov = r[o:o + 512 * T].view(np.float64).reshape(8, 8, T).transpose(2, 0, 1).copy()
        o += 512 * T
        d = dict(frame=int(hdr[0]), next_id=int(hdr[1]), overflow=int(hdr[2]), bad_warp=int(hdr[3]), mean=mean, cov=cov,
                 raw=r)
        for name, dt in (("state", np.int32), ("flags", np.int32), ("tid", np.int32), ("start", np.int32),
                         ("last", np.int32), ("idx", np.int32), ("score", np.float32), ("cls", np.float32)):
            d[name] = r[o:o + 4 * T].view(dt).copy()
            o += 4 * T
        res.append(d)
    return res


def gemm_f32(A, B, b_kcontig, bias=None, bias_mode=0, act=0, res=None):
    """Test hook: A [M,K]; B [N,K] (b_kcontig) or [K,N]; returns C [M,N]."""
    lib = load_library()
    M, K = A.shape
    N = B.shape[0] if b_kcontig else B.shape[1]
    C = torch.empty((M, N), dtype=torch.float32, device=A.device)
    _check(_launch(("gemm", (M, N, K), None), A.device, lib.yolosod_gemm_f32, _dev(A, "A"), 0, K, _dev(B, "B"), 0, B.shape[1], int(b_kcontig), _dev(C, "C"), 0, N,
                                M, N, K, 1, None if bias is None else _dev(bias, "bias"), bias_mode, act,
                                None if res is None else _dev(res, "res"), _stream(A.device)), "gemm_f32")
    return C


def layernorm(x, w, b, eps):
    lib = load_library()
    rows, C = x.shape
    y = torch.empty_like(x)
    _check(_launch(("layernorm", (rows, C), None), x.device, lib.yolosod_layernorm, _dev(x, "x"), _dev(y, "y"), rows, C, _dev(w, "w"), _dev(b, "b"), float(eps),
                                 _stream(x.device)), "layernorm")
    return y


def attention(qkv, n_seq, L, C, heads):
    lib = load_library()
    out = torch.empty((n_seq * L, C), dtype=torch.float32, device=qkv.device)
    _check(_launch(("attention", (n_seq, L, C), heads), qkv.device, lib.yolosod_attention, _dev(qkv, "qkv"), _dev(out, "out"), n_seq, L, C, heads, _stream(qkv.device)), "attention")
    return out


def gemm_bf16(A, B, b_kcontig, bias=None, bias_mode=0, act=0, res=None, batch=None):
    """Test hook: A [M,K] bf16; B [N,K] (b_kcontig) or [K,N] bf16; returns C [M,N] bf16 (fp32 accumulation).
    ``batch``: B [batch,N,K] / [batch,K,N] and res [batch,M,N] with batch strides b_bs / c_bs, A either shared [M,K]
    (a_bs = 0, as A2_Attn's weight) or [batch,M,K]; returns C [batch,M,N]. bias_mode 1: bias [M], 2: bias [N]."""
    lib = load_library()
    M, K = A.shape[-2:]
    nb = 1 if batch is None else int(batch)
    Bm = B.shape[-2:]
    N = Bm[0] if b_kcontig else Bm[1]
    if batch is not None and (B.dim() != 3 or B.shape[0] != nb or A.dim() not in (2, 3)
                              or (A.dim() == 3 and A.shape[0] != nb) or (res is not None and res.shape != (nb, M, N))):
        raise RuntimeError("gemm_bf16: batched operands must be [batch, ...]")
    C = torch.empty((M, N) if batch is None else (nb, M, N), dtype=_BF16, device=A.device)
    a_bs = M * K if A.dim() == 3 else 0
    b_bs, c_bs = (0, 0) if batch is None else (Bm[0] * Bm[1], M * N)
    _check(_launch(("gemm_bf16", (M, N, K), None if batch is None else nb), A.device, lib.yolosod_gemm_bf16,
                   _dev(A, "A", _BF16), a_bs, K, _dev(B, "B", _BF16), b_bs, Bm[1], int(b_kcontig), _dev(C, "C", _BF16),
                   c_bs, N, M, N, K, nb, None if bias is None else _dev(bias, "bias"), bias_mode, act,
                   None if res is None else _dev(res, "res", _BF16), _stream(A.device)), "gemm_bf16")
    return C


def gemm_bf16_tile(M, N, batch=1) -> int:
    """The N extent (64 or 128) of the tile the bf16 GEMM takes for (M, N, batch) (yolosod_debug_gemm_bf16_tile)."""
    return int(load_library().yolosod_debug_gemm_bf16_tile(int(M), int(N), int(batch)))


def gemm_bf16_last_tile():
    """The tile of the last bf16 GEMM launch of this process (None: none yet)."""
    r = int(load_library().yolosod_debug_gemm_bf16_last_tile())
    return None if r < 0 else r


def gemm_bf16_launches() -> dict:
    """bf16 GEMM launches of this process per tile: {64: n, 128: n}."""
    lib = load_library()
    return {t: int(lib.yolosod_debug_gemm_bf16_launches(t)) for t in (64, 128)}


SWIN_BF16_ROUTES = ("decomposed_tok2", "decomposed_tokln", "fused_2byte", "fused_chunked")


def swin_bf16_route(B, C, num_heads, H, W, window, hid):
    """What the bf16 SwinBlock runs for this shape under the current switches (yolosod_debug_swin_bf16_route, host
    only): one of SWIN_BF16_ROUTES, or None for a shape it refuses."""
    r = int(load_library().yolosod_debug_swin_bf16_route(int(B), int(C), int(num_heads), int(H), int(W), int(window),
                                                         int(hid)))
    return None if r < 0 else SWIN_BF16_ROUTES[r]


def swin_bf16_last_route():
    """The route of the last bf16 SwinBlock launch of this process (None: none yet)."""
    r = int(load_library().yolosod_debug_swin_bf16_last_route())
    return None if r < 0 else SWIN_BF16_ROUTES[r]


def attention_bf16_form(L, C, heads):
    """(head dim, key blocks) of the bf16 attention kernel instance for sequences of L tokens, None if refused."""
    r = int(load_library().yolosod_debug_attention_bf16_form(int(L), int(C), int(heads)))
    return None if r < 0 else divmod(r, 100)


def attention_bf16_last_form():
    """(head dim, key blocks) of the last bf16 attention launch of this process (None: none yet)."""
    r = int(load_library().yolosod_debug_attention_bf16_last_form())
    return None if r < 0 else divmod(r, 100)


def attention_bf16(qkv, n_seq, L, C, heads):
    """Test hook: bf16 attention over n_seq contiguous sequences of L rows of qkv [n_seq*L, 3C] -> [n_seq*L, C]."""
    lib = load_library()
    out = torch.empty((n_seq * L, C), dtype=_BF16, device=qkv.device)
    _check(_launch(("attention_bf16", (n_seq, L, C), heads), qkv.device, lib.yolosod_attention_bf16,
                   _dev(qkv, "qkv", _BF16), _dev(out, "out", _BF16), n_seq, L, C, heads, _stream(qkv.device)),
           "attention_bf16")
    return out
