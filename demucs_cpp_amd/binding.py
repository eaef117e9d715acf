"""ctypes binding of the C ABI in include/demucs_hip.h (libdemucs_hip.so, built in-tree
by `make` / __graft_entry__.build()).

This module is plumbing for tests and bench.py; the product is the shared library.
There is deliberately NO fallback: if the library is missing, or no GPU is usable, the
calls raise.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("DMX_LIB", os.path.join(ROOT, "demucs_cpp_amd", "lib", "libdemucs_hip.so"))

LAYOUT_EIGEN = 0
LAYOUT_PLANAR = 1
SEGMENT_SAMPLES = 343980
MAX_SHIFT = 22050
MAX_BAG = 8  # include/demucs_hip.h DMX_MAX_BAG (and n_models * n_shifts <= 256)

# every symbol include/demucs_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "dmx_last_error", "dmx_device_count", "dmx_model_load", "dmx_model_free", "dmx_model_n_sources",
    "dmx_model_n_tensors", "dmx_model_device", "dmx_ctx_create", "dmx_ctx_free", "dmx_ctx_segment_samples",
    "dmx_ctx_max_batch", "dmx_ctx_arena_bytes", "dmx_ctx_synchronize", "dmx_ctx_set_stream", "dmx_segment_infer",
    "dmx_segment_infer_device", "dmx_track_infer", "dmx_track_geometry", "dmx_track_stats_device",
    "dmx_track_gather_device", "dmx_track_overlap_add_device", "dmx_debug_tap", "dmx_debug_n_ops",
    "dmx_debug_profile", "dmx_ctx_set_model", "dmx_model_clone",
    "dmx_debug_plan_info", "dmx_debug_op_info", "dmx_debug_arena_fill", "dmx_debug_arena_io", "dmx_debug_run_op", "dmx_debug_op_cfgs",
    "dmx_debug_run_op_as", "dmx_debug_run_attention_as",
    "dmx_engine_create", "dmx_engine_free", "dmx_engine_n_devices", "dmx_engine_n_models", "dmx_engine_n_sources",
    "dmx_resample_length", "dmx_resample_filter", "dmx_resample_device", "dmx_resample",
    "dmx_ctx_create_gemm", "dmx_ctx_gemm", "dmx_default_gemm", "dmx_set_default_gemm", "dmx_debug_split_weights", "dmx_debug_split_activations", "dmx_debug_split_activations_fp16",
    "dmx_model_arch", "dmx_engine_arch", "dmx_engine_transport", "dmx_engine_set_finish", "dmx_engine_finish", "dmx_engine_root_ctx", "dmx_engine_track_infer", "dmx_engine_partition",
    "dmx_tracks_infer", "dmx_tracks_infer_opts", "dmx_track_geometry_overlap",
    "dmx_output_count", "dmx_output_bytes", "dmx_tracks_infer_pcm", "dmx_pcm_encode_device", "dmx_pcm_encode",
    "dmx_bag_weights", "dmx_tracks_infer_bag",
    "dmx_remix_two_stems", "dmx_remix_check", "dmx_tracks_infer_remix", "dmx_remix_encode_device", "dmx_remix_encode",
    "dmx_flac_bound", "dmx_flac_workspace_bytes", "dmx_flac_encode_device", "dmx_flac_encode", "dmx_tracks_infer_flac",
    "dmx_flac_encode_device_level", "dmx_flac_encode_level", "dmx_flac_encode_device_timed", "dmx_ctx_set_flac_level", "dmx_ctx_flac_level",
    "dmx_flac_probe", "dmx_flac_decode_workspace_bytes", "dmx_flac_decode_device", "dmx_flac_decode", "dmx_tracks_infer_from_flac", "dmx_flac_decode_profile",
    "dmx_tracks_infer_rates", "dmx_tracks_infer_from_flac_rates", "dmx_resample_ready",
    "dmx_loudness_coefficients", "dmx_loudness_gain_table", "dmx_loudness_check", "dmx_loudness_workspace_bytes", "dmx_loudness_device",
    "dmx_loudness_device_timed", "dmx_loudness", "dmx_loud_encode_device", "dmx_loud_encode",
    "dmx_tracks_infer_loud", "dmx_tracks_infer_from_flac_loud",
    "dmx_true_peak_filter", "dmx_meters_workspace_bytes", "dmx_meters_device", "dmx_meters_device_timed", "dmx_meters",
    "dmx_loud_encode_meters_device", "dmx_loud_encode_meters", "dmx_tracks_infer_meters", "dmx_tracks_infer_from_flac_meters",
    "dmx_limiter_tables", "dmx_limiter_slopes", "dmx_limiter_workspace_bytes", "dmx_limit_device", "dmx_limit_device_timed", "dmx_limit",
    "dmx_limiter_check", "dmx_loud_encode_limit_device", "dmx_loud_encode_limit", "dmx_tracks_infer_limit", "dmx_tracks_infer_from_flac_limit",
]

TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_P2P = 0, 1, 2
GEMM_F32, GEMM_BF16X3, GEMM_FP16X3 = 0, 1, 2  # include/demucs_hip.h DMX_GEMM_* (FP16X3: opt-in, linear layers with fp16 terms)
GEMM_NAMES = {GEMM_F32: "f32", GEMM_BF16X3: "bf16x3", GEMM_FP16X3: "fp16x3"}
FINISH_ROOT, FINISH_OWNER = 0, 1
PCM_F32, PCM_S16, PCM_S24 = 0, 1, 2  # include/demucs_hip.h DMX_PCM_*
CLIP_NONE, CLIP_RESCALE, CLIP_CLAMP = 0, 1, 2  # DMX_CLIP_*
MAX_OUTPUTS = 8  # DMX_MAX_OUTPUTS
OTHER_ADD, OTHER_MINUS, OTHER_NONE = 0, 1, 2  # DMX_OTHER_*


class OutputSpec(ctypes.Structure):
    """dmx_output_spec: encoding PCM_*, clip CLIP_*, stem -1 (all stems) or the stem of two-stems mode.
    The defaults are demucs's: 16 bit, rescale, all stems."""
    _fields_ = [("encoding", ctypes.c_int), ("clip", ctypes.c_int), ("stem", ctypes.c_int)]

    def __init__(self, encoding=PCM_S16, clip=CLIP_RESCALE, stem=-1):
        super().__init__(int(encoding), int(clip), int(stem))


class _RemixSpecC(ctypes.Structure):
    _fields_ = [("encoding", ctypes.c_int), ("clip", ctypes.c_int), ("n_out", ctypes.c_int), ("gains", ctypes.c_void_p)]


class RemixSpec:
    """dmx_remix_spec: `gains` is an (n_out, S + 1) matrix over the S stems and, in the last column, the original mixture;
    encoding PCM_*, clip CLIP_*. The object keeps the gain array alive for the C structure (`.c`) that points into it.
    gains None builds a structure with a NULL matrix (for the error path)."""

    def __init__(self, gains, encoding=PCM_S16, clip=CLIP_RESCALE, n_out=None):
        self.gains = None if gains is None else np.ascontiguousarray(gains, np.float32)
        if self.gains is not None:
            assert self.gains.ndim == 2, "gains: expected an (n_out, S + 1) matrix"
        self.encoding, self.clip = int(encoding), int(clip)
        self.n_out = int(n_out) if n_out is not None else (0 if self.gains is None else self.gains.shape[0])
        self.c = _RemixSpecC(self.encoding, self.clip, self.n_out, None if self.gains is None else self.gains.ctypes.data)

    def output_spec(self) -> "OutputSpec":
        """the encoding and clip mode as an OutputSpec (for output_bytes / pcm_views)"""
        return OutputSpec(self.encoding, self.clip, -1)


_lib = None
PROGRESS_FN = ctypes.CFUNCTYPE(None, ctypes.c_float, ctypes.c_char_p, ctypes.c_void_p)


class DmxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[dmx error {code}] {msg}")
        self.code = code


def lib():
    global _lib
    if _lib is None:
        # PyTorch-ROCm bundles its own libamdhip64.so.7; a process must hold ONE HIP runtime.
        # Importing torch first makes the dynamic linker bind our NEEDED libamdhip64.so.7 to the
        # copy torch already loaded (same SONAME), so torch tensors / RCCL and this library share
        # the device context. (Loading ours first left torch with "No HIP GPUs are available".)
        if os.environ.get("DMX_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except Exception:  # torch is plumbing only; the library works without it
                pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `make` or __graft_entry__.build() (no fallback exists)")
        L = ctypes.CDLL(LIB_PATH)
        vp, i64, ci, fp = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
        L.dmx_last_error.restype = ctypes.c_char_p
        L.dmx_model_load.argtypes = [ctypes.c_char_p, ci, ctypes.POINTER(vp)]
        L.dmx_model_free.argtypes = [vp]
        for f in ("dmx_model_n_sources", "dmx_model_n_tensors", "dmx_model_device", "dmx_model_arch"):
            getattr(L, f).argtypes = [vp]
        L.dmx_ctx_create.argtypes = [vp, i64, ci, ctypes.POINTER(vp)]
        L.dmx_ctx_create_gemm.argtypes = [vp, i64, ci, ci, ctypes.POINTER(vp)]
        L.dmx_ctx_gemm.argtypes = [vp]
        L.dmx_set_default_gemm.argtypes = [ci]
        L.dmx_debug_split_weights.argtypes = [fp, i64, fp, fp]
        L.dmx_debug_split_weights.restype = i64
        L.dmx_debug_split_activations.argtypes = [ci, fp, i64, fp]
        L.dmx_debug_split_activations_fp16.argtypes = [ci, fp, i64, ci, fp]
        L.dmx_ctx_free.argtypes = [vp]
        L.dmx_ctx_segment_samples.argtypes = [vp]
        L.dmx_ctx_segment_samples.restype = i64
        L.dmx_ctx_max_batch.argtypes = [vp]
        L.dmx_ctx_arena_bytes.argtypes = [vp]
        L.dmx_ctx_arena_bytes.restype = i64
        L.dmx_ctx_synchronize.argtypes = [vp]
        L.dmx_ctx_set_stream.argtypes = [vp, vp]
        L.dmx_segment_infer.argtypes = [vp, fp, fp, ci]
        L.dmx_segment_infer_device.argtypes = [vp, fp, fp, ci]
        L.dmx_track_infer.argtypes = [vp, fp, i64, ci, fp, ci, vp, vp]
        L.dmx_tracks_infer.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp]
        L.dmx_tracks_infer_opts.argtypes = [vp, ci, vp, vp, ci, ctypes.c_float, vp, vp, ci, vp, vp]
        L.dmx_track_geometry_overlap.argtypes = [i64, i64, ci, ctypes.c_float, ctypes.POINTER(i64), ctypes.POINTER(ci), ctypes.POINTER(i64)]
        L.dmx_output_count.argtypes = [vp, vp]
        L.dmx_output_bytes.argtypes = [vp, i64]
        L.dmx_output_bytes.restype = i64
        L.dmx_tracks_infer_pcm.argtypes = [vp, ci, vp, vp, ci, ctypes.c_float, vp, vp, vp, vp, ci, vp, vp]
        L.dmx_pcm_encode_device.argtypes = [ci, vp, ci, i64, i64, vp, vp, vp, vp]
        L.dmx_pcm_encode.argtypes = [ci, vp, ci, i64, vp, vp, vp]
        L.dmx_bag_weights.argtypes = [ci, ci, vp, vp, vp]
        L.dmx_tracks_infer_bag.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, ctypes.c_float, vp, vp, vp, vp, ci, vp, vp]
        L.dmx_remix_two_stems.argtypes = [ci, ci, ci, vp, vp]
        L.dmx_remix_check.argtypes = [ci, vp]
        L.dmx_tracks_infer_remix.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, ctypes.c_float, vp, vp, vp, vp, ci, vp, vp]
        L.dmx_remix_encode_device.argtypes = [ci, vp, ci, i64, i64, vp, vp, vp, vp, vp]
        L.dmx_remix_encode.argtypes = [ci, vp, ci, i64, vp, vp, vp, vp]
        L.dmx_flac_bound.argtypes = [ci, i64]
        L.dmx_flac_bound.restype = i64
        L.dmx_flac_workspace_bytes.argtypes = [ci, i64]
        L.dmx_flac_workspace_bytes.restype = i64
        L.dmx_flac_encode_device.argtypes = [ci, vp, ci, i64, ci, vp, vp, vp, vp]
        L.dmx_flac_encode.argtypes = [ci, vp, ci, i64, ci, vp, vp]
        L.dmx_flac_encode_device_level.argtypes = [ci, vp, ci, i64, ci, ci, vp, vp, vp, vp]
        L.dmx_flac_encode_level.argtypes = [ci, vp, ci, i64, ci, ci, vp, vp]
        L.dmx_flac_encode_device_timed.argtypes = [ci, vp, ci, i64, ci, ci, vp, vp, vp, vp, vp]
        L.dmx_ctx_set_flac_level.argtypes = [vp, ci]
        L.dmx_ctx_flac_level.argtypes = [vp]
        L.dmx_flac_probe.argtypes = [vp, i64, vp]
        L.dmx_flac_decode_workspace_bytes.argtypes = [vp, i64]
        L.dmx_flac_decode_workspace_bytes.restype = i64
        L.dmx_flac_decode_device.argtypes = [ci, vp, i64, vp, ci, vp, vp, vp, vp]
        L.dmx_flac_decode.argtypes = [ci, vp, i64, vp, ci, vp, vp]
        L.dmx_flac_decode_profile.argtypes = [ci, vp, i64, vp, ci, vp, vp, vp, vp, vp]
        L.dmx_tracks_infer_from_flac.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, ctypes.c_float, vp, vp, ci, vp, vp, vp, vp, vp, vp]
        L.dmx_tracks_infer_from_flac_rates.argtypes = L.dmx_tracks_infer_from_flac.argtypes
        L.dmx_tracks_infer_rates.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, ci, ctypes.c_float, vp, vp, ci, vp, vp, vp, ci, vp, vp]
        L.dmx_resample_ready.argtypes = [i64, i64, ci, ci, i64]
        L.dmx_resample_ready.restype = i64
        L.dmx_loudness_coefficients.argtypes = [ci, vp]
        L.dmx_loudness_gain_table.argtypes = [vp]
        L.dmx_loudness_check.argtypes = [vp, ci]
        L.dmx_loudness_workspace_bytes.argtypes = [i64]
        L.dmx_loudness_workspace_bytes.restype = i64
        L.dmx_loudness_device.argtypes = [ci, vp, i64, i64, ci, vp, vp, vp, vp]
        L.dmx_loudness_device_timed.argtypes = [ci, vp, i64, i64, ci, vp, vp, vp, vp, vp]
        L.dmx_loudness.argtypes = [ci, vp, i64, ci, ci, vp, vp]
        L.dmx_loud_encode_device.argtypes = [ci, vp, ci, i64, i64, vp, vp, vp, ci, vp, vp, vp, vp, vp]
        L.dmx_loud_encode.argtypes = [ci, vp, ci, i64, vp, vp, vp, ci, vp, vp, vp]
        L.dmx_tracks_infer_loud.argtypes = L.dmx_tracks_infer_rates.argtypes + [vp, vp]
        L.dmx_tracks_infer_from_flac_loud.argtypes = L.dmx_tracks_infer_from_flac.argtypes + [vp, vp]
        L.dmx_true_peak_filter.argtypes = [ci, vp, vp]
        L.dmx_meters_workspace_bytes.argtypes = [i64]
        L.dmx_meters_workspace_bytes.restype = i64
        L.dmx_meters_device.argtypes = L.dmx_loudness_device.argtypes + [vp]
        L.dmx_meters_device_timed.argtypes = [ci, vp, i64, i64, ci, vp, vp, vp]
        L.dmx_meters.argtypes = L.dmx_loudness.argtypes + [vp]
        L.dmx_loud_encode_meters_device.argtypes = L.dmx_loud_encode_device.argtypes + [vp]
        L.dmx_loud_encode_meters.argtypes = L.dmx_loud_encode.argtypes + [vp]
        L.dmx_tracks_infer_meters.argtypes = L.dmx_tracks_infer_loud.argtypes + [vp]
        L.dmx_tracks_infer_from_flac_meters.argtypes = L.dmx_tracks_infer_from_flac_loud.argtypes + [vp]
        L.dmx_limiter_tables.argtypes = [vp, vp, vp]
        L.dmx_limiter_slopes.argtypes = [ci, ctypes.c_double, ctypes.c_double, vp, vp]
        L.dmx_limiter_workspace_bytes.argtypes = [i64]
        L.dmx_limiter_workspace_bytes.restype = i64
        L.dmx_limit_device.argtypes = [ci, vp, i64, i64, ci, ctypes.c_float, ctypes.c_float, ci, vp, vp, vp, vp]
        L.dmx_limit_device_timed.argtypes = L.dmx_limit_device.argtypes + [vp]
        L.dmx_limit.argtypes = [ci, vp, i64, ci, ci, ctypes.c_float, ctypes.c_float, ci, vp, vp, vp, vp]
        L.dmx_limiter_check.argtypes = [vp, vp, ci]
        L.dmx_loud_encode_limit_device.argtypes = L.dmx_loud_encode_meters_device.argtypes + [vp, vp]
        L.dmx_loud_encode_limit.argtypes = L.dmx_loud_encode_meters.argtypes + [vp, vp]
        L.dmx_tracks_infer_limit.argtypes = L.dmx_tracks_infer_meters.argtypes + [vp, vp]
        L.dmx_tracks_infer_from_flac_limit.argtypes = L.dmx_tracks_infer_from_flac_meters.argtypes + [vp, vp]
        L.dmx_tracks_infer_flac.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, ctypes.c_float, vp, vp, ci, vp, vp, vp, ci, vp, vp]
        L.dmx_track_geometry.argtypes = [vp, i64, ci, ctypes.POINTER(i64), ctypes.POINTER(ci), ctypes.POINTER(i64)]
        L.dmx_track_stats_device.argtypes = [vp, fp, i64, fp]
        L.dmx_track_gather_device.argtypes = [vp, fp, i64, fp, ci, vp, ci, fp]
        L.dmx_track_overlap_add_device.argtypes = [vp, fp, ci, i64, ci, fp, fp, ci]
        L.dmx_debug_tap.argtypes = [vp, ctypes.c_char_p, vp, fp]
        L.dmx_debug_n_ops.argtypes = [vp]
        L.dmx_debug_profile.argtypes = [vp, ci, ci, ctypes.c_char_p, ci]
        L.dmx_debug_plan_info.argtypes = [vp, ci, vp, vp, vp, vp]
        L.dmx_debug_op_info.argtypes = [vp, ci, ci, ctypes.c_char_p, ci]
        L.dmx_debug_arena_fill.argtypes = [vp, ci, ctypes.c_uint]
        L.dmx_debug_arena_io.argtypes = [vp, i64, i64, fp, ci]
        L.dmx_debug_run_op.argtypes = [vp, ci, ci]
        L.dmx_debug_op_cfgs.argtypes = [vp, ci, ci, vp, ci]
        L.dmx_debug_run_op_as.argtypes = [vp, ci, ci, ci, ci, ctypes.c_char_p, ci]
        L.dmx_debug_run_attention_as.argtypes = [vp, ci, ci, ci]
        L.dmx_ctx_set_model.argtypes = [vp, vp]
        L.dmx_engine_create.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, ctypes.POINTER(ci), ci, ci, ci, ctypes.POINTER(vp)]
        L.dmx_engine_free.argtypes = [vp]
        L.dmx_engine_set_finish.argtypes = [vp, ci]
        for f in ("dmx_engine_n_devices", "dmx_engine_n_models", "dmx_engine_n_sources", "dmx_engine_transport", "dmx_engine_finish"):
            getattr(L, f).argtypes = [vp]
        L.dmx_engine_root_ctx.argtypes = [vp, ci]
        L.dmx_engine_root_ctx.restype = vp
        L.dmx_engine_track_infer.argtypes = [vp, fp, i64, ctypes.POINTER(ci), fp, ci, vp, vp]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise DmxError(rc, lib().dmx_last_error().decode(errors="replace"))


DEBUG_NO_KERNEL = 6  # dmx_debug_run_op_as / dmx_debug_run_attention_as: no such kernel, nothing launched
ATTENTION_FORMS = ("wg64", "wg128", "pair")  # csrc/attention_select.h AttentionForm, by value


def parse_op_info(text: str) -> dict:
    """key=value words of dmx_debug_op_info / dmx_debug_run_op_as -> dict: integers as int, 'lo:hi,' lists as [(lo, hi)]"""
    d = {}
    for word in text.split():
        k, _, v = word.partition("=")
        if k in ("reads", "writes", "scratch", "rowstat"):
            d[k] = [tuple(int(x) for x in r.split(":")) for r in v.split(",") if r]
        elif k in ("name", "label", "form"):
            d[k] = v
        elif k == "scale":
            d[k] = float(v)
        else:
            d[k] = int(v)
    return d


def device_count() -> int:
    return lib().dmx_device_count()


class Model:
    """demucscpp::demucs_model + load_demucs_model (src/model.hpp:285-554, :649)."""

    def __init__(self, path: str, device: int = 0):
        self.h = ctypes.c_void_p()
        _chk(lib().dmx_model_load(path.encode(), device, ctypes.byref(self.h)))
        self.n_sources = lib().dmx_model_n_sources(self.h)
        self.n_tensors = lib().dmx_model_n_tensors(self.h)
        self.arch = lib().dmx_model_arch(self.h)  # 4: HTDemucs v4, 3: Demucs v3 (hdemucs_mmi)
        self.device = device

    def close(self):
        if self.h:
            lib().dmx_model_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_gemm() -> int:
    return lib().dmx_default_gemm()


def set_default_gemm(gemm: int):
    """GEMM arithmetic of contexts (and engines) created from now on: GEMM_F32 | GEMM_BF16X3 | GEMM_FP16X3."""
    _chk(lib().dmx_set_default_gemm(gemm))


def split_weights(w: np.ndarray):
    """(w1, w2, n_inexact): bf16 bit patterns of the two-term weight split of GEMM_BF16X3 (host function)."""
    w = np.ascontiguousarray(w, np.float32).ravel()
    w1 = np.zeros(w.size, np.uint16)
    w2 = np.zeros(w.size, np.uint16)
    bad = lib().dmx_debug_split_weights(w.ctypes.data, w.size, w1.ctypes.data, w2.ctypes.data)
    return w1, w2, int(bad)


def split_activations(x: np.ndarray, device: int = 0) -> np.ndarray:
    """(3, n) bf16 bit patterns a1, a2, a3 of the kernels' three-term activation split (runs on the GPU)."""
    x = np.ascontiguousarray(x, np.float32).ravel()
    planes = np.zeros((3, x.size), np.uint16)
    _chk(lib().dmx_debug_split_activations(device, x.ctypes.data, x.size, planes.ctypes.data))
    return planes


def split_activations_fp16(x: np.ndarray, scale_exp: int = 0, device: int = 0) -> np.ndarray:
    """(3, n) fp16 bit patterns h1, h2, h3 of the fp16-term split of x * 2^scale_exp (GEMM_FP16X3; runs on the GPU)."""
    x = np.ascontiguousarray(x, np.float32).ravel()
    planes = np.zeros((3, x.size), np.uint16)
    _chk(lib().dmx_debug_split_activations_fp16(device, x.ctypes.data, x.size, int(scale_exp), planes.ctypes.data))
    return planes


# ---- marshalling of the track calls (Context.track, Context.tracks_*, Engine.track): one helper per duty. What a helper
# returns beside the ctypes pointers is what the caller keeps alive until the library call has returned.
def _progress_thunk(progress):
    """(the PROGRESS_FN object, the pointer to pass) of a progress(fraction, message) callable; (None, None) without one"""
    if not progress:
        return None, None
    cb = PROGRESS_FN(lambda p, m, u: progress(p, m.decode()))
    return cb, ctypes.cast(cb, ctypes.c_void_p)


def _pointers(arrays):
    return (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def _shift_array(shift_offsets, T: int, Q: Optional[int], n_shifts: int):
    """the c_int array of shift offsets of shape (T, n_shifts), or (T, Q, n_shifts) with models; None stays None"""
    if shift_offsets is None:
        return None
    arr = np.asarray(shift_offsets, np.int64)
    want = (T, n_shifts) if Q is None else (T, Q, n_shifts)
    assert arr.shape == want, f"shift_offsets: expected shape {want}, got {arr.shape}"
    return (ctypes.c_int * max(arr.size, 1))(*[int(v) for v in arr.ravel()])


def _models_weights(models, weights, S: int):
    """(model pointers or None, Q, weights pointer or None, the weights array): models None is the context's own model
    (Q 0); a None entry becomes a NULL model, which the library refuses"""
    Q = 0 if models is None else len(models)
    mp = None if models is None else (ctypes.c_void_p * max(Q, 1))(*[m.h.value if m is not None else None for m in models])
    if weights is None:
        return mp, Q, None, None
    warr = np.ascontiguousarray(weights, np.float32)
    assert warr.shape == (Q, S), f"weights: expected shape {(Q, S)}, got {warr.shape}"
    return mp, Q, warr.ctypes.data, warr


def _track_inputs(audios, layout: int):
    """(T, lengths, the arrays passed, their pointers, the c_int64 lengths) of (2, n_t) tracks: float32 and contiguous as
    they are, or for LAYOUT_EIGEN their transposed copies, [n][2] == column-major 2 x n"""
    audios = [np.ascontiguousarray(a, np.float32) for a in audios]
    ns = [a.shape[1] for a in audios]
    src = [np.ascontiguousarray(a.T) for a in audios] if layout == LAYOUT_EIGEN else audios
    return len(ns), ns, src, _pointers(src), (ctypes.c_int64 * max(len(ns), 1))(*ns)


def _fp32_results(out, ns, S: int, layout: int):
    """(pointers to write through, finish): `out` is the caller's list of (S, 2, n_t) float32 arrays or None (allocated);
    finish() returns it, for LAYOUT_EIGEN after copying back the images the library wrote (flat index s + S*(c + 2*i))"""
    if out is None:
        out = [np.zeros((S, 2, n), np.float32) for n in ns]
    assert len(out) == len(ns)
    for o, n in zip(out, ns):
        assert o.shape == (S, 2, n) and o.dtype == np.float32 and o.flags.c_contiguous
    if layout != LAYOUT_EIGEN:
        return _pointers(out), lambda: out
    dst = [np.zeros((n, 2, S), np.float32) for n in ns]

    def finish():
        for o, img in zip(out, dst):
            o[...] = img.transpose(2, 1, 0)
        return out
    return _pointers(dst), finish


def _byte_results(want, out, exact: bool):
    """(buffers, their pointers): one np.uint8 buffer of want[t] bytes per track, allocated, or the caller's `out`, which
    must have exactly that size (the PCM forms) or at least that size (the FLAC forms, whose sizes are bounds)"""
    bufs = out if out is not None else [np.zeros(w if exact else max(w, 1), np.uint8) for w in want]
    assert len(bufs) == len(want)
    for b, w in zip(bufs, want):
        assert b.dtype == np.uint8 and b.ndim == 1 and (b.size == w if exact else b.size >= w) and b.flags.c_contiguous
    return bufs, _pointers(bufs)


def _flat_result(arr, count: int, dtype):
    """a flat array of at least `count` entries (peaks, sizes): the caller's, checked, or a new one"""
    if arr is None:
        arr = np.zeros(max(count, 1), dtype)
    assert arr.dtype == dtype and arr.ndim == 1 and arr.size >= count and arr.flags.c_contiguous
    return arr


def _frame_bytes(encoding: int) -> int:
    """bytes of one stereo frame of PCM_*"""
    return {PCM_F32: 8, PCM_S16: 4, PCM_S24: 6}.get(encoding, 8)


def _remix_bytes(spec: "RemixSpec", ns, flac: bool):
    """bytes of one output of every track under a RemixSpec: its PCM, or the bound of its .flac file (0 where the library
    refuses the arguments, which the call itself then reports)"""
    if not flac:
        return [n * _frame_bytes(spec.encoding) for n in ns]
    return [max(lib().dmx_flac_bound(24 if spec.encoding == PCM_S24 else 16, n), 0) for n in ns]


def _pcm_results(bufs, spec: "OutputSpec", ns, n_out: int):
    return [pcm_views(b, spec, n, n_out) for b, n in zip(bufs, ns)]


def _flac_files(bufs, bounds, sizes, n_out: int):
    """files[t][o]: output o of track t starts at o * bounds[t] and has sizes[t * n_out + o] bytes"""
    return [[bytes(b[o * bd:o * bd + int(sizes[t * n_out + o])]) for o in range(n_out)] for t, (b, bd) in enumerate(zip(bufs, bounds))]


def _cut_peaks(peaks, T: int, n_out: int):
    return [peaks[t * n_out:(t + 1) * n_out] for t in range(T)]


class Context:
    def __init__(self, model: Model, segment_samples: int = 0, max_batch: int = 1, gemm: Optional[int] = None):
        self.model = model
        self.h = ctypes.c_void_p()
        if gemm is None:
            _chk(lib().dmx_ctx_create(model.h, segment_samples, max_batch, ctypes.byref(self.h)))
        else:
            _chk(lib().dmx_ctx_create_gemm(model.h, segment_samples, max_batch, gemm, ctypes.byref(self.h)))
        self.gemm = lib().dmx_ctx_gemm(self.h)
        self.seg = lib().dmx_ctx_segment_samples(self.h)
        self.max_batch = max_batch
        self.S = model.n_sources

    def close(self):
        if self.h:
            lib().dmx_ctx_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def arena_bytes(self) -> int:
        return lib().dmx_ctx_arena_bytes(self.h)

    @property
    def flac_level(self) -> int:
        """the compression level of tracks_flac() and tracks_from_flac(flac_out=True): 0 (default) FIXED predictors alone,
        1 + LPC order 8, 2 + LPC orders 8 and 12 (dmx_ctx_set_flac_level)"""
        return lib().dmx_ctx_flac_level(self.h)

    @flac_level.setter
    def flac_level(self, level: int):
        _chk(lib().dmx_ctx_set_flac_level(self.h, int(level)))

    def synchronize(self):
        _chk(lib().dmx_ctx_synchronize(self.h))

    def set_model(self, model: "Model"):
        """Rebind to another model of the same architecture on the same device (the fine-tuned bag shares one arena)."""
        _chk(lib().dmx_ctx_set_model(self.h, model.h))
        self.model = model

    def set_stream(self, hip_stream: Optional[int]):
        """Order the context's device work on a caller-owned hipStream_t (raw handle, e.g.
        torch.cuda.Stream().cuda_stream); None returns to the context's own stream."""
        _chk(lib().dmx_ctx_set_stream(self.h, ctypes.c_void_p(hip_stream) if hip_stream else None))

    # ---- host-pointer API
    def segment(self, mix: np.ndarray) -> np.ndarray:
        """mix (2, seg) planar -> (S, 2, seg) planar; demucscpp::model_inference."""
        mix = np.ascontiguousarray(mix, np.float32)
        assert mix.shape == (2, self.seg)
        out = np.zeros((self.S, 2, self.seg), np.float32)
        _chk(lib().dmx_segment_infer(self.h, mix.ctypes.data, out.ctypes.data, LAYOUT_PLANAR))
        return out

    def segment_eigen(self, mix_interleaved: np.ndarray) -> np.ndarray:
        """Eigen memory images: in (seg, 2) interleaved, out flat image of Tensor3dXf(S,2,seg)."""
        mix = np.ascontiguousarray(mix_interleaved, np.float32)
        out = np.zeros(self.S * 2 * self.seg, np.float32)
        _chk(lib().dmx_segment_infer(self.h, mix.ctypes.data, out.ctypes.data, LAYOUT_EIGEN))
        return out

    def track(self, audio: np.ndarray, shift_offset: int, progress=None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """audio (2, n) planar -> (S, 2, n); demucscpp::demucs_inference. `out`: reuse a result buffer."""
        audio = np.ascontiguousarray(audio, np.float32)
        n = audio.shape[1]
        if out is None:
            out = np.zeros((self.S, 2, n), np.float32)
        assert out.shape == (self.S, 2, n) and out.dtype == np.float32 and out.flags.c_contiguous
        cb, cbp = _progress_thunk(progress)
        _chk(lib().dmx_track_infer(self.h, audio.ctypes.data, n, shift_offset, out.ctypes.data, LAYOUT_PLANAR, cbp, None))
        return out

    # ---- many tracks in one call: every method assembles the pieces of the helpers above, makes one call and shapes the result
    def _output_count(self, spec: "OutputSpec") -> int:
        n_out = lib().dmx_output_count(self.model.h, ctypes.byref(spec))
        if n_out < 0:
            raise DmxError(5, lib().dmx_last_error().decode(errors="replace"))
        return n_out

    def tracks(self, audios, shift_offsets=None, progress=None, out=None, layout: int = LAYOUT_PLANAR) -> List[np.ndarray]:
        """Several (2, n_t) planar tracks -> list of (S, 2, n_t) in ONE call (dmx_tracks_infer: their segments share batches);
        each result is bit-identical to track() of that track. shift_offsets: None or one per track (-1: rand() % 22050,
        drawn in track order). `out`: a list of result buffers to reuse. layout=LAYOUT_EIGEN passes the tracks and receives
        the results through the C ABI as Eigen column-major images; the arrays seen by the caller are the same."""
        T, ns, src, ap, na = _track_inputs(audios, layout)
        op, finish = _fp32_results(out, ns, self.S, layout)
        so = (ctypes.c_int * max(T, 1))(*shift_offsets) if shift_offsets is not None else None
        cb, cbp = _progress_thunk(progress)
        _chk(lib().dmx_tracks_infer(self.h, T, ap, na, so, op, layout, cbp, None))
        return finish()

    def tracks_opts(self, audios, n_shifts: int = 1, overlap: float = 0.25, shift_offsets=None, progress=None, out=None,
                    layout: int = LAYOUT_PLANAR) -> List[np.ndarray]:
        """tracks() with demucs's shifts ensemble and segment overlap (dmx_tracks_infer_opts): each track is run as n_shifts
        copies, copy k shifted by shift_offsets[t, k], and the copies' normalised results are averaged before
        de-normalisation. shift_offsets: None or an int array of shape (T, n_shifts), -1 entries drawn as rand() % 22050 in
        (track, copy) order. n_shifts=1, overlap=0.25 gives the bits of tracks()."""
        T, ns, src, ap, na = _track_inputs(audios, layout)
        op, finish = _fp32_results(out, ns, self.S, layout)
        so = _shift_array(shift_offsets, T, None, n_shifts)
        cb, cbp = _progress_thunk(progress)
        _chk(lib().dmx_tracks_infer_opts(self.h, T, ap, na, int(n_shifts), float(overlap), so, op, layout, cbp, None))
        return finish()

    def tracks_pcm(self, audios, spec: Optional[OutputSpec] = None, n_shifts: int = 1, overlap: float = 0.25, shift_offsets=None,
                   progress=None, layout: int = LAYOUT_PLANAR, out=None, loudness=None, meters: bool = False, limit_report: bool = False):
        """loudness: None, or a LoudnessSpec - the spec's outputs as 0/1 gains (the same bits) through dmx_tracks_infer_loud;
        returns (outs, peaks, report) as tracks_remix() does, with meters=True (outs, peaks, report, meters).
        tracks_opts() whose stems leave the GPU as WAV data (dmx_tracks_infer_pcm): two-stems, clip mode and sample
        format are applied on the device. Returns (outs, peaks): outs[t] is a list of n_out arrays, np.int16 (n, 2),
        np.uint8 (n, 2, 3) (packed little-endian 24 bit) or np.float32 (n, 2); peaks[t] is an np.float32 (n_out,) array.
        `out`: a list of np.uint8 buffers of n_out * output_bytes(spec, n_t) bytes to reuse (the results are views of them)."""
        spec = spec if spec is not None else OutputSpec()
        if loudness is not None:
            assert out is None, "loudness=: buffers to reuse are not taken"
            g = np.eye(self.S, self.S + 1, dtype=np.float32) if spec.stem < 0 else remix_two_stems(self.S, spec.stem, OTHER_ADD)
            return self.tracks_rates(audios, None, RemixSpec(g, spec.encoding, spec.clip), False, None, None, n_shifts, overlap, shift_offsets,
                                     progress, layout, loudness, meters, limit_report)
        assert not meters and not limit_report, "meters=True and limit_report=True need loudness="
        T, ns, src, ap, na = _track_inputs(audios, layout)
        n_out = self._output_count(spec)
        bufs, op = _byte_results([n_out * output_bytes(spec, n) for n in ns], out, exact=True)
        peaks = _flat_result(None, T * n_out, np.float32)
        so = _shift_array(shift_offsets, T, None, n_shifts)
        cb, cbp = _progress_thunk(progress)
        _chk(lib().dmx_tracks_infer_pcm(self.h, T, ap, na, int(n_shifts), float(overlap), so, ctypes.byref(spec), op,
                                        peaks.ctypes.data, layout, cbp, None))
        return _pcm_results(bufs, spec, ns, n_out), _cut_peaks(peaks, T, n_out)

    def tracks_bag(self, models, audios, weights=None, n_shifts: int = 1, overlap: float = 0.25, shift_offsets=None,
                   spec: Optional[OutputSpec] = None, progress=None, layout: int = LAYOUT_PLANAR, out=None):
        """Several tracks through a bag of models in ONE call (dmx_tracks_infer_bag): `models` are Model objects of this
        context's architecture, `weights` None (the diagonal, fine-tuned bag: stem i from model i) or a (Q, S) matrix of
        weights >= 0 (equal weights: an ensemble). shift_offsets: None or an int array of shape (T, Q, n_shifts), -1
        entries drawn as rand() % 22050 in that row-major order. spec None: a list of (S, 2, n_t) float32 arrays as
        tracks_opts(); else (outs, peaks) as tracks_pcm(). The context stays bound to its own model."""
        T, ns, src, ap, na = _track_inputs(audios, layout)
        mp, Q, wp, keep = _models_weights(list(models), weights, self.S)
        so = _shift_array(shift_offsets, T, Q, n_shifts)
        cb, cbp = _progress_thunk(progress)
        if spec is None:
            op, finish = _fp32_results(out, ns, self.S, layout)
            sp = pk = None
        else:
            n_out = self._output_count(spec)
            bufs, op = _byte_results([n_out * output_bytes(spec, n) for n in ns], out, exact=True)
            peaks = _flat_result(None, T * n_out, np.float32)
            sp, pk = ctypes.byref(spec), peaks.ctypes.data
        _chk(lib().dmx_tracks_infer_bag(self.h, mp, Q, wp, T, ap, na, int(n_shifts), float(overlap), so, sp, op, pk, layout, cbp, None))
        return finish() if spec is None else (_pcm_results(bufs, spec, ns, n_out), _cut_peaks(peaks, T, n_out))

    def tracks_remix(self, audios, spec: RemixSpec, models=None, weights=None, n_shifts: int = 1, overlap: float = 0.25,
                     shift_offsets=None, progress=None, layout: int = LAYOUT_PLANAR, out=None, peaks=None, loudness=None,
                     meters: bool = False, limit_report: bool = False):
        """tracks_pcm() whose outputs are rows of gains over the stems and the original mixture (dmx_tracks_infer_remix).
        loudness: None, or a LoudnessSpec - the call goes through dmx_tracks_infer_loud and returns (outs, peaks, report), report
        a (T, n_out + 1) array of LOUDNESS_DTYPE, per track its outputs and then its mixture. meters=True (with loudness=): the call
        goes through dmx_tracks_infer_meters and returns (outs, peaks, report, meters), meters a (T, n_out + 1) array of METERS_DTYPE.
        models None: this context's model, shift_offsets (T, n_shifts); else a bag as tracks_bag(), shift_offsets
        (T, Q, n_shifts). Returns (outs, peaks) in the shapes of tracks_pcm(), n_out = spec.n_out. `out` / `peaks`: buffers
        to reuse (np.uint8 of n_out * output_bytes bytes per track; a flat np.float32 array of at least T * n_out entries)."""
        if loudness is not None:
            assert out is None and peaks is None, "loudness=: buffers to reuse are not taken"
            return self.tracks_rates(audios, None, spec, False, models, weights, n_shifts, overlap, shift_offsets, progress, layout, loudness,
                                     meters, limit_report)
        assert not meters and not limit_report, "meters=True and limit_report=True need loudness="
        T, ns, src, ap, na = _track_inputs(audios, layout)
        n_out = max(spec.n_out, 0)
        bufs, op = _byte_results([n_out * b for b in _remix_bytes(spec, ns, False)], out, exact=True)
        peaks = _flat_result(peaks, T * n_out, np.float32)
        mp, Q, wp, keep = _models_weights(models, weights, self.S)
        so = _shift_array(shift_offsets, T, None if models is None else Q, n_shifts)
        cb, cbp = _progress_thunk(progress)
        _chk(lib().dmx_tracks_infer_remix(self.h, mp, Q, wp, T, ap, na, int(n_shifts), float(overlap), so, ctypes.byref(spec.c), op,
                                          peaks.ctypes.data, layout, cbp, None))
        return _pcm_results(bufs, spec.output_spec(), ns, n_out), _cut_peaks(peaks, T, n_out)

    def tracks_from_flac(self, files, spec: RemixSpec, models=None, weights=None, n_shifts: int = 1, overlap: float = 0.25,
                         shift_offsets=None, flac_out: bool = False, progress=None, track_status=None, out=None, any_rate: bool = False,
                         loudness=None, meters: bool = False, limit_report: bool = False):
        """meters=True (with loudness=): through dmx_tracks_infer_from_flac_meters, and the meters report is returned last.
        A loudness spec with LOUD_LIMIT, or limit_report=True: through dmx_tracks_infer_from_flac_limit; the limiter's report last.
        tracks_remix() (flac_out False) or tracks_flac() at 44100 Hz (flac_out True) on tracks given as the bytes of .flac
        files (dmx_tracks_infer_from_flac). any_rate: every track runs at the rate of its file, as tracks_rates() runs it
        (dmx_tracks_infer_from_flac_rates); the outputs have the file's frames and rate. Returns (outs, peaks, track_status): track_status np.int64 (T, 2) = {status, good}
        per track. A damaged track raises DmxError after all work has drained; pass `track_status` (np.int64, T * 2, flat) to
        keep what the call learned, and `.partial` of the error holds (outs, peaks) of that call. `out`: buffers to reuse, as
        tracks_remix() / tracks_flac() take them."""
        T, n_out = len(files), max(spec.n_out, 0)
        imgs = [np.frombuffer(f, np.uint8) for f in files]
        ns = []
        for t, f in enumerate(imgs):  # the sizes of the outputs come from the probe, before any GPU work
            try:
                ns.append(int(flac_probe(f).total_samples))
            except DmxError as e:
                raise DmxError(e.code, f"track {t}: {e}") from None
        per = _remix_bytes(spec, ns, flac_out)
        bufs, op = _byte_results([max(n_out * b, 1) for b in per], out, exact=False)
        sizes = _flat_result(None, T * n_out, np.int64)
        peaks = _flat_result(None, T * n_out, np.float32)
        if track_status is None:
            track_status = np.zeros(2 * max(T, 1), np.int64)
        assert track_status.dtype == np.int64 and track_status.ndim == 1 and track_status.size >= 2 * T
        mp, Q, wp, keep = _models_weights(models, weights, self.S)
        so = _shift_array(shift_offsets, T, None if models is None else Q, n_shifts)
        cb, cbp = _progress_thunk(progress)
        fn = (ctypes.c_int64 * max(T, 1))(*[f.size for f in imgs])
        call = lib().dmx_tracks_infer_from_flac_rates if any_rate else lib().dmx_tracks_infer_from_flac
        extra = ()
        if loudness is not None:  # the report comes back as well; the one entry point runs every track at the rate of its file
            assert out is None, "loudness=: buffers to reuse are not taken"
            for t, f in enumerate(imgs):
                if not any_rate and flac_probe(f).sample_rate != 44100:  # what dmx_tracks_infer_from_flac says of such a file
                    raise DmxError(5, f"tracks_from_flac: track {t}: sample rate {flac_probe(f).sample_rate} (any_rate=True takes other rates)")
            tail = _LoudTail(loudness, meters, limit_report, (max(T, 1),), n_out)
            call, extra = tail.pick(lib(), "dmx_tracks_infer_from_flac"), tail.args
        else:
            assert not meters and not limit_report, "meters=True and limit_report=True need loudness="
        rc = call(self.h, mp, Q, wp, T, _pointers(imgs), fn, int(n_shifts), float(overlap), so, ctypes.byref(spec.c), 1 if flac_out else 0, op,
                  sizes.ctypes.data, peaks.ctypes.data, track_status.ctypes.data, cbp, None, *extra)
        outs = _flac_files(bufs, per, sizes, n_out) if flac_out else _pcm_results(bufs, spec.output_spec(), ns, n_out)
        pk = _cut_peaks(peaks, T, n_out)
        if rc != 0:
            e = DmxError(rc, lib().dmx_last_error().decode(errors="replace"))
            e.partial = (outs, pk)
            raise e
        if loudness is not None:
            return (outs, pk, track_status[:2 * T].reshape(T, 2)) + tail.results(T)
        return outs, pk, track_status[:2 * T].reshape(T, 2)

    def tracks_rates(self, audios, rates, spec: Optional[RemixSpec] = None, flac: bool = False, models=None, weights=None,
                     n_shifts: int = 1, overlap: float = 0.25, shift_offsets=None, progress=None, layout: int = LAYOUT_PLANAR, loudness=None,
                     meters: bool = False, limit_report: bool = False):
        """loudness: None, or a LoudnessSpec (a RemixSpec is then required; rates may be None: all 44100) - the call goes through
        dmx_tracks_infer_loud and returns (outs, peaks, report), report a (T, n_out + 1) array of LOUDNESS_DTYPE; with meters=True
        through dmx_tracks_infer_meters, and (outs, peaks, report, meters) with meters a (T, n_out + 1) array of METERS_DTYPE.
        A loudness spec with LOUD_LIMIT, or limit_report=True: through dmx_tracks_infer_limit; limit_report=True returns a (T, n_out)
        array of LIMIT_DTYPE last.
        Tracks at their own sample rates (dmx_tracks_infer_rates): audios[t] is (2, n_t) at rates[t] Hz; a track that is not
        at 44100 Hz is converted on the device in front of the model and its stems behind it. spec None: a list of (S, 2, n_t)
        float32 arrays as tracks_opts() / tracks_bag(); a RemixSpec: (outs, peaks) as tracks_remix(), or with flac=True
        (files, peaks) as tracks_flac(), every file at its track's rate. models / weights / shift_offsets as tracks_remix()."""
        T, ns, src, ap, na = _track_inputs(audios, layout)
        assert rates is not None or loudness is not None
        assert loudness is not None or not (meters or limit_report), "meters=True and limit_report=True need loudness="
        assert rates is None or len(rates) == T
        ra = None if rates is None else (ctypes.c_int * max(T, 1))(*[int(r) for r in rates])
        mp, Q, wp, keep = _models_weights(models, weights, self.S)
        so = _shift_array(shift_offsets, T, None if models is None else Q, n_shifts)
        cb, cbp = _progress_thunk(progress)
        if spec is None:
            assert not flac, "FLAC files need a RemixSpec"
            op, finish = _fp32_results(None, ns, self.S, layout)
            sp = sz = pk = None
        else:
            n_out = max(spec.n_out, 0)
            per = _remix_bytes(spec, ns, flac)
            bufs, op = _byte_results([n_out * b for b in per], None, exact=False)
            sizes = _flat_result(None, T * n_out, np.int64)
            peaks = _flat_result(None, T * n_out, np.float32)
            sp, sz, pk = ctypes.byref(spec.c), sizes.ctypes.data, peaks.ctypes.data
        if loudness is not None:
            tail = _LoudTail(loudness, meters, limit_report, (max(T, 1),), 0 if spec is None else n_out)
            _chk(tail.pick(lib(), "dmx_tracks_infer")(self.h, mp, Q, wp, T, ap, na, ra, int(n_shifts), float(overlap), so, sp, 1 if flac else 0, op,
                                                      sz, pk, layout, cbp, None, *tail.args))
        else:
            _chk(lib().dmx_tracks_infer_rates(self.h, mp, Q, wp, T, ap, na, ra, int(n_shifts), float(overlap), so, sp, 1 if flac else 0, op, sz,
                                              pk, layout, cbp, None))
        if spec is None:
            return finish()
        outs = _flac_files(bufs, per, sizes, n_out) if flac else _pcm_results(bufs, spec.output_spec(), ns, n_out)
        if loudness is not None:
            return (outs, _cut_peaks(peaks, T, n_out)) + tail.results(T)
        return outs, _cut_peaks(peaks, T, n_out)

    def tracks_flac(self, audios, spec: RemixSpec, models=None, weights=None, n_shifts: int = 1, overlap: float = 0.25,
                    shift_offsets=None, sample_rate: int = 44100, progress=None, layout: int = LAYOUT_PLANAR, out=None, sizes=None,
                    peaks=None, loudness=None, meters: bool = False, limit_report: bool = False):
        """tracks_remix() whose outputs leave as .flac files (dmx_tracks_infer_flac): spec.encoding PCM_S16 or PCM_S24.
        Returns (files, peaks): files[t][o] the bytes of track t's output o, peaks as tracks_remix(). `out`: buffers to reuse
        (np.uint8 of n_out * flac_bound(bits, n) bytes per track); `sizes`: a flat np.int64 array of at least T * n_out."""
        if loudness is not None:  # (files, peaks, report)
            assert out is None and sizes is None and peaks is None, "loudness=: buffers to reuse are not taken"
            assert int(sample_rate) == 44100, "loudness=: the tracks are at 44100 Hz; tracks_rates() takes tracks at other rates"
            return self.tracks_rates(audios, None, spec, True, models, weights, n_shifts, overlap, shift_offsets, progress, layout, loudness,
                                     meters, limit_report)
        assert not meters and not limit_report, "meters=True and limit_report=True need loudness="
        T, ns, src, ap, na = _track_inputs(audios, layout)
        n_out = max(spec.n_out, 0)
        bits = 24 if spec.encoding == PCM_S24 else 16
        bounds = [max(flac_bound(bits, n), 0) if n >= 1 else 0 for n in ns]  # raises on a bad argument, unlike _remix_bytes
        bufs, op = _byte_results([n_out * b for b in bounds], out, exact=False)
        sizes = _flat_result(sizes, T * n_out, np.int64)
        peaks = _flat_result(peaks, T * n_out, np.float32)
        mp, Q, wp, keep = _models_weights(models, weights, self.S)
        so = _shift_array(shift_offsets, T, None if models is None else Q, n_shifts)
        cb, cbp = _progress_thunk(progress)
        _chk(lib().dmx_tracks_infer_flac(self.h, mp, Q, wp, T, ap, na, int(n_shifts), float(overlap), so, ctypes.byref(spec.c),
                                         int(sample_rate), op, sizes.ctypes.data, peaks.ctypes.data, layout, cbp, None))
        return _flac_files(bufs, bounds, sizes, n_out), _cut_peaks(peaks, T, n_out)

    def track_geometry(self, n: int, shift_offset: int) -> Tuple[int, int, int]:
        ln, st, ns = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        _chk(lib().dmx_track_geometry(self.h, n, shift_offset, ctypes.byref(ln), ctypes.byref(ns), ctypes.byref(st)))
        return ln.value, ns.value, st.value

    # ---- device-pointer API (raw addresses, e.g. torch.Tensor.data_ptr())
    def segment_device(self, d_mix: int, d_out: int, batch: int):
        _chk(lib().dmx_segment_infer_device(self.h, d_mix, d_out, batch))

    def track_stats_device(self, d_audio: int, n: int, d_stats: int):
        _chk(lib().dmx_track_stats_device(self.h, d_audio, n, d_stats))

    def track_gather_device(self, d_audio: int, n: int, d_stats: int, shift_offset: int, seg_idx: List[int], d_mix: int):
        arr = (ctypes.c_int * len(seg_idx))(*seg_idx)
        _chk(lib().dmx_track_gather_device(self.h, d_audio, n, d_stats, shift_offset, arr, len(seg_idx), d_mix))

    def track_overlap_add_device(self, d_seg_out: int, n_segments: int, n: int, shift_offset: int, d_stats: int, d_out: int,
                                 layout: int = LAYOUT_PLANAR):
        _chk(lib().dmx_track_overlap_add_device(self.h, d_seg_out, n_segments, n, shift_offset, d_stats, d_out, layout))

    # ---- debug
    def tap(self, name: str) -> Optional[np.ndarray]:
        shape = (ctypes.c_int64 * 8)()
        nd = lib().dmx_debug_tap(self.h, name.encode(), shape, None)
        if nd < 0:
            return None
        shp = [shape[i] for i in range(nd)]
        out = np.zeros(shp, np.float32)
        lib().dmx_debug_tap(self.h, name.encode(), shape, out.ctypes.data)
        return out

    # ---- one op at a time (include/demucs_hip.h; tests/test_gpu_op_parity.py)
    def plan_info(self, batch: int):
        """(number of ops, floats of the arena, floats the plan of `batch` uses, floats of its leading constants)"""
        n, a, p, k = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _chk(lib().dmx_debug_plan_info(self.h, batch, ctypes.byref(n), ctypes.byref(a), ctypes.byref(p), ctypes.byref(k)))
        return n.value, a.value, p.value, k.value

    def op_info(self, batch: int, i: int) -> dict:
        """the key=value words of dmx_debug_op_info; ranges as lists of (lo, hi)"""
        buf = ctypes.create_string_buffer(4096)
        if lib().dmx_debug_op_info(self.h, batch, i, buf, 4096) < 0:
            raise RuntimeError(f"no op {i}")
        return parse_op_info(buf.value.decode())

    def arena_fill(self, batch: int, pattern: int):
        _chk(lib().dmx_debug_arena_fill(self.h, batch, pattern & 0xFFFFFFFF))

    def arena_write(self, off: int, values: np.ndarray):
        v = np.ascontiguousarray(values, np.float32)
        _chk(lib().dmx_debug_arena_io(self.h, off, v.size, v.ctypes.data, 1))

    def arena_read(self, off: int, n: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        out = np.empty(n, np.float32) if out is None else out
        _chk(lib().dmx_debug_arena_io(self.h, off, n, out.ctypes.data, 0))
        return out

    def run_op(self, batch: int, i: int):
        _chk(lib().dmx_debug_run_op(self.h, batch, i))

    def op_cfgs(self, batch: int, i: int):
        arr = (ctypes.c_int * 16)()
        n = lib().dmx_debug_op_cfgs(self.h, batch, i, arr, 16)
        if n < 0:
            raise RuntimeError(f"op {i} is no GEMM of the plan")
        return [arr[k] for k in range(n)]

    def run_op_as(self, batch: int, i: int, cfg: int, lin_mode: int) -> Optional[dict]:
        """runs GEMM i on tile cfg; None where no such kernel exists (nothing launched), else the copy's choice"""
        buf = ctypes.create_string_buffer(512)
        rc = lib().dmx_debug_run_op_as(self.h, batch, i, cfg, lin_mode, buf, 512)
        if rc == DEBUG_NO_KERNEL:
            return None
        _chk(rc)
        return parse_op_info(buf.value.decode())

    def run_attention_as(self, batch: int, i: int, form: str) -> Optional[str]:
        """runs attention op i in form "wg64" / "wg128" / "pair"; None where that form does not exist (nothing launched), else the form"""
        rc = lib().dmx_debug_run_attention_as(self.h, batch, i, ATTENTION_FORMS.index(form))
        if rc == DEBUG_NO_KERNEL:
            return None
        _chk(rc)
        return form

    def profile(self, batch: int = 1, reps: int = 3):
        """[(op name, kernel, ms per launch, algorithmic flops, algorithmic bytes)]"""
        cap = 1 << 17
        self.profile_geometry = {}
        buf = ctypes.create_string_buffer(cap)
        n = lib().dmx_debug_profile(self.h, batch, reps, buf, cap)
        if n < 0:
            raise RuntimeError("profile failed")
        rows = []
        for ln in buf.value.decode().split("\n"):
            if not ln:
                continue
            nm, k, ms, fl, by = ln.split("\t")[:5]
            rows.append((nm, k, float(ms), float(fl), float(by)))
            self.profile_geometry[nm] = ln.split("\t")[5] if ln.count("\t") >= 5 else ""
        return rows


def track_geometry(segment_samples: int, n: int, shift_offset: int, overlap: float = 0.25) -> Tuple[int, int, int]:
    """(shifted length, number of segments, stride) of the segment loop at any overlap (dmx_track_geometry_overlap; no GPU)"""
    ln, st, ns = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    _chk(lib().dmx_track_geometry_overlap(segment_samples, n, shift_offset, float(overlap), ctypes.byref(ln), ctypes.byref(ns),
                                          ctypes.byref(st)))
    return ln.value, ns.value, st.value


def bag_weights(n_models: int, n_sources: int, weights=None):
    """(effective weights (Q, S), their fp32 column sums (S,)) of a bag (dmx_bag_weights; no GPU): weights None is the
    diagonal and needs n_models == n_sources; raises DmxError on an invalid matrix."""
    wp = None
    if weights is not None:
        warr = np.ascontiguousarray(weights, np.float32)
        assert warr.shape == (n_models, n_sources), f"weights: expected shape {(n_models, n_sources)}, got {warr.shape}"
        wp = warr.ctypes.data
    eff = np.zeros((max(n_models, 1), max(n_sources, 1)), np.float32)
    sums = np.zeros(max(n_sources, 1), np.float32)
    big = np.zeros((MAX_BAG, 8), np.float32)  # the library writes at most n_models x n_sources, both checked first
    _chk(lib().dmx_bag_weights(int(n_models), int(n_sources), wp, big.ctypes.data, sums.ctypes.data if n_sources <= sums.size else None))
    eff[...] = big.ravel()[:n_models * n_sources].reshape(n_models, n_sources)
    return eff, sums


def output_bytes(spec: OutputSpec, n: int) -> int:
    """bytes of one output of n frames under `spec` (dmx_output_bytes; no GPU); raises on an invalid spec"""
    b = lib().dmx_output_bytes(ctypes.byref(spec), n)
    if b < 0:
        raise DmxError(5, lib().dmx_last_error().decode(errors="replace"))
    return b


def pcm_views(buf: np.ndarray, spec: OutputSpec, n: int, n_out: int) -> List[np.ndarray]:
    """the n_out consecutive chunks of a dmx_tracks_infer_pcm / dmx_pcm_encode result as typed arrays (views of buf)"""
    per = output_bytes(spec, n)
    chunks = [buf[o * per:(o + 1) * per] for o in range(n_out)]
    if spec.encoding == PCM_S16:
        return [c.view("<i2").reshape(n, 2) for c in chunks]
    if spec.encoding == PCM_S24:
        return [c.reshape(n, 2, 3) for c in chunks]
    return [c.view("<f4").reshape(n, 2) for c in chunks]


def pcm_encode(planes: np.ndarray, spec: OutputSpec, device: int = 0):
    """The PCM output stage alone (dmx_pcm_encode): planes (S, 2, n) float32 -> (list of n_out arrays as tracks_pcm, peaks)."""
    planes = np.ascontiguousarray(planes, np.float32)
    S, two, n = planes.shape
    assert two == 2
    n_out = S if spec.stem < 0 else 2
    buf = np.zeros(max(n_out * max(lib().dmx_output_bytes(ctypes.byref(spec), n), 0), 1), np.uint8)
    peaks = np.zeros(n_out, np.float32)
    _chk(lib().dmx_pcm_encode(device, planes.ctypes.data, S, n, ctypes.byref(spec), buf.ctypes.data, peaks.ctypes.data))
    return pcm_views(buf, spec, n, n_out), peaks


def remix_two_stems(n_sources: int, stem: int, method: int = OTHER_ADD) -> np.ndarray:
    """the gain matrix (n_out, n_sources + 1) of demucs's --two-stems with --other-method add | minus | none
    (dmx_remix_two_stems; no GPU): OTHER_ADD [stem; the other stems added], OTHER_MINUS [stem; mixture - stem], OTHER_NONE [stem]."""
    g = np.zeros((2, 8), np.float32)  # the library writes at most 2 x (n_sources + 1), n_sources <= 6 checked first
    n_out = ctypes.c_int(0)
    _chk(lib().dmx_remix_two_stems(int(n_sources), int(stem), int(method), g.ctypes.data, ctypes.byref(n_out)))
    return g.ravel()[:n_out.value * (n_sources + 1)].reshape(n_out.value, n_sources + 1).copy()


def remix_check(n_sources: int, spec: RemixSpec):
    """validates a RemixSpec for a model of n_sources sources (dmx_remix_check; no GPU); raises DmxError naming the field"""
    if spec.gains is not None and spec.n_out >= 1:
        assert spec.gains.size >= spec.n_out * (n_sources + 1), "gains: fewer than n_out x (n_sources + 1) entries"
    _chk(lib().dmx_remix_check(int(n_sources), ctypes.byref(spec.c)))


def remix_encode(planes: np.ndarray, mix: Optional[np.ndarray], spec: RemixSpec, device: int = 0):
    """The remix output stage alone (dmx_remix_encode): planes (S, 2, n) float32, mix (2, n) float32 (the layout of the
    audio that tracks_remix() takes) or None -> (list of n_out arrays as tracks_pcm, peaks)."""
    planes = np.ascontiguousarray(planes, np.float32)
    S, two, n = planes.shape
    assert two == 2
    mi = None
    if mix is not None:
        assert mix.shape == (2, n)
        mi = np.ascontiguousarray(np.asarray(mix, np.float32).T)
    n_out = max(spec.n_out, 0)
    fb = _frame_bytes(spec.encoding)
    buf = np.zeros(max(n_out * n * fb, 1), np.uint8)
    peaks = np.zeros(max(n_out, 1), np.float32)
    _chk(lib().dmx_remix_encode(device, planes.ctypes.data, S, n, None if mi is None else mi.ctypes.data, ctypes.byref(spec.c),
                                buf.ctypes.data, peaks.ctypes.data))
    return pcm_views(buf, spec.output_spec(), n, n_out), peaks[:n_out]


LOUD_MEASURE, LOUD_MIXTURE, LOUD_EACH = 0, 1, 2  # DMX_LOUD_*
LUFS_UNMEASURABLE = -(2 ** 31)  # DMX_LUFS_UNMEASURABLE
LOUD_MIN_RATE = 4000  # DMX_LOUD_MIN_RATE
LOUD_TRUE_PEAK = 0x100  # DMX_LOUD_TRUE_PEAK, OR-ed into the mode: max_peak is a true-peak ceiling
LOUD_UNITY = 3  # DMX_LOUD_UNITY: the limiter without loudnorm (needs LOUD_LIMIT)
LOUD_LIMIT = 0x200  # DMX_LOUD_LIMIT, OR-ed into the mode: the look-ahead limiter holds max_peak, the gain is not lowered
LIMIT_ATTACK_MS, LIMIT_RELEASE_MS = 5.0, 100.0  # DMX_LIMIT_*: the times in which the reduction moves by 10 dB


class LoudnessSpec(ctypes.Structure):
    """dmx_loudness_spec: mode LOUD_*, the target in LUFS (finite, in [-70, 0]) and the ceiling of the sample peak as a linear
    value (> 0; inf: none). The default ceiling is -1 dBFS. true_peak: the ceiling is one of the true peak (-1 dBTP), the flag
    LOUD_TRUE_PEAK in the mode. limit: the flag LOUD_LIMIT (loud_encode then goes through dmx_loud_encode_limit); attack_ms and
    release_ms are the limiter's times, kept beside the struct (dmx_limiter_spec)."""
    _fields_ = [("mode", ctypes.c_int), ("target_lufs", ctypes.c_float), ("max_peak", ctypes.c_float)]
    attack_ms, release_ms = LIMIT_ATTACK_MS, LIMIT_RELEASE_MS  # of a spec that was not made by __init__ (a copy of the bytes): the defaults

    def __init__(self, mode=LOUD_MIXTURE, target_lufs=-14.0, max_peak=10.0 ** (-1.0 / 20.0), true_peak: bool = False, limit: bool = False,
                 attack_ms: float = LIMIT_ATTACK_MS, release_ms: float = LIMIT_RELEASE_MS):
        super().__init__(int(mode) | (LOUD_TRUE_PEAK if true_peak else 0) | (LOUD_LIMIT if limit else 0), float(target_lufs), float(max_peak))
        self.attack_ms, self.release_ms = float(attack_ms), float(release_ms)

    def limiter(self):
        return LimiterSpec(self.attack_ms, self.release_ms)


class LoudnessResult(ctypes.Structure):
    """dmx_loudness_result: lufs_c = rint(100 L) or LUFS_UNMEASURABLE, the gain applied, and the unquantised L (NaN)"""
    _fields_ = [("lufs_c", ctypes.c_int32), ("gain", ctypes.c_float), ("lufs", ctypes.c_double)]


LOUDNESS_DTYPE = np.dtype([("lufs_c", "<i4"), ("gain", "<f4"), ("lufs", "<f8")])  # an array of dmx_loudness_result


class MetersResult(ctypes.Structure):
    """dmx_meters_result: the true peak (linear, of the signal as measured), and in hundredths of a LU or LUFS_UNMEASURABLE the
    loudness range and the largest momentary and short-term loudness"""
    _fields_ = [("true_peak", ctypes.c_float), ("lra_c", ctypes.c_int32), ("max_momentary_c", ctypes.c_int32), ("max_short_c", ctypes.c_int32)]


METERS_DTYPE = np.dtype([("true_peak", "<f4"), ("lra_c", "<i4"), ("max_momentary_c", "<i4"), ("max_short_c", "<i4")])  # dmx_meters_result


def true_peak_filter(rate: int):
    """(F, taps): the oversampling factor at `rate` and the 12 F + 1 float32 taps of the true-peak filter (dmx_true_peak_filter; no GPU)"""
    F = ctypes.c_int(0)
    t = np.zeros(49, np.float32)
    _chk(lib().dmx_true_peak_filter(int(rate), ctypes.byref(F), t.ctypes.data))
    return F.value, t[:12 * F.value + 1].copy()


def meters_workspace_bytes(n: int) -> int:
    return lib().dmx_meters_workspace_bytes(int(n))


def meters(x: np.ndarray, rate: int, interleaved: bool = False, device: int = 0):
    """loudness() plus the meters of one stereo signal (dmx_meters): -> (LoudnessResult, e, MetersResult)"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[0] if interleaved else x.shape[1]
    assert x.shape == ((n, 2) if interleaved else (2, n))
    res, m = LoudnessResult(), MetersResult()
    e = np.zeros((2, n // ((int(rate) + 5) // 10) if rate > 0 else 0), np.float64)
    _chk(lib().dmx_meters(device, x.ctypes.data, n, int(bool(interleaved)), int(rate), ctypes.byref(res), e.ctypes.data, ctypes.byref(m)))
    return res, e, m


def loudness_coefficients(rate: int) -> np.ndarray:
    """the K-weighting's two biquads at `rate`: b0 b1 b2 a1 a2 of the shelf, then of the high-pass (dmx_loudness_coefficients; no GPU)"""
    c = np.zeros(10, np.float64)
    _chk(lib().dmx_loudness_coefficients(int(rate), c.ctypes.data))
    return c


def loudness_gain_table() -> np.ndarray:
    """T[i] = (float)10^((i - 6000) / 2000), 12001 floats (dmx_loudness_gain_table; no GPU)"""
    t = np.zeros(12001, np.float32)
    _chk(lib().dmx_loudness_gain_table(t.ctypes.data))
    return t


def loudness_check(spec: Optional[LoudnessSpec], rate: int):
    """validates a LoudnessSpec for a signal at `rate` (dmx_loudness_check; no GPU); raises DmxError naming the field"""
    _chk(lib().dmx_loudness_check(None if spec is None else ctypes.byref(spec), int(rate)))


def loudness_workspace_bytes(n: int) -> int:
    return lib().dmx_loudness_workspace_bytes(int(n))


def loudness(x: np.ndarray, rate: int, interleaved: bool = False, device: int = 0):
    """Integrated loudness of one stereo signal (dmx_loudness): x (2, n) float32 or, interleaved, (n, 2) ->
    (LoudnessResult, e) with e (2, n // hop) float64 the K-weighted energies of the 100 ms hops."""
    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[0] if interleaved else x.shape[1]
    assert x.shape == ((n, 2) if interleaved else (2, n))
    res = LoudnessResult()
    e = np.zeros((2, n // ((int(rate) + 5) // 10) if rate > 0 else 0), np.float64)
    _chk(lib().dmx_loudness(device, x.ctypes.data, n, int(bool(interleaved)), int(rate), ctypes.byref(res), e.ctypes.data))
    return res, e


def limiter_check(spec: Optional[LoudnessSpec], rate: int):
    """validates a LoudnessSpec that may carry LOUD_LIMIT or be LOUD_UNITY, with its limiter times (dmx_limiter_check; no GPU)"""
    lim = None if spec is None else spec.limiter()
    _chk(lib().dmx_limiter_check(None if spec is None else ctypes.byref(spec), None if lim is None else ctypes.byref(lim), int(rate)))


class _LoudTail:
    """what a call behind the loudness stage appends to its arguments and to its results - the one marshalling path of the
    `_loud` / `_meters` / `_limit` entry points: the spec and the loudness report; with meters=True the meters report; with
    LOUD_LIMIT in the spec's mode or limit_report=True the limiter's times and its report. shape: () or (T,)."""

    def __init__(self, loud, meters: bool, limit_report: bool, shape, n_out: int):
        self.meters, self.limit_report = bool(meters), bool(limit_report)
        self.limited = self.limit_report or bool(loud.mode & LOUD_LIMIT)
        self.report = np.zeros(shape + (n_out + 1,), LOUDNESS_DTYPE)
        self.mrep = np.zeros(shape + (n_out + 1,), METERS_DTYPE) if meters else None
        self.lrep = np.zeros(shape + (max(n_out, 1),), LIMIT_DTYPE) if self.limited else None
        self.n_out = n_out
        self._keep = (loud, loud.limiter())
        self.args = (ctypes.byref(loud), self.report.ctypes.data)
        if self.limited:
            self.args += (None if self.mrep is None else self.mrep.ctypes.data, ctypes.byref(self._keep[1]), self.lrep.ctypes.data)
        elif meters:
            self.args += (self.mrep.ctypes.data,)

    def pick(self, L, stem: str):
        plain = "" if stem == "dmx_loud_encode" else "_loud"
        return getattr(L, stem + ("_limit" if self.limited else "_meters" if self.meters else plain))

    def results(self, T=None):
        cut = (lambda a: a) if T is None else (lambda a: a[:T])
        return (cut(self.report),) + ((cut(self.mrep),) if self.meters else ()) + ((cut(self.lrep)[..., :self.n_out],) if self.limit_report else ())


def loud_encode(planes: np.ndarray, mix: np.ndarray, spec: RemixSpec, loud: LoudnessSpec, rate: int, device: int = 0, meters: bool = False,
                limit_report: bool = False):
    """The remix output stage behind the loudness stage (dmx_loud_encode): planes (S, 2, n) float32, mix (2, n) float32 ->
    (list of n_out arrays as tracks_pcm, peaks, report) with report a (n_out + 1,) array of LOUDNESS_DTYPE, the mixture last.
    meters=True (dmx_loud_encode_meters): (outs, peaks, report, meters), meters a (n_out + 1,) array of METERS_DTYPE.
    A spec with LOUD_LIMIT, or limit_report=True, goes through dmx_loud_encode_limit; limit_report=True returns a (n_out,) array of
    LIMIT_DTYPE last."""
    planes = np.ascontiguousarray(planes, np.float32)
    S, two, n = planes.shape
    assert two == 2 and mix is not None and mix.shape == (2, n)
    mi = np.ascontiguousarray(np.asarray(mix, np.float32).T)
    n_out = max(spec.n_out, 0)
    buf = np.zeros(max(n_out * n * _frame_bytes(spec.encoding), 1), np.uint8)
    peaks = np.zeros(max(n_out, 1), np.float32)
    tail = _LoudTail(loud, meters, limit_report, (), n_out)
    a = tail.args
    _chk(tail.pick(lib(), "dmx_loud_encode")(device, planes.ctypes.data, S, n, mi.ctypes.data, ctypes.byref(spec.c), a[0], int(rate), buf.ctypes.data,
                                             peaks.ctypes.data, *a[1:]))
    return (pcm_views(buf, spec.output_spec(), n, n_out), peaks[:n_out]) + tail.results()


class LimiterSpec(ctypes.Structure):
    """dmx_limiter_spec: the attack and release times in ms, finite and in [0.1, 10000]"""
    _fields_ = [("attack_ms", ctypes.c_float), ("release_ms", ctypes.c_float)]

    def __init__(self, attack_ms=LIMIT_ATTACK_MS, release_ms=LIMIT_RELEASE_MS):
        super().__init__(float(attack_ms), float(release_ms))


class LimitResult(ctypes.Structure):
    """dmx_limit_result: the sample peak and (with true_peak, else 0) the true peak of the limited signal, the largest reduction
    in units of 1 / 65536 octave, and the frames whose reduction is not 0"""
    _fields_ = [("peak_out", ctypes.c_float), ("true_peak_out", ctypes.c_float), ("max_reduction", ctypes.c_int32),
                ("limited_frames", ctypes.c_int64)]


LIMIT_DTYPE = np.dtype([("peak_out", "<f4"), ("true_peak_out", "<f4"), ("max_reduction", "<i4"), ("limited_frames", "<i8")],
                       align=True)  # an array of dmx_limit_result


def limiter_tables():
    """(LUT int32 [4096], THI float32 [385], TLO float32 [4096]) of the limiter (dmx_limiter_tables; no GPU)"""
    lut, thi, tlo = np.zeros(4096, np.int32), np.zeros(385, np.float32), np.zeros(4096, np.float32)
    _chk(lib().dmx_limiter_tables(lut.ctypes.data, thi.ctypes.data, tlo.ctypes.data))
    return lut, thi, tlo


def limiter_slopes(rate: int, attack_ms: float = LIMIT_ATTACK_MS, release_ms: float = LIMIT_RELEASE_MS):
    """(qa, qr) in units per frame (dmx_limiter_slopes; no GPU); raises DmxError naming the field"""
    qa, qr = ctypes.c_int32(0), ctypes.c_int32(0)
    _chk(lib().dmx_limiter_slopes(int(rate), float(attack_ms), float(release_ms), ctypes.byref(qa), ctypes.byref(qr)))
    return qa.value, qr.value


def limiter_workspace_bytes(n: int) -> int:
    return lib().dmx_limiter_workspace_bytes(int(n))


def limit(x: np.ndarray, rate: int, max_peak: float, gain: float = 1.0, true_peak: bool = False, attack_ms: float = LIMIT_ATTACK_MS,
          release_ms: float = LIMIT_RELEASE_MS, interleaved: bool = False, device: int = 0):
    """The look-ahead peak limiter alone on one stereo signal (dmx_limit): x (2, n) float32 or, interleaved, (n, 2) ->
    (M int32 (n,) the required reduction, G float32 (n,) the gain plane, LimitResult). The limited signal is (gain * x) * G."""
    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[0] if interleaved else x.shape[1]
    assert x.shape == ((n, 2) if interleaved else (2, n))
    M, G, res = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32), LimitResult()
    spec = LimiterSpec(attack_ms, release_ms)
    _chk(lib().dmx_limit(device, x.ctypes.data, n, int(bool(interleaved)), int(rate), float(gain), float(max_peak), int(bool(true_peak)),
                         ctypes.byref(spec), M.ctypes.data, G.ctypes.data, ctypes.byref(res)))
    return M[:n], G[:n], res


def flac_bound(bits: int, n: int) -> int:
    """an upper bound of the .flac file of n frames of `bits` (16 | 24) bit stereo (dmx_flac_bound; no GPU); raises on a bad argument"""
    b = lib().dmx_flac_bound(int(bits), int(n))
    if b < 0:
        raise DmxError(5, f"dmx_flac_bound: bad argument (bits {bits}, n {n})")
    return b


def flac_encode(pcm: np.ndarray, bits: int, sample_rate: int = 44100, device: int = 0, level: int = 0) -> bytes:
    """The FLAC stage alone (dmx_flac_encode / dmx_flac_encode_level): pcm as the PCM stage returns it - np.int16 (n, 2) for
    bits 16, np.uint8 (n, 2, 3) for bits 24 - -> the bytes of the .flac file. level 0 | 1 | 2: FIXED predictors alone, + LPC
    order 8, + LPC orders 8 and 12."""
    pcm = np.ascontiguousarray(pcm)
    if bits == 16:
        assert pcm.dtype == np.int16 and pcm.ndim == 2 and pcm.shape[1] == 2
    else:
        assert pcm.dtype == np.uint8 and pcm.ndim == 3 and pcm.shape[1:] == (2, 3)
    n = pcm.shape[0]
    out = np.zeros(max(lib().dmx_flac_bound(int(bits), n), 1), np.uint8)
    size = ctypes.c_int64(0)
    if level == 0:
        _chk(lib().dmx_flac_encode(device, pcm.ctypes.data, int(bits), n, int(sample_rate), out.ctypes.data, ctypes.byref(size)))
    else:
        _chk(lib().dmx_flac_encode_level(device, pcm.ctypes.data, int(bits), n, int(sample_rate), int(level), out.ctypes.data,
                                         ctypes.byref(size)))
    return bytes(out[:size.value])


class FlacInfo(ctypes.Structure):
    """dmx_flac_info: what dmx_flac_probe reads from a file's header"""
    _fields_ = [("sample_rate", ctypes.c_int), ("channels", ctypes.c_int), ("bits", ctypes.c_int), ("total_samples", ctypes.c_int64),
                ("min_block", ctypes.c_int), ("max_block", ctypes.c_int), ("min_frame", ctypes.c_int), ("max_frame", ctypes.c_int),
                ("variable_blocking", ctypes.c_int), ("first_frame", ctypes.c_int64)]


FLAC_OK, FLAC_BROKEN, FLAC_TOO_MANY_CANDIDATES = 0, 1, 2


def flac_probe(data) -> FlacInfo:
    """the header of a .flac file's bytes (dmx_flac_probe; no GPU); raises DmxError with the probe's message"""
    buf = np.frombuffer(bytes(data), np.uint8)
    info = FlacInfo()
    _chk(lib().dmx_flac_probe(buf.ctypes.data if buf.size else None, int(buf.size), ctypes.byref(info)))
    return info


def flac_decode(data, encoding: int = PCM_F32, device: int = 0):
    """The FLAC input stage alone (dmx_flac_decode): the bytes of a .flac file -> (samples, status, good, info). samples:
    np.float32 (n, 2) for PCM_F32, np.int16 (n, 2) for PCM_S16, np.uint8 (n, 2, 3) for PCM_S24; [good, n) is zero."""
    buf = np.frombuffer(bytes(data), np.uint8)
    info = flac_probe(buf)
    n = int(info.total_samples)
    out = np.zeros((n, 2), np.float32) if encoding == PCM_F32 else np.zeros((n, 2), np.int16) if encoding == PCM_S16 \
        else np.zeros((n, 2, 3), np.uint8)
    status = np.zeros(2, np.int64)
    _chk(lib().dmx_flac_decode(device, buf.ctypes.data, int(buf.size), ctypes.byref(info), int(encoding), out.ctypes.data,
                               status.ctypes.data))
    return out, int(status[0]), int(status[1]), info


def resample_length(n_in: int, rate_in: int, rate_out: int) -> int:
    L = lib()
    L.dmx_resample_length.restype = ctypes.c_int64
    L.dmx_resample_length.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    return L.dmx_resample_length(n_in, rate_in, rate_out)


def resample_ready(n_in_final: int, n_in: int, rate_in: int, rate_out: int, n_out: int) -> int:
    """dmx_resample_ready (pure host): the outputs that are final once the inputs [0, n_in_final) are; -1: invalid argument"""
    return lib().dmx_resample_ready(n_in_final, n_in, rate_in, rate_out, n_out)


def resample_filter(rate_in: int, rate_out: int):
    """(up, down, taps) of the polyphase filter of csrc/resample.hip (host function, no GPU)."""
    L = lib()
    L.dmx_resample_filter.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int]
    up, down, nt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _chk(L.dmx_resample_filter(rate_in, rate_out, ctypes.byref(up), ctypes.byref(down), ctypes.byref(nt), None, 0))
    taps = np.zeros(nt.value, np.float32)
    _chk(L.dmx_resample_filter(rate_in, rate_out, None, None, None, taps.ctypes.data, nt.value))
    return up.value, down.value, taps


def resample(x: np.ndarray, rate_in: int, rate_out: int, interleaved: bool = False, device: int = 0) -> np.ndarray:
    """x (planes, n) planar or (n, planes) interleaved float32 -> the same layout at rate_out (GPU, host buffers)."""
    L = lib()
    L.dmx_resample.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               ctypes.c_void_p]
    x = np.ascontiguousarray(x, np.float32)
    n, planes = (x.shape[0], x.shape[1]) if interleaved else (x.shape[1], x.shape[0])
    m = resample_length(n, rate_in, rate_out)
    if m < 0:
        raise ValueError(f"invalid rates {rate_in} -> {rate_out}")
    out = np.zeros((m, planes) if interleaved else (planes, m), np.float32)
    _chk(L.dmx_resample(device, x.ctypes.data, n, planes, 1 if interleaved else 0, rate_in, rate_out, out.ctypes.data))
    return out


def engine_partition(n_segments, n_devices):
    """[(device l) -> [(model, g0, g1), ...]]: the contiguous balanced dealing of csrc/engine.cpp."""
    M = len(n_segments)
    ns = (ctypes.c_int * M)(*n_segments)
    out = (ctypes.c_int * (n_devices * M * 2))()
    L = lib()
    L.dmx_engine_partition.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    _chk(L.dmx_engine_partition(ns, M, n_devices, out))
    res = []
    for l in range(n_devices):
        res.append([(m, out[(l * M + m) * 2], out[(l * M + m) * 2 + 1]) for m in range(M)
                    if out[(l * M + m) * 2 + 1] > out[(l * M + m) * 2]])
    return res


class Engine:
    """Several GPUs and / or a bag of models in one process (csrc/engine.cpp): demucs_inference with the
    (model, segment) items sharded over `devices`; `devices` may repeat an id (logical devices on one GPU)."""

    def __init__(self, model_files, devices=None, max_batch: int = 4, transport: int = TRANSPORT_AUTO, finish: Optional[int] = None):
        files = (ctypes.c_char_p * len(model_files))(*[f.encode() for f in model_files])
        devs = (ctypes.c_int * len(devices))(*devices) if devices else None
        self.h = ctypes.c_void_p()
        _chk(lib().dmx_engine_create(files, len(model_files), devs, len(devices) if devices else 0, max_batch, transport,
                                     ctypes.byref(self.h)))
        self.S = lib().dmx_engine_n_sources(self.h)
        self.n_models = lib().dmx_engine_n_models(self.h)
        self.n_devices = lib().dmx_engine_n_devices(self.h)
        self.transport = lib().dmx_engine_transport(self.h)
        if finish is not None:
            self.set_finish(finish)

    def set_finish(self, finish: int):
        """FINISH_ROOT: blocks gathered and overlap-added on the first device; FINISH_OWNER: every device finishes
        the stretch of the track its segments cover (only segment tails are exchanged). Same bits."""
        _chk(lib().dmx_engine_set_finish(self.h, finish))

    @property
    def finish(self) -> int:
        return lib().dmx_engine_finish(self.h)

    def close(self):
        if self.h:
            lib().dmx_engine_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def track(self, audio: np.ndarray, shift_offsets, progress=None, out: Optional[np.ndarray] = None,
              layout: int = LAYOUT_PLANAR) -> np.ndarray:
        """audio (2, n) planar -> (S, 2, n); one shift offset per model. `out`: reuse a result buffer.
        layout=LAYOUT_EIGEN passes the track and receives the result through the C ABI as Eigen column-major
        images (what the C++ shim does); the arrays seen by the caller are the same."""
        audio = np.ascontiguousarray(audio, np.float32)
        n = audio.shape[1]
        so = (ctypes.c_int * self.n_models)(*shift_offsets)
        cb, cbp = _progress_thunk(progress)
        if layout == LAYOUT_EIGEN:
            a = np.ascontiguousarray(audio.T)  # [n][2] == column-major 2 x n
            img = np.zeros((n, 2, self.S), np.float32)  # flat index s + S*(c + 2*i)
            _chk(lib().dmx_engine_track_infer(self.h, a.ctypes.data, n, so, img.ctypes.data, LAYOUT_EIGEN, cbp, None))
            res = np.ascontiguousarray(img.transpose(2, 1, 0))
            if out is not None:
                out[...] = res
                return out
            return res
        if out is None:
            out = np.zeros((self.S, 2, n), np.float32)
        assert out.shape == (self.S, 2, n) and out.dtype == np.float32 and out.flags.c_contiguous
        _chk(lib().dmx_engine_track_infer(self.h, audio.ctypes.data, n, so, out.ctypes.data, LAYOUT_PLANAR, cbp, None))
        return out

