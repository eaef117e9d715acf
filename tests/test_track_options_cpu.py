"""The shifts ensemble and segment overlap (include/demucs_hip.h dmx_tracks_infer_opts, dmx_track_geometry_overlap): the
segment-loop geometry at any overlap and the argument checks that run before any GPU work. No GPU needed."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMX_ERR_ARG = 5
OVERLAPS = [0.0, 0.1, 0.25, 0.5, 0.75, 0.9]
SEGMENTS = [8000, 16384, 343980]


@pytest.fixture(scope="module")
def dmx():
    so = os.path.join(ROOT, "demucs_cpp_amd", "lib", "libdemucs_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", ROOT, "demucs_cpp_amd/lib/libdemucs_hip.so"], stdout=subprocess.DEVNULL)
    from demucs_cpp_amd import binding
    return binding


def _stride(seg, ov):
    return int(np.float32(np.float32(1) - np.float32(ov)) * np.float32(seg))


def test_header_constants(dmx):
    hdr = open(os.path.join(ROOT, "include", "demucs_hip.h")).read()
    assert "#define DMX_MAX_SHIFTS 32" in hdr
    assert "dmx_tracks_infer_opts" in dmx.EXPORTS and "dmx_track_geometry_overlap" in dmx.EXPORTS


@pytest.mark.parametrize("seg", SEGMENTS)
@pytest.mark.parametrize("ov", OVERLAPS)
def test_geometry_table(dmx, seg, ov):
    st = _stride(seg, ov)
    for n, shift in ((2, 0), (2, 22049), (seg, 4033), (7 * seg + 13, 12436), (10_584_000, 0)):
        ln, nseg, stride = dmx.track_geometry(seg, n, shift, ov)
        assert stride == st, (seg, ov, stride, st)
        assert ln == n + 22050 - shift
        assert nseg == math.ceil(ln / stride)


def test_geometry_strides_at_the_test_segment_and_the_production_default(dmx):
    assert [dmx.track_geometry(8000, 100, 0, ov)[2] for ov in (0.0, 0.25, 0.5, 0.75, 0.9)] == [8000, 6000, 4000, 2000, 800]
    assert dmx.track_geometry(343980, 10_584_000, 4033, 0.25)[1:] == (42, 257985)  # a 4-minute track, as dmx_track_geometry
    assert dmx.track_geometry(343980, 10_584_000, 4033)[1:] == (42, 257985)  # the default overlap


@pytest.mark.parametrize("ov", [-0.01, 0.9001, 0.95, 1.0, float("nan"), float("inf")])
def test_geometry_rejects_overlap_outside_the_range(dmx, ov):
    L = dmx.lib()
    ln, st, ns = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    rc = L.dmx_track_geometry_overlap(8000, 1000, 0, ov, ctypes.byref(ln), ctypes.byref(ns), ctypes.byref(st))
    assert rc == DMX_ERR_ARG
    assert "overlap" in L.dmx_last_error().decode()


@pytest.mark.parametrize("shift", [-1, 22050, 100000])
def test_geometry_rejects_a_shift_out_of_range(dmx, shift):
    with pytest.raises(dmx.DmxError, match="shift_offset"):
        dmx.track_geometry(8000, 1000, shift, 0.25)


def test_geometry_rejects_empty_tracks_and_segments(dmx):
    for seg, n in ((0, 100), (8000, 0), (-5, 100)):
        with pytest.raises(dmx.DmxError, match="dmx_track_geometry_overlap"):
            dmx.track_geometry(seg, n, 0, 0.25)


def test_tracks_infer_opts_rejects_a_null_context_before_anything(dmx):
    L = dmx.lib()
    a = np.zeros((2, 100), np.float32)
    o = np.zeros((4, 2, 100), np.float32)
    ap = (ctypes.c_void_p * 1)(a.ctypes.data)
    op = (ctypes.c_void_p * 1)(o.ctypes.data)
    na = (ctypes.c_int64 * 1)(100)
    rc = L.dmx_tracks_infer_opts(None, 1, ap, na, 2, 0.25, None, op, dmx.LAYOUT_PLANAR, None, None)
    assert rc == DMX_ERR_ARG
    msg = L.dmx_last_error().decode()
    assert "dmx_tracks_infer_opts" in msg and "null context" in msg, msg
    assert not o.any()
