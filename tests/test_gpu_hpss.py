"""Harmonic/percussive split on the GPU (csrc/hpss.hip) against tests/hpss_spec.py: the medians and the
masks of the filter kernel as bits, the stage by max |out - ref| / max |ref| within 8 x the distance of the specification's
own float32 mode (STFT and inverse in single precision through pocketfft) from its complex128 mode, computed per case."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hpss_spec  # noqa: E402
from demucs_cpp_amd import binding as dmx  # noqa: E402

pytestmark = pytest.mark.gpu

TF, TB = dmx.hpss_geometry()  # the tile of the filter kernel: frames, bins (a pure host function)
# planes, frames, bins, kernel_h, kernel_p
SHAPES = {
    "cell": (1, 1, 1, 31, 31),
    "folds": (1, 5, 7, 31, 31),          # the extent is below the half window: repeated reflection
    "past_a_tile": (2, TF + 1, TB + 1, 31, 31),
    "stage_row": (1, 40, 2049, 17, 3),
}
SPARE, SENTINEL = 3, -7.5  # row = bins + SPARE; what the spare columns of the outputs hold and must keep


@functools.lru_cache(maxsize=None)
def magnitudes(shape, ties):
    planes, frames, bins = SHAPES[shape][:3]
    rng = np.random.default_rng(sorted(SHAPES).index(shape))
    S = rng.integers(0, 4, (planes, frames, bins)).astype(np.float32) if ties else np.abs(rng.standard_normal((planes, frames, bins))).astype(np.float32)
    if shape == "past_a_tile":
        S[:, :20, :40] = 0.0  # inside it both medians are zero: the z < FLT_MIN rule of the masks
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def spec_medians(shape, ties):
    kh, kp = SHAPES[shape][3:]
    H, P = zip(*(hpss_spec.medians(S, kh, kp) for S in magnitudes(shape, ties)))
    return np.stack(H), np.stack(P)


def run_filter(S, spec, what):
    """S as spectra with im = 0 (so the magnitude is re, exactly) in rows of bins + SPARE; the two outputs' columns and spares"""
    import torch
    planes, frames, bins = S.shape
    row = bins + SPARE
    D = np.full((planes, frames, row), 1e30, np.complex64)
    D[..., :bins] = S
    d_spec = torch.from_numpy(D).cuda()
    a, b = (torch.full((planes, frames, row), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(2))
    dmx.hpss_filter(d_spec.data_ptr(), planes, frames, bins, row, spec, what, a.data_ptr(), b.data_ptr(), torch.cuda.current_stream().cuda_stream)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert (a[..., bins:] == SENTINEL).all() and (b[..., bins:] == SENTINEL).all()
    return a[..., :bins], b[..., :bins]


@pytest.mark.parametrize("ties", [False, True], ids=["gaussian", "ties"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_medians_equal_the_specification_as_bits(shape, ties):
    kh, kp = SHAPES[shape][3:]
    H, P = run_filter(magnitudes(shape, ties), dmx.HpssSpec(kh, kp), dmx.HPSS_MEDIANS)
    refH, refP = spec_medians(shape, ties)
    assert H.tobytes() == refH.tobytes() and P.tobytes() == refP.tobytes()


@pytest.mark.parametrize("margins", [(1.0, 1.0), (2.0, 3.0)])
@pytest.mark.parametrize("power", [1, 2])
def test_masks_equal_the_specification_as_bits(power, margins):
    shape = "past_a_tile"
    Mh, Mp = run_filter(magnitudes(shape, False), dmx.HpssSpec(31, 31, power, *margins), dmx.HPSS_MASKS)
    refH, refP = spec_medians(shape, False)
    refMh, refMp = hpss_spec.masks(refH, refP, power, *margins)
    assert (np.maximum(refH, refP) == 0).any() and (refMh[np.maximum(refH, refP) == 0] == (0.5 if margins == (1.0, 1.0) else 0.0)).all()
    assert Mh.tobytes() == refMh.tobytes() and Mp.tobytes() == refMp.tobytes()


N = 36 * 1024 + 5  # more than 31 frames, more than one chunk of the inverse
# J, C, n, margins, residual
CASES = {"short_mono": (1, 1, 3000, (1.0, 1.0), 0), "stereo": (2, 2, N, (1.0, 1.0), 0), "residual": (1, 2, N, (2.0, 2.0), 1)}


@functools.lru_cache(maxsize=None)
def case(name):
    """the input (a tone, clicks and a noise floor 40 dB under the peak, which keeps every median far above the rounding of an
    fp32 STFT), the reference and the specification's own float32 distance from it"""
    J, C, n, margins, residual = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    t = np.arange(n)
    x = 0.5 * np.sin(2 * np.pi * (440.0 + 110.0 * np.arange(J * C).reshape(J, C, 1)) / 44100.0 * t) + 0.01 * rng.standard_normal((J, C, n))
    x[..., 700::2900] += 0.5
    x = x.astype(np.float32)
    ref = hpss_spec.hpss(x, margin_h=margins[0], margin_p=margins[1], residual=bool(residual))
    d = distance(hpss_spec.hpss(x, margin_h=margins[0], margin_p=margins[1], residual=bool(residual), dtype=np.float32), ref)
    for a in (x, ref):
        a.setflags(write=False)
    return x, ref, d


def distance(out, ref):
    return float(np.abs(out.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_stage_equals_the_specification(name):
    J, C, n, margins, residual = CASES[name]
    x, ref, d = case(name)
    out = dmx.hpss(x, dmx.HpssSpec(margin_h=margins[0], margin_p=margins[1], residual=residual))
    err = distance(out, ref)
    print(name, "max error / max |ref|", err, "the specification's float32 mode", d, "bound", 8 * d)
    assert out.shape == ref.shape == (J, 2 + residual, C, n) and out.dtype == np.float32
    assert err <= 8 * d
    if margins == (1.0, 1.0):  # the masks add up to one
        back = distance(out[:, 0] + out[:, 1], x)
        print(name, "harmonic + percussive against the input", back)
        assert back <= 8 * d
    else:
        assert np.abs(out[:, 2]).max() > 1e-3  # the margins leave a residual


def test_equal_bits_on_a_stream_of_the_caller_and_in_the_timed_call():
    import torch
    name = "residual"
    J, C, n, margins, residual = CASES[name]
    x, _, _ = case(name)
    s = dmx.HpssSpec(margin_h=margins[0], margin_p=margins[1], residual=residual)
    first, again = dmx.hpss(x, s), dmx.hpss(x, s)
    assert first.tobytes() == again.tobytes()
    nbytes = dmx.hpss_workspace_bytes(s, J, C, n)
    d_x = torch.tensor(x).cuda()
    d_out, d_work = torch.empty((J, 3, C, n), device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    args = [0, d_x.data_ptr(), J, C, n, n, ctypes.byref(s), d_out.data_ptr(), n, d_work.data_ptr()]
    with pytest.raises(dmx.DmxError, match="work_bytes") as e:
        dmx._chk(dmx.lib().dmx_hpss_device(*args, nbytes - 1, stream.cuda_stream))
    assert e.value.code == 5  # DMX_ERR_ARG
    dmx._chk(dmx.lib().dmx_hpss_device(*args, nbytes, stream.cuda_stream))
    stream.synchronize()
    assert d_out.cpu().numpy().tobytes() == first.tobytes()
    d_out.zero_()
    ms = (ctypes.c_float * 4)(*([-1.0] * 4))
    dmx._chk(dmx.lib().dmx_hpss_device_timed(*args, nbytes, None, ms))
    got = list(ms)
    assert all(np.isfinite(v) and v >= 0.0 for v in got[:3]) and got[3] == -1.0
    assert d_out.cpu().numpy().tobytes() == first.tobytes()
