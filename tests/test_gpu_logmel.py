"""The log-mel stage on the GPU (csrc/logmel.hip): binding.logmel against tests/logmel_spec.py elementwise,
|out - ref| <= 2^-24 |ref| + 8 D. The first term is the one rounding to fp32. D is the largest difference, in output units, between
the specification's two binary64 routes (np.fft.rfft, and the explicit product with the cos / sin matrix), measured on the CPU with
the committed specification and written below; the factor 8 covers a third summation order, the MFMA's."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logmel_spec  # noqa: E402
from demucs_cpp_amd import binding as dmx  # noqa: E402

pytestmark = pytest.mark.gpu

W80 = dict(sr=16000, n_fft=400, hop=160, n_mels=80, log_mode=dmx.LOG_WHISPER)
DB = dict(log_mode=dmx.LOG_DB, amin=1e-10, top_db=80.0)
# name: spec fields, planes, N, input ("noise" | "silent": plane 1 is zero | "steps": 1e-5 of the amplitude in the second half), D
CASES = {
    # three chunks of 40 frames, the last 3000 of 6400 samples; 40 frames fill no tile; a sine on plane 0; five mel tiles
    "whisper_chunks": (dict(W80, chunk_frames=40), 3, 2 * 6400 + 3000, "silent", 5.551115123125783e-15),
    # eight mel tiles, 201 bins in 13 tiles; both halves in one chunk, so the clamp at max - 8 acts
    "whisper128_steps": (dict(W80, n_mels=128), 1, 7013, "steps", 7.993605777301127e-15),
    "db_steps": (dict(W80, **DB), 3, 7013, "steps", 2.4158453015843406e-13),
    "db_silent": (dict(W80, **DB, chunk_frames=25), 3, 9000, "silent", 1.3500311979441904e-13),
    # the smallest transform; fmin and fmax inside the band leave zero blocks in W
    "nfft64_band": (dict(sr=8000, n_fft=64, hop=16, n_mels=20, fmin=300.0, fmax=3000.0, log_mode=dmx.LOG_NONE), 2, 1003, "noise", 9.71445146547012e-17),
    # reflection covers most of the signal; HTK, no norm; a one-wave tile
    "nfft2048_short": (dict(sr=22050, n_fft=2048, hop=512, n_mels=128, mel_scale=dmx.MEL_HTK, mel_norm=dmx.MEL_NORM_NONE, **DB), 1, 1030,
                       "noise", 2.6423307986078726e-14),
    # hop = n_fft: no overlap; 71 frames, two tiles
    "hop_is_nfft": (dict(sr=16000, n_fft=128, hop=128, n_mels=40, log_mode=dmx.LOG_DB, amin=1e-10, top_db=0.0), 1, 70 * 128 + 5, "noise", 4.973799150320701e-14),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """seeded Gaussian noise of amplitude 0.1 (no deep spectral nulls), a sine added on plane 0; the reference, computed once"""
    fields, P, N, kind, _ = CASES[name]
    spec = dmx.LogmelSpec(**fields)
    rng = np.random.default_rng(sorted(CASES).index(name))
    x = 0.1 * rng.standard_normal((P, N))
    x[0] += 0.2 * np.sin(2 * np.pi * 440.0 / spec.sr * np.arange(N))
    if kind == "silent":
        x[1] = 0.0
    if kind == "steps":
        x[:, N // 2:] *= 1e-5
    x = x.astype(np.float32)
    ref = logmel_spec.logmel(x, spec)
    x.setflags(write=False), ref.setflags(write=False)
    return spec, x, ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_logmel_equals_the_specification(name):
    _, P, N, kind, D = CASES[name]
    spec, x, ref = case(name)
    out = dmx.logmel(x, spec)
    assert out.shape == ref.shape and out.dtype == np.float32
    err = np.abs(out.astype(np.float64) - ref)
    print(name, "max error", err.max(), "D", D, "worst error / bound", (err / (2.0 ** -24 * np.abs(ref) + 8 * D + 1e-300)).max())
    assert np.all(err <= 2.0 ** -24 * np.abs(ref) + 8 * D)
    if kind == "silent":  # exactly -1.5, or exactly 10 log10 amin
        assert np.all(out[1] == (-1.5 if spec.log_mode == dmx.LOG_WHISPER else -100.0))
    if kind == "steps":  # the clamp acts: the quiet half sits on the floor
        assert (ref[0] == ref[0].min()).sum() > ref[0].size // 4


def test_equal_bits_twice_on_a_stream_of_the_caller_and_from_stems():
    import torch
    spec, x, _ = case("whisper_chunks")
    P, N = x.shape
    first, again = dmx.logmel(x, spec), dmx.logmel(x, spec)
    assert first.tobytes() == again.tobytes()
    stride = N + 7  # planes apart by more than their length
    nbytes = dmx.logmel_workspace_bytes(spec, P, N)
    d_x = torch.zeros((P, stride), dtype=torch.float32, device="cuda")
    d_x[:, :N] = torch.tensor(x).cuda()
    d_out, d_work = torch.empty(first.shape, dtype=torch.float32, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    args = [0, d_x.data_ptr(), P, N, stride, ctypes.byref(spec), d_out.data_ptr(), d_work.data_ptr()]
    with pytest.raises(dmx.DmxError, match="work_bytes"):
        dmx._chk(dmx.lib().dmx_logmel_device(*args, nbytes - 1, stream.cuda_stream))
    dmx._chk(dmx.lib().dmx_logmel_device(*args, nbytes, stream.cuda_stream))
    stream.synchronize()
    assert d_out.cpu().numpy().tobytes() == first.tobytes()
    # a 44.1 kHz stereo pair: the fp32 mono fold, dmx_resample, the stage
    stems = (0.1 * np.random.default_rng(7).standard_normal((2, 2, 20000))).astype(np.float32)
    mono = np.float32(0.5) * (stems[:, 0] + stems[:, 1])
    want = dmx.logmel(dmx.resample(mono, 44100, spec.sr), spec)
    assert dmx.logmel_from_stems(stems, 44100, spec).tobytes() == want.tobytes()
