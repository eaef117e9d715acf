"""The log-mel stage without a GPU: the pure host functions of the library against tests/logmel_spec.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logmel_spec  # noqa: E402
from demucs_cpp_amd import binding as dmx  # noqa: E402

HTK_BAND = dict(sr=22050, n_fft=2048, hop=512, n_mels=128, fmin=300.0, fmax=9000.0, mel_scale=dmx.MEL_HTK, mel_norm=dmx.MEL_NORM_NONE)


@pytest.mark.parametrize("spec", [dmx.logmel_preset("whisper"), dmx.logmel_preset("whisper128"), dmx.logmel_preset("librosa"),
                                  dmx.LogmelSpec(**HTK_BAND), dmx.LogmelSpec(sr=8000, n_fft=64, hop=16, n_mels=20, fmin=300.0, fmax=3000.0)])
def test_filters_agree_with_the_specification(spec):
    W, ref = dmx.logmel_filters(spec), logmel_spec.filters(spec)
    # a weight is (bin - hz) / dhz * norm: the band edges hz carry a few roundings of log / exp at up to fmax, so their error
    # is below 8 eps fmax, and the division by dhz >= min dhz and the norm scale it: 16 eps fmax / min dhz, times the largest norm
    hz = logmel_spec.mel_to_hz(np.linspace(logmel_spec.hz_to_mel(spec.fmin, spec.mel_scale), logmel_spec.hz_to_mel(spec.fmax, spec.mel_scale),
                                           spec.n_mels + 2), spec.mel_scale)
    norm = (2.0 / (hz[2:] - hz[:-2])).max() if spec.mel_norm == dmx.MEL_NORM_SLANEY else 1.0
    bound = 16 * np.finfo(np.float64).eps * spec.fmax / np.diff(hz).min() * norm
    assert W.shape == ref.shape and np.abs(W - ref).max() <= bound
    assert (W > 0).any(axis=1).all()  # no empty filter in these


def test_presets_frames_refusals_and_the_tile():
    w, w128, lib = dmx.logmel_preset("whisper"), dmx.logmel_preset("whisper128"), dmx.logmel_preset("librosa")
    assert (w.sr, w.n_fft, w.hop, w.n_mels, w.fmin, w.fmax, w.chunk_frames, w.log_mode) == (16000, 400, 160, 80, 0.0, 8000.0, 3000, dmx.LOG_WHISPER)
    assert (w.mel_scale, w.mel_norm, w128.n_mels, w128.chunk_frames) == (dmx.MEL_SLANEY, dmx.MEL_NORM_SLANEY, 128, 3000)
    assert (lib.sr, lib.n_fft, lib.hop, lib.n_mels, lib.log_mode, lib.amin, lib.top_db, lib.chunk_frames) == (22050, 2048, 512, 128, dmx.LOG_DB, 1e-10, 80.0, 0)
    with pytest.raises(dmx.DmxError, match="name"):
        dmx.logmel_preset("kaldi")
    assert dmx.logmel_frames(w, 16000 * 70) == (3, 3000) and dmx.logmel_frames(w, 1) == (1, 3000)
    assert dmx.logmel_frames(lib, 1025) == (1, 3) and dmx.logmel_frames(lib, 22050) == (1, 44)
    for field, spec, n in (("n_fft", dmx.LogmelSpec(n_fft=408), -1), ("n_fft", dmx.LogmelSpec(n_fft=4096), -1), ("hop", dmx.LogmelSpec(hop=401), -1),
                           ("hop", dmx.LogmelSpec(hop=0), -1), ("n_mels", dmx.LogmelSpec(n_mels=129), -1), ("fmin", dmx.LogmelSpec(fmax=8000.5), -1),
                           ("fmin", dmx.LogmelSpec(fmin=8000.0), -1), ("mel_scale", dmx.LogmelSpec(mel_scale=2), -1),
                           ("mel_norm", dmx.LogmelSpec(mel_norm=2), -1), ("log_mode", dmx.LogmelSpec(log_mode=3), -1),
                           ("chunk_frames", dmx.LogmelSpec(chunk_frames=-1), -1), ("chunk_frames", dmx.LogmelSpec(chunk_frames=1), -1),
                           ("amin", dmx.LogmelSpec(log_mode=dmx.LOG_DB, amin=0.0), -1), ("n 1024", lib, 1024), ("n 0", w, 0)):
        with pytest.raises(dmx.DmxError) as e:
            dmx.logmel_check(spec, n)
        assert e.value.code == 5 and field in str(e.value)
        assert dmx.logmel_workspace_bytes(spec, 1, max(n, 0)) == -1
    dmx.logmel_check(lib, 1025)
    # the tile: a divisor of n_fft as the slab depth, whole waves, inside the 160 KB of a workgroup at the extremes
    for n_fft in (64, 400, 2048):
        for hop in (1, 3, 61, 64, n_fft // 4, n_fft - 1, n_fft):
            ft, depth, lds = dmx.logmel_geometry(dmx.LogmelSpec(n_fft=n_fft, hop=hop))
            skew = (4 - hop) % 64
            span = (ft - 1) * hop + n_fft
            assert ft in (16, 32, 64) and depth % 4 == 0 and n_fft % depth == 0
            assert lds >= 4 * (span + skew * ((span - 1) // hop)) + 2 * depth * 256 and lds <= 160 * 1024
    assert dmx.logmel_geometry(w)[0] == 64 and dmx.logmel_geometry(w)[2] <= 80 * 1024  # two workgroups share a CU


def test_the_npy_writer_is_read_by_numpy(tmp_path):
    for shape in ((3, 80, 3000), (7,), (2, 0, 5)):
        data = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) / 3
        dmx.npy_write(str(tmp_path / "a.mel.npy"), data)
        back = np.load(tmp_path / "a.mel.npy")
        assert back.dtype == np.float32 and back.shape == shape and np.array_equal(back, data)
