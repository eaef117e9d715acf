"""The timed entry points (dmx_*_device_timed, dmx_flac_decode_profile; include/demucs_hip.h): only the bench tools call them, so a
slip in one shows as a wrong benchmark number. Each is run behind the plain entry point of its stage on the same device memory, at
the smallest shape of the stage's own GPU test that still spans more than one tile: both return DMX_OK, the entries of ms the
header promises are finite and not negative, the entries behind them keep a sentinel, the outputs equal the plain call's bit for
bit (equal inputs give equal bits), and a null ms is DMX_ERR_ARG by name. No time is compared with another."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bss_cases  # noqa: E402
import flac_spec as fs  # noqa: E402
import limiter_cases as lcs  # noqa: E402
import loudness_cases as lc  # noqa: E402
import loudness_spec as ls  # noqa: E402
import meters_cases as mc  # noqa: E402
from demucs_cpp_amd import binding as dmx  # noqa: E402
from test_gpu_logmel import CASES as LOGMEL_CASES  # noqa: E402
from test_gpu_wiener import CASES as WIENER_CASES  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG = 5  # DMX_ERR_ARG
SENTINEL = np.float32(-12345.0)
SPARE = 3  # entries of ms behind the promised ones


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _zeros(nbytes, dtype=None):
    import torch
    return torch.zeros(nbytes, dtype=dtype or torch.uint8, device="cuda")


def _bytes(*tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in tensors]


def _timed(call, promised, null_text="null ms pointer"):
    """call(ms) -> rc, ms a pointer or None: the promised entries, the sentinel behind them, and the null ms"""
    ms = np.full(promised + SPARE, SENTINEL, np.float32)
    dmx._chk(call(ms.ctypes.data))
    print("ms", ms[:promised])
    assert np.all(np.isfinite(ms[:promised])) and np.all(ms[:promised] >= 0.0)
    assert np.all(ms[promised:] == SENTINEL)
    with pytest.raises(dmx.DmxError, match=null_text) as e:
        dmx._chk(call(None))
    assert e.value.code == ERR_ARG


def test_loudness_device_timed():
    rate, name = 8000, "tile+1"  # two tiles, five hops
    n = lc.lengths(rate)[name]
    d_x, H, L = _dev(lc.signal(rate, name, n, "noise")), n // ls.hop(rate), dmx.lib()
    import torch
    out = []
    for timed in (False, True):
        res, e, work = _zeros(16), _zeros(2 * H, torch.float64), _zeros(dmx.loudness_workspace_bytes(n))
        args = [0, d_x.data_ptr(), n, n, rate, res.data_ptr(), e.data_ptr(), work.data_ptr(), None]
        if timed:
            _timed(lambda ms: L.dmx_loudness_device_timed(*args, ms), 5)
        else:
            dmx._chk(L.dmx_loudness_device(*args))
        out.append(_bytes(res, e))
    assert out[0] == out[1]


def test_meters_device_timed():
    """the timed call keeps its results to itself: the true peak it leaves in the workspace, behind the loudness slot, is the plain call's"""
    rate, n = 48000, mc.T + 7  # F = 4, two true-peak tiles
    d_x, L = _dev(mc.tp_signal(rate, n, "lowpass")), dmx.lib()
    at = dmx.loudness_workspace_bytes(n)
    res, met = _zeros(16), _zeros(16)
    work = [_zeros(at + dmx.meters_workspace_bytes(n)) for _ in range(2)]
    dmx._chk(L.dmx_meters_device(0, d_x.data_ptr(), n, n, rate, res.data_ptr(), None, work[0].data_ptr(), None, met.data_ptr()))
    _timed(lambda ms: L.dmx_meters_device_timed(0, d_x.data_ptr(), n, n, rate, work[1].data_ptr(), None, ms), 3)
    plain, timed, m = _bytes(work[0], work[1], met)
    assert plain[at:at + 4] == timed[at:at + 4] == m[:4] and m[:4] != bytes(4)


@pytest.mark.parametrize("tp", (False, True), ids=("sample", "true_peak"))
def test_limit_device_timed(tp):
    rate, n = 44100, 2 * lcs.T + 3
    g, c = (float(v) for v in lcs.params("noise")[:2])  # the default times
    d_x, L = _dev(lcs.signal(n, "noise")), dmx.lib()
    out = []
    for timed in (False, True):
        res, work = _zeros(dmx.LIMIT_DTYPE.itemsize), _zeros(dmx.limiter_workspace_bytes(n))
        args = [0, d_x.data_ptr(), n, n, rate, g, c, int(tp), None, res.data_ptr(), work.data_ptr(), None]
        if timed:
            _timed(lambda ms: L.dmx_limit_device_timed(*args, ms), 5)
        else:
            dmx._chk(L.dmx_limit_device(*args))
        r, w = _bytes(res, work)
        out.append((r, w[:4 * n]))  # the result and M
    assert out[0] == out[1]
    assert np.frombuffer(out[0][0], dmx.LIMIT_DTYPE)[0]["limited_frames"] > 0


def test_flac_encode_device_timed():
    n, bits, level = 3 * 4096 + 123, 24, 1
    d_pcm, L = _dev(fs.pcm_bytes(fs.crafted("sine_noise", n, bits), bits).copy()), dmx.lib()
    import torch
    out = []
    for timed in (False, True):
        d_out, d_size = _zeros(dmx.flac_bound(bits, n)), torch.full((1,), -1, dtype=torch.int64, device="cuda")
        d_work = _zeros(L.dmx_flac_workspace_bytes(bits, n))
        args = [0, d_pcm.data_ptr(), bits, n, 48000, level, d_out.data_ptr(), d_size.data_ptr(), d_work.data_ptr(), None]
        if timed:
            _timed(lambda ms: L.dmx_flac_encode_device_timed(*args, ms), 3)
        else:
            dmx._chk(L.dmx_flac_encode_device_level(*args))
        out.append(_bytes(d_size, d_out))
    assert out[0] == out[1]
    assert 42 <= np.frombuffer(out[0][0], np.int64)[0] <= dmx.flac_bound(bits, n)


def test_flac_decode_profile():
    """this entry point names no pointer in its null check: `null pointer`, ms included"""
    n, bits = 4097, 16  # two frames
    x = fs.crafted("sine_noise", n, bits)
    data = dmx.flac_encode(fs.pcm_bytes(x, bits).view("<i2").reshape(-1, 2), bits)
    info, L = dmx.flac_probe(data), dmx.lib()
    import torch
    d_file = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = []
    for timed in (False, True):
        d_work = _zeros(L.dmx_flac_decode_workspace_bytes(ctypes.byref(info), len(data)))
        d_out, d_status = _zeros((n * 8 + 15) // 16 * 16), torch.full((2,), -7, dtype=torch.int64, device="cuda")
        args = [0, d_file.data_ptr(), len(data), ctypes.byref(info), dmx.PCM_F32, d_out.data_ptr(), d_status.data_ptr(), d_work.data_ptr(), None]
        if timed:
            _timed(lambda ms: L.dmx_flac_decode_profile(*args, ms), 5, null_text="null pointer")
        else:
            dmx._chk(L.dmx_flac_decode_device(*args))
        out.append(_bytes(d_status, d_out))
    assert out[0] == out[1]
    assert np.frombuffer(out[0][0], np.int64).tolist() == [0, n]


def test_bss_eval_device_timed():
    name = "scalar"
    _, J, C, Lf, N, W, H, _, _, _ = bss_cases.case(name)
    refs, ests = bss_cases.signals(name)
    d_refs, d_ests, spec, L = _dev(refs), _dev(ests), dmx.BssSpec(W, H, Lf), dmx.lib()
    import torch
    out = []
    for timed in (False, True):
        metrics, status = _zeros(4 * J * dmx.bss_windows(N, W, H), torch.float64), _zeros(1, torch.int32)
        filters, work = _zeros(J * J * C * Lf * C, torch.float64), _zeros(dmx.bss_eval_workspace_bytes(J, C, N, Lf))
        args = [0, d_refs.data_ptr(), d_ests.data_ptr(), J, C, N, N, ctypes.byref(spec), metrics.data_ptr(), status.data_ptr(),
                filters.data_ptr(), work.data_ptr(), None]
        if timed:
            _timed(lambda ms: L.dmx_bss_eval_device_timed(*args, ms), 6)
        else:
            dmx._chk(L.dmx_bss_eval_device(*args))
        out.append(_bytes(metrics, status, filters))
    assert out[0] == out[1]
    assert np.frombuffer(out[0][1], np.int32)[0] == 0 and np.isfinite(np.frombuffer(out[0][0], np.float64)).any()


@pytest.mark.parametrize("iterations", (1, 2))
def test_wiener_device_timed(iterations):
    """iterations + 2 entries: the count follows the spec, not the size of the events' array"""
    J, C, N, _, res, wl, amp = WIENER_CASES["two_blocks"][:7]
    rng = np.random.default_rng(iterations)
    src = amp * rng.standard_normal((J, C, N))
    d_mix, d_est = _dev(src.sum(axis=0).astype(np.float32)), _dev((src + 0.3 * amp * rng.standard_normal((J, C, N))).astype(np.float32))
    spec, L = dmx.WienerSpec(iterations, res, wl), dmx.lib()
    nbytes = dmx.wiener_workspace_bytes(spec, J, C, N)
    import torch
    out = []
    for timed in (False, True):
        d_out, d_work = _zeros(J * C * N, torch.float32), _zeros(nbytes)
        args = [0, d_mix.data_ptr(), d_est.data_ptr(), J, C, N, N, ctypes.byref(spec), d_out.data_ptr(), d_work.data_ptr(), nbytes, None]
        if timed:
            _timed(lambda ms: L.dmx_wiener_device_timed(*args, ms), iterations + 2)
        else:
            dmx._chk(L.dmx_wiener_device(*args))
        out.append(_bytes(d_out))
    assert out[0] == out[1] and np.frombuffer(out[0][0], np.float32).any()


def test_logmel_device_timed():
    fields, P, N, _, _ = LOGMEL_CASES["nfft64_band"]  # the smallest transform
    spec, L = dmx.LogmelSpec(**fields), dmx.lib()
    d_x = _dev((0.1 * np.random.default_rng(0).standard_normal((P, N))).astype(np.float32))
    chunks, frames = dmx.logmel_frames(spec, N)
    nbytes = dmx.logmel_workspace_bytes(spec, P, N)
    import torch
    out = []
    for timed in (False, True):
        d_out, d_work = _zeros(P * chunks * spec.n_mels * frames, torch.float32), _zeros(nbytes)
        args = [0, d_x.data_ptr(), P, N, N, ctypes.byref(spec), d_out.data_ptr(), d_work.data_ptr(), nbytes, None]
        if timed:
            _timed(lambda ms: L.dmx_logmel_device_timed(*args, ms), 3)
        else:
            dmx._chk(L.dmx_logmel_device(*args))
        out.append(_bytes(d_out))
    assert out[0] == out[1] and np.frombuffer(out[0][0], np.float32).any()
