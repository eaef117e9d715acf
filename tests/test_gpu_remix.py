"""Outputs remixed on the GPU from the stems and the original mixture (include/demucs_hip.h dmx_tracks_infer_remix /
dmx_remix_encode, csrc/pcm.hip remix kernels, binding Context.tracks_remix / remix_encode, demucscpp::
demucs_inference_batch_remix through cli/demucs_batch.cpp.main --other-method / --remix). Every comparison is exact (bytes, or
float bit patterns with NaN equal to NaN: pcm_spec.same) against the NumPy specification tests/remix_spec.py (run with
-m gpu on an MI355X)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pcm_spec as ps
import remix_spec as rs
from test_gpu_pcm_output import _crafted, _five, _offsets, _read

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SEG = {4: 8000, 6: 8000, 3: 16384}  # reduced segments, as tests/test_gpu_pcm_output.py
ENCODINGS = [ps.PCM_F32, ps.PCM_S16, ps.PCM_S24]
CLIPS = [ps.CLIP_NONE, ps.CLIP_RESCALE, ps.CLIP_CLAMP]
LENGTHS = [1, 2, 3, 4, 5, 7, 255, 256, 1023, 100003]  # edge groups, one block, grid stride


@pytest.fixture(scope="module")
def stage():
    """the binding for the tests of the stage alone: no model runs, so they are not repeated per GEMM arithmetic"""
    from demucs_cpp_amd import binding

    assert binding.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return binding


def _mixture(v, seed):
    """(2, n): the sum of the stems plus a little noise, as a real mixture is (the stems' NaN / inf come along)"""
    rng = np.random.default_rng(seed)
    with np.errstate(all="ignore"):
        return (v.sum(0, dtype=F) + rng.uniform(-1e-3, 1e-3, v.shape[1:])).astype(F)


def _eight(S):
    """8 outputs with fractional gains, every one using the mixture column"""
    rng = np.random.default_rng(8 + S)
    g = rng.uniform(-1.2, 1.2, (8, S + 1)).astype(F)
    g[rng.uniform(size=g.shape) < 0.35] = 0
    g[:, S] = [0.9, -0.4, 1, 0.3, -1, 0.7, 0.05, -0.6]
    return g


def _matrices(S):
    m = [("identity", rs.identity(S))]
    for stem in (0, S - 1):
        for name, method in (("add", rs.OTHER_ADD), ("minus", rs.OTHER_MINUS), ("none", rs.OTHER_NONE)):
            m.append((f"{name} {stem}", rs.two_stems(S, stem, method)))
    return m + [("fractional", rs.fractional(S)), ("eight", _eight(S))]


def _assert_same(got, peaks, want, wpeaks, what):
    assert len(got) == len(want), what
    assert np.array_equal(np.asarray(peaks).view(np.uint32), wpeaks.view(np.uint32)), (what, peaks, wpeaks)
    for o, (g, w) in enumerate(zip(got, want)):
        assert ps.same(g, w), f"{what} output {o}: {int((np.asarray(g) != np.asarray(w)).sum())} elements differ"


# ---- 1. the stage alone equals the specification
@pytest.mark.parametrize("S", [4, 6])
def test_stage_alone_equals_the_specification(S, stage):
    dmx = stage
    frac = rs.fractional(S)
    assert (frac != 0).any(0).all() and (_eight(S)[:, S] != 0).all()
    teeth = 0
    on = off = 0
    for n in LENGTHS:
        v = _crafted(S, n, 100 * S + n)
        mix = _mixture(v, n)
        # teeth: on this very input a contracted evaluation (product fused into the sum) is another result
        spec_out, fused = rs.outputs(v, mix, frac), rs.contracted(v, mix, frac)
        differ = int((np.isfinite(spec_out) & np.isfinite(fused) & (spec_out != fused)).sum())
        assert differ > 0 or n < 255, (n, differ)
        teeth += differ
        for name, g in _matrices(S):
            outs = rs.outputs(v, mix, g)
            wpeaks = np.array([ps.peak(o) for o in outs], F)
            on += int((F(1.01) * wpeaks[np.isfinite(wpeaks)] > 1).sum())
            off += int((F(1.01) * wpeaks <= 1).sum())
            for enc in ENCODINGS:
                for clip in CLIPS:
                    got, peaks = dmx.remix_encode(v, mix, dmx.RemixSpec(g, enc, clip))
                    want = [ps.encode_output(o, enc, clip, p) for o, p in zip(outs, wpeaks)]
                    _assert_same(got, peaks, want, wpeaks, f"S {S} n {n} matrix {name} encoding {enc} clip {clip}")
    assert teeth > 1000, teeth
    assert on and off, (on, off)  # the rescale branch taken and not taken


def test_a_nan_in_a_stem_nobody_asked_for_does_not_spread(stage):
    dmx = stage
    S, n = 4, 1023
    rng = np.random.default_rng(9)
    v = rng.uniform(-0.5, 0.5, (S, 2, n)).astype(F)
    mix = _mixture(v, 1)
    v[1] = np.nan  # gain 0 in every row below
    v[0, 1, 5::7] = np.nan
    g = np.array([[0, 0, 0.7, -0.35, 0], [0, 0, 0, -1, 1], [0, 0, 1 / 3, 0, 0.5]], F)
    for enc, clip in ((ps.PCM_F32, ps.CLIP_NONE), (ps.PCM_F32, ps.CLIP_RESCALE), (ps.PCM_S16, ps.CLIP_RESCALE)):
        got, peaks = dmx.remix_encode(v, mix, dmx.RemixSpec(g, enc, clip))
        want, wpeaks = rs.encode(v, mix, g, enc, clip)
        _assert_same(got, peaks, want, wpeaks, f"encoding {enc} clip {clip}")
        assert np.isfinite(peaks).all() and (peaks > 0).all()
        if enc == ps.PCM_F32:
            assert all(np.isfinite(o).all() for o in got)
    # and a NaN mixture is not read when its column is zero (nor a NULL one: the device entry test)
    got, _ = dmx.remix_encode(v, np.full_like(mix, np.nan), dmx.RemixSpec(g[:1], ps.PCM_F32, ps.CLIP_NONE))
    assert np.isfinite(got[0]).all()


# ---- 2. new equals old
@pytest.mark.parametrize("S", [4, 6])
def test_zero_one_matrices_give_the_bytes_of_the_output_spec_stage(S, stage):
    dmx = stage
    for n in (3, 256, 100003):
        v = _crafted(S, n, 7 * S + n)
        for enc in ENCODINGS:
            for clip in CLIPS:
                for stem in (0, 1, S - 1):
                    old, opk = dmx.pcm_encode(v, dmx.OutputSpec(enc, clip, stem))
                    new, npk = dmx.remix_encode(v, None, dmx.RemixSpec(dmx.remix_two_stems(S, stem, dmx.OTHER_ADD), enc, clip))
                    _assert_same(new, npk, old, opk, f"S {S} n {n} add {stem} encoding {enc} clip {clip}")
                old, opk = dmx.pcm_encode(v, dmx.OutputSpec(enc, clip, -1))
                new, npk = dmx.remix_encode(v, None, dmx.RemixSpec(rs.identity(S), enc, clip))
                _assert_same(new, npk, old, opk, f"S {S} n {n} identity encoding {enc} clip {clip}")


# ---- 3. the device entry
def test_stage_alone_on_device_memory_strides_alignments_and_padding(stage):
    """dmx_remix_encode_device: planes at a stride larger than n and 4 bytes off 16-byte alignment, the mixture 4 and 8
    bytes off it, outputs at the 16-byte rounded stride, a caller's stream; nothing is written behind the last output's padding"""
    import torch

    dmx = stage
    S, n, stride, tail = 4, 1021, 1027, 64
    v = _crafted(S, n, 5)
    mix = _mixture(v, 6)
    g = _eight(S)
    d_in = torch.zeros(S * 2 * stride + 3, device="cuda")
    d_in[1:1 + S * 2 * stride].view(S * 2, stride)[:, :n] = torch.from_numpy(v.reshape(S * 2, n)).cuda()  # base 4 bytes off 16
    d_mix = torch.zeros(2 * n + 4, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_mix.data_ptr() % 16 == 0
    for enc, per in ((ps.PCM_S16, 4), (ps.PCM_S24, 6), (ps.PCM_F32, 8)):
        for clip in (ps.CLIP_RESCALE, ps.CLIP_NONE):
            for off in (1, 2, 0):  # floats: the mixture 4 bytes, 8 bytes off, and aligned
                d_mix.zero_()
                d_mix[off:off + 2 * n] = torch.from_numpy(np.ascontiguousarray(mix.T).reshape(-1)).cuda()
                spec = dmx.RemixSpec(g, enc, clip)
                ostride = (n * per + 15) // 16 * 16
                d_out = torch.full((8 * ostride + tail,), 0x5A, dtype=torch.uint8, device="cuda")
                d_pk = torch.full((8,), -1.0, device="cuda")
                s = torch.cuda.Stream()
                torch.cuda.synchronize()
                dmx._chk(dmx.lib().dmx_remix_encode_device(0, d_in.data_ptr() + 4, S, n, stride, d_mix.data_ptr() + 4 * off,
                                                           ctypes.byref(spec.c), d_out.data_ptr(), d_pk.data_ptr(), s.cuda_stream))
                s.synchronize()
                want, wpeaks = rs.encode(v, mix, g, enc, clip)
                raw = d_out.cpu().numpy()
                assert np.array_equal(d_pk.cpu().numpy().view(np.uint32), wpeaks.view(np.uint32))
                for o in range(8):
                    got = dmx.pcm_views(raw[o * ostride:o * ostride + n * per], spec.output_spec(), n, 1)[0]
                    assert ps.same(got, want[o]), (enc, clip, off, o)
                assert (raw[8 * ostride:] == 0x5A).all(), (enc, clip, off)  # behind the last output's (up to 15 bytes of) padding
    # a NULL mixture: accepted when its column is zero, refused with a message otherwise, and nothing is written then
    L = dmx.lib()
    spec = dmx.RemixSpec(rs.identity(S), ps.PCM_S16, ps.CLIP_RESCALE)
    ostride = (n * 4 + 15) // 16 * 16
    d_out = torch.full((S * ostride,), 0x5A, dtype=torch.uint8, device="cuda")
    d_pk = torch.full((8,), -1.0, device="cuda")
    dmx._chk(L.dmx_remix_encode_device(0, d_in.data_ptr() + 4, S, n, stride, None, ctypes.byref(spec.c), d_out.data_ptr(), d_pk.data_ptr(), None))
    torch.cuda.synchronize()
    want, wpeaks = ps.encode(v, ps.PCM_S16, ps.CLIP_RESCALE, -1)
    raw = d_out.cpu().numpy()
    for o in range(S):
        assert ps.same(dmx.pcm_views(raw[o * ostride:o * ostride + n * 4], spec.output_spec(), n, 1)[0], want[o]), o
    d_out.fill_(0x5A); d_pk.fill_(-1.0)
    bad = dmx.RemixSpec(rs.two_stems(S, 3, rs.OTHER_MINUS), ps.PCM_S16, ps.CLIP_RESCALE)
    assert L.dmx_remix_encode_device(0, d_in.data_ptr() + 4, S, n, stride, None, ctypes.byref(bad.c), d_out.data_ptr(), d_pk.data_ptr(), None) == 5
    assert "null d_mix pointer, and the mixture column of the gains is not all zero" in L.dmx_last_error().decode()
    assert L.dmx_remix_encode_device(0, d_in.data_ptr() + 4, S, n, stride, d_mix.data_ptr() + 2, ctypes.byref(bad.c), d_out.data_ptr(),
                                     d_pk.data_ptr(), None) == 5 and "4-byte aligned" in L.dmx_last_error().decode()
    assert L.dmx_remix_encode_device(0, d_in.data_ptr() + 4, S, n, stride, d_mix.data_ptr(), ctypes.byref(bad.c), d_out.data_ptr() + 4,
                                     d_pk.data_ptr(), None) == 5 and "16-byte aligned" in L.dmx_last_error().decode()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all() and (d_pk.cpu().numpy() == -1.0).all()


# ---- 4. end to end = the specification applied to the fp32 call and the input audio
def _check_tracks(got, peaks, ref, audios, g, enc, clip, what):
    on = off = 0
    for t, (o, pk, r, a) in enumerate(zip(got, peaks, ref, audios)):
        want, wpeaks = rs.encode(r, a, g, enc, clip)
        _assert_same(o, pk, want, wpeaks, f"{what} track {t}")
        on += int((F(1.01) * wpeaks > 1).sum())
        off += int((F(1.01) * wpeaks <= 1).sum())
    return on, off


@pytest.mark.parametrize("N,ov", [(1, 0.25), (3, 0.5)])
@pytest.mark.parametrize("key", [4, 6, 3])
def test_tracks_remix_equals_the_specification_on_tracks_opts_and_the_audio(key, N, ov, dmx, tmp_models):
    seg = SEG[key]
    audios = _five(seg, 41 + key)
    offs = _offsets(5, N)
    m = dmx.Model(tmp_models[key])
    S = m.n_sources
    ctx = dmx.Context(m, seg, 3)  # every track but the shortest is finished in several pieces
    ref = ctx.tracks_opts(audios, N, ov, offs)
    minus, frac = dmx.remix_two_stems(S, S - 1, dmx.OTHER_MINUS), rs.fractional(S)
    on = off = 0
    for name, g in (("minus", minus), ("fractional", frac)):
        for enc, clip in ((ps.PCM_S16, ps.CLIP_RESCALE), (ps.PCM_F32, ps.CLIP_NONE)):
            got, peaks = ctx.tracks_remix(audios, dmx.RemixSpec(g, enc, clip), n_shifts=N, overlap=ov, shift_offsets=offs)
            a, b = _check_tracks(got, peaks, ref, audios, g, enc, clip, f"model {key} N {N} overlap {ov} {name} {(enc, clip)}")
            if clip == ps.CLIP_RESCALE:
                on, off = on + a, off + b
            if name == "minus" and enc == ps.PCM_F32:  # float32 / none: exactly audio - stem in fp32
                for t in range(5):
                    assert np.array_equal(got[t][0].view(np.uint32), np.ascontiguousarray(ref[t][S - 1].T).view(np.uint32)), t
                    assert np.array_equal(got[t][1].view(np.uint32), np.ascontiguousarray((audios[t] - ref[t][S - 1]).T).view(np.uint32)), t
    assert on > 0 and off > 0, (on, off)
    again = ctx.tracks_opts(audios, N, ov, offs)  # the fp32 call behind remix calls on the same context: the same bits
    assert all(np.array_equal(r, g) for r, g in zip(ref, again))
    ctx.close(); m.close()


def test_batching_and_layout_do_not_change_a_byte_and_add_is_tracks_pcm(dmx, tmp_models):
    seg = SEG[4]
    audios = _five(seg, 78)
    offs = _offsets(5, 1)
    m = dmx.Model(tmp_models[4])
    spec = dmx.RemixSpec(_eight(4), ps.PCM_S24, ps.CLIP_RESCALE)
    clamp = dmx.RemixSpec(rs.fractional(4), ps.PCM_S16, ps.CLIP_CLAMP)  # encoded and copied out piece by piece
    base = None
    for mb in (3, 1, 8):
        ctx = dmx.Context(m, seg, mb)
        res = [ctx.tracks_remix(audios, s, shift_offsets=offs, layout=lay) for s in (spec, clamp) for lay in (dmx.LAYOUT_PLANAR, dmx.LAYOUT_EIGEN)]
        if base is None:
            base = res[0], res[2]
            ref = ctx.tracks_opts(audios, 1, 0.25, offs)
            _check_tracks(*base[0], ref, audios, spec.gains, ps.PCM_S24, ps.CLIP_RESCALE, "eight rows")
            _check_tracks(*base[1], ref, audios, clamp.gains, ps.PCM_S16, ps.CLIP_CLAMP, "clamp")
            for stem in (0, 3):  # the add matrix: the bytes of tracks_pcm with that stem
                for enc, clip in ((ps.PCM_S16, ps.CLIP_RESCALE), (ps.PCM_S24, ps.CLIP_NONE)):
                    old, opk = ctx.tracks_pcm(audios, dmx.OutputSpec(enc, clip, stem), shift_offsets=offs)
                    new, npk = ctx.tracks_remix(audios, dmx.RemixSpec(dmx.remix_two_stems(4, stem, dmx.OTHER_ADD), enc, clip), shift_offsets=offs)
                    for t in range(5):
                        _assert_same(new[t], npk[t], old[t], opk[t], f"add {stem} {(enc, clip)} track {t}")
        for i, (outs, pks) in enumerate(res):
            want_o, want_p = base[i // 2]
            for t in range(5):
                _assert_same(outs[t], pks[t], want_o[t], want_p[t], f"max_batch {mb} call {i} track {t}")
        ctx.close()
    m.close()


# ---- 5. a bag
def test_bag_remix_equals_the_specification_on_the_fp32_bag(dmx, tmp_path):
    from demucs_cpp_amd.weights import write_synthetic_model

    paths = []
    for i in range(4):
        paths.append(str(tmp_path / f"ggml-model-htdemucs_ft_{i}-4s-f16.bin"))
        write_synthetic_model(paths[-1], 4, 50 + i)
    seg = SEG[4]
    audios = [a * F(8) for a in _five(seg, 15)]  # loud enough for the rescale branch
    offs = np.array([[[(4033 * (t + 1) + 977 * q + 31 * k) % 22050 for k in range(2)] for q in range(4)] for t in range(5)])
    models = [dmx.Model(p) for p in paths]
    ctx = dmx.Context(models[1], seg, 3)
    before = ctx.tracks(audios[1:3], [5, 4033])
    fp32 = ctx.tracks_bag(models, audios, n_shifts=2, overlap=0.25, shift_offsets=offs)  # weights None: the diagonal
    g = rs.fractional(4)
    on = off = 0
    for enc, clip in ((ps.PCM_S16, ps.CLIP_RESCALE), (ps.PCM_F32, ps.CLIP_NONE)):
        got, peaks = ctx.tracks_remix(audios, dmx.RemixSpec(g, enc, clip), models=models, n_shifts=2, overlap=0.25, shift_offsets=offs)
        a, b = _check_tracks(got, peaks, fp32, audios, g, enc, clip, f"bag {(enc, clip)}")
        on, off = on + a, off + b
    assert on > 0
    after = ctx.tracks(audios[1:3], [5, 4033])  # the context is bound to its own model (model 1) again
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    with pytest.raises(dmx.DmxError, match="dmx_tracks_infer_remix: weights: stem 3 has no model"):
        ctx.tracks_remix(audios, dmx.RemixSpec(g), models=models[:3], weights=np.eye(3, 4), shift_offsets=offs[:, :3, :1])
    after = ctx.tracks(audios[1:3], [5, 4033])
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    ctx.close()
    for m in models:
        m.close()


# ---- 6. errors on a live context, progress
def test_errors_on_a_live_context_name_the_field_and_write_nothing(dmx, tmp_models):
    seg = SEG[4]
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    audios = _five(seg, 5)[:3]
    ns = [a.shape[1] for a in audios]
    ok = rs.fractional(4)
    nan, zero = ok.copy(), ok.copy()
    nan[1, 4], zero[0] = np.nan, 0
    cases = [(dmx.RemixSpec(ok, n_out=0), "remix spec: n_out must be in [1, 8], got 0"),
             (dmx.RemixSpec(np.ones((9, 5), F)), "remix spec: n_out must be in [1, 8], got 9"),
             (dmx.RemixSpec(None, n_out=3), "remix spec: null gain matrix"),
             (dmx.RemixSpec(nan), "remix spec: output 1, source 4 (the mixture): gain nan is not finite"),
             (dmx.RemixSpec(zero), "remix spec: output 0 has no non-zero gain"),
             (dmx.RemixSpec(ok, encoding=5), "remix spec: encoding 5"),
             (dmx.RemixSpec(ok, clip=-2), "remix spec: clip -2")]
    outs = [np.full(9 * n * 8, 0xA5, np.uint8) for n in ns]
    pk = np.full(3 * 9, -7.0, F)
    for spec, what in cases:
        fb = {ps.PCM_F32: 8, ps.PCM_S16: 4, ps.PCM_S24: 6}.get(spec.encoding, 8)
        views = [o[:max(spec.n_out, 0) * n * fb] for o, n in zip(outs, ns)]
        with pytest.raises(dmx.DmxError) as e:
            ctx.tracks_remix(audios, spec, shift_offsets=[[0], [0], [0]], out=views, peaks=pk)
        assert e.value.code == 5 and "dmx_tracks_infer_remix: " + what in str(e.value), str(e.value)
        assert all((o == 0xA5).all() for o in outs) and (pk == -7.0).all(), what
    for kw, what in (({"shift_offsets": [[0], [22050], [0]]}, "track 1"), ({"n_shifts": 0, "shift_offsets": None}, "n_shifts"),
                     ({"overlap": 0.95, "shift_offsets": [[0], [0], [0]]}, "overlap"), ({"weights": np.ones((1, 4)), "shift_offsets": None}, "weights given without models")):
        views = [o[:3 * n * 4] for o, n in zip(outs, ns)]
        with pytest.raises(dmx.DmxError, match=what):
            if "weights" in kw:  # through the C ABI: the binding would size the weights by the models
                w = np.ones(4, F)
                ap = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in audios])
                op = (ctypes.c_void_p * 3)(*[v_.ctypes.data for v_ in views])
                dmx._chk(dmx.lib().dmx_tracks_infer_remix(ctx.h, None, 0, w.ctypes.data, 3, ap, (ctypes.c_int64 * 3)(*ns), 1, 0.25, None,
                                                          ctypes.byref(dmx.RemixSpec(ok).c), op, pk.ctypes.data, dmx.LAYOUT_PLANAR, None, None))
            else:
                ctx.tracks_remix(audios, dmx.RemixSpec(ok), out=views, peaks=pk, **kw)
        assert all((o == 0xA5).all() for o in outs) and (pk == -7.0).all(), what
    # the context still works, and the same call with good arguments fills every byte
    views = [o[:3 * n * 8] for o, n in zip(outs, ns)]
    got, peaks = ctx.tracks_remix(audios, dmx.RemixSpec(ok, ps.PCM_F32, ps.CLIP_NONE), shift_offsets=[[1], [2], [3]], out=views, peaks=pk)
    ref = ctx.tracks(audios, [1, 2, 3])
    _check_tracks(got, peaks, ref, audios, ok, ps.PCM_F32, ps.CLIP_NONE, "after the errors")
    assert (pk[:9] >= 0).all() and (pk[9:] == -7.0).all()
    ctx.close(); m.close()


@pytest.mark.parametrize("clip", [ps.CLIP_RESCALE, ps.CLIP_CLAMP])
def test_progress_is_monotone_and_ends_at_one(clip, dmx, tmp_models):
    seg = SEG[4]
    audios = _five(seg, 14)
    offs = _offsets(5, 2)
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, seg, 3)
    msgs = []
    ctx.tracks_remix(audios, dmx.RemixSpec(rs.fractional(4), ps.PCM_S16, clip), n_shifts=2, shift_offsets=offs,
                     progress=lambda p, s: msgs.append((p, s)))
    ps_ = [p for p, _ in msgs]
    total = sum(ctx.track_geometry(a.shape[1], s)[1] for a, o in zip(audios, offs) for s in o)
    assert len(ps_) == 1 + (total + 2) // 3  # the start, then one report per batch
    assert all(b >= a for a, b in zip(ps_, ps_[1:])), ps_
    assert ps_[0] == 0.0 and abs(ps_[-1] - 1.0) < 1e-6
    ctx.close(); m.close()


# ---- 7. the batch CLI
def test_cli_other_method_and_remix(dmx, tmp_models, golden_dir, tmp_path):
    from wavio import read_wav

    batch = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
    assert os.path.exists(batch), "CLI not built (make cli)"
    wav = os.path.join(golden_dir, "gspi_stereo_short.wav")
    env = dict(os.environ, DMX_SHIFT_OFFSET="4033", DMX_BATCH="2")
    _, audio = read_wav(wav)
    m = dmx.Model(tmp_models[4]); ctx = dmx.Context(m, 0, 2)
    n = audio.shape[1]

    def run(extra, out):
        return subprocess.run([batch] + extra + [tmp_models[4], str(tmp_path / out), wav], env=env, capture_output=True, text=True, timeout=600)

    r = run(["--two-stems", "vocals", "--other-method", "minus", "--int24"], "minus")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want, _ = ctx.tracks_remix([audio], dmx.RemixSpec(dmx.remix_two_stems(4, 3, dmx.OTHER_MINUS), ps.PCM_S24, ps.CLIP_RESCALE), shift_offsets=[[4033]])
    d = tmp_path / "minus" / "gspi_stereo_short"
    assert sorted(os.listdir(d)) == ["target_0_vocals.wav", "target_1_no_vocals.wav"]
    for o, f in enumerate(("target_0_vocals.wav", "target_1_no_vocals.wav")):
        tag, nch, rate, bits, data = _read(d / f)
        assert (tag, nch, rate, bits) == (1, 2, 44100, 24) and len(data) == n * 6, f
        assert data == want[0][o].tobytes(), f

    text = "karaoke=mix-vocals,backing=drums+bass+other+-12dB*vocals"
    r = run(["--remix", text, "--clip-mode", "clamp"], "remix")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    g = np.array([[0, 0, 0, -1, 1], [1, 1, 1, F(10 ** (-12 / 20)), 0]], F)
    want, _ = ctx.tracks_remix([audio], dmx.RemixSpec(g, ps.PCM_S16, ps.CLIP_CLAMP), shift_offsets=[[4033]])
    d = tmp_path / "remix" / "gspi_stereo_short"
    assert sorted(os.listdir(d)) == ["target_0_karaoke.wav", "target_1_backing.wav"]
    for o, f in enumerate(("target_0_karaoke.wav", "target_1_backing.wav")):
        tag, nch, rate, bits, data = _read(d / f)
        assert (tag, nch, rate, bits) == (1, 2, 44100, 16) and len(data) == n * 4, f
        assert data == want[0][o].tobytes(), f

    r = run(["--two-stems", "drums", "--other-method", "none", "--float32", "--clip-mode", "none"], "none")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.listdir(tmp_path / "none" / "gspi_stereo_short") == ["target_0_drums.wav"]
    tag, nch, rate, bits, data = _read(tmp_path / "none" / "gspi_stereo_short" / "target_0_drums.wav")
    ref = ctx.tracks_opts([audio], 1, 0.25, [[4033]])[0]
    assert (tag, nch, rate, bits) == (3, 2, 44100, 32) and data == np.ascontiguousarray(ref[0].T).tobytes()

    r = run(["--remix", "g=guitar+mix"], "guitar")  # a stem name, but not of this model: known after loading
    assert r.returncode == 1 and "Usage" not in r.stderr and "unknown source 'guitar'" in r.stderr, r.stderr[-500:]
    assert not (tmp_path / "guitar").exists()
    ctx.close(); m.close()
