"""Remixed outputs without a GPU (include/demucs_hip.h dmx_remix_two_stems / dmx_remix_check / dmx_tracks_infer_remix /
dmx_remix_encode, demucscpp::parse_remix, the batch CLI's --other-method / --remix parsing) and the self-checks of the NumPy
specification tests/remix_spec.py against tests/pcm_spec.py. The kernels are pinned against that specification in
tests/test_gpu_remix.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pcm_spec as ps
import remix_spec as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMX_ERR_ARG = 5
BATCH = os.path.join(ROOT, "cli", "demucs_batch.cpp.main")
PARSE = os.path.join(ROOT, "tests", "_build", "remix_parse_harness")
F = np.float32


@pytest.fixture(scope="module")
def dmx():
    so = os.path.join(ROOT, "demucs_cpp_amd", "lib", "libdemucs_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", ROOT, "demucs_cpp_amd/lib/libdemucs_hip.so"], stdout=subprocess.DEVNULL)
    from demucs_cpp_amd import binding
    return binding


def _special_data(S, n, seed):
    """(stems (S, 2, n), mixture (2, n)) carrying pcm_spec's special values in every stem and in the mixture"""
    rng = np.random.default_rng(seed)
    sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 1.0, -1.0, 0.99, -0.99, 3.0, -1.25], F)
    v = rng.uniform(-0.6, 0.6, (S, 2, n)).astype(F)
    for s in range(S):
        v[s].reshape(-1)[s:s + len(sp)] = np.roll(sp, s)  # the stems' specials meet each other's ordinary values and specials
        v[s].reshape(-1)[-len(sp):] = sp
    mix = (v[:, :, :].sum(0) + rng.uniform(-1e-3, 1e-3, (2, n))).astype(F)
    mix.reshape(-1)[40:40 + len(sp)] = sp
    return v, mix


# ---- the specification against pcm_spec: the three consequences
@pytest.mark.parametrize("S", [4, 6])
def test_spec_zero_one_gains_are_the_two_stems_and_all_stems_outputs_bit_for_bit(S):
    v, mix = _special_data(S, 301, S)
    for stem in range(S):
        got = rs.outputs(v, mix, rs.two_stems(S, stem, rs.OTHER_ADD))
        assert ps.same(got, ps.outputs(v, stem)), stem
        assert ps.same(rs.outputs(v, None, rs.two_stems(S, stem, rs.OTHER_NONE)), v[stem:stem + 1])
        for enc in (ps.PCM_F32, ps.PCM_S16, ps.PCM_S24):
            for clip in (ps.CLIP_NONE, ps.CLIP_RESCALE, ps.CLIP_CLAMP):
                a, pa = rs.encode(v, mix, rs.two_stems(S, stem, rs.OTHER_ADD), enc, clip)
                b, pb = ps.encode(v, enc, clip, stem)
                assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
                assert all(ps.same(x, y) for x, y in zip(a, b)), (stem, enc, clip)
    assert ps.same(rs.outputs(v, mix, rs.identity(S)), ps.outputs(v, -1))  # a -0 and a NaN stay what they are
    assert np.array_equal(np.signbit(rs.outputs(v, None, rs.identity(S))), np.signbit(v))


@pytest.mark.parametrize("S", [4, 6])
def test_spec_minus_is_exactly_mixture_minus_stem(S):
    v, mix = _special_data(S, 301, 10 + S)
    with np.errstate(all="ignore"):
        for stem in range(S):
            got = rs.outputs(v, mix, rs.two_stems(S, stem, rs.OTHER_MINUS))
            assert ps.same(got[0], v[stem]) and ps.same(got[1], (mix - v[stem]).astype(F)), stem
    assert np.isnan(got).any() and np.isinf(got).any()


def test_spec_skips_zero_gain_sources_and_rounds_product_and_sum_separately():
    S, n = 4, 4096
    rng = np.random.default_rng(2)
    v = rng.uniform(-0.3, 0.3, (S, 2, n)).astype(F)
    mix = v.sum(0).astype(F)
    g = rs.fractional(S)
    assert (g != 0).any(0).all()  # every column is used
    poisoned = v.copy()
    poisoned[1] = np.nan
    assert np.isfinite(rs.outputs(poisoned, mix, g)[1]).all() and np.isnan(rs.outputs(poisoned, mix, g)[[0, 2]]).all()  # row 1 skips stem 1
    assert np.isfinite(rs.outputs(v, np.full_like(mix, np.nan), g)[[0, 2]]).all()
    # against float64: each output is within the fp32 roundings of its few terms, and a contracted evaluation differs
    want = np.einsum("os,scn->ocn", g[:, :S].astype(np.float64), v.astype(np.float64)) + g[:, S, None, None] * mix.astype(np.float64)
    got = rs.outputs(v, mix, g)
    assert np.abs(got - want).max() <= 5 * 2.0 ** -24 * np.abs(g).sum(1).max() * 0.6
    diff = [(rs.contracted(v, mix, g)[o] != got[o]).mean() for o in range(3)]
    assert diff[0] > 0.01 and diff[2] > 0.01 and diff[1] == 0, diff  # row 1's gains are powers of two: both forms are exact


# ---- the ABI
def test_header_constants_and_exports(dmx):
    hdr = open(os.path.join(ROOT, "include", "demucs_hip.h")).read()
    for line in ("#define DMX_MAX_OUTPUTS 8", "#define DMX_OTHER_ADD 0", "#define DMX_OTHER_MINUS 1", "#define DMX_OTHER_NONE 2"):
        assert line in hdr, line
    assert re.search(r"typedef struct dmx_remix_spec\s*\{\s*int encoding, clip, n_out;[^}]*const float \*gains;", hdr)
    for sym in ("dmx_remix_two_stems", "dmx_remix_check", "dmx_tracks_infer_remix", "dmx_remix_encode_device", "dmx_remix_encode"):
        assert sym in dmx.EXPORTS and hasattr(dmx.lib(), sym) and re.search(r"\b%s\(" % sym, hdr), sym
    declared = set(re.findall(r"\b(dmx_[a-z0-9_]+)\(", hdr))
    assert declared == set(dmx.EXPORTS), declared ^ set(dmx.EXPORTS)
    assert (dmx.MAX_OUTPUTS, dmx.OTHER_ADD, dmx.OTHER_MINUS, dmx.OTHER_NONE) == (rs.MAX_OUTPUTS, rs.OTHER_ADD, rs.OTHER_MINUS, rs.OTHER_NONE)
    d = dmx.RemixSpec(rs.identity(4))  # demucs's defaults
    assert (d.c.encoding, d.c.clip, d.c.n_out) == (dmx.PCM_S16, dmx.CLIP_RESCALE, 4) and d.c.gains == d.gains.ctypes.data


@pytest.mark.parametrize("S", [1, 2, 4, 6])
def test_remix_two_stems_gives_the_three_matrices(S, dmx):
    for stem in range(S):
        for method in (rs.OTHER_ADD, rs.OTHER_MINUS, rs.OTHER_NONE):
            if method == rs.OTHER_ADD and S == 1:
                with pytest.raises(dmx.DmxError, match="at least 2 sources"):
                    dmx.remix_two_stems(S, stem, method)
                continue
            g = dmx.remix_two_stems(S, stem, method)
            assert g.dtype == F and np.array_equal(g, rs.two_stems(S, stem, method)), (S, stem, method)
            dmx.remix_check(S, dmx.RemixSpec(g))
    for args, what in (((4, 4, 0), "stem 4 of a 4-source model"), ((4, -1, 0), "stem -1"), ((4, 0, 3), "method 3"), ((4, 0, -1), "method -1"),
                       ((0, 0, 0), "n_sources must be in [1, 6], got 0"), ((7, 0, 0), "n_sources must be in [1, 6], got 7")):
        with pytest.raises(dmx.DmxError, match=re.escape(what)):
            dmx.remix_two_stems(*args)
    g = np.full(10, 9.0, F)
    n_out = ctypes.c_int(-3)
    assert dmx.lib().dmx_remix_two_stems(4, 0, 1, None, ctypes.byref(n_out)) == DMX_ERR_ARG and "gains_out" in dmx.lib().dmx_last_error().decode()
    assert dmx.lib().dmx_remix_two_stems(4, 9, 1, g.ctypes.data, ctypes.byref(n_out)) == DMX_ERR_ARG
    assert (g == 9.0).all() and n_out.value == -3  # nothing written on error


def _bad_specs(dmx, S=4):
    """(RemixSpec, the message's text) for every rejection of dmx_remix_check"""
    ok = rs.fractional(S)
    nan, inf, zero = ok.copy(), ok.copy(), ok.copy()
    nan[2, 1], inf[1, S], zero[2] = np.nan, -np.inf, 0
    nine = np.ones((9, S + 1), F)
    return [
        (dmx.RemixSpec(ok, n_out=0), "remix spec: n_out must be in [1, 8], got 0"),
        (dmx.RemixSpec(nine), "remix spec: n_out must be in [1, 8], got 9"),
        (dmx.RemixSpec(ok, n_out=-1), "remix spec: n_out must be in [1, 8], got -1"),
        (dmx.RemixSpec(None, n_out=2), "remix spec: null gain matrix"),
        (dmx.RemixSpec(nan), "remix spec: output 2, source 1: gain nan is not finite"),
        (dmx.RemixSpec(inf), "remix spec: output 1, source 4 (the mixture): gain -inf is not finite"),
        (dmx.RemixSpec(zero), "remix spec: output 2 has no non-zero gain"),
        (dmx.RemixSpec(ok, encoding=3), "remix spec: encoding 3"),
        (dmx.RemixSpec(ok, encoding=-1), "remix spec: encoding -1"),
        (dmx.RemixSpec(ok, clip=3), "remix spec: clip 3"),
        (dmx.RemixSpec(ok, clip=-1), "remix spec: clip -1"),
    ]


def test_remix_check_names_every_rejection(dmx):
    L = dmx.lib()
    for S in (4, 6):
        dmx.remix_check(S, dmx.RemixSpec(rs.fractional(S)))
        dmx.remix_check(S, dmx.RemixSpec(np.ones((8, S + 1), F), dmx.PCM_F32, dmx.CLIP_NONE))
        dmx.remix_check(S, dmx.RemixSpec(rs.identity(S), dmx.PCM_S24, dmx.CLIP_CLAMP))
    seen = set()
    for spec, what in _bad_specs(dmx):
        assert L.dmx_remix_check(4, ctypes.byref(spec.c)) == DMX_ERR_ARG, what
        msg = L.dmx_last_error().decode()
        assert msg == "dmx_remix_check: " + what or msg.startswith("dmx_remix_check: " + what + " ("), msg
        seen.add(msg)
    assert len(seen) == len(_bad_specs(dmx))  # each failure has a message of its own
    assert L.dmx_remix_check(4, None) == DMX_ERR_ARG and "remix spec: null" in L.dmx_last_error().decode()
    for S in (0, 7, -1):
        assert L.dmx_remix_check(S, ctypes.byref(dmx.RemixSpec(np.ones((1, 8), F)).c)) == DMX_ERR_ARG
        assert "n_sources must be in [1, 6]" in L.dmx_last_error().decode()
    # the first failure in the documented order wins: n_out, the matrix, the gains, the rows, the encoding, the clip mode
    both = rs.fractional(4)
    both[0, 0] = np.inf
    assert L.dmx_remix_check(4, ctypes.byref(dmx.RemixSpec(both, encoding=9, clip=9).c)) == DMX_ERR_ARG
    assert "output 0, source 0" in L.dmx_last_error().decode()
    assert L.dmx_remix_check(4, ctypes.byref(dmx.RemixSpec(rs.fractional(4), encoding=9, clip=9).c)) == DMX_ERR_ARG
    assert "encoding 9" in L.dmx_last_error().decode()


def _call_tracks(dmx, spec, ctx=None):
    L = dmx.lib()
    a = np.zeros((2, 100), F)
    o = np.full(8 * 100 * 8, 0xA5, np.uint8)
    pk = np.full(8, -7.0, F)
    ap = (ctypes.c_void_p * 1)(a.ctypes.data)
    op = (ctypes.c_void_p * 1)(o.ctypes.data)
    na = (ctypes.c_int64 * 1)(100)
    rc = L.dmx_tracks_infer_remix(ctx, None, 0, None, 1, ap, na, 1, 0.25, None, ctypes.byref(spec.c) if spec is not None else None, op,
                                  pk.ctypes.data, dmx.LAYOUT_PLANAR, None, None)
    assert (o == 0xA5).all() and (pk == -7.0).all()  # nothing written
    return rc, L.dmx_last_error().decode()


def test_tracks_infer_remix_rejects_a_bad_spec_and_a_null_context_before_anything(dmx):
    """no context, no device. Without a context there is no model to give the gain matrix its width: the spec's other
    fields are checked, then the context is missed (the gains of a bad spec on a live context: tests/test_gpu_remix.py)"""
    rc, msg = _call_tracks(dmx, None)
    assert rc == DMX_ERR_ARG and msg == "dmx_tracks_infer_remix: remix spec: null", msg
    for spec, what in _bad_specs(dmx):
        rc, msg = _call_tracks(dmx, spec)
        assert rc == DMX_ERR_ARG and msg.startswith("dmx_tracks_infer_remix: "), msg
        if "output" in what:  # a gain: needs the model
            assert msg == "dmx_tracks_infer_remix: null context", msg
        else:
            assert what in msg, msg
    rc, msg = _call_tracks(dmx, dmx.RemixSpec(rs.fractional(4)))
    assert rc == DMX_ERR_ARG and msg == "dmx_tracks_infer_remix: null context", msg


def test_remix_encode_rejects_bad_arguments_before_the_device(dmx):
    L = dmx.lib()
    x = np.zeros((4, 2, 8), F)
    mix = np.zeros((8, 2), F)
    out = np.full(8 * 8 * 8, 0xA5, np.uint8)
    pk = np.full(8, -7.0, F)
    for spec, what in _bad_specs(dmx):
        for fn, args in (("dmx_remix_encode", (0, x.ctypes.data, 4, 8, mix.ctypes.data, ctypes.byref(spec.c), out.ctypes.data, pk.ctypes.data)),
                         ("dmx_remix_encode_device", (0, x.ctypes.data, 4, 8, 8, mix.ctypes.data, ctypes.byref(spec.c), out.ctypes.data,
                                                      pk.ctypes.data, None))):
            assert getattr(L, fn)(*args) == DMX_ERR_ARG, (fn, what)
            assert L.dmx_last_error().decode().startswith(fn + ": " + what), L.dmx_last_error()
    good = dmx.RemixSpec(rs.fractional(4))
    nomix = dmx.RemixSpec(rs.identity(4))
    for args, what in (((0, x.ctypes.data, 4, 8, None, ctypes.byref(good.c), out.ctypes.data, pk.ctypes.data), "null mix pointer"),
                       ((0, x.ctypes.data, 4, 0, None, ctypes.byref(nomix.c), out.ctypes.data, pk.ctypes.data), "n < 1"),
                       ((0, None, 4, 8, None, ctypes.byref(nomix.c), out.ctypes.data, pk.ctypes.data), "null pointer"),
                       ((0, x.ctypes.data, 7, 8, None, ctypes.byref(nomix.c), out.ctypes.data, pk.ctypes.data), "n_sources must be in [1, 6], got 7")):
        assert L.dmx_remix_encode(*args) == DMX_ERR_ARG and what in L.dmx_last_error().decode(), (what, L.dmx_last_error())
    assert L.dmx_remix_encode_device(0, x.ctypes.data, 4, 8, 8, None, ctypes.byref(good.c), out.ctypes.data, pk.ctypes.data, None) == DMX_ERR_ARG
    assert "null d_mix pointer, and the mixture column of the gains is not all zero" in L.dmx_last_error().decode()
    assert L.dmx_remix_encode_device(0, x.ctypes.data, 4, 8, 7, None, ctypes.byref(nomix.c), out.ctypes.data, pk.ctypes.data, None) == DMX_ERR_ARG
    assert "plane_stride" in L.dmx_last_error().decode()
    assert (out == 0xA5).all() and (pk == -7.0).all()


# ---- demucscpp::parse_remix / remix_two_stems (the shim), through tests/remix_parse_harness.cpp
def _harness(*args):
    if not os.path.exists(PARSE):
        subprocess.check_call(["make", "-C", ROOT, "tests/_build/remix_parse_harness"], stdout=subprocess.DEVNULL)
    r = subprocess.run([PARSE] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    if r.returncode != 0:
        return r.returncode, r.stderr.strip()
    rows = [ln.split() for ln in r.stdout.splitlines()]
    return [w[0] for w in rows], np.array([[int(h, 16) for h in w[1:]] for w in rows], np.uint32).view(F)


def test_parse_remix_grammar():
    names, g = _harness("parse", 4, "karaoke=mix-vocals,backing=drums+bass+other+-12dB*vocals")
    db12 = F(10 ** (-12 / 20))
    assert names == ["karaoke", "backing"]
    assert np.array_equal(g.view(np.uint32), np.array([[0, 0, 0, -1, 1], [1, 1, 1, db12, 0]], F).view(np.uint32))
    assert g[1, 3].view(np.uint32) == np.float32(10 ** (-12 / 20)).view(np.uint32) == 0x3E809BCC
    names, g = _harness("parse", 6, "a=+0.5*piano-.25*mix+3.*guitar,b_2=-6dB*drums,c=-mix+-0dB*bass")
    assert names == ["a", "b_2", "c"]
    want = np.zeros((3, 7), F)
    want[0, [5, 6, 4]] = [0.5, -0.25, 3.0]
    want[1, 0] = -F(10 ** (6 / 20))  # a leading minus is the term's sign: minus (6 dB up)
    want[2, [6, 1]] = [-1, 1]
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (g, want)
    names, g = _harness("two_stems", 6, 4, rs.OTHER_MINUS)
    assert names == ["guitar", "no_guitar"] and np.array_equal(g, rs.two_stems(6, 4, rs.OTHER_MINUS))
    names, g = _harness("two_stems", 4, 3, rs.OTHER_NONE)
    assert names == ["vocals"] and np.array_equal(g, rs.two_stems(4, 3, rs.OTHER_NONE))
    for text, what in (("karaoke=mix-flute", "term '-flute': unknown source 'flute'"), ("a=guitar", "unknown source 'guitar'"),
                       ("=mix", "empty output name"), ("a=1e3*mix", "term '1e3*mix': bad gain '1e3'"), ("a=x*mix", "bad gain 'x'"),
                       ("a=mix+*bass", "term '+*bass': bad gain ''"), ("a=1.2.3*mix", "bad gain '1.2.3'"), ("a=dB*mix", "bad gain 'dB'"),
                       ("a=mix,a=bass", "output name 'a' given twice"), ("a=mix+0.5*mix", "source 'mix' appears twice"),
                       ("a", "expected NAME=TERMS"), ("a=", "no terms"), ("a=mix,", "expected NAME=TERMS"), ("a/b=mix", "contains '/'"),
                       ("a=mix-", "unknown source ''"), ("a=--bass", "bad gain '-'"),
                       (",".join(f"o{i}=mix" for i in range(9)), "more than 8 outputs")):
        rc, err = _harness("parse", 4, text)
        assert rc == 2 and err.startswith("remix: ") and what in err, (text, err)


# ---- the batch CLI's options: usage errors come before the model is loaded
@pytest.mark.parametrize("extra,what", [
    (["--other-method", "minus"], "--other-method needs --two-stems"),
    (["--other-method", "subtract", "--two-stems", "vocals"], ""),
    (["--two-stems", "vocals", "--other-method", ""], ""),
    (["--remix", "k=mix-vocals", "--two-stems", "vocals"], "--remix and --two-stems exclude each other"),
    (["--two-stems", "vocals", "--other-method", "none", "--remix", "k=mix"], "--remix and --two-stems exclude each other"),
    (["--remix", "k=mix-flute"], "unknown source 'flute'"),
    (["--remix", "=mix-vocals"], "empty output name"),
    (["--remix", "k=mix-1e3*vocals"], "term '-1e3*vocals': bad gain '1e3'"),
    (["--remix", "k=mix-x*vocals"], "bad gain 'x'"),
    (["--remix", "k=0.5dBs*vocals"], "bad gain '0.5dBs'"),
    (["--remix", ""], "expected NAME=TERMS"),
])
def test_cli_usage_errors(extra, what, tmp_path):
    if not os.path.exists(BATCH):
        subprocess.check_call(["make", "-C", ROOT, "cli/demucs_batch.cpp.main"], stdout=subprocess.DEVNULL)
    args = [BATCH] + extra + [str(tmp_path / "no-such-model.bin"), str(tmp_path / "out"), str(tmp_path / "no-such.wav")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (extra, r.stdout, r.stderr)
    assert "Usage" in r.stderr and "--other-method add|minus|none" in r.stderr and "--remix NAME=" in r.stderr, r.stderr
    assert what in r.stderr, r.stderr
    assert "Error loading model" not in r.stderr and not (tmp_path / "out").exists()


@pytest.mark.parametrize("extra", [["--two-stems", "vocals", "--other-method", "minus"], ["--other-method", "none", "--two-stems", "piano", "--int24"],
                                   ["--two-stems", "bass", "--other-method", "add", "--clip-mode", "clamp"],
                                   ["--remix", "karaoke=mix-vocals,backing=drums+bass+other+-12dB*vocals"],
                                   ["--float32", "--remix", "g=guitar+0.5*piano", "--shifts", "2", "--clip-mode", "none"]])
def test_cli_valid_options_get_as_far_as_the_model(extra, tmp_path):
    """all six stem names parse (whether the loaded model has the stem is known only after loading)"""
    args = [BATCH] + extra + [str(tmp_path / "no-such-model.bin"), str(tmp_path / "out"), str(tmp_path / "no-such.wav")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage" not in r.stderr and "Error loading model" in r.stderr, (r.stdout, r.stderr)
