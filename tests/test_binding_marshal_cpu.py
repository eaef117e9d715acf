"""What the eight Context.tracks_* methods hand to the C ABI and how they shape what comes back, against a recording fake of
the library (no GPU, no libdemucs_hip.so). The fake turns every argument into an address or a number, so the test does not
depend on how the binding spells a pointer. Every expectation is written from the inputs below."""
import ctypes

import numpy as np
import pytest

from demucs_cpp_amd import binding as dmx

T, NS, S, Q, N = 2, (5, 3), 4, 2, 2
FB = {dmx.PCM_F32: 8, dmx.PCM_S16: 4, dmx.PCM_S24: 6}
TAIL = "N overlap so spec out peaks layout cb user"
SIG = {"dmx_tracks_infer": "h T in n so out layout cb user",
       "dmx_tracks_infer_opts": "h T in n N overlap so out layout cb user",
       "dmx_tracks_infer_pcm": "h T in n " + TAIL,
       "dmx_tracks_infer_bag": "h models Q w T in n " + TAIL,
       "dmx_tracks_infer_remix": "h models Q w T in n " + TAIL,
       "dmx_tracks_infer_flac": "h models Q w T in n N overlap so spec rate out sizes peaks layout cb user",
       "dmx_tracks_infer_from_flac": "h models Q w T in n N overlap so spec flac out sizes peaks status cb user",
       "dmx_tracks_infer_rates": "h models Q w T in n rates N overlap so spec flac out sizes peaks layout cb user"}
SIG["dmx_tracks_infer_from_flac_rates"] = SIG["dmx_tracks_infer_from_flac"]


class RemixC(ctypes.Structure):  # dmx_remix_spec, include/demucs_hip.h
    _fields_ = [("encoding", ctypes.c_int), ("clip", ctypes.c_int), ("n_out", ctypes.c_int), ("gains", ctypes.c_void_p)]


def addr(a):
    if a is None or isinstance(a, (int, float)):
        return a or 0
    return ctypes.addressof(a._obj) if hasattr(a, "_obj") else (ctypes.cast(a, ctypes.c_void_p).value or 0)


def mem(address, dtype, count):
    size = count * np.dtype(dtype).itemsize
    return np.frombuffer((ctypes.c_char * size).from_address(address), dtype) if size else np.zeros(0, dtype)


def bound(bits, n):  # the fake's dmx_flac_bound
    return 40 + n * bits // 2


def pattern(t, size):  # the bytes the fake writes into track t's output buffer
    return ((7 * t + np.arange(size)) % 251).astype(np.uint8)


class Fake:
    def __init__(self):
        self.calls, self.rc = [], 0

    def __getattr__(self, name):
        if name not in SIG:
            raise AttributeError(name)
        return lambda *args: self.tracks(name, SIG[name].split(), [addr(a) for a in args])

    def dmx_last_error(self):
        return b"fake failure"

    def dmx_output_count(self, model, spec):
        return S if mem(addr(spec), "<i4", 3)[2] < 0 else 2

    def dmx_output_bytes(self, spec, n):
        return n * FB[int(mem(addr(spec), "<i4", 3)[0])]

    def dmx_flac_bound(self, bits, n):
        return bound(bits, n)

    def dmx_flac_probe(self, data, size, info):  # the fake "file": its first byte is the frame count
        info = info._obj
        info.sample_rate, info.channels, info.bits, info.total_samples = 44100, 2, 16, int(mem(data, "u1", 1)[0])
        return 0

    def tracks(self, fn, names, args):
        assert len(names) == len(args), (fn, len(args))
        a = dict(zip(names, args))
        nT, nQ, files = a["T"], a.get("Q", 0), "from_flac" in fn
        n = [int(v) for v in mem(a["n"], "<i8", nT)]
        src = [int(v) for v in mem(a["in"], "<u8", nT)]
        frames = [int(mem(p, "u1", 1)[0]) for p in src] if files else n
        rec = {k: a.get(k) for k in ("h", "T", "N", "overlap", "layout", "rate", "flac")}
        rec.update(fn=fn, Q=nQ, n=n, in_addr=src, user=a["user"],
                   inputs=[mem(p, "u1", k).copy() if files else mem(p, "<f4", 2 * k).copy() for p, k in zip(src, n)],
                   rates=[int(v) for v in mem(a["rates"], "<i4", nT)] if "rates" in a else None,
                   models=[int(v) for v in mem(a["models"], "<u8", nQ)] if a.get("models") else None,
                   w=mem(a["w"], "<f4", nQ * S).tolist() if a.get("w") else None,
                   so=mem(a["so"], "<i4", nT * (a.get("N", 1) * max(nQ, 1))).tolist() if a["so"] else None,
                   nonnull={k for k in ("out", "sizes", "peaks", "status", "cb") if a.get(k)})
        dst = rec["out_addr"] = [int(v) for v in mem(a["out"], "<u8", nT)]
        rec["spec"], n_out = None, 0
        if a.get("spec") and fn in ("dmx_tracks_infer_pcm", "dmx_tracks_infer_bag"):
            enc, clip, stem = (int(v) for v in mem(a["spec"], "<i4", 3))
            rec["spec"], n_out = (enc, clip, stem), S if stem < 0 else 2
        elif a.get("spec"):
            r = RemixC.from_address(a["spec"])
            enc, n_out = r.encoding, r.n_out
            rec["spec"] = (enc, r.clip, n_out, mem(r.gains, "<f4", n_out * (S + 1)).tolist())
        for t, k in enumerate(frames):
            if rec["spec"] is None:
                mem(dst[t], "<f4", S * 2 * k)[:] = 1000 * t + np.arange(S * 2 * k)
            elif fn == "dmx_tracks_infer_flac" or a.get("flac"):
                size = n_out * bound(24 if enc == dmx.PCM_S24 else 16, k)
                mem(dst[t], "u1", size)[:] = pattern(t, size)
                mem(a["sizes"], "<i8", nT * n_out)[t * n_out:(t + 1) * n_out] = 10 + 3 * t + np.arange(n_out)
            else:
                mem(dst[t], "u1", n_out * k * FB[enc])[:] = pattern(t, n_out * k * FB[enc])
        if a.get("peaks"):
            mem(a["peaks"], "<f4", nT * n_out)[:] = 0.5 + np.arange(nT * n_out)
        if a.get("status"):
            mem(a["status"], "<i8", 2 * nT)[:] = [v for t in range(nT) for v in (t, 100 + t)]
        if a["cb"]:
            dmx.PROGRESS_FN(a["cb"])(0.5, b"half", None)
        self.calls.append(rec)
        return self.rc


@pytest.fixture
def env(monkeypatch):
    fake = Fake()
    monkeypatch.setattr(dmx, "_lib", fake)
    models = [object.__new__(dmx.Model) for _ in range(Q)]
    for i, m in enumerate(models):
        m.h = ctypes.c_void_p(0x2000 + 16 * i)
    ctx = object.__new__(dmx.Context)
    ctx.h, ctx.S, ctx.model = 0x1000, S, models[0]
    yield ctx, models, fake
    for o in models + [ctx]:  # nothing for __del__ to free
        o.h = None


AUDIOS = [(100 * t + np.arange(2 * n)).reshape(2, n).astype(np.float32) for t, n in enumerate(NS)]
FILES = [bytes([n]) + bytes(range(9 + t)) for t, n in enumerate(NS)]
WEIGHTS = (np.arange(Q * S, dtype=np.float32) / 8).reshape(Q, S)
GAINS = (np.arange(3 * (S + 1), dtype=np.float32) / 4).reshape(3, S + 1)
RATES = [48000, 32000]
PLANAR, EIGEN, CLAMP = dmx.LAYOUT_PLANAR, dmx.LAYOUT_EIGEN, dmx.CLIP_CLAMP
# (method, form of its outputs, encoding, the values of `bag` it can take)
KINDS = [("tracks", "fp32", 0, (False,)), ("tracks_opts", "fp32", 0, (False,)), ("tracks_bag", "fp32", 0, (True,)),
         ("tracks_rates", "fp32", 0, (False, True)), ("tracks_pcm", "pcm", dmx.PCM_S16, (False,)), ("tracks_bag", "pcm", dmx.PCM_S24, (True,)),
         ("tracks_remix", "pcm", dmx.PCM_F32, (False, True)), ("tracks_rates", "pcm", dmx.PCM_S16, (False, True)),
         ("tracks_from_flac", "pcm", dmx.PCM_S24, (False, True)), ("tracks_flac", "flac", dmx.PCM_S16, (False, True)),
         ("tracks_rates", "flac", dmx.PCM_S24, (False, True)), ("tracks_from_flac", "flac", dmx.PCM_S16, (False, True))]
CASES = [(kind, form, enc, layout, bag, full) for kind, form, enc, bags in KINDS for bag in bags for full in (False, True)
         for layout in ((PLANAR,) if kind == "tracks_from_flac" else (PLANAR, EIGEN))]  # files have no layout


@pytest.mark.parametrize("kind,form,enc,layout,bag,full", CASES)
def test_what_the_library_sees_and_what_comes_back(env, kind, form, enc, layout, bag, full):
    """full: everything optional is given - shift offsets, weights, a progress callback and the caller's buffers"""
    ctx, models, fake = env
    files, log = kind == "tracks_from_flac", []
    shape = (T,) if kind == "tracks" else (T, Q, N) if bag else (T, N)
    so = 20 + np.arange(int(np.prod(shape))).reshape(shape) if full else None
    n_out = 0 if form == "fp32" else 2 if kind in ("tracks_pcm", "tracks_bag") else 3
    per = [bound(24 if enc == dmx.PCM_S24 else 16, n) if form == "flac" else n * FB[enc] for n in NS]  # bytes of one output
    remix, ospec = dmx.RemixSpec(GAINS, enc, CLAMP), dmx.OutputSpec(enc, CLAMP, 1)
    kw = dict(shift_offsets=so, progress=(lambda p, m: log.append((p, m))) if full else None)
    kw.update({} if kind == "tracks" else dict(n_shifts=N, overlap=0.5), **({} if files else dict(layout=layout)))
    if bag:
        kw.update(weights=WEIGHTS if full else None, **({} if kind == "tracks_bag" else dict(models=models)))
    reuse = status = flat = None
    if full and kind != "tracks_rates":  # a buffer of a FLAC form, or for files, may be larger than needed; a PCM buffer is exact
        reuse = [np.zeros((S, 2, n), np.float32) if form == "fp32" else np.zeros(n_out * p + (5 if form == "flac" or files else 0), np.uint8)
                 for n, p in zip(NS, per)]
        kw.update(out=reuse)
    if full and kind in ("tracks_remix", "tracks_flac"):
        flat = dict(peaks=np.zeros(T * n_out + 1, np.float32), **(dict(sizes=np.zeros(T * n_out + 2, np.int64)) if kind == "tracks_flac" else {}))
        kw.update(flat)
    if files:
        status = np.full(2 * T + 1, -7, np.int64) if full else None
        kw.update(flac_out=form == "flac", any_rate=full, track_status=status)
    if kind in ("tracks_pcm", "tracks_bag") and form == "pcm":
        kw.update(spec=ospec)
    if kind == "tracks_rates" and form != "fp32":
        kw.update(spec=remix, flac=form == "flac")
    if kind == "tracks_flac":
        kw.update(sample_rate=48000)
    args = {"tracks_bag": (models, AUDIOS), "tracks_from_flac": (FILES, remix), "tracks_rates": (AUDIOS, RATES), "tracks_remix": (AUDIOS, remix),
            "tracks_flac": (AUDIOS, remix)}.get(kind, (AUDIOS,))
    res = getattr(ctx, kind)(*args, **kw)

    rec = fake.calls[-1]  # ---- what the library saw
    fn = {"tracks": "dmx_tracks_infer", "tracks_from_flac": "dmx_tracks_infer_from_flac" + ("_rates" if full else "")}.get(kind, "dmx_tracks_infer_" + kind[7:])
    nonnull = {"out"} | ({"cb"} if full else set()) | ({"peaks"} if n_out else set()) | ({"status"} if files else set())
    if form == "flac" or files or (kind == "tracks_rates" and n_out):
        nonnull.add("sizes")
    want = dict(fn=fn, h=0x1000, T=T, user=0, Q=Q if bag else 0, models=[0x2000, 0x2010] if bag else None, nonnull=nonnull,
                w=WEIGHTS.ravel().tolist() if bag and full else None, so=None if so is None else so.ravel().tolist(),
                N=None if kind == "tracks" else N, overlap=None if kind == "tracks" else 0.5, layout=None if files else layout,
                n=[len(f) for f in FILES] if files else list(NS), rates=RATES if kind == "tracks_rates" else None,
                rate=48000 if kind == "tracks_flac" else None, flac=int(form == "flac") if files or kind == "tracks_rates" else None,
                spec=None if not n_out else (enc, CLAMP, 1) if n_out == 2 else (enc, CLAMP, 3, GAINS.ravel().tolist()))
    assert {k: rec[k] for k in want} == want and log == ([(0.5, "half")] if full else [])
    for got, a, f in zip(rec["inputs"], AUDIOS, FILES):  # Eigen: [n][2], the column-major image of (2, n)
        assert got.tobytes() == (f if files else a.tobytes() if layout == PLANAR else np.stack([a[0], a[1]], 1).tobytes())
    if layout == PLANAR and not files:
        assert rec["in_addr"] == [a.ctypes.data for a in AUDIOS]  # contiguous float32 tracks are passed as they are
    if reuse is not None and (layout == PLANAR or n_out):
        assert rec["out_addr"] == [b.ctypes.data for b in reuse]  # and the library writes into the caller's buffers

    if form == "fp32":  # ---- what comes back
        for t, (o, n) in enumerate(zip(res, NS)):
            image = np.arange(S * 2 * n).reshape(S, 2, n) if layout == PLANAR else np.fromfunction(lambda s, c, i: s + S * (c + 2 * i), (S, 2, n))
            assert o.shape == (S, 2, n) and o.dtype == np.float32 and o.flags.c_contiguous and np.array_equal(o, 1000 * t + image)
            assert reuse is None or o is reuse[t]
        return
    outs, peaks = res[:2]
    for t, (n, p) in enumerate(zip(NS, per)):
        assert peaks[t].dtype == np.float32 and peaks[t].tolist() == [0.5 + t * n_out + o for o in range(n_out)] and len(outs[t]) == n_out
        for o, v in enumerate(outs[t]):
            if form == "flac":  # the file of output o starts at o * bound and has the size the library reported
                assert type(v) is bytes and v == pattern(t, n_out * p)[o * p:o * p + 10 + 3 * t + o].tobytes()
                continue
            e = pattern(t, n_out * p)[o * p:(o + 1) * p]
            e = e.view("<i2").reshape(n, 2) if enc == dmx.PCM_S16 else e.reshape(n, 2, 3) if enc == dmx.PCM_S24 else e.view("<f4").reshape(n, 2)
            assert v.dtype == e.dtype and v.shape == e.shape and np.array_equal(v, e) and (reuse is None or np.shares_memory(v, reuse[t]))
    if flat is not None:
        assert all(np.shares_memory(p, flat["peaks"]) for p in peaks) and ("sizes" not in flat or flat["sizes"][:6].tolist() == [10, 11, 12, 13, 14, 15])
    if files:
        assert res[2].dtype == np.int64 and res[2].tolist() == [[0, 100], [1, 101]]
        assert status is None or (np.shares_memory(res[2], status) and status[-1] == -7)


def test_from_flac_failure_keeps_what_was_learned(env):
    ctx, _, fake = env
    fake.rc = 7
    status = np.zeros(2 * T, np.int64)
    with pytest.raises(dmx.DmxError, match=r"\[dmx error 7\] fake failure") as ei:
        ctx.tracks_from_flac(FILES, dmx.RemixSpec(GAINS, dmx.PCM_S16), track_status=status)
    outs, peaks = ei.value.partial
    assert ei.value.code == 7 and status.tolist() == [0, 100, 1, 101]
    assert [p.tolist() for p in peaks] == [[0.5, 1.5, 2.5], [3.5, 4.5, 5.5]]
    assert np.array_equal(outs[1][2], pattern(1, 3 * 3 * 4)[2 * 12:3 * 12].view("<i2").reshape(3, 2))


def test_argument_checks_and_no_tracks(env):
    ctx, models, fake = env
    with pytest.raises(AssertionError, match=r"shift_offsets: expected shape \(2, 2\), got \(2, 3\)"):
        ctx.tracks_opts(AUDIOS, N, shift_offsets=np.zeros((T, 3)))
    with pytest.raises(AssertionError, match=r"shift_offsets: expected shape \(2, 2, 2\), got \(2, 2\)"):
        ctx.tracks_flac(AUDIOS, dmx.RemixSpec(GAINS), models=models, n_shifts=N, shift_offsets=np.zeros((T, N)))
    with pytest.raises(AssertionError, match=r"weights: expected shape \(2, 4\), got \(4, 2\)"):
        ctx.tracks_bag(models, AUDIOS, WEIGHTS.T)
    with pytest.raises(AssertionError):  # PCM buffers are exact, .flac buffers may be larger
        ctx.tracks_pcm(AUDIOS, out=[np.zeros(S * n * 4 + 1, np.uint8) for n in NS])
    assert fake.calls == []
    ctx.tracks_bag([None, models[1]], AUDIOS, WEIGHTS)  # the error path of the library: a NULL model is passed on
    assert fake.calls[-1]["models"] == [0, 0x2010]
    assert ctx.tracks([]) == [] and ctx.tracks_opts([]) == [] and ctx.tracks_rates([], []) == []
    assert ctx.tracks_pcm([]) == ([], []) and ctx.tracks_remix([], dmx.RemixSpec(GAINS)) == ([], [])
    assert ctx.tracks_flac([], dmx.RemixSpec(GAINS), models=models) == ([], [])
    outs, peaks, st = ctx.tracks_from_flac([], dmx.RemixSpec(GAINS))
    assert (outs, peaks, st.shape) == ([], [], (0, 2)) and all(c["T"] == 0 for c in fake.calls[1:])
