"""NumPy restatement of the remix output stage (csrc/pcm.hip remix_gather; include/demucs_hip.h dmx_remix_spec; DESIGN.md
section 2.10). There is no reference arithmetic, so this text is what the kernels are pinned against, exactly.

    sources  src[0..S) the S stems (S, 2, n); src[S] the mixture (2, n): the caller's track as passed in.
    output o, gains g[o][0..S]: the sources are visited in increasing index; a source with gain 0 is skipped and NOT READ;
             the first visited source gives a = g * x, each later one p = g * x, a = a + p. Every product and every sum is
             its own correctly rounded fp32 operation (NumPy float32 arithmetic is exactly that): no fused multiply-add.
    peak, clip, encode of each output: pcm_spec's.

contracted() is what a build that fuses each later product into its sum would compute: the product (exact in float64)
plus the addend, rounded to float32 without rounding the product first. The GPU test uses it to show that its data can tell
the two apart; nothing is compared against it.
"""
import numpy as np

import pcm_spec as ps

F = np.float32
OTHER_ADD, OTHER_MINUS, OTHER_NONE = 0, 1, 2
MAX_OUTPUTS = 8


def _sources(v, mix):
    v = np.asarray(v, F)
    src = [v[s] for s in range(v.shape[0])]
    src.append(None if mix is None else np.asarray(mix, F))
    return src


def outputs(v, mix, gains):
    """v (S, 2, n) float32, mix (2, n) float32 or None, gains (n_out, S + 1) -> (n_out, 2, n) float32"""
    gains = np.asarray(gains, F)
    src = _sources(v, mix)
    assert gains.ndim == 2 and gains.shape[1] == len(src)
    outs = []
    with np.errstate(all="ignore"):
        for row in gains:
            acc = None
            for g, x in zip(row, src):
                if g == 0:
                    continue  # not read
                assert x is not None, "the mixture column is used but there is no mixture"
                p = (F(g) * x).astype(F)
                acc = p if acc is None else (acc + p).astype(F)
            assert acc is not None, "a row with no non-zero gain"
            outs.append(acc)
    return np.stack(outs)


def contracted(v, mix, gains):
    """the same with every later product fused into its sum (one rounding): NOT the specification"""
    gains = np.asarray(gains, F)
    src = _sources(v, mix)
    outs = []
    with np.errstate(all="ignore"):
        for row in gains:
            acc = None
            for g, x in zip(row, src):
                if g == 0:
                    continue
                if acc is None:
                    acc = (F(g) * x).astype(F)
                else:
                    acc = (np.float64(g) * x.astype(np.float64) + acc.astype(np.float64)).astype(F)
            outs.append(acc)
    return np.stack(outs)


def encode(v, mix, gains, encoding, clip_mode):
    """-> (list of n_out encoded outputs as pcm_spec.encode, np.float32 (n_out,) peaks)"""
    outs = outputs(v, mix, gains)
    peaks = np.array([ps.peak(o) for o in outs], F)
    return [ps.encode_output(o, encoding, clip_mode, p) for o, p in zip(outs, peaks)], peaks


def two_stems(S, stem, method):
    """the matrices of demucs's --other-method add | minus | none (dmx_remix_two_stems)"""
    g = np.zeros((1 if method == OTHER_NONE else 2, S + 1), F)
    g[0, stem] = 1
    if method == OTHER_ADD:
        g[1, :S] = 1
        g[1, stem] = 0
    elif method == OTHER_MINUS:
        g[1, stem], g[1, S] = -1, 1
    return g


def identity(S):
    return np.eye(S, S + 1, dtype=F)


def fractional(S):
    """three rows that use every column: non-power-of-two gains, a power-of-two row on the mixture, thirds"""
    g = np.zeros((3, S + 1), F)
    g[0, :4] = [0.7, -0.35, 1, 0.25]
    g[1, 3], g[1, S] = -0.5, 1
    g[2, :S] = F(1) / F(3)
    if S > 4:
        g[0, S - 1] = -1.3
        g[1, 4] = 0.15
    return g
