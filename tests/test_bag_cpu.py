"""Bags of models on the track path without a GPU (include/demucs_hip.h dmx_bag_weights / dmx_tracks_infer_bag; the
specification: tests/bag_spec.py): the weight matrix, the exports, and the checks that run before
any GPU work."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bag_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMX_ERR_ARG = 5


@pytest.fixture(scope="module")
def dmx():
    so = os.path.join(ROOT, "demucs_cpp_amd", "lib", "libdemucs_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", ROOT, "demucs_cpp_amd/lib/libdemucs_hip.so"], stdout=subprocess.DEVNULL)
    from demucs_cpp_amd import binding
    return binding


def test_header_constants_and_exports(dmx):
    hdr = open(os.path.join(ROOT, "include", "demucs_hip.h")).read()
    assert "#define DMX_MAX_BAG 8" in hdr
    assert "n_models * n_shifts <= 256" in hdr
    assert dmx.MAX_BAG == bag_spec.MAX_BAG == 8
    assert "dmx_bag_weights" in dmx.EXPORTS and "dmx_tracks_infer_bag" in dmx.EXPORTS
    assert hasattr(dmx.Context, "tracks_bag") and hasattr(dmx, "bag_weights")
    # the engine is untouched: its sentence in the header stays
    assert "The engine (several GPUs, the fine-tuned bag) is out of scope: dmx_engine_track_infer returns fp32." in hdr


@pytest.mark.parametrize("S", [1, 4, 6])
def test_null_weights_are_the_diagonal(dmx, S):
    w, W = dmx.bag_weights(S, S)
    assert np.array_equal(w, np.eye(S, dtype=np.float32))
    assert np.array_equal(W, np.ones(S, np.float32))
    ws, Ws = bag_spec.effective_weights(S, S)
    assert np.array_equal(w, ws) and np.array_equal(W, Ws)


def test_sums_are_fp32_in_increasing_model_order_over_the_nonzero_weights(dmx):
    rng = np.random.default_rng(5)
    for Q, S in ((1, 4), (2, 4), (3, 4), (8, 6), (5, 1)):
        m = rng.uniform(0.01, 3.0, (Q, S)).astype(np.float32)
        m[rng.uniform(size=(Q, S)) < 0.3] = 0
        m[0, m.sum(0) == 0] = 0.3  # no empty stem
        for q in range(Q):
            if not m[q].any():
                m[q, 0] = 1.7  # no empty model
        w, W = dmx.bag_weights(Q, S, m)
        ws, Ws = bag_spec.effective_weights(Q, S, m)
        assert np.array_equal(w, m) and np.array_equal(w, ws)
        assert np.array_equal(W, Ws), (Q, S)
    # an order-dependent case: 2^24 + 1 + 1 in fp32 is 2^24, 1 + 1 + 2^24 is 2^24 + 2
    _, W = dmx.bag_weights(3, 1, [[2.0 ** 24], [1], [1]])
    assert W[0] == np.float32(2.0 ** 24)
    _, W = dmx.bag_weights(3, 1, [[1], [1], [2.0 ** 24]])
    assert W[0] == np.float32(2.0 ** 24 + 2)


def _call(dmx, Q, S, weights):
    L = dmx.lib()
    eff = np.full(64, -7.0, np.float32)
    sums = np.full(8, -7.0, np.float32)
    wa = np.ascontiguousarray(weights, np.float32) if weights is not None else None
    rc = L.dmx_bag_weights(Q, S, wa.ctypes.data if wa is not None else None, eff.ctypes.data, sums.ctypes.data)
    return rc, L.dmx_last_error().decode(), eff, sums


REJECTED = [
    (0, 4, None, "n_models must be in [1, 8], got 0"),
    (9, 4, np.ones((9, 4)), "n_models must be in [1, 8], got 9"),
    (-1, 4, None, "n_models"),
    (3, 4, None, "needs n_models == n_sources"),
    (2, 4, [[1, 1, 1, 1], [1, -0.5, 1, 1]], "model 1, stem 1"),
    (2, 4, [[1, 1, 1, 1], [1, 1, float("nan"), 1]], "model 1, stem 2"),
    (2, 4, [[float("inf"), 1, 1, 1], [1, 1, 1, 1]], "model 0, stem 0"),
    (2, 4, [[1, 0, 1, 1], [1, 0, 1, 1]], "weights: stem 1 has no model"),
    (4, 4, [[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0]], "weights: model 3 has no non-zero weight"),
]


@pytest.mark.parametrize("Q,S,weights,what", REJECTED)
def test_rejections_name_what_is_wrong_and_write_nothing(dmx, Q, S, weights, what):
    rc, msg, eff, sums = _call(dmx, Q, S, weights)
    assert rc == DMX_ERR_ARG
    assert what in msg and "dmx_bag_weights" in msg, msg
    assert (eff == -7).all() and (sums == -7).all()
    if 1 <= Q <= 8:
        with pytest.raises(ValueError) as e:
            bag_spec.effective_weights(Q, S, weights)
        assert what.split(":")[-1].strip() in str(e.value) or what in str(e.value)
    with pytest.raises((dmx.DmxError, AssertionError)):
        dmx.bag_weights(Q, S, weights)


def test_a_null_context_is_rejected_with_nothing_written(dmx):
    L = dmx.lib()
    a = np.zeros((2, 100), np.float32)
    o = np.zeros((4, 2, 100), np.float32)
    pk = np.zeros(4, np.float32)
    ap = (ctypes.c_void_p * 1)(a.ctypes.data)
    op = (ctypes.c_void_p * 1)(o.ctypes.data)
    na = (ctypes.c_int64 * 1)(100)
    mp = (ctypes.c_void_p * 4)(None, None, None, None)
    for spec in (None, ctypes.byref(dmx.OutputSpec())):
        rc = L.dmx_tracks_infer_bag(None, mp, 4, None, 1, ap, na, 1, 0.25, None, spec, op, pk.ctypes.data, dmx.LAYOUT_PLANAR, None, None)
        assert rc == DMX_ERR_ARG
        msg = L.dmx_last_error().decode()
        assert "dmx_tracks_infer_bag" in msg and "null context" in msg, msg
        assert not o.any() and not pk.any()


def test_the_specification_stays_inside_its_tolerance():
    """tests/bag_spec.py steps 3-4 against the float64 recombination of the models' own de-normalised results: the bound the
    GPU tests use (2^-20 (max |out_q| + |mean|)) leaves room above the specification's own error (a few 2^-24)."""
    rng = np.random.default_rng(9)
    Q, S, n = 3, 4, 20000
    w = np.array([[0.3, 0, 1.7, 0.45], [0.6, 2.2, 0, 0.45], [0, 0.9, 0.1, 0.45]], np.float32)
    eff, _ = bag_spec.effective_weights(Q, S, w)
    worst = 0.0
    for std, mean in ((0.1, 0.01), (0.37, -0.2), (1.0, 0.0)):
        e = rng.standard_normal((Q, S, 2, n)).astype(np.float32)
        outs = [(e[q].astype(np.float64) * np.float32(std) + np.float32(mean)).astype(np.float32) for q in range(Q)]
        got = bag_spec.combine(e, eff, std, mean)
        ref = bag_spec.recombine64(outs, eff)
        tol = bag_spec.tolerance(outs, mean)
        err = float(np.abs(got - ref).max())
        worst = max(worst, err / tol)
        assert err <= tol, (std, mean, err, tol)
    assert worst < 0.5  # 2^-20 is 16 roundings of 2^-24; the specification needs a few
    # a wrong W, a missing division or swapped models are orders of magnitude outside
    bad = bag_spec.combine(e, eff, std, mean) * np.float32(1.01)
    assert float(np.abs(bad - ref).max()) > 100 * tol


def test_one_model_at_weight_one_and_duplicates_reproduce_the_single_model_bits():
    rng = np.random.default_rng(10)
    e = rng.standard_normal((1, 4, 2, 5000)).astype(np.float32)
    std, mean = np.float32(0.21), np.float32(0.03)
    single = bag_spec._fma(e[0], std, mean)
    ones = np.ones((1, 4), np.float32)
    assert np.array_equal(bag_spec.combine(e, ones, std, mean), single)
    dup = np.concatenate([e, e])
    for wv in (1.0, 2.0):
        assert np.array_equal(bag_spec.combine(dup, np.full((2, 4), wv, np.float32), std, mean), single)
    # the diagonal picks stem s from model s
    e4 = rng.standard_normal((4, 4, 2, 1000)).astype(np.float32)
    got = bag_spec.combine(e4, np.eye(4, dtype=np.float32), std, mean)
    for s in range(4):
        assert np.array_equal(got[s], bag_spec._fma(e4[s, s], std, mean))
