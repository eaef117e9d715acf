"""The op-level harness checked on the CPU, before a GPU is involved (tests/op_reference.py, tests/cpu_interp.cpp interp_step):
 * the bounds are not too tight: the interpreter's own fp32 arithmetic, op by op on the inputs of the precise chain, stays
   within the bound tests/test_gpu_op_parity.py holds every HIP kernel to;
 * the plan with K / V operand planes (what a bf16x3 context builds by default) computes what the fp32 plan and the oracle do;
 * the check has teeth: small deliberate mistakes in a GEMM, the row-resident DConv and the LSTM are each rejected;
 * the step interface runs as a stand-alone program (the form in which it was run under AddressSanitizer / UBSan)."""
import os
import subprocess

import numpy as np
import pytest

import op_reference as R
import oracle_lib as orc

ROOT = R.ROOT


@pytest.fixture(scope="module")
def L():
    return R.lib()


def make_ref(L, tmp_models, case, mode):
    key, seg, B, _ = R.CASES[case]
    ref = R.Ref(L, tmp_models[key], seg, B, mode, mode != "f32" and key != 3)
    rng = np.random.default_rng(seg + B)
    ref.set_mix((0.1 * rng.standard_normal((B, 2, seg))).astype(np.float32))
    return ref


def sweep_float_vs_precise(ref, mode):
    """every op: fp32 step and precise step from the same inputs; the worst |float - r| / (c u s) per op"""
    rows = []
    i = 0
    while i < ref.n_ops:
        op = ref.ops[i]
        if op["kind"] == R.OP_TAP:
            i += 1
            continue
        pair = op["kind"] == R.OP_ISTFT and op.get("fused", 0)
        steps = [i, i + 1] if pair else [i]
        last = ref.ops[steps[-1]]
        hull = [rg for j in steps for rg in ref.ops[j]["writes"]]
        saved = [ref.A[lo:hi].copy() for lo, hi in hull]
        for j in steps:
            ref.step(j, False)
        fidx = R.written(ref, last)
        fvals = ref.A.view(np.uint32).copy() if R.plane_range(last) else None
        fg = ref.A[fidx].copy()
        for (lo, hi), v in zip(hull, saved):
            ref.A[lo:hi] = v
        hterms = last["kind"] == R.OP_IGEMM and last["arith"] == 2
        assert R.step_pair(ref, i, hterms) == steps[-1]
        snap = R.snapshot(ref, last)
        pr = R.plane_range(last)
        keep = fidx if not pr else fidx[(fidx < pr[0]) | (fidx >= pr[1])]
        assert np.array_equal(keep, snap["idx"]), f"{last['name']}: the two arithmetics wrote different elements"
        if pr:
            fg = fvals.view(np.float32)[snap["idx"]]
        q = R.ratios(fg, snap["r"], snap["s"])
        if pr:
            total, _ = R.bf16_planes_sum(fvals[pr[0]:pr[1]].view(np.uint16), last["kvPlane"])
            q = np.concatenate([q, R.ratios(total, *snap["planes"])])
        rows.append((last["name"], last.get("label"), R.bound_c(last, mode), float(q.max()) if q.size else 0.0, R.rms(q)))
        i = steps[-1] + 1
    return rows


@pytest.mark.parametrize("case,mode", [(c, m) for c, v in R.CASES.items() for m in v[3]])
def test_fp32_interpreter_stays_within_the_op_bounds(case, mode, L, tmp_models):
    ref = make_ref(L, tmp_models, case, mode)
    rows = sweep_float_vs_precise(ref, mode)
    ref.close()
    over = [r for r in rows if not r[3] <= r[2]]
    assert len(rows) > 100 and not over, over[:8]


def test_plane_plan_end_to_end_equals_fp32_plan_and_oracle(L, tmp_models):
    """seg 16384: planes on both branches. The kvPlanes plan interpreted end to end (EPI_KPL / EPI_VT + attention reading the
    planes) against the plain plan and the oracle, to the 2e-5 of tests/test_plan_interp.py"""
    seg = 16384
    rng = np.random.default_rng(5)
    mix = (0.1 * rng.standard_normal((1, 2, seg))).astype(np.float32)
    ref = R.Ref(L, tmp_models[4], seg, 1, "bf16x3", True)
    assert sum(1 for o in ref.ops if o["kind"] == R.OP_IGEMM and o["epi"] in (R.EPI_KPL, R.EPI_VT)) >= 8
    assert sum(1 for o in ref.ops if o["kind"] == R.OP_ATTENTION and o["planes"]) >= 4
    mi = np.ascontiguousarray(mix.transpose(0, 2, 1))
    out = np.zeros((1, 4, 2, seg), np.float32)
    L.interp_run(ref.h, mi.ctypes.data, out.ctypes.data)
    ref.close()
    h = L.interp_create(tmp_models[4].encode(), seg, 1)
    plain = np.zeros_like(out)
    L.interp_run(h, mi.ctypes.data, plain.ctypes.data)
    L.interp_free(h)
    m = orc.OracleModel(tmp_models[4])
    want = m.segment(mix[0])
    m.close()
    peak = np.abs(want).max()
    assert np.abs(out[0] - plain[0]).max() / peak < 2e-5
    assert np.abs(out[0] - want).max() / peak < 2e-5


_judge = R.rejects  # the GPU test's verdict on what an implementation left in the arena: True = rejected


def _teeth(L, tmp_models, case, mode, plans):
    """plans: op name -> function(ref, op, snap, honest arena (uint32), run) returning {mistake: corrupted arena}. The interpreter's
    fp32 step plays the kernel on a canary-filled arena (`run(mutate_inputs)`); every corrupted arena must be rejected and the
    honest one accepted. The corruptions are made HERE, on the output array or on the uploaded input: the interpreter stays the
    specification and holds no deliberate mistake."""
    ref = make_ref(L, tmp_models, case, mode)
    seen = {}
    for i, op in enumerate(ref.ops):
        if op["kind"] == R.OP_TAP:
            continue
        if op["name"] not in plans:
            ref.step(i, True, chained=bool(op["kind"] == R.OP_OLA and op.get("fused")))
            continue

        def run(mutate=None):
            saved, before = R.canary_arena(ref, op["reads"], R.CANARY_A)
            if mutate:
                mutate(ref.A)
                before = ref.A.view(np.uint32).copy()
            ref.step(i, False)
            got = ref.A.view(np.uint32).copy()
            ref.A[:] = saved
            return got, before

        honest, before = run()
        ref.step(i, True)  # (none of the target ops' results feed a later target through an in-place tensor that matters here)
        snap = R.snapshot(ref, op)
        _, q0 = R.check_op(op, mode, honest, before, snap)
        rms_honest = R.rms(q0)
        assert not _judge(op, mode, honest, before, snap, rms_honest)
        for what, (got, bef) in plans[op["name"]](ref, op, snap, honest, before, run).items():
            assert _judge(op, mode, got, bef, snap, rms_honest), f"{op['name']}: not rejected: {what}"
            seen[(op["name"], what)] = True
        if {n for n, _ in seen} == set(plans):
            break
    ref.close()
    return seen


def _gemm_mistakes(ref, op, snap, honest, before, run):
    """a K projection that writes fp32 q columns and the bf16 planes of k: plain linear layer, rows contiguous"""
    M, K, Kp, n0, ldy, y = op["M"], op["K"], op["Kp"], op["kvCol0"], op["ldy"], op["y"]
    x = ref.A[op["reads"][0][0]:op["reads"][0][0] + M * K].reshape(M, K).copy()
    W = ref.W[op["w_w"]:op["w_w"] + op["N"] * Kp].reshape(op["N"], Kp)
    bias = ref.W[op["bias_w"]:op["bias_w"] + op["N"]]
    rows = y + ldy * np.arange(M)
    assert np.isin(rows + n0 - 1, snap["idx"]).all()
    out = {}

    def variant(f):
        g = honest.copy()
        f(g.view(np.float32), g)
        return g, before

    def drop_k(a, _):
        a[rows + n0 // 2] -= x[:, K - 1] * W[n0 // 2, K - 1]

    def no_bias(a, _):
        for n in range(n0 - 16, n0):
            a[rows + n] -= bias[n]

    def scaled(a, _):
        for n in range(16, 32):
            a[rows + n] *= np.float32(1.0 + 2.0 ** -12)

    def past(a, _):
        assert y + M * ldy not in snap["idx"]
        a[y + M * ldy] = 1.0

    def third_plane(_, g):
        lo, hi = R.plane_range(op)
        w = g[lo:hi].view(np.uint16)
        w[2 * op["kvPlane"]:3 * op["kvPlane"]] = 0

    out["the last k of one output column dropped"] = variant(drop_k)
    out["no bias in the last column block"] = variant(no_bias)
    out["one 16-column fragment scaled by 1 + 2^-12"] = variant(scaled)
    out["one element written past the last row"] = variant(past)
    out["the third operand plane zero"] = variant(third_plane)
    return out


def _shifted_input(floats):
    def make(ref, op, snap, honest, before, run):
        lo, hi = op["reads"][0]

        def shift(A):
            A[lo:hi] = np.roll(A[lo:hi].copy(), floats(op))

        return {"the input taken one row off (a shifted pad / tap)": run(shift)}
    return make


def _dconv_mistakes(ref, op, snap, honest, before, run):
    C = op["K"] // 3
    out = _shifted_input(lambda o: o["K"] // 3)(ref, op, snap, honest, before, run)  # one position along the innermost row axis
    g = honest.copy()
    a = g.view(np.float32)
    sel = snap["idx"][(snap["idx"] - op["writes"][0][0]) % C == 5]
    a[sel] *= np.float32(1.0 + 2.0 ** -12)
    out["one channel of the row scaled by 1 + 2^-12"] = (g, before)
    return out


def _lstm_mistakes(ref, op, snap, honest, before, run):
    H, T, o = op["K"], op["T"], op["writes"][0][0]
    out = {}
    g = honest.copy()
    a = g.view(np.float32)
    r1, r2 = o + 1 * 2 * H + H, o + 2 * 2 * H + H  # the backward direction's half of time steps 1 and 2 of the first segment
    tmp = a[r1:r1 + H].copy()
    a[r1:r1 + H] = a[r2:r2 + H]
    a[r2:r2 + H] = tmp
    out["two time steps of the backward direction swapped"] = (g, before)
    g = honest.copy()
    a = g.view(np.float32)
    a[o + 3:o + 2 * H * T:2 * H] *= np.float32(1.0 + 2.0 ** -12)
    out["one hidden unit scaled by 1 + 2^-12"] = (g, before)
    return out


def test_the_check_rejects_small_mistakes(L, tmp_models):
    """Each of these is rejected by the verdict the GPU test applies (value bound, containment, RMS rule: one function for both
    tests), and the honest fp32 result is accepted: in a GEMM with operand planes a dropped k, a missing bias, a fragment off by
    2^-12, a write past the last row, a zero third plane; a strided conv and the row-resident DConv reading one row off; a DConv
    channel and an LSTM unit off by 2^-12; two LSTM time steps swapped."""
    seen = _teeth(L, tmp_models, "4s_8000", "bf16x3", {"encoder.1.conv": _shifted_input(lambda o: 4),
                                                         "encoder.1.dconv": _dconv_mistakes,
                                                         "crosstransformer.layers.0.qk": _gemm_mistakes})
    assert len(seen) == 8, seen
    seen = _teeth(L, tmp_models, "v3_7000", "f32", {"encoder.4.dconv0.lstm0": _lstm_mistakes})
    assert len(seen) == 2, seen


def test_step_interface_as_a_stand_alone_program(tmp_models):
    """tests/op_step_main.cpp (its own main, nothing of Python in the process): steps every op of a small plan in both arithmetics,
    reads every accessor and runs the small GEMMs with every seeded mistake. OP_STEP_MAIN names another build of it - the one
    compiled with -fsanitize=address,undefined is how the step interface was checked for memory errors and undefined behaviour."""
    exe = os.environ.get("OP_STEP_MAIN") or os.path.join(ROOT, "tests", "_build", "op_step_main")
    if not os.environ.get("OP_STEP_MAIN"):
        subprocess.check_call(["make", "-C", ROOT, "op_step"], stdout=subprocess.DEVNULL)
    for key, gemm, kv in ((4, 1, 1), (3, 0, 0)):
        r = subprocess.run([exe, tmp_models[key], "8000", "1", str(gemm), str(kv)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "steps ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
