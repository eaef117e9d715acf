"""The crafted operands of tests/value_cases.py proven on the CPU, before a GPU is involved:
 * the census conditions hold: on every crafted op every value class its shape can reach holds at least 256 evaluations (the
   statistics classes and the seam of dmx_erff: what value_cases.UNREACHABLE derives) and no class more than 60 % of its group; a
   gemm_plain operand puts one non-zero into a sum, an fp16-term one two;
 * every crafted value and every reference output is finite;
 * the yardstick stays inside: the interpreter's own fp32 arithmetic passes check_op on every crafted op (with K_eff where the
   operand has one), and where the RMS rule applies its RMS is not 0;
 * one op of every kernel instance of the nine families is crafted in every case (the GPU test launches exactly these);
 * teeth: numpy models of gn_act, a GELU, a GLU and an fp16-term linear layer, the statistics reduction and the LSTM pass the GPU
   test's verdict (op_reference.rejects) when honest; with a seeded mistake they are rejected on the crafted operands and accepted
   on smooth operands of the same op (for the late stale h: of the same layer at the sweep's 7 steps) - the gap, shown once, on the
   CPU. SEEDED lists the mistakes and, where one of the design's cannot show on any operand, says why and which one stands in.
DMX_OP_PARITY_RECORD=<dir> writes op_parity_values_cpu.txt (profiles/op_parity_values_cpu.txt is such a record)."""
import os

import numpy as np
import pytest

import op_reference as R
import value_cases as VC

SWEEPS = [(c, m) for c, v in VC.CASES.items() for m in v[3]]


@pytest.fixture(scope="module")
def L():
    return R.lib()


def make_ref(L, tmp_models, case, mode):
    key, seg, B, _ = VC.CASES[case]
    return R.Ref(L, tmp_models[key], seg, B, mode, mode != "f32" and key != 3)


def both_steps(ref, i, op, mode, K_eff):
    """the fp32 interpreter on a canary arena, then the precise step, from the operands in the arena. Returns (snap, before, census,
    (worst, rms) of the fp32 interpreter or the mismatch's text)"""
    saved, before = R.canary_arena(ref, op["reads"], R.CANARY_A)
    ref.step(i, False)
    got = ref.A.view(np.uint32).copy()
    ref.A[:] = saved
    ref.step(i, True, hterms=op["kind"] == R.OP_IGEMM and op["arith"] == 2)
    census = ref.census()
    snap = R.snapshot(ref, op)
    ref.A[:] = saved  # (an in-place op has overwritten its operand)
    try:
        worst, q = R.check_op(op, mode, got, before, snap, K_eff)
        verdict = (worst, R.rms(q))
    except R.OpMismatch as e:
        verdict = str(e)
    return snap, before, census, verdict


def sweep_case(L, tmp_models, case, mode):
    ref = make_ref(L, tmp_models, case, mode)
    rows = []
    for inst, i in VC.select(ref, case).items():
        op, fam = ref.ops[i], inst[0]
        row = dict(name=op["name"], inst=inst, fam=fam, op=op, infos=[], knz=[], verdicts=[], census=dict.fromkeys(R.CENSUS, 0), finite=True,
                   records=VC.records_of(ref, i, fam))
        for rnd in range(VC.rounds_of(ref, i, fam)):
            info = VC.craft(ref, i, case, rnd)
            row["finite"] &= all(bool(np.isfinite(ref.A[lo:hi]).all()) for lo, hi in op["reads"])
            snap, _, census, verdict = both_steps(ref, i, op, mode, info["K_eff"])
            row["finite"] &= bool(np.isfinite(snap["r"]).all() and np.isfinite(snap["s"]).all())
            for k, v in census.items():
                row["census"][k] = max(row["census"][k], v) if k == "gemm_row_nonzeros_max" else row["census"][k] + v
            row["infos"].append(info)
            row["knz"].append(census["gemm_row_nonzeros_max"])
            row["verdicts"].append(verdict)
        row["c"] = R.bound_c(R.effective(op, row["infos"][-1]["K_eff"]), mode)
        rows.append(row)
    ref.close()
    return rows


@pytest.fixture(scope="module")
def sweeps(L, tmp_models):
    out = {key: sweep_case(L, tmp_models, *key) for key in SWEEPS}
    d = os.environ.get("DMX_OP_PARITY_RECORD")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "op_parity_values_cpu.txt"), "w") as f:
            f.write("# case\tmode\top\tkernel instance\tc\trounds\tfp32 interpreter: worst |g - r| / (u s), RMS per round\tcensus (classes that hold evaluations)\n")
            for (case, mode), rows in out.items():
                for r in rows:
                    v = "; ".join(x if isinstance(x, str) else f"{x[0]:.3f}, {x[1]:.4f}" for x in r["verdicts"])
                    f.write(f"{case}\t{mode}\t{r['name']}\t{' '.join(str(k) for k in r['inst'])}\t{r['c']}\t{len(r['infos'])}\t{v}\t"
                            + " ".join(f"{k}={n}" for k, n in r["census"].items() if n) + "\n")
    return out


def test_every_kernel_instance_of_every_family_is_crafted(sweeps):
    for (case, mode), rows in sweeps.items():
        fams = {r["fam"] for r in rows}
        if case in VC.LSTM_ONLY:
            assert fams == {"lstm"} and {(r["op"]["K"], r["op"]["T"]) for r in rows} == {(192, 65), (384, 33)}
            continue
        want = {"gemm_plain", "gemm_pro", "stats_reduce", "dconv_row"}
        want |= {"group_stats", "gn_act", "lstm"} if case.startswith("v3") else {"layernorm"}
        want |= {"gemm_hterms"} if mode == "fp16x3" else set()
        assert fams == want, (case, mode, fams ^ want)
        assert len({r["inst"] for r in rows}) == len(rows) >= 15


def test_the_census_conditions_hold(sweeps):
    for key, rows in sweeps.items():
        for r in rows:
            bad = VC.census_failures(r["fam"], r["op"], r["infos"], r["census"], r["records"])
            assert not bad, (key, r["name"], bad)
            if r["fam"] in ("gemm_plain", "gemm_hterms"):
                assert r["knz"] == [f["K_eff"] for f in r["infos"]], (key, r["name"], r["knz"])


def test_every_crafted_value_and_every_reference_output_is_finite(sweeps):
    for key, rows in sweeps.items():
        assert all(r["finite"] for r in rows), (key, [r["name"] for r in rows if not r["finite"]])


def test_the_fp32_interpreter_stays_within_the_bound_and_its_rms_is_not_zero(sweeps):
    for (case, mode), rows in sweeps.items():
        for r in rows:
            for v, f in zip(r["verdicts"], r["infos"]):
                assert not isinstance(v, str), (case, mode, r["name"], v)
                if R.bound_c(R.effective(r["op"], f["K_eff"]), mode) > R.RMS_MIN_C:
                    assert v[1] > 0.0, (case, mode, r["name"], "the yardstick of the RMS rule is 0")


def test_a_state_written_at_step_0_still_changes_the_lstm_output_at_step_T_minus_1(L, tmp_models):
    """the 'remember' units (forget gate open, input gate open on the first step only): the cell gate's sign at step 0 is the sign of
    the output 64 (32) steps later, in both directions - the memory the two exchange buffers must carry through every reuse"""
    case, mode = "v3_66560", "bf16x3"
    ref = make_ref(L, tmp_models, case, mode)
    for inst, i in VC.select(ref, case).items():
        op = ref.ops[i]
        H, T = op["K"], op["T"]
        VC.craft(ref, i, case, 0)
        X = ref.view(ref.operands(i)["xproj"]).reshape(1, T, 2, H, 4)
        out = op["writes"][0][0]
        first, last = {0: 0, 1: T - 1}, {0: T - 1, 1: 0}  # the time index of a direction's first and last step
        at = [out + (last[d] * 2 + d) * H + j for d in (0, 1) for j in (0, 8)]  # units 0 and 8: kind 'remember', either sign
        ref.step(i, True)
        before = ref.R[at].copy()
        for d in (0, 1):
            X[0, first[d], d, [0, 8], 2] *= -1.0  # (the recurrent term is 0 on a direction's first step: xproj IS the pre-activation)
        ref.step(i, True)
        after = ref.R[at].copy()
        assert np.all(np.abs(before) > 0.7) and np.allclose(after, -before, rtol=1e-6), (op["name"], before, after)
    ref.close()


def test_the_fp16_term_rows_hold_the_branches_of_the_row_scale(sweeps):
    for r in sweeps[("4s_8000", "fp16x3")]:
        if r["fam"] == "gemm_hterms":
            kinds = {k: sum(f["rows"][k] for f in r["infos"]) for k in r["infos"][0]["rows"]}
            assert [f["K_eff"] for f in r["infos"]] == [1, 2]
            assert set(kinds) == {"zero", "2^-130", "2^-120", "1", "2^100", "1 and 2^-20", "2^10 and 2^-10"} and min(kinds.values()) >= 8, (r["name"], kinds)


# ---------------------------------------------------------------------------------------------------------------------------------
# teeth: numpy models of five ops that take a seeded mistake
ERF_A = (-0.0005843715625815094, 0.004958246368914843, -0.026736384257674217, 0.11280667781829834, -0.3761231601238251, 1.1283791065216064)
ERF_B = (0.0002812488819472492, -0.004376694560050964, 0.03201308846473694, -0.149833083152771, -0.9193801283836365, -1.6268224716186523,
         -0.0002986486360896379)


def erf_model(x, coef=0.0, clamp=True):
    """kernels.h dmx_erff in double, rounded once. coef: added to the upper range's linear coefficient; clamp: min(|x|, 4)"""
    x = x.astype(np.float64)
    t = np.minimum(np.abs(x), 4.0) if clamp else np.abs(x)
    a = np.polyval(ERF_A, x * x) * x
    cb = list(ERF_B)
    cb[5] += coef
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.copysign(1.0 - np.exp2(np.polyval(cb, t)), x)
    return np.where(t < 0.92, a, r)


def gelu_model(v, **kw):
    with np.errstate(over="ignore", invalid="ignore"):
        return (0.5 * v.astype(np.float64) * (1.0 + erf_model(v * np.float32(0.70710678118654752440), **kw))).astype(np.float32)


def sigmoid_model(v, flip=False):
    v = v.astype(np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-v))
    return np.where(flip & (np.abs(v) > 17.0), 1.0 - s, s).astype(np.float32)


def tanh_model(v, mistake):
    with np.errstate(over="ignore", invalid="ignore"):
        if mistake == "tanh_quotient":  # (e^2v - 1) / (e^2v + 1) in fp32: inf / inf beyond v = 44.4
            e = np.exp(np.float32(2.0) * v)
            return (e - np.float32(1.0)) / (e + np.float32(1.0))
        t = np.tanh(v.astype(np.float64)).astype(np.float32)
        if mistake == "tanh_small":  # taken as v below 2^-10, and wrong by a factor 1 + 2^-12 there
            t = np.where(np.abs(v) < 2.0 ** -10, v * np.float32(1.0 + 2.0 ** -12), t)
    return t


def arena_view(A, geo):
    return np.lib.stride_tricks.as_strided(A[geo["off"]:], (geo["nb"], geo["rows"], geo["cols"]), (4 * geo["batch"], 4 * geo["ld"], 4))


def w_of(ref, geo):
    return ref.W[geo["off"]:geo["off"] + geo["cols"]]


def gn_act_model(ref, i, op, A, mistake):
    geo = ref.operands(i)
    rowOff, rowsOut, G = geo["rows"][:3]
    x = arena_view(A, geo["act"])[:, rowOff:rowOff + rowsOut]
    B, _, C = x.shape
    rec = arena_view(A, geo["epistats"])[0].reshape(B, G, 4)
    mean, rstd = np.repeat(rec[:, :, 0], C // G, 1)[:, None, :], np.repeat(rec[:, :, 1], C // G, 1)[:, None, :]
    gn = (x - mean) * rstd * w_of(ref, geo["W.w"]) + w_of(ref, geo["W.b"])
    if op["mode"] == 1:
        kw = {"coef": mistake[1]} if isinstance(mistake, tuple) else {"clamp": mistake != "no_clamp"}
        v = gelu_model(gn, **kw)
    else:
        v = gn[:, :, :C // 2] * sigmoid_model(gn[:, :, C // 2:], flip=mistake == "sigmoid_flip")
    if "W.scale" in geo:
        v = v * w_of(ref, geo["W.scale"])
    if "res" in geo:
        v = v + arena_view(A, geo["res"])
    return v.astype(np.float32)


def gelu_linear_model(ref, i, op, A, mistake):
    geo = ref.operands(i)
    W, bias = VC.weights_of(ref, op)
    x = arena_view(A, geo["act"]).astype(np.float64)
    v = (x @ W.T.astype(np.float64) + bias).astype(np.float32)
    kw = {"coef": mistake[1]} if isinstance(mistake, tuple) else {"clamp": mistake != "no_clamp"}
    return gelu_model(v, **kw)


def glu_linear_model(ref, i, op, A, mistake):
    """a 1 x 1 conv with the GLU epilogue: columns in paired order (model_pack.cpp paired_row), no table"""
    geo = ref.operands(i)
    W, bias = VC.weights_of(ref, op)
    v = (arena_view(A, geo["act"]).astype(np.float64) @ W.T.astype(np.float64) + bias).astype(np.float32)
    c = np.arange(op["N"] // 2)
    na = (c // 16) * 32 + c % 16
    return (v[:, :, na] * sigmoid_model(v[:, :, na + 16], flip=mistake == "sigmoid_flip")).astype(np.float32)


def hterms_linear_model(ref, i, op, A, mistake):
    """a plain linear layer on fp16 terms (igemm_common.h rowscale_of, split3 in fp16): the row scaled by 2^s, s = 14 - floor(log2 max)
    capped at 126, split into three fp16 terms (a value beyond fp16's range is inf and its remainders NaN, as on the device),
    the products summed in double, scaled back, + bias. sexp_floor: s also bounded BELOW, at -64 - the cap applied to both ends"""
    geo = ref.operands(i)
    W, bias = VC.weights_of(ref, op)
    x = arena_view(A, geo["act"]).copy()
    e = ((np.abs(x).max(2).view(np.uint32) >> 23) & 0xFF).astype(np.int64) - 127
    s = np.minimum(14 - e, 126)
    if mistake == "sexp_floor":
        s = np.maximum(s, -64)
    with np.errstate(over="ignore", invalid="ignore"):
        a = x * np.ldexp(np.float32(1.0), s)[:, :, None].astype(np.float32)
        h1 = a.astype(np.float16).astype(np.float32)
        h2 = (a - h1).astype(np.float16).astype(np.float32)
        h3 = (a - h1 - h2).astype(np.float16).astype(np.float32)
        acc = (h1.astype(np.float64) + h2 + h3) @ W.T.astype(np.float64)
        return (acc * np.ldexp(1.0, -s)[:, :, None] + bias).astype(np.float32)


def stats_reduce_model(ref, i, op, A, mistake):
    geo = ref.operands(i)
    G, count, mode, eps_bits = geo["reduce"][:4]
    eps = float(np.array([eps_bits], np.uint32).view(np.float32)[0])
    P = arena_view(A, geo["rowstat"]).astype(np.float64)
    B, R_, NB2 = P.shape
    out = np.zeros((B, G, 4), np.float32)
    for b in range(B):
        for g in range(G):
            blk = P[b, g::G].reshape(-1, 2)
            s, q = blk[:, 0].sum(), blk[:, 1].sum()
            mean = s / count
            var = (q - count * mean * mean) / (count - 1.0)
            if mistake != "no_var_clamp":
                var = max(var, 0.0)
            with np.errstate(invalid="ignore"):
                sd = np.sqrt(var)
                out[b, g] = [mean, 1.0 / np.sqrt(var + eps) if mode == 0 else 1.0 / (sd + eps), sd, 0.0]
    return out


def lstm_model(ref, i, op, A, mistake):
    geo = ref.operands(i)
    H, T, B = op["K"], op["T"], geo["xproj"]["nb"]
    U = ref.W[geo["W.whh"]["off"]:geo["W.whh"]["off"] + 8 * H * H].reshape(2, 4 * H, H)
    X = arena_view(A, geo["xproj"]).reshape(B, T, 2, H, 4)
    out = np.zeros((B, T, 2, H), np.float32)
    flip = mistake == "sigmoid_flip"
    for b in range(B):
        for d in range(2):
            h, c, h2 = np.zeros(H, np.float32), np.zeros(H, np.float32), np.zeros(H, np.float32)
            for step in range(T):
                t = step if d == 0 else T - 1 - step
                used = h.copy()
                if mistake == "stale_h" or (mistake == "stale_h_late" and step >= 8):  # one block of 16 units read from the exchange
                    used[:16] = h2[:16]                                                  # buffer as it was two steps ago
                pre = X[b, t, d] + (U[d] @ used).reshape(H, 4)
                c = sigmoid_model(pre[:, 1], flip) * c + sigmoid_model(pre[:, 0], flip) * tanh_model(pre[:, 2], mistake)
                h2, h = h, sigmoid_model(pre[:, 3], flip) * tanh_model(c, mistake)
                out[b, t, d] = h
    return out


def smooth_gn_act(ref, i, op, rng):
    geo = ref.operands(i)
    ref.view(geo["act"])[...] = VC.f32(0.7 * rng.standard_normal(ref.view(geo["act"]).shape))
    ref.view(geo["epistats"])[0][:] = VC.f32([0.0, 1.0, 1.0, 0.0])


def smooth_linear(ref, i, op, rng):
    W, _ = VC.weights_of(ref, op)
    x = ref.view(ref.operands(i)["act"])
    x[...] = VC.f32(0.9 / (np.sqrt(np.mean(W.astype(np.float64) ** 2)) * np.sqrt(op["K"])) * rng.standard_normal(x.shape))


def smooth_stats_reduce(ref, i, op, rng):
    geo = ref.operands(i)
    P = ref.view(geo["rowstat"])
    n_per = geo["reduce"][1] * geo["reduce"][0] / (P.shape[1] * P.shape[2] // 2)
    e, z = rng.standard_normal(P.shape[:2] + (P.shape[2] // 2,)), rng.standard_normal(P.shape[:2] + (P.shape[2] // 2,))
    P[:, :, 0::2] = VC.f32(0.3 * n_per + np.sqrt(n_per) * e)
    P[:, :, 1::2] = VC.f32(n_per * 1.09 + 0.6 * np.sqrt(n_per) * e + np.sqrt(0.5 * n_per) * z)


def smooth_lstm(ref, i, op, rng):
    x = ref.view(ref.operands(i)["xproj"])
    x[...] = VC.f32(0.5 * rng.standard_normal(x.shape))


# (case, arithmetic, family, op filter, model, smooth operands, mistakes[, the case of the smooth operands if another]). The mistakes:
#   erf_coef      the linear coefficient of dmx_erff's upper range off by d. It moves erf by at most d ln 2 max t erfc(t) = 0.12 d, most
#                 near the seam: GELU by 1.0e6 d u |v|. The K_eff = 1 bound in fp32 is c = 9 times s = |gelu| + 1.13 (|a w| + |b|), 1.2
#                 (negative side) to 2 |v|: 11 to 18 u |v|. d = 1e-5 (10 u |v|) is inside it on any finite operand; d = 2e-5 is the
#                 first round figure outside it on both sides and is what is seeded. The window is narrow: from 5e-5 on the RMS rule
#                 rejects the mistake on the smooth operands of the same layer as well (6 to 8 % of their arguments are near the seam),
#                 as it does from 1e-5 on for gn_act, whose c = 20 puts it under that rule
#   no_clamp      min(|x|, 4) removed: the degree-6 exponent turns upwards and overflows exp2 beyond |z| about 11
#   sigmoid_flip  the sigmoid returning 1 - sigma for |v| > 17
#   tanh_quotient the LSTM's tanh as (e^2v - 1) / (e^2v + 1): NaN once |c| passes 44 (T = 65 only). It stands in for "tanh taken as v
#                 and wrong by 1 + 2^-12 below 2^-10", which no operand can show: the reference grants the LSTM's tanh the magnitude 1
#                 whatever |v| (cpu_interp.cpp tanh_), so h = o tanh(c) near 0 is allowed T (K + 24) u / 2, four orders above it
#   stale_h_late  one block of 16 units reads h of step - 2 from the eighth step on (an exchange buffer's fourth reuse): the same LSTM
#                 layer never gets there on the smooth case's 7 steps. (Stale from the first reuse on is rejected on any operands.)
#   no_var_clamp  the variance clamp removed
#   sexp_floor    the fp16-term row scale's exponent bounded below as well (at -64): the 2^100 rows overflow fp16. It stands in for "a
#                 zero row scaled by 1", which no output can show: the products of a zero row are zero under any scale
LINEAR1 = lambda op: op["act"] == 1 and op["epi"] == R.EPI_LINEAR and "linear1" in op["name"]  # noqa: E731
SEEDED = [
    ("v3_7000", "f32", "gn_act", lambda op: op["mode"] == 1, gn_act_model, smooth_gn_act, ["no_clamp"]),
    ("v3_7000", "f32", "gn_act", lambda op: op["mode"] == 2, gn_act_model, smooth_gn_act, ["sigmoid_flip"]),
    ("6s_7000", "f32", "gemm_plain", LINEAR1, gelu_linear_model, smooth_linear, ["no_clamp", ("erf_coef", 2e-5)]),
    ("6s_7000", "bf16x3", "gemm_plain", lambda op: op["epi"] == R.EPI_GLU and op["name"] == "tencoder.0.rewrite", glu_linear_model, smooth_linear,
     ["sigmoid_flip"]),
    ("4s_8000", "fp16x3", "gemm_hterms", lambda op: op["name"] == "channel_upsampler", hterms_linear_model, smooth_linear, ["sexp_floor"]),
    ("4s_8000", "bf16x3", "stats_reduce", lambda op: True, stats_reduce_model, smooth_stats_reduce, ["no_var_clamp"]),
    ("v3_66560", "bf16x3", "lstm", lambda op: op["T"] == 65, lstm_model, smooth_lstm, ["sigmoid_flip", "tanh_quotient"]),
    ("v3_66560", "bf16x3", "lstm", lambda op: op["K"] == 192, lstm_model, smooth_lstm, ["stale_h_late"], "v3_7000"),
]


def verdicts(L, tmp_models, case, mode, fam, pick, model, smooth, mistakes, smooth_case=None):
    """{mistake (None: the honest model): (rejected on the crafted operands in some round, rejected on the smooth ones)}"""
    out = {m: [False, False] for m in [None] + list(mistakes)}
    for where, at in ((0, case), (1, smooth_case or case)):
        ref = make_ref(L, tmp_models, at, mode)
        i = next(k for k, o in enumerate(ref.ops) if VC.family_of(o) == fam and pick(o))
        op = ref.ops[i]
        for rnd in range(VC.rounds_of(ref, i, fam) if where == 0 else 1):
            if where == 0:
                K_eff = VC.craft(ref, i, at, rnd)["K_eff"]
            else:
                rng = np.random.default_rng(VC.seed_of(at, op, 99))
                VC.fill_reads(ref, op, rng)
                smooth(ref, i, op, rng)
                K_eff = None
            snap, before, _, verdict = both_steps(ref, i, op, mode, K_eff)
            assert not isinstance(verdict, str), verdict
            assert np.all(np.diff(snap["idx"]) == 1), "the models write one contiguous range"
            for m in out:
                got = before.copy()
                got.view(np.float32)[snap["idx"]] = model(ref, i, op, before.view(np.float32), m).ravel()
                out[m][where] |= R.rejects(op, mode, got, before, snap, verdict[1], K_eff)
        ref.close()
    return op["name"], {m: tuple(v) for m, v in out.items()}


@pytest.mark.parametrize("k", range(len(SEEDED)))
def test_seeded_mistakes_are_rejected_on_crafted_operands_and_accepted_on_smooth_ones(k, L, tmp_models):
    case, mode, fam, pick, model, smooth, mistakes = SEEDED[k][:7]
    name, v = verdicts(L, tmp_models, case, mode, fam, pick, model, smooth, mistakes, *SEEDED[k][7:])
    assert v[None] == (False, False), f"{name}: the honest model is rejected {v[None]}"
    for m in mistakes:
        assert v[m] == (True, False), f"{name}: {m}: rejected (crafted, smooth) = {v[m]}"
