"""The crafted attention operands (tests/attention_cases.py) proven on the CPU, before a GPU is involved:
 * the conditions of the design hold for every attention op of every case: every decision of the deferred maximum at least 1 exp2
   unit from the threshold, every level within +-128, every class of decision its shape can have taken after tile 0;
 * interp_set_attention writes the operands where the op reads them: the precise step equals an independent numpy fp64 softmax;
 * the interpreter's own fp32 arithmetic stays within the existing bound on the crafted operands, and its RMS (the yardstick of the
   RMS rule) is at least what a plain random fill gives;
 * teeth: the numpy tile model passes the GPU test's verdict (op_reference.rejects) honest and with the maximum raised on every
   tile; with the rescale of O or of the row sum skipped, alpha taken from the neighbouring query or the mask off by one it is
   rejected on the crafted operands - and the three rescale mistakes are ACCEPTED on the random fill (no bit differs: nothing is
   ever rescaled there), which is why these operands were needed. A mask off by one lets another key through whatever the values,
   so it is rejected on both.
One op of every distinct (shape, operand form) of a case is stepped; the conditions are computed for all of them.
DMX_OP_PARITY_RECORD=<dir> writes op_parity_crafted_cpu.txt (profiles/op_parity_crafted_cpu.txt is such a record)."""
import os

import numpy as np
import pytest

import attention_cases as AC
import op_reference as R

# (case, arithmetic): planes and fp32-K/V plans at head dims 64 and 48, LocalState at 48 and 96
SWEEPS = [("4s_49152", "bf16x3"), ("4s_40960", "bf16x3"), ("4s_40960", "f32"), ("6s_24576", "bf16x3"), ("6s_24576", "f32"), ("v3_133120", "f32")]


@pytest.fixture(scope="module")
def L():
    return R.lib()


def attention_ops(ops):
    return [i for i, o in enumerate(ops) if o["kind"] in (R.OP_ATTENTION, R.OP_LOCAL_ATTN)]


def implementation_arena(before, snap, out):
    g = before.copy()
    g.view(np.float32)[snap["idx"]] = out.ravel()
    return g


def sweep_case(L, tmp_models, case, mode):
    key, seg, B, _ = AC.CASES[case]
    ref = R.Ref(L, tmp_models[key], seg, B, mode, mode != "f32" and key != 3)
    rows, seen = [], set()
    for i in attention_ops(ref.ops):
        op = ref.ops[i]
        shape = AC.shape_of(op, B)
        x = AC.craft(shape, AC.seed_of(case, op))
        counts, margin, raises, decisions = AC.op_events(shape, x)
        row = dict(i=i, name=op["name"], shape=shape, planes=op.get("planes", 0), counts=counts, margin=margin, raises=raises,
                   decisions=decisions, levels=x["levels"], kinds=x["kinds"])
        rows.append(row)
        form = (shape["Tq"], shape["Tk"], shape["hs"], shape["loc"], row["planes"])
        if form in seen:
            continue
        seen.add(form)
        rnd = AC.random_fill(shape, AC.seed_of(case, op))
        row["random_raises"] = AC.op_events(shape, rnd)[2]
        for tag, ops in (("crafted", x), ("random", rnd)):
            ref.set_attention(i, ops["q"], ops["k"], ops["v"], ops["decay"])
            saved, before = R.canary_arena(ref, op["reads"], R.CANARY_A)
            ref.step(i, False)
            fp32 = ref.A.view(np.uint32).copy()
            ref.A[:] = saved
            ref.step(i, True)
            snap = R.snapshot(ref, op)
            assert snap["idx"].size == shape["B"] * shape["Tq"] * shape["H"] * shape["hs"] and np.all(np.diff(snap["idx"]) == 1)
            want = AC.softmax_fp64(shape, ops).ravel()
            row[tag + "_roundtrip"] = float(np.abs(snap["r"] - want).max() / np.abs(want).max())
            try:
                worst, q = R.check_op(op, mode, fp32, before, snap)
                row[tag + "_fp32"] = (worst, R.rms(q))
            except R.OpMismatch as e:
                row[tag + "_fp32"] = (str(e), float("nan"))
                continue
            rms_f = R.rms(q)
            verdict = {}
            for what in (None, "never_defer_threshold_0") + AC.MISTAKES:
                out = AC.tile_model(shape, ops, mistake=what if what in AC.MISTAKES else None, threshold=0.0 if what == "never_defer_threshold_0" else AC.DEFER)
                got = implementation_arena(before, snap, out)
                verdict[what] = R.rejects(op, mode, got, before, snap, rms_f)
                if what is None:
                    _, qm = R.check_op(op, mode, got, before, snap) if not verdict[what] else (0, np.zeros(1))
                    row[tag + "_model_rms"] = R.rms(qm)
                    honest = out
                elif what in AC.VALUE_DRIVEN:
                    verdict[what + "_same_bits"] = bool(np.array_equal(out.view(np.uint32), honest.view(np.uint32)))
            row[tag + "_verdict"] = verdict
    ref.close()
    return rows


@pytest.fixture(scope="module")
def sweeps(L, tmp_models):
    out = {(case, mode): sweep_case(L, tmp_models, case, mode) for case, mode in SWEEPS}
    d = os.environ.get("DMX_OP_PARITY_RECORD")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "op_parity_crafted_cpu.txt"), "w") as f:
            f.write("# case\tmode\top\tTq\tTk\ths\tplanes\traises / decisions after tile 0\tsmallest margin\tlargest |level|\t" + "\t".join(AC.CLASSES) +
                    "\tfp32 interpreter: worst, RMS (crafted)\tRMS (random fill)\ttile model RMS (crafted)\traises on the random fill\n")
            for (case, mode), rows in out.items():
                for r in rows:
                    s = r["shape"]
                    f.write(f"{case}\t{mode}\t{r['name']}\t{s['Tq']}\t{s['Tk']}\t{s['hs']}\t{r['planes']}\t{r['raises']} / {r['decisions']}\t{r['margin']:.2f}\t"
                            f"{r['levels']:.1f}\t" + "\t".join(str(r["counts"][c]) for c in AC.CLASSES))
                    if "crafted_fp32" in r:
                        cw, cr = r["crafted_fp32"]
                        f.write(f"\t{cw if isinstance(cw, str) else format(cw, '.3f')}, {cr:.4f}\t{r['random_fp32'][1]:.4f}\t{r.get('crafted_model_rms', float('nan')):.4f}\t{r['random_raises']}")
                    f.write("\n")
    return out


def stepped(sweeps):
    return [(key, r) for key, rows in sweeps.items() for r in rows if "crafted_roundtrip" in r]


def test_the_cases_have_the_token_counts_and_the_operand_forms_they_are_for(sweeps):
    for (case, mode), rows in sweeps.items():
        if case in AC.TOKENS:
            assert len(rows) == 10 and {(r["shape"]["Tq"], r["shape"]["Tk"]) for r in rows} == {(a, b) for a in AC.TOKENS[case] for b in AC.TOKENS[case]}
        else:
            assert {r["shape"]["hs"]: r["shape"]["Tq"] for r in rows} == AC.LOC_T[case] and max(r["shape"]["Tq"] for r in rows) >= 130
    forms = {(r["shape"]["hs"], bool(r["planes"]), r["shape"]["loc"]) for _, r in stepped(sweeps)}
    assert forms >= {(64, True, False), (64, False, False), (48, True, False), (48, False, False), (48, False, True), (96, False, True)}


def test_every_decision_keeps_its_margin_and_every_level_its_range(sweeps):
    for key, rows in sweeps.items():
        for r in rows:
            assert r["margin"] >= AC.MARGIN, (key, r["name"], r["margin"])
            assert r["levels"] <= 128.0, (key, r["name"], r["levels"])


def test_every_class_of_decision_is_taken_after_tile_0(sweeps):
    for key, rows in sweeps.items():
        for r in rows:
            missing = [c for c in AC.classes_possible(r["shape"]) if r["counts"][c] == 0]
            assert not missing, (key, r["name"], missing, r["counts"])
            assert r["raises"] >= AC.raises_expected(r["shape"]), (key, r["name"], r["raises"])


def test_the_setter_round_trip_equals_numpy_fp64(sweeps):
    for key, r in stepped(sweeps):
        assert r["crafted_roundtrip"] <= 1e-12 and r["random_roundtrip"] <= 1e-12, (key, r["name"], r["crafted_roundtrip"], r["random_roundtrip"])


def test_the_fp32_interpreter_stays_within_the_bound_on_crafted_operands(sweeps):
    for key, r in stepped(sweeps):
        for tag in ("crafted_fp32", "random_fp32"):
            assert not isinstance(r[tag][0], str), (key, r["name"], r[tag][0])


def test_the_yardstick_is_no_smaller_than_on_a_random_fill(sweeps):
    for key, r in stepped(sweeps):
        assert r["crafted_fp32"][1] >= r["random_fp32"][1], (key, r["name"], r["crafted_fp32"][1], r["random_fp32"][1])


def test_the_check_rejects_the_rescale_mistakes_on_crafted_operands_only(sweeps):
    for key, r in stepped(sweeps):
        c, n = r["crafted_verdict"], r["random_verdict"]
        where = (key, r["name"])
        assert not c[None] and not c["never_defer_threshold_0"], (where, c)
        assert not n[None] and not n["never_defer_threshold_0"], (where, n)
        masked = r["shape"]["Tk"] % AC.KT != 0
        for what in AC.MISTAKES:
            if not masked if what == "mask_off_by_one" else AC.raises_expected(r["shape"]) == 0:
                continue  # (whole key tiles: no mask; LocalState at T = 65: nothing the decay could raise)
            assert c[what], f"{where}: not rejected on the crafted operands: {what}"
        assert r["random_raises"] == 0, where
        for what in AC.VALUE_DRIVEN:
            assert not n[what] and n[what + "_same_bits"], f"{where}: {what} shows on a random fill"
