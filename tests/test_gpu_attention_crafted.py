"""The attention kernels on crafted operands (tests/attention_cases.py): every attention op of four small plans, alone, on operands
that make fragments raise the deferred running maximum after the first key tile - the value-driven branch of
attention_common.h att_softmax_pre that the operands of a random mixture never take (tests/test_attention_crafted_cpu.py shows
both, and that the check below rejects a rescale that is skipped or takes the wrong alpha).

Per attention op (the chain is not stepped: the ops are independent): the crafted operands are written through
interp_set_attention into the reference's arena and from there into the op's read ranges on the device; the reference takes its
precise step; the plan's own form is launched from canary A and again with canary B outside the read ranges and judged by
op_reference.check_launch (value bound, containment, reads, and the RMS rule against the interpreter's fp32 arithmetic on the same
operands) - the very check tests/test_gpu_op_parity.py applies. Then every other form (dmx_debug_run_attention_as: wg64, wg128,
pair where it exists) must leave bit-identical outputs (the claim of attention_select.h) and keep containment; a form that does
not exist must be refused. Across the module every kernel instance listed in KERNELS has run on crafted operands. One case runs
once more under DMX_KV_PLANES=0: the fp32-K/V path of the split kernel must give the bits of the planes path (the claim in the
header of attention_split.hip).

Cases: attention_cases.CASES. v3_133120 is the smallest segment at which a LocalState op has T >= 130 (T = segment / 1024 for
encoder.4, half of it for encoder.5: 130 and 65 tokens); its arena is 56.5 M floats (226 MB on the device; the interpreter's
host arena with the precise values and magnitudes 1.0 GB).

On a HIP error the binding raises and nothing more is launched by any op-level test (op_reference.DEVICE_ERROR).
DMX_OP_PARITY_RECORD=<dir> writes op_parity_crafted_<case>_<mode>.txt (profiles/op_parity_crafted_*.txt are such records)."""
import os

import numpy as np
import pytest

import attention_cases as AC
import op_reference as R

pytestmark = pytest.mark.gpu

FORMS = ("wg64", "wg128", "pair")
# (kernel, form, head dim, reads operand planes): every instance of the three attention kernels a plan can launch
KERNELS = ({("attention", f, hs, False) for f in ("wg64", "wg128") for hs in (64, 48)}
           | {("attention_split", f, hs, pl) for f in ("wg64", "wg128") for hs in (64, 48) for pl in (False, True)}
           | {("attention_split", "pair", hs, True) for hs in (64, 48)}
           | {("attention_loc", "wg64", hs, False) for hs in (48, 96)})
RUNS = {}  # (case, mode, planes switch) -> what run_case returned


@pytest.fixture(scope="module")
def L():
    return R.lib()


@pytest.fixture(scope="module")
def dmxb():
    from demucs_cpp_amd import binding

    assert binding.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return binding


def kernel_of(op, form):
    if op["kind"] == R.OP_LOCAL_ATTN:
        return ("attention_loc", form, op["K"], False)
    return (op["label"], form, op["K"], bool(op["planes"]) and op["T"] % AC.KT == 0)


def form_exists(op, form, mode):
    if op["kind"] == R.OP_LOCAL_ATTN:
        return form == "wg64"
    return form != "pair" or bool(op["split"] and op["planes"] and op["T"] % AC.KT == 0 and mode != "f32")


def check_case_shapes(case, ops):
    if case in AC.TOKENS:
        want = {(a, b) for a in AC.TOKENS[case] for b in AC.TOKENS[case]}
        assert len(ops) == 10 and {(o["Tq"], o["T"]) for o in ops} == want, [(o["name"], o["Tq"], o["T"]) for o in ops]
    else:
        assert {o["K"]: o["T"] for o in ops} == AC.LOC_T[case] and all(o["kind"] == R.OP_LOCAL_ATTN for o in ops)


def run_ops(pair, all_forms):
    ref, ctx, B, mode = pair.ref, pair.ctx, pair.B, pair.mode
    rows, failures, launched, bits_of = [], [], set(), {}
    att = [i for i, o in enumerate(pair.gops) if o["kind"] in (R.OP_ATTENTION, R.OP_LOCAL_ATTN)]
    check_case_shapes(pair.case, [pair.gops[i] for i in att])
    for i in att:
        op = pair.gops[i]
        shape = AC.shape_of(op, B)
        x = AC.craft(shape, AC.seed_of(pair.case, op))
        ref.set_attention(i, x["q"], x["k"], x["v"], x["decay"])
        reads = op["reads"]
        values = [ref.A[lo:hi].copy() for lo, hi in reads]
        ref.step(i, True)
        snap = R.snapshot(ref, op)
        own = op["form"] if op["kind"] == R.OP_ATTENTION else "wg64"
        try:
            launched.add(kernel_of(op, own))
            worst, rms_g, rms_f, bits = R.check_launch(pair, i, i, op, reads, values, snap)
            bits_of[op["name"]] = bits
            counts, margin, raises, decisions = AC.op_events(shape, x)
            rows.append((op["name"], kernel_of(op, own), R.bound_c(op, mode), worst, rms_g, rms_f, raises, decisions, margin, counts))
            for form in FORMS if all_forms else ():
                if form == own:
                    continue
                pair.prepare(R.CANARY_A, reads, values)
                ran = ctx.run_attention_as(B, i, form)
                if (ran is not None) != form_exists(op, form, mode):
                    raise R.OpMismatch(f"{op['name']}: form {form} {'ran' if ran else 'was refused'}")
                if ran is None:
                    continue
                launched.add(kernel_of(op, form))
                got = ctx.arena_read(0, pair.ctx_floats, pair.buf).view(np.uint32)
                before = R.expected_arena(pair.ctx_floats, R.CANARY_A, pair.consts_u32, reads, values)
                try:
                    R.check_op(op, mode, got, before, snap)
                except R.OpMismatch as e:
                    raise R.OpMismatch(f"as {form}: {e}")
                if not np.array_equal(R.written_bits(lambda lo, hi: got[lo:hi], op, snap), bits):
                    raise R.OpMismatch(f"{op['name']}: form {form} differs in bits from the plan's form {own}")
        except R.OpMismatch as e:  # (every op is reported, not the first only)
            failures.append(str(e))
    return rows, failures, launched, bits_of


def run_case(dmxb, L, tmp_models, case, mode, planes_off=False, all_forms=True):
    key = (case, mode, planes_off)
    if key not in RUNS:
        pair = R.Pair(dmxb, L, tmp_models, case, mode, cases=AC.CASES)
        try:
            pair.assert_same_plan()
            RUNS[key] = run_ops(pair, all_forms)
        except dmxb.DmxError as e:
            R.DEVICE_ERROR.append(str(e))
            raise
        finally:
            pair.close()
        record(case, mode, "_noplanes" if planes_off else "", RUNS[key])
    return RUNS[key]


def record(case, mode, tag, run):
    d = os.environ.get("DMX_OP_PARITY_RECORD")
    if not d:
        return
    os.makedirs(d, exist_ok=True)
    rows, failures, _, _ = run
    with open(os.path.join(d, f"op_parity_crafted_{case}_{mode}{tag}.txt"), "w") as f:
        f.write("# op\tkernel form hs planes\tc\tworst |g - r| / (u s)\tRMS (g - r) / (u s)\tRMS of the fp32 interpreter\t"
                "raises / decisions after tile 0\tsmallest margin\t" + "\t".join(AC.CLASSES) + "\n")
        for name, kern, c, worst, rg, rf, raises, decisions, margin, counts in rows:
            f.write(f"{name}\t{' '.join(str(k) for k in kern)}\t{c}\t{worst:.3f}\t{rg:.4f}\t{'-' if rf is None else format(rf, '.4f')}\t"
                    f"{raises} / {decisions}\t{margin:.2f}\t" + "\t".join(str(counts[k]) for k in AC.CLASSES) + "\n")
        for msg in failures:
            f.write(f"# MISMATCH {msg}\n")


PARAMS = [(c, m) for c, v in AC.CASES.items() for m in v[3]]


@pytest.mark.parametrize("case,mode", PARAMS)
def test_attention_on_crafted_operands_in_every_form(case, mode, dmxb, L, tmp_models):
    rows, failures, _, _ = run_case(dmxb, L, tmp_models, case, mode)
    assert not failures, failures[:12]
    assert len(rows) == (10 if case in AC.TOKENS else 4)
    for name, _, _, _, _, _, raises, _, margin, _ in rows:  # the operands are the ones the CPU test proved
        assert margin >= AC.MARGIN and (raises >= 5 or "encoder.5." in name), (name, margin, raises)


def test_every_kernel_instance_ran_on_crafted_operands(dmxb, L, tmp_models):
    launched = set()
    for case, mode in PARAMS:
        launched |= run_case(dmxb, L, tmp_models, case, mode)[2]
    assert not KERNELS - launched, f"never launched on crafted operands: {sorted(KERNELS - launched)}"


def test_the_fp32_kv_path_gives_the_bits_of_the_planes_path(dmxb, L, tmp_models, monkeypatch):
    """4s_49152 in bf16x3: every attention op reads operand planes. Under DMX_KV_PLANES=0 (read per plan) the same ops split fp32 K / V
    rows themselves: the same crafted K / V (the planes hold their exact split) must give the same output bits"""
    case, mode = "4s_49152", "bf16x3"
    _, failures, launched, bits = run_case(dmxb, L, tmp_models, case, mode)
    assert not failures and all(k[3] for k in launched if k[0] == "attention_split"), (failures[:4], launched)
    monkeypatch.setenv("DMX_KV_PLANES", "0")
    _, failures0, launched0, bits0 = run_case(dmxb, L, tmp_models, case, mode, planes_off=True, all_forms=False)
    assert not failures0, failures0[:12]
    assert launched0 and not any(k[3] for k in launched0), launched0
    assert set(bits) == set(bits0) and len(bits) == 10
    differ = [n for n in bits if not np.array_equal(bits[n], bits0[n])]
    assert not differ, f"outputs differ in bits between the planes path and the fp32-K/V path: {differ}"
