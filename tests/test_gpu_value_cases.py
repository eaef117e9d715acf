"""The kernels with value-dependent code on crafted operands (tests/value_cases.py): GELU and GLU epilogues and prologues of the
GEMMs past the seam and the clamp of dmx_erff and past the points where the sigmoid's exponential saturates and overflows, the
fp16-term row scale on zero, denormal and huge rows, LayerNorm, the GroupNorm statistics and the statistics reduction on rows
with a far mean, constant, zero and spiked rows (the variance clamp), gn_act, the row-resident DConv, and the LSTM with saturated
and vanishing gates at T = 65 and 33. tests/test_value_cases_cpu.py proves the operands, shows that the check below rejects seeded
mistakes on them and accepts the same mistakes on smooth operands.

Per (case, arithmetic) one op of every kernel instance of the nine families (value_cases.select) is taken alone, the chain is not
stepped: per round the crafted operands go from the reference's arena into the op's read ranges on the device, the reference
takes its precise step, and the plan's kernel is launched from canary A and again with canary B outside the read ranges and
judged by op_reference.check_launch (value bound - with K_eff where the operand puts one or two non-zeros into a sum -,
containment, reads, and the RMS rule against the interpreter's fp32 arithmetic on the same operands): the very check
tests/test_gpu_op_parity.py applies. In two cases one GEMM of every distinct (prologue, epilogue, activation) also runs on every
tile and family of its shape (op_reference.run_variants with the same K_eff: each distinct kernel meets the bound of its own
arithmetic, kernels of one arithmetic are bit-identical). Every instance a case's plan launches among the families has run.

The LSTM kernels spin on partner workgroups with a bounded count; a raised status word comes back as an error of the launch and
ends the run, like any HIP error: nothing more is launched by any op-level test (op_reference.DEVICE_ERROR).
DMX_OP_PARITY_RECORD=<dir> writes op_parity_values_<case>_<mode>.txt (profiles/op_parity_values_*.txt are such records)."""
import os

import numpy as np
import pytest

import op_reference as R
import value_cases as VC

pytestmark = pytest.mark.gpu

SIBLINGS = (("4s_8000", "bf16x3"), ("6s_7000", "f32"))
RUNS = {}


@pytest.fixture(scope="module")
def L():
    return R.lib()


@pytest.fixture(scope="module")
def dmxb():
    from demucs_cpp_amd import binding

    assert binding.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return binding


def run_ops(pair, siblings):
    ref, mode, case = pair.ref, pair.mode, pair.case
    rows, failures, launched, variants, shapes = [], [], set(), {"checked": 0, "refused": set()}, set()
    for inst, i in VC.select(ref, case).items():
        op, fam = pair.gops[i], inst[0]
        for rnd in range(VC.rounds_of(ref, i, fam)):
            info = VC.craft(ref, i, case, rnd)
            reads = op["reads"]
            values = [ref.A[lo:hi].copy() for lo, hi in reads]
            ref.step(i, True, hterms=op["kind"] == R.OP_IGEMM and op["arith"] == 2)
            census = ref.census()
            snap = R.snapshot(ref, op)
            c = R.bound_c(R.effective(op, info["K_eff"]), mode)
            try:
                launched.add(inst)
                worst, rms_g, rms_f, bits = R.check_launch(pair, i, i, op, reads, values, snap, info["K_eff"])
                rows.append((op["name"], inst, rnd, c, worst, rms_g, rms_f, census))
                shape = (op.get("pro"), op.get("epi"), op.get("act"))
                if siblings and op["kind"] == R.OP_IGEMM and rnd == 0 and shape not in shapes:
                    shapes.add(shape)
                    R.run_variants(pair, i, op, reads, values, snap, bits, variants, [], info["K_eff"])
            except R.OpMismatch as e:  # (every op is reported, not the first only)
                failures.append(f"round {rnd}: {e}")
                rows.append((op["name"], inst, rnd, c, float("nan"), float("nan"), None, census))
    want = {VC.instance_of(ref, i) for i in range(ref.n_ops)} - {None}
    if case in VC.LSTM_ONLY:
        want = {w for w in want if w[0] == "lstm"}
    return rows, failures, launched, want, variants


def run_case(dmxb, L, tmp_models, case, mode):
    key = (case, mode)
    if key not in RUNS:
        pair = R.Pair(dmxb, L, tmp_models, case, mode, cases=VC.CASES)
        try:
            pair.assert_same_plan()
            RUNS[key] = run_ops(pair, key in SIBLINGS)
        except dmxb.DmxError as e:
            R.DEVICE_ERROR.append(str(e))
            raise
        finally:
            pair.close()
        record(case, mode, RUNS[key])
    return RUNS[key]


def record(case, mode, run):
    d = os.environ.get("DMX_OP_PARITY_RECORD")
    if not d:
        return
    os.makedirs(d, exist_ok=True)
    rows, failures, _, _, variants = run
    with open(os.path.join(d, f"op_parity_values_{case}_{mode}.txt"), "w") as f:
        f.write("# op\tkernel instance\tround\tc\tworst |g - r| / (u s)\tRMS (g - r) / (u s)\tRMS of the fp32 interpreter (ops under the RMS rule)\t"
                "census (classes that hold evaluations)\n")
        for name, inst, rnd, c, worst, rg, rf, census in rows:
            f.write(f"{name}\t{' '.join(str(k) for k in inst)}\t{rnd}\t{c}\t{worst:.3f}\t{rg:.4f}\t{'-' if rf is None else format(rf, '.4f')}\t"
                    + " ".join(f"{k}={n}" for k, n in census.items() if n) + "\n")
        if (case, mode) in SIBLINGS:
            f.write(f"# sibling kernels checked on crafted operands: {variants['checked']}\n")
        for msg in failures:
            f.write(f"# MISMATCH {msg}\n")


PARAMS = [(c, m) for c, v in VC.CASES.items() for m in v[3]]


@pytest.mark.parametrize("case,mode", PARAMS)
def test_crafted_operands_against_fp64(case, mode, dmxb, L, tmp_models):
    rows, failures, _, want, _ = run_case(dmxb, L, tmp_models, case, mode)
    assert not failures, failures[:12]
    assert len(rows) >= len(want)


@pytest.mark.parametrize("case,mode", PARAMS)
def test_every_kernel_instance_ran_on_crafted_operands(case, mode, dmxb, L, tmp_models):
    _, _, launched, want, _ = run_case(dmxb, L, tmp_models, case, mode)
    assert want and not want - launched, f"never launched on crafted operands: {sorted(want - launched, key=str)}"


@pytest.mark.parametrize("case,mode", SIBLINGS)
def test_sibling_kernels_meet_the_bound_and_the_bit_claim_on_crafted_operands(case, mode, dmxb, L, tmp_models):
    _, failures, _, _, variants = run_case(dmxb, L, tmp_models, case, mode)
    assert not failures, failures[:12]
    assert variants["checked"] >= 8, variants
