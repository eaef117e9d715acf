"""Every op of a plan, alone, on known inputs: the HIP kernel the context would launch against an fp64 evaluation of the same op
(tests/cpu_interp.cpp interp_step in double; tests/op_reference.py holds the bound and the check, tests/test_op_reference_cpu.py
tests the harness itself without a GPU).

Per launching op, in plan order: the device arena is filled with canary A (a quiet NaN), the reference chain's values are
uploaded over the op's read ranges, the op is launched alone (dmx_debug_run_op: launch_op on the context's stream, then a checked
synchronisation), and the arena comes back. Then
  values       every element the reference wrote is within c u s of the fp64 value (op_reference.bound_c); K / V operand planes
               by the fp64 sum of their three bf16 terms, which must be an fp32 number split in order;
  containment  every other float of the arena - outside the write ranges, row padding and cropped positions inside them, the
               constants, the inputs - is bit for bit what it was (the scratch ranges an op declares are exempt);
  reads        a second launch with canary B (a large finite value) in the unread part writes the same bits: the op_access read
               ranges the two-stream waits are derived from are the only reads;
  rms          wherever the worst-case bound is loose (every op whose c exceeds op_reference.RMS_MIN_C: GEMMs, attention, LayerNorm,
               STFT / inverse STFT, LSTM, LocalState, the row-resident DConv, ...) the RMS of (g - r) / (u s) is at most 4 x that
               of the interpreter's fp32 arithmetic on the same inputs (op_reference.rms_rule_ok: no floor, no exception).
The constants (window, twiddles, window sums, positional tables) are restored by both fills: a read of a constant the op does not
declare is NOT detected by the second launch (constants are never written after context creation, so no wait depends on them).
Inputs always come from the reference chain, so one wrong kernel cannot mask or poison the next. On a HIP error the binding
raises and the test ends there: nothing more is launched.

The variant sweep runs every GEMM of two cases on every tile of its shape's chain (dmx_debug_run_op_as), see
test_every_tile_and_family_*.

What the sweep does NOT reach, and what does: its inputs are what a 0.1 randn mixture produces through synthetic weights. On those
the attention kernels raise their deferred running maximum on the first key tile only, run in 64-query workgroups only, and see
LocalState with a handful of tokens in one masked tile: tests/test_gpu_attention_crafted.py covers those paths on operands
written straight into the attention ops' read ranges. And on those no GELU argument passes the clamp of dmx_erff (8 % are in its
upper range at all), no sigmoid or LSTM gate saturates, no normalised row has a mean beyond half its deviation or is constant,
zero or spiked, no variance is clamped, no fp16-term row is zero, denormal or huge, and the LSTM runs 7 and 4 steps:
tests/test_gpu_value_cases.py covers those classes, one op per kernel instance, on operands written by role into the ops' read
ranges (tests/value_cases.py; the census of the reference says which classes a launch evaluated). Pair, check_launch,
written_bits and run_variants are shared by the three tests: op_reference.py. Still unreached by any of them
(value_cases.UNREACHABLE): the variance clamp of group_stats as a DECIDED class (a constant group of elements is launched, but
whether its one-pass variance rounds below zero is up to the order of a double summation; only fp32 partials, the statistics
reduction's input, can be made to decide it), and the row-resident DConv's activations beyond their middle ranges (a GroupNorm
in front of each bounds them).

DMX_OP_PARITY_RECORD=<dir> writes the per-op figures (profiles/op_parity_*.txt are such records)."""
import os

import numpy as np
import pytest

import op_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return R.lib()


@pytest.fixture(scope="module")
def dmxb():
    from demucs_cpp_amd import binding

    assert binding.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    return binding


Pair, DEVICE_ERROR, written_bits = R.Pair, R.DEVICE_ERROR, R.written_bits  # (shared with tests/test_gpu_attention_crafted.py)


def check_launch(pair, i, j, op, reads, values, snap, rows, launched, variants):
    launched.append((op.get("cfg", -1), op.get("family", -1), op.get("label")))
    worst, rms_g, rms_f, bits_a = R.check_launch(pair, i, j, op, reads, values, snap)
    with np.errstate(divide="ignore", invalid="ignore"):
        loose = float(np.nanmedian(snap["s"] / np.abs(snap["r"]))) if snap["idx"].size else 0.0  # how far s is above |r|: the bound's slack
    rows.append((op["name"], op.get("label"), op.get("K", 0), R.bound_c(op, pair.mode), worst, rms_g, rms_f, loose))
    if variants is not None and op["kind"] == R.OP_IGEMM:
        R.run_variants(pair, j, op, reads, values, snap, bits_a, variants, launched)


def sweep(pair, variants=None):
    try:
        return sweep_ops(pair, variants)
    except pair.dmxb.DmxError as e:
        DEVICE_ERROR.append(str(e))
        raise


def sweep_ops(pair, variants):
    """the whole plan, op by op. variants: run every GEMM on every tile / family of its shape as well (run_variants) - the other ops
    then only advance the reference chain (test_every_op_against_fp64 checks them)"""
    ref, ctx, B, mode = pair.ref, pair.ctx, pair.B, pair.mode
    rows, launched, failures = [], [], []
    i = 0
    while i < ref.n_ops:
        gop = pair.gops[i]
        if gop["kind"] == R.OP_TAP:
            i += 1
            continue
        fused = gop["kind"] == R.OP_ISTFT and not gop["launches"]
        j = i + 1 if fused else i
        op = pair.gops[j]
        assert op["launches"]
        reads = op["reads"]
        values = [ref.A[lo:hi].copy() for lo, hi in reads]  # before the step: in-place ops overwrite them
        hterms = op["kind"] == R.OP_IGEMM and op["arith"] == 2
        # ---- the reference: fp32 interpreter (the yardstick of the RMS rule), then the precise step the chain continues from
        if fused:
            ref.step(i, True)
            ref.step(j, True, chained=True)
        else:
            ref.step(i, True, hterms=hterms)
        if variants is not None and op["kind"] != R.OP_IGEMM:
            i = j + 1
            continue
        snap = R.snapshot(ref, op)
        try:
            check_launch(pair, i, j, op, reads, values, snap, rows, launched, variants)
        except R.OpMismatch as e:  # (every op is reported, not the first only: the chain does not depend on the device's results)
            failures.append(str(e))
        i = j + 1
    return rows, launched, failures


def record(pair, rows, failures, tag=""):
    d = os.environ.get("DMX_OP_PARITY_RECORD")
    if not d:
        return
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, f"op_parity_{pair.case}_{pair.mode}{tag}.txt"), "w") as f:
        f.write("# op\tkernel\tK\tc\tworst |g - r| / (u s)\tRMS (g - r) / (u s)\tRMS of the fp32 interpreter (ops under the RMS rule)\tmedian s / |r|\n")
        for name, label, K, c, worst, rg, rf, loose in rows:
            f.write(f"{name}\t{label}\t{K}\t{c}\t{worst:.3f}\t{rg:.4f}\t{'-' if rf is None else format(rf, '.4f')}\t{loose:.3g}\n")
        for msg in failures:
            f.write(f"# MISMATCH {msg}\n")


@pytest.mark.parametrize("case,mode", [(c, m) for c, v in R.CASES.items() for m in v[3]])
def test_every_op_against_fp64(case, mode, dmxb, L, tmp_models):
    pair = Pair(dmxb, L, tmp_models, case, mode)
    try:
        pair.assert_same_plan()
        rows, _, failures = sweep(pair)
        record(pair, rows, failures)
        assert not failures, failures[:12]
        assert len(rows) > 100
    finally:
        pair.close()


def test_every_op_against_fp64_with_a_silent_segment(dmxb, L, tmp_models):
    """one of the two segments all zeros: standard deviation 0, exact zeros wherever the magnitude is 0"""
    pair = Pair(dmxb, L, tmp_models, "4s_8000", "bf16x3", zero_segment=True)
    try:
        pair.assert_same_plan()
        rows, _, failures = sweep(pair)
        record(pair, rows, failures, "_silent")
        assert not failures, failures[:12]
    finally:
        pair.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# every tile and every kernel family
UNUSED_CFGS = {1, 17, 18}  # gemm_tiles.h DMX_TILES: 1 is never chosen, 17 / 18 have no kernel (the slots keep the numbering)
FAMILIES = {1: "GF_DIRECT", 2: "GF_TILE", 3: "GF_LIN256", 4: "GF_SPLIT_STAGED", 5: "GF_SPLIT_STAGED_LIN", 6: "GF_SPLIT_LIN", 7: "GF_SPLIT_LINH",
            8: "GF_SPLIT_LINW", 9: "GF_SPLIT_WIDE_CONV", 10: "GF_SPLIT_NARROW"}
# not reachable in f32 / bf16x3 contexts: the fp16-term linear kernel exists in fp16x3 contexts only (test_every_op_against_fp64
# [4s_8000-fp16x3] launches it as the plan's own choice)
EXEMPT_FAMILIES = {7}


@pytest.fixture(scope="module")
def variant_sweeps(dmxb, L, tmp_models):
    out = {}
    for case in ("4s_8000", "6s_7000"):
        for mode in ("f32", "bf16x3"):
            pair = Pair(dmxb, L, tmp_models, case, mode)
            try:
                pair.assert_same_plan()
                variants = {"checked": 0, "refused": set()}
                rows, launched, failures = sweep(pair, variants)
                record(pair, rows, failures, "_variants")
                out[(case, mode)] = (variants, launched, failures)
            finally:
                pair.close()
    return out


def test_every_tile_and_family_meets_the_bound_and_the_sibling_claims(variant_sweeps):
    for key, (variants, _, failures) in variant_sweeps.items():
        assert not failures, (key, failures[:12])
        assert variants["checked"] > 50, (key, variants["checked"])


def test_every_tile_and_family_is_launched(variant_sweeps):
    cfgs, fams = set(), set()
    for _, launched, _ in variant_sweeps.values():
        cfgs |= {c for c, _, _ in launched if c >= 0}
        fams |= {f for _, f, _ in launched if f > 0}
    want_cfgs = (set(range(17)) | {19, 20}) - UNUSED_CFGS
    assert not want_cfgs - cfgs, f"tile cfgs never launched: {sorted(want_cfgs - cfgs)}"
    want_fams = set(FAMILIES) - EXEMPT_FAMILIES
    assert not want_fams - fams, f"kernel families never launched: {[FAMILIES[f] for f in sorted(want_fams - fams)]}"
