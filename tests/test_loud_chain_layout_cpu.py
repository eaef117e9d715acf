"""The workspace layout of the loudness / limiter output chain (csrc/loud_chain.h), printed by a
stand-alone CPU program (tests/loud_chain_harness.cpp) in its plain form and under AddressSanitizer and UBSan.

One rule lays out the stage alone (the reports are the caller's buffers) and a track slot (the reports live in the workspace).
What is held here: the regions are disjoint, aligned as the kernels need and inside the total; the stage's totals EQUAL what
include/demucs_hip.h documents - a caller allocates from those formulas; a slot's total never exceeds what a slot took before
the rule was written."""
import itertools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the limiter's tile is 2048 frames; 2^36 - 1 is the longest signal the entry points take: the arithmetic is 64-bit
LENGTHS = (1, 2, 3, 4, 5, 2047, 2048, 2049, 65 * 2048 + 5, 2 ** 36 - 1)
REPORT, METERS, LIMIT_KEPT, LIMIT_RESULT = 16, 16, 64, 24  # sizeof the three result structs; bytes kept per limiter result


@pytest.fixture(scope="module")
def exes():
    subprocess.check_call(["make", "-C", ROOT, "chain_harness", "chain_harness_asan"], stdout=subprocess.DEVNULL)
    return {k: os.path.join(ROOT, "tests", "_build", v) for k, v in (("plain", "loud_chain_harness"), ("asan", "loud_chain_harness_asan"))}


def _run(exe):
    r = subprocess.run([exe] + [str(n) for n in LENGTHS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(line) for line in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def cases(exes):
    return _run(exes["plain"])


def test_every_case_is_printed(cases):
    want = set()
    for n, n_out, meters, by_tp, limited, inside in itertools.product(LENGTHS, range(1, 9), (0, 1), (0, 1), (0, 1), (0, 1)):
        for envs in {1, n_out}:
            want.add((n, n_out, meters, by_tp, limited, envs, inside))
    got = [(c["n"], c["n_out"], c["meters"], c["by_tp"], c["limited"], c["envs"], c["inside"]) for c in cases]
    assert len(got) == len(set(got)) and set(got) == want


def test_the_sanitizer_form_prints_the_same(exes, cases):
    assert _run(exes["asan"]) == cases


def _regions(c):
    """(name, offset, bytes, alignment) of every region the case has"""
    k = c["n_out"]
    out = [("slots", 0, (k + 1) * c["slot_bytes"], 16), ("gains", c["gains"], 4 * k, 4)]
    if c["tp_words"]:
        out.append(("true_peaks", c["true_peaks"], 4 * c["tp_words"], 4))
    if c["inside"]:
        out.append(("report", c["report"], REPORT * (k + 1), 8))
        if c["meters"]:
            out.append(("meters_out", c["meters_out"], METERS * (k + 1), 4))
    if c["limited"]:
        out.append(("lim", c["lim"], c["envs"] * c["env_bytes"], 64))
        out.append(("lim_res", c["lim_res"], LIMIT_RESULT * k, 8))
    return out


def test_regions_are_disjoint_aligned_and_inside_the_total(cases):
    for c in cases:
        regs = _regions(c)
        for name, off, size, align in regs:
            assert off >= 0 and off % align == 0 and off + size <= c["total"], (name, c)
        for (na, a, sa, _), (nb, b, sb, _) in itertools.combinations(regs, 2):
            assert a + sa <= b or b + sb <= a, (na, nb, c)
        assert c["slot_bytes"] == c["W"] and c["slot_bytes"] % 16 == 0
        if c["limited"]:  # envelope e at lim + e * env_bytes, 16-byte aligned; the results keep 64 bytes each
            assert c["env_bytes"] == c["Lw"] and c["env_bytes"] % 16 == 0
            assert c["lim_res"] + LIMIT_KEPT * c["n_out"] == c["total"]
        else:
            assert (c["lim"], c["lim_res"]) == (-1, -1)
        if not c["inside"]:
            assert (c["report"], c["meters_out"]) == (-1, -1)
        elif not c["meters"]:
            assert c["meters_out"] == -1


def test_the_true_peaks_are_those_the_chain_measures(cases):
    """outputs when (true-peak ceiling and no limiter) or meters; the mixture's with meters alone"""
    for c in cases:
        k = c["n_out"]
        want = k + 1 if c["meters"] else k if c["by_tp"] and not c["limited"] else 0
        assert c["tp_words"] == want, c
        assert (c["true_peaks"] == -1) == (want == 0), c


def test_the_stage_totals_are_the_documented_ones(cases):
    """include/demucs_hip.h: dmx_loud_encode_device (n_out + 1) W + 64; dmx_loud_encode_meters_device (n_out + 1) (W + Mw) + 64;
    dmx_loud_encode_limit_device that figure rounded up to 64, plus n_out (Lw + 64); the stage takes n_out envelopes"""
    seen = 0
    for c in cases:
        if c["inside"] or c["envs"] != c["n_out"]:
            continue
        k, W, Mw, Lw = c["n_out"], c["W"], c["Mw"], c["Lw"]
        plain = (k + 1) * (W + (Mw if c["meters"] else 0)) + 64
        want = (plain + 63) // 64 * 64 + k * (Lw + 64) if c["limited"] else plain
        assert c["total"] == want, c
        seen += 1
    assert seen == len(LENGTHS) * 8 * 8


def _slot_bytes_before(c):
    """PcmOut::loudBytes of the commit before this layout: behind the n_out + 1 slots 64 bytes of gains and the report; with
    true peaks 64 bytes of them and a meters report; the limiter's part at a multiple of 64 behind the meters' (if any)"""
    k, W, Lw = c["n_out"], c["W"], c["Lw"]
    tp_offset = (k + 1) * W + 64 + REPORT * (k + 1)
    if c["limited"]:
        lim_offset = (tp_offset + (64 + METERS * (k + 1) if c["meters"] else 0) + 63) // 64 * 64
        return lim_offset + c["envs"] * Lw + 64 * k
    true_peaks = c["by_tp"] or c["meters"]
    return tp_offset + (64 + METERS * (k + 1) if true_peaks else 0)


def test_a_slot_takes_no_more_than_before(cases):
    seen = 0
    for c in cases:
        if c["inside"]:
            assert c["total"] <= _slot_bytes_before(c), c
            seen += 1
    assert seen * 2 == len(cases)


def test_the_workspace_sizes_are_the_three_formulas(cases):
    """W, Mw and Lw as the plan headers define them (loudness_plan.h, meters_plan.h, limiter_plan.h)"""
    for c in cases:
        n = c["n"]
        assert c["W"] == 64 + (n + 4095) // 4096 * (64 + 16 * 12) + 16 * (n // 400)
        assert c["Mw"] == 64
        assert c["Lw"] == 8 * ((n + 3) // 4 * 4) + 64 * ((n + 2047) // 2048)
