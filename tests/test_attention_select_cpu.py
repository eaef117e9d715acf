"""The form rule of the exact-split attention kernel (demucs_cpp_amd/csrc/attention_select.h: wg64 / wg128 / pair, decided once per
plan on the host) through a stand-alone harness over the plans a context builds (tests/attention_select_harness.cpp). No GPU: that
every form computes the same bits is what tests/test_gpu_attention_pair.py checks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_build", "attention_select_harness")

F32, BF16X3, FP16X3 = 0, 1, 2
SEGS = {4: (6000, 10000, 343980), 6: (6000, 343980), 3: (6000, 20000, 343980)}  # the grid of tests/test_gemm_select_cpu.py
BATCHES = (1, 2, 6, 8, 42)


@pytest.fixture(scope="module")
def harness():
    srcs = [os.path.join(ROOT, "tests", "attention_select_harness.cpp")] + [
        os.path.join(ROOT, "demucs_cpp_amd", "csrc", f) for f in ("attention_select.h", "plan.cpp", "plan.h", "model_pack.cpp", "gemm_select.cpp", "gemm_select.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(EXE) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["make", "-C", ROOT, "att_harness"], stdout=subprocess.DEVNULL)

    def run(*args):
        return subprocess.run([EXE] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
    return run


def big_shape_before(Tq, H, B):
    """att_use_big_shape as it stood before the rule moved to attention_select.h (attention_common.h), restated"""
    wg128, wg64 = (Tq + 127) // 128 * H * B, (Tq + 63) // 64 * H * B
    return wg128 >= 1024 and float((wg128 + 511) // 512) <= 0.6 * float((wg64 + 511) // 512)


def plans(run, model, ns):
    rows = []
    args = [f"{seg}:{b}:{g}" for seg in SEGS[ns] for b in BATCHES for g in (F32, BF16X3, FP16X3)]
    for ln in run("plans", model, *args).splitlines():
        seg, b, g, name, tq, tk, h, hs, planes, f0, f1, f2 = ln.split()
        rows.append(dict(seg=int(seg), B=int(b), gemm=int(g), name=name, Tq=int(tq), Tk=int(tk), H=int(h), hs=int(hs), planes=int(planes),
                         forms=(f0, f1, f2)))
    return rows


def test_both_halves_pass_the_same_number_of_barriers(harness):
    lines = [tuple(int(x) for x in ln.split()) for ln in harness("barriers", 64).splitlines()]
    assert [l[0] for l in lines] == list(range(1, 65))
    for nt, a, b in lines:
        assert a == b == 3 + 2 * nt, (nt, a, b)  # stagger / closing barrier, two in the prologue, two per key tile


@pytest.mark.parametrize("ns", [4, 6])
def test_switched_off_the_rule_is_the_shape_rule_it_replaced(ns, harness, tmp_models):
    rows = plans(harness, tmp_models[ns], ns)
    assert len(rows) == 10 * len(SEGS[ns]) * len(BATCHES) * 3
    seen = set()
    for r in rows:
        want = "wg128" if big_shape_before(r["Tq"], r["H"], r["B"]) else "wg64"
        assert r["forms"][0] == want, r
        seen.add(want)
        # by rule: the paired form only where the 128-query shape stood, and only for ops that read operand planes
        assert r["forms"][1] in (want, "pair"), r
        if r["forms"][1] == "pair":
            assert want == "wg128" and r["planes"], r
    assert seen == {"wg64", "wg128"}  # (the grid reaches both shapes: 42 full segments take the big one)


@pytest.mark.parametrize("ns", [4, 6, 3])
def test_pair_never_without_planes_other_head_dims_f32_or_v3(ns, harness, tmp_models):
    rows = plans(harness, tmp_models[ns], ns)
    if ns == 3:
        assert not rows  # Demucs v3 has no transformer: LocalState attention is another op kind and never takes this kernel
        return
    assert {r["hs"] for r in rows} == {64 if ns == 4 else 48}
    for r in rows:
        if r["gemm"] == F32:
            assert not r["planes"], r  # f32 contexts write no operand planes
        eligible = r["planes"] and r["Tk"] % 64 == 0
        assert (r["forms"][2] == "pair") == bool(eligible), r  # "2": wherever the kernel exists, at any size
        if not r["planes"]:
            assert "pair" not in r["forms"], r
    assert any(r["forms"][2] == "pair" for r in rows) and any(r["gemm"] != F32 and not r["planes"] for r in rows)
    # hand-made shapes: the full-size frequency-branch op at 42 segments in every switch position ...
    for mode in (0, 1, 2):
        for hs, planes in ((32, 1), (96, 1), (128, 1), (64, 0), (48, 0)):
            assert harness("form", 2688, 2688, 8, 42, hs, planes, mode).strip() == "wg128", (mode, hs, planes)
        assert harness("form", 2688, 2700, 8, 42, 64, 1, mode).strip() == "wg128"  # a ragged key tile: no planes form
    assert harness("form", 2688, 2688, 8, 42, 64, 1, 2).strip() == "pair"
    assert harness("form", 2688, 2688, 8, 42, 64, 1, 0).strip() == "wg128"
    assert harness("form", 64, 64, 8, 1, 48, 1, 2).strip() == "pair" and harness("form", 64, 64, 8, 1, 48, 1, 1).strip() == "wg64"
