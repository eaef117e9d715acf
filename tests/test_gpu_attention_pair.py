"""The paired form of the exact-split attention kernel (attention_split.hip attention_split_pair_kernel: two 128-query halves in one
512-thread workgroup, one phase apart) against the unpaired forms of the same context. Every form runs the same arithmetic in the
same order, so nothing may differ in a single bit: the plans' whole arenas after one run from the same canary (which also catches a
store outside an op's rows), the stems, and repeated runs beside another context's work on the same GPU.

DMX_ATT_PAIR is read when a plan is built (exec.cpp dmx_get_plan): 2 = the paired kernel wherever it exists, 0 = never."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0BEEF  # a quiet NaN: a row that a kernel fails to write shows in the stems as well
# (model, segment samples, batch): freq / time tokens
CASES = {
    "4s_16384_b1": (4, 16384, 1),  # 128 / 64: a workgroup whose second half has no tile, a half-filled tile, nt = 2 and 1
    "4s_49152_b1": (4, 49152, 1),  # 384 / 192: planes on both branches, odd tile counts per XCD, a ragged last tile, nt = 6 and 3
    "4s_40960_b3": (4, 40960, 3),  # 320 / 160: nt = 5; the time branch's keys are no whole tiles: paired and fp32-K/V ops in one plan
    "6s_16384_b2": (6, 16384, 2),  # head dim 48 and its zeroed padding slots
}
DEVICE_ERROR = []  # the first failed launch: nothing more is launched after it


class Run:
    """One bf16x3 context whose plan of batch B was built under DMX_ATT_PAIR = pair (None: unset), with device buffers of its own"""

    def __init__(self, dmxb, model, seg, B, pair, monkeypatch, mixes):
        import torch
        self.torch, self.B = torch, B
        if pair is None:
            monkeypatch.delenv("DMX_ATT_PAIR", raising=False)
        else:
            monkeypatch.setenv("DMX_ATT_PAIR", pair)
        self.ctx = dmxb.Context(model, seg, B, gemm=dmxb.GEMM_BF16X3)
        self.n_ops, self.floats, _, _ = self.ctx.plan_info(B)  # (builds the plan: the switch is read here)
        self.ops = [self.ctx.op_info(B, i) for i in range(self.n_ops)]
        self.d_mix = torch.from_numpy(np.ascontiguousarray(mixes.transpose(0, 2, 1))).cuda()
        self.d_out = torch.zeros((B, model.n_sources, 2, seg), device="cuda")
        torch.cuda.synchronize()

    def run(self):
        assert not DEVICE_ERROR, f"an earlier launch failed on the device, nothing more is launched: {DEVICE_ERROR[0]}"
        try:
            self.ctx.segment_device(self.d_mix.data_ptr(), self.d_out.data_ptr(), self.B)
            self.ctx.synchronize()
            return self.d_out.cpu().numpy()
        except Exception as e:  # a HIP error: the device state is unknown from here on
            DEVICE_ERROR.append(repr(e))
            raise

    def arena(self):
        return self.ctx.arena_read(0, self.floats).view(np.uint32)

    def attention(self):
        return [o for o in self.ops if o.get("label") == "attention_split"]


@pytest.mark.parametrize("case", list(CASES))
def test_paired_attention_equals_the_unpaired_forms_bitwise(case, tmp_models, monkeypatch):
    from demucs_cpp_amd import binding as dmxb

    assert not DEVICE_ERROR, f"an earlier launch failed on the device, nothing more is launched: {DEVICE_ERROR[0]}"
    ns, seg, B = CASES[case]
    mixes = (0.1 * np.random.default_rng(seg + B).standard_normal((B, 2, seg))).astype(np.float32)
    model = dmxb.Model(tmp_models[ns], 0)
    pair = Run(dmxb, model, seg, B, "2", monkeypatch, mixes)
    plain = Run(dmxb, model, seg, B, "0", monkeypatch, mixes)
    other = Run(dmxb, model, seg, B, None, monkeypatch, mixes)  # the default plan, for the concurrent runs below

    # the form is the plan's: paired exactly where the op reads operand planes, nowhere when switched off
    att = pair.attention()
    assert len(att) == len(plain.attention()) == 10 and len(pair.ops) == len(plain.ops)
    assert all((o["form"] == "pair") == bool(o["planes"]) for o in att), [(o["name"], o["form"], o["planes"]) for o in att]
    assert any(o["form"] == "pair" for o in att)
    assert all(o["form"] in ("wg64", "wg128") for o in plain.attention())
    assert {o["K"] for o in att} == {48 if ns == 6 else 64}
    if case == "4s_40960_b3":
        assert any(not o["planes"] for o in att)
    if case == "4s_49152_b1":
        assert all(o["planes"] for o in att) and {o["T"] // 64 for o in att} == {6, 3}

    # one run each from the same canary: the whole arenas word for word, and the stems
    for r in (pair, plain):
        r.ctx.arena_fill(B, CANARY)
    out_pair, out_plain = pair.run(), plain.run()
    a, b = pair.arena(), plain.arena()
    diff = np.flatnonzero(a != b)
    assert diff.size == 0, f"{diff.size} arena words differ, first at float {diff[0]}"
    assert np.isfinite(out_plain).all()
    assert np.array_equal(out_pair.view(np.uint32), out_plain.view(np.uint32))

    # six more runs beside another context of the GPU that runs the default plan from another host thread
    stop, err = threading.Event(), []

    def neighbour():
        try:
            while not stop.is_set() and not DEVICE_ERROR:
                other.run()
        except Exception as e:
            err.append(repr(e))

    th = threading.Thread(target=neighbour)
    th.start()
    try:
        bad = [k for k in range(6) if not np.array_equal(pair.run().view(np.uint32), out_plain.view(np.uint32))]
    finally:
        stop.set()
        th.join()
    assert not err, err
    assert not bad, f"runs {bad} of 6 differ beside a concurrent context"
    for r in (pair, plain, other):
        r.ctx.close()
    model.close()
