#!/usr/bin/env python
"""The ten attention ops of the bf16x3 segment plan with the paired kernel off (DMX_ATT_PAIR=0) and on wherever it exists (2), in ONE
process: per batch size the two plans are built and profiled in turn, ROUNDS times each (dmx_debug_profile: HIP events around REPS
launches of every op, after one plan run on a seeded mix so that the arena holds real activations). Prints the table and, with OUT set,
writes it to that file.  BATCHES=42,24,12,4,1 ROUNDS=2 REPS=5 NS=4 OUT=table.txt python tools/attention_pair_ab.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demucs_cpp_amd import binding as dmx  # noqa: E402
from demucs_cpp_amd.weights import write_synthetic_model  # noqa: E402

ns = int(os.environ.get("NS", "4"))
batches = [int(b) for b in os.environ.get("BATCHES", "42,24,12,4,1").split(",")]
rounds, reps = int(os.environ.get("ROUNDS", "2")), int(os.environ.get("REPS", "5"))
path = f"/tmp/prof_ops_{ns}s.bin"
if not os.path.exists(path):
    write_synthetic_model(path, ns, 0 if ns == 4 else 3)
m = dmx.Model(path)
out = open(os.environ["OUT"], "w") if os.environ.get("OUT") else None


def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


say(f"# attention ops of the {ns}s bf16x3 segment plan, ms per launch (best of {rounds} profiles of {reps} launches); DMX_ATT_PAIR=0 | 2")
for B in batches:
    best, forms, shape = {}, {}, {}
    for rnd in range(rounds):
        for mode in ("0", "2"):
            os.environ["DMX_ATT_PAIR"] = mode
            ctx = dmx.Context(m, 0, B, gemm=dmx.GEMM_BF16X3)
            mix = (0.1 * torch.randn((B, ctx.seg, 2), generator=torch.Generator().manual_seed(5)) + 0.02).cuda()
            res = torch.zeros((B, m.n_sources, 2, ctx.seg), device="cuda")
            ctx.segment_device(mix.data_ptr(), res.data_ptr(), B)
            ctx.synchronize()
            n_ops = ctx.plan_info(B)[0]
            info = {o["name"]: o for o in (ctx.op_info(B, i) for i in range(n_ops)) if o.get("label") == "attention_split"}
            for nm, k, ms, fl, by in ctx.profile(B, reps):
                if k == "attention_split":
                    best[(nm, mode)] = min(best.get((nm, mode), 1e9), ms)
                    forms[(nm, mode)] = info[nm]["form"]
                    shape[nm] = (info[nm]["Tq"], info[nm]["T"], info[nm]["planes"], fl)
            ctx.close()
            del mix, res
    say(f"\nbatch {B}")
    say(f"{'op':44s} {'Tq':>5s} {'Tk':>5s} pl {'form0':>6s} {'ms':>8s} {'TF/s':>6s} {'form2':>6s} {'ms':>8s} {'TF/s':>6s} {'2/0':>6s}")
    tot = {"0": 0.0, "2": 0.0}
    for nm in sorted(shape):
        tq, tk, pl, fl = shape[nm]
        a, b = best[(nm, "0")], best[(nm, "2")]
        tot["0"] += a
        tot["2"] += b
        say(f"{nm:44s} {tq:5d} {tk:5d} {pl:2d} {forms[(nm, '0')]:>6s} {a:8.4f} {fl / a / 1e9:6.1f} {forms[(nm, '2')]:>6s} {b:8.4f} {fl / b / 1e9:6.1f} {b / a:6.3f}")
    say(f"{'sum':44s} {'':5s} {'':5s}    {'':>6s} {tot['0']:8.4f} {'':6s} {'':>6s} {tot['2']:8.4f} {'':6s} {tot['2'] / tot['0']:6.3f}")
m.close()
