"""The host-only plan of the multi-track path (demucs_cpp_amd/csrc/tracks_plan.cpp) without a GPU: the stand-alone
tests/tracks_plan_harness.cpp prints the plan of a case as JSON, and every property the executor in csrc/tracks_exec.cpp relies on
is recomputed here by brute force from the geometry alone (shift, stride, segment): which segments cover which samples,
what has been dealt by which batch, which tracks are live. Nothing here restates the plan's own index arithmetic: the
position of a (track, copy, row) in a model's sequence is looked up in the sequence the plan prints.

TRACKS_PLAN_HARNESS names another build of the harness (e.g. one compiled with -fsanitize=address,undefined)."""
import itertools
import json
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SHIFT = 22050
SEG = 8000
OVERLAPS = [0.0, 0.25, 0.5, 0.9]
BQN = list(itertools.product([1, 3, 8], [1, 2, 4], [1, 2, 5]))
FIVE = [2, int(SEG * 0.4), SEG, int(SEG * 3.3), int(SEG * 7.9)]  # test_gpu_multitrack._five
SHORT = int(SEG * 1.3)
POOL = [0, 22049, 4033, 12436, 7, 6865, 5427, 21999, 1, 11025]
TRACK_SETS = {"five": FIVE, "twenty": [SHORT] * 20, "four": [SHORT] * 4}


def stride_of(overlap):
    """(int)((1 - overlap) * segment) in fp32: dmx_track_geometry_overlap's stride"""
    return int((np.float32(1) - np.float32(overlap)) * np.float32(SEG))


def n_segments(n, shift, stride):
    return -(-(n + MAX_SHIFT - shift) // stride)


def shifts_of(lengths, Q, N, stride):
    """T x Q x N shifts out of POOL (0 and 22049 among them); with N >= 2 the first two copies of every other (track,
    model) are a pair whose shifted lengths straddle a multiple of the stride: their segment counts differ by one"""
    out = []
    for t, n in enumerate(lengths):
        for q in range(Q):
            s = [POOL[(3 * t + 5 * q + k) % len(POOL)] for k in range(N)]
            if N >= 2 and (t + q) % 2 == 1:
                s[0] = (n + MAX_SHIFT - 1) % stride  # shifted length = 1 mod stride: one segment more than ...
                s[1] = s[0] + 1                      # ... a multiple of the stride
            out += s
    return out


def equal_shifts(T, n, Q, N, stride, B):
    """The same N shifts for every track and model of T equal tracks, chosen (from the geometry alone) so that the
    items of FOUR tracks are a multiple of max_batch in every model. A ring is sized from how far back the overlap-adds
    read at the END of their batch, which depends on where a track's items fall between the batch boundaries; with this
    choice the twenty-track case is the four-track case five times over, batch boundaries included, so the two can differ
    in nothing but the number of tracks. With N = 5 two of the copies are a pair whose segment counts differ by one."""
    s = [POOL[k] for k in range(N)]
    if N == 5:
        s[2] = (n + MAX_SHIFT - 1) % stride
        s[3] = s[2] + 1
    need = B // math.gcd(B, 4)
    for last in range(0, MAX_SHIFT, 499):
        s[-1] = last
        if sum(n_segments(n, x, stride) for x in s) % need == 0:
            return s * (T * Q)
    raise AssertionError("no such shifts")


def _harness():
    exe = os.environ.get("TRACKS_PLAN_HARNESS")
    if exe:
        return exe
    exe = os.path.join(ROOT, "tests", "_build", "tracks_plan_harness")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", ROOT, "plan_harness"], stdout=subprocess.DEVNULL)
    return exe


@pytest.fixture(scope="module")
def plans():
    """every case of the matrix through ONE run of the harness: {(tracks, B, Q, N, overlap): (case, plan)}"""
    cases = {}
    for name, lengths in TRACK_SETS.items():
        for (B, Q, N), ov in itertools.product(BQN, OVERLAPS):
            stride = stride_of(ov)
            shifts = shifts_of(lengths, Q, N, stride) if name == "five" else equal_shifts(len(lengths), SHORT, Q, N, stride, B)
            cases[(name, B, Q, N, ov)] = dict(seg=SEG, stride=stride, B=B, Q=Q, N=N, n=lengths, shifts=shifts)
    text = "".join(" ".join(map(str, [c["seg"], c["stride"], c["B"], c["Q"], c["N"], 1] + c["n"] + c["shifts"])) + "\n"
                   for c in cases.values())
    res = subprocess.run([_harness()], input=text, capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(cases)
    return {key: (case, json.loads(line)) for (key, case), line in zip(cases.items(), lines)}


def test_the_strides_of_the_matrix():
    assert [stride_of(o) for o in OVERLAPS] == [8000, 6000, 4000, 800]


def check_plan(case, P):
    seg, stride, B, Q, N, lengths = case["seg"], case["stride"], case["B"], case["Q"], case["N"], case["n"]
    T = len(lengths)
    assert "error" not in P, P
    assert (P["T"], P["Q"], P["N"], P["B"], P["seg"], P["stride"]) == (T, Q, N, B, seg, stride)
    shifts = np.array(case["shifts"]).reshape(T, Q, N)
    nseg = -(-(np.array(lengths)[:, None, None] + MAX_SHIFT - shifts) // stride)
    assert [c["shift"] for c in P["copies"]] == case["shifts"]
    assert [c["nseg"] for c in P["copies"]] == nseg.reshape(-1).tolist()
    assert P["nmax"] == max(lengths) and P["Mtot"] == int(nseg.sum()) and P["M"] == nseg.sum(axis=(0, 2)).tolist()

    # the sequences: every (track, copy, row) once, in (track, row, copy) order. where[q][t][k][g]: its place
    where = []
    for q in range(Q):
        its = [tuple(i) for i in P["items"][q]]
        assert its == sorted(its, key=lambda i: (i[0], i[2], i[1]))
        assert sorted(its) == [(t, k, g) for t in range(T) for k in range(N) for g in range(nseg[t, q, k])]
        w = [[np.zeros(nseg[t, q, k], np.int64) for k in range(N)] for t in range(T)]
        for i, (t, k, g) in enumerate(its):
            w[t][k][g] = i
        where.append(w)
        for t in range(T):
            x = P["tm"][t * Q + q]
            mine = [i for i, it in enumerate(its) if it[0] == t]
            assert (x["g0"], x["m"]) == (mine[0], len(mine)) and mine == list(range(mine[0], mine[0] + len(mine)))

    # batches: the model whose next item has the lowest (track, row), the lowest q on a tie; <= B items in sequence order
    pos, dealt, kFirst, kLast, total = [0] * Q, [], [None] * T, [None] * T, 0
    for k, b in enumerate(P["batches"]):
        nxt = {q: (P["items"][q][pos[q]][0], P["items"][q][pos[q]][2], q) for q in range(Q) if pos[q] < P["M"][q]}
        assert b["q"] == min(nxt.values())[2]
        q = b["q"]
        assert b["g0"] == pos[q] and b["nb"] == min(B, P["M"][q] - pos[q]) and 1 <= b["nb"] <= B
        for t, _, _ in P["items"][q][pos[q]:pos[q] + b["nb"]]:
            kFirst[t] = k if kFirst[t] is None else kFirst[t]
            kLast[t] = k
        pos[q] += b["nb"]
        total += b["nb"]
        assert P["cum"][k] == total
        dealt.append(list(pos))
    assert pos == P["M"]  # every item of every model in exactly one batch
    nB = len(P["batches"])
    assert [j["kFirst"] for j in P["jobs"]] == kFirst and [j["kLast"] for j in P["jobs"]] == kLast
    assert [j["n"] for j in P["jobs"]] == lengths

    # pieces tile [0, n) in order, one per batch of [kFirst, kLast], the last in kLast; coverage; ring safety
    R = P["R"]
    done = [0] * T
    starts = [[[np.arange(nseg[t, q, k]) * stride - (MAX_SHIFT - shifts[t, q, k]) for k in range(N)] for q in range(Q)]
              for t in range(T)]  # the first output sample of every segment
    for k, pcs in enumerate(P["pieces"]):
        assert [pc["t"] for pc in pcs] == [t for t in range(T) if kFirst[t] <= k <= kLast[t]]
        for pc in pcs:
            t, lo, hi = pc["t"], pc["lo"], pc["hi"]
            assert lo == done[t] and lo <= hi <= lengths[t]
            assert (hi == lengths[t]) == (k == kLast[t])
            done[t] = hi
            if hi == lo:
                continue
            for q in range(Q):
                g0 = P["tm"][t * Q + q]["g0"]
                read = np.concatenate([where[q][t][r][(starts[t][q][r] < hi) & (starts[t][q][r] + seg > lo)] for r in range(N)])
                assert read.size >= N  # every copy covers every sample
                assert read.max() < dealt[k][q], "a segment covering the piece is not dealt yet"
                assert read.min() - g0 == pc["itemLo"][q]
                assert read.min() + R[q] >= dealt[k][q], "an item the piece reads has been overwritten"
    assert done == lengths
    for b in P["batches"]:
        assert b["g0"] % R[b["q"]] + b["nb"] <= R[b["q"]]
    for q in range(Q):
        assert R[q] == P["M"][q] or (R[q] % B == 0 and 2 * B <= R[q] < P["M"][q])
    assert P["ringOff"] == [sum(R[:q]) for q in range(Q)] and P["ringBlocks"] == sum(R)

    # slots: held during [kFirst, kLast + 1]; taken over only from a track that finished in batch kFirst - 2 or earlier
    live = [sum(kFirst[t] <= k <= kLast[t] + 1 for t in range(T)) for k in range(nB + 1)]
    assert P["nSlots"] == max(live)
    holder = {}
    for t, j in enumerate(P["jobs"]):
        assert 0 <= j["slot"] < P["nSlots"]
        prev = holder.get(j["slot"])
        assert bool(j["takeover"]) == (prev is not None)
        if prev is not None:
            assert kLast[prev] <= kFirst[t] - 2
        holder[j["slot"]] = t
    for a, b in itertools.combinations(range(T), 2):
        if P["jobs"][a]["slot"] == P["jobs"][b]["slot"]:
            assert kLast[a] + 1 < kFirst[b] or kLast[b] + 1 < kFirst[a]

    # PCM ranges: tile [0, n), every boundary but n a multiple of 4, none past its batch's piece
    done, final = [0] * T, [0] * T
    assert len(P["pcm"]) == nB
    for k, rs in enumerate(P["pcm"]):
        for pc in P["pieces"][k]:
            final[pc["t"]] = pc["hi"]
        for t, lo, hi in rs:
            assert lo == done[t] and lo < hi <= final[t] and lo % 4 == 0 and (hi % 4 == 0 or hi == lengths[t])
            assert kFirst[t] <= k <= kLast[t]
            done[t] = hi
    assert done == lengths


@pytest.mark.parametrize("B,Q,N", BQN)
@pytest.mark.parametrize("tracks", list(TRACK_SETS))
def test_plan_invariants(plans, tracks, B, Q, N):
    for ov in OVERLAPS:
        case, P = plans[(tracks, B, Q, N, ov)]
        check_plan(case, P)


def test_the_matrix_has_copies_whose_segment_counts_differ(plans):
    for (name, B, Q, N, ov), (case, P) in plans.items():
        uneven = [x for x in P["tm"] if x["nMax"] > x["nMin"]]
        if name == "five" and N >= 2 or N == 5:
            assert uneven, (name, B, Q, N, ov)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_one_copy_at_overlap_025_needs_two_batches_of_ring(plans, B):
    for name in TRACK_SETS:
        _, P = plans[(name, B, 1, 1, 0.25)]
        assert P["R"] == [min(P["M"][0], 2 * B)]


@pytest.mark.parametrize("B,Q,N", BQN)
def test_the_ring_does_not_grow_with_the_number_of_tracks(plans, B, Q, N):
    for ov in OVERLAPS:
        _, four = plans[("four", B, Q, N, ov)]
        _, twenty = plans[("twenty", B, Q, N, ov)]
        assert twenty["ringBlocks"] == four["ringBlocks"] and twenty["R"] == four["R"], (ov, four["R"], twenty["R"])
