"""Crafted operands for the attention ops, and a numpy model of the kernels' tile algorithm that says in advance which branch every
fragment takes (tests/test_attention_crafted_cpu.py proves the design without a GPU, tests/test_gpu_attention_crafted.py runs
the HIP kernels on it).

The one value-driven branch of attention.hip / attention_split.hip is in attention_common.h att_softmax_pre: per fragment of 16
consecutive queries (aligned at 16: one MFMA column block, the unit of the ballot in every form) and per tile of 64 keys, the running
maximum is raised - and O and the row sum rescaled by alpha = exp2(m_old - m_new) - only when some query's tile maximum exceeds
its running maximum by more than 16 in the exp2 domain. On the operands a random mixture produces that happens on tile 0 only.

Operands. Head dims 0 .. nt-1 carry a score level per (query, key tile): k[s][tile(s)] = G, q[t][j] = level[t][j] / (G scale
log2 e), so key s gets level[t][tile(s)] added to its score in exp2 units. The remaining dims of q and k and all of v are
standard normal, seeded by (batch, head): inside a tile the scores keep their random spread (std about 1.4 exp2 units), every query
keeps dozens of comparable contributors and no output is a single v row. The level of (query, tile) is the designed tile MAXIMUM
minus the largest random score of that tile, so the maxima the kernel sees are the designed ones to fp32 rounding and every
decision has the margin its kind was designed with. Kinds of fragments (KINDS): see kind_levels. Where the keys are no whole
tiles, one more dim (index nt) is a level of the last valid key Tk - 1 alone: the kernels stage keys beyond Tk as copies of that
row and mask them, so a spike on it is what shows a mask that is off by one.

LocalState (Demucs v3) has no level dims: there the decay term -|key - query| g(query) drives the maximum up tile after tile
towards the diagonal. Fragments take a large slope (chosen per fragment from LOC_SLOPES as the first one whose decisions all keep
the margin), a slope near zero, or both mixed query by query.

Every level is within +-128 exp2 units and every value finite."""
import zlib

import numpy as np

KT = 64          # keys per tile
FRAG = 16        # queries per fragment
DEFER = 16.0     # attention_common.h kDeferLog2
LOG2E = 1.4426950408889634
G = 8.0          # the K side of a level dim (a bf16 number: the operand planes hold it in one term)
MARGIN = 1.0     # every decision is at least this far from the threshold, in exp2 units
OP_ATTENTION, OP_LOCAL_ATTN = 5, 12
MISTAKES = ("skip_o", "skip_l", "alpha_from_neighbour", "mask_off_by_one")
VALUE_DRIVEN = MISTAKES[:3]  # invisible unless a fragment raises its maximum after tile 0; the mask's mistake shows on any input

# model key of the tmp_models fixture, segment samples, batch, arithmetics: the smallest segments at which every path has at least 3
# key tiles or a masked tile behind full ones; tokens = segment / 128 (frequency branch) and segment / 256 (time branch)
CASES = {
    "4s_49152": (4, 49152, 1, ("f32", "bf16x3")),   # 384 / 192: planes on both branches, self- and cross-attention, the pair exists
    "4s_40960": (4, 40960, 1, ("f32", "bf16x3")),   # 320 / 160: time keys 2.5 tiles (fp32 K/V in the split kernel, masked), ragged query tiles
    "6s_24576": (6, 24576, 2, ("f32", "bf16x3")),   # 192 / 96: head dim 48, a masked tile, batch strides
    "v3_133120": (3, 133120, 1, ("f32", "bf16x3")),  # LocalState T = 130 (3 tiles, 2 keys in the masked one) and T = 65
}
TOKENS = {"4s_49152": (384, 192), "4s_40960": (320, 160), "6s_24576": (192, 96)}
LOC_T = {"v3_133120": {48: 130, 96: 65}}  # head dim -> T

KINDS = ("mixed", "accumulate", "descending", "under_over", "first_dominant", "offset_plus", "offset_minus", "masked_spike")
LOC_KINDS = ("large", "zero", "mixed")
LOC_SLOPES = tuple(0.30 + 0.04 * i for i in range(16))  # exp2 units per key: 19 .. 58 per tile


def seed_of(case, op):
    """the seed of an op's operands: by case and op name, so that two plans of one case (with and without operand planes: other op
    indices) craft the same operands"""
    return zlib.crc32((case + "/" + op["name"]).encode())


def shape_of(op, B):
    """the sizes of an attention op from its op_info words"""
    if op["kind"] == OP_LOCAL_ATTN:
        hd = op["K"]
        return dict(B=B, Tq=op["T"], Tk=op["T"], H=4, hs=hd, scale=float(np.float32(1.0) / np.sqrt(np.float32(hd))), loc=True)
    assert op["kind"] == OP_ATTENTION and op["B"] == B
    return dict(B=B, Tq=op["Tq"], Tk=op["T"], H=op["H"], hs=op["K"], scale=float(np.float32(op["scale"])), loc=False)


def loc_slope(decay):
    """decay logits [T][4] of one head -> g(query) in natural units: sum_n (n + 1) / 2 * sigmoid(d_n) / 2"""
    d = decay.astype(np.float64)
    return ((np.arange(4) + 1) / 2.0 * 0.5 / (1.0 + np.exp(-d))).sum(1)


def scores(q, k, scale, decay=None):
    """fp64 scores of one (batch, head) in the exp2 domain, one row per lane of the ballot: [Tq rounded up to 16][Tk]. Rows beyond
    Tq are what the kernels compute there: the last query again (LocalState: with the distance and the diagonal of the row's own
    index). decay: LocalState logits [T][4] of this head"""
    Tq, Tk = q.shape[0], k.shape[0]
    n = -(-Tq // FRAG) * FRAG
    rows = np.minimum(np.arange(n), Tq - 1)
    S = (q.astype(np.float64)[rows] @ k.astype(np.float64).T) * (float(np.float32(scale)) * LOG2E)
    if decay is not None:
        g = loc_slope(decay)[rows] * LOG2E
        qrow, key = np.arange(n)[:, None], np.arange(Tk)[None, :]
        S = np.where(qrow == key, -100.0 * LOG2E, S - np.abs(key - qrow) * g[:, None])
    return S


def events(S, threshold=DEFER):
    """walks the tiles as the kernel does. S: scores(). Per (fragment, tile): raised, margin (distance of the decision from the
    threshold: > 0), and per query alpha (1 where nothing is raised), tmax and the running maximum before the tile"""
    n, Tk = S.shape
    nf, nt = n // FRAG, -(-Tk // KT)
    ev = dict(raised=np.zeros((nf, nt), bool), margin=np.full((nf, nt), np.inf), alpha=np.ones((nf, nt, FRAG)),
              tmax=np.zeros((nf, nt, FRAG)), mrun=np.zeros((nf, nt, FRAG)))
    m = np.full(n, -np.inf)
    for t in range(nt):
        tm = S[:, t * KT:min(Tk, (t + 1) * KT)].max(1)
        x = (tm - (m + threshold)).reshape(nf, FRAG)
        up = (x > 0).any(1)
        if t > 0:
            ev["margin"][:, t] = np.where(up, x.max(1), -x.max(1))
        mnew = np.where(np.repeat(up, FRAG), np.maximum(m, tm), m)
        with np.errstate(invalid="ignore"):
            alpha = np.where(np.isinf(m), 0.0, np.exp2(m - mnew))
        ev["raised"][:, t], ev["alpha"][:, t], ev["tmax"][:, t], ev["mrun"][:, t] = up, alpha.reshape(nf, FRAG), tm.reshape(nf, FRAG), m.reshape(nf, FRAG)
        m = mnew
    return ev


CLASSES = ("raise_all_small", "raise_some_between", "raise_some_one", "deferred_over", "under", "raise_last", "raise_masked")


def classes(ev, Tq, Tk):
    """counts of the (fragment, tile) decisions after tile 0 by class, over the real queries of each fragment:
    raise_all_small: raised, every alpha <= 2^-16; raise_some_between: raised, some alpha strictly between 2^-16 and 1;
    raise_some_one: raised, some alpha == 1; deferred_over: not raised though some tmax > mrun; under: every tmax <= mrun;
    raise_last: raised on the last tile; raise_masked: that tile is a masked one"""
    nf, nt, _ = ev["alpha"].shape
    real = (np.arange(nf * FRAG) < Tq).reshape(nf, 1, FRAG)
    a, up = ev["alpha"], ev["raised"]
    later = np.arange(nt)[None, :] > 0
    over = ((ev["tmax"] > ev["mrun"]) & real).any(2)
    small = ((a <= 2.0 ** -16) | ~real).all(2)
    c = {
        "raise_all_small": up & small,
        "raise_some_between": up & ((a > 2.0 ** -16) & (a < 1.0) & real).any(2),
        "raise_some_one": up & ((a == 1.0) & real).any(2),
        "deferred_over": ~up & over,
        "under": ~over,
        "raise_last": up & (np.arange(nt)[None, :] == nt - 1),
    }
    c["raise_masked"] = c["raise_last"] & (Tk % KT != 0)
    return {k: int((v & later).sum()) for k, v in c.items()}


def classes_possible(shape):
    """the classes a shape can have: all of them from two tiles up; a raise in a masked tile where the keys are no whole tiles.
    LocalState, where the decay alone sets the levels: tile t is 16 over the tiles before it only for a query whose diagonal
    lies 16 / slope keys inside it, so a tile raises only if it holds at least 32 keys (LOC_SLOPES: up to 0.9 per key, and the
    margin) - T = 130 cannot raise in its last tile of 2 keys, T = 65 not at all"""
    Tk = shape["Tk"]
    nt = -(-Tk // KT)
    if nt < 2:
        return ()
    if shape["loc"]:
        room = lambda t: min(Tk, (t + 1) * KT) - t * KT >= 32
        c = ("deferred_over", "under")
        if any(room(t) for t in range(1, nt)):
            c += ("raise_all_small", "raise_some_between", "raise_some_one")
        if room(nt - 1):
            c += ("raise_last",) + (("raise_masked",) if Tk % KT else ())
        return c
    return tuple(c for c in CLASSES if c != "raise_masked" or Tk % KT)


def raises_expected(shape):
    """the least number of raises after tile 0 an op's crafted operands must take: 10 (LocalState, where a third of the fragments can
    raise at all: 5), 0 where the shape cannot raise"""
    return 0 if "raise_some_one" not in classes_possible(shape) else 5 if shape["loc"] else 10


# ---------------------------------------------------------------------------------------------------------------------------------
# the designed tile maxima of one fragment
def kind_levels(kind, nt, frag, rng, masked):
    """D [16][nt]: the designed maximum of every (query, tile) in exp2 units, and spike [16] or None: the designed score of the last
    valid key where it has a level of its own (the tile's other keys then stay at D).
      mixed           one trigger query climbs 22 per tile (a raise on every tile, its alpha 2^-22); the other 15 drift by -4 .. +6
                      per tile and ride along with alpha between 2^-6 and 1, one of them always falling (alpha exactly 1), one
                      always climbing by 5 (alpha 2^-5)
      accumulate      +10 per tile: tile 1 is deferred with P up to 2^10, tile 2 raises by 20, and so on in turns
      descending      -6 per tile: never raised after tile 0
      under_over      0, +12, +13, +13 .. deferred, then +40 on the last tile
      first_dominant  +60 on the first tile, -100 after it: every later P underflows to 0
      offset_plus / offset_minus   0, 9, 18, 10, 20, 12 (deferred, raised by 18, under, deferred, under) on a common +-100
      masked_spike    -2 per tile, the masked tile 3 under the running maximum; the last valid key alone is 40 over it for the
                      trigger query and -2 .. +5 around it for the others"""
    jit = lambda a: rng.uniform(-a, a, (FRAG, nt))
    base = rng.uniform(-3.0, 3.0, (FRAG, 1))
    j = np.arange(nt)[None, :].astype(np.float64)
    spike = None
    if kind == "mixed":
        trig = (3 + 5 * frag) % FRAG
        steps = rng.uniform(-4.0, 6.0, (FRAG, nt))
        steps[:, 0] = 0.0
        steps[(trig + 1) % FRAG, 1:] = -3.0
        steps[(trig + 2) % FRAG, 1:] = 5.0
        D = np.cumsum(steps, 1)
        D[trig] = 22.0 * j[0]
        D = D + base
    elif kind == "accumulate":
        D = 10.0 * j + jit(0.4) + base
    elif kind == "descending":
        D = -6.0 * j + jit(0.4) + base
    elif kind == "under_over":
        seq = np.array([0.0, 12.0] + [13.0] * max(nt - 2, 0))[:nt]
        if nt > 1:
            seq[-1] = 40.0
        D = seq[None, :] + jit(0.4) + base
    elif kind == "first_dominant":
        D = np.where(j == 0, 60.0, -100.0) + jit(0.4)
    elif kind in ("offset_plus", "offset_minus"):
        seq = np.array([0.0, 9.0, 18.0, 10.0, 20.0, 12.0])[np.arange(nt) % 6]
        D = seq[None, :] + jit(0.3) + (100.0 if kind == "offset_plus" else -100.0)
    elif kind == "masked_spike":
        assert masked and nt > 1
        trig = (7 + 3 * frag) % FRAG
        D = -2.0 * j + jit(0.4) + base
        D[:, -1] = D[:, 0] - 3.0
        u = rng.uniform(-2.0, 5.0, FRAG)
        u[trig], u[(trig + 1) % FRAG], u[(trig + 2) % FRAG] = 40.0, -1.0, 4.0
        spike = D[:, 0] + u
    else:
        raise ValueError(kind)
    return D, spike


def kinds_of(shape, b, h):
    """the kind of every fragment of (batch, head): the list rotates with the head, so that every kind meets every position and, where a
    (batch, head) has fewer fragments than there are kinds, the heads of an op still have all of them"""
    nt, masked = -(-shape["Tk"] // KT), shape["Tk"] % KT != 0
    pool = [k for k in KINDS if k != "masked_spike" or (masked and nt > 1)]
    nf = -(-shape["Tq"] // FRAG)
    rot = 3 * (b * shape["H"] + h)
    return [pool[(f + rot) % len(pool)] for f in range(nf)]


def craft_head(shape, seed, b, h):
    """operands of one (batch, head): q [Tq][hs], k / v [Tk][hs] fp32 and the levels written [Tq][nt (+ 1)]"""
    Tq, Tk, hs = shape["Tq"], shape["Tk"], shape["hs"]
    nt, masked = -(-Tk // KT), Tk % KT != 0
    nl = nt + (1 if masked else 0)
    rng = np.random.default_rng([seed, b, h])
    q, k, v = (rng.standard_normal((n, hs)).astype(np.float32) for n in (Tq, Tk, Tk))
    q[:, :nl], k[:, :nl] = 0.0, 0.0
    k[np.arange(Tk), np.arange(Tk) // KT] = G
    if masked:
        k[Tk - 1, nt] = G
    c = float(np.float32(shape["scale"])) * LOG2E
    rnd = (q.astype(np.float64) @ k.astype(np.float64).T) * c  # (the level dims of q are still zero: the random part alone)
    kinds = kinds_of(shape, b, h)
    levels = np.zeros((Tq, nl))
    for f, kind in enumerate(kinds):
        r0, r1 = f * FRAG, min(Tq, (f + 1) * FRAG)
        D, spike = kind_levels(kind, nt, f, rng, masked)
        for t in range(nt):
            hi = min(Tk, (t + 1) * KT) - (1 if spike is not None and t == nt - 1 else 0)
            levels[r0:r1, t] = D[:r1 - r0, t] - rnd[r0:r1, t * KT:hi].max(1)
        if spike is not None:
            levels[r0:r1, nt] = spike[:r1 - r0] - levels[r0:r1, nt - 1] - rnd[r0:r1, Tk - 1]
    q[:, :nl] = (levels / (G * c)).astype(np.float32)
    return q, k, v, levels, kinds


def craft_loc_head(shape, seed, b, h):
    """LocalState: q / k / v standard normal, decay logits [T][4] by fragment kind (LOC_KINDS)"""
    T, hs = shape["Tq"], shape["hs"]
    rng = np.random.default_rng([seed, b, h])
    q, k, v = (rng.standard_normal((T, hs)).astype(np.float32) for _ in range(3))
    decay = np.full((T, 4), -12.0, np.float32)  # slope 2.5 sigmoid(-12) = 1.5e-5 per key: no level at all
    nf = -(-T // FRAG)
    kinds = [LOC_KINDS[(f + b * shape["H"] + h) % len(LOC_KINDS)] for f in range(nf)]
    logit = lambda g2: float(np.log((g2 / (2.5 * LOG2E)) / (1.0 - g2 / (2.5 * LOG2E))))
    for f, kind in enumerate(kinds):
        r0, r1 = f * FRAG, min(T, (f + 1) * FRAG)
        if kind == "zero":
            continue
        rows = np.arange(r0, r1) if kind == "large" else np.arange(r0, r1)[(np.arange(r0, r1) % 2) == 1]
        for g2 in LOC_SLOPES:
            decay[rows] = logit(g2)
            # the fragment's lanes: its rows, and behind the last query the rows the kernel computes there
            S = scores(q, k, shape["scale"], decay)[r0:r0 + FRAG]
            if events(S)["margin"].min() >= MARGIN + 0.5:
                break
    return q, k, v, decay, kinds


def craft(shape, seed):
    """crafted operands of an op: dict q [B][Tq][H hs], k, v [B][Tk][H hs], decay [B][T][16] or None, levels (the largest |level|
    written), kinds {(b, h): [kind of every fragment]}"""
    B, H, hs = shape["B"], shape["H"], shape["hs"]
    q = np.zeros((B, shape["Tq"], H * hs), np.float32)
    k, v = (np.zeros((B, shape["Tk"], H * hs), np.float32) for _ in range(2))
    decay = np.zeros((B, shape["Tq"], 16), np.float32) if shape["loc"] else None
    top, kinds = 0.0, {}
    for b in range(B):
        for h in range(H):
            sl = slice(h * hs, (h + 1) * hs)
            if shape["loc"]:
                q[b, :, sl], k[b, :, sl], v[b, :, sl], decay[b, :, 4 * h:4 * h + 4], kinds[(b, h)] = craft_loc_head(shape, seed, b, h)
            else:
                q[b, :, sl], k[b, :, sl], v[b, :, sl], lv, kinds[(b, h)] = craft_head(shape, seed, b, h)
                top = max(top, float(np.abs(lv).max()))
    return dict(q=q, k=k, v=v, decay=decay, levels=top, kinds=kinds)


def random_fill(shape, seed):
    """a plain random fill of the same ranges: standard normal q / k / v, LocalState slopes of about 0.01 per key. No fragment
    raises its maximum after tile 0 on it"""
    rng = np.random.default_rng([seed, 77])
    B, C = shape["B"], shape["H"] * shape["hs"]
    q = rng.standard_normal((B, shape["Tq"], C)).astype(np.float32)
    k, v = (rng.standard_normal((B, shape["Tk"], C)).astype(np.float32) for _ in range(2))
    decay = (rng.standard_normal((B, shape["Tq"], 16)) - 6.0).astype(np.float32) if shape["loc"] else None
    return dict(q=q, k=k, v=v, decay=decay, levels=0.0, kinds={})


def head(x, shape, b, h):
    return x[b, :, h * shape["hs"]:(h + 1) * shape["hs"]]


def op_events(shape, x):
    """events of every (batch, head) of an op on operands x: (class counts summed, smallest margin, raises after tile 0, decisions
    after tile 0)"""
    total, margin, raises, decisions = {c: 0 for c in CLASSES}, np.inf, 0, 0
    for b in range(shape["B"]):
        for h in range(shape["H"]):
            d = x["decay"][b, :, 4 * h:4 * h + 4] if shape["loc"] else None
            ev = events(scores(head(x["q"], shape, b, h), head(x["k"], shape, b, h), shape["scale"], d))
            for c, n in classes(ev, shape["Tq"], shape["Tk"]).items():
                total[c] += n
            margin = min(margin, float(ev["margin"].min()))
            raises += int(ev["raised"][:, 1:].sum())
            decisions += ev["raised"][:, 1:].size
    return total, margin, raises, decisions


# ---------------------------------------------------------------------------------------------------------------------------------
# the deferred algorithm in numpy fp32
def tile_model_head(q, k, v, scale, decay=None, mistake=None, threshold=DEFER):
    """one (batch, head): q [Tq][hs], k / v [Tk][hs] -> [Tq][hs] fp32, tile by tile with the deferred maximum per fragment.
    mistake: skip_o (O not rescaled), skip_l (the row sum not rescaled), alpha_from_neighbour (alpha of query t ^ 1),
    mask_off_by_one (the masked tile lets key Tk through: the staged copy of row Tk - 1). threshold 0 (the running maximum raised
    whenever a score exceeds it) is no mistake: other bits, same values"""
    f32 = np.float32
    Tq, Tk, hs = q.shape[0], k.shape[0], q.shape[1]
    n, nt = -(-Tq // FRAG) * FRAG, -(-Tk // KT)
    rows = np.minimum(np.arange(n), Tq - 1)
    qs = (q[rows] * f32(f32(scale) * f32(LOG2E))).astype(f32)
    if mistake == "mask_off_by_one" and Tk % KT:
        k, v, Tk = np.concatenate([k, k[-1:]]), np.concatenate([v, v[-1:]]), Tk + 1
    g = (loc_slope(decay)[rows] * LOG2E).astype(f32) if decay is not None else None
    m, l, o = np.full(n, -np.inf, f32), np.zeros(n, f32), np.zeros((n, hs), f32)
    for t in range(nt):
        ks, vs = k[t * KT:min(Tk, (t + 1) * KT)], v[t * KT:min(Tk, (t + 1) * KT)]
        s = (qs @ ks.T).astype(f32)
        if g is not None:
            key, qrow = (t * KT + np.arange(ks.shape[0]))[None, :], np.arange(n)[:, None]
            s = np.where(key == qrow, f32(-100.0 * LOG2E), s - np.abs(key - qrow).astype(f32) * g[:, None]).astype(f32)
        tm = s.max(1)
        up = np.repeat((tm > m + f32(threshold)).reshape(-1, FRAG).any(1), FRAG)
        mnew = np.where(up, np.maximum(m, tm), m).astype(f32)
        with np.errstate(invalid="ignore"):
            alpha = np.where(np.isinf(m), f32(0), np.exp2(m - mnew)).astype(f32)
        if mistake == "alpha_from_neighbour":
            alpha = alpha[np.arange(n) ^ 1]
        if mistake != "skip_l":
            l = l * alpha
        if mistake != "skip_o":
            o = o * alpha[:, None]
        m = mnew
        p = np.exp2(s - m[:, None]).astype(f32)
        l = (l + p.sum(1, dtype=f32)).astype(f32)
        o = (o + p @ vs).astype(f32)
    return (o / l[:, None]).astype(f32)[:Tq]


def tile_model(shape, x, mistake=None, threshold=DEFER):
    """the op's output [B][Tq][H hs] on operands x (craft / random_fill)"""
    out = np.zeros((shape["B"], shape["Tq"], shape["H"] * shape["hs"]), np.float32)
    for b in range(shape["B"]):
        for h in range(shape["H"]):
            d = x["decay"][b, :, 4 * h:4 * h + 4] if shape["loc"] else None
            out[b, :, h * shape["hs"]:(h + 1) * shape["hs"]] = tile_model_head(head(x["q"], shape, b, h), head(x["k"], shape, b, h),
                                                                               head(x["v"], shape, b, h), shape["scale"], d, mistake, threshold)
    return out


def softmax_fp64(shape, x):
    """independent fp64 softmax(Q K^T scale) V of the op, LocalState with its decay and the -100 diagonal"""
    out = np.zeros((shape["B"], shape["Tq"], shape["H"] * shape["hs"]))
    for b in range(shape["B"]):
        for h in range(shape["H"]):
            q, k, v = (head(x[n], shape, b, h).astype(np.float64) for n in ("q", "k", "v"))
            if shape["loc"]:
                s = q @ k.T / float(np.sqrt(np.float32(shape["hs"])))
                T = shape["Tq"]
                dist = np.abs(np.arange(T)[None, :] - np.arange(T)[:, None])
                s = s - dist * loc_slope(x["decay"][b, :, 4 * h:4 * h + 4])[:, None]
                s[np.arange(T), np.arange(T)] = -100.0
            else:
                s = (q @ k.T) * float(np.float32(shape["scale"]))
            p = np.exp(s - s.max(1, keepdims=True))
            out[b, :, h * shape["hs"]:(h + 1) * shape["hs"]] = (p / p.sum(1, keepdims=True)) @ v
    return out
