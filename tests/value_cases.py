"""Crafted operands for the kernels with value-dependent code outside attention: the GELU and GLU epilogues and prologues of the
GEMMs, the fp16-term row scale, LayerNorm, the GroupNorm statistics and their application, the statistics reduction, the
row-resident DConv and the LSTM (tests/test_value_cases_cpu.py proves the design without a GPU, tests/test_gpu_value_cases.py
runs the HIP kernels on it; tests/attention_cases.py is the same for the attention kernels).

The operands of the op-by-op sweep (tests/test_gpu_op_parity.py) are what a 0.1 randn mixture produces through synthetic
weights: no GELU argument beyond the clamp of dmx_erff, no saturated gate, no row with a mean far from zero, no constant row.
Here every op is taken alone (the chain is not stepped): its operands are written where it reads them, by role
(cpu_interp.cpp interp_operands), and the census of the reference's precise step (interp_census) says which value classes the
launch evaluated. Every crafted value is finite.

Families (family_of) and their operands:
  gemm_plain   GEMMs without a prologue whose epilogue has GELU or GLU. At most ONE non-zero reaches each output's sum: the
               non-zeros sit on a lattice wider than the kernel's footprint (one per row for a linear layer), each a power of
               two 2^e with alternating sign, e dealt from a grid that spans 2^-20 .. past the sigmoid's overflow point relative
               to the op's median |w|. The pre-activation is then fl(2^e w + b) exactly in every arithmetic and family, and the
               bound is taken with K_eff = 1: it judges the function, not a K-term sum. Every other lattice point of a GELU op is
               no power of two: it is (t - b) / w for one column, t within 2^-11 of the seam |z| = 0.92 of dmx_erff on either
               side (a product of one fp32 number and an fp16-number weight: exact in the fp32 kernels, five partial products in
               the split ones - the 6 K_eff of the bound).
  gemm_pro     GEMMs with a prologue: dense standard normal rows under per-row power-of-two gains around crafted statistics
               records (rstd in {2^-10, 1, 1 / sqrt eps}, |mean| in {0, 8, 512} sigma); the op's own K.
  gemm_hterms  linear layers on fp16 terms under a per-row scale (fp16x3 contexts): zero rows, rows whose only non-zero is
               2^-130 (a denormal), 2^-120, 1 or 2^100 (K_eff = 1), and in a second round rows of two non-zeros 2^20 apart (K_eff = 2).
  layernorm, group_stats, stats_reduce
               rows, groups or partials built in fp64 and rounded once: sigma in {2^-20, 1, 2^12} x |mean| / sigma in {0, 8, 512},
               constant (sigma = 0, a large mean), zero, one spike among zeros; the partials of a constant group are chosen so
               that q - n mean^2 is negative by more than any summation order can change (the clamp).
  gn_act       dense elements under per-element gains around crafted records, both modes.
  dconv_row    the row tensor under per-(segment, bin) gains and offsets, zero rows, constant rows and rows with one spike.
  lstm         xproj crafted per hidden unit (index mod 8) against the recurrent term W_hh h of an fp64 walk of the recurrence:
               forget gate open with the input gate open on the first step only (memory from step 0 to T), forget gate closed,
               input and cell gates saturated (|c| grows by 1 a step), all four pre-activations below 2^-12, output gate
               closed, signs alternating in t, two smooth units.
An op with fewer records than kinds takes several ROUNDS (rounds_of): the kinds are dealt round-robin over records and rounds."""
import zlib

import numpy as np

import op_reference as R

# model key of the tmp_models fixture, segment samples, batch, arithmetics. v3_66560 is used for its eight LSTM ops only (T = 65 at
# H = 192, T = 33 at H = 384: the exchange buffers are reused 32 / 16 times); its arena is 28,415,936 floats
CASES = {
    "4s_8000": R.CASES["4s_8000"],
    "6s_7000": R.CASES["6s_7000"],
    "v3_7000": R.CASES["v3_7000"],
    "v3_66560": (3, 66560, 1, ("bf16x3",)),
}
LSTM_ONLY = ("v3_66560",)
EPS = 1e-5
SEAM = 0.92 * np.sqrt(2.0)  # |v| at which dmx_erff changes range

FAMILIES = ("gemm_plain", "gemm_pro", "gemm_hterms", "layernorm", "group_stats", "stats_reduce", "gn_act", "dconv_row", "lstm")
STAT_KINDS = [(s, r) for s in (2.0 ** -20, 1.0, 2.0 ** 12) for r in (0.0, 8.0, 512.0)] + ["constant", "zero", "spike"]
RECORDS = [(rstd, m) for rstd in (2.0 ** -10, 1.0, 1.0 / np.sqrt(EPS)) for m in (0.0, 8.0, 512.0)]  # (rstd, |mean| / sigma)


def family_of(op):
    k = op["kind"]
    if k == R.OP_IGEMM:
        if op["pro"] != 0:
            return "gemm_pro"
        if op["arith"] == 2:
            return "gemm_hterms"
        if op["act"] == 1 or op["epi"] in (R.EPI_GLU, R.EPI_GN_GLU_SCALE_RES):
            return "gemm_plain"
        return None
    return {R.OP_LAYERNORM: "layernorm", R.OP_GROUP_STATS: "group_stats", R.OP_STATS_REDUCE: "stats_reduce", R.OP_GN_ACT: "gn_act",
            R.OP_DCONV_ROW: "dconv_row", R.OP_LSTM: "lstm"}.get(k)


def instance_of(ref, i):
    """the kernel instance op i launches, or None for an op of no family: GEMMs by (label, cfg, family, pro, epi, act), the LSTM by
    H, gn_act by mode, the statistics reduction by which of its three kernels the group count selects, the row DConv by C"""
    op = ref.ops[i]
    fam = family_of(op)
    if fam is None:
        return None
    if op["kind"] == R.OP_IGEMM:
        return (fam, op["label"], op["cfg"], op["family"], op["pro"], op["epi"], op["act"])
    if fam == "lstm":
        return (fam, op["K"])
    if fam == "gn_act":
        return (fam, op["mode"])
    if fam == "stats_reduce":
        G = ref.operands(i)["reduce"][0]
        return (fam, "G>=32" if G >= 32 else "G>1" if G > 1 else "G=1")
    if fam == "dconv_row":
        return (fam, op["K"])
    return (fam,)


def select(ref, case):
    """instance -> index of the first op of the plan that launches it (LSTM_ONLY cases: the LSTM instances alone)"""
    out = {}
    for i in range(ref.n_ops):
        inst = instance_of(ref, i)
        if inst is not None and (case not in LSTM_ONLY or inst[0] == "lstm"):
            out.setdefault(inst, i)
    return out


def seed_of(case, op, rnd=0):
    return zlib.crc32(f"{case}/{op['name']}/{rnd}".encode())


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def fill_reads(ref, op, rng, scale=0.1):
    """every range the op reads outside the plan's constants: a smooth fill (residuals, whatever no role crafts)"""
    for lo, hi in op["reads"]:
        lo = max(lo, ref.consts)
        if hi > lo:
            ref.A[lo:hi] = f32(scale * rng.standard_normal(hi - lo))


def weights_of(ref, op):
    """(W [N][K], bias [N]) of a GEMM"""
    W = ref.W[op["w_w"]:op["w_w"] + op["N"] * op["Kp"]].reshape(op["N"], op["Kp"])[:, :op["K"]]
    return W, ref.W[op["bias_w"]:op["bias_w"] + op["N"]]


def rounds_of(ref, i, fam):
    """launches of op i on crafted operands: enough for every kind of record to be dealt once"""
    geo = ref.operands(i)
    if fam == "group_stats":
        op = ref.ops[i]
        records = (op["writes"][0][1] - op["writes"][0][0]) // 4
        return -(-len(STAT_KINDS) // records)
    if fam == "stats_reduce":
        return -(-(len(STAT_KINDS)) // (geo["rowstat"]["nb"] * geo["reduce"][0]))
    if fam == "gn_act":
        return -(-len(RECORDS) // geo["epistats"]["rows"])
    if fam == "gemm_pro":
        return -(-len(RECORDS) // geo["prostats"]["rows"])
    if fam == "gemm_plain":  # an op of a few rows holds a few non-zeros: rounds until the grid of exponents has been dealt twice
        grid, points = gemm_plain_grid(ref, i, ref.ops[i])
        return min(4, -(-2 * len(grid) // max(points // 2, 1)))
    if fam == "gemm_hterms":
        return 2
    return 1


def standard(rng, shape):
    """standard normal along the last axes of each leading index, then centred and scaled in fp64 to mean 0 and unbiased variance 1 exactly"""
    z = rng.standard_normal(shape)
    flat = z.reshape(shape[0], -1)
    flat -= flat.mean(1, keepdims=True)
    flat /= flat.std(1, ddof=1, keepdims=True)
    return z


def stat_block(kind, rng, n, j):
    """n elements of statistics kind `kind` (STAT_KINDS) in fp64; j varies the constants"""
    if kind == "zero":
        return np.zeros(n)
    if kind == "constant":
        return np.full(n, float(np.float32(977.123 + 0.37 * (j % 50))))
    if kind == "spike":
        x = np.zeros(n)
        x[(j * 7919) % n] = 3.7 * (-1) ** j
        return x
    sigma, ratio = kind
    return sigma * (ratio * (-1) ** j + standard(rng, (1, n))[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# GEMMs
def lattice(conv):
    """(in1, e) of the non-zeros: input rows span1 apart (no two taps of one output can meet two of them) and, inside a row of
    L0 Cin elements, exactly seg0 apart from an offset that varies with the row - every window of seg0 elements holds one"""
    L1, L0, Cin, S1, stride1, dil1, pad1, seg0 = conv[:8]
    span1 = (S1 - 1) * dil1 + 1
    pts = []
    for in1 in range(min(span1 // 2, L1 - 1), L1, span1):
        for e in range((in1 * 7919 + 13) % seg0, L0 * Cin, seg0):
            pts.append((in1, e))
    return pts


def an_output_of(conv, in1, e):
    """one output (p1, p0) that gathers input element (in1, e), and at which k; None if there is none"""
    L1, L0, Cin, S1, stride1, dil1, pad1, seg0, stride0, pad0, P1, P0 = conv[:12]
    for s1 in range(S1):
        t = in1 + pad1 - s1 * dil1
        if t % stride1 or not 0 <= t // stride1 < P1:
            continue
        for p0 in range(P0):
            o = e - (p0 * stride0 - pad0) * Cin
            if 0 <= o < seg0:
                return t // stride1, p0, s1 * seg0 + o
    return None


GELU_TARGETS = (2.0 ** -20, 2.0 ** -12, 2.0 ** -6, 0.25, 0.7, 1.0, 1.6, 2.5, 4.0, 6.0, 8.0, 12.0, 24.0, 48.0)
GLU_TARGETS = (2.0 ** -20, 2.0 ** -8, 0.25, 0.5, 2.0, 4.0, 8.0, 12.0, 24.0, 40.0, 64.0, 100.0, 160.0, 256.0, 400.0)


def gemm_plain_grid(ref, i, op):
    """(exponents of the powers of two, lattice points of the whole operand)"""
    geo = ref.operands(i)
    W, _ = weights_of(ref, op)
    wmed = float(np.median(np.abs(W[W != 0])))
    grid = [int(np.round(np.log2(t / wmed))) for t in (GELU_TARGETS if op["act"] == 1 else GLU_TARGETS)]
    return grid, geo["act"]["nb"] * len(lattice(geo["conv"]))


def craft_gemm_plain(ref, i, op, rng, rnd):
    geo = ref.operands(i)
    conv, act = geo["conv"], geo["act"]
    L1, L0, Cin = conv[:3]
    W, bias = weights_of(ref, op)
    gelu = op["act"] == 1
    grid, points = gemm_plain_grid(ref, i, op)
    X = np.zeros((act["nb"], L1, L0 * Cin), np.float32)
    q = seam = 0
    pw = 11 * rnd  # a later round starts elsewhere in the grid, with the other signs: 11 is coprime to both grid lengths (14, 15)
    for b in range(act["nb"]):
        for in1, e in lattice(conv):
            a = None
            if gelu and q % 2 == 1:  # every other point of a GELU op aims one column at the seam of dmx_erff
                hit = an_output_of(conv, in1, e)
                if hit is not None:
                    n = (q // 2 + rnd) % op["N"]
                    t = (-1.0) ** (q // 4) * SEAM * (1.0 + (-1.0) ** (q // 2) * 2.0 ** -11)
                    w = float(W[n, hit[2]])
                    if w != 0 and 2.0 ** -20 < abs((t - float(bias[n])) / w) < 2.0 ** 16:
                        a = (t - float(bias[n])) / w
                        seam += 1
            if a is None:
                a = (-1.0) ** pw * 2.0 ** grid[pw % len(grid)]
                pw += 1
            X[b, in1, e] = a
            q += 1
    ref.view(act)[...] = X.reshape(act["nb"], L1 * L0, Cin)
    return dict(K_eff=1, points=q, seam=seam)


def record(rstd, ratio, j):
    """a statistics record {mean, scale, std, 0} of sigma = 1 / rstd and |mean| = ratio sigma"""
    return f32([(-1.0) ** j * ratio / rstd, rstd, 1.0 / rstd, 0.0])


PRO_GAINS = tuple(2.0 ** e for e in (-20, -8, -2, 0, 1, 2, 3, 4, 5))


def craft_gemm_pro(ref, i, op, rng, rnd):
    geo = ref.operands(i)
    conv, act, st = geo["conv"], geo["act"], geo["prostats"]
    G = st["rows"] // act["nb"]
    L1, L0, Cin, S1, _, _, _, seg0, stride0, pad0 = conv[:10]
    assert G == 1 or (G == L0 and S1 == 1 and seg0 == Cin and stride0 == 1 and pad0 == 0), "a group per output position: 1x1 only"
    recs = ref.view(st)[0]
    X = ref.view(act)
    z = rng.standard_normal((act["nb"], act["rows"], Cin))
    for b in range(act["nb"]):
        for g in range(G):
            j = b * G + g
            rstd, ratio = RECORDS[(j + rnd * st["rows"]) % len(RECORDS)]
            recs[j] = record(rstd, ratio, j)
            rows = np.arange(act["rows"]) if G == 1 else np.arange(g, act["rows"], L0)
            gains = np.array(PRO_GAINS)[(rows + j) % len(PRO_GAINS)]
            X[b, rows] = f32(float(recs[j][0]) + gains[:, None] * z[b, rows] / rstd)
    if "epistats" in geo:
        er = ref.view(geo["epistats"])[0]
        for j in range(er.shape[0]):
            rstd, ratio = RECORDS[(j + 4 + rnd * er.shape[0]) % len(RECORDS)]
            er[j] = record(rstd, ratio, j + 1)
    return dict(K_eff=None)


def craft_gemm_hterms(ref, i, op, rng, rnd):
    """round 0: rows of at most one non-zero (K_eff = 1); round 1: the rows of two non-zeros, between zero rows (K_eff = 2)"""
    geo = ref.operands(i)
    conv, act = geo["conv"], geo["act"]
    assert conv[3] == 1 and conv[1] == 1 and conv[7] == conv[2], "a linear layer: one row of K contiguous floats per output row"
    K = conv[2]
    X = np.zeros((act["nb"], act["rows"], K), np.float32)
    names = ("zero", "2^-130", "2^-120", "1", "2^100", "1 and 2^-20", "2^10 and 2^-10")
    rows = dict.fromkeys(names, 0)
    for b in range(act["nb"]):
        for r in range(act["rows"]):
            q = b * act["rows"] + r
            k1, k2, sg = (q * 7919 + 5) % K, (q * 104729 + 11) % K, (-1.0) ** (q // 5)
            kind = q % 5 if rnd == 0 else (0, 5, 6)[q % 3]
            rows[names[kind]] += 1
            if kind in (1, 2, 3, 4):
                X[b, r, k1] = sg * np.float32(2.0) ** np.float32((-130, -120, 0, 100)[kind - 1])
            elif kind in (5, 6) and k1 != k2:
                X[b, r, k1], X[b, r, k2] = sg * (1.0, 2.0 ** 10)[kind - 5], -sg * (2.0 ** -20, 2.0 ** -10)[kind - 5]
    ref.view(act)[...] = X
    return dict(K_eff=1 if rnd == 0 else 2, rows=rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# normalisations and statistics
def craft_layernorm(ref, i, op, rng):
    X = ref.view(ref.operands(i)["act"])[0]
    for r in range(X.shape[0]):
        X[r] = f32(stat_block(STAT_KINDS[r % len(STAT_KINDS)], rng, X.shape[1], r))
    return dict(K_eff=None)


def craft_group_stats(ref, i, op, rng, rnd):
    act = ref.operands(i)["act"]
    X = ref.view(act)
    records = (op["writes"][0][1] - op["writes"][0][0]) // 4
    G = records // act["nb"]
    gs = act["cols"] // G
    for b in range(act["nb"]):
        for g in range(G):
            j = b * G + g
            kind = STAT_KINDS[(j + rnd * records) % len(STAT_KINDS)]
            X[b, :, g * gs:(g + 1) * gs] = f32(stat_block(kind, rng, act["rows"] * gs, j + rnd)).reshape(act["rows"], gs)
    return dict(K_eff=None)


def constant_partials(n_per, parts, j):
    """the fp32 partials (n v, n v^2) of a constant group, v chosen so that sum q - n mean^2 is negative by more than 2^-27 of q:
    decided by the one rounding of the partials, far above what an order of summation in double can move (2^-52 a term)"""
    for t in range(200):
        v = float(np.float32(977.123 + 0.37 * ((j + 17 * t) % 50) + 0.011 * t))
        s, q = float(np.float32(n_per * v)), float(np.float32(n_per * v * v))
        n = n_per * parts
        if parts * q - n * (parts * s / n) ** 2 < -2.0 ** -27 * parts * q:
            return s, q
    raise AssertionError("no constant whose rounded partials give a negative variance")


def craft_stats_reduce(ref, i, op, rng, rnd):
    geo = ref.operands(i)
    rs, (G, count) = geo["rowstat"], geo["reduce"][:2]
    P = ref.view(rs)  # [B][R][NB * 2]
    R_, NB = rs["rows"], rs["cols"] // 2
    for b in range(rs["nb"]):
        for g in range(G):
            j = b * G + g
            rows = np.arange(g, R_, G)
            parts = rows.size * NB
            n_per = count / parts
            kind = STAT_KINDS[(j + rnd * rs["nb"] * G) % len(STAT_KINDS)]
            s, q = np.zeros(parts), np.zeros(parts)
            if kind == "constant":
                s[:], q[:] = constant_partials(n_per, parts, j + rnd)
            elif kind == "spike":
                s[(j * 7919) % parts], q[(j * 7919) % parts] = 3.7 * (-1) ** j, 3.7 ** 2
            elif kind != "zero":
                sigma, ratio = kind
                m = sigma * ratio * (-1) ** j
                e, z = rng.standard_normal(parts), rng.standard_normal(parts)
                s = n_per * m + sigma * np.sqrt(n_per) * e
                q = n_per * (m * m + sigma * sigma) + 2.0 * m * sigma * np.sqrt(n_per) * e + sigma * sigma * np.sqrt(2.0 * n_per) * z * 0.5
            blk = np.stack([s, q], 1).reshape(rows.size, NB * 2)
            P[b, rows] = f32(blk)
    return dict(K_eff=None)


ACT_GAINS = tuple(2.0 ** e for e in (-20, -8, -3, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8))


def craft_gn_act(ref, i, op, rng, rnd):
    geo = ref.operands(i)
    act, st = geo["act"], geo["epistats"]
    G = geo["rows"][2]
    recs = ref.view(st)[0]
    X = ref.view(act)
    gs = act["cols"] // G
    z = rng.standard_normal((act["nb"], act["rows"], act["cols"]))
    gains = np.array(ACT_GAINS)[(np.arange(act["rows"])[:, None] * 5 + np.arange(act["cols"])[None, :]) % len(ACT_GAINS)]
    for b in range(act["nb"]):
        for g in range(G):
            j = b * G + g
            rstd, ratio = RECORDS[(j + rnd * st["rows"]) % len(RECORDS)]
            recs[j] = record(rstd, ratio, j)
            c = slice(g * gs, (g + 1) * gs)
            X[b, :, c] = f32(float(recs[j][0]) + gains[:, c] * z[b, :, c] / rstd)
    return dict(K_eff=None)


ROW_KINDS = 12


def craft_dconv_row(ref, i, op, rng):
    geo = ref.operands(i)["rowtensor"]
    C, T = op["K"] // 3, op["T"]
    F = geo["rows"] // T
    X = ref.view(geo).reshape(geo["nb"], T, F, C)
    z = rng.standard_normal(X.shape)
    for b in range(geo["nb"]):
        for f in range(F):
            kind = (b * F + f) % ROW_KINDS
            if kind == 0:
                X[b, :, f] = 0.0
            elif kind == 1:  # one spike: after the GroupNorm of the hidden tensor its neighbourhood is far out in the GELU's upper range
                X[b, :, f] = f32(0.05 * z[b, :, f])
                X[b, (f * 3) % T, f, (f * 5) % C] = 40.0 * (-1.0) ** f
            elif kind == 11:  # a constant row: the hidden tensor varies with the conv's bias and the padded edges only
                X[b, :, f] = np.float32(3.0 * (-1.0) ** f)
            elif kind == 2:  # an offset of 8 sigma
                X[b, :, f] = f32(8.0 * (-1.0) ** f + z[b, :, f])
            else:
                X[b, :, f] = f32(2.0 ** (-20 + 3 * (kind - 3)) * z[b, :, f])  # gains 2^-20 .. 2^1
    return dict(K_eff=None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the LSTM
def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-v))


UNIT_KINDS = ("remember", "forget", "saturate", "tiny", "closed", "alternate", "smooth", "smooth")


def craft_lstm(ref, i, op, rng):
    """xproj [B][T][2][4 H] (column 4 j + gate, gates i | f | g | o) against an fp64 walk of the recurrence: the pre-activation of
    a crafted unit is what its kind wants, whatever W_hh h adds"""
    geo = ref.operands(i)
    xp, wg = geo["xproj"], geo["W.whh"]
    H, T, B = op["K"], op["T"], xp["nb"]
    U = ref.W[wg["off"]:wg["off"] + 2 * 4 * H * H].astype(np.float64).reshape(2, 4 * H, H)
    X = ref.view(xp).reshape(B, T, 2, H, 4)
    kind = np.arange(H) % 8
    sgn = np.where((np.arange(H) // 8) % 2 == 0, 1.0, -1.0)
    smooth = 0.5 * rng.standard_normal((B, T, 2, H, 4))
    tiny = 2.0 ** -13 * rng.uniform(-1.0, 1.0, (B, T, 2, H, 4))
    for b in range(B):
        for d in range(2):
            h, c = np.zeros(H), np.zeros(H)
            for step in range(T):
                t = step if d == 0 else T - 1 - step
                rec = (U[d] @ h).reshape(H, 4)
                want = smooth[b, t, d].copy()  # the pre-activations
                k = kind == 0
                want[k] = np.stack([np.full(H, 20.0 if step == 0 else -20.0), np.full(H, 20.0), 20.0 * sgn, np.full(H, 20.0)], 1)[k]
                want[kind == 1, 1] = -20.0
                want[kind == 1, 2] = 3.0 * sgn[kind == 1]
                want[kind == 4, :3] = np.stack([np.full(H, 20.0), np.full(H, 20.0), 3.0 * sgn], 1)[kind == 4]  # (c grows behind the closed gate)
                k = kind == 2
                want[k] = np.stack([np.full(H, 20.0), np.full(H, 20.0), 20.0 * sgn, np.full(H, 20.0)], 1)[k]
                want[kind == 3] = tiny[b, t, d][kind == 3]
                want[kind == 4, 3] = -20.0
                want[kind == 5] = (3.0 * (-1.0) ** t * sgn)[kind == 5, None]
                x = f32(want - rec)
                x[kind >= 6] = f32(smooth[b, t, d])[kind >= 6]
                X[b, t, d] = x
                pre = x.astype(np.float64) + rec
                c = sigmoid64(pre[:, 1]) * c + sigmoid64(pre[:, 0]) * np.tanh(pre[:, 2])
                h = sigmoid64(pre[:, 3]) * np.tanh(c)
    return dict(K_eff=None)


def roles_outside_reads(ref, i):
    """the operand roles of op i (interp_operands) that do not lie inside one of the op's declared read ranges - what is written
    there would reach the reference and not the device"""
    reads = ref.ops[i]["reads"]
    bad = []
    for role, g in ref.operands(i).items():
        if isinstance(g, dict) and not role.startswith("W."):
            lo, hi = g["off"], g["off"] + (g["nb"] - 1) * g["batch"] + (g["rows"] - 1) * g["ld"] + g["cols"]
            if not any(rlo <= lo and hi <= rhi for rlo, rhi in reads):
                bad.append((role, lo, hi))
    return bad


def craft(ref, i, case, rnd=0):
    """writes round `rnd` of op i's crafted operands into the reference's arena; returns dict(K_eff, ...)"""
    op = ref.ops[i]
    fam = family_of(op)
    assert not roles_outside_reads(ref, i), (op["name"], roles_outside_reads(ref, i), op["reads"])
    rng = np.random.default_rng(seed_of(case, op, rnd))
    fill_reads(ref, op, rng)
    if fam == "gemm_plain":
        return craft_gemm_plain(ref, i, op, rng, rnd)
    if fam == "gemm_pro":
        return craft_gemm_pro(ref, i, op, rng, rnd)
    if fam == "gemm_hterms":
        return craft_gemm_hterms(ref, i, op, rng, rnd)
    if fam == "layernorm":
        return craft_layernorm(ref, i, op, rng)
    if fam == "group_stats":
        return craft_group_stats(ref, i, op, rng, rnd)
    if fam == "stats_reduce":
        return craft_stats_reduce(ref, i, op, rng, rnd)
    if fam == "gn_act":
        return craft_gn_act(ref, i, op, rng, rnd)
    if fam == "dconv_row":
        return craft_dconv_row(ref, i, op, rng)
    assert fam == "lstm"
    return craft_lstm(ref, i, op, rng)


# ---------------------------------------------------------------------------------------------------------------------------------
# The classes a crafted op must have evaluated, as sums of census bins (op_reference.CENSUS)
GELU6 = {k: [k] for k in ("gelu-lo", "gelu-mid", "gelu-hi", "gelu+lo", "gelu+mid", "gelu+hi")}
SEAMS = {"gelu_edge_below": ["gelu_edge_below"], "gelu_edge_above": ["gelu_edge_above"]}
SIG8 = {}
for _s in "-+":
    SIG8.update({f"sig{_s}<1": [f"sig{_s}<2^-10", f"sig{_s}<1"], f"sig{_s}1-17": [f"sig{_s}<9", f"sig{_s}<17"], f"sig{_s}17-89": [f"sig{_s}<89"],
                 f"sig{_s}>=89": [f"sig{_s}>=89"]})
LSTM_SIG = {"sig<2^-10": ["sig-<2^-10", "sig+<2^-10"], "sig<1": ["sig-<1", "sig+<1"], "sig1-9": ["sig-<9", "sig+<9"],
            "sig>9": ["sig-<17", "sig+<17", "sig-<89", "sig+<89", "sig->=89", "sig+>=89"]}
LSTM_TANH = {"tanh<2^-10": ["tanh-<2^-10", "tanh+<2^-10"], "tanh<1": ["tanh-<1", "tanh+<1"], "tanh1-9": ["tanh-<9", "tanh+<9"],
             "tanh>9": ["tanh->=9", "tanh+>=9"]}
STAT_RATIO = {k: [k] for k in ("stat_zero", "stat_const", "stat_ratio<1", "stat_ratio<64", "stat_ratio>=64")}
STAT_SIGMA = {k: [k] for k in ("stat_sigma<2^-10", "stat_sigma<2^6", "stat_sigma>=2^6")}
EVALS = 256  # evaluations a class of a function must hold

# classes a family's shapes cannot reach, and why
UNREACHABLE = {
    "seams on a dense operand": "gemm_pro, gn_act and dconv_row evaluate GELU on dense random arguments: one lands within 2^-10 of the seam by chance "
                                "only (about one in a thousand); gemm_plain aims at it",
    "stat_clamped outside stats_reduce": "layernorm_kernel is two-pass; group_stats sums elements in double, where the sign of q - n mean^2 of a constant group "
                                         "is decided by the order of summation (2^-52 a term) - only fp32 partials can be made to decide it",
    "stat_spike in stats_reduce": "the op sees partials, not elements: the census cannot tell a spike from a spread",
    "dconv_row beyond the middle range": "both activations sit behind a GroupNorm over the row: the argument is bounded by sqrt(n - 1) |w| + |b| of the "
                                         "synthetic affine, about 3; constant and zero ROWS are written, but the statistics are those of conv outputs, which the bias "
                                         "and the padded edges spread: no constant set, no clamp",
    "lstm_c>=8 at T < 9": "|c| grows by at most 1 a step",
    "256 records": "a statistics class counts rows, groups or records, and an op has 2 to 256 of them: every kind is dealt round-robin, so a class holds "
                   "at least records // 16, and at least 1 over the rounds of an op with fewer records than kinds",
    "256 seam hits": "one output per lattice point can be aimed at the seam; a shape with P points aims P / 2 of them, a quarter on each side and sign: a seam "
                     "class holds at least min(256, hits // 4)",
}


def classes_possible(fam, op, infos, records):
    """[(group, {class: census bins}, least count per class)] for an op of family fam; infos: what craft returned per round"""
    stat_min = max(1, records // 16)
    if fam == "gemm_plain":
        if op["act"] == 1:
            return [("gelu", GELU6, EVALS), ("seam", SEAMS, min(EVALS, sum(f["seam"] for f in infos) // 4))]
        return [("sigmoid", SIG8, EVALS)]
    if fam == "gemm_pro":
        out = [("gelu", GELU6, EVALS)] if op["pro"] == 2 or op["act"] == 1 else []
        return out + ([("sigmoid", SIG8, EVALS)] if op["epi"] == R.EPI_GN_GLU_SCALE_RES else [])
    if fam == "gemm_hterms":
        return []
    if fam in ("layernorm", "group_stats"):
        return [("ratio", STAT_RATIO, stat_min), ("sigma", STAT_SIGMA, stat_min), ("spike", {"stat_spike": ["stat_spike"]}, stat_min)]
    if fam == "stats_reduce":
        return [("ratio", STAT_RATIO, stat_min), ("sigma", STAT_SIGMA, stat_min), ("clamp", {"stat_clamped": ["stat_clamped"]}, stat_min)]
    if fam == "gn_act":
        return [("gelu", GELU6, EVALS)] if op["mode"] == 1 else [("sigmoid", SIG8, EVALS)]
    if fam == "dconv_row":
        return [("gelu", {k: GELU6[k] for k in ("gelu-lo", "gelu-mid", "gelu+lo", "gelu+mid")}, EVALS),
                ("sigmoid", {k: SIG8[k] for k in ("sig-<1", "sig-1-17", "sig+<1", "sig+1-17")}, EVALS)]
    assert fam == "lstm"
    return [("sigmoid", LSTM_SIG, EVALS), ("tanh", LSTM_TANH, EVALS)] + ([("cell", {"lstm_c>=8": ["lstm_c>=8"]}, EVALS)] if op["T"] >= 9 else [])


def census_failures(fam, op, infos, census, records):
    """the census conditions: every possible class holds its least count, no class of a group more than 60 % of the group"""
    bad = []
    for group, classes, least in classes_possible(fam, op, infos, records):
        counts = {k: sum(census[b] for b in bins) for k, bins in classes.items()}
        total = sum(counts.values())
        for k, n in counts.items():
            if n < least:
                bad.append(f"{group}: {k} holds {n} < {least}")
            if len(counts) > 1 and n > 0.6 * total:
                bad.append(f"{group}: {k} holds {n} of {total}: more than 60 %")
    return bad


def records_of(ref, i, fam):
    geo = ref.operands(i)
    if fam == "layernorm":
        return geo["act"]["rows"]
    if fam == "group_stats":
        return (ref.ops[i]["writes"][0][1] - ref.ops[i]["writes"][0][0]) // 4
    if fam == "stats_reduce":
        return geo["rowstat"]["nb"] * geo["reduce"][0]
    return 0
