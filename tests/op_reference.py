"""The op-level reference shared by tests/test_op_reference_cpu.py (no GPU) and tests/test_gpu_op_parity.py: the step interface of
tests/cpu_interp.cpp (one op of a plan at a time, in fp32 or in double with a magnitude per written element) and the error bound
each op's fp32 implementation is held to.

The bound. u = 2^-24. For an element the reference wrote, r its value in double and s its magnitude (cpu_interp.cpp struct P: the
sum of the absolute values of the terms added to form it, carried through products and through the non-linear functions by
their Lipschitz constants), an fp32 implementation g passes when |g - r| <= c u s. c counts the fp32 roundings on the longest
path to an element (`bound_c`, one derivation per line); there is no absolute term: where s = 0 the result must be exactly 0.
An implementation that rounds to nearest makes an error of at most u/2 per operation relative to the partial result, which s
bounds, so c roundings stay within c u s / 2: the table holds with a factor two in hand, none of it fitted to a kernel."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libcpu_interp.so")
U = 2.0 ** -24

OP_IGEMM, OP_STATS_REDUCE, OP_STFT, OP_LAYERNORM, OP_GN_APPLY, OP_ATTENTION, OP_ISTFT, OP_OLA, OP_TAP = range(9)
OP_GROUP_STATS, OP_GN_ACT, OP_LSTM, OP_LOCAL_ATTN, OP_DCONV_ROW = range(9, 14)
EPI_LINEAR, EPI_SCALE_RES, EPI_GLU, EPI_GN_GLU_SCALE_RES, EPI_STATS_ONLY, EPI_TRCONV, EPI_STATS_FACT, EPI_KPL, EPI_VT = range(9)
GEMM = {"f32": 0, "bf16x3": 1, "fp16x3": 2}

# model key of the tmp_models fixture, segment samples, batch, arithmetics: what each shape is for (the issue's table)
CASES = {
    "4s_16384": (4, 16384, 1, ("bf16x3",)),          # operand planes on both branches (128 and 64 key tokens)
    "4s_8000": (4, 8000, 2, ("bf16x3", "fp16x3")),   # planes on the frequency branch only; time lengths 2000 / 500 / 125 / 32; batch strides
    "6s_7000": (6, 7000, 2, ("f32", "bf16x3")),      # 7 frames; 56 and 28 tokens (no whole key tile); head dim 48; N = 96 last transposed conv
    "v3_7000": (3, 7000, 2, ("f32", "bf16x3")),      # LSTM, LocalState, GroupStats / GnAct, the k4 / s2 transposed conv
}


# the value classes of cpu_interp.cpp's census, in its order
CENSUS = (["gelu-lo", "gelu-mid", "gelu-hi", "gelu+lo", "gelu+mid", "gelu+hi", "gelu_edge_below", "gelu_edge_above"]
          + [f"sig{s}{c}" for s in "-+" for c in ("<2^-10", "<1", "<9", "<17", "<89", ">=89")]
          + [f"tanh{s}{c}" for s in "-+" for c in ("<2^-10", "<1", "<9", ">=9")]
          + ["stat_all", "stat_zero", "stat_const", "stat_ratio<1", "stat_ratio<64", "stat_ratio>=64", "stat_sigma<2^-10", "stat_sigma<2^6",
             "stat_sigma>=2^6", "stat_clamped", "stat_spike", "lstm_c>=8", "gemm_row_nonzeros_max"])


def lib():
    srcs = [os.path.join(ROOT, "tests", "cpu_interp.cpp")] + [os.path.join(ROOT, "demucs_cpp_amd", "csrc", f)
                                                              for f in ("plan.cpp", "plan.h", "model_pack.cpp", "gemm_select.cpp", "plan_describe.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["make", "-C", ROOT, "interp"], stdout=subprocess.DEVNULL)
    L = ctypes.CDLL(SO)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    L.interp_create_chosen.restype = vp
    L.interp_create_chosen.argtypes = [ctypes.c_char_p, i64, ci, ci, ci]
    L.interp_create.restype = vp
    L.interp_create.argtypes = [ctypes.c_char_p, i64, ci]
    L.interp_free.argtypes = [vp]
    L.interp_n_ops.argtypes = [vp]
    for f in ("interp_arena_floats", "interp_const_floats", "interp_mix_off", "interp_out_off"):
        getattr(L, f).restype = i64
        getattr(L, f).argtypes = [vp]
    for f in ("interp_arena", "interp_mask", "interp_precise", "interp_magnitude"):
        getattr(L, f).restype = vp
        getattr(L, f).argtypes = [vp]
    L.interp_planes.restype = i64
    L.interp_planes.argtypes = [vp, vp, vp]
    L.interp_op_info.argtypes = [vp, ci, ctypes.c_char_p, ci]
    L.interp_step.argtypes = [vp, ci, ci]
    L.interp_set_attention.argtypes = [vp, ci, vp, vp, vp, vp]
    L.interp_run.argtypes = [vp, vp, vp]
    L.interp_weights.restype = vp
    L.interp_weights.argtypes = [vp]
    L.interp_weight_floats.restype = i64
    L.interp_weight_floats.argtypes = [vp]
    L.interp_operands.argtypes = [vp, ci, ctypes.c_char_p, ci]
    L.interp_census.argtypes = [vp, ci]
    return L


def _view(addr, n, dtype):
    return np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctypes.c_ubyte)), shape=(n * np.dtype(dtype).itemsize,)).view(dtype)


class Ref:
    """One interpreter handle: the plan a context of arithmetic `gemm` builds, its arena and the step interface."""

    def __init__(self, L, path, seg, B, gemm, kv_planes):
        from demucs_cpp_amd.binding import parse_op_info

        self.L = L
        self.h = L.interp_create_chosen(path.encode(), seg, B, GEMM[gemm], int(kv_planes))
        assert self.h
        self.n_ops = L.interp_n_ops(self.h)
        self.floats = L.interp_arena_floats(self.h)
        self.consts = L.interp_const_floats(self.h)
        self.mix_off, self.out_off = L.interp_mix_off(self.h), L.interp_out_off(self.h)
        self.A = _view(L.interp_arena(self.h), self.floats, np.float32)
        self.W = _view(L.interp_weights(self.h), L.interp_weight_floats(self.h), np.float32)
        self.text, self.ops = [], []
        buf = ctypes.create_string_buffer(4096)
        for i in range(self.n_ops):
            assert L.interp_op_info(self.h, i, buf, 4096) > 0
            self.text.append(buf.value.decode())
            self.ops.append(parse_op_info(self.text[-1]))
        self.mask = self.R = self.S = None

    def set_mix(self, mix):
        """mix (B, 2, seg) -> the arena's [B][seg][2]"""
        m = np.ascontiguousarray(mix.transpose(0, 2, 1), np.float32).ravel()
        self.A[self.mix_off:self.mix_off + m.size] = m

    def step(self, i, precise, hterms=False, chained=False):
        assert self.L.interp_step(self.h, i, (1 if precise else 0) | (2 if hterms else 0) | (4 if chained else 0)) == 0
        if self.mask is None:
            self.mask = _view(self.L.interp_mask(self.h), self.floats, np.uint8)
        if precise and self.R is None:
            self.R = _view(self.L.interp_precise(self.h), self.floats, np.float64)
            self.S = _view(self.L.interp_magnitude(self.h), self.floats, np.float32)

    def set_attention(self, i, q, k, v, decay=None):
        """operands of attention op i written where the op reads them (cpu_interp.cpp interp_set_attention): q [B][Tq][H hs], k / v
        [B][Tk][H hs]; decay [B][T][16] for a LocalState op"""
        arr = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (q, k, v, decay)]
        assert self.L.interp_set_attention(self.h, i, *[None if a is None else a.ctypes.data for a in arr]) == 0

    def operands(self, i):
        """where op i reads its operands, by role (cpu_interp.cpp interp_operands): role -> dict(off, rows, cols, ld, batch, nb); the
        words conv, rows and reduce -> their tuple of integers"""
        buf = ctypes.create_string_buffer(1024)
        assert self.L.interp_operands(self.h, i, buf, 1024) >= 0
        out = {}
        for word in buf.value.decode().split():
            role, v = word.split("=")
            v = tuple(int(t) for t in v.split(":"))
            out[role] = v if role in ("conv", "rows", "reduce") else dict(zip(("off", "rows", "cols", "ld", "batch", "nb"), v))
        return out

    def view(self, geo):
        """the arena elements of one operand (operands()) as an array [nb][rows][cols] that writes through"""
        return np.lib.stride_tricks.as_strided(self.A[geo["off"]:], (geo["nb"], geo["rows"], geo["cols"]), (4 * geo["batch"], 4 * geo["ld"], 4))

    def census(self):
        """evaluations per value class of the last precise step (cpu_interp.cpp interp_census): name -> count"""
        n = self.L.interp_census(None, 0)
        arr = (ctypes.c_longlong * n)()
        self.L.interp_census(arr, n)
        assert n == len(CENSUS)
        return dict(zip(CENSUS, (int(v) for v in arr)))

    def planes(self):
        """(r, s) of the last precise step's K / V operand planes, indexed like the elements of plane 0; None if it wrote none"""
        r, s = ctypes.c_void_p(), ctypes.c_void_p()
        n = self.L.interp_planes(self.h, ctypes.byref(r), ctypes.byref(s))
        if n == 0:
            return None
        return _view(r.value, n, np.float64).copy(), _view(s.value, n, np.float32).copy()

    def close(self):
        if self.h:
            self.mask = self.R = self.S = self.A = self.W = None
            self.L.interp_free(self.h)
            self.h = None


def written(ref, op):
    """indices (into the arena) of the elements the last step wrote, taken inside the op's write ranges - and a check that it wrote
    nothing outside them"""
    idx = []
    for lo, hi in op["writes"]:
        idx.append(lo + np.flatnonzero(ref.mask[lo:hi]))
    idx = np.unique(np.concatenate(idx)) if idx else np.zeros(0, np.int64)
    assert int(ref.mask.sum()) == idx.size, f"{op['name']}: the reference wrote outside the op's write ranges"
    return idx


def launches(op):
    """does the op launch a kernel of its own (GPU word `launches`; for the interpreter's plan: every op but a marker)"""
    return op.get("launches", int(op["kind"] != OP_TAP)) != 0


def bound_c(op, mode):
    """c of |g - r| <= c u s for the op as described by dmx_debug_op_info / interp_op_info, in a context of arithmetic `mode`"""
    kind, K = op["kind"], op.get("K", 0)
    split = mode != "f32"
    if kind == OP_IGEMM:
        arith = op["arith"] if op["family"] != 0 else (1 if split else 0)  # (interpreter plans of a split mode: the split bound)
        # fp32 operands: one fmaf chain of K terms. bf16 terms: five partial products per k, each accumulated in fp32, and the dropped
        # a3 w2 product <= u |a w| per k: 6 K. fp16 terms: three products per k (6 K covers it; the dropped remainders are in s)
        c = (K if arith == 0 else 6 * K) + 8  # + 8: bias, activation (GELU: dmx_erff's 9.7e-8 = 1.6 u, three products), scale, residual
        if op["pro"] == 1:
            c += 2  # PRO_AFFINE: a subtraction and a product per operand element
        if op["pro"] == 2:
            c += 12  # PRO_GN_GELU: subtract, two scales, affine (4), GELU (erf 2, three products, the sqrt(1/2) scale: 6), fma slack 2
        if op["epi"] in (EPI_GLU, EPI_GN_GLU_SCALE_RES):
            c += 8  # sigmoid: negate-scale, exp2, add, rcp (1 ulp each), product, table / scale product and add
        if op["epi"] == EPI_GN_GLU_SCALE_RES:
            c += 8  # GroupNorm of both halves: subtract, two scales, affine
        if op["stat"]:
            c += op["BN"] + 2  # the column block's additions, the square
        return c
    if kind == OP_ATTENTION:
        T = op["T"]
        # scores: hs terms (x 6 in bf16 terms), scale, running maximum subtracted, exp2 of a scaled argument (2), the sum over keys
        # (T), one rescale per 16-key step of the online form (T / 16, twice: sum and output), reciprocal and product, then T
        # weighted values (x 6 in bf16 terms: the weights are split as well)
        return (6 if op.get("split", int(split)) else 1) * (K + T) + T + T // 8 + 16
    if kind == OP_LAYERNORM:
        return 2 * K + 8  # mean: K additions; variance: K more; subtract, two scales, affine, positional add
    if kind == OP_STATS_REDUCE or kind == OP_GROUP_STATS:
        return 8  # sums in double on the device: the roundings of mean, sqrt, add eps, reciprocal and of the stores
    if kind in (OP_STFT, OP_ISTFT, OP_OLA):
        # 12 radix-2 stages (or fewer of higher radix), per stage a complex product (4 products, 2 additions with fp32 twiddles: 6)
        # and an addition, + window, scale, the overlap-add's 4 terms with their normalisation, the time branch's affine
        return 8 * 12 + 16
    if kind == OP_GN_APPLY:
        return 6
    if kind == OP_GN_ACT:
        return 20  # GroupNorm of two channels (2 x 4), sigmoid or GELU (6), product, scale, residual
    if kind == OP_LSTM:
        # per step: a gate sums H terms onto the projection; sigmoid / tanh (exp2, rcp: 6), the cell update (3), tanh and product.
        # The reference's magnitudes are those of ONE step (cpu_interp.cpp run_lstm re-bases the state), so the steps before an
        # output enter as one allowance each: T of them
        return op["T"] * (K + 24)
    if kind == OP_LOCAL_ATTN:
        T = op["T"]
        return K + 2 * T + T // 8 + 32  # as attention in fp32 + the four decay terms and their sigmoids
    if kind == OP_DCONV_ROW:
        # per layer: K1 (3 C terms), GroupNorm + GELU (12), K2 (16 terms), GroupNorm + GLU + scale + residual (16); statistics in
        # double, taken as numbers of their own (cpu_interp.cpp inner_stats). Two layers, fp32 MFMAs in every arithmetic
        return 2 * (K + 16 + 28)
    return 0


def ratios(g, r, s):
    """|g - r| / (u s) per element; an element with s = 0 must be exactly 0: its ratio is 0 or inf"""
    d = np.abs(g.astype(np.float64) - r)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = d / (U * s.astype(np.float64))
    q[(s == 0) & (d == 0)] = 0.0
    q[~np.isfinite(g)] = np.inf
    return q


def rms(q):
    q = q[np.isfinite(q)]
    return float(np.sqrt(np.mean(q * q))) if q.size else 0.0


# The RMS rule. The worst-case bound is loose wherever c is large (a K-term sum is allowed K roundings in one direction); there
# the RMS of (g - r) / (u s) over the op's outputs must not exceed RMS_CAP times the same statistic of the interpreter's fp32
# arithmetic on the same inputs - the reference's own fp32 error. 4: five partial products per k give sqrt(5) in a random-walk
# model, and the MFMA's 4-wide summation order differs from the k-ordered chain. No floor and no exception: the largest ratio
# measured on an MI355X is 3.3 (the STFT: fp32 butterflies against the interpreter's double FFT rounded once), GEMMs <= 1.16.
# Ops with c <= RMS_MIN_C (a handful of roundings per element: gn_apply, the statistics ops) are at the worst-case bound anyway.
RMS_CAP = 4.0
RMS_MIN_C = 16


def rms_rule_applies(op, mode):
    return bound_c(op, mode) > RMS_MIN_C


def rms_rule_ok(rms_impl, rms_fp32):
    return rms_impl <= RMS_CAP * rms_fp32


def bf16_planes_sum(words, n):
    """three bf16 planes of n elements (uint16, [3][n]) -> (fp64 sum, the three terms as fp64)"""
    t = (words[:3 * n].astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(3, n)
    return t.sum(0), t


def step_pair(ref, i, hterms):
    """steps op i and, if it is a fused inverse STFT, the overlap-add after it, in double. Returns the index of the op that launched
    (the last one stepped)"""
    op = ref.ops[i]
    if op["kind"] == OP_ISTFT and op.get("fused", 0):
        ref.step(i, True)
        ref.step(i + 1, True, chained=True)
        return i + 1
    ref.step(i, True, hterms=hterms)
    return i


# ---------------------------------------------------------------------------------------------------------------------------------
# The check itself: what an implementation of op `op` left in an arena that held `canary` everywhere but in the op's read ranges
# and the plan's constants, against the reference's last precise step. Used on the GPU (the HIP kernel's arena) and, in
# tests/test_op_reference_cpu.py, on the interpreter's own fp32 arithmetic with and without deliberate mistakes.
CANARY_A = 0x7FC0DEAD  # a quiet NaN with a recognisable payload
CANARY_B = int(np.float32(-3.0e37).view(np.uint32))  # a large finite value: whatever reads it without declaring so changes its result


class OpMismatch(AssertionError):
    pass


def plane_range(op):
    """[lo, hi) floats of the three bf16 operand planes a K / V projection writes, or None"""
    if op["kind"] == OP_IGEMM and "kv" in op:
        return op["kv"], op["kv"] + (3 * op["kvPlane"] + 1) // 2
    return None


def snapshot(ref, op):
    """what the last precise step of the reference wrote: indices of its fp32 results, their r and s, and the planes' (r, s)"""
    idx = written(ref, op)
    pr = plane_range(op)
    if pr:
        idx = idx[(idx < pr[0]) | (idx >= pr[1])]
    return {"idx": idx, "r": ref.R[idx].copy(), "s": ref.S[idx].copy(), "planes": ref.planes() if pr else None}


def expected_arena(n_floats, canary, consts_u32, reads, read_values):
    """the arena before the launch: the canary everywhere but in the constants and in the op's read ranges (their uploaded values)"""
    e = np.full(n_floats, canary, np.uint32)
    e[:consts_u32.size] = consts_u32
    for (lo, hi), v in zip(reads, read_values):
        e[lo:hi] = v.view(np.uint32)
    return e


def effective(op, K_eff):
    """the op with the number of non-zero terms its operands really put into each sum in place of K (None: the op as it is): the
    same line of bound_c's table, for operands crafted so that a sum has K_eff terms"""
    return op if K_eff is None else dict(op, K=K_eff)


def check_op(op, mode, arena_u32, before_u32, snap, K_eff=None):
    """arena_u32: what the implementation left of before_u32 (expected_arena). Raises OpMismatch; returns (worst ratio, the ratios
    of every compared element)"""
    name, c = op["name"], bound_c(effective(op, K_eff), mode)
    g = arena_u32.view(np.float32)
    # ---- values
    q = ratios(g[snap["idx"]], snap["r"], snap["s"])
    allq = [q]
    pr = plane_range(op)
    if pr:
        n = op["kvPlane"]
        pr_r, pr_s = snap["planes"]
        total, terms = bf16_planes_sum(arena_u32[pr[0]:pr[1]].view(np.uint16), n)
        if not (np.isfinite(total).all() and (total.astype(np.float32).astype(np.float64) == total).all()):
            raise OpMismatch(f"{name}: the three plane terms do not add up to an fp32 number everywhere")
        a = np.abs(total)
        if not ((np.abs(terms[1]) <= 2.0 ** -8 * a).all() and (np.abs(terms[2]) <= 2.0 ** -16 * a).all()):
            raise OpMismatch(f"{name}: plane terms out of order (|a2| <= 2^-8 |v|, |a3| <= 2^-16 |v|)")
        allq.append(ratios(total, pr_r, pr_s))
    allq = np.concatenate(allq)
    worst = float(allq.max()) if allq.size else 0.0
    if not worst <= c:
        k = int(np.argmax(allq))
        raise OpMismatch(f"{name}: |g - r| = {worst:.4g} u s exceeds c = {c} (element {k} of {allq.size}; label {op.get('label')})")
    # ---- containment: outside what the reference wrote (and the scratch the op declares) every float still holds the canary
    touched = np.flatnonzero(arena_u32 != before_u32)
    allowed = np.zeros(arena_u32.size, bool)
    allowed[snap["idx"]] = True
    if pr:
        allowed[pr[0]:pr[1]] = True
    for lo, hi in op["scratch"]:
        allowed[lo:hi] = True
    bad = touched[~allowed[touched]]
    if bad.size:
        inside = any(lo <= bad[0] < hi for lo, hi in op["writes"])
        raise OpMismatch(f"{name}: {bad.size} elements changed that the op does not write, first at {int(bad[0])} "
                         f"({'inside' if inside else 'OUTSIDE'} its write ranges {op['writes']})")
    return worst, allq


def canary_arena(ref, op_reads, canary):
    """prepares the interpreter's arena as the device's is prepared (expected_arena). Returns (the saved arena: restore with
    ref.A[:] = saved, the prepared image)"""
    saved = ref.A.copy()
    before = expected_arena(ref.floats, canary, saved.view(np.uint32)[:ref.consts], op_reads, [saved[lo:hi] for lo, hi in op_reads])
    ref.A.view(np.uint32)[:] = before
    return saved, before


# ---------------------------------------------------------------------------------------------------------------------------------
# The GPU side of the op-level tests (tests/test_gpu_op_parity.py, tests/test_gpu_attention_crafted.py, tests/test_gpu_value_cases.py): a context beside the
# interpreter handle of the same plan, and the check of one launch.
DEVICE_ERROR = []  # the first error the library reported from the device: after it no op-level test launches anything


class Pair:
    """a context and the interpreter handle of the same plan; `cases`: the table `case` is a key of (default CASES)"""

    def __init__(self, dmxb, L, tmp_models, case, mode, zero_segment=False, cases=None):
        assert not DEVICE_ERROR, f"an earlier launch failed on the device, nothing more is launched: {DEVICE_ERROR[0]}"
        self.dmxb = dmxb
        key, seg, B, _ = (cases or CASES)[case]
        self.B, self.mode, self.case = B, mode, case
        self.model = dmxb.Model(tmp_models[key], 0)
        self.ctx = dmxb.Context(self.model, seg, B, gemm=GEMM[mode])
        self.n_ops, self.ctx_floats, self.floats, self.consts = self.ctx.plan_info(B)
        self.gops = [self.ctx.op_info(B, i) for i in range(self.n_ops)]
        # a split context of a v4 model asks for K / V operand planes and falls back to the fp32-K/V form where a projection cannot
        # take its exact-split kernel (exec.cpp dmx_get_plan): the reference is built the same way
        self.ref = Ref(L, tmp_models[key], seg, B, mode, mode != "f32" and key != 3)
        if self.ref.floats != self.floats and not any(o["kind"] == OP_ATTENTION and o.get("planes") for o in self.gops):
            self.ref.close()
            self.ref = Ref(L, tmp_models[key], seg, B, mode, False)
        rng = np.random.default_rng(seg + B)
        mix = (0.1 * rng.standard_normal((B, 2, seg))).astype(np.float32)
        if zero_segment:
            mix[B - 1] = 0.0
        self.ref.set_mix(mix)
        # the constants as the LIBRARY computed them (the interpreter's come from another compiler: window sums differ in the last bit)
        self.ctx.arena_fill(B, CANARY_A)
        self.consts_u32 = self.ctx.arena_read(0, self.consts).view(np.uint32).copy()
        self.buf = np.empty(self.ctx_floats, np.float32)

    def assert_same_plan(self):
        ref = self.ref
        assert ref.n_ops == self.n_ops and ref.floats == self.floats and ref.consts == self.consts
        for a, b in zip(ref.ops, self.gops):
            assert (a["name"], a["kind"], a["reads"], a["writes"], a["scratch"]) == (b["name"], b["kind"], b["reads"], b["writes"], b["scratch"])

    def prepare(self, canary, reads, values):
        self.ctx.arena_fill(self.B, canary)
        for (lo, hi), v in zip(reads, values):
            self.ctx.arena_write(lo, v)

    def close(self):
        self.ref.close()
        self.ctx.close()
        self.model.close()


def float_rms(ref, i, j, snap, op):
    """RMS ratio of the interpreter's fp32 arithmetic for ops i .. j on the current inputs; leaves the arena as it was"""
    hull = [rg for k in range(i, j + 1) for rg in ref.ops[k]["writes"]]
    saved = [ref.A[lo:hi].copy() for lo, hi in hull]
    for k in range(i, j + 1):
        ref.step(k, False)
    q = [ratios(ref.A[snap["idx"]], snap["r"], snap["s"])]
    pr = plane_range(op)
    if pr:
        total, _ = bf16_planes_sum(ref.A[pr[0]:pr[1]].view(np.uint16), op["kvPlane"])
        q.append(ratios(total, *snap["planes"]))
    for (lo, hi), v in zip(hull, saved):
        ref.A[lo:hi] = v
    return rms(np.concatenate(q))


def written_bits(fetch, op, snap):
    """the bits of everything the op wrote; fetch(lo, hi) -> the arena's uint32 words [lo, hi) (write ranges only are asked for)"""
    pr, idx, out = plane_range(op), snap["idx"], []
    for lo, hi in op["writes"]:
        words = fetch(lo, hi)
        out.append(words[idx[(idx >= lo) & (idx < hi)] - lo])
        if pr and lo <= pr[0] and pr[1] <= hi:
            out.append(words[pr[0] - lo:pr[1] - lo])
    return np.concatenate(out)


def check_launch(pair, i, j, op, reads, values, snap, K_eff=None):
    """Op j of the context's plan (the reference stepped ops i .. j: a fused pair, else i == j) launched alone on `values` in its
    read ranges: from canary A (value bound and containment: check_op), again with canary B in everything it does not declare to
    read (the same bits), and the RMS rule against the interpreter's fp32 arithmetic on the same inputs. Raises OpMismatch;
    returns (worst ratio, RMS of the kernel, RMS of the fp32 interpreter or None, the bits the kernel wrote)"""
    ref, ctx, B, mode = pair.ref, pair.ctx, pair.B, pair.mode
    # ---- the kernel on canary A
    pair.prepare(CANARY_A, reads, values)
    ctx.run_op(B, j)
    got = ctx.arena_read(0, pair.ctx_floats, pair.buf).view(np.uint32)
    before = expected_arena(pair.ctx_floats, CANARY_A, pair.consts_u32, reads, values)
    worst, q = check_op(op, mode, got, before, snap, K_eff)
    bits_a = written_bits(lambda lo, hi: got[lo:hi], op, snap)
    # ---- the same launch with canary B in everything it does not declare to read
    pair.prepare(CANARY_B, reads, values)
    ctx.run_op(B, j)
    bits_b = written_bits(lambda lo, hi: ctx.arena_read(lo, hi - lo).view(np.uint32), op, snap)
    if not np.array_equal(bits_b, bits_a):
        k = int(np.flatnonzero(bits_b != bits_a)[0])
        raise OpMismatch(f"{op['name']}: the result depends on arena contents outside its declared read ranges (first at written element {k})")
    rms_g = rms(q)
    rms_f = None
    if rms_rule_applies(effective(op, K_eff), mode):
        # the interpreter's fp32 arithmetic on the same inputs (restored: the precise step may have worked in place)
        after = [ref.A[lo:hi].copy() for lo, hi in reads]
        for (lo, hi), v in zip(reads, values):
            ref.A[lo:hi] = v
        rms_f = float_rms(ref, i, j, snap, op)
        for (lo, hi), v in zip(reads, after):
            ref.A[lo:hi] = v
        # the precise results are the chain: put them back over what the fp32 step restored
        ref.A[snap["idx"]] = snap["r"].astype(np.float32)
        if not rms_rule_ok(rms_g, rms_f):
            raise OpMismatch(f"{op['name']}: RMS of (g - r) / (u s) = {rms_g:.4f}, the fp32 interpreter's is {rms_f:.4f} (cap {RMS_CAP} x)")
    return worst, rms_g, rms_f, bits_a


def run_variants(pair, j, op, reads, values, snap, bits_plan, variants, launched, K_eff=None):
    """GEMM j on every tile cfg of its shape (dmx_debug_op_cfgs) under lin_mode 0 / 1 / 3: each distinct (cfg, family, wnf) meets the
    op's bound; results of one arithmetic are bit-identical whatever the tile or family (gemm_tiles.h DMX_TILES: siblings keep the column
    decomposition; gemm_select.h: all families of one arithmetic give the same bits) - row-statistics partials included, among
    tiles of one column block width. The direct kernels (cfg 8, chosen by shape alone, with a k order of their own: dgemm.hip) are
    outside that claim: where the plan's kernel is one, the tile variants are compared with each other. K_eff: as check_op takes it
    (crafted operands: a sibling of another arithmetic than the plan's is held to ITS line of the table at that K)."""
    ctx, B = pair.ctx, pair.B
    DIRECT = 8
    seen = {(op["cfg"], op["family"], op["wnf"])}
    claim = lambda o: (o["arith"], o["BN"] if op["stat"] else 0)
    bases = {} if op["cfg"] == DIRECT else {claim(op): (bits_plan, op)}
    for cfg in ctx.op_cfgs(B, j):
        for lin_mode in (0, 1, 3):
            pair.prepare(CANARY_A, reads, values)
            ch = ctx.run_op_as(B, j, cfg, lin_mode)
            if ch is None:
                variants["refused"].add((cfg, op["pro"], op["epi"]))
                continue
            key = (ch["cfg"], ch["family"], ch["wnf"])
            launched.append((ch["cfg"], ch["family"], ch["label"]))
            if key in seen:
                continue
            seen.add(key)
            vop = dict(op, **ch)
            got = ctx.arena_read(0, pair.ctx_floats, pair.buf).view(np.uint32)
            before = expected_arena(pair.ctx_floats, CANARY_A, pair.consts_u32, reads, values)
            try:
                check_op(vop, pair.mode, got, before, snap, K_eff)
            except OpMismatch as e:
                raise OpMismatch(f"as cfg {ch['cfg']} family {ch['family']} wnf {ch['wnf']} ({ch['label']}): {e}")
            bits = written_bits(lambda lo, hi: got[lo:hi], op, snap)
            base_bits, base = bases.setdefault(claim(vop), (bits.copy(), vop))
            if not np.array_equal(bits, base_bits):
                raise OpMismatch(f"{op['name']}: cfg {ch['cfg']} family {ch['family']} ({ch['label']}) differs in bits from "
                                   f"cfg {base['cfg']} family {base['family']} ({base['label']}) in the same arithmetic")
            variants["checked"] += 1


def rejects(op, mode, got, before, snap, rms_fp32, K_eff=None):
    """the GPU tests' verdict on what an implementation left in the arena (value bound and containment: check_op; the RMS rule against
    rms_fp32, the interpreter's fp32 figure): True = rejected. The teeth tests apply it to seeded mistakes"""
    try:
        _, q = check_op(op, mode, got, before, snap, K_eff)
    except OpMismatch:
        return True
    return rms_rule_applies(effective(op, K_eff), mode) and not rms_rule_ok(rms(q), rms_fp32)
