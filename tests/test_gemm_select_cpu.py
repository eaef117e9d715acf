"""The kernel selection of the per-segment executor (demucs_cpp_amd/csrc/gemm_select.cpp: which kernel runs an OP_IGEMM, decided once
per plan on the host) by brute force over models, segment lengths, batch sizes, GEMM modes and the values of the exact-split A/B
switch, through tests/cpu_interp.cpp. No GPU: that every family computes the bits of its arithmetic is what the GPU suite checks."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "_build", "libcpu_interp.so")

F32, BF16X3, FP16X3 = 0, 1, 2
EPI_LINEAR, EPI_TRCONV, EPI_KPL, EPI_VT = 0, 5, 7, 8
# plan.h GemmFamily
NONE, DIRECT, TILE, LIN256, STAGED, STAGED_LIN, LIN, LINH, LINW, WIDE_CONV, NARROW = range(11)
SPLIT = (STAGED, STAGED_LIN, LIN, LINH, LINW, WIDE_CONV, NARROW)
SEGS = {4: (6000, 10000, 343980), 6: (6000, 343980), 3: (6000, 20000, 343980)}  # 10000 / 6000 / 20000: the golden segments
BATCHES = (1, 2, 6, 8, 42)
LABELS = {"dgemm_direct", "igemm_lin256x128", "igemm_splith_128x128", "igemm_splith_64x128", "igemm_split_128x256", "igemm_split_128x192",
          "igemm_split_128x96d", "igemm_split_128x64d", "igemm_split_128x32d"} | {
    f"igemm{s}_{t}" for s, ts in (("", "128x128 64x64 128x96 128x48 256x16 128x32 128x64 64x128 64x96 64x48 64x32 128x16 32x128 32x64 256x96"),
                                   ("_split", "128x128 128x96 128x48 64x128 64x64 64x96 64x48 32x128 32x64")) for t in ts.split()}


@pytest.fixture(scope="module")
def interp():
    srcs = [os.path.join(ROOT, "tests", "cpu_interp.cpp")] + [os.path.join(ROOT, "demucs_cpp_amd", "csrc", f)
                                                              for f in ("plan.cpp", "plan.h", "model_pack.cpp", "gemm_select.cpp", "gemm_select.h", "gemm_tiles.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["make", "-C", ROOT, "interp"], stdout=subprocess.DEVNULL)
    L = ctypes.CDLL(SO)
    L.interp_create_plan.restype = ctypes.c_void_p
    L.interp_create_plan.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int]
    L.interp_free.argtypes = [ctypes.c_void_p]
    L.interp_select_dump.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int] * 3 + [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    L.interp_select_one.argtypes = [ctypes.c_void_p, ctypes.c_char_p] + [ctypes.c_int] * 8 + [ctypes.c_char_p, ctypes.c_int]
    L.interp_tiles.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.interp_direct_probe.argtypes = [ctypes.c_int] * 6
    return L


def parse(text):
    ops = []
    for ln in text.splitlines():
        name, cfg, epi, ht, fam, arith, wnf, label, exists = ln.split()
        ops.append(dict(name=name, cfg=int(cfg), epi=int(epi), hterms=int(ht), family=int(fam), arith=int(arith), wnf=int(wnf), label=label,
                        exists=int(exists)))
    return ops


def dump(L, h, seg, b, gemm, lin, inexact=""):
    buf = ctypes.create_string_buffer(1 << 18)
    n = L.interp_select_dump(h, seg, b, gemm, lin, inexact.encode(), buf, 1 << 18)
    assert n > 0, n  # (-3: a second call of the selection gave another choice)
    return parse(buf.value.decode())


def one(L, h, name, gemm, lin=1, cfg=-2, epi=-2, N=-2, Np=-2, res=-2, rowstat=-2):
    buf = ctypes.create_string_buffer(1024)
    assert L.interp_select_one(h, name.encode(), gemm, lin, cfg, epi, N, Np, res, rowstat, buf, 1024) > 0
    return parse(buf.value.decode())[0]


@pytest.mark.parametrize("ns", [4, 6, 3])
def test_every_op_gets_one_choice_with_one_arithmetic(ns, interp, tmp_models):
    arith_of = {}  # (segment, GEMM mode, op name) -> arithmetic: the same at every batch size and switch value
    seen = set()
    h = interp.interp_create_plan(tmp_models[ns].encode(), 6000, 1)  # (the model; the selection plans every case itself)
    assert h
    for seg in SEGS[ns]:
        for b in BATCHES:
            for gemm in (F32, BF16X3, FP16X3):
                for lin in range(5):
                    ops = dump(interp, h, seg, b, gemm, lin)  # every OP_IGEMM has a line: exactly one choice, the same when asked again
                    assert len({o["name"] for o in ops}) == len(ops) > 20
                    for o in ops:
                        where = (seg, b, gemm, lin, o)
                        assert o["family"] != NONE and o["label"] in LABELS, where
                        assert o["exists"], where  # the chosen kernel is compiled and its launcher takes the op (gemm_kernel_exists)
                        assert (o["arith"] != 0) == (o["family"] in SPLIT), where
                        assert (o["family"] == DIRECT) == (o["cfg"] == 8) or o["arith"], where
                        if gemm == F32:
                            assert o["family"] in (DIRECT, TILE, LIN256), where
                        assert (o["arith"] == 2) == (o["family"] == LINH), where
                        if o["arith"] == 2:
                            assert gemm == FP16X3 and o["hterms"], where
                        if o["epi"] in (EPI_KPL, EPI_VT):
                            assert o["family"] in (LIN, LINH, LINW), where
                        if o["arith"] and o["cfg"] in (5, 12):
                            assert o["label"] == "igemm_split_128x32d" and o["family"] == NARROW and o["wnf"] == 2, where
                        if o["arith"] and o["cfg"] in (6, 13):
                            assert o["label"] == "igemm_split_128x64d" and o["family"] == NARROW and o["wnf"] == 4, where
                        assert arith_of.setdefault((seg, gemm, o["name"]), o["arith"]) == o["arith"], where
                        seen.add(o["family"])
    interp.interp_free(h)
    want = set(SPLIT) | {DIRECT, TILE}
    if ns == 3:  # no transformer: no linear-layer kernels, no operand planes
        want -= {LIN, LINH, LINW, STAGED_LIN}
    assert want <= seen, want - seen


@pytest.mark.parametrize("ns", [4, 6])
def test_inexact_weights_of_one_plane_projection_remove_all_of_them(ns, interp, tmp_models):
    h = interp.interp_create_plan(tmp_models[ns].encode(), 6000, 1)
    for b in (1, 42):
        for gemm in (BF16X3, FP16X3):
            ops = dump(interp, h, 343980, b, gemm, 1)
            planes = [o for o in ops if o["epi"] in (EPI_KPL, EPI_VT)]
            assert len(planes) >= 10
            rebuilt = dump(interp, h, 343980, b, gemm, 1, inexact=planes[3]["name"])
            assert not [o for o in rebuilt if o["epi"] in (EPI_KPL, EPI_VT)]
            # the fp32-K/V form names its projections otherwise (qkv / kv): the one that reads the marked weights keeps fp32
            assert all(o["arith"] for o in ops if o["name"].startswith("crosstransformer."))
            assert [o for o in rebuilt if o["name"].startswith("crosstransformer.") and o["arith"] == 0]
        assert not [o for o in dump(interp, h, 343980, b, F32, 1) if o["epi"] in (EPI_KPL, EPI_VT)]
    interp.interp_free(h)


def test_narrow_split_tiles_refuse_residuals_and_row_statistics(interp, tmp_models, monkeypatch):
    """Hand-made ops on the narrow tile cfgs (5 / 12: 32 columns, 6 / 13: 64): the direct-fragment kernel has no residual operand on
    its linear epilogue and row statistics only in its 32-wide linear form, so such ops keep their fp32 kernel - decided from the
    plan's fields (an earlier form asked the launcher with null placeholder pointers and labelled them split)."""
    monkeypatch.setenv("DMX_INTERP_GEMM", "1")  # the handle's plan as a split context lays it out
    h = interp.interp_create_plan(tmp_models[4].encode(), 343980, 42)
    ops = dump(interp, h, 343980, 42, BF16X3, 1)
    k1 = next(o for o in ops if o["family"] == NARROW and o["epi"] == EPI_LINEAR)  # a DConv K1 of the C = 192 levels
    tr = next(o for o in ops if o["family"] == NARROW and o["epi"] == EPI_TRCONV)  # the frequency branch's last transposed conv
    for gemm in (BF16X3, FP16X3):
        for lin in range(5):
            for cfg, np_ in ((5, 32), (12, 32), (6, 64), (13, 64)):
                kw = dict(gemm=gemm, lin=lin, cfg=cfg, Np=np_)
                assert one(interp, h, k1["name"], rowstat=-1, res=-1, **kw)["family"] == NARROW  # the base case is one the kernel takes
                o = one(interp, h, k1["name"], rowstat=-1, res=64, **kw)
                assert o["family"] == TILE and o["arith"] == 0 and not o["label"].startswith("igemm_split") and o["exists"], o
                o = one(interp, h, k1["name"], rowstat=64, res=-1, **kw)
                assert (o["family"] == NARROW) == (np_ == 32) and o["exists"], o
            for cfg in (6, 13):
                assert one(interp, h, tr["name"], gemm=gemm, lin=lin, cfg=cfg, rowstat=-1)["family"] == NARROW
                o = one(interp, h, tr["name"], gemm=gemm, lin=lin, cfg=cfg, rowstat=64)
                assert o["family"] == TILE and o["arith"] == 0 and o["exists"], o
            for cfg in (5, 12):  # no transposed-conv form at 32 columns
                o = one(interp, h, tr["name"], gemm=gemm, lin=lin, cfg=cfg, N=32, Np=32, rowstat=-1)
                assert o["family"] == TILE and o["exists"], o
    interp.interp_free(h)


def test_labels_are_the_tile_tables(interp):
    """LABELS above is a hand-written pin: the labels the tile table (csrc/gemm_tiles.h) can produce - the fp32 and the exact-split
    label of every tile that has a kernel - plus the labels of the kernels no tile cfg stands for."""
    buf = ctypes.create_string_buffer(1 << 14)
    assert interp.interp_tiles(buf, 1 << 14) > 0
    rows = [ln.split() for ln in buf.value.decode().splitlines()]
    assert [int(r[0]) for r in rows] == list(range(21))
    table = {lab for r in rows if int(r[8]) != 0 for lab in r[9:11] if lab != "-"}
    split_only = {"igemm_splith_128x128", "igemm_splith_64x128", "igemm_split_128x256", "igemm_split_128x192", "igemm_split_128x96d"}
    assert not table & split_only
    assert table | split_only == LABELS


def test_direct_kernel_list_has_one_meaning(interp):
    """One list, two users: over a brute-force sweep of shapes, the rule that sends an op of an fp32 plan to the direct kernels
    (choose_tile) and the existence answer for the direct kernel (gemm_kernel_exists) agree - both read DMX_DIRECT_COMBOS and the
    column-chunk rule of csrc/gemm_tiles.h. Column fragments 24 and 48 (N = 384, 768) reach the chunk rule."""
    PRO_NONE, PRO_GN_GELU = 0, 2
    EPI_GN_GLU_SCALE_RES = 3
    routed = set()
    for nf in list(range(1, 13)) + [24, 48]:
        for s1 in (1, 3):
            for seg0 in (8, 12, 16, 24, 32, 48, 96):
                for pro in range(3):
                    for epi in range(9):
                        for res in (0, 1):
                            for n in (16 * nf, 16 * nf - 4):  # a full and a partly filled last fragment
                                r = interp.interp_direct_probe(n, s1, seg0, pro, epi, res)
                                assert r in (0, 3), (n, s1, seg0, pro, epi, res, r)
                                if r:
                                    routed.add((nf, s1, seg0, pro, epi))
                                    assert not (res and epi in (EPI_LINEAR, EPI_TRCONV))  # no residual operand on these epilogues
    chunked = {(nf, 1, seg0, PRO_GN_GELU, EPI_GN_GLU_SCALE_RES) for nf in (24, 48) for seg0 in (24, 48)}
    assert chunked <= routed and len(routed - chunked) == 18  # every row of the list and of the chunk rule, and nothing else
    assert (1, 3, 48, PRO_NONE, EPI_LINEAR) in routed and (6, 1, 48, PRO_NONE, 2) in routed
