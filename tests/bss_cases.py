"""The seeded cases of the BSS Eval tests (tests/test_bss_cpu.py, tests/test_gpu_bss.py): the smallest shapes at which a kernel
of csrc/bss.hip can go wrong. Sources are white noise ("corr": source 1 = 0.9 source 0 + 0.1 noise); estimates are 3-tap random
FIR mixtures of all references plus noise, so that all four error terms are non-zero.

d and dx are the largest difference between route B and route A of tests/bss_spec.py on the case, in dB over the finite
entries and, for the filters, relative to max |X|: what binary64 normal equations cost on that input. The last bits of a
BLAS result depend on its thread count (3 threads give what neither 2 nor 4 do), so each literal is the largest value over
both routes run with 1, 2, 3, 4, 6, 8 and 16 BLAS threads, unrounded, and the tests run both routes with ONE thread, which is
one of those and the same sum on every machine: reference() and route_b() below. The GPU must agree with route A within max(16 d, 1e-9 dB) and 16 dx (summation order and Cholesky
against LU are the same class of error; the factor allows for the longer trees). The literals were printed by

    python tests/bss_cases.py

which also checks the conditions the table promises, at every thread count: route B's masks equal route A's, every window
of a case that is not degenerate is finite for every kept source (at least 4 of them wherever the case has 4: "scalar",
"order512-4095" and "default-taps" have 2, 3 and 2 windows), "drop" has exactly windows 2-3 empty and source 1 NaN everywhere.
"""
import functools
import os
import sys

import numpy as np
from threadpoolctl import threadpool_limits

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bss_spec  # noqa: E402

GRAM_CHUNK = 65536  # csrc/bss_plan.h kBssGramChunk (the workspace sizes of tests/test_bss_cpu.py change with it)

#        name           J  C  L    N                 W      H      kind    d          dx
CASES = [
    ("scalar",          1, 1, 1,   100,              50,    50,    "",     1.0658141036401503e-14, 1.2737087236904106e-16),
    ("overlap",         2, 2, 5,   1000,             256,   128,   "",     1.4210854715202004e-14, 6.41493994452567e-16),
    ("order444",        6, 2, 37,  3001,             500,   500,   "",     4.263256414560601e-14, 1.3472564537799942e-15),
    ("order512-4095",   4, 2, 64,  4095,             1024,  1024,  "",     2.042810365310288e-14, 7.992191169464291e-16),
    ("order512-4096",   4, 2, 64,  4096,             1024,  1024,  "",     2.842170943040401e-14, 7.876706483954727e-16),
    ("order512-4097",   4, 2, 64,  4097,             1024,  1024,  "",     1.7763568394002505e-14, 1.3000359744984052e-15),
    ("corr",            2, 2, 16,  2000,             400,   400,   "corr", 1.8829382497642655e-13, 4.3438648278065965e-14),
    ("default-taps",    2, 2, 512, 6000,             2205,  2205,  "",     1.7763568394002505e-14, 2.1529921402333237e-15),
    ("short",           2, 2, 64,  40,               44100, 44100, "",     0.0,       0.0),
    ("drop",            3, 2, 16,  2000,             250,   250,   "drop", 2.842170943040401e-14, 1.4364169621883946e-15),
    ("chunk-1",         2, 1, 8,   GRAM_CHUNK - 1,   16000, 16000, "",     2.1316282072803006e-14, 1.234024418851153e-15),
    ("chunk+1",         2, 1, 8,   GRAM_CHUNK + 1,   16000, 16000, "",     2.4868995751603507e-14, 8.77200634150587e-16),
]
DEGENERATE = ("short", "drop")  # "short": N < L makes the basis rank deficient (order 256, 103 rows): the failure rule applies
NAMES = [c[0] for c in CASES]


def case(name):
    return CASES[NAMES.index(name)]


def signals(name):
    """(refs, ests): (J, C, N) float32"""
    _, J, C, L, N, W, H, kind, _, _ = case(name)
    rng = np.random.default_rng(NAMES.index(name) + 1)
    refs = rng.standard_normal((J, C, N))
    if kind == "corr":
        refs[1] = 0.9 * refs[0] + 0.1 * refs[1]
    if kind == "drop":
        refs[1] = 0.0
    h = 0.2 * rng.standard_normal((J, C, J, C, 3))  # estimate (i, c'') <- reference (j, c), 3 taps
    for i in range(J):
        for c in range(C):
            h[i, c, i, c, 0] += 1.0
    ests = 0.1 * rng.standard_normal((J, C, N))
    for i in range(J):
        for c in range(C):
            for j in range(J):
                for c2 in range(C):
                    ests[i, c] += np.convolve(refs[j, c2], h[i, c, j, c2])[:N]
    if kind == "drop":
        ests[0, :, 2 * W:4 * W] = 0.0
    return refs.astype(np.float32), ests.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(name):
    """route A on the case with one BLAS thread, computed once and shared"""
    _, J, C, L, N, W, H, _, _, _ = case(name)
    refs, ests = signals(name)
    with threadpool_limits(limits=1):
        return bss_spec.route_a(refs, ests, L, W, H)


def route_b(name):
    """route B on the case with one BLAS thread"""
    _, J, C, L, N, W, H, _, _, _ = case(name)
    refs, ests = signals(name)
    with threadpool_limits(limits=1):
        return bss_spec.route_b(refs, ests, L, W, H)


THREADS = (1, 2, 3, 4, 6, 8, 16)


def main():
    for name, J, C, L, N, W, H, kind, _, _ in CASES:
        refs, ests = signals(name)
        kept, d, dx, ok = bss_spec.kept_sources(refs), 0.0, 0.0, True
        for t in THREADS:
            with threadpool_limits(limits=t):
                a, b = bss_spec.route_a(refs, ests, L, W, H), bss_spec.route_b(refs, ests, L, W, H)
            dt, dxt, same = bss_spec.distance(a, b)
            d, dx = max(d, dt), max(dx, dxt)
            fin = np.isfinite(a["sdr"]) & np.isfinite(a["isr"]) & np.isfinite(a["sar"])
            ok = ok and same and (name in DEGENERATE or all(fin[j].all() and fin[j].sum() >= min(4, fin.shape[1]) for j in kept))
            if name == "drop":
                ok = ok and np.isnan(a["sdr"][1]).all() and all(np.array_equal(np.where(np.isnan(a["sdr"][j]))[0], [2, 3]) for j in kept)
        print(f"{name:15s} d {d!r}  dx {dx!r}  status {a['status']}  windows {a['sdr'].shape[1]}  conditions {'hold' if ok else 'FAIL'}")


if __name__ == "__main__":
    main()
