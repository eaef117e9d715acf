#!/usr/bin/env python3
"""Compare the gfx950 machine code of named kernels between two builds of libdemucs_hip.so (no GPU needed).

  tools/kernel_isa_diff.py OLD.so NEW.so --same REGEX --fp REGEX > profiles/NAME.txt

Kernels whose (demangled) name matches --same must have the identical instruction sequence (mnemonics and operands; branch
targets and addresses are left out, since they move with the code). Kernels matching --fp must have the same multiset of
floating-point instructions (v_*_f32, v_fma*, v_div_*, v_rcp*, v_cvt_f32_*), no scratch, the same LDS and a VGPR count in the
same occupancy step; their other differences are listed. Exit status 1 when a rule is broken. The code objects are cut out of
the library the way tests/test_isa_rules.py does it."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from test_isa_rules import OBJDUMP, code_objects  # noqa: E402

READELF = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")
FP = re.compile(r"^(v_\w*_f32\w*|v_fma\w*|v_div_\w+|v_rcp\w*|v_cvt_f32_\w+)$")


def kernels(lib):
    """{demangled name: (instructions, {vgpr, scratch, lds})} of every kernel of the library"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for i, co in enumerate(code_objects(lib)):
            f = os.path.join(d, f"co{i}.co")
            open(f, "wb").write(co)
            notes = subprocess.run([READELF, "--notes", f], capture_output=True, text=True, check=True).stdout
            meta = {}
            for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
                g = lambda k: re.search(rf"\.{k}:\s*(\S+)", blk).group(1)  # noqa: E731
                meta[g("name")] = {"vgpr": int(g("vgpr_count")), "sgpr": int(g("sgpr_count")), "scratch": int(g("private_segment_fixed_size")),
                                   "lds": int(g("group_segment_fixed_size"))}
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", f], capture_output=True, text=True,
                                  check=True).stdout
            for m in re.finditer(r"^<?(\S+?)>?:\n((?:[ \t]+.*\n|\n)+)", text, flags=re.M):
                sym = m.group(1).lstrip("0123456789abcdef <").rstrip(">")
                if sym not in meta:
                    continue
                ins = []
                for line in m.group(2).splitlines():
                    line = line.split("//")[0].strip()
                    if not line or line.startswith("s_nop") or line.startswith("s_code_end"):
                        continue
                    ins.append(re.sub(r"\b(s_c?branch\w*|s_call\w*)\s.*", r"\1", line))
                name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip() or sym
                out[name] = (ins, meta[sym])
    return out


def occupancy(vgpr):
    """waves per SIMD that a VGPR count allows on CDNA3/4 (512 registers, granule 8, at most 8 waves)"""
    return min(8, 512 // max(8, -(-vgpr // 8) * 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--same", required=True)
    ap.add_argument("--fp", required=True)
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    bad = 0
    print("# kernel_isa_diff: old = parent commit's library, new = this tree's")
    for name in sorted(old):
        short = name.split("(")[0]
        if name not in new:
            if re.search(a.same, name) or re.search(a.fp, name):
                print(f"MISSING in new: {name}")
                bad += 1
            continue
        (io, mo), (in_, mn) = old[name], new[name]
        if re.search(a.fp, name):
            fo = collections.Counter(x.split()[0] for x in io if FP.match(x.split()[0]))
            fn = collections.Counter(x.split()[0] for x in in_ if FP.match(x.split()[0]))
            ok = fo == fn and mn["scratch"] == 0 and mo["lds"] == mn["lds"] and occupancy(mo["vgpr"]) == occupancy(mn["vgpr"])
            bad += not ok
            print(f"{'OK  ' if ok else 'FAIL'} fp-multiset  {short}: {len(io)} -> {len(in_)} instructions, "
                  f"{sum(fo.values())} -> {sum(fn.values())} floating-point, VGPR {mo['vgpr']} -> {mn['vgpr']} "
                  f"(waves/SIMD {occupancy(mo['vgpr'])} -> {occupancy(mn['vgpr'])}), SGPR {mo['sgpr']} -> {mn['sgpr']}, LDS {mo['lds']} -> {mn['lds']}, "
                  f"scratch {mo['scratch']} -> {mn['scratch']}")
            for k in sorted(set(fo) | set(fn)):
                if fo[k] != fn[k]:
                    print(f"       floating-point differs: {k} {fo[k]} -> {fn[k]}")
            co = collections.Counter(x.split()[0] for x in io)
            cn = collections.Counter(x.split()[0] for x in in_)
            for k in sorted(set(co) | set(cn)):
                if co[k] != cn[k]:
                    print(f"       other: {k} {co[k]} -> {cn[k]}")
        elif re.search(a.same, name):
            ok = io == in_ and mo == mn
            bad += not ok
            print(f"{'OK  ' if ok else 'FAIL'} identical    {short}: {len(io)} instructions, VGPR {mn['vgpr']}, LDS {mn['lds']}, "
                  f"scratch {mn['scratch']}")
    print(f"# {bad} rule(s) broken")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
