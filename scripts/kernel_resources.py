#!/usr/bin/env python3
"""Per-instance register, scratch and LDS figures of named kernels, from the compiler's resource remarks.

Build with the remarks on and keep the log, then name the kernels:

    make -C customknowledgegraphembedding_amd clean
    make -C customknowledgegraphembedding_amd -j16 -O \\
        HIPFLAGS="<the Makefile's HIPFLAGS> -Rpass-analysis=kernel-resource-usage" 2> build.log
    python scripts/kernel_resources.py build.log rank_sweep_kernel rank_pairs_kernel

(-O keeps each unit's remarks together: interleaved remarks of parallel units cannot be told apart.)

One line per instance: kernel, template arguments as mangled (FN, CH, V, G, ...), VGPRs, AGPRs, scratch bytes per
lane, spilled VGPRs, static LDS bytes (dynamic LDS is the launch's and not in the remarks), waves per SIMD, and with
--sgprs the total SGPRs. Exits 1
when an instance with G <= 4 has scratch or spills (--max-g changes the bound)."""
import argparse
import re
import sys

FN_NAMES = {0: "TransE", 1: "DistMult", 2: "ComplEx", 3: "RotatE", 4: "InterHT", 5: "pRotatE", 7: "PairRE"}


def parse(path):
    """{mangled name: {field: int}} from the remarks (a kernel compiled in several units appears once)."""
    out, cur = {}, None
    # the remark's text follows "remark: " directly or after the kernel's source position (file:line:column:)
    name_re = re.compile(r"remark: (?:\S+:\d+:\d+: )?Function Name: (\S+)")
    field_re = re.compile(r"remark:\s+(?:\S+:\d+:\d+:\s+)?([A-Za-z][A-Za-z /\[\]]*?):\s+(\d+)")
    for line in open(path, errors="replace"):
        m = name_re.search(line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = field_re.search(line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def template_args(mangled):
    """The integer / bool template arguments of a mangled kernel name, in order."""
    m = re.search(r"I((?:L[ib]\d+E)+)E", mangled)
    return [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1))] if m else []


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("log")
    ap.add_argument("kernels", nargs="+")
    ap.add_argument("--max-g", type=int, default=4, help="instances up to this G must not spill")
    ap.add_argument("--sgprs", action="store_true", help="a last column with the total SGPRs")
    a = ap.parse_args()
    res = parse(a.log)
    bad = 0
    print("kernel fn ch V G rest | VGPRs AGPRs scratch_B/lane vgpr_spill static_LDS_B waves/SIMD"
          + (" SGPRs" if a.sgprs else ""))
    rows = []
    for mangled, f in res.items():
        for k in a.kernels:
            if re.search(r"\d+%s(I|E|v)" % re.escape(k), mangled):
                t = template_args(mangled)
                rows.append((k, t, f))
    for k, t, f in sorted(rows, key=lambda r: (r[0], r[1])):
        fn, ch, v, g = (t + [0, 0, 0, 0])[:4]
        scratch, spill = f.get("ScratchSize [bytes/lane]", -1), f.get("VGPRs Spill", -1)
        flag = ""
        if g <= a.max_g and (scratch != 0 or spill != 0):
            bad += 1
            flag = "  <-- spills"
        print(f"{k} {FN_NAMES.get(fn, fn)} {'head' if ch else 'tail'} V{v} G{g} {t[4:]} | {f.get('VGPRs', -1)} "
              f"{f.get('AGPRs', -1)} {scratch} {spill} {f.get('LDS Size [bytes/block]', -1)} "
              f"{f.get('Occupancy [waves/SIMD]', -1)}{' %d' % f.get('TotalSGPRs', -1) if a.sgprs else ''}{flag}")
    print(f"{len(rows)} instances, {bad} spilling at G <= {a.max_g}")
    return 1 if bad or not rows else 0


if __name__ == "__main__":
    sys.exit(main())
