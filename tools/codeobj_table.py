#!/usr/bin/env python3
"""Per-kernel resource table of a build, from the compiler's own remarks.

Compile the library with `-Rpass-analysis=kernel-resource-usage` added to HIPFLAGS of __graft_entry__.py and keep stderr:

    hipcc <HIPFLAGS> -Rpass-analysis=kernel-resource-usage csrc/fv3_api.hip -o lib.so 2> build.log
    python tools/codeobj_table.py build.log profiles/codeobj_<build_id>.csv
    python tools/codeobj_table.py --diff profiles/codeobj_A.csv profiles/codeobj_B.csv

The table has one row per kernel: demangled name, SGPRs, VGPRs, AGPRs, scratch bytes per lane, occupancy (waves per SIMD), SGPR and
VGPR spills, LDS bytes per block.  --diff lists every kernel present in both tables whose row differs and the kernels only one of
them has; exit status 1 if a common kernel differs."""
import csv
import re
import subprocess
import sys

FIELDS = [("TotalSGPRs", "sgprs"), ("VGPRs", "vgprs"), ("AGPRs", "agprs"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("SGPRs Spill", "sgpr_spill"), ("VGPRs Spill", "vgpr_spill"),
          ("LDS Size [bytes/block]", "lds")]
COLS = ["kernel"] + [c for _, c in FIELDS]


def parse(log):
    rows, cur = {}, None
    pat = re.compile(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis")
    for line in open(log, errors="replace"):
        m = pat.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = rows.setdefault(val, {})
        elif cur is not None:
            for name, col in FIELDS:
                if key == name:
                    cur[col] = val
    names = list(rows)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n") if names else []
    return {(dem[i] if i < len(dem) and dem[i] else n): rows[n] for i, n in enumerate(names)}


def load(path):
    return {r["kernel"]: r for r in csv.DictReader(open(path))}


def main(argv):
    if len(argv) == 4 and argv[1] == "--diff":
        a, b = load(argv[2]), load(argv[3])
        changed = [k for k in a if k in b and any(a[k][c] != b[k][c] for c in COLS[1:])]
        for k in changed:
            print("CHANGED", k, {c: (a[k][c], b[k][c]) for c in COLS[1:] if a[k][c] != b[k][c]})
        only_a, only_b = [k for k in a if k not in b], [k for k in b if k not in a]
        for k in only_a:
            print("ONLY IN", argv[2], k)
        for k in only_b:
            print("ONLY IN", argv[3], k)
        print(f"{len(a)} / {len(b)} kernels, {len(a) - len(only_a)} in both, {len(changed)} of them changed, "
              f"{len(only_a)} / {len(only_b)} in one only")
        return 1 if changed else 0
    if len(argv) != 3:
        sys.exit(__doc__)
    rows = parse(argv[1])
    with open(argv[2], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(COLS)
        for k in sorted(rows):
            w.writerow([k] + [rows[k].get(c, "") for c in COLS[1:]])
    print(f"{argv[2]}: {len(rows)} kernels")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
