#!/usr/bin/env python3
"""Per-kernel resource figures from hipcc's -Rpass-analysis=kernel-resource-usage report, and the
comparison of two builds (a cross-compile: no GPU needed).

    hipcc $(make -s print-HIPFLAGS) -shared -o /tmp/a.so pathtracercuda_amd/csrc/pt_kernels.hip -lrccl \\
          -Rpass-analysis=kernel-resource-usage 2> new.txt          # the same on the other tree: old.txt
    python tools/kernel_usage.py new.txt [--against old.txt] [--out profiles/NAME.json]

With --against: every kernel of the old report must have identical figures in the new one (exit 1 otherwise);
the kernels only the new report has are listed with their figures.
"""
import argparse
import hashlib
import json
import re
import subprocess
import sys


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s*Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[-Rpass-analysis", line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def table_hash(table):
    """sha256 of the whole table (mangled name -> figures, keys sorted): a build of the same tree prints the same one
    (`python tools/kernel_usage.py report.txt` shows it as table_sha256), so a recorded comparison can be re-checked."""
    return hashlib.sha256(json.dumps(table, sort_keys=True).encode()).hexdigest()


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("report")
    ap.add_argument("--against")
    ap.add_argument("--out")
    ap.add_argument("--against-label", help="what the --against report is of (a commit id and how it was made)")
    a = ap.parse_args()
    new = parse(a.report)
    record = {"kernels": len(new), "table_sha256": table_hash(new)}
    rc = 0
    if a.against:
        old = parse(a.against)
        changed = sorted(k for k in old if old[k] != new.get(k))
        added = sorted(k for k in new if k not in old)
        names = demangle(added + changed)
        if a.against_label:
            record["parent_report"] = a.against_label
        record.update(parent_kernels=len(old), parent_table_sha256=table_hash(old), parent_trace_kernel_instantiations=sum("trace_kernel" in k for k in old),
                      parent_kernels_with_other_figures=[names[k] for k in changed],
                      new_kernels={names[k]: new[k] for k in added})
        rc = 1 if changed else 0
    else:
        names = demangle(sorted(new))
        record["figures"] = {names[k]: new[k] for k in sorted(new)}
    text = json.dumps(record, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)
    sys.exit(rc)


if __name__ == "__main__":
    main()
