#!/usr/bin/env python3
"""Per-dispatch k_huff times of the last headline step in a rocprofv3 kernel
trace (scripts/huff_trace.sh): the step's `n` trial launches in order (probe
launch, then the search launches, per sub-batch) and the step's totals per
kernel.  usage: huff_trace.py <kernel_trace.csv> [n = 12]"""
import csv
import sys
from collections import defaultdict


def short(name):
    for k in ("k_huff", "k_fdct_color", "k_fdct_gray", "k_list_count", "k_scan", "k_ffscan", "k_stuff", "k_resize"):
        if k in name:
            return k
    return None


def main():
    path, n = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 12
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            k = short(r["Kernel_Name"])
            if k:
                grid = "x".join(r.get(f"Grid_Size_{a}", "?") for a in "XYZ")
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k, grid))
    rows.sort()
    huff = [i for i, r in enumerate(rows) if r[2] == "k_huff"]
    if len(huff) < n:
        sys.exit(f"only {len(huff)} k_huff dispatches in {path}")
    first = huff[-n]
    while first > 0 and rows[first][2] != "k_fdct_color":  # the step starts with its first sub-batch's FDCT
        first -= 1
    step = rows[first:]
    print(f"last step: {len(step)} dispatches, {(step[-1][1] - step[0][0]) / 1e6:.3f} ms from first start to last end")
    print("k_huff dispatches (us, grid):")
    for i in huff[-n:]:
        s, e, _, grid = rows[i]
        print(f"  +{(s - step[0][0]) / 1e3:9.1f} us  {(e - s) / 1e3:8.1f} us  grid {grid}")
    tot, cnt = defaultdict(int), defaultdict(int)
    for s, e, k, _ in step:
        tot[k] += e - s
        cnt[k] += 1
    print("per kernel (ms, launches):")
    for k in sorted(tot, key=tot.get, reverse=True):
        print(f"  {k:14s} {tot[k] / 1e6:8.3f} ms  {cnt[k]:3d}")
    busy = sum(tot.values()) / 1e6
    print(f"  {'all':14s} {busy:8.3f} ms")


if __name__ == "__main__":
    main()
