"""Summary of a rocprofv3 --kernel-trace run of tools/bilstm_step.py legs (one directory per leg): per kernel family the launches, the
summed kernel time and the time the family's kernels kept the device busy (union of their intervals), per step; for the persistent
recurrences also how much of that union had two of them resident at once.
usage: python tools/bilstm_trace.py STEPS DIR [DIR ...]     (STEPS: steps the traced process ran, warm-up included)"""
import csv
import glob
import os
import sys


def family(name):
    n = name.lower()
    if "lstm_persist" in n and "bwd" in n:
        return "recurrence_bwd"
    if "lstm_persist" in n:
        return "recurrence_fwd"
    if "gemm" in n or "mfma" in n:
        return "gemm"
    return "other"


def union(iv):
    tot, cur_s, cur_e = 0, None, None
    for s, e in sorted(iv):
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                tot += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    return tot + (cur_e - cur_s if cur_e is not None else 0)


def depth2(iv):
    """time with at least two intervals open"""
    ev = sorted([(s, 1) for s, _ in iv] + [(e, -1) for _, e in iv])
    depth, last, tot = 0, None, 0
    for t, d in ev:
        if depth >= 2:
            tot += t - last
        depth += d
        last = t
    return tot


def main():
    steps = float(sys.argv[1])
    for d in sys.argv[2:]:
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        rows = []
        for f in files:
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
        if not rows:
            print("%s: no kernel trace" % d)
            continue
        fams = {}
        for n, s, e in rows:
            fams.setdefault(family(n), []).append((s, e))
        print("%s: %d kernels, device busy %.2f ms/step" % (os.path.basename(d.rstrip("/")), len(rows),
                                                             union([(s, e) for _, s, e in rows]) / steps / 1e6))
        rec = fams.get("recurrence_fwd", []) + fams.get("recurrence_bwd", [])
        for f in sorted(fams):
            iv = fams[f]
            print("  %-15s %6.1f launches  sum %7.2f ms  busy %7.2f ms  mean %8.1f us" % (
                f, len(iv) / steps, sum(e - s for s, e in iv) / steps / 1e6, union(iv) / steps / 1e6,
                sum(e - s for s, e in iv) / len(iv) / 1e3))
        if rec:
            print("  recurrences: busy %.2f ms/step, two resident at once %.2f ms/step" % (union(rec) / steps / 1e6, depth2(rec) / steps / 1e6))


if __name__ == "__main__":
    main()
