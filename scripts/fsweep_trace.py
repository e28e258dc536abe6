"""Per-piece device times of the filtered invariance sweep from a rocprofv3 kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python bench.py --gpus 1 --config 2 --steps 3 --warmup 1
    python scripts/fsweep_trace.py DIR

A filtered sweep is the run of dispatches that starts at vmul_sq_kernel and ends at the last sweep_list_kernel before a
dispatch of another family.  Of the list sweeps of one run the last is the open list's (it follows the classification and
reads its count from the device), the earlier ones are the screen columns' and the unpenalised columns'.  A 16-byte fill
right before vmul_sq_kernel is the memset of the meta words."""
import csv
import glob
import statistics
import sys

FAMILY = ("shadow_sweep_kernel", "sweep_reduce_kernel", "filter_classify_kernel", "sweep_list_kernel", "sweep_list_reduce_kernel")


def piece(name):
    """The family a dispatch is listed under; the shadow launch by the kind of copy in its template arguments."""
    k = next(k for k in FAMILY if k in name)
    if k == "shadow_sweep_kernel":
        return k + (", q15" if "ShadowQ15" in name else ", float32" if "ShadowF32" in name else "")
    return k


def main(d):
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
    rows = []
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    pieces = {}
    spans, idle = [], []
    full = []
    i = 0
    while i < len(rows):
        s, e, name = rows[i]
        if "sweep_kernel<double" in name and "false" in name and "shadow" not in name and e - s > 500000:
            full.append(e - s)
        if "vmul_sq_kernel" not in name:
            i += 1
            continue
        if i > 0 and "fillBuffer" in rows[i - 1][2] and s - rows[i - 1][1] < 200000:
            pieces.setdefault("memset (fillBuffer)", []).append(rows[i - 1][1] - rows[i - 1][0])
        pieces.setdefault("vmul_sq_kernel", []).append(e - s)
        j = i + 1
        lists = []
        busy = e - s
        last_end = e
        while j < len(rows) and any(k in rows[j][2] for k in FAMILY):
            s2, e2, n2 = rows[j]
            busy += e2 - s2
            last_end = e2
            if "sweep_list_kernel" in n2:
                lists.append(e2 - s2)
            else:
                pieces.setdefault(piece(n2), []).append(e2 - s2)
            j += 1
        if lists:
            pieces.setdefault("sweep_list_kernel, open list", []).append(lists[-1])
            for t in lists[:-1]:
                pieces.setdefault("sweep_list_kernel, screen / unpenalised", []).append(t)
        spans.append(last_end - s)
        idle.append(last_end - s - busy)
        i = j
    print("filtered sweeps: %d" % len(spans))
    for k, v in pieces.items():
        print("  %-42s calls %5d  avg %8.1f us  median %8.1f  min %8.1f  max %8.1f" % (
            k, len(v), statistics.mean(v) / 1e3, statistics.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3))
    if spans:
        print("  vmul_sq start -> end of the open-list sweep: avg %.1f us, median %.1f us; of it between dispatches: avg %.1f us" % (
            statistics.mean(spans) / 1e3, statistics.median(spans) / 1e3, statistics.mean(idle) / 1e3))
    if full:
        print("full sweep_kernel (f64, all columns): calls %d avg %.1f us" % (len(full), statistics.mean(full) / 1e3))


if __name__ == "__main__":
    main(sys.argv[1])
