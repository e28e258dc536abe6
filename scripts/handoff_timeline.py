"""Copy dispatches on the solver's stream and the idle next to them, from a rocprofv3 trace taken with --kernel-trace and
--memory-copy-trace (rocpd database).  scripts/timeline.py reads kernels only; this one merges the memory copies in.

    python scripts/handoff_timeline.py <results.db> --paths N [--top K]

The stream with the most kernels is the solver's.  Its kernels and every memory copy recorded on it are put on one time axis.  A
copy is named by direction and size class (H2D<=64B, D2H<=128KB, ...); a runtime blit kernel (__amd_rocclr_*) that lies inside a
recorded copy is that copy and is dropped.  Printed, per path (totals / N): copy dispatches, their busy time, the idle next to a
copy by (previous -> next) pair, the idle at pass openings (a gap that ends at la_open_kernel, gather_i32_kernel or a strip
kernel: reported apart), and the remaining idle.  Gaps above 5 ms are python between paths and are left out.
"""
import re
import sqlite3
import sys
from collections import defaultdict

OPENERS = ("la_open_kernel", "gather_i32_kernel", "strip_lt_kernel", "strip_reduce_kernel")


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    m = re.match(r"(?:void )?(?:ahip::)?([A-Za-z_0-9:]+)", name)
    return (m.group(1) if m else name)[:40]


def size_class(b):
    for lim, tag in ((64, "<=64B"), (1024, "<=1KB"), (16384, "<=16KB"), (131072, "<=128KB"), (1 << 20, "<=1MB")):
        if b <= lim:
            return tag
    return ">1MB"


def copy_name(name, size):
    n = name.upper()
    d = "H2D" if "HOST_TO_DEVICE" in n else "D2H" if "DEVICE_TO_HOST" in n else "D2D" if "DEVICE_TO_DEVICE" in n else "H2H" if "HOST_TO_HOST" in n else name[-12:]
    return f"copy:{d}{size_class(size)}"


def is_copy(n):
    return n.startswith("copy:") or n.startswith("__amd_rocclr_")


def main():
    db = sys.argv[1]
    npaths = int(sys.argv[sys.argv.index("--paths") + 1]) if "--paths" in sys.argv else 1
    top = int(sys.argv[sys.argv.index("--top") + 1]) if "--top" in sys.argv else 30
    c = sqlite3.connect(db)
    kern = [(short(n), s, e, q) for n, s, e, q in c.execute("select name, start, end, stream_id from kernels order by start")]
    if not kern:
        print("no kernels")
        return
    cnt = defaultdict(int)
    for k in kern:
        cnt[k[3]] += 1
    main_s = max(cnt, key=cnt.get)
    print("# kernels per stream:", dict(cnt), "; solver stream =", main_s)
    try:
        cps = list(c.execute("select name, start, end, stream_id, size from memory_copies order by start"))
    except sqlite3.OperationalError as ex:
        print("# no memory_copies view:", ex)
        cps = []
    ccnt = defaultdict(int)
    for r in cps:
        ccnt[r[3]] += 1
    print("# memory copies per stream:", dict(ccnt))
    copies = [(copy_name(n, sz), s, e, sz) for n, s, e, q, sz in cps if q == main_s]
    ks = [(n, s, e, 0) for n, s, e, q in kern if q == main_s]
    # a blit kernel inside a recorded copy is that copy
    ev, ci, dropped = [], 0, 0
    for k in ks:
        if k[0].startswith("__amd_rocclr_"):
            while ci < len(copies) and copies[ci][2] < k[1]:
                ci += 1
            j, hit = ci, False
            while j < len(copies) and copies[j][1] <= k[1]:
                if copies[j][2] >= k[2]:
                    hit = True
                    break
                j += 1
            if hit:
                dropped += 1
                continue
        ev.append(k)
    ev += copies
    ev.sort(key=lambda r: r[1])
    print(f"# {len(ks)} kernels and {len(copies)} copies on the solver stream; {dropped} blit kernels counted as their copy; /{npaths} paths")

    busy = defaultdict(lambda: [0, 0.0, 0])
    for n, s, e, sz in ev:
        b = busy[n]
        b[0] += 1
        b[1] += (e - s) / 1e3
        b[2] += sz
    pair = defaultdict(lambda: [0, 0.0])
    idle = {"copy": 0.0, "open": 0.0, "other": 0.0}
    last_end, last_name = ev[0][2], ev[0][0]
    for n, s, e, _ in ev[1:]:
        g = (s - last_end) / 1e3
        if 0 < g <= 5000:
            kind = "open" if n in OPENERS else "copy" if (is_copy(n) or is_copy(last_name)) else "other"
            idle[kind] += g
            if kind != "other":
                pr = pair[(kind, last_name, n)]
                pr[0] += 1
                pr[1] += g
        if e > last_end:
            last_end, last_name = e, n
    P = float(npaths)
    ncopy = sum(b[0] for n, b in busy.items() if is_copy(n))
    tcopy = sum(b[1] for n, b in busy.items() if is_copy(n))
    print(f"\nper path: copy dispatches {ncopy / P:.0f}, copy busy {tcopy / 1e3 / P:.2f} ms, idle next to a copy {idle['copy'] / 1e3 / P:.2f} ms,"
          f" idle at pass openings {idle['open'] / 1e3 / P:.2f} ms, other idle {idle['other'] / 1e3 / P:.2f} ms")
    print(f"per path: copy busy + copy-adjacent idle = {(tcopy + idle['copy']) / 1e3 / P:.2f} ms")
    print("\n# copies by kind (per path: count, busy ms, bytes)")
    for n, b in sorted(busy.items(), key=lambda kv: -kv[1][1]):
        if is_copy(n):
            print(f"  {n:>40s} {b[0] / P:8.1f}  {b[1] / 1e3 / P:8.3f} ms  {b[2] / P:12.0f} B")
    for kind, title in (("copy", "idle next to a copy"), ("open", "idle at pass openings (out of scope)")):
        print(f"\n# {title}, by (previous -> next), per path, top {top}")
        rows = [(k, v) for k, v in pair.items() if k[0] == kind]
        for (_, a, b), (cn, g) in sorted(rows, key=lambda kv: -kv[1][1])[:top]:
            print(f"  {a:>36s} -> {b:<36s} {cn / P:7.1f} gaps  {g / 1e3 / P:7.3f} ms  avg {g / cn:7.1f} us")
    print("\n# busy by kernel on the solver stream (per path)")
    for n, b in sorted(busy.items(), key=lambda kv: -kv[1][1])[:16]:
        if not is_copy(n):
            print(f"  {n:>40s} {b[0] / P:8.1f}  {b[1] / 1e3 / P:8.3f} ms")


if __name__ == "__main__":
    main()
