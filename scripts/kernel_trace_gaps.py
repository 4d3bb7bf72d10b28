"""From a `rocprofv3 --kernel-trace --output-format csv` directory: the average duration of one
kernel's dispatches and the average gap between consecutive ones (begin(i+1) - end(i)).

  python scripts/kernel_trace_gaps.py DIR [--kernel unpack_kernel<1, 0>] [--last 50] [--json OUT]

The last `--last` dispatches are taken (the timed steps of a bench.py run come last among the
headline kernel's launches); one JSON line is printed.
"""
import argparse, csv, glob, json, os, statistics


def dispatches(d, kernel):
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if kernel in r["Kernel_Name"].replace(", ", ",").replace(",", ", "):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    return rows


def summarise(rows, last):
    rows = rows[-last:] if last else rows
    dur = [e - b for b, e in rows]
    gaps = [rows[i + 1][0] - rows[i][1] for i in range(len(rows) - 1)]
    out = {"launches": len(rows)}
    if dur:
        out.update(avg_kernel_us=round(statistics.mean(dur) / 1e3, 3),
                   min_kernel_us=round(min(dur) / 1e3, 3), max_kernel_us=round(max(dur) / 1e3, 3))
    if gaps:
        out.update(avg_gap_us=round(statistics.mean(gaps) / 1e3, 3),
                   median_gap_us=round(statistics.median(gaps) / 1e3, 3),
                   max_gap_us=round(max(gaps) / 1e3, 3),
                   avg_period_us=round((rows[-1][0] - rows[0][0]) / (len(rows) - 1) / 1e3, 3))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--kernel", default="unpack_kernel<1, 0>")
    ap.add_argument("--last", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = summarise(dispatches(a.dir, a.kernel), a.last)
    res["kernel"] = a.kernel
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
