"""Durations of a named kernel and the idle gaps between its consecutive launches, from a rocprofv3 kernel-trace CSV (parse only; CPU).
Usage: python tools/launch_gaps.py <kernel_trace.csv> <substring of the kernel's name> [--max-gap-us 1000] [--skip N] [--last N] [--beside SUBSTRING]

A gap is start(launch i+1) - end(launch i) of the launches whose name contains the substring, in start order; gaps above --max-gap-us are
the pauses between the passes of a program (synchronise, set-up) and are left out, as the first --skip launches are (warm-up); --last N keeps
only the last N launches (the timed steps of a program that warms up with the same kernel).  With
--beside, the same figures for a second kernel and its end relative to the start of the named launch it overlaps (a side-stream launch).
Prints one JSON object: n, median, mean, p10, p90 in microseconds."""
import argparse
import csv
import json


def stats(v):
    v = sorted(v)
    if not v:
        return {"n": 0}

    def q(p):
        x = p * (len(v) - 1)
        lo = int(x)
        hi = min(lo + 1, len(v) - 1)
        return v[lo] + (v[hi] - v[lo]) * (x - lo)
    return {"n": len(v), "median_us": q(0.5), "mean_us": sum(v) / len(v), "p10_us": q(0.1), "p90_us": q(0.9)}


def launches(rows, needle):
    out = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows if needle in r["Kernel_Name"]]
    out.sort()
    return out


def gaps_of(path, needle, max_gap_us=1000.0, skip=0, beside=None, last=0):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    ls = launches(rows, needle)[skip:]
    if last > 0:
        ls = ls[-last:]
    res = {"trace": path, "kernel": ls[0][2][:90] if ls else None, "names_matched": len({x[2] for x in ls}),
           "duration": stats([(e - s) / 1e3 for s, e, _ in ls])}
    g = [(ls[i + 1][0] - ls[i][1]) / 1e3 for i in range(len(ls) - 1)]
    res[f"gap_below_{max_gap_us:g}us"] = stats([x for x in g if x <= max_gap_us])
    res["gaps_left_out"] = sum(1 for x in g if x > max_gap_us)
    if beside:
        bs = launches(rows, beside)
        res["beside"] = {"kernel": bs[0][2][:90] if bs else None, "duration": stats([(e - s) / 1e3 for s, e, _ in bs])}
        # each side launch against the named launch that starts nearest to it
        ends, starts = [], []
        j = 0
        for s, e, _ in bs:
            while j + 1 < len(ls) and abs(ls[j + 1][0] - s) <= abs(ls[j][0] - s):
                j += 1
            if ls and abs(ls[j][0] - s) <= max_gap_us * 1e3:
                ends.append((e - ls[j][0]) / 1e3)
                starts.append((s - ls[j][0]) / 1e3)
        res["beside"]["end_minus_named_start"] = stats(ends)
        res["beside"]["start_minus_named_start"] = stats(starts)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trace")
    ap.add_argument("kernel")
    ap.add_argument("--max-gap-us", type=float, default=1000.0)
    ap.add_argument("--skip", type=int, default=0)
    ap.add_argument("--last", type=int, default=0)
    ap.add_argument("--beside", default=None)
    a = ap.parse_args()
    print(json.dumps(gaps_of(a.trace, a.kernel, a.max_gap_us, a.skip, a.beside, a.last)))
