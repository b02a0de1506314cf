#!/usr/bin/env python3
"""Where a launch's tree fold runs relative to the voice kernels, from a rocprofv3 --kernel-trace CSV of a plain `bench.py`
(a run of its own, no counters):   python tools/fold_overlap_trace.py <..._kernel_trace.csv>
Prints one JSON object: per-kernel duration statistics of the headline voice kernel's 64-block launches and of the folds,
the idle time between consecutive voice kernels, and for every fold whether its start and end lie inside the interval of a
voice kernel (with the fold on a stream of its own that is the launch after the fold's; on one stream no fold does)."""
import csv
import json
import statistics
import sys


def stats(xs):
    if not xs:
        return None
    return {"count": len(xs), "mean_us": statistics.fmean(xs), "median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


def main():
    voice, fold = [], []
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            name, t0, t1 = r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            q = r.get("Queue_Id", "")
            if "voice_pipe_kernel" in name and 0.3e6 <= t1 - t0 < 5e6:  # the 64-block launches (tools/trace_summary.py)
                voice.append((t0, t1, q))
            elif "fold_tree" in name:
                fold.append((t0, t1, q, "fold_tree_wave_kernel" if "fold_tree_wave_kernel" in name else "fold_tree_kernel"))
    voice.sort()
    fold.sort()
    # the timed steps are the last 64-block launches of a plain run: 32 steps of four launches unless the command line says otherwise
    n_timed = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    timed = voice[-n_timed:]
    lo, hi = (timed[0][0], timed[-1][1]) if timed else (0, 0)
    gaps = [(b[0] - a[1]) * 1e-3 for a, b in zip(timed, timed[1:])]
    folds_timed = [x for x in fold if lo <= x[0] <= hi]
    inside = 0
    beside = []  # durations of the voice kernels that had a fold inside them
    for x in folds_timed:
        for v in timed:
            if v[0] <= x[0] and x[1] <= v[1]:
                inside += 1
                beside.append((v[1] - v[0]) * 1e-3)
                break
    # how long after the end of the voice kernel before it a fold starts, and how long after a fold's end the next voice kernel starts
    after_voice, before_voice = [], []
    for x in folds_timed:
        ends = [v[1] for v in timed if v[1] <= x[0]]
        starts = [v[0] for v in timed if v[0] >= x[1]]
        if ends:
            after_voice.append((x[0] - max(ends)) * 1e-3)
        if starts:
            before_voice.append((min(starts) - x[1]) * 1e-3)
    excerpt = sorted([(v[0], v[1], v[2], "voice") for v in timed[8:14]] + [(x[0], x[1], x[2], x[3]) for x in folds_timed[8:14]])
    excerpt = [{"kernel": k, "queue": q, "start_us": (a - lo) * 1e-3, "end_us": (b - lo) * 1e-3} for a, b, q, k in excerpt]
    span = (hi - lo) * 1e-3
    out = {
        "voice_kernel_64_block_launches_all": stats([(b - a) * 1e-3 for a, b, _ in voice]),
        "timed_run": {
            "voice_kernels": stats([(b - a) * 1e-3 for a, b, _ in timed]),
            "folds": stats([(b - a) * 1e-3 for a, b, _, _ in folds_timed]),
            "fold_kernel": sorted({x[3] for x in folds_timed}),
            "idle_between_voice_kernels": stats(gaps),
            "span_per_launch_us": span / len(timed) if timed else None,
            "folds_with_start_and_end_inside_a_voice_kernel": inside,
            "folds_in_the_run": len(folds_timed),
            "voice_kernels_with_a_fold_inside": stats(beside),
            "fold_start_after_the_voice_kernel_before_it_ends": stats(after_voice),
            "next_voice_kernel_start_after_a_fold_ends": stats(before_voice),
            "queues": {"voice": sorted({v[2] for v in timed}), "fold": sorted({x[2] for x in folds_timed})},
            "excerpt": excerpt,
        },
    }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
