#!/usr/bin/env python3
"""What the events of a multi-block launch cost the voice kernel: the headline bank (C3, 16 384 voices, f32, 64-block
launches, the bench's two bank-wide triggers per launch) timed with the library's own HIP-event timing
(knh_bank_timing_reset / _read) in three variants, alternately, all after one prewarm:

  events        the bench's triggers, the library's default path (range events in the kernel arguments where the build has them)
  events_lists  the same with KNH_RANGE_LAUNCHES=0: per-voice lists in pinned host memory (all a build without range launches has)
  no_events     no parameter call at all: the kernel reads no event (have_events false)

events_lists - events is what the per-voice lists cost a launch.  no_events is the floor the issue asks for, with a caveat the
figures show: without triggers every envelope is at rest, so the launch also does not pay for the two tiles the triggers
land in.  Prints one JSON line; --out FILE also writes it there.

    python tools/range_events_ab.py [--rounds 7] [--launches 24] [--out profiles/x.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=16384)
    ap.add_argument("--block-size", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=64, help="blocks per launch")
    ap.add_argument("--launches", type=int, default=24, help="timed launches per variant and round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--prewarm-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import knaster_amd
    from knaster_amd import _lib as L
    from knaster_amd import configs

    w = configs.config("C3", n_voices=args.voices, block_size=args.block_size)
    mine = np.arange(w.n_voices, dtype=np.uint32)

    def make(env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)  # (the switch is read when the bank is created)
        try:
            b = knaster_amd.VoiceBank(w.stages, w.n_voices, w.sample_type, w.out_channels, L.MIX_TREE, rank=0, world=1)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        for s, a in w.ctor.items():
            b.set_ctor_args(s, a)
        b.init(configs.SAMPLE_RATE, w.block_size)
        return b, b.prepare_many(mine, w.restart[0], w.restart[1], L.VALUE_TRIGGER), b.prepare_many(mine, w.release[0], w.release[1], L.VALUE_TRIGGER)

    variants = {"events": (make({}), True), "events_lists": (make({"KNH_RANGE_LAUNCHES": "0"}), True), "no_events": (make({}), False)}

    def launches(name, n):
        (b, restart, release), ev = variants[name]
        for _ in range(n):
            if ev:
                b.param_apply_prepared(restart, 0)
                b.param_apply_prepared(release, args.blocks // 2)
            b.process_blocks_device(args.blocks)

    for name in variants:  # first-use allocations
        launches(name, 2)
        variants[name][0][0].synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:  # bring the shader clock up
        launches("events", 2)
        variants["events"][0][0].synchronize()
    runs = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name in variants:
            b = variants[name][0][0]
            launches(name, 2)
            b.synchronize()
            b.timing_reset(True)
            launches(name, args.launches)
            b.synchronize()
            ms, n = b.timing_read()
            b.timing_reset(False)
            runs[name].append(ms / max(n, 1) * 1e3)
    res = {"workload": {"config": "C3", "voices": w.n_voices, "block_size": w.block_size, "blocks_per_launch": args.blocks, "sample_type": "f32"},
           "unit": "us of voice kernel per launch (HIP events around the launch)", "launches_per_round": args.launches, "rounds": args.rounds,
           "variants": {}}
    for name, us in runs.items():
        b = variants[name][0][0]
        stats = b.event_stats() if hasattr(b, "event_stats") else None
        res["variants"][name] = {"us_per_launch": us, "median": statistics.median(us), "spread": max(us) - min(us),
                                 "event_stats_range_list_bytes": stats}
        b.close()
    med = {k: v["median"] for k, v in res["variants"].items()}
    res["lists_minus_default_us"] = med["events_lists"] - med["events"]
    res["lists_minus_default_frac_of_launch"] = (med["events_lists"] - med["events"]) / med["events_lists"]
    res["events_minus_no_events_us"] = med["events"] - med["no_events"]
    res["lists_minus_no_events_us"] = med["events_lists"] - med["no_events"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
