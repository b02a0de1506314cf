#!/usr/bin/env python3
"""Kernel time of the pitch-envelope voice, us per 512-frame block at 16 384 voices, f32, in its two spellings:
  source  [ENV_AR | ENV_SOURCE, MUL_CONST, ADD_CONST, SIN_WT | AR_FREQ, MUL_ENV_ASR]   (KNH_STAGE_FLAG_ENV_SOURCE)
  twin    [INPUT, MUL_ENV_AR, MUL_CONST, ADD_CONST, SIN_WT | AR_FREQ, MUL_ENV_ASR] on a bank input that is all ones: the only
          way to spell the voice without the flag (an input plane and a load per sample more)
Both are plain chains and take the fused pipeline.  A repeat is a fresh bank, 8 warm-up blocks, then LAUNCHES launches of 64
blocks with every pitch envelope restarted in front of each launch (so that the tiles do not all sit in the constant path);
the spellings alternate, REPEATS times, in one process on one device.  Reported: each repeat, the median per spelling, and
the spread (max - min) of each spelling's own repeats.  A library without the flag runs the twin alone."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import knaster_amd
from knaster_amd import _lib as L, configs
from knaster_amd.bank import Stage

N, BS, WARMUP, BLOCKS = 16384, 512, 8, 64
ENV_SOURCE = getattr(L, "STAGE_FLAG_ENV_SOURCE", None)


def voice(spelling):
    p = configs.voice_parameters(N)
    col = lambda a: np.asarray(a, dtype=np.float64).reshape(N, -1)
    tail = [Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST), Stage(L.STAGE_SIN_WT, flags=L.STAGE_FLAG_AR_FREQ), Stage(L.STAGE_MUL_ENV_ASR)]
    u = (np.arange(N) % 97) / 97.0
    pitch_env = np.stack([0.002 + 0.008 * u, 0.05 + 0.15 * u], axis=1)  # 2 .. 10 ms up, 50 .. 200 ms down: most of a launch's 683 ms moving
    tail_ctor = [col(0.5 * p["freq"]), col(p["freq"]), col(p["freq"]), np.stack([p["attack"], p["release"]], axis=1)]
    if spelling == "source":
        st, ctor = [Stage(L.STAGE_MUL_ENV_AR, flags=ENV_SOURCE)] + tail, [pitch_env] + tail_ctor
    else:
        st, ctor = [Stage(L.STAGE_INPUT), Stage(L.STAGE_MUL_ENV_AR)] + tail, [col(np.zeros(N)), pitch_env] + tail_ctor
    env = len(st) - 5
    return st, dict(enumerate(ctor)), env, len(st) - 1


def measure(spelling, launches):
    st, ctor, env, amp = voice(spelling)
    b = knaster_amd.VoiceBank(st, N, L.F32, 2, L.MIX_TREE, in_channels=0 if spelling == "source" else 1)
    for s, a in ctor.items():
        b.set_ctor_args(s, a)
    b.init(48000, BS)
    v = np.arange(N, dtype=np.uint32)
    ones = None if spelling == "source" else np.ones((BLOCKS, 1, BS), dtype=np.float32)
    b.param_apply_many(v, amp, 3, L.VALUE_TRIGGER)
    b.param_apply_many(v, env, 2, L.VALUE_TRIGGER)
    if ones is not None:
        b.set_input(ones[:WARMUP])
    b.process_blocks_device(WARMUP)
    b.synchronize()
    b.timing_reset(True)
    for _ in range(launches):
        b.param_apply_many(v, env, 2, L.VALUE_TRIGGER)
        if ones is not None:
            b.set_input(ones)
        b.process_blocks_device(BLOCKS)
    b.synchronize()
    kms, _ = b.timing_read()
    sig, form = b.debug_signature(), int(b.debug_words()[2])
    b.close()
    us = kms * 1e3 / (BLOCKS * launches)
    print(json.dumps({"spelling": spelling, "signature": sig, "form": form, "us_per_block_kernel": round(us, 3)}), flush=True)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=16, help="launches of 64 blocks timed per repeat")
    args = ap.parse_args()
    if knaster_amd.lib.load().knh_device_count() < 1:
        raise SystemExit("bench_env_source: no gfx950 device visible; there is no CPU path")
    spellings = ["twin"] + (["source"] if ENV_SOURCE is not None else [])
    runs = {s: [] for s in spellings}
    for _ in range(args.repeats):
        for s in spellings:
            runs[s].append(measure(s, args.launches))
    out = {"n_voices": N, "block_size": BS, "blocks_timed_per_repeat": BLOCKS * args.launches, "repeats": args.repeats}
    for s in spellings:
        out[s + "_us_median"] = round(statistics.median(runs[s]), 3)
        out[s + "_us_spread"] = round(max(runs[s]) - min(runs[s]), 3)
    if "source" in runs:
        out["source_minus_twin_us"] = round(out["source_us_median"] - out["twin_us_median"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
