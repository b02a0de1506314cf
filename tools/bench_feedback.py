#!/usr/bin/env python3
"""What a feedback edge costs (KNH_STAGE_FLAG_FEEDBACK; not the headline bench, see bench.py): configs.feedback_comb beside the
same voice with the edge removed and beside D3 (one delay stage per voice), f32, 512-frame blocks, kernel time from the banks'
own device events.  The three banks are timed in turn, `repeats` times, after a warm-up of each.  One JSON line per bank and
repeat, then a summary per bank size: medians, min-max spread, and the edge's cost per voice-sample.
    tools/bench_feedback.py [voices ...]        default: 16384 65536"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import knaster_amd
from knaster_amd import _lib as L, configs

BLOCK, BLOCKS, LAUNCHES, REPEATS = 512, 32, 6, 5


def make(w):
    b = knaster_amd.VoiceBank(w.stages, w.n_voices, w.sample_type, w.out_channels, L.MIX_TREE)
    for s, a in w.ctor.items():
        b.set_ctor_args(s, a)
    b.init(configs.SAMPLE_RATE, w.block_size)
    v = np.arange(w.n_voices, dtype=np.uint32)
    b.param_apply_many(v, w.restart[0], w.restart[1], L.VALUE_TRIGGER)
    if w.delay_times is not None:
        b.param_apply_many(v, 3, 0, L.VALUE_FLOAT, w.delay_times)
    for stage, param, values in w.param_sets:
        b.param_apply_many(v, stage, param, L.VALUE_FLOAT, values)
    for _ in range(3):  # untimed: first-use allocations, the clock
        b.process_blocks_device(BLOCKS)
    b.synchronize()
    return b


def ring_bytes_per_voice_sample(w):
    """A sample read and a sample written per delay stage and per feedback edge."""
    rings = sum(s.kind in (L.STAGE_SAMPLE_DELAY, L.STAGE_ALLPASS_DELAY, L.STAGE_ALLPASS_FB_DELAY) or
                (s.kind == L.STAGE_INPUT and bool(s.flags & L.STAGE_FLAG_FEEDBACK)) for s in w.stages)
    return 2 * (8 if w.sample_type else 4) * rings


for nv in [int(a) for a in sys.argv[1:]] or [16384, 65536]:
    loads = {"feedback_comb": configs.feedback_comb(nv, BLOCK), "comb_no_edge": configs.feedback_comb(nv, BLOCK, feedback=False),
             "D3": configs.config("D3", n_voices=nv, block_size=BLOCK)}
    banks = {k: make(w) for k, w in loads.items()}
    us = {k: [] for k in loads}
    for rep in range(REPEATS):
        for k, b in banks.items():
            b.timing_reset(True)
            for _ in range(LAUNCHES):
                b.process_blocks_device(BLOCKS)
            b.synchronize()
            kms, n = b.timing_read()
            us[k].append(kms * 1e3 / (n * BLOCKS))
            vs = float(nv) * BLOCK / (us[k][-1] * 1e-6)
            print(json.dumps({"config": k, "voices": nv, "block_size": BLOCK, "sample_type": "f32", "repeat": rep, "signature": b.debug_signature(),
                              "form": int(b.debug_words()[2]), "us_per_block_kernel": us[k][-1], "kernel_only_voice_samples_per_s": vs,
                              "ring_bytes_per_voice_sample": ring_bytes_per_voice_sample(loads[k]),
                              "ring_TBps": vs * ring_bytes_per_voice_sample(loads[k]) / 1e12}), flush=True)
    for b in banks.values():
        b.close()
    med = {k: float(np.median(x)) for k, x in us.items()}
    vs = {k: float(nv) * BLOCK / (m * 1e-6) for k, m in med.items()}
    print(json.dumps({"summary": True, "voices": nv, "us_per_block_median": med, "us_per_block_min_max": {k: [min(x), max(x)] for k, x in us.items()},
                      "voice_samples_per_s": vs, "ring_TBps": {k: vs[k] * ring_bytes_per_voice_sample(loads[k]) / 1e12 for k in loads},
                      "edge_ns_per_voice_sample": (med["feedback_comb"] - med["comb_no_edge"]) * 1e3 / (float(nv) * BLOCK),
                      "edge_us_per_block": med["feedback_comb"] - med["comb_no_edge"]}), flush=True)
