#!/usr/bin/env python3
"""Kernel time of the C3 voice with its oscillator on a Wavetable (OscWt.wr_mul -> SvfFilter -> * EnvAsr): 16 384 voices,
512-frame blocks, f32, beside the same chain on SinWt fused at init (KNH_JIT=1: SinWt's table read from LDS).

  sinwt     the C3 chain itself, fused
  saw17     a 17-table band-limited saw: every sample gathered from the 1.1 MB entry in device memory
  one-lds   a single table, staged to LDS in the sine table's place
  one-gath  the same single table with KNH_WT_LDS=0: gathered

The four banks are made once and measured in turn, several rounds, so that whatever else shares the machine falls on all of
them alike; median and spread of the rounds per variant, one JSON line each, then the ratios to sinwt."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import knaster_amd
from knaster_amd import _lib as L, configs
from knaster_amd.bank import Stage

HARMONIC_LIMITS = [625, 416, 277, 185, 123, 82, 54, 36, 24, 16, 10, 7, 4, 3, 2, 1, 0]  # wavetable.rs:378-386


def saw_tables(end_harmonic=600):
    """Wavetable::new().add_saw(0, end_harmonic, 1.0) (wavetable.rs:545-552, 247-261), normalised by table 0's peak."""
    k = np.arange(16384, dtype=np.float64) / 16384.0 * np.pi * 2.0
    tables = np.zeros((17, 16384))
    acc = np.zeros(16384)
    ends = [min(end_harmonic, lim) for lim in HARMONIC_LIMITS]
    for h in range(max(ends) + 1):
        acc = acc + np.sin(k * (h + 1)) * (1.0 / ((h + 1) * np.pi))
        for i, e in enumerate(ends):
            if e == h and e > 0:
                tables[i] = acc
    return (tables / np.abs(tables[0]).max()).astype(np.float32)


def make(variant, n, bs):
    w = configs.config("C3", n_voices=n, block_size=bs, sample_type=L.F32)
    os.environ["KNH_JIT"] = "1"
    os.environ.pop("KNH_WT_LDS", None)
    stages = list(w.stages)
    if variant != "sinwt":
        stages[0] = Stage(L.STAGE_SIN_WT, flags=L.STAGE_FLAG_WAVETABLE)
    if variant == "one-gath":
        os.environ["KNH_WT_LDS"] = "0"
    b = knaster_amd.VoiceBank(stages, n, L.F32, 2, L.MIX_TREE)
    for s, a in w.ctor.items():
        b.set_ctor_args(s, a)
    if variant == "saw17":
        b.add_wavetable(0, saw_tables())
    elif variant != "sinwt":
        b.add_wavetable(0, saw_tables()[0])
    b.init(48000, bs)
    b.param_apply_many(np.arange(n, dtype=np.uint32), 3, 3, L.VALUE_TRIGGER)
    b.process_blocks_device(8)  # warm-up: code objects loaded, the attack under way
    b.synchronize()
    return b


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    bs, blocks, rounds = 512, 32, 9
    names = ["sinwt", "saw17", "one-lds", "one-gath"]
    banks = {v: make(v, n, bs) for v in names}
    us = {v: [] for v in names}
    for _ in range(rounds):
        for v in names:
            b = banks[v]
            b.timing_reset(True)
            b.process_blocks_device(blocks)
            b.synchronize()
            ms, _launches = b.timing_read()
            us[v].append(ms * 1e3 / blocks)
    med = {v: float(np.median(us[v])) for v in names}
    for v in names:
        print(json.dumps({"variant": v, "signature": banks[v].debug_signature(), "form": int(banks[v].debug_words()[2]), "voices": n,
                          "us_per_block_kernel_median": round(med[v], 3), "min": round(min(us[v]), 3), "max": round(max(us[v]), 3),
                          "ratio_to_sinwt": round(med[v] / med["sinwt"], 4)}), flush=True)
    for b in banks.values():
        b.close()


if __name__ == "__main__":
    main()
