#!/usr/bin/env python3
"""Kernel time of the C3-shaped voice with an audio-rate link in front of it, next to the voice without one: us per 512-frame
block at 16 384 voices, f32, after 8 warm-up blocks, over 64 blocks, all three in one run on one device.
  (a) B3 as it is: PolyBlep.wr_mul -> Svf -> * EnvAsr (a chain: the pipelined kernel form)
  (b) lfo -> SinWt.ar_params() "freq" linked, .wr_mul -> Svf -> * EnvAsr
  (c) lfo -> PolyBlep(Rectangle).ar_params() "pulse_width" linked, .wr_mul -> Svf -> * EnvAsr
(b) and (c) are graphs: they run in the one-wavefront whole-chain kernel fused at init, the linked node sample by sample."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import knaster_amd
from knaster_amd import _lib as L, configs
from knaster_amd.bank import Stage

N, BS, WARMUP, BLOCKS = 16384, 512, 8, 64


def linked_voice(osc, ar_param, osc_ctor):
    p = configs.voice_parameters(N)
    col = lambda a: np.asarray(a, dtype=np.float64).reshape(N, -1)
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST), Stage(osc, ar_param=ar_param, input2=3),
          Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR)]
    depth, offset = (0.3 * p["freq"], p["freq"]) if osc == L.STAGE_SIN_WT else (np.full(N, 0.45), np.full(N, 0.5))
    svf = np.stack([np.full(N, float(L.SVF_LOW)), p["cutoff"], p["q"], np.zeros(N)], axis=1)
    ctor = {0: col(0.2 * p["freq"]), 1: col(depth), 2: col(offset), 3: osc_ctor(p), 4: col(np.full(N, 1.0 / N)), 5: svf,
            6: np.stack([p["attack"], p["release"]], axis=1)}
    return st, ctor, (6, 3)


def measure(name, stages, ctor, restart):
    b = knaster_amd.VoiceBank(stages, N, L.F32, 2, L.MIX_TREE)
    for s, a in ctor.items():
        b.set_ctor_args(s, a)
    b.init(48000, BS)
    b.param_apply_many(np.arange(N, dtype=np.uint32), restart[0], restart[1], L.VALUE_TRIGGER)
    b.process_blocks_device(WARMUP)
    b.synchronize()
    b.timing_reset(True)
    b.process_blocks_device(BLOCKS)
    b.synchronize()
    kms, _ = b.timing_read()
    sig = b.debug_signature()
    b.close()
    us = kms * 1e3 / BLOCKS
    print(json.dumps({"voice": name, "signature": sig if len(sig) < 80 else sig[:77] + "...", "us_per_block_kernel": round(us, 2)}), flush=True)
    return us


w = configs.config("B3")
a = measure("a: B3", w.stages, w.ctor, w.restart)
b_us = measure("b: lfo -> SinWt freq linked", *linked_voice(L.STAGE_SIN_WT, 1, lambda p: p["freq"].reshape(N, 1)))
c_us = measure("c: lfo -> PolyBlep(Rectangle) pulse_width linked",
               *linked_voice(L.STAGE_POLYBLEP, 2, lambda p: np.stack([np.full(N, 5.0), p["freq"]], axis=1)))
print(json.dumps({"n_voices": N, "block_size": BS, "blocks_timed": BLOCKS, "a_us": round(a, 2), "b_us": round(b_us, 2), "c_us": round(c_us, 2),
                  "c_over_b": round(c_us / b_us, 2)}), flush=True)
