#!/usr/bin/env python3
"""What knh_bank_restart_voices costs, beside what a host had to do without it.

For C3 and for D3 (C3 with a SampleDelay, 0.25 s rings in HBM) at 16 384 voices, a 64-block launch
  (a) with nothing restarted,
  (b) with all voices restarted in front of it,
  (c) with 64 voices restarted in front of it,
each timed on the host clock from before the restart call to after knh_bank_synchronize, alternating, medians reported.
Every window also holds the next note of the voices concerned (the envelope's trigger, the delay chain's delay time), as
a host sends it with or without the restart: (b) is compared with (a) for all voices, (c) with (a) for the same 64; and
  (d) knh_bank_destroy + knh_bank_create + constructor arguments + knh_bank_init of the same bank in the same process.
`flush_ms` is the device part of (b) alone: from after the restart call (the host's construction is over) to the end of a
knh_bank_read_done_frames, which puts the rows on the device and waits -- the pinned table's trip over PCIe and the kernel;
for D3 the kernel zeroes every ring (voices x ring stride x 4 bytes), and `ring_clear_GBps` is those bytes over flush_ms (a
lower bound of the kernel's own rate).  One JSON line per config.  Needs a gfx950 device."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import knaster_amd
from knaster_amd import _lib as L, configs

BLOCKS, REPEATS = 64, 9


def make(w):
    b = knaster_amd.VoiceBank(w.stages, w.n_voices, w.sample_type, w.out_channels, L.MIX_TREE)
    for s, a in w.ctor.items():
        b.set_ctor_args(s, a)
    b.init(configs.SAMPLE_RATE, w.block_size)
    return b


def note_on(b, w, v):
    """The next note of the voices v: the envelope's trigger and, for the delay chain, the voice's delay time."""
    b.param_apply_many(v, w.restart[0], w.restart[1], L.VALUE_TRIGGER)
    if w.delay_times is not None:
        b.param_apply_many(v, 3, 0, L.VALUE_FLOAT, w.delay_times[v])


def main():
    nv = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    for name in ("C3", "D3"):
        w = configs.config(name, n_voices=nv)
        b = make(w)
        every = np.arange(nv, dtype=np.uint32)
        some = np.arange(0, nv, nv // 64, dtype=np.uint32)[:64]
        note_on(b, w, every)
        # a window: [restart the voices r,] their next note, one 64-block launch, wait
        windows = (("a_all", every, False), ("b", every, True), ("a_64", some, False), ("c", some, True))

        def window(r, restart):
            t0 = time.perf_counter()
            if restart:
                b.restart_voices(r)
            t1 = time.perf_counter()
            note_on(b, w, r)
            b.process_blocks_device(BLOCKS)
            b.synchronize()
            return time.perf_counter() - t0, t1 - t0
        for _ in range(2):  # warm up every shape the timed windows use
            for _key, r, restart in windows:
                window(r, restart)
        t = {k: [] for k, _r, _x in windows}
        t.update({"call_all": [], "flush_all": []})
        for _ in range(REPEATS):
            for key, r, restart in windows:
                total, call = window(r, restart)
                t[key].append(total)
                if key == "b":
                    t["call_all"].append(call)
            b.restart_voices(every)
            t0 = time.perf_counter()
            b.read_done_frames()
            t["flush_all"].append(time.perf_counter() - t0)
            note_on(b, w, every)
            b.process_blocks_device(1)
            b.synchronize()
        b.close()
        d = []
        b = make(w)
        for _ in range(3):
            b.synchronize()
            t0 = time.perf_counter()
            b.close()
            b = make(w)
            b.synchronize()
            d.append(time.perf_counter() - t0)
        b.close()
        med = {k: statistics.median(x) * 1e3 for k, x in t.items()}
        ring_bytes = nv * 12000 * 4 if name == "D3" else 0
        print(json.dumps({
            "config": name, "voices": nv, "blocks_per_launch": BLOCKS,
            "a_note_on_all_ms": med["a_all"], "b_all_restarted_ms": med["b"], "a_note_on_64_ms": med["a_64"], "c_64_restarted_ms": med["c"],
            "b_minus_a_ms": med["b"] - med["a_all"], "c_minus_a_ms": med["c"] - med["a_64"],
            "a_all_spread_ms": [min(t["a_all"]) * 1e3, max(t["a_all"]) * 1e3], "a_64_spread_ms": [min(t["a_64"]) * 1e3, max(t["a_64"]) * 1e3],
            "restart_call_all_ms": med["call_all"], "flush_all_ms": med["flush_all"],
            "d_destroy_create_init_ms": statistics.median(d) * 1e3,
            "ring_bytes": ring_bytes, "ring_clear_GBps": ring_bytes / (med["flush_all"] * 1e-3) / 1e9 if ring_bytes else None,
        }), flush=True)


if __name__ == "__main__":
    main()
