#!/usr/bin/env python3
"""Times every BASELINE.json workload on one GPU (not the headline bench; see bench.py).
Prints one JSON line per config: UGen-samples/s with outputs left in HBM, 32 blocks per launch."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import knaster_amd
from knaster_amd import _lib as L, configs


def run(name, n_voices=None, launches=16, blocks=32, allow_fma=False, host_threads=0, detune=None):
    w = configs.config(name, n_voices=n_voices)
    if detune is not None and name in ("G1", "G2"):  # with one detune everywhere (0: no f64 phase, no sin)
        w.ctor[len(w.stages) - 1][:, 1] = detune
    b = knaster_amd.VoiceBank(w.stages, w.n_voices, w.sample_type, w.out_channels, L.MIX_TREE, -1, allow_fma, host_threads)
    for s, a in w.ctor.items():
        b.set_ctor_args(s, a)
    b.init(configs.SAMPLE_RATE, w.block_size)
    v = np.arange(w.n_voices, dtype=np.uint32)
    if w.restart:
        b.param_apply_many(v, w.restart[0], w.restart[1], L.VALUE_TRIGGER)
    for stage, param in w.restart_more:
        b.param_apply_many(v, stage, param, L.VALUE_TRIGGER)
    if w.delay_times is not None:
        b.param_apply_many(v, 3, 0, L.VALUE_FLOAT, w.delay_times)
    for stage, param, values in w.param_sets:  # D4: every delay stage's delay_time and feedback
        b.param_apply_many(v, stage, param, L.VALUE_FLOAT, values)
    step = [0]
    # the application's own work of deciding what changes when is not the engine's: C5's event arrays are made up front
    c5 = {}
    if name == "C5":
        for blk in range(blocks * (launches + 3)):
            e = configs.c5_events(w, blk)
            c5[blk] = None if e is None else b.prepare_many(e[0], e[1], e[2], e[3], e[4], None, e[5])

    def events(k):
        for i in range(k):
            if name == "C5":
                e = c5[step[0] + i]
                if e is not None:
                    b.param_apply_prepared(e, block_offset=i)
            elif w.release and (step[0] + i) % 64 == 32:
                b.param_apply_many(v, w.release[0], w.release[1], L.VALUE_TRIGGER, block_offset=i)
            elif w.restart and (step[0] + i) % 64 == 0 and step[0] + i > 0:
                b.param_apply_many(v, w.restart[0], w.restart[1], L.VALUE_TRIGGER, block_offset=i)
                for stage, param in w.restart_more:
                    b.param_apply_many(v, stage, param, L.VALUE_TRIGGER, block_offset=i)
        step[0] += k
    for _ in range(3):  # untimed: first-use allocations (both of the alternating record / list buffers), the clock
        events(blocks)
        b.process_blocks_device(blocks)
    b.synchronize()
    b.timing_reset(True)
    t0 = time.perf_counter()
    for _ in range(launches):
        events(blocks)
        b.process_blocks_device(blocks)
    b.synchronize()
    dt = time.perf_counter() - t0
    kms, n = b.timing_read()
    # UGens per voice as SURVEY.md 8(d) counts them for the BASELINE.json configs (C2: SinNumeric + gain; C5: modulator,
    # scale/offset math, carrier); any other workload: the reference nodes its chain stands for
    ugens = {"C1": 3, "C2": 2, "C3": 4, "C4": 4, "C5": 3}.get(name) or knaster_amd.chain_ugen_count(w.stages)
    work = float(w.n_voices) * w.block_size * ugens * blocks * launches
    rd, wr = b.algorithmic_bytes_per_voice_block()
    if w.delay_times is not None:  # the ring: one sample read and one written per frame
        rd += 4 * w.block_size
        wr += 4 * w.block_size
    extra = {}
    n_delays = sum(s.kind in (L.STAGE_SAMPLE_DELAY, L.STAGE_ALLPASS_DELAY, L.STAGE_ALLPASS_FB_DELAY) for s in w.stages)
    if n_delays:  # ring traffic alone: a sample read and one written per delay stage and voice-sample (8 bytes in f32)
        word = 8 if w.sample_type else 4
        if n_delays > 1:
            rd += n_delays * word * w.block_size
            wr += n_delays * word * w.block_size
        extra = {"delay_stages": n_delays, "signature": b.debug_signature(), "form": int(b.debug_words()[2]),
                 "ring_TBps": 2 * word * n_delays * float(w.n_voices) * w.block_size * blocks * n / (kms * 1e-3) / 1e12}
    if name in ("G1", "G2"):  # 24 long rings + the two short ones, one sample read and one written per frame each; the staged input; two outputs
        # (G2's second staging plane is in algorithmic_bytes_per_voice_block already)
        word = 8 if w.sample_type else 4
        rd += (24 + 2 + 1) * word * w.block_size
        wr += (24 + 2 + 1 + 2) * word * w.block_size
        vs = float(w.n_voices) * w.block_size * blocks
        extra = {"voice_samples_per_s": vs * launches / dt, "kernel_only_voice_samples_per_s": vs * n / (kms * 1e-3),
                 "ring_algorithmic_GBps": 50 * word * vs * n / (kms * 1e-3) / 1e9, "blocks_per_launch": blocks,
                 "detune": "per voice" if detune is None else detune}
    print(json.dumps({"config": name, "voices": w.n_voices, "block_size": w.block_size, "sample_type": "f64" if w.sample_type else "f32",
                      "ugens_per_voice": ugens, "allow_fma": allow_fma, "host_threads": max(1, host_threads), "ugen_samples_per_s": work / dt,
                      "kernel_only_ugen_samples_per_s": work / (kms * 1e-3), "us_per_block_kernel": kms * 1e3 / (n * blocks),
                      "hbm_algorithmic_GBps": (rd + wr) * w.n_voices * blocks * n / (kms * 1e-3) / 1e9, **extra}), flush=True)
    b.close()


def run_sampler(case, n_voices=16384, block_size=512, launches=16, blocks=32, repeats=3):
    """The sampler workload, BufferReader -> x const in f32, every voice looping at a rate and from a start of its own.
    case "shared": one Buffer of 1 s for every voice (knh_bank_set_buffer alone -- also what a build without the pool runs);
    case "pool": 64 Buffers of about 1 s each (knh_bank_add_buffer), voice v on entry v % 64.
    One JSON line per repeat: the kernel time per block from the bank's own device events."""
    from knaster_amd.bank import Stage
    stages = [Stage(L.STAGE_BUFFER_READER), Stage(L.STAGE_MUL_CONST)]
    rng = np.random.default_rng(7)
    v = np.arange(n_voices, dtype=np.uint32)
    u = v.astype(np.int64)
    ctor = np.stack([0.5 + 1.5 * ((u * 2654435761) % 1000) / 1000.0, np.ones(n_voices), 0.9 * ((u * 40503) % 997) / 997.0], axis=1)
    n_buffers = 64 if case == "pool" else 1
    for rep in range(repeats):
        b = knaster_amd.VoiceBank(stages, n_voices, L.F32, 2, L.MIX_TREE)
        b.set_ctor_args(0, ctor)
        b.set_ctor_args(1, np.full((n_voices, 1), 1.0 / n_voices))
        if case == "pool":
            for k in range(n_buffers):
                b.add_buffer(0, rng.uniform(-1, 1, 48000 + 37 * k).astype(np.float32), 48000.0)
            b.assign_buffers(0, v, v % n_buffers)
        else:
            b.set_buffer(0, rng.uniform(-1, 1, 48000).astype(np.float32), 48000.0)
        b.init(configs.SAMPLE_RATE, block_size)
        for _ in range(3):
            b.process_blocks_device(blocks)
        b.synchronize()
        b.timing_reset(True)
        t0 = time.perf_counter()
        for _ in range(launches):
            b.process_blocks_device(blocks)
        b.synchronize()
        dt = time.perf_counter() - t0
        kms, n = b.timing_read()
        print(json.dumps({"config": "sampler", "case": case, "buffers": n_buffers, "voices": n_voices, "block_size": block_size, "sample_type": "f32",
                          "signature": b.debug_signature(), "repeat": rep, "us_per_block_kernel": kms * 1e3 / (n * blocks),
                          "us_per_block_wall": dt * 1e6 / (launches * blocks),
                          "kernel_only_voice_samples_per_s": float(n_voices) * block_size * blocks * n / (kms * 1e-3)}), flush=True)
        b.close()


def run_sampler_stereo(n_voices=16384, block_size=512, launches=8, blocks=32, repeats=4):
    """The stereo sampler, f32, every voice looping at a rate of its own on one of 64 Buffers of about 1 s.  Two banks in this
    process, timed in turn (A, B, A, B, ...) after a warm-up of each, by the banks' own device events around launches that end
    in a synchronise:
      A  one stereo reader (BufferReader<F, U2> on interleaved two-channel Buffers), a MUL_CONST per channel, connected outputs;
      B  two mono readers on the voice's entry of a one-channel pool, a MUL_CONST each, connected outputs -- the voice the
         library ran before it had a stereo reader: the yardstick.
    A voice-sample is one frame of one voice, both channels.  Both fetch 16 pool bytes per voice-sample (two frames of two
    f32 samples; two readers x two samples); A with two 8-byte loads and one read pointer, B with four 4-byte loads and two.
    One JSON line per repeat and bank, then a summary: medians, the spread between B's own repeats, and whether A is within it."""
    from knaster_amd.bank import Stage
    CH1 = Stage(L.STAGE_BUFFER_READER, flags=L.STAGE_FLAG_READER_CH1, input=1)
    stages = {"A": [Stage(L.STAGE_BUFFER_READER), CH1, Stage(L.STAGE_MUL_CONST, input=1), Stage(L.STAGE_MUL_CONST, input=2)],
              "B": [Stage(L.STAGE_BUFFER_READER), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_BUFFER_READER), Stage(L.STAGE_MUL_CONST)]}
    outs = {"A": (2, 3), "B": (1, 3)}
    rng = np.random.default_rng(7)
    v = np.arange(n_voices, dtype=np.uint32)
    u = v.astype(np.int64)
    ctor = np.stack([0.5 + 1.5 * ((u * 2654435761) % 1000) / 1000.0, np.ones(n_voices), np.zeros(n_voices)], axis=1)
    n_buffers = 64
    buffers = [rng.uniform(-1, 1, (48000 + 37 * k, 2)).astype(np.float32) for k in range(n_buffers)]
    banks = {}
    for name in ("A", "B"):
        b = knaster_amd.VoiceBank(stages[name], n_voices, L.F32, 2, L.MIX_TREE)
        for s, st in enumerate(stages[name]):
            if st.kind == L.STAGE_MUL_CONST:
                b.set_ctor_args(s, np.full((n_voices, 1), 1.0 / n_voices))
            elif not st.flags:
                b.set_ctor_args(s, ctor)
        for k in range(n_buffers):
            if name == "A":
                b.add_buffer(0, buffers[k], 48000.0, channels=2)
            else:
                b.add_buffer(0, np.ascontiguousarray(buffers[k][:, 0]), 48000.0)
        b.assign_buffers(0, v, v % n_buffers)
        b.connect_outputs(*outs[name])
        b.init(configs.SAMPLE_RATE, block_size)
        for _ in range(3):  # untimed: first-use allocations, the clock
            b.process_blocks_device(blocks)
        b.synchronize()
        banks[name] = b
    us = {"A": [], "B": []}
    for rep in range(repeats):
        for name in ("A", "B"):
            b = banks[name]
            b.timing_reset(True)
            for _ in range(launches):
                b.process_blocks_device(blocks)
            b.synchronize()
            kms, n = b.timing_read()
            us[name].append(kms * 1e3 / (n * blocks))
            print(json.dumps({"config": "sampler", "case": "stereo", "bank": name, "buffers": n_buffers, "voices": n_voices, "block_size": block_size,
                              "sample_type": "f32", "signature": b.debug_signature(), "repeat": rep, "us_per_block_kernel": us[name][-1],
                              "kernel_only_voice_samples_per_s": float(n_voices) * block_size / (us[name][-1] * 1e-6),
                              "pool_bytes_per_voice_sample": 16, "pool_loads_per_voice_sample": 2 if name == "A" else 4}), flush=True)
    for b in banks.values():
        b.close()
    med = {k: float(np.median(x)) for k, x in us.items()}
    spread = max(us["B"]) - min(us["B"])
    print(json.dumps({"config": "sampler", "case": "stereo", "summary": True, "us_per_block_A": med["A"], "us_per_block_B": med["B"],
                      "voice_samples_per_s_A": float(n_voices) * block_size / (med["A"] * 1e-6),
                      "voice_samples_per_s_B": float(n_voices) * block_size / (med["B"] * 1e-6),
                      "B_spread_us": spread, "A_minus_B_us": med["A"] - med["B"], "A_within_B_spread": bool(med["A"] - med["B"] <= spread)}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "sampler":  # tools/bench_configs.py sampler shared|pool|stereo: BASELINE.md section 4, the sampler rows
        for case in sys.argv[2:] or ["shared", "pool"]:
            if case == "stereo":
                run_sampler_stereo()
            else:
                run_sampler(case)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "ab":  # the configs that run on kernels other than the headline one
        run("C3", n_voices=65536)
        run("C3", n_voices=262144, launches=4)
        run("D3")
        run("D3", n_voices=65536)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "D4":  # five delay stages per voice, and D3's one beside them: BASELINE.md section 4, the D4 rows
        for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 1):
            run("D3")
            run("D3", n_voices=65536)
            run("D4")
            run("D4", n_voices=65536)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "G1":  # the reverb: 4 096 voices, 64 blocks per launch; the same with no detune; D3 beside it
        run("G1", launches=8, blocks=64)
        run("G1", launches=8, blocks=64, detune=0.0)
        run("D3", n_voices=65536)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "G2":  # the reverb with a stereo input beside G1, in turn: tools/bench_configs.py G2 [repeats]
        for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 3):
            run("G1", launches=8, blocks=64)
            run("G2", launches=8, blocks=64)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "only":  # tools/bench_configs.py only C5 C3 C2:1024 ...
        for spec in sys.argv[2:]:
            name, _, nv = spec.partition(":")
            run(name, n_voices=int(nv) if nv else None)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "c5":  # the host-bound config against the number of host threads
        for k in (0, 2, 4, 8, 12):
            run("C5", host_threads=k, launches=16)
        sys.exit(0)
    run("C1")
    run("C2")
    run("C3")
    run("C3", allow_fma=True)
    run("C3", n_voices=65536)
    run("C3", n_voices=262144, launches=4)
    run("C4", n_voices=8192)
    run("C4")
    run("C5")
    run("C5", host_threads=4)
    run("B3")
    run("D3")
    run("D3", n_voices=65536)
    run("D3", n_voices=262144, launches=4)
