// The decision table of knaster_amd/csrc/kernel_form.hpp: (what init knows of a bank, the form switches) -> the candidate
// forms in the order init tries them.  Every expected row is written out by hand from the thresholds of DESIGN.md section 4
// (256 / 512 / 1 024 voice groups, f64 and delay chains one round of the pipeline, several delays four per workgroup); none
// is computed by the function under test.  No HIP, no library: plain g++.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../knaster_amd/csrc/kernel_form.hpp"

using namespace knh;

namespace {
int failures = 0, rows = 0;

struct Want {
  uint32_t kind;
  unsigned waves = 0;     // MANY_WAVE, WHOLE_CHAIN_FUSED
  int layout = -1;        // PIPELINE
  bool long_tiles = false, pair = false;
};
const uint32_t ONE = KNH_DEBUG_FORM_WHOLE_CHAIN, PIPE = KNH_DEBUG_FORM_PIPELINE, MANY = KNH_DEBUG_FORM_MANY_WAVE, ONE_FUSED = KNH_DEBUG_FORM_WHOLE_CHAIN_FUSED,
               PIPE_FUSED = KNH_DEBUG_FORM_PIPELINE_FUSED, INTERP = KNH_DEBUG_FORM_FRAME_INTERP, FRAME = KNH_DEBUG_FORM_FRAME_JIT;
Want many(unsigned w) { return Want{MANY, w}; }
Want fused(unsigned jw) { return Want{ONE_FUSED, jw}; }
const Want IN_PLACE{PIPE, 0, 2, true, false}, FOLD{PIPE, 0, 1, true, false}, MIXER{PIPE, 0, 0, false, false}, PAIR{PIPE, 0, 2, false, true};

FormInputs::Prebuilt prebuilt(bool one_wave, bool mixer, bool fold, bool in_place, bool pair, bool wide) {
  FormInputs::Prebuilt p;
  p.one_wave = one_wave;
  p.pipe[0] = {mixer, false};
  p.pipe[1] = {fold, true};
  p.pipe[2] = {in_place, true};
  p.pair = pair;
  p.wide = wide;
  return p;
}
const FormInputs::Prebuilt ALL = prebuilt(true, true, true, true, true, true), NONE = prebuilt(false, false, false, false, false, false);

// a chain of `groups` voice groups (the last one of a single voice when there are several)
FormInputs chain(const char* sig, unsigned groups, const FormInputs::Prebuilt& pre, bool f64 = false, size_t bs = 64) {
  FormInputs in;
  in.signature = sig;
  in.n_voices = groups > 1 ? (groups - 1) * 64u + 1u : 64u;
  in.f64 = f64;
  in.block_size = bs;
  in.n_stages = in.signature.size();
  for (char c : in.signature) in.n_delays += c == 'D' || c == 'Y' || c == 'Z';
  in.dag = in.signature.find('@') != std::string::npos;
  in.prebuilt = pre;
  return in;
}

void check(const std::string& what, const FormInputs& in, const FormSwitches& sw, std::initializer_list<Want> want, const char* sig = nullptr) {
  ++rows;
  const FormPlan plan = plan_forms(in, sw);
  bool ok = plan.n == static_cast<int>(want.size()) && plan.signature == (sig ? sig : in.signature);
  int k = 0;
  for (const Want& w : want) {
    if (!ok) break;
    const FormCandidate& c = plan.candidate[k++];
    ok = c.kind == w.kind && c.waves == w.waves && c.pipe_layout == w.layout && c.long_tiles == w.long_tiles && c.pair == w.pair;
  }
  if (ok) return;
  ++failures;
  std::printf("FAIL %s: signature %s, %d candidates:", what.c_str(), plan.signature.c_str(), plan.n);
  for (int i = 0; i < plan.n; ++i)
    std::printf(" (kind %u waves %u layout %d long %d pair %d)", plan.candidate[i].kind, plan.candidate[i].waves, plan.candidate[i].pipe_layout,
                plan.candidate[i].long_tiles, plan.candidate[i].pair);
  std::printf("\n");
}

std::string at(const char* what, unsigned groups) { return std::string(what) + ", " + std::to_string(groups) + " groups"; }

const char* const NAMES[9] = {"KNH_JIT", "KNH_PIPELINE", "KNH_PIPE_BIG", "KNH_PAIR", "KNH_WIDE", "KNH_INTERP", "KNH_FRAME_JIT", "KNH_JIT_PIPE", "KNH_JIT_WAVES"};
FormSwitches env(std::initializer_list<std::pair<const char*, const char*>> set) {
  for (const char* n : NAMES) unsetenv(n);
  for (const auto& kv : set) setenv(kv.first, kv.second, 1);
  return form_switches_from_env();
}
void expect(bool cond, const char* what) {
  ++rows;
  if (!cond) { ++failures; std::printf("FAIL %s\n", what); }
}
}  // namespace

int main() {
  const FormSwitches def = env({});
  expect(!def.jit && def.pipeline == 1 && def.pipe_layouts == 7u && def.pair == -1 && !def.wide_set && def.interp && def.frame_jit && def.jit_pipe && def.jit_waves == 0,
         "the defaults");

  // 1. a pre-built chain, f32: the pipeline for one round of 256 groups, the pair for 257-512, four whole-chain wavefronts
  //    per workgroup up to 1 024 groups, eight beyond
  for (unsigned g : {1u, 2u, 256u}) check(at("C3 f32", g), chain("WmSA", g, ALL), def, {IN_PLACE});
  for (unsigned g : {257u, 512u}) check(at("C3 f32", g), chain("WmSA", g, ALL), def, {PAIR});
  for (unsigned g : {513u, 1024u}) check(at("C3 f32", g), chain("WmSA", g, ALL), def, {many(4)});
  check(at("C3 f32", 1025), chain("WmSA", 1025, ALL), def, {many(8)});
  //    ... without a pair built: the pipeline's second round
  const FormInputs::Prebuilt NO_PAIR = prebuilt(true, true, true, true, false, true), NO_WIDE = prebuilt(true, true, true, true, true, false);
  for (unsigned g : {1u, 2u, 256u, 257u, 512u}) check(at("C3 f32, no pair", g), chain("WmSA", g, NO_PAIR), def, {IN_PLACE});
  for (unsigned g : {513u, 1024u}) check(at("C3 f32, no pair", g), chain("WmSA", g, NO_PAIR), def, {many(4)});
  check(at("C3 f32, no pair", 1025), chain("WmSA", 1025, NO_PAIR), def, {many(8)});
  //    ... without a wide entry: the pipeline at any size
  for (unsigned g : {1u, 2u, 256u, 513u, 1024u, 1025u}) check(at("C3 f32, no wide entry", g), chain("WmSA", g, NO_WIDE), def, {IN_PLACE});
  for (unsigned g : {257u, 512u}) check(at("C3 f32, no wide entry", g), chain("WmSA", g, NO_WIDE), def, {PAIR});

  // 2. the same chain in f64: one round of the pipeline, no pair
  for (unsigned g : {1u, 2u, 256u}) check(at("C4 f64", g), chain("WmSA", g, ALL, true), def, {IN_PLACE});
  for (unsigned g : {257u, 512u, 513u, 1024u}) check(at("C4 f64", g), chain("WmSA", g, ALL, true), def, {many(4)});
  check(at("C4 f64", 1025), chain("WmSA", 1025, ALL, true), def, {many(8)});

  // 3. a delay chain (pre-built with the mixer layout only): one round of the pipeline in f32 too
  const FormInputs::Prebuilt DELAY = prebuilt(true, true, false, false, false, true);
  check(at("D3", 256), chain("WmSDA", 256, DELAY), def, {MIXER});
  check(at("D3", 257), chain("WmSDA", 257, DELAY), def, {many(4)});
  check(at("D3", 1024), chain("WmSDA", 1024, DELAY), def, {many(4)});
  check(at("D3", 1025), chain("WmSDA", 1025, DELAY), def, {many(8)});
  check(at("two delays", 256), chain("WmDZ", 256, DELAY), def, {MIXER});
  check(at("two delays", 1025), chain("WmDZ", 1025, DELAY), def, {many(4)});
  check(at("five delays", 4096), chain("WmDZZZZA", 4096, DELAY), def, {many(4)});

  // 4. a block that is not whole long tiles (64 frames, f64: 32) takes the 32-sample pipeline; the pair has the short tiles anyway
  check("f32, block of 64", chain("WmSA", 3, ALL, false, 64), def, {IN_PLACE});
  check("f32, block of 96", chain("WmSA", 3, ALL, false, 96), def, {MIXER});
  check("f32, block of 100", chain("WmSA", 3, ALL, false, 100), def, {MIXER});
  check("f64, block of 32", chain("WmSA", 3, ALL, true, 32), def, {IN_PLACE});
  check("f64, block of 48", chain("WmSA", 3, ALL, true, 48), def, {MIXER});
  check("f32, block of 96, 300 groups", chain("WmSA", 300, ALL, false, 96), def, {PAIR});

  // 5. no pre-built kernel: a fused pipeline for two rounds (f64, or a delay: one), fused whole-chain wavefronts beyond; behind
  //    the fused pipeline what takes the voice if it is not built
  for (unsigned g : {1u, 2u, 512u}) check(at("fused f32", g), chain("WLA", g, NONE), def, {{PIPE_FUSED}, fused(1)});
  for (unsigned g : {513u, 1024u}) check(at("fused f32", g), chain("WLA", g, NONE), def, {fused(4)});
  check(at("fused f32", 1025), chain("WLA", 1025, NONE), def, {fused(8)});
  check(at("fused f64", 256), chain("WLA", 256, NONE, true), def, {{PIPE_FUSED}, fused(1)});
  check(at("fused f64", 257), chain("WLA", 257, NONE, true), def, {fused(4)});
  check(at("fused f64", 1025), chain("WLA", 1025, NONE, true), def, {fused(8)});
  check(at("fused, a delay", 256), chain("WLDA", 256, NONE), def, {{PIPE_FUSED}, fused(1)});
  check(at("fused, a delay", 257), chain("WLDA", 257, NONE), def, {fused(4)});
  check(at("fused, several delays", 100), chain("WDYZ", 100, NONE), def, {{PIPE_FUSED}, fused(1)});
  check(at("fused, several delays", 1024), chain("WDYZ", 1024, NONE), def, {fused(4)});
  check(at("fused, several delays", 1025), chain("WDYZ", 1025, NONE), def, {fused(4)});

  // 6. a pre-built one-wavefront kernel and nothing else: a single group stays on it, more fuse a pipeline (up to 512 groups)
  const FormInputs::Prebuilt ONE_ONLY = prebuilt(true, false, false, false, false, false);
  check(at("one-wavefront kernel only", 1), chain("WLA", 1, ONE_ONLY), def, {{ONE}});
  check(at("one-wavefront kernel only", 2), chain("WLA", 2, ONE_ONLY), def, {{PIPE_FUSED}, {ONE}});
  check(at("one-wavefront kernel only", 512), chain("WLA", 512, ONE_ONLY), def, {{PIPE_FUSED}, {ONE}});
  check(at("one-wavefront kernel only, f64", 512), chain("WLA", 512, ONE_ONLY, true), def, {{PIPE_FUSED}, {ONE}});
  check(at("one-wavefront kernel only", 513), chain("WLA", 513, ONE_ONLY), def, {{ONE}});

  // 7. a graph voice: the fused one-wavefront kernel at any size, whatever KNH_JIT_WAVES says
  const char* const GRAPH = "WmD@2+@2,3AJ#3";
  check(at("graph voice", 1), chain(GRAPH, 1, NONE), def, {fused(1)});
  check(at("graph voice", 2000), chain(GRAPH, 2000, NONE), def, {fused(1)});
  check("graph voice, KNH_JIT_WAVES=4", chain(GRAPH, 3, NONE), env({{"KNH_JIT_WAVES", "4"}}), {fused(1)});

  // 8. oscillators and arithmetic alone: a lane per frame -- the kernel built at init, then the interpreter, then (neither
  //    fits the LDS) a fused lane-per-voice form
  FormInputs osc = chain("WW+@1,2#2", 1, NONE);
  osc.n_stages = 3;
  osc.frame_eligible = true;
  check("oscillators, a graph", osc, def, {{FRAME}, {INTERP}, fused(1)});
  check("oscillators, KNH_FRAME_JIT=0", osc, env({{"KNH_FRAME_JIT", "0"}}), {{INTERP}, fused(1)});
  check("oscillators, KNH_FRAME_JIT=1", osc, env({{"KNH_FRAME_JIT", "1"}}), {{FRAME}, {INTERP}, fused(1)});
  check("oscillators, KNH_INTERP=0", osc, env({{"KNH_INTERP", "0"}}), {fused(1)});
  check("oscillators, KNH_INTERP=1", osc, env({{"KNH_INTERP", "1"}}), {{FRAME}, {INTERP}, fused(1)});
  FormInputs osc_chain = chain("Wm", 1, NONE);
  osc_chain.frame_eligible = true;
  check("oscillators, a chain", osc_chain, def, {{FRAME}, {INTERP}, {PIPE_FUSED}});
  check("oscillators, a chain, KNH_FRAME_JIT=0", osc_chain, env({{"KNH_FRAME_JIT", "0"}}), {{INTERP}, {PIPE_FUSED}, fused(1)});
  { FormInputs in = osc; in.block_size = 1024; check("oscillators, block of 1024", in, def, {{FRAME}, {INTERP}, fused(1)}); }
  { FormInputs in = osc; in.block_size = 1025; check("oscillators, block of 1025", in, def, {fused(1)}); }
  { FormInputs in = osc; in.connected = true; check("oscillators, two connected outputs", in, def, {fused(1)}); }
  { FormInputs in = osc; in.n_stages = 4096; check("oscillators, 4096 stages", in, def, {{FRAME}, {INTERP}, fused(1)}); }
  { FormInputs in = osc; in.n_stages = 4097; check("oscillators, 4097 stages", in, def, {fused(1)}); }
  { FormInputs in = osc_chain; in.prebuilt = ONE_ONLY; check("oscillators with a pre-built kernel", in, def, {{ONE}}); }

  // 9. a mono reader on a pool of two-channel Buffers: 'C' for 'F', nothing pre-built is used
  { FormInputs in = chain("Fm", 3, ALL); in.two_channel_pool = true; check("two-channel pool", in, def, {{PIPE_FUSED}, fused(1)}, "Cm"); }
  { FormInputs in = chain("FmF", 600, ALL); in.two_channel_pool = true; check("two-channel pool, 600 groups", in, def, {fused(4)}, "CmC"); }
  { FormInputs in = chain("Fm", 3, ALL); check("one-channel pool", in, def, {IN_PLACE}, "Fm"); }
  { FormInputs in = chain("WmSA", 3, ALL); in.two_channel_pool = true; check("two-channel pool, no reader", in, def, {IN_PLACE}); }

  // 10. every switch at each value it accepts, and at one it ignores
  check("KNH_JIT=1", chain("WmSA", 3, ALL), env({{"KNH_JIT", "1"}}), {{PIPE_FUSED}, fused(1)});
  check("KNH_JIT=1, 600 groups", chain("WmSA", 600, ALL), env({{"KNH_JIT", "1"}}), {fused(4)});
  check("KNH_JIT=0", chain("WmSA", 3, ALL), env({{"KNH_JIT", "0"}}), {IN_PLACE});
  check("KNH_JIT=yes (ignored)", chain("WmSA", 3, ALL), env({{"KNH_JIT", "yes"}}), {IN_PLACE});
  check("KNH_PIPELINE=0", chain("WmSA", 3, ALL), env({{"KNH_PIPELINE", "0"}}), {{ONE}});
  check("KNH_PIPELINE=0, 256 groups", chain("WmSA", 256, ALL), env({{"KNH_PIPELINE", "0"}}), {{ONE}});
  check("KNH_PIPELINE=0, 300 groups", chain("WmSA", 300, ALL), env({{"KNH_PIPELINE", "0"}}), {many(4)});
  check("KNH_PIPELINE=0, nothing pre-built", chain("WLA", 3, NONE), env({{"KNH_PIPELINE", "0"}}), {fused(1)});
  check("KNH_PIPELINE=1", chain("WmSA", 3, ALL), env({{"KNH_PIPELINE", "1"}}), {IN_PLACE});
  check("KNH_PIPELINE=2", chain("WmSA", 3, ALL), env({{"KNH_PIPELINE", "2"}}), {IN_PLACE});
  check("KNH_PIPELINE=3 (ignored)", chain("WmSA", 3, ALL), env({{"KNH_PIPELINE", "3"}}), {IN_PLACE});
  check("KNH_PIPE_BIG=0", chain("WmSA", 3, ALL), env({{"KNH_PIPE_BIG", "0"}}), {MIXER});
  check("KNH_PIPE_BIG=1", chain("WmSA", 3, ALL), env({{"KNH_PIPE_BIG", "1"}}), {FOLD});
  check("KNH_PIPE_BIG=1, block of 96", chain("WmSA", 3, ALL, false, 96), env({{"KNH_PIPE_BIG", "1"}}), {MIXER});
  check("KNH_PIPE_BIG=2 (the default)", chain("WmSA", 3, ALL), env({{"KNH_PIPE_BIG", "2"}}), {IN_PLACE});
  check("KNH_PIPE_BIG=7 (the default)", chain("WmSA", 3, ALL), env({{"KNH_PIPE_BIG", "7"}}), {IN_PLACE});
  check("KNH_PAIR=1", chain("WmSA", 3, ALL), env({{"KNH_PAIR", "1"}}), {PAIR});
  check("KNH_PAIR=1, f64, 1025 groups", chain("WmSA", 1025, ALL, true), env({{"KNH_PAIR", "1"}}), {PAIR});
  check("KNH_PAIR=1, no pair built", chain("WmSA", 300, NO_PAIR), env({{"KNH_PAIR", "1"}}), {IN_PLACE});
  check("KNH_PAIR=0", chain("WmSA", 300, ALL), env({{"KNH_PAIR", "0"}}), {IN_PLACE});
  check("KNH_PAIR=2 (no pair either)", chain("WmSA", 300, ALL), env({{"KNH_PAIR", "2"}}), {IN_PLACE});
  check("KNH_PAIR=1 with KNH_PIPELINE=0", chain("WmSA", 300, ALL), env({{"KNH_PAIR", "1"}, {"KNH_PIPELINE", "0"}}), {many(4)});
  check("KNH_WIDE=4", chain("WmSA", 3, ALL), env({{"KNH_WIDE", "4"}}), {many(4)});
  check("KNH_WIDE=8", chain("WmSA", 3, ALL), env({{"KNH_WIDE", "8"}}), {many(8)});
  check("KNH_WIDE=16", chain("WmSA", 3, ALL), env({{"KNH_WIDE", "16"}}), {many(16)});
  check("KNH_WIDE=0, 600 groups", chain("WmSA", 600, ALL), env({{"KNH_WIDE", "0"}}), {IN_PLACE});
  check("KNH_WIDE=5 (none), 600 groups", chain("WmSA", 600, ALL), env({{"KNH_WIDE", "5"}}), {IN_PLACE});
  check("KNH_WIDE=0 with KNH_PIPELINE=0, 600 groups", chain("WmSA", 600, ALL), env({{"KNH_WIDE", "0"}, {"KNH_PIPELINE", "0"}}), {{ONE}});
  check("KNH_WIDE=4 without a wide entry", chain("WmSA", 3, NO_WIDE), env({{"KNH_WIDE", "4"}}), {IN_PLACE});
  check("KNH_WIDE=4 where the pair is taken", chain("WmSA", 300, ALL), env({{"KNH_WIDE", "4"}}), {PAIR});
  check("KNH_JIT_PIPE=0", chain("WLA", 3, NONE), env({{"KNH_JIT_PIPE", "0"}}), {fused(1)});
  check("KNH_JIT_PIPE=0, one-wavefront kernel only", chain("WLA", 3, ONE_ONLY), env({{"KNH_JIT_PIPE", "0"}}), {{ONE}});
  check("KNH_JIT_PIPE=1", chain("WLA", 3, NONE), env({{"KNH_JIT_PIPE", "1"}}), {{PIPE_FUSED}, fused(1)});
  check("KNH_JIT_WAVES=1, 600 groups", chain("WLA", 600, NONE), env({{"KNH_JIT_WAVES", "1"}}), {fused(1)});
  check("KNH_JIT_WAVES=4", chain("WLA", 3, NONE), env({{"KNH_JIT_PIPE", "0"}, {"KNH_JIT_WAVES", "4"}}), {fused(4)});
  check("KNH_JIT_WAVES=8", chain("WLA", 3, NONE), env({{"KNH_JIT_PIPE", "0"}, {"KNH_JIT_WAVES", "8"}}), {fused(8)});
  check("KNH_JIT_WAVES=16", chain("WLA", 3, NONE), env({{"KNH_JIT_PIPE", "0"}, {"KNH_JIT_WAVES", "16"}}), {fused(16)});
  check("KNH_JIT_WAVES=16, f64: eight", chain("WLA", 3, NONE, true), env({{"KNH_JIT_PIPE", "0"}, {"KNH_JIT_WAVES", "16"}}), {fused(8)});
  check("KNH_JIT_WAVES=2 (ignored), 600 groups", chain("WLA", 600, NONE), env({{"KNH_JIT_WAVES", "2"}}), {fused(4)});
  check("KNH_JIT_WAVES=4 behind a fused pipeline", chain("WLA", 3, NONE), env({{"KNH_JIT_WAVES", "4"}}), {{PIPE_FUSED}, fused(4)});
  for (const char* n : NAMES) unsetenv(n);

  // what the launch path asks of the form taken
  const auto facts = [](const Want& w, bool f64) {
    FormCandidate c;
    c.kind = w.kind; c.waves = w.waves; c.pipe_layout = w.layout; c.long_tiles = w.long_tiles; c.pair = w.pair;
    return form_facts(c, f64);
  };
  const auto is = [](const FormFacts& f, uint32_t tile, bool ranges, bool resident, bool per_voice) {
    return f.tile_frames == tile && f.walks_ranges == ranges && f.can_be_resident == resident && f.rows_per_voice == per_voice;
  };
  expect(is(facts(IN_PLACE, false), 64, true, true, false) && is(facts(IN_PLACE, true), 32, true, true, false), "facts: the in-place pipeline");
  expect(is(facts(MIXER, false), 32, true, true, false) && is(facts(MIXER, true), 16, true, true, false), "facts: the mixer pipeline");
  expect(is(facts(FOLD, false), 64, true, false, false), "facts: the fold pipeline has no mixer wavefront: never resident");
  expect(is(facts(PAIR, false), 32, true, false, false), "facts: the pair is never resident");
  expect(is(facts(Want{PIPE_FUSED}, false), 32, true, true, false) && is(facts(Want{PIPE_FUSED}, true), 16, true, true, false), "facts: the fused pipeline");
  expect(is(facts(Want{ONE}, false), 64, false, true, false) && is(facts(fused(1), true), 64, false, true, false), "facts: the one-wavefront kernels");
  expect(is(facts(many(4), false), 64, false, false, false), "facts: four per workgroup");
  expect(is(facts(Want{FRAME}, false), 64, false, false, true) && is(facts(Want{INTERP}, true), 64, false, false, true), "facts: a lane per frame");

  if (failures) {
    std::printf("%d of %d rows failed\n", failures, rows);
    return 1;
  }
  std::printf("ok   kernel_form: %d rows\n", rows);
  return 0;
}
