// kernel_form.hpp -- which kernel form a bank takes: the one place where that is decided.  plan_forms() is a pure function
// from what knh_bank_init knows of the bank (FormInputs) and the form switches of the environment (FormSwitches) to the
// candidate forms in the order init tries them (FormPlan); form_facts() says what the launch path needs to know of the form
// that was taken.  Bank<F>::init (voice_bank.hpp) fills the inputs, builds what a candidate needs built and keeps the first
// that stands.  No HIP in here: the CPU test tests/cpp/kernel_form_test.cpp holds the decision to a hand-written table.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "../../include/knaster_hip.h"

namespace knh {

// The nine form switches, read when a bank is initialised (A/B measurements and tests; none changes what is computed).
struct FormSwitches {
  bool jit = false;            // KNH_JIT=1: run-time fusion also for chains that have pre-built kernels
  int pipeline = 1;            // KNH_PIPELINE: 0 = no wave pipeline, pre-built or fused; 1 (default) or 2 = wave pipelines
  // KNH_PIPE_BIG, the pipeline layouts a bank may take (bit i = layout i of voice_pipe.hpp: PIPE_MIXER, PIPE_FOLD,
  // PIPE_INPLACE).  0: 32-sample tiles and the mixer wavefront only; 1: also 64-sample tiles with the fold in the last stage
  // group (round 1's form); default (2, or anything else): also 64-sample tiles, the last group in place and a mixer
  // wavefront on the fourth SIMD.
  unsigned pipe_layouts = 7u;
  int pair = -1;               // KNH_PAIR: 1 = the two-groups-per-workgroup pipeline wherever it is built, set to anything else = never, -1 = not set
  bool wide_set = false;       // KNH_WIDE is set: `wide` whole-chain wavefronts per workgroup (4, 8 or 16 take effect, anything else means none)
  int wide = 0;
  bool interp = true;          // KNH_INTERP=0: never a lane per frame
  bool frame_jit = true;       // KNH_FRAME_JIT=0: the lane-per-frame voices are interpreted
  bool jit_pipe = true;        // KNH_JIT_PIPE=0: no pipeline is fused at init
  unsigned jit_waves = 0;      // KNH_JIT_WAVES=1|4|8|16: wavefronts per workgroup of the fused whole-chain form, 0 = not set (or any other value)
};

inline FormSwitches form_switches_from_env() {
  FormSwitches s;
  const auto first = [](const char* name) { const char* e = std::getenv(name); return e ? e[0] : '\0'; };
  s.jit = first("KNH_JIT") == '1';
  const char level = first("KNH_PIPELINE");
  s.pipeline = level >= '0' && level <= '2' ? level - '0' : 1;
  const char big = first("KNH_PIPE_BIG");
  s.pipe_layouts = big == '0' ? 1u : (big == '1' ? 3u : 7u);
  if (std::getenv("KNH_PAIR")) s.pair = first("KNH_PAIR") == '1' ? 1 : 0;
  if (const char* e = std::getenv("KNH_WIDE")) { s.wide_set = true; s.wide = std::atoi(e); }
  s.interp = first("KNH_INTERP") != '0';
  s.frame_jit = first("KNH_FRAME_JIT") != '0';
  s.jit_pipe = first("KNH_JIT_PIPE") != '0';
  if (const char* e = std::getenv("KNH_JIT_WAVES")) { const int v = std::atoi(e); if (v == 1 || v == 4 || v == 8 || v == 16) s.jit_waves = static_cast<unsigned>(v); }
  return s;
}

// What the decision reads.
struct FormInputs {
  std::string signature;          // kernel_registry.hpp
  uint32_t n_voices = 0;
  bool f64 = false;
  size_t block_size = 0;
  bool connected = false;         // two connected outputs (knh_bank_connect_outputs)
  size_t n_stages = 0;
  bool frame_eligible = false;    // every stage is one a lane per FRAME can run (stage_table.hpp frame_eligible)
  bool dag = false;               // the voice is a graph, not a chain (signature_is_dag)
  unsigned n_delays = 0;          // 'D', 'Y' and 'Z' stages
  bool two_channel_pool = false;  // the BufferReader pool holds two-channel Buffers
  // what is pre-built for the signature (find_kernel, find_pipe, find_wide)
  struct Prebuilt {
    bool one_wave = false;                                    // the one-wavefront kernel
    struct Layout { bool built = false, long_tiles = false; } pipe[3];  // the pipeline, one voice group per workgroup, by layout
    bool pair = false;                                        // the pipeline with two voice groups per workgroup
    bool wide = false;                                        // 4 / 8 / 16 whole-chain wavefronts per workgroup
  } prebuilt;
};

// One kernel form: its KNH_DEBUG_FORM_* kind and the variant beneath it.
struct FormCandidate {
  uint32_t kind = KNH_DEBUG_FORM_WHOLE_CHAIN;
  int pipe_layout = -1;     // PIPELINE: 0 PIPE_MIXER, 1 PIPE_FOLD, 2 PIPE_INPLACE
  bool long_tiles = false;  // PIPELINE: 64-sample tiles (f64: 32), not 32 (16)
  bool pair = false;        // PIPELINE: two voice groups per workgroup
  unsigned waves = 0;       // MANY_WAVE: 4, 8 or 16 wavefronts per workgroup; WHOLE_CHAIN_FUSED: 1, 4, 8 or 16 (jw)
};

// The candidates in the order init tries them.  A lane-per-frame form that does not fit or does not build gives way to the
// next candidate; so does a fused pipeline of a chain with several delay stages.
struct FormPlan {
  std::string signature;  // the inputs', or with 'C' for every 'F': a mono reader on a pool of two-channel Buffers
  FormCandidate candidate[3];
  int n = 0;
  void add(uint32_t kind, unsigned waves = 0) { candidate[n].kind = kind; candidate[n].waves = waves; ++n; }
};

inline FormPlan plan_forms(const FormInputs& in, const FormSwitches& sw) {
  FormPlan plan;
  plan.signature = in.signature;
  FormInputs::Prebuilt pre = in.prebuilt;
  // A mono reader on a pool of two-channel Buffers plays channel 0 of the interleaved frames -- a stage of its own
  // (knh_dev::BufferReaderCh0, 'C' for 'F'), so the voice is fused whatever was pre-built for its mono form.
  if (in.two_channel_pool && plan.signature.find('F') != std::string::npos) {
    std::replace(plan.signature.begin(), plan.signature.end(), 'F', 'C');
    pre = FormInputs::Prebuilt{};
  }
  const unsigned groups = (in.n_voices + 63u) / 64u;
  const bool several_delays = in.n_delays > 1;
  // a chain without a pre-built one-wavefront kernel has no pre-built form at all: it is fused at init (hiprtc)
  const bool entry = pre.one_wave && !sw.jit;

  // ---- the pre-built forms ----
  // The 64-sample-tile pipeline is used where one is built: measured 3 % faster than the 32-sample form over C3's note
  // cycle, 12 % with every envelope at rest.  The preferred layout first: in place, fold, mixer.
  int layout = -1;
  for (int l = 2; l >= 0 && entry && sw.pipeline >= 1 && layout < 0; --l)
    if (((sw.pipe_layouts >> l) & 1u) && pre.pipe[l].built) layout = l;
  // Occupancy regime: the wave pipeline minimises latency when every 64-voice group can have a CU to itself (<= ~1.5 groups
  // per CU); beyond that throughput wins and the groups are packed 4 or 8 to a workgroup (one or two wavefronts per SIMD)
  // sharing one staged sine table.
  // Banks of more 64-voice groups than the chip has CUs: two groups per workgroup, each with its own pipeline, sharing the
  // staged sine table -- two wavefronts per SIMD (voice_pipe.hpp, GPW).  One round of it renders 512 groups.
  // Measured (us per 512-frame block, profiles/r03_form_sweep.txt): C3 f32 at 320 / 512 groups 17.8 / 18.5 against 23.5 / 23.8
  // for one group per workgroup and 25.5 / 25.8 for four whole-chain wavefronts per workgroup; from 640 groups on the latter
  // win (26.1-27.1 up to 1 024 groups against 34.7-35.1).  f64 gains nothing from it (38.6-39.1 against 37.0-37.2: an f64
  // wavefront alone already keeps its SIMD's f64 pipe busy).  So: f32 banks of 257-512 groups.
  const bool pair = entry && sw.pipeline >= 1 && pre.pair && (sw.pair >= 0 ? sw.pair == 1 : (groups > 256u && groups <= 512u && !in.f64));
  unsigned wide_waves = 0;
  if (entry && !pair && pre.wide) {
    const bool pipe = layout >= 0;
    // The pipeline takes ceil(groups / 256 CUs) rounds of its one-group-per-CU time, the 4-group kernel one round of the
    // whole chain's single-wavefront time up to 1 024 groups, the 8-group kernel one of two wavefronts per SIMD up to 2 048.
    // Measured on C3 / C4 (us per 512-frame block, profiles/r03_form_sweep.txt): f32 pipeline 23.5 at 257-512 groups, 35 at
    // 513-768, against 25.5-27.1 flat for four groups per workgroup and 37-40 for eight (79.6 at 4 096 groups, where sixteen
    // take 85.6 -- their tiles are too short for the 32-sample visits the others make); f64 pipeline 39.6-40.1 at 257-512
    // groups against 37.0-38.7 flat for four per workgroup, 68-72 for eight up to 2 048.  So: the pipeline for two rounds in
    // f32, one in f64; four groups per workgroup up to 1 024 groups, eight beyond.
    const unsigned pipe_max = in.f64 ? 256u : 512u;
    int ww = groups <= pipe_max && pipe ? 0 : (groups <= 1024u ? 4 : 8);
    if (!pipe && groups <= 256u) ww = 0;
    // A chain with a delay (rings in HBM, moved as whole lines: voice_stages.hpp RingLines) is bound by memory, and the
    // pipeline has one wavefront per voice group to keep requests in flight: beyond one round of it the whole-chain forms
    // win (D3, us per block, profiles/r04_delay_forms.txt: 20 480 voices 57.8 / 51.8, 65 536 117 / 67.9 for four per
    // workgroup, 131 072 233 / 126 / 118 for eight).  (Rounds 1-3 kept every delay chain on the pipeline: a lane per
    // voice's 16-byte pieces ran at 2.0 TB/s in any form.)
    if (pipe && in.n_delays > 0) ww = groups <= 256u ? 0 : (groups <= 1024u ? 4 : 8);
    // Several delay stages per voice: four wavefronts per workgroup at any size -- a wavefront that shares its SIMD's
    // registers has no room for four delays' tiles (kernels_wide.hip KNH_WIDE_RINGS)
    if (ww == 8 && several_delays) ww = 4;
    if (sw.wide_set) ww = sw.wide;
    if (ww == 4 || ww == 8 || ww == 16) wide_waves = static_cast<unsigned>(ww);
  }
  // The 64-sample-tile pipeline only where the block is made of whole tiles: a partial tile runs sample by sample, and a
  // 32- or 96-frame block would be half partial tiles (its 32-sample form has none).  The pair has the short tiles.
  if (!pair && layout > 0 && in.block_size % (in.f64 ? 32u : 64u) != 0) layout = pre.pipe[0].built ? 0 : -1;
  const bool pipe = pair || layout >= 0;

  // ---- a lane per frame ----
  // Voices made of SinWt oscillators and arithmetic alone (graphs, or chains without a pre-built kernel) are not run a lane
  // per voice at all: every stage is a pure function of the frame index, so a lane per FRAME it is (voice_frame.hpp) --
  // measured 10-27 times the lane-per-voice form from one voice to 65 536 (tools/bench_fm_cascade.py), and the only form that
  // takes the reference's 1 531-stage cascade.  By default as one straight-line kernel built at init, else interpreted
  // (kernels_interp.hip).  (A voice with two connected outputs is not one of them: the frame kernels hand out one signal.)
  // Whether the voice fits the LDS is init's to find out, with the parsed program: if not, the next candidate takes it.
  if (!entry && in.block_size <= 1024 && in.n_stages <= 4096 && !in.connected && in.frame_eligible && sw.interp) {
    if (sw.frame_jit) plan.add(KNH_DEBUG_FORM_FRAME_JIT);
    plan.add(KNH_DEBUG_FORM_FRAME_INTERP);
  }

  // ---- fused at init ----
  // Beyond the pipeline's reach a fused chain runs as whole-chain wavefronts sharing a staged sine table, four to a workgroup
  // (one per SIMD) up to 1 024 groups, eight beyond -- the forms of the pre-built chains; four at any size with several
  // delay stages (at eight, four delays' tiles spill).  A voice that is a graph keeps the one-wavefront form (its signals'
  // registers leave no room to share a SIMD), whatever KNH_JIT_WAVES says.  Sixteen f64 tiles do not fit beside the table.
  // The fused pipeline covers two rounds of 256 voice groups in f32; one in f64 and for chains with a delay, whose rings want
  // as many wavefronts as there are to keep requests in flight: the thresholds of the pre-built chains.  (A chain with a
  // pre-built one-wavefront kernel but no pre-built wide form keeps the fused pipeline up to 512 groups.)
  const unsigned jit_pipe_max = !entry && (in.f64 || in.n_delays > 0) ? 256u : 512u;
  unsigned jw = !in.dag && groups > jit_pipe_max ? (groups <= 1024u ? 4u : 8u) : 1u;
  if (jw == 8u && several_delays) jw = 4u;
  if (sw.jit_waves && !in.dag) jw = sw.jit_waves;
  if (in.f64 && jw == 16u) jw = 8u;
  // Chains without a pre-built pipelined kernel are fused as one: up to two voice groups per CU the pipelined form wins by a
  // wide margin.  (A single voice group with a pre-built kernel stays on it: nothing to gain, and no compile at init.  A
  // voice that is a graph runs in the single-wave form: the pipeline's edges carry one signal.)
  const bool fuse_pipe = !pipe && wide_waves == 0 && sw.pipeline >= 1 && groups <= jit_pipe_max && sw.jit_pipe && !(entry && groups == 1) && !in.dag;
  if (fuse_pipe) plan.add(KNH_DEBUG_FORM_PIPELINE_FUSED);
  // Behind a fused pipeline: what takes the voice if the pipeline has no room for several delay stages' tiles (a RingLines
  // tile per stage group beside the table and the edges: voice_pipe.hpp's LDS sum).  (A voice both lane-per-frame forms are
  // tried for has no delay stage: the fused pipeline is the last it can come to.)
  if (plan.n == 3) return plan;
  if (!entry) {
    plan.add(KNH_DEBUG_FORM_WHOLE_CHAIN_FUSED, jw);
  } else if (wide_waves != 0) {
    plan.add(KNH_DEBUG_FORM_MANY_WAVE, wide_waves);
  } else if (pipe) {
    FormCandidate& c = plan.candidate[plan.n];
    plan.add(KNH_DEBUG_FORM_PIPELINE);
    c.pair = pair;
    c.pipe_layout = pair ? 2 : layout;  // (the pair is built in place)
    c.long_tiles = !pair && pre.pipe[layout].long_tiles;
  } else {
    plan.add(KNH_DEBUG_FORM_WHOLE_CHAIN);
  }
  return plan;
}

// What the launch path needs to know of the form a bank runs in.
struct FormFacts {
  uint32_t tile_frames = 64;    // frames per tile the form hands its rows over in (voice_pipe.hpp PipeTile; the one-wavefront kernel: 64)
  bool walks_ranges = false;    // the pipelined kernels walk range events (voice_pipe.hpp), resident or launched; the others take per-voice lists
  bool can_be_resident = false; // every workgroup can be resident at once and the fold server can take the rows
  bool rows_per_voice = false;  // the fold kernels get a row per voice (a lane per frame), not one per wavefront
};

inline FormFacts form_facts(const FormCandidate& c, bool f64) {
  const bool prebuilt_pipe = c.kind == KNH_DEBUG_FORM_PIPELINE, pipelined = prebuilt_pipe || c.kind == KNH_DEBUG_FORM_PIPELINE_FUSED;
  const bool frames = c.kind == KNH_DEBUG_FORM_FRAME_INTERP || c.kind == KNH_DEBUG_FORM_FRAME_JIT;
  FormFacts f;
  // (voice_pipe.hpp PipeTile: 32 frames, f64 16, twice that in the layouts with the long tiles; jit.hip fuses pipelines in the
  // mixer layout with the short tiles)
  if (pipelined) f.tile_frames = (f64 ? 16u : 32u) * (prebuilt_pipe && c.long_tiles ? 2u : 1u);
  f.walks_ranges = pipelined;
  // the one-wavefront kernels, pre-built or fused, and the pipelines with a mixer wavefront (not PIPE_FOLD) and one voice group per workgroup
  f.can_be_resident = !frames && c.kind != KNH_DEBUG_FORM_MANY_WAVE && !(prebuilt_pipe && (c.pair || c.pipe_layout == 1));
  f.rows_per_voice = frames;
  return f;
}

}  // namespace knh
