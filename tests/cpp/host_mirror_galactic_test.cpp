// The Galactic reverb in the C++ host mirror (knaster_amd/host/knaster_host.hpp): `voice.out({0, 0}) >> g.push(Galactic(..))`
// is traced into the mono descriptor, `(l | r) >> g.push(Galactic(..))` into KNH_STAGE_GALACTIC with `input` / `input2`, a node
// shared between l and r once; its two outputs go to graph outputs 0 and 1.  Built and run by tests/test_host_mirror_galactic.py.
//   host_mirror_galactic_test --plan   : no device needed
//   host_mirror_galactic_test --gpu    : the traced banks render what the hand-written descriptors render
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../knaster_amd/host/knaster_host.hpp"

using namespace knaster;

static int g_fail = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++g_fail;                                                       \
    }                                                                 \
  } while (0)
#define RUN(name)                                                         \
  do {                                                                    \
    int before = g_fail;                                                  \
    try { name(); } catch (const std::exception& e) { std::printf("  EXCEPTION %s\n", e.what()); ++g_fail; } \
    std::printf("%s %s\n", g_fail == before ? "ok  " : "FAIL", #name);    \
  } while (0)

static const int kVoices = 8;
static double freq_of(int v) { return 110.0 * (v + 1) + 0.37 * v; }
// replace, detune, brightness, bigness, wet, fpd_l, fpd_r: different in every voice, no detune (the bit-exact case)
static std::vector<double> gal_args(int v) {
  return {0.5 + 0.05 * v, 0.0, 0.3 + 0.08 * v, 0.1 * v, 0.4 + 0.07 * v, 16386.0 + 977.0 * v, 99991.0 + 1013.0 * v};
}
static UGenSpec galactic_of(int v) {
  const std::vector<double> a = gal_args(v);
  return Galactic(a[0], a[1], a[2], a[3], a[4], static_cast<uint32_t>(a[5]), static_cast<uint32_t>(a[6]));
}

// one signal on both inputs
template <typename F>
static void mono_voices(GraphEdit<F>& g) {
  for (int v = 0; v < kVoices; ++v) {
    auto s = g.push(SinWt(freq_of(v))) * 0.1;
    (s.out({0, 0}) >> g.push(galactic_of(v))).to_graph_out();
  }
}
static const knh_stage_desc kMono[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_GALACTIC, 0, 0, 0, 0, 0}};
static std::vector<double> mono_args(int stage, int v) {
  if (stage == 0) return {freq_of(v)};
  if (stage == 1) return {0.1};
  return gal_args(v);
}

// two oscillators a little apart, one per input
template <typename F>
static void stereo_voices(GraphEdit<F>& g) {
  for (int v = 0; v < kVoices; ++v) {
    auto l = g.push(SinWt(freq_of(v))) * 0.1;
    auto r = g.push(SinWt(freq_of(v) * 1.01)) * 0.05;
    ((l | r) >> g.push(galactic_of(v))).to_graph_out();
  }
}
static const knh_stage_desc kStereo[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0},
                                         {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_GALACTIC, 0, 0, 0, 2, 4}};
static std::vector<double> stereo_args(int stage, int v) {
  if (stage == 0) return {freq_of(v)};
  if (stage == 1) return {0.1};
  if (stage == 2) return {freq_of(v) * 1.01};
  if (stage == 3) return {0.05};
  return gal_args(v);
}

// a dry oscillator on the left, its filtered version on the right: the oscillator is shared, and traced once
template <typename F>
static void shared_voices(GraphEdit<F>& g) {
  for (int v = 0; v < kVoices; ++v) {
    auto osc = g.push(SinWt(freq_of(v)));
    auto dry = osc * 0.1;
    auto wet = osc >> g.push(SvfFilter(SvfFilterType::Low, 900.0 + 300.0 * v, 0.8, 0.0));
    auto rev = (dry | wet) >> g.push(galactic_of(v));
    rev.to_graph_out();
  }
}
static const knh_stage_desc kShared[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_SVF, 0, 0, 0, 1, 0},
                                         {KNH_STAGE_GALACTIC, 0, 0, 0, 2, 3}};
static std::vector<double> shared_args(int stage, int v) {
  if (stage == 0) return {freq_of(v)};
  if (stage == 1) return {0.1};
  if (stage == 2) return {0.0, 900.0 + 300.0 * v, 0.8, 0.0};
  return gal_args(v);
}

template <size_t N>
static void check_plan(const Graph<float>& graph, const knh_stage_desc (&want)[N], std::vector<double> (*args)(int, int)) {
  CHECK(graph.num_banks() == 1);
  if (graph.num_banks() != 1) return;
  const auto& b = graph.bank(0);
  CHECK(b.n_voices == static_cast<uint32_t>(kVoices) && b.plan.stages.size() == N);
  if (b.plan.stages.size() != N) return;
  for (size_t s = 0; s < N; ++s) {
    const knh_stage_desc& st = b.plan.stages[s];
    CHECK(st.kind == want[s].kind && st.input == want[s].input && st.input2 == want[s].input2);
    CHECK(st.flags == 0 && st.delayed_changes_per_block == 0 && st.ar_param == 0);
    CHECK(b.plan.stage_args[s] == args(static_cast<int>(s), 0));  // (voice 0's constructor arguments)
  }
  // the reverb makes both graph outputs itself: nothing for knh_bank_connect_outputs
  CHECK(b.plan.out_stage[0] == -1 && b.plan.out_stage[1] == -1);
}

static void plan_the_mono_spelling_is_the_mono_chain() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) { mono_voices(g); });
  check_plan(*graph, kMono, mono_args);
}
static void plan_stacked_signals_are_input_and_input2() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) { stereo_voices(g); });
  check_plan(*graph, kStereo, stereo_args);
}
static void plan_a_shared_node_is_traced_once() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) { shared_voices(g); });
  check_plan(*graph, kShared, shared_args);
}
static void plan_the_reverb_has_its_parameters() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  bool threw = false;
  graph->edit([&](GraphEdit<float>& g) {
    auto rev = (g.push(SinWt(440.0)) * 0.1).out({0, 0}) >> g.push(galactic_of(0));
    rev.to_graph_out();
    for (const char* name : {"replace", "detune", "brightness", "bigness", "wet"}) rev.param(name).set(0.5);
    try { rev.param("pan"); } catch (const GraphError&) { threw = true; }
  });
  CHECK(threw && graph->num_banks() == 1);
}
static void plan_what_is_not_such_a_voice_is_refused() {
  auto refused = [](uint32_t outputs, auto build) {
    auto [graph, processor] = AudioProcessor<float>::create(outputs, {64, 48000});
    graph->plan_only = true;
    bool threw = false;
    try { graph->edit(build); } catch (const GraphError&) { threw = true; }
    return threw && graph->num_banks() == 0;  // ... and no bank was created
  };
  // a one-output graph
  CHECK(refused(1, [](GraphEdit<float>& g) { ((g.push(SinWt(440.0)) * 0.1).out({0, 0}) >> g.push(galactic_of(0))).to_graph_out(); }));
  CHECK(refused(1, [](GraphEdit<float>& g) { ((g.push(SinWt(440.0)) * 0.1).out({0, 0}) >> g.push(galactic_of(0))).out({0}).to_graph_out(); }));
  // anything behind the reverb
  CHECK(refused(2, [](GraphEdit<float>& g) {
    auto rev = (g.push(SinWt(440.0)) * 0.1).out({0, 0}) >> g.push(galactic_of(0));
    (rev * 0.5).to_graph_out();
  }));
  CHECK(refused(2, [](GraphEdit<float>& g) {
    auto rev = (g.push(SinWt(440.0)) * 0.1).out({0, 0}) >> g.push(galactic_of(0));
    (rev.out({0}) >> g.push(Pan2(0.25))).to_graph_out();
  }));
  // its outputs the other way round
  CHECK(refused(2, [](GraphEdit<float>& g) {
    auto rev = (g.push(SinWt(440.0)) * 0.1).out({0, 0}) >> g.push(galactic_of(0));
    rev.out({1, 0}).to_graph_out();
  }));
  // one input only
  CHECK(refused(2, [](GraphEdit<float>& g) { ((g.push(SinWt(440.0)) * 0.1) >> g.push(galactic_of(0))).to_graph_out(); }));
  CHECK(refused(2, [](GraphEdit<float>& g) { g.push(galactic_of(0)).to_graph_out(); }));
  // an input taken directly from a bank input (the node of a KNH_STAGE_INPUT stage)
  CHECK(refused(2, [](GraphEdit<float>& g) {
    auto in = g.push(UGenSpec(KNH_STAGE_INPUT, {0.0}));
    auto r = g.push(SinWt(440.0)) * 0.1;
    ((in | r) >> g.push(galactic_of(0))).to_graph_out();
  }));
  CHECK(refused(2, [](GraphEdit<float>& g) {
    auto in = g.push(UGenSpec(KNH_STAGE_INPUT, {0.0}));
    auto l = g.push(SinWt(440.0)) * 0.1;
    ((l | in) >> g.push(galactic_of(0))).to_graph_out();
  }));
}

// the traced bank against a bank made from the hand-written descriptor, block by block, bit for bit
template <size_t N, typename Build>
static void gpu_traced_equals_descriptor(const knh_stage_desc (&want)[N], std::vector<double> (*args)(int, int), Build build, bool sides_differ) {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->edit([&](GraphEdit<float>& g) { build(g); });
  CHECK(graph->num_banks() == 1);
  if (graph->num_banks() != 1) return;
  knh_bank_desc d{};
  d.abi_version = KNH_ABI_VERSION;
  d.n_voices = kVoices;
  d.sample_type = KNH_F32;
  d.n_stages = N;
  d.stages = want;
  d.out_channels = 2;
  d.mix_mode = KNH_MIX_TREE;
  d.device = -1;
  knh_bank* h = nullptr;
  CHECK(knh_bank_create(&d, &h) == KNH_OK);
  if (!h) { std::printf("  %s\n", knh_last_error(nullptr)); return; }
  for (size_t s = 0; s < N; ++s) {
    std::vector<double> all;
    for (int v = 0; v < kVoices; ++v) { auto a = args(static_cast<int>(s), v); all.insert(all.end(), a.begin(), a.end()); }
    if (!all.empty()) CHECK(knh_bank_set_ctor_args(h, static_cast<uint32_t>(s), 0, kVoices, all.data(), static_cast<uint32_t>(all.size() / kVoices)) == KNH_OK);
  }
  CHECK(knh_bank_init(h, 48000, 64) == KNH_OK);
  float peak[2] = {0.f, 0.f};
  int differ = 0;
  for (int block = 0; block < 6; ++block) {
    float out[2][64];
    CHECK(knh_bank_process_block(h, 64, 0, 64u * block, out, nullptr) == KNH_OK);
    processor->run_without_inputs();
    auto got = processor->output_block();
    for (size_t i = 0; i < 64; ++i) {
      differ += std::memcmp(&out[0][i], &out[1][i], 4) != 0;
      const float l = got.read(0, i), r = got.read(1, i);
      CHECK(std::memcmp(&l, &out[0][i], 4) == 0 && std::memcmp(&r, &out[1][i], 4) == 0);
      peak[0] = std::fmax(peak[0], std::fabs(out[0][i]));
      peak[1] = std::fmax(peak[1], std::fabs(out[1][i]));
    }
  }
  CHECK(peak[0] > 1e-3f && peak[1] > 1e-3f && std::isfinite(peak[0]) && std::isfinite(peak[1]));
  if (sides_differ) CHECK(differ > 100);  // a left and a right that are not each other's copy
  knh_bank_destroy(h);
}
static void gpu_mono_equals_descriptor() { gpu_traced_equals_descriptor(kMono, mono_args, [](GraphEdit<float>& g) { mono_voices(g); }, false); }
static void gpu_stereo_equals_descriptor() { gpu_traced_equals_descriptor(kStereo, stereo_args, [](GraphEdit<float>& g) { stereo_voices(g); }, true); }

int main(int argc, char** argv) {
  bool plan = false, gpu = false;
  for (int i = 1; i < argc; ++i) {
    plan = plan || !std::strcmp(argv[i], "--plan");
    gpu = gpu || !std::strcmp(argv[i], "--gpu");
  }
  if (!plan && !gpu) plan = true;
  if (plan) {
    RUN(plan_the_mono_spelling_is_the_mono_chain);
    RUN(plan_stacked_signals_are_input_and_input2);
    RUN(plan_a_shared_node_is_traced_once);
    RUN(plan_the_reverb_has_its_parameters);
    RUN(plan_what_is_not_such_a_voice_is_refused);
  }
  if (gpu) {
    if (knh_device_count() < 1) { std::printf("no gfx950 device\n"); return 2; }
    RUN(gpu_mono_equals_descriptor);
    RUN(gpu_stereo_equals_descriptor);
  }
  std::printf("%s (%d failures)\n", g_fail ? "HOST MIRROR GALACTIC FAILED" : "HOST MIRROR GALACTIC PASSED", g_fail);
  return g_fail ? 1 : 0;
}
