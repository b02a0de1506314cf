// Two different signals on the two graph outputs in the C++ host mirror: `(l | r).to_graph_out()` and
// `l.to_graph_out_channels({0}); r.to_graph_out_channels({1})` (graph_edit.rs:363-394, 1219-1368) trace ONE voice holding both
// subgraphs, a shared node once, and connect its two outputs (knh_bank_connect_outputs).  Built and run by
// tests/test_host_mirror_stereo.py.
//   host_mirror_stereo_test --plan   : no device needed
//   host_mirror_stereo_test --gpu    : the traced banks render what hand-written descriptors plus knh_bank_connect_outputs render
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

static const int kVoices = 5;
static double freq_of(int v) { return 110.0 * (v + 1) + 0.37 * v; }

// two detuned oscillators, one per side: no node is shared
template <typename F>
static void detuned_voices(GraphEdit<F>& g) {
  for (int v = 0; v < kVoices; ++v) {
    auto l = g.push(SinWt(freq_of(v))) * 0.5;
    auto r = g.push(SinWt(freq_of(v) * 1.5)) * 0.25;
    (l | r).to_graph_out();
  }
}
static const knh_stage_desc kDetuned[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0},
                                          {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0}};
static const uint32_t kDetunedOuts[2] = {1, 3};
static std::vector<double> detuned_args(int stage, int v) {
  if (stage == 0) return {freq_of(v)};
  if (stage == 1) return {0.5};
  if (stage == 2) return {freq_of(v) * 1.5};
  return {0.25};
}

// a raw oscillator (scaled) on the left, its filtered version on the right: the oscillator is shared, and traced once;
// connected in two calls
template <typename F>
static void dry_and_filtered_voices(GraphEdit<F>& g) {
  for (int v = 0; v < kVoices; ++v) {
    auto osc = g.push(SinWt(freq_of(v)));
    auto dry = osc * 0.5;
    auto wet = osc >> g.push(SvfFilter(SvfFilterType::Low, 900.0 + 300.0 * v, 0.8 + 0.1 * v, 0.0));
    dry.to_graph_out_channels({0});
    wet.to_graph_out_channels({1});
  }
}
static const knh_stage_desc kShared[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_SVF, 0, 0, 0, 1, 0}};
static const uint32_t kSharedOuts[2] = {1, 2};
static std::vector<double> shared_args(int stage, int v) {
  if (stage == 0) return {freq_of(v)};
  if (stage == 1) return {0.5};
  return {0.0, 900.0 + 300.0 * v, 0.8 + 0.1 * v, 0.0};
}

template <size_t N>
static void check_plan(const Graph<float>& graph, const knh_stage_desc (&want)[N], const uint32_t (&outs)[2], std::vector<double> (*args)(int, int)) {
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
  CHECK(b.plan.out_stage[0] == static_cast<int>(outs[0]) && b.plan.out_stage[1] == static_cast<int>(outs[1]));
}

static void plan_stacked_signals_are_one_voice() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) { detuned_voices(g); });
  check_plan(*graph, kDetuned, kDetunedOuts, detuned_args);
}
static void plan_a_shared_node_is_traced_once() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) { dry_and_filtered_voices(g); });
  check_plan(*graph, kShared, kSharedOuts, shared_args);
}
static void plan_the_same_signal_twice_stays_the_mono_voice() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) {
    auto s = g.push(SinWt(440.0)) * 0.5;
    (s | s).to_graph_out();                          // what .out({0, 0}) spells
    auto t = g.push(SinWt(220.0)) * 0.5;
    t.out({0, 0}).to_graph_out_channels({0, 1});
  });
  CHECK(graph->num_banks() == 1);
  if (graph->num_banks() != 1) return;
  CHECK(graph->bank(0).n_voices == 2 && graph->bank(0).plan.stages.size() == 2);
  CHECK(graph->bank(0).plan.out_stage[0] == -1 && graph->bank(0).plan.out_stage[1] == -1);
}
static void plan_what_is_not_a_voice_is_refused() {
  auto expect_error = [](auto build) {
    auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
    graph->plan_only = true;
    bool threw = false;
    try { graph->edit(build); } catch (const GraphError&) { threw = true; }
    return threw;
  };
  // a Pan2 keeps its rule: its two outputs on graph outputs 0 and 1, in order, nothing beside them
  CHECK(expect_error([](GraphEdit<float>& g) {
    auto p = g.push(SinWt(440.0)) >> g.push(Pan2(0.25));
    auto o = g.push(SinWt(220.0)) * 0.5;
    (p.out({0}) | o).to_graph_out();
  }));
  // one graph output left without a signal
  CHECK(expect_error([](GraphEdit<float>& g) { (g.push(SinWt(440.0)) * 0.5).to_graph_out_channels({0}); }));
  // ... and the graph is usable afterwards: the half voice is dropped, the next edit commits
  {
    auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
    graph->plan_only = true;
    bool threw = false;
    try {
      graph->edit([](GraphEdit<float>& g) { (g.push(SinWt(440.0)) * 0.5).to_graph_out_channels({0}); });
    } catch (const GraphError&) { threw = true; }
    CHECK(threw && graph->num_banks() == 0);
    graph->edit([](GraphEdit<float>& g) { detuned_voices(g); });
    CHECK(graph->num_banks() == 1 && graph->bank(0).n_voices == static_cast<uint32_t>(kVoices));
    if (graph->num_banks() == 1) CHECK(graph->bank(0).plan.out_stage[0] == 1 && graph->bank(0).plan.out_stage[1] == 3);
  }
  // two signals on one graph output
  CHECK(expect_error([](GraphEdit<float>& g) {
    (g.push(SinWt(440.0)) * 0.5).to_graph_out_channels({0});
    (g.push(SinWt(220.0)) * 0.5).to_graph_out_channels({0});
  }));
}

// the traced bank against a bank made from the hand-written descriptor and knh_bank_connect_outputs, block by block, bit for bit
template <size_t N, typename Build>
static void gpu_traced_equals_descriptor(const knh_stage_desc (&want)[N], const uint32_t (&outs)[2], std::vector<double> (*args)(int, int), Build build) {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->edit([&](GraphEdit<float>& g) { build(g); });
  CHECK(graph->num_banks() == 1 && knh_bank_output_stage(graph->bank(0).h, 0) == outs[0] && knh_bank_output_stage(graph->bank(0).h, 1) == outs[1]);
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
  CHECK(knh_bank_connect_outputs(h, 2, outs) == KNH_OK);
  for (size_t s = 0; s < N; ++s) {
    std::vector<double> all;
    for (int v = 0; v < kVoices; ++v) { auto a = args(static_cast<int>(s), v); all.insert(all.end(), a.begin(), a.end()); }
    if (!all.empty()) CHECK(knh_bank_set_ctor_args(h, static_cast<uint32_t>(s), 0, kVoices, all.data(), static_cast<uint32_t>(all.size() / kVoices)) == KNH_OK);
  }
  CHECK(knh_bank_init(h, 48000, 64) == KNH_OK);
  float peak[2] = {0.f, 0.f};
  int differ = 0;
  for (int block = 0; block < 3; ++block) {
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
  CHECK(differ > 100);  // a left and a right that are not each other's copy
  knh_bank_destroy(h);
}
static void gpu_stacked_equals_descriptor() { gpu_traced_equals_descriptor(kDetuned, kDetunedOuts, detuned_args, [](GraphEdit<float>& g) { detuned_voices(g); }); }
static void gpu_shared_node_equals_descriptor() { gpu_traced_equals_descriptor(kShared, kSharedOuts, shared_args, [](GraphEdit<float>& g) { dry_and_filtered_voices(g); }); }

int main(int argc, char** argv) {
  bool plan = false, gpu = false;
  for (int i = 1; i < argc; ++i) {
    plan = plan || !std::strcmp(argv[i], "--plan");
    gpu = gpu || !std::strcmp(argv[i], "--gpu");
  }
  if (!plan && !gpu) plan = true;
  if (plan) {
    RUN(plan_stacked_signals_are_one_voice);
    RUN(plan_a_shared_node_is_traced_once);
    RUN(plan_the_same_signal_twice_stays_the_mono_voice);
    RUN(plan_what_is_not_a_voice_is_refused);
  }
  if (gpu) {
    if (knh_device_count() < 1) { std::printf("no gfx950 device\n"); return 2; }
    RUN(gpu_stacked_equals_descriptor);
    RUN(gpu_shared_node_equals_descriptor);
  }
  std::printf("%s (%d failures)\n", g_fail ? "HOST MIRROR STEREO FAILED" : "HOST MIRROR STEREO PASSED", g_fail);
  return g_fail ? 1 : 0;
}
