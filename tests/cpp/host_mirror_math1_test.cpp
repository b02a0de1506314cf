// The Math1UGen factories of the C++ host mirror (knaster/src/math_ugens.rs: fract ceil exp trunc floor sqrt) and what
// `trace` makes of them.  Built and run by tests/test_host_mirror_math1.py.
//   host_mirror_math1_test --plan   : no device needed
//   host_mirror_math1_test --gpu    : the traced banks render what hand-written descriptors of the same voices render
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

// (sine * 3.0) >> floor() >> svf: a chain stays a chain
template <typename F>
static void chain_voices(GraphEdit<F>& g) {
  for (int v = 0; v < kVoices; ++v) {
    auto s = g.push(SinWt(freq_of(v)));
    auto fl = g.push(floor());  // the mirror's factory: no argument, so it stands beside <cmath>'s floor(double)
    auto svf = g.push(SvfFilter(SvfFilterType::Low, 900.0 + 300.0 * v, 0.8 + 0.1 * v, 0.0));
    (((s * 3.0) >> fl) >> svf).out({0, 0}).to_graph_out();
  }
}
static const knh_stage_desc kChain[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_MATH1_FLOOR, 0, 0, 0, 0, 0},
                                        {KNH_STAGE_SVF, 0, 0, 0, 0, 0}};
static std::vector<double> chain_args(int stage, int v) {
  if (stage == 0) return {freq_of(v)};
  if (stage == 1) return {3.0};
  if (stage == 3) return {0.0, 900.0 + 300.0 * v, 0.8 + 0.1 * v, 0.0};
  return {};
}

// the root of (trunc(4 a) + b + 5.5) feeds a fract and a ceil, whose sum is the voice: a fan-out, explicit operands
template <typename F>
static void graph_voices(GraphEdit<F>& g) {
  for (int v = 0; v < kVoices; ++v) {
    auto a = g.push(SinWt(freq_of(v)));
    auto b = g.push(SinWt(freq_of(v) * 1.5));
    auto t = (a * 4.0) >> g.push(knaster::trunc());
    auto r = ((t + b) + 5.5) >> g.push(knaster::sqrt());
    auto fr = r >> g.push(fract());
    auto ce = r >> g.push(ceil());
    ((fr + ce) >> g.push(knaster::exp())).out({0, 0}).to_graph_out();
  }
}
static const knh_stage_desc kGraph[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0},    {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0},  {KNH_STAGE_MATH1_TRUNC, 0, 0, 0, 0, 0},
                                        {KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0},    {KNH_STAGE_MATH_ADD, 0, 0, 0, 3, 4},   {KNH_STAGE_ADD_CONST, 0, 0, 0, 0, 0},
                                        {KNH_STAGE_MATH1_SQRT, 0, 0, 0, 0, 0}, {KNH_STAGE_MATH1_FRACT, 0, 0, 0, 0, 0}, {KNH_STAGE_MATH1_CEIL, 0, 0, 0, 7, 0},
                                        {KNH_STAGE_MATH_ADD, 0, 0, 0, 8, 9},  {KNH_STAGE_MATH1_EXP, 0, 0, 0, 0, 0}};
static std::vector<double> graph_args(int stage, int v) {
  if (stage == 0) return {freq_of(v)};
  if (stage == 1) return {4.0};
  if (stage == 3) return {freq_of(v) * 1.5};
  if (stage == 5) return {5.5};
  return {};
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
}

static void plan_chain_stays_a_chain() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) { chain_voices(g); });
  check_plan(*graph, kChain, chain_args);
  for (const knh_stage_desc& st : graph->bank(0).plan.stages) CHECK(st.input == 0);
  CHECK(knh_chain_ugen_count(kChain, 4) == 5);  // SinWt, Constant, MathUGen Mul, Math1UGen Floor, SvfFilter
}
static void plan_fan_out_names_its_operands() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) { graph_voices(g); });
  check_plan(*graph, kGraph, graph_args);
}
static void plan_a_math1_node_has_no_parameters() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  bool threw = false;
  graph->edit([&](GraphEdit<float>& g) {
    auto s = g.push(SinWt(440.0));
    auto e = g.push(knaster::exp());
    (s >> e).out({0, 0}).to_graph_out();
    try { e.param("value"); } catch (const GraphError&) { threw = true; }
  });
  CHECK(threw);
  CHECK(std::floor(2.5) == 2.0 && floor(2.5) == 2.0 && sqrt(4.0) == 2.0);  // <cmath>'s functions are still what one argument finds
}

// the traced bank against a bank made from the hand-written descriptor, block by block, bit for bit
template <size_t N, typename Build>
static void gpu_traced_equals_descriptor(const knh_stage_desc (&want)[N], std::vector<double> (*args)(int, int), Build build) {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->edit([&](GraphEdit<float>& g) { build(g); });
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
  float peak = 0.f;
  for (int block = 0; block < 3; ++block) {
    float out[2][64];
    CHECK(knh_bank_process_block(h, 64, 0, 64u * block, out, nullptr) == KNH_OK);
    processor->run_without_inputs();
    auto got = processor->output_block();
    for (size_t i = 0; i < 64; ++i) {
      CHECK(std::memcmp(&out[0][i], &out[1][i], 4) == 0);
      const float l = got.read(0, i), r = got.read(1, i);
      CHECK(std::memcmp(&l, &out[0][i], 4) == 0 && std::memcmp(&r, &out[1][i], 4) == 0);
      peak = std::fmax(peak, std::fabs(out[0][i]));
    }
  }
  CHECK(peak > 1e-3f && std::isfinite(peak));
  knh_bank_destroy(h);
}
static void gpu_chain_equals_descriptor() { gpu_traced_equals_descriptor(kChain, chain_args, [](GraphEdit<float>& g) { chain_voices(g); }); }
static void gpu_fan_out_equals_descriptor() { gpu_traced_equals_descriptor(kGraph, graph_args, [](GraphEdit<float>& g) { graph_voices(g); }); }

int main(int argc, char** argv) {
  bool plan = false, gpu = false;
  for (int i = 1; i < argc; ++i) {
    plan = plan || !std::strcmp(argv[i], "--plan");
    gpu = gpu || !std::strcmp(argv[i], "--gpu");
  }
  if (!plan && !gpu) plan = true;
  if (plan) {
    RUN(plan_chain_stays_a_chain);
    RUN(plan_fan_out_names_its_operands);
    RUN(plan_a_math1_node_has_no_parameters);
  }
  if (gpu) {
    if (knh_device_count() < 1) { std::printf("no gfx950 device\n"); return 2; }
    RUN(gpu_chain_equals_descriptor);
    RUN(gpu_fan_out_equals_descriptor);
  }
  std::printf("%s (%d failures)\n", g_fail ? "HOST MIRROR MATH1 FAILED" : "HOST MIRROR MATH1 PASSED", g_fail);
  return g_fail ? 1 : 0;
}
