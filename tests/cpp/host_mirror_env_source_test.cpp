// Envelopes as signals in the C++ host mirror: what `trace` makes of an envelope node that is not just the right-hand side
// of a `*` -- an ENV_SOURCE stage (KNH_STAGE_FLAG_ENV_SOURCE) with its wrappers behind it -- and that a plain
// `signal * env` is still one MUL_ENV_* stage.  Built and run by tests/test_host_mirror_env_source.py.
//   host_mirror_env_source_test --plan   : no device needed
//   host_mirror_env_source_test --gpu    : the traced filter-envelope bank renders what the hand-written descriptor renders
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
static const uint16_t ES = KNH_STAGE_FLAG_ENV_SOURCE;
static double freq_of(int v) { return 110.0 * (v + 1) + 0.37 * v; }
static double attack_of(int v) { return 0.0004 + 0.0003 * v; }
static double release_of(int v) { return 0.002 + 0.0005 * v; }

// knh_stage_desc: kind, flags, delayed_changes_per_block, ar_param, input, input2
// The filter envelope: (sine * EnvAsr) >> SvfFilter.ar_params(), cutoff_freq linked to EnvAr.wr_mul(3000).wr_add(200)
template <typename F>
static void filter_voices(GraphEdit<F>& g, std::vector<typename Sig<F>::Parameter>* restart) {
  for (int v = 0; v < kVoices; ++v) {
    auto s = g.push(SinWt(freq_of(v)));
    auto amp = g.push(EnvAsr(attack_of(v), 0.01));
    auto fe = g.push(EnvAr(attack_of(v), release_of(v)).wr_mul(3000.0).wr_add(200.0));
    auto svf = g.push(SvfFilter(SvfFilterType::Low, 1000.0, 0.9, 0.0).ar_params());
    svf.link("cutoff_freq", fe);
    ((s * amp) >> svf).out({0, 0}).to_graph_out();
    if (restart) { restart->push_back(amp.param("t_restart")); restart->push_back(fe.param("t_restart")); }
  }
}
static const knh_stage_desc kFilter[] = {{KNH_STAGE_MUL_ENV_AR, ES, 0, 0, 0, 0}, {KNH_STAGE_WR_MUL, 0, 0, 0, 0, 0}, {KNH_STAGE_WR_ADD, 0, 0, 0, 0, 0},
                                         {KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0},     {KNH_STAGE_MUL_ENV_ASR, 0, 0, 0, 0, 0}, {KNH_STAGE_SVF, 0, 0, 1, 0, 3}};
static std::vector<double> filter_args(int stage, int v) {
  switch (stage) {
    case 0: return {attack_of(v), release_of(v)};
    case 1: return {3000.0};
    case 2: return {200.0};
    case 3: return {freq_of(v)};
    case 4: return {attack_of(v), 0.01};
    default: return {0.0, 1000.0, 0.9, 0.0};
  }
}

template <size_t N>
static void check_plan(const Graph<float>& graph, const knh_stage_desc (&want)[N]) {
  CHECK(graph.num_banks() == 1);
  if (graph.num_banks() != 1) return;
  const auto& b = graph.bank(0);
  CHECK(b.n_voices == static_cast<uint32_t>(kVoices) && b.plan.stages.size() == N);
  if (b.plan.stages.size() != N) return;
  for (size_t s = 0; s < N; ++s) {
    const knh_stage_desc& st = b.plan.stages[s];
    CHECK(st.kind == want[s].kind && st.flags == want[s].flags && st.input == want[s].input && st.input2 == want[s].input2 && st.ar_param == want[s].ar_param);
  }
}
template <typename Build>
static std::unique_ptr<Graph<float>> planned(Build build) {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) { for (int v = 0; v < kVoices; ++v) build(g, v); });
  return std::move(graph);
}

static void plan_filter_envelope_is_a_source_with_its_wrappers() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) { filter_voices<float>(g, nullptr); });
  check_plan(*graph, kFilter);
  if (graph->num_banks() == 1)
    for (int s = 0; s < 6; ++s) CHECK(graph->bank(0).plan.stage_args[s] == filter_args(s, 0));
  CHECK(knh_chain_ugen_count(kFilter, 6) == 1 + 1 + 2 + 1);  // EnvAr (wrapped), SinWt, EnvAsr + Mul, SvfFilter
}
static void plan_wrapped_envelope_inside_a_product() {
  auto graph = planned([](GraphEdit<float>& g, int v) {
    auto s = g.push(SinWt(freq_of(v)));
    (s * g.push(EnvAsr(attack_of(v), release_of(v)).wr_mul(0.5))).out({0, 0}).to_graph_out();
  });
  static const knh_stage_desc want[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_MUL_ENV_ASR, ES, 0, 0, 0, 0}, {KNH_STAGE_WR_MUL, 0, 0, 0, 0, 0},
                                        {KNH_STAGE_MATH_MUL, 0, 0, 0, 1, 3}};
  check_plan(*graph, want);
}
static void plan_envelope_read_by_a_product_and_a_link() {
  auto graph = planned([](GraphEdit<float>& g, int v) {
    auto s = g.push(SinWt(freq_of(v)));
    auto e = g.push(EnvAsr(attack_of(v), release_of(v)));
    auto s2 = g.push(SinWt(55.0).ar_params());
    s2.link("phase_offset", e * 400.0);
    ((s * e) + s2).out({0, 0}).to_graph_out();
  });
  // ONE source stage, read by the MathUGen Mul and by the `* 400` in front of the second oscillator's phase_offset
  static const knh_stage_desc want[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0},    {KNH_STAGE_MUL_ENV_ASR, ES, 0, 0, 0, 0}, {KNH_STAGE_MATH_MUL, 0, 0, 0, 1, 2},
                                        {KNH_STAGE_MUL_CONST, 0, 0, 0, 2, 0}, {KNH_STAGE_SIN_WT, 0, 0, 2, 0, 4},       {KNH_STAGE_MATH_ADD, 0, 0, 0, 3, 5}};
  check_plan(*graph, want);
}
static void plan_envelope_on_the_graph_output_and_under_plus() {
  auto alone = planned([](GraphEdit<float>& g, int v) { g.push(EnvAr(attack_of(v), release_of(v))).out({0, 0}).to_graph_out(); });
  static const knh_stage_desc want_alone[] = {{KNH_STAGE_MUL_ENV_AR, ES, 0, 0, 0, 0}};
  check_plan(*alone, want_alone);
  auto plus = planned([](GraphEdit<float>& g, int v) { (g.push(Envelope(0.0, {{0.001, 1.0}, {0.002 + 0.0001 * v, 0.0}})) + 0.25).out({0, 0}).to_graph_out(); });
  static const knh_stage_desc want_plus[] = {{KNH_STAGE_MUL_ENVELOPE, ES, 0, 0, 0, 0}, {KNH_STAGE_ADD_CONST, 0, 0, 0, 0, 0}};
  check_plan(*plus, want_plus);
}
static void plan_signal_times_envelope_is_still_one_stage() {
  auto graph = planned([](GraphEdit<float>& g, int v) {
    auto s = g.push(SinWt(freq_of(v)).wr_mul(0.1));
    auto f = g.push(SvfFilter(SvfFilterType::Low, 900.0, 0.8, 0.0));
    ((s >> f) * g.push(EnvAsr(attack_of(v), release_of(v)))).out({0, 0}).to_graph_out();
  });
  static const knh_stage_desc want[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_WR_MUL, 0, 0, 0, 0, 0}, {KNH_STAGE_SVF, 0, 0, 0, 0, 0},
                                        {KNH_STAGE_MUL_ENV_ASR, 0, 0, 0, 0, 0}};  // C3's plan, as ever
  check_plan(*graph, want);
  auto left = planned([](GraphEdit<float>& g, int v) { (g.push(EnvAr(attack_of(v), release_of(v))) * g.push(SinWt(freq_of(v)))).out({0, 0}).to_graph_out(); });
  static const knh_stage_desc want_left[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_MUL_ENV_AR, 0, 0, 0, 0, 0}};
  check_plan(*left, want_left);
}

// the traced bank against a bank made from the hand-written descriptor, block by block, bit for bit
static void gpu_filter_envelope_equals_descriptor() {
  const size_t N = 6;
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  std::vector<Sig<float>::Parameter> restart;
  graph->edit([&](GraphEdit<float>& g) { filter_voices<float>(g, &restart); });
  knh_bank_desc d{};
  d.abi_version = KNH_ABI_VERSION;
  d.n_voices = kVoices;
  d.sample_type = KNH_F32;
  d.n_stages = N;
  d.stages = kFilter;
  d.out_channels = 2;
  d.mix_mode = KNH_MIX_TREE;
  d.device = -1;
  knh_bank* h = nullptr;
  CHECK(knh_bank_create(&d, &h) == KNH_OK);
  if (!h) { std::printf("  %s\n", knh_last_error(nullptr)); return; }
  for (size_t s = 0; s < N; ++s) {
    std::vector<double> all;
    for (int v = 0; v < kVoices; ++v) { auto a = filter_args(static_cast<int>(s), v); all.insert(all.end(), a.begin(), a.end()); }
    CHECK(knh_bank_set_ctor_args(h, static_cast<uint32_t>(s), 0, kVoices, all.data(), static_cast<uint32_t>(all.size() / kVoices)) == KNH_OK);
  }
  CHECK(knh_bank_init(h, 48000, 64) == KNH_OK);
  float peak = 0.f;
  for (int block = 0; block < 5; ++block) {
    if (block == 0) {
      for (auto& p : restart) p.trig();
      for (int v = 0; v < kVoices; ++v) {
        CHECK(knh_bank_param_apply(h, v, 4, 3, KNH_VALUE_TRIGGER, 0.0, 0) == KNH_OK);  // the amplitude EnvAsr's t_restart
        CHECK(knh_bank_param_apply(h, v, 0, 2, KNH_VALUE_TRIGGER, 0.0, 0) == KNH_OK);  // the filter EnvAr's
      }
    }
    float out[2][64];
    CHECK(knh_bank_process_block(h, 64, 0, 64u * block, out, nullptr) == KNH_OK);
    processor->run_without_inputs();
    auto got = processor->output_block();
    for (size_t i = 0; i < 64; ++i) {
      const float l = got.read(0, i), r = got.read(1, i);
      CHECK(std::memcmp(&l, &out[0][i], 4) == 0 && std::memcmp(&r, &out[1][i], 4) == 0);
      peak = std::fmax(peak, std::fabs(out[0][i]));
    }
  }
  CHECK(peak > 1e-3f && std::isfinite(peak));
  knh_bank_destroy(h);
}

int main(int argc, char** argv) {
  bool plan = false, gpu = false;
  for (int i = 1; i < argc; ++i) {
    plan = plan || !std::strcmp(argv[i], "--plan");
    gpu = gpu || !std::strcmp(argv[i], "--gpu");
  }
  if (!plan && !gpu) plan = true;
  if (plan) {
    RUN(plan_filter_envelope_is_a_source_with_its_wrappers);
    RUN(plan_wrapped_envelope_inside_a_product);
    RUN(plan_envelope_read_by_a_product_and_a_link);
    RUN(plan_envelope_on_the_graph_output_and_under_plus);
    RUN(plan_signal_times_envelope_is_still_one_stage);
  }
  if (gpu) {
    if (knh_device_count() < 1) { std::printf("no gfx950 device\n"); return 2; }
    RUN(gpu_filter_envelope_equals_descriptor);
  }
  std::printf("%s (%d failures)\n", g_fail ? "HOST MIRROR ENV SOURCE FAILED" : "HOST MIRROR ENV SOURCE PASSED", g_fail);
  return g_fail ? 1 : 0;
}
