// Feedback edges in the C++ host mirror: what `trace` makes of a.to_feedback(b) / a.to_feedback_replace(b) -- a
// KNH_STAGE_FLAG_FEEDBACK stage that names the tapped node, plus a MATH_ADD where the input already had an edge -- and the
// reference's two vectors (graph_tests.rs:185-254) rendered through the mirror.  TestInPlusParamUGen is `x + value` here, its
// unconnected input a SinWt of 0 Hz (sin(0) = 0 in every frame).  Built and run by tests/test_host_mirror_feedback.py.
//   host_mirror_feedback_test --plan   : no device needed
//   host_mirror_feedback_test --gpu    : the vectors, block by block
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

static const uint16_t FB = KNH_STAGE_FLAG_FEEDBACK;

// knh_stage_desc: kind, flags, delayed_changes_per_block, ar_param, input, input2
template <size_t N>
static void check_plan(const Graph<float>& graph, const knh_stage_desc (&want)[N], int out_l = -1, int out_r = -1) {
  CHECK(graph.num_banks() == 1);
  if (graph.num_banks() != 1) return;
  const auto& b = graph.bank(0);
  CHECK(b.plan.stages.size() == N);
  if (b.plan.stages.size() != N) return;
  for (size_t s = 0; s < N; ++s) {
    const knh_stage_desc& st = b.plan.stages[s];
    CHECK(st.kind == want[s].kind && st.flags == want[s].flags && st.input == want[s].input && st.input2 == want[s].input2 && st.ar_param == want[s].ar_param);
  }
  CHECK(b.plan.out_stage[0] == out_l && b.plan.out_stage[1] == out_r);
}
template <typename Build>
static std::unique_ptr<Graph<float>> planned(Build build) {
  auto [graph, processor] = AudioProcessor<float>::create(2, {16, 48000});
  graph->plan_only = true;
  graph->edit([&](GraphEdit<float>& g) { build(g); });
  return std::move(graph);
}

// feedback_nodes: n0(+1.25) -> n1(+0.125) -> feedback -> n0; n1 to the graph output
template <typename F>
static void vector_later(GraphEdit<F>& g, bool replace) {
  auto n0 = g.push(SinWt(0.0)) + 1.25;
  auto n1 = n0 + 0.125;
  if (replace) n1.to_feedback_replace(n0);
  else n1.to_feedback(n0);
  n1.out({0, 0}).to_graph_out();
}
// feedback_nodes2: n2(+1.25) -> feedback -> n3(+0.125) -> graph output: an edge that needed no feedback is delayed all the same
template <typename F>
static void vector_earlier(GraphEdit<F>& g) {
  auto n2 = g.push(SinWt(0.0)) + 1.25;
  auto n3 = g.push(SinWt(0.0)) + 0.125;
  n2.to_feedback_replace(n3).out({0, 0}).to_graph_out();
}

static void plan_replace_is_the_flagged_stage() {
  auto graph = planned([](GraphEdit<float>& g) { vector_later<float>(g, true); });
  // the edge's source takes the input's place: the 0 Hz oscillator is no longer read, the stage names the tap (stage 2, a later one)
  static const knh_stage_desc want[] = {{KNH_STAGE_INPUT, FB, 0, 0, 3, 0}, {KNH_STAGE_ADD_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_ADD_CONST, 0, 0, 0, 0, 0}};
  check_plan(*graph, want);
  CHECK(knh_chain_ugen_count(want, 3) == 2 + 2 + 2);  // FeedbackSink + FeedbackSource, and a Constant + MathUGen per `+ value`
  CHECK(graph->bank(0).plan.stage_args[0].empty());  // no constructor arguments (no channel)
}
static void plan_additive_is_a_math_add_of_the_two() {
  auto graph = planned([](GraphEdit<float>& g) { vector_later<float>(g, false); });
  static const knh_stage_desc want[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_INPUT, FB, 0, 0, 5, 0}, {KNH_STAGE_MATH_ADD, 0, 0, 0, 1, 2},
                                        {KNH_STAGE_ADD_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_ADD_CONST, 0, 0, 0, 0, 0}};
  check_plan(*graph, want);
}
static void plan_additive_onto_an_empty_input_is_the_edge_alone() {
  auto graph = planned([](GraphEdit<float>& g) {
    auto s = g.push(SinWt(220.0));
    auto lp = g.push(OnePoleLpf(900.0));  // nothing on its input yet
    auto mix = (s + (lp * 0.5));
    mix.to_feedback(lp);
    mix.out({0, 0}).to_graph_out();
  });
  static const knh_stage_desc want[] = {{KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0}, {KNH_STAGE_INPUT, FB, 0, 0, 5, 0}, {KNH_STAGE_ONEPOLE_LPF, 0, 0, 0, 0, 0},
                                        {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_MATH_ADD, 0, 0, 0, 1, 4}};
  check_plan(*graph, want);
}
static void plan_a_node_only_the_edge_reads_comes_behind_the_output() {
  auto graph = planned([](GraphEdit<float>& g) { vector_earlier<float>(g); });
  // n3's stages first (the output's), n2's behind them: the voice's signal is stage 1 on both graph outputs
  static const knh_stage_desc want[] = {{KNH_STAGE_INPUT, FB, 0, 0, 4, 0}, {KNH_STAGE_ADD_CONST, 0, 0, 0, 0, 0}, {KNH_STAGE_SIN_WT, 0, 0, 0, 0, 0},
                                        {KNH_STAGE_ADD_CONST, 0, 0, 0, 0, 0}};
  check_plan(*graph, want, 1, 1);
}
static void plan_refusals() {
  bool threw = false;
  try {
    planned([](GraphEdit<float>& g) {
      auto s = g.push(SinWt(220.0));
      s.to_feedback(g.push(Constant(1.0)));
    });
  } catch (const GraphError&) { threw = true; }
  CHECK(threw);
}

template <typename Build>
static void render(Build build, const float (&want)[3]) {
  auto [graph, processor] = AudioProcessor<float>::create(2, {16, 48000});
  graph->edit([&](GraphEdit<float>& g) { build(g); });
  for (int block = 0; block < 3; ++block) {
    processor->run_without_inputs();
    auto got = processor->output_block();
    for (size_t i = 0; i < 16; ++i) CHECK(got.read(0, i) == want[block] && got.read(1, i) == want[block]);
  }
}
static void gpu_reference_vectors() {
  const float later[3] = {1.375f, 2.75f, 4.125f}, earlier[3] = {0.125f, 1.375f, 1.375f};
  render([](GraphEdit<float>& g) { vector_later<float>(g, true); }, later);
  render([](GraphEdit<float>& g) { vector_later<float>(g, false); }, later);
  render([](GraphEdit<float>& g) { vector_earlier<float>(g); }, earlier);
}

int main(int argc, char** argv) {
  bool plan = false, gpu = false;
  for (int i = 1; i < argc; ++i) {
    plan = plan || !std::strcmp(argv[i], "--plan");
    gpu = gpu || !std::strcmp(argv[i], "--gpu");
  }
  if (!plan && !gpu) plan = true;
  if (plan) {
    RUN(plan_replace_is_the_flagged_stage);
    RUN(plan_additive_is_a_math_add_of_the_two);
    RUN(plan_additive_onto_an_empty_input_is_the_edge_alone);
    RUN(plan_a_node_only_the_edge_reads_comes_behind_the_output);
    RUN(plan_refusals);
  }
  if (gpu) {
    if (knh_device_count() < 1) { std::printf("no gfx950 device\n"); return 2; }
    RUN(gpu_reference_vectors);
  }
  std::printf("%s (%d failures)\n", g_fail ? "HOST MIRROR FEEDBACK FAILED" : "HOST MIRROR FEEDBACK PASSED", g_fail);
  return g_fail ? 1 : 0;
}
