// knaster/examples/buffer_player.rs through the C++ host mirror, as written: a two-channel Buffer
// (Buffer::from_vec_interleaved), `BufferReader::<_, U2>::new(buffer, 1.0, false)`, `(play * amp.out([0, 0])).to_graph_out()`,
// then t_restart / looping / start_s / end_s traffic on `play`.  The graph calls trace into ONE connected voice: the reader
// stage, its second output (KNH_STAGE_FLAG_READER_CH1), a MUL_CONST per channel, the two products on graph outputs 0 and 1.
// Built and run by tests/test_host_mirror_buffer_player.py.
//   host_mirror_buffer_player_test --plan   : no device needed
//   host_mirror_buffer_player_test --gpu    : the traced bank renders, block by block under the example's sequence of changes,
//                                             what the hand-written descriptor bank renders
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

static const uint32_t kSampleRate = 48000;
static const size_t kBlock = 64, kFrames = 4800;  // a tenth of a second of stereo
static const double kLength = static_cast<double>(kFrames) / kSampleRate;

// a Buffer of this test's own: two tones and seeded noise, other ones in the right channel
static std::vector<double> stereo_samples() {
  std::vector<double> s(kFrames * 2);
  uint32_t lcg = 12345u;
  auto noise = [&]() { lcg = lcg * 1664525u + 1013904223u; return (static_cast<double>(lcg >> 8) / 8388608.0) - 1.0; };
  for (size_t i = 0; i < kFrames; ++i) {
    const double t = static_cast<double>(i) / kSampleRate;
    s[2 * i] = 0.5 * std::sin(2 * M_PI * 210.0 * t) + 0.25 * std::sin(2 * M_PI * 1333.0 * t + 0.3) + 0.1 * noise();
    s[2 * i + 1] = 0.4 * std::sin(2 * M_PI * 347.0 * t + 1.0) + 0.3 * std::sin(2 * M_PI * 2111.0 * t) + 0.1 * noise();
  }
  return s;
}

// the example's parameter handles, and its sequence of changes with the sleeps turned into block numbers and the times
// scaled to this Buffer (the example's is two seconds long: x kLength / 2)
template <typename P>
struct Handles { P t_restart, looping, start_s, end_s, amp_value; };  // (amp_value: not in the example -- the one Constant that scales both channels)
template <typename H>
static void changes_of_block(int block, H& h) {
  const double k = kLength / 2.0;
  switch (block) {
    case 3: h.t_restart.trig(); h.looping.set(true); break;
    case 6: h.looping.set(false); break;
    case 9: h.t_restart.trig(); h.looping.set(true); h.start_s.set(0.1 * k); h.end_s.set(0.9 * k); break;
    case 12: h.start_s.set(0.3 * k); h.end_s.set(0.5 * k); break;
    case 14: h.start_s.set(1.4 * k); h.end_s.set(1.5 * k); break;
    case 16: h.start_s.set(0.9 * k); h.end_s.set(1.1 * k); h.amp_value.set(0.25); break;  // one Constant: both channels get the new gain
    case 18: h.start_s.set(0.95 * k); h.end_s.set(1.05 * k); break;
    case 20: h.start_s.set(0.975 * k); h.end_s.set(1.025 * k); break;
    default: break;
  }
}
static const int kBlocks = 24;

// the descriptor of the issue's section 2: reader, its second output, a MUL_CONST per channel; outputs 2 and 3 connected
static const knh_stage_desc kPlayer[] = {{KNH_STAGE_BUFFER_READER, 0, 0, 0, 0, 0},
                                         {KNH_STAGE_BUFFER_READER, KNH_STAGE_FLAG_READER_CH1, 0, 0, 1, 0},
                                         {KNH_STAGE_MUL_CONST, 0, 0, 0, 1, 0},
                                         {KNH_STAGE_MUL_CONST, 0, 0, 0, 2, 0}};
static const uint32_t kPlayerOuts[2] = {2, 3};

// the example's graph.edit closure, as written
template <typename F>
static Handles<typename Sig<F>::Parameter> buffer_player(GraphEdit<F>& g, std::shared_ptr<const Buffer<F>> buffer, int* play_node) {
  auto play = g.push(BufferReader<F>(buffer, 1.0, false));
  auto amp = g.push(Constant(0.5));
  (play * amp.out({0, 0})).to_graph_out();
  *play_node = play.node();
  return {play.param("t_restart"), play.param("looping"), play.param("start_s"), play.param("end_s"), amp.param("value")};
}

static void plan_the_example_is_one_connected_voice() {
  auto [graph, processor] = AudioProcessor<double>::create(2, {kBlock, kSampleRate});
  graph->plan_only = true;
  auto buffer = Buffer<double>::from_vec_interleaved(stereo_samples(), 2, kSampleRate);
  CHECK(buffer->num_channels == 2 && buffer->num_frames() == kFrames);
  int play_node = -1;
  graph->edit([&](GraphEdit<double>& g) {
    auto play = g.push(BufferReader<double>(buffer, 1.0, false));
    CHECK(play.nodes().size() == 2 && play.channels()[0] == 0 && play.channels()[1] == 1);  // one node, a handle of two channels
    CHECK(play.nodes()[0] == play.nodes()[1]);
    auto amp = g.push(Constant(0.5));
    auto scaled = play * amp.out({0, 0});
    CHECK(scaled.nodes().size() == 2);
    scaled.to_graph_out();
    play_node = play.node();
  });
  CHECK(graph->num_banks() == 1);
  if (graph->num_banks() != 1) return;
  const auto& b = graph->bank(0);
  CHECK(b.n_voices == 1 && b.plan.stages.size() == 4);
  if (b.plan.stages.size() != 4) return;
  for (size_t s = 0; s < 4; ++s) {
    const knh_stage_desc& st = b.plan.stages[s];
    CHECK(st.kind == kPlayer[s].kind && st.flags == kPlayer[s].flags && st.input == kPlayer[s].input && st.input2 == 0);
    CHECK(st.delayed_changes_per_block == 0 && st.ar_param == 0);
  }
  CHECK(b.plan.out_stage[0] == 2 && b.plan.out_stage[1] == 3);
  CHECK((b.plan.stage_args[0] == std::vector<double>{1.0, 0.0, 0.0}) && b.plan.stage_args[1].empty());
  CHECK((b.plan.stage_args[2] == std::vector<double>{0.5}) && (b.plan.stage_args[3] == std::vector<double>{0.5}));
  // parameters of `play` address the reader stage; the second output has no node behind it
  CHECK(b.plan.stage_node[0] == play_node && b.plan.stage_node[1] == -1);
  CHECK(knh_chain_ugen_count(b.plan.stages.data(), 4) == 5);  // BufferReader + 2 x (Constant + MathUGen): what the header says it counts
}
static void plan_parameter_names_are_the_readers() {
  auto [graph, processor] = AudioProcessor<double>::create(2, {kBlock, kSampleRate});
  graph->plan_only = true;
  auto buffer = Buffer<double>::from_vec_interleaved(stereo_samples(), 2, kSampleRate);
  bool unknown_refused = false;
  graph->edit([&](GraphEdit<double>& g) {
    int node = -1;
    auto h = buffer_player<double>(g, buffer, &node);
    changes_of_block(9, h);  // every kind of value the example sends is accepted by the handles: trigger, bool, float
    auto play2 = g.push(BufferReader<double>(buffer, 1.0, false));
    for (const char* name : {"rate", "looping", "start_s", "duration_s", "end_s", "t_restart"}) (void)play2.param(name);
    try { (void)play2.param("value"); } catch (const GraphError&) { unknown_refused = true; }
    play2.to_graph_out();  // the two channels directly on the two graph outputs: reader + its second output, connected
  });
  CHECK(unknown_refused);
  CHECK(graph->num_banks() == 2);
  if (graph->num_banks() != 2) return;
  const auto& raw = graph->bank(1);
  CHECK(raw.plan.stages.size() == 2 && raw.plan.stages[1].flags == KNH_STAGE_FLAG_READER_CH1 && raw.plan.stages[1].input == 1);
  CHECK(raw.plan.out_stage[0] == 0 && raw.plan.out_stage[1] == 1);
}
static void plan_a_one_channel_buffer_stays_the_mono_reader() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {kBlock, kSampleRate});
  graph->plan_only = true;
  auto mono = Buffer<float>::from_vec(std::vector<float>(100, 0.25f), 44100.0);
  CHECK(mono->num_channels == 1 && mono->num_frames() == 100);
  graph->edit([&](GraphEdit<float>& g) { (g.push(BufferReader<float>(mono, 1.0, true)) * 0.5).out({0, 0}).to_graph_out(); });
  CHECK(graph->num_banks() == 1);
  if (graph->num_banks() != 1) return;
  const auto& b = graph->bank(0);
  CHECK(b.plan.stages.size() == 2 && b.plan.stages[0].flags == 0 && b.plan.stages[1].input == 0 && b.plan.out_stage[0] == -1);
  bool threw = false;
  try { (void)Buffer<float>::from_vec_interleaved(std::vector<float>(9, 0.f), 2, 44100.0); } catch (const std::exception&) { threw = true; }
  CHECK(threw);  // nine samples are not whole stereo frames
}

struct RawHandles {  // the same changes through the C ABI on the hand-written bank: voice 0, the reader stage
  knh_bank* h;
  struct P {
    knh_bank* h; uint32_t index; uint32_t stage; int stage2;  // stage2 >= 0: the same change to a second stage
    void trig() { CHECK(knh_bank_param_apply(h, 0, stage, index, KNH_VALUE_TRIGGER, 0.0, 0) == KNH_OK); }
    void set(bool v) { CHECK(knh_bank_param_apply(h, 0, stage, index, KNH_VALUE_BOOL, 0.0, v ? 1 : 0) == KNH_OK); }
    void set(double v) {
      CHECK(knh_bank_param_apply(h, 0, stage, index, KNH_VALUE_FLOAT, v, 0) == KNH_OK);
      if (stage2 >= 0) CHECK(knh_bank_param_apply(h, 0, static_cast<uint32_t>(stage2), index, KNH_VALUE_FLOAT, v, 0) == KNH_OK);
    }
  } t_restart, looping, start_s, end_s, amp_value;
  explicit RawHandles(knh_bank* b)
      : h(b), t_restart{b, 5, 0, -1}, looping{b, 1, 0, -1}, start_s{b, 2, 0, -1}, end_s{b, 4, 0, -1}, amp_value{b, 0, 2, 3} {}
};

static void gpu_the_example_renders_what_the_descriptor_renders() {
  auto [graph, processor] = AudioProcessor<double>::create(2, {kBlock, kSampleRate});
  auto samples = stereo_samples();
  auto buffer = Buffer<double>::from_vec_interleaved(samples, 2, kSampleRate);
  int play_node = -1;
  std::unique_ptr<Handles<Sig<double>::Parameter>> handles;
  graph->edit([&](GraphEdit<double>& g) { handles.reset(new Handles<Sig<double>::Parameter>(buffer_player<double>(g, buffer, &play_node))); });
  CHECK(graph->num_banks() == 1);
  if (graph->num_banks() != 1) return;
  CHECK(knh_bank_output_stage(graph->bank(0).h, 0) == 2 && knh_bank_output_stage(graph->bank(0).h, 1) == 3);
  CHECK(knh_bank_buffer_count(graph->bank(0).h, 0) == 1);

  knh_bank_desc d{};
  d.abi_version = KNH_ABI_VERSION;
  d.n_voices = 1;
  d.sample_type = KNH_F64;
  d.n_stages = 4;
  d.stages = kPlayer;
  d.out_channels = 2;
  d.mix_mode = KNH_MIX_TREE;
  d.device = -1;
  knh_bank* h = nullptr;
  CHECK(knh_bank_create(&d, &h) == KNH_OK);
  if (!h) { std::printf("  %s\n", knh_last_error(nullptr)); return; }
  CHECK(knh_bank_connect_outputs(h, 2, kPlayerOuts) == KNH_OK);
  const double reader_args[3] = {1.0, 0.0, 0.0}, half = 0.5;
  CHECK(knh_bank_set_ctor_args(h, 0, 0, 1, reader_args, 3) == KNH_OK);
  CHECK(knh_bank_set_ctor_args(h, 2, 0, 1, &half, 1) == KNH_OK && knh_bank_set_ctor_args(h, 3, 0, 1, &half, 1) == KNH_OK);
  uint32_t index = 99;
  CHECK(knh_bank_add_buffer_interleaved(h, 0, samples.data(), kFrames, 2, kSampleRate, &index) == KNH_OK && index == 0);
  CHECK(knh_bank_init(h, kSampleRate, kBlock) == KNH_OK);
  RawHandles raw(h);
  double peak[2] = {0.0, 0.0};
  int differ = 0;
  for (int block = 0; block < kBlocks; ++block) {
    changes_of_block(block, *handles);
    changes_of_block(block, raw);
    double out[2][kBlock];
    CHECK(knh_bank_process_block(h, kBlock, 0, kBlock * block, out, nullptr) == KNH_OK);
    processor->run_without_inputs();
    auto got = processor->output_block();
    for (size_t i = 0; i < kBlock; ++i) {
      const double l = got.read(0, i), r = got.read(1, i);
      CHECK(std::memcmp(&l, &out[0][i], 8) == 0 && std::memcmp(&r, &out[1][i], 8) == 0);
      differ += std::memcmp(&out[0][i], &out[1][i], 8) != 0;
      peak[0] = std::fmax(peak[0], std::fabs(out[0][i]));
      peak[1] = std::fmax(peak[1], std::fabs(out[1][i]));
    }
    // the first sample of the first block is the Buffer's first frame times 0.5, each channel its own
    if (block == 0) CHECK(out[0][0] == samples[0] * 0.5 && out[1][0] == samples[1] * 0.5);
  }
  CHECK(peak[0] > 1e-2 && peak[1] > 1e-2 && std::isfinite(peak[0]) && std::isfinite(peak[1]));
  CHECK(differ > 500);  // a left and a right that are not each other's copy
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
    RUN(plan_the_example_is_one_connected_voice);
    RUN(plan_parameter_names_are_the_readers);
    RUN(plan_a_one_channel_buffer_stays_the_mono_reader);
  }
  if (gpu) {
    if (knh_device_count() < 1) { std::printf("no gfx950 device\n"); return 2; }
    RUN(gpu_the_example_renders_what_the_descriptor_renders);
  }
  std::printf("%s (%d failures)\n", g_fail ? "HOST MIRROR BUFFER PLAYER FAILED" : "HOST MIRROR BUFFER PLAYER PASSED", g_fail);
  return g_fail ? 1 : 0;
}
