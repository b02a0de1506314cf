// The Wavetable value type and the OscWt node of the C++ host mirror (dsp/wavetable.rs:396-610, ugens/osc.rs:28-87).
// Built and run by tests/test_host_mirror_wavetable.py.
//   host_mirror_wavetable_test --plan   : no device needed -- the builders, and what `trace` makes of an OscWt
//   host_mirror_wavetable_test --gpu    : g.push(OscWt(wt, 220)) renders the blocks of the same bank made through the C ABI
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

// the per-table harmonic limit, (20000 / (32 * 1.5^i)) as usize in f32 (wavetable.rs:378-386)
static const size_t kLimit[17] = {625, 416, 277, 185, 123, 82, 54, 36, 24, 16, 10, 7, 4, 3, 2, 1, 0};

template <typename F>
static bool all_zero(const F* t) {
  for (size_t k = 0; k < kTableSize; ++k)
    if (t[k] != F(0)) return false;
  return true;
}

// Wavetable().add_sine(h, 1, 0) leaves exactly the partial tables with ceil(h) <= limit[i] non-zero and equal to each other
template <typename F>
static void add_sine_case(double h) {
  Wavetable<F> w;
  w.add_sine(h, 1.0, 0.0);
  int first = -1, filled = 0;
  for (size_t i = 0; i < kPartialTables; ++i) {
    const bool want = static_cast<size_t>(std::ceil(h)) <= kLimit[i];
    CHECK(all_zero(w.table(i)) == !want);
    if (!want) continue;
    ++filled;
    if (first < 0) first = static_cast<int>(i);
    CHECK(std::memcmp(w.table(static_cast<size_t>(first)), w.table(i), kTableSize * sizeof(F)) == 0);
  }
  CHECK(filled > 0 && first == 0);
  // the samples: an f64 phase stepped by h * 2 pi / 16384, rounded by F::new (NonAaWavetable::add_sine, :219-226)
  double ph = 0.0;
  const double step = (h * 3.14159265358979323846 * 2.0) / 16384.0;
  for (size_t k = 0; k < 64; ++k) { CHECK(w.table(0)[k] == static_cast<F>(std::sin(ph))); ph += step; }
}
static void cpu_add_sine_fills_the_tables_within_the_harmonic_limit() {
  for (size_t i = 0; i < kPartialTables; ++i) CHECK(kMaxHarmonic[i] == kLimit[i]);
  for (double h : {1.0, 3.0, 17.0, 600.0}) { add_sine_case<float>(h); add_sine_case<double>(h); }
  // 600 <= 625 only: one table; 17: tables 0 .. 8 (24 >= 17 > 16)
  Wavetable<float> w;
  w.add_sine(17.0, 1.0, 0.0);
  CHECK(!all_zero(w.table(8)) && all_zero(w.table(9)));
}
static void cpu_from_buffer_gives_seventeen_equal_tables() {
  std::vector<float> buf(kTableSize);
  for (size_t k = 0; k < kTableSize; ++k) buf[k] = static_cast<float>(k % 97) - 48.0f;
  Wavetable<float> w = Wavetable<float>::from_buffer(buf);
  for (size_t i = 0; i < kPartialTables; ++i) CHECK(std::memcmp(w.table(i), buf.data(), kTableSize * sizeof(float)) == 0);
  CHECK(w.single());
  bool threw = false;
  try { Wavetable<float>::from_buffer(std::vector<float>(100)); } catch (const std::exception&) { threw = true; }
  CHECK(threw);
  CHECK(Wavetable<double>::sine().single() && !Wavetable<float>().add_saw(0, 40, 1.0).single());
}
static void cpu_saw_multiply_normalize() {
  Wavetable<double> w;
  w.add_saw(0, 1000, 1.0);
  // table 15 holds harmonics 0 ..= 1 (its limit), table 16 none (min(1000, 0) > 0 fails): wavetable.rs:545-552
  CHECK(all_zero(w.table(16)) && !all_zero(w.table(15)));
  const double PI = 3.14159265358979323846;
  for (size_t k : {size_t(1), size_t(4097), size_t(16383)}) {
    double want = 0.0;
    for (int h = 0; h <= 1; ++h) want += (std::sin(static_cast<double>(k) / 16384.0 * PI * 2.0 * (h + 1) + 0.0) * (1.0 / ((h + 1) * PI))) * 1.0;
    CHECK(w.table(15)[k] == want);
  }
  Wavetable<double> n = w;
  n.normalize();
  double peak0 = 0.0;
  for (size_t k = 0; k < kTableSize; ++k) peak0 = std::fmax(peak0, std::fabs(n.table(0)[k]));
  CHECK(std::fabs(peak0 - 1.0) < 1e-12);  // by table 0's loudest sample, every table scaled alike
  double loud = 0.0;
  for (size_t k = 0; k < kTableSize; ++k) loud = std::fmax(loud, std::fabs(w.table(0)[k]));
  CHECK(n.table(15)[4097] == w.table(15)[4097] * (1.0 / loud));
  Wavetable<double> m = w;
  m.multiply(0.5);
  CHECK(m.table(3)[77] == w.table(3)[77] * 0.5);
}

static const int kVoices = 5;
static double freq_of(int v) { return 220.0 * (v + 1) + 0.37 * v; }
static std::shared_ptr<const Wavetable<float>> saw() {
  Wavetable<float> w;
  w.add_saw(0, 600, 1.0).normalize();
  return std::make_shared<const Wavetable<float>>(w);
}
static void plan_an_osc_wt_is_a_flagged_sin_wt() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  graph->plan_only = true;
  auto wt = saw();
  graph->edit([&](GraphEdit<float>& g) {
    for (int v = 0; v < kVoices; ++v) {
      auto o = g.push(OscWt(wt, freq_of(v)));
      (o * 0.25).out({0, 0}).to_graph_out();
      o.param("freq");  // its three parameters by name
      o.param("phase_offset");
      o.param("reset_phase");
    }
  });
  CHECK(graph->num_banks() == 1);
  const auto& b = graph->bank(0);
  CHECK(b.n_voices == 5u && b.plan.stages.size() == 2);
  CHECK(b.plan.stages[0].kind == KNH_STAGE_SIN_WT && b.plan.stages[0].flags == KNH_STAGE_FLAG_WAVETABLE);
  CHECK(b.plan.stages[1].kind == KNH_STAGE_MUL_CONST && b.plan.stage_args[0] == std::vector<double>{freq_of(0)});
}

// g.push(OscWt(wt, f)) against the same bank made through the C ABI, block by block, bit for bit
static void gpu_osc_wt_equals_the_c_abi_bank() {
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  auto wt = saw();
  const Wavetable<float> flat = Wavetable<float>::from_buffer(std::vector<float>(wt->table(3), wt->table(3) + kTableSize));
  graph->edit([&](GraphEdit<float>& g) {
    for (int v = 0; v < kVoices; ++v) {  // odd voices on a from_buffer Wavetable of their own each: stored as one table
      auto o = v % 2 ? g.push(OscWt(flat, freq_of(v))) : g.push(OscWt(wt, freq_of(v)));
      (o * 0.25).out({0, 0}).to_graph_out();
    }
  });
  const knh_stage_desc st[2] = {{KNH_STAGE_SIN_WT, KNH_STAGE_FLAG_WAVETABLE, 0, 0, 0, 0}, {KNH_STAGE_MUL_CONST, 0, 0, 0, 0, 0}};
  knh_bank_desc d{};
  d.abi_version = KNH_ABI_VERSION;
  d.n_voices = kVoices;
  d.sample_type = KNH_F32;
  d.n_stages = 2;
  d.stages = st;
  d.out_channels = 2;
  d.mix_mode = KNH_MIX_TREE;
  d.device = -1;
  knh_bank* h = nullptr;
  CHECK(knh_bank_create(&d, &h) == KNH_OK);
  if (!h) { std::printf("  %s\n", knh_last_error(nullptr)); return; }
  uint32_t index = 99;
  CHECK(knh_bank_add_wavetable(h, 0, wt->tables.data(), 17, &index) == KNH_OK && index == 0);
  CHECK(knh_bank_add_wavetable(h, 0, flat.table(0), 1, &index) == KNH_OK && index == 1);
  CHECK(knh_bank_wavetable_count(h, 0) == 2);
  std::vector<double> freq, gain(kVoices, 0.25);
  std::vector<uint32_t> voices, entries;
  for (int v = 0; v < kVoices; ++v) { freq.push_back(freq_of(v)); voices.push_back(v); entries.push_back(v % 2); }
  CHECK(knh_bank_set_ctor_args(h, 0, 0, kVoices, freq.data(), 1) == KNH_OK);
  CHECK(knh_bank_set_ctor_args(h, 1, 0, kVoices, gain.data(), 1) == KNH_OK);
  CHECK(knh_bank_assign_wavetables(h, 0, voices.size(), voices.data(), entries.data(), nullptr) == KNH_OK);
  CHECK(knh_bank_init(h, 48000, 64) == KNH_OK);
  CHECK(graph->num_banks() == 1 && knh_bank_wavetable_count(graph->bank(0).h, 0) == 3);  // wt once, a copy of `flat` per odd voice
  float peak = 0.f;
  for (int block = 0; block < 3; ++block) {
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
    RUN(cpu_add_sine_fills_the_tables_within_the_harmonic_limit);
    RUN(cpu_from_buffer_gives_seventeen_equal_tables);
    RUN(cpu_saw_multiply_normalize);
    RUN(plan_an_osc_wt_is_a_flagged_sin_wt);
  }
  if (gpu) {
    if (knh_device_count() < 1) { std::printf("no gfx950 device\n"); return 2; }
    RUN(gpu_osc_wt_equals_the_c_abi_bank);
  }
  std::printf("%s (%d failures)\n", g_fail ? "HOST MIRROR WAVETABLE FAILED" : "HOST MIRROR WAVETABLE PASSED", g_fail);
  return g_fail ? 1 : 0;
}
