// Reader voices through the C++ host mirror (knaster_amd/host/knaster_host.hpp): voices of one chain shape made on different
// Buffers share a bank whose pool holds every distinct Buffer once.
//   --create : no device needed -- the pool calls are accepted and the edit fails only at knh_bank_init (no CPU path)
//   --gpu    : four looping voices with gains of their own on three Buffers of constants (one Buffer twice): the mix is the
//              expected one only if every voice reads the Buffer it was made on
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../knaster_amd/host/knaster_host.hpp"

using namespace knaster;

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "--gpu") == 0;
  auto a = Buffer<float>::from_vec(std::vector<float>(300, 0.5f), 44100.0);
  auto b = Buffer<float>::from_vec(std::vector<float>(77, -0.25f), 8000.0);
  auto c = Buffer<float>::from_vec(std::vector<float>(5, 0.75f), 96000.0);
  const float gain[4] = {0.5f, 0.25f, 0.125f, 0.0625f}, value[4] = {0.5f, -0.25f, 0.5f, 0.75f};
  auto [graph, processor] = AudioProcessor<float>::create(2, {64, 48000});
  try {
    graph->edit([&](GraphEdit<float>& g) {
      const std::shared_ptr<const Buffer<float>> of[4] = {a, b, a, c};
      for (int i = 0; i < 4; ++i) {
        auto s = g.push(BufferReader<float>(of[i], 1.0 + 0.5 * i, true));
        (s * static_cast<double>(gain[i])).out({0, 0}).to_graph_out();
      }
    });
  } catch (const GraphError& e) {
    if (!gpu && std::string(e.what()).find("no CPU path") != std::string::npos) {
      std::printf("ok   pool accepted, init refused without a device\n");
      return 0;
    }
    std::printf("FAILED: %s\n", e.what());
    return 1;
  }
  if (!gpu) {  // (a machine with a device: the edit went through)
    std::printf("ok   pool accepted\n");
    return 0;
  }
  if (graph->num_banks() != 1 || knh_bank_buffer_count(graph->bank(0).h, 0) != 3) { std::printf("FAILED: one bank, three pooled Buffers expected\n"); return 1; }
  // 0.296875; any other pairing of these voices and Buffers is at least 0.015 away (every product is exact in f32)
  float want = 0.f;
  for (int i = 0; i < 4; ++i) want += gain[i] * value[i];
  for (int blk = 0; blk < 4; ++blk) {
    processor->run_without_inputs();
    // (constants interpolate to themselves up to rounding)
    for (size_t f = 0; f < 64; ++f) {
      const float got = processor->output_block().channel_as_slice(0)[f];
      if (!(std::fabs(got - want) <= 1e-6f)) { std::printf("FAILED: block %d frame %zu: %g, want %g\n", blk, f, got, want); return 1; }
    }
  }
  std::printf("ok   reader voices on their own Buffers\n");
  return 0;
}
