// The host's freq_to_table_index (knaster_amd/csrc/stage_table.hpp wt_table_index: the partial table of a Wavetable a frequency
// reads, dsp/wavetable.rs:329-377) for f32 bit patterns given in hex on the command line: one index per line.  CPU only, no
// library: tests/test_wavetable_abi.py compares the output with its numpy restatement.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/knaster_hip.h"
#include "../../knaster_amd/csrc/stage_table.hpp"
int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const uint32_t bits = static_cast<uint32_t>(std::strtoul(argv[i], nullptr, 16));
    float f;
    std::memcpy(&f, &bits, 4);
    std::printf("%u\n", wt_table_index(f));
  }
  return 0;
}
