// Compiles ONE chain signature with the library's run-time fusion (hiprtc) and says how it went -- no GPU needed: the compile
// itself is host work, only loading the result asks for a device.  A compiler crash kills this process, not a host's:
// tools/jit_compile_fuzz.py runs it over random voices.  A signature is what knh_bank_debug_signature prints: a chain
// ("WSA"), a graph with its signal slots ("...#R"), a graph with two connected outputs ("...#R:l,r").
//   make -C tests/cpp bin/jit_compile_check
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../include/knaster_hip.h"
#include "jit.hpp"
#include "jit_cache.hpp"    // --sha256: the cache's hash function against a known implementation (tests/test_jit_cache.py)
#include "stage_table.hpp"  // partition_chain: how knh_bank_init cuts a plain chain into pipeline groups
int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: jit_compile_check <signature> [f64] [fma] [pipe | frame] | --sha256 <text>\n"); return 2; }
  if (!std::strcmp(argv[1], "--sha256")) {
    knh_jit::Sha256 h;
    const char* t = argc > 2 ? argv[2] : "";
    h.update(t, std::strlen(t));
    std::puts(h.hex().c_str());
    return 0;
  }
  struct PrintStats {  // where the kernel came from (knh_jit_stats)
    ~PrintStats() {
      uint64_t m = 0, d = 0, h = 0, i = 0;
      knh_jit_stats(&m, &d, &h, &i);
      std::printf("jit stats: memory %llu disk %llu helper %llu in-process %llu\n", (unsigned long long)m, (unsigned long long)d, (unsigned long long)h, (unsigned long long)i);
    }
  } print_stats;
  bool f64 = false, fma = false, pipe = false, frame = false;
  for (int i = 2; i < argc; ++i) { f64 = f64 || !std::strcmp(argv[i], "f64"); fma = fma || !std::strcmp(argv[i], "fma"); pipe = pipe || !std::strcmp(argv[i], "pipe"); frame = frame || !std::strcmp(argv[i], "frame"); }
  std::string err;
  const knh::JitKernel* k = nullptr;
  if (frame) {  // the lane-per-frame kernel a voice of SinWt oscillators and arithmetic gets at init (voice_frame.hpp): a statement per stage
    static const char kinds[] = "masdvq*+-/Wcrftwe";  // kernel_registry.hpp's INTERP_* numbering, by signature character
    std::vector<knh::FrameOp> ops;
    unsigned slot = 0, n_sig = 1;
    const char* p = argv[1];
    while (*p && *p != '#') {
      const char c = *p++;
      const char* at = std::strchr(kinds, c);
      if (!at || !std::strchr(kFrameSigs, c)) { std::printf("FAILED: stage '%c' does not run a lane per frame\n", c); return 1; }
      int v[3] = {c == 'W' ? -1 : 0, -1, 0};  // a plain chain: one signal, in place
      if (*p == '@') {
        ++p;
        for (int j = 0; j < 3; ++j) {
          v[j] = -1;
          if (*p == '_') { ++p; } else { v[j] = 0; while (*p >= '0' && *p <= '9') v[j] = v[j] * 10 + (*p++ - '0'); }
          if (*p == ',') ++p;
        }
      }
      ops.push_back(knh::FrameOp{static_cast<unsigned>(at - kinds), static_cast<unsigned>(std::max(v[0], 0)), static_cast<unsigned>(std::max(v[1], 0)), static_cast<unsigned>(std::max(v[2], 0)), slot});
      for (const KindInfo& ki : kKinds)  // the stage's state words: the first kind with this signature character (kinds that share one share its slots)
        if (ki.sig == c) { slot += static_cast<unsigned>(ki.n_slots); break; }
    }
    if (*p == '#') n_sig = static_cast<unsigned>(std::atoi(p + 1));
    if (ops.empty() || n_sig == 0) { std::puts("FAILED: empty frame voice"); return 1; }
    k = knh::jit_frame_kernel(ops.data(), static_cast<unsigned>(ops.size()), n_sig, ops.back().o, slot, 1, 64, f64, &err);
  } else if (pipe) {  // the pipelined form a plain chain of up to 512 voice groups gets at init
    unsigned cuts[2] = {0, 0};
    const unsigned n_cuts = partition_chain(argv[1], cuts);
    k = knh::jit_pipe_kernel(argv[1], cuts, n_cuts, f64, fma, &err);
  } else {
    k = knh::jit_voice_kernel(argv[1], f64, fma, &err);
  }
  if (k) { std::puts("compiled and loaded"); return 0; }
  // with no device the compile is followed by a failing load: that is a successful compile
  if (err.rfind("hipGetDevice", 0) == 0 || err.rfind("hipModuleLoadData", 0) == 0) { std::puts("compiled"); return 0; }
  std::printf("FAILED: %.1500s\n", err.c_str());
  return 1;
}
