// kernels_restart.hip -- knh_bank_restart_voices on the device: the listed voices become freshly constructed nodes.
//
// What the reference does when a voice's envelope reports done (graph.rs:2483-2513, free_node_when_done) and the host pushes
// the same chain for the next note: every node is new -- phases, filter memories, noise seeds, envelope state, delay
// buffers (`vec![F::ZERO; len]`), WrPreciseTiming's next_delay.  The host has run the construction again (Bank::construct_stage,
// the function knh_bank_init runs) and left, in pinned memory, one row of state words per restarted voice; between two
// launches the voices' state is in device memory, so one workgroup per restarted voice puts its row there:
//   state[slot][voice] for every slot, the voice's done frame, its armed delays (the resolver's persistent state,
//   kernels_events.hip), its segment rows, and its delay ring zeroed.
// Not sent as EV_SET events: a whole bank restarted is slots x voices of them against a staging capacity of 2 048 per
// workgroup, and rings and tables are not slots.  No workgroup reads what another writes: no waits, no atomics.
#include <hip/hip_runtime.h>

#include "../../include/knaster_hip.h"
#include "kernel_registry.hpp"

namespace knh {
using namespace knh_dev;

namespace {

constexpr u32 kRestartThreads = 256;

template <typename W>
__global__ void __launch_bounds__(kRestartThreads) restart_voices_kernel(RestartArgs a) {
  const u32 k = blockIdx.x, t = threadIdx.x;
  const u32 v = a.voices[k];
  if (v >= a.n_voices) return;  // (the host has checked)
  W* state = static_cast<W*>(a.state);
  const W* row = static_cast<const W*>(a.words) + static_cast<size_t>(k) * a.n_slots;
  for (u32 s = t; s < a.n_slots; s += kRestartThreads) state[static_cast<long>(s) * a.stride + v] = row[s];
  if (t == 0) a.done_frames[v] = 0xFFFFFFFFu;
  if (a.armed)  // WrPreciseTiming::next_delay of every parameter: a new node has none armed
    for (u32 p = t; p < a.n_params_total; p += kRestartThreads) a.armed[static_cast<size_t>(p) * a.n_voices + v] = 0;
  if (a.seg_table) {
    const u32 n = a.seg_max * 3u;
    for (u32 i = t; i < n; i += kRestartThreads) a.seg_table[static_cast<size_t>(v) * n + i] = a.seg_rows[static_cast<size_t>(k) * n + i];
  }
  if (a.delay_ring) {
    // The voice's rings, one per delay stage, and nothing else: stage r's is [base_r + v * stride_r, + stride_r) samples.
    // Bases and strides are multiples of 32 samples and the allocation 256-byte aligned, so a ring is whole 16-byte pieces
    // from a 128-byte line on; consecutive lanes store consecutive pieces (a wavefront's store is 1 KiB in a row).  The
    // neighbours' rings, the other stages' and the spare ring behind the last one are never touched.
    static_assert(sizeof(a.ring_stride) / sizeof(a.ring_stride[0]) == KNH_MAX_DELAY_STAGES, "a base and a stride per delay stage");
    const size_t word = a.f64 ? 8u : 4u;
    for (u32 r = 0; r < a.n_rings && r < (u32)KNH_MAX_DELAY_STAGES; ++r) {
      const size_t ring_bytes = static_cast<size_t>(a.ring_stride[r]) * word;
      uint4* ring = reinterpret_cast<uint4*>(static_cast<char*>(a.delay_ring) + static_cast<size_t>(a.ring_base[r]) * word + static_cast<size_t>(v) * ring_bytes);
      const size_t n16 = ring_bytes / 16u;
      for (size_t i = t; i < n16; i += kRestartThreads) ring[i] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

}  // namespace

hipError_t launch_restart_voices(const RestartArgs& a, unsigned count, hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (a.f64) hipLaunchKernelGGL(restart_voices_kernel<u64>, dim3(count), dim3(kRestartThreads), 0, s, a);
  else hipLaunchKernelGGL(restart_voices_kernel<u32>, dim3(count), dim3(kRestartThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace knh
