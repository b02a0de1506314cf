// resident_call.hpp -- ResidentCall<F>: the per-block call on a resident launch (voice_chain.hpp, Resident).
// knh_bank_process_block -- the call the reference makes once per block (Task::run, knaster_graph/src/task.rs:25-31) -- of
// a bank on the pipelined kernel form with a mixer wavefront: the first such call launches the kernel, and it stays until
// something else needs the device state (any other entry point that reads it or launches), another bank launches on the
// device, or the host stays away for KNH_RESIDENT_IDLE_US (default 5 000).  KNH_RESIDENT=0: never (a launch per call).
// Which kernel forms can be resident is the bank's business (Bank::res_possible); everything between the host and a kernel
// that is -- the command word, the relay, the granule rows, the fold server, the hand-over of the block -- is kept here.
// Included by bank.hip only.
#pragma once

namespace {

// A resident kernel keeps every CU's LDS: another bank's launch on the same device could not start beside it.  So there is at
// most one per device, and whoever is about to launch anything there asks it to leave first.  One mutex guards every
// transition (a bank is single-caller, but two banks may belong to two threads).
struct ResidentSlot {
  std::mutex mu;
  knh_bank* owner[64] = {};
  void* call[64] = {};
  void (*leave[64])(void*) = {};
};
inline ResidentSlot& resident_slot() {
  static ResidentSlot s;
  return s;
}

template <typename F>
struct ResidentCall {
  // What the bank hands over, once, when its kernel form is chosen.
  struct Setup {
    knh_bank* bank;               // fail() / warn(), the device, and the slot's owner key
    hipStream_t own_stream;       // the voice kernel's
    uint32_t n_rows;              // 64-voice rows
    uint32_t fold_planes, out_channels, block_size, tile_frames;
    bool can_finish;              // the chain has a stage that can end a voice (chain_can_finish)
    uint32_t* const* ev_start;    // the bank's two pinned event lists: [2] each, read at every launch
    Event* const* events;
    // launches the bank's voice kernel, in whatever form it has, as a resident one on own_stream
    std::function<hipError_t(const knh_dev::Resident&)> launch_voice;
  };

  ResidentCall() = default;
  ResidentCall(const ResidentCall&) = delete;
  ResidentCall& operator=(const ResidentCall&) = delete;
  ~ResidentCall() {
    if (!cfg.bank) return;
    (void)hipSetDevice(cfg.bank->device);
    (void)leave();  // (both kernels have then ended: nothing reads what is freed here)
    if (res_stream) { (void)hipStreamSynchronize(res_stream); (void)hipStreamDestroy(res_stream); }
    void* dev[] = {bell_is_device ? static_cast<void*>(bell) : nullptr, d_relay, d_rows, d_wg_flags, d_group_rows, d_group_flags, d_arrivals, d_group_arrivals};
    for (void* p : dev) if (p) (void)hipFree(p);
    void* host[] = {bell_is_device ? nullptr : static_cast<void*>(bell), h_out, h_done};
    for (void* p : host) if (p) (void)hipHostFree(p);
  }
  void setup(const Setup& s) { cfg = s; }

  // KNH_RESIDENT, and the kernels having started side by side the one time they were tried
  bool enabled() {
    if (policy < 0) {
      const char* e = std::getenv("KNH_RESIDENT");
      policy = e && e[0] == '0' ? 0 : 1;
    }
    return policy == 1;
  }
  // not sitting out calls after another bank asked this one to leave
  bool ready() const { return cooldown.load(std::memory_order_relaxed) == 0; }
  // a call that went the launch-per-call way: one fewer to sit out
  void sat_out() {
    uint32_t c = cooldown.load(std::memory_order_relaxed);
    if (c) cooldown.compare_exchange_strong(c, c - 1, std::memory_order_relaxed);  // (lost to an eviction just now: its 256 stands)
  }
  void stats(uint64_t* c, uint64_t* l) const { if (c) *c = calls; if (l) *l = launches; }
  // diagnostics: the last call's milestones on the device clock (ticks of 10 ns): the voice kernel saw the command, the fold
  // server's root did, its first tile was complete, its last tile was, it had written everything
  void trace(uint64_t* five) const {
    for (int k = 0; k < 5; ++k) five[k] = 0;
    if (!h_done) return;
    for (int k = 0; k < 5; ++k) std::memcpy(&five[k], h_done + 8 + 2 * k, 8);
  }

  // The resident kernel, if one is running, ends; the voices' state is in device memory when this returns.
  int leave() {
    if (!on.load(std::memory_order_relaxed)) return KNH_OK;
    std::lock_guard<std::mutex> lock(resident_slot().mu);
    return leave_locked(false);
  }
  // before `bank` launches anything on `device`: no other bank's resident kernel is in the way
  static void make_room(int device, const knh_bank* bank) {
    ResidentSlot& rs = resident_slot();
    if (device < 0 || device >= 64) return;
    std::lock_guard<std::mutex> lock(rs.mu);
    if (rs.owner[device] && rs.owner[device] != bank) rs.leave[device](rs.call[device]);
  }

  // One block through the resident kernel: frames [fb, fe) of the block into out_host ([channels][block_size], written at
  // their place).  which_list: which of the bank's two pinned event lists holds the call's events (n_ranges of them range
  // events, 0: per-voice lists), -1: none.  KNH_ERR_UNSUPPORTED_CHAIN: the kernels would not run side by side; nothing was
  // rendered, and this bank takes the launch per call from now on.
  int call(uint32_t fb, uint32_t fe, int which_list, uint32_t n_ranges, void* out_host, uint32_t* out_flags) {
    ResidentSlot& rs = resident_slot();
    std::lock_guard<std::mutex> lock(rs.mu);
    const int device = cfg.bank->device;
    KNH_HIP(hipSetDevice(device));
    { int rc = alloc(); if (rc != KNH_OK) return rc; }
    if (device >= 0 && device < 64 && rs.owner[device] && rs.owner[device] != cfg.bank) rs.leave[device](rs.call[device]);
    const bool have_events = which_list >= 0;
    const uint64_t payload = (static_cast<uint64_t>(fb) << 24) | (static_cast<uint64_t>(fe) << 40) | (have_events ? 1ull << 56 : 0ull) |
                             (which_list == 1 ? 1ull << 57 : 0ull) | (have_events ? static_cast<uint64_t>(n_ranges & 15u) << 59 : 0ull);
    uint32_t ep = 0;
    auto ring = [&]() -> int {  // the next epoch's command; a kernel to take it if there is none
      epoch = (epoch + 1u) & 0xFFFFFFu;
      ep = epoch;
      if (!on.load(std::memory_order_relaxed)) { int rc = launch(ep); if (rc != KNH_OK) return rc; }  // (KNH_ERR_UNSUPPORTED_CHAIN: no resident launch for this bank after all)
#if defined(__x86_64__)
      __builtin_ia32_sfence();  // the event list is in memory before the word that announces it
#endif
      __atomic_store_n(bell, static_cast<uint64_t>(ep) | payload, __ATOMIC_RELEASE);
#if defined(__x86_64__)
      if (bell_is_device) __builtin_ia32_sfence();
#endif
      return KNH_OK;
    };
    { int rc = ring(); if (rc != KNH_OK) return rc; }
    calls += 1;
    const auto t0 = std::chrono::steady_clock::now();
    // Waits for something the device stores (`ready`): 0 = there; kRestart = the kernel had ended by itself and the command has
    // gone out again under a new epoch (whatever was read so far belongs to no call: start over); anything else = an error.
    constexpr int kRestart = -12345;
    auto wait_for = [&](auto&& ready) -> int {
      for (uint64_t spin = 1;; ++spin) {
        if (ready()) return 0;
        if ((spin & 0x3FFFu) == 0) {
          const hipError_t q = hipStreamQuery(cfg.own_stream);
          if (q == hipSuccess) {
            // The kernel has ended by itself (the host was away for longer than its patience) just as this command was written.
            // Its workgroup 0 left "leave" in the relay under THIS epoch, so the command goes out again under the next one, to a
            // new launch.
            if (ready()) return 0;
            if (debug()) std::fprintf(stderr, "[knh resident] the kernel ended without answering epoch %u (done word %u, %.3f ms into the call, server stream %s; root wavefronts at %x %x %x %x)\n", ep, h_done[0],
                                      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), hipStreamQuery(res_stream) == hipSuccess ? "idle" : "busy",
                                      h_done[20], h_done[21], h_done[22], h_done[23]);
            // (its fold server has then heard "leave" over the relay too.  A server that is still busy was in the middle of a
            // call: the voice kernel took the command, and taking it again would render the block twice.)
            hipError_t qs = hipStreamQuery(res_stream);
            for (int k = 0; k < 200 && qs == hipErrorNotReady; ++k) { std::this_thread::sleep_for(std::chrono::microseconds(500)); qs = hipStreamQuery(res_stream); }
            on.store(false, std::memory_order_relaxed);
            if (qs != hipSuccess) {
              policy = 0;
              (void)leave_locked(false);
              return fail(KNH_ERR_DEVICE, "the resident voice kernel ended in the middle of a call (its mix never arrived)");
            }
            int rc = ring();
            if (rc != KNH_OK) return rc;
            return kRestart;
          } else if (q != hipErrorNotReady) {
            on.store(false, std::memory_order_relaxed);
            return fail(KNH_ERR_DEVICE, std::string("hipStreamQuery: ") + hipGetErrorString(q));
          }
          if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 10.0) {
            return fail(KNH_ERR_DEVICE, "the resident kernel did not answer within 10 s");
          }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
    };
    // The block arrives tile by tile as granules {sample bits, tag = epoch << 8 | tile}: every frame is taken the moment its
    // tag is there (the early tiles while the kernel is still at the later ones), a mono mix copied to every channel; the
    // call's done / running counts come as one more granule behind the last tile.
    constexpr size_t W = sizeof(F) == 8 ? 2 : 1;
    const size_t block_size = cfg.block_size;
    const uint32_t n = fe - fb, tf = cfg.tile_frames, planes = cfg.fold_planes, out_channels = cfg.out_channels;
    F* const out = static_cast<F*>(out_host);
    uint64_t flag_word = 0;
    for (bool again = true; again;) {
      again = false;
      for (uint32_t rel = 0; rel < n && !again; ++rel) {
        const uint32_t tag = (ep << 8) | ((rel / tf) & 0xFFu);
        for (uint32_t p = 0; p < planes && !again; ++p) {
          volatile uint64_t* g = h_out + (static_cast<size_t>(p) * block_size + fb + rel) * W;
          // (the device's stores took these lines out of the CPU's caches: a tile that has landed is eight cache misses in a row
          // unless they are asked for together -- 0.7 us at the end of every call)
          if ((reinterpret_cast<uintptr_t>(g) & 63u) == 0) {
            __builtin_prefetch(const_cast<const uint64_t*>(g) + 8, 0, 3);
            __builtin_prefetch(const_cast<const uint64_t*>(g) + 16, 0, 3);
            __builtin_prefetch(const_cast<const uint64_t*>(g) + 24, 0, 3);
            __builtin_prefetch(const_cast<const uint64_t*>(g) + 32, 0, 3);
          }
          uint64_t w0 = 0, w1 = 0;
          auto ready = [&]() -> bool {
            w0 = __atomic_load_n(g, __ATOMIC_RELAXED);
            if (static_cast<uint32_t>(w0 >> 32) != tag) return false;
            if (W == 2) { w1 = __atomic_load_n(g + 1, __ATOMIC_RELAXED); if (static_cast<uint32_t>(w1 >> 32) != tag) return false; }
            return true;
          };
          if (!ready()) {
            const int rc = wait_for(ready);
            if (rc == kRestart) { again = true; break; }
            if (rc != 0) return rc;
          }
          F v;
          if (W == 1) { const uint32_t bits = static_cast<uint32_t>(w0); std::memcpy(&v, &bits, sizeof(F) < 4 ? sizeof(F) : 4); }
          else { const uint64_t bits = (w0 & 0xFFFFFFFFull) | (w1 << 32); std::memcpy(&v, &bits, sizeof(F)); }
          if (planes == 2) out[static_cast<size_t>(p) * block_size + fb + rel] = v;
          else for (uint32_t c = 0; c < out_channels; ++c) out[static_cast<size_t>(c) * block_size + fb + rel] = v;
        }
      }
      if (again) continue;
      volatile uint64_t* gf = h_out + static_cast<size_t>(planes) * block_size * W;
      const uint32_t ftag = (ep << 8) | 255u;
      auto fready = [&]() -> bool { flag_word = __atomic_load_n(gf, __ATOMIC_RELAXED); return static_cast<uint32_t>(flag_word >> 32) == ftag; };
      if (!fready()) {
        const int rc = wait_for(fready);
        if (rc == kRestart) { again = true; continue; }
        if (rc != 0) return rc;
      }
    }
    if (out_flags) *out_flags = done_flags(static_cast<uint32_t>(flag_word) & 0xFFFFu, (static_cast<uint32_t>(flag_word) >> 16) & 0xFFFFu, cfg.can_finish);
    return KNH_OK;
  }

 private:
  int fail(int code, const std::string& msg) { return cfg.bank->fail(code, msg); }
  static bool debug() { static const bool d = std::getenv("KNH_DEBUG_RES") != nullptr; return d; }
  static hipError_t launch_server(const knh_dev::ResServerArgs<float>& a, hipStream_t s) { return knh::launch_res_server_f32(a, s); }
  static hipError_t launch_server(const knh_dev::ResServerArgs<double>& a, hipStream_t s) { return knh::launch_res_server_f64(a, s); }
  static void leave_thunk(void* self) { static_cast<ResidentCall<F>*>(self)->leave_locked(true); }
  // the caller holds resident_slot().mu
  int leave_locked(bool evicted) {
    if (!on.load(std::memory_order_relaxed)) return KNH_OK;
    const int device = cfg.bank->device;
    KNH_HIP(hipSetDevice(device));
    epoch = (epoch + 1u) & 0xFFFFFFu;
    const uint64_t cmd = static_cast<uint64_t>(epoch) | (1ull << 58);
    __atomic_store_n(bell, cmd, __ATOMIC_RELEASE);
#if defined(__x86_64__)
    if (bell_is_device) __builtin_ia32_sfence();
#endif
    hipError_t e = hipStreamSynchronize(cfg.own_stream);  // (bounded on the device side: every wait of the kernels is)
    const hipError_t e2 = hipStreamSynchronize(res_stream);
    if (e == hipSuccess) e = e2;
    on.store(false, std::memory_order_relaxed);
    ResidentSlot& rs = resident_slot();
    if (device >= 0 && device < 64 && rs.owner[device] == cfg.bank) { rs.owner[device] = nullptr; rs.call[device] = nullptr; rs.leave[device] = nullptr; }
    if (evicted) cooldown.store(256, std::memory_order_relaxed);
    if (e != hipSuccess) return fail(KNH_ERR_DEVICE, std::string("the resident kernel ended with an error: ") + hipGetErrorString(e));
    return KNH_OK;
  }
  int alloc() {
    if (h_done) return KNH_OK;
    const int device = cfg.bank->device;
    int large_bar = 0;
    (void)hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, device);
    if (large_bar) {
      void* p = nullptr;
      if (hipExtMallocWithFlags(&p, 64, hipDeviceMallocFinegrained) == hipSuccess && p) {
        KNH_HIP(hipMemset(p, 0xFF, 64));
        KNH_HIP(hipDeviceSynchronize());
        bell = bell_dev = static_cast<uint64_t*>(p);
        bell_is_device = true;
      }
    }
    if (!bell) {  // (a device without a large BAR: the command word in mapped host memory)
      KNH_HIP(hipHostMalloc(&bell, 64, hipHostMallocMapped | hipHostMallocCoherent));
      bell_dev = bell;
      *bell = ~0ull;
    }
    max_tiles = (cfg.block_size + cfg.tile_frames - 1) / cfg.tile_frames;
    {
      // granules: every one starts with a tag no call will ever carry (all ones)
      const size_t w = sizeof(F) == 8 ? 2 : 1, rows = cfg.n_rows;
      const size_t n_rows = static_cast<size_t>(max_tiles) * 2 * rows * 64 * w, n_group = static_cast<size_t>(max_tiles) * 2 * 8 * 64 * w;
      KNH_HIP(hipMalloc(&d_rows, n_rows * 8));
      KNH_HIP(hipMemset(d_rows, 0xFF, n_rows * 8));
      KNH_HIP(hipMalloc(&d_group_rows, n_group * 8));
      KNH_HIP(hipMemset(d_group_rows, 0xFF, n_group * 8));
      KNH_HIP(hipMalloc(&d_wg_flags, rows * 8));
      KNH_HIP(hipMemset(d_wg_flags, 0xFF, rows * 8));
      KNH_HIP(hipMalloc(&d_group_flags, 64));
      KNH_HIP(hipMemset(d_group_flags, 0xFF, 64));
      KNH_HIP(hipMalloc(&d_arrivals, (static_cast<size_t>(max_tiles) + 1) * 8 * sizeof(uint32_t)));
      KNH_HIP(hipMemset(d_arrivals, 0, (static_cast<size_t>(max_tiles) + 1) * 8 * sizeof(uint32_t)));
      KNH_HIP(hipMalloc(&d_group_arrivals, (static_cast<size_t>(max_tiles) + 1) * sizeof(uint32_t)));
      KNH_HIP(hipMemset(d_group_arrivals, 0, (static_cast<size_t>(max_tiles) + 1) * sizeof(uint32_t)));
      // The fold server must run BESIDE the voice kernel, so it must not sit behind it in one hardware queue (the runtime
      // multiplexes streams onto a few).  A stream of another priority gets a queue of its own; launch() checks that both
      // kernels have started before anything relies on it.
      int prio_low = 0, prio_high = 0;
      (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
      if (hipStreamCreateWithPriority(&res_stream, hipStreamNonBlocking, prio_high) != hipSuccess) KNH_HIP(hipStreamCreateWithFlags(&res_stream, hipStreamNonBlocking));
    }
    KNH_HIP(hipMalloc(&d_relay, 1024));  // the command word, and (words 16 ..) a call's range events (voice_chain.hpp RES_RELAY_RANGES)
    KNH_HIP(hipMemset(d_relay, 0xFF, 1024));
    {
      const size_t n_gran = 2 * static_cast<size_t>(cfg.block_size) * (sizeof(F) == 8 ? 2 : 1) + 8;
      KNH_HIP(hipHostMalloc(&h_out, n_gran * sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent));
      std::memset(h_out, 0xFF, n_gran * sizeof(uint64_t));  // (a tag no call carries)
    }
    uint32_t* done = nullptr;
    KNH_HIP(hipHostMalloc(&done, 256, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(done, 0, 256);
    done[0] = 0xFFFFFFFFu; done[1] = 0u; done[2] = 0u; done[4] = 0xFFFFFFFFu; done[5] = 0xFFFFFFFFu;
    KNH_HIP(hipDeviceSynchronize());
    if (const char* e = std::getenv("KNH_RESIDENT_IDLE_US")) { const long us = std::atol(e); if (us >= 50 && us <= 2000000) idle_ticks = static_cast<uint64_t>(us) * 100u; }
    h_done = done;
    return KNH_OK;
  }
  // the caller holds resident_slot().mu; the command word already carries `first_epoch`'s command or will
  int launch(uint32_t first_epoch) {
    if (debug()) std::fprintf(stderr, "[knh resident] launch, first epoch %u, %u voice rows, tile %u frames\n", first_epoch, cfg.n_rows, cfg.tile_frames);
    knh_dev::Resident r{};
    r.bell = reinterpret_cast<const knh_dev::u64*>(bell_dev);
    r.relay = reinterpret_cast<knh_dev::u64*>(d_relay);
    r.rows = reinterpret_cast<knh_dev::u64*>(d_rows);
    r.wg_flags = reinterpret_cast<knh_dev::u64*>(d_wg_flags);
    for (int k = 0; k < 2; ++k) { r.ev_start[k] = cfg.ev_start[k]; r.events[k] = cfg.events[k]; }
    r.idle_ticks = idle_ticks;
    r.host_started = h_done + 4;
    r.first_epoch = first_epoch;
    r.max_tiles = max_tiles;
    // (0: only workgroup 0 reads the host's word, also when it lives in device memory.  With every workgroup reading it, a
    // command that arrives just as workgroup 0 gives up waiting would be taken by some workgroups and not by it: the relay makes
    // workgroup 0 the one place where "this command" or "leave" is decided.  Costs 0.5 us per call.)
    r.bell_is_device = 0u;
    {  // the fold server first: a handful of wavefronts that will sit beside the voice kernel's workgroups
      knh_dev::ResServerArgs<F> sa{};
      sa.relay = reinterpret_cast<const knh_dev::u64*>(d_relay);
      sa.bell = nullptr;  // (as for the voice kernel: the relay decides)
      sa.rows = reinterpret_cast<const knh_dev::u64*>(d_rows);
      sa.wg_flags = reinterpret_cast<const knh_dev::u64*>(d_wg_flags);
      sa.group_rows = reinterpret_cast<knh_dev::u64*>(d_group_rows);
      sa.group_flags = reinterpret_cast<knh_dev::u64*>(d_group_flags);
      sa.host_out = reinterpret_cast<knh_dev::u64*>(h_out);
      sa.host_done = h_done;
      sa.idle_ticks = idle_ticks;
      sa.first_epoch = first_epoch;
      sa.n_rows = cfg.n_rows;
      sa.planes = cfg.fold_planes;
      sa.out_channels = cfg.out_channels;
      sa.block_size = cfg.block_size;
      sa.tile_frames = cfg.tile_frames;
      KNH_HIP(launch_server(sa, res_stream));
    }
    KNH_HIP(cfg.launch_voice(r));
    on.store(true, std::memory_order_relaxed);
    launches += 1;
    ResidentSlot& rs = resident_slot();
    const int device = cfg.bank->device;
    if (device >= 0 && device < 64) { rs.owner[device] = cfg.bank; rs.call[device] = this; rs.leave[device] = &ResidentCall<F>::leave_thunk; }
    // Both kernels are running?  (If the two streams share a hardware queue, the second kernel waits for the first to END --
    // which, for kernels that wait for each other's work, is never in time.  Then this bank keeps to a launch per call.)
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spin = 0;; ++spin) {
      if (__atomic_load_n(&h_done[4], __ATOMIC_ACQUIRE) == first_epoch && __atomic_load_n(&h_done[5], __ATOMIC_ACQUIRE) == first_epoch) break;
      if ((spin & 0xFFu) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.05) {
        if (debug()) std::fprintf(stderr, "[knh resident] handshake failed: voice %u server %u (want %u)\n", h_done[4], h_done[5], first_epoch);
        policy = 0;
        cfg.bank->warn("the resident voice kernel and its fold server did not start side by side (a shared hardware queue?): this bank launches per call");
        int rc = leave_locked(false);
        return rc != KNH_OK ? rc : KNH_ERR_UNSUPPORTED_CHAIN;  // (call: the bank falls back to an ordinary launch)
      }
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
    }
    return KNH_OK;
  }

  Setup cfg{};
  int policy = -1;                     // -1 not decided, 0 never, 1 where possible
  // `on` and `cooldown` are also written by another bank's thread, through the slot's eviction (leave_thunk, under the slot
  // mutex); the owner looks at each once per call without the mutex, hence atomics (relaxed: the mutex orders everything else)
  std::atomic<bool> on{false};         // a resident kernel is running (or has ended by itself) on own_stream
  std::atomic<uint32_t> cooldown{0};   // calls to sit out after another bank asked this one to leave
  uint32_t epoch = 0;                  // the last epoch handed out (24 bits); under the slot mutex
  uint64_t* bell = nullptr;            // the command word as the host writes it ...
  uint64_t* bell_dev = nullptr;        // ... and as the kernel reads it (the same fine-grained device word behind a large BAR; else mapped pinned memory)
  bool bell_is_device = false;
  uint64_t* d_relay = nullptr;
  uint64_t *d_rows = nullptr, *d_wg_flags = nullptr, *d_group_rows = nullptr, *d_group_flags = nullptr;  // granules (voice_chain.hpp)
  uint32_t *d_arrivals = nullptr, *d_group_arrivals = nullptr;
  hipStream_t res_stream = nullptr;    // the fold server runs beside the voice kernel
  uint64_t* h_out = nullptr;           // mapped pinned: the block as the fold server's root leaves it, granules {sample bits, tag}: [plane][block_size][W], then the flags granule
  uint32_t* h_done = nullptr;          // mapped pinned: epoch, done count, running count
  uint32_t max_tiles = 0;
  uint64_t idle_ticks = 500000;        // 5 ms of the 100 MHz clock
  uint64_t calls = 0, launches = 0;
};

}  // namespace
