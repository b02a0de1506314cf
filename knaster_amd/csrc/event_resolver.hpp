// event_resolver.hpp -- DevEventResolver: WrPreciseTiming change queues resolved on the device (kernels_events.hip).
// Stages wrapped in WrPreciseTiming whose setters need no host library call (SinWt, SinNumeric, constants and wr_mul,
// the EnvAsr / EnvAr times and triggers): the host appends the call's record to pinned memory and that is all; armed
// delays, queue order, capacity, the patches and the per-voice lists are the resolver kernels' (KNH_DEV_EVENTS=0: the host's,
// as in round 2).  Stages that do need the host (SvfFilter: tan, one-pole: exp, ...) keep the host path (Bank::qfuture,
// resolve_qrecs); a node's queue lives in exactly one of the two places, and the bank decides which.  Included by bank.hip only.
#pragma once

namespace {

// Calls to a node wrapped in WrPreciseTiming (and in nothing that keeps host state of its own): one compact record per
// call, per block in arrival order.
struct QRec {         // (the same bytes as knh_dev::DevRec: records of device-resolved stages are read by the resolver kernels as they are)
  uint32_t voice;
  uint16_t delay;     // set_delay_within_block_for_param value, when `arm` is set
  uint16_t stage;     // (graph-shaped voices hold up to 512 stages, frame-parallel ones 4 096)
  uint8_t param;
  uint8_t kb;         // bits 0-3 ParameterValue kind, bit 4 arm, bit 5 has a value
  uint16_t block;     // device-resolved stages: the block of the launch the call is addressed to
  uint32_t pad;
  union { double f; int64_t i; } v;
  uint32_t kind() const { return kb & 15u; }
  bool arm() const { return (kb & 0x10u) != 0; }
  bool has_value() const { return (kb & 0x20u) != 0; }
};
static_assert(sizeof(QRec) == sizeof(knh_dev::DevRec) && offsetof(QRec, v) == offsetof(knh_dev::DevRec, value) &&
              offsetof(QRec, block) == offsetof(knh_dev::DevRec, block) && offsetof(QRec, kb) == offsetof(knh_dev::DevRec, kb), "QRec is DevRec");

struct DevEventResolver {
  struct Setup {
    knh_bank* bank;  // fail() and the device
    uint32_t n_voices, n_params_total, block_size, sample_rate;
    bool f64;
    double f2pi;
  };
  // The per-voice lists of one launch, as the voice kernel's arguments take them.
  struct Lists { const uint32_t* ev_start; const Event* events; };

  DevEventResolver() = default;
  DevEventResolver(const DevEventResolver&) = delete;
  DevEventResolver& operator=(const DevEventResolver&) = delete;
  // The owner has made the streams that read these buffers idle (quiesce(), and the stream of its last launch).
  ~DevEventResolver() {
    if (!ev_stream) return;
    (void)hipSetDevice(cfg.bank->device);
    quiesce();
    void* dev[] = {d_stages, d_armed, d_ev_cnt, d_rec_start, d_out_start[0], d_out_start[1], d_keys, d_recs, d_out_events[0], d_out_events[1]};
    for (void* p : dev)
      if (p) (void)hipFree(p);
    for (int b = 0; b < 2; ++b) {
      if (recs_done[b]) (void)hipEventDestroy(recs_done[b]);
      if (lists_free[b]) (void)hipEventDestroy(lists_free[b]);
      if (h_recs2[b]) (void)hipHostFree(h_recs2[b]);
    }
    if (h_overflow) (void)hipHostFree(h_overflow);
    (void)hipStreamDestroy(ev_stream);
  }

  // `stages`: the table the kernels read, widx >= 0 for the stages resolved here.
  int init(const Setup& setup, const std::vector<knh_dev::DevStage>& stages) {
    cfg = setup;
    const size_t nv = cfg.n_voices;
    KNH_HIP(hipStreamCreateWithFlags(&ev_stream, hipStreamNonBlocking));
    KNH_HIP(hipMalloc(&d_stages, stages.size() * sizeof(knh_dev::DevStage)));
    KNH_HIP(hipMemcpy(d_stages, stages.data(), stages.size() * sizeof(knh_dev::DevStage), hipMemcpyHostToDevice));
    KNH_HIP(hipHostMalloc(&h_overflow, 64, hipHostMallocMapped | hipHostMallocCoherent));
    *h_overflow = 0u;
    KNH_HIP(hipMalloc(&d_armed, static_cast<size_t>(cfg.n_params_total) * nv * sizeof(uint16_t)));
    KNH_HIP(hipMemset(d_armed, 0, static_cast<size_t>(cfg.n_params_total) * nv * sizeof(uint16_t)));
    KNH_HIP(hipMalloc(&d_ev_cnt, nv * 3 * sizeof(uint32_t)));
    KNH_HIP(hipMemset(d_ev_cnt, 0, nv * 3 * sizeof(uint32_t)));  // (kept zero by the resolver's last pass)
    KNH_HIP(hipMalloc(&d_rec_start, (nv + 1) * sizeof(uint32_t)));
    for (int b = 0; b < 2; ++b) {
      KNH_HIP(hipMalloc(&d_out_start[b], (nv + 1) * sizeof(uint32_t)));
      KNH_HIP(hipEventCreateWithFlags(&recs_done[b], hipEventDisableTiming));
      KNH_HIP(hipEventCreateWithFlags(&lists_free[b], hipEventDisableTiming));
    }
    return KNH_OK;
  }
  bool active() const { return ev_stream != nullptr; }
  bool pending() const { return n_recs > 0; }
  void quiesce() { if (ev_stream) (void)hipStreamSynchronize(ev_stream); }
  // a resolver kernel of an earlier launch found a change queue full and dropped the change
  bool take_overflow() {
    if (!h_overflow || __atomic_load_n(h_overflow, __ATOMIC_RELAXED) == 0u) return false;
    __atomic_store_n(h_overflow, 0u, __ATOMIC_RELAXED);
    return true;
  }

  // Room for `more` records behind those already there; tail() is then where they go, commit() counts them in.  (A batch
  // writes its records in place: knh_bank_param_apply_many.)
  int reserve(size_t more) {
    const unsigned b = recs_parity;
    if (n_recs + more <= h_recs_cap[b]) return KNH_OK;
    const size_t cap = std::max<size_t>((n_recs + more) * 2, 16384);
    QRec* fresh = nullptr;
    KNH_HIP(hipSetDevice(cfg.bank->device));
    KNH_HIP(hipHostMalloc(&fresh, cap * sizeof(QRec)));
    if (n_recs) std::memcpy(fresh, h_recs2[b], n_recs * sizeof(QRec));
    if (h_recs2[b]) KNH_HIP(hipHostFree(h_recs2[b]));  // (the buffer being filled is not one a kernel reads)
    h_recs2[b] = fresh;
    h_recs_cap[b] = cap;
    h_recs = fresh;
    return KNH_OK;
  }
  QRec* tail() { return h_recs + n_recs; }
  void commit(size_t n, uint32_t block_offset) {
    n_recs += n;
    recs_max_block = std::max(recs_max_block, block_offset);
  }
  int push(uint32_t block_offset, QRec r) {
    int rc = reserve(1);
    if (rc != KNH_OK) return rc;
    r.block = static_cast<uint16_t>(block_offset);
    *tail() = r;
    commit(1, block_offset);
    return KNH_OK;
  }

  // The launch's records -> the per-voice event lists in device memory, merged with the host-made list (host_start /
  // host_events, pinned; host_start null: none).  Enqueued on a stream of the resolver's own; `s`, the voice kernel's,
  // waits for it.  *out: what the voice kernel reads.
  int resolve(hipStream_t s, uint32_t n_blocks, uint32_t fb, uint32_t fe, const uint32_t* host_start, const Event* host_events, size_t host_total, Lists* out) {
    const unsigned b = recs_parity;
    size_t n_now = n_recs;
    if (recs_max_block >= n_blocks) {  // calls addressed beyond this launch: they wait, in the other buffer, for the next one
      const unsigned o = b ^ 1u;
      if (recs_busy[o]) { KNH_HIP(hipEventSynchronize(recs_done[o])); recs_busy[o] = false; }
      size_t keep = 0, later = 0;
      for (size_t i = 0; i < n_recs; ++i) later += h_recs[i].block >= n_blocks;
      if (later > h_recs_cap[o]) {
        if (h_recs2[o]) KNH_HIP(hipHostFree(h_recs2[o]));
        h_recs2[o] = nullptr;
        h_recs_cap[o] = std::max<size_t>(later * 2, 16384);
        KNH_HIP(hipHostMalloc(&h_recs2[o], h_recs_cap[o] * sizeof(QRec)));
      }
      later = 0;
      uint32_t mx = 0;
      for (size_t i = 0; i < n_recs; ++i) {
        if (h_recs[i].block >= n_blocks) {
          QRec r = h_recs[i];
          r.block = static_cast<uint16_t>(r.block - n_blocks);
          mx = std::max<uint32_t>(mx, r.block);
          h_recs2[o][later++] = r;
        } else {
          h_recs[keep++] = h_recs[i];
        }
      }
      n_now = keep;
      n_recs = later;  // what the next launch starts with
      recs_max_block = mx;
    } else {
      n_recs = 0;
      recs_max_block = 0;
    }
    const unsigned set = out_parity;
    out_parity ^= 1u;
    if (n_now > d_keys_cap) {
      KNH_HIP(hipStreamSynchronize(ev_stream));
      if (d_keys) KNH_HIP(hipFree(d_keys));
      if (d_recs) KNH_HIP(hipFree(d_recs));
      d_keys = nullptr; d_recs = nullptr;
      d_keys_cap = std::max<size_t>(n_now * 2, 16384);
      KNH_HIP(hipMalloc(&d_keys, d_keys_cap * sizeof(knh_dev::u64)));
      KNH_HIP(hipMalloc(&d_recs, d_keys_cap * sizeof(knh_dev::DevRec)));
    }
    if (host_total + n_now > d_out_cap[set]) {
      if (lists_busy[set]) { KNH_HIP(hipEventSynchronize(lists_free[set])); lists_busy[set] = false; }
      KNH_HIP(hipStreamSynchronize(ev_stream));
      if (d_out_events[set]) KNH_HIP(hipFree(d_out_events[set]));
      d_out_events[set] = nullptr;
      d_out_cap[set] = std::max<size_t>((host_total + n_now) * 2, 16384);
      KNH_HIP(hipMalloc(&d_out_events[set], d_out_cap[set] * sizeof(Event)));
    }
    if (lists_busy[set]) { KNH_HIP(hipStreamWaitEvent(ev_stream, lists_free[set], 0)); lists_busy[set] = false; }
    const uint32_t nv = cfg.n_voices;
    knh_dev::EventResolveArgs ra{};
    ra.recs = reinterpret_cast<const knh_dev::DevRec*>(h_recs2[b]);
    ra.n_recs = static_cast<uint32_t>(n_now);
    ra.stages = d_stages;
    ra.n_voices = nv;
    ra.block_size = cfg.block_size;
    ra.frame_begin = fb;
    ra.frame_end = fe;
    ra.n_blocks = n_blocks;
    ra.sample_rate = cfg.sample_rate;
    ra.f64 = cfg.f64 ? 1u : 0u;
    ra.f2pi = cfg.f2pi;
    ra.armed = d_armed;
    ra.host_start = host_start;
    ra.host_events = host_events;
    ra.cnt = d_ev_cnt;
    ra.val_cnt = d_ev_cnt + nv;
    ra.cursor = d_ev_cnt + 2 * static_cast<size_t>(nv);
    ra.rec_start = d_rec_start;
    ra.keys = d_keys;
    ra.dev_recs = d_recs;
    ra.out_start = d_out_start[set];
    ra.out_events = d_out_events[set];
    ra.overflow = h_overflow;
    KNH_HIP(knh::launch_resolve_events(ra, ev_stream));
    KNH_HIP(hipEventRecord(recs_done[b], ev_stream));  // the records are read, and the lists complete: one event says both
    recs_busy[b] = true;
    last_resolve = static_cast<int>(b);
    KNH_HIP(hipStreamWaitEvent(s, recs_done[b], 0));  // the voice kernel reads this set
    out_in_use = static_cast<int>(set);
    // the host goes on filling the other buffer
    recs_parity = b ^ 1u;
    if (recs_busy[recs_parity]) { KNH_HIP(hipEventSynchronize(recs_done[recs_parity])); recs_busy[recs_parity] = false; }
    h_recs = h_recs2[recs_parity];
    out->ev_start = d_out_start[set];
    out->events = d_out_events[set];
    return KNH_OK;
  }
  // knh_bank_restart_voices.  The calls already recorded for the marked voices addressed nodes that no longer exist: dropped
  // (the buffer being filled is not one a kernel reads).
  void drop_voices(const std::vector<uint8_t>& marked) {
    size_t w = 0;
    uint32_t mx = 0;
    for (size_t i = 0; i < n_recs; ++i) {
      if (marked[h_recs[i].voice]) continue;
      mx = std::max<uint32_t>(mx, h_recs[i].block);
      h_recs[w++] = h_recs[i];
    }
    n_recs = w;
    recs_max_block = mx;
  }
  // The armed delays are the resolver's persistent device state; the restart kernel clears the restarted voices' on `s`, the
  // stream of the coming launch.  Ordered by events against the resolver's own stream, which runs beside the voice kernels:
  // the kernel starts after the resolver's last pass (restart_may_write), the next pass after the kernel (restart_written).
  unsigned short* armed() const { return d_armed; }
  int restart_may_write(hipStream_t s) {
    if (last_resolve >= 0) KNH_HIP(hipStreamWaitEvent(s, recs_done[last_resolve], 0));
    return KNH_OK;
  }
  int restart_written(hipEvent_t done) {
    KNH_HIP(hipStreamWaitEvent(ev_stream, done, 0));
    return KNH_OK;
  }
  // The voice kernel of the launch is enqueued on `s`: the resolver may rewrite the set of lists it reads once it has.
  int kernel_enqueued(hipStream_t s) {
    if (out_in_use < 0) return KNH_OK;
    KNH_HIP(hipEventRecord(lists_free[out_in_use], s));
    lists_busy[out_in_use] = true;
    out_in_use = -1;
    return KNH_OK;
  }

 private:
  int fail(int code, const std::string& msg) { return cfg.bank->fail(code, msg); }
  Setup cfg{};
  QRec* h_recs2[2] = {nullptr, nullptr};      // pinned; two alternate: the resolver of a launch reads one while the host fills the other
  size_t h_recs_cap[2] = {0, 0};
  hipEvent_t recs_done[2] = {nullptr, nullptr};
  bool recs_busy[2] = {false, false};
  unsigned recs_parity = 0;
  int last_resolve = -1;                      // the buffer whose recs_done marks the end of the resolver's last pass
  QRec* h_recs = nullptr;                    // = h_recs2[recs_parity]
  size_t n_recs = 0;
  uint32_t recs_max_block = 0;
  knh_dev::DevStage* d_stages = nullptr;
  uint16_t* d_armed = nullptr;
  uint32_t *d_ev_cnt = nullptr, *d_rec_start = nullptr;
  knh_dev::u64* d_keys = nullptr;
  knh_dev::DevRec* d_recs = nullptr;          // the launch's records, copied by the counting kernel (one pass over PCIe)
  size_t d_keys_cap = 0;
  // The resolver runs on a stream of its own, so that it works on launch k + 1 while the voice kernel of launch k runs; the
  // lists it makes therefore come in two sets, used alternately: a set is rewritten only after the voice kernel that read it
  // has finished (lists_free), and a voice kernel starts only when its set is complete (recs_done of that launch).
  hipStream_t ev_stream = nullptr;
  hipEvent_t lists_free[2] = {nullptr, nullptr};
  bool lists_busy[2] = {false, false};
  uint32_t* d_out_start[2] = {nullptr, nullptr};
  Event* d_out_events[2] = {nullptr, nullptr};
  size_t d_out_cap[2] = {0, 0};
  unsigned out_parity = 0;
  int out_in_use = -1;                        // the set the voice kernel being launched reads
  uint32_t* h_overflow = nullptr;             // mapped pinned: a resolver kernel found a change queue full
};

}  // namespace
