// voice_bank.hpp -- Bank<F>: one voice range on one GPU.  The host keeps a shadow of every *parameter-derived* quantity
// (never of audio-evolving state) and turns each UGen::param_apply into device state patches: all transcendental work (tan /
// pow / sqrt / exp for filter coefficients, the f64 phase-increment product) happens here with the same libm the reference's
// std-backed num-traits would call; WrPreciseTiming's queues, WrSmoothParams' ramps, the per-launch event lists and the
// launch itself.  Which kernel form the bank runs in is decided in one place, kernel_form.hpp: init asks it for the
// candidates, builds what the first that stands needs and keeps it as one value (`form`); nothing else looks further.  Two
// protocols with the device live behind types of their own, each owning its resources: the per-block call on a resident
// launch (resident_call.hpp) and the change queues the device resolves (event_resolver.hpp).
// Included by bank.hip only.
#pragma once

namespace {

// The streams knh_bank_process_blocks_begin gives its launches (bank.hip), whichever bank made them: a launch on one of them --
// a rank's or a shard's local bank sees only the stream -- keeps to it (Bank::process, overlap_now).
struct HostPipeStreams {
  std::mutex m;
  std::vector<hipStream_t> streams;
  void add(hipStream_t s) { std::lock_guard<std::mutex> l(m); streams.push_back(s); }
  void remove(hipStream_t s) { std::lock_guard<std::mutex> l(m); streams.erase(std::remove(streams.begin(), streams.end(), s), streams.end()); }
  bool has(hipStream_t s) { std::lock_guard<std::mutex> l(m); return std::find(streams.begin(), streams.end(), s) != streams.end(); }
};
inline HostPipeStreams& host_pipe_streams() {
  static HostPipeStreams h;
  return h;
}

template <typename F>
struct Bank final : knh_bank {
  typedef typename knh_dev::WordOf<F>::type W;
  // The kernel form the bank's launches take, chosen at init (kernel_form.hpp): its kind and variant, how it is launched --
  // a pre-built kernel's launch function, or the kernel hiprtc built at init -- and what the launch path asks of it.
  struct ChosenForm {
    knh::FormCandidate is;
    knh::FormFacts facts;
    knh::VoiceLaunchFn<F> fn = nullptr;   // the pre-built forms
    const knh::JitKernel* jit = nullptr;  // the fused forms, and the lane-per-frame kernel built at init (voice_frame.hpp, jit_frame_kernel)
  } form;
  // a voice of SinWt oscillators and arithmetic run a lane per frame: its program (the interpreter, kernels_interp.hip, reads it
  // on the device; the kernel built at init is written from it), the SinWt stages' slots, the built kernel's voices per workgroup
  std::vector<knh_dev::InterpOp> h_prog;
  knh_dev::InterpOp* d_prog = nullptr;
  unsigned interp_sigs = 0, interp_out = 0;
  uint32_t* d_sin_slots = nullptr;
  unsigned frame_vpw = 1, n_sin = 0;
  uint64_t env_ranks = 0;  // VoiceKernelArgs::env_ranks (graph-shaped voices with several envelope stages)
  std::string signature;
  const char* debug_signature() const override { return signature.c_str(); }
  void set_outputs(bool conn, uint32_t left, uint32_t right, const std::string& sig) override {
    knh_bank::set_outputs(conn, left, right, sig);
    signature = sig;  // (no pre-built kernel has two connected outputs: such a voice is fused at init)
  }
  uint32_t nv = 0;
  long stride = 0;

  // construction-time values
  std::vector<std::vector<double>> ctor;  // [stage][voice * n_ctor + a]
  // parameter shadows (only what a later setter needs to read back)
  struct Shadow {
    std::vector<F> a, b, c;        // SinWt: a=freq | Svf: a=cutoff b=q c=gain_db | Env: a=attack_s b=release_s
    std::vector<uint8_t> ty;       // Svf filter type
  };
  std::vector<Shadow> shadow;
  double f2pi = 0.0;
  // WrPreciseTiming state: next_delay per (param, voice) for wrapped stages; queues keyed by voice*n_stages+stage
  std::vector<uint16_t> next_delay;  // [n_params_total][nv], allocated only if some stage is wrapped
  // WrPreciseTiming::waiting_changes of every wrapped node, flattened: (key = voice * n_stages + stage, change)
  // in arrival order; grouped per node when the block is assembled.
  std::vector<std::pair<uint64_t, QueuedChange>> queued;
  // WrSmoothParams (smooth_params.rs:12-311) for stages flagged KNH_STAGE_FLAG_SMOOTH_PARAMS: the ramp state
  // lives on the host, exactly as it lives on the reference's audio thread; once per (partial) block every
  // ramp in flight hands its interpolated value to the wrapped node's setter.
  struct SmoothState {
    bool linear = false;
    double current_value = 0, start_value = 0, end_value = 0;
    size_t duration_frames = 0, frames_elapsed = 0;
    uint8_t audio_rate = 0;
    bool done = true;
    double interpolated() const {
      double mix = static_cast<double>(frames_elapsed) / static_cast<double>(duration_frames);
      return (end_value - start_value) * mix + start_value;
    }
  };
  std::vector<std::vector<SmoothState>> smooth;      // [stage][voice * n_params + param], flagged stages only
  std::vector<uint64_t> smooth_active;               // nodes (voice * n_stages + stage) with a ramp possibly in flight
  std::vector<std::vector<uint32_t>> smooth_mark;    // [stage][voice]: bit 0 = listed in smooth_active; rest = last ticked epoch
  uint32_t smooth_epoch = 0;
  // Device state patches of the next launch, in application order: block 0's immediate changes as they
  // arrive, then (at process time) block 0's queued changes, block 1's immediate ones, ...
  std::vector<HostEvent> pending;
  bool pending_needs_sort = false;   // some voice may have events out of frame order
  // The same change for a run of neighbouring voices (a whole bank's note-on or note-off in one knh_bank_param_apply_many):
  // one record instead of an event per voice.  `at` = how many events `pending` held when it arrived (its place in the
  // application order).  A resident call whose events are nothing but a few of these passes them on as they are (ResCall,
  // voice_chain.hpp: 32 bytes each over PCIe instead of 16 per voice), and so does an ordinary launch of a pipelined kernel
  // (in its kernel arguments: upload_events); anything else turns them into per-voice events first.
  struct RangeEvent { uint32_t v0, v1, frame, op, slot; uint64_t bits; size_t at; };
  std::vector<RangeEvent> pending_ranges, sent_ranges;
  uint32_t res_n_ranges = 0;         // the list upload_events has just made holds this many range events (0: per-voice lists)
  void expand_ranges() {
    if (pending_ranges.empty()) return;
    size_t extra = 0;
    for (const RangeEvent& r : pending_ranges) extra += r.v1 - r.v0;
    std::vector<HostEvent> out;
    out.reserve(pending.size() + extra);
    size_t k = 0;
    auto emit = [&](const RangeEvent& r) { for (uint32_t v = r.v0; v < r.v1; ++v) out.push_back(HostEvent{v, r.frame, r.op, r.slot, r.bits}); };
    for (size_t i = 0; i < pending.size(); ++i) {
      while (k < pending_ranges.size() && pending_ranges[k].at <= i) emit(pending_ranges[k++]);
      out.push_back(pending[i]);
    }
    while (k < pending_ranges.size()) emit(pending_ranges[k++]);
    pending.swap(out);
    pending_ranges.clear();
  }
  // The pipelined kernels (voice_pipe.hpp) walk range events, resident or launched (form.facts.walks_ranges): an ordinary
  // launch's range events travel in the kernel arguments.  KNH_RANGE_LAUNCHES=0, read when the bank is made: every launch
  // takes per-voice lists, as before (A/B runs, tests).
  bool range_launches = [] { const char* e = std::getenv("KNH_RANGE_LAUNCHES"); return !(e && e[0] == '0'); }();
  uint32_t launch_n_ranges = 0;      // the launch upload_events has just prepared takes this many range events (0: per-voice lists, or none)
  Event launch_range_recs[2 * knh_dev::LAUNCH_RANGES_MAX];
  // knh_bank_event_stats: launches that took range events, launches that took per-voice lists, bytes of lists handed to kernels
  uint64_t ev_range_launches = 0, ev_list_launches = 0, ev_list_bytes = 0;
  void event_stats(uint64_t* three) override { three[0] = ev_range_launches; three[1] = ev_list_launches; three[2] = ev_list_bytes; }
  uint32_t frame_base = 0;           // absolute frame of frame 0 of the block being assembled
  // param_apply / set_delay calls addressed to later blocks of the next multi-block launch
  struct Call { uint8_t is_delay; uint16_t delay; uint32_t voice, stage, param, kind; double f; int64_t i; };
  std::vector<std::vector<Call>> future;  // [block_offset]
  // Calls to a node wrapped in WrPreciseTiming (and in nothing that keeps host state of its own): one compact record
  // (QRec, event_resolver.hpp) per call, per block in arrival order.  When the block is assembled a single pass replays them
  // against the armed delays and each node's queue state (precise_timing.rs:65-135) and writes the device events; no queue
  // is ever materialised.
  std::vector<std::vector<QRec>> qfuture;  // [block_offset]
  struct NodeQ { uint32_t epoch; uint16_t at; uint16_t taken : 15, blocked : 1; };  // a node's queue during the block `epoch`
  std::vector<NodeQ> node_q;               // [voice * n_wrapped + wrapped index of the stage]
  std::vector<int> wrapped_index;          // [stage] -> index among the stages of this kind, or -1
  uint32_t n_wrapped = 0, q_epoch = 0;
  bool fastq(const StageInfo& S) const { return S.dcpb > 0 && !(S.flags & KNH_STAGE_FLAG_SMOOTH_PARAMS); }
  std::vector<QRec>& qblock(uint32_t block_offset) {
    if (qfuture.size() <= block_offset) qfuture.resize(block_offset + 1);
    return qfuture[block_offset];
  }
  // Which wrapped stages have their change queues resolved on the device (event_resolver.hpp): their records go to the
  // resolver, every other wrapped stage's to qfuture (the host path).
  std::vector<uint8_t> stage_dev;             // [stage]
  std::vector<uint8_t> dev_class;             // [stage * 8 + param]: 1 + the value kind a device-resolved node's parameter takes, 0: not one
  DevEventResolver resolver;
  static bool dev_resolvable_kind(uint16_t kind) {
    switch (kind) {
      case KNH_STAGE_SIN_WT: case KNH_STAGE_SIN_NUMERIC: case KNH_STAGE_MUL_ENV_ASR: case KNH_STAGE_MUL_ENV_AR:
      case KNH_STAGE_MUL_CONST: case KNH_STAGE_ADD_CONST: case KNH_STAGE_SUB_CONST: case KNH_STAGE_DIV_CONST: case KNH_STAGE_POW_CONST:
      case KNH_STAGE_WR_MUL: return true;
      default: return false;
    }
  }
  int push_rec(uint32_t block_offset, const QRec& r) {
    if (stage_dev[r.stage]) return resolver.push(block_offset, r);
    qblock(block_offset).push_back(r);
    return KNH_OK;
  }

  // device
  hipStream_t own_stream = nullptr;
  W* d_state = nullptr;
  float* d_sine = nullptr;
  double* d_seg_table = nullptr;  // segment Envelope: [voice][seg_max][3]
  uint32_t seg_max = 0;
  // BufferReader's pool of Buffers: one device allocation, entry k's samples from pool[k].off on (every start rounded up to
  // 64 samples); the host copies are staged in the entries until init.  A voice plays the entry buf_id[voice] says.
  // Every entry has the channel count of the first one (1, or 2: interleaved frames); `off` counts samples, n_frames frames.
  F* d_buffer = nullptr;
  struct PoolEntry { std::vector<F> samples; double sr = 0.0; uint32_t n_frames = 0, off = 0, channels = 1; };
  std::vector<PoolEntry> pool;
  uint32_t pool_channels() const { return pool.empty() ? 0u : pool[0].channels; }
  std::vector<uint32_t> buf_id;                      // [voice], empty: every voice on entry 0
  // BufferReader shadows, [reader][voice]: start_frame, dur_frame, rate.  A chain may hold several readers (a graph voice
  // that sums two): each has a start, a length and a rate of its own, so a seconds-valued setter or a restart of one reads
  // its own shadows and not the ones the reader constructed last left behind.
  std::vector<double> buf_start, buf_dur, buf_rate;
  size_t reader_at(const StageInfo& S, uint32_t v) const {  // S: a BufferReader stage of `stages`
    size_t k = 0;
    for (const StageInfo& T : stages) {
      if (&T == &S) break;
      k += T.reader();  // (a reader's second output, KNH_STAGE_FLAG_READER_CH1, is no reader: it has no shadows)
    }
    return k * nv + v;
  }
  const PoolEntry& buf_of(uint32_t v) const { return pool[buf_id.empty() ? 0u : buf_id[v]]; }
  // Seconds::from_secs_f64(secs).to_samples_f64(buffer_sr), time.rs:59-64,92-96
  static double secs_to_frames(double secs, double buffer_sr) {
    const double whole = std::floor(secs);
    const uint32_t tes = sat_u32((secs - std::trunc(secs)) * 282240000.0);
    return static_cast<double>(sat_u32(whole)) * buffer_sr + (static_cast<double>(tes) * buffer_sr) / 282240000.0;
  }
  // BufferReader::new(pool[buf_id[v]], rate, looping).start_at(start_s) and its init (buffer.rs:40-57, :106-115) for voice v,
  // a = the three constructor arguments: the voice's shadows, and every slot of the stage handed to put(rel, word).
  // linked: `rate` is driven at audio rate (knh_dev::BufferReaderP) -- the device multiplies base_rate by every sample of the
  // driver, so the entry's base_rate is a slot pair of its own, and follows the voice to another entry like the rest.
  template <typename Put>
  void reader_construct(const StageInfo& S, uint32_t v, const double* a, Put&& put) {
    const bool linked = S.ar_param != 0;
    const size_t r = reader_at(S, v);
    const PoolEntry& e = buf_of(v);
    const double base_rate = e.sr / static_cast<double>(sample_rate);  // Buffer::buf_rate_scale
    const double length_seconds = static_cast<double>(e.n_frames) / e.sr;
    const double start = secs_to_frames(a[2], e.sr), dur = secs_to_frames(length_seconds, e.sr);
    buf_start[r] = start; buf_dur[r] = dur; buf_rate[r] = a[0];
    auto put2 = [&](int rel, double d) {
      const uint64_t b = to_bits(d);
      put(rel, static_cast<uint32_t>(b));
      put(rel + 1, static_cast<uint32_t>(b >> 32));
    };
    put2(0, start);             // jump_to(start_frame)
    put2(2, base_rate * a[0]);  // base_rate * rate, the per-sample step
    put2(4, start);
    put2(6, start + dur);
    put(8, 0u);                 // finished = false
    put(9, a[1] != 0.0 ? 1u : 0u);
    put(10, e.off);
    put(11, e.n_frames);
    if (linked) put2(12, base_rate);
  }
  // the pool's size in samples with `n_samples` (frames x channels) in place of entry `at` (at == pool.size(): one more entry), every entry padded to 64
  uint64_t pool_samples_with(size_t at, uint64_t n_samples) const {
    uint64_t total = 0;
    for (size_t k = 0; k < pool.size(); ++k) total += ((k == at ? n_samples : static_cast<uint64_t>(pool[k].n_frames) * pool[k].channels) + 63ull) & ~63ull;
    if (at == pool.size()) total += (n_samples + 63ull) & ~63ull;
    return total;
  }
  // The delay stages' rings: one per (delay stage, voice), all in one allocation.  Stage after stage in chain order, each
  // stage's rings [voice][that stage's stride] of F, the stride the stage's own longest ring rounded up to the granule -- a
  // 40 ms delay beside a 1.7 ms allpass costs one 40 ms ring per voice, not two.  Behind the last stage's rings the spare
  // ring (RingLines' sink, voice_stages.hpp).  A device stage finds its ring by its first granule (its slot 3, Ctx::delay_stride
  // = kRingGranule): 32 samples, so every ring starts on a 128-byte line and is whole 16-byte pieces.
  static constexpr uint32_t kRingGranule = 32;
  struct DelayRings { uint32_t stage, stride; uint64_t base; };  // stride and base (of voice 0's ring) in samples, multiples of the granule
  void* d_delay = nullptr;
  uint32_t delay_stride = 0;        // kRingGranule once there are rings
  uint32_t ring_sink_row = 0;       // the spare ring's first granule
  // Feedback edges (KNH_STAGE_FLAG_FEEDBACK): a ring of one block per (edge, voice), entries of `rings` behind the delay stages'
  // (so knh_bank_restart_voices clears them with the rest), edge after edge in stage order and all of one stride -- a device
  // stage finds edge e's ring of voice v from these two numbers alone (knh_dev::FbRingT).
  uint32_t fb_row0 = 0, fb_granules = 0;
  std::vector<DelayRings> rings;    // per delay stage, in chain order
  std::vector<int> ring_of_stage;   // [stage] -> its entry of `rings`, -1: no delay stage
  std::vector<uint32_t> delay_len;  // [delay stage (entry of `rings`)][voice]: ring length (samples)
  uint32_t& ring_len(size_t stage, uint32_t v) { return delay_len[static_cast<size_t>(ring_of_stage[stage]) * nv + v]; }
  uint32_t ring_row(size_t stage, uint32_t v) const {
    const DelayRings& r = rings[static_cast<size_t>(ring_of_stage[stage])];
    return static_cast<uint32_t>((r.base + static_cast<uint64_t>(v) * r.stride) / kRingGranule);
  }
  std::vector<double> env_start;  // Envelope::start_value per voice (t_restart restores it)
  std::vector<uint32_t> env_nseg;
  F* d_partials = nullptr;
  F* d_out = nullptr;
  F* d_voices = nullptr;
  uint32_t* d_done = nullptr;
  uint32_t* d_flags = nullptr;
  uint32_t flags_turn = 0;          // which of the three flag sets the next launch uses
  uint32_t* flags_last = nullptr;   // the set of the last launch (knh_bank_debug_words)
  hipStream_t flags_stream = nullptr;  // the stream of the last launch, whose fold kernel cleared the set of this one
  bool flags_stream_set = false;
  // A launch's tree fold beside the next launch's voice kernel (process): the voice kernels of such launches run
  // on a stream of the bank's, their folds -- in the form that needs no LDS -- on another, and the caller's stream waits for
  // each fold.  Two sets of partial rows alternate; the second is made when the first such launch comes.
  // KNH_FOLD_OVERLAP=0, read when the bank is made: every launch keeps to the caller's stream (A/B runs, tests).
  // KNH_FOLD_WAVE=1: the single-stream tree folds of up to 256 rows take the LDS-free form too (tests of that form alone).
  bool fold_overlap = [] { const char* e = std::getenv("KNH_FOLD_OVERLAP"); return !(e && e[0] == '0'); }();
  bool fold_wave_always = [] { const char* e = std::getenv("KNH_FOLD_WAVE"); return e && e[0] == '1'; }();
  hipStream_t voice_stream = nullptr, fold_stream = nullptr;
  hipEvent_t caller_at = nullptr;                      // recorded on the caller's stream at the start of such a call
  hipEvent_t voice_done[2] = {nullptr, nullptr};       // [set of partial rows]: the voice kernel that wrote it is through
  hipEvent_t fold_done[2] = {nullptr, nullptr};        // [set of partial rows]: the fold that read it is through
  bool fold_busy[2] = {false, false};                  // fold_done[k] has been recorded
  F* d_partials2 = nullptr;
  uint32_t overlap_turn = 0;                           // the set of partial rows the next such launch writes
  bool last_overlapped = false;                        // the launch before ran on the bank's streams
  uint64_t overlapped_launches = 0, wave_folds = 0;  // knh_bank_debug_words 9 and 10
  int ensure_overlap_streams(unsigned n_waves) {
    // The two streams must not share a hardware queue with each other or with the caller's stream: a fold that sits in the
    // queue of the voice kernels runs between them, not beside them (measured: profiles/r15_fold_overlap.json).  A process has
    // few hardware queues and the runtime hands streams of one priority the same ones in turn, but it keeps the queues of each
    // priority apart: the voice stream takes the highest priority, the fold stream -- whose work is hidden and never
    // urgent -- the lowest, and the caller's stream is whatever the caller made it.
    if (!voice_stream || !fold_stream) {
      int least = 0, greatest = 0;
      KNH_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
      if (!voice_stream) KNH_HIP(hipStreamCreateWithPriority(&voice_stream, hipStreamNonBlocking, greatest));
      if (!fold_stream) KNH_HIP(hipStreamCreateWithPriority(&fold_stream, hipStreamNonBlocking, least));
    }
    if (!caller_at) KNH_HIP(hipEventCreateWithFlags(&caller_at, hipEventDisableTiming));
    for (int k = 0; k < 2; ++k) {
      if (!voice_done[k]) KNH_HIP(hipEventCreateWithFlags(&voice_done[k], hipEventDisableTiming));
      if (!fold_done[k]) KNH_HIP(hipEventCreateWithFlags(&fold_done[k], hipEventDisableTiming));
    }
    if (!d_partials2) KNH_HIP(hipMalloc(&d_partials2, static_cast<size_t>(partials_blocks) * fold_planes * n_waves * block_size * sizeof(F)));
    return KNH_OK;
  }
  // pinned host staging
  // Event lists are read by the kernel straight from pinned host memory (each is read once, a few hundred KB per
  // launch): no copy in the stream, the kernel's first waves pull them over PCIe while the others start.  Two
  // buffers alternate; one is rewritten only after the kernel that read it has finished (list_done).
  uint32_t* h_ev_start2[2] = {nullptr, nullptr};
  Event* h_events2[2] = {nullptr, nullptr};
  size_t h_events_cap2[2] = {0, 0};
  hipEvent_t list_done[2] = {nullptr, nullptr};
  bool list_busy[2] = {false, false};
  unsigned list_parity = 0;
  int list_in_use = -1;            // buffer the kernel being launched reads
  uint32_t* h_ev_start = nullptr;  // the buffer of the launch being assembled
  Event* h_events = nullptr;
  F* h_out = nullptr;  // [channels][block] then 2 x u32 flags
  // Blocking calls with a host destination (knh_bank_process_block: the call the reference makes once per block) hand the
  // mixed block over without a copy command: the fold kernel writes it into h_out -- mapped pinned host memory -- and then
  // an epoch number into h_done, which the host polls (knh_dev::HostDone).  Every other call takes the copies and the
  // stream wait.
  uint32_t* h_done = nullptr;        // pinned: [0] epoch, [1] flags[0], [2] flags[1]
  uint32_t* d_fold_count = nullptr;  // device: workgroups of the fold kernel that are through
  uint32_t done_epoch = 0;
  // the per-block call on a resident launch (resident_call.hpp); which kernel forms can be resident is decided here
  ResidentCall<F> resident;
  void resident_stats(uint64_t* calls, uint64_t* launches) override { resident.stats(calls, launches); }
  void resident_trace(uint64_t* five) override { resident.trace(five); }
  bool res_possible() const {
    // Kernel forms in which every workgroup can be resident at once and the fold server can take the rows (kernel_form.hpp
    // form_facts: the pipelined forms with a mixer wavefront and one voice group per workgroup, and the one-wavefront kernel,
    // pre-built or fused at run time); up to 256 voice groups (the server folds 8 x 32 rows), tree mix, no bank inputs (their
    // upload rides in a stream).
    return form.facts.can_be_resident && !uses_input && desc.mix_mode == KNH_MIX_TREE && (nv + 63u) / 64u <= 256u && block_size <= 4096;
  }
  void fill_launch_args(VoiceKernelArgs<F>& a, uint32_t n_blocks, uint32_t fb, uint32_t fe) {
    a.state = d_state;
    a.stride = stride;
    a.n_voices = nv;
    a.env_ranks = env_ranks;
    a.block_size = static_cast<uint32_t>(block_size);
    a.n_blocks = n_blocks;
    a.frame_begin = fb;
    a.frame_end = fe;
    a.sine_table = wt_lds ? reinterpret_cast<const float*>(d_wavetables) : d_sine;  // (wt_lds: an f32 bank whose wavetables are one table, at offset 0)
    a.f2pi = f2pi;
    a.sample_rate = sample_rate;
    a.seg_table = d_seg_table;
    a.seg_max = seg_max;
    a.delay_ring = d_delay;
    a.delay_stride = delay_stride;
    a.ring_sink_row = ring_sink_row;
    a.fb_row0 = fb_row0;
    a.fb_granules = fb_granules;
    a.buffer = d_buffer;
    a.wavetables = d_wavetables;
    a.input = nullptr;
    a.in_channels = desc.in_channels;
    a.ev_start = nullptr;
    a.events = nullptr;
    a.partials = d_partials;
    a.voices_out = nullptr;
    a.done_frames = d_done;
    a.flags = d_flags;
    a.res = knh_dev::Resident{};
    a.n_ranges = 0;
  }
  // timing
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> timing_pool;
  size_t timing_used = 0;
  double timing_ms = 0.0;
  uint64_t timing_launches = 0;

  // What may still read or write the bank's memory is idle before any of it is freed: the bank's own stream (a resident
  // kernel is asked to leave first), the resolver's, and the stream the last launch was given.  The members that own
  // resources of their own (resident, resolver) free them after this body, when those streams are idle too.
  ~Bank() override {
    if (device >= 0) (void)hipSetDevice(device);
    (void)resident.leave();
    if (own_stream) (void)hipStreamSynchronize(own_stream);
    resolver.quiesce();
    if (flags_stream_set && flags_stream != own_stream) (void)hipStreamSynchronize(flags_stream);
    // the bank's voice and fold streams go with it: a bank that is closed leaves no hardware queue taken
    for (hipStream_t st : {voice_stream, fold_stream})
      if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (caller_at) (void)hipEventDestroy(caller_at);
    for (int k = 0; k < 2; ++k) {
      if (voice_done[k]) (void)hipEventDestroy(voice_done[k]);
      if (fold_done[k]) (void)hipEventDestroy(fold_done[k]);
    }
    void* dev_ptrs[] = {d_state, d_sine, d_seg_table, d_delay, d_buffer, d_wavetables, d_partials, d_partials2, d_out, d_voices, d_done, d_flags, d_input, d_prog, d_sin_slots, d_fold_count};
    for (void* p : dev_ptrs)
      if (p) (void)hipFree(p);
    void* host_ptrs[] = {h_ev_start2[0], h_ev_start2[1], h_events2[0], h_events2[1], h_out, h_input, h_done, h_rs_voices, h_rs_words, h_rs_seg};
    for (void* p : host_ptrs)
      if (p) (void)hipHostFree(p);
    for (hipEvent_t e : list_done)
      if (e) (void)hipEventDestroy(e);
    if (in_copied) (void)hipEventDestroy(in_copied);
    if (rs_done) (void)hipEventDestroy(rs_done);
    for (auto& p : timing_pool) {
      (void)hipEventDestroy(p.first);
      (void)hipEventDestroy(p.second);
    }
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }

  int set_ctor(uint32_t stage, uint32_t first, uint32_t count, const double* args, uint32_t n_args) override {
    if (initialised) return fail(KNH_ERR_INVALID_ARGUMENT, "constructor arguments must be set before init");
    if (stage >= stages.size()) return fail(KNH_ERR_OUT_OF_RANGE, "stage out of range");
    if (static_cast<uint64_t>(first) + count > nv) return fail(KNH_ERR_OUT_OF_RANGE, "voice range out of range");
    if (stages[stage].kind == KNH_STAGE_MUL_ENVELOPE && stages[stage].n_ctor < 0) {
      // Envelope::new(start, segments): the first call fixes the bank-wide segment capacity
      if (n_args < 6 || (n_args - 4) % 2 != 0) return fail(KNH_ERR_INVALID_ARGUMENT, "Envelope takes 4 + 2 * n_max constructor arguments");
      stages[stage].n_ctor = static_cast<int>(n_args);
      ctor[stage].assign(static_cast<size_t>(nv) * n_args, 0.0);
    }
    if (static_cast<int>(n_args) != stages[stage].n_ctor) return fail(KNH_ERR_INVALID_ARGUMENT, "wrong number of constructor arguments");
    if (n_args && !args) return fail(KNH_ERR_INVALID_ARGUMENT, "null args");
    std::copy(args, args + static_cast<size_t>(count) * n_args, ctor[stage].begin() + static_cast<size_t>(first) * n_args);
    return KNH_OK;
  }

  // knh_bank_set_buffer (entry 0 of the pool, made or replaced) and knh_bank_add_buffer (one more entry)
  // (n_channels 2: Buffer::from_vec_interleaved, dsp/buffer.rs:70-78 -- n_frames * 2 samples, frame by frame)
  int put_buffer(size_t at, const char* who, uint32_t stage, const void* samples, size_t n_frames, uint32_t n_channels, double sr) {
    if (initialised) return fail(KNH_ERR_INVALID_ARGUMENT, std::string(who) + " comes before knh_bank_init");
    if (stage >= stages.size() || !stages[stage].reader()) return fail(KNH_ERR_INVALID_ARGUMENT, "not a BufferReader stage");
    if (n_channels < 1 || n_channels > 2) return fail(KNH_ERR_INVALID_ARGUMENT, "a Buffer has one or two channels");
    // the channel count is the pool's: the first entry fixes it (replacing the only entry may change it)
    if (!pool.empty() && !(at == 0 && pool.size() == 1) && n_channels != pool_channels())
      return fail(KNH_ERR_INVALID_ARGUMENT, pool_channels() == 2 ? "every Buffer of this pool has two channels (knh_bank_add_buffer_interleaved): the first entry fixes the pool's channel count"
                                                               : "every Buffer of this pool has one channel: the first entry fixes the pool's channel count");
    if (!samples || n_frames == 0 || n_frames >= (1ull << 31) || !(sr > 0.0) || !std::isfinite(sr)) return fail(KNH_ERR_INVALID_ARGUMENT, "empty buffer or bad sample rate");
    // a voice's offset into the pool is one 32-bit slot word
    const uint64_t n_samples = static_cast<uint64_t>(n_frames) * n_channels;
    if (pool_samples_with(at, n_samples) > 0xFFFFFFFFull) return fail(KNH_ERR_INVALID_ARGUMENT, "the pool of buffers would hold more than 2^32 - 1 samples");
    std::vector<F> copy(static_cast<const F*>(samples), static_cast<const F*>(samples) + n_samples);  // (first: nothing changes if it does not fit)
    if (at == pool.size()) pool.emplace_back();
    PoolEntry& e = pool[at];
    e.samples.swap(copy);
    e.sr = sr;
    e.n_frames = static_cast<uint32_t>(n_frames);
    e.channels = n_channels;
    return KNH_OK;
  }
  int set_buffer(uint32_t stage, const void* samples, size_t n_frames, double sr) override {
    if (pool_channels() == 2) return fail(KNH_ERR_INVALID_ARGUMENT, "knh_bank_set_buffer makes a single-channel entry: every Buffer of this pool has two channels");
    return put_buffer(0, "knh_bank_set_buffer", stage, samples, n_frames, 1, sr);
  }
  int add_buffer(uint32_t stage, const void* samples, size_t n_frames, uint32_t n_channels, double sr, uint32_t* out_index) override {
    const size_t at = pool.size();
    int rc = put_buffer(at, n_channels == 1 ? "knh_bank_add_buffer" : "knh_bank_add_buffer_interleaved", stage, samples, n_frames, n_channels, sr);
    if (rc == KNH_OK && out_index) *out_index = static_cast<uint32_t>(at);
    return rc;
  }
  void drop_last_buffer(uint32_t) override {
    if (!initialised && !pool.empty()) pool.pop_back();
  }
  uint32_t buffer_count(uint32_t stage) const override {
    return stage < stages.size() && stages[stage].reader() ? static_cast<uint32_t>(pool.size()) : 0u;
  }
  // knh_bank_assign_buffers.  Before init: the entry each voice is constructed on (and, with `args`, its constructor
  // arguments).  After init: the voice's reader becomes a new one on that entry -- every slot of the stage is patched at the
  // first frame of the next launch, the way a parameter change is, and the shadows the seconds-valued setters read follow.
  int assign_buffers(uint32_t stage, size_t count, const uint32_t* voices, const uint32_t* ids, const double* args) override {
    if (stage >= stages.size() || !stages[stage].reader()) return fail(KNH_ERR_INVALID_ARGUMENT, "not a BufferReader stage");
    if (count && (!voices || !ids)) return fail(KNH_ERR_INVALID_ARGUMENT, "null array");
    const StageInfo& S = stages[stage];
    if (initialised) {
      if (!args) return fail(KNH_ERR_INVALID_ARGUMENT, "after knh_bank_init knh_bank_assign_buffers needs the new reader's constructor arguments");
      if (S.flags & KNH_STAGE_FLAG_SMOOTH_PARAMS) return fail(KNH_ERR_UNSUPPORTED_CHAIN, "a BufferReader wrapped in WrSmoothParams keeps its buffer after knh_bank_init");
      for (const StageInfo& T : stages)  // (the voice's single done frame could not be told apart from the old reader's end)
        if (T.kind == KNH_STAGE_MUL_ENV_ASR || T.kind == KNH_STAGE_MUL_ENV_AR || T.kind == KNH_STAGE_MUL_ENVELOPE)
          return fail(KNH_ERR_UNSUPPORTED_CHAIN, "a chain in which an envelope can mark a voice done keeps its buffers after knh_bank_init");
    }
    for (size_t k = 0; k < count; ++k) {
      if (voices[k] >= nv) return fail(KNH_ERR_OUT_OF_RANGE, "voice out of range");
      if (ids[k] >= pool.size()) return fail(KNH_ERR_OUT_OF_RANGE, "buffer index out of range");
    }
    if (count == 0) return KNH_OK;
    if (buf_id.empty()) buf_id.assign(nv, 0u);
    if (!initialised) {
      for (size_t k = 0; k < count; ++k) {
        buf_id[voices[k]] = ids[k];
        if (args) std::copy(args + 3 * k, args + 3 * k + 3, ctor[stage].begin() + static_cast<size_t>(voices[k]) * 3);
      }
      return KNH_OK;
    }
    note_frame(frame_base);
    pending.reserve(pending.size() + count * static_cast<size_t>(S.n_slots));
    for (size_t k = 0; k < count; ++k) {
      const uint32_t v = voices[k];
      buf_id[v] = ids[k];
      // the new reader's constructor arguments are the voice's from here on, as knh_bank_assign_wavetables' are: a later
      // knh_bank_restart_voices constructs the reader the voice has, not the first one's rate on the new Buffer
      std::copy(args + 3 * k, args + 3 * k + 3, ctor[stage].begin() + static_cast<size_t>(v) * 3);
      reader_construct(S, v, args + 3 * k, [&](int rel, uint32_t word) {
        pending.push_back(HostEvent{v, frame_base, knh_dev::EV_SET, static_cast<uint32_t>(S.slot_base + rel), word});
      });
    }
    return KNH_OK;
  }

  // ---- OscWt's Wavetables (KNH_STAGE_FLAG_WAVETABLE) -----------------------------------------------------------
  // A pool per flagged stage; all of them in ONE device allocation, stage after stage, entry after entry, each entry 17
  // tables of 16384 samples in a row or one (Wavetable::from_buffer: one table that serves as all seventeen).  `off` counts
  // samples from the start of the allocation and is a multiple of 16384.  The host copies are staged in the entries until init.
  // The device reads at `table word + a 14-bit index` (knh_dev::OscWtT): every table word the host writes is
  // off + k * 16384 with k < n_tables of an entry of this list.
  F* d_wavetables = nullptr;
  bool wt_lds = false;  // the bank plays one f32 table and its kernel stages it to LDS in the sine table's place (init)
  struct WtEntry { std::vector<F> samples; uint32_t n_tables = 1, off = 0; };
  std::vector<std::vector<WtEntry>> wt_pool;   // [stage]
  std::vector<std::vector<uint32_t>> wt_id;    // [stage][voice], empty: every voice on entry 0
  const std::vector<WtEntry>& wt_entries(uint32_t stage) const {
    static const std::vector<WtEntry> none;
    return stage < wt_pool.size() ? wt_pool[stage] : none;
  }
  const WtEntry& wt_of(size_t stage, uint32_t v) const { return wt_pool[stage][stage < wt_id.size() && !wt_id[stage].empty() ? wt_id[stage][v] : 0u]; }
  uint64_t wt_samples() const {
    uint64_t total = 0;
    for (const auto& entries : wt_pool)
      for (const WtEntry& e : entries) total += static_cast<uint64_t>(e.n_tables) * kWavetableSize;
    return total;
  }
  // the two words of a voice's OscWt that say where it reads: the partial table Wavetable::get picks for `freq`
  // (wavetable.rs:606-609, freq.to_f32()), and the entry itself
  static uint32_t wt_table_word(const WtEntry& e, F freq) {
    return e.off + (e.n_tables == kWavetableTables ? wt_table_index(static_cast<float>(freq)) * kWavetableSize : 0u);
  }
  static uint32_t wt_entry_word(const WtEntry& e) { return e.off | (e.n_tables == kWavetableTables ? 1u : 0u); }
  int add_wavetable(uint32_t stage, const void* samples, uint32_t n_tables, uint32_t* out_index) override {
    if (initialised) return fail(KNH_ERR_INVALID_ARGUMENT, "knh_bank_add_wavetable comes before knh_bank_init");
    if (stage >= stages.size() || !stages[stage].wavetable()) return fail(KNH_ERR_INVALID_ARGUMENT, "not a KNH_STAGE_FLAG_WAVETABLE stage");
    if (!samples) return fail(KNH_ERR_INVALID_ARGUMENT, "null wavetable");
    if (n_tables != 1 && n_tables != kWavetableTables) return fail(KNH_ERR_INVALID_ARGUMENT, "a Wavetable is 17 partial tables of 16384 samples, or 1 that serves as all of them");
    const size_t n = static_cast<size_t>(n_tables) * kWavetableSize;
    // a voice's table is one 32-bit slot word
    if (wt_samples() + n > 0xFFFFFFFFull) return fail(KNH_ERR_INVALID_ARGUMENT, "the bank's wavetables would hold more than 2^32 - 1 samples");
    WtEntry e;
    e.samples.assign(static_cast<const F*>(samples), static_cast<const F*>(samples) + n);  // (first: nothing changes if it does not fit)
    e.n_tables = n_tables;
    if (wt_pool.size() < stages.size()) wt_pool.resize(stages.size());
    wt_pool[stage].push_back(std::move(e));
    if (out_index) *out_index = static_cast<uint32_t>(wt_pool[stage].size() - 1);
    return KNH_OK;
  }
  void drop_last_wavetable(uint32_t stage) override {
    if (!initialised && stage < wt_pool.size() && !wt_pool[stage].empty()) wt_pool[stage].pop_back();
  }
  uint32_t wavetable_count(uint32_t stage) const override {
    return stage < stages.size() && stages[stage].wavetable() ? static_cast<uint32_t>(wt_entries(stage).size()) : 0u;
  }
  // knh_bank_assign_wavetables.  Before init: the entry each voice's OscWt is constructed on (and, with `args`, its freq).
  // After init: the voice's node becomes a new OscWt on that entry -- every slot of the stage is patched at the first frame
  // of the next launch, the way a parameter change is; the shadow, the constructor argument and the wrapper's smoothing follow.
  int assign_wavetables(uint32_t stage, size_t count, const uint32_t* voices, const uint32_t* ids, const double* args) override {
    if (stage >= stages.size() || !stages[stage].wavetable()) return fail(KNH_ERR_INVALID_ARGUMENT, "not a KNH_STAGE_FLAG_WAVETABLE stage");
    if (count && (!voices || !ids)) return fail(KNH_ERR_INVALID_ARGUMENT, "null array");
    if (initialised && !args) return fail(KNH_ERR_INVALID_ARGUMENT, "after knh_bank_init knh_bank_assign_wavetables needs the new oscillator's constructor argument");
    const StageInfo& S = stages[stage];
    const size_t n_entries = wt_entries(stage).size();
    for (size_t k = 0; k < count; ++k) {
      if (voices[k] >= nv) return fail(KNH_ERR_OUT_OF_RANGE, "voice out of range");
      if (ids[k] >= n_entries) return fail(KNH_ERR_OUT_OF_RANGE, "wavetable index out of range");
    }
    if (count == 0) return KNH_OK;
    if (wt_id.size() < stages.size()) wt_id.resize(stages.size());
    if (wt_id[stage].empty()) wt_id[stage].assign(nv, 0u);
    if (initialised) {
      note_frame(frame_base);
      pending.reserve(pending.size() + count * static_cast<size_t>(S.n_slots));
      if (S.dcpb > 0) {  // changes still waiting in the old node's WrPreciseTiming queue went with it (as at a restart: forget_voices)
        std::vector<uint8_t> named(nv, 0);
        for (size_t k = 0; k < count; ++k) named[voices[k]] = 1;
        const uint64_t ns = stages.size();
        for (auto& recs : qfuture)
          recs.erase(std::remove_if(recs.begin(), recs.end(), [&](const QRec& r) { return r.stage == stage && named[r.voice] && r.has_value(); }), recs.end());
        queued.erase(std::remove_if(queued.begin(), queued.end(), [&](const std::pair<uint64_t, QueuedChange>& q) { return q.first % ns == stage && named[q.first / ns]; }), queued.end());
      }
    }
    for (size_t k = 0; k < count; ++k) {
      const uint32_t v = voices[k];
      wt_id[stage][v] = ids[k];
      if (args) ctor[stage][v] = args[k];
      if (!initialised) continue;
      if (!smooth[stage].empty()) std::fill_n(smooth[stage].begin() + static_cast<size_t>(v) * S.n_params, S.n_params, SmoothState{});
      if (S.dcpb > 0 && !next_delay.empty())
        for (int p = 0; p < S.n_params; ++p) next_delay[static_cast<size_t>(S.param_base + p) * nv + v] = 0;
      (void)construct_stage(stage, v, args + k, [&](int rel, W word) {
        pending.push_back(HostEvent{v, frame_base, knh_dev::EV_SET, static_cast<uint32_t>(S.slot_base + rel), static_cast<uint64_t>(word)});
      });
    }
    return KNH_OK;
  }

  // the bank node's input channels for the next launch
  F* d_input = nullptr;           // [in_blocks_cap][in_channels][block_size]
  F* h_input = nullptr;           // pinned staging of the same
  uint32_t in_blocks_cap = 0, in_blocks_set = 0;
  const void* in_device = nullptr;  // set_input_device: read where it is
  bool in_host_pending = false;
  hipEvent_t in_copied = nullptr;   // recorded behind the upload of h_input, on the stream of that launch
  bool in_copy_pending = false;
  bool uses_input = false;
  int set_input(uint32_t n_blocks, const void* host, const void* dev) override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    if (desc.in_channels == 0) return fail(KNH_ERR_INVALID_ARGUMENT, "the bank has no input channels (knh_bank_desc.in_channels)");
    if (n_blocks == 0 || n_blocks > 4096 || (!host && !dev)) return fail(KNH_ERR_INVALID_ARGUMENT, "knh_bank_set_input: n_blocks in 1..4096 and a buffer");
    KNH_HIP(hipSetDevice(device));
    in_blocks_set = n_blocks;
    in_device = dev;
    in_host_pending = false;
    if (dev) return KNH_OK;
    const size_t elems = static_cast<size_t>(n_blocks) * desc.in_channels * block_size;
    if (n_blocks > in_blocks_cap) {
      KNH_HIP(hipDeviceSynchronize());
      if (d_input) KNH_HIP(hipFree(d_input));
      if (h_input) KNH_HIP(hipHostFree(h_input));
      d_input = nullptr; h_input = nullptr;
      KNH_HIP(hipMalloc(&d_input, elems * sizeof(F)));
      KNH_HIP(hipHostMalloc(&h_input, elems * sizeof(F)));
      in_blocks_cap = n_blocks;
    } else if (in_copy_pending) {
      // the upload of the launch before may still be reading the staging buffer -- on whatever stream that launch was
      // given (the caller's, the pipelined host output's, a rank bank's), hence an event and not a stream to wait for
      KNH_HIP(hipEventSynchronize(in_copied));
      in_copy_pending = false;
    }
    std::memcpy(h_input, host, elems * sizeof(F));
    in_host_pending = true;
    return KNH_OK;
  }

  // ---- construction: UGen::new + UGen::init of one node ------------------------------------
  // knh_bank_init runs prepare_stage and then construct_stage for every voice; knh_bank_restart_voices runs construct_stage
  // again for the voices it names.  This is the one statement of how each stage kind is constructed.
  bool svf_ic2_neg0 = false;     // KNH_DEBUG_SVF_IC2_NEG0=1 (tests only), read at init
  std::vector<double> seg_rows;  // segment Envelope: the host's copy of d_seg_table, [voice][seg_max][3]
  static W fw(F x) { return static_cast<W>(to_bits(x)); }
  // The ring a delay stage constructed with `a` allocates, in samples (delay.rs:24-31, :107-123).
  int delay_ring_len(const StageInfo& S, const double* a, uint32_t* out) {
    const uint32_t sr = sample_rate;
    if (S.kind == KNH_STAGE_SAMPLE_DELAY) {
      // Seconds::from_secs_f64 / to_secs_f64 (knaster_primitives/src/time.rs:59-74), then `as usize`
      const double secs_in = a[0];
      if (!(secs_in >= 0.0) || secs_in >= 4294967296.0) return fail(KNH_ERR_INVALID_ARGUMENT, "SampleDelay: max delay out of range");
      const uint32_t whole = static_cast<uint32_t>(std::floor(secs_in));
      const uint32_t tes = sat_u32((secs_in - std::floor(secs_in)) * 282240000.0);
      const double secs = static_cast<double>(whole) + static_cast<double>(tes) / 282240000.0;
      const double nf = secs * static_cast<double>(sr);
      if (!(nf >= 1.0)) return fail(KNH_ERR_INVALID_ARGUMENT, "SampleDelay: the ring would be empty (the reference divides by zero)");
      if (nf >= 1073741824.0) return fail(KNH_ERR_INVALID_ARGUMENT, "SampleDelay: max delay too long");
      *out = static_cast<uint32_t>(nf);
      return KNH_OK;
    }
    const double secs_in = a[0];
    if (!(secs_in >= 0.0) || secs_in >= 4294967296.0) return fail(KNH_ERR_INVALID_ARGUMENT, "AllpassDelay: max delay out of range");
    const uint64_t whole = static_cast<uint64_t>(std::floor(secs_in));
    const uint64_t tes = sat_u32((secs_in - std::floor(secs_in)) * 282240000.0);
    const uint64_t nsamp = whole * sr + tes * static_cast<uint64_t>(sr) / 282240000ull;  // Seconds::to_samples, time.rs:86-90
    if (nsamp == 0) return fail(KNH_ERR_INVALID_ARGUMENT, "AllpassDelay: the ring would be empty (the reference takes a remainder by zero)");
    if (nsamp >= (1ull << 30)) return fail(KNH_ERR_INVALID_ARGUMENT, "AllpassDelay: max delay too long");
    *out = static_cast<uint32_t>(nsamp);
    return KNH_OK;
  }
  // What does not depend on the voice: the stage's shadows and tables are sized, the chain-wide refusals made.
  int prepare_stage(size_t si) {
    const StageInfo& S = stages[si];
    Shadow& sh = shadow[si];
    switch (S.kind) {
      case KNH_STAGE_SIN_WT:
        sh.a.resize(nv);
        if (S.wavetable() && wt_entries(static_cast<uint32_t>(si)).empty()) return fail(KNH_ERR_INVALID_ARGUMENT, "KNH_STAGE_FLAG_WAVETABLE stage without knh_bank_add_wavetable");
        break;
      case KNH_STAGE_SVF: sh.a.resize(nv); sh.b.resize(nv); sh.c.resize(nv); sh.ty.resize(nv); break;
      case KNH_STAGE_MUL_ENV_ASR: case KNH_STAGE_MUL_ENV_AR: sh.a.resize(nv); sh.b.resize(nv); break;
      case KNH_STAGE_MUL_ENVELOPE: {
        if (S.n_ctor < 0) return fail(KNH_ERR_INVALID_ARGUMENT, "Envelope stage without constructor arguments");
        const uint32_t n_max = static_cast<uint32_t>((S.n_ctor - 4) / 2);
        env_start.assign(nv, 0.0); env_nseg.assign(nv, 0); seg_max = n_max; seg_rows.assign(static_cast<size_t>(nv) * n_max * 3, 0.0);
      } break;
      case KNH_STAGE_BUFFER_READER: {
        if (S.ch1()) break;  // the second output of a reader: nothing of its own
        if (pool.empty()) return fail(KNH_ERR_INVALID_ARGUMENT, "BufferReader stage without knh_bank_set_buffer or knh_bank_add_buffer");
        if (S.dcpb > 0) return fail(KNH_ERR_INVALID_ARGUMENT, "BufferReader cannot be wrapped in WrPreciseTiming here");
        if (reader_at(S, 0) == 0) {  // the chain's first reader: the shadows of all of them, the pool's layout
          size_t readers = 0;
          for (const StageInfo& T : stages) readers += T.reader();
          buf_start.assign(readers * nv, 0.0); buf_dur.assign(readers * nv, 0.0); buf_rate.assign(readers * nv, 0.0);
          uint64_t off = 0;  // in samples (put_buffer has kept the sum within 32 bits)
          for (PoolEntry& e : pool) { e.off = static_cast<uint32_t>(off); off += (static_cast<uint64_t>(e.n_frames) * e.channels + 63ull) & ~63ull; }
        }
      } break;
      case KNH_STAGE_INPUT: uses_input = uses_input || !S.feedback(); break;  // (a feedback edge's ring comes behind the delay stages': init)
      case KNH_STAGE_ALLPASS_FB_DELAY: case KNH_STAGE_ALLPASS_DELAY: case KNH_STAGE_SAMPLE_DELAY: {
        // the stage's rings: behind the delay stages before it, as far apart as its own longest ring asks
        uint32_t mx = 0;
        for (uint32_t v = 0; v < nv; ++v) {
          uint32_t len = 0;
          int rc = delay_ring_len(S, ctor[si].data() + static_cast<size_t>(v) * S.n_ctor, &len);
          if (rc != KNH_OK) return rc;
          mx = std::max(mx, len);
        }
        const uint64_t base = rings.empty() ? 0u : rings.back().base + static_cast<uint64_t>(nv) * rings.back().stride;
        const uint32_t own = (mx + kRingGranule - 1u) / kRingGranule * kRingGranule;
        // (a ring is named by its first granule in a 32-bit state word; the spare ring's comes behind the last one)
        if ((base + static_cast<uint64_t>(nv) * own) / kRingGranule >= 0xFFFFFFFFull) return fail(KNH_ERR_INVALID_ARGUMENT, "the delay rings of the bank are too long in sum");
        ring_of_stage[si] = static_cast<int>(rings.size());
        rings.push_back(DelayRings{static_cast<uint32_t>(si), own, base});
        delay_len.resize(rings.size() * nv, 0u);
      } break;
      default: break;
    }
    return KNH_OK;
  }
  // Node `si` of voice v from its constructor arguments `a`: every slot of the stage through put(rel, word) (a slot not put is
  // zero), the shadows the setters read, the voice's segment rows.
  template <typename Put>
  int construct_stage(size_t si, uint32_t v, const double* a, Put&& put) {
    const StageInfo& S = stages[si];
    Shadow& sh = shadow[si];
    const uint32_t sr = sample_rate;
    const F sr_as_f32 = static_cast<F>(static_cast<float>(sr));  // F::new(sample_rate as f32)
    switch (S.kind) {
      case KNH_STAGE_SIN_WT: {  // osc.rs:110-123,142-147
        F freq = static_cast<F>(a[0]);
        sh.a[v] = freq;
        put(0, 0);
        put(1, 0);
        put(2, sat_u32(static_cast<double>(freq) * f2pi));
        if (S.wavetable()) {  // OscWt: init (osc.rs:82-86), then freq(a[0]) (:44-47) -- knaster_hip.h, the decision at the flag
          const WtEntry& e = wt_of(si, v);
          put(3, wt_table_word(e, freq));
          put(4, wt_entry_word(e));
        }
      } break;
      case KNH_STAGE_SIN_NUMERIC: {  // osc.rs:231-236,253-261
        F freq = static_cast<F>(a[0]);
        put(0, fw(F(0)));
        put(1, fw(F(0)));
        put(2, fw(freq / sr_as_f32));
      } break;
      case KNH_STAGE_SVF: {  // svf.rs:64-79,134-141
        double tyd = a[0];
        uint32_t ty = (tyd >= 0 && tyd <= 8) ? static_cast<uint32_t>(tyd) : 0u;
        sh.ty[v] = static_cast<uint8_t>(ty);
        sh.a[v] = static_cast<F>(a[1]); sh.b[v] = static_cast<F>(a[2]); sh.c[v] = static_cast<F>(a[3]);
        F co[6];
        svf_coeffs<F>(ty, sh.a[v], sh.b[v], sh.c[v], sr_as_f32, co);
        put(0, fw(F(0)));
        put(1, fw(svf_ic2_neg0 && v % 3 == 0 ? F(-0.0) : F(0)));
        for (int k = 0; k < 6; ++k) put(2 + k, fw(co[k]));
        if (S.n_slots == 12) {  // a parameter driven at audio rate: the setter runs on the device and needs the other values
          put(8, fw(sh.a[v])); put(9, fw(sh.b[v])); put(10, fw(sh.c[v]));
          put(11, ty);
        }
      } break;
      case KNH_STAGE_ONEPOLE_LPF:    // onepole.rs:118-129
      case KNH_STAGE_ONEPOLE_HPF: {  // onepole.rs:157-167 (b1 = 0 -> exp(0) = 1)
        F freq = S.kind == KNH_STAGE_ONEPOLE_LPF ? static_cast<F>(a[0]) : F(0);
        F f = freq / sr_as_f32;
        F b1 = std::exp(F(-2.0) * Consts<F>::PI * f);
        F a0 = F(1.0) - b1;
        put(0, fw(F(0)));
        put(1, fw(a0));
        put(2, fw(b1));
      } break;
      case KNH_STAGE_MUL_ENV_ASR:
      case KNH_STAGE_MUL_ENV_AR: {  // envelopes.rs:33-43,135-151 / :187-197,268-284
        F atk = static_cast<F>(a[0]), rel = static_cast<F>(a[1]);
        sh.a[v] = atk; sh.b[v] = rel;
        F ar = atk == F(0) ? F(1) : F(1) / (atk * static_cast<F>(sr));
        F rr = rel == F(0) ? F(1) : F(1) / (rel * static_cast<F>(sr));
        put(0, 0);          // Stopped
        put(1, fw(F(0)));   // t
        put(2, fw(ar));
        put(3, fw(rr));
        put(4, fw(F(1)));   // release_scale
      } break;
      case KNH_STAGE_MUL_ENVELOPE: {  // envelopes.rs:373-400 (+ builder methods), init :404-406
        const uint32_t n_max = static_cast<uint32_t>((S.n_ctor - 4) / 2);
        uint32_t n_seg = a[3] >= 1 ? static_cast<uint32_t>(a[3]) : 1u;
        if (n_seg > n_max) n_seg = n_max;
        env_start[v] = a[0];
        env_nseg[v] = n_seg;
        const double dt = a[1] * (1.0 / static_cast<double>(sr));  // time_scale * base_scale
        auto put2 = [&](int rel, double d) {
          uint64_t b = to_bits(d);
          put(rel, static_cast<W>(static_cast<uint32_t>(b)));
          put(rel + 1, static_cast<W>(static_cast<uint32_t>(b >> 32)));
        };
        put(0, 0);  // Stopped
        put(1, 0);
        put2(2, 0.0);
        put2(4, a[0]);  // from_value = start_value
        put2(6, dt);
        put(8, n_seg);
        put(9, a[2] != 0.0 ? 1u : 0u);
        put(10, v);
        for (uint32_t k = 0; k < n_max; ++k) {
          const double dur = a[4 + 2 * k], val = a[5 + 2 * k];
          double* row = &seg_rows[(static_cast<size_t>(v) * n_max + k) * 3];
          row[0] = dur; row[1] = 1.0 / dur; row[2] = val;  // EnvelopeSegment::new, envelopes.rs:327-333
        }
      } break;
      case KNH_STAGE_BUFFER_READER: {  // buffer.rs:40-57 (new, start_at), :106-115 (init)
        if (S.ch1()) break;  // (no slots: the reader stage holds the node)
        reader_construct(S, v, a, [&](int rel, uint32_t word) { put(rel, static_cast<W>(word)); });
      } break;
      case KNH_STAGE_PHASOR: {  // osc.rs:181-188 (new), :197-200 (init: step = freq * (1 / sample_rate))
        const double step = a[0] * (1.0 / static_cast<double>(sr));
        const uint64_t sb = to_bits(step);
        put(0, 0);
        put(1, 0);
        put(2, static_cast<W>(static_cast<uint32_t>(sb)));
        put(3, static_cast<W>(static_cast<uint32_t>(sb >> 32)));
      } break;
      case KNH_STAGE_SAFETY_LIMITER: break;
      case KNH_STAGE_INPUT: {
        if (S.feedback()) break;  // a feedback edge: no channel, no state (its ring is found by edge and voice)
        if (!(a[0] >= 0.0) || a[0] >= static_cast<double>(desc.in_channels)) return fail(KNH_ERR_INVALID_ARGUMENT, "KNH_STAGE_INPUT: channel is not below knh_bank_desc.in_channels");
        put(0, static_cast<W>(static_cast<uint32_t>(a[0])));
      } break;
      case KNH_STAGE_MATH_ADD: case KNH_STAGE_MATH_SUB: case KNH_STAGE_MATH_MUL: case KNH_STAGE_MATH_DIV: case KNH_STAGE_MATH_POW: break;  // no state
      case KNH_STAGE_MATH1_CEIL: case KNH_STAGE_MATH1_SQRT: case KNH_STAGE_MATH1_FLOOR: case KNH_STAGE_MATH1_TRUNC: case KNH_STAGE_MATH1_FRACT:
      case KNH_STAGE_MATH1_EXP: break;  // Math1UGen (math.rs:167-305): no constructor arguments, no state
      case KNH_STAGE_WHITE_NOISE: case KNH_STAGE_PINK_NOISE: case KNH_STAGE_BROWN_NOISE: {
        // fastrand::Rng::with_seed(next_randomness_seed()) (noise.rs:34,66,134): the state is the seed
        const uint64_t seed = a[0] >= 0.0 ? static_cast<uint64_t>(a[0]) : 0u;
        put(0, static_cast<W>(static_cast<uint32_t>(seed)));
        put(1, static_cast<W>(static_cast<uint32_t>(seed >> 32)));
        if (S.kind == KNH_STAGE_BROWN_NOISE) put(2, to_bits(F(0)));
        if (S.kind == KNH_STAGE_PINK_NOISE) {  // noise.rs:64-75: counter 1, everything else zero
          put(2, 1u);
          for (int k = 3; k < 14; ++k) put(k, to_bits(F(0)));
        }
      } break;
      case KNH_STAGE_RANDOM_LIN: {  // noise.rs:172-200: new() draws the first value, init() turns freq into a step and draws the second
        uint64_t rng = (a[0] >= 0.0 ? static_cast<uint64_t>(a[0]) : 0u) * 94u + 53u;
        auto draw = [&rng]() {  // fastrand 2.3.0 Rng::f32 (wyrand), restated: voice_stages.hpp NoiseRng
          rng += 0x2d358dccaa6c78a5ull;
          const unsigned __int128 t = static_cast<unsigned __int128>(rng) * static_cast<unsigned __int128>(rng ^ 0x8bb84b93962eacc9ull);
          const uint32_t r = static_cast<uint32_t>(static_cast<uint64_t>(t) ^ static_cast<uint64_t>(t >> 64));
          const uint32_t bits = 0x3F800000u + (r >> 9);
          float f;
          std::memcpy(&f, &bits, 4);
          return f - 1.0f;
        };
        const F first = static_cast<F>(draw());              // current_value: F::new(rng.f32())
        const F inc = F(1) / static_cast<F>(sr);             // freq_to_phase_inc = F::ONE / F::from(sample_rate)
        const F step = static_cast<F>(a[1]) * inc;           // phase_step *= freq_to_phase_inc
        const F old_target = first + F(0);                   // new_value(): current_value + current_change_width
        const F second = static_cast<F>(draw());
        put(0, static_cast<W>(static_cast<uint32_t>(rng)));
        put(1, static_cast<W>(static_cast<uint32_t>(rng >> 32)));
        put(2, to_bits(old_target));
        put(3, to_bits(static_cast<F>(second - old_target)));
        put(4, to_bits(F(0)));
        put(5, to_bits(step));
      } break;
      case KNH_STAGE_POLYBLEP: {  // polyblep.rs:136-153: new(waveform, freq), init -> set_freq: dt = freq / sample_rate
        const F srf = static_cast<F>(sr);  // F::from(sample_rate)
        const F freq = static_cast<F>(a[1]);
        const F dt = freq != F(0) ? freq / srf : F(0);
        const uint64_t wf = a[0] >= 0.0 && a[0] < 14.0 ? static_cast<uint64_t>(a[0]) : 0u;
        put(0, fw(F(0)));
        put(1, fw(dt));
        put(2, fw(F(0.5)));
        put(3, static_cast<W>(wf));
        put(4, (dt * srf >= srf / F(4)) ? 1u : 0u);  // get_freq_in_hz() >= sample_rate / 4, :210
      } break;
      case KNH_STAGE_ALLPASS_FB_DELAY:  // delay.rs:221-229: an AllpassDelay and feedback = 0
      case KNH_STAGE_ALLPASS_DELAY: {  // delay.rs:107-123: buffer = max_delay_seconds.to_samples(sample_rate) zeros
        uint32_t nsamp = 0;
        { int rc = delay_ring_len(S, a, &nsamp); if (rc != KNH_OK) return rc; }
        ring_len(si, v) = nsamp;
        put(0, 0);  // write_frame
        put(1, 0);  // read_frame
        put(2, static_cast<W>(nsamp));
        put(3, ring_row(si, v));
        put(4, fw(F(1)));  // AllpassInterpolator::new: coeff, prev_input, prev_output all ONE (:61-67)
        put(5, fw(F(1)));
        put(6, fw(F(1)));
        if (S.kind == KNH_STAGE_ALLPASS_FB_DELAY) put(7, fw(F(0)));
      } break;
      case KNH_STAGE_SAMPLE_DELAY: {  // delay.rs:24-31 (new), :45-49 (init)
        uint32_t len = 0;
        { int rc = delay_ring_len(S, a, &len); if (rc != KNH_OK) return rc; }
        ring_len(si, v) = len;
        put(0, 0);    // write_position
        put(1, len);  // len - delay_samples, delay_samples = 0
        put(2, len);
        put(3, ring_row(si, v));
      } break;
      case KNH_STAGE_WR_POWI:  // WrPowi::new(ugen, value: i32), wrappers_core/math.rs:591-595
        put(0, static_cast<W>(static_cast<uint32_t>(static_cast<int32_t>(a[0]))));
        break;
      case KNH_STAGE_PAN2: {  // Pan2::new(pan: f32), pan.rs:18-23; the gains of process(), :33-35, as F::new(..)
        float gl, gr;
        pan2_gains(static_cast<float>(a[0]), &gl, &gr);
        put(0, fw(static_cast<F>(gl)));
        put(1, fw(static_cast<F>(gr)));
      } break;
      default:  // Constant / wrapper value: util.rs:43-45, wrappers_core/math.rs:21-23
        put(0, fw(static_cast<F>(a[0])));
        break;
    }
    return KNH_OK;
  }

  // ---- UGen::init for every node of every voice --------------------------------------
  int init(uint32_t sr, size_t bs) override {
    if (initialised) return fail(KNH_ERR_INVALID_ARGUMENT, "already initialised");
    if (sr == 0 || bs == 0 || bs > 65535) return fail(KNH_ERR_INVALID_ARGUMENT, "sample_rate/block_size out of range (block_size <= 65535)");
    int ndev = knh_device_count();
    if (ndev <= 0) return fail(KNH_ERR_NO_DEVICE, "no gfx950 device visible; this engine has no CPU path");
    if (desc.device >= 0) device = desc.device;
    else KNH_HIP(hipGetDevice(&device));
    KNH_HIP(hipSetDevice(device));
    // The pool's channel count is known now.  A reader's second output needs a second channel (in the reference it reads the
    // neighbouring sample and runs off the end); a mono reader on a pool of two-channel Buffers plays channel 0 of the
    // interleaved frames (BufferReader<F, U1> on a stereo Buffer: index * num_channels + 0) -- a stage of its own, 'C' for 'F'
    // in the plan's signature below.
    for (const StageInfo& S : stages)
      if (S.ch1() && pool_channels() == 1) return fail(KNH_ERR_INVALID_ARGUMENT, "a KNH_STAGE_FLAG_READER_CH1 stage needs a pool of two-channel Buffers (knh_bank_add_buffer_interleaved with n_channels = 2)");
    // The kernel form (kernel_form.hpp): what the decision reads, the candidates in its order, the first that stands.  The
    // plan's signature becomes the bank's when init gets to its end: a refused init changes nothing.
    const bool f64 = sizeof(F) == 8, fma = desc.allow_fma != 0;
    knh::FormInputs in;
    in.signature = signature;
    // Where OscWt's samples come from, decided here beside the staging of the sine table.  Staged to LDS: the voice has one
    // flagged stage, its pool is a single one-table entry, the table is the 64 KiB of f32 the forms keep a place for (an f64
    // table is 128 KiB: gathered) and no SinWt of the voice needs that place -- the whole bank then reads one table exactly as
    // SinWt reads the sine table ('g' for 'M', 'h' for 'k').  Anything else, and KNH_WT_LDS=0 (A/B runs, tests): gathered from
    // the allocation in device memory, which is always correct.
    wt_lds = false;
    {
      size_t flagged = 0, at = 0;
      for (size_t si = 0; si < stages.size(); ++si)
        if (stages[si].wavetable()) { ++flagged; at = si; }
      const char* const e = std::getenv("KNH_WT_LDS");
      if (flagged == 1 && !f64 && !(e && e[0] == '0') && wt_entries(static_cast<uint32_t>(at)).size() == 1 && wt_entries(static_cast<uint32_t>(at))[0].n_tables == 1 &&
          in.signature.find_first_of("WR") == std::string::npos) {
        wt_lds = true;
        std::replace(in.signature.begin(), in.signature.end(), 'M', 'g');
        std::replace(in.signature.begin(), in.signature.end(), 'k', 'h');
      }
    }
    in.n_voices = nv;
    in.f64 = f64;
    in.block_size = bs;
    in.connected = connected;
    in.n_stages = stages.size();
    in.frame_eligible = std::all_of(stages.begin(), stages.end(), [](const StageInfo& S) { return frame_eligible(S.kind, S.flags, S.dcpb, S.ar_param); });
    in.dag = signature_is_dag(signature);
    in.n_delays = static_cast<unsigned>(std::count_if(signature.begin(), signature.end(), [](char c) { return c == 'D' || c == 'Y' || c == 'Z'; }));
    in.two_channel_pool = pool_channels() == 2;
    const char* const prebuilt_key = signature.c_str();
    in.prebuilt.one_wave = knh::find_kernel(prebuilt_key) != nullptr;
    for (int l = 0; l < 3; ++l)
      if (const knh::PipeEntry* p = knh::find_pipe(prebuilt_key, 1u << l)) in.prebuilt.pipe[l] = {true, p->long_tiles != 0};
    in.prebuilt.pair = knh::find_pipe(prebuilt_key, 1u << 2 /* PIPE_INPLACE */, 2) != nullptr;
    in.prebuilt.wide = knh::find_wide(prebuilt_key) != nullptr;
    const knh::FormPlan plan = knh::plan_forms(in, knh::form_switches_from_env());
    const std::string& sig = plan.signature;
    env_ranks = envelope_task_ranks(sig, stages, connected ? out_stage : nullptr);
    bool chosen = false, frame_asked = false, frame_fits = false;
    for (int k = 0; k < plan.n && !chosen; ++k) {
      ChosenForm f;
      f.is = plan.candidate[k];
      f.facts = knh::form_facts(f.is, f64);
      std::string why;
      switch (f.is.kind) {
        case KNH_DEBUG_FORM_FRAME_JIT:
        case KNH_DEBUG_FORM_FRAME_INTERP: {
          if (!frame_asked) {  // the parsed program says whether a voice fits the LDS a lane per frame
            frame_asked = true;
            if (!parse_frame_program(sig, stages, &h_prog, &interp_sigs, &interp_out)) return fail(KNH_ERR_UNSUPPORTED_CHAIN, "interpreter: malformed graph signature");
            frame_fits = knh::interp_lds_bytes(static_cast<unsigned>(h_prog.size()), static_cast<unsigned>(n_slots), interp_sigs, static_cast<unsigned>(bs), f64) <= 158u * 1024u;
          }
          if (!frame_fits) continue;
          if (f.is.kind == KNH_DEBUG_FORM_FRAME_INTERP) break;
          const unsigned tpv = ((static_cast<unsigned>(bs) + 63u) / 64u) * 64u;
          const size_t nwp = (static_cast<size_t>(n_slots) + 3u) & ~size_t(3);
          // voices per workgroup: as many as keep every CU busy, fit 1 024 threads and (beside the 64 KiB table) the LDS
          unsigned vpw = std::max(1u, nv / 256u);
          vpw = std::min(vpw, 1024u / tpv);
          while (vpw > 1u && 65536u + vpw * nwp * sizeof(W) > 156u * 1024u) --vpw;
          if (65536u + vpw * nwp * sizeof(W) > 156u * 1024u) continue;
          std::vector<knh::FrameOp> fops(h_prog.size());
          for (size_t i = 0; i < h_prog.size(); ++i) fops[i] = knh::FrameOp{h_prog[i].kind, h_prog[i].a, h_prog[i].b, h_prog[i].o, h_prog[i].slot};
          f.jit = knh::jit_frame_kernel(fops.data(), static_cast<unsigned>(fops.size()), interp_sigs, interp_out, static_cast<unsigned>(n_slots), vpw, tpv, f64, &why);
          if (!f.jit) {
            warnings.push_back("frame-parallel kernel not built (" + why.substr(0, 300) + "): the interpreter runs the voice");
            continue;
          }
          frame_vpw = vpw;
        } break;
        case KNH_DEBUG_FORM_PIPELINE_FUSED: {
          // the chain is cut into at most three stage groups of similar cost (estimated instructions per sample) and
          // instantiated as voice_pipe_kernel
          unsigned cuts[2];
          const unsigned n_cuts = partition_chain(sig, cuts);
          f.jit = knh::jit_pipe_kernel(sig.c_str(), cuts, n_cuts, f64, fma, &why);
          if (!f.jit) {
            // A chain of several delay stages for which the pipeline has no room is not refused: the next candidate takes it.
            const bool crashed = why.rfind("JIT_CRASH: ", 0) == 0;
            if (crashed || in.n_delays <= 1 || k + 1 == plan.n) return fail(crashed ? KNH_ERR_INTERNAL : KNH_ERR_UNSUPPORTED_CHAIN, "run-time fusion of chain '" + sig + "' (pipelined) failed: " + why);
            warnings.push_back("pipelined kernel not built (" + why.substr(0, 300) + "): the whole-chain form runs the voice");
            continue;
          }
        } break;
        case KNH_DEBUG_FORM_WHOLE_CHAIN_FUSED:
          f.jit = knh::jit_voice_kernel(sig.c_str(), f64, fma, &why, f.is.waves);
          if (!f.jit) return fail(why.rfind("JIT_CRASH: ", 0) == 0 ? KNH_ERR_INTERNAL : KNH_ERR_UNSUPPORTED_CHAIN, "run-time fusion of chain '" + sig + "' failed: " + why);
          break;
        case KNH_DEBUG_FORM_PIPELINE: {
          const knh::PipeEntry* p = knh::find_pipe(prebuilt_key, 1u << f.is.pipe_layout, f.is.pair ? 2 : 1);
          f.fn = launch_fn(p->f32, p->f64);
        } break;
        case KNH_DEBUG_FORM_MANY_WAVE: {
          const knh::WideEntry* w = knh::find_wide(prebuilt_key);
          f.fn = f.is.waves == 4 ? launch_fn(w->f32_w4, w->f64_w4) : f.is.waves == 8 ? launch_fn(w->f32_w8, w->f64_w8) : launch_fn(w->f32_w16, w->f64_w16);
        } break;
        default: {  // KNH_DEBUG_FORM_WHOLE_CHAIN
          const knh::KernelEntry* e = knh::find_kernel(prebuilt_key);
          f.fn = launch_fn(e->f32, e->f64);
        } break;
      }
      form = f;
      chosen = true;
    }
    if (!chosen) return fail(KNH_ERR_INTERNAL, "no kernel form stands for chain '" + sig + "'");
    const bool rows_per_voice = form.facts.rows_per_voice;
    sample_rate = sr;
    block_size = bs;
    stride = (static_cast<long>(nv) + 63) / 64 * 64;
    // osc.rs:144-145
    f2pi = 16384.0 * 65536.0 * (1.0 / static_cast<double>(sr));

    std::vector<W> st(static_cast<size_t>(n_slots) * stride, W(0));
    shadow.assign(stages.size(), Shadow{});
    // KNH_DEBUG_SVF_IC2_NEG0=1, tests only: every third voice's SvfFilter starts with ic2eq = -0.0, the one state no call of the
    // reference can produce and the one in which the low-pass tiles must take the general step (Svf::low_pass)
    const char* const neg0_env = std::getenv("KNH_DEBUG_SVF_IC2_NEG0");
    svf_ic2_neg0 = neg0_env && neg0_env[0] == '1';
    rings.clear();
    delay_len.clear();
    ring_of_stage.assign(stages.size(), -1);
    {  // the wavetables' places in their one allocation (add_wavetable has kept the sum within 32 bits)
      uint64_t off = 0;
      for (auto& entries : wt_pool)
        for (WtEntry& e : entries) { e.off = static_cast<uint32_t>(off); off += static_cast<uint64_t>(e.n_tables) * kWavetableSize; }
    }
    for (size_t si = 0; si < stages.size(); ++si) {
      const StageInfo& S = stages[si];
      const double* ca = ctor[si].data();
      { int rc = prepare_stage(si); if (rc != KNH_OK) return rc; }
      for (uint32_t v = 0; v < nv; ++v) {
        int rc = construct_stage(si, v, ca + static_cast<size_t>(v) * S.n_ctor,
                                 [&](int rel, W word) { st[static_cast<size_t>(S.slot_base + rel) * stride + v] = word; });
        if (rc != KNH_OK) return rc;
      }
    }
    fb_row0 = fb_granules = 0;
    for (size_t si = 0; si < stages.size(); ++si) {
      if (!stages[si].feedback()) continue;
      // FeedbackSink's buffer: one block (graph.rs:153-155), zero until the first block has gone through
      const uint64_t base = rings.empty() ? 0u : rings.back().base + static_cast<uint64_t>(nv) * rings.back().stride;
      const uint32_t own = (static_cast<uint32_t>(bs) + kRingGranule - 1u) / kRingGranule * kRingGranule;
      if ((base + static_cast<uint64_t>(nv) * own) / kRingGranule >= 0xFFFFFFFFull) return fail(KNH_ERR_INVALID_ARGUMENT, "the delay rings of the bank are too long in sum");
      if (fb_granules == 0) { fb_row0 = static_cast<uint32_t>(base / kRingGranule); fb_granules = own / kRingGranule; }
      ring_of_stage[si] = static_cast<int>(rings.size());
      rings.push_back(DelayRings{static_cast<uint32_t>(si), own, base});
      delay_len.resize(rings.size() * nv, 0u);
    }
    // device allocations
    KNH_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
    KNH_HIP(hipMalloc(&d_state, st.size() * sizeof(W)));
    KNH_HIP(hipMemcpy(d_state, st.data(), st.size() * sizeof(W), hipMemcpyHostToDevice));
    {  // NonAaWavetable::sine(), wavetable.rs:130-139: f64 sin, rounded to f32
      std::vector<float> table(16384);
      const double PI = 3.14159265358979323846;
      for (int i = 0; i < 16384; ++i) table[i] = static_cast<float>(std::sin((static_cast<double>(i) / 16384.0) * PI * 2.0));
      KNH_HIP(hipMalloc(&d_sine, 16384 * sizeof(float)));
      KNH_HIP(hipMemcpy(d_sine, table.data(), 16384 * sizeof(float), hipMemcpyHostToDevice));
    }
    if (!pool.empty()) {
      const size_t total = static_cast<size_t>(pool_samples_with(pool.size(), 0));
      KNH_HIP(hipMalloc(&d_buffer, total * sizeof(F)));
      KNH_HIP(hipMemset(d_buffer, 0, total * sizeof(F)));
      for (PoolEntry& e : pool) {
        KNH_HIP(hipMemcpy(d_buffer + e.off, e.samples.data(), e.samples.size() * sizeof(F), hipMemcpyHostToDevice));
        std::vector<F>().swap(e.samples);
      }
    }
    if (wt_samples() != 0) {
      KNH_HIP(hipMalloc(&d_wavetables, static_cast<size_t>(wt_samples()) * sizeof(F)));
      for (auto& entries : wt_pool)
        for (WtEntry& e : entries) {
          KNH_HIP(hipMemcpy(d_wavetables + e.off, e.samples.data(), e.samples.size() * sizeof(F), hipMemcpyHostToDevice));
          std::vector<F>().swap(e.samples);
        }
    }
    if (!rings.empty()) {
      // the sum over the delay stages of nv x the stage's stride
      const uint64_t samples = rings.back().base + static_cast<uint64_t>(nv) * rings.back().stride;
      uint32_t mx = 0;
      for (const DelayRings& r : rings) mx = std::max(mx, r.stride);
      delay_stride = kRingGranule;
      ring_sink_row = static_cast<uint32_t>(samples / kRingGranule);
      // (+ a spare ring behind the last one, as long as the longest: where lanes without a voice move their lines, voice_stages.hpp RingLines)
      const size_t bytes = (static_cast<size_t>(samples) + mx) * sizeof(F) + 4096;
      size_t free_b = 0, total_b = 0;
      KNH_HIP(hipMemGetInfo(&free_b, &total_b));
      if (bytes > free_b) return fail(KNH_ERR_DEVICE, "SampleDelay: the delay rings do not fit in device memory");
      KNH_HIP(hipMalloc(&d_delay, bytes));
      KNH_HIP(hipMemset(d_delay, 0, bytes));  // vec![F::ZERO; len]
    }
    if (!seg_rows.empty()) {
      KNH_HIP(hipMalloc(&d_seg_table, seg_rows.size() * sizeof(double)));
      KNH_HIP(hipMemcpy(d_seg_table, seg_rows.data(), seg_rows.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    const size_t n_waves = rows_per_voice ? nv : (nv + 63) / 64;  // rows the fold kernels take: one per wavefront, or (a lane per frame) one per voice
    if (rows_per_voice) {
      KNH_HIP(hipMalloc(&d_prog, h_prog.size() * sizeof(knh_dev::InterpOp)));
      KNH_HIP(hipMemcpy(d_prog, h_prog.data(), h_prog.size() * sizeof(knh_dev::InterpOp), hipMemcpyHostToDevice));
      std::vector<uint32_t> sins;
      for (const knh_dev::InterpOp& op : h_prog)
        if (op.kind == knh_dev::INTERP_SIN_WT) sins.push_back(op.slot);
      n_sin = static_cast<unsigned>(sins.size());
      KNH_HIP(hipMalloc(&d_sin_slots, std::max<size_t>(1, sins.size()) * sizeof(uint32_t)));
      if (!sins.empty()) KNH_HIP(hipMemcpy(d_sin_slots, sins.data(), sins.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    pan = !sig.empty() && (stages.back().kind == KNH_STAGE_PAN2 || connected);  // a Pan2 ends the chain, or two outputs are connected: every voice has a left and a right signal
    fold_planes = pan ? 2u : 1u;
    KNH_HIP(hipMalloc(&d_partials, fold_planes * n_waves * bs * sizeof(F)));
    KNH_HIP(hipMalloc(&d_out, desc.out_channels * bs * sizeof(F)));
    KNH_HIP(hipMemset(d_out, 0, desc.out_channels * bs * sizeof(F)));
    KNH_HIP(hipMalloc(&d_done, static_cast<size_t>(nv) * sizeof(uint32_t)));
    KNH_HIP(hipMemset(d_done, 0xFF, static_cast<size_t>(nv) * sizeof(uint32_t)));
    // three sets of 16 words, used by the launches in turn: the fold kernel of launch N clears the counters of launch N + 2's
    // set (it may run beside launch N + 1's voice kernel, which accumulates into its own: process)
    KNH_HIP(hipMalloc(&d_flags, 64 * sizeof(uint32_t)));  // (+ a fourth set: a resident launch's diagnostics)
    KNH_HIP(hipMemset(d_flags, 0, 64 * sizeof(uint32_t)));
    for (int b = 0; b < 2; ++b) {
      KNH_HIP(hipHostMalloc(&h_ev_start2[b], (static_cast<size_t>(nv) + 2) * sizeof(uint32_t)));
      // room for two events per voice from the start: a list that has to grow later costs a resident kernel its place (it knows
      // the lists by their addresses)
      h_events_cap2[b] = std::max<size_t>(2048, 2 * static_cast<size_t>(nv));
      KNH_HIP(hipHostMalloc(&h_events2[b], h_events_cap2[b] * sizeof(Event)));
      KNH_HIP(hipEventCreateWithFlags(&list_done[b], hipEventDisableTiming));
    }
    KNH_HIP(hipHostMalloc(&h_out, desc.out_channels * bs * sizeof(F) + 2 * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
    KNH_HIP(hipHostMalloc(&h_done, 64, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h_done, 0, 64);
    KNH_HIP(hipMalloc(&d_fold_count, sizeof(uint32_t)));
    KNH_HIP(hipMemset(d_fold_count, 0, sizeof(uint32_t)));
    if (desc.mix_mode == KNH_MIX_LEFT_FOLD) KNH_HIP(ensure_voices());
    bool any_wrapped = false;
    for (auto& S : stages) any_wrapped = any_wrapped || S.dcpb > 0;
    if (any_wrapped) next_delay.assign(static_cast<size_t>(n_params_total) * nv, 0);
    wrapped_index.assign(stages.size(), -1);
    n_wrapped = 0;
    for (size_t si = 0; si < stages.size(); ++si)
      if (fastq(stages[si])) wrapped_index[si] = static_cast<int>(n_wrapped++);
    node_q.assign(static_cast<size_t>(nv) * n_wrapped, NodeQ{0u, 0, 0, 0});
    {  // which of the wrapped nodes have their queues resolved on the device (kernels_events.hip): up to eight per voice
      const char* de = std::getenv("KNH_DEV_EVENTS");
      stage_dev.assign(stages.size(), 0);
      std::vector<knh_dev::DevStage> ds(stages.size());
      int n_dev = 0;
      for (size_t si = 0; si < stages.size(); ++si) {
        const StageInfo& S = stages[si];
        const bool on = fastq(S) && dev_resolvable_kind(S.kind) && !S.wavetable() && n_dev < 8 && !(de && de[0] == '0') && S.slot_base < 65536 && n_params_total < 65536;
        ds[si] = knh_dev::DevStage{S.kind, S.dcpb, static_cast<unsigned short>(S.slot_base), static_cast<unsigned short>(S.param_base), S.flags, S.ar_param,
                                   static_cast<short>(on ? n_dev : -1), 0};
        if (on) { stage_dev[si] = 1; ++n_dev; }
      }
      dev_class.assign(stages.size() * 8u, 0);
      for (size_t si = 0; si < stages.size(); ++si)
        if (stage_dev[si])
          for (int pp = 0; pp < stages[si].n_params && pp < 8; ++pp) dev_class[si * 8u + pp] = static_cast<uint8_t>(1 + expected_value_kind(stages[si].kind, pp));
      if (n_dev > 0) {
        const int rc = resolver.init(DevEventResolver::Setup{this, nv, static_cast<uint32_t>(n_params_total), static_cast<uint32_t>(bs), sr, sizeof(F) == 8, f2pi}, ds);
        if (rc != KNH_OK) return rc;
      }
    }
    smooth.assign(stages.size(), {});
    smooth_mark.assign(stages.size(), {});
    for (size_t si = 0; si < stages.size(); ++si)
      if (stages[si].flags & KNH_STAGE_FLAG_SMOOTH_PARAMS) {
        smooth[si].assign(static_cast<size_t>(nv) * stages[si].n_params, SmoothState{});
        smooth_mark[si].assign(nv, 0u);
      }
    can_finish = chain_can_finish(stages);
    {  // the per-block call on a resident launch (resident_call.hpp): what it needs to know of this bank, now that the kernel form is chosen
      typename ResidentCall<F>::Setup rs{};
      rs.bank = this;
      rs.own_stream = own_stream;
      rs.n_rows = (nv + 63u) / 64u;
      rs.fold_planes = fold_planes;
      rs.out_channels = desc.out_channels;
      rs.block_size = static_cast<uint32_t>(bs);
      rs.tile_frames = form.facts.tile_frames;
      rs.can_finish = can_finish;
      rs.ev_start = h_ev_start2;
      rs.events = h_events2;
      rs.launch_voice = [this](const knh_dev::Resident& r) {
        VoiceKernelArgs<F> a;
        fill_launch_args(a, 1, 0, static_cast<uint32_t>(block_size));
        a.flags = d_flags + 48;  // (a set of its own: the three the ordinary launches rotate stay as their fold kernels left them)
        a.res = r;
        return launch_voice(a, (nv + 63) / 64, own_stream);
      };
      resident.setup(rs);
    }
    signature = sig;
    initialised = true;
    return KNH_OK;
  }
  bool can_finish = false;   // the chain has a stage that can end a voice (ALL_DONE is reported only then)
  bool pan = false;          // the chain ends in a Pan2, or has two connected outputs
  F* stage_out = nullptr;    // set by a bank that wraps this one (galactic_bank.hpp): the voices' signals of the block go here, [n_voices][block_size] -- [2][n_voices][block_size], left plane then right, when two outputs are connected
  unsigned fold_planes = 1;  // channel planes of the partial rows and of the per-voice output: 2 for a Pan2 chain and for connected outputs
  hipError_t ensure_voices() {
    if (d_voices) return hipSuccess;
    return hipMalloc(&d_voices, static_cast<size_t>(fold_planes) * nv * block_size * sizeof(F));
  }

  // ---- restarting voices ---------------------------------------------------------------
  // knh_bank_restart_voices: what the reference has after a voice's nodes are freed (graph.rs:2483-2513) and the same chain is
  // pushed and initialised again.  The host runs the construction again at the call (construct_stage: the shadows the setters
  // read are the new nodes' from then on) and keeps the voices' rows; the next launch -- or whatever reads the state first --
  // puts them on the device, in front of its voice kernel on its stream (restart_voices_kernel, kernels_restart.hip).
  bool mid_block = false;             // the last process call ended inside a block
  std::vector<uint8_t> rs_mark;       // [voice]: named by the call being made
  std::vector<int32_t> rs_row;        // [voice] -> its row among those waiting, -1: none
  std::vector<uint32_t> rs_voices;    // the rows waiting for the device: voice, state words, segment rows
  std::vector<W> rs_words;
  std::vector<double> rs_seg;
  uint32_t* h_rs_voices = nullptr;    // pinned: what the kernel reads
  W* h_rs_words = nullptr;
  double* h_rs_seg = nullptr;
  size_t h_rs_cap = 0;                // rows
  hipEvent_t rs_done = nullptr;       // behind the last restart kernel
  bool rs_busy = false;
  int set_voice_ctor(uint32_t stage, size_t count, const uint32_t* voices, const double* args, uint32_t n_args, bool keep) override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    if (stage >= stages.size()) return fail(KNH_ERR_OUT_OF_RANGE, "stage out of range");
    const StageInfo& S = stages[stage];
    if (static_cast<int>(n_args) != S.n_ctor) return fail(KNH_ERR_INVALID_ARGUMENT, "wrong number of constructor arguments");
    if (count && (!voices || (n_args && !args))) return fail(KNH_ERR_INVALID_ARGUMENT, "null array");
    for (size_t k = 0; k < count; ++k)
      if (voices[k] >= nv) return fail(KNH_ERR_OUT_OF_RANGE, "voice out of range");
    if (mid_block) return fail(KNH_ERR_INVALID_ARGUMENT, "a block is partly processed: voices restart between blocks");
    for (size_t k = 0; k < count; ++k) {  // what knh_bank_init would refuse, and a ring the allocation made at init cannot hold
      const double* a = args + k * n_args;
      if (S.kind == KNH_STAGE_SAMPLE_DELAY || S.kind == KNH_STAGE_ALLPASS_DELAY || S.kind == KNH_STAGE_ALLPASS_FB_DELAY) {
        uint32_t len = 0;
        int rc = delay_ring_len(S, a, &len);
        if (rc != KNH_OK) return rc;
        // (the stage's own rings: another delay stage's longer ones are no room for this one's)
        if (len > rings[static_cast<size_t>(ring_of_stage[stage])].stride) return fail(KNH_ERR_OUT_OF_RANGE, "the delay's ring would be longer than the rings allocated at knh_bank_init");
      }
      if (S.kind == KNH_STAGE_INPUT && !S.feedback() && (!(a[0] >= 0.0) || a[0] >= static_cast<double>(desc.in_channels)))
        return fail(KNH_ERR_INVALID_ARGUMENT, "KNH_STAGE_INPUT: channel is not below knh_bank_desc.in_channels");
    }
    for (size_t k = 0; k < count && n_args && keep; ++k)
      std::copy(args + k * n_args, args + (k + 1) * n_args, ctor[stage].begin() + static_cast<size_t>(voices[k]) * n_args);
    return KNH_OK;
  }
  // Everything already said to the nodes of the marked voices is dropped -- patches of the coming launch and of later ones,
  // calls kept for later blocks, records and changes waiting in a WrPreciseTiming queue, ramps of WrSmoothParams -- and the
  // wrappers' host state is a new node's: they addressed nodes that no longer exist.
  void forget_voices(const std::vector<uint8_t>& marked, const std::vector<uint32_t>& list) {
    expand_ranges();
    auto drop = [&](auto& vec, auto&& voice_of) {
      vec.erase(std::remove_if(vec.begin(), vec.end(), [&](const auto& x) { return marked[voice_of(x)] != 0; }), vec.end());
    };
    drop(pending, [](const HostEvent& e) { return e.voice; });
    for (auto& calls : future) drop(calls, [](const Call& c) { return c.voice; });
    for (auto& recs : qfuture) drop(recs, [](const QRec& r) { return r.voice; });
    const uint64_t ns = stages.size();
    drop(queued, [ns](const std::pair<uint64_t, QueuedChange>& q) { return static_cast<uint32_t>(q.first / ns); });
    drop(smooth_active, [ns](uint64_t key) { return static_cast<uint32_t>(key / ns); });
    if (resolver.active()) resolver.drop_voices(marked);
    for (uint32_t v : list) {
      for (size_t si = 0; si < stages.size(); ++si) {
        const StageInfo& S = stages[si];
        if (!smooth[si].empty()) {
          std::fill_n(smooth[si].begin() + static_cast<size_t>(v) * S.n_params, S.n_params, SmoothState{});
          smooth_mark[si][v] = 0u;
        }
        if (S.dcpb > 0 && !next_delay.empty())
          for (int p = 0; p < S.n_params; ++p) next_delay[static_cast<size_t>(S.param_base + p) * nv + v] = 0;
      }
      for (uint32_t w = 0; w < n_wrapped; ++w) node_q[static_cast<size_t>(v) * n_wrapped + w] = NodeQ{0u, 0, 0, 0};
    }
  }
  int restart_voices(size_t count, const uint32_t* voices) override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    if (count && !voices) return fail(KNH_ERR_INVALID_ARGUMENT, "null array");
    for (size_t k = 0; k < count; ++k)
      if (voices[k] >= nv) return fail(KNH_ERR_OUT_OF_RANGE, "voice out of range");
    if (mid_block) return fail(KNH_ERR_INVALID_ARGUMENT, "a block is partly processed: voices restart between blocks");
    if (count == 0) return KNH_OK;
    { int rl = resident.leave(); if (rl != KNH_OK) return rl; }  // (a resident kernel holds the voices' state in its registers)
    rs_mark.assign(nv, 0);
    if (rs_row.empty()) rs_row.assign(nv, -1);
    std::vector<uint32_t> list;  // each voice once
    for (size_t k = 0; k < count; ++k)
      if (!rs_mark[voices[k]]) { rs_mark[voices[k]] = 1; list.push_back(voices[k]); }
    forget_voices(rs_mark, list);
    const size_t n_seg = static_cast<size_t>(seg_max) * 3u;
    for (uint32_t v : list) {
      if (rs_row[v] < 0) {  // (restarted twice between two launches: the later construction stands)
        rs_row[v] = static_cast<int32_t>(rs_voices.size());
        rs_voices.push_back(v);
        rs_words.resize(rs_voices.size() * static_cast<size_t>(n_slots));
        rs_seg.resize(rs_voices.size() * n_seg);
      }
      W* row = rs_words.data() + static_cast<size_t>(rs_row[v]) * n_slots;
      std::fill_n(row, n_slots, W(0));
      for (size_t si = 0; si < stages.size(); ++si) {
        const StageInfo& S = stages[si];
        int rc = construct_stage(si, v, ctor[si].data() + static_cast<size_t>(v) * (S.n_ctor > 0 ? S.n_ctor : 0),
                                 [&](int rel, W word) { row[S.slot_base + rel] = word; });
        if (rc != KNH_OK) return rc;  // (not reached: the arguments were checked when they were given)
      }
      if (n_seg) std::copy_n(seg_rows.begin() + static_cast<size_t>(v) * n_seg, n_seg, rs_seg.begin() + static_cast<size_t>(rs_row[v]) * n_seg);
    }
    return KNH_OK;
  }
  // The rows that wait go to the device on `s`, the stream of what reads the state next.
  int flush_restart(hipStream_t s) {
    if (rs_voices.empty()) return KNH_OK;
    const size_t n = rs_voices.size(), n_seg = static_cast<size_t>(seg_max) * 3u;
    if (flags_stream_set && flags_stream != s) KNH_HIP(hipStreamSynchronize(flags_stream));  // the launch before wrote the state in that stream's order
    if (!rs_done) KNH_HIP(hipEventCreateWithFlags(&rs_done, hipEventDisableTiming));
    if (rs_busy) { KNH_HIP(hipEventSynchronize(rs_done)); rs_busy = false; }  // the kernel of the restart before reads the pinned rows
    if (n > h_rs_cap) {
      void* old[] = {h_rs_voices, h_rs_words, h_rs_seg};
      for (void* p : old)
        if (p) KNH_HIP(hipHostFree(p));
      h_rs_voices = nullptr; h_rs_words = nullptr; h_rs_seg = nullptr;
      h_rs_cap = 0;
      const size_t cap = std::max<size_t>(n, 64);
      KNH_HIP(hipHostMalloc(&h_rs_voices, cap * sizeof(uint32_t)));
      KNH_HIP(hipHostMalloc(&h_rs_words, std::max<size_t>(cap * static_cast<size_t>(n_slots), 1) * sizeof(W)));
      if (n_seg) KNH_HIP(hipHostMalloc(&h_rs_seg, cap * n_seg * sizeof(double)));
      h_rs_cap = cap;
    }
    std::copy(rs_voices.begin(), rs_voices.end(), h_rs_voices);
    std::copy(rs_words.begin(), rs_words.end(), h_rs_words);
    if (n_seg) std::copy(rs_seg.begin(), rs_seg.end(), h_rs_seg);
    knh_dev::RestartArgs ra{};
    ra.voices = h_rs_voices;
    ra.words = h_rs_words;
    ra.seg_rows = h_rs_seg;
    ra.state = d_state;
    ra.stride = stride;
    ra.n_slots = static_cast<uint32_t>(n_slots);
    ra.n_voices = nv;
    ra.f64 = sizeof(F) == 8 ? 1u : 0u;
    ra.done_frames = d_done;
    ra.armed = resolver.active() ? resolver.armed() : nullptr;
    ra.n_params_total = static_cast<uint32_t>(n_params_total);
    ra.seg_table = n_seg ? d_seg_table : nullptr;
    ra.seg_max = seg_max;
    ra.delay_ring = d_delay;
    ra.n_rings = static_cast<uint32_t>(rings.size());  // (at most KNH_MAX_DELAY_STAGES: build_signature)
    for (size_t r = 0; r < rings.size() && r < static_cast<size_t>(KNH_MAX_DELAY_STAGES); ++r) { ra.ring_base[r] = rings[r].base; ra.ring_stride[r] = rings[r].stride; }
    if (resolver.active()) { int rc = resolver.restart_may_write(s); if (rc != KNH_OK) return rc; }
    KNH_HIP(knh::launch_restart_voices(ra, static_cast<unsigned>(n), s));
    KNH_HIP(hipEventRecord(rs_done, s));
    rs_busy = true;
    if (resolver.active()) { int rc = resolver.restart_written(rs_done); if (rc != KNH_OK) return rc; }
    for (uint32_t v : rs_voices) rs_row[v] = -1;
    rs_voices.clear(); rs_words.clear(); rs_seg.clear();
    return KNH_OK;
  }

  // ---- parameter changes ----------------------------------------------------------------
  int check_target(uint32_t voice, uint32_t stage, uint32_t param) {
    // a Math1UGen has no parameters at all (math.rs:167-305): a call that names one is a mistake about the stage, not an index a
    // little too large -- every parameter entry point comes through here (or through RankBank's copy of these checks).  Ahead of
    // the initialised check on purpose: the chain is known from knh_bank_create on (knaster_hip.h says so)
    if (stage < stages.size() && is_math1_kind(stages[stage].kind)) return fail(KNH_ERR_INVALID_ARGUMENT, "a KNH_STAGE_MATH1_* stage has no parameters");
    if (stage < stages.size() && no_params_message(stages[stage])) return fail(KNH_ERR_INVALID_ARGUMENT, no_params_message(stages[stage]));  // (the same rule: it is no node)
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    if (voice >= nv) return fail(KNH_ERR_OUT_OF_RANGE, "voice out of range");
    if (stage >= stages.size()) return fail(KNH_ERR_OUT_OF_RANGE, "stage out of range");
    if (param >= static_cast<uint32_t>(stages[stage].n_params)) return fail(KNH_ERR_OUT_OF_RANGE, "parameter index out of range");
    return KNH_OK;
  }
  int set_delay(uint32_t voice, uint32_t stage, uint32_t param, uint16_t delay) override {
    int rc = check_target(voice, stage, param);
    if (rc != KNH_OK) return rc;
    const StageInfo& S = stages[stage];
    if (S.dcpb == 0) {  // ugen.rs:339-341
      warn("Parameter delay set, but the stage is not wrapped in WrPreciseTiming; no effect");
      return KNH_OK;
    }
    if (fastq(S)) {
      QRec r{};
      r.voice = voice; r.delay = delay; r.stage = static_cast<uint16_t>(stage); r.param = static_cast<uint8_t>(param); r.kb = 0x10u;
      return push_rec(0, r);
    }
    next_delay[static_cast<size_t>(S.param_base + param) * nv + voice] = delay;  // precise_timing.rs:146-148
    return KNH_OK;
  }
  int param_apply(uint32_t voice, uint32_t stage, uint32_t param, uint32_t kind, double f, int64_t i) override {
    int rc = check_target(voice, stage, param);
    if (rc != KNH_OK) return rc;
    const StageInfo& S = stages[stage];
    if (!kind_ok(S, param, kind)) return fail(KNH_ERR_WRONG_VALUE_KIND, "parameter value kind does not match the parameter type");
    if (fastq(S) && frame_base == 0) {  // (frame_base != 0: a replay inside process, which has its own order)
      return push_rec(0, make_qrec(voice, stage, param, kind, f, i, 0, false));
    }
    if (S.dcpb > 0) {  // WrPreciseTiming::param_apply, precise_timing.rs:126-135
      uint16_t d = next_delay[static_cast<size_t>(S.param_base + param) * nv + voice];
      if (d != 0) {  // capacity (DELAYED_CHANGES_PER_BLOCK) is enforced per node when the block is assembled
        queued.emplace_back(static_cast<uint64_t>(voice) * stages.size() + stage, QueuedChange{d, param, kind, f, i});
        return KNH_OK;
      }
    }
    deliver(voice, stage, param, kind, f, i, frame_base);
    return KNH_OK;
  }
  static QRec make_qrec(uint32_t voice, uint32_t stage, uint32_t param, uint32_t kind, double f, int64_t i, uint16_t delay, bool arm) {
    QRec r{};
    r.voice = voice; r.delay = delay; r.stage = static_cast<uint16_t>(stage); r.param = static_cast<uint8_t>(param);
    r.kb = static_cast<uint8_t>((kind & 15u) | (arm ? 0x10u : 0u) | 0x20u);
    if (kind == KNH_VALUE_FLOAT) r.v.f = f; else r.v.i = i;
    return r;
  }
  static bool kind_ok(const StageInfo& S, uint32_t param, uint32_t kind) {
    const int want = expected_value_kind(S.kind, param);
    if (static_cast<int>(kind) == want) return true;
    // ParameterValue::Smoothing is accepted by a WrSmoothParams-wrapped node for its Float parameters; without
    // the wrapper the reference's generated param_apply panics on it (knaster_macros/src/lib.rs:601-606,752-757)
    return kind == KNH_VALUE_SMOOTHING && (S.flags & KNH_STAGE_FLAG_SMOOTH_PARAMS) && want == KNH_VALUE_FLOAT;
  }
  // WrSmoothParams::param_apply (smooth_params.rs:210-259) in front of the node's own setters.
  void deliver(uint32_t voice, uint32_t stage, uint32_t param, uint32_t kind, double f, int64_t iv, uint32_t frame) {
    const StageInfo& S = stages[stage];
    if (!(S.flags & KNH_STAGE_FLAG_SMOOTH_PARAMS) || (kind != KNH_VALUE_FLOAT && kind != KNH_VALUE_SMOOTHING)) {
      apply_now(voice, stage, param, f, iv, frame, pending);
      return;
    }
    SmoothState& st = smooth[stage][static_cast<size_t>(voice) * S.n_params + param];
    if (kind == KNH_VALUE_SMOOTHING) {  // set_smoothing, :30-102
      if (iv == 0) {
        if (st.linear) {
          double cv = st.interpolated();
          st = SmoothState{};
          st.current_value = cv;
        }
        return;
      }
      const size_t dur = static_cast<size_t>(static_cast<double>(static_cast<float>(f)) * static_cast<double>(sample_rate));
      if (!st.linear) {
        double cv = st.current_value;
        st.linear = true;
        st.start_value = cv;
        st.end_value = cv;
        st.frames_elapsed = 0;
      } else if (st.done) {
        st.start_value = st.end_value;
        st.frames_elapsed = 0;
      } else {
        st.start_value = st.interpolated();
      }
      st.duration_frames = dur;
      st.audio_rate = iv == 2;
      st.done = true;
      return;
    }
    if (!st.linear) {  // no smoothing selected for this parameter: straight through
      apply_now(voice, stage, param, f, iv, frame, pending);
      return;
    }
    st.start_value = st.done ? st.end_value : st.interpolated();
    st.end_value = f;
    st.done = false;
    st.frames_elapsed = 0;
    uint32_t& mark = smooth_mark[stage][voice];
    if (!(mark & 1u)) {
      mark |= 1u;
      smooth_active.push_back(static_cast<uint64_t>(voice) * stages.size() + stage);
    }
  }
  // WrSmoothParams::process_block's block-rate step (:188-197) for one node, at the start of a (partial) block.
  void smooth_tick(uint32_t voice, uint32_t stage, uint32_t frame) {
    const StageInfo& S = stages[stage];
    SmoothState* st = &smooth[stage][static_cast<size_t>(voice) * S.n_params];
    for (int p = 0; p < S.n_params; ++p) {
      SmoothState& x = st[p];
      if (!x.linear || x.done) continue;  // next_value, :263-300 (frame_in_block is 0 on this path)
      const double v = x.interpolated();
      if (x.frames_elapsed == x.duration_frames) x.done = true;
      else if (x.audio_rate) x.frames_elapsed += 1;
      else x.frames_elapsed = std::min(x.frames_elapsed + block_size, x.duration_frames);
      apply_now(voice, stage, static_cast<uint32_t>(p), v, 0, frame_base + frame, pending);
    }
    smooth_mark[stage][voice] = (smooth_mark[stage][voice] & 1u) | (smooth_epoch << 1);
  }
  // The same two calls addressed to block `block_offset` of the next multi-block launch: validated now,
  // replayed in order when that block is assembled.
  int check_call(uint32_t voice, uint32_t stage, uint32_t param, uint32_t kind) override {
    int rc = check_target(voice, stage, param);
    if (rc != KNH_OK) return rc;
    if (!kind_ok(stages[stage], param, kind)) return fail(KNH_ERR_WRONG_VALUE_KIND, "parameter value kind does not match the parameter type");
    return KNH_OK;
  }
  int call_at(uint32_t block_offset, bool is_delay, uint32_t voice, uint32_t stage, uint32_t param, uint32_t kind, double f,
              int64_t i, uint16_t delay) override {
    if (block_offset == 0) return is_delay ? set_delay(voice, stage, param, delay) : param_apply(voice, stage, param, kind, f, i);
    int rc = check_target(voice, stage, param);
    if (rc != KNH_OK) return rc;
    if (block_offset >= 65536) return fail(KNH_ERR_OUT_OF_RANGE, "block_offset too large");
    if (!is_delay && !kind_ok(stages[stage], param, kind))
      return fail(KNH_ERR_WRONG_VALUE_KIND, "parameter value kind does not match the parameter type");
    if (fastq(stages[stage])) {
      if (is_delay) {
        QRec r{};
        r.voice = voice; r.delay = delay; r.stage = static_cast<uint16_t>(stage); r.param = static_cast<uint8_t>(param); r.kb = 0x10u;
        return push_rec(block_offset, r);
      }
      return push_rec(block_offset, make_qrec(voice, stage, param, kind, f, i, 0, false));
    }
    if (future.size() <= block_offset) future.resize(block_offset + 1);
    future[block_offset].push_back(Call{static_cast<uint8_t>(is_delay), delay, voice, stage, param, kind, f, i});
    return KNH_OK;
  }

  // A parameter whose device patches depend on the new value alone (no shadow of an earlier value is read, and no other
  // parameter's patches touch the same words): a call for a later block of the launch can be turned into its patches
  // at once, instead of being kept and replayed when that block is assembled.  Stages wrapped in WrPreciseTiming or
  // WrSmoothParams keep state on the host per call and always take the general path.
  bool direct_ok(const StageInfo& S, uint32_t param) const {
    if (S.dcpb > 0 || (S.flags & KNH_STAGE_FLAG_SMOOTH_PARAMS)) return false;
    switch (S.kind) {
      case KNH_STAGE_SVF: return false;             // every setter recomputes from the three shadows
      case KNH_STAGE_BUFFER_READER: return false;   // start / duration / rate shadows
      case KNH_STAGE_SIN_WT: return !(S.wavetable() && param == 0);  // OscWt's table word is the new freq's on the voice's entry at that block
      case KNH_STAGE_MUL_ENV_ASR: case KNH_STAGE_MUL_ENV_AR: return param >= 2;  // the times skip when unchanged (shadow); the triggers do not
      default: return true;
    }
  }
  // knh_bank_param_apply_range: an envelope trigger for the voices [v0, v1) is one range event, in O(1); anything else is the
  // batch it stands for (bank_base.hpp).
  int apply_range(uint32_t v0, uint32_t v1, uint32_t stage, uint32_t param, uint32_t kind, double f, int64_t iv) override {
    if (v1 > v0 && v1 <= nv && v1 - v0 >= 16 && initialised && stage < stages.size() && kind == KNH_VALUE_TRIGGER &&
        param < static_cast<uint32_t>(stages[stage].n_params) && kind_ok(stages[stage], param, kind) && direct_ok(stages[stage], param) &&
        (stages[stage].kind == KNH_STAGE_MUL_ENV_ASR || stages[stage].kind == KNH_STAGE_MUL_ENV_AR) &&
        !(stages[stage].ar_param != 0 && param + 1u == stages[stage].ar_param) && pending_ranges.size() < 64) {
      const StageInfo& S = stages[stage];
      note_frame(0u);
      const bool release = S.kind == KNH_STAGE_MUL_ENV_ASR && param == 2;
      pending_ranges.push_back(RangeEvent{v0, v1, 0u, release ? static_cast<uint32_t>(knh_dev::EV_ENV_ASR_RELEASE) : static_cast<uint32_t>(knh_dev::EV_SET),
                                          static_cast<uint32_t>(S.slot_base), release ? 0ull : 1ull, pending.size()});
      return KNH_OK;
    }
    return knh_bank::apply_range(v0, v1, stage, param, kind, f, iv);
  }
  // knh_bank_param_apply_many[_at]: runs of calls to the same (stage, parameter, kind) -- how a host sends "this parameter
  // of these voices" -- are checked once and turned into patches in one pass; anything else goes call by call.
  int apply_many(uint32_t block_offset, size_t count, const uint32_t* voices, const uint32_t* stgs, const uint32_t* params,
                 const uint32_t* kinds, const double* fvalues, const int64_t* ivalues, const uint16_t* delays) override {
    if (!initialised || count < 16 || block_offset >= 65536) return knh_bank::apply_many(block_offset, count, voices, stgs, params, kinds, fvalues, ivalues, delays);
    int rc = KNH_OK;
    size_t k = 0;
    while (k < count) {
      if (resolver.active()) {
        // Calls to nodes whose queues the DEVICE resolves: one table look-up and one 24-byte record in pinned memory per call,
        // whatever the order of stages and parameters in the batch (a host that addresses two parameters of alternate voices
        // -- BASELINE config C5 -- sends runs of one call).  dev_class[stage][param] = 1 + the ParameterValue kind it takes.
        const size_t ns = stages.size();
        if (stgs[k] < ns && params[k] < 8u && kinds[k] < 8u && dev_class[stgs[k] * 8u + params[k]] == kinds[k] + 1u) {
          int r2 = resolver.reserve(count - k);
          if (r2 != KNH_OK) return r2;
          uint64_t* out = reinterpret_cast<uint64_t*>(resolver.tail());  // three 8-byte words per record (QRec's layout)
          const uint64_t blk = static_cast<uint64_t>(block_offset & 0xFFFFu) << 16;
          size_t p = k, w = 0;
          for (; p < count; ++p) {
            const uint32_t st = stgs[p], pr = params[p], kd = kinds[p];
            if (!(st < ns && pr < 8u && kd < 8u && dev_class[st * 8u + pr] == kd + 1u)) break;
            const uint32_t v = voices[p];
            if (v >= nv) { rc = fail(KNH_ERR_OUT_OF_RANGE, "voice out of range"); continue; }
            const uint64_t d = delays ? delays[p] : 0u;
            uint64_t val;
            if (kd == KNH_VALUE_FLOAT) { const double f = fvalues ? fvalues[p] : 0.0; std::memcpy(&val, &f, 8); }
            else { const int64_t iv = ivalues ? ivalues[p] : 0; std::memcpy(&val, &iv, 8); }
            out[3 * w + 0] = static_cast<uint64_t>(v) | (d << 32) | (static_cast<uint64_t>(st) << 48);
            out[3 * w + 1] = static_cast<uint64_t>(pr) | (static_cast<uint64_t>(kd | (d ? 0x10u : 0u) | 0x20u) << 8) | blk;
            out[3 * w + 2] = val;
            ++w;
          }
          resolver.commit(w, block_offset);
          k = p;
          continue;
        }
      }
      size_t e = k + 1;
      {  // (64 entries at a time without a branch in between -- the compiler vectorises that -- then the ragged end one by one:
         // a bank's 16 384 triggers are 200 KB of arrays to look through)
        const uint32_t s0 = stgs[k], p0 = params[k], k0 = kinds[k];
        while (e + 64 <= count) {
          uint32_t d = 0;
          for (size_t q = e; q < e + 64; ++q) d |= (stgs[q] ^ s0) | (params[q] ^ p0) | (kinds[q] ^ k0);
          if (d) break;
          e += 64;
        }
      }
      while (e < count && stgs[e] == stgs[k] && params[e] == params[k] && kinds[e] == kinds[k]) ++e;
      bool direct = e - k >= 16 && stgs[k] < stages.size() && params[k] < static_cast<uint32_t>(stages[stgs[k]].n_params) &&
                    kind_ok(stages[stgs[k]], params[k], kinds[k]) && direct_ok(stages[stgs[k]], params[k]);
      if (direct && delays)
        for (size_t q = k; q < e && direct; ++q) direct = delays[q] == 0;  // an armed delay on an unwrapped stage: the warning path
      // Calls already kept for that block (they are replayed when the block is assembled) come first: a later call must not
      // overtake them by being turned into its patches now (two changes of one parameter in one block: the last one holds).
      if (direct && block_offset > 0 && block_offset < future.size() && !future[block_offset].empty()) direct = false;
      // (runs of any length: a host that addresses two parameters of alternate voices sends runs of one)
      const bool queued_run = !direct && stgs[k] < stages.size() && params[k] < static_cast<uint32_t>(stages[stgs[k]].n_params) &&
                              fastq(stages[stgs[k]]) && kind_ok(stages[stgs[k]], params[k], kinds[k]) && kinds[k] != KNH_VALUE_SMOOTHING;
      if (queued_run) {  // calls to a WrPreciseTiming-wrapped node: one record each (arm the delay, then the value)
        std::vector<QRec>& q = qblock(block_offset);
        if (q.capacity() < q.size() + (e - k)) q.reserve(std::max(q.size() + (count - k), q.capacity() * 2));
        const uint32_t stage = stgs[k], param = params[k], kind = kinds[k];
        for (size_t p = k; p < e; ++p) {
          const uint32_t v = voices[p];
          if (v >= nv) { rc = fail(KNH_ERR_OUT_OF_RANGE, "voice out of range"); continue; }
          const uint16_t d = delays ? delays[p] : 0;
          q.push_back(make_qrec(v, stage, param, kind, fvalues ? fvalues[p] : 0.0, ivalues ? ivalues[p] : 0, d, d > 0));
        }
      } else if (direct && kinds[k] == KNH_VALUE_TRIGGER && (stages[stgs[k]].kind == KNH_STAGE_MUL_ENV_ASR || stages[stgs[k]].kind == KNH_STAGE_MUL_ENV_AR) &&
                 !(stages[stgs[k]].ar_param != 0 && params[k] + 1u == stages[stgs[k]].ar_param)) {
        // An envelope trigger for a run of voices (the note-on / note-off of a whole bank): the patch is the same for every voice
        // (apply_now: EV_SET state = Attacking, or the release op) -- one event template, stamped with each voice's index.
        const StageInfo& S = stages[stgs[k]];
        const uint32_t frame = block_offset * static_cast<uint32_t>(block_size);
        note_frame(frame);
        const bool release = S.kind == KNH_STAGE_MUL_ENV_ASR && params[k] == 2;
        HostEvent t{0u, frame, release ? static_cast<uint32_t>(knh_dev::EV_ENV_ASR_RELEASE) : static_cast<uint32_t>(knh_dev::EV_SET), static_cast<uint32_t>(S.slot_base), release ? 0ull : 1ull};
        {  // neighbouring voices in rising order (the usual way to address a bank): one range event
          bool run = voices[e - 1] < nv && pending_ranges.size() < 64;
          size_t q = k + 1;
          for (; q + 64 <= e && run; q += 64) {  // (branch-free runs of 64, as above)
            uint32_t d = 0;
            for (size_t j = q; j < q + 64; ++j) d |= voices[j] - voices[j - 1] - 1u;
            run = d == 0;
          }
          for (; q < e && run; ++q) run = voices[q] == voices[q - 1] + 1u;
          if (run) {
            pending_ranges.push_back(RangeEvent{voices[k], voices[e - 1] + 1u, frame, t.op, t.slot, t.bits, pending.size()});
            k = e;
            continue;
          }
        }
        const size_t at = pending.size();
        pending.resize(at + (e - k));
        HostEvent* out = pending.data() + at;
        size_t w = 0;
        for (size_t q = k; q < e; ++q) {
          const uint32_t v = voices[q];
          if (v >= nv) { rc = fail(KNH_ERR_OUT_OF_RANGE, "voice out of range"); continue; }
          t.voice = v;
          out[w++] = t;
        }
        pending.resize(at + w);
      } else if (direct) {
        const uint32_t stage = stgs[k], param = params[k];
        const uint32_t frame = block_offset * static_cast<uint32_t>(block_size);
        pending.reserve(pending.size() + (e - k) * 2);
        for (size_t q = k; q < e; ++q) {
          const uint32_t v = voices[q];
          if (v >= nv) { rc = fail(KNH_ERR_OUT_OF_RANGE, "voice out of range"); continue; }
          apply_now(v, stage, param, fvalues ? fvalues[q] : 0.0, ivalues ? ivalues[q] : 0, frame, pending);
        }
      } else {
        int r = knh_bank::apply_many(block_offset, e - k, voices + k, stgs + k, params + k, kinds + k, fvalues ? fvalues + k : nullptr,
                                     ivalues ? ivalues + k : nullptr, delays ? delays + k : nullptr);
        if (r != KNH_OK) rc = r;
      }
      k = e;
    }
    return rc;
  }

  // The parameter setters of each UGen, restated as "new shadow value -> device patches".
  // Events reach `pending` in application order; a voice's list must also be in frame order.  As long as every new event's
  // frame is at least the largest one seen, both hold by construction and the per-voice sort of upload_events is skipped.
  uint32_t pending_max_frame = 0;
  void note_frame(uint32_t frame) {
    if (frame < pending_max_frame) pending_needs_sort = true;
    else pending_max_frame = frame;
  }
  void apply_now(uint32_t v, uint32_t stage, uint32_t param, double f, int64_t iv, uint32_t frame, std::vector<HostEvent>& out) {
    const StageInfo& S = stages[stage];
    Shadow& sh = shadow[stage];
    // a parameter a signal drives at audio rate ignores ordinary changes while the link stands (audio_rate.rs:70-74)
    if (S.ar_param != 0 && param + 1u == S.ar_param) return;
    note_frame(frame);
    auto set = [&](int rel, uint64_t bits) { out.push_back(HostEvent{v, frame, knh_dev::EV_SET, static_cast<uint32_t>(S.slot_base + rel), bits}); };
    const F sr_as_f32 = static_cast<F>(static_cast<float>(sample_rate));
    switch (S.kind) {
      case KNH_STAGE_SIN_WT:
        if (param == 0) {  // osc.rs:127-130; ignored while an audio-rate buffer drives it (audio_rate.rs:70-74)
          if (S.flags & KNH_STAGE_FLAG_AR_FREQ) return;
          F freq = static_cast<F>(f);
          sh.a[v] = freq;
          set(2, sat_u32(static_cast<double>(freq) * f2pi));
          if (S.wavetable()) set(3, wt_table_word(wt_of(stage, v), freq));  // OscWt::freq keeps self.freq: the table Wavetable::get picks moves with the increment
        } else if (param == 1) {  // osc.rs:133-135
          set(1, sat_u32(f * 65536.0));
        } else {
          set(0, 0);  // reset_phase
        }
        break;
      case KNH_STAGE_SIN_NUMERIC:
        if (param == 0) set(2, to_bits(static_cast<F>(f) / sr_as_f32));  // osc.rs:240-242
        else if (param == 1) set(1, to_bits(static_cast<F>(f)));
        else set(0, to_bits(F(0)));
        break;
      case KNH_STAGE_SVF: {  // svf.rs:81-133: every setter recomputes the coefficients
        if (param == 0) sh.a[v] = static_cast<F>(f);
        else if (param == 1) sh.b[v] = static_cast<F>(f);
        else if (param == 2) sh.c[v] = static_cast<F>(f);
        else if (param == 3) sh.ty[v] = (iv >= 0 && iv <= 8) ? static_cast<uint8_t>(iv) : 0;  // knaster_macros/src/lib.rs:44-47
        F co[6];
        svf_coeffs<F>(sh.ty[v], sh.a[v], sh.b[v], sh.c[v], sr_as_f32, co);
        for (int k = 0; k < 6; ++k) set(2 + k, to_bits(co[k]));
        if (S.n_slots == 12) {  // the values the device-side setter reads (another parameter of this filter is driven at audio rate)
          if (param == 0) set(8, to_bits(sh.a[v]));
          else if (param == 1) set(9, to_bits(sh.b[v]));
          else if (param == 2) set(10, to_bits(sh.c[v]));
          else if (param == 3) set(11, sh.ty[v]);
        }
      } break;
      case KNH_STAGE_ONEPOLE_LPF:
      case KNH_STAGE_ONEPOLE_HPF: {  // onepole.rs:135-139,172-176 -> :35-46
        F fr = static_cast<F>(f) / static_cast<F>(sample_rate);
        F b1 = std::exp(F(-2.0) * Consts<F>::PI * fr);
        set(2, to_bits(b1));
        set(1, to_bits(F(1.0) - b1));
      } break;
      case KNH_STAGE_MUL_ENV_ASR:
      case KNH_STAGE_MUL_ENV_AR:
        if (param == 0 || param == 1) {  // envelopes.rs:85-110 / :236-261 (skip when unchanged)
          std::vector<F>& secs = param == 0 ? sh.a : sh.b;
          F s = static_cast<F>(f);
          if (secs[v] != s) {
            secs[v] = s;
            F rate = s == F(0) ? F(1) : F(1) / (s * static_cast<F>(sample_rate));
            set(param == 0 ? 2 : 3, to_bits(rate));
          }
        } else if (S.kind == KNH_STAGE_MUL_ENV_ASR && param == 2) {  // t_release needs the live state: device op
          out.push_back(HostEvent{v, frame, knh_dev::EV_ENV_ASR_RELEASE, static_cast<uint32_t>(S.slot_base), 0});
        } else {
          set(0, 1);  // t_restart: state = Attacking, t untouched (envelopes.rs:47-49,131-133)
        }
        break;
      case KNH_STAGE_BUFFER_READER: {  // buffer.rs:62-103
        auto set2 = [&](int rel, double d) {
          const uint64_t b = to_bits(d);
          set(rel, static_cast<uint32_t>(b));
          set(rel + 1, static_cast<uint32_t>(b >> 32));
        };
        const double buffer_sr = buf_of(v).sr;  // the voice's own Buffer's: seconds become its frames, its rate scale
        const size_t r = reader_at(S, v);
        switch (param) {
          case 0: buf_rate[r] = f; set2(2, (buffer_sr / static_cast<double>(sample_rate)) * f); break;
          case 1: set(9, iv != 0 ? 1u : 0u); break;
          case 2: buf_start[r] = secs_to_frames(f, buffer_sr); set2(4, buf_start[r]); set2(6, buf_start[r] + buf_dur[r]); break;
          case 3: buf_dur[r] = secs_to_frames(f, buffer_sr); set2(6, buf_start[r] + buf_dur[r]); break;
          case 4: set2(6, secs_to_frames(f, buffer_sr)); break;
          default: set2(0, buf_start[r]); set(8, 0); break;  // t_restart -> reset -> jump_to(start_frame)
        }
      } break;
      case KNH_STAGE_POLYBLEP: {  // polyblep.rs:158-182
        const F srf = static_cast<F>(sample_rate);
        if (param == 0) {
          const F dt = static_cast<F>(f) / srf;
          set(1, to_bits(dt));
          set(4, (dt * srf >= srf / F(4)) ? 1u : 0u);
        } else if (param == 1) {
          set(2, to_bits(static_cast<F>(f)));
        } else {  // Waveform::from(PInteger): out of range -> default (Sawtooth)
          set(3, iv >= 0 && iv < 14 ? static_cast<uint64_t>(iv) : 0u);
        }
      } break;
      case KNH_STAGE_PAN2: {  // Pan2::pan(pan: f32), pan.rs:26-29 (the macro hands the PFloat over `as f32`)
        float gl, gr;
        pan2_gains(static_cast<float>(f), &gl, &gr);
        set(0, to_bits(static_cast<F>(gl)));
        set(1, to_bits(static_cast<F>(gr)));
      } break;
      case KNH_STAGE_RANDOM_LIN: {  // noise.rs:213-221: phase_step = F::new(value) * freq_to_phase_inc
        const F inc = F(1) / static_cast<F>(sample_rate);
        set(5, to_bits(static_cast<F>(static_cast<F>(f) * inc)));
      } break;
      case KNH_STAGE_PHASOR: {  // osc.rs:189-196
        const uint64_t sb = to_bits(f * (1.0 / static_cast<double>(sample_rate)));
        set(2, static_cast<uint32_t>(sb));
        set(3, static_cast<uint32_t>(sb >> 32));
      } break;
      case KNH_STAGE_ALLPASS_FB_DELAY:
        if (param == 1) {  // feedback, :237-240
          set(7, to_bits(static_cast<F>(f)));
          break;
        }
        [[fallthrough]];  // delay_time, :231-236: set_delay_in_frames without the length check of AllpassDelay's
      case KNH_STAGE_ALLPASS_DELAY: {  // delay_time, :136-143 -> set_delay_in_frames, :160-174
        const double delay_frames = f * static_cast<double>(sample_rate);
        const uint32_t len = ring_len(stage, v);
        if (!(delay_frames < static_cast<double>(len))) {  // `(delay_frames as usize) < buffer.len()` fails: ignored
          if (S.kind == KNH_STAGE_ALLPASS_FB_DELAY) warn("AllpassFeedbackDelay: delay_time longer than the ring, change ignored");
          break;
        }
        F num = static_cast<F>(delay_frames);  // F::new; a negative or NaN value casts to 0 frames above, and goes on as it is
        const F fl = std::floor(num);
        uint32_t whole = fl > F(0) ? static_cast<uint32_t>(fl) : 0u;  // to_usize().unwrap() on a negative value panics in the reference
        F delta = num - fl;
        if (num > F(0.5) && delta < F(0.5)) {
          delta += F(1);
          whole -= 1u;
        }
        out.push_back(HostEvent{v, frame, knh_dev::EV_ALLPASS_DELAY, static_cast<uint32_t>(S.slot_base), whole});
        set(4, to_bits((F(1) - delta) / (F(1) + delta)));  // AllpassInterpolator::set_delta, :74-76
      } break;
      case KNH_STAGE_SAMPLE_DELAY: {  // delay.rs:33-36: delay_samples = (seconds * sample_rate) as usize
        const double ds = f * static_cast<double>(sample_rate);
        const uint32_t len = ring_len(stage, v);
        if (!(ds < static_cast<double>(len) + 1.0)) {  // the reference would read outside its buffer
          warn("SampleDelay: delay_time longer than the ring, change ignored");
          break;
        }
        const uint32_t d = ds > 0.0 ? static_cast<uint32_t>(ds) : 0u;  // NaN and negatives -> 0, as `as usize` does
        set(1, len - d);
      } break;
      case KNH_STAGE_MUL_ENVELOPE: {  // envelopes.rs:478-524
        auto set2 = [&](int rel, double d) {
          uint64_t b = to_bits(d);
          set(rel, static_cast<uint32_t>(b));
          set(rel + 1, static_cast<uint32_t>(b >> 32));
        };
        if (param == 0) {  // time_scale = F::new(value).to_f64()
          set2(6, static_cast<double>(static_cast<F>(f)) * (1.0 / static_cast<double>(sample_rate)));
        } else if (param == 1) {  // jump_to_segment (clamped), state = Running { segment, 0.0 }
          uint64_t j = iv < 0 ? 0 : static_cast<uint64_t>(iv);
          if (j >= env_nseg[v]) j = env_nseg[v] - 1;
          set(0, 1);
          set2(2, 0.0);
          set(1, j);
        } else if (param == 2) {  // t_restart
          set(0, 1);
          set2(2, 0.0);
          set2(4, env_start[v]);
          set(1, 0);
        } else {  // t_stop needs the live time: device op
          out.push_back(HostEvent{v, frame, knh_dev::EV_SEGENV_STOP, static_cast<uint32_t>(S.slot_base), 0});
        }
      } break;
      default:  // Constant::value (util.rs:47-50) / WrMul "wr_mul" (wrappers_core/math.rs:92-98)
        set(0, to_bits(static_cast<F>(f)));
        break;
    }
  }

  // The records of one block, in arrival order: set_delay_within_block_for_param arms (precise_timing.rs:146-148),
  // param_apply queues when a delay is armed (:126-135, capacity DELAYED_CHANGES_PER_BLOCK) and applies at once otherwise,
  // and process_block's change loop (:65-114) applies a node's queued changes first in, first out, each at
  // max(its delay, where the node's block has got to) -- a change behind one that is not due inside the processed range
  // is never reached.  A node's events come out in frame order by construction.
  struct DueRec { uint32_t rec; uint32_t due; };
  std::vector<DueRec> due_scratch;
  void resolve_qrecs(std::vector<QRec>& recs, uint32_t frame_begin, uint32_t frame_end) {
    if (recs.empty()) return;
    q_epoch += 1;
    if (q_epoch == 0) {  // wrapped around: no stale state may look current
      std::fill(node_q.begin(), node_q.end(), NodeQ{0u, 0, 0, 0});
      q_epoch = 1;
    }
    pending.reserve(pending.size() + recs.size());
    // Two passes, as the reference's time runs: a call without an armed delay goes straight through to the node when it is
    // made -- between two blocks, so BEFORE every queued change of the block is applied (those are applied inside
    // process_block) -- whatever the order the calls arrived in.  That order matters for setters that compute from what
    // the other parameters are at that moment (SvfFilter's cutoff / q / gain, the envelope times): a cutoff set at once
    // after a q change was queued is computed with the old q, and the q change, when due, with the new cutoff.
    due_scratch.clear();
    for (size_t ri = 0; ri < recs.size(); ++ri) {
      const QRec& r = recs[ri];
      const StageInfo& S = stages[r.stage];
      uint16_t& armed = next_delay[static_cast<size_t>(S.param_base + r.param) * nv + r.voice];
      if (r.arm()) armed = r.delay;
      if (!r.has_value()) continue;
      const double f = r.kind() == KNH_VALUE_FLOAT ? r.v.f : 0.0;
      const int64_t iv = r.kind() == KNH_VALUE_FLOAT ? 0 : r.v.i;
      if (armed == 0) {  // no delay armed: straight through, before the block
        apply_now(r.voice, r.stage, r.param, f, iv, frame_base, pending);
        continue;
      }
      NodeQ& q = node_q[static_cast<size_t>(r.voice) * n_wrapped + static_cast<uint32_t>(wrapped_index[r.stage])];
      if (q.epoch != q_epoch) q = NodeQ{q_epoch, static_cast<uint16_t>(frame_begin), 0, 0};
      if (q.taken >= S.dcpb) {  // precise_timing.rs:129-134: the queue was full when this change arrived
        if (q.taken == S.dcpb) { warn("Not enough space for scheduled changes in WrPreciseTiming, change ignored"); q.taken = static_cast<uint16_t>(std::min<uint32_t>(S.dcpb + 1u, 32767u)); }
        continue;
      }
      q.taken = static_cast<uint16_t>(q.taken + 1);
      if (q.blocked) continue;  // behind a change that is not due in this block: never reached
      const uint32_t due = std::max<uint32_t>(armed, q.at);
      if (due > frame_end) { q.blocked = 1; continue; }
      q.at = static_cast<uint16_t>(due);
      due_scratch.push_back(DueRec{static_cast<uint32_t>(ri), due});
    }
    for (const auto& d : due_scratch) {  // (a node's queued changes: first in, first out, their due frames never decrease)
      const QRec& r = recs[d.rec];
      const StageInfo& S = stages[r.stage];
      const double f = r.kind() == KNH_VALUE_FLOAT ? r.v.f : 0.0;
      const int64_t iv = r.kind() == KNH_VALUE_FLOAT ? 0 : r.v.i;
      const uint32_t due = d.due;
      const size_t first_ev = pending.size();
      apply_now(r.voice, r.stage, r.param, f, iv, frame_base + due, pending);
      if (due > frame_begin) {  // a split point: the node's block restarts here (precise_timing.rs:104-110)
        if (pending.size() == first_ev) {
          note_frame(frame_base + due);
          pending.push_back(HostEvent{r.voice, frame_base + due, knh_dev::EV_NOP, static_cast<uint32_t>(S.slot_base), 0});
        }
        for (size_t e = first_ev; e < pending.size(); ++e) pending[e].op |= knh_dev::EV_SPLIT;
      }
    }
    recs.clear();
  }

  // WrPreciseTiming::process_block's change loop (precise_timing.rs:65-114) for every wrapped node
  // with queued changes: FIFO with head-of-line blocking, changes past the processed range are lost.
  void resolve_queues(uint32_t frame_begin, uint32_t frame_end) {  // block-relative range; events get frame_base added
    smooth_epoch = (smooth_epoch + 1) & 0x7FFFFFFFu;
    if (!queued.empty()) {
      // group by node, keeping arrival order inside each node's queue
      // (callers that walk the voices in order, as the batched entry points are normally used, arrive sorted)
      auto by_node = [](const auto& a, const auto& b) { return a.first < b.first; };
      if (!std::is_sorted(queued.begin(), queued.end(), by_node)) std::stable_sort(queued.begin(), queued.end(), by_node);
      size_t i = 0;
      std::vector<std::pair<uint32_t, const QueuedChange*>> due_list;
      while (i < queued.size()) {
        const uint64_t key = queued[i].first;
        const uint32_t voice = static_cast<uint32_t>(key / stages.size());
        const uint32_t stage = static_cast<uint32_t>(key % stages.size());
        const uint32_t cap = stages[stage].dcpb;
        const bool smoothed = (stages[stage].flags & KNH_STAGE_FLAG_SMOOTH_PARAMS) != 0;
        uint32_t at = frame_begin, taken = 0;
        bool blocked = false;
        due_list.clear();
        for (; i < queued.size() && queued[i].first == key; ++i) {
          if (taken >= cap) {  // precise_timing.rs:129-134: the queue was full when this change arrived
            if (taken == cap) warn("Not enough space for scheduled changes in WrPreciseTiming, change ignored");
            ++taken;
            continue;
          }
          ++taken;
          if (blocked) continue;  // behind a change that is not due in this block: never reached
          const QueuedChange& c = queued[i].second;
          uint32_t due = std::max<uint32_t>(c.delay, at);
          if (due > frame_end) { blocked = true; continue; }
          at = due;
          due_list.emplace_back(due, &c);
        }
        // WrPreciseTiming::process_block (precise_timing.rs:65-114): apply what is due, run the inner
        // (partial) block from there, repeat.  An inner WrSmoothParams steps its ramps at the start of
        // every one of those partial blocks.
        size_t k = 0;
        uint32_t seg = frame_begin;
        bool first = true;
        while (true) {
          const size_t first_ev = pending.size();
          while (k < due_list.size() && due_list[k].first <= seg) {
            const QueuedChange& c = *due_list[k].second;
            deliver(voice, stage, c.param, c.kind, c.f, c.i, frame_base + seg);
            ++k;
          }
          if (seg < frame_end && smoothed) smooth_tick(voice, stage, seg);
          if (!first) {  // a split point: the node's block restarts here (precise_timing.rs:104-110)
            if (pending.size() == first_ev)
              pending.push_back(HostEvent{voice, frame_base + seg, knh_dev::EV_NOP, static_cast<uint32_t>(stages[stage].slot_base), 0});
            for (size_t e = first_ev; e < pending.size(); ++e) pending[e].op |= knh_dev::EV_SPLIT;
            pending_needs_sort = true;
          }
          if (k >= due_list.size()) break;
          seg = due_list[k].first;
          first = false;
        }
      }
      queued.clear();
    }
    // nodes with a ramp in flight that were not stepped above: one step at the start of the block
    if (!smooth_active.empty()) {
      size_t w = 0;
      for (size_t r = 0; r < smooth_active.size(); ++r) {
        const uint64_t key = smooth_active[r];
        const uint32_t voice = static_cast<uint32_t>(key / stages.size());
        const uint32_t stage = static_cast<uint32_t>(key % stages.size());
        if ((smooth_mark[stage][voice] >> 1) != smooth_epoch) smooth_tick(voice, stage, frame_begin);
        bool alive = false;
        const SmoothState* st = &smooth[stage][static_cast<size_t>(voice) * stages[stage].n_params];
        for (int p = 0; p < stages[stage].n_params; ++p) alive = alive || (st[p].linear && !st[p].done);
        if (alive) smooth_active[w++] = key;
        else smooth_mark[stage][voice] &= ~1u;
      }
      smooth_active.resize(w);
      pending_needs_sort = true;
    }
  }

  // ---- processing ---------------------------------------------------------------------------
  // Events addressed past the blocks of this launch (a call for block k of a later launch, turned into patches at once):
  // they stay in `pending`, k launches' worth of blocks earlier, for the next launch.
  std::vector<HostEvent> later;
  // allow_ranges: the call goes to a resident launch of a pipelined kernel (up to 15 range events ride with its command);
  // launch_ranges: to an ordinary launch of one, which takes up to LAUNCH_RANGES_MAX in its kernel arguments (launch_n_ranges,
  // launch_range_recs) -- nothing is written to the pinned lists then, and no workgroup reads host memory for its events.
  int upload_events(hipStream_t s, bool* have_events, uint32_t n_blocks, bool allow_ranges = false, bool launch_ranges = false) {
    *have_events = false;
    later.clear();
    res_n_ranges = 0;
    launch_n_ranges = 0;
    const uint64_t horizon = static_cast<uint64_t>(n_blocks) * block_size;
    if (!pending_ranges.empty()) {
      bool as_ranges = (allow_ranges || launch_ranges) && pending.empty() && pending_ranges.size() <= (allow_ranges ? 15u : static_cast<size_t>(knh_dev::LAUNCH_RANGES_MAX));
      for (const RangeEvent& r : pending_ranges) as_ranges = as_ranges && r.frame < horizon;
      if (!as_ranges) expand_ranges();
    }
    if (!allow_ranges && launch_ranges && !pending_ranges.empty()) {  // (pending is empty: see above)
      // Every voice walks the records in order and applies those due: in frame order, then, calls for one frame in the order
      // they arrived -- the order the per-voice lists are sorted into below.
      std::stable_sort(pending_ranges.begin(), pending_ranges.end(), [](const RangeEvent& x, const RangeEvent& y) { return x.frame < y.frame; });
      for (size_t j = 0; j < pending_ranges.size(); ++j) {
        const RangeEvent& r = pending_ranges[j];
        launch_range_recs[2 * j] = Event{r.frame, (r.slot & 0xFFFFFFu) | (r.op << 24), r.bits};
        launch_range_recs[2 * j + 1] = Event{r.v0, r.v1, 0ull};
      }
      launch_n_ranges = static_cast<uint32_t>(pending_ranges.size());
      pending_ranges.clear();
      pending_needs_sort = false;
      pending_max_frame = 0;
      *have_events = true;
      return KNH_OK;
    }
    if (pending_max_frame >= horizon && !pending.empty()) {
      size_t w = 0;
      for (const HostEvent& e : pending) {
        if (e.frame >= horizon) { later.push_back(e); later.back().frame -= static_cast<uint32_t>(horizon); }
        else pending[w++] = e;
      }
      pending.resize(w);
    }
    // A resident call's per-voice events that are the same few changes for a run of neighbouring voices -- a bank's note-on
    // sent as one param_apply per voice, "this cutoff for all of them" -- are range events too: 32 bytes per change instead of
    // 16 per voice and change fetched over PCIe (a bank's 16 384 single triggers: 14 us of the call).
    if (allow_ranges && pending_ranges.empty() && pending.size() >= 32 && later.empty() && !pending_needs_sort) {
      const uint32_t v_first = pending[0].voice;
      size_t k = 1;
      while (k < pending.size() && pending[k].voice == v_first) ++k;  // the first voice's events
      bool same = k <= 15 && pending.size() % k == 0;
      const size_t n_v = same ? pending.size() / k : 0;
      same = same && v_first + n_v <= nv;
      for (size_t i = k; same && i < pending.size(); ++i) {
        const HostEvent& e = pending[i];
        const HostEvent& f = pending[i % k];
        same = e.voice == v_first + i / k && e.frame == f.frame && e.op == f.op && e.slot == f.slot && e.bits == f.bits;
      }
      if (same) {
        for (size_t j = 0; j < k; ++j) {
          const HostEvent& f = pending[j];
          pending_ranges.push_back(RangeEvent{v_first, v_first + static_cast<uint32_t>(n_v), f.frame, f.op, f.slot, f.bits, 0});
        }
        pending.clear();
      }
    }
    const size_t total = pending.empty() ? 2 * pending_ranges.size() : pending.size();
    auto finish = [&] {
      pending.clear();
      pending_needs_sort = false;
      pending_max_frame = 0;
      if (!later.empty()) {
        pending.swap(later);
        pending_needs_sort = true;  // conservatively: their order among what arrives next is not tracked
        for (const HostEvent& e : pending) pending_max_frame = std::max(pending_max_frame, e.frame);
      }
    };
    if (total == 0) { finish(); return KNH_OK; }
    const unsigned lb = list_parity;
    list_parity ^= 1u;
    if (list_busy[lb]) {  // the kernel that read this buffer two launches ago must be done with it
      KNH_HIP(hipEventSynchronize(list_done[lb]));
      list_busy[lb] = false;
    }
    if (total > h_events_cap2[lb]) {
      { int rl = resident.leave(); if (rl != KNH_OK) return rl; }  // (a resident kernel knows the list by its address)
      size_t cap = std::max<size_t>(total, 1024) * 2;
      if (h_events2[lb]) KNH_HIP(hipHostFree(h_events2[lb]));
      h_events2[lb] = nullptr;
      KNH_HIP(hipHostMalloc(&h_events2[lb], cap * sizeof(Event)));
      h_events_cap2[lb] = cap;
    }
    h_ev_start = h_ev_start2[lb];
    h_events = h_events2[lb];
    list_in_use = static_cast<int>(lb);
    if (!pending_ranges.empty()) {  // (pending is empty: see above) the call's events as range events, two records each
      for (size_t j = 0; j < pending_ranges.size(); ++j) {
        const RangeEvent& r = pending_ranges[j];
        Event& d = h_events[2 * j];
        d.frame = r.frame;
        d.slot_op = (r.slot & 0xFFFFFFu) | (r.op << 24);
        d.bits = r.bits;
        Event& w = h_events[2 * j + 1];
        w.frame = r.v0;
        w.slot_op = r.v1;
        w.bits = 0;
      }
      res_n_ranges = static_cast<uint32_t>(pending_ranges.size());
      sent_ranges.swap(pending_ranges);
      pending_ranges.clear();
      finish();
      *have_events = true;
      return KNH_OK;
    }
    uint32_t* start = h_ev_start;  // nv + 2 words
    // Already in voice order (a batch of triggers for voices 0 .. N - 1, the common big list): one pass, no sort.
    bool in_voice_order = true;
    {
      uint32_t prev = 0;
      for (const HostEvent& e : pending) { if (e.voice < prev) { in_voice_order = false; break; } prev = e.voice; }
    }
    if (in_voice_order) {
      uint32_t v_next = 0, i = 0;
      for (const HostEvent& e : pending) {
        while (v_next <= e.voice) start[v_next++] = i;
        Event& d = h_events[i++];
        d.frame = e.frame;
        d.slot_op = (e.slot & 0xFFFFFFu) | (e.op << 24);
        d.bits = e.bits;
      }
      while (v_next <= nv) start[v_next++] = i;
    } else {
    // counting sort by voice (stable: keeps application order): counts two places up, so that after the prefix sum
    // start[v + 1] is where voice v's events begin, and after the scatter (which advances it) where voice v + 1's do
    std::fill(start, start + nv + 2, 0u);
    for (const HostEvent& e : pending) start[e.voice + 2]++;
    for (uint32_t v = 0; v < nv; ++v) start[v + 2] += start[v + 1];
    for (const HostEvent& e : pending) {
      Event& d = h_events[start[e.voice + 1]++];
      d.frame = e.frame;
      d.slot_op = (e.slot & 0xFFFFFFu) | (e.op << 24);
      d.bits = e.bits;
    }
    }
    if (pending_needs_sort) {  // then each voice's few events by frame (stable)
      for (uint32_t v = 0; v < nv; ++v) {
        Event* b = h_events + h_ev_start[v];
        Event* e = h_events + h_ev_start[v + 1];
        auto by_frame = [](const Event& x, const Event& y) { return x.frame < y.frame; };
        if (e - b > 1 && !std::is_sorted(b, e, by_frame)) std::stable_sort(b, e, by_frame);
      }
    }
    (void)s;
    finish();
    *have_events = true;
    return KNH_OK;
  }

  int process(uint32_t n_blocks, size_t ftp, size_t offset, uint64_t /*clock*/, void* out_host, void* out_device, void* voices_host,
              uint32_t* out_flags, void* stream, bool sync, bool accumulate) override {
    if (accumulate && !out_device) return fail(KNH_ERR_INVALID_ARGUMENT, "accumulation needs a device output buffer");
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    if (offset + ftp > block_size) return fail(KNH_ERR_INVALID_ARGUMENT, "block_start_offset + frames_to_process exceeds block_size");
    if (n_blocks == 0 || n_blocks > 4096) return fail(KNH_ERR_INVALID_ARGUMENT, "n_blocks must be in 1..4096");
    if (n_blocks > 1 && (offset != 0 || ftp != block_size)) return fail(KNH_ERR_INVALID_ARGUMENT, "multi-block launches process whole blocks");
    if (n_blocks > 1 && voices_host) return fail(KNH_ERR_INVALID_ARGUMENT, "per-voice output is only available for single blocks");
    KNH_HIP(hipSetDevice(device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : own_stream;
    if (resolver.take_overflow()) warn("Not enough space for scheduled changes in WrPreciseTiming, change ignored");
    const uint32_t fb = static_cast<uint32_t>(offset), fe = static_cast<uint32_t>(offset + ftp);
    const bool restart_flushed = !rs_voices.empty();  // (the restart kernel goes to `s`: a voice kernel on the bank's stream waits for it)
    { int rr = flush_restart(s); if (rr != KNH_OK) return rr; }  // voices restarted since the last launch: their new state first
    mid_block = fe < block_size;
    // Assemble the launch's state patches block by block, in the order the reference would apply them.
    for (uint32_t b = 0; b < n_blocks; ++b) {
      frame_base = b * static_cast<uint32_t>(block_size);
      if (b > 0 && b < future.size()) {
        for (const Call& c : future[b]) {
          if (c.is_delay) set_delay(c.voice, c.stage, c.param, c.delay);
          else param_apply(c.voice, c.stage, c.param, c.kind, c.f, c.i);
        }
      }
      if (b < qfuture.size()) resolve_qrecs(qfuture[b], fb, fe);
      resolve_queues(fb, fe);
    }
    frame_base = 0;
    if (!qfuture.empty()) {  // records addressed beyond this launch move up (their vectors keep their capacity)
      if (qfuture.size() <= n_blocks) {
        for (auto& q : qfuture) q.clear();
      } else {
        std::rotate(qfuture.begin(), qfuture.begin() + n_blocks, qfuture.end());
        for (size_t k = qfuture.size() - n_blocks; k < qfuture.size(); ++k) qfuture[k].clear();
      }
    }
    // (whether this call goes to a resident launch -- below -- decides what its events may look like)
    const bool res_now = sync && out_host && !out_device && !voices_host && !stream && n_blocks == 1 && fe > fb && !accumulate && !timing &&
                         !resolver.pending() && res_possible() && resident.enabled() && resident.ready();
    bool have_events = false;
    // (the device's resolver merges the host's per-voice lists into its own: lists it is, then)
    const bool ranges_now = !res_now && range_launches && form.facts.walks_ranges && !resolver.pending();
    int rc = upload_events(s, &have_events, n_blocks, res_now && form.facts.walks_ranges, ranges_now);
    if (rc != KNH_OK) return rc;
    if (!future.empty()) {  // calls addressed beyond this launch move up; those now due for the next
                            // block are applied right away, ahead of anything that arrives later
      if (future.size() <= n_blocks) future.clear();
      else future.erase(future.begin(), future.begin() + n_blocks);
      if (!future.empty()) {
        std::vector<Call> due;
        due.swap(future[0]);
        for (const Call& c : due) {
          if (c.is_delay) set_delay(c.voice, c.stage, c.param, c.delay);
          else param_apply(c.voice, c.stage, c.param, c.kind, c.f, c.i);
        }
      }
    }
    // The call the reference makes -- one whole or partial block into host memory, blocking -- on a resident launch where the
    // bank's kernel form has one (res_possible); anything else first asks a resident kernel (this bank's, or another bank's
    // on this device) to leave: it would be in the way of the launch, and it holds the voices' state in its registers.
    {
      if (res_now) {
        const int held_list = list_in_use, call_list = have_events ? list_in_use : -1;
        if (call_list >= 0) { list_busy[call_list] = false; list_in_use = -1; }  // (no stream order to keep: the call is over when it returns)
        rc = resident.call(fb, fe, call_list, res_n_ranges, out_host, out_flags);
        if (rc != KNH_ERR_UNSUPPORTED_CHAIN) return rc;
        list_in_use = held_list;  // the kernels would not run side by side: this call, and the bank from now on, takes the launch per call
        if (res_n_ranges) {  // the launch per call reads per-voice lists: the call's range events once more, spelled out
          pending_ranges.swap(sent_ranges);
          for (RangeEvent& r : pending_ranges) r.at = 0;
          rc = upload_events(s, &have_events, n_blocks, false);
          if (rc != KNH_OK) return rc;
        }
      }
      resident.sat_out();
      rc = resident.leave();
      if (rc != KNH_OK) return rc;
      ResidentCall<F>::make_room(device, this);
    }
    const bool want_voices = voices_host != nullptr || (desc.mix_mode == KNH_MIX_LEFT_FOLD) || stage_out != nullptr;
    if (desc.mix_mode == KNH_MIX_LEFT_FOLD && n_blocks > 1)
      return fail(KNH_ERR_INVALID_ARGUMENT, "KNH_MIX_LEFT_FOLD processes one block per call");
    if (stage_out && n_blocks > 1) return fail(KNH_ERR_INTERNAL, "a bank that feeds a following stage renders one block per launch");
    if (want_voices && !stage_out) KNH_HIP(ensure_voices());
    const bool rows_per_voice = form.facts.rows_per_voice;  // (a lane per frame: the rows are the voices' signals)
    const unsigned n_waves = rows_per_voice ? nv : (nv + 63) / 64;
    // This launch's fold beside the next launch's voice kernel: an ordinary launch of a pipelined kernel whose tree mix stays on
    // the device and whose caller does not wait for it; up to 256 rows (the LDS-free fold's reach).  Where it was measured not
    // to pay it is not done (profiles/r15_fold_overlap.json, legs_first_cut_overlap_in_every_form): the whole-chain forms (a one-voice bank: -0.3 % kernel-only), and
    // the launches of knh_bank_process_blocks_begin, which has two launches in flight on a stream of its own and a copy to the
    // host behind each (-23 %).
    const bool overlap_now = fold_overlap && !sync && out_device && !voices_host && !stage_out && desc.mix_mode == KNH_MIX_TREE &&
                             form.facts.walks_ranges && !rows_per_voice && n_waves <= 256u && fe > fb && !host_pipe_streams().has(s);
    if (n_blocks > partials_blocks) {
      KNH_HIP(hipStreamSynchronize(s));
      if (voice_stream) KNH_HIP(hipStreamSynchronize(voice_stream));  // (what reads or writes either set of rows is idle)
      if (fold_stream) KNH_HIP(hipStreamSynchronize(fold_stream));
      const size_t bytes = static_cast<size_t>(n_blocks) * fold_planes * n_waves * block_size * sizeof(F);
      KNH_HIP(hipFree(d_partials));
      d_partials = nullptr;
      KNH_HIP(hipMalloc(&d_partials, bytes));
      if (d_partials2) {
        KNH_HIP(hipFree(d_partials2));
        d_partials2 = nullptr;
        KNH_HIP(hipMalloc(&d_partials2, bytes));
      }
      partials_blocks = n_blocks;
    }
    if (overlap_now) { int r2 = ensure_overlap_streams(n_waves); if (r2 != KNH_OK) return r2; }
    if (!out_device && n_blocks > out_blocks) {
      KNH_HIP(hipStreamSynchronize(s));
      KNH_HIP(hipFree(d_out));
      d_out = nullptr;
      KNH_HIP(hipMalloc(&d_out, static_cast<size_t>(n_blocks) * desc.out_channels * block_size * sizeof(F)));
      KNH_HIP(hipMemsetAsync(d_out, 0, static_cast<size_t>(n_blocks) * desc.out_channels * block_size * sizeof(F), s));
      if (h_out) KNH_HIP(hipHostFree(h_out));
      h_out = nullptr;
      KNH_HIP(hipHostMalloc(&h_out, static_cast<size_t>(n_blocks) * desc.out_channels * block_size * sizeof(F) + 2 * sizeof(uint32_t),
                            hipHostMallocMapped | hipHostMallocCoherent));
      out_blocks = n_blocks;
    }

    if (flags_stream_set && flags_stream != s) KNH_HIP(hipStreamSynchronize(flags_stream));  // that set was cleared in the other stream's order
    flags_stream = s;
    flags_stream_set = true;
    // (the fold of this launch clears the set of the launch after the next: the next launch's kernel may be running beside it)
    uint32_t* const flags_now = d_flags + 16 * flags_turn;
    uint32_t* const flags_next = d_flags + 16 * ((flags_turn + 2u) % 3u);
    flags_turn = (flags_turn + 1u) % 3u;
    flags_last = flags_now;
    VoiceKernelArgs<F> a;
    fill_launch_args(a, n_blocks, fb, fe);
    if (uses_input) {
      if (in_blocks_set != n_blocks) return fail(KNH_ERR_INVALID_ARGUMENT, "a bank with KNH_STAGE_INPUT stages needs knh_bank_set_input for exactly the blocks of this call");
      if (in_device) {
        a.input = in_device;
      } else {
        if (in_host_pending) {
          KNH_HIP(hipMemcpyAsync(d_input, h_input, static_cast<size_t>(n_blocks) * desc.in_channels * block_size * sizeof(F), hipMemcpyHostToDevice, s));
          if (!in_copied) KNH_HIP(hipEventCreateWithFlags(&in_copied, hipEventDisableTiming));
          KNH_HIP(hipEventRecord(in_copied, s));
          in_copy_pending = true;
        }
        in_host_pending = false;
        a.input = d_input;
      }
      in_blocks_set = 0;  // one set_input per process call
    }
    // The stream the voice kernel goes to.  An overlapped launch's kernel runs on the bank's voice stream, behind the kernel of
    // the launch before and beside that launch's fold.  It waits for the caller's stream only where that stream carries
    // something the kernel reads -- the bank's input, a restart of voices, a launch that kept to the caller's stream: the
    // caller's stream itself waits for every fold (below), so a kernel that always waited for it would start after the fold
    // it is meant to run beside.  What else the caller enqueued before this call -- readers of the output buffer, an earlier
    // reduce of it -- is ordered in front of the fold, which is what writes that buffer.
    hipStream_t vs = s;
    const uint32_t row_set = overlap_now ? overlap_turn : 0u;
    if (overlap_now) {
      overlap_turn ^= 1u;
      vs = voice_stream;
      a.partials = row_set ? d_partials2 : d_partials;
      KNH_HIP(hipEventRecord(caller_at, s));
      if (!last_overlapped || uses_input || restart_flushed) KNH_HIP(hipStreamWaitEvent(vs, caller_at, 0));
      // The rows this kernel writes were read by the fold of the launch before the last, and that fold cleared this launch's
      // flag set.  The HOST waits for that fold, not the voice stream: a wait for another queue's event is a packet between two
      // voice kernels that costs the chip ~15 us of every launch (profiles/r15_fold_overlap.json), while the fold in question
      // ran beside the kernel before this one -- the call returns at once unless the caller is two launches ahead of the device,
      // and then the device still has a launch queued behind the one it is running.
      if (fold_busy[row_set]) KNH_HIP(hipEventSynchronize(fold_done[row_set]));
    }
    a.ev_start = have_events && !launch_n_ranges ? h_ev_start : nullptr;  // pinned host memory, device-visible
    a.events = h_events;
    if (launch_n_ranges) {  // the launch's events are range events: they travel in the kernel arguments
      a.n_ranges = launch_n_ranges;
      std::copy(launch_range_recs, launch_range_recs + 2 * launch_n_ranges, a.ranges);
      ev_range_launches += 1;
    } else if (have_events) {
      ev_list_launches += 1;
      ev_list_bytes += static_cast<uint64_t>(h_ev_start[nv]) * sizeof(Event) + (static_cast<uint64_t>(nv) + 1u) * sizeof(uint32_t);
    }
    if (resolver.pending()) {  // calls to nodes whose queues the device resolves: the lists are made there, the host's merged in
      DevEventResolver::Lists lists{};
      int r2 = resolver.resolve(vs, n_blocks, fb, fe, have_events ? h_ev_start : nullptr, h_events, have_events ? h_ev_start[nv] : 0u, &lists);
      if (r2 != KNH_OK) return r2;
      a.ev_start = lists.ev_start;
      a.events = lists.events;
      if (!have_events) ev_list_launches += 1;  // (lists the device made: a per-voice list launch all the same)
    }
    a.voices_out = want_voices ? (stage_out ? stage_out : d_voices) : nullptr;
    a.flags = flags_now;
    std::pair<hipEvent_t, hipEvent_t>* tp = nullptr;
    if (timing) {
      if (timing_used == timing_pool.size()) {
        if (timing_pool.size() >= 8192) {
          int r = timing_collect();
          if (r != KNH_OK) return r;
        } else {
          hipEvent_t e0, e1;
          KNH_HIP(hipEventCreate(&e0));
          KNH_HIP(hipEventCreate(&e1));
          timing_pool.emplace_back(e0, e1);
        }
      }
      tp = &timing_pool[timing_used++];
    }
    // An overlapped launch of a pre-built kernel carries its events in the dispatch itself (knh::LaunchEvents): the timing
    // pair, or else the event its fold waits for.  Everywhere else they are recorded around the kernel.
    const bool carried = overlap_now && !form.jit;
    if (tp && !carried) KNH_HIP(hipEventRecord(tp->first, vs));
    if (carried) knh::launch_events() = tp ? knh::LaunchEvents{tp->first, tp->second} : knh::LaunchEvents{nullptr, voice_done[row_set]};
    const hipError_t launched = rows_per_voice ? launch_frames(a, vs) : launch_voice(a, n_waves, vs);
    // (a launcher that takes the events clears them: one that left them would have launched a kernel whose fold waits for an
    // event nobody records -- no wait at all)
    const bool events_left = knh::launch_events().start || knh::launch_events().stop;
    knh::launch_events() = knh::LaunchEvents{};
    KNH_HIP(launched);
    if (carried && events_left) {
      (void)hipStreamSynchronize(vs);
      return fail(KNH_ERR_INTERNAL, "the launcher of this kernel form did not take the launch's events (knh::launch_voice_kernel)");
    }
    if (tp && !carried) KNH_HIP(hipEventRecord(tp->second, vs));
    // (the interpreter's rows are the voices' signals; one plane: a voice with two connected outputs never runs there, init)
    if (stage_out && rows_per_voice)
      KNH_HIP(hipMemcpyAsync(stage_out, d_partials, static_cast<size_t>(nv) * block_size * sizeof(F), hipMemcpyDeviceToDevice, s));
    { int r2 = resolver.kernel_enqueued(vs); if (r2 != KNH_OK) return r2; }
    if (have_events && list_in_use >= 0) {
      KNH_HIP(hipEventRecord(list_done[list_in_use], vs));
      list_busy[list_in_use] = true;
      list_in_use = -1;
    }

    // A blocking call for host memory: the fold kernel writes into the pinned block itself and tells the host when it is through
    const bool hand_over = sync && out_host && !out_device && !voices_host && fe > fb;
    F* dst = out_device ? static_cast<F*>(out_device) : (hand_over ? h_out : d_out);
    knh_dev::HostDone hd{nullptr, nullptr, nullptr, 0u};
    if (hand_over) {
      done_epoch += 1;
      if (done_epoch == 0) done_epoch = 1;
      hd = knh_dev::HostDone{h_done, d_fold_count, flags_now, done_epoch};
    }
    // A Pan2 chain's row sets are [block][channel][rows][frame] and its output [block][channel][frame]: the fold sees
    // twice as many "blocks" of one channel each.
    const unsigned fold_channels = pan ? 1u : desc.out_channels;
    // (the interpreter's rows ARE the voices' signals: one buffer serves both mix orders and the per-voice debug output)
    if (overlap_now) {
      // The fold on the bank's fold stream: behind this launch's voice kernel, and behind what the caller's stream held when
      // the call began (readers of `dst`).  The caller's stream waits for it: whatever the caller enqueues after this call sees
      // the mixed blocks and the flags, as it does behind a launch that kept to that stream.
      if (!carried) KNH_HIP(hipEventRecord(voice_done[row_set], vs));
      KNH_HIP(hipStreamWaitEvent(fold_stream, carried && tp ? tp->second : voice_done[row_set], 0));
      KNH_HIP(hipStreamWaitEvent(fold_stream, caller_at, 0));
      KNH_HIP(launch_fold_wave(a.partials, n_waves, static_cast<unsigned>(block_size), fb, fe, dst, fold_channels, static_cast<unsigned>(block_size), n_blocks * fold_planes, accumulate, flags_next, fold_stream));
      KNH_HIP(hipEventRecord(fold_done[row_set], fold_stream));
      fold_busy[row_set] = true;
      KNH_HIP(hipStreamWaitEvent(s, fold_done[row_set], 0));
      last_overlapped = true;
      overlapped_launches += 1;
      wave_folds += 1;
      return KNH_OK;
    }
    last_overlapped = false;
    if (desc.mix_mode == KNH_MIX_LEFT_FOLD)
      KNH_HIP(launch_fold(false, rows_per_voice ? d_partials : d_voices, nv, static_cast<unsigned>(block_size), fb, fe, dst, fold_channels, static_cast<unsigned>(block_size), fold_planes, accumulate, flags_next, s, hand_over ? &hd : nullptr));
    else if (fold_wave_always && !hand_over && n_waves <= 256u && fe > fb) {
      KNH_HIP(launch_fold_wave(d_partials, n_waves, static_cast<unsigned>(block_size), fb, fe, dst, fold_channels, static_cast<unsigned>(block_size), n_blocks * fold_planes, accumulate, flags_next, s));
      wave_folds += 1;
    } else
      KNH_HIP(launch_fold(true, d_partials, n_waves, static_cast<unsigned>(block_size), fb, fe, dst, fold_channels, static_cast<unsigned>(block_size), n_blocks * fold_planes, accumulate, flags_next, s, hand_over ? &hd : nullptr));

    if (!sync) return KNH_OK;
    const size_t blk_elems = desc.out_channels * block_size;
    const size_t out_bytes = static_cast<size_t>(n_blocks) * blk_elems * sizeof(F);
    uint32_t* h_flags = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(h_out) + static_cast<size_t>(out_blocks) * blk_elems * sizeof(F));
    if (hand_over) {
      // Poll the epoch word (the kernel's last store, a system-scope release).  A stream that has finished without the
      // word having moved means the kernel failed: hipStreamQuery says how; it is asked rarely (it is a driver call).
      volatile uint32_t* ep = h_done;
      for (uint64_t spin = 1;; ++spin) {
        if (__atomic_load_n(ep, __ATOMIC_ACQUIRE) == done_epoch) break;
        if ((spin & 0x3FFFu) == 0) {
          const hipError_t q = hipStreamQuery(s);
          if (q == hipSuccess) {
            if (__atomic_load_n(ep, __ATOMIC_ACQUIRE) == done_epoch) break;
            KNH_HIP(hipStreamSynchronize(s));
            if (__atomic_load_n(ep, __ATOMIC_ACQUIRE) != done_epoch) return fail(KNH_ERR_DEVICE, "the fold kernel finished without handing its block over");
            break;
          }
          if (q != hipErrorNotReady) return fail(KNH_ERR_DEVICE, std::string("hipStreamQuery: ") + hipGetErrorString(q));
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
      h_flags[0] = h_done[1];
      h_flags[1] = h_done[2];
    } else {
      if (out_host) KNH_HIP(hipMemcpyAsync(h_out, dst, out_bytes, hipMemcpyDeviceToHost, s));
      KNH_HIP(hipMemcpyAsync(h_flags, flags_now, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      if (voices_host)
        KNH_HIP(hipMemcpyAsync(voices_host, rows_per_voice ? d_partials : d_voices, static_cast<size_t>(fold_planes) * nv * block_size * sizeof(F), hipMemcpyDeviceToHost, s));
      KNH_HIP(hipStreamSynchronize(s));
    }
    if (out_host) {
      if (n_blocks > 1) {
        std::memcpy(out_host, h_out, out_bytes);
      } else {
        for (uint32_t c = 0; c < desc.out_channels; ++c)
          std::memcpy(static_cast<F*>(out_host) + c * block_size + offset, h_out + c * block_size + offset, ftp * sizeof(F));
      }
    }
    if (out_flags) *out_flags = done_flags(h_flags[0], h_flags[1], can_finish);
    return KNH_OK;
  }
  uint32_t partials_blocks = 1, out_blocks = 1;
  // a lane per frame: the kernel built at init, or the interpreter
  hipError_t launch_frames(const VoiceKernelArgs<F>& a, hipStream_t s) {
    F* const rows = d_partials;
    if (form.jit) {
      struct { VoiceKernelArgs<F> a; F* rows; const uint32_t* sin_slots; uint32_t n_sin; } args{a, rows, d_sin_slots, n_sin};
      return knh::jit_frame_launch(form.jit, &args, sizeof(args), (a.n_voices + frame_vpw - 1u) / frame_vpw, s);
    }
    const unsigned n_ops = static_cast<unsigned>(h_prog.size()), n_words = static_cast<unsigned>(n_slots);
    if constexpr (sizeof(F) == 4) return knh::launch_interp_f32(a, d_prog, n_ops, n_words, interp_sigs, interp_out, rows, s);
    else return knh::launch_interp_f64(a, d_prog, n_ops, n_words, interp_sigs, interp_out, rows, s);
  }
  hipError_t launch_voice(const VoiceKernelArgs<F>& a, unsigned n_waves, hipStream_t s) {
    return form.jit ? knh::jit_launch(form.jit, &a, sizeof(a), n_waves, s) : form.fn(a, n_waves, s);
  }
  // a pre-built kernel's launch function for the bank's sample type and allow_fma
  knh::VoiceLaunchFn<F> launch_fn(const knh::VoiceLaunchFn<float> (&f32)[2], const knh::VoiceLaunchFn<double> (&f64)[2]) const {
    if constexpr (sizeof(F) == 4) return f32[desc.allow_fma ? 1 : 0];
    else return f64[desc.allow_fma ? 1 : 0];
  }
  static hipError_t launch_fold(bool tree, const float* rows, unsigned n, unsigned len, unsigned fb, unsigned fe, float* out, unsigned ch, unsigned os, unsigned nb, bool acc, uint32_t* zf, hipStream_t s, const knh_dev::HostDone* hd) {
    return knh::launch_fold_f32(tree, rows, n, len, fb, fe, out, ch, os, nb, acc, zf, s, hd);
  }
  static hipError_t launch_fold(bool tree, const double* rows, unsigned n, unsigned len, unsigned fb, unsigned fe, double* out, unsigned ch, unsigned os, unsigned nb, bool acc, uint32_t* zf, hipStream_t s, const knh_dev::HostDone* hd) {
    return knh::launch_fold_f64(tree, rows, n, len, fb, fe, out, ch, os, nb, acc, zf, s, hd);
  }
  static hipError_t launch_fold_wave(const float* rows, unsigned n, unsigned len, unsigned fb, unsigned fe, float* out, unsigned ch, unsigned os, unsigned nb, bool acc, uint32_t* zf, hipStream_t s) {
    return knh::launch_fold_wave_f32(rows, n, len, fb, fe, out, ch, os, nb, acc, zf, s);
  }
  static hipError_t launch_fold_wave(const double* rows, unsigned n, unsigned len, unsigned fb, unsigned fe, double* out, unsigned ch, unsigned os, unsigned nb, bool acc, uint32_t* zf, hipStream_t s) {
    return knh::launch_fold_wave_f64(rows, n, len, fb, fe, out, ch, os, nb, acc, zf, s);
  }

  int read_done_frames(uint32_t* out) override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    if (!out) return fail(KNH_ERR_INVALID_ARGUMENT, "null output");
    { int rl = resident.leave(); if (rl != KNH_OK) return rl; }  // (a resident kernel's stores reach the copy engine when it ends)
    KNH_HIP(hipSetDevice(device));
    { int rr = flush_restart(own_stream); if (rr != KNH_OK) return rr; }  // (restarted voices have no done frame)
    KNH_HIP(hipStreamSynchronize(own_stream));
    KNH_HIP(hipMemcpy(out, d_done, static_cast<size_t>(nv) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return KNH_OK;
  }
  int debug_read(uint32_t* out16) override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    { int rl = resident.leave(); if (rl != KNH_OK) return rl; }
    KNH_HIP(hipSetDevice(device));
    KNH_HIP(hipDeviceSynchronize());
    KNH_HIP(hipMemcpy(out16, flags_last ? flags_last : d_flags, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    // word 2 (no kernel writes it): the kernel form the bank's launches take
    out16[2] = form.is.kind;
    // word 3 (no kernel writes it): the voices per workgroup of a whole-block launch in the lane-per-frame forms, 0 in every other
    out16[3] = !form.facts.rows_per_voice ? 0u
             : form.jit ? frame_vpw
             : knh::interp_voices_per_workgroup(nv, static_cast<unsigned>(h_prog.size()), static_cast<unsigned>(n_slots), interp_sigs, static_cast<unsigned>(block_size), sizeof(F) == 8);
    // words 9 and 10, the host's in an ordinary build: launches so far whose fold went to the bank's fold stream, beside the
    // launch after them, and launches whose tree fold took the form without LDS.  (A -DKNH_DAG_STAMPS build's kernels write
    // their stamps into words 4..11: there the stamps stay.)
#ifndef KNH_DAG_STAMPS
    out16[9] = static_cast<uint32_t>(overlapped_launches);
    out16[10] = static_cast<uint32_t>(wave_folds);
#endif
    return KNH_OK;
  }
  int synchronize() override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    { int rl = resident.leave(); if (rl != KNH_OK) return rl; }
    KNH_HIP(hipSetDevice(device));
    KNH_HIP(hipDeviceSynchronize());
    return KNH_OK;
  }
  int timing_collect() {
    KNH_HIP(hipDeviceSynchronize());
    for (size_t k = 0; k < timing_used; ++k) {
      float ms = 0.f;
      KNH_HIP(hipEventElapsedTime(&ms, timing_pool[k].first, timing_pool[k].second));
      timing_ms += ms;
      timing_launches += 1;
    }
    timing_used = 0;
    return KNH_OK;
  }
  int timing_reset(int enable) override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    { int rl = resident.leave(); if (rl != KNH_OK) return rl; }  // (kernel time is measured launch by launch: a timed bank launches per call)
    KNH_HIP(hipSetDevice(device));
    int rc = timing_collect();
    if (rc != KNH_OK) return rc;
    timing_ms = 0.0;
    timing_launches = 0;
    timing = enable != 0;
    return KNH_OK;
  }
  int timing_read(double* ms, uint64_t* launches) override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    KNH_HIP(hipSetDevice(device));
    int rc = timing_collect();
    if (rc != KNH_OK) return rc;
    if (ms) *ms = timing_ms;
    if (launches) *launches = timing_launches;
    return KNH_OK;
  }
};

}  // namespace
