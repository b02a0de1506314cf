// galactic_bank.hpp -- a bank whose chain ends in KNH_STAGE_GALACTIC (knaster_airwindows/src/galactic.rs:14-400): the chain
// before the reverb is an ordinary Bank<F> (voice_bank.hpp: any kernel form it would take anyway, its events and queues
// untouched) that renders each block's per-voice signals into a staging buffer, [n_voices][block_size] -- 8 bytes per
// voice-sample against the ~200 the reverb's rings move -- and the reverb kernel (voice_galactic.hpp) reads them, one
// wavefront per voice, and writes the voice's left and right signals, [2][n_voices][block_size], which the fold kernels mix
// as they mix a Pan2 chain's two planes.  (l | r) >> Galactic (the stage names both of its inputs): the chain before the
// reverb is that ordinary bank with two connected outputs (l, r) -- knh_bank_connect_outputs' machinery and signature -- the
// staging buffer is its two planes, [2][n_voices][block_size], and the reverb kernel's stereo-input variant reads the left
// plane on its left side and the right plane on its right; everything else is the same.
// A launch of n blocks is n such pairs of kernels in stream order: the reverb's
// parameters take effect at a block boundary (at the next `process`, galactic.rs:172-201), so a call addressed to block b of
// the launch is applied on the host between the kernels of block b - 1 and b.  Included by bank.hip only.
//
// RING LAYOUT: per voice contiguous -- voice v's 24 rings lie one after the other (left 0..11, right 0..11, each start
// rounded up to 64 samples) in one stretch of ring_stride samples.  A wavefront serves one voice and touches 24 short
// consecutive pieces per run; per voice contiguous keeps those 24 streams inside ~550 KB (one or two 2 MB pages of the
// translation cache) where a ring-major layout would spread them over 24 regions n_voices * ring apart.
//
// The per-block scalars (regen, attenuate, lowpass, drift, size -> lengths, wet) are computed here in F, in the reference's
// operation order (galactic.rs:176-191), powi by the multiply-by-squaring of compiler-builtins' __powisf2 / __powidf2.
#pragma once
#include "voice_galactic.hpp"

namespace {

constexpr uint32_t kGalacticDelayTimes[12] = {6480, 3660, 1720, 680, 9700, 6000, 2320, 940, 15220, 8460, 4540, 3200};  // galactic.rs:39-41

template <typename F>
inline F gal_powi(F a, int b) {  // b > 0
  F r = 1;
  for (;;) {
    if (b & 1) r *= a;
    b /= 2;
    if (b == 0) break;
    a *= a;
  }
  return r;
}

template <typename F>
struct GalacticBank final : knh_bank {
  std::unique_ptr<Bank<F>> inner;  // the chain without its last stage
  uint32_t nv = 0;
  uint32_t gstage = 0;             // index of the Galactic stage (the last)
  std::vector<double> gctor;       // [nv][7]
  std::vector<F> par;              // [nv][5]: replace, detune, brightness, bigness, wet as F (param_apply: value as F)
  std::vector<unsigned char> drifted;  // the voice has run a block with detune != 0: vib_m may have left 3.0
  std::vector<knh_dev::GalParams<F>> h_params;
  bool params_dirty = true;
  uint32_t base_len[12] = {};
  uint32_t ring_off[12] = {};
  uint32_t right_off = 0;
  uint64_t ring_stride = 0;
  F overallscale = 0;
  struct Call { uint32_t voice, param; double f; };
  std::vector<std::vector<Call>> future;  // calls addressed to later blocks of the next launch
  bool stereo_in = false;  // (l | r) >> Galactic: the inner bank has two connected outputs, the staging buffer two planes
  F* d_stage = nullptr;    // [nv][block]; stereo_in: [2][nv][block]
  F* d_gvoices = nullptr;  // [2][nv][block]
  F* d_rings = nullptr;
  knh_dev::GalParams<F>* d_params = nullptr;
  knh_dev::GalState<F>* d_state = nullptr;
  F* d_out = nullptr;
  F* h_out = nullptr;
  uint32_t out_blocks = 0;
  hipStream_t own_stream = nullptr;

  ~GalacticBank() override {
    if (initialised) {
      (void)hipSetDevice(device);
      (void)hipDeviceSynchronize();
    }
    inner.reset();
    if (initialised) (void)hipSetDevice(device);
    if (d_stage) (void)hipFree(d_stage);
    if (d_gvoices) (void)hipFree(d_gvoices);
    if (d_rings) (void)hipFree(d_rings);
    if (d_params) (void)hipFree(d_params);
    if (d_state) (void)hipFree(d_state);
    if (d_out) (void)hipFree(d_out);
    if (d_inner_mix) (void)hipFree(d_inner_mix);
    if (h_out) (void)hipHostFree(h_out);
    if (own_stream) (void)hipStreamDestroy(own_stream);
    for (auto& e : timing_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  }
  int adopt(int rc) {
    if (rc != KNH_OK) err = inner->err;
    return rc;
  }
  bool mine(uint32_t stage) const { return stage == gstage; }

  int set_ctor(uint32_t stage, uint32_t first, uint32_t count, const double* args, uint32_t n_args) override {
    if (!mine(stage)) return adopt(inner->set_ctor(stage, first, count, args, n_args));
    if (initialised) return fail(KNH_ERR_INVALID_ARGUMENT, "constructor arguments must be set before init");
    if (static_cast<uint64_t>(first) + count > nv) return fail(KNH_ERR_OUT_OF_RANGE, "voice range out of range");
    if (n_args != 7) return fail(KNH_ERR_INVALID_ARGUMENT, "wrong number of constructor arguments");
    if (!args) return fail(KNH_ERR_INVALID_ARGUMENT, "null args");
    std::copy(args, args + static_cast<size_t>(count) * 7, gctor.begin() + static_cast<size_t>(first) * 7);
    return KNH_OK;
  }
  int set_buffer(uint32_t stage, const void* samples, size_t n_frames, double sr) override {
    if (mine(stage)) return fail(KNH_ERR_INVALID_ARGUMENT, "stage is not a BufferReader");
    return adopt(inner->set_buffer(stage, samples, n_frames, sr));
  }
  int add_buffer(uint32_t stage, const void* samples, size_t n_frames, uint32_t n_channels, double sr, uint32_t* out_index) override {
    if (mine(stage)) return fail(KNH_ERR_INVALID_ARGUMENT, "stage is not a BufferReader");
    return adopt(inner->add_buffer(stage, samples, n_frames, n_channels, sr, out_index));
  }
  int assign_buffers(uint32_t stage, size_t count, const uint32_t* voices, const uint32_t* ids, const double* ctor) override {
    if (mine(stage)) return fail(KNH_ERR_INVALID_ARGUMENT, "stage is not a BufferReader");
    return adopt(inner->assign_buffers(stage, count, voices, ids, ctor));
  }
  uint32_t buffer_count(uint32_t stage) const override { return mine(stage) ? 0u : inner->buffer_count(stage); }
  int add_wavetable(uint32_t stage, const void* samples, uint32_t n_tables, uint32_t* out_index) override {
    if (mine(stage)) return fail(KNH_ERR_INVALID_ARGUMENT, "not a KNH_STAGE_FLAG_WAVETABLE stage");
    return adopt(inner->add_wavetable(stage, samples, n_tables, out_index));
  }
  int assign_wavetables(uint32_t stage, size_t count, const uint32_t* voices, const uint32_t* ids, const double* ctor) override {
    if (mine(stage)) return fail(KNH_ERR_INVALID_ARGUMENT, "not a KNH_STAGE_FLAG_WAVETABLE stage");
    return adopt(inner->assign_wavetables(stage, count, voices, ids, ctor));
  }
  uint32_t wavetable_count(uint32_t stage) const override { return mine(stage) ? 0u : inner->wavetable_count(stage); }
  // The reverb's 24 rings and its state live here, not in the inner bank, and have no restart yet
  int set_voice_ctor(uint32_t, size_t, const uint32_t*, const double*, uint32_t, bool) override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    return fail(KNH_ERR_UNSUPPORTED_CHAIN, "the voices of a chain that ends in Galactic cannot be restarted");
  }
  int restart_voices(size_t, const uint32_t*) override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    return fail(KNH_ERR_UNSUPPORTED_CHAIN, "the voices of a chain that ends in Galactic cannot be restarted");
  }
  int set_input(uint32_t n_blocks, const void* host, const void* dev) override {
    if (n_blocks > 1) return fail(KNH_ERR_INVALID_ARGUMENT, "a chain that ends in Galactic takes its bank inputs one block per call");
    return adopt(inner->set_input(n_blocks, host, dev));
  }
  static bool bigness_ok(F b) { return b >= F(0) && b <= F(1); }  // (NaN fails both)

  int init(uint32_t sr, size_t bs) override {
    if (initialised) return fail(KNH_ERR_INVALID_ARGUMENT, "already initialised");
    for (uint32_t v = 0; v < nv; ++v) {
      const double* c = &gctor[static_cast<size_t>(v) * 7];
      for (int k = 5; k < 7; ++k)
        if (!(c[k] >= 1.0 && c[k] <= 4294967295.0) || c[k] != std::floor(c[k]))
          return fail(KNH_ERR_INVALID_ARGUMENT, "Galactic: fpd_l and fpd_r are integers in 1 .. 2^32 - 1 (0 would stay 0 in xorshift32)");
      if (!bigness_ok(static_cast<F>(c[3]))) return fail(KNH_ERR_OUT_OF_RANGE, "Galactic: bigness must be within 0 .. 1");
    }
    int rc = inner->init(sr, bs);
    if (rc != KNH_OK) return adopt(rc);
    device = inner->device;
    sample_rate = sr;
    block_size = bs;
    KNH_HIP(hipSetDevice(device));
    uint32_t off = 0;
    for (int i = 0; i < 12; ++i) {  // galactic.rs:52-60
      base_len[i] = static_cast<uint32_t>((static_cast<double>(kGalacticDelayTimes[i]) / 44100.) * static_cast<double>(sr));
      ring_off[i] = off;
      off += (base_len[i] + 63u) & ~63u;
    }
    // a run needs min(delay_length) >= 2 (read() must not return the sample just written); the shortest ring at bigness 0
    if (static_cast<uint32_t>(static_cast<F>(base_len[3]) * F(0.1)) < 2u)
      return fail(KNH_ERR_INVALID_ARGUMENT, "Galactic: the sample rate is too low for its shortest delay line");
    right_off = off;
    ring_stride = 2ull * off;
    {
      double os = 1.0;  // galactic.rs:70-73
      os /= 44100.0;
      os *= static_cast<double>(sr);
      overallscale = static_cast<F>(os);
    }
    const size_t ring_bytes = static_cast<size_t>(nv) * ring_stride * sizeof(F);
    const size_t stage_planes = stereo_in ? 2 : 1;
    const size_t other = static_cast<size_t>(nv) * ((2 + stage_planes) * bs * sizeof(F) + sizeof(knh_dev::GalState<F>) + sizeof(knh_dev::GalParams<F>)) + (1u << 20);
    size_t free_b = 0, total_b = 0;
    KNH_HIP(hipMemGetInfo(&free_b, &total_b));
    if (ring_bytes + other > free_b) return fail(KNH_ERR_DEVICE, "Galactic: the delay rings do not fit in device memory");
    KNH_HIP(hipMalloc(&d_rings, ring_bytes));
    KNH_HIP(hipMemset(d_rings, 0, ring_bytes));  // vec![F::ZERO; len]
    KNH_HIP(hipMalloc(&d_stage, stage_planes * nv * bs * sizeof(F)));
    KNH_HIP(hipMemset(d_stage, 0, stage_planes * nv * bs * sizeof(F)));
    KNH_HIP(hipMalloc(&d_gvoices, 2 * static_cast<size_t>(nv) * bs * sizeof(F)));
    KNH_HIP(hipMemset(d_gvoices, 0, 2 * static_cast<size_t>(nv) * bs * sizeof(F)));
    KNH_HIP(hipMalloc(&d_params, static_cast<size_t>(nv) * sizeof(knh_dev::GalParams<F>)));
    KNH_HIP(hipMalloc(&d_state, static_cast<size_t>(nv) * sizeof(knh_dev::GalState<F>)));
    std::vector<knh_dev::GalState<F>> st(nv);
    std::memset(static_cast<void*>(st.data()), 0, st.size() * sizeof(knh_dev::GalState<F>));
    for (uint32_t v = 0; v < nv; ++v) {  // Galactic::new, galactic.rs:145-170
      const double* c = &gctor[static_cast<size_t>(v) * 7];
      par[v * 5 + 0] = static_cast<F>(c[0]);
      par[v * 5 + 1] = static_cast<F>(c[1]);
      par[v * 5 + 2] = static_cast<F>(c[2]);
      par[v * 5 + 3] = static_cast<F>(c[3]);
      par[v * 5 + 4] = static_cast<F>(c[4]);
      st[v].vib_m = 3.;
      st[v].oldfpd = 429496.7295;
      st[v].fpd_l = static_cast<uint32_t>(c[5]);
      st[v].fpd_r = static_cast<uint32_t>(c[6]);
    }
    KNH_HIP(hipMemcpy(d_state, st.data(), st.size() * sizeof(knh_dev::GalState<F>), hipMemcpyHostToDevice));
    KNH_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
    inner->stage_out = d_stage;
    params_dirty = true;
    initialised = true;
    return KNH_OK;
  }

  // galactic.rs:176-191 for voice v, as the next `process` would compute them
  void voice_params(uint32_t v, knh_dev::GalParams<F>& p) {
    const F one = 1;
    const F replace = par[v * 5 + 0], detune = par[v * 5 + 1], brightness = par[v * 5 + 2], bigness = par[v * 5 + 3], wetp = par[v * 5 + 4];
    const F regen = F(0.0625) + ((one - replace) * F(0.0625));
    const F attenuate = (one - (regen / F(0.125))) * F(1.333);
    const F lowpass = gal_powi<F>(F(1.00001) - (one - brightness), 2) / std::sqrt(overallscale);
    const F drift = gal_powi<F>(detune, 3) * F(0.001);
    const F size = (bigness * F(0.9)) + F(0.1);
    const F wet = one - gal_powi<F>(one - wetp, 3);
    p.regen = regen;
    p.attenuate = attenuate;
    p.lowpass = lowpass;
    p.one_minus_lowpass = one - lowpass;
    p.wet = wet;
    p.one_minus_wet = one - wet;
    p.drift = static_cast<double>(drift);
    uint32_t mn = 0xFFFFFFFFu;
    for (int i = 0; i < 12; ++i) {  // set_delay_length_fraction, delay.rs:337-342
      uint32_t l = static_cast<uint32_t>(static_cast<F>(base_len[i]) * size);
      l = std::min(std::max(l, 1u), base_len[i]);  // (bigness is kept within 0 .. 1: this never binds)
      p.len[i] = l;
      mn = std::min(mn, l);
    }
    p.run = std::max(1u, std::min<uint32_t>(knh_dev::GAL_RUN, mn - 1u));
    if (!(p.drift == 0.0)) drifted[v] = 1;
    p.const_off = drifted[v] ? 0u : 1u;
    // vib_m is still 3.0 (galactic.rs:160): the two offsets of :237-239 are constants
    p.off_l = (std::sin(3.) + 1.0) * 127.;
    p.off_r = (std::sin(3. + (3.14159265358979323846264338327950288 / 2.0)) + 1.0) * 127.;
  }
  int upload_params(hipStream_t s) {
    if (!params_dirty) return KNH_OK;
    // (the copy below reads pageable memory: it has returned from the vector before the call comes back)
    for (uint32_t v = 0; v < nv; ++v) voice_params(v, h_params[v]);
    KNH_HIP(hipMemcpyAsync(d_params, h_params.data(), static_cast<size_t>(nv) * sizeof(knh_dev::GalParams<F>), hipMemcpyHostToDevice, s));
    KNH_HIP(hipStreamSynchronize(s));
    params_dirty = false;
    return KNH_OK;
  }

  int check_mine(uint32_t voice, uint32_t param) {
    if (voice >= nv) return fail(KNH_ERR_OUT_OF_RANGE, "voice out of range");
    if (param >= 5) return fail(KNH_ERR_OUT_OF_RANGE, "param out of range");
    return KNH_OK;
  }
  int apply_mine(uint32_t voice, uint32_t param, uint32_t kind, double f) {
    int rc = check_mine(voice, param);
    if (rc != KNH_OK) return rc;
    if (kind != KNH_VALUE_FLOAT) return fail(KNH_ERR_WRONG_VALUE_KIND, "Galactic's parameters are floats");
    const F val = static_cast<F>(f);
    if (param == 3 && !bigness_ok(val)) return fail(KNH_ERR_OUT_OF_RANGE, "Galactic: bigness must be within 0 .. 1");
    par[voice * 5 + param] = val;
    params_dirty = true;
    return KNH_OK;
  }
  int param_apply(uint32_t voice, uint32_t stage, uint32_t param, uint32_t kind, double f, int64_t i) override {
    if (!mine(stage)) return adopt(inner->param_apply(voice, stage, param, kind, f, i));
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    return apply_mine(voice, param, kind, f);
  }
  int set_delay(uint32_t voice, uint32_t stage, uint32_t param, uint16_t delay) override {
    if (!mine(stage)) return adopt(inner->set_delay(voice, stage, param, delay));
    int rc = check_mine(voice, param);
    if (rc != KNH_OK) return rc;
    return delay == 0 ? KNH_OK : fail(KNH_ERR_INVALID_ARGUMENT, "Galactic is not wrapped in WrPreciseTiming: its parameters change at block boundaries");
  }
  int check_call(uint32_t voice, uint32_t stage, uint32_t param, uint32_t kind) override {
    if (!mine(stage)) return adopt(inner->check_call(voice, stage, param, kind));
    int rc = check_mine(voice, param);
    if (rc != KNH_OK) return rc;
    return kind == KNH_VALUE_FLOAT ? KNH_OK : fail(KNH_ERR_WRONG_VALUE_KIND, "Galactic's parameters are floats");
  }
  int call_at(uint32_t block_offset, bool is_delay, uint32_t voice, uint32_t stage, uint32_t param, uint32_t kind, double f, int64_t i,
              uint16_t delay) override {
    if (!mine(stage)) return adopt(inner->call_at(block_offset, is_delay, voice, stage, param, kind, f, i, delay));
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    if (is_delay) return set_delay(voice, stage, param, delay);
    if (block_offset == 0) return apply_mine(voice, param, kind, f);
    if (block_offset >= 4096) return fail(KNH_ERR_INVALID_ARGUMENT, "block_offset must be below 4096");
    int rc = check_mine(voice, param);
    if (rc != KNH_OK) return rc;
    if (kind != KNH_VALUE_FLOAT) return fail(KNH_ERR_WRONG_VALUE_KIND, "Galactic's parameters are floats");
    if (param == 3 && !bigness_ok(static_cast<F>(f))) return fail(KNH_ERR_OUT_OF_RANGE, "Galactic: bigness must be within 0 .. 1");
    if (future.size() <= block_offset) future.resize(block_offset + 1);
    future[block_offset].push_back(Call{voice, param, f});
    return KNH_OK;
  }

  int process(uint32_t n_blocks, size_t ftp, size_t offset, uint64_t clock, void* out_host, void* out_device, void* voices_host,
              uint32_t* out_flags, void* stream, bool sync, bool accumulate) override {
    if (accumulate && !out_device) return fail(KNH_ERR_INVALID_ARGUMENT, "accumulation needs a device output buffer");
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    if (offset + ftp > block_size) return fail(KNH_ERR_INVALID_ARGUMENT, "block_start_offset + frames_to_process exceeds block_size");
    if (n_blocks == 0 || n_blocks > 4096) return fail(KNH_ERR_INVALID_ARGUMENT, "n_blocks must be in 1..4096");
    if (n_blocks > 1 && (offset != 0 || ftp != block_size)) return fail(KNH_ERR_INVALID_ARGUMENT, "multi-block launches process whole blocks");
    if (n_blocks > 1 && voices_host) return fail(KNH_ERR_INVALID_ARGUMENT, "per-voice output is only available for single blocks");
    if (desc.mix_mode == KNH_MIX_LEFT_FOLD && n_blocks > 1) return fail(KNH_ERR_INVALID_ARGUMENT, "KNH_MIX_LEFT_FOLD processes one block per call");
    KNH_HIP(hipSetDevice(device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : own_stream;
    const uint32_t fb = static_cast<uint32_t>(offset), fe = static_cast<uint32_t>(offset + ftp);
    const size_t blk = 2 * block_size;  // out: [n_blocks][2][block_size]
    if (!out_device && n_blocks > out_blocks) {
      KNH_HIP(hipStreamSynchronize(s));
      if (d_out) KNH_HIP(hipFree(d_out));
      d_out = nullptr;
      if (h_out) KNH_HIP(hipHostFree(h_out));
      h_out = nullptr;
      KNH_HIP(hipMalloc(&d_out, static_cast<size_t>(n_blocks) * blk * sizeof(F)));
      KNH_HIP(hipMemsetAsync(d_out, 0, static_cast<size_t>(n_blocks) * blk * sizeof(F), s));
      KNH_HIP(hipHostMalloc(&h_out, static_cast<size_t>(n_blocks) * blk * sizeof(F)));
      out_blocks = n_blocks;
    }
    F* const dst = out_device ? static_cast<F*>(out_device) : d_out;
    std::pair<hipEvent_t, hipEvent_t>* tp = nullptr;
    if (timing) {  // device time of the whole launch: source chain, reverb and fold kernels of every block
      if (timing_used == timing_pool.size()) {
        if (timing_pool.size() >= 4096) {
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
      KNH_HIP(hipEventRecord(tp->first, s));
    }
    for (uint32_t b = 0; b < n_blocks; ++b) {
      if (b > 0 && b < future.size())
        for (const Call& c : future[b]) (void)apply_mine(c.voice, c.param, KNH_VALUE_FLOAT, c.f);
      int rc = upload_params(s);
      if (rc != KNH_OK) return rc;
      // the chain before the reverb: this block's voices into d_stage (its own mix of them is not used)
      rc = inner->process(1, ftp, offset, clock + static_cast<uint64_t>(b) * block_size, nullptr, inner_mix(), nullptr, nullptr, s, false, false);
      if (rc != KNH_OK) return adopt(rc);
      knh_dev::GalacticArgs<F> a;
      a.in = d_stage;
      a.out = d_gvoices;
      a.rings = d_rings;
      a.params = d_params;
      a.state = d_state;
      a.ring_stride = ring_stride;
      for (int i = 0; i < 12; ++i) a.ring_off[i] = ring_off[i];
      a.right_off = right_off;
      a.n_voices = nv;
      a.block_size = static_cast<uint32_t>(block_size);
      a.frame_begin = fb;
      a.frame_end = fe;
      KNH_HIP(launch(a, stereo_in, s));
      // the two planes are the two channels: the fold sees two "blocks" of one channel each (as for a Pan2 chain)
      KNH_HIP(launch_fold(desc.mix_mode != KNH_MIX_LEFT_FOLD, d_gvoices, nv, static_cast<unsigned>(block_size), fb, fe, dst + static_cast<size_t>(b) * blk, 1u,
                          static_cast<unsigned>(block_size), 2u, accumulate, s));
    }
    if (tp) KNH_HIP(hipEventRecord(tp->second, s));
    if (!future.empty()) {  // calls addressed beyond this launch move up; those now due are applied right away
      if (future.size() <= n_blocks) future.clear();
      else future.erase(future.begin(), future.begin() + n_blocks);
      if (!future.empty()) {
        for (const Call& c : future[0]) (void)apply_mine(c.voice, c.param, KNH_VALUE_FLOAT, c.f);
        future[0].clear();
      }
    }
    if (!sync) return KNH_OK;
    const size_t out_bytes = static_cast<size_t>(n_blocks) * blk * sizeof(F);
    if (out_host) KNH_HIP(hipMemcpyAsync(h_out, dst, out_bytes, hipMemcpyDeviceToHost, s));
    if (voices_host) KNH_HIP(hipMemcpyAsync(voices_host, d_gvoices, 2 * static_cast<size_t>(nv) * block_size * sizeof(F), hipMemcpyDeviceToHost, s));
    KNH_HIP(hipStreamSynchronize(s));
    if (out_host) {
      if (n_blocks > 1) {
        std::memcpy(out_host, h_out, out_bytes);
      } else {
        for (uint32_t c = 0; c < 2; ++c)
          std::memcpy(static_cast<F*>(out_host) + c * block_size + offset, h_out + c * block_size + offset, ftp * sizeof(F));
      }
    }
    if (out_flags) *out_flags = 0;  // a reverb tail does not end with its input: the bank never reports itself done
    return KNH_OK;
  }
  F* d_inner_mix = nullptr;  // where the inner bank's own mix goes (not used): one block of each of its output channels
  F* inner_mix() {
    if (!d_inner_mix) {
      if (hipMalloc(&d_inner_mix, (stereo_in ? 2 : 1) * block_size * sizeof(F)) != hipSuccess) return nullptr;
    }
    return d_inner_mix;
  }
  static hipError_t launch(const knh_dev::GalacticArgs<float>& a, bool stereo, hipStream_t s) { return knh::launch_galactic_f32(a, stereo, s); }
  static hipError_t launch(const knh_dev::GalacticArgs<double>& a, bool stereo, hipStream_t s) { return knh::launch_galactic_f64(a, stereo, s); }
  static hipError_t launch_fold(bool tree, const float* rows, unsigned n, unsigned len, unsigned fb, unsigned fe, float* out, unsigned ch, unsigned os, unsigned nb, bool acc, hipStream_t s) {
    return knh::launch_fold_f32(tree, rows, n, len, fb, fe, out, ch, os, nb, acc, nullptr, s, nullptr);
  }
  static hipError_t launch_fold(bool tree, const double* rows, unsigned n, unsigned len, unsigned fb, unsigned fe, double* out, unsigned ch, unsigned os, unsigned nb, bool acc, hipStream_t s) {
    return knh::launch_fold_f64(tree, rows, n, len, fb, fe, out, ch, os, nb, acc, nullptr, s, nullptr);
  }

  int read_done_frames(uint32_t* out) override { return adopt(inner->read_done_frames(out)); }
  int synchronize() override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    KNH_HIP(hipSetDevice(device));
    KNH_HIP(hipStreamSynchronize(own_stream));
    return adopt(inner->synchronize());
  }
  int debug_read(uint32_t* out16) override { return adopt(inner->debug_read(out16)); }
  const char* debug_signature() const override { return inner->debug_signature(); }
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> timing_pool;
  size_t timing_used = 0;
  double timing_ms = 0.0;
  uint64_t timing_launches = 0;
  int timing_collect() {
    for (size_t k = 0; k < timing_used; ++k) {
      KNH_HIP(hipEventSynchronize(timing_pool[k].second));
      float ms = 0.f;
      KNH_HIP(hipEventElapsedTime(&ms, timing_pool[k].first, timing_pool[k].second));
      timing_ms += ms;
      ++timing_launches;
    }
    timing_used = 0;
    return KNH_OK;
  }
  int timing_reset(int enable) override {
    if (!initialised) return fail(KNH_ERR_NOT_INITIALISED, "bank not initialised");
    KNH_HIP(hipSetDevice(device));
    int rc = timing_collect();
    if (rc != KNH_OK) return rc;
    timing = enable != 0;
    timing_ms = 0.0;
    timing_launches = 0;
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
