// voice_galactic.hpp -- KNH_STAGE_GALACTIC on the device: airwindows' Galactic reverb as ported in
// knaster_airwindows/src/galactic.rs:14-400 on StaticSampleDelay (knaster_core_dsp/src/ugens/delay.rs:308-416), one stereo
// reverb per voice, its 24 long rings in HBM.  Citations are file:line in the knaster repo.
//
// A LANE PER FRAME, A WAVEFRONT PER VOICE.  read() after write_and_advance() returns what was written delay_length - 1
// samples ago, and the feedback of the third bank re-enters only through the first bank's rings.  So over a run of
// T < min(delay_length) consecutive samples nothing that is read from a ring was written inside the run: the three banks are
// feed-forward over the run, lane k computes sample k of it, and every ring access is ONE load and ONE store of T
// consecutive samples (modulo the wrap) per wavefront -- 24 coalesced 256-byte (f32) reads and writes per 64 samples, never a
// lane gathering single samples out of the voice's 550 KB.  All 24 loads are issued before the first store (lane k reads the
// slot lane k + 1 writes), with a wavefront fence between.  T = min(64, min(delay_length) - 1), computed on the host per
// voice and block (GalParams::run): 64 at every sample rate from 44.1 kHz up at any bigness; shorter runs, down to sample
// by sample, below that.  The one step after a shrink that leaves `position` beyond the new length (delay.rs:395-398 wraps
// with % delay_length only after the write) is restated as it is: slot(0) = position, slot(k) = ((position + 1) % len + k - 1) % len.
//
// WHAT STAYS SERIAL over the run, in this order:
//   1. the two xorshift32 streams and the f64 phase vib_m with its reset (galactic.rs:226-230, :364-385): values that are the
//      same for every lane, stepped T times by the whole wavefront (integer work the compiler keeps in scalar registers),
//      lane k keeping step k's.  A voice whose detune is 0 skips the phase (it cannot move).
//   2. the input dither, the write to the 256-sample ring and its interpolated read are per lane: the ring lives in LDS as a
//      LINEAR history (the last 256 samples written, then the run's own), because lane k must see the ring as it was at
//      sample k.  sin() of the f64 phase is the device library's; a voice that never had detune > 0 gets the two offsets from
//      the host (vib_m is still its initial 3.0), which also makes that case bit-exact.
//   3. the one-pole iir_a: y = y * (1 - lowpass) + x[k] * lowpass in order (no re-associated scan: bit-exactness), the products
//      per lane, the recurrence by the whole wavefront over LDS, lane k keeping step k's.
//   4. the three banks: per lane.   5. iir_b like iir_a.   6. wet/dry and the output dither: per lane.
// The dependency between the halves is per run, not per sample.
//
// The L and R rings of a pair are written in lockstep with one length, so one position serves both: 12 positions.
//
// Output dither (galactic.rs:364-385 with frexp, :390-400): the exponent is taken from the f32's bits; exp + 62 >= 64 wraps the
// reference's 2_u64.pow to 0 in a release build (no dither at |s| >= 2), which is what happens here (knaster_hip.h).
#pragma once
#include <hip/hip_runtime.h>

namespace knh_dev {

typedef unsigned int gu32;
constexpr int GAL_RINGS = 12;      // per channel
constexpr int GAL_DETUNE = 256;    // the two short rings (galactic.rs:65-66)
constexpr int GAL_RUN = 64;

// per voice and block, computed on the host in F in the reference's order (galactic.rs:176-191)
template <typename F>
struct GalParams {
  double drift;          // drift.to_f64()
  double off_l, off_r;   // const_off: (sin(vib_m) + 1) * 127 and its quarter-turn twin, vib_m = 3.0
  F regen, attenuate, lowpass, one_minus_lowpass, wet, one_minus_wet;
  gu32 len[GAL_RINGS];   // delay_length after set_delay_length_fraction
  gu32 run;              // T
  gu32 const_off;
};
template <typename F>
struct GalState {
  double vib_m, oldfpd;
  gu32 fpd_l, fpd_r;
  gu32 dpos;             // position of the two 256-sample rings (they advance together)
  gu32 pos[GAL_RINGS];
  gu32 pad;
  F iir[4];              // iir_al, iir_ar, iir_bl, iir_br
  F fb[2][4];            // feedback
  F hist[2][GAL_DETUNE]; // the 256-sample rings, oldest sample first
};
template <typename F>
struct GalacticArgs {
  const F* in;           // [n_voices][block_size]: the voice's mono signal (both inputs of the reverb); the stereo-input
                         // variant: [2][n_voices][block_size], the left input's plane, then the right input's
  F* out;                // [2][n_voices][block_size]
  F* rings;              // [n_voices][ring_stride]: per voice, left rings 0..11 then right rings 0..11
  const GalParams<F>* params;
  GalState<F>* state;
  unsigned long long ring_stride;
  gu32 ring_off[GAL_RINGS];
  gu32 right_off;
  gu32 n_voices, block_size, frame_begin, frame_end;
};

template <typename F>
__device__ __forceinline__ F gal_mix(const F* b, int i) {  // galactic.rs:285-289
  return b[i] - (b[(1 + i) & 3] + b[(2 + i) & 3] + b[(3 + i) & 3]);
}
__device__ __forceinline__ gu32 gal_xorshift(gu32 x) {
  x ^= x << 13;
  x ^= x >> 17;
  x ^= x << 5;
  return x;
}
// the factor 2_u64.pow(exp + 62) as f64 of galactic.rs:372 for the sample s (see the header comment)
__device__ __forceinline__ double gal_dither_scale(float s) {
  if (s == 0.0f) return 4611686018427387904.0;  // exp = 0
  const gu32 e = (__float_as_uint(s) >> 23) & 0xFFu;
  if (e == 0xFFu) return (__float_as_uint(s) & 0x7FFFFFu) ? 4611686018427387904.0 /* NaN as u32 = 0 */
                                                           : 2305843009213693952.0 /* inf: u32::MAX + 62 wraps to 61 */;
  if (e <= 126u) return 4611686018427387904.0;  // |s| < 1: exp <= 0 -> 0, 2^62
  if (e == 127u) return 9223372036854775808.0;  // 1 <= |s| < 2: 2^63
  return 0.0;                                   // 2^64 and beyond wrap to 0
}

// StereoIn: (l | r) >> Galactic -- the two inputs are different signals: a load, a faint-input test and a dry term per side
// (galactic.rs:208-219, :350-357).  false: one signal on both inputs, one load and one test (what x_l == x_r makes of them).
template <typename F, bool StereoIn>
__global__ void __launch_bounds__(64) galactic_kernel(GalacticArgs<F> a) {
  __shared__ F hist[2][GAL_DETUNE + GAL_RUN];
  __shared__ F ser[2][GAL_RUN];
  const gu32 v = blockIdx.x;
  const gu32 lane = threadIdx.x;
  if (v >= a.n_voices) return;
  GalState<F>& st = a.state[v];
  const GalParams<F>& P = a.params[v];
  F* const ring = a.rings + (unsigned long long)v * a.ring_stride;
  for (int q = 0; q < GAL_DETUNE / 64; ++q) {
    hist[0][lane + 64 * q] = st.hist[0][lane + 64 * q];
    hist[1][lane + 64 * q] = st.hist[1][lane + 64 * q];
  }
  double vib = st.vib_m, oldfpd = st.oldfpd;
  gu32 fl = __builtin_amdgcn_readfirstlane(st.fpd_l), fr = __builtin_amdgcn_readfirstlane(st.fpd_r);
  gu32 dpos = __builtin_amdgcn_readfirstlane(st.dpos);
  gu32 pos[GAL_RINGS], len[GAL_RINGS];
#pragma unroll
  for (int i = 0; i < GAL_RINGS; ++i) {
    pos[i] = __builtin_amdgcn_readfirstlane(st.pos[i]);
    len[i] = __builtin_amdgcn_readfirstlane(P.len[i]);
  }
  F ya_l = st.iir[0], ya_r = st.iir[1], yb_l = st.iir[2], yb_r = st.iir[3];
  F fb0[4], fb1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { fb0[i] = st.fb[0][i]; fb1[i] = st.fb[1][i]; }
  const F regen = P.regen, attenuate = P.attenuate, lowpass = P.lowpass, oml = P.one_minus_lowpass, wet = P.wet, omw = P.one_minus_wet;
  const double drift = P.drift;
  const bool drifting = !(drift == 0.0);
  const bool const_off = P.const_off != 0u;
  gu32 run = __builtin_amdgcn_readfirstlane(P.run);
  if (run < 1u) run = 1u;
  if (run > (gu32)GAL_RUN) run = GAL_RUN;
  const F* in = a.in + (unsigned long long)v * a.block_size;
  F* out_l = a.out + (unsigned long long)v * a.block_size;
  F* out_r = a.out + ((unsigned long long)a.n_voices + v) * a.block_size;
  __syncthreads();

  for (gu32 n = a.frame_begin; n < a.frame_end;) {
    const gu32 left = a.frame_end - n;
    const gu32 T = left < run ? left : run;
    const bool active = lane < T;
    // 1. the values every lane shares, stepped in order; lane k keeps step k's
    gu32 fl0 = 0, fr0 = 0, fl1 = 0, fr1 = 0;
    double my_vib = vib;
    for (gu32 j = 0; j < T; ++j) {
      if (drifting) {  // galactic.rs:226-230
        vib += oldfpd * drift;
        if (vib > 6.28318530717958647692528676655900577) {
          vib = 0.0;
          oldfpd = 0.4294967295 + ((double)fl * 0.0000000000618);
        }
      }
      const gu32 nl = gal_xorshift(fl), nr = gal_xorshift(fr);
      if (lane == j) { fl0 = fl; fr0 = fr; fl1 = nl; fr1 = nr; my_vib = vib; }
      fl = nl;
      fr = nr;
    }
    // 2. input dither, the 256-sample rings (galactic.rs:208-246)
    F x = active ? in[n + lane] : (F)0;
    const bool faint = (double)(x < (F)0 ? -x : x) < 1.18e-23;
    const F x_l = faint ? (F)((double)fl0 * 1.18e-17) : x;
    F x_r;
    if constexpr (StereoIn) {  // the right input's plane, its own test (galactic.rs:215-219)
      const F xr = active ? in[(unsigned long long)a.n_voices * a.block_size + n + lane] : (F)0;
      const bool faint_r = (double)(xr < (F)0 ? -xr : xr) < 1.18e-23;
      x_r = faint_r ? (F)((double)fr0 * 1.18e-17) : xr;
    } else {
      x_r = faint ? (F)((double)fr0 * 1.18e-17) : x;
    }
    if (active) {
      hist[0][GAL_DETUNE + lane] = x_l * attenuate;
      hist[1][GAL_DETUNE + lane] = x_r * attenuate;
    }
    __syncthreads();
    F a_l, a_r;
    {
      const gu32 p = (dpos + lane + 1u) & (GAL_DETUNE - 1u);  // `position` after this sample's write
      double off_l = P.off_l, off_r = P.off_r;
      if (!const_off) {
        off_l = (sin(my_vib) + 1.0) * 127.0;
        off_r = (sin(my_vib + (3.14159265358979323846264338327950288 / 2.0)) + 1.0) * 127.0;
      }
      const F idx_l = (F)((double)p + off_l), idx_r = (F)((double)p + off_r);
      // read_at_lin (delay.rs:378-392): slot (p + d) % 256 holds the sample written 255 - d samples ago, d = 0 .. 254
      gu32 dl0 = (gu32)floor(idx_l) - p, dl1 = (gu32)ceil(idx_l) - p, dr0 = (gu32)floor(idx_r) - p, dr1 = (gu32)ceil(idx_r) - p;
      dl0 = dl0 > 255u ? 255u : dl0; dl1 = dl1 > 255u ? 255u : dl1;  // (an index the reference would panic on stays inside the history)
      dr0 = dr0 > 255u ? 255u : dr0; dr1 = dr1 > 255u ? 255u : dr1;
      const F lo_l = hist[0][lane + 1u + dl0], hi_l = hist[0][lane + 1u + dl1];
      const F lo_r = hist[1][lane + 1u + dr0], hi_r = hist[1][lane + 1u + dr1];
      a_l = lo_l + (hi_l - lo_l) * (idx_l - trunc(idx_l));
      a_r = lo_r + (hi_r - lo_r) * (idx_r - trunc(idx_r));
    }
    // 3. iir_a (galactic.rs:248-251)
    ser[0][lane] = a_l * lowpass;
    ser[1][lane] = a_r * lowpass;
    __syncthreads();
    for (gu32 j = 0; j < T; ++j) {
      ya_l = (ya_l * oml) + ser[0][j];
      ya_r = (ya_r * oml) + ser[1][j];
      if (lane == j) { a_l = ya_l; a_r = ya_r; }
    }
    __syncthreads();
    // 4. the three banks of four rings (galactic.rs:258-343): all reads, then all writes
    F rl[GAL_RINGS], rr[GAL_RINGS];
    gu32 wslot[GAL_RINGS];
#pragma unroll
    for (int i = 0; i < GAL_RINGS; ++i) {
      const gu32 L = len[i];
      gu32 p1 = pos[i] + 1u;
      if (p1 >= L) p1 %= L;
      gu32 rs = p1 + lane;          // the slot read() sees after this lane's write_and_advance
      if (rs >= L) rs -= L;
      gu32 ws = p1 + lane - 1u;     // (lane 0: not used)
      if (lane > 0u && ws >= L) ws -= L;
      wslot[i] = lane == 0u ? pos[i] : ws;
      gu32 np = p1 + T - 1u;
      if (np >= L) np -= L;
      pos[i] = np;
      rl[i] = active ? ring[a.ring_off[i] + rs] : (F)0;
      rr[i] = active ? ring[a.right_off + a.ring_off[i] + rs] : (F)0;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    F nf0[4], nf1[4];  // the feedback this sample leaves: galactic.rs:327-334
#pragma unroll
    for (int i = 0; i < 4; ++i) { nf0[i] = gal_mix(rl + 8, i); nf1[i] = gal_mix(rr + 8, i); }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      F p0 = __shfl_up(nf0[i], 1), p1 = __shfl_up(nf1[i], 1);  // the feedback the sample before left
      if (lane == 0u) { p0 = fb0[i]; p1 = fb1[i]; }
      const gu32 last = T - 1u;
      fb0[i] = __shfl(nf0[i], (int)last);
      fb1[i] = __shfl(nf1[i], (int)last);
      if (active) {
        ring[a.ring_off[i] + wslot[i]] = (p1 * regen) + a_l;                 // left rings take feedback[1], :259-265
        ring[a.right_off + a.ring_off[i] + wslot[i]] = (p0 * regen) + a_r;
        ring[a.ring_off[4 + i] + wslot[4 + i]] = gal_mix(rl, i);
        ring[a.right_off + a.ring_off[4 + i] + wslot[4 + i]] = gal_mix(rr, i);
        ring[a.ring_off[8 + i] + wslot[8 + i]] = gal_mix(rl + 4, i);
        ring[a.right_off + a.ring_off[8 + i] + wslot[8 + i]] = gal_mix(rr + 4, i);
      }
    }
    F o_l = (((((F)0 + rl[8]) + rl[9]) + rl[10]) + rl[11]) * (F)0.125;  // iter().sum() starts from zero
    F o_r = (((((F)0 + rr[8]) + rr[9]) + rr[10]) + rr[11]) * (F)0.125;
    // 5. iir_b (galactic.rs:345-348)
    ser[0][lane] = o_l * lowpass;
    ser[1][lane] = o_r * lowpass;
    __syncthreads();
    for (gu32 j = 0; j < T; ++j) {
      yb_l = (yb_l * oml) + ser[0][j];
      yb_r = (yb_r * oml) + ser[1][j];
      if (lane == j) { o_l = yb_l; o_r = yb_r; }
    }
    // 6. wet/dry, output dither (galactic.rs:350-385)
    if (wet < (F)1) {
      o_l = (o_l * wet) + (x_l * omw);
      o_r = (o_r * wet) + (x_r * omw);
    }
    o_l += (F)((((double)fl1 - 2147483647.0) * 5.5e-36) * gal_dither_scale((float)o_l));
    o_r += (F)((((double)fr1 - 2147483647.0) * 5.5e-36) * gal_dither_scale((float)o_r));
    if (active) {
      out_l[n + lane] = o_l;
      out_r[n + lane] = o_r;
    }
    // the history moves up by the run
    F keep[2][GAL_DETUNE / 64];
#pragma unroll
    for (int q = 0; q < GAL_DETUNE / 64; ++q) {
      keep[0][q] = hist[0][lane + 64 * q + T];
      keep[1][q] = hist[1][lane + 64 * q + T];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < GAL_DETUNE / 64; ++q) {
      hist[0][lane + 64 * q] = keep[0][q];
      hist[1][lane + 64 * q] = keep[1][q];
    }
    __syncthreads();
    dpos = (dpos + T) & (GAL_DETUNE - 1u);
    n += T;
  }
  for (int q = 0; q < GAL_DETUNE / 64; ++q) {
    st.hist[0][lane + 64 * q] = hist[0][lane + 64 * q];
    st.hist[1][lane + 64 * q] = hist[1][lane + 64 * q];
  }
  if (lane == 0u) {
    st.vib_m = vib;
    st.oldfpd = oldfpd;
    st.fpd_l = fl;
    st.fpd_r = fr;
    st.dpos = dpos;
#pragma unroll
    for (int i = 0; i < GAL_RINGS; ++i) st.pos[i] = pos[i];
    st.iir[0] = ya_l; st.iir[1] = ya_r; st.iir[2] = yb_l; st.iir[3] = yb_r;
#pragma unroll
    for (int i = 0; i < 4; ++i) { st.fb[0][i] = fb0[i]; st.fb[1][i] = fb1[i]; }
  }
}

}  // namespace knh_dev

namespace knh {
// one wavefront per voice, frames [frame_begin, frame_end) of one block (kernels_galactic.hip)
// stereo_in: the variant that reads a left and a right input plane
hipError_t launch_galactic_f32(const knh_dev::GalacticArgs<float>& a, bool stereo_in, hipStream_t s);
hipError_t launch_galactic_f64(const knh_dev::GalacticArgs<double>& a, bool stereo_in, hipStream_t s);
}  // namespace knh
