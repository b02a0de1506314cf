// kernels_galactic.hip -- the Galactic reverb stage (voice_galactic.hpp): one wavefront per voice, a lane per frame.
// Built with -ffp-contract=off like every other kernel here: no multiply-add is fused where the reference has two roundings.
#include "voice_galactic.hpp"

namespace knh {
using namespace knh_dev;

template <typename F>
static hipError_t launch_galactic(const GalacticArgs<F>& a, bool stereo_in, hipStream_t s) {
  if (a.n_voices == 0 || a.frame_end <= a.frame_begin) return hipSuccess;
  if (stereo_in) hipLaunchKernelGGL((galactic_kernel<F, true>), dim3(a.n_voices), dim3(64), 0, s, a);
  else hipLaunchKernelGGL((galactic_kernel<F, false>), dim3(a.n_voices), dim3(64), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_galactic_f32(const GalacticArgs<float>& a, bool stereo_in, hipStream_t s) { return launch_galactic<float>(a, stereo_in, s); }
hipError_t launch_galactic_f64(const GalacticArgs<double>& a, bool stereo_in, hipStream_t s) { return launch_galactic<double>(a, stereo_in, s); }

}  // namespace knh
