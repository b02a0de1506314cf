// kernels_galactic.hip -- the Galactic reverb stage (voice_galactic.hpp): one wavefront per voice, a lane per frame.
// Built with -ffp-contract=off like every other kernel here: no multiply-add is fused where the reference has two roundings.
#include "voice_galactic.hpp"

namespace knh {
using namespace knh_dev;

template <typename F>
static hipError_t launch_galactic(const GalacticArgs<F>& a, hipStream_t s) {
  if (a.n_voices == 0 || a.frame_end <= a.frame_begin) return hipSuccess;
  hipLaunchKernelGGL((galactic_kernel<F>), dim3(a.n_voices), dim3(64), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_galactic_f32(const GalacticArgs<float>& a, hipStream_t s) { return launch_galactic<float>(a, s); }
hipError_t launch_galactic_f64(const GalacticArgs<double>& a, hipStream_t s) { return launch_galactic<double>(a, s); }

}  // namespace knh
