// Weight-gradient GEMMs (dw.hip) in their own translation unit: the operand-type x tile-shape
// instantiations of k_dw compile in parallel with the phase-kernel sets.
#include "dw.hip"

namespace spp {
void launch_dw_kernels(const DwJob* jobs, const int* item_job, const int* item_split, int nitems, int nlds,
                       int njobs, int64_t max_elems, bool bf16, int big_waves, hipStream_t st) {
  const auto thin = bf16 ? k_dw<true> : k_dw<false>;  // named before k_dw_big8<> (dw.hip: the order of emission)
  if (nlds > 0) {
    if (bf16)
      hipLaunchKernelGGL(k_dw_big16, dim3(nlds), dim3(kDwThreads), 0, st, jobs, item_job, item_split);
    else if (big_waves == 8)
      hipLaunchKernelGGL(k_dw_big8<>, dim3(nlds), dim3(kDwBig8Threads), 0, st, jobs, item_job, item_split);
    else
      hipLaunchKernelGGL(k_dw_big, dim3(nlds), dim3(kDwThreads), 0, st, jobs, item_job, item_split);
  }
  if (nitems > nlds)
    hipLaunchKernelGGL(thin, dim3(nitems - nlds), dim3(kDwThreads), 0, st, jobs, item_job + nlds, item_split + nlds);
  hipLaunchKernelGGL(k_dw_reduce, dim3(cdiv(max_elems, 256), njobs), dim3(256), 0, st, jobs);
}
}  // namespace spp
