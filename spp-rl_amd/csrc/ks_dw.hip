// Weight-gradient GEMMs (dw.hip) in their own translation unit: the operand-type x tile-shape
// instantiations of k_dw compile in parallel with the phase-kernel sets.
#include "dw.hip"

namespace spp {
void launch_dw_kernels(const DwJob* jobs, const int* item_job, const int* item_split, int nitems, int nlds, int nthin,
                       int njobs, int64_t max_elems, bool bf16, int big_waves, hipStream_t st) {
  const auto rest = bf16 ? k_dw<true> : k_dw<false>;  // named before k_dw_big8<> (dw.hip: the order of emission)
  if (nlds > 0) {
    if (bf16)
      hipLaunchKernelGGL(k_dw_big16, dim3(nlds), dim3(kDwThreads), 0, st, jobs, item_job, item_split);
    else if (big_waves == 8)
      hipLaunchKernelGGL(k_dw_big8<>, dim3(nlds), dim3(kDwBig8Threads), 0, st, jobs, item_job, item_split);
    else
      hipLaunchKernelGGL(k_dw_big, dim3(nlds), dim3(kDwThreads), 0, st, jobs, item_job, item_split);
  }
  // the thin run is the table's tail (plan_dw), a workgroup per item part; k_dw takes what lies between
  if (nthin > 0)
    hipLaunchKernelGGL(k_dw_thin<>, dim3(nthin * (kDwThinSplit ? 2 : 1)), dim3(kDwThinThreads), 0, st, jobs,
                       item_job + (nitems - nthin), item_split + (nitems - nthin));
  if (nitems - nthin > nlds)
    hipLaunchKernelGGL(rest, dim3(nitems - nthin - nlds), dim3(kDwThreads), 0, st, jobs, item_job + nlds,
                       item_split + nlds);
  hipLaunchKernelGGL(k_dw_reduce, dim3(cdiv(max_elems, 256), njobs), dim3(256), 0, st, jobs);
}
}  // namespace spp
