// The tap-reuse 3x3 instantiations (tile configs 11-13, launch_tap) of the implicit-GEMM kernel,
// forward and stride-1 data gradient: igemm_kernel.h, launched by igemm.hip.
#include "igemm_kernel.h"

hipError_t igemm_launch_tap(int mode, const void* params, int cfg, hipStream_t s) {
  if (mode == MODE_FWD) return launch_any_tap<MODE_FWD>(params_from(params), cfg, s);
  if (mode == MODE_DGRAD) return launch_any_tap<MODE_DGRAD>(params_from(params), cfg, s);
  return hipErrorInvalidValue;
}
hipError_t igemm_trace_copy_tap(unsigned long long* host) { return trace_copy_unit(host); }
