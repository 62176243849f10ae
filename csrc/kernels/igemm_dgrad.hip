// The data-gradient instantiations of the implicit-GEMM kernel (tile configs 0-6; tap reuse: igemm_tap.hip):
// igemm_kernel.h, launched by igemm.hip.
#include "igemm_kernel.h"

hipError_t igemm_launch_dgrad(const void* params, int cfg, hipStream_t s) {
  return launch_any<MODE_DGRAD>(params_from(params), cfg, s);
}
hipError_t igemm_trace_copy_dgrad(unsigned long long* host) { return trace_copy_unit(host); }
