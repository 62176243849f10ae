// The generic weight-gradient instantiations of the implicit-GEMM kernel:
// igemm_kernel.h, launched by igemm.hip.
#include "igemm_kernel.h"

hipError_t igemm_launch_wgrad(const void* params, int cfg, hipStream_t s) {
  return launch_any<MODE_WGRAD>(params_from(params), cfg, s);
}
hipError_t igemm_trace_copy_wgrad(unsigned long long* host) { return trace_copy_unit(host); }
