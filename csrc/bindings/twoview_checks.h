// Argument checks that the ops of the two-view pretraining losses share (barlow_ops.cpp,
// vicreg_ops.cpp). `family` is the op family's name in the messages.
#pragma once
#include "conv_internal.h"
#include "loss_gemm_plan.h"

namespace sdx_bind {

inline void check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), name,
              " must be a contiguous fp32 GPU tensor");
}

// -> (n, D) of the two views
inline std::pair<int64_t, int64_t> check_views(const char* family, const torch::Tensor& z1, const torch::Tensor& z2,
                                               double n_total) {
  namespace lg = sdx_lossgemm;
  check_f32(z1, "z1");
  check_f32(z2, "z2");
  TORCH_CHECK(z1.dim() == 2 && z1.sizes() == z2.sizes() && z1.device() == z2.device(), family,
              ": z1 and z2 must be [N][D] tensors of equal shape on one device");
  const int64_t n = z1.size(0), D = z1.size(1);
  TORCH_CHECK(D % 64 == 0 && D >= lg::kMinD && D <= lg::kMaxD, family, ": D = 64·j with 64 <= D <= ", lg::kMaxD);
  TORCH_CHECK(n >= 1 && n_total >= 2 && n_total >= (double)n && n_total < (double)(1 << 24), family,
              ": N >= 2 rows (at least this rank's)");
  TORCH_CHECK(lg::supported(n, D), family, ": sizes");   // both plans' supported()
  return {n, D};
}

inline void check_vec(const torch::Tensor& t, int64_t elems, const torch::Tensor& like, const char* name) {
  check_f32(t, name);
  TORCH_CHECK(t.numel() == elems && t.device() == like.device(), name, ": ", elems, " fp32 elements on the views' device");
}

// g: the upstream scalar gradient, a GPU tensor of one element
inline void check_g(const torch::Tensor& g, const torch::Tensor& like) {
  check_f32(g, "g");
  TORCH_CHECK(g.numel() == 1 && g.device() == like.device(), "g: one fp32 element on the views' device");
}

// the batch size N of the formulas: n_total, or this rank's rows when it is 0
inline double total(const torch::Tensor& z1, int64_t n_total) { return n_total > 0 ? (double)n_total : (double)z1.size(0); }

}  // namespace sdx_bind
