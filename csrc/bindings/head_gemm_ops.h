// The projection head's GEMM stages on the igemm MFMA kernels (head_ops.cpp), shared by the
// MLP / linear head and the BatchNorm head (head_bn_ops.cpp).
#pragma once
#include "conv_internal.h"

namespace sdx_bind {
void check_2d(const torch::Tensor& t, at::ScalarType dt, const char* name);
// a cached constant fp32 vector of n elements on dev
const torch::Tensor& const_vec(const torch::Device& dev, int64_t n, float v);
// y[rows][out] = x[rows][in] · W[out][in]ᵀ + bias (ReLU); bf16 or fp32 output
torch::Tensor gemm_fwd(const torch::Tensor& x, const torch::Tensor& w, const torch::Tensor& bias, bool relu,
                       bool out_f32);
torch::Tensor to_bf16(const torch::Tensor& x);
// sink[c] += Σ_rows slab[rows][nsets][C] set 0
void colsum_into(const torch::Tensor& slab, int64_t rows, int nsets, int64_t C, torch::Tensor& sink);
// dW (+)= dyᵀ·x into an fp32 [out][in] sink
void gemm_wgrad(const torch::Tensor& dy, const torch::Tensor& x, torch::Tensor& sink);
// dx[rows][in] = dy[rows][out] · Wt[in][out]ᵀ, optionally ReLU-masked (head_ops.cpp)
torch::Tensor gemm_dgrad(const torch::Tensor& dy, const torch::Tensor& wt, int64_t in, bool out_f32,
                         const torch::Tensor* relu_ref, torch::Tensor* bias_sink, torch::Tensor* slab_out = nullptr);
}  // namespace sdx_bind
