// Internal interface of the conv/BN binding layer: conv_ops.cpp (convolutions, knobs),
// bn_ops.cpp (BatchNorm, SyncBN dispatch), block_ops.cpp (residual-block executor, BN3 fold),
// side_stream.cpp (side-stream fork) and head_ops.cpp (the projection head as 1x1 GEMMs on
// the same kernels). The Python-visible ops are positional adapters over these functions.
#pragma once
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>

#include <initializer_list>
#include <vector>

#include "launchers.h"

namespace sdx_bind {
using OptT = c10::optional<torch::Tensor>;

// ---- checks ---------------------------------------------------------------------------
void check_bf16_nhwc(const torch::Tensor& t, const char* name);
void check_vec(const torch::Tensor& t, int64_t C, const char* name);
const float* opt_ptr(const OptT& t, int64_t C, const char* name);
// fused BN+ReLU input prologue / recomputed ReLU mask: both vectors or neither
void in_bn_ptrs(const OptT& sc, const OptT& sh, int64_t C, const float** ps, const float** pt);
// ReLU bitmask of an activation: uint8 [numel/8], bit i of byte e = value 8e+i > 0
void check_mask(const torch::Tensor& m, int64_t numel, const char* name);

// ---- geometry -------------------------------------------------------------------------
// forward direction: output P x Q derived from the input, filter, stride and pad
ConvGeom conv_geom(int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t R, int64_t S, int64_t stride,
                   int64_t pad);
ConvGeom fwd_geom(const torch::Tensor& x, const torch::Tensor& w, int64_t stride, int64_t pad);
// backward direction: dy [N,P,Q,K], wt [C,R,S,K(+cat)], input H x W given
ConvGeom dgrad_geom(const torch::Tensor& dy, const torch::Tensor& wt, int64_t H, int64_t W, int64_t stride,
                    int64_t pad);
// tile config for an M x Ncol GEMM with reduction Kdim (fill: charge idle CUs of the last round)
int auto_cfg(int64_t M, int64_t Ncol, int64_t Kdim = 0, bool fill = false);

// ---- convolutions (conv_ops.cpp) ------------------------------------------------------
// returns [y, statistics slab]. epi: GEMM epilogue; no_out: statistics only, the output is
// not stored (first pass of a forward-folded BN3)
std::vector<torch::Tensor> conv_fwd(torch::Tensor x, torch::Tensor w, int64_t stride, int64_t pad, bool want_stats,
                                    int64_t cfg, OptT in_scale, OptT in_shift, const GemmEpi* epi = nullptr,
                                    bool no_out = false);
// What a data gradient does besides dx = dy * wt: where dx goes, what is added to it, and
// the two BN3-fold modes of a stride-1 1x1 dgrad (block_ops.cpp).
struct DgradOpts {
  OptT out, addend, addend_mask;
  int64_t addend_sub = 0;             // > 1: compact addend on the stride-s subgrid
  bool add_pre = false;               // the addend joins the fp32 accumulators before the bf16 rounding
  // K-concatenated dgrad (igemm.hip): the reduction runs over [dy | cat] with
  // wt = [Wd | Mx] ([C][1][1][K + K2]) and adds the fp32 bias before rounding —
  // da2 = dz·Wd + a2·Mx + b in one GEMM
  const torch::Tensor* cat = nullptr;
  const torch::Tensor* cat_bias = nullptr;
};
// fused BN-backward statistics of dx for the BN whose pre-BN tensor is ya (and yb, a second
// BN fed by the same gradient: projection shortcut). ReLU mask from `mask_bits` (1 bit per
// element) or recomputed as ya·msc + msh > 0. An empty ya: the BN input was never stored
// (forward-folded BN3) and the caller fills extra_rows rows of the slab.
struct DgradStat {
  torch::Tensor ya, ma;
  OptT yb, mb, mask_bits, msc, msh;
  int store_masked = 0;
  int64_t extra_rows = 0;
};
torch::Tensor conv_dgrad(torch::Tensor dy, torch::Tensor wt, int64_t H, int64_t W, int64_t stride, int64_t pad,
                         int64_t cfg, const DgradOpts& o = {});
// returns [dx, slab [rows][2|3][C]]
std::vector<torch::Tensor> conv_dgrad_bnstat(torch::Tensor dy, torch::Tensor wt, int64_t H, int64_t W,
                                             int64_t stride, int64_t pad, int64_t cfg, const DgradOpts& o,
                                             const DgradStat& st);
// dW (+)= wgrad(dy, x) (fp32, KRSC), split-K slab reduced deterministically
torch::Tensor conv_wgrad(torch::Tensor dy, torch::Tensor x, int64_t R, int64_t S, int64_t stride, int64_t pad,
                         int64_t splits, int64_t cfg, OptT out, bool accumulate, OptT in_scale, OptT in_shift);
bool splitk_merge_enabled();

// ---- BatchNorm (bn_ops.cpp) -----------------------------------------------------------
// ticket counters + fp64 scratch of the single-launch column reduction (bn.hip col_reduce)
// (nslots / z: one block per emulated rank of a fused SyncBN exchange, XgmiCol mode 2)
unsigned* reduce_counters(const torch::Device& dev, int nslots = 1);
torch::Tensor reduce_scratch(const torch::Tensor& like, int64_t rows, int64_t nsets, int64_t C, int z = 1);
// the fused SyncBN exchange of one BN on communicator `comm` (off: reduce -> all-reduce -> epilogue)
struct FusedX {
  XgmiCol x{};
  bool on = false;
  int z() const { return on && x.mode == 2 && !x.solo ? x.world : 1; }
  const XgmiCol* p() const { return on ? &x : nullptr; }
};
FusedX fused_exchange(int64_t comm);

struct BnState {   // per-BN forward results kept for backward
  torch::Tensor sc, sh, mu, iv;
};
// Forward statistics of one BN from a conv's slab. comm: small-communicator handle
// (comm_ops.cpp); 0 = this process's statistics only, else SyncBN over its ranks.
BnState bn_forward(const torch::Tensor& slab, double count, const torch::Tensor& g, const torch::Tensor& b,
                   const torch::Tensor& rm, const torch::Tensor& rv, double eps, double mom, bool training,
                   int64_t comm);
// residual input of bn_apply: mode 0 none, 1 r·scale2 + shift2, 2 r as it is
struct BnResidual {
  OptT r, scale2, shift2;
  int64_t mode = 0;
};
torch::Tensor bn_apply(torch::Tensor y, torch::Tensor scale, torch::Tensor shift, const BnResidual& res, bool relu,
                       OptT mask_out);
// One BN's backward operands. dγ/dβ go to freshly allocated tensors, or are ADDED into the
// gradient sinks (the parameters' .grad views); all sinks of a call are given together.
struct BnBwdSet {
  OptT gamma, mean, invstd, dgamma_sink, dbeta_sink;
};
// The elementwise backward source: dz = dout·[ReLU mask], read with the pre-BN tensor ya
// (and yb of a second BN fed by the same gradient). Mask: from the stored activation or
// its bitmask `outv`, or (outv None, msc/msh given) recomputed as ya·msc + msh > 0.
struct BnBwdSrc {
  torch::Tensor dout;
  OptT outv;
  torch::Tensor ya;
  OptT yb, msc, msh;
};
// BN-backward coefficients [coef_a, coef_b, dga, dba, dgb, dbb] of one or two BNs, from the
// elementwise source `src` or from a fused-dgrad statistics slab [rows][2|3][C] (exactly one
// of the two), SyncBN over `comm` (0: local)
std::vector<torch::Tensor> bn_bwd_coefs(int64_t comm, const BnBwdSrc* src, const torch::Tensor* slab, double count,
                                        const BnBwdSet& a, const BnBwdSet& b = {});
// returns [dya, dyb, dz]
std::vector<torch::Tensor> bn_bwd_apply(const BnBwdSrc& s, torch::Tensor ca, OptT cb, bool want_dz);

// ---- side stream (side_stream.cpp) ----------------------------------------------------
// tensors read by side-stream work, released after the join (no recordStream: blocks
// return to the allocator in program order instead of behind side-stream events)
std::vector<torch::Tensor>& side_stash();
// an event of the pool recorded on the current stream / the current stream waits for one
hipEvent_t stream_mark();
void stream_wait(hipEvent_t ev);
// Fork: the side stream (a hipStream_t handle, not 0) waits for everything queued on the
// current stream so far, `keep` stays alive until the join, and the returned guard makes
// the side stream current for its lifetime.
c10::hip::HIPStreamGuard side_fork(int64_t side, const torch::Device& dev, std::initializer_list<torch::Tensor> keep);
}  // namespace sdx_bind
