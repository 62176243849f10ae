// Bindings for the BatchNorm kernels (bn.hip): statistics reduce / finalize / apply, the
// backward reduce / coefficients / apply, and the SyncBN dispatch of both directions.
#include "ops_decl.h"
#include "conv_internal.h"
#include "launchers.h"

#include <map>
#include <mutex>
#include <utility>

namespace sdx_bind {

// Ticket counters of the single-launch column reduction: zeroed once per device, reset by
// each launch's last block; consecutive launches rotate through slots so launches on
// different streams never share a counter.
// nslots consecutive slots: one per emulated rank of a fused SyncBN exchange (XgmiCol mode 2)
unsigned* reduce_counters(const torch::Device& dev, int nslots) {
  constexpr int kSlots = 256, kPerSlot = 64;   // 64 column groups = 4096 channels
  TORCH_CHECK(nslots >= 1 && nslots <= kXgmiMaxPeers, "counter slots");
  static std::mutex mu;
  static std::map<int, std::pair<torch::Tensor, int>> pool;
  std::lock_guard<std::mutex> lk(mu);
  auto& e = pool[dev.index()];
  if (!e.first.defined())
    e.first = torch::zeros({kSlots * kPerSlot}, torch::TensorOptions().dtype(at::kInt).device(dev));
  int slot = e.second;
  if (slot + nslots > kSlots) slot = 0;
  e.second = (slot + nslots) % kSlots;
  return reinterpret_cast<unsigned*>(e.first.data_ptr<int>()) + slot * kPerSlot;
}

torch::Tensor reduce_scratch(const torch::Tensor& like, int64_t rows, int64_t nsets, int64_t C, int z) {
  return torch::empty({z * col_reduce_gy((int)rows) * nsets * C}, like.options().dtype(at::kDouble));
}

// the fused SyncBN exchange of one BN (xGMI communicators; csrc/kernels/bn.hip XgmiCol)
FusedX fused_exchange(int64_t comm) {
  FusedX f;
  if (comm != 0) f.on = small_comm_fused(comm, &f.x);
  return f;
}

namespace {

// How one BN's sums cross the ranks of communicator `comm`: not at all (world 1), inside
// the reduction launch (fused xGMI exchange), or by an in-place RCCL all-reduce between the
// reduction and its epilogue. Either way the epilogue sees the global row count, and dγ/dβ
// keep this rank's 1/world share (BnCoefArgs::grad_scale).
struct SyncPlan {
  int world = 1;
  FusedX fx;
  bool rccl() const { return world > 1 && !fx.on; }
  const FusedX* fused() const { return fx.on ? &fx : nullptr; }
};
SyncPlan sync_plan(int64_t comm) {
  SyncPlan p;
  p.world = small_comm_world(comm);
  if (p.world > 1) p.fx = fused_exchange(comm);
  return p;
}

void check_slab(const torch::Tensor& slab, int64_t nsets) {
  TORCH_CHECK(slab.is_cuda() && slab.scalar_type() == at::kFloat && slab.dim() == 3 && slab.size(1) == nsets &&
                  slab.is_contiguous(),
              "slab must be [rows, ", nsets, ", C] float32");
  TORCH_CHECK(slab.size(2) <= 4096, "C <= 4096");
}

torch::Tensor bn_stats_reduce(torch::Tensor slab) {
  check_slab(slab, 2);
  c10::DeviceGuard dg(slab.device());
  const int64_t rows = slab.size(0), C = slab.size(2);
  auto out = torch::empty({2, C}, slab.options().dtype(at::kDouble));
  auto scratch = reduce_scratch(slab, rows, 2, C);
  check_hip(launch_col_reduce(slab.data_ptr<float>(), rows, 2, C, scratch.data_ptr<double>(),
                              reduce_counters(slab.device()), out.data_ptr<double>(), 0, nullptr, nullptr,
                              cur_stream()),
            "bn_stats_reduce");
  return out;
}

struct FinalizeOut {
  torch::Tensor scale, shift, mean, invstd;
};

BnFinalizeArgs finalize_args(const torch::Tensor& like, int64_t C, double count, const OptT& gamma, const OptT& beta,
                             double eps, double momentum, bool update, const OptT& running_mean,
                             const OptT& running_var, FinalizeOut& o) {
  BnFinalizeArgs a{};
  a.count = count;
  a.gamma = opt_ptr(gamma, C, "gamma");
  a.beta = opt_ptr(beta, C, "beta");
  a.eps = (float)eps;
  a.momentum = (float)momentum;
  a.update_running = update ? 1 : 0;
  if (update) {
    TORCH_CHECK(running_mean.has_value() && running_var.has_value(), "running stats required for update");
    check_vec(*running_mean, C, "running_mean");
    check_vec(*running_var, C, "running_var");
    a.running_mean = running_mean->data_ptr<float>();
    a.running_var = running_var->data_ptr<float>();
  }
  auto fo = like.options().dtype(at::kFloat);
  o.scale = torch::empty({C}, fo);
  o.shift = torch::empty({C}, fo);
  o.mean = torch::empty({C}, fo);
  o.invstd = torch::empty({C}, fo);
  a.scale = o.scale.data_ptr<float>();
  a.shift = o.shift.data_ptr<float>();
  a.mean = o.mean.data_ptr<float>();
  a.invstd = o.invstd.data_ptr<float>();
  return a;
}

std::vector<torch::Tensor> bn_finalize(torch::Tensor sums, double count, OptT gamma, OptT beta, double eps,
                                       double momentum, bool update, OptT running_mean, OptT running_var) {
  TORCH_CHECK(sums.is_cuda() && sums.scalar_type() == at::kDouble && sums.dim() == 2 && sums.size(0) == 2 &&
                  sums.is_contiguous(),
              "sums must be [2, C] float64");
  const int64_t C = sums.size(1);
  c10::DeviceGuard dg(sums.device());
  FinalizeOut o;
  const BnFinalizeArgs a =
      finalize_args(sums, C, count, gamma, beta, eps, momentum, update, running_mean, running_var, o);
  check_hip(launch_bn_finalize(sums.data_ptr<double>(), C, a, cur_stream()), "bn_finalize");
  return {o.scale, o.shift, o.mean, o.invstd};
}

// conv stat slab -> (scale, shift, mean, invstd) in ONE launch (no cross-rank reduction)
// fx (fused SyncBN exchange): the sums are exchanged across ranks inside the same launch
// and `count` must be the global row count
std::vector<torch::Tensor> bn_stats_finalize(torch::Tensor slab, double count, OptT gamma, OptT beta, double eps,
                                             double momentum, bool update, OptT running_mean, OptT running_var,
                                             const FusedX* fx = nullptr) {
  check_slab(slab, 2);
  c10::DeviceGuard dg(slab.device());
  const int64_t rows = slab.size(0), C = slab.size(2);
  FinalizeOut o;
  const BnFinalizeArgs a =
      finalize_args(slab, C, count, gamma, beta, eps, momentum, update, running_mean, running_var, o);
  auto sums = torch::empty({2, C}, slab.options().dtype(at::kDouble));
  const int z = fx ? fx->z() : 1;
  auto scratch = reduce_scratch(slab, rows, 2, C, z);
  check_hip(launch_col_reduce(slab.data_ptr<float>(), rows, 2, C, scratch.data_ptr<double>(),
                              reduce_counters(slab.device(), z), sums.data_ptr<double>(), 1, &a, nullptr, cur_stream(),
                              fx ? fx->p() : nullptr),
            "bn_stats_finalize");
  return {o.scale, o.shift, o.mean, o.invstd};
}

std::vector<torch::Tensor> bn_eval_affine(OptT gamma, OptT beta, torch::Tensor rm, torch::Tensor rv, double eps) {
  const int64_t C = rm.numel();
  check_vec(rm, C, "running_mean");
  check_vec(rv, C, "running_var");
  c10::DeviceGuard dg(rm.device());
  auto scale = torch::empty({C}, rm.options()), shift = torch::empty({C}, rm.options());
  check_hip(launch_bn_eval_affine(C, opt_ptr(gamma, C, "gamma"), opt_ptr(beta, C, "beta"), rm.data_ptr<float>(),
                                  rv.data_ptr<float>(), (float)eps, scale.data_ptr<float>(), shift.data_ptr<float>(),
                                  cur_stream()),
            "bn_eval_affine");
  return {scale, shift};
}

}  // namespace

// The SyncBN dispatch of the forward statistics: one launch reduces and finalizes the conv's
// slab (with the fused exchange inside it), or reduce -> RCCL all-reduce of the fp64
// (Σy, Σy²), in place on the compute stream -> finalize.
BnState bn_forward(const torch::Tensor& slab, double count, const torch::Tensor& g, const torch::Tensor& b,
                   const torch::Tensor& rm, const torch::Tensor& rv, double eps, double mom, bool training,
                   int64_t comm) {
  if (!training) {
    auto r = bn_eval_affine(g, b, rm, rv, eps);
    return {r[0], r[1], torch::Tensor(), torch::Tensor()};
  }
  const SyncPlan sp = sync_plan(comm);
  std::vector<torch::Tensor> r;
  if (sp.rccl()) {
    auto sums = bn_stats_reduce(slab);
    small_all_reduce_(comm, sums);
    r = bn_finalize(sums, count * sp.world, g, b, eps, mom, true, rm, rv);
  } else {
    r = bn_stats_finalize(slab, count * sp.world, g, b, eps, mom, true, rm, rv, sp.fused());
    if (sp.fx.on) small_comm_fused_issued(comm);
  }
  return {r[0], r[1], r[2], r[3]};
}

torch::Tensor bn_apply(torch::Tensor y, torch::Tensor scale, torch::Tensor shift, const BnResidual& res, bool relu,
                       OptT mask_out) {
  check_bf16_nhwc(y, "y");
  const int64_t C = y.size(3);
  check_vec(scale, C, "scale");
  check_vec(shift, C, "shift");
  const void* rp = nullptr;
  const float *s2 = nullptr, *t2 = nullptr;
  TORCH_CHECK(res.mode >= 0 && res.mode <= 2, "res_mode");
  if (res.mode != 0) {
    TORCH_CHECK(res.r.has_value(), "residual tensor required");
    check_bf16_nhwc(*res.r, "residual");
    TORCH_CHECK(res.r->sizes() == y.sizes(), "residual shape mismatch");
    rp = res.r->data_ptr();
    if (res.mode == 1) {
      s2 = opt_ptr(res.scale2, C, "scale2");
      t2 = opt_ptr(res.shift2, C, "shift2");
      TORCH_CHECK(s2 && t2, "scale2/shift2 required for res_mode 1");
    }
  }
  c10::DeviceGuard dg(y.device());
  auto out = torch::empty_like(y);
  void* mp = nullptr;
  if (mask_out.has_value()) {
    check_mask(*mask_out, y.numel(), "mask_out");
    mp = mask_out->data_ptr();
  }
  check_hip(launch_bn_apply(y.data_ptr(), scale.data_ptr<float>(), shift.data_ptr<float>(), rp, s2, t2, (int)res.mode,
                            relu ? 1 : 0, out.data_ptr(), y.numel(), C, cur_stream(), mp),
            "bn_apply");
  return out;
}

namespace {

void check_bwd_C(int64_t C) {
  TORCH_CHECK(C <= 2048 && (C & (C - 1)) == 0 && C >= 8, "bn backward supports power-of-two C in [8, 2048]");
}

// the ReLU mask operand of a backward pass: the activation itself or its bitmask
void mask_source(const BnBwdSrc& s, const void** op, const void** om) {
  if (!s.outv.has_value()) return;
  if (s.outv->scalar_type() == at::kByte) {
    check_mask(*s.outv, s.dout.numel(), "out (bitmask)");
    *om = s.outv->data_ptr();
  } else {
    check_bf16_nhwc(*s.outv, "out");
    TORCH_CHECK(s.outv->sizes() == s.dout.sizes(), "out shape");
    *op = s.outv->data_ptr();
  }
}

struct BwdIn {
  const void* op = nullptr;
  const void* om = nullptr;   // ReLU bitmask instead of the activation
  const void* ybp = nullptr;
  const float* map = nullptr;
  const float* mbp = nullptr;
  const float* mk_s = nullptr;
  const float* mk_t = nullptr;
  int64_t C = 0;
  int nsum() const { return ybp ? 3 : 2; }
};

BwdIn bwd_inputs(const BnBwdSrc& s, const BnBwdSet& a, const BnBwdSet& b) {
  BwdIn in;
  check_bf16_nhwc(s.dout, "dout");
  check_bf16_nhwc(s.ya, "ya");
  in.C = s.dout.size(3);
  check_bwd_C(in.C);
  TORCH_CHECK(s.ya.sizes() == s.dout.sizes(), "ya shape");
  check_vec(*a.mean, in.C, "mean_a");
  in.map = a.mean->data_ptr<float>();
  mask_source(s, &in.op, &in.om);
  if (s.yb.has_value()) {
    check_bf16_nhwc(*s.yb, "yb");
    TORCH_CHECK(s.yb->sizes() == s.dout.sizes(), "yb shape");
    TORCH_CHECK(b.mean.has_value(), "mean_b required");
    check_vec(*b.mean, in.C, "mean_b");
    in.ybp = s.yb->data_ptr();
    in.mbp = b.mean->data_ptr<float>();
  }
  in_bn_ptrs(s.msc, s.msh, in.C, &in.mk_s, &in.mk_t);
  return in;
}

// The elementwise backward reduction: [Σdz, Σdz·(ya − μa)(, Σdz·(yb − μb))] as fp64 sums
// [2|3][C] in one launch; ca: the coefficient epilogue in the same launch; fx: the fused
// SyncBN exchange in front of it
torch::Tensor bwd_reduce(const BnBwdSrc& s, const BwdIn& in, const BnCoefArgs* ca, const FusedX* fx, const char* what) {
  const int64_t C = in.C;
  const int nsum = in.nsum();
  const int g = bn_bwd_reduce_blocks(s.dout.numel(), C);
  const int z = fx ? fx->z() : 1;
  auto sums = torch::empty({nsum, C}, s.dout.options().dtype(at::kDouble));
  auto partial = torch::empty({g, nsum, C}, s.dout.options().dtype(at::kFloat));
  auto scratch = reduce_scratch(s.dout, g, nsum, C, z);
  check_hip(launch_bn_bwd_reduce(s.dout.data_ptr(), in.op, s.ya.data_ptr(), in.map, in.ybp, in.mbp, s.dout.numel(), C,
                                 partial.data_ptr<float>(), scratch.data_ptr<double>(),
                                 reduce_counters(s.dout.device(), z), sums.data_ptr<double>(), ca ? 2 : 0, ca,
                                 cur_stream(), in.mk_s, in.mk_t, in.om, fx ? fx->p() : nullptr),
            what);
  return sums;
}

struct CoefOut {
  torch::Tensor coef_a, coef_b, dga, dba, dgb, dbb;
  std::vector<torch::Tensor> list() const { return {coef_a, coef_b, dga, dba, dgb, dbb}; }
};

BnCoefArgs coef_args(const torch::Tensor& like, int64_t C, int nsets, double count, const BnBwdSet& sa,
                     const BnBwdSet& sb, CoefOut& o, double grad_scale) {
  TORCH_CHECK(nsets == 1 || nsets == 2, "1 or 2 BN sets");
  TORCH_CHECK(sa.mean.has_value() && sa.invstd.has_value(), "mean_a/inv_a required");
  check_vec(*sa.mean, C, "mean_a");
  check_vec(*sa.invstd, C, "inv_a");
  auto fo = like.options().dtype(at::kFloat);
  const bool sinks = sa.dgamma_sink.has_value();
  TORCH_CHECK(!sinks || (sa.dbeta_sink.has_value() &&
                         (nsets == 1 || (sb.dgamma_sink.has_value() && sb.dbeta_sink.has_value()))),
              "all gradient sinks must be given together");
  BnCoefArgs a{};
  a.count = count;
  a.accumulate = sinks ? 1 : 0;
  a.grad_scale = grad_scale;
  o.coef_a = torch::empty({3, C}, fo);
  o.dga = sinks ? *sa.dgamma_sink : torch::empty({C}, fo);
  o.dba = sinks ? *sa.dbeta_sink : torch::empty({C}, fo);
  if (sinks) {
    check_vec(o.dga, C, "sink_ga");
    check_vec(o.dba, C, "sink_ba");
  }
  a.g_a = opt_ptr(sa.gamma, C, "g_a");
  a.mean_a = sa.mean->data_ptr<float>();
  a.inv_a = sa.invstd->data_ptr<float>();
  a.coef_a = o.coef_a.data_ptr<float>();
  a.dgamma_a = o.dga.data_ptr<float>();
  a.dbeta_a = o.dba.data_ptr<float>();
  if (nsets == 2) {
    o.coef_b = torch::empty({3, C}, fo);
    o.dgb = sinks ? *sb.dgamma_sink : torch::empty({C}, fo);
    o.dbb = sinks ? *sb.dbeta_sink : torch::empty({C}, fo);
    if (sinks) {
      check_vec(o.dgb, C, "sink_gb");
      check_vec(o.dbb, C, "sink_bb");
    }
    a.g_b = opt_ptr(sb.gamma, C, "g_b");
    a.mean_b = opt_ptr(sb.mean, C, "mean_b");
    a.inv_b = opt_ptr(sb.invstd, C, "inv_b");
    TORCH_CHECK(a.mean_b && a.inv_b, "mean_b/inv_b required");
    a.coef_b = o.coef_b.data_ptr<float>();
    a.dgamma_b = o.dgb.data_ptr<float>();
    a.dbeta_b = o.dbb.data_ptr<float>();
  } else {
    o.coef_b = o.dgb = o.dbb = torch::empty({0}, fo);
  }
  return a;
}

std::vector<torch::Tensor> bn_bwd_coef(torch::Tensor sums, double count, const BnBwdSet& sa, const BnBwdSet& sb,
                                       double grad_scale) {
  TORCH_CHECK(sums.is_cuda() && sums.scalar_type() == at::kDouble && sums.dim() == 2 && sums.is_contiguous(),
              "sums must be [nsets+1, C] float64");
  const int64_t C = sums.size(1);
  const int nsets = (int)sums.size(0) - 1;
  c10::DeviceGuard dg(sums.device());
  CoefOut o;
  const BnCoefArgs a = coef_args(sums, C, nsets, count, sa, sb, o, grad_scale);
  check_hip(launch_bn_bwd_coef(sums.data_ptr<double>(), nsets, C, a, cur_stream()), "bn_bwd_coef");
  return o.list();
}

}  // namespace

// The SyncBN dispatch of the backward coefficients. Without RCCL in between, the reduction's
// last block evaluates the coefficients in the same launch (after the fused exchange, if
// any); with it: reduce -> in-place all-reduce of the sums -> coefficients.
std::vector<torch::Tensor> bn_bwd_coefs(int64_t comm, const BnBwdSrc* src, const torch::Tensor* slab, double count,
                                        const BnBwdSet& sa, const BnBwdSet& sb) {
  TORCH_CHECK((src != nullptr) != (slab != nullptr), "bn_bwd_coefs: one statistics source");
  BwdIn in;
  int64_t rows = 0, nsum, C;
  if (src) {
    in = bwd_inputs(*src, sa, sb);
    nsum = in.nsum();
    C = in.C;
  } else {
    TORCH_CHECK(slab->dim() == 3 && (slab->size(1) == 2 || slab->size(1) == 3), "slab: [rows][2|3][C]");
    check_slab(*slab, slab->size(1));
    rows = slab->size(0); nsum = slab->size(1); C = slab->size(2);
  }
  const torch::Tensor& like = src ? src->dout : *slab;
  c10::DeviceGuard dg(like.device());
  torch::Tensor sums, scratch;
  if (slab) sums = torch::empty({nsum, C}, like.options().dtype(at::kDouble));
  const SyncPlan sp = sync_plan(comm);
  // the slab's column reduction (its scratch comes before the coefficient tensors unless the
  // exchange is fused: the allocation order is part of the step's memory behaviour)
  if (slab && !sp.fx.on) scratch = reduce_scratch(like, rows, nsum, C);
  auto slab_reduce = [&](const BnCoefArgs* ca) {
    if (!scratch.defined()) scratch = reduce_scratch(like, rows, nsum, C, sp.fx.z());
    check_hip(launch_col_reduce(slab->data_ptr<float>(), rows, (int)nsum, C, scratch.data_ptr<double>(),
                                reduce_counters(like.device(), sp.fx.z()), sums.data_ptr<double>(), ca ? 2 : 0,
                                nullptr, ca, cur_stream(), sp.fx.p()),
              "bn_bwd_coef_slab");
  };
  if (sp.rccl()) {
    if (src) sums = bwd_reduce(*src, in, nullptr, nullptr, "bn_bwd_reduce");
    else slab_reduce(nullptr);
    small_all_reduce_(comm, sums);
    return bn_bwd_coef(sums, count * sp.world, sa, sb, 1.0 / sp.world);
  }
  CoefOut o;
  const BnCoefArgs a = coef_args(like, C, (int)nsum - 1, count * sp.world, sa, sb, o, 1.0 / sp.world);
  if (src) bwd_reduce(*src, in, &a, sp.fused(), "bn_bwd_reduce_coef");
  else slab_reduce(&a);
  if (sp.fx.on) small_comm_fused_issued(comm);
  return o.list();
}

std::vector<torch::Tensor> bn_bwd_apply(const BnBwdSrc& s, torch::Tensor ca, OptT cb, bool want_dz) {
  const torch::Tensor& dout = s.dout;
  check_bf16_nhwc(dout, "dout");
  check_bf16_nhwc(s.ya, "ya");
  const int64_t C = dout.size(3);
  TORCH_CHECK(s.ya.sizes() == dout.sizes(), "ya shape");
  TORCH_CHECK(ca.is_cuda() && ca.scalar_type() == at::kFloat && ca.numel() == 3 * C && ca.is_contiguous(), "coef_a");
  const void* op = nullptr;
  const void* om = nullptr;
  mask_source(s, &op, &om);
  c10::DeviceGuard dg(dout.device());
  auto dya = torch::empty_like(dout);
  torch::Tensor dyb, dz;
  const void* ybp = nullptr;
  const float* cbp = nullptr;
  if (s.yb.has_value()) {
    check_bf16_nhwc(*s.yb, "yb");
    TORCH_CHECK(s.yb->sizes() == dout.sizes(), "yb shape");
    TORCH_CHECK(cb.has_value() && cb->numel() == 3 * C && cb->scalar_type() == at::kFloat, "coef_b");
    ybp = s.yb->data_ptr();
    cbp = cb->data_ptr<float>();
    dyb = torch::empty_like(dout);
  } else {
    dyb = torch::empty({0}, dout.options());
  }
  const float *mk_s, *mk_t;
  in_bn_ptrs(s.msc, s.msh, C, &mk_s, &mk_t);
  dz = want_dz ? torch::empty_like(dout) : torch::empty({0}, dout.options());
  check_hip(launch_bn_bwd_apply(dout.data_ptr(), op, s.ya.data_ptr(), ca.data_ptr<float>(), ybp, cbp, dya.data_ptr(),
                                ybp ? dyb.data_ptr() : nullptr, want_dz ? dz.data_ptr() : nullptr, dout.numel(), C,
                                cur_stream(), mk_s, mk_t, om),
            "bn_bwd_apply");
  return {dya, dyb, dz};
}

namespace {

// Column reduction + cross-rank exchange of a statistics slab in ONE launch (the fused
// SyncBN path without an epilogue): tests, the start-up self-check of an xGMI communicator
// and the per-BN latency probe (tools/syncbn_latency.py). Real communicator: slab
// [rows][nsets][C] -> global sums [nsets][C]. Emulated (XEMU): slab [W][rows][nsets][C],
// virtual rank z reduces slab[z], or [rows][nsets][C] shared by identical ranks; rank 0's
// global sums are returned.
torch::Tensor syncbn_exchange_sums(int64_t comm, torch::Tensor slab) {
  FusedX fx = fused_exchange(comm);
  TORCH_CHECK(fx.on, "syncbn_exchange_sums: not a fused (xGMI) communicator of > 1 ranks");
  TORCH_CHECK(slab.is_cuda() && slab.scalar_type() == at::kFloat && slab.is_contiguous(), "slab: contiguous fp32");
  const bool emu = fx.x.mode == 2;
  // emulated ranks: [W][rows][nsets][C] (rank z reduces slab[z]) or [rows][nsets][C] (identical ranks)
  TORCH_CHECK(slab.dim() == 3 || (emu && slab.dim() == 4), "slab: [rows][nsets][C]",
              emu ? " or [W][rows][nsets][C]" : "");
  if (slab.dim() == 4) TORCH_CHECK(slab.size(0) == fx.x.world, "slab: one block per emulated rank");
  const int64_t rows = slab.size(-3), nsets = slab.size(-2), C = slab.size(-1);
  TORCH_CHECK(nsets >= 1 && nsets <= 3 && C >= 1 && C <= 4096 && rows >= 1, "slab shape");
  if (slab.dim() == 4) fx.x.slab_zstride = (long)(rows * nsets * C);
  c10::DeviceGuard dg(slab.device());
  auto sums = torch::empty({nsets, C}, slab.options().dtype(at::kDouble));
  auto scratch = reduce_scratch(slab, rows, nsets, C, fx.z());
  check_hip(launch_col_reduce(slab.data_ptr<float>(), (int)rows, (int)nsets, (int)C, scratch.data_ptr<double>(),
                              reduce_counters(slab.device(), fx.z()), sums.data_ptr<double>(), 0, nullptr, nullptr,
                              cur_stream(), fx.p()),
            "syncbn_exchange_sums");
  small_comm_fused_issued(comm);
  return sums;
}

}  // namespace

// the Python-visible ops: positional arguments packed into the operand sets above
void register_bn(pybind11::module& m) {
  using T = torch::Tensor;
  m.def("syncbn_exchange_sums", &syncbn_exchange_sums,
        "column reduction + cross-rank exchange of a BN statistics slab in one launch (fused xGMI communicators)");
  m.def("bn_stats_reduce", &bn_stats_reduce);
  m.def("bn_finalize", &bn_finalize);
  m.def("bn_stats_finalize",
        [](T slab, double count, OptT gamma, OptT beta, double eps, double momentum, bool update, OptT running_mean,
           OptT running_var) {
          return bn_stats_finalize(slab, count, gamma, beta, eps, momentum, update, running_mean, running_var);
        },
        "conv stat slab -> BN affine in one launch");
  m.def("bn_eval_affine", &bn_eval_affine);
  m.def("bn_apply",
        [](T y, T scale, T shift, OptT r, OptT scale2, OptT shift2, int64_t res_mode, bool relu, OptT mask_out) {
          return bn_apply(y, scale, shift, BnResidual{r, scale2, shift2, res_mode}, relu, mask_out);
        },
        pybind11::arg("y"), pybind11::arg("scale"), pybind11::arg("shift"),
        pybind11::arg("r") = pybind11::none(), pybind11::arg("scale2") = pybind11::none(),
        pybind11::arg("shift2") = pybind11::none(), pybind11::arg("res_mode") = 0, pybind11::arg("relu") = true,
        pybind11::arg("mask_out") = pybind11::none());
  m.def("bn_bwd_reduce",
        [](T dout, OptT outv, T ya, T ma, OptT yb, OptT mb, OptT msc, OptT msh) {
          const BnBwdSrc s{dout, outv, ya, yb, msc, msh};
          BnBwdSet a, b;
          a.mean = ma;
          b.mean = mb;
          const BwdIn in = bwd_inputs(s, a, b);
          c10::DeviceGuard dg(dout.device());
          return bwd_reduce(s, in, nullptr, nullptr, "bn_bwd_reduce");
        },
        pybind11::arg("dout"), pybind11::arg("outv"), pybind11::arg("ya"),
        pybind11::arg("ma"), pybind11::arg("yb") = pybind11::none(), pybind11::arg("mb") = pybind11::none(),
        pybind11::arg("msc") = pybind11::none(), pybind11::arg("msh") = pybind11::none());
  m.def("bn_bwd_coef",
        [](T sums, double count, OptT g_a, T mean_a, T inv_a, OptT g_b, OptT mean_b, OptT inv_b, OptT sink_ga,
           OptT sink_ba, OptT sink_gb, OptT sink_bb, double grad_scale) {
          return bn_bwd_coef(sums, count, {g_a, mean_a, inv_a, sink_ga, sink_ba}, {g_b, mean_b, inv_b, sink_gb, sink_bb},
                             grad_scale);
        },
        pybind11::arg("sums"), pybind11::arg("count"), pybind11::arg("g_a"),
        pybind11::arg("mean_a"), pybind11::arg("inv_a"), pybind11::arg("g_b") = pybind11::none(),
        pybind11::arg("mean_b") = pybind11::none(), pybind11::arg("inv_b") = pybind11::none(),
        pybind11::arg("sink_ga") = pybind11::none(), pybind11::arg("sink_ba") = pybind11::none(),
        pybind11::arg("sink_gb") = pybind11::none(), pybind11::arg("sink_bb") = pybind11::none(),
        pybind11::arg("grad_scale") = 1.0);
  // bn_bwd_reduce + bn_bwd_coef in one elementwise launch + one reduction launch
  m.def("bn_bwd_reduce_coef",
        [](T dout, OptT outv, T ya, T ma, OptT yb, OptT mb, OptT msc, OptT msh, double count, OptT g_a, T inv_a,
           OptT g_b, OptT inv_b, OptT sink_ga, OptT sink_ba, OptT sink_gb, OptT sink_bb) {
          const BnBwdSrc s{dout, outv, ya, yb, msc, msh};
          return bn_bwd_coefs(0, &s, nullptr, count, {g_a, ma, inv_a, sink_ga, sink_ba},
                              {g_b, mb, inv_b, sink_gb, sink_bb});
        },
        pybind11::arg("dout"), pybind11::arg("outv"),
        pybind11::arg("ya"), pybind11::arg("ma"), pybind11::arg("yb") = pybind11::none(),
        pybind11::arg("mb") = pybind11::none(), pybind11::arg("msc") = pybind11::none(),
        pybind11::arg("msh") = pybind11::none(), pybind11::arg("count") = 1.0, pybind11::arg("g_a") = pybind11::none(),
        pybind11::arg("inv_a") = pybind11::none(), pybind11::arg("g_b") = pybind11::none(),
        pybind11::arg("inv_b") = pybind11::none(), pybind11::arg("sink_ga") = pybind11::none(),
        pybind11::arg("sink_ba") = pybind11::none(), pybind11::arg("sink_gb") = pybind11::none(),
        pybind11::arg("sink_bb") = pybind11::none());
  m.def("bn_bwd_coef_slab",
        [](int64_t comm, T slab, double count, OptT g_a, T mean_a, T inv_a, OptT g_b, OptT mean_b, OptT inv_b,
           OptT sink_ga, OptT sink_ba, OptT sink_gb, OptT sink_bb) {
          return bn_bwd_coefs(comm, nullptr, &slab, count, {g_a, mean_a, inv_a, sink_ga, sink_ba},
                              {g_b, mean_b, inv_b, sink_gb, sink_bb});
        },
        "BN-backward coefficients (+dγ/dβ into sinks) from a dgrad stat slab",
        pybind11::arg("comm"), pybind11::arg("slab"), pybind11::arg("count"), pybind11::arg("g_a"),
        pybind11::arg("mean_a"), pybind11::arg("inv_a"), pybind11::arg("g_b") = pybind11::none(),
        pybind11::arg("mean_b") = pybind11::none(), pybind11::arg("inv_b") = pybind11::none(),
        pybind11::arg("sink_ga") = pybind11::none(), pybind11::arg("sink_ba") = pybind11::none(),
        pybind11::arg("sink_gb") = pybind11::none(), pybind11::arg("sink_bb") = pybind11::none());
  m.def("bn_bwd_apply",
        [](T dout, OptT outv, T ya, T ca, OptT yb, OptT cb, bool want_dz, OptT msc, OptT msh) {
          return bn_bwd_apply(BnBwdSrc{dout, outv, ya, yb, msc, msh}, ca, cb, want_dz);
        },
        pybind11::arg("dout"), pybind11::arg("outv"), pybind11::arg("ya"),
        pybind11::arg("ca"), pybind11::arg("yb") = pybind11::none(), pybind11::arg("cb") = pybind11::none(),
        pybind11::arg("want_dz") = false, pybind11::arg("msc") = pybind11::none(),
        pybind11::arg("msh") = pybind11::none());
}

}  // namespace sdx_bind
