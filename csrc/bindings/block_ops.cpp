// Native residual-block executor: the whole forward / backward kernel sequence of a
// Bottleneck or BasicBlock (reference math: networks/resnet_big.py:7-67) in ONE host
// call, so the per-kernel Python + binding overhead (≈15-25 µs per launch, measured)
// leaves the training step. SyncBN statistics go through a native small communicator
// (comm_ops.cpp: a dedicated RCCL communicator or a one-shot xGMI arena) called in place
// on the compute stream — no Python or c10d work queue between a BN's reduction and its
// finalize. Weight gradients run on the caller's side stream (side_stream.cpp: fork by
// event, operands stashed until the join).
#include "ops_decl.h"
#include "conv_internal.h"
#include "launchers.h"

namespace sdx_bind {
namespace {

using sdx_plan::knobs;

// The tensor list block_fwd returns and block_bwd takes back as `saved` + `bnst`
// (ops/block.py): eight slots, then kBnStride tensors per BN in the order bn1, bn2, (bn3),
// (shortcut bn). Slot 0 is the block output in the result and the block input x in `saved`.
enum BlockSlot { kOut = 0, kX = 0, kY1, kA1, kY2, kA2, kY3, kYs, kMask, kSlots };
enum BnSlot { kSc = 0, kSh, kMu, kIv, kBnStride };

double rows_of(const torch::Tensor& y) { return (double)(y.numel() / y.size(3)); }

bool sub_addend_enabled() {
  static const bool on = sdx_plan::env_flag("SDX_SUB_ADDEND", true);
  return on;
}

bool dgrad_bnstat_enabled() {
  static const bool on = sdx_plan::env_flag("SDX_DGRAD_BNSTAT", true);
  return on;
}

DgradOpts into(OptT out, OptT addend, OptT addend_mask = {}, int64_t addend_sub = 0) {
  DgradOpts o;
  o.out = out; o.addend = addend; o.addend_mask = addend_mask; o.addend_sub = addend_sub;
  return o;
}

// dW (+)= wgrad(dy, x) into the parameter's gradient sink, on the side stream if given
void side_wgrad(const torch::Tensor& dy, const torch::Tensor& x, int64_t R, int64_t S, int64_t stride, int64_t pad,
                const torch::Tensor& sink, int64_t side) {
  if (side == 0) {
    conv_wgrad(dy, x, R, S, stride, pad, 0, -1, sink, true, c10::nullopt, c10::nullopt);
    return;
  }
  // dy / x stay alive until the side stream is joined (ops/streams.py join -> side_stash_release)
  auto guard = side_fork(side, dy.device(), {dy, x});
  // the reduction into the parameter sink joins the block's one multi-tensor launch
  // (block_bwd flushes it before returning, i.e. before the sinks are announced final)
  if (splitk_merge_enabled() && !splitk_deferring(cur_stream())) splitk_defer_begin(cur_stream());
  conv_wgrad(dy, x, R, S, stride, pad, 0, -1, sink, true, c10::nullopt, c10::nullopt);
}

// BN3 fold (bnfold.hip): dW3 (+)= diag(A)·G + diag(D)·W3·S + E ⊗ Σa2 with G = dzᵀ·a2 and
// S = a2ᵀ·a2 (two 1x1 wgrad GEMMs) — on the side stream after the coefficients are known
// S = a2ᵀ·a2 [K][1][1][K] and cs = Σ_rows a2 [K] (fp32) on the current stream
std::vector<torch::Tensor> fold_gram_now(const torch::Tensor& a2) {
  const int64_t K3 = a2.size(3);
  auto opt = a2.options().dtype(at::kFloat);
  auto Sm = torch::empty({K3, 1, 1, K3}, opt);
  conv_wgrad(a2, a2, 1, 1, 1, 0, 0, -1, Sm, false, c10::nullopt, c10::nullopt);
  auto part = torch::empty({bnfold_colsum_blocks(), K3}, opt);
  auto cs = torch::empty({K3}, opt);
  check_hip(launch_bnfold_colsum(a2.data_ptr(), a2.numel() / K3, (int)K3, part.data_ptr<float>(), cs.data_ptr<float>(),
                                 cur_stream()),
            "bnfold_colsum");
  return {Sm, cs, part};
}

// the Gram of a folded conv's input, issued at forward time on the (then idle) side stream;
// backward consumes it on the same stream (FIFO), so no further synchronisation is needed
std::vector<torch::Tensor> fold_gram(torch::Tensor a2, int64_t side) {
  check_bf16_nhwc(a2, "a2");
  if (side == 0) return fold_gram_now(a2);
  auto guard = side_fork(side, a2.device(), {a2});
  return fold_gram_now(a2);
}

// Gpre: G = dzᵀ·a2 already computed on the main stream (forward-folded BN3, whose backward
// statistics need it first)
void side_fold_wgrad(const torch::Tensor& dz, const torch::Tensor& a2, const torch::Tensor& w3,
                     const torch::Tensor& coef, const torch::Tensor& sink, int64_t side,
                     const torch::Tensor* gram = nullptr, const torch::Tensor* Gpre = nullptr) {
  // its own split-K reductions (G, S) are read right after by bnfold_wgrad: issue any queued
  // sink reductions first and keep this call's undeferred
  if (side != 0 && splitk_deferring(reinterpret_cast<hipStream_t>(side))) check_hip(splitk_flush(), "splitk_flush");
  const int64_t C3 = dz.size(3), K3 = a2.size(3);
  auto body = [&]() {
    auto opt = coef.options();
    torch::Tensor G;
    if (Gpre != nullptr) {
      G = *Gpre;
    } else {
      G = torch::empty({C3, 1, 1, K3}, opt);
      conv_wgrad(dz, a2, 1, 1, 1, 0, 0, -1, G, false, c10::nullopt, c10::nullopt);
    }
    torch::Tensor Sm, cs, part;
    if (gram != nullptr) {
      Sm = gram[0];
      cs = gram[1];
    } else {
      auto g3 = fold_gram_now(a2);
      Sm = g3[0];
      cs = g3[1];
      part = g3[2];
    }
    check_hip(launch_bnfold_wgrad(coef.data_ptr<float>(), G.data_ptr<float>(), Sm.data_ptr<float>(),
                                  cs.data_ptr<float>(), 1, w3.data_ptr(), (int)C3, (int)K3, sink.data_ptr<float>(),
                                  1, cur_stream()),
              "bnfold_wgrad");
    if (side != 0) {
      side_stash().push_back(G);
      side_stash().push_back(Sm);
      side_stash().push_back(cs);
      if (part.defined()) side_stash().push_back(part);
    }
  };
  if (side == 0) {
    body();
    return;
  }
  auto guard = side_fork(side, dz.device(), {dz, a2, w3, coef});
  body();
}

// BN3 fold, main-stream part. K-concatenated (SDX_FOLD_CAT, default): one [K][1][1][C + K]
// bf16 tensor [Wd | Mx] with Wd = diag(A)·W3 (dgrad layout) and Mx = W3ᵀ·diag(D)·W3, plus the
// fp32 bias b = Eᵀ·W3 — conv3's dgrad then reduces over [dz | a2] (DgradOpts::cat). Otherwise
// Wd and T = a2·Mx + b (bf16), the D·y3 + E part of dy3 pushed through conv3's data gradient
// and added to its accumulators before the rounding (DgradOpts::add_pre).
struct FoldOps {
  torch::Tensor w;      // Wd, or [Wd | Mx] when cat
  torch::Tensor t;      // T (not cat)
  torch::Tensor bias;   // b (cat)
  bool cat = false;
  // the mode of the folded conv's dgrad; a2 (the conv's input) must outlive the options
  DgradOpts dgrad_opts(const torch::Tensor& a2) const {
    DgradOpts o;
    if (cat) {
      o.cat = &a2;
      o.cat_bias = &bias;
    } else {
      o.addend = t;
      o.add_pre = true;
    }
    return o;
  }
};
bool fold_cat_enabled() {
  static const bool on = sdx_plan::env_flag("SDX_FOLD_CAT", true);
  return on;
}
FoldOps fold_dgrad_operands(const torch::Tensor& coef, const torch::Tensor& w3, const torch::Tensor& wt3,
                            const torch::Tensor& a2, const torch::Tensor& mu, const torch::Tensor* gram) {
  const int64_t C3 = w3.size(0), K3 = w3.size(3);
  TORCH_CHECK(w3.size(1) == 1 && w3.size(2) == 1 && wt3.size(0) == K3 && wt3.size(3) == C3 && a2.size(3) == K3 &&
                  coef.numel() == 3 * C3,
              "bn3 fold: conv3 must be 1x1 [C][1][1][K] with a2 of K channels");
  const int64_t rows = a2.numel() / K3;
  TORCH_CHECK(rows < (1LL << 31), "bn3 fold: too many rows");
  check_vec(mu, C3, "fold mu");
  // conv3's dgrad: dy = dz (C3 channels) on a2's pixels
  const ConvGeom gd = conv_geom(a2.size(0), a2.size(1), a2.size(2), K3, C3, 1, 1, 1, 0);
  FoldOps r;
  r.bias = torch::empty({K3}, coef.options());
  const float* cs = gram != nullptr ? gram[1].data_ptr<float>() : nullptr;
  if (fold_cat_enabled() && sdx_plan::dgrad_cat_supported(gd, (int)K3, knobs())) {
    r.cat = true;
    r.w = torch::empty({K3, 1, 1, C3 + K3}, w3.options());
    uint16_t* wc = reinterpret_cast<uint16_t*>(r.w.data_ptr());
    check_hip(launch_bnfold_prep(coef.data_ptr<float>(), w3.data_ptr(), wt3.data_ptr(), (int)C3, (int)K3, wc, wc + C3,
                                 r.bias.data_ptr<float>(), mu.data_ptr<float>(), cs, (long)rows, cur_stream(),
                                 (int)(C3 + K3), (int)(C3 + K3)),
              "bnfold_prep");
    return r;
  }
  r.w = torch::empty_like(wt3);
  auto mx = torch::empty({K3, 1, 1, K3}, w3.options());
  check_hip(launch_bnfold_prep(coef.data_ptr<float>(), w3.data_ptr(), wt3.data_ptr(), (int)C3, (int)K3, r.w.data_ptr(),
                               mx.data_ptr(), r.bias.data_ptr<float>(), mu.data_ptr<float>(), cs, (long)rows,
                               cur_stream()),
            "bnfold_prep");
  const ConvGeom g = conv_geom(rows, 1, 1, K3, K3, 1, 1, 1, 0);   // T = a2·Mx + b as a [rows] x K3 GEMM
  r.t = torch::empty_like(a2);
  const GemmEpi epi{r.bias.data_ptr<float>(), 0, 0};
  check_hip(launch_conv_fwd(g, a2.data_ptr(), mx.data_ptr(), r.t.data_ptr(), nullptr, auto_cfg(rows, K3, K3, true),
                            cur_stream(), nullptr, nullptr, &epi),
            "bnfold T gemm");
  return r;
}

// bn: [gamma, beta, running_mean, running_var] per BN, in the order bn1, bn2, (bn3), (shortcut bn)
// returns the BlockSlot layout [out, y1, a1, y2, a2|-, y3|-, ys|-, omask (uint8 ReLU bits of
// out; training only)], then sc, sh, mu, iv per BN
//
// fold_fwd (bottleneck, training; ops/block.py decides): the forward half of the BN3 fold —
// conv3 runs twice, first for its BN statistics only (nothing stored), then with the BN3
// apply + residual + ReLU + output bits in its epilogue, so y3 is never written nor re-read
// (≈2 passes over the block's widest tensor); its backward takes Σdz·y3 from W3 and dzᵀ·a2
// (block_bwd, bnfold_rowdot) instead of re-reading y3. Projection blocks: the residual is the
// shortcut's pre-BN output with the shortcut BN applied in the same epilogue (that BN's
// statistics are final before pass 2), which replaces the separate two-input apply pass
//
// side (optional HIP stream): a projection block's shortcut conv (+ its statistics slab) runs
// there, concurrently with the main branch conv1 -> bn1 -> conv2 -> ...; its BN finalize (and
// any SyncBN exchange) stays on the compute stream after the join, so exchanges keep one order
std::vector<torch::Tensor> block_fwd(torch::Tensor x, std::vector<torch::Tensor> w, std::vector<torch::Tensor> bn,
                                     int64_t stride, bool bottleneck, bool proj, bool training, double eps,
                                     double momentum, int64_t comm, bool fold_fwd = false, int64_t side = 0) {
  const int nconv = bottleneck ? 3 : 2;
  TORCH_CHECK((int)w.size() == nconv + (proj ? 1 : 0), "block_fwd: weight count");
  TORCH_CHECK(bn.size() == w.size() * 4, "block_fwd: 4 BN tensors per conv");
  // BN i's forward statistics from a conv's slab (SyncBN over comm)
  auto bn_fwd = [&](int i, const torch::Tensor& slab, double count) {
    return bn_forward(slab, count, bn[i * 4], bn[i * 4 + 1], bn[i * 4 + 2], bn[i * 4 + 3], eps, momentum, training,
                      comm);
  };
  // conv + BN i forward: the conv's epilogue emits per-tile statistics, one launch reduces and
  // finalizes them (or reduce -> SyncBN exchange -> finalize)
  auto conv_bn = [&](const torch::Tensor& in, int i, int64_t s, int64_t p) -> std::pair<torch::Tensor, BnState> {
    auto c = conv_fwd(in, w[i], s, p, training, -1, c10::nullopt, c10::nullopt);
    return {c[0], bn_fwd(i, c[1], rows_of(c[0]))};
  };
  auto relu_bn = [](const torch::Tensor& y, const BnState& s) {
    return bn_apply(y, s.sc, s.sh, {}, true, c10::nullopt);
  };
  std::vector<BnState> st;
  std::vector<torch::Tensor> out(kMask);
  // shortcut conv on the side stream: outputs allocated on the compute stream (they are
  // read there after the join), the side stream only writes them
  torch::Tensor ys_side, slab_side;
  hipEvent_t sc_done = nullptr;
  if (proj && training && side != 0) {
    const torch::Tensor& ws = w[nconv];
    check_bf16_nhwc(x, "x");
    check_bf16_nhwc(ws, "w_shortcut");
    TORCH_CHECK(ws.size(3) == x.size(3) && ws.size(1) == 1 && ws.size(2) == 1, "block_fwd: 1x1 shortcut");
    const ConvGeom gs = fwd_geom(x, ws, stride, 0);
    const int64_t M = (int64_t)gs.N * gs.P * gs.Q;
    const int cfg = auto_cfg(M, gs.K, gs.C, true);
    ys_side = torch::empty({gs.N, gs.P, gs.Q, gs.K}, x.options());
    slab_side = torch::empty({sdx_plan::cdiv(M, sdx_plan::tile_m(cfg)), 2, gs.K}, x.options().dtype(at::kFloat));
    auto guard = side_fork(side, x.device(), {});
    check_hip(launch_conv_fwd(gs, x.data_ptr(), ws.data_ptr(), ys_side.data_ptr(), slab_side.data_ptr<float>(), cfg,
                              cur_stream()),
              "block_fwd shortcut conv (side stream)");
    sc_done = stream_mark();
  }
  const int64_t s1 = bottleneck ? 1 : stride, p1 = bottleneck ? 0 : 1;
  auto c1 = conv_bn(x, 0, s1, p1);
  st.push_back(c1.second);
  auto a1 = relu_bn(c1.first, st[0]);
  const int64_t s2 = bottleneck ? stride : 1;
  auto c2 = conv_bn(a1, 1, s2, 1);
  st.push_back(c2.second);
  torch::Tensor last = c2.first, a2;
  int lastbn = 1;
  // identity blocks: the residual is x (stride 1, same width); projection blocks: the
  // shortcut's pre-BN output ys, normalised in the same epilogue
  fold_fwd = fold_fwd && bottleneck && training && w[2].size(1) == 1 && w[2].size(2) == 1 &&
             (proj || (stride == 1 && w[2].size(0) == x.size(3))) && sdx_plan::fwd_bnapply_supported(knobs());
  torch::Tensor o, ys;
  // the projection shortcut's output and BN statistics (joins the side stream if it ran there)
  auto shortcut = [&] {
    if (sc_done != nullptr) {
      stream_wait(sc_done);
      st.push_back(bn_fwd(nconv, slab_side, rows_of(ys_side)));
      ys = ys_side;
    } else {
      auto cs = conv_bn(x, nconv, stride, 0);
      st.push_back(cs.second);
      ys = cs.first;
    }
  };
  // the block output's ReLU mask for backward: 1 bit per element instead of re-reading out
  // (identity blocks: out has x's shape; projection / strided blocks: the last conv's)
  torch::Tensor omask;
  if (bottleneck) {
    a2 = relu_bn(c2.first, st[1]);
    if (fold_fwd) {
      // pass 1: BN3 statistics (nothing stored) -> finalize (SyncBN: fused exchange) ;
      // pass 2: out = relu(bn3(y3) + x) (projection: + bn_s(ys)) and its bits straight from
      // conv3's epilogue
      auto c3s = conv_fwd(a2, w[2], 1, 0, true, -1, c10::nullopt, c10::nullopt, nullptr, true);
      st.push_back(bn_fwd(2, c3s[1], rows_of(a2)));
      GemmEpi epi{};
      epi.bn_scale = st[2].sc.data_ptr<float>();
      epi.bn_shift = st[2].sh.data_ptr<float>();
      if (proj) {
        shortcut();
        TORCH_CHECK(ys.size(0) == a2.size(0) && ys.size(1) == a2.size(1) && ys.size(2) == a2.size(2) &&
                        ys.size(3) == w[2].size(0),
                    "block_fwd: shortcut output shape");
        epi.resid = ys.data_ptr();
        epi.resid_scale = st[3].sc.data_ptr<float>();
        epi.resid_shift = st[3].sh.data_ptr<float>();
      } else {
        epi.resid = x.data_ptr();
      }
      omask = torch::empty({rows_of(a2) * w[2].size(0) / 8}, x.options().dtype(at::kByte));
      epi.mask_out = omask.data_ptr<uint8_t>();
      o = conv_fwd(a2, w[2], 1, 0, false, -1, c10::nullopt, c10::nullopt, &epi)[0];
      last = torch::Tensor();
    } else {
      auto c3 = conv_bn(a2, 2, 1, 0);
      st.push_back(c3.second);
      last = c3.first;
    }
    lastbn = 2;
  }
  if (training && !omask.defined())
    omask = torch::empty({last.numel() / 8}, last.options().dtype(at::kByte));
  const OptT om = training ? OptT(omask) : OptT();
  if (fold_fwd) {
    // out computed by conv3's epilogue
  } else if (proj) {
    shortcut();
    o = bn_apply(last, st[lastbn].sc, st[lastbn].sh, {ys, st[nconv].sc, st[nconv].sh, 1}, true, om);
  } else {
    o = bn_apply(last, st[lastbn].sc, st[lastbn].sh, {x, {}, {}, 2}, true, om);
  }
  out.push_back(omask);    // kMask (before the per-BN state)
  out[kOut] = o;
  out[kY1] = c1.first;
  out[kA1] = a1;
  out[kY2] = c2.first;
  out[kA2] = bottleneck ? a2 : torch::Tensor();
  out[kY3] = bottleneck ? last : torch::Tensor();   // undefined with fold_fwd (y3 never stored)
  out[kYs] = ys;
  for (auto& b : st) {   // kBnStride tensors per BN, in BnSlot order
    out.push_back(b.sc);
    out.push_back(b.sh);
    out.push_back(b.mu);
    out.push_back(b.iv);
  }
  return out;
}

// saved: the BlockSlot layout [x, y1, a1, y2, a2|-, y3|-, ys|-, out or its uint8 ReLU bitmask] ;
// bnst: [sc, sh, mu, iv] per BN (fwd order)
// wt: dgrad-layout weights (conv order); dw: fp32 gradient sinks (conv order);
// bng: [gamma, dgamma_sink, dbeta_sink] per BN. Returns dx.
//
// Cross-block BN-statistics hand-off (SDX_DGRAD_BNSTAT): in_slab (optional) holds this
// block's OUTPUT-BN backward sums [rows][2|3][C], computed by the NEXT block's final dgrad
// (the one that produced dout); prev = [y_last, mean_last, y_short|-, mean_short|-, omask]
// of the PREVIOUS native block (whose output is x): the final dgrad here computes that
// block's sums from the dx it stores. Returns [dx, slab for the previous block | undefined].
std::vector<torch::Tensor> block_bwd(torch::Tensor dout, std::vector<torch::Tensor> saved,
                                     std::vector<torch::Tensor> bnst, std::vector<torch::Tensor> wt,
                                     std::vector<torch::Tensor> dw, std::vector<torch::Tensor> bng, int64_t stride,
                                     bool bottleneck, bool proj, int64_t side, int64_t comm, OptT in_slab,
                                     std::vector<torch::Tensor> prev, std::vector<torch::Tensor> fold_w) {
  const int nconv = bottleneck ? 3 : 2;
  const int nbn = nconv + (proj ? 1 : 0);
  // the side-stream sink reductions queued by side_wgrad go out as one launch when the block
  // is done (before the caller announces the sinks final); dropped if the block throws
  struct DeferGuard {
    bool ok = false;
    ~DeferGuard() {
      if (!ok) splitk_defer_cancel();
    }
  } defer_guard;
  TORCH_CHECK((int)wt.size() == nbn && (int)dw.size() == nbn && (int)bng.size() == 3 * nbn &&
                  (int)bnst.size() == kBnStride * nbn && saved.size() == kSlots,
              "block_bwd: argument counts");
  const torch::Tensor &x = saved[kX], &y1 = saved[kY1], &a1 = saved[kA1], &y2 = saved[kY2], &a2 = saved[kA2],
                      &y3 = saved[kY3], &ys = saved[kYs], &out = saved[kMask];
  auto S = [&](int i, int k) { return bnst[i * kBnStride + k]; };
  // BN i's backward operands: gamma, saved statistics, the dγ / dβ sinks
  auto bset = [&](int i) { return BnBwdSet{bng[i * 3], S(i, kMu), S(i, kIv), bng[i * 3 + 1], bng[i * 3 + 2]}; };
  const int64_t H = x.size(1), W = x.size(2);
  const int lastbn = nconv - 1;
  const torch::Tensor& ylast = bottleneck ? y3 : y2;
  // forward-folded BN3 (block_fwd fold_fwd): y3 was never stored
  const bool no_y3 = bottleneck && (!y3.defined() || y3.numel() == 0);
  const double cnt_last = rows_of(y2), cnt1 = rows_of(y1);   // conv3 is 1x1 stride 1: y3 rows = y2 rows
  torch::Tensor dylast, dys, dz;
  const bool have_slab = in_slab.has_value() && in_slab->defined() && in_slab->numel() > 0;
  if (have_slab) TORCH_CHECK(in_slab->size(1) == (proj ? 3 : 2), "block_bwd: in_slab set count");
  // BN3 fold (bnfold.hip): fold_w = [conv3 forward weights] was passed because this block
  // published the fold marker (prev[5]) to the next block, whose final dgrad then stored
  // dout already masked (dz = dout·[out > 0]) together with in_slab
  // projection blocks: fold_w = [conv3, shortcut] folds both BNs (stride-1 shortcut only: its
  // input is then x itself); fold_w = [conv3] folds BN3 and materialises only the shortcut's dys
  // fold_w may be followed by the forward-time Grams of the folded convs' inputs (fold_gram):
  // [W3, (Ws)] or [W3, (Ws), S3, cs3, (Ss, css)]
  const size_t nfw = fold_w.size() == 3 || fold_w.size() == 6 ? fold_w.size() / 3 : fold_w.size();
  const bool grams = nfw != fold_w.size();
  const bool fold = bottleneck && have_slab && nfw >= 1 && nfw <= (proj ? 2u : 1u) && fold_w[0].defined() &&
                    (nfw == 1 || (stride == 1 && fold_w[1].defined()));
  const bool fold_sc = fold && proj && nfw == 2;
  TORCH_CHECK(!no_y3 || fold, "block_bwd: a forward-folded block needs its BN3 fold (next block's slab)");
  const torch::Tensor* gram3 = grams ? &fold_w[nfw] : nullptr;
  const torch::Tensor* grams_sc = grams && nfw == 2 ? &fold_w[nfw + 2] : nullptr;
  torch::Tensor coef3, coefs, Gfold;
  if (no_y3) {
    // Σdz·y3 = Σ_k W3[c][k]·(dzᵀ·a2)[c][k]: G on the main stream (the fold's wgrad reuses it),
    // written into the two extra rows the next block's final dgrad left in in_slab (a
    // projection block's third set, Σdz·(ys − μs), came from that dgrad's epilogue)
    const int64_t C3 = dout.size(3), K3 = a2.size(3), ns = in_slab->size(1);
    TORCH_CHECK(in_slab->size(0) > 2 && in_slab->size(2) == C3 && fold_w[0].size(0) == C3 &&
                    fold_w[0].size(3) == K3,
                "block_bwd: forward-folded BN3 slab / weights");
    Gfold = torch::empty({C3, 1, 1, K3}, dout.options().dtype(at::kFloat));
    conv_wgrad(dout, a2, 1, 1, 1, 0, 0, -1, Gfold, false, c10::nullopt, c10::nullopt);
    float* rows = in_slab->data_ptr<float>() + (in_slab->size(0) - 2) * ns * C3;
    check_hip(launch_bnfold_rowdot(Gfold.data_ptr<float>(), fold_w[0].data_ptr(), (int)C3, (int)K3, (int)ns, rows,
                                   cur_stream()),
              "bnfold_rowdot");
  }
  {
    // the output BN's coefficients (projection: and the shortcut BN's, fed by the same dz):
    // from the next block's slab, or from an elementwise pass over dout under out's ReLU mask
    const BnBwdSrc src{dout, out, ylast, proj ? OptT(ys) : OptT()};
    auto c = bn_bwd_coefs(comm, have_slab ? nullptr : &src, have_slab ? &*in_slab : nullptr, cnt_last, bset(lastbn),
                          proj ? bset(nconv) : BnBwdSet{});
    if (fold) {
      coef3 = c[0];
      dz = dout;
      if (fold_sc)
        coefs = c[1];
      else if (proj)   // dout is already masked: dys = A'·dz + D'·ys + E' without a ReLU mask
        dys = bn_bwd_apply({dz, {}, ys}, c[1], c10::nullopt, false)[0];
    } else if (proj) {
      auto r = bn_bwd_apply(src, c[0], c[1], false);
      dylast = r[0];
      dys = r[1];
    } else {
      // identity shortcut: its gradient dz = dout·[out > 0] is never materialised when the ReLU
      // bitmask is available — the last dgrad epilogue adds dout under the mask
      const bool bitmask = out.scalar_type() == at::kByte;
      auto r = bn_bwd_apply(src, c[0], c10::nullopt, !bitmask);
      dylast = r[0];
      dz = bitmask ? torch::Tensor() : r[2];
    }
  }
  // dgrad whose output da is the gradient of the block-internal BN i's ReLU output; the BN's
  // Σda·m, Σda·m·(y−μ) come from the dgrad epilogue (SDX_DGRAD_BNSTAT=0: separate pass)
  auto dgrad_bn = [&](const torch::Tensor& dyo, const torch::Tensor& w, const torch::Tensor& y, int64_t st,
                      int64_t pad, int i, double cnt, const DgradOpts& o = {}) -> std::pair<torch::Tensor, torch::Tensor> {
    if (dgrad_bnstat_enabled()) {
      DgradStat ds;
      ds.ya = y; ds.ma = S(i, kMu); ds.msc = S(i, kSc); ds.msh = S(i, kSh);
      auto r = conv_dgrad_bnstat(dyo, w, y.size(1), y.size(2), st, pad, -1, o, ds);
      return {r[0], bn_bwd_coefs(comm, nullptr, &r[1], cnt, bset(i))[0]};
    }
    auto da = conv_dgrad(dyo, w, y.size(1), y.size(2), st, pad, -1, o);
    const BnBwdSrc src{da, {}, y, {}, S(i, kSc), S(i, kSh)};
    return {da, bn_bwd_coefs(comm, &src, nullptr, cnt, bset(i))[0]};
  };
  // dy of the block-internal BN i from the gradient da of its ReLU output (mask recomputed from y)
  auto bn_relu_bwd = [&](const torch::Tensor& da, const torch::Tensor& y, const torch::Tensor& coef, int i) {
    return bn_bwd_apply({da, {}, y, {}, S(i, kSc), S(i, kSh)}, coef, c10::nullopt, false)[0];
  };
  torch::Tensor dy1;
  if (bottleneck) {
    std::pair<torch::Tensor, torch::Tensor> r2;
    if (fold) {
      // da2 = dz·(diag(A)·W3) + T: no dy3 tensor; dW3 from dzᵀ·a2 and a2ᵀ·a2 on the side stream
      auto op = fold_dgrad_operands(coef3, fold_w[0], wt[2], a2, S(lastbn, kMu), gram3);
      side_fold_wgrad(dz, a2, fold_w[0], coef3, dw[2], side, gram3, Gfold.defined() ? &Gfold : nullptr);
      r2 = dgrad_bn(dz, op.w, y2, 1, 0, 1, cnt_last, op.dgrad_opts(a2));
    } else {
      side_wgrad(dylast, a2, 1, 1, 1, 0, dw[2], side);
      r2 = dgrad_bn(dylast, wt[2], y2, 1, 0, 1, cnt_last);
    }
    auto dy2 = bn_relu_bwd(r2.first, y2, r2.second, 1);
    side_wgrad(dy2, a1, 3, 3, stride, 1, dw[1], side);
    auto r1 = dgrad_bn(dy2, wt[1], y1, stride, 1, 0, cnt1);
    dy1 = bn_relu_bwd(r1.first, y1, r1.second, 0);
    side_wgrad(dy1, x, 1, 1, 1, 0, dw[0], side);
  } else {
    side_wgrad(dylast, a1, 3, 3, 1, 1, dw[1], side);
    auto r1 = dgrad_bn(dylast, wt[1], y1, 1, 1, 0, cnt1);
    dy1 = bn_relu_bwd(r1.first, y1, r1.second, 0);
    side_wgrad(dy1, x, 3, 3, stride, 1, dw[0], side);
  }
  const int64_t s1 = bottleneck ? 1 : stride, p1 = bottleneck ? 0 : 1;
  // the final dgrad (the one that stores dx) optionally emits the previous block's output-BN sums
  const bool want_prev = dgrad_bnstat_enabled() && prev.size() >= 5 && prev[4].defined() && prev[4].numel() > 0;
  // the previous block folds its BN3 backward: store its dz = dx·[out_prev > 0], not dx
  const bool prev_fold = want_prev && prev.size() >= 6 && prev[5].defined() && prev[5].numel() > 0;
  torch::Tensor prev_slab;
  auto last_dgrad = [&](const DgradOpts& o) -> torch::Tensor {
    if (!want_prev) return conv_dgrad(dy1, wt[0], H, W, s1, p1, -1, o);
    const bool two = prev[2].defined() && prev[2].numel() > 0;
    // the previous block folded its BN3 forward too (no y3): Σdz and −μ·Σdz here, two slab
    // rows left for its Σdz·y3 (block_bwd no_y3)
    const bool prev_noy = !prev[0].defined() || prev[0].numel() == 0;
    TORCH_CHECK(!prev_noy || prev_fold, "block_bwd: previous block without y3 must fold");
    DgradStat ds;
    ds.ya = prev[0]; ds.ma = prev[1]; ds.mask_bits = prev[4];
    if (two) {
      ds.yb = prev[2];
      ds.mb = prev[3];
    }
    ds.store_masked = prev_fold ? 1 : 0;
    ds.extra_rows = prev_noy ? 2 : 0;
    auto r = conv_dgrad_bnstat(dy1, wt[0], H, W, s1, p1, -1, o, ds);
    prev_slab = r[1];
    return r[0];
  };
  torch::Tensor dx;
  if (fold_sc) {
    // shortcut BN folded like BN3: dx_sc = dz·(diag(A')·Ws) + x·(Wsᵀ·diag(D')·Ws) + E'ᵀ·Ws
    auto op = fold_dgrad_operands(coefs, fold_w[1], wt[nconv], x, S(nconv, kMu), grams_sc);
    side_fold_wgrad(dz, x, fold_w[1], coefs, dw[nconv], side, grams_sc);
    dx = conv_dgrad(dz, op.w, H, W, 1, 0, -1, op.dgrad_opts(x));
    dx = last_dgrad(into(dx, dx));
  } else if (proj) {
    side_wgrad(dys, x, 1, 1, stride, 0, dw[nconv], side);
    if (stride > 1 && sub_addend_enabled()) {
      // the strided 1x1 shortcut's data gradient lives on the stride-s subgrid only: compute
      // it compactly (a stride-1 1x1 dgrad on the P x Q grid) and let the final dgrad add it
      // there — no zero sub-pixel classes written, no zeros re-read as the addend
      auto dxs = conv_dgrad(dys, wt[nconv], dys.size(1), dys.size(2), 1, 0, -1);
      dx = last_dgrad(into({}, dxs, {}, stride));
    } else {
      dx = conv_dgrad(dys, wt[nconv], H, W, stride, 0, -1);
      dx = last_dgrad(into(dx, dx));
    }
  } else if (dz.defined()) {
    dx = last_dgrad(into({}, dz));
  } else {
    dx = last_dgrad(into({}, dout, out));
  }
  check_hip(splitk_flush(), "splitk_flush");
  defer_guard.ok = true;
  return {dx, prev_slab};
}

// ---- test-only bindings of the BN3 fold kernels (tests/bnfold_checks.py) -----------------
// Thin wrappers over the launchers: every extent a kernel reads or writes is checked here,
// the shape rules of the kernels themselves (which K and C they take) are left to the
// launchers, whose hipErrorInvalidValue comes back as a RuntimeError before any launch.

void check_f32(const torch::Tensor& t, int64_t numel, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == numel, name,
              " must be a contiguous float32 GPU tensor of ", numel, " elements");
}

void check_bf16_flat(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous(), name,
              " must be a contiguous bf16 GPU tensor");
}

// w [C][1][1][K] bf16 -> (C, K)
std::pair<int64_t, int64_t> fold_weight_dims(const torch::Tensor& w) {
  check_bf16_flat(w, "w");
  TORCH_CHECK(w.dim() == 4 && w.size(1) == 1 && w.size(2) == 1 && w.size(0) > 0 && w.size(3) > 0 &&
                  w.size(0) < (1 << 20) && w.size(3) < (1 << 20),
              "w must be [C][1][1][K]");
  return {w.size(0), w.size(3)};
}

// Wd, Mx and b into caller-supplied (flat) outputs: wd_out holds rows of ldw elements (0: C),
// mx_out rows of ldm (0: K); the concatenated layout is mx_out = wd_out[C:], ldw = ldm = C + K
void bnfold_prep_test(torch::Tensor coef, torch::Tensor w, torch::Tensor wt, OptT mu, OptT cs, int64_t rows,
                      int64_t ldw, int64_t ldm, torch::Tensor wd_out, torch::Tensor mx_out, torch::Tensor bias_out) {
  const auto [C, K] = fold_weight_dims(w);
  check_bf16_flat(wt, "wt");
  TORCH_CHECK(wt.dim() == 4 && wt.size(0) == K && wt.size(1) == 1 && wt.size(2) == 1 && wt.size(3) == C,
              "wt must be [K][1][1][C]");
  check_f32(coef, 3 * C, "coef");
  check_f32(bias_out, K, "bias_out");
  check_bf16_flat(wd_out, "wd_out");
  check_bf16_flat(mx_out, "mx_out");
  TORCH_CHECK(rows >= 0 && rows < (1LL << 31) && ldw >= 0 && ldm >= 0 && ldw < (1 << 24) && ldm < (1 << 24),
              "bnfold_prep: rows, ldw or ldm out of range");
  const int64_t lw = ldw == 0 ? C : ldw, lm = ldm == 0 ? K : ldm;
  TORCH_CHECK(wd_out.numel() >= (K - 1) * lw + C, "wd_out too small for K rows of ldw");
  TORCH_CHECK(mx_out.numel() >= (K - 1) * lm + K, "mx_out too small for K rows of ldm");
  const float* pmu = opt_ptr(mu, C, "mu");
  const float* pcs = opt_ptr(cs, K, "cs");
  c10::DeviceGuard dg(w.device());
  check_hip(launch_bnfold_prep(coef.data_ptr<float>(), w.data_ptr(), wt.data_ptr(), (int)C, (int)K, wd_out.data_ptr(),
                               mx_out.data_ptr(), bias_out.data_ptr<float>(), pmu, pcs, (long)rows, cur_stream(),
                               (int)ldw, (int)ldm),
            "bnfold_prep");
}

// x [rows][K] bf16 -> (cs [K], partial [bnfold_colsum_blocks()][K])
std::vector<torch::Tensor> bnfold_colsum_test(torch::Tensor x, OptT partial) {
  check_bf16_flat(x, "x");
  TORCH_CHECK(x.dim() == 2 && x.size(1) > 0 && x.numel() < (1LL << 31), "x must be [rows][K] bf16");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "x must be 16-byte aligned");
  const int64_t rows = x.size(0), K = x.size(1);
  c10::DeviceGuard dg(x.device());
  auto opt = x.options().dtype(at::kFloat);
  const int64_t nb = bnfold_colsum_blocks();
  torch::Tensor part = partial.has_value() && partial->defined() ? *partial : torch::empty({nb, K}, opt);
  check_f32(part, nb * K, "partial");
  auto cs = torch::empty({K}, opt);
  check_hip(launch_bnfold_colsum(x.data_ptr(), (long)rows, (int)K, part.data_ptr<float>(), cs.data_ptr<float>(),
                                 cur_stream()),
            "bnfold_colsum");
  return {cs, part};
}

// sink [C][K] (+)= diag(A)·G + diag(D)·W3·S + E ⊗ Σ_b cs[b]; returns the sink
torch::Tensor bnfold_wgrad_test(torch::Tensor coef, torch::Tensor G, torch::Tensor S, torch::Tensor cs,
                                torch::Tensor w, torch::Tensor sink, bool accumulate) {
  const auto [C, K] = fold_weight_dims(w);
  check_f32(coef, 3 * C, "coef");
  check_f32(G, C * K, "G");
  check_f32(S, K * K, "S");
  check_f32(sink, C * K, "sink");
  TORCH_CHECK(cs.dim() == 2 && cs.size(1) == K, "cs must be [ncs][K]");
  check_f32(cs, cs.size(0) * K, "cs");
  c10::DeviceGuard dg(w.device());
  check_hip(launch_bnfold_wgrad(coef.data_ptr<float>(), G.data_ptr<float>(), S.data_ptr<float>(), cs.data_ptr<float>(),
                                (int)cs.size(0), w.data_ptr(), (int)C, (int)K, sink.data_ptr<float>(),
                                accumulate ? 1 : 0, cur_stream()),
            "bnfold_wgrad");
  return sink;
}

// Σ_k W[c][k]·G[c][k] as fp32 hi / lo into set 1 of out [2][ns][C]; returns out
torch::Tensor bnfold_rowdot_test(torch::Tensor G, torch::Tensor w, int64_t ns, torch::Tensor out) {
  const auto [C, K] = fold_weight_dims(w);
  check_f32(G, C * K, "G");
  TORCH_CHECK(ns >= 0 && ns <= 16 && out.dim() == 3 && out.size(0) == 2 && out.size(1) == ns && out.size(2) == C,
              "out must be [2][ns][C]");
  check_f32(out, 2 * ns * C, "out");
  c10::DeviceGuard dg(w.device());
  check_hip(launch_bnfold_rowdot(G.data_ptr<float>(), w.data_ptr(), (int)C, (int)K, (int)ns, out.data_ptr<float>(),
                                 cur_stream()),
            "bnfold_rowdot");
  return out;
}

}  // namespace

void register_block(pybind11::module& m) {
  m.def("bnfold_prep", &bnfold_prep_test, "BN3 fold (test only): Wd, Mx and b into caller-supplied outputs",
        pybind11::arg("coef"), pybind11::arg("w"), pybind11::arg("wt"), pybind11::arg("mu") = pybind11::none(),
        pybind11::arg("cs") = pybind11::none(), pybind11::arg("rows") = 0, pybind11::arg("ldw") = 0,
        pybind11::arg("ldm") = 0, pybind11::arg("wd_out"), pybind11::arg("mx_out"), pybind11::arg("bias_out"));
  m.def("bnfold_colsum", &bnfold_colsum_test, "BN3 fold (test only): column sums of x [rows][K] -> (cs, partial)",
        pybind11::arg("x"), pybind11::arg("partial") = pybind11::none());
  m.def("bnfold_wgrad", &bnfold_wgrad_test, "BN3 fold (test only): the folded weight gradient into sink",
        pybind11::arg("coef"), pybind11::arg("G"), pybind11::arg("S"), pybind11::arg("cs"), pybind11::arg("w"),
        pybind11::arg("sink"), pybind11::arg("accumulate"));
  m.def("bnfold_rowdot", &bnfold_rowdot_test, "BN3 fold (test only): Σ_k W·G as fp32 hi / lo slab rows",
        pybind11::arg("G"), pybind11::arg("w"), pybind11::arg("ns"), pybind11::arg("out"));
  m.def("side_stash_release", [] { side_stash().clear(); },
        "drop the tensors kept alive for side-stream wgrads (after join)");
  m.def("block_fwd", &block_fwd, "native residual-block forward (whole kernel sequence; comm: SyncBN handle or 0)",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("bn"), pybind11::arg("stride"),
        pybind11::arg("bottleneck"), pybind11::arg("proj"), pybind11::arg("training"), pybind11::arg("eps"),
        pybind11::arg("momentum"), pybind11::arg("comm") = 0, pybind11::arg("fold_fwd") = false,
        pybind11::arg("side") = 0);
  m.def("fold_gram", &fold_gram,
        "BN3 fold: [a2ᵀ·a2, Σ_rows a2, scratch] of a folded conv's input, issued on the side stream",
        pybind11::arg("a2"), pybind11::arg("side"));
  m.def("block_bwd", &block_bwd, "native residual-block backward (dgrad chain + side-stream wgrads)",
        pybind11::arg("dout"), pybind11::arg("saved"), pybind11::arg("bnst"), pybind11::arg("wt"),
        pybind11::arg("dw"), pybind11::arg("bng"), pybind11::arg("stride"), pybind11::arg("bottleneck"),
        pybind11::arg("proj"), pybind11::arg("side"), pybind11::arg("comm") = 0,
        pybind11::arg("in_slab") = pybind11::none(), pybind11::arg("prev") = std::vector<torch::Tensor>(),
        pybind11::arg("fold_w") = std::vector<torch::Tensor>());
}

}  // namespace sdx_bind
