// Bindings for the implicit-GEMM convolution kernels (igemm.hip, wgrad1x1.hip, wgrad3x3.hip).
// Host-side shape/dtype/layout checks run before every launch.
#include "ops_decl.h"
#include "conv_internal.h"
#include "launchers.h"

#include <atomic>
#include <utility>

namespace sdx_bind {

using sdx_plan::knobs;
using sdx_plan::knobs_mut;

void check_bf16_nhwc(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 4 && t.is_contiguous(), name, " must be a contiguous 4-D (NHWC) tensor");
  TORCH_CHECK(t.size(3) % 8 == 0, name, ": channel count must be a multiple of 8");
  TORCH_CHECK(t.numel() < (1LL << 31), name, " too large for 32-bit GEMM indexing");
}

void check_vec(const torch::Tensor& t, int64_t C, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == C, name,
              " must be a contiguous float32 GPU vector of length C");
}

const float* opt_ptr(const OptT& t, int64_t C, const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
  check_vec(*t, C, name);
  return t->data_ptr<float>();
}

void in_bn_ptrs(const OptT& sc, const OptT& sh, int64_t C, const float** ps, const float** pt) {
  *ps = opt_ptr(sc, C, "in_scale");
  *pt = opt_ptr(sh, C, "in_shift");
  TORCH_CHECK((*ps == nullptr) == (*pt == nullptr), "in_scale and in_shift must be given together");
}

void check_mask(const torch::Tensor& m, int64_t numel, const char* name) {
  TORCH_CHECK(m.is_cuda() && m.scalar_type() == at::kByte && m.is_contiguous() && m.numel() * 8 == numel, name,
              " must be a contiguous uint8 GPU tensor of numel/8 bytes");
}

ConvGeom conv_geom(int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t R, int64_t S, int64_t stride,
                   int64_t pad) {
  ConvGeom g{};
  g.N = (int)N; g.H = (int)H; g.W = (int)W; g.C = (int)C; g.K = (int)K; g.R = (int)R; g.S = (int)S;
  g.stride = (int)stride; g.pad = (int)pad;
  g.P = (g.H + 2 * g.pad - g.R) / g.stride + 1;
  g.Q = (g.W + 2 * g.pad - g.S) / g.stride + 1;
  return g;
}

ConvGeom fwd_geom(const torch::Tensor& x, const torch::Tensor& w, int64_t stride, int64_t pad) {
  return conv_geom(x.size(0), x.size(1), x.size(2), x.size(3), w.size(0), w.size(1), w.size(2), stride, pad);
}

ConvGeom dgrad_geom(const torch::Tensor& dy, const torch::Tensor& wt, int64_t H, int64_t W, int64_t stride,
                    int64_t pad) {
  ConvGeom g{};
  g.N = dy.size(0); g.P = dy.size(1); g.Q = dy.size(2); g.K = dy.size(3);
  g.C = wt.size(0); g.R = wt.size(1); g.S = wt.size(2);
  g.H = H; g.W = W; g.stride = stride; g.pad = pad;
  return g;
}

// Every dispatch decision (tile config, main loop, splits, slab rows) is a plan of
// conv_plan.h under the process's knobs; the setters below write those knobs.
int auto_cfg(int64_t M, int64_t Ncol, int64_t Kdim, bool fill) { return sdx_plan::auto_cfg(M, Ncol, Kdim, fill, knobs()); }

std::vector<torch::Tensor> conv_fwd(torch::Tensor x, torch::Tensor w, int64_t stride, int64_t pad, bool want_stats,
                                    int64_t cfg, OptT in_scale, OptT in_shift, const GemmEpi* epi, bool no_out) {
  check_bf16_nhwc(x, "x");
  check_bf16_nhwc(w, "w");
  TORCH_CHECK(w.size(3) == x.size(3), "weight Cin != input C");
  TORCH_CHECK(stride >= 1 && pad >= 0, "bad stride/pad");
  const ConvGeom g = fwd_geom(x, w, stride, pad);
  TORCH_CHECK(g.P > 0 && g.Q > 0, "empty output");
  TORCH_CHECK(g.K % 8 == 0, "Cout must be a multiple of 8");
  c10::DeviceGuard dg(x.device());
  const sdx_plan::FwdPlan plan = sdx_plan::plan_fwd(g, cfg, in_scale.has_value(), knobs());
  TORCH_CHECK(!no_out || (want_stats && epi == nullptr), "statistics-only conv: stats, no epilogue");
  auto y = no_out ? torch::Tensor() : torch::empty({g.N, g.P, g.Q, g.K}, x.options());
  torch::Tensor slab;
  float* sp = nullptr;
  if (want_stats) {
    slab = torch::empty({plan.m_tiles, 2, g.K}, x.options().dtype(at::kFloat));
    sp = slab.data_ptr<float>();
  } else {
    slab = torch::empty({0}, x.options().dtype(at::kFloat));
  }
  const float *isc, *ish;
  in_bn_ptrs(in_scale, in_shift, g.C, &isc, &ish);
  check_hip(launch_conv_fwd(g, x.data_ptr(), w.data_ptr(), no_out ? nullptr : y.data_ptr(), sp, plan.cfg, cur_stream(),
                            isc, ish, epi),
            "conv_fwd");
  return {y, slab};
}

namespace {

// conv with a per-output-channel fp32 bias (+ ReLU) applied to the fp32 accumulators before
// the bf16 rounding, no statistics: an eval-mode conv + BatchNorm (+ ReLU) with the BN
// folded into the weights and the bias (linear-probe encoder, ops/linear_probe.py)
torch::Tensor conv_fwd_bias(torch::Tensor x, torch::Tensor w, int64_t stride, int64_t pad, torch::Tensor bias,
                            bool relu) {
  check_vec(bias, w.size(0), "bias");
  GemmEpi epi{};
  epi.bias = bias.data_ptr<float>();
  epi.relu = relu ? 1 : 0;
  return conv_fwd(x, w, stride, pad, false, -1, c10::nullopt, c10::nullopt, &epi)[0];
}

// One data gradient's checked request: geometry, the K-concatenated operand's width and the
// plan, computed once for the launches and for the statistics slab
struct DgradReq {
  ConvGeom g;
  int64_t cat_ch;
  sdx_plan::DgradPlan plan;
};
DgradReq dgrad_request(const torch::Tensor& dy, const torch::Tensor& wt, int64_t H, int64_t W, int64_t stride,
                       int64_t pad, int64_t cfg, bool bstat, const DgradOpts& o) {
  check_bf16_nhwc(dy, "dy");
  check_bf16_nhwc(wt, "wt");
  DgradReq r{};
  r.cat_ch = o.cat != nullptr ? o.cat->size(3) : 0;
  TORCH_CHECK(wt.size(3) == dy.size(3) + r.cat_ch, "wt last dim must be Cout (+ the concatenated operand's channels)");
  if (o.cat != nullptr) {
    check_bf16_nhwc(*o.cat, "cat a2");
    TORCH_CHECK(stride == 1 && pad == 0 && wt.size(1) == 1 && wt.size(2) == 1 && o.cat->size(0) == dy.size(0) &&
                    o.cat->size(1) == dy.size(1) && o.cat->size(2) == dy.size(2),
                "K-concatenated dgrad: stride-1 1x1, a2 on dy's pixels");
    TORCH_CHECK(o.cat_bias != nullptr && o.cat_bias->is_cuda() && o.cat_bias->scalar_type() == at::kFloat &&
                    o.cat_bias->is_contiguous() && o.cat_bias->numel() == wt.size(0),
                "K-concatenated dgrad: fp32 bias [C]");
  }
  ConvGeom& g = r.g;
  g = dgrad_geom(dy, wt, H, W, stride, pad);
  TORCH_CHECK(stride >= 1 && (g.H + 2 * pad - g.R) / stride + 1 == g.P && (g.W + 2 * pad - g.S) / stride + 1 == g.Q,
              "dgrad geometry mismatch");
  TORCH_CHECK(g.C % 8 == 0, "Cin must be a multiple of 8");
  r.plan = sdx_plan::plan_dgrad(g, cfg, (int)r.cat_ch, bstat, knobs());
  TORCH_CHECK(r.plan.ok, "conv_dgrad: tile config ", r.plan.cfg, " does not run this geometry");
  return r;
}

// bs (optional): fused BN-backward statistics; its slab must hold the plan's rows
torch::Tensor conv_dgrad_impl(torch::Tensor dy, torch::Tensor wt, const DgradReq& rq, const DgradOpts& o,
                              BnBwdStat* bs) {
  const ConvGeom& g = rq.g;
  const sdx_plan::DgradPlan& plan = rq.plan;
  const int64_t addend_sub = o.addend_sub, stride = g.stride;
  TORCH_CHECK(o.cat == nullptr || !o.addend.has_value(), "K-concatenated dgrad: no addend");
  c10::DeviceGuard dg(dy.device());
  torch::Tensor dx;
  if (o.out.has_value()) {
    dx = *o.out;
    check_bf16_nhwc(dx, "out");
    TORCH_CHECK(dx.size(0) == g.N && dx.size(1) == g.H && dx.size(2) == g.W && dx.size(3) == g.C, "out shape");
  } else {
    dx = torch::empty({g.N, g.H, g.W, g.C}, dy.options());
  }
  const void* add = nullptr;
  TORCH_CHECK(addend_sub >= 0, "addend_sub");
  if (o.addend.has_value()) {
    check_bf16_nhwc(*o.addend, "addend");
    if (addend_sub > 1) {
      // compact addend on the stride-s subgrid (h, w ≡ 0 mod s)
      const int64_t s_ = addend_sub;
      TORCH_CHECK(o.addend->size(0) == g.N && o.addend->size(1) == (g.H + s_ - 1) / s_ &&
                      o.addend->size(2) == (g.W + s_ - 1) / s_ && o.addend->size(3) == g.C,
                  "compact addend shape [N, ceil(H/s), ceil(W/s), C]");
      TORCH_CHECK(!o.addend_mask.has_value(), "addend_mask is not supported with a compact addend");
    } else {
      TORCH_CHECK(o.addend->sizes() == dx.sizes(), "addend shape");
    }
    add = o.addend->data_ptr();
  }
  const void* amask = nullptr;
  if (o.addend_mask.has_value()) {
    TORCH_CHECK(add != nullptr, "addend_mask needs an addend");
    TORCH_CHECK(o.addend_mask->is_cuda() && o.addend_mask->scalar_type() == at::kByte &&
                    o.addend_mask->is_contiguous() && o.addend_mask->numel() * 8 == dx.numel(),
                "addend_mask: uint8 [numel/8]");
    amask = o.addend_mask->data_ptr();
  }
  if (bs) bs->row0 = 0;
  if (stride == 1) {
    // BN3 fold: the addend joins the accumulators before rounding (kernels built with SDX_ADD_PRE)
    static const GemmEpi pre{nullptr, 0, 0, 1};
    const GemmEpi* epi = (o.add_pre && add != nullptr && addend_sub == 0 && amask == nullptr) ? &pre : nullptr;
    GemmEpi ce{};
    if (o.cat != nullptr) {
      ce.cat_a = o.cat->data_ptr();
      ce.cat_ch = (int)rq.cat_ch;
      ce.bias_pre = o.cat_bias->data_ptr<float>();
      epi = &ce;
    }
    check_hip(launch_conv_dgrad_class(g, 0, 0, dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), add, plan.cfg,
                                      cur_stream(), amask, bs, add ? (int)addend_sub : 0, epi),
              "conv_dgrad");
    return dx;
  }
  // sub-pixel classes: each gets the taps r ≡ ph+pad, s ≡ pw+pad (mod stride); by default all
  // of them in one launch (plan.merged, SDX_DGRAD_MERGE)
  if (plan.merged) {
    check_hip(launch_conv_dgrad_merged(g, plan, dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), add, cur_stream(), amask,
                                       bs, add ? (int)addend_sub : 0),
              "conv_dgrad(merged classes)");
    return dx;
  }
  for (int i = 0; i < plan.ncls; ++i) {
    // each class reads its taps straight from the full Wt (no per-class weight copy; a
    // class without taps writes zeros and never reads B)
    const sdx_plan::DgradClass& c = plan.cls[i];
    check_hip(launch_conv_dgrad_class(g, c.ph, c.pw, dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), add, plan.cfg,
                                      cur_stream(), amask, bs, add ? (int)addend_sub : 0),
              "conv_dgrad(class)");
    if (bs) bs->row0 += c.m_tiles;
  }
  return dx;
}

}  // namespace

torch::Tensor conv_dgrad(torch::Tensor dy, torch::Tensor wt, int64_t H, int64_t W, int64_t stride, int64_t pad,
                         int64_t cfg, const DgradOpts& o) {
  const DgradReq rq = dgrad_request(dy, wt, H, W, stride, pad, cfg, false, o);
  return conv_dgrad_impl(dy, wt, rq, o, nullptr);
}

std::vector<torch::Tensor> conv_dgrad_bnstat(torch::Tensor dy, torch::Tensor wt, int64_t H, int64_t W,
                                             int64_t stride, int64_t pad, int64_t cfg, const DgradOpts& o,
                                             const DgradStat& st) {
  const DgradReq rq = dgrad_request(dy, wt, H, W, stride, pad, cfg, true, o);
  const int64_t C = wt.size(0);
  // an empty ya: the BN input was never stored (forward-folded BN3) — the epilogue sums
  // Σdz and Σdz·(0 − μ); the caller fills extra_rows rows of the slab with the Σdz·y terms
  const bool no_y = !st.ya.defined() || st.ya.numel() == 0;
  const int64_t elems = dy.size(0) * H * W * C;
  if (!no_y) {
    check_bf16_nhwc(st.ya, "ya");
    TORCH_CHECK(st.ya.size(0) == dy.size(0) && st.ya.size(1) == H && st.ya.size(2) == W && st.ya.size(3) == C,
                "ya shape");
  }
  TORCH_CHECK(st.extra_rows >= 0 && (!no_y || !st.msc.has_value()), "no-ya statistics: ReLU mask from bits");
  check_vec(st.ma, C, "ma");
  BnBwdStat bs{};
  bs.ya = no_y ? nullptr : st.ya.data_ptr();
  bs.ma = st.ma.data_ptr<float>();
  if (st.yb.has_value()) {
    check_bf16_nhwc(*st.yb, "yb");
    TORCH_CHECK(st.yb->size(0) == dy.size(0) && st.yb->size(1) == H && st.yb->size(2) == W && st.yb->size(3) == C,
                "yb shape");
    TORCH_CHECK(st.mb.has_value(), "mb required with yb");
    check_vec(*st.mb, C, "mb");
    bs.yb = st.yb->data_ptr();
    bs.mb = st.mb->data_ptr<float>();
  }
  if (st.mask_bits.has_value()) {
    TORCH_CHECK(st.mask_bits->is_cuda() && st.mask_bits->scalar_type() == at::kByte &&
                    st.mask_bits->is_contiguous() && st.mask_bits->numel() * 8 == elems,
                "mask_bits: uint8 [numel/8]");
    bs.mask = st.mask_bits->data_ptr<uint8_t>();
  } else if (st.msc.has_value()) {
    TORCH_CHECK(st.msh.has_value(), "msh required with msc");
    check_vec(*st.msc, C, "msc");
    check_vec(*st.msh, C, "msh");
    bs.msc = st.msc->data_ptr<float>();
    bs.msh = st.msh->data_ptr<float>();
  }
  const int rows = rq.plan.rows;
  const int ns = st.yb.has_value() ? 3 : 2;
  auto slab = torch::empty({rows + st.extra_rows, ns, C}, dy.options().dtype(at::kFloat));
  bs.slab = slab.data_ptr<float>();
  TORCH_CHECK(!st.store_masked || (st.mask_bits.has_value() && stride == 1),
              "store_masked: stride-1 with a ReLU bitmask");
  bs.store_masked = st.store_masked;
  auto dx = conv_dgrad_impl(dy, wt, rq, o, &bs);
  return {dx, slab};
}

torch::Tensor conv_wgrad(torch::Tensor dy, torch::Tensor x, int64_t R, int64_t S, int64_t stride, int64_t pad,
                         int64_t splits, int64_t cfg, c10::optional<torch::Tensor> out, bool accumulate,
                         OptT in_scale, OptT in_shift) {
  check_bf16_nhwc(dy, "dy");
  check_bf16_nhwc(x, "x");
  TORCH_CHECK(dy.size(0) == x.size(0), "batch mismatch");
  const ConvGeom g = conv_geom(x.size(0), x.size(1), x.size(2), x.size(3), dy.size(3), R, S, stride, pad);
  TORCH_CHECK(g.P == dy.size(1) && g.Q == dy.size(2), "wgrad geometry mismatch");
  c10::DeviceGuard dg(x.device());
  const int64_t M = g.K, Ncol = (int64_t)R * S * g.C;
  torch::Tensor dw;
  if (out.has_value()) {
    dw = *out;
    TORCH_CHECK(dw.is_cuda() && dw.scalar_type() == at::kFloat && dw.numel() == M * Ncol, "out: fp32 [K,R,S,C]");
    const bool krsc = dw.dim() == 4 && ((dw.size(0) == g.K && dw.size(1) == g.C && dw.size(2) == R &&
                                         dw.is_contiguous(at::MemoryFormat::ChannelsLast)) ||
                                        (dw.size(1) == R && dw.size(3) == g.C && dw.is_contiguous()));
    TORCH_CHECK(krsc, "out must be KRSC-contiguous (channels_last [K,C,R,S] or contiguous [K,R,S,C])");
  } else {
    dw = torch::empty({g.K, R, S, g.C}, x.options().dtype(at::kFloat));
    accumulate = false;
  }
  const float *isc, *ish;
  in_bn_ptrs(in_scale, in_shift, g.C, &isc, &ish);
  // the kernel family, tile config, splits and slab size: sdx_plan::plan_wgrad
  const sdx_plan::WgradPlan plan = sdx_plan::plan_wgrad(g, splits, cfg, accumulate, in_scale.has_value(), knobs());
  TORCH_CHECK(cfg != 9 || plan.ok, "conv_wgrad: cfg 9 needs a pad-1 3x3 conv of stride 1 or 2 on square images with output width in {4,8,16,32}, C,K % 64 == 0");
  TORCH_CHECK(cfg != 10 || plan.ok, "conv_wgrad: cfg 10 needs a 1x1 conv with K,C % 128 == 0 (stride 1, or stride s with H = s*P, W = s*Q), or stride 1 with K or C = 64");
  TORCH_CHECK(plan.ok, "conv_wgrad: no such tile config: ", cfg);
  torch::Tensor part;
  if (plan.slab_elems > 0) part = torch::empty({plan.slab_elems}, x.options().dtype(at::kFloat));
  float* pp = part.defined() ? part.data_ptr<float>() : nullptr;
  const int acc = accumulate ? 1 : 0;
  if (plan.family == sdx_plan::WGRAD_1X1)
    check_hip(launch_wgrad1x1(g, plan, dy.data_ptr(), x.data_ptr(), pp, dw.data_ptr<float>(), acc, cur_stream()),
              "conv_wgrad(1x1)");
  else if (plan.family == sdx_plan::WGRAD_3X3)
    check_hip(launch_wgrad3x3(g, plan, dy.data_ptr(), x.data_ptr(), pp, dw.data_ptr<float>(), acc, cur_stream()),
              "conv_wgrad(3x3)");
  else
    check_hip(launch_conv_wgrad(g, plan, dy.data_ptr(), x.data_ptr(), pp, dw.data_ptr<float>(), acc, cur_stream(), isc,
                                ish),
              "conv_wgrad");
  // a split-K slab whose reduction was queued (splitk_defer_begin) stays alive until the side
  // stream is joined (side_stash), i.e. past its deferred reduction launch
  if (part.defined() && splitk_deferring(cur_stream())) side_stash().push_back(part);
  return dw;
}

// SDX_SPLITK_MERGE=0 (or splitk_merge_set(False)): one split-K reduction launch per weight
// gradient (round-3 behaviour)
static std::atomic<int>& splitk_merge_flag() {
  static std::atomic<int> on{sdx_plan::env_flag("SDX_SPLITK_MERGE", true) ? 1 : 0};
  return on;
}
bool splitk_merge_enabled() { return splitk_merge_flag().load(std::memory_order_relaxed) != 0; }

namespace {

// block target of the dedicated 1x1 / 3x3 wgrad kernels' split heuristic: SDX_W3_BLOCKS
// (default 128, half the chip: the eager step runs them on the side stream beside the
// critical path). A step captured as one hipGraph chain runs them alone, in line, so
// PretrainEngine.enable_cuda_graph raises it to the whole chip for the capture
// (wgrad_block_target_set).
int64_t wgrad_block_target_set(int64_t n) {
  TORCH_CHECK(n >= 1 && n <= 4096, "block target in [1, 4096]");
  return std::exchange(knobs_mut().w3_blocks, (long long)n);
}

// host-only: no GPU call, no allocation (the plan functions of conv_plan.h under knobs())
pybind11::object conv_plan(int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t R, int64_t S, int64_t stride,
                           int64_t pad, bool dgrad, bool full, std::string kind, bool in_bn, bool bnstat,
                           int64_t cat_ch, int64_t splits, int64_t cfg, bool accumulate) {
  namespace py = pybind11;
  TORCH_CHECK(stride >= 1 && R >= 1 && S >= 1, "conv_plan: bad geometry");
  const ConvGeom g = conv_geom(N, H, W, C, K, R, S, stride, pad);
  if (kind.empty()) kind = dgrad ? "dgrad" : "fwd";
  auto tap_list = [](bool tap, const sdx_plan::TapGeom& t) {
    py::list l;
    const int v[8] = {t.t_rw, t.t_rs, t.t_imgs, t.t_is, t.t_hp, t.t_nhp, t.t_ky, t.t_nch};
    for (int i = 0; i < 8; ++i) l.append(tap ? v[i] : 0);
    return l;
  };
  py::dict d;
  if (kind == "fwd") {
    const sdx_plan::FwdPlan p = sdx_plan::plan_fwd(g, full ? cfg : -1, in_bn, knobs());
    if (!full) return py::make_tuple(p.cfg, p.m_tiles);
    py::list dep, one, grid;
    dep.append(p.depth); one.append(p.one ? 1 : 0); grid.append(p.m_tiles * p.n_tiles);
    d["cfg"] = p.cfg; d["mt"] = p.m_tiles; d["nt"] = p.n_tiles; d["ok"] = p.ok;
    d["depth"] = dep; d["one"] = one; d["grid"] = grid; d["tap"] = tap_list(p.tap && p.ok, p.tg);
    return d;
  }
  if (kind == "dgrad") {
    const sdx_plan::DgradPlan p = sdx_plan::plan_dgrad(g, full ? cfg : -1, (int)cat_ch, bnstat, knobs());
    if (!full) return py::make_tuple(p.cfg, g.stride == 1 ? (int64_t)p.rows : (int64_t)-1);
    py::list dep, one, grid, cmt, mmt;
    const int launches = p.merged ? (p.ncls > 0 ? 1 : 0) : p.ncls;
    for (int i = 0; i < launches; ++i) {
      dep.append(p.depth[i]); one.append(p.one[i] ? 1 : 0);
      grid.append(p.merged ? p.grid : p.cls[i].m_tiles * p.n_tiles);
    }
    for (int ph = 0; ph < g.stride; ++ph)      // per (ph, pw), 0 for an empty class
      for (int pw = 0; pw < g.stride; ++pw) {
        int mt = 0;
        for (int i = 0; i < p.ncls; ++i)
          if (p.cls[i].ph == ph && p.cls[i].pw == pw) mt = p.cls[i].m_tiles;
        cmt.append(mt);
      }
    if (p.merged)
      for (int i = 0; i < p.ncls; ++i) mmt.append(p.cls[i].m_tiles);   // the kernel's class order
    d["cfg"] = p.cfg; d["mt"] = p.rows; d["nt"] = p.n_tiles; d["ok"] = p.ok;
    d["merged"] = p.merged; d["class_mt"] = cmt; d["merged_mt"] = mmt;
    d["depth"] = dep; d["one"] = one; d["grid"] = grid; d["tap"] = tap_list(p.tap && p.ok, p.tg);
    return d;
  }
  TORCH_CHECK(kind == "wgrad" && full, "conv_plan: kind is fwd, dgrad or wgrad (wgrad: full=True)");
  const sdx_plan::WgradPlan p = sdx_plan::plan_wgrad(g, splits, cfg, accumulate, in_bn, knobs());
  TORCH_CHECK(p.ok, "conv_plan: cfg ", cfg, " does not run this weight gradient");
  static const char* const w1n[] = {"plain", "pipe", "pipe_gen", "big"};
  static const char* const w3n[] = {"plain", "pad", "s2", "s2pad"};
  const bool w1 = p.family == sdx_plan::WGRAD_1X1, w3 = p.family == sdx_plan::WGRAD_3X3;
  d["family"] = w1 ? "1x1" : w3 ? "3x3" : "generic";
  d["variant"] = w1 ? w1n[p.w1.kind] : w3 ? w3n[p.w3.kind] : "";
  d["cfg"] = p.cfg; d["steps"] = p.steps; d["per"] = p.per; d["splits"] = p.splits;
  d["tiles"] = p.tiles; d["slices"] = p.slices; d["slab_elems"] = p.slab_elems; d["direct"] = p.direct;
  d["grid"] = p.grid; d["depth"] = p.depth; d["bn"] = w1 ? p.w1.bn : 0; d["pairs"] = w1 && p.w1.pairs ? 1 : 0;
  d["slot"] = w3 ? p.w3.slot : 0; d["ok"] = true;
  return d;
}

// the Python-visible dgrads: positional arguments packed into DgradOpts / DgradStat
DgradOpts dgrad_opts(OptT out, OptT addend, OptT addend_mask, int64_t addend_sub) {
  DgradOpts o;
  o.out = out; o.addend = addend; o.addend_mask = addend_mask; o.addend_sub = addend_sub;
  return o;
}

}  // namespace

void register_conv(pybind11::module& m) {
  m.def("conv_fwd_bias", &conv_fwd_bias,
        "implicit-GEMM conv forward with a per-channel fp32 bias (+ReLU) epilogue (eval-mode folded BN)",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("stride"), pybind11::arg("pad"), pybind11::arg("bias"),
        pybind11::arg("relu"));
  m.def("wgrad1x1_pairs_set", [](int64_t on) { return (int64_t)std::exchange(knobs_mut().w1_pairs, on ? 1 : 0); },
        "pixel-pair 1x1 wgrad for 64-channel sides on (1) / off (0); returns the previous value", pybind11::arg("on"));
  m.def("igemm_one_k_set", [](int64_t mode, int64_t k) { return (int64_t)std::exchange(knobs_mut().one_k[mode == 0 ? 0 : 1], (int)k); },
        "longest GEMM reduction on the single-stage LDS-DMA loop (mode 0 fwd, 1 dgrad); returns the previous limit",
        pybind11::arg("mode"), pybind11::arg("k"));
  m.def("wgrad_block_target_set", &wgrad_block_target_set,
        "block target of the dedicated 1x1/3x3 wgrad kernels' split heuristic (SDX_W3_BLOCKS); returns the previous value",
        pybind11::arg("n"));
  m.def("wgrad1x1_big_set", [](int64_t mode) { return (int64_t)std::exchange(knobs_mut().w1_big, mode < 0 ? 0 : mode > 2 ? 2 : (int)mode); },
        "256-row LDS-DMA 1x1 wgrad kernel: 0 off, 1 long-split shapes (default), 2 every eligible shape; returns the previous value",
        pybind11::arg("mode"));
  m.def("conv_plan", &conv_plan,
        "host-only dispatch plan of a conv pass under the current knobs. Positional call: (tile config, "
        "statistics-slab M-tiles; -1 for strided dgrads) of a plain fwd / dgrad. full=True: the whole plan of "
        "kind 'fwd' | 'dgrad' | 'wgrad' as a dict (tests/test_conv_plan.py, tools/conv_plan_golden.py)",
        pybind11::arg("N"), pybind11::arg("H"), pybind11::arg("W"), pybind11::arg("C"), pybind11::arg("K"),
        pybind11::arg("R"), pybind11::arg("S"), pybind11::arg("stride"), pybind11::arg("pad"), pybind11::arg("dgrad"),
        pybind11::arg("full") = false, pybind11::arg("kind") = "", pybind11::arg("in_bn") = false,
        pybind11::arg("bnstat") = false, pybind11::arg("cat_ch") = 0, pybind11::arg("splits") = 0,
        pybind11::arg("cfg") = -1, pybind11::arg("accumulate") = false);
  // runtime switch of the tap-reuse loop (tests / in-process A/B)
  m.def("tap3_set", [](int64_t on) { return (int64_t)std::exchange(knobs_mut().tap3, (int)on); },
        "tap-reuse 3x3 conv loop on (1) / off (0) for auto tile selection; returns the previous value",
        pybind11::arg("on"));
  m.def("igemm_trace", [] {
    const int n = 2 * igemm_trace_slots();
    auto t = torch::empty({n}, torch::TensorOptions().dtype(at::kLong));
    check_hip(igemm_trace_copy(reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>()), cur_stream()),
              "igemm_trace");
    return t.view({2, n / 2});
  }, "diagnostic conv main-loop timeline of the last traced launch (SDX_IGEMM_TRACE=1)");
  m.def("conv_fwd",
        [](torch::Tensor x, torch::Tensor w, int64_t stride, int64_t pad, bool want_stats, int64_t cfg, OptT in_scale,
           OptT in_shift) { return conv_fwd(x, w, stride, pad, want_stats, cfg, in_scale, in_shift); },
        "implicit-GEMM conv forward (NHWC bf16) + BN stat slab [+ BN+ReLU prologue]",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("stride"), pybind11::arg("pad"),
        pybind11::arg("want_stats"), pybind11::arg("cfg") = -1, pybind11::arg("in_scale") = pybind11::none(),
        pybind11::arg("in_shift") = pybind11::none());
  m.def("conv_dgrad",
        [](torch::Tensor dy, torch::Tensor wt, int64_t H, int64_t W, int64_t stride, int64_t pad, int64_t cfg, OptT out,
           OptT addend, OptT addend_mask, int64_t addend_sub) {
          return conv_dgrad(dy, wt, H, W, stride, pad, cfg, dgrad_opts(out, addend, addend_mask, addend_sub));
        },
        "implicit-GEMM conv data gradient (strided: sub-pixel classes)",
        pybind11::arg("dy"), pybind11::arg("wt"), pybind11::arg("H"), pybind11::arg("W"), pybind11::arg("stride"),
        pybind11::arg("pad"), pybind11::arg("cfg") = -1, pybind11::arg("out") = pybind11::none(),
        pybind11::arg("addend") = pybind11::none(), pybind11::arg("addend_mask") = pybind11::none(),
        pybind11::arg("addend_sub") = 0);
  m.def("conv_dgrad_cat",
        [](torch::Tensor dy, torch::Tensor wt, torch::Tensor a2, torch::Tensor bias, int64_t cfg,
           c10::optional<torch::Tensor> ya, c10::optional<torch::Tensor> ma) -> std::vector<torch::Tensor> {
          DgradOpts o;
          o.cat = &a2;
          o.cat_bias = &bias;
          if (!ya.has_value()) return {conv_dgrad(dy, wt, dy.size(1), dy.size(2), 1, 0, cfg, o)};
          DgradStat st;
          st.ya = *ya;
          st.ma = *ma;
          return conv_dgrad_bnstat(dy, wt, dy.size(1), dy.size(2), 1, 0, cfg, o, st);
        },
        "K-concatenated stride-1 1x1 data gradient dx = dy·Wt[:, :K] + a2·Wt[:, K:] + bias (BN3 fold); with ya / ma "
        "also the BN-backward statistics slab (ReLU mask recomputed as ya > 0 is not applied: raw sums)",
        pybind11::arg("dy"), pybind11::arg("wt"), pybind11::arg("a2"), pybind11::arg("bias"), pybind11::arg("cfg") = -1,
        pybind11::arg("ya") = pybind11::none(), pybind11::arg("ma") = pybind11::none());
  m.def("conv_wgrad", &conv_wgrad, "implicit-GEMM conv weight gradient (fp32, split-K slab)", pybind11::arg("dy"),
        pybind11::arg("x"), pybind11::arg("R"), pybind11::arg("S"), pybind11::arg("stride"), pybind11::arg("pad"),
        pybind11::arg("splits") = 0, pybind11::arg("cfg") = -1, pybind11::arg("out") = pybind11::none(),
        pybind11::arg("accumulate") = false, pybind11::arg("in_scale") = pybind11::none(),
        pybind11::arg("in_shift") = pybind11::none());
  m.def("splitk_merge_set", [](bool on) { return (int64_t)splitk_merge_flag().exchange(on ? 1 : 0); },
        "merge a residual block's side-stream split-K reductions into one launch (returns the previous setting)");
  // test hooks of the deferred multi-tensor split-K reduction (splitk.hip), which block_bwd
  // alone reaches otherwise: host-only, on the current stream (a non-default one: the null
  // stream never defers). Slabs queued meanwhile live in side_stash until side_stash_release.
  m.def("splitk_defer_begin", [] { splitk_defer_begin(cur_stream()); },
        "queue the current stream's split-K reductions until splitk_defer_flush (tests)");
  m.def("splitk_defer_flush", [] { check_hip(splitk_flush(), "splitk_defer_flush"); },
        "issue the queued split-K reductions as one multi-tensor launch and stop deferring (tests)");
  m.def("splitk_defer_cancel", [] { splitk_defer_cancel(); }, "drop the queue and stop deferring (tests)");
  m.def("conv_dgrad_bnstat",
        [](torch::Tensor dy, torch::Tensor wt, int64_t H, int64_t W, int64_t stride, int64_t pad, int64_t cfg, OptT out,
           OptT addend, OptT addend_mask, torch::Tensor ya, torch::Tensor ma, OptT yb, OptT mb, OptT mask_bits,
           OptT msc, OptT msh, int64_t addend_sub, int store_masked, int64_t extra_rows) {
          return conv_dgrad_bnstat(dy, wt, H, W, stride, pad, cfg, dgrad_opts(out, addend, addend_mask, addend_sub),
                                   DgradStat{ya, ma, yb, mb, mask_bits, msc, msh, store_masked, extra_rows});
        },
        "dgrad + fused BN-backward statistics of dx (slab [rows][2|3][C] for bn_bwd_coef_slab)",
        pybind11::arg("dy"), pybind11::arg("wt"), pybind11::arg("H"), pybind11::arg("W"), pybind11::arg("stride"),
        pybind11::arg("pad"), pybind11::arg("cfg") = -1, pybind11::arg("out") = pybind11::none(),
        pybind11::arg("addend") = pybind11::none(), pybind11::arg("addend_mask") = pybind11::none(),
        pybind11::arg("ya"), pybind11::arg("ma"), pybind11::arg("yb") = pybind11::none(),
        pybind11::arg("mb") = pybind11::none(), pybind11::arg("mask_bits") = pybind11::none(),
        pybind11::arg("msc") = pybind11::none(), pybind11::arg("msh") = pybind11::none(),
        pybind11::arg("addend_sub") = 0, pybind11::arg("store_masked") = 0, pybind11::arg("extra_rows") = 0);
}

}  // namespace sdx_bind
