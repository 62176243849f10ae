// BatchNorm projector head on the native path: L − 1 hidden layers Linear(bias=False) ->
// BatchNorm1d -> ReLU and a last Linear(bias=False), one host call per direction.
//
//   forward   fb = bf16(feat)                                   cast kernel (head.hip)
//             per hidden layer: (a, yb, μ, rstd) = hbn_fwd      ONE launch (head_bn.hip): GEMM +
//                                                               statistics + normalise + ReLU
//             z = a·W_lastᵀ   (fp32)                            FWD GEMM of the MLP head
//   backward  dzb = bf16(dz)
//             per layer, last to first:
//               da = dy_next·W_next                             DGRAD GEMM
//               (dy, a) = hbn_bwd(da, yb, μ, rstd, γ, β)        ONE launch; dγ, dβ into the sinks;
//                                                               a recomputed, not kept from forward
//               dW_next += dy_nextᵀ·a                           WGRAD GEMM (side stream)
//             dW_0 += dy_0ᵀ·fb; dfeat = dy_0·W_0  (fp32)
//
// Kept for backward per hidden layer: yb (bf16 [N][H]) and μ, rstd (fp32 [H]).
#include "head_bn_plan.h"
#include "head_gemm_ops.h"
#include "ops_decl.h"

#include <c10/hip/HIPGuard.h>

namespace sdx_bind {
namespace {

using TensorList = std::vector<torch::Tensor>;

void check_w2(const torch::Tensor& w, int64_t rows, int64_t cols, const char* name) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 && w.is_contiguous() && w.numel() == rows * cols, name,
              " must be a contiguous bf16 GPU tensor of ", rows, "x", cols, " elements");
}

const uint16_t* bf(const torch::Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
uint16_t* bf_mut(torch::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

// one hidden layer forward -> [a, yb, mu, rstd]
TensorList layer_fwd(const torch::Tensor& x, const torch::Tensor& w, const torch::Tensor& gamma,
                     const torch::Tensor& beta, torch::Tensor& rmean, torch::Tensor& rvar, double momentum,
                     double eps, int64_t strip) {
  check_2d(x, at::kBFloat16, "x");
  const int64_t N = x.size(0), K = x.size(1), H = gamma.numel();
  TORCH_CHECK(sdx_hbn::supported(N, K, H), "head_bn_layer_fwd: rows ", N, ", in ", K, ", out ", H,
              " outside the native range (2 <= rows <= 2048, in = 64j <= 8192, out = 32j <= 8192)");
  check_w2(w, H, K, "W");
  check_vec(gamma, H, "gamma");
  check_vec(beta, H, "beta");
  check_vec(rmean, H, "running_mean");
  check_vec(rvar, H, "running_var");
  TORCH_CHECK(momentum >= 0.0 && momentum <= 1.0 && eps > 0.0, "momentum in [0, 1] and eps > 0 required");
  auto yb = torch::empty({N, H}, x.options());
  auto a = torch::empty({N, H}, x.options());
  auto mu = torch::empty({H}, x.options().dtype(at::kFloat));
  auto rstd = torch::empty({H}, x.options().dtype(at::kFloat));
  HbnFwdArgs p{bf(x),         bf(w),           gamma.data_ptr<float>(), beta.data_ptr<float>(),
               rmean.data_ptr<float>(), rvar.data_ptr<float>(), bf_mut(yb), bf_mut(a),
               mu.data_ptr<float>(),    rstd.data_ptr<float>(), (int)N,     (int)K,
               (int)H,        (float)momentum, (float)eps};
  check_hip(launch_hbn_fwd(p, (int)strip, cur_stream()), "hbn_fwd");
  return {a, yb, mu, rstd};
}

// one hidden layer backward -> dy; dγ, dβ added into the sinks; a_out: the recomputed activation
torch::Tensor layer_bwd(const torch::Tensor& da, const torch::Tensor& yb, const torch::Tensor& mu,
                        const torch::Tensor& rstd, const torch::Tensor& gamma, const torch::Tensor& beta,
                        torch::Tensor& sink_gamma, torch::Tensor& sink_beta, torch::Tensor* a_out) {
  check_2d(da, at::kBFloat16, "da");
  check_2d(yb, at::kBFloat16, "yb");
  const int64_t N = yb.size(0), H = yb.size(1);
  TORCH_CHECK(da.size(0) == N && da.size(1) == H, "da / yb shapes differ");
  sdx_hbn::BwdPlan pl;
  TORCH_CHECK(sdx_hbn::make_bwd(N, H, &pl), "head_bn_layer_bwd: rows ", N, ", columns ", H,
              " outside the native range (2 <= rows <= 2048, columns = 32j <= 8192)");
  for (const auto* v : {&mu, &rstd, &gamma, &beta}) check_vec(*v, H, "mu / rstd / gamma / beta");
  check_vec(sink_gamma, H, "gamma sink");
  check_vec(sink_beta, H, "beta sink");
  auto dy = torch::empty({N, H}, da.options());
  if (a_out != nullptr) *a_out = torch::empty({N, H}, da.options());
  HbnBwdArgs p{bf(da),
               bf(yb),
               mu.data_ptr<float>(),
               rstd.data_ptr<float>(),
               gamma.data_ptr<float>(),
               beta.data_ptr<float>(),
               sink_gamma.data_ptr<float>(),
               sink_beta.data_ptr<float>(),
               bf_mut(dy),
               a_out != nullptr ? bf_mut(*a_out) : nullptr,
               (int)N,
               (int)H};
  check_hip(launch_hbn_bwd(p, cur_stream()), "hbn_bwd");
  return dy;
}

TensorList head_bn_layer_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor gamma, torch::Tensor beta,
                             torch::Tensor rmean, torch::Tensor rvar, double momentum, double eps, int64_t strip) {
  c10::DeviceGuard dg(x.device());
  return layer_fwd(x, w, gamma, beta, rmean, rvar, momentum, eps, strip);
}

torch::Tensor head_bn_layer_bwd(torch::Tensor da, torch::Tensor yb, torch::Tensor mu, torch::Tensor rstd,
                                torch::Tensor gamma, torch::Tensor beta, torch::Tensor sink_gamma,
                                torch::Tensor sink_beta) {
  c10::DeviceGuard dg(da.device());
  return layer_bwd(da, yb, mu, rstd, gamma, beta, sink_gamma, sink_beta, nullptr);
}

// can every hidden layer of a head with these sizes run on hbn_fwd / hbn_bwd?
bool head_bn_supported(int64_t rows, int64_t dim_in, int64_t hidden, int64_t layers) {
  return (layers == 2 || layers == 3) && sdx_hbn::supported(rows, dim_in, hidden) &&
         (layers == 2 || sdx_hbn::supported(rows, hidden, hidden));
}

// feat [N][D] fp32|bf16; ws: L weights bf16 [out][in]; gammas .. rvars: L − 1 fp32 vectors.
// Returns [z fp32 [N][O], fb bf16 [N][D], then per hidden layer yb, mu, rstd].
TensorList head_bn_fwd(torch::Tensor feat, TensorList ws, TensorList gammas, TensorList betas, TensorList rmeans,
                       TensorList rvars, double momentum, double eps) {
  TORCH_CHECK(feat.dim() == 2, "feat must be [N, D]");
  const size_t L = ws.size();
  TORCH_CHECK((L == 2 || L == 3) && gammas.size() == L - 1 && betas.size() == L - 1 && rmeans.size() == L - 1 &&
                  rvars.size() == L - 1,
              "head_bn_fwd: 2 or 3 weights and one gamma, beta, running_mean, running_var per hidden layer");
  feat = feat.contiguous();
  check_2d(feat, feat.scalar_type() == at::kBFloat16 ? at::kBFloat16 : at::kFloat, "feat");
  c10::DeviceGuard dg(feat.device());
  auto fb = to_bf16(feat);
  TensorList out{torch::Tensor(), fb};
  torch::Tensor x = fb;
  for (size_t i = 0; i + 1 < L; ++i) {
    auto r = layer_fwd(x, ws[i], gammas[i], betas[i], rmeans[i], rvars[i], momentum, eps, 0);
    x = r[0];
    out.insert(out.end(), r.begin() + 1, r.end());
  }
  const int64_t O = ws[L - 1].numel() / x.size(1);
  out[0] = gemm_fwd(x, ws[L - 1], const_vec(feat.device(), O, 0.f), false, true);
  return out;
}

// dz [N][O] fp32; saved: fb and per hidden layer yb, mu, rstd; wts: L dgrad layouts (Wᵀ, [in][out]);
// sws / sgs / sbs: the weight, γ and β gradient sinks. Returns dfeat fp32 [N][D].
// side (a stream handle, 0 = none): the weight gradients run on the wgrad side stream
torch::Tensor head_bn_bwd(torch::Tensor dz, torch::Tensor fb, TensorList ybs, TensorList mus, TensorList rstds,
                          TensorList gammas, TensorList betas, TensorList wts, TensorList sws, TensorList sgs,
                          TensorList sbs, int64_t side) {
  const size_t L = wts.size();
  TORCH_CHECK((L == 2 || L == 3) && sws.size() == L, "head_bn_bwd: 2 or 3 weights, one sink each");
  for (const auto* v : {&ybs, &mus, &rstds, &gammas, &betas, &sgs, &sbs})
    TORCH_CHECK(v->size() == L - 1, "head_bn_bwd: one entry per hidden layer required");
  dz = dz.contiguous();
  check_2d(dz, at::kFloat, "dz");
  check_2d(fb, at::kBFloat16, "fb");
  TORCH_CHECK(dz.size(0) == fb.size(0), "dz / fb rows");
  c10::DeviceGuard dg(dz.device());
  torch::Tensor dy = to_bf16(dz);   // the gradient of layer i + 1's GEMM output
  for (size_t i = L - 1; i-- > 0;) {
    const int64_t Hi = ybs[i].size(1);
    auto da = gemm_dgrad(dy, wts[i + 1], Hi, false, nullptr, nullptr);
    torch::Tensor a;
    auto dyi = layer_bwd(da, ybs[i], mus[i], rstds[i], gammas[i], betas[i], sgs[i], sbs[i], &a);
    if (side != 0) {
      // everything queued so far, then the listed tensors stay alive until the join (side_stream.cpp)
      auto guard = side_fork(side, dz.device(), {dy, a});
      gemm_wgrad(dy, a, sws[i + 1]);
    } else {
      gemm_wgrad(dy, a, sws[i + 1]);
    }
    dy = dyi;
  }
  if (side != 0) {
    auto guard = side_fork(side, dz.device(), {dy, fb});
    gemm_wgrad(dy, fb, sws[0]);
  } else {
    gemm_wgrad(dy, fb, sws[0]);
  }
  return gemm_dgrad(dy, wts[0], fb.size(1), true, nullptr, nullptr);
}

}  // namespace

void register_head_bn(pybind11::module& m) {
  namespace py = pybind11;
  m.def("head_bn_layer_fwd", &head_bn_layer_fwd,
        "Linear + BatchNorm1d + ReLU in one launch (head_bn.hip hbn_fwd) -> [a, yb, mu, rstd]; updates the running "
        "statistics in place",
        py::arg("x"), py::arg("w"), py::arg("gamma"), py::arg("beta"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("momentum") = 0.1, py::arg("eps") = 1e-5, py::arg("strip") = 0);
  m.def("head_bn_layer_bwd", &head_bn_layer_bwd,
        "BatchNorm1d + ReLU backward in one launch (hbn_bwd) -> dy; adds the gamma / beta gradients into the sinks",
        py::arg("da"), py::arg("yb"), py::arg("mu"), py::arg("rstd"), py::arg("gamma"), py::arg("beta"),
        py::arg("sink_gamma"), py::arg("sink_beta"));
  m.def("head_bn_supported", &head_bn_supported, py::arg("rows"), py::arg("dim_in"), py::arg("hidden"),
        py::arg("layers"));
  m.def("head_bn_fwd", &head_bn_fwd, "BatchNorm projector head forward -> [z fp32, fb bf16, (yb, mu, rstd) per layer]",
        py::arg("feat"), py::arg("ws"), py::arg("gammas"), py::arg("betas"), py::arg("running_means"),
        py::arg("running_vars"), py::arg("momentum") = 0.1, py::arg("eps") = 1e-5);
  m.def("head_bn_bwd", &head_bn_bwd, "BatchNorm projector head backward: gradients into the sinks, returns dfeat fp32",
        py::arg("dz"), py::arg("fb"), py::arg("ybs"), py::arg("mus"), py::arg("rstds"), py::arg("gammas"),
        py::arg("betas"), py::arg("wts"), py::arg("sws"), py::arg("sgs"), py::arg("sbs"), py::arg("side") = 0);
}

}  // namespace sdx_bind
