// SwAV loss (swav.hip): prototype scores S_v = ẑ_v·Cᵀ of the two views, Sinkhorn-Knopp over
// exp(S/ε), the swapped soft-target cross-entropy and the backward (ops/swav.py, losses/swav.py).
// swav_fwd / swav_bwd are what the autograd node calls on one rank; the forward stages are also ops
// of their own, between which a multi-rank run all-reduces the prototype sums r.
#include "launchers.h"
#include "ops_decl.h"
#include "swav_plan.h"
#include "twoview_checks.h"

namespace sdx_bind {
namespace {

namespace sp = sdx_swav;

void check_hyper(double eps, double temp, int64_t iters) {
  auto ok = [](double w) { return w > 0.0 && w < 1e30; };
  TORCH_CHECK(ok(eps) && ok(temp) && iters >= 1, "swav: eps and temp must be finite and > 0, iters >= 1");
}

// S or dS [2n][Kp] for K prototypes -> n
int64_t check_scores(const torch::Tensor& S, int64_t K, const char* name) {
  check_f32(S, name);
  TORCH_CHECK(S.dim() == 2 && S.size(0) % 2 == 0 && S.size(1) == sp::padded(K), name,
              " must be [2N][Kp], Kp = 64·ceil(K / 64)");
  const int64_t n = S.size(0) / 2;
  TORCH_CHECK(sp::supported(n, sp::kMinD, K), "swav: N >= 2, 2 <= K <= ", sp::kMaxK, ", 2N·Kp < 2^31");
  return n;
}

double total(int64_t n, int64_t n_total) {
  const double nt = n_total > 0 ? (double)n_total : (double)n;
  TORCH_CHECK(nt >= (double)n && nt < (double)(1 << 24), "swav: n_total counts at least this rank's rows");
  return nt;
}

// C's rows are normalised in place -> (zhat [2n][D], rnorm [2n])
std::vector<torch::Tensor> swav_prep(torch::Tensor z1, torch::Tensor z2, torch::Tensor C) {
  check_f32(z1, "z1");
  check_f32(z2, "z2");
  check_f32(C, "C");
  TORCH_CHECK(z1.dim() == 2 && z1.sizes() == z2.sizes() && C.dim() == 2 && C.size(1) == z1.size(1) &&
                  z1.device() == z2.device() && z1.device() == C.device(),
              "swav: z1, z2 [N][D] and C [K][D] on one device");
  const int64_t n = z1.size(0), D = z1.size(1), K = C.size(0);
  TORCH_CHECK(sp::supported(n, D, K), "swav: N >= 2, D = 64·j <= ", sp::kMaxD, ", 2 <= K <= ", sp::kMaxK);
  c10::DeviceGuard dg(z1.device());
  auto zhat = torch::empty({2 * n, D}, z1.options());
  auto rnorm = torch::empty({2 * n}, z1.options());
  check_hip(launch_swav_prep(z1.data_ptr<float>(), z2.data_ptr<float>(), C.data_ptr<float>(), (int)n, (int)D, (int)K,
                             zhat.data_ptr<float>(), rnorm.data_ptr<float>(), cur_stream()),
            "swav_prep");
  return {zhat, rnorm};
}

// -> (S [2n][Kp], part [2][ceil(n / 64)][K])
std::vector<torch::Tensor> swav_scores(torch::Tensor zhat, torch::Tensor C, double eps) {
  check_f32(zhat, "zhat");
  check_f32(C, "C");
  TORCH_CHECK(zhat.dim() == 2 && zhat.size(0) % 2 == 0 && C.dim() == 2 && C.size(1) == zhat.size(1) &&
                  zhat.device() == C.device(),
              "swav: zhat [2N][D] and C [K][D] on one device");
  const int64_t n = zhat.size(0) / 2, D = zhat.size(1), K = C.size(0);
  sp::Plan pl{};
  TORCH_CHECK(sp::make_plan(n, D, K, &pl), "swav: N >= 2, D = 64·j <= ", sp::kMaxD, ", 2 <= K <= ", sp::kMaxK);
  check_hyper(eps, 1.0, 1);
  c10::DeviceGuard dg(zhat.device());
  auto S = torch::empty({2 * n, (int64_t)pl.kp}, zhat.options());
  auto part = torch::empty({2, (int64_t)pl.s_tiles_m, K}, zhat.options());
  check_hip(launch_swav_scores(zhat.data_ptr<float>(), C.data_ptr<float>(), (int)n, (int)D, (int)K, eps,
                               S.data_ptr<float>(), part.data_ptr<float>(), cur_stream()),
            "swav_scores");
  return {S, part};
}

torch::Tensor swav_rowsum(torch::Tensor part) {
  check_f32(part, "part");
  TORCH_CHECK(part.dim() == 3 && part.size(0) == 2 && part.size(1) >= 1, "part must be [2][T][K]");
  const int64_t T = part.size(1), K = part.size(2);
  TORCH_CHECK(K >= sp::kMinK && K <= sp::kMaxK && T < (1 << 24), "swav_rowsum: sizes");
  c10::DeviceGuard dg(part.device());
  auto r = torch::empty({2, K}, part.options());
  check_hip(launch_swav_rowsum(part.data_ptr<float>(), (int)T, (int)K, r.data_ptr<float>(), cur_stream()),
            "swav_rowsum");
  return r;
}

// one iteration from the (all-reduced) r: last ? (u [2][K], c [2n]) : (part [2][ceil(n / 16)][K])
std::vector<torch::Tensor> swav_sinkhorn(torch::Tensor S, torch::Tensor r, double eps, bool last, int64_t n_total) {
  check_f32(r, "r");
  TORCH_CHECK(r.dim() == 2 && r.size(0) == 2 && r.device() == S.device(), "r must be [2][K] on S's device");
  const int64_t K = r.size(1);
  const int64_t n = check_scores(S, K, "S");
  const double nt = total(n, n_total);
  check_hyper(eps, 1.0, 1);
  c10::DeviceGuard dg(S.device());
  if (last) {
    auto u = torch::empty({2, K}, S.options());
    auto c = torch::empty({2 * n}, S.options());
    check_hip(launch_swav_sinkhorn(S.data_ptr<float>(), r.data_ptr<float>(), (int)n, (int)K, eps, nt, nullptr,
                                   u.data_ptr<float>(), c.data_ptr<float>(), cur_stream()),
              "swav_sinkhorn");
    return {u, c};
  }
  auto part = torch::empty({2, sp::ceil_div(n, sp::kStrip), K}, S.options());
  check_hip(launch_swav_sinkhorn(S.data_ptr<float>(), r.data_ptr<float>(), (int)n, (int)K, eps, nt,
                                 part.data_ptr<float>(), nullptr, nullptr, cur_stream()),
            "swav_sinkhorn");
  return {part};
}

// -> (loss [1] of this rank's rows, dS [2n][Kp], qsum [2n])
std::vector<torch::Tensor> swav_loss_grad(torch::Tensor S, torch::Tensor u, torch::Tensor c, double eps, double temp,
                                          int64_t n_total) {
  check_f32(u, "u");
  TORCH_CHECK(u.dim() == 2 && u.size(0) == 2 && u.device() == S.device(), "u must be [2][K] on S's device");
  const int64_t K = u.size(1);
  const int64_t n = check_scores(S, K, "S");
  check_vec(c, 2 * n, S, "c");
  const double nt = total(n, n_total);
  check_hyper(eps, temp, 1);
  c10::DeviceGuard dg(S.device());
  auto dS = torch::empty_like(S);
  auto qsum = torch::empty({2 * n}, S.options());
  auto rowloss = torch::empty({n}, S.options().dtype(at::kDouble));
  auto loss = torch::empty({1}, S.options());
  check_hip(launch_swav_loss_grad(S.data_ptr<float>(), u.data_ptr<float>(), c.data_ptr<float>(), (int)n, (int)K, eps,
                                  temp, nt, dS.data_ptr<float>(), qsum.data_ptr<float>(), rowloss.data_ptr<double>(),
                                  loss.data_ptr<float>(), cur_stream()),
            "swav_loss_grad");
  return {loss, dS, qsum};
}

// the whole forward on one rank -> (loss, zhat, rnorm, dS); C's rows are normalised in place
std::vector<torch::Tensor> swav_fwd(torch::Tensor z1, torch::Tensor z2, torch::Tensor C, double eps, double temp,
                                    int64_t iters) {
  check_hyper(eps, temp, iters);
  auto pr = swav_prep(z1, z2, C);
  auto sc = swav_scores(pr[0], C, eps);
  auto part = sc[1];
  std::vector<torch::Tensor> uc;
  for (int64_t it = 0; it < iters; ++it) {
    auto r = swav_rowsum(part);
    auto out = swav_sinkhorn(sc[0], r, eps, it + 1 == iters, 0);
    if (it + 1 == iters) uc = out; else part = out[0];
  }
  auto lg = swav_loss_grad(sc[0], uc[0], uc[1], eps, temp, 0);
  return {lg[0], pr[0], pr[1], lg[1]};
}

// g: the upstream scalar gradient (a GPU tensor of one element) -> (dz [2n][D], dC [K][D], dzhat [2n][D]);
// freeze: the dC GEMM is skipped and dC is zeros
std::vector<torch::Tensor> swav_bwd(torch::Tensor zhat, torch::Tensor rnorm, torch::Tensor C, torch::Tensor dS,
                                    torch::Tensor g, bool freeze) {
  check_f32(zhat, "zhat");
  check_f32(C, "C");
  TORCH_CHECK(zhat.dim() == 2 && C.dim() == 2 && C.size(1) == zhat.size(1) && zhat.device() == C.device(),
              "swav: zhat [2N][D] and C [K][D] on one device");
  const int64_t D = zhat.size(1), K = C.size(0);
  const int64_t n = check_scores(dS, K, "dS");
  TORCH_CHECK(zhat.size(0) == 2 * n && dS.device() == zhat.device() && sp::supported(n, D, K), "swav_bwd: sizes");
  check_vec(rnorm, 2 * n, zhat, "rnorm");
  check_g(g, zhat);
  c10::DeviceGuard dg(zhat.device());
  auto dzhat = torch::empty_like(zhat), dz = torch::empty_like(zhat);
  auto dC = freeze ? torch::zeros_like(C) : torch::empty_like(C);
  check_hip(launch_swav_bwd(zhat.data_ptr<float>(), rnorm.data_ptr<float>(), C.data_ptr<float>(),
                            dS.data_ptr<float>(), g.data_ptr<float>(), (int)n, (int)D, (int)K,
                            dzhat.data_ptr<float>(), dz.data_ptr<float>(), freeze ? nullptr : dC.data_ptr<float>(),
                            cur_stream()),
            "swav_bwd");
  return {dz, dC, dzhat};
}

bool swav_supported_op(int64_t n, int64_t D, int64_t K, int64_t iters) { return sp::supported(n, D, K, iters); }

}  // namespace

void register_swav(pybind11::module& m) {
  namespace py = pybind11;
  m.def("swav_supported", &swav_supported_op, "shapes the SwAV kernels take", py::arg("n"), py::arg("D"), py::arg("K"),
        py::arg("iters") = 1);
  m.def("swav_prep", &swav_prep, "(zhat [2N][D], rnorm [2N]); C's rows are normalised in place", py::arg("z1"),
        py::arg("z2"), py::arg("C"));
  m.def("swav_scores", &swav_scores, "(S [2N][Kp] = zhat·Cᵀ with zero padding, partials of the first prototype sum)",
        py::arg("zhat"), py::arg("C"), py::arg("eps") = 0.05);
  m.def("swav_rowsum", &swav_rowsum, "partials [2][T][K] -> r [2][K], added in ascending order", py::arg("part"));
  m.def("swav_sinkhorn", &swav_sinkhorn, "one Sinkhorn iteration: last ? (u, c) : (partials of the next r,)",
        py::arg("S"), py::arg("r"), py::arg("eps") = 0.05, py::arg("last") = false, py::arg("n_total") = 0);
  m.def("swav_loss_grad", &swav_loss_grad, "(loss of these rows, dS, Σ_k q per row)", py::arg("S"), py::arg("u"),
        py::arg("c"), py::arg("eps") = 0.05, py::arg("temp") = 0.1, py::arg("n_total") = 0);
  m.def("swav_fwd", &swav_fwd, "SwAV loss forward: (loss, zhat, rnorm, dS); C is normalised in place", py::arg("z1"),
        py::arg("z2"), py::arg("C"), py::arg("eps") = 0.05, py::arg("temp") = 0.1, py::arg("iters") = 3);
  m.def("swav_bwd", &swav_bwd, "SwAV loss backward: (dz [2N][D], dC, dzhat)", py::arg("zhat"), py::arg("rnorm"),
        py::arg("C"), py::arg("dS"), py::arg("g"), py::arg("freeze") = false);
}

}  // namespace sdx_bind
