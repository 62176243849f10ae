// VICReg loss (vicreg.hip): the symmetric auto-covariances C_v = x̄_vᵀx̄_v / (N − 1) of the two
// views' centred projections, the loss terms and the gradient G_v read off them, and the backward
// (ops/vicreg.py, losses/vicreg.py). vicreg_fwd / vicreg_bwd are what the autograd node calls on one
// rank; the forward stages are also ops of their own, between which a multi-rank run all-reduces
// the column sums and C.
#include "launchers.h"
#include "ops_decl.h"
#include "twoview_checks.h"
#include "vicreg_plan.h"

namespace sdx_bind {
namespace {

namespace vp = sdx_vicreg;

void check_sums(const torch::Tensor& sums, int64_t D, const char* what) {
  TORCH_CHECK(sums.is_cuda() && sums.scalar_type() == at::kDouble && sums.is_contiguous() && sums.dim() == 2 &&
                  sums.size(0) == 3 && sums.size(1) == D,
              what, ": sums must be a contiguous fp64 GPU tensor [3][D]");
}

void check_weights(double sim, double stdw, double cov, double eps) {
  auto ok = [](double w) { return w >= 0.0 && w < 1e30; };
  TORCH_CHECK(ok(sim) && ok(stdw) && ok(cov) && ok(eps), "vicreg: the weights and eps must be finite and >= 0");
}

// sums fp64 [3][D] = (Σz1, Σz2, Σ(z1 − z2)²); finalize: also mu [2][D]
std::vector<torch::Tensor> vicreg_colstats(torch::Tensor z1, torch::Tensor z2, bool finalize, int64_t n_total) {
  const double nt = total(z1, n_total);
  auto [n, D] = check_views("vicreg", z1, z2, finalize ? nt : 2.0 + (double)z1.size(0));
  c10::DeviceGuard dg(z1.device());
  auto sums = torch::empty({3, D}, z1.options().dtype(at::kDouble));
  torch::Tensor mu;
  if (finalize) mu = torch::empty({2, D}, z1.options());
  check_hip(launch_vic_colstats(z1.data_ptr<float>(), z2.data_ptr<float>(), (int)n, (int)D, sums.data_ptr<double>(),
                                finalize ? mu.data_ptr<float>() : nullptr, finalize ? nt : (double)n, cur_stream()),
            "vicreg_colstats");
  if (!finalize) return {sums};
  return {sums, mu};
}

torch::Tensor vicreg_stats_finalize(torch::Tensor sums, int64_t n_total) {
  TORCH_CHECK(sums.dim() == 2, "sums: [3][D]");
  const int64_t D = sums.size(1);
  check_sums(sums, D, "vicreg_stats_finalize");
  TORCH_CHECK(D % 64 == 0 && D >= vp::kMinD && D <= vp::kMaxD && n_total >= 2, "vicreg_stats_finalize: sizes");
  c10::DeviceGuard dg(sums.device());
  auto mu = torch::empty({2, D}, sums.options().dtype(at::kFloat));
  check_hip(launch_vic_stats_finalize(sums.data_ptr<double>(), (int)D, (double)n_total, mu.data_ptr<float>(),
                                      cur_stream()),
            "vicreg_stats_finalize");
  return mu;
}

torch::Tensor vicreg_cov(torch::Tensor z1, torch::Tensor z2, torch::Tensor mu, int64_t n_total) {
  const double nt = total(z1, n_total);
  auto [n, D] = check_views("vicreg", z1, z2, nt);
  check_vec(mu, 2 * D, z1, "mu");
  c10::DeviceGuard dg(z1.device());
  auto C = torch::empty({2, D, D}, z1.options());
  check_hip(launch_vic_cov(z1.data_ptr<float>(), z2.data_ptr<float>(), mu.data_ptr<float>(), (int)n, (int)D, nt,
                           C.data_ptr<float>(), cur_stream()),
            "vicreg_cov");
  return C;
}

// C [2][D][D] becomes G in place -> (loss [1], terms [3], G (the same storage), coef [2][D])
std::vector<torch::Tensor> vicreg_loss_grad(torch::Tensor C, torch::Tensor sums, double sim, double stdw, double cov,
                                            double eps, int64_t n_total) {
  check_f32(C, "C");
  TORCH_CHECK(C.dim() == 3 && C.size(0) == 2 && C.size(1) == C.size(2), "C must be [2][D][D]");
  const int64_t D = C.size(1);
  vp::Plan pl{};
  TORCH_CHECK(n_total >= 2 && n_total < (1 << 24) && vp::make_plan(1, D, &pl),
              "vicreg_loss_grad: D = 64·j with 64 <= D <= ", vp::kMaxD, ", N >= 2");
  check_sums(sums, D, "vicreg_loss_grad");
  TORCH_CHECK(sums.device() == C.device(), "vicreg_loss_grad: sums on C's device");
  check_weights(sim, stdw, cov, eps);
  c10::DeviceGuard dg(C.device());
  auto coef = torch::empty({2, D}, C.options());
  auto loss = torch::empty({1}, C.options());
  auto terms = torch::empty({3}, C.options());
  auto parts = torch::empty({2 * (int64_t)pl.loss_blocks}, C.options().dtype(at::kDouble));
  check_hip(launch_vic_loss_grad(C.data_ptr<float>(), sums.data_ptr<double>(), (int)D, sim, stdw, cov, (float)eps,
                                 (double)n_total, loss.data_ptr<float>(), terms.data_ptr<float>(),
                                 coef.data_ptr<float>(), parts.data_ptr<double>(), cur_stream()),
            "vicreg_loss_grad");
  return {loss, terms, C, coef};
}

// the whole forward on one rank: 4 launches -> (loss, terms, G, mu, coef)
std::vector<torch::Tensor> vicreg_fwd(torch::Tensor z1, torch::Tensor z2, double sim, double stdw, double cov,
                                      double eps) {
  check_weights(sim, stdw, cov, eps);
  auto st = vicreg_colstats(z1, z2, true, 0);
  auto C = vicreg_cov(z1, z2, st[1], 0);
  auto out = vicreg_loss_grad(C, st[0], sim, stdw, cov, eps, z1.size(0));
  return {out[0], out[1], out[2], st[1], out[3]};
}

// g: the upstream scalar gradient (a GPU tensor of one element) -> (dz1, dz2)
std::vector<torch::Tensor> vicreg_bwd(torch::Tensor z1, torch::Tensor z2, torch::Tensor G, torch::Tensor mu,
                                      torch::Tensor coef, torch::Tensor g, double sim, int64_t n_total) {
  const double nt = total(z1, n_total);
  auto [n, D] = check_views("vicreg", z1, z2, nt);
  check_vec(G, 2 * D * D, z1, "G");
  check_vec(mu, 2 * D, z1, "mu");
  check_vec(coef, 2 * D, z1, "coef");
  check_g(g, z1);
  check_weights(sim, 0.0, 0.0, 0.0);
  c10::DeviceGuard dg(z1.device());
  auto dz1 = torch::empty_like(z1), dz2 = torch::empty_like(z2);
  check_hip(launch_vic_bwd(z1.data_ptr<float>(), z2.data_ptr<float>(), G.data_ptr<float>(), mu.data_ptr<float>(),
                           coef.data_ptr<float>(), g.data_ptr<float>(), (int)n, (int)D, sim, nt, dz1.data_ptr<float>(),
                           dz2.data_ptr<float>(), cur_stream()),
            "vicreg_bwd");
  return {dz1, dz2};
}

bool vicreg_supported_op(int64_t n, int64_t D) { return vp::supported(n, D); }

}  // namespace

void register_vicreg(pybind11::module& m) {
  namespace py = pybind11;
  m.def("vicreg_supported", &vicreg_supported_op, "shapes the VICReg kernels take", py::arg("n"), py::arg("D"));
  m.def("vicreg_colstats", &vicreg_colstats, "per-column (Σz1, Σz2, Σ(z1 − z2)²) in fp64 (+ mu [2][D] when finalize)",
        py::arg("z1"), py::arg("z2"), py::arg("finalize") = true, py::arg("n_total") = 0);
  m.def("vicreg_stats_finalize", &vicreg_stats_finalize, "mu of both views from the column sums of N rows",
        py::arg("sums"), py::arg("n_total"));
  m.def("vicreg_cov", &vicreg_cov, "C_v = x̄_vᵀ·x̄_v / (N − 1) over the given rows, [2][D][D], symmetric bit for bit",
        py::arg("z1"), py::arg("z2"), py::arg("mu"), py::arg("n_total") = 0);
  m.def("vicreg_loss_grad", &vicreg_loss_grad, "C -> G in place; (loss, terms, G, coef)", py::arg("C"), py::arg("sums"),
        py::arg("sim"), py::arg("std"), py::arg("cov"), py::arg("eps"), py::arg("n_total"));
  m.def("vicreg_fwd", &vicreg_fwd, "VICReg loss forward: (loss, terms, G, mu, coef)", py::arg("z1"), py::arg("z2"),
        py::arg("sim") = 25.0, py::arg("std") = 25.0, py::arg("cov") = 1.0, py::arg("eps") = 1e-4);
  m.def("vicreg_bwd", &vicreg_bwd, "VICReg loss backward: (dz1, dz2)", py::arg("z1"), py::arg("z2"), py::arg("G"),
        py::arg("mu"), py::arg("coef"), py::arg("g"), py::arg("sim"), py::arg("n_total") = 0);
}

}  // namespace sdx_bind
