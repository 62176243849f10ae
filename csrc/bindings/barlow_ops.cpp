// Barlow Twins loss (barlow.hip): batch-standardised cross-correlation C = ẑ1ᵀẑ2 / N, its loss and
// gradient G, and the backward through the standardisation (ops/barlow.py, losses/barlow.py).
// barlow_fwd / barlow_bwd are what the autograd node calls on one rank; the forward stages are
// also ops of their own, between which a multi-rank run all-reduces the column sums and C.
#include "barlow_plan.h"
#include "launchers.h"
#include "ops_decl.h"
#include "twoview_checks.h"

namespace sdx_bind {
namespace {

namespace bp = sdx_barlow;

// sums fp64 [2][2][D] = per view (Σz, Σz²); finalize: also stats [2][2][D] = per view (μ, rstd)
std::vector<torch::Tensor> barlow_colstats(torch::Tensor z1, torch::Tensor z2, double eps, bool finalize,
                                           int64_t n_total) {
  const double nt = total(z1, n_total);
  auto [n, D] = check_views("barlow", z1, z2, finalize ? nt : 2.0 + (double)z1.size(0));
  c10::DeviceGuard dg(z1.device());
  auto sums = torch::empty({2, 2, D}, z1.options().dtype(at::kDouble));
  torch::Tensor stats;
  if (finalize) stats = torch::empty({2, 2, D}, z1.options());
  check_hip(launch_bt_colstats(z1.data_ptr<float>(), z2.data_ptr<float>(), (int)n, (int)D, sums.data_ptr<double>(),
                               finalize ? stats.data_ptr<float>() : nullptr, finalize ? nt : (double)n, (float)eps,
                               cur_stream()),
            "barlow_colstats");
  if (!finalize) return {sums};
  return {sums, stats};
}

torch::Tensor barlow_stats_finalize(torch::Tensor sums, int64_t n_total, double eps) {
  TORCH_CHECK(sums.is_cuda() && sums.scalar_type() == at::kDouble && sums.is_contiguous() && sums.dim() == 3 &&
                  sums.size(0) == 2 && sums.size(1) == 2,
              "sums: contiguous fp64 GPU tensor [2][2][D]");
  const int64_t D = sums.size(2);
  TORCH_CHECK(D % 64 == 0 && D >= bp::kMinD && D <= bp::kMaxD && n_total >= 2, "barlow_stats_finalize: sizes");
  c10::DeviceGuard dg(sums.device());
  auto stats = torch::empty({2, 2, D}, sums.options().dtype(at::kFloat));
  check_hip(launch_bt_stats_finalize(sums.data_ptr<double>(), (int)D, (double)n_total, (float)eps,
                                     stats.data_ptr<float>(), cur_stream()),
            "barlow_stats_finalize");
  return stats;
}

torch::Tensor barlow_xcorr(torch::Tensor z1, torch::Tensor z2, torch::Tensor stats, int64_t n_total) {
  const double nt = total(z1, n_total);
  auto [n, D] = check_views("barlow", z1, z2, nt);
  check_vec(stats, 4 * D, z1, "stats");
  c10::DeviceGuard dg(z1.device());
  auto C = torch::empty({D, D}, z1.options());
  check_hip(launch_bt_xcorr(z1.data_ptr<float>(), z2.data_ptr<float>(), stats.data_ptr<float>(), (int)n, (int)D, nt,
                            C.data_ptr<float>(), cur_stream()),
            "barlow_xcorr");
  return C;
}

// C [D][D] becomes G in place -> (loss [], G (the same storage), r [2][D])
std::vector<torch::Tensor> barlow_loss_grad(torch::Tensor C, double lam, int64_t n_total) {
  check_f32(C, "C");
  TORCH_CHECK(C.dim() == 2 && C.size(0) == C.size(1), "C must be [D][D]");
  const int64_t D = C.size(0);
  bp::Plan pl{};
  TORCH_CHECK(n_total >= 2 && bp::make_plan(1, D, &pl), "barlow_loss_grad: D = 64·j with 64 <= D <= ", bp::kMaxD,
              ", N >= 2");
  c10::DeviceGuard dg(C.device());
  auto r = torch::empty({2, D}, C.options());
  auto loss = torch::empty({}, C.options());
  auto r2_part = torch::empty({pl.r2_partial_elems}, C.options());
  auto loss_part = torch::empty({pl.loss_blocks}, C.options().dtype(at::kDouble));
  check_hip(launch_bt_loss_grad(C.data_ptr<float>(), (int)D, (float)lam, (double)n_total, r.data_ptr<float>(),
                                loss.data_ptr<float>(), r2_part.data_ptr<float>(), loss_part.data_ptr<double>(),
                                cur_stream()),
            "barlow_loss_grad");
  return {loss, C, r};
}

// the whole forward on one rank: 4 launches -> (loss, G, stats, r)
std::vector<torch::Tensor> barlow_fwd(torch::Tensor z1, torch::Tensor z2, double lam, double eps) {
  auto st = barlow_colstats(z1, z2, eps, true, 0);
  auto C = barlow_xcorr(z1, z2, st[1], 0);
  auto out = barlow_loss_grad(C, lam, z1.size(0));
  return {out[0], out[1], st[1], out[2]};
}

// g: the upstream scalar gradient (a GPU tensor of one element) -> (dz1, dz2)
std::vector<torch::Tensor> barlow_bwd(torch::Tensor z1, torch::Tensor z2, torch::Tensor G, torch::Tensor stats,
                                      torch::Tensor r, torch::Tensor g, int64_t n_total) {
  const double nt = total(z1, n_total);
  auto [n, D] = check_views("barlow", z1, z2, nt);
  check_vec(G, D * D, z1, "G");
  check_vec(stats, 4 * D, z1, "stats");
  check_vec(r, 2 * D, z1, "r");
  check_g(g, z1);
  c10::DeviceGuard dg(z1.device());
  auto dz1 = torch::empty_like(z1), dz2 = torch::empty_like(z2);
  check_hip(launch_bt_bwd(z1.data_ptr<float>(), z2.data_ptr<float>(), G.data_ptr<float>(), stats.data_ptr<float>(),
                          r.data_ptr<float>(), g.data_ptr<float>(), (int)n, (int)D, nt, dz1.data_ptr<float>(),
                          dz2.data_ptr<float>(), cur_stream()),
            "barlow_bwd");
  return {dz1, dz2};
}

bool barlow_supported_op(int64_t n, int64_t D) { return bp::supported(n, D); }

}  // namespace

void register_barlow(pybind11::module& m) {
  namespace py = pybind11;
  m.def("barlow_supported", &barlow_supported_op, "shapes the Barlow Twins kernels take", py::arg("n"), py::arg("D"));
  m.def("barlow_colstats", &barlow_colstats, "per-column (Σz, Σz²) of both views in fp64 (+ (μ, rstd) when finalize)",
        py::arg("z1"), py::arg("z2"), py::arg("eps") = 1e-5, py::arg("finalize") = true, py::arg("n_total") = 0);
  m.def("barlow_stats_finalize", &barlow_stats_finalize, "(μ, rstd) of both views from the column sums of N rows",
        py::arg("sums"), py::arg("n_total"), py::arg("eps") = 1e-5);
  m.def("barlow_xcorr", &barlow_xcorr, "C = ẑ1ᵀ·ẑ2 / N over the given rows", py::arg("z1"), py::arg("z2"),
        py::arg("stats"), py::arg("n_total") = 0);
  m.def("barlow_loss_grad", &barlow_loss_grad, "C -> G in place; (loss, G, r)", py::arg("C"), py::arg("lam"),
        py::arg("n_total"));
  m.def("barlow_fwd", &barlow_fwd, "Barlow Twins loss forward: (loss, G, stats, r)", py::arg("z1"), py::arg("z2"),
        py::arg("lam"), py::arg("eps") = 1e-5);
  m.def("barlow_bwd", &barlow_bwd, "Barlow Twins loss backward: (dz1, dz2)", py::arg("z1"), py::arg("z2"),
        py::arg("G"), py::arg("stats"), py::arg("r"), py::arg("g"), py::arg("n_total") = 0);
}

}  // namespace sdx_bind
