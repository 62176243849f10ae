// DINO loss (dino.hip): the cross-entropy between the teacher's centred softmax and the student's over K
// prototypes, both logit matrices streamed through MFMA tiles and never written, the backward to the
// student's rows and prototype weights, and the centre's EMA (ops/dino.py, losses/dino.py).
#include "dino_plan.h"
#include "launchers.h"
#include "ops_decl.h"
#include "twoview_checks.h"

namespace sdx_bind {
namespace {

namespace dp = sdx_dino;

// zs [2n][D] and vs [K][D] (or tensors shaped like them) -> the plan
dp::Plan check_shapes(const torch::Tensor& z, const torch::Tensor& v) {
  check_f32(z, "z");
  check_f32(v, "v");
  TORCH_CHECK(z.dim() == 2 && v.dim() == 2 && z.size(0) % 2 == 0 && z.size(1) == v.size(1) && z.device() == v.device(),
              "dino: rows [2N][D] (two views stacked) and prototypes [K][D] on one device");
  dp::Plan pl{};
  TORCH_CHECK(dp::make_plan(z.size(0) / 2, z.size(1), v.size(0), &pl), "dino: N >= 1 per view, D = 64·j <= ", dp::kMaxD,
              ", K = 64·j in [", dp::kMinK, ", ", dp::kMaxK, "]");
  return pl;
}

void check_like(const torch::Tensor& t, const torch::Tensor& like, const char* name) {
  check_f32(t, name);
  TORCH_CHECK(t.sizes() == like.sizes() && t.device() == like.device(), "dino: ", name, " has the wrong shape or device");
}

void check_planes(const torch::Tensor& t, int64_t rows, int64_t D, const torch::Tensor& like, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous() && t.dim() == 3 && t.size(0) == 2 &&
                  t.size(1) == rows && t.size(2) == D && t.device() == like.device(),
              "dino: ", name, " must be contiguous bf16 planes [2][", rows, "][", D, "] on the rows' device");
}

double check_total(const dp::Plan& pl, int64_t n_total, double ts, double tt) {
  const double nt = n_total > 0 ? (double)n_total : (double)pl.n;
  TORCH_CHECK(nt >= (double)pl.n && nt < (double)(1 << 24), "dino: n_total counts at least this rank's samples");
  TORCH_CHECK(ts > 0.0 && ts < 1e30 && tt > 0.0 && tt < 1e30, "dino: the temperatures must be finite and > 0");
  return nt;
}

const uint16_t* planes(const torch::Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
uint16_t* planes_mut(torch::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

// -> (zs_pl, zt_pl [2][rp][D], cs_pl, ct_pl [2][K][D], 1/‖zs‖ [2N], 1/‖vs‖ [K], zsum = Σ ẑ_t [D] fp64)
std::vector<torch::Tensor> dino_prep(torch::Tensor zs, torch::Tensor zt, torch::Tensor vs, torch::Tensor vt) {
  const dp::Plan pl = check_shapes(zs, vs);
  check_like(zt, zs, "zt");
  check_like(vt, vs, "vt");
  c10::DeviceGuard dg(zs.device());
  const auto bf = zs.options().dtype(at::kBFloat16), f64 = zs.options().dtype(at::kDouble);
  auto zs_pl = torch::empty({2, (int64_t)pl.rp, (int64_t)pl.d}, bf), zt_pl = torch::empty_like(zs_pl);
  auto cs_pl = torch::empty({2, (int64_t)pl.k, (int64_t)pl.d}, bf), ct_pl = torch::empty_like(cs_pl);
  auto rzs = torch::empty({2 * (int64_t)pl.n}, zs.options()), rvs = torch::empty({(int64_t)pl.k}, zs.options());
  auto rzt64 = torch::empty({2 * (int64_t)pl.n}, f64), zsum = torch::empty({(int64_t)pl.d}, f64);
  check_hip(launch_dino_prep(zs.data_ptr<float>(), zt.data_ptr<float>(), vs.data_ptr<float>(), vt.data_ptr<float>(), pl.n,
                             pl.d, pl.k, planes_mut(zs_pl), planes_mut(zt_pl), planes_mut(cs_pl), planes_mut(ct_pl),
                             rzs.data_ptr<float>(), rvs.data_ptr<float>(), rzt64.data_ptr<double>(),
                             zsum.data_ptr<double>(), cur_stream()),
            "dino_prep");
  return {zs_pl, zt_pl, cs_pl, ct_pl, rzs, rvs, zsum};
}

dp::Plan check_all_planes(int64_t n, const torch::Tensor& zs_pl, const torch::Tensor& zt_pl, const torch::Tensor& cs_pl,
                          const torch::Tensor& ct_pl, const torch::Tensor& center) {
  TORCH_CHECK(cs_pl.dim() == 3, "dino: cs_pl must be planes [2][K][D]");
  dp::Plan pl{};
  TORCH_CHECK(dp::make_plan(n, cs_pl.size(2), cs_pl.size(1), &pl), "dino: sizes");
  check_planes(cs_pl, pl.k, pl.d, cs_pl, "cs_pl");
  check_planes(ct_pl, pl.k, pl.d, cs_pl, "ct_pl");
  check_planes(zs_pl, pl.rp, pl.d, cs_pl, "zs_pl");
  check_planes(zt_pl, pl.rp, pl.d, cs_pl, "zt_pl");
  check_f32(center, "center");
  TORCH_CHECK(center.numel() == pl.k && center.device() == cs_pl.device(), "dino: center must hold K fp32 elements");
  return pl;
}

// n: samples per view on this rank -> (loss [1] of these rows over 2·n_total, lse_s [rp], lse_t [rp],
// part [5][k_splits][rp])
std::vector<torch::Tensor> dino_sweep_fwd(torch::Tensor zs_pl, torch::Tensor zt_pl, torch::Tensor cs_pl,
                                          torch::Tensor ct_pl, torch::Tensor center, int64_t n, double temp_s,
                                          double temp_t, int64_t n_total) {
  const dp::Plan pl = check_all_planes(n, zs_pl, zt_pl, cs_pl, ct_pl, center);
  const double nt = check_total(pl, n_total, temp_s, temp_t);
  c10::DeviceGuard dg(center.device());
  auto part = torch::empty({5, (int64_t)pl.k_splits, (int64_t)pl.rp}, center.options());
  auto lse_s = torch::empty({(int64_t)pl.rp}, center.options()), lse_t = torch::empty_like(lse_s);
  auto loss = torch::empty({1}, center.options());
  check_hip(launch_dino_fwd(planes(zs_pl), planes(zt_pl), planes(cs_pl), planes(ct_pl), center.data_ptr<float>(), pl.n,
                            pl.d, pl.k, temp_s, temp_t, nt, part.data_ptr<float>(), lse_s.data_ptr<float>(),
                            lse_t.data_ptr<float>(), loss.data_ptr<float>(), cur_stream()),
            "dino_fwd");
  return {loss, lse_s, lse_t, part};
}

// the whole forward -> (loss, lse_s, lse_t, zs_pl, zt_pl, cs_pl, ct_pl, rzs, rvs, zsum)
std::vector<torch::Tensor> dino_fwd(torch::Tensor zs, torch::Tensor zt, torch::Tensor vs, torch::Tensor vt,
                                    torch::Tensor center, double temp_s, double temp_t, int64_t n_total) {
  auto pr = dino_prep(zs, zt, vs, vt);
  auto sw = dino_sweep_fwd(pr[0], pr[1], pr[2], pr[3], center, zs.size(0) / 2, temp_s, temp_t, n_total);
  return {sw[0], sw[1], sw[2], pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[6]};
}

// g: the upstream scalar gradient (a GPU tensor of one element) -> (dz [2N][D], dV [K][D]); without
// want_dv (the prototypes are frozen) the prototype sweep is not launched and dV is an empty tensor
std::vector<torch::Tensor> dino_bwd(torch::Tensor zs, torch::Tensor vs, torch::Tensor zs_pl, torch::Tensor zt_pl,
                                    torch::Tensor cs_pl, torch::Tensor ct_pl, torch::Tensor rzs, torch::Tensor rvs,
                                    torch::Tensor center, torch::Tensor lse_s, torch::Tensor lse_t, torch::Tensor g,
                                    double temp_s, double temp_t, int64_t n_total, bool want_dv) {
  const dp::Plan pl = check_shapes(zs, vs);
  check_all_planes(pl.n, zs_pl, zt_pl, cs_pl, ct_pl, center);
  TORCH_CHECK(cs_pl.size(1) == pl.k && cs_pl.size(2) == pl.d && cs_pl.device() == zs.device(),
              "dino_bwd: the planes do not belong to these rows and prototypes");
  check_vec(rzs, 2 * (int64_t)pl.n, zs, "rzs");
  check_vec(rvs, pl.k, zs, "rvs");
  check_vec(lse_s, pl.rp, zs, "lse_s");
  check_vec(lse_t, pl.rp, zs, "lse_t");
  check_g(g, zs);
  const double nt = check_total(pl, n_total, temp_s, temp_t);
  c10::DeviceGuard dg(zs.device());
  auto zslab = torch::empty({(int64_t)pl.k_splits, (int64_t)pl.rp, (int64_t)pl.d}, zs.options());
  auto dz = torch::empty_like(zs);
  torch::Tensor vslab, dv = torch::empty({0}, zs.options());
  if (want_dv) {
    dv = torch::empty_like(vs);
    if (pl.r_splits > 1) vslab = torch::empty({(int64_t)pl.r_splits, (int64_t)pl.k, (int64_t)pl.d}, zs.options());
  }
  check_hip(launch_dino_bwd(zs.data_ptr<float>(), vs.data_ptr<float>(), planes(zs_pl), planes(zt_pl), planes(cs_pl),
                            planes(ct_pl), rzs.data_ptr<float>(), rvs.data_ptr<float>(), center.data_ptr<float>(),
                            lse_s.data_ptr<float>(), lse_t.data_ptr<float>(), g.data_ptr<float>(), pl.n, pl.d, pl.k,
                            temp_s, temp_t, nt, zslab.data_ptr<float>(),
                            vslab.defined() ? vslab.data_ptr<float>() : nullptr, dz.data_ptr<float>(),
                            want_dv ? dv.data_ptr<float>() : nullptr, cur_stream()),
            "dino_bwd");
  return {dz, dv};
}

// -> m·center + (1 − m)·(the column mean of the teacher logits over rows_total rows), from zsum = Σ ẑ_t
// over ALL ranks' rows
torch::Tensor dino_center(torch::Tensor vt, torch::Tensor zsum, torch::Tensor center, double m, int64_t rows_total) {
  check_f32(vt, "vt");
  check_f32(center, "center");
  TORCH_CHECK(vt.dim() == 2 && dp::supported(1, vt.size(1), vt.size(0)), "dino_center: vt must be [K][D] in range");
  TORCH_CHECK(zsum.is_cuda() && zsum.scalar_type() == at::kDouble && zsum.is_contiguous() && zsum.numel() == vt.size(1) &&
                  zsum.device() == vt.device(),
              "dino_center: zsum must hold D fp64 elements on vt's device");
  TORCH_CHECK(center.numel() == vt.size(0) && center.device() == vt.device(), "dino_center: center must hold K elements");
  TORCH_CHECK(m >= 0.0 && m <= 1.0 && rows_total >= 1, "dino_center: 0 <= m <= 1 and rows_total >= 1");
  c10::DeviceGuard dg(vt.device());
  auto out = torch::empty_like(center);
  check_hip(launch_dino_center(vt.data_ptr<float>(), zsum.data_ptr<double>(), center.data_ptr<float>(), (int)vt.size(0),
                               (int)vt.size(1), m, (double)rows_total, out.data_ptr<float>(), cur_stream()),
            "dino_center");
  return out;
}

bool dino_supported_op(int64_t n, int64_t D, int64_t K) { return dp::supported(n, D, K); }

// -> (spans of the prototype axis in the row sweeps, spans of the sample axis in the prototype sweep)
std::pair<int64_t, int64_t> dino_splits(int64_t n, int64_t D, int64_t K) {
  dp::Plan pl{};
  TORCH_CHECK(dp::make_plan(n, D, K, &pl), "dino: sizes");
  return {pl.k_splits, pl.r_splits};
}

}  // namespace

void register_dino(pybind11::module& m) {
  namespace py = pybind11;
  m.def("dino_supported", &dino_supported_op, "shapes the DINO kernels take", py::arg("n"), py::arg("D"), py::arg("K"));
  m.def("dino_splits", &dino_splits, "(prototype spans of the row sweeps, sample spans of the prototype sweep)",
        py::arg("n"), py::arg("D"), py::arg("K"));
  m.def("dino_prep", &dino_prep, "(zs, zt, cs, ct planes, 1/‖zs‖, 1/‖vs‖, Σ ẑ_t as fp64)", py::arg("zs"), py::arg("zt"),
        py::arg("vs"), py::arg("vt"));
  m.def("dino_sweep_fwd", &dino_sweep_fwd, "(loss, lse_s, lse_t, the 5-tuple partials [5][splits][rp]) from the planes",
        py::arg("zs_pl"), py::arg("zt_pl"), py::arg("cs_pl"), py::arg("ct_pl"), py::arg("center"), py::arg("n"),
        py::arg("temp_s") = 0.1, py::arg("temp_t") = 0.04, py::arg("n_total") = 0);
  m.def("dino_fwd", &dino_fwd, "DINO loss forward: (loss, lse_s, lse_t, the four planes, 1/‖zs‖, 1/‖vs‖, Σ ẑ_t)",
        py::arg("zs"), py::arg("zt"), py::arg("vs"), py::arg("vt"), py::arg("center"), py::arg("temp_s") = 0.1,
        py::arg("temp_t") = 0.04, py::arg("n_total") = 0);
  m.def("dino_bwd", &dino_bwd, "DINO loss backward: (dz [2N][D], dV [K][D] or an empty tensor)", py::arg("zs"),
        py::arg("vs"), py::arg("zs_pl"), py::arg("zt_pl"), py::arg("cs_pl"), py::arg("ct_pl"), py::arg("rzs"),
        py::arg("rvs"), py::arg("center"), py::arg("lse_s"), py::arg("lse_t"), py::arg("g"), py::arg("temp_s") = 0.1,
        py::arg("temp_t") = 0.04, py::arg("n_total") = 0, py::arg("want_dv") = true);
  m.def("dino_center", &dino_center, "m·center + (1 − m)·mean teacher logit per prototype, from Σ ẑ_t", py::arg("vt"),
        py::arg("zsum"), py::arg("center"), py::arg("m"), py::arg("rows_total"));
}

}  // namespace sdx_bind
