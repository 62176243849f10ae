// NNCLR loss (nnclr.hip): the top-1 search of both views' projections in the support queue (MoCo's two
// bf16 planes [2][K][D]), the cross-view InfoNCE of the neighbours against the predictions, and its
// backward for the predictions (ops/nnclr.py, losses/nnclr.py). The enqueue is moco_ops.cpp's.
#include "launchers.h"
#include "nnclr_plan.h"
#include "ops_decl.h"
#include "twoview_checks.h"

namespace sdx_bind {
namespace {

namespace np = sdx_nnclr;

// x [2r][D] fp32, the two views stacked -> (r, D)
std::pair<int64_t, int64_t> check_rows(const torch::Tensor& x, const char* name) {
  check_f32(x, name);
  TORCH_CHECK(x.dim() == 2 && x.size(0) >= 2 && x.size(0) % 2 == 0, name, " must be [2·rows][D], view-major");
  const int64_t r = x.size(0) / 2, D = x.size(1);
  TORCH_CHECK(D % 64 == 0 && D >= np::kMinD && D <= np::kMaxD && 2 * r * D < (1LL << 31), "nnclr: D = 64·j <= ",
              np::kMaxD);
  return {r, D};
}

// planes [2][2r][D] bf16 -> r
int64_t check_planes(const torch::Tensor& t, int64_t D, const torch::Tensor& like, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous() && t.dim() == 3 && t.size(0) == 2 &&
                  t.size(1) >= 2 && t.size(1) % 2 == 0 && t.size(2) == D && t.device() == like.device(),
              name, " must be a contiguous bf16 GPU tensor [2][2·rows][D] on one device");
  return t.size(1) / 2;
}

int64_t plane_dim(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() == 3 && t.size(2) % 64 == 0 && t.size(2) >= np::kMinD && t.size(2) <= np::kMaxD, name,
              ": D = 64·j <= ", np::kMaxD);
  return t.size(2);
}

// queue [2][K][D] bf16 -> K
int64_t check_queue(const torch::Tensor& queue, int64_t D, const torch::Tensor& like) {
  TORCH_CHECK(queue.is_cuda() && queue.scalar_type() == at::kBFloat16 && queue.is_contiguous() && queue.dim() == 3 &&
                  queue.size(0) == 2 && queue.size(2) == D && queue.device() == like.device(),
              "nnclr: queue must be a contiguous bf16 GPU tensor [2][K][D] on the rows' device");
  const int64_t K = queue.size(1);
  TORCH_CHECK(K % 64 == 0 && K >= np::kMinK && K <= np::kMaxK, "nnclr: K = 64·j in [", np::kMinK, ", ", np::kMaxK, "]");
  return K;
}

np::Plan plan(int64_t n, int64_t N, int64_t D, int64_t K, double temp, int64_t pos_offset) {
  TORCH_CHECK(temp > 0.0 && temp < 1e30, "nnclr: temp must be finite and > 0");
  TORCH_CHECK(pos_offset >= 0 && pos_offset + n <= N, "nnclr: rows pos_offset .. pos_offset + n of the N gathered rows");
  np::Plan pl{};
  TORCH_CHECK(np::make_plan(n, N, D, K, &pl), "nnclr: sizes");
  return pl;
}

uint16_t* bits(const torch::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

auto bf16_like(const torch::Tensor& x) { return x.options().dtype(at::kBFloat16); }

// z [2n][D], p [2N][D] or none -> (zhat [2n][D], zpl [2][2n][D], ppl [2][2N][D], rp [2N]); the last two are
// empty without p
std::vector<torch::Tensor> nnclr_prep(torch::Tensor z, c10::optional<torch::Tensor> p) {
  const auto [n, D] = check_rows(z, "z");
  c10::DeviceGuard dg(z.device());
  auto zhat = torch::empty_like(z);
  auto zpl = torch::empty({2, 2 * n, D}, bf16_like(z));
  check_hip(launch_nnclr_prep(z.data_ptr<float>(), (int)(2 * n), (int)D, zhat.data_ptr<float>(), bits(zpl), nullptr,
                              cur_stream()),
            "nnclr_prep");
  auto ppl = torch::empty({0}, bf16_like(z)), rp = torch::empty({0}, z.options());
  if (p.has_value()) {
    const auto [N, Dp] = check_rows(*p, "p");
    TORCH_CHECK(Dp == D && p->device() == z.device() && N >= n, "nnclr: p must be [2N][D] on z's device, N >= n");
    ppl = torch::empty({2, 2 * N, D}, bf16_like(z));
    rp = torch::empty({2 * N}, z.options());
    check_hip(launch_nnclr_prep(p->data_ptr<float>(), (int)(2 * N), (int)D, nullptr, bits(ppl), rp.data_ptr<float>(),
                                cur_stream()),
              "nnclr_prep");
  }
  return {zhat, zpl, ppl, rp};
}

// -> (idx [2n] int32, sim [2n], nnpl [2][2n][D] = queue[:, idx])
std::vector<torch::Tensor> nnclr_search(torch::Tensor zpl, torch::Tensor queue) {
  const int64_t D = plane_dim(zpl, "zpl");
  const int64_t n = check_planes(zpl, D, zpl, "zpl");
  const int64_t K = check_queue(queue, D, zpl);
  const np::Plan pl = plan(n, n, D, K, 1.0, 0);
  c10::DeviceGuard dg(zpl.device());
  auto i32 = zpl.options().dtype(at::kInt);
  auto pair = torch::empty({(int64_t)pl.search.splits, 2 * n, 2}, i32);
  auto idx = torch::empty({2 * n}, i32);
  auto sim = torch::empty({2 * n}, zpl.options().dtype(at::kFloat));
  auto nnpl = torch::empty_like(zpl);
  check_hip(launch_nnclr_search(bits(zpl), bits(queue), (int)n, (int)D, (int)K, pair.data_ptr<int>(),
                                idx.data_ptr<int>(), sim.data_ptr<float>(), bits(nnpl), cur_stream()),
            "nnclr_search");
  return {idx, sim, nnpl};
}

// -> (loss [1] of this rank's 2n rows over 2N, lse [2n], part [splits][2n][2])
std::vector<torch::Tensor> nnclr_sweep_fwd(torch::Tensor nnpl, torch::Tensor ppl, double temp, int64_t pos_offset) {
  const int64_t D = plane_dim(nnpl, "nnpl");
  const int64_t n = check_planes(nnpl, D, nnpl, "nnpl");
  const int64_t N = check_planes(ppl, D, nnpl, "ppl");
  const np::Plan pl = plan(n, N, D, np::kMinK, temp, pos_offset);
  c10::DeviceGuard dg(nnpl.device());
  auto f32 = nnpl.options().dtype(at::kFloat);
  auto part = torch::empty({(int64_t)pl.fwd.splits, 2 * n, 2}, f32);
  auto lse = torch::empty({2 * n}, f32);
  auto term = torch::empty({2 * n}, nnpl.options().dtype(at::kDouble));
  auto loss = torch::empty({1}, f32);
  check_hip(launch_nnclr_fwd(bits(nnpl), bits(ppl), (int)n, (int)N, (int)D, temp, (int)pos_offset,
                             part.data_ptr<float>(), lse.data_ptr<float>(), term.data_ptr<double>(),
                             loss.data_ptr<float>(), cur_stream()),
            "nnclr_fwd");
  return {loss, lse, part};
}

// the whole forward -> (loss, lse, idx, sim, zhat, nnpl, ppl, rp)
std::vector<torch::Tensor> nnclr_fwd(torch::Tensor z, torch::Tensor p, torch::Tensor queue, double temp,
                                     int64_t pos_offset) {
  auto pr = nnclr_prep(z, p);
  auto se = nnclr_search(pr[1], queue);
  auto sw = nnclr_sweep_fwd(se[2], pr[2], temp, pos_offset);
  return {sw[0], sw[1], se[0], se[1], pr[0], se[2], pr[2], pr[3]};
}

// g: the upstream scalar gradient (a GPU tensor of one element) -> (dp [2N][D], slab [splits][2N][D])
std::vector<torch::Tensor> nnclr_bwd(torch::Tensor nnpl, torch::Tensor ppl, torch::Tensor p, torch::Tensor rp,
                                     torch::Tensor lse, torch::Tensor g, double temp, int64_t pos_offset) {
  const auto [N, D] = check_rows(p, "p");
  const int64_t n = check_planes(nnpl, D, p, "nnpl");
  TORCH_CHECK(check_planes(ppl, D, p, "ppl") == N, "nnclr_bwd: ppl must hold p's rows");
  check_vec(rp, 2 * N, p, "rp");
  check_vec(lse, 2 * n, p, "lse");
  check_g(g, p);
  const np::Plan pl = plan(n, N, D, np::kMinK, temp, pos_offset);
  c10::DeviceGuard dg(p.device());
  auto slab = torch::empty({(int64_t)pl.bwd.splits, 2 * N, D}, p.options());
  auto dp = torch::empty_like(p);
  check_hip(launch_nnclr_bwd(bits(nnpl), bits(ppl), p.data_ptr<float>(), rp.data_ptr<float>(), lse.data_ptr<float>(),
                             g.data_ptr<float>(), (int)n, (int)N, (int)D, temp, (int)pos_offset,
                             slab.data_ptr<float>(), dp.data_ptr<float>(), cur_stream()),
            "nnclr_bwd");
  return {dp, slab};
}

bool nnclr_supported_op(int64_t n, int64_t N, int64_t D, int64_t K) { return np::supported(n, N, D, K); }

// -> (search splits, queue rows of a search span, forward splits, backward splits)
std::vector<int64_t> nnclr_splits(int64_t n, int64_t N, int64_t D, int64_t K) {
  np::Plan pl{};
  TORCH_CHECK(np::make_plan(n, N, D, K, &pl), "nnclr: sizes");
  return {pl.search.splits, (int64_t)pl.search.span_tiles * np::kTileRows, pl.fwd.splits, pl.bwd.splits};
}

}  // namespace

void register_nnclr(pybind11::module& m) {
  namespace py = pybind11;
  m.def("nnclr_supported", &nnclr_supported_op, "shapes the NNCLR kernels take", py::arg("n"), py::arg("N"),
        py::arg("D"), py::arg("K"));
  m.def("nnclr_splits", &nnclr_splits, "(search splits, rows of a search span, forward splits, backward splits)",
        py::arg("n"), py::arg("N"), py::arg("D"), py::arg("K"));
  m.def("nnclr_prep", &nnclr_prep, "(zhat, planes of zhat, planes of phat, 1/‖p‖)", py::arg("z"),
        py::arg("p") = py::none());
  m.def("nnclr_search", &nnclr_search, "(idx int32, similarity, planes of queue[idx]) for the planes of zhat",
        py::arg("zpl"), py::arg("queue"));
  m.def("nnclr_sweep_fwd", &nnclr_sweep_fwd, "(loss, lse, (max, sumexp) partials [splits][2n][2])", py::arg("nnpl"),
        py::arg("ppl"), py::arg("temp") = 0.1, py::arg("pos_offset") = 0);
  m.def("nnclr_fwd", &nnclr_fwd, "NNCLR loss forward: (loss, lse, idx, sim, zhat, nnpl, ppl, 1/‖p‖)", py::arg("z"),
        py::arg("p"), py::arg("queue"), py::arg("temp") = 0.1, py::arg("pos_offset") = 0);
  m.def("nnclr_bwd", &nnclr_bwd, "NNCLR loss backward: (dp [2N][D], the per-split dphat slabs)", py::arg("nnpl"),
        py::arg("ppl"), py::arg("p"), py::arg("rp"), py::arg("lse"), py::arg("g"), py::arg("temp") = 0.1,
        py::arg("pos_offset") = 0);
}

}  // namespace sdx_bind
