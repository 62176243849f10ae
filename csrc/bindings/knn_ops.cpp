// Weighted k-NN evaluation (knn.hip): per-query top-k of Q·Bᵀ with a running list (the
// Nq x Nb matrix is never written) and the exp(sim/T) class vote with top-1/5 hits
// (ops/knn.py, engine/knn.py).
#include "conv_internal.h"
#include "knn_plan.h"
#include "launchers.h"
#include "ops_decl.h"

hipError_t launch_knn_topk(const float* q, const float* bank, int nq, int nb, int D, int k, int n_split,
                           int rows_per_split, float* slab_s, int* slab_i, float* sims, int* idx, hipStream_t s);
hipError_t launch_knn_vote(const float* sims, const int* idx, const int64_t* bank_labels, const int64_t* labels,
                           int nq, int nb, int k, int n_cls, float T, float* scores, float* rowhit, float* stats,
                           hipStream_t s);

namespace sdx_bind {
namespace {

void check_rows(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.dim() == 2 && t.is_contiguous(), name,
              " must be a contiguous fp32 GPU tensor [rows][D]");
}

// The k largest q·b per query, by similarity descending, then bank index ascending.
// Returns [sims [Nq][k] fp32, idx [Nq][k] int32]. n_split = 0: a split count that fills the chip.
std::vector<torch::Tensor> knn_topk(torch::Tensor q, torch::Tensor bank, int64_t k, int64_t n_split) {
  check_rows(q, "q");
  check_rows(bank, "bank");
  const int64_t nq = q.size(0), nb = bank.size(0), D = q.size(1);
  TORCH_CHECK(bank.size(1) == D, "knn_topk: q [Nq][D] and bank [Nb][D] must share D");
  TORCH_CHECK(bank.device() == q.device(), "knn_topk: q and bank on one device");
  TORCH_CHECK(sdx_knn::dim_supported(D), "knn_topk: D = 64·2^j <= 2048");
  TORCH_CHECK(nq >= 1 && nb >= 1, "knn_topk: empty q or bank");
  TORCH_CHECK(k >= 1 && k <= sdx_knn::kMaxK && k <= nb, "knn_topk: 1 <= k <= min(", sdx_knn::kMaxK, ", Nb)");
  TORCH_CHECK(n_split >= 0 && n_split <= sdx_knn::kMaxSplits, "knn_topk: 0 <= n_split <= ", sdx_knn::kMaxSplits);
  TORCH_CHECK(nq * D < (1LL << 31) && nb * D < (1LL << 31) && nq * k < (1LL << 31), "knn_topk: sizes");
  sdx_knn::Plan plan{};
  TORCH_CHECK(sdx_knn::make_plan(nq, nb, k, n_split, &plan), "knn_topk: sizes");
  c10::DeviceGuard dg(q.device());
  auto fo = q.options();
  auto io = q.options().dtype(at::kInt);
  auto sims = torch::empty({nq, k}, fo);
  auto idx = torch::empty({nq, k}, io);
  torch::Tensor slab_s, slab_i;
  if (plan.n_split > 1) {
    slab_s = torch::empty({plan.slab_elems}, fo);
    slab_i = torch::empty({plan.slab_elems}, io);
  }
  check_hip(launch_knn_topk(q.data_ptr<float>(), bank.data_ptr<float>(), (int)nq, (int)nb, (int)D, (int)k,
                            plan.n_split, plan.rows_per_split, plan.n_split > 1 ? slab_s.data_ptr<float>() : nullptr,
                            plan.n_split > 1 ? slab_i.data_ptr<int>() : nullptr, sims.data_ptr<float>(),
                            idx.data_ptr<int>(), cur_stream()),
            "knn_topk");
  return {sims, idx};
}

// The split count knn_topk launches for n_split = 0 (profiles, tests)
int64_t knn_num_splits(int64_t nq, int64_t nb, int64_t k, int64_t n_split) {
  sdx_knn::Plan plan{};
  TORCH_CHECK(sdx_knn::make_plan(nq, nb, k, n_split, &plan), "knn_num_splits: sizes");
  return plan.n_split;
}

// scores[q][c] = Σ_{neighbours of class c} exp(sim/T) in list order; with labels also
// stats [2] = (hits@1, hits@5) by the rank rule #{c : score_c > score_label} < kk.
std::vector<torch::Tensor> knn_vote(torch::Tensor sims, torch::Tensor idx, torch::Tensor bank_labels, int64_t n_cls,
                                    double T, OptT labels) {
  check_rows(sims, "sims");
  const int64_t nq = sims.size(0), k = sims.size(1), nb = bank_labels.numel();
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kInt && idx.is_contiguous() && idx.dim() == 2 &&
                  idx.size(0) == nq && idx.size(1) == k,
              "idx must be a contiguous int32 GPU tensor of the shape of sims");
  TORCH_CHECK(bank_labels.is_cuda() && bank_labels.scalar_type() == at::kLong && bank_labels.is_contiguous() &&
                  bank_labels.dim() == 1,
              "bank_labels: int64 [Nb]");
  TORCH_CHECK(idx.device() == sims.device() && bank_labels.device() == sims.device(), "knn_vote: one device");
  TORCH_CHECK(nq >= 1 && k >= 1 && k <= sdx_knn::kMaxK, "knn_vote: 1 <= k <= ", sdx_knn::kMaxK);
  TORCH_CHECK(nb >= 1 && nb < (1LL << 31), "knn_vote: bank size");
  TORCH_CHECK(n_cls >= 1 && n_cls <= sdx_knn::kMaxClasses, "knn_vote: 1 <= n_cls <= ", sdx_knn::kMaxClasses);
  TORCH_CHECK(T > 0.0, "knn_vote: T > 0");
  TORCH_CHECK(nq * n_cls < (1LL << 31) && nq * k < (1LL << 31), "knn_vote: sizes");
  if (labels.has_value())
    TORCH_CHECK(labels->is_cuda() && labels->scalar_type() == at::kLong && labels->numel() == nq &&
                    labels->is_contiguous() && labels->device() == sims.device(),
                "labels: int64 [Nq]");
  c10::DeviceGuard dg(sims.device());
  auto fo = sims.options();
  auto scores = torch::empty({nq, n_cls}, fo);
  auto stats = torch::zeros({2}, fo);
  torch::Tensor rowhit;
  if (labels.has_value()) rowhit = torch::empty({nq, 2}, fo);
  check_hip(launch_knn_vote(sims.data_ptr<float>(), idx.data_ptr<int>(), bank_labels.data_ptr<int64_t>(),
                            labels.has_value() ? labels->data_ptr<int64_t>() : nullptr, (int)nq, (int)nb, (int)k,
                            (int)n_cls, (float)T, scores.data_ptr<float>(),
                            labels.has_value() ? rowhit.data_ptr<float>() : nullptr, stats.data_ptr<float>(),
                            cur_stream()),
            "knn_vote");
  return {scores, stats};
}

}  // namespace

void register_knn(pybind11::module& m) {
  m.def("knn_topk", &knn_topk, "per-query top-k of q·bankᵀ (similarity descending, then index ascending)",
        pybind11::arg("q"), pybind11::arg("bank"), pybind11::arg("k"), pybind11::arg("n_split") = 0);
  m.def("knn_num_splits", &knn_num_splits, "bank splits knn_topk launches", pybind11::arg("nq"), pybind11::arg("nb"),
        pybind11::arg("k"), pybind11::arg("n_split") = 0);
  m.def("knn_vote", &knn_vote, "exp(sim/T) class vote of k-NN lists (+ top-1/5 hit counts when labels are given)",
        pybind11::arg("sims"), pybind11::arg("idx"), pybind11::arg("bank_labels"), pybind11::arg("n_cls"),
        pybind11::arg("T"), pybind11::arg("labels") = pybind11::none());
}

}  // namespace sdx_bind
