// Linear-probe classifier (linear_ce.hip): fused logits + cross-entropy + top-k hits, and
// the gradient + SGD update, for the native linear evaluation (ops/linear_probe.py;
// reference main_linear.py:166-244); linear_ce_sweep_step: G such classifiers with their own
// lr / wd on one feature batch (linear_ce_sweep.hip); ce_head_fwd / ce_head_bwd: the same classifier as a
// trainable node of the supervised model (ops/ce_head.py; reference main_ce.py), whose
// parameter gradients accumulate into the gradient sinks.
#include "conv_internal.h"
#include "launchers.h"
#include "ops_decl.h"

namespace sdx_bind {
namespace {

void check_f32(const torch::Tensor& t, std::vector<int64_t> shape, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.sizes() == shape, name,
              " must be a contiguous fp32 GPU tensor of shape ", shape);
}

// The row-indexed ops (*_rows): x is a feature bank [N][K] and labels its labels [N]; the batch is
// the bank rows rows[0..B) (int64, on the bank's device, values in [0, N): device-resident, so
// the values themselves are not checked here — the kernels clamp the address into the bank and
// the checked build traps). Returns the batch size: rows' length, or x's without rows.
int64_t batch_rows(const torch::Tensor& x, const torch::Tensor& labels, const OptT& rows) {
  TORCH_CHECK(x.dim() == 2, "x [B][K]");
  const int64_t N = x.size(0);
  if (!rows.has_value()) return N;
  TORCH_CHECK(rows->is_cuda() && rows->scalar_type() == at::kLong && rows->dim() == 1 && rows->is_contiguous() &&
                  rows->get_device() == x.get_device(),
              "rows: contiguous int64 [B] on the bank's device");
  TORCH_CHECK(N >= 1 && labels.numel() == N && labels.is_cuda() && labels.get_device() == x.get_device(),
              "rows: a bank x [N][K] with labels [N] on its device, N >= 1");
  return rows->numel();
}

const int64_t* rows_ptr(const OptT& rows) { return rows.has_value() ? rows->data_ptr<int64_t>() : nullptr; }

// the shape / dtype checks shared by linear_ce_step and the ce_head ops
void check_classifier(const torch::Tensor& x, const torch::Tensor& W, const torch::Tensor& b,
                      const torch::Tensor& labels, const OptT& rows = c10::nullopt) {
  TORCH_CHECK(x.dim() == 2 && W.dim() == 2, "x [B][K], W [C][K]");
  const int64_t N = x.size(0), K = x.size(1), C = W.size(0);
  check_f32(x, {N, K}, "x");
  check_f32(W, {C, K}, "W");
  check_f32(b, {C}, "b");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong && labels.numel() == N && labels.is_contiguous(),
              rows.has_value() ? "labels: int64 [N], one per bank row" : "labels: int64 [B]");
  const int64_t B = batch_rows(x, labels, rows);
  TORCH_CHECK(B >= 1 && linear_ce_supported((int)K, (int)C) && ((K / 64) & (K / 64 - 1)) == 0,
              "linear_ce: K = 64·2^j <= 2048, C <= 1024");
  TORCH_CHECK(B * C < (1LL << 31) && B * K < (1LL << 31), "linear_ce: sizes");
}

// One classifier batch. train: logits, the mean-CE gradient and the SGD update of (W, b)
// with momentum buffers (bufW, bufb; `first` = no momentum history yet); eval: logits only.
// Returns [logits [B][C], stats [3] = (Σ_rows CE, top-1 hits, top-5 hits)].
std::vector<torch::Tensor> linear_ce_step_impl(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                               torch::Tensor labels, OptT rows, OptT bufW, OptT bufb, double lr,
                                               double momentum, double wd, bool first, bool train) {
  check_classifier(x, W, b, labels, rows);
  const int64_t B = batch_rows(x, labels, rows), N = x.size(0), K = x.size(1), C = W.size(0);
  if (train) {
    TORCH_CHECK(bufW.has_value() && bufb.has_value(), "momentum buffers required for a training step");
    check_f32(*bufW, {C, K}, "bufW");
    check_f32(*bufb, {C}, "bufb");
  }
  c10::DeviceGuard dg(x.device());
  auto fo = x.options();
  auto logits = torch::empty({B, C}, fo);
  auto rowstat = torch::empty({B, 3}, fo);
  auto stats = torch::empty({3}, fo);
  torch::Tensor dz;
  if (train) dz = torch::empty({B, C}, fo);
  check_hip(launch_linear_ce_fwd(x.data_ptr<float>(), W.data_ptr<float>(), b.data_ptr<float>(),
                                 labels.data_ptr<int64_t>(), (int)B, (int)K, (int)C, (float)(1.0 / B),
                                 logits.data_ptr<float>(), train ? dz.data_ptr<float>() : nullptr,
                                 rowstat.data_ptr<float>(), cur_stream(), rows_ptr(rows), (long)N),
            "linear_ce_fwd");
  check_hip(launch_linear_ce_sgd(x.data_ptr<float>(), train ? dz.data_ptr<float>() : nullptr, (int)B, (int)K, (int)C,
                                 train ? W.data_ptr<float>() : nullptr, train ? b.data_ptr<float>() : nullptr,
                                 train ? bufW->data_ptr<float>() : nullptr, train ? bufb->data_ptr<float>() : nullptr,
                                 (float)lr, (float)momentum, (float)wd, first ? 1 : 0, rowstat.data_ptr<float>(),
                                 stats.data_ptr<float>(), cur_stream(), rows_ptr(rows), (long)N),
            "linear_ce_sgd");
  return {logits, stats};
}

std::vector<torch::Tensor> linear_ce_step(torch::Tensor x, torch::Tensor W, torch::Tensor b, torch::Tensor labels,
                                          OptT bufW, OptT bufb, double lr, double momentum, double wd, bool first,
                                          bool train) {
  return linear_ce_step_impl(x, W, b, labels, c10::nullopt, bufW, bufb, lr, momentum, wd, first, train);
}

// linear_ce_step on the bank rows `rows`: bit-identical to linear_ce_step(x[rows], ..., labels[rows], ...)
std::vector<torch::Tensor> linear_ce_step_rows(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                               torch::Tensor labels, torch::Tensor rows, OptT bufW, OptT bufb,
                                               double lr, double momentum, double wd, bool first, bool train) {
  return linear_ce_step_impl(x, W, b, labels, rows, bufW, bufb, lr, momentum, wd, first, train);
}

// Test-only: linear_ce_step's second launch alone, on a caller-supplied dz [B][C] and rowstat
// [B][3] (tests/test_gpu_aux_oracle.py feeds it integers, where every sum is exact). Updates W,
// b, bufW, bufb in place (contiguous fp32, views of a larger buffer allowed); returns stats [3].
torch::Tensor linear_ce_sgd_raw(torch::Tensor x, torch::Tensor dz, torch::Tensor W, torch::Tensor b,
                                torch::Tensor bufW, torch::Tensor bufb, double lr, double momentum, double wd,
                                bool first, torch::Tensor rowstat) {
  TORCH_CHECK(x.dim() == 2 && W.dim() == 2, "x [B][K], W [C][K]");
  const int64_t B = x.size(0), K = x.size(1), C = W.size(0);
  check_f32(x, {B, K}, "x");
  check_f32(W, {C, K}, "W");
  check_f32(b, {C}, "b");
  check_f32(dz, {B, C}, "dz");
  check_f32(bufW, {C, K}, "bufW");
  check_f32(bufb, {C}, "bufb");
  check_f32(rowstat, {B, 3}, "rowstat");
  TORCH_CHECK(B >= 1 && linear_ce_supported((int)K, (int)C) && ((K / 64) & (K / 64 - 1)) == 0,
              "linear_ce: K = 64·2^j <= 2048, C <= 1024");
  TORCH_CHECK(B * C < (1LL << 31) && B * K < (1LL << 31), "linear_ce: sizes");
  const int dev = x.get_device();
  for (const torch::Tensor* t : {&dz, &W, &b, &bufW, &bufb, &rowstat})
    TORCH_CHECK(t->get_device() == dev, "linear_ce_sgd_raw: one device");
  auto aligned = [](const torch::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr<float>()) % 16 == 0; };
  TORCH_CHECK(aligned(x) && aligned(W) && aligned(bufW), "linear_ce_sgd_raw: x, W and bufW must be 16-byte aligned");
  c10::DeviceGuard dg(x.device());
  auto stats = torch::empty({3}, x.options());
  check_hip(launch_linear_ce_sgd(x.data_ptr<float>(), dz.data_ptr<float>(), (int)B, (int)K, (int)C,
                                 W.data_ptr<float>(), b.data_ptr<float>(), bufW.data_ptr<float>(),
                                 bufb.data_ptr<float>(), (float)lr, (float)momentum, (float)wd, first ? 1 : 0,
                                 rowstat.data_ptr<float>(), stats.data_ptr<float>(), cur_stream()),
            "linear_ce_sgd_raw");
  return stats;
}

// One batch of a hyper-parameter sweep (linear_ce_sweep.hip): G classifiers W [G][C][K], b [G][C]
// on the same features x [B][K], head g with lrs[g] / wds[g]; momentum and `first` are shared.
// train: bufW [G][C][K], bufb [G][C]; eval: no buffers. Views of larger tensors are allowed when
// contiguous and 16-byte aligned. Everything is checked before anything is allocated or launched.
// Returns [logits [G][B][C], stats [G][3]]; head g is bit-identical to linear_ce_step alone.
std::vector<torch::Tensor> linear_ce_sweep_step_impl(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                                     torch::Tensor labels, OptT rows, OptT bufW, OptT bufb,
                                                     const std::vector<double>& lrs, double momentum,
                                                     const std::vector<double>& wds, bool first, bool train) {
  TORCH_CHECK(x.dim() == 2 && W.dim() == 3, "x [B][K], W [G][C][K]");
  const int64_t N = x.size(0), K = x.size(1), G = W.size(0), C = W.size(1);
  TORCH_CHECK(G >= 1 && G <= kLinearSweepMaxHeads, "linear_ce_sweep: 1 <= G <= ", kLinearSweepMaxHeads, ", got ", G);
  TORCH_CHECK((int64_t)lrs.size() == G && (int64_t)wds.size() == G, "linear_ce_sweep: ", G, " heads need ", G,
              " learning rates and weight decays, got ", lrs.size(), " and ", wds.size());
  check_f32(x, {N, K}, "x");
  check_f32(W, {G, C, K}, "W");
  check_f32(b, {G, C}, "b");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong && labels.numel() == N && labels.is_contiguous(),
              rows.has_value() ? "labels: int64 [N], one per bank row" : "labels: int64 [B]");
  const int64_t B = batch_rows(x, labels, rows);
  TORCH_CHECK(B >= 1 && linear_ce_sweep_supported((int)G, (int)K, (int)C),
              "linear_ce_sweep: K = 64·2^j <= 2048, 1 <= C <= 1024, B >= 1");
  TORCH_CHECK(G * B * C < (1LL << 31) && B * K < (1LL << 31) && G * C * K < (1LL << 31), "linear_ce_sweep: sizes");
  auto aligned = [](const torch::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr<float>()) % 16 == 0; };
  // (a bank is read in place at any 4-byte alignment)
  TORCH_CHECK((rows.has_value() || aligned(x)) && aligned(W), "linear_ce_sweep: x and W must be 16-byte aligned");
  const int dev = x.get_device();
  TORCH_CHECK(W.get_device() == dev && b.get_device() == dev && labels.get_device() == dev,
              "linear_ce_sweep: one device");
  if (train) {
    TORCH_CHECK(bufW.has_value() && bufb.has_value(), "momentum buffers required for a training step");
    check_f32(*bufW, {G, C, K}, "bufW");
    check_f32(*bufb, {G, C}, "bufb");
    TORCH_CHECK(bufW->get_device() == dev && bufb->get_device() == dev, "linear_ce_sweep: one device");
    TORCH_CHECK(aligned(*bufW), "linear_ce_sweep: bufW must be 16-byte aligned");
  }
  c10::DeviceGuard dg(x.device());
  auto fo = x.options();
  auto logits = torch::empty({G, B, C}, fo);
  auto rowstat = torch::empty({G, B, 3}, fo);
  auto stats = torch::empty({G, 3}, fo);
  torch::Tensor dz;
  if (train) dz = torch::empty({G, B, C}, fo);
  float lr[kLinearSweepMaxHeads], wd[kLinearSweepMaxHeads];
  for (int64_t g = 0; g < G; ++g) {
    lr[g] = (float)lrs[g];
    wd[g] = (float)wds[g];
  }
  check_hip(launch_linear_ce_sweep_fwd(x.data_ptr<float>(), W.data_ptr<float>(), b.data_ptr<float>(),
                                       labels.data_ptr<int64_t>(), (int)G, (int)B, (int)K, (int)C, (float)(1.0 / B),
                                       logits.data_ptr<float>(), train ? dz.data_ptr<float>() : nullptr,
                                       rowstat.data_ptr<float>(), cur_stream(), rows_ptr(rows), (long)N),
            "linear_ce_sweep_fwd");
  check_hip(launch_linear_ce_sweep_sgd(x.data_ptr<float>(), train ? dz.data_ptr<float>() : nullptr, (int)G, (int)B,
                                       (int)K, (int)C, train ? W.data_ptr<float>() : nullptr,
                                       train ? b.data_ptr<float>() : nullptr,
                                       train ? bufW->data_ptr<float>() : nullptr,
                                       train ? bufb->data_ptr<float>() : nullptr, lr, wd, (float)momentum,
                                       first ? 1 : 0, rowstat.data_ptr<float>(), stats.data_ptr<float>(),
                                       cur_stream(), rows_ptr(rows), (long)N),
            "linear_ce_sweep_sgd");
  return {logits, stats};
}

std::vector<torch::Tensor> linear_ce_sweep_step(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                                torch::Tensor labels, OptT bufW, OptT bufb, std::vector<double> lrs,
                                                double momentum, std::vector<double> wds, bool first, bool train) {
  return linear_ce_sweep_step_impl(x, W, b, labels, c10::nullopt, bufW, bufb, lrs, momentum, wds, first, train);
}

// linear_ce_sweep_step on the bank rows `rows`: bit-identical to the plain op on x[rows], labels[rows]
std::vector<torch::Tensor> linear_ce_sweep_step_rows(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                                     torch::Tensor labels, torch::Tensor rows, OptT bufW, OptT bufb,
                                                     std::vector<double> lrs, double momentum,
                                                     std::vector<double> wds, bool first, bool train) {
  return linear_ce_sweep_step_impl(x, W, b, labels, rows, bufW, bufb, lrs, momentum, wds, first, train);
}

// Training form, forward: [logits [B][C], dz [B][C] = (softmax − onehot) / B, rowstat [B][3],
// stats [3], loss []]. reduce: also sum the row statistics into stats / loss now (a forward
// that no backward follows); otherwise ce_head_bwd writes them.
std::vector<torch::Tensor> ce_head_fwd(torch::Tensor x, torch::Tensor W, torch::Tensor b, torch::Tensor labels,
                                       bool reduce) {
  check_classifier(x, W, b, labels);
  const int64_t B = x.size(0), K = x.size(1), C = W.size(0);
  c10::DeviceGuard dg(x.device());
  auto fo = x.options();
  auto logits = torch::empty({B, C}, fo);
  auto dz = torch::empty({B, C}, fo);
  auto rowstat = torch::empty({B, 3}, fo);
  auto stats = torch::empty({3}, fo);
  auto loss = torch::empty({}, fo);
  check_hip(launch_linear_ce_fwd(x.data_ptr<float>(), W.data_ptr<float>(), b.data_ptr<float>(),
                                 labels.data_ptr<int64_t>(), (int)B, (int)K, (int)C, (float)(1.0 / B),
                                 logits.data_ptr<float>(), dz.data_ptr<float>(), rowstat.data_ptr<float>(),
                                 cur_stream()),
            "ce_head_fwd");
  if (reduce)
    check_hip(launch_ce_head_bwd(nullptr, nullptr, nullptr, (int)B, (int)K, (int)C, nullptr, nullptr, nullptr, nullptr,
                                 rowstat.data_ptr<float>(), stats.data_ptr<float>(), loss.data_ptr<float>(),
                                 cur_stream()),
              "ce_head_stats");
  return {logits, dz, rowstat, stats, loss};
}

// the second label vector and the scalars of the soft-target ops (Mixup / CutMix / label smoothing)
void check_soft(const char* op, const torch::Tensor& labels2, int64_t B, int dev, double lam, double eps) {
  TORCH_CHECK(labels2.is_cuda() && labels2.scalar_type() == at::kLong && labels2.numel() == B &&
                  labels2.is_contiguous() && labels2.get_device() == dev,
              op, ": labels2: int64 [B] on x's device");
  TORCH_CHECK(lam >= 0.0 && lam <= 1.0, op, ": lam must be in [0, 1], got ", lam);
  TORCH_CHECK(eps >= 0.0 && (float)eps < 1.f, op, ": eps must be in [0, 1), got ", eps);
}

// ce_head_fwd with the soft target t_c = (1 − eps)·(lam·[c = labels] + (1 − lam)·[c = labels2]) + eps / C:
// the same outputs, hits counted against `labels`; the backward op is ce_head_bwd, unchanged.
// labels2 = labels, lam = 1, eps = 0 is bit-identical to ce_head_fwd.
std::vector<torch::Tensor> ce_head_fwd_soft(torch::Tensor x, torch::Tensor W, torch::Tensor b, torch::Tensor labels,
                                            torch::Tensor labels2, double lam, double eps, bool reduce) {
  check_classifier(x, W, b, labels);
  const int64_t B = x.size(0), K = x.size(1), C = W.size(0);
  check_soft("ce_head_fwd_soft", labels2, B, x.get_device(), lam, eps);
  c10::DeviceGuard dg(x.device());
  auto fo = x.options();
  auto logits = torch::empty({B, C}, fo);
  auto dz = torch::empty({B, C}, fo);
  auto rowstat = torch::empty({B, 3}, fo);
  auto stats = torch::empty({3}, fo);
  auto loss = torch::empty({}, fo);
  check_hip(launch_linear_ce_fwd_soft(x.data_ptr<float>(), W.data_ptr<float>(), b.data_ptr<float>(),
                                      labels.data_ptr<int64_t>(), labels2.data_ptr<int64_t>(), (float)lam, (float)eps,
                                      (int)B, (int)K, (int)C, (float)(1.0 / B), logits.data_ptr<float>(),
                                      dz.data_ptr<float>(), rowstat.data_ptr<float>(), cur_stream()),
            "ce_head_fwd_soft");
  if (reduce)
    check_hip(launch_ce_head_bwd(nullptr, nullptr, nullptr, (int)B, (int)K, (int)C, nullptr, nullptr, nullptr, nullptr,
                                 rowstat.data_ptr<float>(), stats.data_ptr<float>(), loss.data_ptr<float>(),
                                 cur_stream()),
              "ce_head_stats");
  return {logits, dz, rowstat, stats, loss};
}

// the teacher's logits and the scalars of the distillation ops (knowledge distillation)
void check_distill(const char* op, const torch::Tensor& teacher, int64_t B, int64_t C, int dev, double temp,
                   double alpha) {
  TORCH_CHECK(teacher.is_cuda() && teacher.scalar_type() == at::kFloat && teacher.is_contiguous() &&
                  teacher.dim() == 2 && teacher.size(0) == B && teacher.size(1) == C && teacher.get_device() == dev,
              op, ": teacher_logits: contiguous fp32 [B, C] = [", B, ", ", C, "] on x's device");
  const float tau = (float)temp;
  TORCH_CHECK(tau > 0.f && std::isfinite(tau) && std::isfinite(1.f / tau), op,
              ": temp must be finite and > 0 (in fp32, with its reciprocal), got ", temp);
  TORCH_CHECK(alpha >= 0.0 && alpha <= 1.0, op, ": alpha must be in [0, 1], got ", alpha);
}

// ce_head_fwd_soft with a teacher (distill_ce.h): loss = (1 − alpha)·soft CE + alpha·temp²·KL(softmax(
// teacher_logits / temp) ‖ softmax(logits / temp)), dz its gradient / B; the same five outputs, hits of
// the logits against `labels`; the backward op is ce_head_bwd, unchanged. alpha = 0 is bit-identical
// to ce_head_fwd_soft; with alpha = 1 a row whose label lies outside [0, C) is valid and scores no hit.
std::vector<torch::Tensor> ce_head_fwd_distill(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                               torch::Tensor labels, torch::Tensor labels2, double lam, double eps,
                                               torch::Tensor teacher_logits, double temp, double alpha, bool reduce) {
  const char* op = "ce_head_fwd_distill";
  check_classifier(x, W, b, labels);
  const int64_t B = x.size(0), K = x.size(1), C = W.size(0);
  check_soft(op, labels2, B, x.get_device(), lam, eps);
  check_distill(op, teacher_logits, B, C, x.get_device(), temp, alpha);
  c10::DeviceGuard dg(x.device());
  auto fo = x.options();
  auto logits = torch::empty({B, C}, fo);
  auto dz = torch::empty({B, C}, fo);
  auto rowstat = torch::empty({B, 3}, fo);
  auto stats = torch::empty({3}, fo);
  auto loss = torch::empty({}, fo);
  check_hip(launch_linear_ce_fwd_distill(x.data_ptr<float>(), W.data_ptr<float>(), b.data_ptr<float>(),
                                         labels.data_ptr<int64_t>(), labels2.data_ptr<int64_t>(), (float)lam,
                                         (float)eps, teacher_logits.data_ptr<float>(), (float)temp, (float)alpha,
                                         (int)B, (int)K, (int)C, (float)(1.0 / B), logits.data_ptr<float>(),
                                         dz.data_ptr<float>(), rowstat.data_ptr<float>(), cur_stream()),
            op);
  if (reduce)
    check_hip(launch_ce_head_bwd(nullptr, nullptr, nullptr, (int)B, (int)K, (int)C, nullptr, nullptr, nullptr, nullptr,
                                 rowstat.data_ptr<float>(), stats.data_ptr<float>(), loss.data_ptr<float>(),
                                 cur_stream()),
              "ce_head_stats");
  return {logits, dz, rowstat, stats, loss};
}

// Training form, backward (one launch): returns dX [B][K] = gout·dz·W (need_dx), accumulates
// dW += gout·dzᵀ·x and db += gout·Σ_b dz into the given destinations (contiguous fp32, views of
// a larger buffer allowed) and writes stats / loss from rowstat. gout: scalar fp32 GPU tensor.
c10::optional<torch::Tensor> ce_head_bwd(torch::Tensor x, torch::Tensor dz, torch::Tensor W, torch::Tensor gout,
                                         torch::Tensor rowstat, torch::Tensor stats, torch::Tensor loss, OptT dW,
                                         OptT db, bool need_dx) {
  TORCH_CHECK(x.dim() == 2 && W.dim() == 2, "x [B][K], W [C][K]");
  const int64_t B = x.size(0), K = x.size(1), C = W.size(0);
  check_f32(x, {B, K}, "x");
  check_f32(W, {C, K}, "W");
  check_f32(dz, {B, C}, "dz");
  check_f32(rowstat, {B, 3}, "rowstat");
  check_f32(stats, {3}, "stats");
  check_f32(loss, {}, "loss");
  TORCH_CHECK(gout.is_cuda() && gout.scalar_type() == at::kFloat && gout.numel() == 1, "gout: one fp32 GPU value");
  TORCH_CHECK(B >= 1 && linear_ce_supported((int)K, (int)C) && ((K / 64) & (K / 64 - 1)) == 0,
              "ce_head: K = 64·2^j <= 2048, C <= 1024");
  TORCH_CHECK(B * C < (1LL << 31) && B * K < (1LL << 31), "ce_head: sizes");
  TORCH_CHECK(dW.has_value() == db.has_value(), "ce_head_bwd: dW and db come together");
  if (dW.has_value()) {
    check_f32(*dW, {C, K}, "dW");
    check_f32(*db, {C}, "db");
    TORCH_CHECK(dW->get_device() == x.get_device() && db->get_device() == x.get_device(), "dW / db: x's device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(dW->data_ptr<float>()) % 16 == 0, "dW must be 16-byte aligned");
  }
  TORCH_CHECK(need_dx || dW.has_value(), "ce_head_bwd: nothing to compute");
  c10::DeviceGuard dg(x.device());
  c10::optional<torch::Tensor> dX;
  if (need_dx) dX = torch::empty({B, K}, x.options());
  check_hip(launch_ce_head_bwd(x.data_ptr<float>(), dz.data_ptr<float>(), W.data_ptr<float>(), (int)B, (int)K, (int)C,
                               gout.data_ptr<float>(), need_dx ? dX->data_ptr<float>() : nullptr,
                               dW.has_value() ? dW->data_ptr<float>() : nullptr,
                               db.has_value() ? db->data_ptr<float>() : nullptr, rowstat.data_ptr<float>(),
                               stats.data_ptr<float>(), loss.data_ptr<float>(), cur_stream()),
            "ce_head_bwd");
  return dX;
}

// ---- the MFMA classifier head (head_gemm.hip): the same ops on bf16x3 GEMMs ---------------
// Same argument lists and return tuples as their FMA siblings above; the wider range
// (K = 64·j <= 4096, C <= 32768) is checked by head_gemm_supported.

bool aligned16(const torch::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr<float>()) % 16 == 0; }

void check_labels(const torch::Tensor& labels, int64_t B, int dev, bool bank = false) {
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong && labels.numel() == B && labels.is_contiguous() &&
                  labels.get_device() == dev,
              bank ? "labels: int64 [N], one per bank row, on the bank's device" : "labels: int64 [B] on x's device");
}

// W [G][C][K] or its single-head [C][K] form (heads = false); everything checked before any
// allocation or launch
std::vector<torch::Tensor> head_gemm_step(const char* op, bool heads, torch::Tensor x, torch::Tensor W,
                                          torch::Tensor b, torch::Tensor labels, OptT rows, OptT bufW, OptT bufb,
                                          const std::vector<double>& lrs, double momentum,
                                          const std::vector<double>& wds, bool first, bool train) {
  TORCH_CHECK(x.dim() == 2 && W.dim() == (heads ? 3 : 2), op, ": x [B][K], W ", heads ? "[G][C][K]" : "[C][K]");
  const int64_t N = x.size(0), K = x.size(1), G = heads ? W.size(0) : 1, C = W.size(heads ? 1 : 0);
  TORCH_CHECK(G >= 1 && G <= kLinearSweepMaxHeads, op, ": 1 <= G <= ", kLinearSweepMaxHeads, ", got ", G);
  TORCH_CHECK((int64_t)lrs.size() == G && (int64_t)wds.size() == G, op, ": ", G, " heads need ", G,
              " learning rates and weight decays, got ", lrs.size(), " and ", wds.size());
  const std::vector<int64_t> wshape = heads ? std::vector<int64_t>{G, C, K} : std::vector<int64_t>{C, K};
  const std::vector<int64_t> bshape = heads ? std::vector<int64_t>{G, C} : std::vector<int64_t>{C};
  check_f32(x, {N, K}, "x");
  check_f32(W, wshape, "W");
  check_f32(b, bshape, "b");
  const int dev = x.get_device();
  check_labels(labels, N, dev, rows.has_value());
  const int64_t B = batch_rows(x, labels, rows);
  TORCH_CHECK(B >= 1 && B < (1LL << 31) && head_gemm_supported((int)G, (int)B, (int)K, (int)C), op,
              ": K % 64 == 0, 64 <= K <= 4096, 1 <= C <= 32768, B >= 1, element counts below 2^31");
  // (a bank is read in place at any 4-byte alignment)
  TORCH_CHECK((rows.has_value() || aligned16(x)) && aligned16(W), op, ": x and W must be 16-byte aligned");
  TORCH_CHECK(W.get_device() == dev && b.get_device() == dev, op, ": one device");
  if (train) {
    TORCH_CHECK(bufW.has_value() && bufb.has_value(), "momentum buffers required for a training step");
    check_f32(*bufW, wshape, "bufW");
    check_f32(*bufb, bshape, "bufb");
    TORCH_CHECK(bufW->get_device() == dev && bufb->get_device() == dev, op, ": one device");
    TORCH_CHECK(aligned16(*bufW), op, ": bufW must be 16-byte aligned");
  }
  c10::DeviceGuard dg(x.device());
  auto fo = x.options();
  auto logits = heads ? torch::empty({G, B, C}, fo) : torch::empty({B, C}, fo);
  auto rowstat = torch::empty({G, B, 3}, fo);
  auto stats = heads ? torch::empty({G, 3}, fo) : torch::empty({3}, fo);
  torch::Tensor dz;
  if (train) dz = torch::empty({G, B, C}, fo);
  float lr[kLinearSweepMaxHeads], wd[kLinearSweepMaxHeads];
  for (int64_t g = 0; g < G; ++g) {
    lr[g] = (float)lrs[g];
    wd[g] = (float)wds[g];
  }
  check_hip(launch_head_gemm_logits(x.data_ptr<float>(), W.data_ptr<float>(), b.data_ptr<float>(),
                                    labels.data_ptr<int64_t>(), (int)G, (int)B, (int)K, (int)C, (float)(1.0 / B),
                                    logits.data_ptr<float>(), train ? dz.data_ptr<float>() : nullptr,
                                    rowstat.data_ptr<float>(), cur_stream(), rows_ptr(rows), (long)N),
            op);
  if (train)
    check_hip(launch_head_gemm_sgd(x.data_ptr<float>(), dz.data_ptr<float>(), (int)G, (int)B, (int)K, (int)C,
                                   W.data_ptr<float>(), b.data_ptr<float>(), bufW->data_ptr<float>(),
                                   bufb->data_ptr<float>(), lr, wd, (float)momentum, first ? 1 : 0,
                                   rowstat.data_ptr<float>(), stats.data_ptr<float>(), cur_stream(), rows_ptr(rows),
                                   (long)N),
              op);
  else
    check_hip(launch_head_gemm_stats((int)G, (int)B, (int)K, (int)C, rowstat.data_ptr<float>(),
                                     stats.data_ptr<float>(), nullptr, cur_stream()),
              op);
  return {logits, stats};
}

std::vector<torch::Tensor> linear_ce_step_mfma(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                               torch::Tensor labels, OptT bufW, OptT bufb, double lr, double momentum,
                                               double wd, bool first, bool train) {
  return head_gemm_step("linear_ce_step_mfma", false, x, W, b, labels, c10::nullopt, bufW, bufb, {lr}, momentum, {wd},
                        first, train);
}

std::vector<torch::Tensor> linear_ce_step_mfma_rows(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                                    torch::Tensor labels, torch::Tensor rows, OptT bufW, OptT bufb,
                                                    double lr, double momentum, double wd, bool first, bool train) {
  return head_gemm_step("linear_ce_step_mfma_rows", false, x, W, b, labels, rows, bufW, bufb, {lr}, momentum, {wd},
                        first, train);
}

std::vector<torch::Tensor> linear_ce_sweep_step_mfma(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                                     torch::Tensor labels, OptT bufW, OptT bufb,
                                                     std::vector<double> lrs, double momentum, std::vector<double> wds,
                                                     bool first, bool train) {
  return head_gemm_step("linear_ce_sweep_step_mfma", true, x, W, b, labels, c10::nullopt, bufW, bufb, lrs, momentum,
                        wds, first, train);
}

std::vector<torch::Tensor> linear_ce_sweep_step_mfma_rows(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                                          torch::Tensor labels, torch::Tensor rows, OptT bufW,
                                                          OptT bufb, std::vector<double> lrs, double momentum,
                                                          std::vector<double> wds, bool first, bool train) {
  return head_gemm_step("linear_ce_sweep_step_mfma_rows", true, x, W, b, labels, rows, bufW, bufb, lrs, momentum, wds,
                        first, train);
}

void check_head_gemm_classifier(const char* op, const torch::Tensor& x, const torch::Tensor& W) {
  TORCH_CHECK(x.dim() == 2 && W.dim() == 2, op, ": x [B][K], W [C][K]");
  const int64_t B = x.size(0), K = x.size(1), C = W.size(0);
  check_f32(x, {B, K}, "x");
  check_f32(W, {C, K}, "W");
  TORCH_CHECK(B >= 1 && B < (1LL << 31) && head_gemm_supported(1, (int)B, (int)K, (int)C), op,
              ": K % 64 == 0, 64 <= K <= 4096, 1 <= C <= 32768, B >= 1, element counts below 2^31");
  TORCH_CHECK(aligned16(x) && aligned16(W) && W.get_device() == x.get_device(), op,
              ": x and W 16-byte aligned on one device");
}

std::vector<torch::Tensor> ce_head_fwd_mfma(torch::Tensor x, torch::Tensor W, torch::Tensor b, torch::Tensor labels,
                                            bool reduce) {
  const char* op = "ce_head_fwd_mfma";
  check_head_gemm_classifier(op, x, W);
  const int64_t B = x.size(0), K = x.size(1), C = W.size(0);
  check_f32(b, {C}, "b");
  TORCH_CHECK(b.get_device() == x.get_device(), op, ": one device");
  check_labels(labels, B, x.get_device());
  c10::DeviceGuard dg(x.device());
  auto fo = x.options();
  auto logits = torch::empty({B, C}, fo);
  auto dz = torch::empty({B, C}, fo);
  auto rowstat = torch::empty({B, 3}, fo);
  auto stats = torch::empty({3}, fo);
  auto loss = torch::empty({}, fo);
  check_hip(launch_head_gemm_logits(x.data_ptr<float>(), W.data_ptr<float>(), b.data_ptr<float>(),
                                    labels.data_ptr<int64_t>(), 1, (int)B, (int)K, (int)C, (float)(1.0 / B),
                                    logits.data_ptr<float>(), dz.data_ptr<float>(), rowstat.data_ptr<float>(),
                                    cur_stream()),
            op);
  if (reduce)
    check_hip(launch_head_gemm_stats(1, (int)B, (int)K, (int)C, rowstat.data_ptr<float>(), stats.data_ptr<float>(),
                                     loss.data_ptr<float>(), cur_stream()),
              op);
  return {logits, dz, rowstat, stats, loss};
}

// ce_head_fwd_soft on the MFMA logits GEMM: bit-identical to ce_head_fwd_mfma for labels2 = labels,
// lam = 1, eps = 0; the backward op is ce_head_bwd_mfma, unchanged
std::vector<torch::Tensor> ce_head_fwd_soft_mfma(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                                 torch::Tensor labels, torch::Tensor labels2, double lam, double eps,
                                                 bool reduce) {
  const char* op = "ce_head_fwd_soft_mfma";
  check_head_gemm_classifier(op, x, W);
  const int64_t B = x.size(0), K = x.size(1), C = W.size(0);
  check_f32(b, {C}, "b");
  TORCH_CHECK(b.get_device() == x.get_device(), op, ": one device");
  check_labels(labels, B, x.get_device());
  check_soft(op, labels2, B, x.get_device(), lam, eps);
  c10::DeviceGuard dg(x.device());
  auto fo = x.options();
  auto logits = torch::empty({B, C}, fo);
  auto dz = torch::empty({B, C}, fo);
  auto rowstat = torch::empty({B, 3}, fo);
  auto stats = torch::empty({3}, fo);
  auto loss = torch::empty({}, fo);
  check_hip(launch_head_gemm_logits_soft(x.data_ptr<float>(), W.data_ptr<float>(), b.data_ptr<float>(),
                                         labels.data_ptr<int64_t>(), labels2.data_ptr<int64_t>(), (float)lam,
                                         (float)eps, (int)B, (int)K, (int)C, (float)(1.0 / B),
                                         logits.data_ptr<float>(), dz.data_ptr<float>(), rowstat.data_ptr<float>(),
                                         cur_stream()),
            op);
  if (reduce)
    check_hip(launch_head_gemm_stats(1, (int)B, (int)K, (int)C, rowstat.data_ptr<float>(), stats.data_ptr<float>(),
                                     loss.data_ptr<float>(), cur_stream()),
              op);
  return {logits, dz, rowstat, stats, loss};
}

// ce_head_fwd_distill on the MFMA logits GEMM: the logits are ce_head_fwd_mfma's bit for bit, alpha = 0
// is bit-identical to ce_head_fwd_soft_mfma; the backward op is ce_head_bwd_mfma, unchanged
std::vector<torch::Tensor> ce_head_fwd_distill_mfma(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                                                    torch::Tensor labels, torch::Tensor labels2, double lam,
                                                    double eps, torch::Tensor teacher_logits, double temp,
                                                    double alpha, bool reduce) {
  const char* op = "ce_head_fwd_distill_mfma";
  check_head_gemm_classifier(op, x, W);
  const int64_t B = x.size(0), K = x.size(1), C = W.size(0);
  check_f32(b, {C}, "b");
  TORCH_CHECK(b.get_device() == x.get_device(), op, ": one device");
  check_labels(labels, B, x.get_device());
  check_soft(op, labels2, B, x.get_device(), lam, eps);
  check_distill(op, teacher_logits, B, C, x.get_device(), temp, alpha);
  c10::DeviceGuard dg(x.device());
  auto fo = x.options();
  auto logits = torch::empty({B, C}, fo);
  auto dz = torch::empty({B, C}, fo);
  auto rowstat = torch::empty({B, 3}, fo);
  auto stats = torch::empty({3}, fo);
  auto loss = torch::empty({}, fo);
  check_hip(launch_head_gemm_logits_distill(x.data_ptr<float>(), W.data_ptr<float>(), b.data_ptr<float>(),
                                            labels.data_ptr<int64_t>(), labels2.data_ptr<int64_t>(), (float)lam,
                                            (float)eps, teacher_logits.data_ptr<float>(), (float)temp, (float)alpha,
                                            (int)B, (int)K, (int)C, (float)(1.0 / B), logits.data_ptr<float>(),
                                            dz.data_ptr<float>(), rowstat.data_ptr<float>(), cur_stream()),
            op);
  if (reduce)
    check_hip(launch_head_gemm_stats(1, (int)B, (int)K, (int)C, rowstat.data_ptr<float>(), stats.data_ptr<float>(),
                                     loss.data_ptr<float>(), cur_stream()),
              op);
  return {logits, dz, rowstat, stats, loss};
}

c10::optional<torch::Tensor> ce_head_bwd_mfma(torch::Tensor x, torch::Tensor dz, torch::Tensor W, torch::Tensor gout,
                                              torch::Tensor rowstat, torch::Tensor stats, torch::Tensor loss, OptT dW,
                                              OptT db, bool need_dx) {
  const char* op = "ce_head_bwd_mfma";
  check_head_gemm_classifier(op, x, W);
  const int64_t B = x.size(0), K = x.size(1), C = W.size(0);
  const int dev = x.get_device();
  check_f32(dz, {B, C}, "dz");
  check_f32(rowstat, {B, 3}, "rowstat");
  check_f32(stats, {3}, "stats");
  check_f32(loss, {}, "loss");
  TORCH_CHECK(gout.is_cuda() && gout.scalar_type() == at::kFloat && gout.numel() == 1, "gout: one fp32 GPU value");
  for (const torch::Tensor* t : {&dz, &rowstat, &stats, &loss, &gout})
    TORCH_CHECK(t->get_device() == dev, op, ": one device");
  TORCH_CHECK(aligned16(dz), op, ": dz must be 16-byte aligned");
  TORCH_CHECK(dW.has_value() == db.has_value(), op, ": dW and db come together");
  if (dW.has_value()) {
    check_f32(*dW, {C, K}, "dW");
    check_f32(*db, {C}, "db");
    TORCH_CHECK(dW->get_device() == dev && db->get_device() == dev, "dW / db: x's device");
    TORCH_CHECK(aligned16(*dW), "dW must be 16-byte aligned");
  }
  TORCH_CHECK(need_dx || dW.has_value(), op, ": nothing to compute");
  c10::DeviceGuard dg(x.device());
  c10::optional<torch::Tensor> dX;
  if (need_dx) dX = torch::empty({B, K}, x.options());
  check_hip(launch_head_gemm_bwd(x.data_ptr<float>(), dz.data_ptr<float>(), W.data_ptr<float>(), (int)B, (int)K,
                                 (int)C, gout.data_ptr<float>(), need_dx ? dX->data_ptr<float>() : nullptr,
                                 dW.has_value() ? dW->data_ptr<float>() : nullptr,
                                 db.has_value() ? db->data_ptr<float>() : nullptr, rowstat.data_ptr<float>(),
                                 stats.data_ptr<float>(), loss.data_ptr<float>(), cur_stream()),
            op);
  return dX;
}

}  // namespace

void register_probe(pybind11::module& m) {
  // the row-indexed steps: x a feature bank [N][K], labels [N], the batch = bank rows `rows` (int64 [B],
  // on the device, in [0, N)), read in place; otherwise the argument lists of their plain siblings
  const char* rows_doc = "on bank rows `rows`: bit-identical to the plain op on x[rows], labels[rows]";
#define SDX_ROWS_OP(name, lr_arg, wd_arg)                                                                         \
  m.def(#name, &name, rows_doc, pybind11::arg("x"), pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"), \
        pybind11::arg("rows"), pybind11::arg("bufW"), pybind11::arg("bufb"), pybind11::arg(lr_arg),               \
        pybind11::arg("momentum"), pybind11::arg(wd_arg), pybind11::arg("first"), pybind11::arg("train"))
  SDX_ROWS_OP(linear_ce_step_rows, "lr", "wd");
  SDX_ROWS_OP(linear_ce_sweep_step_rows, "lrs", "wds");
  SDX_ROWS_OP(linear_ce_step_mfma_rows, "lr", "wd");
  SDX_ROWS_OP(linear_ce_sweep_step_mfma_rows, "lrs", "wds");
#undef SDX_ROWS_OP
  m.def("linear_ce_step_mfma", &linear_ce_step_mfma,
        "linear_ce_step on bf16x3 MFMA GEMMs (head_gemm.hip): K = 64·j <= 4096, C <= 32768",
        pybind11::arg("x"), pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"), pybind11::arg("bufW"),
        pybind11::arg("bufb"), pybind11::arg("lr"), pybind11::arg("momentum"), pybind11::arg("wd"),
        pybind11::arg("first"), pybind11::arg("train"));
  m.def("linear_ce_sweep_step_mfma", &linear_ce_sweep_step_mfma,
        "linear_ce_sweep_step on bf16x3 MFMA GEMMs; head g is bit-identical to linear_ce_step_mfma",
        pybind11::arg("x"), pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"), pybind11::arg("bufW"),
        pybind11::arg("bufb"), pybind11::arg("lrs"), pybind11::arg("momentum"), pybind11::arg("wds"),
        pybind11::arg("first"), pybind11::arg("train"));
  m.def("ce_head_fwd_mfma", &ce_head_fwd_mfma, "ce_head_fwd on bf16x3 MFMA GEMMs", pybind11::arg("x"),
        pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"), pybind11::arg("reduce"));
  m.def("ce_head_fwd_soft", &ce_head_fwd_soft,
        "ce_head_fwd with a two-label, label-smoothed target (Mixup / CutMix / label smoothing)", pybind11::arg("x"),
        pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"), pybind11::arg("labels2"),
        pybind11::arg("lam"), pybind11::arg("eps"), pybind11::arg("reduce"));
  m.def("ce_head_fwd_soft_mfma", &ce_head_fwd_soft_mfma, "ce_head_fwd_soft on the bf16x3 MFMA logits GEMM",
        pybind11::arg("x"), pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"),
        pybind11::arg("labels2"), pybind11::arg("lam"), pybind11::arg("eps"), pybind11::arg("reduce"));
  m.def("ce_head_fwd_distill", &ce_head_fwd_distill,
        "ce_head_fwd_soft blended with the temperature-scaled KL to a teacher's logits (knowledge distillation)",
        pybind11::arg("x"), pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"),
        pybind11::arg("labels2"), pybind11::arg("lam"), pybind11::arg("eps"), pybind11::arg("teacher_logits"),
        pybind11::arg("temp"), pybind11::arg("alpha"), pybind11::arg("reduce"));
  m.def("ce_head_fwd_distill_mfma", &ce_head_fwd_distill_mfma, "ce_head_fwd_distill on the bf16x3 MFMA logits GEMM",
        pybind11::arg("x"), pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"),
        pybind11::arg("labels2"), pybind11::arg("lam"), pybind11::arg("eps"), pybind11::arg("teacher_logits"),
        pybind11::arg("temp"), pybind11::arg("alpha"), pybind11::arg("reduce"));
  m.def("ce_head_bwd_mfma", &ce_head_bwd_mfma, "ce_head_bwd on bf16x3 MFMA GEMMs", pybind11::arg("x"),
        pybind11::arg("dz"), pybind11::arg("W"), pybind11::arg("gout"), pybind11::arg("rowstat"),
        pybind11::arg("stats"), pybind11::arg("loss"), pybind11::arg("dW"), pybind11::arg("db"),
        pybind11::arg("need_dx"));
  m.def("head_gemm_supported", &head_gemm_supported, "whether the MFMA classifier head runs (G, B, K, C)",
        pybind11::arg("G"), pybind11::arg("B"), pybind11::arg("K"), pybind11::arg("C"));
  m.def("ce_head_fwd", &ce_head_fwd,
        "trainable classifier + mean cross-entropy, forward: logits, dz, row statistics (+ their sums when reduce)",
        pybind11::arg("x"), pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"), pybind11::arg("reduce"));
  m.def("ce_head_bwd", &ce_head_bwd,
        "trainable classifier backward: dX, dW += , db += (gradient sinks), statistics; one launch",
        pybind11::arg("x"), pybind11::arg("dz"), pybind11::arg("W"), pybind11::arg("gout"), pybind11::arg("rowstat"),
        pybind11::arg("stats"), pybind11::arg("loss"), pybind11::arg("dW"), pybind11::arg("db"),
        pybind11::arg("need_dx"));
  m.def("linear_ce_step", &linear_ce_step,
        "linear classifier + mean cross-entropy + top-1/5 hits (+ gradient and SGD update when train)",
        pybind11::arg("x"), pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"), pybind11::arg("bufW"),
        pybind11::arg("bufb"), pybind11::arg("lr"), pybind11::arg("momentum"), pybind11::arg("wd"),
        pybind11::arg("first"), pybind11::arg("train"));
  m.def("linear_ce_sgd_raw", &linear_ce_sgd_raw,
        "test-only: the gradient + SGD launch of linear_ce_step on a caller-supplied dz and rowstat -> stats [3]",
        pybind11::arg("x"), pybind11::arg("dz"), pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("bufW"),
        pybind11::arg("bufb"), pybind11::arg("lr"), pybind11::arg("momentum"), pybind11::arg("wd"),
        pybind11::arg("first"), pybind11::arg("rowstat"));
  m.def("linear_ce_sweep_step", &linear_ce_sweep_step,
        "G linear classifiers with per-head lr / wd on one feature batch: logits [G][B][C], stats [G][3] "
        "(+ gradients and SGD updates when train); head g is bit-identical to linear_ce_step",
        pybind11::arg("x"), pybind11::arg("W"), pybind11::arg("b"), pybind11::arg("labels"), pybind11::arg("bufW"),
        pybind11::arg("bufb"), pybind11::arg("lrs"), pybind11::arg("momentum"), pybind11::arg("wds"),
        pybind11::arg("first"), pybind11::arg("train"));
}

}  // namespace sdx_bind
