// Bindings for the GPU data-pipeline kernels (aug.hip).
#include "ops_decl.h"
#include "blur_plan.h"
#include "launchers.h"

namespace sdx_bind {
namespace {

struct AugArgs {
  bool ragged;
  const int64_t* seed_dev;
  int64_t B;
  float mean[3], std[3];
  int H, W;
  long n_data;
  const int64_t* offs;
  const int32_t* hw;
};

// the argument checks both augmentation ops share
AugArgs check_aug_args(const torch::Tensor& data, const torch::Tensor& idx, int64_t S, int64_t n_views,
                       const std::vector<double>& mean, const std::vector<double>& std,
                       const c10::optional<torch::Tensor>& seed_t, const c10::optional<torch::Tensor>& offs,
                       const c10::optional<torch::Tensor>& hw) {
  AugArgs a{};
  const bool ragged = offs.has_value();
  TORCH_CHECK(ragged == hw.has_value(), "offs and hw must be given together");
  if (ragged) {
    TORCH_CHECK(data.is_cuda() && data.scalar_type() == at::kByte && data.dim() == 1 && data.is_contiguous(),
                "ragged data must be a contiguous uint8 GPU byte vector");
    TORCH_CHECK(offs->is_cuda() && offs->scalar_type() == at::kLong && offs->dim() == 1 && offs->is_contiguous(),
                "offs must be a contiguous int64 GPU vector");
    TORCH_CHECK(hw->is_cuda() && hw->scalar_type() == at::kInt && hw->dim() == 2 && hw->size(1) == 2 &&
                    hw->size(0) == offs->size(0) && hw->is_contiguous(),
                "hw must be a contiguous int32 [N, 2] GPU tensor");
  } else {
    TORCH_CHECK(data.is_cuda() && data.scalar_type() == at::kByte && data.dim() == 4 && data.size(3) == 3 &&
                    data.is_contiguous(),
                "data must be a contiguous uint8 [N,H,W,3] GPU tensor");
  }
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kLong && idx.dim() == 1 && idx.is_contiguous(),
              "idx must be a contiguous int64 GPU vector");
  TORCH_CHECK(mean.size() == 3 && std.size() == 3, "mean/std need 3 values");
  TORCH_CHECK(S >= 1 && n_views >= 1 && idx.size(0) >= 1, "bad sizes");
  if (seed_t.has_value()) {
    TORCH_CHECK(seed_t->is_cuda() && seed_t->scalar_type() == at::kLong && seed_t->numel() == 1,
                "seed_t must be an int64 GPU scalar");
    a.seed_dev = seed_t->data_ptr<int64_t>();
  }
  a.ragged = ragged;
  a.B = idx.size(0);
  for (int k = 0; k < 3; ++k) { a.mean[k] = (float)mean[k]; a.std[k] = (float)std[k]; }
  a.H = ragged ? 0 : (int)data.size(1);
  a.W = ragged ? 0 : (int)data.size(2);
  a.n_data = ragged ? (long)offs->size(0) : (long)data.size(0);
  a.offs = ragged ? offs->data_ptr<int64_t>() : nullptr;
  a.hw = ragged ? hw->data_ptr<int32_t>() : nullptr;
  return a;
}

// seed_t (optional int64 GPU scalar) overrides `seed` at kernel run time, so a captured
// hipGraph draws fresh augmentations on every replay.
torch::Tensor gpu_augment(torch::Tensor data, torch::Tensor idx, int64_t S, int64_t n_views, int64_t seed,
                          std::vector<double> mean, std::vector<double> std, double scale_lo, double scale_hi,
                          double ratio_lo, double ratio_hi, double jitter_p, double bright, double contrast,
                          double sat, double hue, double gray_p, bool do_crop, bool do_flip,
                          c10::optional<torch::Tensor> seed_t, c10::optional<torch::Tensor> offs,
                          c10::optional<torch::Tensor> hw) {
  const AugArgs a = check_aug_args(data, idx, S, n_views, mean, std, seed_t, offs, hw);
  c10::DeviceGuard dg(data.device());
  auto out = torch::empty({n_views * a.B, S, S, 8}, data.options().dtype(at::kBFloat16));
  check_hip(launch_gpu_augment(data.data_ptr<uint8_t>(), idx.data_ptr<int64_t>(), (int)a.B, a.H, a.W, (int)S,
                               (int)n_views, (uint64_t)seed, a.mean, a.std, (float)scale_lo, (float)scale_hi,
                               (float)ratio_lo, (float)ratio_hi, (float)jitter_p, (float)bright, (float)contrast,
                               (float)sat, (float)hue, (float)gray_p, do_crop ? 1 : 0, do_flip ? 1 : 0, a.seed_dev,
                               out.data_ptr(), cur_stream(), a.n_data, a.offs, a.hw),
            "gpu_augment");
  return out;
}

// gpu_augment with the Gaussian-blur stage (aug.hip aug_blur_kernel). blur_kernel 0 = automatic
// from S, rows 0 = automatic rows per barrier round (blur_plan.h); a request the plan cannot
// serve is an error here, never another kernel.
torch::Tensor gpu_augment_blur(torch::Tensor data, torch::Tensor idx, int64_t S, int64_t n_views, int64_t seed,
                               std::vector<double> mean, std::vector<double> std, double scale_lo, double scale_hi,
                               double ratio_lo, double ratio_hi, double jitter_p, double bright, double contrast,
                               double sat, double hue, double gray_p, bool do_crop, bool do_flip, double blur_p,
                               int64_t blur_kernel, double sigma_lo, double sigma_hi,
                               c10::optional<torch::Tensor> seed_t, c10::optional<torch::Tensor> offs,
                               c10::optional<torch::Tensor> hw, int64_t rows) {
  const AugArgs a = check_aug_args(data, idx, S, n_views, mean, std, seed_t, offs, hw);
  TORCH_CHECK(blur_p >= 0.0 && blur_p <= 1.0, "blur_p must be in [0, 1]");
  TORCH_CHECK((float)sigma_lo > 0.f && (float)sigma_lo <= (float)sigma_hi, "blur sigma needs 0 < lo <= hi");
  TORCH_CHECK(blur_kernel == 0 || (blur_kernel >= 3 && blur_kernel % 2 == 1), "blur kernel size must be odd and >= 3");
  const int64_t k = blur_kernel > 0 ? blur_kernel : sdx_blur::auto_kernel(S);
  TORCH_CHECK((k - 1) / 2 <= S - 1, "blur radius ", (k - 1) / 2, " exceeds size - 1 = ", S - 1,
              ": reflect padding is undefined");
  TORCH_CHECK(rows >= 0 && rows <= sdx_blur::kMaxRows, "rows per round must be in [0, ", sdx_blur::kMaxRows, "]");
  sdx_blur::Plan pl{};
  TORCH_CHECK(sdx_blur::make_plan(S, blur_kernel, rows, &pl), "blur of kernel size ", k, " at size ", S,
              " does not fit the ", sdx_blur::kLdsPerCu / 1024, " KiB LDS");
  c10::DeviceGuard dg(data.device());
  auto out = torch::empty({n_views * a.B, S, S, 8}, data.options().dtype(at::kBFloat16));
  check_hip(launch_gpu_augment_blur(data.data_ptr<uint8_t>(), idx.data_ptr<int64_t>(), (int)a.B, a.H, a.W, (int)S,
                                    (int)n_views, (uint64_t)seed, a.mean, a.std, (float)scale_lo, (float)scale_hi,
                                    (float)ratio_lo, (float)ratio_hi, (float)jitter_p, (float)bright,
                                    (float)contrast, (float)sat, (float)hue, (float)gray_p, do_crop ? 1 : 0,
                                    do_flip ? 1 : 0, (float)blur_p, (int)blur_kernel, (float)sigma_lo,
                                    (float)sigma_hi, (int)rows, a.seed_dev, out.data_ptr(), cur_stream(), a.n_data,
                                    a.offs, a.hw),
            "gpu_augment_blur");
  return out;
}

// The evaluation transform (aug.hip eval_crop_kernel): Resize(resize) on the shorter side,
// antialiased bilinear, CenterCrop(S), normalize; one view of every idx image, no draws.
torch::Tensor gpu_eval_crop(torch::Tensor data, torch::Tensor idx, int64_t S, int64_t resize,
                            std::vector<double> mean, std::vector<double> std, c10::optional<torch::Tensor> offs,
                            c10::optional<torch::Tensor> hw) {
  TORCH_CHECK(S >= 1, "crop size must be >= 1, got ", S);
  TORCH_CHECK(resize >= S && resize <= 32768, "resize must be in [S, 32768] = [", S, ", 32768], got ", resize);
  const AugArgs a = check_aug_args(data, idx, S, 1, mean, std, c10::nullopt, offs, hw);
  TORCH_CHECK(a.ragged || (a.H >= 1 && a.W >= 1), "data has no pixels");
  c10::DeviceGuard dg(data.device());
  auto out = torch::empty({a.B, S, S, 8}, data.options().dtype(at::kBFloat16));
  check_hip(launch_gpu_eval_crop(data.data_ptr<uint8_t>(), idx.data_ptr<int64_t>(), (int)a.B, a.H, a.W, (int)S,
                                 (int)resize, a.mean, a.std, out.data_ptr(), cur_stream(), a.n_data, a.offs, a.hw),
            "gpu_eval_crop");
  return out;
}

// Mixup (mode 1) / CutMix (mode 2) of an augmented batch x [B][H][W][8] bf16 with its roll(1, 0)
// (mix.hip), out of place. One lam and one box [y0, y1) x [x0, x1) per call, by value. `out`
// (optional): the destination, x's shape and dtype, not overlapping x. Everything is checked
// before the launch: a refused call writes nothing.
torch::Tensor mix_views(torch::Tensor x, int64_t mode, double lam, int64_t y0, int64_t y1, int64_t x0, int64_t x1,
                        c10::optional<torch::Tensor> out) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16, "mix_views: x must be a bf16 GPU tensor");
  TORCH_CHECK(x.dim() == 4 && x.size(3) == 8, "mix_views: x must be [B, H, W, 8]");
  TORCH_CHECK(x.is_contiguous(), "mix_views: x must be contiguous");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2);
  TORCH_CHECK(B >= 1 && H >= 1 && W >= 1, "mix_views: empty batch");
  TORCH_CHECK(B * H * W < (1LL << 31), "mix_views: B·H·W must be below 2^31");
  TORCH_CHECK(mode == kMixMixup || mode == kMixCutmix, "mix_views: mode 1 (mixup) or 2 (cutmix), got ", mode);
  TORCH_CHECK(lam >= 0.0 && lam <= 1.0, "mix_views: lam must be in [0, 1], got ", lam);
  if (mode == kMixCutmix) {
    TORCH_CHECK(0 <= y0 && y0 <= y1 && y1 <= H && 0 <= x0 && x0 <= x1 && x1 <= W, "mix_views: box [", y0, ", ", y1,
                ") x [", x0, ", ", x1, ") leaves the ", H, " x ", W, " image");
  } else {
    y0 = y1 = x0 = x1 = 0;   // (unused)
  }
  if (out.has_value()) {
    TORCH_CHECK(out->is_cuda() && out->get_device() == x.get_device() && out->scalar_type() == at::kBFloat16 &&
                    out->is_contiguous() && out->sizes() == x.sizes(),
                "mix_views: out must be a contiguous bf16 tensor of x's shape on x's device");
  }
  c10::DeviceGuard dg(x.device());
  auto o = out.has_value() ? *out : torch::empty_like(x);
  check_hip(launch_mix_views(x.data_ptr(), o.data_ptr(), (int)B, (int)H, (int)W, (int)mode, (float)lam, (int)y0,
                             (int)y1, (int)x0, (int)x1, cur_stream()),
            "mix_views");
  return o;
}

}  // namespace

void register_data(pybind11::module& m) {
  m.def("mix_views", &mix_views, "Mixup (mode 1) / CutMix (mode 2) of a [B, H, W, 8] bf16 batch with its roll(1, 0)",
        pybind11::arg("x"), pybind11::arg("mode"), pybind11::arg("lam"), pybind11::arg("y0"), pybind11::arg("y1"),
        pybind11::arg("x0"), pybind11::arg("x1"), pybind11::arg("out") = pybind11::none());
  m.def("gpu_augment", &gpu_augment, "fused SimCLR augmentation -> NHWC bf16 (C padded to 8)",
        pybind11::arg("data"), pybind11::arg("idx"), pybind11::arg("S"), pybind11::arg("n_views"),
        pybind11::arg("seed"), pybind11::arg("mean"), pybind11::arg("std"), pybind11::arg("scale_lo"),
        pybind11::arg("scale_hi"), pybind11::arg("ratio_lo"), pybind11::arg("ratio_hi"), pybind11::arg("jitter_p"),
        pybind11::arg("bright"), pybind11::arg("contrast"), pybind11::arg("sat"), pybind11::arg("hue"),
        pybind11::arg("gray_p"), pybind11::arg("do_crop"), pybind11::arg("do_flip"),
        pybind11::arg("seed_t") = pybind11::none(), pybind11::arg("offs") = pybind11::none(),
        pybind11::arg("hw") = pybind11::none());
  m.def("gpu_augment_blur", &gpu_augment_blur,
        "fused SimCLR augmentation with the Gaussian-blur stage -> NHWC bf16 (C padded to 8)",
        pybind11::arg("data"), pybind11::arg("idx"), pybind11::arg("S"), pybind11::arg("n_views"),
        pybind11::arg("seed"), pybind11::arg("mean"), pybind11::arg("std"), pybind11::arg("scale_lo"),
        pybind11::arg("scale_hi"), pybind11::arg("ratio_lo"), pybind11::arg("ratio_hi"), pybind11::arg("jitter_p"),
        pybind11::arg("bright"), pybind11::arg("contrast"), pybind11::arg("sat"), pybind11::arg("hue"),
        pybind11::arg("gray_p"), pybind11::arg("do_crop"), pybind11::arg("do_flip"), pybind11::arg("blur_p"),
        pybind11::arg("blur_kernel"), pybind11::arg("sigma_lo"), pybind11::arg("sigma_hi"),
        pybind11::arg("seed_t") = pybind11::none(), pybind11::arg("offs") = pybind11::none(),
        pybind11::arg("hw") = pybind11::none(), pybind11::arg("rows") = 0);
  m.def("gpu_eval_crop", &gpu_eval_crop,
        "Resize(resize) on the shorter side + CenterCrop(S) + normalize -> NHWC bf16 (C padded to 8)",
        pybind11::arg("data"), pybind11::arg("idx"), pybind11::arg("S"), pybind11::arg("resize"),
        pybind11::arg("mean"), pybind11::arg("std"), pybind11::arg("offs") = pybind11::none(),
        pybind11::arg("hw") = pybind11::none());
}

}  // namespace sdx_bind
