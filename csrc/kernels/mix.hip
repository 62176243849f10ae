// Mixup / CutMix of an augmented batch (supervised trainer: --mixup, --cutmix): one streaming
// pass over the dense NHWC bf16 batch x [B][H][W][8] the augmentation kernels leave in HBM,
// out of place. The partner of image i is image (i − 1) mod B (roll(1, 0)): no permutation
// tensor. One λ and one box per launch (batch mode), passed by value: nothing is drawn on the
// device and nothing is read back.
//
//   CutMix  out[i] = x[i−1] inside the box [y0, y1) x [x0, x1), x[i] outside: the 16 bytes of the
//           pixel are copied as they are (padded channels included), one load per pixel.
//   Mixup   out[i] = bf16(λ·x[i] + (1 − λ)·x[i−1]): λ and 1 − λ in fp32, the two products and
//           the sum each rounded to fp32 (no fused multiply-add), then the one bf16 rounding
//           of the augmentation kernels' store (pack_bf2: round to nearest even).
//
// A thread moves whole 16-byte pixels: one 16-byte load per operand pixel, one 16-byte store.
// Memory-bound: the grid is capped at 2 blocks per CU and strides over the rest, 4 pixels of a
// thread in flight at a time.
#include "common.h"
#include "launchers.h"

using namespace sdx;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2 * 256;   // 2 blocks on each of the 256 CUs

template <int MODE>
__global__ __launch_bounds__(kThreads) void mix_views_kernel(const uint4* __restrict__ x, uint4* __restrict__ out,
                                                             uint32_t npix, uint32_t img, FastDiv d_img, FastDiv d_w,
                                                             float lam, int y0, int y1, int x0, int x1) {
  const uint32_t stride = gridDim.x * kThreads;
  const float lam1 = 1.f - lam;
#pragma unroll 4
  for (uint32_t p = blockIdx.x * kThreads + threadIdx.x; p < npix; p += stride) {
    // pixel p of image i; its partner is the same pixel of image i − 1, image B − 1 for i = 0
    const uint32_t i = fdiv(p, d_img);
    const uint32_t q = p - i * img;
    const uint32_t pp = i == 0 ? p + (npix - img) : p - img;
    SDX_DCHECK(q < img && pp < npix && pp - fdiv(pp, d_img) * img == q);
    if constexpr (MODE == kMixCutmix) {
      const int y = (int)fdiv(q, d_w);
      const int xx = (int)(q - (uint32_t)y * d_w.d);
      const bool inside = y >= y0 && y < y1 && xx >= x0 && xx < x1;
      out[p] = x[inside ? pp : p];
    } else {
      float a[8], b[8], r[8];
      unpack8(x[p], a);
      unpack8(x[pp], b);
#pragma unroll
      for (int c = 0; c < 8; ++c) r[c] = __fadd_rn(__fmul_rn(lam, a[c]), __fmul_rn(lam1, b[c]));
      out[p] = pack8(r);
    }
  }
}

}  // namespace

hipError_t launch_mix_views(const void* x, void* out, int B, int H, int W, int mode, float lam, int y0, int y1, int x0,
                            int x1, hipStream_t s) {
  if (x == nullptr || out == nullptr || B < 1 || H < 1 || W < 1) return hipErrorInvalidValue;
  if (((uintptr_t)x | (uintptr_t)out) & 15) return hipErrorInvalidValue;
  const long npix = (long)B * H * W;
  if (npix >= (1L << 31)) return hipErrorInvalidValue;   // 32-bit pixel indices (FastDiv's range)
  // out of place: the partner of a pixel may be written before it is read otherwise
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out, bytes = (uintptr_t)npix * 16;
  if (xa < oa + bytes && oa < xa + bytes) return hipErrorInvalidValue;
  if (!(lam >= 0.f && lam <= 1.f)) return hipErrorInvalidValue;   // (a NaN fails both)
  if (mode != kMixMixup && mode != kMixCutmix) return hipErrorInvalidValue;
  if (mode == kMixCutmix && !(0 <= y0 && y0 <= y1 && y1 <= H && 0 <= x0 && x0 <= x1 && x1 <= W))
    return hipErrorInvalidValue;
  const uint32_t img = (uint32_t)H * (uint32_t)W;
  const long blocks = (npix + kThreads - 1) / kThreads;
  const dim3 grid((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), blk(kThreads);
  const FastDiv d_img = make_fastdiv(img), d_w = make_fastdiv((uint32_t)W);
  if (mode == kMixCutmix)
    hipLaunchKernelGGL(mix_views_kernel<kMixCutmix>, grid, blk, 0, s, (const uint4*)x, (uint4*)out, (uint32_t)npix,
                       img, d_img, d_w, lam, y0, y1, x0, x1);
  else
    hipLaunchKernelGGL(mix_views_kernel<kMixMixup>, grid, blk, 0, s, (const uint4*)x, (uint4*)out, (uint32_t)npix, img,
                       d_img, d_w, lam, y0, y1, x0, x1);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
