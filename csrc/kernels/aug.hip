// GPU SimCLR augmentation: the whole torchvision pipeline of the reference
// (main_supcon.py:170-179: RandomResizedCrop(size, scale=(0.2,1)), RandomHorizontalFlip,
// RandomApply(ColorJitter(0.4,0.4,0.4,0.1), p=0.8), RandomGrayscale(p=0.2), ToTensor,
// Normalize) for a batch of uint8 HWC images resident in HBM, writing the network input
// directly: NHWC bf16 with channels padded to 8 (16-byte pixels for the stem conv's
// implicit-GEMM gather), views stacked view-major ([v0 batch; v1 batch]) as the
// reference's torch.cat([images[0], images[1]]) (main_supcon.py:256).
//
// One 256-thread workgroup per (sample, view). Randomness is a counter-based hash of
// (seed, sample index, view, draw), so a step is reproducible and needs no RNG state.
// Contrast needs the image mean at its position in the (random) jitter order, so the
// pixel pipeline runs twice when contrast is active: pass 1 up to the contrast op
// (block-reduced grey mean), pass 2 the full chain.
#include "blur_plan.h"
#include "common.h"
#include "launchers.h"

using namespace sdx;

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

struct Rng {
  uint64_t key;
  uint32_t ctr;
  __device__ float uni() {  // [0, 1)
    const uint64_t v = mix64(key ^ mix64(0x1234567ull + ctr++));
    return (float)(v >> 40) * (1.0f / 16777216.0f);
  }
};

struct AugParams {
  const uint8_t* data;     // [n_data][H][W][3], or ragged (offs != nullptr): image i at data + offs[i]
  const int64_t* offs;     // optional [n_data] byte offsets of native-resolution images
  const int32_t* hw;       // optional [n_data][2] their (height, width)
  long n_data;             // images in `data` (bounds checks)
  const int64_t* idx;      // [B]
  uint16_t* out;           // [n_views*B][S][S][8]
  int B, H, W, S, n_views;
  uint64_t seed;
  const int64_t* seed_dev;   // optional: seed read from device memory (hipGraph replays)
  float mean[3], inv_std[3];
  float scale_lo, scale_hi, ratio_lo, ratio_hi;
  float jitter_p, bright, contrast, sat, hue, gray_p;
  int do_crop, do_flip;
};

struct ViewParams {
  float ci, cj, ch, cw;    // crop box (top, left, height, width) in source pixels
  bool flip, jitter, gray;
  float fb, fc, fs, fh;    // jitter factors
  int order[4];            // 0 brightness, 1 contrast, 2 saturation, 3 hue
};

__device__ void make_view_params(const AugParams& p, Rng& rng, ViewParams& v, int Hi, int Wi) {
  const float H = Hi, W = Wi;
  v.ci = 0.f; v.cj = 0.f; v.ch = H; v.cw = W;
  if (p.do_crop) {
    const float area = H * W;
    const float lr0 = logf(p.ratio_lo), lr1 = logf(p.ratio_hi);
    bool found = false;
    for (int t = 0; t < 10 && !found; ++t) {
      const float target = area * (p.scale_lo + (p.scale_hi - p.scale_lo) * rng.uni());
      const float ar = expf(lr0 + (lr1 - lr0) * rng.uni());
      const float w = rintf(sqrtf(target * ar)), h = rintf(sqrtf(target / ar));
      if (w > 0.f && w <= W && h > 0.f && h <= H) {
        v.ci = floorf(rng.uni() * (H - h + 1.f));
        v.cj = floorf(rng.uni() * (W - w + 1.f));
        v.ch = h; v.cw = w;
        found = true;
      }
    }
    if (!found) {  // central crop, ratio clamped (torchvision fallback)
      const float in_ratio = W / H;
      float w, h;
      if (in_ratio < p.ratio_lo) { w = W; h = rintf(w / p.ratio_lo); }
      else if (in_ratio > p.ratio_hi) { h = H; w = rintf(h * p.ratio_hi); }
      else { w = W; h = H; }
      v.ci = floorf((H - h) * 0.5f); v.cj = floorf((W - w) * 0.5f); v.ch = h; v.cw = w;
    }
  }
  v.flip = p.do_flip && rng.uni() < 0.5f;
  v.jitter = rng.uni() < p.jitter_p;
  v.fb = 1.f + p.bright * (2.f * rng.uni() - 1.f);
  v.fc = 1.f + p.contrast * (2.f * rng.uni() - 1.f);
  v.fs = 1.f + p.sat * (2.f * rng.uni() - 1.f);
  v.fh = p.hue * (2.f * rng.uni() - 1.f);
  // random permutation of the 4 jitter ops (Fisher-Yates)
  for (int i = 0; i < 4; ++i) v.order[i] = i;
  for (int i = 3; i > 0; --i) {
    const int j = (int)(rng.uni() * (i + 1)) % (i + 1);
    const int t = v.order[i]; v.order[i] = v.order[j]; v.order[j] = t;
  }
  v.gray = rng.uni() < p.gray_p;
  if (p.bright <= 0.f && p.contrast <= 0.f && p.sat <= 0.f && p.hue <= 0.f) v.jitter = false;
}

__device__ __forceinline__ float grey(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

__device__ void adjust_hue(float& r, float& g, float& b, float hf) {
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  const float cr = mx - mn;
  const float v = mx;
  const float s = cr / (mx == 0.f ? 1.f : mx);
  const float crd = cr == 0.f ? 1.f : cr;
  const float rc = (mx - r) / crd, gc = (mx - g) / crd, bc = (mx - b) / crd;
  float h;
  if (mx == r) h = bc - gc;
  else if (mx == g) h = 2.f + rc - bc;
  else h = 4.f + gc - rc;
  h = h / 6.f + 1.f;
  h = h - floorf(h);
  h = h + hf;
  h = h - floorf(h);
  const float h6 = h * 6.f;
  const float i = floorf(h6);
  const float f = h6 - i;
  const float pp = clamp01(v * (1.f - s)), q = clamp01(v * (1.f - s * f)), t = clamp01(v * (1.f - s * (1.f - f)));
  switch (((int)i) % 6) {
    case 0: r = v; g = t; b = pp; break;
    case 1: r = q; g = v; b = pp; break;
    case 2: r = pp; g = v; b = t; break;
    case 3: r = pp; g = q; b = v; break;
    case 4: r = t; g = pp; b = v; break;
    default: r = v; g = pp; b = q; break;
  }
}

// bilinear sample (align_corners=False) of the crop box, then flip
__device__ void sample_pixel(const AugParams& p, const uint8_t* img, int H, int W, const ViewParams& v, int oy,
                             int ox, float& r, float& g, float& b) {
  const int xs = v.flip ? (p.S - 1 - ox) : ox;
  float sy = (oy + 0.5f) * (v.ch / p.S) - 0.5f + v.ci;
  float sx = (xs + 0.5f) * (v.cw / p.S) - 0.5f + v.cj;
  sy = fminf(fmaxf(sy, v.ci), v.ci + v.ch - 1.f);
  sx = fminf(fmaxf(sx, v.cj), v.cj + v.cw - 1.f);
  const int y0 = (int)floorf(sy), x0 = (int)floorf(sx);
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const float wy = sy - y0, wx = sx - x0;
  SDX_DCHECK(y0 >= 0 && x0 >= 0 && y0 < H && x0 < W && y1 < H && x1 < W);
  const uint8_t* p00 = img + ((size_t)y0 * W + x0) * 3;
  const uint8_t* p01 = img + ((size_t)y0 * W + x1) * 3;
  const uint8_t* p10 = img + ((size_t)y1 * W + x0) * 3;
  const uint8_t* p11 = img + ((size_t)y1 * W + x1) * 3;
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float top = p00[k] + (p01[k] - (float)p00[k]) * wx;
    const float bot = p10[k] + (p11[k] - (float)p10[k]) * wx;
    c[k] = (top + (bot - top) * wy) * (1.f / 255.f);
  }
  r = c[0]; g = c[1]; b = c[2];
}

// apply jitter ops order[0..n_ops) (contrast uses `cmean`)
__device__ void jitter_ops(const ViewParams& v, int n_ops, float cmean, float& r, float& g, float& b) {
  for (int k = 0; k < n_ops; ++k) {
    switch (v.order[k]) {
      case 0: r = clamp01(r * v.fb); g = clamp01(g * v.fb); b = clamp01(b * v.fb); break;
      case 1:
        r = clamp01(v.fc * r + (1.f - v.fc) * cmean);
        g = clamp01(v.fc * g + (1.f - v.fc) * cmean);
        b = clamp01(v.fc * b + (1.f - v.fc) * cmean);
        break;
      case 2: {
        const float gy = grey(r, g, b);
        r = clamp01(v.fs * r + (1.f - v.fs) * gy);
        g = clamp01(v.fs * g + (1.f - v.fs) * gy);
        b = clamp01(v.fs * b + (1.f - v.fs) * gy);
        break;
      }
      default: adjust_hue(r, g, b, v.fh); break;
    }
  }
}

// The per-pixel pipeline shared by aug_kernel and aug_blur_kernel: one copy, so a view the blur
// kernel leaves un-blurred is bit-equal to aug_kernel's by construction.

// pass 1: grey mean at the contrast position over the S x S pixels (0 when contrast is not
// applied); `red`: 4 floats of LDS
__device__ __forceinline__ float contrast_mean(const AugParams& p, const uint8_t* img, int H, int W,
                                               const ViewParams& v, float* red) {
  const int npix = p.S * p.S;
  float cmean = 0.f;
  int cpos = -1;
  if (v.jitter)
    for (int k = 0; k < 4; ++k)
      if (v.order[k] == 1) cpos = k;
  if (cpos >= 0) {
    float acc = 0.f;
    for (int pix = threadIdx.x; pix < npix; pix += 256) {
      float r, g, bb;
      sample_pixel(p, img, H, W, v, pix / p.S, pix % p.S, r, g, bb);
      jitter_ops(v, cpos, 0.f, r, g, bb);
      acc += grey(r, g, bb);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    cmean = (red[0] + red[1] + red[2] + red[3]) / (float)npix;
  }
  return cmean;
}

// sample -> jitter -> gray: the colour pixel in [0, 1] before normalize
__device__ __forceinline__ void colour_pixel(const AugParams& p, const uint8_t* img, int H, int W, const ViewParams& v,
                                             float cmean, int oy, int ox, float& r, float& g, float& bb) {
  sample_pixel(p, img, H, W, v, oy, ox, r, g, bb);
  if (v.jitter) jitter_ops(v, 4, cmean, r, g, bb);
  if (v.gray) { const float gy = grey(r, g, bb); r = g = bb = gy; }
}

// normalize, round to bf16 once, store the 16-byte pixel (channels 3..7 zero)
__device__ __forceinline__ void store_pixel(const AugParams& p, uint16_t* out, int pix, float r, float g, float bb) {
  r = (r - p.mean[0]) * p.inv_std[0];
  g = (g - p.mean[1]) * p.inv_std[1];
  bb = (bb - p.mean[2]) * p.inv_std[2];
  reinterpret_cast<uint4*>(out)[pix] = make_uint4(pack_bf2(r, g), pack_bf2(bb, 0.f), 0u, 0u);
}

// pass 2 of a view without blur: every pixel straight from the source to the store
__device__ __forceinline__ void plain_view(const AugParams& p, const uint8_t* img, int H, int W, const ViewParams& v,
                                           float cmean, uint16_t* out) {
  const int npix = p.S * p.S;
  for (int pix = threadIdx.x; pix < npix; pix += 256) {
    float r, g, bb;
    colour_pixel(p, img, H, W, v, cmean, pix / p.S, pix % p.S, r, g, bb);
    store_pixel(p, out, pix, r, g, bb);
  }
}

__global__ __launch_bounds__(256) void aug_kernel(AugParams p) {
  __shared__ float red[4];
  __shared__ ViewParams vp;
  const int b = blockIdx.x, view = blockIdx.y;
  const int64_t src = p.idx[b];
  SDX_DCHECK(p.n_data <= 0 || (src >= 0 && src < p.n_data));
  // dense [N][H][W][3] store, or native-resolution images (ImageFolder: RandomResizedCrop
  // samples its box from the original pixels, as torchvision does on the decoded image)
  const int H = p.offs ? p.hw[2 * src] : p.H, W = p.offs ? p.hw[2 * src + 1] : p.W;
  const uint8_t* img = p.offs ? p.data + p.offs[src] : p.data + (size_t)src * p.H * p.W * 3;
  if (threadIdx.x == 0) {
    const uint64_t seed = p.seed_dev ? (uint64_t)p.seed_dev[0] : p.seed;
    Rng rng{mix64(seed * 0x100000001b3ull + (uint64_t)src * 31ull + (uint64_t)view * 0x9E37ull + (uint64_t)b), 0};
    make_view_params(p, rng, vp, H, W);
  }
  __syncthreads();
  const ViewParams v = vp;
  const float cmean = contrast_mean(p, img, H, W, v, red);
  const int npix = p.S * p.S;
  plain_view(p, img, H, W, v, cmean, p.out + ((size_t)view * p.B + b) * npix * 8);
}

// ---- Gaussian blur stage (SimCLR recipe at ImageNet-sized inputs) ---------------------------
// RandomApply(GaussianBlur(k, sigma ~ U(lo, hi)), p) between grayscale and normalize, as the
// torchvision tensor gaussian_blur: separable, taps w_j ~ exp(-0.5 (j/sigma)^2) normalised to
// sum 1, reflect padding, no clamp. Two more draws per view after the gray draw, so every
// earlier draw of the view is the same with the stage on or off.
//
// A blurred view is streamed through LDS top to bottom (sizes: blur_plan.h), `rows` rows per
// round, fp32 from the uint8 source to the one bf16 rounding at the store:
//   A  pre-blur pixels (sample -> jitter -> gray) of the next `rows` rows into `stage`
//   B  their horizontal blur into slots (y % ring_rows) of `ring`
//   C  the output rows whose 2r+1 ring rows are now complete: vertical blur, normalize, store
// C of one round and A of the next touch disjoint buffers, so a round costs two barriers.
// A view whose blur draw is false runs aug_kernel's pixel loop unchanged.
struct BlurParams {
  float blur_p, sig_lo, sig_hi;
  int r, rows, ring_rows, strip, stage_w, w_floats;
};

__device__ __forceinline__ int reflect_idx(int i, int n) {
  i = i < 0 ? -i : i;
  return i > n - 1 ? 2 * (n - 1) - i : i;
}

__global__ __launch_bounds__(256) void aug_blur_kernel(AugParams p, BlurParams q) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float red[4];
  __shared__ ViewParams vp;
  __shared__ float sigma_sh;   // < 0: this view is not blurred
  const int b = blockIdx.x, view = blockIdx.y;
  const int64_t src = p.idx[b];
  SDX_DCHECK(p.n_data <= 0 || (src >= 0 && src < p.n_data));
  const int H = p.offs ? p.hw[2 * src] : p.H, W = p.offs ? p.hw[2 * src + 1] : p.W;
  const uint8_t* img = p.offs ? p.data + p.offs[src] : p.data + (size_t)src * p.H * p.W * 3;
  if (threadIdx.x == 0) {
    const uint64_t seed = p.seed_dev ? (uint64_t)p.seed_dev[0] : p.seed;
    Rng rng{mix64(seed * 0x100000001b3ull + (uint64_t)src * 31ull + (uint64_t)view * 0x9E37ull + (uint64_t)b), 0};
    make_view_params(p, rng, vp, H, W);
    const bool blur = rng.uni() < q.blur_p;
    const float sg = q.sig_lo + (q.sig_hi - q.sig_lo) * rng.uni();
    sigma_sh = blur ? sg : -1.f;
  }
  __syncthreads();
  // read in place: with dynamic LDS in the kernel a private copy's order[] (indexed at run
  // time) would live in scratch
  const ViewParams& v = vp;
  const float sigma = sigma_sh;
  const int S = p.S, npix = S * S;
  // pass 1 runs over the un-blurred pixels, and a view whose blur draw is false is aug_kernel's
  const float cmean = contrast_mean(p, img, H, W, v, red);
  uint16_t* out = p.out + ((size_t)view * p.B + b) * npix * 8;
  if (sigma < 0.f) {
    plain_view(p, img, H, W, v, cmean, out);
    return;
  }

  const int R = q.r, K = 2 * q.r + 1, rows = q.rows, ring_rows = q.ring_rows, strip = q.strip, sw = q.stage_w;
  float* w = lds;                         // [R + 1] w[|j|]
  float* stage = lds + q.w_floats;        // [rows][3][sw]
  float* ring = stage + rows * 3 * sw;    // [ring_rows][3][strip]
  for (int j = threadIdx.x; j <= R; j += 256) {
    const float t = (float)j / sigma;
    w[j] = expf(-0.5f * t * t);
  }
  __syncthreads();
  // every thread adds the taps in the same order (-R..R): one deterministic normaliser
  float wsum = 0.f;
  for (int j = -R; j <= R; ++j) wsum += w[j < 0 ? -j : j];
  __syncthreads();
  for (int j = threadIdx.x; j <= R; j += 256) w[j] = w[j] / wsum;
  __syncthreads();

  const int n_rounds = (S + rows - 1) / rows;
  for (int x0 = 0; x0 < S; x0 += strip) {
    const int tw = min(strip, S - x0);                        // output columns of this strip
    const int xa = max(0, x0 - R), xb = min(S, x0 + tw + R);  // staged columns [xa, xb)
    const int pw = xb - xa;
    SDX_DCHECK(pw <= sw && tw <= strip);
    int o_next = 0;   // first output row not yet stored
    for (int n = 0; n <= n_rounds; ++n) {
      if (n < n_rounds) {   // A
        const int y0 = n * rows, nr = min(rows, S - y0);
        for (int i = threadIdx.x; i < nr * pw; i += 256) {
          const int rr = i / pw, t = i - rr * pw;
          float r, g, bb;
          colour_pixel(p, img, H, W, v, cmean, y0 + rr, xa + t, r, g, bb);
          SDX_DCHECK(rr >= 0 && rr < rows && t >= 0 && t < sw);
          float* d = stage + rr * 3 * sw + t;
          d[0] = r; d[sw] = g; d[2 * sw] = bb;
        }
      }
      if (n > 0) {   // C: rows up to y1 are in the ring
        const int y1 = min(n * rows, S) - 1;
        const int o_end = y1 == S - 1 ? S : y1 - R + 1;
        const int cnt = max(0, o_end - o_next);
        for (int i = threadIdx.x; i < cnt * tw; i += 256) {
          const int oo = i / tw, t = i - oo * tw;
          const int o = o_next + oo;
          float a0 = 0.f, a1 = 0.f, a2 = 0.f;
          if (o - R >= 0 && o + R <= S - 1) {
            SDX_DCHECK(o - R > y1 - ring_rows && o + R <= y1);
            int s = (o - R) % ring_rows;
            for (int j = 0; j < K; ++j) {
              const float wj = w[j < R ? R - j : j - R];
              const float* row = ring + s * 3 * strip + t;
              a0 += wj * row[0]; a1 += wj * row[strip]; a2 += wj * row[2 * strip];
              if (++s == ring_rows) s = 0;
            }
          } else {
            for (int j = -R; j <= R; ++j) {
              const int yy = reflect_idx(o + j, S);
              SDX_DCHECK(yy >= 0 && yy < S && yy > y1 - ring_rows && yy <= y1);
              const float wj = w[j < 0 ? -j : j];
              const float* row = ring + (yy % ring_rows) * 3 * strip + t;
              a0 += wj * row[0]; a1 += wj * row[strip]; a2 += wj * row[2 * strip];
            }
          }
          SDX_DCHECK(o >= 0 && o < S && x0 + t < S);
          store_pixel(p, out, o * S + x0 + t, a0, a1, a2);
        }
        o_next += cnt;
      }
      if (n == n_rounds) break;
      __syncthreads();
      {   // B
        const int y0 = n * rows, nr = min(rows, S - y0);
        for (int i = threadIdx.x; i < nr * tw; i += 256) {
          const int rr = i / tw, t = i - rr * tw;
          const int x = x0 + t;
          const float* srow = stage + rr * 3 * sw;
          float a0 = 0.f, a1 = 0.f, a2 = 0.f;
          if (x - R >= 0 && x + R <= S - 1) {
            const float* sp = srow + (x - R - xa);
            SDX_DCHECK(x - R - xa >= 0 && x + R - xa < pw);
            for (int j = 0; j < K; ++j) {
              const float wj = w[j < R ? R - j : j - R];
              a0 += wj * sp[j]; a1 += wj * sp[sw + j]; a2 += wj * sp[2 * sw + j];
            }
          } else {
            for (int j = -R; j <= R; ++j) {
              const int u = reflect_idx(x + j, S) - xa;
              SDX_DCHECK(u >= 0 && u < pw);
              const float wj = w[j < 0 ? -j : j];
              a0 += wj * srow[u]; a1 += wj * srow[sw + u]; a2 += wj * srow[2 * sw + u];
            }
          }
          const int s = (y0 + rr) % ring_rows;
          SDX_DCHECK(s >= 0 && s < ring_rows && t < strip);
          float* d = ring + s * 3 * strip + t;
          d[0] = a0; d[strip] = a1; d[2 * strip] = a2;
        }
      }
      __syncthreads();
    }
  }
}

// ---- evaluation transform: Resize(R) on the shorter side + CenterCrop(S) + normalize ----------
// The torchvision evaluation pipeline over the resident store (dense or ragged), one view, no
// draws. Resize is the antialiased bilinear (triangle) filter of
// F.interpolate(mode="bilinear", antialias=True): for an axis n_in -> n_out and output i,
//   scale = n_in / n_out, support = max(scale, 1), c = scale (i + 0.5),
//   taps j in [max(0, floor(c - support + 0.5)), min(n_in, floor(c + support + 0.5))),
//   weight max(0, 1 - |j - c + 0.5| / support), divided by the sum over the window.
// Window bounds and the tap offsets are exact integers over 2 n_out (so every implementation
// agrees on every window, and the weights carry no error of a rounded centre): with
// sup = max(n_in, n_out), a = (2i + 1) n_in + n_out,
//   lo = floor((a - 2 sup) / (2 n_out)), hi = floor((a + 2 sup) / (2 n_out)), clamped, and tap j
//   weighs 1 - |2 j n_out + n_out - (2i + 1) n_in| / (2 sup).
// At scale 1 the window is {i, i + 1} with weights {1, 0}: the resample is the identity, and the
// pixel reaches store_pixel as value * (1/255) exactly as aug_kernel's un-cropped sample does.
// fp32 from the uint8 source to the one bf16 rounding; no uint8 intermediate image.
//
// Grid (image, band of kEvalBand output rows), 256 threads. The band's vertical windows are
// worked out once into static LDS (their size does not depend on the scale); a thread owns
// output columns (its horizontal window is worked out once per column) and walks the band's
// rows: per source row of the vertical window the horizontal window, all in registers. Every
// loop is bounded by the image's own H and W, whatever the scale.
constexpr int kEvalBand = 24;   // 224 rows: 9 bands and a partial one

struct AxisTaps {
  int lo, hi;       // source taps [lo, hi), inside [0, n_in)
  int num0;         // 2 lo n_out + n_out - (2i + 1) n_in; tap j: num0 + 2 (j - lo) n_out
  float inv_sum;    // 1 / sum of the window's weights
};

__device__ __forceinline__ float tap_weight(int num, float k) { return fmaxf(0.f, 1.f - fabsf((float)num) * k); }

// window of output coordinate i of an axis n_in -> n_out (1 <= n_in, 0 <= i < n_out);
// k = 1 / (2 max(n_in, n_out))
__device__ __forceinline__ AxisTaps axis_taps(int n_in, int n_out, int i, float k) {
  const int64_t sup2 = 2 * (int64_t)max(n_in, n_out);
  const int64_t a = (int64_t)(2 * (int64_t)i + 1) * n_in + n_out;
  const int64_t d = 2 * (int64_t)n_out;
  int64_t lo, hi;
  if (a + sup2 < (int64_t)1 << 31) {   // the 32-bit divide is several times cheaper
    lo = a > sup2 ? (uint32_t)(a - sup2) / (uint32_t)d : 0;
    hi = (uint32_t)(a + sup2) / (uint32_t)d;
  } else {
    lo = a > sup2 ? (a - sup2) / d : 0;
    hi = (a + sup2) / d;
  }
  AxisTaps t;
  t.lo = (int)min(lo, (int64_t)n_in - 1);
  t.hi = (int)min(hi, (int64_t)n_in);
  t.hi = max(t.hi, t.lo + 1);
  t.num0 = (int)(t.lo * d + n_out - (2 * (int64_t)i + 1) * n_in);
  float sum = 0.f;
  int num = t.num0;
  for (int j = t.lo; j < t.hi; ++j, num += (int)d) sum += tap_weight(num, k);
  t.inv_sum = 1.f / sum;
  return t;
}

// torchvision's CenterCrop offset int(round(d / 2.0)): half to even
__device__ __forceinline__ int crop_offset(int d) {
  int t = d >> 1;
  if ((d & 1) && (t & 1)) ++t;
  return t;
}

__global__ __launch_bounds__(256) void eval_crop_kernel(AugParams p, int R, int cw_log2) {
  __shared__ AxisTaps ytaps[kEvalBand];
  const int b = blockIdx.x;
  const int64_t src = p.idx[b];
  SDX_DCHECK(p.n_data <= 0 || (src >= 0 && src < p.n_data));
  const int H = p.offs ? p.hw[2 * src] : p.H, W = p.offs ? p.hw[2 * src + 1] : p.W;
  const uint8_t* img = p.offs ? p.data + p.offs[src] : p.data + (size_t)src * p.H * p.W * 3;
  SDX_DCHECK(H >= 1 && W >= 1);
  if (H < 1 || W < 1) return;   // a malformed store entry: nothing to read
  const int S = p.S;
  // resized size: the shorter side becomes R, the longer floor(R long / short); never past
  // int (an absurd aspect would only distort, not read out of bounds: the taps are clamped)
  const int64_t lng = (int64_t)R * max(H, W) / min(H, W);
  const int ol = (int)min(lng, (int64_t)0x3fffffff);
  const int oh = H <= W ? R : ol, ow = H <= W ? ol : R;
  const int top = crop_offset(oh - S), left = crop_offset(ow - S);
  const float ky = 0.5f / (float)max(H, oh), kx = 0.5f / (float)max(W, ow);

  const int y0 = blockIdx.y * kEvalBand, nrows = min(kEvalBand, S - y0);
  if ((int)threadIdx.x < nrows) ytaps[threadIdx.x] = axis_taps(H, oh, top + y0 + (int)threadIdx.x, ky);
  __syncthreads();

  const int cw = 1 << cw_log2;            // threads across a row; 256 / cw rows at a time
  const int tx = threadIdx.x & (cw - 1), ty = threadIdx.x >> cw_log2, rstep = 256 >> cw_log2;
  const int dx = 2 * ow, dy = 2 * oh;
  uint16_t* out = p.out + (size_t)b * S * S * 8;
  for (int x = tx; x < S; x += cw) {
    const AxisTaps xt = axis_taps(W, ow, left + x, kx);
    SDX_DCHECK(xt.lo >= 0 && xt.lo < xt.hi && xt.hi <= W);
    for (int r = ty; r < nrows; r += rstep) {
      const AxisTaps yt = ytaps[r];
      SDX_DCHECK(yt.lo >= 0 && yt.lo < yt.hi && yt.hi <= H);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      int ny = yt.num0;
      for (int j = yt.lo; j < yt.hi; ++j, ny += dy) {
        const uint8_t* row = img + ((size_t)j * W + xt.lo) * 3;
        float h0 = 0.f, h1 = 0.f, h2 = 0.f;
        int nx = xt.num0;
        for (int i = xt.lo; i < xt.hi; ++i, nx += dx, row += 3) {
          const float wx = tap_weight(nx, kx);
          h0 += wx * (float)row[0]; h1 += wx * (float)row[1]; h2 += wx * (float)row[2];
        }
        const float wy = tap_weight(ny, ky);
        a0 += wy * h0; a1 += wy * h1; a2 += wy * h2;
      }
      const float nrm = xt.inv_sum * yt.inv_sum;
      SDX_DCHECK(y0 + r < S && x < S);
      store_pixel(p, out, (y0 + r) * S + x, a0 * nrm * (1.f / 255.f), a1 * nrm * (1.f / 255.f),
                  a2 * nrm * (1.f / 255.f));
    }
  }
}

AugParams make_params(const uint8_t* data, const int64_t* idx, int B, int H, int W, int S, int n_views, uint64_t seed,
                      const float* mean, const float* std, float scale_lo, float scale_hi, float ratio_lo,
                      float ratio_hi, float jitter_p, float bright, float contrast, float sat, float hue, float gray_p,
                      int do_crop, int do_flip, const int64_t* seed_dev, void* out, long n_data, const int64_t* offs,
                      const int32_t* hw) {
  AugParams p{};
  p.offs = offs;
  p.hw = hw;
  p.n_data = n_data;
  p.data = data; p.idx = idx; p.out = (uint16_t*)out;
  p.B = B; p.H = H; p.W = W; p.S = S; p.n_views = n_views; p.seed = seed;
  for (int k = 0; k < 3; ++k) { p.mean[k] = mean[k]; p.inv_std[k] = 1.f / std[k]; }
  p.scale_lo = scale_lo; p.scale_hi = scale_hi; p.ratio_lo = ratio_lo; p.ratio_hi = ratio_hi;
  p.jitter_p = jitter_p; p.bright = bright; p.contrast = contrast; p.sat = sat; p.hue = hue; p.gray_p = gray_p;
  p.do_crop = do_crop; p.do_flip = do_flip;
  p.seed_dev = seed_dev;
  return p;
}

}  // namespace

hipError_t launch_gpu_augment(const uint8_t* data, const int64_t* idx, int B, int H, int W, int S, int n_views,
                              uint64_t seed, const float* mean, const float* std, float scale_lo, float scale_hi,
                              float ratio_lo, float ratio_hi, float jitter_p, float bright, float contrast,
                              float sat, float hue, float gray_p, int do_crop, int do_flip, const int64_t* seed_dev,
                              void* out, hipStream_t s, long n_data, const int64_t* offs, const int32_t* hw) {
  const AugParams p = make_params(data, idx, B, H, W, S, n_views, seed, mean, std, scale_lo, scale_hi, ratio_lo,
                                  ratio_hi, jitter_p, bright, contrast, sat, hue, gray_p, do_crop, do_flip, seed_dev,
                                  out, n_data, offs, hw);
  hipLaunchKernelGGL(aug_kernel, dim3(B, n_views), dim3(256), 0, s, p);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

// The same launch with the blur stage (one workgroup per (sample, view), one launch for the
// batch). blur_k 0 = automatic, rows 0 = automatic (blur_plan.h); a request the plan refuses
// is hipErrorInvalidValue, never a launch of something else.
hipError_t launch_gpu_augment_blur(const uint8_t* data, const int64_t* idx, int B, int H, int W, int S, int n_views,
                                   uint64_t seed, const float* mean, const float* std, float scale_lo,
                                   float scale_hi, float ratio_lo, float ratio_hi, float jitter_p, float bright,
                                   float contrast, float sat, float hue, float gray_p, int do_crop, int do_flip,
                                   float blur_p, int blur_k, float sigma_lo, float sigma_hi, int rows,
                                   const int64_t* seed_dev, void* out, hipStream_t s, long n_data,
                                   const int64_t* offs, const int32_t* hw) {
  sdx_blur::Plan pl{};
  if (!sdx_blur::make_plan(S, blur_k, rows, &pl) || !(sigma_lo > 0.f) || !(sigma_lo <= sigma_hi))
    return hipErrorInvalidValue;
  const AugParams p = make_params(data, idx, B, H, W, S, n_views, seed, mean, std, scale_lo, scale_hi, ratio_lo,
                                  ratio_hi, jitter_p, bright, contrast, sat, hue, gray_p, do_crop, do_flip, seed_dev,
                                  out, n_data, offs, hw);
  BlurParams q{};
  q.blur_p = blur_p; q.sig_lo = sigma_lo; q.sig_hi = sigma_hi;
  q.r = pl.r; q.rows = pl.rows; q.ring_rows = pl.ring_rows; q.strip = pl.strip; q.stage_w = pl.stage_w;
  q.w_floats = pl.w_floats;
  if (pl.lds_bytes > sdx_blur::kLdsDefault) {
    // above 64 KiB the kernel's dynamic-LDS limit has to be raised (once per device: to the most
    // any plan can ask for). `raised` is only a cache and is not synchronised: two threads racing
    // on it at worst both set the attribute to the same value.
    static bool raised[64] = {};
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !raised[dev]) {
      if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(aug_blur_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(sdx_blur::kLdsPerCu - sdx_blur::kStaticLds));
          e != hipSuccess)
        return e;
      if (dev >= 0 && dev < 64) raised[dev] = true;
    }
  }
  hipLaunchKernelGGL(aug_blur_kernel, dim3(B, n_views), dim3(256), (size_t)pl.lds_bytes, s, p, q);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

// Resize(R) on the shorter side + CenterCrop(S) + normalize of B images (eval_crop_kernel): one
// view, out [B][S][S][8]. 1 <= S <= R <= 32768, else hipErrorInvalidValue.
hipError_t launch_gpu_eval_crop(const uint8_t* data, const int64_t* idx, int B, int H, int W, int S, int R,
                                const float* mean, const float* std, void* out, hipStream_t s, long n_data,
                                const int64_t* offs, const int32_t* hw) {
  if (B < 1 || S < 1 || S > R || R > 32768 || (!offs && (H < 1 || W < 1))) return hipErrorInvalidValue;
  const AugParams p = make_params(data, idx, B, H, W, S, 1, 0, mean, std, 1.f, 1.f, 1.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f,
                                  0.f, 0, 0, nullptr, out, n_data, offs, hw);
  int cw_log2 = 0;
  while (cw_log2 < 8 && (1 << cw_log2) < S) ++cw_log2;
  hipLaunchKernelGGL(eval_crop_kernel, dim3(B, (S + kEvalBand - 1) / kEvalBand), dim3(256), 0, s, p, R, cw_log2);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
