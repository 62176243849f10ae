// Linear-probe SWEEP: G classifiers of one shape (C classes, K features), each with its own
// learning rate and weight decay, trained on ONE feature batch in the two launches that
// linear_ce.hip spends on a single classifier. The frozen encoder's features are the same for
// every setting of a hyper-parameter sweep, so the feature matrix is read once per launch
// instead of once per head:
//
//   linear_ce_sweep_fwd  block = 4 rows, as linear_ce_fwd: every lane keeps its K/64 feature
//                        columns of the 4 rows in registers, loaded once and reused for every
//                        head. Heads go one after another through the same z[4][1024] LDS tile
//                        (logits, barrier, row softmax / CE / hits, barrier), so the limit is
//                        C <= 1024 per head, not G·C <= 1024.
//   linear_ce_sweep_sgd  thread = 4 consecutive weights of one class index for all G heads:
//                        x[b][k..k+3] is read once per row and feeds G independent fmaf chains
//                        over dz[g][b][c] (rows in index order), then each head's SGD update
//                        with that head's lr and wd; the last block does the G biases the same
//                        way and sums each head's row statistics in row order (fp32).
//
// Layouts: W [G][C][K], bias [G][C], momentum buffers alike, logits / dz [G][B][C],
// rowstat [G][B][3], stats [G][3]; lr and wd per head travel by value in the kernel arguments.
//
// Every head's arithmetic is, operation for operation, that of linear_ce_fwd_kernel /
// linear_ce_sgd_kernel (the same lane-strided dot products, xor-butterfly reductions, __expf /
// __logf softmax, `above < k` hit rule and update expressions): head g of a sweep step is
// bit-identical to linear_ce_step run alone with that head's lr and wd
// (tests/test_gpu_probe_sweep.py). No atomics: bit-identical from run to run.
#include "common.h"
#include "launchers.h"

using namespace sdx;

namespace {

constexpr int kRows = 4;          // rows per forward block (one wave per row for the softmax)
constexpr int kMaxClasses = 1024;
constexpr int kMaxHeads = kLinearSweepMaxHeads;

struct SweepHyper {
  float lr[kMaxHeads];
  float wd[kMaxHeads];
};

__device__ __forceinline__ float lane_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float lane_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// KJ = K / 64 feature columns per lane. ROWS: batch row b is row rows[b] of the bank x [N][K],
// labels [N], as in linear_ce.hip (the plain instantiation takes rows = nullptr, N = 0 unread)
template <int KJ, bool ROWS>
__global__ __launch_bounds__(256) void linear_ce_sweep_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
    const int64_t* __restrict__ labels, const int64_t* __restrict__ rows, long N, int G, int B, int C, float gscale,
    float* __restrict__ logits, float* __restrict__ dz, float* __restrict__ rowstat) {
  constexpr int K = 64 * KJ;
  __shared__ float z[kRows][kMaxClasses];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r0 = blockIdx.x * kRows;
  float xv[kRows][KJ];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int row = r0 + r;
    size_t src = (size_t)row;
    if constexpr (ROWS) src = row < B ? bank_row(rows, row, N) : 0;
#pragma unroll
    for (int j = 0; j < KJ; ++j) xv[r][j] = row < B ? x[src * K + 64 * j + lane] : 0.f;
  }
  // wave wv owns row r0 + wv in every head's softmax
  const int row = r0 + wv;
  const int lab = row < B ? (int)labels[ROWS ? bank_row(rows, row, N) : (size_t)row] : -1;
  for (int g = 0; g < G; ++g) {
    const float* Wg = W + (size_t)g * C * K;
    const float* bg = bias + (size_t)g * C;
    for (int c = wv; c < C; c += 4) {
      const float* wr = Wg + (size_t)c * K;
      float acc[kRows] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const float w = wr[64 * j + lane];
#pragma unroll
        for (int r = 0; r < kRows; ++r) acc[r] = fmaf(xv[r][j], w, acc[r]);
      }
      const float b = bg[c];
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const float s = lane_sum(acc[r]);
        if (lane == 0) z[r][c] = s + b;
      }
    }
    __syncthreads();
    // row softmax / cross-entropy / top-k hits of head g
    if (row < B) {
      const size_t ro = (size_t)g * B + row;
      float m = -INFINITY;
      for (int c = lane; c < C; c += 64) m = fmaxf(m, z[wv][c]);
      m = lane_max(m);
      float s = 0.f;
      for (int c = lane; c < C; c += 64) s += __expf(z[wv][c] - m);
      s = lane_sum(s);
      const float lse = m + __logf(s);
      const bool ok = lab >= 0 && lab < C;
      const float zl = ok ? z[wv][lab] : 0.f;
      float above = 0.f;
      for (int c = lane; c < C; c += 64) {
        const float v = z[wv][c];
        logits[ro * C + c] = v;
        above += v > zl ? 1.f : 0.f;
        if (dz != nullptr) dz[ro * C + c] = (__expf(v - lse) - (c == lab ? 1.f : 0.f)) * gscale;
      }
      above = lane_sum(above);
      if (lane == 0) {
        rowstat[ro * 3 + 0] = ok ? lse - zl : NAN;
        rowstat[ro * 3 + 1] = (ok && above < 1.f) ? 1.f : 0.f;
        rowstat[ro * 3 + 2] = (ok && above < 5.f) ? 1.f : 0.f;
      }
    }
    __syncthreads();   // the tile is the next head's
  }
}

// grid: ceil(C*K/4 / 256) weight blocks + 1 (biases + statistics); W == nullptr: statistics only.
// RM (RowMode, common.h): where batch row b of x comes from
template <int G, int RM>
__global__ __launch_bounds__(256) void linear_ce_sweep_sgd_kernel(
    const float* __restrict__ x, const float* __restrict__ dz, const int64_t* __restrict__ rows, long N, int B, int K,
    int C, float* __restrict__ W, float* __restrict__ bias, float* __restrict__ bufW, float* __restrict__ bufb,
    SweepHyper hp, float mom, int first, const float* __restrict__ rowstat, float* __restrict__ stats) {
  const int nw4 = C * K / 4;
  const size_t bc = (size_t)B * C;
  if (blockIdx.x + 1 < gridDim.x) {
    if (W == nullptr) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nw4) return;
    const int c = e / (K / 4), k = (e - c * (K / 4)) * 4;
    float4 g[G];
#pragma unroll
    for (int h = 0; h < G; ++h) g[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = 0; b < B; ++b) {
      const float4 v = load_x4<RM>(x, rows, N, b, K, k);
#pragma unroll
      for (int h = 0; h < G; ++h) {
        const float d = dz[h * bc + (size_t)b * C + c];
        g[h].x = fmaf(d, v.x, g[h].x);
        g[h].y = fmaf(d, v.y, g[h].y);
        g[h].z = fmaf(d, v.z, g[h].z);
        g[h].w = fmaf(d, v.w, g[h].w);
      }
    }
    const size_t ck = (size_t)C * K;
#pragma unroll
    for (int h = 0; h < G; ++h) {
      const float lr = hp.lr[h], wd = hp.wd[h];
      float4* wp = reinterpret_cast<float4*>(W + h * ck + (size_t)c * K + k);
      float4* bp = reinterpret_cast<float4*>(bufW + h * ck + (size_t)c * K + k);
      float4 w = *wp, bu = *bp;
      const float gg[4] = {g[h].x, g[h].y, g[h].z, g[h].w};
      float* ww = reinterpret_cast<float*>(&w);
      float* bb = reinterpret_cast<float*>(&bu);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float d = gg[q] + wd * ww[q];
        bb[q] = first ? d : fmaf(mom, bb[q], d);
        ww[q] -= lr * bb[q];
      }
      *wp = w;
      *bp = bu;
    }
    return;
  }
  // last block: bias gradients + updates, statistics in row order
  if (W != nullptr) {
    for (int c = threadIdx.x; c < C; c += 256) {
#pragma unroll
      for (int h = 0; h < G; ++h) {
        const float lr = hp.lr[h], wd = hp.wd[h];
        float* bh = bias + (size_t)h * C;
        float* uh = bufb + (size_t)h * C;
        float g = 0.f;
        for (int b = 0; b < B; ++b) g += dz[h * bc + (size_t)b * C + c];
        const float d = g + wd * bh[c];
        uh[c] = first ? d : fmaf(mom, uh[c], d);
        bh[c] -= lr * uh[c];
      }
    }
  }
  if (threadIdx.x < 3 * G) {
    const int h = threadIdx.x / 3, j = threadIdx.x - 3 * h;
    const float* rs = rowstat + (size_t)h * B * 3;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += rs[(size_t)b * 3 + j];
    stats[threadIdx.x] = s;
  }
}

bool sweep_shape_ok(int G, int B, int K, int C) {
  if (G < 1 || G > kMaxHeads || B < 1 || C < 1 || C > kMaxClasses) return false;
  if (K < 64 || K > 64 * 32 || K % 64 != 0 || ((K / 64) & (K / 64 - 1)) != 0) return false;
  const long lim = 1L << 31;
  return (long)G * B * C < lim && (long)B * K < lim && (long)G * C * K < lim;
}

}  // namespace

bool linear_ce_sweep_supported(int G, int K, int C) { return sweep_shape_ok(G, 1, K, C); }

hipError_t launch_linear_ce_sweep_fwd(const float* x, const float* W, const float* bias, const int64_t* labels, int G,
                                      int B, int K, int C, float gscale, float* logits, float* dz, float* rowstat,
                                      hipStream_t s, const int64_t* rows, long N) {
  if (!sweep_shape_ok(G, B, K, C) || (rows != nullptr && N < 1)) return hipErrorInvalidValue;
  if (x == nullptr || W == nullptr || bias == nullptr || labels == nullptr || logits == nullptr || rowstat == nullptr)
    return hipErrorInvalidValue;
  // (a bank is read 4 bytes at a time here: any alignment)
  if (((rows == nullptr ? (uintptr_t)x : 0) | (uintptr_t)W) & 15) return hipErrorInvalidValue;
  const dim3 grid((B + kRows - 1) / kRows), blk(256);
  switch (K / 64) {
#define SDX_LCS(KJ)                                                                                              \
  case KJ:                                                                                                      \
    if (rows != nullptr)                                                                                        \
      hipLaunchKernelGGL((linear_ce_sweep_fwd_kernel<KJ, true>), grid, blk, 0, s, x, W, bias, labels, rows, N, G, \
                         B, C, gscale, logits, dz, rowstat);                                                    \
    else                                                                                                        \
      hipLaunchKernelGGL((linear_ce_sweep_fwd_kernel<KJ, false>), grid, blk, 0, s, x, W, bias, labels, rows, N, G, \
                         B, C, gscale, logits, dz, rowstat);                                                    \
    break;
    SDX_LCS(1) SDX_LCS(2) SDX_LCS(4) SDX_LCS(8) SDX_LCS(16) SDX_LCS(32)
#undef SDX_LCS
    default:
      return hipErrorInvalidValue;
  }
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_linear_ce_sweep_sgd(const float* x, const float* dz, int G, int B, int K, int C, float* W,
                                      float* bias, float* bufW, float* bufb, const float* lrs, const float* wds,
                                      float mom, int first, const float* rowstat, float* stats, hipStream_t s,
                                      const int64_t* rows, long N) {
  if (!sweep_shape_ok(G, B, K, C) || (rows != nullptr && N < 1)) return hipErrorInvalidValue;
  if (rowstat == nullptr || stats == nullptr) return hipErrorInvalidValue;
  SweepHyper hp = {};
  if (W != nullptr) {
    // the training form: every operand, and 16-byte accesses to x, W and the momentum buffer
    if (x == nullptr || dz == nullptr || bias == nullptr || bufW == nullptr || bufb == nullptr || lrs == nullptr ||
        wds == nullptr)
      return hipErrorInvalidValue;
    if (((rows == nullptr ? (uintptr_t)x : 0) | (uintptr_t)W | (uintptr_t)bufW) & 15) return hipErrorInvalidValue;
    for (int h = 0; h < G; ++h) {
      hp.lr[h] = lrs[h];
      hp.wd[h] = wds[h];
    }
  }
  const int nw4 = C * K / 4;
  const dim3 grid(W != nullptr ? (nw4 + 255) / 256 + 1 : 1), blk(256);
  switch (G) {
#define SDX_LCS(GG)                                                                                              \
  case GG:                                                                                                      \
    if (rows == nullptr)                                                                                        \
      hipLaunchKernelGGL((linear_ce_sweep_sgd_kernel<GG, kRowsNone>), grid, blk, 0, s, x, dz, rows, N, B, K, C,  \
                         W, bias, bufW, bufb, hp, mom, first, rowstat, stats);                                  \
    else if (((uintptr_t)x & 15) == 0)                                                                          \
      hipLaunchKernelGGL((linear_ce_sweep_sgd_kernel<GG, kRowsVec>), grid, blk, 0, s, x, dz, rows, N, B, K, C,   \
                         W, bias, bufW, bufb, hp, mom, first, rowstat, stats);                                  \
    else                                                                                                        \
      hipLaunchKernelGGL((linear_ce_sweep_sgd_kernel<GG, kRowsScalar>), grid, blk, 0, s, x, dz, rows, N, B, K,   \
                         C, W, bias, bufW, bufb, hp, mom, first, rowstat, stats);                               \
    break;
    SDX_LCS(1) SDX_LCS(2) SDX_LCS(3) SDX_LCS(4) SDX_LCS(5) SDX_LCS(6) SDX_LCS(7) SDX_LCS(8)
    SDX_LCS(9) SDX_LCS(10) SDX_LCS(11) SDX_LCS(12) SDX_LCS(13) SDX_LCS(14) SDX_LCS(15) SDX_LCS(16)
#undef SDX_LCS
    default:
      return hipErrorInvalidValue;
  }
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
