// SwAV loss for gfx950 (--method SwAV, two crops): the prototype scores of both views, Sinkhorn-Knopp
// over them, the swapped soft-target cross-entropy and the backward. The GEMMs run on
// v_mfma_f32_16x16x32_bf16 with fp32 operands split into bf16 hi + lo (bf16x3_stage.h) on the double-
// buffered 64 x 128 tile loop mma_tile (loss_gemm.h), their tiles walked in groups per XCD
// (grouped_walk, xcd_remap). fp32 in, fp32 out.
//
//   swav_prep       one wave per row of (z1; z2; C): Σx² in fp64, the lanes strided over D and added by
//                   a butterfly; ẑ = z·rn with rn = fp32(1 / max(‖z‖, 1e-12)) and rn itself for the views,
//                   C's row scaled in place.
//   swav_scores     S_v = ẑ_v·Cᵀ, both views in one launch (tile ranges), both operands read along
//                   their rows. S has the leading dimension Kp = 64·ceil(K / 64); a prototype row
//                   >= K is staged as zeros, so the padding columns are stored as exact zeros. The
//                   epilogue adds E = exp((S − 1)/ε) over the tile's 64 rows from the accumulators
//                   (8 in a lane, the 4 row groups by two shuffles, the 2 row waves through LDS) and
//                   writes row (view, tile row) of the first prototype sum's partials.
//   swav_rowsum     partials [2][T][K] -> r [2][K], the T rows added in ascending order. r is the
//                   one tensor a multi-rank run all-reduces, so the Sinkhorn kernel takes r and not
//                   the partials: the partials are added once, not once per strip, u = 1/(K·r) costs a
//                   lane one division per 4 rows, and no K floats of LDS (64 KiB at K = 16384, all a
//                   workgroup can name statically) are held for them.
//   swav_sinkhorn   one launch per iteration; a workgroup owns 16 sample rows of one view, a wave 4 of
//                   them: c_b = Σ_k E[b][k]·u_k with the lanes strided over K, E recomputed from S,
//                   fp64 partials and a butterfly. v_b = 1/(N·c_b) goes through LDS and thread t then
//                   adds E[b][k]·v_b over the strip's rows, ascending, for the columns k ≡ t (mod 256):
//                   one row of the next r's partials. The last launch writes u and c instead.
//   swav_loss_grad  a workgroup per sample b reads rows b of S_1 and S_2 three times (L2): the maxima;
//                   Z_v = Σ exp((S_v − max)/τ) and Σ_k q_v in fp64; then q_v = u_v·E_v/c_v and
//                   p_v = exp(·)/Z_v on the fly, the row's Σ q_2·log p_1 + q_1·log p_2 in fp64 and
//                   dS_1 = (p_1·Σq_2 − q_2)/(2Nτ), dS_2 alike, the padding columns zero.
//                   swav_loss_finish (one block) adds the row terms in a fixed order.
//   swav_gemm       dẑ = dS·C (A along its rows over the padded K, B strided) and dC = g·dSᵀ·ẑ (both
//                   strided, the reduction over the 2N rows of both views at once) on the same loop.
//   swav_dz         one wave per row: dz = g·(dẑ − ẑ·(ẑ·dẑ))·rn, the dot product in fp64.
//
// Determinism: no atomics, no split reduction, no cross-workgroup wait; every cross-workgroup sum
// goes through a partials buffer that a later launch adds in a fixed order.
#include "common.h"
#include "launchers.h"
#include "loss_gemm.h"
#include "swav_plan.h"

using namespace sdx;

namespace {

namespace sp = sdx_swav;
using namespace sdx_stage;   // Operand, mma_tile

constexpr int TM = sp::kTileM;
constexpr int TN = sp::kTile;
constexpr int ROW_B = kStageRowB;
constexpr int STAGE_B = 2 * 2 * (TM + TN) * ROW_B;   // 48 KiB

// 256 threads: the 4 wave sums added in wave order, the result in every thread
__device__ __forceinline__ double block_sum(double v, double* slot) {
  v = wave_sum_f64(v);
  __syncthreads();   // the slots' last readers are done
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

__device__ __forceinline__ float block_max(float v, float* slot) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(slot[0], slot[1]), fmaxf(slot[2], slot[3]));
}

// ---- swav_prep -------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void swav_prep_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                        float* C, int n, int D, int K, float* __restrict__ zhat,
                                                        float* __restrict__ rnorm) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= 2 * n + K) return;
  const bool proto = row >= 2 * n;
  const float* src = proto ? C + (size_t)(row - 2 * n) * D
                           : (row < n ? z1 + (size_t)row * D : z2 + (size_t)(row - n) * D);
  float* dst = proto ? C + (size_t)(row - 2 * n) * D : zhat + (size_t)row * D;
  double ss = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double x = (double)src[d];
    ss += x * x;
  }
  ss = wave_sum_f64(ss);
  const float rn = (float)(1.0 / fmax(sqrt(ss), 1e-12));
  for (int d = lane; d < D; d += 64) dst[d] = src[d] * rn;   // a lane rewrites what it alone read
  if (!proto && lane == 0) rnorm[row] = rn;
}

// ---- swav_scores -----------------------------------------------------------------------------

struct ScoreParams {
  Operand a[2];   // ẑ_v [N][D]
  Operand b;      // C [K][D]
  float* S;       // [2N][Kp]
  float* part;    // [2][tiles_m][K]
  int N, K, Kp, chunks, tiles_m, tiles_n, tiles;   // tiles per view
  float inv_eps;
};

__global__ __launch_bounds__(256) void swav_scores_kernel(ScoreParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[STAGE_B];
  __shared__ float colsum[2][TN];
  const int lt = xcd_remap(blockIdx.x, 2 * p.tiles);
  const int view = lt >= p.tiles ? 1 : 0;
  const sp::TilePos tp = sp::grouped_walk(lt - view * p.tiles, p.tiles_m, p.tiles_n, sp::kGroup);
  SDX_DCHECK(tp.row < p.tiles_m && tp.col < p.tiles_n);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wm = wv >> 1, wn = wv & 1, h = lane >> 4, c = lane & 15;
  const int m0 = tp.row * TM, n0 = tp.col * TN;
  f32x4 acc[TM / 32][4];
  mma_tile<TM, kRow, kRaw, kRow, kRaw, false>(p.a[view], p.b, m0, n0, p.chunks, false, stage, acc);
  float* S = p.S + (size_t)view * p.N * p.Kp;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int n = n0 + wn * 64 + 16 * u + c;
    float e = 0.f;
#pragma unroll
    for (int t = 0; t < TM / 32; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * (TM / 2) + 16 * t + 4 * h + r;
        if (m < p.N && n < p.Kp) {
          SDX_DCHECK((size_t)m * p.Kp + n < (size_t)p.N * p.Kp);
          S[(size_t)m * p.Kp + n] = acc[t][u][r];
          e += __expf((acc[t][u][r] - 1.f) * p.inv_eps);
        }
      }
    e += __shfl_xor(e, 16, 64);
    e += __shfl_xor(e, 32, 64);
    if (h == 0) colsum[wm][wn * 64 + 16 * u + c] = e;
  }
  __syncthreads();
  const int n = n0 + (int)threadIdx.x;
  if (threadIdx.x < TN && n < p.K)
    p.part[((size_t)view * p.tiles_m + tp.row) * p.K + n] = colsum[0][threadIdx.x] + colsum[1][threadIdx.x];
}

// ---- swav_rowsum, swav_sinkhorn --------------------------------------------------------------

__global__ __launch_bounds__(256) void swav_rowsum_kernel(const float* __restrict__ part, int T, int K,
                                                          float* __restrict__ r) {
  const int e = blockIdx.x * 256 + threadIdx.x;   // (view, k)
  if (e >= 2 * K) return;
  const int view = e >= K ? 1 : 0, k = e - view * K;
  const float* p = part + (size_t)view * T * K + k;
  float s = 0.f;
  for (int t = 0; t < T; ++t) s += p[(size_t)t * K];
  r[e] = s;
}

// part != nullptr: one row of the next r's partials per strip; else u [2][K] and c [2N]
__global__ __launch_bounds__(256) void swav_sinkhorn_kernel(const float* __restrict__ S, const float* __restrict__ r,
                                                            int N, int K, int Kp, int strips, float inv_eps,
                                                            float n_total, float* __restrict__ part,
                                                            float* __restrict__ u_out, float* __restrict__ c_out) {
  constexpr int WR = sp::kWaveRows;
  __shared__ float vrow[sp::kStrip];
  const int view = (int)blockIdx.x >= strips ? 1 : 0;
  const int strip = (int)blockIdx.x - view * strips;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* Sv = S + (size_t)view * N * Kp;
  const float* rv = r + (size_t)view * K;
  const float kf = (float)K;
  const int b0 = strip * sp::kStrip + wv * WR;
  const float* row[WR];
#pragma unroll
  for (int j = 0; j < WR; ++j) row[j] = Sv + (size_t)(b0 + j < N ? b0 + j : N - 1) * Kp;
  double acc[WR] = {};
  for (int k = lane; k < K; k += 64) {
    const float u = 1.f / (kf * rv[k]);
#pragma unroll
    for (int j = 0; j < WR; ++j) acc[j] += (double)(__expf((row[j][k] - 1.f) * inv_eps) * u);
  }
#pragma unroll
  for (int j = 0; j < WR; ++j) {
    const float cb = (float)wave_sum_f64(acc[j]);
    if (lane == 0) {
      const bool in = b0 + j < N;
      if (in && c_out != nullptr) c_out[(size_t)view * N + b0 + j] = cb;
      vrow[wv * WR + j] = in ? 1.f / (n_total * cb) : 0.f;   // a row past the view adds nothing
    }
  }
  if (part == nullptr) {
    if (strip == 0)
      for (int k = tid; k < K; k += 256) u_out[(size_t)view * K + k] = 1.f / (kf * rv[k]);
    return;
  }
  __syncthreads();
  float* out = part + ((size_t)view * strips + strip) * K;
  for (int k = tid; k < K; k += 256) {
    double s = 0.0;
#pragma unroll 4
    for (int j = 0; j < sp::kStrip; ++j) {
      const int b = strip * sp::kStrip + j;
      const float sv = Sv[(size_t)(b < N ? b : N - 1) * Kp + k];
      s += (double)(__expf((sv - 1.f) * inv_eps) * vrow[j]);
    }
    out[k] = (float)s;
  }
}

// ---- swav_loss_grad --------------------------------------------------------------------------

// scale = 1/(2·N·τ)
__global__ __launch_bounds__(256) void swav_loss_grad_kernel(const float* __restrict__ S, const float* __restrict__ u,
                                                             const float* __restrict__ c, int N, int K, int Kp,
                                                             float inv_eps, float inv_temp, float scale,
                                                             float* __restrict__ dS, float* __restrict__ qsum,
                                                             double* __restrict__ rowloss) {
  __shared__ float fslot[4];
  __shared__ double dslot[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* s1 = S + (size_t)b * Kp;
  const float* s2 = S + (size_t)(N + b) * Kp;
  const float* u1 = u;
  const float* u2 = u + K;
  const float rc1 = 1.f / c[b], rc2 = 1.f / c[N + b];
  float m1 = -2.f, m2 = -2.f;   // |S| <= 1 up to rounding
  for (int k = tid; k < K; k += 256) {
    m1 = fmaxf(m1, s1[k]);
    m2 = fmaxf(m2, s2[k]);
  }
  m1 = block_max(m1, fslot);
  m2 = block_max(m2, fslot);
  double z1 = 0.0, z2 = 0.0, q1s = 0.0, q2s = 0.0;
  for (int k = tid; k < K; k += 256) {
    const float a1 = s1[k], a2 = s2[k];
    z1 += (double)__expf((a1 - m1) * inv_temp);
    z2 += (double)__expf((a2 - m2) * inv_temp);
    q1s += (double)(u1[k] * __expf((a1 - 1.f) * inv_eps) * rc1);
    q2s += (double)(u2[k] * __expf((a2 - 1.f) * inv_eps) * rc2);
  }
  const float Z1 = (float)block_sum(z1, dslot), Z2 = (float)block_sum(z2, dslot);
  const float sq1 = (float)block_sum(q1s, dslot), sq2 = (float)block_sum(q2s, dslot);
  const float rz1 = 1.f / Z1, rz2 = 1.f / Z2;
  const float lz1 = __logf(Z1), lz2 = __logf(Z2);
  float* d1 = dS + (size_t)b * Kp;
  float* d2 = dS + (size_t)(N + b) * Kp;
  double l = 0.0;
  for (int k = tid; k < Kp; k += 256) {
    if (k >= K) {
      d1[k] = 0.f;
      d2[k] = 0.f;
      continue;
    }
    const float a1 = s1[k], a2 = s2[k];
    const float x1 = (a1 - m1) * inv_temp, x2 = (a2 - m2) * inv_temp;
    const float p1 = __expf(x1) * rz1, p2 = __expf(x2) * rz2;
    const float q1 = u1[k] * __expf((a1 - 1.f) * inv_eps) * rc1;
    const float q2 = u2[k] * __expf((a2 - 1.f) * inv_eps) * rc2;
    l += (double)q2 * (double)(x1 - lz1) + (double)q1 * (double)(x2 - lz2);
    d1[k] = (p1 * sq2 - q2) * scale;
    d2[k] = (p2 * sq1 - q1) * scale;
  }
  l = block_sum(l, dslot);
  if (tid == 0) {
    rowloss[b] = l;
    qsum[b] = sq1;
    qsum[N + b] = sq2;
  }
}

// one block: thread t the rows ≡ t (mod 256) ascending, then the 256 partials in thread order
__global__ __launch_bounds__(256) void swav_loss_finish_kernel(const double* __restrict__ rowloss, int N,
                                                               double n_total, float* __restrict__ loss) {
  __shared__ double part[256];
  double s = 0.0;
  for (int b = threadIdx.x; b < N; b += 256) s += rowloss[b];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = 0.0;
  for (int t = 0; t < 256; ++t) s += part[t];
  loss[0] = (float)(-s / (2.0 * n_total));
}

// ---- backward --------------------------------------------------------------------------------

struct GemmParams {
  Operand a, b;
  float* out;       // [M][ldo]
  const float* g;   // scales the output; nullptr: 1
  int M, N, ldo, chunks, tiles_m, tiles_n;
};

template <int MA, int MB>
__global__ __launch_bounds__(256) void swav_gemm_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[STAGE_B];
  const sp::TilePos tp = sp::grouped_walk(xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n), p.tiles_m, p.tiles_n,
                                          sp::kGroup);
  SDX_DCHECK(tp.row < p.tiles_m && tp.col < p.tiles_n);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wm = wv >> 1, wn = wv & 1, h = lane >> 4, c = lane & 15;
  const int m0 = tp.row * TM, n0 = tp.col * TN;
  f32x4 acc[TM / 32][4];
  mma_tile<TM, MA, kRaw, MB, kRaw, false>(p.a, p.b, m0, n0, p.chunks, false, stage, acc);
  const float go = p.g != nullptr ? p.g[0] : 1.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int n = n0 + wn * 64 + 16 * u + c;
    if (n >= p.N) continue;
#pragma unroll
    for (int t = 0; t < TM / 32; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * (TM / 2) + 16 * t + 4 * h + r;
        if (m >= p.M) continue;
        SDX_DCHECK((size_t)m * p.ldo + n < (size_t)p.M * p.ldo);
        p.out[(size_t)m * p.ldo + n] = go * acc[t][u][r];
      }
  }
}

__global__ __launch_bounds__(256) void swav_dz_kernel(const float* __restrict__ zhat, const float* __restrict__ rnorm,
                                                      const float* __restrict__ dzhat, const float* __restrict__ g,
                                                      int rows, int D, float* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* zh = zhat + (size_t)row * D;
  const float* dh = dzhat + (size_t)row * D;
  double dot = 0.0;
  for (int d = lane; d < D; d += 64) dot += (double)zh[d] * (double)dh[d];
  const float dt = (float)wave_sum_f64(dot);
  const float sc = g[0] * rnorm[row];
  for (int d = lane; d < D; d += 64) dz[(size_t)row * D + d] = (dh[d] - zh[d] * dt) * sc;
}

bool pos(double x) { return x > 0.0 && x < 1e30; }

}  // namespace

bool swav_supported(long n, long D, long K, long iters) { return sp::supported(n, D, K, iters); }

hipError_t launch_swav_prep(const float* z1, const float* z2, float* C, int n, int D, int K, float* zhat,
                            float* rnorm, hipStream_t s) {
  if (!sp::supported(n, D, K) || z1 == nullptr || z2 == nullptr || C == nullptr || zhat == nullptr ||
      rnorm == nullptr)
    return hipErrorInvalidValue;
  const int rows = 2 * n + K;
  hipLaunchKernelGGL(swav_prep_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, z1, z2, C, n, D, K, zhat, rnorm);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_swav_scores(const float* zhat, const float* C, int n, int D, int K, double eps, float* S,
                              float* part, hipStream_t s) {
  sp::Plan pl;
  if (!sp::make_plan(n, D, K, &pl) || zhat == nullptr || C == nullptr || S == nullptr || part == nullptr ||
      !pos(eps) || !sp::aligned16(zhat) || !sp::aligned16(C))
    return hipErrorInvalidValue;
  ScoreParams p = {};
  p.a[0] = operand(zhat, n, D, D, 1);
  p.a[1] = operand(zhat + (size_t)n * D, n, D, D, 1);
  p.b = operand(C, K, D, D, 1);
  p.S = S; p.part = part;
  p.N = n; p.K = K; p.Kp = pl.kp; p.chunks = pl.s_chunks;
  p.tiles_m = pl.s_tiles_m; p.tiles_n = pl.s_tiles_n; p.tiles = pl.s_tiles;
  p.inv_eps = (float)(1.0 / eps);
  hipLaunchKernelGGL(swav_scores_kernel, dim3(2 * pl.s_tiles), dim3(256), 0, s, p);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_swav_rowsum(const float* part, int T, int K, float* r, hipStream_t s) {
  if (part == nullptr || r == nullptr || T < 1 || K < sp::kMinK || K > sp::kMaxK) return hipErrorInvalidValue;
  hipLaunchKernelGGL(swav_rowsum_kernel, dim3((2 * K + 255) / 256), dim3(256), 0, s, part, T, K, r);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_swav_sinkhorn(const float* S, const float* r, int n, int K, double eps, double n_total, float* part,
                                float* u, float* c, hipStream_t s) {
  sp::Plan pl;
  if (!sp::make_plan(n, sp::kMinD, K, &pl) || S == nullptr || r == nullptr || !pos(eps) || !(n_total >= n))
    return hipErrorInvalidValue;
  if (part == nullptr && (u == nullptr || c == nullptr)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(swav_sinkhorn_kernel, dim3(2 * pl.strips), dim3(256), 0, s, S, r, n, K, pl.kp, pl.strips,
                     (float)(1.0 / eps), (float)n_total, part, part != nullptr ? nullptr : u,
                     part != nullptr ? nullptr : c);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_swav_loss_grad(const float* S, const float* u, const float* c, int n, int K, double eps, double temp,
                                 double n_total, float* dS, float* qsum, double* rowloss, float* loss,
                                 hipStream_t s) {
  sp::Plan pl;
  if (!sp::make_plan(n, sp::kMinD, K, &pl) || S == nullptr || u == nullptr || c == nullptr || dS == nullptr ||
      qsum == nullptr || rowloss == nullptr || loss == nullptr || !pos(eps) || !pos(temp) || !(n_total >= n))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(swav_loss_grad_kernel, dim3(n), dim3(256), 0, s, S, u, c, n, K, pl.kp, (float)(1.0 / eps),
                     (float)(1.0 / temp), (float)(1.0 / (2.0 * n_total * temp)), dS, qsum, rowloss);
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(swav_loss_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)rowloss, n, n_total, loss);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_swav_bwd(const float* zhat, const float* rnorm, const float* C, const float* dS, const float* g,
                           int n, int D, int K, float* dzhat, float* dz, float* dC, hipStream_t s) {
  sp::Plan pl;
  if (!sp::make_plan(n, D, K, &pl) || zhat == nullptr || rnorm == nullptr || C == nullptr || dS == nullptr ||
      g == nullptr || dzhat == nullptr || dz == nullptr || !sp::aligned16(dS))
    return hipErrorInvalidValue;
  GemmParams p = {};
  p.a = operand(dS, 2 * n, pl.kp, pl.kp, 1);   // (row, k), the padding columns are zeros
  p.b = operand(C, D, K, 1, D);                // (d, k) at C[k][d]
  p.out = dzhat; p.g = nullptr;
  p.M = 2 * n; p.N = D; p.ldo = D; p.chunks = pl.z_chunks; p.tiles_m = pl.z_tiles_m; p.tiles_n = pl.z_tiles_n;
  hipLaunchKernelGGL((swav_gemm_kernel<kRow, kTrans>), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, s, p);
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(swav_dz_kernel, dim3((2 * n + 3) / 4), dim3(256), 0, s, zhat, rnorm, (const float*)dzhat, g, 2 * n,
                     D, dz);
  SDX_LAUNCH_CHECK();
  if (dC == nullptr) return hipSuccess;   // frozen prototypes
  p.a = operand(dS, K, 2 * n, 1, pl.kp);       // (k, row) at dS[row][k]
  p.b = operand(zhat, D, 2 * n, 1, D);         // (d, row) at ẑ[row][d]
  p.out = dC; p.g = g;
  p.M = K; p.N = D; p.ldo = D; p.chunks = pl.c_chunks; p.tiles_m = pl.c_tiles_m; p.tiles_n = pl.c_tiles_n;
  hipLaunchKernelGGL((swav_gemm_kernel<kTrans, kTrans>), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, s, p);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
