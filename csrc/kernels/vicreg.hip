// VICReg loss for gfx950 (--method VICReg): the two D x D auto-covariances of the column-centred
// projections, the variance hinge and covariance penalty read off them, and the backward, on
// v_mfma_f32_16x16x32_bf16 with fp32 operands split into bf16 hi + lo (a product is hi·hi + hi·lo +
// lo·hi, three MFMAs, the lo·lo term dropped). The staging (bf16x3_stage.h), the column-statistics
// sum (loss_gemm.h) and the tile map grouped_walk (loss_gemm_plan.h, with tri_fold) are shared with barlow.hip;
// the tile loop mma_tile (loss_gemm.h) is used here alone.
// fp32 in, fp32 out.
//
//   vic_colstats   per-column Σz1, Σz2 and Σ(z1 − z2)² in fp64 ([3][D]): a block owns 64 columns of
//                  both views, its 4 waves rows n ≡ w (mod 4) in ascending order, the 4 partials are
//                  added in wave order. Finalised in the same launch to μ [2][D] when the batch is on
//                  one rank; vic_stats_finalize does it alone after an all-reduce of the sums. The
//                  third row is the invariance term, so it needs no reduction of its own.
//   vic_cov        C_v = x̄_vᵀ·x̄_v / (N − 1), both views in one launch. C_v is symmetric, so a
//                  workgroup (4 waves, 2 x 2) owns one 128 x 128 tile (ti, tj) with ti <= tj only:
//                  T(T + 1)/2 tiles per view instead of T². The triangle is folded into a rectangle
//                  (tri_fold) that is walked 4 rows down before the next column (grouped_walk), and xcd_remap
//                  puts consecutive logical tiles on one XCD: tiles resident together share operand
//                  strips in that XCD's L2. The reduction (the batch) goes through LDS in 32-row
//                  chunks, ascending, never split; lanes run along the columns (kTrans) and an element
//                  is centred, masked and split when it is committed. The chunk loop is double-
//                  buffered: two (hi, lo) image pairs for A and B, 64 KiB, ONE barrier per chunk —
//                  chunk k + 1 is loaded before the MFMAs of chunk k and committed to the other
//                  buffer after them. A diagonal tile stages its strip once and both MFMA operands
//                  read that one image; its wave below the diagonal (rows 64.., columns ..63) issues no
//                  MFMAs. Epilogue: an off-diagonal tile stores acc / (N − 1) at (ti, tj) and the same
//                  fp32 values at (tj, ti). The mirror needs no LDS pass: the 4 accumulator registers
//                  of a lane are 4 consecutive rows of the tile, i.e. 4 consecutive columns of the
//                  mirror, so it is stored straight from the registers as one float4 per lane and
//                  accumulator — 64-byte segments per row, as the direct store has. A diagonal tile
//                  stores only the entries with column >= row, each at both places. C_v is therefore
//                  symmetric bit for bit and everything after it is a plain row-major consumer.
//   vic_loss_grad  one pass over C [2][D][D]: a block owns 8 rows of one view, a thread 4 adjacent
//                  columns of every 1024. G_v = 4ν/(D(N − 1))·offdiag(C_v) overwrites C_v; the thread
//                  that owns a diagonal element writes coef_v[j] = μ·[S < 1]/(2·D·(N − 1)·S), S =
//                  sqrt(C_jj + ε), and adds the hinge relu(1 − S). Thread partials in fp32, fp64 from
//                  there on, one slot per block. vic_loss_finish (one block) adds the slots and the
//                  third colstats row in fp64 — thread t the entries ≡ t (mod 256) ascending, then the
//                  256 partials in thread order — and writes terms [3] and the loss, device scalars.
//   vic_bwd        dz_v = g·(x̄_v·G_v − coef_v ⊙ x̄_v + 2λ/(N·D)·(z_v − z_other)), both views in one
//                  launch (tile ranges), 64 x 128 output tiles, reduction over D on the same double-
//                  buffered loop. A = x̄_v is staged along its rows and centred on commit; B = G_v is
//                  read along its rows for both views (G_v is symmetric). The epilogue recomputes x̄_v
//                  and z_v − z_other at the accumulator's coordinates; g is a device scalar.
//
// Determinism: no atomics, no split reduction; every sum's order is a function of (n, D).
#include "common.h"
#include "launchers.h"
#include "loss_gemm.h"
#include "vicreg_plan.h"

using namespace sdx;

namespace {

namespace vp = sdx_vicreg;
using namespace sdx_stage;   // Operand, Stager, mma_tile, add_row_groups

constexpr int TN = vp::kTile;
constexpr int ROW_B = kStageRowB;

// ---- vic_cov -----------------------------------------------------------------------------

struct CovParams {
  Operand x[2];   // per view: element (i = column of z, r = batch row) at z[r·D + i], μ of the view
  float* C;       // [2][D][D]
  int D, chunks, T, fold_w, fold_h, tiles;   // tiles per view
  float nm1;      // N − 1
};

__global__ __launch_bounds__(256) void vic_cov_kernel(CovParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[2 * 2 * (TN + TN) * ROW_B];   // 64 KiB
  const int lt = xcd_remap(blockIdx.x, 2 * p.tiles);
  const int view = lt >= p.tiles ? 1 : 0;
  // logical tile of one view -> the folded rectangle, walked in groups -> (ti, tj), ti <= tj
  const vp::TilePos rc = vp::grouped_walk(lt - view * p.tiles, p.fold_h, p.fold_w, vp::kGroup);
  const vp::TilePos tt = vp::tri_fold(rc.row, rc.col, p.T);
  const int ti = tt.row, tj = tt.col;
  SDX_DCHECK(ti >= 0 && ti <= tj && tj < p.T);
  const Operand& x = p.x[view];
  const int D = p.D;
  float* C = p.C + (size_t)view * D * D;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wm = wv >> 1, wn = wv & 1, h = lane >> 4, c = lane & 15;
  const int m0 = ti * TN, n0 = tj * TN;
  f32x4 acc[4][4];
  if (ti != tj) {
    mma_tile<TN, kTrans, kCentre, kTrans, kCentre, false>(x, x, m0, n0, p.chunks, false, stage, acc);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = n0 + wn * 64 + 16 * u + c;
      if (n >= D) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int mb = m0 + wm * 64 + 16 * t + 4 * h;   // 4 | mb and 64 | D: the 4 rows are in or out together
        if (mb >= D) continue;
        SDX_DCHECK(mb + 3 < D);
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = acc[t][u][r] / p.nm1;
          C[(size_t)(mb + r) * D + n] = v[r];
        }
        *reinterpret_cast<float4*>(C + (size_t)n * D + mb) = make_float4(v[0], v[1], v[2], v[3]);   // the mirror
      }
    }
  } else {
    const bool below = wm > wn;   // rows 64.., columns ..63 of a diagonal tile: the mirror of wave (0, 1)
    mma_tile<TN, kTrans, kCentre, kTrans, kCentre, true>(x, x, m0, n0, p.chunks, below, stage, acc);
    if (below) return;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = n0 + wn * 64 + 16 * u + c;
      if (n >= D) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm * 64 + 16 * t + 4 * h + r;
          if (m > n) continue;   // m <= n < D
          const float v = acc[t][u][r] / p.nm1;
          C[(size_t)m * D + n] = v;
          if (m != n) C[(size_t)n * D + m] = v;
        }
    }
  }
}

// ---- vic_bwd -----------------------------------------------------------------------------

struct BwdView {
  Operand a, b;        // A = x̄_v [n][k] (kRow, centred), B[d][k] = G_v[d][k] (kRow)
  const float* z;      // epilogue: this view's z and μ, the other view's z, coef_v
  const float* zo;
  const float* mu;
  const float* coef;
  float* out;
};

struct BwdParams {
  BwdView v[2];
  int M, N, chunks, tiles_m, tiles_n, tiles;
  float sim2;          // 2λ/(N·D)
  const float* g;
};

__global__ __launch_bounds__(256) void vic_bwd_kernel(BwdParams p) {
  constexpr int TM = vp::kTileMB;
  __shared__ __attribute__((aligned(16))) unsigned char stage[2 * 2 * (TM + TN) * ROW_B];   // 48 KiB
  const int view = (int)blockIdx.x >= p.tiles ? 1 : 0;
  const BwdView& bv = p.v[view];
  const vp::TilePos tp = vp::grouped_walk(xcd_remap((int)blockIdx.x - view * p.tiles, p.tiles), p.tiles_m,
                                          p.tiles_n, vp::kGroup);
  SDX_DCHECK(tp.row < p.tiles_m && tp.col < p.tiles_n);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wm = wv >> 1, wn = wv & 1, h = lane >> 4, c = lane & 15;
  const int m0 = tp.row * TM, n0 = tp.col * TN;
  f32x4 acc[TM / 32][4];
  mma_tile<TM, kRow, kCentre, kRow, kRaw, false>(bv.a, bv.b, m0, n0, p.chunks, false, stage, acc);
  const float go = p.g[0];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int n = n0 + wn * 64 + 16 * u + c;
    if (n >= p.N) continue;
    const float mu = bv.mu[n], cf = bv.coef[n];
#pragma unroll
    for (int t = 0; t < TM / 32; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * (TM / 2) + 16 * t + 4 * h + r;
        if (m >= p.M) continue;
        const size_t e = (size_t)m * p.N + n;
        SDX_DCHECK(e < (size_t)p.M * p.N);
        const float zv = bv.z[e];
        bv.out[e] = go * (acc[t][u][r] - cf * (zv - mu) + p.sim2 * (zv - bv.zo[e]));
      }
  }
}

// ---- statistics, loss ------------------------------------------------------------------------

__global__ __launch_bounds__(256) void vic_colstats_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                           int n, int D, double* __restrict__ sums,
                                                           float* __restrict__ mu, double n_total) {
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int col = blockIdx.x * vp::kStatCols + cl;
  double s1 = 0.0, s2 = 0.0, q = 0.0;
#pragma unroll 8
  for (int i = rg; i < n; i += 4) {
    const double a = (double)z1[(size_t)i * D + col], b = (double)z2[(size_t)i * D + col];
    const double d = a - b;
    s1 += a;
    s2 += b;
    q += d * d;
  }
  double s[3] = {s1, s2, q};
  if (add_row_groups(s)) {
    sums[col] = s[0];
    sums[(size_t)D + col] = s[1];
    sums[2 * (size_t)D + col] = s[2];
    if (mu != nullptr) {
      mu[col] = (float)(s[0] / n_total);
      mu[(size_t)D + col] = (float)(s[1] / n_total);
    }
  }
}

__global__ __launch_bounds__(256) void vic_stats_finalize_kernel(const double* __restrict__ sums, int D,
                                                                 double n_total, float* __restrict__ mu) {
  const int e = blockIdx.x * 256 + threadIdx.x;   // (view, column): rows 0 and 1 of sums
  if (e < 2 * D) mu[e] = (float)(sums[e] / n_total);
}

// scale = 4ν/(D(N − 1)), cf = μ/(2·D·(N − 1))
__global__ __launch_bounds__(256) void vic_loss_grad_kernel(float* __restrict__ C, int D, float scale, float cf,
                                                            float eps, float* __restrict__ coef,
                                                            double* __restrict__ cov_part,
                                                            double* __restrict__ std_part) {
  constexpr int RB = vp::kLossRows;
  __shared__ double part[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int per_view = D / RB;
  const int view = (int)blockIdx.x >= per_view ? 1 : 0;
  const int i0 = ((int)blockIdx.x - view * per_view) * RB;
  float* Cv = C + (size_t)view * D * D;
  float cs = 0.f, hs = 0.f;
  for (int j0 = tid * 4; j0 < D; j0 += 1024) {
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int i = i0 + r;
      float4* pc = reinterpret_cast<float4*>(Cv + (size_t)i * D + j0);
      const float4 c4 = *pc;
      const float x[4] = {c4.x, c4.y, c4.z, c4.w};
      float g[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i == j0 + e) {
          const float S = sqrtf(x[e] + eps);
          hs += fmaxf(1.f - S, 0.f);
          coef[(size_t)view * D + i] = S < 1.f ? cf / S : 0.f;
          g[e] = 0.f;
        } else {
          cs += x[e] * x[e];
          g[e] = scale * x[e];
        }
      }
      *pc = make_float4(g[0], g[1], g[2], g[3]);
    }
  }
  const double cw = wave_sum_f64((double)cs), hw = wave_sum_f64((double)hs);
  if (lane == 0) {
    part[0][wv] = cw;
    part[1][wv] = hw;
  }
  __syncthreads();
  if (tid == 0) {
    cov_part[blockIdx.x] = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
    std_part[blockIdx.x] = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
  }
}

// one block. sim_row: the third colstats row (Σ_n (z1 − z2)² per column, the whole batch)
__global__ __launch_bounds__(256) void vic_loss_finish_kernel(const double* __restrict__ sim_row,
                                                              const double* __restrict__ cov_part,
                                                              const double* __restrict__ std_part, int D, int nblk,
                                                              double n_total, double sim_w, double std_w, double cov_w,
                                                              float* __restrict__ loss, float* __restrict__ terms) {
  __shared__ double part[3][256];
  const int tid = threadIdx.x;
  double s = 0.0, cv = 0.0, sd = 0.0;
  for (int j = tid; j < D; j += 256) s += sim_row[j];
  for (int b = tid; b < nblk; b += 256) {
    cv += cov_part[b];
    sd += std_part[b];
  }
  part[0][tid] = s;
  part[1][tid] = cv;
  part[2][tid] = sd;
  __syncthreads();
  if (tid != 0) return;
  s = cv = sd = 0.0;
  for (int t = 0; t < 256; ++t) {
    s += part[0][t];
    cv += part[1][t];
    sd += part[2][t];
  }
  const double l_sim = s / (n_total * (double)D), l_std = 0.5 * sd / (double)D, l_cov = cv / (double)D;
  terms[0] = (float)l_sim;
  terms[1] = (float)l_std;
  terms[2] = (float)l_cov;
  loss[0] = (float)(sim_w * l_sim + std_w * l_std + cov_w * l_cov);
}

bool weight_ok(double w) { return w >= 0.0 && w < 1e30; }

}  // namespace

bool vicreg_supported(long n, long D) { return vp::supported(n, D); }

hipError_t launch_vic_colstats(const float* z1, const float* z2, int n, int D, double* sums, float* mu,
                               double n_total, hipStream_t s) {
  vp::Plan pl;
  if (!vp::make_plan(n, D, &pl) || z1 == nullptr || z2 == nullptr || sums == nullptr) return hipErrorInvalidValue;
  if (!(n_total >= n)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vic_colstats_kernel, dim3(pl.stat_blocks), dim3(256), 0, s, z1, z2, n, D, sums, mu, n_total);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_vic_stats_finalize(const double* sums, int D, double n_total, float* mu, hipStream_t s) {
  if (!vp::supported(1, D) || sums == nullptr || mu == nullptr || !(n_total >= 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vic_stats_finalize_kernel, dim3((2 * D + 255) / 256), dim3(256), 0, s, sums, D, n_total, mu);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_vic_cov(const float* z1, const float* z2, const float* mu, int n, int D, double n_total, float* C,
                          hipStream_t s) {
  vp::Plan pl;
  if (!vp::make_plan(n, D, &pl) || z1 == nullptr || z2 == nullptr || mu == nullptr || C == nullptr)
    return hipErrorInvalidValue;
  if (!vp::aligned16(C) || !(n_total >= n) || !(n_total >= 2)) return hipErrorInvalidValue;
  CovParams p = {};
  p.x[0] = operand(z1, D, n, 1, D, mu);
  p.x[1] = operand(z2, D, n, 1, D, mu + D);
  p.C = C;
  p.D = D; p.chunks = pl.c_chunks; p.T = pl.c_t; p.fold_w = pl.c_fold_w; p.fold_h = pl.c_fold_h; p.tiles = pl.c_tiles;
  p.nm1 = (float)(n_total - 1.0);
  hipLaunchKernelGGL(vic_cov_kernel, dim3(2 * pl.c_tiles), dim3(256), 0, s, p);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_vic_loss_grad(float* C, const double* sums, int D, double sim_w, double std_w, double cov_w,
                                float eps, double n_total, float* loss, float* terms, float* coef, double* parts,
                                hipStream_t s) {
  vp::Plan pl;
  if (!vp::make_plan(1, D, &pl) || C == nullptr || sums == nullptr || loss == nullptr || terms == nullptr ||
      coef == nullptr || parts == nullptr)
    return hipErrorInvalidValue;
  if (!vp::aligned16(C) || !(n_total >= 2) || !weight_ok(sim_w) || !weight_ok(std_w) || !weight_ok(cov_w) ||
      !(eps >= 0.f))
    return hipErrorInvalidValue;
  const double dn = (double)D * (n_total - 1.0);
  double* cov_part = parts;
  double* std_part = parts + pl.loss_blocks;
  hipLaunchKernelGGL(vic_loss_grad_kernel, dim3(pl.loss_blocks), dim3(256), 0, s, C, D, (float)(4.0 * cov_w / dn),
                     (float)(std_w / (2.0 * dn)), eps, coef, cov_part, std_part);
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(vic_loss_finish_kernel, dim3(1), dim3(256), 0, s, sums + 2 * (size_t)D, (const double*)cov_part,
                     (const double*)std_part, D, pl.loss_blocks, n_total, sim_w, std_w, cov_w, loss, terms);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_vic_bwd(const float* z1, const float* z2, const float* G, const float* mu, const float* coef,
                          const float* g, int n, int D, double sim_w, double n_total, float* dz1, float* dz2,
                          hipStream_t s) {
  vp::Plan pl;
  if (!vp::make_plan(n, D, &pl) || z1 == nullptr || z2 == nullptr || G == nullptr || mu == nullptr ||
      coef == nullptr || g == nullptr || dz1 == nullptr || dz2 == nullptr)
    return hipErrorInvalidValue;
  if (!vp::aligned16(z1) || !vp::aligned16(z2) || !vp::aligned16(G) || !vp::aligned16(mu) || !(n_total >= n) ||
      !weight_ok(sim_w))
    return hipErrorInvalidValue;
  BwdParams p = {};
  const float* zs[2] = {z1, z2};
  float* outs[2] = {dz1, dz2};
  for (int v = 0; v < 2; ++v) {
    p.v[v].a = operand(zs[v], n, D, D, 1, mu + (size_t)v * D);
    p.v[v].b = operand(G + (size_t)v * D * D, D, D, D, 1);
    p.v[v].z = zs[v];
    p.v[v].zo = zs[1 - v];
    p.v[v].mu = mu + (size_t)v * D;
    p.v[v].coef = coef + (size_t)v * D;
    p.v[v].out = outs[v];
  }
  p.M = n; p.N = D; p.chunks = pl.b_chunks;
  p.tiles_m = pl.b_tiles_m; p.tiles_n = pl.b_tiles_n; p.tiles = pl.b_tiles;
  p.sim2 = (float)(2.0 * sim_w / (n_total * (double)D));
  p.g = g;
  hipLaunchKernelGGL(vic_bwd_kernel, dim3(2 * pl.b_tiles), dim3(256), 0, s, p);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
