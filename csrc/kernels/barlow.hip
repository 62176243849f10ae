// Barlow Twins loss for gfx950 (--method BarlowTwins): the D x D cross-correlation of the two
// views' batch-standardised embeddings, its loss and gradient, and the backward through the
// standardisation, on v_mfma_f32_16x16x32_bf16 with fp32 operands split into bf16 hi + lo
// (a product is hi·hi + hi·lo + lo·hi, three MFMAs, the lo·lo term dropped; as head_gemm.hip).
// fp32 in, fp32 out.
//
//   bt_colstats   per-column Σz and Σz² of both views (grid.y = view) in fp64: a block owns 64
//                 columns, its 4 waves rows n ≡ w (mod 4) in ascending order, the 4 partials are
//                 added in wave order. Finalised in the same launch to (μ, rstd) when the batch is
//                 on one rank; bt_stats_finalize does it alone after an all-reduce of the sums.
//   bt_gemm       one tile loop, two uses. A workgroup (4 waves, 2 x 2) owns a TM x 128 output
//                 tile, a wave (TM/2) x 64 of it in TM/32 x 4 accumulators. The reduction goes
//                 through LDS in 32-wide chunks (one MFMA k-block), ascending, never split. An
//                 operand is staged as two bf16 images (hi, lo) of 64-byte rows [output index]
//                 [32 reduction steps], 16-byte chunks XOR-swizzled. The next chunk's global loads
//                 are issued before this chunk's MFMAs and stay raw in registers; standardising,
//                 masking and splitting happen when they are committed to LDS.
//                   xcorr  C[i][j] = Σ_n ẑ1[n][i]·ẑ2[n][j] / N, TM = 128. The reduction index (the
//                          batch) is the outer one in memory for both operands: a lane reads 8
//                          batch rows of one column (lanes along the columns, 256 bytes per wave
//                          and row) and writes one 16-byte chunk (kTrans). A staged element is
//                          (z − μ_col)·rstd_col; rows n >= n and columns >= D are staged as zeros
//                          after standardisation (the address is clamped, no load is skipped).
//                   bwd    dz_v[n][d] = rstd_v[d]·(Σ_k ẑ_o[n][k]·B[k][d] / N − ẑ_v[n][d]·r_v[d])·g,
//                          TM = 64, both views in one launch (tile ranges). ẑ_o is staged along its
//                          rows (kRow: two float4 per slot, μ and rstd of the 8 reduction steps
//                          read next to them). B = Gᵀ for view 1 (kRow on G) and G for view 2
//                          (kTrans on G). The epilogue recomputes ẑ_v at the accumulator's
//                          coordinates.
//                 Tile order: xcd_remap puts consecutive logical tiles on one XCD, and logical
//                 tiles walk 4 tile rows down before the next tile column (grouped_walk in
//                 loss_gemm_plan.h), so tiles resident together share operand strips in that XCD's L2.
//                 The loop is Barlow's own, on one LDS buffer with two barriers per chunk; vicreg.hip's
//                 double-buffered loop (mma_tile in loss_gemm.h) is not used here: see
//                 profiles/loss_gemm_share.txt.
//   bt_loss_grad  one pass over C: a block owns 8 rows, a thread 4 adjacent columns of every
//                 1024. G overwrites C; r1 = row sums of G⊙C / N, complete in the block (lane
//                 butterfly, then the 4 waves in order); the block's column sums of G⊙C (8 rows,
//                 row order, one thread each) and its loss partial (fp64 from the thread partials
//                 on) go to per-block slots. bt_loss_finish adds the slots in block order in fp64:
//                 r2 and the loss, a device scalar.
//
// Determinism: no atomics, no split reduction; every sum's order is a function of (n, D).
#include "barlow_plan.h"
#include "common.h"
#include "launchers.h"
#include "loss_gemm.h"

using namespace sdx;

namespace {

namespace bp = sdx_barlow;
using namespace sdx_stage;   // Operand, Stager, sw_off, add_row_groups: shared with vicreg.hip

constexpr int KC = bp::kChunk;
constexpr int TN = bp::kTile;
constexpr int ROW_B = kStageRowB;   // bytes of one staged bf16 row

struct ViewParams {
  Operand a, b;
  const float* z;      // bwd epilogue: this view's z, μ, rstd, r
  const float* mu;
  const float* rstd;
  const float* r;
  float* out;
};

struct GemmParams {
  ViewParams v[2];
  int M, N, chunks, tiles_m, tiles_n, tiles;
  float n_total;
  const float* g;
};

enum Epilogue { kXcorr = 0, kBwd = 1 };

// TM x 128 output tile (tm, tn) of view vp: acc[t][u][r] = Σ_k a[m0 + wm·TM/2 + 16t + 4h + r][k] ·
// b[n0 + 64·wn + 16u + c][k]
template <int TM, int MA, bool STDA, int MB, bool STDB, int EPI>
__device__ __forceinline__ void gemm_tile(const GemmParams& p, const ViewParams& vp, int tm, int tn,
                                          unsigned char* stage) {
  constexpr int MT = TM / 32;
  unsigned char* a_hi = stage;
  unsigned char* a_lo = a_hi + TM * ROW_B;
  unsigned char* b_hi = a_lo + TM * ROW_B;
  unsigned char* b_lo = b_hi + TN * ROW_B;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  const int h = lane >> 4;   // 16-lane group: reduction sub-block of the fragments, row group of the accumulator
  const int c = lane & 15;   // fragment row / accumulator column
  const int m0 = tm * TM, n0 = tn * TN;

  Stager<MA, STDA, TM> sa;
  Stager<MB, STDB, TN> sb;
  sa.init(vp.a, m0, tid);
  sb.init(vp.b, n0, tid);
  sa.load(vp.a, 0);
  sb.load(vp.b, 0);

  f32x4 acc[MT][4];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kc = 0; kc < p.chunks; ++kc) {
    sa.commit(vp.a, kc * KC, a_hi, a_lo);
    sb.commit(vp.b, kc * KC, b_hi, b_lo);
    __syncthreads();
    if (kc + 1 < p.chunks) {   // the next chunk's loads fly under this chunk's MFMAs
      sa.load(vp.a, (kc + 1) * KC);
      sb.load(vp.b, (kc + 1) * KC);
    }
    bf16x8 o_hi[4], o_lo[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int boff = sw_off(wn * 64 + 16 * u + c, h);
      o_hi[u] = *reinterpret_cast<const bf16x8*>(b_hi + boff);
      o_lo[u] = *reinterpret_cast<const bf16x8*>(b_lo + boff);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int aoff = sw_off(wm * (TM / 2) + 16 * t + c, h);
      const bf16x8 f_hi = *reinterpret_cast<const bf16x8*>(a_hi + aoff);
      const bf16x8 f_lo = *reinterpret_cast<const bf16x8*>(a_lo + aoff);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f_hi, o_hi[u], acc[t][u], 0, 0, 0);
        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f_hi, o_lo[u], acc[t][u], 0, 0, 0);
        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f_lo, o_hi[u], acc[t][u], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  const float nt = p.n_total;
  float go = 1.f;
  if constexpr (EPI == kBwd) go = p.g[0];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int n = n0 + wn * 64 + 16 * u + c;
    if (n >= p.N) continue;
    float mu = 0.f, rs = 0.f, rr = 0.f;
    if constexpr (EPI == kBwd) {
      mu = vp.mu[n];
      rs = vp.rstd[n];
      rr = vp.r[n];
    }
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * (TM / 2) + 16 * t + 4 * h + r;
        if (m >= p.M) continue;
        const size_t e = (size_t)m * p.N + n;
        SDX_DCHECK(e < (size_t)p.M * p.N);
        const float v = acc[t][u][r] / nt;
        if constexpr (EPI == kXcorr) {
          vp.out[e] = v;
        } else {
          const float zh = (vp.z[e] - mu) * rs;
          vp.out[e] = rs * (v - zh * rr) * go;
        }
      }
  }
}

// logical tile -> (tm, tn): grouped_walk (loss_gemm_plan.h) behind the XCD remap
__device__ __forceinline__ void tile_coords(const GemmParams& p, int bid, int* tm, int* tn) {
  const bp::TilePos tp = bp::grouped_walk(xcd_remap(bid, p.tiles), p.tiles_m, p.tiles_n, bp::kGroup);
  *tm = tp.row;
  *tn = tp.col;
  SDX_DCHECK(*tm < p.tiles_m && *tn < p.tiles_n);
}

__global__ __launch_bounds__(256) void bt_xcorr_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[2 * (bp::kTileMX + TN) * ROW_B];
  int tm, tn;
  tile_coords(p, blockIdx.x, &tm, &tn);
  gemm_tile<bp::kTileMX, kTrans, true, kTrans, true, kXcorr>(p, p.v[0], tm, tn, stage);
}

__global__ __launch_bounds__(256) void bt_bwd_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[2 * (bp::kTileMB + TN) * ROW_B];
  const int view = (int)blockIdx.x >= p.tiles ? 1 : 0;
  int tm, tn;
  tile_coords(p, (int)blockIdx.x - view * p.tiles, &tm, &tn);
  if (view == 0)   // dz1 = ẑ2·Gᵀ: B[d][k] = G[d][k], the reduction along G's rows
    gemm_tile<bp::kTileMB, kRow, true, kRow, false, kBwd>(p, p.v[0], tm, tn, stage);
  else             // dz2 = ẑ1·G: B[d][k] = G[k][d], G transposed on the way in
    gemm_tile<bp::kTileMB, kRow, true, kTrans, false, kBwd>(p, p.v[1], tm, tn, stage);
}

// ---- statistics, loss ------------------------------------------------------------------------

__device__ __forceinline__ void finalize_col(double s, double q, double n_total, float eps, float* mu, float* rstd) {
  const double mean = s / n_total;
  double var = q / n_total - mean * mean;
  var = var > 0.0 ? var : 0.0;
  *mu = (float)mean;
  *rstd = (float)(1.0 / sqrt(var + (double)eps));
}

__global__ __launch_bounds__(256) void bt_colstats_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                          int n, int D, double* __restrict__ sums,
                                                          float* __restrict__ stats, double n_total, float eps) {
  const int view = blockIdx.y;
  const float* z = view ? z2 : z1;
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int col = blockIdx.x * bp::kStatCols + cl;
  double s = 0.0, q = 0.0;
#pragma unroll 8
  for (int i = rg; i < n; i += 4) {
    const double x = (double)z[(size_t)i * D + col];
    s += x;
    q += x * x;
  }
  double sq[2] = {s, q};
  if (add_row_groups(sq)) {
    sums[(size_t)(view * 2 + 0) * D + col] = sq[0];
    sums[(size_t)(view * 2 + 1) * D + col] = sq[1];
    if (stats != nullptr)
      finalize_col(sq[0], sq[1], n_total, eps, stats + (size_t)(view * 2 + 0) * D + col,
                   stats + (size_t)(view * 2 + 1) * D + col);
  }
}

__global__ __launch_bounds__(256) void bt_stats_finalize_kernel(const double* __restrict__ sums, int D,
                                                                double n_total, float eps,
                                                                float* __restrict__ stats) {
  const int e = blockIdx.x * 256 + threadIdx.x;   // (view, column)
  if (e >= 2 * D) return;
  const int view = e / D, col = e - view * D;
  finalize_col(sums[(size_t)(view * 2 + 0) * D + col], sums[(size_t)(view * 2 + 1) * D + col], n_total, eps,
               stats + (size_t)(view * 2 + 0) * D + col, stats + (size_t)(view * 2 + 1) * D + col);
}

__global__ __launch_bounds__(256) void bt_loss_grad_kernel(float* __restrict__ C, int D, float lam, float n_total,
                                                           float* __restrict__ r1, float* __restrict__ r2_part,
                                                           double* __restrict__ loss_part) {
  constexpr int RB = bp::kLossRows;
  __shared__ float row_part[4][RB];
  __shared__ double loss_w[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int i0 = blockIdx.x * RB;
  const float two_lam = 2.f * lam;
  float rs[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) rs[r] = 0.f;
  float ls = 0.f;
  for (int j0 = tid * 4; j0 < D; j0 += 1024) {
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int i = i0 + r;
      float4* pc = reinterpret_cast<float4*>(C + (size_t)i * D + j0);
      const float4 c4 = *pc;
      const float x[4] = {c4.x, c4.y, c4.z, c4.w};
      float g[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool diag = i == j0 + e;
        const float d = x[e] - 1.f;
        g[e] = diag ? 2.f * d : two_lam * x[e];
        const float t = diag ? d * d : lam * (x[e] * x[e]);
        const float gc = g[e] * x[e];
        rs[r] += gc;
        cs[e] += gc;
        ls += t;
      }
      *pc = make_float4(g[0], g[1], g[2], g[3]);
    }
    *reinterpret_cast<float4*>(r2_part + (size_t)blockIdx.x * D + j0) = make_float4(cs[0], cs[1], cs[2], cs[3]);
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const float v = wave_sum(rs[r]);
    if (lane == 0) row_part[wv][r] = v;
  }
  const double lw = wave_sum_f64((double)ls);
  if (lane == 0) loss_w[wv] = lw;
  __syncthreads();
  if (tid < RB) r1[i0 + tid] = (((row_part[0][tid] + row_part[1][tid]) + row_part[2][tid]) + row_part[3][tid]) / n_total;
  if (tid == 0) loss_part[blockIdx.x] = ((loss_w[0] + loss_w[1]) + loss_w[2]) + loss_w[3];
}

// blocks [0, gridDim.x − 1): r2 of 256 columns each, the slots added in block order; the last
// block: the loss
__global__ __launch_bounds__(256) void bt_loss_finish_kernel(const float* __restrict__ r2_part,
                                                             const double* __restrict__ loss_part, int D, int nblk,
                                                             double n_total, float* __restrict__ r2,
                                                             float* __restrict__ loss) {
  if (blockIdx.x + 1 == gridDim.x) {
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int b = 0; b < nblk; ++b) s += loss_part[b];
      loss[0] = (float)s;
    }
    return;
  }
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= D) return;
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < nblk; ++b) s += (double)r2_part[(size_t)b * D + j];
  r2[j] = (float)(s / n_total);
}

}  // namespace

bool barlow_supported(long n, long D) { return bp::supported(n, D); }

hipError_t launch_bt_colstats(const float* z1, const float* z2, int n, int D, double* sums, float* stats,
                              double n_total, float eps, hipStream_t s) {
  bp::Plan pl;
  if (!bp::make_plan(n, D, &pl) || z1 == nullptr || z2 == nullptr || sums == nullptr) return hipErrorInvalidValue;
  if (!(n_total >= n) || !(eps >= 0.f)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bt_colstats_kernel, dim3(pl.stat_blocks, 2), dim3(256), 0, s, z1, z2, n, D, sums, stats, n_total,
                     eps);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_bt_stats_finalize(const double* sums, int D, double n_total, float eps, float* stats,
                                    hipStream_t s) {
  if (!bp::supported(1, D) || sums == nullptr || stats == nullptr || !(n_total >= 1) || !(eps >= 0.f))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(bt_stats_finalize_kernel, dim3((2 * D + 255) / 256), dim3(256), 0, s, sums, D, n_total, eps,
                     stats);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_bt_xcorr(const float* z1, const float* z2, const float* stats, int n, int D, double n_total,
                           float* C, hipStream_t s) {
  bp::Plan pl;
  if (!bp::make_plan(n, D, &pl) || z1 == nullptr || z2 == nullptr || stats == nullptr || C == nullptr)
    return hipErrorInvalidValue;
  if (!(n_total >= n)) return hipErrorInvalidValue;
  GemmParams p = {};
  // element (i = column of z, r = batch row) at z[r·D + i]
  p.v[0].a = operand(z1, D, n, 1, D, stats, stats + D);
  p.v[0].b = operand(z2, D, n, 1, D, stats + 2 * (size_t)D, stats + 3 * (size_t)D);
  p.v[0].out = C;
  p.M = D; p.N = D; p.chunks = pl.x_chunks;
  p.tiles_m = pl.x_tiles_m; p.tiles_n = pl.x_tiles_n; p.tiles = pl.x_tiles;
  p.n_total = (float)n_total;
  hipLaunchKernelGGL(bt_xcorr_kernel, dim3(pl.x_tiles), dim3(256), 0, s, p);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_bt_loss_grad(float* C, int D, float lam, double n_total, float* r, float* loss, float* r2_part,
                               double* loss_part, hipStream_t s) {
  bp::Plan pl;
  if (!bp::make_plan(1, D, &pl) || C == nullptr || r == nullptr || loss == nullptr || r2_part == nullptr ||
      loss_part == nullptr)
    return hipErrorInvalidValue;
  if (!bp::aligned16(C) || !bp::aligned16(r2_part) || !(n_total >= 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bt_loss_grad_kernel, dim3(pl.loss_blocks), dim3(256), 0, s, C, D, lam, (float)n_total, r, r2_part,
                     loss_part);
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(bt_loss_finish_kernel, dim3(pl.finish_blocks), dim3(256), 0, s, (const float*)r2_part,
                     (const double*)loss_part, D, pl.loss_blocks, n_total, r + D, loss);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_bt_bwd(const float* z1, const float* z2, const float* G, const float* stats, const float* r,
                         const float* g, int n, int D, double n_total, float* dz1, float* dz2, hipStream_t s) {
  bp::Plan pl;
  if (!bp::make_plan(n, D, &pl) || z1 == nullptr || z2 == nullptr || G == nullptr || stats == nullptr ||
      r == nullptr || g == nullptr || dz1 == nullptr || dz2 == nullptr)
    return hipErrorInvalidValue;
  if (!bp::aligned16(z1) || !bp::aligned16(z2) || !bp::aligned16(G) || !bp::aligned16(stats) || !(n_total >= n))
    return hipErrorInvalidValue;
  const float* mu1 = stats;
  const float* rs1 = stats + D;
  const float* mu2 = stats + 2 * (size_t)D;
  const float* rs2 = stats + 3 * (size_t)D;
  GemmParams p = {};
  // view 1: A = ẑ2 [n][k], B[d][k] = G[d][k]
  p.v[0].a = operand(z2, n, D, D, 1, mu2, rs2);
  p.v[0].b = operand(G, D, D, D, 1);
  p.v[0].z = z1; p.v[0].mu = mu1; p.v[0].rstd = rs1; p.v[0].r = r; p.v[0].out = dz1;
  // view 2: A = ẑ1 [n][k], B[d][k] = G[k][d]
  p.v[1].a = operand(z1, n, D, D, 1, mu1, rs1);
  p.v[1].b = operand(G, D, D, 1, D);
  p.v[1].z = z2; p.v[1].mu = mu2; p.v[1].rstd = rs2; p.v[1].r = r + D; p.v[1].out = dz2;
  p.M = n; p.N = D; p.chunks = pl.b_chunks;
  p.tiles_m = pl.b_tiles_m; p.tiles_n = pl.b_tiles_n; p.tiles = pl.b_tiles;
  p.n_total = (float)n_total;
  p.g = g;
  hipLaunchKernelGGL(bt_bwd_kernel, dim3(2 * pl.b_tiles), dim3(256), 0, s, p);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
