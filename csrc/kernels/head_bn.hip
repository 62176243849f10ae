// BatchNorm projector head (Linear -> BatchNorm1d -> ReLU hidden layers of the Barlow Twins /
// VICReg projectors): two column-strip-owned kernels, one launch per hidden layer and direction.
//
// The head's GEMMs have few rows (both views of the local batch, N <= 2048) and many columns, and
// BatchNorm1d reduces over exactly those rows. A workgroup that owns ALL rows of a narrow strip of
// output columns therefore holds every value a column's statistics need in its own accumulators:
//
//   hbn_fwd   yb = bf16(x·Wᵀ)                      MFMA, fp32 accumulation
//             μ = Σ yb / N, σ² = Σ (yb − μ)² / N   from the rounded accumulators, fixed order
//             a = bf16(relu(γ·(yb − μ)·rstd + β))  in registers; yb, a, μ, rstd and the running
//                                                  statistics stored by the same launch
//   hbn_bwd   dŷ = da·[γ·x̂ + β > 0], x̂ = (yb − μ)·rstd   recomputed from yb (hbn_affine: the same
//                                                  fp32 expression as the forward, so the mask agrees)
//             dβ = Σ dŷ, dγ = Σ dŷ·x̂               added into the gradient sinks
//             dy = γ·rstd·(dŷ − dβ/N − x̂·dγ/N)     from the registers the sums were taken from
//
// No statistics slab, no reduction launch, no apply pass, no atomics: every sum runs in-lane over
// the rows, then over the 16 lanes of a DPP row, then over the waves through LDS, in one order.
//
// hbn_fwd data movement. D = W_strip · xᵀ: the MFMA's M index is the output column, its N index
// the row, so a lane of the 16x16 accumulator holds 4 consecutive columns of ONE row and (32-wide
// strips: two column blocks interleaved in fours) stores 8 columns = 16 bytes of yb and a. The
// strip of W is what the waves share: it streams through LDS in chunks of 64 reduction elements,
// double-buffered, one barrier per chunk, 16-byte cells XOR-swizzled by row so that the 16 rows a
// fragment read touches sit on distinct banks. x is NOT shared (a row fragment belongs to one
// wave), so its operands go from global memory straight into the MFMA's B registers, 16 bytes per
// lane, one k-step ahead of the products; at N = 2048 a chunk of x would not fit in LDS twice.
#include "common.h"
#include "head_bn_plan.h"
#include "launchers.h"

using namespace sdx;
using namespace sdx_hbn;

namespace {

// x̂ and the BN output before the ReLU, the one definition both directions use
__device__ __forceinline__ float hbn_xhat(float y, float mu, float rstd) { return (y - mu) * rstd; }
__device__ __forceinline__ float hbn_affine(float g, float xh, float b) { return __fmaf_rn(g, xh, b); }

__device__ __forceinline__ float round_bf(float v) { return bf2f(f2bf(v)); }

template <int SW, int FR>
__global__ __launch_bounds__(kThreads) void hbn_fwd_kernel(const HbnFwdArgs p) {
  constexpr int NB = SW / 16;          // 16-column MFMA blocks of the strip
  constexpr int ROW_B = kChunk * 2;    // bytes of one W row of a chunk
  __shared__ __attribute__((aligned(16))) unsigned char wlds[2][SW * ROW_B];
  __shared__ float red[kWaves][SW];
  __shared__ float col_s[2][SW];       // μ, rstd of the strip

  const int t = threadIdx.x, wave = t >> 6, l = t & 63, n = l & 15, g = l >> 4;
  const int N = p.N, K = p.K, H = p.H;
  const int col0 = blockIdx.x * SW;
  const unsigned char* xg = reinterpret_cast<const unsigned char*>(p.x);

  // W staging: thread t < SW·8 moves 16-byte cell (t & 7) of strip row t >> 3 (whole waves)
  const bool stager = t < SW * 8;
  const int wr = t >> 3, wch = t & 7;
  const uint16_t* wsrc = p.w + (size_t)(col0 + (stager ? wr : 0)) * K + wch * 8;
  const int wdst = wr * ROW_B + ((wch ^ (wr & 7)) << 4);
  // A fragment: accumulator row m = this lane's n; block b's row m is strip column
  // 8·(m / 4) + 4·b + m % 4 (32-wide) so that lane group g ends up with columns 8g .. 8g + 7
  int arow[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) arow[b] = NB == 2 ? 8 * (n >> 2) + 4 * b + (n & 3) : n;

  // fragment j of this wave: rows 16·(j·kWaves + wave) ..; tail rows read row N − 1 instead
  uint32_t xoff[FR];
  bool live[FR];
#pragma unroll
  for (int j = 0; j < FR; ++j) {
    const int r0 = 16 * (j * kWaves + wave);
    live[j] = r0 < N;
    const int r = r0 + n < N ? r0 + n : N - 1;
    xoff[j] = ((uint32_t)r * (uint32_t)K + 8u * g) * 2u;
  }
  auto load_x = [&](int step, bf16x8 (&xf)[FR]) {
#pragma unroll
    for (int j = 0; j < FR; ++j)
      if (live[j]) xf[j] = *reinterpret_cast<const bf16x8*>(xg + xoff[j] + (uint32_t)step * 64u);
  };

  f32x4 acc[FR][NB];
  bf16x8 xa[FR], xb[FR];
#pragma unroll
  for (int j = 0; j < FR; ++j) {
    xa[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    xb[j] = xa[j];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[j][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto products = [&](const unsigned char* wb, int ks, const bf16x8 (&xf)[FR]) {
    bf16x8 af[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
      af[b] = *reinterpret_cast<const bf16x8*>(wb + arow[b] * ROW_B + (((ks * 4 + g) ^ (arow[b] & 7)) << 4));
#pragma unroll
    for (int j = 0; j < FR; ++j)
      if (live[j]) {
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[j][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[b], xf[j], acc[j][b], 0, 0, 0);
      }
  };

  const int chunks = K / kChunk;
  load_x(0, xa);
  if (stager) *reinterpret_cast<uint4*>(wlds[0] + wdst) = *reinterpret_cast<const uint4*>(wsrc);
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    const bool more = c + 1 < chunks;
    uint4 wreg = make_uint4(0, 0, 0, 0);
    if (more && stager) wreg = *reinterpret_cast<const uint4*>(wsrc + (size_t)(c + 1) * kChunk);
    const unsigned char* wb = wlds[c & 1];
    load_x(2 * c + 1, xb);
    products(wb, 0, xa);
    if (more) load_x(2 * c + 2, xa);
    products(wb, 1, xb);
    // the other buffer: every wave left it at the previous barrier
    if (more && stager) *reinterpret_cast<uint4*>(wlds[(c + 1) & 1] + wdst) = wreg;
    __syncthreads();
  }

  // ---- the strip's whole pre-activation is in acc: round, statistics, normalise, store ----
  bool rowok[FR];
#pragma unroll
  for (int j = 0; j < FR; ++j) {
    rowok[j] = 16 * (j * kWaves + wave) + n < N;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[j][b][i] = round_bf(acc[j][b][i]);
  }
  auto colidx = [&](int b, int i) { return NB == 2 ? 8 * g + 4 * b + i : 4 * g + i; };
  // Σ over this wave's rows of f(value), per column of the lane -> red[wave][column]
  auto wave_cols = [&](auto f) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < FR; ++j) s += rowok[j] ? f(acc[j][b][i], b, i) : 0.f;
        s = row16_sum(s);
        if (n == 0) red[wave][colidx(b, i)] = s;
      }
  };
  auto strip_total = [&]() {
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) tot += red[w][t];
    return tot;
  };
  const float fn = (float)N;
  wave_cols([](float y, int, int) { return y; });
  __syncthreads();
  if (t < SW) col_s[0][t] = strip_total() / fn;
  __syncthreads();
  float mu[NB][4], rs[NB][4];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) mu[b][i] = col_s[0][colidx(b, i)];
  wave_cols([&](float y, int b, int i) {
    const float d = y - mu[b][i];
    return d * d;
  });
  __syncthreads();
  if (t < SW) {
    const float var = strip_total() / fn;
    const float m = col_s[0][t], rstd = 1.0f / sqrtf(var + p.eps);
    col_s[1][t] = rstd;
    p.mu[col0 + t] = m;
    p.rstd[col0 + t] = rstd;
    const float mom = p.momentum;
    p.rmean[col0 + t] = (1.0f - mom) * p.rmean[col0 + t] + mom * m;
    p.rvar[col0 + t] = (1.0f - mom) * p.rvar[col0 + t] + mom * (var * (fn / (fn - 1.0f)));
  }
  __syncthreads();
  float ga[NB][4], be[NB][4];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rs[b][i] = col_s[1][colidx(b, i)];
      ga[b][i] = p.gamma[col0 + colidx(b, i)];
      be[b][i] = p.beta[col0 + colidx(b, i)];
    }
#pragma unroll
  for (int j = 0; j < FR; ++j) {
    if (!rowok[j]) continue;
    const size_t o = (size_t)(16 * (j * kWaves + wave) + n) * H + col0 + (NB == 2 ? 8 : 4) * g;
    uint32_t yw[NB * 2], aw[NB * 2];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float av[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        av[i] = fmaxf(hbn_affine(ga[b][i], hbn_xhat(acc[j][b][i], mu[b][i], rs[b][i]), be[b][i]), 0.f);
      yw[2 * b] = pack_bf2(acc[j][b][0], acc[j][b][1]);
      yw[2 * b + 1] = pack_bf2(acc[j][b][2], acc[j][b][3]);
      aw[2 * b] = pack_bf2(av[0], av[1]);
      aw[2 * b + 1] = pack_bf2(av[2], av[3]);
    }
    if constexpr (NB == 2) {
      *reinterpret_cast<uint4*>(p.yb + o) = make_uint4(yw[0], yw[1], yw[2], yw[3]);
      *reinterpret_cast<uint4*>(p.a + o) = make_uint4(aw[0], aw[1], aw[2], aw[3]);
    } else {   // a 16-wide strip gives a lane 4 columns: 8-byte stores
      *reinterpret_cast<uint2*>(p.yb + o) = make_uint2(yw[0], yw[1]);
      *reinterpret_cast<uint2*>(p.a + o) = make_uint2(aw[0], aw[1]);
    }
  }
}

// Thread (wave w, lane l): 8 columns (half = l >> 5) of rows j·256 + 32·w + (l & 31), so the 16
// lanes of a DPP row hold the same columns of 16 consecutive rows.
template <int RPT>
__global__ __launch_bounds__(kThreads) void hbn_bwd_kernel(const HbnBwdArgs p) {
  __shared__ float red[2][kWaves][2][kBwdStrip];
  __shared__ float tot_s[2][kBwdStrip];
  const int t = threadIdx.x, wave = t >> 6, l = t & 63, half = l >> 5;
  const int N = p.N, H = p.H;
  const int col = blockIdx.x * kBwdStrip + half * 8;
  float ga[8], be[8], mu[8], rs[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ga[i] = p.gamma[col + i];
    be[i] = p.beta[col + i];
    mu[i] = p.mu[col + i];
    rs[i] = p.rstd[col + i];
  }
  uint4 dv[RPT], yv[RPT];
  bool ok[RPT];
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int row = j * kBwdRowsPass + wave * 32 + (l & 31);
    ok[j] = row < N;
    dv[j] = yv[j] = make_uint4(0, 0, 0, 0);
    if (ok[j]) {
      const size_t o = (size_t)row * H + col;
      dv[j] = *reinterpret_cast<const uint4*>(p.da + o);
      yv[j] = *reinterpret_cast<const uint4*>(p.yb + o);
    }
  }
  // x̂, the BN output v and dŷ = da·[v > 0] of row j's 8 columns, from the packed registers
  auto row_terms = [&](int j, float (&xh)[8], float (&v)[8], float (&dh)[8]) {
    float d[8], y[8];
    unpack8(dv[j], d);
    unpack8(yv[j], y);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      xh[i] = hbn_xhat(y[i], mu[i], rs[i]);
      v[i] = hbn_affine(ga[i], xh[i], be[i]);
      dh[i] = v[i] > 0.f ? d[i] : 0.f;
    }
  };
  float sb[8], sg[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) sb[i] = sg[i] = 0.f;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {   // rows past N hold da = 0
    float xh[8], v[8], dh[8];
    row_terms(j, xh, v, dh);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sb[i] += dh[i];
      sg[i] += dh[i] * xh[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float b = row16_sum(sb[i]), gsum = row16_sum(sg[i]);
    if ((l & 15) == 0) {
      red[0][wave][(l >> 4) & 1][half * 8 + i] = b;
      red[1][wave][(l >> 4) & 1][half * 8 + i] = gsum;
    }
  }
  __syncthreads();
  if (t < 2 * kBwdStrip) {
    const int which = t >> 4, c = t & 15;
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) tot += red[which][w][0][c] + red[which][w][1][c];
    tot_s[which][c] = tot;
    float* sink = which ? p.sink_gamma : p.sink_beta;   // one writer per column
    sink[blockIdx.x * kBwdStrip + c] += tot;
  }
  __syncthreads();
  const float inv_n = 1.0f / (float)N;
  float mb[8], mg[8], sc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    mb[i] = tot_s[0][half * 8 + i] * inv_n;
    mg[i] = tot_s[1][half * 8 + i] * inv_n;
    sc[i] = ga[i] * rs[i];
  }
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    if (!ok[j]) continue;
    float xh[8], v[8], dh[8], out[8];
    row_terms(j, xh, v, dh);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = sc[i] * (dh[i] - mb[i] - xh[i] * mg[i]);
    const size_t o = (size_t)(j * kBwdRowsPass + wave * 32 + (l & 31)) * H + col;
    *reinterpret_cast<uint4*>(p.dy + o) = pack8(out);
    if (p.a_out != nullptr) {   // the layer's activation, recomputed for the next layer's weight gradient
#pragma unroll
      for (int i = 0; i < 8; ++i) out[i] = fmaxf(v[i], 0.f);
      *reinterpret_cast<uint4*>(p.a_out + o) = pack8(out);
    }
  }
}

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

template <int SW, int FR>
hipError_t fwd_go(const HbnFwdArgs& a, int strips, hipStream_t s) {
  hipLaunchKernelGGL((hbn_fwd_kernel<SW, FR>), dim3(strips), dim3(kThreads), 0, s, a);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

template <int RPT>
hipError_t bwd_go(const HbnBwdArgs& a, int strips, hipStream_t s) {
  hipLaunchKernelGGL((hbn_bwd_kernel<RPT>), dim3(strips), dim3(kThreads), 0, s, a);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

}  // namespace

hipError_t launch_hbn_fwd(const HbnFwdArgs& a, int strip, hipStream_t s) {
  FwdPlan pl;
  if (!make_fwd(a.N, a.K, a.H, strip, &pl)) return hipErrorInvalidValue;
  if (!(al16(a.x) && al16(a.w) && al16(a.yb) && al16(a.a))) return hipErrorInvalidValue;
  if (pl.strip == 32) {
    switch (pl.frags) {
      case 1: return fwd_go<32, 1>(a, pl.strips, s);
      case 2: return fwd_go<32, 2>(a, pl.strips, s);
      case 4: return fwd_go<32, 4>(a, pl.strips, s);
      case 8: return fwd_go<32, 8>(a, pl.strips, s);
    }
    return hipErrorInvalidValue;
  }
  switch (pl.frags) {
    case 1: return fwd_go<16, 1>(a, pl.strips, s);
    case 2: return fwd_go<16, 2>(a, pl.strips, s);
    case 4: return fwd_go<16, 4>(a, pl.strips, s);
    case 8: return fwd_go<16, 8>(a, pl.strips, s);
    case 16: return fwd_go<16, 16>(a, pl.strips, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_hbn_bwd(const HbnBwdArgs& a, hipStream_t s) {
  BwdPlan pl;
  if (!make_bwd(a.N, a.H, &pl)) return hipErrorInvalidValue;
  if (!(al16(a.da) && al16(a.yb) && al16(a.dy) && al16(a.a_out))) return hipErrorInvalidValue;
  switch (pl.rows_per_thread) {
    case 1: return bwd_go<1>(a, pl.strips, s);
    case 2: return bwd_go<2>(a, pl.strips, s);
    case 4: return bwd_go<4>(a, pl.strips, s);
    case 8: return bwd_go<8>(a, pl.strips, s);
  }
  return hipErrorInvalidValue;
}
