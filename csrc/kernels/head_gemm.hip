// MFMA classifier head for gfx950: the three GEMMs of a linear classifier trained with
// cross-entropy (logits, feature gradient, weight gradient) on v_mfma_f32_16x16x32_bf16 with
// fp32 operands split into bf16 hi + lo pairs, for the linear probe, the probe sweep and the
// supervised CE head (--head_gemm mfma). Any K = 64·j <= 4096 and any C <= 32768.
//
//   head_gemm   one template, three operand forms (head_gemm_plan.h):
//                 NT  Z[B][G·C]  = X[B][K]·W[G·C][K]ᵀ + bias     -> logits [G][B][C]
//                 NN  dX[B][K]   = gout·dZ[B][C]·W[C][K]
//                 TN  Gw[G·C][K] = dZ[G][B][C]ᵀ·X[B][K]          -> dW += gout·Gw   (CE head)
//                                                                 -> SGD update in place (probe)
//               A workgroup (4 waves) owns one 64 x 64 output tile; wave w holds output columns
//               16w..16w+15 of all 64 rows (4 accumulators). The reduction goes through LDS in
//               64-wide chunks, ascending, never split. While it is staged every fp32 element x
//               becomes hi = RNE_bf16(x), lo = RNE_bf16(x − hi) in two bf16 images of 128-byte
//               rows (XOR-swizzled 16-byte chunks, as knn.hip); a product is hi·hi + hi·lo +
//               lo·hi, three MFMAs, the lo·lo term dropped. Operands whose reduction index is
//               the outer one in memory (W in NN, dZ and X in TN) are transposed on the way in:
//               a lane reads 8 reduction steps of one output index (lanes along the contiguous
//               index) and writes one 16-byte chunk. Rows, columns and reduction tails out of
//               range are staged as zeros: the load address is clamped into the tensor and the
//               value replaced, no load is skipped. The next chunk's loads fly under the MFMAs.
//               The TN launch carries role blocks after its tiles: one thread per bias column
//               (Σ_b dz in row order, then db += gout·Σ or the SGD update), the last of them also
//               the row statistics, summed in row order in fp64.
//   ce_rows     one wave per logits row (the G·B rows of [G][B][C]): row softmax from global
//               memory for any C, dz = (softmax − onehot)·gscale, rowstat = (lse − z_label,
//               hit@1, hit@5) with the rank rule #{z_c > z_label} < k; NaN loss and no hits for
//               a label out of range.
//   head_stats  the statistics role alone (evaluation, a forward that no backward follows).
//   row map     the row-indexed probe / sweep step (RowMap, launchers' `rows`): x is a feature bank
//               and batch row b its row rows[b]. The NT launch indirects the A operand's output
//               index when the stager fixes its row bases, the TN launch the kTrans operand's
//               reduction index (8 wave-uniform index reads per slot in front of the 8 dword
//               loads), ce_rows reads labels[rows[b]]. Same tiles, chunks and sums: bit-identical
//               to the plain step on x[rows], labels[rows]; no launch and no copy is added.
//
// Launches: training step NT + ce_rows + TN = 3 for any G; evaluation NT + ce_rows + head_stats
// = 3; CE head forward NT + ce_rows = 2 (+ head_stats when no backward follows), backward
// NN + TN = 2.
//
// Determinism: no atomics, no split reduction; an output element is accumulated chunk by chunk
// in the same order wherever it sits in its tile, and nothing depends on G or on the grid, so
// results are bit-identical from run to run and head g of a sweep is bit-identical to a
// single-head step with that head's lr and wd.
#include <limits.h>

#include "common.h"
#include "distill_ce.h"
#include "head_gemm_plan.h"
#include "launchers.h"
#include "soft_ce.h"

using namespace sdx;

namespace {

namespace hg = sdx_headgemm;

constexpr int T = hg::kTile;
constexpr int KC = hg::kChunk;
constexpr int ROW_B = KC * 2;        // bytes of one staged bf16 row
constexpr int IMG_B = T * ROW_B;     // one 64-row bf16 image (8 KiB)

enum LoadMode {
  kVec = 0,        // reduction contiguous and 16-byte aligned rows: two float4 per slot
  kRowScalar = 1,  // reduction contiguous, any row stride: 8 dword loads per slot
  kTrans = 2,      // output index contiguous, reduction strided: 8 dword loads, lanes along the rows
};
enum Epilogue { kLogits = 0, kDx = 1, kDw = 2, kSgd = 3 };
// the row-indexed step: x is a feature bank and batch row b is its row rows[b]
enum RowMapUse {
  kMapNone = 0,
  kMapOut = 1,   // the operand's output index goes through the map (x as A of the NT logits GEMM)
  kMapRed = 2,   // its reduction index does (x as the kTrans operand of the TN weight-gradient GEMM)
};

// element (i, r) — i the output index of this operand, r the reduction index — lives at
// p[(i / hc)·hs + (i % hc)·si + r·sr]; hc = INT_MAX: no heads
struct Operand {
  const float* p;
  int lim_i, lim_r, hc;
  long hs, si, sr;
};

// batch row -> bank row (common.h bank_row). Every head_gemm_kernel / ce_rows_kernel instantiation
// takes it as its last / third argument; the plain ones ({nullptr, 0}) never read it
struct RowMap {
  const int64_t* rows;
  long n;   // bank rows
};

struct HeadHyper {
  float lr[hg::kMaxHeads];
  float wd[hg::kMaxHeads];
};

struct GemmParams {
  Operand a, b;
  int M, N, chunks, tiles_n, tiles;
  int G, B, C, K;
  float* out;            // logits / dX / dW
  const float* bias;     // NT
  const float* gout;     // NN, TN-dW: the upstream scalar gradient
  float* W;              // TN-SGD
  float* bufW;
  float* bvec;           // bias (SGD) or db (dW)
  float* bufb;
  HeadHyper hp;
  float mom;
  int first;
  const float* dz;       // role blocks
  const float* rowstat;
  float* stats;
  float* loss;           // CE head only
};

__device__ __forceinline__ int sw_off(int row, int chunk) { return row * ROW_B + ((chunk ^ (row & 7)) << 4); }

// 8 floats -> 8 bf16 hi + 8 bf16 lo, one 16-byte LDS write each (knn.hip commit_one)
__device__ __forceinline__ void commit8(const float (&xs)[8], unsigned char* hi_img, unsigned char* lo_img, int off) {
  uint32_t wh[4], wl[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    wh[j] = pack_bf2(xs[2 * j], xs[2 * j + 1]);
    const float h0 = __uint_as_float(wh[j] << 16), h1 = __uint_as_float(wh[j] & 0xffff0000u);
    wl[j] = pack_bf2(xs[2 * j] - h0, xs[2 * j + 1] - h1);
  }
  *reinterpret_cast<uint4*>(hi_img + off) = make_uint4(wh[0], wh[1], wh[2], wh[3]);
  *reinterpret_cast<uint4*>(lo_img + off) = make_uint4(wl[0], wl[1], wl[2], wl[3]);
}

// A thread stages two (row, 8-element chunk) slots of a 64 x 64 operand tile per step.
template <int MODE, int MAP = kMapNone>
struct Stager {
  const float* base[2];   // clamped row base
  bool ok[2];
  int off[2];             // LDS byte offset of the slot
  int rch[2];             // first reduction element of the slot inside the chunk

  __device__ __forceinline__ void init(const Operand& o, const RowMap& rm, int i0, int tid) {
    static_assert(MAP == kMapNone || (MAP == kMapOut && MODE != kTrans) || (MAP == kMapRed && MODE == kTrans),
                  "x is staged along its rows (NT) or transposed (TN)");
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int row = MODE == kTrans ? (tid & 63) : ps * 32 + (tid >> 3);
      const int chunk = MODE == kTrans ? (tid >> 6) + 4 * ps : (tid & 7);
      const int i = i0 + row;
      ok[ps] = i < o.lim_i;
      const int ic = ok[ps] ? i : o.lim_i - 1;
      if constexpr (MAP == kMapOut) {
        // (x has no heads) the clamped batch row's bank row: out-of-tile rows still load, then zero
        base[ps] = o.p + bank_row(rm.rows, ic, rm.n) * o.si;
      } else {
        const int hd = ic / o.hc;
        base[ps] = o.p + (size_t)hd * o.hs + (size_t)(ic - hd * o.hc) * o.si;
      }
      off[ps] = sw_off(row, chunk);
      rch[ps] = chunk * 8;
    }
  }

  __device__ __forceinline__ void load(const Operand& o, const RowMap& rm, int r0, float (&v)[2][8]) const {
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      if constexpr (MAP == kMapRed) {
        // a wave stages one 8-step chunk of the slot (chunk = wave + 4·ps), so the 8 batch rows
        // and their bank rows are wave-uniform: scalar index loads, then the 8 dword loads
        const int rb = __builtin_amdgcn_readfirstlane(r0 + rch[ps]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = rb + j;
          const bool rok = r < o.lim_r;
          const int rc = rok ? r : o.lim_r - 1;
          const float x = base[ps][bank_row(rm.rows, rc, rm.n) * (size_t)o.sr];
          v[ps][j] = (ok[ps] && rok) ? x : 0.f;
        }
      } else if constexpr (MODE == kVec) {
        // lim_r is a multiple of the chunk: no reduction tail on this path
        const float4* s = reinterpret_cast<const float4*>(base[ps] + r0 + rch[ps]);
        const float4 v0 = s[0], v1 = s[1];
        const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) v[ps][j] = ok[ps] ? x[j] : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = r0 + rch[ps] + j;
          const bool rok = r < o.lim_r;
          const int rc = rok ? r : o.lim_r - 1;
          const float x = base[ps][(size_t)rc * o.sr];
          v[ps][j] = (ok[ps] && rok) ? x : 0.f;
        }
      }
    }
  }
};

// Σ_rows of one bias column (fp32, row order), then its epilogue; the last role block also sums
// the row statistics (fp64, row order). role = index of this role block, n_role their count.
template <int EPI>
__device__ __forceinline__ void role_block(const GemmParams& p, int role, int n_role) {
  const int GC = p.G * p.C;
  if (p.dz != nullptr) {
    const int n = role * hg::kBiasPerBlock + (int)threadIdx.x;
    if (n < GC) {
      const int g = n / p.C, c = n - g * p.C;
      const float* col = p.dz + (size_t)g * p.B * p.C + c;
      float s = 0.f;
      for (int b = 0; b < p.B; ++b) s += col[(size_t)b * p.C];
      if constexpr (EPI == kDw) {
        p.bvec[n] += __fmul_rn(p.gout[0], s);
      } else if constexpr (EPI == kSgd) {
        const float lr = p.hp.lr[g], wd = p.hp.wd[g];
        const float d = s + wd * p.bvec[n];
        p.bufb[n] = p.first ? d : fmaf(p.mom, p.bufb[n], d);
        p.bvec[n] -= lr * p.bufb[n];
      }
    }
  }
  if (role + 1 == n_role && (int)threadIdx.x < 3 * p.G) {
    const int h = threadIdx.x / 3, j = threadIdx.x - 3 * h;
    const float* rs = p.rowstat + (size_t)h * p.B * 3;
    double s = 0.0;
    for (int b = 0; b < p.B; ++b) s += (double)rs[(size_t)b * 3 + j];
    p.stats[threadIdx.x] = (float)s;
    if (p.loss != nullptr && threadIdx.x == 0) p.loss[0] = (float)(s / (double)p.B);
  }
}

// MAPA / MAPB: x read from the bank through rm, as the A operand by output index (NT) or the B
// operand by reduction index (TN); tiles, chunk order and every sum are the same either way
template <int LA, int LB, int EPI, int MAPA = kMapNone, int MAPB = kMapNone>
__global__ __launch_bounds__(256) void head_gemm_kernel(GemmParams p, RowMap rm) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[4 * IMG_B];   // a hi, a lo, b hi, b lo
  const int bid = blockIdx.x;
  if constexpr (EPI == kDw || EPI == kSgd) {
    if (bid >= p.tiles) {
      role_block<EPI>(p, bid - p.tiles, (int)gridDim.x - p.tiles);
      return;
    }
  }
  unsigned char* a_hi = stage;
  unsigned char* a_lo = stage + IMG_B;
  unsigned char* b_hi = stage + 2 * IMG_B;
  unsigned char* b_lo = stage + 3 * IMG_B;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int h = lane >> 4;   // 16-lane group: reduction sub-block of the fragments, row group of the accumulator
  const int c = lane & 15;   // fragment row / accumulator column
  const int tm = bid / p.tiles_n, tn = bid - tm * p.tiles_n;
  const int m0 = tm * T, n0 = tn * T;

  Stager<LA, MAPA> sa;
  Stager<LB, MAPB> sb;
  sa.init(p.a, rm, m0, tid);
  sb.init(p.b, rm, n0, tid);
  float va[2][8], vb[2][8];
  sa.load(p.a, rm, 0, va);
  sb.load(p.b, rm, 0, vb);

  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kc = 0; kc < p.chunks; ++kc) {
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      commit8(va[ps], a_hi, a_lo, sa.off[ps]);
      commit8(vb[ps], b_hi, b_lo, sb.off[ps]);
    }
    __syncthreads();
    if (kc + 1 < p.chunks) {   // the next chunk's loads fly under this chunk's MFMAs
      sa.load(p.a, rm, (kc + 1) * KC, va);
      sb.load(p.b, rm, (kc + 1) * KC, vb);
    }
    // acc[t][r] = Σ_k a[m0 + 16t + 4h + r][k] · b[n0 + 16wv + c][k]
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int boff = sw_off(wv * 16 + c, 4 * s + h);
      const bf16x8 o_hi = *reinterpret_cast<const bf16x8*>(b_hi + boff);
      const bf16x8 o_lo = *reinterpret_cast<const bf16x8*>(b_lo + boff);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int aoff = sw_off(16 * t + c, 4 * s + h);
        const bf16x8 f_hi = *reinterpret_cast<const bf16x8*>(a_hi + aoff);
        const bf16x8 f_lo = *reinterpret_cast<const bf16x8*>(a_lo + aoff);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f_hi, o_hi, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f_hi, o_lo, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f_lo, o_hi, acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  const int n = n0 + wv * 16 + c;
  if (n >= p.N) return;
  float go = 1.f;
  if constexpr (EPI == kDx || EPI == kDw) go = p.gout[0];
  float bn = 0.f;
  int gh = 0, gc = n;
  if constexpr (EPI == kLogits) {
    bn = p.bias[n];
    gh = n / p.C;
    gc = n - gh * p.C;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 16 * t + 4 * h + r;
      if (m >= p.M) continue;
      const float v = acc[t][r];
      if constexpr (EPI == kLogits) {
        SDX_DCHECK(gh < p.G && m < p.B);
        p.out[((size_t)gh * p.B + m) * p.C + gc] = v + bn;
      } else if constexpr (EPI == kDx) {
        p.out[(size_t)m * p.N + n] = __fmul_rn(go, v);
      } else if constexpr (EPI == kDw) {
        // (the product is rounded on its own: the sum into the sink is no fused multiply-add)
        float* d = p.out + (size_t)m * p.N + n;
        *d = *d + __fmul_rn(go, v);
      } else {
        const int g = m / p.C;
        const float lr = p.hp.lr[g], wd = p.hp.wd[g];
        const size_t e = (size_t)m * p.N + n;
        float w = p.W[e], bu = p.bufW[e];
        const float d = v + wd * w;
        bu = p.first ? d : fmaf(p.mom, bu, d);
        w -= lr * bu;
        p.W[e] = w;
        p.bufW[e] = bu;
      }
    }
}

__global__ __launch_bounds__(256) void head_stats_kernel(GemmParams p) { role_block<kLogits>(p, 0, 1); }

// rows = G·B logits rows of C classes; labels [B] shared by the heads, or (MAPPED) the bank's
// labels [rm.n] read at rm.rows[b]
template <bool MAPPED>
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits,
                                                      const int64_t* __restrict__ labels, RowMap rm, int rows, int B,
                                                      int C, float gscale, float* __restrict__ dz,
                                                      float* __restrict__ rowstat) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * hg::kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* z = logits + (size_t)row * C;
  const int64_t lab64 = labels[MAPPED ? bank_row(rm.rows, row % B, rm.n) : (size_t)(row % B)];
  const bool ok = lab64 >= 0 && lab64 < C;
  const int lab = ok ? (int)lab64 : -1;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, z[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(z[c] - m);
  s = wave_sum(s);
  const float lse = m + __logf(s);
  const float zl = ok ? z[lab] : 0.f;
  float above = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = z[c];
    above += v > zl ? 1.f : 0.f;
    if (dz != nullptr) dz[(size_t)row * C + c] = (__expf(v - lse) - (c == lab ? 1.f : 0.f)) * gscale;
  }
  above = wave_sum(above);
  if (lane == 0) {
    rowstat[(size_t)row * 3 + 0] = ok ? lse - zl : NAN;
    rowstat[(size_t)row * 3 + 1] = (ok && above < 1.f) ? 1.f : 0.f;
    rowstat[(size_t)row * 3 + 2] = (ok && above < 5.f) ? 1.f : 0.f;
  }
}

// The SOFT form of ce_rows_kernel<false> for one head (Mixup / CutMix / label smoothing): rows = B
// logits rows, two labels per row and the target weights of soft_ce.h; the logits stay where the
// GEMM wrote them
__global__ __launch_bounds__(256) void ce_rows_soft_kernel(const float* __restrict__ logits,
                                                           const int64_t* __restrict__ labels,
                                                           const int64_t* __restrict__ labels2, SoftTarget t, int B,
                                                           int C, float gscale, float* __restrict__ dz,
                                                           float* __restrict__ rowstat) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * hg::kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= B) return;
  const int64_t la = labels[row], lb = labels2[row];
  const bool ok = la >= 0 && la < C && lb >= 0 && lb < C;
  soft_ce_row(logits + (size_t)row * C, C, ok ? (int)la : -1, ok ? (int)lb : -1, ok, t, gscale, nullptr,
              dz != nullptr ? dz + (size_t)row * C : nullptr, rowstat + (size_t)row * 3, lane);
}

// The DISTILL form of ce_rows_soft_kernel (knowledge distillation: --distill_ckpt): the same grid
// and rows per block; the row's wave also reads the teacher's logits row (distill_ce.h)
__global__ __launch_bounds__(256) void ce_rows_distill_kernel(const float* __restrict__ logits,
                                                              const int64_t* __restrict__ labels,
                                                              const int64_t* __restrict__ labels2, SoftTarget t,
                                                              const float* __restrict__ teacher, DistillArgs d, int B,
                                                              int C, float gscale, float* __restrict__ dz,
                                                              float* __restrict__ rowstat) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * hg::kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= B) return;
  const int64_t la = labels[row], lb = labels2[row];
  const bool ok = la >= 0 && la < C && lb >= 0 && lb < C;
  distill_ce_row(logits + (size_t)row * C, teacher + (size_t)row * C, C, ok ? (int)la : -1, ok ? (int)lb : -1, ok, t,
                 d, gscale, nullptr, dz != nullptr ? dz + (size_t)row * C : nullptr, rowstat + (size_t)row * 3, lane);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

Operand operand(const float* p, int lim_i, int lim_r, long si, long sr, int hc = INT_MAX, long hs = 0) {
  Operand o;
  o.p = p; o.lim_i = lim_i; o.lim_r = lim_r; o.hc = hc; o.hs = hs; o.si = si; o.sr = sr;
  return o;
}

void set_form(GemmParams& p, const hg::Form& f) {
  p.M = f.m; p.N = f.n; p.chunks = f.chunks; p.tiles_n = f.tiles_n; p.tiles = f.tiles;
}

}  // namespace

bool head_gemm_supported(int G, int B, int K, int C) { return hg::supported(G, B, K, C); }

hipError_t launch_head_gemm_logits(const float* x, const float* W, const float* bias, const int64_t* labels, int G,
                                   int B, int K, int C, float gscale, float* logits, float* dz, float* rowstat,
                                   hipStream_t s, const int64_t* rows, long N) {
  hg::Plan pl;
  if (!hg::make_plan(G, B, K, C, &pl) || (rows != nullptr && N < 1)) return hipErrorInvalidValue;
  if (x == nullptr || W == nullptr || bias == nullptr || labels == nullptr || logits == nullptr || rowstat == nullptr)
    return hipErrorInvalidValue;
  // (a bank may sit at any 4-byte alignment: its rows are then staged 4 bytes at a time)
  if ((rows == nullptr && !aligned16(x)) || !aligned16(W) || !aligned16(logits) || (dz != nullptr && !aligned16(dz)))
    return hipErrorInvalidValue;
  GemmParams p = {};
  p.a = operand(x, B, K, K, 1);
  p.b = operand(W, G * C, K, K, 1);
  set_form(p, pl.nt);
  p.G = G; p.B = B; p.C = C; p.K = K;
  p.out = logits;
  p.bias = bias;
  const RowMap rm = {rows, N};
  const dim3 grid(pl.nt.tiles), rgrid(pl.row_blocks), blk(256);
  if (rows == nullptr) {
    hipLaunchKernelGGL((head_gemm_kernel<kVec, kVec, kLogits>), grid, blk, 0, s, p, rm);
    SDX_LAUNCH_CHECK();
    hipLaunchKernelGGL(ce_rows_kernel<false>, rgrid, blk, 0, s, logits, labels, rm, pl.rows, B, C, gscale, dz,
                       rowstat);
    SDX_LAUNCH_CHECK();
    return hipSuccess;
  }
  if (aligned16(x))   // K = 64·j: every bank row is 16-byte aligned when the bank is
    hipLaunchKernelGGL((head_gemm_kernel<kVec, kVec, kLogits, kMapOut>), grid, blk, 0, s, p, rm);
  else
    hipLaunchKernelGGL((head_gemm_kernel<kRowScalar, kVec, kLogits, kMapOut>), grid, blk, 0, s, p, rm);
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ce_rows_kernel<true>, rgrid, blk, 0, s, logits, labels, rm, pl.rows, B, C, gscale, dz, rowstat);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_head_gemm_logits_soft(const float* x, const float* W, const float* bias, const int64_t* labels,
                                        const int64_t* labels2, float lam, float eps, int B, int K, int C,
                                        float gscale, float* logits, float* dz, float* rowstat, hipStream_t s) {
  hg::Plan pl;
  if (!hg::make_plan(1, B, K, C, &pl)) return hipErrorInvalidValue;
  if (x == nullptr || W == nullptr || bias == nullptr || labels == nullptr || labels2 == nullptr ||
      logits == nullptr || rowstat == nullptr)
    return hipErrorInvalidValue;
  if (!aligned16(x) || !aligned16(W) || !aligned16(logits) || (dz != nullptr && !aligned16(dz)))
    return hipErrorInvalidValue;
  if (!(lam >= 0.f && lam <= 1.f) || !(eps >= 0.f && eps < 1.f)) return hipErrorInvalidValue;
  GemmParams p = {};
  p.a = operand(x, B, K, K, 1);
  p.b = operand(W, C, K, K, 1);
  set_form(p, pl.nt);
  p.G = 1; p.B = B; p.C = C; p.K = K;
  p.out = logits;
  p.bias = bias;
  // the plain launcher's logits GEMM, then the soft row kernel
  hipLaunchKernelGGL((head_gemm_kernel<kVec, kVec, kLogits>), dim3(pl.nt.tiles), dim3(256), 0, s, p,
                     RowMap{nullptr, 0});
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ce_rows_soft_kernel, dim3(pl.row_blocks), dim3(256), 0, s, logits, labels, labels2,
                     make_soft_target(lam, eps, C), B, C, gscale, dz, rowstat);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_head_gemm_logits_distill(const float* x, const float* W, const float* bias, const int64_t* labels,
                                           const int64_t* labels2, float lam, float eps, const float* teacher,
                                           float tau, float alpha, int B, int K, int C, float gscale, float* logits,
                                           float* dz, float* rowstat, hipStream_t s) {
  hg::Plan pl;
  if (!hg::make_plan(1, B, K, C, &pl)) return hipErrorInvalidValue;
  if (x == nullptr || W == nullptr || bias == nullptr || labels == nullptr || labels2 == nullptr ||
      teacher == nullptr || logits == nullptr || rowstat == nullptr)
    return hipErrorInvalidValue;
  if (!aligned16(x) || !aligned16(W) || !aligned16(logits) || (dz != nullptr && !aligned16(dz)))
    return hipErrorInvalidValue;
  if (!(lam >= 0.f && lam <= 1.f) || !(eps >= 0.f && eps < 1.f)) return hipErrorInvalidValue;
  if (!distill_args_ok(tau, alpha)) return hipErrorInvalidValue;
  GemmParams p = {};
  p.a = operand(x, B, K, K, 1);
  p.b = operand(W, C, K, K, 1);
  set_form(p, pl.nt);
  p.G = 1; p.B = B; p.C = C; p.K = K;
  p.out = logits;
  p.bias = bias;
  // the plain launcher's logits GEMM, then the distill row kernel
  hipLaunchKernelGGL((head_gemm_kernel<kVec, kVec, kLogits>), dim3(pl.nt.tiles), dim3(256), 0, s, p,
                     RowMap{nullptr, 0});
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ce_rows_distill_kernel, dim3(pl.row_blocks), dim3(256), 0, s, logits, labels, labels2,
                     make_soft_target(lam, eps, C), teacher, make_distill_args(tau, alpha), B, C, gscale, dz,
                     rowstat);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_head_gemm_stats(int G, int B, int K, int C, const float* rowstat, float* stats, float* loss,
                                  hipStream_t s) {
  if (!hg::supported(G, B, K, C) || rowstat == nullptr || stats == nullptr) return hipErrorInvalidValue;
  GemmParams p = {};
  p.G = G; p.B = B; p.C = C; p.K = K;
  p.rowstat = rowstat;
  p.stats = stats;
  p.loss = loss;
  hipLaunchKernelGGL(head_stats_kernel, dim3(1), dim3(256), 0, s, p);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_head_gemm_sgd(const float* x, const float* dz, int G, int B, int K, int C, float* W, float* bias,
                                float* bufW, float* bufb, const float* lrs, const float* wds, float mom, int first,
                                const float* rowstat, float* stats, hipStream_t s, const int64_t* rows, long N) {
  hg::Plan pl;
  if (!hg::make_plan(G, B, K, C, &pl) || (rows != nullptr && N < 1)) return hipErrorInvalidValue;
  if (x == nullptr || dz == nullptr || W == nullptr || bias == nullptr || bufW == nullptr || bufb == nullptr ||
      lrs == nullptr || wds == nullptr || rowstat == nullptr || stats == nullptr)
    return hipErrorInvalidValue;
  if ((rows == nullptr && !aligned16(x)) || !aligned16(dz) || !aligned16(W) || !aligned16(bufW))
    return hipErrorInvalidValue;
  GemmParams p = {};
  p.a = operand(dz, G * C, B, 1, C, C, (long)B * C);
  p.b = operand(x, K, B, 1, K);
  set_form(p, pl.tn);
  p.G = G; p.B = B; p.C = C; p.K = K;
  p.W = W; p.bufW = bufW; p.bvec = bias; p.bufb = bufb;
  for (int h = 0; h < G; ++h) {
    p.hp.lr[h] = lrs[h];
    p.hp.wd[h] = wds[h];
  }
  p.mom = mom;
  p.first = first;
  p.dz = dz; p.rowstat = rowstat; p.stats = stats;
  const dim3 grid(pl.tn.tiles + pl.bias_blocks);
  if (rows == nullptr)
    hipLaunchKernelGGL((head_gemm_kernel<kTrans, kTrans, kSgd>), grid, dim3(256), 0, s, p, RowMap{nullptr, 0});
  else
    hipLaunchKernelGGL((head_gemm_kernel<kTrans, kTrans, kSgd, kMapNone, kMapRed>), grid, dim3(256), 0, s, p,
                       RowMap{rows, N});
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_head_gemm_bwd(const float* x, const float* dz, const float* W, int B, int K, int C,
                                const float* gout, float* dX, float* dW, float* db, const float* rowstat,
                                float* stats, float* loss, hipStream_t s) {
  hg::Plan pl;
  if (!hg::make_plan(1, B, K, C, &pl)) return hipErrorInvalidValue;
  if (x == nullptr || dz == nullptr || W == nullptr || gout == nullptr || rowstat == nullptr || stats == nullptr ||
      loss == nullptr)
    return hipErrorInvalidValue;
  if ((dW == nullptr) != (db == nullptr) || (dX == nullptr && dW == nullptr)) return hipErrorInvalidValue;
  if (!aligned16(x) || !aligned16(dz) || !aligned16(W) || !aligned16(dX) || !aligned16(dW))
    return hipErrorInvalidValue;
  GemmParams p = {};
  p.G = 1; p.B = B; p.C = C; p.K = K;
  p.gout = gout;
  if (dX != nullptr) {
    p.a = operand(dz, B, C, C, 1);
    p.b = operand(W, K, C, 1, K);
    set_form(p, pl.nn);
    p.out = dX;
    hipLaunchKernelGGL((head_gemm_kernel<kRowScalar, kTrans, kDx>), dim3(pl.nn.tiles), dim3(256), 0, s, p,
                       RowMap{nullptr, 0});
    SDX_LAUNCH_CHECK();
  }
  p.rowstat = rowstat; p.stats = stats; p.loss = loss;
  if (dW != nullptr) {
    p.a = operand(dz, C, B, 1, C, C, (long)B * C);
    p.b = operand(x, K, B, 1, K);
    set_form(p, pl.tn);
    p.out = dW;
    p.bvec = db;
    p.dz = dz;
    hipLaunchKernelGGL((head_gemm_kernel<kTrans, kTrans, kDw>), dim3(pl.tn.tiles + pl.bias_blocks), dim3(256), 0, s,
                       p, RowMap{nullptr, 0});
  } else {
    hipLaunchKernelGGL(head_stats_kernel, dim3(1), dim3(256), 0, s, p);
  }
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
