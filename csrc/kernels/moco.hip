// MoCo v2 loss for gfx950 (--method MoCo): InfoNCE of N query rows against their keys and a queue of
// K negatives that is a constant of the step, with the backward for the queries alone. The queue is kept
// as two bf16 planes [2][K][D], hi = bf16_rn(x) and lo = bf16_rn(x − hi), its value hi + lo: both planes
// are MFMA operands as they lie in memory, so a tile goes global -> registers -> LDS as 16-byte cells with
// no conversion. Products are bf16x3 (hi·hi + hi·lo + lo·hi) on v_mfma_f32_16x16x32_bf16. fp32 in and out.
//
//   moco_prep     one wave per row i: Σq², Σk² in fp64 (lanes strided over D, a butterfly), q̂ = q·rn_q,
//                 k̂ = k·rn_k with rn = fp32(1 / max(‖x‖, 1e-12)), and l⁺_i = q̂_i·k̂_i as an fp64 dot.
//   moco_sweep    grid (row blocks, splits). A workgroup owns 64 q rows, a wave 16 of them: their hi/lo
//                 fragments are split once and stay in registers. It walks one contiguous span of the
//                 queue in tiles of 32 rows through two LDS buffers: tile t + 1 is loaded to registers
//                 before the MFMAs of tile t and committed after them, ONE barrier per tile. The tile
//                 product is Sᵀ = Q_tile·q̂ᵀ, so a lane holds ONE q row (column c) and 8 queue rows.
//                 FWD: the lane keeps an online (max, sumexp) of its q row; the 4 lane groups of a wave
//                 are merged by two shuffles and one pair per (split, row) is written. Each wave sees
//                 the whole span, so nothing is left for the workgroup to combine.
//                 BWD: p = exp(s/T − lse) is formed in the accumulator layout, split to hi/lo and used
//                 as the B operand of dq̂ᵀ[d][row] += Q_tileᵀ·Pᵀ (supcon.hip's accumulator-as-operand
//                 step), the A operand by transposed LDS reads of the same staged tile. One slab per
//                 split, stored as float4 straight from the accumulators.
//   moco_finish   one block: per row the split pairs and l⁺/T are merged in split order to lse_i; the
//                 row terms l⁺/T − lse in fp64, thread t the rows ≡ t (mod 256) ascending, then the 256
//                 partials in thread order; loss = −Σ / n_total, a device scalar.
//   moco_dq       one wave per row: dq̂ = (Σ_split slab + (p⁺ − 1)·k̂)·g/(n_total·T), the slabs in split
//                 order, then dq = (dq̂ − q̂·(q̂·dq̂))·rn_q with the dot in fp64. Nothing for k or the queue.
//   moco_enqueue  one wave per key row: split to hi/lo, 4-byte vector stores into both planes at slot
//                 (ptr + i) mod K; a second one-thread launch then advances the device-resident ptr
//                 (inside the first, a late workgroup would read the advanced value). No host sync.
//
// Staging: 16-byte loads committed through swizzled cells, not LDS-DMA. A DMA load lays a wave's cells
// down linearly behind one base, so a row of 2·D bytes (a multiple of 128) would put the 16 rows of a
// fragment read on the same banks; the register path lets every cell take the XOR-swizzled slot that
// supcon.hip measured conflict-free for both read patterns used here (ds_read_b128 along a row,
// ds_read_b64_tr_b16 down a column). D = 64 and 192, whose rows are no multiple of 256 bytes, pad the
// row by 16 bytes instead.
//
// Determinism: no atomics, no cross-workgroup wait; the split count is a function of (N, K) and every
// cross-split sum is added by a later launch in split order.
#include "common.h"
#include "launchers.h"
#include "moco_plan.h"

using namespace sdx;

namespace {

namespace mp = sdx_moco;

constexpr int TK = mp::kTileRows;
constexpr int RB = mp::kRowBlock;
static_assert(TK == 32 && RB == 64, "the sweep is written for 32-row tiles and 4 waves x 16 q rows");

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int D>
constexpr int row_stride() {
  return D % 128 == 0 ? 2 * D : 2 * D + 16;
}

// byte offset of (row, byte of the bf16 row) in a staged plane image
template <int D>
__device__ __forceinline__ int q_off(int row, int byte) {
  if constexpr (D % 128 == 0) {
    const int sw = (row & 7) << 1;
    return row * (D * 2) + (((byte >> 4) ^ sw) << 4) + (byte & 15);
  } else {
    return row * (D * 2 + 16) + byte;
  }
}

// 8 floats -> the hi and lo fragments (element j in the low half of word j / 2)
__device__ __forceinline__ void split8(const float (&x)[8], bf16x8& hi, bf16x8& lo) {
  uint32_t wh[4], wl[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    wh[j] = pack_bf2(x[2 * j], x[2 * j + 1]);
    const float h0 = __uint_as_float(wh[j] << 16), h1 = __uint_as_float(wh[j] & 0xffff0000u);
    wl[j] = pack_bf2(x[2 * j] - h0, x[2 * j + 1] - h1);
  }
  hi = __builtin_bit_cast(bf16x8, (u32x4){wh[0], wh[1], wh[2], wh[3]});
  lo = __builtin_bit_cast(bf16x8, (u32x4){wl[0], wl[1], wl[2], wl[3]});
}

// A tile of a plane is 32·D contiguous bf16: thread tid moves the 16-byte cells tid, tid + 256, ... of
// both planes, raw in registers between load() and commit().
template <int D>
struct TileStage {
  static constexpr int CPT = D / 64;   // cells of a thread per plane and tile
  static constexpr int CPR = D / 8;    // cells per row
  static constexpr int TILE_B = TK * row_stride<D>();
  u32x4 raw[2][CPT];
  int off[CPT];

  __device__ __forceinline__ void init(int tid) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int idx = i * 256 + tid;
      off[i] = q_off<D>(idx / CPR, 16 * (idx % CPR));
    }
  }

  // tile t of a queue whose planes hold whole tiles: t < K / 32
  __device__ __forceinline__ void load(const uint16_t* hi, const uint16_t* lo, int t) {
    const u32x4* sh = reinterpret_cast<const u32x4*>(hi + (size_t)t * TK * D) + threadIdx.x;
    const u32x4* sl = reinterpret_cast<const u32x4*>(lo + (size_t)t * TK * D) + threadIdx.x;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      raw[0][i] = sh[i * 256];
      raw[1][i] = sl[i * 256];
    }
  }

  __device__ __forceinline__ void commit(unsigned char* buf) const {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      *reinterpret_cast<u32x4*>(buf + off[i]) = raw[0][i];
      *reinterpret_cast<u32x4*>(buf + TILE_B + off[i]) = raw[1][i];
    }
  }
};

// ---- moco_prep -------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void moco_prep_kernel(const float* __restrict__ q, const float* __restrict__ k, int n,
                                                        int D, float* __restrict__ qhat, float* __restrict__ rq,
                                                        float* __restrict__ khat, float* __restrict__ lpos) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* qs = q + (size_t)row * D;
  const float* ks = k + (size_t)row * D;
  double sq = 0.0, sk = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double a = (double)qs[d], b = (double)ks[d];
    sq += a * a;
    sk += b * b;
  }
  sq = wave_sum_f64(sq);
  sk = wave_sum_f64(sk);
  const float rnq = (float)(1.0 / fmax(sqrt(sq), 1e-12));
  const float rnk = (float)(1.0 / fmax(sqrt(sk), 1e-12));
  double dot = 0.0;
  for (int d = lane; d < D; d += 64) {
    const float a = qs[d] * rnq, b = ks[d] * rnk;
    qhat[(size_t)row * D + d] = a;
    khat[(size_t)row * D + d] = b;
    dot += (double)a * (double)b;
  }
  dot = wave_sum_f64(dot);
  if (lane == 0) {
    rq[row] = rnq;
    lpos[row] = (float)dot;
  }
}

// ---- moco_sweep ------------------------------------------------------------------------------

struct SweepParams {
  const float* qhat;        // [N][D]
  const uint16_t* queue;    // [2][K][D] bf16 planes
  const float* lse;         // [N] (bwd)
  float2* part;             // fwd: [splits][N] (max, sumexp)
  float* slab;              // bwd: [splits][N][D]
  int N, K, tiles, span_tiles;
  float inv_temp;
};

template <int D, bool BWD>
__global__ __launch_bounds__(256) void moco_sweep_kernel(SweepParams p) {
  constexpr int KS = D / 32;                   // MFMA k-steps over the feature dim
  constexpr int RS = row_stride<D>();
  constexpr int TILE_B = TK * RS;              // one plane image
  constexpr int BUF = 2 * TILE_B;              // hi + lo
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int h = lane >> 4;       // 16-lane group
  const int c = lane & 15;       // column of the MFMA tile = this lane's q row
  const int own = blockIdx.x * RB + wv * 16 + c;
  const int own_ld = own < p.N ? own : p.N - 1;   // a row past N is computed on a copy and not written
  const int split = blockIdx.y;

  // ---- q fragments (B operand of the tile product), split once ----
  bf16x8 ob_hi[KS], ob_lo[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const float4* src = reinterpret_cast<const float4*>(p.qhat + (size_t)own_ld * D + 32 * s + 8 * h);
    const float4 v0 = src[0], v1 = src[1];
    const float xs[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    split8(xs, ob_hi[s], ob_lo[s]);
  }

  float own_lse = 0.f;
  if constexpr (BWD) own_lse = p.lse[own_ld];
  float run_m = -INFINITY, run_l = 0.f;
  // bwd accumulators: dq̂ᵀ tiles [d = 16q + 4h + r][row = c]
  f32x4 acc2[BWD ? D / 16 : 1];
#pragma unroll
  for (int q = 0; q < (BWD ? D / 16 : 1); ++q) acc2[q] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int t_begin = split * p.span_tiles;
  const int t_end = t_begin + p.span_tiles < p.tiles ? t_begin + p.span_tiles : p.tiles;
  const uint16_t* plane_hi = p.queue;
  const uint16_t* plane_lo = p.queue + (size_t)p.K * D;

  TileStage<D> st;
  st.init(tid);
  st.load(plane_hi, plane_lo, t_begin);
  st.commit(smem);
  for (int t = t_begin; t < t_end; ++t) {
    unsigned char* cur = smem + ((t - t_begin) & 1) * BUF;
    unsigned char* nxt = smem + ((t - t_begin + 1) & 1) * BUF;
    // tile t is visible, and every wave is done reading the buffer that tile t + 1 goes to
    __syncthreads();
    const bool more = t + 1 < t_end;
    if (more) st.load(plane_hi, plane_lo, t + 1);   // in flight under this tile's MFMAs
    const unsigned char* lds_hi = cur;
    const unsigned char* lds_lo = cur + TILE_B;

    // ---- Sᵀ tiles: acc[t2][r] = <queue[32t + 16·t2 + 4h + r], q̂[c]> ----
    f32x4 acc[2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      acc[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int off = q_off<D>(16 * t2 + c, (32 * s + 8 * h) * 2);
        const bf16x8 a_hi = *reinterpret_cast<const bf16x8*>(lds_hi + off);
        const bf16x8 a_lo = *reinterpret_cast<const bf16x8*>(lds_lo + off);
        acc[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, ob_hi[s], acc[t2], 0, 0, 0);
        acc[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, ob_lo[s], acc[t2], 0, 0, 0);
        acc[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, ob_hi[s], acc[t2], 0, 0, 0);
      }
    }

    if constexpr (!BWD) {
      float sv[8];
      float tmax = -INFINITY;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        sv[k] = acc[k >> 2][k & 3] * p.inv_temp;
        tmax = fmaxf(tmax, sv[k]);
      }
      const float mn = fmaxf(run_m, tmax);
      float l = run_l * __expf(run_m - mn);   // the first tile: 0·exp(−inf) = 0
#pragma unroll
      for (int k = 0; k < 8; ++k) l += __expf(sv[k] - mn);
      run_m = mn;
      run_l = l;
    } else {
      // ---- Pᵀ in the accumulator layout, split into the hi/lo B fragments ----
      float pv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) pv[k] = __expf(acc[k >> 2][k & 3] * p.inv_temp - own_lse);
      bf16x8 g_hi, g_lo;
      split8(pv, g_hi, g_lo);
      // ---- dq̂ᵀ[d][row] += Σ_j queue[j][d]·Pᵀ[j][row]; the A operand by transposed LDS reads ----
      const int qq = c >> 2, pp = c & 3;
#pragma unroll
      for (int q = 0; q < D / 16; ++q) {
        bf16x8 a2_hi, a2_lo;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const int off = q_off<D>(16 * tt + 4 * h + qq, (16 * q + 4 * pp) * 2);
          const bf16x4 th = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(lds_hi + off));
          const bf16x4 tl = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(lds_lo + off));
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a2_hi[4 * tt + e] = th[e];
            a2_lo[4 * tt + e] = tl[e];
          }
        }
        acc2[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2_hi, g_hi, acc2[q], 0, 0, 0);
        acc2[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2_hi, g_lo, acc2[q], 0, 0, 0);
        acc2[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2_lo, g_hi, acc2[q], 0, 0, 0);
      }
    }
    if (more) st.commit(nxt);
  }

  if constexpr (!BWD) {
    // the 4 lane groups that hold the same q row, merged in a fixed order
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float m2 = __shfl_xor(run_m, off, 64);
      const float l2 = __shfl_xor(run_l, off, 64);
      const float mn = fmaxf(run_m, m2);
      run_l = run_l * __expf(run_m - mn) + l2 * __expf(m2 - mn);
      run_m = mn;
    }
    if (h == 0 && own < p.N) {
      SDX_DCHECK(split < (int)gridDim.y);
      p.part[(size_t)split * p.N + own] = make_float2(run_m, run_l);
    }
  } else {
    if (own < p.N) {
      float* dst = p.slab + ((size_t)split * p.N + own) * D + 4 * h;
#pragma unroll
      for (int q = 0; q < D / 16; ++q)
        *reinterpret_cast<float4*>(dst + 16 * q) = make_float4(acc2[q][0], acc2[q][1], acc2[q][2], acc2[q][3]);
    }
  }
}

// ---- moco_finish -----------------------------------------------------------------------------

__global__ __launch_bounds__(256) void moco_finish_kernel(const float2* __restrict__ part,
                                                          const float* __restrict__ lpos, int N, int splits,
                                                          float inv_temp, double n_total, float* __restrict__ lse,
                                                          float* __restrict__ loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) {
    const float xp = lpos[i] * inv_temp;
    float m = xp, l = 1.f;
    for (int sp = 0; sp < splits; ++sp) {
      const float2 v = part[(size_t)sp * N + i];
      const float mn = fmaxf(m, v.x);
      l = l * __expf(m - mn) + v.y * __expf(v.x - mn);
      m = mn;
    }
    const float L = m + __logf(l);
    lse[i] = L;
    s += (double)xp - (double)L;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = 0.0;
  for (int t = 0; t < 256; ++t) s += red[t];
  loss[0] = (float)(-s / n_total);
}

// ---- moco_dq ---------------------------------------------------------------------------------

// scale = 1/(n_total·T)
__global__ __launch_bounds__(256) void moco_dq_kernel(const float* __restrict__ slab, int splits,
                                                      const float* __restrict__ qhat, const float* __restrict__ rq,
                                                      const float* __restrict__ khat, const float* __restrict__ lse,
                                                      const float* __restrict__ lpos, const float* __restrict__ g,
                                                      int N, int D, float inv_temp, float scale,
                                                      float* __restrict__ dq) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float pm1 = __expf(lpos[row] * inv_temp - lse[row]) - 1.f;
  const float sc = g[0] * scale;
  float v[4], qh[4];
  double dot = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = lane + 64 * j;
    v[j] = 0.f;
    qh[j] = 0.f;
    if (d < D) {
      float a = slab[(size_t)row * D + d];
      for (int sp = 1; sp < splits; ++sp) a += slab[((size_t)sp * N + row) * D + d];
      a += pm1 * khat[(size_t)row * D + d];
      v[j] = a * sc;
      qh[j] = qhat[(size_t)row * D + d];
      dot += (double)qh[j] * (double)v[j];
    }
  }
  const float dt = (float)wave_sum_f64(dot);
  const float rn = rq[row];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = lane + 64 * j;
    if (d < D) dq[(size_t)row * D + d] = (v[j] - qh[j] * dt) * rn;
  }
}

// ---- moco_enqueue ----------------------------------------------------------------------------

__global__ __launch_bounds__(256) void moco_enqueue_kernel(const float* __restrict__ keys, int n, int D, int K,
                                                           const int64_t* __restrict__ ptr,
                                                           uint16_t* __restrict__ queue) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  int64_t p0 = ptr[0] % K;
  if (p0 < 0) p0 += K;
  const int slot = (int)((p0 + row) % K);
  const float* src = keys + (size_t)row * D;
  uint32_t* hi = reinterpret_cast<uint32_t*>(queue + (size_t)slot * D);
  uint32_t* lo = reinterpret_cast<uint32_t*>(queue + ((size_t)K + slot) * D);
  for (int d2 = lane; d2 < D / 2; d2 += 64) {
    const float2 x = *reinterpret_cast<const float2*>(src + 2 * d2);
    const uint32_t wh = pack_bf2(x.x, x.y);
    const float h0 = __uint_as_float(wh << 16), h1 = __uint_as_float(wh & 0xffff0000u);
    hi[d2] = wh;
    lo[d2] = pack_bf2(x.x - h0, x.y - h1);
  }
}

__global__ void moco_ptr_kernel(int64_t* ptr, int n, int K) {
  int64_t p0 = ptr[0] % K;
  if (p0 < 0) p0 += K;
  ptr[0] = (p0 + n) % K;
}

template <bool BWD>
hipError_t launch_sweep(const mp::Plan& pl, const SweepParams& p, hipStream_t s) {
  const dim3 grid(pl.row_blocks, pl.splits);
  switch (pl.d) {
    case 64: hipLaunchKernelGGL((moco_sweep_kernel<64, BWD>), grid, dim3(256), 0, s, p); break;
    case 128: hipLaunchKernelGGL((moco_sweep_kernel<128, BWD>), grid, dim3(256), 0, s, p); break;
    case 192: hipLaunchKernelGGL((moco_sweep_kernel<192, BWD>), grid, dim3(256), 0, s, p); break;
    case 256: hipLaunchKernelGGL((moco_sweep_kernel<256, BWD>), grid, dim3(256), 0, s, p); break;
    default: return hipErrorInvalidValue;
  }
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

bool pos(double x) { return x > 0.0 && x < 1e30; }

}  // namespace

bool moco_supported(long n, long D, long K) { return mp::supported(n, D, K); }

hipError_t launch_moco_prep(const float* q, const float* k, int n, int D, float* qhat, float* rq, float* khat,
                            float* lpos, hipStream_t s) {
  if (n < 1 || D < mp::kMinD || D > mp::kMaxD || D % 64 != 0 || (long)n * D >= (1L << 31) || q == nullptr ||
      k == nullptr || qhat == nullptr || rq == nullptr || khat == nullptr || lpos == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(moco_prep_kernel, dim3((n + 3) / 4), dim3(256), 0, s, q, k, n, D, qhat, rq, khat, lpos);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_moco_fwd(const float* qhat, const float* lpos, const uint16_t* queue, int n, int D, int K,
                           double temp, double n_total, float* part, float* lse, float* loss, hipStream_t s) {
  mp::Plan pl;
  if (!mp::make_plan(n, D, K, &pl) || qhat == nullptr || lpos == nullptr || queue == nullptr || part == nullptr ||
      lse == nullptr || loss == nullptr || !pos(temp) || !(n_total >= n) || !mp::aligned16(qhat) ||
      !mp::aligned16(queue) || !mp::aligned16(part))
    return hipErrorInvalidValue;
  SweepParams p = {};
  p.qhat = qhat; p.queue = queue; p.part = reinterpret_cast<float2*>(part);
  p.N = n; p.K = K; p.tiles = pl.tiles; p.span_tiles = pl.span_tiles;
  p.inv_temp = (float)(1.0 / temp);
  hipError_t e = launch_sweep<false>(pl, p, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(moco_finish_kernel, dim3(1), dim3(256), 0, s, (const float2*)p.part, lpos, n, pl.splits,
                     p.inv_temp, n_total, lse, loss);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_moco_bwd(const float* qhat, const float* rq, const float* khat, const uint16_t* queue,
                           const float* lse, const float* lpos, const float* g, int n, int D, int K, double temp,
                           double n_total, float* slab, float* dq, hipStream_t s) {
  mp::Plan pl;
  if (!mp::make_plan(n, D, K, &pl) || qhat == nullptr || rq == nullptr || khat == nullptr || queue == nullptr ||
      lse == nullptr || lpos == nullptr || g == nullptr || slab == nullptr || dq == nullptr || !pos(temp) ||
      !(n_total >= n) || !mp::aligned16(qhat) || !mp::aligned16(queue) || !mp::aligned16(slab))
    return hipErrorInvalidValue;
  SweepParams p = {};
  p.qhat = qhat; p.queue = queue; p.lse = lse; p.slab = slab;
  p.N = n; p.K = K; p.tiles = pl.tiles; p.span_tiles = pl.span_tiles;
  p.inv_temp = (float)(1.0 / temp);
  hipError_t e = launch_sweep<true>(pl, p, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(moco_dq_kernel, dim3((n + 3) / 4), dim3(256), 0, s, (const float*)slab, pl.splits, qhat, rq, khat,
                     lse, lpos, g, n, D, p.inv_temp, (float)(1.0 / (n_total * temp)), dq);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_moco_enqueue(const float* keys, int n, int D, int K, int64_t* ptr, uint16_t* queue, hipStream_t s) {
  // n <= K: two key rows never share a slot
  if (!mp::supported(1, D, K) || n < 1 || n > K || keys == nullptr || ptr == nullptr || queue == nullptr ||
      ((uintptr_t)keys & 7) != 0 || ((uintptr_t)queue & 3) != 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(moco_enqueue_kernel, dim3((n + 3) / 4), dim3(256), 0, s, keys, n, D, K, (const int64_t*)ptr,
                     queue);
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(moco_ptr_kernel, dim3(1), dim3(1), 0, s, ptr, n, K);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
