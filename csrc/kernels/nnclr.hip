// NNCLR loss for gfx950 (--method NNCLR): every projection's nearest neighbour in a support queue of K
// rows, then a cross-view InfoNCE of the neighbours of view v against the predictions of view 1 − v, with
// the backward for the predictions alone. The queue is MoCo's: two bf16 planes [2][K][D], hi = bf16_rn(x)
// and lo = bf16_rn(x − hi), its value hi + lo. Every MFMA operand of this unit lies in memory as such a
// pair of planes (ẑ, p̂, and the neighbours, which are copies of queue rows), so a tile goes global ->
// registers -> LDS as 16-byte cells and a held row global -> registers with no conversion. Products are
// bf16x3 (hi·hi + hi·lo + lo·hi) on v_mfma_f32_16x16x32_bf16. fp32 in and out.
//
//   nnclr_prep    one wave per row: Σx² in fp64, rn = fp32(1 / max(‖x‖, 1e-12)), x̂ = x·rn as fp32 (what the
//                 enqueue takes) and as hi/lo planes. Launched for z [2n][D] and for p [2N][D].
//   nnclr_search  grid (row blocks of the 2n ẑ rows, splits of the queue). A workgroup holds 64 ẑ rows, a
//                 wave 16 of them, as hi/lo fragments in registers and walks ONE contiguous span of the
//                 queue in 32-row tiles through two LDS buffers: tile t + 1 is loaded to registers before
//                 the MFMAs of tile t and committed after them, ONE barrier per tile. Sᵀ = Q_tile·ẑᵀ, so a
//                 lane holds one query row (column c) and 8 queue rows in ascending index: it keeps a
//                 running (best, index) under strict >, so the lowest index of equal values stays. The 4
//                 lane groups of a query row combine at the end of the span (greater value, then lower
//                 index). One (value, index) pair per (split, row).
//   nnclr_pick    one wave per row: the pairs merged in split order under the same rule; idx (int32), the
//                 winning similarity, and the winning queue row copied plane by plane into [2][2n][D].
//   nnclr_sweep   grid (row blocks, splits, views), the same tile pipeline over a ragged streamed axis (a
//                 row past its end is a copy of the last and is masked).
//                 FWD: holds 64 neighbour rows of view v, streams the N p̂ rows of view 1 − v, an online
//                 (max, sumexp) per held row, one pair per (split, row).
//                 BWD: holds 64 p̂ rows k of view 1 − v, streams the n neighbour rows i of view v. The tile
//                 is recomputed, P = exp(s/τ − lse_i) − [i + pos_offset = k] is formed in the accumulator
//                 layout, where i is the accumulator ROW: the normaliser is one value per accumulator
//                 row, 8 per lane and tile. P is split to hi/lo and is the B operand of
//                 dp̂ᵀ[d][k] += nn_tileᵀ·Pᵀ, the A operand by transposed LDS reads of the staged tile. Rows
//                 i >= n have P = 0 exactly. One slab per split, float4 stores from the accumulators.
//   nnclr_finish  one wave per neighbour row: the split pairs merged in split order to lse; the positive
//                 logit nn_v[i]·p̂_{1−v}[i + pos_offset] as an fp64 dot of the planes' values; the row term
//                 lse − l⁺/τ in fp64.
//   nnclr_total   one block: the row terms in fp64, thread t the rows ≡ t (mod 256) ascending, then the
//                 256 partials in thread order; loss = Σ / (2N), a device scalar.
//   nnclr_dp      one wave per p row: dp̂ = Σ_split slab·g/(2N·τ) in split order, then
//                 dp = (dp̂ − p̂·(p̂·dp̂))·rn with the dot in fp64. Nothing for z or the queue.
//
// Staging is moco.hip's choice, for its reasons: 16-byte loads committed through XOR-swizzled cells (rows
// of D = 64 and 192 padded by 16 bytes instead), conflict-free for ds_read_b128 along a row and
// ds_read_b64_tr_b16 down a column.
//
// Determinism: no atomics, no cross-workgroup wait; every split count is a function of the sizes and
// every cross-split combination is made by a later launch in split order.
#include "common.h"
#include "launchers.h"
#include "nnclr_plan.h"

using namespace sdx;

namespace {

namespace np = sdx_nnclr;

constexpr int TK = np::kTileRows;
constexpr int RB = np::kRowBlock;
static_assert(TK == 32 && RB == 64, "the kernels are written for 32-row tiles and 4 waves x 16 held rows");

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int D>
constexpr int row_stride() {
  return D % 128 == 0 ? 2 * D : 2 * D + 16;
}

// byte offset of (row, byte of the bf16 row) in a staged plane image
template <int D>
__device__ __forceinline__ int t_off(int row, int byte) {
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

__device__ __forceinline__ float bf_value(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// s/τ rounded once, in the forward and in the backward alike: left to the compiler, the product is fused into
// the subtraction that follows it (x·it − lse) in one sweep and not in the other, and where lse is the logit
// itself, as with one streamed row, exp(x − lse) − 1 is then an ulp instead of 0
__device__ __forceinline__ float logit(float s, float it) {
  float x = s * it;
  asm volatile("" : "+v"(x));
  return x;
}

// (m, l) <- (m, l) + (m2, l2) of an online logsumexp; a side that has seen no row is (−inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& l, float m2, float l2) {
  const float mn = fmaxf(m, m2);
  const float ms = mn == -INFINITY ? 0.f : mn;
  l = l * __expf(m - ms) + l2 * __expf(m2 - ms);
  m = mn;
}

// (best, bi) <- the better of two candidates: the greater value, at equal value the lower index
__device__ __forceinline__ void top_merge(float& best, int& bi, float v2, int i2) {
  if (v2 > best || (v2 == best && i2 < bi)) {
    best = v2;
    bi = i2;
  }
}

// Rows first .. first + 31 of a pair of planes [rows][D]: thread tid moves the 16-byte cells tid,
// tid + 256, ... of both planes, raw in registers between load() and commit(). A row past the planes'
// end is read as a copy of the last row; the caller masks it.
template <int D>
struct TileStage {
  static constexpr int CPT = D / 64;   // cells of a thread per plane and tile
  static constexpr int CPR = D / 8;    // cells per row
  static constexpr int TILE_B = TK * row_stride<D>();
  u32x4 raw[2][CPT];
  int off[CPT], row[CPT], col[CPT];

  __device__ __forceinline__ void init(int tid) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int idx = i * 256 + tid;
      row[i] = idx / CPR;
      col[i] = 8 * (idx % CPR);
      off[i] = t_off<D>(row[i], 2 * col[i]);
    }
  }

  __device__ __forceinline__ void load(const uint16_t* hi, const uint16_t* lo, int first, int rows) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int r = first + row[i] < rows ? first + row[i] : rows - 1;
      const size_t e = (size_t)r * D + col[i];
      raw[0][i] = *reinterpret_cast<const u32x4*>(hi + e);
      raw[1][i] = *reinterpret_cast<const u32x4*>(lo + e);
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

// the hi/lo fragments of one held row (the B operand of the tile product): 16-byte loads of the planes
template <int D>
__device__ __forceinline__ void held_fragments(const uint16_t* hi, const uint16_t* lo, int h, bf16x8 (&f_hi)[D / 32],
                                               bf16x8 (&f_lo)[D / 32]) {
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    f_hi[s] = *reinterpret_cast<const bf16x8*>(hi + 32 * s + 8 * h);
    f_lo[s] = *reinterpret_cast<const bf16x8*>(lo + 32 * s + 8 * h);
  }
}

// acc[t2][r] = <tile row 16·t2 + 4h + r, held row c>, bf16x3. LO_FIRST adds the tile's lo plane before the
// held row's: the backward sweep, whose tile and held row are the forward's held row and tile, then sums
// the same three products in the forward's order and recomputes its logits bit for bit.
template <int D, bool LO_FIRST = false>
__device__ __forceinline__ void tile_product(const unsigned char* lds_hi, const unsigned char* lds_lo, int c, int h,
                                             const bf16x8 (&f_hi)[D / 32], const bf16x8 (&f_lo)[D / 32],
                                             f32x4 (&acc)[2]) {
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    acc[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < D / 32; ++s) {
      const int off = t_off<D>(16 * t2 + c, (32 * s + 8 * h) * 2);
      const bf16x8 a_hi = *reinterpret_cast<const bf16x8*>(lds_hi + off);
      const bf16x8 a_lo = *reinterpret_cast<const bf16x8*>(lds_lo + off);
      acc[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, f_hi[s], acc[t2], 0, 0, 0);
      if constexpr (LO_FIRST) {
        acc[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, f_hi[s], acc[t2], 0, 0, 0);
        acc[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, f_lo[s], acc[t2], 0, 0, 0);
      } else {
        acc[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, f_lo[s], acc[t2], 0, 0, 0);
        acc[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, f_hi[s], acc[t2], 0, 0, 0);
      }
    }
  }
}

// ---- nnclr_prep ------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void nnclr_prep_kernel(const float* __restrict__ x, int rows, int D,
                                                         float* __restrict__ xhat, uint16_t* __restrict__ planes,
                                                         float* __restrict__ rn) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float2* src = reinterpret_cast<const float2*>(x + (size_t)row * D);
  double ss = 0.0;
  for (int d2 = lane; d2 < D / 2; d2 += 64) {
    const float2 a = src[d2];
    ss += (double)a.x * (double)a.x + (double)a.y * (double)a.y;
  }
  ss = wave_sum_f64(ss);
  const float r = (float)(1.0 / fmax(sqrt(ss), 1e-12));
  uint32_t* hi = reinterpret_cast<uint32_t*>(planes + (size_t)row * D);
  uint32_t* lo = reinterpret_cast<uint32_t*>(planes + ((size_t)rows + row) * D);
  for (int d2 = lane; d2 < D / 2; d2 += 64) {
    const float2 a = src[d2];
    const float x0 = a.x * r, x1 = a.y * r;
    if (xhat != nullptr) *reinterpret_cast<float2*>(xhat + (size_t)row * D + 2 * d2) = make_float2(x0, x1);
    const uint32_t wh = pack_bf2(x0, x1);
    const float h0 = __uint_as_float(wh << 16), h1 = __uint_as_float(wh & 0xffff0000u);
    hi[d2] = wh;
    lo[d2] = pack_bf2(x0 - h0, x1 - h1);
  }
  if (lane == 0 && rn != nullptr) rn[row] = r;
}

// ---- nnclr_search ----------------------------------------------------------------------------

struct SearchParams {
  const uint16_t* zpl;      // [2][R][D], R = 2n
  const uint16_t* queue;    // [2][K][D]
  int2* pair;               // [splits][R] (value bits, index)
  int R, K, tiles, span_tiles;
};

template <int D>
__global__ __launch_bounds__(256) void nnclr_search_kernel(SearchParams p) {
  constexpr int KS = D / 32;
  constexpr int TILE_B = TK * row_stride<D>();
  constexpr int BUF = 2 * TILE_B;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int h = lane >> 4;
  const int c = lane & 15;       // column of the MFMA tile = this lane's query row
  const int own = blockIdx.x * RB + wv * 16 + c;
  const int own_ld = own < p.R ? own : p.R - 1;   // a row past R is computed on a copy and not written
  const int split = blockIdx.y;

  bf16x8 f_hi[KS], f_lo[KS];
  held_fragments<D>(p.zpl + (size_t)own_ld * D, p.zpl + ((size_t)p.R + own_ld) * D, h, f_hi, f_lo);

  const int t_begin = split * p.span_tiles;
  const int t_end = t_begin + p.span_tiles < p.tiles ? t_begin + p.span_tiles : p.tiles;
  const uint16_t* plane_hi = p.queue;
  const uint16_t* plane_lo = p.queue + (size_t)p.K * D;

  // the index stays inside the span whatever the values are: nnclr_pick reads the queue at it
  float best = -INFINITY;
  int bi = TK * t_begin + 4 * h;

  TileStage<D> st;
  st.init(tid);
  st.load(plane_hi, plane_lo, TK * t_begin, p.K);
  st.commit(smem);
  for (int t = t_begin; t < t_end; ++t) {
    unsigned char* cur = smem + ((t - t_begin) & 1) * BUF;
    unsigned char* nxt = smem + ((t - t_begin + 1) & 1) * BUF;
    // tile t is visible, and every wave is done reading the buffer that tile t + 1 goes to
    __syncthreads();
    const bool more = t + 1 < t_end;
    if (more) st.load(plane_hi, plane_lo, TK * (t + 1), p.K);   // in flight under this tile's MFMAs
    f32x4 acc[2];
    tile_product<D>(cur, cur + TILE_B, c, h, f_hi, f_lo, acc);
    // queue rows 32t + 16·(k / 4) + 4h + (k % 4): ascending in k
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float v = acc[k >> 2][k & 3];
      if (v > best) {
        best = v;
        bi = TK * t + 16 * (k >> 2) + 4 * h + (k & 3);
      }
    }
    if (more) st.commit(nxt);
  }

#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const float v2 = __shfl_xor(best, off, 64);
    const int i2 = __shfl_xor(bi, off, 64);
    top_merge(best, bi, v2, i2);
  }
  if (h == 0 && own < p.R) p.pair[(size_t)split * p.R + own] = make_int2(__float_as_int(best), bi);
}

// ---- nnclr_pick ------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void nnclr_pick_kernel(const int2* __restrict__ pair, int splits, int R,
                                                         const uint16_t* __restrict__ queue, int K, int D,
                                                         int* __restrict__ idx, float* __restrict__ sim,
                                                         uint16_t* __restrict__ nnpl) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  int2 v = pair[row];
  float best = __int_as_float(v.x);
  int bi = v.y;
  for (int sp = 1; sp < splits; ++sp) {
    v = pair[(size_t)sp * R + row];
    top_merge(best, bi, __int_as_float(v.x), v.y);
  }
  bi = bi < 0 ? 0 : (bi < K ? bi : K - 1);   // already so by construction
  if (lane == 0) {
    idx[row] = bi;
    sim[row] = best;
  }
  const uint32_t* sh = reinterpret_cast<const uint32_t*>(queue + (size_t)bi * D);
  const uint32_t* sl = reinterpret_cast<const uint32_t*>(queue + ((size_t)K + bi) * D);
  uint32_t* dh = reinterpret_cast<uint32_t*>(nnpl + (size_t)row * D);
  uint32_t* dl = reinterpret_cast<uint32_t*>(nnpl + ((size_t)R + row) * D);
  for (int d2 = lane; d2 < D / 2; d2 += 64) {
    dh[d2] = sh[d2];
    dl[d2] = sl[d2];
  }
}

// ---- nnclr_sweep -----------------------------------------------------------------------------

struct SweepParams {
  const uint16_t* nnpl;     // [2][2n][D] the neighbours
  const uint16_t* ppl;      // [2][2N][D] p̂
  const float* lse;         // [2n] (bwd)
  float2* part;             // fwd: [splits][2n] (max, sumexp)
  float* slab;              // bwd: [splits][2N][D]
  int n, N, pos_offset, tiles, span_tiles;
  float inv_temp;
};

template <int D, bool BWD>
__global__ __launch_bounds__(256) void nnclr_sweep_kernel(SweepParams p) {
  constexpr int KS = D / 32;
  constexpr int TILE_B = TK * row_stride<D>();
  constexpr int BUF = 2 * TILE_B;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int h = lane >> 4;
  const int c = lane & 15;       // column of the MFMA tile = this lane's held row
  const int split = blockIdx.y;
  const int v = blockIdx.z;      // the neighbours' view; the predictions are of view 1 − v
  // held rows [hbase, hbase + hrows) of hpl, streamed rows [sbase, sbase + srows) of spl
  const uint16_t* hpl = BWD ? p.ppl : p.nnpl;
  const uint16_t* spl = BWD ? p.nnpl : p.ppl;
  const int hrows = BWD ? p.N : p.n, srows = BWD ? p.n : p.N;
  const int hbase = BWD ? (1 - v) * p.N : v * p.n, sbase = BWD ? v * p.n : (1 - v) * p.N;
  const size_t hplane = (size_t)2 * hrows * D, splane = (size_t)2 * srows * D;

  const int own = blockIdx.x * RB + wv * 16 + c;
  const int own_ld = own < hrows ? own : hrows - 1;   // a row past the end is computed on a copy and not written
  bf16x8 f_hi[KS], f_lo[KS];
  {
    const uint16_t* src = hpl + (size_t)(hbase + own_ld) * D;
    held_fragments<D>(src, src + hplane, h, f_hi, f_lo);
  }

  float run_m = -INFINITY, run_l = 0.f;
  // bwd accumulators: dp̂ᵀ tiles [d = 16q + 4h + r][row = c]
  f32x4 acc2[BWD ? D / 16 : 1];
#pragma unroll
  for (int q = 0; q < (BWD ? D / 16 : 1); ++q) acc2[q] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int t_begin = split * p.span_tiles;
  const int t_end = t_begin + p.span_tiles < p.tiles ? t_begin + p.span_tiles : p.tiles;
  const uint16_t* plane_hi = spl + (size_t)sbase * D;
  const uint16_t* plane_lo = plane_hi + splane;

  TileStage<D> st;
  st.init(tid);
  st.load(plane_hi, plane_lo, TK * t_begin, srows);
  st.commit(smem);
  for (int t = t_begin; t < t_end; ++t) {
    unsigned char* cur = smem + ((t - t_begin) & 1) * BUF;
    unsigned char* nxt = smem + ((t - t_begin + 1) & 1) * BUF;
    __syncthreads();
    const bool more = t + 1 < t_end;
    if (more) st.load(plane_hi, plane_lo, TK * (t + 1), srows);
    const unsigned char* lds_hi = cur;
    const unsigned char* lds_lo = cur + TILE_B;
    // this lane's streamed rows: j(k) = 32t + 16·(k / 4) + 4h + (k % 4)
    float row_lse[8];
    if constexpr (BWD) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int j = TK * t + 16 * (k >> 2) + 4 * h + (k & 3);
        row_lse[k] = p.lse[sbase + (j < srows ? j : srows - 1)];
      }
    }

    f32x4 acc[2];
    tile_product<D, BWD>(lds_hi, lds_lo, c, h, f_hi, f_lo, acc);

    if constexpr (!BWD) {
      float sv[8];
      float tmax = -INFINITY;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int j = TK * t + 16 * (k >> 2) + 4 * h + (k & 3);
        sv[k] = j < srows ? logit(acc[k >> 2][k & 3], p.inv_temp) : -INFINITY;
        tmax = fmaxf(tmax, sv[k]);
      }
      const float mn = fmaxf(run_m, tmax);
      const float ms = mn == -INFINITY ? 0.f : mn;   // a lane whose rows so far are all past the end
      float l = run_l * __expf(run_m - ms);
#pragma unroll
      for (int k = 0; k < 8; ++k) l += __expf(sv[k] - ms);
      run_m = mn;
      run_l = l;
    } else {
      // ---- Pᵀ in the accumulator layout, split into the hi/lo B fragments ----
      float pv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int j = TK * t + 16 * (k >> 2) + 4 * h + (k & 3);
        const float e = __expf(logit(acc[k >> 2][k & 3], p.inv_temp) - row_lse[k]) -
                        (j + p.pos_offset == own ? 1.f : 0.f);
        pv[k] = j < srows ? e : 0.f;
      }
      bf16x8 g_hi, g_lo;
      split8(pv, g_hi, g_lo);
      // ---- dp̂ᵀ[d][row] += Σ_j nn[j][d]·Pᵀ[j][row]; the A operand by transposed LDS reads ----
      const int qq = c >> 2, pp = c & 3;
#pragma unroll
      for (int q = 0; q < D / 16; ++q) {
        bf16x8 a2_hi, a2_lo;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const int off = t_off<D>(16 * tt + 4 * h + qq, (16 * q + 4 * pp) * 2);
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
    // the 4 lane groups that hold the same neighbour row, merged in a fixed order
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float m2 = __shfl_xor(run_m, off, 64);
      const float l2 = __shfl_xor(run_l, off, 64);
      lse_merge(run_m, run_l, m2, l2);
    }
    if (h == 0 && own < hrows) p.part[(size_t)split * 2 * p.n + hbase + own] = make_float2(run_m, run_l);
  } else {
    if (own < hrows) {
      float* dst = p.slab + ((size_t)split * 2 * p.N + hbase + own) * D + 4 * h;
#pragma unroll
      for (int q = 0; q < D / 16; ++q)
        *reinterpret_cast<float4*>(dst + 16 * q) = make_float4(acc2[q][0], acc2[q][1], acc2[q][2], acc2[q][3]);
    }
  }
}

// ---- nnclr_finish, nnclr_total ---------------------------------------------------------------

__global__ __launch_bounds__(256) void nnclr_finish_kernel(const float2* __restrict__ part, int splits,
                                                           const uint16_t* __restrict__ nnpl,
                                                           const uint16_t* __restrict__ ppl, int n, int N, int D,
                                                           int pos_offset, double inv_temp, float* __restrict__ lse,
                                                           double* __restrict__ term) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= 2 * n) return;
  const int v = row / n, i = row - v * n;
  float m = -INFINITY, l = 0.f;
  for (int sp = 0; sp < splits; ++sp) {
    const float2 x = part[(size_t)sp * 2 * n + row];
    lse_merge(m, l, x.x, x.y);
  }
  const float L = m + __logf(l);
  const uint16_t* a = nnpl + (size_t)row * D;
  const uint16_t* b = ppl + (size_t)((1 - v) * N + i + pos_offset) * D;
  const size_t ap = (size_t)2 * n * D, bp = (size_t)2 * N * D;
  double dot = 0.0;
  for (int d = lane; d < D; d += 64)
    dot += ((double)bf_value(a[d]) + (double)bf_value(a[ap + d])) * ((double)bf_value(b[d]) + (double)bf_value(b[bp + d]));
  dot = wave_sum_f64(dot);
  if (lane == 0) {
    lse[row] = L;
    term[row] = (double)L - dot * inv_temp;
  }
}

__global__ __launch_bounds__(256) void nnclr_total_kernel(const double* __restrict__ term, int rows, double rows_total,
                                                          float* __restrict__ loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256) s += term[i];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = 0.0;
  for (int t = 0; t < 256; ++t) s += red[t];
  loss[0] = (float)(s / rows_total);
}

// ---- nnclr_dp --------------------------------------------------------------------------------

// scale = 1/(2N·τ); rows = 2N
__global__ __launch_bounds__(256) void nnclr_dp_kernel(const float* __restrict__ slab, int splits,
                                                       const float* __restrict__ pin, const float* __restrict__ rp,
                                                       const float* __restrict__ g, int rows, int D, float scale,
                                                       float* __restrict__ dp) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float sc = g[0] * scale;
  const float rn = rp[row];
  float v[4], ph[4];
  double dot = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = lane + 64 * j;
    v[j] = 0.f;
    ph[j] = 0.f;
    if (d < D) {
      float a = slab[(size_t)row * D + d];
      for (int sp = 1; sp < splits; ++sp) a += slab[((size_t)sp * rows + row) * D + d];
      v[j] = a * sc;
      ph[j] = pin[(size_t)row * D + d] * rn;
      dot += (double)ph[j] * (double)v[j];
    }
  }
  const float dt = (float)wave_sum_f64(dot);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = lane + 64 * j;
    if (d < D) dp[(size_t)row * D + d] = (v[j] - ph[j] * dt) * rn;
  }
}

template <bool BWD>
hipError_t launch_sweep(const np::Plan& pl, const SweepParams& p, hipStream_t s) {
  const np::Cut& c = BWD ? pl.bwd : pl.fwd;
  const dim3 grid(c.blocks, c.splits, 2);
  switch (pl.d) {
    case 64: hipLaunchKernelGGL((nnclr_sweep_kernel<64, BWD>), grid, dim3(256), 0, s, p); break;
    case 128: hipLaunchKernelGGL((nnclr_sweep_kernel<128, BWD>), grid, dim3(256), 0, s, p); break;
    case 192: hipLaunchKernelGGL((nnclr_sweep_kernel<192, BWD>), grid, dim3(256), 0, s, p); break;
    case 256: hipLaunchKernelGGL((nnclr_sweep_kernel<256, BWD>), grid, dim3(256), 0, s, p); break;
    default: return hipErrorInvalidValue;
  }
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

bool pos(double x) { return x > 0.0 && x < 1e30; }

}  // namespace

bool nnclr_supported(long n, long N, long D, long K) { return np::supported(n, N, D, K); }

hipError_t launch_nnclr_prep(const float* x, int rows, int D, float* xhat, uint16_t* planes, float* rn,
                             hipStream_t s) {
  if (rows < 1 || D < np::kMinD || D > np::kMaxD || D % 64 != 0 || (long)rows * D >= (1L << 31) || x == nullptr ||
      planes == nullptr || ((uintptr_t)x & 7) != 0 || ((uintptr_t)xhat & 7) != 0 || ((uintptr_t)planes & 3) != 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(nnclr_prep_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, rows, D, xhat, planes, rn);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_nnclr_search(const uint16_t* zpl, const uint16_t* queue, int n, int D, int K, int* pair, int* idx,
                               float* sim, uint16_t* nnpl, hipStream_t s) {
  np::Plan pl;
  if (!np::make_plan(n, n, D, K, &pl) || zpl == nullptr || queue == nullptr || pair == nullptr || idx == nullptr ||
      sim == nullptr || nnpl == nullptr || !np::aligned16(zpl) || !np::aligned16(queue) || !np::aligned16(nnpl) ||
      ((uintptr_t)pair & 7) != 0)
    return hipErrorInvalidValue;
  SearchParams p = {};
  p.zpl = zpl; p.queue = queue; p.pair = reinterpret_cast<int2*>(pair);
  p.R = 2 * n; p.K = K; p.tiles = pl.search.tiles; p.span_tiles = pl.search.span_tiles;
  const dim3 grid(pl.search.blocks, pl.search.splits);
  switch (D) {
    case 64: hipLaunchKernelGGL(nnclr_search_kernel<64>, grid, dim3(256), 0, s, p); break;
    case 128: hipLaunchKernelGGL(nnclr_search_kernel<128>, grid, dim3(256), 0, s, p); break;
    case 192: hipLaunchKernelGGL(nnclr_search_kernel<192>, grid, dim3(256), 0, s, p); break;
    case 256: hipLaunchKernelGGL(nnclr_search_kernel<256>, grid, dim3(256), 0, s, p); break;
    default: return hipErrorInvalidValue;
  }
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(nnclr_pick_kernel, dim3((2 * n + 3) / 4), dim3(256), 0, s, (const int2*)p.pair, pl.search.splits,
                     2 * n, queue, K, D, idx, sim, nnpl);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_nnclr_fwd(const uint16_t* nnpl, const uint16_t* ppl, int n, int N, int D, double temp, int pos_offset,
                            float* part, float* lse, double* term, float* loss, hipStream_t s) {
  np::Plan pl;
  if (!np::make_plan(n, N, D, np::kMinK, &pl) || nnpl == nullptr || ppl == nullptr || part == nullptr ||
      lse == nullptr || term == nullptr || loss == nullptr || !pos(temp) || pos_offset < 0 ||
      (long)pos_offset + n > N || !np::aligned16(nnpl) || !np::aligned16(ppl) || !np::aligned16(part) ||
      ((uintptr_t)term & 7) != 0)
    return hipErrorInvalidValue;
  SweepParams p = {};
  p.nnpl = nnpl; p.ppl = ppl; p.part = reinterpret_cast<float2*>(part);
  p.n = n; p.N = N; p.pos_offset = pos_offset; p.tiles = pl.fwd.tiles; p.span_tiles = pl.fwd.span_tiles;
  p.inv_temp = (float)(1.0 / temp);
  hipError_t e = launch_sweep<false>(pl, p, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(nnclr_finish_kernel, dim3((2 * n + 3) / 4), dim3(256), 0, s, (const float2*)p.part, pl.fwd.splits,
                     nnpl, ppl, n, N, D, pos_offset, 1.0 / temp, lse, term);
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(nnclr_total_kernel, dim3(1), dim3(256), 0, s, (const double*)term, 2 * n, 2.0 * (double)N, loss);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_nnclr_bwd(const uint16_t* nnpl, const uint16_t* ppl, const float* pin, const float* rp,
                            const float* lse, const float* g, int n, int N, int D, double temp, int pos_offset,
                            float* slab, float* dp, hipStream_t s) {
  np::Plan pl;
  if (!np::make_plan(n, N, D, np::kMinK, &pl) || nnpl == nullptr || ppl == nullptr || pin == nullptr ||
      rp == nullptr || lse == nullptr || g == nullptr || slab == nullptr || dp == nullptr || !pos(temp) ||
      pos_offset < 0 || (long)pos_offset + n > N || !np::aligned16(nnpl) || !np::aligned16(ppl) ||
      !np::aligned16(slab))
    return hipErrorInvalidValue;
  SweepParams p = {};
  p.nnpl = nnpl; p.ppl = ppl; p.lse = lse; p.slab = slab;
  p.n = n; p.N = N; p.pos_offset = pos_offset; p.tiles = pl.bwd.tiles; p.span_tiles = pl.bwd.span_tiles;
  p.inv_temp = (float)(1.0 / temp);
  hipError_t e = launch_sweep<true>(pl, p, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(nnclr_dp_kernel, dim3((2 * N + 3) / 4), dim3(256), 0, s, (const float*)slab, pl.bwd.splits, pin, rp,
                     g, 2 * N, D, (float)(1.0 / (2.0 * (double)N * temp)), dp);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
