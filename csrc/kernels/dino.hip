// DINO loss for gfx950 (--method DINO), two global crops: the cross-entropy between the teacher's
// centred, sharpened softmax and the student's softmax over K prototypes (up to 131 072), with the
// backward to the student's projector outputs z and to the student's unnormalised prototype weights V.
// Neither [2N][K] logit matrix is ever written: both are formed tile by tile in MFMA accumulators, in
// the forward and again in both backward sweeps. Products are bf16x3 (hi·hi + hi·lo + lo·hi) on
// v_mfma_f32_16x16x32_bf16. fp32 in and out.
//
//   dino_prep      one wave per row of the four operands (student and teacher rows, student and teacher
//                  prototypes): Σx² in fp64, rn = 1 / max(‖x‖, 1e-12), x̂ = x·fp32(rn) split to bf16 hi / lo
//                  (bf16x3_stage.h's commit8) into planes [2][rows][D], the MFMA operands as they lie in
//                  memory. The sample planes pad each view to np rows (dino_plan.h) with zero rows.
//   dino_colsum    Σ_i ẑ_t,i as an fp64 D-vector, rows in a fixed order: the teacher logits' column mean
//                  is linear in it (dino_center), so no sweep carries a column reduction.
//   dino_sweep     <D, HELD, BWD>. A workgroup of 4 waves holds 64 rows of one side, student and teacher
//                  fragment together, as hi / lo B operands in registers, and streams the other side's
//                  student and teacher planes through two LDS buffers of swizzled 16-byte cells: tile
//                  t + 1 is loaded to registers before the MFMAs of tile t and committed after them, ONE
//                  barrier per tile. Both products Sᵀ = streamed_s·held_sᵀ and Tᵀ = streamed_t·held_tᵀ
//                  come from the same loop; a lane holds ONE held row (column c) and 4 or 8 streamed rows.
//                  HELD = rows, FWD: streams a prototype span; per lane the online (max_s, sum_s),
//                    (max_t, sum_t) and a = Σ exp((t − c)/τ_t − max_t)·s, rescaled when max_t moves;
//                    the 4 lane groups merged by shuffles, one 5-tuple per (split, row).
//                  HELD = rows, BWD: dS = exp(s/τ_s − lse_s) − exp((t − c)/τ_t − lse_t) in the
//                    accumulator layout, split to hi / lo and fed as the B operand of
//                    dẑ_sᵀ[d][row] += Ĉ_s,tileᵀ·dSᵀ, the A operand by transposed LDS reads of the staged
//                    student tile. One slab per split.
//                  HELD = prototypes, BWD: the roles exchanged. Holds 64 prototypes of both networks,
//                    streams the student rows of view 1 − v with the teacher rows of view v (the teacher
//                    tile index is shifted by one view), lse read along the streamed axis and c along the
//                    held one, dĈ_sᵀ[d][k] += ẑ_s,tileᵀ·dS. With one sample span the weight-norm backward
//                    dV_k = (dĈ_k − Ĉ_k(Ĉ_k·dĈ_k))/‖V_k‖ runs here from the accumulators; else slabs.
//                  A 16-row tile (D > 128) feeds the second product to v_mfma_f32_16x16x16_bf16.
//   dino_finish    one block: per row the split 5-tuples merged in split order, lse_s, lse_t saved (+inf
//                  for a pad row, which zeroes its dS), the row terms lse_s − a/(τ_s·sum_t) in fp64,
//                  thread t the rows ≡ t (mod 256) ascending, then the 256 partials in thread order.
//   dino_norm_bwd  one wave per row: v = g/(2N·τ_s)·Σ_split slab in split order, then
//                  (v − x̂(x̂·v))·rn with the dot in fp64: dz from the row slabs, dV from the prototype slabs.
//   dino_center    one wave per prototype: c ← m·c + (1 − m)·V_t,k·(Σ_i ẑ_t,i)/(‖V_t,k‖·2N), all in fp64.
//
// Determinism: no atomics, no cross-workgroup wait; both split counts are functions of the shape and
// every cross-split sum is added by a later launch in split order.
#include "bf16x3_stage.h"
#include "common.h"
#include "dino_plan.h"
#include "launchers.h"

using namespace sdx;

namespace {

namespace dp = sdx_dino;

constexpr int RB = dp::kRowBlock;
static_assert(RB == 64, "the sweep is written for 4 waves x 16 held rows");

enum Held { kRows = 0, kProtos = 1 };

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <int D>
constexpr int row_stride() {
  return D % 128 == 0 ? 2 * D : 2 * D + 16;
}

// byte offset of (row, byte of the bf16 row) in a staged plane image (moco.hip's layout: XOR-swizzled
// cells where a row is a multiple of 256 bytes, a 16-byte pad per row elsewhere)
template <int D>
__device__ __forceinline__ int q_off(int row, int byte) {
  if constexpr (D % 128 == 0) {
    const int sw = (row & 7) << 1;
    return row * (D * 2) + (((byte >> 4) ^ sw) << 4) + (byte & 15);
  } else {
    return row * (D * 2 + 16) + byte;
  }
}

// N floats -> the hi and lo fragment words (element j in the low half of word j / 2)
template <int W>
__device__ __forceinline__ void split_words(const float* x, uint32_t (&wh)[W], uint32_t (&wl)[W]) {
#pragma unroll
  for (int j = 0; j < W; ++j) {
    wh[j] = pack_bf2(x[2 * j], x[2 * j + 1]);
    const float h0 = __uint_as_float(wh[j] << 16), h1 = __uint_as_float(wh[j] & 0xffff0000u);
    wl[j] = pack_bf2(x[2 * j] - h0, x[2 * j + 1] - h1);
  }
}

// A staged tile is four images: student hi, student lo, teacher hi, teacher lo, each TK·D contiguous
// bf16 in memory. Thread tid moves the 16-byte cells tid, tid + 256, ... of every image, raw in
// registers between load() and commit().
template <int D, int TK>
struct TileStage {
  static constexpr int CELLS = TK * D / 8;
  static constexpr int CPT = (CELLS + 255) / 256;
  static constexpr int CPR = D / 8;
  static constexpr int IMG = TK * row_stride<D>();
  u32x4 raw[4][CPT];
  int off[CPT];

  static __device__ __forceinline__ bool mine(int i) { return CELLS % 256 == 0 || i * 256 + (int)threadIdx.x < CELLS; }

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int idx = i * 256 + threadIdx.x;
      off[i] = mine(i) ? q_off<D>(idx / CPR, 16 * (idx % CPR)) : 0;
    }
  }

  // ts, tt: the student and the teacher tile index; lo_off: elements from a hi plane to its lo plane
  __device__ __forceinline__ void load(const uint16_t* ps, const uint16_t* pt, size_t lo_off, int ts, int tt) {
    const uint16_t* bs = ps + (size_t)ts * TK * D;
    const uint16_t* bt = pt + (size_t)tt * TK * D;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      if (!mine(i)) continue;
      const int cell = i * 256 + threadIdx.x;
      raw[0][i] = reinterpret_cast<const u32x4*>(bs)[cell];
      raw[1][i] = reinterpret_cast<const u32x4*>(bs + lo_off)[cell];
      raw[2][i] = reinterpret_cast<const u32x4*>(bt)[cell];
      raw[3][i] = reinterpret_cast<const u32x4*>(bt + lo_off)[cell];
    }
  }

  __device__ __forceinline__ void commit(unsigned char* buf) const {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      if (!mine(i)) continue;
#pragma unroll
      for (int im = 0; im < 4; ++im) *reinterpret_cast<u32x4*>(buf + im * IMG + off[i]) = raw[im][i];
    }
  }
};

// ---- dino_prep -------------------------------------------------------------------------------

struct PrepJob {
  const float* x;      // [rows][D], the views stacked (n rows each)
  uint16_t* planes;    // [2][prows][D]
  float* rn;           // [rows] or nullptr
  double* rn64;        // [rows] or nullptr
  int n, np, prows;    // prows = views·np
};
struct PrepJobs {
  PrepJob j[4];
};

__global__ __launch_bounds__(256) void dino_prep_kernel(PrepJobs jobs, int D) {
  const PrepJob jb = jobs.j[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int pr = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pr >= jb.prows) return;
  const int view = pr / jb.np, i = pr - view * jb.np;
  unsigned char* hi = reinterpret_cast<unsigned char*>(jb.planes + (size_t)pr * D);
  unsigned char* lo = reinterpret_cast<unsigned char*>(jb.planes + ((size_t)jb.prows + pr) * D);
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (i >= jb.n) {   // a pad row: zero planes
    if (lane < D / 8) sdx_stage::commit8(v, hi, lo, 16 * lane);
    return;
  }
  const int row = view * jb.n + i;
  const float* src = jb.x + (size_t)row * D;
  double ss = 0.0;
  if (lane < D / 8) {
    const float4 a = reinterpret_cast<const float4*>(src)[2 * lane], b = reinterpret_cast<const float4*>(src)[2 * lane + 1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += (double)v[e] * (double)v[e];
  }
  ss = wave_sum_f64(ss);
  const double rn = 1.0 / fmax(sqrt(ss), 1e-12);
  const float rnf = (float)rn;
  if (lane < D / 8) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= rnf;
    sdx_stage::commit8(v, hi, lo, 16 * lane);
  }
  if (lane == 0) {
    if (jb.rn != nullptr) jb.rn[row] = rnf;
    if (jb.rn64 != nullptr) jb.rn64[row] = rn;
  }
}

// zsum[d] = Σ_r x[r][d]·rn64[r]: a workgroup owns 16 columns (D / 16 workgroups), 64 row groups of 16
// lanes, group g the rows ≡ g (mod 64) ascending, then the groups in order
__global__ __launch_bounds__(1024) void dino_colsum_kernel(const float* __restrict__ x, const double* __restrict__ rn64,
                                                           int rows, int D, double* __restrict__ zsum) {
  __shared__ double red[64][16];
  const int col = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int d = blockIdx.x * 16 + col;   // < D: the grid is D / 16
  double s = 0.0;
  for (int r = grp; r < rows; r += 64) s += (double)x[(size_t)r * D + d] * rn64[r];
  red[grp][col] = s;
  __syncthreads();
  if (grp != 0) return;
  s = 0.0;
  for (int g = 0; g < 64; ++g) s += red[g][col];
  zsum[d] = s;
}

// ---- dino_sweep ------------------------------------------------------------------------------

struct SweepParams {
  const uint16_t* held_s;   // planes [2][held_rows][D]
  const uint16_t* held_t;
  const uint16_t* strm_s;   // planes [2][strm_rows][D]
  const uint16_t* strm_t;
  const float* center;      // [K]
  const float* lse_s;       // [rp] (bwd), indexed by the student row
  const float* lse_t;       // [rp] (bwd), the lse of the teacher row that goes with that student row
  float* part;              // fwd: [5][splits][rp]
  float* slab;              // bwd: [splits][held_rows][D]
  const float* v;           // the epilogue of the prototype sweep: V_s [K][D], 1/‖V_s‖ [K], g [1], dV [K][D]
  const float* rv;
  const float* g;
  float* dv;
  int held_rows, strm_rows, np;
  int tiles, span_tiles;
  float its, itt, scale;    // 1/τ_s, 1/τ_t, 1/(2N·τ_s)
};

template <int D, int HELD, bool BWD>
__global__ __launch_bounds__(256) void dino_sweep_kernel(SweepParams p) {
  constexpr int TK = dp::tile_rows(D);
  constexpr int NT = TK / 16;                  // 16-row MFMA tiles per staged tile
  constexpr int NV = 4 * NT;                   // streamed rows per lane and tile
  constexpr int KS = D / 32;                   // MFMA k-steps over the feature dim
  constexpr int IMG = TK * row_stride<D>();    // one plane image
  constexpr int BUF = 4 * IMG;                 // student hi, lo, teacher hi, lo
  static_assert(2 * BUF <= 65536, "two staged tiles must fit the static LDS of a workgroup");
  static_assert(HELD == kRows || BWD, "the forward holds rows");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int h = lane >> 4;       // 16-lane group
  const int c = lane & 15;       // column of the MFMA tile = this lane's held row
  const int own = blockIdx.x * RB + wv * 16 + c;   // < held_rows: the grid covers whole row blocks
  const int split = blockIdx.y;
  SDX_DCHECK(own < p.held_rows);
  // the teacher row that goes with student row r is row (r + np) mod rp: the same sample, the other view
  int own_t = own;
  if constexpr (HELD == kRows) own_t = own + p.np >= p.held_rows ? own + p.np - p.held_rows : own + p.np;
  const size_t held_lo = (size_t)p.held_rows * D, strm_lo = (size_t)p.strm_rows * D;

  // ---- held fragments (B operands of both tile products) ----
  bf16x8 hs_hi[KS], hs_lo[KS], ht_hi[KS], ht_lo[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const size_t es = (size_t)own * D + 32 * s + 8 * h, et = (size_t)own_t * D + 32 * s + 8 * h;
    hs_hi[s] = *reinterpret_cast<const bf16x8*>(p.held_s + es);
    hs_lo[s] = *reinterpret_cast<const bf16x8*>(p.held_s + held_lo + es);
    ht_hi[s] = *reinterpret_cast<const bf16x8*>(p.held_t + et);
    ht_lo[s] = *reinterpret_cast<const bf16x8*>(p.held_t + held_lo + et);
  }

  // per held row: the saved lse pair (rows held) or the centre (prototypes held)
  float own_a = 0.f, own_b = 0.f;
  if constexpr (BWD && HELD == kRows) {
    own_a = p.lse_s[own];
    own_b = p.lse_t[own];
  }
  if constexpr (HELD == kProtos) own_a = p.center[own];

  float ms = -INFINITY, ls = 0.f, mt = -INFINITY, lt = 0.f, aa = 0.f;
  // bwd accumulators: the transposed gradient tiles [d = 16q + 4h + r][held row = c]
  f32x4 acc2[BWD ? D / 16 : 1];
#pragma unroll
  for (int q = 0; q < (BWD ? D / 16 : 1); ++q) acc2[q] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int t_begin = split * p.span_tiles;
  const int t_end = t_begin + p.span_tiles < p.tiles ? t_begin + p.span_tiles : p.tiles;
  // prototypes held: the teacher tile of the other view
  const int view_tiles = p.np / TK;
  auto teacher_tile = [&](int t) {
    if constexpr (HELD == kRows) return t;
    return t + view_tiles >= p.tiles ? t + view_tiles - p.tiles : t + view_tiles;
  };

  TileStage<D, TK> st;
  st.init();
  st.load(p.strm_s, p.strm_t, strm_lo, t_begin, teacher_tile(t_begin));
  st.commit(smem);
  for (int t = t_begin; t < t_end; ++t) {
    unsigned char* cur = smem + ((t - t_begin) & 1) * BUF;
    unsigned char* nxt = smem + ((t - t_begin + 1) & 1) * BUF;
    // tile t is visible, and every wave is done reading the buffer that tile t + 1 goes to
    __syncthreads();
    const bool more = t + 1 < t_end;
    if (more) st.load(p.strm_s, p.strm_t, strm_lo, t + 1, teacher_tile(t + 1));   // in flight under the MFMAs

    // per streamed row (4 consecutive ones per MFMA tile): the centre (rows held) or the lse pair
    f32x4 va[NT], vb[NT];
#pragma unroll
    for (int t2 = 0; t2 < NT; ++t2) {
      const int r0 = t * TK + 16 * t2 + 4 * h;
      if constexpr (HELD == kRows) {
        va[t2] = *reinterpret_cast<const f32x4*>(p.center + r0);
        vb[t2] = va[t2];
      } else {
        va[t2] = *reinterpret_cast<const f32x4*>(p.lse_s + r0);
        vb[t2] = *reinterpret_cast<const f32x4*>(p.lse_t + r0);
      }
    }

    // ---- Sᵀ and Tᵀ tiles: acc[t2][r] = <streamed[TK·t + 16·t2 + 4h + r], held[c]> ----
    f32x4 as[NT], at[NT];
#pragma unroll
    for (int t2 = 0; t2 < NT; ++t2) {
      as[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
      at[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int off = q_off<D>(16 * t2 + c, (32 * s + 8 * h) * 2);
        const bf16x8 s_hi = *reinterpret_cast<const bf16x8*>(cur + off);
        const bf16x8 s_lo = *reinterpret_cast<const bf16x8*>(cur + IMG + off);
        const bf16x8 t_hi = *reinterpret_cast<const bf16x8*>(cur + 2 * IMG + off);
        const bf16x8 t_lo = *reinterpret_cast<const bf16x8*>(cur + 3 * IMG + off);
        as[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(s_hi, hs_hi[s], as[t2], 0, 0, 0);
        at[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(t_hi, ht_hi[s], at[t2], 0, 0, 0);
        as[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(s_hi, hs_lo[s], as[t2], 0, 0, 0);
        at[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(t_hi, ht_lo[s], at[t2], 0, 0, 0);
        as[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(s_lo, hs_hi[s], as[t2], 0, 0, 0);
        at[t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(t_lo, ht_hi[s], at[t2], 0, 0, 0);
      }
    }

    if constexpr (!BWD) {
      float xs[NV], xt[NV];
      float smax = -INFINITY, tmax = -INFINITY;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        xs[k] = as[k >> 2][k & 3] * p.its;
        xt[k] = (at[k >> 2][k & 3] - va[k >> 2][k & 3]) * p.itt;
        smax = fmaxf(smax, xs[k]);
        tmax = fmaxf(tmax, xt[k]);
      }
      const float ns = fmaxf(ms, smax), nt = fmaxf(mt, tmax);
      const float rt = __expf(mt - nt);     // the first tile: 0·exp(−inf) = 0
      float l = ls * __expf(ms - ns), l2 = lt * rt, a = aa * rt;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        l += __expf(xs[k] - ns);
        const float e = __expf(xt[k] - nt);
        l2 += e;
        a = fmaf(e, as[k >> 2][k & 3], a);
      }
      ms = ns; ls = l; mt = nt; lt = l2; aa = a;
    } else {
      // ---- dS in the accumulator layout, split into the hi / lo B fragments ----
      float pv[NV];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const float s = as[k >> 2][k & 3], tv = at[k >> 2][k & 3];
        const float Ls = HELD == kRows ? own_a : va[k >> 2][k & 3];
        const float Lt = HELD == kRows ? own_b : vb[k >> 2][k & 3];
        const float cc = HELD == kRows ? va[k >> 2][k & 3] : own_a;
        pv[k] = __expf(s * p.its - Ls) - __expf((tv - cc) * p.itt - Lt);
      }
      uint32_t wh[NV / 2], wl[NV / 2];
      split_words<NV / 2>(pv, wh, wl);
      // ---- grad ᵀ[d][held] += Σ_j streamed_s[j][d]·dSᵀ[j][held]; the A operand by transposed LDS reads ----
      const int qq = c >> 2, pp = c & 3;
      if constexpr (NT == 2) {
        const bf16x8 g_hi = __builtin_bit_cast(bf16x8, (u32x4){wh[0], wh[1], wh[2], wh[3]});
        const bf16x8 g_lo = __builtin_bit_cast(bf16x8, (u32x4){wl[0], wl[1], wl[2], wl[3]});
#pragma unroll
        for (int q = 0; q < D / 16; ++q) {
          bf16x8 a2_hi, a2_lo;
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) {
            const int off = q_off<D>(16 * tt + 4 * h + qq, (16 * q + 4 * pp) * 2);
            const bf16x4 th = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(cur + off));
            const bf16x4 tl = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(cur + IMG + off));
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
      } else {
        // one 16-row tile: k = 16, a lane's 4 dS values are the B fragment of a 16x16x16
        const bf16x4 g_hi = __builtin_bit_cast(bf16x4, (u32x2){wh[0], wh[1]});
        const bf16x4 g_lo = __builtin_bit_cast(bf16x4, (u32x2){wl[0], wl[1]});
#pragma unroll
        for (int q = 0; q < D / 16; ++q) {
          const int off = q_off<D>(4 * h + qq, (16 * q + 4 * pp) * 2);
          const bf16x4 th = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(cur + off));
          const bf16x4 tl = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(cur + IMG + off));
          acc2[q] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(th, g_hi, acc2[q], 0, 0, 0);
          acc2[q] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(th, g_lo, acc2[q], 0, 0, 0);
          acc2[q] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(tl, g_hi, acc2[q], 0, 0, 0);
        }
      }
    }
    if (more) st.commit(nxt);
  }

  if constexpr (!BWD) {
    // the 4 lane groups that hold the same row, merged in a fixed order
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float ms2 = __shfl_xor(ms, off, 64), ls2 = __shfl_xor(ls, off, 64);
      const float mt2 = __shfl_xor(mt, off, 64), lt2 = __shfl_xor(lt, off, 64), aa2 = __shfl_xor(aa, off, 64);
      const float ns = fmaxf(ms, ms2), nt = fmaxf(mt, mt2);
      ls = ls * __expf(ms - ns) + ls2 * __expf(ms2 - ns);
      const float r1 = __expf(mt - nt), r2 = __expf(mt2 - nt);
      lt = lt * r1 + lt2 * r2;
      aa = aa * r1 + aa2 * r2;
      ms = ns;
      mt = nt;
    }
    if (h == 0) {
      const size_t plane = (size_t)gridDim.y * p.held_rows;
      float* dst = p.part + (size_t)split * p.held_rows + own;
      dst[0] = ms; dst[plane] = ls; dst[2 * plane] = mt; dst[3 * plane] = lt; dst[4 * plane] = aa;
    }
  } else if (HELD == kProtos && p.dv != nullptr) {
    // one sample span: the weight-norm backward of this prototype row, straight from the accumulators
    const float sc = p.g[0] * p.scale, rn = p.rv[own];
    const float* vrow = p.v + (size_t)own * D + 4 * h;
    double dot = 0.0;
#pragma unroll
    for (int q = 0; q < D / 16; ++q) {
      const float4 x = *reinterpret_cast<const float4*>(vrow + 16 * q);
      acc2[q] = f32x4{acc2[q][0] * sc, acc2[q][1] * sc, acc2[q][2] * sc, acc2[q][3] * sc};
      dot += (double)(x.x * rn) * (double)acc2[q][0] + (double)(x.y * rn) * (double)acc2[q][1] +
             (double)(x.z * rn) * (double)acc2[q][2] + (double)(x.w * rn) * (double)acc2[q][3];
    }
    dot += __shfl_xor(dot, 16, 64);
    dot += __shfl_xor(dot, 32, 64);
    const float dt = (float)dot;
    float* dst = p.dv + (size_t)own * D + 4 * h;
#pragma unroll
    for (int q = 0; q < D / 16; ++q) {
      const float4 x = *reinterpret_cast<const float4*>(vrow + 16 * q);
      *reinterpret_cast<float4*>(dst + 16 * q) =
          make_float4((acc2[q][0] - x.x * rn * dt) * rn, (acc2[q][1] - x.y * rn * dt) * rn,
                      (acc2[q][2] - x.z * rn * dt) * rn, (acc2[q][3] - x.w * rn * dt) * rn);
    }
  } else {
    float* dst = p.slab + ((size_t)split * p.held_rows + own) * D + 4 * h;
#pragma unroll
    for (int q = 0; q < D / 16; ++q)
      *reinterpret_cast<float4*>(dst + 16 * q) = make_float4(acc2[q][0], acc2[q][1], acc2[q][2], acc2[q][3]);
  }
}

// ---- dino_finish -----------------------------------------------------------------------------

__global__ __launch_bounds__(256) void dino_finish_kernel(const float* __restrict__ part, int rp, int np, int n,
                                                          int splits, float its, double n_total,
                                                          float* __restrict__ lse_s, float* __restrict__ lse_t,
                                                          float* __restrict__ loss) {
  __shared__ double red[256];
  const size_t plane = (size_t)splits * rp;
  double s = 0.0;
  for (int r = threadIdx.x; r < rp; r += 256) {
    if (r % np >= n) {   // a pad row: exp(x − inf) = 0 in both backward sweeps
      lse_s[r] = INFINITY;
      lse_t[r] = INFINITY;
      continue;
    }
    float ms = -INFINITY, ls = 0.f, mt = -INFINITY, lt = 0.f, a = 0.f;
    for (int sp = 0; sp < splits; ++sp) {
      const float* src = part + (size_t)sp * rp + r;
      const float ms2 = src[0], ls2 = src[plane], mt2 = src[2 * plane], lt2 = src[3 * plane], a2 = src[4 * plane];
      const float ns = fmaxf(ms, ms2), nt = fmaxf(mt, mt2);
      ls = ls * __expf(ms - ns) + ls2 * __expf(ms2 - ns);
      const float r1 = __expf(mt - nt), r2 = __expf(mt2 - nt);
      lt = lt * r1 + lt2 * r2;
      a = a * r1 + a2 * r2;
      ms = ns;
      mt = nt;
    }
    const float Ls = ms + logf(ls);
    lse_s[r] = Ls;
    lse_t[r] = mt + logf(lt);
    s += (double)Ls - (double)its * (double)a / (double)lt;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = 0.0;
  for (int t = 0; t < 256; ++t) s += red[t];
  loss[0] = (float)(s / (2.0 * n_total));
}

// ---- dino_norm_bwd ---------------------------------------------------------------------------

// out[r] = (v − x̂(x̂·v))·rn[r], v = g·scale·Σ_split slab[split][pad(r)], x̂ = x[r]·rn[r]. pad(r) is
// the row's index in the padded planes: r for r < n, else r − n + np.
__global__ __launch_bounds__(256) void dino_norm_bwd_kernel(const float* __restrict__ slab, int splits, int slab_rows,
                                                            const float* __restrict__ x, const float* __restrict__ rnv,
                                                            const float* __restrict__ g, float scale, int rows, int n,
                                                            int np, int D, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int pr = row < n ? row : row - n + np;
  const float sc = g[0] * scale, rn = rnv[row];
  float v[4], xh[4];
  double dot = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = lane + 64 * j;
    v[j] = 0.f;
    xh[j] = 0.f;
    if (d < D) {
      float a = slab[(size_t)pr * D + d];
      for (int sp = 1; sp < splits; ++sp) a += slab[((size_t)sp * slab_rows + pr) * D + d];
      v[j] = a * sc;
      xh[j] = x[(size_t)row * D + d] * rn;
      dot += (double)xh[j] * (double)v[j];
    }
  }
  const float dt = (float)wave_sum_f64(dot);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = lane + 64 * j;
    if (d < D) out[(size_t)row * D + d] = (v[j] - xh[j] * dt) * rn;
  }
}

// ---- dino_center -----------------------------------------------------------------------------

__global__ __launch_bounds__(256) void dino_center_kernel(const float* __restrict__ vt, const double* __restrict__ zsum,
                                                          const float* __restrict__ cin, int K, int D, double m,
                                                          double rows_total, float* __restrict__ cout) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= K) return;
  double ss = 0.0, dt = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double x = (double)vt[(size_t)k * D + d];
    ss += x * x;
    dt += x * zsum[d];
  }
  ss = wave_sum_f64(ss);
  dt = wave_sum_f64(dt);
  if (lane == 0) cout[k] = (float)(m * (double)cin[k] + (1.0 - m) * (dt / fmax(sqrt(ss), 1e-12) / rows_total));
}

template <int HELD, bool BWD>
hipError_t launch_sweep(int d, dim3 grid, const SweepParams& p, hipStream_t s) {
  switch (d) {
    case 64: hipLaunchKernelGGL((dino_sweep_kernel<64, HELD, BWD>), grid, dim3(256), 0, s, p); break;
    case 128: hipLaunchKernelGGL((dino_sweep_kernel<128, HELD, BWD>), grid, dim3(256), 0, s, p); break;
    case 192: hipLaunchKernelGGL((dino_sweep_kernel<192, HELD, BWD>), grid, dim3(256), 0, s, p); break;
    case 256: hipLaunchKernelGGL((dino_sweep_kernel<256, HELD, BWD>), grid, dim3(256), 0, s, p); break;
    default: return hipErrorInvalidValue;
  }
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

bool pos(double x) { return x > 0.0 && x < 1e30; }

}  // namespace

bool dino_supported(long n, long D, long K) { return dp::supported(n, D, K); }

hipError_t launch_dino_prep(const float* zs, const float* zt, const float* vs, const float* vt, int n, int D, int K,
                            uint16_t* zs_pl, uint16_t* zt_pl, uint16_t* cs_pl, uint16_t* ct_pl, float* rzs, float* rvs,
                            double* rzt64, double* zsum, hipStream_t s) {
  dp::Plan pl;
  if (!dp::make_plan(n, D, K, &pl) || zs == nullptr || zt == nullptr || vs == nullptr || vt == nullptr ||
      zs_pl == nullptr || zt_pl == nullptr || cs_pl == nullptr || ct_pl == nullptr || rzs == nullptr ||
      rvs == nullptr || rzt64 == nullptr || zsum == nullptr || !dp::aligned16(zs) || !dp::aligned16(zt) ||
      !dp::aligned16(vs) || !dp::aligned16(vt) || !dp::aligned16(zs_pl) || !dp::aligned16(zt_pl) ||
      !dp::aligned16(cs_pl) || !dp::aligned16(ct_pl))
    return hipErrorInvalidValue;
  PrepJobs jobs;
  jobs.j[0] = PrepJob{zs, zs_pl, rzs, nullptr, n, pl.np, pl.rp};
  jobs.j[1] = PrepJob{zt, zt_pl, nullptr, rzt64, n, pl.np, pl.rp};
  jobs.j[2] = PrepJob{vs, cs_pl, rvs, nullptr, K, K, K};
  jobs.j[3] = PrepJob{vt, ct_pl, nullptr, nullptr, K, K, K};
  const int most = pl.rp > K ? pl.rp : K;
  hipLaunchKernelGGL(dino_prep_kernel, dim3((most + 3) / 4, 4), dim3(256), 0, s, jobs, D);
  SDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(dino_colsum_kernel, dim3(D / 16), dim3(1024), 0, s, zt, (const double*)rzt64, 2 * n, D, zsum);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_dino_fwd(const uint16_t* zs_pl, const uint16_t* zt_pl, const uint16_t* cs_pl, const uint16_t* ct_pl,
                           const float* center, int n, int D, int K, double temp_s, double temp_t, double n_total,
                           float* part, float* lse_s, float* lse_t, float* loss, hipStream_t s) {
  dp::Plan pl;
  if (!dp::make_plan(n, D, K, &pl) || zs_pl == nullptr || zt_pl == nullptr || cs_pl == nullptr || ct_pl == nullptr ||
      center == nullptr || part == nullptr || lse_s == nullptr || lse_t == nullptr || loss == nullptr ||
      !pos(temp_s) || !pos(temp_t) || !(n_total >= n) || !dp::aligned16(zs_pl) || !dp::aligned16(zt_pl) ||
      !dp::aligned16(cs_pl) || !dp::aligned16(ct_pl) || !dp::aligned16(center))
    return hipErrorInvalidValue;
  SweepParams p = {};
  p.held_s = zs_pl; p.held_t = zt_pl; p.strm_s = cs_pl; p.strm_t = ct_pl; p.center = center; p.part = part;
  p.held_rows = pl.rp; p.strm_rows = K; p.np = pl.np; p.tiles = pl.k_tiles; p.span_tiles = pl.k_span;
  p.its = (float)(1.0 / temp_s); p.itt = (float)(1.0 / temp_t);
  hipError_t e = launch_sweep<kRows, false>(D, dim3(pl.row_blocks, pl.k_splits), p, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dino_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)part, pl.rp, pl.np, n, pl.k_splits,
                     p.its, n_total, lse_s, lse_t, loss);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_dino_bwd(const float* zs, const float* vs, const uint16_t* zs_pl, const uint16_t* zt_pl,
                           const uint16_t* cs_pl, const uint16_t* ct_pl, const float* rzs, const float* rvs,
                           const float* center, const float* lse_s, const float* lse_t, const float* g, int n, int D,
                           int K, double temp_s, double temp_t, double n_total, float* zslab, float* vslab, float* dz,
                           float* dv, hipStream_t s) {
  dp::Plan pl;
  if (!dp::make_plan(n, D, K, &pl) || zs == nullptr || vs == nullptr || zs_pl == nullptr || zt_pl == nullptr ||
      cs_pl == nullptr || ct_pl == nullptr || rzs == nullptr || rvs == nullptr || center == nullptr ||
      lse_s == nullptr || lse_t == nullptr || g == nullptr || zslab == nullptr || dz == nullptr || !pos(temp_s) ||
      !pos(temp_t) || !(n_total >= n) || (dv != nullptr && pl.r_splits > 1 && vslab == nullptr) ||
      !dp::aligned16(zs_pl) || !dp::aligned16(zt_pl) || !dp::aligned16(cs_pl) || !dp::aligned16(ct_pl) ||
      !dp::aligned16(center) || !dp::aligned16(lse_s) || !dp::aligned16(lse_t) || !dp::aligned16(zslab) ||
      !dp::aligned16(vslab) || !dp::aligned16(vs) || !dp::aligned16(dv))
    return hipErrorInvalidValue;
  SweepParams p = {};
  p.center = center; p.lse_s = lse_s; p.lse_t = lse_t; p.np = pl.np;
  p.its = (float)(1.0 / temp_s); p.itt = (float)(1.0 / temp_t); p.scale = (float)(1.0 / (2.0 * n_total * temp_s));
  SweepParams pr = p;
  pr.held_s = zs_pl; pr.held_t = zt_pl; pr.strm_s = cs_pl; pr.strm_t = ct_pl; pr.slab = zslab;
  pr.held_rows = pl.rp; pr.strm_rows = K; pr.tiles = pl.k_tiles; pr.span_tiles = pl.k_span;
  hipError_t e = launch_sweep<kRows, true>(D, dim3(pl.row_blocks, pl.k_splits), pr, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dino_norm_bwd_kernel, dim3((2 * n + 3) / 4), dim3(256), 0, s, (const float*)zslab, pl.k_splits,
                     pl.rp, zs, rzs, g, p.scale, 2 * n, n, pl.np, D, dz);
  SDX_LAUNCH_CHECK();
  if (dv == nullptr) return hipSuccess;   // the prototypes are frozen: no weight gradient this step
  SweepParams pk = p;
  pk.held_s = cs_pl; pk.held_t = ct_pl; pk.strm_s = zs_pl; pk.strm_t = zt_pl;
  pk.held_rows = K; pk.strm_rows = pl.rp; pk.tiles = pl.r_tiles; pk.span_tiles = pl.r_span;
  if (pl.r_splits == 1) {
    pk.v = vs; pk.rv = rvs; pk.g = g; pk.dv = dv;
  } else {
    pk.slab = vslab;
  }
  e = launch_sweep<kProtos, true>(D, dim3(pl.proto_blocks, pl.r_splits), pk, s);
  if (e != hipSuccess) return e;
  if (pl.r_splits > 1) {
    hipLaunchKernelGGL(dino_norm_bwd_kernel, dim3((K + 3) / 4), dim3(256), 0, s, (const float*)vslab, pl.r_splits, K,
                       vs, rvs, g, p.scale, K, K, K, D, dv);
    SDX_LAUNCH_CHECK();
  }
  return hipSuccess;
}

hipError_t launch_dino_center(const float* vt, const double* zsum, const float* center, int K, int D, double m,
                              double rows_total, float* out, hipStream_t s) {
  if (!dp::supported(1, D, K) || vt == nullptr || zsum == nullptr || center == nullptr || out == nullptr ||
      !(m >= 0.0 && m <= 1.0) || !(rows_total >= 1.0))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(dino_center_kernel, dim3((K + 3) / 4), dim3(256), 0, s, vt, zsum, center, K, D, m, rows_total, out);
  SDX_LAUNCH_CHECK();
  return hipSuccess;
}
