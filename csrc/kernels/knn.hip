// Weighted k-NN evaluation for gfx950: per-query top-k of the cosine-similarity matrix
// Q·Bᵀ without ever writing the Nq x Nb matrix, and the exp(sim/T) class vote.
//
//   knn_topk   grid = (64-query tiles) x (S bank splits). A workgroup (4 waves) owns 64
//              queries, one query per accumulator lane column of its wave (the S^T = bank·qᵀ
//              tile form of supcon.hip's forward), and streams its bank split through LDS
//              in 64-row tiles. The feature dimension goes through LDS in 64-column chunks
//              (queries and bank rows alike, as bf16 hi/lo images in the XOR-swizzled row
//              layout of supcon.hip), so D up to 2048 needs no more registers than D = 64.
//              The next chunk's global loads are in flight while the MFMAs of the current
//              one run. Every query keeps its k best (similarity, index) pairs in LDS as a
//              binary heap with the worst kept pair at the root: the root is the admission
//              threshold, a candidate that beats it replaces it and sifts down. The four
//              16-lane groups of a wave hold different bank rows of the same 16 queries and
//              take turns; inside a turn the 16 heaps advance in parallel, one lane each.
//              At the end every heap is rank-sorted and written to its (split, query) slab.
//   knn_merge  one wave per query: the S sorted lists merge by rank (own position + a binary
//              search in every other list); ranks < k are written to sims / idx.
//   knn_vote   one wave per query: scores[c] = Σ_{neighbours of class c} exp(sim/T), fp32, in
//              list order; with labels, hits@1/@5 by the rank rule of linear_ce.hip
//              (#{c : score_c > score_label} < kk), summed over queries in fixed order.
//
// Order everywhere: similarity descending, then bank index ascending — a total order, so the
// selected set, and with it the output, depends neither on the split count nor on the order
// in which candidates arrive. One (query, bank row) similarity is accumulated in the same K
// order wherever the row sits (chunk ascending, hi·hi, hi·lo, lo·hi per 32 columns).
// No floating-point atomics anywhere.
//
// Precision: fp32 inputs split into bf16 hi + lo, three v_mfma_f32_16x16x32_bf16 per
// product: error <= 3·2^-18·Σ|q_i b_i| + D·2^-24 for unit rows.
#include <limits.h>

#include "common.h"
#include "knn_plan.h"
#include "launchers.h"

using namespace sdx;

namespace {

constexpr int QT = sdx_knn::kQueryTile;   // 64 queries per workgroup
constexpr int BT = sdx_knn::kBankTile;    // 64 bank rows per tile
constexpr int KC = 64;                    // feature columns per staged chunk
constexpr int ROW_B = KC * 2;             // bytes of one staged bf16 row
constexpr int IMG_B = 64 * ROW_B;         // one 64-row bf16 image (8 KiB)

struct KnnParams {
  const float* q;      // [nq][D]
  const float* bank;   // [nb][D]
  float* out_s;        // [n_split][nq][k]
  int* out_i;          // [n_split][nq][k]
  int nq, nb, D, k, rows_per_split, n_split;
};

// 128-B rows of eight 16-B chunks, chunk index XOR-swizzled by the row: the ds_read_b128 of
// the tile product (16 rows, one chunk column) and the staging ds_write_b128 (8 lanes = the
// 8 chunks of one row) both spread over all banks
__device__ __forceinline__ int sw_off(int row, int chunk) { return row * ROW_B + ((chunk ^ (row & 7)) << 4); }

// (s, i) ranks before (t, j): higher similarity, then lower bank index
__device__ __forceinline__ bool better(float s, int i, float t, int j) { return s > t || (s == t && i < j); }

template <int KCAP>
__global__ __launch_bounds__(256) void knn_topk_kernel(KnnParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[4 * IMG_B];   // q hi, q lo, bank hi, bank lo
  __shared__ float l_sim[QT * KCAP];
  __shared__ int l_idx[QT * KCAP];
  unsigned char* q_hi = stage;
  unsigned char* q_lo = stage + IMG_B;
  unsigned char* b_hi = stage + 2 * IMG_B;
  unsigned char* b_lo = stage + 3 * IMG_B;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int h = lane >> 4;   // 16-lane group
  const int c = lane & 15;   // accumulator column = query of this lane within the wave
  const int D = p.D, k = p.k;
  const int q0 = blockIdx.x * QT;
  const int b_begin = blockIdx.y * p.rows_per_split;
  int b_end = b_begin + p.rows_per_split;
  if (b_end > p.nb) b_end = p.nb;

  float* my_s = l_sim + (wv * 16) * KCAP;   // the 16 lists of this wave
  int* my_i = l_idx + (wv * 16) * KCAP;
  for (int e = lane; e < 16 * KCAP; e += 64) {
    my_s[e] = -INFINITY;
    my_i[e] = INT_MAX;
  }

  // staging: thread = one 8-float chunk (sk) of rows sr and sr + 32 of each operand
  const int sr = tid >> 3, sk = tid & 7;
  float4 pq[2][2], pb[2][2];
  auto issue_loads = [&](int b0, int kc) {
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int row = ps * 32 + sr;
      int qrow = q0 + row;
      if (qrow > p.nq - 1) qrow = p.nq - 1;
      const float4* qs = reinterpret_cast<const float4*>(p.q + (size_t)qrow * D + kc * KC + sk * 8);
      pq[ps][0] = qs[0];
      pq[ps][1] = qs[1];
      const int brow = b0 + row;
      if (brow < b_end) {
        SDX_DCHECK(brow >= 0 && brow < p.nb);
        const float4* bs = reinterpret_cast<const float4*>(p.bank + (size_t)brow * D + kc * KC + sk * 8);
        pb[ps][0] = bs[0];
        pb[ps][1] = bs[1];
      } else {
        pb[ps][0] = make_float4(0.f, 0.f, 0.f, 0.f);
        pb[ps][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  auto commit_one = [&](const float4 v0, const float4 v1, unsigned char* hi_img, unsigned char* lo_img, int off) {
    // RNE hi, then RNE of the exact remainder: two packed conversions per pair of floats
    const float xs[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    uint32_t wh[4], wl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wh[j] = pack_bf2(xs[2 * j], xs[2 * j + 1]);
      const float h0 = __uint_as_float(wh[j] << 16), h1 = __uint_as_float(wh[j] & 0xffff0000u);
      wl[j] = pack_bf2(xs[2 * j] - h0, xs[2 * j + 1] - h1);
    }
    const uint4 vh = make_uint4(wh[0], wh[1], wh[2], wh[3]);
    const uint4 vl = make_uint4(wl[0], wl[1], wl[2], wl[3]);
    *reinterpret_cast<uint4*>(hi_img + off) = vh;
    *reinterpret_cast<uint4*>(lo_img + off) = vl;
  };

  const int n_chunk = D / KC;

  if (b_begin < b_end) issue_loads(b_begin, 0);
  for (int b0 = b_begin; b0 < b_end; b0 += BT) {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < n_chunk; ++kc) {
#pragma unroll
      for (int ps = 0; ps < 2; ++ps) {
        const int off = sw_off(ps * 32 + sr, sk);
        commit_one(pq[ps][0], pq[ps][1], q_hi, q_lo, off);
        commit_one(pb[ps][0], pb[ps][1], b_hi, b_lo, off);
      }
      __syncthreads();
      {   // the next chunk's loads fly under this chunk's MFMAs
        int nkc = kc + 1, nb0 = b0;
        if (nkc == n_chunk) { nkc = 0; nb0 += BT; }
        if (nb0 < b_end) issue_loads(nb0, nkc);
      }
      // S^T tiles: acc[t][r] = <bank[b0 + 16t + 4h + r], query[q0 + 16wv + c]>
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int qoff = sw_off(wv * 16 + c, 4 * s + h);
        const bf16x8 o_hi = *reinterpret_cast<const bf16x8*>(q_hi + qoff);
        const bf16x8 o_lo = *reinterpret_cast<const bf16x8*>(q_lo + qoff);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int boff = sw_off(16 * t + c, 4 * s + h);
          const bf16x8 a_hi = *reinterpret_cast<const bf16x8*>(b_hi + boff);
          const bf16x8 a_lo = *reinterpret_cast<const bf16x8*>(b_lo + boff);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, o_hi, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, o_lo, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, o_hi, acc[t], 0, 0, 0);
        }
      }
      __syncthreads();
    }

    // ---- selection: the heaps of this wave's 16 queries are touched by this wave only. Heap
    // of query c: slot p at my_[p * 16 + c] (the 16 lanes of a group read one slot of 16 heaps
    // from 16 consecutive banks), the worst kept entry at the root. A candidate that beats the
    // root replaces it and sifts down. The four 16-lane groups hold different bank rows of the
    // same 16 queries, so they take turns; inside a turn 16 heaps advance in parallel. ----
    float* ls = my_s + c;
    int* li = my_i + c;
    bool any = false;
    {
      const float rs = ls[0];
      const int ri = li[0];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int bi = b0 + 16 * t + 4 * h + r;
          any = any || (bi < b_end && better(acc[t][r], bi, rs, ri));
        }
    }
    if (__ballot(any) != 0ull) {
      for (int hh = 0; hh < 4; ++hh) {
        if (h == hh && any) {
          float rs = ls[0];
          int ri = li[0];
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int bi = b0 + 16 * t + 4 * h + r;
              const float s = acc[t][r];
              if (bi < b_end && better(s, bi, rs, ri)) {
                int pos = 0;
                while (true) {
                  const int l = 2 * pos + 1;
                  if (l >= k) break;
                  float cs = ls[l * 16];
                  int ci = li[l * 16];
                  int cp = l;
                  if (l + 1 < k) {   // the worse of the two children
                    const float s2 = ls[(l + 1) * 16];
                    const int i2 = li[(l + 1) * 16];
                    if (better(cs, ci, s2, i2)) { cs = s2; ci = i2; cp = l + 1; }
                  }
                  if (!better(s, bi, cs, ci)) break;
                  ls[pos * 16] = cs;
                  li[pos * 16] = ci;
                  pos = cp;
                }
                ls[pos * 16] = s;
                li[pos * 16] = bi;
                rs = ls[0];
                ri = li[0];
              }
            }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }

  // ---- rank-sort every list and write it to this split's slab ----
  __builtin_amdgcn_wave_barrier();
  for (int cc = 0; cc < 16; ++cc) {
    const int qrow = q0 + wv * 16 + cc;
    if (qrow >= p.nq) break;
    const float* cls = my_s + cc;
    const int* cli = my_i + cc;
    float* os = p.out_s + ((size_t)blockIdx.y * p.nq + qrow) * k;
    int* oi = p.out_i + ((size_t)blockIdx.y * p.nq + qrow) * k;
    for (int e = lane; e < k; e += 64) {
      const float s = cls[e * 16];
      const int i = cli[e * 16];
      int rank = 0;
      for (int j = 0; j < k; ++j) {
        const float t = cls[j * 16];
        const int u = cli[j * 16];
        rank += (better(t, u, s, i) || (t == s && u == i && j < e)) ? 1 : 0;
      }
      SDX_DCHECK(rank >= 0 && rank < k);
      os[rank] = s;
      oi[rank] = i;
    }
  }
}

// One wave per query: merge the S sorted lists of a query by rank.
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ slab_s,
                                                        const int* __restrict__ slab_i, int nq, int k, int n_split,
                                                        float* __restrict__ sims, int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int qrow = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qrow >= nq) return;
  const size_t stride = (size_t)nq * k;
  const size_t base = (size_t)qrow * k;
  for (int e = lane; e < n_split * k; e += 64) {
    const int a = e / k, pa = e - a * k;
    const float s = slab_s[a * stride + base + pa];
    const int i = slab_i[a * stride + base + pa];
    if (i == INT_MAX) continue;   // an unfilled slot of a split shorter than k
    int rank = pa;
    for (int b = 0; b < n_split && rank < k; ++b) {
      if (b == a) continue;
      const float* ts = slab_s + b * stride + base;
      const int* ti = slab_i + b * stride + base;
      int lo = 0, hi = k;   // entries of list b that rank before (s, i)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (better(ts[mid], ti[mid], s, i)) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < k) {
      sims[base + rank] = s;
      idx[base + rank] = i;
    }
  }
}

// One wave per query, 4 queries per block.
__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ sims, const int* __restrict__ idx,
                                                       const int64_t* __restrict__ bank_labels,
                                                       const int64_t* __restrict__ labels, int nq, int nb, int k,
                                                       int n_cls, float T, float* __restrict__ scores,
                                                       float* __restrict__ rowhit) {
  __shared__ float sc[4][sdx_knn::kMaxClasses];
  __shared__ float wt[4][sdx_knn::kMaxK];
  __shared__ int lb[4][sdx_knn::kMaxK];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int qrow = blockIdx.x * 4 + wv;
  if (qrow >= nq) return;
  for (int j = lane; j < k; j += 64) {
    const int id = idx[(size_t)qrow * k + j];
    SDX_DCHECK(id >= 0 && id < nb);
    int l = -1;
    if (id >= 0 && id < nb) l = (int)bank_labels[id];
    SDX_DCHECK(l >= 0 && l < n_cls);
    wt[wv][j] = expf(sims[(size_t)qrow * k + j] / T);
    lb[wv][j] = l;
  }
  __builtin_amdgcn_wave_barrier();
  // lane = classes lane, lane + 64, ...: each class adds its neighbours' weights in list order
  for (int cls = lane; cls < n_cls; cls += 64) {
    float a = 0.f;
    for (int j = 0; j < k; ++j)
      if (lb[wv][j] == cls) a += wt[wv][j];
    sc[wv][cls] = a;
    scores[(size_t)qrow * n_cls + cls] = a;
  }
  if (labels == nullptr) return;
  __builtin_amdgcn_wave_barrier();
  const int lab = (int)labels[qrow];
  const bool ok = lab >= 0 && lab < n_cls;
  const float own = ok ? sc[wv][lab] : 0.f;
  float above = 0.f;
  for (int cls = lane; cls < n_cls; cls += 64) above += sc[wv][cls] > own ? 1.f : 0.f;
  above = wave_sum(above);
  if (lane == 0) {
    rowhit[(size_t)qrow * 2 + 0] = (ok && above < 1.f) ? 1.f : 0.f;
    rowhit[(size_t)qrow * 2 + 1] = (ok && above < 5.f) ? 1.f : 0.f;
  }
}

// stats[j] = Σ_rows rowhit[row][j]: every thread sums one contiguous run of rows, thread 0
// adds the runs in order (the counts are small integers: exact in fp32)
__global__ __launch_bounds__(256) void knn_hits_kernel(const float* __restrict__ rowhit, int nq,
                                                       float* __restrict__ stats) {
  __shared__ float part[256][2];
  const int per = (nq + 255) / 256;
  const int lo = threadIdx.x * per;
  int hi = lo + per;
  if (hi > nq) hi = nq;
  float a = 0.f, b = 0.f;
  for (int r = lo; r < hi; ++r) {
    a += rowhit[(size_t)r * 2];
    b += rowhit[(size_t)r * 2 + 1];
  }
  part[threadIdx.x][0] = a;
  part[threadIdx.x][1] = b;
  __syncthreads();
  if (threadIdx.x < 2) {
    float t = 0.f;
    for (int w = 0; w < 256; ++w) t += part[w][threadIdx.x];
    stats[threadIdx.x] = t;
  }
}

}  // namespace

hipError_t launch_knn_topk(const float* q, const float* bank, int nq, int nb, int D, int k, int n_split,
                           int rows_per_split, float* slab_s, int* slab_i, float* sims, int* idx, hipStream_t s) {
  if (!sdx_knn::dim_supported(D) || k < 1 || k > sdx_knn::kMaxK || k > nb || nq < 1 || n_split < 1 ||
      rows_per_split < 1 || rows_per_split % BT != 0 || (long)n_split * rows_per_split < nb ||
      (long)(n_split - 1) * rows_per_split >= nb)
    return hipErrorInvalidValue;
  if (n_split > 1 && (slab_s == nullptr || slab_i == nullptr)) return hipErrorInvalidValue;
  KnnParams p{};
  p.q = q; p.bank = bank;
  p.out_s = n_split > 1 ? slab_s : sims;
  p.out_i = n_split > 1 ? slab_i : idx;
  p.nq = nq; p.nb = nb; p.D = D; p.k = k; p.rows_per_split = rows_per_split; p.n_split = n_split;
  const dim3 grid((nq + QT - 1) / QT, n_split);
  if (k <= 64) hipLaunchKernelGGL((knn_topk_kernel<64>), grid, dim3(256), 0, s, p);
  else if (k <= 128) hipLaunchKernelGGL((knn_topk_kernel<128>), grid, dim3(256), 0, s, p);
  else if (k <= 200) hipLaunchKernelGGL((knn_topk_kernel<200>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((knn_topk_kernel<256>), grid, dim3(256), 0, s, p);
  SDX_LAUNCH_CHECK();
  if (n_split > 1) {
    hipLaunchKernelGGL(knn_merge_kernel, dim3((nq + 3) / 4), dim3(256), 0, s, slab_s, slab_i, nq, k, n_split, sims,
                       idx);
    SDX_LAUNCH_CHECK();
  }
  return hipSuccess;
}

hipError_t launch_knn_vote(const float* sims, const int* idx, const int64_t* bank_labels, const int64_t* labels,
                           int nq, int nb, int k, int n_cls, float T, float* scores, float* rowhit, float* stats,
                           hipStream_t s) {
  if (nq < 1 || k < 1 || k > sdx_knn::kMaxK || n_cls < 1 || n_cls > sdx_knn::kMaxClasses || !(T > 0.f))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(knn_vote_kernel, dim3((nq + 3) / 4), dim3(256), 0, s, sims, idx, bank_labels, labels, nq, nb, k,
                     n_cls, T, scores, rowhit);
  SDX_LAUNCH_CHECK();
  if (labels != nullptr) {
    hipLaunchKernelGGL(knn_hits_kernel, dim3(1), dim3(256), 0, s, rowhit, nq, stats);
    SDX_LAUNCH_CHECK();
  }
  return hipSuccess;
}
