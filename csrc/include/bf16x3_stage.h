// LDS staging of the split-bf16 (hi + lo) MFMA GEMMs of the pretraining losses (barlow.hip,
// vicreg.hip): an fp32 operand is read from global memory 32 reduction steps at a time, optionally
// centred or standardised per column of z, masked, split into bf16 hi + lo and written as two images
// of 64-byte rows [output index][32 reduction steps], 16-byte chunks XOR-swizzled. The loaded values
// stay raw in registers between load() and commit(), so the next chunk's global loads can fly under
// this chunk's MFMAs. VICReg's chunk loop (mma_tile) is in loss_gemm.h, Barlow's in barlow.hip. Device
// code, but for the launchers' operand() builder.
#pragma once
#include "common.h"

namespace sdx_stage {

using namespace sdx;

constexpr int kStageChunk = 32;             // reduction elements per staged chunk (one MFMA k-block)
constexpr int kStageRowB = kStageChunk * 2; // bytes of one staged bf16 row

enum StageMode {
  kRow = 0,    // reduction contiguous in memory: two float4 per slot
  kTrans = 1,  // output index contiguous, reduction strided: 8 dword loads, lanes along the output index
};

enum StageStat {
  kRaw = 0,     // staged as read
  kStd = 1,     // (x − mu)·rstd
  kCentre = 2,  // x − mu (rstd is not read)
};

// element (i, r), i the output index of this operand and r the reduction index, lives at
// p[i·si + r·sr]. The statistics are indexed by the column of z: i for kTrans, r for kRow.
struct Operand {
  const float* p;
  const float* mu;
  const float* rstd;
  int lim_i, lim_r;
  long si, sr;
};

// launcher side: element (i, r) at p[i·si + r·sr], i < lim_i, r < lim_r; the statistics where the mode reads them
inline Operand operand(const float* p, int lim_i, int lim_r, long si, long sr, const float* mu = nullptr,
                       const float* rstd = nullptr) {
  Operand o;
  o.p = p; o.mu = mu; o.rstd = rstd; o.lim_i = lim_i; o.lim_r = lim_r; o.si = si; o.sr = sr;
  return o;
}

__device__ __forceinline__ int sw_off(int row, int chunk) {
  return row * kStageRowB + ((chunk ^ ((row >> 1) & 3)) << 4);
}

// 8 floats -> 8 bf16 hi + 8 bf16 lo, one 16-byte LDS write each
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

// A thread stages ROWS / 64 (row, 8-step chunk) slots of a ROWS x 32 operand tile per step.
template <int MODE, int STD, int ROWS>
struct Stager {
  static constexpr int SLOTS = ROWS / 64;
  const float* base[SLOTS];   // clamped row base
  bool ok[SLOTS];
  int off[SLOTS];             // LDS byte offset of the slot
  int rch[SLOTS];             // first reduction element of the slot inside the chunk
  float mu_i[SLOTS], rs_i[SLOTS];   // kTrans: the slot's column statistics
  float raw[SLOTS][8];        // loaded, not yet standardised
  float mu_r[SLOTS][8], rs_r[SLOTS][8];   // kRow: statistics of the 8 reduction steps

  __device__ __forceinline__ void init(const Operand& o, int i0, int tid) {
#pragma unroll
    for (int ps = 0; ps < SLOTS; ++ps) {
      const int row = MODE == kTrans ? (tid & (ROWS - 1)) : ps * 64 + (tid >> 2);
      const int chunk = MODE == kTrans ? (tid / ROWS) + (256 / ROWS) * ps : (tid & 3);
      const int i = i0 + row;
      ok[ps] = i < o.lim_i;
      const int ic = ok[ps] ? i : o.lim_i - 1;
      base[ps] = o.p + (size_t)ic * o.si;
      off[ps] = sw_off(row, chunk);
      rch[ps] = chunk * 8;
      if constexpr (MODE == kTrans && STD != kRaw) mu_i[ps] = o.mu[ic];
      if constexpr (MODE == kTrans && STD == kStd) rs_i[ps] = o.rstd[ic];
    }
  }

  __device__ __forceinline__ void load(const Operand& o, int r0) {
#pragma unroll
    for (int ps = 0; ps < SLOTS; ++ps) {
      if constexpr (MODE == kRow) {
        // lim_r is a multiple of the chunk: no reduction tail on this path
        const int r = r0 + rch[ps];
        const float4* s = reinterpret_cast<const float4*>(base[ps] + r);
        const float4 v0 = s[0], v1 = s[1];
        raw[ps][0] = v0.x; raw[ps][1] = v0.y; raw[ps][2] = v0.z; raw[ps][3] = v0.w;
        raw[ps][4] = v1.x; raw[ps][5] = v1.y; raw[ps][6] = v1.z; raw[ps][7] = v1.w;
        if constexpr (STD != kRaw) {
          const float4* m = reinterpret_cast<const float4*>(o.mu + r);
          const float4 m0 = m[0], m1 = m[1];
          mu_r[ps][0] = m0.x; mu_r[ps][1] = m0.y; mu_r[ps][2] = m0.z; mu_r[ps][3] = m0.w;
          mu_r[ps][4] = m1.x; mu_r[ps][5] = m1.y; mu_r[ps][6] = m1.z; mu_r[ps][7] = m1.w;
        }
        if constexpr (STD == kStd) {
          const float4* q = reinterpret_cast<const float4*>(o.rstd + r);
          const float4 q0 = q[0], q1 = q[1];
          rs_r[ps][0] = q0.x; rs_r[ps][1] = q0.y; rs_r[ps][2] = q0.z; rs_r[ps][3] = q0.w;
          rs_r[ps][4] = q1.x; rs_r[ps][5] = q1.y; rs_r[ps][6] = q1.z; rs_r[ps][7] = q1.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = r0 + rch[ps] + j;
          const int rc = r < o.lim_r ? r : o.lim_r - 1;
          raw[ps][j] = base[ps][(size_t)rc * o.sr];
        }
      }
    }
  }

  // r0: the chunk that load() fetched
  __device__ __forceinline__ void commit(const Operand& o, int r0, unsigned char* hi_img, unsigned char* lo_img) const {
#pragma unroll
    for (int ps = 0; ps < SLOTS; ++ps) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float x = raw[ps][j];
        bool keep = ok[ps];
        if constexpr (MODE == kRow) {
          if constexpr (STD == kStd) x = (x - mu_r[ps][j]) * rs_r[ps][j];
          if constexpr (STD == kCentre) x = x - mu_r[ps][j];
        } else {
          if constexpr (STD == kStd) x = (x - mu_i[ps]) * rs_i[ps];
          if constexpr (STD == kCentre) x = x - mu_i[ps];
          keep = keep && (r0 + rch[ps] + j < o.lim_r);
        }
        v[j] = keep ? x : 0.f;   // zero AFTER centring: a padding row is not −μ
      }
      commit8(v, hi_img, lo_img, off[ps]);
    }
  }
};

}  // namespace sdx_stage
