// The tile of the training products (train_dense.hip, train_conv.hip):
//   C[i][j] = sum_r A(r, i) B(r, j),  r ascending over [r_begin, r_end), from +0.
// 256 threads, a 64 x 64 tile of C per workgroup, 32 x 32 per wave (2 x 2 16x16x4 MFMAs);
// r walks in chunks of 16 through LDS, the next chunk held in registers while this one computes.
// v_mfma_f32_16x16x4_f32 is an exact k-ordered fmaf chain, and every output element is reduced by
// one wave in one fixed order, so the result is the chain `gemm_chain` of tests/train_reference.py
// whatever the operands are.
//
// An operand is any type with
//   bool r_contig                     neighbouring threads of a load walk r (else the other axis)
//   float at(int64_t r, int64_t i)    the element, 0.0f where i (or the gather behind it) is out
//                                     of range; r is already known to lie in [r_begin, r_end)
#pragma once

#include "common.h"

namespace snnqp {
namespace gg {

constexpr int GT = 64;     // tile edge
constexpr int GR = 16;     // r per chunk
constexpr int GLD = GT + 4;

using f32x4 = __attribute__((ext_vector_type(4))) float;

// A(r, i) = p[r * sr + i * si] for i < n.
struct Strided {
  const float *__restrict__ p;
  int64_t sr, si, n;
  bool r_contig;
  __device__ __forceinline__ float at(int64_t r, int64_t i) const {
    return i < n ? p[r * sr + i * si] : 0.0f;
  }
};

inline Strided make_strided(const float *p, int64_t sr, int64_t si, int64_t n) {
  return Strided{p, sr, si, n, sr == 1 && si != 1};
}

// Element q (0..3) of this thread's share of one GR x GT operand chunk: (rr, ii) in the chunk.
// When the r axis is the contiguous one, neighbouring threads walk r; else they walk i.
__device__ __forceinline__ void chunk_coord(int tid, int q, bool r_contig, int &rr, int &ii) {
  const int idx = tid + 256 * q;
  if (r_contig) {
    rr = idx % GR;
    ii = idx / GR;
  } else {
    rr = idx / GT;
    ii = idx % GT;
  }
}

template <class Op>
__device__ __forceinline__ void load_chunk(const Op &op, int64_t r0, int64_t r_end, int64_t i0,
                                           int tid, float (&reg)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int rr, ii;
    chunk_coord(tid, q, op.r_contig, rr, ii);
    const int64_t r = r0 + rr;
    reg[q] = r < r_end ? op.at(r, i0 + ii) : 0.0f;
  }
}

__device__ __forceinline__ void store_chunk(float (*lds)[GLD], bool r_contig, int tid,
                                            const float (&reg)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int rr, ii;
    chunk_coord(tid, q, r_contig, rr, ii);
    lds[rr][ii] = reg[q];
  }
}

// The whole workgroup calls this once; acc is this wave's 32 x 32 of the tile at (i0, j0).
template <class OpA, class OpB>
__device__ __forceinline__ void tile_chain(const OpA &a, const OpB &b, int64_t i0, int64_t j0,
                                           int64_t r_begin, int64_t r_end, f32x4 (&acc)[2][2]) {
  __shared__ float As[GR][GLD];
  __shared__ float Bs[GR][GLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = (wave & 1) * 32, wj = (wave >> 1) * 32;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float ra[4], rb[4];
  load_chunk(a, r_begin, r_end, i0, tid, ra);
  load_chunk(b, r_begin, r_end, j0, tid, rb);
  const int kl = lane >> 4, il = lane & 15;
  for (int64_t r0 = r_begin; r0 < r_end; r0 += GR) {
    __syncthreads();                       // the previous chunk's reads are done
    store_chunk(As, a.r_contig, tid, ra);
    store_chunk(Bs, b.r_contig, tid, rb);
    __syncthreads();
    if (r0 + GR < r_end) {
      load_chunk(a, r0 + GR, r_end, i0, tid, ra);
      load_chunk(b, r0 + GR, r_end, j0, tid, rb);
    }
#pragma unroll
    for (int kk = 0; kk < GR; kk += 4) {
      // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
      float av[2], bv[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) av[x] = As[kk + kl][wi + 16 * x + il];
#pragma unroll
      for (int y = 0; y < 2; ++y) bv[y] = Bs[kk + kl][wj + 16 * y + il];
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
          acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[x], bv[y], acc[x][y], 0, 0, 0);
    }
  }
}

// f(i, j, v) for every element of this wave's share that lies inside [I] x [J].
// C/D: col = lane & 15, row = (lane >> 4) * 4 + reg
template <class F>
__device__ __forceinline__ void tile_store(const f32x4 (&acc)[2][2], int64_t i0, int64_t j0,
                                           int64_t I, int64_t J, F f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = (wave & 1) * 32, wj = (wave >> 1) * 32;
  const int kl = lane >> 4, il = lane & 15;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t i = i0 + wi + 16 * x + kl * 4 + g;
        const int64_t j = j0 + wj + 16 * y + il;
        if (i < I && j < J) f(i, j, acc[x][y][g]);
      }
}

}  // namespace gg
}  // namespace snnqp
