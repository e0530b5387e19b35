// What the two K-group dense kernels (dense_mfma.hip: int32 sums, dense_fp6.hip: the same
// integers in float32) run behind their K loops: the merge of the groups' accumulator tiles
// into one LDS tile, and the neuron over that tile.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace snnqp {

// Accumulator tiles of the KG wave groups -> one LDS tile et[row][128]: group KG - 1 stores its
// partial sums, the others add theirs on top, a barrier after each (exact: integers).
// C/D layout: col = n = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * h, h = lane >> 5 (the
// caller's own n and h: recomputed here from the lane they cost the paired LDS accesses)
template <int RT, int KG, typename E, typename V16>
__device__ __forceinline__ void dense_tile_merge(E *et, const V16 (&acc)[RT], int grp, int wave,
                                                 int n, int h, bool wave_on) {
#pragma unroll
  for (int g = KG - 1; g >= 0; --g) {
    if (wave_on && grp == g) {
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = r * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          E *e = et + row * 128 + wave * 32 + n;
          *e = (g == KG - 1) ? acc[r][i] : *e + acc[r][i];
        }
    }
    lds_barrier();
  }
}

// The neuron over the tile: one (sample, feature) pair per thread and pass -- dequantise,
// [BatchNorm], neuron_step over the T currents of the pair in order, u in a register; 64
// consecutive features of one sample per wave, so a ballot is two output words.
// E = int: the accumulator itself, plus 128 * col_sum[feat] when OFFS (uint8 rows entered the
// MFMA as x - 128); E = float: an exact integer.
template <bool OFFS, typename E>
__device__ __forceinline__ void dense_tile_neurons(const E *et, const int32_t *col_sum, const Dequant &dq,
                                                   const BnP &bn, const NeuronP &nrn, int T, int B, int N,
                                                   int SB, int b0, int nsamp, const float *u0,
                                                   float *u_out, uint32_t *s_out, int nthreads) {
  static_assert(std::is_same<E, int>::value || !OFFS, "the offset is added to an int32 accumulator");
  const int lane = threadIdx.x & 63;
  const int CW = (N + 31) >> 5;
  for (int p = threadIdx.x; p < SB * 128; p += nthreads) {
    const int bl = p >> 7, col = p & 127;
    const int feat = blockIdx.y * 128 + col;
    const bool live = bl < nsamp && feat < N;
    float bmean = 0.f, bmul = 1.f, bbias = 0.f, dec = 0.f, u = 0.0f;
    int off = 0;
    if (live) {
      if (OFFS) off = 128 * col_sum[feat];
      if (bn.mean) { bmean = bn.mean[feat]; bmul = bn.mul[feat]; bbias = bn.bias[feat]; }
      if (nrn.kind == SNNQP_NEURON_LIF) dec = nrn.decay[feat];
      if (u0) u = u0[(int64_t)(b0 + bl) * N + feat];
    }
    for (int t = 0; t < T; ++t) {
      bool s = false;
      if (live) {
        const E v = et[(bl * T + t) * 128 + col];
        float cur;
        if constexpr (std::is_same<E, int>::value) cur = dequant_acc(v + off, dq);
        else cur = div_exact(v, dq) * dq.m;
        if (bn.mean) cur = bn_apply(cur, bmean, bmul, bbias);
        s = neuron_step(u, cur, nrn, dec);
      }
      const unsigned long long m = __ballot(s);
      const int word = (blockIdx.y * 128 + (col & 64)) >> 5;     // wave-uniform
      if (bl < nsamp) {
        uint32_t *o = s_out + ((int64_t)t * B + (b0 + bl)) * CW;
        if (lane == 0 && word < CW) o[word] = (uint32_t)m;
        if (lane == 32 && word + 1 < CW) o[word + 1] = (uint32_t)(m >> 32);
      }
    }
    if (live && u_out) u_out[(int64_t)(b0 + bl) * N + feat] = u;
  }
}

}  // namespace snnqp
