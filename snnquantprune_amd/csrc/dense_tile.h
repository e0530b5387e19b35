// What the MFMA dense kernels share (who uses which, and what stayed in the kernels):
// the staging task of row-major rows and the spike-word mask, the swizzle of 128-byte LDS rows and the
// counted-wait barrier of a chunk, the hand-over between the workgroups of a tile (host half: kernels.h),
// and for the two K-group kernels the merge of the groups' tiles and the neuron over the merged tile.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace snnqp {

// Staging task `task` of a workgroup is unit task % WPR of tile row task / WPR, the same for every chunk;
// tile row = sample * T + t.  off: the row's offset from the workgroup's first sample in units of the
// strides (< 2^31: launch check); mask: all ones for a live row (in_tile: the task exists at all).  The
// loads of a K loop are unconditional (a dead row reads row 0) and the mask is applied when the word is
// expanded: a load under a lane mask makes the compiler wait with vmcnt(0), which drains the ring.
struct RowTask { uint32_t off, mask; };
template <int WPR>
__device__ __forceinline__ RowTask row_task(int task, bool in_tile, int rows, int T, int64_t xs_t, int64_t xs_b) {
  const int row = task / WPR;
  const bool live = in_tile && row < rows;
  RowTask r = {0u, live ? 0xFFFFFFFFu : 0u};
  if (live) {
    const int bl = row / T, t = row - bl * T;
    r.off = (uint32_t)((int64_t)t * xs_t + (int64_t)bl * xs_b);
  }
  return r;
}

// a staged spike word as it enters LDS: zero for a dead row and for word `chunk_word` >= KW (the load
// re-read the row's last word there); the sign of the difference as a mask, no select
__device__ __forceinline__ uint32_t bit_word_masked(uint32_t word, uint32_t rmask, int chunk_word, int KW) {
  return word & rmask & (uint32_t)((chunk_word - KW) >> 31);
}

// Byte address of 16-byte piece `piece` (of 8) of row `row` in an image of 128-byte rows: pieces swizzled
// by (row >> 1) & 7, so that the 16 lanes a ds_read_b128 serves per cycle ({0-3, 12-15, 20-27}, ...) hit
// 16 different bank quads (quad = 8 (row & 1) + (piece ^ (row >> 1) & 7)): the read of an A fragment and
// the ds_write_b128 of the staging are conflict-free.  The swizzle repeats every 16 rows; flipping bit 0
// of `piece` flips bit 4 of the address only.
__device__ __forceinline__ int swz128_addr(int row, int piece) {
  return row * 128 + ((piece ^ ((row >> 1) & 7)) << 4);
}

// The barrier that ends a chunk and publishes the image staged during it, which nobody reads before the
// chunk after next.  LDS operations of a wave complete in order and the PF youngest are the fragment
// reads of the NEXT chunk: waiting until only those are outstanding retires every write of this chunk
// without draining the fragments (no scalar load is in flight: the loops issue none).
template <int PF>
__device__ __forceinline__ void chunk_barrier() {
  asm volatile("s_waitcnt lgkmcnt(%0)\n\ts_barrier" : : "n"(PF) : "memory");
}

// The hand-over, the only cross-workgroup protocol of the library: `parts` workgroups each leave a payload
// in a caller workspace and draw a ticket; the one that draws the last reads the others' payloads (in its
// kernel) and goes on, the others are done.  Recipe R1 of cdna_hip_programming.md: the payload by agent-scope
// relaxed stores (write-through), every storing wave drains, one relaxed agent-scope ticket, agent-scope
// relaxed loads by the last arriver -- NO release / acquire fence: on this part a pair writes back /
// invalidates an L2, ~ 20 us per launch (0.075 ms against 0.066 unsplit).  The host zeroes the tickets in
// front of every launch (handoff_arm, kernels.h); nobody resets one.
// handoff_publish: dst[i] = load(i), i < n, by the workgroup's `nthreads` threads, every store drained.
template <typename V, typename F>
__device__ __forceinline__ void handoff_publish(V *dst, int n, int nthreads, F &&load) {
  for (int i = threadIdx.x; i < n; i += nthreads)
    __hip_atomic_store(dst + i, load(i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
// Behind the publication: true in every thread of the workgroup that drew the last of `parts` tickets; a
// ticket too many goes to the device's status word.  lds_flag: a word of LDS free until the call returns.
__device__ __forceinline__ bool handoff_last_arriver(uint32_t *ticket_word, uint32_t parts, uint32_t *status,
                                                     uint32_t *lds_flag) {
  if (threadIdx.x == 0) {
    const uint32_t ticket = __hip_atomic_fetch_add(ticket_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket >= parts && status) *(volatile uint32_t *)status = SNNQP_STATUS_TICKET;
    *lds_flag = ticket + 1u == parts ? 1u : 0u;
  }
  __syncthreads();
  return *lds_flag != 0u;
}

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
