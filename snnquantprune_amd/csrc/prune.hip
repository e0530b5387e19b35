// Magnitude pruning on the device: which entries of `mask` a prune event zeroes.
//
// The rule (include/snnqp.h states it as snnqp_magnitude_prune's contract): with m entries already
// pruned (mask word == +-0) and a target of k, the k - m unpruned entries that are smallest by
// key = bits(|w|) as uint32, ties by ascending index, get mask = +0.0f; k <= m writes nothing.
// Every decision is an integer compare or an integer count, so the result is a function of the
// values alone: not of the grid, of the order atomics arrive in, or of the device.
//
// Eight launches on one stream behind one memset of the workspace, no host read:
//   hist<0>   counts m and histograms bits 31..21 of every unpruned key
//   pick<0>   one workgroup: need = k - m (0: the launch is over, every later kernel returns at
//             once); the bucket that holds the need-th smallest key, and the rank left inside it
//   hist<1>, pick<1>   the same on bits 20..10 of the keys inside that bucket
//   hist<2>, pick<2>   and on bits 9..0: the cut key, and r = how many of the keys EQUAL to it go
//   ties      per workgroup, the number of unpruned keys equal to the cut in its index range
//   apply     every key below the cut, and the first r equal to it in index order: rank = the tie
//             counts of the workgroups before + the ties met so far in the range + the wave
//             offsets + the lane's position in its wave's ballot
// A workgroup owns the contiguous range [b per, (b + 1) per) of the index, per a multiple of the
// workgroup size, in every kernel.  A histogram lives in LDS; a lane collects a run of equal
// buckets in a register before it adds (weights of one layer share their exponent: the top
// buckets are hot), and the non-zero LDS counters are flushed with one global atomic each.
// Counters are 32-bit: n < 2^32.  Global values are written with vector stores and atomics only.
#include "kernels.h"

namespace snnqp {

constexpr int PRUNE_THREADS = 256;
constexpr int PRUNE_WAVES = PRUNE_THREADS / 64;
constexpr int PRUNE_BUCKETS = 2048;           // 11 bits; the 10-bit pass uses the lower half
constexpr int PRUNE_MAX_BLOCKS = 1024;
constexpr int PRUNE_BLOCK_ITEMS = 4096;       // the smallest range a workgroup owns (but the last)

// workspace, in 32-bit words
constexpr int PS_M = 0;                       // already-pruned entries
constexpr int PS_ACTIVE = 1;                  // 1: k > m, the later kernels work
constexpr int PS_NEED = 2;                    // rank (1-based) still to find inside the prefix
constexpr int PS_PREFIX = 3;                  // the key bits decided so far; after pick<2>: the cut
constexpr int PS_STATE_WORDS = 16;
constexpr int PS_HIST = PS_STATE_WORDS;       // [3][PRUNE_BUCKETS]
constexpr int PS_TIES = PS_HIST + 3 * PRUNE_BUCKETS;   // [PRUNE_MAX_BLOCKS]
constexpr int PS_WORDS = PS_TIES + PRUNE_MAX_BLOCKS;

struct PruneArgs {
  const uint32_t *w;
  uint32_t *mask;
  uint32_t *ws;
  int64_t n, per;
  uint32_t k;
};

template <int PASS> __device__ __forceinline__ uint32_t prune_bucket(uint32_t key) {
  return PASS == 0 ? key >> 21 : PASS == 1 ? (key >> 10) & 0x7FFu : key & 0x3FFu;
}
// the bits of the key the passes before PASS decided
template <int PASS> __device__ __forceinline__ uint32_t prune_decided(uint32_t key) {
  return PASS == 0 ? 0u : PASS == 1 ? key >> 21 : key >> 10;
}

template <int PASS>
__global__ void __launch_bounds__(PRUNE_THREADS)
prune_hist_kernel(const PruneArgs a) {
  __shared__ uint32_t hist[PRUNE_BUCKETS];
  if (PASS > 0 && a.ws[PS_ACTIVE] == 0) return;
  const uint32_t prefix = PASS > 0 ? a.ws[PS_PREFIX] : 0u;
  const int tid = threadIdx.x;
  for (int i = tid; i < PRUNE_BUCKETS; i += PRUNE_THREADS) hist[i] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * a.per;
  const int64_t hi = lo + a.per < a.n ? lo + a.per : a.n;
  uint32_t run_bucket = 0, run = 0, pruned = 0;
  for (int64_t i = lo + tid; i < hi; i += PRUNE_THREADS) {
    const uint32_t mk = a.mask[i] & 0x7FFFFFFFu;
    const uint32_t key = a.w[i] & 0x7FFFFFFFu;
    if (mk == 0) {
      ++pruned;
    } else if (prune_decided<PASS>(key) == prefix) {
      const uint32_t b = prune_bucket<PASS>(key);
      if (b != run_bucket) {
        if (run) atomicAdd(&hist[run_bucket], run);
        run_bucket = b;
        run = 0;
      }
      ++run;
    }
  }
  if (run) atomicAdd(&hist[run_bucket], run);
  if (PASS == 0 && pruned) atomicAdd(&a.ws[PS_M], pruned);
  __syncthreads();
  uint32_t *g = a.ws + PS_HIST + PASS * PRUNE_BUCKETS;
  for (int i = tid; i < PRUNE_BUCKETS; i += PRUNE_THREADS) {
    const uint32_t c = hist[i];
    if (c) atomicAdd(&g[i], c);
  }
}

// one workgroup: the bucket b with count(buckets < b) < need <= count(buckets <= b)
template <int PASS>
__global__ void __launch_bounds__(PRUNE_THREADS)
prune_pick_kernel(const PruneArgs a) {
  constexpr int PER = PRUNE_BUCKETS / PRUNE_THREADS;
  __shared__ uint32_t part[PRUNE_THREADS];
  __shared__ uint32_t need_s;
  const int tid = threadIdx.x;
  if (tid == 0) {
    uint32_t need;
    if (PASS == 0) {
      const uint32_t m = a.ws[PS_M];
      need = a.k > m ? a.k - m : 0u;
      a.ws[PS_ACTIVE] = need ? 1u : 0u;
    } else {
      need = a.ws[PS_ACTIVE] ? a.ws[PS_NEED] : 0u;
    }
    need_s = need;
  }
  const uint32_t *g = a.ws + PS_HIST + PASS * PRUNE_BUCKETS;
  uint32_t h[PER], sum = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    h[j] = g[tid * PER + j];
    sum += h[j];
  }
  part[tid] = sum;
  __syncthreads();
  const uint32_t need = need_s;
  if (need == 0) return;
  uint32_t below = 0;                         // keys in the buckets of the lanes before this one
  for (int t = 0; t < tid; ++t) below += part[t];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (below < need && need - below <= h[j]) {          // exactly one lane, one j
      const uint32_t b = (uint32_t)(tid * PER + j);
      const uint32_t prefix = PASS == 0 ? 0u : a.ws[PS_PREFIX];
      a.ws[PS_PREFIX] = PASS == 0 ? b : PASS == 1 ? (prefix << 11) | b : (prefix << 10) | b;
      a.ws[PS_NEED] = need - below;
    }
    below += h[j];
  }
}

__global__ void __launch_bounds__(PRUNE_THREADS)
prune_ties_kernel(const PruneArgs a) {
  __shared__ uint32_t wave_n[PRUNE_WAVES];
  if (a.ws[PS_ACTIVE] == 0) return;
  const uint32_t cut = a.ws[PS_PREFIX];
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * a.per;
  const int64_t hi = lo + a.per < a.n ? lo + a.per : a.n;
  uint32_t cnt = 0;
  for (int64_t i = lo + tid; i < hi; i += PRUNE_THREADS)
    cnt += ((a.mask[i] & 0x7FFFFFFFu) != 0 && (a.w[i] & 0x7FFFFFFFu) == cut) ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((tid & 63) == 0) wave_n[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    uint32_t s = 0;
#pragma unroll
    for (int v = 0; v < PRUNE_WAVES; ++v) s += wave_n[v];
    a.ws[PS_TIES + blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(PRUNE_THREADS)
prune_apply_kernel(const PruneArgs a) {
  __shared__ uint32_t wave_n[PRUNE_WAVES];
  if (a.ws[PS_ACTIVE] == 0) return;
  const uint32_t cut = a.ws[PS_PREFIX], r = a.ws[PS_NEED];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ties in the ranges before this one
  uint32_t before = 0;
  for (int b = tid; b < (int)blockIdx.x; b += PRUNE_THREADS) before += a.ws[PS_TIES + b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
  if (lane == 0) wave_n[wave] = before;
  __syncthreads();
  uint32_t running = 0;
#pragma unroll
  for (int v = 0; v < PRUNE_WAVES; ++v) running += wave_n[v];
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * a.per;
  const int64_t hi = lo + a.per < a.n ? lo + a.per : a.n;
  for (int64_t base = lo; base < hi; base += PRUNE_THREADS) {       // uniform trip count
    const int64_t i = base + tid;
    const bool valid = i < hi;
    const bool live = valid && (a.mask[i] & 0x7FFFFFFFu) != 0;
    const uint32_t key = valid ? a.w[i] & 0x7FFFFFFFu : 0u;
    const bool tie = live && key == cut;
    const unsigned long long bal = __ballot(tie);
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t off = 0, total = 0;
#pragma unroll
    for (int v = 0; v < PRUNE_WAVES; ++v) {
      const uint32_t c = wave_n[v];
      off += v < wave ? c : 0u;
      total += c;
    }
    const uint32_t rank = running + off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (live && (key < cut || (tie && rank < r))) a.mask[i] = 0u;    // +0.0f
    running += total;
    __syncthreads();
  }
}

int64_t magnitude_prune_workspace_bytes(int64_t n) {
  SNNQP_REQUIRE(n >= 0 && n < (1ll << 32), SNNQP_EINVAL,
                "magnitude_prune: n = %lld outside [0, 2^32) (32-bit counters)", (long long)n);
  return (int64_t)PS_WORDS * 4;
}

int run_magnitude_prune(const float *w, float *mask, int64_t n, int64_t k, void *ws, int64_t ws_bytes,
                        hipStream_t st) {
  SNNQP_REQUIRE(n >= 0, SNNQP_EINVAL, "magnitude_prune: n = %lld < 0", (long long)n);
  SNNQP_REQUIRE(k >= 0 && k <= n, SNNQP_EINVAL, "magnitude_prune: k = %lld outside [0, n = %lld]", (long long)k,
                (long long)n);
  if (n == 0) return SNNQP_OK;
  SNNQP_REQUIRE(n < (1ll << 32), SNNQP_EINVAL, "magnitude_prune: n = %lld >= 2^32 (32-bit counters)", (long long)n);
  SNNQP_REQUIRE(w && mask && ws, SNNQP_EINVAL, "magnitude_prune: null argument");
  SNNQP_REQUIRE((((uintptr_t)w | (uintptr_t)mask | (uintptr_t)ws) & 3) == 0, SNNQP_EINVAL,
                "magnitude_prune: w, mask and workspace must be 4-byte aligned");
  SNNQP_REQUIRE(ws_bytes >= (int64_t)PS_WORDS * 4, SNNQP_EINVAL, "magnitude_prune: workspace of %lld bytes, %lld needed",
                (long long)ws_bytes, (long long)PS_WORDS * 4);
  if (k == 0) return SNNQP_OK;                // k <= m whatever m is: nothing to write
  PruneArgs a;
  a.w = (const uint32_t *)w; a.mask = (uint32_t *)mask; a.ws = (uint32_t *)ws; a.n = n; a.k = (uint32_t)k;
  int64_t blocks = ceil_div64(n, PRUNE_BLOCK_ITEMS);
  if (blocks > PRUNE_MAX_BLOCKS) blocks = PRUNE_MAX_BLOCKS;
  a.per = ceil_div64(ceil_div64(n, blocks), PRUNE_THREADS) * PRUNE_THREADS;
  blocks = ceil_div64(n, a.per);              // (no empty range at the end)
  SNNQP_REQUIRE(blocks >= 1 && blocks <= PRUNE_MAX_BLOCKS, SNNQP_EINVAL, "magnitude_prune: %lld workgroups, grid too large",
                (long long)blocks);
  SNNQP_HIP(hipMemsetAsync(ws, 0, (size_t)PS_WORDS * 4, st));
  const dim3 grid((unsigned)blocks), one(1), block(PRUNE_THREADS);
  hipLaunchKernelGGL(prune_hist_kernel<0>, grid, block, 0, st, a);
  hipLaunchKernelGGL(prune_pick_kernel<0>, one, block, 0, st, a);
  hipLaunchKernelGGL(prune_hist_kernel<1>, grid, block, 0, st, a);
  hipLaunchKernelGGL(prune_pick_kernel<1>, one, block, 0, st, a);
  hipLaunchKernelGGL(prune_hist_kernel<2>, grid, block, 0, st, a);
  hipLaunchKernelGGL(prune_pick_kernel<2>, one, block, 0, st, a);
  hipLaunchKernelGGL(prune_ties_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(prune_apply_kernel, grid, block, 0, st, a);
  SNNQP_CHECK_LAUNCH("magnitude_prune kernels");
  return SNNQP_OK;
}

}  // namespace snnqp

using namespace snnqp;

extern "C" {

int snnqp_magnitude_prune(const float *w, float *mask, int64_t n, int64_t k, void *workspace,
                          int64_t workspace_bytes, snnqp_stream_t stream) {
  return run_magnitude_prune(w, mask, n, k, workspace, workspace_bytes, (hipStream_t)stream);
}

int64_t snnqp_magnitude_prune_workspace_bytes(int64_t n) { return magnitude_prune_workspace_bytes(n); }

}  // extern "C"
