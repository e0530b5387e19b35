// Rate encoder (examples/input_pipeline.py:286-296, the `mnist` branch: static images, Poisson-
// encoded into num_frames count frames): one launch turns B rows of a device-resident uint8 image
// set into [B][T][K] counts (SNNQP_U8) or bit-packed spikes (SNNQP_BITS).  DESIGN.md 16.
//
// Every decision is an integer one: the hash u = fmix32(c ^ (t * K + k)) of the element under the
// row's key c, compared with the thresholds table[v][.] of the pixel's value v (include/snnqp.h
// states the contract).  The kernel compares min(u, 2^32 - 2) instead of u: that is the rule "an
// entry of 2^32 - 1 stands for 2^32" without a second test -- no clamped hash reaches such an
// entry, and against every smaller entry 2^32 - 2 compares as 2^32 - 1 does.
//
// One workgroup per (row b, chunk of tc steps).  The table goes into LDS once (Poisson: all of it,
// 16 KiB; Bernoulli: column 0, 1 KiB).  A lane owns a UNIT of the row -- four consecutive elements
// (bytes) or the 32 elements of one spike word (bits) -- reads the sample's bytes of that unit
// once, looks their thresholds up once, keeps them in registers (4 x 15, 4 x 1 or 32 x 1) and
// walks its steps of the chunk with them: per element and step the work is one hash and its
// compares, no memory access.  A row of fewer than 256 units shares the workgroup between `ts`
// steps (lane = step * wp + unit, wp the power of two that holds the units), so short rows keep
// their lanes busy.  c is uniform per workgroup (scalar arithmetic).
//
// Stores: a spike word is one dword; lanes of consecutive units store consecutive dwords.  The
// four bytes of a unit are one dword store as well, whatever the row's alignment (K % 4 != 0 puts
// three rows of four off a 4-byte boundary): the store is written as a 4-byte copy of unknown
// alignment, which on gfx950 under HSA (unaligned access mode) the compiler emits as one
// global_store_dword; the sample's bytes are read the same way.  Only the row's partial tail
// (K % 4 elements) takes byte stores.  No atomics, vector stores only.
#include "kernels.h"

namespace snnqp {

constexpr int ENC_THREADS = 256;

struct RateEncodeArgs {
  const uint8_t *images;
  const int32_t *sample;
  const uint32_t *sample_id;
  const uint32_t *table;
  void *out;
  int64_t os_b, os_t;                     // elements (bytes) or words (bits)
  int32_t S, T, K;
  uint32_t seed, draw;
  int32_t tc, nchunks, wp_log2;           // steps per workgroup, chunks per row, log2 of the unit lanes
};

// the murmur3 finaliser (include/snnqp.h states it as part of snnqp_events_bin_aug's contract)
__device__ __forceinline__ uint32_t enc_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ uint32_t enc_draw(uint32_t c, uint32_t e) {
  const uint32_t u = enc_fmix32(c ^ e);
  return u < 0xFFFFFFFEu ? u : 0xFFFFFFFEu;
}

// what every workgroup starts with: its row, its steps, the row's key and image (null: a sample
// outside [0, S), which encodes as an image of zeros)
struct EncodeRow {
  int32_t b, t0, t1, unit, tsub, wp, ts;
  uint32_t c;
  const uint8_t *img;
};

__device__ __forceinline__ EncodeRow encode_row(const RateEncodeArgs &a) {
  EncodeRow r;
  const int tid = threadIdx.x;
  r.b = (int32_t)(blockIdx.x / (uint32_t)a.nchunks);
  r.t0 = (int32_t)(blockIdx.x % (uint32_t)a.nchunks) * a.tc;
  r.t1 = r.t0 + a.tc < a.T ? r.t0 + a.tc : a.T;
  r.wp = 1 << a.wp_log2;
  r.ts = ENC_THREADS >> a.wp_log2;
  r.unit = tid & (r.wp - 1);
  r.tsub = tid >> a.wp_log2;
  const int32_t s = a.sample[r.b];
  r.img = (uint32_t)s < (uint32_t)a.S ? a.images + (int64_t)s * a.K : nullptr;
  r.c = enc_fmix32(enc_fmix32(a.seed ^ enc_fmix32(a.draw)) ^ a.sample_id[r.b]);
  return r;
}

// n <= N bytes of the row from element k0 on, the rest zero; a whole unit as dwords (of any alignment)
template <int N>
__device__ __forceinline__ void encode_pixels(const uint8_t *img, int32_t k0, int32_t n, uint32_t (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = 0;
  if (!img) return;
  const uint8_t *p = img + k0;
  if (n == N) {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
      uint32_t w;
      __builtin_memcpy(&w, p + i, 4);
      v[i] = w & 0xFFu; v[i + 1] = (w >> 8) & 0xFFu; v[i + 2] = (w >> 16) & 0xFFu; v[i + 3] = w >> 24;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i < n) v[i] = p[i];
  }
}

// POISSON false: 0 / 1 bytes from column 0; true: counts 0..15 from columns 0..14
template <bool POISSON>
__global__ void __launch_bounds__(ENC_THREADS)
rate_encode_u8_kernel(const RateEncodeArgs a) {
  constexpr int NT = POISSON ? 15 : 1;
  __shared__ __attribute__((aligned(16))) uint32_t tab[POISSON ? 256 * 16 : 256];
  const int tid = threadIdx.x;
  if constexpr (POISSON) {
    for (int i = tid; i < 256 * 16; i += ENC_THREADS) tab[i] = a.table[i];
  } else {
    tab[tid] = a.table[tid * 16];
  }
  __syncthreads();
  const EncodeRow r = encode_row(a);
  const int32_t K = a.K, nunits = (K + 3) >> 2;
  uint8_t *const row0 = (uint8_t *)a.out + r.b * a.os_b;
  for (int32_t u = r.unit; u < nunits; u += r.wp) {
    const int32_t k0 = 4 * u, n = K - k0 < 4 ? K - k0 : 4;
    uint32_t v[4], th[4][NT];
    encode_pixels<4>(r.img, k0, n, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (POISSON) {
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
        const v4u *q = (const v4u *)(tab + v[i] * 16);
        const v4u q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
#pragma unroll
        for (int j = 0; j < 4; ++j) { th[i][j] = q0[j]; th[i][4 + j] = q1[j]; th[i][8 + j] = q2[j]; }
#pragma unroll
        for (int j = 0; j < 3; ++j) th[i][12 + j] = q3[j];
      } else {
        th[i][0] = tab[v[i]];
      }
    }
    for (int32_t t = r.t0 + r.tsub; t < r.t1; t += r.ts) {
      const uint32_t e0 = (uint32_t)t * (uint32_t)K + (uint32_t)k0;
      uint32_t word = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t h = enc_draw(r.c, e0 + i);
        uint32_t val = 0;
        if constexpr (POISSON) {
#pragma unroll
          for (int j = 0; j < NT; ++j) val += h >= th[i][j] ? 1u : 0u;
        } else {
          val = h < th[i][0] ? 1u : 0u;
        }
        word |= val << (8 * i);
      }
      uint8_t *dst = row0 + t * a.os_t + k0;
      if (n == 4) {
        __builtin_memcpy(dst, &word, 4);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < n) dst[i] = (uint8_t)(word >> (8 * i));
      }
    }
  }
}

// Bernoulli spikes as ops.PackedSpikes words: element k in bit (k & 31) of word (k >> 5); the
// bits of a row's last word past K get the threshold 0, which no hash is below
__global__ void __launch_bounds__(ENC_THREADS)
rate_encode_bits_kernel(const RateEncodeArgs a) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = a.table[threadIdx.x * 16];
  __syncthreads();
  const EncodeRow r = encode_row(a);
  const int32_t K = a.K, nwords = (K + 31) >> 5;
  uint32_t *const row0 = (uint32_t *)a.out + r.b * a.os_b;
  for (int32_t w = r.unit; w < nwords; w += r.wp) {
    const int32_t k0 = 32 * w, n = K - k0 < 32 ? K - k0 : 32;
    uint32_t v[32], th[32];
    encode_pixels<32>(r.img, k0, n, v);
#pragma unroll
    for (int i = 0; i < 32; ++i) th[i] = i < n ? tab[v[i]] : 0u;
    for (int32_t t = r.t0 + r.tsub; t < r.t1; t += r.ts) {
      const uint32_t e0 = (uint32_t)t * (uint32_t)K + (uint32_t)k0;
      uint32_t word = 0;
#pragma unroll
      for (int i = 0; i < 32; ++i) word |= (enc_draw(r.c, e0 + i) < th[i] ? 1u : 0u) << i;
      row0[t * a.os_t + w] = word;
    }
  }
}

int run_rate_encode(const uint8_t *images, int32_t S, const int32_t *sample, const uint32_t *sample_id,
                    int32_t B, int32_t T, int32_t K, uint32_t seed, uint32_t draw, const uint32_t *table,
                    int kind, void *out, int out_type, int64_t os_b, int64_t os_t, hipStream_t st) {
  SNNQP_REQUIRE(S >= 0 && B >= 0 && T >= 0 && K >= 1, SNNQP_EINVAL,
                "rate_encode: bad shape (S %d, B %d, T %d, K %d; K >= 1)", S, B, T, K);
  SNNQP_REQUIRE((int64_t)T * K < (1ll << 32), SNNQP_EINVAL,
                "rate_encode: T * K = %lld elements per sample do not fit the 32-bit element index",
                (long long)((int64_t)T * K));
  SNNQP_REQUIRE(kind == SNNQP_ENCODE_BERNOULLI || kind == SNNQP_ENCODE_POISSON, SNNQP_EINVAL,
                "rate_encode: kind must be SNNQP_ENCODE_BERNOULLI or SNNQP_ENCODE_POISSON");
  SNNQP_REQUIRE(out_type == SNNQP_U8 || out_type == SNNQP_BITS, SNNQP_EINVAL,
                "rate_encode: out_type must be SNNQP_U8 or SNNQP_BITS");
  SNNQP_REQUIRE(!(kind == SNNQP_ENCODE_POISSON && out_type == SNNQP_BITS), SNNQP_EINVAL,
                "rate_encode: Poisson counts do not fit SNNQP_BITS (Bernoulli only)");
  if (B == 0 || T == 0) return SNNQP_OK;
  SNNQP_REQUIRE(images && sample && sample_id && table && out, SNNQP_EINVAL, "rate_encode: null argument");
  SNNQP_REQUIRE(((uintptr_t)table & 3) == 0 && (out_type != SNNQP_BITS || ((uintptr_t)out & 3) == 0), SNNQP_EINVAL,
                "rate_encode: the table and SNNQP_BITS words must be 4-byte aligned");
  const bool bits = out_type == SNNQP_BITS;
  const int32_t units = bits ? (K + 31) / 32 : (K + 3) / 4;
  RateEncodeArgs a;
  a.images = images; a.sample = sample; a.sample_id = sample_id; a.table = table; a.out = out;
  a.os_b = os_b; a.os_t = os_t; a.S = S; a.T = T; a.K = K; a.seed = seed; a.draw = draw;
  a.wp_log2 = 0;
  while (a.wp_log2 < 8 && (1 << a.wp_log2) < units) ++a.wp_log2;
  // steps per workgroup: up to 8 per lane (the thresholds are looked up once per chunk), fewer
  // while that leaves the chip short of workgroups
  const int32_t ts = ENC_THREADS >> a.wp_log2;
  int32_t per_lane = 8;
  auto chunks = [&](int32_t m) { return (int32_t)(((int64_t)T + (int64_t)ts * m - 1) / ((int64_t)ts * m)); };
  while (per_lane > 1 && (int64_t)B * chunks(per_lane) < 1024) per_lane >>= 1;
  a.tc = ts * per_lane;
  a.nchunks = chunks(per_lane);
  const int64_t grid = (int64_t)B * a.nchunks;
  SNNQP_REQUIRE(grid < (1ll << 31), SNNQP_EINVAL, "rate_encode: %lld workgroups, grid too large", (long long)grid);
  if (bits) {
    hipLaunchKernelGGL(rate_encode_bits_kernel, dim3((unsigned)grid), dim3(ENC_THREADS), 0, st, a);
  } else if (kind == SNNQP_ENCODE_POISSON) {
    hipLaunchKernelGGL(rate_encode_u8_kernel<true>, dim3((unsigned)grid), dim3(ENC_THREADS), 0, st, a);
  } else {
    hipLaunchKernelGGL(rate_encode_u8_kernel<false>, dim3((unsigned)grid), dim3(ENC_THREADS), 0, st, a);
  }
  SNNQP_CHECK_LAUNCH("rate_encode_kernel");
  return SNNQP_OK;
}

}  // namespace snnqp

using namespace snnqp;

extern "C" {

int snnqp_rate_encode(const uint8_t *images, int32_t S, const int32_t *sample, const uint32_t *sample_id,
                      int32_t B, int32_t T, int32_t K, uint32_t seed, uint32_t draw, const uint32_t *table,
                      int kind, void *out, int out_type, int64_t os_b, int64_t os_t, snnqp_stream_t stream) {
  return run_rate_encode(images, S, sample, sample_id, B, T, K, seed, draw, table, kind, out, out_type, os_b, os_t,
                         (hipStream_t)stream);
}

}  // extern "C"
