// Batched event front end (examples/input_pipeline.py:63-139 split_by = "time", :142-219
// split_by = "number"): one launch bins B rows of ragged, device-resident event streams into
// [B][T] frames of H x W x 2 counts, written straight in the format the event layer reads
// (SNNQP_U8, SNNQP_EV4, SNNQP_EV1).  DESIGN.md 13.
//
// One workgroup per (row, frame, band).  A band is up to 16 384 consecutive pixels of the frame
// in index order (pixel = y * W + x), one 32-bit LDS word per pixel: polarity 0 counts in bits
// 0..15, polarity 1 in bits 16..31 -- a 128 x 128 frame is one band of 64 KiB, two workgroups per
// CU.  Bands are cut in pixels, not rows, so every band begins on a 16-pixel boundary: a whole
// EV1 word, 16 EV4 bytes, 32 uint8 bytes, whatever W is.  A frame of several bands (ASL-DVS,
// 240 x 240: four) has each band's workgroup walk the same slice and keep its own pixels.
//
// The frame's events are a contiguous slice of the sample: arithmetic in number mode, two
// 64-ary searches over the sample's sorted times in time mode (waves 0 and 1, one bound each,
// three rounds of one load for 2^18 events).  The slice is streamed 16 bytes per lane and
// counted with LDS integer atomics (integer adds commute: the result is bit-reproducible).
// 16-bit halves stay exact because the slice is walked in chunks of 65 280 events with a clamp
// of every half to 255 between chunks: min(min(a, 255) + b, 255) = min(a + b, 255), and every
// format saturates at or below 255 and flags above 15 / above 1, which the clamp preserves.
//
// AUG (snnqp_events_bin_aug): the row's snnqp_event_aug_t record, read once per
// workgroup (b is uniform: scalar loads), turns every event's decode into flip, shift, cutout,
// hashed drop and polarity swap before the same LDS add -- per-event integer decisions on values
// the lane already holds.  The slice, the searches, the chunks and the clamp are those of the
// untouched sample (the clamp then counts walked events, dropped ones included: only more
// conservative); a frame the record empties walks nothing and writes its zero band.
//
// MIX (snnqp_events_bin_mix): a second slice -- the partner sample's slice of the same
// frame, under the partner's record -- walked into the same histogram.  One more integer test per
// event: the primary's events inside the row's box are dropped, the partner's outside it.  The
// halves are clamped between the two walks as between two chunks, and the events that reach the add
// are counted per thread, summed in LDS and added to counts[b] once per workgroup and sample.
#include "kernels.h"

#include <cmath>
#include <mutex>
#include <type_traits>

namespace snnqp {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

constexpr int EB_BAND_PIX = 16384;        // pixels (LDS words) of a band: 64 KiB
constexpr int EB_CHUNK = 65280;           // 65535 - 255, a multiple of 4

struct EventsBinArgs {
  const uint32_t *addr;
  const int32_t *times;
  const int64_t *offsets;
  const int32_t *sample;
  const int32_t *start;
  void *out;
  int32_t *flags;
  float scale;
  int32_t S, T, step_us, H, W, mode, nbands;
};
// the augmenting kernel's: the plain kernel keeps the argument block it had
struct EventsBinAugArgs : EventsBinArgs {
  const snnqp_event_aug_t *aug;
};
// the mixing kernel's (any of the five may be null: an unmixed launch, identity records, no counts)
struct EventsBinMixArgs : EventsBinAugArgs {
  const int32_t *sample2;
  const int32_t *start2;
  const snnqp_event_aug_t *aug2;
  const int32_t *box;
  unsigned long long *counts;
};
// the kernel's variants.  Plain ints and a traits struct: the kernels' names must mangle alike in
// the host and the device compilation, which number an unnamed enum's type differently.
constexpr int EB_PLAIN = 0, EB_AUG = 1, EB_MIX = 2;
template <int VAR> struct EventsBinArgsOf { using type = EventsBinArgs; };
template <> struct EventsBinArgsOf<EB_AUG> { using type = EventsBinAugArgs; };
template <> struct EventsBinArgsOf<EB_MIX> { using type = EventsBinMixArgs; };
template <int VAR>
using EventsBinKernelArgs = typename EventsBinArgsOf<VAR>::type;

// First index i of [a, b) with times[i] > key (STRICT) or >= key: every round the wave probes 64
// evenly spaced elements and keeps the stretch in front of the first that satisfies the test.
// On unsorted times the answer means nothing, but a and b never leave the range they came with.
template <bool STRICT>
__device__ __forceinline__ int64_t first_index(const int32_t *__restrict__ times, int64_t a, int64_t b,
                                               int64_t key, int lane) {
  while (a < b) {
    const int64_t step = (b - a + 63) >> 6;
    const int64_t idx = a + (lane + 1) * step - 1;
    bool hit = true;
    if (idx < b) {
      const int64_t t = times[idx];
      hit = STRICT ? t > key : t >= key;
    }
    const uint64_t m = __ballot(hit);
    if (m == 0) return b;
    const int k = __builtin_ctzll(m);
    const int64_t probe = a + (k + 1) * step - 1;      // satisfies the test, or lies beyond b
    a += k * step;
    b = probe < b ? probe : b;
  }
  return a;
}

__device__ __forceinline__ uint32_t sat_half(uint32_t v, uint32_t cap) { return v < cap ? v : cap; }

// the murmur3 finaliser (include/snnqp.h states it as part of snnqp_events_bin_aug's contract)
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// MIX only: the workgroup's kept events of the primary and of the partner
__device__ __forceinline__ unsigned long long *kept_events_lds() {
  __shared__ unsigned long long sum[2];
  return sum;
}

template <int OUT, int VAR>
__global__ void __launch_bounds__(512)
events_bin_kernel(const EventsBinKernelArgs<VAR> a) {
  constexpr bool AUG = VAR != EB_PLAIN, MIX = VAR == EB_MIX;
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
  __shared__ int64_t range[MIX ? 4 : 2];
  const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int64_t blk = blockIdx.x;
  const int band = (int)(blk % a.nbands);
  const int64_t fi = blk / a.nbands;                    // b * T + f
  const int f = (int)(fi % a.T);
  const int b = (int)(fi / a.T);
  const int32_t npix = a.H * a.W;
  const int32_t p0 = band * EB_BAND_PIX;
  const int32_t np = npix - p0 < EB_BAND_PIX ? npix - p0 : EB_BAND_PIX;
  const int32_t nalloc = (np + 15) & ~15;               // whole EV1 words; the padding stays zero

  for (int i = tid * 4; i < nalloc; i += nth * 4) *(v4u *)(hist + i) = (v4u){0, 0, 0, 0};

  // the row's record; a frame it empties keeps o0 = o1 = 0: no search round, no walk, a zero band
  snnqp_event_aug_t g = {};
  bool live = true;
  uint32_t hseed = 0;
  if constexpr (AUG) {
    if constexpr (MIX) {
      if (a.aug) g = a.aug[b];
    } else {
      g = a.aug[b];
    }
    live = !(f >= g.f0 && f < g.f1);
    hseed = fmix32(g.seed);
  }

  // MIX: the partner's record and the row's box.  `rect` is what the walk in hand tests its events
  // against, keeping those inside it (`keep_in`, the partner's walk) or those outside it; it stays
  // empty for an unmixed row and for a frame outside [g0, g1), whose primary walk then drops nothing.
  [[maybe_unused]] snnqp_event_aug_t g2 = {};
  [[maybe_unused]] int32_t rect[4] = {0, 0, 0, 0};
  [[maybe_unused]] bool keep_in = false, live2 = false;
  [[maybe_unused]] int32_t s2 = -1;
  [[maybe_unused]] uint64_t kept = 0;
  [[maybe_unused]] unsigned long long *kept_sum = nullptr;
  if constexpr (MIX) {
    kept_sum = kept_events_lds();
    if (tid < 2) kept_sum[tid] = 0;
    if (a.sample2) s2 = a.sample2[b];
    if (s2 >= 0 && s2 < a.S) {
      const int32_t *bx = a.box + (int64_t)b * 6;
      if (f >= bx[4] && f < bx[5]) {
        rect[0] = bx[0]; rect[1] = bx[1]; rect[2] = bx[2]; rect[3] = bx[3];
        if (a.aug2) g2 = a.aug2[b];
        live2 = rect[2] > rect[0] && rect[3] > rect[1] && !(f >= g2.f0 && f < g2.f1);
      }
    }
  }

  // the sample's events, then the frame's slice of them
  const int32_t s = a.sample[b];
  int64_t o0 = 0, o1 = 0;
  if (s >= 0 && s < a.S && live) {
    o0 = a.offsets[s];
    o1 = a.offsets[s + 1];
    if (o1 < o0) o1 = o0;
  }
  int64_t p0s = 0, p1s = 0;                             // MIX: the partner's events, its frame's slice
  if constexpr (MIX) {
    if (live2) {
      p0s = a.offsets[s2];
      p1s = a.offsets[s2 + 1];
      if (p1s < p0s) p1s = p0s;
    }
  }
  int64_t e0, e1, q0 = 0, q1 = 0;
  if (a.mode == 0) {
    const int64_t di = (o1 - o0) / a.T;                 // n < T: everything in the last frame
    e0 = o0 + f * di;
    e1 = f == a.T - 1 ? o1 : e0 + di;
    if constexpr (MIX) {
      const int64_t dq = (p1s - p0s) / a.T;
      q0 = p0s + f * dq;
      q1 = f == a.T - 1 ? p1s : q0 + dq;
    }
  } else if constexpr (MIX) {
    if (wave < 4) {                                     // waves 0, 1: the primary's bounds; 2, 3: the partner's
      const bool second = wave >= 2;
      const int32_t origin = second ? (a.start2 ? a.start2[b] : 0) : a.start[b];
      const int64_t lo = (int64_t)origin + (int64_t)f * a.step_us;
      const int64_t ra = second ? p0s : o0, rb = second ? p1s : o1;
      const int64_t r = (wave & 1) == 0 ? first_index<true>(a.times, ra, rb, lo, lane)
                                        : first_index<false>(a.times, ra, rb, lo + a.step_us, lane);
      if (lane == 0) range[wave] = r;
    }
    __syncthreads();
    e0 = range[0];
    e1 = range[1];
    q0 = range[2];
    q1 = range[3];
  } else {
    if (wave < 2) {
      const int64_t lo = (int64_t)a.start[b] + (int64_t)f * a.step_us;
      const int64_t r = wave == 0 ? first_index<true>(a.times, o0, o1, lo, lane)             // lo < t
                                  : first_index<false>(a.times, o0, o1, lo + a.step_us, lane);  // t < hi
      if (lane == 0) range[wave] = r;
    }
    __syncthreads();
    e0 = range[0];
    e1 = range[1];
  }
  __syncthreads();                                      // the histogram is zero

  const bool unit = a.scale == 1.0f;
  const float scale = a.scale;
  const int32_t H = a.H, W = a.W;
  // n: the event's index in the stream (AUG: its index within the sample is what the drop hashes;
  // `first` is the first event of the sample the walk in hand reads)
  [[maybe_unused]] int64_t first = o0;
  auto one = [&](uint32_t w, int64_t n) {
    int32_t x = (int32_t)(w & 0x3FFFu), y = (int32_t)((w >> 14) & 0x3FFFu);
    if (!unit) {
      x = (int32_t)fminf(floorf((float)x / scale), 65536.0f);
      y = (int32_t)fminf(floorf((float)y / scale), 65536.0f);
    }
    if (x >= W || y >= H) return;                       // (never negative: scale > 0)
    if constexpr (AUG) {
      if (g.flags & 1u) x = W - 1 - x;
      if (g.flags & 2u) y = H - 1 - y;
      // the shift in unsigned arithmetic, so that no record overflows: a dx outside (-W, W) lands
      // outside [0, W) modulo 2^32 as well.  One unsigned test per axis catches the negatives.
      x = (int32_t)((uint32_t)x + (uint32_t)g.dx);
      y = (int32_t)((uint32_t)y + (uint32_t)g.dy);
      if ((uint32_t)x >= (uint32_t)W || (uint32_t)y >= (uint32_t)H) return;
      if (x >= g.cut_x0 && x < g.cut_x1 && y >= g.cut_y0 && y < g.cut_y1) return;
      if (fmix32(hseed ^ (uint32_t)(n - (MIX ? first : o0))) < g.drop_below) return;
      w ^= (g.flags & 4u) << 26;                        // bit 2 onto the polarity, bit 28
    }
    if constexpr (MIX) {
      const bool in = x >= rect[0] && x < rect[2] && y >= rect[1] && y < rect[3];
      if (in != keep_in) return;
    }
    const uint32_t pb = (uint32_t)(y * W + x - p0);
    if constexpr (MIX) {
      if (pb < (uint32_t)np) ++kept;                    // (each pixel lies in one band: counted once)
    }
    if (pb < (uint32_t)np) atomicAdd(&hist[pb], (w >> 28) & 1u ? 0x10000u : 1u);
  };
  auto four = [&](const v4u &w, int64_t n) { one(w.x, n); one(w.y, n + 1); one(w.z, n + 2); one(w.w, n + 3); };

  // MIX walks twice: the primary's slice, then -- with the partner's record, seed and first event,
  // and the box kept instead of dropped -- the partner's.  `more` clamps the halves after the
  // primary's last chunk as between two chunks, so every half stands at 255 or below when the
  // partner's chunks of 65 280 begin.  (The other variants' single pass is the loop it always was.)
  [[maybe_unused]] uint64_t kept_a = 0;
  for (int pass = 0; pass < (MIX ? 2 : 1); ++pass) {
    if constexpr (MIX) {
      if (pass == 1) {
        if (q0 >= q1) break;
        kept_a = kept;
        kept = 0;
        g = g2;
        hseed = fmix32(g2.seed);
        first = p0s;
        keep_in = true;
        e0 = q0;
        e1 = q1;
      }
    }
    const bool more = MIX && pass == 0 && q0 < q1;
    for (int64_t c0 = e0; c0 < e1; c0 += EB_CHUNK) {
      const int64_t c1 = c0 + EB_CHUNK < e1 ? c0 + EB_CHUNK : e1;
      // up to three events in front of the first 16-byte boundary, whole 16-byte words, the rest
      int64_t h = c0 + ((4 - (int)(((uintptr_t)(a.addr + c0) >> 2) & 3)) & 3);
      if (h > c1) h = c1;
      const int64_t nv = (c1 - h) >> 2;
      if (c0 + tid < h) one(a.addr[c0 + tid], c0 + tid);
      const v4u *bv = (const v4u *)(a.addr + h);
      int64_t i = tid;
      for (; i + 3 * nth < nv; i += 4 * nth) {          // four loads in flight per lane
        const v4u w0 = bv[i], w1 = bv[i + nth], w2 = bv[i + 2 * nth], w3 = bv[i + 3 * nth];
        four(w0, h + 4 * i);
        four(w1, h + 4 * (i + nth));
        four(w2, h + 4 * (i + 2 * nth));
        four(w3, h + 4 * (i + 3 * nth));
      }
      for (; i < nv; i += nth) four(bv[i], h + 4 * i);
      const int64_t t0 = h + nv * 4;
      if (t0 + tid < c1) one(a.addr[t0 + tid], t0 + tid);
      if (c1 < e1 || more) {                            // more to come: make room in the halves
        __syncthreads();
        for (int j = tid * 4; j < nalloc; j += nth * 4) {
          v4u w = *(v4u *)(hist + j);
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = sat_half(w[k] & 0xFFFFu, 255u) | (sat_half(w[k] >> 16, 255u) << 16);
          *(v4u *)(hist + j) = w;
        }
        __syncthreads();
      }
    }
  }
  if constexpr (MIX) {
    // (a partner's walk that never began leaves the primary's count in `kept`)
    const uint64_t na = keep_in ? kept_a : kept, nb = keep_in ? kept : 0;
    if (a.counts && na) atomicAdd(&kept_sum[0], (unsigned long long)na);
    if (a.counts && nb) atomicAdd(&kept_sum[1], (unsigned long long)nb);
  }
  __syncthreads();
  if constexpr (MIX) {
    if (a.counts && tid < 2 && kept_sum[tid]) atomicAdd(a.counts + (int64_t)b * 2 + tid, kept_sum[tid]);
  }

  // ---- the frame's band, in the wire format ------------------------------------------------------
  uint32_t gt = 0;
  if constexpr (OUT == SNNQP_U8) {
    uint8_t *dst = (uint8_t *)a.out + (fi * npix + p0) * 2;
    const int nbody = ((uintptr_t)dst & 7) == 0 ? (np & ~3) : 0;
    auto pair = [](uint32_t w) { return sat_half(w & 0xFFFFu, 255u) | (sat_half(w >> 16, 255u) << 8); };
    for (int i = tid * 4; i < nbody; i += nth * 4) {    // four pixels, eight bytes per lane
      const v4u w = *(const v4u *)(hist + i);
      *(v2u *)(dst + 2 * i) = (v2u){pair(w.x) | (pair(w.y) << 16), pair(w.z) | (pair(w.w) << 16)};
    }
    for (int i = nbody + tid; i < np; i += nth) {
      const uint32_t w = hist[i];
      dst[2 * i] = (uint8_t)sat_half(w & 0xFFFFu, 255u);
      dst[2 * i + 1] = (uint8_t)sat_half(w >> 16, 255u);
    }
  } else if constexpr (OUT == SNNQP_EV4) {
    uint8_t *dst = (uint8_t *)a.out + (fi * npix + p0);
    const int nbody = ((uintptr_t)dst & 3) == 0 ? (np & ~3) : 0;
    auto nib = [&](uint32_t w) {
      const uint32_t c0 = w & 0xFFFFu, c1 = w >> 16;
      gt |= (c0 > 15u) | (c1 > 15u);
      return sat_half(c0, 15u) | (sat_half(c1, 15u) << 4);
    };
    for (int i = tid * 4; i < nbody; i += nth * 4) {    // four pixels, four bytes per lane
      const v4u w = *(const v4u *)(hist + i);
      *(uint32_t *)(dst + i) = nib(w.x) | (nib(w.y) << 8) | (nib(w.z) << 16) | (nib(w.w) << 24);
    }
    for (int i = nbody + tid; i < np; i += nth) dst[i] = (uint8_t)nib(hist[i]);
  } else {
    // EV1: element (pixel * 2 + polarity) is bit (i & 31) of word (i >> 5), 16 pixels a word.  A
    // lane gathers the 8 bits of four pixels, the four lanes of a word OR theirs together (the
    // units of a word are in the loop together: nalloc / 4 and the stride are multiples of 4).
    const int64_t fwords = ((int64_t)npix + 15) >> 4;
    uint32_t *dst = (uint32_t *)a.out + fi * fwords + (p0 >> 4);
    for (int u = tid; u < nalloc / 4; u += nth) {
      const v4u w = *(const v4u *)(hist + 4 * u);
      uint32_t bits = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t c0 = w[k] & 0xFFFFu, c1 = w[k] >> 16;
        gt |= (c0 > 1u) | (c1 > 1u);
        bits |= ((c0 ? 1u : 0u) | (c1 ? 2u : 0u)) << (2 * k);
      }
      uint32_t word = bits << (8 * (lane & 3));
      word |= (uint32_t)__shfl_xor((int)word, 1);
      word |= (uint32_t)__shfl_xor((int)word, 2);
      if ((lane & 3) == 0) dst[u >> 2] = word;
    }
  }
  if constexpr (OUT != SNNQP_U8) {
    if (a.flags && __ballot(gt != 0) != 0 && lane == 0)
      atomicOr(a.flags, OUT == SNNQP_EV4 ? SNNQP_FLAG_GT_15 : SNNQP_FLAG_GT_ONE);
  }
}

// what snnqp_events_bin_mix adds to the augmenting launch's arguments
struct EventsMix {
  const int32_t *sample2, *start2;
  const snnqp_event_aug_t *aug2;
  const int32_t *box;
  int64_t *counts;
};

// more than 64 KiB of LDS (the 64 KiB band plus the slice bounds) needs the limit raised, once per
// device and kernel
template <int OUT, int VAR>
static int events_bin_launch(const EventsBinArgs &a, const snnqp_event_aug_t *aug, const EventsMix *mix, int64_t grid,
                             int threads, size_t lds, hipStream_t st) {
  if (lds + 64 > 65536) {
    static std::once_flag once[MAX_DEVICES];
    static hipError_t raised[MAX_DEVICES];
    const int dev = stream_device(st);
    SNNQP_REQUIRE(dev >= 0 && dev < MAX_DEVICES, SNNQP_EHIP,
                  "events_bin: device %d is outside the library's tables (%d devices)", dev, MAX_DEVICES);
    std::call_once(once[dev], [dev] {
      DeviceGuard guard(dev);
      raised[dev] = !guard.ok ? hipErrorInvalidDevice
                              : hipFuncSetAttribute((const void *)events_bin_kernel<OUT, VAR>,
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, EB_BAND_PIX * 4);
      if (raised[dev] != hipSuccess) (void)hipGetLastError();
    });
    SNNQP_REQUIRE(raised[dev] == hipSuccess, SNNQP_EHIP, "events_bin: cannot raise the LDS limit on device %d: %s",
                  dev, hipGetErrorString(raised[dev]));
  }
  EventsBinKernelArgs<VAR> ka;
  static_cast<EventsBinArgs &>(ka) = a;
  if constexpr (VAR != EB_PLAIN) ka.aug = aug;
  if constexpr (VAR == EB_MIX) {
    ka.sample2 = mix->sample2; ka.start2 = mix->start2; ka.aug2 = mix->aug2; ka.box = mix->box;
    ka.counts = (unsigned long long *)mix->counts;
  }
  hipLaunchKernelGGL((events_bin_kernel<OUT, VAR>), dim3((unsigned)grid), dim3(threads), lds, st, ka);
  SNNQP_CHECK_LAUNCH("events_bin_kernel");
  return SNNQP_OK;
}

// (mix: the mixing kernel, whatever aug is; else aug null: the plain kernel)
template <int OUT>
static int events_bin_launch(const EventsBinArgs &a, const snnqp_event_aug_t *aug, const EventsMix *mix, int64_t grid,
                             int threads, size_t lds, hipStream_t st) {
  if (mix) return events_bin_launch<OUT, EB_MIX>(a, aug, mix, grid, threads, lds, st);
  return aug ? events_bin_launch<OUT, EB_AUG>(a, aug, nullptr, grid, threads, lds, st)
             : events_bin_launch<OUT, EB_PLAIN>(a, nullptr, nullptr, grid, threads, lds, st);
}

// all three entry points: the checks, the geometry and the launch
static int events_bin(const uint32_t *addr, const int32_t *times, const int64_t *offsets, int32_t S,
                      const int32_t *sample, const int32_t *start, int32_t B, int mode, int32_t T,
                      int32_t step_us, int32_t H, int32_t W, float scale, const snnqp_event_aug_t *aug,
                      const EventsMix *mix, void *out, int out_type, int32_t *flags, snnqp_stream_t stream) {
  SNNQP_REQUIRE(S >= 0 && B >= 0 && T >= 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384, SNNQP_EINVAL,
                "events_bin: bad shape (S %d, B %d, T %d, H %d, W %d; H, W <= 16384)", S, B, T, H, W);
  SNNQP_REQUIRE(mode == 0 || mode == 1, SNNQP_EINVAL, "events_bin: mode must be 0 (number) or 1 (time)");
  SNNQP_REQUIRE(std::isfinite(scale) && scale > 0.0f, SNNQP_EINVAL, "events_bin: scale must be positive");
  SNNQP_REQUIRE(out_type == SNNQP_U8 || out_type == SNNQP_EV4 || out_type == SNNQP_EV1, SNNQP_EINVAL,
                "events_bin: out_type must be SNNQP_U8, SNNQP_EV4 or SNNQP_EV1");
  if (mode == 1) {
    SNNQP_REQUIRE(step_us > 0, SNNQP_EINVAL, "events_bin: step_us must be positive in time mode");
    SNNQP_REQUIRE(times && start, SNNQP_EINVAL, "events_bin: time mode needs times and start");
  }
  if (mix && mix->sample2) {
    SNNQP_REQUIRE(mix->box, SNNQP_EINVAL, "events_bin_mix: sample2 needs a box per row");
    SNNQP_REQUIRE(mode != 1 || mix->start2, SNNQP_EINVAL, "events_bin_mix: time mode with sample2 needs start2");
  }
  if (B == 0 || T == 0) return SNNQP_OK;
  // (addr may be null when no sample has an event: the kernel reads it only inside a sample's range)
  SNNQP_REQUIRE(offsets && sample && out, SNNQP_EINVAL, "events_bin: null argument");
  SNNQP_REQUIRE(((uintptr_t)addr & 3) == 0 && (out_type != SNNQP_EV1 || ((uintptr_t)out & 3) == 0), SNNQP_EINVAL,
                "events_bin: addr and EV1 frames must be 4-byte aligned");
  SNNQP_REQUIRE(((uintptr_t)aug & 3) == 0, SNNQP_EINVAL, "events_bin: the aug records must be 4-byte aligned");
  if (mix)
    SNNQP_REQUIRE(((uintptr_t)mix->aug2 & 3) == 0 && ((uintptr_t)mix->box & 3) == 0 && ((uintptr_t)mix->counts & 7) == 0,
                  SNNQP_EINVAL, "events_bin_mix: aug2 and box must be 4-byte aligned, counts 8-byte aligned");
  const int32_t npix = H * W;
  EventsBinArgs a;
  a.addr = addr; a.times = times; a.offsets = offsets; a.sample = sample; a.start = start;
  a.out = out; a.flags = flags; a.scale = scale;
  a.S = S; a.T = T; a.step_us = step_us; a.H = H; a.W = W; a.mode = mode;
  a.nbands = (npix + EB_BAND_PIX - 1) / EB_BAND_PIX;
  const int64_t grid = (int64_t)B * T * a.nbands;
  SNNQP_REQUIRE(grid < (1ll << 31), SNNQP_EINVAL, "events_bin: %lld workgroups, grid too large", (long long)grid);
  const int32_t band = npix < EB_BAND_PIX ? npix : EB_BAND_PIX;
  const size_t lds = (size_t)((band + 15) & ~15) * 4;
  const int threads = band <= 4096 ? 256 : 512;
  hipStream_t st = (hipStream_t)stream;
  if (out_type == SNNQP_U8) return events_bin_launch<SNNQP_U8>(a, aug, mix, grid, threads, lds, st);
  if (out_type == SNNQP_EV4) return events_bin_launch<SNNQP_EV4>(a, aug, mix, grid, threads, lds, st);
  return events_bin_launch<SNNQP_EV1>(a, aug, mix, grid, threads, lds, st);
}

}  // namespace snnqp

using namespace snnqp;

extern "C" {

int snnqp_events_bin(const uint32_t *addr, const int32_t *times, const int64_t *offsets, int32_t S,
                     const int32_t *sample, const int32_t *start, int32_t B, int mode, int32_t T,
                     int32_t step_us, int32_t H, int32_t W, float scale,
                     void *out, int out_type, int32_t *flags, snnqp_stream_t stream) {
  return events_bin(addr, times, offsets, S, sample, start, B, mode, T, step_us, H, W, scale, nullptr, nullptr, out,
                    out_type, flags, stream);
}

int snnqp_events_bin_aug(const uint32_t *addr, const int32_t *times, const int64_t *offsets, int32_t S,
                         const int32_t *sample, const int32_t *start, int32_t B, int mode, int32_t T,
                         int32_t step_us, int32_t H, int32_t W, float scale, const snnqp_event_aug_t *aug,
                         void *out, int out_type, int32_t *flags, snnqp_stream_t stream) {
  return events_bin(addr, times, offsets, S, sample, start, B, mode, T, step_us, H, W, scale, aug, nullptr, out,
                    out_type, flags, stream);
}

int snnqp_events_bin_mix(const uint32_t *addr, const int32_t *times, const int64_t *offsets, int32_t S,
                         const int32_t *sample, const int32_t *start, const snnqp_event_aug_t *aug,
                         const int32_t *sample2, const int32_t *start2, const snnqp_event_aug_t *aug2,
                         const int32_t *box, int64_t *counts, int32_t B, int mode, int32_t T, int32_t step_us,
                         int32_t H, int32_t W, float scale, void *out, int out_type, int32_t *flags,
                         snnqp_stream_t stream) {
  const EventsMix mix = {sample2, start2, aug2, box, counts};
  return events_bin(addr, times, offsets, S, sample, start, B, mode, T, step_us, H, W, scale, aug, &mix, out, out_type,
                    flags, stream);
}

}  // extern "C"
