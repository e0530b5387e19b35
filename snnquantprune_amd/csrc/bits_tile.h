// The operand layout of the bit-input 3x3 conv (conv3x3_bits.hip, the fused block, and its currents
// form conv3x3_currents.hip): a workgroup of four waves on one 4x8-pixel tile, wave w = output
// channels [32 w, +32), the K walk over the MFMA-tiled codes `wt`, the halo image in LDS and how a
// lane reads its A fragments from it.  The kernels keep what is theirs -- the pipeline around these
// steps and the epilogue.  gfx950 only.
//
// LDS image of one halo (10 x 6 pixels x Cin spike bits, expanded to the A format: fp4 through a
// byte -> 8-nibble LDS table, bytes by arithmetic): one plane per 64 fp4 / 32 byte channels (32 B per
// pixel), rows of 12 pixels, the two 16-byte halves (fp4: channel groups 2 p, 2 p + 1) swapped on odd
// rows: every tap/half offset is an instruction immediate and the reads are bank-conflict free.  An
// odd fp6 G leaves group G - 1 alone in the first half of the last plane; its k-steps pair two taps
// instead (pair_tap) and read it through lane bases of their own.  A 16-channel last group (fp6) is
// staged with its 8 bytes in both halves of its 16-byte slot; the two 8-byte pieces of a lane
// (k16_tap) come from the half that keeps the 32 lanes of a ds_read_b64 group on 64 different banks.
#pragma once
#include <type_traits>

#include "conv_tile.h"

namespace snnqp {

typedef __attribute__((address_space(3))) const v4i lds_cv4i_t;

constexpr int F6_PITCH = HPITCH;             // pixels per LDS halo row (10 used)
constexpr int F6_ROWS = 6;                   // halo rows of a 4x8 patch
constexpr int F6_NT = 256;                   // threads of a workgroup: 4 waves
constexpr int F6_PLANE = F6_ROWS * HPITCH * 32;   // one k-step plane of a halo image
constexpr int F6_TAB = FP4_TAB_BYTES;        // byte -> 8 fp4 nibbles (tile_util.h)

// 32 int8 codes in k order (lo = k 0..15, hi = k 16..31) -> 32 fp6 values, value j
// at bits [6j, 6j + 6) of 6 dwords (the B fragment of one lane for one k-step)
__device__ __forceinline__ void fp6_pack32(const v4i &lo, const v4i &hi, int (&d)[6]) {
  uint32_t t[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    t[i] = squeeze6(fp6_codes4((uint32_t)lo[i]));
    t[4 + i] = squeeze6(fp6_codes4((uint32_t)hi[i]));
  }
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    d[3 * g + 0] = (int)(t[4 * g] | (t[4 * g + 1] << 24));
    d[3 * g + 1] = (int)((t[4 * g + 1] >> 8) | (t[4 * g + 2] << 16));
    d[3 * g + 2] = (int)((t[4 * g + 2] >> 16) | (t[4 * g + 3] << 8));
  }
}

// FMT: the matrix instruction the contraction runs on
//   FMT_FP6: v_mfma_scale_f32_32x32x64_f8f6f4, fp4 spikes x fp6 codes (|code| <= 7), K = 64
//   FMT_I8 : v_mfma_i32_32x32x32_i8, byte spikes x int8 codes (any 8-bit code), K = 32
enum { FMT_FP6 = 0, FMT_I8 = 1 };

// fp6, odd G: the tap lane half h reads in pair k-step p of the last group -- (0, 3), (1, 4),
// (2, 5) one halo row apart, (6, 7), (8, -) one pixel apart; "tap 9" has zero codes
__host__ __device__ constexpr int pair_tap(int p, int h) { return p < 3 ? p + 3 * h : 2 * p + h; }

// fp6, 16-channel last group: the tap of piece i (k rows 32 h + 16 i .. + 15) of lane half h in
// k-step q = 0 .. 2 of that group -- h = 0: taps q and 6 + q (two halo rows apart), h = 1: tap
// 3 + q and nothing ("tap 9": zero codes; the piece re-reads tap 6 + q)
__host__ __device__ constexpr int k16_tap(int q, int h, int i) { return i == 0 ? q + 3 * h : h == 0 ? 6 + q : 9; }

// One K walk: instruction FMT over CIN input channels (a multiple of 16; `wt` is padded to whole
// 32-channel groups), in (tap, 32-channel group) pairs, two per fp6 k-step, one per int8 k-step.  A
// last group of which only the lower 16 channels can spike (CIN = 16, 48, 80, 112) is walked in (tap,
// 16-channel) units and the upper 16 rows of its tiles are not read: fp6 three k-steps of three
// units (k16_tap), int8 the five k-steps of the pair walk, one unit per lane half.
template <int FMT, int CIN>
struct BitsTile {
  static_assert(CIN % 16 == 0 && CIN >= 16 && CIN <= 128, "one to eight 16-channel half groups");
  static constexpr bool I8 = FMT == FMT_I8;
  typedef typename std::conditional<I8, v16i, v16f>::type acc_t;
  static constexpr int BR = I8 ? 4 : 6;                 // registers of one B fragment
  static constexpr int WPP = (CIN + 31) / 32;           // spike words (32-channel groups) per pixel
  static constexpr int GW = CIN / 32;                   // groups walked whole
  static constexpr bool HALF = CIN % 32 != 0;           // group GW: its lower 16 channels only
  static constexpr int NP = I8 ? WPP : (WPP + 1) / 2;   // planes of the halo image
  static constexpr int NPL = I8 ? GW : GW / 2;          // planes read whole: both lane halves at one tap
  // k-steps of the pair walk (pair_tap) over the first half of plane NPL: fp6, the last whole
  // group when their number is odd; int8, the lower 16 channels of a 16-channel last group
  static constexpr int PAIRS = (I8 ? HALF : GW % 2 == 1) ? 5 : 0;
  static constexpr int PGRP = I8 ? GW : GW - 1;         // the group the pair walk covers
  static constexpr int K16 = !I8 && HALF ? 3 : 0;       // fp6 k-steps over a 16-channel last group (k16_tap)
  static constexpr int KS = 9 * NPL + PAIRS + K16;      // MFMAs of one halo image
  static constexpr int NPD = NPL > 0 ? NPL : 1;         // (divisor of the whole-plane k-step index)
  static constexpr int HALO_B = NP * F6_PLANE;          // one halo image

  // B operand of the wave whose channels start at cout_base, lane = (n, h), for the whole launch:
  // k-step ks = NPL tap + kk (< 9 NPL) covers channels 64 kk .. +63 of the tap; lane (n, h) holds
  // k = 32 h + j, i.e. both 16-byte halves of int8 tile WPP tap + 2 kk + h; pair k-step 9 NPL + p:
  // lane half h holds group PGRP of tap pair_tap(p, h)
  // k16 k-step 9 NPL + PAIRS + q: lane half h holds rows 0 .. 15 of group GW's tiles of taps
  // k16_tap(q, h, 0) and k16_tap(q, h, 1)
  // (int8: k-step ks = GW tap + kk is int8 tile WPP tap + kk as it is, lane (n, h) holds
  // k = 16 h + j; pair k-step p: rows 0 .. 15 of group GW's tile of tap pair_tap(p, h))
  static __device__ __forceinline__ void load_b(int (&bf)[KS][BR], const int8_t *wt, int cout_base,
                                                bool wave_on, int n, int h) {
    const int lane = 32 * h + n;
    const v4i *wtile = (const v4i *)wt + (int64_t)(cout_base >> 5) * (9 * WPP) * 64;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if constexpr (I8) {
        const int ptap = pair_tap(ks - 9 * NPL, h);
        const bool pair = ks >= 9 * NPL;
        const int idx = pair ? (ptap * WPP + GW) * 64 + n : ((ks / NPD) * WPP + ks % NPD) * 64 + lane;
        const v4i t = wave_on && !(pair && ptap >= 9) ? wtile[idx] : v4i{0, 0, 0, 0};
        bf[ks][0] = t.x; bf[ks][1] = t.y; bf[ks][2] = t.z; bf[ks][3] = t.w;
      } else if (ks >= 9 * NPL + PAIRS) {
        const int q = ks - 9 * NPL - PAIRS;
        const int t0 = k16_tap(q, h, 0), t1 = k16_tap(q, h, 1);
        v4i lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
        if (wave_on) lo = wtile[(t0 * WPP + GW) * 64 + n];
        if (wave_on && t1 < 9) hi = wtile[(t1 * WPP + GW) * 64 + n];
        fp6_pack32(lo, hi, bf[ks]);
      } else {
        const int ptap = pair_tap(ks - 9 * NPL, h);
        const bool pair = ks >= 9 * NPL;
        const int ks8 = pair ? ptap * WPP + PGRP : (ks / NPD) * WPP + (ks % NPD) * 2 + h;
        v4i lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
        if (wave_on && !(pair && ptap >= 9)) {
          lo = wtile[ks8 * 64 + n];
          hi = wtile[ks8 * 64 + 32 + n];
        }
        fp6_pack32(lo, hi, bf[ks]);
      }
    }
  }

  // Lane bases of one halo image: what a lane adds an instruction immediate to
  struct Bases {
    uint32_t e, o, pv, ph, ka, kb;
    // ... of the image d bytes further on
    __device__ __forceinline__ Bases at(uint32_t d) const { return Bases{e + d, o + d, pv + d, ph + d, ka + d, kb + d}; }
  };
  // ... of the image at LDS address lds0.  Lane (n, h) is pixel (ty, tx) of the tile
  static __device__ __forceinline__ Bases bases(uint32_t lds0, int n, int h) {
    const int ty = ((n >> 2) & 1) | ((n >> 4) << 1);
    const int tx = (n & 3) | (((n >> 3) & 1) << 2);
    // A fragment of tap (dy, dx), half kk: pixel (ty + dy, tx + dx), 32 B per pixel, the two
    // 16-byte lane halves swapped on odd halo rows.  With the 12-pixel row pitch this makes
    // every ds_read_b128 of the wave bank-conflict free (tools/ubench/lds_conv_patterns.hip).
    const uint32_t pixb = lds0 + (uint32_t)((ty * F6_PITCH + tx) * 32);
    const uint32_t abase_even = pixb + (uint32_t)((h ^ (ty & 1)) * 16);       // dy = 0, 2
    const uint32_t abase_odd = pixb + (uint32_t)((h ^ (ty & 1) ^ 1) * 16);    // dy = 1
    // pair k-steps (first half of plane NPL): half h one halo row lower (taps p, p + 3) or one
    // pixel to the right (taps 6 + 2q, 7 + 2q); the same swizzle, so still conflict free
    const uint32_t abase_pv = pixb + (uint32_t)(h * F6_PITCH * 32 + ((ty ^ h) & 1) * 16);
    const uint32_t abase_ph = pixb + (uint32_t)(h * 32 + (ty & 1) * 16);
    // k16 k-steps (group GW: half GW & 1 of plane GW / 2, its 8 bytes in both halves of the 16-byte
    // slot): piece 0 at taps q / 3 + q (half h one halo row lower), piece 1 at tap 6 + q for both
    // halves.  The 8-byte half alternates every two halo rows, so that with the 16-byte swizzle the
    // four rows of a 32-lane group sit in four different quarters of a pixel's 32 bytes: every
    // ds_read_b64 is bank-conflict free (tests/test_conv_k16_cpu.py)
    const uint32_t abase_ka = pixb + (uint32_t)(h * F6_PITCH * 32 + (((GW ^ ty ^ h) & 1) * 16) +
                                                (((ty + h) >> 1) & 1) * 8);
    const uint32_t abase_kb = pixb + (uint32_t)((((GW ^ ty) & 1) * 16) + (((ty >> 1) & 1) ^ 1) * 8);
    return Bases{abase_even, abase_odd, abase_pv, abase_ph, abase_ka, abase_kb};
  }

  // Staging task of a thread: spike word wi of halo pixel (hy, hx), and where it lands
  struct Stage {
    int wi, hy, hx, wpm;   // wpm: spike words of a pixel in memory
    bool task;             // (the first F6_ROWS * HALO * WPP threads have one)
    uint32_t dst, tabl;    // LDS address in the image at lds0; this lane's copy of the fp4 table
    uint32_t sh2, sh3;     // fp4: the shifts of the word's third and fourth table read
  };
  // (tab: LDS address of the fp4 table, fp4_table_fill)
  static __device__ __forceinline__ Stage stage_task(uint32_t lds0, uint32_t tab, int tid, int Cin) {
    Stage s;
    const int s_pix = tid / WPP;
    s.wi = tid % WPP;
    s.task = tid < F6_ROWS * HALO * WPP;
    // a pixel has ceil(Cin / 32) spike words in memory; the groups beyond them (codes padded
    // wider than that, snnqp_weight_t.wt_cin) are zero spikes against zero codes
    s.wpm = (Cin + 31) >> 5;
    s.hy = s_pix / HALO, s.hx = s_pix % HALO;
    // fp4: word wi = half wi & 1 of plane wi >> 1; bytes: word wi = both halves of plane wi
    s.dst = lds0 + (uint32_t)((I8 ? s.wi : s.wi >> 1) * F6_PLANE + (s.hy * F6_PITCH + s.hx) * 32 +
                              ((((I8 ? 0 : s.wi) & 1) ^ (s.hy & 1)) * 16));
    s.tabl = fp4_table_lane(tab, tid & 63);
    // fp6, 16-channel last group: its 8 bytes (channels 0 .. 15: bytes 0, 1 of the word) twice; the
    // upper half of the word is not looked at
    s.sh2 = K16 && s.wi == GW ? 0u : 16u, s.sh3 = K16 && s.wi == GW ? 8u : 24u;
    return s;
  }

  // Expanding spike word sw, in two steps so that a pipeline can put them in different slots.
  // expand: fp4, the four table reads -- byte k of the word -> its entry in this lane's copy:
  // conflict-free whatever the bytes of the 32 lanes are (int8: nothing to read)
  static __device__ __forceinline__ void expand(const Stage &s, uint32_t sw, v4i &e) {
    if constexpr (!I8) {
      if (s.task) {
        e.x = (int)fp4_table_entry(s.tabl, sw & 0xFFu);
        e.y = (int)fp4_table_entry(s.tabl, (sw >> 8) & 0xFFu);
        if constexpr (K16 > 0) {
          e.z = (int)fp4_table_entry(s.tabl, (sw >> s.sh2) & 0xFFu);
          e.w = (int)fp4_table_entry(s.tabl, (sw >> s.sh3) & 0xFFu);
        } else {
          e.z = (int)fp4_table_entry(s.tabl, (sw >> 16) & 0xFFu);
          e.w = (int)fp4_table_entry(s.tabl, sw >> 24);
        }
      }
    }
  }
  // write: into the image bufoff bytes behind lds0 -- fp4, what expand read; int8, the word's bits
  // as bytes, the upper 16 channels in the other half of the pixel (swapped on odd rows)
  static __device__ __forceinline__ void write(const Stage &s, uint32_t bufoff, uint32_t sw, const v4i &e) {
    if (I8) {
      if (s.task) {
        const uint32_t d = s.dst + bufoff;
        *(lds_v4i_t *)(uintptr_t)d = expand16(sw & 0xFFFFu);        // channels 0..15
        *(lds_v4i_t *)(uintptr_t)(s.hy & 1 ? d - 16 : d + 16) = expand16(sw >> 16);
      }
    } else if (s.task) {
      *(lds_v4i_t *)(uintptr_t)(s.dst + bufoff) = e;
    }
  }

  // A fragment of k-step ks from the halo image whose lane bases are ib
  static __device__ __forceinline__ v4i a_read(const Bases &ib, int ks) {
    if (ks >= 9 * NPL + PAIRS) {                // k16 k-step: two 8-byte pieces
      typedef __attribute__((address_space(3))) const v2i lds_cv2i_t;
      const int q = ks - 9 * NPL - PAIRS;
      const uint32_t off = (uint32_t)((GW >> 1) * F6_PLANE + q * 32);
      const v2i p0 = *(lds_cv2i_t *)(uintptr_t)(ib.ka + off);
      const v2i p1 = *(lds_cv2i_t *)(uintptr_t)(ib.kb + off + 2 * F6_PITCH * 32);
      return v4i{p0.x, p0.y, p1.x, p1.y};
    }
    if (ks >= 9 * NPL) {                        // pair k-step: the padding half ("tap 9")
      const int p = ks - 9 * NPL;               // reads pixel (2, 3), inside the image
      const uint32_t off = (uint32_t)(NPL * F6_PLANE + (p < 3 ? p : 2 * F6_PITCH + 2 * (p - 3)) * 32);
      return *(lds_cv4i_t *)(uintptr_t)((p < 3 ? ib.pv : ib.ph) + off);
    }
    const int tap = ks / NPD;
    const uint32_t off = (uint32_t)((ks % NPD) * F6_PLANE + ((tap / 3) * F6_PITCH + tap % 3) * 32);
    return *(lds_cv4i_t *)(uintptr_t)(((tap / 3) & 1 ? ib.o : ib.e) + off);
  }

  // c + A fragment av x B fragment b.  fp6: the E8M0 block scales 2^(s - 127) of A and B are
  // instruction constants (127: 1)
  template <int SCALE_A, int SCALE_B>
  static __device__ __forceinline__ acc_t mfma(const v4i &av, const int (&b)[BR], const acc_t &c) {
    if constexpr (I8) {
      return __builtin_amdgcn_mfma_i32_32x32x32_i8(av, v4i{b[0], b[1], b[2], b[3]}, c, 0, 0, 0);
    } else {
      return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
          v8i{av.x, av.y, av.z, av.w, 0, 0, 0, 0}, v8i{b[0], b[1], b[2], b[3], b[4], b[5], 0, 0}, c,
          4 /* A: fp4 */, 2 /* B: fp6 */, 0, SCALE_A, 0, SCALE_B);
    }
  }
};

}  // namespace snnqp
