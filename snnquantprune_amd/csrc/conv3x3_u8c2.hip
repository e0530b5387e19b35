// Fused SpikingBlock for the first 3x3 / stride 1 / pad 1 QuantConv layer of the DVS128
// topology (examples/tcja/models.py:111-147, Cin = 2 event-count frames): implicit-GEMM
// int8 MFMA (v_mfma_i32_32x32x32_i8) + dequantisation + eval BatchNorm + neuron update +
// optional 2x2 max-pool, with the T loop inside the kernel (conv3x3_u8c2_kernel), the plan of
// a launch (u8c2_plan) and its launcher (launch_conv3x3_u8c2).  The checks and the dispatch both
// fused conv kernels share are in conv3x3_mfma.hip, the work queues in workqueue.hip.
//
// C/D layout of the MFMA: lane = output channel, register = pixel, so the per-channel
// dequant / BatchNorm constants are per-lane registers, the membrane potentials of a
// tile stay in 16 VGPRs for all T, and the v_cmp that thresholds a register *is* the
// packed spike word of two pixels (64-bit lane mask); pooling is an OR of those masks.
#include <type_traits>

#include "conv_tile.h"

namespace snnqp {

// ---------------------------------------------------------------------------
// u8 event-count input with Cin = 2 (the DVS polarity pair, conv0): K = 18 of
// one 32-deep MFMA step.  One MFMA feeds 1024 neuron updates, so the kernel is
// bound by the epilogue and everything else is kept off the VALU:
//  * the halo of ALL timesteps of a patch (a chunk of <= 32) is staged in LDS at
//    once, so the t loop has no global loads and no barriers;
//  * each timestep image holds the 10 x 10 x 2-byte halo twice, copy c with pixel
//    hx at byte 2 hx + 2 c of its 24-byte row: the 8 bytes that start at any pixel
//    are then a 4-byte-aligned ds_read2_b32 in the copy of the pixel's parity, and
//    a lane's A fragment is two such reads and no arithmetic:
//      half 0: k 0..7 = row dy 0, k 8..15 = row dy 1   (byte b = 2 dx + cin, b < 6)
//      half 1: k 16..23 = row dy 2, k 24..31 = constants {127,127,127,127,1,0,0,0}
//    bytes 6, 7 of a row read belong to the next pixel; their B rows are zero;
//  * the constant k rows carry the table address: B rows 24..28 of a channel sum
//    to the byte address of its entry of acc = 0 (C = 0, no accumulator preload).
//
// The table modes (LUTM, sized by the host for the input values it EXPECTS: the hint
// x_limit) are valid only while every staged input value is <= x_limit.  Nothing is
// trusted: while a chunk's halo sits in registers on its way to LDS the workgroup takes
// its maximum, and a chunk that holds a larger value (a hot pixel, event counts where
// binary frames were expected, a stale hint) runs the general path -- input as x - 128,
// arithmetic dequantisation, any count up to 255 -- for that chunk only.  The largest
// value a launch saw goes to x_seen[0] and the count of staged chunks by their largest value to
// x_seen[1..5] (<= 1, <= 2, <= 7, <= 31, above), from which the caller refines its next hint without
// ever waiting for it (no inspection pass, no host synchronisation before the launch).
// ---------------------------------------------------------------------------
constexpr int HROW2 = 24;                 // LDS bytes per halo row
constexpr int HCOPY2 = HALO * HROW2;      // one copy of one timestep
constexpr int HCONST2 = 2 * HCOPY2;       // the 8 constant bytes
constexpr int HIMG2 = 496;                // one timestep image
constexpr int TCHUNK = 32;                // most timesteps staged per pass
constexpr int U8C2_WPS = 4;               // waves per SIMD the kernel is compiled for (128 VGPRs)
constexpr int STG_N = TCHUNK / 2;           // timesteps a staging thread loads per chunk (every other one)

typedef int v2i_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef __attribute__((address_space(3))) const v2i_a4 lds_cv2i_t;

// LDS bytes of the u8c2 kernel: images | table | spike words
__host__ __device__ inline int u8c2_table_bytes(int lutm, int bound, int rows) {
  const int b = lutm == LUT_CHANNEL ? rows * 128 : lutm == LUT_SHARED ? (2 * bound + 2) * 4 : 0;
  return (b + 15) & ~15;
}

// IN: SNNQP_U8 (one byte per count) or SNNQP_EV1 (bit-packed binary frames, snnqp.h): the
// same kernel behind another staging loop.  EV1 frames cannot hold a value above 1, so the
// table modes need no check of the chunk (and the chunk no reduction, no atomic and one
// barrier less); a thread stages one halo ROW of one timestep -- 20 bits out of two words,
// expanded through a 256-entry byte -> 8-byte LDS table -- instead of one pixel.
// Waves per SIMD the variants are compiled for (profiles/r05_conv0_waves.txt).  The bit-packed
// variants: five.  With the potentials' life starting behind the staging code (template parameter
// ONE: nothing carried in or out, one chunk) they need about 90 registers and spill nothing: 4.95 ms
// on the headline layer against 5.32-5.35 for four waves (122 registers) on the same box; the
// general variant (potentials carried, several chunks) spills 31 dwords around its staging code at
// five waves and is still the faster one (5.10-5.18).
#ifndef SNNQP_U8C2_EV1_WPS
#define SNNQP_U8C2_EV1_WPS 5
#endif
// The byte formats' ONE variants: 102-103 registers and no scratch at four waves (128 with 40 bytes of
// scratch before the potentials moved behind the staging code): uint8 5.80 -> 5.56 ms, counts 5.85
// -> 5.67, nibbles 6.18 -> 6.00, float32 6.06 -> 5.85.  At five waves they spill 6 dwords per patch:
// 5.24 (uint8) / 5.51 (float32), counts unchanged (their tables leave LDS for four workgroups) --
// not taken while it costs scratch traffic.
#ifndef SNNQP_U8C2_ONE_WPS
#define SNNQP_U8C2_ONE_WPS 4
#endif
// SIX waves for the one variant that fits 80 registers without a spill -- bit-packed frames, ONE,
// per-channel tables, the tau = 2^j neuron with reset to 0, fused pool: the headline's -- with its
// table entries read in two halves (tile_epilogue_parts), tile 1's fragment and output word at
// immediate offsets from tile 0's and the wave index a scalar: 4.82-4.83 ms against 4.96-4.98 at
// five waves on the same box.  Its siblings would spill 2-6 dwords per patch at six: five.
#ifndef SNNQP_U8C2_EV1_ONE_WPS
#define SNNQP_U8C2_EV1_ONE_WPS 6
#endif
// The spread instances (below) with the fused pool: six, like the instance they stand in for.
#ifndef SNNQP_U8C2_SPREAD_WPS
#define SNNQP_U8C2_SPREAD_WPS 6
#endif
template <int NF, bool POOL, int LUTM, int IN, bool ONE, bool SPREAD = false>
constexpr int u8c2_waves() {
  if (SPREAD && POOL) return SNNQP_U8C2_SPREAD_WPS;
  if (IN == SNNQP_EV1 && ONE && LUTM == LUT_CHANNEL && NF == NF_MUL0 && POOL) return SNNQP_U8C2_EV1_ONE_WPS;
  if (IN == SNNQP_EV1) return SNNQP_U8C2_EV1_WPS;
  return ONE ? SNNQP_U8C2_ONE_WPS : U8C2_WPS;
}
// HALF (the half group): a launch whose weight says that the last 16 of its output
// channels never fire (snnqp_weight_t.cout_fire + 16 == Cout, Cout a multiple of 32).  The wave of
// the last 32 channels then computes 16 channels, and spends the lanes of the other 16 on a second
// pixel: lane n >= 16 holds the SAME channel as lane n - 16 with its taps one halo row lower (B: zeros
// in k 0..7, rows dy 0, 1, 2 in k 8..31), the A fragment is four halo rows Y .. Y + 3 of the patch's
// even image rows Y = 2 ty, and column n >= 16 of the product is the channel's accumulator at the pixel
// one image row below.  One MFMA and 16 potentials per lane cover the whole 8x8 patch: half the neuron
// updates.  All 32 k rows carry taps, so the table address comes in as the C operand; lane n >= 16 builds
// its twin's table (codes, BatchNorm) in its own slot.  The other waves, the staging, the barriers, the
// flush and the queue are the full path's.
//
// SPREAD (the wave spread): the launches of that family that would leave waves idle or
// unevenly loaded -- 64 channels (two waves idle), and 96 channels with the half group (32 / 32 / 16 /
// 0 registers of neuron updates per wave and timestep) -- with the same work on every wave.  The
// four (channel group g, tile) units of channels 0..63 go one to a wave: wave w computes tile w & 1 of
// group g = w >> 1, one MFMA and 16 potentials, and stores word g of that tile's pixels.  With HALF
// every wave also issues the half group's MFMA (the operands of the HALF wave above) and runs the
// epilogue on a quarter of its product: the columns 4 (w & 1) ..+3 of the image rows 4 g ..+3, which
// the wave brings into registers 0..3 by permuting the rows of its A operand (lane n reads the pixel
// of lane n ^ 8 w; EP_QUARTER, conv_tile.h), and stores word 2 of those pixels.  The matrix pipe, nearly
// idle in this kernel, computes that product four times; the vector work of a patch-step is the same
// and every wave carries 16 (+ 4) potentials.  The tables are built as ever, wave = channel group
// (wave 2: the half group's twins); a wave then takes the table addresses of the groups it computes
// from the scratch.  Staging, barriers, flush, queue and LDS plan are the full path's.
//
// Q16 (the quarter on a 16x16x64 matrix instruction; SPREAD with HALF): a wave's quarter
// IS the product of one v_mfma_i32_16x16x64_i8 -- 16 channels x 16 pixels in four registers -- so the wave
// issues that instead of the half group's whole 32x32x32 product: A row r = pixel r of its 4x4 quarter, B
// column c = channel 64 + c with the taps in lane groups 0 and 1, C = four registers of the table address
// (lane groups 1 and 3 read the twin's copy of the channel's table: 32 distinct banks per 32 lanes), and
// EP_QUARTER16 (conv_tile.h) places the words where EP_QUARTER does.
// The tap rule of the B operand: k row kk = 8 dy + b carries byte b = 2 dx + cin of halo row dy (b < 6:
// bytes 6, 7 of a row read belong to the next pixel), which meets weight row (3 dy + dx) * 2 + cin =
// 6 dy + b of HWIO with Cin = 2.  Whether kk is a tap, and its weight row.
__device__ __forceinline__ bool tap_row(int kk, int &row) {
  row = 6 * (kk >> 3) + (kk & 7);
  return kk >= 0 && kk < 24 && (kk & 7) < 6;
}

template <int NF, bool POOL, int LUTM, int IN = SNNQP_U8, bool ONE = false, bool HALF = false, bool SPREAD = false,
          bool Q16 = false>
__global__ void __launch_bounds__(256, (u8c2_waves<NF, POOL, LUTM, IN, ONE, SPREAD>()))
conv3x3_u8c2_kernel(ConvMfmaArgs a) {
  constexpr int FL = OutStage<POOL>::FL;
  constexpr bool EV1 = IN == SNNQP_EV1;
  static_assert(!(HALF || SPREAD) || (EV1 && ONE && LUTM == LUT_CHANNEL && NF == NF_MUL0),
                "the half group, the wave spread: bit-packed frames, one chunk, per-channel tables, NF_MUL0");
  static_assert(!Q16 || (HALF && SPREAD), "the 16x16x64 quarter: the spread launch with the half group");
  constexpr bool EV4 = IN == SNNQP_EV4;     // one byte per pixel: polarity 0 low nibble, 1 high
  // float32 frames as the reference hands them over (flax_qconv.py:101): eight bytes per pixel,
  // converted to the two count bytes and checked while they wait in registers (snnqp.h, x_flags)
  constexpr bool F32IN = IN == SNNQP_F32;
  static_assert(TCHUNK % FL == 0, "flush period must divide the staging chunk");
  // a predicated launch (snnqp_conv_lif_forward_pred: the frames again in their own format behind
  // a speculative bit-packed launch) returns at once unless the word is set -- before any
  // workgroup has touched a queue word, which therefore stay zero for the slot's next user
  if constexpr (!EV1) {
    if (a.pred && *(const volatile int32_t *)a.pred == 0) return;
  }
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tc = a.tchunk;                       // <= TCHUNK
  const int lut_off = tc * HIMG2;
  uint32_t *obuf = (uint32_t *)(lds + lut_off + u8c2_table_bytes(LUTM, a.lut_bound, a.lut_rows));
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // (scalar: what hangs on it stays out of the VGPRs)
  const int n = lane & 31, h = lane >> 5;
  const int cout_base = blockIdx.y * 128 + wave * 32;
  const bool wave_on = cout_base < a.Cout;
  const int cout = wave_on ? cout_base + n : n;
  const int cpar = cout < a.Cout ? cout : a.Cout - 1;      // parameter loads
  // (the channels from cout_fire on are the caller's silent ones: their bits are stored as zeros)
  uint32_t cmask = chan_mask(cout_base, a.cout_fire);
  // the wave of the half group (a scalar), and the channel whose codes and table this lane holds
  const bool half_wave = HALF && cout_base + 32 == a.Cout;
  const int ctab = half_wave && n >= 16 ? cout - 16 : cout;
  // workgroup words behind the spike-word ring:
  //   [0] smallest non-zero |input current| of this workgroup's channels (table kernels):
  //       decides whether the membrane update may be one fused multiply-add
  //   [1] largest input value of the chunk being staged   [2] the claimed next patch
  uint32_t *wgw = obuf + OutStage<POOL>::BYTES / 4;
  if (tid == 0) { wgw[0] = 0x7F800000u; wgw[1] = 0u; }
  // EV1: byte of 8 input bits -> 8 operand bytes, in the scale of the kernel's path: 16 x
  // (per-channel tables), 4 x (shared table), or x - 128 (no table: general path)
  typedef int v2i_a8 __attribute__((ext_vector_type(2)));
  v2i_a8 *xtab = (v2i_a8 *)(wgw + 4);
  if (EV1) {
    const uint32_t one = LUTM == LUT_CHANNEL ? 16u : LUTM == LUT_SHARED ? 4u : 0x81u;
    const uint32_t zero = LUTM == LUT_NONE ? 0x80u : 0u;
    uint32_t e[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j >> 2] |= (((uint32_t)tid >> j) & 1u ? one : zero) << (8 * (j & 3));
    xtab[tid] = v2i_a8{(int)e[0], (int)e[1]};       // 256 threads, 256 entries
  }
  if (LUTM != LUT_NONE) lds_barrier();
  // tables and constants become visible with the first staging barrier
  if (LUTM == LUT_SHARED) {
    build_lut((float *)(lds + lut_off), a.lut_bound, a.dq, tid);
    if (NF == NF_MUL0) {             // BatchNorm of every entry, per channel: may the update fuse?
      lds_barrier();
      atomicMin(wgw, lut_bn_min_bits((const float *)(lds + lut_off), a.lut_bound, a.bn,
                                     blockIdx.y * 128, a.Cout, tid, 256));
    }
  }
  int ch_row0 = 0, ch_col = 0;      // LUT_CHANNEL: the table row and column of this lane's entry of acc = 0
  int hg_row0 = 0, hg_col = 0;      // SPREAD: the same of this lane's channel of the half group
  if (LUTM == LUT_CHANNEL) {
    // what this lane's channel can accumulate: the sums of its positive and |negative| codes
    // (the lane halves hold k 0..15 and 16..23 of the same channel), times the largest input
    int pos = 0, neg = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      int row;
      if (tap_row(16 * h + j, row) && wave_on && cout < a.Cout) {      // (a wave beyond Cout: one row per lane)
        const int code = a.w[(int64_t)row * a.Cout + ctab];
        pos += code > 0 ? code : 0;
        neg += code < 0 ? -code : 0;
      }
    }
    pos += __shfl_xor(pos, 32);
    neg += __shfl_xor(neg, 32);
    uint32_t *scr = obuf;            // (the spike-word ring is not in use before the first patch)
    // the bank column of this channel's table and its place in the column's stack (conv_tile.h)
    int slot = 4 * n + wave;
    if (a.ch_slots) slot = a.ch_slots[blockIdx.y * 128 + wave * 32 + n] & 127;
    if (h == 0) {
      scr[slot] = (uint32_t)((pos + neg) * a.x_limit + 1);
      scr[128 + wave * 32 + n] = (uint32_t)(neg * a.x_limit);
      scr[256 + wave * 32 + n] = (uint32_t)slot;
    }
    lds_barrier();
    ch_col = slot >> 2;
    const int start = lut_column_start(scr, slot);
    int total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) total += (int)scr[(slot & ~3) + k];
    ch_row0 = start + neg * a.x_limit;
    if constexpr (SPREAD) {
      // the entries of acc = 0 this wave reads in the loop: channel n of its own group w >> 1, and of
      // the half group (group 2), as the waves of those groups just wrote them down
      auto entry_of = [&](int grp, int &row0, int &col) {
        int s = 4 * n + grp;
        if (a.ch_slots) s = a.ch_slots[blockIdx.y * 128 + grp * 32 + n] & 127;
        row0 = lut_column_start(scr, s) + (int)scr[128 + grp * 32 + n];
        col = s >> 2;
      };
      entry_of(wave >> 1, ch_row0, ch_col);
      if (HALF) entry_of(2, hg_row0, hg_col);
    }
    // a column taller than the launch reserved: snnqp_weight_t.ch_stack_max is below the codes it
    // came with.  Its entries are not written (reads beyond the allocation return zeros): wrong
    // currents, reported -- the next call fails until the status is reset (snnqp.h).
    if (total > a.lut_rows && a.status) *(volatile uint32_t *)a.status = SNNQP_STATUS_BOUND;
    const uint32_t mb = build_lut_channel<HALF>((float *)(lds + lut_off), scr, a.lut_rows, a.dq, a.bn,
                                                blockIdx.y * 128, a.Cout, tid);
    atomicMin(wgw, mb);
    lds_barrier();                   // the scratch becomes the spike-word ring again
  }
  if (tid < tc) {
    *(uint32_t *)(lds + tid * HIMG2 + HCONST2) = 0x7F7F7F7Fu;
    *(uint32_t *)(lds + tid * HIMG2 + HCONST2 + 4) = 0x00000001u;
  }

  // B operands.  Table path (`bf`): the codes (x 8 for per-channel tables) and, over the
  // constant k rows, the byte address of this lane's table entry of acc = 0 as 127 q + r
  // (rows 24..27 take q in parts of at most 127, row 28 takes r).  General path (`bfg`): the
  // plain codes; the input is taken as x - 128 (a signed int8 for every count up to 255;
  // padding pixels are x = 0 like any other) and 128 * sum_k w[k] is added back to the
  // accumulator in the epilogue (an integer below 2^24: exact in float32).
  // The half-group wave: all 32 k rows are taps (lanes n >= 16: the twin's, one halo row lower) and the
  // address goes in as C (tab0).
  float acc_off = 0.0f;
  int tab0 = 0;
  v4i bf, bfg;
  v4i bfh = {0, 0, 0, 0};           // SPREAD with HALF: the half group's B fragment (`bf`: the own group's)
  if constexpr (SPREAD) {
    // lane (n, h) holds k = 16 h .. 16 h + 15 of one channel: `shift` = 0, the address `bias` of its table
    // entry of acc = 0 in the constant rows (own group), or every k row a tap, `shift` = 8 for the twin
    // lanes n >= 16 (half group: the address is the C operand)
    auto taps = [&](int chan, int shift, bool all_taps, int bias) {
      int q = bias / 127;
      const int r = bias - 127 * q;
      int v[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        uint32_t pk = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 16 * h + 4 * d + j, kk = k - shift;
          uint32_t bv = 0;
          int row;
          if (all_taps || k < 24) {
            if (tap_row(kk, row)) bv = (uint8_t)(a.w[(int64_t)row * a.Cout + chan] * 8);
          } else if (k < 28) {
            const int part = q < 127 ? q : 127;
            q -= part;
            bv = (uint32_t)part;
          } else if (k == 28) {
            bv = (uint32_t)r;
          }
          pk |= bv << (8 * j);
        }
        v[d] = (int)pk;
      }
      return v4i{v[0], v[1], v[2], v[3]};
    };
    const int tbase = (int)lds_addr(lds) + lut_off;
    bf = taps(blockIdx.y * 128 + (wave >> 1) * 32 + n, 0, false, tbase + 4 * (ch_row0 * 32 + ch_col));
    bfg = bf;                       // (bit-packed frames within per-channel tables: no general path)
    if (HALF) {
      tab0 = tbase + 4 * (hg_row0 * 32 + hg_col);
      if constexpr (Q16) {
        // lane (c = lane & 15, kb = lane >> 4) holds bytes 16 kb ..+15 of channel 64 + c: byte j of group kb
        // meets byte j of group kb of A -- k rows 0..7, 8..15 (kb 0) and 16..23 (kb 1) are the halo rows dy 0,
        // 1, 2, every other byte is zero.  No twin lanes, no shifted taps.
        const int chan = blockIdx.y * 128 + 64 + (lane & 15), kb = lane >> 4;
        int v[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          uint32_t pk = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            int row;
            if (tap_row(16 * kb + 4 * d + j, row)) pk |= (uint32_t)(uint8_t)(a.w[(int64_t)row * a.Cout + chan] * 8) << (8 * j);
          }
          v[d] = (int)pk;
        }
        bfh = v4i{v[0], v[1], v[2], v[3]};
      } else {
        bfh = taps(blockIdx.y * 128 + 64 + (n & 15), n >= 16 ? 8 : 0, true, 0);
      }
    }
  } else {
    int bias = 0;
    if (LUTM == LUT_SHARED) bias = (int)lds_addr(lds) + lut_off + 4 * a.lut_bound;
    if (LUTM == LUT_CHANNEL)     // row of acc = 0 of this lane's channel, its column
      bias = (int)lds_addr(lds) + lut_off + 4 * (ch_row0 * 32 + ch_col);
    if (HALF) tab0 = bias;
    int q = bias / 127;
    const int r = bias - 127 * q;
    int wsum = 0;
    int v[4], vg[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      uint32_t pk = 0, pkg = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 16 * h + 4 * d + j;
        uint32_t bv = 0, bg = 0;
        int row;
        if (HALF && half_wave) {
          if (tap_row(n >= 16 ? k - 8 : k, row)) bv = (uint8_t)(a.w[(int64_t)row * a.Cout + ctab] * 8);
        } else if (k < 24) {
          if (tap_row(k, row) && cout < a.Cout) {
            const int code = a.w[(int64_t)row * a.Cout + cout];
            wsum += code;
            bg = (uint8_t)code;
            bv = (uint8_t)(LUTM == LUT_CHANNEL ? code * 8 : code);   // see build_lut_channel
          }
        } else if (k < 28) {
          const int part = q < 127 ? q : 127;
          q -= part;
          bv = (uint32_t)part;
        } else if (k == 28) {
          bv = (uint32_t)r;
        }
        pk |= bv << (8 * j);
        pkg |= bg << (8 * j);
      }
      v[d] = (int)pk;
      vg[d] = (int)pkg;
    }
    bf = v4i{v[0], v[1], v[2], v[3]};
    bfg = v4i{vg[0], vg[1], vg[2], vg[3]};
    // the two lane halves hold k 0..15 and 16..23 of the same channel
    acc_off = 128.0f * (float)(wsum + __shfl_xor(wsum, 32));
  }

  LaneConsts lc = {0.f, 1.f, 0.f, 0.f, a.nrn.vr};
  if (a.bn.mean) { lc.bmean = a.bn.mean[cpar]; lc.bmul = a.bn.mul[cpar]; lc.bbias = a.bn.bias[cpar]; }
  if (a.nrn.kind == SNNQP_NEURON_LIF) lc.dec = a.nrn.decay[cpar];

  const int ty = ((n >> 2) & 1) | ((n >> 4) << 1);
  const int tx = (n & 3) | (((n >> 3) & 1) << 2);
  // the two 8-byte reads of this lane's fragment (tile 1 is 4 halo rows further)
  const int cpy = tx & 1;
  const int px0 = (int)lds_addr(lds) + cpy * HCOPY2 + 2 * tx + 2 * cpy;
  // (the half-group wave: halo rows Y + 2 h and, at an immediate offset, Y + 2 h + 1 of image row Y = 2 ty)
  // (the wave that runs the half group's loop: under SPREAD every wave runs a quarter of it instead)
  const bool half_loop = half_wave && !SPREAD;
  const int tyh = half_loop ? 2 * ty : ty;
  int offA[2], offB[2];
#pragma unroll
  for (int tl = 0; tl < 2; ++tl) {
    offA[tl] = px0 + (tyh + 4 * tl + (h ? 2 : 0)) * HROW2;
    offB[tl] = h ? (int)lds_addr(lds) + HCONST2 : px0 + (ty + 4 * tl + 1) * HROW2;
  }
  // (the half-group wave reads no second fragment: the register carries its table address, the C operand)
  if (HALF && half_loop) offB[1] = tab0;
  const uint8_t *xb = (const uint8_t *)a.x;
  // (the half-group wave: lane = (pooled) pixel of the patch, sixteen or all sixty-four of them)
  int ob0 = (half_loop ? lane : out_pix<POOL>(0, lane)) * 4 + wave;
  int ob1 = out_pix<POOL>(1, lane) * 4 + wave;
  const bool store_lane = POOL ? lane < (half_loop ? 16 : 8) : (half_loop || lane < 32);
  // SPREAD: the own unit is tile w & 1 of group g = w >> 1 (fragment: offA[0], offB[0]; word g of the
  // tile's pixels: ob0, stored by `store_lane`, masked by `cmask`); the quarter of the half group reads
  // the four halo rows of the pixel of lane n ^ 8 w (offA[1], + HROW2; C: offB[1]) and leaves word 2 of
  // pixel (row 4 g + r, column 4 (w & 1) + i) in lane 4 r + i, pooled: of pixel (row 2 g + (lane >> 2),
  // column 2 (w & 1) + (lane & 1)) in lanes 0, 1, 4, 5 (ob1, `quarter_lane`, `qmask`)
  bool quarter_lane = false;
  uint32_t qmask = 0u;
  if constexpr (SPREAD) {
    const int g = wave >> 1, q = wave & 1;
    offA[0] = q ? offA[1] : offA[0];
    offB[0] = q ? offB[1] : offB[0];
    ob0 = out_pix<POOL>(q, lane) * 4 + g;
    cmask = chan_mask(blockIdx.y * 128 + g * 32, a.cout_fire);
    if (HALF) {
      const int np = n ^ (8 * wave);
      const int typ = ((np >> 2) & 1) | ((np >> 4) << 1), txp = (np & 3) | (((np >> 3) & 1) << 2);
      offA[1] = (int)lds_addr(lds) + cpy * HCOPY2 + 2 * txp + 2 * cpy + (2 * typ + 2 * h) * HROW2;
      if constexpr (Q16) {
        // row r = lane & 15 of A is pixel r of the quarter, block r >> 2 of its 2x2 pool blocks and place
        // r & 3 inside it (EP_QUARTER16, conv_tile.h); lane group kb reads halo rows 2 (kb & 1) and, an
        // immediate HROW2 further, 2 (kb & 1) + 1 below the pixel's: dy 0, 1 (kb 0) and dy 2 with the row
        // under it (kb 1; LDS of this image or the next bytes of the allocation, met by zeros of B, as are
        // all bytes of kb 2, 3)
        const int rq = lane & 15, kb = lane >> 4;
        const int py = 4 * g + 2 * (rq >> 3) + ((rq >> 1) & 1), px = 4 * q + 2 * ((rq >> 2) & 1) + (rq & 1);
        const int cq = px & 1;
        offA[1] = (int)lds_addr(lds) + cq * HCOPY2 + 2 * px + 2 * cq + (py + 2 * (kb & 1)) * HROW2;
      }
      offB[1] = tab0;
      const int pix = POOL ? (2 * g + ((lane >> 2) & 1)) * 4 + 2 * q + (lane & 1)
                           : (4 * g + ((lane >> 2) & 3)) * 8 + 4 * q + (lane & 3);
      ob1 = pix * 4 + 2;
      quarter_lane = POOL ? lane < 8 && (lane & 2) == 0 : lane < 16;
      qmask = chan_mask(blockIdx.y * 128 + 64, a.cout_fire);
    }
  }
  uint32_t seen = 0;                       // largest input value this thread's waves met
  // staged chunks by their largest value: <= 1, <= 2, <= 7, <= 31, above (workgroup-uniform
  // counters; they reach x_seen[1..5] once, at the end of the launch)
  uint32_t hist[6] = {0, 0, 0, 0, 0, 0};
  // staging tasks: waves 0-1 take the even timesteps of a chunk, waves 2-3 the odd ones; the
  // first 100 threads of each pair take one halo pixel each.  The timestep is uniform over a
  // wave, so a load is a scalar frame address plus this thread's 32-bit pixel offset.
  const int s_pix = tid & 127;
  const bool s_task = s_pix < HALO * HALO;
  const int s_half = __builtin_amdgcn_readfirstlane(tid >> 7);
  const int s_dst = (s_pix / HALO) * HROW2 + (s_pix % HALO) * 2;

  PatchWalk pw(a);
  // patch indices (+ one grid stride) stay below 2^31 (run_conv3x3_mfma refuses launches of
  // 2^30 patches or more) and are workgroup-uniform: scalar registers
  int r = __builtin_amdgcn_readfirstlane((int)pw.first);
  uint32_t processed = 0;                       // patches of this workgroup (scalar)
  while (r < (int)pw.count) {
    ++processed;
    int claimed = 0;
    if (pw.queue && tid == 0) claimed = (int)pw.claim();   // next patch, a patch ahead
    int b, y0, x0;
    pw.decode(a, r, b, y0, x0);

    // ONE: no potentials carried in or out and all timesteps in one chunk -- the potentials then
    // start their life behind the staging code instead of through it (32 registers the staging
    // does not have to work around)
    float u[2][16];
    if constexpr (!ONE) {
      if (a.u0 && wave_on) u_io<true>(u, a, b, y0, x0, cout, h);
      else zero_u(u);
    }
    uint32_t pseen = 0;                  // largest input value of this patch so far
    const int s_gy = y0 + s_pix / HALO - 1, s_gx = x0 + s_pix % HALO - 1;
    const bool s_valid = s_task && s_gy >= 0 && s_gy < a.H && s_gx >= 0 && s_gx < a.W;
    // byte offset of the pixel within a frame (frames are below 2 GiB: launch check); threads
    // without a pixel read the frame's first one and drop it
    const uint32_t s_off = s_valid ? (uint32_t)(s_gy * a.W + s_gx) * (EV4 ? 1u : F32IN ? 8u : 2u) : 0u;
    const uint8_t *s_frames = xb + (int64_t)b * a.xs_b * (F32IN ? 4 : 1);
    // EV1: the 20 bits of a halo row start `lead` bits before pixel x0 of the row (none when
    // x0 = 0: the pixel left of the image does not exist); pixels outside the image are
    // cleared by a mask of two bits per halo column (workgroup-uniform: scalars)
    const uint32_t e_lead = x0 > 0 ? 2u : 0u;
    const int e_hi = min(HALO - 1, a.W - x0);                  // last halo column inside the image
    const uint32_t e_colmask = ((1u << (2 * (e_hi + 1))) - 1u) & ~((1u << (2 - (int)e_lead)) - 1u);
    const uint32_t e_fwords = (uint32_t)(((int64_t)a.H * a.W * 2 + 31) >> 5);
    const uint32_t *e_frames = (const uint32_t *)a.x + (int64_t)b * a.xs_b;

    for (int t0 = 0; t0 < a.T; t0 += tc) {
      const int nt = min(tc, a.T - t0);
      bool general = LUTM == LUT_NONE;
      if constexpr (EV1) {
        // ---- stage the chunk from bit-packed frames: one (timestep, halo row) per thread ----
        lds_barrier();                     // previous readers of the LDS images are done
        for (int task = tid; task < nt * HALO; task += 256) {
          const int tt = task / HALO, hy = task - tt * HALO;
          const int gy = y0 + hy - 1;
          const bool rv = gy >= 0 && gy < a.H;
          const uint32_t start = (uint32_t)((rv ? gy : 0) * a.W + x0) * 2u - e_lead;
          const uint32_t wi = start >> 5;
          const uint32_t *f = e_frames + (int64_t)(t0 + tt) * a.xs_t;
          // (the word behind the frame's last one is never needed: its bits would be pixels
          // beyond the image, which the mask clears)
          const uint32_t lo = f[wi], hi = f[min(wi + 1u, e_fwords - 1u)];
          uint32_t v = __builtin_amdgcn_alignbit(hi, lo, start & 31u);
          v = (v << (2u - e_lead)) & (rv ? e_colmask : 0u);
          const v2i_a8 d0 = xtab[v & 0xFFu], d1 = xtab[(v >> 8) & 0xFFu], d2 = xtab[(v >> 16) & 0xFu];
          uint8_t *row = lds + tt * HIMG2 + hy * HROW2;
          *(v2i_a8 *)row = d0;
          *(v2i_a8 *)(row + 8) = d1;
          *(v2i_a8 *)(row + 16) = d2;
          // copy 1: the same bytes two to the right (pixel hx at byte 2 hx + 2)
          const uint32_t q0 = (uint32_t)d0.x, q1 = (uint32_t)d0.y, q2 = (uint32_t)d1.x,
                         q3 = (uint32_t)d1.y, q4 = (uint32_t)d2.x, q5 = (uint32_t)d2.y;
          uint8_t *row1 = row + HCOPY2;
          *(v2i_a8 *)row1 = v2i_a8{(int)(q0 << 16), (int)__builtin_amdgcn_alignbit(q1, q0, 16)};
          *(v2i_a8 *)(row1 + 8) = v2i_a8{(int)__builtin_amdgcn_alignbit(q2, q1, 16),
                                         (int)__builtin_amdgcn_alignbit(q3, q2, 16)};
          *(v2i_a8 *)(row1 + 16) = v2i_a8{(int)__builtin_amdgcn_alignbit(q4, q3, 16),
                                          (int)__builtin_amdgcn_alignbit(q5, q4, 16)};
        }
        lds_barrier();
      } else {
      // ---- stage the chunk: load, take the maximum, choose the path, write ----
      // Thread = one halo pixel (both polarities: 2 bytes) of every other timestep: its only
      // per-patch state is one source pointer, so nothing else is live while the byte pairs
      // wait in registers for the workgroup to agree on the path.
      uint32_t v[STG_N];
      uint32_t mx = 0;
      if constexpr (F32IN) {
        // two rounds of STG_N / 2 eight-byte loads: the raw pairs need two registers each
        uint32_t fbad = 0;
#pragma unroll
        for (int r0 = 0; r0 < STG_N; r0 += STG_N / 2) {
          typedef float f2v __attribute__((ext_vector_type(2)));
          f2v raw[STG_N / 2];
#pragma unroll
          for (int i = r0; i < r0 + STG_N / 2; ++i) {
            const int tt = 2 * i + s_half;
            raw[i - r0] = f2v{0.0f, 0.0f};
            if (tt < nt) raw[i - r0] = *(const f2v *)(s_frames + (int64_t)(t0 + tt) * a.xs_t * 4 + s_off);
          }
#pragma unroll
          for (int i = r0; i < r0 + STG_N / 2; ++i) {
            // fl(cvt(x)) - x is +0.0 exactly for the integers v_cvt_u32_f32 holds (-0.0 counts
            // as 0), NaN for NaN, non-zero otherwise; the range is checked on the integers
            const f2v f = raw[i - r0];
            const uint32_t ua = __float2uint_rz(f.x), ub = __float2uint_rz(f.y);
            fbad |= __float_as_uint(__uint2float_rn(ua) - f.x) | __float_as_uint(__uint2float_rn(ub) - f.y);
            fbad |= (ua | ub) >> 8;
            v[i] = (ua & 0xFFu) | ((ub & 0xFFu) << 8);
          }
        }
        fbad = s_valid ? fbad : 0u;
        if (__ballot(fbad != 0u) != 0ull && lane == 0 && a.x_flags) atomicOr(a.x_flags, SNNQP_FLAG_NOT_INTEGER);
      } else {
#pragma unroll
      for (int i = 0; i < STG_N; ++i) {    // all loads first; the skip is a scalar branch
        const int tt = 2 * i + s_half;
        v[i] = 0;
        if (tt < nt) {
          if constexpr (EV4) {           // nibble-packed counts: the two bytes the uint8 frame would hold
            const uint32_t pb = *(s_frames + (int64_t)(t0 + tt) * a.xs_t + s_off);
            v[i] = (pb | (pb << 4)) & 0x0F0Fu;          // 0xHL -> 0x0H0L
          } else {
            v[i] = *(const uint16_t *)(s_frames + (int64_t)(t0 + tt) * a.xs_t + s_off);
          }
        }
      }
      }
#pragma unroll
      for (int i = 0; i < STG_N; ++i) {
        v[i] = s_valid ? v[i] : 0u;
        mx = max(mx, max(v[i] & 0xFFu, v[i] >> 8));
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
      // The halo is written in the scale of the path the hint EXPECTS (round 5; it used to wait
      // for the workgroup's verdict: a barrier more per chunk, and every write behind the
      // reduction) while the chunk's maximum travels through an LDS atomic; a chunk that exceeds
      // the hint -- rare by construction of the hint -- is loaded and written again in the
      // general path's scale.
      // (every wave read the last chunk's maximum before the barriers of its run_chunk)
      if (tid == 0) wgw[1] = 0u;
      lds_barrier();                       // previous readers of the LDS images are done
      if (s_task) {
#pragma unroll
        for (int i = 0; i < STG_N; ++i) {
          const int tt = 2 * i + s_half;
          if (tt < nt) {    // table modes: both bytes scale without a carry (counts <= 31 / 7)
            const uint16_t val = (uint16_t)(LUTM == LUT_NONE      ? v[i] ^ 0x8080u    // x - 128
                                            : LUTM == LUT_CHANNEL ? v[i] << 4
                                                                  : v[i] << 2);
            uint8_t *p = lds + tt * HIMG2 + s_dst;
            *(uint16_t *)p = val;
            *(uint16_t *)(p + HCOPY2 + 2) = val;
          }
        }
      }
      if (lane == 0 && mx != 0) atomicMax(&wgw[1], mx);
      lds_barrier();
      const uint32_t cmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)wgw[1]);   // one word
      seen = max(seen, cmax);
      pseen = max(pseen, cmax);
      hist[0] += cmax <= 1u;
      hist[1] += cmax == 2u;
      hist[2] += cmax > 2u && cmax <= 7u;
      hist[3] += cmax > 7u && cmax <= 31u;
      hist[4] += cmax > 31u;
      hist[5] += cmax == 3u;
      general = LUTM == LUT_NONE || cmax > (uint32_t)a.x_limit;
      if (LUTM != LUT_NONE && general) {
        // the rare chunk: its values again (an L2 hit; nothing was kept in registers for it)
        if (s_task) {
#pragma unroll 1
          for (int tt = s_half; tt < nt; tt += 2) {
            uint32_t w2 = 0;
            if (s_valid) {
              if constexpr (F32IN) {
                typedef float f2v __attribute__((ext_vector_type(2)));
                const f2v f = *(const f2v *)(s_frames + (int64_t)(t0 + tt) * a.xs_t * 4 + s_off);
                w2 = (__float2uint_rz(f.x) & 0xFFu) | ((__float2uint_rz(f.y) & 0xFFu) << 8);
              } else if constexpr (EV4) {
                const uint32_t pb = *(s_frames + (int64_t)(t0 + tt) * a.xs_t + s_off);
                w2 = (pb | (pb << 4)) & 0x0F0Fu;
              } else {
                w2 = *(const uint16_t *)(s_frames + (int64_t)(t0 + tt) * a.xs_t + s_off);
              }
            }
            const uint16_t val = (uint16_t)(w2 ^ 0x8080u);
            uint8_t *p = lds + tt * HIMG2 + s_dst;
            *(uint16_t *)p = val;
            *(uint16_t *)(p + HCOPY2 + 2) = val;
          }
        }
        lds_barrier();
      }
      }
      // the FL-step blocks of the chunk: table path (with the membrane update as a fused
      // multiply-add where that is proven bit-identical for this launch) or general path
      auto run_chunk = [&](auto mode_tag, auto fma_tag) {
      constexpr int MODE = decltype(mode_tag)::value;
      constexpr bool FMA = decltype(fma_tag)::value;
      constexpr bool OFFS = MODE == LUT_NONE;
      const v4i bw = OFFS ? bfg : bf;
      if constexpr (SPREAD) {
        // every wave: its own (group, tile) unit, then its quarter of the half group's product
        int ctab0 = offB[1];
        asm volatile("" : "+v"(ctab0));
        // (made per patch, like the half-group wave's; only registers 0..3 of the product are read, so only
        // those of C are given a value: the other twelve need no register of their own)
        const v4i c4 = {ctab0, ctab0, ctab0, ctab0};
        const v16i c0 = __builtin_shufflevector(c4, c4, 0, 1, 2, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
        for (int tf = 0; tf < nt; tf += FL) {
          const int nf = min(FL, nt - tf);
#pragma unroll 1
          for (int tt = tf; tt < tf + nf; ++tt) {
            const uint32_t img = (uint32_t)(tt * HIMG2);
            uint32_t *o = obuf + ((t0 + tt) % FL) * (OutStage<POOL>::NPIX * 4);
            {
              const v2i_a4 lo = *(lds_cv2i_t *)(uintptr_t)(img + (uint32_t)offA[0]);
              const v2i_a4 hi = *(lds_cv2i_t *)(uintptr_t)(img + (uint32_t)offB[0]);
              v16i acc = splat16(0);
              acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4i{lo.x, lo.y, hi.x, hi.y}, bw, acc, 0, 0, 0);
              const uint32_t word = tile_epilogue_parts<NF, POOL, MODE, FMA, OFFS, EP_TILE, 4, 2>(
                  acc, u[0], a.dq, lc, a.nrn, lane, acc_off);
              if (store_lane) o[ob0] = word & cmask;
            }
            if constexpr (Q16) {
              const v2i_a4 lo = *(lds_cv2i_t *)(uintptr_t)(img + (uint32_t)offA[1]);
              const v2i_a4 hi = *(lds_cv2i_t *)(uintptr_t)(img + (uint32_t)offA[1] + (uint32_t)HROW2);
              const v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(v4i{lo.x, lo.y, hi.x, hi.y}, bfh, c4, 0, 0, 0);
              const uint32_t word = quarter16_epilogue<NF, POOL, MODE, FMA, OFFS>(acc, u[1], a.dq, lc, a.nrn, acc_off);
              if (quarter_lane) o[ob1] = word & qmask;
            } else if constexpr (HALF) {
              const v2i_a4 lo = *(lds_cv2i_t *)(uintptr_t)(img + (uint32_t)offA[1]);
              const v2i_a4 hi = *(lds_cv2i_t *)(uintptr_t)(img + (uint32_t)offA[1] + (uint32_t)HROW2);
              const v16i acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4i{lo.x, lo.y, hi.x, hi.y}, bfh, c0,
                                                                     0, 0, 0);
              const uint32_t word = tile_epilogue_parts<NF, POOL, MODE, FMA, OFFS, EP_QUARTER, 2, 1>(
                  acc, u[1], a.dq, lc, a.nrn, lane, acc_off);
              if (quarter_lane) o[ob1] = word & qmask;
            }
          }
          lds_barrier();
          flush_out<POOL>(obuf, a, t0 + tf, nf, b, y0, x0, tid);
          lds_barrier();
        }
        return;
      }
      if constexpr (HALF) {
        // the wave of the half group, on a scalar branch: one MFMA from C = the table address, 16
        // potentials, one word per (pooled) pixel of the patch; the barriers and the flush are the
        // other waves'
        if (half_loop) {
          // (sixteen registers, made per patch: as a loop invariant they would live through the staging code)
          int ctab0 = offB[1];
          asm volatile("" : "+v"(ctab0));
          const v16i c0 = splat16(ctab0);
          for (int tf = 0; tf < nt; tf += FL) {
            const int nf = min(FL, nt - tf);
#pragma unroll 1
            for (int tt = tf; tt < tf + nf; ++tt) {
              const uint32_t img = (uint32_t)(tt * HIMG2);
              const v2i_a4 lo = *(lds_cv2i_t *)(uintptr_t)(img + (uint32_t)offA[0]);
              const v2i_a4 hi = *(lds_cv2i_t *)(uintptr_t)(img + (uint32_t)offA[0] + (uint32_t)HROW2);
              const v16i acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4i{lo.x, lo.y, hi.x, hi.y}, bw, c0,
                                                                     0, 0, 0);
              const uint32_t word = tile_epilogue_parts<NF, POOL, MODE, FMA, OFFS, EP_HALFW, 4, 2>(
                  acc, u[0], a.dq, lc, a.nrn, lane, acc_off);
              if (store_lane) {
                uint32_t *o = obuf + ((t0 + tt) % FL) * (OutStage<POOL>::NPIX * 4);
                o[ob0] = word & cmask;
              }
            }
            lds_barrier();
            flush_out<POOL>(obuf, a, t0 + tf, nf, b, y0, x0, tid);
            lds_barrier();
          }
          return;
        }
      }
      for (int tf = 0; tf < nt; tf += FL) {          // FL steps, then flush
        const int nf = min(FL, nt - tf);
        // a wave beyond Cout (a launch of 32, 64 or 96 channels: a compacted block)
        // has no channel to compute: it stages, flushes and takes the barriers, nothing else.  The
        // waves of a workgroup start on a varying SIMD, so the freed issue slots spread evenly
        // over the SIMDs (a scalar branch: `wave` and Cout are uniform)
#pragma unroll 1
        for (int tt = tf; tt < (wave_on ? tf + nf : tf); ++tt) {
          const uint32_t img = (uint32_t)(tt * HIMG2);
          uint32_t words[2];
#pragma unroll
          for (int tl = 0; tl < 2; ++tl) {
            // (tile 1 is four halo rows below tile 0: an immediate offset of the read, no register)
            const v2i_a4 lo = *(lds_cv2i_t *)(uintptr_t)(img + (uint32_t)offA[0] + (uint32_t)(tl * 4 * HROW2));
            const v2i_a4 hi = *(lds_cv2i_t *)(uintptr_t)(img + (uint32_t)offB[tl]);
            v16i acc = splat16(0);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4i{lo.x, lo.y, hi.x, hi.y}, bw, acc,
                                                        0, 0, 0);
            // (the six-wave build reads its table entries in two halves: eight in flight, not sixteen)
            if constexpr (u8c2_waves<NF, POOL, LUTM, IN, ONE>() >= 6)
              words[tl] = tile_epilogue_parts<NF, POOL, MODE, FMA, OFFS, EP_TILE, 4, 2>(acc, u[tl], a.dq, lc, a.nrn,
                                                                                        lane, acc_off);
            else
              words[tl] = tile_epilogue<NF, POOL, MODE, FMA, OFFS>(acc, u[tl], a.dq, lc, a.nrn,
                                                                     lane, acc_off);
          }
          if (store_lane) {
            uint32_t *o = obuf + ((t0 + tt) % FL) * (OutStage<POOL>::NPIX * 4);
            o[ob0] = words[0] & cmask;
            o[ob0 + (POOL ? 32 : 128)] = words[1] & cmask;       // out_pix(1, lane) = out_pix(0, lane) + 8 / + 32
          }
        }
        lds_barrier();
        flush_out<POOL>(obuf, a, t0 + tf, nf, b, y0, x0, tid);
        lds_barrier();
      }
      };
      if constexpr (ONE) zero_u(u);
      if (general) {
        run_chunk(std::integral_constant<int, LUT_NONE>{}, std::false_type{});
      } else if constexpr (LUTM != LUT_NONE) {
        // a patch whose earlier chunk took the general path holds potentials the table
        // path's power-of-two argument does not cover: fused only while the whole patch
        // so far stayed within the tables
        const bool fma_ok = NF == NF_MUL0 && pseen <= (uint32_t)a.x_limit &&
                            lif_fma_is_exact(wgw[0], a.nrn.k_log2, a.T, a.u0 != nullptr);
        if (fma_ok) run_chunk(std::integral_constant<int, LUTM>{}, std::true_type{});
        else run_chunk(std::integral_constant<int, LUTM>{}, std::false_type{});
      }
      if constexpr (ONE) break;          // (a.T <= tc: the launcher's condition for this variant)
    }
    if (!ONE && a.u_out && wave_on) u_io<false>(u, a, b, y0, x0, cout, h);
    int r_next = r + (int)pw.stride;
    if (pw.queue) {                      // the claimed patch, to the whole workgroup
      if (tid == 0) wgw[2] = (uint32_t)claimed;
      lds_barrier();
      r_next = __builtin_amdgcn_readfirstlane((int)wgw[2]);
    }
    r = r_next;
  }
  if (a.x_seen && tid == 0) {
    if (seen != 0) atomicMax(a.x_seen, seen);
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (hist[k] != 0) atomicAdd((uint32_t *)a.x_seen + 1 + k, hist[k]);
  }
  if (pw.queue && tid == 0) pw.finish(processed, a.npatch, a.status);
}

// ---------------------------------------------------------------------------
// host side: the plan of a launch and the launcher run_conv3x3_mfma (conv3x3_mfma.hip) hands over to
// ---------------------------------------------------------------------------

// What an event-layer launch is made of -- table mode, staging chunk, LDS bytes, the ONE, HALF,
// SPREAD and Q16 variants -- decided in one place for the launch and for the predicates
// snnqp_conv_event_half_group / snnqp_conv_event_wave_spread / snnqp_conv_event_quarter16.
namespace {
struct U8c2Plan {
  int32_t x_limit, lut_bound, lut_rows, tchunk;
  bool lut, lutc, one, half, spread, quarter16;
  size_t ldsb;
};
U8c2Plan u8c2_plan(int in_type, int32_t T, int32_t Cout, const snnqp_weight_t *w, int nf, bool has_state,
                   bool pl, int x_max) {
  U8c2Plan p;
  // |acc| <= abs_sum_max * x_max; small enough -> dequantise through an LDS table
  // (the A operand then carries 4 * x, which must stay an int8).  For U8 input x_max is the
  // value the caller EXPECTS not to be exceeded (0 / unknown: binary events); the kernel
  // checks every chunk it stages and runs the general path where the hint does not hold
  const bool ev1 = in_type == SNNQP_EV1;
  const int64_t xm = ev1 ? 1 : (x_max > 0 ? x_max : 1);
  p.x_limit = (int32_t)(xm > 255 ? 255 : xm);
  const int64_t bound = (int64_t)w->abs_sum_max * xm;
  p.lut = w->abs_sum_max > 0 && xm > 0 && xm <= LUT_XMAX && bound <= LUT_CAP;
  p.lut_bound = p.lut ? (int32_t)bound : 0;
  p.tchunk = T >= TCHUNK ? TCHUNK : T;
  // images | table | spike-word ring | 4 workgroup words | EV1: byte -> 8-byte table
  const size_t lds_fixed = (size_t)p.tchunk * HIMG2 + 16 + (ev1 ? 2048 : 0) +
                           (pl ? OutStage<true>::BYTES : OutStage<false>::BYTES);
  // per-channel tables (BatchNorm folded in; the accumulator counts table rows of 128 B: A = 16 x
  // input, B = 8 x code), every channel over its own accumulator range, stacked per LDS bank
  // (conv_tile.h build_lut_channel): ch_stack_max x the largest input + 4 rows -- 8 x abs_sum_max
  // bounds it when the caller does not know
  const int64_t stack = w->ch_stack_max > 0 ? (int64_t)w->ch_stack_max : 8 * (int64_t)w->abs_sum_max;
  const int64_t crows = stack * xm + 4;
  p.lutc = p.lut && crows <= LUT2_ROWS && xm <= 7 && w->code_max > 0 && w->code_max <= 15;
  p.lut_rows = p.lutc ? (int32_t)crows : 0;
  const int lm = p.lutc ? LUT_CHANNEL : p.lut ? LUT_SHARED : LUT_NONE;
  // LDS decides how many workgroups share a CU (every variant needs < 128 VGPRs: up to four
  // waves per SIMD): stage fewer timesteps per pass rather than lose a workgroup to LDS --
  // four per CU measured 7.1 ms on the headline shape, three 7.8, two 11.2.  Any chunk length
  // works (the staging loops test every timestep against it), so the chunk is the largest
  // that fits: at T = 20 all of it in ONE pass (5.35 ms against 5.57 for 16 + 4: a staging
  // phase, a flush and three barriers fewer per patch), at T = 50 20 + 20 + 10.
  const size_t lds_rest = lds_fixed - (size_t)p.tchunk * HIMG2 + u8c2_table_bytes(lm, p.lut_bound, p.lut_rows);
  for (int wgs = 4; wgs >= 2; --wgs) {
    const size_t per_wg = (size_t)(160 * 1024) / wgs - 512;
    int tc = p.tchunk;
    while (tc > 16 && (size_t)tc * HIMG2 + lds_rest > per_wg) tc -= 1;
    if ((size_t)tc * HIMG2 + lds_rest <= per_wg) {
      p.tchunk = tc;
      break;
    }
  }
  p.ldsb = (size_t)p.tchunk * HIMG2 + lds_rest;
  // nothing carried in or out and every timestep in one chunk: the variant whose potentials start
  // their life behind the staging code (template parameter ONE)
  p.one = !has_state && T <= p.tchunk;
  // ... and of those, the launch whose last 16 channels are silent by the caller's word: the last
  // 32-channel group in a 16-channel half (template parameter HALF; snnqp_set_event_half_group)
  p.half = event_half_group_enabled() && ev1 && p.one && p.lutc && nf == NF_MUL0 && w->cout_fire > 0 &&
           w->cout_fire % 16 == 0 && w->cout_fire + 16 == Cout && Cout % 32 == 0;
  // ... and of that family the two launches whose four waves would carry unequal work: 96 channels
  // with the half group, and 64 channels (template parameter SPREAD; snnqp_set_event_wave_spread)
  p.spread = event_wave_spread_enabled() && ev1 && p.one && p.lutc && nf == NF_MUL0 &&
             (p.half ? Cout == 96 : Cout == 64);
  // ... and of those the one that runs quarters of the half group: each from a 16x16x64 product (template
  // parameter Q16; snnqp_set_event_quarter16)
  p.quarter16 = event_quarter16_enabled() && p.half && p.spread;
  return p;
}
}  // namespace

// The two predicates: `who` opens the messages, `flag` is the plan's answer.
static int event_plan_flag(const char *who, bool U8c2Plan::*flag, int in_type, int32_t T, const snnqp_conv_geom_t *g,
                           const snnqp_weight_t *w, const snnqp_neuron_t *nrn, bool has_state, int pool, int x_max) {
  SNNQP_REQUIRE(g && w && nrn, SNNQP_EINVAL, "%s: null descriptor", who);
  SNNQP_REQUIRE(pool == 1 || pool == 2, SNNQP_EINVAL, "%s: pool must be 1 or 2", who);
  SNNQP_REQUIRE(T >= 0, SNNQP_EINVAL, "%s: negative T", who);
  if (in_type != SNNQP_EV1 || T == 0) return 0;
  BlockCall c;
  c.in_type = in_type; c.g = g; c.w = w; c.nrn = nrn;
  if (conv3x3_mfma_unsupported(c)) return 0;
  SNNQP_REQUIRE(w->L >= 1.0f, SNNQP_EINVAL, "dequant L must be >= 1");
  if (int rc = conv3x3_check_cout_fire(who, w, g->Cout)) return rc;
  return u8c2_plan(in_type, T, g->Cout, w, neuron_form(make_neuron(nrn)), has_state, pool == 2, x_max).*flag ? 1 : 0;
}

int conv3x3_event_half_group(int in_type, int32_t T, const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                             const snnqp_neuron_t *nrn, bool has_state, int pool, int x_max) {
  return event_plan_flag("conv_event_half_group", &U8c2Plan::half, in_type, T, g, w, nrn, has_state, pool, x_max);
}

int conv3x3_event_wave_spread(int in_type, int32_t T, const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                              const snnqp_neuron_t *nrn, bool has_state, int pool, int x_max) {
  return event_plan_flag("conv_event_wave_spread", &U8c2Plan::spread, in_type, T, g, w, nrn, has_state, pool, x_max);
}

int conv3x3_event_quarter16(int in_type, int32_t T, const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                            const snnqp_neuron_t *nrn, bool has_state, int pool, int x_max) {
  return event_plan_flag("conv_event_quarter16", &U8c2Plan::quarter16, in_type, T, g, w, nrn, has_state, pool, x_max);
}

// The instance of a launch, one template parameter per step: table mode (launch_conv3x3_u8c2), neuron
// form, input format, then pool and ONE.
template <int NF, int LUTM, int IN>
static void launch_u8c2_pool(const ConvMfmaArgs &a, bool pool, bool one, unsigned gy, hipStream_t st, size_t lds) {
  if (pool && one) launch_persistent(conv3x3_u8c2_kernel<NF, true, LUTM, IN, true>, a, gy, st, lds);
  else if (pool) launch_persistent(conv3x3_u8c2_kernel<NF, true, LUTM, IN>, a, gy, st, lds);
  else if (one) launch_persistent(conv3x3_u8c2_kernel<NF, false, LUTM, IN, true>, a, gy, st, lds);
  else launch_persistent(conv3x3_u8c2_kernel<NF, false, LUTM, IN>, a, gy, st, lds);
}

template <int NF, int LUTM>
static void launch_u8c2_in(const ConvMfmaArgs &a, int in_type, bool pool, bool one, unsigned gy, hipStream_t st,
                           size_t lds) {
  if (in_type == SNNQP_EV1) launch_u8c2_pool<NF, LUTM, SNNQP_EV1>(a, pool, one, gy, st, lds);
  else if (in_type == SNNQP_EV4) launch_u8c2_pool<NF, LUTM, SNNQP_EV4>(a, pool, one, gy, st, lds);
  else if (in_type == SNNQP_F32) launch_u8c2_pool<NF, LUTM, SNNQP_F32>(a, pool, one, gy, st, lds);
  else launch_u8c2_pool<NF, LUTM, SNNQP_U8>(a, pool, one, gy, st, lds);
}

template <int LUTM>
static void launch_u8c2_nf(const ConvMfmaArgs &a, int nf, int in_type, bool pool, bool one, unsigned gy,
                           hipStream_t st, size_t lds) {
  if (nf == NF_MUL0) launch_u8c2_in<NF_MUL0, LUTM>(a, in_type, pool, one, gy, st, lds);
  else if (nf == NF_MUL) launch_u8c2_in<NF_MUL, LUTM>(a, in_type, pool, one, gy, st, lds);
  else if (nf == NF_DIV) launch_u8c2_in<NF_DIV, LUTM>(a, in_type, pool, one, gy, st, lds);
  else launch_u8c2_in<NF_DECAY, LUTM>(a, in_type, pool, one, gy, st, lds);
}

// The half-group and spread instances: bit-packed frames, ONE, per-channel tables, NF_MUL0 (u8c2_plan)
template <bool HALF, bool SPREAD, bool Q16 = false>
static void launch_u8c2_event(const ConvMfmaArgs &a, bool pool, unsigned gy, hipStream_t st, size_t lds) {
  if (pool) launch_persistent(conv3x3_u8c2_kernel<NF_MUL0, true, LUT_CHANNEL, SNNQP_EV1, true, HALF, SPREAD, Q16>, a, gy, st, lds);
  else launch_persistent(conv3x3_u8c2_kernel<NF_MUL0, false, LUT_CHANNEL, SNNQP_EV1, true, HALF, SPREAD, Q16>, a, gy, st, lds);
}

int launch_conv3x3_u8c2(ConvMfmaArgs a, int in_type, const snnqp_weight_t *w, int x_max, int32_t *x_flags,
                        hipStream_t st) {
  a.patch_h = 8;                             // this kernel's patch: two tiles of 4x8 pixels
  a.tiles_y = (a.H + 7) / 8;
  a.npatch = (int64_t)a.B * a.tiles_y * a.tiles_x;
  const int nf = neuron_form(a.nrn);          // which straight-line epilogue (conv_tile.h)
  const bool pl = a.pool == 2;
  const unsigned gy = (unsigned)((a.Cout + 127) / 128);
  const U8c2Plan plan = u8c2_plan(in_type, a.T, a.Cout, w, nf, a.u0 || a.u_out, pl, x_max);
  a.x_limit = plan.x_limit;
  a.lut_bound = plan.lut_bound;
  a.tchunk = plan.tchunk;
  a.lut_rows = plan.lut_rows;
  a.ch_slots = plan.lutc && w->ch_stack_max > 0 ? w->ch_slots : nullptr;
  a.cout_fire = w->cout_fire > 0 ? w->cout_fire : a.Cout;
  // (the last check: nothing may be launched before a launch that is refused)
  if (in_type == SNNQP_F32) {
    SNNQP_REQUIRE(x_flags != nullptr && (((uintptr_t)a.x) & 7) == 0 && a.xs_t % 2 == 0 && a.xs_b % 2 == 0,
                  SNNQP_EINVAL, "conv3x3 mfma: float32 frames need x_flags and 8-byte aligned pixels");
    if (int rc = zero_words_async((uint32_t *)x_flags, 1, st)) return rc;
    a.x_flags = x_flags;
  }
  if (plan.lut) check_code_bound_once(stream_device(st), a.w, (int64_t)9 * a.Cin, a.Cout, w->abs_sum_max, st);
  if (plan.quarter16) launch_u8c2_event<true, true, true>(a, pl, gy, st, plan.ldsb);
  else if (plan.half && plan.spread) launch_u8c2_event<true, true>(a, pl, gy, st, plan.ldsb);
  else if (plan.spread) launch_u8c2_event<false, true>(a, pl, gy, st, plan.ldsb);
  else if (plan.half) launch_u8c2_event<true, false>(a, pl, gy, st, plan.ldsb);
  else if (plan.lutc) launch_u8c2_nf<LUT_CHANNEL>(a, nf, in_type, pl, plan.one, gy, st, plan.ldsb);
  else if (plan.lut) launch_u8c2_nf<LUT_SHARED>(a, nf, in_type, pl, plan.one, gy, st, plan.ldsb);
  else launch_u8c2_nf<LUT_NONE>(a, nf, in_type, pl, plan.one, gy, st, plan.ldsb);
  return SNNQP_OK;
}

}  // namespace snnqp
