// Device helpers shared by the conv3x3 MFMA kernels, the event layer (conv3x3_u8c2.hip) as well
// as the bit-input conv (conv3x3_bits.hip, conv3x3_currents.hip): launch arguments, patch schedule,
// LDS tables, the neuron epilogue on the MFMA C/D layout, spike-word staging.  What only the
// bit-input conv uses -- its halo image and operand layout -- is in bits_tile.h.  gfx950 only.
#pragma once
#include "kernels.h"

namespace snnqp {

// Two neurons (two pixels of one channel) travel through the epilogue side by side.
// As SCALAR float32 instructions: on gfx950 the packed forms (v_pk_fma/mul/add_f32) take
// two passes anyway and, unlike scalar VALU ops, do not overlap with an MFMA in flight
// (tools/ubench/mfma_overlap_classes.hip: 4 v_pk_fma + 1 MFMA = 25.5 ns against 9.7 +
// 13.9 apart; 8 v_fma_f32 + 1 f8f6f4 MFMA = 21.7 ns against 18.4 + 15.3).
struct v2f {
  float x, y;
};
__device__ __forceinline__ v2f operator+(v2f a, v2f b) { return v2f{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ v2f operator-(v2f a, v2f b) { return v2f{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ v2f operator*(v2f a, v2f b) { return v2f{a.x * b.x, a.y * b.y}; }
__device__ __forceinline__ v2f operator+(v2f a, float b) { return v2f{a.x + b, a.y + b}; }
__device__ __forceinline__ v2f operator-(v2f a, float b) { return v2f{a.x - b, a.y - b}; }
__device__ __forceinline__ v2f operator*(v2f a, float b) { return v2f{a.x * b, a.y * b}; }
__device__ __forceinline__ v2f operator-(v2f a) { return v2f{-a.x, -a.y}; }
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) {
  return v2f{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y)};
}


// Dequantisation by LDS table (fast neuron path only).  The accumulator is made
// to BE the table address: the A operand carries 4x the input (spike bytes {0,4},
// event counts << 2) and the MFMA chain starts from C = byte address of the entry
// of acc = 0, so ds_read_b32 takes the MFMA result as is (no index arithmetic).
//   LUT_SHARED : one table, entry = fl(fl(acc / L) * m), |acc| <= LUT_CAP
//   LUT_CHANNEL: one table per output channel with BatchNorm applied to the entry
//                as well (conv0: each channel over its own accumulator range), so the
//                epilogue starts at the membrane update
enum { LUT_NONE = 0, LUT_SHARED = 1, LUT_CHANNEL = 2 };
// 4095: a 32 KiB table.  conv0 on event counts with 8-bit codes (|acc| <= sum|w| * x_max, a few
// thousand) then still dequantises by table and keeps three workgroups per CU; in the bits
// kernel the entry of acc = 0 stays an instruction immediate (< 64 KiB from the LDS base).
constexpr int LUT_CAP = 4095;
// LUT_CHANNEL: at most 32 KiB of tables -- three workgroups per CU still fit; taller tables cost
// an occupancy step that the shared table does not (headline layer, count frames, hint 3 / 229 rows:
// 6.68 ms; hint 4 / 304 rows at two workgroups per CU: 8.58; shared table: 7.03)
constexpr int LUT2_ROWS = 256;
constexpr int LUT_XMAX = 31;                    // 4 * x must stay an int8

constexpr int HALO = 10;
// LDS image of one timestep's halo for the int8 kernels: four planes (the 32-channel
// k-steps kk of a tap), rows of HPITCH pixels, 32 B per pixel = the two 16-byte lane
// halves, swapped on odd halo rows.  Every tap / k-step / tile offset of an A fragment
// is then an instruction immediate on one of two lane bases, and the wave's
// ds_read_b128 are bank-conflict free (tools/ubench/lds_conv_patterns.hip: 222
// B/clk/CU; the earlier pixel-major image with an XOR swizzle measured 63).
constexpr int HPITCH = 12;
constexpr int HPLANE = HALO * HPITCH * 32;      // one k-step plane

struct ConvMfmaArgs {
  const void *x;
  int64_t xs_t, xs_b;
  int32_t T, B, H, W, Cin, Cout;
  const int8_t *w;   // HWIO int8 codes
  const int8_t *wt;  // the same codes, MFMA-tiled (snnqp_pack_codes_mfma)
  Dequant dq;
  BnP bn;
  NeuronP nrn;
  const float *u0;
  float *u_out;
  uint32_t *s_out;
  int32_t pool;
  int32_t tiles_y, tiles_x;
  int64_t npatch;
  int32_t lut_bound;  // > 0: |acc| <= lut_bound while inputs <= x_limit, dequant by LDS table
  int32_t lut_rows;   // u8c2 kernel, LUT_CHANNEL: rows (of 32 entries) the launch reserved for the tables
  const int32_t *ch_slots;  // u8c2 kernel, LUT_CHANNEL: table slot of every channel (snnqp_weight_t), or null
  int32_t x_limit;    // u8c2 kernel: largest input value the table mode is sized for
  int32_t *x_seen;    // u8c2 kernel: (nullable) atomically max-ed with the largest input seen
  int32_t *x_flags;   // u8c2 kernel, float32 frames: OR-ed with SNNQP_FLAG_NOT_INTEGER (snnqp.h)
  int32_t xcd_split;  // patch schedule keeps a sample on one XCD (grid % 8 == 0, B >= 8)
  int32_t tchunk;     // u8c2 kernel: timesteps staged per pass (<= 32)
  uint32_t *sched;    // work queues of this launch (launch_persistent), or null: static walk
  uint32_t *status;   // the device's status word (runtime.hip), or null
  int32_t patch_h;    // rows of a patch: 8 (two 4x8 tiles), or 4 (conv3x3_bits.hip, one tile)
  const int32_t *pred;  // u8c2 kernel on byte / float32 frames: (nullable) the launch runs only if *pred != 0
  int32_t cout_fire;  // u8c2 kernel: the stored spike bits from this channel on are zeros (snnqp_weight_t; Cout: all may fire)
};

// Work queues of one launch: per blockIdx.y, one patch counter per XCD queue and one count
// of finished workgroups (the last one zeroes the words for the slot's next user).
constexpr int SCHED_Y = 8;                  // blockIdx.y values a slot serves (Cout <= 1024)
constexpr int SCHED_WORDS = SCHED_Y * 16;   // words of one slot
// Sized by launches outstanding, not by launches per step: a caller that enqueues 20 steps
// without a fence, each step's first two conv blocks cut into 8 batch chunks (tools/corun_ab.py),
// has 20 x (8 + 8 + 1) = 340 launches behind the one that runs.  512 slots are 256 KiB of words.
constexpr int SCHED_SLOTS = 512;            // launches in flight per device
constexpr int SCHED_CAPTURE_SLOTS = 960;    // launches captured into graphs per device (never reused)

// Patch schedule of a persistent workgroup.  With xcd_split the workgroups that
// share an XCD (blockIdx.x % 8 under the observed round-robin placement -- a speed
// assumption only) walk the samples b = xcd (mod 8), neighbouring patches at the
// same time, so the halo lines neighbouring patches share are served by that
// XCD's L2 instead of being fetched once per XCD.
struct PatchWalk {
  int64_t first, count, stride;
  int ppb, xcd;
  bool split;
  uint32_t *queue;    // this workgroup's patch counter, or null
  uint32_t *done;
  __device__ __forceinline__ explicit PatchWalk(const ConvMfmaArgs &a) {
    ppb = a.tiles_y * a.tiles_x;
    split = a.xcd_split != 0;
    if (split) {
      xcd = blockIdx.x & 7;
      first = blockIdx.x >> 3;
      stride = gridDim.x >> 3;
      count = (int64_t)((a.B - xcd + 7) >> 3) * ppb;
    } else {
      xcd = 0;
      first = blockIdx.x;
      stride = gridDim.x;
      count = a.npatch;
    }
    queue = a.sched ? a.sched + blockIdx.y * 16 + xcd : nullptr;
    done = a.sched ? a.sched + blockIdx.y * 16 + 8 : nullptr;
  }
  // Dynamic schedule: the first patch of a workgroup is its static one; every further patch
  // is claimed from the queue (workgroups that the CU's oldest-first issue favours finish
  // their patches sooner and would otherwise idle while the youngest still has a quarter
  // of its static share left: 4.75 against 7.44 ms measured inside conv0).  One thread
  // claims, a patch ahead so that the atomic's round trip hides behind the patch.
  // (never beyond `count`, whatever the counter holds: a word that was not zero at the start
  // of the launch must not cost an out-of-range patch index -- it costs patches, and finish()
  // reports that)
  __device__ __forceinline__ int64_t claim() const {
    const int64_t r = stride + (int64_t)atomicAdd(queue, 1u);
    return r < count ? r : count;
  }
  // After the last claim of the workgroup (one thread): add the patches this workgroup processed
  // to the launch's tally and count the workgroup; the last one of the launch checks the tally
  // against the number of patches the launch had -- a queue word that was not zero when the
  // launch began (an aborted launch, a graph replayed concurrently with itself) makes
  // workgroups skip patches, which must not pass silently: the device's status word gets
  // SNNQP_STATUS_QUEUE_CORRUPT and the next call into the library fails (runtime.hip) -- and
  // zeroes the slot for its next user.
  __device__ __forceinline__ void finish(uint32_t processed, int64_t npatch, uint32_t *status) const {
    atomicAdd(done + 1, processed);
    __threadfence();
    const uint32_t total = gridDim.x;
    if (atomicAdd(done, 1u) + 1u == total) {
      __threadfence();
      const uint32_t tally = atomicAdd(done + 1, 0u);
      if (tally != (uint32_t)npatch && status) *(volatile uint32_t *)status = SNNQP_STATUS_QUEUE_CORRUPT;
      for (int i = 0; i < 8; ++i) done[i - 8] = 0u;
      done[1] = 0u;
      __threadfence();
      *done = 0u;
    }
  }
  __device__ __forceinline__ void decode(const ConvMfmaArgs &a, int64_t r, int &b, int &y0,
                                         int &x0) const {
    const int within = (int)(r % ppb);
    const int bi = (int)(r / ppb);
    b = split ? xcd + 8 * bi : bi;
    y0 = (within / a.tiles_x) * a.patch_h;
    x0 = (within % a.tiles_x) * 8;
  }
};

// old with lane `lane` replaced by the wave-uniform `val` (v_writelane_b32).
// This hipcc has no __builtin_amdgcn_writelane; binding the LLVM intrinsic by its
// name keeps the instruction visible to the compiler, which then inserts the wait
// states a VALU-written SGPR needs before it (inline asm would hide that hazard).
extern "C" __device__ uint32_t snnqp_writelane_i32(uint32_t, uint32_t, uint32_t)
    __asm("llvm.amdgcn.writelane.i32");
__device__ __forceinline__ uint32_t writelane_u32(uint32_t val, int lane, uint32_t old) {
  return snnqp_writelane_i32(val, (uint32_t)lane, old);
}

// u with the lanes of `mask` zeroed: the hard reset reuses the ballot of the
// threshold compare (written as a C++ select the compiler emits a second, negated
// v_cmp per element).  VALU readers of a VALU-written SGPR need no wait states.
__device__ __forceinline__ float reset_where(float u, unsigned long long mask) {
  float r;
  asm("v_cndmask_b32_e64 %0, %1, 0, %2" : "=v"(r) : "v"(u), "s"(mask));
  return r;
}

struct LaneConsts {
  float bmean, bmul, bbias, dec;
  float vr;      // v_reset (a VGPR operand of the reset select when it is not 0)
};

// Output-channel block of a wave when Cout is not a multiple of 32: `cout` is the real
// channel (u_io skips lanes beyond Cout), `cpar` a clamped index for the per-channel
// parameter loads, `cmask` the bits of the block's spike word that exist.
__device__ __forceinline__ uint32_t chan_mask(int cout_base, int Cout) {
  const int valid = Cout - cout_base;
  return valid >= 32 ? 0xFFFFFFFFu : valid <= 0 ? 0u : (1u << valid) - 1u;
}

// The neuron update forms of spiking_learning.py, one straight-line epilogue each
// (template parameter NF of the conv kernels):
//   NF_MUL0   u += (x - u) * m, reset to 0        multi_step_LIF with tau = 2^j (m = 1/tau,
//                                                 exact) and parametric_leaky_IF (m =
//                                                 sigmoid(tau)), v_reset = 0     :381,410
//   NF_MUL    u += (x - (u - v_reset)) * m        the same neurons, v_reset != 0
//   NF_DIV    u += (x - (u - v_reset)) / tau      multi_step_LIF, any other tau    :410
//   NF_DECAY  u = u * decay[c] + x                LIF (per-feature sigmoid(tau))   :432
// all followed by s = (u >= v_th) and the hard reset u = s ? v_reset : u (:412-414).
enum { NF_MUL0 = 1, NF_MUL = 2, NF_DIV = 3, NF_DECAY = 4 };

__host__ inline int neuron_form(const NeuronP &n) {
  if (n.kind == SNNQP_NEURON_LIF) return NF_DECAY;
  if (n.inv_k == 0.0f) return NF_DIV;               // multi_step_LIF, tau not a power of two
  return n.vr == 0.0f ? NF_MUL0 : NF_MUL;
}

// (LDS by absolute address, tile_util.h: a table read takes the MFMA result itself as the address)
__device__ __forceinline__ float lds_read_f32(uint32_t addr) {
  return *(lds_cfloat_t *)(uintptr_t)addr;
}

// lut[i] = fl(fl((i - bound) / L) * m): the dequantised current of accumulator
// value i - bound, built once per workgroup (same exact division, common.h).
__device__ __forceinline__ void build_lut(float *lut, int bound, const Dequant &dq,
                                          int tid, int nthreads = 256) {
  for (int i = tid; i <= 2 * bound; i += nthreads) lut[i] = dequant_acc(i - bound, dq);
}

// Per-channel tables of the workgroup's 128 output channels: one block per wave,
// [acc + bound][32 channels] (rows of 128 B), entry = BatchNorm_c(dequant(acc)), the
// same op sequence the epilogue would run (bn_apply on dequant_acc), so folding
// changes no bit.  With this order lane (channel c) reads LDS bank c whatever its
// accumulator is: the table reads of a wave never conflict (the channel-major order
// [channel][acc] lost half of its LDS cycles to conflicts of the lanes with acc != 0).
// The accumulator must then count 128 B per unit: A carries 16 x input, B 8 x code.
// LUT_CHANNEL tables (conv3x3_u8c2.hip): every channel of the workgroup's 128 keeps the entries of
// acc = -neg_c x_limit .. +pos_c x_limit (pos_c / neg_c = the sums of its positive / |negative|
// codes: what its accumulator can reach with inputs 0 .. x_limit) in ONE of the 32 bank columns of
// a table of 128-byte rows, stacked with the three other channels of that column: slot = 4 x column
// + position (snnqp_weight_t.ch_slots; default column = c mod 32, position = wave).  The 32 channels
// of a wave sit in 32 different columns, so its lanes never collide whatever their accumulators
// are, and the table is as tall as the tallest column -- not four times the widest channel's
// symmetric range.
//   scr[0..127]    rows by slot           scr[128..255]  neg_c x_limit by channel
//   scr[256..383]  slot by channel
// Returns the bits of the smallest non-zero |entry| this thread wrote (+inf if none).
__device__ __forceinline__ int lut_column_start(const uint32_t *scr, int slot) {
  int st = 0;
  for (int k = 0; k < (slot & 3); ++k) st += (int)scr[(slot & ~3) + k];
  return st;
}
// TWIN (the half-group launch, conv3x3_u8c2.hip): the slots of the last 16 channels hold the tables
// of the 16 channels before them -- their rows and neg_c came from the twin's codes, and so do
// the BatchNorm constants here.
template <bool TWIN = false>
__device__ __forceinline__ uint32_t build_lut_channel(float *lut, const uint32_t *scr, int max_rows,
                                                      const Dequant &dq, const BnP &bn, int cout0,
                                                      int Cout, int tid) {
  uint32_t minbits = 0x7F800000u;
  const int c = tid & 127, hf = tid >> 7;
  const int slot = (int)scr[256 + c], col = slot >> 2;
  const int st = lut_column_start(scr, slot);
  const int rows = (int)scr[slot], negx = (int)scr[128 + c];
  if (st + rows > max_rows) return minbits;                    // (reported by the caller)
  int co = cout0 + c < Cout ? cout0 + c : Cout - 1;
  if (TWIN && cout0 + c >= Cout - 16 && cout0 + c < Cout) co -= 16;
  float bm = 0.f, bmul = 1.f, bb = 0.f;
  if (bn.mean) { bm = bn.mean[co]; bmul = bn.mul[co]; bb = bn.bias[co]; }
  for (int i = hf; i < rows; i += 2) {
    const float y = bn_apply(dequant_acc(i - negx, dq), bm, bmul, bb);
    lut[(st + i) * 32 + col] = y;
    const uint32_t mag = __float_as_uint(y) & 0x7FFFFFFFu;
    if (mag != 0u && mag < minbits) minbits = mag;
  }
  return minbits;
}

// fma(d, 2^-j, u) == fl(u + fl(d * 2^-j)) for all T steps of a launch that starts from
// u = 0 when every input current x is 0 or has |x| >= 2^(j (T + 1) - 126):
// all x are then multiples of q = 2^(e_min - 23); by induction u_t and d_t = fl(x - u_t)
// are multiples of q 2^(-j t) (rounding a multiple of a power of two to 24 bits keeps
// it one), so d_t 2^-j is a multiple of q 2^(-j (t + 1)) >= 2^-149 with the significand
// of d_t: representable, the product rounds nothing away.  `min_x_bits` = bits of the
// smallest non-zero |x| the launch can see.
__host__ __device__ __forceinline__ bool lif_fma_is_exact(uint32_t min_x_bits, int j, int T, bool has_u0) {
  if (has_u0 || j < 0) return false;
  const long long e = (long long)j * (T + 1) - 126;     // needed exponent of min |x|
  if (e > 100) return false;
  const uint32_t need = e <= -126 ? 0x00800000u : (uint32_t)(e + 127) << 23;
  return min_x_bits >= need;
}

// Smallest non-zero |BatchNorm_c(entry)| (as float32 bits) over the shared table and the 128
// channels of a workgroup: the `min_x_bits` of lif_fma_is_exact for the kernels that apply
// BatchNorm in the epilogue.  Same operation order as the epilogue.  nthreads % 128 == 0,
// so a thread keeps one channel.
__device__ __forceinline__ uint32_t lut_bn_min_bits(const float *lut, int bound, const BnP &bn,
                                                    int cout0, int Cout, int tid, int nthreads) {
  int c = cout0 + (tid & 127);
  if (c >= Cout) c = Cout - 1;
  float mean = 0.f, mul = 1.f, bias = 0.f;
  if (bn.mean) { mean = bn.mean[c]; mul = bn.mul[c]; bias = bn.bias[c]; }
  uint32_t mb = 0x7F800000u;
  for (int i = tid >> 7; i <= 2 * bound; i += nthreads >> 7) {
    float x = lut[i] - mean;
    x = x * mul;
    x = x + bias;
    const uint32_t b = __float_as_uint(x) & 0x7FFFFFFFu;
    if (b != 0 && b < mb) mb = b;
  }
  return mb;
}

// Dequantised currents of two accumulator registers (two pixels, same channel).
// Table modes: the register is the LDS address of its entry.  Otherwise packed
// float32 ops (v_pk_*_f32 keep every rounding of the scalar sequence).
// `off` (an integer < 2^24 as float, exact): constant added to the accumulator first --
// the u8 kernel accumulates (x - 128) * w so that counts up to 255 are int8 operands,
// and adds 128 * sum(w) back here.
template <int LUTM, bool OFFS = false>
__device__ __forceinline__ v2f dequant_pair(int a0, int a1, const Dequant &dq, float off = 0.0f) {
  if (LUTM != LUT_NONE) return v2f{lds_read_f32((uint32_t)a0), lds_read_f32((uint32_t)a1)};
  v2f a = {(float)a0, (float)a1};
  if (OFFS) a = a + off;
  const v2f q = fma2(a, v2f{dq.rL, dq.rL}, a * dq.rLlo);     // exact a / L (common.h)
  return q * dq.m;
}

// u -> u' for two pixels of one channel (before threshold and reset).
// FMA (NF_MUL0 only): u + d * m as one fused multiply-add.  Identical to the two-step
// form whenever d * m is exact, i.e. never a subnormal with bits shifted out; the
// caller proves that for the launch (lif_fma_is_exact) before taking this variant.
template <int NF, bool FMA = false, bool PACKED = true>
__device__ __forceinline__ v2f neuron_update(v2f x, v2f u, const LaneConsts &lc,
                                             const NeuronP &nrn) {
  if (NF == NF_DECAY) {
    const v2f ud = u * lc.dec;
    return ud + x;
  }
  // u - 0 == u exactly, so NF_MUL0 skips the subtraction
  if (FMA && PACKED) {
    // conv0's table kernel: no MFMA worth overlapping (one per 1024 updates), and one
    // v_pk_add + one v_pk_fma per pair issue in fewer slots than four scalar ops
    // (measured 7.8 against 8.1 ms), so this variant keeps the packed forms
    typedef float v2fp __attribute__((ext_vector_type(2)));
    const v2fp up = {u.x, u.y}, xp = {x.x, x.y};
    const v2fp dp = NF == NF_MUL0 ? xp - up : xp - (up - lc.vr);
    const v2fp r = __builtin_elementwise_fma(dp, v2fp{nrn.inv_k, nrn.inv_k}, up);
    return v2f{r.x, r.y};
  }
  const v2f d = NF == NF_MUL0 ? x - u : x - (u - lc.vr);
  if (NF == NF_DIV) return u + v2f{d.x / nrn.k, d.y / nrn.k};
  if (FMA) return fma2(d, v2f{nrn.inv_k, nrn.inv_k}, u);
  const v2f dk = d * nrn.inv_k;
  return u + dk;
}

// hard reset of the lanes in `mask`
template <int NF>
__device__ __forceinline__ float neuron_reset(float u, unsigned long long mask,
                                              const LaneConsts &lc) {
  if (NF == NF_MUL0) return reset_where(u, mask);
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(u), "v"(lc.vr), "s"(mask));
  return r;
}

// BatchNorm (unless the table already applied it) + neuron for two dequantised
// currents (two pixels, same channel).  With float32 subnormals kept (hipcc default)
// (u - v_th) >= 0  <=>  u >= v_th.
template <int NF, bool BNDONE, bool FMA = false>
__device__ __forceinline__ void neuron_pair(v2f y, float &u0, float &u1,
                                            const LaneConsts &lc, const NeuronP &nrn,
                                            unsigned long long &m0,
                                            unsigned long long &m1) {
  v2f x = y;
  if (!BNDONE) {
    x = x - lc.bmean;
    x = x * lc.bmul;
    x = x + lc.bbias;
  }
  const v2f uu = neuron_update<NF, FMA>(x, v2f{u0, u1}, lc, nrn);
  m0 = __ballot(uu.x >= nrn.vth);
  m1 = __ballot(uu.y >= nrn.vth);
  u0 = neuron_reset<NF>(uu.x, m0, lc);
  u1 = neuron_reset<NF>(uu.y, m1, lc);
}

// Where the two compare masks of register pair p (registers 2 p, 2 p + 1) go: the masks are
// wave-uniform, so v_writelane drops each word into the lane that stores it (no per-lane compare
// masks to keep in SGPRs).  `myw` in, `myw` out.  Three forms of the product exist:
//   EP_TILE   : one 32x32 tile.  The lane mask of register i holds pixel (ty = 2*(i>>3), tx = i&7) in
//               its low half and (ty + 1, tx) in its high half.  The word a lane stores:
//                 POOL : lanes 0..7  = pooled pixel (pty = lane >> 2, ptx = lane & 3)
//                 !POOL: lanes 0..31 = pixel row `lane` of the tile
//   EP_HALFW  : the half-group wave (conv3x3_u8c2.hip).  Lanes n and n + 16 hold ONE channel at the
//               pixels (Y, tx) and (Y + 1, tx), Y = 2 ty the even image rows of the 8x8 patch, so the
//               64-bit mask of register i (tx = i & 7, g = i >> 3) is four 16-channel fields: image rows
//               4 g .. 4 g + 3.  The 2x2 pool's row pair lies inside a lane half.  In bits 0..15 (bits
//               16..31 are zero):
//                 POOL : lanes 0..15 = pooled pixel `lane` of the patch (4 x 4)
//                 !POOL: lanes 0..63 = pixel `lane` of the patch (8 x 8)
//   EP_QUARTER: the same fields over registers 0..3 (the spread launch, conv3x3_u8c2.hip): a wave that
//               runs one quarter of the half group's product.  The wave permutes the ROWS of its A
//               operand so that its quarter -- columns 4 q .. 4 q + 3 of image rows 4 g .. 4 g + 3 --
//               arrives in registers 0..3 whatever (g, q) is: register i = column 4 q + i.
//                 POOL : lanes j, 4 + j (j = 0, 1) = pooled pixel (row 2 g, 2 g + 1; column 2 q + j)
//                 !POOL: lanes 4 r + i (r, i = 0..3) = pixel (row 4 g + r, column 4 q + i)
// The two field forms are one placement: pooled words in lane rows of 4 (the quarter fills two of
// a row), the others in rows of PW pixels -- the patch's 8, the quarter's 4.
enum { EP_TILE = 0, EP_HALFW = 1, EP_QUARTER = 2 };
template <int FORM, bool POOL>
__device__ __forceinline__ uint32_t place_words(unsigned long long m0, unsigned long long m1, int p, uint32_t myw) {
  if (FORM == EP_TILE && POOL) {
    const unsigned long long o = m0 | m1;
    const uint32_t pw = (uint32_t)o | (uint32_t)(o >> 32);
    myw = writelane_u32(pw, p, myw);
  } else if (FORM == EP_TILE) {
    const int r0 = (2 * p & 3) + 8 * (p >> 1);      // row of register 2 p, low half
    myw = writelane_u32((uint32_t)m0, r0, myw);
    myw = writelane_u32((uint32_t)(m0 >> 32), r0 + 4, myw);
    myw = writelane_u32((uint32_t)m1, r0 + 1, myw);
    myw = writelane_u32((uint32_t)(m1 >> 32), r0 + 5, myw);
  } else {
    constexpr int PW = FORM == EP_HALFW ? 8 : 4;
    const int g = p >> 2, j = p & 3;                // (the quarter: g = 0)
    if (POOL) {
      const unsigned long long o = m0 | m1;
      const uint32_t lo = (uint32_t)o, hi = (uint32_t)(o >> 32);
      myw = writelane_u32((lo | (lo >> 16)) & 0xFFFFu, 8 * g + j, myw);          // pooled row 2 g
      myw = writelane_u32((hi | (hi >> 16)) & 0xFFFFu, 8 * g + 4 + j, myw);      // pooled row 2 g + 1
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        myw = writelane_u32((uint32_t)(m0 >> (16 * r)) & 0xFFFFu, (4 * g + r) * PW + 2 * j, myw);
        myw = writelane_u32((uint32_t)(m1 >> (16 * r)) & 0xFFFFu, (4 * g + r) * PW + 2 * j + 1, myw);
      }
    }
  }
  return myw;
}

// BatchNorm + neuron + spike words of PARTS x PAIRS register pairs of a product, from register 0 on.
// The table reads (dequant_pair) of a part are issued first, then its pairs are processed; the
// scheduling barrier keeps the parts apart.  Returns the word this lane stores (place_words).
//   <EP_TILE, 4, 2>   : a tile in two halves of four pairs: eight table reads in flight instead of
//                       sixteen -- fewer registers alive, for the build that buys a sixth wave per
//                       SIMD with them (conv3x3_u8c2.hip)
//   <EP_HALFW, 4, 2>  : the product of the half-group wave, the same way
//   <EP_QUARTER, 2, 1>: a quarter of it: four potentials, four table reads
// (`lane` is not read.  It stays a parameter, here and in tile_epilogue: without it the no-pool
// half-group instances come out of the register allocator with other register numbers, and the
// assembly of this kernel is what its refactors are compared by: DESIGN.md 4.2.)
template <int NF, bool POOL, int LUTM, bool FMA, bool OFFS, int FORM, int PAIRS, int PARTS>
__device__ __forceinline__ uint32_t tile_epilogue_parts(const v16i &acc, float (&u)[16], const Dequant &dq, const LaneConsts &lc,
                                                        const NeuronP &nrn, int lane, float off = 0.0f) {
  uint32_t myw = 0;
#pragma unroll
  for (int g = 0; g < PARTS; ++g) {
    v2f y[PAIRS];
#pragma unroll
    for (int j = 0; j < PAIRS; ++j) {
      const int i = 2 * PAIRS * g + 2 * j;
      y[j] = dequant_pair<LUTM, OFFS>(acc[i], acc[i + 1], dq, off);
    }
#pragma unroll
    for (int j = 0; j < PAIRS; ++j) {     // masks are consumed pair by pair
      const int i = 2 * PAIRS * g + 2 * j;
      unsigned long long m0, m1;
      neuron_pair<NF, LUTM == LUT_CHANNEL, FMA>(y[j], u[i], u[i + 1], lc, nrn, m0, m1);
      myw = place_words<FORM, POOL>(m0, m1, i >> 1, myw);
    }
    if (PARTS > 1) __builtin_amdgcn_sched_barrier(0);
  }
  return myw;
}

// EP_QUARTER16: the quarter as the product of a 16x16x64 matrix instruction (the spread launch with
// the quarter16 switch, conv3x3_u8c2.hip): lane = (channel c = lane & 15, lane group gq = lane >> 4),
// register i = pixel 4 gq + i of the wave's 4x4 quarter, and the pixels are ordered so that a lane
// group's four registers are ONE 2x2 pool block: block gq at rows 2 (gq >> 1) ..+1, columns 2 (gq & 1)
// ..+1 of the quarter, register i at (i >> 1, i & 1) inside it.  The 64-bit mask of register i is then
// four 16-channel fields, one pixel each, and the words land in the lanes EP_QUARTER puts them in:
//   POOL : the OR of the four masks, field gq -> lane 4 (gq >> 1) + (gq & 1)
//   !POOL: field gq of register i -> lane 4 r + x, (r, x) the pixel's row and column in the quarter
constexpr int EP_QUARTER16 = 3;
template <bool POOL>
__device__ __forceinline__ uint32_t place_words_quarter16(const unsigned long long (&m)[4]) {
  uint32_t myw = 0;
  if (POOL) {
    const unsigned long long o = (m[0] | m[1]) | (m[2] | m[3]);
#pragma unroll
    for (int gq = 0; gq < 4; ++gq)
      myw = writelane_u32((uint32_t)(o >> (16 * gq)) & 0xFFFFu, 4 * (gq >> 1) + (gq & 1), myw);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq)
        myw = writelane_u32((uint32_t)(m[i] >> (16 * gq)) & 0xFFFFu,
                            4 * (2 * (gq >> 1) + (i >> 1)) + 2 * (gq & 1) + (i & 1), myw);
  }
  return myw;
}

// BatchNorm + neuron + spike word of the four registers of that product: four table reads, two pairs
// (tile_epilogue_parts' sequence on a 4-register tuple; u[0..3] are the quarter's potentials).
template <int NF, bool POOL, int LUTM, bool FMA, bool OFFS>
__device__ __forceinline__ uint32_t quarter16_epilogue(const v4i &acc, float (&u)[16], const Dequant &dq,
                                                       const LaneConsts &lc, const NeuronP &nrn, float off = 0.0f) {
  v2f y[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) y[j] = dequant_pair<LUTM, OFFS>(acc[2 * j], acc[2 * j + 1], dq, off);
  unsigned long long m[4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
    neuron_pair<NF, LUTM == LUT_CHANNEL, FMA>(y[j], u[2 * j], u[2 * j + 1], lc, nrn, m[2 * j], m[2 * j + 1]);
  return place_words_quarter16<POOL>(m);
}

// The neurons of a whole tile from its 8 dequantised pairs (tile_epilogue below; a function of its
// own: folded into tile_epilogue_parts<EP_TILE, 8, 1> the bit-packed instance with carried potentials
// allocates its registers differently)
template <int NF, bool POOL, bool BNDONE, bool FMA = false>
__device__ __forceinline__ uint32_t tile_neurons(const v2f (&y)[8], float (&u)[16],
                                                 const LaneConsts &lc, const NeuronP &nrn) {
  uint32_t myw = 0;
#pragma unroll
  for (int i = 0; i < 16; i += 2) {     // masks are consumed pair by pair
    unsigned long long m0, m1;
    neuron_pair<NF, BNDONE, FMA>(y[i >> 1], u[i], u[i + 1], lc, nrn, m0, m1);
    myw = place_words<EP_TILE, POOL>(m0, m1, i >> 1, myw);
  }
  return myw;
}

// Whole-tile epilogue (used where no MFMA stream runs beside it): all table
// reads are issued first, then the pairs are processed.
template <int NF, bool POOL, int LUTM, bool FMA = false, bool OFFS = false>
__device__ __forceinline__ uint32_t tile_epilogue(const v16i &acc, float (&u)[16],
                                                  const Dequant &dq,
                                                  const LaneConsts &lc,
                                                  const NeuronP &nrn, int lane, float off = 0.0f) {
  v2f y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = dequant_pair<LUTM, OFFS>(acc[2 * j], acc[2 * j + 1], dq, off);
  return tile_neurons<NF, POOL, LUTM == LUT_CHANNEL, FMA>(y, u, lc, nrn);
}

// Spike words are staged in LDS, obuf[slot = t % FL][pixel][4 words of the 128-
// channel block], and flushed with 16-byte stores: no global store sits in the
// per-timestep loop (vmcnt stays a pure load counter there).
template <bool POOL>
struct OutStage {
  static constexpr int NPIX = POOL ? 16 : 64;   // (pooled) pixels of one patch
  static constexpr int FL = POOL ? 32 : 8;      // timesteps between flushes
  static constexpr int BYTES = FL * NPIX * 16;
};

// patch-pixel index this lane's word of tile `tl` belongs to
template <bool POOL>
__device__ __forceinline__ int out_pix(int tl, int lane) {
  if (POOL) return (tl * 2 + ((lane >> 2) & 1)) * 4 + (lane & 3);
  const int ty = ((lane >> 2) & 1) | (((lane >> 4) & 1) << 1);
  const int tx = (lane & 3) | (((lane >> 3) & 1) << 2);
  return (tl * 4 + ty) * 8 + tx;
}

// Writes timesteps [t0, t0 + n) of the patch at (y0, x0) (full-resolution
// coordinates) from obuf (a ring of SLOTS timesteps) to global memory.  All NT
// threads of the workgroup take part.
template <bool POOL, int SLOTS, int NT, int NPIX = OutStage<POOL>::NPIX>
__device__ __forceinline__ void flush_ring(const uint32_t *obuf, const ConvMfmaArgs &a,
                                           int t0, int n, int b, int y0, int x0, int tid) {
  constexpr int PW = POOL ? 4 : 8;              // patch width in output pixels
  const int CW = (a.Cout + 31) >> 5;
  const int cwb = blockIdx.y * 4;
  const int nw = min(4, CW - cwb);
  const int OH = POOL ? a.H >> 1 : a.H, OW = POOL ? a.W >> 1 : a.W;
  const int oy0 = POOL ? y0 >> 1 : y0, ox0 = POOL ? x0 >> 1 : x0;
  for (int i = tid; i < n * NPIX; i += NT) {
    const int slot = i / NPIX, pix = i % NPIX;
    const int t = t0 + slot;
    const uint32_t *src = obuf + ((t % SLOTS) * NPIX + pix) * 4;
    const int oy = oy0 + pix / PW, ox = ox0 + pix % PW;
    if (oy >= OH || ox >= OW) continue;          // edge patch of an image not 8-aligned
    uint32_t *dst = a.s_out + ((((int64_t)t * a.B + b) * OH + oy) * OW + ox) * CW + cwb;
    if (nw == 4 && (CW & 3) == 0) {
      *(v4i *)dst = *(const v4i *)src;
    } else {
      for (int w = 0; w < nw; ++w) dst[w] = src[w];
    }
  }
}

template <bool POOL>
__device__ __forceinline__ void flush_out(const uint32_t *obuf, const ConvMfmaArgs &a,
                                          int t0, int n, int b, int y0, int x0, int tid) {
  flush_ring<POOL, OutStage<POOL>::FL, 256>(obuf, a, t0, n, b, y0, x0, tid);
}

// membrane potentials of one tile (tl) of the patch <-> global memory
template <bool LOAD>
__device__ __forceinline__ void u_io_tile(float (&u)[16], const ConvMfmaArgs &a, int b,
                                          int y0, int x0, int cout, int h, int tl) {
  float *uo = a.u_out;
  const float *ui = a.u0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int y = y0 + tl * 4 + (h | ((i >> 3) << 1));
    const int x = x0 + (i & 7);
    const int64_t o = (((int64_t)b * a.H + y) * a.W + x) * a.Cout + cout;
    const bool in = y < a.H && x < a.W && cout < a.Cout;
    if (LOAD) u[i] = in ? ui[o] : 0.0f;
    else if (in) uo[o] = u[i];
  }
}

template <bool LOAD>
__device__ __forceinline__ void u_io(float (&u)[2][16], const ConvMfmaArgs &a,
                                     int b, int y0, int x0, int cout, int h) {
  float *uo = a.u_out;
  const float *ui = a.u0;
#pragma unroll
  for (int tl = 0; tl < 2; ++tl)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int y = y0 + tl * 4 + (h | ((i >> 3) << 1));
      const int x = x0 + (i & 7);
      const int64_t o = (((int64_t)b * a.H + y) * a.W + x) * a.Cout + cout;
      const bool in = y < a.H && x < a.W && cout < a.Cout;
      if (LOAD) u[tl][i] = in ? ui[o] : 0.0f;
      else if (in) uo[o] = u[tl][i];
    }
}

__device__ __forceinline__ void zero_u(float (&u)[2][16]) {
#pragma unroll
  for (int tl = 0; tl < 2; ++tl)
#pragma unroll
    for (int i = 0; i < 16; ++i) u[tl][i] = 0.0f;
}

__device__ __forceinline__ v16i splat16(int v) {
  return v16i{v, v, v, v, v, v, v, v, v, v, v, v, v, v, v, v};
}

// Work-queue words of one launch on `dev`, the device of `st` (the pool: workqueue.hip): the slot's
// words and its index, or nullptr -- the launch then takes the static walk.  sched_release records
// the event that marks the slot busy until the launch is done.
uint32_t *sched_acquire(hipStream_t st, int dev, int *slot);
void sched_release(int dev, int slot, hipStream_t st);

template <typename K>
static inline void launch_persistent(K kernel, ConvMfmaArgs a, unsigned gy, hipStream_t st,
                                     size_t dyn_lds = 0, int threads = 256) {
  const int dev = stream_device(st);
  int slot = -1;
  a.sched = gy <= (unsigned)SCHED_Y ? sched_acquire(st, dev, &slot) : nullptr;   // npatch < 2^30: run_conv3x3_mfma
  a.status = a.sched ? device_status_word(dev) : nullptr;
  const unsigned gx = persistent_grid((const void *)kernel, threads, dyn_lds, dev, a.npatch, a.B, &a.xcd_split);
  hipLaunchKernelGGL(kernel, dim3(gx, gy), dim3(threads), dyn_lds, st, a);
  if (a.sched) sched_release(dev, slot, st);
}

// The check of the caller's silent channels (snnqp.h) that run_conv3x3_mfma and
// snnqp_conv_event_half_group share -- a malformed value is refused before anything runs.  `who`
// opens the message.  (conv3x3_mfma.hip)
int conv3x3_check_cout_fire(const char *who, const snnqp_weight_t *w, int32_t Cout);
// the input channels `wt` is padded to: one 32-channel group per int8 tile of a tap
inline int wt_cin_pad(const snnqp_weight_t *w, int32_t Cin) { return w->wt_cin ? w->wt_cin : (Cin + 31) / 32 * 32; }

// The two launchers run_conv3x3_mfma hands a checked launch to; `a` holds the fields both kernels
// read, each launcher adds what only its kernel consumes and picks the instance.
// conv3x3_bits.hip: bit-packed input, Cin <= 128.  How the accumulator becomes the current --
// DQ_ARITH (three float32 instructions), DQ_ONE (L == 1: one multiply), DQ_TABLE (fp6 instruction,
// NF_MUL0, 0 < a.lut_bound = abs_sum_max <= DQT_MAXA: an LDS table addressed by the accumulator's
// bit pattern)
enum { DQ_ARITH = 1, DQ_ONE = 2, DQ_TABLE = 3 };
constexpr int DQT_MAXA = 2047;
void launch_conv3x3_bits(ConvMfmaArgs a, const snnqp_weight_t *w, const snnqp_neuron_t *nrn, hipStream_t st);
// conv3x3_u8c2.hip: the event layer (Cin = 2) on U8 / EV1 / EV4 / F32 frames; SNNQP_OK or the error
// of its own checks
int launch_conv3x3_u8c2(ConvMfmaArgs a, int in_type, const snnqp_weight_t *w, int x_max, int32_t *x_flags,
                        hipStream_t st);
// snnqp_set_conv_k16 (api.hip): whether launch_conv3x3_bits picks the 16-less walks
bool conv_k16_enabled();
// snnqp_set_event_half_group (api.hip): whether launch_conv3x3_u8c2 picks the half-group instances
bool event_half_group_enabled();
// snnqp_set_event_wave_spread (api.hip): whether launch_conv3x3_u8c2 picks the spread instances
bool event_wave_spread_enabled();
// snnqp_set_event_quarter16 (api.hip): whether the 96 / 80 spread launch takes its quarter of the half
// group from a 16x16x64 matrix instruction
bool event_quarter16_enabled();

}  // namespace snnqp
