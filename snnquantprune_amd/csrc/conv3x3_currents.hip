// QuantConv(3x3, stride 1, pad 1) alone over bit-packed spikes, Cin <= 128, any int8 weight codes:
// the currents form of conv3x3_bits.hip.  Replaces lax.conv_general_dilated at
// flax_qconv.py:158-168 where the input is a spike raster and no neuron follows in the same launch
// (QuantConv.__call__ on its own; the training forward of a conv block, which needs the currents
// for its batch statistics).
//
// The contraction is the fused kernel's: v_mfma_scale_f32_32x32x64_f8f6f4 (fp4 spikes x fp6 codes)
// for codes of magnitude <= 7, v_mfma_i32_32x32x32_i8 otherwise; K runs over (tap, 32-channel
// group) pairs of the codes `wt` (snnqp_pack_codes_mfma, padded along Cin to 32 G), two per fp6
// k-step, an odd G's last group through the pair_tap walk.  A last half group is walked whole (zero
// spikes against zero codes: the same sums).  Same workgroup (4 waves on one 4x8-pixel tile, wave w
// = output channels [32 w, +32) of blockIdx.y's 128, its B fragments in registers for the whole
// launch), same halo image in LDS (conv_tile.h), same persistent patch walk -- static here: a patch
// is one image's tile, not T timesteps of it, so there is nothing for a work queue to balance.
//
// There is no time axis to pipeline over; patches are pipelined instead.  Two halo images: while
// the waves run the MFMAs of patch r from one, the spike words of the workgroup's next patch are
// in flight from global memory; they are expanded into the other image after the MFMAs, and ONE
// barrier per patch publishes them (every wave is then also done reading the image that the patch
// after next will overwrite).
//
// Epilogue: the accumulator (an exact integer on either instruction) becomes fl(fl(acc / L) * m)
// with the instructions of DQ_ARITH (the exact two-instruction division of common.h, one
// multiply) and is stored through u_io_tile's mapping: lane (n, h) = channel, register i = pixel
// row h | ((i >> 3) << 1), column i & 7, so the 32 lanes of a half wave store 128 contiguous bytes.
// Stores are scalar float32 / int32, predicated on the image and on Cout: nothing beyond 4-byte
// alignment is assumed of x, y and acc.
#include <type_traits>

#include "conv_tile.h"

namespace snnqp {

template <int FMT, int WPP>
__global__ void __launch_bounds__(F6_NT, 2)
conv3x3_currents_kernel(ConvMfmaArgs a, int32_t *acc_out) {
  static_assert(WPP >= 1 && WPP <= 4, "one to four 32-channel groups");
  constexpr bool I8 = FMT == FMT_I8;
  typedef typename std::conditional<I8, v16i, v16f>::type acc_t;
  constexpr int BR = I8 ? 4 : 6;                 // registers of one B fragment
  constexpr int NP = I8 ? WPP : (WPP + 1) / 2;   // planes of the halo image
  constexpr int NPL = I8 ? WPP : WPP / 2;        // planes read whole: both lane halves at one tap
  constexpr int PAIRS = !I8 && WPP % 2 == 1 ? 5 : 0;   // fp6, odd group count: pair_tap k-steps
  constexpr int KS = 9 * NPL + PAIRS;            // MFMAs of one patch
  constexpr int NPD = NPL > 0 ? NPL : 1;
  constexpr int HALO_B = NP * F6_PLANE;          // one halo image
  constexpr int TAB_OFF = 2 * HALO_B;
  __shared__ __attribute__((aligned(128))) uint8_t lds[TAB_OFF + (I8 ? 0 : F6_TAB)];
  const uint32_t lds0 = lds_addr(lds) & 0x3FFFFu;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 31, h = lane >> 5;
  const int cout_base = blockIdx.y * 128 + wave * 32;
  const bool wave_on = cout_base < a.Cout;
  const int cout = cout_base + n;

  if (!I8) fp4_table_fill((uint32_t *)(lds + TAB_OFF), tid, F6_NT);

  // B operand, as conv3x3_bits.hip holds it: k-step ks = NPL tap + kk covers channels 64 kk .. +63
  // of the tap (int8: 32 kk .. +31), pair k-step 9 NPL + p group WPP - 1 of tap pair_tap(p, h)
  int bf[KS][BR];
  {
    const v4i *wtile = (const v4i *)a.wt + (int64_t)(cout_base >> 5) * (9 * WPP) * 64;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if constexpr (I8) {
        const v4i t = wave_on ? wtile[((ks / NPD) * WPP + ks % NPD) * 64 + lane] : v4i{0, 0, 0, 0};
        bf[ks][0] = t.x; bf[ks][1] = t.y; bf[ks][2] = t.z; bf[ks][3] = t.w;
      } else {
        const int ptap = pair_tap(ks - 9 * NPL, h);
        const bool pair = ks >= 9 * NPL;
        const int ks8 = pair ? ptap * WPP + (WPP - 1) : (ks / NPD) * WPP + (ks % NPD) * 2 + h;
        v4i lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
        if (wave_on && !(pair && ptap >= 9)) {
          lo = wtile[ks8 * 64 + n];
          hi = wtile[ks8 * 64 + 32 + n];
        }
        fp6_pack32(lo, hi, bf[ks]);
      }
    }
  }

  const int ty = ((n >> 2) & 1) | ((n >> 4) << 1);
  const int tx = (n & 3) | (((n >> 3) & 1) << 2);
  // lane bases of an A fragment (conv3x3_bits.hip): whole planes on even / odd tap rows, the pair
  // k-steps one halo row lower / one pixel to the right for lane half 1
  const uint32_t pixb = lds0 + (uint32_t)((ty * F6_PITCH + tx) * 32);
  const uint32_t abase_even = pixb + (uint32_t)((h ^ (ty & 1)) * 16);
  const uint32_t abase_odd = pixb + (uint32_t)((h ^ (ty & 1) ^ 1) * 16);
  const uint32_t abase_pv = pixb + (uint32_t)(h * F6_PITCH * 32 + ((ty ^ h) & 1) * 16);
  const uint32_t abase_ph = pixb + (uint32_t)(h * 32 + (ty & 1) * 16);

  // staging task of this thread: word wi of halo pixel pix
  const int s_pix = tid / WPP, s_wi = tid % WPP;
  const bool s_task = tid < F6_ROWS * HALO * WPP;
  const int wpm = (a.Cin + 31) >> 5;             // spike words of a pixel in memory
  const int s_hy = s_pix / HALO, s_hx = s_pix % HALO;
  const uint32_t s_dst = lds0 + (uint32_t)((I8 ? s_wi : s_wi >> 1) * F6_PLANE +
                                           (s_hy * F6_PITCH + s_hx) * 32 +
                                           ((((I8 ? 0 : s_wi) & 1) ^ (s_hy & 1)) * 16));
  const uint32_t tabl = fp4_table_lane(lds0 + TAB_OFF, lane);
  const uint32_t *xb = (const uint32_t *)a.x;

  PatchWalk pw(a);                               // a.sched == nullptr: the static walk
  // the halo word of this thread's task in patch r (0 outside the image and beyond the words a
  // pixel has: codes padded wider than that meet zero spikes)
  auto stage_load = [&](int64_t r) -> uint32_t {
    int b, y0, x0;
    pw.decode(a, r, b, y0, x0);
    const int gy = y0 + s_hy - 1, gx = x0 + s_hx - 1;
    const bool valid = s_task && s_wi < wpm && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    return valid ? xb[(int64_t)b * a.xs_b + ((int64_t)gy * a.W + gx) * wpm + s_wi] : 0u;
  };
  auto stage_write = [&](uint32_t sw, uint32_t bufoff) {
    typedef __attribute__((address_space(3))) v4i lds_v4i_t;
    if (!s_task) return;
    const uint32_t d = s_dst + bufoff;
    if (I8) {
      *(lds_v4i_t *)(uintptr_t)d = expand16(sw & 0xFFFFu);                       // channels 0..15
      *(lds_v4i_t *)(uintptr_t)(s_hy & 1 ? d - 16 : d + 16) = expand16(sw >> 16);
    } else {
      v4i e;                                     // byte k of the word -> its 8 fp4 nibbles
      e.x = (int)*(lds_cu32_t *)(uintptr_t)(((sw & 0xFFu) << 7) + tabl);
      e.y = (int)*(lds_cu32_t *)(uintptr_t)((((sw >> 8) & 0xFFu) << 7) + tabl);
      e.z = (int)*(lds_cu32_t *)(uintptr_t)((((sw >> 16) & 0xFFu) << 7) + tabl);
      e.w = (int)*(lds_cu32_t *)(uintptr_t)(((sw >> 24) << 7) + tabl);
      *(lds_v4i_t *)(uintptr_t)d = e;
    }
  };
  auto a_read = [&](uint32_t bufoff, int ks) -> v4i {
    if (ks >= 9 * NPL) {                         // pair k-step: the padding half ("tap 9") reads
      const int p = ks - 9 * NPL;                // pixel (2, 3), inside the image
      const uint32_t off = (uint32_t)(NPL * F6_PLANE + (p < 3 ? p : 2 * F6_PITCH + 2 * (p - 3)) * 32);
      return *(lds_cv4i_t *)(uintptr_t)((p < 3 ? abase_pv : abase_ph) + bufoff + off);
    }
    const int tap = ks / NPD;
    const uint32_t off = (uint32_t)((ks % NPD) * F6_PLANE + ((tap / 3) * F6_PITCH + tap % 3) * 32);
    return *(lds_cv4i_t *)(uintptr_t)(((tap / 3) & 1 ? abase_odd : abase_even) + bufoff + off);
  };

  lds_barrier();                                 // the table is visible
  int64_t r = pw.first;
  if (r < pw.count) stage_write(stage_load(r), 0u);
  lds_barrier();
  uint32_t buf = 0u;                             // byte offset of the image patch r is read from
  while (r < pw.count) {
    int b, y0, x0;
    pw.decode(a, r, b, y0, x0);
    const int64_t rn = r + pw.stride;
    const bool more = rn < pw.count;
    uint32_t sw_next = 0u;
    if (more) sw_next = stage_load(rn);          // in flight behind the MFMAs

    acc_t acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (wave_on) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const v4i av = a_read(buf, ks);
        if constexpr (I8) {
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(
              av, v4i{bf[ks][0], bf[ks][1], bf[ks][2], bf[ks][3]}, acc, 0, 0, 0);
        } else {
          acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
              v8i{av.x, av.y, av.z, av.w, 0, 0, 0, 0},
              v8i{bf[ks][0], bf[ks][1], bf[ks][2], bf[ks][3], bf[ks][4], bf[ks][5], 0, 0}, acc,
              4 /* A: fp4 */, 2 /* B: fp6 */, 0, 127, 0, 127);
        }
      }
    }
    if (more) stage_write(sw_next, buf ^ (uint32_t)HALO_B);

    if (wave_on) {
      float cur[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float af = (float)acc[i];          // exact integer
        cur[i] = div_exact(af, a.dq) * a.dq.m;   // fl(fl(acc / L) * m), as DQ_ARITH
      }
      u_io_tile<false>(cur, a, b, y0, x0, cout, h, 0);     // a.u_out = y [B][H][W][Cout]
      if (acc_out) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int y = y0 + (h | ((i >> 3) << 1)), x = x0 + (i & 7);
          if (y < a.H && x < a.W && cout < a.Cout)
            acc_out[(((int64_t)b * a.H + y) * a.W + x) * a.Cout + cout] = (int)acc[i];
        }
      }
    }
    lds_barrier();                               // image of patch rn written, image of r read
    buf ^= (uint32_t)HALO_B;
    r = rn;
  }
}

template <int FMT, int WPP>
static void launch_currents(ConvMfmaArgs a, int32_t *acc, unsigned gy, hipStream_t st) {
  const auto kernel = conv3x3_currents_kernel<FMT, WPP>;
  const unsigned gx = persistent_grid((const void *)kernel, F6_NT, 0, stream_device(st), a.npatch, a.B, &a.xcd_split);
  hipLaunchKernelGGL(kernel, dim3(gx, gy), dim3(F6_NT), 0, st, a, acc);
}

template <int FMT>
static void launch_currents_wpp(const ConvMfmaArgs &a, int wpp, int32_t *acc, unsigned gy, hipStream_t st) {
  if (wpp == 1) launch_currents<FMT, 1>(a, acc, gy, st);
  else if (wpp == 2) launch_currents<FMT, 2>(a, acc, gy, st);
  else if (wpp == 3) launch_currents<FMT, 3>(a, acc, gy, st);
  else launch_currents<FMT, 4>(a, acc, gy, st);
}

const char *conv3x3_currents_unsupported(int in_type, int64_t NB, const snnqp_conv_geom_t *g,
                                         const snnqp_weight_t *w, const int8_t *wt) {
  if (w->wtype != SNNQP_W_I8) return "weights are not int8 codes";
  if (const char *why = conv3x3_geometry_unsupported(g)) return why;
  if (in_type != SNNQP_BITS) return "input must be bit-packed spikes";
  if (g->Cin < 1 || g->Cin > 128) return "bit input needs Cin <= 128";
  if (!wt) return "MFMA-tiled codes `wt` not given";
  const int cin_pad = wt_cin_pad(w, g->Cin);
  if (cin_pad % 32 != 0 || cin_pad < g->Cin || cin_pad > 128)
    return "wt_cin must be a multiple of 32 in [Cin, 128]";
  // the kernel keeps a patch index (+ one grid stride) in 32 bits
  if (NB > 0 && NB * (int64_t)((g->H + 3) / 4) * ((g->W + 7) / 8) >= ((int64_t)1 << 30))
    return "2^30 patches or more in one launch";
  return nullptr;
}

int run_conv3x3_currents(const void *x, int64_t NB, const snnqp_conv_geom_t *g,
                         const snnqp_weight_t *w, const int8_t *wt, float *y, int32_t *acc,
                         hipStream_t st) {
  SNNQP_REQUIRE(NB >= 0 && NB < (1ll << 31), SNNQP_EINVAL, "conv3x3 currents: bad NB");
  SNNQP_REQUIRE(w->w && ((x && y) || NB == 0), SNNQP_EINVAL, "conv3x3 currents: null pointer");
  SNNQP_REQUIRE(w->L >= 1.0f, SNNQP_EINVAL, "dequant L must be >= 1");
  if (NB == 0) return SNNQP_OK;
  ConvMfmaArgs a = {};
  a.x = x;
  a.xs_t = 0;
  a.xs_b = (int64_t)g->H * g->W * ((g->Cin + 31) / 32);
  a.T = 1; a.B = (int32_t)NB;
  a.H = g->H; a.W = g->W; a.Cin = g->Cin; a.Cout = g->Cout;
  a.w = (const int8_t *)w->w;
  a.wt = wt;
  a.dq = make_dequant(w->L, w->m);
  a.bn = make_bn(nullptr);
  a.nrn = make_neuron(nullptr);
  a.u_out = y;
  a.pool = 1;
  a.patch_h = 4;
  a.tiles_y = (g->H + 3) / 4; a.tiles_x = (g->W + 7) / 8;
  a.npatch = NB * a.tiles_y * a.tiles_x;
  const unsigned gy = (unsigned)((g->Cout + 127) / 128);
  const int wpp = wt_cin_pad(w, g->Cin) / 32;
  // codes exact in fp6 -> the f8f6f4 instruction; wider or unknown -> int8
  if (w->code_max > 0 && w->code_max <= 7) launch_currents_wpp<FMT_FP6>(a, wpp, acc, gy, st);
  else launch_currents_wpp<FMT_I8>(a, wpp, acc, gy, st);
  SNNQP_CHECK_LAUNCH("conv3x3 currents kernel");
  return SNNQP_OK;
}

}  // namespace snnqp
