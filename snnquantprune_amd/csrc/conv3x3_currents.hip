// QuantConv(3x3, stride 1, pad 1) alone over bit-packed spikes, Cin <= 128, any int8 weight codes:
// the currents form of conv3x3_bits.hip.  Replaces lax.conv_general_dilated at
// flax_qconv.py:158-168 where the input is a spike raster and no neuron follows in the same launch
// (QuantConv.__call__ on its own; the training forward of a conv block, which needs the currents
// for its batch statistics).
//
// The contraction is the fused kernel's, BitsTile (bits_tile.h): v_mfma_scale_f32_32x32x64_f8f6f4
// (fp4 spikes x fp6 codes) for codes of magnitude <= 7, v_mfma_i32_32x32x32_i8 otherwise; K runs
// over (tap, 32-channel group) pairs of the codes `wt` (snnqp_pack_codes_mfma, padded along Cin to
// 32 G), two per fp6 k-step, an odd G's last group through the pair_tap walk.  A last half group is
// walked whole (zero spikes against zero codes: the same sums).  Same workgroup (4 waves on one
// 4x8-pixel tile, wave w = output channels [32 w, +32) of blockIdx.y's 128, its B fragments in
// registers for the whole launch), same halo image in LDS, same persistent patch walk (conv_tile.h)
// -- static here: a patch is one image's tile, not T timesteps of it, so there is nothing for a work
// queue to balance.
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
#include "bits_tile.h"

namespace snnqp {

template <int FMT, int WPP>
__global__ void __launch_bounds__(F6_NT, 2)
conv3x3_currents_kernel(ConvMfmaArgs a, int32_t *acc_out) {
  static_assert(WPP >= 1 && WPP <= 4, "one to four 32-channel groups");
  typedef BitsTile<FMT, 32 * WPP> W;             // the walk over whole groups
  typedef typename W::acc_t acc_t;
  constexpr int KS = W::KS;                      // MFMAs of one patch
  static_assert(KS == 9 * W::NPL + W::PAIRS && W::K16 == 0 && W::PAIRS == (!W::I8 && WPP % 2 == 1 ? 5 : 0),
                "no half group: whole planes, and the pair walk of an odd fp6 group count");
  constexpr int HALO_B = W::HALO_B;              // one halo image
  constexpr int TAB_OFF = 2 * HALO_B;
  __shared__ __attribute__((aligned(128))) uint8_t lds[TAB_OFF + (W::I8 ? 0 : F6_TAB)];
  const uint32_t lds0 = lds_addr(lds) & 0x3FFFFu;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 31, h = lane >> 5;
  const int cout_base = blockIdx.y * 128 + wave * 32;
  const bool wave_on = cout_base < a.Cout;
  const int cout = cout_base + n;

  if (!W::I8) fp4_table_fill((uint32_t *)(lds + TAB_OFF), tid, F6_NT);

  int bf[KS][W::BR];                             // the wave's B fragments, for the whole launch
  W::load_b(bf, a.wt, cout_base, wave_on, n, h);
  const typename W::Bases img0 = W::bases(lds0, n, h);   // lane bases of the first halo image
  // staging task of this thread: spike word stg.wi of halo pixel (stg.hy, stg.hx)
  const typename W::Stage stg = W::stage_task(lds0, lds0 + TAB_OFF, tid, a.Cin);
  const uint32_t *xb = (const uint32_t *)a.x;

  PatchWalk pw(a);                               // a.sched == nullptr: the static walk
  // the halo word of this thread's task in patch r (0 outside the image and beyond the words a
  // pixel has: codes padded wider than that meet zero spikes)
  auto stage_load = [&](int64_t r) -> uint32_t {
    int b, y0, x0;
    pw.decode(a, r, b, y0, x0);
    const int gy = y0 + stg.hy - 1, gx = x0 + stg.hx - 1;
    const bool valid = stg.task && stg.wi < stg.wpm && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    return valid ? xb[(int64_t)b * a.xs_b + ((int64_t)gy * a.W + gx) * stg.wpm + stg.wi] : 0u;
  };
  auto stage_write = [&](uint32_t sw, uint32_t bufoff) {   // expanded and written in one go
    v4i e = {0, 0, 0, 0};
    W::expand(stg, sw, e);
    W::write(stg, bufoff, sw, e);
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
      const typename W::Bases img = img0.at(buf);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        acc = W::template mfma<127, 127>(W::a_read(img, ks), bf[ks], acc);
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
