// Host side shared by the two fused 3x3 / stride 1 / pad 1 MFMA conv kernels: what they support
// (conv3x3_mfma_unsupported) and the dispatch (run_conv3x3_mfma), which checks a launch, fills the
// arguments both kernels read and hands over to the launcher of the input format -- bit-packed
// spikes: conv3x3_bits.hip, event frames (Cin = 2): conv3x3_u8c2.hip.  No kernel lives here.
#include "conv_tile.h"

namespace snnqp {

const char *conv3x3_mfma_unsupported(int in_type, const snnqp_conv_geom_t *g,
                                     const snnqp_weight_t *w, const int8_t *wt,
                                     const snnqp_neuron_t *nrn, int s_type) {
  if (w->wtype != SNNQP_W_I8) return "weights are not int8 codes";
  if (g->KH != 3 || g->KW != 3) return "kernel is not 3x3";
  if (g->stride_h != 1 || g->stride_w != 1) return "stride is not 1";
  if (g->pad_h_lo != 1 || g->pad_h_hi != 1 || g->pad_w_lo != 1 || g->pad_w_hi != 1)
    return "padding is not ((1,1),(1,1))";
  if (g->in_dil_h != 1 || g->in_dil_w != 1 || g->k_dil_h != 1 || g->k_dil_w != 1)
    return "dilated convolution";
  if (g->groups != 1) return "grouped convolution";
  if (g->H <= 0 || g->W <= 0) return "empty image";    // any size: edge patches are clipped
  if (g->Cout <= 0) return "no output channels";    // any count: the last word is masked
  if (s_type != SNNQP_BITS) return "spike output must be bit-packed";
  if (in_type == SNNQP_BITS) {
    // any width up to 128: `wt` is tiled from the kernel zero-padded along Cin to
    // 32 ceil(Cin / 32) (or wt_cin); the spike words beyond ceil(Cin / 32) are not read
    if (g->Cin < 1 || g->Cin > 128) return "bit input needs Cin <= 128";
  } else if (in_type == SNNQP_U8) {     // any count 0..255 (taken as x - 128 without a table)
    if (g->Cin != 2) return "u8 input needs Cin == 2";
    if ((int64_t)g->H * g->W * 2 >= (int64_t)1 << 31) return "u8 frame of 2 GiB or more";
  } else if (in_type == SNNQP_EV1) {    // bit-packed binary event frames, staged directly
    if (g->Cin != 2) return "EV1 frames have Cin == 2";
    if ((int64_t)g->H * g->W * 2 >= (int64_t)1 << 31) return "EV1 frame of 2^31 bits or more";
  } else if (in_type == SNNQP_EV4) {    // nibble-packed count frames (<= 15), staged directly
    if (g->Cin != 2) return "EV4 frames have Cin == 2";
    if ((int64_t)g->H * g->W >= (int64_t)1 << 31) return "EV4 frame of 2 GiB or more";
  } else if (in_type == SNNQP_F32) {    // integer-valued float32 frames, staged in place and checked
    if (g->Cin != 2) return "float32 input into integer codes needs Cin == 2";
    if ((int64_t)g->H * g->W * 8 >= (int64_t)1 << 31) return "float32 frame of 2 GiB or more";
  } else {
    return "input must be BITS, U8, EV1, EV4 or (Cin == 2) F32";
  }
  if (nrn->kind == SNNQP_NEURON_LIF && !nrn->decay) return "LIF without decay";
  if (in_type == SNNQP_BITS && !wt) return "MFMA-tiled codes `wt` not given";
  return nullptr;
}

int conv3x3_check_weight(const char *who, const snnqp_weight_t *w, const snnqp_bn_t *bn, int32_t Cout) {
  SNNQP_REQUIRE(w->L >= 1.0f, SNNQP_EINVAL, "dequant L must be >= 1");
  SNNQP_CHECK_BN(bn);
  SNNQP_REQUIRE(w->cout_fire == 0 || (w->cout_fire > 0 && w->cout_fire % 16 == 0 && w->cout_fire <= Cout),
                SNNQP_EINVAL, "%s: cout_fire %d is not a multiple of 16 in (0, Cout = %d]", who,
                w->cout_fire, Cout);
  return SNNQP_OK;
}

int run_conv3x3_mfma(const void *x, int in_type, int64_t xs_t, int64_t xs_b,
                     int32_t T, int32_t B, const snnqp_conv_geom_t *g,
                     const snnqp_weight_t *w, const int8_t *wt,
                     const snnqp_bn_t *bn, const snnqp_neuron_t *nrn,
                     const float *u0, float *u_out, uint32_t *s_out, int pool,
                     int x_max, int32_t *x_seen, int32_t *x_flags, hipStream_t st, const int32_t *pred) {
  SNNQP_REQUIRE(w->w && ((x && s_out) || T == 0 || B == 0), SNNQP_EINVAL, "conv3x3 mfma: null pointer");
  SNNQP_REQUIRE(!pred || in_type == SNNQP_U8 || in_type == SNNQP_F32 || in_type == SNNQP_EV4, SNNQP_EUNSUPPORTED,
                "conv3x3 mfma: only the event layer on byte / nibble / float32 frames takes a predicate");   // (an empty batch has no buffers)
  SNNQP_REQUIRE(in_type != SNNQP_BITS || wt, SNNQP_EINVAL,
                "conv3x3 mfma: bit input needs the MFMA-tiled codes `wt`");
  const int cin_pad = wt_cin_pad(w, g->Cin);
  SNNQP_REQUIRE(in_type != SNNQP_BITS || (cin_pad % 32 == 0 && cin_pad >= g->Cin && cin_pad <= 128),
                SNNQP_EINVAL, "conv3x3 mfma: wt_cin must be a multiple of 32 in [Cin, 128]");
  SNNQP_REQUIRE(T >= 0 && B >= 0, SNNQP_EINVAL, "conv3x3 mfma: negative T/B");
  if (int rc = conv3x3_check_weight("conv3x3 mfma", w, bn, g->Cout)) return rc;
  if (T == 0 || B == 0) return SNNQP_OK;
  // the kernels keep a patch index (+ one grid stride) in a 32-bit scalar register; the
  // smallest patch is the bits kernel's 4 x 8 pixels
  SNNQP_REQUIRE((int64_t)B * ((g->H + 3) / 4) * ((g->W + 7) / 8) < ((int64_t)1 << 30),
                SNNQP_EUNSUPPORTED, "conv3x3 mfma: more than 2^30 patches in one launch");
  ConvMfmaArgs a = {};
  a.x = x; a.xs_t = xs_t; a.xs_b = xs_b; a.T = T; a.B = B;
  a.H = g->H; a.W = g->W; a.Cin = g->Cin; a.Cout = g->Cout;
  a.w = (const int8_t *)w->w;
  a.wt = wt;
  a.dq = make_dequant(w->L, w->m);
  a.bn = make_bn(bn);
  a.nrn = make_neuron(nrn);
  a.u0 = u0; a.u_out = u_out; a.s_out = s_out; a.pool = pool;
  a.x_seen = x_seen;
  a.pred = pred;
  a.tiles_x = (g->W + 7) / 8;                 // (tiles_y, patch_h, npatch: the launcher's patch)
  if (in_type == SNNQP_BITS) {
    launch_conv3x3_bits(a, w, nrn, st);
  } else if (int rc = launch_conv3x3_u8c2(a, in_type, w, x_max, x_flags, st)) {
    return rc;
  }
  SNNQP_CHECK_LAUNCH("conv3x3 mfma kernel");
  return SNNQP_OK;
}

}  // namespace snnqp
