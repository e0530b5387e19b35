// Host side shared by the two fused 3x3 / stride 1 / pad 1 MFMA conv kernels: what they support
// (conv3x3_mfma_unsupported) and the dispatch (run_conv3x3_mfma), which checks a launch, fills the
// arguments both kernels read and hands over to the launcher of the input format -- bit-packed
// spikes: conv3x3_bits.hip, event frames (Cin = 2): conv3x3_u8c2.hip.  No kernel lives here.
#include "conv_tile.h"

namespace snnqp {

const char *conv3x3_geometry_unsupported(const snnqp_conv_geom_t *g) {
  if (g->KH != 3 || g->KW != 3) return "kernel is not 3x3";
  if (g->stride_h != 1 || g->stride_w != 1) return "stride is not 1";
  if (g->pad_h_lo != 1 || g->pad_h_hi != 1 || g->pad_w_lo != 1 || g->pad_w_hi != 1)
    return "padding is not ((1,1),(1,1))";
  if (g->in_dil_h != 1 || g->in_dil_w != 1 || g->k_dil_h != 1 || g->k_dil_w != 1)
    return "dilated convolution";
  if (g->groups != 1) return "grouped convolution";
  if (g->H <= 0 || g->W <= 0) return "empty image";    // any size: edge patches are clipped
  if (g->Cout <= 0) return "no output channels";    // any count: the last word is masked
  return nullptr;
}

const char *conv3x3_mfma_unsupported(const BlockCall &c) {
  const snnqp_conv_geom_t *g = c.g;
  const int in_type = c.in_type;
  if (c.w->wtype != SNNQP_W_I8) return "weights are not int8 codes";
  if (const char *why = conv3x3_geometry_unsupported(g)) return why;
  if (c.s_type != SNNQP_BITS) return "spike output must be bit-packed";
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
  if (c.nrn->kind == SNNQP_NEURON_LIF && !c.nrn->decay) return "LIF without decay";
  if (in_type == SNNQP_BITS && !c.wt) return "MFMA-tiled codes `wt` not given";
  return nullptr;
}

int conv3x3_check_cout_fire(const char *who, const snnqp_weight_t *w, int32_t Cout) {
  SNNQP_REQUIRE(w->cout_fire == 0 || (w->cout_fire > 0 && w->cout_fire % 16 == 0 && w->cout_fire <= Cout),
                SNNQP_EINVAL, "%s: cout_fire %d is not a multiple of 16 in (0, Cout = %d]", who,
                w->cout_fire, Cout);
  return SNNQP_OK;
}

int run_conv3x3_mfma(const BlockCall &c) {
  const snnqp_conv_geom_t *g = c.g;
  const int in_type = c.in_type;
  // (this kernel's own checks stand between the pointers and the sizes, so the pointer line does too)
  SNNQP_REQUIRE(c.w->w && ((c.x && c.s_out) || c.T == 0 || c.B == 0), SNNQP_EINVAL, "conv3x3 mfma: null pointer");
  SNNQP_REQUIRE(!c.pred || in_type == SNNQP_U8 || in_type == SNNQP_F32 || in_type == SNNQP_EV4, SNNQP_EUNSUPPORTED,
                "conv3x3 mfma: only the event layer on byte / nibble / float32 frames takes a predicate");   // (an empty batch has no buffers)
  SNNQP_REQUIRE(in_type != SNNQP_BITS || c.wt, SNNQP_EINVAL,
                "conv3x3 mfma: bit input needs the MFMA-tiled codes `wt`");
  const int cin_pad = wt_cin_pad(c.w, g->Cin);
  SNNQP_REQUIRE(in_type != SNNQP_BITS || (cin_pad % 32 == 0 && cin_pad >= g->Cin && cin_pad <= 128),
                SNNQP_EINVAL, "conv3x3 mfma: wt_cin must be a multiple of 32 in [Cin, 128]");
  const int entry = block_entry("conv3x3 mfma", c, true);
  if (entry < 0) return entry;
  if (int rc = conv3x3_check_cout_fire("conv3x3 mfma", c.w, g->Cout)) return rc;
  if (entry == BLOCK_EMPTY) return SNNQP_OK;
  // the kernels keep a patch index (+ one grid stride) in a 32-bit scalar register; the
  // smallest patch is the bits kernel's 4 x 8 pixels
  SNNQP_REQUIRE((int64_t)c.B * ((g->H + 3) / 4) * ((g->W + 7) / 8) < ((int64_t)1 << 30),
                SNNQP_EUNSUPPORTED, "conv3x3 mfma: more than 2^30 patches in one launch");
  ConvMfmaArgs a = {};
  fill_block_args(a, c);
  a.H = g->H; a.W = g->W; a.Cin = g->Cin; a.Cout = g->Cout;
  a.w = (const int8_t *)c.w->w; a.wt = c.wt;
  a.pool = c.pool; a.x_seen = c.x_seen; a.pred = c.pred;
  a.tiles_x = (g->W + 7) / 8;                 // (tiles_y, patch_h, npatch: the launcher's patch)
  if (in_type == SNNQP_BITS) {
    launch_conv3x3_bits(a, c.w, c.nrn, c.st);
  } else if (int rc = launch_conv3x3_u8c2(a, in_type, c.w, c.x_max, c.x_flags, c.st)) {
    return rc;
  }
  SNNQP_CHECK_LAUNCH("conv3x3 mfma kernel");
  return SNNQP_OK;
}

}  // namespace snnqp
