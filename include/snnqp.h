/* snnqp.h -- C ABI of libsnnqp.so: the MI355X (gfx950) implementation of the
 * quantized / pruned SNN time-stepped forward pass of
 * Intelligent-Microsystems-Lab/SNNQuantPrune.
 *
 * The reference has no FFI: its hot path is Python on JAX (XLA emits the device
 * code).  Each entry point below therefore replaces a *Python call site* of the
 * reference; the `replaces:` lines give that call site (paths relative to the
 * reference checkout).  INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add at each of them.
 *
 * Conventions
 *  - every pointer named x/w/y/u/s/... is a DEVICE pointer owned by the caller
 *    (torch); the library allocates nothing that outlives a call, with one exception:
 *    the fused conv kernels keep 736 KiB of work-queue counters per device (the device of
 *    `stream`): 512 round-robin slots for eager launches -- a slot is zeroed on `stream`
 *    right before its launch and guarded by an event, so launches that run at the same time,
 *    on whatever streams, never share a counter; a launch that finds its slot still in
 *    flight (more than 512 conv launches outstanding on the device) walks its patches
 *    statically instead: same results, no queue -- and 960 slots that launches captured into
 *    a graph take one each until snnqp_workqueue_capture_release hands them back (the pool
 *    must exist before the capture: one eager launch on the device); 64 bytes of page-locked
 *    host memory per device hold the status word (snnqp_device_status);
 *  - descriptor structs (snnqp_*_t) are HOST structs read during the call;
 *  - all work is enqueued on `stream` (a hipStream_t); no call synchronises;
 *  - return value: 0 on success, <0 on error (SNNQP_E*); the message is
 *    available from snnqp_last_error() on the calling thread;
 *  - activations are time-major [T][B]...[C], channels innermost (NHWC), as
 *    inside the reference model (examples/tcja/models.py:109); `x_stride_t` /
 *    `x_stride_b` let a [B][T]... tensor be consumed in place;
 *  - SNNQP_BITS tensors pack channel c of a row into bit (c & 31) of 32-bit
 *    word (c >> 5); a row has ceil(C / 32) words.
 */
#ifndef SNNQP_H_
#define SNNQP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *snnqp_stream_t; /* hipStream_t */

enum {
  SNNQP_OK = 0,
  SNNQP_EINVAL = -1,       /* bad argument / shape */
  SNNQP_EUNSUPPORTED = -2, /* valid request the chosen kernel cannot serve */
  SNNQP_EHIP = -3          /* HIP runtime error */
};

/* element type of an activation tensor.
 * SNNQP_EV1 / SNNQP_EV4 are wire formats of the model INPUT, the 2-channel event frames
 * [H][W][2] of examples/input_pipeline.py:195-218 (what the host feeds, examples/
 * input_pipeline.py:17-27, 655 360 B per DVS128 sample as uint8):
 *   SNNQP_EV1  binary frames, one bit per element in index order: element
 *              i = (y * W + x) * 2 + polarity is bit (i & 31) of 32-bit word (i >> 5); a
 *              frame takes ceil(H * W * 2 / 32) words (frames are word-aligned) =
 *              numpy.packbits(frame.ravel(), bitorder="little") -- 81 920 B per sample;
 *   SNNQP_EV4  count frames with counts <= 15, one byte per pixel: polarity 0 in bits
 *              0..3, polarity 1 in bits 4..7; a frame takes H * W bytes -- 327 680 B.
 * Strides of such tensors are in words (EV1) / bytes (EV4). */
enum { SNNQP_F32 = 0, SNNQP_U8 = 1, SNNQP_BITS = 2, SNNQP_EV1 = 3, SNNQP_EV4 = 4 };
/* element type of a weight tensor */
enum { SNNQP_W_F32 = 0, SNNQP_W_I8 = 1 };
/* neuron models, spiking_learning.py:357-438 */
enum {
  SNNQP_NEURON_NONE = 0,
  SNNQP_NEURON_MULTI_STEP_LIF = 1,      /* spiking_learning.py:390-416 */
  SNNQP_NEURON_PARAMETRIC_LEAKY_IF = 2, /* spiking_learning.py:357-387 */
  SNNQP_NEURON_LIF = 3                  /* spiking_learning.py:419-438 */
};
/* surrogate derivatives of the spike functions, spiking_learning.py:139-241 (training) */
enum {
  SNNQP_SURR_FAST_SIGMOID = 0,   /* 1 / (10 |x| + 1)^2       */
  SNNQP_SURR_ATAN = 1,           /* 1 / (1 + (pi x)^2)        */
  SNNQP_SURR_SLAYER = 2,         /* exp(-5 |x|)               */
  SNNQP_SURR_SMOOTH_STEP = 3,    /* 1 on [-0.5, 0.5), else 0  */
  SNNQP_SURR_PIECEWISE_LINEAR = 4 /* relu(1 - 2 |x|)          */
};
/* quantisers, quant.py */
enum {
  SNNQP_Q_DUQ = 0,              /* quant.py:428-469  p0 = a, p1 = c           */
  SNNQP_Q_UNIFORM_STATIC = 1,   /* quant.py:322-358  p0 = xmax                */
  SNNQP_Q_PARAMETRIC_D = 2,     /* quant.py:361-425  p0 = step size           */
  SNNQP_Q_PARAMETRIC_D_XMAX = 3 /* quant.py:494-625  p0 = d, p1 = xmax (clipped) */
};
/* kernel selection for the fused blocks */
enum { SNNQP_IMPL_AUTO = 0, SNNQP_IMPL_GENERIC = 1, SNNQP_IMPL_MFMA = 2 };

/* flags written (OR-ed) by the checking kernels into a device int32 */
enum {
  SNNQP_FLAG_CODE_OVERFLOW = 1, /* |code| > 127: does not fit int8          */
  SNNQP_FLAG_MASK_NOT_BINARY = 2,
  SNNQP_FLAG_NOT_INTEGER = 4,   /* activation not an integer in [0, 255]    */
  SNNQP_FLAG_GT_ONE = 8,        /* activation > 1 (not a binary spike)      */
  SNNQP_FLAG_GT_127 = 16,       /* activation > 127 (not an int8 MFMA operand) */
  SNNQP_FLAG_GT_15 = 32         /* activation > 15 (does not fit an EV4 nibble)      */
};

/* Weights after the transforms of flax_qdense.py:74-85 / flax_qconv.py:147-156.
 * SNNQP_W_I8: integer codes (already multiplied by the 0/1 prune mask); the
 * contraction accumulates exactly in int32 and the current is
 * fl(fl(acc / L) * m)  (DuQ: L = n_lv - 1, m = c, quant.py:443,467; the other
 * quantisers: L = 1, m = step).  SNNQP_W_F32: fake-quantised float kernel; the
 * contraction is a float32 fmaf chain over k ascending ((kh, kw, cin) order).
 * Layout: [K][N] for dense, HWIO for convolutions, as the reference's params. */
typedef struct {
  int32_t wtype;
  const void *w;
  float L;
  float m;
  int32_t abs_sum_max; /* W_I8: a bound of |acc| per unit of input: with the non-negative
                        * inputs of the integer kernels (spikes, counts <= x_max),
                        * |acc| <= abs_sum_max * x_max.  Tightest: max over outputs of
                        * max(sum of positive codes, sum of |negative codes|); the
                        * max of sum_k |code| is valid too.  0 = unknown */
  int32_t code_max;    /* W_I8: max |code|; 0 = unknown.  Codes of magnitude <= 7 are
                          exact in fp6 (e2m3) and may take the f8f6f4 MFMA */
  const int32_t *col_sum; /* W_I8, dense layers, nullable: device int32 [N], sum over k of the
                          codes of each output feature.  Lets the MFMA dense kernel read
                          uint8 rows as x - 128 (any count 0..255) and add 128 * col_sum back */
  const void *wt_fp6;  /* W_I8, dense layers, nullable: the codes as fp6 MFMA tiles
                          (snnqp_pack_codes_fp6; needs code_max <= 7).  With it a dense block
                          over bit-packed rows runs on the f8f6f4 MFMA: 6 bits per code from
                          HBM / L2, K = 64 per instruction */
  uint32_t min_current_bits; /* float32 bits of the smallest non-zero |input current| the block
                          can see with the BatchNorm it is used with -- snnqp_current_min()
                          with bound = abs_sum_max (bit-packed inputs);
                          lets the conv kernels run u + (x - u) / tau as one fused
                          multiply-add when that is provably bit-identical.  0 = unknown */
  int32_t ch_stack_max; /* W_I8, the 2-channel event layer, 0 = unknown: with range(c) = the sum of
                          |code| of output channel c, the largest sum of the ranges of the four
                          channels that share an LDS bank column (ch_slots; without it the
                          channels 128 g + 32 w + n, w = 0..3).  Sizes the per-channel
                          dequantisation tables (a channel's table covers its own accumulator
                          range; the four channels of a column are stacked); unknown:
                          8 x abs_sum_max.  A value below the codes' is reported
                          (SNNQP_STATUS_BOUND) */
  const int32_t *ch_slots; /* W_I8, the event layer, nullable: device int32 [ceil(Cout / 128) * 128],
                          for every channel 4 * column + position: which of the 32 bank columns
                          of its 128-channel group holds its table and where in the column's
                          stack of four.  The 32 channels of a wave (32 w .. 32 w + 31) must name
                          32 different columns and no slot twice -- a balanced assignment keeps
                          the tallest column, hence the table, small.  NULL: column n = c mod 32,
                          position w */
  int32_t wt_cin;      /* W_I8, 3x3 conv blocks over bit-packed spikes: the input-channel count
                          `wt` was zero-padded to (snnqp_conv_lif_forward), a multiple of 32 in
                          [Cin, 128]; 0 = 32 ceil(Cin / 32), the packing rule.  Where Cin leaves the
                          upper 16 channels of the last 32-channel group empty (16 ceil(Cin / 16)
                          + 16 equals the padding), the upper 16 rows of that group's tiles are
                          not read (snnqp_set_conv_k16) */
  int32_t cout_fire;   /* W_I8, the 2-channel event layer (snnqp_conv_lif_forward[_pred] on U8 / EV1 /
                          EV4 / F32 frames, IMPL_MFMA route): the caller's assertion that the output
                          channels cout_fire .. Cout - 1 never fire -- silent padding of a compacted
                          block.  0 = every channel may fire; otherwise a multiple of 16 in (0, Cout],
                          anything else is refused before a launch.  Like the BatchNorm flags it is
                          not checked against the codes: the spike bits from cout_fire on are stored
                          as zeros, so a wrong value loses spikes without an error.  With cout_fire
                          + 16 == Cout and Cout a multiple of 32, a launch on bit-packed frames
                          (EV1), pool 1 or 2, no state carried in or out, every timestep in one
                          staging chunk, per-channel tables and the v_reset = 0 neuron with a
                          multiplied time constant computes the last 32-channel group in a
                          16-channel half: half the neuron updates of that group
                          (snnqp_set_event_half_group, snnqp_conv_event_half_group).  For such a
                          weight ch_stack_max / ch_slots must size the slot of channel cout_fire + j
                          for max(range(cout_fire + j), range(cout_fire - 16 + j)): on the half path
                          the slot holds the table of that twin.  The field takes the four bytes
                          that were tail padding: the struct's size and every other offset are as
                          before, and a caller that zeroes the struct says 0. */
} snnqp_weight_t;

/* Eval-mode BatchNorm folded on the host: y = fl(fl(fl(x - mean) * mul) + bias),
 * mul = rsqrt(var + eps) * scale (examples/tcja/models.py:101-107, applied at
 * spiking_learning.py:457-458).  All three device arrays have Cout entries.
 * `flags`: facts the caller knows about the arrays (it folded them on the host):
 * SNNQP_BN_MEAN_ZERO / SNNQP_BN_BIAS_ZERO = every mean / bias entry is +-0.0, so that
 * fl(x - 0) and fl(x + 0) equal x and a kernel may skip the instruction (a freshly
 * initialised BatchNorm has both).  Equal as numbers: for x = -0.0 the skipped form keeps
 * -0.0 where fl(-0.0 + 0.0) is +0.0.  The sign of a zero current never changes a spike or a
 * non-zero potential; it can show in the sign bit of a membrane potential that is exactly
 * zero (u_out), which compares equal.  SNNQP_BN_MUL_UNIFORM = every `mul` entry holds the same
 * bits (a freshly initialised BatchNorm: rsqrt(1 + eps) for every channel): a kernel that reads the
 * dequantised current from a table all channels share may fold the multiply into the entries --
 * fl(x * mul) computed once per entry instead of once per neuron update, the same float32
 * product.  0 = nothing known; other bits are refused. */
#define SNNQP_BN_MEAN_ZERO 1
#define SNNQP_BN_BIAS_ZERO 2
#define SNNQP_BN_MUL_UNIFORM 4
typedef struct {
  const float *mean;
  const float *mul;
  const float *bias;
  int32_t flags;
} snnqp_bn_t;

/* Neuron parameters.  `k`: tau for MULTI_STEP_LIF, sigmoid(tau_param) for
 * PARAMETRIC_LEAKY_IF; `decay`: device [Cout] sigmoid(tau) for LIF. */
typedef struct {
  int32_t kind;
  float k;
  float v_threshold;
  float v_reset;
  const float *decay;
} snnqp_neuron_t;

/* Convolution geometry (flax_qconv.py:76-94, :158-168); 1-D convolutions use
 * H = KH = 1.  A dense layer is the 1x1 convolution on a 1x1 image. */
typedef struct {
  int32_t H, W, Cin, Cout;
  int32_t KH, KW;
  int32_t stride_h, stride_w;
  int32_t pad_h_lo, pad_h_hi, pad_w_lo, pad_w_hi;
  int32_t in_dil_h, in_dil_w;   /* input_dilation  (lhs) */
  int32_t k_dil_h, k_dil_w;     /* kernel_dilation (rhs) */
  int32_t groups;               /* feature_group_count   */
} snnqp_conv_geom_t;

/* Geometry of a 3-D convolution (flax_qconv.py:93-171 with three spatial axes; index 0 = depth,
 * 1 = height, 2 = width): images [D][H][W][Cin], kernels [KD][KH][KW][Cin / groups][Cout]. */
typedef struct {
  int32_t D, H, W, Cin, Cout;
  int32_t KD, KH, KW;
  int32_t stride[3];
  int32_t pad_lo[3], pad_hi[3];
  int32_t in_dil[3];            /* input_dilation  (lhs) */
  int32_t k_dil[3];             /* kernel_dilation (rhs) */
  int32_t groups;               /* feature_group_count   */
} snnqp_conv3d_geom_t;

/* ABI version of this header: bumped whenever a struct or a signature below changes
 * (100: round 1; 200: snnqp_bn_t.flags, x_max / x_seen of snnqp_conv_lif_forward;
 * 300: SNNQP_EV1 / SNNQP_EV4 frame types, snnqp_pack_frames / snnqp_unpack_frames,
 * snnqp_fallback_counts; 301: snnqp_conv_dequant_form; 400: snnqp_dense_head_forward, snnqp_device_status,
 * snnqp_workqueue_*, snnqp_dense_lif_forward_ws; 500: float32 inputs into integer blocks --
 * x_flags of snnqp_conv_lif_forward / snnqp_dense_lif_forward_ws / snnqp_dense_head_forward, the
 * predicated snnqp_*_if entry points, snnqp_pack_bits_checked, snnqp_conv_gated_forward,
 * snnqp_dense_gated_forward, snnqp_quantize_ex, snnqp_conv_forward_if,
 * snnqp_conv3d_*; 501: snnqp_weight_t.ch_stack_max / ch_slots, the *_gated_*_ex pack calls; 502:
 * snnqp_pack_frames_checked, snnqp_conv_lif_forward_pred, SNNQP_BN_MUL_UNIFORM; 503:
 * snnqp_scatter_spike_channels; 505: training of the dense blocks -- SNNQP_SURR_*,
 * snnqp_lif_forward_save, snnqp_lif_backward, snnqp_dense_weight_grad, snnqp_dense_input_grad;
 * 506: training of the conv blocks -- snnqp_conv_weight_grad, snnqp_conv_input_grad,
 * snnqp_conv_grad_splits, snnqp_conv_weight_grad_workspace_bytes, snnqp_maxpool2x2_backward;
 * 507: snnqp_conv_forward_ex -- currents from the bit-input MFMA conv; within 507, layout-
 * compatible: snnqp_weight_t.cout_fire in the struct's former tail padding,
 * snnqp_set_event_half_group, snnqp_conv_event_half_group, snnqp_set_event_wave_spread,
 * snnqp_conv_event_wave_spread, snnqp_set_event_quarter16, snnqp_conv_event_quarter16; training of
 * CextNet's gated stages --
 * snnqp_gate_pool_grad_gate, snnqp_gate_pool_grad_input, snnqp_conv_weight_grad_f64,
 * snnqp_conv_weight_grad_f64_workspace_bytes; the batched event front end snnqp_events_bin and its augmenting
 * form snnqp_events_bin_aug with snnqp_event_aug_t and its mixing form snnqp_events_bin_mix; the host-side
 * query snnqp_conv_float_form; the host-side plan queries snnqp_conv_gated_plan,
 * snnqp_dense_gated_plan, snnqp_dense_wide_plan, snnqp_dense_fp6_plan, snnqp_dense_mfma_plan;
 * streaming inference --
 * snnqp_dense_head_forward_state, snnqp_vote_accumulate, snnqp_vote_counts; the rate encoder
 * snnqp_rate_encode with SNNQP_ENCODE_*; training of the PLIF and LIF neurons --
 * snnqp_neuron_forward_save, snnqp_neuron_backward, snnqp_neuron_backward_splits,
 * snnqp_neuron_backward_workspace_bytes; training over windows of a recording --
 * snnqp_lif_forward_save_state, snnqp_lif_backward_state, snnqp_neuron_forward_save_state,
 * snnqp_neuron_backward_state; training a conv block with rematerialisation --
 * snnqp_bn_lif_forward_state, snnqp_maxpool2x2_backward_h; magnitude pruning on the device --
 * snnqp_magnitude_prune, snnqp_magnitude_prune_workspace_bytes: new entry points, nothing else moves).
 * A binding compares snnqp_version()
 * with the SNNQP_VERSION it was written against and refuses a library of another version (_lib.py does). */
#define SNNQP_VERSION 507
int snnqp_version(void);
const char *snnqp_last_error(void);
/* Extra compiler flags the library was built with: "" for the product build
 * (snnquantprune_amd/csrc/build.py); diagnostic builds (tools/diag_build.py, written
 * under diag_build/, never in-tree) report their -D switches here.  Tests and bench.py
 * refuse a library whose string is not empty. */
const char *snnqp_build_flags(void);

/* Output spatial size of `g` (same rule as lax.conv_general_dilated). */
/* The K walk of the bit-input 3x3 conv kernel (snnqp_conv_lif_forward, SNNQP_IMPL_MFMA, BITS
 * input).  1 (the default): when Cin mod 32 is in 1..16 the kernel walks the last 32-channel group
 * in 16-channel units and reads neither the upper 16 rows of that group's tiles in `wt` nor bits
 * 16..31 of a pixel's last spike word.  0: it walks whole groups (the same results: those bits are
 * zero by the contract of the input, those rows zero by the packing rule).  Process-wide, for the
 * launches enqueued after the call; returns the previous setting.  A negative argument only
 * queries. */
int snnqp_set_conv_k16(int enabled);
/* The half group of the event layer (snnqp_weight_t.cout_fire).  1 (the default): a launch that
 * meets the conditions stated there computes the last channel group in a 16-channel half.  0: it
 * computes the whole group and cout_fire only masks the stored bits (the same results).
 * Process-wide, for the launches enqueued after the call; returns the previous setting.  A negative
 * argument only queries. */
int snnqp_set_event_half_group(int enabled);
/* 1 when snnqp_conv_lif_forward(x of `in_type`, T, g, w, nrn, pool, x_max; IMPL_AUTO / IMPL_MFMA)
 * would run on the half-group path under the current setting, 0 when not (has_state: u0 or u_out
 * given), a negative error for a null or malformed descriptor.  Launches nothing. */
int snnqp_conv_event_half_group(int in_type, int32_t T, const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                                const snnqp_neuron_t *nrn, int has_state, int pool, int x_max);
/* The wave spread of the event layer.  1 (the default): among the launches of the half group's family
 * (bit-packed frames, pool 1 or 2, no state carried, one staging chunk, per-channel tables, the
 * v_reset = 0 neuron with a multiplied time constant) the two whose four waves would carry unequal
 * work -- Cout = 96 on the half-group path, and Cout = 64 not on it -- give every wave one (channel
 * group, 4x8 tile) unit of channels 0..63 and, at 96, a quarter of the half group's neuron updates.
 * 0: wave w computes channel group w (the same results).  Process-wide, for the launches enqueued
 * after the call; returns the previous setting.  A negative argument only queries. */
int snnqp_set_event_wave_spread(int enabled);
/* 1 when that launch would run on the spread path under the current settings (of this switch and of
 * snnqp_set_event_half_group), 0 when not, a negative error: as snnqp_conv_event_half_group. */
int snnqp_conv_event_wave_spread(int in_type, int32_t T, const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                                 const snnqp_neuron_t *nrn, int has_state, int pool, int x_max);
/* The quarter of the half group in the spread launch of Cout = 96.  1 (the default): a wave takes its
 * quarter -- 16 channels x 16 pixels -- from one 16x16x64 int8 matrix instruction with a four-register
 * product.  0: it issues the half group's whole 32x32x32 product and reads four registers of it (the
 * same results).  Process-wide, for the launches enqueued after the call; returns the previous setting.
 * A negative argument only queries. */
int snnqp_set_event_quarter16(int enabled);
/* 1 when that launch would take its quarters that way under the current settings (of this switch, of
 * snnqp_set_event_wave_spread and of snnqp_set_event_half_group), 0 when not, a negative error: as
 * snnqp_conv_event_half_group. */
int snnqp_conv_event_quarter16(int in_type, int32_t T, const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                               const snnqp_neuron_t *nrn, int has_state, int pool, int x_max);

int snnqp_conv_out_shape(const snnqp_conv_geom_t *g, int32_t *OH, int32_t *OW);

/* ---- weight transforms --------------------------------------------------
 * replaces: cfg.weight(bits, g_scale)(kernel) + prune()(kernel_fwd) at
 *           flax_qdense.py:74-85 and flax_qconv.py:147-156
 *           (quantiser forwards quant.py:322-625, prune quant.py:472-491).
 * w, mask (nullable), fq_out (nullable, float32 fake-quantised*mask),
 * codes_out (nullable, int8 codes*mask), flags (nullable int32, OR-ed).
 * Rounding is round-half-to-even (jnp.round, quant.py:88-90). */
int snnqp_quantize(int kind, const float *w, const float *mask, int64_t n,
                   int bits, float p0, float p1, float *fq_out,
                   int8_t *codes_out, int32_t *flags, snnqp_stream_t stream);
/* The same with the reference's `sign` argument (Quantizer.__call__(x, sign), quant.py:331,
 * :374, :439, :512): sign = 0 quantises to the unsigned levels 0 .. 2^bits - 1 (num_levels /
 * q_pos = 2^bits - 1, lower clip bound 0; DuQ keeps hard_tanh and only changes n_lv,
 * quant.py:458-467).  snnqp_quantize is sign = 1, what QuantDense / QuantConv pass
 * (flax_qdense.py:76).  int8 codes exist for unsigned widths up to 7 bits only
 * (SNNQP_FLAG_CODE_OVERFLOW beyond). */
int snnqp_quantize_ex(int kind, const float *w, const float *mask, int64_t n,
                      int bits, int sign, float p0, float p1, float *fq_out,
                      int8_t *codes_out, int32_t *flags, snnqp_stream_t stream);

/* Layout step of the pack: int8 codes [K][N] (dense kernel / flattened HWIO
 * convolution kernel, as the reference stores them) -> MFMA B-operand tiles
 * wt[Npad/32][K/32][64][16]: for column block nb and k-step ks, lane
 * l = (n & 31) + 32 h holds bytes k = 32 ks + 16 h + j (j < 16) of column
 * n = 32 nb + (l & 31); columns >= N are zero.  One contiguous 1 KiB read per
 * wave and k-step.  K and Npad must be multiples of 32. */
int snnqp_pack_codes_mfma(const int8_t *w, int64_t K, int32_t N, int32_t Npad,
                          int8_t *wt, snnqp_stream_t stream);

/* The "packed int load" of a dense kernel whose codes have magnitude <= 7 (DuQ up to 4 bits):
 * int8 codes [K][N] -> fp6 (e2m3) B-operand tiles of v_mfma_scale_f32_32x32x64_f8f6f4,
 * wt6[Npad/32][ceil(K/64)][1536 B]: for column block nb and k-step ks, lane l = (n & 31) + 32 h
 * holds k = 64 ks + 32 h + j (j < 32) of column n = 32 nb + (l & 31), value j at bits
 * [6 j, 6 j + 6) of six dwords; a tile stores dwords 0..3 of its 64 lanes (1 KiB), then dwords
 * 4..5 (512 B).  Rows beyond K and columns beyond N are zero.  0.75 bytes per code. */
int snnqp_pack_codes_fp6(const int8_t *w, int64_t K, int32_t N, int32_t Npad, void *wt6,
                         snnqp_stream_t stream);

/* ---- activation format helpers ------------------------------------------
 * replaces: nothing in the reference (its activations are float32 arrays);
 * they convert between the reference's float32 layout and the packed formats
 * the kernels read/write.  rows x C logical elements. */
int snnqp_inspect_f32(const float *x, int64_t n, int32_t *flags,
                      snnqp_stream_t stream);
/* inspect_u8: *flags (zeroed by the caller) = (max(x) << 8) | SNNQP_FLAG_GT_* bits */
int snnqp_inspect_u8(const uint8_t *x, int64_t n, int32_t *flags,
                     snnqp_stream_t stream);
int snnqp_f32_to_u8(const float *x, uint8_t *y, int64_t n,
                    snnqp_stream_t stream);
/* narrow_f32: inspect_f32 + f32_to_u8 + inspect_u8 in one pass over x.  flags[0]
 * (zeroed by the caller) = (max << 8) | SNNQP_FLAG_GT_*, flags[1] = SNNQP_FLAG_NOT_INTEGER
 * or 0; y is the uint8 copy, meaningful when flags[1] == 0. */
int snnqp_narrow_f32(const float *x, uint8_t *y, int64_t n, int32_t *flags,
                     snnqp_stream_t stream);
/* Event frames between uint8 [frames][H][W][2] and the wire formats SNNQP_EV1 /
 * SNNQP_EV4 (device side of the host feed; the host packs with the same layout).
 * pack: a value the format cannot hold is saturated (EV1: > 1 -> 1, EV4: > 15 -> 15) and
 * flagged (SNNQP_FLAG_GT_ONE / SNNQP_FLAG_GT_15 OR-ed into the nullable device word
 * `flags`).  unpack: exact inverse on every tensor that packed without a flag. */
int snnqp_pack_frames(const uint8_t *x, int64_t frames, int32_t H, int32_t W, int fmt,
                      void *y, int32_t *flags, snnqp_stream_t stream);
int snnqp_unpack_frames(const void *x, int fmt, int64_t frames, int32_t H, int32_t W,
                        uint8_t *y, snnqp_stream_t stream);
/* uint8 (in_type SNNQP_U8) or float32 (SNNQP_F32: the reference's own input dtype,
 * flax_qconv.py:101) frames [frames][H][W][2] -> SNNQP_EV1 in ONE pass at the rate of HBM, with
 * the check the event layer would make while staging them: `flags` (required; zeroed by this call
 * on `stream`) receives SNNQP_FLAG_GT_ONE when a value is neither 0 (-0.0 counts) nor 1, and
 * SNNQP_FLAG_NOT_INTEGER when a float32 value is not an integer in [0, 255].  A flagged result is
 * not the tensor: it serves as the speculative half of
 *     snnqp_pack_frames_checked(x, ..., ev1, flags);
 *     snnqp_conv_lif_forward(ev1, SNNQP_EV1, ...);                 binary frames: 1/8 .. 1/32 of the bytes,
 *     snnqp_conv_lif_forward_pred(flags, x, in_type, ...);         the event layer's fastest variant
 * where the last call redoes the block on the frames as they are iff the word is set. */
int snnqp_pack_frames_checked(const void *x, int in_type, int64_t frames, int32_t H, int32_t W,
                              uint32_t *y, int32_t *flags, snnqp_stream_t stream);
int snnqp_pack_bits(const void *x, int in_type, int64_t rows, int32_t C,
                    uint32_t *bits, snnqp_stream_t stream);
/* the same, and SNNQP_FLAG_GT_ONE is OR-ed into the device word `flags` (nullable; zeroed by the
 * caller) when an element is neither 0 nor 1 -- the raster then is not the tensor */
int snnqp_pack_bits_checked(const void *x, int in_type, int64_t rows, int32_t C,
                            uint32_t *bits, int32_t *flags, snnqp_stream_t stream);
int snnqp_unpack_bits(const uint32_t *bits, int64_t rows, int32_t C, float *y,
                      snnqp_stream_t stream);

/* ---- connection only (no neuron) ------------------------------------------
 * replaces: lax.dot_general at flax_qdense.py:87-89 and
 *           lax.conv_general_dilated at flax_qconv.py:158-168.
 * x: NB images [NB][H][W][Cin] (type in_type); y: float32 [NB][OH][OW][Cout];
 * acc (nullable): int32 accumulators, same shape (W_I8 with integer input). */
int snnqp_conv_forward(const void *x, int in_type, int64_t NB,
                       const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                       float *y, int32_t *acc, snnqp_stream_t stream);
/* Which kernel snnqp_conv_forward(x, in_type, NB, g, w, y, acc = NULL) runs.  Launches nothing; `x`
 * is looked at for its address only and never dereferenced.  A negative SNNQP_E* for a null or
 * malformed descriptor (null g, w, w->w or x; NB outside [0, 2^31); unknown input or weight type; a
 * geometry snnqp_conv_forward refuses).  SNNQP_FLOAT_FORM_DIRECT (0): the direct-form kernel, one
 * thread per output -- integer codes, or a float32 kernel whose geometry the float32 MFMA
 * connection does not serve (strided, dilated, grouped, or pad_lo + pad_hi != K - 1).  Otherwise
 * that connection (y[m][n] = the k-ascending float32 fmaf chain from +0), as tile + mode:
 *   SNNQP_FLOAT_FORM_TILE(f)  64 or 128: a workgroup owns tile x tile outputs.  128 when
 *                             ceil(M / 128) * ceil(N / 128) >= 192 and N > 64, M = NB H W, N = Cout.
 *   SNNQP_FLOAT_FORM_MODE(f)  how a chunk of 16 k is staged: 0 float32, Cin % 16 == 0; 1 float32,
 *                             Cin % 4 == 0; 2 element by element (any type and Cin); 3 uint8 / spike
 *                             words with one tap per chunk (a 1 x 1 kernel -- uint8: Cin % 8 == 0 --
 *                             or Cin % 16 == 0; uint8 only when x is 8-byte aligned, else mode 2).
 * Modes 0 and 1 read float32 x, and Cout % 4 == 0 reads w, in 16-byte units: nothing is promised
 * for such pointers aligned below 16 bytes. */
#define SNNQP_FLOAT_FORM_DIRECT 0
#define SNNQP_FLOAT_FORM_TILE(f) ((f) & ~3)
#define SNNQP_FLOAT_FORM_MODE(f) ((f) & 3)
int snnqp_conv_float_form(const void *x, int in_type, int64_t NB,
                          const snnqp_conv_geom_t *g, const snnqp_weight_t *w);
/* The same call site with a choice of kernel.  On integer codes and a spike raster
 * snnqp_conv_forward runs the direct-form kernel, one thread per output; here the 3x3 / stride 1
 * / pad 1 connection over SNNQP_BITS input with 1 <= Cin <= 128 (any H, W, Cout) runs as an MFMA
 * implicit GEMM that hands back currents: v_mfma_scale_f32_32x32x64_f8f6f4 (fp4 spikes x fp6
 * codes) for code_max in 1..7, v_mfma_i32_32x32x32_i8 for wider or unknown codes.  The
 * accumulator is the same exact integer and y = fl(fl(acc / L) * m) is computed with the same
 * instructions, so y and acc hold the bits snnqp_conv_forward writes.
 * wt    the codes tiled by snnqp_pack_codes_mfma exactly as snnqp_conv_lif_forward documents
 *       (HWIO kernel zero-padded along Cin to 32 ceil(Cin / 32), or to w->wt_cin, flattened to
 *       [9 * that][Cout]); bits of a pixel's last spike word beyond Cin must be zero.
 * acc   nullable int32, the shape of y: the accumulators.
 * impl  SNNQP_IMPL_GENERIC: exactly snnqp_conv_forward (its float32 MFMA route for W_F32
 *       included; wt is not read).  SNNQP_IMPL_MFMA: the kernel above, or SNNQP_EUNSUPPORTED with
 *       the reason (weights not int8 codes; not 3x3 / stride 1 / pad 1 / undilated / ungrouped;
 *       input not SNNQP_BITS; Cin > 128; wt NULL; wt_cin not a multiple of 32 in [Cin, 128]; 2^30
 *       patches of 4x8 pixels or more).  SNNQP_IMPL_AUTO: that kernel when it can, otherwise
 *       snnqp_conv_forward.  A refused call has launched nothing and leaves y and acc untouched;
 *       NB == 0 enqueues nothing.  snnqp_fallback_counts is not touched: it counts fused blocks.
 * x, y and acc need 4-byte alignment only. */
int snnqp_conv_forward_ex(const void *x, int in_type, int64_t NB,
                          const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                          const int8_t *wt, float *y, int32_t *acc, int impl,
                          snnqp_stream_t stream);
/* The same, executed only if *pred != 0 when the stream reaches it: the float32 connection behind
 * a speculative integer one (a float32 tensor narrowed by snnqp_narrow_f32, whose flag word is
 * `pred`) -- QuantDense / QuantConv called on their own with float32 inputs
 * (flax_qdense.py:67, flax_qconv.py:101).  Direct form, same fmaf chain. */
int snnqp_conv_forward_if(const int32_t *pred, const void *x, int in_type, int64_t NB,
                          const snnqp_conv_geom_t *g, const snnqp_weight_t *w, float *y,
                          snnqp_stream_t stream);

/* ---- 3-D QuantConv, alone or as a SpikingBlock --------------------------------------------
 * replaces: lax.conv_general_dilated at flax_qconv.py:158-168 for kernels with three spatial axes
 *           (and SpikingBlock.__call__, spiking_learning.py:446-462, around it).
 * x [T][B][D][H][W][Cin] (strides in elements, words for SNNQP_BITS; types F32 / U8 / BITS);
 * nrn null or kind SNNQP_NEURON_NONE: the connection alone (pass T = 1, B = the number of images),
 * s_out = float32 currents [B][OD][OH][OW][Cout] (s_type SNNQP_F32); else s_out = spikes
 * [T][B][OD][OH][OW][Cout] (F32 or BITS), u0 / u_out [B][OD][OH][OW][Cout].  Contracts as everywhere:
 * int8 codes x integer input = exact int32 sum, then fl(fl(acc / L) * m); float32 weights = fmaf
 * chain over (kd, kh, kw, cin) ascending.  Direct form (one thread per output neuron): no shipped
 * model has a 3-D layer.  pred (nullable): skip the launch unless *pred != 0, as the *_if calls. */
int snnqp_conv3d_out_shape(const snnqp_conv3d_geom_t *g, int32_t *OD, int32_t *OH, int32_t *OW);
int snnqp_conv3d_lif_forward(const int32_t *pred, const void *x, int in_type, int64_t x_stride_t,
                             int64_t x_stride_b, int32_t T, int32_t B,
                             const snnqp_conv3d_geom_t *g, const snnqp_weight_t *w,
                             const snnqp_bn_t *bn, const snnqp_neuron_t *nrn, const float *u0,
                             float *u_out, void *s_out, int s_type, snnqp_stream_t stream);

/* ---- connection on gate x raster (no neuron) ------------------------------------
 * replaces: QuantConv (flax_qconv.py:93-171; 3x3, stride 1, pad 1) on the product of a spike
 *           raster and a per-(image, channel) gate -- the conv block behind a TCJA gate,
 *           x = s * sigmoid(...)[:, :, None, None, :], examples/tcja/models.py:95-97 -> :149-187.
 * The 'gint' contraction: the gate of a channel multiplies all
 * nine taps of that channel, so it is factored out of them --
 *     I[p][c][o] = sum over the taps of code * s          (exact integer, on the matrix pipe)
 *     acc[p][o]  = fmaf(gate[c], I[p][c][o], acc[p][o])   for c = 0 .. Cin - 1, from +0
 *     y[p][o]    = fl(fl(acc / L) * m)
 * s     [NB][H][W][ceil(Cin / 32)] spike words (SNNQP_BITS), gate [NB][Cin] float32,
 * y     float32 [NB][H][W][Cout].  w: SNNQP_W_I8 codes with code_max <= 7 (DuQ up to 4 bits; up to
 * 127 with the _ex pack below), HWIO; packed: the same codes as snnqp_pack_codes_gated lays them out
 * (snnqp_conv_gated_packed_bytes bytes).  Cin in {32, 64, 96, 128}; any H, W, Cout.
 * SNNQP_EUNSUPPORTED otherwise: the caller multiplies (snnqp_apply_gate) and takes the float32
 * connection (snnqp_conv_forward). */
int64_t snnqp_conv_gated_packed_bytes(int32_t Cin, int32_t Cout);
int snnqp_pack_codes_gated(const int8_t *w, int32_t Cin, int32_t Cout, void *packed,
                           snnqp_stream_t stream);
/* Codes beyond e2m3 (code_max = max |code| up to 127: DuQ up to 8 bits, the reference's shipped TCJA
 * configs): packed as two six-bit digits in the e3m2 format, code = 16 hi + lo, in the two K blocks
 * of the matrix instruction with a block scale of 2^4 on the second -- one instruction still
 * returns the exact integer sum of a channel's taps, at the same rate.  The _ex forms take code_max (<= 7: the fp6 layout above);
 * snnqp_conv_gated_forward picks the kernel by w->code_max, `packed` must come from the pack call
 * with the same code_max. */
int64_t snnqp_conv_gated_packed_bytes_ex(int32_t Cin, int32_t Cout, int32_t code_max);
int snnqp_pack_codes_gated_ex(const int8_t *w, int32_t Cin, int32_t Cout, int32_t code_max,
                              void *packed, snnqp_stream_t stream);
int snnqp_conv_gated_forward(const uint32_t *s, const float *gate, int64_t NB,
                             const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                             const void *packed, float *y, snnqp_stream_t stream);
/* Which launches snnqp_conv_gated_forward makes for Cout outputs and w->code_max = code_max (and
 * which layout snnqp_pack_codes_gated_ex writes).  Launches nothing.  The outputs are walked in
 * tiles of 32, OT = ceil(Cout / 32):
 *   full_groups  gridDim.y of the launch whose workgroups hold four tiles each (0: no such launch);
 *                workgroup row y holds the tiles 4 y .. 4 y + 3.
 *   rest_tiles   0..3: the tiles of the one further launch (gridDim.y = 1) on the last OT % 4 tiles.
 *   wide         0: e2m3 codes (code_max <= 7); 1: two e3m2 digits per code and the 2^4 block scale.
 * SNNQP_EINVAL for Cout < 1, code_max outside 1..127 or a null pointer. */
int snnqp_conv_gated_plan(int32_t Cout, int32_t code_max, int32_t *full_groups, int32_t *rest_tiles,
                          int32_t *wide);

/* The same contraction for a QuantDense (flax_qdense.py:87-89) on the channel-major flattening of
 * gate x raster -- the first dense block behind the second TCJA gate, x[(c HW + p)] = gate[c] *
 * s[p][c], examples/tcja/models.py:97 -> :189-190 -> :200-216:
 *     I[c][o] = sum over the HW positions of code[c HW + p][o] * s[p][c]     (exact integer)
 *     acc[o]  = fmaf(gate[c], I[c][o], acc[o])   for c = 0 .. C - 1, from +0
 *     y[o]    = fl(fl(acc / L) * m)
 * s [NB][HW][ceil(C / 32)] spike words, gate [NB][C] float32, y float32 [NB][N]; w: SNNQP_W_I8
 * codes [C HW][N] with code_max <= 7; packed: snnqp_pack_codes_dense_gated's layout
 * (snnqp_dense_gated_packed_bytes bytes).  HW <= 16, C in {32, 64, 96, 128}; SNNQP_EUNSUPPORTED
 * otherwise (the caller multiplies the gate out and takes snnqp_conv_forward). */
int64_t snnqp_dense_gated_packed_bytes(int32_t C, int32_t N);
int snnqp_pack_codes_dense_gated(const int8_t *w, int32_t C, int32_t HW, int32_t N, void *packed,
                                 snnqp_stream_t stream);
/* (codes up to 127 as two e3m2 digits, as snnqp_pack_codes_gated_ex: the _ex forms take code_max) */
int64_t snnqp_dense_gated_packed_bytes_ex(int32_t C, int32_t N, int32_t code_max);
int snnqp_pack_codes_dense_gated_ex(const int8_t *w, int32_t C, int32_t HW, int32_t N, int32_t code_max,
                                    void *packed, snnqp_stream_t stream);
int snnqp_dense_gated_forward(const uint32_t *s, const float *gate, int64_t NB, int32_t HW,
                              int32_t C, int32_t N, const snnqp_weight_t *w,
                              const void *packed, float *y, snnqp_stream_t stream);
/* The launch of snnqp_dense_gated_forward for N outputs and w->code_max = code_max (and the layout
 * snnqp_pack_codes_dense_gated_ex writes).  Launches nothing.
 *   grid_y  workgroups per 32 images: each holds up to 512 outputs, four tiles of 32 per wave.
 *   wide    as snnqp_conv_gated_plan.
 * SNNQP_EINVAL for N < 1, code_max outside 1..127 or a null pointer. */
int snnqp_dense_gated_plan(int32_t N, int32_t code_max, int32_t *grid_y, int32_t *wide);

/* ---- fused SpikingBlock ---------------------------------------------------
 * replaces: SpikingBlock.__call__ (nn.scan over T of connection -> norm ->
 *           neuron), spiking_learning.py:446-462, with QuantConv / QuantDense
 *           as connection_fn, nn.BatchNorm (eval) as norm_fn, and -- when
 *           pool == 2 -- the 2x2 max-pool that follows it in
 *           examples/tcja/models.py:145-147.
 * x     [T][B][H][W][Cin] with element strides x_stride_t / x_stride_b
 *       (words for SNNQP_BITS); rows [H][W][Cin] are contiguous.
 * bn    nullable.  u0 nullable (zeros, initialize_carry :464-472),
 *       float32 [B][OH][OW][Cout].  u_out nullable, same shape.
 * s_out spikes, type s_type (SNNQP_F32: 0.0/1.0, or SNNQP_BITS),
 *       [T][B][OH/pool][OW/pool][Cout].
 * impl  SNNQP_IMPL_GENERIC: direct form, any geometry / types.
 *       SNNQP_IMPL_MFMA: MFMA implicit GEMM (fp6 codes x fp4 spikes when
 *       code_max <= 7, else int8); needs W_I8, 3x3 / stride 1 / pad 1 / no
 *       dilation / groups 1 and (BITS input with Cin <= 128 and `wt` = the codes
 *       of the kernel zero-padded along Cin to Cpad = 32 ceil(Cin / 32) (or to
 *       w->wt_cin, a wider multiple of 32 up to 128), tiled by snnqp_pack_codes_mfma
 *       with K = 9 * Cpad (row = tap * Cpad + cin: int8 tile tap * Cpad / 32 + group);
 *       a pixel keeps its ceil(Cin / 32) spike words, zero bits beyond Cin (bits 16..31 of the
 *       last word are not even read when Cin mod 32 is in 1..16, snnqp_set_conv_k16) --
 *       or U8 input with Cin == 2, any count 0..255; or EV1 / EV4 input, Cin == 2: the packed
 *       frames are staged directly, 1/8 (binary) or 1/2 (counts <= 15) of the uint8 bytes;
 *       x_max / x_seen apply to EV4 as to U8), s_type BITS;
 *       any H, W, Cout and neuron kind.  SNNQP_IMPL_AUTO picks MFMA when it can.
 *       EV1 / EV4 input is read by the MFMA kernel only: a block it does not take (s_type F32,
 *       impl GENERIC, ...) is refused with SNNQP_EUNSUPPORTED and not counted as a fallback --
 *       unpack the frames first (snnqp_unpack_frames).
 * x_max the largest input value the caller EXPECTS (1 for spikes and binary event frames;
 *       0 = unknown, taken as 1): with the weights' abs_sum_max it sizes the LDS tables the
 *       MFMA kernels dequantise through.  It is a hint, not a promise: the U8 kernel takes
 *       the maximum of every chunk of input it stages and runs the general path (any count up
 *       to 255, arithmetic dequantisation) for a chunk that exceeds it -- same results, slower.
 * x_seen nullable, EIGHT device words the caller zeroes: [0] is atomically max-ed with the
 *       largest U8 input value the launch met, [1..5] receive the number of staged chunks (a
 *       patch x up to 32 timesteps) whose largest value was <= 1, 2, <= 7, <= 31, above; [6] the
 *       number of those whose largest value was exactly 3 (part of [3]: the per-channel tables
 *       reach a hint of 3 on typical pruned layers, not 7); [7] is reserved.  From these the caller refines its next hint asynchronously -- a hint
 *       that covers MOST chunks is the fast one: a hot pixel then costs its own few chunks the
 *       general path instead of the whole batch the slower tables.  Nothing ever waits for it.
 * FLOAT32 INPUT INTO INTEGER CODES (the reference casts every input to float32, flax_qconv.py:101,
 *       flax_qdense.py:67; its event frames and spike rasters are integer-valued float32 tensors).
 *       With SNNQP_W_I8 weights, in_type SNNQP_F32 and Cin == 2 the event-layer MFMA kernel stages
 *       the float32 frames IN PLACE (strides in elements): every value is converted to its uint8
 *       count on the way into LDS and checked while it waits in a register.  x_flags: one device
 *       word, zeroed by this call on `stream` in front of the kernel; the kernel ORs
 *       SNNQP_FLAG_NOT_INTEGER into it when a staged value is not an integer in [0, 255] (-0.0
 *       counts as 0) -- the launch's results are then meaningless and the caller's
 *       snnqp_conv_lif_forward_if(x_flags, ...) with the float32 kernel, enqueued right behind,
 *       redoes the block.  Nothing is read back: the pair is enqueued unconditionally and can be
 *       captured into a graph.  x_flags is required for this combination, ignored otherwise.
 *       Other geometries refuse float32 input into integer codes (SNNQP_EUNSUPPORTED): narrow
 *       it with snnqp_narrow_f32 / snnqp_pack_bits_checked (their flag words serve as the
 *       predicate in the same way). */
int snnqp_conv_lif_forward(const void *x, int in_type, int64_t x_stride_t,
                           int64_t x_stride_b, int32_t T, int32_t B,
                           const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                           const int8_t *wt, const snnqp_bn_t *bn,
                           const snnqp_neuron_t *nrn, const float *u0,
                           float *u_out, void *s_out, int s_type, int pool,
                           int impl, int x_max, int32_t *x_seen, int32_t *x_flags,
                           snnqp_stream_t stream);

/* snnqp_conv_lif_forward on the event layer's MFMA kernel (3x3, stride 1, pad 1, Cin = 2; in_type
 * SNNQP_U8, SNNQP_EV4 or SNNQP_F32), enqueued unconditionally but EXECUTED only if *pred != 0 when the
 * stream reaches it: the frames in their own format behind a speculative launch on their
 * bit-packed copy (snnqp_pack_frames_checked).  Same arguments and results as
 * snnqp_conv_lif_forward with SNNQP_IMPL_MFMA (x_flags is zeroed on the stream whether or not the
 * kernel runs; x_seen is reported into only when it runs); SNNQP_EUNSUPPORTED for any other block.
 * When it does not run it costs one grid of workgroups that return at once.
 * replaces: the same call site as snnqp_conv_lif_forward. */
int snnqp_conv_lif_forward_pred(const int32_t *pred, const void *x, int in_type, int64_t x_stride_t,
                                int64_t x_stride_b, int32_t T, int32_t B,
                                const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                                const int8_t *wt, const snnqp_bn_t *bn,
                                const snnqp_neuron_t *nrn, const float *u0,
                                float *u_out, void *s_out, int s_type, int pool,
                                int x_max, int32_t *x_seen, int32_t *x_flags,
                                snnqp_stream_t stream);

/* The same block on the direct-form kernel (any geometry, any types; SNNQP_W_F32 weights: the
 * fmaf chain over (kh, kw, cin) ascending), enqueued unconditionally but EXECUTED only if
 * *pred != 0 when the stream reaches it (pred: a device word, e.g. the x_flags of the speculative
 * integer launch in front of it, or flags[1] of snnqp_narrow_f32).  It writes the same outputs
 * (pool == 2: the 2x2 max-pool fused, spikes [T][B][OH/2][OW/2][Cout]); when it does not run it
 * costs one small grid.  Together: a float32 tensor whose values are all integers in [0, 255]
 * gets the exact-integer contraction, any other tensor the reference's float32 one -- decided per
 * tensor on the device, with no read-back.
 * replaces: the same call site as snnqp_conv_lif_forward. */
int snnqp_conv_lif_forward_if(const int32_t *pred, const void *x, int in_type, int64_t x_stride_t,
                              int64_t x_stride_b, int32_t T, int32_t B,
                              const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                              const snnqp_bn_t *bn, const snnqp_neuron_t *nrn, const float *u0,
                              float *u_out, void *s_out, int s_type, int pool,
                              snnqp_stream_t stream);

/* Blocks that SNNQP_IMPL_AUTO handed to the direct-form kernel since the library was loaded
 * (or the last reset): it serves every geometry and type, 20-25 x slower than the MFMA kernels.
 * `reason` (nullable, reason_len bytes) receives why the last one fell back, e.g.
 * "conv: bit input needs Cin <= 128".  With SNNQP_LOG_FALLBACKS set in the environment every
 * new reason is also printed to stderr.  No reference counterpart (diagnostic). */
int snnqp_fallback_counts(int64_t *conv_blocks, int64_t *dense_blocks, char *reason,
                          int32_t reason_len, int reset);

/* ---- device status, work-queue bookkeeping (no reference counterpart: diagnostics) ----------
 * The conv kernels walk their patches through per-launch work queues and the split-K dense
 * kernel hands partial sums over through tickets; both rely on counters that are zero when a
 * launch begins.  A launch that ends with its bookkeeping not adding up (its results may be
 * wrong) stores a code in the device's status word -- page-locked host memory, read without any
 * synchronisation -- and every later snnqp_conv_lif_forward / snnqp_dense_lif_forward /
 * snnqp_dense_head_forward on that device returns SNNQP_EHIP until the word is reset. */
#define SNNQP_STATUS_QUEUE_CORRUPT 1u /* a conv launch's patches did not add up */
#define SNNQP_STATUS_TICKET 2u        /* a split-K dense launch drew a ticket out of range */
#define SNNQP_STATUS_BOUND 4u         /* snnqp_weight_t.abs_sum_max below a one-sided code sum of its
                                       * weights (checked once per weights on the device, after the
                                       * first launch that used them: the conv kernels size their
                                       * dequantisation tables by it) */
int snnqp_device_status(int device, uint32_t *codes, int reset);
/* Launches captured into a graph take a work-queue slot of their own (see the top of this file).
 * mark: the number of capture slots handed out on `device` so far.  release: the slots handed out
 * between two marks go back to the pool -- call it when the graph that was captured between the
 * marks has been destroyed and its last replay has completed. */
int snnqp_workqueue_capture_mark(int device, int64_t *mark);
int snnqp_workqueue_capture_release(int device, int64_t mark_begin, int64_t mark_end);
/* Since the library was loaded (or the last reset): conv launches that walked their patches
 * statically because no capture slot was left / because their eager slot was still in flight
 * (same results, worse balance), and bit-input conv launches that ran the arithmetic
 * dequantisation because the device failed (or, under capture, had not yet run) the probe of the
 * matrix pipe's float32-denormal arithmetic that SNNQP_DQ_TABLE rests on (same results). */
int snnqp_workqueue_stats(int64_t *captured_static, int64_t *busy_static,
                          int64_t *dequant_fallbacks, int reset);
/* test hook: writes `value` into word `word` of the capture slot that was handed out at `mark`
 * (synchronous) */
int snnqp_debug_workqueue_poke(int device, int64_t mark, int word, uint32_t value);

/* How the bit-input 3x3 MFMA kernels of snnqp_conv_lif_forward turn the integer accumulator
 * into the current fl(fl(acc / L) * m) for these weights and this neuron (host-side query, no
 * device work; < 0: error).  SNNQP_DQ_ARITH: three float32 instructions per value;
 * SNNQP_DQ_ONE: L == 1, one multiply; SNNQP_DQ_TABLE: codes within +-7, multi-step LIF / PLIF
 * with v_reset = 0 and abs_sum_max <= 2047 -- the accumulator's bit pattern is the address of
 * the current in an LDS table, no vector instruction (csrc/conv3x3_bits.hip).  All three give
 * the same bits.  No reference counterpart (diagnostic). */
#define SNNQP_DQ_ARITH 1
#define SNNQP_DQ_ONE 2
#define SNNQP_DQ_TABLE 3
int snnqp_conv_dequant_form(const snnqp_weight_t *w, const snnqp_neuron_t *nrn);

/* Smallest non-zero |BatchNorm_c(fl(fl(acc / L) * m))| over |acc| <= bound and the Cout
 * channels (bn nullable: identity), as float32 bits, atomically min-ed into *out_bits
 * (device word the caller initialises to 0x7F800000).  For snnqp_weight_t.min_current_bits:
 * once per (weights, BatchNorm) version. */
int snnqp_current_min(const snnqp_weight_t *w, const snnqp_bn_t *bn, int32_t bound,
                      int32_t Cout, uint32_t *out_bits, snnqp_stream_t stream);

/* Same for QuantDense: x [T][B][K], weights [K][N] (GENERIC) .
 * IMPL_MFMA additionally needs `wt`: the int8 codes tiled by
 * snnqp_pack_codes_mfma (Npad = N rounded up to 32; K rows zero-padded to a multiple
 * of 32 when K is not one), s_type BITS and either BITS input (zero bits beyond K),
 * T <= 96, or U8 input (any count 0..255, read in place: no packing pass, no inspection)
 * with w->col_sum, K % 16 == 0, K <= 65536, 16-byte aligned rows and T <= 64.  With
 * w->wt_fp6 and code_max <= 7, BITS rows run on the fp4 x fp6 MFMA instead (T <= 160, `wt` not
 * needed).  Longer runs and everything else: the direct-form kernel.  (More than 128 features
 * with T <= 64: a workgroup per 256 / 512-column block that reads every row once,
 * csrc/dense_wide.hip; else 128 columns per workgroup, csrc/dense_mfma.hip.) */
int snnqp_dense_lif_forward(const void *x, int in_type, int64_t x_stride_t,
                            int64_t x_stride_b, int32_t T, int32_t B, int32_t K,
                            int32_t N, const snnqp_weight_t *w,
                            const int8_t *wt, const snnqp_bn_t *bn,
                            const snnqp_neuron_t *nrn, const float *u0,
                            float *u_out, void *s_out, int s_type, int impl,
                            snnqp_stream_t stream);

/* The same with a workspace: the fp4 x fp6 kernel then may split K over several workgroups per
 * tile of rows (the read-out of config C3: 32768 -> 110 gives 256 workgroups of 80 rows too few
 * rows to amortise the 3 MB of codes each of them streams; two workgroups of 160 rows per tile
 * stream half each), handing partial sums over through `ws`.  ws: device memory, 256-byte
 * aligned, at least snnqp_dense_workspace_bytes(...) bytes, used by one launch at a time (its
 * content need not survive between launches: the call zeroes the tickets at its head on `stream`
 * in front of the kernel -- a kernel node when the stream is being captured -- so that nothing an
 * earlier launch, an aborted replay or a stray store left there can reach this one).
 * ws = NULL or too small: no split, as snnqp_dense_lif_forward.
 * snnqp_dense_workspace_bytes returns 0 when the split would not be used.
 * x_flags: float32 rows into integer codes (see snnqp_conv_lif_forward): the wide kernel (more
 * than 128 features, T <= 64, K % 16 == 0, rows 16-byte aligned, w->col_sum) stages them in place
 * and reports into the word; required then, ignored otherwise; other shapes refuse the
 * combination (SNNQP_EUNSUPPORTED: narrow the rows with snnqp_narrow_f32 first). */
int64_t snnqp_dense_workspace_bytes(int in_type, int32_t T, int32_t B, int32_t K, int32_t N,
                                    const snnqp_weight_t *w);
int snnqp_dense_lif_forward_ws(const void *x, int in_type, int64_t x_stride_t,
                               int64_t x_stride_b, int32_t T, int32_t B, int32_t K,
                               int32_t N, const snnqp_weight_t *w,
                               const int8_t *wt, const snnqp_bn_t *bn,
                               const snnqp_neuron_t *nrn, const float *u0,
                               float *u_out, void *s_out, int s_type, int impl,
                               int32_t *x_flags, void *ws, int64_t ws_bytes, snnqp_stream_t stream);
/* The launch snnqp_dense_lif_forward_ws makes on the fp4 x fp6 kernel for T steps, B samples, K
 * inputs and N features with this workspace (`ws` is looked at for its address only and never
 * dereferenced; NULL: none).  Launches nothing, makes no GPU call.  The answer is the launch's own
 * decision: the cost model, then the measurement knob SNNQP_DENSE_FP6_PLAN="rt,ks" (read when a
 * workspace is given; a value that is malformed, has rt * 32 < T, or splits more tiles than the
 * 4096-byte ticket head has words -- 1024 -- is ignored), then the workspace: a split plan that
 * needs more than ws_bytes, or a `ws` not 256-byte aligned, gives way to the best unsplit plan.
 *   rt   1..5 row tiles of 32 rows per workgroup: a workgroup owns floor(32 rt / T) samples
 *   ks   1, 2 or 4 workgroups per tile of rows along K
 *   gx   workgroups along the batch; the grid is gx x ceil(N / 128) x ks, tiles = gx ceil(N / 128)
 *   gcz  0 when unsplit; else the 512-deep pieces of K (two chunks of 256, one per wave group) that
 *        workgroup z of a tile walks from piece z * gcz on -- the last may get fewer, or none.
 * A split launch needs 4096 + tiles * ks * rt * 32 * 128 * 4 bytes of workspace.
 * SNNQP_EINVAL for sizes below 1 or a null pointer; SNNQP_EUNSUPPORTED for T > 160, as the launch. */
int snnqp_dense_fp6_plan(int32_t T, int32_t B, int32_t K, int32_t N, const void *ws, int64_t ws_bytes,
                         int32_t *rt, int32_t *ks, int32_t *gx, int32_t *gcz);
/* The launch snnqp_dense_lif_forward makes on the int8 128-column kernel (SNNQP_IMPL_MFMA, at most
 * 128 features or more than 64 timesteps) for rows of `in_type` (SNNQP_BITS or SNNQP_U8), T steps,
 * B samples and N features.  Launches nothing, makes no GPU call.  The answer is the launch's own
 * decision: the largest row tile that still gives 200 workgroups, else the smallest that holds a
 * sample, then the measurement knob SNNQP_DENSE_MFMA_RT=1..3 (read on every call; a value with
 * 32 rt < T, or above 2 for uint8 rows, is ignored).
 *   rt  1..3 row tiles of 32 rows per workgroup (uint8 rows: 1..2)
 *   sb  floor(32 rt / T) samples per workgroup
 *   gx  ceil(B / sb) workgroups along the batch      gy  ceil(N / 128) along the features
 * SNNQP_EINVAL for sizes below 1, another in_type or a null pointer; SNNQP_EUNSUPPORTED for T > 96
 * (uint8 rows: T > 64), as the launch. */
int snnqp_dense_mfma_plan(int in_type, int32_t T, int32_t B, int32_t N, int32_t *rt, int32_t *sb,
                          int32_t *gx, int32_t *gy);
/* the dense block on the direct-form kernel, executed only if *pred != 0 (snnqp_conv_lif_forward_if) */
int snnqp_dense_lif_forward_if(const int32_t *pred, const void *x, int in_type, int64_t x_stride_t,
                               int64_t x_stride_b, int32_t T, int32_t B, int32_t K, int32_t N,
                               const snnqp_weight_t *w, const snnqp_bn_t *bn,
                               const snnqp_neuron_t *nrn, const float *u0, float *u_out,
                               void *s_out, int s_type, snnqp_stream_t stream);

/* ---- the dense head as one launch -----------------------------------------------
 * replaces: the two dense SpikingBlocks and the vote that end CextNet,
 *           examples/tcja/models.py:200-255 --
 *             SpikingBlock(QuantDense(N1), neuron) -> SpikingBlock(QuantDense(N2), neuron)
 *             -> mean over T -> mean over each class's `group` neurons
 *           (per block spiking_learning.py:446-462 with flax_qdense.py:74-89; no norm_fn, no
 *           bias: models.py:200-208, 231-236), i.e. config C2 of BASELINE.json as a whole.
 * x     [T][B][K] by strides, SNNQP_U8 (any count 0..255, read in place; needs w1->col_sum,
 *       K % 16 == 0, 16-byte aligned rows), SNNQP_BITS (zero bits beyond K), or SNNQP_F32 -- the
 *       rows as the reference holds them (flax_qdense.py:67), read in place under the same
 *       conditions as uint8 rows: 4 x the bytes, checked on the way into LDS; x_flags as for
 *       snnqp_conv_lif_forward (required for SNNQP_F32; when the word comes back set, the caller's
 *       predicated launches -- snnqp_dense_lif_forward_if with the float32 kernel of the first
 *       block into s1_out, snnqp_dense_lif_forward_if of the second block, snnqp_vote_if -- redo
 *       the head).
 * w1/wt1  int8 codes [K][N1] and their tiles (snnqp_pack_codes_mfma, Npad = N1 rounded up to 32,
 *       K rows zero-padded to a multiple of 32); w2/wt2 the same for [N1][N2] (its K is N1).
 * logits  float32 [B][N2 / group], as snnqp_vote gives them.
 * s1_out / s2_out  nullable: the two spike rasters, SNNQP_BITS [T][B][ceil(N / 32)], as
 *       snnqp_dense_lif_forward writes them (the hidden raster otherwise never leaves the CU).
 * Membrane potentials start from zero (initialize_carry, spiking_learning.py:464-472) and are
 * not returned: a caller that carries state uses snnqp_dense_head_forward_state (below), or
 * snnqp_dense_lif_forward per block.
 * ws / ws_bytes  nullable workspace (device memory, 256-byte aligned, one launch at a time; its
 *       tickets are zeroed on `stream` by every call, as for snnqp_dense_lif_forward_ws;
 *       snnqp_dense_head_workspace_bytes says how much, 0 = it would not be used).  With it a batch that fills at most half the chip (config C2: B = 256) runs as two
 *       workgroups per tile of samples, each with half of the hidden columns -- half of the first
 *       block's codes through a CU's L1, the bound of the launch -- which hand their halves of the
 *       hidden raster over through `ws`; the last arriver runs the second block and the vote.
 * SNNQP_EUNSUPPORTED (nothing enqueued) unless N1 <= 512, N2 <= 128, 1 <= T <= 64 and both
 * weights are W_I8 with tiles: the caller then runs the blocks one by one. */
int64_t snnqp_dense_head_workspace_bytes(int32_t T, int32_t B, int32_t N1);
/* The form of the wide dense kernel for T steps, B samples and N features (N1 of the head).
 * Launches nothing.  fused != 0: snnqp_dense_head_forward, else the stand-alone wide block
 * (snnqp_dense_lif_forward with N > 128); may_split: a usable workspace is at hand.
 *   rt      1..4 row tiles of 32 rows per workgroup    ct  1 or 2 column tiles of 256 per workgroup
 *   sph     samples per lane half (a workgroup owns 2 sph samples)
 *   csplit  1: the head's hidden columns split over two workgroups per tile of samples (ct = 1)
 * SNNQP_EINVAL for sizes below 1 or a null pointer; SNNQP_EUNSUPPORTED for T > 64, or N > 512 fused. */
int snnqp_dense_wide_plan(int32_t T, int32_t B, int32_t N, int fused, int may_split, int32_t *rt,
                          int32_t *ct, int32_t *sph, int32_t *csplit);
int snnqp_dense_head_forward(const void *x, int in_type, int64_t x_stride_t,
                             int64_t x_stride_b, int32_t T, int32_t B, int32_t K,
                             int32_t N1, const snnqp_weight_t *w1, const int8_t *wt1,
                             const snnqp_neuron_t *nrn1, int32_t N2,
                             const snnqp_weight_t *w2, const int8_t *wt2,
                             const snnqp_neuron_t *nrn2, int32_t group,
                             uint32_t *s1_out, uint32_t *s2_out, float *logits,
                             int32_t *x_flags, void *ws, int64_t ws_bytes, snnqp_stream_t stream);
/* The same launch for a recording that arrives window by window (T = the window's steps):
 * u1 [B][N1], u2 [B][N2]  float32 membranes of the two blocks, read as the initial state and
 *       written as the final one, IN PLACE: each potential is loaded and stored by the one lane
 *       that owns its (sample, feature), the store behind the load.
 * counts [B][N2]  int32: the window's spike counts of the second block are added in (plain load,
 *       add, store by the owning lane; snnqp_vote_counts turns them into the running vote).
 * logits stays the vote over THIS window.  Same inputs, same refusals, same workspace rule as
 * snnqp_dense_head_forward; SNNQP_EINVAL for a null u1, u2 or counts.  The column split is served:
 * the two workgroups of a tile own disjoint columns of u1, and u2 / counts are touched by the last
 * arriver alone, so snnqp_dense_wide_plan and snnqp_dense_head_workspace_bytes answer for both
 * entries.  Float32 rows: the launch has updated u1 / u2 / counts by the time x_flags is known, so a
 * caller with a float32 stand-by hands this entry COPIES of the state and lets its predicated
 * launches read the originals (ops.dense_head_forward_state). */
int snnqp_dense_head_forward_state(const void *x, int in_type, int64_t x_stride_t,
                                   int64_t x_stride_b, int32_t T, int32_t B, int32_t K,
                                   int32_t N1, const snnqp_weight_t *w1, const int8_t *wt1,
                                   const snnqp_neuron_t *nrn1, int32_t N2,
                                   const snnqp_weight_t *w2, const int8_t *wt2,
                                   const snnqp_neuron_t *nrn2, int32_t group,
                                   float *u1, float *u2, int32_t *counts,
                                   uint32_t *s1_out, uint32_t *s2_out, float *logits,
                                   int32_t *x_flags, void *ws, int64_t ws_bytes, snnqp_stream_t stream);

/* ---- element-wise pieces ----------------------------------------------------
 * replaces: neural_dynamics(u, x) scanned over T, spiking_learning.py:460
 *           (multi_step_LIF :403-416, parametric_leaky_IF :370-387, LIF :426-438)
 *           with the optional norm_fn of :457-458 in front.
 * x float32 [T][R][C] currents; u0/u_out [R][C]; s_out [T][R][C] (F32/BITS). */
int snnqp_lif_forward(const float *x, int32_t T, int64_t R, int32_t C,
                      const snnqp_bn_t *bn, const snnqp_neuron_t *nrn,
                      const float *u0, float *u_out, void *s_out, int s_type,
                      snnqp_stream_t stream);

/* replaces: nn.BatchNorm(use_running_average=True), examples/tcja/models.py:101-107 */
int snnqp_batchnorm_forward(const float *x, int64_t rows, int32_t C,
                            const snnqp_bn_t *bn, float *y,
                            snnqp_stream_t stream);

/* replaces: lax.reduce_window(max, (1,1,2,2,1)), examples/tcja/models.py:145-147
 * x [NB][H][W][C] (F32 or BITS) -> y [NB][H/2][W/2][C]. */
int snnqp_maxpool2x2(const void *x, int type, int64_t NB, int32_t H, int32_t W,
                     int32_t C, void *y, snnqp_stream_t stream);

/* ---- TCJA attention pieces (examples/tcja/models.py:41-99) ---------------------
 * replaces: jnp.mean(x_seq, axis=[2, 3]) (:42): x [NB][HW][C] (F32 or BITS) ->
 *           y float32 [NB][C], sequential float32 sum over pixels / HW. */
int snnqp_spatial_mean(const void *x, int type, int64_t NB, int32_t HW, int32_t C,
                       float *y, snnqp_stream_t stream);
/* replaces: jax.nn.sigmoid(conv_c_out * conv_t_out) (:95): g = sigmoid(a * b),
 *           float32 product, logistic in float64 rounded once. */
int snnqp_sigmoid_gate(const float *a, const float *b, int64_t n, float *g,
                       snnqp_stream_t stream);
/* replaces: x_seq * out[:, :, None, None, :] (:97): y[img][p][c] = x * g[img][c]. */
int snnqp_apply_gate(const void *x, int type, const float *g, int64_t NB, int32_t HW,
                     int32_t C, float *y, snnqp_stream_t stream);

/* ---- event front end and probes ------------------------------------------------
 * replaces: preprocess_data_number, examples/input_pipeline.py:142-219
 *           (split_by = "number"): N time-ordered events (x, y, polarity) ->
 *           T frames of N // T events (the last takes the remainder), counts per
 *           pixel and polarity (channel 0 = polarity 0).  counts int32
 *           [T][H][W][2] (zeroed here); frames_u8 optional saturated copy.
 *           Coordinates are divided by `scale` (config.resolution_scale). */
int snnqp_events_to_frames(const int32_t *ex, const int32_t *ey, const int32_t *ep,
                           int64_t N, int32_t T, int32_t H, int32_t W, float scale,
                           int32_t *counts, uint8_t *frames_u8, snnqp_stream_t stream);
/* replaces: preprocess_data_number (examples/input_pipeline.py:142-219) and preprocess_data_time
 *           (:63-131) over a whole batch, in one launch and without an intermediate: B rows of
 *           ragged event streams that live on the device -> [B][T] frames of H x W x 2 counts,
 *           written in the format the event layer reads.  (The division by time_step *
 *           input_scale of :137 is the caller's.)
 * mode 0 "number", mode 1 "time".
 * addr    one word per event: x in bits 0..13, y in bits 14..27, polarity (0 / non-zero) in bit 28;
 *         read only inside a sample's range, so it may be null when no sample has an event
 * times   int32 microseconds, one per event; mode 1 only (nullable in mode 0); non-decreasing
 *         within every sample
 * offsets int64 [S + 1]: sample s owns events offsets[s] .. offsets[s + 1] - 1
 * sample  int32 [B]: which sample each batch row decodes (any order, repeats allowed); a value
 *         outside [0, S) yields zero frames for that row
 * start   int32 [B]: window origin per row, mode 1 only
 * out     [B][T] frames of H x W x 2, as out_type SNNQP_U8 / SNNQP_EV4 / SNNQP_EV1 lays a frame out;
 *         every byte / word is written, empty frames included (the caller zeroes nothing)
 * flags   nullable device word, OR-ed with SNNQP_FLAG_GT_15 / SNNQP_FLAG_GT_ONE as snnqp_pack_frames does
 * H, W are the output size: x' = floor(float(x) / scale), the same for y, and an event outside
 * [0, W) x [0, H) is dropped.  Number mode: with n events in the sample and di = n / T, frame f takes
 * events [f * di, (f + 1) * di) and the last frame the rest (n < T: all of them).  Time mode: frame f
 * takes the events with start + f * step_us < t < start + (f + 1) * step_us, both ends strict (an
 * event on a window edge is in no frame), compared in 64 bits; with unsorted times the counts are
 * unspecified but every access stays inside the sample.  Counts are exact before they saturate:
 * SNNQP_U8 at 255 silently, SNNQP_EV4 at 15 and SNNQP_EV1 at 1 with the flag.
 * SNNQP_EINVAL, checked on the host before anything is launched: bad shapes (H, W in 1 .. 16384),
 * an unknown mode or out_type, scale <= 0, and in mode 1 step_us <= 0 or a null times / start.
 * B == 0 or T == 0 returns SNNQP_OK without a launch. */
int snnqp_events_bin(const uint32_t *addr, const int32_t *times, const int64_t *offsets, int32_t S,
                     const int32_t *sample, const int32_t *start, int32_t B, int mode, int32_t T,
                     int32_t step_us, int32_t H, int32_t W, float scale,
                     void *out, int out_type, int32_t *flags, snnqp_stream_t stream);
/* One row's event augmentation for snnqp_events_bin_aug: 48 bytes, a device array of B records. */
typedef struct snnqp_event_aug {
  uint32_t flags;                              /* bit 0 flip x, bit 1 flip y, bit 2 swap polarity; other bits 0 */
  int32_t dx, dy;                              /* |dx|, |dy| <= 16384 */
  int32_t cut_x0, cut_y0, cut_x1, cut_y1;      /* half-open, frame pixels */
  int32_t f0, f1;                              /* frames [f0, f1) come out empty */
  uint32_t drop_below, seed, reserved;         /* reserved = 0 */
} snnqp_event_aug_t;
/* replaces: nothing in the reference (it trains on the recordings as they are); the usual event
 *           augmentations -- flips, translation, cutout, EventDrop's random / area / time drops,
 *           polarity swap -- as per-event decisions inside snnqp_events_bin's launch.
 * Arguments, checks (SNNQP_EINVAL, on the host, before anything is launched), formats and flags are
 * snnqp_events_bin's; aug == NULL is exactly snnqp_events_bin.
 * aug     [B] records on the device, 4-byte aligned; row b is decoded under aug[b]
 * A frame f of row b with f0 <= f < f1 is all zero.  Every other frame takes the slice
 * snnqp_events_bin gives it -- that of the untouched sample: number mode cuts equal counts over all
 * its events, time mode searches the same times -- and passes each event through, in this order:
 *   1. x' = floor(float(x) / scale), the same for y; outside [0, W) x [0, H): dropped
 *   2. flip:   x = W - 1 - x (bit 0), y = H - 1 - y (bit 1)
 *   3. shift:  x += dx, y += dy; outside the frame: dropped (zero fill, no wrap-around)
 *   4. cutout: dropped if cut_x0 <= x < cut_x1 and cut_y0 <= y < cut_y1 (final frame pixels; empty
 *      when cut_x1 <= cut_x0 or cut_y1 <= cut_y0)
 *   5. drop:   dropped if fmix32(fmix32(seed) ^ (uint32_t)i) < drop_below (0: nothing is dropped;
 *      2^32 - 1: all but the events whose hash is 2^32 - 1), i the event's index within its sample
 *      (0 for the sample's first event), low 32 bits, and fmix32 the murmur3 finaliser in 32-bit
 *      unsigned arithmetic:  h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 *   6. swap:   with bit 2 an event of polarity 0 counts in channel 1 and the reverse
 *   7. counted as snnqp_events_bin counts it: exact before it saturates, the same flags.
 * Integer adds commute: two launches give the same bytes.
 * The records live on the device, so nothing in them is checked.  Out of range they do this and no
 * more: the shift is added modulo 2^32, so |dx| >= W or |dy| >= H drops every event of the row;
 * the rectangle and [f0, f1) are compared as signed 32-bit values, whatever they hold; bits 3..31
 * of flags and `reserved` are ignored.  Whatever the records hold, the launch reads aug[0 .. B - 1]
 * and the events snnqp_events_bin would read, and writes `out` and `flags` only. */
int snnqp_events_bin_aug(const uint32_t *addr, const int32_t *times, const int64_t *offsets, int32_t S,
                         const int32_t *sample, const int32_t *start, int32_t B, int mode, int32_t T,
                         int32_t step_us, int32_t H, int32_t W, float scale, const snnqp_event_aug_t *aug,
                         void *out, int out_type, int32_t *flags, snnqp_stream_t stream);
/* replaces: nothing in the reference; mixing two recordings (EventMix, the CutMix branch of NDA):
 *           a box of row b's space-time volume is taken from a partner sample, inside
 *           snnqp_events_bin_aug's launch, and the events of either that survive are counted.
 * Arguments, checks, formats and flags are snnqp_events_bin_aug's (aug may be null: the identity), and
 * sample2  int32 [B], nullable: the partner sample of each row; a value outside [0, S), or a null
 *          array, leaves the row unmixed: the bytes of snnqp_events_bin_aug and counts[b][1] += 0
 * start2   int32 [B]: the partner's window origin, mode 1 only
 * aug2     [B] records, 4-byte aligned, nullable (the identity): row b's partner is decoded under aug2[b]
 * box      int32 [B][6]: x0, y0, x1, y1, g0, g1 -- final frame pixels and frames, half-open, compared
 *          as signed 32-bit values, whatever they hold; empty when x1 <= x0, y1 <= y0 or g1 <= g0
 * counts   int64 [B][2], 8-byte aligned, nullable, zeroed by the caller: counts[b][0] += the events
 *          of sample[b], counts[b][1] += the events of sample2[b] that reached the count of rule 7
 *          (before any saturation), over all frames of row b
 * Frame f of a mixed row b is the sum of two slices, each that of its own untouched sample (number
 * mode cuts each sample's own equal counts; time mode searches from start[b] and start2[b]):
 *   - sample[b]'s slice of frame f: every event passes rules 1-6 of aug[b] and is then dropped if
 *     x0 <= x < x1 and y0 <= y < y1 and g0 <= f < g1;
 *   - sample2[b]'s slice of frame f, read only when g0 <= f < g1 and aug2[b] does not empty f: every
 *     event passes rules 1-6 of aug2[b] (rule 5 hashes its index within sample2[b]) and is then
 *     dropped unless x0 <= x < x1 and y0 <= y < y1.
 *   7. counted as snnqp_events_bin counts it: the sum is exact before it saturates, the same flags.
 * Integer adds commute: two launches give the same bytes and the same counts.
 * SNNQP_EINVAL, on the host, before anything is launched: snnqp_events_bin's refusals, sample2 with a
 * null box, and in mode 1 sample2 with a null start2.  B == 0 or T == 0 returns SNNQP_OK without a
 * launch.  Whatever the records and boxes hold, the launch reads them, sample2, start2 and the events
 * of the two samples' slices, and writes `out`, `flags` and `counts` only. */
int snnqp_events_bin_mix(const uint32_t *addr, const int32_t *times, const int64_t *offsets, int32_t S,
                         const int32_t *sample, const int32_t *start, const snnqp_event_aug_t *aug,
                         const int32_t *sample2, const int32_t *start2, const snnqp_event_aug_t *aug2,
                         const int32_t *box, int64_t *counts, int32_t B, int mode, int32_t T, int32_t step_us,
                         int32_t H, int32_t W, float scale, void *out, int out_type, int32_t *flags,
                         snnqp_stream_t stream);
/* replaces: the `mnist` branch of examples/input_pipeline.py:286-296 (static images, Poisson-
 *           encoded into num_frames count frames) over a whole batch, in one launch: B rows of a
 *           device-resident uint8 image set -> [B][T][K] counts or spikes.
 * images    uint8 [S][K]
 * sample    int32 [B]: which row of `images` each batch row encodes (any order, repeats allowed); a
 *           value outside [0, S) encodes as an image of zeros
 * sample_id uint32 [B]: the id of each row in the key below -- the sample's index in the whole
 *           source, not in the slice that happens to be resident
 * table     uint32 [256][16], 4-byte aligned: the thresholds of each pixel value.  An entry of
 *           2^32 - 1 stands for 2^32: no hash reaches it
 * kind      SNNQP_ENCODE_BERNOULLI or SNNQP_ENCODE_POISSON
 * out       element (b, t, k) at os_b * b + os_t * t + k, out_type SNNQP_U8: bytes, strides in
 *           bytes; SNNQP_BITS (Bernoulli only): int32 words, element k in bit (k & 31) of word
 *           (k >> 5), the unused high bits of a row's last word 0, strides in words, 4-byte
 *           aligned.  os_b = T * row, os_t = row is batch-major [B][T][K]; os_b = row, os_t = B * row
 *           time-major [T][B][K] (row = K bytes or (K + 31) / 32 words).  Every element of every
 *           (b, t) row is written and nothing else; the strides are the caller's to get right.
 * For row b, step t and element k, in 32-bit unsigned arithmetic (fmix32: snnqp_events_bin_aug):
 *   e = t * K + k
 *   c = fmix32(fmix32(seed ^ fmix32(draw)) ^ sample_id[b])
 *   u = fmix32(c ^ e)
 *   v = images[sample[b]][k]
 *   Bernoulli: 1 iff u < table[v][0], else 0
 *   Poisson:   the number of j in 0..14 with u >= table[v][j] (0..15; entry 15 is unused
 *              padding and must be 0)
 * The value at (sample_id, t, k) depends on nothing else: not on B, the row's place in the batch,
 * the strides or out_type.  Two launches give the same bytes.
 * SNNQP_EINVAL, checked on the host before anything is launched: T * K >= 2^32, K < 1, negative
 * S, B or T, an unknown kind or out_type, Poisson with SNNQP_BITS, and -- with B * T > 0 -- a null
 * or misaligned pointer.  B == 0 or T == 0 returns SNNQP_OK without a launch. */
#define SNNQP_ENCODE_BERNOULLI 0
#define SNNQP_ENCODE_POISSON 1
int snnqp_rate_encode(const uint8_t *images, int32_t S, const int32_t *sample, const uint32_t *sample_id,
                      int32_t B, int32_t T, int32_t K, uint32_t seed, uint32_t draw, const uint32_t *table,
                      int kind, void *out, int out_type, int64_t os_b, int64_t os_t, snnqp_stream_t stream);
/* replaces: the activation-density probes sown at examples/tcja/models.py:128-142
 *           (consumed by examples/sparsity.py:143-170): non-zero count of each of
 *           NB slices of n elements (C innermost; F32, U8 or BITS). */
int snnqp_density(const void *x, int type, int64_t NB, int64_t n, int32_t C, int32_t *nnz,
                  snnqp_stream_t stream);

/* replaces: the rate "vote", examples/tcja/models.py:253-255
 * s [T][B][N] (F32 or BITS) -> logits float32 [B][N / group]:
 * mean over T (sequential float32 sum / T), then mean over `group` neurons. */
int snnqp_vote(const void *s, int type, int32_t T, int32_t B, int32_t N,
               int32_t group, float *logits, snnqp_stream_t stream);
/* executed only if *pred != 0 (snnqp_conv_lif_forward_if) */
int snnqp_vote_if(const int32_t *pred, const void *s, int type, int32_t T, int32_t B, int32_t N,
                  int32_t group, float *logits, snnqp_stream_t stream);
/* The vote of a raster that arrives window by window, kept as integer counts.
 * snnqp_vote_accumulate: s [T][B][N] (F32 holding 0 / 1, or BITS; any N) -- each neuron's spike
 *   count over the T steps is added into counts int32 [B][N] (one owner per (b, n), plain loads and
 *   stores; T = 0 adds nothing).
 * snnqp_vote_counts: counts [B][N] -> logits float32 [B][N / group] = snnqp_vote of the raster the
 *   counts were taken from: (float)count / (float)steps, then the in-order mean over `group`
 *   (exact while steps < 2^24).  steps_b int32 [B] on the device gives every row its own number of
 *   steps (`steps` is then ignored); null: all rows share `steps`.  A row with 0 steps votes 0. */
int snnqp_vote_accumulate(const void *s, int type, int32_t T, int32_t B, int32_t N, int32_t *counts,
                          snnqp_stream_t stream);
int snnqp_vote_counts(const int32_t *counts, int32_t steps, const int32_t *steps_b, int32_t B, int32_t N,
                      int32_t group, float *logits, snnqp_stream_t stream);

/* replaces: nothing in the reference (it computes every output channel); the blocks of a model
 * whose pruned channels cannot fire compute the others only, and this restores the
 * full raster where one is sown: bit-packed s [npix][ceil(cin/32)] -> out [npix][ceil(cout/32)],
 * input channel c to output channel map[c] (int32 [cin]; entries outside [0, cout) are dropped),
 * every other channel zero. */
int snnqp_scatter_spike_channels(const uint32_t *s, int64_t npix, int32_t cin, const int32_t *map,
                                 int32_t cout, uint32_t *out, snnqp_stream_t stream);

/* ---- training of the dense blocks (csrc/train_dense.hip) ------------------------------------
 * The surrogate-gradient backward of SpikingBlock(QuantDense, multi_step_LIF) as jax.grad
 * differentiates examples/tcja/models.py:191-255.  All tensors float32, time-major.
 *
 * replaces: the scan of spiking_learning.py:403-416 in train mode, keeping its residual:
 *           x [T][R][C] currents, zero initial state -> h_out [T][R][C] the potential before
 *           the reset (u + (x - (u - v_reset)) / tau), s_out [T][R][C] spikes 0.0 / 1.0 -- the
 *           same arithmetic as snnqp_lif_forward.  multi_step_LIF only (else SNNQP_EUNSUPPORTED). */
int snnqp_lif_forward_save(const float *x, int32_t T, int64_t R, int32_t C,
                           const snnqp_neuron_t *nrn, float *h_out, float *s_out,
                           snnqp_stream_t stream);
/* the backward of that scan, t = T-1 .. 0, with gu_T = 0 and no gradient through the reset:
 *   gh_t = gs_t sigma'(h_t - v_th) + gu_t (1 - s_t),  gI_t = gh_t / tau,  gu_{t-1} = gh_t (1 - 1/tau)
 * sigma' = SNNQP_SURR_*.  Upstream either gs [T][R][C] or, with the vote of
 * examples/tcja/models.py:253-255 fused, glogits [R][C / group]: gs_t[r][c] = glogits[r][c / group]
 * / (group T) (exactly one of the two is non-null).  gI [T][R][C]. */
int snnqp_lif_backward(const float *h, const float *gs, const float *glogits, int32_t group,
                       int32_t T, int64_t R, int32_t C, const snnqp_neuron_t *nrn,
                       int surrogate, float *gI, snnqp_stream_t stream);
/* The two scans over one window of a recording (truncated BPTT): the arithmetic
 * of the two entries above, step for step, from and to a carried membrane.
 *   u0     float32 [R][C], nullable (zeros): the membrane the window starts from
 *   u_out  float32 [R][C], nullable: receives u_T = s_{T-1} ? v_reset : h_{T-1}; may be u0's buffer
 *          (one lane owns one element).  T == 0 writes u_out = u0 and nothing else.
 *   gu_T   float32 [R][C], nullable (zeros): the gradient arriving at u_T; it enters step T-1 as
 *          gu_t (1 - s_t) does for every other step (no gradient through the reset condition)
 *   gu0    float32 [R][C], nullable: receives the recurrence's last gu, gh_0 (1 - 1/tau) = dL/du0;
 *          T == 0 writes gu0 = gu_T
 * With glogits, T in glogits / (group T) is the window's own length: a window's logits are the
 * vote over that window. */
int snnqp_lif_forward_save_state(const float *x, int32_t T, int64_t R, int32_t C,
                                 const snnqp_neuron_t *nrn, const float *u0, float *u_out,
                                 float *h_out, float *s_out, snnqp_stream_t stream);
int snnqp_lif_backward_state(const float *h, const float *gs, const float *glogits, int32_t group,
                             int32_t T, int64_t R, int32_t C, const snnqp_neuron_t *nrn,
                             int surrogate, const float *gu_T, float *gI, float *gu0,
                             snnqp_stream_t stream);
/* gw [K][N] = sum_m x[m][k] gI[m][n] over x [M][K], gI [M][N], m ascending (exact f32 MFMA,
 * one fixed order: bitwise reproducible). */
int snnqp_dense_weight_grad(const float *x, const float *gI, int64_t M, int32_t K, int32_t N,
                            float *gw, snnqp_stream_t stream);
/* gx [M][K] = (sum_n gI[m][n] w[k][n]) * mask[m][k] over gI [M][N], w [K][N]; mask [M][K]
 * optional (the dropout mask of the block's input). */
int snnqp_dense_input_grad(const float *gI, const float *w, const float *mask, int64_t M,
                           int32_t K, int32_t N, float *gx, snnqp_stream_t stream);

/* ---- training of the neurons with parameters (csrc/train_neuron.hip) -------------------------
 * parametric_leaky_IF (k = m = sigmoid(tau), one scalar) and LIF (decay[c] = sigmoid(tau[c])),
 * spiking_learning.py:357-387 and :419-438.  multi_step_LIF has no parameter: its scans are the
 * two entry points above, and these answer SNNQP_EUNSUPPORTED for it, naming them.  LIF without
 * `decay` is SNNQP_EINVAL.  All tensors float32, time-major; 64-bit index arithmetic; grids beyond
 * the launch limits are SNNQP_EINVAL; every refusal is decided on the host before any launch.
 *
 * replaces: the scan in train mode, keeping its residual: x [T][R][C] currents, zero initial
 *           state -> h_out the potential before the reset, s_out the spikes 0.0 / 1.0 -- the
 *           arithmetic of snnqp_lif_forward for the same neuron, bit for bit:
 *             PLIF  h = u + fl(fl(x - fl(u - v_reset)) m)      LIF  h = fl(fl(u decay[c]) + x) */
int snnqp_neuron_forward_save(const float *x, int32_t T, int64_t R, int32_t C,
                              const snnqp_neuron_t *nrn, float *h_out, float *s_out,
                              snnqp_stream_t stream);
/* the backward of that scan, t = T-1 .. 0, gu_T = 0, no gradient through the reset condition:
 *   gh_t = g_t sigma'(h_t - v_th) + gu_t (1 - s_t),  u_{t-1} = s_{t-1} ? v_reset : h_{t-1},  u_{-1} = 0
 *   PLIF  gI_t = gh_t m,  gu_{t-1} = gh_t fl(1 - m),   gparam[0] = sum_{t,r,c} gh_t d_t,
 *         d_t = fl(x_t - fl(u_{t-1} - v_reset)) recomputed from x (the tensor the scan consumed)
 *   LIF   gI_t = gh_t,    gu_{t-1} = gh_t decay[c],    gparam[c] = sum_{t,r} gh_t u_{t-1};  x unused
 * Upstream gs [T][R][C] or glogits [R][C / group] (the fused vote), exactly one, as
 * snnqp_lif_backward.  gparam is float64, [1] for PLIF and [C] for LIF: every product is formed in
 * float64 from its two float32 factors (exact) and added in float64 in a fixed order -- the rows
 * are cut into `splits` (1..max(R, 1)) contiguous ranges whose lengths differ by at most one, a
 * range is walked r ascending and t descending within a row, the ranges of a feature are added in
 * order (more than 32 of them: in groups of 32 consecutive ranges, then the groups in order) and,
 * for PLIF, the features in order.  No atomics: bitwise reproducible for a given
 * `splits`.  `workspace` holds the partials (snnqp_neuron_backward_workspace_bytes).  T == 0 or
 * R == 0 writes zero sums and launches nothing. */
int snnqp_neuron_backward(const float *h, const float *x, const float *gs, const float *glogits,
                          int32_t group, int32_t T, int64_t R, int32_t C,
                          const snnqp_neuron_t *nrn, int surrogate, int32_t splits, float *gI,
                          double *gparam, void *workspace, int64_t workspace_bytes,
                          snnqp_stream_t stream);
/* The PLIF / LIF scans over one window of a recording: u0, u_out, gu_T and gu0 as in
 * snnqp_lif_forward_save_state / snnqp_lif_backward_state (gu0 = gh_0 fl(1 - m) for PLIF,
 * gh_0 decay[c] for LIF).  The backward reads u0 (nullable: zeros) as u_{-1} in the t = 0 term of
 * both sums: d_0 = fl(x_0 - fl(u0 - v_reset)) for PLIF, gh_0 u0 for LIF.  The range split, the
 * float64 partials, the reduction order and the workspace are snnqp_neuron_backward's.  T == 0 or
 * R == 0 writes zero sums, gu0 = gu_T, and launches no kernel. */
int snnqp_neuron_forward_save_state(const float *x, int32_t T, int64_t R, int32_t C,
                                    const snnqp_neuron_t *nrn, const float *u0, float *u_out,
                                    float *h_out, float *s_out, snnqp_stream_t stream);
int snnqp_neuron_backward_state(const float *h, const float *x, const float *u0, const float *gs,
                                const float *glogits, int32_t group, int32_t T, int64_t R,
                                int32_t C, const snnqp_neuron_t *nrn, int surrogate, int32_t splits,
                                const float *gu_T, float *gI, float *gu0, double *gparam,
                                void *workspace, int64_t workspace_bytes, snnqp_stream_t stream);
/* Host only.  The default `splits`: min(max(R, 1), ceil(LANES / C)) -- a function of the shapes
 * alone (the device is not asked); LANES is a constant of the build, DESIGN.md 17.  A negative
 * SNNQP_E* on a bad shape. */
int snnqp_neuron_backward_splits(int32_t T, int64_t R, int32_t C);
/* Host only.  Bytes of `workspace` for `splits` ranges and neuron `kind` (SNNQP_NEURON_*), or a
 * negative SNNQP_E*. */
int64_t snnqp_neuron_backward_workspace_bytes(int32_t T, int64_t R, int32_t C, int32_t splits,
                                              int kind);

/* ---- training of the conv blocks (csrc/train_conv.hip) ---------------------------------------
 * The two gradient products of a 2-D convolution (flax_qconv.py:158-168 differentiated) and the
 * pool's gradient routing.  All tensors float32: x [NB][H][W][Cin], gI [NB][OH][OW][Cout], w and
 * gw HWIO [KH][KW][Cin][Cout].  Geometry served: groups == 1, every dilation 1, non-negative
 * explicit padding, any kernel size and stride; anything else is SNNQP_EUNSUPPORTED, decided on
 * the host before any launch.  Each product is the r-ascending fmaf chain from +0 (the contract
 * of snnqp_dense_weight_grad) over the explicitly gathered matrices, a tap outside the image
 * reading as the literal 0.0.  Index arithmetic is 64-bit; grids beyond the launch limits are
 * SNNQP_EINVAL.
 *
 * gw[(kh KW + kw) Cin + ci][co] = sum_r x[n, oh sh + kh - pt, ow sw + kw - pl, ci] gI[r][co],
 * r = (n OH + oh) OW + ow ascending over Rn = NB OH OW rows.  r is cut into `splits` (1..64)
 * contiguous ranges of L = 16 ceil(ceil(Rn / 16) / splits) rows (trailing ranges may be empty),
 * each its own chain from +0 into workspace[s] ([KH KW Cin][Cout] each); a second kernel forms
 * ((p0 + p1) + p2) + ... in float32 in s order.  No atomics: bitwise reproducible for a given
 * `splits`.  With splits == 1 gw is written directly and `workspace` is not read (may be null).
 * NB == 0 writes zeros to gw and touches nothing else. */
int snnqp_conv_weight_grad(const float *x, const float *gI, int64_t NB,
                           const snnqp_conv_geom_t *g, int32_t splits, float *workspace,
                           float *gw, snnqp_stream_t stream);
/* Host only.  Bytes of `workspace` for `splits` ranges (0 for one), or a negative SNNQP_E*. */
int64_t snnqp_conv_weight_grad_workspace_bytes(const snnqp_conv_geom_t *g, int32_t splits);
/* Host only.  The default `splits` for NB images: a function of the shapes alone (the device is
 * not asked, so a gradient does not depend on the machine), in 1..64: tiles x splits near 1024
 * workgroups, no range shorter than 256 rows.  A negative SNNQP_E* on a geometry not served. */
int snnqp_conv_grad_splits(const snnqp_conv_geom_t *g, int64_t NB);
/* snnqp_conv_weight_grad's sum with the chain in float64, for a layer whose gradient cancels too
 * far for a float32 chain (CextNet's first block: the most rows, count frames with a large mean
 * against a gI that sums to zero).  Same tensors and geometry.  r is cut into
 * S = min(1024, max(1, ceil(Rn / 1024))) contiguous ranges of ceil(Rn / S) rows; each range is the
 * r-ascending chain acc = acc + (double)x (double)gI from +0 (the product is exact, the addition
 * rounds once) into workspace[s] ([KH KW Cin][Cout] doubles); a second kernel forms
 * ((p0 + p1) + p2) + ... in float64 in s order and rounds to float32 once.  No atomics: bitwise
 * reproducible.  `workspace` holds snnqp_conv_weight_grad_f64_workspace_bytes(g, NB) bytes (host
 * only; a negative SNNQP_E* on a geometry not served).  NB == 0 writes zeros to gw.  One lane per
 * element of gw: meant for a small KH KW Cin. */
int snnqp_conv_weight_grad_f64(const float *x, const float *gI, int64_t NB,
                               const snnqp_conv_geom_t *g, double *workspace, float *gw,
                               snnqp_stream_t stream);
int64_t snnqp_conv_weight_grad_f64_workspace_bytes(const snnqp_conv_geom_t *g, int64_t NB);
/* gx[n, ih, iw, ci] = sum_r gI[n, oh, ow, co] w[kh, kw, ci, co], r = (kh KW + kw) Cout + co
 * ascending, oh = (ih + pt - kh) / sh and likewise ow; the tap reads 0.0 where that is not an
 * integer in range. */
int snnqp_conv_input_grad(const float *gI, const float *w, int64_t NB,
                          const snnqp_conv_geom_t *g, float *gx, snnqp_stream_t stream);
/* The gradient of snnqp_maxpool2x2 on float32 s [NB][H][W][C]: each gp [NB][H/2][W/2][C] element
 * goes to the first position, in row-major window order, that holds the window's maximum; every
 * other position, and a trailing odd row or column, gets 0.  gs [NB][H][W][C]. */
int snnqp_maxpool2x2_backward(const float *s, const float *gp, int64_t NB, int32_t H, int32_t W,
                              int32_t C, float *gs, snnqp_stream_t stream);

/* ---- training of a conv block with rematerialisation (csrc/train_remat.hip) ------------------
 * What a block that keeps neither its currents nor h runs chunk by chunk.  All
 * tensors float32; one lane per element e = r C + c; 64-bit index arithmetic; grids beyond the
 * launch limits are SNNQP_EINVAL; every refusal is decided on the host before any launch.
 *
 * The batch-statistics normalisation and snnqp_lif_forward_save_state in one pass:
 *   y_t = fl(fl(fl(cur_t - mean[t][c]) mul[t][c]) + bias[c]), then that entry's step on y_t.
 *   cur    [T][R][C] the raw currents;  mean, mul [T][C] the per-step mean and the multiplier
 *          fl(fl(1 / sqrt(fl(var + eps))) scale) (computed by the caller);  bias [C]
 *   u0, u_out  as snnqp_lif_forward_save_state's (u0 null: zeros; may be one buffer)
 *   h_out, s_out [T][R][C], each nullable: what is not wanted is not written
 * y is never written.  T == 0 writes u_out = u0 and nothing else.  Null cur, mean, mul or bias
 * with T R C > 0 is SNNQP_EINVAL.  multi_step_LIF only: a neuron with a parameter is
 * SNNQP_EUNSUPPORTED, naming snnqp_neuron_forward_save_state, the scan that serves it. */
int snnqp_bn_lif_forward_state(const float *cur, const float *mean, const float *mul,
                               const float *bias, int32_t T, int64_t R, int32_t C,
                               const snnqp_neuron_t *nrn, const float *u0, float *u_out,
                               float *h_out, float *s_out, snnqp_stream_t stream);
/* snnqp_maxpool2x2_backward with the pool's input taken as s = ((h - vth) >= 0) ? 1 : 0, the
 * forward's own compare on h [NB][H][W][C]: the same rule (first maximum in row-major window
 * order, zeros in a trailing odd row or column), and no spike raster in memory. */
int snnqp_maxpool2x2_backward_h(const float *h, float vth, const float *gp, int64_t NB, int32_t H,
                                int32_t W, int32_t C, float *gs, snnqp_stream_t stream);

/* ---- training of CextNet's gated stages (csrc/train_gate.hip) --------------------------------
 * The backward of p = maxpool2x2(y), y[n, h, w, c] = x[n, h, w, c] gate[n, c], with the spatial
 * mean m = snnqp_spatial_mean(x) the gate is a function of (examples/tcja/models.py:41-99,
 * :184-187).  All tensors float32: x, gx [NB][H][W][C] (general values, not only 0 / 1), gate,
 * ggate, gm [NB][C], gp [NB][H/2][W/2][C].  p*(window) is the first position, in the row-major
 * window order (0,0), (0,1), (1,0), (1,1), at which y_i = fl(x_i gate) attains the window's
 * maximum, by the compare rule of snnqp_maxpool2x2_backward applied to y (a later position wins
 * only when strictly greater; with gate == 0 every y_i is equal and the first position wins).
 * Index arithmetic is 64-bit, every access is predicated; H, W, C > 0; a grid beyond the launch
 * limits is SNNQP_EINVAL; shapes and null pointers are refused on the host before any launch.
 * NB == 0 returns SNNQP_OK and writes nothing (no pointer is looked at).
 *
 * ggate[n, c] = sum over windows of gp[n, ph, pw, c] x[n, p*, c]: one fmaf chain from +0,
 * acc = fmaf(gp, x, acc), over (ph, pw) ascending, ph the slow index -- never cut into ranges, so
 * the order is a function of (H, W) alone.  No atomics: bitwise reproducible.  With H < 2 or
 * W < 2 there is no window: ggate = +0 and gp is not read (may be null). */
int snnqp_gate_pool_grad_gate(const float *x, const float *gate, const float *gp, int64_t NB,
                              int32_t H, int32_t W, int32_t C, float *ggate,
                              snnqp_stream_t stream);
/* gx[n, h, w, c] = fl(route + fl(gm[n, c] / (float)(H W))): route = fl(gp[n, h/2, w/2, c]
 * gate[n, c]) where (h, w) is p* of its window and +0 elsewhere (a trailing odd row or column
 * belongs to no window); the second term is the VJP of snnqp_spatial_mean, which divides its
 * sum by (float)(H W) -- the same division, not a multiplication by a reciprocal. */
int snnqp_gate_pool_grad_input(const float *x, const float *gate, const float *gp, const float *gm,
                               int64_t NB, int32_t H, int32_t W, int32_t C, float *gx,
                               snnqp_stream_t stream);

/* ---- magnitude pruning on the device (csrc/prune.hip) ------------------------------------------
 * replaces: the mask selection of update_prune_mask / the global masks,
 *           examples/train_inpt_spikingjelly.py:147-157, :174-223, when it runs inside the training
 *           loop (a prune event) instead of once on the host.
 * w, mask float32 [n], 0 <= k <= n.  An entry is already pruned iff mask[i] == 0 (either zero);
 * m = their number.  k <= m: nothing is written.  Otherwise the k - m unpruned entries that are
 * smallest by the key bits(|w[i]|) read as uint32 (-0 equals +0, denormals in order, Inf above
 * every finite value, NaN above Inf), ties on the key by ascending index, get mask[i] = +0.0f; no
 * other word of `mask` is written, whatever value it holds.  Only integer compares and counts
 * decide: the result is a function of (w, mask, k), bitwise the same on every launch.
 * One stream, no host read, no synchronisation: m is counted and k <= m decided on the device.  A
 * three-pass radix select (11 / 11 / 10 bits of the key, LDS histograms flushed with integer
 * atomics into `workspace`) finds the cut; a last pass in which every workgroup owns a contiguous
 * index range writes the zeros.  `workspace`: snnqp_magnitude_prune_workspace_bytes(n) bytes,
 * 4-byte aligned, zeroed by the call on `stream`; its contents afterwards mean nothing.
 * Refused on the host before any launch (SNNQP_EINVAL): n < 0; k < 0 or k > n; n >= 2^32 (the
 * counters are 32-bit); a null or misaligned w, mask or workspace with n > 0; workspace_bytes below
 * the query's answer.  n == 0 returns SNNQP_OK and looks at no pointer.  The grid is a function of n
 * alone, at most 1024 workgroups: it never passes a launch limit. */
int snnqp_magnitude_prune(const float *w, float *mask, int64_t n, int64_t k, void *workspace,
                          int64_t workspace_bytes, snnqp_stream_t stream);
/* Host only.  The bytes of `workspace` for n entries, or SNNQP_EINVAL for n outside [0, 2^32). */
int64_t snnqp_magnitude_prune_workspace_bytes(int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* SNNQP_H_ */
