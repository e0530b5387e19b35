// Entry points of the fused SpikingBlock (spiking_learning.py:446-462) and the
// dispatch between the direct-form kernel and the int8 MFMA kernels.
#include "common.h"
#include "kernels.h"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>

using namespace snnqp;

// A block that IMPL_AUTO hands to the direct-form kernel runs 20-25 x slower than on the MFMA
// kernels (one thread per output neuron): counted, with the reason, so that a caller (and
// bench.py's JSON line) can see the cliff instead of guessing at it.
namespace {
std::atomic<int64_t> g_fallback_conv{0}, g_fallback_dense{0};
std::mutex g_fallback_mu;
char g_fallback_reason[256] = "";

void note_fallback(bool dense, const char *why) {
  (dense ? g_fallback_dense : g_fallback_conv).fetch_add(1, std::memory_order_relaxed);
  static const bool log = std::getenv("SNNQP_LOG_FALLBACKS") != nullptr;
  std::lock_guard<std::mutex> lock(g_fallback_mu);
  const bool fresh = std::strncmp(g_fallback_reason + (dense ? 7 : 6), why ? why : "", 200) != 0;
  std::snprintf(g_fallback_reason, sizeof(g_fallback_reason), "%s%s", dense ? "dense: " : "conv: ",
                why ? why : "");
  if (log && fresh)
    std::fprintf(stderr, "libsnnqp: %s block on the direct-form kernel: %s\n",
                 dense ? "dense" : "conv", why ? why : "");
}

// a dense layer as the direct-form kernel sees it: a 1x1 convolution on a 1x1 image
snnqp_conv_geom_t dense_geom(int32_t K, int32_t N) {
  snnqp_conv_geom_t g;
  g.H = 1; g.W = 1; g.Cin = K; g.Cout = N; g.KH = 1; g.KW = 1;
  g.stride_h = g.stride_w = 1;
  g.pad_h_lo = g.pad_h_hi = g.pad_w_lo = g.pad_w_hi = 0;
  g.in_dil_h = g.in_dil_w = g.k_dil_h = g.k_dil_w = 1;
  g.groups = 1;
  return g;
}

#define SNNQP_CHECK_NEURON_KIND(nrn, who)                                                      \
  SNNQP_REQUIRE((nrn)->kind >= SNNQP_NEURON_MULTI_STEP_LIF && (nrn)->kind <= SNNQP_NEURON_LIF, \
                SNNQP_EINVAL, "%s: unknown neuron kind %d", who, (nrn)->kind)

// the preamble of the three conv entry points (the x_flags rule: the forms that stage float32 frames)
int conv_preamble(const char *who, const BlockCall &c, bool predicated, bool stages_f32) {
  SNNQP_REQUIRE((c.pred || !predicated) && c.g && c.w && c.nrn, SNNQP_EINVAL, "%s: null %s", who,
                predicated ? "argument" : "descriptor");
  if (stages_f32 && c.in_type == SNNQP_F32 && c.w->wtype == SNNQP_W_I8)
    SNNQP_REQUIRE(c.x_flags, SNNQP_EINVAL, "%s: float32 input into integer codes needs x_flags (snnqp.h)", who);
  if (int rc = refuse_after_device_report(c.st, who)) return rc;
  SNNQP_CHECK_NEURON_KIND(c.nrn, who);
  SNNQP_REQUIRE(c.pool == 1 || c.pool == 2, SNNQP_EINVAL, "%s: pool must be 1 or 2", who);
  return SNNQP_OK;
}
}  // namespace

namespace snnqp {
int block_entry(const char *who, const BlockCall &c, bool ptrs) {
  const bool empty = c.T == 0 || c.B == 0;
  SNNQP_REQUIRE(ptrs && ((c.x && c.s_out) || empty), SNNQP_EINVAL, "%s: null pointer", who);
  SNNQP_REQUIRE(c.T >= 0 && c.B >= 0, SNNQP_EINVAL, "%s: negative T/B", who);
  SNNQP_REQUIRE(c.w->L >= 1.0f, SNNQP_EINVAL, "dequant L must be >= 1");
  SNNQP_CHECK_BN(c.bn);
  return empty ? BLOCK_EMPTY : SNNQP_OK;
}

int dense_rows_broken(const BlockCall &c, int in_type, int samples, int64_t steps, int64_t extent) {
  const int64_t align = in_type == SNNQP_U8 ? 16 : 4;       // of the strides, in elements: 16 bytes
  int broken = c.xs_t < 0 || c.xs_b < 0 ? ROWS_NEGATIVE : 0;
  if ((in_type == SNNQP_U8 || in_type == SNNQP_F32) &&
      ((((uintptr_t)c.x) & 15) != 0 || c.xs_t % align != 0 || c.xs_b % align != 0))
    broken |= ROWS_UNALIGNED;
  if ((steps * c.xs_t + samples * c.xs_b + extent) * (in_type == SNNQP_F32 ? 4 : 1) >= ((int64_t)1 << 31))
    broken |= ROWS_REACH;
  return broken;
}
}  // namespace snnqp

extern "C" {

int snnqp_fallback_counts(int64_t *conv_blocks, int64_t *dense_blocks, char *reason,
                          int32_t reason_len, int reset) {
  if (conv_blocks) *conv_blocks = g_fallback_conv.load(std::memory_order_relaxed);
  if (dense_blocks) *dense_blocks = g_fallback_dense.load(std::memory_order_relaxed);
  std::lock_guard<std::mutex> lock(g_fallback_mu);
  if (reason && reason_len > 0) {
    std::strncpy(reason, g_fallback_reason, (size_t)reason_len - 1);
    reason[reason_len - 1] = 0;
  }
  if (reset) {
    g_fallback_conv = 0;
    g_fallback_dense = 0;
    g_fallback_reason[0] = 0;
  }
  return SNNQP_OK;
}

int snnqp_conv_dequant_form(const snnqp_weight_t *w, const snnqp_neuron_t *nrn) {
  SNNQP_REQUIRE(w && nrn, SNNQP_EINVAL, "conv_dequant_form: null descriptor");
  SNNQP_REQUIRE(w->wtype == SNNQP_W_I8, SNNQP_EINVAL, "conv_dequant_form: int8 codes only");
  return conv3x3_bits_dequant_form(w, nrn);
}

int snnqp_conv_event_half_group(int in_type, int32_t T, const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                                const snnqp_neuron_t *nrn, int has_state, int pool, int x_max) {
  SNNQP_REQUIRE(g && w && nrn, SNNQP_EINVAL, "conv_event_half_group: null descriptor");
  SNNQP_CHECK_NEURON_KIND(nrn, "conv_event_half_group");
  return conv3x3_event_half_group(in_type, T, g, w, nrn, has_state != 0, pool, x_max);
}

int snnqp_conv_event_wave_spread(int in_type, int32_t T, const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                                 const snnqp_neuron_t *nrn, int has_state, int pool, int x_max) {
  SNNQP_REQUIRE(g && w && nrn, SNNQP_EINVAL, "conv_event_wave_spread: null descriptor");
  SNNQP_CHECK_NEURON_KIND(nrn, "conv_event_wave_spread");
  return conv3x3_event_wave_spread(in_type, T, g, w, nrn, has_state != 0, pool, x_max);
}

int snnqp_conv_event_quarter16(int in_type, int32_t T, const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                               const snnqp_neuron_t *nrn, int has_state, int pool, int x_max) {
  SNNQP_REQUIRE(g && w && nrn, SNNQP_EINVAL, "conv_event_quarter16: null descriptor");
  SNNQP_CHECK_NEURON_KIND(nrn, "conv_event_quarter16");
  return conv3x3_event_quarter16(in_type, T, g, w, nrn, has_state != 0, pool, x_max);
}

int snnqp_conv_lif_forward(const void *x, int in_type, int64_t x_stride_t,
                           int64_t x_stride_b, int32_t T, int32_t B,
                           const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                           const int8_t *wt, const snnqp_bn_t *bn,
                           const snnqp_neuron_t *nrn,
                           const float *u0, float *u_out, void *s_out,
                           int s_type, int pool, int impl, int x_max, int32_t *x_seen,
                           int32_t *x_flags, snnqp_stream_t stream) {
  const BlockCall c{x, in_type, x_stride_t, x_stride_b, T, B, w, wt, bn, nrn, u0, u_out, s_out, s_type,
                    x_flags, nullptr, (hipStream_t)stream, g, pool, x_max, x_seen};
  if (int rc = conv_preamble("conv_lif_forward", c, false, true)) return rc;
  SNNQP_REQUIRE(impl >= SNNQP_IMPL_AUTO && impl <= SNNQP_IMPL_MFMA, SNNQP_EINVAL,
                "conv_lif_forward: unknown impl %d", impl);
  const char *why = conv3x3_mfma_unsupported(c);
  if (impl == SNNQP_IMPL_MFMA)
    SNNQP_REQUIRE(!why, SNNQP_EUNSUPPORTED, "conv_lif_forward: MFMA kernel: %s", why);
  if (!why && impl != SNNQP_IMPL_GENERIC) return run_conv3x3_mfma(c);
  // the direct-form kernel reads no packed event frames: refused here, before it counts as a fallback
  SNNQP_REQUIRE(in_type != SNNQP_EV1 && in_type != SNNQP_EV4, SNNQP_EUNSUPPORTED,
                "conv_lif_forward: packed event frames need bit-packed spike output; unpack them first "
                "(%s)", why ? why : "impl = GENERIC");
  SNNQP_REQUIRE(!(in_type == SNNQP_F32 && w->wtype == SNNQP_W_I8), SNNQP_EUNSUPPORTED,
                "conv_lif_forward: float32 input into integer codes is staged by the event-layer MFMA "
                "kernel only (%s); narrow it first (snnqp_narrow_f32 / snnqp_pack_bits_checked)",
                why ? why : "impl = GENERIC");
  SNNQP_REQUIRE(pool == 1, SNNQP_EUNSUPPORTED,
                "conv_lif_forward: the direct-form kernel does not fuse the "
                "max-pool; call snnqp_maxpool2x2 after it");
  if (impl == SNNQP_IMPL_AUTO) note_fallback(false, why);
  return run_generic(c, nullptr, nullptr);
}

int snnqp_conv_lif_forward_pred(const int32_t *pred, const void *x, int in_type, int64_t x_stride_t,
                                int64_t x_stride_b, int32_t T, int32_t B,
                                const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                                const int8_t *wt, const snnqp_bn_t *bn,
                                const snnqp_neuron_t *nrn,
                                const float *u0, float *u_out, void *s_out,
                                int s_type, int pool, int x_max, int32_t *x_seen,
                                int32_t *x_flags, snnqp_stream_t stream) {
  const BlockCall c{x, in_type, x_stride_t, x_stride_b, T, B, w, wt, bn, nrn, u0, u_out, s_out, s_type,
                    x_flags, pred, (hipStream_t)stream, g, pool, x_max, x_seen};
  if (int rc = conv_preamble("conv_lif_forward_pred", c, true, true)) return rc;
  SNNQP_REQUIRE(in_type == SNNQP_U8 || in_type == SNNQP_F32 || in_type == SNNQP_EV4, SNNQP_EUNSUPPORTED,
                "conv_lif_forward_pred: byte, nibble or float32 frames (the event layer's own formats)");
  const char *why = conv3x3_mfma_unsupported(c);
  SNNQP_REQUIRE(!why, SNNQP_EUNSUPPORTED, "conv_lif_forward_pred: MFMA kernel: %s", why);
  return run_conv3x3_mfma(c);
}

int snnqp_conv_lif_forward_if(const int32_t *pred, const void *x, int in_type, int64_t x_stride_t,
                              int64_t x_stride_b, int32_t T, int32_t B,
                              const snnqp_conv_geom_t *g, const snnqp_weight_t *w,
                              const snnqp_bn_t *bn, const snnqp_neuron_t *nrn, const float *u0,
                              float *u_out, void *s_out, int s_type, int pool,
                              snnqp_stream_t stream) {
  const BlockCall c{x, in_type, x_stride_t, x_stride_b, T, B, w, nullptr, bn, nrn, u0, u_out, s_out, s_type,
                    nullptr, pred, (hipStream_t)stream, g, pool};
  if (int rc = conv_preamble("conv_lif_forward_if", c, true, false)) return rc;
  return run_generic(c, nullptr, nullptr);
}

int snnqp_dense_lif_forward_if(const int32_t *pred, const void *x, int in_type, int64_t x_stride_t,
                               int64_t x_stride_b, int32_t T, int32_t B, int32_t K, int32_t N,
                               const snnqp_weight_t *w, const snnqp_bn_t *bn,
                               const snnqp_neuron_t *nrn, const float *u0, float *u_out,
                               void *s_out, int s_type, snnqp_stream_t stream) {
  SNNQP_REQUIRE(pred && w && nrn && K > 0 && N > 0, SNNQP_EINVAL, "dense_lif_forward_if: bad argument");
  if (int rc = refuse_after_device_report((hipStream_t)stream, "dense_lif_forward_if")) return rc;
  SNNQP_CHECK_NEURON_KIND(nrn, "dense_lif_forward_if");
  const snnqp_conv_geom_t g = dense_geom(K, N);
  const BlockCall c{x, in_type, x_stride_t, x_stride_b, T, B, w, nullptr, bn, nrn, u0, u_out, s_out, s_type,
                    nullptr, pred, (hipStream_t)stream, &g};
  return run_generic(c, nullptr, nullptr);
}

int snnqp_current_min(const snnqp_weight_t *w, const snnqp_bn_t *bn, int32_t bound,
                      int32_t Cout, uint32_t *out_bits, snnqp_stream_t stream) {
  return run_current_min(w, bn, bound, Cout, out_bits, (hipStream_t)stream);
}

int64_t snnqp_dense_workspace_bytes(int in_type, int32_t T, int32_t B, int32_t K, int32_t N,
                                    const snnqp_weight_t *w) {
  if (!w || dense_fp6_unsupported(in_type, K, N, w)) return 0;
  return dense_fp6_workspace_bytes(T, B, K, N);
}

int snnqp_dense_lif_forward(const void *x, int in_type, int64_t x_stride_t,
                            int64_t x_stride_b, int32_t T, int32_t B, int32_t K,
                            int32_t N, const snnqp_weight_t *w,
                            const int8_t *wt, const snnqp_bn_t *bn,
                            const snnqp_neuron_t *nrn, const float *u0,
                            float *u_out, void *s_out, int s_type, int impl,
                            snnqp_stream_t stream) {
  return snnqp_dense_lif_forward_ws(x, in_type, x_stride_t, x_stride_b, T, B, K, N, w, wt, bn, nrn, u0,
                                    u_out, s_out, s_type, impl, nullptr, nullptr, 0, stream);
}

int snnqp_dense_lif_forward_ws(const void *x, int in_type, int64_t x_stride_t,
                               int64_t x_stride_b, int32_t T, int32_t B, int32_t K,
                               int32_t N, const snnqp_weight_t *w,
                               const int8_t *wt, const snnqp_bn_t *bn,
                               const snnqp_neuron_t *nrn, const float *u0,
                               float *u_out, void *s_out, int s_type, int impl,
                               int32_t *x_flags, void *ws, int64_t ws_bytes, snnqp_stream_t stream) {
  SNNQP_REQUIRE(w && nrn, SNNQP_EINVAL, "dense_lif_forward: null descriptor");
  const bool f32_int = in_type == SNNQP_F32 && w->wtype == SNNQP_W_I8;
  if (f32_int)
    SNNQP_REQUIRE(x_flags != nullptr, SNNQP_EINVAL,
                  "dense_lif_forward: float32 rows into integer codes need x_flags (snnqp.h)");
  if (int rc = refuse_after_device_report((hipStream_t)stream, "dense_lif_forward")) return rc;
  SNNQP_REQUIRE(K > 0 && N > 0, SNNQP_EINVAL, "dense_lif_forward: bad K/N");
  SNNQP_CHECK_NEURON_KIND(nrn, "dense_lif_forward");
  SNNQP_REQUIRE(impl >= SNNQP_IMPL_AUTO && impl <= SNNQP_IMPL_MFMA, SNNQP_EINVAL,
                "dense_lif_forward: unknown impl %d", impl);
  const snnqp_conv_geom_t g = dense_geom(K, N);
  const BlockCall c{x, in_type, x_stride_t, x_stride_b, T, B, w, wt, bn, nrn, u0, u_out, s_out, s_type,
                    x_flags, nullptr, (hipStream_t)stream, &g, 1, 0, nullptr, K, N, ws, ws_bytes};
  // The routes, best first: fp6 tiles over bit-packed rows; more than 128 features, every row read
  // once; then the 128-column kernel, the one whose reason a caller gets to see.
  if (impl != SNNQP_IMPL_GENERIC) {
    if (!dense_fp6_unsupported(c)) return run_dense_fp6(c);
    if (!dense_wide_unsupported(c)) return run_dense_wide(c);
  }
  SNNQP_REQUIRE(!f32_int, SNNQP_EUNSUPPORTED,
                "dense_lif_forward: float32 rows into integer codes are staged by the wide MFMA kernel only "
                "(more than 128 features, T <= 64, K %% 16 == 0, 16-byte aligned rows); narrow them first "
                "(snnqp_narrow_f32)");
  const char *why = dense_mfma_unsupported(c);
  if (impl == SNNQP_IMPL_MFMA)
    SNNQP_REQUIRE(!why, SNNQP_EUNSUPPORTED, "dense_lif_forward: MFMA kernel: %s", why);
  if (!why && impl != SNNQP_IMPL_GENERIC) return run_dense_mfma(c);
  if (impl == SNNQP_IMPL_AUTO) note_fallback(true, why);
  return run_generic(c, nullptr, nullptr);
}

}  // extern "C"
