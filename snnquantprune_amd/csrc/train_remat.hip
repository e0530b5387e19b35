// Training of a conv block with rematerialisation (conv_train.RematConvBlock): the
// block keeps neither its currents nor h, and recomputes them chunk by chunk in the backward.
//
//   snnqp_bn_lif_forward_state   the batch-statistics normalisation and the multi_step_LIF scan of
//                                one chunk in one pass, from a membrane u0 to u_T: what such a block
//                                runs twice per step, once forward and once to recompute h
//   snnqp_maxpool2x2_backward_h  snnqp_maxpool2x2_backward with the pool's input taken from h by
//                                the forward's own compare, so no spike raster is written again
//
// Both are memory-bound walks, one lane per element e = r C + c, every access along e.
#include "common.h"

namespace snnqp {
namespace {

// y_t = fl(fl(fl(cur_t - mean[t][c]) * mul[t][c]) + bias[c]) (conv_train.bn_normalise: three
// roundings, -ffp-contract=off keeps them), then the step of lif_save_state_kernel
// (train_dense.hip), expression for expression.  y is never written.  u0 and u_out may be one
// buffer: a lane reads its element before it writes it, and no other lane touches it.
__global__ void bn_lif_state_kernel(const float *__restrict__ cur, const float *__restrict__ mean,
                                    const float *__restrict__ mul, const float *__restrict__ bias,
                                    int32_t T, int64_t n, int32_t C, NeuronP p, const float *u0,
                                    float *u_out, float *__restrict__ h_out,
                                    float *__restrict__ s_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int32_t c = (int32_t)(e % C);
  float u = u0 ? u0[e] : 0.0f;
  const float b = T > 0 ? bias[c] : 0.0f;
  for (int32_t t = 0; t < T; ++t) {
    const int64_t o = (int64_t)t * n + e;
    const int64_t k = (int64_t)t * C + c;
    float x = cur[o] - mean[k];
    x = x * mul[k];
    x = x + b;
    float d = x - (u - p.vr);                                        // :410
    float h = u + (p.inv_k != 0.0f ? d * p.inv_k : d / p.k);
    bool s = (h - p.vth) >= 0.0f;                                    // :412
    if (h_out) h_out[o] = h;
    if (s_out) s_out[o] = s ? 1.0f : 0.0f;
    u = s ? p.vr : h;                                                // :414
  }
  if (u_out) u_out[e] = u;
}

// pool_backward_kernel (train_conv.hip) on s = ((h - vth) >= 0): one lane per element of
// gs [NB][H][W][C].  Window order (0,0), (0,1), (1,0), (1,1); a later position replaces the choice
// only when strictly greater, so ties go to the first.
__global__ void pool_backward_h_kernel(const float *__restrict__ hp, float vth,
                                       const float *__restrict__ gp, int64_t n, int32_t H,
                                       int32_t W, int32_t C, float *__restrict__ gs) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int32_t c = (int32_t)(e % C);
  int64_t t = e / C;
  const int32_t w = (int32_t)(t % W);
  t /= W;
  const int32_t h = (int32_t)(t % H);
  const int64_t img = t / H;
  const int32_t PH = H / 2, PW = W / 2, ph = h >> 1, pw = w >> 1;
  float out = 0.0f;
  if (ph < PH && pw < PW) {
    const int64_t base = ((img * H + 2 * ph) * W + 2 * pw) * C + c;
    const int64_t off[4] = {0, C, (int64_t)W * C, (int64_t)W * C + C};
    int best = 0;
    float vb = (hp[base] - vth) >= 0.0f ? 1.0f : 0.0f;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float v = (hp[base + off[k]] - vth) >= 0.0f ? 1.0f : 0.0f;
      if (v > vb) {
        vb = v;
        best = k;
      }
    }
    if (best == (h & 1) * 2 + (w & 1)) out = gp[((img * PH + ph) * PW + pw) * C + c];
  }
  gs[e] = out;
}

}  // namespace
}  // namespace snnqp

using namespace snnqp;

extern "C" {

int snnqp_bn_lif_forward_state(const float *cur, const float *mean, const float *mul,
                               const float *bias, int32_t T, int64_t R, int32_t C,
                               const snnqp_neuron_t *nrn, const float *u0, float *u_out,
                               float *h_out, float *s_out, snnqp_stream_t stream) {
  SNNQP_REQUIRE(T >= 0 && R >= 0 && C > 0, SNNQP_EINVAL, "bn_lif_forward_state: bad shape");
  SNNQP_REQUIRE(nrn && nrn->kind == SNNQP_NEURON_MULTI_STEP_LIF, SNNQP_EUNSUPPORTED,
                "bn_lif_forward_state: multi_step_LIF only; the scan of a neuron with a parameter "
                "is snnqp_neuron_forward_save_state");
  SNNQP_REQUIRE((double)R * C * (T > 0 ? T : 1) < 0x1p62, SNNQP_EINVAL,
                "bn_lif_forward_state: too large");
  const int64_t n = R * C;
  if (n == 0 || (T == 0 && !u_out)) return SNNQP_OK;
  SNNQP_REQUIRE(T == 0 || (cur && mean && mul && bias), SNNQP_EINVAL,
                "bn_lif_forward_state: null argument");
  const int64_t blocks = ceil_div64(n, 256);
  SNNQP_REQUIRE(blocks < (1ll << 31), SNNQP_EINVAL, "bn_lif_forward_state: grid too large");
  // T == 0: the loop has no step, and the launch writes u_out = u0 (or zeros)
  hipLaunchKernelGGL(bn_lif_state_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, cur, mean, mul, bias, T, n, C, make_neuron(nrn), u0,
                     u_out, h_out, s_out);
  SNNQP_CHECK_LAUNCH("bn_lif_state_kernel");
  return SNNQP_OK;
}

int snnqp_maxpool2x2_backward_h(const float *h, float vth, const float *gp, int64_t NB, int32_t H,
                                int32_t W, int32_t C, float *gs, snnqp_stream_t stream) {
  SNNQP_REQUIRE(NB >= 0 && H >= 0 && W >= 0 && C > 0, SNNQP_EINVAL,
                "maxpool2x2_backward_h: bad shape");
  SNNQP_REQUIRE((double)NB * H * W * C < 0x1p62, SNNQP_EINVAL, "maxpool2x2_backward_h: too large");
  const int64_t n = NB * H * W * C;
  if (n == 0) return SNNQP_OK;
  SNNQP_REQUIRE(h && gs && (gp || H < 2 || W < 2), SNNQP_EINVAL,
                "maxpool2x2_backward_h: null argument");
  const int64_t blocks = ceil_div64(n, 256);
  SNNQP_REQUIRE(blocks < (1ll << 31), SNNQP_EINVAL, "maxpool2x2_backward_h: grid too large");
  hipLaunchKernelGGL(pool_backward_h_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, h, vth, gp, n, H, W, C, gs);
  SNNQP_CHECK_LAUNCH("pool_backward_h_kernel");
  return SNNQP_OK;
}

}  // extern "C"
