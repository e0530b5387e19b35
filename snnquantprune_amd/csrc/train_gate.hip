// Training of CextNet's gated stages: the backward of
//
//   p = maxpool2x2(y),  y[n, h, w, c] = x[n, h, w, c] * gate[n, c],
//
// together with the spatial mean m[n, c] = (sum_{h, w} x[n, h, w, c]) / (H W) the gate is computed
// from (examples/tcja/models.py:41-99, :184-187).  All tensors float32, NHWC.
//
//   snnqp_gate_pool_grad_gate   ggate[n, c] = sum_windows gp[n, ph, pw, c] x[n, p*(window), c]
//   snnqp_gate_pool_grad_input  gx[n, h, w, c] = route + gm[n, c] / (H W)
//
// p* is the first position of a window, in the order (0,0), (0,1), (1,0), (1,1), at which
// y_i = fl(x_i gate) attains the window's maximum: the compare rule of snnqp_maxpool2x2_backward
// (a later position replaces the choice only when strictly greater), applied to y.  Both kernels
// evaluate it with the same function, so they route alike.
#include "common.h"

namespace snnqp {
namespace {

// The winning position 0..3 of the window whose (0,0) element is x[base].
__device__ __forceinline__ int first_max_gated(const float *__restrict__ x, int64_t base,
                                               int64_t rowC, int32_t C, float g, float *xsel) {
  const int64_t off[4] = {0, C, rowC, rowC + C};
  float xb = x[base];
  float vb = xb * g;
  int best = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const float xv = x[base + off[k]];
    const float v = xv * g;
    if (v > vb) {
      vb = v;
      xb = xv;
      best = k;
    }
  }
  *xsel = xb;
  return best;
}

// One lane per (n, c), consecutive lanes on consecutive channels (rows of x and gp coalesce).  The
// sum is one fmaf chain from +0 over the windows in ascending (ph, pw): a function of (H, W) alone.
__global__ void __launch_bounds__(256)
gate_grad_gate_kernel(const float *__restrict__ x, const float *__restrict__ gate,
                      const float *__restrict__ gp, int64_t n, int32_t H, int32_t W, int32_t C,
                      float *__restrict__ ggate) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int64_t img = e / C;
  const int32_t c = (int32_t)(e - img * C);
  const int32_t PH = H / 2, PW = W / 2;
  const int64_t rowC = (int64_t)W * C;
  const float g = gate[e];
  float acc = 0.0f;
  for (int32_t ph = 0; ph < PH; ++ph) {
    const int64_t xrow = (img * H + 2 * ph) * rowC + c;
    const int64_t grow = ((img * PH + ph) * PW) * (int64_t)C + c;
    for (int32_t pw = 0; pw < PW; ++pw) {
      float xsel;
      first_max_gated(x, xrow + (int64_t)2 * pw * C, rowC, C, g, &xsel);
      acc = __builtin_fmaf(gp[grow + (int64_t)pw * C], xsel, acc);
    }
  }
  ggate[e] = acc;
}

// One lane per element of gx [NB][H][W][C].
__global__ void __launch_bounds__(256)
gate_grad_input_kernel(const float *__restrict__ x, const float *__restrict__ gate,
                       const float *__restrict__ gp, const float *__restrict__ gm, int64_t n,
                       int32_t H, int32_t W, int32_t C, float *__restrict__ gx) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int32_t c = (int32_t)(e % C);
  int64_t t = e / C;
  const int32_t w = (int32_t)(t % W);
  t /= W;
  const int32_t h = (int32_t)(t % H);
  const int64_t img = t / H;
  const int32_t PH = H / 2, PW = W / 2, ph = h >> 1, pw = w >> 1;
  float route = 0.0f;
  if (ph < PH && pw < PW) {
    const float g = gate[img * C + c];
    const int64_t rowC = (int64_t)W * C;
    float xsel;
    const int best = first_max_gated(x, ((img * H + 2 * ph) * W + 2 * pw) * (int64_t)C + c, rowC,
                                     C, g, &xsel);
    if (best == (h & 1) * 2 + (w & 1)) route = gp[((img * PH + ph) * PW + pw) * (int64_t)C + c] * g;
  }
  // the VJP of snnqp_spatial_mean's y = acc / (float)HW: the same division
  gx[e] = route + gm[img * C + c] / (float)(H * W);
}

}  // namespace
}  // namespace snnqp

using namespace snnqp;

extern "C" {

int snnqp_gate_pool_grad_gate(const float *x, const float *gate, const float *gp, int64_t NB,
                              int32_t H, int32_t W, int32_t C, float *ggate,
                              snnqp_stream_t stream) {
  SNNQP_REQUIRE(NB >= 0 && H > 0 && W > 0 && C > 0, SNNQP_EINVAL, "gate_pool_grad_gate: bad shape");
  SNNQP_REQUIRE((double)NB * H * W * C < 0x1p62 && (int64_t)H * W < (1ll << 31), SNNQP_EINVAL,
                "gate_pool_grad_gate: too large");
  if (NB == 0) return SNNQP_OK;
  SNNQP_REQUIRE(x && gate && ggate && (gp || H < 2 || W < 2), SNNQP_EINVAL,
                "gate_pool_grad_gate: null argument");
  const int64_t n = NB * C;
  const int64_t blocks = ceil_div64(n, 256);
  SNNQP_REQUIRE(blocks < (1ll << 31), SNNQP_EINVAL, "gate_pool_grad_gate: grid too large");
  hipLaunchKernelGGL(gate_grad_gate_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, x, gate, gp, n, H, W, C, ggate);
  SNNQP_CHECK_LAUNCH("gate_grad_gate_kernel");
  return SNNQP_OK;
}

int snnqp_gate_pool_grad_input(const float *x, const float *gate, const float *gp, const float *gm,
                               int64_t NB, int32_t H, int32_t W, int32_t C, float *gx,
                               snnqp_stream_t stream) {
  SNNQP_REQUIRE(NB >= 0 && H > 0 && W > 0 && C > 0, SNNQP_EINVAL,
                "gate_pool_grad_input: bad shape");
  SNNQP_REQUIRE((double)NB * H * W * C < 0x1p62 && (int64_t)H * W < (1ll << 31), SNNQP_EINVAL,
                "gate_pool_grad_input: too large");
  if (NB == 0) return SNNQP_OK;
  SNNQP_REQUIRE(x && gate && gm && gx && (gp || H < 2 || W < 2), SNNQP_EINVAL,
                "gate_pool_grad_input: null argument");
  const int64_t n = NB * H * W * C;
  const int64_t blocks = ceil_div64(n, 256);
  SNNQP_REQUIRE(blocks < (1ll << 31), SNNQP_EINVAL, "gate_pool_grad_input: grid too large");
  hipLaunchKernelGGL(gate_grad_input_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, x, gate, gp, gm, n, H, W, C, gx);
  SNNQP_CHECK_LAUNCH("gate_grad_input_kernel");
  return SNNQP_OK;
}

}  // extern "C"
