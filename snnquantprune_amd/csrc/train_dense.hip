// Training of the dense SNN (DenseSNN, configs C1 / C2): the pieces of the surrogate-gradient
// backward pass through time (examples/tcja/models.py:191-255 differentiated by jax.grad).
//
//   snnqp_lif_forward_save   multi_step_LIF scan over float32 currents that also writes the
//                            pre-reset potential h_t (the residual of the backward)
//   snnqp_lif_backward       the time-reversed scan, one lane per (row, feature), with the
//                            surrogate derivative as a template and the vote backward fused
//   snnqp_lif_forward_save_state, snnqp_lif_backward_state
//                            the same two scans over one window of a recording: the forward starts
//                            from a membrane u0 and hands u_T on, the backward takes the gradient
//                            arriving at u_T and hands on the one of u0
//   snnqp_dense_weight_grad  gW[k][n] = sum_m x[m][k] gI[m][n]       (f32-input MFMA)
//   snnqp_dense_input_grad   gx[m][k] = (sum_n gI[m][n] w[k][n]) * mask[m][k]
//
// Both products run on v_mfma_f32_16x16x4_f32, which is an exact k-ordered fmaf chain; every
// output element is reduced by one wave in one fixed order (no atomics), so gradients are
// bitwise reproducible run to run.
#include "common.h"
#include "grad_gemm.h"
#include "surrogate.h"

namespace snnqp {
namespace {

// The forward of neuron_step (common.h) for MULTI_STEP_LIF, keeping h before the reset.
__global__ void lif_save_kernel(const float *__restrict__ x, int32_t T, int64_t n,
                                NeuronP p, float *__restrict__ h_out, float *__restrict__ s_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float u = 0.0f;
  for (int32_t t = 0; t < T; ++t) {
    const int64_t o = (int64_t)t * n + e;
    float d = x[o] - (u - p.vr);                                     // :410
    float h = u + (p.inv_k != 0.0f ? d * p.inv_k : d / p.k);
    bool s = (h - p.vth) >= 0.0f;                                    // :412
    h_out[o] = h;
    s_out[o] = s ? 1.0f : 0.0f;
    u = s ? p.vr : h;                                                // :414
  }
}

// lif_save_kernel from the membrane u0 (null: zeros), with u_T handed on (u_out, nullable).  The
// step is lif_save_kernel's, expression for expression.  u0 and u_out may be one buffer: a lane
// reads its element before it writes it, and no other lane touches it.
__global__ void lif_save_state_kernel(const float *__restrict__ x, int32_t T, int64_t n, NeuronP p,
                                      const float *u0, float *u_out, float *__restrict__ h_out,
                                      float *__restrict__ s_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float u = u0 ? u0[e] : 0.0f;
  for (int32_t t = 0; t < T; ++t) {
    const int64_t o = (int64_t)t * n + e;
    float d = x[o] - (u - p.vr);                                     // :410
    float h = u + (p.inv_k != 0.0f ? d * p.inv_k : d / p.k);
    bool s = (h - p.vth) >= 0.0f;                                    // :412
    h_out[o] = h;
    s_out[o] = s ? 1.0f : 0.0f;
    u = s ? p.vr : h;                                                // :414
  }
  if (u_out) u_out[e] = u;
}

// gh_t = gs_t sigma'(h_t - vth) + gu_t (1 - s_t);  gI_t = gh_t / tau;  gu_{t-1} = gh_t (1 - 1/tau).
// VOTE: gs_t[r][c] = glogits[r][c / group] / (group T) (models.py:253-255), no [T][R][C] upstream.
template <int S, bool VOTE>
__global__ void lif_backward_kernel(const float *__restrict__ h, const float *__restrict__ gs,
                                    const float *__restrict__ glogits, int32_t group,
                                    int32_t T, int64_t R, int32_t C, NeuronP p,
                                    float *__restrict__ gI) {
  const int64_t n = R * C;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float inv = p.inv_k != 0.0f ? p.inv_k : 1.0f / p.k;
  const float keep = 1.0f - inv;
  float gv = 0.0f;
  if constexpr (VOTE) {
    const int64_t r = e / C;
    const int32_t c = (int32_t)(e - r * C);
    gv = glogits[r * (C / group) + c / group] / (float)((int64_t)group * T);
  }
  float gu = 0.0f;                                                   // gu_T = 0
  for (int32_t t = T - 1; t >= 0; --t) {
    const int64_t o = (int64_t)t * n + e;
    const float x = h[o] - p.vth;
    const float s = x >= 0.0f ? 1.0f : 0.0f;                          // the forward's spike
    const float g = VOTE ? gv : gs[o];
    const float gh = g * surrogate_grad<S>(x) + gu * (1.0f - s);
    gI[o] = p.inv_k != 0.0f ? gh * p.inv_k : gh / p.k;
    gu = gh * keep;
  }
}

// lif_backward_kernel with gu_T given (null: zeros) and the recurrence's last gu, dL/du0, handed
// on (gu0, nullable).  u_T = s_{T-1} ? vr : h_{T-1}, so gu_T enters step T-1 as every gu_t does.
template <int S, bool VOTE>
__global__ void lif_backward_state_kernel(const float *__restrict__ h, const float *__restrict__ gs,
                                          const float *__restrict__ glogits, int32_t group,
                                          int32_t T, int64_t R, int32_t C, NeuronP p,
                                          const float *gu_T, float *__restrict__ gI, float *gu0) {
  const int64_t n = R * C;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float inv = p.inv_k != 0.0f ? p.inv_k : 1.0f / p.k;
  const float keep = 1.0f - inv;
  float gv = 0.0f;
  if constexpr (VOTE) {
    const int64_t r = e / C;
    const int32_t c = (int32_t)(e - r * C);
    if (T > 0) gv = glogits[r * (C / group) + c / group] / (float)((int64_t)group * T);
  }
  float gu = gu_T ? gu_T[e] : 0.0f;
  for (int32_t t = T - 1; t >= 0; --t) {
    const int64_t o = (int64_t)t * n + e;
    const float x = h[o] - p.vth;
    const float s = x >= 0.0f ? 1.0f : 0.0f;                          // the forward's spike
    const float g = VOTE ? gv : gs[o];
    const float gh = g * surrogate_grad<S>(x) + gu * (1.0f - s);
    gI[o] = p.inv_k != 0.0f ? gh * p.inv_k : gh / p.k;
    gu = gh * keep;
  }
  if (gu0) gu0[e] = gu;
}

template <int S>
int launch_backward_state(const float *h, const float *gs, const float *glogits, int32_t group,
                          int32_t T, int64_t R, int32_t C, const NeuronP &p, const float *gu_T,
                          float *gI, float *gu0, hipStream_t st) {
  const int64_t blocks = ceil_div64(R * C, 256);
  if (glogits)
    hipLaunchKernelGGL((lif_backward_state_kernel<S, true>), dim3((unsigned)blocks), dim3(256), 0,
                       st, h, gs, glogits, group, T, R, C, p, gu_T, gI, gu0);
  else
    hipLaunchKernelGGL((lif_backward_state_kernel<S, false>), dim3((unsigned)blocks), dim3(256), 0,
                       st, h, gs, glogits, group, T, R, C, p, gu_T, gI, gu0);
  SNNQP_CHECK_LAUNCH("lif_backward_state_kernel");
  return SNNQP_OK;
}

template <int S>
int launch_backward(const float *h, const float *gs, const float *glogits, int32_t group,
                    int32_t T, int64_t R, int32_t C, const NeuronP &p, float *gI,
                    hipStream_t st) {
  const int64_t blocks = ceil_div64(R * C, 256);
  if (glogits)
    hipLaunchKernelGGL((lif_backward_kernel<S, true>), dim3((unsigned)blocks), dim3(256), 0, st,
                       h, gs, glogits, group, T, R, C, p, gI);
  else
    hipLaunchKernelGGL((lif_backward_kernel<S, false>), dim3((unsigned)blocks), dim3(256), 0, st,
                       h, gs, glogits, group, T, R, C, p, gI);
  SNNQP_CHECK_LAUNCH("lif_backward_kernel");
  return SNNQP_OK;
}

// ---- C[i][j] = sum_r A(r, i) B(r, j) (* mask[i][j]) -----------------------------------------
// A(r, i) = a[r * a_sr + i * a_si], B(r, j) = b[r * b_sr + j * b_sj]; C row-major [I][J].
// The tile is grad_gemm.h's.
__global__ __launch_bounds__(256) void grad_gemm_kernel(gg::Strided a, gg::Strided b, int64_t Rn,
                                                        const float *__restrict__ mask,
                                                        float *__restrict__ c) {
  const int64_t i0 = (int64_t)blockIdx.y * gg::GT, j0 = (int64_t)blockIdx.x * gg::GT;
  const int64_t J = b.n;
  gg::f32x4 acc[2][2];
  gg::tile_chain(a, b, i0, j0, 0, Rn, acc);
  gg::tile_store(acc, i0, j0, a.n, J, [&](int64_t i, int64_t j, float v) {
    if (mask) v = v * mask[i * J + j];
    c[i * J + j] = v;
  });
}

int launch_gemm(const float *a, int64_t a_sr, int64_t a_si, const float *b, int64_t b_sr,
                int64_t b_sj, int64_t I, int64_t J, int64_t Rn, const float *mask, float *c,
                hipStream_t st, const char *name) {
  const int64_t gx = ceil_div64(J, gg::GT), gy = ceil_div64(I, gg::GT);
  SNNQP_REQUIRE(gx < 65536 && gy < 65536, SNNQP_EINVAL, "%s: grid too large", name);
  hipLaunchKernelGGL(grad_gemm_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st,
                     gg::make_strided(a, a_sr, a_si, I), gg::make_strided(b, b_sr, b_sj, J), Rn,
                     mask, c);
  SNNQP_CHECK_LAUNCH(name);
  return SNNQP_OK;
}

}  // namespace
}  // namespace snnqp

using namespace snnqp;

extern "C" {

int snnqp_lif_forward_save(const float *x, int32_t T, int64_t R, int32_t C,
                           const snnqp_neuron_t *nrn, float *h_out, float *s_out,
                           snnqp_stream_t stream) {
  SNNQP_REQUIRE(T >= 0 && R >= 0 && C > 0, SNNQP_EINVAL, "lif_forward_save: bad shape");
  SNNQP_REQUIRE(nrn && nrn->kind == SNNQP_NEURON_MULTI_STEP_LIF, SNNQP_EUNSUPPORTED,
                "lif_forward_save: multi_step_LIF only");
  const int64_t n = R * C;
  if (n == 0 || T == 0) return SNNQP_OK;
  SNNQP_REQUIRE(x && h_out && s_out, SNNQP_EINVAL, "lif_forward_save: null argument");
  const int64_t blocks = ceil_div64(n, 256);
  SNNQP_REQUIRE(blocks < (1ll << 31), SNNQP_EINVAL, "lif_forward_save: grid too large");
  hipLaunchKernelGGL(lif_save_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, x, T, n, make_neuron(nrn), h_out, s_out);
  SNNQP_CHECK_LAUNCH("lif_save_kernel");
  return SNNQP_OK;
}

int snnqp_lif_backward(const float *h, const float *gs, const float *glogits, int32_t group,
                       int32_t T, int64_t R, int32_t C, const snnqp_neuron_t *nrn,
                       int surrogate, float *gI, snnqp_stream_t stream) {
  SNNQP_REQUIRE(T >= 0 && R >= 0 && C > 0, SNNQP_EINVAL, "lif_backward: bad shape");
  SNNQP_REQUIRE(nrn && nrn->kind == SNNQP_NEURON_MULTI_STEP_LIF, SNNQP_EUNSUPPORTED,
                "lif_backward: multi_step_LIF only");
  SNNQP_REQUIRE((gs == nullptr) != (glogits == nullptr), SNNQP_EINVAL,
                "lif_backward: exactly one of gs / glogits");
  SNNQP_REQUIRE(!glogits || (group > 0 && C % group == 0), SNNQP_EINVAL,
                "lif_backward: %d features not divisible by group %d", C, group);
  const int64_t n = R * C;
  if (n == 0 || T == 0) return SNNQP_OK;
  SNNQP_REQUIRE(h && gI, SNNQP_EINVAL, "lif_backward: null argument");
  SNNQP_REQUIRE(ceil_div64(n, 256) < (1ll << 31), SNNQP_EINVAL, "lif_backward: grid too large");
  const NeuronP p = make_neuron(nrn);
  hipStream_t st = (hipStream_t)stream;
  switch (surrogate) {
    case SNNQP_SURR_FAST_SIGMOID:
      return launch_backward<SNNQP_SURR_FAST_SIGMOID>(h, gs, glogits, group, T, R, C, p, gI, st);
    case SNNQP_SURR_ATAN:
      return launch_backward<SNNQP_SURR_ATAN>(h, gs, glogits, group, T, R, C, p, gI, st);
    case SNNQP_SURR_SLAYER:
      return launch_backward<SNNQP_SURR_SLAYER>(h, gs, glogits, group, T, R, C, p, gI, st);
    case SNNQP_SURR_SMOOTH_STEP:
      return launch_backward<SNNQP_SURR_SMOOTH_STEP>(h, gs, glogits, group, T, R, C, p, gI, st);
    case SNNQP_SURR_PIECEWISE_LINEAR:
      return launch_backward<SNNQP_SURR_PIECEWISE_LINEAR>(h, gs, glogits, group, T, R, C, p, gI,
                                                          st);
    default:
      set_error("lif_backward: unknown surrogate %d", surrogate);
      return SNNQP_EINVAL;
  }
}

int snnqp_lif_forward_save_state(const float *x, int32_t T, int64_t R, int32_t C,
                                 const snnqp_neuron_t *nrn, const float *u0, float *u_out,
                                 float *h_out, float *s_out, snnqp_stream_t stream) {
  SNNQP_REQUIRE(T >= 0 && R >= 0 && C > 0, SNNQP_EINVAL, "lif_forward_save_state: bad shape");
  SNNQP_REQUIRE(nrn && nrn->kind == SNNQP_NEURON_MULTI_STEP_LIF, SNNQP_EUNSUPPORTED,
                "lif_forward_save_state: multi_step_LIF only");
  const int64_t n = R * C;
  if (n == 0 || (T == 0 && !u_out)) return SNNQP_OK;
  SNNQP_REQUIRE(T == 0 || (x && h_out && s_out), SNNQP_EINVAL,
                "lif_forward_save_state: null argument");
  const int64_t blocks = ceil_div64(n, 256);
  SNNQP_REQUIRE(blocks < (1ll << 31), SNNQP_EINVAL, "lif_forward_save_state: grid too large");
  // T == 0: the loop has no step, and the launch writes u_out = u0 (or zeros)
  hipLaunchKernelGGL(lif_save_state_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, x, T, n, make_neuron(nrn), u0, u_out, h_out, s_out);
  SNNQP_CHECK_LAUNCH("lif_save_state_kernel");
  return SNNQP_OK;
}

int snnqp_lif_backward_state(const float *h, const float *gs, const float *glogits, int32_t group,
                             int32_t T, int64_t R, int32_t C, const snnqp_neuron_t *nrn,
                             int surrogate, const float *gu_T, float *gI, float *gu0,
                             snnqp_stream_t stream) {
  SNNQP_REQUIRE(T >= 0 && R >= 0 && C > 0, SNNQP_EINVAL, "lif_backward_state: bad shape");
  SNNQP_REQUIRE(nrn && nrn->kind == SNNQP_NEURON_MULTI_STEP_LIF, SNNQP_EUNSUPPORTED,
                "lif_backward_state: multi_step_LIF only");
  SNNQP_REQUIRE((gs == nullptr) != (glogits == nullptr), SNNQP_EINVAL,
                "lif_backward_state: exactly one of gs / glogits");
  SNNQP_REQUIRE(!glogits || (group > 0 && C % group == 0), SNNQP_EINVAL,
                "lif_backward_state: %d features not divisible by group %d", C, group);
  const int64_t n = R * C;
  if (n == 0 || (T == 0 && !gu0)) return SNNQP_OK;
  SNNQP_REQUIRE(T == 0 || (h && gI), SNNQP_EINVAL, "lif_backward_state: null argument");
  SNNQP_REQUIRE(ceil_div64(n, 256) < (1ll << 31), SNNQP_EINVAL,
                "lif_backward_state: grid too large");
  const NeuronP p = make_neuron(nrn);
  hipStream_t st = (hipStream_t)stream;
  // T == 0: the loop has no step, and the launch writes gu0 = gu_T (or zeros)
  switch (surrogate) {
    case SNNQP_SURR_FAST_SIGMOID:
      return launch_backward_state<SNNQP_SURR_FAST_SIGMOID>(h, gs, glogits, group, T, R, C, p, gu_T,
                                                            gI, gu0, st);
    case SNNQP_SURR_ATAN:
      return launch_backward_state<SNNQP_SURR_ATAN>(h, gs, glogits, group, T, R, C, p, gu_T, gI, gu0,
                                                    st);
    case SNNQP_SURR_SLAYER:
      return launch_backward_state<SNNQP_SURR_SLAYER>(h, gs, glogits, group, T, R, C, p, gu_T, gI,
                                                      gu0, st);
    case SNNQP_SURR_SMOOTH_STEP:
      return launch_backward_state<SNNQP_SURR_SMOOTH_STEP>(h, gs, glogits, group, T, R, C, p, gu_T,
                                                           gI, gu0, st);
    case SNNQP_SURR_PIECEWISE_LINEAR:
      return launch_backward_state<SNNQP_SURR_PIECEWISE_LINEAR>(h, gs, glogits, group, T, R, C, p,
                                                                gu_T, gI, gu0, st);
    default:
      set_error("lif_backward_state: unknown surrogate %d", surrogate);
      return SNNQP_EINVAL;
  }
}

int snnqp_dense_weight_grad(const float *x, const float *gI, int64_t M, int32_t K, int32_t N,
                            float *gw, snnqp_stream_t stream) {
  SNNQP_REQUIRE(M >= 0 && K > 0 && N > 0, SNNQP_EINVAL, "dense_weight_grad: bad shape");
  SNNQP_REQUIRE(gw && ((x && gI) || M == 0), SNNQP_EINVAL, "dense_weight_grad: null argument");
  // C[k][n] = sum_m x[m][k] gI[m][n]
  return launch_gemm(x, K, 1, gI, N, 1, K, N, M, nullptr, gw, (hipStream_t)stream,
                     "dense_weight_grad");
}

int snnqp_dense_input_grad(const float *gI, const float *w, const float *mask, int64_t M,
                           int32_t K, int32_t N, float *gx, snnqp_stream_t stream) {
  SNNQP_REQUIRE(M >= 0 && K > 0 && N > 0, SNNQP_EINVAL, "dense_input_grad: bad shape");
  SNNQP_REQUIRE((gI && w && gx) || M == 0, SNNQP_EINVAL, "dense_input_grad: null argument");
  if (M == 0) return SNNQP_OK;
  // C[m][k] = sum_n gI[m][n] w[k][n]: r = n, i = m, j = k
  return launch_gemm(gI, 1, N, w, 1, N, M, K, N, mask, gx, (hipStream_t)stream,
                     "dense_input_grad");
}

}  // extern "C"
