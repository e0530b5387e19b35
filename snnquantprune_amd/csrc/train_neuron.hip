// Training of the neurons that have something to learn: parametric_leaky_IF (one scalar tau,
// m = sigmoid(tau)) and LIF (a decay sigmoid(tau[c]) per feature), spiking_learning.py:357-387
// and :419-438 differentiated by jax.grad.  DESIGN.md 17.
//
//   snnqp_neuron_forward_save   the scan of common.h's neuron_step over float32 currents that also
//                               writes the pre-reset potential h_t (the residual of the backward)
//   snnqp_neuron_backward       the time-reversed scan -> gI, and the float64 sums the parameter's
//                               gradient is made of: Gm = sum gh d (PLIF), Gd_c = sum gh u (LIF)
//   snnqp_neuron_forward_save_state, snnqp_neuron_backward_state
//                               the same two over one window of a recording: from a membrane u0 to
//                               u_T, from the gradient arriving at u_T to the one of u0, and with
//                               u_{-1} = u0 in the t = 0 term of the sums
//
// The rows are cut into `splits` contiguous ranges; one lane per (range, feature), adjacent lanes
// on adjacent features.  A lane walks its rows ascending and each row's t descending, forms every
// product in float64 from the two float32 factors (exact) and adds it to its float64 partial; a
// second kernel adds the partials of a feature in range order (in groups of 32 ranges, then the
// groups in order, when there are more than 32) and, for PLIF, a last one adds the features in
// order.  No atomics: the sums are bitwise reproducible for a given `splits`, and `splits` is a
// function of the shapes alone.
#include "common.h"
#include "surrogate.h"

namespace snnqp {
namespace {

// lanes the default `splits` aims at (DESIGN.md 17.5 has the timings that chose it)
constexpr int64_t kLanesAimed = 262144;

template <int KIND>
__global__ void neuron_save_kernel(const float *__restrict__ x, int32_t T, int64_t n, int32_t C,
                                   NeuronP p, float *__restrict__ h_out,
                                   float *__restrict__ s_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float dec = 0.0f;
  if constexpr (KIND == SNNQP_NEURON_LIF) dec = p.decay[e % C];
  float u = 0.0f;
  for (int32_t t = 0; t < T; ++t) {
    const int64_t o = (int64_t)t * n + e;
    float h;
    if constexpr (KIND == SNNQP_NEURON_PARAMETRIC_LEAKY_IF) {
      float d = x[o] - (u - p.vr);                                   // :381
      h = u + d * p.k;
    } else {
      h = u * dec + x[o];                                            // :432
    }
    bool s = (h - p.vth) >= 0.0f;                                    // :383 / :434
    h_out[o] = h;
    s_out[o] = s ? 1.0f : 0.0f;
    u = s ? p.vr : h;                                                // :385 / :436
  }
}

// neuron_save_kernel from the membrane u0 (null: zeros), with u_T handed on (u_out, nullable): the
// step is neuron_save_kernel's, expression for expression.  u0 and u_out may be one buffer: a lane
// reads its element before it writes it, and no other lane touches it.
template <int KIND>
__global__ void neuron_save_state_kernel(const float *__restrict__ x, int32_t T, int64_t n,
                                         int32_t C, NeuronP p, const float *u0, float *u_out,
                                         float *__restrict__ h_out, float *__restrict__ s_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float dec = 0.0f;
  if constexpr (KIND == SNNQP_NEURON_LIF) dec = p.decay[e % C];
  float u = u0 ? u0[e] : 0.0f;
  for (int32_t t = 0; t < T; ++t) {
    const int64_t o = (int64_t)t * n + e;
    float h;
    if constexpr (KIND == SNNQP_NEURON_PARAMETRIC_LEAKY_IF) {
      float d = x[o] - (u - p.vr);                                   // :381
      h = u + d * p.k;
    } else {
      h = u * dec + x[o];                                            // :432
    }
    bool s = (h - p.vth) >= 0.0f;                                    // :383 / :434
    h_out[o] = h;
    s_out[o] = s ? 1.0f : 0.0f;
    u = s ? p.vr : h;                                                // :385 / :436
  }
  if (u_out) u_out[e] = u;
}

// first row of range s when R rows are cut into `splits` ranges whose lengths differ by at most one
__device__ __forceinline__ int64_t range_begin(int64_t s, int64_t base, int64_t rem) {
  return s * base + (s < rem ? s : rem);
}

// gh_t = g_t sigma'(h_t - vth) + gu_t (1 - s_t), gu_T = 0, u_{t-1} = s_{t-1} ? vr : h_{t-1}, u_{-1} = 0
//   PLIF: gI_t = gh_t m, gu_{t-1} = gh_t (1 - m), partial += gh_t (x_t - (u_{t-1} - vr))
//   LIF:  gI_t = gh_t,   gu_{t-1} = gh_t d_c,     partial += gh_t u_{t-1}
// VOTE: g_t[r][c] = glogits[r][c / group] / (group T), as lif_backward_kernel's.
template <int KIND, int S, bool VOTE>
__global__ void neuron_backward_kernel(const float *__restrict__ h, const float *__restrict__ x,
                                       const float *__restrict__ gs,
                                       const float *__restrict__ glogits, int32_t group, int32_t T,
                                       int64_t R, int32_t C, int32_t splits, NeuronP p,
                                       float *__restrict__ gI, double *__restrict__ partial) {
  const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= (int64_t)splits * C) return;
  const int64_t sp = lane / C;
  const int32_t c = (int32_t)(lane - sp * C);
  const int64_t base = R / splits, rem = R % splits;
  const int64_t r0 = range_begin(sp, base, rem), r1 = range_begin(sp + 1, base, rem);
  const int64_t n = R * C;
  constexpr bool PLIF = KIND == SNNQP_NEURON_PARAMETRIC_LEAKY_IF;
  const float w = PLIF ? 1.0f - p.k : p.decay[c];                    // what gu keeps of gh
  double acc = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t e = r * C + c;
    float gv = 0.0f;
    if constexpr (VOTE) gv = glogits[r * (C / group) + c / group] / (float)((int64_t)group * T);
    float gu = 0.0f;                                                 // gu_T = 0
    float hc = h[(int64_t)(T - 1) * n + e];
    for (int32_t t = T - 1; t >= 0; --t) {
      const int64_t o = (int64_t)t * n + e;
      float up = 0.0f;                                               // u_{-1} = 0
      float hp = 0.0f;
      if (t > 0) {
        hp = h[o - n];
        up = (hp - p.vth) >= 0.0f ? p.vr : hp;
      }
      const float xh = hc - p.vth;
      const float s = xh >= 0.0f ? 1.0f : 0.0f;                       // the forward's spike
      const float g = VOTE ? gv : gs[o];
      const float gh = g * surrogate_grad<S>(xh) + gu * (1.0f - s);
      if constexpr (PLIF) {
        gI[o] = gh * p.k;
        const float d = x[o] - (up - p.vr);                          // the forward's own difference
        acc += (double)gh * (double)d;
      } else {
        gI[o] = gh;
        acc += (double)gh * (double)up;
      }
      gu = gh * w;
      hc = hp;
    }
  }
  partial[lane] = acc;
}

// neuron_backward_kernel over a window: gu_T given (null: zeros), u_{-1} = u0[e] (null: zeros) in
// the t = 0 term of both sums, and the recurrence's last gu, dL/du0, handed on (gu0, nullable).
// The host launches it with T > 0 only.
template <int KIND, int S, bool VOTE>
__global__ void neuron_backward_state_kernel(const float *__restrict__ h,
                                             const float *__restrict__ x,
                                             const float *__restrict__ u0,
                                             const float *__restrict__ gs,
                                             const float *__restrict__ glogits, int32_t group,
                                             int32_t T, int64_t R, int32_t C, int32_t splits,
                                             NeuronP p, const float *gu_T, float *__restrict__ gI,
                                             float *gu0, double *__restrict__ partial) {
  const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= (int64_t)splits * C) return;
  const int64_t sp = lane / C;
  const int32_t c = (int32_t)(lane - sp * C);
  const int64_t base = R / splits, rem = R % splits;
  const int64_t r0 = range_begin(sp, base, rem), r1 = range_begin(sp + 1, base, rem);
  const int64_t n = R * C;
  constexpr bool PLIF = KIND == SNNQP_NEURON_PARAMETRIC_LEAKY_IF;
  const float w = PLIF ? 1.0f - p.k : p.decay[c];                    // what gu keeps of gh
  double acc = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t e = r * C + c;
    float gv = 0.0f;
    if constexpr (VOTE) gv = glogits[r * (C / group) + c / group] / (float)((int64_t)group * T);
    float gu = gu_T ? gu_T[e] : 0.0f;
    float hc = h[(int64_t)(T - 1) * n + e];
    for (int32_t t = T - 1; t >= 0; --t) {
      const int64_t o = (int64_t)t * n + e;
      float up = 0.0f;
      float hp = 0.0f;
      if (t > 0) {
        hp = h[o - n];
        up = (hp - p.vth) >= 0.0f ? p.vr : hp;
      } else if (u0) {
        up = u0[e];                                                  // u_{-1} = u0
      }
      const float xh = hc - p.vth;
      const float s = xh >= 0.0f ? 1.0f : 0.0f;                       // the forward's spike
      const float g = VOTE ? gv : gs[o];
      const float gh = g * surrogate_grad<S>(xh) + gu * (1.0f - s);
      if constexpr (PLIF) {
        gI[o] = gh * p.k;
        const float d = x[o] - (up - p.vr);                          // the forward's own difference
        acc += (double)gh * (double)d;
      } else {
        gI[o] = gh;
        acc += (double)gh * (double)up;
      }
      gu = gh * w;
      hc = hp;
    }
    if (gu0) gu0[e] = gu;
  }
  partial[lane] = acc;
}

// ranges are added in groups of kGroup, then the groups: two short chains in place of one long one
constexpr int32_t kGroup = 32;

// out[g][c] = ((p[g kGroup][c] + p[g kGroup + 1][c]) + ...) over the ranges of group g: one lane per
// (group, feature).  With `per` >= `splits` there is one group, and out is [C].
__global__ void sum_ranges_kernel(const double *__restrict__ partial, int32_t splits, int32_t per,
                                  int32_t C, double *__restrict__ out) {
  const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t groups = (splits + per - 1) / per;
  if (lane >= groups * C) return;
  const int64_t g = lane / C;
  const int32_t c = (int32_t)(lane - g * C);
  const int64_t s0 = g * per, s1 = s0 + per < splits ? s0 + per : splits;
  double acc = 0.0;
  for (int64_t s = s0; s < s1; ++s) acc += partial[s * C + c];
  out[lane] = acc;
}

// out[0] = ((v[0] + v[1]) + v[2]) + ...: one lane, C is a layer's width
__global__ void sum_features_kernel(const double *__restrict__ v, int32_t C,
                                    double *__restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double acc = 0.0;
  for (int32_t c = 0; c < C; ++c) acc += v[c];
  out[0] = acc;
}

struct BackwardArgs {
  const float *h, *x, *gs, *glogits;
  int32_t group, T;
  int64_t R;
  int32_t C, splits;
  NeuronP p;
  float *gI;
  double *partial;
  hipStream_t st;
  // snnqp_neuron_backward_state: `state` picks the window's kernel, which takes the three pointers
  bool state;
  const float *u0, *gu_T;
  float *gu0;
};

template <int KIND, int S>
int launch_backward(const BackwardArgs &a) {
  const int64_t blocks = ceil_div64((int64_t)a.splits * a.C, 256);
  if (a.state) {
    if (a.glogits)
      hipLaunchKernelGGL((neuron_backward_state_kernel<KIND, S, true>), dim3((unsigned)blocks),
                         dim3(256), 0, a.st, a.h, a.x, a.u0, a.gs, a.glogits, a.group, a.T, a.R, a.C,
                         a.splits, a.p, a.gu_T, a.gI, a.gu0, a.partial);
    else
      hipLaunchKernelGGL((neuron_backward_state_kernel<KIND, S, false>), dim3((unsigned)blocks),
                         dim3(256), 0, a.st, a.h, a.x, a.u0, a.gs, a.glogits, a.group, a.T, a.R, a.C,
                         a.splits, a.p, a.gu_T, a.gI, a.gu0, a.partial);
    SNNQP_CHECK_LAUNCH("neuron_backward_state_kernel");
    return SNNQP_OK;
  }
  if (a.glogits)
    hipLaunchKernelGGL((neuron_backward_kernel<KIND, S, true>), dim3((unsigned)blocks), dim3(256),
                       0, a.st, a.h, a.x, a.gs, a.glogits, a.group, a.T, a.R, a.C, a.splits, a.p,
                       a.gI, a.partial);
  else
    hipLaunchKernelGGL((neuron_backward_kernel<KIND, S, false>), dim3((unsigned)blocks), dim3(256),
                       0, a.st, a.h, a.x, a.gs, a.glogits, a.group, a.T, a.R, a.C, a.splits, a.p,
                       a.gI, a.partial);
  SNNQP_CHECK_LAUNCH("neuron_backward_kernel");
  return SNNQP_OK;
}

template <int KIND>
int launch_backward_surrogate(int surrogate, const BackwardArgs &a) {
  switch (surrogate) {
    case SNNQP_SURR_FAST_SIGMOID: return launch_backward<KIND, SNNQP_SURR_FAST_SIGMOID>(a);
    case SNNQP_SURR_ATAN: return launch_backward<KIND, SNNQP_SURR_ATAN>(a);
    case SNNQP_SURR_SLAYER: return launch_backward<KIND, SNNQP_SURR_SLAYER>(a);
    case SNNQP_SURR_SMOOTH_STEP: return launch_backward<KIND, SNNQP_SURR_SMOOTH_STEP>(a);
    default: return launch_backward<KIND, SNNQP_SURR_PIECEWISE_LINEAR>(a);
  }
}

bool known_surrogate(int s) {
  return s == SNNQP_SURR_FAST_SIGMOID || s == SNNQP_SURR_ATAN || s == SNNQP_SURR_SLAYER ||
         s == SNNQP_SURR_SMOOTH_STEP || s == SNNQP_SURR_PIECEWISE_LINEAR;
}

// PLIF / LIF, and LIF with its decays; multi_step_LIF has its own entry points
int check_kind(const snnqp_neuron_t *nrn, const char *who, const char *old_entry) {
  SNNQP_REQUIRE(nrn, SNNQP_EINVAL, "%s: null neuron", who);
  SNNQP_REQUIRE(nrn->kind != SNNQP_NEURON_MULTI_STEP_LIF, SNNQP_EUNSUPPORTED,
                "%s: multi_step_LIF has no parameter; its scan is %s", who, old_entry);
  SNNQP_REQUIRE(nrn->kind == SNNQP_NEURON_PARAMETRIC_LEAKY_IF || nrn->kind == SNNQP_NEURON_LIF,
                SNNQP_EUNSUPPORTED, "%s: neuron kind %d not supported", who, nrn->kind);
  SNNQP_REQUIRE(nrn->kind != SNNQP_NEURON_LIF || nrn->decay, SNNQP_EINVAL,
                "%s: LIF needs its per-feature decay", who);
  return SNNQP_OK;
}

int64_t range_groups(int32_t splits) { return splits > kGroup ? ceil_div64(splits, kGroup) : 0; }

int64_t workspace_doubles(int32_t C, int32_t splits, int kind) {
  // the partials [splits][C], the group sums [ceil(splits / 32)][C] when there are more than 32
  // ranges; PLIF: and the per-feature sums [C] the last kernel adds up
  return ((int64_t)splits + range_groups(splits) + (kind == SNNQP_NEURON_PARAMETRIC_LEAKY_IF ? 1 : 0)) * C;
}

}  // namespace
}  // namespace snnqp

using namespace snnqp;

extern "C" {

int snnqp_neuron_forward_save(const float *x, int32_t T, int64_t R, int32_t C,
                              const snnqp_neuron_t *nrn, float *h_out, float *s_out,
                              snnqp_stream_t stream) {
  SNNQP_REQUIRE(T >= 0 && R >= 0 && C > 0, SNNQP_EINVAL, "neuron_forward_save: bad shape");
  if (int rc = check_kind(nrn, "neuron_forward_save", "snnqp_lif_forward_save")) return rc;
  const int64_t n = R * C;
  if (n == 0 || T == 0) return SNNQP_OK;
  SNNQP_REQUIRE(x && h_out && s_out, SNNQP_EINVAL, "neuron_forward_save: null argument");
  const int64_t blocks = ceil_div64(n, 256);
  SNNQP_REQUIRE(blocks < (1ll << 31), SNNQP_EINVAL, "neuron_forward_save: grid too large");
  const NeuronP p = make_neuron(nrn);
  if (p.kind == SNNQP_NEURON_PARAMETRIC_LEAKY_IF)
    hipLaunchKernelGGL(neuron_save_kernel<SNNQP_NEURON_PARAMETRIC_LEAKY_IF>,
                       dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, T, n, C, p,
                       h_out, s_out);
  else
    hipLaunchKernelGGL(neuron_save_kernel<SNNQP_NEURON_LIF>, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, x, T, n, C, p, h_out, s_out);
  SNNQP_CHECK_LAUNCH("neuron_save_kernel");
  return SNNQP_OK;
}

int snnqp_neuron_backward_splits(int32_t T, int64_t R, int32_t C) {
  SNNQP_REQUIRE(T >= 0 && R >= 0 && C > 0, SNNQP_EINVAL, "neuron_backward_splits: bad shape");
  int64_t s = ceil_div64(kLanesAimed, C);
  if (s > R) s = R;
  if (s < 1) s = 1;
  SNNQP_REQUIRE(s * C <= (int64_t)INT32_MAX, SNNQP_EINVAL, "neuron_backward_splits: bad shape");
  return (int)s;
}

int64_t snnqp_neuron_backward_workspace_bytes(int32_t T, int64_t R, int32_t C, int32_t splits,
                                              int kind) {
  SNNQP_REQUIRE(T >= 0 && R >= 0 && C > 0, SNNQP_EINVAL,
                "neuron_backward_workspace_bytes: bad shape");
  SNNQP_REQUIRE(splits >= 1 && splits <= (R > 1 ? R : 1), SNNQP_EINVAL,
                "neuron_backward_workspace_bytes: splits %d outside 1..max(R, 1)", splits);
  SNNQP_REQUIRE(kind == SNNQP_NEURON_PARAMETRIC_LEAKY_IF || kind == SNNQP_NEURON_LIF,
                SNNQP_EUNSUPPORTED, "neuron_backward_workspace_bytes: neuron kind %d not supported",
                kind);
  return workspace_doubles(C, splits, kind) * (int64_t)sizeof(double);
}

// The host side of snnqp_neuron_backward (`state` false: u0, gu_T and gu0 are not looked at) and
// snnqp_neuron_backward_state; `who` names the entry in its refusals.
static int neuron_backward_host(const char *who, const char *old_entry, bool state, const float *h,
                                const float *x, const float *u0, const float *gs,
                                const float *glogits, int32_t group, int32_t T, int64_t R, int32_t C,
                                const snnqp_neuron_t *nrn, int surrogate, int32_t splits,
                                const float *gu_T, float *gI, float *gu0, double *gparam,
                                void *workspace, int64_t workspace_bytes, snnqp_stream_t stream) {
  SNNQP_REQUIRE(T >= 0 && R >= 0 && C > 0, SNNQP_EINVAL, "%s: bad shape", who);
  if (int rc = check_kind(nrn, who, old_entry)) return rc;
  SNNQP_REQUIRE((gs == nullptr) != (glogits == nullptr), SNNQP_EINVAL,
                "%s: exactly one of gs / glogits", who);
  SNNQP_REQUIRE(!glogits || (group > 0 && C % group == 0), SNNQP_EINVAL,
                "%s: %d features not divisible by group %d", who, C, group);
  SNNQP_REQUIRE(known_surrogate(surrogate), SNNQP_EINVAL, "%s: unknown surrogate %d", who,
                surrogate);
  SNNQP_REQUIRE(splits >= 1 && splits <= (R > 1 ? R : 1), SNNQP_EINVAL,
                "%s: splits %d outside 1..max(R, 1)", who, splits);
  const bool plif = nrn->kind == SNNQP_NEURON_PARAMETRIC_LEAKY_IF;
  const int64_t need = workspace_doubles(C, splits, nrn->kind) * (int64_t)sizeof(double);
  SNNQP_REQUIRE(workspace_bytes >= need, SNNQP_EINVAL, "%s: workspace of %lld bytes, %lld needed",
                who, (long long)workspace_bytes, (long long)need);
  SNNQP_REQUIRE(gparam, SNNQP_EINVAL, "%s: null argument", who);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nparam = plif ? 1 : C;
  if (R == 0 || T == 0) {                                            // zero sums, nothing launched
    SNNQP_HIP(hipMemsetAsync(gparam, 0, nparam * sizeof(double), st));
    if (state && gu0 && R > 0) {                                     // no step: gu0 = gu_T
      const size_t bytes = (size_t)(R * C) * sizeof(float);
      if (gu_T && gu_T != gu0)
        SNNQP_HIP(hipMemcpyAsync(gu0, gu_T, bytes, hipMemcpyDeviceToDevice, st));
      else if (!gu_T)
        SNNQP_HIP(hipMemsetAsync(gu0, 0, bytes, st));
    }
    return SNNQP_OK;
  }
  SNNQP_REQUIRE(h && gI && workspace && (x || !plif), SNNQP_EINVAL, "%s: null argument", who);
  const int64_t lanes = (int64_t)splits * C;
  SNNQP_REQUIRE(lanes <= (int64_t)INT32_MAX && ceil_div64(lanes, 256) < (1ll << 31), SNNQP_EINVAL,
                "%s: grid too large", who);
  double *partial = (double *)workspace;
  BackwardArgs a{h, x, gs, glogits, group, T, R, C, splits, make_neuron(nrn), gI, partial, st,
                 state, u0, gu_T, gu0};
  int rc = plif ? launch_backward_surrogate<SNNQP_NEURON_PARAMETRIC_LEAKY_IF>(surrogate, a)
                : launch_backward_surrogate<SNNQP_NEURON_LIF>(surrogate, a);
  if (rc) return rc;
  const int64_t groups = range_groups(splits);
  double *group_sums = partial + lanes;
  double *per_feature = plif ? group_sums + groups * C : gparam;
  const double *rows = partial;
  int32_t nrows = splits;
  if (groups) {
    hipLaunchKernelGGL(sum_ranges_kernel, dim3((unsigned)ceil_div64(groups * C, 256)), dim3(256), 0,
                       st, partial, splits, kGroup, C, group_sums);
    SNNQP_CHECK_LAUNCH("sum_ranges_kernel");
    rows = group_sums;
    nrows = (int32_t)groups;
  }
  hipLaunchKernelGGL(sum_ranges_kernel, dim3((unsigned)ceil_div64(C, 256)), dim3(256), 0, st, rows,
                     nrows, nrows, C, per_feature);
  SNNQP_CHECK_LAUNCH("sum_ranges_kernel");
  if (plif) {
    hipLaunchKernelGGL(sum_features_kernel, dim3(1), dim3(64), 0, st, per_feature, C, gparam);
    SNNQP_CHECK_LAUNCH("sum_features_kernel");
  }
  return SNNQP_OK;
}

int snnqp_neuron_backward(const float *h, const float *x, const float *gs, const float *glogits,
                          int32_t group, int32_t T, int64_t R, int32_t C,
                          const snnqp_neuron_t *nrn, int surrogate, int32_t splits, float *gI,
                          double *gparam, void *workspace, int64_t workspace_bytes,
                          snnqp_stream_t stream) {
  return neuron_backward_host("neuron_backward", "snnqp_lif_backward", false, h, x, nullptr, gs,
                              glogits, group, T, R, C, nrn, surrogate, splits, nullptr, gI, nullptr,
                              gparam, workspace, workspace_bytes, stream);
}

int snnqp_neuron_backward_state(const float *h, const float *x, const float *u0, const float *gs,
                                const float *glogits, int32_t group, int32_t T, int64_t R,
                                int32_t C, const snnqp_neuron_t *nrn, int surrogate, int32_t splits,
                                const float *gu_T, float *gI, float *gu0, double *gparam,
                                void *workspace, int64_t workspace_bytes, snnqp_stream_t stream) {
  return neuron_backward_host("neuron_backward_state", "snnqp_lif_backward_state", true, h, x, u0,
                              gs, glogits, group, T, R, C, nrn, surrogate, splits, gu_T, gI, gu0,
                              gparam, workspace, workspace_bytes, stream);
}

int snnqp_neuron_forward_save_state(const float *x, int32_t T, int64_t R, int32_t C,
                                    const snnqp_neuron_t *nrn, const float *u0, float *u_out,
                                    float *h_out, float *s_out, snnqp_stream_t stream) {
  SNNQP_REQUIRE(T >= 0 && R >= 0 && C > 0, SNNQP_EINVAL, "neuron_forward_save_state: bad shape");
  if (int rc = check_kind(nrn, "neuron_forward_save_state", "snnqp_lif_forward_save_state"))
    return rc;
  const int64_t n = R * C;
  if (n == 0 || (T == 0 && !u_out)) return SNNQP_OK;
  SNNQP_REQUIRE(T == 0 || (x && h_out && s_out), SNNQP_EINVAL,
                "neuron_forward_save_state: null argument");
  const int64_t blocks = ceil_div64(n, 256);
  SNNQP_REQUIRE(blocks < (1ll << 31), SNNQP_EINVAL, "neuron_forward_save_state: grid too large");
  const NeuronP p = make_neuron(nrn);
  // T == 0: the loop has no step, and the launch writes u_out = u0 (or zeros)
  if (p.kind == SNNQP_NEURON_PARAMETRIC_LEAKY_IF)
    hipLaunchKernelGGL(neuron_save_state_kernel<SNNQP_NEURON_PARAMETRIC_LEAKY_IF>,
                       dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, T, n, C, p, u0,
                       u_out, h_out, s_out);
  else
    hipLaunchKernelGGL(neuron_save_state_kernel<SNNQP_NEURON_LIF>, dim3((unsigned)blocks),
                       dim3(256), 0, (hipStream_t)stream, x, T, n, C, p, u0, u_out, h_out, s_out);
  SNNQP_CHECK_LAUNCH("neuron_save_state_kernel");
  return SNNQP_OK;
}

}  // extern "C"
