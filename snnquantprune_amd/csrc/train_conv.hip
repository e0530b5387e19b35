// Training of the conv blocks (ConvDenseSNN): the two gradient products of a 2-D convolution and
// the gradient routing of the 2x2 max pool.  All tensors float32, NHWC images, HWIO kernels.
//
//   snnqp_conv_weight_grad    gw[(kh KW + kw) Cin + ci][co] = sum_r x[n, oh sh + kh - pt,
//                             ow sw + kw - pl, ci] gI[r][co],  r = (n OH + oh) OW + ow
//   snnqp_conv_input_grad     gx[n, ih, iw, ci] = sum_r gI[n, oh, ow, co] w[kh, kw, ci, co],
//                             r = (kh KW + kw) Cout + co
//   snnqp_maxpool2x2_backward gp to the first maximum of each window
//
// Both products are grad_gemm.h's tile with gathering operands: the im2col matrix is never
// formed, a tap outside the image reads as the literal 0.0 and takes its place in the chain.
// The weight gradient's r can be cut into contiguous ranges, one workgroup each, summed by a
// second kernel in range order: no atomics, so the gradient is bitwise reproducible.
#include "common.h"
#include "grad_gemm.h"

namespace snnqp {
namespace {

struct ConvP {
  int32_t H, W, Cin, Cout, KH, KW, sh, sw, pt, pl, OH, OW;
};

// e = (img * n + rem) with 0 <= rem < n, n = rows * cols of one image, then rem = a * cols + b.
// Both divisions are 32-bit when e and n fit (every shipped shape); the 64-bit path keeps the
// index arithmetic right for any shape the host lets through.
__device__ __forceinline__ void split_pixel(int64_t e, int64_t n, int32_t cols, int64_t &img,
                                            int32_t &a, int32_t &b) {
  if (e < (1ll << 31) && n < (1ll << 31)) {
    const uint32_t q = (uint32_t)e / (uint32_t)n, rem = (uint32_t)e - q * (uint32_t)n;
    img = q;
    a = (int32_t)(rem / (uint32_t)cols);
    b = (int32_t)(rem - (uint32_t)a * (uint32_t)cols);
  } else {
    img = e / n;
    const int64_t rem = e - img * n;
    a = (int32_t)(rem / cols);
    b = (int32_t)(rem - (int64_t)a * cols);
  }
}

// i = (tap * C + c), tap = kh * KW + kw; i < 2^31 (check_geom).
__device__ __forceinline__ void split_tap(int64_t i, int32_t C, int32_t KW, int32_t &kh,
                                          int32_t &kw, int32_t &c) {
  const uint32_t tap = (uint32_t)i / (uint32_t)C;
  c = (int32_t)((uint32_t)i - tap * (uint32_t)C);
  kh = (int32_t)(tap / (uint32_t)KW);
  kw = (int32_t)(tap - (uint32_t)kh * (uint32_t)KW);
}

// A(r, i) of the weight gradient: r = (n, oh, ow), i = (kh, kw, ci).
struct XGather {
  const float *__restrict__ x;
  ConvP g;
  int64_t n;                                   // KH KW Cin
  static constexpr bool r_contig = false;
  __device__ __forceinline__ float at(int64_t r, int64_t i) const {
    if (i >= n) return 0.0f;
    int32_t kh, kw, ci, oh, ow;
    int64_t img;
    split_tap(i, g.Cin, g.KW, kh, kw, ci);
    split_pixel(r, (int64_t)g.OH * g.OW, g.OW, img, oh, ow);
    const int64_t ih = (int64_t)oh * g.sh + kh - g.pt, iw = (int64_t)ow * g.sw + kw - g.pl;
    if (ih < 0 || ih >= g.H || iw < 0 || iw >= g.W) return 0.0f;
    return x[((img * g.H + ih) * g.W + iw) * g.Cin + ci];
  }
};

// t / s when that is an integer in [0, n), else -1; t may be negative.
__device__ __forceinline__ int64_t exact_quotient(int64_t t, int32_t s, int32_t n) {
  if (t < 0) return -1;
  int64_t q;
  if (t < (1ll << 31)) {
    const uint32_t q32 = (uint32_t)t / (uint32_t)s;
    if (q32 * (uint32_t)s != (uint32_t)t) return -1;
    q = q32;
  } else {
    q = t / s;
    if (q * s != t) return -1;
  }
  return q < n ? q : -1;
}

// A(r, m) of the input gradient: r = (kh, kw, co), m = (n, ih, iw).
struct GIGather {
  const float *__restrict__ gI;
  ConvP g;
  int64_t n;                                   // NB H W
  static constexpr bool r_contig = true;
  __device__ __forceinline__ float at(int64_t r, int64_t m) const {
    if (m >= n) return 0.0f;
    int32_t kh, kw, co, ih, iw;
    int64_t img;
    split_tap(r, g.Cout, g.KW, kh, kw, co);
    split_pixel(m, (int64_t)g.H * g.W, g.W, img, ih, iw);
    const int64_t oh = exact_quotient((int64_t)ih + g.pt - kh, g.sh, g.OH);
    const int64_t ow = exact_quotient((int64_t)iw + g.pl - kw, g.sw, g.OW);
    if (oh < 0 || ow < 0) return 0.0f;
    return gI[((img * g.OH + oh) * g.OW + ow) * g.Cout + co];
  }
};

// B(r, ci) of the input gradient: w[kh, kw, ci, co].
struct WGather {
  const float *__restrict__ w;
  int32_t Cin, Cout;
  static constexpr bool r_contig = true;
  __device__ __forceinline__ float at(int64_t r, int64_t ci) const {
    if (ci >= Cin) return 0.0f;
    const uint32_t tap = (uint32_t)r / (uint32_t)Cout, co = (uint32_t)r - tap * (uint32_t)Cout;
    return w[((int64_t)tap * Cin + ci) * Cout + co];
  }
};

// blockIdx.z = the range s of r: rows [s L, min(Rn, (s + 1) L)) into out + s I J.
__global__ __launch_bounds__(256) void conv_wgrad_kernel(XGather a, gg::Strided b, int64_t Rn,
                                                         int64_t L, float *__restrict__ out) {
  const int64_t i0 = (int64_t)blockIdx.y * gg::GT, j0 = (int64_t)blockIdx.x * gg::GT;
  const int64_t I = a.n, J = b.n;
  const int64_t r_begin = (int64_t)blockIdx.z * L;
  const int64_t r_end = r_begin + L < Rn ? r_begin + L : Rn;
  float *__restrict__ c = out + (int64_t)blockIdx.z * I * J;
  gg::f32x4 acc[2][2];
  gg::tile_chain(a, b, i0, j0, r_begin, r_end, acc);
  gg::tile_store(acc, i0, j0, I, J, [&](int64_t i, int64_t j, float v) { c[i * J + j] = v; });
}

// gw = ((p0 + p1) + p2) + ... over the ranges' partial sums ws [splits][n].
__global__ void split_sum_kernel(const float *__restrict__ ws, int32_t splits, int64_t n,
                                 float *__restrict__ gw) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float v = ws[e];
  for (int32_t s = 1; s < splits; ++s) v = v + ws[(int64_t)s * n + e];
  gw[e] = v;
}

// The weight gradient accumulated in float64: one lane per element (i, co) of gw and range
// blockIdx.y of r, consecutive lanes on consecutive co (rows of gI coalesce, the gathered x is one
// address per i).  The product of two float32 values is exact in float64, so each step of the
// r-ascending chain rounds once, in the addition.
__global__ __launch_bounds__(256) void conv_wgrad_f64_kernel(XGather a, const float *__restrict__ gI,
                                                             int64_t J, int64_t Rn, int64_t L,
                                                             double *__restrict__ out) {
  const int64_t n = a.n * J;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int64_t i = e / J, j = e - i * J;
  const int64_t r_begin = (int64_t)blockIdx.y * L;
  const int64_t r_end = r_begin + L < Rn ? r_begin + L : Rn;
  double acc = 0.0;
  if (r_begin < r_end) {
    // the tap of this lane is fixed; (img, oh, ow) of r is split once and walked from there
    const ConvP &g = a.g;
    int32_t kh, kw, ci, oh, ow;
    int64_t img;
    split_tap(i, g.Cin, g.KW, kh, kw, ci);
    split_pixel(r_begin, (int64_t)g.OH * g.OW, g.OW, img, oh, ow);
    for (int64_t r = r_begin; r < r_end; ++r) {
      const int64_t ih = (int64_t)oh * g.sh + kh - g.pt, iw = (int64_t)ow * g.sw + kw - g.pl;
      const float xv = (ih < 0 || ih >= g.H || iw < 0 || iw >= g.W)
                           ? 0.0f
                           : a.x[((img * g.H + ih) * g.W + iw) * g.Cin + ci];
      acc = acc + (double)xv * (double)gI[r * J + j];
      if (++ow == g.OW) {
        ow = 0;
        if (++oh == g.OH) {
          oh = 0;
          ++img;
        }
      }
    }
  }
  out[(int64_t)blockIdx.y * n + e] = acc;
}

// gw = fl32(((p0 + p1) + p2) + ...) over the ranges' float64 partial sums ws [splits][n].
__global__ void split_sum_f64_kernel(const double *__restrict__ ws, int32_t splits, int64_t n,
                                     float *__restrict__ gw) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  double v = ws[e];
  for (int32_t s = 1; s < splits; ++s) v = v + ws[(int64_t)s * n + e];
  gw[e] = (float)v;
}

// blockIdx.x walks the pixels (the long axis), blockIdx.y the input channels.
__global__ __launch_bounds__(256) void conv_igrad_kernel(GIGather a, WGather b, int64_t Rn,
                                                         float *__restrict__ gx) {
  const int64_t i0 = (int64_t)blockIdx.x * gg::GT, j0 = (int64_t)blockIdx.y * gg::GT;
  const int64_t J = b.Cin;
  gg::f32x4 acc[2][2];
  gg::tile_chain(a, b, i0, j0, 0, Rn, acc);
  gg::tile_store(acc, i0, j0, a.n, J, [&](int64_t i, int64_t j, float v) { gx[i * J + j] = v; });
}

// One lane per element of gs [NB][H][W][C].  Window order (0,0), (0,1), (1,0), (1,1); a later
// position replaces the choice only when strictly greater, so ties go to the first.
__global__ void pool_backward_kernel(const float *__restrict__ s, const float *__restrict__ gp,
                                     int64_t n, int32_t H, int32_t W, int32_t C,
                                     float *__restrict__ gs) {
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
    float vb = s[base];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float v = s[base + off[k]];
      if (v > vb) {
        vb = v;
        best = k;
      }
    }
    if (best == (h & 1) * 2 + (w & 1)) out = gp[((img * PH + ph) * PW + pw) * C + c];
  }
  gs[e] = out;
}

// Decided on the host before any launch: what the gradient kernels serve.
int check_geom(const snnqp_conv_geom_t *g, const char *name, ConvP *p) {
  SNNQP_REQUIRE(g, SNNQP_EINVAL, "%s: null geometry", name);
  int32_t OH, OW;
  if (int rc = snnqp_conv_out_shape(g, &OH, &OW)) return rc;
  SNNQP_REQUIRE(g->H > 0 && g->W > 0 && g->Cin > 0 && g->Cout > 0, SNNQP_EINVAL,
                "%s: bad shape", name);
  SNNQP_REQUIRE(g->groups == 1 && g->in_dil_h == 1 && g->in_dil_w == 1 && g->k_dil_h == 1 &&
                    g->k_dil_w == 1,
                SNNQP_EUNSUPPORTED, "%s: groups == 1 and dilations 1 only", name);
  SNNQP_REQUIRE(g->pad_h_lo >= 0 && g->pad_h_hi >= 0 && g->pad_w_lo >= 0 && g->pad_w_hi >= 0,
                SNNQP_EUNSUPPORTED, "%s: negative padding", name);
  SNNQP_REQUIRE((int64_t)g->KH * g->KW < (1ll << 31) / g->Cin &&
                    (int64_t)g->KH * g->KW < (1ll << 31) / g->Cout,
                SNNQP_EINVAL, "%s: kernel too large", name);
  SNNQP_REQUIRE((double)g->H * g->W * g->Cin < 0x1p62 && (double)OH * OW * g->Cout < 0x1p62,
                SNNQP_EINVAL, "%s: image too large", name);
  *p = ConvP{g->H, g->W, g->Cin, g->Cout, g->KH, g->KW, g->stride_h, g->stride_w,
             g->pad_h_lo, g->pad_w_lo, OH, OW};
  return SNNQP_OK;
}

// NB images keep every element index inside int64.
bool images_fit(const ConvP &p, int64_t NB) {
  const double a = (double)p.H * p.W * p.Cin, b = (double)p.OH * p.OW * p.Cout;
  return NB >= 0 && (double)NB * (a > b ? a : b) < 0x1p62;
}

// The default number of ranges: tiles x splits near WG_TARGET workgroups (4 on each of 256 CUs),
// every range at least MIN_CHUNKS chunks of 16 rows, at most 64.  Shapes only.
constexpr int64_t WG_TARGET = 1024, MIN_CHUNKS = 16, MAX_SPLITS = 64;

int default_splits(const ConvP &p, int64_t NB) {
  const int64_t I = (int64_t)p.KH * p.KW * p.Cin;
  const int64_t tiles = ceil_div64(I, gg::GT) * ceil_div64(p.Cout, gg::GT);
  const int64_t chunks = ceil_div64(NB * p.OH * p.OW, gg::GR);
  int64_t s = ceil_div64(WG_TARGET, tiles);
  if (s > chunks / MIN_CHUNKS) s = chunks / MIN_CHUNKS;
  if (s > MAX_SPLITS) s = MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

// The ranges of the float64 weight gradient: about F64_ROWS rows each, at most F64_MAX_SPLITS (a
// lane walks its range row by row, so the ranges are what fills the machine).  Shapes only.
constexpr int64_t F64_ROWS = 1024, F64_MAX_SPLITS = 1024;

int f64_splits(int64_t Rn) {
  const int64_t s = ceil_div64(Rn, F64_ROWS);
  return s < 1 ? 1 : s > F64_MAX_SPLITS ? (int)F64_MAX_SPLITS : (int)s;
}

}  // namespace
}  // namespace snnqp

using namespace snnqp;

extern "C" {

int snnqp_conv_grad_splits(const snnqp_conv_geom_t *g, int64_t NB) {
  ConvP p;
  if (int rc = check_geom(g, "conv_grad_splits", &p)) return rc;
  SNNQP_REQUIRE(images_fit(p, NB), SNNQP_EINVAL, "conv_grad_splits: bad NB");
  return default_splits(p, NB);
}

int64_t snnqp_conv_weight_grad_workspace_bytes(const snnqp_conv_geom_t *g, int32_t splits) {
  ConvP p;
  if (int rc = check_geom(g, "conv_weight_grad_workspace_bytes", &p)) return rc;
  SNNQP_REQUIRE(splits >= 1 && splits <= MAX_SPLITS, SNNQP_EINVAL,
                "conv_weight_grad_workspace_bytes: splits %d outside 1..64", splits);
  if (splits == 1) return 0;
  return (int64_t)splits * p.KH * p.KW * p.Cin * p.Cout * (int64_t)sizeof(float);
}

int snnqp_conv_weight_grad(const float *x, const float *gI, int64_t NB,
                           const snnqp_conv_geom_t *g, int32_t splits, float *workspace,
                           float *gw, snnqp_stream_t stream) {
  ConvP p;
  if (int rc = check_geom(g, "conv_weight_grad", &p)) return rc;
  SNNQP_REQUIRE(images_fit(p, NB), SNNQP_EINVAL, "conv_weight_grad: bad NB");
  SNNQP_REQUIRE(splits >= 1 && splits <= MAX_SPLITS, SNNQP_EINVAL,
                "conv_weight_grad: splits %d outside 1..64", splits);
  const int64_t Rn = NB * p.OH * p.OW;
  if (Rn == 0) splits = 1;                     // zeros, straight into gw
  SNNQP_REQUIRE(gw && ((x && gI) || Rn == 0) && (workspace || splits == 1), SNNQP_EINVAL,
                "conv_weight_grad: null argument");
  const int64_t I = (int64_t)p.KH * p.KW * p.Cin, J = p.Cout;
  const int64_t gx = ceil_div64(J, gg::GT), gy = ceil_div64(I, gg::GT);
  SNNQP_REQUIRE(gx < (1ll << 31) && gy < 65536, SNNQP_EINVAL, "conv_weight_grad: grid too large");
  SNNQP_REQUIRE(ceil_div64(I * J, 256) < (1ll << 31), SNNQP_EINVAL,
                "conv_weight_grad: grid too large");
  const int64_t L = gg::GR * ceil_div64(ceil_div64(Rn, gg::GR), splits);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conv_wgrad_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)splits),
                     dim3(256), 0, st, XGather{x, p, I}, gg::make_strided(gI, J, 1, J), Rn, L,
                     splits == 1 ? gw : workspace);
  SNNQP_CHECK_LAUNCH("conv_wgrad_kernel");
  if (splits > 1) {
    hipLaunchKernelGGL(split_sum_kernel, dim3((unsigned)ceil_div64(I * J, 256)), dim3(256), 0, st,
                       workspace, splits, I * J, gw);
    SNNQP_CHECK_LAUNCH("split_sum_kernel");
  }
  return SNNQP_OK;
}

int64_t snnqp_conv_weight_grad_f64_workspace_bytes(const snnqp_conv_geom_t *g, int64_t NB) {
  ConvP p;
  if (int rc = check_geom(g, "conv_weight_grad_f64_workspace_bytes", &p)) return rc;
  SNNQP_REQUIRE(images_fit(p, NB), SNNQP_EINVAL, "conv_weight_grad_f64_workspace_bytes: bad NB");
  return (int64_t)f64_splits(NB * p.OH * p.OW) * p.KH * p.KW * p.Cin * p.Cout *
         (int64_t)sizeof(double);
}

int snnqp_conv_weight_grad_f64(const float *x, const float *gI, int64_t NB,
                               const snnqp_conv_geom_t *g, double *workspace, float *gw,
                               snnqp_stream_t stream) {
  ConvP p;
  if (int rc = check_geom(g, "conv_weight_grad_f64", &p)) return rc;
  SNNQP_REQUIRE(images_fit(p, NB), SNNQP_EINVAL, "conv_weight_grad_f64: bad NB");
  const int64_t Rn = NB * p.OH * p.OW;
  SNNQP_REQUIRE(gw && workspace && ((x && gI) || Rn == 0), SNNQP_EINVAL,
                "conv_weight_grad_f64: null argument");
  const int64_t I = (int64_t)p.KH * p.KW * p.Cin, J = p.Cout;
  const int64_t blocks = ceil_div64(I * J, 256);
  SNNQP_REQUIRE(blocks < (1ll << 31), SNNQP_EINVAL, "conv_weight_grad_f64: grid too large");
  const int splits = f64_splits(Rn);
  const int64_t L = ceil_div64(Rn, splits);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conv_wgrad_f64_kernel, dim3((unsigned)blocks, (unsigned)splits), dim3(256), 0,
                     st, XGather{x, p, I}, gI, J, Rn, L, workspace);
  SNNQP_CHECK_LAUNCH("conv_wgrad_f64_kernel");
  hipLaunchKernelGGL(split_sum_f64_kernel, dim3((unsigned)blocks), dim3(256), 0, st, workspace,
                     splits, I * J, gw);
  SNNQP_CHECK_LAUNCH("split_sum_f64_kernel");
  return SNNQP_OK;
}

int snnqp_conv_input_grad(const float *gI, const float *w, int64_t NB,
                          const snnqp_conv_geom_t *g, float *gx, snnqp_stream_t stream) {
  ConvP p;
  if (int rc = check_geom(g, "conv_input_grad", &p)) return rc;
  SNNQP_REQUIRE(images_fit(p, NB), SNNQP_EINVAL, "conv_input_grad: bad NB");
  if (NB == 0) return SNNQP_OK;
  SNNQP_REQUIRE(w && gx && (gI || p.OH == 0 || p.OW == 0), SNNQP_EINVAL,
                "conv_input_grad: null argument");
  const int64_t M = NB * p.H * p.W, Rn = (int64_t)p.KH * p.KW * p.Cout;
  const int64_t bx = ceil_div64(M, gg::GT), by = ceil_div64(p.Cin, gg::GT);
  SNNQP_REQUIRE(bx < (1ll << 31) && by < 65536, SNNQP_EINVAL, "conv_input_grad: grid too large");
  hipLaunchKernelGGL(conv_igrad_kernel, dim3((unsigned)bx, (unsigned)by), dim3(256), 0,
                     (hipStream_t)stream, GIGather{gI, p, M}, WGather{w, p.Cin, p.Cout}, Rn, gx);
  SNNQP_CHECK_LAUNCH("conv_igrad_kernel");
  return SNNQP_OK;
}

int snnqp_maxpool2x2_backward(const float *s, const float *gp, int64_t NB, int32_t H, int32_t W,
                              int32_t C, float *gs, snnqp_stream_t stream) {
  SNNQP_REQUIRE(NB >= 0 && H >= 0 && W >= 0 && C > 0, SNNQP_EINVAL,
                "maxpool2x2_backward: bad shape");
  SNNQP_REQUIRE((double)NB * H * W * C < 0x1p62, SNNQP_EINVAL, "maxpool2x2_backward: too large");
  const int64_t n = NB * H * W * C;
  if (n == 0) return SNNQP_OK;
  SNNQP_REQUIRE(s && gs && (gp || H < 2 || W < 2), SNNQP_EINVAL,
                "maxpool2x2_backward: null argument");
  const int64_t blocks = ceil_div64(n, 256);
  SNNQP_REQUIRE(blocks < (1ll << 31), SNNQP_EINVAL, "maxpool2x2_backward: grid too large");
  hipLaunchKernelGGL(pool_backward_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, s, gp, n, H, W, C, gs);
  SNNQP_CHECK_LAUNCH("pool_backward_kernel");
  return SNNQP_OK;
}

}  // extern "C"
