// What the two gated ('gint') connections (conv_gated.hip, dense_gated.hip) and their packers
// share: the fp6 encoders, the two-digit form of wide codes, the packer of the code operand, and
// the matrix instruction and store value of the main kernels.  gfx950 only.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace snnqp {

// integer -7..7 -> fp6 e2m3 (bias 1, four significant bits: every integer up to 7 is exact)
__host__ __device__ inline uint32_t fp6_e2m3(int v) {
  const uint32_t tab[8] = {0u, 8u, 16u, 20u, 24u, 26u, 28u, 30u};
  return tab[v < 0 ? -v : v] | (v < 0 ? 32u : 0u);
}
// integer -8..8 -> fp6 e3m2 (bias 3, three significant bits: every integer up to 8 is exact;
// 1 = 0x0C, 2 = 0x10, 3 = 0x12, 4 = 0x14, 5 = 0x15, 6 = 0x16, 7 = 0x17, 8 = 0x18)
__host__ __device__ inline uint32_t fp6_e3m2(int v) {
  const uint32_t tab[9] = {0x00u, 0x0Cu, 0x10u, 0x12u, 0x14u, 0x15u, 0x16u, 0x17u, 0x18u};
  return tab[v < 0 ? -v : v] | (v < 0 ? 0x20u : 0u);
}

// Codes up to 7 are one e2m3 value (the narrow form); the wide form serves the rest:
// Codes beyond e2m3 (|code| <= 127: up to 8 bits) as TWO six-bit digits, code = 16 hi + lo with lo in
// [-8, 7], hi in [-8, 8] -- exact in the OTHER fp6 format, e3m2 -- one digit per 32-deep K block of
// the 64-deep instruction: the block scale of the second block is 2^4 (v_mfma_scale: an E8M0 scale
// per lane half = per K block), so ONE instruction returns sum(lo s) + 16 sum(hi s): the exact
// integer, at the fp6 rate and with not one vector instruction more than the narrow form.  (fp8
// digits work too -- tools/ubench/mfma_fp8_kmap.hip, mfma_fp8_digits.hip: an 8-bit operand beside a
// 4-bit one counts k differently, the digits then sit in bytes 0..8 / 16..24 of the lanes of half 0
// -- and were the first version: twice the matrix-pipe time and eight operand dwords, 2.09 ms for
// CextNet's 8-bit layer against 1.38 with e3m2.)  The lanes of half 0 hold the lo digits of a
// column's K elements, the lanes of half 1 the hi digits; the spike operand holds the same K
// elements in both lane halves.
inline bool gated_wide(int32_t code_max) { return code_max > 7; }
// the digit of `code` for K block h: lo (h = 0) or hi (h = 1)
__host__ __device__ inline int gated_digit(int code, int h) {
  const int lo = ((code + 8) & 15) - 8;
  return h ? (code - lo) / 16 : lo;
}
// f(std::true_type / std::false_type): the run-time form as a template argument
template <typename F>
inline void gated_form(bool wide, F f) {
  if (wide) f(std::true_type{});
  else f(std::false_type{});
}

// six-bit value e at bits [6 slot, 6 slot + 6) of a record of DW dwords (slot < 32 DW / 6); a
// value may straddle two dwords
template <int DW>
__device__ __forceinline__ void fp6_put(uint32_t (&d)[DW], int slot, uint32_t e) {
  const int k = (6 * slot) >> 5, sh = (6 * slot) & 31;
  d[k] |= e << sh;
  if (sh > 26) d[k + 1] |= e >> (32 - sh);
}

// The code operand of a gated kernel: out[c][ot][lane][DW], lane (n, h) = column o = 32 ot + n of
// channel c, K block h; columns beyond NO are zero.  SRC says where the source keeps code (r, c, o)
// of the R codes a (channel, column) pair has -- at(r, c, o) -- and where the narrow form puts it:
// six-bit slot slot(r) of the lane of half half(r).  Wide: digit h of code r in slot r.
template <int DW, bool WIDE, typename SRC>
__global__ void __launch_bounds__(256)
pack_codes_gated_kernel(const int8_t *w, SRC src, int32_t C, int32_t R, int32_t NO, int32_t OT, uint32_t *out) {
  const int64_t total = (int64_t)C * OT * 64;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int lane = (int)(i & 63), n = lane & 31, h = lane >> 5;
    const int ot = (int)((i >> 6) % OT), c = (int)((i >> 6) / OT);
    const int o = ot * 32 + n;
    uint32_t d[DW] = {};
    if (o < NO) {
      for (int r = 0; r < R; ++r) {
        const int code = w[src.at(r, c, o)];
        if (WIDE) fp6_put(d, r, fp6_e3m2(gated_digit(code, h)));
        else if (src.half(r) == h) fp6_put(d, src.slot(r), fp6_e2m3(code));
      }
    }
    for (int j = 0; j < DW; ++j) out[i * DW + j] = d[j];
  }
}

// the launch of the above for codes up to code_max; `name` opens the message of a failed launch
template <int DW, typename SRC>
int pack_codes_gated(const char *name, const int8_t *w, SRC src, int32_t C, int32_t R, int32_t NO,
                     int32_t code_max, void *packed, hipStream_t st) {
  const int OT = (NO + 31) / 32;
  const int64_t blocks = ((int64_t)C * OT * 64 + 255) / 256;
  gated_form(gated_wide(code_max), [&](auto wide) {
    hipLaunchKernelGGL((pack_codes_gated_kernel<DW, decltype(wide)::value, SRC>),
                       dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, w, src, C, R, NO, OT,
                       (uint32_t *)packed);
  });
  SNNQP_CHECK_LAUNCH(name);
  return SNNQP_OK;
}

// ---- the main kernels ---------------------------------------------------------------------------
// operand formats of v_mfma_scale_f32_32x32x64_f8f6f4 (cbsz / blgp)
enum { MFMA_E2M3 = 2, MFMA_E3M2 = 3, MFMA_FP4 = 4 };

__device__ __forceinline__ v16f gated_zero16() { return v16f{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

// E8M0 scale of the code operand's K block h, from the lanes of half h: 2^0, wide: 2^4 on the hi digits
template <bool WIDE>
__device__ __forceinline__ int gated_scale(int h) { return WIDE ? (h ? 131 : 127) : 127; }

// the exact integer sums of one (32 x 32, K = 64) tile from C = 0: fp4 spikes against fp6 codes
// (CODES_A: the codes are the A operand), `scale` = gated_scale<WIDE>(h)
template <bool WIDE, bool CODES_A>
__device__ __forceinline__ v16f gated_mfma(v8i A, v8i B, int scale) {
  constexpr int codes = WIDE ? MFMA_E3M2 : MFMA_E2M3;
  if constexpr (CODES_A)
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, gated_zero16(), codes, MFMA_FP4, 0, scale, 0, 127);
  else
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, gated_zero16(), MFMA_FP4, codes, 0, 127, 0, scale);
}

// C/D layout: lane (n, h) holds column n; its register i is this row of a tile whose rows start at row0
__device__ __forceinline__ int gated_acc_row(int i, int h, int row0 = 0) {
  return row0 + (i & 3) + 8 * (i >> 2) + 4 * h;
}

// current = fl(fl(acc / L) * m)
__device__ __forceinline__ float gated_current(float acc, float L, float m) {
  const float q = acc / L;
  return q * m;
}

}  // namespace snnqp
