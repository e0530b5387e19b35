// Small device helpers the MFMA kernels share: vector types, LDS addressing, the LDS-only
// barrier, spike bits -> operand bytes / fp4 nibbles, int8 codes -> packed fp6.  gfx950 only.
#pragma once
#include "common.h"

namespace snnqp {

typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

// LDS accesses by absolute 32-bit LDS address (address space 3): the table reads
// take the MFMA result itself as the address, with no per-read base add.
typedef __attribute__((address_space(3))) const float lds_cfloat_t;
typedef __attribute__((address_space(3))) const uint8_t lds_cu8_t;
typedef __attribute__((address_space(3))) const uint32_t lds_cu32_t;
typedef __attribute__((address_space(3))) v4i lds_v4i_t;
__device__ __forceinline__ uint32_t lds_addr(const void *p) {
  return (uint32_t)(uintptr_t)(lds_cu8_t *)p;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also fences
// global memory, i.e. waits (vmcnt(0)) for the spike stores of the previous step
// and the prefetched halo loads -- a full memory round trip per timestep.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// the low 4 spike bits of w -> 4 bytes {0, 1}
__device__ __forceinline__ uint32_t expand4(uint32_t w) {
  return ((w & 0xFu) * 0x00204081u) & 0x01010101u;
}
// 16 spike bits -> 16 bytes {0, 1}
__device__ __forceinline__ v4i expand16(uint32_t b) {
  return v4i{(int)expand4(b), (int)expand4(b >> 4), (int)expand4(b >> 8), (int)expand4(b >> 12)};
}

// byte -> 8 fp4 nibbles (bit i set -> 1.0 = 0x2 in nibble i), 32 interleaved copies: entry e of
// copy c at dword 32 e + c, so lane l of a 32-lane group reads bank l whatever its byte is
// (ds_read_b32 banks: (a / 4) % 32)
constexpr int FP4_TAB_BYTES = 256 * 32 * 4;
__device__ __forceinline__ void fp4_table_fill(uint32_t *tab, int tid, int nthreads) {
  for (int i = tid; i < 256 * 32; i += nthreads) {
    const int e = i >> 5;
    uint32_t v = 0;
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) v |= ((e >> bit) & 1) ? (0x2u << (4 * bit)) : 0u;
    tab[i] = v;
  }
}
// this lane's copy of the table at LDS address `tab`
__device__ __forceinline__ uint32_t fp4_table_lane(uint32_t tab, int lane) {
  return tab + (uint32_t)(lane & 31) * 4;
}
// the entry of `byte` (< 256) in the copy `tabl` (fp4_table_lane): its 8 nibbles
__device__ __forceinline__ uint32_t fp4_table_entry(uint32_t tabl, uint32_t byte) {
  return *(lds_cu32_t *)(uintptr_t)((byte << 7) + tabl);
}

// 4 int8 codes (|c| <= 7) -> 4 e2m3 codes, one per byte
__device__ __forceinline__ uint32_t fp6_codes4(uint32_t x) {
  const uint32_t m1 = (x >> 7) & 0x01010101u;       // 1 where negative
  const uint32_t mag = (x ^ (m1 * 0xFFu)) + m1;     // |c| per byte (no carries)
  // magnitude 0..7 -> 0x00 0x08 0x10 0x14 0x18 0x1A 0x1C 0x1E (v_perm byte select)
  const uint32_t code = __builtin_amdgcn_perm(0x1E1C1A18u, 0x14100800u, mag);
  return code | (m1 << 5);
}

// four 6-bit codes in the bytes of c -> 24 contiguous bits
__device__ __forceinline__ uint32_t squeeze6(uint32_t c) {
  return (c & 0x3Fu) | ((c >> 2) & 0xFC0u) | ((c >> 4) & 0x3F000u) | ((c >> 6) & 0xFC0000u);
}

}  // namespace snnqp
