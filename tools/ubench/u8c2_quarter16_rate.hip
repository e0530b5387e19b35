// The event layer's quarter of the half group (the wave spread), one wave-step of it in
// two forms, to see whether the 16x16x64 matrix instruction is the cheaper way to 4 registers of product:
//   FORM 32  v_mfma_i32_32x32x32_i8 from a 16-register C of which registers 0..3 are defined and read
//            (what the spread instance issues today)
//   FORM 16  v_mfma_i32_16x16x64_i8 from a 4-register C
// The timed sequence is the kernel's dependent chain: two 8-byte fragment reads -> matrix instruction
// from a C operand that carries the table address -> 4 table gathers -> 4 neuron updates (two packed
// pairs).  Three placements:
//   ALONE   the quarter and nothing else
//   BEHIND  a whole own tile first (reads -> 32x32x32 from C = 0 -> 16 gathers -> 16 updates, the
//           tile-step of u8c2_tile_rate.hip), then the quarter: the spread instance's order
//   AHEAD   the quarter's reads and matrix instruction issued before the own tile's epilogue, its
//           gathers and updates behind it: the order the 4-register form would make room for
// at 4, 5 and 6 waves per SIMD (workgroups of four waves, one per SIMD, as the kernel's).  Plain LDS
// reads and matrix instructions on an array the workgroup owns; one float per thread is stored.
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float v2f __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v16i __attribute__((ext_vector_type(16)));

enum { ALONE = 0, BEHIND = 1, AHEAD = 2 };

__device__ __forceinline__ void update_pair(v2f &u, v2f x, v2f kv, float th, unsigned &word, int j) {
  v2f t;
  unsigned long long m0, m1;
  asm volatile("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(t) : "v"(x), "v"(u));
  asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(t) : "v"(t), "v"(kv), "v"(u));
  asm volatile("v_cmp_le_f32_e64 %0, %1, %2" : "=s"(m0) : "v"(th), "v"(t.x));
  asm volatile("v_cmp_le_f32_e64 %0, %1, %2" : "=s"(m1) : "v"(th), "v"(t.y));
  asm volatile("v_cndmask_b32_e64 %0, %1, 0, %2" : "=v"(u.x) : "v"(t.x), "s"(m0));
  asm volatile("v_cndmask_b32_e64 %0, %1, 0, %2" : "=v"(u.y) : "v"(t.y), "s"(m1));
  const unsigned long long m = m0 | m1;
  const unsigned w = (unsigned)m | (unsigned)(m >> 32);
  asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(word) : "s"(w), "n"(0));
}

constexpr int TABLE_F = 4096, IMG_W = 2048;

template <int FORM, int PLACE, int WPS>
__global__ void __launch_bounds__(256, WPS) k(float *out, int iters, float kk, float th) {
  // one array: the table at LDS offset 0 (an accumulator IS a table address), the A image behind it
  __shared__ __attribute__((aligned(16))) float smem[TABLE_F + IMG_W];
  float *table = smem;
  int *img = (int *)(smem + TABLE_F);
  for (int i = threadIdx.x; i < TABLE_F; i += 256) table[i] = 0.25f + (i & 7) * 0.125f;
  for (int i = threadIdx.x; i < IMG_W; i += 256) img[i] = 0;      // product = C: every address in the table
  __syncthreads();
  const int lane = threadIdx.x & 63;
  v2f u[8], uq[2];
  for (int i = 0; i < 8; ++i) u[i] = v2f{0.01f * lane, 0.02f * i};
  for (int i = 0; i < 2; ++i) uq[i] = v2f{0.03f * lane, 0.05f * i};
  const v2f kv = {kk, kk};
  unsigned word = 0;
  const v4i bw = {0x04040404, 0x04040404, 0x04040404, 0x04040404};
  const unsigned tb = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)table;   // 0
  const unsigned ib = (unsigned)(uintptr_t)(__attribute__((address_space(3))) int *)img + lane * 8;
  // the quarter's C: this lane's table entry, 32 distinct banks in either 32-lane half
  const int ctab = (int)tb + (lane & 31) * 4 + (lane >> 5) * 128;

  for (int it = 0; it < iters; ++it) {
    int ctab0 = ctab;
    asm volatile("" : "+v"(ctab0));
    int q4[4];
    auto quarter_mfma = [&]() {
      v2i lo, hi;
      asm volatile("ds_read_b64 %0, %1 offset:2048" : "=v"(lo) : "v"(ib));
      asm volatile("ds_read_b64 %0, %1 offset:2072" : "=v"(hi) : "v"(ib));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (FORM == 16) {
        v4i acc = {ctab0, ctab0, ctab0, ctab0};
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(v4i{lo.x, lo.y, hi.x, hi.y}, bw, acc, 0, 0, 0);
        asm volatile("" : "+v"(acc));
#pragma unroll
        for (int i = 0; i < 4; ++i) q4[i] = acc[i];
      } else {
        const v4i c4 = {ctab0, ctab0, ctab0, ctab0};
        v16i acc = __builtin_shufflevector(c4, c4, 0, 1, 2, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4i{lo.x, lo.y, hi.x, hi.y}, bw, acc, 0, 0, 0);
        asm volatile("" : "+v"(acc));
#pragma unroll
        for (int i = 0; i < 4; ++i) q4[i] = acc[i];
      }
    };
    auto quarter_epilogue = [&]() {
      float xr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) asm volatile("ds_read_b32 %0, %1" : "=v"(xr[i]) : "v"((unsigned)q4[i]));
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(2 - 2 * j) : "memory");
        v2f x = v2f{xr[2 * j], xr[2 * j + 1]};
        asm volatile("" : "+v"(x));
        update_pair(uq[j], x, kv, th, word, j);
      }
    };
    if (PLACE == ALONE) {
      quarter_mfma();
      quarter_epilogue();
    } else {
      // the own tile: reads -> MFMA from C = 0 -> 16 gathers, consumed pair by pair -> 16 updates
      v2i lo, hi;
      asm volatile("ds_read_b64 %0, %1" : "=v"(lo) : "v"(ib));
      asm volatile("ds_read_b64 %0, %1 offset:1024" : "=v"(hi) : "v"(ib));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4i{lo.x, lo.y, hi.x, hi.y}, bw, acc, 0, 0, 0);
      asm volatile("" : "+v"(acc));
      if (PLACE == AHEAD) quarter_mfma();
      float xr[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("ds_read_b32 %0, %1" : "=v"(xr[i]) : "v"(tb + (unsigned)acc[i]));
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(14 - 2 * j) : "memory");
        v2f x = v2f{xr[2 * j], xr[2 * j + 1]};
        asm volatile("" : "+v"(x));
        update_pair(u[j], x, kv, th, word, j);
      }
      if (PLACE == BEHIND) quarter_mfma();
      quarter_epilogue();
    }
  }
  float s = (float)word;
  for (int i = 0; i < 8; ++i) s += u[i].x + u[i].y;
  for (int i = 0; i < 2; ++i) s += uq[i].x + uq[i].y;
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int FORM, int PLACE, int WPS>
double run(float *out) {
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  const int iters = 10000; float ms = 0, best = 1e30f;
  for (int rep = 0; rep < 3; ++rep) {           // the first launch warms up; the faster of the other two
    (void)hipEventRecord(e0);
    hipLaunchKernelGGL((k<FORM, PLACE, WPS>), dim3(256 * WPS), dim3(256), 0, 0, out, iters, 0.5f, 1.0f);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1); (void)hipEventElapsedTime(&ms, e0, e1);
    if (rep > 0 && ms < best) best = ms;
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return best * 1e6 / ((double)iters * WPS) * 2.4;    // SIMD cycles per wave-step at 2.4 GHz
}

template <int PLACE, int WPS>
void row(const char *name, float *out) {
  const double c32 = run<32, PLACE, WPS>(out), c16 = run<16, PLACE, WPS>(out);
  printf("%-34s %d waves/SIMD: 32x32x32 %7.1f   16x16x64 %7.1f   difference %6.1f SIMD cycles per wave-step\n",
         name, WPS, c32, c16, c32 - c16);
}

template <int PLACE>
void rows(const char *name, float *out) {
  row<PLACE, 4>(name, out);
  row<PLACE, 5>(name, out);
  row<PLACE, 6>(name, out);
}

int main() {
  float *out;
  if (hipMalloc(&out, 256 * 6 * 256 * 4) != hipSuccess) { printf("no device memory\n"); return 1; }
  printf("one wave-step of the half group's quarter, SIMD cycles at 2.4 GHz (256 CUs x WPS workgroups of 4 waves)\n");
  rows<ALONE>("quarter alone", out);
  rows<BEHIND>("own tile, then the quarter", out);
  rows<AHEAD>("quarter's MFMA ahead of the tile", out);
  if (hipDeviceSynchronize() != hipSuccess) { printf("device error\n"); return 1; }
  (void)hipFree(out);
  return 0;
}
