// Fused SpikingBlock(QuantDense, neuron) (spiking_learning.py:446-462 with
// flax_qdense.py:87 as the connection) on int8 MFMA: bit-packed spikes x int8
// codes -> int32 -> dequantise -> [BatchNorm] -> neuron over T -> packed spikes.
// A second instantiation (IN = SNNQP_U8) reads uint8 rows as they are -- the [B, T, K]
// event-count input of a dense-only model (config C2) -- with no packing pass and no
// inspection of the values: a byte x enters the MFMA as the int8 x - 128 (x ^ 0x80, exact
// for every count 0..255) and 128 * sum_k w[k][n] (snnqp_weight_t.col_sum) is added back to
// the int32 accumulator.
//
// The connection is stateless across t, so the contraction is one GEMM over
// rows m = (sample, t); only the neuron is sequential:
//  * a workgroup owns SB samples x all T steps (<= RT*32 rows) and a block of 128
//    output features; it is 8 waves = two groups of 4 (32 features per wave) that
//    split K: group g walks the chunks c = g (mod 2) with its own LDS buffers, and the
//    int32 partial tiles are added once at the end;
//  * K is walked in chunks of 256: the rows' spike bits are expanded to {0,1}
//    bytes in LDS (row stride 256 B, 16-byte chunks XOR-swizzled by row so the
//    ds_read_b128 of an A fragment is conflict-free); the B fragments stream
//    from the MFMA-tiled codes (snnqp_pack_codes_mfma: one contiguous 1 KiB
//    read per wave and k-step) straight into registers and are reused by the
//    RT row tiles; spike words and B fragments are requested three chunks ahead of
//    their use (register rings, counted s_waitcnt), and inside a chunk every wave
//    interleaves its MFMAs with its share of the loads and of the next chunk's
//    expansion, slot by slot (fused_chunk);
//  * after the K loop the int32 tile goes through LDS once so that each thread
//    gets the T currents of one (sample, feature) pair in order, runs the
//    neuron with u in a register and ballots the spikes into 32-bit words.
#include <cstdlib>
#include <type_traits>

#include "dense_tile.h"

namespace snnqp {

constexpr int BK = 256;          // k per chunk (bytes per LDS row)
constexpr int KSC = BK / 32;     // MFMA k-steps per chunk

struct DenseMfmaArgs {
  const uint32_t *x;             // bit-packed rows (words) or uint8 rows (bytes)
  const int32_t *col_sum;        // U8 input: sum over k of the codes of each feature
  int64_t xs_t, xs_b;            // word (bits) / byte (u8) strides
  int32_t T, B, K, N, KS, SB;    // KS = ceil(K / 32), SB samples per workgroup
  const int8_t *wt;              // MFMA-tiled codes [Npad/32][KS][64][16]
  Dequant dq;
  BnP bn;
  NeuronP nrn;
  const float *u0;
  float *u_out;
  uint32_t *s_out;
};

// (the barriers order LDS traffic only, lds_barrier: the K loop keeps the next chunk's global
// loads in flight across them)
__device__ __forceinline__ int a_addr(int row, int c16) {
  return row * BK + ((c16 ^ (row & 15)) << 4);
}

constexpr int KGROUPS = 2;       // wave groups splitting K

template <int RT, int IN>
__global__ void __launch_bounds__(256 * KGROUPS)
dense_mfma_kernel(DenseMfmaArgs a) {
  constexpr bool U8 = IN == SNNQP_U8;
  constexpr int ROWS = RT * 32;
  // staging tasks of a row and chunk: one 32-bit spike word -> 32 bytes, or one 16-byte piece
  // of uint8 counts -> the same 16 bytes ^ 0x80
  constexpr int WPR = U8 ? BK / 16 : BK / 32;
  typedef typename std::conditional<U8, v4i, uint32_t>::type stg_t;
  constexpr int NTASK = ROWS * WPR;
  constexpr int TPT = (NTASK + 255) / 256;
  // two A buffers per group; the epilogue tile (ROWS x 128 int32) overlays them
  constexpr int ABYTES = ROWS * BK;
  constexpr int EBYTES = ROWS * 128 * 4;
  constexpr int LDSB = (2 * KGROUPS * ABYTES > EBYTES) ? 2 * KGROUPS * ABYTES : EBYTES;
  __shared__ __attribute__((aligned(16))) uint8_t lds[LDSB];

  // (group and wave indices in scalar registers: so are the addresses of the B fragments)
  const int grp = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);   // K group of this wave
  const int tid = threadIdx.x & 255, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint8_t *abuf = lds + grp * 2 * ABYTES;
  const int n = lane & 31, h = lane >> 5;
  const int b0 = blockIdx.x * a.SB;
  const int nsamp = min(a.SB, a.B - b0);
  const int rows = nsamp * a.T;                   // live rows of this workgroup
  const int nb = blockIdx.y * 4 + wave;           // 32-column block of this wave
  const bool wave_on = nb * 32 < a.N;
  const int nchunks = (a.KS + KSC - 1) / KSC;      // chunk j of this group = 2 j + grp

  v16i acc[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
    acc[r] = v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

  // Global loads run D - 1 chunks ahead of their use, in rings of D register sets (spike
  // words and B fragments): a chunk of MFMAs is about 0.3 us of a wave, a loaded global round
  // trip several times that -- with one chunk of lookahead the K loop ran at the pace of the
  // memory latency, not of the matrix pipe or of LDS.  (uint8 rows stage four times the
  // registers per chunk: one chunk less of lookahead.)
  constexpr int D = U8 ? 3 : 4;
  constexpr int U = D % 2 ? 2 * D : D;             // unroll: ring slot i % D, LDS buffer i & 1
  stg_t stgr[D][TPT];
  // staging tasks: word wi of row `row`, the same (row, wi) for every chunk; the loads of the K
  // loop are unconditional, clamped addresses and the value dropped afterwards (dense_tile.h)
  uint32_t roff[TPT];                              // word / byte offset within this workgroup's samples
  uint32_t rmask[TPT];
  const uint32_t *xw = a.x + (U8 ? 0 : (int64_t)b0 * a.xs_b);
  const uint8_t *xbytes = (const uint8_t *)a.x + (U8 ? (int64_t)b0 * a.xs_b : 0);
#pragma unroll
  for (int k = 0; k < TPT; ++k) {
    const RowTask rt = row_task<WPR>(tid + k * 256, tid + k * 256 < NTASK, rows, a.T, a.xs_t, a.xs_b);
    roff[k] = rt.off; rmask[k] = rt.mask;
  }
  auto chunk_word = [&](int chunk, int k) { return (chunk * KGROUPS + grp) * WPR + (tid + k * 256) % WPR; };
  // uint8: 16-byte piece `chunk_word` of the row; K is a multiple of 16 (launch check).  Pieces
  // beyond K re-read the row's first one and are stored as zero bytes (the k-steps of a chunk
  // beyond K reuse the last real k-step's codes); the rows beyond `rows` need no masking,
  // nothing reads their accumulators
  auto stage_load1 = [&](int chunk, int k) -> stg_t {
    if constexpr (U8) {
      const int piece = chunk_word(chunk, k);
      return *(const v4i *)(xbytes + roff[k] + (uint32_t)(piece * 16 < a.K ? piece * 16 : 0));
    } else {
      return xw[roff[k] + (uint32_t)min(chunk_word(chunk, k), a.KS - 1)];
    }
  };
  auto stage_load = [&](stg_t (&stg)[TPT], int chunk) {
#pragma unroll
    for (int k = 0; k < TPT; ++k) stg[k] = stage_load1(chunk, k);
  };
  // the words of dead rows and of k beyond K are zeroed here, by masks (a select next to the
  // load would put its wait there)
  auto stage_store = [&](const stg_t (&stg)[TPT], int chunk, int buf) {
    uint8_t *base = abuf + buf * ABYTES;
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
      const int task = tid + k * 256;
      if (task < NTASK) {
        const int row = task / WPR, wi = task % WPR;
        if constexpr (U8) {
          const v4i v = stg[k];
          const int m = chunk_word(chunk, k) * 16 < a.K ? -1 : 0;
          *(v4i *)(base + a_addr(row, wi)) =
              v4i{(v.x ^ (int)0x80808080) & m, (v.y ^ (int)0x80808080) & m,
                  (v.z ^ (int)0x80808080) & m, (v.w ^ (int)0x80808080) & m};
        } else {
          const uint32_t wv = bit_word_masked(stg[k], rmask[k], chunk_word(chunk, k), a.KS);   // KS = words of a row
          *(v4i *)(base + a_addr(row, wi * 2)) = expand16(wv & 0xFFFFu);
          *(v4i *)(base + a_addr(row, wi * 2 + 1)) = expand16(wv >> 16);
        }
      }
    }
  };

  // B fragments of a whole chunk (KSC k-steps) are prefetched into registers next to the A
  // words of that chunk
  const v4i *wtile = (const v4i *)a.wt + ((int64_t)(wave_on ? nb : 0) * a.KS) * 64;   // wave-uniform
  v4i bfr[D][KSC];
  auto load_b = [&](v4i (&bf)[KSC], int chunk) {
#pragma unroll
    for (int ks = 0; ks < KSC; ++ks) {
      // (k-steps beyond K meet zero A bytes: any codes do)
      const int kg = min((chunk * KGROUPS + grp) * KSC + ks, a.KS - 1);
      bf[ks] = (wtile + (int64_t)kg * 64)[lane];
    }
  };
  // One chunk of the K loop, as NSLOT = KSC * RT slots: slot s issues MFMA s of chunk c, the
  // A-fragment read of slot s + PF, and an even share of everything else the iteration has to
  // do -- the global loads of chunk c + D - 1 and the expansion of the spike words of chunk
  // c + 1 into the other LDS buffer (one dword of 4 bytes per piece: bit field, multiply, mask).
  // Vector instructions only overlap the matrix pipe when the SAME wave issues them between
  // its MFMAs: with the chunk as "all MFMAs, then all staging" the two never co-executed
  // (SQ_VALU_MFMA_COEXEC_CYCLES 2 % of the MFMA-busy cycles, each of MFMA / VALU / LDS busy a
  // third of the time), whichever way the two waves of a SIMD were phased.
  constexpr int NSLOT = KSC * RT;
  constexpr int PF = 3;                               // A fragments in flight
  constexpr int LSTEP = NSLOT / TPT;                  // slots between two staging loads
  static_assert(NSLOT % TPT == 0 && LSTEP >= 2, "one staging load every LSTEP slots");
  constexpr int PPT = U8 ? 4 : 8;                     // dwords a staging task expands to
  constexpr int NPIECE = TPT * PPT;                   // dwords the thread expands per chunk
  // loop-invariant LDS offsets: fragment reads (per k-step; row tile and buffer are immediates)
  // and the 16-byte stores of each staging task
  int rd_off[KSC];
#pragma unroll
  for (int ks = 0; ks < KSC; ++ks) rd_off[ks] = a_addr(n, ks * 2 + h);
  int wr_off[TPT][2];
#pragma unroll
  for (int k = 0; k < TPT; ++k) {
    const int task = tid + k * 256;
    const int row = task < NTASK ? task / WPR : 0, wi = task % WPR;
    wr_off[k][0] = U8 ? a_addr(row, wi) : a_addr(row, wi * 2);
    wr_off[k][1] = U8 ? 0 : a_addr(row, wi * 2 + 1);
  }
  auto frag = [&](int rbuf, int s) -> v4i {
    return *(const v4i *)(abuf + rbuf * ABYTES + (s % RT) * 32 * BK + rd_off[s / RT]);
  };
  auto fused_chunk = [&](int rbuf, const v4i (&bf)[KSC], stg_t (&ld_stg)[TPT], v4i (&ld_bf)[KSC],
                         int ld_chunk, const stg_t (&st_stg)[TPT], int st_chunk) {
    v4i av[PF + 1];
#pragma unroll
    for (int s = 0; s < PF; ++s) av[s] = frag(rbuf, s);
    stg_t wv[TPT];
    int inK[TPT];                      // uint8: all ones while the piece lies inside K
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
      inK[k] = -1;
      if constexpr (U8) {
        wv[k] = st_stg[k];
        inK[k] = chunk_word(st_chunk, k) * 16 < a.K ? -1 : 0;
      } else {
        wv[k] = bit_word_masked(st_stg[k], rmask[k], chunk_word(st_chunk, k), a.KS);
      }
    }
    v4i ex = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      // (a wave beyond N multiplies block 0's codes into accumulators nobody reads)
      acc[s % RT] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[s % (PF + 1)], bf[s / RT], acc[s % RT], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (s + PF < NSLOT) av[(s + PF) % (PF + 1)] = frag(rbuf, s + PF);
      // global loads of the chunk D - 1 ahead: one B fragment per row-tile round, the spike
      // words in the first slots
      if (s % RT == 0) {
        const int ks = s / RT;
        const int kg = min((ld_chunk * KGROUPS + grp) * KSC + ks, a.KS - 1);
        ld_bf[ks] = (wtile + (int64_t)kg * 64)[lane];
      }
      if (s % LSTEP == 1 && s / LSTEP < TPT) {
        const int k = s / LSTEP;
        ld_stg[k] = stage_load1(ld_chunk, k);
      }
      // expansion pieces p with p * NSLOT / NPIECE == s
#pragma unroll
      for (int p = 0; p < NPIECE; ++p) {
        if (p * NSLOT / NPIECE == s) {
          const int k = p / PPT, d = p & 3;
          // the word passes through an empty volatile asm in every slot that expands a piece
          // of it: the piece cannot be computed before its slot (sched_barrier alone orders
          // instructions, not the values they were selected from)
          if constexpr (U8) {
            asm volatile("" : "+v"(wv[k]));
            ex[d] = (wv[k][d] ^ (int)0x80808080) & inK[k];
            if (d == 3 && tid + k * 256 < NTASK)
              *(v4i *)(abuf + (rbuf ^ 1) * ABYTES + wr_off[k][0]) = ex;
          } else {
            const int hf = (p / 4) & 1;
            asm volatile("" : "+v"(wv[k]));
            ex[d] = (int)expand4(wv[k] >> (16 * hf + 4 * d));
            if (d == 3 && tid + k * 256 < NTASK)
              *(v4i *)(abuf + (rbuf ^ 1) * ABYTES + wr_off[k][hf]) = ex;
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // chunks beyond K contribute zero A bytes (any codes do), so the loop runs over groups of U
  // chunks without a tail case
#pragma unroll
  for (int d = 0; d < D - 1; ++d) {
    stage_load(stgr[d], d);
    load_b(bfr[d], d);
  }
  stage_store(stgr[0], 0, 0);
  lds_barrier();
  const int ngc = (nchunks + KGROUPS - 1) / KGROUPS;     // chunks per group
  for (int c = 0; c < ngc; c += U) {
#pragma unroll
    for (int i = 0; i < U; ++i) {                        // chunk c + i: ring slot i % D, LDS buffer i & 1
      fused_chunk(i & 1, bfr[i % D], stgr[(i + D - 1) % D], bfr[(i + D - 1) % D], c + i + D - 1,
                  stgr[(i + 1) % D], c + i + 1);
      lds_barrier();
    }
  }

  // int32 tile -> LDS [row][128], then one (sample, feature) pair per thread (dense_tile.h);
  // uint8 input: 128 * sum_k w[k][feat] is added back (the x - 128 operand)
  int *et = (int *)lds;
  dense_tile_merge<RT, KGROUPS>(et, acc, grp, wave, n, h, wave_on);
  dense_tile_neurons<U8>(et, a.col_sum, a.dq, a.bn, a.nrn, a.T, a.B, a.N, a.SB, b0, nsamp, a.u0, a.u_out,
                         a.s_out, 256 * KGROUPS);
}

const char *dense_codes_unsupported(const BlockCall &c, int in_type) {
  if (c.w->wtype != SNNQP_W_I8) return "weights are not int8 codes";
  if (!c.wt) return "MFMA-tiled codes `wt` not given";
  if (in_type != SNNQP_BITS && in_type != SNNQP_U8) return "input must be bit-packed or uint8";
  if (c.s_type != SNNQP_BITS) return "spike output must be bit-packed";
  if (in_type == SNNQP_U8) {
    // uint8 rows are read in 16-byte pieces, as x - 128 against the int8 codes
    if (!c.w->col_sum) return "uint8 input needs snnqp_weight_t.col_sum";
    if (c.K % 16) return "uint8 input needs K % 16 == 0";
    if (c.K > 65536) return "uint8 input needs K <= 65536 (int32 accumulator)";
  }
  // bit-packed: any K -- the tiles `wt` are zero-padded to ceil(K / 32) k-steps and the packed
  // input rows carry zero bits beyond K
  if (c.nrn->kind == SNNQP_NEURON_LIF && !c.nrn->decay) return "LIF without decay";
  return nullptr;
}

const char *dense_mfma_unsupported(const BlockCall &c) {
  if (const char *why = dense_codes_unsupported(c, c.in_type)) return why;
  if (c.T > (c.in_type == SNNQP_U8 ? 64 : 96))
    return "more than 96 (uint8 input: 64) timesteps (one sample must fit a row tile)";
  // 32-bit word offsets from the workgroup's first sample (at most 96); a row: ceil(K / 32) units of any type
  const int rows = dense_rows_broken(c, c.in_type, 96, c.T > 0 ? c.T - 1 : 0, (c.K + 31) / 32);
  if (rows & ROWS_UNALIGNED) return "uint8 rows not 16-byte aligned";
  if (rows) return "input strides beyond 32-bit word offsets within a workgroup";
  return nullptr;
}

template <int RT, int IN>
static void launch_dense(const DenseMfmaArgs &a, unsigned gx, unsigned gy, hipStream_t st) {
  hipLaunchKernelGGL((dense_mfma_kernel<RT, IN>), dim3(gx, gy), dim3(256 * KGROUPS), 0, st, a);
}

// The launch of T x B rows, N wide: what run_dense_mfma launches and what snnqp_dense_mfma_plan
// reports.  No GPU call.  The largest row tile that still gives the chip enough workgroups, else the
// smallest one that holds a whole sample (most workgroups); uint8 rows: at most 64 rows (their
// staging ring takes the registers of the third row tile).  SNNQP_DENSE_MFMA_RT=1..3 forces the
// row tiles where they hold a sample: a measurement knob, read on every call.
struct DenseMfmaPlan { int rt, sb; unsigned gx, gy; };
static DenseMfmaPlan plan_dense_mfma(bool u8, int32_t T, int32_t B, int32_t N) {
  DenseMfmaPlan p = {};
  p.gy = (unsigned)((N + 127) / 128);
  static const int rts[3] = {3, 2, 1};
  for (int i = u8 ? 1 : 0; i < 3; ++i) {
    const int sb = rts[i] * 32 / T;
    if (sb < 1) continue;
    p.rt = rts[i];
    if ((int64_t)((B + sb - 1) / sb) * p.gy >= 200) break;
  }
  if (const char *e = std::getenv("SNNQP_DENSE_MFMA_RT")) {
    const int forced = std::atoi(e);
    if (forced >= 1 && forced <= (u8 ? 2 : 3) && 32 * forced >= T) p.rt = forced;
  }
  if (p.rt > 0) {
    p.sb = p.rt * 32 / T;
    p.gx = (unsigned)((B + p.sb - 1) / p.sb);
  }
  return p;
}

int run_dense_mfma(const BlockCall &c) {
  if (int rc = block_entry("dense mfma", c, true)) return rc < 0 ? rc : SNNQP_OK;
  const int32_t T = c.T, B = c.B, N = c.N;
  const bool u8 = c.in_type == SNNQP_U8;
  if (u8)
    SNNQP_REQUIRE(((uintptr_t)c.x & 15) == 0 && c.xs_t % 16 == 0 && c.xs_b % 16 == 0, SNNQP_EUNSUPPORTED,
                  "dense mfma: uint8 rows must be 16-byte aligned");
  DenseMfmaArgs a;
  fill_block_args(a, c);
  a.K = c.K; a.N = N; a.KS = (c.K + 31) / 32;
  a.wt = c.wt; a.col_sum = c.w->col_sum;
  const DenseMfmaPlan p = plan_dense_mfma(u8, T, B, N);
  SNNQP_REQUIRE(p.rt > 0, SNNQP_EUNSUPPORTED, "dense mfma: T too large");
  const int rt = p.rt;
  const unsigned gx = p.gx, gy = p.gy;
  a.SB = p.sb;
  if (u8) {
    if (rt == 2) launch_dense<2, SNNQP_U8>(a, gx, gy, c.st);
    else launch_dense<1, SNNQP_U8>(a, gx, gy, c.st);
  } else {
    switch (rt) {
      case 3: launch_dense<3, SNNQP_BITS>(a, gx, gy, c.st); break;
      case 2: launch_dense<2, SNNQP_BITS>(a, gx, gy, c.st); break;
      default: launch_dense<1, SNNQP_BITS>(a, gx, gy, c.st); break;
    }
  }
  SNNQP_CHECK_LAUNCH("dense_mfma_kernel");
  return SNNQP_OK;
}

}  // namespace snnqp

extern "C" int snnqp_dense_mfma_plan(int in_type, int32_t T, int32_t B, int32_t N, int32_t *rt, int32_t *sb,
                                     int32_t *gx, int32_t *gy) {
  using namespace snnqp;
  SNNQP_REQUIRE(rt && sb && gx && gy, SNNQP_EINVAL, "dense_mfma_plan: null argument");
  SNNQP_REQUIRE(in_type == SNNQP_BITS || in_type == SNNQP_U8, SNNQP_EINVAL,
                "dense_mfma_plan: input must be bit-packed or uint8");
  SNNQP_REQUIRE(T >= 1 && B >= 1 && N >= 1, SNNQP_EINVAL, "dense_mfma_plan: bad sizes");
  const bool u8 = in_type == SNNQP_U8;
  SNNQP_REQUIRE(T <= (u8 ? 64 : 96), SNNQP_EUNSUPPORTED,
                "dense_mfma_plan: more than 96 (uint8 input: 64) timesteps (one sample must fit a row tile)");
  const DenseMfmaPlan p = plan_dense_mfma(u8, T, B, N);
  *rt = p.rt; *sb = p.sb; *gx = (int32_t)p.gx; *gy = (int32_t)p.gy;
  return SNNQP_OK;
}
