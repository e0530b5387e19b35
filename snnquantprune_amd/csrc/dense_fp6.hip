// Fused SpikingBlock(QuantDense, neuron) (spiking_learning.py:446-462 with flax_qdense.py:87
// as the connection) for codes of magnitude <= 7 (DuQ up to 4 bits, quant.py:443,467) on the
// block-scaled f8f6f4 MFMA: bit-packed spikes as fp4 (e2m1: 0 / 1.0) x codes as fp6 (e2m3:
// every integer up to 7 exact) -> float32 sums of integers below 2^24, i.e. the same integer
// the int8 kernel (dense_mfma.hip) accumulates -> dequantise -> [BatchNorm] -> neuron over T
// -> packed spikes.  Against the int8 formulation: K = 64 per MFMA at twice the rate (a
// quarter of the matrix time), the codes PACKED at 6 bits in HBM / L2 (snnqp_pack_codes_fp6:
// three quarters of the bytes every workgroup streams), and the spike bits expanded through
// a byte -> 8-nibble LDS table (one lookup per 8 spikes; bits -> bytes took three vector
// instructions per 4 spikes).
//
// Same decomposition as dense_mfma.hip: a workgroup owns SB samples x all T steps (<= RT * 32
// rows) and 128 output features; 8 waves = two groups of 4 (32 features per wave) that split
// K (group g walks the chunks c = g mod 2, own LDS buffers; the partial tiles are added once
// at the end -- exact: integers).  K is walked in chunks of 256: the rows' spike words become
// 128 bytes of fp4 per row in LDS (16-byte pieces XOR-swizzled by row: the ds_read_b128 of an
// A fragment is conflict-free), the B fragments (24 bytes per lane and k-step) stream from the
// fp6 tiles into registers and are reused by the RT row tiles.  A chunk is only 4 RT MFMAs, so
// the K loop must not drain at its barrier: THREE A buffers per group -- chunk c computes from
// buffer c mod 3 while the words of chunk c + 2 are expanded into buffer (c + 2) mod 3, so the
// barrier at the end of chunk c publishes a buffer that is first read a whole chunk later, and
// the first fragments of chunk c + 1 are requested BEFORE that barrier (its wait is counted:
// it retires the chunk's LDS writes, not the fragments in flight).  Spike words are requested
// four chunks ahead, B fragments two (register rings of three), and every wave interleaves its
// MFMAs with its share of the loads and of the expansion, slot by slot.
#include <cstdlib>

#include "dense_tile.h"

namespace snnqp {

namespace {

constexpr int F6_BK = 256;            // k per chunk
constexpr int F6_KSC = F6_BK / 64;    // MFMA k-steps per chunk
constexpr int F6_ROWB = F6_BK / 2;    // LDS bytes of a row per chunk (fp4)
constexpr int F6_TAB = FP4_TAB_BYTES;  // byte -> 8 fp4 nibbles (tile_util.h)
constexpr int F6_KGROUPS = 2;
constexpr int F6_TILE = 1536;         // bytes of one B tile: 64 lanes x (16 + 8)

struct DenseFp6Args {
  const uint32_t *x;
  int64_t xs_t, xs_b;            // word strides
  int32_t T, B, K, N, KW, KS, SB;   // KW = ceil(K / 32) words per row, KS = ceil(K / 64) k-steps
  const uint8_t *wt6;            // fp6 tiles [Npad/32][KS][1536] (snnqp_pack_codes_fp6)
  Dequant dq;
  BnP bn;
  NeuronP nrn;
  const float *u0;
  float *u_out;
  uint32_t *s_out;
  // K split over workgroups (blockIdx.z): partial tiles and tickets in a caller-owned workspace
  int32_t ksplit, gcz;           // workgroups per tile; group-chunks of one of them
  uint32_t *tickets;             // [tiles], zeroed on the stream in front of every launch (handoff_arm)
  float *slabs;                  // [tiles][ksplit][ROWS * 128]
  uint32_t *status;              // the device's status word (runtime.hip), or null
};

static_assert(F6_ROWB == 128, "the A images are swz128_addr's rows (dense_tile.h)");

}  // namespace

// fp6 tiles of a dense kernel: for the 32-column block nb and the 64-deep k-step ks, lane
// l = (n & 31) + 32 h holds the codes of k = 64 ks + 32 h + j (j < 32) of column
// n = 32 nb + (l & 31) as e2m3 values, value j at bits [6 j, 6 j + 6) of six dwords; the tile
// stores dwords 0..3 of the 64 lanes (1 KiB), then dwords 4..5 (512 B): two coalesced reads
// per wave and k-step.  Rows beyond K and columns beyond N are zero codes.
__global__ void __launch_bounds__(256)
pack_codes_fp6_kernel(const int8_t *__restrict__ w, int64_t K, int32_t N, int32_t Npad,
                      uint32_t *__restrict__ wt6) {
  const int64_t KS = (K + 63) / 64;
  const int64_t total = (int64_t)(Npad / 32) * KS * 64;          // one thread per (tile, lane)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(i & 63);
    const int64_t tile = i >> 6;
    const int64_t ks = tile % KS, nb = tile / KS;
    const int64_t n = nb * 32 + (lane & 31);
    const int64_t k0 = ks * 64 + 32 * (lane >> 5);
    uint32_t t[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      uint32_t x = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t k = k0 + 4 * q + j;
        const int c = (n < N && k < K) ? (int)w[k * N + n] : 0;
        x |= (uint32_t)(uint8_t)c << (8 * j);
      }
      t[q] = squeeze6(fp6_codes4(x));
    }
    uint32_t d[6];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      d[3 * g + 0] = t[4 * g] | (t[4 * g + 1] << 24);
      d[3 * g + 1] = (t[4 * g + 1] >> 8) | (t[4 * g + 2] << 16);
      d[3 * g + 2] = (t[4 * g + 2] >> 16) | (t[4 * g + 3] << 8);
    }
    uint32_t *tb = wt6 + tile * (F6_TILE / 4);
    tb[lane * 4 + 0] = d[0]; tb[lane * 4 + 1] = d[1]; tb[lane * 4 + 2] = d[2]; tb[lane * 4 + 3] = d[3];
    tb[256 + lane * 2 + 0] = d[4]; tb[256 + lane * 2 + 1] = d[5];
  }
}

template <int RT>
__global__ void __launch_bounds__(256 * F6_KGROUPS)
dense_fp6_kernel(DenseFp6Args a) {
  constexpr int ROWS = RT * 32;
  constexpr int WPR = F6_BK / 32;                 // spike words per row per chunk
  constexpr int NTASK = ROWS * WPR;
  constexpr int TPT = NTASK / 256;                // = RT
  static_assert(TPT == RT, "one spike word per thread and row tile");
  constexpr int ABYTES = ROWS * F6_ROWB;
  constexpr int EBYTES = ROWS * 128 * 4;
  constexpr int NBUF = 3;                         // A buffers of a group (see the header)
  constexpr int WORK = (NBUF * F6_KGROUPS * ABYTES > EBYTES) ? NBUF * F6_KGROUPS * ABYTES : EBYTES;
  __shared__ __attribute__((aligned(128))) uint8_t lds[F6_TAB + WORK];
  uint8_t *work = lds + F6_TAB;

  const int grp = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);   // K group of this wave
  const int tid = threadIdx.x & 255, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint8_t *abuf = work + grp * NBUF * ABYTES;
  const int n = lane & 31, h = lane >> 5;
  const int b0 = blockIdx.x * a.SB;
  const int nsamp = min(a.SB, a.B - b0);
  const int rows = nsamp * a.T;                   // live rows of this workgroup
  const int nb = blockIdx.y * 4 + wave;           // 32-column block of this wave
  const bool wave_on = nb * 32 < a.N;
  const int nchunks = (a.KS + F6_KSC - 1) / F6_KSC;   // chunk j of this group = 2 j + grp
  const int ngc_all = (nchunks + F6_KGROUPS - 1) / F6_KGROUPS;  // chunks per group over all of K
  // K split over workgroups: this one walks the group-chunks [gc0, gc0 + ngc)
  const int gc0 = a.ksplit > 1 ? (int)blockIdx.z * a.gcz : 0;
  const int ngc = a.ksplit > 1 ? max(0, min(a.gcz, ngc_all - gc0)) : ngc_all;
  // Every workgroup streams the same code tiles.  Walking K in the same order, all of them ask
  // for the same lines at the same time; the sums are exact integers, so the walk may start
  // anywhere: step `lc` of the loop is chunk (lc + rot) mod ngc, with one `rot` per XCD
  // (blockIdx.x mod 8 under the observed round-robin placement -- a speed assumption only).
  // The workgroups of an XCD still share each tile in its L2 (measured HBM-side traffic 106 MB
  // against 104 MB unrotated; a rotation per WORKGROUP thrashes the 4 MiB L2 with 32 different
  // tiles at a time: 162 MB), the eight XCDs no longer hit the same memory channels together:
  // 0.072 ms against 0.078.
  const int rot = (int)(((blockIdx.x & 7u) * (unsigned)ngc) >> 3);
  auto phys = [&](int lc) -> int {     // loop step -> this group's chunk; steps beyond ngc: a dead chunk
    const int pc = lc + rot >= ngc ? lc + rot - ngc : lc + rot;
    return lc < ngc ? gc0 + pc : nchunks;
  };

  // the byte -> 8 nibbles table, at the start of LDS
  fp4_table_fill((uint32_t *)lds, threadIdx.x, 256 * F6_KGROUPS);
  const uint32_t tabl = fp4_table_lane(lds_addr(lds), lane);

  v16f acc[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
    acc[r] = v16f{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

  // rings of D = 3 register sets, slot = chunk mod 3 like the LDS buffer: the spike words of
  // chunk c + 4 are requested while those of c + 2 are expanded (c + 3 waits), the B fragments
  // of chunk c + 2 while those of c are multiplied (c + 1 waits)
  constexpr int D = 3;
  uint32_t stgr[D][TPT];
  uint32_t roff[TPT], rmask[TPT];
  const uint32_t *xw = a.x + (int64_t)b0 * a.xs_b;
#pragma unroll
  for (int k = 0; k < TPT; ++k) {
    const RowTask rt = row_task<WPR>(tid + k * 256, true, rows, a.T, a.xs_t, a.xs_b);   // NTASK = 256 TPT
    roff[k] = rt.off; rmask[k] = rt.mask;
  }
  // word `chunk_word` of the row; words beyond K re-read the row's last one and are masked
  auto chunk_word = [&](int chunk, int k) { return (chunk * F6_KGROUPS + grp) * WPR + (tid + k * 256) % WPR; };
  auto stage_load1 = [&](int chunk, int k) -> uint32_t {
    return xw[roff[k] + (uint32_t)min(chunk_word(chunk, k), a.KW - 1)];
  };
  auto masked = [&](uint32_t w, int chunk, int k) -> uint32_t {
    return bit_word_masked(w, rmask[k], chunk_word(chunk, k), a.KW);
  };
  auto lookup = [&](uint32_t w, int d) -> int {
    return (int)fp4_table_entry(tabl, (w >> (8 * d)) & 0xFFu);
  };
  int wr_off[TPT];
#pragma unroll
  for (int k = 0; k < TPT; ++k) {
    const int task = tid + k * 256;
    wr_off[k] = swz128_addr(task / WPR, task % WPR);
  }

  const uint8_t *wtile = a.wt6 + ((int64_t)(wave_on ? nb : 0) * a.KS) * F6_TILE;   // wave-uniform
  int bfr[D][F6_KSC][6];
  auto load_b1 = [&](int (&bf)[6], int chunk, int ks) {
    // (k-steps beyond K meet zero A nibbles: any codes do)
    const int kg = min((chunk * F6_KGROUPS + grp) * F6_KSC + ks, a.KS - 1);
    const uint8_t *tb = wtile + (int64_t)kg * F6_TILE;
    const v4i lo = ((const v4i *)tb)[lane];
    const v2i hi = ((const v2i *)(tb + 1024))[lane];
    bf[0] = lo.x; bf[1] = lo.y; bf[2] = lo.z; bf[3] = lo.w; bf[4] = hi.x; bf[5] = hi.y;
  };

  constexpr int NSLOT = F6_KSC * RT;                  // MFMAs of one chunk
  constexpr int PF = 3;                               // A fragments in flight
  int rd_off[F6_KSC];
#pragma unroll
  for (int ks = 0; ks < F6_KSC; ++ks) rd_off[ks] = swz128_addr(n, ks * 2 + h);
  auto frag = [&](int rbuf, int s) -> v4i {
    // row tile s % RT: 32 rows further (the swizzle repeats every 16 rows)
    return *(const v4i *)(abuf + rbuf * ABYTES + (s % RT) * 32 * F6_ROWB + rd_off[s / RT]);
  };
  // One chunk as NSLOT slots: slot s issues MFMA s and the A-fragment read of slot s + PF --
  // which, in the last PF slots, is fragment s + PF - NSLOT of the NEXT chunk, from its own
  // buffer -- plus an even share of the chunk's other work: the global loads (spike words of
  // chunk c + 4, B fragments of chunk c + 2) and, in the slots before the last PF, the table
  // lookups / LDS writes that expand the spike words of chunk c + 2 into buffer (c + 2) mod 3.
  constexpr int NPIECE = TPT * 5;                     // per word: 4 lookups, 1 write
  constexpr int XSLOT = NSLOT - PF;                   // slots that carry expansion pieces
  static_assert(NSLOT % (PF + 1) == 0, "the fragment ring keeps its phase from chunk to chunk");
  v4i av[PF + 1];
  auto fused_chunk = [&](int rbuf, const int (&bf)[F6_KSC][6], uint32_t (&ld_stg)[TPT], int ld_schunk,
                         int (&ld_bf)[F6_KSC][6], int ld_bchunk, const uint32_t (&st_stg)[TPT],
                         int st_chunk) {
    const int nbuf = rbuf == NBUF - 1 ? 0 : rbuf + 1, wbuf = nbuf == NBUF - 1 ? 0 : nbuf + 1;
    uint32_t wv[TPT];
#pragma unroll
    for (int k = 0; k < TPT; ++k) wv[k] = masked(st_stg[k], st_chunk, k);
    v4i ex = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const v4i af = av[s % (PF + 1)];
      const int ks = s / RT;
      acc[s % RT] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
          v8i{af.x, af.y, af.z, af.w, 0, 0, 0, 0},
          v8i{bf[ks][0], bf[ks][1], bf[ks][2], bf[ks][3], bf[ks][4], bf[ks][5], 0, 0}, acc[s % RT],
          4 /* A: fp4 */, 2 /* B: fp6 */, 0, 127, 0, 127);
      __builtin_amdgcn_sched_barrier(0);
      if (s + PF < NSLOT) av[(s + PF) % (PF + 1)] = frag(rbuf, s + PF);
      else av[(s + PF) % (PF + 1)] = frag(nbuf, s + PF - NSLOT);
      if (s % RT == 0) load_b1(ld_bf[s / RT], ld_bchunk, s / RT);
      if (s % F6_KSC == 1 && s / F6_KSC < TPT) ld_stg[s / F6_KSC] = stage_load1(ld_schunk, s / F6_KSC);
#pragma unroll
      for (int p = 0; p < NPIECE; ++p) {
        if (p * XSLOT / NPIECE == s) {
          const int k = p / 5, d = p % 5;
          asm volatile("" : "+v"(wv[k]));
          if (d < 4) ex[d] = lookup(wv[k], d);
          else *(v4i *)(abuf + wbuf * ABYTES + wr_off[k]) = ex;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    chunk_barrier<PF>();                            // publishes buffer wbuf
  };

  lds_barrier();                                  // the table is visible
  // prologue: words of chunks 0..3, B fragments of chunks 0..1 requested; chunks 0 and 1 expanded
#pragma unroll
  for (int d = 0; d < D; ++d) {
#pragma unroll
    for (int k = 0; k < TPT; ++k) stgr[d][k] = stage_load1(phys(d), k);
  }
#pragma unroll
  for (int d = 0; d < 2; ++d) {
#pragma unroll
    for (int ks = 0; ks < F6_KSC; ++ks) load_b1(bfr[d][ks], phys(d), ks);
  }
#pragma unroll
  for (int d = 0; d < 2; ++d) {
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
      const uint32_t w = masked(stgr[d][k], phys(d), k);
      *(v4i *)(abuf + d * ABYTES + wr_off[k]) = v4i{lookup(w, 0), lookup(w, 1), lookup(w, 2), lookup(w, 3)};
    }
  }
  // (ring slots 0 and 1 are free again: chunk 3 goes to slot 0 now, chunk 4 to slot 1 in step 0)
#pragma unroll
  for (int k = 0; k < TPT; ++k) stgr[0][k] = stage_load1(phys(3), k);
  lds_barrier();
#pragma unroll
  for (int s = 0; s < PF; ++s) av[s] = frag(0, s);
  for (int c = 0; c < ngc; c += D) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      // step c + i: compute from buffer i, B slot i; request the words of chunk c + i + 4 into
      // slot (i + 1) % 3 and the B fragments of chunk c + i + 2 into slot (i + 2) % 3; expand
      // the words of chunk c + i + 2 (slot (i + 2) % 3) into buffer (i + 2) % 3
      fused_chunk(i, bfr[i], stgr[(i + 1) % D], phys(c + i + 4), bfr[(i + 2) % D], phys(c + i + 2),
                  stgr[(i + 2) % D], phys(c + i + 2));
    }
  }
  lds_barrier();                                  // every wave is done with the A buffers

  // partial tiles -> LDS [row][128] as float (exact integers; dense_tile.h)
  float *et = (float *)work;
  dense_tile_merge<RT, F6_KGROUPS>(et, acc, grp, wave, n, h, wave_on);

  // K split over workgroups: every workgroup of a tile leaves its partial tile (exact integers
  // in float32) in its slab; the last arriver adds the others' slabs to its own tile and goes on
  // to the neuron (the hand-over of dense_tile.h)
  if (a.ksplit > 1) {
    typedef unsigned long long u64;
    const int tile = blockIdx.y * gridDim.x + blockIdx.x;
    u64 *mine = (u64 *)(a.slabs + ((int64_t)tile * a.ksplit + blockIdx.z) * (ROWS * 128));
    const u64 *et64 = (const u64 *)et;
    handoff_publish(mine, ROWS * 64, 256 * F6_KGROUPS, [&](int i) { return et64[i]; });
    // (the flag: the byte -> nibble table is no longer needed)
    if (!handoff_last_arriver(a.tickets + tile, (uint32_t)a.ksplit, a.status, (uint32_t *)lds)) return;
    for (int z = 0; z < a.ksplit; ++z) {
      if (z == (int)blockIdx.z) continue;
      const u64 *other = (const u64 *)(a.slabs + ((int64_t)tile * a.ksplit + z) * (ROWS * 128));
      for (int i = threadIdx.x; i < ROWS * 64; i += 256 * F6_KGROUPS) {
        const u64 o = __hip_atomic_load(other + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        et[2 * i] += __uint_as_float((uint32_t)o);
        et[2 * i + 1] += __uint_as_float((uint32_t)(o >> 32));
      }
    }
    __syncthreads();
  }

  dense_tile_neurons<false>(et, nullptr, a.dq, a.bn, a.nrn, a.T, a.B, a.N, a.SB, b0, nsamp, a.u0, a.u_out,
                            a.s_out, 256 * F6_KGROUPS);
}

template <int RT>
static void launch_dense_fp6(const DenseFp6Args &a, unsigned gx, unsigned gy, hipStream_t st) {
  hipLaunchKernelGGL((dense_fp6_kernel<RT>), dim3(gx, gy, (unsigned)(a.ksplit > 1 ? a.ksplit : 1)),
                     dim3(256 * F6_KGROUPS), 0, st, a);
}

// Rows of a workgroup and workgroups per tile along K.  A workgroup streams the code matrix of
// its K range through its CU's vector L1, which is what bounds this kernel: more row tiles
// amortise that stream, but only while the grid still covers the chip; a split of K over `ks`
// workgroups per tile (partial tiles and tickets in a caller workspace, the last arriver of a
// tile runs the neuron) fills the chip when the batch alone does not.  The model behind the
// choice, in microseconds at K = 32768, fitted to the read-out (T = 20): a launch takes (rounds of
// workgroups over the 256 CUs) x (11 + (9.5 + 15.5 RT) / ks) -- B = 1024 unsplit: RT 3 / 4 / 5 =
// 0.067 / 0.084 / 0.098 ms -- plus, when split, the hand-over, 6 + 0.09 per KB of slab moved.
// Measured (write-through hand-over): B = 16 / 64 / 100 split (RT 1, ks 4) 0.025 / 0.027 / 0.031 ms
// against 0.042 / 0.043 / 0.044 unsplit; B = 1024 forced to (RT 5, ks 2) 0.071, (3, 2) 0.080,
// (5, 4) 0.096 against 0.066 unsplit -- with more rows per workgroup the per-k cost of a workgroup
// (fragment reads, expansion, MFMAs per row tile) grows as fast as the stream shrinks -- so the
// headline stays unsplit.  (SNNQP_DENSE_FP6_PLAN="rt,ks" forces a plan: a measurement knob.)
// workspace = the ticket head of kernels.h, then the slabs
struct Fp6Plan { int rt, ks; };
static Fp6Plan pick_fp6_plan(int T, int B, int K, unsigned gy, bool may_split) {
  const int nchunks = ((K + 63) / 64 + F6_KSC - 1) / F6_KSC;
  Fp6Plan best = {0, 1};
  double best_cost = 0;
  for (int ks = 1; ks <= (may_split ? 4 : 1); ks *= 2) {
    if (ks > 1 && (K < 8192 || nchunks < 8 * ks)) break;
    for (int rt = 1; rt <= 5; ++rt) {
      const int sb = rt * 32 / T;
      if (sb < 1) continue;
      const int64_t wgs = (int64_t)((B + sb - 1) / sb) * gy * ks;
      if (ks > 1 && wgs / ks > HANDOFF_TICKET_BYTES / 4) continue;      // a ticket per tile
      const double kscale = (double)K / 32768.0;
      const double cost = (double)((wgs + 255) / 256) * (11.0 + kscale * (9.5 + 15.5 * rt) / ks) +
                          (ks > 1 ? 6.0 + 0.09 * (rt * 16 * ks) : 0.0);
      if (best.rt == 0 || cost < best_cost - 1e-9 || (cost < best_cost + 1e-9 && ks == best.ks)) {
        best = Fp6Plan{rt, ks};
        best_cost = cost;
      }
    }
  }
  return best;
}

static int64_t fp6_workspace_bytes(const Fp6Plan &p, int T, int B, unsigned gy) {
  if (p.ks <= 1) return 0;
  const int sb = p.rt * 32 / T;
  const int64_t tiles = (int64_t)((B + sb - 1) / sb) * gy;
  return HANDOFF_TICKET_BYTES + tiles * p.ks * (int64_t)(p.rt * 32 * 128) * 4;
}

int64_t dense_fp6_workspace_bytes(int32_t T, int32_t B, int32_t K, int32_t N) {
  if (T <= 0 || B <= 0 || T > 160) return 0;
  const unsigned gy = (unsigned)((N + 127) / 128);
  return fp6_workspace_bytes(pick_fp6_plan(T, B, K, gy, true), T, B, gy);
}

const char *dense_fp6_unsupported(int in_type, int32_t K, int32_t N, const snnqp_weight_t *w) {
  if (in_type != SNNQP_BITS || w->wtype != SNNQP_W_I8) return "not int8 codes over bit-packed rows";
  if (!w->wt_fp6 || w->code_max <= 0 || w->code_max > 7) return "no fp6 tiles of codes known to fit fp6";
  return K <= 0 || N <= 0 ? "bad K/N" : nullptr;
}

const char *dense_fp6_unsupported(const BlockCall &c) {
  if (const char *why = dense_fp6_unsupported(c.in_type, c.K, c.N, c.w)) return why;
  if (c.s_type != SNNQP_BITS) return "spike output must be bit-packed";
  if (c.T > 160) return "more than 160 timesteps";
  if ((int64_t)7 * c.K >= ((int64_t)1 << 24)) return "a partial sum float32 may not hold exactly";
  if (c.nrn->kind == SNNQP_NEURON_LIF && !c.nrn->decay) return "LIF without decay";
  if (dense_rows_broken(c, SNNQP_BITS, 160, c.T > 0 ? c.T - 1 : 0, (c.K + 31) / 32))
    return "input strides beyond 32-bit word offsets within a workgroup";
  return nullptr;
}

// The launch of T x B rows, K deep, N wide with this workspace: what run_dense_fp6 launches and
// what snnqp_dense_fp6_plan reports.  No GPU call.
struct Fp6Launch {
  int rt, ks;        // row tiles of a workgroup; workgroups per tile along K
  int sb;            // samples of a workgroup
  unsigned gx, gy;   // the grid (z: ks)
  int gcz;           // group-chunks of one workgroup of a split tile; 0: unsplit
};
static int plan_dense_fp6(int32_t T, int32_t B, int32_t K, int32_t N, const void *ws, int64_t ws_bytes,
                          Fp6Launch *out) {
  const unsigned gy = (unsigned)((N + 127) / 128);
  // the workspace decides: the plan with a K split when the caller brought enough of it
  // (snnqp_dense_workspace_bytes, zero-filled once), else the best plan without
  Fp6Plan plan = pick_fp6_plan(T, B, K, gy, ws != nullptr);
  if (const char *e = ws ? std::getenv("SNNQP_DENSE_FP6_PLAN") : nullptr) {     // "rt,ks": measurement knob
    int r = 0, k = 0;
    if (std::sscanf(e, "%d,%d", &r, &k) == 2 && r >= 1 && r <= 5 && r * 32 >= T && (k == 1 || k == 2 || k == 4)) {
      // a ticket per tile in the fixed head, as in the planner: a forced split of more tiles is not a plan
      const int sb = r * 32 / T;
      if (k == 1 || (int64_t)((B + sb - 1) / sb) * gy <= HANDOFF_TICKET_BYTES / 4) plan = Fp6Plan{r, k};
    }
  }
  if (plan.ks > 1 && !handoff_ws_usable(ws, ws_bytes, fp6_workspace_bytes(plan, T, B, gy)))
    plan = pick_fp6_plan(T, B, K, gy, false);
  SNNQP_REQUIRE(plan.rt > 0, SNNQP_EUNSUPPORTED, "dense fp6: T too large");
  out->rt = plan.rt; out->ks = plan.ks;
  out->sb = plan.rt * 32 / T;
  out->gx = (unsigned)((B + out->sb - 1) / out->sb);
  out->gy = gy;
  out->gcz = 0;
  if (plan.ks > 1) {
    const int nchunks = ((K + 63) / 64 + F6_KSC - 1) / F6_KSC;
    const int ngc_all = (nchunks + F6_KGROUPS - 1) / F6_KGROUPS;
    out->gcz = (ngc_all + plan.ks - 1) / plan.ks;
  }
  return SNNQP_OK;
}

int run_dense_fp6(const BlockCall &c) {
  if (int rc = block_entry("dense fp6", c, c.w->wt_fp6 != nullptr)) return rc < 0 ? rc : SNNQP_OK;
  const int32_t T = c.T, B = c.B, K = c.K, N = c.N;
  DenseFp6Args a = {};
  fill_block_args(a, c);
  a.K = K; a.N = N; a.KW = (K + 31) / 32; a.KS = (K + 63) / 64;
  a.wt6 = (const uint8_t *)c.w->wt_fp6;
  Fp6Launch p;
  if (int rc = plan_dense_fp6(T, B, K, N, c.ws, c.ws_bytes, &p)) return rc;
  const int rt = p.rt;
  const unsigned gx = p.gx, gy = p.gy;
  a.SB = p.sb;
  a.ksplit = p.ks;
  if (p.ks > 1) {
    a.gcz = p.gcz;
    void *slabs;
    if (int rc = handoff_arm(c.ws, (int64_t)gx * gy, c.st, &a.tickets, &slabs, &a.status)) return rc;
    a.slabs = (float *)slabs;
  }
  switch (rt) {
    case 5: launch_dense_fp6<5>(a, gx, gy, c.st); break;
    case 4: launch_dense_fp6<4>(a, gx, gy, c.st); break;
    case 3: launch_dense_fp6<3>(a, gx, gy, c.st); break;
    case 2: launch_dense_fp6<2>(a, gx, gy, c.st); break;
    default: launch_dense_fp6<1>(a, gx, gy, c.st); break;
  }
  SNNQP_CHECK_LAUNCH("dense_fp6_kernel");
  return SNNQP_OK;
}

}  // namespace snnqp

extern "C" int snnqp_dense_fp6_plan(int32_t T, int32_t B, int32_t K, int32_t N, const void *ws,
                                    int64_t ws_bytes, int32_t *rt, int32_t *ks, int32_t *gx, int32_t *gcz) {
  using namespace snnqp;
  SNNQP_REQUIRE(rt && ks && gx && gcz, SNNQP_EINVAL, "dense_fp6_plan: null argument");
  SNNQP_REQUIRE(T >= 1 && B >= 1 && K >= 1 && N >= 1, SNNQP_EINVAL, "dense_fp6_plan: bad sizes");
  Fp6Launch p;
  if (int rc = plan_dense_fp6(T, B, K, N, ws, ws_bytes, &p)) return rc;
  *rt = p.rt; *ks = p.ks; *gx = (int32_t)p.gx; *gcz = p.gcz;
  return SNNQP_OK;
}

extern "C" int snnqp_pack_codes_fp6(const int8_t *w, int64_t K, int32_t N, int32_t Npad,
                                    void *wt6, snnqp_stream_t stream) {
  using namespace snnqp;
  SNNQP_REQUIRE(w && wt6 && K > 0 && N > 0, SNNQP_EINVAL, "pack_codes_fp6: bad argument");
  SNNQP_REQUIRE(Npad >= N && (Npad & 31) == 0, SNNQP_EINVAL,
                "pack_codes_fp6: Npad must be a multiple of 32, Npad >= N");
  const int64_t total = (int64_t)(Npad / 32) * ((K + 63) / 64) * 64;
  const int64_t blocks = ceil_div64(total, 256);
  hipLaunchKernelGGL(pack_codes_fp6_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     (hipStream_t)stream, w, K, N, Npad, (uint32_t *)wt6);
  SNNQP_CHECK_LAUNCH("pack_codes_fp6_kernel");
  return SNNQP_OK;
}
