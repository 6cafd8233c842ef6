// mbx_bits1.hip -- COUNT scans of shallow bit-plane plans (k_scan_bits1, one plane per term), their
// batched and shared-plane forms for chains of captured launches (k_scan_bits1_batch,
// k_scan_bits1_shared; the chain itself: mbx_fuse.cpp) and their launchers.
#include "mbx_planes.hpp"

namespace mbx {

// ------------------------------------------- shallow bit-plane COUNT scan
//
// A plan whose every bound is decided on its column's top kept bit (depth <= 1:
// C3, any bound that is round at that bit, two-key columns) reads at most one
// plane per term, NP per tile, and needs none of k_scan_bits' per-bound state:
// its predicate is a bitwise function of the tile's NP dwords.  The host works
// that function out before the launch (bits1_plan_of: the term and conjunct
// rules of mbx_planes.hpp over probe words) and the kernel arguments carry its 2^NP-row
// truth table and the NP plane pointers, nothing else of the plan.  A tile then
// costs one select per table node, and what is left per lane is the loads: a
// wave issues all of a batch's -- kB tiles x (NP planes + the deleted image), 12
// sixteen-byte loads per lane where that divides -- before it waits for the
// first: one round trip for a C3 segment.  A tile's address is scalar (only the
// lane offset is a register), so the 48 load registers fit 64 VGPRs, 8 waves
// per SIMD.
// Four planes keep 8 loads per lane live (10 with the deleted image): the third
// tile's 4 would spill beside the 8 partial results of a four-plane table.
constexpr int bits1_batch(int np, bool del) {
  return np >= 4 ? 2 : 12 / (np + (del ? 1 : 0) > 0 ? np + (del ? 1 : 0) : 1);
}

// Plane slots and truth table of a shallow plan: the predicate over probe
// words, plane k's probe holding bit k of every index 0..15
static Bits1Launch bits1_plan_of(const KBitPlan& B) {
  constexpr uint32_t kProbe[kSliceMaxTerms] = {0xAAAAu, 0xCCCCu, 0xF0F0u, 0xFF00u};
  Bits1Launch P{};
  uint32_t r[kSliceMaxTerms] = {0u, 0u, 0u, 0u};
  int slot = 0;
  for (int ti = 0; ti < B.nterms; ++ti) {
    const KBitTerm& t = B.terms[ti];
    uint32_t probe = 0u;
    if (bit_term_depth(t.meta) > 0) {
      P.pl[slot] = t.planes;
      probe = kProbe[slot++];
    }
    r[ti] = bit_term1<uint32_t>(t.meta, t.lo, t.hi, probe);
  }
  P.table = bit_cnf(bit_cnf_of(B), r) & 0xFFFFu;
  return P;
}

// The selected rows of one dword of NP planes.  Shannon expansion of the truth
// table: for each value c of planes 1.. the rows are (x[0] & la[c]) ^ lb[c]
// (plane 0, its complement or a constant); plane k then picks between the two
// halves that differ in its bit.
template <int NP>
__device__ __forceinline__ uint32_t bits1_rows(const uint32_t (&x)[NP > 0 ? NP : 1],
                                               const uint32_t (&la)[1 << (NP > 0 ? NP - 1 : 0)],
                                               const uint32_t (&lb)[1 << (NP > 0 ? NP - 1 : 0)]) {
  constexpr int kC = 1 << (NP > 0 ? NP - 1 : 0);
  uint32_t g[kC];
#pragma unroll
  for (int c = 0; c < kC; ++c) g[c] = (x[0] & la[c]) ^ lb[c];
#pragma unroll
  for (int k = 1; k < NP; ++k)
#pragma unroll
    for (int c = 0; c < (kC >> k); ++c) g[c] = (x[k] & g[2 * c + 1]) | (~x[k] & g[2 * c]);
  return g[0];
}

// The address of a lane's 16 bytes of the tile that starts at the uniform
// address p, as scalar base + 32-bit lane offset: one VGPR per address instead
// of two.  Both halves pass through an empty asm the optimizer cannot look
// through -- left alone, hipcc hoists the widened lane offset (or base + lane
// offset) out of the tile loop as a 64-bit vector value and every load pays a
// 64-bit vector add and a register pair.
__device__ __forceinline__ const char* bit_tile_lane(const uint32_t* p, int lane) {
  uint64_t a = reinterpret_cast<uint64_t>(p);
  uint32_t off = (uint32_t)lane * 16u;
  asm("" : "+s"(a));
  asm("" : "+v"(off));
  return reinterpret_cast<const char*>(a) + off;
}
__device__ __forceinline__ v4u bit_tile_load(const uint32_t* p, int lane) {
  return __builtin_nontemporal_load((gv4u*)bit_tile_lane(p, lane));
}

// Segments, tile ownership, the partial tile and the deleted image as in
// k_scan_bits; kB tiles per batch instead of U.  Tile numbers fit 32 bits
// (rows < 2^40, and the host holds tiles_per_block to the table's tiles), so
// the segment bounds and the loop's compares are 32-bit scalar arithmetic.
// FIN: kPlaneFinPacked or kPlaneFinFrame.
// The body is mbx_scan_bits1_body.hpp, the text of both kernels over the record P.  As a __device__
// function that both call it cost this kernel 4 to 14 instructions per instantiation (hipcc reduces
// the tile loop's induction differently after inlining); included, its code is what it was.
template <int NP, bool DEL, int FIN>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_scan_bits1(Bits1Launch P) {
#define MBX_BITS1_GRID_X gridDim.x
#include "mbx_scan_bits1_body.hpp"
#undef MBX_BITS1_GRID_X
}

// A run of independent shallow COUNT scans recorded back to back in a graph
// capture, as one launch (Bits1Fuse, mbx_fuse.cpp): grid row y is query y, its record
// picked from the kernel arguments by a scalar index, and runs k_scan_bits1's
// body as it stands -- blockIdx.x, the query's blocks and its own ticket area
// are what a launch of its own would see.  Blocks are dispatched x-fastest, so
// a query's tail and finalize run under the next query's loads, and the run
// pays one launch's ramp and drain.  Every query of a batch is the same
// instantiation over the same number of blocks, nb.  A grid row is nb rounded
// up to the chip's 8 XCDs (the padding blocks leave at once): workgroups go to
// the XCDs round-robin in dispatch order, so block x of every row runs on XCD
// x % 8 as in a launch of its own, and queries over the same planes find their
// segments in the L2 that read them last.
template <int NP, bool DEL, int FIN>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_scan_bits1_batch(Bits1Batch B) {
  if (blockIdx.x >= B.nb) return;
  const Bits1Launch& P = B.q[blockIdx.y];
#define MBX_BITS1_GRID_X B.nb
#include "mbx_scan_bits1_body.hpp"
#undef MBX_BITS1_GRID_X
}

// Queries of a chain that read the same planes (same pl[0..NP), deleted image,
// rows and segment: a *plane group*) differ only in their truth table, and
// every such query's COUNT is a sum of the same 2^NP minterm populations
//   m_i = popcount(live & AND_k (bit k of i ? x_k : ~x_k)),  count_q = sum of m_i over the set bits i of table_q.
// k_scan_bits1_shared reads a group's planes once: grid row y is group y, the
// loop is k_scan_bits1's (tile ownership, kB loads per wave before the first
// wait, scalar tile addresses, partial tile, deleted image), and a lane keeps,
// in place of the one query's popcount, the 2^NP subset counts
//   S_T = popcount(live & AND_{k in T} x_k),  T a set of planes (S_0: the live rows),
// one AND and one popcount-accumulate each; m_i follows from them by inclusion-
// exclusion, once per block.  k_scan_bits1 drops a tile the clamp loads again
// as a whole and masks the partial tile's result; here S_0 and the all-zero
// minterm count rows on their own, so (1) such a tile adds to no counter and
// (2) in the partial tile `valid` is the live rows of every subset.  After
// the block's exact reduction thread m < members works count_m out of the
// block's totals and hands it in as member m's own launch would: its ticket
// area (that of its position in the chain), count word or frame, nan_out.
constexpr int bits1_top_plane(int s) { return s >= 8 ? 3 : (s >= 4 ? 2 : (s >= 2 ? 1 : 0)); }

// c[T] += S_T of one dword: a[T] = a[T without its top plane] & that plane
template <int NP, bool LIVE>
__device__ __forceinline__ void bits1_subsets(uint32_t (&c)[1 << NP], const uint32_t (&x)[NP], uint32_t live) {
  uint32_t a[1 << NP];
  a[0] = live;
  if (LIVE) c[0] += (uint32_t)__popc(live);
#pragma unroll
  for (int s = 1; s < (1 << NP); ++s) {
    const int k = bits1_top_plane(s), rest = s ^ (1 << k);
    a[s] = (rest == 0 && !LIVE) ? x[k] : (a[rest] & x[k]);
    c[s] += (uint32_t)__popc(a[s]);
  }
}

// 8 waves per SIMD like k_scan_bits1; four planes' 16 counters are not held to it (they spill if they are)
template <int NP, bool DEL, int FIN>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NP >= 4 ? 4 : 8, 8))) void k_scan_bits1_shared(
    Bits1Shared S) {
  static_assert(NP >= 1 && NP <= kSliceMaxTerms, "a chain without planes stays one grid row per query");
  constexpr int kB = bits1_batch(NP, DEL);
  constexpr int kM = 1 << NP;
  constexpr int kTileDwords = kBitTileRows / 32;
  // Group blockIdx.y's record, held in scalar registers from here on: every scalar load of the
  // kernel is issued above the padding-block branch (the record of a valid blockIdx.y is always
  // readable) and the first plane load waits for them once.  With nb a field of its own behind the
  // records, hipcc loaded it, waited and branched, and only then loaded the record: a second round
  // trip to cold kernel-argument lines in front of every block's first plane byte.
  const Bits1Group& G = S.g[blockIdx.y];
  struct {
    int64_t nrows;
    int32_t tiles_per_block;
    const uint32_t* pl[NP];
    const uint64_t* deleted;
    uint32_t first, count;
  } P;
  P.nrows = G.nrows;
  P.tiles_per_block = G.tiles_per_block;
#pragma unroll
  for (int k = 0; k < NP; ++k) P.pl[k] = G.pl[k];
  P.deleted = G.deleted;
  uint32_t fc;  // first, count: 16 bits each
  __builtin_memcpy(&fc, &G.first, sizeof(fc));
  uint32_t nblocks = G.nb;
  asm volatile("" : "+s"(P.nrows), "+s"(P.tiles_per_block), "+s"(fc), "+s"(nblocks));
#pragma unroll
  for (int k = 0; k < NP; ++k) asm volatile("" : "+s"(P.pl[k]));
  if constexpr (DEL) asm volatile("" : "+s"(P.deleted));
  if (blockIdx.x >= nblocks) return;
  P.first = fc & 0xFFFFu;
  P.count = fc >> 16;
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int members = (int)P.count;
  // Thread m's member record is a vector load from the kernel arguments (threads past the group's
  // members read its last one and drop it), issued after the last tile.  Left alone, hipcc sinks it
  // below the barrier, a whole round trip on the block's tail; member_pin holds it above the barrier
  // and waits for it there, so the block's reduction covers most of the trip.  (Issued before the
  // first plane load it costs that load a wait: hipcc settles every pending load at the loop's head.)
  const Bits1Member& Mr = S.m[(int)P.first + min((int)threadIdx.x, members - 1)];
  uint64_t out = 0, ticket = 0, nan_out = 0;
  uint32_t table = 0;
  int32_t groups = 0;
  auto member_load = [&]() {
    out = reinterpret_cast<uint64_t>(Mr.out);
    table = Mr.table;
    if constexpr (FIN == kPlaneFinPacked) {
      ticket = reinterpret_cast<uint64_t>(Mr.ticket);
      nan_out = reinterpret_cast<uint64_t>(Mr.nan_out);
      groups = Mr.ticket_groups;
    }
  };
  auto member_pin = [&]() {
    if constexpr (FIN == kPlaneFinPacked)
      asm volatile("" : "+v"(out), "+v"(ticket), "+v"(nan_out), "+v"(table), "+v"(groups));
    else
      asm volatile("" : "+v"(out), "+v"(table));
  };
  const int tp = (int)(P.nrows / kBitTileRows);     // the full tiles = the partial tile's number
  const int prows = (int)(P.nrows % kBitTileRows);  // the partial tile's rows
  const int t0 = (int)blockIdx.x * P.tiles_per_block;
  const int t1 = min(t0 + P.tiles_per_block, tp + (prows != 0 ? 1 : 0));
  const uint32_t* pl[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) pl[k] = P.pl[k];
  gu32* del = (gu32*)P.deleted;
  const bool del16 = DEL && (reinterpret_cast<uintptr_t>(P.deleted) & 15) == 0;  // uniform

  uint32_t c[kM];  // the lane's S_T
#pragma unroll
  for (int s = 0; s < kM; ++s) c[s] = 0u;
  const int tf = min(t1, tp);  // full tiles in the main loop
  for (int base = min(t0 + wave, tf); base < tf; base += kWaves * kB) {
    v4u x[kB][NP], dead[kB];
    // every load of the batch, unconditional; a tile past the full tiles is the last one again, and is not counted
    int64_t dw[kB];  // the tile's first dword in every plane (uniform)
#pragma unroll
    for (int u = 0; u < kB; ++u) {
      dw[u] = (int64_t)min(base + u * kWaves, tf - 1) * kTileDwords;
#pragma unroll
      for (int k = 0; k < NP; ++k) x[u][k] = bit_tile_load(pl[k] + dw[u], lane);
    }
    if (DEL) {
      if (del16) {
#pragma unroll
        for (int u = 0; u < kB; ++u) dead[u] = bit_tile_load(reinterpret_cast<const uint32_t*>(P.deleted) + dw[u], lane);
      } else {
#pragma unroll
        for (int u = 0; u < kB; ++u) {
          gu32* d = (gu32*)bit_tile_lane(reinterpret_cast<const uint32_t*>(P.deleted) + dw[u], lane);
#pragma unroll
          for (int i = 0; i < 4; ++i) dead[u][i] = d[i];
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // no use of a loaded tile is scheduled among the loads: one wait, after the last

#pragma unroll
    for (int u = 0; u < kB; ++u) {
      if (base + u * kWaves < tf) {  // uniform: a tile loaded again counts nowhere, S_0 included
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t xi[NP];
#pragma unroll
          for (int k = 0; k < NP; ++k) xi[k] = x[u][k][i];
          bits1_subsets<NP, DEL>(c, xi, DEL ? ~dead[u][i] : ~0u);
        }
        if (!DEL) c[0] += 128u;  // the lane's rows of a full tile, all live
      }
    }
  }
  // the partial tile, owned like any other tile of [t0, t1)
  if (prows != 0 && tp >= t0 + wave && tp < t1 && (tp - t0 - wave) % kWaves == 0) {
    v4u xp[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) xp[k] = bit_tile_load(pl[k] + (int64_t)tp * kTileDwords, lane);
    const int64_t dw = (int64_t)tp * kTileDwords + lane * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rem = prows - (lane * 4 + i) * 32;  // the dword's rows below nrows
      uint32_t valid = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
      if (DEL && rem > 0) valid &= ~del[dw + i];
      uint32_t xi[NP];
#pragma unroll
      for (int k = 0; k < NP; ++k) xi[k] = xp[k][i];
      bits1_subsets<NP, true>(c, xi, valid);
    }
  }
  member_load();
  // The block's S_T, exact.  A lane's counter is at most 128 rows x its wave's tiles of the segment,
  // below wave_sum_dpp's 2^26 for any segment under 2^20 tiles: one sum per counter; else wave_count's two.
  __shared__ uint64_t wsum[kWaves][kM];
  const bool small = P.tiles_per_block < (1 << 20);  // uniform
#pragma unroll
  for (int s = 0; s < kM; ++s) {
    const uint64_t wc = small ? (uint64_t)wave_sum_dpp(c[s]) : wave_count(c[s]);
    if (lane == 0) wsum[wave][s] = wc;
  }
  member_pin();
  __syncthreads();
  if ((int)threadIdx.x >= members) return;
  // member threadIdx.x, from here on in lanes of their own: nothing below is forced uniform
  uint64_t f[kM];
#pragma unroll
  for (int s = 0; s < kM; ++s) {
    f[s] = wsum[0][s];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) f[s] += wsum[w][s];
  }
#pragma unroll
  for (int k = 0; k < NP; ++k)  // S_T -> m_i: rows that hold T's planes and none of the others
#pragma unroll
    for (int s = 0; s < kM; ++s)
      if (((s >> k) & 1) == 0) f[s] -= f[s | (1 << k)];
  uint64_t total = 0;
#pragma unroll
  for (int s = 0; s < kM; ++s) total += ((table >> s) & 1u) != 0u ? f[s] : 0ull;
  if (FIN == kPlaneFinFrame)  // result unused: a no-return atomic, nothing waits for it in the block
    __hip_atomic_fetch_add(reinterpret_cast<uint64_t*>(out) + (blockIdx.x % kFrameSlots) * kFrameSlotStride,
                           pack_count((int64_t)total, 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    packed_count_finalize(reinterpret_cast<uint32_t*>(ticket), groups, (int64_t)total, 0,
                          reinterpret_cast<int64_t*>(out), reinterpret_cast<int32_t*>(nan_out), nblocks);
}

// ---------------------------------------------------------------- launchers

// The instantiation as values for the chain code.  Made only here, where the ladder below ends: the
// batch and shared kernels that exist are those of the k_scan_bits1 instantiations it can launch.
template <int NP, bool DEL, int FIN>
constexpr Bits1Kernels bits1_kernels() {
  Bits1Kernels K = {&k_scan_bits1<NP, DEL, FIN>, &k_scan_bits1_batch<NP, DEL, FIN>, nullptr, NP, DEL, FIN};
  if constexpr (NP > 0) K.shared = &k_scan_bits1_shared<NP, DEL, FIN>;
  return K;
}

template <int NP, bool DEL, int FIN>
static void bits1_launch_del(const Bits1Launch& P, dim3 grid, hipStream_t s, Bits1Fuse* fuse) {
  static constexpr Bits1Kernels K = bits1_kernels<NP, DEL, FIN>();
  if (fuse && bits1_fuse_join(fuse, P, grid, s, K)) return;
  hipLaunchKernelGGL((k_scan_bits1<NP, DEL, FIN>), grid, dim3(kBlock), 0, s, P);
  if (fuse && bits1_fuse_on(fuse)) bits1_fuse_start(fuse, P, K, grid, s);
}

template <int NP, int FIN>
static void bits1_launch(const ScanLaunch& L, const KBitPlan& B, dim3 grid, hipStream_t s, Bits1Fuse* fuse) {
  Bits1Launch P = bits1_plan_of(B);
  const int64_t ntiles = (L.nrows + kBitTileRows - 1) / kBitTileRows;
  P.nrows = L.nrows;
  P.tiles_per_block = (int32_t)std::min(L.tiles_per_block, std::max<int64_t>(ntiles, 1));  // the grid is the same
  P.deleted = L.deleted;
  P.out = L.count_out;
  P.ticket = L.ticket;
  P.nan_out = L.nan_out;
  P.ticket_groups = L.ticket_groups;
  if (L.deleted)
    bits1_launch_del<NP, true, FIN>(P, grid, s, fuse);
  else
    bits1_launch_del<NP, false, FIN>(P, grid, s, fuse);
}

template <int FIN>
static hipError_t bits1_launch_np(const ScanLaunch& L, const KBitPlan& B, dim3 grid, hipStream_t s, Bits1Fuse* fuse) {
  switch (bit_plan_reads(B)) {  // one plane per term that reads
    case 0: bits1_launch<0, FIN>(L, B, grid, s, fuse); break;
    case 1: bits1_launch<1, FIN>(L, B, grid, s, fuse); break;
    case 2: bits1_launch<2, FIN>(L, B, grid, s, fuse); break;
    case 3: bits1_launch<3, FIN>(L, B, grid, s, fuse); break;
    case 4: bits1_launch<4, FIN>(L, B, grid, s, fuse); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_scan_bits1(const ScanLaunch& L, const KBitPlan& B, int fin, dim3 grid, hipStream_t s,
                             Bits1Fuse* fuse) {
  if (fin == kPlaneFinFrame) return bits1_launch_np<kPlaneFinFrame>(L, B, grid, s, fuse);
  return bits1_launch_np<kPlaneFinPacked>(L, B, grid, s, fuse);
}

}  // namespace mbx
