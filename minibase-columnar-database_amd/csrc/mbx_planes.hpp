// mbx_planes.hpp -- what the plane-scan translation units share: mbx_slices.hip (byte planes),
// mbx_bits.hip (bit planes), mbx_bits1.hip (shallow bit-plane plans) and mbx_fuse.cpp (chains of
// captured shallow launches).  The epilogue choice, the term and conjunct rules over row masks, the
// shallow kernels' launch records and the seam between the shallow launchers and the chain code.
#pragma once
#include <type_traits>

#include "mbx_device.hpp"

namespace mbx {

// a lane's selected rows -> the block's arrival, in the launch's PlaneFin form
// (plane_fin_of picks it on the host)
template <int FIN>
__device__ __forceinline__ void plane_finish(uint32_t cnt, const ScanLaunch& L) {
  if constexpr (FIN == kPlaneFinGeneral)
    plane_count_general(cnt, L);
  else
    plane_count_finish<FIN>(cnt, L.count_out, L.ticket, L.ticket_groups, L.nan_out);
}

struct SliceCnf {
  int32_t nconj, never;
  uint32_t cmask[kSliceMaxTerms];
};

// The term and conjunct rules of the bit-plane scans are written once over the row-mask type V:
// v4u in the kernels (a lane's 128 rows of a tile), uint32_t where the host
// works a shallow plan's truth table out before the launch (bits1_plan_of).
// (bit_neg .. bit_dhi, the fields of a term's meta word: mbx_internal.hpp)
template <class V = v4u>
__host__ __device__ __forceinline__ V bit_splat(uint32_t f) {
  if constexpr (std::is_same<V, uint32_t>::value) {
    return f;
  } else {
    V v = {f, f, f, f};
    return v;
  }
}

// plane j (x) against bit j of the bound `k >= bits` (UPPER: `k <= bits`) of
// depth d.  y: the rows beyond the bound on this bit, were the bound's bit the
// other value -- a lower bound's 1 / an upper bound's 0 lets only equal rows
// go on (n = 0), the other value also passes the rows beyond it (n = ~0).
template <bool UPPER, class V>
__host__ __device__ __forceinline__ void bit_step(V& ok, V& eq, const V& x, uint32_t bits, int j, int d) {
  const uint32_t a = j < d ? ~0u : 0u;
  const uint32_t n = (((bits >> j) & 1u) != (UPPER ? 1u : 0u)) ? 0u : ~0u;
  const V y = UPPER ? ~x : x;
  ok |= eq & y & bit_splat<V>(n & a);
  eq &= (y ^ bit_splat<V>(n)) | bit_splat<V>(~a);
}

__device__ __forceinline__ uint32_t bit_popc(const v4u& v) {
  return (uint32_t)(__popc(v[0]) + __popc(v[1]) + __popc(v[2]) + __popc(v[3]));
}

struct BitTerms {
  const uint32_t* pl[kSliceMaxTerms];
  uint32_t lo[kSliceMaxTerms], hi[kSliceMaxTerms], meta[kSliceMaxTerms];
  int nterms;
  int64_t pstride;
};

// The rows every required conjunct selects, given each term's rows
template <class V>
__host__ __device__ __forceinline__ V bit_cnf(const SliceCnf& cn, const V (&r)[kSliceMaxTerms]) {
  V a = bit_splat<V>(cn.never ? 0u : ~0u);
#pragma unroll
  for (int q = 0; q < kSliceMaxTerms; ++q)
    if (q < cn.nconj) {
      V o = bit_splat<V>(0u);
#pragma unroll
      for (int ti = 0; ti < kSliceMaxTerms; ++ti)
        if ((cn.cmask[q] >> ti) & 1u) o |= r[ti];
      a &= o;
    }
  return a;
}

__host__ __device__ __forceinline__ SliceCnf bit_cnf_of(const KBitPlan& B) {
  SliceCnf cn;
  cn.nconj = B.nconj;
  cn.never = B.never;
#pragma unroll
  for (int q = 0; q < kSliceMaxTerms; ++q) cn.cmask[q] = B.cmask[q];
  return cn;
}

// k_scan_bits1's kernel arguments: what the kernel reads and nothing else of
// ScanLaunch, 88 bytes, what the first plane load needs (rows, segment, plane
// pointers, deleted image) in front -- one round of scalar loads and one wait
// before that load.  The kernel finishes in the two hot forms only
// (kPlaneFinPacked / kPlaneFinFrame); launch_scan_bits sends every other form
// of a shallow plan to k_scan_bits.
struct Bits1Launch {
  int64_t nrows;
  int32_t tiles_per_block;             // bit tiles; at most the table's, so tile numbers stay in 32 bits
  uint32_t table;                      // bit i: rows whose plane-k bit is bit k of i are selected
  const uint32_t* pl[kSliceMaxTerms];  // slot k: plane 0 of the k-th term that reads one
  const uint64_t* deleted;             // device or null
  int64_t* out;                        // the count word (kPlaneFinPacked) / the count frame (kPlaneFinFrame)
  uint32_t* ticket;                    // kPlaneFinPacked
  int32_t* nan_out;
  int32_t ticket_groups;
  int32_t pad_;
};

// A term of depth <= 1 over plane 0 of its column (x: any value at depth 0)
template <class V>
__host__ __device__ __forceinline__ V bit_term1(uint32_t m, uint32_t lo, uint32_t hi, const V& x) {
  V lok = bit_splat<V>(bit_slo(m) == kSliceHolds ? ~0u : 0u), leq = bit_splat<V>(bit_slo(m) == kSliceEqual ? ~0u : 0u);
  V hok = bit_splat<V>(bit_shi(m) == kSliceHolds ? ~0u : 0u), heq = bit_splat<V>(bit_shi(m) == kSliceEqual ? ~0u : 0u);
  bit_step<false>(lok, leq, x, lo, 0, bit_dlo(m));
  bit_step<true>(hok, heq, x, hi, 0, bit_dhi(m));
  const V v = (lok | leq) & (hok | heq);
  return bit_neg(m) ? ~v : v;
}

// k_scan_bits1_batch's kernel arguments: the records of a chain's queries, one per grid row
constexpr unsigned kXcds = 8;  // a grid row is nb rounded up to the chip's XCDs (mbx_bits1.hip says why)
struct Bits1Batch {
  Bits1Launch q[kMaxFuse];
  uint32_t nb;  // blocks per query
  uint32_t pad_;
};
static_assert(sizeof(Bits1Launch) == 88, "k_scan_bits1's kernel arguments");
static_assert(sizeof(Bits1Batch) == kMaxFuse * 88 + 8 && sizeof(Bits1Batch) <= 4096, "a batch fits the kernel arguments");

// k_scan_bits1_shared's kernel arguments: the chain by plane groups.
// A group's record is all a block reads before its first plane load, the launch's
// nb included: one round of scalar loads and one wait, as in k_scan_bits1.
struct Bits1Group {
  int64_t nrows;
  int32_t tiles_per_block;
  uint16_t first, count;               // its members: m[first, first + count)
  const uint32_t* pl[kSliceMaxTerms];
  const uint64_t* deleted;             // device or null
  uint32_t nb;                         // blocks per group: the same in every record of a launch
  uint32_t pad_;
};
struct Bits1Member {
  int64_t* out;      // the count word (kPlaneFinPacked) / the count frame (kPlaneFinFrame)
  uint32_t* ticket;  // kPlaneFinPacked
  int32_t* nan_out;
  uint32_t table;
  int32_t ticket_groups;
};
struct Bits1Shared {
  Bits1Group g[kMaxFuse];   // what the first plane load needs
  Bits1Member m[kMaxFuse];  // in group order
};
static_assert(sizeof(Bits1Group) == 64 && sizeof(Bits1Member) == 32, "k_scan_bits1_shared's records");
static_assert(sizeof(Bits1Shared) == kMaxFuse * 96 && sizeof(Bits1Shared) <= 4096, "the groups fit the kernel arguments");

#ifndef MBX_BITS_U
#define MBX_BITS_U 2
#endif
// The PlaneFin of a COUNT launch over planes.  The two hot forms -- the packed
// in-launch finalize and the count frame -- have kernels that carry nothing
// else; write-through (the fin_mode knob, or a grid packed_count_fits refuses),
// kFinSegOnly, kFinSeparate / no ticket and a launch with segment counts take
// the general form.
inline int plane_fin_of(const ScanLaunch& L) {
  if (L.seg_counts) return kPlaneFinGeneral;
  if (L.fin_mode == kFinFrame) return kPlaneFinFrame;
  if (L.fin_mode == kFinPackedCount && L.ticket) return kPlaneFinPacked;
  return kPlaneFinGeneral;
}

// ---- between the shallow launchers (mbx_bits1.hip) and the chain code (mbx_fuse.cpp)
//
// One instantiation <NP, DEL, FIN> of the shallow kernels, as values: what the chain code needs of it.
// mbx_bits1.hip makes one where its launch ladder ends, so the entries are the ladder's instantiations.
struct Bits1Kernels {
  void (*one)(Bits1Launch);     // k_scan_bits1
  void (*batch)(Bits1Batch);    // k_scan_bits1_batch
  void (*shared)(Bits1Shared);  // k_scan_bits1_shared; null for np == 0
  int np;
  bool del;
  int fin;  // kPlaneFinPacked or kPlaneFinFrame
};
constexpr int bits1_key(int np, bool del, int fin) { return np * 4 + (del ? 2 : 0) + (fin == kPlaneFinFrame ? 1 : 0); }

// a shallow plan's launch in one of the two hot forms (launch_scan_bits, which has checked B)
hipError_t launch_scan_bits1(const ScanLaunch& L, const KBitPlan& B, int fin, dim3 grid, hipStream_t s,
                             Bits1Fuse* fuse);
bool bits1_fuse_on(const Bits1Fuse* f);  // the open capture fuses
// true: P is grid row f->n of the chain's node now and needs no launch
bool bits1_fuse_join(Bits1Fuse* f, Bits1Launch P, dim3 grid, hipStream_t s, const Bits1Kernels& K);
// the launch just recorded starts a chain of one: today's single kernel node
void bits1_fuse_start(Bits1Fuse* f, const Bits1Launch& P, const Bits1Kernels& K, dim3 grid, hipStream_t s);

}  // namespace mbx
