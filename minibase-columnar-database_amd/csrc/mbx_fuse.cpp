// mbx_fuse.cpp -- chains of captured shallow COUNT launches: the host bookkeeping that makes one kernel
// node of a run of k_scan_bits1 launches recorded back to back in a graph capture.  Host code only:
// mbx_bits1.hip has the kernels and hands each launch over with its Bits1Kernels entry.
#include <new>

#include "mbx_planes.hpp"

namespace mbx {

// The chain's rules (launch_scan_bits' `fuse`).
// While a capture is open the context keeps the last k_scan_bits1 launch it recorded: its graph
// node, its instantiation and grid, and the launch records of the chain so far.  The next such
// launch joins the chain -- no node is added, the chain's node becomes k_scan_bits1_batch over one
// more grid row -- when nothing else was recorded in between (the stream's capture dependencies are
// still exactly that node), it is the same instantiation over the same number of blocks, the batch
// has room and its output overlaps no output of the batch.  The queries of a batch run concurrently:
// they read planes nothing in the batch writes, write distinct words and arrive on ticket areas of
// their own, so each result is what its own launch gives; everything else recorded keeps its order
// against the whole batch.  The graph stays linear.  A graph call that fails leaves the nodes as
// they are and ends fusion on the context for good: a capture never fails because of a chain.
struct Bits1Fuse {
  bool on = false;      // the open capture fuses
  bool broken = false;  // a graph call failed on this context
  hipGraphNode_t node = nullptr;  // the chain's kernel node, the capture's tail when it was recorded; null: no chain
  int key = 0;          // bits1_key of the chain's instantiation
  unsigned gx = 0;      // its blocks per query
  void* func = nullptr; // the node's kernel and grid as last set: what a replay record repeats
  dim3 grid;
  int n = 0;            // its queries
  int64_t launches = 0, scans = 0;  // this capture: nodes that hold more than one query, the queries in them
  int64_t groups = 0, shared = 0;   // this capture: the plane groups of those nodes, the queries in groups of several
  int chain_groups = 0, chain_shared = 0;  // the chain's part of both (0 while it is one query)
  Bits1Batch B;
  Bits1Shared S;  // B by plane groups, when one of them holds two queries
};

// What the chain's node runs, by value: mbx_graph_launch repeats it as a plain launch when the node
// is the whole graph.  The arguments are the node's own -- k_scan_bits1's record for a chain of one,
// the batch, or the plane groups.
struct Bits1Replay {
  void* func;
  dim3 grid;
  union Args {
    Bits1Launch one;
    Bits1Batch batch;
    Bits1Shared shared;
    Args() {}
  } a;
};

Bits1Fuse* bits1_fuse_new() { return new (std::nothrow) Bits1Fuse(); }
void bits1_fuse_free(Bits1Fuse* f) { delete f; }
void bits1_fuse_begin(Bits1Fuse* f, bool on) {
  f->on = on && !f->broken;
  f->node = nullptr;
  f->n = 0;
  f->launches = f->scans = 0;
  f->groups = f->shared = 0;
  f->chain_groups = f->chain_shared = 0;
}
void bits1_fuse_cut(Bits1Fuse* f) {
  f->node = nullptr;
  f->n = 0;
}
bool bits1_fuse_on(const Bits1Fuse* f) { return f->on; }
static void bits1_fuse_break(Bits1Fuse* f) {
  (void)hipGetLastError();
  f->broken = true;
  f->on = false;
  f->node = nullptr;
}

// the stream's only capture dependency, or null (none, several, or not capturing)
static hipGraphNode_t bits1_capture_tail(Bits1Fuse* f, hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0;
  if (hipStreamGetCaptureInfo_v2(s, &st, nullptr, nullptr, &deps, &nd) != hipSuccess) {
    bits1_fuse_break(f);
    return nullptr;
  }
  return st == hipStreamCaptureStatusActive && nd == 1 && deps ? deps[0] : nullptr;
}

void bits1_fuse_end(Bits1Fuse* f, int64_t* fused_launches, int64_t* fused_scans, int64_t* plane_groups,
                    int64_t* shared_scans, hipStream_t s, Bits1Replay** replay) {
  if (replay) {
    *replay = nullptr;
    // a live chain whose node is still the last thing recorded; whether it is the only thing is the caller's to see
    if (f->on && f->node && f->n >= 1 && f->func && bits1_capture_tail(f, s) == f->node) {
      Bits1Replay* r = new (std::nothrow) Bits1Replay();
      if (r) {
        r->func = f->func;
        r->grid = f->grid;
        if (f->n == 1)
          r->a.one = f->B.q[0];
        else if (f->chain_shared > 0)
          r->a.shared = f->S;
        else
          r->a.batch = f->B;
        *replay = r;
      }
    }
  }
  if (fused_launches) *fused_launches = f->launches;
  if (fused_scans) *fused_scans = f->scans;
  if (plane_groups) *plane_groups = f->groups;
  if (shared_scans) *shared_scans = f->shared;
  f->on = false;
  f->node = nullptr;
  f->n = 0;
}

void bits1_replay_free(Bits1Replay* r) { delete r; }
hipError_t bits1_replay_launch(const Bits1Replay* r, hipStream_t s) {
  void* args[1] = {const_cast<Bits1Replay::Args*>(&r->a)};
  return hipLaunchKernel(r->func, r->grid, dim3(kBlock), args, 0, s);
}

// the launch just recorded starts a chain of one: today's single kernel node
void bits1_fuse_start(Bits1Fuse* f, const Bits1Launch& P, const Bits1Kernels& K, dim3 grid, hipStream_t s) {
  f->node = nullptr;
  hipGraphNode_t tail = bits1_capture_tail(f, s);
  hipGraphNodeType ty = hipGraphNodeTypeEmpty;
  if (!tail || hipGraphNodeGetType(tail, &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) return;
  f->node = tail;
  f->key = bits1_key(K.np, K.del, K.fin);
  f->gx = grid.x;
  f->func = reinterpret_cast<void*>(K.one);
  f->grid = grid;
  f->n = 1;
  f->chain_groups = f->chain_shared = 0;
  f->B.q[0] = P;
}

// The chain's n queries by plane groups, in f->S: query j joins the first group whose planes (slot
// for slot), deleted image, rows and segment are its own, else opens one; members in group order,
// each with the ticket area of its place in the chain.  Returns the groups; *shared: the queries
// in groups of several.
static int bits1_fuse_groups(Bits1Fuse* f, int n, int* shared) {
  int of[kMaxFuse], ng = 0;
  Bits1Shared& S = f->S;
  for (int j = 0; j < n; ++j) {
    const Bits1Launch& q = f->B.q[j];
    int g = 0;
    for (; g < ng; ++g) {
      const Bits1Group& G = S.g[g];
      bool same = G.nrows == q.nrows && G.tiles_per_block == q.tiles_per_block && G.deleted == q.deleted;
      for (int k = 0; k < kSliceMaxTerms; ++k) same = same && G.pl[k] == q.pl[k];
      if (same) break;
    }
    if (g == ng) {
      Bits1Group& G = S.g[ng++];
      G.nrows = q.nrows;
      G.tiles_per_block = q.tiles_per_block;
      G.count = 0;
      for (int k = 0; k < kSliceMaxTerms; ++k) G.pl[k] = q.pl[k];
      G.deleted = q.deleted;
      G.nb = f->gx;
      G.pad_ = 0;
    }
    S.g[g].count += 1;
    of[j] = g;
  }
  int at = 0;
  *shared = 0;
  for (int g = 0; g < ng; ++g) {
    S.g[g].first = (uint16_t)at;
    if (S.g[g].count > 1) *shared += S.g[g].count;
    for (int j = 0; j < n; ++j)
      if (of[j] == g) {
        const Bits1Launch& q = f->B.q[j];
        S.m[at++] = Bits1Member{q.out, q.ticket, q.nan_out, q.table, q.ticket_groups};
      }
  }
  return ng;
}

// true: P is grid row f->n of the chain's node now and needs no launch
bool bits1_fuse_join(Bits1Fuse* f, Bits1Launch P, dim3 grid, hipStream_t s, const Bits1Kernels& K) {
  if (!f->node || f->key != bits1_key(K.np, K.del, K.fin) || f->gx != grid.x || f->n >= kMaxFuse) return false;
  // the count word, or the whole count frame
  const uintptr_t bytes = K.fin == kPlaneFinFrame ? sizeof(int64_t) * kFrameSlots * kFrameSlotStride : sizeof(int64_t);
  const uintptr_t o = reinterpret_cast<uintptr_t>(P.out);
  for (int j = 0; j < f->n; ++j) {
    const uintptr_t q = reinterpret_cast<uintptr_t>(f->B.q[j].out);
    if (o < q + bytes && q < o + bytes) return false;
  }
  const hipGraphNode_t tail = bits1_capture_tail(f, s);
  if (!tail || tail != f->node) return false;  // something else was recorded since (or the call failed)
  if (K.fin == kPlaneFinPacked) P.ticket += (size_t)f->n * kTicketWords;
  f->B.q[f->n] = P;
  int shared = 0;
  int groups = bits1_fuse_groups(f, f->n + 1, &shared);
  if (K.np == 0) groups = f->n + 1, shared = 0;  // no planes to share: every query a group of its own
  void* args[1] = {&f->B};
  hipKernelNodeParams kp{};
  kp.func = reinterpret_cast<void*>(K.batch);
  f->B.nb = f->gx;
  kp.gridDim = dim3((f->gx + kXcds - 1) / kXcds * kXcds, (unsigned)(f->n + 1));
  if (shared > 0) {  // a group of several (np > 0): one grid row per group, groups of one ride along
    args[0] = &f->S;
    kp.func = reinterpret_cast<void*>(K.shared);
    kp.gridDim.y = (unsigned)groups;
  }
  kp.blockDim = dim3(kBlock);
  kp.sharedMemBytes = 0;
  kp.kernelParams = args;
  kp.extra = nullptr;
  if (hipGraphKernelNodeSetParams(f->node, &kp) != hipSuccess) {
    bits1_fuse_break(f);  // the node is what it was: the chain so far
    return false;
  }
  f->n += 1;
  f->func = kp.func;
  f->grid = kp.gridDim;
  f->launches += f->n == 2 ? 1 : 0;
  f->scans += f->n == 2 ? 2 : 1;
  f->groups += groups - f->chain_groups;
  f->shared += shared - f->chain_shared;
  f->chain_groups = groups;
  f->chain_shared = shared;
  return true;
}

}  // namespace mbx
