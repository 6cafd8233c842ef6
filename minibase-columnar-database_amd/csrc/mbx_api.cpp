// mbx_api.cpp -- the library and context part of the C-ABI (include/mbx.h).
//
// What every other host file of the C-ABI stands on: the thread-local error
// text, mbx_init / mbx_free / mbx_sync and the context's scratch (partials,
// diagnostic stamps, the pinned HostScratch), the tuning knobs (one table,
// mbx_set_tuning), and the raw device helpers (mbx_dev_*, mbx_probe_read,
// mbx_diag_*).  The families live beside their kernels: tables in
// mbx_table.cpp, the plan compiler in mbx_plan.cpp, scans and the launch
// decision in mbx_scan.cpp, BitSets in mbx_bitmap.cpp, late materialisation
// and cursors in mbx_cursor.cpp.
// Nothing here computes a query result on the CPU: every row-level operation
// is a kernel launch on the context stream.
#include <cctype>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "mbx_objects.hpp"  // with include/mbx.h, the HIP runtime and mbx_internal.hpp

using namespace mbx;

// ------------------------------------------------------------------ errors

static thread_local std::string g_err;

int mbx::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// ------------------------------------------------------------------ tuning

// how mbx_set_tuning turns the requested value of a knob into the stored one
enum KnobRule : uint8_t {
  kAsIs,       // stored as requested
  kFlag,       // != 0
  kWithin,     // lo .. hi as requested, anything else stores `other`
  kIntRange,   // scan_int_range: 0, 1 or 2, anything else is MBX_E_INVALID
  kFinMode,    // as requested; the A/B-only modes are MBX_E_UNSUPPORTED without -DMBX_DIAG
  kSelectDbg,  // as requested; the A/B-only bits are MBX_E_UNSUPPORTED without -DMBX_DIAG
};

// One row per field of MbxTuning (mbx_objects.hpp documents the knobs; its
// member initialisers are the defaults).  A 32-bit knob's rule sees
// (int32_t)value, a 64-bit knob's the whole value.
struct Knob {
  const char* name;  // as mbx_set_tuning spells it; a -DMBX_DIAG build reads MBX_<NAME> from the environment
  uint16_t offset, width;  // the field: an int32_t or an int64_t of MbxTuning
  KnobRule rule;
  int64_t lo, hi, other;  // kWithin
  bool sees32;            // a 64-bit knob whose rule sees (int32_t)value
};

#define KNOB(field, ...) {#field, offsetof(MbxTuning, field), sizeof(MbxTuning::field), __VA_ARGS__}
static const Knob kKnobs[] = {
    // stored as requested
    KNOB(tiles_per_block, kAsIs), KNOB(force_generic, kAsIs), KNOB(scan_hoist, kAsIs), KNOB(scan_ri, kAsIs),
    KNOB(sink_lds, kAsIs), KNOB(ticket_groups, kAsIs), KNOB(join_plain, kAsIs), KNOB(distinct_lds_probes, kAsIs),
    KNOB(gather_fused, kAsIs), KNOB(cursor_prefetch, kAsIs), KNOB(scan_select_fused, kAsIs),
    // on / off
    KNOB(gather_pair, kFlag), KNOB(scan_words_wt, kFlag), KNOB(comm_same_stream, kFlag), KNOB(auto_slice, kFlag),
    KNOB(auto_bitslice, kFlag), KNOB(bits_shallow, kFlag), KNOB(graph_fuse_counts, kFlag),
    // a range, or one value of two
    KNOB(join_chunk_words, kWithin, 1, kJoinChunkWords, kJoinChunkWords),  // the join's scratch bound does not grow
    KNOB(cnf_store, kWithin, 0, 3, 0), KNOB(cnf_lookback, kWithin, 0, 2, 0),
    KNOB(cnf_flag_stride, kWithin, kFlagStride, kFlagStride, 1), KNOB(select_flag_stride, kWithin, 1, 1, kFlagStride),
    KNOB(scan_select_waves, kWithin, 4, 4, 16), KNOB(cnf_blocks, kWithin, 0, INT32_MAX, 0),
    KNOB(select_blocks, kWithin, 1, INT32_MAX, 1024),  // never a zero / negative grid divisor
    KNOB(bitmap_plane_floor, kWithin, 0, INT32_MAX, -1, true),
    // their own checks
    KNOB(scan_int_range, kIntRange), KNOB(fin_mode, kFinMode), KNOB(select_dbg, kSelectDbg),
};
#undef KNOB

// the fields of an aggregate: the most initialisers its list-initialisation takes
struct AnyField { template <class T> constexpr operator T() const { return T(); } };
template <class S, class... A>
constexpr int field_count(...) { return (int)sizeof...(A); }
template <class S, class... A>
constexpr auto field_count(int) -> decltype(S{A{}..., AnyField{}}, 0) { return field_count<S, A..., AnyField>(0); }
static_assert(sizeof(kKnobs) / sizeof(kKnobs[0]) == field_count<MbxTuning>(0), "one kKnobs row per MbxTuning field");

static int knob_apply(MbxTuning& t, const Knob& k, int64_t value) {
  const int64_t x = k.width == 4 || k.sees32 ? (int32_t)value : value;
  const int32_t v = (int32_t)x;
  int64_t stored = x;
  switch (k.rule) {
    case kAsIs: break;
    case kFlag: stored = x != 0; break;
    case kWithin: stored = x < k.lo || x > k.hi ? k.other : x; break;
    case kIntRange:
      if (v < 0 || v > 2) return fail(MBX_E_INVALID, "mbx_set_tuning: scan_int_range %d (0, 1 or 2)", v);
      break;
    case kFinMode:
#ifndef MBX_DIAG
      // kFinFences (plain stores + fences) and kFinSegOnly forced on a COUNT
      // scan (no count) exist for A/B measurements only
      if (v == kFinFences || v == kFinSegOnly)
        return fail(MBX_E_UNSUPPORTED, "mbx_set_tuning: fin_mode %d needs a -DMBX_DIAG build", v);
#endif
      break;
    case kSelectDbg:
      // k_select_ids takes bits 0-1, the one-launch selections bits 4-6: A/B
      // forms a production build compiles out (kDiagDbg)
      if (((v & 3) | ((v >> 4) & 983)) & ~kDiagDbg)
        return fail(MBX_E_UNSUPPORTED, "mbx_set_tuning: select_dbg %d needs a -DMBX_DIAG build", v);
      break;
  }
  char* field = reinterpret_cast<char*>(&t) + k.offset;
  if (k.width == 4) *reinterpret_cast<int32_t*>(field) = (int32_t)stored;
  else *reinterpret_cast<int64_t*>(field) = stored;
  return MBX_OK;
}

// The context's tuning at mbx_init and after mbx_set_tuning("reset"): the
// production defaults, MbxTuning's member initialisers.  A -DMBX_DIAG build
// (tools/build_diag.sh, tools/build_variant.sh) then takes each knob's
// MBX_<NAME> from the environment through the setter's rule (a value the rule
// rejects leaves the default); the default library reads no environment at
// all -- tests and tools drive the same knobs through mbx_set_tuning.
static void tuning_defaults(MbxTuning& t) {
  t = MbxTuning();
#ifdef MBX_DIAG
  for (const Knob& k : kKnobs) {
    char name[64] = "MBX_";  // the rest is zeroed: the name stays terminated
    size_t n = 4;
    for (const char* p = k.name; *p && n + 1 < sizeof(name); p++) name[n++] = (char)toupper((unsigned char)*p);
    const char* e = getenv(name);
    if (e && *e) knob_apply(t, k, atoll(e));
  }
#endif
}

extern "C" int mbx_set_tuning(mbx_ctx* c, const char* knob, int64_t value) {
  NOTNULL(c);
  NOTNULL(knob);
  if (!strcmp(knob, "reset")) {
    tuning_defaults(c->tune);
    return MBX_OK;
  }
  for (const Knob& k : kKnobs)
    if (!strcmp(knob, k.name)) return knob_apply(c->tune, k, value);
  return fail(MBX_E_INVALID, "mbx_set_tuning: unknown knob `%s`", knob);
}

// ----------------------------------------------------------------- helpers

int mbx::ensure_partials(mbx_ctx* c, int64_t n) {
  if (n <= c->partials_cap) return MBX_OK;
  if (c->partials) HIPCHK(hipFree(c->partials));
  c->partials = nullptr;
  const int64_t cap = n < 4096 ? 4096 : n;
  HIPCHK(hipMalloc(&c->partials, sizeof(Partial) * cap));
  c->partials_cap = cap;
  return MBX_OK;
}

int mbx::stamps_of(mbx_ctx* c, int64_t** out) {
  const bool on = (c->tune.select_dbg & 8) != 0;
  if (on && !c->stamps) HIPCHK(hipMalloc(&c->stamps, sizeof(int64_t) * 4 * kMaxStampBlocks));
  *out = on ? c->stamps : nullptr;
  return MBX_OK;
}

int mbx::set_device(mbx_ctx* c) {
  HIPCHK(hipSetDevice(c->device));
  return MBX_OK;
}

// ----------------------------------------------------------------- library

extern "C" int mbx_abi_version(void) { return MBX_ABI_VERSION; }

extern "C" const char* mbx_last_error(void) { return g_err.c_str(); }

extern "C" int mbx_device_count(int32_t* n) {
  NOTNULL(n);
  int k = 0;
  hipError_t e = hipGetDeviceCount(&k);
  if (e != hipSuccess) {
    *n = 0;
    return fail(MBX_E_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *n = k;
  return MBX_OK;
}

extern "C" int mbx_init(int32_t device, mbx_ctx** out) {
  NOTNULL(out);
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return fail(MBX_E_DEVICE, "mbx_init: no HIP device visible (the executor has no CPU fallback)");
  if (device < 0 || device >= n) return fail(MBX_E_INVALID, "mbx_init: device %d of %d", device, n);
  mbx_ctx* c = new (std::nothrow) mbx_ctx();
  if (!c) return fail(MBX_E_NOMEM, "mbx_init: host allocation");
  c->device = device;
  tuning_defaults(c->tune);
  int rc = MBX_OK;
  do {
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&c->dagg, sizeof(AggOut));
    if (e == hipSuccess) e = hipMalloc(&c->dcount, sizeof(int64_t) * 2);
    if (e == hipSuccess) e = hipMalloc(&c->dnan, sizeof(int32_t) * 4);
    if (e == hipSuccess) e = hipMemset(c->dnan, 0, sizeof(int32_t) * 4);
    if (e == hipSuccess) e = hipMalloc(&c->ticket, sizeof(uint32_t) * kTicketWords * kMaxFuse);
    if (e == hipSuccess) e = hipMemset(c->ticket, 0, sizeof(uint32_t) * kTicketWords * kMaxFuse);
    if (e == hipSuccess) e = hipHostMalloc(&c->pinned, 256, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&c->lookback, sizeof(int64_t) * kLookbackWords);
    if (e == hipSuccess) e = hipMemset(c->lookback, 0, sizeof(int64_t) * kLookbackWords);
    if (e != hipSuccess) {
      rc = fail(MBX_E_DEVICE, "mbx_init: %s", hipGetErrorString(e));
      break;
    }
    if (!(c->fuse = bits1_fuse_new())) {
      rc = fail(MBX_E_NOMEM, "mbx_init: host allocation");
      break;
    }
    rc = ensure_partials(c, 4096);
  } while (0);
  if (rc != MBX_OK) {
    mbx_free(c);
    return rc;
  }
  *out = c;
  return MBX_OK;
}

extern "C" int mbx_free(mbx_ctx* c) {
  if (!c) return MBX_OK;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  comm_release_of(c);
  hipFree(c->partials);
  hipFree(c->dagg);
  hipFree(c->dcount);
  hipFree(c->dnan);
  hipFree(c->ticket);
  bits1_fuse_free(c->fuse);
  hipFree(c->ids_scratch);
  hipFree(c->stamps);
  hipFree(c->lookback);
  if (c->pinned) hipHostFree(c->pinned);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
  return MBX_OK;
}

// Waits for the context stream and reports what the *_async scans enqueued
// since the last mbx_sync raised: a NaN reached by a float compare sets the
// sticky word dnan[1] (the kernels' last block), read and cleared here.
extern "C" int mbx_sync(mbx_ctx* c) {
  NOTNULL(c);
  if (c->capturing) return fail(MBX_E_INVALID, "mbx_sync inside a graph capture");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = comm_sync(c)) return rc;
  int32_t* h = &c->pinned->sticky_nan;
  HIPCHK(hipMemcpyAsync(h, c->dnan + 1, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (*h) {
    HIPCHK(hipMemsetAsync(c->dnan + 1, 0, sizeof(int32_t), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return fail(MBX_E_TYPE,
                "NaN in a float comparison in an asynchronous scan (TupleUtils falls through to the string compare "
                "and raises)");
  }
  return MBX_OK;
}

extern "C" void* mbx_stream(mbx_ctx* c) { return c ? (void*)c->stream : nullptr; }

extern "C" int mbx_dev_alloc(mbx_ctx* c, int64_t bytes, void** dev) {
  NOTNULL(c);
  NOTNULL(dev);
  *dev = nullptr;
  if (bytes <= 0) return fail(MBX_E_INVALID, "dev_alloc: %lld bytes", (long long)bytes);
  if (c->capturing) return fail(MBX_E_INVALID, "dev_alloc inside a graph capture");
  HIPCHK(hipSetDevice(c->device));
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)bytes) != hipSuccess) return fail(MBX_E_NOMEM, "dev_alloc: %lld bytes", (long long)bytes);
  hipError_t e = hipMemsetAsync(p, 0, (size_t)bytes, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    hipFree(p);
    return fail(MBX_E_DEVICE, "dev_alloc: %s", hipGetErrorString(e));
  }
  *dev = p;
  return MBX_OK;
}

extern "C" int mbx_dev_free(mbx_ctx* c, void* dev) {
  NOTNULL(c);
  if (!dev) return MBX_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipFree(dev));
  return MBX_OK;
}

extern "C" int mbx_dev_download(mbx_ctx* c, const void* dev, void* host, int64_t bytes) {
  NOTNULL(c);
  NOTNULL(dev);
  NOTNULL(host);
  if (bytes < 0) return fail(MBX_E_INVALID, "dev_download: %lld bytes", (long long)bytes);
  if (c->capturing) return fail(MBX_E_INVALID, "dev_download inside a graph capture");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(host, dev, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MBX_OK;
}

extern "C" int mbx_probe_read(mbx_ctx* c, const mbx_table* t, const int32_t* cols, int32_t ncols,
                              int64_t tiles_per_block, int32_t interleave, int64_t grid) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(cols);
  if (ncols < 1 || ncols > kMaxProbeCols) return fail(MBX_E_INVALID, "probe: ncols %d not in 1..%d", ncols, kMaxProbeCols);
  ProbeArgs A{};
  for (int i = 0; i < ncols; ++i) {
    if (cols[i] < 0 || cols[i] >= (int32_t)t->cols.size() || t->cols[cols[i]].stride_w != 1)
      return fail(MBX_E_INVALID, "probe: column %d is not a 4-byte column of the table", cols[i]);
    A.cols[i] = (const int32_t*)t->cols[cols[i]].dev;
  }
  A.ncols = ncols;
  A.interleave = interleave ? 1 : 0;
  A.nrows = t->nrows;
  A.tiles_per_block = tiles_per_block > 0 ? tiles_per_block : tiles_per_block_for(c, t->nrows);
  const int64_t ntiles = t->nrows / kTileRows;
  A.grid = interleave ? (grid > 0 ? grid : 1024) : (ntiles + A.tiles_per_block - 1) / A.tiles_per_block;
  if (A.grid < 1) A.grid = 1;
  if (A.grid > (1 << 20)) return fail(MBX_E_INVALID, "probe: grid %lld too large", (long long)A.grid);
  if (int rc = ensure_partials(c, A.grid)) return rc;
  A.sink = (uint32_t*)c->partials;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(launch_read_probe(A, c->stream));
  return MBX_OK;
}

extern "C" int mbx_diag_select_stamps(mbx_ctx* c, int64_t* host, int64_t nblocks) {
  NOTNULL(c);
  NOTNULL(host);
  if (!c->stamps) return fail(MBX_E_INVALID, "diag_select_stamps: no stamped launch (select_dbg bit 3)");
  if (nblocks < 0 || nblocks > kMaxStampBlocks) return fail(MBX_E_INVALID, "diag_select_stamps: %lld blocks",
                                                            (long long)nblocks);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(host, c->stamps, sizeof(int64_t) * 4 * (size_t)nblocks, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MBX_OK;
}

extern "C" int mbx_diag_lookback_epoch(mbx_ctx* c, int64_t epoch) {
  NOTNULL(c);
  if (epoch < 0 || epoch > 0x7fffffff) return fail(MBX_E_INVALID, "diag_lookback_epoch: %lld", (long long)epoch);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(c->lookback, &epoch, sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MBX_OK;
}
