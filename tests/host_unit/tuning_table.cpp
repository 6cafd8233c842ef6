// CPU dump of mbx_set_tuning (tests/test_tuning_table.py): for every knob named
// on the command line and every probe value, a default-constructed mbx_ctx on
// the stack takes mbx_set_tuning(&ctx, knob, value) and one line goes out --
// the return code, every MbxTuning field, and the error text of a failure.
// mbx_set_tuning touches only ctx.tune, so no HIP call is made and no GPU is
// needed.  Then, per knob, "reset" after a change, and one unknown name.
#include <cstdio>
#include <cstring>

#include "../../minibase-columnar-database_amd/csrc/mbx_objects.hpp"

// every field of MbxTuning, in the struct's order
#define TUNING_FIELDS(F)                                                                              \
  F(tiles_per_block) F(force_generic) F(scan_hoist) F(scan_int_range) F(scan_ri) F(sink_lds)          \
  F(ticket_groups) F(fin_mode) F(join_plain) F(join_chunk_words) F(distinct_lds_probes)               \
  F(gather_fused) F(gather_pair) F(cnf_store) F(cnf_lookback) F(cnf_flag_stride) F(cnf_blocks)        \
  F(select_blocks) F(cursor_prefetch) F(scan_select_fused) F(scan_select_waves) F(select_flag_stride) \
  F(scan_words_wt) F(comm_same_stream) F(auto_slice) F(auto_bitslice) F(bits_shallow)                 \
  F(graph_fuse_counts) F(bitmap_plane_floor) F(select_dbg)

static const long long kValues[] = {-2, -1, 0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 8, 128, 512, 32, 64,
                                    1LL << 24, (1LL << 24) + 1, 1LL << 31, 1LL << 40};

static void dump(const char* knob, long long value, int rc, const MbxTuning& t) {
  printf("%s %lld -> %d |", knob, value, rc);
#define F(f) printf(" %lld", (long long)t.f);
  TUNING_FIELDS(F)
#undef F
  if (rc != MBX_OK) printf(" | %s", mbx_last_error());
  printf("\n");
}

int main(int argc, char** argv) {
  printf("# knob value -> rc |");
#define F(f) printf(" " #f);
  TUNING_FIELDS(F)
#undef F
  printf(" | error\n");
  {
    mbx_ctx ctx;
    dump("(defaults)", 0, MBX_OK, ctx.tune);
    const int rc = mbx_set_tuning(&ctx, "reset", 0);
    dump("reset", 0, rc, ctx.tune);
  }
  for (int i = 1; i < argc; i++)
    for (long long v : kValues) {
      mbx_ctx ctx;
      const int rc = mbx_set_tuning(&ctx, argv[i], v);
      dump(argv[i], v, rc, ctx.tune);
    }
  for (int i = 1; i < argc; i++) {
    mbx_ctx ctx;
    mbx_set_tuning(&ctx, argv[i], 3);
    const int rc = mbx_set_tuning(&ctx, "reset", 0);
    char label[128];
    snprintf(label, sizeof(label), "reset-after-%s", argv[i]);
    dump(label, 3, rc, ctx.tune);
  }
  {
    mbx_ctx ctx;
    const int rc = mbx_set_tuning(&ctx, "no_such_knob", 1);
    dump("no_such_knob", 1, rc, ctx.tune);
  }
  return 0;
}
