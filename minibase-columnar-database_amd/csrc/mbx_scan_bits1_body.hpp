// mbx_scan_bits1_body.hpp -- the body of k_scan_bits1 and k_scan_bits1_batch (mbx_bits1.hip), included
// inside each kernel: NP, DEL, FIN are the kernel's template parameters, P its Bits1Launch record (the
// kernel argument / record blockIdx.y of the batch), the macro MBX_BITS1_GRID_X the blocks of P's query
// (a named constant in its place changes k_scan_bits1's code).  No include guard: it is text.
  constexpr int kB = bits1_batch(NP, DEL);
  constexpr int kNP = NP > 0 ? NP : 1, kC = 1 << (kNP - 1);
  constexpr int kTileDwords = kBitTileRows / 32;
  // The epilogue's arguments, held in scalar registers from here on: left alone, hipcc loads them
  // after the block's barrier, a scalar memory round trip between the last plane load and the
  // block's atomic.  Here they ride in the one round of argument loads before the first plane load.
  uint64_t out = reinterpret_cast<uint64_t>(P.out), ticket = reinterpret_cast<uint64_t>(P.ticket);
  uint64_t nan_out = reinterpret_cast<uint64_t>(P.nan_out);
  int32_t groups = P.ticket_groups;
  uint32_t nblocks = MBX_BITS1_GRID_X;
  if constexpr (FIN == kPlaneFinPacked)
    asm volatile("" : "+s"(out), "+s"(ticket), "+s"(nan_out), "+s"(groups), "+s"(nblocks));
  else
    asm volatile("" : "+s"(out));
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int tp = (int)(P.nrows / kBitTileRows);     // the full tiles = the partial tile's number
  const int prows = (int)(P.nrows % kBitTileRows);  // the partial tile's rows
  const int t0 = (int)blockIdx.x * P.tiles_per_block;
  const int t1 = min(t0 + P.tiles_per_block, tp + (prows != 0 ? 1 : 0));
  const uint32_t* pl[kNP];
#pragma unroll
  for (int k = 0; k < kNP; ++k) pl[k] = P.pl[k];
  uint32_t la[kC], lb[kC];  // uniform: bits1_rows' leaves
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    const uint32_t f0 = (P.table >> (2 * c)) & 1u, f1 = (P.table >> (2 * c + 1)) & 1u;
    lb[c] = f0 ? ~0u : 0u;
    la[c] = f0 != f1 ? ~0u : 0u;
  }
  gu32* del = (gu32*)P.deleted;
  const bool del16 = DEL && (reinterpret_cast<uintptr_t>(P.deleted) & 15) == 0;  // uniform

  uint32_t cnt = 0;
  const int tf = min(t1, tp);  // full tiles in the main loop
  for (int base = min(t0 + wave, tf); base < tf; base += kWaves * kB) {
    v4u x[kB][kNP], dead[kB];
    // every load of the batch, unconditional; a tile past the full tiles is the last one again, and is not counted
    int64_t dw[kB];  // the tile's first dword in every plane (uniform)
#pragma unroll
    for (int u = 0; u < kB; ++u) {
      dw[u] = (int64_t)min(base + u * kWaves, tf - 1) * kTileDwords;
      x[u][0] = bit_splat(0u);
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
      uint32_t c = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t xi[kNP];
#pragma unroll
        for (int k = 0; k < kNP; ++k) xi[k] = x[u][k][i];
        const uint32_t rows = bits1_rows<NP>(xi, la, lb);
        c += (uint32_t)__popc(DEL ? rows & ~dead[u][i] : rows);
      }
      cnt += base + u * kWaves < tf ? c : 0u;
    }
  }
  // the partial tile, owned like any other tile of [t0, t1)
  if (prows != 0 && tp >= t0 + wave && tp < t1 && (tp - t0 - wave) % kWaves == 0) {
    v4u xp[kNP];
    xp[0] = bit_splat(0u);
#pragma unroll
    for (int k = 0; k < NP; ++k) xp[k] = bit_tile_load(pl[k] + (int64_t)tp * kTileDwords, lane);
    const int64_t dw = (int64_t)tp * kTileDwords + lane * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rem = prows - (lane * 4 + i) * 32;  // the dword's rows below nrows
      uint32_t valid = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
      if (DEL && rem > 0) valid &= ~del[dw + i];
      uint32_t xi[kNP];
#pragma unroll
      for (int k = 0; k < kNP; ++k) xi[k] = xp[k][i];
      cnt += (uint32_t)__popc(bits1_rows<NP>(xi, la, lb) & valid);
    }
  }
  plane_count_finish<FIN>(cnt, reinterpret_cast<int64_t*>(out), reinterpret_cast<uint32_t*>(ticket), groups,
                          reinterpret_cast<int32_t*>(nan_out), nblocks);
