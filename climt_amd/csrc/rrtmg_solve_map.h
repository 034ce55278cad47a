// rrtmg_solve_map.h -- THE LAUNCH-ORDER RULE of the solve kernels (rrtmg_sw.hip, rrtmg_lw.hip): blockIdx.x -> the workgroup's
// tiles and work item.  Plain C++: tools/solve_map_check.cpp runs it on the CPU for every (W, GPB) the kernels use.
//
// A solve workgroup is W wavefronts = W consecutive entries of ITS variant's compacted tile list (SwDev / LwDev::tlist, nmine
// entries: ngrp groups of W) x one work item (position k of the heaviest-first order SwTab / LwTab::sched, nitem of them).
// Launch order: BLOCKS of GPB tile groups (W x GPB = 128 tiles in the shortwave, 32 in the longwave); within a block work items
// heaviest first, tile groups fastest -- a block's prep rows (58 MB at 60 layers and 128 tiles) are read by its work items while
// they are still cached, however many tiles the launch covers (a large chunk of a grid with both kinds of tiles: 2048 tiles are
// 0.94 GB of prep rows, re-read from HBM by every work item in item-major order).  Up to one block of tiles there is one block:
// the order of rounds 1-4.  The last block of the order holds the remaining groups.
// The launch was sized for every tile of the chunk (the host does not know the counts); the workgroups with work are the FIRST
// ngrp x nitem of the dispatch order and dense in it, the others exit at once behind them.  (A workgroup that exits at once
// still has to be PLACED with its 138 KB of LDS: interleaved with real ones -- a padded grid in round 2, or 8192 McICA columns
// with every fourth tile cloud-free before this mapping, 3.64 ms against 2.93 with clouds everywhere -- half the real
// workgroups wait for a CU that still holds another.)
// Speed only, never correctness -- as long as every (group, item) with work is produced exactly once.
#pragma once

#ifdef __HIPCC__
#define RRTMG_SOLVE_MAP_HD __host__ __device__ __forceinline__
#else
#define RRTMG_SOLVE_MAP_HD inline
#endif

namespace rrtmg {

// work: false = the workgroup exits at once (workgroup-uniform); first: the group's first list entry (entries first .. first +
// W - 1, those below nmine exist); k: the position in sched
struct SolveWork { bool work; int first, k; };
template <int W, int GPB>
RRTMG_SOLVE_MAP_HD SolveWork solve_map(int q, int nmine, int nitem) {
  const int ngrp = (nmine + W - 1) / W;
  const int per = GPB * nitem, nfull = ngrp / GPB;
  if (q >= ngrp * nitem) return {false, 0, 0};
  const int gpb = q < nfull * per ? GPB : ngrp - nfull * GPB, r = q < nfull * per ? q % per : q - nfull * per;
  const int grp = (q < nfull * per ? q / per : nfull) * GPB + r % gpb;
  return {true, grp * W, r / gpb};
}

}  // namespace rrtmg
