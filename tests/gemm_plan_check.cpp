// Host-only check of the GEMM launch planner (csrc/gemm_plan.h): prints the
// plan of every "M N K m_dynamic precision" group on the command line, one
// line each: tile grid gen may_split c_stream workspace_bytes.
// Driven by tests/test_gemm_plan.py.
//
// With a leading "--variant" the groups are GEMM calls,
// "M N K m_dynamic k_dynamic a_trans b_trans a2 precision Meff Keff" (Meff,
// Keff: the values of the device-side counters, or M, K), and a line names the
// kernel instantiation the call runs and the plan the device evaluates at the
// effective shape: tile gen a_trans b_trans ragged a2 | mode S tiles
// min(grid, tiles * S) kstep ns grid.  (Precision 0: the one fp32 kernel per
// layout; mode / S are split_for's, kstep and ns print as 0.)
// Driven by tests/test_gemm_exact_cases.py.
#include "../posecnn_amd/csrc/gemm_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int variants(int argc, char** argv) {
  using namespace pcnn_gk;
  if (argc % 11 != 0) return 2;
  for (int i = 0; i + 10 < argc; i += 11) {
    int a[11];
    for (int j = 0; j < 11; j++) a[j] = atoi(argv[i + j]);
    const int M = a[0], N = a[1], K = a[2], mdyn = a[3], kdyn = a[4], at = a[5], bt = a[6], a2 = a[7], prec = a[8],
              Meff = a[9], Keff = a[10];
    const LaunchPlan p = plan_launch(M, N, K, mdyn != 0, prec);
    if (prec == 0) {
      const int S = split_for(Meff, N, Keff);
      const long tiles = (long)((Meff + kF32Tile - 1) / kF32Tile) * ((N + kF32Tile - 1) / kF32Tile);
      const long items = tiles * S;
      printf("%d 1 %d %d 0 %d %d %d %ld %ld 0 0 %d\n", p.tile, at, bt, a2, (int)(S > 1), S, tiles,
             items < p.grid ? items : (long)p.grid, p.grid);
      continue;
    }
    const bool ragged = split_ragged(at != 0, bt != 0, M, N, K, kdyn != 0);
    XPlan pl = x_plan(Meff, N, Keff, p.tile, p.grid, split_bk(prec));
    if (!p.gen) {  // the lean kernel form runs whole tiles
      pl.mode = 0;
      pl.S = 1;
    }
    const int items = pl.tiles * pl.S;
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", p.tile, (int)p.gen, at, bt, (int)ragged, a2, pl.mode, pl.S,
           pl.tiles, items < p.grid ? items : p.grid, (pl.ns + pl.S - 1) / pl.S, pl.ns, p.grid);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "--variant") == 0) return variants(argc - 2, argv + 2);
  if ((argc - 1) % 5 != 0) return 2;
  for (int i = 1; i + 4 < argc; i += 5) {
    const int M = atoi(argv[i]), N = atoi(argv[i + 1]), K = atoi(argv[i + 2]), dyn = atoi(argv[i + 3]),
              prec = atoi(argv[i + 4]);
    const pcnn_gk::LaunchPlan p = pcnn_gk::plan_launch(M, N, K, dyn != 0, prec);
    printf("%d %d %d %d %d %zu\n", p.tile, p.grid, (int)p.gen, (int)p.may_split, (int)p.c_stream,
           pcnn_gk::gemm_workspace_bytes(M, N, K, dyn != 0, prec));
  }
  return 0;
}
