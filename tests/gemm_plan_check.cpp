// Host-only check of the GEMM launch planner (csrc/gemm_plan.h): prints the
// plan of every "M N K m_dynamic precision" group on the command line, one
// line each: tile grid gen may_split c_stream workspace_bytes.
// Driven by tests/test_gemm_plan.py.
#include "../posecnn_amd/csrc/gemm_plan.h"
#include <stdio.h>
#include <stdlib.h>

int main(int argc, char** argv) {
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
