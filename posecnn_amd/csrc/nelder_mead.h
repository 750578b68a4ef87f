// The bounded Nelder-Mead search of posecnn_amd/synthesize/icp.py
// nelder_mead_steps, in its operation order and in double, once for every
// device search: the 7-D pose searches over optEnergy records
// (pose_search.hip: one workgroup, cooperating workgroups, speculative
// rounds) and the 6-D refineWithOpt over optEnergy3D (pose3d.hip).  They are
// pinned bit for bit to the Python search or to the oracle, so every detail
// of the order below (x + 0.0, sum / n, fr >= vn choosing the inside
// contraction, the budget-truncated shrink) is part of the contract.
//
// Simplex x0 + step_i e_i with step = min(0.25 (ub - lb), 0.75 (ub - x0),
// 0.75 (x0 - lb)); each iteration a stable sort, the centroid of the best n
// (a sequential sum / n), reflection, expansion, contraction (outside /
// inside), shrink toward the best; trial points clamped to the bounds; at
// most max_eval evaluations.  One workgroup runs a search: thread 0 keeps the
// simplex in LDS, every thread takes part in every evaluation and holds the
// same values, so the control flow is uniform over the workgroup.
//
// The evaluator Ev supplies the objective and decides when points are
// evaluated:
//   Ev::kBatch          1: on demand, one point at a time.  4: in batches of
//                       up to four points.
//   value(xs, k)        the value of xs[k], in every thread.  On demand, the
//                       evaluation happens here: a workgroup barrier comes
//                       before any thread but thread 0 (which wrote it) reads
//                       xs[k], and another after the evaluator's last write
//                       to LDS.  In batches, it returns what prefetch left.
//   prefetch(xs, cnt)   batches only: evaluate xs[0 .. cnt) now, between
//                       workgroup barriers.
//   Ev::kBarrierAfterReflection
//                       one more workgroup barrier after the reflection's
//                       value.  value() already ends behind a barrier, so
//                       nothing depends on it; the record searches have
//                       always had it and keep it, the 6-D search never had.
//   failed()            workgroup-uniform: an evaluation could not complete
//                       and the search ends (constant false where evaluations
//                       cannot fail)
// Every call is made by all threads of the workgroup.  The four candidate
// points of an iteration are pure functions of the centroid, the worst point
// and the bounds: a batching evaluator gets all four at once and may evaluate
// them together, an on-demand one gets each when the sequential algorithm
// asks for its value.  Either way the search asks only for the values the
// sequential algorithm uses, and counts only those.
#pragma once
#include <hip/hip_runtime.h>

namespace pcnn_nm {

template <int N>
struct Simplex {
  double pts[N + 1][N], vals[N + 1];  // the simplex and its values
  double lb[N], ub[N];                // the bounds (set by the caller's thread 0, with pts[0] = x0)
  double cen[N];
  double xs[4][N];  // points handed to the evaluator
};

// Runs the search from s.pts[0] within s.lb / s.ub (written by thread 0 before
// the call) and returns the evaluation count; the simplex and its values are
// left in s (visible to every thread).
template <int N, class Ev>
__device__ __forceinline__ int search(Simplex<N>& s, Ev& ev, int max_eval) {
  constexpr int B = Ev::kBatch;
  static_assert(B == 1 || B == 4, "on demand, or the iteration's four candidates in one batch");
  const int t = threadIdx.x;
  auto clampq = [&](int e, double v) { return fmin(fmax(v, s.lb[e]), s.ub[e]); };  // np.minimum(np.maximum(p, lb), ub)
  // xs[0 .. cnt) (set by thread 0) become rows first .. first + cnt - 1
  auto place = [&](int first, int cnt) {
    if constexpr (B > 1) ev.prefetch(s.xs, cnt);
    for (int k = 0; k < cnt; k++) {
      const double v = ev.value(s.xs, k);
      if (t == 0) {
        for (int e = 0; e < N; e++) s.pts[first + k][e] = s.xs[k][e];
        s.vals[first + k] = v;
      }
    }
  };
  // candidate k of an iteration (thread 0): 0 reflection, 1 expansion,
  // 2 outside contraction (from the reflection), 3 inside contraction
  auto candidate = [&](int k) {
    for (int e = 0; e < N; e++) {
      const double c = s.cen[e], w = s.pts[N][e];
      s.xs[k][e] = clampq(e, k == 0   ? c + (c - w)
                             : k == 1 ? c + 2.0 * (c - w)
                             : k == 2 ? c + 0.5 * (s.xs[0][e] - c)
                                      : c + 0.5 * (w - c));
    }
  };
  auto candidate_value = [&](int k) {
    if constexpr (B == 1)
      if (t == 0) candidate(k);
    return ev.value(s.xs, k);
  };
  if (t == 0) {
    for (int i = 0; i < N; i++) {
      const double x0 = s.pts[0][i];
      const double step = fmin(0.25 * (s.ub[i] - s.lb[i]), fmin(0.75 * (s.ub[i] - x0), 0.75 * (x0 - s.lb[i])));
      for (int e = 0; e < N; e++) s.pts[i + 1][e] = s.pts[0][e] + (e == i ? step : 0.0);
    }
  }
  __syncthreads();  // the evaluator's LDS state set up by the caller is visible before failed() reads it
  for (int i0 = 0; i0 <= N && !ev.failed(); i0 += B) {  // the initial simplex (one batch on the host: the same values)
    const int cnt = min(B, N + 1 - i0);
    if (t == 0)
      for (int k = 0; k < cnt; k++)
        for (int e = 0; e < N; e++) s.xs[k][e] = s.pts[i0 + k][e];
    place(i0, cnt);
  }
  int nev = N + 1;
  // nev and failed() (read after an evaluation's barrier) are identical in
  // every thread; a failed evaluation ends the search in the whole workgroup
  while (nev < max_eval && !ev.failed()) {
    __syncthreads();
    if (t == 0) {
      for (int i = 1; i <= N; i++) {  // stable insertion sort (np.argsort kind="stable")
        for (int j = i; j > 0 && s.vals[j] < s.vals[j - 1]; j--) {
          const double tv = s.vals[j];
          s.vals[j] = s.vals[j - 1];
          s.vals[j - 1] = tv;
          for (int e = 0; e < N; e++) {
            const double tp = s.pts[j][e];
            s.pts[j][e] = s.pts[j - 1][e];
            s.pts[j - 1][e] = tp;
          }
        }
      }
      for (int e = 0; e < N; e++) {  // np.mean(pts[:-1], axis=0): rows added in order, then / n
        double sm = s.pts[0][e];
        for (int i = 1; i < N; i++) sm = sm + s.pts[i][e];
        s.cen[e] = sm / (double)N;
      }
      if constexpr (B > 1)
        for (int k = 0; k < 4; k++) candidate(k);
    }
    if constexpr (B > 1) ev.prefetch(s.xs, 4);
    const double fr = candidate_value(0);
    nev++;
    if constexpr (Ev::kBarrierAfterReflection) __syncthreads();
    const double v0 = s.vals[0], vn1 = s.vals[N - 1];
    // Thread 0 updates only the worst row before the next barrier, so v0 and
    // vn1 are safe; vn is read where no update can be under way.  In batches
    // that is here, before a barrier (value() has none).  On demand it is in
    // the contraction branch, where thread 0's update waits behind value().
    double vn = 0.0;
    if constexpr (B > 1) {
      vn = s.vals[N];
      __syncthreads();
    }
    if (fr < v0 && nev < max_eval) {
      const double fe = candidate_value(1);
      nev++;
      if (t == 0) {
        const bool take_e = fe < fr;
        for (int e = 0; e < N; e++) s.pts[N][e] = take_e ? s.xs[1][e] : s.xs[0][e];
        s.vals[N] = take_e ? fe : fr;
      }
    } else if (fr < vn1) {
      if (t == 0) {
        for (int e = 0; e < N; e++) s.pts[N][e] = s.xs[0][e];
        s.vals[N] = fr;
      }
    } else if (nev < max_eval) {
      if constexpr (B == 1) vn = s.vals[N];
      const int kc = fr >= vn ? 3 : 2;
      const double fc = candidate_value(kc);
      nev++;
      if (fc < fmin(fr, vn)) {
        if (t == 0) {
          for (int e = 0; e < N; e++) s.pts[N][e] = s.xs[kc][e];
          s.vals[N] = fc;
        }
      } else {
        const int m = min(N, max_eval - nev);
        for (int i0 = 1; i0 <= m && !ev.failed(); i0 += B) {  // shrink toward the best (one batch on the host)
          const int cnt = min(B, m + 1 - i0);
          __syncthreads();
          if (t == 0)
            for (int k = 0; k < cnt; k++)
              for (int e = 0; e < N; e++)
                s.xs[k][e] = clampq(e, s.pts[0][e] + 0.5 * (s.pts[i0 + k][e] - s.pts[0][e]));
          place(i0, cnt);
        }
        nev += m > 0 ? m : 0;
      }
    }
  }
  __syncthreads();
  return nev;
}

// np.argmin over the simplex values: the first minimum
template <int N>
__device__ __forceinline__ int best(const Simplex<N>& s) {
  int b = 0;
  for (int i = 1; i <= N; i++)
    if (s.vals[i] < s.vals[b]) b = i;
  return b;
}

}  // namespace pcnn_nm
