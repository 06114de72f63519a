// Point-to-point ICP (include/gaussreg_hip_icp.h): the loop  match -> fp64 sums -> Umeyama -> stop test
// without leaving the device.  The support grid of cloud_nn.hip (cloud_grid.hpp) is built ONCE over ref; the source points
// are put ONCE into the order ascending (cell of p_i under T_0, i) by the stable radix sort of sort.hip -- not by the
// atomic-cursor scatter, whose order inside a cell varies between runs: the sums below are taken in this order, so it has
// to be the same in every call.
//
//   icp_init_kernel       T <- T_0
//   icp_key_kernel        one thread per source point: finiteness flag, key = cell of the point under T_0
//   (sort_pairs_u64_iota: stable, so equal cells keep ascending i)
//   icp_gather_kernel     (x, y, z, i) of the source into that order
//   per round t = 0 .. max_iterations, every kernel starting with a uniform "flag raised or done: return":
//   icp_match_kernel      one thread per ordered source point: p = T_t src, its cell by binary search of the boundaries,
//                         the CAP = 1 shell search with the face and box bound -> match_j / match_d at its position; a
//                         query no rule stops within MAX_SHELLS shells is appended to the list
//   icp_fallback_kernel   one WAVE per listed query scans the whole support, writes the same two arrays
//   icp_sums_kernel       workgroup b reads positions [b SUM_CHUNK, (b + 1) SUM_CHUNK): n, sum src, sum ref, sum src_a ref_b,
//                         sum |src|^2 and S = sum d in fp64 (PointToPoint::add), thread t takes positions t, t + 256, ..
//                         of the chunk in order, then the DPP wave sum and the four wave totals in wave order -> one
//                         partial row
//   icp_fold_kernel       ONE workgroup: thread t adds rows t, t + 256, .. in order, same tree; thread 0 records history[t],
//                         applies the stop rule, runs umeyama_from_sums (PointToPoint::update) and stores T_(t+1), t + 1 -- or done, the status,
//                         transform_out and stats_out
//   icp_scatter_kernel    match_j / match_d of the reported evaluation back into the caller's source order
// The host enqueues max_iterations + 1 rounds blindly -- round max_iterations always stops -- and then makes the call's one
// read-back: flag, status, iteration count.
//
// All of it but the estimator below -- its sums, what a matched pair adds to them, its update -- lives in cloud_icp_shared.hpp, which
// cloud_icp_plane.hip (point-to-plane) instantiates with another estimator.
//
// Reproducibility: the order of the source, the chunking, the trees and the fold depend on the shapes alone; a listed
// query's match lands at its own position whatever the order of the list; only integer atomics are used.
#include "cloud_icp_shared.hpp"

namespace gr {
namespace {

struct PointToPoint {
  static constexpr int NSUM = 18, I_N = 0, I_S = 17;  // n, sum src (3), sum ref (3), sum src_a ref_b (9), sum |src|^2, S
  static constexpr double MIN_PAIRS = 3.0;
  struct Args {
    int with_scale;
  };
  static constexpr const char* ARG_NAMES = "";
  static bool args_ok(const Args&) { return true; }
  static void after_grid(const Args&, int64_t, int32_t*, hipStream_t) {}
  static const char* flag_text(int32_t) { return "points must be finite"; }
  __device__ static __forceinline__ void add(double (&v)[NSUM], float4 q, int32_t j, float d, const float* __restrict__ ref,
                                             const float*, const Args&) {
    const double a[3] = {(double)q.x, (double)q.y, (double)q.z};
    const double r[3] = {(double)ref[3 * (int64_t)j], (double)ref[3 * (int64_t)j + 1], (double)ref[3 * (int64_t)j + 2]};
    v[0] += 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[1 + c] += a[c];
      v[4 + c] += r[c];
#pragma unroll
      for (int e = 0; e < 3; ++e) v[7 + c * 3 + e] += a[c] * r[e];
    }
    v[16] += (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    v[17] += (double)d;
  }
  __device__ static bool update(const double* sum, const float*, const Args& a, float* Tn) {
    return umeyama_from_sums(sum[0], sum + 1, sum + 4, sum + 7, sum[16], a.with_scale, Tn);
  }
};

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_cloud_icp_workspace_bytes(int64_t n_src, int64_t n_ref, int max_iterations) {
  return icp_workspace_bytes<PointToPoint>(n_src, n_ref, max_iterations);
}

extern "C" int gr_cloud_icp(const float* src, int64_t nq, const float* ref, int64_t ns, const float* h_transform0,
                            float max_dist2, int with_scale, int max_iterations, double relative_fitness,
                            double relative_rmse, float* transform_out, double* stats_out, int64_t* index, float* dist2,
                            double* history, int* h_status, void* ws, size_t ws_bytes, void* stream) {
  return icp_run<PointToPoint>("cloud icp", "cloud_icp_grid", "cloud_icp_iterate", src, nq, ref, ns, h_transform0, max_dist2,
                               {with_scale}, max_iterations, relative_fitness, relative_rmse, transform_out, stats_out, index,
                               dist2, history, h_status, ws, ws_bytes, static_cast<hipStream_t>(stream));
}
