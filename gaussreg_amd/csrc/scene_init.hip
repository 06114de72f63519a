// Scene initialisation from a point cloud: the exact k nearest neighbours of every point of ONE cloud,
// what upstream 3DGS's create_from_pcd takes from simple_knn.distCUDA2.
//
// The result is defined by exhaustive enumeration (include/gaussreg_hip.h): d(i, j) = ((dx*dx + dy*dy) + dz*dz) in fp32,
// neighbours = the k smallest j != i under the order (d, j).
//
// The search is that of cloud_grid.hpp (the grid, the shell loop, the face bound and its proof are there) with the cloud
// as both support and query cloud, in its SELF form:
//   * the query's own index is excluded -- by index, so a twin at distance 0 is a neighbour like any other;
//   * there is no cap, so the block a search is confined to is the whole grid;
//   * the support's bounding box is neither built nor read: a query that is a support point lies inside the box, every
//     box term of the stopping bound would be exactly +0, and (f + 0) + 0 == f in fp32.
// So the grid is built by cloud_build_support_grid (which keeps the cell of every sorted point here, since the points are
// their own queries), and gs_knn_query_kernel<CAP> is one thread per cell-ordered point around shell_search.  A query that
// has not stopped after MAX_SHELLS shells (an outlier among empty cells, a cloud of identical points) starts over and
// scans every point, in its own lane.
#include "cloud_grid.hpp"

namespace gr {
namespace {

template <int CAP>
__global__ __launch_bounds__(QUERY_THREADS) void gs_knn_query_kernel(const float4* __restrict__ sorted,
                                                                     const int32_t* __restrict__ sorted_cell,
                                                                     const int32_t* __restrict__ start, const float* __restrict__ B,
                                                                     int32_t n, int D, int k, float* __restrict__ dist2,
                                                                     int64_t* __restrict__ index, float* __restrict__ mean) {
  const int64_t s = (int64_t)blockIdx.x * QUERY_THREADS + threadIdx.x;
  if (s >= n) return;
  const float4 q = sorted[s];
  const int32_t qi = __float_as_int(q.w);
  float bd[CAP];
  int32_t bj[CAP];
  clear_best<CAP>(bd, bj);
  if (!shell_search<CAP, true>(sorted, start, B, nullptr, D, sorted_cell[s], q.x, q.y, q.z, INFINITY, bd, bj, qi)) {
    clear_best<CAP>(bd, bj);
    scan_range<CAP, true>(sorted, 0, n, q.x, q.y, q.z, INFINITY, bd, bj, qi);
  }
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < CAP; ++t) {
    if (t < k) {
      if (dist2) dist2[(int64_t)qi * k + t] = bd[t];
      if (index) index[(int64_t)qi * k + t] = bj[t];
      sum = t == 0 ? bd[0] : sum + bd[t];
    }
  }
  if (mean) mean[qi] = sum / (float)k;
}

struct KnnWorkspace {
  SupportGrid g;      // over the cloud, sorted_cell kept; misc[0] is the finiteness flag
  size_t zero_bytes;  // from g.count: counts, cursors and misc
  size_t bytes;
};

KnnWorkspace carve_knn(void* ws, int64_t n) {
  const int D = cloud_grid_dim(n);
  const size_t cells = (size_t)D * D * D;
  Carver c(ws);
  KnnWorkspace w;
  w.g.B = c.take<float>(3 * DMAX);
  w.g.count = c.take<int32_t>(2 * cells + 1 + MISC);
  w.g.cursor = w.g.count + cells + 1;
  w.g.misc = w.g.cursor + cells;
  w.zero_bytes = (2 * cells + 1 + MISC) * sizeof(int32_t);
  w.g.scan_ws = c.take<int32_t>(scan_ws_ints((int64_t)cells + 1));
  w.g.cell = c.take<int32_t>((size_t)n);
  w.g.sorted_cell = c.take<int32_t>((size_t)n);
  w.g.sorted = c.take<float4>((size_t)n);
  w.bytes = c.used();
  return w;
}

bool knn_shape_ok(int64_t n, int k) { return k >= 1 && k <= GR_GS_KNN_MAX_K && n > k && n < (1ll << 31); }

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_gs_knn_workspace_bytes(int64_t n, int k) {
  if (!knn_shape_ok(n, k)) return 0;
  return carve_knn(nullptr, n).bytes;
}

extern "C" int gr_gs_knn(const float* points, int64_t n, int k, float* dist2, int64_t* index, float* mean, void* ws,
                         size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(k >= 1 && k <= GR_GS_KNN_MAX_K, "gs knn: k = %d outside [1, %d]", k, GR_GS_KNN_MAX_K);
  GR_REQUIRE(n > k && n < (1ll << 31), "gs knn: n = %lld outside (k, 2^31)", (long long)n);
  GR_REQUIRE(points, "gs knn: null points");
  const KnnWorkspace w = carve_knn(ws, n);
  if (!ws || ws_bytes < w.bytes) {
    set_error("gs knn: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
    return GR_ERR_WORKSPACE;
  }
  {
    KernelTimer timer("gs_knn_grid", stream);
    const int rc = cloud_build_support_grid(points, n, w.g, w.g.count, w.zero_bytes, stream, /*with_box=*/false);
    if (rc != GR_OK) return rc;
  }
  // the one host read-back of a call
  int32_t h_flag = 0;
  GR_HIP(hipMemcpyAsync(&h_flag, w.g.misc, sizeof h_flag, hipMemcpyDeviceToHost, stream));
  GR_HIP(hipStreamSynchronize(stream));
  GR_REQUIRE(h_flag == 0, "gs knn: points must be finite");
  if (!dist2 && !index && !mean) return GR_OK;
  const int D = cloud_grid_dim(n);
  const unsigned qblocks = (unsigned)((n + QUERY_THREADS - 1) / QUERY_THREADS);
  KernelTimer timer("gs_knn_query", stream);
#define GR_KNN_LAUNCH(CAP)                                                                                                   \
  hipLaunchKernelGGL(gs_knn_query_kernel<CAP>, dim3(qblocks), dim3(QUERY_THREADS), 0, stream, w.g.sorted, w.g.sorted_cell,   \
                     w.g.count, w.g.B, (int32_t)n, D, k, dist2, index, mean)
  if (k == 1) GR_KNN_LAUNCH(1);
  else if (k <= 3) GR_KNN_LAUNCH(3);
  else if (k <= 5) GR_KNN_LAUNCH(5);
  else GR_KNN_LAUNCH(8);
#undef GR_KNN_LAUNCH
  GR_LAUNCH_CHECK();
  return GR_OK;
}
