// gr_node_correspondences: the ground-truth superpoint (patch) correspondences of a training step, fused
// (get_node_correspondences, geotransformer/modules/registration/matching.py:231-315).  The reference gathers two
// (B, K, 3) point sets for every pair of patches whose enclosing spheres touch and builds a (B, K, K) distance tensor and
// two boolean tensors of that shape; here no per-pair tensor exists:
//   1. nc_prepare_kernel (one wave per node): the transformed source nodes and patches, written once, and per node the
//      enclosing radius over its valid points and the number of valid points (0 for a masked node).
//   2. nc_pair_kernel (one 256-thread workgroup per reference node): the valid points of the reference patch are
//      compacted into LDS.  Each wave takes blocks of 64 source nodes: every lane runs the sphere test of one, a ballot
//      lists the survivors, and for each survivor the lanes hold the source points (K / 64 per lane) and walk the
//      reference points with broadcast LDS reads.  "Source point has a partner" is a lane-private flag, "reference point
//      has a partner" a ballot.  The wave writes the overlaps of its 64 pairs (0 where the pair was pruned) in one
//      coalesced store, and the workgroup the number of pairs with overlap > 0 of its row.
//   3. an exclusive scan of the row counts, then nc_compact_kernel (one wave per row): ballot-ranked, ordered writes.
// No float atomics and no atomics for ordering: every output word has one writer, two calls leave the same bits.
// The distance is differences first, then squares ((dx*dx + dy*dy) + dz*dz, no FMA: -ffp-contract=off).
#include <algorithm>

#include "../../include/gaussreg_hip_train_matching.h"
#include "common.hpp"

namespace gr {
namespace {

constexpr int NC_MAXK = 256;
constexpr int NC_T = 256;  // threads of a pair workgroup: 4 waves
constexpr int NC_WAVES = NC_T / WAVE;

__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// info[node] = {x, y, z, radius}; cnt[node] = valid points (0: the node is masked or its patch is empty)
__global__ __launch_bounds__(WAVE) void nc_prepare_kernel(const float* __restrict__ ref_nodes, const float* __restrict__ src_nodes,
                                                          const float* __restrict__ ref_pts, const float* __restrict__ src_pts,
                                                          int M, int N, int K, const float* __restrict__ T,
                                                          const uint8_t* __restrict__ ref_masks, const uint8_t* __restrict__ src_masks,
                                                          const uint8_t* __restrict__ ref_knn_masks,
                                                          const uint8_t* __restrict__ src_knn_masks, float4* __restrict__ ref_info,
                                                          int32_t* __restrict__ ref_cnt, float4* __restrict__ src_info,
                                                          int32_t* __restrict__ src_cnt, float* __restrict__ tsrc) {
  const int lane = threadIdx.x;
  const bool is_src = (int)blockIdx.x >= M;
  const int node = is_src ? (int)blockIdx.x - M : (int)blockIdx.x;
  const float* nodes = is_src ? src_nodes : ref_nodes;
  const float* pts = (is_src ? src_pts : ref_pts) + (size_t)node * K * 3;
  const uint8_t* nmask = is_src ? src_masks : ref_masks;
  const uint8_t* kmask = is_src ? src_knn_masks : ref_knn_masks;
  float r[12];
  if (is_src) {
#pragma unroll
    for (int a = 0; a < 12; ++a) r[a] = T[a];
  }
  float cx = nodes[3 * (size_t)node], cy = nodes[3 * (size_t)node + 1], cz = nodes[3 * (size_t)node + 2];
  if (is_src) {
    const float x = cx, y = cy, z = cz;
    cx = r[0] * x + r[1] * y + r[2] * z + r[3];
    cy = r[4] * x + r[5] * y + r[6] * z + r[7];
    cz = r[8] * x + r[9] * y + r[10] * z + r[11];
  }
  float rad = 0.f;
  int cnt = 0;
  for (int s = lane; s < K; s += WAVE) {
    float x = pts[3 * s], y = pts[3 * s + 1], z = pts[3 * s + 2];
    if (is_src) {
      const float tx = r[0] * x + r[1] * y + r[2] * z + r[3];
      const float ty = r[4] * x + r[5] * y + r[6] * z + r[7];
      const float tz = r[8] * x + r[9] * y + r[10] * z + r[11];
      x = tx, y = ty, z = tz;
      float* o = tsrc + ((size_t)node * K + s) * 3;
      o[0] = x, o[1] = y, o[2] = z;
    }
    const bool valid = kmask == nullptr || kmask[(size_t)node * K + s] != 0;
    if (valid) {
      const float dx = x - cx, dy = y - cy, dz = z - cz;
      rad = fmaxf(rad, sqrtf(dx * dx + dy * dy + dz * dz));  // (fmaxf drops a NaN: the sphere test only prunes)
      ++cnt;
    }
  }
  rad = wave_max_f32(rad);
  cnt = wave_sum_i32_dpp(cnt);
  if (nmask != nullptr && nmask[node] == 0) cnt = 0;
  if (lane == 0) {
    (is_src ? src_info : ref_info)[node] = make_float4(cx, cy, cz, rad);
    (is_src ? src_cnt : ref_cnt)[node] = cnt;
  }
}

// the counts of one candidate pair: rc = reference points with a partner, sc = source points with one.  NCH = ceil(K / 64)
template <int NCH>
__device__ __forceinline__ void nc_pair_counts(const float* __restrict__ rx, const float* __restrict__ ry,
                                               const float* __restrict__ rz, int kr, const float* __restrict__ tp,
                                               const uint8_t* __restrict__ smask, int K, float r2, int lane, int& rc, int& sc) {
  float qx[NCH], qy[NCH], qz[NCH];
  bool qv[NCH], flag[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int s = c * WAVE + lane;
    const bool in = s < K;
    qv[c] = in && (smask == nullptr || smask[s] != 0);
    qx[c] = in ? tp[3 * s] : 0.f;
    qy[c] = in ? tp[3 * s + 1] : 0.f;
    qz[c] = in ? tp[3 * s + 2] : 0.f;
    flag[c] = false;
  }
  int count = 0;
  for (int r = 0; r < kr; ++r) {
    const float px = rx[r], py = ry[r], pz = rz[r];  // one address for the wave: LDS broadcast
    bool any = false;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float dx = px - qx[c], dy = py - qy[c], dz = pz - qz[c];
      const bool hit = qv[c] && (dx * dx + dy * dy + dz * dz < r2);
      flag[c] |= hit;
      any |= hit;
    }
    count += __ballot(any) != 0ull ? 1 : 0;
  }
  rc = count;
  sc = 0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) sc += __popcll(__ballot(flag[c]));
}

__global__ __launch_bounds__(NC_T) void nc_pair_kernel(const float* __restrict__ ref_pts, const uint8_t* __restrict__ ref_knn_masks,
                                                       const uint8_t* __restrict__ src_knn_masks, int N, int K, float r2,
                                                       const float4* __restrict__ ref_info, const int32_t* __restrict__ ref_cnt,
                                                       const float4* __restrict__ src_info, const int32_t* __restrict__ src_cnt,
                                                       const float* __restrict__ tsrc, float* __restrict__ overlaps,
                                                       int32_t* __restrict__ row_cnt) {
  __shared__ float rx[NC_MAXK], ry[NC_MAXK], rz[NC_MAXK];
  __shared__ int wave_n[NC_WAVES];
  const int i = blockIdx.x;
  const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
  const int rv = ref_cnt[i];  // valid reference points; 0: nothing of this row can overlap
  float* orow = overlaps + (size_t)i * N;
  if (rv == 0) {
    for (int j = t; j < N; j += NC_T) orow[j] = 0.f;
    if (t == 0) row_cnt[i] = 0;
    return;
  }
  // compact the valid reference points into LDS (their order does not matter: only counts leave)
  {
    const bool valid = t < K && (ref_knn_masks == nullptr || ref_knn_masks[(size_t)i * K + t] != 0);
    const unsigned long long b = __ballot(valid);
    if (lane == 0) wave_n[wave] = __popcll(b);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wave_n[w];
    if (valid) {
      const int pos = base + __popcll(b & ((1ull << lane) - 1ull));
      const float* p = ref_pts + ((size_t)i * K + t) * 3;
      rx[pos] = p[0], ry[pos] = p[1], rz[pos] = p[2];
    }
    __syncthreads();
  }
  const float4 ci = ref_info[i];
  const float pr = sqrtf(r2) * 1.0001f;
  const int nch = (K + WAVE - 1) / WAVE;
  int found = 0;  // pairs with overlap > 0 among this lane's source nodes
  for (int j0 = wave * WAVE; j0 < N; j0 += NC_T) {
    const int j = j0 + lane;
    bool cand = false;
    if (j < N && src_cnt[j] > 0) {
      const float4 cj = src_info[j];
      const float dx = ci.x - cj.x, dy = ci.y - cj.y, dz = ci.z - cj.z;
      const float d = sqrtf(dx * dx + dy * dy + dz * dz);
      // conservative: the limit is widened by far more than the fp32 error of d and of the radii; a NaN keeps the pair
      const float err = 4e-6f * (fabsf(ci.x) + fabsf(ci.y) + fabsf(ci.z) + fabsf(cj.x) + fabsf(cj.y) + fabsf(cj.z));
      cand = !(d > (ci.w + cj.w + pr) * 1.0001f + err);
    }
    unsigned long long todo = __ballot(cand);
    float mine = 0.f;
    while (todo != 0ull) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const int jj = j0 + b;
      const float* tp = tsrc + (size_t)jj * K * 3;
      const uint8_t* sm = src_knn_masks == nullptr ? nullptr : src_knn_masks + (size_t)jj * K;
      int rc, sc;
      switch (nch) {
        case 1: nc_pair_counts<1>(rx, ry, rz, rv, tp, sm, K, r2, lane, rc, sc); break;
        case 2: nc_pair_counts<2>(rx, ry, rz, rv, tp, sm, K, r2, lane, rc, sc); break;
        case 3: nc_pair_counts<3>(rx, ry, rz, rv, tp, sm, K, r2, lane, rc, sc); break;
        default: nc_pair_counts<4>(rx, ry, rz, rv, tp, sm, K, r2, lane, rc, sc); break;
      }
      const int sv = src_cnt[jj];
      const float ov = ((float)rc / (float)rv + (float)sc / (float)sv) / 2.f;
      if (lane == b) mine = ov;
    }
    if (j < N) {
      orow[j] = mine;
      found += mine > 0.f ? 1 : 0;
    }
  }
  found = wave_sum_i32_dpp(found);
  __syncthreads();  // (wave_n is read above)
  if (lane == 0) wave_n[wave] = found;
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int w = 0; w < NC_WAVES; ++w) s += wave_n[w];
    row_cnt[i] = s;
  }
}

__global__ __launch_bounds__(WAVE) void nc_compact_kernel(const float* __restrict__ overlaps, int N, const int32_t* __restrict__ row_off,
                                                          const int32_t* __restrict__ total, int64_t capacity,
                                                          int64_t* __restrict__ corr_indices, float* __restrict__ corr_overlaps,
                                                          int64_t* __restrict__ count) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i == 0 && lane == 0) *count = (int64_t)total[0];
  const float* orow = overlaps + (size_t)i * N;
  int64_t base = row_off[i];
  for (int j0 = 0; j0 < N; j0 += WAVE) {
    const int j = j0 + lane;
    const float v = j < N ? orow[j] : 0.f;
    const bool keep = v > 0.f;
    const unsigned long long b = __ballot(keep);
    const int64_t pos = base + __popcll(b & ((1ull << lane) - 1ull));
    if (keep && pos < capacity) {
      corr_indices[2 * pos] = i;
      corr_indices[2 * pos + 1] = j;
      corr_overlaps[pos] = v;
    }
    base += __popcll(b);
  }
}

struct NcWorkspace {
  float4 *ref_info, *src_info;
  int32_t *ref_cnt, *src_cnt, *row_cnt, *row_off, *total, *scan_ws;
  float *tsrc, *overlaps;
  size_t bytes;
};

NcWorkspace nc_carve(void* ws, int64_t M, int64_t N, int64_t K) {
  Carver c(ws);
  NcWorkspace w;
  w.ref_info = c.take<float4>(M);
  w.src_info = c.take<float4>(N);
  w.ref_cnt = c.take<int32_t>(M);
  w.src_cnt = c.take<int32_t>(N);
  w.row_cnt = c.take<int32_t>(M);
  w.row_off = c.take<int32_t>(M);
  w.total = c.take<int32_t>(1);
  w.scan_ws = c.take<int32_t>(scan_ws_ints(M));
  w.tsrc = c.take<float>((size_t)N * K * 3);
  w.overlaps = c.take<float>((size_t)M * N);
  w.bytes = c.used() + 256;  // the carves start 256-byte aligned inside the caller's buffer
  return w;
}

bool nc_shape_ok(int64_t M, int64_t N, int64_t K) {
  return M >= 0 && N >= 0 && K >= 0 && K <= NC_MAXK && M < (1ll << 31) && N < (1ll << 31) && M * N < (1ll << 31) &&
         (M + N) < (1ll << 31);
}

}  // namespace
}  // namespace gr

using namespace gr;

extern "C" size_t gr_node_correspondences_workspace_bytes(int64_t m, int64_t n, int64_t k) {
  if (!nc_shape_ok(m, n, k)) return 0;
  return nc_carve(nullptr, m, n, k).bytes;
}

extern "C" int gr_node_correspondences(const float* ref_nodes, const float* src_nodes, const float* ref_knn_points,
                                       const float* src_knn_points, int64_t m, int64_t n, int64_t k, const float* transform_dev,
                                       float pos_radius_sq, const uint8_t* ref_masks, const uint8_t* src_masks,
                                       const uint8_t* ref_knn_masks, const uint8_t* src_knn_masks, int64_t* corr_indices,
                                       float* corr_overlaps, int64_t capacity, int64_t* count_dev, float* dense_overlaps,
                                       void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  GR_REQUIRE(m >= 0 && n >= 0 && k >= 0 && capacity >= 0, "node_correspondences: bad sizes");
  if (k > NC_MAXK) {
    set_error("node_correspondences: patches of more than %d points are not supported (K = %lld)", NC_MAXK, (long long)k);
    return GR_ERR_UNSUPPORTED;
  }
  GR_REQUIRE(nc_shape_ok(m, n, k), "node_correspondences: sizes too large (M * N must stay below 2^31)");
  GR_REQUIRE(count_dev, "node_correspondences: null argument");
  if (m == 0 || n == 0 || k == 0) {
    GR_HIP(hipMemsetAsync(count_dev, 0, sizeof(int64_t), stream));
    if (dense_overlaps && m * n > 0) GR_HIP(hipMemsetAsync(dense_overlaps, 0, (size_t)m * n * sizeof(float), stream));
    return GR_OK;
  }
  GR_REQUIRE(ref_nodes && src_nodes && ref_knn_points && src_knn_points && transform_dev, "node_correspondences: null argument");
  GR_REQUIRE(capacity == 0 || (corr_indices && corr_overlaps), "node_correspondences: null argument");
  const size_t need = gr_node_correspondences_workspace_bytes(m, n, k);
  if (!ws || ws_bytes < need) {
    set_error("node_correspondences: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    return GR_ERR_WORKSPACE;
  }
  NcWorkspace w = nc_carve(reinterpret_cast<void*>(align_up(reinterpret_cast<size_t>(ws), 256)), m, n, k);
  float* overlaps = dense_overlaps ? dense_overlaps : w.overlaps;
  KernelTimer timer("node_correspondences", stream);
  hipLaunchKernelGGL(nc_prepare_kernel, dim3((unsigned)(m + n)), dim3(WAVE), 0, stream, ref_nodes, src_nodes, ref_knn_points,
                     src_knn_points, (int)m, (int)n, (int)k, transform_dev, ref_masks, src_masks, ref_knn_masks, src_knn_masks,
                     w.ref_info, w.ref_cnt, w.src_info, w.src_cnt, w.tsrc);
  hipLaunchKernelGGL(nc_pair_kernel, dim3((unsigned)m), dim3(NC_T), 0, stream, ref_knn_points, ref_knn_masks, src_knn_masks, (int)n,
                     (int)k, pos_radius_sq, w.ref_info, w.ref_cnt, w.src_info, w.src_cnt, w.tsrc, overlaps, w.row_cnt);
  GR_LAUNCH_CHECK();
  const int rc = exclusive_scan_i32(w.row_cnt, w.row_off, m, 1, m, w.scan_ws, w.total, stream);
  if (rc != GR_OK) return rc;
  hipLaunchKernelGGL(nc_compact_kernel, dim3((unsigned)m), dim3(WAVE), 0, stream, overlaps, (int)n, w.row_off, w.total, capacity,
                     corr_indices, corr_overlaps, count_dev);
  GR_LAUNCH_CHECK();
  return GR_OK;
}
