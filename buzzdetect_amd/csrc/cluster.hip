// k-means clustering for gfx950 (include/buzzdetect_cluster.h): one Lloyd iteration over [W][1024] embeddings where they lie.
//
//   cluster_assign_kernel     a wave owns 32 rows and walks the column tiles of the packed centroids one after another, each by
//                             dense_tile_walk (dense_device.h: the bits of bd_search_scores).  A lane keeps the best (t, j) of
//                             its own columns for its 16 rows in registers; at the end the 32 lanes of a half meet in a
//                             butterfly on (t, j) pairs, lower j winning ties.  No [W][K] matrix exists anywhere.
//   cluster_count_kernel      a workgroup per slice of 1024 rows counts its labels in LDS (integer additions: any order).
//   cluster_scan_kernel       one workgroup: per cluster the total over the slices, the clusters' exclusive scan (offsets), and
//                             in place of every slice's count the place of the slice's first row with that label.
//   cluster_place_kernel      one wave per slice, 64 rows a round in ascending order: a row's place is its label's cursor plus
//                             the number of lower lanes with the same label; the last such lane moves the cursor on.
//   cluster_chunks_kernel     one workgroup: the first chunk of every cluster (an exclusive scan of ceil(count / 256)).
//   cluster_partial_kernel    a workgroup per (cluster, chunk): 256 threads of four channels each add up to 256 whole rows in
//                             ascending member order, read through `order` at 4 KB a row.
//   cluster_finish_kernel     a workgroup per cluster: the chain over its partials, the centroid, its squared norm, and its
//                             place in the packed form; workgroups K .. 32 ceil(K / 32) - 1 write the padding's zeros.
//   cluster_stats_kernel      a wave per slice of 256 rows: four additions a lane, one butterfly; an integer count beside it.
//
// No floating-point number is added atomically, no result depends on the grid, every output element has one writer, inputs are
// only read, element offsets are 64-bit, and every index read from memory (a label, a row id, an offset) is brought into range
// before it addresses anything.
#include "bd_internal.h"
#include "bd_error.h"
#include "cluster_device.h"
#include "dense_device.h"
#include "simsearch_device.h"

#include "../../include/buzzdetect_cluster.h"

#include <algorithm>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kThreads = 256;
constexpr int kQuads = BD_CLUSTER_DIM / 4;               // float4 per row: one per thread of a workgroup
constexpr int kScanThreads = BD_CLUSTER_MAX_CLUSTERS;    // a thread per cluster
static_assert(kQuads == kThreads, "a thread owns four channels of a row");
static_assert(cluster::kSuper % 4 == 0, "dense_tile_walk takes whole groups of four super-steps");
static_assert(BD_CLUSTER_ORDER_SLICE % 64 == 0 && BD_CLUSTER_ORDER_SLICE % kThreads == 0, "a slice is whole rounds");
static_assert((kScanThreads & (kScanThreads - 1)) == 0 && kScanThreads <= 1024, "the scan doubles its stride");

__global__ __launch_bounds__(kThreads) void cluster_assign_kernel(const float* __restrict__ E, int W, const float* __restrict__ n2,
                                                                   const float4* __restrict__ Cf, const float* __restrict__ c2,
                                                                   int K, int n_super, int metric,
                                                                   int32_t* __restrict__ labels, float* __restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const int tr = 4 * blockIdx.x + (threadIdx.x >> 6);   // 32-row tile: the four waves of a workgroup read neighbouring rows
    if (32 * tr >= W) return;                             // (no barrier in this kernel)
    const int half = lane >> 5;
    const int arow = min(32 * tr + (lane & 31), W - 1);   // always in bounds; rows past W are never stored
    const float* ap = E + (size_t)arow * BD_CLUSTER_DIM + 4 * half;

    float bt[16];
    int bj[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        bt[r] = INFINITY;
        bj[r] = lane & 31;                                // the lane's column of tile 0: what wins if everything is +INFINITY
    }
    const int tiles = (K + 31) / 32;
#pragma unroll 1
    for (int tc = 0; tc < tiles; ++tc) {
        const float4* bp = Cf + (size_t)tc * n_super * 64 + lane;
        // (n_super is an argument, as in headset.hip: known at compile time, the walk unrolls whole and spills)
        const dense_v16f acc = dense_tile_walk(ap, bp, BD_CLUSTER_DIM, n_super, half);
        const int col = 32 * tc + (lane & 31);
        if (col < K) {                                    // a padded column never enters: it stays (+INFINITY, j >= K) at most
            const float cc = metric == BD_CLUSTER_EUCLIDEAN ? c2[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float t = metric == BD_CLUSTER_EUCLIDEAN ? cc - 2.0f * acc[r] : -acc[r];
                if (t != t) t = INFINITY;
                if (t < bt[r]) {                          // the lane's columns ascend: a tie keeps the lower one
                    bt[r] = t;
                    bj[r] = col;
                }
            }
        }
    }
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) {                   // within a half: the 32 columns of the lanes' running bests
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float ot = __shfl_xor(bt[r], m, 64);
            const int oj = __shfl_xor(bj[r], m, 64);
            if (ot < bt[r] || (ot == bt[r] && oj < bj[r])) {
                bt[r] = ot;
                bj[r] = oj;
            }
        }
    }
    // every lane of a half now holds its 16 rows' results: lane r of the half stores row r
    float t = bt[0];
    int j = bj[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) {
        if ((lane & 31) == r) {
            t = bt[r];
            j = bj[r];
        }
    }
    const int r = lane & 31;
    const int row = 32 * tr + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (r < 16 && row < W) {
        labels[row] = j;
        dist[row] = cluster::assigned_distance(n2[row], t, metric);
    }
}

__global__ __launch_bounds__(kThreads) void cluster_count_kernel(const int32_t* __restrict__ labels, int W, int K,
                                                                  int32_t* __restrict__ hist) {
    __shared__ int h[BD_CLUSTER_MAX_CLUSTERS];
    const int tid = threadIdx.x;
    for (int j = tid; j < K; j += kThreads) h[j] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * BD_CLUSTER_ORDER_SLICE;
#pragma unroll
    for (int u = 0; u < BD_CLUSTER_ORDER_SLICE / kThreads; ++u) {
        const int64_t r = first + u * kThreads + tid;
        if (r < W) atomicAdd(&h[cluster::clamp_label(labels[r], K)], 1);      // (LDS, integers: the sum is the same in any order)
    }
    __syncthreads();
    for (int j = tid; j < K; j += kThreads) hist[(size_t)blockIdx.x * K + j] = h[j];
}

// the exclusive scan of one value per thread over a workgroup of kScanThreads; *total gets the sum.  Ends with a barrier.
__device__ __forceinline__ int scan_exclusive(int v, int tid, int (*buf)[kScanThreads], int* total) {
    buf[0][tid] = v;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kScanThreads; d <<= 1) {
        int x = buf[cur][tid];
        if (tid >= d) x += buf[cur][tid - d];
        buf[cur ^ 1][tid] = x;
        __syncthreads();
        cur ^= 1;
    }
    const int inclusive = buf[cur][tid];
    *total = buf[cur][kScanThreads - 1];
    __syncthreads();
    return inclusive - v;
}

__global__ __launch_bounds__(kScanThreads) void cluster_scan_kernel(int32_t* __restrict__ hist, int slices, int K,
                                                                     int32_t* __restrict__ offsets) {
    __shared__ int buf[2][kScanThreads];
    const int j = threadIdx.x;
    int total = 0;
    if (j < K)
        for (int s = 0; s < slices; ++s) total += hist[(size_t)s * K + j];
    int all;
    const int first = scan_exclusive(total, j, buf, &all);
    if (j < K) offsets[j] = first;
    if (j == 0) offsets[K] = all;
    if (j < K) {
        int at = first;
        for (int s = 0; s < slices; ++s) {                // (this thread is the only one that touches column j)
            const int n = hist[(size_t)s * K + j];
            hist[(size_t)s * K + j] = at;
            at += n;
        }
    }
}

__global__ __launch_bounds__(64) void cluster_place_kernel(const int32_t* __restrict__ labels, int W, int K,
                                                            const int32_t* __restrict__ base, int32_t* __restrict__ order) {
    __shared__ int cursor[BD_CLUSTER_MAX_CLUSTERS];
    const int lane = threadIdx.x;
    for (int j = lane; j < K; j += 64) cursor[j] = base[(size_t)blockIdx.x * K + j];
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * BD_CLUSTER_ORDER_SLICE;
    for (int round = 0; round < BD_CLUSTER_ORDER_SLICE / 64 && first + 64 * round < W; ++round) {
        const int64_t r = first + 64 * round + lane;
        const bool valid = r < W;
        const int label = valid ? cluster::clamp_label(labels[r], K) : -1;
        int rank = 0, same = 0;
        for (int i = 0; i < 64; ++i) {
            const int li = __shfl(label, i, 64);
            same += li == label ? 1 : 0;
            rank += li == label && i < lane ? 1 : 0;
        }
        if (valid) {
            const int at = cursor[label] + rank;
            if (at >= 0 && at < W) order[at] = (int32_t)r;     // (always, for counts of these labels)
        }
        __syncthreads();
        if (valid && rank == same - 1) cursor[label] += same;  // the last lane with this label: one writer per cursor
        __syncthreads();
    }
}

// a cluster's segment as the kernels read it: inside [0, W] and not negative in length, whatever the offsets hold
__device__ __forceinline__ void segment(const int32_t* __restrict__ offsets, int j, int W, int* lo, int* hi) {
    *lo = min(max(offsets[j], 0), W);
    *hi = min(max(offsets[j + 1], *lo), W);
}

__global__ __launch_bounds__(kScanThreads) void cluster_chunks_kernel(const int32_t* __restrict__ offsets, int W, int K,
                                                                       int32_t* __restrict__ chunk_first) {
    __shared__ int buf[2][kScanThreads];
    const int j = threadIdx.x;
    int n = 0;
    if (j < K) {
        int lo, hi;
        segment(offsets, j, W, &lo, &hi);
        n = cluster::chunks_of(hi - lo);
    }
    int all;
    const int first = scan_exclusive(n, j, buf, &all);
    if (j < K) chunk_first[j] = first;
    if (j == 0) chunk_first[K] = all;
}

__global__ __launch_bounds__(kThreads) void cluster_partial_kernel(const float4* __restrict__ E, int W, const float* __restrict__ n2,
                                                                    const int32_t* __restrict__ order,
                                                                    const int32_t* __restrict__ offsets,
                                                                    const int32_t* __restrict__ chunk_first, int K, int metric,
                                                                    float4* __restrict__ partial) {
    __shared__ int s_row[BD_CLUSTER_CHUNK];
    __shared__ float s_rinv[BD_CLUSTER_CHUNK];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    if (b >= chunk_first[K]) return;                      // (the whole workgroup: the grid is the largest number of chunks)
    int lo = 0, hi = K;                                   // the last cluster whose first chunk is <= b: it is not empty
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_first[mid] <= b) lo = mid; else hi = mid;
    }
    const int j = lo;
    int seg_lo, seg_hi;
    segment(offsets, j, W, &seg_lo, &seg_hi);
    const int start = min(seg_lo + (b - chunk_first[j]) * BD_CLUSTER_CHUNK, seg_hi);
    const int n = min(BD_CLUSTER_CHUNK, seg_hi - start);
    if (tid < n) {
        const int r = min(max(order[start + tid], 0), W - 1);
        s_row[tid] = r;
        s_rinv[tid] = metric == BD_CLUSTER_COSINE ? cluster::row_rinv(n2[r]) : 1.0f;
    }
    __syncthreads();
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 8
    for (int i = 0; i < n; ++i) {
        const float4 x = E[(size_t)s_row[i] * kQuads + tid];
        const float ri = s_rinv[i];
        acc.x = cluster::chain_add(acc.x, cluster::member_term(x.x, ri, metric));
        acc.y = cluster::chain_add(acc.y, cluster::member_term(x.y, ri, metric));
        acc.z = cluster::chain_add(acc.z, cluster::member_term(x.z, ri, metric));
        acc.w = cluster::chain_add(acc.w, cluster::member_term(x.w, ri, metric));
    }
    partial[(size_t)b * kQuads + tid] = acc;
}

__global__ __launch_bounds__(kThreads) void cluster_finish_kernel(const float4* __restrict__ partial, int max_chunks,
                                                                   const int32_t* __restrict__ offsets,
                                                                   const int32_t* __restrict__ chunk_first, int W, int K,
                                                                   int metric, const float4* __restrict__ prev,
                                                                   float4* __restrict__ centroids, float4* __restrict__ packed,
                                                                   float* __restrict__ c2) {
    __shared__ __attribute__((aligned(16))) float s_rowf[BD_CLUSTER_DIM];
    __shared__ float s_m2;
    const int tid = threadIdx.x;
    const int j = blockIdx.x;
    if (j >= K) {                                         // the padding of the last column tile
        packed[cluster::packed_quad(j, tid)] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    int lo, hi;
    segment(offsets, j, W, &lo, &hi);
    const int count = hi - lo;
    const int first = chunk_first[j];
    const int chunks = min(cluster::chunks_of(count), max(max_chunks - first, 0));
    float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (chunks > 0) sum = partial[(size_t)first * kQuads + tid];
    for (int c = 1; c < chunks; ++c) {
        const float4 p = partial[(size_t)(first + c) * kQuads + tid];
        sum.x = cluster::chain_add(sum.x, p.x);
        sum.y = cluster::chain_add(sum.y, p.y);
        sum.z = cluster::chain_add(sum.z, p.z);
        sum.w = cluster::chain_add(sum.w, p.w);
    }
    float4* s_row = reinterpret_cast<float4*>(s_rowf);
    float m2 = 0.0f;
    if (metric == BD_CLUSTER_COSINE) {                    // (uniform)
        s_row[tid] = sum;
        __syncthreads();
        if (tid < 64) {
            const float v = search::butterfly_wave(search::norm_chain(s_rowf, tid));
            if (tid == 0) s_m2 = v;
        }
        __syncthreads();
        m2 = s_m2;
    }
    float4 c;
    if (cluster::keeps_previous(count, m2, metric)) {
        c = prev[(size_t)j * kQuads + tid];
    } else {
        const float d = cluster::centroid_denominator(count, m2, metric);
        c.x = cluster::centroid_value(sum.x, d);
        c.y = cluster::centroid_value(sum.y, d);
        c.z = cluster::centroid_value(sum.z, d);
        c.w = cluster::centroid_value(sum.w, d);
    }
    centroids[(size_t)j * kQuads + tid] = c;
    packed[cluster::packed_quad(j, tid)] = c;
    s_row[tid] = c;                                       // (wave 0's reads of the sum row lie before the barrier above)
    __syncthreads();
    if (tid < 64) {
        const float v = search::butterfly_wave(search::norm_chain(s_rowf, tid));
        if (tid == 0) c2[j] = v;
    }
}

__global__ __launch_bounds__(kThreads) void cluster_stats_kernel(const float* __restrict__ dist, const int32_t* __restrict__ labels,
                                                                  const int32_t* __restrict__ prev, int W,
                                                                  float* __restrict__ partial, int32_t* __restrict__ changed) {
    const int lane = threadIdx.x & 63;
    const int64_t slice = 4 * (int64_t)blockIdx.x + (threadIdx.x >> 6);
    const int64_t first = slice * BD_CLUSTER_STAT_SLICE;
    if (first >= W) return;                               // (no barrier in this kernel)
    const float v = search::butterfly_wave(cluster::stat_chain(dist, first, W, lane));
    int n = cluster::stat_changed(labels, prev, first, W, lane);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m, 64);
    if (lane == 0) {
        partial[slice] = v;
        changed[slice] = n;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
int check_rows(const std::string& fn, int64_t W) {
    if (W < 0 || W > BD_CLUSTER_MAX_ROWS)
        return fail(BD_EINVAL, fn + "rows = " + std::to_string(W) + ", a call takes 0.." + std::to_string(BD_CLUSTER_MAX_ROWS));
    return BD_OK;
}

int check_clusters(const std::string& fn, int32_t K) {
    if (K < 1 || K > BD_CLUSTER_MAX_CLUSTERS)
        return fail(BD_EINVAL, fn + "n_clusters = " + std::to_string(K) + ", allowed are 1.." + std::to_string(BD_CLUSTER_MAX_CLUSTERS));
    return BD_OK;
}

int check_metric(const std::string& fn, int32_t metric) {
    if (metric != BD_CLUSTER_EUCLIDEAN && metric != BD_CLUSTER_COSINE) return fail(BD_EINVAL, fn + "unknown metric " + std::to_string(metric));
    return BD_OK;
}

int check_pointer(const std::string& fn, const char* name, const void* p, int align) {
    if (!p) return fail(BD_EINVAL, fn + name + " is null");
    if ((uintptr_t)p % (uintptr_t)align) return fail(BD_EINVAL, fn + name + " is not " + std::to_string(align) + "-byte aligned");
    return BD_OK;
}

size_t align_256(size_t n) { return (n + 255) / 256 * 256; }

// the workspace: [first chunk of every cluster and the total][a count per (order slice, cluster)][a row per chunk]
struct Layout {
    int slices, max_chunks;
    size_t chunk_first, hist, partial, total;
};

Layout layout(int64_t W, int32_t K) {
    Layout L;
    L.slices = (int)((W + BD_CLUSTER_ORDER_SLICE - 1) / BD_CLUSTER_ORDER_SLICE);
    L.max_chunks = (int)(W / BD_CLUSTER_CHUNK) + K;      // sum over clusters of ceil(n / 256) <= floor(W / 256) + K
    L.chunk_first = 0;
    L.hist = align_256((size_t)(K + 1) * 4);
    L.partial = L.hist + align_256((size_t)L.slices * K * 4);
    L.total = L.partial + (size_t)L.max_chunks * BD_CLUSTER_DIM * 4;
    return L;
}

int check_workspace(const std::string& fn, const void* ws, int64_t bytes, const Layout& L) {
    const int rc = check_pointer(fn, "workspace_dev", ws, 16);
    if (rc != BD_OK) return rc;
    if (bytes < (int64_t)L.total)
        return fail(BD_EWORKSPACE, fn + "workspace_bytes = " + std::to_string(bytes) + ", needed are " + std::to_string(L.total));
    return BD_OK;
}

// what bd_cluster_order and its host restatement refuse alike (the pointers' alignment aside)
int check_order(const std::string& fn, const int32_t* labels, int64_t W, int32_t K, const int32_t* order, const int32_t* offsets) {
    int rc = check_clusters(fn, K);
    if (rc != BD_OK) return rc;
    if ((rc = check_rows(fn, W)) != BD_OK) return rc;
    if (W == 0) return BD_OK;
    if ((rc = check_pointer(fn, "labels", labels, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "order", order, 4)) != BD_OK) return rc;
    return check_pointer(fn, "offsets", offsets, 4);
}

int check_centroids(const std::string& fn, const float* e, int64_t W, const float* n2, const int32_t* order, const int32_t* offsets,
                    int32_t K, int32_t metric, const float* prev, const float* centroids, const float* packed, const float* c2) {
    int rc = check_clusters(fn, K);
    if (rc != BD_OK) return rc;
    if ((rc = check_rows(fn, W)) != BD_OK) return rc;
    if ((rc = check_metric(fn, metric)) != BD_OK) return rc;
    if (W == 0) return BD_OK;
    if ((rc = check_pointer(fn, "e", e, 16)) != BD_OK) return rc;
    if (metric == BD_CLUSTER_COSINE && (rc = check_pointer(fn, "n2", n2, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "order", order, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "offsets", offsets, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "prev", prev, 16)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "centroids", centroids, 16)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "packed", packed, 16)) != BD_OK) return rc;
    return check_pointer(fn, "c2", c2, 4);
}

int check_stats(const std::string& fn, const float* dist, const int32_t* labels, const int32_t* prev, int64_t W, const float* partial,
                const int32_t* changed) {
    int rc = check_rows(fn, W);
    if (rc != BD_OK) return rc;
    if (W == 0) return BD_OK;
    if ((rc = check_pointer(fn, "dist", dist, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "labels", labels, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "prev_labels", prev, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "partial", partial, 4)) != BD_OK) return rc;
    return check_pointer(fn, "changed", changed, 4);
}

float host_norm(const float* row) {
    float v[64];
    for (int lane = 0; lane < 64; ++lane) v[lane] = search::norm_chain(row, lane);
    return search::butterfly_host(v);
}

}  // namespace
}  // namespace bd

extern "C" {

int bd_cluster_abi_version(void) { return BD_CLUSTER_ABI_VERSION; }

int64_t bd_cluster_workspace_bytes(int64_t rows, int32_t n_clusters) {
    const std::string fn = "bd_cluster_workspace_bytes: ";
    int rc = bd::check_clusters(fn, n_clusters);
    if (rc != BD_OK) return rc;
    if ((rc = bd::check_rows(fn, rows)) != BD_OK) return rc;
    return (int64_t)bd::layout(rows, n_clusters).total;
}

int bd_cluster_assign(const float* e_dev, int64_t rows, const float* n2_dev, const float* packed_dev, const float* c2_dev,
                      int32_t n_clusters, int32_t metric, int32_t* labels_dev, float* dist_dev, void* stream) {
    const std::string fn = "bd_cluster_assign: ";
    int rc = bd::check_clusters(fn, n_clusters);
    if (rc != BD_OK) return rc;
    if ((rc = bd::check_rows(fn, rows)) != BD_OK) return rc;
    if ((rc = bd::check_metric(fn, metric)) != BD_OK) return rc;
    if (rows == 0) return BD_OK;
    if ((rc = bd::check_pointer(fn, "e_dev", e_dev, 16)) != BD_OK) return rc;
    if ((rc = bd::check_pointer(fn, "n2_dev", n2_dev, 4)) != BD_OK) return rc;
    if ((rc = bd::check_pointer(fn, "packed_dev", packed_dev, 16)) != BD_OK) return rc;
    if (metric == BD_CLUSTER_EUCLIDEAN && (rc = bd::check_pointer(fn, "c2_dev", c2_dev, 4)) != BD_OK) return rc;
    if ((rc = bd::check_pointer(fn, "labels_dev", labels_dev, 4)) != BD_OK) return rc;
    if ((rc = bd::check_pointer(fn, "dist_dev", dist_dev, 4)) != BD_OK) return rc;
    hipLaunchKernelGGL(bd::cluster_assign_kernel, dim3((unsigned)((rows + 127) / 128)), dim3(bd::kThreads), 0,
                       static_cast<hipStream_t>(stream), e_dev, (int)rows, n2_dev, reinterpret_cast<const float4*>(packed_dev),
                       c2_dev, (int)n_clusters, bd::cluster::kSuper, (int)metric, labels_dev, dist_dev);
    return bd::hip_result(fn);
}

int bd_cluster_order(const int32_t* labels_dev, int64_t rows, int32_t n_clusters, int32_t* order_dev, int32_t* offsets_dev,
                     void* workspace_dev, int64_t workspace_bytes, void* stream) {
    const std::string fn = "bd_cluster_order: ";
    int rc = bd::check_order(fn, labels_dev, rows, n_clusters, order_dev, offsets_dev);
    if (rc != BD_OK) return rc;
    if (rows == 0) return BD_OK;
    const bd::Layout L = bd::layout(rows, n_clusters);
    if ((rc = bd::check_workspace(fn, workspace_dev, workspace_bytes, L)) != BD_OK) return rc;
    int32_t* hist = reinterpret_cast<int32_t*>(static_cast<char*>(workspace_dev) + L.hist);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(bd::cluster_count_kernel, dim3((unsigned)L.slices), dim3(bd::kThreads), 0, s, labels_dev, (int)rows,
                       (int)n_clusters, hist);
    hipLaunchKernelGGL(bd::cluster_scan_kernel, dim3(1), dim3(bd::kScanThreads), 0, s, hist, L.slices, (int)n_clusters, offsets_dev);
    hipLaunchKernelGGL(bd::cluster_place_kernel, dim3((unsigned)L.slices), dim3(64), 0, s, labels_dev, (int)rows, (int)n_clusters,
                       hist, order_dev);
    return bd::hip_result(fn);
}

int bd_cluster_order_host(const int32_t* labels, int64_t rows, int32_t n_clusters, int32_t* order, int32_t* offsets) {
    const std::string fn = "bd_cluster_order_host: ";
    const int rc = bd::check_order(fn, labels, rows, n_clusters, order, offsets);
    if (rc != BD_OK) return rc;
    if (rows == 0) return BD_OK;
    for (int64_t r = 0; r < rows; ++r)
        if (labels[r] < 0 || labels[r] >= n_clusters)
            return bd::fail(BD_ERANGE, fn + "labels[" + std::to_string(r) + "] = " + std::to_string(labels[r]) + " is outside 0.." +
                                           std::to_string(n_clusters - 1));
    std::vector<int32_t> cursor((size_t)n_clusters + 1, 0);
    for (int64_t r = 0; r < rows; ++r) ++cursor[(size_t)labels[r] + 1];
    for (int32_t j = 0; j < n_clusters; ++j) cursor[(size_t)j + 1] += cursor[j];
    for (int32_t j = 0; j <= n_clusters; ++j) offsets[j] = cursor[j];
    for (int64_t r = 0; r < rows; ++r) order[cursor[labels[r]]++] = (int32_t)r;
    return BD_OK;
}

int bd_cluster_centroids(const float* e_dev, int64_t rows, const float* n2_dev, const int32_t* order_dev, const int32_t* offsets_dev,
                         int32_t n_clusters, int32_t metric, const float* prev_dev, float* centroids_dev, float* packed_dev,
                         float* c2_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    const std::string fn = "bd_cluster_centroids: ";
    int rc = bd::check_centroids(fn, e_dev, rows, n2_dev, order_dev, offsets_dev, n_clusters, metric, prev_dev, centroids_dev,
                                 packed_dev, c2_dev);
    if (rc != BD_OK) return rc;
    if (rows == 0) return BD_OK;
    const bd::Layout L = bd::layout(rows, n_clusters);
    if ((rc = bd::check_workspace(fn, workspace_dev, workspace_bytes, L)) != BD_OK) return rc;
    char* ws = static_cast<char*>(workspace_dev);
    int32_t* chunk_first = reinterpret_cast<int32_t*>(ws + L.chunk_first);
    float4* partial = reinterpret_cast<float4*>(ws + L.partial);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(bd::cluster_chunks_kernel, dim3(1), dim3(bd::kScanThreads), 0, s, offsets_dev, (int)rows, (int)n_clusters,
                       chunk_first);
    hipLaunchKernelGGL(bd::cluster_partial_kernel, dim3((unsigned)L.max_chunks), dim3(bd::kThreads), 0, s,
                       reinterpret_cast<const float4*>(e_dev), (int)rows, n2_dev, order_dev, offsets_dev, chunk_first,
                       (int)n_clusters, (int)metric, partial);
    hipLaunchKernelGGL(bd::cluster_finish_kernel, dim3((unsigned)((n_clusters + 31) / 32 * 32)), dim3(bd::kThreads), 0, s, partial,
                       L.max_chunks, offsets_dev, chunk_first, (int)rows, (int)n_clusters, (int)metric,
                       reinterpret_cast<const float4*>(prev_dev), reinterpret_cast<float4*>(centroids_dev),
                       reinterpret_cast<float4*>(packed_dev), c2_dev);
    return bd::hip_result(fn);
}

int bd_cluster_centroids_host(const float* e, int64_t rows, const float* n2, const int32_t* order, const int32_t* offsets,
                              int32_t n_clusters, int32_t metric, const float* prev, float* centroids, float* packed, float* c2) {
    namespace cl = bd::cluster;
    const std::string fn = "bd_cluster_centroids_host: ";
    const int rc = bd::check_centroids(fn, e, rows, n2, order, offsets, n_clusters, metric, prev, centroids, packed, c2);
    if (rc != BD_OK) return rc;
    if (rows == 0) return BD_OK;
    for (int32_t j = 0; j < n_clusters; ++j)
        if (offsets[j] < 0 || offsets[j] > offsets[j + 1] || offsets[j + 1] > rows)
            return bd::fail(BD_ERANGE, fn + "offsets[" + std::to_string(j) + "..] do not ascend within 0.." + std::to_string(rows));
    for (int64_t i = offsets[0]; i < offsets[n_clusters]; ++i)
        if (order[i] < 0 || order[i] >= rows)
            return bd::fail(BD_ERANGE, fn + "order[" + std::to_string(i) + "] = " + std::to_string(order[i]) + " is no row");
    const int tiles = (n_clusters + 31) / 32;
    std::vector<float> sum(BD_CLUSTER_DIM), part(BD_CLUSTER_DIM);
    for (int32_t j = 0; j < 32 * tiles; ++j) {
        if (j >= n_clusters) {
            for (int q = 0; q < BD_CLUSTER_DIM / 4; ++q)
                for (int u = 0; u < 4; ++u) packed[4 * cl::packed_quad(j, q) + u] = 0.0f;
            continue;
        }
        const int count = offsets[j + 1] - offsets[j];
        for (int c = 0; c < cl::chunks_of(count); ++c) {
            const int start = offsets[j] + c * BD_CLUSTER_CHUNK;
            const int n = std::min(BD_CLUSTER_CHUNK, offsets[j + 1] - start);
            std::fill(part.begin(), part.end(), 0.0f);
            for (int i = 0; i < n; ++i) {
                const int32_t r = order[start + i];
                const float ri = metric == BD_CLUSTER_COSINE ? cl::row_rinv(n2[r]) : 1.0f;
                const float* x = e + (size_t)r * BD_CLUSTER_DIM;
                for (int ch = 0; ch < BD_CLUSTER_DIM; ++ch) part[ch] = cl::chain_add(part[ch], cl::member_term(x[ch], ri, metric));
            }
            for (int ch = 0; ch < BD_CLUSTER_DIM; ++ch) sum[ch] = c == 0 ? part[ch] : cl::chain_add(sum[ch], part[ch]);
        }
        if (count == 0) std::fill(sum.begin(), sum.end(), 0.0f);
        const float m2 = metric == BD_CLUSTER_COSINE ? bd::host_norm(sum.data()) : 0.0f;
        float* out = centroids + (size_t)j * BD_CLUSTER_DIM;
        if (cl::keeps_previous(count, m2, metric)) {
            for (int ch = 0; ch < BD_CLUSTER_DIM; ++ch) out[ch] = prev[(size_t)j * BD_CLUSTER_DIM + ch];
        } else {
            const float d = cl::centroid_denominator(count, m2, metric);
            for (int ch = 0; ch < BD_CLUSTER_DIM; ++ch) out[ch] = cl::centroid_value(sum[ch], d);
        }
        for (int q = 0; q < BD_CLUSTER_DIM / 4; ++q)
            for (int u = 0; u < 4; ++u) packed[4 * cl::packed_quad(j, q) + u] = out[4 * q + u];
        c2[j] = bd::host_norm(out);
    }
    return BD_OK;
}

int bd_cluster_stats(const float* dist_dev, const int32_t* labels_dev, const int32_t* prev_labels_dev, int64_t rows,
                     float* partial_dev, int32_t* changed_dev, void* stream) {
    const std::string fn = "bd_cluster_stats: ";
    const int rc = bd::check_stats(fn, dist_dev, labels_dev, prev_labels_dev, rows, partial_dev, changed_dev);
    if (rc != BD_OK) return rc;
    if (rows == 0) return BD_OK;
    const int64_t slices = (rows + BD_CLUSTER_STAT_SLICE - 1) / BD_CLUSTER_STAT_SLICE;
    hipLaunchKernelGGL(bd::cluster_stats_kernel, dim3((unsigned)((slices + 3) / 4)), dim3(bd::kThreads), 0,
                       static_cast<hipStream_t>(stream), dist_dev, labels_dev, prev_labels_dev, (int)rows, partial_dev, changed_dev);
    return bd::hip_result(fn);
}

int bd_cluster_stats_host(const float* dist, const int32_t* labels, const int32_t* prev_labels, int64_t rows, float* partial,
                          int32_t* changed) {
    namespace cl = bd::cluster;
    const int rc = bd::check_stats("bd_cluster_stats_host: ", dist, labels, prev_labels, rows, partial, changed);
    if (rc != BD_OK) return rc;
    const int64_t slices = (rows + BD_CLUSTER_STAT_SLICE - 1) / BD_CLUSTER_STAT_SLICE;
    for (int64_t s = 0; s < slices; ++s) {
        float v[64];
        int n = 0;
        for (int lane = 0; lane < 64; ++lane) {
            v[lane] = cl::stat_chain(dist, s * BD_CLUSTER_STAT_SLICE, rows, lane);
            n += cl::stat_changed(labels, prev_labels, s * BD_CLUSTER_STAT_SLICE, rows, lane);
        }
        partial[s] = bd::search::butterfly_host(v);
        changed[s] = n;
    }
    return BD_OK;
}

}  // extern "C"
