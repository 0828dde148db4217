// Search by example for gfx950 (include/buzzdetect_search.h): a score per (window, query) from the embeddings of a pass where
// they lie, and a running top-k per query, so that no [W][1024] row goes back to the host.
//
//   search_norms_kernel    a wave per row: 64 chains of 16 fused multiply-adds, one butterfly (simsearch_device.h).
//   search_scores_kernel   S = E Q^T on v_mfma_f32_32x32x2_f32 by dense_tile_walk (dense_device.h: the walk of the dense
//                          heads, headset.hip): a wave owns a 32 x 32 tile and walks K = 1024 alone, E straight from global memory,
//                          the queries from the fragment order bd_search_pack_queries wrote.  A workgroup is 2 x 2 waves.  The
//                          epilogue divides by the root of the row's squared norm (cosine) and stores by two element strides.
//   search_update_kernel   a workgroup per query.  LDS holds 2048 keys: the state in [0, k), survivors parked behind it.  The
//                          candidates are keyed in chunks of 1024; one that does not beat the state's k-th key is dropped, the
//                          others take the next free slot (an LDS counter: their order does not matter).  When the next chunk
//                          might not fit, and at the end, a bitonic network sorts the state and the parked keys (zero-padded to
//                          a power of two) best first, which leaves the k best in [0, k) and a new k-th key.  From an empty
//                          state the first sort comes after 1024 - 1948 candidates; from then on few candidates survive, and
//                          a call whose candidates all lose sorts nothing.  The order on keys is total and keys are distinct,
//                          so the outcome is the k largest of the set whatever the chunks and the slots were.
//
// Nothing is added atomically in global memory, no result depends on the grid, every output element has one writer, and inputs are only read:
// the launches are idempotent apart from the state, which bd_search_update advances by design.
#include "bd_internal.h"
#include "bd_error.h"
#include "dense_device.h"
#include "simsearch_device.h"

#include "../../include/buzzdetect_search.h"

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kSearchThreads = 256;
constexpr int kSearchSuper = BD_SEARCH_DIM / 8;          // super-steps of the K walk (a multiple of 4)
constexpr int kSortKeys = 2 * BD_SEARCH_MAX_K;           // 16 KB of LDS
constexpr int kSortPairs = kSortKeys / 2 / kSearchThreads;      // compare-exchanges per thread and step of the network, at most
constexpr int kSortChunk = 4 * kSearchThreads;           // candidates keyed between two looks at the room left in LDS
static_assert(kSearchSuper % 4 == 0, "dense_tile_walk takes whole groups of four super-steps");
static_assert((kSortKeys & (kSortKeys - 1)) == 0, "the network sorts a power of two");
static_assert(kSortPairs * 2 * kSearchThreads == kSortKeys, "a step's pairs are whole rounds of the workgroup");
static_assert(kSortChunk <= kSortKeys - BD_SEARCH_MAX_K, "a chunk fits behind the largest state");

__global__ __launch_bounds__(kSearchThreads) void search_norms_kernel(const float* __restrict__ E, int W, float* __restrict__ n2) {
    const int lane = threadIdx.x & 63;
    const int row = 4 * blockIdx.x + (threadIdx.x >> 6);
    if (row >= W) return;                                 // (no barrier in this kernel)
    const float v = search::butterfly_wave(search::norm_chain(E + (size_t)row * BD_SEARCH_DIM, lane));
    if (lane == 0) n2[row] = v;
}

__global__ __launch_bounds__(kSearchThreads) void search_scores_kernel(const float* __restrict__ E, int W,
                                                                        const float4* __restrict__ Qf, int Q, int metric,
                                                                        const float* __restrict__ n2, float* __restrict__ S,
                                                                        long long row_stride, long long col_stride) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tr = 2 * blockIdx.x + (wave & 1);           // 32-row tile of S
    const int tc = 2 * blockIdx.y + (wave >> 1);          // 32-query tile
    if (32 * tr >= W || 32 * tc >= Q) return;             // (no barrier in this kernel)
    const int half = lane >> 5;
    const int arow = min(32 * tr + (lane & 31), W - 1);   // always in bounds; rows past W are never stored
    const float* ap = E + (size_t)arow * BD_SEARCH_DIM + 4 * half;
    const float4* bp = Qf + (size_t)tc * kSearchSuper * 64 + lane;

    const dense_v16f acc = dense_tile_walk(ap, bp, BD_SEARCH_DIM, kSearchSuper, half);

    const int col = 32 * tc + (lane & 31);
    if (col >= Q) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = 32 * tr + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row >= W) continue;
        float v = acc[r];
        if (metric == BD_SEARCH_COSINE) {
            const float n = n2[row];
            v = n < BD_SEARCH_NORM_FLOOR ? 0.0f : __fdiv_rn(v, sqrtf(n));
        }
        S[(long long)row * row_stride + (long long)col * col_stride] = v;
    }
}

// Sorts buf[0, n) best (largest) first, n a power of two <= kSortKeys: a bitonic network, one barrier per step.  A thread's (up
// to) four pairs of a step are disjoint from everyone's: all loads first, so that the LDS latencies overlap, then the exchanges.
// Ends with a barrier.
__device__ __forceinline__ void sort_keys(uint64_t* buf, int n, int tid) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            uint64_t a[kSortPairs], b[kSortPairs];
            int at[kSortPairs];
#pragma unroll
            for (int u = 0; u < kSortPairs; ++u) {
                const int t = tid + u * kSearchThreads;
                const int i = 2 * t - (t & (stride - 1));
                at[u] = t < n / 2 ? i : -1;
                a[u] = b[u] = 0;
                if (at[u] >= 0) {
                    a[u] = buf[i];
                    b[u] = buf[i + stride];
                }
            }
#pragma unroll
            for (int u = 0; u < kSortPairs; ++u) {
                const int i = at[u];
                // the last round (size == n) is descending throughout
                if (i >= 0 && (a[u] < b[u]) == ((i & size) == 0)) {
                    buf[i] = b[u];
                    buf[i + stride] = a[u];
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kSearchThreads) void search_update_kernel(const float* __restrict__ S, int W, long long row_stride,
                                                                        long long col_stride, uint32_t base_id,
                                                                        uint64_t* __restrict__ keys, int k) {
    __shared__ uint64_t buf[kSortKeys];
    __shared__ int s_count;                               // survivors parked behind the state since the last sort
    const int tid = threadIdx.x;
    uint64_t* __restrict__ state = keys + (size_t)blockIdx.x * k;
    const float* __restrict__ col = S + (long long)blockIdx.x * col_stride;
    for (int i = tid; i < k; i += kSearchThreads) buf[i] = state[i];
    if (tid == 0) s_count = 0;
    __syncthreads();
    const int room = kSortKeys - k;                       // >= kSortChunk: a chunk always fits behind a freshly sorted state
    uint64_t kth = buf[k - 1];                            // 0 while the state has an empty slot: everything beats it
    for (int w0 = 0; w0 < W + kSortChunk; w0 += kSortChunk) {
        // (every thread reads the same count: the barrier below separates this read from the next chunk's additions)
        const int parked = s_count;
        const bool last = w0 >= W;
        __syncthreads();
        if (last ? parked > 0 : parked + kSortChunk > room) {
            int n = 2;
            while (n < k + parked) n <<= 1;               // <= kSortKeys: k + parked <= k + room
            for (int i = k + parked + tid; i < n; i += kSearchThreads) buf[i] = 0;
            if (tid == 0) s_count = 0;
            __syncthreads();
            sort_keys(buf, n, tid);                       // the k best of (state + parked) are in [0, k) again
            kth = buf[k - 1];
        }
        if (last) break;
#pragma unroll
        for (int u = 0; u < kSortChunk / kSearchThreads; ++u) {
            const int w = w0 + u * kSearchThreads + tid;
            if (w < W) {
                const uint64_t key = search::make_key(col[(long long)w * row_stride], base_id + (uint32_t)w);
                if (key > kth) buf[k + atomicAdd(&s_count, 1)] = key;     // (the order of the parked keys does not matter)
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < k; i += kSearchThreads) state[i] = buf[i];
}

int check_windows(const std::string& fn, int64_t W) {
    if (W < 0 || W > BD_SEARCH_MAX_WINDOWS)
        return fail(BD_EINVAL, fn + "windows = " + std::to_string(W) + ", a call takes 0.." + std::to_string(BD_SEARCH_MAX_WINDOWS));
    return BD_OK;
}

int check_queries(const std::string& fn, int32_t Q) {
    if (Q < 1 || Q > BD_SEARCH_MAX_QUERIES)
        return fail(BD_EINVAL, fn + "n_queries = " + std::to_string(Q) + ", allowed are 1.." + std::to_string(BD_SEARCH_MAX_QUERIES));
    return BD_OK;
}

// what bd_search_update and its host restatement refuse alike
int check_update(const std::string& fn, const float* scores, int64_t W, int32_t Q, int64_t row_stride, int64_t col_stride,
                 int64_t base_id, const uint64_t* keys, int32_t k) {
    int rc = check_queries(fn, Q);
    if (rc != BD_OK) return rc;
    if (k < 1 || k > BD_SEARCH_MAX_K) return fail(BD_EINVAL, fn + "k = " + std::to_string(k) + ", allowed are 1.." + std::to_string(BD_SEARCH_MAX_K));
    if ((rc = check_windows(fn, W)) != BD_OK) return rc;
    if (base_id < 0) return fail(BD_EINVAL, fn + "base_id = " + std::to_string(base_id) + " is negative");
    if (base_id + W > 0xFFFFFFFFll)
        return fail(BD_ERANGE, fn + "base_id + windows = " + std::to_string(base_id + W) + " is past the last id, 4294967295");
    if (row_stride == 0 || col_stride == 0) return fail(BD_EINVAL, fn + (row_stride == 0 ? "row_stride" : "col_stride") + " is 0");
    if (!keys) return fail(BD_EINVAL, fn + "keys is null");
    if (W > 0 && !scores) return fail(BD_EINVAL, fn + "scores is null");
    return BD_OK;
}

}  // namespace
}  // namespace bd

extern "C" {

int bd_search_abi_version(void) { return BD_SEARCH_ABI_VERSION; }

int64_t bd_search_packed_floats(int32_t n_queries) {
    const int rc = bd::check_queries("bd_search_packed_floats: ", n_queries);
    if (rc != BD_OK) return rc;
    return (int64_t)bd::dense_packed_floats(BD_SEARCH_DIM, n_queries);
}

int bd_search_pack_queries(const float* queries, int32_t n_queries, float* packed) {
    const std::string fn = "bd_search_pack_queries: ";
    const int rc = bd::check_queries(fn, n_queries);
    if (rc != BD_OK) return rc;
    if (!queries || !packed) return bd::fail(BD_EINVAL, fn + (queries ? "packed" : "queries") + " is null");
    std::vector<float> kernel((size_t)BD_SEARCH_DIM * n_queries);        // [K][N], as a Dense layer's kernel
    for (int q = 0; q < n_queries; ++q)
        for (int c = 0; c < BD_SEARCH_DIM; ++c) kernel[(size_t)c * n_queries + q] = queries[(size_t)q * BD_SEARCH_DIM + c];
    bd::dense_pack_weights(kernel.data(), BD_SEARCH_DIM, n_queries, packed);
    return BD_OK;
}

int bd_search_norms(const float* e_dev, int64_t windows, float* n2_dev, void* stream) {
    const std::string fn = "bd_search_norms: ";
    const int rc = bd::check_windows(fn, windows);
    if (rc != BD_OK) return rc;
    if (windows == 0) return BD_OK;
    if (!e_dev || !n2_dev) return bd::fail(BD_EINVAL, fn + (e_dev ? "n2_dev" : "e_dev") + " is null");
    if ((uintptr_t)e_dev % 4 || (uintptr_t)n2_dev % 4) return bd::fail(BD_EINVAL, fn + "misaligned buffer");
    hipLaunchKernelGGL(bd::search_norms_kernel, dim3((unsigned)((windows + 3) / 4)), dim3(bd::kSearchThreads), 0,
                       static_cast<hipStream_t>(stream), e_dev, (int)windows, n2_dev);
    return bd::hip_result(fn);
}

int bd_search_norms_host(const float* e, int64_t windows, float* n2) {
    const std::string fn = "bd_search_norms_host: ";
    const int rc = bd::check_windows(fn, windows);
    if (rc != BD_OK) return rc;
    if (windows == 0) return BD_OK;
    if (!e || !n2) return bd::fail(BD_EINVAL, fn + (e ? "n2" : "e") + " is null");
    for (int64_t w = 0; w < windows; ++w) {
        float v[64];
        for (int lane = 0; lane < 64; ++lane) v[lane] = bd::search::norm_chain(e + (size_t)w * BD_SEARCH_DIM, lane);
        n2[w] = bd::search::butterfly_host(v);
    }
    return BD_OK;
}

int bd_search_scores(const float* e_dev, int64_t windows, const float* packed_dev, int32_t n_queries, int32_t metric,
                     const float* n2_dev, float* scores_dev, int64_t row_stride, int64_t col_stride, void* stream) {
    const std::string fn = "bd_search_scores: ";
    int rc = bd::check_queries(fn, n_queries);
    if (rc != BD_OK) return rc;
    if ((rc = bd::check_windows(fn, windows)) != BD_OK) return rc;
    if (metric != BD_SEARCH_DOT && metric != BD_SEARCH_COSINE) return bd::fail(BD_EINVAL, fn + "unknown metric " + std::to_string(metric));
    if (row_stride == 0 || col_stride == 0) return bd::fail(BD_EINVAL, fn + (row_stride == 0 ? "row_stride" : "col_stride") + " is 0");
    if (!packed_dev || (uintptr_t)packed_dev % 16) return bd::fail(BD_EINVAL, fn + "packed_dev is null or not 16-byte aligned");
    if (windows == 0) return BD_OK;
    if (!e_dev || (uintptr_t)e_dev % 16) return bd::fail(BD_EINVAL, fn + "e_dev is null or not 16-byte aligned");
    if (!scores_dev || (uintptr_t)scores_dev % 4) return bd::fail(BD_EINVAL, fn + "scores_dev is null or misaligned");
    if (metric == BD_SEARCH_COSINE && (!n2_dev || (uintptr_t)n2_dev % 4))
        return bd::fail(BD_EINVAL, fn + "n2_dev is null or misaligned (BD_SEARCH_COSINE reads the rows' squared norms)");
    hipLaunchKernelGGL(bd::search_scores_kernel, dim3((unsigned)((windows + 63) / 64), (unsigned)((n_queries + 63) / 64)),
                       dim3(bd::kSearchThreads), 0, static_cast<hipStream_t>(stream), e_dev, (int)windows,
                       reinterpret_cast<const float4*>(packed_dev), (int)n_queries, (int)metric, n2_dev, scores_dev,
                       (long long)row_stride, (long long)col_stride);
    return bd::hip_result(fn);
}

int bd_search_update(const float* scores_dev, int64_t windows, int32_t n_queries, int64_t row_stride, int64_t col_stride,
                     int64_t base_id, uint64_t* keys_dev, int32_t k, void* stream) {
    const std::string fn = "bd_search_update: ";
    const int rc = bd::check_update(fn, scores_dev, windows, n_queries, row_stride, col_stride, base_id, keys_dev, k);
    if (rc != BD_OK) return rc;
    if ((uintptr_t)keys_dev % 8 || (uintptr_t)scores_dev % 4) return bd::fail(BD_EINVAL, fn + "misaligned buffer");
    if (windows == 0) return BD_OK;
    hipLaunchKernelGGL(bd::search_update_kernel, dim3((unsigned)n_queries), dim3(bd::kSearchThreads), 0,
                       static_cast<hipStream_t>(stream), scores_dev, (int)windows, (long long)row_stride, (long long)col_stride,
                       (uint32_t)base_id, keys_dev, (int)k);
    return bd::hip_result(fn);
}

int bd_search_update_host(const float* scores, int64_t windows, int32_t n_queries, int64_t row_stride, int64_t col_stride,
                          int64_t base_id, uint64_t* keys, int32_t k) {
    const int rc = bd::check_update("bd_search_update_host: ", scores, windows, n_queries, row_stride, col_stride, base_id, keys, k);
    if (rc != BD_OK) return rc;
    if (windows == 0) return BD_OK;
    std::vector<uint64_t> all;
    for (int32_t q = 0; q < n_queries; ++q) {
        uint64_t* state = keys + (size_t)q * k;
        all.clear();
        for (int i = 0; i < k; ++i)
            if (state[i]) all.push_back(state[i]);
        for (int64_t w = 0; w < windows; ++w)
            all.push_back(bd::search::make_key(scores[w * row_stride + q * col_stride], (uint32_t)(base_id + w)));
        const size_t keep = std::min<size_t>((size_t)k, all.size());
        std::partial_sort(all.begin(), all.begin() + keep, all.end(), std::greater<uint64_t>());
        for (size_t i = 0; i < (size_t)k; ++i) state[i] = i < keep ? all[i] : 0;
    }
    return BD_OK;
}

int64_t bd_search_decode_host(const uint64_t* keys, int64_t n, float* scores, uint32_t* ids) {
    if (n < 0 || (n > 0 && (!keys || !scores || !ids))) return bd::fail(BD_EINVAL, "bd_search_decode_host: null argument or n negative");
    int64_t real = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (keys[i]) {
            scores[i] = bd::search::key_score(keys[i]);
            ids[i] = bd::search::key_id(keys[i]);
            ++real;
        } else {
            scores[i] = -INFINITY;
            ids[i] = 0xFFFFFFFFu;
        }
    }
    return real;
}

}  // extern "C"
