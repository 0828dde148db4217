// k-nearest-neighbour lists for gfx950 (include/buzzdetect_knn.h): for every query row the k most similar candidate rows, over
// [W][1024] embeddings where they lie.
//
//   knn_roots_kernel    a thread per row: the root of its squared norm, 0 below the norm floor (cosine only).
//   knn_update_kernel   a workgroup owns 128 query rows and sweeps the candidates in panels of 128.  16 channels at a time both
//                       panels are staged in LDS from the row-major rows (a row's 16 channels lie 20 floats apart: the float4
//                       reads of 16 rows cover the 64 banks once), the next 16 already on their way into registers.  Each of the
//                       four waves keeps 64 x 64 sims in four accumulator tiles of v_mfma_f32_32x32x2_f32 and feeds them in the
//                       order of dense_tile_walk (dense_device.h), so a dot has the bits of bd_search_scores.  After the walk
//                       the panel is keyed in eight rounds of at most 16 candidates a row: a lane compares its key with the row's
//                       k-th best (LDS) and parks a survivor in the row's pending list (32 slots, an LDS counter).  After every
//                       round a wave merges the rows of its own whose list holds more than 16 - the state from global memory,
//                       lane i slot i, the pending keys beside it, one bitonic network over 128 keys in registers - and lowers
//                       the threshold; at the end every row is merged.  A row is merged by the same wave and a slot of the state
//                       is read and written by the same lane throughout.
//
// No floating-point number is added atomically, no workgroup waits for another, no [Wq][Wc] matrix exists anywhere, every
// output element has one writer, inputs are only read, and element offsets are 64-bit.
#include "bd_internal.h"
#include "bd_error.h"
#include "dense_device.h"
#include "knn_device.h"
#include "simsearch_device.h"

#include "../../include/buzzdetect_knn.h"

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kThreads = 256;
constexpr int kQuads = BD_KNN_DIM / 4;                   // float4 per row
constexpr int kBlock = 128;                              // query rows of a workgroup, candidate rows of a panel
constexpr int kChunk = 16;                               // channels staged at a time: two super-steps of the walk
constexpr int kChunks = BD_KNN_DIM / kChunk;
constexpr int kStride = kChunk + 4;                      // floats between staged rows
constexpr int kStage = kBlock * (kChunk / 4) / kThreads; // float4 of a panel's chunk a thread stages
constexpr int kPending = 32;                             // slots of a row's pending list
constexpr int kRound = 16;                               // candidates a row meets between two looks at its list
static_assert(kBlock == 4 * 32 && kThreads == 4 * 64, "2 x 2 waves of 2 x 2 tiles");
static_assert(kStage == 2 && kChunk == 16, "a thread stages rows t / 4 and t / 4 + 64, quad t % 4");
static_assert(2 * kRound <= kPending && BD_KNN_MAX_K + kPending <= 128, "a round fits behind a list left alone; the network sorts 128");
static_assert(BD_KNN_MAX_K <= 64, "lane i holds slot i of the state");

__global__ __launch_bounds__(kThreads) void knn_roots_kernel(const float* __restrict__ n2, int64_t W, float* __restrict__ roots) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r < W) roots[r] = knn::root(n2[r]);
}

// One bitonic network over the 128 keys of a wave, best (largest) first: position i < 64 is x0 of lane i, position 64 + i is x1.
__device__ __forceinline__ void sort_128(uint64_t& x0, uint64_t& x1, int lane) {
#pragma unroll
    for (int size = 2; size <= 128; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride == 64) {                           // positions lane and lane + 64: the last round, descending
                const uint64_t hi = x0 > x1 ? x0 : x1, lo = x0 > x1 ? x1 : x0;
                x0 = hi;
                x1 = lo;
            } else {
                const uint64_t o0 = __shfl_xor((unsigned long long)x0, stride, 64);
                const uint64_t o1 = __shfl_xor((unsigned long long)x1, stride, 64);
                const bool lower = (lane & stride) == 0;
                // a block of `size` positions is descending where (position & size) == 0; size == 128 is descending throughout
                const bool desc0 = (lane & size) == 0;
                const bool desc1 = ((lane + 64) & size) == 0;
                const bool max0 = lower == desc0, max1 = lower == desc1;
                x0 = max0 ? (x0 > o0 ? x0 : o0) : (x0 > o0 ? o0 : x0);
                x1 = max1 ? (x1 > o1 ? x1 : o1) : (x1 > o1 ? o1 : x1);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void knn_update_kernel(const float4* __restrict__ Q, int64_t Wq,
                                                               const float* __restrict__ roots_q, uint32_t q_base,
                                                               const float4* __restrict__ Cd, int64_t Wc,
                                                               const float* __restrict__ roots_c, uint32_t c_base, int metric,
                                                               int exclude_self, uint64_t* __restrict__ keys, int k) {
    __shared__ __attribute__((aligned(16))) float s_q[kBlock][kStride];
    __shared__ __attribute__((aligned(16))) float s_c[kBlock][kStride];
    __shared__ uint64_t s_pend[kBlock][kPending];
    __shared__ uint64_t s_kth[kBlock];                    // the row's k-th best key: 0 while the state has an empty slot
    __shared__ int s_count[kBlock];
    __shared__ float s_rq[kBlock], s_rc[kBlock];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int64_t q0 = (int64_t)blockIdx.x * kBlock;
    const int nq = (int)min((int64_t)kBlock, Wq - q0);    // >= 1: the grid has the blocks that hold rows

    if (tid < kBlock) {
        const bool real = tid < nq;
        s_kth[tid] = real ? keys[(size_t)(q0 + tid) * k + (k - 1)] : ~0ull;      // nothing beats a row that is not there
        s_count[tid] = 0;
        s_rq[tid] = real && metric == BD_KNN_COSINE ? roots_q[q0 + tid] : 1.0f;
    }

    // merges row (of the workgroup's 128) into its state; the whole wave calls it with the same row
    auto merge = [&](int row) {
        uint64_t* state = keys + (size_t)(q0 + row) * k;
        const int parked = min(s_count[row], kPending);
        uint64_t x0 = lane < k ? state[lane] : 0;
        uint64_t x1 = lane < parked ? s_pend[row][lane] : 0;
        sort_128(x0, x1, lane);
        if (lane < k) state[lane] = x0;
        if (lane == k - 1) s_kth[row] = x0;
        if (lane == 0) s_count[row] = 0;
    };

    // staging: thread (sr, sq) brings quad sq of rows sr and sr + 64 of both panels
    const int sq = tid & 3;
    const int sr = tid >> 2;
    const float4* qrow0 = Q + (size_t)(q0 + min(sr, nq - 1)) * kQuads + sq;                   // always in bounds
    const float4* qrow1 = Q + (size_t)(q0 + min(sr + 64, nq - 1)) * kQuads + sq;

    // a wave's 64 x 64 block: query rows 64 wr .., candidates 64 wc .. of the panel
    const int wr = wave & 1;
    const int wc = wave >> 1;
    const float* frag_q = &s_q[64 * wr + (lane & 31)][4 * half];
    const float* frag_c = &s_c[64 * wc + (lane & 31)][4 * half];

    // a lane keys one sim of its column and parks it if it beats the row's k-th best
    auto meet = [&](float dot, int row, uint32_t cid, float rc) {
        const bool self = exclude_self && cid == q_base + (uint32_t)(q0 + row);
        const uint64_t key = search::make_key(knn::similarity(dot, s_rq[row], rc, metric), cid);
        if (row < nq && !self && key > s_kth[row]) {
            const int slot = atomicAdd(&s_count[row], 1);              // (the order of the parked keys does not matter)
            if (slot < kPending) s_pend[row][slot] = key;              // (always: at most 16 waited, at most 16 come)
        }
    };
    // (accumulator r of a tile by a constant index: a loop over r leaves the tile in memory)
#define BD_KNN_MEET(i, j, r) meet(acc[i][j][r], 64 * wr + 32 * i + ((r) & 3) + 8 * ((r) >> 2) + 4 * half, cid, rc);
#define BD_KNN_MEET_TILE(i, j)                                                                                          \
    BD_KNN_MEET(i, j, 0) BD_KNN_MEET(i, j, 1) BD_KNN_MEET(i, j, 2) BD_KNN_MEET(i, j, 3) BD_KNN_MEET(i, j, 4) BD_KNN_MEET(i, j, 5)    \
    BD_KNN_MEET(i, j, 6) BD_KNN_MEET(i, j, 7) BD_KNN_MEET(i, j, 8) BD_KNN_MEET(i, j, 9) BD_KNN_MEET(i, j, 10) BD_KNN_MEET(i, j, 11) \
    BD_KNN_MEET(i, j, 12) BD_KNN_MEET(i, j, 13) BD_KNN_MEET(i, j, 14) BD_KNN_MEET(i, j, 15)
    // after a round: the wave's own rows 32 wave .. 32 wave + 31 whose list could not take another round
    auto drain = [&]() {
        const int waiting = lane < 32 ? s_count[32 * wave + lane] : 0;
        uint64_t full = __ballot(waiting > kRound);
        while (full) {
            const int b = __ffsll((unsigned long long)full) - 1;
            full &= full - 1;
            merge(32 * wave + b);
        }
    };
#define BD_KNN_ROUND(wcol, j, hh)                                                        \
        if (wc == wcol && ((lane & 31) >> 4) == hh) {                                    \
            const int col = 64 * wc + 32 * j + (lane & 31);                              \
            if (col < nc) {                                                              \
                const uint32_t cid = c_base + (uint32_t)(c0 + col);                      \
                const float rc = s_rc[col];                                              \
                BD_KNN_MEET_TILE(0, j)                                                   \
                BD_KNN_MEET_TILE(1, j)                                                   \
            }                                                                            \
        }                                                                                \
        __syncthreads();                                                                 \
        drain();                                                                         \
        __syncthreads();

#pragma unroll 1
    for (int64_t c0 = 0; c0 < Wc; c0 += kBlock) {
        const int nc = (int)min((int64_t)kBlock, Wc - c0);
        // (the last barrier of the panel before lies between the rounds' reads of s_rc and this)
        if (tid < kBlock) s_rc[tid] = tid < nc && metric == BD_KNN_COSINE ? roots_c[c0 + tid] : 1.0f;
        const float4* crow0 = Cd + (size_t)(c0 + min(sr, nc - 1)) * kQuads + sq;
        const float4* crow1 = Cd + (size_t)(c0 + min(sr + 64, nc - 1)) * kQuads + sq;

        dense_v16f acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

        float4 pq0 = qrow0[0], pq1 = qrow1[0], pc0 = crow0[0], pc1 = crow1[0];
#pragma unroll 1
        for (int ch = 0; ch < kChunks; ++ch) {
            *reinterpret_cast<float4*>(&s_q[sr][4 * sq]) = pq0;
            *reinterpret_cast<float4*>(&s_q[sr + 64][4 * sq]) = pq1;
            *reinterpret_cast<float4*>(&s_c[sr][4 * sq]) = pc0;
            *reinterpret_cast<float4*>(&s_c[sr + 64][4 * sq]) = pc1;
            __syncthreads();
            if (ch + 1 < kChunks) {                       // in flight under the matrix instructions below
                const int at = (ch + 1) * (kChunk / 4);
                pq0 = qrow0[at];
                pq1 = qrow1[at];
                pc0 = crow0[at];
                pc1 = crow1[at];
            }
#pragma unroll
            for (int ss = 0; ss < kChunk / 8; ++ss) {     // a super-step: channels 8 ss + 4 half .. + 3 of the chunk
                const float4 a0 = *reinterpret_cast<const float4*>(frag_q + 8 * ss);
                const float4 a1 = *reinterpret_cast<const float4*>(frag_q + 32 * kStride + 8 * ss);
                const float4 b0 = *reinterpret_cast<const float4*>(frag_c + 8 * ss);
                const float4 b1 = *reinterpret_cast<const float4*>(frag_c + 32 * kStride + 8 * ss);
#define BD_KNN_STEP(m)                                                                         \
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.m, b0.m, acc[0][0], 0, 0, 0); \
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.m, b1.m, acc[0][1], 0, 0, 0); \
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.m, b0.m, acc[1][0], 0, 0, 0); \
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.m, b1.m, acc[1][1], 0, 0, 0);
                BD_KNN_STEP(x)
                BD_KNN_STEP(y)
                BD_KNN_STEP(z)
                BD_KNN_STEP(w)
#undef BD_KNN_STEP
            }
            __syncthreads();
        }

        // the panel's candidates meet the lists: round (wave column, tile column, half of the tile's columns)
        BD_KNN_ROUND(0, 0, 0)
        BD_KNN_ROUND(0, 0, 1)
        BD_KNN_ROUND(0, 1, 0)
        BD_KNN_ROUND(0, 1, 1)
        BD_KNN_ROUND(1, 0, 0)
        BD_KNN_ROUND(1, 0, 1)
        BD_KNN_ROUND(1, 1, 0)
        BD_KNN_ROUND(1, 1, 1)
    }
#undef BD_KNN_ROUND
#undef BD_KNN_MEET_TILE
#undef BD_KNN_MEET
    // every row's state is written, whether anything waits for it or not
    for (int b = 0; b < 32; ++b)
        if (32 * wave + b < nq) merge(32 * wave + b);
}

// ---------------------------------------------------------------------------------------------------- host side
int check_pointer(const std::string& fn, const char* name, const void* p, int align) {
    if (!p) return fail(BD_EINVAL, fn + name + " is null");
    if ((uintptr_t)p % (uintptr_t)align) return fail(BD_EINVAL, fn + name + " is not " + std::to_string(align) + "-byte aligned");
    return BD_OK;
}

int check_rows(const std::string& fn, const char* name, int64_t W) {
    if (W < 0 || W > BD_KNN_MAX_ROWS)
        return fail(BD_EINVAL, fn + name + " = " + std::to_string(W) + ", a call takes 0.." + std::to_string(BD_KNN_MAX_ROWS));
    return BD_OK;
}

int check_base(const std::string& fn, const char* name, int64_t base, int64_t W) {
    if (base < 0) return fail(BD_EINVAL, fn + name + " = " + std::to_string(base) + " is negative");
    if (base + W > 0xFFFFFFFFll)
        return fail(BD_ERANGE, fn + name + " + rows = " + std::to_string(base + W) + " is past the last id, 4294967295");
    return BD_OK;
}

// what bd_knn_update and its host restatement refuse alike (row_align: 16 on the device, 4 on the host)
int check_update(const std::string& fn, const float* q, int64_t Wq, const float* n2_q, int64_t q_base, const float* c, int64_t Wc,
                 const float* n2_c, int64_t c_base, int32_t metric, int32_t exclude_self, const uint64_t* keys, int32_t k,
                 int row_align) {
    if (k < 1 || k > BD_KNN_MAX_K) return fail(BD_EINVAL, fn + "k = " + std::to_string(k) + ", allowed are 1.." + std::to_string(BD_KNN_MAX_K));
    int rc = check_rows(fn, "query_rows", Wq);
    if (rc != BD_OK) return rc;
    if ((rc = check_rows(fn, "candidate_rows", Wc)) != BD_OK) return rc;
    if ((rc = check_base(fn, "q_base_id", q_base, Wq)) != BD_OK) return rc;
    if ((rc = check_base(fn, "c_base_id", c_base, Wc)) != BD_OK) return rc;
    if (metric != BD_KNN_DOT && metric != BD_KNN_COSINE) return fail(BD_EINVAL, fn + "unknown metric " + std::to_string(metric));
    if (exclude_self != 0 && exclude_self != 1)
        return fail(BD_EINVAL, fn + "exclude_self = " + std::to_string(exclude_self) + ", allowed are 0 and 1");
    if (Wq == 0 || Wc == 0) return BD_OK;
    if ((rc = check_pointer(fn, "queries", q, row_align)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "candidates", c, row_align)) != BD_OK) return rc;
    if (metric == BD_KNN_COSINE) {
        if ((rc = check_pointer(fn, "n2_q", n2_q, 4)) != BD_OK) return rc;
        if ((rc = check_pointer(fn, "n2_c", n2_c, 4)) != BD_OK) return rc;
    }
    return check_pointer(fn, "keys", keys, 8);
}

size_t align_256(size_t n) { return (n + 255) / 256 * 256; }

// the workspace: [a root per query row][a root per candidate row]
int64_t workspace_bytes(int64_t Wq, int64_t Wc) { return (int64_t)(align_256((size_t)Wq * 4) + align_256((size_t)Wc * 4)); }

constexpr int kHostBlock = 16;                           // candidates whose chains run side by side on the host

// the chains of one query row against a block of candidates: qc = the row in chain order, ct [BD_KNN_DIM][kHostBlock] = the
// block in chain order, transposed.  Twice, as pca.hip's gram_tile_body: fmaf is correctly rounded either way.
__attribute__((always_inline)) inline void dots_body(const float* qc, const float* ct, float* acc) {
    for (int j = 0; j < kHostBlock; ++j) acc[j] = 0.0f;
    for (int t = 0; t < BD_KNN_DIM; ++t)
        for (int j = 0; j < kHostBlock; ++j) acc[j] = knn::dot_step(qc[t], ct[(size_t)t * kHostBlock + j], acc[j]);
}

void dots_plain(const float* qc, const float* ct, float* acc) { dots_body(qc, ct, acc); }

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2,fma"))) void dots_fma(const float* qc, const float* ct, float* acc) { dots_body(qc, ct, acc); }
bool have_fma() { return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma"); }
#else
void dots_fma(const float* qc, const float* ct, float* acc) { dots_body(qc, ct, acc); }
bool have_fma() { return false; }
#endif

}  // namespace
}  // namespace bd

extern "C" {

int bd_knn_abi_version(void) { return BD_KNN_ABI_VERSION; }

int64_t bd_knn_workspace_bytes(int64_t query_rows, int64_t candidate_rows) {
    const std::string fn = "bd_knn_workspace_bytes: ";
    int rc = bd::check_rows(fn, "query_rows", query_rows);
    if (rc != BD_OK) return rc;
    if ((rc = bd::check_rows(fn, "candidate_rows", candidate_rows)) != BD_OK) return rc;
    return bd::workspace_bytes(query_rows, candidate_rows);
}

int bd_knn_update(const float* queries_dev, int64_t query_rows, const float* n2_q_dev, int64_t q_base_id,
                  const float* candidates_dev, int64_t candidate_rows, const float* n2_c_dev, int64_t c_base_id, int32_t metric,
                  int32_t exclude_self, uint64_t* keys_dev, int32_t k, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    const std::string fn = "bd_knn_update: ";
    int rc = bd::check_update(fn, queries_dev, query_rows, n2_q_dev, q_base_id, candidates_dev, candidate_rows, n2_c_dev, c_base_id,
                              metric, exclude_self, keys_dev, k, 16);
    if (rc != BD_OK) return rc;
    if (query_rows == 0 || candidate_rows == 0) return BD_OK;
    if ((rc = bd::check_pointer(fn, "workspace", workspace_dev, 16)) != BD_OK) return rc;
    const int64_t need = bd::workspace_bytes(query_rows, candidate_rows);
    if (workspace_bytes < need)
        return bd::fail(BD_EWORKSPACE, fn + "workspace_bytes = " + std::to_string(workspace_bytes) + ", needed are " + std::to_string(need));
    float* roots_q = static_cast<float*>(workspace_dev);
    float* roots_c = reinterpret_cast<float*>(static_cast<char*>(workspace_dev) + bd::align_256((size_t)query_rows * 4));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (metric == BD_KNN_COSINE) {
        hipLaunchKernelGGL(bd::knn_roots_kernel, dim3((unsigned)((query_rows + bd::kThreads - 1) / bd::kThreads)), dim3(bd::kThreads),
                           0, s, n2_q_dev, query_rows, roots_q);
        hipLaunchKernelGGL(bd::knn_roots_kernel, dim3((unsigned)((candidate_rows + bd::kThreads - 1) / bd::kThreads)),
                           dim3(bd::kThreads), 0, s, n2_c_dev, candidate_rows, roots_c);
    }
    hipLaunchKernelGGL(bd::knn_update_kernel, dim3((unsigned)((query_rows + bd::kBlock - 1) / bd::kBlock)), dim3(bd::kThreads), 0, s,
                       reinterpret_cast<const float4*>(queries_dev), query_rows, roots_q, (uint32_t)q_base_id,
                       reinterpret_cast<const float4*>(candidates_dev), candidate_rows, roots_c, (uint32_t)c_base_id, (int)metric,
                       (int)exclude_self, keys_dev, (int)k);
    return bd::hip_result(fn);
}

int bd_knn_update_host(const float* queries, int64_t query_rows, const float* n2_q, int64_t q_base_id, const float* candidates,
                       int64_t candidate_rows, const float* n2_c, int64_t c_base_id, int32_t metric, int32_t exclude_self,
                       uint64_t* keys, int32_t k) {
    namespace kn = bd::knn;
    const std::string fn = "bd_knn_update_host: ";
    const int rc = bd::check_update(fn, queries, query_rows, n2_q, q_base_id, candidates, candidate_rows, n2_c, c_base_id, metric,
                                    exclude_self, keys, k, 4);
    if (rc != BD_OK) return rc;
    if (query_rows == 0 || candidate_rows == 0) return BD_OK;
    const bool fma = bd::have_fma();
    std::vector<float> qc((size_t)query_rows * BD_KNN_DIM);             // the query rows in chain order
    for (int64_t i = 0; i < query_rows; ++i)
        for (int t = 0; t < BD_KNN_DIM; ++t) qc[(size_t)i * BD_KNN_DIM + t] = queries[(size_t)i * BD_KNN_DIM + kn::chain_channel(t)];
    std::vector<std::vector<uint64_t>> all((size_t)query_rows);
    for (int64_t i = 0; i < query_rows; ++i)
        for (int s = 0; s < k; ++s)
            if (keys[(size_t)i * k + s]) all[(size_t)i].push_back(keys[(size_t)i * k + s]);
    auto prune = [&](std::vector<uint64_t>& v) {
        const size_t keep = std::min<size_t>((size_t)k, v.size());
        std::partial_sort(v.begin(), v.begin() + keep, v.end(), std::greater<uint64_t>());
        v.resize(keep);
    };
    std::vector<float> ct((size_t)BD_KNN_DIM * bd::kHostBlock);
    float acc[bd::kHostBlock];
    for (int64_t j0 = 0; j0 < candidate_rows; j0 += bd::kHostBlock) {
        const int n = (int)std::min<int64_t>(bd::kHostBlock, candidate_rows - j0);
        for (int t = 0; t < BD_KNN_DIM; ++t)
            for (int j = 0; j < bd::kHostBlock; ++j)
                ct[(size_t)t * bd::kHostBlock + j] = j < n ? candidates[(size_t)(j0 + j) * BD_KNN_DIM + kn::chain_channel(t)] : 0.0f;
        for (int64_t i = 0; i < query_rows; ++i) {
            if (fma) bd::dots_fma(qc.data() + (size_t)i * BD_KNN_DIM, ct.data(), acc);
            else bd::dots_plain(qc.data() + (size_t)i * BD_KNN_DIM, ct.data(), acc);
            const uint32_t qid = (uint32_t)(q_base_id + i);
            const float rq = metric == BD_KNN_COSINE ? kn::root(n2_q[i]) : 1.0f;
            std::vector<uint64_t>& mine = all[(size_t)i];
            for (int j = 0; j < n; ++j) {
                const uint32_t cid = (uint32_t)(c_base_id + j0 + j);
                if (exclude_self && cid == qid) continue;
                const float rcand = metric == BD_KNN_COSINE ? kn::root(n2_c[j0 + j]) : 1.0f;
                mine.push_back(bd::search::make_key(kn::similarity(acc[j], rq, rcand, metric), cid));
            }
            if (mine.size() >= (size_t)k + 1024) prune(mine);
        }
    }
    for (int64_t i = 0; i < query_rows; ++i) {
        prune(all[(size_t)i]);
        for (int s = 0; s < k; ++s) keys[(size_t)i * k + s] = (size_t)s < all[(size_t)i].size() ? all[(size_t)i][(size_t)s] : 0;
    }
    return BD_OK;
}

int64_t bd_knn_decode_host(const uint64_t* keys, int64_t n, int32_t* ids, float* sims) {
    const std::string fn = "bd_knn_decode_host: ";
    if (n < 0) return bd::fail(BD_EINVAL, fn + "n = " + std::to_string(n) + " is negative");
    if (n == 0) return 0;
    if (!keys || !ids || !sims) return bd::fail(BD_EINVAL, fn + (!keys ? "keys" : !ids ? "ids" : "sims") + " is null");
    for (int64_t i = 0; i < n; ++i)
        if (keys[i] && bd::search::key_id(keys[i]) > 0x7FFFFFFFu)
            return bd::fail(BD_ERANGE, fn + "keys[" + std::to_string(i) + "] holds id " + std::to_string(bd::search::key_id(keys[i])) +
                                           ", past 2147483647");
    int64_t real = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (keys[i]) {
            ids[i] = (int32_t)bd::search::key_id(keys[i]);
            sims[i] = bd::search::key_score(keys[i]);
            ++real;
        } else {
            ids[i] = -1;
            sims[i] = 0.0f;
        }
    }
    return real;
}

}  // extern "C"
