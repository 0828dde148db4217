// Streaming PCA for gfx950 (include/buzzdetect_pca.h): column sums and the Gram matrix of [W][1024] embeddings where they lie,
// and the projection of rows on up to 64 components with its residual.
//
//   pca_sums_kernel      a workgroup per slice of 256 rows: 256 threads of four channels each add the slice's shifted rows in
//                        ascending order, read (through `pick`) at 4 KB a row.
//   pca_gram_kernel      a workgroup per (128 x 128 block of the upper triangle, slice of 1024 rows).  The slice's row ids go to
//                        LDS once (-1 for an absent row); then 32 rows at a time the block's two column panels are staged in LDS
//                        as t = E - shift, the next 32 rows already on their way into registers.  Each of the four waves keeps a
//                        64 x 64 block in four accumulator tiles of v_mfma_f32_32x32x2_f32: per pair of rows four LDS reads of
//                        one float feed four instructions.  A diagonal block stages one panel and idles its wave below the
//                        diagonal.  The accumulators go to the workspace in register order (coalesced), tiles with ti <= tj only.
//   pca_finish_kernel    a thread per element of the 528 tiles: the chain over the slices' partials, then gram[i][j] and its
//                        mirror image (a diagonal tile's elements mirror each other by themselves).
//   pca_project_kernel   a wave owns 32 rows: their centred squared norms (a butterfly per row), the one or two column tiles by
//                        dense_tile_walk (dense_device.h: the bits of bd_search_scores), y from the accumulators, u to LDS,
//                        and lane r of the wave runs row r's chain over the components for the residual.
//
// No floating-point number is added atomically, no result depends on the grid, every output element has one writer, inputs are
// only read, element offsets are 64-bit, and every row id read from memory is brought into range before it addresses anything.
#include "bd_internal.h"
#include "bd_error.h"
#include "dense_device.h"
#include "pca_device.h"
#include "simsearch_device.h"

#include "../../include/buzzdetect_pca.h"

#include <algorithm>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kThreads = 256;
constexpr int kQuads = BD_PCA_DIM / 4;                   // float4 per row
constexpr int kSuper = BD_PCA_DIM / 8;                   // super-steps of the projection's walk over a row
constexpr int kBlock = 128;                              // side of a workgroup's block of the Gram matrix
constexpr int kBlocksAcross = BD_PCA_DIM / kBlock;
constexpr int kBlocks = kBlocksAcross * (kBlocksAcross + 1) / 2;
constexpr int kChunkRows = 32;                           // rows of a slice staged at a time
static_assert(BD_PCA_SLICE % kChunkRows == 0 && kChunkRows % 2 == 0, "a slice is whole chunks, a chunk whole pairs of rows");
constexpr int kPanelStride = kBlock + 32;                // floats between staged rows: the odd row of a pair starts 32 banks on
constexpr int kStageRows = kChunkRows / (kThreads / (kBlock / 4));     // rows of a chunk a thread stages, per panel
static_assert(kQuads == kThreads, "a thread of the sums owns four channels of a row");
static_assert(kSuper % 4 == 0, "dense_tile_walk takes whole groups of four super-steps");
static_assert(kBlock == 4 * 32 && kThreads == 4 * 64, "2 x 2 waves of 2 x 2 tiles");
static_assert(kStageRows * (kThreads / 32) == kChunkRows && kBlock / 4 == 32, "32 threads stage a row of a panel");
static_assert(BD_PCA_SLICE % kThreads == 0 && BD_PCA_SUM_SLICE == kThreads, "the row ids are staged in whole rounds");
static_assert(BD_PCA_MAX_COMPONENTS == 64, "the projection keeps two column tiles of u in LDS");

// the id of the call's row r as the kernels stage it: the row of E, or -1 for a row past R and for an absent row
__device__ __forceinline__ int staged_row(int64_t r, int64_t R, const int32_t* __restrict__ pick, int64_t rows_total,
                                          const float* __restrict__ n2) {
    if (r >= R) return -1;
    const int64_t id = pca::clamp_row(pick ? (int64_t)pick[r] : r, rows_total);
    return pca::row_present(n2[id]) ? (int)id : -1;
}

__device__ __forceinline__ float4 term4(const float4 x, const float4 s) {
    return make_float4(pca::term(x.x, s.x), pca::term(x.y, s.y), pca::term(x.z, s.z), pca::term(x.w, s.w));
}

__global__ __launch_bounds__(kThreads) void pca_sums_kernel(const float4* __restrict__ E, int64_t rows_total,
                                                             const int32_t* __restrict__ pick, int64_t R,
                                                             const float* __restrict__ n2, const float4* __restrict__ shift,
                                                             float4* __restrict__ partial) {
    __shared__ int s_row[BD_PCA_SUM_SLICE];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * BD_PCA_SUM_SLICE;
    s_row[tid] = staged_row(first + tid, R, pick, rows_total, n2);
    __syncthreads();
    const int n = (int)min((int64_t)BD_PCA_SUM_SLICE, R - first);
    const float4 sh = shift ? shift[tid] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 8
    for (int i = 0; i < n; ++i) {
        const int id = s_row[i];
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (id >= 0) t = term4(E[(size_t)id * kQuads + tid], sh);
        acc.x = pca::chain_add(acc.x, t.x);
        acc.y = pca::chain_add(acc.y, t.y);
        acc.z = pca::chain_add(acc.z, t.z);
        acc.w = pca::chain_add(acc.w, t.w);
    }
    partial[(size_t)blockIdx.x * kQuads + tid] = acc;
}

__global__ __launch_bounds__(kThreads) void pca_gram_kernel(const float4* __restrict__ E, int64_t rows_total,
                                                             const int32_t* __restrict__ pick, int64_t R,
                                                             const float* __restrict__ n2, const float4* __restrict__ shift,
                                                             float* __restrict__ partial) {
    __shared__ int s_row[BD_PCA_SLICE];
    __shared__ __attribute__((aligned(16))) float s_panel[2][kChunkRows][kPanelStride];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    int bi = 0, rem = blockIdx.x;                         // block (bi, bj), bi <= bj, of the upper triangle
    while (rem >= kBlocksAcross - bi) {
        rem -= kBlocksAcross - bi;
        ++bi;
    }
    const int bj = bi + rem;
    const bool diag = bi == bj;
    const int64_t first = (int64_t)blockIdx.y * BD_PCA_SLICE;
#pragma unroll
    for (int u = 0; u < BD_PCA_SLICE / kThreads; ++u)
        s_row[u * kThreads + tid] = staged_row(first + u * kThreads + tid, R, pick, rows_total, n2);
    __syncthreads();
    const int n = (int)min((int64_t)BD_PCA_SLICE, R - first);            // >= 1: the grid has the slices that hold rows
    const int chunks = (n + kChunkRows - 1) / kChunkRows;

    // staging: thread (rg, cq) brings rows rg + 8 u of a chunk, channels 4 cq .. 4 cq + 3 of both panels
    const int cq = tid & 31;
    const int rg = tid >> 5;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 sh_a = shift ? shift[bi * (kBlock / 4) + cq] : zero4;
    const float4 sh_b = shift ? shift[bj * (kBlock / 4) + cq] : zero4;
    float4 pa[kStageRows], pb[kStageRows];
    auto fetch = [&](int c) {
#pragma unroll
        for (int u = 0; u < kStageRows; ++u) {
            const int id = s_row[c * kChunkRows + rg + 8 * u];
            pa[u] = pb[u] = zero4;
            if (id >= 0) {
                const float4* row = E + (size_t)id * kQuads;
                pa[u] = term4(row[bi * (kBlock / 4) + cq], sh_a);
                if (!diag) pb[u] = term4(row[bj * (kBlock / 4) + cq], sh_b);
            }
        }
    };

    // a wave's 64 x 64 block: rows (of the Gram matrix) 64 wr .. of the A panel, columns 64 wc .. of the B panel
    const int wr = wave & 1;
    const int wc = wave >> 1;
    const bool below = diag && wr > wc;                   // wholly below the diagonal: nothing of it is stored
    const float* pan_a = &s_panel[0][lane >> 5][64 * wr + (lane & 31)];
    const float* pan_b = &s_panel[diag ? 0 : 1][lane >> 5][64 * wc + (lane & 31)];
    dense_v16f acc00, acc01, acc10, acc11;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc00[r] = acc01[r] = acc10[r] = acc11[r] = 0.0f;

    fetch(0);
#pragma unroll 1
    for (int c = 0; c < chunks; ++c) {
#pragma unroll
        for (int u = 0; u < kStageRows; ++u) {
            *reinterpret_cast<float4*>(&s_panel[0][rg + 8 * u][4 * cq]) = pa[u];
            if (!diag) *reinterpret_cast<float4*>(&s_panel[1][rg + 8 * u][4 * cq]) = pb[u];
        }
        __syncthreads();
        if (c + 1 < chunks) fetch(c + 1);                 // in flight under the matrix instructions below
        if (!below) {
            const int pairs = min(kChunkRows, n - c * kChunkRows + 1) / 2;      // an odd tail takes its zero row along
            // the next pair's fragments come out of LDS under this pair's four instructions
            float a0 = pan_a[0], a1 = pan_a[32], b0 = pan_b[0], b1 = pan_b[32];
            for (int m = 0; m < pairs; ++m) {
                const int nx = 2 * min(m + 1, kChunkRows / 2 - 1) * kPanelStride;      // (stays inside the chunk)
                const float na0 = pan_a[nx], na1 = pan_a[nx + 32], nb0 = pan_b[nx], nb1 = pan_b[nx + 32];
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
                a0 = na0;
                a1 = na1;
                b0 = nb0;
                b1 = nb1;
            }
        }
        __syncthreads();
    }
    if (below) return;
    float* out = partial + (size_t)blockIdx.y * pca::kTiles * pca::kTileFloats + lane;
    const int ti = 4 * bi + 2 * wr, tj = 4 * bj + 2 * wc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        out[(size_t)pca::tile_index(ti, tj) * pca::kTileFloats + 64 * r] = acc00[r];
        out[(size_t)pca::tile_index(ti, tj + 1) * pca::kTileFloats + 64 * r] = acc01[r];
        if (ti + 1 <= tj) out[(size_t)pca::tile_index(ti + 1, tj) * pca::kTileFloats + 64 * r] = acc10[r];
        out[(size_t)pca::tile_index(ti + 1, tj + 1) * pca::kTileFloats + 64 * r] = acc11[r];
    }
}

__global__ __launch_bounds__(kThreads) void pca_finish_kernel(const float* __restrict__ partial, int slices, int accumulate,
                                                               float* __restrict__ gram) {
    const int tile = blockIdx.x;                          // (uniform over the workgroup)
    int ti = 0, rem = tile;
    while (rem >= pca::kTilesAcross - ti) {
        rem -= pca::kTilesAcross - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int e = blockIdx.y * kThreads + threadIdx.x;    // accumulator register e / 64 of lane e % 64
    const float* p = partial + (size_t)tile * pca::kTileFloats + e;
    const size_t step = (size_t)pca::kTiles * pca::kTileFloats;
    float sum = p[0];
    for (int s = 1; s < slices; ++s) sum = pca::chain_add(sum, p[(size_t)s * step]);
    const int i = 32 * ti + pca::acc_row(e >> 6, e & 63);
    const int j = 32 * tj + (e & 31);
    if (accumulate) sum = pca::chain_add(gram[(size_t)i * BD_PCA_DIM + j], sum);
    gram[(size_t)i * BD_PCA_DIM + j] = sum;
    if (ti != tj) gram[(size_t)j * BD_PCA_DIM + i] = sum;
}

__global__ __launch_bounds__(kThreads) void pca_project_kernel(const float* __restrict__ E, int W, const float4* __restrict__ Vf,
                                                                int d, int n_super, const float* __restrict__ mv,
                                                                const float* __restrict__ scale, const float* __restrict__ mean,
                                                                float* __restrict__ y, float* __restrict__ resid) {
    __shared__ float s_u[kThreads / 64][32][BD_PCA_MAX_COMPONENTS + 1];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int tr = 4 * blockIdx.x + wave;                 // the wave's 32 rows
    const bool live = 32 * (int64_t)tr < W;               // (uniform over the wave; every wave meets the barrier below)
    const int half = lane >> 5;
    float c2 = 0.0f;                                      // lanes r and r + 32: the centred squared norm of the wave's row r
    if (live) {
#pragma unroll 1
        for (int rr = 0; rr < 32; ++rr) {
            const int row = min(32 * tr + rr, W - 1);     // always in bounds; rows past W are never stored
            const float v = search::butterfly_wave(pca::centred_norm_chain(E + (size_t)row * BD_PCA_DIM, mean, lane));
            if ((lane & 31) == rr) c2 = v;
        }
        const int arow = min(32 * tr + (lane & 31), W - 1);
        const float* ap = E + (size_t)arow * BD_PCA_DIM + 4 * half;
        const int tiles = (d + 31) / 32;
#pragma unroll 1
        for (int tc = 0; tc < tiles; ++tc) {
            const float4* bp = Vf + (size_t)tc * n_super * 64 + lane;
            // (n_super is an argument, as in cluster.hip: known at compile time, the walk unrolls whole and spills)
            const dense_v16f acc = dense_tile_walk(ap, bp, BD_PCA_DIM, n_super, half);
            const int col = 32 * tc + (lane & 31);
            const bool mine = col < d;
            const float m = mine ? mv[col] : 0.0f;
            const float sc = mine ? scale[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = pca::acc_row(r, lane);     // the row within the wave's 32
                const float c2r = __shfl(c2, lr, 64);     // (every lane takes part)
                const float u = pca::centred_score(acc[r], m);
                const int row = 32 * tr + lr;
                if (mine) {
                    s_u[wave][lr][col] = u;
                    if (row < W) y[(size_t)row * d + col] = pca::row_present(c2r) ? pca::coordinate(u, sc) : pca::quiet_nan();
                }
            }
        }
    }
    __syncthreads();
    const int row = 32 * tr + lane;
    if (live && resid && lane < 32 && row < W) {
        float q = 0.0f;
        for (int j = 0; j < d; ++j) q = pca::energy_step(q, s_u[wave][lane][j]);
        resid[row] = pca::row_present(c2) ? pca::residual(c2, q) : pca::quiet_nan();
    }
}

// ---------------------------------------------------------------------------------------------------- host side
int check_pointer(const std::string& fn, const char* name, const void* p, int align) {
    if (!p) return fail(BD_EINVAL, fn + name + " is null");
    if ((uintptr_t)p % (uintptr_t)align) return fail(BD_EINVAL, fn + name + " is not " + std::to_string(align) + "-byte aligned");
    return BD_OK;
}

// what sums and gram, device and host, refuse alike about their rows; BD_OK with R == 0 means: nothing to do
int check_rows(const std::string& fn, const float* e, int64_t rows_total, const int32_t* pick, int64_t R, const float* n2,
               const float* shift) {
    if (R < 0 || R > BD_PCA_MAX_ROWS) return fail(BD_EINVAL, fn + "R = " + std::to_string(R) + ", a call takes 0.." + std::to_string(BD_PCA_MAX_ROWS));
    if (R == 0) return BD_OK;
    if (rows_total < 1 || rows_total > 0x7FFFFFFFll)
        return fail(BD_EINVAL, fn + "rows_total = " + std::to_string(rows_total) + ", allowed are 1..2147483647");
    int rc = check_pointer(fn, "e", e, 16);
    if (rc != BD_OK) return rc;
    if (pick) {
        if ((rc = check_pointer(fn, "pick", pick, 4)) != BD_OK) return rc;
    } else if (R > rows_total) {
        return fail(BD_EINVAL, fn + "R = " + std::to_string(R) + " rows of rows_total = " + std::to_string(rows_total) + " without a pick");
    }
    if ((rc = check_pointer(fn, "n2", n2, 4)) != BD_OK) return rc;
    if (shift && (rc = check_pointer(fn, "shift", shift, 16)) != BD_OK) return rc;
    return BD_OK;
}

int check_pick(const std::string& fn, const int32_t* pick, int64_t R, int64_t rows_total) {
    if (!pick) return BD_OK;
    for (int64_t r = 0; r < R; ++r)
        if (pick[r] < 0 || pick[r] >= rows_total)
            return fail(BD_ERANGE, fn + "pick[" + std::to_string(r) + "] = " + std::to_string(pick[r]) + " is outside 0.." +
                                       std::to_string(rows_total - 1));
    return BD_OK;
}

int check_accumulate(const std::string& fn, int32_t accumulate) {
    if (accumulate != 0 && accumulate != 1) return fail(BD_EINVAL, fn + "accumulate = " + std::to_string(accumulate) + ", allowed are 0 and 1");
    return BD_OK;
}

int check_project(const std::string& fn, const float* e, int64_t W, const float* weights, const char* weights_name,
                  int weights_align, int32_t d, const float* mv, const float* scale, const float* mean, const float* y,
                  const float* resid) {
    if (d < 1 || d > BD_PCA_MAX_COMPONENTS)
        return fail(BD_EINVAL, fn + "d = " + std::to_string(d) + ", allowed are 1.." + std::to_string(BD_PCA_MAX_COMPONENTS));
    if (W < 0 || W > BD_SEARCH_MAX_WINDOWS)
        return fail(BD_EINVAL, fn + "W = " + std::to_string(W) + ", a call takes 0.." + std::to_string(BD_SEARCH_MAX_WINDOWS));
    if (W == 0) return BD_OK;
    int rc = check_pointer(fn, "e", e, 16);
    if (rc != BD_OK) return rc;
    if ((rc = check_pointer(fn, weights_name, weights, weights_align)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "mv", mv, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "scale", scale, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "mean", mean, 16)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "y", y, 4)) != BD_OK) return rc;
    if (resid && (rc = check_pointer(fn, "resid", resid, 4)) != BD_OK) return rc;
    return BD_OK;
}

int64_t slices_of(int64_t R) { return (R + BD_PCA_SLICE - 1) / BD_PCA_SLICE; }

int64_t workspace_bytes(int64_t R) { return slices_of(R) * pca::kTiles * pca::kTileFloats * (int64_t)sizeof(float); }

// the host's id of the call's row r, or -1 for an absent row (pick has been checked)
int64_t host_row(int64_t r, const int32_t* pick, const float* n2) {
    const int64_t id = pick ? (int64_t)pick[r] : r;
    return pca::row_present(n2[id]) ? id : -1;
}

// one tile's chains over n staged rows t [n][BD_PCA_DIM]: acc [32][32] from zero.  Twice: as the compiler makes it for any
// x86-64, where every step is a call of fmaf, and for processors with fused multiply-add instructions, where it is one
// instruction for eight elements; fmaf is correctly rounded either way, so the bits are the same.
__attribute__((always_inline)) inline void gram_tile_body(const float* t, int64_t n, int ci, int cj, float* acc) {
    for (int e = 0; e < pca::kTileFloats; ++e) acc[e] = 0.0f;
    for (int64_t r = 0; r < n; ++r) {
        const float* a = t + (size_t)r * BD_PCA_DIM + ci;
        const float* b = t + (size_t)r * BD_PCA_DIM + cj;
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) acc[32 * i + j] = pca::gram_step(a[i], b[j], acc[32 * i + j]);
    }
}

void gram_tile_plain(const float* t, int64_t n, int ci, int cj, float* acc) { gram_tile_body(t, n, ci, cj, acc); }

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2,fma"))) void gram_tile_fma(const float* t, int64_t n, int ci, int cj, float* acc) {
    gram_tile_body(t, n, ci, cj, acc);
}
bool have_fma() { return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma"); }
#else
void gram_tile_fma(const float* t, int64_t n, int ci, int cj, float* acc) { gram_tile_body(t, n, ci, cj, acc); }
bool have_fma() { return false; }
#endif

float host_centred_norm(const float* row, const float* mean) {
    float v[64];
    for (int lane = 0; lane < 64; ++lane) v[lane] = pca::centred_norm_chain(row, mean, lane);
    return search::butterfly_host(v);
}

}  // namespace
}  // namespace bd

extern "C" {

int bd_pca_abi_version(void) { return BD_PCA_ABI_VERSION; }

int bd_pca_sums(const float* e_dev, int64_t rows_total, const int32_t* pick_dev, int64_t R, const float* n2_dev,
                const float* shift_dev, float* partial_dev, void* stream) {
    const std::string fn = "bd_pca_sums: ";
    int rc = bd::check_rows(fn, e_dev, rows_total, pick_dev, R, n2_dev, shift_dev);
    if (rc != BD_OK) return rc;
    if (R == 0) return BD_OK;
    if ((rc = bd::check_pointer(fn, "partial", partial_dev, 16)) != BD_OK) return rc;
    const int64_t slices = (R + BD_PCA_SUM_SLICE - 1) / BD_PCA_SUM_SLICE;
    hipLaunchKernelGGL(bd::pca_sums_kernel, dim3((unsigned)slices), dim3(bd::kThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4*>(e_dev), rows_total, pick_dev, R, n2_dev,
                       reinterpret_cast<const float4*>(shift_dev), reinterpret_cast<float4*>(partial_dev));
    return bd::hip_result(fn);
}

int bd_pca_sums_host(const float* e, int64_t rows_total, const int32_t* pick, int64_t R, const float* n2, const float* shift,
                     float* partial) {
    namespace pc = bd::pca;
    const std::string fn = "bd_pca_sums_host: ";
    int rc = bd::check_rows(fn, e, rows_total, pick, R, n2, shift);
    if (rc != BD_OK) return rc;
    if (R == 0) return BD_OK;
    if ((rc = bd::check_pointer(fn, "partial", partial, 4)) != BD_OK) return rc;
    if ((rc = bd::check_pick(fn, pick, R, rows_total)) != BD_OK) return rc;
    for (int64_t first = 0; first < R; first += BD_PCA_SUM_SLICE) {
        float* out = partial + (size_t)(first / BD_PCA_SUM_SLICE) * BD_PCA_DIM;
        for (int c = 0; c < BD_PCA_DIM; ++c) out[c] = 0.0f;
        for (int64_t r = first; r < std::min<int64_t>(first + BD_PCA_SUM_SLICE, R); ++r) {
            const int64_t id = bd::host_row(r, pick, n2);
            for (int c = 0; c < BD_PCA_DIM; ++c) {
                const float t = id < 0 ? 0.0f : pc::term(e[(size_t)id * BD_PCA_DIM + c], shift ? shift[c] : 0.0f);
                out[c] = pc::chain_add(out[c], t);
            }
        }
    }
    return BD_OK;
}

int64_t bd_pca_workspace_bytes(int64_t R) {
    if (R < 0 || R > BD_PCA_MAX_ROWS)
        return bd::fail(BD_EINVAL, "bd_pca_workspace_bytes: R = " + std::to_string(R) + ", a call takes 0.." + std::to_string(BD_PCA_MAX_ROWS));
    return bd::workspace_bytes(R);
}

int bd_pca_gram(const float* e_dev, int64_t rows_total, const int32_t* pick_dev, int64_t R, const float* n2_dev,
                const float* shift_dev, int32_t accumulate, float* gram_dev, void* workspace_dev, int64_t workspace_bytes,
                void* stream) {
    const std::string fn = "bd_pca_gram: ";
    int rc = bd::check_accumulate(fn, accumulate);
    if (rc != BD_OK) return rc;
    if ((rc = bd::check_rows(fn, e_dev, rows_total, pick_dev, R, n2_dev, shift_dev)) != BD_OK) return rc;
    if (R == 0) return BD_OK;
    if ((rc = bd::check_pointer(fn, "gram", gram_dev, 16)) != BD_OK) return rc;
    if ((rc = bd::check_pointer(fn, "workspace", workspace_dev, 16)) != BD_OK) return rc;
    if (workspace_bytes < bd::workspace_bytes(R))
        return bd::fail(BD_EWORKSPACE, fn + "workspace_bytes = " + std::to_string(workspace_bytes) + ", needed are " +
                                           std::to_string(bd::workspace_bytes(R)));
    const int slices = (int)bd::slices_of(R);
    float* partial = static_cast<float*>(workspace_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(bd::pca_gram_kernel, dim3((unsigned)bd::kBlocks, (unsigned)slices), dim3(bd::kThreads), 0, s,
                       reinterpret_cast<const float4*>(e_dev), rows_total, pick_dev, R, n2_dev,
                       reinterpret_cast<const float4*>(shift_dev), partial);
    hipLaunchKernelGGL(bd::pca_finish_kernel, dim3((unsigned)bd::pca::kTiles, (unsigned)(bd::pca::kTileFloats / bd::kThreads)),
                       dim3(bd::kThreads), 0, s, partial, slices, (int)accumulate, gram_dev);
    return bd::hip_result(fn);
}

int bd_pca_gram_host(const float* e, int64_t rows_total, const int32_t* pick, int64_t R, const float* n2, const float* shift,
                     int32_t accumulate, float* gram) {
    namespace pc = bd::pca;
    const std::string fn = "bd_pca_gram_host: ";
    int rc = bd::check_accumulate(fn, accumulate);
    if (rc != BD_OK) return rc;
    if ((rc = bd::check_rows(fn, e, rows_total, pick, R, n2, shift)) != BD_OK) return rc;
    if (R == 0) return BD_OK;
    if ((rc = bd::check_pointer(fn, "gram", gram, 4)) != BD_OK) return rc;
    if ((rc = bd::check_pick(fn, pick, R, rows_total)) != BD_OK) return rc;
    const bool fma = bd::have_fma();
    std::vector<float> t((size_t)BD_PCA_SLICE * BD_PCA_DIM);
    std::vector<float> total((size_t)pc::kTiles * pc::kTileFloats);
    float acc[pc::kTileFloats];
    for (int64_t first = 0; first < R; first += BD_PCA_SLICE) {
        const int64_t n = std::min<int64_t>(BD_PCA_SLICE, R - first);
        const int64_t padded = n + (n & 1);               // an odd count takes one row of zeros along
        for (int64_t r = 0; r < padded; ++r) {
            const int64_t id = r < n ? bd::host_row(first + r, pick, n2) : -1;
            float* row = t.data() + (size_t)r * BD_PCA_DIM;
            for (int c = 0; c < BD_PCA_DIM; ++c)
                row[c] = id < 0 ? 0.0f : pc::term(e[(size_t)id * BD_PCA_DIM + c], shift ? shift[c] : 0.0f);
        }
        for (int ti = 0; ti < pc::kTilesAcross; ++ti)
            for (int tj = ti; tj < pc::kTilesAcross; ++tj) {
                if (fma) bd::gram_tile_fma(t.data(), padded, 32 * ti, 32 * tj, acc);
                else bd::gram_tile_plain(t.data(), padded, 32 * ti, 32 * tj, acc);
                float* sum = total.data() + (size_t)pc::tile_index(ti, tj) * pc::kTileFloats;
                for (int x = 0; x < pc::kTileFloats; ++x) sum[x] = first == 0 ? acc[x] : pc::chain_add(sum[x], acc[x]);
            }
    }
    for (int ti = 0; ti < pc::kTilesAcross; ++ti)
        for (int tj = ti; tj < pc::kTilesAcross; ++tj) {
            const float* sum = total.data() + (size_t)pc::tile_index(ti, tj) * pc::kTileFloats;
            for (int i = 0; i < 32; ++i)
                for (int j = 0; j < 32; ++j) {
                    float* up = gram + (size_t)(32 * ti + i) * BD_PCA_DIM + 32 * tj + j;
                    const float v = accumulate ? pc::chain_add(*up, sum[32 * i + j]) : sum[32 * i + j];
                    *up = v;
                    if (ti != tj) gram[(size_t)(32 * tj + j) * BD_PCA_DIM + 32 * ti + i] = v;
                }
        }
    return BD_OK;
}

int bd_pca_project(const float* e_dev, int64_t W, const float* packed_dev, int32_t d, const float* mv_dev, const float* scale_dev,
                   const float* mean_dev, float* y_dev, float* resid_dev, void* stream) {
    const std::string fn = "bd_pca_project: ";
    const int rc = bd::check_project(fn, e_dev, W, packed_dev, "packed", 16, d, mv_dev, scale_dev, mean_dev, y_dev, resid_dev);
    if (rc != BD_OK) return rc;
    if (W == 0) return BD_OK;
    hipLaunchKernelGGL(bd::pca_project_kernel, dim3((unsigned)((W + 127) / 128)), dim3(bd::kThreads), 0,
                       static_cast<hipStream_t>(stream), e_dev, (int)W, reinterpret_cast<const float4*>(packed_dev), (int)d,
                       bd::kSuper, mv_dev, scale_dev, mean_dev, y_dev, resid_dev);
    return bd::hip_result(fn);
}

int bd_pca_project_host(const float* e, int64_t W, const float* scores, int32_t d, const float* mv, const float* scale,
                        const float* mean, float* y, float* resid) {
    namespace pc = bd::pca;
    const std::string fn = "bd_pca_project_host: ";
    const int rc = bd::check_project(fn, e, W, scores, "scores", 4, d, mv, scale, mean, y, resid);
    if (rc != BD_OK) return rc;
    for (int64_t w = 0; w < W; ++w) {
        const float c2 = bd::host_centred_norm(e + (size_t)w * BD_PCA_DIM, mean);
        const bool present = pc::row_present(c2);
        float q = 0.0f;
        for (int j = 0; j < d; ++j) {
            const float u = pc::centred_score(scores[(size_t)w * d + j], mv[j]);
            y[(size_t)w * d + j] = present ? pc::coordinate(u, scale[j]) : pc::quiet_nan();
            q = pc::energy_step(q, u);
        }
        if (resid) resid[w] = present ? pc::residual(c2, q) : pc::quiet_nan();
    }
    return BD_OK;
}

}  // extern "C"
