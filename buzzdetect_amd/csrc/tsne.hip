// The neighbour-preserving 2-D map for gfx950 (include/buzzdetect_tsne.h): exact t-SNE from the neighbour lists.
//
//   tsne_affinities_kernel   a wave per row, a lane per slot: the bisection on beta with butterflies for the sums.
//   tsne_attract_kernel      a wave per row: lane l over edges l, l + 64, .. in stored order, one butterfly per coordinate.
//   tsne_repulse_kernel      the hot path, pure vector f32: a one-wave workgroup owns BD_TSNE_ROWS_PER_BLOCK rows, four per lane
//                            in registers, and one slice of BD_TSNE_SLICE candidates staged in LDS (16 KB); every LDS read is a
//                            broadcast that serves four pairs, and the four rows' chains are the instruction-level parallelism.
//                            The grid is (row blocks x slices); a (row, slice) partial has one writer.
//   tsne_finish_kernel       a thread per row: the slices' partials in ascending order.
//   tsne_slice_sums_kernel   a wave per (slice, column); tsne_totals_kernel one lane per column over the slices' sums.
//   tsne_update_kernel       a thread per row: gradient, gains, velocity, position; tsne_centre_kernel subtracts the mean.
//   tsne_kl_kernel           a wave per row over its edges.
//
// No floating-point number is added atomically, no result depends on the grid, every output element has one writer, no
// workgroup waits for another, inputs are only read, element offsets are 64-bit, and every index read from memory (a
// neighbour, a row's edge range) is brought into range before it addresses anything.
#include "bd_internal.h"
#include "bd_error.h"
#include "tsne_device.h"

#include "../../include/buzzdetect_tsne.h"

#include <algorithm>
#include <string>
#include <vector>

#pragma clang fp contract(off)

namespace bd {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerLane = BD_TSNE_ROWS_PER_BLOCK / 64;

// the workspace, in floats: [slices][3][rows] partials of the repulsion, then what WsLayout names
struct WsLayout {
    int64_t slices, part, zpart, tot, mpart, rowkl, klpart, floats;
};

WsLayout ws_layout(int64_t rows) {
    WsLayout w;
    w.slices = tsne::slices_of(rows);
    w.part = 0;
    w.zpart = w.part + 3 * w.slices * rows;
    w.tot = w.zpart + w.slices;                 // Z, sum of y[.][0], sum of y[.][1], the divergence
    w.mpart = w.tot + 4;
    w.rowkl = w.mpart + 2 * w.slices;
    w.klpart = w.rowkl + rows;
    w.floats = w.klpart + w.slices;
    return w;
}

int64_t ws_bytes(int64_t rows) { return (ws_layout(rows).floats * 4 + 255) / 256 * 256; }

__global__ __launch_bounds__(kThreads) void tsne_affinities_kernel(const int32_t* __restrict__ ids, const float* __restrict__ sims,
                                                                    int64_t N, int k, float perplexity, float* __restrict__ p,
                                                                    float* __restrict__ beta) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= N) return;                                   // (uniform over the wave; no barrier in this kernel)
    const bool slot = lane < k;
    const size_t at = (size_t)i * k + (slot ? lane : 0);
    const bool ok = slot && tsne::usable(ids[at], sims[at]);
    float d = ok ? tsne::distance(sims[at]) : INFINITY;
    float dmin = d;
    int m = ok ? 1 : 0;
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
        dmin = fminf(dmin, __shfl_xor(dmin, x, 64));
        m += __shfl_xor(m, x, 64);
    }
    d = ok ? d - dmin : 0.0f;
    float out = 0.0f, b = 0.0f;
    if (m > 0 && (float)m <= perplexity) {
        out = ok ? cluster::div_rn(1.0f, (float)m) : 0.0f;
    } else if (m > 0) {
        const float target = logf(perplexity);
        tsne::Bisect bs = tsne::bisect_start();
#pragma unroll 1
        for (int step = 0; step < BD_TSNE_BISECTIONS; ++step) {
            const float e = tsne::kernel_term(ok, d, bs.beta);
            tsne::bisect_step(bs, search::butterfly_wave(e), search::butterfly_wave(d * e), target);
        }
        const float e = tsne::kernel_term(ok, d, bs.beta);
        out = cluster::div_rn(e, search::butterfly_wave(e));
        b = bs.beta;
    }
    if (slot) p[at] = out;
    if (lane == 0) beta[i] = b;
}

__global__ __launch_bounds__(kThreads) void tsne_attract_kernel(const int64_t* __restrict__ row_start, const int32_t* __restrict__ nbr,
                                                                 const float* __restrict__ P, int64_t N, int64_t E,
                                                                 const float2* __restrict__ y, float2* __restrict__ attr) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= N) return;                                   // (no barrier in this kernel)
    const int64_t lo = tsne::clamp_index(row_start[i], 0, E);
    const int64_t hi = tsne::clamp_index(row_start[i + 1], lo, E);
    const float2 yi = y[i];
    float ax = 0.0f, ay = 0.0f;
    for (int64_t e = lo + lane; e < hi; e += 64) {
        const float2 yj = y[tsne::clamp_index(nbr[e], 0, N - 1)];
        tsne::attract(P[e], yi.x, yi.y, yj.x, yj.y, ax, ay);
    }
    ax = search::butterfly_wave(ax);
    ay = search::butterfly_wave(ay);
    if (lane == 0) attr[i] = make_float2(ax, ay);
}

__global__ __launch_bounds__(64) void tsne_repulse_kernel(const float2* __restrict__ y, int64_t N, float* __restrict__ part) {
    __shared__ float2 s_y[BD_TSNE_SLICE];
    const int lane = threadIdx.x;
    const int64_t first_i = (int64_t)blockIdx.x * BD_TSNE_ROWS_PER_BLOCK;
    const int64_t slice = blockIdx.y;
    const int64_t first_j = slice * BD_TSNE_SLICE;
    const int nj = N - first_j < BD_TSNE_SLICE ? (int)(N - first_j) : BD_TSNE_SLICE;        // >= 1: the grid has ceil(N / slice) slices
    for (int t = lane; t < nj; t += 64) s_y[t] = y[first_j + t];
    __syncthreads();
    float xi[kRowsPerLane], yi[kRowsPerLane];
    int self[kRowsPerLane];                               // where row i lies in this slice (outside 0 .. nj - 1: not in it)
    tsne::Force f[kRowsPerLane];
#pragma unroll
    for (int r = 0; r < kRowsPerLane; ++r) {
        const int64_t i = first_i + lane + 64 * r;
        const float2 v = y[i < N ? i : N - 1];                // rows past N walk along with the last row and store nothing
        xi[r] = v.x;
        yi[r] = v.y;
        const int64_t rel = i - first_j;
        self[r] = rel >= 0 && rel < BD_TSNE_SLICE ? (int)rel : -1;
        f[r] = tsne::Force{0.0f, 0.0f, 0.0f};
    }
#pragma unroll 2
    for (int t = 0; t < nj; ++t) {
        const float2 c = s_y[t];
#pragma unroll
        for (int r = 0; r < kRowsPerLane; ++r) tsne::repel(xi[r], yi[r], c.x, c.y, t == self[r], f[r]);
    }
    float* px = part + (size_t)slice * 3 * (size_t)N;
#pragma unroll
    for (int r = 0; r < kRowsPerLane; ++r) {
        const int64_t i = first_i + lane + 64 * r;
        if (i < N) {
            px[i] = f[r].x;
            px[(size_t)N + i] = f[r].y;
            px[2 * (size_t)N + i] = f[r].z;
        }
    }
}

__global__ __launch_bounds__(kThreads) void tsne_finish_kernel(const float* __restrict__ part, int64_t N, int64_t slices,
                                                                float2* __restrict__ rep, float* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    float rx = 0.0f, ry = 0.0f, rz = 0.0f;
    for (int64_t s = 0; s < slices; ++s) {
        const float* px = part + (size_t)s * 3 * (size_t)N;
        rx = tsne::chain_add(rx, px[i]);
        ry = tsne::chain_add(ry, px[(size_t)N + i]);
        rz = tsne::chain_add(rz, px[2 * (size_t)N + i]);
    }
    rep[i] = make_float2(rx, ry);
    z[i] = rz;
}

// out[col][slice]; grid (slices, ncol), one wave
__global__ __launch_bounds__(64) void tsne_slice_sums_kernel(const float* __restrict__ src, int ncol, int64_t N, float* __restrict__ out) {
    const float a = tsne::slice_chain(src, ncol, (int)blockIdx.y, (int64_t)blockIdx.x * BD_TSNE_SLICE, N, threadIdx.x);
    const float total = search::butterfly_wave(a);
    if (threadIdx.x == 0) out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// tot[col] = the chain over parts[col][0 .. slices - 1]; one wave, a lane per column; `copy` (may be null) takes tot[0]
__global__ __launch_bounds__(64) void tsne_totals_kernel(const float* __restrict__ parts, int ncol, int64_t slices, float* __restrict__ tot,
                                                          float* __restrict__ copy) {
    const int c = threadIdx.x;
    if (c >= ncol) return;
    float a = 0.0f;
    for (int64_t s = 0; s < slices; ++s) a = tsne::chain_add(a, parts[(size_t)c * slices + s]);
    tot[c] = a;
    if (c == 0 && copy) *copy = a;
}

__global__ __launch_bounds__(kThreads) void tsne_update_kernel(float2* __restrict__ y, float2* __restrict__ v, float2* __restrict__ gain,
                                                                const float2* __restrict__ attr, const float2* __restrict__ rep,
                                                                int64_t N, float exaggeration, float momentum, float rate,
                                                                float min_gain, const float* __restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const float Z = *total;
    const float2 a = attr[i], r = rep[i];
    float2 yy = y[i], vv = v[i], gg = gain[i];
    const float gx = tsne::gradient(exaggeration, a.x, r.x, Z), gy = tsne::gradient(exaggeration, a.y, r.y, Z);
    gg.x = tsne::gain_next(gg.x, gx, vv.x, min_gain);
    gg.y = tsne::gain_next(gg.y, gy, vv.y, min_gain);
    vv.x = tsne::velocity_next(momentum, vv.x, rate, gg.x, gx);
    vv.y = tsne::velocity_next(momentum, vv.y, rate, gg.y, gy);
    yy.x = yy.x + vv.x;
    yy.y = yy.y + vv.y;
    y[i] = yy;
    v[i] = vv;
    gain[i] = gg;
}

__global__ __launch_bounds__(kThreads) void tsne_centre_kernel(float2* __restrict__ y, int64_t N, const float* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    float2 yy = y[i];
    yy.x = yy.x - tsne::mean_of(sums[0], N);
    yy.y = yy.y - tsne::mean_of(sums[1], N);
    y[i] = yy;
}

__global__ __launch_bounds__(kThreads) void tsne_kl_kernel(const int64_t* __restrict__ row_start, const int32_t* __restrict__ nbr,
                                                            const float* __restrict__ P, int64_t N, int64_t E, const float2* __restrict__ y,
                                                            const float* __restrict__ total, float* __restrict__ rowkl) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= N) return;                                   // (no barrier in this kernel)
    const int64_t lo = tsne::clamp_index(row_start[i], 0, E);
    const int64_t hi = tsne::clamp_index(row_start[i + 1], lo, E);
    const float log_total = logf(*total);
    const float2 yi = y[i];
    float t = 0.0f;
    for (int64_t e = lo + lane; e < hi; e += 64) {
        const float2 yj = y[tsne::clamp_index(nbr[e], 0, N - 1)];
        t = tsne::chain_add(t, tsne::kl_term(P[e], yi.x, yi.y, yj.x, yj.y, log_total));
    }
    t = search::butterfly_wave(t);
    if (lane == 0) rowkl[i] = t;
}

// ---------------------------------------------------------------------------------------------------- host side
int check_pointer(const std::string& fn, const char* name, const void* p, int align) {
    if (!p) return fail(BD_EINVAL, fn + name + " is null");
    if ((uintptr_t)p % (uintptr_t)align) return fail(BD_EINVAL, fn + name + " is not " + std::to_string(align) + "-byte aligned");
    return BD_OK;
}

int check_rows(const std::string& fn, int64_t N) {
    if (N < 0 || N > BD_TSNE_MAX_ROWS)
        return fail(BD_EINVAL, fn + "rows = " + std::to_string(N) + ", a call takes 0.." + std::to_string(BD_TSNE_MAX_ROWS));
    return BD_OK;
}

int check_workspace(const std::string& fn, int64_t N, const void* ws, int64_t bytes) {
    int rc = check_pointer(fn, "workspace", ws, 16);
    if (rc != BD_OK) return rc;
    if (bytes < ws_bytes(N))
        return fail(BD_EINVAL, fn + "workspace_bytes = " + std::to_string(bytes) + ", " + std::to_string(N) + " rows take " +
                                   std::to_string(ws_bytes(N)));
    return BD_OK;
}

int check_affinities(const std::string& fn, const int32_t* ids, const float* sims, int64_t N, int32_t k, float perplexity,
                     const float* p, const float* beta) {
    if (k < 1 || k > BD_TSNE_MAX_K) return fail(BD_EINVAL, fn + "k = " + std::to_string(k) + ", allowed are 1.." + std::to_string(BD_TSNE_MAX_K));
    if (!(perplexity >= 1.0f) || perplexity - perplexity != 0.0f)
        return fail(BD_EINVAL, fn + "perplexity = " + std::to_string(perplexity) + " must be finite and at least 1");
    int rc = check_rows(fn, N);
    if (rc != BD_OK || N == 0) return rc;
    if ((rc = check_pointer(fn, "ids", ids, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "sims", sims, 4)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "p", p, 4)) != BD_OK) return rc;
    return check_pointer(fn, "beta", beta, 4);
}

int check_graph(const std::string& fn, const int64_t* row_start, const int32_t* nbr, const float* P, int64_t N, int64_t E, const float* y) {
    if (E < 0) return fail(BD_EINVAL, fn + "edges = " + std::to_string(E) + " is negative");
    int rc = check_rows(fn, N);
    if (rc != BD_OK || N == 0) return rc;
    if ((rc = check_pointer(fn, "row_start", row_start, 8)) != BD_OK) return rc;
    if (E > 0 && (rc = check_pointer(fn, "nbr", nbr, 4)) != BD_OK) return rc;
    if (E > 0 && (rc = check_pointer(fn, "p", P, 4)) != BD_OK) return rc;
    return check_pointer(fn, "y", y, 8);
}

// what only the host can look at
int check_graph_host(const std::string& fn, const int64_t* row_start, const int32_t* nbr, int64_t N, int64_t E) {
    if (row_start[0] != 0 || row_start[N] != E)
        return fail(BD_ERANGE, fn + "row_start runs from " + std::to_string(row_start[0]) + " to " + std::to_string(row_start[N]) +
                                   ", not from 0 to edges = " + std::to_string(E));
    for (int64_t i = 0; i < N; ++i)
        if (row_start[i] > row_start[i + 1]) return fail(BD_ERANGE, fn + "row_start[" + std::to_string(i) + "..] does not ascend");
    for (int64_t e = 0; e < E; ++e)
        if (nbr[e] < 0 || nbr[e] >= N) return fail(BD_ERANGE, fn + "nbr[" + std::to_string(e) + "] = " + std::to_string(nbr[e]) + " is no row");
    return BD_OK;
}

int check_update(const std::string& fn, const float* y, const float* v, const float* gain, const float* attr, const float* rep,
                 const float* z, int64_t N) {
    int rc = check_rows(fn, N);
    if (rc != BD_OK || N == 0) return rc;
    if ((rc = check_pointer(fn, "y", y, 8)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "v", v, 8)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "gain", gain, 8)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "attr", attr, 8)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "rep", rep, 8)) != BD_OK) return rc;
    return check_pointer(fn, "z", z, 4);
}

int check_repulse(const std::string& fn, const float* y, int64_t N, const float* rep, const float* z) {
    int rc = check_rows(fn, N);
    if (rc != BD_OK || N == 0) return rc;
    if ((rc = check_pointer(fn, "y", y, 8)) != BD_OK) return rc;
    if ((rc = check_pointer(fn, "rep", rep, 8)) != BD_OK) return rc;
    return check_pointer(fn, "z", z, 4);
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// the slice sums of column `col` of src [rows][ncol] on the host
float slice_sums_host(const float* src, int ncol, int col, int64_t N) {
    float total = 0.0f;
    for (int64_t first = 0; first < N; first += BD_TSNE_SLICE) {
        float lanes[64];
        for (int lane = 0; lane < 64; ++lane) lanes[lane] = tsne::slice_chain(src, ncol, col, first, N, lane);
        total = tsne::chain_add(total, search::butterfly_host(lanes));
    }
    return total;
}

}  // namespace
}  // namespace bd

extern "C" {

int bd_tsne_abi_version(void) { return BD_TSNE_ABI_VERSION; }

int64_t bd_tsne_workspace_bytes(int64_t rows) {
    const int rc = bd::check_rows("bd_tsne_workspace_bytes: ", rows);
    return rc != BD_OK ? rc : bd::ws_bytes(rows);
}

int bd_tsne_affinities(const int32_t* ids_dev, const float* sims_dev, int64_t rows, int32_t k, float perplexity, float* p_dev,
                       float* beta_dev, void* stream) {
    const std::string fn = "bd_tsne_affinities: ";
    const int rc = bd::check_affinities(fn, ids_dev, sims_dev, rows, k, perplexity, p_dev, beta_dev);
    if (rc != BD_OK || rows == 0) return rc;
    hipLaunchKernelGGL(bd::tsne_affinities_kernel, dim3(bd::blocks_of(rows, bd::kWaves)), dim3(bd::kThreads), 0,
                       static_cast<hipStream_t>(stream), ids_dev, sims_dev, rows, (int)k, perplexity, p_dev, beta_dev);
    return bd::hip_result(fn);
}

int bd_tsne_affinities_host(const int32_t* ids, const float* sims, int64_t rows, int32_t k, float perplexity, float* p, float* beta) {
    namespace ts = bd::tsne;
    const int rc = bd::check_affinities("bd_tsne_affinities_host: ", ids, sims, rows, k, perplexity, p, beta);
    if (rc != BD_OK) return rc;
    const float target = logf(perplexity);
    for (int64_t i = 0; i < rows; ++i) {
        bool ok[64];
        float d[64], e[64], s[64], a[64];
        float dmin = INFINITY;
        int m = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const size_t at = (size_t)i * k + (lane < k ? lane : 0);
            ok[lane] = lane < k && ts::usable(ids[at], sims[at]);
            d[lane] = ok[lane] ? ts::distance(sims[at]) : INFINITY;
            dmin = fminf(dmin, d[lane]);
            m += ok[lane] ? 1 : 0;
        }
        for (int lane = 0; lane < 64; ++lane) d[lane] = ok[lane] ? d[lane] - dmin : 0.0f;
        float b = 0.0f;
        if (m > 0 && (float)m <= perplexity) {
            for (int lane = 0; lane < 64; ++lane) e[lane] = ok[lane] ? bd::cluster::div_rn(1.0f, (float)m) : 0.0f;
        } else if (m > 0) {
            ts::Bisect bs = ts::bisect_start();
            for (int step = 0; step < BD_TSNE_BISECTIONS; ++step) {
                for (int lane = 0; lane < 64; ++lane) {
                    s[lane] = ts::kernel_term(ok[lane], d[lane], bs.beta);
                    a[lane] = d[lane] * s[lane];
                }
                const float sum = bd::search::butterfly_host(s);
                ts::bisect_step(bs, sum, bd::search::butterfly_host(a), target);
            }
            for (int lane = 0; lane < 64; ++lane) s[lane] = e[lane] = ts::kernel_term(ok[lane], d[lane], bs.beta);
            const float sum = bd::search::butterfly_host(s);
            for (int lane = 0; lane < 64; ++lane) e[lane] = bd::cluster::div_rn(e[lane], sum);
            b = bs.beta;
        } else {
            for (int lane = 0; lane < 64; ++lane) e[lane] = 0.0f;
        }
        for (int lane = 0; lane < k; ++lane) p[(size_t)i * k + lane] = e[lane];
        beta[i] = b;
    }
    return BD_OK;
}

int bd_tsne_attract(const int64_t* row_start_dev, const int32_t* nbr_dev, const float* p_dev, int64_t rows, int64_t edges,
                    const float* y_dev, float* attr_dev, void* stream) {
    const std::string fn = "bd_tsne_attract: ";
    int rc = bd::check_graph(fn, row_start_dev, nbr_dev, p_dev, rows, edges, y_dev);
    if (rc != BD_OK || rows == 0) return rc;
    if ((rc = bd::check_pointer(fn, "attr", attr_dev, 8)) != BD_OK) return rc;
    hipLaunchKernelGGL(bd::tsne_attract_kernel, dim3(bd::blocks_of(rows, bd::kWaves)), dim3(bd::kThreads), 0,
                       static_cast<hipStream_t>(stream), row_start_dev, nbr_dev, p_dev, rows, edges,
                       reinterpret_cast<const float2*>(y_dev), reinterpret_cast<float2*>(attr_dev));
    return bd::hip_result(fn);
}

int bd_tsne_attract_host(const int64_t* row_start, const int32_t* nbr, const float* p, int64_t rows, int64_t edges, const float* y,
                         float* attr) {
    const std::string fn = "bd_tsne_attract_host: ";
    int rc = bd::check_graph(fn, row_start, nbr, p, rows, edges, y);
    if (rc != BD_OK || rows == 0) return rc;
    if ((rc = bd::check_pointer(fn, "attr", attr, 8)) != BD_OK) return rc;
    if ((rc = bd::check_graph_host(fn, row_start, nbr, rows, edges)) != BD_OK) return rc;
    for (int64_t i = 0; i < rows; ++i) {
        float ax[64], ay[64];
        for (int lane = 0; lane < 64; ++lane) {
            ax[lane] = ay[lane] = 0.0f;
            for (int64_t e = row_start[i] + lane; e < row_start[i + 1]; e += 64)
                bd::tsne::attract(p[e], y[2 * i], y[2 * i + 1], y[2 * (size_t)nbr[e]], y[2 * (size_t)nbr[e] + 1], ax[lane], ay[lane]);
        }
        attr[2 * i] = bd::search::butterfly_host(ax);
        attr[2 * i + 1] = bd::search::butterfly_host(ay);
    }
    return BD_OK;
}

int bd_tsne_repulse(const float* y_dev, int64_t rows, float* rep_dev, float* z_dev, void* workspace_dev, int64_t workspace_bytes,
                    void* stream) {
    const std::string fn = "bd_tsne_repulse: ";
    int rc = bd::check_repulse(fn, y_dev, rows, rep_dev, z_dev);
    if (rc != BD_OK || rows == 0) return rc;
    if ((rc = bd::check_workspace(fn, rows, workspace_dev, workspace_bytes)) != BD_OK) return rc;
    const bd::WsLayout w = bd::ws_layout(rows);
    float* ws = static_cast<float*>(workspace_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(bd::tsne_repulse_kernel, dim3(bd::blocks_of(rows, BD_TSNE_ROWS_PER_BLOCK), (unsigned)w.slices), dim3(64), 0, s,
                       reinterpret_cast<const float2*>(y_dev), rows, ws + w.part);
    hipLaunchKernelGGL(bd::tsne_finish_kernel, dim3(bd::blocks_of(rows, bd::kThreads)), dim3(bd::kThreads), 0, s, ws + w.part, rows,
                       w.slices, reinterpret_cast<float2*>(rep_dev), z_dev);
    return bd::hip_result(fn);
}

int bd_tsne_repulse_host(const float* y, int64_t rows, float* rep, float* z) {
    const int rc = bd::check_repulse("bd_tsne_repulse_host: ", y, rows, rep, z);
    if (rc != BD_OK) return rc;
    for (int64_t i = 0; i < rows; ++i) {
        float rx = 0.0f, ry = 0.0f, rz = 0.0f;
        for (int64_t first = 0; first < rows; first += BD_TSNE_SLICE) {
            bd::tsne::Force f{0.0f, 0.0f, 0.0f};
            const int64_t last = std::min<int64_t>(first + BD_TSNE_SLICE, rows);
            for (int64_t j = first; j < last; ++j) bd::tsne::repel(y[2 * i], y[2 * i + 1], y[2 * j], y[2 * j + 1], j == i, f);
            rx = bd::tsne::chain_add(rx, f.x);
            ry = bd::tsne::chain_add(ry, f.y);
            rz = bd::tsne::chain_add(rz, f.z);
        }
        rep[2 * i] = rx;
        rep[2 * i + 1] = ry;
        z[i] = rz;
    }
    return BD_OK;
}

int bd_tsne_update(float* y_dev, float* v_dev, float* gain_dev, const float* attr_dev, const float* rep_dev, const float* z_dev,
                   int64_t rows, float exaggeration, float momentum, float rate, float min_gain, float* total_dev, void* workspace_dev,
                   int64_t workspace_bytes, void* stream) {
    const std::string fn = "bd_tsne_update: ";
    int rc = bd::check_update(fn, y_dev, v_dev, gain_dev, attr_dev, rep_dev, z_dev, rows);
    if (rc != BD_OK || rows == 0) return rc;
    if (total_dev && (rc = bd::check_pointer(fn, "total", total_dev, 4)) != BD_OK) return rc;
    if ((rc = bd::check_workspace(fn, rows, workspace_dev, workspace_bytes)) != BD_OK) return rc;
    const bd::WsLayout w = bd::ws_layout(rows);
    float* ws = static_cast<float*>(workspace_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned per_row = bd::blocks_of(rows, bd::kThreads);
    hipLaunchKernelGGL(bd::tsne_slice_sums_kernel, dim3((unsigned)w.slices, 1), dim3(64), 0, s, z_dev, 1, rows, ws + w.zpart);
    hipLaunchKernelGGL(bd::tsne_totals_kernel, dim3(1), dim3(64), 0, s, ws + w.zpart, 1, w.slices, ws + w.tot, total_dev);
    hipLaunchKernelGGL(bd::tsne_update_kernel, dim3(per_row), dim3(bd::kThreads), 0, s, reinterpret_cast<float2*>(y_dev),
                       reinterpret_cast<float2*>(v_dev), reinterpret_cast<float2*>(gain_dev), reinterpret_cast<const float2*>(attr_dev),
                       reinterpret_cast<const float2*>(rep_dev), rows, exaggeration, momentum, rate, min_gain, ws + w.tot);
    hipLaunchKernelGGL(bd::tsne_slice_sums_kernel, dim3((unsigned)w.slices, 2), dim3(64), 0, s, y_dev, 2, rows, ws + w.mpart);
    hipLaunchKernelGGL(bd::tsne_totals_kernel, dim3(1), dim3(64), 0, s, ws + w.mpart, 2, w.slices, ws + w.tot + 1, (float*)nullptr);
    hipLaunchKernelGGL(bd::tsne_centre_kernel, dim3(per_row), dim3(bd::kThreads), 0, s, reinterpret_cast<float2*>(y_dev), rows,
                       ws + w.tot + 1);
    return bd::hip_result(fn);
}

int bd_tsne_update_host(float* y, float* v, float* gain, const float* attr, const float* rep, const float* z, int64_t rows,
                        float exaggeration, float momentum, float rate, float min_gain, float* total) {
    namespace ts = bd::tsne;
    const int rc = bd::check_update("bd_tsne_update_host: ", y, v, gain, attr, rep, z, rows);
    if (rc != BD_OK || rows == 0) return rc;
    const float Z = bd::slice_sums_host(z, 1, 0, rows);
    if (total) *total = Z;
    for (int64_t at = 0; at < 2 * rows; ++at) {
        const float g = ts::gradient(exaggeration, attr[at], rep[at], Z);
        gain[at] = ts::gain_next(gain[at], g, v[at], min_gain);
        v[at] = ts::velocity_next(momentum, v[at], rate, gain[at], g);
        y[at] = y[at] + v[at];
    }
    const float mx = ts::mean_of(bd::slice_sums_host(y, 2, 0, rows), rows), my = ts::mean_of(bd::slice_sums_host(y, 2, 1, rows), rows);
    for (int64_t i = 0; i < rows; ++i) {
        y[2 * i] = y[2 * i] - mx;
        y[2 * i + 1] = y[2 * i + 1] - my;
    }
    return BD_OK;
}

int bd_tsne_kl(const int64_t* row_start_dev, const int32_t* nbr_dev, const float* p_dev, int64_t rows, int64_t edges, const float* y_dev,
               const float* z_dev, float* kl_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    const std::string fn = "bd_tsne_kl: ";
    int rc = bd::check_graph(fn, row_start_dev, nbr_dev, p_dev, rows, edges, y_dev);
    if (rc != BD_OK || rows == 0) return rc;
    if ((rc = bd::check_pointer(fn, "z", z_dev, 4)) != BD_OK) return rc;
    if ((rc = bd::check_pointer(fn, "kl", kl_dev, 4)) != BD_OK) return rc;
    if ((rc = bd::check_workspace(fn, rows, workspace_dev, workspace_bytes)) != BD_OK) return rc;
    const bd::WsLayout w = bd::ws_layout(rows);
    float* ws = static_cast<float*>(workspace_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(bd::tsne_slice_sums_kernel, dim3((unsigned)w.slices, 1), dim3(64), 0, s, z_dev, 1, rows, ws + w.zpart);
    hipLaunchKernelGGL(bd::tsne_totals_kernel, dim3(1), dim3(64), 0, s, ws + w.zpart, 1, w.slices, ws + w.tot, (float*)nullptr);
    hipLaunchKernelGGL(bd::tsne_kl_kernel, dim3(bd::blocks_of(rows, bd::kWaves)), dim3(bd::kThreads), 0, s, row_start_dev, nbr_dev, p_dev,
                       rows, edges, reinterpret_cast<const float2*>(y_dev), ws + w.tot, ws + w.rowkl);
    hipLaunchKernelGGL(bd::tsne_slice_sums_kernel, dim3((unsigned)w.slices, 1), dim3(64), 0, s, ws + w.rowkl, 1, rows, ws + w.klpart);
    hipLaunchKernelGGL(bd::tsne_totals_kernel, dim3(1), dim3(64), 0, s, ws + w.klpart, 1, w.slices, ws + w.tot + 3, kl_dev);
    return bd::hip_result(fn);
}

int bd_tsne_kl_host(const int64_t* row_start, const int32_t* nbr, const float* p, int64_t rows, int64_t edges, const float* y,
                    const float* z, float* kl) {
    const std::string fn = "bd_tsne_kl_host: ";
    int rc = bd::check_graph(fn, row_start, nbr, p, rows, edges, y);
    if (rc != BD_OK) return rc;
    if ((rc = bd::check_pointer(fn, "kl", kl, 4)) != BD_OK) return rc;
    if (rows == 0) {
        *kl = 0.0f;
        return BD_OK;
    }
    if ((rc = bd::check_pointer(fn, "z", z, 4)) != BD_OK) return rc;
    if ((rc = bd::check_graph_host(fn, row_start, nbr, rows, edges)) != BD_OK) return rc;
    const float log_total = logf(bd::slice_sums_host(z, 1, 0, rows));
    std::vector<float> rowkl((size_t)rows);
    for (int64_t i = 0; i < rows; ++i) {
        float t[64];
        for (int lane = 0; lane < 64; ++lane) {
            t[lane] = 0.0f;
            for (int64_t e = row_start[i] + lane; e < row_start[i + 1]; e += 64)
                t[lane] = bd::tsne::chain_add(t[lane], bd::tsne::kl_term(p[e], y[2 * i], y[2 * i + 1], y[2 * (size_t)nbr[e]],
                                                                         y[2 * (size_t)nbr[e] + 1], log_total));
        }
        rowkl[(size_t)i] = bd::search::butterfly_host(t);
    }
    *kl = bd::slice_sums_host(rowkl.data(), 1, 0, rows);
    return BD_OK;
}

}  // extern "C"
