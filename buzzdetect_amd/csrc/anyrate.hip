// Any-ratio downmix + resample for gfx950 (include/buzzdetect_anyrate.h; the streamer's np.mean(axis=1) +
// librosa.resample(y, orig_sr, 16000), src/stream/worker.py:116-128, for the rates bd_resample's one-pass plans do not
// cover: ratios that do not reduce to <= 4096 and HQ decimations beyond ~43 : 1).
//
// y[j] = sum_i mono[i] h[j down - i up + half] with h the soxr_hq-class Kaiser-windowed sinc of
// oracle/resample_oracle.py.  47 999 -> 16 000 Hz is 16000 / 47999: h has 9 M taps, of which one output uses ~567, a
// different 567 for each of 16 000 consecutive outputs.  So the coefficients come from the continuous prototype
// g(t) = h(up t), t = i - j down / up input samples, kept as a table of rows g(q - W - phase), q = 0 .. 2 W:
//
//   up <= 256   `up` rows, row r = phase r / up: the polyphase rows of h, exactly (768 kHz: one row of 9 067 taps);
//   otherwise   259 rows at phases -1/256 .. 257/256.  An output at phase (p + a) / 256 takes a dot product of its input
//               span with each of the rows p - 1 .. p + 2 and combines the four with the cubic Lagrange weights of a
//               (the interpolation is linear in the rows, so it is applied once per output, not once per tap).  The
//               interpolation error of a 256-phase cubic on this prototype is below 1e-9 of full scale; the float32
//               rounding of the rows (6e-8 relative) is the floor.
//
// Layout.  Consecutive outputs have unrelated phases, so with one output per lane every coefficient load would touch
// 64 rows (64 cache lines).  Here a WAVE owns an output: lane l takes taps l, l + 64, ... of the row, so a row is read
// as consecutive 256-byte lines and the staged input as consecutive LDS words (no bank conflict), and the four
// Lagrange rows are four such streams.  The table of a 3 : 1 ratio is 259 x 576 floats (597 kB) and stays in L2.  A
// (value, delta) pair per entry would halve the loads of a linear interpolation but needs 4096 phases for the same
// error, 16 x the table, which no longer fits L2; four plain rows of a small table are the cheaper stream.
//
// anyrate_kernel<T, EXACT>: a 4-wave workgroup owns a tile of tj <= 64 consecutive outputs.  Per piece of kp taps
// (one piece where the filter span fits, else the span is walked piece by piece) it stages the channel mean of the
// inputs the tile's outputs need over those taps in LDS (zeros outside the signal), then wave w runs outputs w, w + 4, ...:
// per lane 1 (EXACT) or 4 accumulators over its taps in increasing tap order, the Lagrange combination, a butterfly
// over the 64 lanes (xor 32, 16, .. 1) and lane 0 adds the piece's value to the output's running sum in LDS.  The
// order of every addition is fixed by (ratio, j) alone: no atomics, no dependence on the launch around it.
// Positions are 64-bit (j down exceeds 2^32).  bd_resample_any_host walks the same lanes in the same order on the host.
#include "bd_internal.h"
#include "bd_error.h"

#include "../../include/buzzdetect_anyrate.h"

#include <cmath>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace bd {
namespace {

constexpr int kArWaves = 4;
constexpr int kArThreads = 64 * kArWaves;
constexpr int kArCap = 12288;               // input samples staged per piece (48 KB)
constexpr int kArMaxTile = 64;

// ---- arithmetic shared by the kernel and the host restatement ----
__host__ __device__ __forceinline__ float ar_pcm(float v) { return v; }
__host__ __device__ __forceinline__ float ar_pcm(short v) { return (float)v * (1.0f / 32768.0f); }

// the channel mean as frontend.hip's mono_at computes it (np.mean(axis=1) in float32)
__host__ __device__ __forceinline__ float ar_mono(const float* __restrict__ in, long long i, int channels) {
    if (channels == 1) return in[i];
    if (channels == 2) return (in[2 * i] + in[2 * i + 1]) * 0.5f;
    const float* __restrict__ frame = in + i * channels;
    return np_row_sum(channels, [&](int ch) { return frame[ch]; }) / (float)channels;
}
__host__ __device__ __forceinline__ float ar_mono(const short* __restrict__ in, long long i, int channels) {
    if (channels == 1) return ar_pcm(in[i]);
    if (channels == 2) return (float)((int)in[2 * i] + (int)in[2 * i + 1]) * (1.0f / 65536.0f);      // exact
    const short* __restrict__ frame = in + i * channels;
    return np_row_sum(channels, [&](int ch) { return ar_pcm(frame[ch]); }) / (float)channels;
}

// Row and Lagrange weights of an output whose position is n + r / up input samples (interpolated tables): the phase
// in 256ths is p + a; the rows p .. p + 3 of the table are the nodes -1, 0, 1, 2 of a.  Products of differences only:
// nothing here can contract into an fma on one side and not on the other.
__host__ __device__ __forceinline__ int ar_phase(int r, int up, float (&lw)[4]) {
    const double phi = ((double)r * (double)BD_ANYRATE_PHASES) / (double)up;
    const int p = (int)phi;
    const double a = phi - (double)p;
    const double am = a - 1.0, ap = a + 1.0, a2 = a - 2.0;
    lw[0] = (float)(a * am * a2 * (-1.0 / 6.0));
    lw[1] = (float)(ap * am * a2 * 0.5);
    lw[2] = (float)(ap * a * a2 * -0.5);
    lw[3] = (float)(ap * a * am * (1.0 / 6.0));
    return p;
}

__host__ __device__ __forceinline__ float ar_combine(const float (&lw)[4], float a0, float a1, float a2, float a3) {
    return fmaf(lw[3], a3, fmaf(lw[2], a2, fmaf(lw[1], a1, lw[0] * a0)));
}

template <typename T, bool EXACT>
__global__ __launch_bounds__(kArThreads) void anyrate_kernel(const T* __restrict__ in, long long n_in, int channels,
                                                             const float* __restrict__ table, const AnyratePlan g,
                                                             float* __restrict__ out, long long n_out) {
    __shared__ float s_x[kArCap];
    __shared__ float s_acc[kArMaxTile];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long j0 = (long long)blockIdx.x * g.tj;
    const int nj = n_out - j0 < g.tj ? (int)(n_out - j0) : g.tj;
    const unsigned long long up = (unsigned long long)g.up, down = (unsigned long long)g.down;
    const long long n0 = (long long)((unsigned long long)j0 * down / up);        // first input position of the tile
    const unsigned long long num_w = (unsigned long long)(j0 + wave) * down;     // this wave's first output
    const long long n_w = (long long)(num_w / up);
    const int r_w = (int)(num_w % up);
    if (tid < kArMaxTile) s_acc[tid] = 0.0f;
    for (int q0 = 0; q0 < g.kw; q0 += g.kp) {
        const int kp = g.kw - q0 < g.kp ? g.kw - q0 : g.kp;
        const long long i_lo = n0 - g.W + q0;
        __syncthreads();                                        // the previous piece is consumed (first: s_acc is zero)
        for (int k = tid; k < kp + g.spread; k += kArThreads) {
            const long long i = i_lo + k;
            s_x[k] = i >= 0 && i < n_in ? ar_mono(in, i, channels) : 0.0f;
        }
        __syncthreads();
        long long n = n_w;
        int r = r_w;
        for (int o = wave; o < nj; o += kArWaves) {
            const float* __restrict__ x = s_x + (int)(n - n0);
            float v;
            if constexpr (EXACT) {
                const float* __restrict__ row = table + (size_t)r * g.kw + q0;
                float a0 = 0.0f;
#pragma unroll 4
                for (int q = lane; q < kp; q += 64) a0 = fmaf(x[q], row[q], a0);
                v = a0;
            } else {
                float lw[4];
                const int p = ar_phase(r, g.up, lw);
                const float* __restrict__ row0 = table + (size_t)p * g.kw + q0;
                const float* __restrict__ row1 = row0 + g.kw;
                const float* __restrict__ row2 = row1 + g.kw;
                const float* __restrict__ row3 = row2 + g.kw;
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll 3
                for (int q = lane; q < kp; q += 64) {
                    const float xv = x[q];
                    a0 = fmaf(xv, row0[q], a0);
                    a1 = fmaf(xv, row1[q], a1);
                    a2 = fmaf(xv, row2[q], a2);
                    a3 = fmaf(xv, row3[q], a3);
                }
                v = ar_combine(lw, a0, a1, a2, a3);
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
            if (lane == 0) s_acc[o] += v;                       // only this wave touches s_acc[o]
            n += g.step_n;
            r += g.step_r;
            if (r >= g.up) {
                r -= g.up;
                ++n;
            }
        }
    }
    __syncthreads();
    if (tid < nj) out[j0 + tid] = s_acc[tid];
}

// ---- design (resample_host.hip's design_taps at BD_RESAMPLE_HQ, oracle/resample_oracle.py taps(), as a function of u) ----
double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 256; ++k) {
        term *= (x / (2.0 * k)) * (x / (2.0 * k));
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

struct Proto {
    long long half;          // h has 2 half + 1 taps
    double cutoff, beta, i0b, gain;

    double shape(double u) const {      // cutoff sinc(cutoff u) kaiser(u / half), |u| <= half
        const double x = cutoff * u;
        const double sinc = u == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        const double rr = half > 0 ? u / (double)half : 0.0;
        return cutoff * sinc * bessel_i0(beta * std::sqrt(rr * rr < 1.0 ? 1.0 - rr * rr : 0.0)) / i0b;
    }
    double at(double u) const { return std::fabs(u) <= (double)half ? gain * shape(u) : 0.0; }
};

Proto design(int up, int down) {
    const int max_rate = up > down ? up : down;
    Proto p;
    const double rej = 20.0 * 20.0 * std::log10(2.0);                       // libsoxr HQ: 20-bit precision
    const double to_3db = (1.6e-6 * rej - 7.5e-4) * rej + 0.646;
    const double fp = (1.0 - 0.05 / to_3db) / max_rate, fs = 1.0 / max_rate;
    const double att = 125.0;
    p.beta = 0.1102 * (att - 8.7);
    p.i0b = bessel_i0(p.beta);
    p.cutoff = 0.5 * (fp + fs);
    const long long n = (long long)std::ceil((att - 7.95) / (2.285 * M_PI * (fs - fp))) + 1;
    p.half = max_rate == 1 ? 0 : n / 2;                                      // equal rates: a copy
    p.gain = 0.0;
    return p;
}

// up / sum_m shape(m): h is normalised to unity DC gain over its integer taps.  Past 2^20 taps the sum is taken over every
// s-th tap (times s): shape is band-limited to ~1 / (2 max_rate) cycles per tap and s stays below max_rate / 1000, so the
// aliases that differ between the two sums lie thousands of transition widths into the stop band (< 1e-12 of the sum).
double proto_gain(const Proto& p, int up) {
    const long long n = 2 * p.half + 1;
    const long long s = n <= (1ll << 20) ? 1 : (n + (1ll << 18) - 1) >> 18;
    double sum = p.shape(0.0);
    for (long long m = s; m <= p.half; m += s) sum += 2.0 * p.shape((double)m);
    return (double)up / (sum * (double)s);
}

}  // namespace

bool anyrate_plan(int up, int down, AnyratePlan* plan) {
    if (up <= 0 || down <= 0 || up >= BD_ANYRATE_MAX_RATE || down >= BD_ANYRATE_MAX_RATE) return false;
    const Proto p = design(up, down);
    AnyratePlan g;
    g.up = up;
    g.down = down;
    g.exact = up <= BD_ANYRATE_PHASES;
    g.rows = g.exact ? up : BD_ANYRATE_PHASES + 3;
    const long long W = p.half / up + 2;
    const long long kw = (2 * W + 1 + 63) / 64 * 64;
    if ((long long)g.rows * kw * 4 > BD_ANYRATE_MAX_TABLE_BYTES) return false;
    g.W = (int)W;
    g.kw = (int)kw;
    g.tj = kArMaxTile;
    for (;;) {                      // the largest tile whose outputs start within half of the staged span
        g.spread = (int)((long long)(g.tj - 1) * down / up) + 2;
        if (g.spread <= kArCap / 2 || g.tj == 1) break;
        g.tj >>= 1;
    }
    const int room = (kArCap - g.spread) / 64 * 64;
    g.kp = g.kw < room ? g.kw : room;
    g.step_n = (long long)kArWaves * down / up;
    g.step_r = (int)((long long)kArWaves * down % up);
    *plan = g;
    return true;
}

void anyrate_table(const AnyratePlan& g, std::vector<float>* table) {
    Proto p = design(g.up, g.down);
    p.gain = proto_gain(p, g.up);
    table->assign((size_t)g.rows * g.kw, 0.0f);
    for (int row = 0; row < g.rows; ++row)
        for (int q = 0; q <= 2 * g.W; ++q) {
            // offset of input n - W + q from an output at n + phase, in taps of h: u = up (q - W - phase)
            const double u = g.exact ? (double)((long long)g.up * (q - g.W) - row)
                                     : (double)g.up * (double)(q - g.W) - (double)g.up * (double)(row - 1) / BD_ANYRATE_PHASES;
            (*table)[(size_t)row * g.kw + q] = (float)p.at(u);
        }
}

void launch_anyrate(const void* in, bool s16, int64_t n_in, int channels, const AnyratePlan& plan, const float* table,
                    float* out, int64_t n_out, hipStream_t stream) {
    if (n_out <= 0) return;
    const unsigned grid = (unsigned)((n_out + plan.tj - 1) / plan.tj);
#define BD_AR_LAUNCH(T, E)                                                                                        \
    hipLaunchKernelGGL((anyrate_kernel<T, E>), dim3(grid), dim3(kArThreads), 0, stream, static_cast<const T*>(in), \
                       (long long)n_in, channels, table, plan, out, (long long)n_out)
    if (s16) { if (plan.exact) BD_AR_LAUNCH(short, true); else BD_AR_LAUNCH(short, false); }
    else { if (plan.exact) BD_AR_LAUNCH(float, true); else BD_AR_LAUNCH(float, false); }
#undef BD_AR_LAUNCH
}

namespace {

// anyrate_kernel on the host: the same tiles, pieces, lanes and order of additions
template <typename T>
void anyrate_host(const T* in, long long n_in, int channels, const AnyratePlan& g, const float* table, float* out,
                  long long n_out) {
    const unsigned long long up = (unsigned long long)g.up, down = (unsigned long long)g.down;
    std::vector<float> s_x((size_t)g.kp + g.spread);
    for (long long j0 = 0; j0 < n_out; j0 += g.tj) {
        const int nj = n_out - j0 < g.tj ? (int)(n_out - j0) : g.tj;
        const long long n0 = (long long)((unsigned long long)j0 * down / up);
        float acc[kArMaxTile] = {0.0f};
        for (int q0 = 0; q0 < g.kw; q0 += g.kp) {
            const int kp = g.kw - q0 < g.kp ? g.kw - q0 : g.kp;
            const long long i_lo = n0 - g.W + q0;
            for (int k = 0; k < kp + g.spread; ++k) {
                const long long i = i_lo + k;
                s_x[k] = i >= 0 && i < n_in ? ar_mono(in, i, channels) : 0.0f;
            }
            for (int o = 0; o < nj; ++o) {
                const unsigned long long num = (unsigned long long)(j0 + o) * down;
                const long long n = (long long)(num / up);
                const int r = (int)(num % up);
                float lw[4] = {1.0f, 0.0f, 0.0f, 0.0f};
                const int p = g.exact ? r : ar_phase(r, g.up, lw);
                const float* row = table + (size_t)p * g.kw + q0;
                const float* x = s_x.data() + (n - n0);
                float v[64];
                for (int lane = 0; lane < 64; ++lane) {
                    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    for (int q = lane; q < kp; q += 64) {
                        a[0] = fmaf(x[q], row[q], a[0]);
                        if (!g.exact)
                            for (int e = 1; e < 4; ++e) a[e] = fmaf(x[q], row[(size_t)e * g.kw + q], a[e]);
                    }
                    v[lane] = g.exact ? a[0] : ar_combine(lw, a[0], a[1], a[2], a[3]);
                }
                for (int m = 32; m >= 1; m >>= 1) {
                    float t[64];
                    for (int lane = 0; lane < 64; ++lane) t[lane] = v[lane] + v[lane ^ m];
                    for (int lane = 0; lane < 64; ++lane) v[lane] = t[lane];
                }
                acc[o] += v[0];
            }
        }
        for (int o = 0; o < nj; ++o) out[j0 + o] = acc[o];
    }
}

void reduce_ratio(int32_t rate_in, int32_t rate_out, int* up, int* down) {
    int a = rate_out, b = rate_in;
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    *up = rate_out / a;
    *down = rate_in / a;
}

// the host restatement's tables: the last few ratios, so that a test's many short calls design each once
struct HostTable {
    int up, down;
    std::shared_ptr<std::vector<float>> table;
};
std::mutex g_host_mutex;
std::vector<HostTable> g_host_tables;

}  // namespace

}  // namespace bd

extern "C" {

int bd_anyrate_abi_version(void) { return BD_ANYRATE_ABI_VERSION; }

int bd_anyrate_supported(int32_t rate_in, int32_t rate_out, int32_t quality) {
    const int old = bd_resample_supported(rate_in, rate_out, quality);      // also the argument checks (and their text)
    if (old != 0) return old;
    if (quality != BD_RESAMPLE_HQ) return 0;
    int up, down;
    bd::reduce_ratio(rate_in, rate_out, &up, &down);
    bd::AnyratePlan plan;
    return bd::anyrate_plan(up, down, &plan) ? 1 : 0;
}

int bd_resample_any_host(const void* in, int32_t is_s16, int64_t n_in, int32_t channels, int32_t rate_in, int32_t rate_out,
                         float* out) {
    if (n_in < 0 || channels <= 0 || rate_in <= 0 || rate_out <= 0 || (!in && n_in > 0)) {
        bd::set_error("bd_resample_any_host: bad argument");
        return BD_EINVAL;
    }
    int up, down;
    bd::reduce_ratio(rate_in, rate_out, &up, &down);
    bd::AnyratePlan plan;
    if (!bd::anyrate_plan(up, down, &plan)) {
        bd::set_error("bd_resample_any_host: rate pair outside the any-ratio range (buzzdetect_anyrate.h)");
        return BD_EINVAL;
    }
    const int64_t n_out = (n_in * up + down - 1) / down;
    if (n_out > 0 && !out) {
        bd::set_error("bd_resample_any_host: null output");
        return BD_EINVAL;
    }
    std::shared_ptr<std::vector<float>> table;
    {
        std::lock_guard<std::mutex> lock(bd::g_host_mutex);
        for (const auto& t : bd::g_host_tables)
            if (t.up == up && t.down == down) table = t.table;
        if (!table) {
            table = std::make_shared<std::vector<float>>();
            bd::anyrate_table(plan, table.get());
            if (bd::g_host_tables.size() >= 4) bd::g_host_tables.erase(bd::g_host_tables.begin());
            bd::g_host_tables.push_back({up, down, table});
        }
    }
    if (is_s16)
        bd::anyrate_host(static_cast<const short*>(in), (long long)n_in, channels, plan, table->data(), out, (long long)n_out);
    else
        bd::anyrate_host(static_cast<const float*>(in), (long long)n_in, channels, plan, table->data(), out, (long long)n_out);
    return BD_OK;
}

}  // extern "C"
