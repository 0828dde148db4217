// YAMNet (MobileNetV1) body on gfx950: embedders/yamnet/yamnet.py:36-106 with the BatchNorms
// (yamnet.py:26-33, scale=False, eps=1e-4) folded into the convolution weights at load time.
// All activations are NHWC float32, exactly the reference's layout.
// TF "SAME" for an even extent with stride 2 pads 0 before / 1 after; stride 1 pads 1 / 1.
//
// Default path (7 launches per pass): stem_reg_kernel (stemreg.hip: layers 1-2 + depthwise 3),
// l4_window_kernel (l4window.hip: pointwise 3, layer 4, depthwise 5), sep_mid_kernel (sepmid.hip: pointwise 5 + layers 6-7),
// sep_chip_kernel (sepchip.hip: layers 8-12 + depthwise 13), tail_gemm_kernel twice (septail.hip: pointwise 13 + depthwise 14,
// pointwise 14 + pool), pool_head_kernel<1> (here: Dense(1024 -> n_classes) on the pooled embeddings).
// The fallbacks behind bd_set_fusion: stem3_kernel (stem3.hip), sep_ws_kernel and pw_res_kernel (sepws.hip).
// This file is the reference layer, one kernel per op (the fused kernels are tested bit for bit against them; they are also the
// exact-f32 mode's tail):
//   conv1_kernel, depthwise_kernel, scale_copy_kernel, pointwise_f16x3_kernel (split-f16), pointwise_kernel (exact-f32 MFMA, with
//   the next depthwise in its epilogue on request), pool_head_kernel<6>
// and the shape rules that pick a kernel for a 1x1 convolution (launch_pointwise, launch_pointwise_ws).  The launch path reads
// no environment and keeps no mutable state besides the once-per-device dynamic-LDS attribute flags.
#include "bd_device.h"

namespace bd {

namespace {

// --------------------------------------------------------------------------- conv1
constexpr int kC1Rows = 4;   // output rows per workgroup

__global__ __launch_bounds__(256) void conv1_kernel(const float* __restrict__ logmel, int patch_step,
                                                    const WindowMap map, int w0,
                                                    const float* __restrict__ w9x32,
                                                    const float* __restrict__ b32,
                                                    float* __restrict__ out) {
    // grid: (48 / kC1Rows, windows); thread = (ow = tid >> 3, c4 = tid & 7)
    const int tid = threadIdx.x;
    const int c4 = tid & 7;
    const int ow = tid >> 3;
    const int win = blockIdx.y;
    const float* patch = logmel + window_frame(map, w0 + win, patch_step) * BD_MEL_BANDS;

    float4 wt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t] = reinterpret_cast<const float4*>(w9x32 + t * 32)[c4];
    const float4 bias = reinterpret_cast<const float4*>(b32)[c4];

#pragma unroll
    for (int rr = 0; rr < kC1Rows; ++rr) {
        const int oh = blockIdx.x * kC1Rows + rr;
        float4 acc = bias;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int ih = 2 * oh + kh;                      // pad_top = 0
            if (ih < BD_PATCH_FRAMES) {
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int iw = 2 * ow + kw;              // pad_left = 0
                    const float v = iw < BD_MEL_BANDS ? patch[ih * BD_MEL_BANDS + iw] : 0.0f;
                    const float4 w = wt[kh * 3 + kw];
                    acc.x = fmaf(v, w.x, acc.x);
                    acc.y = fmaf(v, w.y, acc.y);
                    acc.z = fmaf(v, w.z, acc.z);
                    acc.w = fmaf(v, w.w, acc.w);
                }
            }
        }
        acc.x = fmaxf(acc.x, 0.0f);
        acc.y = fmaxf(acc.y, 0.0f);
        acc.z = fmaxf(acc.z, 0.0f);
        acc.w = fmaxf(acc.w, 0.0f);
        reinterpret_cast<float4*>(out + (((size_t)win * 48 + oh) * 32 + ow) * 32)[c4] = acc;
    }
}

// --------------------------------------------------------------------------- depthwise
// One thread = OWB consecutive outputs of one row for one float4 of channels: the 3 x ((OWB-1)*S+3)
// input patch is loaded once into registers and reused by the OWB outputs (4.5 instead of 9 loads per
// output at stride 1), the 9 taps are loaded once per thread.  Channels are the fastest thread index,
// so a wavefront reads/writes whole 128-byte-or-longer runs of the NHWC rows.
// TF SAME: stride 1 pads 1 before; stride 2 on the even extents used here pads 0 before, 1 after.
template <int STRIDE, int OWB>
__global__ __launch_bounds__(256) void depthwise_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                        const float* __restrict__ w9xc,
                                                        const float* __restrict__ bias, int windows, int H,
                                                        int W, int C, int OH, int OW,
                                                        unsigned* __restrict__ amax) {
    constexpr int PAD = STRIDE == 1 ? 1 : 0;
    float cmax = 0.0f;                       // calibration pass (amax != null): largest output of this thread
    constexpr int NCOL = (OWB - 1) * STRIDE + 3;
    const int c4n = C >> 2;
    const int owg = OW / OWB;
    const long long total = (long long)windows * OH * owg * c4n;
    // workgroups go to the XCDs round-robin by ID: give every XCD a contiguous run of the index space, so that
    // IDs b and b + 8 (same L2, dispatched together) are neighbours and the input rows they share are fetched once
    const unsigned per_ = gridDim.x >> 3;
    const unsigned bid = blockIdx.x < per_ * 8 ? (blockIdx.x & 7) * per_ + (blockIdx.x >> 3) : blockIdx.x;
    for (long long i = bid * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
        const int c4 = (int)(i % c4n);
        long long t = i / c4n;
        const int og = (int)(t % owg);
        t /= owg;
        const int oh = (int)(t % OH);
        const long long n = t / OH;
        const int ow0 = og * OWB;
        const float4* src = reinterpret_cast<const float4*>(in + (size_t)n * H * W * C) + c4;
        float4 wt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wt[k] = reinterpret_cast<const float4*>(w9xc + k * C)[c4];
        const float4 b = reinterpret_cast<const float4*>(bias)[c4];
        float4 acc[OWB];
#pragma unroll
        for (int o = 0; o < OWB; ++o) acc[o] = b;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int ih = oh * STRIDE + kh - PAD;
            const bool row_ok = ih >= 0 && ih < H;
            float4 col[NCOL];
#pragma unroll
            for (int c = 0; c < NCOL; ++c) {
                const int iw = ow0 * STRIDE + c - PAD;
                col[c] = (row_ok && iw >= 0 && iw < W) ? src[((size_t)ih * W + iw) * c4n]
                                                       : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int o = 0; o < OWB; ++o)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float4 v = col[o * STRIDE + kw];
                    const float4 w = wt[kh * 3 + kw];
                    acc[o].x = fmaf(v.x, w.x, acc[o].x);
                    acc[o].y = fmaf(v.y, w.y, acc[o].y);
                    acc[o].z = fmaf(v.z, w.z, acc[o].z);
                    acc[o].w = fmaf(v.w, w.w, acc[o].w);
                }
        }
        float4* dst = reinterpret_cast<float4*>(out + (((size_t)n * OH + oh) * OW + ow0) * C) + c4;
#pragma unroll
        for (int o = 0; o < OWB; ++o) {
            float4 r = acc[o];
            r.x = fmaxf(r.x, 0.0f);
            r.y = fmaxf(r.y, 0.0f);
            r.z = fmaxf(r.z, 0.0f);
            r.w = fmaxf(r.w, 0.0f);
            dst[(size_t)o * c4n] = r;
            cmax = fmaxf(fmaxf(cmax, r.x), fmaxf(fmaxf(r.y, r.z), r.w));
        }
    }
    if (amax) {                              // outputs are >= 0 (or NaN, which fmaxf drops): float bits order like unsigned
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cmax = fmaxf(cmax, __shfl_xor(cmax, o, 64));
        if ((threadIdx.x & 63) == 0 && cmax > 0.0f) atomicMax(amax, __float_as_uint(cmax));
    }
}

// dst = src * factor (the stage tap of a depthwise output in the f16 modes: factor = 2^-act_exp, exact)
__global__ __launch_bounds__(256) void scale_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n,
                                                         float factor) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) dst[i] = src[i] * factor;
}

// --------------------------------------------------------------------------- pointwise GEMM
// C[m][n] = relu(sum_k A[m][k] * Wt[n][k] + bias[n]).  A = NHWC activations flattened to
// [rows = windows*H*W][K = Cin]; Wt = folded kernel stored [Cout][Cin] so that both operands
// have K contiguous and one ds_read_b128 feeds four MFMA k-steps.
//
// Workgroup = WGM x WGN waves on a BM x BN tile, BK = 32 per LDS stage, register-staged double
// buffering: the global_load_dwordx4 of stage t+1 are issued before the MFMAs of stage t and
// written to the other LDS buffer after them, one barrier per stage.
// v_mfma_f32_32x32x2_f32 operand map: lane l supplies A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31]; which k a step covers is free as long as both operands agree, so
// lane-half h takes k = 8*s + 4*h + j for the j-th MFMA of super-step s (one b128 per operand).
// Rows past M are loaded from row M-1 (always in bounds) and never stored.
#ifndef BD_PW_ABLATE
#define BD_PW_ABLATE 0      // developer builds: 1 = no global loads in the loop, 2 = no fragment reads, 4 = no MFMAs, 8 = no stores
#endif
constexpr int kBK = 32;
constexpr int kLds = kBK + 4;   // row stride in floats: 144 B = odd multiple of 16 B -> conflict-free b128
// an operand fragment from LDS (developer build 2: a register value instead; by value, so that no address escapes)
typedef float pw4 __attribute__((ext_vector_type(4)));   // native vectors: SSA values, nothing for the compiler to keep in memory
// operand pointers that are re-pointed inside the tile loop: the address space is lost through the loop's phi nodes and the
// loads become flat_load (counted in lgkmcnt too: every LDS wait then waits for them) unless it is spelled out
typedef const __attribute__((address_space(1))) float* pw_gptr;
typedef const __attribute__((address_space(1))) pw4* pw_gptr4;
__device__ __forceinline__ pw4 pw_frag(const float* p, pw4 instead) {
    if (BD_PW_ABLATE & 2) return instead;
    return *reinterpret_cast<const pw4*>(p);
}

// With NH > 0 the kernel also applies the NEXT layer's depthwise 3x3 (stride NS, TF SAME padding) to its output, an NH x NW
// map per window: a 96-row tile is whole windows (one 12 x 8 map, four 6 x 4 maps or sixteen 3 x 2 maps), so the tile goes
// through LDS as f32 (bias + ReLU applied) and what reaches HBM - `C` - is the depthwise output [windows][NH / NS][NW / NS][N];
// the 1x1 output itself never exists.  depthwise_kernel's chain (shift, the taps in (kh, kw) order, zeros outside the map).
template <int BM, int BN, int WGM, int WGN, int NH = 0, int NW = 0, int NS = 1>
__global__ __launch_bounds__(WGM* WGN * 64, (NH > 0 ? 2 : 1)) void pointwise_kernel(const float* __restrict__ A,
                                                                  const float* __restrict__ Wt,
                                                                  const float* __restrict__ bias,
                                                                  float* __restrict__ C, long long M, int N,
                                                                  int K, int tiles_n, long long tiles, int xcd_map,
                                                                  const float* __restrict__ ndw_w,
                                                                  const float* __restrict__ ndw_b, int windows) {
    constexpr int NT = WGM * WGN * 64;
    constexpr bool NDW = NH > 0;
    static_assert(!NDW || (BM % (NH * NW) == 0 && BN == 128 && NT % 32 == 0), "whole windows per tile");
    constexpr int WM = BM / WGM, WN = BN / WGN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int RPP = NT / 8;                  // tile rows covered by one float4-per-thread pass
    constexpr int LA = BM / RPP, LB = BN / RPP;  // float4 global loads per thread per stage
    static_assert(BM % RPP == 0 && BN % RPP == 0 && WM % 32 == 0 && WN % 32 == 0, "tile shape");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;                      // [2][BM * kLds]
    float* const Bs = smem + 2 * BM * kLds;      // [2][BN * kLds]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave / WGN, wc = wave % WGN;
    const int lrow = tid >> 3;   // 0 .. RPP-1
    const int lc4 = tid & 7;     // float4 column within the 32-wide k slab
    const int st_off = lrow * kLds + lc4 * 4;
    const int frow = lane & 31;
    const int fk = (lane >> 5) * 4;
    const int half = lane >> 5;
    const float* const a_frag = As + (wr * WM + frow) * kLds + fk;
    const float* const b_frag = Bs + (wc * WN + frow) * kLds + fk;

    // Persistent workgroups walk tiles blockIdx.x, + gridDim.x, ... as ONE stream of K stages: the first stage of the next
    // tile is loaded behind the last product of this one, and this tile's stores drain behind the next tile's products (a
    // workgroup that ends on its stores holds its CU share until they retire: 14 of 124 us on a 512 -> 512 layer).
    // Tile order: the n-tiles of one m-tile are neighbours; with xcd_map (m-tiles a multiple of 8) they sit on ONE XCD
    // (workgroups go to the XCDs round-robin by ID and the grid is a multiple of 8), so the A rows they share come from one L2.
#define BD_PW_ORIGIN(T_, M0_, N0_)                                                   \
    {                                                                                \
        long long tile_m_;                                                           \
        int tile_n_;                                                                 \
        if (xcd_map) {                                                               \
            const long long idx_ = (T_) >> 3;                                        \
            tile_n_ = (int)(idx_ % tiles_n);                                         \
            tile_m_ = (idx_ / tiles_n) * 8 + ((T_) & 7);                             \
        } else {                                                                     \
            tile_m_ = (T_) / tiles_n;                                                \
            tile_n_ = (int)((T_) % tiles_n);                                         \
        }                                                                            \
        M0_ = tile_m_ * BM;                                                          \
        N0_ = tile_n_ * BN;                                                          \
    }
    // rows past M are loaded from row M-1 (always in bounds) and never stored
#define BD_PW_POINT(M0_, N0_)                                                        \
    {                                                                                \
        _Pragma("unroll") for (int i = 0; i < LA; ++i) {                             \
            long long m_ = (M0_) + lrow + RPP * i;                                   \
            m_ = m_ < M ? m_ : M - 1;                                                \
            ap[i] = (pw_gptr)A + (size_t)m_ * K + lc4 * 4;                           \
        }                                                                            \
        _Pragma("unroll") for (int i = 0; i < LB; ++i) bp[i] = (pw_gptr)Wt + (size_t)((N0_) + lrow + RPP * i) * K + lc4 * 4; \
    }
    pw_gptr ap[LA];
    pw_gptr bp[LB];

    long long t = blockIdx.x;
    if (t >= tiles) return;
    long long m0;
    int n0;
    BD_PW_ORIGIN(t, m0, n0)
    BD_PW_POINT(m0, n0)

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    pw4 ra[LA], rb[LB];
#pragma unroll
    for (int i = 0; i < LA; ++i) ra[i] = *(pw_gptr4)(ap[i]);
#pragma unroll
    for (int i = 0; i < LB; ++i) rb[i] = *(pw_gptr4)(bp[i]);
#pragma unroll
    for (int i = 0; i < LA; ++i) *reinterpret_cast<pw4*>(As + st_off + RPP * i * kLds) = ra[i];
#pragma unroll
    for (int i = 0; i < LB; ++i) *reinterpret_cast<pw4*>(Bs + st_off + RPP * i * kLds) = rb[i];
    __syncthreads();

#define BD_PW_COMPUTE(BUF)                                                                              \
    {                                                                                                   \
        const float* as_ = a_frag + (BUF) * BM * kLds;                                                  \
        const float* bs_ = b_frag + (BUF) * BN * kLds;                                                  \
        _Pragma("unroll") for (int s = 0; s < kBK / 8; ++s) {                                           \
            pw4 av[TM], bv[TN];                                                                      \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) av[i] = pw_frag(as_ + i * 32 * kLds + s * 8, ra[0]); \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) bv[j] = pw_frag(bs_ + j * 32 * kLds + s * 8, rb[0]); \
            if (BD_PW_ABLATE & 4) {                                                                     \
                _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j) \
                    acc[i][j][s] += av[i].x * bv[j].y;                                                  \
            } else                                                                                      \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j) { \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].x, bv[j].x, acc[i][j], 0, 0, 0); \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].y, bv[j].y, acc[i][j], 0, 0, 0); \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].z, bv[j].z, acc[i][j], 0, 0, 0); \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].w, bv[j].w, acc[i][j], 0, 0, 0); \
            }                                                                                           \
        }                                                                                               \
    }

    const int nk = K / kBK;
    int buf = 0;
    for (;;) {
        const long long tn = t + gridDim.x;
        const bool more = tn < tiles;
        long long nm0 = 0;
        int nn0 = 0;
        for (int kt = 0; kt < nk; ++kt) {
            const bool last = kt + 1 == nk;
            const bool feed = !last || more;     // a stage follows this one: load it now, store it to LDS after the product
            int koff = (kt + 1) * kBK;
            if (last) {                          // ... the first stage of the next tile
                koff = 0;
                if (more) {
                    BD_PW_ORIGIN(tn, nm0, nn0)
                    BD_PW_POINT(nm0, nn0)
                }
            }
            // unconditional (the very last stage of a workgroup re-reads its tile's first stage and drops it): loads under a
            // branch make the compiler wait for them at the join, in FRONT of the product they are meant to hide behind
            if (!(BD_PW_ABLATE & 1)) {
#pragma unroll
                for (int i = 0; i < LA; ++i) ra[i] = *(pw_gptr4)(ap[i] + koff);
#pragma unroll
                for (int i = 0; i < LB; ++i) rb[i] = *(pw_gptr4)(bp[i] + koff);
            }
            asm volatile("" ::: "memory");       // keeps the loads HERE: their only use is under `feed`, and the compiler sinks them there
            BD_PW_COMPUTE(buf)
            if (feed && !(NDW && last)) {        // (with the depthwise epilogue the tile passes through these buffers first)
                float* an = As + (buf ^ 1) * BM * kLds + st_off;
                float* bn = Bs + (buf ^ 1) * BN * kLds + st_off;
#pragma unroll
                for (int i = 0; i < LA; ++i) *reinterpret_cast<pw4*>(an + RPP * i * kLds) = ra[i];
#pragma unroll
                for (int i = 0; i < LB; ++i) *reinterpret_cast<pw4*>(bn + RPP * i * kLds) = rb[i];
                __syncthreads();
            }
            buf ^= 1;
        }
        if constexpr (NDW) {
            constexpr int PWN = NH * NW, WPT = BM / PWN;         // positions per window, windows per tile
            constexpr int OH = NH / (NS ? NS : 1), OW = NW / (NS ? NS : 1), OPW = OH * OW;
            constexpr int PAD = NS == 1 ? 1 : 0;
            constexpr int PS = BN + 4;                           // row stride of the f32 tile
            constexpr int TASKS = WPT * OPW * (BN / 4);
            float* const P = smem;                               // [BM + 1][PS], over the stage buffers
            const int c4 = tid & (BN / 4 - 1);                   // this thread's channel quad (NT is a multiple of 32)
            pw4 tw[9];
            pw4 tb = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 9; ++k) tw[k] = *(pw_gptr4)((pw_gptr)ndw_w + (size_t)k * N + n0 + c4 * 4);
            tb = *(pw_gptr4)((pw_gptr)ndw_b + n0 + c4 * 4);
            __syncthreads();                                     // every wave has read its last fragments
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float b = bias[n0 + wc * WN + j * 32 + frow];
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        P[(wr * WM + i * 32 + 4 * half + (r & 3) + 8 * (r >> 2)) * PS + wc * WN + j * 32 + frow] = fmaxf(acc[i][j][r] + b, 0.0f);
                        acc[i][j][r] = 0.0f;
                    }
            }
            if (tid < BN / 4) *reinterpret_cast<pw4*>(P + BM * PS + tid * 4) = pw4{0.0f, 0.0f, 0.0f, 0.0f};   // what a tap outside the map reads
            __syncthreads();
            const long long win0 = m0 / PWN;
            const bool whole = win0 + WPT <= windows;            // (stores under a branch each wait for the one before)
            if constexpr (NS == 1) {
                // stride 1: a thread owns a COLUMN of a window's map (and a channel quad) and walks the input rows once - each row
                // is tap row 0 of the output below it, 1 of its own, 2 of the one above - so an output's chain still runs
                // in (kh, kw) order, with 3 NH LDS reads per NH outputs instead of 9 NH
                constexpr int ITEMS = WPT * NW * (BN / 4);
                static_assert(ITEMS % NT == 0, "whole rounds of column items");
#pragma unroll 1
                for (int u = 0; u < ITEMS / NT; ++u) {
                    const int q = (tid + NT * u) / (BN / 4);
                    const int col = q % NW, w = q / NW;
                    pw4 o[NH];
#pragma unroll
                    for (int r = 0; r < NH; ++r) o[r] = tb;
#pragma unroll
                    for (int r = -1; r <= NH; ++r) {
                        pw4 v[3];
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) {
                            const int cc = col - 1 + kw;
                            const bool ok = r >= 0 && r < NH && cc >= 0 && cc < NW;
                            v[kw] = *reinterpret_cast<const pw4*>(P + (ok ? w * PWN + r * NW + cc : BM) * PS + c4 * 4);    // row BM: zeros
                        }
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) {
                            if (r + 1 < NH) o[r + 1 < NH ? r + 1 : 0] = __builtin_elementwise_fma(v[kw], tw[kw], o[r + 1 < NH ? r + 1 : 0]);
                        }
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) {
                            if (r >= 0 && r < NH) o[r >= 0 && r < NH ? r : 0] = __builtin_elementwise_fma(v[kw], tw[3 + kw], o[r >= 0 && r < NH ? r : 0]);
                        }
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) {
                            if (r >= 1) o[r >= 1 ? r - 1 : 0] = __builtin_elementwise_fma(v[kw], tw[6 + kw], o[r >= 1 ? r - 1 : 0]);
                        }
                    }
                    if (whole || win0 + w < windows) {
                        float* const dst = C + (((size_t)(win0 + w) * OH) * OW + col) * N + n0 + c4 * 4;
#pragma unroll
                        for (int r = 0; r < NH; ++r) {
                            pw4 a = o[r];
                            a.x = fmaxf(a.x, 0.0f);
                            a.y = fmaxf(a.y, 0.0f);
                            a.z = fmaxf(a.z, 0.0f);
                            a.w = fmaxf(a.w, 0.0f);
                            *reinterpret_cast<pw4*>(dst + (size_t)r * OW * N) = a;
                        }
                    }
                }
            } else {
#pragma unroll 3
                for (int u = 0; u < (TASKS + NT - 1) / NT; ++u) {
                    const int idx = tid + NT * u;
                    const int pos = idx / (BN / 4);
                    const int w = pos / OPW, o = pos % OPW, oh = o / OW, ow = o % OW;
                    pw4 a = tb;
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) {
                            const int ih = oh * NS + kh - PAD, iw = ow * NS + kw - PAD;
                            const bool ok = ih >= 0 && ih < NH && iw >= 0 && iw < NW && (TASKS % NT == 0 || idx < TASKS);
                            const pw4 v = *reinterpret_cast<const pw4*>(P + (ok ? (w * PWN + ih * NW + iw) : BM) * PS + c4 * 4);   // row BM: zeros
                            a = __builtin_elementwise_fma(v, tw[kh * 3 + kw], a);
                        }
                    a.x = fmaxf(a.x, 0.0f);
                    a.y = fmaxf(a.y, 0.0f);
                    a.z = fmaxf(a.z, 0.0f);
                    a.w = fmaxf(a.w, 0.0f);
                    float* const dst = C + (((size_t)(win0 + w) * OH + oh) * OW + ow) * N + n0 + c4 * 4;
                    if (whole && TASKS % NT == 0) *reinterpret_cast<pw4*>(dst) = a;
                    else if ((TASKS % NT == 0 || idx < TASKS) && win0 + w < windows) *reinterpret_cast<pw4*>(dst) = a;
                }
            }
            if (more) {                                          // the next tile's first stage, held in registers since the last product
                __syncthreads();                                 // the tile has been read
                float* an = As + buf * BM * kLds + st_off;
                float* bn = Bs + buf * BN * kLds + st_off;
#pragma unroll
                for (int i = 0; i < LA; ++i) *reinterpret_cast<pw4*>(an + RPP * i * kLds) = ra[i];
#pragma unroll
                for (int i = 0; i < LB; ++i) *reinterpret_cast<pw4*>(bn + RPP * i * kLds) = rb[i];
                __syncthreads();
            }
        } else {
        // epilogue: C/D map of the 32x32 tile: col = lane & 31, row = (r & 3) + 8*(r >> 2) + 4*(lane >> 5).  A tile inside
            // M stores without a branch per row: under a branch each store gets its own s_waitcnt vmcnt(0) (for the bias load),
            // which on gfx9 also waits for the store before it - sixteen memory round trips in a row per 32 x 32 tile.
            const bool whole = m0 + BM <= M;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wc * WN + j * 32 + frow;
                const float b = bias[n];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const long long mb = m0 + wr * WM + i * 32 + 4 * half;
                    float* const crow = C + (size_t)mb * N + n;
                    if (whole && !(BD_PW_ABLATE & 8)) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) crow[(size_t)((r & 3) + 8 * (r >> 2)) * N] = fmaxf(acc[i][j][r] + b, 0.0f);
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const long long m = mb + (r & 3) + 8 * (r >> 2);
                            if (m < M && (!(BD_PW_ABLATE & 8) || acc[i][j][r] == 12345.678f)) C[(size_t)m * N + n] = fmaxf(acc[i][j][r] + b, 0.0f);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
                }
            }
        }
        if (!more) break;
        t = tn;
        m0 = nm0;
        n0 = nn0;
    }
#undef BD_PW_COMPUTE
#undef BD_PW_ORIGIN
#undef BD_PW_POINT
}

// --------------------------------------------------------------------------- pointwise GEMM, split-f16
// Same contraction on the f16 matrix cores (v_mfma_f32_32x32x16_f16, 16x the f32-MFMA rate) without
// giving up f32 accuracy: every f32 operand x is carried as two halves x = hi + lo with
// hi = f16(x), lo = f16(x - hi)  (22 significand bits), and
//     a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi      (the dropped a_lo*b_lo term is ~2^-22 relative)
// Products of two f16 are exact in f32 and the MFMA accumulates in f32, so the result differs from the
// f32 chain by ~1e-7 relative — measured on the whole network: same max |dlogit| vs the f64 oracle as
// the exact-f32 kernel.  Weights are split once on the host; activations are split while they are staged
// from HBM into LDS.
//
//
// LDS tiles are [rows][32 f16], swizzled by swz64 (bd_device.h).  Operand map of v_mfma_f32_32x32x16_f16: lane l supplies
// A[row l & 31][k = 8*(l >> 5) + j] and B[k = 8*(l >> 5) + j][col l & 31], j = 0..7.

// Epilogue of a 32x32 tile accumulated TRANSPOSED (weights fed as the MFMA "A" operand, activations as
// "B"): lane l then owns output row m = l & 31 and, per register quad g, the four consecutive channels
// n = 8 g + 4 (l >> 5) + 0..3 - one 16-byte store per quad instead of four 4-byte ones.  Products and
// their k order are those of the untransposed form.
__device__ __forceinline__ void store_tile_t(const f32x16& acc, const float* __restrict__ unscale_n,
                                             const float* __restrict__ bias_n, float* crow, bool live, int half) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 b = *reinterpret_cast<const float4*>(bias_n + 8 * g + 4 * half);
        const float4 u = *reinterpret_cast<const float4*>(unscale_n + 8 * g + 4 * half);
        float4 v;
        v.x = fmaxf(fmaf(acc[4 * g + 0], u.x, b.x), 0.0f);
        v.y = fmaxf(fmaf(acc[4 * g + 1], u.y, b.y), 0.0f);
        v.z = fmaxf(fmaf(acc[4 * g + 2], u.z, b.z), 0.0f);
        v.w = fmaxf(fmaf(acc[4 * g + 3], u.w, b.w), 0.0f);
        if (live) *reinterpret_cast<float4*>(crow + 8 * g + 4 * half) = v;
    }
}

template <int BM, int BN, int WGM, int WGN, bool PLAIN>
__global__ __launch_bounds__(WGM* WGN * 64) void pointwise_f16x3_kernel(
    const float* __restrict__ A, const _Float16* __restrict__ Whi, const _Float16* __restrict__ Wlo,
    const float* __restrict__ unscale, const float* __restrict__ bias, float* __restrict__ C, long long M, int N, int K,
    int tiles_n, unsigned* __restrict__ range_flag) {
    float rmax = 0.0f;
    constexpr int NT = WGM * WGN * 64;
    constexpr int WM = BM / WGM, WN = BN / WGN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int RPP = NT / 8;
    constexpr int LA = BM / RPP;            // float4 loads of A per thread per stage
    constexpr int BCH = BN * 4 / NT;        // 16-byte chunks per thread per stage, for each of W_hi / W_lo
    static_assert(BM % RPP == 0 && (BN * 4) % NT == 0 && WM % 32 == 0 && WN % 32 == 0, "tile shape");
    constexpr int A_BYTES = BM * 64, B_BYTES = BN * 64;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* const Ah = smem_raw;                    // [2][A_BYTES]
    char* const Al = Ah + 2 * A_BYTES;
    char* const Bh = Al + 2 * A_BYTES;            // [2][B_BYTES]
    char* const Bl = Bh + 2 * B_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave / WGN, wc = wave % WGN;
    const long long tile_m = blockIdx.x / tiles_n;
    const int tile_n = blockIdx.x % tiles_n;
    const long long m0 = tile_m * BM;
    const int n0 = tile_n * BN;

    const int lrow = tid >> 3;
    const int lc4 = tid & 7;
    const float* ap[LA];
    int a_st[LA];
#pragma unroll
    for (int i = 0; i < LA; ++i) {
        long long m = m0 + lrow + RPP * i;
        m = m < M ? m : M - 1;
        ap[i] = A + (size_t)m * K + lc4 * 4;
        a_st[i] = swz64(lrow + RPP * i, lc4 >> 1) + (lc4 & 1) * 8;
    }
    const _Float16* bph[BCH];
    const _Float16* bpl[BCH];
    int b_st[BCH];
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
        const int id = tid + NT * i;
        const int row = id >> 2, slot = id & 3;
        bph[i] = Whi + (size_t)(n0 + row) * K + slot * 8;
        bpl[i] = Wlo + (size_t)(n0 + row) * K + slot * 8;
        b_st[i] = swz64(row, slot);
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    float4 ra[LA];
    uint4 rbh[BCH], rbl[BCH];

#define BD_F16_LOAD(KOFF)                                                                                \
    {                                                                                                    \
        _Pragma("unroll") for (int i = 0; i < LA; ++i) ra[i] = *reinterpret_cast<const float4*>(ap[i] + (KOFF)); \
        _Pragma("unroll") for (int i = 0; i < BCH; ++i) {                                                \
            rbh[i] = *reinterpret_cast<const uint4*>(bph[i] + (KOFF));                                   \
            rbl[i] = *reinterpret_cast<const uint4*>(bpl[i] + (KOFF));                                   \
        }                                                                                                \
    }
#define BD_F16_STORE(BUF)                                                                                \
    {                                                                                                    \
        _Pragma("unroll") for (int i = 0; i < LA; ++i) {                                                 \
            const float4 v = ra[i];                                                                      \
            rmax = range_of(rmax, v);                                                                    \
            f16x4 hi, lo;                                                                                \
            split_f16(v.x, v.y, v.z, v.w, hi, lo);                                                      \
            *reinterpret_cast<f16x4*>(Ah + (BUF) * A_BYTES + a_st[i]) = hi;                              \
            *reinterpret_cast<f16x4*>(Al + (BUF) * A_BYTES + a_st[i]) = lo;                              \
        }                                                                                                \
        _Pragma("unroll") for (int i = 0; i < BCH; ++i) {                                                \
            *reinterpret_cast<uint4*>(Bh + (BUF) * B_BYTES + b_st[i]) = rbh[i];                          \
            *reinterpret_cast<uint4*>(Bl + (BUF) * B_BYTES + b_st[i]) = rbl[i];                          \
        }                                                                                                \
    }

    const int frow = lane & 31;
    const int fh = lane >> 5;
#define BD_F16_COMPUTE(BUF)                                                                              \
    {                                                                                                    \
        _Pragma("unroll") for (int s = 0; s < 2; ++s) {                                                  \
            f16x8 ah[TM], al[TM], bh[TN], bl[TN];                                                        \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                             \
                const int off = (BUF) * A_BYTES + swz64(wr * WM + i * 32 + frow, 2 * s + fh);            \
                ah[i] = *reinterpret_cast<const f16x8*>(Ah + off);                                       \
                al[i] = *reinterpret_cast<const f16x8*>(Al + off);                                       \
            }                                                                                            \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                             \
                const int off = (BUF) * B_BYTES + swz64(wc * WN + j * 32 + frow, 2 * s + fh);            \
                bh[j] = *reinterpret_cast<const f16x8*>(Bh + off);                                       \
                bl[j] = *reinterpret_cast<const f16x8*>(Bl + off);                                       \
            }                                                                                            \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j) { \
                if constexpr (!PLAIN) {                                                                  \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[j], al[i], acc[i][j], 0, 0, 0); \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[j], ah[i], acc[i][j], 0, 0, 0); \
                }                                                                                        \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[j], ah[i], acc[i][j], 0, 0, 0);    \
            }                                                                                            \
        }                                                                                                \
    }

    BD_F16_LOAD(0)
    BD_F16_STORE(0)
    __syncthreads();
    const int nk = K / 32;
    for (int kt = 0; kt + 1 < nk; ++kt) {
        const int buf = kt & 1;
        BD_F16_LOAD((kt + 1) * 32)
        BD_F16_COMPUTE(buf)
        BD_F16_STORE(buf ^ 1)
        __syncthreads();
    }
    BD_F16_COMPUTE((nk - 1) & 1)
#undef BD_F16_LOAD
#undef BD_F16_STORE
#undef BD_F16_COMPUTE

    // transposed accumulators: lane owns row m0 + .. + (lane & 31), 16-byte stores (store_tile_t)
    const int half = lane >> 5;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const long long m = m0 + wr * WM + i * 32 + frow;
        float* crow = C + (size_t)(m < M ? m : 0) * N;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nb = n0 + wc * WN + j * 32;
            store_tile_t(acc[i][j], unscale + nb, bias + nb, crow + nb, m < M, half);
        }
    }
    range_report(rmax, range_flag);
}

template <int BM, int BN, int WGM, int WGN, bool PLAIN>
void launch_pw16_(const float* A, const _Float16* Whi, const _Float16* Wlo, const float* unscale, const float* bias, float* C,
                  long long M, int N, int K, unsigned* range_flag, hipStream_t stream) {
    constexpr int NT = WGM * WGN * 64;
    constexpr size_t lds = 2u * 2u * (BM + BN) * 64;
    allow_dynamic_lds<&pointwise_f16x3_kernel<BM, BN, WGM, WGN, PLAIN>>((int)lds);
    const int tiles_n = N / BN;
    const long long tiles = ((M + BM - 1) / BM) * tiles_n;
    hipLaunchKernelGGL((pointwise_f16x3_kernel<BM, BN, WGM, WGN, PLAIN>), dim3((unsigned)tiles), dim3(NT), lds, stream, A,
                       Whi, Wlo, unscale, bias, C, M, N, K, tiles_n, range_flag);
}

template <int BM, int BN, int WGM, int WGN>
void launch_pw16(const float* A, const _Float16* Whi, const _Float16* Wlo, const float* unscale, const float* bias, float* C,
                 long long M, int N, int K, bool plain, unsigned* range_flag, hipStream_t stream) {
    if (plain) launch_pw16_<BM, BN, WGM, WGN, true>(A, Whi, Wlo, unscale, bias, C, M, N, K, range_flag, stream);
    else launch_pw16_<BM, BN, WGM, WGN, false>(A, Whi, Wlo, unscale, bias, C, M, N, K, range_flag, stream);
}

template <int BM, int BN, int WGM, int WGN, int NH = 0, int NW = 0, int NS = 1>
void launch_pw(const float* A, const float* Wt, const float* bias, float* C, long long M, int N, int K,
               hipStream_t stream, const float* ndw_w = nullptr, const float* ndw_b = nullptr, int windows = 0) {
    constexpr int NT = WGM * WGN * 64;
    constexpr size_t lds = 2u * (BM + BN) * kLds * sizeof(float);
    static_assert(NH == 0 || lds >= (size_t)(BM + 1) * (BN + 4) * sizeof(float), "the f32 tile of the depthwise epilogue (+ a row of zeros) fits the stage buffers");
    allow_dynamic_lds<&pointwise_kernel<BM, BN, WGM, WGN, NH, NW, NS>>((int)lds);
    const int tiles_n = N / BN;
    const long long tiles_m = (M + BM - 1) / BM;
    const long long tiles = tiles_m * tiles_n;
    // persistent: as many workgroups as fit the chip at once (by LDS: 160 KB per CU; by waves: 8 per SIMD), a multiple of 8
    int per_cu = (int)(160 * 1024 / lds);
    if (per_cu > 2048 / NT) per_cu = 2048 / NT;
    if (per_cu < 1) per_cu = 1;
    long long grid = (long long)cu_count() * per_cu / 8 * 8;
    if (grid > tiles) grid = tiles;
    if (grid < 1) grid = 1;                   // (a device with fewer than 8 resident workgroups: never a zero-sized launch)
    const int xcd_map = tiles_m % 8 == 0 && grid % 8 == 0;
    hipLaunchKernelGGL((pointwise_kernel<BM, BN, WGM, WGN, NH, NW, NS>), dim3((unsigned)grid), dim3(NT), lds, stream, A, Wt,
                       bias, C, M, N, K, tiles_n, tiles, xcd_map, ndw_w, ndw_b, windows);
}

// --------------------------------------------------------------------------- pool + head
template <int POOL>   // 6: act = [window][6][1024] is pooled here; 1: act = [window][1024] is already the pooled embedding
__global__ __launch_bounds__(256) void pool_head_kernel(const float* __restrict__ act,
                                                        const float* __restrict__ head_wt,
                                                        const float* __restrict__ head_b, int n_classes,
                                                        float* __restrict__ emb, float* __restrict__ logits) {
    // one workgroup per window; act = [window][6][1024]
    __shared__ float s_part[4][BD_MAX_CLASSES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const size_t win = blockIdx.x;
    const float4* src = reinterpret_cast<const float4*>(act + win * POOL * BD_EMBEDDING_SIZE);
    float4 s = src[tid];
    if constexpr (POOL > 1) {
#pragma unroll
        for (int p = 1; p < POOL; ++p) {
            const float4 v = src[p * (BD_EMBEDDING_SIZE / 4) + tid];
            s.x += v.x;
            s.y += v.y;
            s.z += v.z;
            s.w += v.w;
        }
        s.x /= (float)POOL;
        s.y /= (float)POOL;
        s.z /= (float)POOL;
        s.w /= (float)POOL;
        if (emb) reinterpret_cast<float4*>(emb + win * BD_EMBEDDING_SIZE)[tid] = s;
    }
    if (!logits) return;

    // classes in groups of 16: all weight rows of a group are in flight together and the 16 butterflies are
    // independent (one class at a time was a chain of 13 dependent L2 round trips, 13 us for 4 MB of input)
    for (int c0 = 0; c0 < n_classes; c0 += 16) {
        float4 w[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = c0 + j < n_classes ? c0 + j : n_classes - 1;
            w[j] = reinterpret_cast<const float4*>(head_wt + (size_t)c * BD_EMBEDDING_SIZE)[tid];
        }
        float p[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) p[j] = fmaf(s.x, w[j].x, fmaf(s.y, w[j].y, fmaf(s.z, w[j].z, s.w * w[j].w)));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int j = 0; j < 16; ++j) p[j] += __shfl_xor(p[j], o, 64);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (lane == 0 && c0 + j < n_classes) s_part[wave][c0 + j] = p[j];
    }
    __syncthreads();
    if (tid < n_classes)
        logits[win * n_classes + tid] =
            ((s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid])) + head_b[tid];
}

}  // namespace

void launch_conv1(const float* logmel, int patch_step, const WindowMap& map, int w0, int windows, const float* w9x32,
                  const float* b32, float* out, hipStream_t stream) {
    if (windows <= 0) return;
    hipLaunchKernelGGL(conv1_kernel, dim3(48 / kC1Rows, windows), dim3(256), 0, stream, logmel, patch_step, map, w0,
                       w9x32, b32, out);
}

template <int STRIDE, int OWB>
static void launch_dw(const float* in, float* out, int windows, const SepLayer& L, hipStream_t stream) {
    const long long total = (long long)windows * L.h_out * (L.w_out / OWB) * (L.cin / 4);
    const long long blocks = (total + 255) / 256;
    const int grid = (int)(blocks < (1 << 20) ? blocks : (1 << 20));
    hipLaunchKernelGGL((depthwise_kernel<STRIDE, OWB>), dim3(grid), dim3(256), 0, stream, in, out, dw_w_of(L), dw_b_of(L),
                       windows, L.h_in, L.w_in, L.cin, L.h_out, L.w_out, L.amax);
}

void launch_scale_copy(const float* src, float* dst, int64_t n, float factor, hipStream_t stream) {
    if (n <= 0) return;
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(scale_copy_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, src, dst,
                       (long long)n, factor);
}

void launch_depthwise(const float* in, float* out, int windows, const SepLayer& L, hipStream_t stream) {
    if (windows <= 0) return;
    const bool wide = L.w_out % 4 == 0;
    if (L.stride == 1) {
        if (wide) launch_dw<1, 4>(in, out, windows, L, stream);
        else launch_dw<1, 2>(in, out, windows, L, stream);
    } else {
        if (wide) launch_dw<2, 4>(in, out, windows, L, stream);
        else launch_dw<2, 2>(in, out, windows, L, stream);
    }
}

// variant: 0 = pick by shape; otherwise an explicit tile (test / tuning hook)
int launch_pointwise_variant(const float* A, const float* Wt, const float* bias, float* C, long long M, int N,
                             int K, int variant, hipStream_t stream) {
    if (M <= 0) return 0;
    if (K % kBK != 0 || N % 64 != 0) return -1;
    if (variant == 0) {
        // tools/gemm_sweep.py 1024 ... f32 on MI355X (round 4, persistent kernel): the first tile of the shape's list that
        // gives every CU a tile; 64 x 64 tiles for small batches
        struct Opt { int variant, bm, bn; };
        static const Opt n64[] = {{8, 64, 64}};
        static const Opt n128_k64[] = {{1, 128, 128}, {8, 64, 64}};
        static const Opt n128[] = {{9, 96, 128}, {8, 64, 64}};
        static const Opt n256[] = {{7, 128, 256}, {9, 96, 128}, {8, 64, 64}};
        static const Opt wide[] = {{9, 96, 128}, {8, 64, 64}};
        const Opt* list = wide;
        int count = 2;
        if (N == 64) { list = n64; count = 1; }
        else if (N == 128 && K <= 64) { list = n128_k64; count = 2; }
        else if (N == 128) { list = n128; count = 2; }
        else if (N == 256) { list = n256; count = 3; }
        variant = 8;
        for (int i = 0; i < count; ++i) {
            if (N % list[i].bn) continue;
            const long long tiles = ((M + list[i].bm - 1) / list[i].bm) * (N / list[i].bn);
            if (tiles >= 256 || i == count - 1) { variant = list[i].variant; break; }
        }
    }
    switch (variant) {
        case 1: if (N % 128) return -1; launch_pw<128, 128, 2, 2>(A, Wt, bias, C, M, N, K, stream); break;
        case 2: launch_pw<128, 64, 2, 2>(A, Wt, bias, C, M, N, K, stream); break;
        case 3: if (N % 128) return -1; launch_pw<256, 128, 4, 2>(A, Wt, bias, C, M, N, K, stream); break;
        case 4: if (N % 128) return -1; launch_pw<192, 128, 2, 2>(A, Wt, bias, C, M, N, K, stream); break;
        case 5: launch_pw<256, 64, 4, 1>(A, Wt, bias, C, M, N, K, stream); break;
        case 6: if (N % 128) return -1; launch_pw<64, 128, 1, 4>(A, Wt, bias, C, M, N, K, stream); break;
        case 7: if (N % 256) return -1; launch_pw<128, 256, 2, 4>(A, Wt, bias, C, M, N, K, stream); break;
        case 8: launch_pw<64, 64, 2, 2>(A, Wt, bias, C, M, N, K, stream); break;
        case 9: if (N % 128) return -1; launch_pw<96, 128, 1, 4>(A, Wt, bias, C, M, N, K, stream); break;
        case 10: launch_pw<96, 64, 1, 2>(A, Wt, bias, C, M, N, K, stream); break;
        default: return -1;
    }
    return 0;
}

// Exact-f32 1x1 convolution of layer L with the depthwise of the NEXT layer applied in the kernel's epilogue (96 x 128 tiles of
// whole windows): in = L's depthwise output [windows][h][w][cin], out = the next layer's depthwise output.  false = shape not
// covered (the caller runs the two kernels).
bool launch_pointwise_next_dw_f32(const float* in, float* out, int windows, const SepLayer& L, const SepLayer& Ln,
                                  hipStream_t stream) {
    if (windows <= 0) return true;
    if (L.cout % 128 != 0 || L.cin % kBK != 0 || Ln.cin != L.cout || Ln.h_in != L.h_out || Ln.w_in != L.w_out) return false;
    const long long M = (long long)windows * L.h_out * L.w_out;
    const int h = L.h_out, w = L.w_out, st = Ln.stride;
#define BD_NDW_CASE(H_, W_, S_)                                                                                         \
    if (h == H_ && w == W_ && st == S_) {                                                                               \
        launch_pw<96, 128, 1, 4, H_, W_, S_>(in, L.pw_wt, L.pw_b, out, M, L.cout, L.cin, stream, Ln.dw_w, Ln.dw_b, windows); \
        return true;                                                                                                    \
    }
    BD_NDW_CASE(12, 8, 1)
    BD_NDW_CASE(12, 8, 2)
    BD_NDW_CASE(6, 4, 1)
    BD_NDW_CASE(6, 4, 2)
#undef BD_NDW_CASE
    return false;
}

// Tile choice for the split-f16 kernel, from tools/gemm_sweep.py on MI355X at 1024 windows; when the
// batch is too small to give every CU a tile of the preferred shape, fall back to smaller tiles.
static int pick_f16x3_variant(long long M, int N, int K) {
    struct Opt { int variant, bm, bn; };
    static const Opt big_k[] = {{9, 256, 256}, {7, 128, 256}, {6, 64, 128}, {8, 64, 64}};     // K >= 256, N >= 512
    static const Opt mid[] = {{7, 128, 256}, {1, 128, 128}, {6, 64, 128}, {8, 64, 64}};        // N == 256
    static const Opt n128[] = {{3, 256, 128}, {1, 128, 128}, {6, 64, 128}, {8, 64, 64}};       // N == 128
    static const Opt n64[] = {{2, 128, 64}, {8, 64, 64}};                                       // N == 64
    static const Opt deep[] = {{2, 128, 64}, {6, 64, 128}, {8, 64, 64}};                        // N == 1024
    const Opt* list;
    int count;
    if (N == 64) { list = n64; count = 2; }
    else if (N == 128) { list = n128; count = 4; }
    else if (N == 256) { list = mid; count = 4; }
    else if (N >= 1024) { list = deep; count = 3; }
    else { list = big_k; count = 4; }
    for (int i = 0; i < count; ++i) {
        if (N % list[i].bn) continue;
        const long long tiles = ((M + list[i].bm - 1) / list[i].bm) * (N / list[i].bn);
        if (tiles >= 256 || i == count - 1) return list[i].variant;
    }
    (void)K;
    return 8;
}

int launch_pointwise_f16x3_variant(const float* A, const void* Whi, const void* Wlo, const float* unscale, const float* bias,
                                   float* C, long long M, int N, int K, int variant, hipStream_t stream, bool plain,
                                   unsigned* range_flag) {
    if (M <= 0) return 0;
    if (K % 32 != 0 || N % 64 != 0) return -1;
    const _Float16* wh = static_cast<const _Float16*>(Whi);
    const _Float16* wl = static_cast<const _Float16*>(Wlo);
    if (variant == 0) variant = pick_f16x3_variant(M, N, K);
    switch (variant) {
        case 1: if (N % 128) return -1; launch_pw16<128, 128, 2, 2>(A, wh, wl, unscale, bias, C, M, N, K, plain, range_flag, stream); break;
        case 2: launch_pw16<128, 64, 2, 2>(A, wh, wl, unscale, bias, C, M, N, K, plain, range_flag, stream); break;
        case 3: if (N % 128) return -1; launch_pw16<256, 128, 4, 2>(A, wh, wl, unscale, bias, C, M, N, K, plain, range_flag, stream); break;
        case 4: if (N % 256) return -1; launch_pw16<128, 256, 2, 2>(A, wh, wl, unscale, bias, C, M, N, K, plain, range_flag, stream); break;
        case 5: launch_pw16<256, 64, 4, 1>(A, wh, wl, unscale, bias, C, M, N, K, plain, range_flag, stream); break;
        case 6: if (N % 128) return -1; launch_pw16<64, 128, 1, 4>(A, wh, wl, unscale, bias, C, M, N, K, plain, range_flag, stream); break;
        case 7: if (N % 256) return -1; launch_pw16<128, 256, 2, 4>(A, wh, wl, unscale, bias, C, M, N, K, plain, range_flag, stream); break;
        case 8: launch_pw16<64, 64, 2, 2>(A, wh, wl, unscale, bias, C, M, N, K, plain, range_flag, stream); break;
        case 9: if (N % 256) return -1; launch_pw16<256, 256, 4, 2>(A, wh, wl, unscale, bias, C, M, N, K, plain, range_flag, stream); break;
        default: return -1;
    }
    return 0;
}

// Pointwise 1x1 convolution on the wave-specialised kernel: the producers only split the input rows into
// f16 hi + lo (no depthwise).  For the stride-2 layers, whose depthwise runs as its own kernel or in the
// previous layer's epilogue.  Same products in the same order as pointwise_f16x3_kernel: bit-identical.
bool launch_pointwise_ws(const float* in, float* out, int64_t rows, const SepLayer& L, hipStream_t stream) {
    if (rows <= 0 || rows >= (1LL << 31) || L.cin < 128 || L.cin % 64 != 0 || L.cout % 256 != 0) return false;
    // layers 5 and 7: few enough input channels for the weights to live in registers (variant 10 keeps the tile kernel)
    if (L.pw_variant16 != 10 && (L.cin == 128 || L.cin == 256) && L.cout <= 2048) {
        launch_pointwise_res(in, out, (int)rows, L, stream);
        return true;
    }
    // (96 x 128 tiles with two workgroups per CU measured the same: 33.1 vs 32.6 us on layer 7)
    launch_pointwise_sep_ws(in, out, rows, L, stream);
    return true;
}

void launch_pointwise(const float* in, float* out, int64_t rows, const SepLayer& L, hipStream_t stream) {
    const bool f16 = L.pw_mode == 1 || L.pw_mode == 2;
    if (f16 && (L.pw_variant16 == 0 || L.pw_variant16 >= 10) && launch_pointwise_ws(in, out, rows, L, stream)) return;
    if (f16)
        launch_pointwise_f16x3_variant(in, L.pw_whi, L.pw_wlo, L.pw_u, L.pw_b, out, rows, L.cout, L.cin, L.pw_variant16,
                                       stream, L.pw_mode == 2, L.range_flag);
    else
        launch_pointwise_variant(in, L.pw_wt, L.pw_b, out, rows, L.cout, L.cin, L.pw_variant, stream);
}

// Fused depthwise+pointwise of layer L followed by the stride-2 depthwise of the NEXT layer; `out` receives
// that depthwise's output [windows][H/2][W/2][L.cout].  Layer 4 + depthwise 5 a window per workgroup (l4window.hip), else
// whole-window tiles of the 12x8 and 6x4 maps (sepws.hip).
bool launch_separable_fused_next_dw(const float* in, float* out, int windows, const SepLayer& L, const SepLayer& next,
                                    hipStream_t stream) {
    return launch_l4_window_next_dw(in, out, windows, L, next, stream) || launch_sep_ws_next_dw(in, out, windows, L, next, stream);
}

void launch_pool_head(const float* act, int windows, const float* head_wt, const float* head_b,
                      int n_classes, float* emb, float* logits, hipStream_t stream) {
    if (windows <= 0) return;
    hipLaunchKernelGGL(pool_head_kernel<6>, dim3(windows), dim3(256), 0, stream, act, head_wt, head_b,
                       n_classes, emb, logits);
}

// Dense head on embeddings that are already pooled: pooled = [windows][1024].
void launch_head(const float* pooled, int windows, const float* head_wt, const float* head_b, int n_classes,
                 float* logits, hipStream_t stream) {
    if (windows <= 0 || !logits) return;
    hipLaunchKernelGGL(pool_head_kernel<1>, dim3(windows), dim3(256), 0, stream, pooled, head_wt, head_b,
                       n_classes, static_cast<float*>(nullptr), logits);
}

}  // namespace bd
