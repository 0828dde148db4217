// The wave-specialised kernels of the one-kernel-per-layer path (bd_set_fusion separable = 7 / 10, and the 1x1 convolutions
// launch_pointwise_ws hands over), split-f16 and plain-f16 modes:
//   sep_ws_kernel   96 x 256 tiles, 4 producer + 4 MFMA waves, slab ring by LDS-DMA: NDW = 1 = layer 6 + depthwise 7; PWO = a
//                   plain 1x1 convolution of a wide layer
//   pw_res_kernel   the 1x1 convolutions of layers 5 and 7: persistent, weights in registers
// Same products in the same order as depthwise_kernel / pointwise_f16x3_kernel (cnn.hip): bit-identical.  Workgroup -> tile
// mapping is XCD-aware (tile_of).
#include "bd_device.h"

namespace bd {

namespace {

// Workgroup (or persistent tile index) -> (row tile, column tile).  Workgroups go to the 8 XCDs round-robin by ID
// (measured: FETCH_SIZE of a K = N = 512 layer is 53.5 MiB per launch when its two column tiles are IDs b, b+1 /
// b+2 / b+4 apart and 32.6 MiB when they are 8, 16, 32 or 64 apart), each XCD has its own L2, and the column tiles
// of one row tile read the same input slab.  IDs b and b + 8 - same XCD, dispatched together - are therefore made
// the column tiles of one row tile, so the second read of the slab is an L2 hit instead of an HBM fetch.
__device__ __forceinline__ void tile_of(unsigned b, unsigned tiles_m, unsigned tn, unsigned& tile_m, unsigned& tile_n) {
    const unsigned full = tiles_m & ~7u;                         // row tiles covered by whole groups of 8
    if (tn > 1 && b < full * tn) {
        tile_n = (b >> 3) % tn;
        tile_m = (b / (8 * tn)) * 8 + (b & 7);
    } else {
        const unsigned r = tn > 1 ? b - full * tn : b;
        tile_m = (tn > 1 ? full : 0) + r / tn;
        tile_n = r % tn;
    }
}

// --------------------------------------------------------------------------- wave-specialised 96 x 256 tile kernel
// Round 1-2's fused separable kernel, reduced in round 6 to the two forms the tree still runs (every option of its tuning
// history - weights staged through LDS, register-staged slabs, 64-channel stages, 64-row tiles, band tiles, the pool
// epilogue, the clock trace - is in git history and DESIGN_HISTORY.md 4.3 / 4.4):
//   PWO = 1           pointwise only (the 1 x 1 convolution of a layer whose depthwise has been applied elsewhere): the default
//                     path's pointwise 13, and the wide layers of the one-kernel-per-op path
//   NDW = 1           depthwise inside the GEMM + the NEXT layer's stride-2 depthwise in the epilogue (layer 6 + depthwise 7
//                     behind bd_set_fusion separable = 7 / 10; whole windows per tile)
// A workgroup is 8 waves; waves 4-7 are PRODUCERS (the f32 input slab arrives by LDS-DMA into a ring of three, they run
// the depthwise on the VALU - or just split the slab - and write the split-f16 A tile of stage k + 1) and waves 0-3 are
// CONSUMERS (weight fragments straight from the fragment-ordered copy into registers, one stage ahead; the MFMAs of
// stage k).  Waves w and w + 4 share a SIMD; one barrier per 32-channel stage.  BM = 96 output positions (3 MFMA row
// tiles: 4 / 1 / 16 whole windows of the 6 x 4 / 12 x 8 / 3 x 2 maps), BN = 256 output channels.  Arithmetic order is that
// of the unfused kernels: bit-identical.
template <int NDW, int PWO, bool PLAIN>
__global__ __launch_bounds__(512, 2) void sep_ws_kernel(
    const float* __restrict__ X, const float* __restrict__ dw_w, const float* __restrict__ dw_b,
    const _Float16* __restrict__ Whi, const _Float16* __restrict__ Wlo, const float* __restrict__ pw_u,
    const float* __restrict__ pw_b,
    float* __restrict__ Cout, long long M, int N, int K, int H, int W, int tiles_n,
    const float* __restrict__ ndw_w, const float* __restrict__ ndw_b, float* __restrict__ out2,
    unsigned* __restrict__ range_flag) {
    float rmax = 0.0f;                        // largest |activation| this thread has split into f16 halves (producers)
    static_assert((NDW == 0 || NDW == 1) && (PWO == 0 || NDW == 0), "pointwise only, or a fused layer with the next depthwise");
    constexpr int BN = 256, XPMAX = 96, BM = 96;
    constexpr int NX = 3;                    // slab buffers: a ring of three, filled by DMA
    constexpr int WN = BN / 4;               // consumer wave tile: BM x WN
    constexpr int TM = BM / 32, TN = WN / 32;
    constexpr int LA = BM / 32;              // depthwise outputs (x4 channels) per producer thread per stage
    constexpr int XS_FLOATS = (XPMAX + 1) * 32;   // + the zero row
    constexpr int A_BYTES = BM * 64;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* const Xs = reinterpret_cast<float*>(smem_raw);             // [3][XS_FLOATS]
    char* const Ah = reinterpret_cast<char*>(Xs + NX * XS_FLOATS);     // [2][A_BYTES]
    char* const Al = Ah + 2 * A_BYTES;
    float* const Wall = reinterpret_cast<float*>(Al + 2 * A_BYTES);    // [10][K] depthwise taps + shift of all K channels

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned tile_m, tile_n;
    tile_of(blockIdx.x, (unsigned)((M + BM - 1) / BM), (unsigned)tiles_n, tile_m, tile_n);
    const long long m0 = (long long)tile_m * BM;
    const int n0 = (int)tile_n * BN;
    const int nk = K / 32;                    // stages; >= 4 (launcher)

    // input slab of this tile: rows [x_lo, x_lo + x_cnt) of X (whole windows, or a band of rows plus its halo rows)
    const int P = H * W;
    long long x_lo;
    int x_cnt;
    if (PWO || P < BM) {                      // no depthwise, or whole windows: the slab is the tile's own rows
        x_lo = m0;
        x_cnt = (int)((M - m0) < BM ? (M - m0) : BM);
    } else {
        // (32-bit arithmetic: the launcher guarantees M < 2^31, and 64-bit division is a ~1000-cycle routine)
        const unsigned m0u = (unsigned)m0;
        const long long n = m0u / (unsigned)P;
        const int oh_a = (int)(m0u % (unsigned)P) / W;
        const int oh_b = oh_a + BM / W;
        const int r0 = oh_a > 0 ? oh_a - 1 : 0;
        const int r1 = oh_b < H ? oh_b + 1 : H;
        x_lo = (n * H + r0) * W;
        x_cnt = (r1 - r0) * W;
    }
    if (wave >= 4) {
        // ================================================================= producers
        const int pt = tid - 256;
        const int lrow = pt >> 3, lc4 = pt & 7;
        int xt[(LA + 2) * 3];
        int a_st[LA];
        {
            // a thread owns LA vertically adjacent outputs (same column, rows oh0 .. oh0+LA-1) of 4 channels: the
            // 3 x 3 neighbourhoods overlap, so it reads (LA+2) x 3 slab values instead of LA x 9
            // (W and the groups per window G = P / LA are powers of two - checked by the launcher - so this index
            //  arithmetic is shifts; as divisions it was a visible part of the ~1900-cycle table set-up)
            const int slot = lrow;
            const int lw = 31 - __builtin_clz(W);
            int wl = 0, g = slot;
            if (P < BM) {
                const int lg = 31 - __builtin_clz(P / LA);
                wl = slot >> lg;
                g = slot & ((1 << lg) - 1);
            }
            const int og = g >> lw, ow = g & (W - 1);
            const int ml0 = wl * P + LA * og * W + ow;
            const int oh0 = (P >= BM ? (int)((unsigned)m0 % (unsigned)P) / W : 0) + LA * og;
            const int xc0 = (int)(m0 + ml0 - x_lo);
#pragma unroll
            for (int r = 0; r < LA + 2; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int ih = oh0 - 1 + r, iw = ow - 1 + c;
                    const bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
                    xt[r * 3 + c] = (ok ? xc0 + (r - 1) * W + (c - 1) : XPMAX) * 32 + lc4 * 4;
                }
#pragma unroll
            for (int i = 0; i < LA; ++i) a_st[i] = swz64(ml0 + i * W, lc4 >> 1) + (lc4 & 1) * 8;
        }
        if (pt < 8 * NX) *reinterpret_cast<v4f*>(Xs + (pt >> 3) * XS_FLOATS + XPMAX * 32 + (pt & 7) * 4) = v4f{0.f, 0.f, 0.f, 0.f};

        int kch_ = 0;                         // first channel of the block the depthwise works on
        (void)kch_;
#define BD_P_DW(XB, AB)                                                                                   \
    {                                                                                                     \
        const float* xs_ = Xs + (XB) * XS_FLOATS;                                                         \
        const float* ws_ = Wall + kch_ + lc4 * 4;                                                         \
        v4f wt[9];                                                                                        \
        _Pragma("unroll") for (int t = 0; t < 9; ++t) wt[t] = *reinterpret_cast<const v4f*>(ws_ + t * K); \
        const v4f bias4 = *reinterpret_cast<const v4f*>(ws_ + 9 * K);                                     \
        v4f xv[(LA + 2) * 3];                                                                             \
        _Pragma("unroll") for (int t = 0; t < (LA + 2) * 3; ++t)                                          \
            xv[t] = *reinterpret_cast<const v4f*>(xs_ + xt[t]);                                           \
        _Pragma("unroll") for (int i = 0; i < LA; ++i) {                                                  \
            v4f a4 = bias4;                                                                               \
            _Pragma("unroll") for (int t = 0; t < 9; ++t)                                                 \
                a4 = __builtin_elementwise_fma(xv[i * 3 + t], wt[t], a4);   /* v_pk_fma_f32: two IEEE fmas per issue */ \
            a4.x = fmaxf(a4.x, 0.0f); a4.y = fmaxf(a4.y, 0.0f); a4.z = fmaxf(a4.z, 0.0f); a4.w = fmaxf(a4.w, 0.0f); \
            rmax = range_of(rmax, a4);                                                                    \
            f16x4 hi, lo;                                                                                 \
            split_f16(a4.x, a4.y, a4.z, a4.w, hi, lo);                                                  \
            *reinterpret_cast<f16x4*>(Ah + (AB) * A_BYTES + a_st[i]) = hi;                                \
            *reinterpret_cast<f16x4*>(Al + (AB) * A_BYTES + a_st[i]) = lo;                                \
        }                                                                                                 \
    }
        {
            // ---- slabs and taps by LDS-DMA into a ring of three, three stages ahead.  One global_load_lds_dwordx4
            // moves 8 slab rows (lane l -> row l >> 3, 16-byte chunk l & 7; LDS address = base + 16 l, exactly the
            // [row][32] layout); the 4 producer waves take the 8-row groups round-robin.  No VGPRs, no ds_write, and -
            // the point - the slab has two full stages to arrive: the barrier waits with a COUNTED vmcnt (everything but
            // the newest stage's DMA), where __syncthreads() would drain to 0 and expose the ~3000-cycle memory latency.
            // Producers issue no other vector-memory operation, so the count is exact.
            constexpr int NG = XPMAX / 8, GPW = NG / 4, ND = GPW;
            const int pw = wave - 4;
            // LDS-DMA is serialised on M0 (the LDS base): a DMA to a new base waits for the previous one to finish,
            // ~300 cycles each.  So a wave takes GPW CONSECUTIVE 8-row groups and reaches them through the
            // instruction's immediate offset, which is added to both addresses - the global pointer is biased
            // back by the same amount - and M0 is written once per stage.
            const float* xsrc[GPW];
#pragma unroll
            for (int q = 0; q < GPW; ++q) {
                int row = 8 * (GPW * pw + q) + (lane >> 3);
                row = row < x_cnt ? row : x_cnt - 1;
                xsrc[q] = X + (size_t)(x_lo + row) * K + (lane & 7) * 4 - 256 * q;
            }
#define BD_X_DMA1(Q, KOFF, XB)                                                                            \
    if constexpr ((Q) < GPW)                                                                              \
        __builtin_amdgcn_global_load_lds(                                                                 \
            (const __attribute__((address_space(1))) void*)(xsrc[(Q) < GPW ? (Q) : 0] + (KOFF)),          \
            (__attribute__((address_space(3))) void*)(Xs + (XB) * XS_FLOATS + GPW * pw * 256), 16, 1024 * (Q), 0);
#define BD_X_DMA(KOFF, XB)                                                                                \
    {                                                                                                     \
        BD_X_DMA1(0, KOFF, XB)                                                                            \
        BD_X_DMA1(1, KOFF, XB)                                                                            \
        BD_X_DMA1(2, KOFF, XB)                                                                            \
        BD_X_DMA1(3, KOFF, XB)                                                                            \
    }
#define BD_P_SYNC(KEEP)                                                                                   \
    {                                                                                                     \
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KEEP) : "memory");                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                \
        __builtin_amdgcn_s_barrier();                                                                     \
        asm volatile("" ::: "memory");                                                                    \
    }
            // PWO: the A tile is the slab itself, split into f16 hi + lo (rows lrow + 32 i, channels 4 lc4 ..)
#define BD_P_CVT(XB, AB)                                                                                  \
    _Pragma("unroll") for (int i = 0; i < LA; ++i) {                                                      \
        const v4f a4 = *reinterpret_cast<const v4f*>(Xs + (XB) * XS_FLOATS + (lrow + 32 * i) * 32 + lc4 * 4); \
        rmax = range_of(rmax, a4);                                                                        \
        f16x4 hi, lo;                                                                                     \
        split_f16(a4.x, a4.y, a4.z, a4.w, hi, lo);                                                      \
        const int st_ = swz64(lrow + 32 * i, lc4 >> 1) + (lc4 & 1) * 8;                                   \
        *reinterpret_cast<f16x4*>(Ah + (AB) * A_BYTES + st_) = hi;                                        \
        *reinterpret_cast<f16x4*>(Al + (AB) * A_BYTES + st_) = lo;                                        \
    }
#define BD_P_WORK(XB, AB)                                                                                 \
    if constexpr (PWO) { BD_P_CVT(XB, AB) } else { BD_P_DW(XB, AB) }
            // first the three slab requests, then the taps + shift of all K channels ([10][K] floats, ordinary loads):
            // the compiler drains vmcnt before the first tap is written to LDS, which also covers the slabs - one
            // memory round trip for the whole prologue instead of two
            if constexpr (NDW == 1) {
                // the NEXT layer's taps + shift of this tile's BN columns for the epilogue, [10][BN] behind the f32 tile: ten 1 KB
                // rows by LDS-DMA, issued before the slabs so that the counted waits below cover them
                float* const Nw = reinterpret_cast<float*>(smem_raw + (size_t)BM * (BN + 4) * 4);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int t = pw + 4 * c;
                    if (t < 10) {
                        const float* src = (t < 9 ? ndw_w + (size_t)t * N : ndw_b) + n0 + 4 * lane;
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                         (__attribute__((address_space(3))) void*)(Nw + t * BN), 16, 0, 0);
                    }
                }
            }
            BD_X_DMA(0, 0)
            BD_X_DMA(32, 1)
            BD_X_DMA(64, 2)
            if constexpr (!PWO) {
                // dw_w is [9][K] contiguous, dw_b [K]: as float4 items i < 9 K / 4 resp. the rest, Wall has the same
                // flat layout.  All loads are issued before the first write (a plain loop made five serial round trips).
                constexpr int TI = 10;            // items per thread at K = 1024
                const int n_w = 9 * (K / 4), n_all = 10 * (K / 4);
                v4f tw_[TI];
#pragma unroll
                for (int j = 0; j < TI; ++j) {
                    const int i = pt + 256 * j;
                    if (i < n_all) tw_[j] = *reinterpret_cast<const v4f*>(i < n_w ? dw_w + 4 * (size_t)i : dw_b + 4 * (size_t)(i - n_w));
                }
#pragma unroll
                for (int j = 0; j < TI; ++j) {
                    const int i = pt + 256 * j;
                    if (i < n_all) *reinterpret_cast<v4f*>(Wall + 4 * (size_t)i) = tw_[j];
                }
            }
            BD_P_SYNC(2 * ND)                 // slab 0 has landed, the taps are written
            BD_P_WORK(0, 0)
            BD_P_SYNC(ND)                     // A[0] written; slab 1 has landed
            int rs = 1;                       // ring slot of slab k+1
            int k = 0;
            for (; k + 3 < nk; ++k) {         // stage k: slab k+3 replaces slab k (consumed during stage k-1)
                const int r3 = rs == 0 ? 2 : rs - 1;
                BD_X_DMA((k + 3) * 32, r3)
                kch_ = (k + 1) * 32;
                BD_P_WORK(rs, (k + 1) & 1)
                BD_P_SYNC(ND)                 // slab k+2 has landed, slab k+3 stays in flight
                rs = rs == 2 ? 0 : rs + 1;
            }
            for (; k + 1 < nk; ++k) {         // the last two depthwise stages: nothing left to request
                kch_ = (k + 1) * 32;
                BD_P_WORK(rs, (k + 1) & 1)
                BD_P_SYNC(0)
                rs = rs == 2 ? 0 : rs + 1;
            }
            BD_P_SYNC(0)                      // consumers' last MFMA stage
#undef BD_X_DMA
#undef BD_X_DMA1
#undef BD_P_SYNC
#undef BD_P_WORK
#undef BD_P_CVT
        }
#undef BD_P_DW
    } else {
    // ===================================================================== consumers
    const int wc = wave;                      // column block of this wave
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    const int frow = lane & 31;
    const int fh = lane >> 5;
    {
        // The consumers do not stage the weights through LDS: with the 1 x 4 consumer layout every wave owns its own WN
        // output columns, so a weight fragment is used by exactly one wave: each lane loads its MFMA B fragments (16 bytes of
        // hi, 16 of lo per k-step and column tile) straight from global/L2 into a double-buffered register set, one stage
        // ahead.  Whi / Wlo are the fragment-order copies (SepLayer::pw_fhi / pw_flo): a load is one contiguous KiB per wave.
        // fragment pointers: column tile j -> row n0 + wc*WN + 32 j + frow of W^T, k offset 8 (2 s + fh)
        const _Float16* wph[TN];
        const _Float16* wpl[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const size_t frag = ((size_t)((n0 + wc * WN) / 32 + j) * (K / 16) * 64 + lane) * 8;
            wph[j] = Whi + frag;
            wpl[j] = Wlo + frag;
        }
        f16x8 b0h[TN][2], b0l[TN][2], b1h[TN][2], b1l[TN][2];    // fragments of an even / an odd stage
#define BD_W_LOAD(BH, BL, KOFF)                                                                           \
    {                                                                                                     \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) _Pragma("unroll") for (int s = 0; s < 2; ++s) {    \
            BH[j][s] = *reinterpret_cast<const f16x8*>(wph[j] + (KOFF) * 32 + 512 * s);                   \
            BL[j][s] = *reinterpret_cast<const f16x8*>(wpl[j] + (KOFF) * 32 + 512 * s);                   \
        }                                                                                                 \
    }
        // one stage = 2 TM steps (k16 step s x row tile i) of 3 TN MFMAs; the A fragments of step n+1 are requested
        // before the MFMAs of step n are issued (reading all TM pairs of a k16 step and then waiting exposed two
        // LDS latencies per stage)
#define BD_W_AFRAG(AH, AL, BUF, N)                                                                        \
    {                                                                                                     \
        const int off = (BUF) * A_BYTES + swz64(((N) % TM) * 32 + frow, 2 * ((N) / TM) + fh);             \
        AH = *reinterpret_cast<const f16x8*>(Ah + off);                                                   \
        AL = *reinterpret_cast<const f16x8*>(Al + off);                                                   \
    }
#define BD_W_MFMA(BUF, BH, BL)                                                                            \
    {                                                                                                     \
        f16x8 ahx[2], alx[2];                                                                             \
        BD_W_AFRAG(ahx[0], alx[0], BUF, 0)                                                                \
        _Pragma("unroll") for (int n = 0; n < 2 * TM; ++n) {                                              \
            if (n + 1 < 2 * TM) BD_W_AFRAG(ahx[(n + 1) & 1], alx[(n + 1) & 1], BUF, n + 1)                \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                              \
                if constexpr (!PLAIN) {                                                                   \
                    acc[n % TM][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alx[n & 1], BH[j][n / TM], acc[n % TM][j], 0, 0, 0); \
                    acc[n % TM][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahx[n & 1], BL[j][n / TM], acc[n % TM][j], 0, 0, 0); \
                }                                                                                         \
                acc[n % TM][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahx[n & 1], BH[j][n / TM], acc[n % TM][j], 0, 0, 0); \
            }                                                                                             \
        }                                                                                                 \
    }
        // stage t = 32 channels; its A block is ring slot t & 1, its fragments b0 (t even) / b1 (t odd)
        const int T = K / 32;                 // even, >= 4
        BD_W_LOAD(b0h, b0l, 0)
        BD_W_LOAD(b1h, b1l, 32)
        __syncthreads();
        __syncthreads();
        int t = 0;
        for (; t + 2 < T; t += 2) {
            BD_W_MFMA(t & 1, b0h, b0l)
            BD_W_LOAD(b0h, b0l, (t + 2) * 32)
            __syncthreads();
            BD_W_MFMA((t + 1) & 1, b1h, b1l)
            BD_W_LOAD(b1h, b1l, (t + 3) * 32)
            __syncthreads();
        }
        BD_W_MFMA(t & 1, b0h, b0l)
        __syncthreads();
        BD_W_MFMA((t + 1) & 1, b1h, b1l)
        __syncthreads();
#undef BD_W_AFRAG
#undef BD_W_LOAD
#undef BD_W_MFMA
    }

    // bias + ReLU into an f32 tile in LDS (every stage buffer is dead after the last barrier)
    float* const Ct = reinterpret_cast<float*>(smem_raw);          // [BM][BN + 4]
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nl = wc * WN + j * 32 + frow;
        const float b = pw_b[n0 + nl], u = pw_u[n0 + nl];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mb = i * 32 + 4 * fh;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = mb + (r & 3) + 8 * (r >> 2);
                Ct[ml * (BN + 4) + nl] = fmaxf(fmaf(acc[i][j][r], u, b), 0.0f);
            }
        }
    }
    }   // consumers

    __syncthreads();
    if constexpr (NDW == 1) {
        // ---- next layer's depthwise (stride 2) on the tile: windows are whole, so every tap is in LDS ----
        // A wave's 64 lanes are the 64 channel quads of ONE output position (8 waves x 3 positions = the tile's 24), so the
        // position, its padding tests and its row arithmetic are scalar; the two maps this runs on (12 x 8: layer 6, 6 x 4:
        // layer 12 on the test-hook path) are compile-time cases, so no division survives; taps and shift were brought to
        // LDS by the producers' prologue.  (Round 2's form - a position per thread with run-time divisions and nine divergent
        // padding branches - was a third of a layer-6 tile's time.)
        const float* Ct = reinterpret_cast<const float*>(smem_raw);
        constexpr int C4 = BN / 4, CTW = BN + 4;
        static_assert(C4 == 64, "a wave per output position");
        const float* Nw = reinterpret_cast<const float*>(smem_raw + (size_t)BM * (BN + 4) * 4);
        const int c4 = tid & 63;
        const int slot = __builtin_amdgcn_readfirstlane(tid >> 6);
        v4f wt[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) wt[t] = *reinterpret_cast<const v4f*>(Nw + t * BN + c4 * 4);
        const v4f shift = *reinterpret_cast<const v4f*>(Nw + 9 * BN + c4 * 4);
        const unsigned m0u = (unsigned)m0;
        auto positions = [&](auto hh_, auto ww_) {
            constexpr int HH = decltype(hh_)::value, WW = decltype(ww_)::value, PP = HH * WW;
            constexpr int OW2 = WW / 2, P2 = (HH / 2) * OW2, NPOS = (BM / PP) * P2;
            static_assert(NPOS == 24, "three output positions per wave");
#pragma unroll
            for (int pp = 0; pp < NPOS; pp += 8) {
                const int ps = pp + slot;
                const int wl = ps / P2, pos2 = ps % P2;
                if (m0 + (long long)wl * PP >= M) continue;
                const int oh = pos2 / OW2, ow = pos2 % OW2;
                const float* base = Ct + (wl * PP + 2 * oh * WW + 2 * ow) * CTW + c4 * 4;
                v4f acc = shift;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        v4f v = {0.f, 0.f, 0.f, 0.f};        // SAME padding: 0 before, 1 after - a wave-uniform test
                        if (2 * oh + kh < HH && 2 * ow + kw < WW) v = *reinterpret_cast<const v4f*>(base + (kh * WW + kw) * CTW);
                        acc = __builtin_elementwise_fma(v, wt[kh * 3 + kw], acc);
                    }
                acc.x = fmaxf(acc.x, 0.0f);
                acc.y = fmaxf(acc.y, 0.0f);
                acc.z = fmaxf(acc.z, 0.0f);
                acc.w = fmaxf(acc.w, 0.0f);
                const long long row2 = (long long)(m0u / (unsigned)PP + wl) * P2 + pos2;
                *reinterpret_cast<v4f*>(out2 + (size_t)row2 * N + n0 + c4 * 4) = acc;
            }
        };
        if (H == 12) positions(std::integral_constant<int, 12>{}, std::integral_constant<int, 8>{});
        else positions(std::integral_constant<int, 6>{}, std::integral_constant<int, 4>{});
    } else {
        // ---- all 8 waves: tile -> HBM as whole rows, 16 bytes per lane ----
        const float* Ct = reinterpret_cast<const float*>(smem_raw);
        constexpr int C4 = BN / 4;                                   // float4 per tile row
#pragma unroll
        for (int it = 0; it < BM * C4 / 512; ++it) {
            const int id = tid + 512 * it;
            const int ml = id / C4, c4 = id % C4;
            const long long m = m0 + ml;
            if (m < M)
                *reinterpret_cast<v4f*>(Cout + (size_t)m * N + n0 + c4 * 4) =
                    *reinterpret_cast<const v4f*>(Ct + ml * (BN + 4) + c4 * 4);
        }
    }
    range_report(rmax, range_flag);
}

template <int NDW, int PWO, bool PLAIN = false>
void launch_sep_ws(const float* X, const SepLayer& L, float* out, long long M, hipStream_t stream,
                   const SepLayer* next = nullptr) {
    if constexpr (!PLAIN) {                   // mode 2: the same kernel with one MFMA per product
        if (L.pw_mode == 2) return launch_sep_ws<NDW, PWO, true>(X, L, out, M, stream, next);
    }
    constexpr int BN = 256, XPMAX = 96, BM = 96;
    constexpr size_t lds_pipe0 = 3u * (XPMAX + 1) * 128 + 2u * 2u * BM * 64;
    const size_t lds_pipe = lds_pipe0 + (!PWO ? (size_t)40 * L.cin : 0);   // + taps and shift of all input channels
    constexpr size_t lds_tile = (size_t)BM * (BN + 4) * 4 + (NDW == 1 ? 40u * BN : 0u);   // NDW = 1: + the next layer's taps and shift
    const size_t lds = lds_pipe > lds_tile ? lds_pipe : lds_tile;
    constexpr size_t lds_pipe_max = lds_pipe0 + (!PWO ? 40u * 1024u : 0u);          // the widest layer has 1024 input channels
    constexpr size_t lds_max = lds_pipe_max > lds_tile ? lds_pipe_max : lds_tile;
    allow_dynamic_lds<&sep_ws_kernel<NDW, PWO, PLAIN>>((int)lds_max);
    const int tiles_n = L.cout / BN;
    const long long tiles = ((M + BM - 1) / BM) * tiles_n;
    hipLaunchKernelGGL((sep_ws_kernel<NDW, PWO, PLAIN>), dim3((unsigned)tiles), dim3(512), lds, stream, X, dw_w_of(L),
                       dw_b_of(L), static_cast<const _Float16*>(L.pw_fhi), static_cast<const _Float16*>(L.pw_flo), L.pw_u, L.pw_b,
                       out, M, L.cout, L.cin, L.h_out, L.w_out, tiles_n, next ? dw_w_of(*next) : nullptr,
                       next ? dw_b_of(*next) : nullptr, out, L.range_flag);
}

// The 1x1 convolutions of layers 5 (128 -> 256) and 7 (256 -> 512) have so few input channels that a wave's share of the
// split-f16 weights - 32 output columns x K, hi and lo - fits its register file: 64 VGPRs at K = 128, 128 at K = 256.
// A workgroup is 8 equal waves, wave w owning columns 32 w .. 32 w + 31 of a 256-column block; it is PERSISTENT
// (one per CU), loads its weight fragments once and then walks 32-row tiles of the input: all waves split the
// next tile into f16 hi + lo in LDS (rows requested three tiles ahead, straight into registers), every wave runs the
// 3 K / 16 MFMAs of its column tile on the current one and writes bias + ReLU from the accumulators (a store
// instruction covers two 128-byte row segments).  No weight traffic after the prologue, no pipeline fill per tile, one
// barrier per tile.  Same products in the same order as pointwise_f16x3_kernel: bit-identical.
template <int K16, bool PLAIN>
__global__ __launch_bounds__(512, 2) void pw_res_kernel(const float* __restrict__ X, const _Float16* __restrict__ Wfhi,
                                                         const _Float16* __restrict__ Wflo, const float* __restrict__ unscale,
                                                         const float* __restrict__ bias,
                                                         float* __restrict__ C, int M, int N, int tiles_n,
                                                         unsigned* __restrict__ range_flag) {
    constexpr int K = 16 * K16;
    constexpr int V = K16 / 4;                // float4 items per thread and tile: 32 rows x K / 4 over 512 threads
    constexpr int RP = 2048 / K;              // rows the 512 threads cover per item
    constexpr int ROWB = 2 * K;               // bytes of a row of one f16 half
    constexpr int HALF = 32 * ROWB;
    constexpr int R = PLAIN ? 1 : 2;          // LDS operations per fragment / per split item
    using S = PwResSchedule<K16, V, R>;
    // [2 buffers][hi, lo][32 rows][K] f16; the 16-byte chunks of a row are XOR-swizzled by the row number
    extern __shared__ __attribute__((aligned(1024))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fh = lane >> 5;

    // column block h and row stream r of this workgroup: IDs b and b + 8 (same XCD, dispatched together) are the
    // column blocks of the same row tiles, so the second read of a tile is an L2 hit
    const unsigned b = blockIdx.x, tn = (unsigned)tiles_n;
    const unsigned h = (b >> 3) % tn;
    const int r = (int)((b / (8 * tn)) * 8 + (b & 7));
    const int streams = (int)(gridDim.x / tn);
    const int n_tiles = (M + 31) >> 5;
    if (r >= n_tiles) return;
    const int ct = (int)h * 8 + wave;         // column tile of this wave

    // split items: thread -> (row r0 + RP j, channels 4 c4 ..) of a tile
    const int r0 = tid / (K / 4), c4 = tid % (K / 4);
    const float* const xcol = X + c4 * 4;
    const unsigned lds0 = pw_lds_addr(smem_raw);
    const unsigned st0 = lds0 + r0 * ROWB + (((c4 >> 1) ^ (r0 & 15)) << 4) + (c4 & 1) * 8;
    // fragment (row frow, k 16 q + 8 fh ..): chunk (2 q + fh) ^ (frow & 15), i.e. fr0 ^ (q << 5) as a byte address
    const unsigned fr0 = lds0 + frow * ROWB + ((fh ^ (frow & 15)) << 4);
    v4f rx[2][V];
    float rmax = 0.0f;
#define BD_R_LOAD(DST, TILE)                                                                              \
    _Pragma("unroll") for (int j = 0; j < V; ++j) {                                                       \
        int row_ = 32 * (TILE) + r0 + RP * j;                                                             \
        row_ = row_ < M ? row_ : M - 1;                                                                   \
        DST[j] = *reinterpret_cast<const v4f*>(xcol + (size_t)row_ * K);                                  \
    }
#define BD_R_SPLIT1(SRC, J, BUF)                                                                          \
    {                                                                                                     \
        const v4f a4 = SRC[J];                                                                            \
        rmax = range_of(rmax, a4);                                                                        \
        f16x4 hi, lo;                                                                                     \
        split_f16(a4.x, a4.y, a4.z, a4.w, hi, lo);                                                      \
        const unsigned st_ = (st0 ^ (((RP * (J)) & 15) << 4)) + RP * (J) * ROWB + (BUF) * 2 * HALF;       \
        pw_lds_store64(st_, hi);                                                                          \
        if constexpr (!PLAIN) pw_lds_store64(st_ + HALF, lo);                                             \
    }
    int t = r;
    BD_R_LOAD(rx[0], t)
    BD_R_LOAD(rx[1], t + streams)

    f16x8 bh[K16], bl[K16];
#pragma unroll
    for (int q = 0; q < K16; ++q) {
        const size_t frag = ((size_t)(ct * K16 + q) * 64 + lane) * 8;
        bh[q] = *reinterpret_cast<const f16x8*>(Wfhi + frag);
        if constexpr (!PLAIN) bl[q] = *reinterpret_cast<const f16x8*>(Wflo + frag);
    }
    const int col = ct * 32 + frow;
    const float bcol = bias[col], ucol = unscale[col];

#pragma unroll
    for (int j = 0; j < V; ++j) BD_R_SPLIT1(rx[0], j, 0)
    BD_R_LOAD(rx[0], t + 2 * streams)
    // the weights have to be in their registers HERE: left to the compiler, their waits land between the MFMAs of the
    // loop, where in steady state they wait for the previous tile's stores instead
#pragma unroll
    for (int q = 0; q < K16; ++q) {
        bh[q] = pw_landed(bh[q]);
        if constexpr (!PLAIN) bl[q] = pw_landed(bl[q]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    // during tile i register set i & 1 holds the rows of tile i + 2 and the other set those of tile i + 1, which are
    // split now and replaced by the request for tile i + 3; the loop is unrolled by two so that the sets are named statically
    auto tile = [&](auto pc) {
        constexpr int p = decltype(pc)::value;                 // = i & 1: LDS buffer of this tile
        constexpr int buf = p;
        // A fragments through a ring of three k-steps, requested two steps ahead: the wave's LDS operations complete in
        // order, so "the fragments of step q have landed" is a count of what was issued after them (PwResSchedule).
        // The rows of the next tile are split into the other buffer in V pieces placed between the MFMAs (past the last
        // tile they are clamped copies nobody reads); once the last piece is taken its registers take the request for
        // the rows two tiles ahead.
        const unsigned ab = fr0 + buf * 2 * HALF;
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        f16x8 fa[3][2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            fa[q][0] = pw_lds_frag<0>(ab ^ (q << 5));
            if constexpr (!PLAIN) fa[q][1] = pw_lds_frag<HALF>(ab ^ (q << 5));
        }
        static_for_pw<0, K16>([&](auto qi) {
            constexpr int q = decltype(qi)::value;
            if constexpr (q + 2 < K16) {
                fa[(q + 2) % 3][0] = pw_lds_frag<0>(ab ^ ((q + 2) << 5));
                if constexpr (!PLAIN) fa[(q + 2) % 3][1] = pw_lds_frag<HALF>(ab ^ ((q + 2) << 5));
            }
            if constexpr (S::split_at(q) >= 0) {
                constexpr int j = S::split_at(q) >= 0 ? S::split_at(q) : 0;
                BD_R_SPLIT1(rx[p ^ 1], j, buf ^ 1)
            }
            pw_lds_wait<S::pending(q)>();
            const f16x8 ah = pw_landed(fa[q % 3][0]);
            if constexpr (!PLAIN) {
                const f16x8 al = pw_landed(fa[q % 3][1]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[q], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[q], acc, 0, 0, 0);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[q], acc, 0, 0, 0);
        });
        BD_R_LOAD(rx[p ^ 1], t + 3 * streams)      // set p ^ 1 held tile i + 1 (split above): now tile i + 3
        const int row0 = 32 * t + 4 * fh;
        float* const crow = C + (size_t)row0 * N + col;
        if (32 * t + 32 <= M) {
#pragma unroll
            for (int e = 0; e < 16; ++e) crow[(size_t)((e & 3) + 8 * (e >> 2)) * N] = fmaxf(fmaf(acc[e], ucol, bcol), 0.0f);
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (row0 + (e & 3) + 8 * (e >> 2) < M) crow[(size_t)((e & 3) + 8 * (e >> 2)) * N] = fmaxf(fmaf(acc[e], ucol, bcol), 0.0f);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        t += streams;
    };
    for (;;) {
        tile(std::integral_constant<int, 0>{});
        if (t >= n_tiles) break;
        tile(std::integral_constant<int, 1>{});
        if (t >= n_tiles) break;
    }
#undef BD_R_LOAD
#undef BD_R_SPLIT1
    range_report(rmax, range_flag);
}

template <int K16, bool PLAIN = false>
void launch_pw_res(const float* X, const SepLayer& L, float* out, int M, hipStream_t stream) {
    if constexpr (!PLAIN) {
        if (L.pw_mode == 2) return launch_pw_res<K16, true>(X, L, out, M, stream);
    }
    constexpr int lds = 2 * 2 * 32 * 32 * K16;
    allow_dynamic_lds<&pw_res_kernel<K16, PLAIN>>(lds);
    const int tiles_n = L.cout / 256;
    const int n_tiles = (M + 31) / 32;
    // one workgroup per CU (256 on MI355X), in whole groups of 8 row streams x tiles_n column blocks
    int streams = 256 / tiles_n;
    if (streams > n_tiles) streams = (n_tiles + 7) / 8 * 8;
    hipLaunchKernelGGL((pw_res_kernel<K16, PLAIN>), dim3((unsigned)(streams * tiles_n)), dim3(512), lds, stream, X,
                       static_cast<const _Float16*>(L.pw_fhi), static_cast<const _Float16*>(L.pw_flo), L.pw_u, L.pw_b, out, M,
                       L.cout, tiles_n, L.range_flag);
}

}  // namespace

// 1x1 convolution of a layer with 128 or 256 input channels (layers 5 and 7) with the weights in registers; the caller has
// checked the shape (launch_pointwise_ws)
void launch_pointwise_res(const float* in, float* out, int rows, const SepLayer& L, hipStream_t stream) {
    if (L.cin == 128) launch_pw_res<8>(in, L, out, rows, stream);
    else launch_pw_res<16>(in, L, out, rows, stream);
}

// 1x1 convolution on the wave-specialised kernel: the producers only split the input rows into f16 hi + lo (no depthwise); the
// caller has checked the shape (launch_pointwise_ws)
void launch_pointwise_sep_ws(const float* in, float* out, int64_t rows, const SepLayer& L, hipStream_t stream) {
    launch_sep_ws<0, 1>(in, L, out, rows, stream);
}

// launch_separable_fused_next_dw on whole-window tiles: only the 12x8 and 6x4 maps.
bool launch_sep_ws_next_dw(const float* in, float* out, int windows, const SepLayer& L, const SepLayer& next, hipStream_t stream) {
    const int P = L.h_out * L.w_out;
    if (L.stride != 1 || next.stride != 2 || windows <= 0 || L.cin < 128 || L.cout % 256 != 0) return false;
    // (the epilogue's position arithmetic is compiled for these two maps)
    if (!((L.h_out == 12 && L.w_out == 8) || (L.h_out == 6 && L.w_out == 4)) || next.cin != L.cout) return false;
    const long long M = (long long)windows * P;
    if (M >= (1LL << 31)) return false;       // the kernel's tile arithmetic is 32-bit
    launch_sep_ws<1, 0>(in, L, out, M, stream, &next);
    return true;
}

}  // namespace bd
