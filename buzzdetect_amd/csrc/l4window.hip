// Layer 4 + depthwise 5 of YAMNet as one kernel, whole windows per persistent workgroup (l4_window_kernel); on the default
// path (PLANES) with layer 3's 1x1 convolution in front, on the split-f16 A tiles stem_reg_kernel<.., true> (stemreg.hip)
// writes.  Its output is what sep_mid_kernel (sepmid.hip) reads.
#include "bd_device.h"

namespace bd {

namespace {

// Layer 4 is the widest map (24 x 16) with the fewest channels (128 -> 128): as 96-row tiles of the generic kernel it is
// four short stages per tile behind a full pipeline fill, and the band tiles that carry depthwise 5 in their epilogue
// compute every other row pair twice.  Here a workgroup is persistent (one per CU), owns WINDOWS b, b + G, .. and walks
// each top to bottom in twelve steps of two map rows (= one 32-row MFMA tile, all 128 input channels at once):
//   waves 0-3 (matrix side)  the split-f16 weights of their 32 output channels live in registers for the whole launch
//                            (64 VGPRs); per step they move two input rows global -> registers -> LDS ring (requested
//                            four steps ahead), run the 24 MFMAs of the row tile the vector side finished in the previous
//                            step, and - round 6 - run depthwise 5 (stride 2) on the tile where it lies, in the
//                            accumulators: lane (channel, half h) holds columns {0-3, 8-11} + 4 h of the tile's two map
//                            rows, i.e. everything four of the eight output columns need but the one column behind each
//                            group of four, which one v_permlane32_swap per group and row brings from the other half.
//                            One output row per step; its third input row arrives a step later - the partial sums wait in
//                            registers, the order of the nine FMAs is unchanged.  (Until round 5 the even-column vector
//                            waves did this from an f32 copy of the tile in LDS: the vector side was the kernel's bound
//                            - 2 550 of its cycles per step against 1 770 - and without that work the kernel takes 54
//                            instead of 69 us, gpurun_out/r06/abl_l4_nodw5.log.)
//   waves 4-11 (vector side) a thread owns four channels (its taps and shift stay in registers) and one map column: the
//                            3x3 depthwise of the step's two outputs from a register window of 4 x 3 inputs that slides
//                            down the map (6 LDS reads per step), split into the A tile of the next MFMA step.  Two vector
//                            waves and one matrix wave per SIMD.
// so nothing is computed twice, layer 4's own output never exists, and the input is read once.  The row tiles of a
// workgroup's windows form ONE stream (tile T = 12 i + s): step K runs the depthwise of tile K and the MFMAs + depthwise 5 of
// tile K - 1, so the pipeline fills once per launch, not once per window; the top and bottom rows of
// a window take zeros instead of their neighbours' rows.  One barrier per step.  Arithmetic order per element equals
// depthwise_kernel / pointwise_f16x3_kernel: bit-identical to the unfused path.
// PLANES (the default launch set since round 7): X is not the layer-3 output but what stem_reg_kernel<.., true> leaves of it
// before layer 3's 1x1 convolution - its split-f16 A tiles as they lay in the stem's LDS, [window][row pair][hi, lo][2 k-halves]
// [32 rows][64 B] (8 KB per row pair, half of the f32 rows) - and the matrix waves run that convolution (the stem's phases G and
// H: the same weight fragments, k order and epilogue, so the same bits) for row pair k + 2 in step k, straight into the ring.
// Per step they copy the image of row pair k + 3 into one of two 8 KB LDS stages (requested a step earlier, 32 B a lane in
// place of 64) and run 12 more MFMAs; the ring keeps its lead of two row pairs.
template <bool PLAIN, bool PLANES>
__global__ __launch_bounds__(768) void l4_window_kernel(
    const float* __restrict__ X, const float* __restrict__ dw_w, const float* __restrict__ dw_b,
    const _Float16* __restrict__ Wfhi, const _Float16* __restrict__ Wflo, const float* __restrict__ pw_u,
    const float* __restrict__ pw_b,
    const float* __restrict__ ndw_w, const float* __restrict__ ndw_b, float* __restrict__ out, int windows,
    unsigned* __restrict__ range_flag, const _Float16* __restrict__ W3fhi, const _Float16* __restrict__ W3flo,
    const float* __restrict__ pw3_u, const float* __restrict__ pw3_b) {
    constexpr int H = 24, W = 16, C = 128, K16 = 8, STEPS = H / 2;
    constexpr int COL_B = C * 4;                       // bytes of one map position, f32
    constexpr int ROW_B = (W + 1) * COL_B;             // ring slot of a map row: 16 columns + a zero column
    constexpr int RING0 = COL_B;                       // a zero column in front of slot 0 (column -1 of slot 0)
    constexpr int A0 = RING0 + 8 * ROW_B;              // A tile [2 buffers][hi, lo][32 rows][128 f16], chunks XOR-swizzled
    constexpr int A_HALF = 32 * 2 * C, A_BUF = 2 * A_HALF;
    constexpr int T5 = A0 + 2 * A_BUF;                 // depthwise 5's taps and shift per channel, [128][12] f32 (10 used): as registers
                                                       // of the matrix waves they would not fit beside the weights (168 per lane)
    constexpr int O5 = T5 + C * 12 * 4;                // finished depthwise-5 rows on their way out, [2 steps][2 rows][8][128] f32: the
                                                       // matrix waves wait for their input rows with a counted vmcnt, which a store
                                                       // of their own in between turns into vmcnt(0) - the vector waves store
    constexpr int O5_ROW = (W / 2) * C * 4, O5_BUF = 2 * O5_ROW;
    constexpr int PL0 = O5 + 2 * O5_BUF;               // PLANES: two stages of a row pair's split-f16 image [hi, lo][2][32][64 B]
    constexpr int PL_B = 8192, PL_HALF = 4096;
    constexpr int W3L = PL0 + 2 * PL_B;                // PLANES, split-f16: layer 3's low weight fragments [wave][4][64 lanes][16 B]
                                                       // (as registers beside the high ones the matrix waves spill)
    constexpr size_t WIN_IN = (size_t)H * W * C, WIN_OUT = (size_t)STEPS * (W / 2) * C;
    static_assert(A0 % 512 == 0, "fragment addresses are formed by XOR");
    static_assert((2 * STEPS) % 8 == 0 && STEPS % 2 == 0, "ring slots and buffer parities carry over from window to window");
    extern __shared__ __attribute__((aligned(1024))) char smem_raw[];
    char* const smem = smem_raw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x, G = gridDim.x;
    if (b >= windows) return;
    const int NT = STEPS * ((windows - b + G - 1) / G);          // row tiles of this workgroup

    // the zero columns: in front of the ring and column 16 of every ring slot
    for (int i = tid; i < 9 * 32; i += 768) {
        const int z = i >> 5;
        *reinterpret_cast<v4f*>(smem + (z == 0 ? 0 : RING0 + (z - 1) * ROW_B + W * COL_B) + (i & 31) * 16) = v4f{0.f, 0.f, 0.f, 0.f};
    }
    for (int i = tid; i < 10 * C; i += 768) {          // taps t = 0 .. 8 and the shift (t = 9) of channel c at [c][t]
        const int t = i / C, c = i - t * C;
        reinterpret_cast<float*>(smem + T5)[c * 12 + t] = t < 9 ? ndw_w[t * C + c] : ndw_b[c];
    }
    float rmax = 0.0f;

    if (wave < 4) {
        // ================================================================= matrix side
        const int frow = lane & 31, fh = lane >> 5;
        const int c4 = tid & 31, col_lo = tid >> 5;    // slab items: 16-byte chunk c4 of columns col_lo and col_lo + 8
        const float* const xt = X + (size_t)b * WIN_IN + (size_t)col_lo * C + c4 * 4;
        char* const ring_t = smem + RING0 + col_lo * COL_B + c4 * 16;
        v4f rs[2][4];                                  // two row pairs in flight
        // row pair J of the stream = rows 2 j, 2 j + 1 of the workgroup's window i (J = 12 i + j), ring slots (2 J + row) & 7
#define BD_L4_LOAD(DST, J)                                                                                \
    {                                                                                                     \
        const int i_ = (J) / STEPS, j_ = (J) - i_ * STEPS;                                                \
        const float* const src_ = xt + (size_t)i_ * G * WIN_IN + (size_t)j_ * (2 * W * C);                \
        _Pragma("unroll") for (int u = 0; u < 4; ++u)                                                     \
            DST[u] = *reinterpret_cast<const v4f*>(src_ + ((u >> 1) * W + 8 * (u & 1)) * C);              \
    }
#define BD_L4_STORE(SRC, J)                                                                               \
    _Pragma("unroll") for (int u = 0; u < 4; ++u)                                                         \
        *reinterpret_cast<v4f*>(ring_t + ((2 * (J) + (u >> 1)) & 7) * ROW_B + 8 * (u & 1) * COL_B) = SRC[u];
        // PLANES: the planes of row pair J (as BD_L4_LOAD: J = 12 i + j) - 16 bytes of each plane per thread - and the stage
        // they go to: stage J & 1
        const char* const pt = reinterpret_cast<const char*>(X) + (size_t)b * STEPS * PL_B + tid * 16;
        v4f rp[2], rq[2];                              // the planes of the next row pair for the stages (rq: the prologue's second)
#define BD_L4_PLOAD(DST, J)                                                                               \
    {                                                                                                     \
        const int i_ = (J) / STEPS, j_ = (J) - i_ * STEPS;                                                \
        const char* const src_ = pt + ((size_t)i_ * G * STEPS + j_) * PL_B;                               \
        DST[0] = *reinterpret_cast<const v4f*>(src_);                                                     \
        if constexpr (!PLAIN) DST[1] = *reinterpret_cast<const v4f*>(src_ + PL_HALF);                     \
    }
#define BD_L4_PSTORE(SRC, J)                                                                              \
    {                                                                                                     \
        char* const st_ = smem + PL0 + ((J) & 1) * PL_B + tid * 16;                                       \
        *reinterpret_cast<v4f*>(st_) = SRC[0];                                                            \
        if constexpr (!PLAIN) *reinterpret_cast<v4f*>(st_ + PL_HALF) = SRC[1];                            \
    }
        if constexpr (PLANES) {
            BD_L4_PLOAD(rp, 0)
            BD_L4_PLOAD(rq, 1)
        } else {
            BD_L4_LOAD(rs[0], 0)
            BD_L4_LOAD(rs[1], 1)
        }
        f16x8 bh[K16], bl[K16];
#pragma unroll
        for (int q = 0; q < K16; ++q) {
            const size_t frag = ((size_t)(wave * K16 + q) * 64 + lane) * 8;
            bh[q] = *reinterpret_cast<const f16x8*>(Wfhi + frag);
            if constexpr (!PLAIN) bl[q] = *reinterpret_cast<const f16x8*>(Wflo + frag);
        }
        const int ncol = 32 * wave + frow;
        const float bcol = pw_b[ncol], ucol = pw_u[ncol];
        // PLANES: layer 3's weight fragments (output channel ncol: the stem's n3) for the whole launch, its scale and shift
        f16x8 w3h[PLANES ? 4 : 1];
        char* const w3l = smem + W3L + (wave * 4 * 64 + lane) * 16;      // fragment q at + q * 1024 (each lane reads what it wrote)
        float u3 = 0.0f, b3 = 0.0f;
        if constexpr (PLANES) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const size_t frag = ((size_t)(wave * 4 + q) * 64 + lane) * 8;
                w3h[q] = *reinterpret_cast<const f16x8*>(W3fhi + frag);
                if constexpr (!PLAIN) *reinterpret_cast<f16x8*>(w3l + q * 1024) = *reinterpret_cast<const f16x8*>(W3flo + frag);
            }
            u3 = pw3_u[ncol];
            b3 = pw3_b[ncol];
        }
        // PLANES: layer 3's 1x1 convolution of row pair J from stage J & 1 (stemreg.hip, phases G and H): accumulator element r is
        // tile row m = 4 fh + (r & 3) + 8 (r >> 2) = map row 2 j + (m >> 4), column m & 15 -> ring slot (2 J + (m >> 4)) & 7
        // (fragment (row frow, k 16 q + 8 fh ..) of a plane: swz64(frow, 2 (q & 1) + fh), i.e. pl_a[q & 1] +
        //  (q >> 1) * 2048 within the stage; the stage J & 1 is the step's parity, a constant: two address registers, the rest
        //  immediate offsets - with PL0 > 65535 in the offsets the compiler keeps eight addresses and spills them)
        typedef const __attribute__((address_space(3))) f16x8* lptrh;
        unsigned pl_a[2];
        pl_a[0] = pw_lds_addr(smem) + (unsigned)(PL0 + frow * 64 + ((fh ^ ((frow >> 2) & 3)) << 4));
        pl_a[1] = pl_a[0] ^ 32u;
        asm("" : "+v"(pl_a[0]), "+v"(pl_a[1]));
        auto pw3 = [&](auto stage_c, int J) {
            constexpr int stage = decltype(stage_c)::value;
            f32x16 acc3;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc3[r] = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned a = pl_a[q & 1] + (unsigned)(stage * PL_B + (q >> 1) * 2048);
                const f16x8 ah = *(lptrh)(size_t)a;
                if constexpr (!PLAIN) {
                    const f16x8 al = *(lptrh)(size_t)(a + PL_HALF);
                    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, w3h[q], acc3, 0, 0, 0);
                    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, *reinterpret_cast<const f16x8*>(w3l + q * 1024), acc3, 0, 0, 0);
                }
                acc3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, w3h[q], acc3, 0, 0, 0);
            }
            char* const rw = smem + RING0 + ncol * 4;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = 4 * fh + (r & 3) + 8 * (r >> 2);
                *reinterpret_cast<float*>(rw + ((2 * J + (m >> 4)) & 7) * ROW_B + (m & 15) * COL_B) = fmaxf(fmaf(acc3[r], u3, b3), 0.0f);
            }
        };
        // depthwise 5 of this lane's channel: the four partial sums (output columns 2 fh, 2 fh + 1, 4 + 2 fh, 5 + 2 fh); its taps
        // and shift are read from LDS when a step needs them
        const float* const t5 = reinterpret_cast<const float*>(smem + T5) + ncol * 12;
        float acc5[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float* const o5 = reinterpret_cast<float*>(smem + O5) + (2 * fh) * C + ncol;
        int s5 = 0;                                    // row tile within its window, of the tile the MFMAs work on
        if constexpr (PLANES) {
            BD_L4_PSTORE(rp, 0)
            BD_L4_PSTORE(rq, 1)
            BD_L4_PLOAD(rp, 2)
            BD_L4_PLOAD(rq, 3)
        } else {
            BD_L4_STORE(rs[0], 0)
            BD_L4_STORE(rs[1], 1)
            BD_L4_LOAD(rs[0], 2)
            BD_L4_LOAD(rs[1], 3)
        }
#pragma unroll
        for (int q = 0; q < K16; ++q) {                // the weights are in their registers before the loop (see pw_res_kernel)
            bh[q] = pw_landed(bh[q]);
            if constexpr (!PLAIN) bl[q] = pw_landed(bl[q]);
        }
        if constexpr (PLANES) {
            // row pairs 0 and 1 into the ring, pair 2 into stage 0, pair 3 in registers (three barriers: the vector side waits
            // at two more than without planes)
            __syncthreads();
            pw3(std::integral_constant<int, 0>{}, 0);
            __syncthreads();
            BD_L4_PSTORE(rp, 2)
            rp[0] = rq[0];
            rp[1] = rq[1];
            pw3(std::integral_constant<int, 1>{}, 1);
        }
        // fragment (row frow, k 16 q + 8 fh ..) sits in chunk (2 q + fh) ^ (frow & 15) of its row: fr0 ^ (q << 5)
        const unsigned fr0 = pw_lds_addr(smem) + (unsigned)(A0 + frow * 2 * C + ((fh ^ (frow & 15)) << 4));
        // accumulator element e is tile row (e & 3) + 8 (e >> 2) + 4 fh: map row m >> 4, column m & 15
        __syncthreads();
        auto step = [&](auto pc, int k) {
            constexpr int p = decltype(pc)::value;     // k & 1
            f32x16 acc;
            if (k >= 1 && k <= NT) {
                // row tile k - 1: A tile buffer (k - 1) & 1 = p ^ 1.  A fragments through a ring of three k-steps, requested
                // two steps ahead, with counted waits (pw_res_kernel)
                const unsigned ab = fr0 + (unsigned)((p ^ 1) * A_BUF);
                using S = PwResSchedule<K16, 0, PLAIN ? 1 : 2>;
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
                f16x8 fa[3][2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    fa[q][0] = pw_lds_frag<0>(ab ^ (q << 5));
                    if constexpr (!PLAIN) fa[q][1] = pw_lds_frag<A_HALF>(ab ^ (q << 5));
                }
                static_for_pw<0, K16>([&](auto qi) {
                    constexpr int q = decltype(qi)::value;
                    if constexpr (q + 2 < K16) {
                        fa[(q + 2) % 3][0] = pw_lds_frag<0>(ab ^ ((q + 2) << 5));
                        if constexpr (!PLAIN) fa[(q + 2) % 3][1] = pw_lds_frag<A_HALF>(ab ^ ((q + 2) << 5));
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
            }
            if constexpr (PLANES) {
                // the planes of row pair k + 3 into stage p ^ 1 (read in step k - 1), a request for those of pair k + 4 (a step
                // ahead: two in flight cost the registers of the weights); row pair k + 2 goes into the ring (from stage p,
                // written in step k - 1) at the end of the step
                if (k + 3 < NT) BD_L4_PSTORE(rp, k + 3)
                if (k + 4 < NT) BD_L4_PLOAD(rp, k + 4)
            } else {
                // the input rows two steps ahead into the ring, a request for those four steps ahead (under the last MFMAs)
                if (k + 2 < NT) { BD_L4_STORE(rs[p], k + 2) }
                if (k + 4 < NT) BD_L4_LOAD(rs[p], k + 4)
            }
            if (k >= 1 && k <= NT) {
                // ---- bias + ReLU, then depthwise 5 on the tile's two map rows 2 s5, 2 s5 + 1: y[r][0 .. 7] = this lane's columns
                // {0-3, 8-11} + 4 fh of row r; nb[r][g] = the column behind group g (column 4 / 12 for half 0: the other half's
                // first of that group; column 8 / 16 for half 1: half 0's first of its second group / the zero padding)
                float y[2][8], nb[2][2];
                const v4f t5a = *reinterpret_cast<const v4f*>(t5), t5b = *reinterpret_cast<const v4f*>(t5 + 4), t5c = *reinterpret_cast<const v4f*>(t5 + 8);
                const float w5[9] = {t5a.x, t5a.y, t5a.z, t5a.w, t5b.x, t5b.y, t5b.z, t5b.w, t5c.x};
                const float b5 = t5c.y;
#pragma unroll
                for (int e = 0; e < 16; ++e) y[e >> 3][e & 7] = fmaxf(fmaf(acc[e], ucol, bcol), 0.0f);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    // v_permlane32_swap vdst, src trades lanes 32-63 of vdst against lanes 0-31 of src: with vdst = own column 0
                    // of the group pair and src = own first column of the second group, half 1 finds half 0's column 8 in vdst
                    // and half 0 finds half 1's column 4 in src; a second swap brings half 1's column 12 to half 0
                    float va = y[r][0], wa = y[r][4], vb = y[r][4], wb = 0.0f;
                    asm("" : "+v"(va), "+v"(wa), "+v"(vb), "+v"(wb));
                    const auto s1 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, va), __builtin_bit_cast(unsigned, wa), false, false);
                    const auto s2 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, vb), __builtin_bit_cast(unsigned, wb), false, false);
                    nb[r][0] = __builtin_bit_cast(float, fh ? (unsigned)s1[0] : (unsigned)s1[1]);
                    nb[r][1] = fh ? 0.0f : __builtin_bit_cast(float, (unsigned)s2[1]);
                }
                // output t of this lane (t = 0, 1: group 0, t = 2, 3: group 1) reads, per input row, in[t][0 .. 2]
#define BD_L4_IN(R, T, KW) ((T) == 0 ? y[R][KW] : (T) == 1 ? ((KW) < 2 ? y[R][2 + (KW)] : nb[R][0]) : (T) == 2 ? y[R][4 + (KW)] : ((KW) < 2 ? y[R][6 + (KW)] : nb[R][1]))
                float* const orow = o5 + (p ^ 1) * (O5_BUF / 4);        // (tile k - 1: buffer of its parity; row slot 0, the last tile's second row slot 1)
                if (s5 > 0) {                          // finishes output row s5 - 1: its kh = 2 row is map row 2 s5
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) acc5[t] = fmaf(BD_L4_IN(0, t, kw), w5[6 + kw], acc5[t]);
                        orow[((t >> 1) * 4 + (t & 1)) * C] = fmaxf(acc5[t], 0.0f);
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {          // starts output row s5: kh = 0, 1
                    acc5[t] = b5;
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) acc5[t] = fmaf(BD_L4_IN(kh, t, kw), w5[3 * kh + kw], acc5[t]);
                }
                if (s5 == STEPS - 1) {                 // map row 24 is the zero padding (multiplied, as depthwise_kernel does)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) acc5[t] = fmaf(0.0f, w5[6 + kw], acc5[t]);
                        orow[((W / 2) + (t >> 1) * 4 + (t & 1)) * C] = fmaxf(acc5[t], 0.0f);
                    }
                    s5 = 0;
                } else {
                    ++s5;
                }
#undef BD_L4_IN
            }
            if constexpr (PLANES) {
                if (k + 2 < NT) pw3(pc, k + 2);            // (behind layer 4's epilogue: its accumulators and A fragments are dead)
            }
            __syncthreads();
        };
        for (int k = 0; k < NT + 2; k += 2) {          // (steps 0 .. NT + 1: NT is even; the last one is idle on both sides)
            step(std::integral_constant<int, 0>{}, k);
            step(std::integral_constant<int, 1>{}, k + 1);
        }
#undef BD_L4_LOAD
#undef BD_L4_STORE
#undef BD_L4_PLOAD
#undef BD_L4_PSTORE
    } else {
        // ================================================================= vector side
        // wave v = 0..7, half-wave hi: channels 4 c4 .. of ONE map column - the even columns in waves 0-3, the odd ones in waves 4-7
        const int v = wave - 4, c4 = lane & 31;
        const int col = v < 4 ? 2 * (2 * v + (lane >> 5)) : 2 * (2 * (v - 4) + (lane >> 5)) + 1;
        v4f w4[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) w4[t] = *reinterpret_cast<const v4f*>(dw_w + t * C + c4 * 4);
        const v4f b4 = *reinterpret_cast<const v4f*>(dw_b + c4 * 4);
        // input row r, columns col - 1 .. col + 1 (column -1 is the zero column in front, column 16 the one behind)
        const char* const xin = smem + RING0 + (col - 1) * COL_B + c4 * 16;
        // A tile: row m = 16 rr + col, channels 4 c4 ..: 8 bytes of chunk c4 >> 1
        int a_st[2];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int m = 16 * rr + col;
            a_st[rr] = A0 + m * 2 * C + (((c4 >> 1) ^ (m & 15)) << 4) + (c4 & 1) * 8;
        }
        v4f xr[4][3];                                  // input rows 2 s - 1 .. 2 s + 2 at [(2 p + i) & 3], three columns
        int s4 = 0;                                    // row tile within its window
        // waves v < 4 also carry the finished depthwise-5 rows from LDS to global memory, 16 bytes per lane: step k stores what the
        // matrix side finished in step k - 1 with tile k - 2 (row s5 - 1 of window i5; behind a window's last tile also row 11)
        const int o_lane = (v & 3) * 64 + lane;        // float4 index within a row of [8][128] f32
        float* const ot = out + (size_t)b * WIN_OUT + (size_t)o_lane * 4;
        int s5 = 0, i5 = 0;
        if constexpr (PLANES) {                        // the matrix side's prologue: row pairs 0 and 1 into the ring
            __syncthreads();
            __syncthreads();
        }
        __syncthreads();
        auto step = [&](auto pc, int k) {
            constexpr int p = decltype(pc)::value;     // k & 1
            if (v < 4 && k >= 2) {
                const char* const ob = smem + O5 + p * O5_BUF + o_lane * 16;          // (tile k - 2: buffer of its parity)
                float* const orow = ot + (size_t)i5 * G * WIN_OUT;
                if (s5 > 0) *reinterpret_cast<v4f*>(orow + (size_t)(s5 - 1) * (W / 2) * C) = *reinterpret_cast<const v4f*>(ob);
                if (s5 == STEPS - 1) {
                    *reinterpret_cast<v4f*>(orow + (size_t)s5 * (W / 2) * C) = *reinterpret_cast<const v4f*>(ob + O5_ROW);
                    s5 = 0;
                    ++i5;
                } else {
                    ++s5;
                }
            }
            if (k < NT) {
                // ---- depthwise 4 of map rows 2 s4, 2 s4 + 1 -> A tile buffer p (ring slots continue across windows)
                if (s4 == 0) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        xr[0][c] = v4f{0.f, 0.f, 0.f, 0.f};
                        xr[1][c] = *reinterpret_cast<const v4f*>(xin + c * COL_B);
                    }
                }
                {
                    const char* const r2 = xin + ((2 * k + 1) & 7) * ROW_B;
#pragma unroll
                    for (int c = 0; c < 3; ++c) xr[(2 * p + 2) & 3][c] = *reinterpret_cast<const v4f*>(r2 + c * COL_B);
                }
                if (s4 + 1 < STEPS) {
                    const char* const r3 = xin + ((2 * k + 2) & 7) * ROW_B;
#pragma unroll
                    for (int c = 0; c < 3; ++c) xr[(2 * p + 3) & 3][c] = *reinterpret_cast<const v4f*>(r3 + c * COL_B);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) xr[(2 * p + 3) & 3][c] = v4f{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    v4f a4 = b4;
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw)
                            a4 = __builtin_elementwise_fma(xr[(2 * p + rr + kh) & 3][kw], w4[kh * 3 + kw], a4);
                    a4.x = fmaxf(a4.x, 0.0f); a4.y = fmaxf(a4.y, 0.0f); a4.z = fmaxf(a4.z, 0.0f); a4.w = fmaxf(a4.w, 0.0f);
                    rmax = range_of(rmax, a4);
                    f16x4 hi, lo;
                    split_f16(a4.x, a4.y, a4.z, a4.w, hi, lo);
                    *reinterpret_cast<f16x4*>(smem + a_st[rr] + p * A_BUF) = hi;
                    if constexpr (!PLAIN) *reinterpret_cast<f16x4*>(smem + a_st[rr] + p * A_BUF + A_HALF) = lo;
                }
                s4 = s4 + 1 == STEPS ? 0 : s4 + 1;
            }
            __syncthreads();
        };
        for (int k = 0; k < NT + 2; k += 2) {
            step(std::integral_constant<int, 0>{}, k);
            step(std::integral_constant<int, 1>{}, k + 1);
        }
    }
    range_report(rmax, range_flag);
}

template <bool PLAIN, bool PLANES>
void launch_l4_window_form(const float* X, const SepLayer* L3, const SepLayer& L, const SepLayer& next, float* out, int windows,
                           hipStream_t stream) {
    constexpr int lds = 512 + 8 * 17 * 512 + 2 * 2 * 32 * 256 + 128 * 12 * 4 + 2 * 2 * 8 * 128 * 4 + (PLANES ? (PLAIN ? 2 : 4) * 8192 : 0);
    allow_dynamic_lds<&l4_window_kernel<PLAIN, PLANES>>(lds);
    const int grid = windows < 256 ? windows : 256;           // one persistent workgroup per CU
    hipLaunchKernelGGL((l4_window_kernel<PLAIN, PLANES>), dim3((unsigned)grid), dim3(768), lds, stream, X, dw_w_of(L), dw_b_of(L),
                       static_cast<const _Float16*>(L.pw_fhi), static_cast<const _Float16*>(L.pw_flo), L.pw_u, L.pw_b, dw_w_of(next),
                       dw_b_of(next), out, windows, L.range_flag,
                       PLANES ? static_cast<const _Float16*>(L3->pw_fhi) : nullptr,
                       PLANES ? static_cast<const _Float16*>(L3->pw_flo) : nullptr, PLANES ? L3->pw_u : nullptr,
                       PLANES ? L3->pw_b : nullptr);
}

void launch_l4_window(const float* X, const SepLayer& L, const SepLayer& next, float* out, int windows, hipStream_t stream) {
    if (L.pw_mode == 2) launch_l4_window_form<true, false>(X, nullptr, L, next, out, windows, stream);
    else launch_l4_window_form<false, false>(X, nullptr, L, next, out, windows, stream);
}

}  // namespace

bool l4_window_planes_supported(const SepLayer& L3, const SepLayer& L4, const SepLayer& L5) {
    return (L3.pw_mode == 1 || L3.pw_mode == 2) && L4.pw_mode == L3.pw_mode && L3.stride == 2 && L3.cin == 64 &&
           L3.cout == 128 && L3.h_out == 24 && L3.w_out == 16 && L3.pw_fhi && L3.pw_flo && L4.stride == 1 && L4.h_out == 24 &&
           L4.w_out == 16 && L4.cin == 128 && L4.cout == 128 && L5.stride == 2 && L5.cin == 128;
}

bool launch_l4_window_planes(const void* planes, const SepLayer& L3, const SepLayer& L4, const SepLayer& L5, float* out,
                             int windows, hipStream_t stream) {
    if (windows <= 0 || !l4_window_planes_supported(L3, L4, L5)) return false;
    const float* const X = static_cast<const float*>(planes);
    if (L4.pw_mode == 2) launch_l4_window_form<true, true>(X, &L3, L4, L5, out, windows, stream);
    else launch_l4_window_form<false, true>(X, &L3, L4, L5, out, windows, stream);
    return true;
}

// launch_separable_fused_next_dw for layer 4 + depthwise 5 (in = the layer-3 output): a window per workgroup
bool launch_l4_window_next_dw(const float* in, float* out, int windows, const SepLayer& L, const SepLayer& next, hipStream_t stream) {
    if (L.stride != 1 || next.stride != 2 || windows <= 0 || L.h_out * L.w_out != 384 || L.w_out != 16 || L.cin != 128 ||
        L.cout != 128 || next.cin != 128)
        return false;
    launch_l4_window(in, L, next, out, windows, stream);
    return true;
}

}  // namespace bd
