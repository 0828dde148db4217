// Layers 1-3 of YAMNet as one kernel, a workgroup per row block (stem3_kernel): the stem of bd_set_fusion stem = 5, and the
// form stem_reg_kernel (stemreg.hip, the default) is tested bit for bit against.
#include "bd_device.h"

namespace bd {

namespace {

// Layers 1-2 (conv 3x3 s2 -> depthwise 3x3 -> pointwise 32 -> 64) and the stride-2 depthwise of layer 3 (yamnet.py:77-80)
// in one kernel, in the arithmetic order of conv1_kernel, depthwise_kernel and the split-f16 pointwise kernel: the layer-2 output
// (the largest tensor of the network, 402 MB per 1024 windows) is never written.  A workgroup owns TWO
// output rows of layer 3's depthwise in one window; they need five layer-2 rows (one is shared with the
// neighbouring workgroup and computed twice), which need seven conv1 rows and fifteen log-mel rows.
//   A  log-mel band -> LDS                       B  conv1 band (7 rows)  -> LDS
//   C  depthwise 2 (5 rows) -> split-f16 A tile   D  [160][32] x [32][64] on the matrix cores
//   E  bias + ReLU -> f32 tile P[160][64] in LDS (rows past the map's edge are the zero padding)
//   F  depthwise 3 (stride 2, SAME = pad 0 before / 1 after) on P -> split-f16 A tile [32][64] in LDS: neither the layer-2
//   output nor the layer-3 depthwise output (100 MB per 1024 windows) touch HBM   G  [32][64] x [64][128] on the matrix cores (wave w:
//   columns 32 w .. 32 w + 31, weights as register fragments from the fragment-order copy)   H  bias + ReLU -> HBM
// Arithmetic order per element equals conv1_kernel / depthwise_kernel / pointwise_f16x3_kernel.
template <bool PLAIN>
__global__ __launch_bounds__(256, 3) void stem3_kernel(const float* __restrict__ logmel, int patch_step,
                                                    const WindowMap map, int w0,
                                                    const float* __restrict__ c1_w, const float* __restrict__ c1_b,
                                                    const float* __restrict__ dw2_w, const float* __restrict__ dw2_b,
                                                    const _Float16* __restrict__ Whi, const _Float16* __restrict__ Wlo,
                                                    const float* __restrict__ pw_u, const float* __restrict__ pw_b,
                                                    const float* __restrict__ dw3_w,
                                                    const float* __restrict__ dw3_b, float* __restrict__ out,
                                                    const _Float16* __restrict__ W3fhi, const _Float16* __restrict__ W3flo,
                                                    const float* __restrict__ pw3_u, const float* __restrict__ pw3_b,
                                                    unsigned* __restrict__ range_flag) {
    float rmax = 0.0f;
    constexpr int R2 = 5;                       // layer-2 rows in the tile
    constexpr int C1R = R2 + 2;                 // conv1 rows incl. halo: 7
    constexpr int LMR = 2 * C1R + 1;            // log-mel rows: 15
    constexpr int BM = R2 * 32;                 // 160 GEMM rows
    constexpr int PW = 68;                      // padded row of the f32 output tile
    // LDS carve-up (50 944 B -> three workgroups per CU): the log-mel band is dead once the conv band exists,
    // so it shares the A tile's bytes; the f32 output tile P overlays everything from phase E on.
    constexpr int OFF_C1 = 0;
    constexpr int OFF_AH = OFF_C1 + C1R * 34 * 32 * 4;              // 30464
    constexpr int OFF_AL = OFF_AH + BM * 64;                        // 40704
    constexpr int P_BYTES = BM * PW * 4;                            // 43520
    constexpr int OFF_A3H = P_BYTES;                                // PW3: layer-3 A tile, [2 halves of 32 k][32 rows][64 B]
    constexpr int OFF_A3L = OFF_A3H + 2 * 32 * 64;
    constexpr int LDS_BYTES = OFF_A3L + 2 * 32 * 64;               // 51712; P aliases from 0
    static_assert(OFF_AL + BM * 64 <= LDS_BYTES, "pipeline buffers must fit");
    static_assert(LMR * 68 * 4 <= 2 * BM * 64, "log-mel band must fit in the A tile it aliases");
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    float (*s_lm)[68] = reinterpret_cast<float (*)[68]>(smem + OFF_AH);
    float (*s_c1)[34][32] = reinterpret_cast<float (*)[34][32]>(smem + OFF_C1);
    char* const s_ah = smem + OFF_AH;
    char* const s_al = smem + OFF_AL;
    float* const P = reinterpret_cast<float*>(smem);               // [BM][PW], valid from phase E on

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int win = blockIdx.y;
    const int ob = blockIdx.x;                  // 0..11: depthwise-3 rows 2 ob, 2 ob + 1
    const int r0 = 4 * ob;                      // first layer-2 row of the tile
    const float* patch = logmel + window_frame(map, w0 + win, patch_step) * BD_MEL_BANDS;

    // this lane's pointwise weight fragments (phase D)
    f16x8 wbh[2], wbl[2];
    {
        const int wrow = (wave & 1) * 32 + (lane & 31);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int koff = (2 * s2 + (lane >> 5)) * 8;
            wbh[s2] = *reinterpret_cast<const f16x8*>(Whi + wrow * 32 + koff);
            wbl[s2] = *reinterpret_cast<const f16x8*>(Wlo + wrow * 32 + koff);
        }
    }

    // every phase's weights are requested one phase ahead (a phase used to begin with a global round trip)
    const int c4 = tid & 7;
    const int col = tid >> 3;
    v4f c1wt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) c1wt[t] = *reinterpret_cast<const v4f*>(c1_w + t * 32 + c4 * 4);
    const v4f c1bias = *reinterpret_cast<const v4f*>(c1_b + c4 * 4);
    // ---- A: log-mel rows 2 (r0 - 1) .. +14, zero halo columns of the conv1 band ----
    for (int i = tid; i < LMR * 17; i += 256) {
        const int j = i / 17, q = i % 17;
        const int ih = 2 * r0 - 2 + j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < 16 && ih >= 0 && ih < BD_PATCH_FRAMES) v = reinterpret_cast<const float4*>(patch + ih * BD_MEL_BANDS)[q];
        *reinterpret_cast<float4*>(&s_lm[j][q * 4]) = v;
    }
    for (int i = tid; i < C1R * 2 * 8; i += 256) {
        const int r = i / 16, side = (i >> 3) & 1, c4 = i & 7;
        *reinterpret_cast<float4*>(&s_c1[r][side ? 33 : 0][c4 * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();

    // ---- B: conv1 rows r0 - 1 .. r0 + 5 ----
    // (consecutive conv1 rows share a log-mel row: a rolling window reads 45 values instead of 63; the four
    //  channels of a tap are two packed fmas)
    v4f d2wt[9];                                // depthwise-2 taps: in flight during the conv1 phase
#pragma unroll
    for (int t = 0; t < 9; ++t) d2wt[t] = *reinterpret_cast<const v4f*>(dw2_w + t * 32 + c4 * 4);
    const v4f d2bias = *reinterpret_cast<const v4f*>(dw2_b + c4 * 4);
    {
        const v4f (&wt)[9] = c1wt;
        const v4f bias = c1bias;
        // a tap row past the patch (log-mel row 96: SAME padding) is skipped, as conv1_kernel does; only the
        // last row block of a window can meet one, so the check lives in its own copy of the loop
        // (as a per-tap condition the compiler turns it into 252 selects)
#define BD_STEM3_CONV1(CHECK)                                                                             \
    {                                                                                                     \
        float lm[3][3];                                                                                   \
        const v4f zero4 = {0.f, 0.f, 0.f, 0.f};                                                           \
        _Pragma("unroll") for (int kw = 0; kw < 3; ++kw) lm[0][kw] = s_lm[0][2 * col + kw];               \
        _Pragma("unroll") for (int i = 0; i < C1R; ++i) {                                                 \
            const int c1r = r0 - 1 + i;                                                                   \
            _Pragma("unroll") for (int kh = 1; kh < 3; ++kh)                                              \
                _Pragma("unroll") for (int kw = 0; kw < 3; ++kw) lm[kh][kw] = s_lm[2 * i + kh][2 * col + kw]; \
            if (!(CHECK) || (c1r >= 0 && c1r < 48)) {   /* the same for the whole workgroup: a scalar branch */ \
                v4f acc = bias;                                                                           \
                _Pragma("unroll") for (int kh = 0; kh < 3; ++kh) {                                        \
                    if (CHECK && 2 * c1r + kh >= BD_PATCH_FRAMES) continue;                               \
                    _Pragma("unroll") for (int kw = 0; kw < 3; ++kw) {                                    \
                        const float v = lm[kh][kw];                                                       \
                        acc = __builtin_elementwise_fma(v4f{v, v, v, v}, wt[kh * 3 + kw], acc);           \
                    }                                                                                     \
                }                                                                                         \
                v4f r4;                                                                                   \
                r4.x = fmaxf(acc.x, 0.0f);                                                                \
                r4.y = fmaxf(acc.y, 0.0f);                                                                \
                r4.z = fmaxf(acc.z, 0.0f);                                                                \
                r4.w = fmaxf(acc.w, 0.0f);                                                                \
                *reinterpret_cast<v4f*>(&s_c1[i][col + 1][c4 * 4]) = r4;                                  \
            } else {                             /* a row above or below the map: the depthwise's zero padding */ \
                *reinterpret_cast<v4f*>(&s_c1[i][col + 1][c4 * 4]) = zero4;                               \
            }                                                                                             \
            _Pragma("unroll") for (int kw = 0; kw < 3; ++kw) lm[0][kw] = lm[2][kw];                       \
        }                                                                                                 \
    }
        // (only the first and the last row block of a window have conv1 rows outside the map or tap rows outside the patch)
        if (ob == 0 || 2 * (r0 + C1R - 2) + 2 >= BD_PATCH_FRAMES || r0 + C1R - 2 >= 48) BD_STEM3_CONV1(true)
        else BD_STEM3_CONV1(false)
#undef BD_STEM3_CONV1
    }
    __syncthreads();

    // ---- C: depthwise 2 for rows r0 .. r0 + 4 -> split-f16 A tile [160][32] ----
    // (rolling window over the conv1 band: 21 LDS reads instead of 45)
    {
        const v4f (&wt)[9] = d2wt;
        const v4f bias = d2bias;
        v4f cv[3][3];
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) cv[kh][kw] = *reinterpret_cast<const v4f*>(&s_c1[kh][col + kw][c4 * 4]);
#pragma unroll
        for (int r = 0; r < R2; ++r) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) cv[2][kw] = *reinterpret_cast<const v4f*>(&s_c1[r + 2][col + kw][c4 * 4]);
            v4f acc = bias;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) acc = __builtin_elementwise_fma(cv[kh][kw], wt[kh * 3 + kw], acc);
            acc.x = fmaxf(acc.x, 0.0f);
            acc.y = fmaxf(acc.y, 0.0f);
            acc.z = fmaxf(acc.z, 0.0f);
            acc.w = fmaxf(acc.w, 0.0f);
            rmax = range_of(rmax, acc);
            f16x4 hi, lo;
            split_f16(acc.x, acc.y, acc.z, acc.w, hi, lo);
            const int off = swz64(r * 32 + col, c4 >> 1) + (c4 & 1) * 8;
            *reinterpret_cast<f16x4*>(s_ah + off) = hi;
            *reinterpret_cast<f16x4*>(s_al + off) = lo;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                cv[0][kw] = cv[1][kw];
                cv[1][kw] = cv[2][kw];
            }
        }
    }
    __syncthreads();

    v4f d3wt[9];                                // depthwise-3 taps (channels 4 (tid & 15) ..): in flight during D and E
#pragma unroll
    for (int t = 0; t < 9; ++t) d3wt[t] = *reinterpret_cast<const v4f*>(dw3_w + t * 64 + (tid & 15) * 4);
    const v4f d3bias = *reinterpret_cast<const v4f*>(dw3_b + (tid & 15) * 4);
    // ---- D: GEMM.  Waves (wr, wc): column tile wc; row tiles wr, wr + 2 and, for wr == 0, 4 ----
    const int wr = wave >> 1, wc = wave & 1;
    const int frow = lane & 31, fh = lane >> 5;
    f32x16 acc2[3];                             // (the first MFMA of a tile takes a literal zero: no 48 moves to clear them)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int rt = wr + 2 * i;                                  // row tile 0..4 (5 = none)
            if (rt < R2) {
                const int off = swz64(rt * 32 + frow, 2 * s2 + fh);
                const f16x8 ah = *reinterpret_cast<const f16x8*>(s_ah + off);
                const f16x8 al = *reinterpret_cast<const f16x8*>(s_al + off);
                f32x16 c = acc2[i];
                if (s2 == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) c[r] = 0.0f;
                }
                // operands swapped: the accumulators hold the TRANSPOSED tile (lane = position, four consecutive
                // channels per register quad), so phase E writes 16 bytes at a time; same products, same k order
                if constexpr (!PLAIN) {
                    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(wbh[s2], al, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(wbl[s2], ah, c, 0, 0, 0);
                }
                acc2[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wbh[s2], ah, c, 0, 0, 0);
            }
        }
    }
    __syncthreads();   // every wave is done with the A tile, the conv band and the log-mel band: P may overwrite them

    // ---- E: bias + ReLU -> P; layer-2 rows past row 47 are the depthwise's zero padding ----
    {
        // transposed accumulators: lane -> position rt * 32 + frow; registers 4 g .. 4 g + 3 -> channels
        // wc * 32 + 8 g + 4 fh + (0..3)
        v4f b4[4], u4[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            b4[g] = *reinterpret_cast<const v4f*>(pw_b + wc * 32 + 8 * g + 4 * fh);
            u4[g] = *reinterpret_cast<const v4f*>(pw_u + wc * 32 + 8 * g + 4 * fh);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int rt = wr + 2 * i;
            if (rt < R2) {
                const bool live = __builtin_amdgcn_readfirstlane((int)(r0 + rt < 48)) != 0;    // the same for the whole wave
                float* prow = P + (rt * 32 + frow) * PW + wc * 32 + 4 * fh;
                if (live) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        // (vector fma: two v_pk_fma_f32 instead of four v_fma_f32; the same IEEE operations)
                        v4f v = __builtin_elementwise_fma(v4f{acc2[i][4 * g + 0], acc2[i][4 * g + 1], acc2[i][4 * g + 2], acc2[i][4 * g + 3]},
                                                          u4[g], b4[g]);
                        v.x = fmaxf(v.x, 0.0f);
                        v.y = fmaxf(v.y, 0.0f);
                        v.z = fmaxf(v.z, 0.0f);
                        v.w = fmaxf(v.w, 0.0f);
                        *reinterpret_cast<v4f*>(prow + 8 * g) = v;
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g) *reinterpret_cast<v4f*>(prow + 8 * g) = v4f{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
    }
    __syncthreads();

    f16x8 w3h[4], w3l[4];                       // this lane's layer-3 weight fragments, k16 steps 0..3 (in flight during F)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const size_t f = ((size_t)(wave * 4 + q) * 64 + lane) * 8;
        w3h[q] = *reinterpret_cast<const f16x8*>(W3fhi + f);
        w3l[q] = *reinterpret_cast<const f16x8*>(W3flo + f);
    }
    // ---- F: depthwise 3, stride 2: out[o][ow][c] from P rows 2o + kh, columns 2ow + kw (column 32 = padding) ----
    // 512 tasks: o (2) x ow (16) x c4 (16); a thread keeps its column and channels in both (o = it).  Every tap is an
    // immediate offset from one pointer; the tap right of column 31 (ow = 15, kw = 2) is read like the others and replaced by
    // the zero padding afterwards (what it reads - the next row, or for the last one the bytes after P - is never used)
    const int c16 = tid & 15, ow = (tid >> 4) & 15;
    const float* const pcol = P + (2 * ow) * PW + c16 * 4;
    const bool right_edge = ow == 15;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int o = it;
        v4f acc = d3bias;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                v4f v = *reinterpret_cast<const v4f*>(pcol + ((2 * o + kh) * 32 + kw) * PW);
                if (kw == 2) {
                    v.x = right_edge ? 0.0f : v.x;
                    v.y = right_edge ? 0.0f : v.y;
                    v.z = right_edge ? 0.0f : v.z;
                    v.w = right_edge ? 0.0f : v.w;
                }
                acc = __builtin_elementwise_fma(v, d3wt[kh * 3 + kw], acc);
            }
        acc.x = fmaxf(acc.x, 0.0f);
        acc.y = fmaxf(acc.y, 0.0f);
        acc.z = fmaxf(acc.z, 0.0f);
        acc.w = fmaxf(acc.w, 0.0f);
        rmax = range_of(rmax, acc);
        f16x4 hi, lo;
        split_f16(acc.x, acc.y, acc.z, acc.w, hi, lo);
        const int c = c16 & 7;
        const int off = (c16 >> 3) * 32 * 64 + swz64(o * 16 + ow, c >> 1) + (c & 1) * 8;
        *reinterpret_cast<f16x4*>(smem + OFF_A3H + off) = hi;
        *reinterpret_cast<f16x4*>(smem + OFF_A3L + off) = lo;
    }
    {
        __syncthreads();
        // ---- G: [32][64] x [64][128], one 32 x 32 tile per wave ----
        f32x16 acc3;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc3[r] = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int off = (q >> 1) * 32 * 64 + swz64(frow, 2 * (q & 1) + fh);
            const f16x8 ah = *reinterpret_cast<const f16x8*>(smem + OFF_A3H + off);
            const f16x8 al = *reinterpret_cast<const f16x8*>(smem + OFF_A3L + off);
            if constexpr (!PLAIN) {
                acc3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, w3h[q], acc3, 0, 0, 0);
                acc3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, w3l[q], acc3, 0, 0, 0);
            }
            acc3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, w3h[q], acc3, 0, 0, 0);
        }
        // ---- H: bias + ReLU, [32][128] block of the layer-3 output (rows are consecutive NHWC positions) ----
        float* dst3 = out + (((size_t)win * 24 + 2 * ob) * 16) * 128;
        const int n = 32 * wave + frow;
        const float b = pw3_b[n], u = pw3_u[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 4 * fh + (r & 3) + 8 * (r >> 2);
            const v2f t2 = __builtin_elementwise_fma(v2f{acc3[r & ~1], acc3[r | 1]}, v2f{u, u}, v2f{b, b});   // one v_pk_fma_f32 per two outputs
            dst3[(size_t)m * 128 + n] = fmaxf((r & 1) ? t2.y : t2.x, 0.0f);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    range_report(rmax, range_flag);
}

}  // namespace

// Layers 1-3 complete: out = [windows][24][16][128], the layer-3 output.
void launch_stem4(const float* logmel, int patch_step, const WindowMap& map, int w0, int windows, const float* c1_w,
                  const float* c1_b, const SepLayer& L2, const SepLayer& L3, float* out, hipStream_t stream) {
    if (windows <= 0) return;
#define BD_STEM4(PLAIN)                                                                                              \
    hipLaunchKernelGGL((stem3_kernel<PLAIN>), dim3(12, windows), dim3(256), 0, stream, logmel, patch_step, map, w0,   \
                       c1_w, c1_b, dw_w_of(L2), dw_b_of(L2), static_cast<const _Float16*>(L2.pw_whi),                     \
                       static_cast<const _Float16*>(L2.pw_wlo), L2.pw_u, L2.pw_b, dw_w_of(L3), dw_b_of(L3), out,            \
                       static_cast<const _Float16*>(L3.pw_fhi), static_cast<const _Float16*>(L3.pw_flo), L3.pw_u, L3.pw_b,  \
                       L2.range_flag)
    if (L2.pw_mode == 2) BD_STEM4(true);
    else BD_STEM4(false);
#undef BD_STEM4
}

}  // namespace bd
