// Layers 8-11 of YAMNet (yamnet.py:86-89: four separable layers of ONE shape, 512 -> 512 channels on the 6 x 4 map, stride 1)
// as one launch in which only the run's first input and last output touch global memory (round 5; VERDICT r4 next #1a).
//
// The hand-off between two layers is a [96 rows = 4 windows][512] tile: 196 KB as f32 or as the next layer's (hi, lo) f16
// operand - more than the CU's 160 KB of LDS.  It does fit the CU when the register file carries part of it:
//
//   * 8 waves, two per SIMD, 256 VGPRs each, all of one kind (no producer waves).  Wave w owns the output columns of the
//     32-column blocks w and w + 8: 3 row tiles x 2 column tiles of v_mfma_f32_32x32x16_f16 = 96 accumulator registers.
//   * At the end of a layer the accumulators ARE the tile: lane (c, h) holds column c and, per 32-row tile, rows
//     {0-3, 8-11, 16-19, 24-27} + 4 h, i.e. the even (h = 0) or odd (h = 1) rows of the stacked 24 x 4 map of the four windows.
//     One v_permlane32_swap per register pair trades the odd rows of windows 0-1 against the even rows of windows 2-3, after
//     which lane (c, h) holds windows 2 h and 2 h + 1 of channel c completely: the next layer's depthwise 3 x 3 runs in
//     registers with compile-time neighbours (no LDS tap reads, no slab, no padding tests), two windows at a time in
//     v_pk_fma_f32.  Taps and shift are per-lane values (one channel per lane): ten global dwords per column block.
//   * Its outputs, split into f16 hi + lo, are the next layer's A operand: stage s (32 input channels) of the K loop is the
//     column block s of the previous layer, so wave w publishes stages w and w + 8 into an LDS ring of 13 stage tiles
//     (13 x 12.1 KB = 157.6 KB); stages 13-15 stay PENDING in the registers of waves 5-7 (48 packed dwords each) until stages
//     0-2 have been consumed, and then take their slots.  Four workgroup barriers per layer (tile published / slots 0-2
//     free / pending published / tile consumed) instead of one per stage: between them the eight waves drift freely and two
//     matrix waves per SIMD cover each other's LDS and L2 latency.  Round 9: the older wave of a SIMD (0-3) takes the
//     tile-consumed barrier behind its depthwise, the younger one (4-7), which leaves the K loop last, in front of it: the
//     older waves publish while the younger ones compute.
//   * Weights as in the 12-wave kernel of rounds 2-5: B fragments straight from the fragment-ordered copy (L2) into registers, two k16 steps
//     ahead.
//
// Arithmetic is that of depthwise_kernel + pointwise_f16x3_kernel bit for bit: the depthwise sums shift +
// taps in row-major tap order with fmaf, ReLU, the split, and per accumulator the products lo*hi, hi*lo, hi*hi of k16 step
// q = 0..31 in ascending order; which wave owns which column block changes nothing.  Taps that fall outside the map are skipped
// instead of multiplied by zero: fma(0, w, a) == a for every a but -0.0, and a sum that starts at a float shift is never -0.0
// unless the shift is (then the result differs in the sign of a zero that the ReLU absorbs).
#include "bd_device.h"

namespace bd {

namespace {

// LDS images of one stage's A tile, both inside a slot of kChipSlotBytes (13 slots = 161 408 B):
//   * the ROW image, pointwise 7's operand only (its LDS-DMA fills it): two halves (hi, lo) of [96 rows][32 k] f16 = 64-byte
//     rows, the 16-byte slot of a row XORed with (row >> 2) & 3 (the 8 rows a ds_read_b128 lane group touches land in different
//     banks), rows 48.. pushed back by one row;
//   * the CHANNEL-MAJOR image (round 10, bd_device.h), every tile a layer publishes from its accumulators: two halves of
//     [32 k][96 rows], 192-byte k-rows, 8-byte chunks XORed with (k >> 1) & 7, 12 288 B.  A lane (one channel, 48 consecutive
//     tile rows) packs hi and lo along the rows as it splits them and writes 12 + 12 ds_write_b64 per column block where 96
//     ds_write_b16 stood (1536 -> 384 wave-level writes per layer and tile); the K loop takes a fragment back with two
//     ds_read_b64_tr_b16.  Both sides are free of bank conflicts (static_asserts in bd_device.h).  The barrier that frees the
//     ring separates the two images.  Values, split, range guard, k order and MFMA operands are those of the row image.
constexpr int kChipHalfBytes = 97 * 64;
constexpr int kChipSlotBytes = 2 * kChipHalfBytes;

constexpr int kChipMaxLayers = 5;
struct ChipChain {
    const float* dw_w[kChipMaxLayers];          // [9][512] depthwise taps * bn scale * 2^act_exp ([512] shift behind them)
    const float* dw_b[kChipMaxLayers];          // [512]
    const _Float16* whi[kChipMaxLayers];        // pointwise weights, MFMA B-fragment order [512/32][512/16][64][8]
    const _Float16* wlo[kChipMaxLayers];
    const float* pw_u[kChipMaxLayers];          // [512] epilogue factors
    const float* pw_b[kChipMaxLayers];          // [512]
    const float* ndw_w;                         // NDW: taps [9][512] + shift [512] of the stride-2 depthwise behind the run
    const _Float16 *w7hi, *w7lo;                // PW7: pointwise 7's weights, B-fragment order [512/32][256/16][64][8]
    const float *u7, *b7;                       // PW7: its epilogue factors / shifts [512]
};
// Pointer `field` of layer `li`, read from the kernel-argument segment with a scalar load (the chain is the kernel's FIRST
// argument, i.e. at offset 0).  Indexing the by-value argument with a run-time layer makes a scratch copy of it; selecting
// among its 30 pointers keeps all of them in scalar registers for the whole kernel (144 of them spilled to lanes).
template <typename T>
__device__ __forceinline__ const T* chain_ptr(int field, int li) {
    typedef const __attribute__((address_space(4))) unsigned long long* kptr;
    const kptr ka = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
    return reinterpret_cast<const T*>(ka[field * kChipMaxLayers + li]);
}
static_assert(sizeof(ChipChain) == (6 * kChipMaxLayers + 5) * 8, "six tables of five pointers + five");

// NDW (layer 12 closes the run and layer 13 is a stride-2 layer): the run's output is not written; layer 13's depthwise
// (3 x 3, stride 2, SAME = pad 0 before / 1 after on the 6 x 4 map: outputs 3 x 2) is applied to it in registers - after the
// same half-wave swap as between the layers a lane holds whole windows of its channel - and only [windows][3][2][512] goes
// to Y: the arithmetic of depthwise_kernel (shift, then the taps in row-major order with fmaf, ReLU).
// PLANES (with NDW): the depthwise-13 output leaves as the two f16 halves the tail's matrix kernel reads (septail.hip): hi plane
// [windows * 6][512] at Y, lo plane behind it - the split and the range guard of the kernel that would otherwise read it as f32.
// PW7: the run opens with pointwise 7 (256 -> 512) instead of reading its output: X is then the split-f16 depthwise-7 output
// sep_mid_kernel<.., DW7OUT> writes (kDw7PlaneBytes per window).  The eight stages of that A operand come in by LDS-DMA
// (buffer_load_dwordx4 ... lds): a DMA lane reads any address, so the ring's swizzle, the 64-byte skew of rows 48.. and the
// tile's row order are all chosen on the address side, with no registers in between.  Pointwise 7 then is one more layer of
// the run with K = 256 (8 stages: no pending ones), its epilogue and the step to depthwise 8 those of every other layer, and
// its arithmetic is that of the layer-7 loop it replaces (sepmid.hip): lo*hi, hi*lo, hi*hi per k16 step in ascending order,
// relu(fma(acc, u, b)).
template <bool PLAIN, int NSLOT, bool TRACE = false, bool NDW = false, bool PLANES = false, bool PW7 = false>
__global__ __launch_bounds__(512, 2) void sep_chip_kernel(const ChipChain ch, const float* X, float* Y, int nl,
                                                           long long M, unsigned* __restrict__ range_flag,
                                                           unsigned long long* __restrict__ dbg = nullptr, int tune = 0) {
    static_assert(NSLOT >= 9 && NSLOT <= 16, "ring size");
    constexpr int K = 512, KQ = K / 16;
    constexpr int NPEND = 16 - NSLOT;              // stages that wait in registers; their owners are waves 8 - NPEND .. 7
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wc = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fh = lane >> 5;
    const long long m0 = (long long)blockIdx.x * 96;
    float rmax = 0.0f;
    // developer aid (-DBD_KERNEL_TRACE build, BD_WS_TRACE=7): shader-clock stamps of waves 0 and 5 of workgroup 0 at every phase edge
    int tsn = 0;
#define CHIP_TS()                                                                                         \
    if constexpr (TRACE) {                                                                                \
        if (blockIdx.x == 0 && lane == 0 && (wc == 0 || wc == 5) && tsn < 64)                             \
            dbg[(wc == 5 ? 64 : 0) + tsn] = __builtin_amdgcn_s_memtime();                                 \
        ++tsn;                                                                                            \
    }
    CHIP_TS()

    // publisher (channel-major image, bd_device.h): lane (frow = k, fh) writes k-row frow, chunks 12 fh + j (tile rows 48 fh + 4 j
    // .. + 3), 8 bytes per half and write; wk0 = the row's key in byte units
    const int wk0 = ((frow >> 1) & 7) << 3;
    // reader of pointwise 7's A operand (the ROW image its LDS-DMA fills: 64-byte rows [row][32 k], 16-byte slots XORed with
    // (row >> 2) & 3, rows 48.. one row further): lane (frow, fh) supplies A[row 32 i + frow][k = 16 s + 8 fh ..] from slot
    // (2 s + fh) ^ key, key = (row >> 2) & 3 =
    // (frow >> 2) & 3 for every i; s = 1 is the s = 0 address with bit 5 flipped.  Row tile 2 is row tile 0 + 4096 + 64 (an
    // immediate); row tile 1 straddles row 48 (the 64-byte skew starts at frow = 16) and keeps its own register.
    const int ra0 = frow * 64 + ((fh ^ ((frow >> 2) & 3)) << 4);
    const int ra1 = ra0 + 2048 + (frow >= 16 ? 64 : 0);
    // reader of every other layer (channel-major image): the two transposed sub-reads of a fragment; k16 step and row tile are
    // immediates (bd_device.h)
    const int rt0 = tr_read_lane_off(lane), rt1 = tr_read_next(rt0);
    const unsigned lane16 = lane * 16, c4 = frow * 4;

    f32x16 acc[3][2];
    unsigned pend[48], out0[48];

    // Depthwise 3 x 3 + shift + ReLU + split of column block J (stage ST) of the tile held as in2[y][x] = (window 2 fh,
    // window 2 fh + 1) at map position (y, x) of channel c: 48 outputs per lane, published into slot ST of the ring, or -
    // always for J = 1, only waves 8 - NPEND .. 7 use them - kept in pend[]: 24 dwords of hi pairs, then 24 of lo pairs.
#define CHIP_DW(J, ST, TAPS)                                                                              \
    {                                                                                                     \
        float wt[9];                                                                                      \
        _Pragma("unroll") for (int t = 0; t < 9; ++t)                                                     \
            wt[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(TAPS, c4, (t * K + 32 * (ST)) * 4, 0)); \
        const float shift = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(TAPS, c4, (9 * K + 32 * (ST)) * 4, 0)); \
        _Pragma("unroll") for (int y = 0; y < 6; ++y)                                                     \
            _Pragma("unroll") for (int xp = 0; xp < 2; ++xp) {                                            \
                v2f a[2];                                                                                 \
                _Pragma("unroll") for (int d = 0; d < 2; ++d) {                                           \
                    const int x = 2 * xp + d;                                                             \
                    a[d] = v2f{shift, shift};                                                             \
                    _Pragma("unroll") for (int kh = 0; kh < 3; ++kh)                                      \
                        _Pragma("unroll") for (int kw = 0; kw < 3; ++kw) {                                \
                            const int iy = y + kh - 1, ix = x + kw - 1;                                   \
                            if (iy < 0 || iy >= 6 || ix < 0 || ix >= 4) continue;                         \
                            a[d] = __builtin_elementwise_fma(in2[iy][ix], v2f{wt[kh * 3 + kw], wt[kh * 3 + kw]}, a[d]); \
                        }                                                                                 \
                }                                                                                         \
                _Pragma("unroll") for (int w = 0; w < 2; ++w) {                                           \
                    const float v0 = fmaxf(w ? a[0].y : a[0].x, 0.0f), v1 = fmaxf(w ? a[1].y : a[1].x, 0.0f); \
                    const f16x2 h_ = {(_Float16)v0, (_Float16)v1};    /* hi of two neighbours along the tile's rows, packed */ \
                    const unsigned hi_ = __builtin_bit_cast(unsigned, h_);                                \
                    unsigned lo_;                                                                         \
                    /* lo halves = f16(v - hi) and the range guard's running maximum, in ONE ordered statement: as a plain */ \
                    /* fmaxf chain the compiler sums the maxima up at the end and keeps (spills) all 48 values until then */ \
                    asm volatile("v_fma_mixlo_f16 %0, %2, -1.0, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"  \
                                 "v_fma_mixhi_f16 %0, %2, -1.0, %4 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"  \
                                 "v_max_f32 %1, %1, %3\n\tv_max_f32 %1, %1, %4"                           \
                                 : "=&v"(lo_), "+v"(rmax) : "v"(hi_), "v"(v0), "v"(v1));                  \
                    const int ci = 2 * (6 * w + y) + xp;    /* rows 48 fh + 24 w + 4 y + 2 xp, + 1: dword xp of chunk 12 fh + 6 w + y */ \
                    if ((J) == 1) { pend[ci] = hi_; pend[24 + ci] = lo_; }                                \
                    else { out0[ci] = hi_; out0[24 + ci] = lo_; }                                         \
                }                                                                                         \
            }                                                                                             \
    }
    // ... and their publication: column block 0 (stage wc) always, column block 1 (stage wc + 8) when its slot exists now
#define CHIP_PUBLISH()                                                                                    \
    {                                                                                                     \
        int wkl = wk0;       /* the address variants are formed per use: as values of the whole kernel they were spilled */ \
        asm volatile("" : "+v"(wkl));                      /* and reloaded behind vmcnt(0) waits */       \
        char* const slot0 = sm + wc * kChipSlotBytes + frow * kTrRowBytes;                                \
        _Pragma("unroll") for (int j = 0; j < 12; ++j) CHIP_PUT(slot0, j, out0)                           \
        if (wc + 8 < NSLOT) {                     /* one wave-uniform branch */                           \
            char* const slot1 = sm + (wc + 8) * kChipSlotBytes + frow * kTrRowBytes;                      \
            _Pragma("unroll") for (int j = 0; j < 12; ++j) CHIP_PUT(slot1, j, pend)                       \
        }                                                                                                 \
    }
    // chunk 12 fh + J of this lane's k-row: hi and lo, one ds_write_b64 each
#define CHIP_PUT(ROW, J, PK)                                                                              \
    {                                                                                                     \
        char* const p_ = (ROW) + ((96 * fh + 8 * (J)) ^ wkl);                                             \
        *reinterpret_cast<u32x2*>(p_) = u32x2{PK[2 * (J)], PK[2 * (J) + 1]};                              \
        *reinterpret_cast<u32x2*>(p_ + kTrHalfBytes) = u32x2{PK[24 + 2 * (J)], PK[25 + 2 * (J)]};         \
    }
    // taps [9][512] and shift [512] of a layer are one [10][512] table (weights_fold.hip lays dw_b16 behind dw_w16; the launcher checks)
#define CHIP_TAPS_RSRC(DW_W) __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(DW_W), 0, 10 * K * 4, 0x00020000)

    // ---------------------------------------------------------------------- the K loop of one layer (KQ_C: k16 steps), the
    // weights WHI / WLO in B-fragment order; leaves the layer's product in acc
    // row_c: the A operand lies in the ROW image (pointwise 7's, filled by LDS-DMA) and is read with ds_read_b128; otherwise in
    // the channel-major image the layers publish, read transposed
    auto k_loop = [&](auto kq_c, auto row_c, const _Float16* const Wfhi, const _Float16* const Wflo) __attribute__((always_inline)) {
        constexpr int KQL = decltype(kq_c)::value;
        constexpr bool ROWIMG = decltype(row_c)::value;
        constexpr int NS = KQL / 2;               // stages
        constexpr int NP = NS > NSLOT ? NS - NSLOT : 0;    // of which pending
        static_assert(NP == 0 || NP == NPEND, "a layer of K = 512 or one that fits the ring");
        // B fragments: column tile (wc, wc + 8), k16 step q -> ((tile * KQ + q) * 64 + lane) * 16 bytes: resource + lane * 16 in
        // one register + a scalar offset.  The first k16 step's are requested in FRONT of the barrier that publishes the A
        // operand (round 6): behind it all eight waves would wait out the same L2 round trip at once
        const __amdgpu_buffer_rsrc_t bhr = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(Wfhi), 0, 16 * KQL * K * 2, 0x00020000);
        const __amdgpu_buffer_rsrc_t blr = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(Wflo), 0, 16 * KQL * K * 2, 0x00020000);
        const int btile = wc * (KQL * 1024);      // bytes of a column tile's fragments: KQ k16 steps of 1 KB
        constexpr int jstep = 8 * KQL * 1024;     // bytes between column tiles wc and wc + 8
        f16x8 bh0[2], bl0[2], bh1[2], bl1[2];
#define CHIP_LB(R, B, Q, J) B[J] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(R, lane16, btile + (J) * jstep + (Q) * 1024, 0));
#define CHIP_BLOAD(BH, BL, Q) { CHIP_LB(bhr, BH, Q, 0) CHIP_LB(blr, BL, Q, 0) CHIP_LB(bhr, BH, Q, 1) CHIP_LB(blr, BL, Q, 1) }
        CHIP_BLOAD(bh0, bl0, 0)
        __syncthreads();                          // stages 0 .. NSLOT - 1 of the layer published
        CHIP_TS()

        // (a zero the compiler cannot form early: as plain constants the 96 clears were hoisted above the barrier into the
        //  depthwise phase, where the accumulators' registers are what its 96 results live in - 43 spills)
        float zero;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = zero;
        // ---- the K loop.  One stage = 6 steps (k16 step s = 0, 1 x row tile i = 0..2) of 6 MFMAs (2 in the plain-f16 mode).
        // Every memory request sits in its own MFMA gap, pinned there by a scheduling barrier (left alone the compiler
        // bunches the four B loads of a k16 step at the top of the stage - an in-order wave then issues no MFMA while they
        // go out - and sinks the A reads to just before their use):
        //   A fragments   a ring of three (hi, lo) pairs, step t uses pair t mod 3 and requests the pair of step t + 2 (the one
        //                 step t - 1 has finished with): two steps = 12 MFMAs between request and use, across stages too.  In
        //                 the channel-major image a fragment is TWO transposed reads (elements 0-3, 4-7), a pair four requests,
        //                 lo before hi (the step's first MFMA takes lo): they fill the gaps the B loads leave, the last of a
        //                 pair four to five MFMAs before its use at the closest (stage table below), 32 requests in 36 gaps;
        //   B fragments   two sets (k16 step 0 / 1 of a stage); a register is requested again in the gap after the last MFMA
        //                 that reads it, three steps = 18 MFMAs before its next use.
#define CHIP_LAH(A, S, I) A = *reinterpret_cast<const f16x8*>(abase + (((I) == 1 ? ra1 : ra0) ^ ((S) << 5)) + ((I) == 2 ? 4096 + 64 : 0));
#define CHIP_LAL(A, S, I) A = *reinterpret_cast<const f16x8*>(abase + (((I) == 1 ? ra1 : ra0) ^ ((S) << 5)) + ((I) == 2 ? 4096 + 64 : 0) + kChipHalfBytes);
#define CHIP_MF(I, J, A, B) acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B, acc[I][J], 0, 0, 0);
#define CHIP_SB __builtin_amdgcn_sched_barrier(0);
#define CHIP_NOP
        // a step: row tile I against both column tiles; M1 .. M6 = the request (or nothing) that follows each MFMA
#define CHIP_STEP(I, AH, AL, BH, BL, M1, M2, M3, M4, M5, M6)                                              \
    if constexpr (!PLAIN) {                                                                               \
        CHIP_MF(I, 0, AL, BH[0]) M1 CHIP_SB                                                               \
        CHIP_MF(I, 0, AH, BL[0]) M2 CHIP_SB                                                               \
    } else {                                                                                              \
        M1 M2                                                                                             \
    }                                                                                                     \
    CHIP_MF(I, 0, AH, BH[0]) M3 CHIP_SB                                                                   \
    if constexpr (!PLAIN) {                                                                               \
        CHIP_MF(I, 1, AL, BH[1]) M4 CHIP_SB                                                               \
        CHIP_MF(I, 1, AH, BL[1]) M5 CHIP_SB                                                               \
    } else {                                                                                              \
        M4 M5                                                                                             \
    }                                                                                                     \
    CHIP_MF(I, 1, AH, BH[1]) M6 CHIP_SB
#define CHIP_STAGES_ROW(FROM, TO)                                                                           \
    if ((FROM) < (TO)) {                                                                                  \
        f16x8 ah0, al0, ah1, al1, ah2, al2;                                                               \
        const char* abase = sm + ((FROM) < NSLOT ? (FROM) : (FROM) - NSLOT) * kChipSlotBytes;             \
        CHIP_LAH(ah0, 0, 0) CHIP_LAL(al0, 0, 0) CHIP_LAH(ah1, 0, 1) CHIP_LAL(al1, 0, 1)                   \
        _Pragma("nounroll") for (int kk = (FROM); kk < (TO); ++kk) {                                      \
            const int q1 = 2 * kk + 1, q2 = 2 * kk + 2 < KQL ? 2 * kk + 2 : 0;    /* (the last stage re-reads step 0: unused) */ \
            const char* const anext = sm + (kk + 1 < (TO) ? (kk + 1 < NSLOT ? kk + 1 : kk + 1 - NSLOT) : (kk < NSLOT ? kk : kk - NSLOT)) * kChipSlotBytes; \
            CHIP_STEP(0, ah0, al0, bh0, bl0, CHIP_LB(bhr, bh1, q1, 0), CHIP_LB(blr, bl1, q1, 0), CHIP_LB(bhr, bh1, q1, 1),  \
                      CHIP_LB(blr, bl1, q1, 1), CHIP_LAH(ah2, 0, 2), CHIP_LAL(al2, 0, 2))                 \
            CHIP_STEP(1, ah1, al1, bh0, bl0, CHIP_LAH(ah0, 1, 0), CHIP_LAL(al0, 1, 0), CHIP_NOP, CHIP_NOP, CHIP_NOP, CHIP_NOP) \
            CHIP_STEP(2, ah2, al2, bh0, bl0, CHIP_LAH(ah1, 1, 1), CHIP_LAL(al1, 1, 1), CHIP_LB(blr, bl0, q2, 0),            \
                      CHIP_LB(bhr, bh0, q2, 0), CHIP_NOP, CHIP_LB(blr, bl0, q2, 1))                       \
            CHIP_STEP(0, ah0, al0, bh1, bl1, CHIP_LB(bhr, bh0, q2, 1), CHIP_LAH(ah2, 1, 2), CHIP_LAL(al2, 1, 2), CHIP_NOP, CHIP_NOP, CHIP_NOP) \
            abase = anext;         /* the first two steps of the next stage (the same stage again behind the last: unused) */ \
            CHIP_STEP(1, ah1, al1, bh1, bl1, CHIP_LAH(ah0, 0, 0), CHIP_LAL(al0, 0, 0), CHIP_NOP, CHIP_NOP, CHIP_NOP, CHIP_NOP) \
            CHIP_STEP(2, ah2, al2, bh1, bl1, CHIP_LAH(ah1, 0, 1), CHIP_LAL(al1, 0, 1), CHIP_NOP, CHIP_NOP, CHIP_NOP, CHIP_NOP) \
        }                                                                                                 \
    }
        // the same in the channel-major image: ring entry n = (hNa, hNb | lNa, lNb), halves of a fragment
#define CHIP_TR(V, HALF, S, I, R)                                                                         \
    V = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(abase + ((R) ? rt1 : rt0) + 64 * (I) + 16 * kTrRowBytes * (S) + (HALF) * kTrHalfBytes));
#define CHIP_FR(A, B) __builtin_bit_cast(f16x8, __builtin_shufflevector(A, B, 0, 1, 2, 3, 4, 5, 6, 7))
#define CHIP_STAGES_TR(FROM, TO)                                                                          \
    if ((FROM) < (TO)) {                                                                                  \
        s16x4 h0a, h0b, l0a, l0b, h1a, h1b, l1a, l1b, h2a, h2b, l2a, l2b;                                 \
        const char* abase = sm + ((FROM) < NSLOT ? (FROM) : (FROM) - NSLOT) * kChipSlotBytes;             \
        CHIP_TR(l0a, 1, 0, 0, 0) CHIP_TR(l0b, 1, 0, 0, 1) CHIP_TR(h0a, 0, 0, 0, 0) CHIP_TR(h0b, 0, 0, 0, 1) \
        CHIP_TR(l1a, 1, 0, 1, 0) CHIP_TR(l1b, 1, 0, 1, 1) CHIP_TR(h1a, 0, 0, 1, 0) CHIP_TR(h1b, 0, 0, 1, 1) \
        _Pragma("nounroll") for (int kk = (FROM); kk < (TO); ++kk) {                                      \
            const int q1 = 2 * kk + 1, q2 = 2 * kk + 2 < KQL ? 2 * kk + 2 : 0;    /* (the last stage re-reads step 0: unused) */ \
            const char* const anext = sm + (kk + 1 < (TO) ? (kk + 1 < NSLOT ? kk + 1 : kk + 1 - NSLOT) : (kk < NSLOT ? kk : kk - NSLOT)) * kChipSlotBytes; \
            CHIP_STEP(0, CHIP_FR(h0a, h0b), CHIP_FR(l0a, l0b), bh0, bl0, CHIP_LB(bhr, bh1, q1, 0), CHIP_LB(blr, bl1, q1, 0),     \
                      CHIP_LB(bhr, bh1, q1, 1), CHIP_LB(blr, bl1, q1, 1), CHIP_TR(l2a, 1, 0, 2, 0), CHIP_TR(l2b, 1, 0, 2, 1))    \
            CHIP_STEP(1, CHIP_FR(h1a, h1b), CHIP_FR(l1a, l1b), bh0, bl0, CHIP_TR(h2a, 0, 0, 2, 0), CHIP_TR(h2b, 0, 0, 2, 1),     \
                      CHIP_TR(l0a, 1, 1, 0, 0), CHIP_TR(l0b, 1, 1, 0, 1), CHIP_TR(h0a, 0, 1, 0, 0), CHIP_TR(h0b, 0, 1, 0, 1))    \
            CHIP_STEP(2, CHIP_FR(h2a, h2b), CHIP_FR(l2a, l2b), bh0, bl0, CHIP_TR(l1a, 1, 1, 1, 0), CHIP_TR(l1b, 1, 1, 1, 1),     \
                      CHIP_LB(blr, bl0, q2, 0), CHIP_LB(bhr, bh0, q2, 0), CHIP_TR(h1a, 0, 1, 1, 0), CHIP_LB(blr, bl0, q2, 1))    \
            CHIP_STEP(0, CHIP_FR(h0a, h0b), CHIP_FR(l0a, l0b), bh1, bl1, CHIP_LB(bhr, bh0, q2, 1), CHIP_TR(h1b, 0, 1, 1, 1),     \
                      CHIP_TR(l2a, 1, 1, 2, 0), CHIP_TR(l2b, 1, 1, 2, 1), CHIP_TR(h2a, 0, 1, 2, 0), CHIP_TR(h2b, 0, 1, 2, 1))    \
            abase = anext;         /* the first two steps of the next stage (the same stage again behind the last: unused) */ \
            CHIP_STEP(1, CHIP_FR(h1a, h1b), CHIP_FR(l1a, l1b), bh1, bl1, CHIP_TR(l0a, 1, 0, 0, 0), CHIP_TR(l0b, 1, 0, 0, 1),     \
                      CHIP_TR(h0a, 0, 0, 0, 0), CHIP_TR(h0b, 0, 0, 0, 1), CHIP_NOP, CHIP_NOP)                                   \
            CHIP_STEP(2, CHIP_FR(h2a, h2b), CHIP_FR(l2a, l2b), bh1, bl1, CHIP_TR(l1a, 1, 0, 1, 0), CHIP_TR(l1b, 1, 0, 1, 1),     \
                      CHIP_TR(h1a, 0, 0, 1, 0), CHIP_TR(h1b, 0, 0, 1, 1), CHIP_NOP, CHIP_NOP)                                   \
        }                                                                                                 \
    }
#define CHIP_STAGES(FROM, TO)                                                                             \
    if constexpr (ROWIMG) {                                                                               \
        CHIP_STAGES_ROW(FROM, TO)                                                                         \
    } else {                                                                                              \
        CHIP_STAGES_TR(FROM, TO)                                                                          \
    }
        typedef short s16x4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) s16x4* lds4;
        CHIP_STAGES(0, NP)
        CHIP_TS()
        if constexpr (NP > 0) {
            __syncthreads();                      // every wave has read stages 0 .. NPEND - 1: their slots are free
            CHIP_TS()
            if (wc >= 8 - NPEND) {
                char* const slot = sm + (wc + 8 - NSLOT) * kChipSlotBytes + frow * kTrRowBytes;
                int wkl = wk0;
                asm volatile("" : "+v"(wkl));
#pragma unroll
                for (int j = 0; j < 12; ++j) CHIP_PUT(slot, j, pend)
            }
        }
        CHIP_TS()
        // ... and the other waves wait for them HERE, not at stage NSLOT: a wave that publishes beside a neighbour's
        // back-to-back MFMAs gets an LDS write through every ~90 cycles (9 000 cycles for its 96, measured) and everyone
        // waited for it ten stages later; with the whole workgroup at the barrier the 96 writes take ~1 000
        if constexpr (NP > 0) __syncthreads();    // pending stages published
        CHIP_TS()
        CHIP_STAGES(NP, NS)
        CHIP_TS()
#undef CHIP_STAGES
#undef CHIP_STAGES_ROW
#undef CHIP_STAGES_TR
#undef CHIP_TR
#undef CHIP_FR
#undef CHIP_STEP
#undef CHIP_BLOAD
#undef CHIP_LB
#undef CHIP_LAH
#undef CHIP_LAL
#undef CHIP_MF
#undef CHIP_SB
#undef CHIP_NOP
    };

    // ---------------------------------------------------------------------- the step from a layer's product to the next layer's
    // A operand: epilogue (U, B of the layer), the half-wave swap, the depthwise of the next layer (TAPS) on the accumulators,
    // the publication into the ring
    auto next_layer = [&](const float* const taps_w, const float* const pu, const float* const pb) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t taps = CHIP_TAPS_RSRC(taps_w);
        const __amdgpu_buffer_rsrc_t pur = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pu), 0, K * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t pbr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pb), 0, K * 4, 0x00020000);
        if (wc >= 4) __syncthreads();             // (the ring-free barrier of the younger waves: see below)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int st = j ? wc + 8 : wc;       // stage of the next layer = column block of this one
            const float u = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(pur, c4, 128 * st, 0));
            const float b = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(pbr, c4, 128 * st, 0));
            // stacked map row R = 8 i + 2 (r >> 2) + owner half, x = r & 3.  Pair q (rows 2 q, 2 q + 1) of windows 0-1 is
            // accumulator quad (q >> 2, q & 3); the same pair of windows 2-3 is quad ((q + 6) >> 2, (q + 6) & 3).
            float ev[12][4];                      // this lane's two windows, local map rows 0..11
#pragma unroll
            for (int q = 0; q < 6; ++q)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const float a01 = fmaxf(fmaf(acc[q >> 2][j][4 * (q & 3) + x], u, b), 0.0f);
                    const float a23 = fmaxf(fmaf(acc[(q + 6) >> 2][j][4 * ((q + 6) & 3) + x], u, b), 0.0f);
                    // v_permlane32_swap vdst, src: lanes 32-63 of vdst <-> lanes 0-31 of src
                    const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a01),
                                                                    __builtin_bit_cast(unsigned, a23), false, false);
                    ev[2 * q][x] = __builtin_bit_cast(float, (unsigned)r[0]);
                    ev[2 * q + 1][x] = __builtin_bit_cast(float, (unsigned)r[1]);
                }
            v2f in2[6][4];
#pragma unroll
            for (int y = 0; y < 6; ++y)
#pragma unroll
                for (int x = 0; x < 4; ++x) in2[y][x] = v2f{ev[y][x], ev[6 + y][x]};
            if (j == 0) CHIP_DW(0, st, taps)
            else CHIP_DW(1, st, taps)
            CHIP_TS()
        }
        // The barrier that frees the ring stands HERE, behind the depthwise: the two matrix waves of a SIMD do not finish a
        // layer's K loop together (the older one gets the pipe first), and everything above needs only the wave's own
        // accumulators - so the early wave's vector work runs beside the late wave's last MFMAs, and the late wave's has the
        // vector unit to itself, instead of both waiting and then sharing it.  That is so for the OLDER wave of a SIMD (waves
        // 0-3).  The younger one (waves 4-7) leaves the K loop last: it takes its barrier - one per wave either way, in a
        // wave-uniform branch - in front of its depthwise, so that the older waves publish while it computes instead of all
        // eight publishing together behind it.  Correct whichever wave is late in fact.
        if (wc < 4) __syncthreads();              // every wave has read every stage: the ring is free for this layer's tile
        CHIP_TS()
        CHIP_PUBLISH()
    };

    const long long rows_left = M - m0;
    const unsigned tile_bytes = (unsigned)(rows_left < 96 ? rows_left : 96) * (K * 4);
    if constexpr (PW7) {
        // ------------------------------------------------------------------ pointwise 7 on the depthwise-7 planes
        // The 8 ring slots of its A operand are one run of 8 x 12 416 B = 97 x 1 KB pieces; piece n is DMA instruction n / 8 of
        // wave n % 8, lane l of it fills the 16 bytes at 16 (64 n + l).  Those are (stage, half, LDS row rho, slot) of the ring
        // image, and slot p of row rho holds channels 8 (p ^ key) .. + 7, key = (rho >> 2) & 3, of tile row rho = 24 w + 4 oy + ox:
        // window w of the tile.  The resource covers the tile's windows in the batch only: rows past it read as zero, and
        // the 64 bytes in front of row 48 (the skew), and the lo halves in the plain-f16 mode, take an offset outside it.
        const long long w0 = m0 / 24, wleft = M / 24 - w0;
        const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(X)) + (size_t)w0 * kDw7PlaneBytes, 0,
            (unsigned)(wleft < 4 ? wleft : 4) * kDw7PlaneBytes, 0x00020000);
        constexpr int kPieces = 8 * kChipSlotBytes / 1024;
        static_assert(kPieces * 1024 == 8 * kChipSlotBytes && 8 * kChipSlotBytes <= NSLOT * kChipSlotBytes, "whole pieces");
#pragma unroll
        for (int t = 0; t < (kPieces + 7) / 8; ++t) {
            const int n = 8 * t + wc;
            if (n >= kPieces) break;                                  // (wave-uniform)
            const int c = 64 * n + lane;                              // 16-byte unit of the 8 slots
            const int s = c / (kChipSlotBytes / 16), cs = c - s * (kChipSlotBytes / 16);
            const int h = cs >= kChipHalfBytes / 16 ? 1 : 0;
            const int o = (cs - h * (kChipHalfBytes / 16)) * 16;      // byte of the half
            const bool skew = o >= 48 * 64 && o < 49 * 64;
            const int rho = o < 48 * 64 ? o >> 6 : (o - 64) >> 6;
            const int p = (o >> 4) & 3, w = rho / 24;
            const unsigned src = (unsigned)(w * kDw7PlaneBytes + s * (kDw7PlaneBytes / 8) + h * (kDw7PlaneBytes / 16) +
                                            (rho - 24 * w) * 64 + ((p ^ ((rho >> 2) & 3)) << 4));
            const unsigned off = skew || (PLAIN && h) ? 0x7ffffff0u : src;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(pr, (__attribute__((address_space(3))) void*)(sm + n * 1024), 16, off, 0, 0, 0);
        }
        // this wave's pieces have landed.  (All of them: a B load behind a piece cannot be waited for alone - loads complete
        // in order - and the K loop's first step waits for B fragments requested in front of its barrier)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        CHIP_TS()
        k_loop(std::integral_constant<int, 16>{}, std::true_type{}, ch.w7hi, ch.w7lo);
        next_layer(ch.dw_w[0], ch.u7, ch.b7);
    } else {
        // ------------------------------------------------------------------ layer 0: its depthwise reads the run's input
        // through a buffer resource that covers exactly this tile's valid rows: a row past the end of the batch (tail tile)
        // reads as zero, with no clamping code, and every load is resource + one per-lane offset register + a scalar row offset
        const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X) + (size_t)m0 * K, 0, tile_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t taps0 = CHIP_TAPS_RSRC(ch.dw_w[0]);
        const unsigned xo = (48u * fh * K) * 4 + c4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int st = j ? wc + 8 : wc;
            v2f in2[6][4];
#pragma unroll
            for (int y = 0; y < 6; ++y)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    in2[y][x].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, xo, ((4 * y + x) * K + 32 * st) * 4, 0));
                    in2[y][x].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, xo, ((24 + 4 * y + x) * K + 32 * st) * 4, 0));
                }
            if (j == 0) CHIP_DW(0, st, taps0)
            else CHIP_DW(1, st, taps0)
            CHIP_TS()
            __builtin_amdgcn_sched_barrier(0);    // (the second block's 48 loads hoisted over the first's sums cost a spill)
        }
        CHIP_PUBLISH()
    }

    for (int li = 0; li < nl; ++li) {
        // ------------------------------------------------------------------ 1 x 1 convolution of layer li
        k_loop(std::integral_constant<int, KQ>{}, std::false_type{}, chain_ptr<_Float16>(2, li), chain_ptr<_Float16>(3, li));
        if (li + 1 == nl) break;
        // ------------------------------------------------------------------ depthwise of layer li + 1 on the accumulators
        next_layer(chain_ptr<float>(0, li + 1), chain_ptr<float>(4, li), chain_ptr<float>(5, li));
    }
#undef CHIP_DW
#undef CHIP_PUBLISH
#undef CHIP_TAPS_RSRC
#undef CHIP_PUT

    // ---------------------------------------------------------------------- the run's output: bias + ReLU from the accumulators
    // (stores past the tile's valid rows are dropped by the resource's range check: no per-store masks)
    {
        const __amdgpu_buffer_rsrc_t pur = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(chain_ptr<float>(4, nl - 1)), 0, K * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t pbr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(chain_ptr<float>(5, nl - 1)), 0, K * 4, 0x00020000);
        if constexpr (!NDW) {
            const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(Y + (size_t)m0 * K, 0, tile_bytes, 0x00020000);
            const unsigned yo = (4u * fh * K) * 4 + c4;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int st = j ? wc + 8 : wc;
                const float u = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(pur, c4, 128 * st, 0));
                const float b = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(pbr, c4, 128 * st, 0));
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, fmaxf(fmaf(acc[i][j][r], u, b), 0.0f)), yrs, yo,
                                                              ((32 * i + 8 * (r >> 2) + (r & 3)) * K + 32 * st) * 4, 0);
            }
        } else {
            // the tile's windows are rows m0 / 24 .. + 3 of the [windows][6][512] output: 6 output rows per window, a quarter
            // of the tile's bytes
            const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(Y + (size_t)(m0 / 4) * K, 0, tile_bytes / 4, 0x00020000);
            _Float16* const yh = reinterpret_cast<_Float16*>(Y);
            const __amdgpu_buffer_rsrc_t yhr = __builtin_amdgcn_make_buffer_rsrc(yh + (size_t)(m0 / 4) * K, 0, tile_bytes / 8, 0x00020000);
            const __amdgpu_buffer_rsrc_t ylr = __builtin_amdgcn_make_buffer_rsrc(yh + (size_t)(M / 4 + m0 / 4) * K, 0, tile_bytes / 8, 0x00020000);
            const __amdgpu_buffer_rsrc_t ntaps = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ch.ndw_w), 0, 10 * K * 4, 0x00020000);
            const unsigned yo = (12u * fh * K) * 4 + c4;            // this lane's windows 2 fh, 2 fh + 1: output rows 12 fh ..
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int st = j ? wc + 8 : wc;
                const float u = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(pur, c4, 128 * st, 0));
                const float b = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(pbr, c4, 128 * st, 0));
                float wt[9];
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    wt[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ntaps, c4, (t * K + 32 * st) * 4, 0));
                const float shift = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ntaps, c4, (9 * K + 32 * st) * 4, 0));
                float ev[12][4];
#pragma unroll
                for (int q = 0; q < 6; ++q)
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const float a01 = fmaxf(fmaf(acc[q >> 2][j][4 * (q & 3) + x], u, b), 0.0f);
                        const float a23 = fmaxf(fmaf(acc[(q + 6) >> 2][j][4 * ((q + 6) & 3) + x], u, b), 0.0f);
                        const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a01),
                                                                        __builtin_bit_cast(unsigned, a23), false, false);
                        ev[2 * q][x] = __builtin_bit_cast(float, (unsigned)r[0]);
                        ev[2 * q + 1][x] = __builtin_bit_cast(float, (unsigned)r[1]);
                    }
#pragma unroll
                for (int oy = 0; oy < 3; ++oy)
#pragma unroll
                    for (int ox = 0; ox < 2; ++ox) {
                        v2f a = {shift, shift};
#pragma unroll
                        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                            for (int kw = 0; kw < 3; ++kw) {
                                const int iy = 2 * oy + kh, ix = 2 * ox + kw;
                                if (iy >= 6 || ix >= 4) continue;            // SAME padding of a stride-2 layer: one row / column behind the map
                                a = __builtin_elementwise_fma(v2f{ev[iy][ix], ev[6 + iy][ix]}, v2f{wt[kh * 3 + kw], wt[kh * 3 + kw]}, a);
                            }
#pragma unroll
                        for (int w = 0; w < 2; ++w) {
                            const float o = fmaxf(w ? a.y : a.x, 0.0f);
                            if constexpr (PLANES) {
                                unsigned pk = (unsigned)__builtin_bit_cast(unsigned short, (_Float16)o);
                                asm volatile("v_fma_mixhi_f16 %0, %0, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\tv_max_f32 %1, %1, |%2|"
                                             : "+v"(pk), "+v"(rmax) : "v"(o));
                                __builtin_amdgcn_raw_buffer_store_b16((unsigned short)pk, yhr, yo >> 1, ((6 * w + 2 * oy + ox) * K + 32 * st) * 2, 0);
                                if constexpr (!PLAIN)
                                    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(pk >> 16), ylr, yo >> 1,
                                                                          ((6 * w + 2 * oy + ox) * K + 32 * st) * 2, 0);
                            } else {
                                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), yrs, yo,
                                                                      ((6 * w + 2 * oy + ox) * K + 32 * st) * 4, 0);
                            }
                        }
                    }
            }
        }
    }
    range_report(rmax, range_flag);
    if constexpr (TRACE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    CHIP_TS()
#undef CHIP_TS
}

template <bool PLAIN, bool NDW, bool PLANES = false, bool PW7 = false>
void launch_chip(const float* in, float* out, const SepLayer* L, int nl, long long M, const float* ndw_w, hipStream_t stream,
                 const SepLayer* L7 = nullptr) {
    ChipChain ch{};
    if (L7) {
        ch.w7hi = static_cast<const _Float16*>(L7->pw_fhi);
        ch.w7lo = static_cast<const _Float16*>(L7->pw_flo);
        ch.u7 = L7->pw_u;
        ch.b7 = L7->pw_b;
    }
    for (int i = 0; i < nl; ++i) {
        ch.dw_w[i] = dw_w_of(L[i]);
        ch.dw_b[i] = dw_b_of(L[i]);
        ch.whi[i] = static_cast<const _Float16*>(L[i].pw_fhi);
        ch.wlo[i] = static_cast<const _Float16*>(L[i].pw_flo);
        ch.pw_u[i] = L[i].pw_u;
        ch.pw_b[i] = L[i].pw_b;
    }
    ch.ndw_w = ndw_w;
    constexpr int NSLOT = 13;
    constexpr int lds = NSLOT * kChipSlotBytes;
    static_assert(lds <= 160 * 1024, "the ring must fit the CU's LDS");
    allow_dynamic_lds<&sep_chip_kernel<PLAIN, NSLOT, false, NDW, PLANES, PW7>>(lds);
    const long long tiles = (M + 95) / 96;
    int tune = 0;
#ifdef BD_KERNEL_TRACE      // developer build only: BD_CHIP_TUNE = policy under test; BD_WS_TRACE=7 stamps workgroup 0
    if (const char* tn = getenv("BD_CHIP_TUNE")) tune = atoi(tn);
    if (traced_launch(
            '7', &sep_chip_kernel<PLAIN, NSLOT, true, NDW, PLANES, PW7>, lds, stream, 64, 5, nullptr,
            [&](unsigned long long* dbg) {
                hipLaunchKernelGGL((sep_chip_kernel<PLAIN, NSLOT, true, NDW, PLANES, PW7>), dim3((unsigned)tiles), dim3(512), lds, stream, ch, in, out, nl,
                                   M, L[0].range_flag, dbg, tune);
            },
            "on-chip run, wave %d, %d layers%s: cycles between stamps (start | %s | per layer: B1, stages 0-2, B2, pend, B3, stages 3-15, "
            "[dw j0, dw j1, B4] | stores):",
            nl, PW7 ? " + pointwise 7" : "", PW7 ? "DMA, B1, -, -, -, stages 0-7, dw j0, dw j1, B4" : "dw0 j0 j1"))
        return;
#endif
    hipLaunchKernelGGL((sep_chip_kernel<PLAIN, NSLOT, false, NDW, PLANES, PW7>), dim3((unsigned)tiles), dim3(512), lds, stream, ch, in, out, nl, M,
                       L[0].range_flag, (unsigned long long*)nullptr, tune);
}

}  // namespace

// A run of stride-1 512 -> 512 layers on the 6 x 4 map with the tiles between its layers kept on the CU: reads `in`, writes
// `out`.  They may be the same buffer: a workgroup has read all rows of its tile before it writes any.  The caller has
// checked the shapes (launch_separable_run_next_dw below).  With `next` (the stride-2 layer behind the run) the run's output is not written:
// next's depthwise is applied in the epilogue and out = [windows][3][2][512] (then `out` must not be `in`: the tiles' rows
// differ).  False (nothing launched) when a layer's shift table does not follow its taps (the kernel reads both through
// one [10][512] resource; weights_fold.hip lays dw_b16 behind dw_w16).
// planes (with next): the output leaves as f16 hi / lo planes [windows * 6][512] (hi at out, lo behind it), what septail.hip reads.
static bool launch_separable_chip(const float* in, float* out, int windows, const SepLayer* L, int nl, hipStream_t stream,
                                  const SepLayer* next, bool planes) {
    if (planes && !next) return false;
    if (nl < 1 || nl > kChipMaxLayers) return false;
    for (int i = 0; i < nl; ++i)
        if (dw_b_of(L[i]) != dw_w_of(L[i]) + 9 * 512) return false;
    if (next && (dw_b_of(*next) != dw_w_of(*next) + 9 * 512 || next->cin != 512 || next->stride != 2 || in == out)) return false;
    const long long M = (long long)windows * 24;
    const float* nw = next ? dw_w_of(*next) : nullptr;
    if (planes) {
        if (L[0].pw_mode == 2) launch_chip<true, true, true>(in, out, L, nl, M, nw, stream);
        else launch_chip<false, true, true>(in, out, L, nl, M, nw, stream);
        return true;
    }
    if (L[0].pw_mode == 2) {
        if (next) launch_chip<true, true>(in, out, L, nl, M, nw, stream);
        else launch_chip<true, false>(in, out, L, nl, M, nw, stream);
    } else {
        if (next) launch_chip<false, true>(in, out, L, nl, M, nw, stream);
        else launch_chip<false, false>(in, out, L, nl, M, nw, stream);
    }
    return true;
}

// The run of stride-1 512 -> 512 layers on the 6 x 4 map (layers 8-11) extended by the layer that closes it - the stride-1
// 512 -> 512 layer whose successor is a stride-2 one (layer 12) - with that successor's depthwise in the epilogue: layers 8-12 +
// depthwise 13 as ONE launch of the on-chip kernel, a -> b = [windows][3][2][512] (planes: as f16 hi / lo planes,
// what septail.hip reads).  Returns the number of layers of L it ran (5) or 0 (the caller goes on layer by layer).
int launch_separable_run_next_dw(const float* a, float* b, int windows, const SepLayer* L, int max_layers, hipStream_t stream,
                                 bool planes) {
    int n = 0;
    while (n < 5 && n + 1 < max_layers) {
        const SepLayer& l = L[n];
        if (l.stride != 1 || l.cin != 512 || l.cout != 512 || l.h_out != 6 || l.w_out != 4 || l.pw_mode != L[0].pw_mode) return 0;
        ++n;
        if (L[n].stride != 1) break;
    }
    if (n < 2 || n > 5 || n >= max_layers || L[n].stride != 2 || L[n].cin != 512 || windows <= 0 || (long long)windows * 24 >= (1LL << 31))
        return 0;
    return launch_separable_chip(a, b, windows, L, n, stream, &L[n], planes) ? n : 0;
}

// Pointwise 7 (L7) on the depthwise-7 planes sep_mid_kernel<.., DW7OUT> writes (kDw7PlaneBytes per window), then the run L[0 ..
// nl - 1] and next's depthwise, out = the planes septail.hip reads: launch_separable_chip(.., next, planes = true) with the
// run's first input computed on the CU.  Would it run?
bool separable_chip_pw7_supported(const SepLayer& L7, const SepLayer* L, int nl, const SepLayer& next, int windows) {
    if (windows <= 0 || (long long)windows * 24 >= (1LL << 31) || nl < 1 || nl > kChipMaxLayers) return false;
    if (L7.cin != 256 || L7.cout != 512 || L7.h_out != 6 || L7.w_out != 4 || L7.pw_mode == 0 || !L7.pw_fhi || !L7.pw_flo)
        return false;
    for (int i = 0; i < nl; ++i)
        if (L[i].stride != 1 || L[i].cin != 512 || L[i].cout != 512 || L[i].h_out != 6 || L[i].w_out != 4 ||
            L[i].pw_mode != L7.pw_mode || dw_b_of(L[i]) != dw_w_of(L[i]) + 9 * 512)
            return false;
    return next.stride == 2 && next.cin == 512 && dw_b_of(next) == dw_w_of(next) + 9 * 512;
}

bool launch_separable_chip_pw7(const void* in, float* out, int windows, const SepLayer& L7, const SepLayer* L, int nl,
                               const SepLayer& next, hipStream_t stream) {
    if (!separable_chip_pw7_supported(L7, L, nl, next, windows) || in == out) return false;
    const float* const X = static_cast<const float*>(in);
    const long long M = (long long)windows * 24;
    if (L7.pw_mode == 2) launch_chip<true, true, true, true>(X, out, L, nl, M, dw_w_of(next), stream, &L7);
    else launch_chip<false, true, true, true>(X, out, L, nl, M, dw_w_of(next), stream, &L7);
    return true;
}

}  // namespace bd
