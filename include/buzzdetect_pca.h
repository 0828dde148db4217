/*
 * buzzdetect_pca.h — C ABI of the streaming principal-component analysis in libbuzzdetect_hip.so (gfx950): the column sums and
 * the 1024 x 1024 Gram matrix of [W][1024] embeddings where they lie, and the projection of rows on up to 64 components with the
 * residual of that projection, for buzzdetect_amd/pca.py.  No row goes back to the host, and a fit is reproducible bit for bit.
 *
 *   bd_pca_sums              per slice of 256 rows the column sums of the shifted rows     (bd_pca_sums_host: the same bits)
 *   bd_pca_workspace_bytes   host only: the scratch bd_pca_gram takes for R rows
 *   bd_pca_gram              the Gram matrix of the shifted rows, written or added to      (bd_pca_gram_host: the same bits)
 *   bd_pca_project           y = (E V^T - mv) * scale and the squared distance from the components' subspace
 *                                                                  (bd_pca_project_host: the same bits, given the scores)
 *
 * Notation.  E is [W][BD_PCA_DIM] float32, 16-byte aligned, W = rows_total.  `pick` is null or int32 [R]: the call's row r is
 * E[pick[r]], or E[r] when pick is null (then R <= W), so a sample is fitted without a gathered copy.  An id outside 0 .. W - 1
 * is refused by the host restatements (BD_ERANGE); the device cannot look before it launches and takes it as the nearest end of
 * the range, so that nothing is read out of bounds.  n2 is bd_search_norms of E (buzzdetect_search.h), indexed like E.  A row
 * whose n2 is not finite holds a NaN or an infinity, or overflows: it is ABSENT and contributes exactly zero to every sum below.
 * `shift` is float32 [BD_PCA_DIM] (16-byte aligned), or null where allowed.  t(r, c) = E[row r][c] - shift[c], one rounded
 * subtraction (E[row r][c] itself with a null shift); for an absent row and for a row past R it is 0.0f.  Every step named below
 * is one correctly rounded float32 operation, and nothing is contracted into a fused multiply-add except where fmaf is named.
 *
 * Sums.  Rows are taken in slices of BD_PCA_SUM_SLICE = 256.  partial[s][c] is the chain 0.0f + t(256 s, c) + t(256 s + 1, c)
 * + ... in ascending r over the slice's rows below R.  One thread owns four neighbouring channels of a slice and reads them 16
 * bytes at a time.  There are (R + 255) / 256 slices; the host adds the partials in float64.
 *
 * Gram.  Rows are taken in slices of BD_PCA_SLICE = 1024.  The matrix is cut into 32 x 32 tiles; tile (ti, tj) holds rows
 * 32 ti .. 32 ti + 31 and columns 32 tj .. 32 tj + 31, and the 528 tiles with ti <= tj are computed.  Slice s gives, for every
 * (i, j) of those tiles, the partial P_s[i][j]: the chain acc = fmaf(t(r, i), t(r, j), acc) from acc = 0.0f in ascending r over
 * the slice's rows below R, and after an odd number of them one more row of zeros.  It is computed on v_mfma_f32_32x32x2_f32,
 * whose result is bit for bit that chain: one instruction consumes rows 2m and 2m + 1 of the slice, in that order.  Both
 * operands of a tile are panels of the same rows read row-major - lane l of a fragment holds t(2m + (l >> 5), 32 tile + (l & 31))
 * - so nothing is transposed anywhere.  A workgroup of four waves owns a 128 x 128 block of the upper triangle and one slice,
 * stages the slice's two panels through LDS 32 rows at a time (the shift is subtracted and absent rows become zeros there, once),
 * and each wave keeps a 64 x 64 block in four accumulator tiles, every fragment it loads feeding two instructions.  The blocking
 * does not enter the bits.  The partials lie in the workspace: [slice][tile][1024], ceil(R / 1024) * 528 * 1024 floats.
 * A finishing pass forms T[i][j] = P_0[i][j] + P_1[i][j] + ..., a chain in ascending s that starts from P_0, and writes
 *   accumulate == 0    gram[i][j] = gram[j][i] = T[i][j]
 *   accumulate == 1    gram[i][j] = gram[j][i] = gram_old[i][j] + T[i][j]
 * for the (i, j) of a tile with ti < tj: the thread that owns (i, j) is the only one that reads or writes either element.  Within
 * a diagonal tile (ti == tj) every element, of both triangles, comes from the tile's own accumulator for it (with accumulate,
 * added to its own old value).  The two triangles are equal all the same: P_s[i][j] and P_s[j][i] are chains of fmaf(a, b, .)
 * and fmaf(b, a, .), which are the same operation, so gram == gram^T in every bit, given a symmetric gram_old.
 *
 * Project.  `packed` is bd_search_pack_queries of the components V [d][BD_PCA_DIM]; a wave owns 32 rows and walks the one or
 * two column tiles by the walk of the Dense heads, so s(w, j) has exactly the bits bd_search_scores(..., BD_SEARCH_DOT) stores
 * for the same rows and the same packed matrix.  c2[w] is the chain and butterfly of bd_search_norms over the row
 * E[w][c] - mean[c] (each difference rounded), computed whether or not `resid` is asked for.  u_j = s(w, j) - mv[j].
 *   y[w][j]   = u_j * scale[j]
 *   q[w]      = the chain 0.0f + u_0 * u_0 + u_1 * u_1 + ... in ascending j, each product rounded, then added
 *   resid[w]  = fmaxf(c2[w] - q[w], 0.0f)                                             (only when resid is not null)
 * A row whose c2 is not finite (a NaN, an infinity or an overflow in it) gets a quiet NaN in every y[w][j] and in resid[w], and
 * spoils no other row.  A row's bits depend on the row and the model alone, not on W or on where the row sits.
 * bd_pca_project_host takes s as bd_search_scores stored it ([W][d], row-major) and restates everything after it.
 *
 * No floating-point number is added atomically, no result depends on the grid, every output element has one writer, inputs
 * are only read, and all element offsets are 64-bit.
 *
 * Limits (refused on the host with the argument named, nothing launched): 0 <= R <= BD_PCA_MAX_ROWS for sums and gram,
 * 1 <= rows_total < 2^31 (and R <= rows_total with a null pick), 0 <= W <= BD_SEARCH_MAX_WINDOWS for project; a count of 0
 * launches nothing and writes nothing, on the host too; 1 <= d <= BD_PCA_MAX_COMPONENTS; accumulate is 0 or 1; non-null pointers
 * (E, shift, mean, packed, gram and the workspace 16-byte aligned, everything else 4-byte aligned), and a workspace of at least
 * bd_pca_workspace_bytes(R) bytes (BD_EWORKSPACE).
 *
 * Conventions are those of buzzdetect_hip.h: 0 on success, a negative BD_E* code on failure, bd_last_error() for the text; the
 * caller owns all device memory; `stream` is a hipStream_t.
 */
#ifndef BUZZDETECT_PCA_H
#define BUZZDETECT_PCA_H

#include <stdint.h>

#include "buzzdetect_hip.h"
#include "buzzdetect_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BD_PCA_ABI_VERSION 1
#define BD_PCA_DIM 1024                         /* floats per row: BD_SEARCH_DIM */
#define BD_PCA_MAX_COMPONENTS 64
#define BD_PCA_MAX_ROWS (1 << 18)               /* rows per call of sums and gram */
#define BD_PCA_SLICE 1024                       /* rows per Gram partial */
#define BD_PCA_SUM_SLICE 256                    /* rows per column-sum partial */

BD_API int bd_pca_abi_version(void);

/* partial [(R + 255) / 256][BD_PCA_DIM]; shift may be null */
BD_API int bd_pca_sums(const float* e_dev, int64_t rows_total, const int32_t* pick_dev, int64_t R, const float* n2_dev,
                       const float* shift_dev, float* partial_dev, void* stream);
BD_API int bd_pca_sums_host(const float* e, int64_t rows_total, const int32_t* pick, int64_t R, const float* n2,
                            const float* shift, float* partial);

/* Host only.  Bytes of scratch for bd_pca_gram over R rows (a negative code for R out of range). */
BD_API int64_t bd_pca_workspace_bytes(int64_t R);

/* gram [BD_PCA_DIM][BD_PCA_DIM]; shift may be null */
BD_API int bd_pca_gram(const float* e_dev, int64_t rows_total, const int32_t* pick_dev, int64_t R, const float* n2_dev,
                       const float* shift_dev, int32_t accumulate, float* gram_dev, void* workspace_dev, int64_t workspace_bytes,
                       void* stream);
BD_API int bd_pca_gram_host(const float* e, int64_t rows_total, const int32_t* pick, int64_t R, const float* n2,
                            const float* shift, int32_t accumulate, float* gram);

/* packed: bd_search_pack_queries of V [d][BD_PCA_DIM]; mv, scale [d]; mean [BD_PCA_DIM]; y [W][d]; resid [W] or null */
BD_API int bd_pca_project(const float* e_dev, int64_t W, const float* packed_dev, int32_t d, const float* mv_dev,
                          const float* scale_dev, const float* mean_dev, float* y_dev, float* resid_dev, void* stream);
/* scores [W][d]: what bd_search_scores(..., BD_SEARCH_DOT, ..., row_stride d, col_stride 1) stored for these rows */
BD_API int bd_pca_project_host(const float* e, int64_t W, const float* scores, int32_t d, const float* mv, const float* scale,
                               const float* mean, float* y, float* resid);

#ifdef __cplusplus
}
#endif

#endif /* BUZZDETECT_PCA_H */
