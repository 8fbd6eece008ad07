/* invpref_ease.h -- C ABI of EASE (Steck, WWW 2019, "Embarrassingly Shallow Autoencoders for Sparse Data"): the item-item ridge
 * model in closed form, and the exact inverse of a symmetric positive definite matrix it is built on.  Compiled from
 * csrc/invpref_ease.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes (INVPREF_EINVAL /
 * EUNSUPPORTED / EWORKSPACE) apply here too.  A header of its own, bound through a table of its own (_capi.parse_header on this
 * file): invpref_hip.h and its ABI version do not move.  Every pointer is device memory; every call enqueues on `stream` and
 * returns without synchronising; nothing is allocated: every call is capturable.  Argument errors are returned before anything
 * touches a device.
 *
 * The model: X [user_num, item_num], x_ui = the number of times (u, i) is listed (a pair listed twice counts twice).
 *   G = X^T X            exact non-negative integers
 *   A = G + lambda I     lambda > 0
 *   P = A^-1
 *   B[i, j] = -P[i, j] / P[j, j]  (i != j),   B[j, j] = 0
 *   score(u, .) = x_u . B
 * All arithmetic is float64; B is stored in fp32, rounded once where it is stored, a score once where it is stored.  Every sum
 * has a fixed order and the only atomics are integer adds in LDS and the two words below: the same bits on every run. */
#ifndef INVPREF_EASE_H
#define INVPREF_EASE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the largest matrix the inverse takes, and so the largest catalogue; larger: INVPREF_EUNSUPPORTED.  Element offsets are 64-bit */
#define INVPREF_EASE_MAX_ITEMS 65536
/* the inverse works on square blocks of this many rows (a float64 block is 32 KB of LDS); ragged last blocks are handled in the
 * kernels, the matrix is never padded */
#define INVPREF_EASE_BLOCK 64
/* columns of one row of G a workgroup counts in LDS at a time */
#define INVPREF_EASE_GRAM_SLICE 8192
/* the counters of G are int32: every entry of G, which its largest diagonal entry sum_u x_ui^2 bounds, must stay below
 * 2^INVPREF_EASE_COUNT_BITS.  The caller checks (ops.ease_lists does, on the host); larger counts wrap */
#define INVPREF_EASE_COUNT_BITS 31

/* bytes of device scratch invpref_spd_inverse_hip of an n x n matrix needs (the triangular factor's inverse, float64 [n, n]).
 * A function of n alone, non-decreasing; 0 for sizes it does not take (n < 1, n > INVPREF_EASE_MAX_ITEMS).  The other entry
 * points need no scratch. */
size_t invpref_ease_workspace_bytes(int64_t n);

/* ---- a = X^T X + lambda I: float64 [item_num, item_num], full and symmetric, EVERY element written by one writer.
 * The positive entries as two CSRs: by user (user_ptr int64 [user_num + 1], user_cols int32 [entries]: item ids) and by item
 * (item_ptr int64 [item_num + 1], item_cols int32 [entries]: user ids).  Row i of a: for every user of item_cols' list i, that
 * user's list is walked and counted into an LDS slice of INVPREF_EASE_GRAM_SLICE columns with integer adds; the slice is stored
 * as float64, lambda added once on the diagonal.
 *   - a column outside its table ([0, item_num) in user_cols, [0, user_num) in item_cols) is skipped, never used as an address,
 *     and counted once in *n_skipped, which is ADDED to
 *   - both row_ptr arrays are clamped to [0, entries] and to ascending order within a row: whatever they hold nothing outside
 *     the arrays is read
 * Null pointers, sizes < 1, a lambda that is not finite and > 0: INVPREF_EINVAL; item_num > INVPREF_EASE_MAX_ITEMS, user_num or
 * entries > 2^31 - 1: INVPREF_EUNSUPPORTED. */
int invpref_ease_gram_hip(const int64_t *user_ptr, const int32_t *user_cols, const int64_t *item_ptr, const int32_t *item_cols,
                          int64_t entries, int64_t user_num, int64_t item_num, double lambda, double *a, int32_t *n_skipped,
                          void *stream);

/* ---- a <- a^-1 in place: a float64 [n, n], symmetric positive definite; only its lower triangle is read, the result is
 * written full, and equal to its transpose bit for bit.  Three phases over blocks of INVPREF_EASE_BLOCK, the block loops on the
 * host and a function of n alone, kernel boundaries the only synchronisation between workgroups:
 *   factor      a = L L^T: a diagonal-block kernel factors L_kk in LDS and leaves L_kk^-1 in the workspace; the panel
 *               L_ik = A_ik L_kk^-T and the trailing update A_ij -= L_ik L_jk^T are float64 MFMA tile products
 *   inverse     W = L^-1 into the workspace by the blocked recurrence W_ij = -sum_{j <= k < i} (L_ii^-1 L_ik) W_kj
 *   product     a = W^T W, the upper triangle mirrored from the lower
 * A non-positive or NaN pivot: the result is NaN throughout and bit 0 of *error_word is set; *error_word is sticky -- the call
 * only ever sets bits.  The kernels never loop on data and never trap.
 * Null pointers, n < 1: INVPREF_EINVAL; n > INVPREF_EASE_MAX_ITEMS: INVPREF_EUNSUPPORTED; a short workspace: INVPREF_EWORKSPACE;
 * a workspace or matrix that is not 16-byte aligned: INVPREF_EINVAL. */
int invpref_spd_inverse_hip(double *a, int64_t n, int32_t *error_word, void *workspace, size_t workspace_bytes, void *stream);

/* ---- b fp32 [item_num, item_num] from p = A^-1 float64 [item_num, item_num]: b[i, j] = fp32(-p[i, j] / p[j, j]), b[j, j] = 0.
 * A column whose p[j, j] is not finite and positive is written as NaN, its diagonal element included, and bit 0 of the sticky
 * *error_word is set. */
int invpref_ease_weights_hip(const double *p, int64_t item_num, float *b, int32_t *error_word, void *stream);

/* ---- out[r, :] = fp32(sum over the entries e of the r-th list, in CSR order, of float64(b[cols[e], :])): out fp32 [out_rows,
 * item_num].  A CSR of `lists` lists: row_ptr int64 [lists + 1] (clamped as above), cols int32 [entries] (entries may be 0, cols
 * then null).  Without list_ids (null) rows must equal lists and the r-th list is list r; with list_ids int32 [rows] it is list
 * list_ids[r] -- a batch of users scored against the CSR of all of them; an id outside [0, lists) is an empty list.  Without
 * row_ids (null) out_rows must equal rows and the r-th list is scored into row r: EVERY row of out is written, by one writer, an
 * empty list with zeros.  With row_ids int32 [rows] it goes to row row_ids[r]; a row id outside [0, out_rows) stores nothing.
 * An entry whose column lies outside [0, item_num) adds nothing and is never used as an address.
 * b and out must be 16-byte aligned (INVPREF_EINVAL otherwise); rows are read as float4 where item_num is a multiple of 4. */
int invpref_ease_scores_hip(const float *b, int64_t item_num, const int64_t *row_ptr, int64_t lists, const int32_t *cols,
                            int64_t entries, const int32_t *list_ids, const int32_t *row_ids, int64_t rows, float *out,
                            int64_t out_rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif
