/* invpref_als.h -- C ABI of weighted matrix factorization by alternating least squares (Hu, Koren, Volinsky, ICDM 2008): the
 * exact row solves of one half-sweep, the Gram matrix they share and the objective.  Compiled from csrc/invpref_als.hip into
 * libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE)
 * apply here too.  A header of its own, bound through a table of its own (_capi.parse_header on this file): invpref_hip.h and
 * its ABI version do not move.  Every pointer is device memory; every call enqueues on `stream` and returns without
 * synchronising; nothing is allocated: every call is capturable.
 *
 * The model: tables X [user_num, D], Y [item_num, D] -- a plain PureMF model.  The data is a list of entries
 * e = (u_e, i_e, p_e, c_e): preference p_e, confidence c_e = 1 + alpha w_e >= 1.  Every user x item pair carries the base term
 * with confidence 1 and preference 0; each entry adds its own correction, so an entry listed twice counts twice:
 *   J = sum_{u,i} (x_u . y_i)^2 + sum_e [ c_e (p_e - x_{u_e} . y_{i_e})^2 - (x_{u_e} . y_{i_e})^2 ] + lambda (|X|^2 + |Y|^2)
 * One half-sweep solves, for every row r of "this" side with S_r its entries and T the OTHER side's table,
 *   (T^T T + lambda I + sum_{e in S_r} (c_e - 1) t_e t_e^T) x_r = sum_{e in S_r} c_e p_e t_e           t_e = T[cols[e]]
 * exactly: normal matrix, right-hand side, Cholesky factor and both triangular solves in float64, ONE rounding to fp32 where
 * the row is stored.  sum_{u,i} (x . y)^2 is sum_u x_u^T (Y^T Y) x_u, never a loop over the grid.
 *
 * One rank-k accumulation serves the Gram product and the rows: rows of T are gathered into LDS INVPREF_ALS_CHUNK at a time and
 * added as 16 x 16 float64 tiles of the lower triangle on the matrix cores, in entry order.  Every sum has a fixed order, only
 * integer atomics are used (the two counters below): the same bits on every run, whatever the launch geometry. */
#ifndef INVPREF_ALS_H
#define INVPREF_ALS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the widest row the solve takes (a float64 lower triangle of 128 x 128 in LDS); wider rows: INVPREF_EUNSUPPORTED */
#define INVPREF_ALS_MAX_FACTORS 128
/* gathered rows staged in LDS at a time */
#define INVPREF_ALS_CHUNK 64
/* a row of MORE entries than this is cut, from its first entry, into pieces of this many entries; each piece is accumulated by
 * a workgroup of its own into a float64 partial, and the solving workgroup adds the partials in piece order */
#define INVPREF_ALS_SPLIT 2048
/* table rows per float64 partial of the Gram product, added in chunk order */
#define INVPREF_ALS_GRAM_ROWS 512

/* bytes of device scratch one half-sweep over `rows` rows against a table of `other_rows` rows with `entries` entries needs;
 * invpref_als_gram_hip of a table of n rows needs invpref_als_workspace_bytes(1, n, 1, D), the objective the same bytes as the
 * half-sweep.  A function of the sizes alone, non-decreasing in each argument; 0 for sizes it does not take (any argument < 1,
 * factor_num > INVPREF_ALS_MAX_FACTORS, a table of more than 2^31 - 1 rows, more than 2^40 entries). */
size_t invpref_als_workspace_bytes(int64_t rows, int64_t other_rows, int64_t entries, int64_t factor_num);

/* ---- gram = table^T table + lambda I: float64 [D, D], full and symmetric, from the fp32 table [rows, D].  Chunks of
 * INVPREF_ALS_GRAM_ROWS rows leave float64 partials in the workspace; a second launch adds them in chunk order. */
int invpref_als_gram_hip(const float *table, int64_t rows, int64_t factor_num, double lambda, double *gram, void *workspace,
                         size_t workspace_bytes, void *stream);

/* ---- one half-sweep.
 * other_table fp32 [other_rows, D] and gram (invpref_als_gram_hip of it); a CSR over this side's rows: row_ptr int64 [rows + 1],
 * cols int32 / conf fp32 / pref fp32 [entries].  out fp32 [out_rows, D]: without row_ids (null) out_rows must equal rows and
 * list r is solved into row r -- EVERY row of out is overwritten, by one writer, a row without entries with zeros.  With
 * row_ids int32 [rows] list r is solved into row row_ids[r] (the fold-in form: the CSR is a batch of arbitrary lists); a
 * row id outside [0, out_rows) stores nothing.
 *   - an entry whose column lies outside [0, other_rows) is skipped, never used as an address, and counted in *n_skipped
 *   - row_ptr is clamped to [0, entries] and to ascending order within a row; it must ascend (a CSR) for long rows' pieces
 *     to be found, but whatever it holds nothing outside the arrays is read
 *   - a non-positive or NaN pivot (a NaN in a table, a negative conf) or a non-finite result: the row is written as NaN and
 *     bit 0 of *error_word is set; *error_word is sticky -- the call only ever sets bits.  The kernel never loops or traps
 *   - n_skipped is ADDED to: the caller zeroes both words when it wants to
 * factor_num <= INVPREF_ALS_MAX_FACTORS of any width and alignment, otherwise INVPREF_EUNSUPPORTED; null pointers (row_ids may
 * be null) and sizes < 1 give INVPREF_EINVAL, a short workspace INVPREF_EWORKSPACE, a misaligned one INVPREF_EINVAL, all before
 * anything touches a device. */
int invpref_als_solve_hip(const float *other_table, int64_t other_rows, int64_t factor_num, const double *gram,
                          const int64_t *row_ptr, const int32_t *cols, const float *conf, const float *pref, int64_t entries,
                          const int32_t *row_ids, int64_t rows, float *out, int64_t out_rows, int32_t *n_skipped,
                          int32_t *error_word, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the objective: out3 float64 = {fit, reg, J} with reg = |X|^2 + |Y|^2, J as above and fit = J - lambda reg.
 * table [rows, D] is the side the CSR's rows name, other_table [other_rows, D] the side its columns name, gram the Gram matrix
 * of other_table WITH lambda on its diagonal (invpref_als_gram_hip's result): the grid term is sum_r (x_r^T gram x_r - lambda
 * |x_r|^2).  Entries with a column outside the table, or outside every row, add nothing.  Partials per fixed block of rows
 * and of entries, added in block order. */
int invpref_als_objective_hip(const float *table, int64_t rows, const float *other_table, int64_t other_rows,
                              int64_t factor_num, const double *gram, double lambda, const int64_t *row_ptr,
                              const int32_t *cols, const float *conf, const float *pref, int64_t entries, double *out3,
                              void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
