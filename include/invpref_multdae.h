/* invpref_multdae.h -- C ABI of Mult-DAE, the multinomial denoising autoencoder of Liang, Krishnan, Hoffman and Jebara
 * ("Variational Autoencoders for Collaborative Filtering", WWW 2018) with the paper's architecture [I -> D -> I]: the encoder
 * (also the inference kernel) and the gradient pass of one optimiser step over B users, whose [B, I] logit and probability
 * matrices never exist in memory.  Compiled from csrc/invpref_multdae.hip into libinvpref_hip.so next to the entry points of
 * invpref_hip.h, whose error codes (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE) and INVPREF_MAX_FACTORS apply here too.  A
 * header of its own, bound through a table of its own (_capi.parse_header on this file): invpref_hip.h and its ABI version do
 * not move.  Every pointer is device memory; every call enqueues on `stream` and returns without synchronising.
 *
 * The model.  Parameters, all fp32: enc [item_num, D], enc_bias [D], dec [item_num, D], dec_bias [item_num].  There is no
 * user table: a user is the list of its items.  The lists are a CSR, ptr int64 [user_num + 1] and cols int32 (the form
 * ops.ease_lists returns); a pair listed twice is two entries and counts twice; an entry has a global index e in that CSR.
 * One step takes B users u_0 .. u_{B-1} (int32 list ids), a dropout probability p in [0, 1), a seed and a step id.  n_u is
 * the length of the list of u and s_u = 1 / sqrt(n_u): where no pair repeats this is the paper's L2 normalisation of the
 * binary input row.
 *   keep(e)  entry e is kept in this step iff word e & 3 of Philox4x32-10 (Salmon et al., SC 2011; Random123's constants) is
 *            >= floor(p 2^32), with
 *              counter (e >> 2, 0, step_id & 0xffffffff, step_id >> 32)      key (seed & 0xffffffff, seed >> 32)
 *            (the low 32 bits of e >> 2).  p = 0 keeps everything and draws nothing.  The draw depends on (seed, step_id, e, p)
 *            and on nothing else: not on which users share a minibatch.  numpy restates it integer for integer
 *            (tests/multdae_ref.py)
 *   encoder  a_u = enc_bias + (s_u / (1 - p)) sum_{e in list u, kept, CSR order} enc[cols[e]]     sum and tanh in float64
 *            z_u = fp32(tanh(a_u)); everything downstream reads the rounded z_u
 *   decoder  l_uj = z_u . dec[j] + dec_bias[j] for EVERY item j;  lse_u = log sum_j exp(l_uj), the row maximum subtracted
 *   loss     score_loss = (1 / B) sum_u sum_{e in list u} (lse_u - l_{u, cols[e]})      the targets are the WHOLE list, not
 *                                                                                       the dropped one
 *            L2_reg = |enc|^2 + |dec|^2     the whole tables, not the biases (as the paper's code regularises)
 *            loss   = score_loss + L2_coe L2_reg
 *            B is always the divisor; a user with an empty list contributes 0 and has z_u = tanh(enc_bias)
 *   gradients, with g_uj = (n_u exp(l_uj - lse_u) - cnt_uj) / B, cnt_uj the entries of list u that name j:
 *            d dec_bias[j] = sum_u g_uj            d dec[j] = sum_u g_uj z_u + 2 L2_coe dec[j]
 *            dz_u = sum_j g_uj dec[j]              da_u = dz_u (1 - z_u^2)           d enc_bias = sum_u da_u
 *            d enc[i] = sum_u sum_{e in list u, kept, cols[e] = i} (s_u / (1 - p)) da_u + 2 L2_coe enc[i]
 * A list id outside [0, user_num) is an empty list; a column outside [0, item_num) adds nothing anywhere and does not count
 * for n_u; in both cases the three loss values of the pass are NaN.  Nothing read from the device is used as an address
 * unchecked. */
#ifndef INVPREF_MULTDAE_H
#define INVPREF_MULTDAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* users of one step / padded entries of one step's index (below) */
#define INVPREF_MULTDAE_MAX_BATCH 1048576
#define INVPREF_MULTDAE_MAX_ENTRIES 1073741824

/* ---- the encoder: z fp32 [batch, D], row b = z of list users[b], OVERWRITTEN.  Also the inference kernel: with dropout == 0
 * it draws nothing and step_id may be null.  One 16-lane group per user walks its list in CSR order, float64 sums.
 * enc [item_num, D], enc_bias [D], ptr int64 [user_num + 1], cols int32 [nnz], users int32 [batch], step_id int64 [1] (read
 * on the device when the launch runs: a replayed graph draws a new mask after the word is bumped).
 * No allocation, no synchronisation, no atomics: capturable.  Null pointers (cols may be null where nnz == 0, step_id where
 * dropout == 0), sizes < 1 (nnz < 0) and a dropout outside [0, 1) give INVPREF_EINVAL; factor_num > INVPREF_MAX_FACTORS, batch
 * > INVPREF_MULTDAE_MAX_BATCH and a table of more than 2^31 - 1 rows INVPREF_EUNSUPPORTED. */
int invpref_multdae_encode_hip(const float *enc, const float *enc_bias, int64_t item_num, int64_t factor_num,
                               const int64_t *ptr, const int32_t *cols, int64_t user_num, int64_t nnz, const int32_t *users,
                               int64_t batch, double dropout, int64_t seed, const int64_t *step_id, float *z, void *stream);

/* bytes of device scratch invpref_multdae_grad_hip needs; 0 for sizes it does not take (any argument < 1, an odd
 * index_entries, factor_num > INVPREF_MAX_FACTORS, batch > INVPREF_MULTDAE_MAX_BATCH, index_entries >
 * INVPREF_MULTDAE_MAX_ENTRIES, more than 2^31 - 1 items).  A function of the sizes alone, non-decreasing in each argument.  It
 * holds z, da and the positives' float64 sums per user, the segment partials of the column pass (at most 1024 + item_num / 64
 * blocks of 64 rows), float64 loss partials and the chunk slots of the item-side walk:
 * O((batch + segments item_num) D + index_entries D / chunk), with NO term proportional to batch * item_num. */
size_t invpref_multdae_workspace_bytes(int64_t item_num, int64_t batch, int64_t index_entries, int64_t factor_num);

/* geometry5 (HOST memory, int64 [5]) = {users per workgroup of the rows launches, items per LDS tile, users per segment of
 * the column pass, entries per chunk of the item-side walk, items per split of the rows launches} for these sizes, so that
 * tests can aim at the seams; the column pass has ceil(batch / segment) segments and the rows launches ceil(item_num / split)
 * splits, the last of each ragged.  A workgroup of the rows launches sweeps split / tile item tiles, one of the column pass
 * segment / 64 user tiles.  INVPREF_EINVAL / EUNSUPPORTED as above. */
int invpref_multdae_geometry(int64_t item_num, int64_t batch, int64_t index_entries, int64_t *geometry5);

/* ---- the gradient pass of one step.
 * index: the inverted index of the step's entries, int32 [5 n2 + batch + 1] with n2 = index_entries, an even number >= 2 and
 * >= the step's entries (the sum of its users' list lengths; a user listed twice in the step brings its list twice).  Entry k
 * of the step is entry ptr[users[b]] + (k - start[b]) of the CSR, b its position in the step:
 *   [0, 2 n2)        list 0: (item row, k) pairs sorted by item row, then by k; the padding, and an entry whose column lies
 *                    outside the table, under the sentinel row 2^31 - 1, which sorts last (the format of invpref_cvib_index_hip)
 *   [2 n2, 4 n2)     list 1: sentinel pairs (-1, 0) only
 *   [4 n2, 5 n2)     the position b of entry k in the step; -1: padding
 *   [5 n2, .. + batch + 1)   start[b], the first k of position b; start[batch] = the step's entries
 * ops.multdae_index builds it once per static minibatch.
 *
 * Launches:
 *   encode    as above, and per user the float64 walk of the positives: sum_e dec[cols[e]], sum_e l_{u, cols[e]}
 *   rows      a workgroup owns 64 users (16 per wave: the z rows are MFMA operands in registers) and sweeps the whole item
 *             table twice in LDS tiles of 64 rows of dec: logits on v_mfma_f32_16x16x4_f32 in a fixed K order, the row
 *             maximum and sum online per lane, combined in float64: lse_u; then n_u p_uj from the finished lse_u and
 *             sum_j n_u p_uj dec[j] as a second MFMA product, tiles of 16 items added in order in float64 (the item table is cut into
 *             splits that workgroups sweep side by side; their partials are added in split order); da_u [batch, D] and a
 *             four-float record per user leave it
 *   columns   a workgroup owns 64 items (16 per wave) and one SEGMENT of the step's users: p_uj recomputed from z_u and the
 *             record (the same bits), cnt_uj counted from list 0 into LDS, sum_u (n_u p_uj - cnt_uj) z_u as an MFMA product
 *             and sum_u (n_u p_uj - cnt_uj) in float64; one partial per (segment, item)
 *   scatter, boundary   csrc/chunk_walk.hpp over list 0: the kept entries' (s_u / (1 - p)) da_u, keep(e) recomputed from
 *             the entry index, into the rows of d enc; float64 sums.  The walk's factors are fp32 (chunk_walk.hpp), so here
 *             s_u / (1 - p) is the float64 value the encoder uses rounded ONCE to fp32: 2^-24 relative on d enc's list terms
 *   items     a 16-lane group per item, the ONE writer of d dec[j], d enc[j], d dec_bias[j]: the segment partials in segment
 *             order over B, what the walk stored, the regulariser gradient; rows no list names are written too
 *   fold      d enc_bias, L2_reg as a fixed-order tree, the three losses
 *   - every element of grad_enc, grad_enc_bias, grad_dec, grad_dec_bias is defined after the call; nobody else zeroes them
 *   - losses3 = {score_loss, L2_reg, loss} is overwritten
 *   - every sum has a fixed order that is a function of the sizes alone; no float atomics; one writer per row per launch:
 *     the same bits on every run
 *   - no allocation, no synchronisation; ids, lists, index and the step id are read on the device when the launches run:
 *     capturable
 * Null pointers (cols may be null where nnz == 0), sizes < 1 (nnz < 0), an odd index_entries, a dropout outside [0, 1) and a
 * misaligned workspace give INVPREF_EINVAL; sizes beyond the limits above INVPREF_EUNSUPPORTED; a short workspace
 * INVPREF_EWORKSPACE -- all before anything touches a device. */
int invpref_multdae_grad_hip(const float *enc, const float *enc_bias, const float *dec, const float *dec_bias, int64_t item_num,
                             int64_t factor_num, const int64_t *ptr, const int32_t *cols, int64_t user_num, int64_t nnz,
                             const int32_t *users, int64_t batch, const int32_t *index, int64_t index_entries, double dropout,
                             int64_t seed, const int64_t *step_id, double L2_coe, float *grad_enc, float *grad_enc_bias,
                             float *grad_dec, float *grad_dec_bias, float *losses3, void *workspace, size_t workspace_bytes,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif
