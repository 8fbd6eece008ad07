/* invpref_lgcn.h -- C ABI of LightGCN (He et al., SIGIR 2020): the propagation of two embedding tables through a static,
 * weighted bipartite graph, and the ego regulariser of one BPR step.  Compiled from csrc/invpref_lgcn.hip into
 * libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE)
 * and INVPREF_MAX_FACTORS apply here too.  A header of its own, bound through a table of its own (_capi.parse_header on this
 * file): invpref_hip.h and its ABI version do not move.  Every pointer INSIDE a side and every table is device memory; the
 * InvPrefLgcnSide structs themselves are host memory, read before the call returns.  Every call enqueues on `stream` and
 * returns without synchronising; nothing is allocated, so the calls are capturable.
 *
 * THE OPERATOR.  With A the [user_num + item_num]^2 matrix whose user rows hold the user side's entries and whose item rows
 * hold the item side's (LightGCN: w = 1 / sqrt(deg_u deg_i) on both, so A is symmetric and the operator its own adjoint),
 *   out = (1 / (K + 1)) sum_{k = 0 .. K} A^k X                         X = (x_user; x_item), K = n_layers
 * The kernels never look at degrees, only at w: any edge weights are propagated.
 *
 * THE ARITHMETIC, fixed here so that numpy restates it (tests/lgcn_ref.py, propagate_rounded):
 *   - layer k + 1 of a destination row is the sum over the row's entries IN CSR ORDER of (double)w * (double)x^k[col],
 *     accumulated in float64 and rounded to fp32 once, where the layer is stored (the product of two fp32 values is exact in
 *     float64, so a fused multiply-add gives the same bits)
 *   - a cut row's (below) piece partials are float64 and are added IN PIECE ORDER, starting from +0, by one writer
 *   - out after layer k is fp32((double)out + (double)x^k / (double)(K + 1)), out = 0 before layer 0: one rounding per layer
 *   - K = 0: out = x, bit for bit
 *   - a row without entries is zero from layer 1 on
 *   - a column id outside the partner table contributes nothing and is never an address; a row_ptr or piece bound that
 *     reaches outside cols is clamped
 * No float atomics, a fixed order for every sum: the same bits on every run.
 *
 * THE PIECE PLAN, made once on the host (ops.lgcn_graph).  A row with more than INVPREF_LGCN_PIECE entries is CUT into
 * consecutive pieces of that length (the last one shorter); a row up to that length, an empty one included, is one piece.
 * The pieces of a side, in row order, tile its entries: piece p is the entries [piece_at[p], piece_at[p + 1]) of row
 * piece_row[p].  piece_slot[p] is -1 for a whole row, which its piece's group stores, and otherwise the piece's float64
 * partial slot; the slots of a cut row are consecutive, cut row c (cut_row[c]) owning [cut_slot[c], cut_slot[c + 1]).  The
 * kernels take the piece bounds from the plan, not from the constant, so a plan cut at another length is propagated the same
 * way (tools/lgcn_rate.py measures the alternatives so). */
#ifndef INVPREF_LGCN_H
#define INVPREF_LGCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* entries of one piece of a cut row -- measured on an MI355X over 8 .. 1 024: a piece is one serial chain
 * of its 16-lane group, and the longest chain sets a layer's time / the most layers of one call */
#define INVPREF_LGCN_PIECE 16
#define INVPREF_LGCN_MAX_LAYERS 8

/* one side of the graph: a CSR over this side's rows with the partner side's rows as columns, and its piece plan */
typedef struct InvPrefLgcnSide {
    int64_t rows;              /* rows of this side's table */
    int64_t nnz;               /* entries of cols / w */
    const int64_t *row_ptr;    /* [rows + 1] */
    const int32_t *cols;       /* [nnz] rows of the PARTNER table (null when nnz is 0) */
    const float *w;            /* [nnz] */
    int64_t n_pieces;          /* >= rows */
    const int32_t *piece_row;  /* [n_pieces] */
    const int64_t *piece_at;   /* [n_pieces + 1] */
    const int32_t *piece_slot; /* [n_pieces] */
    int64_t n_cut;             /* cut rows */
    int64_t n_slots;           /* partial slots: the pieces of the cut rows */
    const int32_t *cut_row;    /* [n_cut] (null when n_cut is 0) */
    const int32_t *cut_slot;   /* [n_cut + 1] (null when n_cut is 0) */
} InvPrefLgcnSide;

/* bytes of device scratch invpref_lgcn_propagate_hip needs: two ping-pong layer tables of [user_num + item_num, factor_num]
 * fp32 and user_slots + item_slots float64 partial slots.  0 for sizes it does not take (a size < 1, a slot count < 0,
 * factor_num > INVPREF_MAX_FACTORS, more than 2^31 - 1 rows or slots).  Non-decreasing in each argument. */
size_t invpref_lgcn_workspace_bytes(int64_t user_num, int64_t item_num, int64_t factor_num, int64_t user_slots,
                                    int64_t item_slots);

/* ---- the propagation.  x_user [user_side->rows, factor_num], x_item [item_side->rows, factor_num] fp32; out_user / out_item
 * alike, OVERWRITTEN, every row defined, distinct from the inputs.  Per layer two launches: one 16-lane group per piece of
 * both sides (user pieces, then item pieces), then one group per cut row of both sides; the kernel boundary is the only
 * synchronisation between workgroups.  The writer of a row of layer k + 1 also brings the row of `out` up to date, and the
 * last layer is never stored.  factor_num <= INVPREF_MAX_FACTORS of any width (rows that are not a multiple of four floats, or
 * tables that are not 16-byte aligned, take an element-wise path) and 0 <= n_layers <= INVPREF_LGCN_MAX_LAYERS, otherwise
 * INVPREF_EUNSUPPORTED, as are more than 2^31 - 1 rows, entries or pieces; null pointers, sizes < 1, n_layers < 0, an output
 * that is an input and a misaligned workspace give INVPREF_EINVAL, a short workspace INVPREF_EWORKSPACE, all before anything
 * touches a device. */
int invpref_lgcn_propagate_hip(const InvPrefLgcnSide *user_side, const InvPrefLgcnSide *item_side, const float *x_user,
                               const float *x_item, int64_t factor_num, int64_t n_layers, float *out_user, float *out_item,
                               void *workspace, size_t workspace_bytes, void *stream);

/* bytes of device scratch invpref_lgcn_reg_hip needs (two int32 count tables, float64 partials); 0 for sizes it does not take */
size_t invpref_lgcn_reg_workspace_bytes(int64_t user_num, int64_t item_num);

/* ---- the ego regulariser of one BPR step over the triplets (users int64, pos_items int64, neg int32: [batch]), taken on
 * the EGO tables P = ego_user [user_num, D], Q = ego_item [item_num, D] (the definition of invpref_bpr.h):
 *   L2_reg = (|P[u]|^2 + |Q[i]|^2 + |Q[j]|^2) / (batch D) summed over the triplets' gathered rows, repeats counted
 *   L1_reg alike with absolute values
 *   every gather adds (2 L2_coe row + L1_coe sign(row)) / (batch D) to that row's gradient
 * A triplet with ANY id outside its table (neg = -1 included) is skipped whole, as invpref_bpr_grad_hip skips it, and then
 * L2_reg, L1_reg and loss are NaN as that pass's four values are.  batch is always the divisor.
 *   - ADDS into grad_user / grad_item (a row with n gathers: fp32((double)grad + n (2 L2_coe x + L1_coe sign(x)) / (batch D)),
 *     one rounding); a row no valid triplet gathers is not touched
 *   - overwrites losses4[1] = L2_reg and losses4[2] = L1_reg, sets losses4[3] = losses4[0] + L2_coe L2_reg + L1_coe L1_reg
 *     (float64 behind the fp32 losses4[0], rounded once) and leaves losses4[0] alone
 * Launches: a stream-ordered zero fill of the counts; gather counts per row by INTEGER atomics; one 16-lane group per table
 * row over the rows with a count, norm partials per workgroup in float64; a fold in a fixed order.  No float atomics: the
 * same bits on every run.  Codes as above. */
int invpref_lgcn_reg_hip(const int64_t *users, const int64_t *pos_items, const int32_t *neg, int64_t batch,
                         const float *ego_user, int64_t user_num, const float *ego_item, int64_t item_num, int64_t factor_num,
                         double L2_coe, double L1_coe, float *grad_user, float *grad_item, float *losses4, void *workspace,
                         size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
