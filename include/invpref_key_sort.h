/* invpref_key_sort.h -- C ABI of the library's own sort: a keys-only LSD radix sort of unsigned 32- or 64-bit keys, and the
 * global AUC of explicit evaluation computed through it in O(n log n) instead of invpref_auc_pairs_hip's O(P Nn).
 *
 * invpref_sort_keys_u32_hip / invpref_sort_keys_u64_hip: keys device [n], sorted ascending as UNSIGNED integers, IN PLACE: the
 *   result stands in keys.  key_bits in [0, 32] / [0, 64] is the caller's bound on the significant low bits; it sets the
 *   number of 8-bit digit passes, ceil(key_bits / 8), and never the result for keys that respect it.  Keys are ordered by
 *   their low key_bits bits and keys equal in those bits keep their input order (every pass is stable), so the result is
 *   defined, and the same on every run, even for keys that break the bound.  key_bits = 0 or n <= 1 launches nothing, needs
 *   neither keys nor a workspace, and returns 0.  A pass is three launches: a digit histogram per tile of
 *   INVPREF_KEY_SORT_TILE keys, a scan over [digit][tile], and a scatter that re-reads the tile, ranks it stably and writes;
 *   the passes alternate between keys and the workspace's buffer, and an odd number of passes ends with a device-to-device
 *   copy back into keys.  Kernel boundaries are the only synchronisation between workgroups: nothing waits on another
 *   workgroup.  The launch geometry depends on n and key_bits alone.
 *
 * invpref_auc_sorted_hip: invpref_auc_pairs_hip's contract (invpref_segment_rank.h) word for word -- values device fp32 [n],
 *   labels device uint8 [n]: 1 positive, 0 negative, any other value leaves the entry out; out device int64 [3] = {C, P, Nn},
 *     C = sum over positives p of ( 2 #{ q negative : key(q) < key(p) } + #{ q negative : key(q) == key(p) } )
 *   with key = order_key of csrc/rank_key.hpp, C = 0 where a class is empty or n = 0 -- and the same integers, at another
 *   cost: one launch writes n keys (a negative's order key; 0xffffffff, above every order key, for everything else) and counts
 *   the classes, sort_keys_u32 orders them, one launch searches the lower and the upper bound of every positive's key.
 *   INVPREF_AUC_SORT_MIN: the entry count from which ops.auc_counts(route='auto') takes this route, measured.
 *
 * invpref_sort_keys_workspace_bytes(n, key_bytes) / invpref_auc_sorted_workspace_bytes(n): 0 for sizes the entry points do not
 *   take (n < 0, n >= 2^31, key_bytes other than 4 or 8), positive otherwise, non-decreasing in n: the alternate buffer of n
 *   keys plus 256 x tiles histogram counters and 256 digit totals (the AUC adds its n keys in front).
 *
 * Compiled from csrc/invpref_key_sort.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes
 * apply here.  A header of its own, bound through a table of its own (_capi.parse_header on this file): invpref_hip.h and its
 * ABI version do not move.  No allocation, no synchronisation, no global state: every call is capturable.  Return codes:
 * INVPREF_EINVAL for a negative n, key_bits out of range, a null pointer that the sizes make necessary; INVPREF_EUNSUPPORTED for
 * n >= 2^31; INVPREF_EWORKSPACE for a null or short workspace; a hipError_t (> 0) if a launch fails; 0 otherwise.  Every
 * argument check runs before anything touches a device. */
#ifndef INVPREF_KEY_SORT_H
#define INVPREF_KEY_SORT_H

#include <stddef.h>
#include <stdint.h>

/* keys one workgroup ranks and scatters per pass */
#define INVPREF_KEY_SORT_TILE 4096
/* entries from which ops.auc_counts(route='auto') sorts: the measured crossover of DESIGN.md §4.5.8 */
#define INVPREF_AUC_SORT_MIN 54000

#ifdef __cplusplus
extern "C" {
#endif

size_t invpref_sort_keys_workspace_bytes(int64_t n, int32_t key_bytes);

int invpref_sort_keys_u32_hip(uint32_t *keys, int64_t n, int32_t key_bits, void *workspace, size_t workspace_bytes,
                              void *stream);

int invpref_sort_keys_u64_hip(uint64_t *keys, int64_t n, int32_t key_bits, void *workspace, size_t workspace_bytes,
                              void *stream);

size_t invpref_auc_sorted_workspace_bytes(int64_t n);

int invpref_auc_sorted_hip(const float *values, const uint8_t *labels, int64_t n, int64_t *out, void *workspace,
                           size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
