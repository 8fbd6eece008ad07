// chunk_walk.hpp -- the chunked scatter and its boundary walk: per-pair gradients summed per destination row, deterministically,
// for rows no row plan knows.  Built on it: CVIB's information term (invpref_cvib.hip), BPR-MF's gradient pass
// (invpref_bpr.hip; LightGCN, invpref_lgcn.hip, trains through that pass on its final tables), the doubly robust pass
// (invpref_dr.hip), sampled-softmax MF's two scatters (invpref_ssm.hip) and DICE's four-table pass (invpref_dice.hip).  Each
// states what is its own in a policy struct (below) and keeps its kernels' names, arguments and launch geometry.  This comment
// is the one statement of the scheme.
//
// What it offers: the geometry (chunk_of, ChunkGeom, chunk_geom, slot_of), the slot and accumulator helpers, clamp_id, the two
// kernel bodies chunk_scatter / chunk_boundary, and -- for the passes that carry the L2 / L1 regularisers, all but CVIB's --
// norms64, reg_of and RegWalk, the policy base that holds everything of a policy but the entries themselves; on top of it
// triplet_ok and TripletWalk, the entries of a pass over signed (u, i+, j-) triplets (BPR's, DICE's) but for where a
// triplet's factor is read.
//
// The input.  Per side (0: user rows, partner table Qi; 1: item rows, partner table Pu) the step's n2 = 2 B positions come
// sorted by destination row as (row, position) entries: the inverted index of invpref_cvib_index_hip, `stride` entries per
// side.  A position that must reach no row is filed under a SENTINEL destination that sorts last (an id >= the side's table; a
// negative one counts too): the first sentinel entry ends the side's list for every group that meets it.
//
// The scatter.  The list is cut into chunks of C consecutive entries (16; 128 beyond 65 536 positions).  One 16-lane group
// (kernel_common.hpp: a row on 16 lanes) owns one chunk of one side and walks it in index order: index entry -> the entry's
// operands -> the partner row, three dependent loads, each stage issued for kAhead entries before the next begins so that
// kAhead chains are in flight together; acc += factor * partner row in float64.  Where the destination changes, the sum goes
//   - to the gradient table, if all of the destination's entries lie inside the chunk: this group is its only writer;
//   - to the chunk's HEAD slot, if it is the chunk's first destination and continues from the previous chunk (entry e0 - 1
//     names it too) -- also when it fills the chunk and continues on both sides: head wins;
//   - to the chunk's TAIL slot, if it is the chunk's last destination and continues into the next chunk (entry e1 names it).
// Two slots of Dp = D rounded up to 4 scalars per chunk and side, written and read under matching conditions: never cleared.
//
// The boundary.  A row that crosses a seam is owned by the chunk in which it STARTS: that chunk's group adds the row's
// partials in chunk order -- its own tail slot, then the head slots of the following chunks ascending -- in float64 and is the
// row's only writer.  The last chunk that starts with the row is found by BISECTION over the chunk starts (sorted like the
// entries; chunk c + 1 starts with the row), so that the head-slot loads are independent: a walk, one dependent index load per
// chunk, was 0.5 ms over the 357 chunks of the most popular item of a 262 144-row minibatch.  A popular row is thus gathered
// by many groups in parallel; only its chunk partials, one per C contributions, are added serially.  Every row has one writer
// and every sum a fixed order -- entries in index order, slots in chunk order: the same bits on every run and device.  kAhead
// and kBatch change what is in flight, not what is added to what.
//
// The policy: a struct of kernel arguments (nothing of it lives in memory) with force-inlined members
//   Slot                          the slot scalar: float rounds every chunk partial to fp32, double keeps it
//   ahead<NC>(), batch<NC>()      kAhead; kBatch, the head slots the boundary loads before its first add (1: a sequential loop)
//   Entry, load(side, pos)        an entry's operands, read at its position clamped into [0, n2)
//   partner(side, entry, pos)     the partner row's id (the walk clamps it into the partner table)
//   valid(entry, y, n2)           does the entry count?  y is the position as the index holds it, unclamped
//   gathers(side, pos), factor(entry, pos)   what a counted entry adds to the destination's count; its partner row's fp32 factor
//   finish<NC, VEC>(table, row, D, count, l16, acc)   at the end of a destination; table: the destination's own
//   StartsRows, finish_row<NC, VEC>(table, side, starts, row, D, count, l16, acc)   optional, in finish's place where the
//                                 policy declares the member type StartsRows: `starts` says that the destination's FIRST
//                                 entry lies in this chunk -- true in exactly one of the chunks a destination spans, so what a
//                                 row must receive once whatever its length goes there (DICE's discrepancy gradient)
//   write_row<NC, VEC>(table, row, D, l16, acc)       static: a finished row into the gradient table (scatter and boundary)
#pragma once
#include <algorithm>
#include <type_traits>

#include "row_pass.hpp"

namespace invpref {

// ---- geometry
__host__ __device__ inline int chunk_of(int64_t n2) { return n2 <= 65536 ? 16 : 128; }
struct ChunkGeom {
    int C, nchunk, Dp;
    size_t slots;   // chunks per side the slot region has room for
    template <typename Slot>
    size_t part_bytes() const { return sizeof(Slot) * 2 * slots * 2 * (size_t)Dp; }   // two sides, head and tail
    unsigned grid() const { return (unsigned)((2 * nchunk + kGroups - 1) / kGroups); }   // one group per (side, chunk)
};
inline ChunkGeom chunk_geom(int64_t B, int64_t D) {
    ChunkGeom G;
    const int64_t n2 = 2 * B;
    G.C = chunk_of(n2);
    G.nchunk = (int)((n2 + G.C - 1) / G.C);
    G.Dp = (int)((D + 3) / 4 * 4);
    // (the chunk grows from 16 to 128 entries beyond 65 536 positions: keep the size non-decreasing across that step)
    G.slots = n2 <= 65536 ? (size_t)G.nchunk : (size_t)std::max(G.nchunk, 4096);
    return G;
}
// the head (tail = 0) or tail (tail = 1) slot of chunk c of a side
template <typename Slot>
__device__ __forceinline__ Slot *slot_of(Slot *part, int nchunk, int Dp, int side, int64_t c, int tail) {
    return part + (((int64_t)side * nchunk + c) * 2 + tail) * Dp;
}

// ---- a chunk slot: Dp scalars, 16-byte aligned (the entries beyond D are the zeros load_row filled in)
template <int NC>
__device__ __forceinline__ void zero_acc(double4_t (&v)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) v[c].x = v[c].y = v[c].z = v[c].w = 0.0;
}
template <int NC>
__device__ __forceinline__ void round_row(const double4_t (&v)[NC], float4 (&r)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) r[c] = make_float4((float)v[c].x, (float)v[c].y, (float)v[c].z, (float)v[c].w);
}
__device__ __forceinline__ void put4(float *p, const double4_t &v) {
    *reinterpret_cast<float4 *>(p) = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
}
__device__ __forceinline__ void put4(double *p, const double4_t &v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
template <int NC, typename Slot>
__device__ __forceinline__ void slot_store(Slot *__restrict__ slot, int Dp, int l16, const double4_t (&v)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int i0 = (l16 + kRow * c) * 4;
        if (i0 < Dp) put4(slot + i0, v[c]);
    }
}
__device__ __forceinline__ double4_t slot4(const float *p) {
    const float4 o = *reinterpret_cast<const float4 *>(p);
    return double4_t{(double)o.x, (double)o.y, (double)o.z, (double)o.w};
}
__device__ __forceinline__ double4_t slot4(const double *p) { return double4_t{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void add4(double4_t &a, const double4_t &b) {
    a.x = a.x + b.x; a.y = a.y + b.y; a.z = a.z + b.z; a.w = a.w + b.w;
}
template <int NC, typename Slot>
__device__ __forceinline__ void slot_add(const Slot *__restrict__ slot, int Dp, int l16, double4_t (&v)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int i0 = (l16 + kRow * c) * 4;
        if (i0 < Dp) add4(v[c], slot4(slot + i0));
    }
}
// a slot's values without a branch: a lane beyond Dp reads the slot's first entries and keeps zeros
template <int NC, typename Slot>
__device__ __forceinline__ void slot_load(const Slot *__restrict__ slot, int Dp, int l16, double4_t (&v)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int i0 = (l16 + kRow * c) * 4;
        const bool in = i0 < Dp;
        const double4_t o = slot4(slot + (in ? i0 : 0));
        v[c].x = in ? o.x : 0.0; v[c].y = in ? o.y : 0.0; v[c].z = in ? o.z : 0.0; v[c].w = in ? o.w : 0.0;
    }
}

// acc += k * r in float64 by fma: k and r hold fp32 values, so the product is exact and these are axpy_row's bits (row_pass.hpp)
template <int NC>
__device__ __forceinline__ void fma_row(double4_t (&acc)[NC], float k, const float4 (&r)[NC]) {
    const double kd = (double)k;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        acc[c].x = __builtin_fma(kd, (double)r[c].x, acc[c].x);
        acc[c].y = __builtin_fma(kd, (double)r[c].y, acc[c].y);
        acc[c].z = __builtin_fma(kd, (double)r[c].z, acc[c].z);
        acc[c].w = __builtin_fma(kd, (double)r[c].w, acc[c].w);
    }
}

// does the policy ask which chunk a destination STARTS in?  (a member type StartsRows: DICE's pass alone)
template <typename Policy, typename = void>
struct starts_rows : std::false_type {};
template <typename Policy>
struct starts_rows<Policy, std::void_t<typename Policy::StartsRows>> : std::true_type {};

__device__ __forceinline__ int clamp_id(int id, int n) { return min(max(id, 0), n - 1); }
__device__ __forceinline__ int64_t clamp_id(int64_t id, int n) { return std::min<int64_t>(std::max<int64_t>(id, 0), n - 1); }

// ---- the scatter: the body of a __launch_bounds__(256) kernel on ChunkGeom::grid() workgroups
template <int NC, bool VEC, typename Policy>
__device__ __forceinline__ void chunk_scatter(const Policy &pol, const float *__restrict__ Pu, int U, const float *__restrict__ Qi,
                                              int I, int D, int B, const int2 *__restrict__ index, int64_t stride, int C,
                                              int nchunk, float *__restrict__ gu, float *__restrict__ gi,
                                              typename Policy::Slot *__restrict__ part, int Dp) {
    using Entry = typename Policy::Entry;
    const int l16 = threadIdx.x & (kRow - 1);
    const int grp = (int)blockIdx.x * kGroups + threadIdx.x / kRow;
    if (grp >= 2 * nchunk) return;
    const int side = grp >= nchunk ? 1 : 0, c = grp - side * nchunk;
    const int n2 = 2 * B;
    const int2 *idx = index + side * stride;
    const int lim = side ? I : U, plim = side ? U : I;
    const float *ptab = side ? Pu : Qi, *dtab = side ? Qi : Pu;   // the partner's table, the destination's
    float *gtab = side ? gi : gu;
    const int e0 = c * C, e1 = min(e0 + C, n2);
    const int first = idx[e0].x;
    if (first < 0 || first >= lim) return;   // the sentinel destination sorts last: nothing left in this list
    const bool head0 = c > 0 && idx[e0 - 1].x == first;
    const int next_id = e1 < n2 ? idx[e1].x : -1;
    double4_t acc[NC];
    zero_acc<NC>(acc);
    int cur = first, cnt = 0;
    bool cur_head = head0, live = true;
    auto flush = [&](bool head, bool tail) {
        if constexpr (starts_rows<Policy>::value) pol.template finish_row<NC, VEC>(dtab, side, !head, cur, D, cnt, l16, acc);
        else pol.template finish<NC, VEC>(dtab, cur, D, cnt, l16, acc);
        if (!head && !tail) Policy::template write_row<NC, VEC>(gtab, cur, D, l16, acc);
        else slot_store<NC>(slot_of(part, nchunk, Dp, side, c, head ? 0 : 1), Dp, l16, acc);
    };
    constexpr int kAhead = Policy::template ahead<NC>();
    for (int e = e0; e < e1 && live; e += kAhead) {
        int2 en[kAhead];
        int pos[kAhead];
        Entry op[kAhead];
        float4 rows[kAhead][NC];
        // three stages, each a batch of independent loads: merged into one loop they would serialise index -> operands -> row
#pragma unroll
        for (int j = 0; j < kAhead; j++) en[j] = idx[min(e + j, e1 - 1)];
#pragma unroll
        for (int j = 0; j < kAhead; j++) {
            pos[j] = min(max(en[j].y, 0), n2 - 1);
            op[j] = pol.load(side, pos[j]);
        }
#pragma unroll
        for (int j = 0; j < kAhead; j++)
            load_row<NC, VEC>(ptab, clamp_id(pol.partner(side, op[j], pos[j]), plim), D, l16, rows[j]);
#pragma unroll
        for (int j = 0; j < kAhead; j++) {
            if (!live || e + j >= e1) continue;
            const int dest = en[j].x;
            if (dest < 0 || dest >= lim) {   // the sentinel destination, from here to the end of the list
                live = false;
                continue;
            }
            if (dest != cur) {
                flush(cur_head, false);
                zero_acc<NC>(acc);
                cur = dest;
                cnt = 0;
                cur_head = false;
            }
            if (!pol.valid(op[j], en[j].y, n2)) continue;
            cnt += pol.gathers(side, pos[j]);
            fma_row<NC>(acc, pol.factor(op[j], pos[j]), rows[j]);
        }
    }
    flush(cur_head, live && next_id == cur);
}

// ---- the boundary: the same launch
template <int NC, bool VEC, typename Policy>
__device__ __forceinline__ void chunk_boundary(const int2 *__restrict__ index, int64_t stride, int B, int C, int nchunk, int U,
                                               int I, int D, int Dp, const typename Policy::Slot *__restrict__ part,
                                               float *__restrict__ gu, float *__restrict__ gi) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int grp = (int)blockIdx.x * kGroups + threadIdx.x / kRow;
    if (grp >= 2 * nchunk) return;
    const int side = grp >= nchunk ? 1 : 0, c = grp - side * nchunk;
    const int n2 = 2 * B;
    const int2 *idx = index + side * stride;
    const int lim = side ? I : U;
    const int e0 = c * C, e1 = min(e0 + C, n2);
    if (e1 >= n2) return;
    const int last = idx[e1 - 1].x;
    if (last < 0 || last >= lim || idx[e1].x != last) return;          // nothing continues into the next chunk
    if (c > 0 && idx[e0].x == last && idx[e0 - 1].x == last) return;   // it started earlier: that chunk's group owns the row
    double4_t sum[NC];
    zero_acc<NC>(sum);
    slot_add<NC>(slot_of(part, nchunk, Dp, side, c, 1), Dp, l16, sum);
    int lo = c + 1, hi = nchunk - 1;   // the last chunk that starts with this row
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (idx[(int64_t)mid * C].x == last) lo = mid;
        else hi = mid - 1;
    }
    int cc = c + 1;
    constexpr int kBatch = Policy::template batch<NC>();
    if constexpr (kBatch > 1) {
        // kBatch head slots loaded before the first is added: the order of the sum is the sequential loop's, and the loads are
        // straight-line code (slot_load: no branch around a load), so they are in flight together
        for (; cc + kBatch - 1 <= lo; cc += kBatch) {
            double4_t v[kBatch][NC];
#pragma unroll
            for (int j = 0; j < kBatch; j++) slot_load<NC>(slot_of(part, nchunk, Dp, side, cc + j, 0), Dp, l16, v[j]);
#pragma unroll
            for (int j = 0; j < kBatch; j++) {
#pragma unroll
                for (int k = 0; k < NC; k++) add4(sum[k], v[j][k]);
            }
        }
    }
    for (; cc <= lo; cc++) slot_add<NC>(slot_of(part, nchunk, Dp, side, cc, 0), Dp, l16, sum);
    Policy::template write_row<NC, VEC>(side ? gi : gu, last, D, l16, sum);
}

// ---- the regularised walk: what the passes with L2_coe * L2_reg + L1_coe * L1_reg in their loss share (BPR, doubly robust)
// a row's squares and absolute values added to the pairs launch's float64 sums, each lane's chunks in order
template <int NC>
__device__ __forceinline__ void norms64(const float4 (&r)[NC], double &sq, double &ab) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        sq = sq + (double)r[c].x * (double)r[c].x;
        sq = sq + (double)r[c].y * (double)r[c].y;
        sq = sq + (double)r[c].z * (double)r[c].z;
        sq = sq + (double)r[c].w * (double)r[c].w;
        ab = ab + fabs((double)r[c].x);
        ab = ab + fabs((double)r[c].y);
        ab = ab + fabs((double)r[c].z);
        ab = ab + fabs((double)r[c].w);
    }
}
// one entry's regulariser gradient: n2 = n * 2 L2_coe / (B D), n1 = n * L1_coe / (B D)
__device__ __forceinline__ double reg_of(double x, double n2, double n1) {
    return n2 * x + n1 * (x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0));   // (a NaN entry: n2 * NaN)
}

// The policy base of such a pass.  The pass's own struct derives from it and adds Entry, load, partner, valid, gathers, factor
// and the fields they read; gathers() says which of the entries added gather the destination row, and so count for `cnt` below.
struct RegWalk {
    using Slot = double;   // a row is rounded to fp32 once however many chunks it spans
    // entries whose index -> ids -> row chain is in flight together (8 NC + 8 registers per entry next to the 8 NC of the
    // float64 accumulator: eight entries of 128-float rows took all 256 registers and left one wave per SIMD)
    template <int NC>
    static constexpr int ahead() { return NC == 1 ? 8 : 4; }
    template <int NC>
    static constexpr int batch() { return 16 / NC; }
    double r2, r1;   // 2 L2_coe / (B D), L1_coe / (B D)

    // acc += cnt * regulariser gradient of the destination row
    template <int NC, bool VEC>
    __device__ __forceinline__ void finish(const float *__restrict__ dtab, int row, int D, int cnt, int l16,
                                           double4_t (&acc)[NC]) const {
        float4 d[NC];
        load_row<NC, VEC>(dtab, row, D, l16, d);
        const double n2r = (double)cnt * r2, n1r = (double)cnt * r1;
#pragma unroll
        for (int k = 0; k < NC; k++) {
            acc[k].x = acc[k].x + reg_of((double)d[k].x, n2r, n1r);
            acc[k].y = acc[k].y + reg_of((double)d[k].y, n2r, n1r);
            acc[k].z = acc[k].z + reg_of((double)d[k].z, n2r, n1r);
            acc[k].w = acc[k].w + reg_of((double)d[k].w, n2r, n1r);
        }
    }
    // rounded once and stored: the tables are zero-filled in front, the writers never read them
    template <int NC, bool VEC>
    static __device__ __forceinline__ void write_row(float *__restrict__ gtab, int row, int D, int l16, const double4_t (&acc)[NC]) {
        float4 r[NC];
        round_row<NC>(acc, r);
        store_row<NC, VEC>(gtab, row, D, l16, r);
    }
};

// ---- the triplet walk: the policy of a pass over 2 B signed positions, (u, i+, +g) at p and (u, j-, -g) at B + p -- BPR's
// pass (LightGCN trains through it too) and, per pair of tables, DICE's
// do all three ids of a triplet lie in their tables?  The passes skip a triplet whole (neg = -1 included) where they do not
__device__ __forceinline__ bool triplet_ok(int64_t u, int64_t i, int j, int U, int I) {
    return u >= 0 && u < U && i >= 0 && i < I && j >= 0 && j < I;
}
// Fetch: a functor of kernel arguments, fetch(p) the factor g of triplet p as its pairs launch recorded it
template <typename Fetch>
struct TripletWalk : RegWalk {
    struct Entry {
        int64_t u, i;   // the triplet's three ids and its g
        int j;
        float g;
    };
    int U, I, B;
    const int64_t *__restrict__ users, *__restrict__ pos_items;
    const int32_t *__restrict__ neg;
    Fetch fetch;

    __device__ __forceinline__ Entry load(int, int pos) const {
        const int p = pos < B ? pos : pos - B;
        return Entry{users[p], pos_items[p], neg[p], fetch(p)};
    }
    __device__ __forceinline__ int64_t partner(int side, const Entry &e, int pos) const {
        return side ? e.u : (pos < B ? e.i : (int64_t)e.j);
    }
    // the whole triplet decides, not the pair: a bad negative silences the positive's position too.  (!triplet_ok() written
    // out in one chain with the position's range: through the call the scatter kernels are compiled to other code)
    __device__ __forceinline__ bool valid(const Entry &e, int y, int n2) const {
        return !(y < 0 || y >= n2 || e.u < 0 || e.u >= U || e.i < 0 || e.i >= I || e.j < 0 || e.j >= I);
    }
    // (a triplet gathers its user row once: the user side counts position p only)
    __device__ __forceinline__ int gathers(int side, int pos) const { return (side || pos < B) ? 1 : 0; }
    __device__ __forceinline__ float factor(const Entry &e, int pos) const { return pos < B ? e.g : -e.g; }
};

}  // namespace invpref
