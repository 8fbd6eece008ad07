// launch.hpp -- the host side of every launch: argument checks of a table set, the run-time value -> kernel instance
// dispatch, the LDS attribute, and the scalars the entry points form for the kernels.  No device code.
#pragma once
#include <math.h>

#include <type_traits>

#include "kernel_common.hpp"

namespace invpref {

// ---- value dispatch: a run-time bool / int becomes a compile-time one.  `f` is a generic lambda taking the value as
// std::true_type / std::false_type / std::integral_constant<int, V> (read it with decltype(v)::value) and returning an int
// status, which is returned.  An int outside the list launches nothing: INVPREF_EUNSUPPORTED.  A combination that has no
// kernel is cut with `if constexpr` on the dispatched values, so that its branch never names one.
template <typename F>
int with_bool(bool v, F &&f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}
template <int... Vs, typename F>
int with_int(int v, F &&f) {
    int rc = INVPREF_EUNSUPPORTED;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}

// more than 64 KB of dynamic LDS has to be asked for, per kernel
template <typename K>
hipError_t ensure_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// the largest row count or list length an entry point that indexes with int takes
constexpr int64_t kI32Max = 2147483647;

inline int check_tables(const InvPrefTables *t, bool pure_mf = false) {
    if (!t) return INVPREF_EINVAL;
    if (t->user_num <= 0 || t->item_num <= 0 || t->env_num <= 0 || t->factor_num <= 0) return INVPREF_EINVAL;
    if (t->factor_num > INVPREF_MAX_FACTORS || t->env_num > INVPREF_MAX_ENVS) return INVPREF_EUNSUPPORTED;
    if (!t->embed_user_invariant || !t->embed_item_invariant) return INVPREF_EINVAL;
    if (pure_mf) return t->env_num == 1 ? 0 : INVPREF_EINVAL;  // INVPREF_PURE_MF: the other five tables are ignored
    if (!t->embed_user_env_aware || !t->embed_item_env_aware || !t->embed_env || !t->classifier_weight ||
        !t->classifier_bias)
        return INVPREF_EINVAL;
    return 0;
}
inline DevTables dev_tables(const InvPrefTables *t) {
    return DevTables{t->embed_user_invariant, t->embed_item_invariant, t->embed_user_env_aware, t->embed_item_env_aware,
                     t->embed_env, t->classifier_weight, t->classifier_bias,
                     (int)t->user_num, (int)t->item_num, (int)t->env_num, (int)t->factor_num};
}
inline DevGrads dev_grads(const InvPrefTables *t) {
    return DevGrads{t->embed_user_invariant, t->embed_item_invariant, t->embed_user_env_aware, t->embed_item_env_aware,
                    t->embed_env, t->classifier_weight, t->classifier_bias};
}
// rows of D floats of these tables can be read as float4 (null pointers count as aligned)
template <typename... P>
bool rows_vec_ok(int64_t D, const P *...tables) {
    return D % 4 == 0 && ((... | reinterpret_cast<uintptr_t>(tables)) & 15u) == 0;
}
inline bool vec_ok(const InvPrefTables *t) {
    return rows_vec_ok(t->factor_num, t->embed_user_invariant, t->embed_item_invariant, t->embed_user_env_aware,
                       t->embed_item_env_aware);
}
inline int nc_of(int D) { return D <= 64 ? 1 : (D <= 128 ? 2 : 4); }
inline int emax_of(int E) { return E <= 4 ? 4 : (E <= 8 ? 8 : 16); }
// with_int / with_bool for kernels over rows of D floats: `f` takes the float4 chunks per lane and whether rows are read as float4
template <typename F>
int with_row_shape(int D, bool vec, F &&f) {
    return with_int<1, 2, 4>(nc_of(D), [&](auto nc_c) { return with_bool(vec, [&](auto vec_c) { return f(nc_c, vec_c); }); });
}

inline int64_t up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
// carves a workspace into parts, every part 16-byte aligned: take() returns the offset of the next part, bytes() the size so far
struct Carver {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += (size_t)up((int64_t)bytes, 16);
        return o;
    }
    size_t bytes() const { return at; }
};

// one row of the device-side schedule, as laid out in include/invpref_hip.h (InvPrefAdamSchedule); the kernels read it too
struct SchedRow {
    AdamScalars ad;
    float alpha;   // gradient-reversal alpha of the step; NaN: use the one of the call's coefficient block
    float pad;
};

inline AdamScalars adam_scalars(int64_t step, double lr, double beta1, double beta2, double eps) {
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    AdamScalars ad;
    ad.step_size = (float)(lr / bc1);
    ad.bc2_sqrt = (float)sqrt(bc2);
    ad.w1 = (float)(1.0 - beta1);
    ad.b2 = (float)beta2;
    ad.w2 = (float)(1.0 - beta2);
    ad.eps = (float)eps;
    return ad;
}

inline StepScalars step_scalars(const InvPrefCoefs *coefs, int64_t batch_norm, int D) {
    StepScalars k;
    k.ca = coefs->invariant_coe; k.cb = coefs->env_aware_coe; k.cc = coefs->env_coe; k.alpha = coefs->alpha;
    k.invB = 1.0f / (float)batch_norm;
    k.r2 = coefs->L2_coe / ((float)batch_norm * (float)D);
    k.r1 = coefs->L1_coe / (2.0f * (float)batch_norm * (float)D);
    return k;
}

}  // namespace invpref
