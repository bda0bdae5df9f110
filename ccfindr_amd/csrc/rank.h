// rank.h -- the padded ranks the kernel families are compiled for, and the run-time dispatch onto them (host side; shared by
// the .hip units that launch rank-templated kernels).
#pragma once
#include <type_traits>

#include "common.h"

namespace vbnmf {

// ---- dispatch over the padded rank (compile-time so factor rows live in registers) ----
#define VBNMF_FOR_EACH_R_UP_TO_64(X) \
    X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(22) X(24) X(26) X(28) X(30) X(32) \
    X(40) X(48) X(56) X(64)
// every padded rank: up to 32 by 2 (one lane per task), 40..64 by 8 (two lanes), 80..128 by 16 (four lanes)
#ifdef VBNMF_DEV_FEW_RANKS              /* development builds only: a few ranks, for a compile check in a minute */
#define VBNMF_FOR_EACH_R(X) X(4) X(6) X(8) X(10) X(20) X(48) X(80)
#define VBNMF_FOR_EACH_R_BATCH(X) X(4) X(6) X(8) X(10)
#else
#define VBNMF_FOR_EACH_R(X) VBNMF_FOR_EACH_R_UP_TO_64(X) X(80) X(96) X(112) X(128)
#define VBNMF_FOR_EACH_R_BATCH(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16)
#endif
constexpr int kBatchMaxPaddedRank = 16;      // the small-matrix regime the batch is for (instantiations cost build time)
static_assert(rank_shares(kBatchMaxPaddedRank) == 1, "the batch sweeps have no form that shares a rank among lanes");

// f(std::integral_constant<int, R>{}) for the padded rank R of one of the lists above; returns f's status.  The lists are
// expanded here and nowhere else: with_rank serves every rank, with_rank_up_to_64 the truncated SVD's dense kernels,
// with_batch_rank the kernels that step a batch of engines.
#define X(RR) case RR: return f(std::integral_constant<int, RR>{});
template <class F>
int with_rank(int R, F &&f)
{
    switch (R) {
        VBNMF_FOR_EACH_R(X)
        default: return fail(VBNMF_ERR_BAD_ARG, "unsupported padded rank %d", R);
    }
}

template <class F>
int with_rank_up_to_64(int R, F &&f)
{
    switch (R) {
        VBNMF_FOR_EACH_R_UP_TO_64(X)
        default: return fail(VBNMF_ERR_BAD_ARG, "unsupported padded rank %d", R);
    }
}

template <class F>
int with_batch_rank(int R, F &&f)
{
    switch (R) {
        VBNMF_FOR_EACH_R_BATCH(X)
        default: return fail(VBNMF_ERR_BAD_ARG, "a batch serves padded ranks up to %d (this engine: %d)", kBatchMaxPaddedRank, R);
    }
}
#undef X

// f(std::true_type{}) or f(std::false_type{}): a run-time switch as a template argument
template <class F>
int with_flag(bool on, F &&f)
{
    return on ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace vbnmf
