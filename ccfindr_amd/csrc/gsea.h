// gsea.h -- gfx950 kernels behind assign_celltype: the enrichment score of every (permutation, cluster, gene set) of the
// reference's p-value loop in one launch per chunk of permutations (included once, by gsea.hip).
//
// Reference: gsea() (R/gsea.R:79-115) as assignCelltype() calls it nperm + 1 times (:57, :65-72), for one cluster k, one set s:
//   :92-94   the rows of the (permuted) meta table whose weight is not NA, in table order                 -> valid, rank
//   :95      x = overlap(gl, gs): the hit flags (:117-128), formed once on the host                        -> hit_row
//   :96-99   no hit: NA                                                                                    -> NaN, on the host
//   :100-102 phit = cumsum(x * gw^p) / its last value                                                      -> C_t / C_last
//   :104-106 pmiss = cumsum(!(gl %in% gs)) / its last value M                                              -> (rank_t - notmiss_t) / M
//   :108     ES = max(phit - pmiss) over all rows
//   :69      Ep += (ES < x), strict                                                                        -> k_gsea_count
//
// What the kernel rests on: a row that is no hit is a miss, and between two hits phit - pmiss cannot rise (correctly rounded
// division and subtraction are monotone), so the maximum over all rows is attained at a hit row or is the last row's value
// C_last / C_last - M / M.  x * gw^p adds exact zeros between the hits, so adding the hits' gw^p alone, in table order, gives the
// bits of the reference's cumsum.  A hit needs its rank among the non-NA rows (1-based) and the number of hits up to and
// including it that are no misses (a gene matched only through a group prefix is both, :104 tests the literal set):
//   dev_t = C_t / C_last - (rank_t - notmiss_t) / M,   ES = max(dev_1 .. dev_T, C_last / C_last - M / M),  NaN if any term is.
//
// The permutations arrive INVERTED: inv[b][row] = the position of meta-table row `row` in permutation b (the host forms the
// inverse while it checks that each row of `perms` is a permutation: no index of this kernel comes unchecked from the caller).
// A hit's position is then one load, and nothing walks the N positions of a cluster without NA rows: rank = position + 1.
// A cluster WITH NA rows gets, per (b, k), a bit per position (valid[k][perms[b][pos]], a wave's ballot per 64 positions) and
// the exclusive popcount prefix of the 64-bit words, in the workgroup's own stretch of a global scratch buffer; a hit's rank
// is prefix[pos / 64] + popcount(word & bits up to pos).  Only then are the permutations themselves on the device as well.
//
// One workgroup of kGseaThreads = 256 takes the work items (b, k) = item / r, item % r in grid strides; the sets of a cluster one
// after the other:
//   1. the set's T hits: (position, index in the set) pairs into LDS, padded to a power of two P with keys 0xFFFFFFFF;
//   2. a bitonic sort of the pairs by position (distinct keys: the result does not depend on the network);
//   3. in sorted order: gw^p -> C[j], rank -> key[j], "no miss" -> flag[j];
//   4. ONE thread adds C and the flags left to right, in place: the order of the fp64 additions is the reference's;
//   5. every thread takes dev_t of its hits; maximum by a NaN-propagating max (exact, so its order does not matter).
// LDS per workgroup: 64 + 14 P bytes (8 C, 4 key, 2 flag) for the largest set of the call, at most 64 + 14 * 4096 = 57408: a plain
// launch.  Sets of more than kGseaMaxSetHits = 4096 hits are refused by the host (VBNMF_ERR_BAD_ARG) -- except sets with M = 0
// (a set holding every gene), which are NaN by :106 whatever their size and never reach the kernel's sort.
// (b, k, s) with T = 0 or M = 0: NaN written, nothing computed.
//
// No floating-point atomics and no order that depends on the grid: the same inputs give the same bits on every call.  Every
// loop is bounded by N, T, P or the item count; every index is checked by the host (gsea.hip, gsea_check) before the launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vbnmf {

constexpr int kGseaWave = 64;
constexpr int kGseaThreads = 256;
constexpr int kGseaWaves = kGseaThreads / kGseaWave;
constexpr int kGseaMaxSetHits = 4096;          // hits of one set the workgroup sorts in LDS
constexpr int kGseaLdsFixed = 64;              // 4 doubles of wave maxima, 4 ints of wave totals, padding
constexpr int kGseaLdsPerHit = 14;
static_assert(kGseaLdsFixed + kGseaLdsPerHit * kGseaMaxSetHits <= 65536, "the sort must fit the LDS of a plain launch");
static_assert((kGseaMaxSetHits & (kGseaMaxSetHits - 1)) == 0 && kGseaMaxSetHits <= 65536, "a power of two whose indices fit 16 bits");

struct GseaArgs {
    int64_t N;                     // rows of the meta table
    int32_t r, nS;
    int32_t nb;                    // permutations of this launch
    int32_t pad;                   // P of the largest set that is computed (a power of two >= 1)
    const int32_t *inv;            // [nb x N] position of every row; NULL: the identity (the observed scores)
    const int32_t *perms;          // [nb x N] row at every position; read for clusters with NA rows only; NULL with inv NULL
    const uint8_t *valid;          // [r x N]
    const uint8_t *has_na;         // [r] some row of the cluster is not valid
    const double *wp;              // [r x N] gw^p
    const int64_t *hit_ptr;        // [r x nS + 1] over (k, s), k major
    const int32_t *hit_row;        // the hits of (k, s), rows ascending
    const uint8_t *hit_is_miss;    // ... 1: the row is also a miss
    const int32_t *M;              // [r x nS] misses among the valid rows; 0 or no hit: the score is NaN
    unsigned long long *words;     // [grid x nW] scratch, nW = ceil(N / 64): validity of the positions (clusters with NA rows)
    int32_t *prefix;               // [grid x nW] ... valid positions before the word
    double *out;                   // [nb x nS x r]
};

// max as R's and numpy's: NaN if either is
__device__ inline double gsea_max(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (a > b ? a : b); }

__global__ __launch_bounds__(kGseaThreads) void k_gsea_perm(const GseaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char gsea_smem[];
    double *s_red = reinterpret_cast<double *>(gsea_smem);                                 // [4] wave maxima
    int *s_tot = reinterpret_cast<int *>(gsea_smem + 32);                                  // [4] wave totals of the prefix scan
    double *s_c = reinterpret_cast<double *>(gsea_smem + kGseaLdsFixed);                   // [pad]
    unsigned int *s_key = reinterpret_cast<unsigned int *>(s_c + A.pad);                   // [pad]
    unsigned short *s_idx = reinterpret_cast<unsigned short *>(s_key + A.pad);             // [pad]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t N = A.N;
    const int64_t nW = (N + 63) >> 6;
    unsigned long long *words = A.words + (int64_t)blockIdx.x * nW;
    int32_t *prefix = A.prefix + (int64_t)blockIdx.x * nW;
    const int64_t items = (int64_t)A.nb * A.r;

    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / A.r;
        const int k = (int)(item - b * A.r);
        const int32_t *inv = A.inv ? A.inv + b * N : nullptr;
        const uint8_t *valid = A.valid + (int64_t)k * N;
        const double *wp = A.wp + (int64_t)k * N;
        const bool na = A.has_na[k] != 0;                                                  // (block-uniform)

        if (na) {
            // a bit per position: is the row that stands there valid
            const int32_t *perm = A.perms ? A.perms + b * N : nullptr;
            for (int64_t w = wave; w < nW; w += kGseaWaves) {
                const int64_t pos = (w << 6) + lane;
                bool v = false;
                if (pos < N) v = valid[perm ? perm[pos] : pos] != 0;
                const unsigned long long bits = __ballot(v);
                if (lane == 0) words[w] = bits;
            }
            __syncthreads();
            // exclusive prefix of the words' popcounts: a contiguous stretch per thread, a scan of the threads' totals
            const int64_t per = (nW + kGseaThreads - 1) / kGseaThreads;
            const int64_t w0 = t * per < nW ? t * per : nW, w1 = w0 + per < nW ? w0 + per : nW;
            int tot = 0;
            for (int64_t w = w0; w < w1; w++) tot += __popcll(words[w]);
            int incl = tot;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(incl, off);
                if (lane >= off) incl += o;
            }
            if (lane == 63) s_tot[wave] = incl;
            __syncthreads();
            int run = incl - tot;
            for (int q = 0; q < wave; q++) run += s_tot[q];
            for (int64_t w = w0; w < w1; w++) { prefix[w] = run; run += __popcll(words[w]); }
            __syncthreads();
        }

#pragma unroll 1
        for (int s = 0; s < A.nS; s++) {
            const int64_t ks = (int64_t)k * A.nS + s;
            const int64_t h0 = A.hit_ptr[ks];
            const int T = (int)(A.hit_ptr[ks + 1] - h0);
            const int M = A.M[ks];
            double *out = A.out + ((int64_t)b * A.nS + s) * A.r + k;
            if (T == 0 || M == 0) {                                                        // (block-uniform) :96-99, :106
                if (t == 0) *out = __builtin_nan("");
                continue;
            }
            int P = 1;
            while (P < T) P <<= 1;                                                         // <= A.pad (host)
            // 1. (position, index) pairs
            for (int j = t; j < P; j += kGseaThreads) {
                unsigned int key = 0xFFFFFFFFu;
                if (j < T) {
                    const int32_t row = A.hit_row[h0 + j];
                    key = (unsigned int)(inv ? inv[row] : row);
                }
                s_key[j] = key;
                s_idx[j] = (unsigned short)j;
            }
            __syncthreads();
            // 2. bitonic sort by position
            for (int kk = 2; kk <= P; kk <<= 1) {
                for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                    for (int i = t; i < P; i += kGseaThreads) {
                        const int l = i ^ jj;
                        if (l > i) {
                            const unsigned int a = s_key[i], c = s_key[l];
                            const bool up = (i & kk) == 0;
                            if ((a > c) == up && a != c) {
                                const unsigned short ia = s_idx[i], ic = s_idx[l];
                                s_key[i] = c; s_key[l] = a;
                                s_idx[i] = ic; s_idx[l] = ia;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            // 3. in sorted order: the weight, the rank among the valid rows, the "no miss" flag
            for (int j = t; j < T; j += kGseaThreads) {
                const int64_t h = h0 + s_idx[j];
                const unsigned int pos = s_key[j];
                unsigned int rank = pos + 1u;
                if (na) {
                    const unsigned long long upto = words[pos >> 6] & (~0ull >> (63 - (pos & 63u)));
                    rank = (unsigned int)prefix[pos >> 6] + (unsigned int)__popcll(upto);
                }
                s_c[j] = wp[A.hit_row[h]];
                s_key[j] = rank;
                s_idx[j] = A.hit_is_miss[h] ? 0 : 1;
            }
            __syncthreads();
            // 4. the running sums, left to right (R/gsea.R:101, :105)
            if (t == 0) {
                double c = 0.0;
                unsigned int nm = 0;
                for (int j = 0; j < T; j++) {
                    c += s_c[j];
                    nm += s_idx[j];
                    s_c[j] = c;
                    s_idx[j] = (unsigned short)nm;
                }
            }
            __syncthreads();
            // 5. the maximum of phit - pmiss over the hits and the last row (:102, :106, :108)
            const double clast = s_c[T - 1], md = (double)M;
            double best = -__builtin_inf();
            for (int j = t; j < T; j += kGseaThreads) {
                const double dev = s_c[j] / clast - (double)(s_key[j] - (unsigned int)s_idx[j]) / md;
                best = gsea_max(best, dev);
            }
            if (t == 0) best = gsea_max(best, clast / clast - md / md);
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) best = gsea_max(best, __shfl_xor(best, off));
            if (lane == 0) s_red[wave] = best;
            __syncthreads();
            if (t == 0) *out = gsea_max(gsea_max(s_red[0], s_red[1]), gsea_max(s_red[2], s_red[3]));
            // (the next set's step 1 writes s_key / s_idx only, which every thread is done reading; s_red is written again
            // after that set's barriers, which thread 0 reaches after this read)
        }
        __syncthreads();                                                                   // words / prefix are free for the next item
    }
}

// exceed[q] += number of the chunk's permutations with es[q] < null[b][q] (R/gsea.R:69, strict; integer arithmetic, one thread
// per (s, k): no atomics).  es[q] NaN: left alone (the host writes -1).
__global__ __launch_bounds__(kGseaThreads) void k_gsea_count(const double *es, const double *null_es, int32_t nb, int64_t nq, long long *exceed)
{
    const int64_t q = (int64_t)blockIdx.x * kGseaThreads + threadIdx.x;
    if (q >= nq) return;
    const double x = es[q];
    if (x != x) return;
    long long c = 0;
    for (int32_t b = 0; b < nb; b++) c += x < null_es[(int64_t)b * nq + q] ? 1 : 0;
    exceed[q] += c;
}

}  // namespace vbnmf
