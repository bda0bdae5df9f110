// qc.h -- gfx950 kernel behind filter_genes: per-gene statistics of the count matrix in one launch over the genes' rows
// (included once, by qc.hip).
//
// Reference: what filter_genes() needs of every gene (R/utils.R:134-194):
//   :139      ncexpr_i = number of stored entries of row i                                              -> nnz
//   :199      gmean_i  = rowMeans = sum_i / m                                                           -> sum (mu = sum / m here, one division)
//   :211-212, :343   sum_j (x_ij - mu_i)^2 over all m cells (calc_vmr divides it by m, rowVars by m - 1) -> ss
//   :329-339  has_mode(row i)                                                                           -> mode
// ss is the centred form, as the reference has it, not sum x^2 - m mu^2: sum over the stored entries of (x - mu)^2, plus
// (m - nnz) mu^2 for the cells that hold a zero.
//
// has_mode, as its code runs (not as its comment says): table(g) counts every distinct value of the WHOLE row, zeros included
// (`tb[names(tb)]` removes nothing); the levels are the values that are present, ascending; the result is TRUE iff some present
// level has fewer occurrences than the next present level (FALSE with fewer than two levels).  A value that does not occur is no
// level: {5: 4 cells, 9: 3 cells, 0: the rest} compares 0 with 5 and 5 with 9, never 8 with 9.  The zeros' level has m - nnz
// occurrences and is absent when that is 0.  The kernel decides rows whose values are all integers in [1, bins); any other row
// (non-integer, negative, too large) gets mode = 2 and the host finishes it with an exact sort-and-count (host.cpp).
//
// Input: the values grouped by gene (rowptr, val), as doubles -- the column indices are not needed.  (Integer counts packed
// into 2-byte words ran the kernel no faster and cost the host more than the shorter upload saved: profiles/qc_times.txt.)
//
// Two row classes.  A persistent grid of 256-thread workgroups pulls TICKETS through a counter; a ticket is kQcTicketRows = 4
// consecutive rows, one per wave.
//   short (nnz <= kQcShortMax = 64): the row's wave takes it alone, one entry per lane, no LDS and no barrier.  The occurrence
//     table is formed in the wave: every lane counts the lanes that hold its value and finds the next larger value present and
//     that one's count (one walk over the row with v_readlane).
//   long: the workgroup takes the ticket's long rows one after the other, kQcPassEntries = 256 entries a pass.  The occurrence
//     table is an LDS histogram of `bins` 32-bit counters filled with LDS integer adds (order-independent: deterministic).  The
//     scan over the present bins gives every thread a contiguous stretch of [1, largest value]; a thread reports its stretch's
//     first and last non-empty counts, and wave 0 carries the last non-empty count across the threads (a scan with the operator
//     "the right operand unless it is empty").  The stretch is cleared as it is read, so the table costs O(largest value) a row.
//
// Order of every floating-point sum (it depends on the row alone -- not on the grid, the ticket or the other rows): entry e of a
// row belongs to lane e (short) or thread e mod 256 (long); a thread adds its entries in ascending order; the lanes of a wave
// are added by xor butterflies (offsets 1, 2, .. 32), the four waves of a long row in order 0..3.  No floating-point atomics:
// the same input gives the same bits on every run.  Every loop is bounded by an entry or bin count.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vbnmf {

constexpr int kQcThreads = 256;
constexpr int kQcWaves = kQcThreads / 64;
constexpr int kQcTicketRows = kQcWaves;        // rows of one ticket: one per wave
constexpr int kQcShortMax = 64;                // longest row a wave takes alone
constexpr int kQcPassEntries = kQcThreads;     // entries of a long row per pass of the workgroup
constexpr int kQcDefaultBins = 4096;           // 16 KB of LDS: eight workgroups a CU
// LDS: 2 x 4 doubles of wave partials, 2 x 256 stretch reports, 4 + 4 + 4 + 4 words (flags, largest values, ticket), then the
// table.  All of it sits in the dynamic region (16-byte aligned base, nothing static in front of it), within the 64 KB a launch
// may ask for without opting in.
constexpr int kQcLdsFixed = 64 + 2 * 4 * kQcThreads + 64;
constexpr int kQcMaxBins = 15360;
static_assert(kQcLdsFixed % 16 == 0 && kQcLdsFixed + 4 * kQcMaxBins <= 65536, "the table must fit the dynamic LDS of a plain launch");

struct QcArgs {
    const int64_t *rowptr;     // [n + 1]
    const double *val;         // [rowptr[n]] the stored values, gene by gene
    int64_t n, m;
    int32_t bins;              // values in [1, bins) are decided here
    int64_t *nnz;              // [n]
    double *sum, *ss;          // [n]
    int32_t *mode;             // [n] 0, 1, or 2 = left to the host
    unsigned int *ticket;      // zero as the launch starts
};

// whether a stored value is an integer in [1, bins)
__device__ inline bool qc_counts(double v, int bins) { return v >= 1.0 && v < (double)bins && v == __builtin_floor(v); }

__device__ inline double qc_wave_sum(double v)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ inline int qc_wave_max(int v)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kQcThreads) void k_gene_stats(const QcArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qc_smem[];
    double *s_red1 = reinterpret_cast<double *>(qc_smem);                      // [4] wave partials of the row sum
    double *s_red2 = s_red1 + kQcWaves;                                        // [4] ... of the centred squares
    int *s_first = reinterpret_cast<int *>(qc_smem + 64);                      // [256] a thread's first non-empty count (0: none)
    int *s_last = s_first + kQcThreads;                                        // [256] ... and its last
    int *s_flag = s_last + kQcThreads;                                         // [4] a rise inside a thread's stretch, by wave
    int *s_bad = s_flag + kQcWaves;                                            // [4] a value outside [1, bins) or not an integer
    int *s_vmax = s_bad + kQcWaves;                                            // [4] largest value entered into the table
    unsigned int *s_ticket = reinterpret_cast<unsigned int *>(s_vmax + kQcWaves);
    unsigned int *hist = reinterpret_cast<unsigned int *>(qc_smem + kQcLdsFixed);   // [bins]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double md = (double)A.m;
    const int bins = A.bins;

    for (int b = t; b < bins; b += kQcThreads) hist[b] = 0u;
    for (;;) {
        if (t == 0) *s_ticket = atomicAdd(A.ticket, 1u);
        __syncthreads();
        const int64_t i0 = (int64_t)*s_ticket * kQcTicketRows;
        if (i0 >= A.n) break;                                                  // (block-uniform)
        const int rows = (int)(A.n - i0 < kQcTicketRows ? A.n - i0 : kQcTicketRows);

        // ---- short rows: wave w takes row i0 + w by itself
        if (wave < rows) {
            const int64_t pw = A.rowptr[i0 + wave], lw = A.rowptr[i0 + wave + 1] - pw;
            if (lw <= kQcShortMax) {
                const int len = __builtin_amdgcn_readfirstlane((int)lw);
                const bool live = lane < len;
                double x = 0.0;
                bool ok = true;
                if (live) { x = A.val[pw + lane]; ok = qc_counts(x, bins); }
                const double s = qc_wave_sum(x);
                const double mu = s / md;
                const double dx = x - mu;
                const double d = qc_wave_sum(live ? dx * dx : 0.0);
                const int64_t zeros = A.m - len;
                const double ss = d + (double)zeros * (mu * mu);
                int mode = 2;
                if (__ballot(!ok) == 0) {
                    // the occurrence table of <= 64 values, in the wave: cnt = lanes that hold this lane's value, nxt / ncnt = the
                    // next larger value present and its count, smaller = some lane holds a smaller value
                    const int v = live ? (int)x : 0;
                    int cnt = 0, nxt = 0x7FFFFFFF, ncnt = 0;
                    bool smaller = false;
                    for (int j = 0; j < len; j++) {
                        const int vj = __builtin_amdgcn_readlane(v, j);
                        cnt += vj == v;
                        smaller = smaller || vj < v;
                        if (vj > v) {
                            if (vj < nxt) { nxt = vj; ncnt = 1; }
                            else if (vj == nxt) ncnt++;
                        }
                    }
                    const bool rise = live && ((ncnt > 0 && cnt < ncnt) || (!smaller && zeros > 0 && zeros < (int64_t)cnt));
                    mode = __ballot(rise) != 0 ? 1 : 0;
                }
                if (lane == 0) {
                    const int64_t i = i0 + wave;
                    A.nnz[i] = len; A.sum[i] = s; A.ss[i] = ss; A.mode[i] = mode;
                }
            }
        }

        // ---- long rows: the whole workgroup, one row after the other
#pragma unroll 1
        for (int w = 0; w < rows; w++) {
            const int64_t p0 = A.rowptr[i0 + w], len = A.rowptr[i0 + w + 1] - p0;
            if (len <= kQcShortMax) continue;                                  // (block-uniform)
            const double *xv = A.val + p0;
            // pass 1: the sum, the table, the largest value
            double s = 0.0;
            int vmax = 0;
            bool bad = false;
            int64_t e = t;
            for (; e + 3 * kQcPassEntries < len; e += 4 * kQcPassEntries) {    // (four loads in flight, added in ascending order)
                const double rr[4] = {xv[e], xv[e + kQcPassEntries], xv[e + 2 * kQcPassEntries], xv[e + 3 * kQcPassEntries]};
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const double x = rr[u];
                    if (qc_counts(x, bins)) { const int v = (int)x; atomicAdd(&hist[v], 1u); vmax = v > vmax ? v : vmax; }
                    else bad = true;
                    s += x;
                }
            }
            for (; e < len; e += kQcPassEntries) {
                const double x = xv[e];
                if (qc_counts(x, bins)) { const int v = (int)x; atomicAdd(&hist[v], 1u); vmax = v > vmax ? v : vmax; }
                else bad = true;
                s += x;
            }
            s = qc_wave_sum(s);
            vmax = qc_wave_max(vmax);
            const bool wbad = __ballot(bad) != 0;
            if (lane == 0) { s_red1[wave] = s; s_vmax[wave] = vmax; s_bad[wave] = wbad ? 1 : 0; }
            __syncthreads();
            const double sum = ((s_red1[0] + s_red1[1]) + s_red1[2]) + s_red1[3];
            const double mu = sum / md;
            int top = s_vmax[0];
#pragma unroll
            for (int k = 1; k < kQcWaves; k++) top = s_vmax[k] > top ? s_vmax[k] : top;
            const bool rbad = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) != 0;
            // pass 2: the centred squares (the row comes from the cache this time)
            double d = 0.0;
            e = t;
            for (; e + 3 * kQcPassEntries < len; e += 4 * kQcPassEntries) {
                const double rr[4] = {xv[e], xv[e + kQcPassEntries], xv[e + 2 * kQcPassEntries], xv[e + 3 * kQcPassEntries]};
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const double dx = rr[u] - mu;
                    d += dx * dx;
                }
            }
            for (; e < len; e += kQcPassEntries) {
                const double dx = xv[e] - mu;
                d += dx * dx;
            }
            d = qc_wave_sum(d);
            // this thread's stretch of the table's bins [1, top]: first and last non-empty counts, a rise inside it; cleared as read
            {
                const int per = (top + kQcThreads - 1) / kQcThreads;
                const int b0 = 1 + t * per;
                int b1 = b0 + per;
                if (b1 > top + 1) b1 = top + 1;
                int first = 0, prev = 0;
                bool rise = false;
                for (int b = b0; b < b1; b++) {
                    const int c = (int)hist[b];
                    if (c) {
                        hist[b] = 0u;
                        if (prev) rise = rise || prev < c;
                        else first = c;
                        prev = c;
                    }
                }
                s_first[t] = first;
                s_last[t] = prev;
                const bool wrise = __ballot(rise) != 0;
                if (lane == 0) { s_red2[wave] = d; s_flag[wave] = wrise ? 1 : 0; }
            }
            __syncthreads();
            if (wave == 0) {
                // lane l joins the reports of threads 4 l .. 4 l + 3, then the last non-empty count is carried across the lanes
                int first = 0, prev = 0;
                bool rise = false;
#pragma unroll
                for (int u = 0; u < kQcThreads / 64; u++) {
                    const int f = s_first[lane * (kQcThreads / 64) + u], la = s_last[lane * (kQcThreads / 64) + u];
                    if (f) {
                        if (prev) rise = rise || prev < f;
                        else first = f;
                        prev = la;
                    }
                }
                int incl = prev;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int o = __shfl_up(incl, off);
                    if (lane >= off && incl == 0) incl = o;
                }
                int64_t before = __shfl_up(incl, 1);
                if (lane == 0) before = 0;
                const int64_t zeros = A.m - len;
                if (before == 0) before = zeros;                               // the zeros' level comes first (absent when 0)
                rise = rise || (first && before > 0 && before < (int64_t)first);
                const bool any = __ballot(rise) != 0 || (s_flag[0] | s_flag[1] | s_flag[2] | s_flag[3]) != 0;
                if (lane == 0) {
                    const int64_t i = i0 + w;
                    const double dd = ((s_red2[0] + s_red2[1]) + s_red2[2]) + s_red2[3];
                    A.nnz[i] = len; A.sum[i] = sum; A.ss[i] = dd + (double)zeros * (mu * mu);
                    A.mode[i] = rbad ? 2 : (any ? 1 : 0);
                }
            }
            // (the next row's pass 1 writes s_red1 / s_vmax / s_bad and the table only; wave 0 has read those before the barrier
            // above, and reaches the next row's first barrier after it is done with s_first / s_last / s_red2 / s_flag)
        }
        __syncthreads();                                                       // the ticket word is free for the next fetch
    }
}

}  // namespace vbnmf
