// tsne_knn.h -- gfx950 kernels of the neighbour-limited t-SNE map (included once, by tsne.hip, after tsne.h).
//
//   N_i = the K indices j != i with the smallest (D_ij, j), in that order (ties in distance go to the lower index) -> k_tsne_knn
//   tsne.h's bisection (tsne_bisect), but over N_i only; p_{j|i} = exp(-beta_i D_ij) * (1 / S_i)                    -> k_tsne_knn
//   P on the pattern {(i, j): j in N_i or i in N_j}, rows with ascending j, (p_{j|i} + p_{i|j}) * 1/(2n)             -> host, tsne.hip
//   A_i = sum over the stored row of P_ij w_ij (y_i - y_j), and the three cost sums                                   -> k_tsne_attract
//   R_i = sum_{j != i} w_ij^2 (y_i - y_j), z_i = sum_{j != i} w_ij over ALL j, exactly                                 -> k_tsne_repulse
//   Z, dY, gains, uY, Y, the cost: k_tsne_update of tsne.h, untouched (the same sums[8][n])
//
// The rules of tsne.h hold: fp64, wave64, no floating-point atomics, every sum in a fixed tree, every loop bounded by n, d, K,
// a tile or kTsneMaxTrips, every index formed from values the host checked.  What a kernel here does as a kernel of tsne.h does
// is that header's function: tsne_distance_row, tsne_bisect, tsne_pair_w, tsne_lane_point, tsne_merge_waves.  The integer counters in LDS (a histogram, a
// fill count) are added to in any order; nothing that is written out depends on the order in which those additions land.
#pragma once
#include "tsne.h"

namespace vbnmf {

constexpr int kTsneKnnMax = 1024;                    // neighbours of a point: the K survivors are sorted in LDS (12 KB)
constexpr int kTsneRepTile = 1024;                   // points j of one repulsion tile, (y_j0, y_j1) only: 16 KB, 256 per wave
constexpr int kTsneAttRows = kTsneWaves;             // rows of P of one attraction workgroup: a wave each
static_assert(kTsneRepTile % kTsneWaves == 0 && kTsneThreads == 256, "a wave takes a whole share of a tile; a thread is a radix bin");
static_assert((size_t)kTsneWaves * 3 * kTsneWave <= 2 * (size_t)kTsneRepTile, "the waves' partial sums fit the tile");

// ---- neighbours and affinities -------------------------------------------------------------------------------------------
struct TsneKnnArgs {
    int32_t n, d, K;
    int32_t affinity;              // also run the bisection (0: the search by itself, vbnmf_knn)
    const double *xt;              // [d][n]
    double *scratch;               // [grid][n] rows of D for n > kTsneLdsRow; NULL otherwise
    double log_u;
    int32_t *idx;                  // [n][K]
    double *dist;                  // [n][K]
    double *beta, *sum_p, *inv_s;  // [n]; with affinity
    int32_t *trips;                // [n]
    double *pcond;                 // [n][K] p_{j|i} of the K neighbours, in the list's order
};

// One workgroup per point i, in grid strides; the row D_i. by tsne_distance_row (LDS up to kTsneLdsRow distances, else the
// workgroup's row of `scratch`).
// Selection: the K-th smallest of the n - 1 composite keys (bits of D_ij, j) -- the bit pattern of a non-negative double
// orders as the double does, and the keys are distinct -- by a radix select from the top: 8 passes over the bytes of D, then,
// only if the tie at the K-th distance is cut, 4 over the bytes of j.  A pass counts the candidates (the keys that match the
// digits chosen so far) by their next byte into 256 LDS counters, thread b holds bin b, an inclusive scan (wave shuffles, then
// the waves' totals) finds the one bin in which the count crosses what is still to take.  The counts are sums of integers:
// they do not depend on the order of the atomic additions.  Then every key <= the K-th is put into LDS at a slot an atomic
// counter hands out -- exactly K of them, in an order that does depend on timing -- and a bitonic sort by (D, j) puts them
// into the one order they have.  Bisection: tsne_bisect over the sorted list, so thread q adds the terms q, q + 256, .. in
// ascending order: k_tsne_affinity's tree over K terms.
__global__ __launch_bounds__(kTsneThreads) void k_tsne_knn(const TsneKnnArgs A)
{
    __shared__ double s_row[kTsneLdsRow];
    __shared__ unsigned long long s_key[kTsneKnnMax];
    __shared__ int s_idx[kTsneKnnMax];
    __shared__ double s_xi[VBNMF_MAX_RANK];
    __shared__ unsigned int s_hist[kTsneThreads];
    __shared__ unsigned int s_wsum[kTsneWaves];
    __shared__ unsigned int s_sel[3];                                          // the chosen bin, what is left to take inside it, its count
    __shared__ unsigned int s_fill;
    __shared__ double s_red[2 * kTsneWaves];
    __shared__ double s_ctl[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = A.n, K = A.K;
    double *row = n <= kTsneLdsRow ? s_row : A.scratch + (int64_t)blockIdx.x * n;
    int P2 = 1;
    while (P2 < K) P2 <<= 1;                                                   // <= kTsneKnnMax: the host checked K

    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        tsne_distance_row(A.xt, n, A.d, i, s_xi, row);
        // ---- the K-th smallest (D, j)
        unsigned long long pk = 0ull, mk = 0ull;                               // the digits of D chosen so far and their mask
        unsigned int pj = 0u, mj = 0u;                                         // ... of j
        unsigned int left = (unsigned int)K;                                   // still to take among the candidates
        int jmax = 0x7fffffff;
#pragma unroll 1
        for (int pass = 0; pass < 12; pass++) {
            const bool onj = pass >= 8;
            const int shift = onj ? 24 - 8 * (pass - 8) : 56 - 8 * pass;
            s_hist[t] = 0u;
            __syncthreads();
            for (int j = t; j < n; j += kTsneThreads) {
                if (j == i) continue;
                const unsigned long long key = (unsigned long long)__double_as_longlong(row[j]);
                if ((key & mk) != pk) continue;
                if (onj && ((unsigned int)j & mj) != pj) continue;
                const unsigned int bin = onj ? ((unsigned int)j >> shift) & 255u : (unsigned int)(key >> shift) & 255u;
                atomicAdd(&s_hist[bin], 1u);
            }
            __syncthreads();
            const unsigned int c = s_hist[t];
            unsigned int v = c;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned int up = __shfl_up(v, off);
                if (lane >= off) v += up;
            }
            if (lane == 63) s_wsum[wave] = v;
            __syncthreads();
            for (int w = 0; w < wave; w++) v += s_wsum[w];
            if (v - c < left && left <= v) { s_sel[0] = (unsigned int)t; s_sel[1] = left - (v - c); s_sel[2] = c; }   // one thread: n - 1 >= K
            __syncthreads();
            const unsigned int bin = s_sel[0];
            left = s_sel[1];
            if (onj) { pj |= bin << shift; mj |= 255u << shift; }
            else { pk |= (unsigned long long)bin << shift; mk |= 255ull << shift; }
            if (pass == 7 && s_sel[2] == left) break;                          // every point at the K-th distance is taken: j decides nothing
            if (pass == 11) jmax = (int)pj;
        }
        // ---- the K keys <= (pk, jmax), then their order
        if (t == 0) s_fill = 0u;
        for (int q = K + t; q < P2; q += kTsneThreads) { s_key[q] = ~0ull; s_idx[q] = 0x7fffffff; }
        __syncthreads();
        for (int j = t; j < n; j += kTsneThreads) {
            if (j == i) continue;
            const unsigned long long key = (unsigned long long)__double_as_longlong(row[j]);
            if (key < pk || (key == pk && j <= jmax)) {
                const unsigned int pos = atomicAdd(&s_fill, 1u);
                if (pos < (unsigned int)K) { s_key[pos] = key; s_idx[pos] = j; }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 2; k <= P2; k <<= 1) {
#pragma unroll 1
            for (int s = k >> 1; s > 0; s >>= 1) {
                for (int e = t; e < P2; e += kTsneThreads) {
                    const int x = e ^ s;
                    if (x > e) {                                               // the pair (e, x) is thread (e mod 256)'s alone
                        const unsigned long long ke = s_key[e], kx = s_key[x];
                        const int je = s_idx[e], jx = s_idx[x];
                        const bool gt = ke > kx || (ke == kx && je > jx);
                        if (gt == ((e & k) == 0)) { s_key[e] = kx; s_key[x] = ke; s_idx[e] = jx; s_idx[x] = je; }
                    }
                }
                __syncthreads();
            }
        }
        for (int q = t; q < K; q += kTsneThreads) {
            A.idx[(int64_t)i * K + q] = s_idx[q];
            A.dist[(int64_t)i * K + q] = __longlong_as_double((long long)s_key[q]);
        }
        if (!A.affinity) continue;                                             // (uniform)
        // ---- the bisection over the K sorted distances, none left out
        const auto dist = [](int q) { return __longlong_as_double((long long)s_key[q]); };
        const TsneBisection b = tsne_bisect(K, -1, dist, A.log_u, s_red, s_ctl);
        const double inv = 1.0 / b.S;
        for (int q = t; q < K; q += kTsneThreads) A.pcond[(int64_t)i * K + q] = exp(-b.beta * dist(q)) * inv;
        if (t == 0) {
            A.beta[i] = b.beta;
            A.sum_p[i] = b.S;
            A.inv_s[i] = inv;
            A.trips[i] = b.trips;
        }
    }
}

// ---- attraction ------------------------------------------------------------------------------------------------------------
struct TsneAttArgs {
    int32_t n;
    int32_t cost;                  // also form the three cost sums
    const int64_t *indptr;         // [n + 1]
    const int32_t *indices;        // [nnz] ascending in a row
    const double *values;          // [nnz] P_ij
    const double *y0, *y1;
    double *sums;                  // rows 0 1 (A) and 5 6 7 (the cost sums) of k_tsne_update's [kTsneForceSums][n]
};

// One WAVE per row of P, in grid strides: lane l adds the row's entries l, l + 64, .. in ascending order, the 64 lanes are
// added in the xor butterfly, lane 0 writes.  A row of any length (K .. n - 1) is spread over the wave; nothing is buffered.
__global__ __launch_bounds__(kTsneThreads) void k_tsne_attract(const TsneAttArgs A)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = A.n;
    for (int64_t i = (int64_t)blockIdx.x * kTsneAttRows + wave; i < n; i += (int64_t)gridDim.x * kTsneAttRows) {
        const int64_t b = A.indptr[i], e = A.indptr[i + 1];
        const double yi0 = A.y0[i], yi1 = A.y1[i];
        double a0 = 0.0, a1 = 0.0, c1 = 0.0, c2 = 0.0, cp = 0.0;
        for (int64_t q = b + lane; q < e; q += kTsneWave) {
            const int j = A.indices[q];
            const double P = A.values[q];
            const double d0 = yi0 - A.y0[j], d1 = yi1 - A.y1[j];
            const double w = tsne_pair_w(d0, d1);
            const double pw = P * w;
            a0 += pw * d0;
            a1 += pw * d1;
            if (A.cost && P > 0.0) {
                c1 += P * log(P);
                c2 += P * log(w);
                cp += P;
            }
        }
        a0 = tsne_wave_sum(a0);
        a1 = tsne_wave_sum(a1);
        c1 = tsne_wave_sum(c1);
        c2 = tsne_wave_sum(c2);
        cp = tsne_wave_sum(cp);
        if (lane == 0) {
            A.sums[i] = a0;
            A.sums[n + i] = a1;
            A.sums[5 * n + i] = c1;
            A.sums[6 * n + i] = c2;
            A.sums[7 * n + i] = cp;
        }
    }
}

// ---- repulsion -------------------------------------------------------------------------------------------------------------
struct TsneRepArgs {
    int32_t n;
    const double *y0, *y1;
    double *sums;                  // rows 2 3 (R) and 4 (z) of k_tsne_update's [kTsneForceSums][n]
};

// The R, z half of k_tsne_force: a workgroup owns the kTsneIBlock points i = blockIdx.x * 64 + lane and streams all j through
// LDS in tiles of kTsneRepTile pairs (y_j0, y_j1).  Wave w takes the entries w * 256 .. w * 256 + 255 of every tile, adds its
// terms in ascending j, and tsne_merge_waves joins the four partial sums.
__global__ __launch_bounds__(kTsneThreads) void k_tsne_repulse(const TsneRepArgs A)
{
    __shared__ __attribute__((aligned(16))) double s_y[2 * kTsneRepTile];
    constexpr int kShare = kTsneRepTile / kTsneWaves;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = A.n;
    const TsneLanePoint pt = tsne_lane_point(n, lane);
    const double yi0 = A.y0[pt.ii], yi1 = A.y1[pt.ii];
    double r0 = 0.0, r1 = 0.0, z = 0.0;

    for (int j0 = 0; j0 < n; j0 += kTsneRepTile) {
        __syncthreads();                                                       // the last tile has been read
        for (int q = t; q < kTsneRepTile; q += kTsneThreads) {
            const int j = j0 + q;
            s_y[2 * q] = j < n ? A.y0[j] : 0.0;
            s_y[2 * q + 1] = j < n ? A.y1[j] : 0.0;
        }
        __syncthreads();
        const int jw = j0 + wave * kShare;
        const int cnt = n - jw < kShare ? n - jw : kShare;                      // (wave-uniform; <= 0: nothing of this tile is the wave's)
        const double *T = s_y + 2 * wave * kShare;
#pragma unroll 4
        for (int q = 0; q < cnt; q++) {
            const double d0 = yi0 - T[2 * q], d1 = yi1 - T[2 * q + 1];
            const double w = tsne_pair_w(d0, d1);
            if (pt.valid && jw + q != pt.i) {
                const double ww = w * w;
                r0 += ww * d0;
                r1 += ww * d1;
                z += w;
            }
        }
    }
    const double mine[3] = {r0, r1, z};
    tsne_merge_waves(mine, s_y, A.sums, 2, n, pt, lane, wave);                 // s_part [kTsneWaves][3][64]
}

}  // namespace vbnmf
