/*
 * vbnmf.h -- C ABI of the MI355X-native VB-NMF update engine (libvbnmf_hip.so).
 *
 * Drop-in boundary for ONE path of ccfindR: the variational-Bayes NMF update step
 *     Rcpp::List vbnmf_update(const Eigen::MatrixXd& X, const Rcpp::List& wh,
 *                             const Rcpp::List& hyper, const Rcpp::NumericVector& fudge)
 * (reference src/vbnmf_update.cpp:16-17), reached from R through
 *     .Call(`_ccfindR_vbnmf_update`, X, wh, hyper, fudge)
 * (reference R/RcppExports.R:4-6, src/RcppExports.cpp:11-22) and called only by
 * vb_iterate (reference R/bayesian.R:339).  INTEGRATION.md shows the Rcpp shim that
 * binds these entry points under the reference's own .Call symbol.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns a vbnmf_status (0 = ok) and
 *     never throws or aborts; vbnmf_last_error() gives the message of the calling
 *     thread's last failure (the shim turns it into Rcpp::stop, as END_RCPP does for
 *     exceptions at src/RcppExports.cpp:21).
 *   - matrices are column-major fp64 exactly as R / Eigen hold them:
 *       lw, ew, dw : n x r        lh, eh, dh : r x m        X : n x m
 *   - dimensions are 64-bit (the reference's `U/=n*m` in int, src/vbnmf_update.cpp:90,
 *     overflows past 2^31-1 elements; here the product is formed in double as the R twin
 *     does, R/bayesian.R:97).
 *   - NaN/Inf are not errors: they propagate into lkh, so the caller's is.na() break
 *     (R/bayesian.R:345) keeps working.
 *   - a HIP device is REQUIRED.  There is no CPU fallback: without a usable gfx950
 *     device every compute entry point fails with VBNMF_ERR_NO_DEVICE.
 *   - one engine = one device = one host thread at a time; distinct engines may be
 *     driven from distinct threads / processes (one process per GPU).
 */
#ifndef VBNMF_H
#define VBNMF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    VBNMF_OK = 0,
    VBNMF_ERR_BAD_ARG = 1,     /* null pointer, non-positive dim, rank out of range, bad index */
    VBNMF_ERR_NO_DEVICE = 2,   /* no HIP device / device is not usable                          */
    VBNMF_ERR_HIP = 3,         /* a HIP runtime call failed (message has the HIP error string)  */
    VBNMF_ERR_OOM = 4,         /* host or device allocation failed                              */
    VBNMF_ERR_STATE = 5        /* call sequence error (e.g. step before set_state)              */
} vbnmf_status;

/* Largest rank an engine takes.  The reference's only bound is rank <= min(n, m) (R/bayesian.R:319-320); here the
 * factor rows live in registers: up to 32 columns per lane, above that two lanes share a task (ranks 33..64, padded
 * to a multiple of 8) and then four (ranks 65..128, padded to a multiple of 16).  The device-resident truncated SVD
 * (vbnmf_engine_svd) holds subspaces of at most VBNMF_MAX_SVD_COLUMNS columns. */
#define VBNMF_MAX_RANK 128
#define VBNMF_MAX_SVD_COLUMNS 64

/* Message of the calling thread's most recent failure ("" if none). Never NULL. */
const char *vbnmf_last_error(void);
/* "major.minor.patch" of this library. */
const char *vbnmf_version(void);
/* Number of visible HIP devices (0 if none / no driver); never fails. */
int32_t vbnmf_device_count(void);

/* ---------------------------------------------------------------------------------
 * Count matrix X.  Host-side canonical copy (compressed sparse columns, zeros dropped)
 * plus the iteration-invariant sum_ij lgamma(X_ij + 1) of src/vbnmf_update.cpp:80-81.
 * Replaces the per-iteration `as.matrix(bundle$mat)` + Rcpp::as<Eigen::MatrixXd> copy
 * (R/bayesian.R:339, src/RcppExports.cpp:15): X is ingested ONCE.
 * --------------------------------------------------------------------------------- */
typedef struct vbnmf_matrix vbnmf_matrix;

/* Dense n x m column-major doubles (what as.matrix() hands the reference). */
int vbnmf_matrix_from_dense(int64_t n, int64_t m, const double *X, vbnmf_matrix **out);
/* dgCMatrix slots (Matrix package; what counts(object) is after read_10x, R/utils.R:34):
 * p = m+1 column pointers, i = 0-based row indices (any order within a column,
 * duplicates are summed), x = values. */
int vbnmf_matrix_from_csc(int64_t n, int64_t m, const int32_t *p, const int32_t *i,
                          const double *x, vbnmf_matrix **out);
/* Compressed sparse rows: p = n+1 row pointers, j = 0-based column indices. */
int vbnmf_matrix_from_csr(int64_t n, int64_t m, const int32_t *p, const int32_t *j,
                          const double *x, vbnmf_matrix **out);
/* Matrix Market file: what read_10x hands the reference through
 * as(Matrix::readMM(count), 'dgCMatrix') (R/utils.R:34; e.g. inst/extdata/matrix.mtx:1-2).
 * Coordinate real / integer / pattern, general / symmetric / skew-symmetric, or the dense
 * array form; 1-based indices; repeated (i, j) are summed; explicit zeros are dropped.
 * Parsed by all host threads straight into compressed columns. */
int vbnmf_matrix_from_mtx(const char *path, vbnmf_matrix **out);
/* The file Matrix::writeMM writes in write_10x (R/utils.R:876): coordinate, general,
 * "integer" when every stored value is one (else "real"), entries by columns. */
int vbnmf_matrix_write_mtx(const vbnmf_matrix *X, const char *path);
/* Read-only view of the canonical compressed columns (m+1 pointers, rows ascending in each
 * column, no zeros); the arrays belong to the handle. */
int vbnmf_matrix_csc(const vbnmf_matrix *X, const int64_t **colptr, const int32_t **row,
                     const double **val);
/* n, m, stored entries, sum lgamma(x+1); any out pointer may be NULL. */
int vbnmf_matrix_info(const vbnmf_matrix *X, int64_t *n, int64_t *m, int64_t *nnz,
                      double *sum_lgamma_x1);
/* The reference's input guards (R/bayesian.R:244-247): counts of all-zero rows / columns. */
int vbnmf_matrix_empty_counts(const vbnmf_matrix *X, int64_t *empty_rows, int64_t *empty_cols);
/* Rank classes for a sweep over several ranks on this matrix (the reference's `for(rank in ranks)`, R/bayesian.R:316,
 * which re-densifies X for every rank and iteration).  The tiled layout depends on the rank only through the LDS row
 * size; with a plan every engine created afterwards takes the geometry of the smallest class at or above its padded
 * rank, so the ranks of the sweep share ONE pair of layouts (max_classes = 1: the class of the largest rank) instead of
 * cutting one per row size.  Results do not depend on the plan beyond the summation order inside a step.
 * count = 0 clears the plan (every rank its own geometry, the default). */
int vbnmf_matrix_plan_ranks(vbnmf_matrix *X, const int32_t *ranks, int32_t count, int32_t max_classes);
/* The same classes without touching a matrix handle: classes[0..*n_classes) = padded ranks, ascending (at most `count`
 * of them).  vb_factorize picks each engine's geometry from this list and hands it to vbnmf_engine_create_geom, so a
 * sweep neither mutates the shared matrix handle nor loses a plan the caller set on it.  vbnmf_padded_rank: the rank as
 * the device pads it (even up to 32, multiples of 8 up to 64, of 16 up to 128); 0 for a rank out of range. */
int vbnmf_plan_classes(const int32_t *ranks, int32_t count, int32_t max_classes, int32_t *classes, int32_t *n_classes);
int32_t vbnmf_padded_rank(int32_t r);
/* Host threads of the library's ingestion and layout cuts (the reference is single-threaded: src/vbnmf_update.cpp has
 * no host parallelism at all).  Default: the cores of the process's affinity mask, at most 32 (VBNMF_HOST_THREADS
 * overrides) -- a cap chosen for ranks that all work at once.  vbnmf_set_host_threads(n) lifts or lowers it for THIS
 * process until called again with 0 and returns the count in force before: the one process of a node that cuts the
 * layouts for its waiting peers (vb_factorize_sharded) takes their cores for the duration of the cut.  Results do not
 * depend on the count (layouts, cell order: fixed chunking; the sums of ingestion are taken once, by the holder of X). */
int32_t vbnmf_host_threads(void);
int32_t vbnmf_set_host_threads(int32_t n);
void vbnmf_matrix_destroy(vbnmf_matrix *X);

/* ---------------------------------------------------------------------------------
 * One ingestion and one pair of tiled layouts per NODE instead of per process.  The reference ships the whole bundle,
 * matrix included, to every MPI slave (R/bayesian.R:252-263); here the processes of a node (one per GPU) share the host's
 * work through memory the caller maps into all of them (e.g. /dev/shm):
 *   builder  : vbnmf_matrix_get_meta -> meta[8]; vbnmf_matrix_export_layout(buf = NULL) cuts (and caches) the layout of one
 *              side and returns the blob size; a second call writes the blob into the shared buffer.
 *   the rest : vbnmf_matrix_shell(meta) -- a handle with X's dimensions and constants but NO entries -- then
 *              vbnmf_matrix_import_layout for each side; engines created on it (whole matrix, that geometry) upload the
 *              imported arrays to their own GPU.  Entry points that need entries (partition engines, _csc, _write_mtx,
 *              _empty_counts, vbnmf_layout_build) answer VBNMF_ERR_STATE on a shell.
 * meta = {n, m, stored entries, all-integer flag, packed-count flag, max value, sum lgamma(x+1), sum(-x log x + x)}.
 * geometry_rank and n_wg must be what the engines will use (vbnmf_engine_create_geom, vbnmf_device_sweep_workgroups).
 * --------------------------------------------------------------------------------- */
int vbnmf_matrix_get_meta(const vbnmf_matrix *X, double *meta);
int vbnmf_matrix_shell(const double *meta, vbnmf_matrix **out);
int vbnmf_matrix_is_shell(const vbnmf_matrix *X);
/* The per-matrix work every whole-matrix layout starts from, ahead of need and safe to call from a second host thread
 * while a layout is being cut: the internal order of the cells and the row-major copy of X (the gene side's input). */
int vbnmf_matrix_prepare(const vbnmf_matrix *X);
/* The same, started on a background host thread the handle owns: returns at once.  Meant for the caller that ingests X
 * for whole-matrix factorisations (vb_factorize, a rank sweep) and has other set-up to do before the first engine. */
int vbnmf_matrix_prepare_async(const vbnmf_matrix *X);
/* Uploads the whole-matrix layout of `side` (geometry_rank, n_wg as for vbnmf_matrix_export_layout; cut now if it is not
 * cached or imported yet) to HIP device `device` ahead of the first engine: engines created afterwards in that geometry
 * on that device share the resident copy (they always do among themselves; this only moves the upload earlier, e.g.
 * beside the wait for the other side's layout). */
int vbnmf_matrix_preload_layout(const vbnmf_matrix *X, int32_t side, int32_t geometry_rank, int32_t n_wg, int32_t device);
int vbnmf_matrix_export_layout(const vbnmf_matrix *X, int32_t side, int32_t geometry_rank, int32_t n_wg,
                               void *buf, int64_t capacity, int64_t *bytes);
int vbnmf_matrix_import_layout(const vbnmf_matrix *X, const void *buf, int64_t bytes);
/* The same without the two copies: ONE copy of a layout's big arrays (the packed entry stream, 200 MB a side at the
 * headline size) per node, in a file on a memory file system that every process maps.
 *   share  : cuts the layout with the entry stream written straight INTO the new file `path` (built as path + ".part" and
 *            renamed when complete: a peer that sees `path` sees all of it); the mapping stays the layout's storage in
 *            this process.  (A layout already cached in ordinary memory is copied into the file instead.)
 *   attach : maps `path` read-only and adopts the entry stream in place; the small index arrays are copied.
 * The file can be unlinked once every process has attached; the memory lives as long as a mapping does. */
int vbnmf_matrix_share_layout(const vbnmf_matrix *X, int32_t side, int32_t geometry_rank, int32_t n_wg, const char *path);
int vbnmf_matrix_attach_layout(const vbnmf_matrix *X, const char *path);
/* Persistent workgroups of the sweep kernels on `device` (one per CU; VBNMF_NWG overrides): the n_wg of the layouts
 * that whole-matrix engines on that device use. */
int vbnmf_device_sweep_workgroups(int32_t device, int32_t *n_wg);
/* First use of `device` by this process ahead of need (HIP context, first allocation, load of the library's code object:
 * ~0.15 s once per process): a process that must wait for something else first spends the wait here. */
int vbnmf_device_warmup(int32_t device);

/* ---------------------------------------------------------------------------------
 * Engine: device-resident state of one factorisation of (a column block of) X at one
 * rank.  Holds what vb_iterate carries between calls, {lw, lh, ew, eh} (R/bayesian.R:
 * 334-339), in HBM, plus X in the tiled device layout.
 * --------------------------------------------------------------------------------- */
typedef struct vbnmf_engine vbnmf_engine;

/* Whole matrix on HIP device `device`, rank 1 <= r <= VBNMF_MAX_RANK. */
int vbnmf_engine_create(const vbnmf_matrix *X, int32_t r, int32_t device, vbnmf_engine **out);
/* Cell-partitioned engine: owns columns [col_begin, col_end) of X; m_global = total
 * number of cells across all partitions (used for the n*m normalisation of lkh).
 * The gene-side state (lw, ew, dw) is replicated in every partition; the caller sums
 * the reduce buffer (below) across partitions between step_local and step_finish. */
int vbnmf_engine_create_part(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end,
                             int64_t m_global, int32_t r, int32_t device, vbnmf_engine **out);
/* The same with the layouts' geometry named per ENGINE: geometry_rank >= r is the rank whose LDS row size the tiled
 * layouts are cut for (the ranks of a sweep, R/bayesian.R:316, share one pair: vbnmf_plan_classes); 0 = the class of the
 * matrix's plan (vbnmf_matrix_plan_ranks), the rank's own geometry without one. */
int vbnmf_engine_create_geom(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, int64_t m_global, int32_t r,
                             int32_t geometry_rank, int32_t device, vbnmf_engine **out);
void vbnmf_engine_destroy(vbnmf_engine *e);

/* n, local m (cells owned), r. */
int vbnmf_engine_dims(const vbnmf_engine *e, int64_t *n, int64_t *m_local, int32_t *r);

/* Load wh$lw (n x r), wh$lh (r x m_local), wh$eh (r x m_local): the three members of
 * `wh` that influence the result (src/vbnmf_update.cpp:22-25; ew is overwritten at :44).
 * Also (re)computes the sufficient statistics of the new state. */
int vbnmf_engine_set_state(vbnmf_engine *e, const double *lw, const double *lh, const double *eh);

/* One vbnmf_update step (src/vbnmf_update.cpp:33-90) on the resident state with
 * hyper = {aw, bw, ah, bh} and fudge.  Outputs:
 *   lkh      wh$lkh, the log evidence per element (:90)
 *   stats[4] mean(log lw), mean(log lh), mean(ew), mean(eh) of the NEW state: the four
 *            reductions hyper_update needs (R/bayesian.R:8-11), so the caller never
 *            downloads the factors between steps.  May be NULL.
 * Synchronous from the caller's view (the lkh read-back is the sync point). */
int vbnmf_engine_step(vbnmf_engine *e, double aw, double bw, double ah, double bh, double fudge,
                      double *lkh, double *stats);

/* Split form of step for cell-partitioned engines.  step_local enqueues the local work
 * and leaves this partition's contribution in the reduce buffer (device memory, `count`
 * doubles); the caller all-reduces (sum) that buffer across partitions on the engine's
 * stream (RCCL), then step_finish produces lkh/stats (identical on every partition).
 * For an unpartitioned engine step == step_local; step_finish with no all-reduce. */
int vbnmf_engine_step_local(vbnmf_engine *e, double aw, double bw, double ah, double bh,
                            double fudge);
int vbnmf_engine_reduce_buffer(vbnmf_engine *e, void **device_ptr, int64_t *count);
int vbnmf_engine_step_finish(vbnmf_engine *e, double *lkh, double *stats);
/* After set_state on a partitioned engine the initial statistics need the same exchange:
 * set_state leaves them in the reduce buffer; all-reduce it, then call this. */
int vbnmf_engine_state_finish(vbnmf_engine *e);

/* The per-rank loop of vb_iterate (R/bayesian.R:336-352) run by the device: up to max_it steps with
 *   - hyper_update (R/bayesian.R:2-53, Niter = 100, Tol = 1e-3) after every step `it` with it > n0 and
 *     it %% dn == 0, `flags` = hyper.update (4 logicals),
 *   - break when lkh is NaN (:345), or when it > 1, it > n0, lkh >= lk0 and |1 - lkh/lk0| < tol (:346-347;
 *     lk0 then keeps the PREVIOUS step's evidence, as the reference leaves it), else lk0 <- lkh (:348).
 * Steps are queued ahead of the device, so no host round trip sits between two steps; kernels queued
 * beyond the break return at once and the state stays exactly as the breaking step left it.
 * hyper[4] = aw, bw, ah, bh (in: initial, out: final).  Outputs (any may be NULL): it = steps done,
 * lk0, lkh of the last step, reason (1 NaN, 2 converged, 3 hyper Newton did not converge -- the
 * reference stops with an error there, :43 -- 4 max_it reached), history[it][9] = lkh, mean log lw,
 * mean log lh, mean ew, mean eh, then aw, bw, ah, bh after that step's update (history_rows >= max_it).
 * A partitioned engine needs an RCCL communicator attached (below); every process then calls this with the
 * same arguments and gets the same results. */
int vbnmf_engine_run(vbnmf_engine *e, double *hyper, double fudge, int32_t max_it, double tol, int32_t n0,
                     int32_t dn, const int32_t *flags, int32_t *it, double *lk0, double *lkh, int32_t *reason,
                     double *history, int64_t history_rows);

/* The restarts of one rank, stepped together.  Reference: vb_factorize runs `nrun` independent factorisations of every
 * rank, `lapply(seq_len(nrun), FUN = vb_iterate, bundle)` (R/bayesian.R:260-261; over Rmpi slaves at :262-263), each the loop of
 * R/bayesian.R:337-352 from its own random start.  On the small matrices ccfindR ships (inst/extdata: 1030 x 450) one such
 * loop cannot fill the GPU -- a step is two dependent launches of ~15 us for microseconds of work on a dozen workgroups -- and
 * concurrent streams or processes do not overlap them (profiles/r05_small_concurrent.txt), so the independent loops share
 * their launches instead: `count` engines of ONE rank on ONE matrix handle (same layouts, grids, update table; each engine
 * its own state, set beforehand), every step two launches for the whole batch, every engine following its own control block
 * (hyper-parameters, evidence, stop -- an engine that has stopped idles through the others' remaining steps).  Per engine the
 * results are those of vbnmf_engine_run on it alone, bit for bit.  hyper: [count][4] in / out; it_out, lk0_out, lkh_out,
 * reason_out: [count] (any may be NULL); history (or NULL): [count][history_rows][9], history_rows >= max_it.
 * Engines: unpartitioned, no communicator, padded rank <= 16, count <= 64, of ONE row width (one rank, or several ranks made
 * under vbnmf_set_engine_padding); the launches go on the first engine's stream. */
/* Grids of the engines the CALLING host thread creates from now on (0, 0: back to the defaults, one workgroup / block per
 * CU): engines meant for a batch of B want 256 / B of each -- B engines step in one launch of B x grid workgroups.  The
 * grid is part of the order of the block-wise sums: engines of different grids agree to rounding, not bit for bit.  (No
 * reference counterpart: launch geometry.) */
int vbnmf_set_engine_grid(int32_t n_wg, int32_t update_blocks);
/* Row width of the engines the CALLING host thread creates from now on: `padded_rank` columns (a padded rank >= the engine's
 * own: even up to 32, a multiple of 8 up to 64, of 16 beyond; 0: back to the rank's own), the columns beyond the rank held at
 * zero.  Engines of DIFFERENT ranks made this way share kernels, layouts and update table and may form one batch: the rank
 * loop of vb_iterate (R/bayesian.R:316) as well as the restarts step in one launch on a small matrix.  A padded engine agrees
 * with the unpadded one to rounding (the width fixes the update's thread mapping), not bit for bit. */
int vbnmf_set_engine_padding(int32_t padded_rank);
int vbnmf_batch_run(vbnmf_engine **engines, int32_t count, double *hyper, double fudge, int32_t max_it, double tol,
                    int32_t n0, int32_t dn, const int32_t *flags, int32_t *it_out, double *lk0_out, double *lkh_out,
                    int32_t *reason_out, double *history, int64_t history_rows);

/* ---------------------------------------------------------------------------------
 * Communicators for cell-partitioned runs.  The reference has no counterpart inside
 * an iteration: its only inter-process mechanism is Rmpi::mpi.applyLB over restarts (R/bayesian.R:262-263),
 * and vb_iterate's loop (R/bayesian.R:337-352) runs in one process.  Here one factorisation can span the GPUs
 * of a node, cells partitioned, one process per GPU, and the per-step exchange -- the sum over partitions of
 * [sw (n x r) | rowSums(eh) (r) | 4 scalars] -- is an RCCL all-reduce over xGMI enqueued by the LIBRARY on
 * the engine's streams, so a binding needs no collective of its own:
 *
 *   rank 0:   vbnmf_comm_unique_id(id)           then broadcast `id` (VBNMF_COMM_ID_BYTES) to every process
 *                                                 by whatever the host language has (Rmpi::mpi.bcast, MPI_Bcast,
 *                                                 torch.distributed.broadcast ...)
 *   all:      vbnmf_comm_create(id, ..., nranks, rank, device, &comm)        ncclCommInitRank
 *             vbnmf_engine_create_part(X, cb, ce, m, r, device, &e) ; vbnmf_engine_attach_comm(e, comm)
 *             vbnmf_engine_set_state(e, ...) ; vbnmf_engine_allreduce(e) ; vbnmf_engine_state_finish(e)
 *             vbnmf_engine_run(e, ...)           the whole loop of vb_iterate, device-driven, on every process;
 *                                                 per step the n x r piece of the all-reduce travels beside the
 *                                                 cell-side half of the sweep and a second, small one (the
 *                                                 sweeps' evidence partials, 8 KB) follows that sweep; every
 *                                                 process takes the same (replicated) stop decision and queues
 *                                                 the same collectives.  Every rank must run the same build
 *                                                 with the same VBNMF_NO_CONTROL_FOLD setting (it decides what
 *                                                 the second exchange carries).
 *        or   vbnmf_engine_step_local(e, ...) ; vbnmf_engine_allreduce(e) ; vbnmf_engine_step_finish(e, ...)
 *
 * librccl is opened at run time (dlopen "librccl.so.1"); without it vbnmf_comm_create fails with
 * VBNMF_ERR_NO_DEVICE and everything else keeps working.
 *
 * A LOCAL GROUP is the same protocol for partition engines that share ONE process and ONE device (RCCL
 * refuses two ranks on a device): tests and single-GPU rehearsals of a partitioned run.  The engines are
 * attached in partition order and driven together through vbnmf_group_state_finish / vbnmf_group_run; the
 * all-reduce is a kernel that adds the partitions' buffers in partition order.
 * --------------------------------------------------------------------------------- */
typedef struct vbnmf_comm vbnmf_comm;
#define VBNMF_COMM_ID_BYTES 128
int vbnmf_comm_unique_id(void *id, int64_t bytes);
int vbnmf_comm_create(const void *id, int64_t bytes, int32_t nranks, int32_t rank, int32_t device,
                      vbnmf_comm **out);
int vbnmf_comm_create_local(int32_t nranks, int32_t device, vbnmf_comm **out);
/* nranks, this process's rank (0 for a local group), kind (0 RCCL, 1 local group); any pointer may be NULL. */
int vbnmf_comm_info(const vbnmf_comm *c, int32_t *nranks, int32_t *rank, int32_t *kind);
void vbnmf_comm_destroy(vbnmf_comm *c);
/* The engine must live on the communicator's device.  An RCCL communicator takes one engine; a local group
 * takes its nranks partition engines, in partition order. */
int vbnmf_engine_attach_comm(vbnmf_engine *e, vbnmf_comm *c);
/* In-place all-reduce (sum, fp64) of the engine's reduce buffer on the engine's stream (RCCL communicators). */
int vbnmf_engine_allreduce(vbnmf_engine *e);
/* Local groups: the state exchange after set_state on every member, and the device-driven loop of the whole
 * group (arguments and results as vbnmf_engine_run; history comes from partition 0 -- all are identical). */
int vbnmf_group_state_finish(vbnmf_comm *c);
int vbnmf_group_run(vbnmf_comm *c, double *hyper, double fudge, int32_t max_it, double tol, int32_t n0,
                    int32_t dn, const int32_t *flags, int32_t *it, double *lk0, double *lkh, int32_t *reason,
                    double *history, int64_t history_rows);

/* Download the current wh members (any pointer may be NULL):
 * lw, ew, dw : n x r ; lh, eh, dh : r x m_local.  dw, dh are variances, as the reference
 * returns them (src/vbnmf_update.cpp:46,56); the R driver takes sqrt later (R/bayesian.R:382-383). */
int vbnmf_engine_get_state(vbnmf_engine *e, double *lw, double *lh, double *ew, double *eh,
                           double *dw, double *dh);

/* The HIP stream (hipStream_t) the engine launches on, for callers that order other
 * device work (an RCCL all-reduce) against it; and the option to adopt a caller's stream. */
int vbnmf_engine_get_stream(vbnmf_engine *e, void **stream);
int vbnmf_engine_set_stream(vbnmf_engine *e, void *stream);

/* Profiling aid for bench.py: when enabled, every step brackets the sweep kernel with HIP
 * events on the engine's stream; get returns the accumulated kernel time and launch
 * count since the last reset and resets them. */
int vbnmf_engine_timing_enable(vbnmf_engine *e, int32_t on);
int vbnmf_engine_timing_get(vbnmf_engine *e, double *sweep_ms, int64_t *sweep_launches);

/* Diagnostic (engine created with env VBNMF_DEBUG_TIMES=1): 100 MHz device timestamps of the last
 * sweep, out[side][wg][2 + 2*waves] = {workgroup start, end, then (start, end) per wave}. */
int vbnmf_engine_debug_times(vbnmf_engine *e, unsigned long long *out, int64_t capacity,
                             int32_t *n_wg, int32_t *waves);

/* Layout facts for roofline accounting / tests (any pointer may be NULL):
 * padded entry slots and bytes the two sweeps stream per step, task counts. */
int vbnmf_engine_layout_info(const vbnmf_engine *e, int64_t *nnz, int64_t *slots_gene_side,
                             int64_t *slots_cell_side, int64_t *stream_bytes_per_step,
                             int64_t *tasks_gene_side, int64_t *tasks_cell_side);

/* ---------------------------------------------------------------------------------
 * Stateless form: the reference's call, one X in, one updated `wh` out
 * (src/vbnmf_update.cpp:16-101).  Builds a throw-away engine on device 0 (or the device the environment variable VBNMF_DEVICE names); use the
 * engine API in a loop.  Outputs as the returned list's lw, lh, ew (= w), eh (= h),
 * dw, dh, lkh (:92-100).
 * --------------------------------------------------------------------------------- */
int vbnmf_update_dense(int64_t n, int64_t m, int32_t r, const double *X,
                       const double *lw_in, const double *lh_in, const double *eh_in,
                       double aw, double bw, double ah, double bh, double fudge,
                       double *lw, double *lh, double *ew, double *eh,
                       double *dw, double *dh, double *lkh);
/* The stateless entries (these two and vbnmf_ml_update_*) keep the LAST ingested matrix and its engine alive between
 * calls, keyed by the content of X: the dimensions, TWO independently seeded 64-bit hashes of every byte handed in (the
 * seed starts every chunk digest, so contents colliding under one seed do not under the other: a 128-bit key) and, on a
 * hit, a comparison of the CSC pointer array resp. of a strided sample (<= 4096 values) of the dense X.  The reference's
 * loop passes the same X thousands of times (R/bayesian.R:339), and a repeat then costs the hashes, the state transfer
 * and one step instead of ingestion + layouts + engine.  Results do not depend on it.  VBNMF_STATELESS_CACHE=0 disables it;
 * vbnmf_stateless_cache_clear() releases what is held (device and host memory). */
void vbnmf_stateless_cache_clear(void);
/* Device buffers of destroyed engines are kept in a per-process pool (at most VBNMF_POOL_MB, default 4096) for the next
 * engine: a rank sweep creates and destroys one engine per (run, rank) unit and every hipFree synchronises the device.
 * This returns what the pool holds to the driver. */
void vbnmf_pool_trim(void);
/* Same with X as dgCMatrix slots (no densification on the R side). */
int vbnmf_update_csc(int64_t n, int64_t m, int32_t r, const int32_t *p, const int32_t *i,
                     const double *x,
                     const double *lw_in, const double *lh_in, const double *eh_in,
                     double aw, double bw, double ah, double bh, double fudge,
                     double *lw, double *lh, double *ew, double *eh,
                     double *dw, double *dh, double *lkh);

/* ---------------------------------------------------------------------------------
 * Maximum-likelihood NMF on the same engine: the step of
 * factorize(), reference R/factorize.R:2-27 (nmf_updateR) with its likelihood :40-49
 * (the two are always called together, :195-196).  The factors live on the device
 * between steps; a VB state and an ML state exclude each other (setting one drops the
 * other).  Partitioned engines: see "ML-NMF with the cells partitioned" below.
 *
 *   ml_set_state  w : n x r column-major, h : r x m column-major (init, :30-38)
 *   ml_step       h <- h .* (t(w) %*% (x/(w h))) / colSums(w), clipped at double eps (:8-15);
 *                 then w <- w .* ((x/(w h)) %*% t(h)) / rowSums(h) on the NEW h (:17-24);
 *                 prior != 0 adds the Gamma prior terms (up + gamma_a - 1, down +
 *                 gamma_a/gamma_b, :10-13,19-22; factorize() itself never sets it).
 *                 *lk = likelihood(mat, w, h) of the updated pair (:40-49).
 *   ml_likelihood likelihood(mat, w, h) (:40-49) of the pair the engine holds now (after
 *                 ml_set_state: of the loaded pair; after ml_step: the value ml_step returned).
 *   ml_get_state  the current w, h (either may be NULL).
 * --------------------------------------------------------------------------------- */
int vbnmf_engine_ml_set_state(vbnmf_engine *e, const double *w, const double *h);
int vbnmf_engine_ml_step(vbnmf_engine *e, int32_t prior, double gamma_a, double gamma_b, double *lk);
/* factorize()'s inner loop under criterion = 'likelihood' (R/factorize.R:194-213) run by the device: up to
 * max_it steps, break when abs(lkold - lk) < tol * abs(lkold) (lkold starts at -Inf), steps queued ahead of
 * the GPU.  Outputs (any may be NULL): it = steps done, lk = likelihood of the last step, reason (2 converged,
 * 4 max_it reached), history[it] = the likelihood after every step (history_rows >= max_it). */
int vbnmf_engine_ml_run(vbnmf_engine *e, int32_t prior, double gamma_a, double gamma_b, int32_t max_it,
                        double tol, int32_t *it, double *lk, int32_t *reason, double *history,
                        int64_t history_rows);

/* The `nrun` restarts factorize() makes of every rank (`for(irun in seq_len(nrun))`, R/factorize.R:181; nrun defaults to 20),
 * their device-driven loops (vbnmf_engine_ml_run: R/factorize.R:194-213 under criterion = 'likelihood') stepped together: four
 * launches per step for the whole batch, every engine following its own control block.  Per engine the results are those of
 * vbnmf_engine_ml_run on it alone, bit for bit.  Engines as for vbnmf_batch_run (one rank, one matrix handle, rank <= 16,
 * count <= 64, grids from vbnmf_set_engine_grid), their states set by vbnmf_engine_ml_set_state.  it_out, lk_out, reason_out:
 * [count] (any may be NULL); history (or NULL): [count][history_rows], history_rows >= max_it. */
int vbnmf_batch_ml_run(vbnmf_engine **engines, int32_t count, int32_t prior, double gamma_a, double gamma_b, int32_t max_it,
                       double tol, int32_t *it_out, double *lk_out, int32_t *reason_out, double *history, int64_t history_rows);
/* The same loop under criterion = 'connectivity' (R/factorize.R:198-208), the rule the reference names for cluster
 * stability, run by the device: every step's H update forms the labels which.max(h[, j]) of its new h and their
 * contingency table against the previous step's; the control step counts nchange = sum(cnn != cnn0) from it
 * (it == 1: npair = m (m - 1) / 2, :200), zstep = nchange == 0 ? zstep + 1 : 0 (:206-207), and stops with reason 2 at
 * zstep == ncnn_step (:208), else with reason 4 at max_it.  No launch is added to the step.  The likelihood is computed,
 * reported and written to the history every step; it stops nothing (a NaN likelihood included, as in the reference).
 * changes (or NULL): the nchange of every step run, changes_rows >= max_it; changes[0] = npair.  Afterwards the labels of
 * the last step are the engine's previous labels: vbnmf_engine_cluster_changes right behind the run reports 0.
 * A partitioned engine with an RCCL communicator attached runs the rule for the whole matrix (below: "ML-NMF with the cells
 * partitioned"); changes[0] is then m_global (m_global - 1) / 2.
 * VBNMF_ERR_BAD_ARG: NULL handle, max_it < 1, ncnn_step < 1; VBNMF_ERR_STATE: before ml_set_state, a partitioned engine
 * without an RCCL communicator (a local group's member: vbnmf_group_ml_run_connectivity). */
int vbnmf_engine_ml_run_connectivity(vbnmf_engine *e, int32_t prior, double gamma_a, double gamma_b, int32_t max_it,
                                     int32_t ncnn_step, int32_t *it, double *lk, int32_t *reason, double *history,
                                     int64_t history_rows, int64_t *changes, int64_t changes_rows);
/* ... of the restarts of a rank stepped together (R/factorize.R:181, :198-208): vbnmf_batch_ml_run's engines, admission
 * rules and four launches per step.  Per engine the results are those of vbnmf_engine_ml_run_connectivity on it alone, bit
 * for bit.  it_out, lk_out, reason_out: [count]; history: [count][history_rows]; changes: [count][changes_rows] (or NULL). */
int vbnmf_batch_ml_run_connectivity(vbnmf_engine **engines, int32_t count, int32_t prior, double gamma_a, double gamma_b,
                                    int32_t max_it, int32_t ncnn_step, int32_t *it_out, double *lk_out, int32_t *reason_out,
                                    double *history, int64_t history_rows, int64_t *changes, int64_t changes_rows);
int vbnmf_engine_ml_likelihood(vbnmf_engine *e, double *lk);
int vbnmf_engine_ml_get_state(vbnmf_engine *e, double *w, double *h);

/* ---------------------------------------------------------------------------------
 * ML-NMF with the cells partitioned (engines of vbnmf_engine_create_part; communicators as above).  Partition p holds
 * its own columns of h and a full copy of w.  One step of nmf_updateR (R/factorize.R:2-27) needs TWO exchanges, because
 * the W update (:17-24) reads statistics of all cells on the new h and the likelihood (:40-49) needs the new w:
 *
 *   h_p <- update (:8-15) on the partition's own statistics, colSums(w) replicated
 *   exchange 1 : [ (x / (w h_new)) %*% t(h_new) summed over the partition's cells (n x r, index-major, padded rank)
 *                | rowSums(h_new) (R) | 0 0 ]                     = the reduce buffer's first n*R + R + 2 doubles
 *   w   <- update (:17-24) on the summed statistics: bit-identical on every partition
 *   exchange 2 : [ sum x log(w h) | sum_{x>0}(-x log x + x) ] over the partition's cells   (:44-47)
 *   lk  = ((data - sum_k colSum(w)_k rowSum(h)_k) + const) / n / m_global                  (:48)
 *
 * Host-stepped (vbnmf_engine_reduce_buffer names the buffer, n*R + R + 4 doubles; `sum` is vbnmf_engine_allreduce or the
 * caller's own in-place sum over the partitions):
 *
 *   vbnmf_engine_ml_set_state(e, w, h_p)      leaves [rowSums(h_p) (R) | 0 0 | data term | constant] in the buffer's TAIL,
 *                                             the R + 4 doubles from offset n*R
 *   sum(tail) ; vbnmf_engine_ml_state_finish(e)                     likelihood of the loaded pair
 *   vbnmf_engine_ml_step_local(e, ...)        1st call of a step: H update, gene-side sweep, exchange 1 packed into the buffer
 *   sum(buffer)                               (at least its first n*R + R + 2 doubles)
 *   vbnmf_engine_ml_step_local(e, ...)        2nd call: W update, cell-side sweep, the TAIL as after ml_set_state
 *   sum(tail)                                 (summing the whole buffer again is harmless: only the tail is read)
 *   vbnmf_engine_ml_step_finish(e, &lk)       the likelihood, the same on every partition
 *
 * The protocol is "sum the buffer at every exchange"; only the tail is READ behind the exchanges marked sum(tail), so a caller may
 * send the tail alone there (vbnmf_engine_reduce_tail names it), and vbnmf_engine_allreduce does -- an optimisation that spares a
 * second n*R all-reduce per step, with the same results as summing everything.  An unpartitioned engine accepts the same calls
 * (nothing to sum).  vbnmf_engine_ml_step on a partitioned engine is VBNMF_ERR_STATE, as vbnmf_engine_step is;
 * vbnmf_engine_ml_step_finish without both ml_step_local calls, and ml_state_finish without a pending ml_set_state, too.
 *
 * Device-driven (R/factorize.R:194-213, criterion = 'likelihood'): vbnmf_engine_ml_run on an engine with an RCCL
 * communicator attached, vbnmf_group_ml_run for a local group -- arguments and results as vbnmf_engine_ml_run, history from
 * partition 0.  Both exchanges are queued by the library, out of place, so the steps queued past the stop change nothing;
 * the control step reads only reduced values, so every partition stops at the same step.  vbnmf_group_ml_state_finish is
 * the exchange behind ml_set_state plus ml_state_finish on every member.  Sums run per partition first, then across the
 * partitions in partition order: results agree with the single engine to rounding, not bit for bit.
 * vbnmf_engine_ml_get_state / ml_likelihood answer for the partition (its own columns of h; the global likelihood).
 * criterion = 'connectivity' (:198-208): vbnmf_engine_ml_run_connectivity on an engine with an RCCL communicator attached,
 * vbnmf_group_ml_run_connectivity for a local group.  The rule counts changed PAIRS of cells and a pair may lie in two
 * partitions, so each partition's H update counts its own cells into its own (r+1) x (r+1) table of [previous label][new
 * label], and exchange 2 of the step grows to
 *   exchange 2 : [ sum x log(w h) | sum_{x>0}(-x log x + x) | the table as (r+1)^2 doubles ]
 * -- entries are cell counts <= m_global < 2^53, so the doubles and their sum are exact in any order and every partition forms
 * nchange = pairs(rows) + pairs(cols) - 2 pairs(cells), zstep and the stop from the same integers.  No third exchange; under
 * the likelihood rule both exchanges keep their lengths.  A local group's member called alone is VBNMF_ERR_STATE.
 * Afterwards every partition's previous labels are those of its own cells at the last step (vbnmf_engine_cluster_ids);
 * vbnmf_engine_cluster_changes on a partition still counts the pairs within that partition only.
 * --------------------------------------------------------------------------------- */
/* Where the TAIL of the reduce buffer starts and how many doubles it holds (n*R, R + 4; either pointer may be NULL). */
int vbnmf_engine_reduce_tail(const vbnmf_engine *e, int64_t *offset, int64_t *count);
int vbnmf_engine_ml_state_finish(vbnmf_engine *e);
int vbnmf_engine_ml_step_local(vbnmf_engine *e, int32_t prior, double gamma_a, double gamma_b);
int vbnmf_engine_ml_step_finish(vbnmf_engine *e, double *lk);
int vbnmf_group_ml_state_finish(vbnmf_comm *c);
int vbnmf_group_ml_run(vbnmf_comm *c, int32_t prior, double gamma_a, double gamma_b, int32_t max_it, double tol,
                       int32_t *it, double *lk, int32_t *reason, double *history, int64_t history_rows);
/* vbnmf_engine_ml_run_connectivity (R/factorize.R:198-208) for the partitions of a local group: arguments and results as
 * there, history and changes from partition 0, changes[0] = m_global (m_global - 1) / 2.
 * VBNMF_ERR_BAD_ARG: max_it < 1, ncnn_step < 1, NULL communicator; VBNMF_ERR_STATE: not a local group, members missing. */
int vbnmf_group_ml_run_connectivity(vbnmf_comm *c, int32_t prior, double gamma_a, double gamma_b, int32_t max_it,
                                    int32_t ncnn_step, int32_t *it, double *lk, int32_t *reason, double *history,
                                    int64_t history_rows, int64_t *changes, int64_t changes_rows);
/* Stateless forms of the same step: nmf_updateR(x, w, h, n, m, r, prior, gamma.a, gamma.b)
 * followed by likelihood(x, w, h) (R/factorize.R:2-27, :40-49); throw-away engine on device 0 (VBNMF_DEVICE overrides). */
int vbnmf_ml_update_dense(int64_t n, int64_t m, int32_t r, const double *X,
                          const double *w_in, const double *h_in,
                          int32_t prior, double gamma_a, double gamma_b,
                          double *w, double *h, double *lk);
int vbnmf_ml_update_csc(int64_t n, int64_t m, int32_t r, const int32_t *p, const int32_t *i,
                        const double *x, const double *w_in, const double *h_in,
                        int32_t prior, double gamma_a, double gamma_b,
                        double *w, double *h, double *lk);

/* ---------------------------------------------------------------------------------
 * Projection of new cells onto a fitted basis: the H half of nmf_updateR (R/factorize.R:8-15) iterated with w
 * untouched, every cell (column) on its own, until that cell's likelihood (:40-49, this column, not divided by n m)
 * meets factorize()'s test abs(lkold - lk) < Tol * abs(lkold) (:208; lkold = -Inf before the first step):
 *   h_kj <- max((h_kj * sum_i w_ik x_ij / (w h)_ij [+ gamma_a - 1]) / (colSums(w)_k [+ gamma_a / gamma_b]), DBL_EPSILON)
 * Reads the handle's canonical compressed columns (what vbnmf_matrix_csc exposes) for cells [col_begin, col_end): no layout
 * is cut and no engine is created; the column range, the basis and the start go to HIP device `device` once and ONE launch
 * takes every cell to its stop (csrc/project.h).  w: n x r column-major, non-negative; h: r x (col_end - col_begin)
 * column-major, in: the start, out: the result.  lk_cell, it_cell, reason_cell (each may be NULL), one value per cell: its
 * likelihood, its iteration count and why it stopped -- 1 converged, 3 NaN likelihood, 4 max_it reached.  A cell's result
 * does not depend on the other cells of the call, bit for bit.  An all-zero column is legal here (its h goes to DBL_EPSILON,
 * or to the prior's mode), and so is an all-zero gene row.
 * VBNMF_ERR_BAD_ARG: a shell matrix (it holds no columns), r < 1 or > VBNMF_MAX_RANK, an empty or outside column range,
 * NULL w or h, max_it < 1; VBNMF_ERR_NO_DEVICE: no gfx950 device. */
int vbnmf_matrix_project(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, int32_t r,
                         const double *w, double *h, int32_t prior, double gamma_a, double gamma_b,
                         int32_t max_it, double tol, int32_t device,
                         double *lk_cell, int32_t *it_cell, int32_t *reason_cell);
/* Constants of that kernel at rank r (host only; any out pointer may be NULL): the stored entries of a cell that the
 * workgroup's threads take in one pass (256 up to rank 32, 128 up to 64, 64 above: longer columns go round again), and the
 * kernel time in ms of the calling thread's most recent vbnmf_matrix_project. */
int vbnmf_project_info(int32_t r, int32_t *pass_entries, double *last_kernel_ms);

/* ---------------------------------------------------------------------------------
 * Projection of new cells onto a VB fit's posterior basis: the H half of vbnmf_updateR (R/bayesian.R:71-95) iterated with
 * q(W) -- lw and ew -- untouched, every cell (column) on its own:
 *   lambda_ij = (lw lh)_ij                                                          (:71, stored entries only)
 *   alh_kj = ah + lh_kj * sum_i lw_ik x_ij / lambda_ij                              (:73, :79)
 *   beh_k  = 1 / (ah / bh + colSums(ew)_k)                                          (:80, the given ew: one value per k)
 *   eh_kj  = alh_kj beh_k ;  dh_kj = alh_kj beh_k^2                                 (:81, :103)
 *   lh_kj  = max(exp(digamma(alh_kj)) beh_k, fudge)                                 (:84, :87)
 * until the cell's evidence at the new lh -- its column of U1 (:90-91) plus its column of U3 (:94-95), not divided by n m;
 * U2 belongs to W and is no part of it --
 *   ev_j = - sum_k colSums(ew)_k eh_kj - sum_i lgamma(x_ij + 1)
 *          - sum_i x_ij [ (((lw log lw) lh)_ij + (lw (lh log lh))_ij) / lambda_ij - log lambda_ij ]
 *          + sum_k [ -(ah/bh) eh_kj - lgamma(ah) + ah log(ah/bh) + alh_kj (1 + log beh_k) + lgamma(alh_kj) ]
 * meets vb_iterate's test (:345-347) for that cell: ev NaN (reason 3); after step it > 1, abs(1 - ev / lk0) < tol (reason 1;
 * lk0 = the previous step's ev); max_it reached (reason 4).  The reference's clause `lkh >= lk0` is NOT applied (the
 * evidence is not monotone under this update and the clause would make a cell's stop hang on rounding, DESIGN.md section
 * 5g), nor is the hyper.update.n0 gate (no hyper-parameter is updated here).
 * Reads the handle's canonical compressed columns for cells [col_begin, col_end) as vbnmf_matrix_project does: no layout, no
 * engine, ONE launch (csrc/vbproject.h).  lw, ew: n x r column-major (lw > 0: lw = exp(digamma(alw)) bew of the fit,
 * :83).  lh: r x (col_end - col_begin) column-major, in: the start, out: the result; eh, dh (each may be NULL): E[H] and
 * Var[H] of the same shape.  ev_cell, it_cell, reason_cell (each may be NULL), one value per cell.  A cell's result does
 * not depend on the other cells of the call, bit for bit.  An all-zero column is legal here (alh = ah).
 * VBNMF_ERR_BAD_ARG: a shell matrix, r < 1 or > VBNMF_MAX_RANK, an empty or outside column range, NULL lw, ew or lh,
 * max_it < 1, ah or bh not > 0; VBNMF_ERR_NO_DEVICE: no gfx950 device. */
int vbnmf_matrix_vb_project(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, int32_t r,
                            const double *lw, const double *ew, double ah, double bh, double fudge,
                            double *lh, double *eh, double *dh,
                            int32_t max_it, double tol, int32_t device,
                            double *ev_cell, int32_t *it_cell, int32_t *reason_cell);
/* The same projection with the prior of H re-estimated on the cells of the call and ONE stop for all of them: the H half of
 * vb_iterate (R/bayesian.R:336-352) with q(W) held.  Step it = 1, 2, .. is the step above for every cell under the current
 * (ah, bh); then, over the cells of the call,
 *   E = sum_j ev_j ;  ehm = mean(eh) ;  lhm = mean(log lh)                        (means over the r * cells components)
 *   if it > n0 and it % dn == 0: hyper_update (:2-53) with hyper.update = (F, F, flags[0], flags[1]): Newton on ah if
 *     flags[0] (Niter 100, Tol 1e-3, :343-344), and bh <- ehm if either flag is set (:50-51 assign ehm in both branches)
 *   stop, in this order (:342-348): the hyper-parameter update did not converge or took a non-finite step (reason 5; ah, bh
 *     keep their values); E NaN (reason 3); it > 1, it > n0 and abs(1 - E / lk0) < tol (reason 1; lk0 = the previous E);
 *     otherwise lk0 <- E, and max_it reached is reason 4.  `lkh >= lk0` is NOT applied, as above.
 * The evidence of a step is taken under the (ah, bh) the step was made with; the returned pair includes the update of the
 * last step.  With both flags 0 the cells take exactly the steps of vbnmf_matrix_vb_project, bit for bit, and only the stop
 * differs.  The means run over the cells of THIS call: a caller who splits the columns estimates one prior per part.
 * One launch per step plus one for the totals and the control step (csrc/vbproject.h); the host looks at the control block
 * every eight steps.  hyper: in ah, bh to start from, out the final pair.  All cells make the same number of steps:
 * it_cell and reason_cell (each may be NULL) are filled with that one value, also returned in it and reason (each may be
 * NULL); evidence (may be NULL): the E of the last step.  history (may be NULL): history_rows x 5 row-major, row it - 1 =
 * [E, lhm, ehm, ah, bh after the update]; rows past history_rows are not written.  Everything else as above.
 * VBNMF_ERR_BAD_ARG: as above, NULL hyper or flags, dn < 1, n0 < 0. */
int vbnmf_matrix_vb_project_coupled(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, int32_t r,
                                    const double *lw, const double *ew, double *hyper, const int32_t *flags,
                                    int32_t n0, int32_t dn, double fudge,
                                    double *lh, double *eh, double *dh,
                                    int32_t max_it, double tol, int32_t device,
                                    double *ev_cell, int32_t *it_cell, int32_t *reason_cell,
                                    int32_t *it, int32_t *reason, double *evidence,
                                    double *history, int64_t history_rows);
/* Constants of that kernel at rank r (host only; any out pointer may be NULL): the stored entries of a cell that the
 * workgroup's threads take in one pass (those of vbnmf_project_info), and the kernel time in ms of the calling thread's
 * most recent vbnmf_matrix_vb_project or vbnmf_matrix_vb_project_coupled. */
int vbnmf_vb_project_info(int32_t r, int32_t *pass_entries, double *last_kernel_ms);

/* ---------------------------------------------------------------------------------
 * Quality control between the file and the fit: what filter_cells / filter_genes (R/utils.R:78-95, :134-194) compute
 * from the counts.  The gene side -- the reference's slow part: calc_vmr densifies (x - means)^2 or loops over the genes
 * (:208-214, :341-344), the gene rescue calls has_mode row by row (:166-171) -- is one launch over the genes' rows on HIP
 * device `device` (csrc/qc.h); the cell totals are a host pass.
 * --------------------------------------------------------------------------------- */
/* Per gene i of the whole matrix, from the stored values of its row (grouped by gene on the library's host threads, then
 * uploaded: as 2- or 4-byte integers where every stored value is an integer that fits, else as doubles):
 *   nnz[i]  = stored entries: ncexpr of R/utils.R:139
 *   sum[i]  = sum_j x_ij; the mean of :199 is sum / m
 *   ss[i]   = sum_j (x_ij - mu_i)^2 over all m cells, mu_i = sum[i] / m formed on the device, in the centred form of
 *             :211-212 and :343: the stored entries' (x - mu)^2 plus (m - nnz) mu^2.  The caller divides by m (:212) or m - 1 (:343).
 *   mode[i] = has_mode(row i) of :329-339 as its code runs: 1 iff, among the distinct values PRESENT in the row (zeros included,
 *             m - nnz of them; ascending), some value has fewer occurrences than the next present one.  Distinct doubles are
 *             distinct values (R's table() merges doubles that agree to 15 significant digits).
 * The kernel decides rows whose values are all integers in [1, hist_bins) with an occurrence table in LDS; the other rows are
 * finished on the host by an exact sort-and-count, host_finished (may be NULL) = their number.  mode holds 0 or 1 on return.
 * hist_bins = 0: the default (vbnmf_qc_info); outside [2, 15360] (the table and the kernel's other 2176 bytes fit the 64 KB of
 * LDS a launch may take): VBNMF_ERR_BAD_ARG.  A shell matrix: VBNMF_ERR_STATE.  No usable device: VBNMF_ERR_NO_DEVICE (checked
 * after the arguments).  Sums are formed in a fixed order (csrc/qc.h) without floating-point atomics: the same matrix gives the
 * same bits on every call. */
int vbnmf_matrix_gene_stats(const vbnmf_matrix *X, int32_t device, int32_t hist_bins, int64_t *nnz, double *sum, double *ss,
                            int32_t *mode, int64_t *host_finished);
/* Matrix::colSums of columns [col_begin, col_end) (R/utils.R:81 filter_cells, :321 normalize_count): each stored column added
 * sequentially, rows ascending -- bit-equal to that sum, on the library's host threads.  Host only: a column's total is one
 * pass over entries the host already holds, cheaper than any upload.  A shell matrix: VBNMF_ERR_STATE. */
int vbnmf_matrix_col_sums(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, double *sums);
/* Constants of k_gene_stats and the calling thread's last vbnmf_matrix_gene_stats (any out pointer may be NULL):
 * short_row_max = the longest row one wave takes alone (R/utils.R:139's ncexpr decides the class); pass_entries = entries of a
 * longer row the workgroup takes per pass -- a ticket of the persistent grid is pass_entries / 64 consecutive rows, one per
 * wave; default_hist_bins; grid_workgroups = the persistent grid's size on device 0 (0 without a device); times_ms[4] = grouping
 * by gene, upload, kernel (device events), host finish (:166-171's rows the kernel left), in ms. */
int vbnmf_qc_info(int32_t *short_row_max, int32_t *pass_entries, int32_t *default_hist_bins, int32_t *grid_workgroups, double *times_ms);
/* Test hook (host only): the host finisher on one row -- has_mode (R/utils.R:329-339) of `len` stored non-zero values among m
 * cells, by sort-and-count.  len outside [0, m]: VBNMF_ERR_BAD_ARG. */
int vbnmf_test_gene_mode_host(int64_t m, int64_t len, const double *values, int32_t *out);

/* ---------------------------------------------------------------------------------
 * Cluster annotation: the enrichment scores of assignCelltype() (R/gsea.R:41-77) -- gsea() (:79-115) once on the meta
 * table as it stands (:57) and once per permutation of its rows (:65-72) -- on HIP device `device` (csrc/gsea.h).
 * The reference walks every cluster x every set x all N rows nperm + 1 times in R; here a (permutation, cluster) is one
 * work item of one launch per chunk of permutations, and a set costs a sort and a walk of its hits alone.
 * --------------------------------------------------------------------------------- */
/* The meta table has N rows and r clusters (columns of glist / gwgt, :54-55).  Per cluster k (arrays [r x N], k major):
 *   valid[k*N + i] = !is.na(gwgt[i, k]) (:92), 0 or 1;   wp[k*N + i] = gwgt[i, k]^p (:100), formed by the caller (any value
 *   on NA rows: it is not read).
 * Per (k, s), s one of nS gene sets: the rows i with overlap() TRUE (:95, :117-128), ascending, in CSR form --
 *   hit_row[hit_ptr[k*nS + s] .. hit_ptr[k*nS + s + 1]), and hit_is_miss = 1 where the row is also a miss of :104 (matched
 *   only through a group prefix, not literally in the set).  Hits stand on valid rows only (:93 drops NA rows first).
 * The library derives M[k, s] = valid rows - hits that are no misses (pm[length(pm)] of :106).
 * perms: nperm x N, row b = sample(N) - 1 of :66: the meta-table row that stands at each position; all clusters share it
 *   (glist[perm,], gwgt[perm,], :67).  nperm = 0: the observed scores only (perms may be NULL).
 * Results:
 *   es[s*r + k]      = ES[s, k] of :108 on the table as it stands; NaN where (k, s) has no hit (NA of :96-99), where M = 0
 *                      (:106 divides by it) or where the hits' weights sum to 0 (:102).
 *   exceed[s*r + k]  = number of permutations b with es < ES_b, strict (:69), formed in integer arithmetic; -1 where es is NaN.
 *                      pvalue of :74 = exceed / nperm.
 *   null_es[(b*nS + s)*r + k] = ES_b[s, k]; may be NULL.
 * The scores are those of the reference's dense cumsum BIT FOR BIT: the hits' weights are added in table order by one thread,
 * the rows between them add exact zeros, and the maximum is attained at a hit or at the last row (csrc/gsea.h).  No
 * floating-point atomics: the same inputs give the same bits on every call.
 * Limits: any N < 2^31 - 64, 1 <= r <= VBNMF_MAX_RANK, any nS.  A set with more than max_set_hits (vbnmf_gsea_info: 4096) hits in
 * a cluster is VBNMF_ERR_BAD_ARG -- the sort lives in LDS -- unless its M is 0 (a set holding every gene: NaN whatever its
 * size).  The permutations are uploaded in chunks of chunk_perms (vbnmf_gsea_info).
 * Everything is checked on the host before a device is looked for, and the device sees no unchecked index:
 * VBNMF_ERR_BAD_ARG for a NULL argument, N, r, nS, nperm out of range, hit_ptr not ascending from 0, hit rows not strictly
 * ascending in [0, N) or on an NA row, a weight wp of a valid row that is not finite (0 * Inf of :101 would be NaN on a row
 * the hits' walk never sees), a row of perms that is no permutation of 0 .. N-1; then VBNMF_ERR_NO_DEVICE. */
int vbnmf_gsea_perm(int32_t device, int64_t N, int32_t r, int32_t nS, const uint8_t *valid, const double *wp, const int64_t *hit_ptr,
                    const int32_t *hit_row, const uint8_t *hit_is_miss, int64_t nperm, const int32_t *perms, double *es,
                    int64_t *exceed, double *null_es);
/* Constants of k_gsea_perm and the calling thread's last vbnmf_gsea_perm (any out pointer may be NULL): wave_width (64);
 * workgroup_size (256: one workgroup per (permutation, cluster) of :65 x :88); max_set_hits = the hits of one (cluster, set)
 * the workgroup sorts in LDS (a cap, not a pass size: vbnmf_gsea_perm refuses more); chunk_perms = permutations of one upload
 * for a table of N rows (64 MB of inverse and permutation rows; the environment variable VBNMF_GSEA_CHUNK_PERMS >= 1 makes it
 * smaller); times_ms[4] = upload, kernels (device events), read-back, host checks with the permutations' inversion, in ms. */
int vbnmf_gsea_info(int64_t N, int32_t *wave_width, int32_t *workgroup_size, int32_t *max_set_hits, int64_t *chunk_perms, double *times_ms);

/* ---------------------------------------------------------------------------------
 * The map of the cells: visualize_clusters() (R/utils.R:692-712) runs Rtsne on t(h) (:700).  Here: the t-SNE authors'
 * exact algorithm (no Barnes-Hut tree, Rtsne's theta = 0) on HIP device `device`, in fp64 with fixed summation trees
 * (csrc/tsne.h, DESIGN.md 5k states every formula).  Rtsne is a CPU package this project cannot run: the algorithm below
 * is pinned by the project's own tests, not by Rtsne's output.  No n x n array exists: the force kernel recomputes
 * P_ij = (exp(-beta_i D_ij) / S_i + exp(-beta_j D_ij) / S_j) / (2n) for every pair of every iteration.
 * --------------------------------------------------------------------------------- */
typedef struct vbnmf_tsne vbnmf_tsne;

/* x: n points x d doubles, row-major (t(h) of :700: a cell's coefficients are contiguous); 1 <= d <= VBNMF_MAX_RANK, n <= 2^31 - 2048.
 * normalize != 0: the column means are subtracted and everything is divided by the largest absolute value (not when that is 0),
 * on the host, sequentially.  No PCA.  Then, on the device, per point i the bisection on beta_i (start 1, at most 200 trips,
 * |H_i - ln perplexity| < 1e-5; S_i = sum_{j != i} exp(-beta_i D_ij) + DBL_MIN, D_ij = sum_k (x_ik - x_jk)^2).
 * A row that uses up its 200 trips keeps the beta of its last update, and S_i is evaluated once more at that beta.
 * The handle keeps x, beta and 1/S on the device; the state (Y, uY, gains) starts unset.
 * All arguments are checked before a device is looked for -- VBNMF_ERR_BAD_ARG for a NULL x or handle, n or d out of range,
 * perplexity not finite, < 1 or not 3 perplexity < n - 1 (Rtsne's rule), a non-finite x -- then VBNMF_ERR_NO_DEVICE.  No CPU
 * fallback. */
int vbnmf_tsne_create(int32_t device, int64_t n, int32_t d, const double *x, double perplexity, int32_t normalize, vbnmf_tsne **handle);
void vbnmf_tsne_destroy(vbnmf_tsne *t);
/* beta[n], sum_p[n] = S_i, trips[n] = evaluations of H_i the bisection made (1 .. 200); any may be NULL. */
int vbnmf_tsne_affinity(vbnmf_tsne *t, double *beta, double *sum_p, int32_t *trips);
/* Y, uY, gains: n x 2 row-major each.  set: Y is required (finite); uY NULL = 0, gains NULL = 1 (the start state of the
 * descent).  get: any may be NULL; VBNMF_ERR_STATE before the first set. */
int vbnmf_tsne_set_state(vbnmf_tsne *t, const double *Y, const double *uY, const double *gains);
int vbnmf_tsne_get_state(vbnmf_tsne *t, double *Y, double *uY, double *gains);
/* One evaluation on the current Y; changes nothing.  A[n x 2] = exaggeration * sum_j P_ij w_ij (y_i - y_j) (the product is
 * the one the update forms first), R[n x 2] = sum_j w_ij^2 (y_i - y_j), z[n] = sum_j w_ij, w_ij = 1 / (1 + |y_i - y_j|^2),
 * cost_i[n] = sum_j P_ij ln(P_ij Z / w_ij) with Z = sum_i z_i (terms with P_ij = 0 count 0; always at exaggeration 1).
 * Any out pointer may be NULL.  exaggeration must be finite.  VBNMF_ERR_STATE before the first set_state. */
int vbnmf_tsne_forces(vbnmf_tsne *t, double exaggeration, double *A, double *R, double *z, double *cost_i);
/* Iterations first_iter .. first_iter + n_iter - 1 (numbered from 1) of the descent, queued on one stream with no
 * synchronisation or read-back between them.  Iteration it: e = exaggeration while it <= stop_lying_iter, else 1;
 * m = momentum while it <= mom_switch_iter, else final_momentum;
 *   dY = e A - R / Z (no factor 4: eta = 200 is tuned to that);  gains = sign(dY) != sign(uY) ? gains + 0.2 : 0.8 gains,
 *   floored at min_gain (sign is -1, 0, +1);  uY = m uY - eta gains dY;  Y += uY;  the column means of Y are subtracted.
 * The cost C = sum_{i != j} P_ij ln(P_ij Z / w_ij) of the Y an iteration leaves is recorded after every iteration `it` with
 * it % cost_every == 0 (cost_every <= 0: never) and after the call's last one: itercosts[k], cost_iters[k] = it, *n_costs
 * their number; the caller provides n_iter / cost_every + 1 entries (n_iter entries at the most).  The device array of the
 * costs is read once, after the last iteration.  n_iter = 0: nothing runs, *n_costs = 0.
 * VBNMF_ERR_BAD_ARG: first_iter < 1, n_iter < 0, a schedule value that is not finite, NULL itercosts, cost_iters or n_costs;
 * VBNMF_ERR_STATE before the first set_state. */
int vbnmf_tsne_run(vbnmf_tsne *t, int32_t first_iter, int32_t n_iter, double exaggeration, int32_t stop_lying_iter,
                   int32_t mom_switch_iter, double momentum, double final_momentum, double eta, double min_gain, int32_t cost_every,
                   double *itercosts, int32_t *cost_iters, int32_t *n_costs);
/* Constants of the kernels and the handle's launches (t may be NULL: the grids are then 0 and the times are those of the
 * calling thread's last vbnmf_tsne_create).  ints[8]: wave width (64), workgroup size of the affinity and force kernels (256),
 * the force kernel's i-block (64 points a workgroup) and j-tile (32 points a pass through LDS), the affinity kernel's LDS row
 * capacity (2048 distances; a longer row lives in the workgroup's row of a global scratch buffer), the affinity grid, the
 * force grid, the update kernel's workgroup size (1024, one workgroup).  times_ms[7]: normalise, upload, affinities (device
 * events) of the create; of the handle's last run the loop (device events over its iterations, without the closing cost
 * evaluation), the read-back, and the last iteration's force and update launch each by itself (device events). */
int vbnmf_tsne_info(vbnmf_tsne *t, int32_t *ints, double *times_ms);

/* The neighbour-limited map (csrc/tsne_knn.h): P supported on the k-nearest-neighbour graph of the points and
 * stored sparse, the attraction a sum over the stored rows, the repulsion still exact over all pairs of Y (no tree, no
 * threshold: the map stays bit-reproducible).  The handle is the one above: vbnmf_tsne_affinity, _set_state, _get_state,
 * _forces, _run, _info and _destroy work on it with their signatures; for it vbnmf_tsne_info's last force time is the force
 * stage as a whole (two launches).
 * neighbors = K, or 0 for floor(3 perplexity).  x, n, d, perplexity, normalize as for vbnmf_tsne_create, whose checks hold,
 * and 1 <= K <= n - 1, perplexity < K (K outcomes cannot carry an entropy of ln perplexity otherwise), K <= the kernel's limit
 * (1024, vbnmf_tsne_knn_info): VBNMF_ERR_BAD_ARG, before a device is looked for.
 * N_i = the K indices j != i with the smallest (D_ij, j) in lexicographic order, kept in that order (ties in distance go to
 * the lower index); the bisection of vbnmf_tsne_create runs over N_i only (S_i = sum_{j in N_i} exp(-beta_i D_ij) + DBL_MIN);
 * p_{j|i} = exp(-beta_i D_ij) * (1 / S_i) for j in N_i and 0 otherwise; P_ij = (p_{j|i} + p_{i|j}) * 1/(2n) on the pattern
 * {(i, j): j in N_i or i in N_j}, stored by rows with ascending j (bit for bit symmetric).  The pattern is built on the host
 * from the device's lists and exponentials. */
int vbnmf_tsne_create_knn(int32_t device, int64_t n, int32_t d, const double *x, double perplexity, int32_t normalize, int32_t neighbors,
                          vbnmf_tsne **handle);
/* idx[n x K], dist[n x K] row-major: N_i and the squared distances D_ij, in the list's order; either may be NULL.
 * VBNMF_ERR_STATE on a dense handle. */
int vbnmf_tsne_neighbors(vbnmf_tsne *t, int32_t *idx, double *dist);
/* The stored P in CSR: *nnz, indptr[n + 1], indices[nnz] (ascending in a row), values[nnz]; any may be NULL, and with
 * indices == NULL only nnz and indptr are given (to size the second call).  VBNMF_ERR_STATE on a dense handle. */
int vbnmf_tsne_sparse_p(vbnmf_tsne *t, int64_t *nnz, int64_t *indptr, int32_t *indices, double *values);
/* The search by itself on the points as given (no normalisation, no perplexity): idx[n x k], dist[n x k] as above.
 * n >= 2, 1 <= d <= VBNMF_MAX_RANK, 1 <= k <= n - 1, k <= the limit, x finite: VBNMF_ERR_BAD_ARG before a device is looked for. */
int vbnmf_knn(int32_t device, int64_t n, int32_t d, const double *x, int32_t k, int32_t *idx, double *dist);
/* ints[10]: the neighbour limit (1024: the K survivors of a row are sorted in LDS, over the next power of two), the search
 * kernel's workgroup size (256), its LDS row capacity (2048 distances), the repulsion kernel's j-tile (1024 points a pass
 * through LDS, 256 a wave) and i-block (64 points a workgroup), the rows of P of one attraction workgroup (4: a wave each);
 * of the handle (0 for NULL) K, nnz, the longest row of P, the attraction grid.
 * times_ms[5]: the search with the bisection (device events; t NULL: the calling thread's last vbnmf_knn or create), the
 * pattern (host clock: read-back, build, upload), and of the last iteration of the last run the attraction, the repulsion
 * and the update launch, each by itself (device events). */
int vbnmf_tsne_knn_info(vbnmf_tsne *t, int64_t *ints, double *times_ms);

/* Cluster of every cell from the coefficients the engine holds:
 * ids[j] = which.max(h[, j])[1], 1-based, first maximum on ties (R/factorize.R:55-56 inside
 * connectivity(), R/utils.R:906 cluster_id); h = the ML coefficient matrix, or E[H] of a VB
 * state.  ids: m_local int32.  Saves the r x m download when only the labels are needed
 * (the connectivity stopping criterion of factorize(), R/factorize.R:198-208). */
int vbnmf_engine_cluster_ids(vbnmf_engine *e, int32_t *ids);

/* The same labels compared with those of the PREVIOUS call: changed = sum(cnn != cnn0) over all pairs of cells, the
 * stopping count of factorize() under criterion = 'connectivity' (R/factorize.R:198-208; cnn = connectivity(h),
 * :51-60), formed on the device from the contingency table of the two labelings -- never from the O(m^2) pair
 * vectors.  changed = -1 on the first call after a state was loaded (the reference starts from npair, :200).
 * ids may be NULL. */
int vbnmf_engine_cluster_changes(vbnmf_engine *e, int64_t *changed, int32_t *ids);

/* ---------------------------------------------------------------------------------
 * Consensus measures of factorize() (R/factorize.R:62-78, :218-230) from the label vectors of the runs, never from
 * the O(m^2) pair vector.  With C_ij = the share of the R runs added so far in which cells i and j carry the same
 * label, over pairs i < j:
 *   sum C_ij = S1 / R,      S1 = sum_a sum_k pairs(n_k(a))
 *   sum C_ij^2 = S2 / R^2,  S2 = sum_{a,b} sum_{k,l} pairs(n_kl(a, b))      (n_kl: contingency table of runs a, b)
 *   dispersion = 1/m + 8 con / m^2,  con = sum (C_ij - 1/2)^2 = S2/R^2 - S1/R + npair/4
 * The accumulator keeps the labels of every run on the device ([max_runs][m] uint8: 1..rank, 0 = no label) and the
 * integer sums S1, S2; every add forms the tables of the new run against all stored runs on the device
 * (csrc/consensus.h).  One handle serves one thread at a time.
 * --------------------------------------------------------------------------------- */
typedef struct vbnmf_consensus vbnmf_consensus;

/* m >= 1 cells, 1 <= rank <= VBNMF_MAX_RANK, max_runs >= 1, on HIP device `device`. */
int vbnmf_consensus_create(int64_t m, int32_t rank, int32_t max_runs, int32_t device, vbnmf_consensus **c);
void vbnmf_consensus_destroy(vbnmf_consensus *c);
/* Forget every run (the next nsmpl sample, the next rank). */
int vbnmf_consensus_reset(vbnmf_consensus *c);
/* Adds the arg-max labels of the engine's current coefficients (vbnmf_engine_cluster_ids' rule: ML h or E[H] of a VB
 * state, first maximum, all-NaN column -> 0) as the next run, device to device on the engine's stream; the engine's own
 * label state (vbnmf_engine_cluster_changes) is left alone.  VBNMF_ERR_STATE: partitioned engine, or no state loaded;
 * VBNMF_ERR_BAD_ARG: m, rank or device differ from the handle's, or max_runs runs are held already. */
int vbnmf_consensus_add_engine(vbnmf_consensus *c, vbnmf_engine *e);
/* The same from m host labels (1-based, 0 = no label; anything outside 0..rank is VBNMF_ERR_BAD_ARG). */
int vbnmf_consensus_add_labels(vbnmf_consensus *c, const int32_t *ids);
/* Runs added, the integer sums, and whether any label so far was 0.  Any output may be NULL. */
int vbnmf_consensus_sums(vbnmf_consensus *c, int32_t *runs, uint64_t *s1, uint64_t *s2, int32_t *unlabelled);
/* dispersion(conav / runs, m) (R/factorize.R:62-67) from the integers, evaluated in double; NaN if any label was 0 (the
 * reference's NA propagates through sum); 1/m for m = 1.  VBNMF_ERR_STATE before the first add. */
int vbnmf_consensus_dispersion(vbnmf_consensus *c, double *disp);
/* The labels of run `run` (0-based), m int32. */
int vbnmf_consensus_labels(vbnmf_consensus *c, int32_t run, int32_t *ids);

/* cophenet(conav / R, m, method) (R/factorize.R:69-78) in grouped form, host only (no GPU needed).  Cells with the same
 * label in every run are at distance 0 from each other and at equal distance from everything else, so any linkage joins
 * them first, at height 0; above that level the dendrogram is that of the G distinct label tuples ("groups") with the
 * group sizes as weights and distance = Hamming distance of the tuples / R.  tuples: [G][R] labels, sizes: [G] cells per
 * group (>= 1).  method: "average", "single" or "complete".  coph = Pearson correlation of distance and cophenetic
 * distance over all m (m - 1) / 2 pairs of cells (within a group both are 0); NaN when either has no variance.
 * Nearest-neighbour chain on a G x G matrix: O(G^2) work and memory.  Ties: among equal nearest neighbours of a group the
 * chain takes the one it came from, else the lowest group number; a merged cluster keeps the lower number of its two parts.
 * The sums over the pairs are long double; above 4096 groups (G^2 / 2 terms) they are compensated sums. */
int vbnmf_cophenetic_grouped(int64_t G, int32_t R, const uint8_t *tuples, const int64_t *sizes, const char *method, double *coph);
/* The same for the runs an accumulator holds: downloads the label matrix, numbers the distinct tuples by their first
 * cell, and calls the function above.  groups = G; if G > max_groups (<= 0: 4096, a 128 MB matrix) or a label was 0,
 * coph = NaN. */
int vbnmf_consensus_cophenetic(vbnmf_consensus *c, const char *method, int64_t max_groups, double *coph, int64_t *groups);
/* Test hook: the grouped coefficient from real-valued group distances dist[G][G] (symmetric, zero diagonal) instead of
 * label tuples, so the agglomeration can be checked on tie-free input. */
int vbnmf_test_cophenetic_dist(int64_t G, const double *dist, const int64_t *sizes, const char *method, double *coph);

/* cophenet(conav / R, m, method) (R/factorize.R:69-78) in grouped form with the agglomeration on HIP device `device`
 * (csrc/cophenet.h), for more groups than the host form is meant for.  Arguments and result as
 * vbnmf_cophenetic_grouped; the dendrogram is the host's, merge for merge (the same rule on the same bits, ties
 * included); the coefficient differs from the host's by the rounding of its sums only (per-merge terms in compensated
 * double there, a long double walk over member pairs here).  Limits, each a status checked before anything is launched:
 *   G >= 1 (G = 1: NaN), 1 <= R <= 65535, every size >= 1                                   VBNMF_ERR_BAD_ARG
 *   G <= 32768: the kernel keeps its activity flags in LDS                                  VBNMF_ERR_BAD_ARG
 *   cells^2 * R / 2 < 2^53, cells = sum of the sizes: the weighted distance sums stay exact VBNMF_ERR_BAD_ARG
 *   no usable device                                                                        VBNMF_ERR_NO_DEVICE
 *   device memory: 16 G^2 bytes (two G x G matrices of doubles: 17 GB at G = 32768); a failed allocation is
 *   VBNMF_ERR_OOM with the byte count in the message.  Everything allocated is freed on every return path. */
int vbnmf_cophenetic_grouped_device(int32_t device, int64_t G, int32_t R, const uint8_t *tuples, const int64_t *sizes, const char *method, double *coph);
/* vbnmf_consensus_cophenetic (R/factorize.R:69-78) with the place of the agglomeration chosen: where = 0 host, 1 the
 * accumulator's device, -1 by size (up to 4096 groups on the host, bit for bit as vbnmf_consensus_cophenetic; above, on
 * the device).  The label tuples are grouped on the host either way.  coph = NaN if a label was 0, if G > max_groups
 * (<= 0: 4096 for where = 0, else 32768), or if the device would have to serve more than 32768 groups. */
int vbnmf_consensus_cophenetic_on(vbnmf_consensus *c, const char *method, int64_t max_groups, int32_t where, double *coph, int64_t *groups);
/* Test hook (R/factorize.R:69-78): vbnmf_test_cophenetic_dist with the dendrogram as a further output, from the host
 * core (where = 0) or the device path (where = 1; -1: by size, as above; `device` is ignored on the host).  merges:
 * [G-1][2], per merge the number of the cluster kept (the lower) and of the cluster dropped; heights: [G-1]; either may
 * be NULL.  On the device a non-finite distance is VBNMF_ERR_BAD_ARG, found before the launch; the limits of
 * vbnmf_cophenetic_grouped_device hold with R = 1. */
int vbnmf_test_cophenetic_trace(int32_t where, int32_t device, int64_t G, const double *dist, const int64_t *sizes, const char *method, double *coph,
                                int64_t *merges, double *heights);

/* vb_init(initializer = 'random') on the device (R/bayesian.R:111-115, 162-170): lw = ew ~ Gamma(shape aw, scale
 * bw/aw), lh = eh ~ Gamma(shape ah, scale bh/ah), dw = dh = 0, followed by what set_state does (a partitioned engine
 * needs the state exchange + state_finish).  Philox4x32-10 counters keyed by `seed`, Marsaglia-Tsang rejection; a
 * draw depends on (seed, factor, global element index) only, so partitions of one matrix draw pieces of the same H.
 * R's own RNG stream cannot be reproduced outside R: "identical seeds" means identical arrays, not R's numbers. */
int vbnmf_engine_random_state(vbnmf_engine *e, double aw, double bw, double ah, double bh, uint64_t seed);

/* Truncated SVD of the resident X, entirely on the device: what irlba::irlba(mat, rank) computes for the svd2
 * initialiser (R/bayesian.R:150-159).  Block subspace iteration on k = the engine's rank columns (create the engine
 * with rank = rank_out + oversampling): sparse products on the tiled layout, CholeskyQR2 orthonormalisation and a
 * k x k Jacobi eigen-solve per iteration; stops when the leading rank_out singular values move by <= tol * s[0], or
 * after maxit iterations.  u: n x rank_out, d: rank_out, vt: rank_out x m (column-major).  Drops any VB / ML state.
 * Fails with VBNMF_ERR_STATE if X has fewer than k independent directions.  Unpartitioned engines only. */
int vbnmf_engine_svd(vbnmf_engine *e, int32_t rank_out, double tol, int32_t maxit, uint64_t seed,
                     double *u, double *d, double *vt, int32_t *iterations);

/* ---------------------------------------------------------------------------------
 * Sparse products with the resident X, the two matrix-vector
 * blocks of a truncated SVD -- what irlba::irlba(mat, rank) computes for the svd2
 * initialiser (R/bayesian.R:150-159) -- on the same tiled layout as the update sweeps:
 *   transpose == 0 :  C (n x r) = X %*% t(B),   B : r x m  (column-major, like h)
 *   transpose != 0 :  C (r x m) = t(B) %*% X,   B : n x r  (column-major, like w)
 * r is the engine's rank.  Uses the factor arrays as operand storage: any VB / ML state
 * the engine held is dropped.  Unpartitioned engines only.
 * --------------------------------------------------------------------------------- */
int vbnmf_engine_spmm(vbnmf_engine *e, int32_t transpose, const double *B, double *C);

/* ---------------------------------------------------------------------------------
 * Host-only inspection of the tiled device layout (no GPU needed): builds the layout
 * for one side at padded rank r and hands out its arrays so tests can check, bit for
 * bit, that the slices hold exactly X.  side 0 = gene side (lanes own genes, minor =
 * cells), 1 = cell side.  The returned pointers belong to the layout object.
 * --------------------------------------------------------------------------------- */
typedef struct vbnmf_layout vbnmf_layout;
typedef struct {
    int32_t side, wide;            /* wide: 0 = 4-byte entries (integer counts; one above 16383 takes several slots of the
                                      same minor), 1 = u32 index + f64 value (non-integer X) */
    int64_t n_major, n_minor;      /* lanes own majors; minors are gathered from LDS */
    int32_t block_width;           /* minors in the widest LDS block (blocks differ: see block_start) */
    int32_t n_blocks;              /* ceil(n_minor / block_width) */
    int32_t max_len;               /* longest task (entries per lane) */
    int32_t n_wg;                  /* persistent workgroups the work list is cut for */
    int32_t row_slots;             /* 16-byte LDS slots per staged factor row at this rank */
    int64_t n_tasks, n_slices;     /* task = run of one major's entries in one block; slice = 64 tasks */
    int64_t n_slots;               /* padded entry slots (all slices) */
    int64_t n_segs;                /* segment = the slices of one block in one workgroup's share */
    const uint32_t *task_major;    /* [n_slices*64] major of task slice*64+lane, 0xFFFFFFFF = idle lane */
    const int32_t *slice_width;    /* [n_slices] entries per lane (multiple of 4) */
    const int64_t *slice_off;      /* [n_slices] first slot of the slice; slot(t, lane) =
                                      off + (t/4)*256 + lane*4 + t%4 */
    const int32_t *slice_block;    /* [n_slices] minor block */
    const int32_t *slice_fast;     /* [n_slices] low 16 bits: leading entries per lane that are stored ones (value exactly 1) in
                                      EVERY lane of the slice (multiple of 8; 0 for wide layouts): the sweep runs them through
                                      a shorter loop; high 16 bits: leading entries that are ones or twos in every lane (>= the
                                      low half; the gene side defers their logarithm).  A task's ones come first, then its twos,
                                      then its other entries. */
    const int64_t *block_start;    /* [n_blocks+1] first minor of each block: boundaries sit where the cumulative entry
                                      count reaches a whole number of workgroup quotas */
    const int32_t *seg_block;      /* [n_segs] */
    const int32_t *wg_seg0;        /* [n_wg+1] segments of each workgroup */
    const int32_t *seg_ptr;        /* [n_segs+1] first slice of each segment; slices are numbered in processing order */
    const int32_t *inv_ptr;        /* [n_major+1] tasks of each major ... */
    const uint32_t *inv_task;      /* [n_tasks]   ... in the order their partials are summed */
    const uint32_t *packed;        /* [n_slots] (count << 18) | (local minor * row_slots << 4)   (wide == 0) */
    const uint32_t *wide_idx;      /* [n_slots] local minor                    (wide == 1) */
    const double *wide_val;        /* [n_slots]                                (wide == 1) */
    const int32_t *cell_perm;      /* [cells of the column range] or NULL: the layout's internal renumbering of the cells
                                      (minors on side 0, majors on side 1): position -> column relative to col_begin.
                                      NULL = as stored.  Cells with alike gene support are stored next to each other, so
                                      a gene's entries fall into fewer cell blocks (csrc/order.cpp; VBNMF_CELL_ORDER=0/1). */
    /* The row index: the partial rows the sweep stores and the updates sum.  A run is a maximal stretch of consecutive live
       lanes of one slice with the same major; with merge == 1 the sweep adds a run's statistics inside the wave and stores
       one row, at the run's first lane (ranks <= 32; VBNMF_MERGE_PIECES=0/1).  merge == 0: row_* equals inv_*. */
    int64_t n_rows;
    const int32_t *row_ptr;        /* [n_major + 1] */
    const uint32_t *row_task;      /* [n_rows] first lanes of the runs of each major, as slice*64+lane ids, in inv_task's order */
    int32_t merge;
} vbnmf_layout_view;

int vbnmf_layout_build(const vbnmf_matrix *X, int64_t col_begin, int64_t col_end, int32_t side,
                       int32_t r, vbnmf_layout **out, vbnmf_layout_view *view);
void vbnmf_layout_destroy(vbnmf_layout *L);

/* ---------------------------------------------------------------------------------
 * Test hooks: the library's own fp64 ln / digamma / lnGamma (which stand in for libm's log
 * and GSL's gsl_sf_psi / gsl_sf_lngamma, reference src/vbnmf_update.cpp:59,63,73,81-89),
 * evaluated on the host build and on the device, so tests can check them against mpmath.
 * kind: 0 = ln(x), 1 = psi(x), 2 = lnGamma(x), 3 = 1/x, 4/5 = raw hardware reciprocal seeds
 * (device only), 6 = the sweep's table-driven ln(x), 7 = psi'(x) of the hyper-parameter Newton update (NaN unless x is
 * a positive finite number).
 * --------------------------------------------------------------------------------- */
int vbnmf_test_special_host(int32_t kind, int64_t n, const double *x, double *y);
int vbnmf_test_special_device(int32_t kind, int64_t n, const double *x, double *y);
/* Test hooks into hyper_update (reference R/bayesian.R:2-53) as the device-driven loops end each step with it: `count`
 * independent cases, case c with flags[4c..] (hyper.update), stats[4c..] = (mean log lw, mean log lh, mean ew, mean eh) and
 * hyper_in[4c..] = (aw, bw, ah, bh).  Out: hyper_out[4c..] (the input, bit for bit, when the update failed or no flag is
 * set), failed[c], iters[c] = Newton iterations run, and trace[200c + 100s + k] = side s's shape (0: aw, 1: ah) after
 * iteration k, NaN where nothing was stored.  _device: one launch on device 0, one wave per case, lanes 0 and 1 in the
 * loops' own two-lane routine; a hyper-parameter that is not finite and > 0 is VBNMF_ERR_BAD_ARG before the launch.
 * _host: the same per-side arithmetic, the two sides in sequence, on the CPU; takes any double. */
int vbnmf_test_hyper_update_host(int64_t count, const int32_t *flags, const double *stats, const double *hyper_in,
                                 double *hyper_out, int32_t *failed, int32_t *iters, double *trace);
int vbnmf_test_hyper_update_device(int64_t count, const int32_t *flags, const double *stats, const double *hyper_in,
                                   double *hyper_out, int32_t *failed, int32_t *iters, double *trace);
/* Test hooks into the dense kernels of the device-resident truncated SVD (csrc/init.h: k_gram, k_small, k_apply,
 * k_normal_init), one launch each with the geometry vbnmf_engine_svd uses, on device 0: host arrays are uploaded, the
 * product's own kernel runs, the results are downloaded (tests/test_gpu_svd_dense.py).  R is the padded width of the
 * blocks, one of the widths the kernels are compiled for (2..32 by 2, 40..64 by 8); anything else, a NULL array or a
 * count outside its range is VBNMF_ERR_BAD_ARG, found before a device is looked for.  Everything allocated is freed on
 * every return path.
 *   gram:   A[N][R] in, the raw block partials gp[256][R*R] of t(A) A out (the caller adds them); all R columns count.
 *   small:  gp[nb][R*R] in (nb = 1: an exact G), k columns in use (1 <= k <= R), mode 0 = Cholesky / 1 = Jacobi.  Out:
 *           S[R*R], S2[R*R] (mode 1; may be NULL), vals[R], status (1 = not positive definite, mode 0), and, if not
 *           NULL, vals_host[R+1]: what the kernel wrote through a pinned device-visible block -- the values and, in
 *           slot R, the sequence number `seq` (mode 1).
 *   apply:  B[N][R] = A[N][R] S[R*R]; in_place != 0 runs the kernel with B = A on the device.
 *   normal: the standard normal block g[nmaj][R] of the range finder, columns r..R-1 zero, keyed by `seed`. */
int vbnmf_test_svd_gram(int32_t R, int64_t N, const double *A, double *gp);
int vbnmf_test_svd_small(int32_t R, int32_t k, int32_t mode, int32_t nb, const double *gp, double seq, double *S, double *S2,
                         double *vals, double *vals_host, int32_t *status);
int vbnmf_test_svd_apply(int32_t R, int64_t N, const double *A, const double *S, int32_t in_place, double *B);
int vbnmf_test_svd_normal(int64_t nmaj, int32_t r, int32_t R, uint64_t seed, double *g);
/* Test hook for the bounded waits: enqueues a host function that sleeps `seconds` (<= 60) on the engine's stream, so
 * the steps queued behind it are late without the GPU being busy.  The waits of vbnmf_engine_step / _run / _ml_run are
 * bounded by VBNMF_WAIT_TIMEOUT_S (seconds of wall clock, default 300): past it the call returns VBNMF_ERR_HIP with a
 * message naming the last completed step, and the engine is left untouched (its destroy neither waits nor frees while
 * work is still queued).  The reference has no analogue: its call is synchronous CPU code (src/RcppExports.cpp:11-22). */
int vbnmf_test_stream_sleep(vbnmf_engine *e, double seconds);
/* Test hook (host only): the stateless cache's content hash of `bytes` bytes under `seed`. */
uint64_t vbnmf_test_hash_bytes(const void *data, int64_t bytes, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* VBNMF_H */
