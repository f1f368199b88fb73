/* epsilon_hip.h - C ABI of the MI355X-native prox-ADMM solver core for Epsilon.
 *
 * This library replaces the solver side of Epsilon that sits behind the CPython extension
 * `epopt._solve` (reference python/epopt/solvemodule.cc).  The payloads are the ones the
 * unchanged frontend already produces:
 *
 *   problem / f_expr   protobuf wire bytes of `Problem` / `Expression`
 *                      (reference proto/epsilon/expression.proto:205-346)
 *   solver_params      protobuf wire bytes of `SolverParams` (proto/epsilon/solver_params.proto)
 *   data               {location -> raw bytes}: dense = float64 column-major
 *                      (reference python/epopt/constant.py:12-17)
 *   variable values    float64, column-major, m*n per variable (solvemodule.cc:24-56,166-176)
 *   status             protobuf wire bytes of `SolverStatus` (proto/epsilon/solver.proto:4-60)
 *
 * Every function returns 0 on success.  A non-zero return is what the reference reports as
 * `_solve.error("CHECK failed")` (solvemodule.cc:158,185,245-248); the message is available
 * from eps_last_error() (thread-local).  There is no CPU fallback: without a HIP device every
 * compute entry point fails with an error.
 *
 * Not re-entrant per solver handle (the reference is not either: solvemodule.cc:17-22,
 * prox/vector_prox.h:75-76); one process drives one GPU.
 */
#ifndef EPSILON_HIP_H_
#define EPSILON_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One entry of the data map / of a variable-value map.
 * Replaces: PyDict {str: str} walked by WriteConstants / GetVariableVector
 * (reference solvemodule.cc:24-43,58-72). */
enum {
  EPS_BLOB_HOST = 0,       /* ptr -> host bytes, len = byte count (the reference's only form) */
  /* Device blobs are borrowed, not copied, and are read on the library's own non-blocking HIP
   * stream.  The entry point that receives them waits for the device once (hipDeviceSynchronize),
   * so work already enqueued by the caller is complete; they must stay alive and unmodified
   * while a solver handle built from them exists. */
  EPS_BLOB_DEVICE_F32 = 1, /* ptr -> device memory, float,  len = element count (borrowed)   */
  EPS_BLOB_DEVICE_F64 = 2  /* ptr -> device memory, double, len = element count (borrowed)   */
};
typedef struct eps_blob {
  const char* key;  /* NUL-terminated location / variable id */
  const void* ptr;  /* host: read during the call only - the solver-handle entry points copy the
                     * bytes, as the reference copies every blob (solvemodule.cc:58-72), so the
                     * caller may free or overwrite them as soon as the call returns;
                     * device: borrowed while a solver handle built from it exists */
  size_t len;
  int kind;
} eps_blob;

/* A CVXPY Parameter binding: (parameter_id, serialized `Constant`).
 * Replaces: the `parameters` iterable of `_solve.solve` (solvemodule.cc:89-106). */
typedef struct eps_param {
  const char* id;
  const void* constant_proto;
  size_t len;
} eps_param;

typedef struct eps_result eps_result; /* status bytes + {variable_id -> float64 bytes} */
typedef struct eps_solver eps_solver; /* a live solver: operators, factorisation, iterates in HBM */

/* ---- process-level ------------------------------------------------------------------------ */

/* Message of the last failed call on this thread ("" if none). */
const char* eps_last_error(void);
/* "epsilon_hip <version> gfx950" */
const char* eps_version(void);
/* Options (all optional): "dtype" = "f32" (default) | "f64"  compute type of subsequent solves
 * (env EPSILON_HIP_DTYPE);  "device" = ordinal, before first use (env EPSILON_HIP_DEVICE /
 * LOCAL_RANK).  Rides outside SolverParams because the frontend passes only its own kwargs
 * (reference python/epopt/cvxpy_solver.py:69).
 * "refine" = "auto" (default) | "<steps>"  fp32 mode only: iterative refinement of the block
 * LDL^T solve behind SUM_SQUARE / ZERO / AFFINE.  The elimination inverts its pivot blocks
 * explicitly (reference vector/block_cholesky.cc:119-133, linear/dense_matrix_impl.cc:21-30); in
 * fp64, as the reference runs, that is harmless, in fp32 the forward error is kappa * 6e-8 per
 * solve.  "auto" estimates the condition of every pivot block at Init (kappa_1 from two passes
 * over the block and its inverse; where that exceeds 1e3, kappa_2 from six power iterations on
 * each) and adds 1 / 2 / 3 refinement steps (residual against the blocks as given) above
 * 1e3 / 3e4 / 3e6; below 1e3 - every BASELINE.json lasso - the solve is the reference's
 * sequence of operations unchanged.
 * "0" switches it off (env EPSILON_HIP_REFINE).
 * "batch_wide" = "0" (default) | "1"  eps_solve_batch runs groups of 8 or more f32 instances that
 * share the data matrix on the wide route (two matrix products per sweep on the f32 matrix
 * instruction, up to 64 instances per read of the matrix); such groups match eps_solve to f32
 * rounding, not bit for bit - see eps_solve_batch.  Any other value is an error that names it
 * (env EPSILON_HIP_BATCH_WIDE).
 * "batch_zero_tall" = "0" (default) | "1"  eps_solve_batch runs the instances on the tall ZERO-term
 * route ("fused_zero_tall", "fused_zero_tall_smooth") that share the data matrix as one group: per
 * sweep one pass over the transposed copy for up to KB of them (the logistic loss: two, around one
 * launch over the samples of all), one launch for the x side of all and one inverse apply for all,
 * each instance bit for bit its own eps_solve.  "0": each such instance is solved alone.
 * "fused_zero_tall" = "0", "fused_zero" = "0" and "fused" = "0" switch the group off with the route.
 * Read at every eps_solve_batch.  Any other value is an error that names it
 * (env EPSILON_HIP_BATCH_ZERO_TALL).
 * "fused_matrix" = "auto" (default) | "0" | "pass" | "wide"  least squares on a matrix variable
 * X (n x k, data map I_k (x) A, at least 256 rows; multi-block driver, one GPU) with an l1 or a
 * row-group (multi-task group lasso) penalty: the k columns run as k members of the batched fused
 * pass ("pass": f32 and f64, per column the arithmetic of the fused vector lasso) or of
 * the wide kernels ("wide": f32 only, results to f32 rounding) inside one solve.  A forced route
 * that the problem cannot take and "0" mean the generic operator path; "auto" picks by shape.
 * Read at every Init.  Any other value is an error that names it (env EPSILON_HIP_FUSED_MATRIX).
 * "fused_zero" = "auto" (default) | "0"  problems whose data enters through an equality, compiled
 * as a ZERO term over private copies (basis pursuit; hinge, deadzone or quantile loss of
 * z = C x + d with an l1 penalty): the sweep as one pass over C, one row kernel and the apply of
 * the cached inverse.  Taken for fat C with 256 to 20480 rows (f64: 10240), rows a multiple of
 * 4 (f64: 2), multi-block driver, one GPU, every operand in the compute type; anything else, "0"
 * and "fused" = "0" mean the generic operator path.  Read at every Init.  Any other value is an
 * error that names it (env EPSILON_HIP_FUSED_ZERO).
 * "fused_zero_tall" = "auto" (default) | "0" | "1"  the same problems with tall C (more rows than
 * columns; hinge or deadzone loss with an l1 penalty; the logistic loss: the next option): the sweep as one
 * pass over a transposed copy of C (made once per Init: the matrix's footprint doubles), one
 * kernel on the x side and the apply of the cached n x n inverse.  "1": wherever the route is
 * supported - 256 to 20480 columns (f64: 10240), columns a multiple of 4 (f64: 2), multi-block
 * driver, one GPU, every operand in the compute type; "0": never; "auto": from the measured floor
 * on the number of columns (256, so "auto" is "1" at present).  "fused_zero" = "0" and
 * "fused" = "0" switch it off as well.  Read at every Init.  Any other value is an error that
 * names it (env EPSILON_HIP_FUSED_ZERO_TALL).
 * "fused_zero_tall_smooth" = "auto" (default) | "0" | "1"  l1 logistic regression with tall C on
 * that route: five launches per sweep - the products C x' over the transposed copy, one kernel
 * over the samples with the logistic prox in it (its fp64 Newton once per sample and sweep), the
 * forward product, the x side and the apply of the cached n x n inverse.  "1": wherever the
 * route is supported - the conditions of "fused_zero_tall" with at most 10240 columns (f64:
 * 5120); "0": never; "auto": from the measured floor on the number of columns (512).
 * "fused_zero_tall" = "0", "fused_zero" = "0" and "fused" = "0" switch it off as well.  It touches
 * nothing but tall problems with a smooth term on z.  Read at every Init.  Any other value is an
 * error that names it (env EPSILON_HIP_FUSED_ZERO_TALL_SMOOTH).
 * "fused_zero_ridge" = "auto" (default) | "0" | "1"  the ZERO-term problems of the three options
 * above with a ridge penalty lam ||x||_2^2 on x in the l1 term's place (the standard SVM,
 * eps-insensitive regression, ridge-regularised logistic regression): on the same routes, fat and
 * tall, the ridge prox as the two multiplies of its scalar block solve in the threshold's place.
 * "1": wherever those routes take the shape; "0": never; "auto": from the measured floors, one per
 * route (a route without one stays generic).  "fused_zero" = "0", "fused_zero_tall" =
 * "0", "fused_zero_tall_smooth" = "0" and "fused" = "0" switch it off with their routes.  Single
 * solves on the multi-block driver; in eps_solve_batch such an instance is solved by itself.  It
 * touches nothing but problems with a ridge term on x.  Read at every Init.  Any other value is an
 * error that names it (env EPSILON_HIP_FUSED_ZERO_RIDGE).
 * "fused_zero_xfree" = "0" (default, and what unset means) | "1"  the same graph forms without a
 * penalty on x, so that x is no copy and lives in the ZERO term alone (least absolute deviations,
 * quantile regression) with tall C: on the route of "fused_zero_tall" in three launches per sweep -
 * the pass over the transposed copy of C, one kernel on the x side that sums the pass's partials and
 * keeps x (no state, no term: x has no constraint row), and the apply of the cached n x n inverse
 * (C^T C / e^2)^-1.  "1": wherever that route is supported and C has more rows than columns (with
 * fewer the inverse does not exist: the generic path); "0": never.  A smooth loss with free x, the
 * two-block driver and sharded solves keep the generic path.  "fused_zero_tall" = "0", "fused_zero"
 * = "0" and "fused" = "0" switch it off as well.  In eps_solve_batch under "batch_zero_tall" = "1"
 * such instances that share C (a path over the quantile) run as one group, each bit for bit its own
 * eps_solve; without it each is solved by itself on the route.  It touches nothing but these
 * problems.  Read at every Init.  Any other value is an error that names it (env
 * EPSILON_HIP_FUSED_ZERO_XFREE).
 * "fused_zero_lp" = "0" (default, and what unset means) | "1"  the same graph forms with a linear
 * term c^T x on x (AFFINE with one dense 1 x n argument map) or the non-negative cone on z
 * (NON_NEGATIVE, its offset with it) in a threshold's place: linear programs min c^T x s.t. A x <= b,
 * and every mix of the two with the l1, ridge, zone and logistic terms of the options above (the
 * sparsest or least-norm point of a polyhedron; a linear cost with a hinge loss).  On the same
 * routes, fat and tall, with the same launches: the linear term is the two steps of its scalar block
 * solve, x = Dinv (-L v + g) with g = -alpha c, the cone max(., 0).  "1": wherever those routes take
 * the shape in their 256-thread forms; "0": never.  Free x with the cone, the two-block driver and
 * sharded solves keep the generic path; the options of the routes switch it off with them (a ridge
 * term beside the cone needs "fused_zero_ridge").  Single solves on the multi-block driver; in
 * eps_solve_batch such an instance is solved by itself.  It touches nothing but problems with one of
 * the two terms.  Read at every Init.  Any other value is an error that names it (env
 * EPSILON_HIP_FUSED_ZERO_LP).
 * "fused_zero_check" = "0" (default, and what unset means) | "1"  the residual check of the fused
 * ZERO-term routes above (fat and tall; zone, logistic and ridge terms; free x).  "0": the driver's
 * generic check on views of the route's state - some thirty small vector launches and a fetch the
 * host waits for before it enqueues the next sweep.  "1": one launch that sums the five squares of
 * either constraint side in double, in a summation order fixed by the two lengths; the host finishes
 * the closed form, the next epoch's sweeps are enqueued behind the check (EPSILON_HIP_PIPELINE_CHECKS=0:
 * not), and if the check says OPTIMAL they are discarded and a snapshot of the iterate is restored.
 * In eps_solve_batch a group's check is then one launch per active member and one fetch.  The
 * iterates do not depend on it, bit for bit; r_norm, s_norm and the two tolerances agree with the
 * generic check's to rounding.  It touches nothing but solves on those routes.  Read at every Init.
 * Any other value is an error that names it (env EPSILON_HIP_FUSED_ZERO_CHECK).
 * "fused_tall" = "auto" (default) | "0" | "1"  least squares with a separable scaled-zone penalty
 * (lasso; deadzone or quantile penalty) whose data matrix has more rows than columns: the prox of
 * the least-squares term is then the cached n x n inverse applied to the iterate minus a constant,
 * and the sweep never reads the matrix - from 1024 columns two launches (the tiles of the packed
 * inverse; their sum with the element-wise chain), below that the dense apply and the chain.
 * "1": wherever the route is supported - vector variable, at least 256 columns, any number of rows
 * above that, multi-block driver, one GPU, f32 and f64; "0": never; "auto": from the measured floor
 * on the number of columns (256, so "auto" is "1" at present).  "fused" = "0" switches
 * it off as well.  In eps_solve_batch the instances on the route that share the inverse (one data
 * matrix, from 1024 columns) run as one group, each bit for bit its own eps_solve.  Read at every
 * Init.  Any other value is an error that names it (env EPSILON_HIP_FUSED_TALL).
 * "fused_resident" = "auto" (default) | "<KiB>"  bytes of the data matrix that the fused pass
 * (single and batched; one GPU) loads with the default cache policy, so that they stay in the
 * 256 MiB Infinity Cache from sweep to sweep, while the rest is streamed with non-temporal loads.
 * "0" streams everything.  "auto": on the single pass of the multi-block driver, what the cache
 * holds beside the sweep's own vectors (and beside the cached inverse where the sweep applies
 * one); on the batched pass, the ZERO-term route and the two-block driver, which have not been
 * timed with a resident share, nothing - a number of KiB applies there too.  The iterates do not
 * depend on it, bit for bit.  Read at every Init.  Any other value is an error that names it
 * (env EPSILON_HIP_FUSED_RESIDENT_KB). */
int eps_set_option(const char* key, const char* value);
/* Number of visible HIP devices (0 if none); never fails. */
int eps_device_count(void);

/* ---- the two entry points of `epopt._solve` ----------------------------------------------- */

/* Replaces `_solve.solve(problem, parameters, solver_params, data)` (solvemodule.cc:110-187).
 * On success *out holds the SolverStatus bytes and one float64 column-major vector per
 * variable reachable from the problem, in lexicographic id order (solvemodule.cc:166). */
int eps_solve(const void* problem, size_t problem_len, const void* solver_params,
              size_t solver_params_len, const eps_blob* data, size_t ndata,
              const eps_param* params, size_t nparams, eps_result** out);

/* K solves that share one data map and one SolverParams, each with its own problem bytes and
 * its own parameter bindings: a regularisation path (lambda lives in the problem bytes), several
 * right-hand sides b (a parameter or another constant blob), cross-validation folds.
 * Contract: out[k] is exactly what eps_solve(problems[k], ..., params[k], nparams[k]) returns -
 * the same SolverStatus (state, num_iterations, residuals; the timing fields are this call's)
 * and the same variable values, bit for bit.  No reference counterpart.
 *   problems[k], problem_lens[k]   serialized `Problem` of instance k (k < count)
 *   params[k], nparams[k]          instance k's bindings; nparams == NULL: none for any instance,
 *                                  params[k] may be NULL where nparams[k] == 0
 *   data, solver_params            shared by all instances; host blobs are read during the call
 *   out                            caller's array of `count` pointers; on success out[k] is
 *                                  instance k's result (input order), owned by the caller and
 *                                  freed with eps_result_free
 * Instances of the fused "least squares + separable threshold" form (the compiled lasso with
 * NORM_1 / SUM_DEADZONE / SUM_HINGE / SUM_QUANTILE, multi-block driver, one GPU) that share the
 * data matrix run together: one Gram product and one inverse for all, then sweeps that read the
 * matrix once for up to KB instances, each instance stopped at its own residual
 * check.  The same holds for instances of the fused ZERO-term form (basis
 * pursuit, hinge / deadzone / logistic loss + l1 in graph form, fat data matrix with at least 256
 * rows, option "fused_zero") that share the data matrix - a lambda path, several right-hand sides:
 * one Gram product and one inverse for all, then per sweep one pass over the matrix for up to KB
 * of them, one launch for the row side of all and one inverse apply for all; lambda, the loss's
 * parameters and vectors, the offset and the right-hand side may differ per instance, so hinge and
 * deadzone instances on one matrix run together.  With the option "batch_zero_tall" = "1" so do the
 * instances with tall data on the tall ZERO-term route (hinge and deadzone together, logistic among
 * themselves).  Every other instance - tall data without that option, the two-block
 * driver, shapes above 10240 rows in f32 or 5120 in f64, sharded solves, and a fused one with no
 * partner - is solved alone by eps_solve's code.  Per-iteration log lines (verbose) are not printed for instances solved together.
 * With the option "batch_wide" = "1" the contract above is relaxed for the members of a WIDE
 * group and for them only: a group as formed above, f32, with at least 8 members (DESIGN.md 3.8;
 * measured: 6.8x the instance-sweeps/s of 8 instances on the default route at K = 32 on the
 * 10^4 x 5*10^4 matrix).  For such a member out[k] has the same state as eps_solve's result;
 * num_iterations is equal except where a residual sits within rounding of its threshold at a
 * check (then one check apart); variables and residuals agree with eps_solve's to f32 rounding
 * (another summation order, no less accurate: every product is summed in levels with compensated
 * running sums).  Two properties hold bit for bit: a wide group returns identical bytes from run
 * to run, and an instance's bytes depend neither on which other instances share its group nor on
 * its position among them.  f64 instances, the two-block driver, groups of fewer than 8 and
 * every instance outside a group keep the exact contract with the option on.
 * Errors: count == 0 or a NULL array fails; an instance that fails to parse, to set up or to
 * solve fails the whole call and eps_last_error() names its index.  On any failure every out[k]
 * is NULL and nothing is left allocated. */
int eps_solve_batch(const void* const* problems, const size_t* problem_lens, size_t count,
                    const void* solver_params, size_t solver_params_len, const eps_blob* data,
                    size_t ndata, const eps_param* const* params, const size_t* nparams,
                    eps_result** out);

/* Replaces `_solve.eval_prox(f_expr, lam, data, v)` (solvemodule.cc:189-242):
 * argmin_x lam*f(x) + 1/2||x - v||^2 for one PROX_FUNCTION expression.  `v` holds one
 * float64 host blob per variable id.  The result has an empty status. */
int eps_eval_prox(const void* f_expr, size_t f_expr_len, double lambda, const eps_blob* data,
                  size_t ndata, const eps_blob* v, size_t nv, eps_result** out);

/* Result accessors (pointers stay valid until eps_result_free). */
int eps_result_status(const eps_result* r, const void** bytes, size_t* len);
size_t eps_result_num_vars(const eps_result* r);
int eps_result_var(const eps_result* r, size_t i, const char** id, const double** values,
                   size_t* count);
/* Copies variable i's values (count * 8 bytes) into the caller's buffer with the library's host
 * threads - the binding's replacement for one thread's memcpy of a 0.8 GB iterate into a fresh
 * Python bytes object (solvemodule.cc:166-176 builds each output string the same way, one copy).
 * 1 if i is out of range or `bytes` is not the variable's size. */
int eps_result_copy_var(const eps_result* r, size_t i, void* dst, size_t bytes);
void eps_result_free(eps_result* r);

/* ---- solver handles: warm start, staged runs, timing --------------------------------------- */
/* Replaces the process-global warm-start cache (solvemodule.cc:22,142-156): the caller keeps the
 * handle, so the data matrix, the cached factorisation and x/y/u stay resident in HBM across
 * calls.  Host blobs are copied by create / set_parameter (free them when the call returns); the
 * copy lives until eps_solver_destroy, as the reference's DataMap does for the life of its
 * Solver (solvemodule.cc:58-72) - a re-Init after a parameter change may have to upload it
 * again - so a handle costs host memory equal to its host blobs (1.9 GB for the 60000 x 4000
 * feature matrix of BASELINE.json configs[3]) for as long as it is cached; device blobs are
 * borrowed until destroy.  Re-binding a location that is already bound replaces its contents:
 * the next eps_solver_init rebuilds everything that depended on it. */
int eps_solver_create(const void* problem, size_t problem_len, const void* solver_params,
                      size_t solver_params_len, const eps_blob* data, size_t ndata,
                      eps_solver** out);
/* (Re)bind a CVXPY Parameter value; takes effect at the next eps_solver_init
 * (reference algorithms/solver.cc:109-116). */
int eps_solver_set_parameter(eps_solver* s, const char* id, const void* constant_proto,
                             size_t len, const eps_blob* data, size_t ndata);
/* Build operators / Gram matrix / factorisation (the reference's Solver::Init()).  With
 * warm_start set in the params, x/y/u of a previous run are kept (prox_admm.cc:115-120). */
int eps_solver_init(eps_solver* s);
/* Run ADMM sweeps: until OPTIMAL / max_iterations if max_sweeps < 0, else at most max_sweeps
 * more.  *sweeps_done may be NULL. */
int eps_solver_run(eps_solver* s, int max_sweeps, int* sweeps_done);
/* Snapshot of status + variables (same layout as eps_solve's result). */
int eps_solver_result(eps_solver* s, eps_result** out);
/* Wall-clock seconds spent in init and in the sweep loop (device-synchronised). */
int eps_solver_timing(const eps_solver* s, double* init_seconds, double* loop_seconds);
void eps_solver_destroy(eps_solver* s);

/* ---- sharded solves over the GPUs of one node (one process per GPU) ------------------------- */
/* No reference counterpart: the reference has no distributed mode.  Each rank
 * passes its LOCAL problem: sharded variables / constraint rows hold this rank's slice, a data
 * matrix feeding a replicated row from a sharded variable holds this rank's column slab.
 * Sharded keys are declared once with eps_shard_keys; the solver then all-reduces exactly the
 * contractions over sharded keys (lasso: m floats per sweep + a few doubles per residual
 * check) and returns each rank's slice of the sharded variables. */
#define EPS_UNIQUE_ID_BYTES 128
/* rank 0: RCCL unique id to be distributed to the other ranks by the caller. */
int eps_comm_unique_id(void* out128);
/* all ranks: join the RCCL communicator (collective call). */
int eps_comm_init_rccl(int rank, int world, const void* id128);
/* all ranks: host-staged collective through a caller-provided function that sums `count`
 * elements (dtype 0 = float, 1 = double) in place across ranks; used by tests that run the
 * ranks on one GPU or over gloo. */
typedef void (*eps_allreduce_fn)(void* host_buf, size_t count, int dtype, void* ctx);
int eps_comm_init_callback(int rank, int world, eps_allreduce_fn fn, void* ctx);
/* One all-reduce + one all-gather of `count` floats over the communicator, checked (sum of ones
 * == world size): a barrier that also takes RCCL's first-use setup out of a timed Init. */
int eps_comm_warmup(size_t count);
/* COLLECTIVE, optional, after eps_comm_init_*: a one-shot peer-write exchange window over the
 * direct xGMI links (HIP IPC) for the per-sweep messages of a column-sharded solve - m floats
 * each, latency-bound.  With it the sharded fused sweep makes no collective call
 * at all: every rank writes its part straight into every peer's window from inside the sweep's
 * own kernels and sums what it received in rank order (csrc/kernels_peer.hip), and the sweeps
 * between two residual checks are replayed from one hipGraph.  The communicator above stays in
 * charge of the large setup messages and of the residual scalars.  `slot_floats` = largest
 * message in 32-bit words (an fp64 solve needs two per row of the m-vector; 0: 16384); `rehearse_ranks` > 1 (single-rank communicator only) makes this process
 * play ONE rank of that many for timing rehearsals on one GPU (results are not a solve's).
 * *enabled = 1 if every rank has the window and its self test passed, else 0 - then nothing
 * changes (RCCL per sweep) and eps_last_error() says why.  The reference has no counterpart
 * (it has no distributed mode). */
int eps_comm_enable_peer(size_t slot_floats, int rehearse_ranks, int* enabled);
/* Drop the window again (every rank, or none): later solves use the communicator's collectives. */
int eps_comm_disable_peer(void);
int eps_comm_shutdown(void);
/* Replace the set of sharded block keys (variable ids and "constraint:<i>" rows). */
int eps_shard_keys(const char* const* keys, size_t nkeys);
/* Consensus form (call after eps_shard_keys, which resets it): every rank passes
 *   minimise f_g(x_g) + h(z)  subject to  x_g - z = 0
 * with x_g and the constraint row sharded and z replicated.  An objective term over sharded
 * variables only is then this rank's OWN term (its argument rows stay on the rank; nothing of
 * it is all-reduced); the update of z all-reduces the n entries of sum_g (x_g + u_g) - the
 * z-averaging step - and the residual norms / the max over per-term norms are reduced across
 * ranks.  The iterates are those of the single-process solve of the stacked problem
 * (terms f_1..f_G, h; G consensus constraints). */
int eps_shard_consensus_terms(int on);

/* Largest condition estimate of a pivot block and refinement step count of the block
 * factorisations set up since the last reset (fp32 mode; see the "refine" option).  Either
 * pointer may be NULL; reset != 0 clears the record afterwards.  Diagnostics / tests. */
int eps_block_solve_stats(double* max_condition, int* max_refine_steps, int reset);

/* ---- live kernel timing ---------------------------------------------------------------------- */
/* When enabled, every hot kernel launch is bracketed by HIP events on the solver's stream.
 * eps_profile_dump writes one line per tag "tag count total_ms\n" (NUL-terminated, truncated
 * to cap) after synchronising; eps_profile_reset clears the totals. */
int eps_profile_enable(int on);
int eps_profile_reset(void);
int eps_profile_dump(char* buf, size_t cap);

/* ---- per-operator entry points (parity tests pin each kernel through these) ----------------- */

/* y = op(A) x for a serialized `LinearMap` (reference linear/linear_map.cc:83-104 +
 * LinearMapImpl::Apply); `transpose` is a bit set: 1 applies the adjoint, 2 applies the map's
 * Inverse() (reference LinearMapImpl::Inverse, e.g. dense_matrix_impl.cc:21-30).
 * x, y: host float64. */
int eps_linear_map_apply(const void* linear_map, size_t len, const eps_blob* data, size_t ndata,
                         int transpose, const double* x, size_t nx, double* y, size_t ny);
/* C = A op B with op = '+' or '*' through the type-dispatch tables (reference
 * linear/linear_map_add.cc:234-284, linear_map_multiply.cc:249-299).  *result_type receives
 * the ImplType of the result (0 dense, 1 sparse, 2 diagonal, 3 scalar, 4 kronecker);
 * dense (m*n float64, column-major) receives its values; ta / tb transpose the operand first. */
int eps_linear_map_binary(char op, const void* a, size_t a_len, int ta, const void* b,
                          size_t b_len, int tb, const eps_blob* data, size_t ndata,
                          int* result_type, int64_t* m, int64_t* n, double* dense,
                          size_t dense_capacity);
/* Inverse of a serialized map (reference LinearMapImpl::Inverse), dense values out. */
int eps_linear_map_inverse(const void* linear_map, size_t len, const eps_blob* data,
                           size_t ndata, double* dense, size_t dense_capacity);
/* Micro-benchmark of the dense mat-vec kernels on device-resident synthetic data: average
 * milliseconds per launch over `iters` launches (HIP events on the solver stream). */
int eps_bench_gemv(int trans, int64_t rows, int64_t cols, int iters, double* ms_avg);
/* HBM ceiling probe on `bytes` of device memory (device_ptr, 16-byte aligned, or NULL for a
 * synthetic buffer): mode 0 = read-only with non-temporal loads, 1 = read-only, 2 = copy to a
 * scratch buffer (bytes read + bytes written); grid = workgroups of 256 threads (0: 2048).
 * Measurement only: bench.py reports the sweep as
 * a fraction of these beside the 8 TB/s vendor peak. */
int eps_bench_stream(const void* device_ptr, size_t bytes, int mode, int grid, int iters,
                     double* ms_avg);
/* Infinity Cache residency probe: reads `bytes` (device_ptr or NULL as above) as columns of 40000
 * bytes, the first resident_bytes / columns bytes of every column (rounded down to 16) with the
 * default cache policy, the rest with non-temporal loads.  Two untimed launches fill the cache;
 * the average is over the `iters` launches after them.  Measurement only. */
int eps_bench_stream_resident(const void* device_ptr, size_t bytes, size_t resident_bytes, int grid,
                              int iters, double* ms_avg);
/* The fused pass's residency rule for an m x n matrix (f64 != 0: fp64) under a budget in bytes
 * (option "fused_resident"): row chunk q of column j - a chunk is the rows one load instruction
 * of the workgroup covers - is loaded to stay in the Infinity Cache iff q < qfull, or q == qfull
 * and j < jcut.  resident_bytes is the total, the largest of this form within the budget.  A pure
 * host function: no device is needed. */
int eps_fused_residency(int64_t m, int64_t n, int f64, int64_t budget_bytes, int* qfull, int64_t* jcut,
                        int64_t* resident_bytes);
/* Test entry: the (qfull, jcut) that the most recent launch of the fused pass in this process,
 * single or batched, received (0, 0 before any).  No iterate depends on the budget, so this is
 * how a test sees that the option reached the kernel. */
int eps_fused_residency_last(int* qfull, int64_t* jcut);
/* Same for C = op(A) op(B) (M x N x K); lower_only = SYRK-style. */
int eps_bench_gemm(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, int lower_only,
                   int iters, double* ms_avg);
/* SPD inverse of an n x n synthetic matrix. */
int eps_bench_spd_inverse(int64_t n, int iters, double* ms_avg);
int eps_bench_spd_inverse_columns(int64_t n, int64_t cnt, int iters, double* ms_avg);
/* Test entry: the explicit inverse (reference linear/dense_matrix_impl.cc:21-30) of one synthetic
 * n x n positive definite matrix computed twice, with the Cholesky step in form_a and form_b
 * (0 = the fused step of the f32 mode, 1 = separate diagonal / panel launches, -1 = default):
 * ||X_a - X_b||_F and ||X_a||_F.  form_a == form_b checks run-to-run determinism (a data race
 * between the workgroups of a launch shows as a non-zero difference, above all on a busy GPU). */
int eps_test_spd_inverse_repeat(int64_t n, int form_a, int form_b, double* diff_fro, double* norm_fro);

/* Test entry: the block LDL^T behind SUM_SQUARE / ZERO / AFFINE (reference
 * vector/block_cholesky.cc) on a caller-given block matrix, with the "dtype" and "refine" options
 * of a solve.  blocks: one serialized `LinearMap` per (row key, column key) - both triangles of
 * the symmetric matrix, every pair at most once; data: the blobs the maps refer to; rhs: one
 * float64 host blob per key.  `mode` selects what runs; the result holds float64 arrays whose ids
 * are tab-separated fields (a fill bound of "no diagonal block" is -1):
 *   "fill"     ComputeFill of every column key of the matrix as given:  "fill\t<key>" -> [bound]
 *   "factor"   BlockCholesky::Compute and, with a rhs, Solve twice on that factorisation:
 *              "trace\t<step>\t<key>" -> [bound] for every key left at that step,
 *              "pivot\t<step>\t<key>" -> [step],  "order\t<i>\t<key>" -> [i],
 *              "L\t<row>\t<col>" and "D_inv\t<row>\t<col>" -> [ImplType, m, n, ImplType of the two
 *              factors of a Kronecker product (else -1, -1), m*n dense values (column-major)],
 *              "x\t<key>" and "x_again\t<key>" -> solution block,
 *              "condition_estimate" -> [kappa],  "refine_steps" -> [steps]
 *   "solve"    the same without the L and D_inv blocks
 *   "forward"  ForwardSub(blocks, keys, rhs) with the blocks taken as L (no factorisation, no
 *   "back"     symmetry asked; BackSub takes them as L^T) over the key order `keys`: "x\t<key>"
 * `keys` is read by "forward" / "back" only.  Argument errors - an unknown mode, no blocks, a null
 * key, a pair given twice, a payload that does not parse, blocks whose sizes or transposes do not
 * fit, a rhs key the matrix (or `keys`) lacks or of another length - fail before any device work and
 * name the key or argument; a matrix with no eliminable key fails in Compute.  *out is NULL on
 * failure. */
typedef struct eps_block {
  const char* row;
  const char* col;
  const void* linear_map; /* protobuf wire bytes of `LinearMap` */
  size_t len;
} eps_block;
int eps_test_block_solve(const char* mode, const eps_block* blocks, size_t nblocks,
                         const eps_blob* data, size_t ndata, const eps_blob* rhs, size_t nrhs,
                         const char* const* keys, size_t nkeys, eps_result** out);

/* Test entry: ONE call of a public launcher of the dense mat-vec layer (csrc/kernels.h: Gemv,
 * Symv, SymvPack + SymvPacked, ReducePartials, SumSq, SumSqDiff, Dot, Axpby, DiagMul) on
 * caller-given operands, in the configured dtype.  `op` and what the operands mean:
 *   "gemv_n"           y = alpha A x + beta y        a: A, rows x cols, leading dimension lda
 *   "gemv_t"           y = alpha A^T x + beta y      (a has (cols - 1) lda + rows entries)
 *   "symv"             y = alpha S x + beta y        a: S, n x n with n = rows, lda = lds
 *   "symv_packed"      the same through SymvPack + SymvPacked into out, and through Symv on the
 *                      same operands into out2
 *   "reduce_partials"  y = alpha sum_k a[k rows + r] + beta y (+ add with with_add), k < nparts
 *   "sumsq" "sumsq_diff" "dot"   slot (+)= sum x^2, sum (x - y)^2, sum x y over n = rows entries;
 *                      the slot holds `preset` before the call, out[0] receives it afterwards
 *   "axpby"            y = alpha x + beta y over n = rows entries; alias_xy: x IS y (x not read
 *                      from the caller)
 *   "diag_mul"         y = alpha a .* x + beta y
 * Every operand is uploaded into a larger allocation and handed to the launcher as the slice that
 * starts *_off elements in: offset 0 is 16-byte aligned, an odd offset is not.  The output y
 * starts as the caller's y_len values between EPS_DENSE_OP_GUARD guard elements on each side, all
 * EPS_DENSE_OP_SENTINEL; out receives guard + y_len + guard values, so a store outside the output
 * shows.  use_work: Symv / SymvPacked with a caller-side workspace instead of the pool's.
 * The argument checks - an unknown op, a null operand or result, a negative size or offset,
 * lda < rows, nparts < 1, an operand whose length is not what the dimensions need - fail before
 * any device work and name the argument. */
#define EPS_DENSE_OP_GUARD 8
#define EPS_DENSE_OP_SENTINEL (-777.25)
typedef struct eps_dense_op {
  const char* op;
  int64_t rows, cols, lda;
  int nparts;
  double alpha, beta;
  const double* a;   int64_t a_len, a_off;
  const double* x;   int64_t x_len, x_off;
  const double* y;   int64_t y_len, y_off;
  const double* add; int64_t add_len, add_off;
  int accumulate, use_work, with_add, alias_xy;
  double preset;
} eps_dense_op;
int eps_test_dense_op(const eps_dense_op* args, double* out, double* out2);

/* Test entry: ONE call of a public launcher of the dense mat-mat layer (csrc/kernels.h: Gemm,
 * GemmBatched, MatCopy, AddDiag, SymmetrizeFromLower, ColAbsSums, KronDense) on caller-given
 * column-major operands, in the configured dtype.  `op` and what the operands mean:
 *   "gemm"          C (M x N, ldc) = alpha op(A) op(B) + beta C; op(A) is M x K, op(B) K x N, a
 *                   transposed operand is stored K x M / N x K; lower_only as in Gemm
 *   "gemm_batched"  the same for batch * outer problems z: A at (z % batch) sA + (z / batch) sA2,
 *                   B likewise, C at z sC
 *   "mat_copy"      c (M x N, contiguous) = alpha a, or alpha a^T with trans_a (a stored N x M); lda
 *   "add_diag"      c (M x M, ldc): c_ii += alpha d_i, or += alpha when d is NULL
 *   "symmetrize"    c (M x M, ldc): the strict upper triangle becomes the mirror of the lower one
 *   "col_abs_sums"  out: the N column sums of |a| (a: M x N, lda), device doubles in every dtype
 *   "kron"          c = kron(a, b), a M x N and b K x batch (!), all three contiguous
 * a, b, c and d are copied verbatim - padding rows and the gaps between batch members included,
 * filled by the caller - into larger allocations, *_off + EPS_DENSE_OP_GUARD elements in (offset
 * 0 is 16-byte aligned, an odd offset is not).  out receives the whole result allocation from
 * c_off on: guard + c_len + guard values (guard + N + guard for col_abs_sums), the guards
 * EPS_DENSE_OP_SENTINEL unless something stored there.  route (at least 16 characters) receives
 * the branch Gemm / GemmBatched took (csrc/kernels.h GemmLastRoute), "" for the other ops.
 * The argument checks - an unknown or null op, a null operand or result, a negative size, offset
 * or stride, a leading dimension below the rows it holds, a buffer whose length is not
 * (cols - 1) ld + rows (plus the strides to the last batch member), results that overlap,
 * lower_only with M != N - fail before any device work and name the argument. */
typedef struct eps_gemm_op {
  const char* op;
  int trans_a, trans_b;
  int64_t M, N, K;
  double alpha, beta;
  int64_t lda, ldb, ldc;
  int64_t a_off, b_off, c_off;
  int64_t batch, outer, sA, sB, sC, sA2, sB2;
  int lower_only;
  const double* a; int64_t a_len;
  const double* b; int64_t b_len;
  const double* c; int64_t c_len;
  const double* d; int64_t d_len;
} eps_gemm_op;
int eps_test_gemm_op(const eps_gemm_op* args, double* out, char* route, size_t route_cap);

/* Test entry: ONE call of a public launcher of the dense factor layer (csrc/kernels.h:
 * SpdInverseInPlace, SpdInverseColumns; csrc/kernels_factor.hip) on a caller-given column-major
 * n x n matrix a (ld n), in the configured dtype.  `op` and what the results mean:
 *   "spd_inverse"          SpdInverseInPlace(W, n, out2 ? &X : NULL): out receives guard + n^2 +
 *                          guard values of W (the inverse, both triangles); out2 (optional) the n^2
 *                          values of X = L^-1, the factor_inverse the whitened route streams
 *   "spd_inverse_columns"  SpdInverseColumns(W, n, lo, cnt, Out) with Out allocated n * out_cols,
 *                          out_cols >= cnt (the padded slab of InverseDistributed): out receives
 *                          guard + n * out_cols + guard values; out2 (optional) the n^2 values of W
 *                          afterwards, whose lower triangle is the Cholesky factor (the strict upper
 *                          triangle is scratch).  cnt == 0 returns right after the factorisation:
 *                          the pure-Cholesky entry.
 * a is uploaded as given, upper triangle included, a_off + EPS_DENSE_OP_GUARD elements into a larger
 * allocation (offset 0 is 16-byte aligned, an odd offset is not); the elements around it and every
 * element of Out start as EPS_DENSE_OP_SENTINEL, so a store outside a result shows in the guards
 * and in the padded columns cnt .. out_cols.  form (-1, 0 or 1, as in eps_test_spd_inverse_repeat)
 * goes through SetPotrfForm for the one call and is back at -1 on every exit path.
 * The argument checks - an unknown or null op, a null a or out, n < 0, a_len != n * n, a negative
 * offset, form outside -1..1, lo < 0, cnt < 0, lo + cnt > n, out_cols < cnt, a result or a slab
 * argument given to an op that has none (today: lo, cnt or out_cols with "spd_inverse"; both ops
 * have an out2) - fail before any device work and name the argument.  A non-positive
 * pivot is the launcher's own error, "dense inverse: matrix is not positive definite", returned as
 * any other error. */
typedef struct eps_factor_op {
  const char* op;
  int64_t n;
  int form;
  const double* a; int64_t a_len, a_off;
  int64_t lo, cnt, out_cols;
} eps_factor_op;
int eps_test_factor_op(const eps_factor_op* args, double* out, double* out2);

/* Test entry: ONE call of one launcher of the sparse layer (csrc/sparse.h: SpmvCsr, SpmmCsrDense,
 * DenseSpmmCsc, ScatterAddCsc; csrc/kernels_sparse.hip) on caller-given operands, in the
 * configured dtype.  The sparse operand is the CSR matrix (ptr, idx, val), rows x cols with nnz
 * stored entries, exactly as the launcher receives it; `op` and what the other operands mean:
 *   "spmv"             y (rows) = alpha S x + beta y; d: x, cols entries; beta == 0 never reads y
 *   "spmm_csr_dense"   C (rows x n, ld rows) = alpha S B; d: B, cols x n column-major with leading
 *                      dimension ld, (n - 1) ld + cols entries
 *   "dense_spmm_csc"   C (n x rows, ld n) = alpha A F, where the CSR operand is that of the
 *                      TRANSPOSE of the sparse factor (F = S^T, cols x rows, i.e. F in CSC form);
 *                      d: A, n x cols column-major with leading dimension ld,
 *                      (cols - 1) ld + n entries
 *   "scatter_add_csc"  W (cols x rows column-major, ld cols) += alpha F, F = S^T as above; y: W;
 *                      entries within one row of the CSR operand must be unique
 * d is uploaded verbatim, padding rows included.  The output starts as the caller's y_len values
 * of y between EPS_DENSE_OP_GUARD guard elements on each side, all EPS_DENSE_OP_SENTINEL; out
 * receives guard + y_len + guard values, so a store outside the output shows.
 * The argument checks - an unknown or null op, a null array or result, a negative size, ptr not of
 * rows + 1 entries, not starting at 0, not monotone or not ending at nnz, idx or val not of nnz
 * entries, a column index outside [0, cols), ld below the rows it holds, d or y not of the length
 * the dimensions need, d, ld, n or beta given to an op that has none - fail before any device
 * work and name the argument: no malformed structure reaches a kernel. */
typedef struct eps_sparse_op {
  const char* op;
  int64_t rows, cols, nnz;
  const int32_t* ptr; int64_t ptr_len;
  const int32_t* idx; int64_t idx_len;
  const double* val;  int64_t val_len;
  double alpha, beta;
  const double* d;    int64_t d_len, ld, n;
  const double* y;    int64_t y_len;
} eps_sparse_op;
int eps_test_sparse_op(const eps_sparse_op* args, double* out);

/* Test entry: the host CSC algebra of csrc/sparse.h (CscTranspose, CscAdd, CscMultiply, CscKron,
 * CscScaleRows, CscScaleCols, CscFromDense, CscFromBlob).  It touches no device.  `op`:
 *   "transpose"                  a^T
 *   "add" "multiply" "kron"      a + b, a b, kron(a, b)
 *   "scale_rows" "scale_cols"    diag(d) a, a diag(d); d of one entry is a scalar
 *   "from_dense"                 the a.m x a.n column-major matrix d without its exact zeros
 *   "from_blob"                  the wire blob (int32 col_ptr[n + 1] | int32 row_index[nnz] |
 *                                float64 values[nnz]) of an a.m x a.n matrix with a.nnz entries
 * An operand is m x n with nnz stored entries in column-compressed form, row indices strictly
 * ascending within each column ("from_dense" and "from_blob" read only a.m, a.n and a.nnz).  The
 * result goes to colptr (colptr_cap entries, at least its n + 1), rowidx and val (nnz_cap entries
 * each); *m, *n and *nnz receive its size.
 * The argument checks - an unknown or null op, a null array or result, a negative size, column
 * pointers not of n + 1 entries, not starting at 0, not monotone or not ending at nnz, rowidx or
 * val not of nnz entries, a row index outside [0, m) or not ascending within its column, operand
 * sizes that do not fit each other, d not of the length the op needs, a result larger than the
 * capacities - name the argument; a malformed blob is CscFromBlob's own error ("sparse blob ..."). */
typedef struct eps_csc {
  int64_t m, n, nnz;
  const int32_t* colptr; int64_t colptr_len;
  const int32_t* rowidx; int64_t rowidx_len;
  const double* val;     int64_t val_len;
} eps_csc;
typedef struct eps_csc_op {
  const char* op;
  eps_csc a, b;
  const double* d;  int64_t d_len;
  const void* blob; size_t blob_len;
  int32_t* colptr;  int64_t colptr_cap;
  int32_t* rowidx;  double* val; int64_t nnz_cap;
} eps_csc_op;
int eps_test_csc_op(const eps_csc_op* args, int64_t* m, int64_t* n, int64_t* nnz);

/* Test entry: a sparse map HANDLE as an operand.  The wire format has no product node, so
 * eps_linear_map_binary cannot be given a sparse map that carries a lazy scalar factor; this
 * entry builds one.  sparse_map: wire bytes of a SPARSE_MATRIX `LinearMap` S with its data blobs.
 * The handle is H = S, transposed with `transpose`, then - with `scaled` - the scalar map product
 * Scalar(scale) * H (SparseMatrixImpl::Scaled: same core, a factor the callers fold into alpha).
 * With p (S.n entries) the map as built is applied to p FIRST and the S.m values go to out2: the
 * core has then cached the CSR copy of the plain direction before the handle asks for its own.
 * `op` and the dense operand d (d_rows x d_cols, column-major, contiguous):
 *   "apply"    out = H d        (d_cols == 1)     "adjoint"  out = H^T d  (d_cols == 1)
 *   "sparse_dense"  out = H * D     "dense_sparse"  out = D * H      (Dense results)
 *   "sparse_plus_dense"  out = H + D     "dense_plus_sparse"  out = D + H
 * out receives the result (column-major) and needs out_cap >= its size.  The argument checks - an
 * unknown or null op, a null payload, operand or result, a map that is not a sparse matrix,
 * a dense operand whose size does not fit, out_cap too small - name the argument. */
typedef struct eps_sparse_handle_op {
  const char* op;
  const void* sparse_map; size_t len;
  const eps_blob* data;   size_t ndata;
  int transpose, scaled;
  double scale;
  const double* p; int64_t p_len;
  const double* d; int64_t d_rows, d_cols;
} eps_sparse_handle_op;
int eps_test_sparse_handle_op(const eps_sparse_handle_op* args, double* out, int64_t out_cap, double* out2);

/* Microbenchmark: average milliseconds of one launch of a standalone elementwise prox kernel on
 * n synthetic elements of the configured dtype - kind 0 scaled-zone (NORM_1) with scalar
 * parameters, 1 with a per-element threshold vector, 2 projection onto R+ (reference
 * prox/scaled_zone.cc:90-101, prox/non_negative.cc:8).  Algorithmic bytes 2 n s (3 n s for kind 1). */
int eps_bench_prox(int kind, int64_t n, int iters, double* ms_avg);

/* Microbenchmark of the singular value decomposition behind the orthogonally-invariant prox
 * operators (reference prox/ortho_invariant.cc:36-50) on the reference's robust-PCA matrix
 * (problems/robust_pca.py:5-22: rank-`rank` part + 10 % sparse part) of the configured dtype:
 * milliseconds and Jacobi sweeps of a cold decomposition and of a warm-started one of a matrix
 * `perturb` away (perturb < 0: skipped).  defects (6 doubles, may be NULL), cold then warm:
 * ||V^T V - I||_F / sqrt(n), ||W V^T - Y||_F / ||Y||_F, ||offdiag(W^T W)||_F / ||diag(W^T W)||_F. */
int eps_bench_svd(int64_t m, int64_t n, int rank, int max_sweeps, double perturb, double* ms_cold,
                  int* sweeps_cold, double* ms_warm, int* sweeps_warm, double* defects);

/* The same decomposition (cold) of a caller-provided m x n column-major float32 matrix in HBM. */
int eps_bench_svd_device(const void* y_dev, int64_t m, int64_t n, int max_sweeps, double* ms, int* sweeps);

/* Exact 1-D total-variation prox of v (n float64) with weight lam
 * (reference prox/total_variation_1d.cc:21 -> glmgen tf_dp). */
int eps_tv1d(const double* v, size_t n, double lam, double* x);

/* The same on device-resident data (the work runs on the library's own non-blocking stream; the
 * call waits for the device first, so v may come straight from the caller's streams): v, x are
 * device pointers to n elements of `kind`
 * (EPS_BLOB_DEVICE_F32 / EPS_BLOB_DEVICE_F64); *levels (may be NULL) receives the depth of the
 * level-set recursion of this call, 0 when the call is trivial (n <= 1 or lam == 0: x = v).
 * Synchronises before returning. */
int eps_tv1d_device(const void* v_dev, void* x_dev, size_t n, int kind, double lam, int* levels);

/* The prox of `count` signals of `len` samples each in one pass: v and x hold the signals one
 * after the other (signal s is v[s * len .. s * len + len - 1]), every signal is solved on its
 * own - no term couples the last sample of one to the first sample of the next - and one lam
 * serves all of them.  len * count must be below 2^31 - 1.  count == 1 is eps_tv1d. */
int eps_tv1d_batch(const double* v, size_t len, size_t count, double lam, double* x);

/* The same on device-resident data, with the conventions of eps_tv1d_device: v, x are device
 * pointers to len * count elements of `kind`, signal s at elements [s * len, (s + 1) * len);
 * *levels (may be NULL) receives the depth of the level-set recursion, the maximum over the
 * signals, 0 when the call is trivial (len <= 1, count == 0 or lam == 0).  Synchronises before
 * returning. */
int eps_tv1d_batch_device(const void* v_dev, void* x_dev, size_t len, size_t count, int kind, double lam,
                          int* levels);

#ifdef __cplusplus
}
#endif

#endif /* EPSILON_HIP_H_ */
