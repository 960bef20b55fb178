/*
 * rpm_hip.h — C ABI of the MI355X-native Radau-pseudospectral NLP-callback engine.
 *
 * This is the drop-in boundary for lpopc's per-iteration hot path.  Every entry
 * point replaces one interface of the reference (paths relative to
 * /root/reference/Lpopc/src, cited per function below).  Plain C types only:
 * `int` is Ipopt::Index, `double` is Ipopt::Number (Core/LpopcIpopt.h:33-82).
 *
 * Conventions
 *   - every function returns 0 on success and a non-zero RPM_E_* code on failure;
 *     no C++ exception ever crosses this boundary (the reference throws
 *     LP_THROW_EXCEPTION, Common/LpException.hpp:78).  The message of the last
 *     failure is available from rpm_last_error().
 *   - the set-up half (rpm_create, rpm_get_nlp_info, rpm_get_bounds_info,
 *     rpm_get_starting_point, structure pass of rpm_eval_jac_g / rpm_eval_h,
 *     rpm_get_phase_tables, rpm_shard_*) is host-only and needs no GPU.
 *   - the evaluation half runs hand-written HIP kernels on gfx950.  There is NO
 *     CPU fallback: without a usable device these calls fail with RPM_E_DEVICE.
 *   - an engine may hold `n_instances` structurally identical OCP instances
 *     (the batched MPC sweep).  All vectors are then instance-major:
 *     x[inst*n + i], g[inst*m + i], values[inst*nnz + k].  n/m/nnz reported by
 *     rpm_get_nlp_info are always per instance.
 */
#ifndef RPM_HIP_H_
#define RPM_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#define RPM_ABI_VERSION 2

/* ---- error codes -------------------------------------------------------- */
enum {
  RPM_OK = 0,
  RPM_E_INVALID = 1,  /* bad argument / inconsistent description (LpSizeChecker, LpBoundsChecker,
                         LpGuessChecker, LpMeshRefiner exceptions in the reference) */
  RPM_E_UNSUPPORTED = 2,
  RPM_E_DEVICE = 3,   /* HIP error or no device */
  RPM_E_NONFINITE = 4 /* a result contains NaN/Inf (the reference always returns true) */
};

/* ---- problem functor ids ------------------------------------------------- */
/* The reference's user callbacks are host C++ virtuals on Armadillo matrices
 * (Core/LpFunctionWrapper.h:50-69); they cannot run on a GPU.  Here the five
 * callbacks (Mayer, Lagrange, Dae, Event, Link) are pointwise device functors
 * compiled into the library and selected by id. */
enum {
  RPM_PROBLEM_LAUNCH = 1,          /* Delta-III ascent, example/launch/Launch.cpp:620-765 */
  RPM_PROBLEM_HYPERSENSITIVE = 2,  /* example/hypersensitive/HyperSensitive.cpp:74-167 */
  RPM_PROBLEM_BRYSON_DENHAM = 3,   /* example/bryson-denham/BrysonDenham.cpp:100-167 */
  RPM_PROBLEM_BRACHISTOCHRONE = 4, /* authored here (BASELINE config 1) */
  RPM_PROBLEM_MIN_TIME_CLIMB = 5,  /* authored here (BASELINE config 2) */
  RPM_PROBLEM_QUADROTOR = 6,       /* authored here (BASELINE config 5) */
  RPM_PROBLEM_PARAM_SLED = 7,      /* authored here: minimum-time sled with one static parameter (nq = 1), known optimum 2.5 */
  RPM_PROBLEM_PARAM_OSC = 8,       /* authored here: two linked phases, two static parameters each (nq = 2), path + events + links on them
                                      (both: limited-memory or RPM_HESSIAN_EXACT_PARAMETERS, never plain RPM_HESSIAN_EXACT) */
  RPM_PROBLEM_USER = 100           /* the functor `rpm::UserProblem` of a user's header, in a library built from that header
                                      (lpopc_amd/userproblem.py, INTEGRATION.md "your own problem"): the stand-in for
                                      subclassing FunctionWrapper (Core/LpFunctionWrapper.h:50-69) */
};

/* first-derive option, Core/LpOptDerive.hpp:29-32 */
enum { RPM_DERIVE_FINITE_DIFFERENCE = 0, RPM_DERIVE_ANALYTIC = 1 };
/* hessian-approximation option, Core/LpNLPWrapper.hpp:71-72 */
enum {
  RPM_HESSIAN_LIMITED_MEMORY = 0,
  RPM_HESSIAN_EXACT = 1,             /* lpopc's own second differences; refused for problems with static parameters (nq > 0) */
  RPM_HESSIAN_EXACT_PARAMETERS = 2   /* "exact-parameters": the same Hessian with the rows of the static parameters by the corrected
                                        formulas (DESIGN.md section 3 lists every departure from Core/LpHessian.cpp); with nq = 0 in
                                        every phase it is RPM_HESSIAN_EXACT bit for bit.  rpm_create turns it into RPM_HESSIAN_EXACT
                                        plus an engine flag: everything downstream sees an exact-Hessian engine */
};
/* how work is split when shard_world > 1 */
enum { RPM_SHARD_NONE = 0, RPM_SHARD_INTERVALS = 1 };

/* ---- problem description (what Phase/Linkage/OptimalProblem setters collect,
 *      Core/LpOptimalProblem.hpp:30-326) ------------------------------------- */
typedef struct rpm_phase_desc {
  int nx, nu, nq, nc, ne;          /* Phase(idx,nx,nu,nq,nc,ne)  :33-37 */
  int n_intervals;                 /* SetMeshPoints/SetNodesPerInterval :174-187 */
  const double* mesh_points;       /* n_intervals+1, must run -1 .. +1 (Core/LpMeshRefiner.cpp:40) */
  const int* nodes_per_interval;   /* n_intervals, each >= 2 */
  double t0_min, tf_min;           /* SetTimeMin(t0,tf) :49 */
  double t0_max, tf_max;           /* SetTimeMax(t0,tf) :57 */
  const double* state_min;         /* nx*3: {state0,state,statef} per state, SetStateMin :65 */
  const double* state_max;         /* nx*3 */
  const double* control_min;       /* nu */
  const double* control_max;
  const double* parameter_min;     /* nq */
  const double* parameter_max;
  const double* path_min;          /* nc */
  const double* path_max;
  const double* event_min;         /* ne */
  const double* event_max;
  int has_duration;                /* SetDuration :126 */
  double duration_min, duration_max;
  int n_guess;                     /* number of guess knots (>=2), SetTimeGuess :132 */
  const double* time_guess;        /* n_guess */
  const double* state_guess;       /* nx*n_guess, knot-fastest per state (SetStateGuess(i,v)) */
  const double* control_guess;     /* nu*n_guess */
  const double* parameter_guess;   /* nq */
} rpm_phase_desc;

typedef struct rpm_link_desc {
  int left_phase, right_phase;     /* 1-based, Linkage(ipair,left,right) :245 */
  int n_links;
  const double* link_min;          /* n_links */
  const double* link_max;
} rpm_link_desc;

typedef struct rpm_problem_desc {
  int abi_version;                 /* RPM_ABI_VERSION */
  int problem_id;                  /* RPM_PROBLEM_* */
  int n_phases;
  const rpm_phase_desc* phases;
  int n_links;
  const rpm_link_desc* links;
  int n_consts;                    /* problem constants handed to the functor (the reference keeps
                                      them in globals, e.g. CONSTANTS in example/launch/Launch.cpp:47-74) */
  const double* consts;
  double fd_tol;                   /* finite-difference-tol, default 1e-6 */
  int first_derive;                /* RPM_DERIVE_* */
  int hessian_approximation;       /* RPM_HESSIAN_* */
  int n_instances;                 /* >=1; structurally identical OCPs evaluated per call */
  int shard_mode;                  /* RPM_SHARD_* */
  int shard_rank, shard_world;     /* this engine computes only the tiles it owns */
} rpm_problem_desc;

typedef struct rpm_engine rpm_engine;

/* ---- lifecycle ------------------------------------------------------------
 * rpm_create does what LpopcAlgorithm::GetSizes/GetBounds/GetGuess do once per mesh
 * (Core/LpLpopcAlgorithm.cpp:143-148): size/bounds/guess checks, NLP layout
 * (Core/LpBoundsChecker.cpp:13-348), collocation tables (Core/RPMGenerator.cpp:43-181),
 * Jacobian structure (Core/LpNLPWrapper.cpp:1106-1578).  Host only. */
int rpm_create(const rpm_problem_desc* desc, rpm_engine** out);
void rpm_destroy(rpm_engine* e);
/* message of the last failed call on this engine (or of the last failed rpm_create when e==NULL) */
const char* rpm_last_error(const rpm_engine* e);
/* bind the engine to HIP device `device_id`, allocate device tables/buffers, create its stream.
 * Called implicitly (device 0) by the first evaluation if omitted. */
int rpm_device_init(rpm_engine* e, int device_id);

/* ---- Ipopt::TNLP surface (Core/LpopcIpopt.h:33-82, Core/LpopcIpopt.cpp) ------- */
/* LpopcIpopt::get_nlp_info, LpopcIpopt.cpp:11-24.  index_style: 0 = C_STYLE. */
int rpm_get_nlp_info(rpm_engine* e, int* n, int* m, int* nnz_jac_g, int* nnz_h_lag, int* index_style);
/* LpopcIpopt::get_bounds_info, LpopcIpopt.cpp:26-82 */
int rpm_get_bounds_info(rpm_engine* e, int n, double* x_l, double* x_u, int m, double* g_l, double* g_u);
/* LpopcIpopt::get_starting_point, LpopcIpopt.cpp:84-104 (requires init_x=1, init_z=0, init_lambda=0) */
int rpm_get_starting_point(rpm_engine* e, int n, int init_x, double* x, int init_z, double* z_L,
                           double* z_U, int m, int init_lambda, double* lambda);
/* LpopcIpopt::eval_f, LpopcIpopt.cpp:106-116 -> NLPWrapper::GetObjFun, LpNLPWrapper.cpp:863 */
int rpm_eval_f(rpm_engine* e, int n, const double* x, int new_x, double* obj_value);
/* LpopcIpopt::eval_grad_f, LpopcIpopt.cpp:118-133 -> GetObjGrad, LpNLPWrapper.cpp:940 */
int rpm_eval_grad_f(rpm_engine* e, int n, const double* x, int new_x, double* grad_f);
/* LpopcIpopt::eval_g, LpopcIpopt.cpp:135-150 -> GetAllCons, LpNLPWrapper.cpp:34 */
int rpm_eval_g(rpm_engine* e, int n, const double* x, int new_x, int m, double* g);
/* LpopcIpopt::eval_jac_g, LpopcIpopt.cpp:152-181: values==NULL -> structure pass (iRow/jCol,
 * 0-based), else values pass -> GetConsJacbi, LpNLPWrapper.cpp:230 */
int rpm_eval_jac_g(rpm_engine* e, int n, const double* x, int new_x, int m, int nele_jac, int* iRow,
                   int* jCol, double* values);
/* Both constraint callbacks in one call (host pointers): what Ipopt's back-to-back eval_g(x, new_x = true) +
 * eval_jac_g(x, new_x = false) pair (LpopcIpopt.cpp:135-181) asks for, for callers that can take both results at once
 * (an SQP / own interior-point loop, the MPC sweep's host driver): one launch writes g straight into the caller's
 * page-locked array and the Jacobian values into HBM, a second queue operation delivers `values`, ONE synchronisation.
 * Same results as the two calls, same options ("pin_host", "zero_copy", "const_once", "delta_values"). */
int rpm_eval_pair(rpm_engine* e, int n, const double* x, int m, double* g, int nele_jac, double* values);
/* LpopcIpopt::eval_h, LpopcIpopt.cpp:183-218 -> LpHessianCalculator::GetHessian, LpHessian.cpp:878 */
int rpm_eval_h(rpm_engine* e, int n, const double* x, int new_x, double obj_factor, int m,
               const double* lambda, int new_lambda, int nele_hess, int* iRow, int* jCol,
               double* values);
/* LpopcIpopt::finalize_solution, LpopcIpopt.cpp:220-246: keeps x, lambda, obj for rpm_get_solution */
int rpm_finalize_solution(rpm_engine* e, int status, int n, const double* x, const double* z_L,
                          const double* z_U, int m, const double* g, const double* lambda,
                          double obj_value);
int rpm_get_solution(rpm_engine* e, int n, double* x, int m, double* lambda, double* obj_value);

/* ---- solution extraction (the step after the NLP solve) -----------------------
 * Nlp2OpConverter::Nlp2OpControl, Core/Nlp2OPConverter.cpp:13-196, for one phase: time, states, controls (with the
 * spline-extrapolated value at tau=+1 appended), costates -W^-1 lambda (and -D(:,N)' lambda at the end point), path
 * multipliers, Hamiltonian, Mayer and Lagrange cost.  Outputs are host arrays with N+1 rows, column-major; any may
 * be NULL.  x / lambda are host arrays; NULL = the solution stored by rpm_finalize_solution.  The time/state/
 * control arrays are also what the reference installs as the next mesh's guess (:149-193). */
int rpm_nlp2op_control(rpm_engine* e, int phase, const double* x, const double* lambda, double* time, double* state,
                       double* control, double* costate, double* pathmult, double* hamiltonian, double* mayer_cost,
                       double* lagrange_cost);
/* Nlp2OpConverter::FinalResultSave, Core/Nlp2OPConverter.cpp:198-223: writes time<k>, state<k>, control<k>, parameter<k>,
 * costate<k>, Hamiltonian<k> (Armadillo raw_ascii: one row per line) for every phase k into `dir`. */
int rpm_final_result_save(rpm_engine* e, const char* dir);

/* ---- mesh-error estimate and ph mesh refinement (after extraction) ------------
 * SolutionErrorChecker::CheckSolutionDiffError, Core/LpSolutionError.cpp:112-169, for one phase: the solution is
 * interpolated onto a mesh with one more LGR point per interval (:46-108), the dynamics are integrated there with
 * inv(D(:,1:)) (Core/RPMGenerator.cpp:85), and rel_err = |integrated - interpolated| / (1 + max of the state's column).
 * rel_err is a host array, (N + K + 1) rows x nx, column-major (K = mesh intervals); *rows receives the row count
 * (rel_err may be NULL to query it).  x is a host array; NULL = the solution stored by rpm_finalize_solution. */
int rpm_solution_error(rpm_engine* e, int phase, const double* x, double* rel_err, int* rows);
/* PhMeshRefineAlg::RefineMesh + ModifySegment, Core/LpPhMeshRefineAlg.cpp:12-100, for one phase: an interval whose
 * largest relative error is <= tol is kept; otherwise it gets Pq = int(log(emax/tol)/log(n)) more nodes, or, when
 * that exceeds nmax, is split into max(ceil((n+Pq)/nmin), 2) intervals of nmin nodes.  Outputs (any may be NULL):
 * new_mesh_points (new_n_intervals + 1), new_nodes_per_interval (new_n_intervals; both need `capacity` >= that
 * count, query it first with NULL arrays), interval_error (K, the per-interval maxima), no_more_refine (1 when
 * every interval met tol: the reference's NoMoreRefine).  The caller installs the new mesh with a new rpm_create,
 * as the reference re-runs GetSizes/GetBounds/GetGuess per mesh (Algorithm/LpLpopcAlgorithm.cpp:147-169). */
int rpm_ph_refine_mesh(rpm_engine* e, int phase, const double* x, double tol, int nmin, int nmax, int capacity,
                       double* new_mesh_points, int* new_nodes_per_interval, int* new_n_intervals,
                       double* interval_error, int* no_more_refine);

/* The refinement decision alone, from a relative_error matrix the caller already holds (host only, no device work). */
int rpm_ph_refine_from_error(rpm_engine* e, int phase, const double* rel_err, double tol, int nmin, int nmax,
                             int capacity, double* new_mesh_points, int* new_nodes_per_interval,
                             int* new_n_intervals, double* interval_error, int* no_more_refine);

/* The estimate for a whole sweep: all phases and all n_instances instances of the engine at once, every instance with its
 * own constants (rpm_set_instance_constants) and static parameters.  Per instance the arithmetic is rpm_solution_error's,
 * sum by sum in the same order, so the results are the same bits.  Sizes (host only, no device needed): KT = sum over the
 * phases of K_p, RT = sum over the phases of (N_p + K_p + 1) * nx_p.  A block of RT doubles holds the phases' relative_error
 * matrices one after the other, each (N_p + K_p + 1) x nx_p column-major, as rpm_solution_error returns them and
 * rpm_hpliu_refine takes them.  Results (any may be NULL):
 *   interval_error  n_instances x KT, instance-major, phase after phase: the per-interval maxima, equal to rpm_ph_refine_mesh's;
 *   rel_err_max     RT: element-wise maximum over the instances that instance_mask includes (NULL mask = all; a NaN stays).
 *                   The instances of a sweep share one transcription, so they share the next mesh: the one the worst
 *                   instance asks for, rpm_ph_refine_from_error(e, p, rel_err_max + offset of phase p, ...);
 *   rel_err         n_instances x RT, every instance's block;
 *   nonfinite       n_instances: 1 when the instance's block holds a NaN or Inf (instances that ended with status 3 or 5).
 * An excluded instance (mask 0) is still estimated and reported; it only stays out of rel_err_max.
 * The _dev form takes device arrays (x packed n_instances x n) and queues three launches (four above 64 instances) on `stream` (a hipStream_t, NULL =
 * the legacy default stream).  The first call on an engine uploads the tables and allocates the workspace; every later call
 * allocates nothing, copies nothing and never synchronises, so it can follow rpm_ipm_solve_dev on the caller's stream and be
 * captured into a graph.  It cannot see its mask: with every instance excluded rel_err_max is all zeros.  The host-pointer
 * form stages its arrays like the other host-pointer calls, blocks, and answers RPM_E_INVALID when rel_err_max is asked for
 * and the mask excludes every instance.  Interval-sharded engines: RPM_E_UNSUPPORTED.  The calling thread's current device
 * is restored.  Option "mesh_err_tile" (0 = automatic, 1, 2, 4, 8, 16): instances per workgroup. */
int rpm_solution_error_batch_sizes(rpm_engine* e, int* n_intervals_total, long long* rel_doubles_total);
int rpm_solution_error_batch_dev(rpm_engine* e, const double* d_x, const int* d_instance_mask, double* d_interval_error,
                                 double* d_rel_err_max, double* d_rel_err, int* d_nonfinite, void* stream);
int rpm_solution_error_batch(rpm_engine* e, const double* x, const int* instance_mask, double* interval_error,
                             double* rel_err_max, double* rel_err, int* nonfinite);

/* A sweep's solutions carried onto another mesh: the fourth step of solve, estimate, refine, re-solve.  `from` is the engine the
 * solutions were computed on, `to` an engine of the same problem (same problem id, phase count, per-phase nx / nu / nq and
 * n_instances) on any other mesh: refined, coarsened or the same; to == from is legal.  x_from: n_instances x from.n, x_to:
 * n_instances x to.n, both instance-major; nonfinite: n_instances ints or NULL, 1 when any carried value of the instance is NaN
 * or Inf (an instance with NaN / Inf or with tf == t0 yields NaN / Inf for itself only).  Per instance, phase and column the
 * arithmetic is that of the one-instance route — rpm_nlp2op_control's time and control-at-tau=1, a new rpm_create carrying them
 * as the guess, rpm_get_starting_point — operation by operation: time[k] = (tf - t0) (tau_k + 1) / 2 + t0, knots
 * 2 (time[k] - time[0]) / (time[N] - time[0]) - 1, the natural cubic spline of LpGuessChecker through the N + 1 knots evaluated
 * at the target's points (states also at 1), t0 = time[0], tf = time[N], static parameters copied.  Only the spline's cubes
 * differ: A * A * A on the device, pow(A, 3) on the host, so the two routes agree to rounding, not to the bit; t0, tf and the
 * parameters agree to the bit.  Multipliers are carried by rpm_carry_multipliers_batch below.  The caller builds the
 * next engine and re-applies per-instance constants and bounds.
 * Argument errors are decided on the host before anything is queued: NULL arrays, engines that do not match, engines bound
 * to different devices, overlapping x_from / x_to: RPM_E_INVALID; interval-sharded engines, a column that does not fit one
 * workgroup's LDS: RPM_E_UNSUPPORTED (columns that do not fit together are dealt over several workgroups).  The message is
 * rpm_last_error(from).
 * The _dev form takes device arrays and queues one launch (two with d_nonfinite) on `stream`.  The first call on a pair of
 * engines uploads a small launch plan (and initialises an engine that has no device yet on the other's device); every later
 * call allocates nothing, copies nothing and never synchronises, so it can follow rpm_ipm_solve_dev on the caller's stream and be
 * captured into a graph.  The host-pointer form stages its arrays and blocks.  The calling thread's current device is
 * restored.  Option "carry_tile" (0 = automatic, 1, 2, 4, 8) on `from`: instances per workgroup; every value gives the same bits. */
int rpm_carry_solution_batch_dev(rpm_engine* from, rpm_engine* to, const double* d_x_from, double* d_x_to, int* d_nonfinite,
                                 void* stream);
int rpm_carry_solution_batch(rpm_engine* from, rpm_engine* to, const double* x_from, double* x_to, int* nonfinite);
/* The constraint multipliers of a sweep carried onto another mesh, as costates: the starting lambda of rpm_ipm_solve_warm on the
 * next mesh.  lambda_from: n_instances x from.m, lambda_to: n_instances x to.m, instance-major; x_from (n_instances x from.n)
 * supplies every phase's t0 and tf, so the knots are those of the solution carry.  Per instance and phase, rows read with the
 * phase's own first row g0:
 *   defect rows of state s:     c_k = -(1 / w_k) lambda[g0 + s N + k], k < N, c_N = the end-point costate -D(:,N)' lambda_s
 *                               (rpm_nlp2op_control's); splined through the N + 1 knots like a state column, evaluated at the
 *                               target's N' points; lambda'[g0' + s N' + j] = -w'_j c(tau'_j)
 *   path rows of constraint j:  p_k = (1 / w_k) lambda[g0 + N nx + j N + k]; the value at tau = 1 by the spline of a control;
 *                               lambda'[g0' + N' nx + j N' + q] = w'_q p(tau'_q)
 *   event rows of the phase, linkage and linear rows after the last phase: copied.
 * The spline, its recurrences and its evaluation are the solution carry's own code (one kernel, columns with a transform before
 * and after).  Bound multipliers are not carried: on a new mesh rpm_ipm_solve_warm with z_L = z_U = NULL forms them from mu_init.
 * Engine matching, argument errors (lambda_from / lambda_to take the place of x_from / x_to in the overlap test; NULL x_from,
 * lambda_from or lambda_to: RPM_E_INVALID), LDS limits, the column split, option "carry_tile", nonfinite, "nothing allocated
 * after the first call on a pair of engines" and graph capture: as rpm_carry_solution_batch[_dev]. */
int rpm_carry_multipliers_batch_dev(rpm_engine* from, rpm_engine* to, const double* d_x_from, const double* d_lambda_from,
                                    double* d_lambda_to, int* d_nonfinite, void* stream);
int rpm_carry_multipliers_batch(rpm_engine* from, rpm_engine* to, const double* x_from, const double* lambda_from, double* lambda_to,
                                int* nonfinite);
/* the row map that carry uses (host only, no device needed): phase < n_phases: rows = {first defect row, first path row, first
 * event row, one past the phase's last row}; phase == n_phases: the rows after the phases, {first, first, first, m}.  A phase
 * out of range: RPM_E_INVALID. */
int rpm_carry_multipliers_layout(rpm_engine* e, int phase, int rows[4]);

/* The receding-horizon step of a sweep: every instance's plan and duals moved on in time on the engine's own mesh.  dt:
 * n_instances x n_phases, instance-major, each phase's own advance in the problem's time unit (a single-phase MPC problem
 * passes n_instances numbers).  x / x_out, z_L, z_U and their outputs: n_instances x n; lambda / lambda_out: n_instances x m;
 * all packed and instance-major as rpm_ipm_solve_warm_dev takes and returns them.  lambda and lambda_out are given together or
 * both NULL; z_L, z_U, z_L_out, z_U_out all or none.
 * Per instance and phase, time[0], time[N] and the knots tau_g are the carry's, from x's t0 and tf.  With tp[q] the phase's own
 * LGR points a value is taken at s_q = tp[q] + 2 dt / (time[N] - time[0]) (state columns and the z of states also at
 * 1.0 + 2 dt / (time[N] - time[0])), clamped into [-1, 1]: a dt past the end of the horizon holds the end value, a negative dt
 * moves back and holds the first value.  A NaN passes through the clamp.
 *   x:       every state and control column is the carry's natural cubic spline through its N + 1 knots (a control's knot at 1
 *            by the spline of a control), evaluated at s_q; t0 = time[0] and tf = time[N] as the carry writes them and the
 *            static parameters are copied: the window keeps its place, the caller's time is relative to the step.
 *   lambda:  defect rows as costates and path rows divided by the weights, with rpm_carry_multipliers_batch's transforms before
 *            and after, evaluated at s_q: lambda'[defect] = -w_q c(s_q), lambda'[path] = w_q p(s_q); event rows and the rows
 *            after the last phase are copied.
 *   z_L, z_U: x's layout column by column, the same knots and point search, but piecewise linear, A y[kl-1] + B y[kr-1] held
 *            between the two knot values against the last ulp of rounding (a control column's knot at 1 holds its last node's
 *            value): non-negative multipliers stay non-negative and inside their column's range, where a spline would not
 *            keep them so.  The entries at t0, tf and the parameters are copied.
 * With dt == 0 the shift of x and of lambda is rpm_carry_solution_batch(e, e, ...) and rpm_carry_multipliers_batch(e, e, ...)
 * bit for bit: one kernel, one copy of the knots, the recurrences, the search and the transforms.
 * nonfinite: n_instances ints or NULL, 1 when any array produced for the instance holds a NaN or Inf; an instance with NaN or
 * Inf anywhere, with tf == t0 or with a NaN dt spoils itself only.
 * Argument errors are decided on the host before anything is queued, the message is rpm_last_error(e): NULL dt, x or x_out,
 * half a pair, an output overlapping any input or another output (the caller ping-pongs two sets of buffers): RPM_E_INVALID;
 * an interval-sharded engine, a column that does not fit one workgroup's LDS: RPM_E_UNSUPPORTED; no device: RPM_E_DEVICE.
 * The _dev form queues one launch per array given, plus one for the verdicts, on `stream`.  After the first call on an engine it
 * allocates nothing, copies nothing and never synchronises: it can follow rpm_ipm_solve_warm_dev and
 * rpm_ipm_get_bound_multipliers_dev on the caller's stream and be captured into a graph.  The host-pointer form stages its
 * arrays and blocks.  The calling thread's current device is restored.  Option "carry_tile" applies; every value gives the
 * same bits. */
int rpm_shift_plan_batch_dev(rpm_engine* e, const double* d_dt, const double* d_x, double* d_x_out, const double* d_lambda,
                             double* d_lambda_out, const double* d_z_L, const double* d_z_U, double* d_z_L_out, double* d_z_U_out,
                             int* d_nonfinite, void* stream);
int rpm_shift_plan_batch(rpm_engine* e, const double* dt, const double* x, double* x_out, const double* lambda, double* lambda_out,
                         const double* z_L, const double* z_U, double* z_L_out, double* z_U_out, int* nonfinite);

/* "The plan at time t" of a sweep: one phase's state and control columns of every instance evaluated at caller-given times.
 * x: n_instances x n as the solver returns it; times: n_instances x n_times, instance-major, in the problem's time unit;
 * out: n_instances x (nx + nu) x n_times, per instance column-major with n_times rows, the nx states first, then the nu
 * controls (the shape of rpm_nlp2op_control's arrays).
 * Per instance time[0], time[N] and the knots are the carry's, from x's t0 and tf.  The coordinate of a time t is
 *   s = 2 (t - time[0]) / (time[N] - time[0]) - 1,   time[0] = post_time(t0, tf, tau_0), time[N] = post_time(t0, tf, 1),
 * the very expression that forms the knots, so t = time[k] gives knot k to the bit; s is clamped into [-1, 1] with comparisons
 * a NaN passes through: outside the horizon the end values are held.  A state column is the carry's natural cubic spline through
 * its N + 1 knots, a control column that spline with its knot at 1 by the spline of a control; both are evaluated at s by the
 * code the carry and the shift evaluate with.  At t = time[k], k < N, the node values of x come back to the bit; at time[N] a
 * state's end value and the control-at-tau=1 row of rpm_nlp2op_batch.
 * nonfinite: n_instances ints or NULL, 1 when any sample of the instance is NaN or Inf; an instance with NaN or Inf in its columns,
 * its t0 / tf or its times, or with tf == t0, spoils itself only.
 * Argument errors are decided on the host before anything is queued, the message is rpm_last_error(e): NULL x, times or out,
 * n_times < 1, a phase out of range, out overlapping x or times: RPM_E_INVALID; an interval-sharded engine, a column that does
 * not fit one workgroup's LDS: RPM_E_UNSUPPORTED; no device: RPM_E_DEVICE.
 * The _dev form queues one launch (two with d_nonfinite) on `stream`.  After the first call on an engine it allocates nothing,
 * copies nothing and never synchronises, whatever n_times is, and can be captured into a graph.  The host-pointer form stages its
 * arrays and blocks.  The calling thread's current device is restored.  Options "carry_tile" and "carry_lds_bytes" apply (the
 * columns are dealt over workgroups by the carry's planner); every value gives the same bits. */
int rpm_sample_plan_batch_dev(rpm_engine* e, int phase, const double* d_x, int n_times, const double* d_times,
                              double* d_out, int* d_nonfinite, void* stream);
int rpm_sample_plan_batch(rpm_engine* e, int phase, const double* x, int n_times, const double* times, double* out, int* nonfinite);

/* The plant of a sweep's closed loop: instance b integrates its own dynamics under its plan's control,
 *   y' = f(t, y, u(t), p_b; consts_b),
 * f the functor's dae() (path outputs ignored), p_b the plan's own static parameters, consts_b the instance's constants
 * (rpm_set_instance_constants), over dt[b] from t_start[b] in n_steps classical Runge-Kutta steps of h = dt[b] / n_steps.
 * x: n_instances x n, the plans; t_start: n_instances, or NULL = the phase's time[0]; dt: n_instances (0 returns the start state,
 * a negative dt integrates backwards); state0: n_instances x nx, or NULL = the plan's own first state values; state_out:
 * n_instances x nx, and it may be the very pointer state0 (a state updated in place); traj: NULL, or n_instances x (n_steps + 1)
 * x nx, instance-major, row i the state after i steps (row 0 the start state).
 * Per step, with t_i = t_start + i h:
 *   k1 = f(t_i, y, u(t_i)), k2 = f(t_i + h / 2, y + (h / 2) k1, u(t_i + h / 2)), k3 = f(t_i + h / 2, y + (h / 2) k2, u(t_i + h / 2)),
 *   k4 = f(t_i + h, y + h k3, u(t_i + h));  acc = k1; acc = acc + 2 k2; acc = acc + 2 k3; acc = acc + k4;  y = y + (h / 6) acc.
 * hold == 0: u(t) is the sampling rule of rpm_sample_plan_batch for the control columns at each stage time, so the control the
 * plant sees is the control the shift and the extraction see; hold == 1: u is that rule at t_start for the whole call, the
 * zero-order hold a digital controller applies.  Past either end of the horizon the end value is held.  Controls are NOT clipped
 * to their bounds: the spline of a plan at its bounds can overshoot them between nodes, and the plant receives what the plan says.
 * One phase per call; events and phase boundaries are the caller's.
 * nonfinite: n_instances ints or NULL, 1 when the start state or the state after any step is NaN or Inf; an instance with a NaN
 * dt, t_start, state or control node, or with tf == t0, spoils itself only.
 * Argument errors are decided on the host before anything is queued, the message is rpm_last_error(e): NULL x, dt or state_out,
 * n_steps outside 1 ... 65536, hold not 0 or 1, a phase out of range, an output overlapping an input or the other output
 * (state_out == state0 excepted): RPM_E_INVALID; an interval-sharded engine, the nu control columns of the phase not fitting one
 * workgroup's LDS even at one instance per workgroup (the integrating lane needs all of them): RPM_E_UNSUPPORTED; no device:
 * RPM_E_DEVICE.
 * The _dev form queues one launch on `stream`; it allocates nothing, copies nothing and never synchronises, so it can follow
 * rpm_ipm_solve_warm_dev and feed rpm_ipm_set_initial_states_dev on the caller's stream and be captured into a graph.  The
 * host-pointer form stages its arrays and blocks.  The calling thread's current device is restored.  Option "rollout_tile"
 * (0 = automatic, 1, 2, 4, 8): instances per workgroup; every value gives the same bits.  "carry_lds_bytes" lowers the LDS a
 * workgroup may use here too.  User-problem libraries carry the kernel for their functor. */
int rpm_rollout_batch_dev(rpm_engine* e, int phase, const double* d_x, const double* d_t_start, const double* d_dt,
                          int n_steps, int hold, const double* d_state0, double* d_state_out, double* d_traj,
                          int* d_nonfinite, void* stream);
int rpm_rollout_batch(rpm_engine* e, int phase, const double* x, const double* t_start, const double* dt, int n_steps, int hold,
                      const double* state0, double* state_out, double* traj, int* nonfinite);

/* Solution extraction for a whole sweep: Nlp2OpConverter::Nlp2OpControl, Core/Nlp2OPConverter.cpp:13-196, for all phases and all
 * n_instances instances of the engine at once, every instance with its own constants (rpm_set_instance_constants) and static
 * parameters.  x: n_instances x n, lambda: n_instances x m, both packed and instance-major as rpm_ipm_solve[_dev] returns them.
 * out: n_instances x EB, instance-major; one instance's block holds the phases one after the other, each phase in this order
 * time (M), state (M nx), control (M nu), costate (M nx), pathmult (M nc), hamiltonian (M), mayer_cost (1), lagrange_cost (1),
 * M = N + 1, every array column-major with M rows: exactly the arrays rpm_nlp2op_control returns, and per instance the same
 * bits (the arithmetic is that call's, operation by operation and sum by sum in the same order).  The path multipliers read
 * lambda without the phase offset, as the reference does (:88), from the base of the instance's own block.
 * rpm_nlp2op_batch_layout (host only, no device needed): the offsets of a phase's eight fields inside an instance's block, in
 * the order above, and EB; either output may be NULL.  A phase out of range: RPM_E_INVALID.
 * nonfinite: n_instances ints or NULL, 1 when the instance's block holds a NaN or Inf; an instance with NaN / Inf in x or lambda,
 * or with tf == t0 where a field divides by tf - t0, spoils its own block only.
 * Argument errors are decided on the host before anything is queued: NULL x, lambda or out: RPM_E_INVALID; an interval-sharded
 * engine, a spline column that does not fit one workgroup's LDS: RPM_E_UNSUPPORTED, with a message; no device: RPM_E_DEVICE.
 * The _dev form takes device arrays and queues one launch (two with d_nonfinite; one more when the spline columns of a phase do
 * not fit one workgroup's LDS and are dealt over several) on `stream` (a hipStream_t, NULL = the legacy default stream).  The
 * first call on an engine may upload a small launch plan and allocate a workspace; every later call allocates nothing, copies
 * nothing and never synchronises, so it can follow rpm_ipm_solve_dev on the caller's stream and be captured into a graph.  The
 * host-pointer form stages its arrays like the other batched host-pointer calls and blocks.  The calling thread's current device
 * is restored.  Option "extract_tile" (0 = automatic, 1, 2, 4, 8): instances per workgroup; every value gives the same bits. */
int rpm_nlp2op_batch_layout(rpm_engine* e, int phase, long long field_offset[8], long long* block_doubles);
int rpm_nlp2op_batch_dev(rpm_engine* e, const double* d_x, const double* d_lambda, double* d_out, int* d_nonfinite, void* stream);
int rpm_nlp2op_batch(rpm_engine* e, const double* x, const double* lambda, double* out, int* nonfinite);

/* hp-Liu refinement: LiuHpMeshRefineAlg::RefineMesh, Core/LpLiuHpMeshRefineAlg.cpp:12-260 (with Reducing_N :438-481,
 * Increasing_N :379-436, Dividing_mesh :321-377, CanWeIncreaseN :606-681; Merging_mesh's verdict is unused by the
 * reference, equal-N satisfied neighbours always merge).  The object keeps the reference's histories (meshes with their
 * per-interval errors, previous solution, previous mesh points) across meshes: create it once per problem
 * (tol = desired-relative-error, nmax = Nmax, ratio_r = R, Core/LpMeshRefiner.h:54-61), call rpm_hpliu_refine after every
 * solve with the engine built on the mesh the previous call returned.  Outputs for all phases: phase p's new mesh
 * points at new_mesh_points[mesh_off[p] .. + new_n_intervals[p]], node counts at new_nodes_per_interval[nodes_off[p]
 * ..]; `capacity` entries each.  rel_err: NULL = estimate on the device (rpm_solution_error), else the caller's matrices
 * phase after phase (host only).  Fails with RPM_E_INVALID + message where the reference would throw or hit an
 * undefined cast (see csrc/rpm_hpliu.cpp). */
typedef struct rpm_hpliu rpm_hpliu;
int rpm_hpliu_create(int n_phases, double tol, int nmax, double ratio_r, rpm_hpliu** out);
void rpm_hpliu_destroy(rpm_hpliu* h);
const char* rpm_hpliu_last_error(const rpm_hpliu* h);
int rpm_hpliu_refine(rpm_hpliu* h, rpm_engine* e, const double* x, const double* rel_err, int capacity,
                     double* new_mesh_points, int* new_nodes_per_interval, int* mesh_off, int* nodes_off,
                     int* new_n_intervals, int* no_more_refine);

/* ---- row f-2: the NLP solve itself, batched and device-resident ---------------------------------------------------
 * The reference hands the TNLP to Ipopt 3.12.3 (NLPSolver::SolveNlp, Core/LpNLPSolver.cpp:13-53: "tol" from the
 * Ipopt-tol option, hessian_approximation from the option list; Ipopt is a third-party dependency that is not in the
 * reference tree).  rpm_ipm restates Ipopt's published algorithm (Waechter & Biegler 2006: primal-dual barrier,
 * fraction-to-the-boundary rule, filter line search with second-order correction, inertia correction, l1 restoration
 * phase, monotone or adaptive barrier update; no NLP scaling, no watchdog, no quality-function oracle) for the engine's
 * n_instances independent NLPs at once — the MPC sweep — with iterates, multipliers, the KKT matrices and their LDL^T
 * factors resident in HBM; per iteration only a few counters cross PCIe.  The engine's hessian_approximation decides what
 * stands for the Hessian of the Lagrangian: RPM_HESSIAN_EXACT = lpopc's finite-difference Hessian (rpm_eval_h);
 * RPM_HESSIAN_LIMITED_MEMORY — lpopc's default, Core/LpNLPWrapper.hpp:71 — = Ipopt's limited-memory BFGS (history 6, scaling
 * s'y / s's, its skipping rule; csrc/rpm_ipm_lbfgs.hip): the KKT matrix of a diagonal Hessian is factored and the low-rank
 * part enters every solve through the Sherman-Morrison-Woodbury formula (12 more substitutions per iteration).  Problems with
 * static parameters (nq > 0) have the limited-memory mode and RPM_HESSIAN_EXACT_PARAMETERS (the parameters sit in the border of
 * the KKT layouts); plain RPM_HESSIAN_EXACT refuses them.  Set the engine's "instance_align" before rpm_ipm_create.
 *   rpm_ipm_set_option: "tol" (1e-8), "max_iter" (3000), "mu_init" (0.1), "bound_push", "bound_frac" (1e-2),
 *                       "delta_c" (1e-9, constraint regularisation that makes the pivot-free LDL^T well defined; keep it
 *                       well below bound_relax_factor),
 *                       "max_line_search" (40), "trace" (0; keep the first N accepted steps of every instance),
 *                       "restoration" (1), "restoration_max_iter" (300), "restoration_penalty" (1000, Ipopt's rho),
 *                       "acceptable_tol" (1e-6), "acceptable_iter" (15), "bound_relax_factor" (1e-8, as Ipopt: finite bounds
 *                       of free unknowns move out by this * max(1, |bound|), so a solution may sit that far outside them),
 *                       "max_soc" (4, second-order correction steps per iteration; 0 = off),
 *                       "mu_strategy" (1, default: adaptive = what lpopc asks Ipopt for, Core/LpNLPSolver.cpp:28, with the
 *                       LOQO oracle and the kkt-error globalisation; 0: the monotone Fiacco-McCormick rule,
 *                       three batched iterations fewer on the quadrotor sweep),
 *                       "sigma_cap" (0 = off; experimental clamp on z/s in the KKT matrix),
 *                       "init_ls_multipliers" (0; 1 = least-squares multipliers at the first iterate, Ipopt's default start),
 *                       "level1_dense" (1 where it applies: the interval blocks of the nested dissection are factored out of
 *                       registers, kkt_factor_dense_kernel, when each has at most 21 block rows of 16 (17 resident, the first
 *                       4 block columns through the storage); 0 = the left-looking kernel; 1 on a layout it does not fit:
 *                       RPM_E_UNSUPPORTED),
 *                       "upper_dense" (1 where it applies: the last level of the nested dissection — and the groups of
 *                       separators of a three-level layout when their band is at least half as wide as long — on that kernel
 *                       too, the last level with its border x border corner eliminated there as well (panels of the corner's
 *                       block columns by substitution); 2 = the corner by the left-looking kernel's unblocked elimination
 *                       (bit for bit what 0 gives); 0 = the left-looking kernel for them; results agree to rounding),
 *                       "fused_fill" (1 where level1_dense runs: that kernel assembles its interval block from the Jacobian,
 *                       Hessian and diagonal terms itself and carries the level-1 forward substitution of the iteration's
 *                       right-hand side along, the fill kernel leaves level-1 storage alone; 0 = separate kernels; same
 *                       results bit for bit; 1 where level 1 does not run on that kernel: RPM_E_UNSUPPORTED),
 *                       "nlp_scaling" (0; 1 = Ipopt's gradient-based NLP scaling, ITS default: objective and constraint rows
 *                       scaled so that no gradient entry at the starting point exceeds "nlp_scaling_max_gradient" (100); the
 *                       multipliers and the objective come back unscaled; DESIGN.md f-2 on why it is off here),
 *                       "ic_hot_start" (0; 1 = an iteration whose predecessor needed delta_w > 0 starts the inertia correction
 *                       at kappa_w^- * delta_w_last instead of 0 while that is >= "ic_hot_min" (1e-10): not Ipopt's rule, an
 *                       experiment),
 *                       the warm start's (rpm_ipm_solve_warm), with Ipopt's names and defaults: "warm_start_bound_push",
 *                       "warm_start_bound_frac", "warm_start_slack_bound_push", "warm_start_slack_bound_frac",
 *                       "warm_start_mult_bound_push" (1e-3 each), "warm_start_mult_init_max" (1e6)
 *   rpm_ipm_set_bounds: variable bounds of one instance (default: the engine's); the fixed/free pattern is shared
 *   rpm_ipm_solve[_dev]: x (n_instances x n, in: starting points, out: solutions; host resp. device pointer),
 *                       lambda (n_instances x m, may be NULL); per instance on the host, any may be NULL: objective,
 *                       status (0 converged, 1 converged to Ipopt's acceptable level, 2 iteration limit, 3 line search failed where Ipopt would enter
 *                       restoration, 4 inertia correction failed, 5 NaN/Inf), iteration count, scaled KKT error; a NaN or Inf in an
 *                       instance's starting point ends that instance with status 5 before its first pass and touches no other
 *   rpm_ipm_get_info:   order of the KKT system, of its banded part, half bandwidth, border size, doubles of storage per
 *                       instance, number of slack variables (one per inequality row) */
typedef struct rpm_ipm rpm_ipm;
int rpm_ipm_create(rpm_engine* e, rpm_ipm** out);
void rpm_ipm_destroy(rpm_ipm* s);
const char* rpm_ipm_last_error(const rpm_ipm* s);
int rpm_ipm_set_option(rpm_ipm* s, const char* key, double value);
int rpm_ipm_set_bounds(rpm_ipm* s, int instance, const double* x_l, const double* x_u);
int rpm_ipm_set_all_bounds(rpm_ipm* s, const double* x_l, const double* x_u);   /* n_instances x n each */
/* The measured initial states of a receding-horizon sweep: state0 is n_instances x nx of `phase`; both calls write
 * lower = upper = state0[b][j] at variable x_state0 + j (N + 1) of every instance and leave every other bound alone, so the
 * next solve is bit for bit the solve after rpm_ipm_set_all_bounds with the same numbers.  Every one of the phase's nx initial
 * states must be fixed in the solver's plan (the KKT layout is shared by all instances), else RPM_E_INVALID naming the first
 * free one; a phase out of range or a NULL array: RPM_E_INVALID; all decided on the host.  The _dev form takes a device array
 * and is one small launch on `stream`: no copy, no synchronisation, capturable into a graph; rpm_ipm_solve[_warm]_dev on the
 * same stream reads what it wrote.  A NaN or Inf measured state ends that instance's next solve with status 5 and disturbs no
 * other instance. */
int rpm_ipm_set_initial_states_dev(rpm_ipm* s, int phase, const double* d_state0, void* stream);
int rpm_ipm_set_initial_states(rpm_ipm* s, int phase, const double* state0);
int rpm_ipm_get_info(rpm_ipm* s, int* kkt_order, int* band_order, int* half_bandwidth, int* border,
                     long long* storage_doubles, int* n_slacks);
int rpm_ipm_get_stats(rpm_ipm* s, int* iterations, int* factorizations, int* trial_points);
/* the factorisation's sub-problems: 5 ints each (order, banded part, border, half bandwidth, doubles per stored column); one
 * entry for the band + border layout, the interval blocks followed by the separator system with nested dissection */
int rpm_ipm_get_subproblems(rpm_ipm* s, int capacity, int* geom, int* n_sub);
/* records of the last solve when option "trace" > 0: 8 doubles per accepted step — f, theta = |c|_1, mu, alpha, alpha_z,
 * delta_w, E_0 at the step's start, backtracking steps */
int rpm_ipm_get_trace(rpm_ipm* s, int instance, int capacity, double* records, int* n_records);
/* restoration phases each instance went through in the last solve (option "restoration", default 1: when the line search
 * gives up at an infeasible point the instance switches, as Ipopt does, to  min rho |p + n|_1 + zeta/2 |D_R (v - v_R)|^2
 * s.t. c(v) - p + n = 0, p, n >= 0 and the bounds  — solved by the same interior-point kernels with p, n eliminated from the
 * Newton system — until the infeasibility is 0.9 of where it entered and the original filter accepts the point; least-squares
 * multipliers on return.  Trace records of restoration iterations carry -1 in the backtracking field.  DESIGN.md f-2) */
int rpm_ipm_get_restorations(rpm_ipm* s, int* per_instance);
/* device time of the last solve spent in the factorisation and in the substitution kernels (HIP events on the solver's
 * stream, summed over its iterations), for roofline figures */
int rpm_ipm_get_kernel_times(rpm_ipm* s, double* factor_ms, double* substitution_ms);
int rpm_ipm_solve(rpm_ipm* s, double* x, double* lambda, double* obj, int* status, int* iterations, double* kkt_error);
/* Ordering contract of the device-resident form: the interior-point loop runs on the engine's private stream.  Before its
 * first read of d_x (and first write of d_lambda) it waits for everything the caller has queued on `stream` (a hipStream_t,
 * NULL = the legacy default stream) up to this call; it returns only after its own stream has drained, so on return the
 * results in d_x / d_lambda are complete for the host and for work queued later on any stream. */
int rpm_ipm_solve_dev(rpm_ipm* s, double* d_x, double* d_lambda, double* obj, int* status, int* iterations,
                      double* kkt_error, void* stream);
/* Warm start in the primal and the dual (Ipopt's warm_start_init_point; not its warm_start_target_mu / _entire_iterate).  x
 * (n_instances x n), lambda (n_instances x m, required) and z_L / z_U (n_instances x n: the multipliers of the variables' lower /
 * upper bounds; both given or both NULL) are in/out, instance-major, values of the caller's unscaled problem.  Everything not
 * named here is as in rpm_ipm_solve: bound relaxation, the fixed / free pattern, fresh instance records, an emptied
 * limited-memory store, mu = mu_init; "init_ls_multipliers" is ignored.  Per instance:
 *   x        pushed inside its relaxed bounds by warm_start_bound_push / _bound_frac (in place of bound_push / bound_frac); fixed
 *            variables sit at their bound
 *   slacks   g(x) pushed inside the relaxed row bounds by warm_start_slack_bound_push / _slack_bound_frac
 *   lambda   clipped to +-warm_start_mult_init_max
 *   z        max(z, warm_start_mult_bound_push) where the bound exists and the variable is free, else 0.  z_L = z_U = NULL:
 *            mu_init / (x - l), mu_init / (u - x) at the pushed x and the relaxed bounds (the start on a new mesh, where no bound
 *            multipliers exist), and none are returned
 *   slack z  from the slack's stationarity -lambda_r - zL + zU = 0: zL = max(-lambda_r, warm_start_mult_bound_push) where the
 *            row has a lower bound, zU = max(lambda_r, ...) where it has an upper one
 *   nlp_scaling = 1: the clipped / floored values go into the scaled problem, lambda~ = (lambda sf) / sc, z~ = z sf (the inverse
 *            of what the solve returns), the slack multipliers from lambda~
 *   a NaN or Inf in an instance's x, lambda or z ends that instance with status 5 and touches no other.
 * rpm_ipm_get_bound_multipliers[_dev]: z_L, z_U (n_instances x n) after the last solve of either kind, unscaled, 0 where there is
 * no bound or the variable is fixed; what rpm_ipm_solve_warm returns in z_L / z_U, bit for bit.  Before any solve: RPM_E_INVALID.
 * The _dev form queues one launch on `stream`.  Ordering contract of rpm_ipm_solve_warm_dev: that of rpm_ipm_solve_dev, for all
 * four arrays.  NULL lambda, exactly one NULL z: RPM_E_INVALID with a message. */
int rpm_ipm_solve_warm(rpm_ipm* s, double* x, double* lambda, double* z_L, double* z_U, double* obj, int* status, int* iterations,
                       double* kkt_error);
int rpm_ipm_solve_warm_dev(rpm_ipm* s, double* d_x, double* d_lambda, double* d_z_L, double* d_z_U, double* obj, int* status,
                           int* iterations, double* kkt_error, void* stream);
int rpm_ipm_get_bound_multipliers(rpm_ipm* s, double* z_L, double* z_U);
int rpm_ipm_get_bound_multipliers_dev(rpm_ipm* s, double* d_z_L, double* d_z_U, void* stream);
/* Solution sensitivities to variables that are FIXED in the solver's plan (x_l == x_u; the pattern is shared by all instances):
 * the measured initial states of a receding-horizon sweep, t0, tf.  Call v = (x, slacks), lambda, z_L, z_U and the relaxed bounds
 * "the state": what the solver holds after a finished solve of either kind, or directly after rpm_ipm_debug_start /
 * rpm_ipm_debug_pass.  Column k (k < n_par, 1 <= n_par <= 32, j = var_index[k]) solves the solver's own reduced system (13),
 *   [ W + Sigma + delta_w I   A' ] [dv]     [ W[free, j] ]
 *   [ A                 -delta_c I ] [dl] = - [ A[:, j]    ]
 * with W the exact Hessian of the Lagrangian at (x, lambda), A the constraint Jacobian (-1 at every slack), Sigma = z_L / (v - v_l)
 * + z_U / (v_u - v) on the free unknowns: the matrix of an iteration, assembled and factored by the same launchers.  delta_w starts
 * at 0 and follows the iteration's inertia correction; where it ends is reported.  The right-hand side, in unknown order: free
 * variable i -(h_1 + h_2 + ...) over the Hessian triplets at {i, j} in ascending triplet index, one addition after the other;
 * constraint row r -(the Jacobian triplets at (r, j), likewise; there is at most one); slacks and fixed unknowns 0.  Results,
 * instance-major: dx (n_instances x n_par x n) = dv on the free variables, 1 at variable j, 0 at every other fixed variable;
 * dlambda (n_instances x n_par x m, or NULL) = dl.  Sigma is taken at the barrier parameter the state ended at, so these are the
 * sensitivities of the barrier problem, and W is as good as the engine's finite-difference-tol makes it.
 *   delta_w (host, n_instances, or NULL)  the regularisation the factorisation ended at (NaN where info is 2)
 *   info    (host, n_instances, or NULL)  0 computed with delta_w = 0; 1 computed with delta_w > 0 (the matrix was regularised: not
 *           a strict local minimum at this mu); 2 left out — the instance's state is non-finite (device status 5) or the
 *           factorisation gave up —, its blocks are NaN and no other instance is touched
 * Ordering contract of the _dev form: that of rpm_ipm_solve_dev (runs on the engine's private stream after what the caller queued
 * on `stream`, returns when drained); var_index, delta_w and info are host arrays.  It reads host counters for the inertia
 * correction, so it is not capturable into a graph.  The work space (n_instances x n_par x right-hand-side length doubles) is
 * allocated on first use, kept, and grows only for a larger n_par.  The iterate, the multipliers, the instance records,
 * rpm_ipm_get_bound_multipliers and the statistics of the last solve are what they were before the call: a following
 * rpm_ipm_solve[_warm] is bit for bit what it is without the call in between.  The calling thread's current device is restored.
 * Solver option "sens_refine" (-1 = automatic, the default: 2 rounds on an engine created with RPM_HESSIAN_EXACT_PARAMETERS whose
 * phases have static parameters, none on every other engine; 0 = none; 1 .. 8 = that many rounds of iterative refinement of every column, sol += K^-1 (rhs - K sol) with
 * the same factors and the residual formed from the matrix's sources — the Hessian and Jacobian triplets, the slacks' -1, the
 * diagonal terms — in a fixed order, so the result is deterministic; the work space triples).  A refined call factors with
 * delta_w starting at 1e-8 instead of 0 (the pivot-free LDL^T is stable on a quasi-definite matrix) and takes the residual against
 * the matrix without it, so the rounds remove what it adds; info is 1 only when the inertia correction went beyond that floor, and
 * delta_w reports where the factorisation ended (1e-8 at info 0).  Where W + Sigma is nearly singular at delta_w = 0 (a bang-bang
 * plan with a fixed static parameter: no curvature in the states, their bounds inactive) the plain columns keep about three digits;
 * two rounds agree with a dense solve to 4e-11 — hence the automatic rounds exactly where sensitivities to a
 * fixed static parameter can be asked for.  Without rounds every bit is what it was.
 * Refusals, all decided on the host before anything is queued — RPM_E_INVALID with a message: NULL var_index or dx, n_par outside
 * 1 .. 32, an index out of range, a duplicate, a free variable (named), no state to take them at; RPM_E_UNSUPPORTED:
 * hessian-approximation = limited-memory (a quasi-Newton W gives no sensitivities), nlp_scaling = 1.
 * rpm_ipm_initial_state_variables (host only): the nx variables rpm_ipm_set_initial_states writes, x_state0 + j (N + 1).
 * rpm_ipm_parameter_variables (host only): the nq static parameters of the phase, x_t0 + 2 + j — with parameter_min ==
 * parameter_max they are fixed variables of the plan, and the columns above are d(plan) / d(parameter). */
int rpm_ipm_initial_state_variables(rpm_ipm* s, int phase, int* var_index /* nx */);
int rpm_ipm_parameter_variables(rpm_ipm* s, int phase, int* var_index /* nq */);
int rpm_ipm_sensitivities_dev(rpm_ipm* s, int n_par, const int* var_index, double* d_dx, double* d_dlambda, double* delta_w, int* info,
                              void* stream);
int rpm_ipm_sensitivities(rpm_ipm* s, int n_par, const int* var_index, double* dx, double* dlambda, double* delta_w, int* info);
/* The predictor (the tangential step of advanced-step NMPC): x_out[b] = x[b], then for k ascending x_out[b] = x_out[b] +
 * dx[b][k] * delta[b][k] — product, then sum —, delta n_instances x n_par (the move of every listed variable); lambda likewise
 * when dlambda, lambda and lambda_out are all given.  Nothing is clipped to the bounds: the pushes of the warm start that follows
 * deal with them.  The _dev form is one launch on `stream`: it allocates nothing, copies nothing and never synchronises
 * (capturable); the host form goes through a device block of the solver's, blocking.  An output that overlaps an input or the other
 * output, a NULL dx / delta / x / x_out, a bad list (as above): RPM_E_INVALID with a message. */
int rpm_ipm_apply_sensitivities_dev(rpm_ipm* s, int n_par, const int* var_index, const double* d_dx, const double* d_dlambda,
                                    const double* d_delta, const double* d_x, double* d_x_out, const double* d_lambda,
                                    double* d_lambda_out, void* stream);
int rpm_ipm_apply_sensitivities(rpm_ipm* s, int n_par, const int* var_index, const double* dx, const double* dlambda, const double* delta,
                                const double* x, double* x_out, const double* lambda, double* lambda_out);
/* test hook (host pointers, synchronous): the evaluation and the right-hand-side gather of rpm_ipm_sensitivities only; rhs:
 * n_instances x n_par x kkt_order in unknown order (variables, slacks, multipliers).  Same refusals. */
int rpm_ipm_debug_sensitivity_rhs(rpm_ipm* s, int n_par, const int* var_index, double* rhs);
/* Solution sensitivities to the instances' CONSTANTS (rpm_set_instance_constants; the shared constants where it was never used):
 * a moved set-point, a mass, a weight.  The state, the matrix, its inertia correction, "sens_refine", info, delta_w, the ordering
 * contract of the _dev form and everything that is left undisturbed are those of rpm_ipm_sensitivities; only the right-hand side
 * and the unpacking differ.  Column k (k < n_par, 1 <= n_par <= 32, j = const_index[k] in 0 .. nconst - 1, no duplicate) of
 * instance b: with c the instance's constants, h = rho (1 + |c_j|), rho the solver option "sens_constant_step" (default 1e-5,
 * refused outside (0, 0.1]) and c+ / c- = c with entry j replaced by c_j + h / c_j - h, the objective gradient, g and the Jacobian
 * values are evaluated at the held x at c+ and at c- by the engine's own batched launchers — the bits of a one-instance engine with
 * those constants set.  The right-hand side, in unknown order: free variable i starts with acc = grad+[i] - grad-[i], then for the
 * Jacobian triplets t of column i inside the state-dependent block, in ascending triplet index, acc = acc + (J+[t] - J-[t]) *
 * lambda[row(t)] — product, then sum —, and the entry is -(acc / (h + h)); constraint row r -((g+[r] - g-[r]) / (h + h)); slacks and
 * fixed variables 0.  Results: dx (n_instances x n_par x n) = dv on the free variables, 0 on every fixed one; dlambda (n_instances x
 * n_par x m, or NULL) = dl; an instance that is left out gets NaN blocks.  The evaluation the matrix is assembled from comes after
 * the perturbed ones.  The perturbed evaluations read a scratch copy of the constants: the engine's own constants — the values, the
 * pointer the kernels read and its stride — are untouched on every exit path.  Cost: 2 n_par evaluations of grad f, g and the
 * Jacobian on top of rpm_ipm_sensitivities' call; the scratch of one constant (two Jacobians, two gradient / g blocks) is allocated
 * on first use, kept, grows only and serves every constant in turn.  These are barrier sensitivities at finite-difference accuracy
 * and do not see a change of the active set.
 * Refusals, all decided on the host before anything is queued — RPM_E_INVALID with a message: a functor without constants, NULL
 * const_index or dx, n_par outside 1 .. 32, an index out of range, a duplicate, no state to take them at; RPM_E_UNSUPPORTED:
 * hessian-approximation = limited-memory, nlp_scaling = 1.
 * rpm_ipm_apply_constant_sensitivities[_dev]: the predictor above with delta (n_instances x n_par) the moves of the listed
 * constants; the same launch, the same contract (the _dev form is one launch, capturable, allocates nothing), the list checked as
 * a list of constants.
 * rpm_ipm_debug_constant_sensitivity_rhs (test hook, host pointers, synchronous): the perturbed evaluations and the gather only;
 * rhs: n_instances x n_par x kkt_order in unknown order.  Same refusals. */
int rpm_ipm_constant_sensitivities_dev(rpm_ipm* s, int n_par, const int* const_index, double* d_dx, double* d_dlambda, double* delta_w,
                                       int* info, void* stream);
int rpm_ipm_constant_sensitivities(rpm_ipm* s, int n_par, const int* const_index, double* dx, double* dlambda, double* delta_w, int* info);
int rpm_ipm_apply_constant_sensitivities_dev(rpm_ipm* s, int n_par, const int* const_index, const double* d_dx, const double* d_dlambda,
                                             const double* d_delta, const double* d_x, double* d_x_out, const double* d_lambda,
                                             double* d_lambda_out, void* stream);
int rpm_ipm_apply_constant_sensitivities(rpm_ipm* s, int n_par, const int* const_index, const double* dx, const double* dlambda,
                                         const double* delta, const double* x, double* x_out, const double* lambda, double* lambda_out);
int rpm_ipm_debug_constant_sensitivity_rhs(rpm_ipm* s, int n_par, const int* const_index, double* rhs);
/* test hook (host pointers): exactly the launches that precede the iteration loop — warm = 0 the cold start (lambda, z_L, z_U
 * ignored), else the warm start above — then the state: v (n_instances x nv: x, then the slacks), zL, zU (n_instances x nv),
 * lambda (n_instances x m), mu and status (n_instances; status 0, or 5 after a non-finite input), all in the solver's (scaled)
 * problem; any output may be NULL.  No step is taken; the last solve's bound multipliers are gone afterwards
 * (rpm_ipm_get_bound_multipliers: RPM_E_INVALID until the next solve). */
int rpm_ipm_debug_start(rpm_ipm* s, int warm, const double* x, const double* lambda, const double* z_L, const double* z_U,
                        double* v_out, double* zL_out, double* zU_out, double* lam_out, double* mu_out, int* status_out);
/* test hook (host pointers, synchronous): the iteration loop's own next steps on the state rpm_ipm_debug_start has just made, and
 * what they wrote.  Valid only directly after rpm_ipm_debug_start on the same solver (no solve and no other debug call in between),
 * else RPM_E_INVALID with a message; a second pass needs a second start.  It launches nothing of its own: the members of the solve
 * loop (IpmLoop) and the production launchers.
 *   stage 1  evaluation of f, grad f, g, the Jacobian ((nlp_scaling) scaled), grad_x L, the residual pass: c, the scalars of the
 *            optimality error, the termination verdict, the barrier update, tau, phi; (limited-memory) the memory's first pass
 *   stage 2  stage 1, then the exact Hessian (exact mode) and the assembly of the KKT matrix and its right-hand side.  Assembly of
 *            the level-1 blocks by the factorisation kernel ("fused_fill") is off for this call, so the fill kernel writes the whole
 *            storage.  Nothing is factored.
 *   stage 3  stage 1, the Hessian, then assembly + factorisation with the inertia correction and the options as they are set,
 *            the substitution and the direction kernel: dz, the step lengths, the slope.  No trial point is evaluated.
 * As in the loop, the steps after stage 1 are skipped when no instance is left running.  Outputs, n_instances rows each, any may be
 * NULL, an array of a later stage than the one asked for is left untouched; all in the solver's (scaled) problem:
 *   after stage 1   obj (1), grad (n), g (m), jac (nnz_jac), c (m), glag (nv: grad_x L, -lambda_r at the slack of row r)
 *   after stage 2   hess (nnz_h), k_storage (storage_doubles of rpm_ipm_get_info), rhs (Nt, unknown order: variables, slacks,
 *                   multipliers); after stage 3 rhs holds the solution of the system and k_storage its factors
 *   after stage 3   dv, dzL, dzU (nv), dlam (m)
 *   always          record (RPM_IPM_RECORD_DOUBLES): the instance record, integers as doubles, in this order —
 *                   mu tau f theta lnsum dinf cinf comp_max comp_min sum_lam sum_z err0 | delta_w delta_w_last alpha_max alpha_z
 *                   alpha alpha_min dphi phi theta_max theta_min | status (the device's: 0 running, 1 converged, 6 acceptable level,
 *                   2 .. 5 as rpm_ipm_solve) iter nfilt accepted refactor npos nneg nbad ls armijo nzb pad | mode resto_it
 *                   enter_resto n_resto n_acc skip_update | th0 zeta mu_r th_r thr_max thr_min phi_r | nrfilt soc_on soc_req soc_p
 *                   use_soc n_soc | alpha_soc az_soc th_old_soc | mu_max refs[0..3] | fixed_mode nrefs n_recalc | th_trial phi_trial
 *                   (theta and phi of the last trial point the line search judged: rpm_ipm_debug_line_search)
 * The last solve's bound multipliers stay gone, as after rpm_ipm_debug_start. */
#define RPM_IPM_RECORD_DOUBLES 66
int rpm_ipm_debug_pass(rpm_ipm* s, int stage, double* obj, double* grad, double* g, double* jac, double* c, double* glag, double* hess,
                       double* k_storage, double* rhs, double* dv, double* dlam, double* dzL, double* dzU, double* record);
/* test hook (host pointers, synchronous): rounds of the filter line search on the direction rpm_ipm_debug_pass(stage 3) has just
 * left.  Valid only directly after a stage-3 pass that left at least one instance running, or directly after itself (no solve, start
 * or pass in between; the read-only rpm_ipm_debug_lbfgs_state and rpm_ipm_debug_slot may come between), else RPM_E_INVALID with a
 * message.  It launches nothing of its own: every round is IpmLoop::line_search_round, the body of the solve loop's line search —
 * where a second-order correction was asked for, its right-hand side, the substitution with the factors in place and its step
 * lengths; then every pending instance's trial point, f and g there, and the verdict of ipm_accept_kernel.  Up to `rounds` (>= 1)
 * rounds run; as in the loop they stop when no instance has a line search pending and none asks for a correction.
 *   filter, filter_count   n_instances x n_filter pairs (theta, phi) and the number of them that count per instance: they replace
 *                          every instance's filter before the first round of this call.  filter_count NULL: the filters stay as they
 *                          are.  n_filter above the filter's capacity (1024) or a count outside 0 .. n_filter: RPM_E_INVALID.
 * Outputs after the last round, n_instances rows each, any may be NULL, all in the solver's (scaled) problem.  An array holds what
 * the last round that wrote it left for the instance; an instance that was not pending keeps its earlier values:
 *   xt (n), objt (1), gt (m)   the trial point v + alpha dv (corrected step: v + alpha_soc dv2) on x, and f, g there
 *   ct (m)                     c(trial): gt - g_l (nlp_scaling: sc g_l) on a row without slack, gt - (s + alpha ds) on a row with one
 *   csoc (m)                   c_soc = alpha c + c(trial) after the first correction, alpha_soc c_soc + c(trial) after a later one
 *   dv2, dzL2, dzU2 (nv), dlam2 (m)   the corrected step, valid once a correction round has run for the instance
 *   soc_rhs, rhs (Nt, unknown order)   the right-hand side of the correction of this call's last round, written only when that
 *                              round ran one, copied before the substitution overwrites it; the solution that stands in its place
 *   record                     as rpm_ipm_debug_pass; th_trial, phi_trial are theta and phi of the trial point just judged
 *   counts (2 ints)            instances whose line search is still pending, instances that ask for a correction next */
int rpm_ipm_debug_line_search(rpm_ipm* s, int rounds, int n_filter, const double* filter, const int* filter_count, double* xt,
                              double* objt, double* gt, double* ct, double* csoc, double* dv2, double* dlam2, double* dzL2, double* dzU2,
                              double* soc_rhs, double* rhs, double* record, int* counts);
/* test hook (host pointers, synchronous): IpmLoop::update — the step, the reset (16), the filter entry (22), the trace record, or
 * the start of the restoration phase resp. of the recalc_y pass, and (limited-memory) grad_x L(x_old, lambda_new) — on what
 * rpm_ipm_debug_line_search has just left.  Valid only directly after it, else RPM_E_INVALID with a message.  Outputs, n_instances
 * rows each, any may be NULL, in the solver's (scaled) problem:
 *   v, zL, zU (nv), lambda (m)     the iterate after the update
 *   filter (n_filter pairs)        the first n_filter entries of the filter's storage; nfilt of the record says how many count
 *   vR, dr2 (nv), pp, nn, zp, zn (m)   the restoration phase's reference point, D_R^2, p, n and their multipliers: written when an
 *                                  instance enters the restoration phase (record: mode 2), stale otherwise
 *   lb_gold (n)                    limited-memory only: grad_x L(x_old, lambda_new) of the running instances
 *   record                         as rpm_ipm_debug_pass (nrfilt: the restoration filter's count)
 * The trace record of the step is read through rpm_ipm_get_trace (option "trace"). */
int rpm_ipm_debug_update(rpm_ipm* s, double* v, double* zL, double* zU, double* lambda, int n_filter, double* filter, double* vR,
                         double* dr2, double* pp, double* nn, double* zp, double* zn, double* lb_gold, double* record);
/* test hooks: KKT position of every unknown ([0,n) variables, slacks, then the m multipliers); factor + solve the
 * caller's matrices given in the band + border storage (host pointers, n_instances of each) */
int rpm_ipm_get_permutation(rpm_ipm* s, int* pos, int capacity);
int rpm_ipm_debug_solve(rpm_ipm* s, const double* k_storage, const double* rhs, double* sol, int* n_pos, int* n_neg);
/* layout-independent forms (band + border, or nested dissection: engine option "ipm_nested" = 1 before rpm_ipm_create — every
 * mesh interval is eliminated by a workgroup of its own up to the states at its first node, the Schur complements add up into
 * a block-tridiagonal separator system + border; same LDL^T without pivoting, same inertia from the signs of D): dense
 * symmetric matrices B x Nt x Nt and vectors in unknown order ([0,n) variables, slacks, multipliers); rpm_ipm_debug_slot
 * tells whether the layout can hold entry (ua, uc) */
int rpm_ipm_debug_solve_dense(rpm_ipm* s, const double* k_dense, const double* rhs, double* sol, int* n_pos, int* n_neg);
int rpm_ipm_debug_slot(rpm_ipm* s, int ua, int uc, long long* offset);
/* test hook, read-only (host pointer, synchronous): the KKT storage of every instance as it stands, n_instances x storage doubles
 * (rpm_ipm_get_info) — after rpm_ipm_debug_solve[_dense] or rpm_ipm_debug_pass(stage 3) the factors (d on the diagonal, L below it,
 * L11^-1 below the diagonal of every 16 x 16 diagonal block), after a stage-2 pass the assembled matrix.  It changes no state and,
 * like rpm_ipm_debug_slot, may come between any two calls. */
int rpm_ipm_debug_storage(rpm_ipm* s, double* k_storage);
/* test hooks of the limited-memory BFGS kernels (host pointers; RPM_E_UNSUPPORTED on a solver with the exact Hessian).  They run
 * the solver's own launchers on the caller's data:
 *   _step   one pass of the update as the solve loop runs it after the residual: x, glag_new = grad_x L(x, lambda), glag_old =
 *           grad_x L(x_previous, lambda) (n_instances x n each), mode / status per instance (NULL = 0: a regular, running
 *           instance).  reset != 0 starts a sequence: bounds and instance records as at the start of a solve, empty memory.
 *           x at fixed variables is the caller's to keep at the bound.
 *   _state  per instance: record[8] = sigma, pairs held, consecutive skips, previous iterate valid, updates, skips, and the two
 *           decision words; M (12 x 12); the pair columns S, Y (6 x n each, oldest first).  A NULL array is left out.
 *   _solve  (K0 - E M^-1 E') d = rhs with the memory as it stands: K0 as nnz lower-triangle entries (rows >= cols, unknown
 *           order, each once; one structure, values n_instances x nnz), rhs and sol n_instances x Nt in unknown order.  Every
 *           instance is made live; an entry the layout has no slot for gives RPM_E_INVALID. */
int rpm_ipm_debug_lbfgs_step(rpm_ipm* s, int reset, const double* x, const double* glag_new, const double* glag_old, const int* mode,
                             const int* status);
int rpm_ipm_debug_lbfgs_state(rpm_ipm* s, double* record, double* M, double* S, double* Y);
int rpm_ipm_debug_lbfgs_solve(rpm_ipm* s, int nnz, const int* rows, const int* cols, const double* vals, const double* rhs, double* sol);

/* ---- device-resident variants (inputs/outputs already in HBM; used by benches, by the
 *      MPC sweep and by any device-side solver).  Pointers are device pointers on the
 *      engine's device; `stream` is a hipStream_t with HIP's own meaning (NULL = the legacy
 *      default stream).  Calls are asynchronous on that stream; the host-pointer entry points
 *      above use a private stream of the engine instead. ------------------------------- */
int rpm_eval_g_dev(rpm_engine* e, const double* d_x, double* d_g, void* stream);
int rpm_eval_jac_g_dev(rpm_engine* e, const double* d_x, double* d_values, void* stream);
/* fused pair: one launch produces g and the Jacobian values of the same x */
int rpm_eval_pair_dev(rpm_engine* e, const double* d_x, double* d_g, double* d_values, void* stream);
int rpm_eval_f_dev(rpm_engine* e, const double* d_x, double* d_obj, void* stream);
int rpm_eval_grad_f_dev(rpm_engine* e, const double* d_x, double* d_grad_f, void* stream);
int rpm_eval_h_dev(rpm_engine* e, const double* d_x, double obj_factor, const double* d_lambda,
                   double* d_values, void* stream);
/* Test hook of the exact Hessian's t0/tf reduction (rpm_hess_tt_kernel alone).  The shipped functors are autonomous, so
 * rpm_eval_h only ever gives that kernel zeros to add.  tmp (HOST): n_instances x tmp_len doubles, tmp_len = 3 * (sum of
 * the phases' N); phase p starts at 3 * (nodes of the phases before it) and holds N per-node terms of the t0t0 entry,
 * then N of tftf, then N of tft0.  out (HOST): [(instance * n_phases + p) * 3 + i], i = 0 t0t0, 1 tft0, 2 tftf, read back
 * from where rpm_eval_h stores them.  An engine with static parameters (nq > 0) reduces more rows than these three and a
 * non-autonomous parameter functor exercises them through rpm_eval_h itself: RPM_E_UNSUPPORTED there.
 * rpm_debug_hess_structure (HOST only, no device): the structure build_hessian_tables gives for a caller-given dependency pattern
 * instead of the device probe's — dep: per phase (nx + nc) x (nx + nu) zeros and ones, column-major, phases concatenated; iRow / jCol
 * (capacity entries, may be NULL to ask for *nnz_h alone).  The engine is left as it was. */
int rpm_debug_hess_structure(rpm_engine* e, const int* dep, int dep_len, int capacity, int* iRow, int* jCol, int* nnz_h);
int rpm_debug_hess_tt(rpm_engine* e, const double* tmp, int tmp_len, double* out);
/* Test hook of the pipelined kernel's tile orders (host arithmetic only): the slot in [0, nh * nb) of a round of tiles that
 * half `half` of workgroup b takes in a launch of nb workgroups of nh halves under "tile_order" = order; -1: bad argument. */
int rpm_debug_tile_slot(int order, int nh, int nb, int b, int half);
/* block until everything queued on the engine's stream has finished */
int rpm_synchronize(rpm_engine* e);

/* ---- engine options ------------------------------------------------------------
 * key                values
 * "fuse_pair"        1 (default): rpm_eval_g(new_x=1) runs the fused pair kernel and the following
 *                    rpm_eval_jac_g(new_x=0) on the same x returns the cached values; 0: separate kernels
 * "dx_mode"          0: scalar ascending-column D.X (bit-identical to the reference's COO loop,
 *                    SparseMatrix/LpSparseMatrix.cpp:142-153); 1: v_mfma_f64_16x16x4 tiles
 * "tile_nodes"       16 | 32 | 64: collocation nodes per workgroup (0 = default 16)
 * "role_loop"        -1 (default): automatic, 0: never, 1: always — the throughput thread layout (64 nodes x 4 role
 *                    groups per workgroup, roles walked sequentially) chosen automatically for large grids
 * "pipeline"         -1 (default): automatic, 0: never, 1: whenever the mesh fits — with the role-looped layout, run the
 *                    persistent pipelined kernel (4 compute waves + 1 DMA wave per workgroup; inputs of the next tile
 *                    prefetched, constant block written by the DMA wave); automatic = every resident workgroup has
 *                    at least two tiles.  get-only "pipeline_active": 1 if the next launch uses it
 * "hess_tile_nodes"  get-only: nodes per workgroup of the exact-Hessian kernel (0 before the first eval_h)
 * "stage_roles"      -1 (default) | 0 | 1: in the pipelined kernel, problem functors that offer their dynamics in stages
 *                    (csrc/problems/problems.hpp `has_stage`: the launch vehicle, the quadrotor) are evaluated in full once per
 *                    node and per perturbation role only in what the perturbed variable enters — the same operations, the
 *                    same bits; -1: where the launch skips the constant block ("persistent_values"), which is bound by the
 *                    dynamics; with all stores the extra registers cost more than the arithmetic saves
 * "tile_order"       0 (default) | 1: in the pipelined kernel, which tiles of a round the workgroups of one XCD take: 0 a contiguous
 *                    eighth (one instance of the 4 x 64 x 16 launch problem), 1 a quarter of each of four eighths (one phase of
 *                    four instances); grids that are no multiple of 8 workgroups take 0.  Same bits; speed only
 * "store_policy"     0 .. 3 = jacobian + 2 * constant, default 1: in the pipelined kernel the Jacobian stores are plain (0) or
 *                    non-temporal (1), the stores of the constant block non-temporal (0) or write-through and non-temporal (1).
 *                    Same bits; speed only
 * "instance_align"   1 (default) or any power of two up to 65536 doubles: in the device-resident calls with n_instances > 1 the g /
 *                    values arrays of consecutive instances are rpm_get_option "stride_g" / "stride_values" doubles
 *                    apart (m, nnz_jac rounded up to this multiple) instead of packed back to back, so that every
 *                    instance starts on a 64/128-byte boundary like a separately allocated array; x stays packed; the
 *                    host-pointer entry points keep the packed layout
 * "const_once"       0 (default) | 1: host-pointer rpm_eval_jac_g downloads the linear and constant tail of `values`
 *                    (they never change, LpNLPWrapper.cpp:242, :715-718) only into a buffer it did not fill on the
 *                    previous call, afterwards just the NL prefix — for callers that hand the same array every
 *                    iteration and leave it alone in between (Ipopt's TNLPAdapter does); one instance per engine
 * "persistent_values" 0 (default) | 1: rpm_eval_jac_g_dev / rpm_eval_pair_dev remember the device `values` arrays they have
 *                    completely written and, called again with the same array, write only the entries that depend on x (and
 *                    the 2(P+L) linear ones): the constant Doffdiag block (Core/LpNLPWrapper.cpp:715-718; 54 % of the
 *                    metric problem's entries) is neither loaded nor stored again — SURVEY.md section 8(d)'s persistent-
 *                    buffer byte count B'.  Contract: the caller leaves that block of the array alone and does not free and
 *                    re-allocate the array in between; setting any option forgets every array (do that after re-allocating).
 *                    Bit-identical `values`.  The device solver (rpm_ipm_*) uses it for its own Jacobian array.
 * "delta_values"     0 (default) | 1: host-pointer rpm_eval_jac_g / rpm_eval_pair deliver `values` by difference: a kernel
 *                    compares the fresh values with a device-side mirror of what this engine last stored into the SAME
 *                    host array and stores only the 512-double runs in which a bit changed — the constant Doffdiag block, the
 *                    linear entries and every finite-difference block that does not depend on x (LpNLPWrapper.cpp:722-728 stores
 *                    them although `dependencies` is all ones, :291) cross PCIe once.  Contract as for "const_once": the caller
 *                    hands the same array and leaves it alone between calls (Ipopt's TNLPAdapter does); the engine checks 64
 *                    sampled entries of the array before every delivery and falls back to a full delivery when one differs or
 *                    the array is a different one.  Needs "pin_host" (the array is page-locked and mapped).  Results are
 *                    bit-identical to a full delivery.  get-only "delta_total_runs": runs this engine owns; "delta_sent_runs": runs
 *                    stored since the previous query of this option (blocking; for tests and reports).
 *                    Interval-sharded engines deliver only the runs they own (host-consumer multi-GPU mode).
 * "ipm_nested"       -1 (default: when the structure allows) | 0 | 1 (must), read by rpm_ipm_create: factor the KKT matrices by
 *                    nested dissection over the mesh intervals (one workgroup per interval and instance instead of one per
 *                    instance: the metric problem's single instance uses 256 CUs instead of one; 0 = one band + border matrix)
 * "ipm_nested_group" 0 (default: automatic) | positions per group: with nested dissection the separator system (block
 *                    tridiagonal along time) of a long mesh is cut once more into groups of this many of its positions, each
 *                    eliminated by a workgroup of its own (automatic: when that system is >= 512 long, groups of ~sqrt(length * bandwidth))
 * "ipm_local_border" 1 (default) | 0, read by rpm_ipm_create: with nested dissection an interval's block carries rows only for the
 *                    unknowns of the global border that its interior has entries with (its phase's t0 and tf, the phase's final
 *                    states for the last interval); 0: every interval carries the whole border (rows of zeros in L)
 * "zero_copy"        1 (default): the tile kernel reads x straight from page-locked host memory and stores g straight into it
 *                    (the caller's arrays with "pin_host", else the engine's staging buffers) — no copy-engine operations,
 *                    one launch + one synchronisation per rpm_eval_g; 0: through the engine's HBM buffers with copy-engine transfers
 * "check_finite"     1 (default): NaN/Inf in a result -> RPM_E_NONFINITE (checked on the device); 0: lpopc's behaviour
 * "pin_host"         0 (default) | 1.  0: the host-pointer entry points copy x into, and g / values / grad_f out of,
 *                    page-locked staging buffers the engine owns (CPU copies); the caller's memory is never handed to
 *                    the HIP runtime, so arrays of any lifetime may be passed (this replaces LpopcIpopt's own heap copy
 *                    of x and element-wise copy-out, Core/LpopcIpopt.cpp:135-181).  1 (opt-in; RpmTNLP asks for it on
 *                    behalf of Ipopt, whose TNLPAdapter hands the same arrays every iteration): arrays of >= 64 KB are
 *                    page-locked (hipHostRegister) the first time they are seen, the kernels read x from and store g into
 *                    them, copy engines and the delta delivery write `values` straight into them.  Registrations live in
 *                    ONE process-wide table shared by every engine of the process (librpm_pin.so): exactly the arrays'
 *                    bytes, never a byte twice, overlapping arrays as one range; an engine holds at most 8 arrays
 *                    (least recently used is let go first) and lets go of all of them in rpm_destroy or when the option
 *                    is set to 0; a range is unregistered when its last holder lets go.  A request the runtime refuses,
 *                    or that partly overlaps memory another engine holds, is served through the staging buffers instead and
 *                    is never silent: get-only "pin_register_failures", "pin_unregister_failures", "pin_overlap_refused"
 *                    (process-wide counts; also "pin_registered", "pin_unregistered", "pin_shared", "pin_merged",
 *                    "pin_evicted", "pin_live", and "pin_held" = this engine's) and the reason in rpm_last_error.
 *                    LIFETIME (option 1 only): a registered array must stay allocated until rpm_destroy, its eviction or
 *                    that release — set the option to 0 BEFORE freeing or unmapping such an array.
 */
/* Parameter sweeps (n_instances > 1): by default every instance shares the problem functor's constants
 * (rpm_problem_desc.consts — the reference keeps them in file-scope globals, example/launch/Launch.cpp:47-74).  This
 * gives instance `instance` its own copy (n = the functor's constant count), e.g. one tracking target per MPC problem;
 * all batched device-resident entry points and rpm_ipm_* then evaluate every instance with its own constants.  The
 * one-instance post-solve entry points keep using instance 0's. */
int rpm_set_instance_constants(rpm_engine* e, int instance, const double* consts, int n);
/* Every instance's constants in ONE blocking upload (a call of rpm_set_instance_constants uploads the whole array each time): what
 * n_instances such calls leave, the one-instance entry points' copy of instance 0 included.  Same refusals. */
int rpm_set_all_instance_constants(rpm_engine* e, const double* consts /* n_instances x n */, int n);
int rpm_set_option(rpm_engine* e, const char* key, int value);
int rpm_get_option(rpm_engine* e, const char* key, int* value);

/* ---- collocation tables of one phase (struct ps, Core/LpCalculateData.hpp:35-41; built like
 *      RPMGenerator::initialize, Core/RPMGenerator.cpp:43-105).  Any output may be NULL.
 *      D is returned as the reference's COO triplets in its own order. ---------------- */
int rpm_get_phase_sizes(rpm_engine* e, int phase, int* n_nodes, int* d_nnz, int* doff_nnz);
int rpm_get_phase_tables(rpm_engine* e, int phase, double* points, double* weights, int* d_rows,
                         int* d_cols, double* d_vals, double* diag_vals, int* doff_rows,
                         int* doff_cols, double* doff_vals);

/* ---- interval sharding helpers (shard_mode = RPM_SHARD_INTERVALS) --------------------
 * A rank's share of g / values is a list of contiguous runs.  Segment s of rank r is
 * dst[off .. off+len) of the full vector and sits at packed offset `pos` of that rank's
 * contiguous send buffer.  which: 0 = g, 1 = jacobian values.  Pass seg==NULL to query the
 * count.  Host only. */
typedef struct rpm_segment { int off, len, pos; } rpm_segment;
int rpm_shard_segments(rpm_engine* e, int which, int rank, rpm_segment* seg, int* n_seg,
                       int* packed_len);
/* pack this rank's runs of a full-size device vector into a contiguous device buffer / scatter a
 * gathered [world][max_packed_len] buffer back into TNLP order */
int rpm_shard_pack_dev(rpm_engine* e, int which, const double* d_full, double* d_packed, void* stream);
int rpm_shard_unpack_dev(rpm_engine* e, int which, const double* d_gathered, int stride,
                         double* d_full, void* stream);

/* ONE collective per step: the runs of g AND of the Jacobian values of ALL the engine's instances that this rank owns go
 * into one slot of rpm_shard_slot_len doubles (the same for every rank, whole 128-byte lines); the caller all-gathers the
 * [world][slot] buffer in place (RCCL; bench.py captures pack, all-gather and unpack in the step's hipGraph) and
 * rpm_shard_unpack_all_dev scatters it into TNLP order (skip_own = 1: this rank's own runs are in place already).  Instance
 * b's share of rank r's slot is [g runs | values runs] at offset b * (packed_len_g(r) + packed_len_values(r)); d_g / d_values
 * use the engine's instance strides ("instance_align").  Bit-identical to the single-GPU vectors (no reductions). */
int rpm_shard_slot_len(rpm_engine* e, long long* slot_doubles);
int rpm_shard_pack_all_dev(rpm_engine* e, const double* d_g, const double* d_values, double* d_slot, void* stream);
int rpm_shard_unpack_all_dev(rpm_engine* e, const double* d_gathered, double* d_g, double* d_values, int skip_own,
                             void* stream);

/* ---- one process, several GPUs: the mesh intervals of ONE NLP sharded over the devices of a node -------------------------
 * The caller this is for is lpopc's NLPSolver::SolveNlp (Core/LpNLPSolver.cpp:13-53): one process, one TNLP object, Ipopt
 * calling it from one thread — a second GPU is only reachable from inside the callback.  A group is one interval-sharded
 * engine per listed device (rank r computes a contiguous run of every phase's tiles, rank 0 also the endpoint rows); the
 * same device may be listed more than once.  Set-up calls (rpm_get_nlp_info, rpm_get_bounds_info, rpm_get_starting_point,
 * the structure passes, rpm_finalize_solution, the post-solve entry points) go to rpm_group_engine(g, 0): sizes and
 * layout are those of the unsharded problem.  Results are bit-identical to a single engine's (no reductions).  Calls on one
 * group are serial, as for an engine. */
#define RPM_GROUP_MAX 16
typedef struct rpm_group rpm_group;
int rpm_group_create(const rpm_problem_desc* desc, int n_devices, const int* device_ids, rpm_group** out);
void rpm_group_destroy(rpm_group* g);
const char* rpm_group_last_error(const rpm_group* g);      /* g == NULL: of the last failed rpm_group_create */
int rpm_group_size(const rpm_group* g);
rpm_engine* rpm_group_engine(rpm_group* g, int rank);
int rpm_group_device_init(rpm_group* g);                   /* optional: binds every engine to its device now */
int rpm_group_set_option(rpm_group* g, const char* key, int value);   /* rpm_set_option on every engine */
/* Host consumer — the TNLP callbacks (Core/LpopcIpopt.cpp:106-217) with every device on the data path: x, g, values are
 * the caller's arrays, page-locked once for all devices ("pin_host" is on in a group: the arrays must stay allocated until
 * rpm_group_destroy or rpm_group_set_option(g, "pin_host", 0)); every device reads x from them and stores ITS rows of g and,
 * by difference ("delta_values"), its runs of `values` straight into them over its own PCIe link; all devices are started
 * before any is waited for.  Objective, gradient and exact Hessian are evaluated by rank 0 (one small kernel each). */
int rpm_group_eval_f(rpm_group* g, int n, const double* x, int new_x, double* obj_value);
int rpm_group_eval_grad_f(rpm_group* g, int n, const double* x, int new_x, double* grad_f);
int rpm_group_eval_g(rpm_group* g, int n, const double* x, int new_x, int m, double* gvec);
int rpm_group_eval_jac_g(rpm_group* g, int n, const double* x, int new_x, int m, int nele_jac, int* iRow, int* jCol, double* values);
int rpm_group_eval_pair(rpm_group* g, int n, const double* x, int m, double* gvec, int nele_jac, double* values);
int rpm_group_eval_h(rpm_group* g, int n, const double* x, int new_x, double obj_factor, int m, const double* lambda, int new_lambda,
                     int nele_hess, int* iRow, int* jCol, double* values);
/* Device consumer on ONE device: d_x, d_g, d_values are arrays in the HBM of rank `home`'s device (instance strides as for
 * rpm_eval_pair_dev); the other ranks' tile kernels read x from and store their rows / runs into them directly over xGMI
 * (hipDeviceEnablePeerAccess) — no pack, no gather.  Blocking: returns when every rank is done. */
int rpm_group_eval_pair_dev(rpm_group* g, int home, const double* d_x, double* d_g, double* d_values);
/* All-gather: d_x[r], d_g[r], d_values[r] are full-size arrays in rank r's HBM; afterwards EVERY rank's g and values are
 * complete: each rank's tile kernel fills its rows / runs in its own arrays and one push kernel stores them into the same
 * places of every peer's arrays, one xGMI link per peer (a direct one-shot all-gather, not a ring).  Blocking. */
int rpm_group_allgather_pair_dev(rpm_group* g, const double* const* d_x, double* const* d_g, double* const* d_values);

/* ---- one process, several GPUs: the INSTANCES of a sweep dealt to the devices (the device solver of row f-2) ---------------
 * desc->n_instances independent NLPs of one transcription (the MPC sweep of BASELINE config 5), share r = instances
 * [B r / N, B (r + 1) / N) on device_ids[r] with an engine and a solver (rpm_ipm_*) of its own; the same device may be listed
 * more than once.  rpm_sweep_solve runs the shares side by side, a host thread each (the solver's loop blocks on its stream);
 * nothing crosses between devices, so every instance's result is what one engine holding all of them computes for it.  Options
 * are rpm_ipm_set_option's and go to every share; per-share objects (traces, kernel times, rpm_set_instance_constants with the
 * share's own instance numbers) through rpm_sweep_solver / rpm_sweep_engine.  Calls on one sweep are serial. */
typedef struct rpm_sweep rpm_sweep;
int rpm_sweep_create(const rpm_problem_desc* desc, int n_devices, const int* device_ids, rpm_sweep** out);
void rpm_sweep_destroy(rpm_sweep* s);
const char* rpm_sweep_last_error(const rpm_sweep* s);      /* s == NULL: of the last failed rpm_sweep_create */
int rpm_sweep_size(const rpm_sweep* s);
rpm_engine* rpm_sweep_engine(rpm_sweep* s, int share);
rpm_ipm* rpm_sweep_solver(rpm_sweep* s, int share);
int rpm_sweep_share(const rpm_sweep* s, int share, int* first_instance, int* n_instances);
int rpm_sweep_set_option(rpm_sweep* s, const char* key, double value);
int rpm_sweep_set_bounds(rpm_sweep* s, int instance, const double* x_l, const double* x_u);   /* instance: 0 .. B - 1 */
int rpm_sweep_solve(rpm_sweep* s, double* x, double* lambda, double* obj, int* status, int* iterations, double* kkt_error);
/* rpm_solution_error_batch over all shares side by side (x: B x n, instance_mask: B or NULL, results as there with B for
 * n_instances).  The shares' rel_err_max blocks are combined by element-wise maximum on the host, so the result is what one
 * engine holding all B instances returns, bit for bit; a share whose instances are all excluded contributes nothing and is no
 * error as long as one instance of the sweep is included. */
int rpm_sweep_solution_error(rpm_sweep* s, const double* x, const int* instance_mask, double* interval_error,
                             double* rel_err_max, double* rel_err, int* nonfinite);
/* rpm_carry_solution_batch on every share side by side (x_from: B x from.n, x_to: B x to.n, nonfinite: B or NULL).  The two
 * sweeps must deal their instances alike (same device list, same n_instances), else RPM_E_INVALID; the message is
 * rpm_sweep_last_error(from). */
int rpm_sweep_carry_solution(rpm_sweep* from, rpm_sweep* to, const double* x_from, double* x_to, int* nonfinite);
/* rpm_carry_multipliers_batch on every share side by side (lambda_from: B x from.m, lambda_to: B x to.m), sweeps dealt alike */
int rpm_sweep_carry_multipliers(rpm_sweep* from, rpm_sweep* to, const double* x_from, const double* lambda_from, double* lambda_to,
                                int* nonfinite);
/* rpm_ipm_solve_warm / rpm_ipm_get_bound_multipliers over all shares at once (x, z_L, z_U: B x n, lambda: B x m) */
int rpm_sweep_solve_warm(rpm_sweep* s, double* x, double* lambda, double* z_L, double* z_U, double* obj, int* status, int* iterations,
                         double* kkt_error);
int rpm_sweep_get_bound_multipliers(rpm_sweep* s, double* z_L, double* z_U);
/* rpm_ipm_sensitivities of every share: dx B x n_par x n, dlambda B x n_par x m or NULL, delta_w and info B or NULL */
int rpm_sweep_sensitivities(rpm_sweep* s, int n_par, const int* var_index, double* dx, double* dlambda, double* delta_w, int* info);
/* rpm_ipm_constant_sensitivities of every share, laid out alike */
int rpm_sweep_constant_sensitivities(rpm_sweep* s, int n_par, const int* const_index, double* dx, double* dlambda, double* delta_w,
                                     int* info);
/* rpm_shift_plan_batch / rpm_ipm_set_initial_states on every share side by side (host arrays, all B instances: dt B x n_phases,
 * state0 B x nx): what one engine holding all B instances computes, bit for bit */
int rpm_sweep_shift_plan(rpm_sweep* s, const double* dt, const double* x, double* x_out, const double* lambda, double* lambda_out,
                         const double* z_L, const double* z_U, double* z_L_out, double* z_U_out, int* nonfinite);
int rpm_sweep_set_initial_states(rpm_sweep* s, int phase, const double* state0);
/* rpm_sample_plan_batch / rpm_rollout_batch on every share side by side (host arrays, all B instances, dealt as
 * rpm_sweep_shift_plan deals them: times B x n_times, out B x (nx + nu) x n_times; t_start, dt B, state0 / state_out B x nx, traj
 * B x (n_steps + 1) x nx): what one engine holding all B instances computes, bit for bit.  NULL x, times, out, dt or state_out, a
 * phase, n_times or n_steps out of range: RPM_E_INVALID with the message in rpm_sweep_last_error(s). */
int rpm_sweep_sample_plan(rpm_sweep* s, int phase, const double* x, int n_times, const double* times, double* out, int* nonfinite);
int rpm_sweep_rollout(rpm_sweep* s, int phase, const double* x, const double* t_start, const double* dt, int n_steps, int hold,
                      const double* state0, double* state_out, double* traj, int* nonfinite);
/* rpm_nlp2op_batch on every share side by side (x: B x n, lambda: B x m, out: B x EB, nonfinite: B or NULL): what one engine
 * holding all B instances returns, bit for bit. */
int rpm_sweep_nlp2op(rpm_sweep* s, const double* x, const double* lambda, double* out, int* nonfinite);
int rpm_sweep_get_stats(rpm_sweep* s, int* iterations, int* factorizations, int* trial_points);

#ifdef __cplusplus
}
#endif
#endif /* RPM_HIP_H_ */
