/*
 * hmpc.h -- C ABI of the MI355X batched MPC/QP solve path.
 *
 * Drop-in boundary for the per-timestep QP of bbokser/hopper-mpc-inertial:
 * every entry point below replaces one piece of the reference's
 * ``Mpc`` class (src/mpc_cvx_euler_3f.py, src/mpc_cvx_euler_2f.py):
 *
 *   hmpc_create          <- Mpc.__init__(t, N, m, g, mu, Jinv, rh)
 *                           (src/mpc_cvx_euler_3f.py:12-39, 2f :12-38)
 *   hmpc_solve_batch     <- Mpc.gen_dt_dynamics + Mpc.build_qp + Mpc.solve_qp
 *                           (3f :71-160, 2f :70-158), one QP per instance,
 *                           B instances per call, device pointers
 *   hmpc_solve_batch_host  same, host pointers (staged through the context's
 *                           device buffers; synchronous)
 *   hmpc_mpcontrol_batch <- Mpc.mpcontrol(x_in, x_ref_in, pf, C, init)
 *                           (3f :41-69): builds the linearisation x_hat
 *                           (init: [x_in; x_ref], else the time shift of the
 *                           previous x*) on device, runs 1 or 2 solves
 *   hmpc_mpcontrol_plan_batch <- the Runner's call (src/robotrunner.py:98-107):
 *                           Mpc.mpcontrol on path_plan_grab(x_ref, k) /
 *                           path_plan_grab(pf_ref, k) read in place from a
 *                           device-resident plan (:228-230), no staging
 *   hmpc_plant_batch     <- Runner.rk4_normalized / dynamics_ct
 *                           (src/robotrunner.py:126-164) for n_steps
 *                           low-level steps, then convert (:19-28)
 *   hmpc_convert_batch   <- convert(X) (src/robotrunner.py:19-28)
 *   hmpc_plan_batch      <- Runner.path_plan_init (src/robotrunner.py:182-226)
 *                           + gait_map (:174-180), one plan per robot
 *   hmpc_gait_batch      <- the Runner loop's gait_scheduler / gait_map calls
 *                           (src/robotrunner.py:92-101)
 *   hmpc_kkt_batch       <- the duals problem.solve() leaves in cvxpy's
 *                           dual_value / OSQP's y (src/mpc_cvx_euler_3f.py:156-157)
 *                           for a given primal point, plus a KKT certificate
 *   hmpc_sens_batch      <- no reference analogue: the Jacobian d u* / d x_in of that
 *                           solve at its active set (feedback gain between solves)
 *   hmpc_vjp_batch       <- no reference analogue: reverse-mode gradients of a loss on
 *                           (u*, x*) with respect to x_in, x_ref and pf at that active set
 *   hmpc_vjp_lin_batch   <- no reference analogue: the same pass with the gradients in
 *                           x_lin and mu as well -- what backpropagation through
 *                           Mpc.mpcontrol (src/mpc_cvx_euler_3f.py:41-69), whose x_guess
 *                           depends on x_in and on the previous solve, needs
 *   hmpc_plant_vjp_batch <- no reference analogue: the adjoint of rk4_normalized / convert
 *                           (src/robotrunner.py:154-164, :19-28), so that a loss on the
 *                           closed-loop trajectory reaches the plan and the start state
 *   hmpc_plant_fb_batch  <- no reference analogue: hmpc_plant_batch with the input of every
 *                           low-level step corrected by hmpc_sens_batch's K_0 (the reference
 *                           holds u*_0 over the period, src/robotrunner.py:104-113)
 *   hmpc_destroy        <- object lifetime
 *
 * Conventions: every array is row-major, contiguous, float64, batch-major
 * (instance b's x_ref is x_ref[b*N*12 .. (b+1)*N*12)).  C holds the contact
 * schedule as 0.0/1.0 like the reference's gait_map.  Errors are returned as
 * negative int codes and never thrown across the ABI; per-instance solver
 * outcomes are written to ``status`` (HMPC_SOLVED, ...).  A status other than
 * HMPC_SOLVED corresponds to the reference raising
 * Exception("\n *** QP FAILED *** \n") (src/mpc_cvx_euler_3f.py:158-159).
 */
#ifndef HMPC_H
#define HMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* return codes (API level) */
#define HMPC_OK 0
#define HMPC_ERR_ARG -1           /* bad argument / null pointer / misaligned */
#define HMPC_ERR_UNSUPPORTED -2   /* (variant, N) without a compiled kernel   */
#define HMPC_ERR_HIP -3           /* HIP runtime error (see hmpc_last_error)  */
#define HMPC_ERR_NOMEM -4

/* per-instance status codes */
#define HMPC_SOLVED 0
#define HMPC_MAX_ITER 1
#define HMPC_PRIMAL_INFEASIBLE 2
#define HMPC_NUMERICAL 3          /* condensed Hessian not positive definite */

/* variants: the two dynamics formulations of the reference */
#define HMPC_VARIANT_3F 3         /* src/mpc_cvx_euler_3f.py: world-frame force */
#define HMPC_VARIANT_2F 2         /* src/mpc_cvx_euler_2f.py: body-frame, fy = 0 */
#define HMPC_VARIANT_CAS 4        /* src/mpc_cas_euler_3f.py: the CasADi/qpOASES
                                     variant's QP as the reference builds it
                                     (second-order discretisation at the yaw of
                                     x_in, one-sided dynamics rows, scalar u_ref;
                                     x_lin and pf are ignored, rf is fixed);
                                     1 <= N <= 11, fp64 only */

/* u_ref semantics */
#define HMPC_UREF_ALIASED 0       /* what cvxpy actually solves: every stage sees
                                     the last stage's u_ref (the default)        */
#define HMPC_UREF_PER_STAGE 1     /* the intended per-stage 2mg*C[k]             */

/* arithmetic of the solve (hmpc_set_precision) */
#define HMPC_PREC_F64 0           /* fp64; the dedicated kernel when N has one (default) */
#define HMPC_PREC_F32 1           /* fp32 arithmetic (BASELINE configs[4]: the tolerance/
                                     throughput trade-off): the dense kernel's fp32
                                     build where N has one (N = 10), else generic */
#define HMPC_PREC_F64_GENERIC 2   /* fp64 on the generic kernel (its fp32 twin's A/B) */
#define HMPC_PREC_F64_RICCATI 3   /* fp64 on the Riccati kernel (any N <= 64; the default
                                     for 10 < N <= 64)                            */
#define HMPC_PREC_F64_DENSE 4     /* fp64 on the dedicated dense kernel of N (compiled
                                     horizons only; the default for N <= 10)      */
#define HMPC_PREC_F32_GENERIC 5   /* fp32 on the generic kernel (round-1 configs[4]) */
#define HMPC_PREC_F32_REFINED 6   /* configs[4]'s fp32 + fp64 iterative refinement: the fp32
                                     dense kernel's factors and active set, then
                                     hmpc_set_refinement() corrections of that active set's
                                     KKT system with fp64 residuals; an instance whose fp64
                                     check fails goes to the fp64 overflow pass (N = 10) */

typedef struct hmpc_ctx hmpc_ctx;

/* ABI version (major*10000 + minor*100 + patch): 1.2.0 = 1.0 + the fp32 dense
   build, HMPC_PREC_F64_RICCATI / _F64_DENSE / _F32_GENERIC, hmpc_kernel_name,
   hmpc_active_capacity, hmpc_plan_batch, hmpc_gait_batch, HMPC_VARIANT_CAS;
   1.3.0 = + hmpc_solve_batch_stats, HMPC_PREC_F32_REFINED, hmpc_set_refinement;
   1.4.0 = + hmpc_set_order;
   1.5.0 = + hmpc_overflow_total;
   1.5.1 = hmpc_kernel_name / hmpc_active_capacity report the last solve's N = 60
           kernel (capacity 64 at small batches);
   1.5.2 = the cross-stream completion event is recorded at a stream switch,
           not after every call (the last call's stream must stay valid);
           + hmpc_kkt_batch, + hmpc_sens_batch, + hmpc_vjp_batch,
           + hmpc_vjp_lin_batch, + hmpc_plant_vjp_batch, + hmpc_plant_fb_batch (additions:
           the version number is unchanged) */
int hmpc_version(void);

/* Which horizons have a dedicated (one- or two-wavefront) kernel for
   `variant`; writes up to `cap` values into `Ns`, returns the count.  Every
   other horizon 1 <= N <= 64 (e.g. the Runner's N = 60) is solved by the
   Riccati kernel (one wavefront per instance, the condensed Hessian factored
   by a backward Riccati recursion), 64 < N <= 128 by the generic dense kernel.
   Every solve with N <= 64 re-solves the rare instances whose active set
   outgrows its kernel's capacity in an overflow pass (capacity 6N).  The
   context's workspaces and counters are shared by its calls, so the context
   orders them itself: a call on a different stream than the context's last
   one first records an event on that last stream and makes its own stream
   wait for it (hipStreamWaitEvent), so the stream of a context's last call
   must stay valid until the context's next call (or hmpc_overflow_total,
   which synchronises it).  Eager calls on one context never overlap; use one
   context per stream for concurrent solves.  Calls enqueued while their stream
   captures a HIP graph are outside this ordering (a replay runs whenever the
   caller launches it): the caller orders a graph's replays against the
   context's other streams, e.g. by synchronising the replay stream before
   the next eager call elsewhere (hmpc_runner.Runner does). */
int hmpc_supported_horizons(int variant, int* Ns, int cap);

/* Mpc.__init__: t = MPC sampling time (s), N = horizon, m (kg), g (m/s^2),
   mu = friction coefficient used when a batch passes mu == NULL,
   Jinv = inverse inertia (row-major 3x3), rh = hip offset (3).
   device = HIP device ordinal to bind the context to. */
int hmpc_create(hmpc_ctx** out, int variant, int N, double t, double m, double g,
                double mu, const double* Jinv, const double* rh, int uref_mode,
                int device);

/* The part of the cost-to-go S_t (t = 1..N, row t - 1) that does not depend on
 * the instance, as the context builds it once at creation for its kernels:
 * out[N][12] = [pp, pv, vv] of the x, y, z axes, then [tt, tw, ww] of yaw.
 * Host only. */
int hmpc_ctg_table(int N, double t, double* out);

/* The translational part of the 3f condensed Hessian, which depends on
 * (N, t, m) only: out[3][N(N+1)/2], for the axes x, y, z the lower triangle
 * (row i at i(i+1)/2) of H[(i, a), (j, a)] through (p_a, v_a).  Host only. */
int hmpc_hess_table(int N, double t, double m, double* out);

int hmpc_destroy(hmpc_ctx* ctx);

/* One QP per instance on the given linearisation x_lin (device pointers).
     x_in  [B,12]       initial state (constraint x[0] == x_in)
     x_lin [B,N+1,12]   linearisation trajectory (rows 0..N-1, cols 0:3 and 5 used)
     x_ref [B,N,12]     reference trajectory
     pf    [B,N,3]      footstep plan
     C     [B,N]        contact schedule (0.0 swing / 1.0 stance)
     mu    [B] or NULL  friction coefficient per instance
   outputs
     u     [B,N,6]      optimal inputs u*
     x     [B,N+1,12]   optimal states x* (may be NULL)
     obj   [B]          optimal objective incl. its constant term (may be NULL)
     status[B]          HMPC_SOLVED / ...
     iters [B]          active-set iterations (may be NULL)
   `stream` is a hipStream_t (NULL = default stream).  Asynchronous. */
int hmpc_solve_batch(hmpc_ctx* ctx, int64_t B,
                     const double* x_in, const double* x_lin, const double* x_ref,
                     const double* pf, const double* C, const double* mu,
                     double* u, double* x, double* obj, int32_t* status, int32_t* iters,
                     void* stream);

/* hmpc_solve_batch plus one more output: active [B] receives each
   instance's final active-set size (the number of inequality rows active at
   the optimum the solver certifies; may be NULL).  The bench feeds its mean
   into the algorithmic flop count (bench.algorithmic_flops). */
int hmpc_solve_batch_stats(hmpc_ctx* ctx, int64_t B,
                           const double* x_in, const double* x_lin, const double* x_ref,
                           const double* pf, const double* C, const double* mu,
                           double* u, double* x, double* obj, int32_t* status, int32_t* iters,
                           int32_t* active, void* stream);

/* Same with host pointers; synchronous. */
int hmpc_solve_batch_host(hmpc_ctx* ctx, int64_t B,
                          const double* x_in, const double* x_lin, const double* x_ref,
                          const double* pf, const double* C, const double* mu,
                          double* u, double* x, double* obj, int32_t* status, int32_t* iters);

/* Mpc.mpcontrol for B independent controllers (device pointers).
   x_prev [B,N+1,12] is read when init == 0 (the previous x*) and always
   overwritten with the new x*.  u [B,N,6] receives the control.  Status is
   the worst status over the (1 or 2) solves.  Asynchronous. */
int hmpc_mpcontrol_batch(hmpc_ctx* ctx, int64_t B, int init,
                         const double* x_in, const double* x_ref, const double* pf,
                         const double* C, const double* mu,
                         double* x_prev, double* u, double* obj, int32_t* status,
                         int32_t* iters, void* stream);

/* Mpc.mpcontrol for B robots against a plan resident on the device
   (src/robotrunner.py:98-107).  x_ref_plan [T,12] and pf_plan [T,3] are the
   Runner's path_plan_init output (one per robot when plan_bstride = T rows,
   shared when 0); robot b's window is rows k, k + f, ..., k + (N-1) f
   (path_plan_grab, f = mpc_factor), which must lie inside [0, T).  C [N] is
   gait_map(N, mpc_dt, t, t0), shared by the batch when C_bstride = 0.
   Otherwise as hmpc_mpcontrol_batch.  Asynchronous. */
int hmpc_mpcontrol_plan_batch(hmpc_ctx* ctx, int64_t B, int init,
                              const double* x_in, const double* x_ref_plan,
                              const double* pf_plan, int64_t T, int64_t plan_bstride,
                              int64_t k, int mpc_factor,
                              const double* C, int64_t C_bstride, const double* mu,
                              double* x_prev, double* u, double* obj, int32_t* status,
                              int32_t* iters, void* stream);

/* The Runner's plant between two MPC solves, for B robots on the device:
   n_steps RK4 steps of dynamics_ct with step dt and the input held
   (src/robotrunner.py:104-113,126-164).  X [B,13] (p, q = [w,x,y,z], v, w:
   the simulator's SE(3) state) is advanced in place.  The held input of robot
   b is U[b*U_bstride .. +6) (pass the mpcontrol output u with U_bstride = 6N
   to take its first row, as the Runner does).  Step s uses the foot position
   pf[b*pf_bstride + s*pf_sstride .. +3) (the Runner's pf_ref[k + s]).
   J [9] is the body inertia (host pointer); m, g, rh and J^-1 come from the
   context.  X_hist [B,n_steps,13] (optional) receives every step's state,
   x_out [B,12] (optional) convert(X) after the last one.  Asynchronous. */
int hmpc_plant_batch(hmpc_ctx* ctx, int64_t B, int n_steps, double dt, const double* J,
                     double* X, const double* U, int64_t U_bstride,
                     const double* pf, int64_t pf_bstride, int64_t pf_sstride,
                     double* X_hist, double* x_out, void* stream);

/* x [B,12] = convert(X [B,13]) (src/robotrunner.py:19-28).  Asynchronous. */
int hmpc_convert_batch(hmpc_ctx* ctx, int64_t B, const double* X, double* x, void* stream);

/* Reverse-mode gradients of one hmpc_plant_batch call: the adjoint of n_steps of
   rk4_normalized (src/robotrunner.py:154-164) and of the convert (:19-28) that
   follows them.  Inputs are that call's (device pointers; J host):
     X0         [B,13]          the state before the call
     X_hist     [B,n_steps,13]  the call's X_hist (required when n_steps >= 2: the
                                checkpoints; its last row is not read)
     U, pf      addressed exactly as in hmpc_plant_batch
   Cotangents (each may be NULL = 0, not all three):
     g_X        [B,13]          on the final state
     g_x_out    [B,12]          on convert(final state)
     g_X_hist   [B,n_steps,13]  on every step's state (its last row adds to g_X)
   Outputs (each may be NULL, not all three):
     grad_X0    [B,13]          all four quaternion components are independent
     grad_U     [B,6]           the held input
     grad_pf    [B,n_steps,3]   per robot and step, whatever strides pf was read with
   dt, J, m, g and rh are constants.  n_steps = 0 is the adjoint of hmpc_convert_batch
   (g_x_out) with g_X added to grad_X0; g_X_hist and grad_pf must then be NULL.  convert
   is differentiated along the branch it took; at its gimbal branch (cos(pitch) <= 4 eps)
   it is not differentiable: the yaw contributes 0 and the result is otherwise undefined.
   Serves every context (CAS included), like hmpc_plant_batch.  Asynchronous, allocates
   nothing (can be captured into a HIP graph). */
int hmpc_plant_vjp_batch(hmpc_ctx* ctx, int64_t B, int n_steps, double dt, const double* J,
                         const double* X0, const double* X_hist,
                         const double* U, int64_t U_bstride,
                         const double* pf, int64_t pf_bstride, int64_t pf_sstride,
                         const double* g_X, const double* g_x_out, const double* g_X_hist,
                         double* grad_X0, double* grad_U, double* grad_pf, void* stream);

/* hmpc_plant_batch under the feedback law of hmpc_sens_batch's gain (no reference analogue:
   the reference holds u*_0 for the whole MPC period).  Low-level step s = 0 .. n_steps-1 of
   robot b applies
     x_s  = convert(X_s)
     xbar = x_nom[b,0] + (s / stage_steps) (x_nom[b,1] - x_nom[b,0])   with HMPC_FB_INTERP,
            else x_nom[b,0]
     d    = x_s - xbar,  d[5] -= 2 pi rint(d[5] / 2 pi)                (the yaw only)
     u_s  = U[b] + K[b] d,  clipped with HMPC_FB_CLIP
   and X_s+1 = rk4_normalized(X_s, u_s, pf[b,s]) with u_s held over the four stages.  Within
   the critical region of the solve's active set u_s is the QP's own optimum for the state
   x_s.  The clip is the QP's input set (src/mpc_cvx_euler_3f.py:113-136, 2f), in this order:
   torques to +-7.78, 7.78, 4; a swing leg (C0 == 0) gets f = 0; a stance leg fz to [0, 206],
   then fx to +-mu_b fz and fy to +-mu_b fz (3f and CAS contexts) or to 0 (2f).
     U      robot b's nominal input u*_0 at U[b*U_bstride .. +6)
     K      its row-major [6][12] gain at K[b*K_bstride .. +72) (K_bstride = 72 for the S
            [B,1,6,12] of hmpc_sens_batch with n_stages = 1)
     x_nom  rows 0 and 1 at x_nom[b*xnom_bstride .. +24) (xnom_bstride = 12 (N+1) for x*
            itself; row 1 is read only with HMPC_FB_INTERP)
     pf     as in hmpc_plant_batch
     C0     the period's contact flag at C0[b*C0_bstride] (the first entry of the solve's C
            row), or NULL = stance
     mu     [B] or NULL = the context's
   Outputs: X in place; X_hist [B,n_steps,13], U_hist [B,n_steps,6] (the applied inputs),
   x_out [B,12] = convert(X) after the last step and sat [B] (the number of steps in which
   the clip moved a component by more than 1e-8 (1 + |bound|), the rule of hmpc_kkt_batch's
   act_tol; 0 without HMPC_FB_CLIP) may each be NULL.  J is a host pointer.  HMPC_ERR_ARG for
   a null X, U, K, x_nom, pf or J, n_steps < 1, stage_steps < 1, an unknown flag bit, a
   negative stride or dt <= 0.  Serves every context, like hmpc_plant_batch.  Asynchronous,
   allocates nothing (can be captured into a HIP graph). */
#define HMPC_FB_CLIP   1
#define HMPC_FB_INTERP 2
int hmpc_plant_fb_batch(hmpc_ctx* ctx, int64_t B, int n_steps, int stage_steps, double dt,
                        const double* J, double* X,
                        const double* U, int64_t U_bstride,
                        const double* K, int64_t K_bstride,
                        const double* x_nom, int64_t xnom_bstride,
                        const double* pf, int64_t pf_bstride, int64_t pf_sstride,
                        const double* C0, int64_t C0_bstride,
                        const double* mu, int flags,
                        double* X_hist, double* U_hist, double* x_out, int32_t* sat, void* stream);

/* Runner.path_plan_init (src/robotrunner.py:182-226) for B robots on the
   device: robot b's plan from its own start x_in[b] and goal xf[b] (convert()ed
   MPC states, [B,12] device) into x_ref [B,T,12] and pf_ref [B,T,3], T = N_run +
   N_k (N_k = N * mpc_factor: the MPC horizon in low-level steps).  curve != 0 is
   the --curve plan with the reference's quirks (:193-201).  t_p, phi_switch,
   t_start and step_adjustment are the Runner's gait constants (:44-49,78-79);
   C_map [T] (optional) receives gait_map(T, dt, t_start, 0) (:213).  Feeds
   hmpc_mpcontrol_plan_batch with plan_bstride = T.  Synchronous on `stream`
   (once per run): returns HMPC_ERR_ARG where the reference raises IndexError
   (a footstep peak moved outside the plan by step_adjustment, or a footstep
   counter past the end of idx_pf, :211-223) or a robot has more than 64
   footstep peaks; the plan is then not valid. */
int hmpc_plan_batch(hmpc_ctx* ctx, int64_t B, int N_run, int N_k, double dt, int curve, double t_p,
                    double phi_switch, double t_start, int step_adjustment, const double* x_in,
                    const double* xf, double* x_ref, double* pf_ref, double* C_map, void* stream);

/* The Runner loop's gait schedule (src/robotrunner.py:92-101,166-180) on the
   device: t = t_start; for step k < n_steps: t += dt, s_hist[k] =
   gait_scheduler(t, t0) (optional output), and at every MPC call (k % mpc_factor
   == 0) the row C_calls[p] = gait_map(N, mpc_dt, t, t0) of [n_calls, N], with
   the reference's float64 time accumulation.  Asynchronous. */
int hmpc_gait_batch(hmpc_ctx* ctx, int n_steps, int mpc_factor, int N, double dt, double mpc_dt, double t_p,
                    double phi_switch, double t_start, double t0, double* C_calls, double* s_hist,
                    void* stream);

/* Arithmetic of every later solve on this context (HMPC_PREC_*; inputs and
   outputs stay fp64 at the ABI).  BASELINE configs[4] asks for fp32 vs fp64:
   fp32 loses most of the 1e-6 tolerance on this ill-conditioned problem
   (reduced Hessian condition ~3e6), see DESIGN.md. */
int hmpc_set_precision(hmpc_ctx* ctx, int precision);

/* Number of fp64 corrections HMPC_PREC_F32_REFINED runs (0..16, default 5:
   each contracts the error by ~cond x eps32, measured max|du| 1.7e-3 / 7.4e-5 /
   3.1e-6 / 1.3e-7 / 6.4e-9 after 2 / 3 / 4 / 5 / 6 on configs[4]; each costs an
   fp64 rollout + adjoint and two fp32 sweeps per instance).  An instance is
   accepted only when its last correction is below 4e-6 (converged), so with
   fewer than about 4 corrections -- 0 included -- nearly every instance fails
   that check and is re-solved by the fp64 overflow pass: the results stay
   exact, the cost is that of the fp64 pass for the whole batch. */
int hmpc_set_refinement(hmpc_ctx* ctx, int corrections);

/* Instance order of later solves (results do not depend on it):
     HMPC_ORDER_AUTO            longest-first for small batches, where the
                                instances that start last set the step time
                                (dense split B <= 8192; Riccati kernel up to 8
                                instances per resident workgroup), else index
     HMPC_ORDER_INDEX           batch index order
     HMPC_ORDER_LONGEST_FIRST   stance-stage buckets, most stance stages first
   Longest-first measured +21 % at configs[1] (B = 4096) and +12 % at the
   Runner's N = 60 (B = 4096); -0.4 % at configs[2], -6 % at configs[3]. */
#define HMPC_ORDER_AUTO 0
#define HMPC_ORDER_INDEX 1
#define HMPC_ORDER_LONGEST_FIRST 2
int hmpc_set_order(hmpc_ctx* ctx, int order);

/* Name of the solve kernel this context's (variant, N, precision) runs on,
   as rocprofv3 demangles it, e.g. "hmpc::ric_kernel<3, 2, 0, 0, 0>" (the Riccati
   horizons above 24 run "hmpc::ric_factor_kernel<...> + hmpc::ric_kernel<..., 2>"); a split launch names
   every class kernel, "hmpc::solve_kernel<3, 10, double, 48, 13> + hmpc::solve_kernel<3, 10,
   double, 0, 0>" (the narrowest first; 2f's full class is the 5N-wide
   "hmpc::solve_kernel<2, 10, double, 50, 20>"; the fp32 builds list the fp64
   "hmpc::swing_kernel<10, 13>" class first).  N = 60 names the last solve's
   kernel: batches up to three workgroups per CU run the capacity-64
   "hmpc::ric_kernel<3, 1, 60, 64, 2>".  Static string, "" when none.  For
   benchmark records and profiles. */
const char* hmpc_kernel_name(hmpc_ctx* ctx);

/* Active-set capacity of that kernel's main pass (-1 when none): instances
   whose active set grows beyond it are re-solved by the overflow pass
   (capacity 6N) inside the same call, so this is a performance figure, not a
   limit (0 for the generic kernel, which has no overflow pass).  N = 60: the
   last solve's (64 for small batches, else 47, whose overflows go first to a
   capacity-64 second tier). */
int hmpc_active_capacity(hmpc_ctx* ctx);

/* Instances the overflow pass has re-solved on this context since it was
   created: the active sets that outgrew the main pass's capacity, and (the
   fp32 + fp64 refinement build) the instances whose fp64 check or
   convergence test failed.  Waits for the context's last solve.  No
   reference analogue: it reports where the GPU path spends its slow pass. */
int hmpc_overflow_total(hmpc_ctx* ctx, int64_t* total);

/* Lagrange multipliers and a KKT certificate of a primal point (x, u) of the
   QP hmpc_solve_batch solves: what problem.solve() leaves in cvxpy's
   dual_value / OSQP's y (src/mpc_cvx_euler_3f.py:156-157).  Inputs as
   hmpc_solve_batch (device pointers); u [B,N,6] and x [B,N+1,12] are the point
   to certify -- a solve's output at any precision, or a point from elsewhere.
   A row is active when its slack is <= act_tol (1 + |bound|) (1e-8 is the
   usual value).  Outputs, in the sign convention of OSQP's y:
     nu   [B,N]     multiplier of x[k][2] >= 0.1, nu >= 0 (nu[0] = 0: that row
                    sits on the fixed x[0]); may be NULL
     lam  [B,N,11]  per stage (may be NULL):
                    0-2   tau_x, tau_y, tau_z (> 0 at the upper bound, < 0 at the lower)
                    3-6   fx - mu fz, -fx - mu fz, fy - mu fz, -fy - mu fz (>= 0)
                    7     fz (> 0 at 206, < 0 at 0)
                    8-10  the fixed fx, fy, fz (swing stages; 2f: fy), free sign
                    unused slots are 0.  At a stance stage with fz = 0 the five
                    force rows are dependent: the minimal nonnegative split is
                    reported (friction rows take the positive and negative parts,
                    fz >= 0 the rest)
     cert [B,5]     primal_eq, primal_ineq, dual_neg, stationarity (scaled by
                    1 + max|q|), complementarity: the certificate of a QP in
                    OSQP form, l <= A z <= u
     flags[B]       HMPC_KKT_SINGULAR when active z rows are dependent given
                    the pinned inputs (their nu is then reported as 0); may be NULL
   Serves the 3f and 2f variants for 1 <= N <= 64 (else HMPC_ERR_UNSUPPORTED).
   Asynchronous, allocates nothing (can be captured into a HIP graph). */
#define HMPC_KKT_SINGULAR 1
int hmpc_kkt_batch(hmpc_ctx* ctx, int64_t B,
                   const double* x_in, const double* x_lin, const double* x_ref,
                   const double* pf, const double* C, const double* mu,
                   const double* u, const double* x, double act_tol,
                   double* nu, double* lam, double* cert, int32_t* flags,
                   void* stream);

/* First-order sensitivity of the optimum to the measured state at a primal
   point (x, u) of the QP hmpc_solve_batch solves:
     S[b,k,c,i] = d u*_k[c] / d x_in[i],   k < n_stages
   with x_lin, x_ref, pf, C and mu held fixed.  mpcontrol's own dependence of
   x_lin[0] on x_in is NOT part of it: the derivative is that of one QP.  Inputs
   as hmpc_kkt_batch (device pointers; x_in and x_ref do not enter the slope but
   are required).  A row is active when its slack is <= act_tol (1 + |bound|),
   the rule of hmpc_kkt_batch, and every active row is held as an equality
   whether or not its multiplier is zero; a stance stage with fz = 0 pins all
   three force components.  n_stages = 1 gives the feedback gain K_0 [B,6,12]
   for u = u*_0 + K_0 (x - x_in) between solves.  Outputs:
     S     [B,n_stages,6,12]   (also the call's only workspace: allocate exactly this)
     flags [B]  HMPC_SENS_SINGULAR when an active z row is dependent given the
                pinned inputs and was dropped (a z row at stage 1 always is).  The
                z row of stage 0 sits on the fixed x[0] and is never held: with
                x_in[2] at 0.1 it would contradict dx_0 = e_2, so S is the
                derivative on the feasible side;
                HMPC_SENS_ZROWS is reserved for a kernel that carries fewer z
                rows than a horizon can hold (S would then be 0): this one
                carries all N - 1 and never sets it.  May be NULL
   Serves the 3f and 2f variants for 1 <= N <= 64 (else HMPC_ERR_UNSUPPORTED);
   n_stages outside 1..N is HMPC_ERR_ARG.  Asynchronous, allocates nothing (can
   be captured into a HIP graph). */
#define HMPC_SENS_SINGULAR 1   /* a dependent active z row was dropped */
#define HMPC_SENS_ZROWS    2   /* more active z rows than the kernel carries; S is 0 */
int hmpc_sens_batch(hmpc_ctx* ctx, int64_t B,
                    const double* x_in, const double* x_lin, const double* x_ref,
                    const double* pf, const double* C, const double* mu,
                    const double* u, const double* x, double act_tol,
                    int n_stages, double* S, int32_t* flags, void* stream);

/* Reverse-mode gradients of the solve: for the cotangents g_u = dL/du* and
   g_x = dL/dx* of a scalar loss,
     grad_theta = (d u* / d theta)' g_u + (d x* / d theta)' g_x,   theta = x_in, x_ref, pf
   at a primal point (x, u) of the QP hmpc_solve_batch solves, with x_lin, C and
   mu held fixed.  The solution map is the one hmpc_sens_batch differentiates:
   one QP with its active set held (slack <= act_tol (1 + |bound|), every active
   row an equality, a stance stage with fz = 0 pins all three force components,
   the z row of stage 0 is never held).  x*_0 = x_in, so g_x[:,0] reaches
   grad_x_in directly.  Inputs as hmpc_sens_batch (device pointers), then
     g_u        [B,N,6]     may be NULL (= 0)
     g_x        [B,N+1,12]  may be NULL (= 0); not both NULL
     grad_x_in  [B,12]      may be NULL (not computed)
     grad_x_ref [B,N,12]    may be NULL
     grad_pf    [B,N,3]     may be NULL; not all three NULL
     flags      [B]         HMPC_VJP_SINGULAR as HMPC_SENS_SINGULAR; may be NULL
   One adjoint solve per instance, whatever the number of parameters.  Serves
   the 3f and 2f variants for 1 <= N <= 64 (else HMPC_ERR_UNSUPPORTED).
   Asynchronous, allocates nothing (can be captured into a HIP graph). */
#define HMPC_VJP_SINGULAR 1   /* a dependent active z row was dropped (as HMPC_SENS_SINGULAR) */
int hmpc_vjp_batch(hmpc_ctx* ctx, int64_t B,
                   const double* x_in, const double* x_lin, const double* x_ref,
                   const double* pf, const double* C, const double* mu,
                   const double* u, const double* x, double act_tol,
                   const double* g_u, const double* g_x,
                   double* grad_x_in, double* grad_x_ref, double* grad_pf,
                   int32_t* flags, void* stream);

/* hmpc_vjp_batch with the gradients in the linearisation point and the friction
   coefficient as well, from the same adjoint solve and the same solution map.
   Inputs as hmpc_vjp_batch, and the multipliers of the primal point as
   hmpc_kkt_batch writes them (device pointers, both required):
     nu         [B,N]
     lam        [B,N,11]
   Outputs (each may be NULL, not all five):
     grad_x_in, grad_x_ref, grad_pf   as hmpc_vjp_batch, bit for bit
     grad_x_lin [B,N+1,12]  written in full: rows 0..N-1, columns 0:3 (position)
                            and 5 (yaw) -- what gen_dt_dynamics reads -- carry the
                            gradient, every other entry is 0.0
     grad_mu    [B]         also written when mu is NULL (the context's default)
     flags      [B]         HMPC_VJP_SINGULAR; may be NULL
   With x_lin[:,0] = x_in and x_lin[:,1:] taken from an earlier solve these are the
   terms a chain rule through Mpc.mpcontrol needs.  Serves the 3f and 2f variants
   for 1 <= N <= 64 (else HMPC_ERR_UNSUPPORTED).  Asynchronous, allocates nothing
   (can be captured into a HIP graph). */
int hmpc_vjp_lin_batch(hmpc_ctx* ctx, int64_t B,
                       const double* x_in, const double* x_lin, const double* x_ref,
                       const double* pf, const double* C, const double* mu,
                       const double* u, const double* x, double act_tol,
                       const double* nu, const double* lam,
                       const double* g_u, const double* g_x,
                       double* grad_x_in, double* grad_x_ref, double* grad_pf,
                       double* grad_x_lin, double* grad_mu,
                       int32_t* flags, void* stream);

/* Last HIP error string of this context ("" if none). */
const char* hmpc_last_error(hmpc_ctx* ctx);

/* Kernel-level timing support for benchmarks: launches the solve kernel
   `reps` times on `stream` between two HIP events and returns the mean
   kernel time in milliseconds through *ms (device pointers as in
   hmpc_solve_batch). */
int hmpc_time_solve_batch(hmpc_ctx* ctx, int64_t B,
                          const double* x_in, const double* x_lin, const double* x_ref,
                          const double* pf, const double* C, const double* mu,
                          double* u, double* x, double* obj, int32_t* status, int32_t* iters,
                          int reps, void* stream, double* ms);

#ifdef __cplusplus
}
#endif

#endif /* HMPC_H */
