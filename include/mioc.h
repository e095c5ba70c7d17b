/*
 * mioc.h -- C ABI of libmioc, the MI355X (gfx950) implementation of the reference's DP
 * trust-region subproblem.
 *
 * The reference (Julia, Jonas477/mixed-integer-optimal-control---algorithm-tools) has no FFI; the
 * entry points below are what a `ccall` glue for its hot path binds (INTEGRATION.md shows the Julia
 * stubs).  Each entry cites the reference interface it replaces.
 *
 * Conventions
 *   - every call returns an int32 status (MIOC_OK == 0, negative on error); no C++ exception
 *     crosses the ABI; mioc_last_error(ctx) returns a NUL-terminated description;
 *   - host arrays are borrowed for the duration of a synchronous call only, column-major
 *     (Julia layout): df[m + nx*i], u[m + nx*i], 0 <= m < nx, 0 <= i < nt;
 *   - a context owns all device memory (value fronts, the compact argmin table, level tables) and
 *     keeps the DP resident between mioc_bellman and mioc_backtrack, so the trust-region halving
 *     path (multi-trust.jl:108-110) costs only a backtrack;
 *   - a context is not thread-safe; distinct contexts may be used concurrently; every call first
 *     selects the context's device (HIP's current device is per host thread).
 */
#ifndef MIOC_H
#define MIOC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------------------------- */
#define MIOC_OK 0
#define MIOC_EINVAL -1      /* bad argument / shape */
#define MIOC_EINEXACT -2    /* |nu - u_old| not integral: the reference's InexactError,
                               HelpFunctions.jl:37,57 (convert(Int64, ...)) */
#define MIOC_ENOMEM -3      /* device allocation failed */
#define MIOC_EHIP -4        /* HIP runtime error */
#define MIOC_EINFEASIBLE -5 /* no finite value within the budget; the reference would read an
                               unwritten U cell at HelpFunctions.jl:116 */
#define MIOC_ESTATE -6      /* call order violated (e.g. backtrack before bellman, B_use > B) */
#define MIOC_ENONFINITE -7  /* non-finite gradient entry */
#define MIOC_ECOMPILE -8    /* the hook source did not compile; the log says why */

/* ---- switching-cost kinds: beta * (sum_m |nu_jm - nu_lm|^p)^(1/p), HelpFunctions.jl:63-67 ----- */
#define MIOC_P_INF 0    /* p = Inf: the reference evaluates (sum |d|^Inf)^(1/Inf) == x^0.0 == 1.0, so
                           every transition (including "no switch") costs beta.  Reproduced. */
#define MIOC_P_ONE 1    /* p = 1: weight = sum_m |d_m| (exact integer) */
#define MIOC_P_INTLUT 2 /* integer p >= 2: weight = table[sum_m |d_m|^p]; the host supplies Julia's
                           Float64(S)^(1/p) for S = 0..table_len-1 */
#define MIOC_P_TABLE 3  /* any p: weight = table[rank_l * L + rank_j] (L*L host-supplied weights) */

/* ---- algorithm selection (mioc_set_option(MIOC_OPT_ALGO, ...)) ----------------------------- */
#define MIOC_OPT_ALGO 1
#define MIOC_ALGO_AUTO 0    /* p=Inf -> class collapse; p=1, beta>0 on an 8^3 or 8^4 product grid ->
                               separable transform; small state (front fits one CU's LDS) -> fused;
                               other large product grids at p=1 -> pyramid; otherwise the generic
                               min-plus sweep */
#define MIOC_ALGO_GENERIC 1 /* per-step min-plus sweep over every (c, l, j): any p */
#define MIOC_ALGO_PINF 2    /* exact p=Inf collapse onto per-budget row minima */
#define MIOC_ALGO_PYRAMID 3 /* p=1 on product grids of consecutive levels: exact L1-ball pyramid */
#define MIOC_ALGO_SEPARABLE 4 /* p=1, beta>0, 8^3 / 8^4 product grid of consecutive levels: separable L1
                                 distance transform in exact fixed point with a certified argmin */
#define MIOC_ALGO_FUSED 5   /* whole DP of each subproblem in ONE workgroup with the value front in LDS
                               (any p; L <= 64, small B): the batch path for small-state problems */
#define MIOC_ALGO_FUSED_SEPARABLE 6 /* the fused DP with the separable L1 transform of MIOC_ALGO_SEPARABLE:
                                       p=1, beta>0, 2-D product grid of consecutive integer levels
                                       (6x6, 4x4, 8x8, 8x4), B < 512 */
#define MIOC_OPT_TIMING 2   /* 1: record HIP events around the dominant kernel (mioc_kernel_stats) */
#define MIOC_OPT_PERSIST 3  /* separable transform: 1 (default) runs the whole DP as one persistent launch
                               whose workgroups hand rows to each other; 0: one launch per step */
#define MIOC_OPT_PRED_FMA 4 /* mioc_pred*: 1 accumulates each ∇f[:,j]'(u_old[:,j] - u[:,j]) with fma, as an
                               FMA-contracted BLAS ddot does; 0 (default): products rounded, then added */
#define MIOC_OPT_SPIN_LIMIT 5 /* separable transform, persistent launch: polls a dependency wait may take
                                 before the launch is abandoned and the DP redone with per-step launches
                                 (default 2^24; a tiny value forces that fallback, for tests) */
#define MIOC_OPT_SDT_BUFFERS 6 /* persistent separable transform: staging buffers (4..256, default 256; more
                                  buffers let rows run further apart, which hides the row hand-off; cut to
                                  the most that keep a subproblem's staging region under 4 GiB; raised to
                                  7·M + 1 (29 on 8^4 grids): with fewer, a row's write-after-read wait can
                                  close a cycle with the one-row-ahead waits of the rows below it, so the DP
                                  would deadlock -- a problem where 7·M + 1 do not fit runs per step) */
#define MIOC_OPT_FSEP_SEGMENTS 7 /* fused separable DP: row segments per subproblem, each on its own workgroup
                                    (0, default: chosen from the batch size -- more than one only when the
                                    batch alone cannot fill the GPU; 1..8: forced; -1: the one-lane-per-row
                                    kernel of mioc_fused.hip) */
#define MIOC_OPT_PINF_WALK 8 /* p=Inf backtrack: 0 (default) the segmented walk -- one subproblem's path spread
                                over many workgroups -- for batches of at most 64 subproblems with >= 512 steps,
                                else one serial walk per subproblem; 1: segmented walk forced; -1: serial walk */
/* option 9 (a two-workgroups-per-row separable driver, opt-in and slower) was removed in round 6: MIOC_EINVAL */
#define MIOC_OPT_SDT_ROW_OWNER 10 /* persistent separable transform: 1 (default) runs the one-row driver
                                     (k_sdt_run1) when the plan gives every workgroup exactly one row (K·B
                                     rows on at least as many CUs); 0: always the general driver (k_sdt_run).
                                     Results and diagnostics are the same either way */

typedef struct mioc_ctx mioc_ctx;

const char *mioc_version(void);

/* Create / destroy a context on HIP device `device`. */
int32_t mioc_create(int32_t device, mioc_ctx **out);
int32_t mioc_destroy(mioc_ctx *ctx);
const char *mioc_last_error(const mioc_ctx *ctx);
int32_t mioc_set_option(mioc_ctx *ctx, int32_t option, int64_t value);

/*
 * Flattened admissible-level iterator: replaces `obj.𝓥` + `obj.iterator`
 * (product_iterator / bounded_sum_iterator, julia_opt/AdmissibleIterators.jl:9-49) as consumed by
 * bellman_TRM! (HelpFunctions.jl:29,49,60) and eval_u_TRM! (HelpFunctions.jl:104-118).
 *   counts[M]          |V_m|
 *   values[sum counts] level values, V_1 then V_2 ...
 *   tuples[L*M]        admissible tuples in iterator order, tuple-major, 1-based level indices
 * The iterator order must be the grid's column-major order filtered (both reference iterators are).
 */
int32_t mioc_set_levels(mioc_ctx *ctx, int64_t M, const int64_t *counts, const int64_t *values, int64_t L,
                        const int32_t *tuples);

/*
 * Switching cost: the `β` and `p` arguments of bellman_TRM! (HelpFunctions.jl:20, :63-67),
 * TRM_parameters.β / .p (multi-trust.jl:27-28).  p_int is p for MIOC_P_INTLUT; `table` as above.
 */
int32_t mioc_set_cost(mioc_ctx *ctx, int32_t p_kind, int64_t p_int, double beta, int64_t table_len,
                      const double *table);

/*
 * bellman_TRM!(∇f, u_old, B, β, p, Δt, nu, U, Φ, iterator)  -- HelpFunctions.jl:20-83,
 * called at multi-trust.jl:112.  U and Φ live in the context (device memory), not on the host:
 * the reference layout would be 2.21 TB for nt=65536, 4096 levels, B=256.
 * Host buffers df (∇f) and u_old: nx x nt column-major.  B = floor(Δ⁰/Δt) (multi-trust.jl:69).
 *
 * Accepted arguments: nx equal to the levels' number of controls, 1 <= K <= 4096 (batch entries),
 * 1 <= nt <= 2^30, 0 <= B <= 2^20, dt finite.  Within that range each algorithm has a budget limit of its own:
 *   MIOC_ALGO_PINF             B + 1 <= 7936 after rounding up to a multiple of 64 (B <= 7935), and at most 64
 *                              budget classes (max_l |nu_l - u_old|_1 <= 63 at every step);
 *   MIOC_ALGO_FUSED            (B + 1 rounded up to 64)/64 * L <= 192 and the front within one CU's 160 KiB of
 *                              LDS (B <= 3390 at L = 2, 3387 at L = 3, 2024 at L = 5);
 *   MIOC_ALGO_FUSED_SEPARABLE  B < 512;
 *   the others                 B <= 2^20, as far as device memory holds the tables.
 * MIOC_ALGO_AUTO takes another algorithm beyond such a limit; a forced algorithm returns MIOC_EINVAL.
 *
 * u_old: integral entries with |u_old| < 4e15 (else MIOC_EINEXACT).  A step whose u_old is further than B from every
 * level makes every cell +Inf, as in the reference: the call returns MIOC_OK and the backtrack reports
 * MIOC_EINFEASIBLE for that subproblem alone.  The context keeps its copy of u_old clamped, per component, to within
 * 1e8 of the level range; mioc_pred*'s tv_old of such a (necessarily infeasible) subproblem is that of the clamped copy.
 *
 * What a failed call leaves behind (mioc_bellman, mioc_bellman_batch_device and mioc_batch_multi alike):
 *   - A call rejected for its arguments (MIOC_EINVAL for nx, K, nt, B or dt, or a NULL pointer) changes nothing:
 *     the previous DP, its inputs and its last backtrack stay valid, and mioc_backtrack*, mioc_pred*,
 *     mioc_get_argmin_table and mioc_get_pinf_tables answer from them exactly as before the call.
 *   - A call that fails after that (MIOC_ENONFINITE, MIOC_EINEXACT, a forced algorithm that does not support the
 *     problem: MIOC_EINVAL from the algorithm's own check, MIOC_ENOMEM, MIOC_EHIP) has given up the previous DP
 *     and holds none: mioc_backtrack*, mioc_pred*, mioc_get_argmin_table and mioc_get_pinf_tables return
 *     MIOC_ESTATE until a bellman call succeeds.
 */
int32_t mioc_bellman(mioc_ctx *ctx, const double *df, const double *u_old, int64_t nx, int64_t nt, int64_t B,
                     double dt);

/*
 * eval_u_TRM!(u, u_old, U, Φ, B, nu)  -- HelpFunctions.jl:98-124, called at multi-trust.jl:110,113.
 * B_use <= B of the last mioc_bellman (the halving path reuses the DP, multi-trust.jl:108-110).
 * u_out: nx x nt column-major level values (obj.x); phi_star: the minimal Φ value (nullable);
 * switch_mask: nt bytes, switch_mask[i] = (u[:,i] != u[:,i-1]), switch_mask[0] = 0 (nullable).
 */
int32_t mioc_backtrack(mioc_ctx *ctx, int64_t B_use, double *u_out, double *phi_star, uint8_t *switch_mask);

/*
 * Batched, device-resident variants (inputs already in HBM; the bench and the multi-GPU batch
 * runner use these).  K independent subproblems sharing levels, cost, nt and B (random restarts):
 *   d_df, d_u_old : K x nx x nt (subproblem-major, each nx x nt column-major), device pointers
 *   d_u_out       : K x nx x nt device pointer;  d_phi_star: K doubles (device, nullable)
 *   d_status      : K int32 (device, nullable): per-subproblem MIOC_OK / MIOC_EINFEASIBLE
 * Work is enqueued on the context's stream; call mioc_synchronize before reading results.
 */
int32_t mioc_bellman_batch_device(mioc_ctx *ctx, int64_t K, const double *d_df, const double *d_u_old,
                                  int64_t nx, int64_t nt, int64_t B, double dt);
int32_t mioc_backtrack_batch_device(mioc_ctx *ctx, int64_t B_use, double *d_u_out, double *d_phi_star,
                                    int32_t *d_status);
/* The same with one budget per subproblem: d_B_use[k] (device, K int32, each 0 <= B_use[k] <= B) -- the
 * per-restart trust-region radii after halving (multi-trust.jl:108-110, B_new = floor(Δᵏ/Δt) per restart).
 * The budgets are validated on the device (no host read-back): a B_use[k] outside [0, B] makes d_status[k] =
 * MIOC_ESTATE and leaves subproblem k's u row NaN; the call itself returns MIOC_OK.  The first backtrack after a DP
 * whose workgroups hand rows to each other inside one launch (persistent separable DP, segmented fused separable
 * DP, segmented p=Inf recursion: small batches) synchronises the stream once, to read that DP's timeout word and
 * redo the DP if a wait timed out; later backtracks of the same DP enqueue without a synchronisation. */
int32_t mioc_backtrack_batch_budgets_device(mioc_ctx *ctx, const int32_t *d_B_use, double *d_u_out, double *d_phi_star,
                                            int32_t *d_status);
int32_t mioc_synchronize(mioc_ctx *ctx);

/*
 * The controls of the last backtrack as 0-based level ranks in iterator order (obj.iterator of
 * eval_u_TRM!, HelpFunctions.jl:110-118: u[:, i] = ν(l_i)): d_ranks_out receives K x nt int32 (device
 * pointer), enqueued on the context's stream.  The multi-GPU batch gathers these (one 16-bit rank per step
 * instead of nx level values) without recovering them from u.
 */
int32_t mioc_get_ranks_device(mioc_ctx *ctx, int32_t *d_ranks_out);

/*
 * Trust-region quantities of the last backtrack, multi-trust.jl:117-127 (pred) with TV_p of
 * HelpFunctions.jl:251-268 (p = the context's cost; p = Inf is the true max norm here, unlike the DP's cost):
 *   int_val = Δt · Σ_j ∇f[:,j]'(u_old[:,j] − u[:,j]);   tv_old = TV_p(u_old, p);   tv_new = TV_p(u, p)
 *   pred    = int_val + β·(tv_old − tv_new)
 * u is the path of the last mioc_backtrack*, ∇f and u_old those of the last mioc_bellman*.  All sums are
 * accumulated in the reference's loop order, so TV_p is bit-identical for p = 1, Inf and MIOC_P_INTLUT (the
 * summand is the host table's Julia pow) and int_val differs from the reference's BLAS dot only by its FMA use
 * (MIOC_OPT_PRED_FMA).  MIOC_P_TABLE needs both controls on the level grid (else MIOC_EINVAL).
 * Outputs are nullable.  mioc_pred: the single-subproblem (host) API, synchronous.
 * mioc_pred_batch_device: K values per output (device pointers), enqueued; errors surface at mioc_synchronize.
 */
int32_t mioc_pred(mioc_ctx *ctx, double *int_val, double *tv_old, double *tv_new, double *pred);
int32_t mioc_pred_batch_device(mioc_ctx *ctx, double *d_int_val, double *d_tv_old, double *d_tv_new, double *d_pred);

/* TV_p(u, p) of K device controls d_u (K x nx x nt, each column-major) into d_tv[K]; enqueued. */
int32_t mioc_tv_device(mioc_ctx *ctx, int64_t K, const double *d_u, int64_t nx, int64_t nt, double *d_tv);

/*
 * Device-resident TRM control (multi-trust.jl:92-163) for K restarts, so that the host reads back one flag per
 * inner-loop chunk instead of K decisions plus stream syncs per inner iteration:
 *   mioc_trm_state_bytes(K): bytes of the zero-initialised state block the caller allocates on the device
 *     (offset 0: gate word, 4: any-active word, 8: copy word; then K doubles Δᵏ, K doubles TV_old, K int32 k,
 *     K int32 flags (1 inner, 2 halved, 4 stopped), K int32 outer iterations per restart).
 *   mioc_trm_attach(ctx, d_state): while the gate word is 0, the kernels of mioc_backtrack_batch*_device,
 *     mioc_pred_batch_device, mioc_ode_eval_device, mioc_ode_program_eval_device (and _eval_mixed_device),
 *     mioc_rows_copy_device, mioc_heat_eval_device and mioc_conv_eval_device return at once; so does the kernel of
 *     mioc_tv_device and of the host mioc_pred, which then leave their outputs as they were (mioc_pred returns the
 *     stale words of its staging buffer): detach around a TV_p or a pred that must run whatever the gate says;
 *     NULL detaches.
 *   mioc_trm_outer_begin_device: multi-trust.jl:99-107 (TV_old = TV_p(u), Δᵏ = Δ⁰, k = 1, budgets = B, every
 *     restart not stopped enters its inner loop; the gate opens if any did).
 *   mioc_trm_inner_end_device: multi-trust.jl:117-158 for the restarts inside their inner loop: pred (with TV_old),
 *     ared, the decision (written to d_decision if not NULL: 0 accept, 1 halve, 2 stop, -1 not in the loop),
 *     obj.x = trial, accept / halve / stop, k += 1, the next budgets; the gate stays open while any restart is
 *     inside its inner loop.  n_per_restart = nt·nx doubles of u, u_old and trial per restart.
 *   mioc_trm_poll: synchronises the stream once and returns {gate, any-active}.
 */
int64_t mioc_trm_state_bytes(int64_t K);
int32_t mioc_trm_attach(mioc_ctx *ctx, void *d_state);
int32_t mioc_trm_outer_begin_device(mioc_ctx *ctx, int64_t K, void *d_state, const double *d_tv_u, double D0,
                                    int64_t B, int32_t *d_budgets);
int32_t mioc_trm_inner_end_device(mioc_ctx *ctx, int64_t K, void *d_state, double sigma, int64_t kmax, double tau,
                                  int64_t B, const double *d_int_val, const double *d_tv_new, const double *d_J_new,
                                  double *d_J_old, double *d_J, double *d_tv_u, int32_t *d_budgets,
                                  int32_t *d_decision, int64_t n_per_restart, const double *d_trial, double *d_u,
                                  double *d_u_old);
int32_t mioc_trm_poll(mioc_ctx *ctx, const void *d_state, int32_t *out);

/*
 * The trust-region step decision of multi-trust.jl:127-158 per subproblem, on the device:
 *   ared = J_old − J_new + β·(tv_old − tv_new);   decision = 2 if pred <= 0 (stop: optimal),
 *   1 if ared < σ·pred (bad step: halve Δ), else 0 (good step: accept).  d_ared nullable; enqueued.
 */
int32_t mioc_trm_decide_device(mioc_ctx *ctx, int64_t K, const double *d_J_old, const double *d_J_new,
                               const double *d_tv_old, const double *d_tv_new, const double *d_pred, double sigma,
                               double *d_ared, int32_t *d_decision);

/*
 * Multi-device batch from one process (SURVEY §8 b, `mioc_batch_multi`): K subproblems in host arrays (K x nx x nt,
 * each nx x nt column-major) are split into contiguous blocks over the nctx contexts -- one per device, each with
 * the same levels and cost already set -- and every block is solved on its context's device from its own host
 * thread: bellman_TRM! at B, then eval_u_TRM! at B_use (<= B).  u_out: K x nx x nt; phi_star, status: K entries
 * (nullable).  Synchronous.  On error the return is the first failing context's status, and
 * mioc_last_error(ctxs[0]) names that context.  (For one process per GPU over RCCL see INTEGRATION.md.)
 */
int32_t mioc_batch_multi(mioc_ctx *const *ctxs, int32_t nctx, int64_t K, const double *df, const double *u_old,
                         int64_t nx, int64_t nt, int64_t B, double dt, int64_t B_use, double *u_out, double *phi_star,
                         int32_t *status);

/*
 * The ODE gradient producer of the reference's TRM examples, batched on the device:
 * eval_f! / eval_df! of julia_opt/ODEObjective.jl:125-184 (explicit Euler forward, trapezoid cost, explicit-Euler
 * adjoint, df = Gu - Fu'λ) with the hooks of example_fishing.jl / example_doubletank.jl / example_vanderpol.jl.
 * d_x: K x nx x nt controls (nx = 3, the DP's input layout); d_J: K objective values (nullable); d_df: K x nx x nt
 * gradients (nullable), ready for mioc_bellman_batch_device.  τ = (T1 - T0) / nt.  params (nullable: the examples'
 * values) holds, in order: fishing α, β, γ, δ, c1, c2, v1[3], v2[3], y0[2] (14); doubletank k1, k2, c[3], y0[2] (7);
 * vanderpol c[3], y0[2] (5).  Enqueued on the context's stream.
 */
#define MIOC_ODE_FISHING 1
#define MIOC_ODE_DOUBLETANK 2
#define MIOC_ODE_VANDERPOL 3
int32_t mioc_ode_eval_device(mioc_ctx *ctx, int32_t problem, int64_t K, const double *d_x, int64_t nx, int64_t nt,
                             double T0, double T1, const double *params, int32_t nparams, double *d_J, double *d_df);

/*
 * User-defined ODE objectives: the reference's extension point (a subclass of AbstractODEObjective with the hooks
 * F!, Fy!, Fu!, G, Gy!, Gu!, julia_opt/ODEObjective.jl:243-248) for problems other than the three above.  The caller
 * hands the six hooks over as HIP source text; the library compiles them into its explicit-Euler / adjoint sweep for
 * gfx950 at run time (hiprtc) and launches that kernel: min ∫ G(t, y, u) dt  s.t.  y' = F(t, y, u), y(T0) = state0,
 * with ny states, nx controls (the DP's discrete ones; with "Mixed controls" below, nu continuous ones in front of
 * them) and nparams parameters.
 *
 * Hook contract.  The text is compiled as HIP C++ in front of the kernel; NY, NX and NP (= ny, nx, nparams) are
 * defined as macros before it.  It may define helper __device__ functions, and it defines exactly these six:
 *
 *   __device__ void   F (const double *p, int i, double t, const double *y, const double *x, double *f);
 *   __device__ void   Fy(const double *p, int i, double t, const double *y, const double *x, double (*fy)[NY]);
 *   __device__ void   Fu(const double *p, int i, double t, const double *y, const double *x, double (*fu)[NX]);
 *   __device__ double G (const double *p, int i, double t, const double *y, const double *x);
 *   __device__ void   Gy(const double *p, int i, double t, const double *y, const double *x, double *gy);
 *   __device__ void   Gu(const double *p, int i, double t, const double *y, const double *x, double *gu);
 *
 *   p: the NP parameters; y: the NY states; x: the NX controls of one time step; t = T0 + i*tau, tau = (T1 - T0)/nt.
 *   F  writes the right-hand side f[r] = F_r(t, y, x), every entry (f is uninitialised);
 *   Fy writes fy[r][c] = dF_r/dy_c;  Fu writes fu[r][m] = dF_r/dx_m;  G returns the running cost;
 *   Gy writes gy[c] = dG/dy_c;  Gu writes gu[m] = dG/dx_m.
 *   fy, fu, gy and gu are zeroed once per evaluation and not between calls (ODEObjective.jl:155-162): a hook may
 *   write only the entries that are not structurally zero, but an entry it writes in one call it writes in all.
 *   Hooks must not touch memory other than their arguments, and they must not write p, y or x.
 *
 * The step index i takes exactly the values the reference passes (0-based here; y_j = the state after j steps,
 * y_0 = state0; x_j = column j of the control):
 *   F   F(i, y_i, x_i) for i = 0..nt-1                                     (the Euler step y_{i+1} = y_i + tau*f)
 *   G   G(0, y_0, x_0) with weight 1/2, then G(i+1, y_{i+1}, x_{i+1}) for i = 0..nt-2, then G(nt-1, y_nt, x_{nt-1})
 *       with weight 1/2 -- the running cost may depend on the control        (ODEObjective.jl:130-146)
 *   Gy  Gy(nt, y_nt, x_{nt-1}) at the terminal, then Gy(i, y_i, x_i) for i = nt-1..1
 *   Fy  Fy(i, y_i, x_i) for i = nt-1..1
 *   Fu, Gu  (i, y_i, x_i) for i = 0..nt-1
 *
 * Rounding order (compiled with -ffp-contract=off and without fast-math, like the library; every sum left to right):
 *   forward    y_r = y_r + tau*f_r;  fval = 0.5*G(0, ..), then fval = fval + G or fval + 0.5*G (last);  J = fval*tau
 *   terminal   lam_r = (-0.5*tau)*gy_r
 *   adjoint    a_c = fy[0][c]*lam[0] + fy[1][c]*lam[1] + ...;  lam_c = lam_c + tau*(a_c - gy_c), all a before any lam
 *   gradient   df[m, i] = (0.0 - (fu[0][m]*lam[0] + fu[1][m]*lam[1] + ...)) + gu[m]
 * For ny = 2, nx = 3 and Gu = 0 this is the order of the built-in examples, so hooks that restate an example term for
 * term reproduce the example's J and df bit for bit.
 *
 * Integrators.  All of the above is the reference's scheme, MIOC_ODE_INT_EULER, which mioc_ode_program_create
 * compiles.  mioc_ode_program_create_ex also offers MIOC_ODE_INT_HEUN (c = (0, 1), a21 = 1, b = (1/2, 1/2)) and
 * MIOC_ODE_INT_RK4 (c = (0, 1/2, 1/2, 1), a21 = a32 = 1/2, a43 = 1, b = (1/6, 1/3, 1/3, 1/6)), each with
 * m = `substeps` steps of h = tau/m inside every control interval.  The reference has no such scheme; it is defined
 * here.  Substep n = i*m + j (i = 0..nt-1 the control interval, j = 0..m-1) starts at t_n = T0 + n*h with the state
 * y_n, y_0 = state0; the control x_i is held over the whole interval i.  With S stages:
 *   forward    Y_1 = y_n,  Y_s = y_n + (h*a_{s,s-1})*k_{s-1};  k_s = F(i, t_n + c_s*h, Y_s, x_i),
 *              g_s = G(i, t_n + c_s*h, Y_s, x_i);  y_{n+1} = y_n + sum_s (h*b_s)*k_s.  The running cost is a
 *              quadrature state: q_0 = 0, q_{n+1} = q_n + sum_s (h*b_s)*g_s, and J = q_{nt*m} -- not the
 *              reference's trapezoid: G sees the control of its own interval.
 *   gradient   the exact derivative of that J by the scheme's discrete adjoint.  w = 0 after the last substep; per
 *              substep n = nt*m-1..0, with the stage states Y_s recomputed from the stored y_n, for s = S..1:
 *                kbar_s = (h*b_s)*w + (h*a_{s+1,s})*Ybar_{s+1}              (s = S: kbar_S = (h*b_S)*w)
 *                Ybar_s = Fy(Y_s)' kbar_s + (h*b_s)*Gy(Y_s),   xbar_i += Fu(Y_s)' kbar_s + (h*b_s)*Gu(Y_s)
 *              then w = w + sum_s Ybar_s.  df[m, i] = xbar_i[m] / tau: the function-space scaling of the reference's
 *              df (the directional derivative of J along d is tau * sum df.*d), so df feeds the DP unchanged.
 *   hooks      every hook sees i = the control interval, t = the stage time t_n + c_s*h, y = the stage state Y_s and
 *              x = x_i.  F and G: every stage of every substep, forward; F again for the stages 1..S-1 in the
 *              backward sweep; Fy, Gy, Fu, Gu (in this order): every stage, s = S..1, of every substep backwards.
 *              fy, fu, gy, gu are zeroed once per evaluation, as above.
 *   rounding   tau = (T1 - T0)/nt, h = tau/m, t_n = T0 + (double)n*h, stage time t_n + (c_s*h); the products c_s*h,
 *              a_{s,s-1}*h, b_s*h are rounded once (b: the doubles 1.0/6.0, 1.0/3.0, 0.5); every sum left to right:
 *                Y_s[r] = y[r] + (a_s h)*k_{s-1}[r];  y[r] = y[r] + (((b_1 h)*k_1[r] + (b_2 h)*k_2[r]) + ...)
 *                q = q + (((b_1 h)*g_1 + (b_2 h)*g_2) + ...);  J = q
 *                kbar_s[r] = (b_s h)*w[r] + (a_{s+1} h)*Ybar_{s+1}[r]
 *                Ybar_s[c] = ((fy[0][c]*kbar_s[0] + fy[1][c]*kbar_s[1]) + ...) + (b_s h)*gy[c]
 *                xbar[m] = xbar[m] + (((fu[0][m]*kbar_s[0] + fu[1][m]*kbar_s[1]) + ...) + (b_s h)*gu[m]), xbar = 0.0
 *                at the start of an interval's backward sweep;  w[c] = w[c] + ((Ybar_S[c] + Ybar_{S-1}[c]) + ...)
 *                df[m, i] = xbar[m] / tau
 *   scratch    with d_df the state at every substep start is stored: K * nt * m * ny doubles of the context's ODE
 *              scratch, grown on demand (MIOC_ENOMEM if that fails); a value-only call (d_df NULL) stores nothing.
 *
 * Implicit integrators.  MIOC_ODE_INT_BEULER (backward Euler: theta = 1, order 1, L-stable) and MIOC_ODE_INT_MIDPOINT
 * (the implicit midpoint rule: theta = 1/2, order 2, A-stable) are for dynamics with fast decaying modes, where an
 * explicit scheme's substep is bounded by stability and not by accuracy.  The reference has no such scheme for its ODE
 * family; it is defined here.  The grid is the one above (h = tau/m, substep n = i*m + j, x_i held over interval i);
 * every hook sees i = the control interval and t = the stage time t_s = (T0 + n*h) + theta*h.
 *   forward    the stage slope k solves k = F(t_s, Y, x_i) with the stage state Y = y_n + (theta*h)*k; then
 *              y_{n+1} = y_n + h*k, q_{n+1} = q_n + h*G(t_s, Y, x_i), q_0 = 0 and J = q_{nt*m} (a quadrature cost, as
 *              for Heun / RK4).
 *   Newton     k = F(t_s, y_n, x_i) to start, then at most MIOC_ODE_NEWTON_MAX = 12 times: Y = y_n + (theta*h)*k;
 *              r = F(Y) - k;  A = I - (theta*h)*Fy(Y);  solve A*delta = r;  k = k + delta.  The iteration stops after
 *              the update for which every component r has |delta_r| <= MIOC_ODE_NEWTON_TOL * max(1, max_r |k_r|)
 *              (1e-10, k the updated slope) and a finite k_r; the comparison is made component by component, so a
 *              NaN fails it.  The update is quadratic: the accepted k is converged to rounding.  Y, G and y_{n+1}
 *              are then taken from the accepted k.
 *   failure    a substep whose iteration has not stopped after MIOC_ODE_NEWTON_MAX updates (no real root, a singular
 *              A through its non-finite delta, non-finite hooks) fails its restart: that restart's J and every entry
 *              of its df row are NaN, no other restart is affected, and the call returns MIOC_OK (the kernel is
 *              asynchronous); the next mioc_bellman_* that is given the row reports MIOC_ENONFINITE.  The iteration
 *              is capped, so the launch always ends.
 *   solve      dense Gaussian elimination in registers, A and the right-hand side b overwritten.  For each column
 *              c = 0..ny-1: for each r = c+1..ny-1 in turn, rows r and c (of A from column c on, and of b) change
 *              places if |A[r][c]| > |A[c][c]| (partial pivoting by conditional swaps); then for each r > c:
 *              f = A[r][c] / A[c][c] (the IEEE quotient), A[r][e] = A[r][e] - f*A[c][e] for e > c, b[r] = b[r] - f*b[c].
 *              Back substitution for r = ny-1..0, the sum left to right:
 *              delta[r] = ((b[r] - A[r][r+1]*delta[r+1]) - A[r][r+2]*delta[r+2] - ...) / A[r][r].
 *   gradient   the exact derivative of that J by the implicit function theorem; no Newton and no F call.  w = 0 after
 *              the last substep; per substep n = nt*m-1..0, with Fy, Gy, Fu, Gu at the stored stage state Y:
 *                kbar = h*w + ((theta*h)*h)*Gy;   solve (I - (theta*h)*Fy)' mu = kbar   (the solve above);
 *                xbar_i += Fu' mu + h*Gu;   w = w + (Fy' mu + h*Gy);   df[m, i] = xbar_i[m] / tau as above.
 *              A singular transposed matrix makes w, and with it the df columns of that and all earlier intervals, NaN.
 *   hooks      F at (t_s, y_n) once per substep, then F and Fy at (t_s, Y) once per Newton update, G at the accepted
 *              Y, forward; Fy, Gy, Fu, Gu at the stored Y of every substep backwards.  fy is zeroed once per evaluation
 *              before the forward sweep, fu, gy and gu once before the backward sweep.
 *   rounding   theta*h and (theta*h)*h are rounded once; t_s = (T0 + (double)n*h) + theta*h; every sum left to right:
 *                Y[r] = y[r] + (theta h)*k[r];  r[r] = f[r] - k[r];  A[r][c] = (r == c ? 1.0 : 0.0) - (theta h)*fy[r][c]
 *                k[r] = k[r] + delta[r];  q = q + h*G;  y[r] = y[r] + h*k[r];  J = q
 *                kbar[r] = h*w[r] + ((theta h) h)*gy[r];  A'[r][c] = (r == c ? 1.0 : 0.0) - (theta h)*fy[c][r]
 *                xbar[m] = xbar[m] + (((fu[0][m]*mu[0] + fu[1][m]*mu[1]) + ...) + h*gu[m])
 *                w[c] = w[c] + (((fy[0][c]*mu[0] + fy[1][c]*mu[1]) + ...) + h*gy[c]);  df[m, i] = xbar[m] / tau
 *   scratch    with d_df the stage state Y of every substep is stored, the same K * nt * m * ny doubles as above; a
 *              value-only call stores nothing.
 *
 * Derived hooks.  mioc_ode_program_create_ad(..., derive, ...) generates the hooks named by the bits of `derive`
 * (MIOC_ODE_DERIVE_FY / _FU / _GY / _GU) from F and G by forward-mode automatic differentiation, for every
 * integrator; derive == 0 is mioc_ode_program_create_ex, the assembled source byte for byte.  With derive != 0 the
 * text defines F and G as templates over the scalar type,
 *   template <class T> __device__ void F(const double *p, int i, double t, const T *y, const T *x, T *f);
 *   template <class T> __device__ T    G(const double *p, int i, double t, const T *y, const T *x);
 * and so every helper that takes y or x.  The skeletons call them with T = double as before: the same expressions,
 * so J is what the non-template text gives, bit for bit.  A generated hook is an ordinary __device__ function with
 * the signature above, placed between the caller's text and the skeleton; it calls F or G once with
 * T = mioc_ad::Dual<N> (a value v and N tangents d[0..N-1], all in registers):
 *   Fy, Gy  N = ny; y[r] = (y_r, e_r), the r-th unit tangent; x[m] = (x_m, 0).  fy[r][c] = f[r].d[c], gy[r] = G.d[r]
 *   Fu, Gu  N = nx; x[m] = (x_m, e_m); y[r] = (y_r, 0).                        fu[r][m] = f[r].d[m], gu[m] = G.d[m]
 * and writes every entry of its output (a structural zero too).  The hooks not in `derive` are the caller's, their
 * contract unchanged.  For every derived hook the head #defines MIOC_DERIVE_FY / _FU / _GY / _GU as 1 (none with
 * derive == 0), so one text may carry hand-written hooks under `#ifndef MIOC_DERIVE_FY ... #endif` and serve any
 * mask.  A hook both defined by hand and named in `derive` is a redefinition, a non-template F or G cannot be called
 * with a Dual: both return MIOC_ECOMPILE with the compiler's message in the log.  The assembled text is the head with
 * the MIOC_DERIVE_* macros, the dual type under `#line 1 "mioc_ad"`, the caller's text under `#line 1 "hooks"` (its
 * diagnostics keep its own line numbers; the 1 MiB limit is the caller's text alone), the generated hooks under
 * `#line 1 "mioc_ad_hooks"`, the skeleton under `#line 1 "mioc_ode_program_skeleton"` (what all integrators share,
 * then the integrator's kernel).  The namespace mioc_ad exists only with derive != 0.  mioc_ode_program_source returns
 * this text.
 *   A generated hook is inlined at each of its call sites like a hand-written one (Heun / RK4: one per stage).  If
 *   the kernel then needs more than the 256 architectural VGPRs (the compiler reports AGPRs in use or vector spills),
 *   the text is compiled a second time with the generated hooks as functions that are called (the head then also
 *   #defines MIOC_AD_NOINLINE): one body each, the same operations in the same order, so J and df do not change;
 *   the log then starts with a line "mioc_ad: ... compiled as functions".
 *   Dual<N> supports: implicit construction and assignment from double (all tangents 0.0); unary + and -;
 *   + - * / and += -= *= /= for Dual o Dual, Dual o double, double o Dual (op= with a Dual on the left); the six
 *   comparisons in the same three forms, on the values; sqrt exp log sin cos tan tanh atan fabs; pow(Dual, double),
 *   pow(Dual, Dual); fmin, fmax (Dual, Dual), (Dual, double), (double, Dual); mioc_ad::value(a), the value of a
 *   double or a Dual.  An integer literal converts like a double.
 *   Tangent rules, for every k = 0..N-1 (v: the result's value, c: a double operand, which is never promoted to a
 *   Dual -- its rule has no term for it; every sum left to right, no contraction, each line as written):
 *     +a          d[k] = a.d[k]                        -a        v = -a.v; d[k] = -a.d[k]
 *     a + b       d[k] = a.d[k] + b.d[k]               a + c, c + a   d[k] = a.d[k]
 *     a - b       d[k] = a.d[k] - b.d[k]               a - c     d[k] = a.d[k];      c - a   d[k] = -a.d[k]
 *     a * b       d[k] = a.d[k]*b.v + a.v*b.d[k]       a * c     d[k] = a.d[k]*c;    c * a   d[k] = c*a.d[k]
 *     a / b       v = a.v/b.v; d[k] = (a.d[k] - v*b.d[k])/b.v
 *     a / c       d[k] = a.d[k]/c                      c / a     v = c/a.v; d[k] = (-(v*a.d[k]))/a.v
 *     a op= b     a = a op b
 *     sqrt(a)     v = sqrt(a.v); d[k] = a.d[k]/(2.0*v)
 *     exp(a)      v = exp(a.v);  d[k] = a.d[k]*v       log(a)    d[k] = a.d[k]/a.v
 *     sin(a)      d[k] = a.d[k]*cos(a.v)               cos(a)    d[k] = a.d[k]*(-sin(a.v))
 *     tan(a)      v = tan(a.v);  d[k] = a.d[k]*(1.0 + v*v)
 *     tanh(a)     v = tanh(a.v); d[k] = a.d[k]*(1.0 - v*v)
 *     atan(a)     d[k] = a.d[k]/(1.0 + a.v*a.v)
 *     fabs(a)     d[k] = a.v < 0.0 ? -a.d[k] : a.d[k]
 *     pow(a, c)   v = pow(a.v, c); d[k] = (c*pow(a.v, c - 1.0))*a.d[k]
 *     pow(a, b)   v = pow(a.v, b.v); d[k] = (b.v*pow(a.v, b.v - 1.0))*a.d[k] + (v*log(a.v))*b.d[k]
 *     fmin(a, b)  b.v < a.v ? b : a;   fmax(a, b)  b.v > a.v ? b : a   (a tie, and a NaN, take the first argument;
 *                 a double that is taken has the tangents 0.0)
 *   No product is ever folded because a tangent is zero: the build has no fast-math, and 0.0*v is not 0.0 for a
 *   negative or non-finite v, so the constant argument's zero tangents are multiplied and added like any other.
 *   Singular points propagate Inf or NaN as the hand-written -1/(2*sqrt(y)) does: sqrt at 0, log at 0, a / b at
 *   b.v = 0, pow of a negative base with a Dual exponent (log of the base), pow(a, c) at a.v = 0 with c < 1; with
 *   a.v = 0 and a.d[k] = 0 such a rule gives 0.0/0.0 or 0.0*Inf = NaN where the derivative's limit may exist.
 *
 * Terminal cost, sampled data, state output.  mioc_ode_program_create_bolza(..., ndata, ..., derive, flags, ...) widens
 * the problem class to  min ∫ G(t, y, u, d(t)) dt + E(T1, y(T1))  s.t.  y' = F(t, y, u, d(t))  and hands the state
 * trajectory back.  Each part is compiled in only when asked for: the head then #defines ND (= ndata, when > 0),
 * MIOC_TERMINAL 1 (flag MIOC_ODE_TERMINAL) and MIOC_STATES 1 (flag MIOC_ODE_STATES) behind NY / NX / NP.  With
 * ndata == 0 and flags == 0 the head is _create_ad's byte for byte and the skeletons preprocess to the same tokens, so
 * such a program is the program it was.  mioc_ode_program_create_ad(...) is _bolza(ndata = 0, flags = 0).
 *   data       d_data is nt x ndata doubles on the device, [i][e], 0 <= ndata <= 16: shared by all restarts and
 *              piecewise constant on the control grid, like x.  The hook signatures do not change.  With ND > 0 the
 *              p a hook receives has NP + ND entries: p[0..NP-1] the parameters, p[NP + e] = data[c][e], where c is
 *              the control column whose x the hook is given:
 *                Euler    column i for F(i, y_i, x_i);  column i+1 for G(i+1, y_{i+1}, x_{i+1});  column nt-1 for the
 *                         last half-weight G and for the terminal Gy(nt, y_nt, x_{nt-1});  column i for everything in
 *                         the backward sweep (Fu, Gu, Gy, Fy at (i, y_i, x_i)).
 *                Heun, RK4, backward Euler, midpoint   column i = the control interval, for every stage and substep,
 *                         forward and backward.
 *              p is never differentiated, so derived hooks need no change.  The kernel reads the row straight from
 *              global memory; the row index is the same for every lane and the pointer is restrict-qualified, so
 *              the rows are scalar loads: d_data must not overlap d_J, d_df or d_Y.
 *   terminal   with MIOC_ODE_TERMINAL the text also defines
 *                __device__ double E (const double *p, double t, const double *y);
 *                __device__ void   Ey(const double *p, double t, const double *y, double *ey);   ey[c] = dE/dy_c
 *              or, with MIOC_ODE_DERIVE_EY (valid only with MIOC_ODE_TERMINAL; the head #defines MIOC_DERIVE_EY 1, for
 *              an `#ifndef MIOC_DERIVE_EY` guard like the other four),
 *                template <class T> __device__ T E(const double *p, double t, const T *y);
 *              and Ey is generated with mioc_ad::Dual<NY> (ey[r] = E.d[r], every entry written).  E and Ey are called
 *              once each, at the last state y_nt (Euler) or y_{nt*m}, with the data of column nt-1 and t the end time
 *              as the skeleton forms it: Euler T0 + (double)nt*tau, the other schemes T0 + (double)(nt*m)*h.  ey is
 *              zeroed once per evaluation, like gy.  A text without E fails to compile under "hooks:N".
 *   rounding   Euler: J = fval*tau + E (one product, one sum);  terminal lam_r = (-0.5*tau)*gy_r - ey_r.
 *              Heun, RK4, backward Euler, midpoint: J = q + E;  the backward sweep starts from w_r = ey_r in place of
 *              0.0.  Nothing else in the orders above changes.
 *   states     with MIOC_ODE_STATES the kernel takes one more pointer, d_Y: K x (nt+1) x ny doubles, [k][i][r], the
 *              state at the control-grid points t_i = T0 + i*tau, i = 0..nt (Euler: y_i; the other schemes: y_{i*m});
 *              row 0 is state0.  Substep and stage states are not output.  It is written in the forward sweep when
 *              d_Y is not NULL, whether or not d_J and d_df are given.  A restart whose Newton iteration fails
 *              (implicit schemes) has all its rows NaN.  The context's scratch and its layout are as before.
 *   MIOC_EINVAL from _bolza: ndata outside 0..16, flag bits other than the two, MIOC_ODE_DERIVE_EY without
 *              MIOC_ODE_TERMINAL (and every case of _create_ad).
 * mioc_ode_program_eval_bolza_device is the body of the two eval entries with d_data and d_Y: nu == 0 applies the
 *   check of mioc_ode_program_eval_device (nx == the levels' M), nu >= 1 that of _eval_mixed_device.  MIOC_EINVAL also
 *   for ndata > 0 with d_data NULL and for d_Y on a program without MIOC_ODE_STATES; d_data is ignored with
 *   ndata == 0.  The two older entries refuse a program with ndata > 0 (MIOC_EINVAL) and work as before on one with
 *   the terminal or the states flag and ndata == 0 (no state output).  Gate, stream and scratch growth as there.
 *
 * Scenarios.  mioc_ode_program_create_scen(..., flags, scen, ...) lets the restarts of one call solve different
 * problems: a scenario is one triple (state0, params, data), and a program compiled for scenarios is evaluated with S
 * of them.  The lane of restart q solves scenario q % S, where q is the restart index k, or j*K + k for the K*R
 * candidates of a fan: with K a multiple of S, restart k and each of its line-search candidates see scenario k % S,
 * and K = S*m gives m starts on each of S problems in one call.  The head #defines MIOC_SCEN 1 (scen bit
 * MIOC_ODE_SCEN) and MIOC_SCEN_DATA 1 (bit MIOC_ODE_SCEN_DATA) behind MIOC_STATES; with scen == 0 the head is
 * _create_bolza's byte for byte and the skeletons preprocess to the same tokens, so such a program is the program it
 * was.  mioc_ode_program_create_bolza(...) is _scen(..., scen = 0, ...).
 *   MIOC_ODE_SCEN       state0 and the parameters are per scenario.  The kernel takes `int S, const double *Y0S, const
 *              double *PS` in place of the by-value state0 and parameters, device arrays with the scenario index
 *              fastest, like the state scratch: d_state0[r*S + s] (ny x S doubles), d_params[e*S + s] (nparams x S;
 *              NULL is allowed with nparams == 0).  Each lane computes s = q % S once and loads its parameters once
 *              into its own copy of p (NP + ND doubles, the copy that ND > 0 already makes), its state0 at the start of
 *              the forward sweep and again for row i = 0 of Euler's backward sweep; with S >= 64 the 64 lanes of a
 *              wave load 64 contiguous doubles.  d_data stays the shared nt x ndata table, read by scalar loads.
 *   MIOC_ODE_SCEN_DATA  (only with MIOC_ODE_SCEN and ndata > 0) the data rows are per scenario as well:
 *              d_data[(c*ndata + e)*S + s], nt x ndata x S doubles, and every lane loads its own row of column c
 *              (ndata vector loads) wherever the shared row was loaded; the columns are those listed under "data".
 *   The arrays are restrict-qualified: they must not overlap d_J, d_df, d_Y or the context's scratch.  The hook
 *   signatures, the hook contract, every rounding order above and the generated hooks do not change (p is still never
 *   differentiated): restart q computes bit for bit what a program without scenarios computes from scenario q % S's
 *   values.  Row 0 of d_Y[q] is scenario q % S's state0.  The bounds of a mixed control stay shared.
 *   MIOC_EINVAL from _create_scen (and _source_scen): scen bits outside 3, scen == MIOC_ODE_SCEN_DATA alone,
 *              MIOC_ODE_SCEN_DATA with ndata == 0 (and every case of _create_bolza).
 * mioc_ode_program_eval_scen_device is the body of mioc_ode_program_eval_bolza_device (the same nu checks, gate, stream
 *   and scratch growth) with S and the device arrays above.  MIOC_EINVAL also for S < 1, K not a multiple of S, d_state0
 *   NULL, d_params NULL with nparams > 0, d_data NULL with ndata > 0, and a program compiled with scen == 0.  The three
 *   older eval entries refuse a scenario program (MIOC_EINVAL).  A refused call leaves the context usable.
 *
 * Sensitivities.  mioc_ode_program_create_sens(..., scen, sens, ...) makes the gradient of J in the numbers the caller
 * put into params and state0 an output of an evaluation: sens bit MIOC_ODE_SENS_P for dJ/dparams, MIOC_ODE_SENS_Y0 for
 * dJ/dstate0.  The head #defines MIOC_SENS <sens> behind MIOC_SCEN* only when sens != 0; every piece of the skeleton
 * that serves it is a macro that is empty without it, so with sens == 0 the text is _create_scen's byte for byte and
 * such a program is the program it was.  mioc_ode_program_create_scen(...) is _sens(..., sens = 0, ...).  The four
 * integrators with an exact discrete adjoint carry it; MIOC_ODE_INT_EULER does not: the reference scheme's df is its
 * own adjoint formula and not the derivative of its trapezoid J, so a parameter gradient consistent with it is not
 * defined (sens != 0 with Euler is MIOC_EINVAL).
 *   outputs    the kernel takes two more pointers behind d_Y: d_Jp, K x nparams doubles [k][e] = dJ_k/dp_e, and d_Jy0,
 *              K x ny doubles [k][r] = dJ_k/dstate0_r.  Plain derivatives: no division by tau.  Only the nparams
 *              parameters are differentiated; the data entries p[NP + e] are not.  With scenarios restart q's rows are
 *              the derivatives in scenario q % S's own parameters and state0.  A restart whose Newton iteration fails
 *              (implicit schemes) has NaN in both rows, no other restart is affected.  They must not overlap the
 *              other arrays.
 *   sweep      the backward sweep runs when any of d_df, d_Jp, d_Jy0 is given: the forward sweep stores its states and
 *              the scratch is grown under the same condition; df is stored only with d_df.  After the sweep the vector
 *              w the adjoint carries is dJ/dstate0.  dJ/dparams is one more accumulator beside xbar, pbar, which is
 *              never reset between intervals.  With both pointers NULL J, df and Y are the sens == 0 program's bit for
 *              bit, and df does not change when d_Jp or d_Jy0 is added.
 *   hooks      with MIOC_ODE_SENS_P the text also defines (unless derived)
 *                __device__ void Fp(const double *p, int i, double t, const double *y, const double *x, double (*fp)[NP]);
 *                __device__ void Gp(const double *p, int i, double t, const double *y, const double *x, double *gp);
 *                __device__ void Ep(const double *p, double t, const double *y, double *ep);     MIOC_ODE_TERMINAL only
 *              fp[r][e] = dF_r/dp_e, gp[e] = dG/dp_e, ep[e] = dE/dp_e, e < NP.  fp, gp and ep are zeroed once per
 *              evaluation like fu and gu: an entry written once is written always.  Fp and Gp are called only when d_Jp
 *              is given, after Fy, Gy, Fu, Gu (in this order: Fy, Gy, Fu, Gu, Fp, Gp) with the same (i, t, y, x) and the
 *              same data row: every stage s = S..1 of every substep backwards (Heun, RK4), the stored stage state of
 *              every substep backwards (backward Euler, midpoint).  Ep is called once when d_Jp is given, after Ey, at
 *              the last state with the data of column nt-1 and the end time t that E sees.
 *   derived    the derive bits MIOC_ODE_DERIVE_FP / _GP / _EP (only with MIOC_ODE_SENS_P; _EP only with
 *              MIOC_ODE_TERMINAL; none is part of MIOC_ODE_DERIVE_ALL) generate Fp, Gp, Ep by forward-mode AD.  A
 *              function named by one of them (F by _FP, G by _GP, E by _EP) is a template over the state type and the
 *              parameter type,
 *                template <class T, class P> __device__ void F(const P *p, int i, double t, const T *y, const T *x, T *f);
 *                template <class T, class P> __device__ T    G(const P *p, int i, double t, const T *y, const T *x);
 *                template <class T, class P> __device__ T    E(const P *p, double t, const T *y);
 *              and so every helper that takes p.  The skeleton and the other generated hooks call it with P = double
 *              as before: the same expressions, the same bits.  The generated Fp / Gp / Ep call it once with
 *              P = T = mioc_ad::Dual<NP>: p[e] = (p_e, e-th unit tangent) for e < NP; the data entries p[NP + e], y and
 *              x carry zero tangents; every output entry is written.  The head #defines MIOC_DERIVE_FP / _GP / _EP 1
 *              for `#ifndef` guards; a hook both written by hand and derived is MIOC_ECOMPILE; the second
 *              (MIOC_AD_NOINLINE) compile applies to them too.  The dual type needs no new rule.
 *   rounding   every sum left to right, no contraction; pbar[e] = 0.0 at the start of the sweep, or ep[e] with
 *              MIOC_ODE_TERMINAL and d_Jp;
 *                Heun / RK4, stage s:  pbar[e] = pbar[e] + (((fp[0][e]*kbar_s[0] + fp[1][e]*kbar_s[1]) + ...) + (b_s h)*gp[e])
 *                theta schemes:        pbar[e] = pbar[e] + (((fp[0][e]*mu[0] + fp[1][e]*mu[1]) + ...) + h*gp[e])
 *                after substep 0:      d_Jp[k*NP + e] = pbar[e];   d_Jy0[k*NY + r] = w[r]
 *   MIOC_EINVAL from _create_sens and _source_sens: sens bits outside 3; sens != 0 with MIOC_ODE_INT_EULER;
 *              MIOC_ODE_SENS_P with nparams == 0 or ny * nparams > 64 (fp lives in registers); a _FP / _GP / _EP bit
 *              without MIOC_ODE_SENS_P; _EP without MIOC_ODE_TERMINAL (and every case of _create_scen).
 * mioc_ode_program_eval_sens_device is the body of every eval entry.  S == 0: the program has no scenarios, state0 and
 *   params are host arrays and the checks are those of mioc_ode_program_eval_bolza_device; S >= 1: a scenario program,
 *   state0 and params are device arrays and the checks are those of mioc_ode_program_eval_scen_device.  MIOC_EINVAL
 *   also for d_Jp on a program without MIOC_ODE_SENS_P, d_Jy0 on one without MIOC_ODE_SENS_Y0, and S not matching the
 *   program's scen.  The four older eval entries accept a sens program and give no sensitivities.  Gate, stream and
 *   error behaviour as for mioc_ode_program_eval_scen_device: a closed gate leaves d_Jp and d_Jy0 untouched, a refused
 *   call leaves the context usable.
 *
 * mioc_ode_program_create needs no context and no GPU: it compiles for gfx950 and keeps the code object.  Limits:
 *   1 <= ny <= 8, 1 <= nx <= 8, 0 <= nparams <= 32, source text of at most 1 MiB (else MIOC_EINVAL).  A compile
 *   failure returns MIOC_ECOMPILE; the compiler's log (also the warnings of a successful compile) is copied into
 *   `log`, NUL-terminated and truncated to log_cap bytes (log nullable).  Diagnostics of the caller's text carry
 *   the file name "hooks" and the text's own line numbers ("hooks:3:...").  MIOC_EHIP: hiprtc could not be loaded.
 * mioc_ode_program_eval_device evaluates K controls like the built-in entry above: d_x K x nx x nt (the DP's
 *   input layout), d_J (K, nullable), d_df (K x nx x nt, nullable), state0 (ny) and params (nparams) host arrays
 *   passed to the kernel by value, tau = (T1 - T0)/nt; nx must equal the levels' number of controls once levels
 *   are set.  The code object is loaded on the context's device at first use and kept per device in the program; a
 *   program may serve several contexts and devices.  Enqueued on the context's stream; gated by mioc_trm_attach.
 * mioc_ode_program_destroy synchronises every device the program ran on, then unloads it; destroy a program before
 *   the contexts' devices are reset, and not while another thread evaluates it.
 */
typedef struct mioc_ode_program mioc_ode_program;
int32_t mioc_ode_program_create(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, mioc_ode_program **out,
                                char *log, int64_t log_cap);
/* The same with an integrator and its substeps per control interval (see "Integrators" above).  MIOC_EINVAL also for
 * an unknown integrator, substeps outside 1..64, and MIOC_ODE_INT_EULER with substeps != 1 (the reference scheme
 * defines no substeps).  mioc_ode_program_create(...) is _ex(..., MIOC_ODE_INT_EULER, 1, ...).  The program carries
 * its integrator and substeps: mioc_ode_program_eval_device takes them from it. */
#define MIOC_ODE_INT_EULER 0
#define MIOC_ODE_INT_HEUN 1
#define MIOC_ODE_INT_RK4 2
#define MIOC_ODE_INT_BEULER 16   /* implicit schemes start at 16 (see "Implicit integrators" above) */
#define MIOC_ODE_INT_MIDPOINT 17
#define MIOC_ODE_NEWTON_MAX 12   /* fixed: the Newton updates per substep, and the relative size of the last one */
#define MIOC_ODE_NEWTON_TOL 1e-10
int32_t mioc_ode_program_create_ex(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t integrator,
                                   int32_t substeps, mioc_ode_program **out, char *log, int64_t log_cap);
/* The same with the hooks named in `derive` generated from templated F and G (see "Derived hooks" above).  MIOC_EINVAL
 * also for bits outside MIOC_ODE_DERIVE_ALL.  mioc_ode_program_create_ex(...) is _ad(..., derive = 0, ...). */
#define MIOC_ODE_DERIVE_FY 1
#define MIOC_ODE_DERIVE_FU 2
#define MIOC_ODE_DERIVE_GY 4
#define MIOC_ODE_DERIVE_GU 8
#define MIOC_ODE_DERIVE_ALL 15
int32_t mioc_ode_program_create_ad(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t integrator,
                                   int32_t substeps, int32_t derive, mioc_ode_program **out, char *log, int64_t log_cap);
/* The same with a terminal cost, ndata columns of sampled data and the state trajectory as an output (see "Terminal
 * cost, sampled data, state output" above). */
#define MIOC_ODE_TERMINAL 1      /* flags: the text defines E (and Ey unless derived) */
#define MIOC_ODE_STATES   2      /* flags: the kernel can write the state trajectory */
#define MIOC_ODE_DERIVE_EY 16    /* derive bit, valid only with MIOC_ODE_TERMINAL; not part of MIOC_ODE_DERIVE_ALL */
int32_t mioc_ode_program_create_bolza(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                      int32_t integrator, int32_t substeps, int32_t derive, int32_t flags,
                                      mioc_ode_program **out, char *log, int64_t log_cap);
/* The text _create_bolza would hand to the compiler for these arguments (its order: "Derived hooks" above), copied
 * into `text`, NUL-terminated and truncated to text_cap bytes like a log (text nullable).  noinline != 0: the text of
 * the second compile, with MIOC_AD_NOINLINE in the head.  Returns the text's length without the NUL (a buffer of that
 * plus one holds all of it), or MIOC_EINVAL exactly where _create_bolza returns it for these arguments.  Needs neither
 * hiprtc nor a GPU. */
int64_t mioc_ode_program_source(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                int32_t integrator, int32_t substeps, int32_t derive, int32_t flags, int32_t noinline,
                                char *text, int64_t text_cap);
/* _create_bolza and _source for a program whose restarts solve different scenarios (see "Scenarios" above); scen == 0
 * is _create_bolza, and _source's text byte for byte. */
#define MIOC_ODE_SCEN      1     /* scen: state0 and the parameters per scenario */
#define MIOC_ODE_SCEN_DATA 2     /* scen: the data rows per scenario as well; only with MIOC_ODE_SCEN and ndata > 0 */
int32_t mioc_ode_program_create_scen(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                     int32_t integrator, int32_t substeps, int32_t derive, int32_t flags, int32_t scen,
                                     mioc_ode_program **out, char *log, int64_t log_cap);
int64_t mioc_ode_program_source_scen(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                     int32_t integrator, int32_t substeps, int32_t derive, int32_t flags, int32_t scen,
                                     int32_t noinline, char *text, int64_t text_cap);
/* _create_scen and _source_scen for a program that can return dJ/dparams and dJ/dstate0 (see "Sensitivities" above);
 * sens == 0 is _create_scen, and _source_scen's text byte for byte. */
#define MIOC_ODE_SENS_P   1      /* sens: dJ/dparams; the text defines Fp, Gp (and Ep with a terminal cost) unless derived */
#define MIOC_ODE_SENS_Y0  2      /* sens: dJ/dstate0 */
#define MIOC_ODE_DERIVE_FP 32    /* derive bits, valid only with MIOC_ODE_SENS_P; not part of MIOC_ODE_DERIVE_ALL */
#define MIOC_ODE_DERIVE_GP 64
#define MIOC_ODE_DERIVE_EP 128   /* only with MIOC_ODE_TERMINAL */
int32_t mioc_ode_program_create_sens(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                     int32_t integrator, int32_t substeps, int32_t derive, int32_t flags, int32_t scen,
                                     int32_t sens, mioc_ode_program **out, char *log, int64_t log_cap);
int64_t mioc_ode_program_source_sens(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                     int32_t integrator, int32_t substeps, int32_t derive, int32_t flags, int32_t scen,
                                     int32_t sens, int32_t noinline, char *text, int64_t text_cap);
int32_t mioc_ode_program_destroy(mioc_ode_program *prog);
int32_t mioc_ode_program_eval_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t K, const double *d_x, int64_t nt,
                                     double T0, double T1, const double *state0, const double *params, double *d_J,
                                     double *d_df);

/*
 * Mixed controls: continuous controls beside the DP's integer ones, for ODE programs.  A mixed
 * control x has nx = nu + nv rows per time step: rows 0..nu-1 are continuous (c), rows nu..nx-1 integer (v), as the
 * reference's rand_func lays them out (HelpFunctions.jl:136-148: x0[1:nu,:], x0[nu+1:nx,:]).  Device layout
 * K x nx x nt as everywhere ((K, nt, nx) row-major).  The bounds are pointwise, d_lo and d_hi of nt x nu doubles
 * ([i][m], the reference's umin[m, i] / umax[m, i]), lo <= hi.  The context's levels describe the nv integer rows
 * only (M = nv): the DP, the backtrack, pred and TV_p see compact K x nv x nt arrays.  The reference announces this
 * algorithm but has no code for it; the continuous step is defined here.
 *
 * mioc_ode_program_eval_mixed_device is mioc_ode_program_eval_device (the same kernel, launch, scratch and gate) with
 *   one different check: 1 <= nu < the program's nx, and once levels are set nx == nu + M (MIOC_EINVAL otherwise).
 *   K may be the K*R candidates of a fan.
 * mioc_rows_copy_device: dst[k][i][dst_row0 + r] = src[k][i][src_row0 + r] for r < nrows, k < K, i < nt, with dst of
 *   dst_nx and src of src_nx rows per step: the split (df -> df_v, x -> v_old) and the join (c, trial_v -> x_trial)
 *   around the DP.  dst == src is allowed with one nx and disjoint rows.  Enqueued on the context's stream; gated by
 *   mioc_trm_attach like mioc_pred_batch_device.  MIOC_EINVAL for a row range outside dst_nx / src_nx (and K > 65535,
 *   nx > 1024, nt >= 2^21).
 * mioc_mixed_state_bytes(K): bytes of the device state block of the continuous step, 1 <= K <= 4096 (else -1):
 *   offset 0 an int32 any-live word; offset 16 K doubles, the step size s; then K int32 flags (1 final, 2 moved),
 *   K int32 jsel (the candidate accepted last, -1 none), K int32 csteps (accepted continuous steps).  The caller
 *   zero-initialises it and writes the first step size s0 into s.
 * mioc_mixed_fan_device: the R candidates of a backtracking line search along the projected gradient, for all K
 *   restarts in one launch (1 <= R <= 16, 1 <= nu <= nx <= 1024).  For restart k and candidate j, with g = d_df:
 *     s_j = s[k] * 2^-j (exact);  for m < nu: t = x - s_j*g (one product, one difference),
 *     c_j = t < lo ? lo : (t > hi ? hi : t)  (a NaN stays a NaN);  rows m >= nu are copied from x.
 *   d_xfan is R x K x nx x nt, candidate-major: a batch of R*K controls for the eval entry.
 *     slope[j*K + k] = tau * sum g*(c - c_j): each term one difference, then one product; the sum starts at 0.0 and
 *     runs over i ascending, m ascending within i, sequentially (one lane folds the terms of an LDS chunk, as for
 *     int_val), so a host loop reproduces every bit.  Not gated.
 * mioc_mixed_select_device: per restart, with STOP = flag 4 of the TRM state block d_trm_state, in this order:
 *     1. a final restart is left alone;
 *     2. STOP and not moved (the flag of the previous call) -> final, left alone;
 *     3. otherwise the smallest j with slope_j > 0 and Jfan_j <= J_old - c1*slope_j (comparisons as written: a NaN
 *        never passes).  Found: rows < nu of xfan[j][k] are copied into x[k]; moved = (J_old - Jfan_j) >
 *        ctol*max(1, |J_old|); J_old = Jfan_j; s = min(2*s_j, smax); jsel = j; csteps += 1.  None: moved = false;
 *        s = s * 2^-R; jsel = -1;
 *     4. if STOP: it is cleared when moved (the DP runs again), else the restart is final.
 *   0 < c1 < 1, smax > 0, ctol >= 0.  Not gated.
 * mioc_mixed_poll: reduces the flags, synchronises the stream once (as mioc_trm_poll) and returns out[0] = the TRM
 *   gate word, out[1] = any restart that is not final and (not STOP or moved).  It takes K from the last
 *   mioc_mixed_select_device on d_mstate (MIOC_ESTATE if there was none).
 */
int32_t mioc_ode_program_eval_mixed_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K,
                                           const double *d_x, int64_t nt, double T0, double T1, const double *state0,
                                           const double *params, double *d_J, double *d_df);
int32_t mioc_ode_program_eval_bolza_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K,
                                           const double *d_x, int64_t nt, double T0, double T1, const double *state0,
                                           const double *params, const double *d_data, double *d_J, double *d_df,
                                           double *d_Y);
int32_t mioc_ode_program_eval_scen_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K,
                                          const double *d_x, int64_t nt, double T0, double T1, int64_t S,
                                          const double *d_state0, const double *d_params, const double *d_data,
                                          double *d_J, double *d_df, double *d_Y);
int32_t mioc_ode_program_eval_sens_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K,
                                          const double *d_x, int64_t nt, double T0, double T1, int64_t S,
                                          const double *state0, const double *params, const double *d_data,
                                          double *d_J, double *d_df, double *d_Y, double *d_Jp, double *d_Jy0);
int32_t mioc_rows_copy_device(mioc_ctx *ctx, int64_t K, int64_t nt, double *d_dst, int64_t dst_nx, int64_t dst_row0,
                              const double *d_src, int64_t src_nx, int64_t src_row0, int64_t nrows);
int64_t mioc_mixed_state_bytes(int64_t K);
int32_t mioc_mixed_fan_device(mioc_ctx *ctx, int64_t K, int64_t R, int64_t nu, int64_t nx, int64_t nt, double tau,
                              const double *d_x, const double *d_df, const double *d_lo, const double *d_hi,
                              void *d_mstate, double *d_xfan, double *d_slope);
int32_t mioc_mixed_select_device(mioc_ctx *ctx, int64_t K, int64_t R, int64_t nu, int64_t nx, int64_t nt, double c1,
                                 double smax, double ctol, void *d_mstate, void *d_trm_state, const double *d_xfan,
                                 const double *d_slope, const double *d_Jfan, double *d_J_old, double *d_x);
int32_t mioc_mixed_poll(mioc_ctx *ctx, void *d_mstate, void *d_trm_state, int32_t *out);

/*
 * Random admissible starts, rand_func_int (HelpFunctions.jl:204-225) on the device: K piecewise-constant controls
 * d_u_out (K x nx x nt, nx = the levels' M) with `jumps` distinct jump times drawn uniformly from steps 1..nt-1
 * (the reference's 2..nt) and a uniformly random admissible level per segment.  jumps < 0: floor(nt / 10), the
 * reference's default.  The stream is counter-based (seed, restart, draw), so a seed reproduces its controls on
 * any device; it is not Julia's MersenneTwister stream (not reproducible outside Julia).  Enqueued.
 * 1 <= nt <= 516096: the kernel keeps one bit per step and 256 counts in LDS, ((nt + 31)/32 + 256) * 4 bytes, and
 * 516096 is the largest nt for which that fits the 64 KB a launch gets; a larger nt, like jumps > nt - 1, is
 * MIOC_EINVAL before anything is launched.
 */
int32_t mioc_rand_start_device(mioc_ctx *ctx, int64_t K, int64_t nt, int64_t jumps, uint64_t seed, double *d_u_out);

/*
 * The PDE heat objective's gradient producer, batched on the device: eval_f / eval_df of
 * julia_opt/PDEObjective.jl:129-199 (implicit-Euler state with SMatLU, trapezoid cost, implicit-Euler adjoint with
 * AMatLU = lu(StateMat'), df_i = (M⁻¹F)ᵀ p_i + Gu) with the hooks of example_heat.jl:135-161 (G = ½(y−yd)ᵀM(y−yd),
 * G_t = γ·Σx, Gu = γ).  mioc_heat_setup takes the matrices the Julia objective already holds (example_heat.jl:101-115;
 * all column-major): M_invA (N x N), M_invF (N x nx), mass = M (N x N), state0 (N), yd (N x (nt+1)); τ = (T1−T0)/nt,
 * StateMat = I + τ·M_invA is factored once on the host.  1 <= N <= 2048, 1 <= nx <= 4.  A mioc_heat_setup that fails
 * validation (MIOC_EINVAL: a size out of range, T1 <= T0, a null input, a non-finite γ or M_invA, a singular StateMat) returns
 * before it touches the context's heat problem: the last successful setup stays in force.  mioc_heat_eval_device:
 * d_x = K x nx x nt controls (the DP's input layout), d_J (K, nullable), d_df (K x nx x nt, nullable).  Enqueued.
 */
int32_t mioc_heat_setup(mioc_ctx *ctx, int64_t N, int64_t nx, int64_t nt, double T0, double T1, double gamma,
                        const double *M_invA, const double *M_invF, const double *mass, const double *state0,
                        const double *yd);
int32_t mioc_heat_eval_device(mioc_ctx *ctx, int64_t K, const double *d_x, double *d_J, double *d_df);
/* The same from host arrays (the Julia objective's x / df, K x nx x nt column-major; J: K), synchronous. */
int32_t mioc_heat_eval(mioc_ctx *ctx, int64_t K, const double *x, double *J, double *df);

/*
 * The signal-reconstruction (convolution) objective's gradient producer, batched on the device (Marko / Wachsmuth
 * §6.2; the reference's main("convolution"), multi-trust.jl:190-192): eval_f_helper / eval_df_helper of
 * julia_opt/example_convolution.jl:128-141, v = K·xᵀ − fvec, J = ½·vᵀ·M·v, df = (Kᵀ·(M·v))ᵀ, with
 *   K    (nt+1) x nt, toeplitz (:104-125): K[r,c] = κ[r−c] for r−c >= 1 and 0 otherwise (1-based) -- strictly lower
 *        triangular Toeplitz, row 1 and the diagonal are zero.  kappa = K[2:nt+1, 1] (nt values) defines it; the
 *        matrix is never stored;
 *   fvec nt+1 values, f_to_vec (:73-81): fvec[i] = target(T0 + τ·i), i = 1..nt+1 -- the grid starts one step AFTER
 *        T0 (the reference's offset, kept: the caller passes obj.fvec as it is);
 *   M    (nt+1)² tridiagonal, Mmat (:85-100): τ/3 at both ends of the diagonal, (2/3)·τ inside, τ/6 beside it;
 *        built here from τ = (T1 − T0) / nt.
 * One control with signed levels (𝓥 = [[-2,-1,0,1,2]]).  1 <= nt <= 16384 (κ is held in LDS).  mioc_conv_eval_device:
 * d_x = K x 1 x nt controls (the DP's input layout), d_J (K, nullable: no value), d_df (K x 1 x nt, nullable: stops
 * after J).  Enqueued.  A restart's J and df do not depend on K or on its position in the batch.  A mioc_conv_setup
 * that fails validation (MIOC_EINVAL: nt out of range, T1 <= T0 or either not finite, a null input, a non-finite κ or
 * fvec) returns before it touches the context's convolution problem: the last successful setup stays in force.
 * Errors: MIOC_EINVAL (the above; eval: K out of range, a null x, the host entry with neither J nor df), MIOC_ESTATE
 * (eval before a successful setup), MIOC_ENOMEM (the context's scratch cannot grow: K x (nt+1) doubles of v for J
 * alone, K x (2·nt+17) with a gradient -- v and the rows of w = M·v, nt+16 each; it is kept between calls and
 * never shrinks).
 * mioc_conv_tiles_per_wave: which variant of the product kernel an evaluation of K restarts at nt runs -- 1 or 2
 * column tiles of 16 per wave (two once (K+15)/16 restart tiles x ceil(nt/32) waves give every SIMD one; the results
 * are the same bit for bit), 0 when nt or K is out of range.  For tests and tools that must know what they exercise;
 * needs no context.
 */
int32_t mioc_conv_tiles_per_wave(int64_t nt, int64_t K);
int32_t mioc_conv_setup(mioc_ctx *ctx, int64_t nt, double T0, double T1, const double *kappa, const double *fvec);
int32_t mioc_conv_eval_device(mioc_ctx *ctx, int64_t K, const double *d_x, double *d_J, double *d_df);
/* The same from host arrays (the Julia objective's x / df, K x 1 x nt; J: K), synchronous. */
int32_t mioc_conv_eval(mioc_ctx *ctx, int64_t K, const double *x, double *J, double *df);

/* The HIP stream the context enqueues on (hipStream_t), for callers that order their own work. */
void *mioc_stream(mioc_ctx *ctx);

/*
 * Kernel timing (MIOC_OPT_TIMING=1): HIP events recorded on the context's stream around the
 * launches of each kernel class.  which: 0 = dominant DP kernel of the last bellman call (generic
 * step sweep or p=Inf recursion), 2 = p=Inf class-table prep,
 * 1 = backtrack.  Returns cumulative milliseconds, launch count and the kernel's name (p=Inf: the name of the
 * recursion kernel that took the DP in window 0, k_pinf_recur, _xr, _mcw or _ws, and of the class-table kernel in
 * window 2, k_pinf_prep, k_pinf_prep_m or k_pinf_prep_small).
 */
int32_t mioc_kernel_stats(mioc_ctx *ctx, int32_t which, double *total_ms, int64_t *launches,
                          const char **name);
int32_t mioc_reset_stats(mioc_ctx *ctx);

/* Which algorithm served the last mioc_bellman* call (MIOC_ALGO_GENERIC / _PINF / _PYRAMID). */
int32_t mioc_last_algo(mioc_ctx *ctx);
/* Which driver ran the last separable-transform DP (before any per-step redo): 0 one launch per step,
 * 1 the general persistent driver (k_sdt_run), 2 the one-row persistent driver (k_sdt_run1). */
int32_t mioc_last_sdt_driver(mioc_ctx *ctx);

/*
 * Diagnostics of the last bellman/backtrack: counters[0] pyramid / separable-transform targets resolved by
 * the exact scan because their winning value has another source value within rounding distance, [1] pyramid
 * targets resolved by the exact scan because their minimum is reached at two levels (separable transform:
 * targets of rows sent straight to the exact scan: few targets, or a value scale outside its binade), [2] backtrack: p=Inf walk steps resolved
 * by the exact scan, or for the U-table walks (generic, pyramid) the run-ahead rounds taken (each round
 * settles up to 64 steps), [3] internal consistency failures (must be 0); [4..7] pyramid internals: rows whose
 * value hash overflowed, targets whose value was not found, values flagged as colliding (after a separable-transform
 * DP, [4] instead counts the persistent driver's rows whose write-after-read wait on the rows above was armed (a staging buffer reused while later rows may still read it), and [6] counts this context's persistent DPs redone with per-step launches: the grid does not fit, or
 * a dependency wait timed out -- 0 on a healthy run; after a fused separable DP, the segmented launches redone with
 * one workgroup per subproblem); [7] fused DP: resident workgroups per CU (occupancy query); [8] fused separable DP:
 * row segments per subproblem (0: the one-lane-per-row kernel); [9] p=Inf segmented walk: subproblems whose path
 * met a state-dependent step and were walked serially (-1: the serial walk ran for all).  n may be up to 10.
 */
int32_t mioc_diagnostics(mioc_ctx *ctx, int64_t *counters, int32_t n);

/*
 * The argmin table `U` of the last bellman call, one step at a time, in the reference's layout
 * (HelpFunctions.jl:74, U[:, c+1, l..., i+1] of multi-trust.jl:76): for subproblem k and step i
 * (0 <= i < nt-1), U_out[c + (B+1)*g] = 0-based iterator rank of the source j minimising Φ_i at budget
 * c and the target level with grid-linear index g (levels in column-major grid order), as an int32.
 * Cells the reference never writes because Φ_i = +Inf there hold -1 when c < b̃(l, i) and are
 * unspecified otherwise (the reference leaves them at whatever `U` held before); the separable transform
 * (MIOC_ALGO_SEPARABLE) reports -1 for every such cell, so its tables equal the reference's.  U_out has
 * (B+1) * prod(counts) entries.  The p=Inf collapse stores class tables instead (MIOC_EINVAL).
 */
int32_t mioc_get_argmin_table(mioc_ctx *ctx, int64_t k, int64_t step, int32_t *U_out);

/*
 * Test access to the tables of the p=Inf collapse (MIOC_ALGO_PINF), which keeps these instead of U: the device rows of
 * subproblem k and step i (0 <= i < nt) of the last bellman call, copied out as they are.
 * With p = Inf the switching weight is 1.0 for every pair (l, j), so K(l, j) = fl(T1(l) + beta) =: K_l does not
 * depend on j (the terminal step i = nt-1 holds T1 alone, no beta), and with b~_l = sum_m |nu_lm - u_old_m(i)| the
 * budget class of level l:
 *   kmin_out  [BWP]  kmin_i[b]: the minimum of K_l over the levels of class b;
 *   k2_out    [BWP]  the second-smallest distinct value of K_l in class b (+Inf: none);
 *   kfirst_out[BWP]  the first rank l attaining kmin_i[b] (-1: the class is empty);
 *                    classes BW..BWP-1 are padding: +Inf, +Inf, -1;
 *   kabs_out  [1]    max |K_l| over the levels of classes < BW (the walk's rounding bound);
 *   R_out     [RP]   the row minima R_i[c] = min_l Phi_i[c, l] = min_b fl(kmin_i[b] + R_{i+1}[c - b]),
 *                    R_{nt-1}[c] = kmin_{nt-1}[c]; +Inf where no level reaches, and in the rows B+1..RP-1;
 *   sizes_out [3]    BW (classes tracked: the batch's largest b~ within B, plus one), BWP (BW padded to a power of two
 *                    >= 8), RP (B + 1 rounded up to a multiple of 64).
 * Every output pointer may be NULL, so a first call can ask for the sizes alone.  A segmented recursion whose hand-off
 * wait timed out is redone before its tables are read, as for mioc_get_argmin_table.
 * MIOC_ESTATE without a DP; MIOC_EINVAL after another algorithm, or for k or step out of range; a rejected call changes
 * nothing.
 */
int32_t mioc_get_pinf_tables(mioc_ctx *ctx, int64_t k, int64_t step, double *R_out, double *kmin_out, double *k2_out,
                             int32_t *kfirst_out, double *kabs_out, int64_t *sizes_out);

#ifdef __cplusplus
}
#endif
#endif /* MIOC_H */
