/* wlhip.h — C ABI of libwlhip.so: the MI355X (gfx950) backend for WaterLily's time-step hot path.
 *
 * Boundary being replaced: the reference has no FFI — it selects a backend by Julia multiple dispatch
 * on the array type (`Simulation(...; mem=ArrayType)`, /root/reference/src/WaterLily.jl:67-68,98;
 * src/Flow.jl:133-146) and generates every kernel from `@loop` through KernelAbstractions
 * (src/core.jl:125-156).  This header is what a Julia package extension binds with `ccall` for a new
 * array type: every entry point cites the reference function it stands in for.
 *
 * Conventions
 *  - Arrays are dense, column-major, x fastest, vector component slowest — byte-identical to the Julia
 *    arrays (scalar (Ng...), vector (Ng...,D), tensor (Ng...,D,D)), so `pointer(a)` is passed with no copy.
 *  - All pointers are DEVICE pointers unless named host_*.  Element type: Float32.
 *  - Every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *    unless it returns a host scalar, in which case it synchronises that stream.  Streams the library opens itself (fork/join
 *    of plane ranges, the communicator's exchange stream) wait for `stream` and are joined back into it before the call returns.
 *  - Handle creation (wl_mg_create, wl_sim_create, wl_sim_create_on, wl_sim_create_slab, the communicator constructors) takes no
 *    stream: it works on the DEFAULT stream and returns finished (synchronised).  It reads the caller's L (= μ₀) there, so the
 *    caller must have synchronised whatever produced the arrays it passes in before it creates the handle.
 *  - A handle's calls may move from one stream to another; the caller orders the two streams (an event, or a synchronisation),
 *    as for any other work on the handle's arrays.
 *  - One host thread at a time: the read-back record, the default reduction workspace and the fork/join events are process-wide.
 *    Driving the library from several host threads at once is not supported, whatever streams and handles the threads use.
 *  - Return value: 0 = ok; >0 = hipError_t; <0 = library error (WL_E*).  wl_last_error_string() gives text.
 *    No exception crosses this boundary.
 *  - Aliasing pois.x≡flow.p, pois.L≡flow.μ₀, pois.z≡flow.σ (src/WaterLily.jl:97) is allowed everywhere.
 */
#ifndef WLHIP_H
#define WLHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WL_EINVAL (-1)   /* bad argument (the reference's @assert failures map here) */
#define WL_ENOGPU (-2)   /* no usable HIP device */
#define WL_ELEVELS (-3)  /* "MultiLevelPoisson requires size=a2ⁿ, where n>2" (src/MultiLevelPoisson.jl:73-74) */
#define WL_ECOMM (-4)    /* halo/collective failure */

/* Grid descriptor of one (slab of a) Cartesian array with one ghost layer per side in x,y and
 * `k0` ghost planes in z.  A single-GPU array is the case gk=0, gnz=nz, k0=1, k1=nz-1.
 * For D==2: nz=1, k0=0, k1=1, gnz=1. */
typedef struct wl_grid {
  int32_t D;        /* 2 or 3 */
  int32_t nx, ny, nz; /* allocated extents INCLUDING ghosts */
  int32_t k0, k1;   /* local z planes [k0,k1) are the interior planes this rank owns */
  int32_t gk;       /* global z index (0-based, ghosts included) of local plane 0 */
  int32_t gnz;      /* global z extent including ghosts */
} wl_grid;

/* convective schemes λ(u,c,d): src/Flow.jl:4-6 */
enum { WL_QUICK = 0, WL_VANLEER = 1, WL_CDS = 2 };

/* ---- lifecycle ---------------------------------------------------------------------------- */
int wl_init(int device);                       /* hipSetDevice + capability check (gfx950)           */
const char* wl_last_error_string(void);
int wl_version(void);
int wl_malloc(void** p, size_t bytes);          /* device allocation owned by the caller (Julia finalizer -> wl_free) */
int wl_free(void* p);
int wl_h2d(void* dst, const void* host_src, size_t bytes, void* stream);   /* `mem(::Array)` ctor, src/Flow.jl:139,143-144 */
int wl_d2h(void* host_dst, const void* src, size_t bytes, void* stream);   /* `Array(a)`                      */
int wl_d2d(void* dst, const void* src, size_t bytes, void* stream);        /* copy / `u⁰ .= u`, src/Flow.jl:157 */
int wl_stream_sync(void* stream);
wl_grid wl_grid_single(int D, const int32_t* dims_with_ghosts);            /* host helper: single-domain descriptor */

/* ---- generic array ops the array type must support ------------------------------ */
int wl_fill(float* a, float v, size_t n, void* stream);                    /* fill!, `r .= 0` src/Flow.jl:39, MultiLevelPoisson.jl:94 */
int wl_scale(float* a, float s, size_t n, void* stream);                   /* `x .*= dt` src/Flow.jl:225             */
int wl_div_scalar(float* a, float s, size_t n, void* stream);              /* `x ./= dt` src/Flow.jl:230             */
int wl_sum(const float* a, size_t n, double* host_out, void* stream);      /* sum(a)     src/Poisson.jl:95            */
int wl_sum_abs_max_abs(const float* a, size_t n, double* host_l1, float* host_linf, void* stream); /* L₁,L∞ src/Poisson.jl:190-191 */
int wl_max(const float* a, size_t n, float* host_out, void* stream);       /* maximum(a) src/Flow.jl:236              */
int wl_dot(const float* a, const float* b, size_t n, double* host_out, void* stream); /* a⋅b  src/Poisson.jl:156,189   */
int wl_L2_inside(const float* a, const wl_grid* g, double* host_out, void* stream);   /* L₂(a) src/Poisson.jl:188; ext/WaterLilyAMDGPUExt.jl:18 */

/* ---- boundary conditions: src/core.jl:200-243 ------------------------------------------------ */
/* BC!(a,U::tuple,saveexit,perdir): all faces, all components, one launch (edge/corner values equal the
 * reference's sequential (i,j) order).  perdir_mask bit (j-1) set = direction j periodic.            */
int wl_bc_vec(float* a, const wl_grid* g, const float* host_U, int saveexit, unsigned perdir_mask, void* stream);
/* Function-valued BCs and body forces that depend on position.  A C ABI cannot call a Julia closure, so the host
   tabulates it: Ub has the shape of `a` and holds uBC(i,loc(i,I),t) on the two outermost layers of every non-periodic direction
   (other cells are never read); G holds g(i,loc(i,I),t)+∂ₜuBC for every cell. */
int wl_bc_vec_fn(float* a, const float* Ub, const wl_grid* g, int saveexit, unsigned perdir_mask, void* stream);  /* BC!(a,uBC::Function,…) src/core.jl:201-219 */
int wl_accelerate_field(float* r, const float* G, const wl_grid* g, void* stream);                               /* accelerate!(r,t,g,U) src/Flow.jl:69-73 */
int wl_bc_per_scalar(float* a, const wl_grid* g, unsigned perdir_mask, void* stream);   /* perBC!   src/core.jl:239-243 */
int wl_exit_bc(float* u, const float* u0, const wl_grid* g, float dt, void* stream);    /* exitBC!  src/core.jl:226-233 */

/* ---- Flow: src/Flow.jl ------------------------------------------------------------------------ */
/* conv_diff!(r,u,Φ,λ;ν,perdir) :38-62 — gather form, one launch; Φ (=flow.σ) receives the same stale
 * ghost-plane fluxes the reference leaves there. Φ may be NULL.                 */
int wl_conv_diff(float* r, const float* u, float* Phi, const wl_grid* g, float nu, unsigned perdir_mask, int scheme, void* stream);
/* BDIM!(a) :176-180 with the neighbouring scale_u! folded in: u = (u*pre + μddn(μ₁,f) + V + μ₀ f)*post,
 * f = u⁰ + dt f − V on all cells.  mu1 may be NULL (== zeros, NoBody fast path), V may be NULL (== zeros). */
int wl_bdim(float* u, const float* u0, float* f, const float* V, const float* mu0, const float* mu1,
            const wl_grid* g, float dt, float pre, float post, void* stream);
int wl_scale_u(float* u, const wl_grid* g, float s, void* stream);                      /* scale_u! :211-214 */
int wl_div(float* z, const float* u, const wl_grid* g, void* stream);                   /* @inside z = div(I,u) :225 */
int wl_project(float* u, const float* L, const float* x, const wl_grid* g, void* stream); /* u[I,i] -= L[I,i]∂ᵢx :227-229 */
/* CFL(a) :234-237 — writes σ=flux_out on the interior and returns min(Δt_max, 1/(max(σ over ALL cells)+5ν)) */
int wl_cfl(const float* u, float* sigma, const wl_grid* g, float nu, float dt_max, float* host_dt, void* stream);
/* sgs!(flow,u,t; νₜ=smagorinsky,S,Cs,Δ) src/util.jl:66-76 — the Smagorinsky–Lilly sub-grid-scale force added to f (= flow.f): S = S(I,u) on inside(σ)
 * (src/Metrics.jl:42-44,140), νₜ(I) = (Cs·Δ)²·sqrt(S[I]:S[I]) (the docstring's code example, :62 — sqrt(S:S), not the sqrt(2S:S) of its prose: scale Cs by 2^¼ for
 * that form), νₜ ≡ 0 on the ghost layer (a zero-initialised S buffer); then the nine (i,j) sweeps over inside_u(N,j) as one gather in the reference's order.
 * sigma (= flow.σ) is scratch, as in the reference: its inside cells receive νₜ, its ghost cells what the reference's sweeps leave there.  At most two launches.
 * 3-D single-domain grids only: a 2-D or z-slab wl_grid returns WL_EINVAL. */
int wl_sgs(float* f, float* sigma, const float* u, const wl_grid* g, float Cs, float Delta, void* stream);

/* ---- Poisson leaf operations: src/Poisson.jl --------------------------------------------------- */
int wl_set_diag(float* D, float* iD, const float* L, const wl_grid* g, void* stream);   /* set_diag! :43-46 */
int wl_mult(float* z, const float* L, const float* D, const float* x, const wl_grid* g, void* stream); /* mult! :63-69 (no perBC, z ghosts zeroed) */
/* residual! :92-98 — r = iD==0 ? 0 : z−Ax; s=Σr/N; if |s|>2eps: r-=s.  No host sync.
 * scratch: device workspace of wl_reduce_workspace_bytes() bytes.                                   */
int wl_residual(float* r, const float* x, const float* z, const float* L, const float* D, const float* iD,
                const wl_grid* g, void* scratch, void* stream);
int wl_increment(float* r, float* x, const float* eps, const float* L, const float* D, const wl_grid* g, float omega, void* stream); /* increment! :100-104 */
int wl_jacobi(float* eps, float* r, float* x, const float* L, const float* D, const float* iD, const wl_grid* g, int it, float omega,
              unsigned perdir_mask, void* stream);                                      /* Jacobi! :111-114 */
int wl_gsrb(float* eps, float* r, float* x, const float* L, const float* D, const float* iD, const wl_grid* g, int it, float omega,
            unsigned perdir_mask, void* stream);                                        /* GaussSeidelRB! :141-148 */
int wl_norms(const float* r, const wl_grid* g, double* host_l1, float* host_linf, void* scratch, void* stream); /* L₁, L∞ :190-191 */
/* single-level solver.  z doubles as pcg!'s work array, exactly as p.z does in the reference. */
int wl_pcg(float* eps, float* r, float* x, float* z, const float* L, const float* D, const float* iD, const wl_grid* g, int it,
           unsigned perdir_mask, void* stream);                                         /* pcg!(p;it=6) :166-186 */
int wl_poisson_solve(float* eps, float* r, float* x, float* z, const float* L, const float* D, const float* iD, const wl_grid* g,
                     double tol, int itmx, unsigned perdir_mask, int* host_n, double* host_r1, float* host_rinf,
                     void* stream);                                                     /* solver!(p::Poisson;tol,itmx) :212-223 */
size_t wl_reduce_workspace_bytes(void);

/* ---- temporal averages: src/Metrics.jl:200-255 --------------------------------- */
/* update!(meanflow,flow) with the weight ε computed by the caller (:237-239); UU may be NULL (uu_stats=false) */
int wl_meanflow_update(float* P, float* U, float* UU, const float* p, const float* u, const wl_grid* g, float eps, void* stream);
int wl_meanflow_uu(float* tau, const float* UU, const float* U, const wl_grid* g, void* stream);   /* uu!(τ,a) :250-252 */

/* ---- flow diagnostics: src/Metrics.jl:27-109 ------------------------------------------------------ */
/* Whole-field forms of the reference's per-index functions (`@inside σ[I] = f(I,u)`): only inside cells of an output are written, its ghost
 * cells keep what they held.  u is the (Ng...,D) velocity array; an output may be flow.σ, it may not overlap u (WL_EINVAL).  ke, ω, ω_mag, ω_θ
 * and λ₂ come from one z-marching kernel that forms J[i][j] = ∂(i,j,I,u) (:42-44) per cell and reads every u value once per tile: one launch
 * per call, and a field has the same bits whichever entry point produced it.  ω, ω_mag, ω_θ, λ₂ and helicity are CartesianIndex{3} methods:
 * a 2-D wl_grid returns WL_EINVAL.  Single-domain grids only: a z-slab wl_grid returns WL_EINVAL for every entry point of this section. */
int wl_ke(float* out, const float* u, const wl_grid* g, const float* host_U /*NULL = 0*/, void* stream);             /* ke(I,u,U) :33-35 (2-D and 3-D) */
int wl_curl(float* out, const float* u, const wl_grid* g, int i /*1..3; 2-D: 3*/, void* stream);                     /* curl(i,I,u) :68 — the cell-EDGE stencil */
int wl_omega(float* out3, const float* u, const wl_grid* g, void* stream);                                           /* ω(I,u) :74 — out3 is a vector array (Ng...,3) */
int wl_omega_mag(float* out, const float* u, const wl_grid* g, void* stream);                                        /* ω_mag(I,u) :80 */
int wl_omega_theta(float* out, const float* u, const wl_grid* g, const float host_z[3], const float host_center[3], void* stream);   /* ω_θ(I,z,center,u) :87-91 */
/* λ₂(I,u) :54-58 — J in Float32 (cross terms as neighbour differences first); S²+Ω² and its middle eigenvalue (closed form) in Float64: accurate to a few
 * eps32·‖S²+Ω²‖ in every cell, where eigenvalues coincide and where the gradient nearly vanishes included; S²+Ω² = 0 gives exactly 0 */
int wl_lambda2(float* out, const float* u, const wl_grid* g, void* stream);
int wl_helicity(float* out, const float* u, const float* omega, const wl_grid* g, void* stream);                     /* helicity(I,u,ω) :99-109, ω a collocated (Ng...,3) array */
/* one pass over u for several fields at once; any NULL output is skipped; at least one non-NULL */
int wl_flow_fields(const float* u, const wl_grid* g, const float* host_U, float* ke, float* omega3, float* omega_mag, float* lambda2, void* stream);
/* out = { Σ_inside ke(I,u,U), Σ_inside ½|ω|², max_inside |ω| } (2-D: curl(3,I,u) for ω): the per-cell Float32 values the field calls produce, summed in
 * Float64; at most two launches; synchronises.  scratch: device workspace of wl_reduce_workspace_bytes() bytes. */
int wl_flow_stats(const float* u, const wl_grid* g, const float* host_U, double out[3], void* scratch /*NULL = library's*/, void* stream);

/* ---- multigrid transfer: src/MultiLevelPoisson.jl ---------------------------------------------- */
int wl_restrict(float* a_coarse, const wl_grid* gc, const float* b_fine, const wl_grid* gf, void* stream);    /* restrict! :49 */
int wl_prolongate(float* a_fine, const wl_grid* gf, const float* b_coarse, const wl_grid* gc, void* stream);  /* prolongate! :50 */
int wl_restrictL(float* a_coarse, const wl_grid* gc, const float* b_fine, const wl_grid* gf, unsigned perdir_mask, void* stream); /* restrictL! :42-48 */
int wl_coarsen_dims(int D, const int32_t* fine, int32_t* coarse);                      /* coarsen_mask/divisible :29,52; returns #dirs coarsened */

/* ---- MultiLevelPoisson handle: struct :61-77, update! :79-86, Vcycle! :88-101, solver! :108-128 -- */
typedef struct wl_mg wl_mg;
/* x, L, z are the caller's (aliased) level-1 arrays; coarse levels and r,ϵ,D,iD are owned by the handle. */
int wl_mg_create(wl_mg** out, float* x, float* L, float* z, const wl_grid* g, unsigned perdir_mask, int maxlevels);
int wl_mg_destroy(wl_mg* mg);
int wl_mg_update(wl_mg* mg, void* stream);
int wl_mg_nlevels(const wl_mg* mg);
int wl_mg_level_grid(const wl_mg* mg, int level, wl_grid* out);
/* name ∈ "L","D","iD","x","eps","r","z" — device pointer of that level's array (tests read pois.levels[k].D etc.).
 * On the multigrid handle of a simulation composite, whose option "rskip" is on by default, the smoother does not store residuals nobody reads: level 0's "r" is brought up to date by this call
 * (if the last smooth! skipped its store: one launch on the stream that smooth! ran on, waited for; ask again after every solve), a coarse level's "r" is
 * unspecified scratch.
 * Writing through these pointers: between public calls the interior cells of every level's "r" and "eps" and of a coarse level's "z", and EVERY cell of a coarse
 * level's "x", are dead — the library writes them before it reads them, whatever they hold (Vcycle!'s fill!(coarse.x,0) clears the ghost cells too, also where it
 * is folded into the level's Jacobi!).  The ghost cells of "r", "eps" and "z" are not: the kernels read them as the zeros they have held since wl_mg_create
 * (a ghost ϵ is multiplied by L = 0, which stops a finite value and not a NaN) — a writer leaves them zero.  tests/test_gpu_deadstore.py overwrites the dead cells. */
float* wl_mg_level_field(const wl_mg* mg, int level, const char* name);
int wl_mg_vcycle(wl_mg* mg, int level, float omega, void* stream);
int wl_mg_smooth(wl_mg* mg, int level, int it, float omega, void* stream);      /* smooth! = GaussSeidelRB! on one level (:106) */
int wl_mg_level_is_const(const wl_mg* mg, int level);   /* 1 if the level's L was verified to be 'constant inside, 0 on wall faces' */
int wl_mg_smoother_kind(const wl_mg* mg, int level);   /* how smooth! runs on the level: 0 one kernel per pass, 1 temporally blocked, 2 blocked pair kernels,
                                                          3 z-split (pair kernels away from the body, general blocked kernels near it) */
int wl_mg_set_fused(wl_mg* mg, int on);   /* bit0 (default 1): temporally blocked smoother on eligible levels, 0: one kernel per pass;
                                             bit1: do not store the final ϵ (scratch of the reference that nothing reads again);
                                             bit2: no pair kernels; bit3: no single-launch coarse tail; bit4: no z-split on body levels;
                                             bit5: coarse tail in global memory instead of LDS (process-wide switch); bit6: x increment of the prolongation not deferred to kernel B;
                                             bit7: z-slabs: the smoother's deep r exchange is not overlapped with kernel A's interior planes;
                                             bit8: the pair smoother's kernels A and B exchange r′ and ϵ_mid through the two dense arrays only, never through the
                                             level's line-aligned exchange buffer (which needs bit1 set, bit6 clear and a pending prolongation: Vcycle! inside solver!) */
/* solver!(ml;tol,itmx): returns iterations in *host_n and the last L₁/L∞; appends to the n history. */
int wl_mg_solve(wl_mg* mg, double tol, int itmx, int* host_n, double* host_r1, float* host_rinf, void* stream);
int wl_mg_history(const wl_mg* mg, int16_t* host_out, int cap);                        /* pois.n :66 */
/* per-iteration log of the last solve: what `@log` prints (:112,117): r∞, r₁, ω */
int wl_mg_last_log(const wl_mg* mg, double* host_r1, double* host_rinf, double* host_omega, int cap);
/* how the last solve applied residual!'s mean shift (:95-97): 0 a pass of its own, 1 inside the finest level's z-marching Jacobi!, 2 the fused projection head; -1 no solve yet */
int wl_mg_shift_path(const wl_mg* mg);

/* ---- Simulation/Flow composite (what bench.py times): src/Flow.jl:156-167, src/WaterLily.jl:128-139 */
typedef struct wl_sim wl_sim;
typedef struct wl_sim_desc {
  int32_t D;
  int32_t dims[3];          /* interior cells N (no ghosts) */
  float uBC[3];             /* tuple boundary velocity */
  float nu, dt0;
  uint32_t perdir_mask;
  int32_t exitBC;
  int32_t scheme;           /* WL_QUICK ... */
  int32_t has_body;         /* 0: NoBody fast path (μ₁≡0, V≡0 never read) */
  /* caller-owned flow arrays (NULL => the handle allocates and owns them) */
  float *u, *u0, *f, *p, *sigma, *V, *mu0, *mu1;
  /* optional caller-owned SPARE velocity array (same size as u).  The fused kernels are out of place (conv_diff!+BDIM! and the
     projection tail write a velocity array other than the one they read) and `u⁰ .= u` (src/Flow.jl:157) is a pointer swap, so
     the handle PERMUTES the roles of the three arrays {u, u0, us} from step to step.  With caller-owned u and u0:
       us given : full-speed path; after every wl_sim_mom_step read the current roles back with wl_sim_field(s,"u"|"u0"|"us")
                  (the Julia binding re-points its HipArray objects; the three buffers stay the caller's to free);
       us NULL  : pointers never move — `u⁰ .= u` is a copy and conv_diff!/BDIM! run as separate passes (slower).
     Convective exit (exitBC=1, single domain): the buffers rotate as well; BC! leaves the x-exit face of u alone (saveexit, src/core.jl:207),
     so that face is copied from the old role holder to the new one at each rotation (one strided plane).  On z-slabs exitBC flows keep the copy.
     What the scratch arrays hold at wl_sim_create, and between calls, does not matter: every cell of `us` (whichever buffer is in that role) and of `f`, and
     the interior cells of `sigma`, are written before they are read — uninitialised memory will do (the Julia binding passes `similar(u)`); σ's GHOST cells are
     live: conv_diff! leaves stale fluxes in the upper ones, nothing ever writes the lower ones, and CFL's maximum(σ) sees them all, as in the reference. */
  float *us;
} wl_sim_desc;
int wl_sim_create(wl_sim** out, const wl_sim_desc* desc);
/* the same on an EXISTING multigrid handle (wl_mg_create on desc->p, desc->mu0, desc->sigma): the Simulation constructor of the
   reference builds the AbstractPoisson first (pois_ctor, src/WaterLily.jl:96-105) and mom_step!(flow,pois) receives both.  The wl_mg
   stays the caller's (destroy the wl_sim first).  Side effects on the adopted handle: the final ϵ of smooth! is no longer stored
   (wl_mg_set_fused bit1 — scratch nothing on the time-step path reads).  WL_EINVAL if the handle was not built on desc's p, mu0, sigma or
   with a different perdir mask. */
int wl_sim_create_on(wl_sim** out, const wl_sim_desc* desc, wl_mg* mg);
int wl_sim_destroy(wl_sim* s);
float* wl_sim_field(wl_sim* s, const char* name);       /* "u","u0","f","p","sigma","V","mu0","mu1","us" (current roles) */
wl_mg* wl_sim_pois(wl_sim* s);
int wl_sim_grid(const wl_sim* s, wl_grid* out);
int wl_sim_init_flow(wl_sim* s, void* stream);          /* BC!(u), u⁰=u, μ₀ BC, (src/Flow.jl:141-145) after the caller filled u */
/* implementation switches (the tests compare the variants bit for bit).  Defaults in brackets.
   "fused_smoother"[1] temporally blocked GaussSeidelRB!   "pair"[1] its two-cells-per-thread constant-coefficient variant
   "constl"[1] constant-coefficient (NoBody) kernels        "fuse_p"[1] fused projection head (div+scale+residual!) and tail
   "fuse_cfl"[1] CFL folded into the corrector's tail       "tail"[1] smallest V-cycle levels in one launch
   "store_f"[0] materialise the intermediates f, z          "store_eps"[0] materialise the smoother's final ϵ
   "overlap"[1] u exchange on a second stream (slabs)       "convz"[0], "convm"[0] alternative conv_diff! kernels (slower)
   "jacobi_march"[1] z-marching constant-coefficient Jacobi  "farmask"[1], "hybrid"[1] BDIM! fast paths away from a body
   "zsplit"[1] pair smoother on the planes away from a body (levels >= 16 M cells; 2: any size, v >= 4: >= v·2^20 cells)
   "defer_shift"[1] residual!'s mean shift + solver!'s first norms folded into the finest level's z-marching Jacobi!
   "skip_fill"[1] Vcycle!'s fill!(coarse.x,0) folded into the coarse level's Jacobi!
   "convt"[1] LDS-tiled z-marching conv_diff!+BDIM! (NoBody, no periodic direction, f not stored; v > 1: on with z-chunks of v planes)
   "bcfold"[1] BC!(u,U) for a tuple U folded into the stores of the kernels that produce u (single domain, no exit, no periodic direction):
   bit 0 the projection tails, bit 1 the tiled conv_diff!+BDIM! (measured slower: off by default)
   "resjac"[1] projection head (div, x·=dt, residual!) + the V-cycle's first Jacobi! in one launch on single-domain NoBody levels (the
   mean shift is checked on the host afterwards; if due, the two-kernel path is taken)   "resjac_min"[6 Mi cells] size gate (tests: 0)
   "lazydt"[1] wl_sim_mom_steps: see there
   "tailspec"[1] the projection tail is queued behind the smoother before the host has read that iteration's norms and gated on the device by solver!'s break test
       (the flag the host then takes its own decision from): it runs iff the iteration was the last one.  Single GPU, the in-place tail and the pair tail with CFL.
   "headspec"[1] the solver's first V-cycle is queued behind the fused projection head before Σr (residual!'s mean-shift test) has been read back — solver! runs at
       least one cycle whatever the norms are; Σr returns with the first iteration's norms, and if the shift was due after all that solve is discarded (inputs untouched)
       and the two-kernel path taken.  Single GPU.  One host round trip per solve fewer.
   "bcdefer"[1] wl_sim_mom_step: BC!(u,U) after the fused conv_diff!+BDIM! is left to the projection that follows — its fused head (and the second tail's flux_out) read U
       on the wall-normal boundary faces, its tail's folded stores rewrite every boundary location — two BC! launches fewer per step; results identical on every cell.
       Only where all of that holds (tuple U, single domain, no periodic direction / exit / body, fused head and folded tails in use); wl_sim_phase applies BC! as before.
   "tailfuse"[1, on grids of at least "tailfuse_min" interior cells] wl_sim_mom_step: the first projection's tail (u −= L∇x, BC!) is evaluated by the
       corrector's conv_diff! loader; the projected predictor velocity is never written (whole tiles, single domain, tuple U, no periodic direction / exit /
       body; results identical).  Setting it to 1 explicitly also sets the gate to 0 (the path at any eligible size); 0 switches it off.
       wl_sim_phase always keeps the tail launch.
   "tailfuse_min"[16 Mi cells = 256³] per handle: the size gate of "tailfuse" (256³ is the smallest size at which it was measured clearly faster; below it
       the separate tail, which can be queued ahead of the solver's convergence read, is kept).  wl_sim_counter("tailfuse_min") reads the gate in force.
   "pdefer"[1] wl_sim_mom_step / wl_sim_mom_steps: a projection tail whose p = x/Δt would be read next by the fused projection head of the same call does not
       store it; that head takes the solver's scaled x and divides on load (same roundings in the same order: identical bits; 4 B/cell less per tail).  The
       predictor's tail when the corrector's head will be fused, the corrector's when another step follows inside wl_sim_mom_steps; the last tail of a call always
       stores.  Not with the sgs model, forcing, a body, slabs, exitBC, a periodic direction or "store_f".  The pressure may end a call in the other of the handle's
       two pressure arrays: wl_sim_field("p") reports the one that holds it; a caller-owned p always receives it (there a single step stores both times).
   "tailwide"[1] the two projection tails run with four x-adjacent cells per thread and 16-byte loads and stores, the plane's x staged through LDS (k_project_wide,
       wl_project.hip): the same statements per cell, the same launches, identical bits.  Where the pair tails run (3-D, constant coefficients, even nx) and,
       in addition, nx·ny is a multiple of 4, nx ≥ 8 and every array of the launch starts on a 16-byte boundary; anything else — and "tailwide" 0 — runs the
       one- and two-cell kernels as before.
   "convf"[1] the tiled conv_diff!+BDIM! evaluates every face flux once (wl_convf.hip); 0: the two-cells-per-thread kernel that re-evaluates upper faces
   "convt_min"[2048] tile-planes below which "convt" leaves the launch to the plane kernel (tests: 0)
   "xdefer"[1] pair smoother: the V-cycle's x += ω·x_c↓ is applied by kernel B together with its own increment (x makes one round trip per smooth!)
       — and, at value 1, kernel A then hands its r′ and ϵ_mid to kernel B as one 16-byte element per cell pair through a line-aligned buffer of the level
       (csrc/wl_abwide.hpp) instead of two dense arrays: single-domain levels without "store_eps", a periodic direction or a body, in the smooth! that absorbs a
       prolongation; 2: the deferred increment with the two dense arrays.  Same bits either way (wl_sim_counter: finest-level smooth! calls that took the buffer)
   "tail_lds"[1] the single-launch coarse tail keeps r, x, ϵ of its levels in LDS (0: in global memory)
   "body_tile"[1] with a body: conv_diff!+BDIM! on the body-free plane ranges through the tiled NoBody kernel ("convt")
   "rskip"[1] the pair smoother's kernel B does not store the residual nobody reads; needs the pair kernels ("fused_smoother", "pair", "constl") and stands down with
       "store_eps", a periodic direction or a body (every coarse level's r, and the finest level's in the iteration at which the last solve of the same projection
       of a step stopped: counted from the second step on; wl_mg_level_field brings that residual up to date when asked)
   "resjac" for tests — 2 (tests): every head is redone through the two-kernel path, and "bcdefer", "pdefer" and "tailspec" are told so in advance and stand down;
       3 (tests): the same, not announced: "bcdefer" and "pdefer" defer and are flushed before the two-kernel head; the gated tail is withheld
   "itmx"[32] solver!'s iteration cap `itmx` (src/MultiLevelPoisson.jl:108)
   Next to one another (tests/optmatrix.py restates these sentences and tests/test_gpu_optmatrix.py holds the path counters to them on every pair of switches):
       the one-launch head needs the constant-coefficient kernels ("constl"), the fused projection ("fuse_p") and the folded mean shift ("defer_shift"), and does not
       run with "store_f", a body, exitBC or a periodic direction; "pdefer", "bcdefer" and "tailspec" build on that head: they stand down wherever it does;
       the gated tail is queued by the speculative first V-cycle: without "headspec", or where the one-launch head does not run, "tailspec" does nothing;
       "bcfold": with bit 1 set, where the tiled kernel runs ("convt"), that kernel has applied BC! itself and "bcdefer" has nothing to defer; "convz" is not the
       fused launch that "bcdefer" defers behind;
       "tailfuse" needs the flux-once tiled launch ("convt", "convf"; not "convz", "convm"), the fused projection ("fuse_p"), constant coefficients ("constl"), a
       folded BC! ("bcfold" not 0) and f not stored ("store_f"); "tailwide" needs the fused projection ("fuse_p") and the constant-coefficient kernels ("constl");
       "xdefer" needs the pair kernels ("fused_smoother", "pair", "constl"); "body_tile" is a branch of the "hybrid" launch, taken for ranges of whole planes when
       f is not stored.  Every switch not named for a path leaves it running. */
int wl_sim_set_option(wl_sim* s, const char* name, int value);
/* "resjac_min", "convt_min", "convt", "convf", "tail_lds", "body_tile", "pair", "jacobi_march", "convm" (and wl_mg_set_fused bits 2 and 5) are PROCESS-wide:
   they choose between kernels that produce identical bits, for every handle of the process.  wl_reset_process_options() restores their defaults. */
int wl_reset_process_options(void);
/* time-dependent but spatially uniform boundary velocity / body force: the host evaluates uBC(i,t₁) and
   g(i,t)+dU(i,t)/dt at t₀ (predictor) and t₁ (corrector) before each mom_step! (src/Flow.jl:156-167, accelerate! :69-73).
   NULL U1 keeps the boundary velocity; NULL a0 and a1 switches the forcing off. */
int wl_sim_set_forcing(wl_sim* s, const float* U1, const float* a0, const float* a1);
int wl_accelerate(float* r, const wl_grid* g, const float a[3], void* stream);   /* accelerate! for a uniform acceleration: r[I,i] += a_i */
/* Built-in sub-grid-scale model of the composite: model 0 = off (default; the step is exactly the one without this call), 1 = Smagorinsky–Lilly.
 * When on, wl_sim_mom_step, wl_sim_mom_steps and wl_sim_phase 1 and 3 do what mom_predict!/mom_correct! do with udf=sgs! (src/Flow.jl:191-193,206-208):
 * wl_sgs after conv_diff! and before accelerate!, on u⁰ in the predictor and on the projected u in the corrector.  Both phases then take the staged sequence
 * conv_diff! -> sgs! -> accelerate! -> BDIM! -> scale_u! -> BC! (r must exist when the model adds to it): the fused conv_diff!+BDIM! launch and what builds on it
 * ("bcdefer", "tailfuse", "lazydt", the body hybrid) stand down.  WL_EINVAL for a 2-D or z-slab handle and for any other `model`. */
int wl_sim_set_sgs(wl_sim* s, int model, float Cs, float Delta);
int wl_sim_update(wl_sim* s, void* stream);             /* update!(pois) after μ₀ changed (measure!, src/WaterLily.jl:148) */
int wl_sim_mom_step(wl_sim* s, void* stream);           /* mom_step!(flow,pois): appends Δt */
/* n × mom_step! in one call — the loop of sim_step!(sim,t_end) without measure! (src/WaterLily.jl:136-139 with remeasure=false).  Same results as n calls of
   wl_sim_mom_step; between its steps the library may keep Δt on the device until the next predictor has been queued (option "lazydt"): one host round trip per
   step fewer.  The Δt history is complete when the call returns. */
int wl_sim_mom_steps(wl_sim* s, int n, void* stream);
int wl_sim_dt(const wl_sim* s, float* host_out, int cap);      /* flow.Δt (host vector, src/Flow.jl:127) */
double wl_sim_time(const wl_sim* s);                    /* time(flow) = sum(Δt[1:end-1]) :174 */
float wl_sim_dt_last(const wl_sim* s);                 /* Δt[end] */
int wl_sim_set_dt_last(wl_sim* s, float dt);           /* Δt[end] = dt: the host owns flow.Δt (src/Flow.jl:127) and may have changed it */
/* sub-phases for parity tests: 0 u⁰.=u;scale_u!(0) 1 mom_predict! 2 mom_project!(1) 3 mom_correct! 4 mom_project!(.5) 5 push!(Δt,CFL) */
int wl_sim_phase(wl_sim* s, int phase, void* stream);
/* analytic initial conditions evaluated on device (apply!(u0,u), src/Flow.jl:81-83): kind 0 = uBC tuple,
 * 1 = wall-bounded 3-D TGV κ=π/N, 2 = periodic TGV κ=2π/N */
int wl_sim_apply_ic(wl_sim* s, int kind, void* stream);
/* measure!(flow, sphere(c,R); ϵ): closed-form AutoBody sphere/circle (src/Body.jl:28-51, src/AutoBody.jl:29-37) */
int wl_sim_measure_sphere(wl_sim* s, const float* host_center, float R, float eps, void* stream);
/* Closed-form AutoBody shapes (src/AutoBody.jl:21,29-37 with the gradient of the sdf written out; arbitrary Julia sdf/map closures
 * cannot cross a C ABI).  WL_BODY_SPHERE: sdf = |m∘(x−c)|−R — m = (1,1,1) the sphere/circle, an axis with m = 0 is dropped: the
 * cylinder along that axis.  WL_BODY_PLANE: sdf = m·(x−c), m the (not necessarily unit) normal pointing into the fluid.
 * A translating body map(x,t) = x − V·t: the caller passes the current c and V, measure! stores V in flow.V (AutoBody.jl:36-37). */
enum { WL_BODY_SPHERE = 1, WL_BODY_PLANE = 2 };
typedef struct wl_body { int32_t kind; float c[3]; float R; float m[3]; float V[3]; } wl_body;
/* the same on the caller's arrays — what measure!(a::Flow,body), pressure_force(sim), viscous_force(sim) bind for a closed-form body */
int wl_measure_body(float* sigma, float* mu0, float* mu1, float* V, const wl_grid* g, const wl_body* host_body, float eps, int exitBC, uint32_t perdir_mask, void* stream);
int wl_pressure_force_body(const float* p, const wl_grid* g, const wl_body* host_body, double out[3], void* stream);
int wl_viscous_force_body(const float* u, const wl_grid* g, float nu, const wl_body* host_body, double out[3], void* stream);
/* pressure_moment(x₀,p,df,body) / viscous_moment(x₀,u,ν,df,body) (src/Metrics.jl:169-188): moments about host_x0[D]; in 2-D the scalar
 * moment is returned in out[0] and out[1] (the reference's broadcast) */
int wl_pressure_moment_body(const float* host_x0, const float* p, const wl_grid* g, const wl_body* host_body, double out[3], void* stream);
int wl_viscous_moment_body(const float* host_x0, const float* u, const wl_grid* g, float nu, const wl_body* host_body, double out[3], void* stream);
int wl_sim_pressure_moment_body(wl_sim* s, const float* host_x0, const wl_body* host_body, double out[3], void* stream);
int wl_sim_viscous_moment_body(wl_sim* s, const float* host_x0, const wl_body* host_body, double out[3], void* stream);
int wl_sim_measure_body(wl_sim* s, const wl_body* host_body, float eps, void* stream);          /* measure! + update!(pois) */
int wl_sim_pressure_force_body(wl_sim* s, const wl_body* host_body, double out[3], void* stream); /* src/Metrics.jl:116-133 */
int wl_sim_viscous_force_body(wl_sim* s, const wl_body* host_body, double out[3], void* stream);  /* src/Metrics.jl:140-154 */
/* pressure_force(sim) for that sphere (src/Metrics.jl:116-133): Float64 accumulation, does not touch flow.f */
int wl_sim_pressure_force_sphere(wl_sim* s, const float* host_center, float R, double* host_out, void* stream);
int wl_sim_viscous_force_sphere(wl_sim* s, const float* center, float R, double* out, void* stream);   /* viscous_force(sim) src/Metrics.jl:140-154 (single domain) */

/* flow diagnostics (src/Metrics.jl:27-109; wl_flow_stats / wl_flow_fields above) on a handle's CURRENT velocity — roles rotate: the array
 * wl_sim_field(s,"u") names.  Outputs may be the handle's sigma.  The step path is not touched.  A z-slab handle returns WL_EINVAL. */
int wl_sim_flow_stats(wl_sim* s, const float* host_U, double out[3], void* stream);
int wl_sim_flow_fields(wl_sim* s, const float* host_U, float* ke, float* omega3, float* omega_mag, float* lambda2, void* stream);

/* ---- point samples, per-step probe records, tracer particles: src/util.jl:17-43 -------------------------------------------------
 * interp.(x, Ref(arr)) :20-43 on the device.  x: n×D point-major (a Julia Vector{SVector{D,Float32}}); out: n×ncomp point-major.
 * ncomp = 1: arr is a scalar array (Ng...), `interp(x, arr)` :26-28.  ncomp = D: arr is the staggered vector array (Ng...,D), `interp(x, varr)` :20-25 —
 * component i is queried at x + ½·eᵢ (shift :23).  Queries are clamped to [0, Ng_d − 2] per direction (_interp_clamp :17-18), so every x is legal (a NaN
 * coordinate is taken as 0); then x += 1.5, i = floor(x), y = x − i and the weighted sum over the 2^D corners in CartesianIndices order (_interp :29-43; the
 * written order — @fastmath @simd leaves the reference's own open).  One thread per point, one launch; n = 0 returns 0 without one.  out may not overlap arr
 * or x (WL_EINVAL); ncomp other than 1 or D and a z-slab wl_grid return WL_EINVAL — as for every entry point of this section.
 * The last argument of wl_interp, wl_sim_sample and wl_advect is the stream (a hipStream_t as void*, NULL = default), with the contract of the Conventions:
 * the call is asynchronous on it.  Their stream-contract scenarios are tests/test_gpu_streams_interp.py. */
int wl_interp(float* out, const float* arr, const wl_grid* g, const float* x, size_t n, int ncomp, void* hip_stream);
/* the same at n device points of a handle's CURRENT u and p (the arrays wl_sim_field(s,"u") and "p" name: roles rotate): u_out n×D or NULL, p_out n or NULL,
 * one launch for both */
int wl_sim_sample(wl_sim* s, const float* x, size_t n, float* u_out, float* p_out, void* hip_stream);
/* m probe points (host, m×D) and room for `capacity` steps.  After every completed mom_step! of this handle (wl_sim_mom_step, each step of wl_sim_mom_steps) one
 * record is appended on the device: m×(D+1) floats, per probe u(x) (D values) then p(x), interpolated as wl_sim_sample does from that step's final u and p.
 * One launch per step on the step's stream, behind the second projection and ahead of CFL; no host round trip; with probes set the corrector's projection tail
 * stores p where option "pdefer" would skip it (same bits on every cell).  A full buffer drops new records (wl_sim_counter "probe_dropped"; "probe_records":
 * those held).  m = 0 switches recording off.  Setting probes discards records not read yet.  Waits for the device. */
int wl_sim_set_probes(wl_sim* s, const float* host_x, int m, int capacity);
/* copies the records taken since the last read (oldest first) to the host, returns their number in *n_records and the index into flow.Δt of the first one's
 * step in *first_step (record r belongs to step first_step + r; its end time is sum(Δt[1:first_step+r+1])); empties the buffer.  Synchronises the stream the
 * records were taken on.  host_out NULL: a query — the two numbers only, nothing is emptied.  cap_records below the number held: WL_EINVAL, nothing read. */
int wl_sim_read_probes(wl_sim* s, float* host_out, int cap_records, int* n_records, int* first_step);
/* one step of a particle swarm (n×D device positions): x⁰ ← x;  x* = x⁰ + Δt·u⁰(x⁰);  x ← x⁰ + ½Δt·(u⁰(x⁰) + u¹(x*)), u(·) the interp of a vector array above.
 * For a direction j in perdir_mask, x_j is wrapped into [0, N_j) afterwards (N_j interior cells); other coordinates are left free — interp clamps the query,
 * not the particle.  x, x_prev and the velocity arrays may not overlap (WL_EINVAL). */
int wl_advect(float* x, float* x_prev, const float* u0, const float* u1, const wl_grid* g, size_t n, float dt, unsigned perdir_mask, void* hip_stream);
/* tracers of a handle: after every completed mom_step! it calls wl_advect with u0 = the array in the u⁰ role (the velocity the step started from,
 * src/Flow.jl:157), u1 = the step's final u and the Δt the step ran with (the reference's pathline extension advances with Δt[end-1] after the step) — one
 * launch per step, independent of the probes'.  The handle owns x and x⁰ (n×D each, x⁰ = x until the first step); n = 0 frees them.  Waits for the device. */
int wl_sim_set_tracers(wl_sim* s, const float* host_x, size_t n);
float* wl_sim_tracers(wl_sim* s, int which /*0 position, 1 position⁰*/, size_t* n);   /* device pointers, for drawing or wl_d2h */

/* ---- composite bodies: closed-form leaves under rigid maps, combined by set operations (src/Body.jl:91-107, RigidMap.jl) -------
 * A wl_bodyset is a postfix program of at most WL_BODYSET_MAX nodes (evaluation stack at most WL_BODYSET_STACK deep, final depth 1).
 * Leaf kinds are those of wl_body plus WL_BODY_CAPSULE: sdf = |ξ−p|−R, p the point of the segment c ± h·m (m the body-frame axis,
 * normalised by the library, h ≥ 0) closest to ξ — the flat plate of WaterLily cases.  A leaf with mapped=1 is evaluated at the
 * body-frame point ξ = R̂(x−x₀−xₚ)+xₚ of its rigid map; n = R̂ᵀg/|R̂ᵀg|, d = sdf/|R̂ᵀg|, velocity V + ω×(x−x₀−xₚ) (2-D: ω = w[0],
 * ω×b = ω(−b₂,b₁)) (src/AutoBody.jl:29-37).  An unmapped leaf measures exactly as wl_body does, with V = 0.  A fourth kind, WL_BODY_LATTICE, takes its
 * distance from sampled data instead of a formula: see "sampled bodies" below for its fields, its out-of-range rule and the lifetime of what it names.
 * UNION takes the smaller (d,n,V) tuple in Julia's isless order (min), INTERSECT the larger (max), NEGATE gives (−d,−n,V); a − b is
 * a ∩ (−b).  σ holds the raw sdf of a single-leaf program and measure(body,x;fastd²=(2+ϵ)²)[1] otherwise (src/Body.jl:67,74).
 * Malformed programs return WL_EINVAL before anything is launched. */
enum { WL_BODY_CAPSULE = 3 };
enum { WL_OP_LEAF = 0, WL_OP_UNION = 1, WL_OP_INTERSECT = 2, WL_OP_NEGATE = 3 };
#define WL_BODYSET_MAX 16
#define WL_BODYSET_STACK 8
typedef struct wl_rigid_map { float x0[3]; float xp[3]; float R[9]; float V[3]; float w[3]; } wl_rigid_map;   /* R row-major (2-D: upper-left 2x2) */
typedef struct wl_body_node { int32_t op; int32_t kind; float c[3]; float R; float m[3]; float h; int32_t mapped; wl_rigid_map map; } wl_body_node;
typedef struct wl_bodyset { int32_t n; wl_body_node node[WL_BODYSET_MAX]; } wl_bodyset;
/* measure(body,x;fastd²) at npts host points host_x[npts·D] (point-major); writes host_d[npts], host_n[npts·D], host_V[npts·D]; synchronises */
int wl_bodyset_measure_points(const wl_bodyset* host_set, int D, const float* host_x, int npts, float fastd2, float* host_d, float* host_n, float* host_V, void* stream);
/* measure!(flow,body;ϵ) on the caller's arrays: one pass writes every element of σ (interior), μ₀, μ₁, V, then BC!(μ₀), BC!(V) */
int wl_measure_bodyset(float* sigma, float* mu0, float* mu1, float* V, const wl_grid* g, const wl_bodyset* host_set, float eps, int exitBC, uint32_t perdir_mask, void* stream);
/* pressure / viscous force (src/Metrics.jl:116-154); host_x0 non-NULL: the moment about x₀ instead (:169-188, 2-D: out[0] = out[1]) */
int wl_pressure_force_bodyset(const float* host_x0, const float* p, const wl_grid* g, const wl_bodyset* host_set, double out[3], void* stream);
int wl_viscous_force_bodyset(const float* host_x0, const float* u, const wl_grid* g, float nu, const wl_bodyset* host_set, double out[3], void* stream);
int wl_sim_measure_bodyset(wl_sim* s, const wl_bodyset* host_set, float eps, void* stream);       /* measure! + halos + update!(pois), as wl_sim_measure_body */
int wl_sim_pressure_force_bodyset(wl_sim* s, const float* host_x0, const wl_bodyset* host_set, double out[3], void* stream);   /* collective on z-slabs */
int wl_sim_viscous_force_bodyset(wl_sim* s, const float* host_x0, const wl_bodyset* host_set, double out[3], void* stream);

/* ---- sampled bodies: a leaf whose distance comes from data (src/Body.jl:74 measure_sdf!, src/util.jl:17-43 interp, src/AutoBody.jl:29-37) -------
 * A wl_sdf_lattice is what measure_sdf!(a, body) leaves in a scalar array: distances, in flow-grid cells, sampled at the cell centres loc(0,I) = I − 1.5 of
 * its own grid, one ghost layer included — sample i (0-based) of a direction sits at lattice coordinate i − ½.  The leaf WL_BODY_LATTICE is the body
 *     AutoBody((ξ,t) -> interp((ξ .- c) ./ s, A) - R, map)            map: the node's rigid map (mapped = 1) or the identity
 * measured by measure(::AutoBody, x, t; fastd²).  Fields of a wl_body_node of this kind:
 *     c     body-frame position of lattice coordinate 0 (sample i then sits at c + s·(i − ½))
 *     m[0]  s > 0: flow-grid cells per sample interval (m[1], m[2] are ignored).  Distances are NOT rescaled: A holds flow-grid cells whatever s is
 *     R     offset subtracted from the sampled value (R > 0 grows the body)
 *     h     the lattice id, wl_sdf_lattice_id, stored as a float (ids are small positive integers: exactly representable)
 * Value: d = interp(q, A) − R with q = (ξ − c)/s: interp's statements as wl_interp follows them — clamp of q to [0, n_d − 2], + 1.5, floor, the 2^D corners in
 * CartesianIndices order, each weight the product over d left to right, Float32, nothing contracted.  d² > fastd² returns n = V = 0.  Otherwise the gradient
 * is what ForwardDiff gives through _interp: g_d = (Σ_J A[J]·(±1)_d·Π_{e≠d} w_e(J))/s over the same corners in the same order, with i = floor(x) held fixed
 * (the cell to the right of a node is used) and g_d = 0 where the clamp moves q_d; then, as for every leaf, the NaN test, n = R̂ᵀg, m = |n|, d /= m, n /= m
 * and V + ω×(x−x₀−xₚ).  This is the one leaf with m ≠ 1 away from a coordinate scaling.  A lattice leaf composes under UNION / INTERSECT / NEGATE like any other.
 *
 * Out of range is defined: the clamp keeps every index inside the array, so no address outside the lattice is ever formed; a point outside the box
 * q ∈ [0, n_d − 2] reads the value at the nearest point of the box and a zero gradient in the clamped directions.  Such a point must take the early exit, so
 * wl_sdf_lattice_create records edge_min = min |A| over the samples a clamped query reads — the two outermost layers of every direction, between which the
 * faces of the box interpolate — (0 if they differ in sign), and with it |d| ≥ edge_min − |R| outside the box.  Calls that measure fields (wl_measure_bodyset,
 * wl_sim_measure_bodyset) return WL_EINVAL before any launch unless edge_min − |R| > 2 + ϵ + 1 for every lattice leaf; the force calls (wl_*_force_bodyset,
 * wl_sim_*_force_bodyset, wl_sim_forces_bodyset, wl_sim_set_force_record), whose fastd² is 1, unless edge_min − |R| > 2.  wl_bodyset_measure_points applies no
 * rule: it takes the caller's fastd² and returns the clamped value.
 *
 * Lifetime: at most 8 lattices are alive in a process; ids start at 1 and are never reused.  A program that names an unknown or destroyed id is refused with
 * WL_EINVAL before anything is launched.  Programs the library keeps — the force recorder's and that of the last wl_sim_forces_bodyset — are looked up again by
 * id before every launch that uses them: after the lattice is destroyed, wl_sim_mom_step / wl_sim_mom_steps on a handle whose recorder names it return WL_EINVAL
 * and launch nothing (set another recorder body, or switch it off, to go on).  wl_sdf_lattice_destroy waits for the device before it frees.
 *
 * wl_sdf_lattice_create copies host_values[dims[0]·…·dims[D−1]] (first index fastest, offsets 64-bit) to the device on its last argument, the stream (a
 * hipStream_t as void*, NULL = default), and synchronises that stream: host_values are the caller's again when it returns.  Its stream-contract scenario
 * is tests/test_gpu_streams_lattice.py.  WL_EINVAL, with the reason, for D ∉ {2,3}, an extent below 3, a sample that is not finite, and a ninth live lattice. */
enum { WL_BODY_LATTICE = 4 };
typedef struct wl_sdf_lattice wl_sdf_lattice;
int wl_sdf_lattice_create(wl_sdf_lattice** out, int D, const int32_t* dims, const float* host_values, void* hip_stream);
int wl_sdf_lattice_destroy(wl_sdf_lattice* lattice);          /* NULL: nothing to do */
int wl_sdf_lattice_id(const wl_sdf_lattice* lattice);         /* 0 for NULL or a handle that is not alive */

/* ---- sampled bodies from meshes: the exact signed distance to a closed surface, sampled into a lattice on the device ----
 * wl_sdf_lattice_from_mesh fills a lattice of dims[0..D) samples with the Euclidean distance to a closed surface given in the body frame, in flow-grid
 * cells: D = 3 — nv vertices (x,y,z rows) and ne triangles as index triples; D = 2 — nv vertices (x,y rows) and ne segments as index pairs that form one
 * or more closed polygons.  Sample i of direction d sits at origin_d + spacing·((float)i_d − 0.5f), the lattice leaf's own statement (c = origin, m[0] =
 * spacing), so Body(("lattice", …, origin, spacing)) puts the surface where the vertices say.  Orientation is outward: counter-clockwise seen from the fluid,
 * so that the signed volume (area) is positive.  The value is negative inside, positive outside, and d = 0 is stored as +0.
 *
 * Per (sample, element) the closest point is found by the region walk of Ericson (Real-Time Collision Detection §5.1.5: vertex A, B, C, edge AB, BC, CA,
 * face; in 2-D vertex A, B, interior) in Float32, one written order, no contraction; a sample keeps the minimum of d² = |p − q|² over the elements in
 * ascending index with a strict <, and with it the winner's region and p − q.  The sign is that of (p − q)·n with the angle-weighted pseudonormal of the
 * winning feature (Bærentzen & Aanæs 2005: the face normal; the normalised sum of the two adjacent face normals on an edge; the normalised angle-weighted
 * sum of the incident face normals at a vertex; in 2-D the edge normal and the normalised sum of the two adjacent unit edge normals), computed on the host
 * in Float64 and rounded to Float32 once.  The search culls by bounding spheres per brick of 4×4×4 (4×16) samples and is exact: with flags = WL_MESH_BRUTE
 * every pair is tested instead, and both forms store the same bits on every sample (csrc/wl_meshsdf.hip).
 *
 * The result is an ordinary lattice: the same table, the same limit of 8 alive, ids never reused, edge_min recorded from the samples as create records it
 * (wl_sdf_lattice_edge_min; the out-of-range rule above applies unchanged — leave 5 + |R| cells of lattice around the surface).  The call works on
 * hip_stream (uploads, one launch, the read-back) and synchronises it, like wl_sdf_lattice_create.  wl_sdf_lattice_read copies the samples of any live
 * lattice to the host (first index fastest) on hip_stream and synchronises it; the scenario for both is tests/test_gpu_streams_meshsdf.py.
 *
 * WL_EINVAL with the reason, decided on the host before any launch or device allocation — the next valid call goes through — for: D ∉ {2,3}; an extent
 * below 3; a spacing that is not finite or not positive; a non-finite origin or vertex; fewer than 4 vertices / 4 triangles (3 / 3 segments); an index
 * outside [0, nv); a triangle of zero area or a segment of zero length; an edge that is not shared by exactly two triangles in opposite directions (open,
 * non-manifold and inconsistently oriented surfaces, and unwelded triangle soup: weld coincident vertices first); in 2-D a vertex that does not have exactly
 * one incoming and one outgoing segment; a signed volume / area that is not positive (oriented inward: reverse the index order); a ninth live lattice. */
enum { WL_MESH_BRUTE = 1 };   /* flags: no culling */
int   wl_sdf_lattice_from_mesh(wl_sdf_lattice** out, int D, const int32_t* dims, const float* host_origin, float spacing,
                               const float* host_vertices, int32_t nv, const int32_t* host_elems, int32_t ne,
                               unsigned flags, void* hip_stream);
int   wl_sdf_lattice_read(const wl_sdf_lattice* lattice, float* host_values, void* hip_stream);  /* the samples, first index fastest; synchronises */
float wl_sdf_lattice_edge_min(const wl_sdf_lattice* lattice);                                    /* what create recorded; 0 for NULL / not alive */

/* ---- deforming meshes: vertex velocities sampled into the lattice, and re-baking a lattice in place ----
 * A lattice may carry velocity samples W next to its distances A: D component planes of dims[0]·…·dims[D−1] floats each, component-major, first index
 * fastest inside a plane, like every vector array of the library.  They hold the velocity ξ̇ of the surface in the BODY frame, in flow-grid cells per unit
 * time, extended off the surface.  The leaf WL_BODY_LATTICE of such a lattice, past the d² > fastd² exit and the NaN exit (where n = V = 0 stays), samples
 *     ωξ_c = interp(q, W_c),  c < D          the cell, the weights and the clamp of the distance; the 2^D corners in the same order, Float32, uncontracted
 * and returns   unmapped: V = ωξ      mapped: V_a = (V + ω×(x−x₀−xₚ))_a + Σ_q R̂[q][a]·ωξ_q   (the sum left to right from 0; ẋ = R̂ᵀξ̇ + the rigid part —
 * the same R̂ᵀ that carries the gradient to n).  A lattice without velocity samples, and every other leaf, returns the bits it returned before.  The velocity
 * belongs to the lattice: wl_body_node, wl_rigid_map and wl_bodyset are unchanged.
 *
 * wl_sdf_lattice_from_moving_mesh is wl_sdf_lattice_from_mesh — the same refusals, the same search, the same distance bits on every sample — plus velocity
 * samples: host_vertex_velocity holds nv rows of D floats, and each sample stores the velocity of its closest surface point, the winner's vertex velocities
 * wa, wb, wc combined with the barycentric pair (v, w) of the region the walk decided (vertex A (0,0), B (1,0), C (0,1); edge AB (v,0), CA (0,w), BC (1−w,w);
 * face (v,w); 2-D: v ∈ {0, 1, t/den}):   W = wa + v·(wb − wa) + w·(wc − wa)   per component, Float32, in this order, uncontracted — a uniform vertex
 * velocity U gives W = U exactly.  Culled and WL_MESH_BRUTE runs store the same W bits.  On the medial axis of the surface, where the closest point jumps,
 * W is discontinuous; a body's band |d| ≤ 2 + ϵ stays clear of it wherever the surface's radius of curvature does.  Also refused: a NULL or non-finite velocity.
 *
 * wl_sdf_lattice_update_mesh re-bakes a lattice that one of the two mesh calls made, in place, from moved vertices (nv rows, the connectivity of its
 * creation) and, for a lattice with velocity samples, new vertex velocities (NULL = zeros).  Id, dims, origin, spacing and the device pointers stay: every
 * program that names the lattice — a handle's body, a force recorder, the last wl_sim_forces_bodyset — picks the new shape up at its next launch (the force
 * band's tile list is rebuilt by the next measure! of the handle, as after any change of the body).  edge_min is recorded again; a surface that has moved
 * too close to the lattice's edge is refused by the next measure!/force call through the out-of-range rule, not here.  The launch is queued on hip_stream, so
 * earlier work on that stream that reads the lattice is ordered before it (work on OTHER streams that still reads it is the caller's to order); the call
 * synchronises hip_stream.  WL_EINVAL on the host, with nothing launched and samples, velocity samples, edge_min and the kept vertices exactly as they were,
 * for: every mesh refusal of wl_sdf_lattice_from_mesh on the moved vertices (non-finite, zero area, signed volume not positive); a lattice not made from a
 * mesh; a lattice that is not alive; a non-NULL velocity on a lattice made without velocity samples; a non-finite velocity; an unknown flag.
 *
 * wl_sdf_lattice_set_velocity attaches or replaces the velocity samples of ANY live lattice from host_w[D·count] (all finite) — for a caller whose own tool
 * made them; wl_sdf_lattice_read_velocity copies them to the host (WL_EINVAL if there are none); both work on hip_stream and synchronise it.
 * wl_sdf_lattice_has_velocity: 1 / 0 (0 for NULL or a handle that is not alive).  The stream scenario of all of these is tests/test_gpu_streams_meshvel.py. */
int wl_sdf_lattice_from_moving_mesh(wl_sdf_lattice** out, int D, const int32_t* dims, const float* host_origin, float spacing,
                                    const float* host_vertices, int32_t nv, const int32_t* host_elems, int32_t ne,
                                    const float* host_vertex_velocity, unsigned flags, void* hip_stream);
int wl_sdf_lattice_update_mesh(wl_sdf_lattice* lattice, const float* host_vertices, const float* host_vertex_velocity, unsigned flags, void* hip_stream);
int wl_sdf_lattice_set_velocity(wl_sdf_lattice* lattice, const float* host_w, void* hip_stream);
int wl_sdf_lattice_read_velocity(const wl_sdf_lattice* lattice, float* host_w, void* hip_stream);
int wl_sdf_lattice_has_velocity(const wl_sdf_lattice* lattice);

/* ---- band-limited baking: search only the bricks near the surface ----
 * measure! reads a body only in the band |d| ≤ 2 + ϵ (the forces in |d| ≤ 1), yet the calls above search every sample of the lattice.  A lattice made by
 * wl_sdf_lattice_from_mesh_band with a band b > 0 (distance units: flow-grid cells) is the full one, clipped: on EVERY sample it stores, as raw bits,
 *     A_band = clip(A_full, −b, +b)          W_band = W_full where |A_full| ≤ b, else +0.0f in every component   (host_vertex_velocity non-NULL)
 * with A_full, W_full what wl_sdf_lattice_from_mesh / _from_moving_mesh store for the same arguments; a clipped sample holds exactly +b or −b with the sign
 * of A_full (a truncated signed distance field).  edge_min is recorded from the stored, clipped samples by the same function; wl_sdf_lattice_read returns
 * them.  The search skips every brick of 4×4×4 (4×16) samples whose bounding spheres prove it wholly beyond the band — such a brick does not meet the
 * surface, one sign search for its first sample serves all its samples — and clips at the store elsewhere (csrc/wl_meshsdf.hip, k_meshsdf<D, VEL, true>).
 * With WL_MESH_BRUTE every (sample, element) pair is visited, no brick is skipped, and the same clip is applied: the same bits.
 *
 * The band is a property of the lattice, fixed at creation (wl_sdf_lattice_band; 0 for the three other creation calls, which work as ever):
 * wl_sdf_lattice_update_mesh re-bakes with it, and a refused update leaves it, like everything else, as it was.  The call applies every refusal of
 * wl_sdf_lattice_from_mesh (and, with velocities, of _from_moving_mesh), and one more: a band that is not finite and positive — WL_EINVAL with the reason,
 * on the host, before any launch or device allocation.  The limit of 8 alive, ids, the stream behaviour (works on hip_stream and synchronises it; the
 * scenario is tests/test_gpu_streams_meshband.py), wl_sdf_lattice_set_velocity, _read_velocity and _has_velocity are unchanged.
 *
 * The band rule.  For a lattice leaf over a banded lattice baked at spacing s, the calls that apply the out-of-range rule above (edge_min − |R| > need,
 * need = 2 + ϵ + 1 for the calls that measure fields, 2 for the force calls) return WL_EINVAL before any launch unless also
 *     band − |R| > need + s·√D
 * and the message names the condition that failed with both numbers.  s is the spacing recorded at BAKING, not the m[0] of the leaf.
 * wl_bodyset_measure_points applies neither rule.  Why this bound — the surface distance is 1-Lipschitz:
 *   1. if one of the 2^D corners of a query's interpolation cell is clipped, |A_full| > b there, so no surface lies within s√D of that corner (b > s√D):
 *      the whole cell lies on one side of the surface;
 *   2. every corner of the cell then has |A_full| > b − s√D: the stored corners share one sign and each has magnitude ≥ b − s√D;
 *   3. the interpolated value, a convex combination, has |v| ≥ b − s√D up to Float32 rounding, so |v − R| > need: the query takes the leaf's early exit
 *      (d·d > fastd²), and the full lattice makes the same query take it for the same reason;
 *   4. conversely a query that does not exit reads unclipped corners only: the value, gradient and velocity bits of the full lattice.
 * So μ₀, μ₁, V, the force terms and every step are those of the full lattice bit for bit, under UNION / INTERSECT / NEGATE as well (a far leaf loses or
 * wins a min / max identically; where it wins, both results are beyond the exit).  Only σ differs, and only where |σ_full| > 2 + ϵ: there it keeps its
 * sign and stays above that magnitude. */
int   wl_sdf_lattice_from_mesh_band(wl_sdf_lattice** out, int D, const int32_t* dims, const float* host_origin, float spacing,
                                    const float* host_vertices, int32_t nv, const int32_t* host_elems, int32_t ne,
                                    const float* host_vertex_velocity /* NULL: no velocity samples */, float band, unsigned flags, void* hip_stream);
float wl_sdf_lattice_band(const wl_sdf_lattice* lattice);      /* 0 for a lattice without a band, for NULL, for a handle that is not alive */

/* ---- force history: pressure/viscous force and moment of a body after every step, from the body's band only (src/Metrics.jl:116-195) --------
 * nds(body,x) is zero outside |d| ≤ 1, so the sums run over a list of ACTIVE TILES — boxes of 64×4×4 array cells (2-D: 64×4) with an interior cell at
 * d² ≤ 1, found by evaluating the body program on every interior cell, in ascending order, rebuilt only when the body changes.  One launch with one
 * workgroup per active tile evaluates the body once per cell and accumulates all twelve Float64 sums; a single-workgroup finish adds the per-tile
 * partials in list order.  The per-cell Float32 terms are those of the four calls above; only the (fixed) order of the Float64 additions differs.
 * A record is 12 doubles: pressure force [0..2], viscous force [3..5], pressure moment [6..8], viscous moment [9..11] about x₀ (2-D: a vector's third
 * slot is 0, the scalar moment sits in both of the first two).  Single-domain handles created with has_body=1; anything else returns WL_EINVAL.
 *
 * wl_sim_set_force_record: after every completed mom_step! of this handle (wl_sim_mom_step, each step of wl_sim_mom_steps) one record of host_set on the
 * step's final p and u is appended on the device — two launches per step on the step's stream (one for a body with no active tile), behind the second
 * projection and ahead of CFL, no host round trip, the step's bits untouched.  host_x0 NULL: moments about the origin.  A full buffer drops new records
 * (wl_sim_counter "force_dropped"; "force_records": those held; "force_tiles": the list's length).  wl_sim_measure_body / _bodyset / _sphere on a handle
 * with a recorder make the body just measured the recorder's body and rebuild the list (pressure_force(sim) means sim.body as it is now); wl_sim_update
 * leaves it alone.  host_set NULL switches recording off.  Setting discards records not read yet.  Waits for the device. */
int wl_sim_set_force_record(wl_sim* s, const wl_bodyset* host_set, const float* host_x0, int capacity);
/* copies the records taken since the last read (oldest first, [n][12]) to the host; *n_records, *first_step, the query form (host_out NULL) and a too small
 * cap_records (WL_EINVAL, nothing read) as wl_sim_read_probes.  Synchronises the stream the records were taken on; empties the buffer. */
int wl_sim_read_forces(wl_sim* s, double* host_out, int cap_records, int* n_records, int* first_step);
/* the same twelve numbers of host_set now, on the handle's current p and u: builds the list (kept: a repeated call with the same body launches the one
 * pass only), runs it on the stream (a hipStream_t as void*, NULL = default) and reads back once: it synchronises that stream.  Independent of the recorder.
 * The stream-contract scenarios of this section are tests/test_gpu_streams_forces.py. */
int wl_sim_forces_bodyset(wl_sim* s, const float* host_x0, const wl_bodyset* host_set, double out[12], void* hip_stream);

/* ---- mean flow: MeanFlow's time averages P, U and UU = ⟨u⊗u⟩ as an observer of a handle (src/Metrics.jl:205-262) --------
 * The handle owns P (cs floats, cs = cells of one scalar array, ghost cells included), U (D·cs) and — mode 2 — UU, zero-initialised, and the time vector t.
 * UU is stored PACKED: the components i ≤ j only, plane i + j(j+1)/2 of cs floats (3 planes in 2-D, 6 in 3-D); UU[I,i,j] and UU[I,j,i] are the same bits.
 * After every `every`-th completed mom_step! since set/reset (wl_sim_mom_step, each step of wl_sim_mom_steps) ONE launch on the step's stream, behind the second
 * projection and ahead of CFL, applies update! (:236-248) to every cell on the step's final p and u: ε = dt/(dt + (t[end]−t[1]) + eps(Float32)) in Float32 on
 * the host with dt = time(flow) − t[end], ε = 1 on the first update; time(flow) is sum(Δt) with the step's own Δt included, what wl_sim_time returns after the
 * step.  On a step that ends with an update the corrector's projection tail stores p where option "pdefer" would skip it (same bits on every cell); other steps
 * launch nothing and defer as without the observer.  Nothing the step reads is written.  Single-domain handles; a z-slab handle returns WL_EINVAL.
 * Counters: wl_sim_counter "mean_updates" (since set), "mean_every" (0: off).  The stream-contract scenarios are tests/test_gpu_streams_meanflow.py.
 *
 * wl_sim_set_meanflow: mode 0 off (frees the averages), 1 P and U, 2 P, U and UU; t_init NaN: time(flow).  The zero fill goes to `hip_stream`; a change of
 * mode waits for the stream of the last update first.  A failed allocation frees everything and returns the error. */
int wl_sim_set_meanflow(wl_sim* s, int mode, int every, float t_init, void* hip_stream);
/* reset!(meanflow; t_init) :229-234: zeroes the averages (on the stream), t = [t_init] (NaN: time(flow)); the period counts from here */
int wl_sim_meanflow_reset(wl_sim* s, float t_init, void* hip_stream);
/* update!(meanflow, flow) now, on the handle's current u and p with time(flow) = wl_sim_time; independent of `every`; one launch, asynchronous */
int wl_sim_meanflow_update(wl_sim* s, void* hip_stream);
/* device pointer to P (which 0), U (1) or the packed UU (2; NULL unless mode 2) and its length in floats; valid until the next wl_sim_set_meanflow */
float* wl_sim_meanflow(wl_sim* s, int which, size_t* n);
/* the packed UU expanded into the caller's device array out[cs·D·D] in the reference's (N…, D, D) layout; tau != 0: uu!'s τ[I,i,j] = UU[I,i,j] − U[I,i]·U[I,j] (:250-252) */
int wl_sim_meanflow_uu(wl_sim* s, float* out, int tau, void* hip_stream);
/* meanflow.t: copies min(length, cap) entries to host `out` (NULL: none) and returns the length */
int wl_sim_meanflow_t(const wl_sim* s, float* out, int cap);

/* ---- separable terms: position-dependent boundary profiles and body forces (csrc/wl_terms.hip) ---------------------------
 * A closure uBC(i,x,t) or g(i,x,t) cannot cross this boundary; its separable form can:
 *     uBC(i,x,t) = Σₖ bₖ(t)·Fₖ[I,i]        g(i,x,t) = Σₖ gₖ(t)·Fₖ[I,i]        k < K ≤ 4
 * with Fₖ device arrays of the shape of u (cs·D floats) that hold the spatial factor at loc(i,I), and K host coefficients per evaluation.  A steady
 * profile is K = 1, b = 1; the rotating frame of test/test_flow.jl:142-158 is K = 4 with sin/cos coefficients.  accelerate! adds g + ∂ₜuBC on all cells
 * (src/Flow.jl:69-73): the acceleration coefficient of term k is aₖ(t) = gₖ(t) + bₖ′(t), on the same field.
 * The combination is formed in one order, every product and sum rounded to Float32, no term skipped (a zero coefficient is multiplied and added):
 *     s = c₀·F₀[q] ;  s = s + cₖ·Fₖ[q]  for k = 1 … K−1.
 *
 * Leaves on caller arrays (F: K host pointers to device arrays, host_c / host_b: K host floats; asynchronous on hip_stream):
 *   wl_accel_terms    r[q] = r[q] + s over the cs·D elements of r — accelerate!(r,t,g,uBC).  One launch, (K+2)·4 B per element; 16-byte accesses when cs·D
 *                     is a multiple of 4 and r and every Fₖ are 16-byte aligned, one element per thread otherwise (the same statements).
 *   wl_bc_vec_terms   BC!(a,uBC::Function,saveexit,perdir,t) (src/core.jl:201-219): what wl_bc_vec_fn does with Ub = the combination, formed on the fly — only
 *                     the two outermost layers of the non-periodic directions of the Fₖ are read.
 *   WL_EINVAL before any launch for: K outside 1 … 4, a NULL array, an Fₖ that is the output array, a non-finite coefficient.
 *
 * On a handle:
 *   wl_sim_set_terms        the handle allocates K device arrays of cs·D floats, copies host_F[k] into them on hip_stream and synchronises it; it owns them.
 *                           Coefficients in force are dropped.  K = 0 frees the arrays and restores the step of a handle that never had any, exactly.
 *   wl_sim_term             the device pointer of term k, for callers that fill a term on the device (NULL: no such term).
 *   wl_sim_set_term_coeffs  K floats each: acc0 = aₖ(t₀) (predictor), acc1 = aₖ(t₁) (corrector), bc1 = bₖ(t₁) (every BC!(u) of the step).  NULL acc0 and acc1:
 *                           no acceleration from the terms (one of the two NULL: zeros); NULL bc1: the boundary values stay the tuple uBC.  They stay in
 *                           force until the next call, so constant coefficients survive wl_sim_mom_steps.
 * With acceleration coefficients the predictor and the corrector take the staged sequence conv_diff! -> sgs! -> accelerate! -> BDIM! -> scale_u! -> BC!
 * (as for wl_sim_set_forcing, whose uniform launch comes first if it is on too); with boundary coefficients every BC!(u) of the step and of wl_sim_init_flow
 * is the terms kernel (exitBC! is untouched) and nothing folds or defers BC!.  2-D and 3-D, with or without a body or the SGS model.
 * Counters (wl_sim_counter): "term_accel" and "term_bc", launches of the two kernels by this handle so far.
 * WL_EINVAL with the reason, before any launch or allocation, for: a z-slab handle; K outside 0 … 4; a NULL field; a non-finite value in a field; a
 * non-finite coefficient; coefficients given while K = 0.  The stream-contract scenarios are tests/test_gpu_streams_terms.py. */
int wl_accel_terms(float* r, int K, const float* const* F, const float* host_c, const wl_grid* g, void* hip_stream);
int wl_bc_vec_terms(float* a, int K, const float* const* F, const float* host_b, const wl_grid* g, int saveexit, unsigned perdir_mask, void* hip_stream);
int wl_sim_set_terms(wl_sim* s, int K, const float* const* host_F, void* hip_stream);
float* wl_sim_term(wl_sim* s, int k);
int wl_sim_set_term_coeffs(wl_sim* s, const float* acc0, const float* acc1, const float* bc1);

/* ---- multi-GPU: z-slab decomposition, one process per GPU (NEW — the reference has no multi-device path,
 * /root/reference/README.md:153-155).  A wl_comm carries the two primitives the slab path needs, stream-ordered:
 * a nearest-neighbour plane exchange along z and an all-gather; scalars (Σr, L₁, L∞, max σ) are combined on
 * device from an all-gather, so every rank takes identical control-flow decisions.  Two implementations:
 *   rccl      — ncclSend/ncclRecv groups + ncclAllGather on the compute stream (RCCL over xGMI), librccl.so.1
 *               resolved at run time so the process shares PyTorch's copy;
 *   callbacks — host function pointers (tests: torch.distributed/gloo staging through host memory).          */
typedef struct wl_comm wl_comm;
typedef int (*wl_sendrecv_fn)(void* ctx, const void* send_lo, void* recv_lo, const void* send_hi, void* recv_hi, size_t bytes, void* stream);
typedef int (*wl_allgather_fn)(void* ctx, const void* send, void* recv, size_t bytes_each, void* stream);
int wl_comm_rccl_unique_id(char out128[128]);
int wl_comm_rccl_create(wl_comm** out, int rank, int size, const char uid128[128]);
/* 1 when librccl.so.1 and every entry point used here resolved (ranks agree on this BEFORE anyone calls ncclCommInitRank) */
int wl_comm_rccl_available(void);
/* second communicator (its own unique id) for the exchanges that run on the communicator's own HIP stream, overlapped with
 * stencil work: one ncclComm_t is then only ever used from one stream.  Collective: every rank calls it, after _create. */
int wl_comm_rccl_add_async(wl_comm* c, const char uid128[128]);
int wl_comm_callbacks_create(wl_comm** out, int rank, int size, void* ctx, wl_sendrecv_fn sendrecv, wl_allgather_fn allgather);
/* TEST mode of a ONE-rank communicator: both neighbours are this rank (z-periodic wrap onto itself), so that the transport
 * calls a one-rank run would skip (ncclSend/ncclRecv groups, in-place ncclAllGather, the scalar combine) execute on a one-GPU box */
int wl_comm_set_loopback(wl_comm* c, int on);
/* REHEARSAL mode of a ONE-rank RCCL communicator: it reports itself as rank `rank` of `size` — slab geometry, wall logic, exchange pattern and
 * byte counts are those of that rank in a `size`-GPU run — while the planes it sends to a neighbour come back as its own ghost planes and
 * all-gathers fill every rank's block with copies of its own.  The flow is not the P-rank flow (the slab sees itself as its neighbours);
 * what it measures on ONE GPU is the rank's compute per step, its exchange rounds/bytes, and the issue cost of the RCCL calls
 * (tools/slab_rank_bench.py -> profiles/r03_slab8_rank_compute.json).  Call right after wl_comm_rccl_create (+ _add_async). */
int wl_comm_set_virtual(wl_comm* c, int rank, int size);
/* rehearsal transport: 1 (default) = every exchange goes through RCCL to this rank itself; 0 = no transfer at all (ghost planes keep what they hold):
 * the difference between the two runs is what issuing the exchanges costs on this box, the second is the rank's pure compute */
int wl_comm_set_virtual_transport(wl_comm* c, int on);
/* z-periodic domain on z-slabs: the halo exchanges wrap around (rank 0's lower neighbour is the last rank).  wl_sim_create sets it from the
 * descriptor's perdir mask; callback transports get both neighbours on every rank and must address them modulo the size. */
int wl_comm_set_periodic(wl_comm* c, int on);
/* test hooks: the overlapped exchange (begin on the communicator's stream + wait) and the device-side scalar combine
 * (d8/f8: one 128-byte device record, 8 doubles then 8 floats; Σ / max over ranks in place) */
int wl_comm_halo_async(wl_comm* c, float* a, const wl_grid* g, int ncomp, int depth, void* stream);
int wl_comm_combine_test(wl_comm* c, double* d8, float* f8, void* stream);
int wl_comm_destroy(wl_comm* c);
int wl_comm_rank(const wl_comm* c);
int wl_comm_size(const wl_comm* c);
/* counters since creation: {halo exchanges, bytes this rank sent in them, scalar combines (all-gather of 128 B), plane all-gathers} */
int wl_comm_stats(const wl_comm* c, int64_t out4[4]);
/* exchange `depth` z-planes of an (ncomp)-component field with both neighbours (test hook; the composites call it internally) */
int wl_halo_exchange(wl_comm* c, float* a, const wl_grid* g, int ncomp, int depth, void* stream);
/* in-place all-gather of the planes [view->k0,view->k1) each rank computed of a replicated (full) array (test hook) */
int wl_allgather_planes(wl_comm* c, float* a, const wl_grid* view, int ncomp, void* stream);
/* slab grid of `rank` for a GLOBAL ghosted size; halo = ghost planes kept in z (2 for velocity-like fields) */
int wl_grid_slab(wl_grid* out, int D, const int32_t* global_dims_with_ghosts, int rank, int size, int halo);
/* Simulation on a z-slab: desc->dims are the GLOBAL interior sizes; arrays are allocated by the handle (caller pointers must be NULL) */
int wl_sim_create_slab(wl_sim** out, const wl_sim_desc* desc, wl_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* WLHIP_H */
