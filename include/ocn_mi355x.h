/* ocn_mi355x.h -- C ABI of libocn_mi355x.so: the MI355X-native NonhydrostaticModel RK3 time-step hot path.
 *
 * This is the drop-in boundary. The reference (Oceananigans v0.100.5) has no FFI: its seam is Julia dispatch on the
 * architecture type (ext/OceananigansAMDGPUExt.jl:34-113) + `launch!(arch, grid, workspec, kernel!, args...)`
 * (src/Utils/kernel_launching.jl:340-380). A Julia maintainer binds these entry points with `ccall` from methods
 * specialised on a new architecture tag; each entry point below names the reference function
 * (file:line, relative to the reference's src/) whose body it replaces.
 *
 * Conventions
 *  - All array arguments are DEVICE pointers to dense column-major parent arrays WITH halos, exactly the memory of
 *    `parent(field.data)` (src/Grids/new_data.jl:36-73): element (i, j, k) (1-based interior index) lives at
 *    (i-1+Hx) + Px*((j-1+Hy) + Py*(k-1+Hz)), P = N + 2H (+1 for Face fields on Bounded dims, grid_utils.jl:66-72).
 *  - Pointers are BORROWED for the duration of the call; the library never frees caller memory. Objects created by
 *    *_create are owned by the library until *_destroy.
 *  - Every entry point returns int: 0 = ok; negative = invalid argument (mirrors the ArgumentErrors the reference
 *    throws at construction time); positive = hipError_t / hipfftResult (+1000) / ncclResult_t (+2000).
 *    ocn_last_error() returns a thread-local message. The library never aborts.
 *  - All work is enqueued on ONE non-blocking HIP stream per device (the reference runs every kernel on the default
 *    stream in program order, kernel_launching.jl:335-336). Entry points are asynchronous w.r.t. the host unless
 *    stated otherwise; ocn_sync() is `sync_device!` (ext/OceananigansAMDGPUExt.jl:112-113).
 *  - location codes: 0 = Center, 1 = Face. topology codes: 0 = Periodic, 1 = Bounded, 2 = FullyConnected (x), 3 = Flat.
 */
#ifndef OCN_MI355X_H
#define OCN_MI355X_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCN_PERIODIC 0
#define OCN_BOUNDED 1
#define OCN_CONNECTED 2     /* FullyConnected: halo owned by a neighbouring rank (distributed_grids.jl:339-346); x only */
#define OCN_RIGHT_CONNECTED 4   /* first rank of a Bounded partitioned x: wall on the WEST side, neighbour on the east (distributed_grids.jl:339-346) */
#define OCN_LEFT_CONNECTED 5    /* last rank: neighbour on the west side, wall on the EAST side; Face-in-x fields hold Nx + 1 faces (grid_utils.jl:43-68) */
#define OCN_FLAT 3          /* Flat: size 1, halo 0, unit spacing and extent; differences 0, interpolations the identity
                             * (Grids/grid_utils.jl, Operators/difference_operators.jl:30-49, Advection/flat_advective_fluxes.jl) */
#define OCN_CENTER 0
#define OCN_FACE 1

#define OCN_OK 0
#define OCN_EINVAL (-1)      /* invalid argument (ArgumentError in the reference) */
#define OCN_ENOTSUP (-2)     /* configuration outside the accelerated hot path */
#define OCN_ESTATE (-3)      /* call sequence error (e.g. library not initialised) */
#define OCN_EFFT (-4)        /* an FFT plan failed its creation-time round-trip self-check (rocFFT note) */

typedef struct ocn_grid_s *ocn_grid_t;
typedef struct ocn_poisson_s *ocn_poisson_t;
typedef struct ocn_model_s *ocn_model_t;
typedef struct ocn_dist_s *ocn_dist_t;
typedef struct ocn_transposable_s *ocn_transposable_t;   /* TransposableField (transposable_field.jl:5-13) */

/* ---------------------------------------------------------------- runtime (src/Architectures.jl:35-123) ---------- */
int ocn_init(int device_id);                                  /* device!(arch, id) */
int ocn_device_count(int *count);                             /* ndevices(arch) (Architectures.jl; distributed_architectures.jl:284-288 assigns node_rank % ndevices) */
int ocn_sync(void);                                           /* sync_device! */
const char *ocn_last_error(void);
const char *ocn_version(void);
int ocn_malloc(void **ptr, size_t bytes);                     /* zeros(arch, FT, dims...) -- memory is zero-filled */
int ocn_free(void *ptr);                                      /* unsafe_free! */
int ocn_memcpy_h2d(void *dst, const void *src, size_t bytes); /* on_architecture(GPU(), a)  (synchronous) */
int ocn_memcpy_d2h(void *dst, const void *src, size_t bytes); /* on_architecture(CPU(), a)  (synchronous) */
int ocn_memcpy_d2d(void *dst, const void *src, size_t bytes); /* device_copy_to! (stream ordered) */
int ocn_memset_zero(void *dst, size_t bytes);
void *ocn_stream(void);                                       /* the hipStream_t all work is enqueued on */
/* enqueue all subsequent work on a caller-owned stream (e.g. torch.cuda.current_stream(), so RCCL collectives issued
 * through torch.distributed are stream-ordered with the kernels; the reference instead calls sync_device! before every
 * MPI call, halo_communication.jl:181) */
int ocn_set_stream(void *hip_stream);
/* back to a library-owned stream (the state after ocn_init). Time-step graphs (ocn_model_time_step) need it: a borrowed stream
 * may be the legacy default stream, which cannot be captured. */
int ocn_own_stream(void);

/* ---------------------------------------------------------------- grid (src/Grids/rectilinear_grid.jl:3-25) ------ */
/* N, H, topo, L: per dimension. dx, dy: regular spacings. dzc / dzf: HOST arrays of Δzᵃᵃᶜ / Δzᵃᵃᶠ for index
 * k = 1-Hz .. Nz+Hz+1 (length Nz + 2Hz + 1, position k-1+Hz); pass NULL for a z-regular grid (then dz is used).
 * Stretched x / y are outside the hot path -> callers must pass regular dx, dy. */
int ocn_grid_create(ocn_grid_t *grid, const int N[3], const int H[3], const int topo[3], const double L[3],
                    double dx, double dy, double dz, const double *dzc, const double *dzf);
int ocn_grid_destroy(ocn_grid_t grid);
int ocn_grid_parent_size(ocn_grid_t grid, const int loc[3], int P[3]);    /* total_size, grid_utils.jl:138-169 */
/* The node coordinates of the grid, which ocn_grid_create (spacings only) does not know: per direction grid.xᶠᵃᵃ[1], grid.xᶜᵃᵃ[1] and
 * grid.xᶠᵃᵃ[N + 1] (x₀ of fractional_x_index at a Face / a Center, Fields/interpolate.jl:67-83,137-188; xᴸ and xᴿ of
 * enforce_boundary_conditions, lagrangian_particle_advection.jl:158-164). zf / zc: HOST arrays of the Nz + 1 face and Nz centre nodes,
 * required for a stretched z (znodes, :181-188), ignored for a regular one. Needed by ocn_interpolate_at, ocn_advect_particles and
 * ocn_model_set_particles (OCN_ESTATE without it). */
int ocn_grid_set_nodes(ocn_grid_t grid, const double first_face[3], const double first_center[3], const double last_face[3],
                       const double *zf, const double *zc);
/* The node TABLES of the grid: per direction HOST arrays of the N + 1 face nodes grid.xᶠᵃᵃ[1 .. N + 1] and the N centre nodes
 * grid.xᶜᵃᵃ[1 .. N] (one of each in a Flat direction), copied to the device. The reference's nodes are elements of Julia ranges, not
 * x₀ + (i - 1) Δ in floating point, so a kernel that hands coordinates to a user's function reads them from here: needed by
 * ocn_evaluate_boundary_function, ocn_model_set_flux_bc_function, ocn_evaluate_forcing_function and OCN_FORCING_FUNCTION terms
 * (OCN_ESTATE without it). The device block is allocated by the first call and rewritten in place by later ones: the programs a model
 * keeps hold addresses inside it. */
int ocn_grid_set_node_tables(ocn_grid_t grid, const double *const faces[3], const double *const centers[3]);

/* ---------------------------------------------------------------- immersed boundaries (ImmersedBoundaries/) ----- */
/* ImmersedBoundaryGrid(grid, GridFittedBottom | GridFittedBoundary) (immersed_boundary_grid.jl, grid_fitted_bottom.jl:99-130,
 * grid_fitted_boundary.jl): the grid gets a grid-fitted immersed boundary. `immersed_cell` is a HOST array, parent-shaped at (Center,
 * Center, Center), halos filled by the caller, 1 = immersed_cell(i, j, k, ibg); NULL clears the boundary. One kernel builds the two device
 * tables everything else reads (csrc/ocn_immersed.h: the periphery byte replaces inactive_cell / immersed_peripheral_node of
 * immersed_boundary_interface.jl:49-54, the orders word the near_*_immersed_boundary_* tests of Advection/immersed_advective_fluxes.jl:
 * 121-183). Needs a halo of the advection buffer + 1 in every non-Flat direction (inflate_halo_size_one_dimension(req, old, _, ::IBG),
 * OCN_EINVAL otherwise) and must be called before a model is created on the grid (OCN_ESTATE otherwise). */
int ocn_grid_set_immersed_boundary(ocn_grid_t grid, const uint8_t *immersed_cell);
/* copies the periphery bytes and the orders words (parent-shaped at ccc; either pointer may be NULL) to the HOST; OCN_ESTATE on a grid
 * without a boundary */
int ocn_grid_get_immersed_flags(ocn_grid_t grid, uint8_t *periphery, uint16_t *orders);
/* mask_immersed_field!(field, value) (mask_immersed_field.jl:53-64): field = value at immersed_peripheral_node of `loc` over :xyz; nothing
 * on a grid without a boundary (the fallback of :46) */
int ocn_mask_immersed_field(ocn_grid_t grid, double *field, const int loc[3], double value);
/* On a grid with a boundary ocn_compute_Gu/Gv/Gw/Gc, ocn_compute_tendencies, ocn_compute_advective_tendency, ocn_add_fplane_coriolis and
 * ocn_compute_closure_tendencies evaluate the immersed methods (conditional fluxes, the boundary-aware cascade); every other closure entry
 * point, the diagnostics and the partitioned models answer OCN_ENOTSUP there. ocn_model_get_option: "immersed" 0 / 1 and
 * "immersed_tendency_path" (0 no boundary, 1 one field per launch, 2 the flux-sharing role kernel: grids periodic in x and y without a Flat
 * direction under tendency_impl 2; tendency_impl 0 forces path 1; both give the same bits). */

/* ---------------------------------------------------------------- halo fills (BoundaryConditions/) -------------- */
/* fill_halo_regions!(field) with the default boundary conditions of field_boundary_conditions.jl:15-25
 * (Periodic -> PeriodicBC copies, fill_halo_regions_periodic.jl:5-33; Bounded+Center -> no-flux one-cell mirror,
 * fill_halo_regions_flux.jl:9-27; Bounded+Face -> impenetrable wall value, fill_halo_regions_open.jl:2-7, skipped when
 * fill_open_bcs == 0). nfields fields of identical location are filled by ONE launch. */
int ocn_fill_halo_regions(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields, int fill_open_bcs);

/* Non-default boundary conditions with constant values on Bounded sides (BoundaryCondition{<:Flux|Value|Gradient|Open},
 * boundary_condition.jl / boundary_condition_classifications.jl). Sides are ordered west, east, south, north, bottom, top.
 * Value / Gradient fill ONE halo cell by linear extrapolation through the boundary face
 * (fill_halo_regions_value_gradient.jl:7-119), Flux fills like no-flux (fill_halo_regions_flux.jl:9-27) and contributes
 * through ocn_compute_flux_bcs, Open sets the wall-normal component on the boundary face (fill_halo_regions_open.jl:2-7).
 * OCN_BC_DEFAULT = what field_boundary_conditions.jl:15-25 assigns. bcs[f][side]; bcs == NULL: all default. */
#define OCN_BC_DEFAULT 0
#define OCN_BC_FLUX 1
#define OCN_BC_VALUE 2
#define OCN_BC_GRADIENT 3
#define OCN_BC_OPEN 4
/* `array` != NULL: an array-valued condition, getbc(condition::AbstractArray, i, j, grid) = condition[i, j] (boundary_condition.jl:164):
 * a BORROWED device pointer to a dense column-major array over the interior extents of the two tangential directions in the order
 * x before y before z -- west / east: (Ny, Nz), south / north: (Nx, Nz), bottom / top: (Nx, Ny) -- that replaces the number `value`
 * point by point (Flux, Value, Gradient and Open conditions alike). It must stay valid while the condition is in use. */
typedef struct { int kind; double value; const double *array; } ocn_bc_t;
int ocn_fill_halo_regions_bcs(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields,
                              const ocn_bc_t (*bcs)[6], int fill_open_bcs);
/* compute_x_bcs! / compute_y_bcs! / compute_z_bcs! (BoundaryConditions/compute_flux_bcs.jl:12-163), called by
 * compute_flux_bc_tendencies! (compute_nonhydrostatic_tendencies.jl:170-184): G[1] += flux A / V, G[N] -= flux A / V */
int ocn_compute_flux_bcs(ocn_grid_t grid, double *G, const int loc[3], const ocn_bc_t bcs[6]);
/* One side (0 west .. 5 top) of a field-dependent Flux condition of the linear family, flux = a + b dep[i, j, k_boundary]: what
 * getbc(::ContinuousBoundaryFunction) (BoundaryConditions/continuous_boundary_function.jl:128-161) evaluates for
 * func(x, y, t, φ, p) = a + b φ with field_dependencies = :φ when φ sits at the location `loc` of the field that carries the condition
 * (identity interpolation). examples/ocean_wind_mixing_and_convection.jl:125-136: a = 0, b = -evaporation_rate, φ = S. General
 * callables cannot cross a C ABI; this family covers relaxation / evaporation / linear-drag conditions. */
int ocn_compute_linear_flux_bc(ocn_grid_t grid, double *G, const int loc[3], int side, double a, double b, const double *dep);
/* One boundary step of OpenBoundaryCondition(value; scheme = PerturbationAdvection(inflow_timescale, outflow_timescale)) on `side`
 * (0 west .. 5 top) of the wall-normal velocity `field` at `loc`: _fill_west_halo! .. _fill_top_halo! for a PAOBC
 * (BoundaryConditions/perturbation_advection.jl:119-180) with step_left_boundary! / step_right_boundary! (:71-117), operation for
 * operation: Δt = isinf(last_stage_dt) ? 0 : last_stage_dt, U = max(0, min(1, Δt / ΔX ū)) on right sides and min(0, max(-1, .)) on left
 * ones, τ by the sign of ū, the quotient (uᴮ ± U uᴬ + ū Δt/τ) / (1 + Δt/τ ± U), ū where τ == 0. ΔX = Δxᶠᶜᶜ, Δyᶜᶠᶜ or Δzᶜᶜᶠ at the boundary
 * index. ū is `value`, or value_array (see ocn_bc_t) when it is not NULL. One launch, one thread per face point. OCN_EINVAL: a side that is
 * not the wall of a Bounded direction, a field that is not the wall-normal velocity of the side, a negative or NaN timescale. */
int ocn_step_open_boundary(ocn_grid_t grid, double *field, const int loc[3], int side, double value, const double *value_array,
                           double inflow_timescale, double outflow_timescale, double last_stage_dt);
/* open_boundary_mass_inflow (Models/NonhydrostaticModels/boundary_mass_fluxes.jl:47-55,181-198) over the sides of sides_mask (bit s = side
 * s, 0 west .. 5 top): Σ u Axᶠᶜᶜ + Σ v Ayᶜᶠᶜ + Σ w Azᶜᶜᶠ over the left faces minus the same over the right ones, summed on the device in a
 * fixed order (two runs give the same bits). u, v, w: haloed fields, NULL where no side of the mask needs one. Synchronous; a diagnostic.
 * OCN_EINVAL: a side of the mask that is not the wall of a Bounded direction, or whose velocity is NULL. */
int ocn_open_boundary_mass_inflow(ocn_grid_t grid, const double *u, const double *v, const double *w, int sides_mask, double *value);
/* enforce_open_boundary_mass_conservation! (boundary_mass_fluxes.jl:224-239). sides[s]: the condition of the wall-normal velocity on side
 * s -- OCN_BC_OPEN or OCN_BC_DEFAULT --, scheme_mask: the sides whose Open condition carries a scheme. The total is the flux through the
 * scheme faces and the array-valued imposed faces (integrated on the device) plus condition * area of the constant imposed faces
 * (initialize_boundary_mass_flux, :57-79); A is the area of the scheme faces alone, and A⁻¹ ∮u dA is subtracted on left scheme faces and
 * added on right ones (:200-214). Two launches, no atomics, a fixed summation order. Nothing is launched without a scheme side (:216).
 * OCN_EINVAL: another kind of condition, an Open side that is no wall, a scheme bit on a side that is not Open, a NULL velocity a face
 * needs. */
int ocn_enforce_open_boundary_mass_conservation(ocn_grid_t grid, double *u, double *v, double *w, const ocn_bc_t sides[6], int scheme_mask);

/* ---------------------------------------------------------------- tendencies ------------------------------------ */
/* compute_Gu!/Gv!/Gw!/Gc! (Models/NonhydrostaticModels/compute_nonhydrostatic_tendencies.jl:138-163) for
 * advection = WENO(order=5), every other term `nothing`. range = {i0,i1,j0,j1,k0,k1} inclusive 1-based
 * (KernelParameters, kernel_launching.jl:25-95) or NULL for the reference's default launch (:xyz, exclude_periphery
 * for velocities). */
int ocn_compute_Gu(ocn_grid_t grid, const double *u, const double *v, const double *w, double *Gu, const int *range);
int ocn_compute_Gv(ocn_grid_t grid, const double *u, const double *v, const double *w, double *Gv, const int *range);
int ocn_compute_Gw(ocn_grid_t grid, const double *u, const double *v, const double *w, double *Gw, const int *range);
int ocn_compute_Gc(ocn_grid_t grid, const double *u, const double *v, const double *w, const double *c, double *Gc,
                   const int *range);
/* compute_interior_tendency_contributions! (…tendencies.jl:49-131): all of Gu, Gv, Gw and ntracers Gc in one fused,
 * flux-sharing pass. */
int ocn_compute_tendencies(ocn_grid_t grid, const double *u, const double *v, const double *w,
                           const double *const *tracers, int ntracers,
                           double *Gu, double *Gv, double *Gw, double *const *Gc, const int *range);
/* One advection term with the advecting velocities apart from the advected field: G = -div(advection, (ua, va, wa), psi), or with
 * accumulate != 0 G = G - div(...). which: 0 div_𝐯u, 1 div_𝐯v, 2 div_𝐯w (Advection/momentum_advection_operators.jl:46-83; psi and G at
 * the location of u / v / w), 3 div_Uc (tracer_advection_operators.jl:29-33; psi and G at ccc). These are the two terms a model with
 * background_fields evaluates per field (nonhydrostatic_tendency_kernel_functions.jl:86-94,148-156,213-221,276-293). All arrays are
 * haloed parents with filled halos; range as for ocn_compute_Gu; entries outside it keep their bits. Follows option "tendency_impl":
 * 2 on a grid the role kernel serves (x, y Periodic, no Flat or reduced-order direction, option "arithmetic" 0) is one launch of the
 * split role kernel, anything else the per-field kernel. */
int ocn_compute_advective_tendency(ocn_grid_t grid, const double *ua, const double *va, const double *wa, const double *psi, int which,
                                   double *G, const int *range, int accumulate);
/* out = a + b over the whole parent array of a field at `loc`, halos included: one IEEE addition per element, what an access to the
 * reference's SumOfArrays{2} computes (Utils/sum_of_arrays.jl:23,39-41) -- the total velocities u + Ū of a model with background fields */
int ocn_sum_parent(ocn_grid_t grid, const double *a, const double *b, const int loc[3], double *out);
/* the same pass with the rk3_substep! of the NEXT stage (runge_kutta_3.jl:179-226) fused in: when a cell's tendency is
 * complete, U_next = U + dt (gamma Gn + zeta Gm) is written to a SECOND set of prognostic arrays (U itself is still read by
 * neighbouring workgroups); the caller then swaps the two sets. fields / next / Gn / Gm are ordered u, v, w, tracers
 * (3 + ntracers). OCN_ENOTSUP when the fused kernel cannot run on this grid (Bounded x / y). */
int ocn_compute_tendencies_and_substep(ocn_grid_t grid, const double *const *fields, int ntracers, double *const *Gn,
                                       const int *range, double *const *next, const double *const *Gm, double dt,
                                       double gamma, double zeta, int has_zeta);

/* buoyancy, gravity along -z: kind 1 = BuoyancyTracer (bT = the buoyancy tracer), kind 2 = SeawaterBuoyancy with
 * a LinearEquationOfState, b = g (α T - β S) (bT = T). _update_hydrostatic_pressure! (update_hydrostatic_pressure.jl:12-22, over
 * i = 0:Nx+1, j = 0:Ny+1) and the -∂x pHY′, -∂y pHY′ terms of the u, v tendencies (nonhydrostatic_tendency_kernel_functions.jl:
 * 14-19,97,159), added to tendencies that hold the advective part (range: the cells whose tendencies are updated, NULL = all). */
int ocn_update_hydrostatic_pressure(ocn_grid_t grid, int kind, const double *bT, const double *S, double g, double alpha, double beta,
                                    double *pHY);
int ocn_add_hydrostatic_pressure_gradient(ocn_grid_t grid, const double *pHY, double *Gu, double *Gv, const int *range);

/* coriolis = FPlane(f) (Coriolis/f_plane.jl:48-52): G_u -= x_f_cross_U = -f active_weighted_ℑxyᶠᶜᶜ(v), G_v -=
 * y_f_cross_U = f active_weighted_ℑxyᶜᶠᶜ(u) (Operators/interpolation_operators.jl:116-130), on tendencies holding the advective part */
int ocn_add_fplane_coriolis(ocn_grid_t grid, double f, const double *u, const double *v, double *Gu, double *Gv, const int *range);

/* coriolis = ConstantCartesianCoriolis(fx, fy, fz) (Coriolis/constant_cartesian_coriolis.jl:70-81): G_u -= x_f_cross_U = ℑxᶠᵃᵃ(fy ℑzᵃᵃᶜ(w) -
 * fz ℑyᵃᶜᵃ(v)), G_v -= y_f_cross_U = ℑyᵃᶠᵃ(fz ℑxᶜᵃᵃ(u) - fx ℑzᵃᵃᶜ(w)), G_w -= z_f_cross_U = ℑzᵃᵃᶠ(fx ℑyᵃᶜᵃ(v) - fy ℑxᶜᵃᵃ(u)): plain
 * two-point averages, the identity along a Flat direction (Operators/interpolation_operators.jl:87-112), on tendencies holding the
 * advective part (nonhydrostatic_tendency_kernel_functions.jl:96,158,223). range as in ocn_add_fplane_coriolis: the cells whose tendencies
 * are updated, within the interior; NULL = every cell of each field, the wall faces excluded. u, v, w with filled halos. */
int ocn_add_cartesian_coriolis(ocn_grid_t grid, double fx, double fy, double fz, const double *u, const double *v, const double *w,
                               double *Gu, double *Gv, double *Gw, const int *range);

/* stokes_drift = UniformStokesDrift (StokesDrifts.jl:170-178; x_curl_Uˢ_cross_U, y_curl_Uˢ_cross_U, z_curl_Uˢ_cross_U, ∂t_uˢ, ∂t_vˢ), on
 * tendencies that hold everything up to the closure term (nonhydrostatic_tendency_kernel_functions.jl:100-101,162-163,226-227):
 *   G_u = (G_u + ℑxzᶠᵃᶜ(w) dzu_c[k]) + dtu_c[k],  G_v = (G_v + ℑyzᵃᶠᶜ(w) dzv_c[k]) + dtv_c[k],
 *   G_w = (G_w + ((-ℑxzᶜᵃᶠ(u)) dzu_f[k] - ℑyzᵃᶜᶠ(v) dzv_f[k])) + 0
 * with ℑxz = ℑz(ℑx ·) etc. (Operators/interpolation_operators.jl:8-15,50-56), the identity along a Flat direction; every operation a
 * separate IEEE multiply or add. The six tables are DEVICE arrays indexed [k - 1]: ∂z_uˢ / ∂z_vˢ at the centres (Nz values) and at the
 * faces (Nz + 1), ∂t_uˢ / ∂t_vˢ at the centres (Nz); they are read while the kernel runs and not copied. A NULL table is a table of zeros
 * (the products are still formed, as the reference multiplies by its zerofunction). range_u / range_v / range_w: the cells of each
 * velocity whose tendency is updated, within the interior; NULL = every cell of that field, the wall faces excluded. u, v, w with
 * filled halos. */
int ocn_add_stokes_drift(ocn_grid_t grid, const double *dzu_c, const double *dzu_f, const double *dzv_c, const double *dzv_f,
                         const double *dtu_c, const double *dtv_c, const double *u, const double *v, const double *w, double *Gu, double *Gv,
                         double *Gw, const int *range_u, const int *range_v, const int *range_w);

/* interpolate(X, field, (ℓx, ℓy, ℓz), grid) (Fields/interpolate.jl:272-336) at n points: out[p] = the trilinear interpolation of `field`
 * (haloed, at `loc`, filled halos) at (x[p], y[p], z[p]). DEVICE pointers. FractionalIndices (:190-262) with a true division for the
 * regular directions and index_binary_search / fractional_index (:30-59) over the nodes of a stretched z; interpolator (:298-310) with
 * unsafe_trunc and the floored mod; _interpolate (:313-336): all eight products, summed left to right. Unlike the reference's @inbounds
 * reads, every corner index is clamped into the parent array, and a NaN or infinite coordinate reads a defined cell (its result is NaN);
 * the clamp changes nothing within one halo cell of the domain. One launch of particle_step_kernel. */
int ocn_interpolate_at(ocn_grid_t grid, int n, const double *x, const double *y, const double *z, const double *field, const int loc[3],
                       double *out);
/* advect_lagrangian_particles! (Models/LagrangianParticleTracking/lagrangian_particle_advection.jl:118-223): x, y, z (DEVICE, n values) move
 * in place by Δt with u, v, w interpolated at them, then enforce_boundary_conditions per direction (:10-46): Bounded bounces with the
 * coefficient of restitution, clamped to the far wall; Periodic wraps with the floored mod; Flat stays. depths (DEVICE, or NULL):
 * _advect_drogued_particles! (drogued_dynamics.jl:45-72) -- the velocities at (x, y, depths[p]), z unchanged. u, v, w with filled halos. */
int ocn_advect_particles(ocn_grid_t grid, int n, double *x, double *y, double *z, const double *depths, double restitution, double dt,
                         const double *u, const double *v, const double *w);
/* The index computation of the two calls above on the HOST -- the same function the kernel runs (interpolator after fractional_x_index /
 * fractional_index, Fields/interpolate.jl:30-83,298-308, with the clamp) -- for n coordinates along one direction with N cells, halo H,
 * topology code topo, at a Face (face != 0) or a Center: idx[2 p], idx[2 p + 1] = i⁻, i⁺ and w[p] = ξ. first_node, spacing: x₀ and Δ of a
 * regular direction; nodes: the HOST node table of a stretched one (N + 1 faces / N centres), else NULL. Needs no device and no ocn_init. */
int ocn_particle_indices_host(int N, int H, int topo, int face, double first_node, double spacing, const double *nodes, int n,
                              const double *coordinate, int *idx, double *w);

/* buoyancy = BuoyancyForce(formulation; gravity_unit_vector) (BuoyancyFormulations/buoyancy_force.jl:47-54): with ĝ = -gravity_unit_vector,
 * G_u += x_dot_g_bᶠᶜᶜ = ghat_x ℑxᶠᵃᵃ(b), G_v += y_dot_g_bᶜᶠᶜ = ghat_y ℑyᵃᶠᵃ(b) (g_dot_b.jl:2-3; nonhydrostatic_tendency_kernel_functions.jl:
 * 95,157), b the buoyancy perturbation of `kind` as in ocn_update_hydrostatic_pressure (bT, S with filled halos); range as above. */
int ocn_add_buoyancy_acceleration(ocn_grid_t grid, int kind, const double *bT, const double *S, double g, double alpha, double beta,
                                  double ghat_x, double ghat_y, double *Gu, double *Gv, const int *range);
/* _update_hydrostatic_pressure! (update_hydrostatic_pressure.jl:12-22) with z_dot_g_bᶜᶜᶠ = ghat_z ℑzᵃᵃᶠ(b) (g_dot_b.jl:4): ghat_z = 1 gives
 * the bits of ocn_update_hydrostatic_pressure */
int ocn_update_hydrostatic_pressure_tilted(ocn_grid_t grid, int kind, const double *bT, const double *S, double g, double alpha, double beta,
                                           double ghat_z, double *pHY);

/* closure = ScalarDiffusivity(ν, κ): isotropic, constant, explicit (SURVEY.md 8f.1 -- the first "next" row).
 * ∂ⱼ_τ₁ⱼ / ∂ⱼ_τ₂ⱼ / ∂ⱼ_τ₃ⱼ / ∇_dot_qᶜ (TurbulenceClosures/closure_kernel_operators.jl:22-48) with viscous_flux_* = -2 ν Σᵢⱼ and
 * diffusive_flux_* = -κ ∂c (abstract_scalar_diffusivity_closure.jl:194-242). ADDS the closure term to tendencies that already
 * hold the advective part, in the order of nonhydrostatic_tendency_kernel_functions.jl:91-100: G = (G - ∂ⱼτᵢⱼ) + 0.
 * kappa: one value per tracer. range as in ocn_compute_tendencies. */
int ocn_compute_closure_tendencies(ocn_grid_t grid, const double *u, const double *v, const double *w,
                                   const double *const *tracers, int ntracers, double nu, const double *kappa,
                                   double *Gu, double *Gv, double *Gw, double *const *Gc, const int *range);
/* the explicit part of closure = ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν, κ) on a vertically Bounded grid
 * (abstract_scalar_diffusivity_closure.jl:245-291): as above, but only the z fluxes at the indices k == 1 | k == Nz + 1 are the explicit
 * ones; elsewhere viscous_flux_uz = -(ν ∂xᶠᶜᶠ w), viscous_flux_vz = -(ν ∂yᶜᶠᶠ w), viscous_flux_wz = 0, diffusive_flux_z = 0.
 * OCN_EINVAL when z is not Bounded. */
int ocn_compute_closure_tendencies_vertically_implicit(ocn_grid_t grid, const double *u, const double *v, const double *w,
                                                       const double *const *tracers, int ntracers, double nu, const double *kappa,
                                                       double *Gu, double *Gv, double *Gw, double *const *Gc, const int *range);
/* implicit_step!(field, implicit_solver, closure, ..., Δt) of one field for constant coefficients (TurbulenceClosures/
 * vertically_implicit_diffusion_solver.jl:58-121,189-213; solve! of Solvers/batched_tridiagonal_solver.jl:110-133,219-245): solves
 * (1 - Δt ∂z coef ∂z) ϕ = ϕ in place over the columns (1..Nx, 1..Ny) and the levels 1..Nz of a haloed field at the location of u, v, w or
 * a tracer; coef = ν for velocities, κ for the tracer. form: 0, the reference-shaped kernel (every thread runs the reference's loop for
 * its column, scratch t in memory) -- the tuned forms that were tried measured slower and are not shipped, any other
 * value answers OCN_EINVAL. OCN_EINVAL when z is not Bounded. */
int ocn_implicit_step_z(ocn_grid_t grid, double *field, const int loc[3], double coef, double dt, int form);
/* the same with the coefficients read from ccc arrays with filled halos -- the eddy viscosity / diffusivities of an LES closure,
 * interpolated to the flux locations (abstract_scalar_diffusivity_closure.jl:310-330: ν[i,j,k], ℑxyᶠᶠᵃ, ℑxzᶠᵃᶠ, ℑyzᵃᶠᶠ, ℑxᶠᵃᵃ, ...) */
int ocn_compute_closure_tendencies_field(ocn_grid_t grid, const double *u, const double *v, const double *w,
                                         const double *const *tracers, int ntracers, const double *nu_e,
                                         const double *const *kappa_e, double *Gu, double *Gv, double *Gw, double *const *Gc,
                                         const int *range);
/* compute_diffusivities!(diffusivity_fields, closure::AnisotropicMinimumDissipation, model; parameters = :xyz)
 * (turbulence_closure_implementations/anisotropic_minimum_dissipation.jl:152-216; Cb = nothing): νₑ and κₑ[t] over the interior from
 * fields with filled halos; the caller fills the halos of the results (ocn_fill_halo_regions, default conditions).
 * range: NULL = the interior (:xyz), or {i0, i1, j0, j1, k0, k1} reaching at most H - 1 cells into the halos -- an x-slab rank
 * computes i = 0 and Nx + 1 from its exchanged velocity / tracer halos instead of exchanging νₑ, κₑ. */
int ocn_compute_amd_diffusivities(ocn_grid_t grid, double Cnu, const double *Ckappa, const double *u, const double *v,
                                  const double *w, const double *const *tracers, int ntracers, double *nu_e,
                                  double *const *kappa_e, const int *range);
/* compute_diffusivities!(diffusivity_fields, closure::Smagorinsky, model; parameters) (turbulence_closure_implementations/Smagorinskys/
 * smagorinsky.jl:92-127): νₑ = (cs² Δᶠ²) sqrt(2 Σ²) with Σ² = ΣᵢⱼΣᵢⱼᶜᶜᶜ (scale_invariant_operators.jl:10-13; strain components
 * velocity_tracer_gradients.jl:25-46) and Δᶠ = cbrt(Δx Δy Δz). lilly == 0: cs² = C² (Smagorinsky(coefficient = C)); lilly != 0:
 * cs² = ς C², ς = Σ² == 0 ? 0 : sqrt(1 - min(1, Cb max(0, N²) / Σ²)), N² = ℑzᵃᵃᶜ(∂z_b) (lilly_coefficient.jl:129-142) with ∂z_b of
 * buoyancy_kind 0 (nothing: 0), 1 (BuoyancyTracer, b_or_T = b: BuoyancyFormulations/buoyancy_tracer.jl:16) or 2 (linear SeawaterBuoyancy,
 * b_or_T = T, S: g (α ∂z T - β ∂z S), seawater_buoyancy.jl:219-224). Fields with filled halos; the caller fills the halos of νₑ.
 * range as in ocn_compute_amd_diffusivities. */
int ocn_compute_smagorinsky_viscosity(ocn_grid_t grid, double C, double Cb, int lilly, int buoyancy_kind, const double *b_or_T,
                                      const double *S, double g, double alpha, double beta, const double *u, const double *v,
                                      const double *w, double *nu_e, const int *range);
/* ONE coefficient update of a dynamic Smagorinsky closure on caller arrays: compute_coefficient_fields! once its schedule has fired
 * (Smagorinskys/dynamic_coefficient.jl:194-217 for a DirectionallyAveragedCoefficient, :292-330 for LagrangianAveraging), that is
 * _compute_Σ!, _compute_Σ̄! (:142-158), _compute_LM_MM! (:160-188; the operators of scale_invariant_operators.jl:47-188) and then
 *   averaging_mask 1..7 (bit d = direction d + 1): J_LM = Average(LM, dims), J_MM = Average(MM, dims) as ocn_reduce_operation forms them
 *                    (the metric where a stretched z is averaged); J_LM, J_MM are reduced fields (no halo and one point along an
 *                    averaged direction). J_LM_prev, J_MM_prev are not read (NULL).
 *   averaging_mask 0 (LagrangianAveraging): parent(J_prev) <- parent(J); initialising != 0: J <- LM, MM, then the WHOLE parent
 *                    <- max(mean(J_LM), minimum_numerator) and mean(J_MM) (:318-321); else _lagrangian_average_LM_MM! (:241-290) with
 *                    Δt = dt writes the interior of J. LM, MM are not written (NULL). Needs ocn_grid_set_nodes / _node_tables
 *                    (OCN_ESTATE).
 * u, v, w: parent arrays with filled halos. Sigma, Sigma_bar, LM, MM: ccc parent arrays whose interior is written; the halo of Sigma is
 * never read (the reference never fills it: a neighbour outside the interior counts as 0). OCN_EINVAL on a Flat direction, halos
 * below 2 or a missing array; OCN_ENOTSUP on a connected topology. */
int ocn_dynamic_smagorinsky_update(ocn_grid_t grid, const double *u, const double *v, const double *w, int averaging_mask,
                                   double minimum_numerator, double dt, int initialising, double *Sigma, double *Sigma_bar, double *LM,
                                   double *MM, double *J_LM, double *J_MM, double *J_LM_prev, double *J_MM_prev);
/* _compute_smagorinsky_viscosity! (smagorinsky.jl:92-106) with square_smagorinsky_coefficient of a dynamic closure
 * (dynamic_coefficient.jl:129-140): νₑ = (cs² Δᶠ²) sqrt(2 Σ²), cs² = J_MM > 0 ? max(J_LM, minimum_numerator) / J_MM : 0, over the
 * interior. J_LM, J_MM laid out as ocn_dynamic_smagorinsky_update leaves them for averaging_mask. */
int ocn_compute_dynamic_smagorinsky_viscosity(ocn_grid_t grid, int averaging_mask, double minimum_numerator, const double *J_LM,
                                              const double *J_MM, const double *u, const double *v, const double *w, double *nu_e);
/* ocn_compute_closure_tendencies_field for a Smagorinsky closure: the momentum terms with νₑ, tracer t's with κ = ℑ(νₑ) / Pr[t] at its
 * flux points -- interpolate, then divide (κᶠᶜᶜ, κᶜᶠᶜ, κᶜᶜᶠ, smagorinsky.jl:141-143) */
int ocn_compute_closure_tendencies_smagorinsky(ocn_grid_t grid, const double *u, const double *v, const double *w,
                                               const double *const *tracers, int ntracers, const double *nu_e, const double *Pr,
                                               double *Gu, double *Gv, double *Gw, double *const *Gc, const int *range);

/* ---------------------------------------------------------------- RK3 (TimeSteppers/runge_kutta_3.jl) ----------- */
/* rk3_substep_field! (:212-226), launched with exclude_periphery (:187). has_zeta == 0 selects the first-stage
 * method `U += Δt γ¹ G¹`. */
/* ab2_step_field! (TimeSteppers/quasi_adams_bashforth_2.jl:160-173), launched with exclude_periphery: U += Δt ((3/2 + χ) Gⁿ -
 * (1/2 + χ) G⁻); χ = -0.5 is the forward-Euler step (G⁻ is not read) */
int ocn_ab2_step(ocn_grid_t grid, double *const *U, const double *const *Gn, const double *const *Gm, const int (*locs)[3],
                 int nfields, double dt, double chi);
int ocn_rk3_substep(ocn_grid_t grid, double *const *U, const double *const *Gn, const double *const *Gm,
                    const int (*locs)[3], int nfields, double dt, double gamma, double zeta, int has_zeta);
/* _cache_field_tendencies! (TimeSteppers/store_tendencies.jl:6-9) */
int ocn_cache_tendencies(ocn_grid_t grid, double *const *Gm, const double *const *Gn, const int (*locs)[3], int nfields);

/* ---------------------------------------------------------------- pressure -------------------------------------- */
/* _compute_source_term! / _fourier_tridiagonal_source_term!(ZDirection) (solve_for_pressure.jl:12-18, 36-42).
 * rhs: interleaved complex double, dense (Nx, Ny, Nz). */
int ocn_compute_source_term(ocn_grid_t grid, const double *u, const double *v, const double *w, double *rhs_complex,
                            int weight_by_dz);
/* _make_pressure_correction! (pressure_correction.jl:31-37) */
int ocn_make_pressure_correction(ocn_grid_t grid, double *u, double *v, double *w, const double *p);
/* the same over {i0, i1, j0, j1, k0, k1} (NULL = everything): an x-slab rank corrects its two boundary strips first, starts the
 * halo exchange of the next update_state! and corrects the interior while the halos are in flight */
int ocn_make_pressure_correction_range(ocn_grid_t grid, double *u, double *v, double *w, const double *p, const int *range);
/* _make_pressure_correction! and `pNHS ./= Δt⁺` (pressure_correction.jl:31-50) in one pass over `range` (NULL = everything): p / divisor
 * goes to a SECOND haloed array `p_divided` (other threads still read p), which the caller makes the pressure field afterwards */
int ocn_make_pressure_correction_divide(ocn_grid_t grid, double *u, double *v, double *w, const double *p, double *p_divided,
                                        double divisor, const int *range);
/* `pNHS ./= Δt⁺` (pressure_correction.jl:48-50): interior of a (Center, Center, Center) field */
int ocn_divide_interior(ocn_grid_t grid, double *p, double divisor);

/* ---------------------------------------------------------------- solvers (src/Solvers) ------------------------- */
/* kind 0: FFTBasedPoissonSolver (fft_based_poisson_solver.jl:52-74); kind 1: FourierTridiagonalPoissonSolver with
 * tridiagonal direction z (fourier_tridiagonal_poisson_solver.jl:75-134); kind -1: pick like
 * NonhydrostaticModels.jl:25-40 (regular z -> 0, stretched z -> 1). */
int ocn_poisson_create(ocn_poisson_t *solver, ocn_grid_t grid, int kind);
int ocn_poisson_destroy(ocn_poisson_t solver);
int ocn_poisson_kind(ocn_poisson_t solver);
/* device pointer to the complex right-hand-side storage (solver.storage / solver.source_term) */
int ocn_poisson_rhs(ocn_poisson_t solver, double **rhs_complex);
/* solve!(ϕ, solver) (fft_based_poisson_solver.jl:95-125 / fourier_tridiagonal_poisson_solver.jl:212-239): consumes the
 * rhs storage, writes the interior of the haloed (C,C,C) field phi. */
int ocn_poisson_solve(ocn_poisson_t solver, double *phi);
/* solve_for_pressure! (solve_for_pressure.jl:91-95) = source term + solve */
int ocn_solve_for_pressure(ocn_poisson_t solver, const double *u, const double *v, const double *w, double *p);
/* solve_batched_tridiagonal_system_kernel! (batched_tridiagonal_solver.jl:213-245), z direction: a, c length Nz-1,
 * b dense (Nx,Ny,Nz) real, f / phi dense complex, t dense real scratch. */
int ocn_batched_tridiagonal_solve_z(int Nx, int Ny, int Nz, const double *a, const double *b, const double *c,
                                    const double *f_complex, double *t, double *phi_complex);

/* ---------------------------------------------------------------- distributed x-slab pieces --------------------- */
/* fill_send_buffers! / recv_from_buffers! (DistributedComputations/communication_buffers.jl:281-313) for Partition(R):
 * west/east buffers of Hx x Py x Pz doubles per field (whole parent extent in y, z: corners ride along; Py, Pz are
 * each field's own -- Face fields on Bounded dimensions have one more plane), field-major, back to back.
 * The exchange itself (MPI.Isend/Irecv in the reference, halo_communication.jl:300,326) is issued by the host layer
 * over RCCL. */
int ocn_pack_x_halos(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields, double *west_send,
                     double *east_send);
int ocn_unpack_x_halos(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields, const double *west_recv,
                       const double *east_recv);
/* the same with only the `depth` (1 <= depth <= Hx) columns next to each side: buffers of depth x Py x Pz doubles per field.
 * The pressure solve reads one column of x halo (u[Nx+1] in the divergence, p[0] in the correction): the host layer exchanges
 * exactly that between the full fills of update_state!, where the reference's generic fill moves Hx columns of u, v, w
 * (pressure_correction.jl:8-20) that nothing reads before they are filled again. */
int ocn_pack_x_halos_depth(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields, int depth,
                           double *west_send, double *east_send);
int ocn_unpack_x_halos_depth(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields, int depth,
                             const double *west_recv, const double *east_recv);
/* DistributedFFTBasedPoissonSolver (distributed_fft_based_poisson_solver.jl:92-188; z Periodic) and
 * DistributedFourierTridiagonalPoissonSolver (distributed_fft_tridiagonal_solver.jl:153-293; z Bounded, regular or
 * stretched) for Partition(R,1,1), split at the two transposes (MPI.Alltoallv!, distributed_transpose.jl:185-191) which
 * the host layer runs as RCCL all-to-alls on the send/recv buffers:
 *   source_term -> forward_yz -> [all_to_all(recv, send)] -> solve_x -> [all_to_all(recv, send)] -> backward_yz -> phi.
 * The right-hand side is real, so only the y modes 0..Ny/2 travel (half the reference's bytes): send/recv hold
 * `buffer_size` complex elements = R equal chunks of (Nxl, ceil((Ny/2+1)/R), Nz). */
typedef struct ocn_dist_poisson_s *ocn_dist_poisson_t;
int ocn_dist_poisson_create(ocn_dist_poisson_t *solver, ocn_grid_t local_grid, int R, int rank, double Lx_global);
int ocn_dist_poisson_destroy(ocn_dist_poisson_t solver);
int ocn_dist_poisson_buffer_size(ocn_dist_poisson_t solver, size_t *complex_elements);
int ocn_dist_poisson_set_buffers(ocn_dist_poisson_t solver, double *send_complex, double *recv_complex);
/* compute_source_term! (solve_for_pressure.jl:12-84) into the solver's own storage */
int ocn_dist_poisson_source_term(ocn_dist_poisson_t solver, const double *u, const double *v, const double *w);
int ocn_dist_poisson_forward_yz(ocn_dist_poisson_t solver);
/* z Periodic and option "dist_substructured" = 1 (default): after the local (y, z) transform every mode is a periodic constant-
 * coefficient tridiagonal system along the partitioned x direction; it is solved by substructuring -- Thomas sweeps on the slab, an
 * ALL-GATHER of 2 values per mode (payload_size complex elements per rank, ~1 MB at 256^3) instead of the two all-to-alls of the
 * whole spectrum, a 2x2 solve per mode and rank-DFT index, a slab correction:
 *   source_term -> forward_local -> [all_gather(gathered, payload)] -> backward_local -> phi.
 * Same solution as the transposed FFT solve to round-off. payload_size = 0: the solver transposes (stages above). */
int ocn_dist_poisson_payload_size(ocn_dist_poisson_t solver, size_t *complex_elements);
/* which local layout the substructured solve runs on (diagnostic): 3 = z-fastest real array, 1-D R2C / C2R plans along z and the y
 * pass by the library's own LDS column-FFT kernel (Ny = 2^m <= 512; default); 2 = z-fastest real array, ONE 2-D (y, z) R2C / C2R plan batched over
 * the local x index, spectrum already in the order of the Thomas sweeps; 1 = the same with 1-D plans (rocFFT refuses the
 * 2-D interleaved-batch layout for some small sizes); 0 = paired real columns + Hermitian separation (option dist_zfirst = 0);
 * -1 = transposing solver */
int ocn_dist_poisson_layout(ocn_dist_poisson_t solver, int *layout);
int ocn_dist_poisson_set_gather_buffers(ocn_dist_poisson_t solver, double *payload_complex, double *gathered_complex);
int ocn_dist_poisson_forward_local(ocn_dist_poisson_t solver);
int ocn_dist_poisson_backward_local(ocn_dist_poisson_t solver, double *phi);
int ocn_dist_poisson_solve_x(ocn_dist_poisson_t solver);
int ocn_dist_poisson_backward_yz(ocn_dist_poisson_t solver, double *phi);

/* ---------------------------------------------------------------- model fast path ------------------------------- */
/* NonhydrostaticModel(; grid, advection = WENO(), tracers, timestepper = :RungeKutta3) with coriolis / buoyancy /
 * closure / forcing = nothing (nonhydrostatic_model.jl:115-244); the ocn_model_set_* calls below add them. Fields are allocated (zeroed)
 * by the library. */
int ocn_model_create(ocn_model_t *model, ocn_grid_t grid, int ntracers);
int ocn_model_destroy(ocn_model_t model);
/* names: "u","v","w","c0".."c7" (tracers), "p" (pNHS), "Gu".."Gc7" (Gⁿ), "Mu".."Mc7" (G⁻). Returns the device
 * pointer of the parent array and its location. Pointers stay valid for the model's lifetime and are stable at
 * time-step boundaries. */
int ocn_model_field(ocn_model_t model, const char *name, double **ptr, int loc[3]);
/* update_state!(model; compute_tendencies) (update_nonhydrostatic_model_state.jl:20-56). As in the reference the tendencies it leaves carry
 * no Flux-boundary-condition terms: compute_flux_bc_tendencies! belongs to the stage that follows (runge_kutta_3.jl:118,134,150). */
int ocn_model_update_state(ocn_model_t model, int compute_tendencies);
/* tail of set!(model; ...) after the interiors were written (set_nonhydrostatic_model.jl:44-57) */
int ocn_model_set_finalize(ocn_model_t model, int enforce_incompressibility);
/* time_step!(model, Δt) (runge_kutta_3.jl:93-170). One call = the three stages; what it leaves is what the reference leaves: the fields,
 * pNHS of the third stage, Gⁿ = G(U³) without Flux-condition terms, G⁻ = G(U¹). Intermediate values nothing can read from outside the call
 * (pNHS of stages 1 and 2, the tendency of the second stage) are not stored: options "skip_stage_pressure", "skip_dead_tendency_store". */
int ocn_model_time_step(ocn_model_t model, double dt);
/* time_step!(model::AbstractModel{<:QuasiAdamsBashforth2TimeStepper}, Δt; euler) (TimeSteppers/quasi_adams_bashforth_2.jl:74-123;
 * SURVEY.md 8f.1): χ = 0.1 is the reference's default; a forward-Euler step is taken when Δt differs from clock.last_Δt (first
 * step) or euler != 0 */
int ocn_model_time_step_ab2(ocn_model_t model, double dt, double chi, int euler);
/* reset!(model.clock); reset!(model.timestepper) (Simulations/simulation.jl:203-213): time = 0, iteration = 0, stage = 1,
 * last_Δt = Inf, Gⁿ = G⁻ = 0. The next time-step starts with update_state! again. */
int ocn_model_reset(ocn_model_t model);
int ocn_model_clock(ocn_model_t model, double *time, int64_t *iteration, int *stage, double *last_dt,
                    double *last_stage_dt);
/* set!(model, checkpointed_clock) (OutputWriters/checkpointer.jl:199-231): restore the clock of a checkpointed state; the fields and
 * the tendencies Gⁿ, G⁻ are restored by copying the checkpointed parent arrays (halos included, like the reference's files) into the
 * arrays ocn_model_field returns, followed by ocn_model_update_state. The coefficient fields of a dynamic Smagorinsky closure are not
 * part of a checkpoint: this call (and ocn_model_reset) sets previous_compute_time to `time` and marks the 𝒥 fields as holding nothing,
 * so the first coefficient update that fires afterwards takes the initialising branch from the restored velocities */
int ocn_model_set_clock(ocn_model_t model, double time, int64_t iteration, int stage, double last_dt, double last_stage_dt);
/* max |∇·u| over the interior (test helper: test/test_time_stepping.jl:124-160); synchronous */
int ocn_model_max_abs_divergence(ocn_model_t model, double *value);
/* cell_advection_timescale(grid, velocities) (Advection/cell_advection_timescale.jl:13-34): min over cells of
 * 1 / (|u|/Δx + |v|/Δy + |w|/Δz) -- what TimeStepWizard multiplies by the CFL number. Synchronous.
 * The raw-pointer form knows no model and no communicator: it reduces over the cells of `grid` only -- on the local grid of a
 * partitioned model that is the rank's own timescale, not the global one. */
int ocn_cell_advection_timescale(ocn_grid_t grid, const double *u, const double *v, const double *w, double *tau);
/* The model form on a partitioned model (ocn_dist_model_create*) returns the minimum over ALL ranks, like the reference's all-reduce
 * (DistributedComputations/distributed_fields.jl:144-196): the maximum of the inverse timescale crosses the model's communicator
 * before the one divide, so every rank gets the bits of the serial model on the global grid. There the call is COLLECTIVE: every
 * rank of the communicator has to make it. */
int ocn_model_cell_advection_timescale(ocn_model_t model, double *tau);
/* hasnan(field) = any(isnan, parent(field)) (Diagnostics/nan_checker.jl:32): `n` doubles starting at `data` (the whole parent
 * array, halos included); *result = 1 if any is NaN */
int ocn_hasnan(const double *data, size_t n, int *result);
int ocn_max_abs_divergence(ocn_grid_t grid, const double *u, const double *v, const double *w, double *value);
/* sets a tuning option of this model only (the keys: ocn_set_option). A creation key fails with OCN_ESTATE, a partitioned key on a
 * single-GPU model with OCN_EINVAL. One more key: "profile" 1 = record HIP events around every tendency evaluation on the launch stream
 * (ocn_model_profile_read). */
int ocn_model_set_option(ocn_model_t model, const char *key, int value);
/* reads this model's value of every option key (ocn_set_option; "fused_step": whether the fused pressure step runs, 0 on a single-GPU
 * model) and what the configuration makes of them: "fused_tendency_active" (1 when a flux-sharing tendency kernel runs for this grid),
 * "fuse_substep_active" (1 when the rk3_substep! of stages 2 and 3 is fused into the preceding tendency evaluation: option
 * "fuse_substep" = 1, flux-sharing kernel, tendencies cached by pointer swap, no Flux boundary condition), "substep_in_tendency_kernel"
 * (1 when that substep rides in the tendency launch itself), "halo_fill_folded" and "stage1_source_fused" (what the last time-step did
 * on a triply periodic grid with the split pressure solve: 1 when the pressure-correction kernel wrote every halo, so that the step
 * launched no halo fill -- option "fused_halo"; 1 when the first RK3 substep rode in the source-term and correction kernels -- option
 * "fuse_substep"), "forcing_path" (ocn_model_set_forcing), "graph_captures",
 * "graph_replays", "graph_failures" (option "use_graph"), which conditional path the model's pressure solver took -- "fused_zfft_active"
 * (1 when solve_for_pressure! runs the z transform, the divide and the inverse z transform as one pass: options "real_fft" and
 * "fused_zfft", FFT solver, Nz = 2^m in 8 .. 1024), "c2r_strided_active" (1 when the Z2D plan writes into the haloed pressure field:
 * options "real_fft" and "c2r_strided" AND rocFFT accepted the plan), "split_solve_active" (1 when the model's pressure step runs the
 * split form -- 1-D x plans on padded rows, the LDS line kernel along y, the correction taken from the dense solution: options
 * "split_solve" and "real_fft", x and y Periodic, Ny = 2^m in 8 .. 1024, Fourier-tridiagonal solver or fused z transform, AND the split
 * form passed its self-check at creation; the 2-D plans run otherwise); all three 0 on a partitioned model -- and, on a partitioned model,
 * "dist_poisson_layout", "dist_yline_active" (1 when the local y transform runs in the LDS line kernel: option "dist_yline", z Bounded,
 * Ny = 2^m in 8 .. 1024 and the kernel passed its check at creation) and "dist_xline_group_active" (1 when the Thomas scans of the
 * x-fastest solve run several lines per wave: option "dist_xline_group", local Nx 32, 64 or 128); both 0 on a single-GPU model */
int ocn_model_get_option(ocn_model_t model, const char *key, int *value);
/* boundary_conditions = (name = FieldBoundaryConditions(side = BoundaryCondition(kind, value)),) of the model
 * constructor (nonhydrostatic_model.jl:115-244); name "u","v","w","c0".. and, with an LES closure, the diffusivity fields "nu_e",
 * "kappa_e0".. (Value / Gradient; boundary_conditions = (κₑ = (b = ...,),)); side 0..5 = west .. top. OCN_EINVAL mirrors
 * the reference's validation: Bounded sides only; Flux/Value/Gradient on Center-located, Open on Face-located fields */
/* buoyancy = nothing (kind 0) | BuoyancyTracer() (kind 1, tracer index) | SeawaterBuoyancy(LinearEquationOfState(α, β), g)
 * (kind 2, tracer indices of T and S). With buoyancy the model carries the hydrostatic pressure anomaly, field name "pHY"
 * (nonhydrostatic_model.jl:144-158). */
int ocn_model_set_buoyancy(ocn_model_t model, int kind, int b_or_T_index, int S_index, double g, double alpha, double beta);
/* coriolis = FPlane(f = f) of the model constructor; enabled = 0: coriolis = nothing */
int ocn_model_set_coriolis(ocn_model_t model, int enabled, double f);
/* coriolis = ConstantCartesianCoriolis(fx, fy, fz) of the model constructor (constant_cartesian_coriolis.jl:32-66); enabled = 0: coriolis =
 * nothing. The model has ONE Coriolis: this and ocn_model_set_coriolis replace one another. The w tendency then has a Coriolis term too
 * (nonhydrostatic_tendency_kernel_functions.jl:223). OCN_ENOTSUP on a partitioned model. ocn_model_get_option answers "coriolis_kind":
 * 0 nothing, 1 FPlane, 2 ConstantCartesianCoriolis. */
int ocn_model_set_cartesian_coriolis(ocn_model_t model, int enabled, double fx, double fy, double fz);
/* buoyancy = BuoyancyForce(formulation; gravity_unit_vector = (gx, gy, gz)) (buoyancy_force.jl:47-54) for the formulation
 * ocn_model_set_buoyancy names; enabled = 0: NegativeZDirection(). The u and v tendencies gain x_dot_g_b, y_dot_g_b and the hydrostatic
 * pressure anomaly integrates ĝ_z ℑzᵃᵃᶠ(b) (g_dot_b.jl:2-4). OCN_EINVAL unless the components are finite and gx² + gy² + gz² ≈ 1
 * (validate_unit_vector, Grids/input_validation.jl:177-186: isapprox, rtol = √eps); OCN_ENOTSUP on a partitioned model.
 * ocn_model_get_option answers "tilted_gravity" (1 with a buoyancy and a gravity_unit_vector). Models with either of these two take the
 * per-value tendency epilogue: "epilogue_march_active" answers 0. */
int ocn_model_set_gravity_unit_vector(ocn_model_t model, int enabled, double gx, double gy, double gz);
/* stokes_drift = UniformStokesDrift(∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ) of the model constructor (StokesDrifts.jl:125-178), evaluated by the caller
 * per level: HOST tables, ∂z at the centres (Nz doubles) and at the faces (Nz + 1), ∂t at the centres (Nz); NULL = zeros. They are copied
 * into device memory the model owns, ordered on the library stream; the call may come between time-steps and replaces any earlier drift
 * whole. enabled = 0: stokes_drift = nothing, the model launches what it launched before (the tables are ignored). The terms follow the
 * closure term and precede the forcing. OCN_EINVAL: NULL model, or a Flat z (a drift that varies with z needs a z direction); OCN_ENOTSUP:
 * a partitioned model; a refused call leaves the model untouched. The tables hold one moment in time: a time-dependent drift is the
 * caller's to refresh between time-steps (all stages of a step then see the same tables). ocn_model_get_option answers "stokes_drift"
 * (0 / 1) and "stokes_path": 0 none, 1 a stand-alone pass (stokes_drift_kernel, after the stand-alone physics kernels: option
 * fused_epilogue = 0, or more linear Flux conditions than the epilogue holds), 2 inside the per-value tendency epilogue (the default;
 * "epilogue_march_active" then answers 0). */
int ocn_model_set_stokes_drift(ocn_model_t model, int enabled, const double *dzu_c, const double *dzu_f, const double *dzv_c,
                               const double *dzv_f, const double *dtu_c, const double *dtv_c);
/* particles = LagrangianParticles(x, y, z; restitution, dynamics) of the model constructor (LagrangianParticleTracking.jl:41-102): HOST
 * arrays of n values, copied into one device block the model owns, ordered on the library stream; replaces the earlier particles whole,
 * their tracked properties included. depths (or NULL): dynamics = DroguedParticleDynamics(depths) (drogued_dynamics.jl:34-72). n = 0 with
 * arrays: zero particles; n = 0 with x = y = z = depths = NULL: particles = nothing, the model launches what it launched before. With
 * particles every RK3 stage ends with step_lagrangian_particles!(model, stage Δt) (runge_kutta_3.jl:128,144,167: γ¹Δt, (γ² + ζ²)Δt and the
 * uncorrected (γ³ + ζ³)Δt) and an AB2 step with step_lagrangian_particles!(model, Δt) (quasi_adams_bashforth_2.jl:108): ONE launch that
 * sets the tracked properties at the position before the move and then moves the particles with total_velocities(model)
 * (nonhydrostatic_model.jl:265-266). OCN_EINVAL: NULL model, n < 0, a NULL array; OCN_ENOTSUP: a partitioned model; OCN_ESTATE: a grid
 * without ocn_grid_set_nodes. A refused call leaves the model untouched. ocn_model_get_option answers "particles" (their number, or 0). */
int ocn_model_set_particles(ocn_model_t model, int n, const double *x, const double *y, const double *z, double restitution,
                            const double *depths);
/* tracked_fields = (property = field,) (LagrangianParticleTracking.jl:89-102; update_lagrangian_particle_properties!,
 * update_lagrangian_particle_properties.jl:6-36): before every move, particles.<property> = the model field `field_name` interpolated at
 * the particles. field_name: "u", "v", "w", "c<n>", "p", "pHY", "nu_e" (as ocn_model_field). At most 8 properties; a property named again
 * takes the new field. OCN_EINVAL: an unknown field, a ninth property, x / y / z as the property; OCN_ESTATE: no particles. */
int ocn_model_track_particle_field(ocn_model_t model, const char *property, const char *field_name);
/* particles.properties.<name> (fetch_output, LagrangianParticleTracking.jl:157-161; the checkpointed `:particles`, checkpointer.jl:60-66):
 * "x", "y", "z", "depths" or a tracked property, n doubles to / from a HOST array, after everything queued on the library stream. */
int ocn_model_particle_property(ocn_model_t model, const char *name, double *host_out);
int ocn_model_set_particle_property(ocn_model_t model, const char *name, const double *host_in);
int ocn_model_particle_count(ocn_model_t model, int *count);           /* length(particles) (:105); 0 for particles = nothing */
/* closure = ScalarDiffusivity(ν = nu, κ = kappa[tracer]) of the model constructor. The model has ONE closure: this replaces any other
 * (an AMD or Smagorinsky closure too: "nu_e" then answers OCN_ESTATE again); all zeros / NULL: closure = nothing */
int ocn_model_set_closure(ocn_model_t model, double nu, const double *kappa);
/* time discretisation of the model's ScalarDiffusivity (scalar_diffusivity.jl:116-141): enabled = 1 is
 * VerticallyImplicitTimeDiscretization() -- the tendencies keep the explicit part only and every substep of RK3 / AB2 is followed by
 * implicit_step! of each prognostic field (runge_kutta_3.jl:179-203, quasi_adams_bashforth_2.jl:127-154); 0 is ExplicitTimeDiscretization().
 * OCN_EINVAL when z is not Bounded ("VerticallyImplicitTimeDiscretization can only be specified on grids that are Bounded in the
 * z-direction.", vertically_implicit_diffusion_solver.jl:149-153); OCN_ENOTSUP with an AMD or Smagorinsky closure, and setting one of
 * those clears it. ocn_model_get_option answers "vertically_implicit", "implicit_step_form" and "epilogue_march_active". */
int ocn_model_set_vertically_implicit(ocn_model_t model, int enabled);
/* closure = AnisotropicMinimumDissipation(Cν = Cnu, Cκ = Ckappa[tracer]) (replaces a ScalarDiffusivity). update_state! then
 * computes the model fields "nu_e", "kappa_e0", ... and fills their halos before the tendencies. */
int ocn_model_set_amd(ocn_model_t model, double Cnu, const double *Ckappa);
/* closure = Smagorinsky(coefficient = C, Pr) (lilly == 0) | SmagorinskyLilly(C, Cb, Pr) (Smagorinskys/smagorinsky.jl:62-83,
 * lilly_coefficient.jl:5-35); Pr: one Prandtl number per tracer. Replaces any other closure. The model then carries "nu_e" only
 * (build_diffusivity_fields, smagorinsky.jl:131-139; "kappa_e*" answers OCN_ESTATE); update_state! computes it with the buoyancy
 * ocn_model_set_buoyancy names at that moment and fills its halos before the tendencies. OCN_EINVAL on a grid with a Flat
 * direction, for C < 0 and for Pr <= 0. */
int ocn_model_set_smagorinsky(ocn_model_t model, double C, double Cb, int lilly, const double *Pr);
/* closure = Smagorinsky(coefficient = DynamicCoefficient(averaging, schedule = IterationInterval(interval, offset), minimum_numerator), Pr)
 * (Smagorinskys/dynamic_coefficient.jl:5-9,114-117; DynamicSmagorinsky, :20-26). averaging_mask: bit d set = direction d + 1 averaged
 * (1..7, DirectionallyAveragedCoefficient), 0 = LagrangianAveraging. Replaces any other closure as ocn_model_set_smagorinsky does. Every
 * update_state! then runs compute_coefficient_fields! (:194-217, :292-330) -- the schedule is (iteration - offset) % interval == 0 on the
 * clock as it stands -- and _compute_smagorinsky_viscosity! with square_smagorinsky_coefficient (:129-140). The model carries "nu_e",
 * "Sigma", "Sigma_bar", "J_LM", "J_MM" and "LM", "MM" (directional; J_LM, J_MM are then reduced fields: one point and no halo along
 * every averaged direction, the parent extent along the others) or "J_LM_prev", "J_MM_prev" (Lagrangian); the names of the other
 * averaging answer OCN_ESTATE. The first update that fires after this call initialises the 𝒥 fields (LagrangianAveraging: the
 * first-time-step branch), also on a model whose clock is past 0. A model with a dynamic coefficient steps without the captured graph. OCN_EINVAL on a grid with a Flat
 * direction or halos below 2, for a mask outside 0..7, interval < 1, a NaN minimum_numerator and Pr <= 0; OCN_ENOTSUP on a partitioned
 * model; OCN_ESTATE for LagrangianAveraging without ocn_grid_set_nodes and ocn_grid_set_node_tables. */
int ocn_model_set_dynamic_smagorinsky(ocn_model_t model, int averaging_mask, double minimum_numerator, int64_t interval, int64_t offset,
                                      const double *Pr);
int ocn_model_set_boundary_condition(ocn_model_t model, const char *name, int side, int kind, double value);
/* the same with an array-valued condition (see ocn_bc_t; borrowed device pointer, valid for the model's lifetime) */
int ocn_model_set_boundary_condition_array(ocn_model_t model, const char *name, int side, int kind, const double *device_array);
/* name.side = OpenBoundaryCondition(value; scheme = PerturbationAdvection(inflow_timescale, outflow_timescale))
 * (BoundaryConditions/perturbation_advection.jl:57-63) for a side whose condition is OCN_BC_OPEN already (number or array; set it first);
 * enabled = 0: scheme = nothing, the imposed form. The velocity fill of compute_pressure_correction! and of set! then leaves such a side
 * alone and ONE launch steps every scheme side with the clock's last_stage_Δt (ocn_step_open_boundary); update_state! never touches the
 * boundary value, which is the scheme's state. enforce_open_boundary_mass_conservation! (pressure_correction.jl:14) follows the fill
 * in every pressure step, two launches (ocn_enforce_open_boundary_mass_conservation); a time-step stays free of synchronisation. A model
 * with a scheme side does not replay a captured time-step (option use_graph): the step's arguments follow the clock. Replacing the
 * side's condition by another Open one keeps the scheme, by any other kind drops it. OCN_EINVAL: a side that is not the wall-normal one
 * of a Bounded direction (u west / east, v south / north, w bottom / top), a side whose condition is not Open, a negative or NaN
 * timescale; OCN_ENOTSUP: a partitioned model. ocn_model_get_option answers "open_boundary_scheme_sides" (their number) and
 * "open_boundary_launches" (the launches they add to a pressure step: 3, or 0 without a scheme side; where an RK3 substep rides in the
 * tendency launch and the model's two sets of arrays swap, one more small launch carries the boundary values over). */
int ocn_model_set_open_boundary_scheme(ocn_model_t model, const char *name, int side, int enabled, double inflow_timescale,
                                       double outflow_timescale);
/* name.side = FluxBoundaryCondition((ξ, η, t, φ, p) -> a + b φ, field_dependencies = dep); dep at the location of `name` */
int ocn_model_set_linear_flux_bc(ocn_model_t model, const char *name, int side, double a, double b, const char *dep);
/* FluxBoundaryCondition(func, field_dependencies = ..., parameters = ...) for ANY function built from the operations below
 * (BoundaryConditions/continuous_boundary_function.jl:104-154, Utils/user_function_arguments.jl:22-39): func(X..., t, deps..., [p]). A
 * closure cannot cross a C ABI; a program can. The caller evaluates func once with symbolic arguments and hands over the operations it
 * performed, in the order it performed them, as a list in SSA form: instruction n defines value n, the operands a, b, c name EARLIER
 * values, the last value is the flux. Every instruction is one IEEE double operation (no contraction, no reassociation; sqrt and / are
 * correctly rounded; exp .. pow are the device math library's).
 *   OCN_EXPR_CONST   imm
 *   OCN_EXPR_COORD   a = 0 / 1: the node coordinate along the first / second tangential direction of the side (x before y before z) at the
 *                    condition's location there -- ξ / η / r nodes with Face in the normal direction (x_boundary_node .. z_boundary_node, :104-117)
 *   OCN_EXPR_TIME    clock.time of the moment of evaluation
 *   OCN_EXPR_FIELD   a = dependency slot: the dependency at boundary-normal index 1 (left sides) or N (right sides), interpolated from its
 *                    location to the condition's in the two tangential directions by the operator interpolation_operator(from, to) names
 *                    (interpolation_utils.jl:55-69; see ocn_operand_t), never in the normal direction (its location there is Nothing)
 *   OCN_EXPR_ADD SUB MUL DIV MIN MAX POW   a op b (min / max as Julia's: NaN propagates)
 *   OCN_EXPR_NEG ABS SQRT EXP LOG SIN COS TANH   op a
 *   OCN_EXPR_LT LE GT GE   a op b ? 1.0 : 0.0
 *   OCN_EXPR_SELECT  a != 0 ? b : c  (ifelse)
 * Operand fields an instruction does not use are 0. */
#define OCN_EXPR_CONST 0
#define OCN_EXPR_COORD 1
#define OCN_EXPR_TIME 2
#define OCN_EXPR_FIELD 3
#define OCN_EXPR_ADD 4
#define OCN_EXPR_SUB 5
#define OCN_EXPR_MUL 6
#define OCN_EXPR_DIV 7
#define OCN_EXPR_NEG 8
#define OCN_EXPR_ABS 9
#define OCN_EXPR_MIN 10
#define OCN_EXPR_MAX 11
#define OCN_EXPR_SQRT 12
#define OCN_EXPR_EXP 13
#define OCN_EXPR_LOG 14
#define OCN_EXPR_SIN 15
#define OCN_EXPR_COS 16
#define OCN_EXPR_TANH 17
#define OCN_EXPR_POW 18
#define OCN_EXPR_LT 19
#define OCN_EXPR_LE 20
#define OCN_EXPR_GT 21
#define OCN_EXPR_GE 22
#define OCN_EXPR_SELECT 23
#define OCN_EXPR_MAX_INSTRUCTIONS 64
#define OCN_EXPR_MAX_DEPENDENCIES 8
typedef struct { int op, a, b, c; double imm; } ocn_expr_ins_t;
/* The program at every point of `side` (0 west .. 5 top) for a condition of a field at `loc` (the entry along the normal direction is
 * ignored): out[a, b] over the interior extents of the two tangential directions, the dense column-major layout ocn_bc_t::array documents.
 * deps[s]: BORROWED haloed device arrays with current halos, at dep_locs[s]. ONE launch on ocn_stream(), one thread per boundary point.
 * OCN_EINVAL, before any launch: n outside 1..OCN_EXPR_MAX_INSTRUCTIONS, an operand index that is not smaller than the instruction's own,
 * an unknown op, a coordinate other than 0 / 1, a dependency slot >= ndeps, ndeps outside 0..OCN_EXPR_MAX_DEPENDENCIES, a NULL that is
 * needed, a side that is not a wall of the grid. OCN_ENOTSUP on a connected topology; OCN_ESTATE without ocn_grid_set_node_tables. */
int ocn_evaluate_boundary_function(ocn_grid_t grid, const ocn_expr_ins_t *program, int n, const int loc[3], int side,
                                   const double *const *deps, const int (*dep_locs)[3], int ndeps, double time, double *out);
/* name.side = FluxBoundaryCondition(func, ...) with the program of func; dep_names: the model fields ("u", "v", "w", "c0" ..) of the
 * dependency slots, read at their own locations (assumed_field_location). The model owns the (Na, Nb) array, sets the side's condition to
 * {OCN_BC_FLUX, 0, array} and keeps the program in a device-resident table. ONE launch evaluates all functions of the model into their
 * arrays (blockIdx.z selects the function) at the two moments the Flux conditions are consumed -- before the epilogue launch a substep
 * rides in, and at the top of compute_flux_bc_tendencies in the steppers -- with the fields, their halos and clock.time of that moment:
 * the stage times of runge_kutta_3.jl. A model without functions launches nothing more than before. A model whose programs read
 * OCN_EXPR_TIME steps without the captured graph (the time is a kernel argument); others keep it and the launch is captured with the rest.
 * A later ocn_model_set_boundary_condition[_array] or ocn_model_set_linear_flux_bc on that side removes the function and frees the array.
 * At most 16 functions per model. OCN_ENOTSUP on a partitioned model; OCN_EINVAL for unknown names, a side where a Flux condition cannot
 * sit, a seventeenth function and the program errors of ocn_evaluate_boundary_function; OCN_ESTATE without ocn_grid_set_node_tables.
 * ocn_model_get_option answers "boundary_functions" (their number), "boundary_function_launches" (launches per evaluation moment: 1 or 0)
 * and "boundary_functions_read_time" (whether some program holds OCN_EXPR_TIME). */
int ocn_model_set_flux_bc_function(ocn_model_t model, const char *name, int side, const ocn_expr_ins_t *program, int n,
                                   const char *const *dep_names, int ndeps);
/* the function's array as last evaluated, copied to host_out (Na * Nb doubles); synchronous. OCN_EINVAL when the side carries no function */
int ocn_model_boundary_function_values(ocn_model_t model, const char *name, int side, double *host_out);
/* forcing = (name = F,) of the model constructor (Forcings/model_forcing.jl; nonhydrostatic_tendency_kernel_functions.jl:81-93, the last
 * term `+ forcing(i, j, k, grid, clock, model_fields)`) for the closure-free forcings of src/Forcings/:
 *   OCN_FORCING_ARRAY       Forcing(array) / forcing = (T = array,): F = array[i, j, k] (forcing.jl:165-177, model_forcing.jl:29)
 *   OCN_FORCING_RELAXATION  Relaxation(; rate, mask, target) (relaxation.jl): F = (rate·mask)(ξ_m) * (target(ξ_t) - φ), φ the field itself
 *                           (the dependency regularize_forcing adds, relaxation.jl:75-78); GaussianMask / PiecewiseLinearMask / LinearTarget
 *                           depend on one coordinate and not on time, so the CALLER evaluates them at the field's location: a binder calls
 *                           the reference's own functions and passes the bits
 * `nterms` terms are summed as MultipleForcings does (multiple_forcings.jl: left to right for N <= 4, `total = 0; total += Fₙ` beyond);
 * G = G_rest + F, Flux-condition terms after it. field 0 .. 2 = u, v, w, 3 + t = tracer t; 1 <= nterms <= OCN_MAX_FORCING_TERMS, 0 clears
 * the field's forcing. OCN_EINVAL: bad field index, kind or direction, a NULL that is needed, too many terms, a table along a Flat
 * direction (relaxation.jl has no 1- or 2-coordinate mask methods: the reference cannot build such a model either). Tables are copied;
 * an array stays BORROWED while it is set. A partitioned model takes its rank-local tables and arrays. Model option "forcing_path"
 * reports which pass adds the term: 0 none; 1 the role tendency kernel (no physics terms, no Flux condition, Periodic z, single GPU: the
 * RK3 substep stays fused); 3 a standalone pass after the tendency launches (every other configuration; the substeps then run as their
 * own launches); 2 (inside the physics epilogue) is reserved and never reported. "fused_forcing" = 0 forces the standalone pass.
 *   OCN_FORCING_FUNCTION    F = program(x, y, z, t, deps...) at the forced field's (i, j, k) (Forcings/continuous_forcing.jl:119-142;
 *                           Relaxation with a function mask or target, relaxation.jl:80-101): a recorded program as above, in which
 *                           OCN_EXPR_COORD a = 0 / 1 / 2 is the x / y / z node of the field's own location, OCN_EXPR_TIME the clock of
 *                           the tendency evaluation (the stage times of runge_kutta_3.jl; tⁿ in AB2) and OCN_EXPR_FIELD a = slot the
 *                           model field dep_names[slot], read at its own location (assumed_field_location) and interpolated to the
 *                           forced field's by the operator interpolation_operator(from, to) names: the lower direction innermost, none
 *                           along a Flat direction. A Relaxation is the program rate * mask(X...) * (target(X..., t) - φ) with φ as
 *                           dependency slot 0; a binder passes every ContinuousForcing this way.
 * The term takes its place in the sum like any other. A field with a function term is completed by forcing_function_kernel (all its terms,
 * in sum order, one launch for all such fields); "forcing_path" then answers 3. Values that depend on no coordinate and no field, or on
 * one coordinate only, are evaluated once per evaluation moment into 1-D tables (one more launch, and only when a program reads
 * OCN_EXPR_TIME: the others' tables are filled when the forcing is set); per cell only the remaining instructions run, on the same
 * operand bits, so the result does not depend on "forcing_function_hoist" (ocn_model_set_option on the model, default 1; 0: the recorded program at every cell).
 * A model whose forcing programs read OCN_EXPR_TIME steps without the captured graph. At most 16 function terms per model.
 * OCN_EINVAL: the program errors of ocn_evaluate_boundary_function (coordinates 0 .. 2 here), a coordinate along a Flat direction, an
 * unknown dependency name, a seventeenth function; OCN_ENOTSUP on a partitioned model; OCN_ESTATE without ocn_grid_set_node_tables.
 * ocn_model_get_option answers "forcing_functions" (their number), "forcing_function_cell_instructions" (the longest per-cell program),
 * "forcing_functions_read_time" and "forcing_function_arithmetic_only" (1: no per-cell program holds EXP .. POW, and the instantiation
 * of the kernel without them runs -- twice the waves per SIMD). */
#define OCN_FORCING_ARRAY 1
#define OCN_FORCING_RELAXATION 2
#define OCN_FORCING_FUNCTION 3
#define OCN_MAX_FORCING_TERMS 8
typedef struct {
    int kind;
    const double *array;        /* ARRAY: DEVICE pointer in the parent layout of a (Center, Center, Center) field of the model's grid
                                   (ocn_grid_parent_size), read at the forced field's own (i, j, k) */
    int mask_dir;               /* -1: mask = onefunction, the factor is `rate_mask` (= rate); 0 / 1 / 2: the table along x / y / z */
    const double *mask_table;   /* HOST, rate * mask(node) at the field's location over the haloed index range of mask_dir (parent size
                                   along it: element ξ - 1 + H holds node ξ) */
    double rate_mask;
    int target_dir;             /* -1: constant target `target` (zerofunction: 0.0); 0 / 1 / 2: the table along x / y / z */
    const double *target_table; /* HOST, target(node), same layout */
    double target;
    /* OCN_FORCING_FUNCTION (all zero for the other kinds): the recorded program, F = program(x, y, z, t, deps...), and the model fields
       ("u", "v", "w", "c0" ..) of its dependency slots; both are copied */
    const ocn_expr_ins_t *program;
    int n;
    const char *const *dep_names;
    int ndeps;
} ocn_forcing_t;
int ocn_model_set_forcing(ocn_model_t model, int field, const ocn_forcing_t *terms, int nterms);
/* A forcing program at every interior point of a field at `loc`, into the interior of `out`, a parent-shaped DEVICE array at `loc`
 * (ocn_grid_parent_size; halos untouched): what an OCN_FORCING_FUNCTION term adds, without a model. deps[s]: BORROWED haloed device arrays
 * with current halos, at dep_locs[s]. hoist: 1 tables + per-cell program (two launches), 0 the recorded program per cell (one); the bits
 * are the same. Synchronous. With Forcing(array), which is borrowed, a caller can refresh an arbitrary forcing between time-steps.
 * Errors as OCN_FORCING_FUNCTION above. */
int ocn_evaluate_forcing_function(ocn_grid_t grid, const ocn_expr_ins_t *program, int n, const int loc[3], const double *const *deps,
                                  const int (*dep_locs)[3], int ndeps, double time, int hoist, double *out);
/* Host arithmetic only (callable before ocn_init): how a forcing program is split. value_class[q] (n ints, may be NULL) is the class of
 * value q: 0 uniform (depends on no coordinate and no field), 1 / 2 / 3 a line value of x / y / z (that coordinate only), 4 a cell value
 * (two coordinates, or a field). *n_cell: the length of the per-cell program -- the cell instructions plus one table load per distinct
 * uniform or line value they consume (one load when the result itself is no cell value). OCN_EINVAL: the program errors above. */
int ocn_forcing_function_plan(const ocn_expr_ins_t *program, int n, int ndeps, int *value_class, int *n_cell);
/* background_fields = (name = B,) of the model constructor (Models/NonhydrostaticModels/background_fields.jl:97-116, BackgroundFields{false}):
 * name is "u", "v", "w" or "c<n>"; parent is a haloed device array at that field's location, BORROWED for the model's lifetime, whose
 * halos hold what the background is there (a function's analytic continuation, not a periodic wrap); NULL removes it (ZeroField).
 * Every tendency evaluation then computes G_φ = -div(U + Ū, φ) - div(U, Φ̄) + ... -- the second term only for fields that have a
 * background -- and ocn_model_cell_advection_timescale uses U + Ū; closures, buoyancy, Coriolis, the hydrostatic pressure anomaly,
 * boundary conditions and the pressure solve see the model's own fields only. update_state! writes U + Ū of the components that have a
 * background over the whole parent array after the halo fill. ocn_model_field answers "bg_<name>" (the caller's array) and
 * "total_u|v|w" (OCN_ESTATE when that field has no background); ocn_model_get_option answers "background_fields" (how many fields have
 * one) and "background_tendency_path" (0 none, 1 per-field kernels, 2 the split role kernel). With a background the RK3 substep and the
 * forcing do not ride in an advection launch: the substep rides in the epilogue pass when the model has one (physics terms or Flux
 * conditions), otherwise "fuse_substep_active" answers 0. The "bg_<name>" pointer is the caller's own array, handed back READ-ONLY: the
 * library never writes it and neither may a holder of that pointer while the model lives. With option "arithmetic" = 1 the background
 * terms are evaluated in the reference's arithmetic (the per-field kernels) while a term 1 without background velocities keeps the
 * contracted one: the two advection terms of one tendency then differ in arithmetic mode. OCN_ENOTSUP on a partitioned model. */
int ocn_model_set_background_field(ocn_model_t model, const char *name, const double *parent);
/* Tuning options (no reference equivalent; the defaults are the tuned values). ocn_set_option sets the library default of a key; may be
 * called before ocn_init. A model copies the defaults when it is created, and ocn_model_set_option changes that model's copy only.
 * Grid-level entry points and standalone solvers (ocn_compute_*, ocn_fill_halo_regions*, ocn_poisson_*, ocn_solve_for_pressure,
 * ocn_dist_poisson_*) read the defaults when they are called.
 * Scopes: step -- read while stepping; creation -- read only when a model or solver is built, so set it with ocn_set_option before
 * creating the model; partitioned -- read by the partitioned step only. Values are 0 / 1 unless a range is given; every key refuses
 * a value outside its range.
 *   tendency evaluation:
 *   "tendency_impl" = 2 (step): 0 the per-field kernels as the reference launches them, 1 the all-fields flux-sharing kernel, 2 the
 *       one-field-per-workgroup flux-sharing kernel; 0 .. 2 (the grid-level tendency entry points take 1 for 0)
 *   "arithmetic" = 0 (step): 0 the reference's IEEE operation sequence in every kernel -- results bit-identical to a faithful CPU
 *       evaluation of weno_interpolants.jl; 1 the opt-in CONTRACTED WENO-5 flux of the one-field-per-workgroup kernel (fma-contracted
 *       sub-stencil polynomials and alpha weights, one normalisation of the weighted sum, reciprocal without the IEEE divide's fix-up,
 *       advecting transport multiplied by the area after its interpolation): fewer FP64 instructions, fields within 1e-12 of mode 0
 *       on O(1) data but not bit-identical; the other tendency kernels ignore it
 *   "role_kchunk" = 0 (step): levels per workgroup of the one-field-per-workgroup kernel, >= 0 (0 = automatic)
 *   "role_ldspad" = 0 (step): extra dynamic LDS per workgroup of that kernel in bytes (experiments), 0 .. 148256 (what the 160 KiB of a
 *       CU leave beside the kernel's own arrays)
 *   "fused_ty" = 7 (step): tile rows of the all-fields kernel, 3 | 7
 *   "fused_kchunk" = 0 (step): levels per workgroup of the all-fields kernel, >= 0 (0 = automatic)
 *   "fused_zwin" = 1 (step): register z-windows in the all-fields kernel
 *   "fused_xcd" = 0 (step): XCD-aware tile order of the all-fields kernel (measured: no effect)
 *   "swap_tendencies" = 1 (step): cache_previous_tendencies! by pointer swap (0: by copy kernel)
 *   "fuse_substep" = 1 (step): the substeps of RK3 stages 2 and 3 fused into the preceding tendency evaluation (second set of
 *       prognostic arrays, swapped twice per time-step); triply periodic grids: the substep of stage 1 fused into the pressure step
 *   "fused_epilogue" = 1 (step): Coriolis, hydrostatic gradient, closure terms (and the substep) as one launch
 *   "fused_forcing" = 1 (step): the forcing term in the tendency kernel when it can ride there (0: always the standalone pass)
 *   "use_graph" = 0 (step): hipGraph replay of the RK3 step (measured: no gain)
 *   physics passes and halo fills:
 *   "epilogue_march" = 1 (step): z-marching tendency epilogue that evaluates every face flux once (0: one thread per value,
 *       everything recomputed -- same bits)
 *   "epilogue_rows" = 4 (step): rows per workgroup of the marching epilogue, 1 .. 8
 *   "epilogue_kchunk" = 0 (step): levels per workgroup of the marching epilogue, >= 0 (0 = automatic)
 *   "amd_march" = 1 (step): z-marching eddy-diffusivity kernel that evaluates every point operand once (0: one thread per cell,
 *       everything recomputed -- same bits)
 *   "smag_march" = 1 (step): z-marching Smagorinsky eddy-viscosity kernel that evaluates every strain point value once (0: one
 *       thread per cell, everything recomputed -- same bits)
 *   "fused_halo" = 1 (step): one launch fills the halos of every Periodic direction of a group of fields (after the wall fills; on
 *       (Periodic, Periodic, Bounded) grids the bounded z fill rides in it too); inside a time-step on a triply periodic grid no launch
 *       at all -- the pressure-correction kernel writes the halos. 0: one launch per Periodic direction, z, y, x, each over the whole
 *       extent of the other two and reading what the previous one wrote -- same bits
 *   pressure solve:
 *   "real_fft" = 1 (step): D2Z / Z2D transforms (0: the reference's complex-to-complex)
 *   "c2r_strided" = 1 (creation): Z2D straight into the interior of the haloed pressure field
 *   "fused_zfft" = 1 (creation): z FFT + divide + inverse z FFT as one LDS pass
 *   "split_solve" = 1 (step): model time-step: 1-D x plans on 128-B-padded rows + LDS column-FFT kernel for y + pressure correction
 *       and p/Δt from the dense solution (the solver prepares it when the option is on at creation)
 *   "line_zl512" = 4 (step): lines per workgroup of the LDS line transforms at 512-point lines, 4 | 8
 *   "skip_stage_pressure" = 1 (step): RK3 stages 1 and 2 do not store their pNHS -- nothing can read it before the next stage
 *       overwrites it; after a time-step the field holds the last stage's pressure either way
 *   "skip_dead_tendency_store" = 1 (step): the tendency evaluated after RK3's second stage feeds the third stage's substep riding
 *       along and is not stored -- nothing else reads it; after a time-step Gⁿ = G(U³) and G⁻ = G(U¹) either way
 *   x-slab and pencil solves:
 *   "dist_substructured" = 1 (creation): gathered interface solve (0: the reference's two transposes)
 *   "dist_zfirst" = 1 (creation): z-fastest local layout
 *   "dist_xfast" = 1 (creation): the substructured solve in the fields' own x-fastest layout
 *   "dist_yline" = 1 (creation): LDS column-FFT kernel for the local y transform
 *   "dist_fuse_source" = 1 (step): source term written straight into the z transform's line buffer
 *   "dist_xline_group" = 1 (step): several short x lines per wave in the Thomas scans
 *   "dist_pencil_transposes" = 1 (creation): pencil partitions take the reference's transposing solver (0: gathered solve)
 *   partitioned step:
 *   "async_halos" = -1 (partitioned): interior / buffer split of update_state! (-1 automatic, 0 off, 1 on)
 *   "thin_halos" = 1 (partitioned): the pressure step exchanges the one column that is read instead of Hx columns
 *   "early_exchange" = 1 (partitioned): update_state!'s exchange starts from make_pressure_correction!
 *   "strip_width" = 0 (partitioned): columns of the buffer strips, >= 0 (0 = automatic; the step needs Hx <= width < Nx / 2)
 *   "fused_step" (alias "dist_fused_step") = 1 (partitioned): the pressure step without fills / copies between its stages on
 *       (connected, Periodic, Periodic) slabs; its buffers are made when a model is created with it, so switching it on later
 *       needs a model created with it (OCN_ENOTSUP otherwise)
 * OCN_EINVAL: NULL or unknown key, value out of range. */
int ocn_set_option(const char *key, int value);
/* sum of the event-timed tendency evaluations since the last read (ms) and their count; synchronous. This is the
 * measurement hook the reference lacks (it is profiled externally with nsys, .buildkite/pipeline-benchmarks.yml:57) */
int ocn_model_profile_read(ocn_model_t model, double *tendency_ms, int *count);

/* test hook: counts the Float32 significands (of 2^23, binade 2^exponent) for which the fast correctly-rounded
 * reciprocal used inside newton_div (Utils/newton_div.jl:8-20) differs from the IEEE divide; exponent -126 .. 127, every binade of
 * normal numbers. 0 up to exponent 125; binades 126 and 127 (subnormal reciprocal) lie outside the reciprocal's domain and differ */
int ocn_debug_rcp_check(int variant, int exponent, unsigned long long *mismatches);
/* sampled check of the Float64 reciprocal used for the WENO weight normalisation against the compiler's IEEE divide:
 * nsamples pseudo-random significands with exponents exp_lo..exp_hi (-1022 .. 1023); returns the number of differing results */
int ocn_debug_rcp64_check(unsigned long long nsamples, int exp_lo, int exp_hi, unsigned long long seed,
                          unsigned long long *mismatches);
/* where the cosine-transform path's permute_indices! (backward = 0) / unpermute_indices! (backward = 1) send element i of a line of
 * length N: destination[i - 1], 1-based -- the tables of Solvers/index_permutations.jl:5-35 (host array, synchronous) */
int ocn_debug_permute_indices(int N, int backward, int *destination);
/* number of Poisson solvers of this process that switched to the per-direction transform path because their multi-dimensional rocFFT
 * plans failed the creation-time self-check (rocFFT returns wrong transforms from such plans while plans of other sizes are alive;
 * the unit-stride 1-D plans of the per-direction path are not affected) */
int ocn_debug_fft_fallbacks(void);

/* ---------------------------------------------------------------- distributed: communicator + partitioned model -- */
/* `Distributed(GPU(); partition = Partition(R))` (DistributedComputations/distributed_architectures.jl:166-302): one process per
 * GPU, x-slabs, ring neighbours with periodic wrap (:391-434). The library owns the communicator: RCCL over xGMI
 * (ncclCommInitRank; librccl is opened at run time by the first of these calls, single-GPU users never load it). Bootstrap as
 * with NCCL: rank 0 calls ocn_dist_unique_id, the caller carries the 128 bytes to every rank (MPI_Bcast, a TCP store, a file),
 * every rank calls ocn_dist_create after ocn_init(local device). Halo transfers run on the library's communication stream
 * between two events: kernels launched afterwards overlap them; the host never synchronises (the reference calls sync_device!
 * before every MPI call, halo_communication.jl:181, distributed_transpose.jl:187). */
int ocn_dist_unique_id(void *id128);
int ocn_dist_create(ocn_dist_t *dist, const void *id128, int world, int rank);
/* The same architecture object over collectives the CALLER supplies -- the seam for MPI.jl in a Julia binder (the reference's
 * own transport), and what the tests use to run R ranks on one card. All buffers are device pointers; `stream` is the library's
 * compute stream (a hipStream_t): the callbacks must order their transfers behind the work already on it and make later work on
 * it wait for them (or synchronise). exchange_start/_wait: `count` doubles per side, what leaves through the west side arrives in the
 * west neighbour's east halo (MPI.Isend/Irecv! + Waitall, halo_communication.jl:300,326,164); all_to_all: piece r of `send`
 * (`count_per_rank` doubles) goes to rank r (MPI.Alltoallv!, distributed_transpose.jl:185-191); all_gather: rank r's `count` doubles
 * land at recv[r * count]; allreduce_max: host scalar in / out. Return 0 on success. */
typedef struct {
    int (*exchange_start)(void *user, const double *west_send, const double *east_send, double *west_recv, double *east_recv,
                          size_t count, void *stream);
    int (*exchange_wait)(void *user, void *stream);
    int (*all_to_all)(void *user, const double *send, double *recv, size_t count_per_rank, void *stream);
    int (*all_gather)(void *user, const double *send, double *recv, size_t count, void *stream);
    int (*allreduce_max)(void *user, double *value);
    void *user;
    /* pencil partitions only (may be NULL otherwise): one exchange with an explicit pair of peer ranks, complete in stream order when it
     * returns -- `lo_send` goes to peer_lo and lands in ITS hi_recv, `hi_send` goes to peer_hi and lands in its lo_recv */
    int (*exchange_peers)(void *user, int peer_lo, int peer_hi, const double *lo_send, const double *hi_send, double *lo_recv,
                          double *hi_recv, size_t count, void *stream);
    /* pencil transposes only (may be NULL otherwise): MPI.Alltoallv! with equal counts on a sub-communicator given as the list of its
     * members' world ranks (this rank included, in group order): chunk q of `send` (count doubles) goes to peers[q], chunk q of `recv`
     * comes from peers[q]; complete in stream order when it returns */
    int (*all_to_all_group)(void *user, const int *peers, int npeers, const double *send, double *recv, size_t count, void *stream);
} ocn_transport_t;
int ocn_dist_create_transport(ocn_dist_t *dist, const ocn_transport_t *transport, int world, int rank);
int ocn_dist_destroy(ocn_dist_t dist);
int ocn_dist_info(ocn_dist_t dist, int *world, int *rank, int *west, int *east);
/* what the TRANSPORT reports: kind 0 = the library's RCCL communicator (comm_ranks / comm_rank / device from ncclCommCount /
 * ncclCommUserRank / ncclCommCuDevice -- the ranks RCCL really connected, MPI.Comm_size / Comm_rank of the reference's communicator,
 * distributed_architectures.jl:262-263), 1 = caller-supplied collectives (the numbers given at creation) */
int ocn_dist_comm_info(ocn_dist_t dist, int *kind, int *comm_ranks, int *comm_rank, int *device);
/* MEASUREMENT / TEST ONLY: a communicator of ONE rank treats x as partitioned with itself as both neighbours, so the complete
 * N > 1 code path runs (and can be timed) on a one-GPU box; results equal the one-rank Periodic run. Set before model creation. */
int ocn_dist_set_self_loop(ocn_dist_t dist, int enabled);
/* the collectives themselves, for callers that orchestrate the stages on their own (send / recv of halo buffers,
 * halo_communication.jl:170-187; transposes, distributed_transpose.jl:185-191) */
int ocn_dist_exchange_start(ocn_dist_t dist, const double *west_send, const double *east_send, double *west_recv, double *east_recv,
                            size_t count);
int ocn_dist_exchange_wait(ocn_dist_t dist);
int ocn_dist_all_to_all(ocn_dist_t dist, const double *send, double *recv, size_t count_per_rank);
int ocn_dist_all_gather(ocn_dist_t dist, const double *send, double *recv, size_t count);
int ocn_dist_allreduce_max(ocn_dist_t dist, double *value);      /* synchronous */
int ocn_dist_barrier(ocn_dist_t dist);                           /* synchronous */
/* NonhydrostaticModel on a Distributed architecture: `local_grid` is this rank's slab (x topology OCN_CONNECTED when x is
 * partitioned: distributed_grids.jl:339-346), `Lx_global` the extent of the global domain along x. The returned handle is an
 * ocn_model_t: every ocn_model_* call works on it (set_option also takes the partitioned options, ocn_set_option);
 * ocn_model_time_step runs the partitioned RK3 step -- fill_halo_regions! with the x exchange
 * (halo_communication.jl:87-110), the interior / buffer split (Models/interleave_communication_and_computation.jl:9-67) or the
 * exchange started from make_pressure_correction!, and solve! of the distributed solvers
 * (distributed_fft_based_poisson_solver.jl:141-178, distributed_fft_tridiagonal_solver.jl:153-257) -- entirely inside the library. */
int ocn_dist_model_create(ocn_model_t *model, ocn_grid_t local_grid, int ntracers, ocn_dist_t dist, double Lx_global);
/* the same for an irregular partition (local_size, distributed_grids.jl:44-58: N / R columns per rank, the remainder on the last one;
 * or any `Sizes`): local_sizes[r] = Nx of rank r. Equal sizes take the distributed solvers; otherwise solve! gathers the source term
 * on every rank and runs the single-GPU solver on the global grid -- every slab layout works, memory and traffic grow with the
 * GLOBAL grid (a fallback, not the scaling path). */
int ocn_dist_model_create_sizes(ocn_model_t *model, ocn_grid_t local_grid, int ntracers, ocn_dist_t dist, double Lx_global,
                                const int *local_sizes);
/* ... and for a Bounded partitioned direction (global_x_topology = OCN_BOUNDED; OCN_PERIODIC: as above): insert_connected_topology
 * (distributed_grids.jl:339-346) -- the first rank's local grid is OCN_RIGHT_CONNECTED (wall on its west side), the last one's
 * OCN_LEFT_CONNECTED, the others OCN_CONNECTED. Boundary conditions and the advection scheme's wall fallbacks
 * (topologically_conditional_interpolation.jl:54-70) act on the wall side only; local_sizes may be NULL (equal slabs). The pressure
 * solve takes the gathered form on the global Bounded grid (cosine transform along x). */
int ocn_dist_model_create_partition(ocn_model_t *model, ocn_grid_t local_grid, int ntracers, ocn_dist_t dist, double Lx_global,
                                    const int *local_sizes, int global_x_topology);
/* Partition(Rx, Ry) pencils (distributed_architectures.jl:354-434: rank = ix * Ry + iy, periodic wrap of the four neighbours):
 * ocn_dist_set_layout fixes the layout of a communicator (ocn_dist_model_create_pencil calls it); the local grid is connected in x when
 * Rx > 1 (codes as above) and in y when Ry > 1: OCN_CONNECTED where the global y direction is Periodic, OCN_RIGHT_CONNECTED (first row
 * of ranks) / OCN_CONNECTED / OCN_LEFT_CONNECTED (last row) where global_y_topology = OCN_BOUNDED. sizes_x[Rx] / sizes_y[Ry]: slab
 * widths (NULL: equal).
 * Every fill makes two hops -- x, then y over the whole x extent -- so corners arrive without corner messages
 * (fill_corners!, halo_communication.jl:137-162); solve! is the gathered solve on the global grid (the reference's pencil transposes,
 * distributed_transpose.jl:12-15, are not built). */
int ocn_dist_set_layout(ocn_dist_t dist, int Rx, int Ry);
int ocn_dist_model_create_pencil(ocn_model_t *model, ocn_grid_t local_grid, int ntracers, ocn_dist_t dist, double Lx_global,
                                 double Ly_global, int Rx, int Ry, const int *sizes_x, const int *sizes_y, int global_x_topology,
                                 int global_y_topology);
/* ---- TransposableField and its transposes (pencil partitions; row f.4 of SURVEY.md 8) ----------------------------------------------
 * TransposableField(field_in, ComplexF64) (transposable_field.jl:49-105) for a field of GLOBAL size (Nx, Ny, Nz) on the communicator's
 * Partition(Rx, Ry) (ocn_dist_set_layout): complex (re, im interleaved) fields without halos, x fastest --
 * zfield (Nx/Rx, Ny/Ry, Nz), yfield (Nx/Rx, Ny, Nz/Ry), xfield (Nx, Ny/Rx, Nz/Ry); yfield is zfield when Ry = 1, xfield is yfield when
 * Rx = 1. Equal chunks as in the reference: Rx | Nx, Ry | Ny, Ry | Nz, Rx | Ny (distributed_fft_based_poisson_solver.jl:213-226). */
int ocn_transposable_create(ocn_transposable_t *field, ocn_dist_t dist, int Nx, int Ny, int Nz);
int ocn_transposable_destroy(ocn_transposable_t field);
/* device pointers and sizes of the three configurations (any output may be NULL) */
int ocn_transposable_fields(ocn_transposable_t field, double **zfield, double **yfield, double **xfield, int zsize[3], int ysize[3], int xsize[3]);
/* transpose_z_to_y! / transpose_y_to_x! / transpose_x_to_y! / transpose_y_to_z! (distributed_transpose.jl:25-95,185-191): pack kernel,
 * all-to-all inside the group of ranks that share ix (z <-> y) or iy (y <-> x), unpack kernel; bit-exact copies; no-ops on slabs (:12-15) */
int ocn_transpose_z_to_y(ocn_transposable_t field);
int ocn_transpose_y_to_x(ocn_transposable_t field);
int ocn_transpose_x_to_y(ocn_transposable_t field);
int ocn_transpose_y_to_z(ocn_transposable_t field);
int ocn_dist_model_max_abs_divergence(ocn_model_t model, double *value);    /* global maximum; synchronous */

/* ---------------------------------------------------------------- diagnostics (AbstractOperations/, Fields/scans.jl) ----------------
 * One operation node: op(▶a(a), ▶b(b)) at `loc` (BinaryOperation, AbstractOperations/binary_operations.jl:5-25,38-43). a / b: BORROWED device
 * parent arrays with filled halos at loc_a / loc_b, or NULL for the number ca / cb. `loc` is the location of the first field operand
 * (binary_operations.jl:109-135); the other field is interpolated to it by the operator interpolation_operator(from, to) names
 * (Operators/interpolation_utils.jl:55-69): 0.5 (f[i] + f[i+1]) to a Center, 0.5 (f[i-1] + f[i]) to a Face, nested z of y of x for two
 * directions and x of y of z for three (Operators/interpolation_operators.jl:8-15,45-71), the identity in a Flat direction (:87-110).
 * OCN_OP_IDENTITY: the field a itself. Partitioned grids (connected topologies) answer OCN_ENOTSUP. */
#define OCN_OP_IDENTITY 0
#define OCN_OP_ADD 1
#define OCN_OP_SUB 2
#define OCN_OP_MUL 3
#define OCN_OP_DIV 4
typedef struct {
    int op;
    const double *a, *b;
    double ca, cb;
    int loc_a[3], loc_b[3];
    int loc[3];
} ocn_operand_t;
/* compute_computed_field! / _compute! (AbstractOperations/computed_field.jl:92-103): out[i, j, k] = operand[i, j, k] over the interior of
 * `out`, a parent array at operand->loc; the halos of `out` are the caller's (fill_halo_regions!, :87, is the next call) */
int ocn_compute_operation(ocn_grid_t grid, const ocn_operand_t *operand, double *out);
/* sum! / maximum! / minimum! of the operand into a reduced field (Fields/field.jl:735-767) and average! (AbstractOperations/
 * metric_field_reductions.jl:34-47) over the operand's interior -- all N + 1 points of a Face field on a Bounded direction.
 * dims_mask: bit d set = direction d + 1 is reduced (1..7). use_metric: the summand is operand * metric with the metric
 * reduction_grid_metric(dims) names (metric_field_reductions.jl:12-21: Δx, Δy, Δz, Az = Δx Δy, Ay = Δx Δz, Ax = Δy Δz, V = Az Δz,
 * Operators/spacings_and_areas_and_volumes.jl:309-311,326-333) at the operand's location -- Integral (:144-150); OCN_REDUCE_AVERAGE then
 * divides by the sum of the metric over the same points (:75-92), and without use_metric by the number of points (conditional_length,
 * Fields/field.jl:722-732). absolute: f = abs (maximum(abs, c)). `out`: the parent array of the reduced field (reduced_location,
 * field.jl:673-687: size 1 and no halo in the reduced directions, the halos of the kept ones untouched).
 * No atomics: block partial sums in a slab of the grid, combined in a fixed order that depends on the grid size and dims_mask only. */
#define OCN_REDUCE_SUM 0
#define OCN_REDUCE_MAXIMUM 1
#define OCN_REDUCE_MINIMUM 2
#define OCN_REDUCE_AVERAGE 3
int ocn_reduce_operation(ocn_grid_t grid, const ocn_operand_t *operand, int kind, int dims_mask, int use_metric, int absolute, double *out);
/* cumsum! / reverse_cumsum! (directional_accumulate!, accumulate_x / _y / _z, Fields/scans.jl:225-306) along direction dim (0, 1, 2):
 * B[start] = A[start], B[i] = B[i ∓ 1] + A[i] in that sequential order; use_metric: A = operand * Δ of the direction (CumulativeIntegral,
 * metric_field_reductions.jl:206-212). `out`: a parent array at operand->loc, interior written. */
int ocn_accumulate_operation(ocn_grid_t grid, const ocn_operand_t *operand, int dim, int reverse, int use_metric, double *out);

/* ---------------------------------------------------------------- stencil programs ---------------------------------------------------
 * KernelFunctionOperation{LX, LY, LZ}(kernel_function, grid, arguments...) (AbstractOperations/kernel_function_operation.jl:58-70), and
 * what Derivative (derivatives.jl), UnaryOperation (unary_operations.jl) and @at (at.jl) lower to. A closure cannot cross this ABI: the
 * host calls kernel_function(i, j, k, grid, args...) ONCE with symbols and records a straight-line program in SSA form -- instruction n
 * defines value n, operands name earlier values, the LAST value is the operand at (i, j, k). The arithmetic ops are the OCN_EXPR_* codes
 * with their meanings (Julia's min / max, correctly rounded sqrt and /, one IEEE operation each, no contraction); the leaves are
 *   OCN_EXPR_CONST       imm
 *   OCN_STENCIL_LOAD     a = argument slot: args[a] at (i + di, j + dj, k + dk)                (getindex of a field)
 *   OCN_STENCIL_SPACING  a = direction 0 / 1 / 2, b = OCN_CENTER / OCN_FACE: Δx, Δy or Δz at that location and at the index shifted by
 *                        the direction's own offset (Operators/spacings_and_areas_and_volumes.jl:44-145); 1 in a Flat direction
 *   OCN_STENCIL_NODE     a = direction, b = location: xnode / ynode / znode at the shifted index (Grids/nodes_and_spacings.jl), from the
 *                        tables of ocn_grid_set_node_tables (OCN_ESTATE without them)
 * OCN_EXPR_COORD, OCN_EXPR_TIME and OCN_EXPR_FIELD are no ops of a stencil program.
 * args: BORROWED device parent arrays with filled halos, arg_locs[3 s + d] their locations; loc: where the operation lives -- its
 * interior (N + 1 points for a Face on a Bounded direction) is what is computed, reduced or accumulated.
 *
 * OCN_EINVAL, before any launch: n outside 1..OCN_STENCIL_MAX_INSTRUCTIONS, nargs outside 0..OCN_STENCIL_MAX_ARGUMENTS, an operand that is
 * no earlier value, an unknown op, a slot >= nargs, an unused field that is not 0, more than OCN_STENCIL_MAX_SLOTS values alive at once,
 * a NULL that is needed, an offset along a Flat direction, and the REACH RULE: with n_out the interior extent of `loc` and n_arg that of
 * the argument along a non-Flat direction d, every LOAD needs off >= -H_d and n_out + off <= n_arg + H_d (a Center argument read from
 * a Face output on a Bounded direction has one point less of room); Δz tables and node tables are checked the same way against their
 * lengths. The message names the argument, the direction and the halo it would need. Connected topologies answer OCN_ENOTSUP.
 *
 * Limits: values live in LDS, one 8-byte word per thread and LIVE value; the kernels have 256 threads, so a slot is 2 KiB and 64 slots
 * are 128 KiB of the 160 KiB of a CU. Slots are reused (ocn_stencil_plan), so the budget is values alive at once, not instructions. */
#define OCN_STENCIL_LOAD 25
#define OCN_STENCIL_SPACING 26
#define OCN_STENCIL_NODE 27
#define OCN_STENCIL_MAX_INSTRUCTIONS 256
#define OCN_STENCIL_MAX_SLOTS 64
#define OCN_STENCIL_MAX_ARGUMENTS 8
typedef struct { int op, a, b, c, di, dj, dk; double imm; } ocn_stencil_ins_t;
typedef struct {
    const ocn_stencil_ins_t *program;
    int n;
    const double *const *args;
    const int *arg_locs;          /* 3 per argument */
    int nargs;
    int loc[3];
} ocn_stencil_operand_t;
/* _compute!(data, operand) (computed_field.jl:100-103) of a stencil operand; see ocn_compute_operation */
int ocn_compute_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, double *out);
/* sum! / maximum! / minimum! / average! (Fields/field.jl:735-767, metric_field_reductions.jl:34-47) of a stencil operand: the splits,
 * the combine order, the metric and `absolute` are those of ocn_reduce_operation -- the same kernels with another evaluator */
int ocn_reduce_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, int kind, int dims_mask, int use_metric, int absolute, double *out);
/* cumsum! / reverse_cumsum! (Fields/scans.jl:225-306) of a stencil operand; see ocn_accumulate_operation */
int ocn_accumulate_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, int dim, int reverse, int use_metric, double *out);
/* the LDS slot of every value: a linear scan over the program -- a value's slot is free again at its last use (the instruction that uses
 * it last may take it for its own result: operands are read before the result is written), a value takes the lowest free slot, the
 * last value stays alive. slot_of_value: n ints; nslots: how many slots the program needs. Host arithmetic only, callable before
 * ocn_init. OCN_EINVAL for the program errors above that need no grid (slot limit included). */
int ocn_stencil_plan(const ocn_stencil_ins_t *program, int n, int nargs, int *slot_of_value, int *nslots);

/* ---------------------------------------------------------------- time averages (OutputWriters/windowed_time_average.jl) -------------
 * accumulate_result! (:216-230): result = (result * T_previous + integrand * dt) / T_current, element by element -- two IEEE multiplies,
 * one add, one correctly rounded divide, in that association, no contraction. The integrand is never stored: each entry point below is
 * its plain counterpart above (same operand rules, same kernels, same splits, chunks and combine orders, so the integrand has the bits
 * the counterpart would have written) with the fold at the store, in the thread that formed the value. `result` is what `out` is for
 * the counterpart and must not be one of the operand's arrays. The three times travel by value: no device-to-host copy, no
 * stream synchronisation.
 * first != 0: the first sample of a window, where advance_time_average! (:236-249) has just zeroed the result and T_previous is 0 --
 * `result` is neither read nor cleared beforehand and becomes (0.0 * 0.0 + integrand * dt) / T_current, the reference's bits: an
 * integrand of -0.0 gives +0.0, and in general the value is not the integrand.
 * ocn_time_average_operation with OCN_OP_IDENTITY (a plain field) folds the WHOLE parent array, halos included, as `@.` on
 * parent(result) does; every other operand is folded over the interior of its location and leaves the halos of `result` alone.
 * OCN_EINVAL before any launch: a NULL result or fold, a non-finite time, T_current <= 0, T_previous < 0, first with T_previous != 0,
 * and every operand error of the counterpart. Connected topologies answer OCN_ENOTSUP. */
typedef struct {
    double T_previous, dt, T_current;
    int first;
} ocn_time_fold_t;
int ocn_time_average_operation(ocn_grid_t grid, const ocn_operand_t *operand, const ocn_time_fold_t *fold, double *result);
/* the fold of n doubles: a materialised integrand of any shape -- a reduced field, which has no location code for an operand -- over its
 * whole parent array; `integrand` and `result` are device arrays of n elements */
int ocn_time_average_parent(const double *integrand, size_t n, const ocn_time_fold_t *fold, double *result);
int ocn_time_average_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, const ocn_time_fold_t *fold, double *result);
int ocn_time_average_reduce_operation(ocn_grid_t grid, const ocn_operand_t *operand, int kind, int dims_mask, int use_metric, int absolute,
                                      const ocn_time_fold_t *fold, double *result);
int ocn_time_average_reduce_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, int kind, int dims_mask, int use_metric, int absolute,
                                    const ocn_time_fold_t *fold, double *result);
int ocn_time_average_accumulate_operation(ocn_grid_t grid, const ocn_operand_t *operand, int dim, int reverse, int use_metric,
                                          const ocn_time_fold_t *fold, double *result);
int ocn_time_average_accumulate_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, int dim, int reverse, int use_metric,
                                        const ocn_time_fold_t *fold, double *result);

#ifdef __cplusplus
}
#endif
#endif
