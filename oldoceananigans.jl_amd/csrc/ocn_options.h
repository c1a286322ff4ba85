// ocn_options.h -- the tuning options of the library (no reference equivalent; the defaults are the tuned values).
// One instance holds the library defaults (g_defaults, written by ocn_set_option); every model takes a copy of it when it is created
// (ocn_model_s::opt, written by ocn_model_set_option). Host code reads the options of the object it works for and passes them down;
// the key table, its validation and the scope of every key are in ocn_api.hip (kOptions).
#pragma once

struct OcnOptions {
    // tendency evaluation
    int tendency_impl = 2;             // 0 per-field kernels (the reference's launch structure), 1 all-fields flux-sharing kernel
                                       // (ocn_tendency_fused.h), 2 one-field-per-workgroup flux-sharing kernel (ocn_tendency_roles.h)
    int arithmetic = 0;                // 0: the reference's operation sequence (bit-identical to the oracle); 1: contracted WENO flux (ocn_device.h)
    int role_kchunk = 0;               // levels per workgroup of the role kernel (0: automatic)
    int role_ldspad = 0;               // experiments: extra dynamic LDS per workgroup (bytes) to limit the workgroups per CU
    // all-fields kernel, tuned on MI355X at 256^3 (tools/tune_fused.py): 64 x 7 tiles, register z-windows, 2 waves/SIMD (no spills);
    // kchunk = 0: levels per workgroup chosen per launch so that the grid fills whole rounds of the chip (see pick_kchunk)
    int fused_ty = 7;
    int fused_kchunk = 0;
    int fused_zwin = 1;
    int fused_xcd = 0;                 // XCD-aware tile order (FusedArgs::xcd_swizzle): measured 1.445 vs 1.440 ms at 256^3 -- no effect, off
    // physics passes
    int epilogue_march = 1;            // closure / Coriolis / pHY′ epilogue as a z-march that shares the symmetric flux tensor (0: one thread per field value)
    int epilogue_rows = 4;             // rows (waves) per block of that kernel
    int epilogue_kchunk = 0;           // levels per block of that kernel (0: automatic)
    int amd_march = 1;                 // eddy diffusivities by the z-marching kernel that shares the point operands (0: one thread per cell, everything recomputed)
    int smag_march = 1;                // Smagorinsky eddy viscosity by its z-marching kernel (0: one thread per cell, every point value recomputed)
    // halo fills
    int fused_halo = 1;                // the periodic fills of all Periodic directions as one launch, with the bounded z fill on (P, P, B) grids
                                       // (0: one launch per direction, z, y, x); inside a time-step on a triply periodic grid they ride in
                                       // the pressure-correction kernel (pressure_step, fold_halos)
    // pressure solve
    int real_fft = 1;                  // D2Z / Z2D transforms (0: the reference's complex-to-complex)
    int c2r_strided = 1;               // Z2D straight into the interior of the haloed pressure field
    int fused_zfft = 1;                // FFT solver, z Periodic, Nz = 2^m <= 1024: z transform + divide + inverse z transform in one pass
    int split_solve = 1;               // model time-step: split (x, y) transforms + pressure correction from the dense solution (see ocn_poisson_s::split)
    int line_zl512 = 4;                // lines per workgroup of the LDS line-FFT kernels at 512-point lines (8: 64 KB of LDS per workgroup)
    int skip_stage_pressure = 1;       // RK3 stages 1, 2: pNHS of the stage is not stored (overwritten by the next stage before anything can read it)
    int skip_dead_tendency_store = 1;  // the tendency evaluated after RK3's second stage is not stored (FusedSubstep::store_G)
    // distributed solvers
    int dist_substructured = 1;        // distributed FFT solver (z Periodic): substructured x solve + one small all-gather instead of two all-to-alls
    int dist_zfirst = 1;               // substructured solve on the z-fastest layout (R2C along z); 0: paired-column layout
    int dist_xfast = 1;                // substructured x solve in the fields' own x-fastest layout (paired z transform in LDS, one-wave-per-line Thomas scans) when sizes allow
    int dist_yline = 1;                // z Bounded: local y transform by strided_line_fft_kernel (Ny = 2^m <= 1024) instead of rocFFT's 1-D strided plan
    int dist_fuse_source = 1;          // x-fastest solve: source term and paired z transform in one kernel (no dense real right-hand side)
    int dist_xline_group = 1;          // x-fastest solve on short local lines (32 / 64 / 128 points): several lines per wave instead of one
    int dist_pencil_transposes = 1;    // pencil partitions of triply Periodic grids: the reference's transposing solver (0: gathered solve)
    // model time-step
    int swap_tendencies = 1;           // cache_previous_tendencies! by pointer swap (0: copy kernel)
    int fuse_substep = 1;              // substeps of RK3 stages 2 and 3 fused into the preceding tendency evaluation (see ocn_model_s::U2);
                                       // triply periodic grids: the substep of stage 1 fused into the pressure step (PendingSubstep)
    int fused_epilogue = 1;            // Coriolis + hydrostatic gradient + closure (+ substep) as one launch
    int fused_forcing = 1;             // the forcing term rides in the role tendency kernel when it can (0: always the standalone pass)
    // One RK3 time-step is ~50 dependent launches. use_graph = 1 captures the step once per (Δt, configuration) into a hipGraph and
    // replays it. OFF by default: measured on MI355X (tools/time_small.py) replay and plain launches take the same time at every size
    // (16^3: 0.436 vs 0.441 ms/step, 256^3: 7.58 vs 7.51) -- small grids are bound by the ~9 us GPU-side latency between DEPENDENT
    // dispatches, which a graph does not remove; only fewer kernels would.
    int use_graph = 0;
    // partitioned model (ocn_dist.h)
    int async_halos = -1;              // -1 automatic (slab wide enough for whole-tile strips), 0 off, 1 on
    int thin_halos = 1;                // pressure step: exchange the ONE column that is read (u[Nx+1], p[0]) instead of Hx columns
    int early_exchange = 1;            // start update_state!'s exchange from make_pressure_correction!
    int strip_width = 0;               // 0 automatic
    int fused_step = 1;                // (connected, Periodic, Periodic) slabs: the pressure step without fills / copies between its stages
};
