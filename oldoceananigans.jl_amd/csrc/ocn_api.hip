// ocn_api.hip -- C ABI (include/ocn_mi355x.h) of the MI355X-native NonhydrostaticModel hot path.
// Host orchestration mirrors the reference functions cited next to each entry point; all device work is enqueued on
// one non-blocking HIP stream.
#include "../../include/ocn_mi355x.h"
#include "ocn_kernels.h"
#include "ocn_options.h"
#include "ocn_tendency_fused.h"
#include "ocn_tendency_roles.h"
#include "ocn_advect_split.h"
#include "ocn_epilogue_march.h"
#include "ocn_forcing.h"
#include "ocn_implicit_z.h"
#include "ocn_particles.h"
#include "ocn_open_boundary.h"
#include "ocn_diagnostics.h"
#include "ocn_boundary_function.h"
#include "ocn_forcing_function.h"
#include "ocn_dynamic_smagorinsky.h"
#include <hipfft/hipfft.h>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

// ---------------------------------------------------------------------------------------------------------------------
// runtime state / error handling
// ---------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static uint64_t g_epoch = 1;             // bumped by every stream change (invalidates captured time-step graphs)
static hipStream_t g_stream = nullptr;   // may legitimately be the null (legacy default) stream after ocn_set_stream
static int g_device = -1;
static bool g_initialized = false;
static bool g_stream_owned = true;
// the library defaults of the tuning options (ocn_set_option): grid-level entry points and standalone solvers read them at call time,
// a model copies them when it is created
static OcnOptions g_defaults;

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail((int)e_, "%s: %s", #expr, hipGetErrorString(e_));     \
    } while (0)
#define FFT_TRY(expr)                                                                            \
    do {                                                                                         \
        hipfftResult r_ = (expr);                                                                \
        if (r_ != HIPFFT_SUCCESS) return fail(1000 + (int)r_, "%s: hipfftResult %d", #expr, (int)r_); \
    } while (0)
#define NEED_INIT()                                                                              \
    do {                                                                                         \
        if (!g_initialized) return fail(OCN_ESTATE, "ocn_init() has not been called");           \
    } while (0)
#define KERNEL_CHECK()                                                                           \
    do {                                                                                         \
        hipError_t e_ = hipGetLastError();                                                       \
        if (e_ != hipSuccess) return fail((int)e_, "kernel launch: %s", hipGetErrorString(e_)); \
    } while (0)

// every device allocation of the library goes through here; OCN_POISON=1 fills fresh memory with NaN bytes so that a
// read of uninitialised device memory shows up as NaN in the parity tests instead of depending on allocator history
static hipError_t dev_alloc(void **p, size_t bytes) {
    static const bool poison = getenv("OCN_POISON") != nullptr;
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess && poison) e = hipMemset(*p, 0xFF, bytes);
    return e;
}

extern "C" const char *ocn_last_error(void) { return g_err; }
extern "C" const char *ocn_version(void) { return "ocn_mi355x 0.1 (gfx950; reference Oceananigans v0.100.5)"; }

extern "C" int ocn_device_count(int *count) {
    if (!count) return fail(OCN_EINVAL, "NULL argument");
    HIP_TRY(hipGetDeviceCount(count));
    return OCN_OK;
}

extern "C" int ocn_init(int device_id) {
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (count <= 0) return fail(OCN_ESTATE, "no HIP device visible");
    if (device_id < 0 || device_id >= count) return fail(OCN_EINVAL, "device_id %d out of range [0, %d)", device_id, count);
    HIP_TRY(hipSetDevice(device_id));
    if (g_initialized && g_device == device_id) return OCN_OK;
    if (g_initialized && g_stream_owned && g_stream) { hipStreamDestroy(g_stream); g_stream = nullptr; }
    HIP_TRY(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    g_stream_owned = true;
    g_device = device_id;
    g_initialized = true;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) g_num_cus = cus;
    return OCN_OK;
}

// run all subsequent work on a stream owned by the caller (e.g. torch.cuda.current_stream() so that RCCL collectives
// issued through torch.distributed are ordered with the kernels without host synchronisation)
extern "C" int ocn_set_stream(void *stream) {
    if (!g_initialized) return fail(OCN_ESTATE, "ocn_init() has not been called");
    if (g_stream && g_stream_owned) { HIP_TRY(hipStreamSynchronize(g_stream)); HIP_TRY(hipStreamDestroy(g_stream)); }
    g_stream = (hipStream_t)stream;
    g_stream_owned = false;
    g_epoch += 1;
    return OCN_OK;
}

// back to a stream created and owned by the library (the state after ocn_init): waits for the borrowed stream first
extern "C" int ocn_own_stream(void) {
    if (!g_initialized) return fail(OCN_ESTATE, "ocn_init() has not been called");
    if (g_stream_owned) return OCN_OK;
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    g_stream_owned = true;
    g_epoch += 1;
    return OCN_OK;
}

extern "C" int ocn_sync(void) { NEED_INIT(); HIP_TRY(hipStreamSynchronize(g_stream)); return OCN_OK; }
extern "C" void *ocn_stream(void) { return (void *)g_stream; }

extern "C" int ocn_malloc(void **ptr, size_t bytes) {
    NEED_INIT();
    if (!ptr) return fail(OCN_EINVAL, "ptr is NULL");
    HIP_TRY(dev_alloc(ptr, bytes ? bytes : 8));
    HIP_TRY(hipMemsetAsync(*ptr, 0, bytes ? bytes : 8, g_stream));
    return OCN_OK;
}
extern "C" int ocn_free(void *ptr) { if (ptr) HIP_TRY(hipFree(ptr)); return OCN_OK; }
extern "C" int ocn_memcpy_h2d(void *dst, const void *src, size_t bytes) {
    NEED_INIT();
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return OCN_OK;
}
extern "C" int ocn_memcpy_d2h(void *dst, const void *src, size_t bytes) {
    NEED_INIT();
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return OCN_OK;
}
extern "C" int ocn_memcpy_d2d(void *dst, const void *src, size_t bytes) {
    NEED_INIT();
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, g_stream));
    return OCN_OK;
}
extern "C" int ocn_memset_zero(void *dst, size_t bytes) {
    NEED_INIT();
    HIP_TRY(hipMemsetAsync(dst, 0, bytes, g_stream));
    return OCN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// grid
// ---------------------------------------------------------------------------------------------------------------------
struct ocn_grid_s {
    DGrid d;
    double L[3];
    bool z_regular;
    double *tables;   // one device allocation holding dzc, dzf, ax, ay, vinv_c, vinv_f, rdzf, rdzc, df2, df
    const double *df2; // Δf² = cbrt((Δx Δy) Δzᶜ)² per level: the Smagorinsky filter width (smagorinsky.jl:99-100), formed on the host
    const double *df;  // Δf itself: the time scale of the Lagrangian-averaged dynamic coefficient (dynamic_coefficient.jl:253)
    std::vector<double> h_dzc, h_dzf;
    // why the advection scheme cannot be evaluated on this grid (empty: it can). A grid whose halo is smaller than the scheme needs
    // -- RectilinearGrid(halo = (1, 1, 1)), what test/test_halo_regions.jl fills -- serves fields, halo fills and the Poisson
    // solvers; tendencies and models need the halo the reference's model constructor would inflate it to.
    std::string advection_error;
    // scratch t of the vertically implicit solve (ocn_implicit_z.h), Nx Ny Nz, allocated on first use
    double *ivd_scratch = nullptr;
    // partial sums of the open-boundary mass flux (ocn_open_boundary.h): one per block of all six faces and one total, allocated on first use
    double *ob_partial = nullptr;
    // node coordinates for particles and point interpolation (ocn_grid_set_nodes): the geometry the index computation reads; `znodes` holds
    // the Nz + 1 face and Nz centre nodes of a stretched z on the device
    PGeom pg = {};
    bool has_nodes = false;
    double *znodes = nullptr;
    // partial results of the diagnostics' reductions (ocn_diagnostics.h): grow-only, allocated on first use
    double *diag_slab = nullptr;
    size_t diag_slab_n = 0;
    // the lowered stencil program of the diagnostic being launched (ocn_diagnostics.h): DG_ST_MAX_INS instructions, allocated on first use
    DgStIns *diag_program = nullptr;
    // ... its host copy, which the queued transfer reads, and the event that says the transfer has read it
    std::vector<DgStIns> diag_program_h;
    hipEvent_t diag_program_copied = nullptr;
    // node tables for functions of the coordinates (ocn_grid_set_node_tables): per direction N + 1 face and N centre nodes, one device block
    double *node_tables = nullptr;
    const double *nodes_f[3] = {}, *nodes_c[3] = {};
    // a grid-fitted immersed boundary (ocn_grid_set_immersed_boundary, ocn_immersed.h): the periphery bytes and the orders words, both
    // parent-shaped at ccc (NULL: none), and the number of live models on the grid -- the boundary may not change under one
    unsigned char *imm_periph = nullptr;
    unsigned short *imm_orders = nullptr;
    int models = 0;
};

static void parent_size(const DGrid &g, const int loc[3], int P[3]) {
    const int N[3] = {g.Nx, g.Ny, g.Nz}, H[3] = {g.Hx, g.Hy, g.Hz}, T[3] = {g.tx, g.ty, g.tz};
    // Face fields hold N + 1 points where the direction ends in a wall on the HIGH side: Bounded and LeftConnected (grid_utils.jl:43-68)
    for (int d = 0; d < 3; ++d) P[d] = N[d] + 2 * H[d] + ((loc[d] == OCN_FACE && wall_hi(T[d])) ? 1 : 0);
}

static FView make_view(const DGrid &g, const double *p, const int loc[3]) {
    int P[3];
    parent_size(g, loc, P);
    FView v;
    v.p = const_cast<double *>(p);
    v.s1 = P[0];
    v.s2 = (long)P[0] * P[1];
    v.off = (g.Hx - 1) + (long)v.s1 * (g.Hy - 1) + v.s2 * (g.Hz - 1);
    return v;
}

// the immersed tables of a grid as the kernels read them (periph == NULL: the grid has no boundary)
static ImmView imm_view(const ocn_grid_s *grid) {
    const DGrid &g = grid->d;
    ImmView v = {};
    v.periph = grid->imm_periph; v.orders = grid->imm_orders;
    const long P0 = g.Nx + 2 * g.Hx, P1 = g.Ny + 2 * g.Hy;
    v.sx = g.tx == OCN_FLAT ? 0 : 1;
    v.sy = g.ty == OCN_FLAT ? 0 : (int)P0;
    v.sz = g.tz == OCN_FLAT ? 0 : P0 * P1;
    v.off = (long)v.sx * (g.Hx - 1) + (long)v.sy * (g.Hy - 1) + v.sz * (g.Hz - 1);
    return v;
}
static bool is_immersed(const ocn_grid_s *grid) { return grid && grid->imm_periph != nullptr; }

static const int LOC_U[3] = {OCN_FACE, OCN_CENTER, OCN_CENTER};
static const int LOC_V[3] = {OCN_CENTER, OCN_FACE, OCN_CENTER};
static const int LOC_W[3] = {OCN_CENTER, OCN_CENTER, OCN_FACE};
static const int LOC_C[3] = {OCN_CENTER, OCN_CENTER, OCN_CENTER};

extern "C" int ocn_grid_create(ocn_grid_t *grid, const int N[3], const int H[3], const int topo[3], const double L[3],
                               double dx, double dy, double dz, const double *dzc, const double *dzf) {
    NEED_INIT();
    if (!grid || !N || !H || !topo || !L) return fail(OCN_EINVAL, "NULL argument");
    std::string adv_error;
    for (int d = 0; d < 3; ++d) {
        if (N[d] < 1) return fail(OCN_EINVAL, "size must be positive (dimension %d)", d);
        if (topo[d] == OCN_FLAT) {
            // Flat direction: one cell, no halo, unit spacing (validate_size / validate_halo of Grids/input_validation.jl)
            if (N[d] != 1 || H[d] != 0) return fail(OCN_EINVAL, "a Flat direction has size 1 and halo 0 (dimension %d)", d);
            const double spacing = d == 0 ? dx : (d == 1 ? dy : dz);
            if (spacing != 1.0 || L[d] != 1.0 || (d == 2 && dzc)) return fail(OCN_EINVAL, "a Flat direction has unit spacing and extent (dimension %d)", d);
            continue;
        }
        const bool connected = topo[d] == OCN_CONNECTED || topo[d] == OCN_RIGHT_CONNECTED || topo[d] == OCN_LEFT_CONNECTED;
        if (topo[d] != OCN_PERIODIC && topo[d] != OCN_BOUNDED && !(connected && d < 2))
            return fail(OCN_ENOTSUP, "topology code %d in dimension %d: only Periodic, Bounded, Flat and (x, y only) Fully / Right / LeftConnected "
                                     "are accelerated", topo[d], d);
        // adapt_advection_order (Advection/adapt_advection_order.jl:90-96): WENO(order=5) stays where N >= 3 and becomes
        // WENO(order = 2N-1) = WENO{2} where N = 2; the halo must hold the adapted scheme's buffer (nonhydrostatic_model.jl:184,
        // inflate_grid_halo_size). N = 1 in a non-Flat direction is refused: the reference keeps Centered(order=4) for the
        // advecting velocities of the OTHER directions' fluxes, which reads two cells into a one-cell halo there.
        char why[256] = "";
        const int B = N[d] >= 3 ? 3 : N[d];
        if (N[d] < 2) snprintf(why, sizeof why, "size 1 in non-Flat dimension %d: make the direction Flat (the reference's adapted "
                                                "UpwindBiased(order=1) scheme reads beyond its one-cell halo)", d);
        else if (H[d] < B) snprintf(why, sizeof why, "halo %d < %d in dimension %d: %s requires halo >= %d", H[d], B, d,
                                    B == 3 ? "WENO(order=5)" : "WENO(order=3)", B);
        if (why[0] && adv_error.empty()) adv_error = why;
        if (H[d] < 1) return fail(OCN_EINVAL, "halo %d < 1 in dimension %d", H[d], d);
        if (N[d] < H[d]) return fail(OCN_EINVAL, "size %d < halo %d in dimension %d", N[d], H[d], d);
        if (!(L[d] > 0)) return fail(OCN_EINVAL, "extent must be positive");
    }
    if (!(dx > 0) || !(dy > 0)) return fail(OCN_EINVAL, "dx, dy must be positive");
    if ((dzc == nullptr) != (dzf == nullptr)) return fail(OCN_EINVAL, "pass both dzc and dzf or neither");
    if (!dzc && !(dz > 0)) return fail(OCN_EINVAL, "dz must be positive for a z-regular grid");
    if (dzc && topo[2] != OCN_BOUNDED)
        return fail(OCN_ENOTSUP, "stretched z requires Bounded z topology (FourierTridiagonalPoissonSolver, "
                                 "fourier_tridiagonal_poisson_solver.jl:88-92)");
    ocn_grid_s *g = new ocn_grid_s();
    g->advection_error = adv_error;
    DGrid &D = g->d;
    D.Nx = N[0]; D.Ny = N[1]; D.Nz = N[2];
    D.Hx = H[0]; D.Hy = H[1]; D.Hz = H[2];
    D.tx = topo[0]; D.ty = topo[1]; D.tz = topo[2];
    D.dx = dx; D.dy = dy; D.az = dx * dy;
    D.rdx = 1.0 / dx; D.rdy = 1.0 / dy;
    D.Bx = (topo[0] == OCN_FLAT || N[0] >= 3) ? 3 : N[0];
    D.By = (topo[1] == OCN_FLAT || N[1] >= 3) ? 3 : N[1];
    D.Bz = (topo[2] == OCN_FLAT || N[2] >= 3) ? 3 : N[2];
    for (int d = 0; d < 3; ++d) g->L[d] = L[d];
    const int n = N[2] + 2 * H[2] + 1;
    g->h_dzc.resize(n); g->h_dzf.resize(n);
    g->z_regular = true;
    for (int q = 0; q < n; ++q) {
        g->h_dzc[q] = dzc ? dzc[q] : dz;
        g->h_dzf[q] = dzf ? dzf[q] : dz;
        if (!(g->h_dzc[q] > 0) || !(g->h_dzf[q] > 0)) { delete g; return fail(OCN_EINVAL, "z spacings must be positive"); }
    }
    for (int k = 1; k <= N[2]; ++k)
        if (g->h_dzc[k - 1 + H[2]] != g->h_dzc[H[2]] || g->h_dzf[k - 1 + H[2]] != g->h_dzc[H[2]]) g->z_regular = false;
    std::vector<double> tab(10 * (size_t)n);
    for (int q = 0; q < n; ++q) {
        const double zc = g->h_dzc[q], zf = g->h_dzf[q];
        tab[0 * n + q] = zc;
        tab[1 * n + q] = zf;
        tab[2 * n + q] = dy * zc;                       // Axᶠᶜᶜ = Δy Δz   (spacings_and_areas_and_volumes.jl:308-335)
        tab[3 * n + q] = dx * zc;                       // Ayᶜᶠᶜ = Δx Δz
        tab[4 * n + q] = 1.0 / ((dx * dy) * zc);        // V⁻¹ = 1 / (Az Δz)  (:369-378, reciprocal_metric_operators.jl)
        tab[5 * n + q] = 1.0 / ((dx * dy) * zf);
        tab[6 * n + q] = 1.0 / zf;
        tab[7 * n + q] = 1.0 / zc;
        const double df = std::cbrt((dx * dy) * zc);
        tab[8 * n + q] = df * df;
        tab[9 * n + q] = df;
    }
    hipError_t e = dev_alloc((void **)&g->tables, tab.size() * sizeof(double));
    if (e != hipSuccess) { delete g; return fail((int)e, "dev_alloc(grid tables): %s", hipGetErrorString(e)); }
    e = hipMemcpy(g->tables, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(g->tables); delete g; return fail((int)e, "hipMemcpy(grid tables): %s", hipGetErrorString(e)); }
    D.dzc = g->tables; D.dzf = g->tables + n; D.ax = g->tables + 2 * n; D.ay = g->tables + 3 * n;
    D.vinv_c = g->tables + 4 * n; D.vinv_f = g->tables + 5 * n; D.rdzf = g->tables + 6 * n;
    D.rdzc = g->tables + 7 * n;
    g->df2 = g->tables + 8 * n;
    g->df = g->tables + 9 * n;
    *grid = g;
    return OCN_OK;
}

extern "C" int ocn_grid_destroy(ocn_grid_t grid) {
    if (!grid) return OCN_OK;
    hipFree(grid->tables);
    hipFree(grid->ivd_scratch);
    hipFree(grid->ob_partial);
    hipFree(grid->znodes);
    hipFree(grid->diag_slab);
    hipFree(grid->diag_program);
    if (grid->diag_program_copied) hipEventDestroy(grid->diag_program_copied);
    hipFree(grid->node_tables);
    hipFree(grid->imm_periph);
    hipFree(grid->imm_orders);
    delete grid;
    return OCN_OK;
}

// the node coordinates of the grid (grid.xᶠᵃᵃ[1], grid.xᶜᵃᵃ[1], grid.xᶠᵃᵃ[Nx + 1] and so on per direction): what fractional_x_index / xnode
// read (Fields/interpolate.jl:67-83,137-188). The grid is created from spacings; its origin arrives here. zf / zc: HOST arrays of the
// Nz + 1 face and Nz centre nodes, needed for a stretched z and ignored for a regular one.
extern "C" int ocn_grid_set_nodes(ocn_grid_t grid, const double first_face[3], const double first_center[3], const double last_face[3],
                                  const double *zf, const double *zc) {
    NEED_INIT();
    if (!grid || !first_face || !first_center || !last_face) return fail(OCN_EINVAL, "NULL argument");
    const DGrid &D = grid->d;
    if (!grid->z_regular && (!zf || !zc)) return fail(OCN_EINVAL, "a stretched z needs its face and centre nodes");
    PGeom pg = {};
    const int N[3] = {D.Nx, D.Ny, D.Nz}, H[3] = {D.Hx, D.Hy, D.Hz}, T[3] = {D.tx, D.ty, D.tz};
    const double d[3] = {D.dx, D.dy, grid->h_dzc[D.Hz]};
    for (int q = 0; q < 3; ++q) {
        pg.N[q] = N[q]; pg.H[q] = H[q]; pg.T[q] = T[q];
        pg.f0[q] = first_face[q]; pg.c0[q] = first_center[q]; pg.d[q] = d[q];
        pg.xL[q] = first_face[q]; pg.xR[q] = last_face[q];
    }
    double *zn = nullptr;
    if (!grid->z_regular) {
        const size_t nf = (size_t)D.Nz + 1, nc = (size_t)D.Nz;
        hipError_t e = dev_alloc((void **)&zn, (nf + nc) * sizeof(double));
        if (e != hipSuccess) return fail((int)e, "dev_alloc(z nodes): %s", hipGetErrorString(e));
        e = hipMemcpy(zn, zf, nf * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(zn + nf, zc, nc * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) { hipFree(zn); return fail((int)e, "hipMemcpy(z nodes): %s", hipGetErrorString(e)); }
        pg.zf = zn; pg.zc = zn + nf;
    }
    HIP_TRY(hipStreamSynchronize(g_stream));          // a launch already queued may still read the old table
    hipFree(grid->znodes);
    grid->znodes = zn;
    grid->pg = pg;
    grid->has_nodes = true;
    return OCN_OK;
}

// the node tables (grid.xᶠᵃᵃ[1 .. N + 1], grid.xᶜᵃᵃ[1 .. N] per direction; one node each in a Flat direction): elements of Julia ranges on the
// reference's side, so they are copied, not recomputed
extern "C" int ocn_grid_set_node_tables(ocn_grid_t grid, const double *const faces[3], const double *const centers[3]) {
    NEED_INIT();
    if (!grid || !faces || !centers) return fail(OCN_EINVAL, "NULL argument");
    const DGrid &D = grid->d;
    const int N[3] = {D.Nx, D.Ny, D.Nz}, T[3] = {D.tx, D.ty, D.tz};
    std::vector<double> h;
    size_t at_f[3], at_c[3];
    for (int d = 0; d < 3; ++d) {
        if (!faces[d] || !centers[d]) return fail(OCN_EINVAL, "NULL node table in dimension %d", d);
        const int nf = T[d] == OCN_FLAT ? 1 : N[d] + 1, nc = T[d] == OCN_FLAT ? 1 : N[d];
        at_f[d] = h.size(); h.insert(h.end(), faces[d], faces[d] + nf);
        at_c[d] = h.size(); h.insert(h.end(), centers[d], centers[d] + nc);
    }
    // The block is allocated once per grid and rewritten IN PLACE by a later call (its size depends on the grid only): the programs of
    // boundary and forcing functions hold addresses inside it (BfFunction::xa, FfFunction::x) for as long as their model lives.
    double *dev = grid->node_tables;
    if (!dev) {
        hipError_t e = dev_alloc((void **)&dev, h.size() * sizeof(double));
        if (e != hipSuccess) return fail((int)e, "dev_alloc(node tables): %s", hipGetErrorString(e));
    }
    HIP_TRY(hipStreamSynchronize(g_stream));          // a launch already queued may still read the old nodes
    hipError_t e = hipMemcpy(dev, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (!grid->node_tables) hipFree(dev); return fail((int)e, "hipMemcpy(node tables): %s", hipGetErrorString(e)); }
    grid->node_tables = dev;
    for (int d = 0; d < 3; ++d) { grid->nodes_f[d] = dev + at_f[d]; grid->nodes_c[d] = dev + at_c[d]; }
    return OCN_OK;
}

extern "C" int ocn_grid_parent_size(ocn_grid_t grid, const int loc[3], int P[3]) {
    if (!grid || !loc || !P) return fail(OCN_EINVAL, "NULL argument");
    parent_size(grid->d, loc, P);
    return OCN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// launch helpers (Utils/kernel_launching.jl: `launch!`, `interior_work_layout`)
// ---------------------------------------------------------------------------------------------------------------------
static inline dim3 grid3(int nx, int ny, int nz, dim3 block) {
    return dim3((nx + block.x - 1) / block.x, (ny + block.y - 1) / block.y, nz);
}
static const dim3 BLK(64, 4, 1);

// kernel_launching.jl:145-195: exclude_periphery drops the first Face index on Bounded dims
static Range6 default_range(const DGrid &g, const int loc[3], bool exclude_periphery) {
    const int N[3] = {g.Nx, g.Ny, g.Nz}, T[3] = {g.tx, g.ty, g.tz};
    int lo[3];
    for (int d = 0; d < 3; ++d)
        // periphery_offset (kernel_launching.jl:145-146) is defined for Bounded; a RightConnected rank owns the same wall face and gets
        // the same exclusion here, so its fields equal the serial run's (the reference launches over that face and resets it by the fill)
        lo[d] = 1 + ((exclude_periphery && loc[d] == OCN_FACE && wall_lo(T[d]) && N[d] > 1) ? 1 : 0);
    return Range6{lo[0], N[0], lo[1], N[1], lo[2], N[2]};
}

static int check_range(const DGrid &g, const int *range, Range6 *out, const int loc[3] = nullptr, bool exclude_periphery = false) {
    if (!range) { if (out) *out = default_range(g, loc, exclude_periphery); return OCN_OK; }
    Range6 r{range[0], range[1], range[2], range[3], range[4], range[5]};
    // stencils reach 3 cells: the tendency of cell i needs psi[i-3 .. i+3]
    if (r.i0 < 1 || r.j0 < 1 || r.k0 < 1 || r.i1 > g.Nx || r.j1 > g.Ny || r.k1 > g.Nz)
        return fail(OCN_EINVAL, "kernel range (%d:%d, %d:%d, %d:%d) exceeds the interior", r.i0, r.i1, r.j0, r.j1, r.k0, r.k1);
    if (out) *out = r;
    return OCN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// halo fills
// ---------------------------------------------------------------------------------------------------------------------
#include "ocn_boundary_conditions.h"   // the kernels and the launchers fill_halo_regions, validate_bc, compute_flux_bcs, compute_linear_flux_bc

extern "C" int ocn_fill_halo_regions(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields, int fill_open_bcs) {
    NEED_INIT();
    if (!grid || !fields || !locs || nfields < 0) return fail(OCN_EINVAL, "invalid argument");
    return fill_halo_regions(g_defaults, grid, fields, locs, nfields, fill_open_bcs != 0);
}

extern "C" int ocn_fill_halo_regions_bcs(ocn_grid_t grid, double *const *fields, const int (*locs)[3], int nfields,
                                         const ocn_bc_t (*bcs)[6], int fill_open_bcs) {
    NEED_INIT();
    if (!grid || !fields || !locs || nfields < 0) return fail(OCN_EINVAL, "invalid argument");
    if (bcs)
        for (int f = 0; f < nfields; ++f)
            for (int sd = 0; sd < 6; ++sd) {
                int rc = validate_bc(grid->d, locs[f], sd, bcs[f][sd].kind);
                if (rc) return rc;
            }
    return fill_halo_regions(g_defaults, grid, fields, locs, nfields, fill_open_bcs != 0, bcs);
}

extern "C" int ocn_compute_linear_flux_bc(ocn_grid_t grid, double *G, const int loc[3], int side, double a, double b, const double *dep) {
    NEED_INIT();
    if (!grid || !G || !loc || !dep || side < 0 || side > 5) return fail(OCN_EINVAL, "invalid argument");
    return compute_linear_flux_bc(grid->d, G, loc, side, a, b, dep);
}

extern "C" int ocn_compute_flux_bcs(ocn_grid_t grid, double *G, const int loc[3], const ocn_bc_t bcs[6]) {
    NEED_INIT();
    if (!grid || !G || !loc || !bcs) return fail(OCN_EINVAL, "NULL argument");
    for (int sd = 0; sd < 6; ++sd) {
        int rc = validate_bc(grid->d, loc, sd, bcs[sd].kind);
        if (rc) return rc;
    }
    return compute_flux_bcs(grid->d, G, loc, bcs);
}

// ---------------------------------------------------------------------------------------------------------------------
// immersed boundaries (ocn_immersed.h)
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int ocn_grid_set_immersed_boundary(ocn_grid_t grid, const unsigned char *immersed_cell) {
    NEED_INIT();
    if (!grid) return fail(OCN_EINVAL, "NULL argument");
    if (grid->models > 0) return fail(OCN_ESTATE, "the immersed boundary of a grid is set before a model is created on it (%d live)", grid->models);
    const DGrid &g = grid->d;
    HIP_TRY(hipStreamSynchronize(g_stream));          // a launch already queued may still read the old tables
    if (!immersed_cell) {
        hipFree(grid->imm_periph); hipFree(grid->imm_orders);
        grid->imm_periph = nullptr; grid->imm_orders = nullptr;
        return OCN_OK;
    }
    auto connected = [](int t) { return t == OCN_CONNECTED || t == OCN_RIGHT_CONNECTED || t == OCN_LEFT_CONNECTED; };
    if (connected(g.tx) || connected(g.ty)) return fail(OCN_ENOTSUP, "ImmersedBoundaryGrid on a partitioned grid is not built");
    ImmGeometry G = {{g.Nx, g.Ny, g.Nz}, {g.Hx, g.Hy, g.Hz}, {g.tx, g.ty, g.tz}};
    const int B[3] = {g.Bx, g.By, g.Bz};
    for (int d = 0; d < 3; ++d)
        if (G.T[d] != OCN_FLAT && G.H[d] < B[d] + 1)
            return fail(OCN_EINVAL, "halo %d < %d in dimension %d: an immersed grid needs the advection buffer + 1 "
                                    "(inflate_halo_size_one_dimension(req, old, _, ::ImmersedBoundaryGrid) = max(req + 1, old))", G.H[d], B[d] + 1, d);
    const size_t n = (size_t)(g.Nx + 2 * g.Hx) * (g.Ny + 2 * g.Hy) * (g.Nz + 2 * g.Hz);
    unsigned char *cell = nullptr, *periph = grid->imm_periph;
    unsigned short *orders = grid->imm_orders;
    hipError_t e = dev_alloc((void **)&cell, n);
    if (e == hipSuccess && !periph) e = dev_alloc((void **)&periph, n);
    if (e == hipSuccess && !orders) e = dev_alloc((void **)&orders, n * sizeof(unsigned short));
    if (e == hipSuccess) e = hipMemcpy(cell, immersed_cell, n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(immersed_flags_kernel, grid3(g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz, BLK), BLK, 0, g_stream, G,
                           (const unsigned char *)cell, periph, orders);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);          // `cell` is released below
    }
    hipFree(cell);
    if (e != hipSuccess) {
        if (!grid->imm_periph) hipFree(periph);
        if (!grid->imm_orders) hipFree(orders);
        return fail((int)e, "ocn_grid_set_immersed_boundary: %s", hipGetErrorString(e));
    }
    grid->imm_periph = periph; grid->imm_orders = orders;
    return OCN_OK;
}

extern "C" int ocn_grid_get_immersed_flags(ocn_grid_t grid, unsigned char *periphery, unsigned short *orders) {
    NEED_INIT();
    if (!grid) return fail(OCN_EINVAL, "NULL argument");
    if (!is_immersed(grid)) return fail(OCN_ESTATE, "the grid has no immersed boundary");
    const DGrid &g = grid->d;
    const size_t n = (size_t)(g.Nx + 2 * g.Hx) * (g.Ny + 2 * g.Hy) * (g.Nz + 2 * g.Hz);
    HIP_TRY(hipStreamSynchronize(g_stream));
    if (periphery) HIP_TRY(hipMemcpy(periphery, grid->imm_periph, n, hipMemcpyDeviceToHost));
    if (orders) HIP_TRY(hipMemcpy(orders, grid->imm_orders, n * sizeof(unsigned short), hipMemcpyDeviceToHost));
    return OCN_OK;
}

// the periphery bit mask_immersed_field! tests for a field at `loc`; -1: (Face, Face, Face), which no field of the model has
static int imm_location_bit(const int loc[3]) {
    const int faces = (loc[0] == OCN_FACE ? 1 : 0) | (loc[1] == OCN_FACE ? 2 : 0) | (loc[2] == OCN_FACE ? 4 : 0);
    static const int bit_of[8] = {IMM_CCC, IMM_FCC, IMM_CFC, IMM_FFC, IMM_CCF, IMM_FCF, IMM_CFF, -1};
    return bit_of[faces];
}

// mask_immersed_field! of n fields in one launch; nothing on a grid without a boundary
static int mask_immersed_fields(const ocn_grid_s *grid, double *const *fields, const int (*locs)[3], int n, double value) {
    if (!is_immersed(grid) || n <= 0) return OCN_OK;
    const DGrid &g = grid->d;
    ImmMaskList L = {};
    L.n = n;
    for (int q = 0; q < n; ++q) {
        L.f[q] = make_view(g, fields[q], locs[q]);
        L.bit[q] = imm_location_bit(locs[q]);
        if (L.bit[q] < 0) return fail(OCN_EINVAL, "mask_immersed_field: no field lives at (Face, Face, Face)");
    }
    hipLaunchKernelGGL(mask_immersed_kernel, grid3(g.Nx, g.Ny, g.Nz * n, BLK), BLK, 0, g_stream, imm_view(grid), L, value, g.Nx, g.Ny, g.Nz);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_mask_immersed_field(ocn_grid_t grid, double *field, const int loc[3], double value) {
    NEED_INIT();
    if (!grid || !field || !loc) return fail(OCN_EINVAL, "NULL argument");
    double *f[1] = {field};
    const int l[1][3] = {{loc[0], loc[1], loc[2]}};
    return mask_immersed_fields(grid, f, l, 1, value);
}

// what an immersed grid does not serve: OCN_ENOTSUP naming the grid and the feature
static int refuse_immersed(const ocn_grid_s *grid, const char *feature) {
    if (!is_immersed(grid)) return OCN_OK;
    return fail(OCN_ENOTSUP, "%s is not served on an ImmersedBoundaryGrid", feature);
}

// ---------------------------------------------------------------------------------------------------------------------
// tendencies
// ---------------------------------------------------------------------------------------------------------------------
template <int F>
static int launch_tendency(const DGrid &g, const double *u, const double *v, const double *w, const double *c, double *G,
                           const int *range, const ImmView *im = nullptr) {
    const int *loc = F == F_U ? LOC_U : (F == F_V ? LOC_V : (F == F_W ? LOC_W : LOC_C));
    Range6 r;
    int rc = check_range(g, range, &r, loc, F != F_C);
    if (rc) return rc;
    const int nx = r.i1 - r.i0 + 1, ny = r.j1 - r.j0 + 1, nz = r.k1 - r.k0 + 1;
    if (nx <= 0 || ny <= 0 || nz <= 0) return OCN_OK;   // "Don't launch kernels with no size" (kernel_launching.jl:370)
    FView fu = make_view(g, u, LOC_U), fv = make_view(g, v, LOC_V), fw = make_view(g, w, LOC_W);
    FView fc = make_view(g, c ? c : u, LOC_C), fG = make_view(g, G, loc);
    // on an immersed grid the advected field is u, v, w or c itself (immersed_tendency_kernel names it apart from the advecting velocities)
    if (im) hipLaunchKernelGGL((immersed_tendency_kernel<F, false>), grid3(nx, ny, nz, BLK), BLK, 0, g_stream, g, *im, fu, fv, fw,
                               F == F_U ? fu : (F == F_V ? fv : (F == F_W ? fw : fc)), fG, r);
    else hipLaunchKernelGGL(tendency_kernel<F>, grid3(nx, ny, nz, BLK), BLK, 0, g_stream, g, fu, fv, fw, fc, fG, r);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_compute_Gu(ocn_grid_t grid, const double *u, const double *v, const double *w, double *Gu, const int *range) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !Gu) return fail(OCN_EINVAL, "NULL argument");
    if (!grid->advection_error.empty()) return fail(OCN_EINVAL, "%s", grid->advection_error.c_str());
    const ImmView im = imm_view(grid);
    return launch_tendency<F_U>(grid->d, u, v, w, nullptr, Gu, range, is_immersed(grid) ? &im : nullptr);
}
extern "C" int ocn_compute_Gv(ocn_grid_t grid, const double *u, const double *v, const double *w, double *Gv, const int *range) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !Gv) return fail(OCN_EINVAL, "NULL argument");
    if (!grid->advection_error.empty()) return fail(OCN_EINVAL, "%s", grid->advection_error.c_str());
    const ImmView im = imm_view(grid);
    return launch_tendency<F_V>(grid->d, u, v, w, nullptr, Gv, range, is_immersed(grid) ? &im : nullptr);
}
extern "C" int ocn_compute_Gw(ocn_grid_t grid, const double *u, const double *v, const double *w, double *Gw, const int *range) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !Gw) return fail(OCN_EINVAL, "NULL argument");
    if (!grid->advection_error.empty()) return fail(OCN_EINVAL, "%s", grid->advection_error.c_str());
    const ImmView im = imm_view(grid);
    return launch_tendency<F_W>(grid->d, u, v, w, nullptr, Gw, range, is_immersed(grid) ? &im : nullptr);
}
extern "C" int ocn_compute_Gc(ocn_grid_t grid, const double *u, const double *v, const double *w, const double *c, double *Gc,
                              const int *range) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !c || !Gc) return fail(OCN_EINVAL, "NULL argument");
    if (!grid->advection_error.empty()) return fail(OCN_EINVAL, "%s", grid->advection_error.c_str());
    const ImmView im = imm_view(grid);
    return launch_tendency<F_C>(grid->d, u, v, w, c, Gc, range, is_immersed(grid) ? &im : nullptr);
}

static bool fused_path(const OcnOptions &o, const DGrid &g, const int *range, int ntr, int impl) {
    // the role kernel's limit is on the plane size, the all-fields kernel's on the array (4 GiB): a role launch falls back to the all-fields
    // kernel, and that one to the per-field kernels
    return (impl == 1 || impl == 2) && fused_tendency_supported(g, range) && ntr <= 3 &&
           ((impl == 2 && role_tendency_supported(o, g)) || fused_tendency_size_supported(g));
}

// whether an immersed grid's tendencies take the flux-sharing kernel (immersed_role_tendency_kernel): tendency_impl 2 (0 forces the per-field
// kernels), reference arithmetic, x and y Periodic, no Flat or reduced-order direction, planes the role kernel's offsets reach
static bool immersed_role_path(const OcnOptions &o, const DGrid &g, const int *range, int ntr, int impl) {
    return impl == 2 && o.arithmetic == 0 && ntr <= 3 && g.tx == OCN_PERIODIC && g.ty == OCN_PERIODIC && fused_tendency_supported(g, range) &&
           role_tendency_supported(o, g);
}

static int compute_tendencies(const OcnOptions &o, const DGrid &g, const double *u, const double *v, const double *w, const double *const *tr,
                              int ntr, double *Gu, double *Gv, double *Gw, double *const *Gc, const int *range, int impl,
                              const FusedSubstep *sub = nullptr, const ForcingTable *ftab = nullptr, const ImmView *im = nullptr) {
    // an immersed grid takes the immersed instantiation of the role kernel ("immersed_tendency_path" 2) where that kernel serves the grid
    // and tendency_impl asks for it, else the per-field kernels, one field per launch (path 1); the two give the same bits
    if (im) {
        if (sub || ftab) return fail(OCN_ESTATE, "fused substep or forcing requested in the tendency launch of an immersed grid");
        if (immersed_role_path(o, g, range, ntr, impl)) {
            int rc = check_range(g, range, nullptr);
            if (rc) return rc;
            if ((rc = launch_role_tendency_immersed(o, g, g_stream, u, v, w, tr, ntr, Gu, Gv, Gw, Gc, range, *im))) return fail(rc, "immersed role tendency launch failed");
            KERNEL_CHECK();
            return OCN_OK;
        }
        impl = 0;
    }
    if (sub && !fused_path(o, g, range, ntr, impl)) return fail(OCN_ESTATE, "fused substep requested on the per-field tendency path");
    if (ftab && !(impl == 2 && fused_path(o, g, range, ntr, impl) && role_tendency_supported(o, g)))
        return fail(OCN_ESTATE, "forcing term requested in a tendency launch other than the role kernel");
    if (fused_path(o, g, range, ntr, impl)) {
        int rc = check_range(g, range, nullptr);
        if (rc) return rc;
        if (impl == 2 && !role_tendency_supported(o, g)) impl = 1;          // planes too large for the role kernel's offsets: the all-fields kernel
        rc = impl == 2 ? launch_role_tendency(o, g, g_stream, u, v, w, tr, ntr, Gu, Gv, Gw, Gc, range, sub, ftab)
                       : launch_fused_tendency(o, g, g_stream, u, v, w, tr, ntr, Gu, Gv, Gw, Gc, range, sub);
        if (rc) return fail(rc, "fused tendency launch failed");
        KERNEL_CHECK();
        return OCN_OK;
    }
    int rc;
    if ((rc = launch_tendency<F_U>(g, u, v, w, nullptr, Gu, range, im))) return rc;
    if ((rc = launch_tendency<F_V>(g, u, v, w, nullptr, Gv, range, im))) return rc;
    if ((rc = launch_tendency<F_W>(g, u, v, w, nullptr, Gw, range, im))) return rc;
    for (int t = 0; t < ntr; ++t)
        if ((rc = launch_tendency<F_C>(g, u, v, w, tr[t], Gc[t], range, im))) return rc;
    return OCN_OK;
}

extern "C" int ocn_compute_tendencies(ocn_grid_t grid, const double *u, const double *v, const double *w,
                                      const double *const *tracers, int ntracers, double *Gu, double *Gv, double *Gw,
                                      double *const *Gc, const int *range) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !Gu || !Gv || !Gw || ntracers < 0 || ntracers > OCN_MAX_FIELDS - 3 ||
        (ntracers > 0 && (!tracers || !Gc)))
        return fail(OCN_EINVAL, "invalid argument");
    if (!grid->advection_error.empty()) return fail(OCN_EINVAL, "%s", grid->advection_error.c_str());
    // (the raw entry points map tendency_impl 0 to the all-fields kernel)
    const ImmView im = imm_view(grid);
    int rc = compute_tendencies(g_defaults, grid->d, u, v, w, tracers, ntracers, Gu, Gv, Gw, Gc, range, g_defaults.tendency_impl ? g_defaults.tendency_impl : 1,
                                nullptr, nullptr, is_immersed(grid) ? &im : nullptr);
    if (rc) return rc;
    KERNEL_CHECK();
    return OCN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// advection with advecting != advected (ocn_advect_split.h): the two advection terms of a model with background_fields
// ---------------------------------------------------------------------------------------------------------------------
static const int *field_loc(int f) { return f == 0 ? LOC_U : (f == 1 ? LOC_V : (f == 2 ? LOC_W : LOC_C)); }

template <int F>
static int launch_advective_tendency(const DGrid &g, const double *const adv[3], const double *psi, double *G, const int *range, bool accumulate,
                                     const ImmView *im = nullptr) {
    const int *loc = field_loc(F);
    Range6 r;
    int rc = check_range(g, range, &r, loc, F != F_C);
    if (rc) return rc;
    const int nx = r.i1 - r.i0 + 1, ny = r.j1 - r.j0 + 1, nz = r.k1 - r.k0 + 1;
    if (nx <= 0 || ny <= 0 || nz <= 0) return OCN_OK;
    const FView fu = make_view(g, adv[0], LOC_U), fv = make_view(g, adv[1], LOC_V), fw = make_view(g, adv[2], LOC_W);
    const FView fp = make_view(g, psi, loc), fG = make_view(g, G, loc);
    if (im) {
        if (accumulate) hipLaunchKernelGGL((immersed_tendency_kernel<F, true>), grid3(nx, ny, nz, BLK), BLK, 0, g_stream, g, *im, fu, fv, fw, fp, fG, r);
        else            hipLaunchKernelGGL((immersed_tendency_kernel<F, false>), grid3(nx, ny, nz, BLK), BLK, 0, g_stream, g, *im, fu, fv, fw, fp, fG, r);
    } else
    if (accumulate) hipLaunchKernelGGL((advective_tendency_kernel<F, true>), grid3(nx, ny, nz, BLK), BLK, 0, g_stream, g, fu, fv, fw, fp, fG, r);
    else            hipLaunchKernelGGL((advective_tendency_kernel<F, false>), grid3(nx, ny, nz, BLK), BLK, 0, g_stream, g, fu, fv, fw, fp, fG, r);
    KERNEL_CHECK();
    return OCN_OK;
}

// whether the split instantiation of the role kernel serves this grid: where the role kernel runs today (tendency_impl 2 on a grid both
// flux-sharing conditions hold for), in the reference's arithmetic -- the contracted arithmetic (option "arithmetic") has no split build
static bool split_role_path(const OcnOptions &o, const DGrid &g, int impl) {
    return impl == 2 && o.arithmetic == 0 && fused_tendency_supported(g, nullptr) && role_tendency_supported(o, g);
}

// -div(advection, adv, psi[f]) of the fields `roles` into G[f] (accumulate: G[f] -= div): one role-kernel launch, or one per-field
// launch each
static int advective_terms(const OcnOptions &o, const DGrid &g, const double *const adv[3], const double *const *psi, double *const *G,
                           const int *roles, int nrole, const int *range, bool accumulate, int impl, const ImmView *im = nullptr) {
    if (nrole <= 0) return OCN_OK;
    if (!im && split_role_path(o, g, impl)) {
        int rc = check_range(g, range, nullptr);
        if (rc) return rc;
        rc = launch_role_split(o, g, g_stream, adv, psi, G, roles, nrole, range, accumulate);
        if (rc) return fail(rc, "split role tendency launch failed");
        KERNEL_CHECK();
        return OCN_OK;
    }
    for (int q = 0; q < nrole; ++q) {
        const int f = roles[q];
        int rc = f == 0 ? launch_advective_tendency<F_U>(g, adv, psi[f], G[f], range, accumulate, im)
               : f == 1 ? launch_advective_tendency<F_V>(g, adv, psi[f], G[f], range, accumulate, im)
               : f == 2 ? launch_advective_tendency<F_W>(g, adv, psi[f], G[f], range, accumulate, im)
                        : launch_advective_tendency<F_C>(g, adv, psi[f], G[f], range, accumulate, im);
        if (rc) return rc;
    }
    return OCN_OK;
}

extern "C" int ocn_compute_advective_tendency(ocn_grid_t grid, const double *ua, const double *va, const double *wa, const double *psi,
                                              int which, double *G, const int *range, int accumulate) {
    NEED_INIT();
    if (!grid || !ua || !va || !wa || !psi || !G) return fail(OCN_EINVAL, "NULL argument");
    if (which < 0 || which > 3) return fail(OCN_EINVAL, "which is 0 (u), 1 (v), 2 (w) or 3 (tracer)");
    if (!grid->advection_error.empty()) return fail(OCN_EINVAL, "%s", grid->advection_error.c_str());
    const double *adv[3] = {ua, va, wa};
    const double *P[OCN_MAX_FIELDS] = {};
    double *Gs[OCN_MAX_FIELDS] = {};
    P[which] = psi; Gs[which] = G;
    const ImmView im = imm_view(grid);
    return advective_terms(g_defaults, grid->d, adv, P, Gs, &which, 1, range, accumulate != 0, g_defaults.tendency_impl, is_immersed(grid) ? &im : nullptr);
}

static int sum_parent(const DGrid &g, const double *a, const double *b, const int loc[3], double *out) {
    int P[3];
    parent_size(g, loc, P);
    const long n = (long)P[0] * P[1] * P[2];
    const int nb = (int)std::min<long>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(sum_parent_kernel, dim3(nb), dim3(256), 0, g_stream, a, b, out, n);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_sum_parent(ocn_grid_t grid, const double *a, const double *b, const int loc[3], double *out) {
    NEED_INIT();
    if (!grid || !a || !b || !loc || !out) return fail(OCN_EINVAL, "NULL argument");
    for (int d = 0; d < 3; ++d)
        if (loc[d] != OCN_CENTER && loc[d] != OCN_FACE) return fail(OCN_EINVAL, "loc[%d] is OCN_CENTER or OCN_FACE", d);
    return sum_parent(grid->d, a, b, loc, out);
}

// ---------------------------------------------------------------------------------------------------------------------
// diagnostics (ocn_diagnostics.h): computed fields, reductions, accumulations of one operation node
// ---------------------------------------------------------------------------------------------------------------------
static void dg_interior_size(const DGrid &g, const int loc[3], int n[3]) {
    const int N[3] = {g.Nx, g.Ny, g.Nz}, T[3] = {g.tx, g.ty, g.tz};
    for (int d = 0; d < 3; ++d) n[d] = N[d] + ((loc[d] == OCN_FACE && wall_hi(T[d])) ? 1 : 0);
}

// a field at `from` read at `to`: interpolation_operator(from, to) (interpolation_utils.jl:55-69) as a stencil corner and strides
static DgLeaf dg_make_leaf(const DGrid &g, const double *p, double c, const int from[3], const int to[3]) {
    DgLeaf l = {};
    l.p = p;
    l.c = c;
    if (!p) return l;
    const int H[3] = {g.Hx, g.Hy, g.Hz}, T[3] = {g.tx, g.ty, g.tz};
    int P[3];
    parent_size(g, from, P);
    const long st[3] = {1L, (long)P[0], (long)P[0] * P[1]};
    l.s1 = P[0];
    l.s2 = st[2];
    l.off = H[0] + st[1] * H[1] + st[2] * H[2];
    long dirs[3];
    for (int d = 0; d < 3; ++d) {
        if (T[d] == OCN_FLAT || from[d] == to[d]) continue;           // identity (interpolation_operators.jl:87-110)
        if (to[d] == OCN_FACE) l.off -= st[d];                        // ℑᶠ: f[i-1], f[i]; ℑᶜ: f[i], f[i+1]
        dirs[l.n++] = st[d];
    }
    // two directions nest as z of y of x (the lower direction innermost), three as x of y of z (interpolation_operators.jl:45-71)
    for (int q = 0; q < l.n; ++q) l.st[q] = l.n == 3 ? dirs[2 - q] : dirs[q];
    return l;
}

static int dg_make_operand(const ocn_grid_s *grid, const ocn_operand_t *op, DgOperand *o) {
    if (!grid || !op) return fail(OCN_EINVAL, "NULL argument");
    const DGrid &g = grid->d;
    const int T[3] = {g.tx, g.ty, g.tz};
    for (int d = 0; d < 3; ++d)
        if (T[d] == OCN_CONNECTED || T[d] == OCN_RIGHT_CONNECTED || T[d] == OCN_LEFT_CONNECTED)
            return fail(OCN_ENOTSUP, "diagnostics on a partitioned grid (connected topology in dimension %d) are not built", d);
    if (op->op < OCN_OP_IDENTITY || op->op > OCN_OP_DIV) return fail(OCN_EINVAL, "unknown operation code %d", op->op);
    const bool binary = op->op != OCN_OP_IDENTITY;
    if (!op->a && !(binary && op->b)) return fail(OCN_EINVAL, "the operation has no field operand (a%s NULL)", binary ? " and b are" : " is");
    const int *first = op->a ? op->loc_a : op->loc_b;
    for (int d = 0; d < 3; ++d) {
        if (op->loc[d] != OCN_CENTER && op->loc[d] != OCN_FACE) return fail(OCN_EINVAL, "loc[%d] is OCN_CENTER or OCN_FACE", d);
        if (op->a && op->loc_a[d] != OCN_CENTER && op->loc_a[d] != OCN_FACE) return fail(OCN_EINVAL, "loc_a[%d] is OCN_CENTER or OCN_FACE", d);
        if (binary && op->b && op->loc_b[d] != OCN_CENTER && op->loc_b[d] != OCN_FACE)
            return fail(OCN_EINVAL, "loc_b[%d] is OCN_CENTER or OCN_FACE", d);
        if (op->loc[d] != first[d])
            return fail(OCN_EINVAL, "the operation's location is that of its first field operand (dimension %d: %d != %d)", d, op->loc[d], first[d]);
    }
    *o = DgOperand{};
    o->op = op->op;
    o->a = dg_make_leaf(g, op->a, op->ca, op->loc_a, op->loc);
    if (binary) o->b = dg_make_leaf(g, op->b, op->cb, op->loc_b, op->loc);
    o->dz = op->loc[2] == OCN_FACE ? g.dzf : g.dzc;
    o->Hz = g.Hz;
    return OCN_OK;
}

// the metric of the directions in `mask` (reduction_grid_metric, metric_field_reductions.jl:12-21)
static void dg_set_metric(const DGrid &g, int mask, DgOperand *o) {
    const bool x = mask & 1, y = mask & 2, z = mask & 4;
    o->mc = (x && y) ? g.az : (x ? g.dx : g.dy);
    o->mmode = (x || y) ? (z ? 3 : 1) : 2;
}

static DgOut dg_make_out(const DGrid &g, const int loc[3], int reduced_mask, double *out) {
    const int H[3] = {g.Hx, g.Hy, g.Hz};
    int P[3];
    parent_size(g, loc, P);
    DgOut w = {};
    w.p = out;
    long stride = 1;
    for (int d = 0; d < 3; ++d) {
        const bool reduced = (reduced_mask >> d) & 1;
        w.s[d] = reduced ? 0 : stride;
        w.off += reduced ? 0 : H[d] * stride;
        stride *= reduced ? 1 : P[d];
    }
    return w;
}

// ---------------------------------------------------------------------------------------------------------------------
// boundary functions (ocn_boundary_function.h): programs of FluxBoundaryCondition(func, field_dependencies, parameters)
// ---------------------------------------------------------------------------------------------------------------------
// the ONE table of the ops on the host: value operands of an instruction (the leaves have none), -1 for an unknown op
static int expr_arity(int op) {
    switch (op) {
    case OCN_EXPR_CONST: case OCN_EXPR_COORD: case OCN_EXPR_TIME: case OCN_EXPR_FIELD: return 0;
    case OCN_EXPR_NEG: case OCN_EXPR_ABS: case OCN_EXPR_SQRT: case OCN_EXPR_EXP: case OCN_EXPR_LOG: case OCN_EXPR_SIN: case OCN_EXPR_COS:
    case OCN_EXPR_TANH: return 1;
    case OCN_EXPR_ADD: case OCN_EXPR_SUB: case OCN_EXPR_MUL: case OCN_EXPR_DIV: case OCN_EXPR_MIN: case OCN_EXPR_MAX: case OCN_EXPR_POW:
    case OCN_EXPR_LT: case OCN_EXPR_LE: case OCN_EXPR_GT: case OCN_EXPR_GE: return 2;
    case OCN_EXPR_SELECT: return 3;
    default: return -1;          // no op of the public enum
    }
}

static int no_connected_topology(const DGrid &g, const char *what) {
    const int T[3] = {g.tx, g.ty, g.tz};
    for (int d = 0; d < 3; ++d)
        if (T[d] == OCN_CONNECTED || T[d] == OCN_RIGHT_CONNECTED || T[d] == OCN_LEFT_CONNECTED)
            return fail(OCN_ENOTSUP, "%s on a partitioned grid (connected topology in dimension %d) are not built", what, d);
    return OCN_OK;
}

// every operand of every instruction names an earlier value (or is 0 where unused): nothing the kernel indexes with is left unchecked
// max_coord: the largest coordinate index (1 on a boundary: two tangential directions; 2 in the volume: x / y / z)
static int bf_validate_program(const ocn_expr_ins_t *program, int n, int ndeps, bool *reads_time, int max_coord = 1) {
    if (n < 1 || n > BF_MAX_INS) return fail(OCN_EINVAL, "a function program has 1..%d instructions; got %d", BF_MAX_INS, n);
    if (ndeps < 0 || ndeps > BF_MAX_DEPS) return fail(OCN_EINVAL, "a function program has 0..%d field dependencies; got %d", BF_MAX_DEPS, ndeps);
    if (!program) return fail(OCN_EINVAL, "NULL program");
    if (reads_time) *reads_time = false;
    for (int q = 0; q < n; ++q) {
        const ocn_expr_ins_t &I = program[q];
        const int values = expr_arity(I.op);          // how many of a, b, c are value operands
        if (values < 0) return fail(OCN_EINVAL, "instruction %d: unknown op %d", q, I.op);
        if (I.op == OCN_EXPR_TIME && reads_time) *reads_time = true;
        if (I.op == OCN_EXPR_COORD && (I.a < 0 || I.a > max_coord))
            return fail(OCN_EINVAL, "instruction %d: coordinate %d is not 0 %s", q, I.a, max_coord == 1 ? "or 1" : ".. 2");
        if (I.op == OCN_EXPR_FIELD && (I.a < 0 || I.a >= ndeps))
            return fail(OCN_EINVAL, "instruction %d: dependency slot %d outside 0..%d", q, I.a, ndeps - 1);
        const int operand[3] = {I.a, I.b, I.c};
        for (int w = 0; w < 3; ++w) {
            if (w < values) {
                if (operand[w] < 0 || operand[w] >= q) return fail(OCN_EINVAL, "instruction %d: operand %d is not an earlier value", q, operand[w]);
            } else if (operand[w] != 0 && !(w == 0 && (I.op == OCN_EXPR_COORD || I.op == OCN_EXPR_FIELD)))
                return fail(OCN_EINVAL, "instruction %d: an unused operand field is not 0", q);
        }
    }
    return OCN_OK;
}

// the function of a condition at `loc` on `side`: extents, coordinate tables, the stencils of its dependencies (dep_field[s]: slot of
// BfFields, at dep_locs[s]) and a copy of the validated program
static int bf_make_function(const ocn_grid_s *grid, const ocn_expr_ins_t *program, int n, const int loc[3], int side, const int *dep_field,
                            const int (*dep_locs)[3], int ndeps, double *out, BfFunction *fn) {
    const DGrid &g = grid->d;
    const int N[3] = {g.Nx, g.Ny, g.Nz}, H[3] = {g.Hx, g.Hy, g.Hz}, T[3] = {g.tx, g.ty, g.tz};
    if (const int rc = no_connected_topology(g, "boundary functions")) return rc;
    if (side < 0 || side > 5) return fail(OCN_EINVAL, "side %d out of range (0..5 = west, east, south, north, bottom, top)", side);
    const int d = side / 2, right = side & 1;
    if (!(right ? wall_hi(T[d]) : wall_lo(T[d]))) return fail(OCN_EINVAL, "side %d is not a wall of the grid (Bounded direction)", side);
    if (!grid->node_tables) return fail(OCN_ESTATE, "the grid has no node tables: call ocn_grid_set_node_tables");
    const int ta = d == 0 ? 1 : 0, tb = d == 2 ? 1 : 2;
    for (int q = 0; q < 3; ++q)
        if (q != d && loc[q] != OCN_CENTER && loc[q] != OCN_FACE) return fail(OCN_EINVAL, "loc[%d] is OCN_CENTER or OCN_FACE", q);
    *fn = BfFunction{};
    fn->n = n; fn->ndeps = ndeps;
    fn->Na = N[ta]; fn->Nb = N[tb];
    fn->out = out;
    fn->xa = loc[ta] == OCN_FACE ? grid->nodes_f[ta] : grid->nodes_c[ta];
    fn->xb = loc[tb] == OCN_FACE ? grid->nodes_f[tb] : grid->nodes_c[tb];
    for (int s = 0; s < ndeps; ++s) {
        const int *from = dep_locs[s];
        for (int q = 0; q < 3; ++q)
            if (from[q] != OCN_CENTER && from[q] != OCN_FACE) return fail(OCN_EINVAL, "dependency %d: loc[%d] is OCN_CENTER or OCN_FACE", s, q);
        int P[3];
        parent_size(g, from, P);
        const long st[3] = {1L, (long)P[0], (long)P[0] * P[1]};
        BfDep &D = fn->dep[s];
        D.field = dep_field[s];
        // interior point (1, 1, 1), moved to the boundary-normal index 1 / N (domain_boundary_indices): no interpolation along the normal
        D.off = H[0] + st[1] * H[1] + st[2] * H[2] + (right ? N[d] - 1 : 0) * st[d];
        D.sa = st[ta]; D.sb = st[tb];
        const int tang[2] = {ta, tb};
        for (int w = 0; w < 2; ++w) {
            const int q = tang[w];
            if (T[q] == OCN_FLAT || from[q] == loc[q]) continue;          // identity (interpolation_operators.jl:87-110)
            if (loc[q] == OCN_FACE) D.off -= st[q];                       // ℑᶠ: f[i-1], f[i]; ℑᶜ: f[i], f[i+1]
            D.st[D.n++] = st[q];                                          // the lower direction innermost (:45-71)
        }
    }
    memcpy(fn->ins, program, sizeof(ocn_expr_ins_t) * (size_t)n);
    return OCN_OK;
}

static void bf_launch(const BfFunction *table_d, int nfun, int na, int nb, const BfFields &fields, double time) {
    hipLaunchKernelGGL(boundary_function_kernel, dim3((na + BF_LANES - 1) / BF_LANES, (nb + BF_ROWS - 1) / BF_ROWS, nfun), dim3(BF_LANES, BF_ROWS), 0,
                       g_stream, table_d, fields, time);
}

extern "C" int ocn_evaluate_boundary_function(ocn_grid_t grid, const ocn_expr_ins_t *program, int n, const int loc[3], int side,
                                              const double *const *deps, const int (*dep_locs)[3], int ndeps, double time, double *out) {
    NEED_INIT();
    if (!grid || !loc || !out) return fail(OCN_EINVAL, "NULL argument");
    int rc = bf_validate_program(program, n, ndeps, nullptr);
    if (rc) return rc;
    if (ndeps > 0 && (!deps || !dep_locs)) return fail(OCN_EINVAL, "NULL dependencies");
    BfFields fields = {};
    int slots[BF_MAX_DEPS];
    for (int s = 0; s < ndeps; ++s) {
        if (!deps[s]) return fail(OCN_EINVAL, "dependency %d is NULL", s);
        fields.p[s] = deps[s];
        slots[s] = s;
    }
    BfFunction fn;
    if ((rc = bf_make_function(grid, program, n, loc, side, slots, dep_locs, ndeps, out, &fn))) return rc;
    BfFunction *table_d = nullptr;
    HIP_TRY(dev_alloc((void **)&table_d, sizeof(BfFunction)));
    hipError_t e = hipMemcpy(table_d, &fn, sizeof(BfFunction), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        bf_launch(table_d, 1, fn.Na, fn.Nb, fields, time);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);          // the table is this call's
    hipFree(table_d);
    if (e != hipSuccess) return fail((int)e, "boundary_function_kernel: %s", hipGetErrorString(e));
    return OCN_OK;
}


// ---------------------------------------------------------------------------------------------------------------------
// forcing functions (ocn_forcing_function.h): programs evaluated in the volume, their line and uniform values hoisted into tables
// ---------------------------------------------------------------------------------------------------------------------
// Host arithmetic only. Every value gets the set of inputs it depends on out of {x, y, z, field} (constants and t add nothing) and from it
// its class: FF_UNIFORM (none), FF_LINE + d (coordinate d only), FF_CELL (two coordinates, or a field). A uniform or line value that a
// cell instruction consumes, or that is the result, is a ROOT: it gets a table. The per-cell program is the cell instructions in their
// recorded order, each root operand replaced by ONE table load (FF_OP_TABLE, a = the root's value index until ff_make_function knows the
// tables' offsets). Nothing else changes: the same operations on the same operands.
struct FfPlan {
    int cls[BF_MAX_INS];
    bool root[BF_MAX_INS];
    int n_cell;
    ocn_expr_ins_t cell[BF_MAX_INS];
};
static void ff_make_plan(const ocn_expr_ins_t *program, int n, FfPlan *P) {
    int mask[BF_MAX_INS];
    for (int q = 0; q < n; ++q) {
        const ocn_expr_ins_t &I = program[q];
        const int operand[3] = {I.a, I.b, I.c};
        mask[q] = I.op == OCN_EXPR_COORD ? 1 << I.a : (I.op == OCN_EXPR_FIELD ? 8 : 0);
        for (int w = 0; w < expr_arity(I.op); ++w) mask[q] |= mask[operand[w]];
        P->cls[q] = mask[q] == 0 ? FF_UNIFORM : (mask[q] == 1 ? FF_LINE : (mask[q] == 2 ? FF_LINE + 1 : (mask[q] == 4 ? FF_LINE + 2 : FF_CELL)));
        P->root[q] = false;
    }
    int at[BF_MAX_INS], load[BF_MAX_INS];          // where a cell value / the load of a root sits in the per-cell program
    for (int q = 0; q < n; ++q) at[q] = load[q] = -1;
    int nc = 0;
    auto table_load = [&](int v) {
        if (load[v] < 0) {
            P->root[v] = true;
            load[v] = nc;
            P->cell[nc++] = ocn_expr_ins_t{FF_OP_TABLE, v, P->cls[v] == FF_UNIFORM ? 3 : P->cls[v] - FF_LINE, 0, 0.0};
        }
        return load[v];
    };
    for (int q = 0; q < n; ++q) {
        if (P->cls[q] != FF_CELL) continue;
        ocn_expr_ins_t I = program[q];
        int *operand[3] = {&I.a, &I.b, &I.c};
        for (int w = 0; w < expr_arity(I.op); ++w) {
            const int v = *operand[w];
            *operand[w] = P->cls[v] == FF_CELL ? at[v] : table_load(v);
        }
        at[q] = nc;
        P->cell[nc++] = I;
    }
    if (P->cls[n - 1] != FF_CELL) { nc = 0; load[n - 1] = -1; table_load(n - 1); }      // the result is a line or uniform value: one load per cell
    P->n_cell = nc;
}

extern "C" int ocn_forcing_function_plan(const ocn_expr_ins_t *program, int n, int ndeps, int *value_class, int *n_cell) {
    int rc = bf_validate_program(program, n, ndeps, nullptr, 2);
    if (rc) return rc;
    FfPlan P;
    ff_make_plan(program, n, &P);
    if (value_class) for (int q = 0; q < n; ++q) value_class[q] = P.cls[q];
    if (n_cell) *n_cell = P.n_cell;
    return OCN_OK;
}

// the function of a forcing of a field at `loc`: the plan, the coordinate tables, the stencils of its dependencies (dep_field[s]: slot of
// BfFields, at dep_locs[s]), a copy of the validated program and the device block of its root tables (the caller owns fn->tab)
static int ff_make_function(const ocn_grid_s *grid, const ocn_expr_ins_t *program, int n, const int loc[3], const int *dep_field,
                            const int (*dep_locs)[3], int ndeps, FfFunction *fn) {
    const DGrid &g = grid->d;
    const int H[3] = {g.Hx, g.Hy, g.Hz}, T[3] = {g.tx, g.ty, g.tz};
    int rc = no_connected_topology(g, "forcing functions");
    if (rc) return rc;
    if (!grid->node_tables) return fail(OCN_ESTATE, "the grid has no node tables: call ocn_grid_set_node_tables");
    for (int q = 0; q < 3; ++q)
        if (loc[q] != OCN_CENTER && loc[q] != OCN_FACE) return fail(OCN_EINVAL, "loc[%d] is OCN_CENTER or OCN_FACE", q);
    *fn = FfFunction{};
    fn->n = n; fn->ndeps = ndeps;
    for (int q = 0; q < n; ++q) {
        if (program[q].op == OCN_EXPR_COORD && T[program[q].a] == OCN_FLAT)
            return fail(OCN_EINVAL, "instruction %d: a coordinate along %c, which is Flat (the function takes the remaining coordinates only)", q, "xyz"[program[q].a]);
        fn->reads_time |= program[q].op == OCN_EXPR_TIME;
    }
    dg_interior_size(g, loc, fn->L);
    for (int d = 0; d < 3; ++d) fn->x[d] = loc[d] == OCN_FACE ? grid->nodes_f[d] : grid->nodes_c[d];
    for (int s = 0; s < ndeps; ++s) {
        const int *from = dep_locs[s];
        for (int q = 0; q < 3; ++q)
            if (from[q] != OCN_CENTER && from[q] != OCN_FACE) return fail(OCN_EINVAL, "dependency %d: loc[%d] is OCN_CENTER or OCN_FACE", s, q);
        int P[3];
        parent_size(g, from, P);
        const long st[3] = {1L, (long)P[0], (long)P[0] * P[1]};
        FfDep &D = fn->dep[s];
        D.field = dep_field[s];
        D.off = H[0] + st[1] * H[1] + st[2] * H[2];                        // interior point (1, 1, 1)
        D.s1 = st[1]; D.s2 = st[2];
        for (int q = 0; q < 3; ++q) {
            if (T[q] == OCN_FLAT || from[q] == loc[q]) continue;          // identity (interpolation_operators.jl:87-110)
            if (loc[q] == OCN_FACE) D.off -= st[q];                       // ℑᶠ: f[i-1], f[i]; ℑᶜ: f[i], f[i+1]
            D.st[D.n++] = st[q];                                          // the lower direction innermost (:45-71)
        }
    }
    memcpy(fn->ins, program, sizeof(ocn_expr_ins_t) * (size_t)n);
    FfPlan P;
    ff_make_plan(program, n, &P);
    long words = 0;
    for (int q = 0; q < n; ++q) {
        fn->cls[q] = (signed char)P.cls[q];
        fn->root[q] = -1;
        if (!P.root[q]) continue;
        fn->root[q] = (int)words;
        words += P.cls[q] == FF_UNIFORM ? 1 : fn->L[P.cls[q] - FF_LINE];
    }
    fn->n_cell = P.n_cell;
    for (int q = 0; q < P.n_cell; ++q) {
        fn->cell[q] = P.cell[q];
        if (P.cell[q].op == FF_OP_TABLE) fn->cell[q].a = fn->root[P.cell[q].a];
    }
    HIP_TRY(dev_alloc((void **)&fn->tab, sizeof(double) * (size_t)std::max(words, 1L)));
    return OCN_OK;
}

// the tables of functions [0, n) of `table_d` (time_only: of those that read t); Lmax: the longest line among them
static void ff_launch_lines(const FfTable *table_d, int n, int Lmax, double time, bool time_only) {
    hipLaunchKernelGGL(forcing_line_kernel, dim3((Lmax + FF_THREADS - 1) / FF_THREADS, 4, n), dim3(FF_THREADS), 0, g_stream, table_d, time,
                       time_only ? 1 : 0);
}
// whether a program holds none of exp, log, sin, cos, tanh, pow: its cells can take the arithmetic-only instantiation
static bool ff_arithmetic_only(const ocn_expr_ins_t *program, int n) {
    for (int q = 0; q < n; ++q)
        if (program[q].op >= OCN_EXPR_EXP && program[q].op <= OCN_EXPR_POW) return false;
    return true;
}
static void ff_launch_cells(const DGrid &g, const ForcingTable *tab_d, const FfTable *table_d, const ForcingLaunch &L, const BfFields &fields, int nx,
                            int ny, int nz, int slots, double time, bool hoist, bool assign, bool arithmetic) {
    hipLaunchKernelGGL(arithmetic ? forcing_function_kernel<true> : forcing_function_kernel<false>, dim3((nx + FF_LANES - 1) / FF_LANES, (ny + FF_ROWS - 1) / FF_ROWS, nz * L.n), dim3(FF_LANES, FF_ROWS),
                       sizeof(double) * FF_THREADS * (size_t)std::max(slots, 1), g_stream, g, tab_d, table_d, L, fields, nz, time, hoist ? 1 : 0,
                       assign ? 1 : 0);
}

extern "C" int ocn_evaluate_forcing_function(ocn_grid_t grid, const ocn_expr_ins_t *program, int n, const int loc[3], const double *const *deps,
                                             const int (*dep_locs)[3], int ndeps, double time, int hoist, double *out) {
    NEED_INIT();
    if (!grid || !loc || !out) return fail(OCN_EINVAL, "NULL argument");
    int rc = bf_validate_program(program, n, ndeps, nullptr, 2);
    if (rc) return rc;
    if (ndeps > 0 && (!deps || !dep_locs)) return fail(OCN_EINVAL, "NULL dependencies");
    BfFields fields = {};
    int slots[BF_MAX_DEPS];
    for (int s = 0; s < ndeps; ++s) {
        if (!deps[s]) return fail(OCN_EINVAL, "dependency %d is NULL", s);
        fields.p[s] = deps[s];
        slots[s] = s;
    }
    // one field (slot 0) with one function term over the interior of `loc`: the tables of a model, made for this call
    auto ft = std::make_unique<FfTable>();
    auto tab = std::make_unique<ForcingTable>();
    *ft = FfTable{}; *tab = ForcingTable{};
    FfFunction &fn = ft->fn[0];
    if ((rc = ff_make_function(grid, program, n, loc, slots, dep_locs, ndeps, &fn))) return rc;
    ft->n = 1;
    memset(ft->fn_of, -1, sizeof(ft->fn_of));
    ft->fn_of[0][0] = 0;
    tab->nterms[0] = 1;
    tab->t[0][0].kind = OCN_FORCING_KIND_FUNCTION;
    tab->r[0] = Range6{1, fn.L[0], 1, fn.L[1], 1, fn.L[2]};
    const FView v = make_view(grid->d, nullptr, loc);
    tab->s1[0] = v.s1; tab->s2[0] = v.s2; tab->off[0] = v.off;
    ForcingLaunch L = {};
    L.n = 1; L.f[0] = 0; L.U[0] = out; L.G[0] = out;
    FfTable *ft_d = nullptr;
    ForcingTable *tab_d = nullptr;
    hipError_t e = dev_alloc((void **)&ft_d, sizeof(FfTable));
    if (e == hipSuccess) e = dev_alloc((void **)&tab_d, sizeof(ForcingTable));
    if (e == hipSuccess) e = hipMemcpy(ft_d, ft.get(), sizeof(FfTable), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tab_d, tab.get(), sizeof(ForcingTable), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (hoist) ff_launch_lines(ft_d, 1, std::max(fn.L[0], std::max(fn.L[1], fn.L[2])), time, false);
        ff_launch_cells(grid->d, tab_d, ft_d, L, fields, fn.L[0], fn.L[1], fn.L[2], hoist ? fn.n_cell : fn.n, time, hoist != 0, true,
                        hoist ? ff_arithmetic_only(fn.cell, fn.n_cell) : ff_arithmetic_only(fn.ins, fn.n));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);          // the tables are this call's
    hipFree(ft_d); hipFree(tab_d); hipFree(fn.tab);
    if (e != hipSuccess) return fail((int)e, "forcing_function_kernel: %s", hipGetErrorString(e));
    return OCN_OK;
}

// the launches below serve both evaluators: O = DgOperand with lds = 0, O = DgStencil<..> with the bytes of its slots
// more dynamic LDS than the runtime grants by default (a CU has 160 KiB; 64 slots of a stencil program are 128 KiB)
#define DG_ALLOW_LDS(kernel, lds)                                                                                       \
    do {                                                                                                                \
        if ((lds) > 48 * 1024)                                                                                          \
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds))); \
    } while (0)

// The launches are templates on where they write as well: W = DgOut, the plain store, or DgOutFold, the running time average
// (ocn_time_average_*). dg_with_out hands `launch` the one the call asks for: `fold` is NULL for the plain entry points.
static int dg_check_fold(const ocn_time_fold_t *fold) {
    if (!fold) return fail(OCN_EINVAL, "NULL argument");
    if (!std::isfinite(fold->T_previous) || !std::isfinite(fold->dt) || !std::isfinite(fold->T_current))
        return fail(OCN_EINVAL, "time fold: T_previous = %g, dt = %g, T_current = %g must be finite", fold->T_previous, fold->dt, fold->T_current);
    if (fold->T_current <= 0) return fail(OCN_EINVAL, "time fold: T_current = %g must be positive", fold->T_current);
    if (fold->T_previous < 0) return fail(OCN_EINVAL, "time fold: T_previous = %g must not be negative", fold->T_previous);
    if (fold->first && fold->T_previous != 0) return fail(OCN_EINVAL, "time fold: the first sample of a window has T_previous = 0, not %g", fold->T_previous);
    return OCN_OK;
}

static DgOutFold dg_fold_out(const DgOut &w, const ocn_time_fold_t &fold) {
    DgOutFold f = {};
    static_cast<DgOut &>(f) = w;
    f.Tp = fold.T_previous;
    f.dt = fold.dt;
    f.Tc = fold.T_current;
    f.first = fold.first != 0;
    return f;
}

template <class F> static int dg_with_out(const DgOut &w, const ocn_time_fold_t *fold, F &&launch) {
    return fold ? launch(dg_fold_out(w, *fold)) : launch(w);
}

template <class O, class W>
static int dg_compute(ocn_grid_s *grid, const O &o, const int n[3], const W &out, size_t lds) {
    DG_ALLOW_LDS((dg_compute_kernel<O, W>), lds);
    hipLaunchKernelGGL((dg_compute_kernel<O, W>), grid3(n[0], n[1], n[2], BLK), BLK, lds, g_stream, o, out, n[0], n[1]);
    KERNEL_CHECK();
    return OCN_OK;
}

static int dg_compute_operation(ocn_grid_t grid, const ocn_operand_t *operand, const ocn_time_fold_t *fold, double *out) {
    if (int rc_ = refuse_immersed(grid, "a diagnostic (its reductions exclude immersed cells through a condition)")) return rc_;
    DgOperand o;
    int rc = dg_make_operand(grid, operand, &o);
    if (rc) return rc;
    int n[3];
    dg_interior_size(grid->d, operand->loc, n);
    if (fold && operand->op == OCN_OP_IDENTITY) {
        // a plain field: the whole parent array of the result, halos included (windowed_time_average.jl:224 broadcasts over parent)
        int P[3];
        parent_size(grid->d, operand->loc, P);
        const long np = (long)P[0] * P[1] * P[2];
        DgOut whole = {};
        whole.p = out;
        hipLaunchKernelGGL(dg_fold_parent_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, g_stream, operand->a, dg_fold_out(whole, *fold), np);
        KERNEL_CHECK();
        return OCN_OK;
    }
    return dg_with_out(dg_make_out(grid->d, operand->loc, 0, out), fold, [&](const auto &w) { return dg_compute(grid, o, n, w, 0); });
}

extern "C" int ocn_compute_operation(ocn_grid_t grid, const ocn_operand_t *operand, double *out) {
    NEED_INIT();
    if (!out) return fail(OCN_EINVAL, "NULL argument");
    return dg_compute_operation(grid, operand, nullptr, out);
}

extern "C" int ocn_time_average_operation(ocn_grid_t grid, const ocn_operand_t *operand, const ocn_time_fold_t *fold, double *result) {
    NEED_INIT();
    if (!result) return fail(OCN_EINVAL, "NULL argument");
    const int rc = dg_check_fold(fold);
    if (rc) return rc;
    return dg_compute_operation(grid, operand, fold, result);
}

// a field of any shape as the integrand (a reduced field has no location code): n doubles of its parent array
extern "C" int ocn_time_average_parent(const double *integrand, size_t n, const ocn_time_fold_t *fold, double *result) {
    NEED_INIT();
    if (!integrand || !result) return fail(OCN_EINVAL, "NULL argument");
    const int rc = dg_check_fold(fold);
    if (rc) return rc;
    if (n == 0 || n > 0x7fffffffL * 256L) return fail(OCN_EINVAL, "n = %zu: between 1 and 2^39", n);
    DgOut whole = {};
    whole.p = result;
    hipLaunchKernelGGL(dg_fold_parent_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g_stream, integrand, dg_fold_out(whole, *fold), (long)n);
    KERNEL_CHECK();
    return OCN_OK;
}

template <int KIND, class O, class W>
static int dg_reduce(ocn_grid_s *grid, const O &o, const int n[3], int mask, const W &out, size_t lds) {
    const bool rj = mask & 2, rk = mask & 4;
    const double count = (double)((mask & 1) ? n[0] : 1) * (rj ? n[1] : 1) * (rk ? n[2] : 1);
    const int e1 = rj ? 1 : n[1], e2 = rk ? 1 : n[2];
    if (!(mask & 1)) {
        DG_ALLOW_LDS((dg_reduce_cols_kernel<KIND, O, W>), lds);
        hipLaunchKernelGGL((dg_reduce_cols_kernel<KIND, O, W>), grid3(n[0], e1, e2, BLK), BLK, lds, g_stream, o, out, n[0], e1, rj ? n[1] : 1, rk ? n[2] : 1, count);
        KERNEL_CHECK();
        return OCN_OK;
    }
    DgRows R;
    R.n0 = n[0]; R.n1 = n[1]; R.n2 = n[2]; R.rj = rj; R.rk = rk;
    R.rows = (rj ? n[1] : 1) * (rk ? n[2] : 1);
    R.nch = (R.rows + DG_ROWS - 1) / DG_ROWS;
    R.count = count;
    const long nout = (long)e1 * e2, nslab = nout * R.nch;
    if (nslab > 0x7fffffffL) return fail(OCN_ENOTSUP, "reduction over %ld blocks", nslab);
    if (R.nch > 1 && grid->diag_slab_n < (size_t)(2 * nslab)) {
        HIP_TRY(hipStreamSynchronize(g_stream));              // a launch already queued may still read the old slab
        hipFree(grid->diag_slab);
        grid->diag_slab = nullptr;
        grid->diag_slab_n = 0;
        HIP_TRY(dev_alloc((void **)&grid->diag_slab, (size_t)(2 * nslab) * sizeof(double)));
        grid->diag_slab_n = (size_t)(2 * nslab);
    }
    DG_ALLOW_LDS((dg_reduce_rows_kernel<KIND, O, W>), lds);
    hipLaunchKernelGGL((dg_reduce_rows_kernel<KIND, O, W>), dim3((unsigned)nslab), dim3(DG_THREADS), lds, g_stream, o, R, out, grid->diag_slab, nslab);
    KERNEL_CHECK();
    if (R.nch > 1) {
        hipLaunchKernelGGL((dg_combine_kernel<KIND, W>), dim3((unsigned)nout), dim3(DG_THREADS), 0, g_stream, R, out, grid->diag_slab, nslab,
                           (int)(KIND == OCN_REDUCE_AVERAGE && o.mmode != 0));
        KERNEL_CHECK();
    }
    return OCN_OK;
}

template <class O, class W>
static int dg_reduce_kind(ocn_grid_s *grid, const O &o, int kind, const int n[3], int mask, const W &out, size_t lds) {
    switch (kind) {
    case OCN_REDUCE_SUM:     return dg_reduce<OCN_REDUCE_SUM>(grid, o, n, mask, out, lds);
    case OCN_REDUCE_MAXIMUM: return dg_reduce<OCN_REDUCE_MAXIMUM>(grid, o, n, mask, out, lds);
    case OCN_REDUCE_MINIMUM: return dg_reduce<OCN_REDUCE_MINIMUM>(grid, o, n, mask, out, lds);
    default:                 return dg_reduce<OCN_REDUCE_AVERAGE>(grid, o, n, mask, out, lds);
    }
}

// cumsum along direction dim of the operand's interior n
template <class O, class W>
static int dg_accumulate(const O &o, const int n[3], int dim, int reverse, const W &w, size_t lds) {
    const dim3 blk(64, 4, 1);
    if (dim == 0) {
        const long nrows = (long)n[1] * n[2];
        DG_ALLOW_LDS((dg_accumulate_rows_kernel<O, W>), lds);
        hipLaunchKernelGGL((dg_accumulate_rows_kernel<O, W>), dim3((unsigned)((nrows + 3) / 4)), dim3(DG_THREADS), lds, g_stream, o, w, n[0], n[1], nrows,
                           reverse != 0);
    } else if (dim == 1) {
        DG_ALLOW_LDS((dg_accumulate_cols_kernel<1, O, W>), lds);
        hipLaunchKernelGGL((dg_accumulate_cols_kernel<1, O, W>), dim3((n[0] + 63) / 64, (n[2] + 3) / 4), blk, lds, g_stream, o, w, n[0], n[2], n[1], reverse != 0);
    } else {
        DG_ALLOW_LDS((dg_accumulate_cols_kernel<2, O, W>), lds);
        hipLaunchKernelGGL((dg_accumulate_cols_kernel<2, O, W>), dim3((n[0] + 63) / 64, (n[1] + 3) / 4), blk, lds, g_stream, o, w, n[0], n[1], n[2], reverse != 0);
    }
    KERNEL_CHECK();
    return OCN_OK;
}

static int dg_reduce_operation(ocn_grid_t grid, const ocn_operand_t *operand, int kind, int dims_mask, int use_metric, int absolute,
                               const ocn_time_fold_t *fold, double *out) {
    if (int rc_ = refuse_immersed(grid, "a diagnostic (its reductions exclude immersed cells through a condition)")) return rc_;
    if (kind < OCN_REDUCE_SUM || kind > OCN_REDUCE_AVERAGE) return fail(OCN_EINVAL, "unknown reduction kind %d", kind);
    if (dims_mask < 1 || dims_mask > 7) return fail(OCN_EINVAL, "dims_mask %d: bits 0..2 name the reduced directions, at least one", dims_mask);
    if (use_metric && (kind == OCN_REDUCE_MAXIMUM || kind == OCN_REDUCE_MINIMUM)) return fail(OCN_EINVAL, "maximum and minimum take no metric");
    DgOperand o;
    int rc = dg_make_operand(grid, operand, &o);
    if (rc) return rc;
    o.absolute = absolute != 0;
    if (use_metric) dg_set_metric(grid->d, dims_mask, &o);
    int n[3];
    dg_interior_size(grid->d, operand->loc, n);
    return dg_with_out(dg_make_out(grid->d, operand->loc, dims_mask, out), fold,
                       [&](const auto &w) { return dg_reduce_kind(grid, o, kind, n, dims_mask, w, 0); });
}

extern "C" int ocn_reduce_operation(ocn_grid_t grid, const ocn_operand_t *operand, int kind, int dims_mask, int use_metric, int absolute,
                                    double *out) {
    NEED_INIT();
    if (!out) return fail(OCN_EINVAL, "NULL argument");
    return dg_reduce_operation(grid, operand, kind, dims_mask, use_metric, absolute, nullptr, out);
}

extern "C" int ocn_time_average_reduce_operation(ocn_grid_t grid, const ocn_operand_t *operand, int kind, int dims_mask, int use_metric,
                                                 int absolute, const ocn_time_fold_t *fold, double *result) {
    NEED_INIT();
    if (!result) return fail(OCN_EINVAL, "NULL argument");
    const int rc = dg_check_fold(fold);
    if (rc) return rc;
    return dg_reduce_operation(grid, operand, kind, dims_mask, use_metric, absolute, fold, result);
}

static int dg_accumulate_operation(ocn_grid_t grid, const ocn_operand_t *operand, int dim, int reverse, int use_metric,
                                   const ocn_time_fold_t *fold, double *out) {
    if (int rc_ = refuse_immersed(grid, "a diagnostic (its reductions exclude immersed cells through a condition)")) return rc_;
    if (dim < 0 || dim > 2) return fail(OCN_EINVAL, "dim %d: 0 (x), 1 (y) or 2 (z)", dim);
    DgOperand o;
    int rc = dg_make_operand(grid, operand, &o);
    if (rc) return rc;
    if (use_metric) dg_set_metric(grid->d, 1 << dim, &o);
    int n[3];
    dg_interior_size(grid->d, operand->loc, n);
    return dg_with_out(dg_make_out(grid->d, operand->loc, 0, out), fold, [&](const auto &w) { return dg_accumulate(o, n, dim, reverse, w, 0); });
}

extern "C" int ocn_accumulate_operation(ocn_grid_t grid, const ocn_operand_t *operand, int dim, int reverse, int use_metric, double *out) {
    NEED_INIT();
    if (!out) return fail(OCN_EINVAL, "NULL argument");
    return dg_accumulate_operation(grid, operand, dim, reverse, use_metric, nullptr, out);
}

extern "C" int ocn_time_average_accumulate_operation(ocn_grid_t grid, const ocn_operand_t *operand, int dim, int reverse, int use_metric,
                                                     const ocn_time_fold_t *fold, double *result) {
    NEED_INIT();
    if (!result) return fail(OCN_EINVAL, "NULL argument");
    const int rc = dg_check_fold(fold);
    if (rc) return rc;
    return dg_accumulate_operation(grid, operand, dim, reverse, use_metric, fold, result);
}

// ---------------------------------------------------------------------------------------------------------------------
// stencil programs (ocn_diagnostics.h): KernelFunctionOperation, Derivative, UnaryOperation as recorded programs
// ---------------------------------------------------------------------------------------------------------------------
// value operands of a stencil instruction (the leaves have none), -1 for what is no op of a stencil program
static int st_arity(int op) {
    if (op == OCN_EXPR_CONST || op == OCN_STENCIL_LOAD || op == OCN_STENCIL_SPACING || op == OCN_STENCIL_NODE) return 0;
    if (op < OCN_EXPR_ADD || op > OCN_EXPR_SELECT) return -1;          // COORD, TIME, FIELD, the planner's table load, anything else
    return expr_arity(op);
}

// what can be checked without a grid: every operand names an earlier value, every field the kernel or the lowering reads is in range
static int st_validate_program(const ocn_stencil_ins_t *program, int n, int nargs) {
    if (n < 1 || n > DG_ST_MAX_INS) return fail(OCN_EINVAL, "a stencil program has 1..%d instructions; got %d", DG_ST_MAX_INS, n);
    if (nargs < 0 || nargs > DG_ST_MAX_ARGS) return fail(OCN_EINVAL, "a stencil program has 0..%d field arguments; got %d", DG_ST_MAX_ARGS, nargs);
    if (!program) return fail(OCN_EINVAL, "NULL program");
    for (int q = 0; q < n; ++q) {
        const ocn_stencil_ins_t &I = program[q];
        const int values = st_arity(I.op);
        if (values < 0) return fail(OCN_EINVAL, "instruction %d: unknown op %d", q, I.op);
        const bool load = I.op == OCN_STENCIL_LOAD, line = I.op == OCN_STENCIL_SPACING || I.op == OCN_STENCIL_NODE;
        if (load && (I.a < 0 || I.a >= nargs)) return fail(OCN_EINVAL, "instruction %d: argument slot %d outside 0..%d", q, I.a, nargs - 1);
        if (line && (I.a < 0 || I.a > 2)) return fail(OCN_EINVAL, "instruction %d: direction %d is not 0 .. 2", q, I.a);
        if (line && I.b != OCN_CENTER && I.b != OCN_FACE) return fail(OCN_EINVAL, "instruction %d: location %d is not OCN_CENTER or OCN_FACE", q, I.b);
        const int operand[3] = {I.a, I.b, I.c}, off[3] = {I.di, I.dj, I.dk};
        for (int w = 0; w < 3; ++w) {
            if (w < values) {
                if (operand[w] < 0 || operand[w] >= q) return fail(OCN_EINVAL, "instruction %d: operand %d is not an earlier value", q, operand[w]);
            } else if (operand[w] != 0 && !((load && w == 0) || (line && w < 2)))
                return fail(OCN_EINVAL, "instruction %d: an unused operand field is not 0", q);
            if (off[w] != 0 && !(load || (line && w == I.a)))
                return fail(OCN_EINVAL, "instruction %d: an offset where the op takes none (d%c = %d)", q, "ijk"[w], off[w]);
        }
    }
    return OCN_OK;
}

// the slot of every value: a linear scan by last use. At instruction q the slots of the operands that are not used later are freed FIRST
// (the kernel reads the operands before it writes the result), then q takes the lowest free slot; a value nobody uses frees its slot at
// once; the last value is the result and stays. Returns the number of slots.
static int st_plan(const ocn_stencil_ins_t *program, int n, int *slot) {
    std::vector<int> last(n);
    for (int q = 0; q < n; ++q) {
        last[q] = q;
        const int operand[3] = {program[q].a, program[q].b, program[q].c};
        for (int w = 0; w < st_arity(program[q].op); ++w) last[operand[w]] = q;
    }
    last[n - 1] = n;
    std::vector<char> used(n + 1, 0);
    int nslots = 0;
    for (int q = 0; q < n; ++q) {
        const int operand[3] = {program[q].a, program[q].b, program[q].c};
        for (int w = 0; w < st_arity(program[q].op); ++w)
            if (last[operand[w]] == q) used[slot[operand[w]]] = 0;
        int s = 0;
        while (used[s]) ++s;
        slot[q] = s;
        used[s] = 1;
        nslots = std::max(nslots, s + 1);
        if (last[q] == q) used[s] = 0;
    }
    return nslots;
}

extern "C" int ocn_stencil_plan(const ocn_stencil_ins_t *program, int n, int nargs, int *slot_of_value, int *nslots) {
    const int rc = st_validate_program(program, n, nargs);
    if (rc) return rc;
    std::vector<int> slot(n);
    const int ns = st_plan(program, n, slot.data());
    if (slot_of_value) for (int q = 0; q < n; ++q) slot_of_value[q] = slot[q];
    if (nslots) *nslots = ns;
    if (ns > DG_ST_MAX_SLOTS)
        return fail(OCN_EINVAL, "the program keeps %d values alive at once: the limit of a stencil program is %d live values (LDS slots)", ns, DG_ST_MAX_SLOTS);
    return OCN_OK;
}

struct StLowered { int n, nslots; bool arith; };

// validate the operand against the grid, lower its program (slots for values, pointers for leaves) and queue the copy into the grid's
// program block: nothing the kernel indexes with is left unchecked
static int dg_lower_stencil(ocn_grid_s *grid, const ocn_stencil_operand_t *op, StLowered *S) {
    if (!grid || !op) return fail(OCN_EINVAL, "NULL argument");
    const DGrid &g = grid->d;
    int rc = no_connected_topology(g, "diagnostics");
    if (rc) return rc;
    if ((rc = st_validate_program(op->program, op->n, op->nargs))) return rc;
    if (op->nargs > 0 && (!op->args || !op->arg_locs)) return fail(OCN_EINVAL, "NULL arguments");
    for (int d = 0; d < 3; ++d)
        if (op->loc[d] != OCN_CENTER && op->loc[d] != OCN_FACE) return fail(OCN_EINVAL, "loc[%d] is OCN_CENTER or OCN_FACE", d);
    for (int s = 0; s < op->nargs; ++s) {
        if (!op->args[s]) return fail(OCN_EINVAL, "argument %d is NULL", s);
        for (int d = 0; d < 3; ++d)
            if (op->arg_locs[3 * s + d] != OCN_CENTER && op->arg_locs[3 * s + d] != OCN_FACE)
                return fail(OCN_EINVAL, "argument %d: loc[%d] is OCN_CENTER or OCN_FACE", s, d);
    }
    const int n = op->n;
    std::vector<int> slot(n);
    S->n = n;
    S->nslots = st_plan(op->program, n, slot.data());
    S->arith = true;
    if (S->nslots > DG_ST_MAX_SLOTS)
        return fail(OCN_EINVAL, "the program keeps %d values alive at once: the limit of a stencil program is %d live values (LDS slots)", S->nslots,
                    DG_ST_MAX_SLOTS);
    const int N[3] = {g.Nx, g.Ny, g.Nz}, H[3] = {g.Hx, g.Hy, g.Hz}, T[3] = {g.tx, g.ty, g.tz};
    int nout[3];
    dg_interior_size(g, op->loc, nout);
    std::vector<DgStIns> low(n);
    for (int q = 0; q < n; ++q) {
        const ocn_stencil_ins_t &I = op->program[q];
        const int off[3] = {I.di, I.dj, I.dk};
        DgStIns &L = low[q];
        L = DgStIns{};
        L.dst = slot[q];
        if (I.op == OCN_EXPR_CONST) {
            L.op = OCN_EXPR_CONST;
            L.imm = I.imm;
        } else if (I.op == OCN_STENCIL_LOAD) {
            const int *from = op->arg_locs + 3 * I.a;
            int narg[3], P[3];
            dg_interior_size(g, from, narg);
            parent_size(g, from, P);
            for (int d = 0; d < 3; ++d) {
                if (T[d] == OCN_FLAT) {
                    if (off[d] != 0) return fail(OCN_EINVAL, "instruction %d: argument %d is read at offset %+d along %c, which is Flat", q, I.a, off[d], "xyz"[d]);
                    continue;
                }
                // parent index H + i + off, i = 0 .. nout - 1, inside 0 .. narg + 2 H - 1
                const int need = std::max(-off[d], nout[d] + off[d] - narg[d]);
                if (need > H[d])
                    return fail(OCN_EINVAL, "instruction %d: argument %d read at offset %+d along %c (%d output points, %d of the argument) needs a halo of %d; "
                                "the grid has %d", q, I.a, off[d], "xyz"[d], nout[d], narg[d], need, H[d]);
            }
            const long st1 = P[0], st2 = (long)P[0] * P[1];
            L.op = DG_ST_LOAD;
            L.s1 = P[0];
            L.s2 = st2;
            L.p = op->args[I.a] + ((H[0] + off[0]) + st1 * (H[1] + off[1]) + st2 * (H[2] + off[2]));
        } else if (I.op == OCN_STENCIL_SPACING) {
            const int d = I.a;
            if (d < 2 || T[2] == OCN_FLAT) {                              // x and y are regular (Δᶜ = Δᶠ); a Flat direction has Δ = 1
                if (T[d] == OCN_FLAT && off[d] != 0) return fail(OCN_EINVAL, "instruction %d: a spacing at offset %+d along %c, which is Flat", q, off[d], "xyz"[d]);
                L.op = OCN_EXPR_CONST;
                L.imm = d == 0 ? g.dx : (d == 1 ? g.dy : 1.0);
            } else {                                                      // tables of Nz + 2 Hz + 1 levels, level k (1-based) at k - 1 + Hz
                const int need = std::max(-off[2], nout[2] + off[2] - (N[2] + 1));
                if (need > H[2])
                    return fail(OCN_EINVAL, "instruction %d: Δz read at offset %+d along z (%d output points) needs a halo of %d; the grid has %d", q, off[2],
                                nout[2], need, H[2]);
                L.op = DG_ST_LINE;
                L.c = 2;
                L.p = (I.b == OCN_FACE ? g.dzf : g.dzc) + (H[2] + off[2]);
            }
        } else if (I.op == OCN_STENCIL_NODE) {
            const int d = I.a;
            if (!grid->node_tables) return fail(OCN_ESTATE, "the grid has no node tables: call ocn_grid_set_node_tables");
            const int len = T[d] == OCN_FLAT ? 1 : N[d] + (I.b == OCN_FACE ? 1 : 0);          // nodes of interior points only
            if (off[d] < 0 || nout[d] + off[d] > len)
                return fail(OCN_EINVAL, "instruction %d: the %c node at offset %+d (%d output points) lies outside the %d interior nodes of the table", q,
                            "xyz"[d], off[d], nout[d], len);
            L.op = DG_ST_LINE;
            L.c = d;
            L.p = (I.b == OCN_FACE ? grid->nodes_f[d] : grid->nodes_c[d]) + off[d];
        } else {
            L.op = I.op;
            const int values = st_arity(I.op);
            L.a = slot[I.a];
            if (values > 1) L.b = slot[I.b];
            if (values > 2) L.c = slot[I.c];
            if (I.op >= OCN_EXPR_EXP && I.op <= OCN_EXPR_POW) S->arith = false;
        }
    }
    // the program the device block already holds (a diagnostic computed again): nothing to transfer
    static_assert(sizeof(DgStIns) == 48, "no padding: the comparison below is of whole instructions");
    std::vector<DgStIns> &held = grid->diag_program_h;
    if (grid->diag_program && held.size() == low.size() && memcmp(held.data(), low.data(), sizeof(DgStIns) * (size_t)n) == 0) return OCN_OK;
    if (!grid->diag_program) HIP_TRY(dev_alloc((void **)&grid->diag_program, sizeof(DgStIns) * DG_ST_MAX_INS));
    // the host copy belongs to the grid and outlives this call; the transfer queued by an earlier call must have read it before it changes
    if (grid->diag_program_copied) HIP_TRY(hipEventSynchronize(grid->diag_program_copied));
    else HIP_TRY(hipEventCreateWithFlags(&grid->diag_program_copied, hipEventDisableTiming));
    held = low;
    // stream-ordered after the launch that read the previous program
    hipError_t e = hipMemcpyAsync(grid->diag_program, held.data(), sizeof(DgStIns) * (size_t)n, hipMemcpyHostToDevice, g_stream);
    if (e == hipSuccess) e = hipEventRecord(grid->diag_program_copied, g_stream);
    if (e != hipSuccess) { held.clear(); return fail((int)e, "stencil program transfer: %s", hipGetErrorString(e)); }
    return OCN_OK;
}

template <bool ARITH>
static DgStencil<ARITH> dg_stencil_operand(const ocn_grid_s *grid, const ocn_stencil_operand_t *op, const StLowered &S) {
    DgStencil<ARITH> o = {};
    o.ins = grid->diag_program;
    o.n = S.n;
    o.dz = op->loc[2] == OCN_FACE ? grid->d.dzf : grid->d.dzc;
    o.Hz = grid->d.Hz;
    return o;
}
template <class O> static void dg_set_metric_of(const DGrid &g, int mask, O *o) {
    DgOperand m = {};
    dg_set_metric(g, mask, &m);
    o->mc = m.mc;
    o->mmode = m.mmode;
}
// DG_ST_MIN_LDS_SLOTS (an A/B build, OCN_EXTRA_FLAGS): ask for at least that many slots of LDS, to time a program at the occupancy a
// larger one would have -- 32 slots are two blocks per CU, 64 one
#ifndef DG_ST_MIN_LDS_SLOTS
#define DG_ST_MIN_LDS_SLOTS 0
#endif
static size_t st_lds_bytes(const StLowered &S) { return sizeof(double) * DG_THREADS * (size_t)std::max(S.nslots, DG_ST_MIN_LDS_SLOTS); }

static int st_compute(ocn_grid_t grid, const ocn_stencil_operand_t *operand, const ocn_time_fold_t *fold, double *out) {
    if (int rc_ = refuse_immersed(grid, "a diagnostic (its reductions exclude immersed cells through a condition)")) return rc_;
    StLowered S;
    const int rc = dg_lower_stencil(grid, operand, &S);
    if (rc) return rc;
    int n[3];
    dg_interior_size(grid->d, operand->loc, n);
    return dg_with_out(dg_make_out(grid->d, operand->loc, 0, out), fold, [&](const auto &w) {
        return S.arith ? dg_compute(grid, dg_stencil_operand<true>(grid, operand, S), n, w, st_lds_bytes(S))
                       : dg_compute(grid, dg_stencil_operand<false>(grid, operand, S), n, w, st_lds_bytes(S));
    });
}

extern "C" int ocn_compute_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, double *out) {
    NEED_INIT();
    if (!out) return fail(OCN_EINVAL, "NULL argument");
    return st_compute(grid, operand, nullptr, out);
}

// a stencil operand has no whole-parent form: a program that is one LOAD of a field is folded over the interior like any other
extern "C" int ocn_time_average_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, const ocn_time_fold_t *fold, double *result) {
    NEED_INIT();
    if (!result) return fail(OCN_EINVAL, "NULL argument");
    const int rc = dg_check_fold(fold);
    if (rc) return rc;
    return st_compute(grid, operand, fold, result);
}

template <bool ARITH>
static int st_reduce(ocn_grid_s *grid, const ocn_stencil_operand_t *operand, const StLowered &S, int kind, int dims_mask, int use_metric,
                     int absolute, const ocn_time_fold_t *fold, double *out) {
    DgStencil<ARITH> o = dg_stencil_operand<ARITH>(grid, operand, S);
    o.absolute = absolute != 0;
    if (use_metric) dg_set_metric_of(grid->d, dims_mask, &o);
    int n[3];
    dg_interior_size(grid->d, operand->loc, n);
    return dg_with_out(dg_make_out(grid->d, operand->loc, dims_mask, out), fold,
                       [&](const auto &w) { return dg_reduce_kind(grid, o, kind, n, dims_mask, w, st_lds_bytes(S)); });
}

static int st_reduce_any(ocn_grid_t grid, const ocn_stencil_operand_t *operand, int kind, int dims_mask, int use_metric, int absolute,
                         const ocn_time_fold_t *fold, double *out) {
    if (int rc_ = refuse_immersed(grid, "a diagnostic (its reductions exclude immersed cells through a condition)")) return rc_;
    if (kind < OCN_REDUCE_SUM || kind > OCN_REDUCE_AVERAGE) return fail(OCN_EINVAL, "unknown reduction kind %d", kind);
    if (dims_mask < 1 || dims_mask > 7) return fail(OCN_EINVAL, "dims_mask %d: bits 0..2 name the reduced directions, at least one", dims_mask);
    if (use_metric && (kind == OCN_REDUCE_MAXIMUM || kind == OCN_REDUCE_MINIMUM)) return fail(OCN_EINVAL, "maximum and minimum take no metric");
    StLowered S;
    const int rc = dg_lower_stencil(grid, operand, &S);
    if (rc) return rc;
    return S.arith ? st_reduce<true>(grid, operand, S, kind, dims_mask, use_metric, absolute, fold, out)
                   : st_reduce<false>(grid, operand, S, kind, dims_mask, use_metric, absolute, fold, out);
}

extern "C" int ocn_reduce_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, int kind, int dims_mask, int use_metric, int absolute,
                                  double *out) {
    NEED_INIT();
    if (!out) return fail(OCN_EINVAL, "NULL argument");
    return st_reduce_any(grid, operand, kind, dims_mask, use_metric, absolute, nullptr, out);
}

extern "C" int ocn_time_average_reduce_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, int kind, int dims_mask, int use_metric,
                                               int absolute, const ocn_time_fold_t *fold, double *result) {
    NEED_INIT();
    if (!result) return fail(OCN_EINVAL, "NULL argument");
    const int rc = dg_check_fold(fold);
    if (rc) return rc;
    return st_reduce_any(grid, operand, kind, dims_mask, use_metric, absolute, fold, result);
}

template <bool ARITH>
static int st_accumulate(ocn_grid_s *grid, const ocn_stencil_operand_t *operand, const StLowered &S, int dim, int reverse, int use_metric,
                         const ocn_time_fold_t *fold, double *out) {
    DgStencil<ARITH> o = dg_stencil_operand<ARITH>(grid, operand, S);
    if (use_metric) dg_set_metric_of(grid->d, 1 << dim, &o);
    int n[3];
    dg_interior_size(grid->d, operand->loc, n);
    return dg_with_out(dg_make_out(grid->d, operand->loc, 0, out), fold,
                       [&](const auto &w) { return dg_accumulate(o, n, dim, reverse, w, st_lds_bytes(S)); });
}

static int st_accumulate_any(ocn_grid_t grid, const ocn_stencil_operand_t *operand, int dim, int reverse, int use_metric,
                             const ocn_time_fold_t *fold, double *out) {
    if (int rc_ = refuse_immersed(grid, "a diagnostic (its reductions exclude immersed cells through a condition)")) return rc_;
    if (dim < 0 || dim > 2) return fail(OCN_EINVAL, "dim %d: 0 (x), 1 (y) or 2 (z)", dim);
    StLowered S;
    const int rc = dg_lower_stencil(grid, operand, &S);
    if (rc) return rc;
    return S.arith ? st_accumulate<true>(grid, operand, S, dim, reverse, use_metric, fold, out)
                   : st_accumulate<false>(grid, operand, S, dim, reverse, use_metric, fold, out);
}

extern "C" int ocn_accumulate_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, int dim, int reverse, int use_metric, double *out) {
    NEED_INIT();
    if (!out) return fail(OCN_EINVAL, "NULL argument");
    return st_accumulate_any(grid, operand, dim, reverse, use_metric, nullptr, out);
}

extern "C" int ocn_time_average_accumulate_stencil(ocn_grid_t grid, const ocn_stencil_operand_t *operand, int dim, int reverse, int use_metric,
                                                   const ocn_time_fold_t *fold, double *result) {
    NEED_INIT();
    if (!result) return fail(OCN_EINVAL, "NULL argument");
    const int rc = dg_check_fold(fold);
    if (rc) return rc;
    return st_accumulate_any(grid, operand, dim, reverse, use_metric, fold, result);
}

static int update_hydrostatic_pressure(const DGrid &g, int kind, const double *bT, const double *S, double grav, double alpha, double beta,
                                       double *pHY, bool tilted = false, double ghat_z = 1.0) {
    if (g.tz == OCN_FLAT) return OCN_OK;                   // update_hydrostatic_pressure!(::ZFlatGrid) = nothing
    const int i0 = g.tx == OCN_FLAT ? 1 : 0, i1 = g.tx == OCN_FLAT ? g.Nx : g.Nx + 1;
    const int j0 = g.ty == OCN_FLAT ? 1 : 0, j1 = g.ty == OCN_FLAT ? g.Ny : g.Ny + 1;
    const BuoyancyArgs B{kind, bT, S, grav, alpha, beta};
    const dim3 blk(64, 4, 1);
    const dim3 grd((i1 - i0 + 64) / 64, (j1 - j0 + 4) / 4);
    if (tilted) {
        TiltedBuoyancyArgs Bt;
        static_cast<BuoyancyArgs &>(Bt) = B;
        Bt.ghat_z = ghat_z;
        if (kind == 1) hipLaunchKernelGGL((hydrostatic_pressure_kernel<1, true>), grd, blk, 0, g_stream, g, make_view(g, bT, LOC_C), Bt, pHY, i0, i1, j0, j1);
        else           hipLaunchKernelGGL((hydrostatic_pressure_kernel<2, true>), grd, blk, 0, g_stream, g, make_view(g, bT, LOC_C), Bt, pHY, i0, i1, j0, j1);
    } else
    if (kind == 1) hipLaunchKernelGGL(hydrostatic_pressure_kernel<1>, grd, blk, 0, g_stream, g, make_view(g, bT, LOC_C), B, pHY, i0, i1, j0, j1);
    else           hipLaunchKernelGGL(hydrostatic_pressure_kernel<2>, grd, blk, 0, g_stream, g, make_view(g, bT, LOC_C), B, pHY, i0, i1, j0, j1);
    KERNEL_CHECK();
    return OCN_OK;
}

static int add_hydrostatic_pressure_gradient(const DGrid &g, const double *pHY, double *Gu, double *Gv, const int *range) {
    Range6 ru, rv;
    int rc;
    if ((rc = check_range(g, range, &ru, LOC_U, true)) || (rc = check_range(g, range, &rv, LOC_V, true))) return rc;
    hipLaunchKernelGGL(hydrostatic_gradient_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, make_view(g, pHY, LOC_C),
                       make_view(g, Gu, LOC_U), make_view(g, Gv, LOC_V), ru, rv);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_update_hydrostatic_pressure(ocn_grid_t grid, int kind, const double *bT, const double *S, double grav, double alpha,
                                               double beta, double *pHY) {
    NEED_INIT();
    if (!grid || !bT || !pHY || (kind != 1 && kind != 2) || (kind == 2 && !S)) return fail(OCN_EINVAL, "invalid argument");
    return update_hydrostatic_pressure(grid->d, kind, bT, S, grav, alpha, beta, pHY);
}

extern "C" int ocn_update_hydrostatic_pressure_tilted(ocn_grid_t grid, int kind, const double *bT, const double *S, double grav, double alpha,
                                                      double beta, double ghat_z, double *pHY) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "BuoyancyForce(gravity_unit_vector)")) return rc_;
    if (!grid || !bT || !pHY || (kind != 1 && kind != 2) || (kind == 2 && !S)) return fail(OCN_EINVAL, "invalid argument");
    return update_hydrostatic_pressure(grid->d, kind, bT, S, grav, alpha, beta, pHY, true, ghat_z);
}

extern "C" int ocn_add_hydrostatic_pressure_gradient(ocn_grid_t grid, const double *pHY, double *Gu, double *Gv, const int *range) {
    NEED_INIT();
    if (!grid || !pHY || !Gu || !Gv) return fail(OCN_EINVAL, "NULL argument");
    return add_hydrostatic_pressure_gradient(grid->d, pHY, Gu, Gv, range);
}

static int add_fplane_coriolis(const DGrid &g, double f, const double *u, const double *v, double *Gu, double *Gv, const int *range,
                               const ImmView *im = nullptr) {
    Range6 ru, rv;
    int rc;
    if ((rc = check_range(g, range, &ru, LOC_U, true)) || (rc = check_range(g, range, &rv, LOC_V, true))) return rc;
    if (im) hipLaunchKernelGGL(immersed_fplane_coriolis_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, *im, f, make_view(g, u, LOC_U),
                               make_view(g, v, LOC_V), make_view(g, Gu, LOC_U), make_view(g, Gv, LOC_V), ru, rv);
    else
    hipLaunchKernelGGL(fplane_coriolis_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, f, make_view(g, u, LOC_U),
                       make_view(g, v, LOC_V), make_view(g, Gu, LOC_U), make_view(g, Gv, LOC_V), ru, rv);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_add_fplane_coriolis(ocn_grid_t grid, double f, const double *u, const double *v, double *Gu, double *Gv, const int *range) {
    NEED_INIT();
    if (!grid || !u || !v || !Gu || !Gv) return fail(OCN_EINVAL, "NULL argument");
    const ImmView im = imm_view(grid);
    return add_fplane_coriolis(grid->d, f, u, v, Gu, Gv, range, is_immersed(grid) ? &im : nullptr);
}

// coriolis = ConstantCartesianCoriolis(fx, fy, fz): G_u -= x_f_cross_U, G_v -= y_f_cross_U, G_w -= z_f_cross_U (cartesian_coriolis_kernel)
static int add_cartesian_coriolis(const DGrid &g, double fx, double fy, double fz, const double *u, const double *v, const double *w, double *Gu,
                                  double *Gv, double *Gw, const int *range) {
    Range6 ru, rv, rw;
    int rc;
    if ((rc = check_range(g, range, &ru, LOC_U, true)) || (rc = check_range(g, range, &rv, LOC_V, true)) || (rc = check_range(g, range, &rw, LOC_W, true)))
        return rc;
    hipLaunchKernelGGL(cartesian_coriolis_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, fx, fy, fz, make_view(g, u, LOC_U),
                       make_view(g, v, LOC_V), make_view(g, w, LOC_W), make_view(g, Gu, LOC_U), make_view(g, Gv, LOC_V), make_view(g, Gw, LOC_W),
                       ru, rv, rw);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_add_cartesian_coriolis(ocn_grid_t grid, double fx, double fy, double fz, const double *u, const double *v, const double *w,
                                          double *Gu, double *Gv, double *Gw, const int *range) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "ConstantCartesianCoriolis")) return rc_;
    if (!grid || !u || !v || !w || !Gu || !Gv || !Gw) return fail(OCN_EINVAL, "NULL argument");
    return add_cartesian_coriolis(grid->d, fx, fy, fz, u, v, w, Gu, Gv, Gw, range);
}

// stokes_drift = UniformStokesDrift: G_u += x_curl_Uˢ_cross_U + ∂t_uˢ, G_v += y_curl_Uˢ_cross_U + ∂t_vˢ, G_w += z_curl_Uˢ_cross_U
// (stokes_drift_kernel); `sd`: device tables, a null one is a table of zeros; each velocity over its own range
static int add_stokes_drift(const DGrid &g, const StokesTables &sd, const double *u, const double *v, const double *w, double *Gu, double *Gv,
                            double *Gw, const int *range_u, const int *range_v, const int *range_w) {
    Range6 ru, rv, rw;
    int rc;
    // the averages read one cell beyond a range in every direction that is not Flat
    if ((g.tx != OCN_FLAT && g.Hx < 1) || (g.ty != OCN_FLAT && g.Hy < 1) || (g.tz != OCN_FLAT && g.Hz < 1))
        return fail(OCN_EINVAL, "the Stokes-drift terms need a halo of at least 1 in every direction that is not Flat");
    if ((rc = check_range(g, range_u, &ru, LOC_U, true)) || (rc = check_range(g, range_v, &rv, LOC_V, true)) ||
        (rc = check_range(g, range_w, &rw, LOC_W, true)))
        return rc;
    hipLaunchKernelGGL(stokes_drift_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, sd, make_view(g, u, LOC_U), make_view(g, v, LOC_V),
                       make_view(g, w, LOC_W), make_view(g, Gu, LOC_U), make_view(g, Gv, LOC_V), make_view(g, Gw, LOC_W), ru, rv, rw);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_add_stokes_drift(ocn_grid_t grid, const double *dzu_c, const double *dzu_f, const double *dzv_c, const double *dzv_f,
                                    const double *dtu_c, const double *dtv_c, const double *u, const double *v, const double *w, double *Gu,
                                    double *Gv, double *Gw, const int *range_u, const int *range_v, const int *range_w) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "stokes_drift")) return rc_;
    if (!grid || !u || !v || !w || !Gu || !Gv || !Gw) return fail(OCN_EINVAL, "NULL argument");
    return add_stokes_drift(grid->d, StokesTables{dzu_c, dzu_f, dzv_c, dzv_f, dtu_c, dtv_c}, u, v, w, Gu, Gv, Gw, range_u, range_v, range_w);
}

// particles: one launch of particle_step_kernel (ocn_particles.h), one thread per particle, 256 per block
static int launch_particles(const PGeom &pg, const ParticleStepArgs &a) {
    if (a.n <= 0) return OCN_OK;
    hipLaunchKernelGGL(particle_step_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, g_stream, pg, a);
    KERNEL_CHECK();
    return OCN_OK;
}
static int loc_bits(const int loc[3]) { return (loc[0] == OCN_FACE ? 1 : 0) | (loc[1] == OCN_FACE ? 2 : 0) | (loc[2] == OCN_FACE ? 4 : 0); }

// interpolate(X, field, (ℓx, ℓy, ℓz), grid) (Fields/interpolate.jl:272-282) at n points; everything a DEVICE pointer
extern "C" int ocn_interpolate_at(ocn_grid_t grid, int n, const double *x, const double *y, const double *z, const double *field,
                                  const int loc[3], double *out) {
    NEED_INIT();
    if (!grid || !x || !y || !z || !field || !loc || !out) return fail(OCN_EINVAL, "NULL argument");
    if (n < 0) return fail(OCN_EINVAL, "n must not be negative");
    if (!grid->has_nodes) return fail(OCN_ESTATE, "the grid has no node coordinates: call ocn_grid_set_nodes");
    for (int d = 0; d < 3; ++d)
        if (loc[d] != OCN_CENTER && loc[d] != OCN_FACE) return fail(OCN_EINVAL, "loc[%d] must be OCN_CENTER or OCN_FACE", d);
    ParticleStepArgs a = {};
    a.n = n;
    a.x = const_cast<double *>(x); a.y = const_cast<double *>(y); a.z = const_cast<double *>(z);        // advect = 0: read only
    a.ntracked = 1;
    a.tracked[0] = TrackedField{make_view(grid->d, field, loc), loc_bits(loc), out};
    return launch_particles(grid->pg, a);
}

// advect_lagrangian_particles! (lagrangian_particle_advection.jl:195-223; drogued_dynamics.jl:45-72 with depths): x, y, z move in place
// with velocities u, v, w (filled halos); with depths the velocities are taken at (x, y, depths[p]) and z stays
extern "C" int ocn_advect_particles(ocn_grid_t grid, int n, double *x, double *y, double *z, const double *depths, double restitution,
                                    double dt, const double *u, const double *v, const double *w) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "particles (LagrangianParticles)")) return rc_;
    if (!grid || !x || !y || !z || !u || !v || !w) return fail(OCN_EINVAL, "NULL argument");
    if (n < 0) return fail(OCN_EINVAL, "n must not be negative");
    if (!grid->has_nodes) return fail(OCN_ESTATE, "the grid has no node coordinates: call ocn_grid_set_nodes");
    ParticleStepArgs a = {};
    a.n = n; a.x = x; a.y = y; a.z = z; a.depths = depths; a.restitution = restitution; a.dt = dt; a.advect = 1;
    a.u = make_view(grid->d, u, LOC_U); a.v = make_view(grid->d, v, LOC_V); a.w = make_view(grid->d, w, LOC_W);
    return launch_particles(grid->pg, a);
}

// The index computation of the particle kernel on the HOST (the same function, particle_interpolator): no device, no ocn_init. For n
// coordinates along direction `dir` of a direction with N cells, halo H and topology `topo`, at a Face (face != 0) or a Center: idx[2 p],
// idx[2 p + 1] = the clamped corner indices i⁻, i⁺ and w[p] = ξ. first_node: the first node at that location; spacing: Δ; nodes: the node
// table of a stretched direction (N + 1 faces or N centres) or NULL.
extern "C" int ocn_particle_indices_host(int N, int H, int topo, int face, double first_node, double spacing, const double *nodes, int n,
                                         const double *coordinate, int *idx, double *w) {
    if (!coordinate || !idx || !w || n < 0 || N < 1 || H < 0) return fail(OCN_EINVAL, "invalid argument");
    PGeom pg = {};
    pg.N[2] = N; pg.H[2] = H; pg.T[2] = topo; pg.f0[2] = pg.c0[2] = first_node; pg.d[2] = spacing;
    pg.zf = pg.zc = nodes;
    for (int p = 0; p < n; ++p) {
        const PInterp r = particle_interpolator(pg, 2, face != 0, coordinate[p]);
        idx[2 * p] = r.lo; idx[2 * p + 1] = r.hi; w[p] = r.w;
    }
    return OCN_OK;
}

// buoyancy = BuoyancyForce(formulation; gravity_unit_vector): G_u += x_dot_g_b, G_v += y_dot_g_b (buoyancy_acceleration_kernel)
static int add_buoyancy_acceleration(const DGrid &g, int kind, const double *bT, const double *S, double grav, double alpha, double beta,
                                     double ghat_x, double ghat_y, double *Gu, double *Gv, const int *range) {
    Range6 ru, rv;
    int rc;
    if ((rc = check_range(g, range, &ru, LOC_U, true)) || (rc = check_range(g, range, &rv, LOC_V, true))) return rc;
    const BuoyancyArgs B{kind, bT, S, grav, alpha, beta};
    if (kind == 1)
        hipLaunchKernelGGL(buoyancy_acceleration_kernel<1>, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, make_view(g, bT, LOC_C), B, ghat_x,
                           ghat_y, make_view(g, Gu, LOC_U), make_view(g, Gv, LOC_V), ru, rv);
    else
        hipLaunchKernelGGL(buoyancy_acceleration_kernel<2>, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, make_view(g, bT, LOC_C), B, ghat_x,
                           ghat_y, make_view(g, Gu, LOC_U), make_view(g, Gv, LOC_V), ru, rv);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_add_buoyancy_acceleration(ocn_grid_t grid, int kind, const double *bT, const double *S, double grav, double alpha, double beta,
                                             double ghat_x, double ghat_y, double *Gu, double *Gv, const int *range) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "BuoyancyForce(gravity_unit_vector)")) return rc_;
    if (!grid || !bT || !Gu || !Gv || (kind != 1 && kind != 2) || (kind == 2 && !S)) return fail(OCN_EINVAL, "invalid argument");
    return add_buoyancy_acceleration(grid->d, kind, bT, S, grav, alpha, beta, ghat_x, ghat_y, Gu, Gv, range);
}

// ---- closures: ScalarDiffusivity, AnisotropicMinimumDissipation, Smagorinsky (kernels: ocn_closures.h) ----
// fn(std::integral_constant<int, F>()) for the run-time field kind F: the kernels take it as a template argument
template <class Fn> static void with_field(int F, Fn fn) {
    switch (F) {
        case F_U: fn(std::integral_constant<int, F_U>()); break;
        case F_V: fn(std::integral_constant<int, F_V>()); break;
        case F_W: fn(std::integral_constant<int, F_W>()); break;
        default: fn(std::integral_constant<int, F_C>()); break;
    }
}

// what the eddy-coefficient closures refuse; `arrays`: the caller is an entry point that takes their coefficient arrays
static int refuse_flat(const DGrid &g, const char *feature, int code = OCN_ENOTSUP, bool arrays = false) {
    if (g.tx != OCN_FLAT && g.ty != OCN_FLAT && g.tz != OCN_FLAT) return OCN_OK;
    return arrays ? fail(code, "eddy-coefficient arrays (%s) need a grid without Flat directions", feature)
                  : fail(code, "%s needs a grid without Flat directions", feature);
}

// the arguments the four ocn_compute_closure_tendencies* entry points share. per_tracer: the argument with one entry per tracer (κ, κₑ or Pr)
static int check_closure_arguments(ocn_grid_t grid, const double *u, const double *v, const double *w, const double *const *tracers, int ntracers,
                                   const void *per_tracer, const double *Gu, const double *Gv, const double *Gw, double *const *Gc,
                                   bool nu_e_missing = false) {
    if (!grid || !u || !v || !w || nu_e_missing || !Gu || !Gv || !Gw || ntracers < 0 || ntracers > OCN_MAX_FIELDS - 3 ||
        (ntracers > 0 && (!tracers || !Gc || !per_tracer)))
        return fail(OCN_EINVAL, "invalid argument");
    return OCN_OK;
}

static int closure_tendencies(const DGrid &g, const double *u, const double *v, const double *w, const double *const *tr, int ntr,
                              double nu, const double *kappa, double *Gu, double *Gv, double *Gw, double *const *Gc, const int *range,
                              const double *nu_e = nullptr, const double *const *kappa_e = nullptr, const double *Pr = nullptr, bool vi = false,
                              const ImmView *im = nullptr) {
    if (im && (nu_e || kappa_e || Pr || vi)) return fail(OCN_ENOTSUP, "eddy-viscosity closures and VerticallyImplicitTimeDiscretization are not served on an ImmersedBoundaryGrid");
    // Pr (Smagorinsky): kappa_e[t] is νₑ and tracer t's coefficient is the interpolated νₑ divided by Pr[t]; Pr[t] == 1 takes the
    // plain instantiation (x / 1.0 is x)
    const FView vu = make_view(g, u, LOC_U), vv = make_view(g, v, LOC_V), vw = make_view(g, w, LOC_W);
    auto launch = [&](int F, const double *c, double *G, const int loc[3], double coef, const double *K, bool prd = false) -> int {
        if (coef == 0.0 && !K) return OCN_OK;
        const bool var = K != nullptr;
        const FView vK = make_view(g, K ? K : u, LOC_C);
        Range6 r;
        int rc = check_range(g, range, &r, loc, F != F_C);
        if (rc) return rc;
        const int nx = r.i1 - r.i0 + 1, ny = r.j1 - r.j0 + 1, nz = r.k1 - r.k0 + 1;
        if (nx <= 0 || ny <= 0 || nz <= 0) return OCN_OK;
        const FView vc = make_view(g, c ? c : u, LOC_C), vG = make_view(g, G, loc);
        const dim3 grd = grid3(nx, ny, nz, BLK);
        with_field(F, [&](auto field) {
            constexpr int FF = decltype(field)::value;
            if (im)             // constant coefficients, explicit, every flux conditional
                hipLaunchKernelGGL((closure_tendency_kernel<FF, false, ImmView>), grd, BLK, 0, g_stream, g, vu, vv, vw, vc, vG, coef, r, false, vK, *im);
            else if (vi)        // constant coefficients, the explicit part of a vertically implicit discretisation
                hipLaunchKernelGGL((closure_tendency_kernel<FF, true>), grd, BLK, 0, g_stream, g, vu, vv, vw, vc, vG, coef, r, false, vK, NoImm());
            else if (prd)       // (tracers only)
                hipLaunchKernelGGL(closure_tendency_prandtl_kernel, grd, BLK, 0, g_stream, g, vu, vv, vw, vc, vG, coef, r, vK);
            else
                hipLaunchKernelGGL((closure_tendency_kernel<FF>), grd, BLK, 0, g_stream, g, vu, vv, vw, vc, vG, coef, r, var, vK, NoImm());
        });
        return OCN_OK;
    };
    int rc;
    if ((rc = launch(F_U, nullptr, Gu, LOC_U, nu, nu_e)) || (rc = launch(F_V, nullptr, Gv, LOC_V, nu, nu_e)) ||
        (rc = launch(F_W, nullptr, Gw, LOC_W, nu, nu_e)))
        return rc;
    for (int t = 0; t < ntr; ++t)
        if ((rc = Pr ? launch(F_C, tr[t], Gc[t], LOC_C, Pr[t], nu_e, Pr[t] != 1.0)
                     : launch(F_C, tr[t], Gc[t], LOC_C, kappa ? kappa[t] : 0.0, kappa_e ? kappa_e[t] : nullptr))) return rc;
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_compute_closure_tendencies(ocn_grid_t grid, const double *u, const double *v, const double *w,
                                              const double *const *tracers, int ntracers, double nu, const double *kappa,
                                              double *Gu, double *Gv, double *Gw, double *const *Gc, const int *range) {
    NEED_INIT();
    if (int rc = check_closure_arguments(grid, u, v, w, tracers, ntracers, kappa, Gu, Gv, Gw, Gc)) return rc;
    if (nu < 0) return fail(OCN_EINVAL, "viscosity must be non-negative");
    const ImmView im = imm_view(grid);
    return closure_tendencies(grid->d, u, v, w, tracers, ntracers, nu, kappa, Gu, Gv, Gw, Gc, range, nullptr, nullptr, nullptr, false,
                              is_immersed(grid) ? &im : nullptr);
}

// the same with the z fluxes of ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν, κ) on a vertically Bounded grid
// (abstract_scalar_diffusivity_closure.jl:245-291): explicit at the z-flux indices 1 and Nz + 1, -(ν ∂x w), -(ν ∂y w), 0, 0 elsewhere
extern "C" int ocn_compute_closure_tendencies_vertically_implicit(ocn_grid_t grid, const double *u, const double *v, const double *w,
                                                                  const double *const *tracers, int ntracers, double nu, const double *kappa,
                                                                  double *Gu, double *Gv, double *Gw, double *const *Gc, const int *range) {
    NEED_INIT();
    if (int rc = check_closure_arguments(grid, u, v, w, tracers, ntracers, kappa, Gu, Gv, Gw, Gc)) return rc;
    if (nu < 0) return fail(OCN_EINVAL, "viscosity must be non-negative");
    if (grid->d.tz != OCN_BOUNDED)
        return fail(OCN_EINVAL, "VerticallyImplicitTimeDiscretization can only be specified on grids that are Bounded in the z-direction.");
    if (int rc = refuse_immersed(grid, "VerticallyImplicitTimeDiscretization")) return rc;
    return closure_tendencies(grid->d, u, v, w, tracers, ntracers, nu, kappa, Gu, Gv, Gw, Gc, range, nullptr, nullptr, nullptr, true);
}

// implicit_step!(field, implicit_solver, closure, ..., Δt) of one field (vertically_implicit_diffusion_solver.jl:189-213 with the
// diagonals of :58-121 and solve! of batched_tridiagonal_solver.jl:110-133,219-245), constant coefficient `coef` (ν for u, v, w; κ of the
// tracer). form: 0, the reference-shaped kernel (scratch t in memory) -- the only form shipped (ocn_implicit_z.h)
// (the scratch has a size the grid fixes and is never reallocated: a captured time-step may hold its address)
static int ivd_workspace(ocn_grid_s *grid) {
    const DGrid &g = grid->d;
    if (grid->ivd_scratch) return OCN_OK;
    hipError_t e = dev_alloc((void **)&grid->ivd_scratch, sizeof(double) * (size_t)g.Nx * g.Ny * g.Nz);
    if (e != hipSuccess) return fail((int)e, "dev_alloc(implicit solve scratch): %s", hipGetErrorString(e));
    return OCN_OK;
}
static int implicit_step_z(ocn_grid_s *grid, double *field, const int loc[3], double coef, double dt, int form) {
    const DGrid &g = grid->d;
    if (g.tz != OCN_BOUNDED)
        return fail(OCN_EINVAL, "VerticallyImplicitTimeDiscretization can only be specified on grids that are Bounded in the z-direction.");
    if (form != 0) return fail(OCN_EINVAL, "form is 0 (the reference-shaped kernel): no other form is shipped");
    const bool fx = loc[0] == OCN_FACE, fy = loc[1] == OCN_FACE, zf = loc[2] == OCN_FACE;
    if ((fx && fy) || (zf && (fx || fy))) return fail(OCN_EINVAL, "location must be that of u, v, w or a tracer");
    if (!(coef >= 0)) return fail(OCN_EINVAL, "diffusivity must be non-negative");
    int rc = ivd_workspace(grid);
    if (rc) return rc;
    const FView phi = make_view(g, field, loc);
    const dim3 grd((g.Nx + 63) / 64, g.Ny), blk(64);
    if (zf) hipLaunchKernelGGL(implicit_step_z_kernel<true>, grd, blk, 0, g_stream, g, phi, grid->ivd_scratch, dt, coef, fx, fy);
    else    hipLaunchKernelGGL(implicit_step_z_kernel<false>, grd, blk, 0, g_stream, g, phi, grid->ivd_scratch, dt, coef, fx, fy);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_implicit_step_z(ocn_grid_t grid, double *field, const int loc[3], double coef, double dt, int form) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "VerticallyImplicitTimeDiscretization")) return rc_;
    if (!grid || !field || !loc) return fail(OCN_EINVAL, "NULL argument");
    return implicit_step_z(grid, field, loc, coef, dt, form);
}

extern "C" int ocn_compute_closure_tendencies_field(ocn_grid_t grid, const double *u, const double *v, const double *w,
                                                    const double *const *tracers, int ntracers, const double *nu_e,
                                                    const double *const *kappa_e, double *Gu, double *Gv, double *Gw, double *const *Gc,
                                                    const int *range) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "a closure with diffusivity fields (AnisotropicMinimumDissipation)")) return rc_;
    if (int rc = check_closure_arguments(grid, u, v, w, tracers, ntracers, kappa_e, Gu, Gv, Gw, Gc, !nu_e)) return rc;
    if (int rc = refuse_flat(grid->d, "AnisotropicMinimumDissipation", OCN_ENOTSUP, true)) return rc;
    return closure_tendencies(grid->d, u, v, w, tracers, ntracers, 0.0, nullptr, Gu, Gv, Gw, Gc, range, nu_e, kappa_e);
}

// the range of an eddy-coefficient kernel: the interior, or `range` -- the stencils reach one cell further, so it may extend into the halos
// by at most H - 1
static int stencil_range(const DGrid &g, const int *range, Range6 *r) {
    *r = Range6{1, g.Nx, 1, g.Ny, 1, g.Nz};
    if (!range) return OCN_OK;
    const int N[3] = {g.Nx, g.Ny, g.Nz}, H[3] = {g.Hx, g.Hy, g.Hz};
    for (int d = 0; d < 3; ++d)
        if (range[2 * d] < 2 - H[d] || range[2 * d + 1] > N[d] + H[d] - 1)
            return fail(OCN_EINVAL, "range [%d, %d] along dimension %d leaves no halo for the stencil", range[2 * d], range[2 * d + 1], d);
    *r = Range6{range[0], range[1], range[2], range[3], range[4], range[5]};
    return OCN_OK;
}

// the launch of a z-marching eddy-coefficient kernel (ocn_closures.h): 63 columns per wave, 4 rows per block, chunks of at most `maxchunk`
// levels so that ~2000 blocks fill the chip
struct MarchGrid { dim3 grd, blk; int kchunk; };
static MarchGrid march_grid(int nx, int ny, int nz, int maxchunk = 1 << 30) {
    const int bx = (nx + 62) / 63, by = (ny + 3) / 4;
    const int want = std::max(1, 2048 / std::max(1, bx * by));
    const int kchunk = std::min(maxchunk, std::max(std::min(nz, 8), (nz + want - 1) / want));
    return MarchGrid{dim3(bx, by, (nz + kchunk - 1) / kchunk), dim3(64, 4), kchunk};
}

static int amd_diffusivities(const OcnOptions &o, const DGrid &g, double Cnu, const double *Ckappa, const double *u, const double *v, const double *w,
                             const double *const *tr, int ntr, double *nu_e, double *const *kappa_e, const int *range = nullptr) {
    if (int rc = refuse_flat(g, "AnisotropicMinimumDissipation")) return rc;
    AmdArgs a;
    a.ntr = ntr; a.Cnu = Cnu;
    if (int rc = stencil_range(g, range, &a.r)) return rc;
    const int nx = a.r.i1 - a.r.i0 + 1, ny = a.r.j1 - a.r.j0 + 1, nz = a.r.k1 - a.r.k0 + 1;
    if (nx <= 0 || ny <= 0 || nz <= 0) return OCN_OK;
    a.u = make_view(g, u, LOC_U); a.v = make_view(g, v, LOC_V); a.w = make_view(g, w, LOC_W);
    a.nu_e = make_view(g, nu_e, LOC_C);
    for (int t = 0; t < ntr; ++t) {
        a.c[t] = make_view(g, tr[t], LOC_C);
        a.kappa_e[t] = make_view(g, kappa_e[t], LOC_C);
        a.Ck[t] = Ckappa[t];
    }
    if (o.amd_march && ntr <= 3) {
        const MarchGrid m = march_grid(nx, ny, nz, OCN_AMD_MAXCHUNK);       // (the kernel's per-level LDS table holds that many levels)
        switch (ntr) {
            case 0: hipLaunchKernelGGL(amd_diffusivities_march_kernel<0>, m.grd, m.blk, 0, g_stream, g, a, m.kchunk); break;
            case 1: hipLaunchKernelGGL(amd_diffusivities_march_kernel<1>, m.grd, m.blk, 0, g_stream, g, a, m.kchunk); break;
            case 2: hipLaunchKernelGGL(amd_diffusivities_march_kernel<2>, m.grd, m.blk, 0, g_stream, g, a, m.kchunk); break;
            default: hipLaunchKernelGGL(amd_diffusivities_march_kernel<3>, m.grd, m.blk, 0, g_stream, g, a, m.kchunk); break;
        }
    } else
        hipLaunchKernelGGL(amd_diffusivities_kernel, grid3(nx, ny, nz, BLK), BLK, 0, g_stream, g, a);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_compute_amd_diffusivities(ocn_grid_t grid, double Cnu, const double *Ckappa, const double *u, const double *v,
                                             const double *w, const double *const *tracers, int ntracers, double *nu_e,
                                             double *const *kappa_e, const int *range) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "AnisotropicMinimumDissipation")) return rc_;
    if (!grid || !u || !v || !w || !nu_e || ntracers < 0 || ntracers > OCN_MAX_FIELDS - 3 || (ntracers > 0 && (!tracers || !kappa_e || !Ckappa)))
        return fail(OCN_EINVAL, "invalid argument");
    return amd_diffusivities(g_defaults, grid->d, Cnu, Ckappa, u, v, w, tracers, ntracers, nu_e, kappa_e, range);
}

extern "C" int ocn_compute_closure_tendencies_smagorinsky(ocn_grid_t grid, const double *u, const double *v, const double *w,
                                                          const double *const *tracers, int ntracers, const double *nu_e, const double *Pr,
                                                          double *Gu, double *Gv, double *Gw, double *const *Gc, const int *range) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "Smagorinsky")) return rc_;
    if (int rc = check_closure_arguments(grid, u, v, w, tracers, ntracers, Pr, Gu, Gv, Gw, Gc, !nu_e)) return rc;
    for (int t = 0; t < ntracers; ++t)
        if (!(Pr[t] > 0)) return fail(OCN_EINVAL, "the Prandtl number must be positive");
    if (int rc = refuse_flat(grid->d, "Smagorinsky", OCN_ENOTSUP, true)) return rc;
    const double one = 1.0;
    return closure_tendencies(grid->d, u, v, w, tracers, ntracers, 0.0, nullptr, Gu, Gv, Gw, Gc, range, nu_e, nullptr, ntracers > 0 ? Pr : &one);
}

// compute_diffusivities!(diffusivity_fields, closure::Smagorinsky, model; parameters) (smagorinsky.jl:113-127)
static int smagorinsky_viscosity(const OcnOptions &o, ocn_grid_t grid, double C, double Cb, bool lilly, int bk, const double *bT, const double *S,
                                 double grav, double alpha, double beta, const double *u, const double *v, const double *w, double *nu_e,
                                 const int *range = nullptr) {
    const DGrid &g = grid->d;
    if (int rc = refuse_flat(g, "Smagorinsky")) return rc;
    SmagArgs a;
    if (int rc = stencil_range(g, range, &a.r)) return rc;
    const int nx = a.r.i1 - a.r.i0 + 1, ny = a.r.j1 - a.r.j0 + 1, nz = a.r.k1 - a.r.k0 + 1;
    if (nx <= 0 || ny <= 0 || nz <= 0) return OCN_OK;
    if (!lilly) bk = 0;                      // the constant coefficient reads no tracer
    a.u = make_view(g, u, LOC_U); a.v = make_view(g, v, LOC_V); a.w = make_view(g, w, LOC_W);
    a.bT = make_view(g, bk >= 1 ? bT : u, LOC_C); a.S = make_view(g, bk == 2 ? S : u, LOC_C);
    a.nu_e = make_view(g, nu_e, LOC_C);
    a.C = C; a.Cb = Cb; a.grav = grav; a.alpha = alpha; a.beta = beta; a.df2 = grid->df2;
    if (o.smag_march) {
        const MarchGrid m = march_grid(nx, ny, nz);
        if (!lilly) hipLaunchKernelGGL((smagorinsky_viscosity_march_kernel<0, false>), m.grd, m.blk, 0, g_stream, g, a, m.kchunk);
        else if (bk == 0) hipLaunchKernelGGL((smagorinsky_viscosity_march_kernel<0, true>), m.grd, m.blk, 0, g_stream, g, a, m.kchunk);
        else if (bk == 1) hipLaunchKernelGGL((smagorinsky_viscosity_march_kernel<1, true>), m.grd, m.blk, 0, g_stream, g, a, m.kchunk);
        else hipLaunchKernelGGL((smagorinsky_viscosity_march_kernel<2, true>), m.grd, m.blk, 0, g_stream, g, a, m.kchunk);
    } else {
        const dim3 grd = grid3(nx, ny, nz, BLK);
        if (!lilly) hipLaunchKernelGGL((smagorinsky_viscosity_kernel<0, false>), grd, BLK, 0, g_stream, g, a);
        else if (bk == 0) hipLaunchKernelGGL((smagorinsky_viscosity_kernel<0, true>), grd, BLK, 0, g_stream, g, a);
        else if (bk == 1) hipLaunchKernelGGL((smagorinsky_viscosity_kernel<1, true>), grd, BLK, 0, g_stream, g, a);
        else hipLaunchKernelGGL((smagorinsky_viscosity_kernel<2, true>), grd, BLK, 0, g_stream, g, a);
    }
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_compute_smagorinsky_viscosity(ocn_grid_t grid, double C, double Cb, int lilly, int buoyancy_kind, const double *b_or_T,
                                                 const double *S, double g, double alpha, double beta, const double *u, const double *v,
                                                 const double *w, double *nu_e, const int *range) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "Smagorinsky")) return rc_;
    if (!grid || !u || !v || !w || !nu_e || buoyancy_kind < 0 || buoyancy_kind > 2 || (buoyancy_kind >= 1 && !b_or_T) || (buoyancy_kind == 2 && !S))
        return fail(OCN_EINVAL, "invalid argument");
    if (!(C >= 0)) return fail(OCN_EINVAL, "the Smagorinsky coefficient must be non-negative");
    return smagorinsky_viscosity(g_defaults, grid, C, Cb, lilly != 0, buoyancy_kind, b_or_T, S, g, alpha, beta, u, v, w, nu_e, range);
}

// ---------------------------------------------------------------------------------------------------------------------
// Smagorinsky(coefficient = DynamicCoefficient(...)) (ocn_dynamic_smagorinsky.h)
// ---------------------------------------------------------------------------------------------------------------------
// the fields of one coefficient update. mask: the averaged directions (bit d), 0 = LagrangianAveraging. LM, MM: directional only;
// J_LM_prev, J_MM_prev: Lagrangian only. ub, vb, wb: scratch for the filtered velocities at the velocities' locations; mean: two doubles
struct DynFields {
    double *Sigma, *Sigma_bar, *LM, *MM, *J_LM, *J_MM, *J_LM_prev, *J_MM_prev;
    double *ub, *vb, *wb, *mean;
};
static int alloc_parent_zeroed(ocn_grid_t grid, const int loc[3], double **p);

static int dynamic_smagorinsky_check_grid(const ocn_grid_s *grid, int mask) {
    const DGrid &g = grid->d;
    if (int rc = refuse_flat(g, "Smagorinsky", OCN_EINVAL)) return rc;
    if (no_connected_topology(g, "a dynamic Smagorinsky coefficient")) return OCN_ENOTSUP;
    if (g.Hx < 2 || g.Hy < 2 || g.Hz < 2) return fail(OCN_EINVAL, "a dynamic Smagorinsky coefficient needs halos of at least 2 (the filtered velocities read u, v, w to ±2)");
    if (mask == 0 && (!grid->has_nodes || !grid->nodes_c[0]))
        return fail(OCN_ESTATE, "LagrangianAveraging interpolates at displaced nodes: call ocn_grid_set_nodes and ocn_grid_set_node_tables first");
    return OCN_OK;
}

// Average(field, dims = mask) of a ccc field as the diagnostics compute it: the metric where the stretched z is reduced
static int dynamic_average(ocn_grid_t grid, const double *field, int mask, bool metric, double *out) {
    ocn_operand_t op = {};
    op.op = OCN_OP_IDENTITY;
    op.a = field;
    return dg_reduce_operation(grid, &op, OCN_REDUCE_AVERAGE, mask, metric && (mask & 4) && !grid->z_regular, 0, nullptr, out);
}

// compute_coefficient_fields! (dynamic_coefficient.jl:194-217 directional, :292-330 Lagrangian) once the schedule has fired
static int dynamic_coefficient_update(ocn_grid_t grid, const DynFields &F, int mask, double jmin, const double *u, const double *v, const double *w,
                                      double dt, bool initialising) {
    const DGrid &g = grid->d;
    const bool lagr = mask == 0;
    DynArgs a = {};
    a.u = make_view(g, u, LOC_U); a.v = make_view(g, v, LOC_V); a.w = make_view(g, w, LOC_W);
    a.ub = make_view(g, F.ub, LOC_U); a.vb = make_view(g, F.vb, LOC_V); a.wb = make_view(g, F.wb, LOC_W);
    a.Sig = make_view(g, F.Sigma, LOC_C); a.Sigb = make_view(g, F.Sigma_bar, LOC_C);
    a.LM = make_view(g, lagr ? F.J_LM : F.LM, LOC_C); a.MM = make_view(g, lagr ? F.J_MM : F.MM, LOC_C);
    a.JLMp = make_view(g, lagr ? F.J_LM_prev : F.J_LM, LOC_C); a.JMMp = make_view(g, lagr ? F.J_MM_prev : F.J_MM, LOC_C);
    a.df2 = grid->df2; a.df = grid->df;
    a.xc = grid->nodes_c[0]; a.yc = grid->nodes_c[1]; a.zc = grid->nodes_c[2];
    a.jmin = jmin; a.dt = dt;
    hipLaunchKernelGGL(dyn_filter_sigma_kernel, grid3(g.Nx + 2, g.Ny + 2, g.Nz + 2, BLK), BLK, 0, g_stream, g, a);
    KERNEL_CHECK();
    const dim3 grd = grid3(g.Nx, g.Ny, g.Nz, BLK);
    hipLaunchKernelGGL(dyn_sigma_bar_kernel, grd, BLK, 0, g_stream, g, a);
    KERNEL_CHECK();
    if (!lagr) {
        hipLaunchKernelGGL(dyn_lm_mm_kernel<false>, grd, BLK, 0, g_stream, g, a, grid->pg);
        KERNEL_CHECK();
        int rc = dynamic_average(grid, F.LM, mask, true, F.J_LM);
        if (!rc) rc = dynamic_average(grid, F.MM, mask, true, F.J_MM);
        return rc;
    }
    int P[3];
    parent_size(g, LOC_C, P);
    const long n = (long)P[0] * P[1] * P[2];
    HIP_TRY(hipMemcpyAsync(F.J_LM_prev, F.J_LM, n * sizeof(double), hipMemcpyDeviceToDevice, g_stream));
    HIP_TRY(hipMemcpyAsync(F.J_MM_prev, F.J_MM, n * sizeof(double), hipMemcpyDeviceToDevice, g_stream));
    if (!initialising) {
        hipLaunchKernelGGL(dyn_lm_mm_kernel<true>, grd, BLK, 0, g_stream, g, a, grid->pg);
        KERNEL_CHECK();
        return OCN_OK;
    }
    // the first updates: 𝒥 <- LM, MM, then the whole parent <- mean(𝒥) (Statistics.mean: the sum over the number of points, no metric)
    hipLaunchKernelGGL(dyn_lm_mm_kernel<false>, grd, BLK, 0, g_stream, g, a, grid->pg);
    KERNEL_CHECK();
    int rc = dynamic_average(grid, F.J_LM, 7, false, F.mean);
    if (!rc) rc = dynamic_average(grid, F.J_MM, 7, false, F.mean + 1);
    if (rc) return rc;
    const dim3 fg((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(dyn_fill_mean_kernel, fg, dim3(256), 0, g_stream, F.J_LM, n, F.mean, 1, jmin);
    hipLaunchKernelGGL(dyn_fill_mean_kernel, fg, dim3(256), 0, g_stream, F.J_MM, n, F.mean + 1, 0, jmin);
    KERNEL_CHECK();
    return OCN_OK;
}

// _compute_smagorinsky_viscosity! with the coefficient of the 𝒥 fields over the interior
static int dynamic_smagorinsky_viscosity(ocn_grid_t grid, int mask, double jmin, const double *J_LM, const double *J_MM, const double *u, const double *v,
                                         const double *w, double *nu_e) {
    const DGrid &g = grid->d;
    SmagArgs a = {};
    a.r = Range6{1, g.Nx, 1, g.Ny, 1, g.Nz};
    a.u = make_view(g, u, LOC_U); a.v = make_view(g, v, LOC_V); a.w = make_view(g, w, LOC_W);
    a.bT = a.u; a.S = a.u;
    a.nu_e = make_view(g, nu_e, LOC_C);
    a.df2 = grid->df2;
    const DgOut where = dg_make_out(g, LOC_C, mask, nullptr);
    DynCoefficient d = {};
    d.jlm = J_LM; d.jmm = J_MM; d.off = where.off; d.jmin = jmin;
    for (int q = 0; q < 3; ++q) d.s[q] = where.s[q];
    hipLaunchKernelGGL(smagorinsky_viscosity_dynamic_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, a, d);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_dynamic_smagorinsky_update(ocn_grid_t grid, const double *u, const double *v, const double *w, int averaging_mask,
                                              double minimum_numerator, double dt, int initialising, double *Sigma, double *Sigma_bar,
                                              double *LM, double *MM, double *J_LM, double *J_MM, double *J_LM_prev, double *J_MM_prev) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "DynamicSmagorinsky")) return rc_;
    if (!grid || !u || !v || !w || !Sigma || !Sigma_bar || !J_LM || !J_MM || averaging_mask < 0 || averaging_mask > 7)
        return fail(OCN_EINVAL, "invalid argument");
    if (averaging_mask != 0 && (!LM || !MM)) return fail(OCN_EINVAL, "directional averaging needs the LM and MM fields");
    if (averaging_mask == 0 && (!J_LM_prev || !J_MM_prev)) return fail(OCN_EINVAL, "LagrangianAveraging needs the previous J fields");
    if (averaging_mask == 0 && !initialising && !std::isfinite(dt)) return fail(OCN_EINVAL, "dt must be finite");
    int rc = dynamic_smagorinsky_check_grid(grid, averaging_mask);
    if (rc) return rc;
    DynFields F = {Sigma, Sigma_bar, LM, MM, J_LM, J_MM, J_LM_prev, J_MM_prev, nullptr, nullptr, nullptr, nullptr};
    const int *locs[3] = {LOC_U, LOC_V, LOC_W};
    double **scratch[3] = {&F.ub, &F.vb, &F.wb};
    for (int c = 0; c < 3 && !rc; ++c) rc = alloc_parent_zeroed(grid, locs[c], scratch[c]);
    if (!rc && dev_alloc((void **)&F.mean, 2 * sizeof(double)) != hipSuccess) rc = fail(OCN_ESTATE, "dev_alloc(means)");
    if (!rc) rc = dynamic_coefficient_update(grid, F, averaging_mask, minimum_numerator, u, v, w, dt, initialising != 0);
    const hipError_t e = hipStreamSynchronize(g_stream);        // the scratch is this call's
    hipFree(F.ub); hipFree(F.vb); hipFree(F.wb); hipFree(F.mean);
    if (!rc && e != hipSuccess) rc = fail((int)e, "hipStreamSynchronize: %s", hipGetErrorString(e));
    return rc;
}

extern "C" int ocn_compute_dynamic_smagorinsky_viscosity(ocn_grid_t grid, int averaging_mask, double minimum_numerator, const double *J_LM,
                                                         const double *J_MM, const double *u, const double *v, const double *w, double *nu_e) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "DynamicSmagorinsky")) return rc_;
    if (!grid || !u || !v || !w || !nu_e || !J_LM || !J_MM || averaging_mask < 0 || averaging_mask > 7) return fail(OCN_EINVAL, "invalid argument");
    const DGrid &g = grid->d;
    if (int rc = refuse_flat(g, "Smagorinsky", OCN_EINVAL)) return rc;
    if (no_connected_topology(g, "a dynamic Smagorinsky coefficient")) return OCN_ENOTSUP;
    return dynamic_smagorinsky_viscosity(grid, averaging_mask, minimum_numerator, J_LM, J_MM, u, v, w, nu_e);
}

extern "C" int ocn_compute_tendencies_and_substep(ocn_grid_t grid, const double *const *fields, int ntracers, double *const *Gn,
                                                  const int *range, double *const *next, const double *const *Gm, double dt,
                                                  double gamma, double zeta, int has_zeta) {
    NEED_INIT();
    if (int rc_ = refuse_immersed(grid, "the fused tendency-and-substep launch")) return rc_;
    if (!grid || !fields || !Gn || !next || ntracers < 0 || ntracers > 3 || (has_zeta && !Gm)) return fail(OCN_EINVAL, "invalid argument");
    for (int f = 0; f < 3 + ntracers; ++f)
        if (!fields[f] || !Gn[f] || !next[f] || (has_zeta && !Gm[f])) return fail(OCN_EINVAL, "NULL field pointer");
    if (!grid->advection_error.empty()) return fail(OCN_EINVAL, "%s", grid->advection_error.c_str());
    const int impl = g_defaults.tendency_impl ? g_defaults.tendency_impl : 1;
    if (!fused_path(g_defaults, grid->d, range, ntracers, impl))
        return fail(OCN_ENOTSUP, "the fused tendency + substep pass needs Periodic / FullyConnected x and y");
    const FusedSubstep sub{next, has_zeta ? Gm : Gn, dt, gamma, zeta, has_zeta ? 1 : 0};
    return compute_tendencies(g_defaults, grid->d, fields[0], fields[1], fields[2], fields + 3, ntracers, Gn[0], Gn[1], Gn[2], Gn + 3, range, impl, &sub);
}

// ---------------------------------------------------------------------------------------------------------------------
// RK3 substep, tendency caching
// ---------------------------------------------------------------------------------------------------------------------
static int fill_substep_args(const DGrid &g, SubstepArgs &a, double *const *U, const double *const *Gn, const double *const *Gm,
                             const int (*locs)[3], int n, bool exclude_periphery, int *maxnx, int *maxny, int *maxnz) {
    if (n < 0 || n > OCN_MAX_FIELDS) return fail(OCN_EINVAL, "nfields out of range");
    a.n = n;
    *maxnx = *maxny = *maxnz = 0;
    for (int f = 0; f < n; ++f) {
        a.U[f] = U[f]; a.Gn[f] = Gn[f]; a.Gm[f] = Gm ? Gm[f] : nullptr;
        a.view[f] = make_view(g, nullptr, locs[f]);
        a.r[f] = default_range(g, locs[f], exclude_periphery);
        *maxnx = std::max(*maxnx, a.r[f].i1 - a.r[f].i0 + 1);
        *maxny = std::max(*maxny, a.r[f].j1 - a.r[f].j0 + 1);
        *maxnz = std::max(*maxnz, a.r[f].k1 - a.r[f].k0 + 1);
    }
    return OCN_OK;
}

static int rk3_substep(const DGrid &g, double *const *U, const double *const *Gn, const double *const *Gm, const int (*locs)[3],
                       int n, double dt, double gamma, double zeta, bool has_zeta) {
    SubstepArgs a;
    int nx, ny, nz;
    int rc = fill_substep_args(g, a, U, Gn, Gm, locs, n, true, &nx, &ny, &nz);
    if (rc || n == 0 || nx <= 0 || ny <= 0 || nz <= 0) return rc;
    hipLaunchKernelGGL(rk3_substep_kernel, grid3(nx, ny, nz * n, BLK), BLK, 0, g_stream, a, dt, gamma, zeta, has_zeta);
    KERNEL_CHECK();
    return OCN_OK;
}

static int ab2_step(const DGrid &g, double *const *U, const double *const *Gn, const double *const *Gm, const int (*locs)[3], int n,
                    double dt, double chi) {
    SubstepArgs a;
    int nx, ny, nz;
    int rc = fill_substep_args(g, a, U, Gn, Gm, locs, n, true, &nx, &ny, &nz);
    if (rc || n == 0 || nx <= 0 || ny <= 0 || nz <= 0) return rc;
    hipLaunchKernelGGL(ab2_step_kernel, grid3(nx, ny, nz * n, BLK), BLK, 0, g_stream, a, dt, chi);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_ab2_step(ocn_grid_t grid, double *const *U, const double *const *Gn, const double *const *Gm, const int (*locs)[3],
                            int nfields, double dt, double chi) {
    NEED_INIT();
    if (!grid || !U || !Gn || !Gm || !locs) return fail(OCN_EINVAL, "NULL argument");
    return ab2_step(grid->d, U, Gn, Gm, locs, nfields, dt, chi);
}

extern "C" int ocn_rk3_substep(ocn_grid_t grid, double *const *U, const double *const *Gn, const double *const *Gm,
                               const int (*locs)[3], int nfields, double dt, double gamma, double zeta, int has_zeta) {
    NEED_INIT();
    if (!grid || !U || !Gn || !locs || (has_zeta && !Gm)) return fail(OCN_EINVAL, "NULL argument");
    return rk3_substep(grid->d, U, Gn, Gm, locs, nfields, dt, gamma, zeta, has_zeta != 0);
}

extern "C" int ocn_cache_tendencies(ocn_grid_t grid, double *const *Gm, const double *const *Gn, const int (*locs)[3], int nfields) {
    NEED_INIT();
    if (!grid || !Gm || !Gn || !locs) return fail(OCN_EINVAL, "NULL argument");
    SubstepArgs a;
    int nx, ny, nz;
    int rc = fill_substep_args(grid->d, a, Gm, Gn, nullptr, locs, nfields, false, &nx, &ny, &nz);
    if (rc || nfields == 0) return rc;
    hipLaunchKernelGGL(cache_tendencies_kernel, grid3(nx, ny, nz * nfields, BLK), BLK, 0, g_stream, a);
    KERNEL_CHECK();
    return OCN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// pressure source term / correction
// ---------------------------------------------------------------------------------------------------------------------
#include "ocn_pressure_step.h"          // the kernels and the launchers source_term, pressure_correction, divide_interior, ...

extern "C" int ocn_compute_source_term(ocn_grid_t grid, const double *u, const double *v, const double *w, double *rhs_complex,
                                       int weight_by_dz) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !rhs_complex) return fail(OCN_EINVAL, "NULL argument");
    return source_term(grid->d, u, v, w, rhs_complex, weight_by_dz != 0);
}

extern "C" int ocn_make_pressure_correction_divide(ocn_grid_t grid, double *u, double *v, double *w, const double *p, double *p_divided,
                                                   double divisor, const int *range) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !p || !p_divided || p_divided == p) return fail(OCN_EINVAL, "invalid argument (p_divided must be a second array)");
    return pressure_correction(grid->d, u, v, w, p, range, p_divided, divisor);
}

extern "C" int ocn_make_pressure_correction_range(ocn_grid_t grid, double *u, double *v, double *w, const double *p, const int *range) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !p) return fail(OCN_EINVAL, "NULL argument");
    return pressure_correction(grid->d, u, v, w, p, range);
}

extern "C" int ocn_make_pressure_correction(ocn_grid_t grid, double *u, double *v, double *w, const double *p) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !p) return fail(OCN_EINVAL, "NULL argument");
    return pressure_correction(grid->d, u, v, w, p);
}

extern "C" int ocn_divide_interior(ocn_grid_t grid, double *p, double divisor) {
    NEED_INIT();
    if (!grid || !p) return fail(OCN_EINVAL, "NULL argument");
    return divide_interior(grid->d, p, divisor);
}

#include "ocn_poisson.h"
#include "ocn_dist_poisson.h"

// ---------------------------------------------------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------------------------------------------------
struct DistModel;
static void dist_model_free(DistModel *dm);
// The physics of a model: ONE coriolis, ONE buoyancy, ONE closure, ONE Stokes drift. A setter assigns its value as a whole, so what replaces
// what follows from the type; which kernels a step then launches is derived from the four in one place (plan, below).
struct Coriolis {
    enum Kind { NONE, FPLANE, CARTESIAN } kind = NONE;    // nothing | FPlane(f) | ConstantCartesianCoriolis(fx, fy, fz): "coriolis_kind" 0 / 1 / 2
    double f = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
};
struct Buoyancy {
    int kind = 0, bT = 0, S = 0;            // 0 nothing, 1 BuoyancyTracer, 2 linear SeawaterBuoyancy; the tracers' indices
    double grav = 0.0, alpha = 0.0, beta = 0.0;
    // BuoyancyForce(formulation; gravity_unit_vector): ĝ = -gravity_unit_vector, kept whatever the formulation is (each has its setter)
    bool tilted = false;
    double ghat[3] = {0.0, 0.0, 1.0};
    bool acts_tilted() const { return tilted && kind != 0; }
};
struct Closure {
    // nothing | ScalarDiffusivity(ν, κ), not all zero | AnisotropicMinimumDissipation(Cν, Cκ) | Smagorinsky(C, Pr) / SmagorinskyLilly(C, Cb, Pr)
    enum Kind { NONE, SCALAR, AMD, SMAGORINSKY } kind = NONE;
    double nu = 0.0, kappa[OCN_MAX_FIELDS] = {};
    // ... with VerticallyImplicitTimeDiscretization(): implicit_step! after every substep. It may be named before the coefficients (kind
    // NONE or SCALAR) and is never true with AMD / SMAGORINSKY
    bool vi = false;
    double Cnu = 0.0, Ckappa[OCN_MAX_FIELDS] = {};
    double C = 0.0, Cb = 0.0, Pr[OCN_MAX_FIELDS] = {};
    bool lilly = false;
    // Smagorinsky(coefficient = DynamicCoefficient(averaging, schedule = IterationInterval(interval, offset), minimum_numerator)): kind
    // SMAGORINSKY with `dynamic`; averaging_mask bit d = direction d + 1 averaged, 0 = LagrangianAveraging
    bool dynamic = false;
    int averaging_mask = 0;
    double minimum_numerator = 0.0;
    int64_t interval = 1, offset = 0;
    bool eddy() const { return kind == AMD || kind == SMAGORINSKY; }      // the closures with diffusivity fields (Smagorinsky: νₑ only, smagorinsky.jl:131-139)
    // the CLO coordinate of the epilogue kernels (ocn_kernels.h, ocn_epilogue_march.h; their closure term: ocn_closures.h): 0 none, 1 constant ν, κ, 2 coefficient arrays, 3 the same with the tracers'
    // coefficient divided by a Prandtl number (Smagorinsky with some Pr ≠ 1), 4 the explicit part of a vertically implicit ScalarDiffusivity
    int clo(int ntr) const {
        for (int t = 0; t < ntr && kind == SMAGORINSKY; ++t)
            if (Pr[t] != 1.0) return 3;
        return eddy() ? 2 : (kind == SCALAR ? (vi ? 4 : 1) : 0);
    }
};
struct StokesDrift {
    // nothing | UniformStokesDrift: six per-level tables in ONE device block owned by the model (`block`; the views point into it)
    bool on = false;
    double *block = nullptr;
    StokesTables tables = {};
};
struct Particles {
    // nothing | LagrangianParticles: x | y | z | depths in ONE device block owned by the model, n doubles each (`depths` NULL without a
    // DroguedParticleDynamics); per tracked property the particles' values (owned) and the slot of the model field it samples
    bool on = false;
    int n = 0;
    double restitution = 1.0;
    double *block = nullptr, *x = nullptr, *y = nullptr, *z = nullptr, *depths = nullptr;
    int ntracked = 0;
    struct Tracked { char property[48]; char field[16]; double **slot; const int *loc; double *values; } tracked[OCN_MAX_TRACKED] = {};
};
struct ocn_model_s {
    ocn_grid_t grid;
    OcnOptions opt;                         // this model's options: the library defaults when it was created, then ocn_model_set_option
    DistModel *dm = nullptr;                // x-slab partition (ocn_dist.h): communicator, distributed solver, halo buffers
    int ntr, nf;
    double *U[OCN_MAX_FIELDS], *Gn[OCN_MAX_FIELDS], *Gm[OCN_MAX_FIELDS];
    // second set of prognostic arrays: the substeps of stages 2 and 3 are fused into the preceding tendency evaluation and
    // write here (other workgroups still read U), then the two sets swap roles. Two swaps per time-step: the pointers
    // handed out by ocn_model_field are the live ones again at every time-step boundary.
    double *U2[OCN_MAX_FIELDS];
    // option use_graph: the captured step (all pointer swaps of a step cancel out, kernel arguments depend on Δt only); `epoch` is
    // bumped by everything that changes what a step launches
    hipGraphExec_t graph_exec = nullptr;
    double graph_dt = 0.0;
    uint64_t graph_epoch = 0, epoch = 1;
    int graph_replays = 0, graph_captures = 0, graph_failures = 0;
    bool halo_fill_folded = false, stage1_source_fused = false;     // report only (ocn_model_get_option): the path the last time-step took
    int loc[OCN_MAX_FIELDS][3];
    ocn_bc_t bcs[OCN_MAX_FIELDS][6] = {};   // field boundary conditions (default: field_boundary_conditions.jl:15-25)
    ocn_bc_t kbcs[OCN_MAX_FIELDS][6] = {};  // ... of the diffusivity fields: [0] = νₑ, [1 + t] = κₑ of tracer t (boundary_conditions = (κₑ = (b = ...,),))
    bool any_kbc = false;
    bool any_bc = false, any_flux_bc = false;
    struct LinBC { bool on = false; int dep = 0; double a = 0.0, b = 0.0; } lin[OCN_MAX_FIELDS][6];   // linear field-dependent Flux
    bool any_linear_flux = false;
    // FluxBoundaryCondition(func, ...) (ocn_boundary_function.h): per function its field, side and the array it is evaluated into (owned; the
    // side's condition is {OCN_BC_FLUX, 0, array}); the device-resident table of the programs, rewritten by the setters
    struct BoundaryFunctions {
        int n = 0;
        struct Slot { int f, side; BfFunction fn; } slot[BF_MAX_FUNCTIONS];
        BfFunction *table_d = nullptr;
        bool reads_time = false;
    } bf;
    // OpenBoundaryCondition(value; scheme = PerturbationAdvection(...)) per side (0 west .. 5 top) of the wall-normal velocity; the areas of
    // the six faces (the partial sums of the mass-flux correction are the grid's)
    OpenScheme ob[6];
    int n_scheme = 0;
    double ob_area[6] = {};
    Coriolis coriolis;
    Buoyancy buoyancy;
    Closure closure;
    StokesDrift stokes;
    Particles particles;
    double *nu_e = nullptr, *kappa_e[OCN_MAX_FIELDS] = {};   // diffusivity_fields.νₑ, .κₑ (ccc, with halos): allocated by the setters, kept
    // the coefficient fields and scratch of a dynamic Smagorinsky closure (allocated by ocn_model_set_dynamic_smagorinsky, freed when another
    // averaging replaces them and with the model) and diffusivity_fields.previous_compute_time (dynamic_coefficient.jl:342)
    DynFields dyn = {};
    double dyn_previous_time = 0.0;
    // the 𝒥 fields hold nothing yet: set by ocn_model_set_dynamic_smagorinsky and by ocn_model_set_clock (a restored model's 𝒥 are not
    // checkpointed), cleared by the first update that fires, which takes the initialising branch whatever the clock says
    bool dyn_uninitialised = true;
    // forcing = (name = F,) (ocn_forcing.h): host copy of the descriptors, the device-resident table the kernels read, the device copies
    // of the tables (per field and term: mask, target)
    ForcingTable forcing_h = {};
    ForcingTable *forcing_d = nullptr;
    double *forcing_tables[OCN_MAX_FIELDS][OCN_MAX_FORCING_TERMS][2] = {};
    // OCN_FORCING_FUNCTION terms (ocn_forcing_function.h): the host copy of their table (it owns every FfFunction::tab), the device-resident
    // one, whether some program reads t, the longest per-cell program and line
    struct ForcingFunctions {
        FfTable h = {};
        FfTable *d = nullptr;
        bool reads_time = false;
        bool hoist = true;              // model option "forcing_function_hoist": tables + per-cell programs (0: the recorded programs per cell)
        int cell_max = 0, ins_max = 0, Lmax = 1;
        bool cell_arith = true, ins_arith = true;       // no per-cell / recorded program holds exp .. pow: the arithmetic-only kernel serves
    } ff;
    double *pHY = nullptr;                  // hydrostatic pressure anomaly (only with buoyancy)
    // background_fields = (u = Ū, b = B̄, ...) (background_fields.jl): borrowed haloed arrays at their field's location (NULL: ZeroField),
    // and the total velocities U + Ū update_state! forms for the components that have one (owned; allocated by the setter)
    const double *bg[OCN_MAX_FIELDS] = {};
    double *tot[3] = {};
    double *p;
    ocn_poisson_t solver;
    double *blockmax;
    // Clock (TimeSteppers/clock.jl:39-45)
    double time = 0, last_dt = INFINITY, last_stage_dt = INFINITY;
    int64_t iteration = 0;
    int stage = 1;
    // live kernel timing for bench.py's roofline block: hipEvent pairs on the launch stream around every tendency
    // evaluation (the dominant kernel), resolved by ocn_model_profile_read
    int profile = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t events_used = 0;
    bool counted = false;                   // this model is in its grid's count of live models (ocn_grid_set_immersed_boundary)
};

static void dynamic_fields_free(DynFields &F) {
    double *all[] = {F.Sigma, F.Sigma_bar, F.LM, F.MM, F.J_LM, F.J_MM, F.J_LM_prev, F.J_MM_prev, F.ub, F.vb, F.wb, F.mean};
    for (double *p : all) hipFree(p);
    F = DynFields{};
}

extern "C" int ocn_model_destroy(ocn_model_t m) {
    if (!m) return OCN_OK;
    if (m->counted) m->grid->models -= 1;
    dynamic_fields_free(m->dyn);
    for (auto &e : m->events) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    if (m->graph_exec) hipGraphExecDestroy(m->graph_exec);
    for (int f = 0; f < m->nf; ++f) { hipFree(m->U[f]); hipFree(m->U2[f]); hipFree(m->Gn[f]); hipFree(m->Gm[f]); }
    hipFree(m->pHY);
    for (int q = 0; q < m->bf.n; ++q) hipFree(m->bf.slot[q].fn.out);
    hipFree(m->bf.table_d);
    hipFree(m->stokes.block);
    hipFree(m->particles.block);
    for (int q = 0; q < m->particles.ntracked; ++q) hipFree(m->particles.tracked[q].values);
    for (int c = 0; c < 3; ++c) hipFree(m->tot[c]);
    hipFree(m->forcing_d);
    for (int q = 0; q < m->ff.h.n; ++q) hipFree(m->ff.h.fn[q].tab);
    hipFree(m->ff.d);
    for (auto &f : m->forcing_tables)
        for (auto &t : f) { hipFree(t[0]); hipFree(t[1]); }
    hipFree(m->nu_e);
    for (int t = 0; t < OCN_MAX_FIELDS; ++t) hipFree(m->kappa_e[t]);
    hipFree(m->p); hipFree(m->blockmax);
    ocn_poisson_destroy(m->solver);
    dist_model_free(m->dm);
    delete m;
    return OCN_OK;
}

// a zeroed haloed parent array at location `loc`, unless *p already has one: the model's arrays and what the setters add to them (never
// inside a captured step)
static int alloc_parent_zeroed(ocn_grid_t grid, const int loc[3], double **p) {
    if (*p) return OCN_OK;
    int P[3];
    parent_size(grid->d, loc, P);
    const size_t bytes = (size_t)P[0] * P[1] * P[2] * sizeof(double);
    hipError_t e = dev_alloc((void **)p, bytes);
    if (e != hipSuccess) { *p = nullptr; return fail((int)e, "dev_alloc(field): %s", hipGetErrorString(e)); }
    e = hipMemsetAsync(*p, 0, bytes, g_stream);
    if (e != hipSuccess) return fail((int)e, "hipMemset(field): %s", hipGetErrorString(e));
    return OCN_OK;
}

static int model_create(ocn_model_t *model, ocn_grid_t grid, int ntracers, bool with_solver) {
    if (!model || !grid) return fail(OCN_EINVAL, "NULL argument");
    if (ntracers < 0 || ntracers > OCN_MAX_FIELDS - 3) return fail(OCN_EINVAL, "ntracers must be in 0..%d", OCN_MAX_FIELDS - 3);
    // the reference's constructor would inflate the halo (inflate_grid_halo_size, nonhydrostatic_model.jl:184); the binder does that
    // before it creates the handle
    if (!grid->advection_error.empty()) return fail(OCN_EINVAL, "%s", grid->advection_error.c_str());
    ocn_model_s *m = new ocn_model_s();
    m->grid = grid; m->opt = g_defaults; m->ntr = ntracers; m->nf = 3 + ntracers;
    for (int f = 0; f < OCN_MAX_FIELDS; ++f) m->U[f] = m->U2[f] = m->Gn[f] = m->Gm[f] = nullptr;
    m->p = nullptr; m->solver = nullptr; m->blockmax = nullptr;
    const int *locs[3] = {LOC_U, LOC_V, LOC_W};
    int rc = OCN_OK;
    for (int f = 0; f < m->nf && !rc; ++f) {
        const int *l = f < 3 ? locs[f] : LOC_C;
        memcpy(m->loc[f], l, sizeof(int) * 3);
        if (!rc) rc = alloc_parent_zeroed(grid, l, &m->U[f]);
        if (!rc) rc = alloc_parent_zeroed(grid, l, &m->U2[f]);
        if (!rc) rc = alloc_parent_zeroed(grid, l, &m->Gn[f]);
        if (!rc) rc = alloc_parent_zeroed(grid, l, &m->Gm[f]);
    }
    if (!rc) rc = alloc_parent_zeroed(grid, LOC_C, &m->p);
    if (!rc) {
        hipError_t e = dev_alloc((void **)&m->blockmax, 1024 * sizeof(double));
        if (e != hipSuccess) rc = fail((int)e, "hipMalloc: %s", hipGetErrorString(e));
    }
    if (!rc && with_solver) rc = poisson_create(&m->solver, grid, -1, &m->opt);
    if (rc) { ocn_model_destroy(m); return rc; }
    grid->models += 1; m->counted = true;
    *model = m;
    return OCN_OK;
}

extern "C" int ocn_model_create(ocn_model_t *model, ocn_grid_t grid, int ntracers) {
    NEED_INIT();
    auto connected = [](int t) { return t == OCN_CONNECTED || t == OCN_RIGHT_CONNECTED || t == OCN_LEFT_CONNECTED; };
    if (grid && (connected(grid->d.tx) || connected(grid->d.ty)))
        return fail(OCN_EINVAL, "a connected x or y direction needs ocn_dist_model_create");
    return model_create(model, grid, ntracers, true);
}

// "u" | "v" | "w" | "cN" -> the index of the prognostic field, -1 when the model has none of that name
static int field_index(const ocn_model_s *m, const char *name) {
    if (!strcmp(name, "u")) return 0;
    if (!strcmp(name, "v")) return 1;
    if (!strcmp(name, "w")) return 2;
    if (name[0] == 'c' && name[1] >= '0' && name[1] <= '9' && !name[2] && name[1] - '0' < m->ntr) return 3 + (name[1] - '0');
    return -1;
}

static int field_lookup(ocn_model_s *m, const char *name, double ***slot, int **loc) {
    const char *q = name;
    char kind = 'U';
    if (!strcmp(name, "p")) { *slot = &m->p; *loc = const_cast<int *>(LOC_C); return OCN_OK; }
    if (!strcmp(name, "pHY")) {
        if (!m->pHY) return fail(OCN_ESTATE, "the model has no hydrostatic pressure anomaly (buoyancy = nothing)");
        *slot = &m->pHY; *loc = const_cast<int *>(LOC_C); return OCN_OK;
    }
    if (!strcmp(name, "nu_e") || !strncmp(name, "kappa_e", 7)) {
        if (!m->closure.eddy()) return fail(OCN_ESTATE, "the model has no eddy diffusivity fields (closure is not an LES closure)");
        *loc = const_cast<int *>(LOC_C);
        if (!strcmp(name, "nu_e")) { *slot = &m->nu_e; return OCN_OK; }
        if (m->closure.kind == Closure::SMAGORINSKY) return fail(OCN_ESTATE, "a Smagorinsky closure has the eddy viscosity nu_e only (the tracers' coefficient is nu_e / Pr at their flux points)");
        const int t = name[7] - '0';
        if (name[7] < '0' || name[7] > '9' || name[8] || t >= m->ntr) return fail(OCN_EINVAL, "no eddy diffusivity field %s", name);
        *slot = &m->kappa_e[t];
        return OCN_OK;
    }
    // the coefficient fields of a dynamic Smagorinsky closure (allocate_coefficient_fields, dynamic_coefficient.jl:219-230,332-345). J_LM and
    // J_MM of a directional average are REDUCED fields: one point and no halo along every averaged direction
    {
        static const char *const names[8] = {"Sigma", "Sigma_bar", "LM", "MM", "J_LM", "J_MM", "J_LM_prev", "J_MM_prev"};
        double **const slots[8] = {&m->dyn.Sigma, &m->dyn.Sigma_bar, &m->dyn.LM, &m->dyn.MM, &m->dyn.J_LM, &m->dyn.J_MM, &m->dyn.J_LM_prev, &m->dyn.J_MM_prev};
        for (int q = 0; q < 8; ++q)
            if (!strcmp(name, names[q])) {
                if (!m->closure.dynamic) return fail(OCN_ESTATE, "the model has no dynamic Smagorinsky coefficient (no field %s)", name);
                if (!*slots[q]) return fail(OCN_ESTATE, "%s averaging has no field %s", m->closure.averaging_mask ? "directional" : "Lagrangian", name);
                *slot = slots[q]; *loc = const_cast<int *>(LOC_C);
                return OCN_OK;
            }
    }
    // background_fields: "bg_<name>" is the caller's array, "total_<name>" a velocity component's U + Ū as of the last update_state!
    if (!strncmp(name, "bg_", 3) || !strncmp(name, "total_", 6)) {
        const bool total = name[0] == 't';
        const int f = field_index(m, name + (total ? 6 : 3));
        if (f < 0 || (total && f > 2)) return fail(OCN_EINVAL, "no background field %s", name);
        if (!m->bg[f]) return fail(OCN_ESTATE, "the model has no background field for %s", name + (total ? 6 : 3));
        *slot = total ? &m->tot[f] : const_cast<double **>(&m->bg[f]);
        *loc = m->loc[f];
        return OCN_OK;
    }
    if (q[0] == 'G' || q[0] == 'M') { kind = q[0]; ++q; }
    const int f = field_index(m, q);
    if (f < 0) return fail(OCN_EINVAL, "name %s not found in model.velocities or model.tracers.", name);
    *slot = kind == 'U' ? &m->U[f] : (kind == 'G' ? &m->Gn[f] : &m->Gm[f]);
    *loc = m->loc[f];
    return OCN_OK;
}

extern "C" int ocn_model_field(ocn_model_t m, const char *name, double **ptr, int loc[3]) {
    if (!m || !name || !ptr) return fail(OCN_EINVAL, "NULL argument");
    double **slot;
    int *l;
    int rc = field_lookup(m, name, &slot, &l);
    if (rc) return rc;
    *ptr = *slot;
    if (loc) memcpy(loc, l, sizeof(int) * 3);
    return OCN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// tuning options (ocn_options.h): the one table of keys behind ocn_set_option, ocn_model_set_option and ocn_model_get_option
// ---------------------------------------------------------------------------------------------------------------------
enum OptionScope {
    OPT_STEP,          // read while stepping: a model's setting takes effect at its next launch
    OPT_CREATION,      // read only when a model or solver is built: ocn_set_option before the model is created
    OPT_PARTITIONED,   // the partitioned step's: refused on a single-GPU model
};
struct OptionRow {
    const char *key;
    int OcnOptions::*member;
    OptionScope scope;
    bool (*valid)(int);           // nullptr: any value
    const char *range;            // the error message when `valid` refuses a value
    const char *alias;            // the library's earlier name of the same option
};
static bool nonneg(int v) { return v >= 0; }
static bool onoff(int v) { return v == 0 || v == 1; }
// role_ldspad is dynamic LDS beside the role kernel's static arrays, FX[2][TY][66] and FY[2][TY + 1][64] doubles (role_tendency_kernel):
// a workgroup may hold at most the 160 KiB of a CU, so what is left for the pad is 163840 bytes minus those arrays (148256 at TY = 7);
// a larger request fails the launch
static constexpr int kRoleStaticLds = 8 * (2 * OCN_ROLE_TY * 66 + 2 * (OCN_ROLE_TY + 1) * 64);
static constexpr int kRoleLdspadMax = 160 * 1024 - kRoleStaticLds;
static_assert(kRoleLdspadMax == 148256 || OCN_ROLE_TY != 7, "the message of role_ldspad states the bound at TY = 7");
static bool ldspad_fits(int v) { return v >= 0 && v <= kRoleLdspadMax; }
static const OptionRow kOptions[] = {
    {"tendency_impl", &OcnOptions::tendency_impl, OPT_STEP, [](int v) { return v >= 0 && v <= 2; }, "tendency_impl is 0, 1 or 2"},
    {"arithmetic", &OcnOptions::arithmetic, OPT_STEP, [](int v) { return v == 0 || v == 1; }, "arithmetic is 0 (reference sequence) or 1 (contracted)"},
    {"role_kchunk", &OcnOptions::role_kchunk, OPT_STEP, nonneg, "role_kchunk must be >= 0 (0 = automatic)"},
    {"role_ldspad", &OcnOptions::role_ldspad, OPT_STEP, ldspad_fits, "role_ldspad is 0 .. 148256 bytes (the 160 KiB of a CU minus the kernel's own LDS)"},
    {"fused_ty", &OcnOptions::fused_ty, OPT_STEP, [](int v) { return v == 3 || v == 7; }, "fused_ty is 3 or 7"},
    {"fused_kchunk", &OcnOptions::fused_kchunk, OPT_STEP, nonneg, "fused_kchunk must be >= 0 (0 = automatic)"},
    {"fused_zwin", &OcnOptions::fused_zwin, OPT_STEP, onoff, "fused_zwin is 0 or 1"},
    {"fused_xcd", &OcnOptions::fused_xcd, OPT_STEP, onoff, "fused_xcd is 0 or 1"},
    {"epilogue_march", &OcnOptions::epilogue_march, OPT_STEP, onoff, "epilogue_march is 0 or 1"},
    {"epilogue_rows", &OcnOptions::epilogue_rows, OPT_STEP, [](int v) { return v >= 1 && v <= 8; }, "epilogue_rows is 1 .. 8"},
    {"epilogue_kchunk", &OcnOptions::epilogue_kchunk, OPT_STEP, nonneg, "epilogue_kchunk must be >= 0 (0 = automatic)"},
    {"amd_march", &OcnOptions::amd_march, OPT_STEP, onoff, "amd_march is 0 or 1"},
    {"smag_march", &OcnOptions::smag_march, OPT_STEP, onoff, "smag_march is 0 or 1"},
    {"fused_halo", &OcnOptions::fused_halo, OPT_STEP, onoff, "fused_halo is 0 or 1"},
    {"real_fft", &OcnOptions::real_fft, OPT_STEP, onoff, "real_fft is 0 or 1"},
    {"c2r_strided", &OcnOptions::c2r_strided, OPT_CREATION, onoff, "c2r_strided is 0 or 1"},
    {"fused_zfft", &OcnOptions::fused_zfft, OPT_CREATION, onoff, "fused_zfft is 0 or 1"},
    {"split_solve", &OcnOptions::split_solve, OPT_STEP, onoff, "split_solve is 0 or 1"},
    {"line_zl512", &OcnOptions::line_zl512, OPT_STEP, [](int v) { return v == 4 || v == 8; }, "line_zl512 is 4 or 8"},
    {"skip_stage_pressure", &OcnOptions::skip_stage_pressure, OPT_STEP, onoff, "skip_stage_pressure is 0 or 1"},
    {"skip_dead_tendency_store", &OcnOptions::skip_dead_tendency_store, OPT_STEP, onoff, "skip_dead_tendency_store is 0 or 1"},
    {"dist_substructured", &OcnOptions::dist_substructured, OPT_CREATION, onoff, "dist_substructured is 0 or 1"},
    {"dist_zfirst", &OcnOptions::dist_zfirst, OPT_CREATION, onoff, "dist_zfirst is 0 or 1"},
    {"dist_xfast", &OcnOptions::dist_xfast, OPT_CREATION, onoff, "dist_xfast is 0 or 1"},
    {"dist_yline", &OcnOptions::dist_yline, OPT_CREATION, onoff, "dist_yline is 0 or 1"},
    {"dist_fuse_source", &OcnOptions::dist_fuse_source, OPT_STEP, onoff, "dist_fuse_source is 0 or 1"},
    {"dist_xline_group", &OcnOptions::dist_xline_group, OPT_STEP, onoff, "dist_xline_group is 0 or 1"},
    {"dist_pencil_transposes", &OcnOptions::dist_pencil_transposes, OPT_CREATION, onoff, "dist_pencil_transposes is 0 or 1"},
    {"swap_tendencies", &OcnOptions::swap_tendencies, OPT_STEP, onoff, "swap_tendencies is 0 or 1"},
    {"fuse_substep", &OcnOptions::fuse_substep, OPT_STEP, onoff, "fuse_substep is 0 or 1"},
    {"fused_epilogue", &OcnOptions::fused_epilogue, OPT_STEP, onoff, "fused_epilogue is 0 or 1"},
    {"fused_forcing", &OcnOptions::fused_forcing, OPT_STEP, onoff, "fused_forcing is 0 or 1"},
    {"use_graph", &OcnOptions::use_graph, OPT_STEP, onoff, "use_graph is 0 or 1"},
    {"async_halos", &OcnOptions::async_halos, OPT_PARTITIONED, [](int v) { return v >= -1 && v <= 1; }, "async_halos is -1 (automatic), 0 or 1"},
    {"thin_halos", &OcnOptions::thin_halos, OPT_PARTITIONED, onoff, "thin_halos is 0 or 1"},
    {"early_exchange", &OcnOptions::early_exchange, OPT_PARTITIONED, onoff, "early_exchange is 0 or 1"},
    {"strip_width", &OcnOptions::strip_width, OPT_PARTITIONED, nonneg, "strip_width must be >= 0 (0 = automatic)"},
    {"fused_step", &OcnOptions::fused_step, OPT_PARTITIONED, onoff, "fused_step is 0 or 1", "dist_fused_step"},
};

static const OptionRow *find_option(const char *key) {
    for (const OptionRow &r : kOptions)
        if (!strcmp(key, r.key) || (r.alias && !strcmp(key, r.alias))) return &r;
    return nullptr;
}
// the row of `key` after checking `value` against it (nullptr: unknown key or refused value, the error is set)
static const OptionRow *option_row(const char *key, int value) {
    const OptionRow *r = find_option(key);
    if (!r) { fail(OCN_EINVAL, "unknown option %s", key); return nullptr; }
    if (r->valid && !r->valid(value)) { fail(OCN_EINVAL, "%s", r->range); return nullptr; }
    return r;
}

extern "C" int ocn_set_option(const char *key, int value) {
    if (!key) return fail(OCN_EINVAL, "NULL argument");
    const OptionRow *r = option_row(key, value);
    if (!r) return OCN_EINVAL;
    g_defaults.*r->member = value;
    return OCN_OK;
}

static bool dist_fused_step_buffers(const ocn_model_s *m);
static int dist_model_get_option(const ocn_model_s *m, const char *key, int *value);
static void dist_abandon_exchange(ocn_model_s *m);
extern "C" int ocn_model_set_option(ocn_model_t m, const char *key, int value) {
    if (!m || !key) return fail(OCN_EINVAL, "NULL argument");
    m->epoch += 1;
    if (!strcmp(key, "profile")) { m->profile = value; m->events_used = 0; return OCN_OK; }
    if (!strcmp(key, "forcing_function_hoist")) {          // a model's own switch, like "profile": not a tuning option of the table
        if (value != 0 && value != 1) return fail(OCN_EINVAL, "forcing_function_hoist is 0 or 1");
        m->ff.hoist = value != 0;
        return OCN_OK;
    }
    const OptionRow *r = option_row(key, value);
    if (!r) return OCN_EINVAL;
    if (r->scope == OPT_CREATION)
        return fail(OCN_ESTATE, "option %s is read when a model is created: set it with ocn_set_option before creating the model", key);
    if (r->scope == OPT_PARTITIONED && !m->dm) return fail(OCN_EINVAL, "option %s belongs to a partitioned model", key);
    if (r->member == &OcnOptions::fused_step && value && !dist_fused_step_buffers(m))
        return fail(OCN_ENOTSUP, "fused_step needs a (connected, Periodic, Periodic) slab with the z-fastest substructured solver");
    m->opt.*r->member = value;
    return OCN_OK;
}

// the form of the vertically implicit solve a model runs (ocn_implicit_z.h): the reference-shaped one, the only one shipped
static int model_ivd_form(const ocn_model_s *) { return 0; }

// background_fields: how many fields carry one, whether a velocity component does (then the advecting velocities are the totals)
static int count_background(const ocn_model_s *m) {
    int n = 0;
    for (int f = 0; f < m->nf; ++f) n += m->bg[f] ? 1 : 0;
    return n;
}
static bool has_background(const ocn_model_s *m) { return count_background(m) > 0; }
static bool has_background_velocity(const ocn_model_s *m) { return m->bg[0] || m->bg[1] || m->bg[2]; }
// total_velocities(model) (nonhydrostatic_model.jl:265-266): the model's own array where a component has no background (ZeroField)
static const double *total_velocity(const ocn_model_s *m, int c) { return m->bg[c] ? m->tot[c] : m->U[c]; }
static int update_total_velocities(ocn_model_s *m) {
    for (int c = 0; c < 3; ++c)
        if (m->bg[c]) {
            int rc = sum_parent(m->grid->d, m->U[c], m->bg[c], m->loc[c], m->tot[c]);
            if (rc) return rc;
        }
    return OCN_OK;
}

static bool has_forcing(const ocn_model_s *m) {
    for (int f = 0; f < m->nf; ++f)
        if (m->forcing_h.nterms[f] > 0) return true;
    return false;
}
// getbc of every function-valued Flux condition with the fields, their halos and the clock of this moment, into the conditions' arrays:
// ONE launch for all of them, none without one
static int evaluate_boundary_functions(ocn_model_s *m) {
    if (m->bf.n == 0) return OCN_OK;
    BfFields fields = {};
    for (int f = 0; f < m->nf; ++f) fields.p[f] = m->U[f];
    int na = 1, nb = 1;
    for (int q = 0; q < m->bf.n; ++q) { na = std::max(na, m->bf.slot[q].fn.Na); nb = std::max(nb, m->bf.slot[q].fn.Nb); }
    bf_launch(m->bf.table_d, m->bf.n, na, nb, fields, m->time);
    KERNEL_CHECK();
    return OCN_OK;
}

static int count_linear_flux(const ocn_model_s *m) {
    int n = 0;
    for (int f = 0; f < m->nf; ++f)
        for (int sd = 0; sd < 6; ++sd) n += m->lin[f][sd].on ? 1 : 0;
    return n;
}

// What a tendency evaluation of this model launches, derived in ONE place from its physics, conditions and options: host arithmetic only,
// no device call. update_state_tail, tendency_epilogue, the time steppers and the report-only keys of ocn_model_get_option read it; none of
// them derives a rule again.
struct StepPlan {
    bool physics;               // a Coriolis, buoyancy, closure or Stokes-drift term exists
    bool epilogue;              // the one-pass epilogue completes the tendencies (without it the stand-alone kernels add the physics terms)
    bool march;                 // ... in its z-marching form, tendency_epilogue_march_kernel (option "epilogue_march_active")
    bool cor, buoy;             // the template coordinates of the epilogue kernels (kEpilogueKernels, kEpilogueMarchKernels) ...
    int clo, ext, ntr;          // ... Closure::clo; EXT bits: 1 ConstantCartesianCoriolis, 2 gravity_unit_vector, 4 of a SeawaterBuoyancy
    bool stokes;                // ... and STOKES: whether the Stokes terms follow the closure term (kEpilogueStokesKernels)
    int stokes_path;            // which pass adds them (option "stokes_path"): 0 none, 1 stand-alone (stokes_drift_kernel), 2 the per-value epilogue
    bool fuse_substep;          // the RK3 substep of the next stage rides along (option "fuse_substep_active") ...
    bool substep_in_advection;  // ... in the advection kernel; otherwise in the epilogue (option "substep_in_tendency_kernel")
    // which pass adds the forcing term (option "forcing_path"): 0 none, 1 the role tendency kernel, 3 the standalone pass (add_forcing_kernel);
    // 2 (inside the physics epilogue) is reserved: that fusion is not built
    int forcing_path;
    int background_path;        // which kernels evaluate the background terms (option "background_tendency_path"): 0 none, 1 per field, 2 the role kernel
};
static StepPlan plan(const ocn_model_s *m) {
    const DGrid &g = m->grid->d;
    const OcnOptions &o = m->opt;
    const Buoyancy &b = m->buoyancy;
    StepPlan p = {};
    p.cor = m->coriolis.kind != Coriolis::NONE; p.buoy = b.kind != 0; p.clo = m->closure.clo(m->ntr); p.ntr = m->ntr;
    // ConstantCartesianCoriolis (1) / gravity_unit_vector (2; 4: of a SeawaterBuoyancy): the EXT instantiations, the only ones with these terms
    p.ext = (m->coriolis.kind == Coriolis::CARTESIAN ? 1 : 0) | (b.acts_tilted() ? (b.kind == 2 ? 6 : 2) : 0);
    p.stokes = m->stokes.on;
    p.physics = p.cor || p.buoy || p.clo != 0 || p.stokes;
    // the one-pass epilogue runs whenever something follows the advective part: physics terms, valued or field-dependent Flux conditions
    const bool flux = m->any_flux_bc || m->any_linear_flux;
    p.epilogue = o.fused_epilogue && (p.physics || flux) && count_linear_flux(m) <= OCN_EPILOGUE_MAX_LIN;
    // whether the closure terms take the z-marching epilogue (ocn_epilogue_march.h): a grid without Flat directions, at most two tracers, and
    // not the explicit part of a vertically implicit discretisation -- that variant exists in the per-value epilogue only, as do the terms of a
    // ConstantCartesianCoriolis, of a buoyancy with a gravity_unit_vector and of a Stokes drift
    p.march = p.epilogue && o.epilogue_march && p.clo >= 1 && p.clo <= 3 && p.ext == 0 && !p.stokes && m->ntr <= 2 && g.tx != OCN_FLAT && g.ty != OCN_FLAT && g.tz != OCN_FLAT;
    // the Stokes terms: inside the per-value epilogue (a fixed rule, no option), else one stand-alone pass after the stand-alone physics kernels
    p.stokes_path = !p.stokes ? 0 : (p.epilogue ? 2 : 1);
    // the forcing term rides in the role tendency kernel (FORCE instantiation) when that kernel completes the tendency by itself: no physics
    // epilogue, no Flux condition, the role kernel on the whole single-GPU grid, reference arithmetic, Periodic z (the Bounded-z instantiation
    // spilled, ocn_tendency_roles.h) -- the configs[1]-plus-sponge case, which keeps the RK3 substep fused. Partitioned models (interior / strip launches) and everything else take the standalone pass.
    const bool forcing = has_forcing(m), background = has_background(m);
    const bool forcing_in_role = forcing && !background && o.fused_forcing && !m->dm && !p.physics && !flux && !p.epilogue && o.tendency_impl == 2 &&
                                 o.arithmetic == 0 && g.tz == OCN_PERIODIC && fused_path(o, g, nullptr, m->ntr, 2) && role_tendency_supported(o, g);
    p.forcing_path = forcing ? ((forcing_in_role && m->ff.h.n == 0) ? 1 : 3) : 0;      // a function term: always the standalone passes
    p.background_path = !background ? 0 : (split_role_path(o, g, o.tendency_impl) ? 2 : 1);
    // without extra physics the substep rides in the fused advection kernel; with Coriolis / buoyancy / closure terms it rides in
    // the epilogue pass that completes the tendencies (any advection path); a valued Flux condition is added after both
    if (!o.fuse_substep || !o.swap_tendencies) p.fuse_substep = false;
    else if (p.forcing_path == 3) p.fuse_substep = false;            // the forcing pass completes G after the launch the substep would ride in
    else if (p.epilogue) p.fuse_substep = true;                      // the epilogue pass also applies the Flux conditions
    else if (background) p.fuse_substep = false;                     // the second advection term follows the launch the substep would ride in
    else p.fuse_substep = !p.physics && !flux && fused_path(o, g, nullptr, m->ntr, o.tendency_impl);
    p.substep_in_advection = p.fuse_substep && !p.epilogue;
    // An immersed grid takes the plainest composition: the per-field immersed kernels complete the advective part, the stand-alone
    // kernels add the physics terms (their immersed instantiations where a term reads the boundary), the forcing pass follows, and every
    // substep is a launch of its own -- no epilogue, no marching form, nothing riding in another launch. The two masks then sit where
    // the reference has them: update_state and pressure_step.
    if (is_immersed(m->grid)) {
        p.epilogue = p.march = p.fuse_substep = p.substep_in_advection = false;
        p.stokes_path = p.stokes ? 1 : 0;
        p.forcing_path = forcing ? 3 : 0;
        p.background_path = background ? 1 : 0;
    }
    return p;
}
static bool has_physics(const ocn_model_s *m) { return plan(m).physics; }

// G = G_rest + F of every forced field (ocn_forcing.h), one launch after the tendency evaluation is complete (advection, physics
// epilogue) and before the Flux-condition terms (compute_flux_bc_tendencies, which the steppers call when the next stage begins)
static bool has_function_term(const ocn_model_s *m, int f) {
    for (int q = 0; q < m->forcing_h.nterms[f]; ++q)
        if (m->forcing_h.t[f][q].kind == OCN_FORCING_KIND_FUNCTION) return true;
    return false;
}
// Fields with a function term (ocn_forcing_function.h) go to forcing_function_kernel, all their terms in sum order, with m->U, their halos
// and the clock of this tendency evaluation; the tables of programs that read t are refilled first. The other fields stay with
// add_forcing_kernel.
static int add_forcing(ocn_model_s *m) {
    for (int functions = 0; functions < 2; ++functions) {
        ForcingLaunch L = {};
        int nx = 0, ny = 0, nz = 0;
        for (int f = 0; f < m->nf; ++f) {
            if (m->forcing_h.nterms[f] <= 0 || has_function_term(m, f) != (functions == 1)) continue;
            const Range6 &r = m->forcing_h.r[f];
            if (r.i1 < r.i0 || r.j1 < r.j0 || r.k1 < r.k0) continue;
            L.f[L.n] = f; L.U[L.n] = m->U[f]; L.G[L.n] = m->Gn[f]; ++L.n;
            nx = std::max(nx, r.i1 - r.i0 + 1); ny = std::max(ny, r.j1 - r.j0 + 1); nz = std::max(nz, r.k1 - r.k0 + 1);
        }
        if (L.n == 0) continue;
        if (!functions) {
            hipLaunchKernelGGL(add_forcing_kernel, grid3(nx, ny, nz * L.n, BLK), BLK, 0, g_stream, m->grid->d, (const ForcingTable *)m->forcing_d, L, nz);
        } else {
            const bool hoist = m->ff.hoist;
            BfFields fields = {};
            for (int f = 0; f < m->nf; ++f) fields.p[f] = m->U[f];
            if (hoist && m->ff.reads_time) ff_launch_lines(m->ff.d, m->ff.h.n, m->ff.Lmax, m->time, true);
            ff_launch_cells(m->grid->d, m->forcing_d, m->ff.d, L, fields, nx, ny, nz, hoist ? m->ff.cell_max : m->ff.ins_max, m->time, hoist, false,
                            hoist ? m->ff.cell_arith : m->ff.ins_arith);
        }
        KERNEL_CHECK();
    }
    return OCN_OK;
}

// The instantiations of the two epilogue kernels: one table per family, indexed by the plan's coordinates. The validity predicates are the
// list of what exists -- a slot they refuse holds nullptr and its kernel is never instantiated.
//   per value: COR x BUOY x CLO 0..4 x EXT x STOKES, where EXT's bit 1 (ConstantCartesianCoriolis) needs COR, bit 2 (gravity_unit_vector)
//              needs BUOY and bit 4 (... of a SeawaterBuoyancy) needs bit 2: EXT in {0, 1, 2, 3, 6, 7}, 20 + 40 kernels, and as many again
//              with the Stokes terms (STOKES, kEpilogueStokesKernels: their arguments end with the tables): 120
//   marching:  COR x BUOY x CLO 1..3 x NTR 0..2, 36 kernels: no EXT terms and no vertically implicit variant (StepPlan::march)
using EpilogueKernel = void (*)(DGrid, EpilogueArgs);
using EpilogueStokesKernel = void (*)(DGrid, EpilogueStokesArgs);
using EpilogueMarchKernel = void (*)(DGrid, EpilogueArgs, Range6, int);
constexpr bool epilogue_valid(bool cor, bool buoy, int clo, int ext) { return clo >= 0 && clo <= 4 && ext >= 0 && ext <= 7 && (!(ext & 1) || cor) && (!(ext & 2) || buoy) && (!(ext & 4) || (ext & 2)); }
constexpr bool epilogue_march_valid(int clo, int ntr) { return clo >= 1 && clo <= 3 && ntr >= 0 && ntr <= 2; }
constexpr int epilogue_slot(bool cor, bool buoy, int clo, int ext) { return (cor ? 1 : 0) + 2 * ((buoy ? 1 : 0) + 2 * (ext + 8 * clo)); }
constexpr int epilogue_march_slot(bool cor, bool buoy, int clo, int ntr) { return (cor ? 1 : 0) + 2 * ((buoy ? 1 : 0) + 2 * (ntr + 3 * clo)); }
template <int I> constexpr EpilogueKernel epilogue_kernel_at() {
    constexpr bool COR = I % 2 != 0, BUOY = I / 2 % 2 != 0; constexpr int EXT = I / 4 % 8, CLO = I / 32;          // (epilogue_slot)
    if constexpr (epilogue_valid(COR, BUOY, CLO, EXT)) return tendency_epilogue_kernel<COR, BUOY, CLO, EXT>; else return nullptr;
}
template <int I> constexpr EpilogueStokesKernel epilogue_stokes_kernel_at() {
    constexpr bool COR = I % 2 != 0, BUOY = I / 2 % 2 != 0; constexpr int EXT = I / 4 % 8, CLO = I / 32;          // (epilogue_slot)
    if constexpr (epilogue_valid(COR, BUOY, CLO, EXT)) return tendency_epilogue_kernel<COR, BUOY, CLO, EXT, true>; else return nullptr;
}
template <int I> constexpr EpilogueMarchKernel epilogue_march_kernel_at() {
    constexpr bool COR = I % 2 != 0, BUOY = I / 2 % 2 != 0; constexpr int NTR = I / 4 % 3, CLO = I / 12;          // (epilogue_march_slot)
    if constexpr (epilogue_march_valid(CLO, NTR)) return tendency_epilogue_march_kernel<COR, BUOY, CLO, NTR>; else return nullptr;
}
template <size_t... I> constexpr std::array<EpilogueKernel, sizeof...(I)> epilogue_kernels(std::index_sequence<I...>) { return {{epilogue_kernel_at<(int)I>()...}}; }
template <size_t... I> constexpr std::array<EpilogueStokesKernel, sizeof...(I)> epilogue_stokes_kernels(std::index_sequence<I...>) { return {{epilogue_stokes_kernel_at<(int)I>()...}}; }
template <size_t... I> constexpr std::array<EpilogueMarchKernel, sizeof...(I)> epilogue_march_kernels(std::index_sequence<I...>) { return {{epilogue_march_kernel_at<(int)I>()...}}; }
static constexpr auto kEpilogueKernels = epilogue_kernels(std::make_index_sequence<epilogue_slot(true, true, 4, 7) + 1>{});
static constexpr auto kEpilogueStokesKernels = epilogue_stokes_kernels(std::make_index_sequence<epilogue_slot(true, true, 4, 7) + 1>{});      // the STOKES half: same slots
static constexpr auto kEpilogueMarchKernels = epilogue_march_kernels(std::make_index_sequence<epilogue_march_slot(true, true, 3, 2) + 1>{});

// Coriolis, hydrostatic pressure gradient and closure terms of every field -- and, when `sub` is given, the RK3 substep of the next
// stage -- in one launch (tendency_epilogue_kernel)
static int tendency_epilogue(ocn_model_s *m, const StepPlan &p, const FusedSubstep *sub) {
    const DGrid &g = m->grid->d;
    const Buoyancy &b = m->buoyancy;
    const Closure &c = m->closure;
    EpilogueArgs a = {};                          // (its run-time term flags stay unset: no kernel reads them, the terms are template arguments)
    a.n = m->nf; a.ntr = m->ntr;
    a.u = make_view(g, m->U[0], LOC_U); a.v = make_view(g, m->U[1], LOC_V); a.w = make_view(g, m->U[2], LOC_W);
    for (int t = 0; t < m->ntr; ++t) a.c[t] = make_view(g, m->U[3 + t], LOC_C);
    a.pHY = make_view(g, m->pHY ? m->pHY : m->p, LOC_C);
    int nx = 0, ny = 0, nz = 0;
    for (int f = 0; f < m->nf; ++f) {
        a.Gn[f] = m->Gn[f]; a.Gm[f] = sub ? sub->Gm[f] : nullptr; a.Un[f] = sub ? sub->Un[f] : nullptr;
        a.r[f] = default_range(g, m->loc[f], f < 3);
        nx = std::max(nx, a.r[f].i1 - a.r[f].i0 + 1); ny = std::max(ny, a.r[f].j1 - a.r[f].j0 + 1); nz = std::max(nz, a.r[f].k1 - a.r[f].k0 + 1);
    }
    a.fcor = m->coriolis.f; a.cfx = m->coriolis.fx; a.cfy = m->coriolis.fy; a.cfz = m->coriolis.fz;
    a.ghat_x = b.ghat[0]; a.ghat_y = b.ghat[1];
    a.bT = b.kind ? m->U[3 + b.bT] : nullptr; a.bS = b.kind == 2 ? m->U[3 + b.S] : nullptr;
    a.grav = b.grav; a.alpha = b.alpha; a.beta = b.beta;
    a.nu = c.nu;
    for (int t = 0; t < m->ntr; ++t) a.kappa[t] = c.kappa[t];
    if (c.kind == Closure::AMD) {
        a.nu_e = make_view(g, m->nu_e, LOC_C);
        for (int t = 0; t < m->ntr; ++t) a.kappa_e[t] = make_view(g, m->kappa_e[t], LOC_C);
    }
    if (c.kind == Closure::SMAGORINSKY) {
        // every tracer's coefficient array is νₑ; with a Pr ≠ 1 the kernels divide the interpolated value by kappa[t] = Pr[t] (CLO 3)
        a.nu_e = make_view(g, m->nu_e, LOC_C);
        for (int t = 0; t < m->ntr; ++t) { a.kappa_e[t] = a.nu_e; a.kappa[t] = c.Pr[t]; }
    }
    a.substep = sub != nullptr; a.has_zeta = sub && sub->has_zeta;
    a.store_G = !sub || sub->store_G;
    a.store_sides = 0;
    a.dt = sub ? sub->dt : 0.0; a.gamma = sub ? sub->gamma : 0.0; a.zeta = sub ? sub->zeta : 0.0;
    // compute_flux_bc_tendencies! belongs to the stage that FOLLOWS (runge_kutta_3.jl:118,134,150: called right before rk3_substep!), not to
    // update_state!: the conditions are folded in only when that stage's substep rides along; otherwise G stays without them and the
    // stepper adds them when the stage begins (compute_flux_bc_tendencies below) -- with the conditions' values of THAT moment
    const bool with_flux = sub != nullptr;
    if (with_flux) {                      // the function-valued conditions of that stage: m->U and the clock are already its own
        const int rc = evaluate_boundary_functions(m);
        if (rc) return rc;
    }
    a.any_flux = m->any_flux_bc && with_flux;
    a.nlin = 0;
    for (int f = 0; f < m->nf; ++f)
        for (int sd = 0; sd < 6; ++sd)
            if (m->lin[f][sd].on && with_flux) {
                if (a.nlin == OCN_EPILOGUE_MAX_LIN) return fail(OCN_ESTATE, "more than %d field-dependent Flux conditions in the fused epilogue", OCN_EPILOGUE_MAX_LIN);
                a.lin[a.nlin].f = f; a.lin[a.nlin].side = sd; a.lin[a.nlin].dep = m->lin[f][sd].dep;
                a.lin[a.nlin].a = m->lin[f][sd].a; a.lin[a.nlin].b = m->lin[f][sd].b;
                ++a.nlin;
            }
    const int T[3] = {g.tx, g.ty, g.tz};
    for (int f = 0; f < OCN_MAX_FIELDS; ++f)
        for (int sd = 0; sd < 6; ++sd) {
            a.has_flux[f][sd] = with_flux && f < m->nf && ((sd & 1) ? wall_hi(T[sd / 2]) : wall_lo(T[sd / 2])) && m->bcs[f][sd].kind == OCN_BC_FLUX &&
                                (m->bcs[f][sd].value != 0.0 || m->bcs[f][sd].array);
            a.flux[f][sd] = f < m->nf ? m->bcs[f][sd].value : 0.0;
            a.flux_arr[f][sd] = f < m->nf ? m->bcs[f][sd].array : nullptr;
            if (sd < 3) a.loc[f][sd] = f < m->nf ? m->loc[f][sd] : 0;
        }
    if (nx <= 0 || ny <= 0 || nz <= 0) return OCN_OK;
    // closure terms on a grid without Flat directions: the z-marching form (ocn_epilogue_march.h) -- the union of the fields' ranges, one
    // column of halo around it readable
    const OcnOptions &o = m->opt;
    if (p.march) {
        Range6 R = a.r[0];
        for (int f = 1; f < m->nf; ++f) {
            R.i0 = std::min(R.i0, a.r[f].i0); R.i1 = std::max(R.i1, a.r[f].i1); R.j0 = std::min(R.j0, a.r[f].j0); R.j1 = std::max(R.j1, a.r[f].j1);
            R.k0 = std::min(R.k0, a.r[f].k0); R.k1 = std::max(R.k1, a.r[f].k1);
        }
        if (R.i0 - 1 >= 1 - g.Hx && R.i1 + 1 <= g.Nx + g.Hx && R.j0 - 1 >= 1 - g.Hy && R.j1 + 1 <= g.Ny + g.Hy && R.k0 - 1 >= 1 - g.Hz && R.k1 + 1 <= g.Nz + g.Hz) {
            const int ni = R.i1 - R.i0 + 1, nj = R.j1 - R.j0 + 1, nk = R.k1 - R.k0 + 1;
            const int bx = (ni + OCN_EPI_MARCH_COLS - 1) / OCN_EPI_MARCH_COLS, by = (nj + o.epilogue_rows - 1) / o.epilogue_rows;
            int kchunk = o.epilogue_kchunk;
            if (kchunk <= 0) {                       // >= ~8 waves per SIMD over the chip, chunks of at least 8 levels
                kchunk = nk;
                while (kchunk > 8 && (long)bx * by * ((nk + kchunk - 1) / kchunk) * o.epilogue_rows < 8192) kchunk = (kchunk + 1) / 2;
            }
            const dim3 mg(bx, by, (nk + kchunk - 1) / kchunk), mb(64, o.epilogue_rows);
            int mask = 0;                 // sides that carry a Flux condition: epilogue_flux_shell_kernel re-does their cells from the STORED tendency
            for (int f = 0; f < m->nf; ++f)
                for (int sd = 0; sd < 6; ++sd)
                    if ((a.any_flux && a.has_flux[f][sd]) || (with_flux && m->lin[f][sd].on)) mask |= 1 << sd;
            a.store_sides = mask;         // (a tendency that is not stored otherwise still is on those sides)
            const EpilogueMarchKernel march = epilogue_march_valid(p.clo, p.ntr) ? kEpilogueMarchKernels[epilogue_march_slot(p.cor, p.buoy, p.clo, p.ntr)] : nullptr;
            if (!march) return fail(OCN_ESTATE, "no tendency_epilogue_march_kernel<COR %d, BUOY %d, CLO %d, NTR %d>", p.cor, p.buoy, p.clo, p.ntr);
            hipLaunchKernelGGL(march, mg, mb, 0, g_stream, g, a, R, kchunk);
            KERNEL_CHECK();
            if (mask) {
                SideList sl;
                sl.n = 0;
                int na = 1, nb = 1;
                for (int sd = 0; sd < 6; ++sd)
                    if ((mask >> sd) & 1) {
                        sl.side[sl.n++] = sd;
                        na = std::max(na, sd < 2 ? g.Ny : g.Nx); nb = std::max(nb, sd < 4 ? g.Nz : g.Ny);
                    }
                hipLaunchKernelGGL(epilogue_flux_shell_kernel, dim3((na + 63) / 64, (nb + 3) / 4, sl.n), dim3(64, 4), 0, g_stream, g, a, mask, sl);
                KERNEL_CHECK();
            }
            return OCN_OK;
        }
    }
    if (!epilogue_valid(p.cor, p.buoy, p.clo, p.ext)) return fail(OCN_ESTATE, "no tendency_epilogue_kernel<COR %d, BUOY %d, CLO %d, EXT %d>", p.cor, p.buoy, p.clo, p.ext);
    const int slot = epilogue_slot(p.cor, p.buoy, p.clo, p.ext);
    if (p.stokes) {
        EpilogueStokesArgs s;
        static_cast<EpilogueArgs &>(s) = a;
        s.sd = m->stokes.tables;
        hipLaunchKernelGGL(kEpilogueStokesKernels[slot], grid3(nx, ny, nz * m->nf, BLK), BLK, 0, g_stream, g, s);
    } else hipLaunchKernelGGL(kEpilogueKernels[slot], grid3(nx, ny, nz * m->nf, BLK), BLK, 0, g_stream, g, a);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_model_get_option(ocn_model_t m, const char *key, int *value) {
    if (!m || !key || !value) return fail(OCN_EINVAL, "NULL argument");
    if (!dist_model_get_option(m, key, value)) return OCN_OK;                        // fused_step, dist_poisson_layout
    if (const OptionRow *r = find_option(key)) { *value = m->opt.*r->member; return OCN_OK; }
    if (!strcmp(key, "graph_replays")) { *value = m->graph_replays; return OCN_OK; }
    if (!strcmp(key, "graph_captures")) { *value = m->graph_captures; return OCN_OK; }
    if (!strcmp(key, "graph_failures")) { *value = m->graph_failures; return OCN_OK; }
    const StepPlan p = plan(m);
    if (!strcmp(key, "forcing_path")) { *value = p.forcing_path; return OCN_OK; }
    // whether the model's grid has an immersed boundary, and which kernels evaluate its tendencies: 0 none, 1 one field per launch, 2 the
    // flux-sharing role kernel
    if (!strcmp(key, "immersed")) { *value = is_immersed(m->grid) ? 1 : 0; return OCN_OK; }
    if (!strcmp(key, "immersed_tendency_path")) {
        *value = !is_immersed(m->grid) ? 0 : (immersed_role_path(m->opt, m->grid->d, nullptr, m->ntr, m->opt.tendency_impl) ? 2 : 1);
        return OCN_OK;
    }
    if (!strcmp(key, "background_fields")) { *value = count_background(m); return OCN_OK; }
    if (!strcmp(key, "background_tendency_path")) { *value = p.background_path; return OCN_OK; }
    if (!strcmp(key, "vertically_implicit")) { *value = m->closure.vi ? 1 : 0; return OCN_OK; }
    // coriolis = nothing (0) | FPlane (1) | ConstantCartesianCoriolis (2); whether the buoyancy has a gravity_unit_vector
    if (!strcmp(key, "coriolis_kind")) { *value = (p.ext & 1) ? 2 : (p.cor ? 1 : 0); return OCN_OK; }
    if (!strcmp(key, "tilted_gravity")) { *value = (p.ext & 2) ? 1 : 0; return OCN_OK; }
    // stokes_drift = nothing (0) | UniformStokesDrift (1); which pass adds its terms: none (0), stokes_drift_kernel (1), the per-value epilogue (2)
    if (!strcmp(key, "stokes_drift")) { *value = p.stokes ? 1 : 0; return OCN_OK; }
    if (!strcmp(key, "stokes_path")) { *value = p.stokes_path; return OCN_OK; }
    // particles = nothing (0) | LagrangianParticles: their number
    if (!strcmp(key, "particles")) { *value = m->particles.on ? m->particles.n : 0; return OCN_OK; }
    // sides with OpenBoundaryCondition(value; scheme = PerturbationAdvection(...)), and the launches they add to a pressure step: the
    // boundary step and the two of the mass-flux correction, or none
    if (!strcmp(key, "open_boundary_scheme_sides")) { *value = m->n_scheme; return OCN_OK; }
    if (!strcmp(key, "open_boundary_launches")) { *value = m->n_scheme ? 3 : 0; return OCN_OK; }
    // function-valued Flux conditions: their number, the launches they add to each moment the conditions are consumed, whether a program reads t
    if (!strcmp(key, "boundary_functions")) { *value = m->bf.n; return OCN_OK; }
    if (!strcmp(key, "boundary_function_launches")) { *value = m->bf.n ? 1 : 0; return OCN_OK; }
    if (!strcmp(key, "boundary_functions_read_time")) { *value = m->bf.reads_time ? 1 : 0; return OCN_OK; }
    // function-valued forcing terms: their number, the longest per-cell program (the recorded ones with forcing_function_hoist = 0), whether a
    // program reads t
    if (!strcmp(key, "forcing_functions")) { *value = m->ff.h.n; return OCN_OK; }
    if (!strcmp(key, "forcing_function_cell_instructions")) { *value = m->ff.hoist ? m->ff.cell_max : m->ff.ins_max; return OCN_OK; }
    if (!strcmp(key, "forcing_function_hoist")) { *value = m->ff.hoist ? 1 : 0; return OCN_OK; }
    // which instantiation of forcing_function_kernel runs: 1 the arithmetic-only one (no exp .. pow per cell), 0 the full one
    if (!strcmp(key, "forcing_function_arithmetic_only")) { *value = m->ff.h.n > 0 && (m->ff.hoist ? m->ff.cell_arith : m->ff.ins_arith) ? 1 : 0; return OCN_OK; }
    if (!strcmp(key, "forcing_functions_read_time")) { *value = m->ff.reads_time ? 1 : 0; return OCN_OK; }
    // which epilogue adds the closure terms: the z-marching one (1) or the per-value one (0) -- the explicit part of a vertically implicit
    // discretisation exists in the per-value epilogue only
    if (!strcmp(key, "epilogue_march_active")) { *value = p.march ? 1 : 0; return OCN_OK; }
    if (!strcmp(key, "implicit_step_form")) { *value = model_ivd_form(m); return OCN_OK; }
    if (!strcmp(key, "fuse_substep_active")) { *value = p.fuse_substep ? 1 : 0; return OCN_OK; }
    // what the last time-step did on a triply periodic grid: the correction kernel wrote the halos (no fill launches), and the first RK3
    // substep rode in the pressure step's kernels
    if (!strcmp(key, "halo_fill_folded")) { *value = m->halo_fill_folded ? 1 : 0; return OCN_OK; }
    if (!strcmp(key, "stage1_source_fused")) { *value = m->stage1_source_fused ? 1 : 0; return OCN_OK; }
    // what the tendency LAUNCH itself carries (bench.py prices its bytes with these): the next stage's substep rides in the advection kernel
    // only without physics / Flux conditions (with them it rides in the epilogue pass); the tendency of the second stage is then not stored
    if (!strcmp(key, "substep_in_tendency_kernel")) { *value = p.substep_in_advection ? 1 : 0; return OCN_OK; }
    // which path solve_for_pressure! takes on this model's solver: the real-transform path (option real_fft, plans that passed their check)
    // with the z transform fused into the spectral divide, and with the Z2D plan that writes into the haloed pressure field -- rocFFT
    // may refuse that plan, the solver then keeps the dense one. Both 0 on the complex path and on a partitioned model (its own solver)
    if (!strcmp(key, "fused_zfft_active") || !strcmp(key, "c2r_strided_active")) {
        const ocn_poisson_s *s = m->solver;
        const bool real_path = s && m->opt.real_fft && !s->general && s->has_r2c && s->has_c2r;
        *value = !real_path ? 0 : (key[0] == 'f' ? (s->kind == 0 && s->zfused) : s->c2r_strided) ? 1 : 0;
        return OCN_OK;
    }
    // whether the model's pressure step runs the split form (1-D x plans on padded rows, strided_line_fft_kernel along y, the correction from
    // the dense solution): the solver's self-check accepted it at creation (poisson_accept_split keeps the 2-D plans otherwise, without a
    // word) and the options still ask for it -- the condition pressure_step itself tests. 0 on the complex path and on a partitioned model
    if (!strcmp(key, "split_solve_active")) {
        const ocn_poisson_s *s = m->solver;
        *value = !m->dm && s && s->split && m->opt.split_solve && m->opt.real_fft && !s->general ? 1 : 0;
        return OCN_OK;
    }
    if (!strcmp(key, "fused_tendency_active")) {
        *value = !is_immersed(m->grid) && fused_path(m->opt, m->grid->d, nullptr, m->ntr, m->opt.tendency_impl) ? 1 : 0;
        return OCN_OK;
    }
    return fail(OCN_EINVAL, "unknown model option '%s'", key);
}

// everything of update_state! that follows the halo fill of the prognostic fields
static int update_state_tail(ocn_model_s *m, bool compute_tend, const FusedSubstep *sub, const int *amd_range) {
    const DGrid &g = m->grid->d;
    const Coriolis &cor = m->coriolis;
    const Buoyancy &b = m->buoyancy;
    const Closure &c = m->closure;
    int rc;
    // the total velocities of a model with background velocities, from the halo-filled prognostic ones (whole parent arrays)
    if (has_background_velocity(m) && (rc = update_total_velocities(m))) return rc;
    // compute_auxiliaries!: compute_diffusivities! over :xyz (update_nonhydrostatic_model_state.jl:58-69), then
    // fill_halo_regions!(model.diffusivity_fields; only_local_halos = true) (:44) with the default ccc conditions
    if (c.eddy()) {
        // Smagorinsky: the buoyancy is the model's at this moment (nothing: N² = 0), and νₑ is the only field
        if (c.kind == Closure::AMD)
            rc = amd_diffusivities(m->opt, g, c.Cnu, c.Ckappa, m->U[0], m->U[1], m->U[2], m->U + 3, m->ntr, m->nu_e, m->kappa_e, amd_range);
        else if (c.dynamic) {
            // compute_coefficient_fields! (dynamic_coefficient.jl:194-217,292-330): previous_compute_time moves on EVERY call, the fields
            // only where the schedule fires -- (iteration - offset) % interval == 0 with the clock as it stands; the Lagrangian average
            // initialises while last_Δt is not finite (until the third tick!) or no time has passed -- and, beyond the reference, at the first
            // update that fires after the closure or the clock was set: the averaging branch would blend with 𝒥⁻ = 0 (T⁻ = Inf, ε = 0) and
            // leave 𝒥ᴹᴹ = 0, νₑ = 0 for the rest of the run
            const double dt = m->time - m->dyn_previous_time;
            m->dyn_previous_time = m->time;
            rc = OCN_OK;
            if ((m->iteration - c.offset) % c.interval == 0) {
                rc = dynamic_coefficient_update(m->grid, m->dyn, c.averaging_mask, c.minimum_numerator, m->U[0], m->U[1], m->U[2], dt,
                                                m->dyn_uninitialised || !std::isfinite(m->last_dt) || dt == 0);
                m->dyn_uninitialised = false;
            }
            if (!rc) rc = dynamic_smagorinsky_viscosity(m->grid, c.averaging_mask, c.minimum_numerator, m->dyn.J_LM, m->dyn.J_MM, m->U[0], m->U[1], m->U[2], m->nu_e);
        } else
            rc = smagorinsky_viscosity(m->opt, m->grid, c.C, c.Cb, c.lilly, b.kind, b.kind ? m->U[3 + b.bT] : nullptr, b.kind == 2 ? m->U[3 + b.S] : nullptr,
                                       b.grav, b.alpha, b.beta, m->U[0], m->U[1], m->U[2], m->nu_e, amd_range);
        if (rc) return rc;
        const int nk = c.kind == Closure::AMD ? 1 + m->ntr : 1;
        double *K[OCN_MAX_FIELDS];
        int kl[OCN_MAX_FIELDS][3];
        K[0] = m->nu_e;
        for (int t = 0; t + 1 < nk; ++t) K[1 + t] = m->kappa_e[t];
        for (int q = 0; q < nk; ++q) memcpy(kl[q], LOC_C, sizeof(int) * 3);
        // (on an x-slab rank amd_range includes i = 0 and Nx + 1: their z halo cell is filled too, the value a serial run's periodic x
        // fill copies there -- the reference's only_local_halos fill leaves it unwritten on a partitioned grid, halo_communication.jl:87-110)
        if ((rc = fill_halo_regions(m->opt, m->grid, K, kl, nk, true, m->any_kbc ? m->kbcs : nullptr, amd_range != nullptr))) return rc;
    }
    // compute_auxiliaries!: update_hydrostatic_pressure! (update_nonhydrostatic_model_state.jl:58-69)
    if (b.kind && (rc = update_hydrostatic_pressure(g, b.kind, m->U[3 + b.bT], m->U[3 + b.S], b.grav, b.alpha, b.beta, m->pHY, b.tilted, b.ghat[2])))
        return rc;
    if (compute_tend) {
        const StepPlan p = plan(m);
        std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
        if (m->profile) {
            if (m->events_used == m->events.size()) {
                std::pair<hipEvent_t, hipEvent_t> e;
                HIP_TRY(hipEventCreate(&e.first));
                HIP_TRY(hipEventCreate(&e.second));
                m->events.push_back(e);
            }
            ev = &m->events[m->events_used++];
            HIP_TRY(hipEventRecord(ev->first, g_stream));
        }
        const bool physics = p.physics || p.epilogue;
        const ImmView imv = imm_view(m->grid);
        const ImmView *im = is_immersed(m->grid) ? &imv : nullptr;
        if (p.background_path) {
            // G = - div(U + Ū, φ) - div(U, Φ̄) ... (nonhydrostatic_tendency_kernel_functions.jl:86-94,148-156,213-221,276-293): term 1 is
            // today's launch when no velocity has a background (U + ZeroField is U), else the split one with the totals; term 2 accumulates
            // over the fields that have a background (div(U, ::ZeroField) = 0). Neither carries the substep or the forcing: a substep rides
            // in the epilogue pass that closes the cells after both terms, or not at all (StepPlan::fuse_substep).
            if (sub && !physics) return fail(OCN_ESTATE, "fused substep requested in the advection launch of a model with background fields");
            int roles[OCN_MAX_FIELDS], nb = 0;
            for (int f = 0; f < m->nf; ++f) roles[f] = f;
            if (has_background_velocity(m)) {
                const double *adv[3] = {total_velocity(m, 0), total_velocity(m, 1), total_velocity(m, 2)};
                rc = advective_terms(m->opt, g, adv, m->U, m->Gn, roles, m->nf, nullptr, false, m->opt.tendency_impl);
            } else
                rc = compute_tendencies(m->opt, g, m->U[0], m->U[1], m->U[2], m->U + 3, m->ntr, m->Gn[0], m->Gn[1], m->Gn[2], m->Gn + 3, nullptr,
                                        m->opt.tendency_impl);
            for (int f = 0; f < m->nf; ++f)
                if (m->bg[f]) roles[nb++] = f;
            const double *adv[3] = {m->U[0], m->U[1], m->U[2]};
            if (!rc) rc = advective_terms(m->opt, g, adv, m->bg, m->Gn, roles, nb, nullptr, true, m->opt.tendency_impl);
        } else
        rc = compute_tendencies(m->opt, g, m->U[0], m->U[1], m->U[2], m->U + 3, m->ntr, m->Gn[0], m->Gn[1], m->Gn[2], m->Gn + 3, nullptr,
                                m->opt.tendency_impl, physics ? nullptr : sub, p.forcing_path == 1 ? m->forcing_d : nullptr, im);
        if (ev) HIP_TRY(hipEventRecord(ev->second, g_stream));
        if (!rc && physics) {
            if (p.epilogue) { if (p.physics || sub) rc = tendency_epilogue(m, p, sub); }      // (Flux conditions alone and no substep: nothing to do)
            else {
                if (sub) return fail(OCN_ESTATE, "fused substep needs the fused epilogue");
                // the reference's order: x/y_dot_g_b, f x U, the hydrostatic gradient, the closure
                if (!rc && b.acts_tilted())
                    rc = add_buoyancy_acceleration(g, b.kind, m->U[3 + b.bT], m->U[3 + b.S], b.grav, b.alpha, b.beta, b.ghat[0], b.ghat[1], m->Gn[0],
                                                   m->Gn[1], nullptr);
                if (!rc && cor.kind == Coriolis::CARTESIAN)
                    rc = add_cartesian_coriolis(g, cor.fx, cor.fy, cor.fz, m->U[0], m->U[1], m->U[2], m->Gn[0], m->Gn[1], m->Gn[2], nullptr);
                if (!rc && cor.kind == Coriolis::FPLANE) rc = add_fplane_coriolis(g, cor.f, m->U[0], m->U[1], m->Gn[0], m->Gn[1], nullptr, im);
                if (!rc && b.kind) rc = add_hydrostatic_pressure_gradient(g, m->pHY, m->Gn[0], m->Gn[1], nullptr);
                if (!rc && c.kind == Closure::SCALAR)
                    rc = closure_tendencies(g, m->U[0], m->U[1], m->U[2], m->U + 3, m->ntr, c.nu, c.kappa, m->Gn[0], m->Gn[1],
                                            m->Gn[2], m->Gn + 3, nullptr, nullptr, nullptr, nullptr, c.vi, im);
                if (!rc && c.eddy())                  // AMD: νₑ and every κₑ; Smagorinsky: νₑ and the Prandtl numbers
                    rc = closure_tendencies(g, m->U[0], m->U[1], m->U[2], m->U + 3, m->ntr, 0.0, nullptr, m->Gn[0], m->Gn[1], m->Gn[2], m->Gn + 3, nullptr,
                                            m->nu_e, c.kind == Closure::AMD ? m->kappa_e : nullptr, c.kind == Closure::AMD ? nullptr : c.Pr);
                if (!rc && p.stokes_path == 1)        // after the closure, before the forcing
                    rc = add_stokes_drift(g, m->stokes.tables, m->U[0], m->U[1], m->U[2], m->Gn[0], m->Gn[1], m->Gn[2], nullptr, nullptr, nullptr);
            }
        }
        // the last interior term: in the role kernel above, or one pass here (then no substep rides along: StepPlan::fuse_substep)
        if (!rc && p.forcing_path == 3) rc = add_forcing(m);
    }
    return rc;
}

// update_state! (update_nonhydrostatic_model_state.jl:20-56)
static int dist_update_state(ocn_model_s *m, bool compute_tend, const FusedSubstep *sub);
// halos_current: the pressure step of the same time-step has just written every halo (pressure_step, fold_halos)
static int update_state(ocn_model_s *m, bool compute_tend, const FusedSubstep *sub = nullptr, bool halos_current = false) {
    if (m->dm) return dist_update_state(m, compute_tend, sub);
    // "Mask immersed tracers" (update_nonhydrostatic_model_state.jl:22-25): first thing, before the halo fill; one launch for all of them
    int rc = mask_immersed_fields(m->grid, m->U + 3, m->loc + 3, m->ntr, 0.0);
    if (rc) return rc;
    rc = halos_current ? OCN_OK : fill_halo_regions(m->opt, m->grid, m->U, m->loc, m->nf, /*fill_open_bcs=*/false, m->any_bc ? m->bcs : nullptr);
    if (rc) return rc;
    return update_state_tail(m, compute_tend, sub, nullptr);
}

// compute_flux_bc_tendencies! (compute_nonhydrostatic_tendencies.jl:170-184): the time steppers call it right before a substep
// (runge_kutta_3.jl:118,134,150; quasi_adams_bashforth_2.jl:99). Stages whose substep rode along with the previous tendency evaluation had
// the conditions folded into that pass (tendency_epilogue); every other substep calls this first.
static int compute_flux_bc_tendencies(ocn_model_s *m) {
    const DGrid &g = m->grid->d;
    int rc = evaluate_boundary_functions(m);
    if (m->any_flux_bc)
        for (int f = 0; f < m->nf && !rc; ++f) rc = compute_flux_bcs(g, m->Gn[f], m->loc[f], m->bcs[f]);
    if (m->any_linear_flux)
        for (int f = 0; f < m->nf && !rc; ++f)
            for (int sd = 0; sd < 6 && !rc; ++sd)
                if (m->lin[f][sd].on)
                    rc = compute_linear_flux_bc(g, m->Gn[f], m->loc[f], sd, m->lin[f][sd].a, m->lin[f][sd].b, m->U[m->lin[f][sd].dep]);
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------------
// open boundaries with a scheme (ocn_open_boundary.h)
// ---------------------------------------------------------------------------------------------------------------------
// face `side` (0 west .. 5 top) of its wall-normal velocity `p`
static ObFace ob_face(const ocn_grid_s *grid, double *p, int side, double value, const double *arr, const OpenScheme &sc) {
    const DGrid &g = grid->d;
    const int d = side / 2, right = side & 1;
    const int N[3] = {g.Nx, g.Ny, g.Nz}, H[3] = {g.Hx, g.Hy, g.Hz};
    int P[3];
    parent_size(g, d == 0 ? LOC_U : (d == 1 ? LOC_V : LOC_W), P);
    const long s[3] = {1, P[0], (long)P[0] * P[1]};
    const long base = H[0] + s[1] * H[1] + s[2] * H[2];            // parent index of the point (1, 1, 1)
    const int ta = d == 0 ? 1 : 0, tb = d == 2 ? 1 : 2;
    ObFace f = {};
    f.p = p; f.from = p; f.dir = d; f.right = right;
    f.sa = s[ta]; f.sb = s[tb]; f.Na = N[ta]; f.Nb = N[tb];
    f.iB = base + (right ? N[d] : 0) * s[d];
    f.iA = base + (right ? N[d] - 1 : 1) * s[d];
    // Δxᶠᶜᶜ, Δyᶜᶠᶜ, Δzᶜᶜᶠ at the boundary index (perturbation_advection.jl:124,134,145,155,166,176)
    f.dX = d == 0 ? g.dx : (d == 1 ? g.dy : grid->h_dzf[(right ? g.Nz : 0) + g.Hz]);
    f.value = value; f.arr = arr; f.tin = sc.tin; f.tout = sc.tout;
    return f;
}
static void ob_add(ObFaces &S, const ObFace &f) {
    S.f[S.n] = f;
    S.f[S.n].first_block = S.nblocks;
    S.nblocks += (int)(((long)f.Na * f.Nb + OB_THREADS - 1) / OB_THREADS);
    S.n += 1;
}
static bool ob_wall(const DGrid &g, int side) {
    const int T[3] = {g.tx, g.ty, g.tz};
    return (side & 1) ? wall_hi(T[side / 2]) : wall_lo(T[side / 2]);
}
// get_west_area .. get_top_area (boundary_mass_fluxes.jl:11-45): Σ Axᶠᶜᶜ, Σ Ayᶜᶠᶜ, Σ Azᶜᶜᶠ over the face
static double ob_face_area(const ocn_grid_s *grid, int side) {
    const DGrid &g = grid->d;
    const int d = side / 2;
    double sum = 0.0;
    if (d == 2) for (long q = 0; q < (long)g.Nx * g.Ny; ++q) sum += g.dx * g.dy;
    else
        for (int k = 1; k <= g.Nz; ++k)
            for (int a = 0; a < (d == 0 ? g.Ny : g.Nx); ++a) sum += (d == 0 ? g.dy : g.dx) * grid->h_dzc[k - 1 + g.Hz];
    return sum;
}
// the grid's buffer of partial sums: the blocks of all six faces, and the total of ocn_open_boundary_mass_inflow after them
static int ob_blocks_of_all_faces(const DGrid &g) {
    const long n[3] = {(long)g.Ny * g.Nz, (long)g.Nx * g.Nz, (long)g.Nx * g.Ny};
    int b = 0;
    for (int d = 0; d < 3; ++d) b += 2 * (int)((n[d] + OB_THREADS - 1) / OB_THREADS);
    return b;
}
static int ob_partial_buffer(ocn_grid_s *grid) {
    if (!grid->ob_partial) HIP_TRY(dev_alloc((void **)&grid->ob_partial, (size_t)(ob_blocks_of_all_faces(grid->d) + 1) * sizeof(double)));
    return OCN_OK;
}

static int ob_step(const ObFaces &S, double last_stage_dt) {
    if (S.n == 0) return OCN_OK;
    const double dt = std::isinf(last_stage_dt) ? 0.0 : last_stage_dt;          // perturbation_advection.jl:76,100
    hipLaunchKernelGGL(open_boundary_step_kernel, dim3(S.nblocks), dim3(OB_THREADS), 0, g_stream, S, dt);
    KERNEL_CHECK();
    return OCN_OK;
}

// the faces of open_boundary_mass_inflow (boundary_mass_fluxes.jl:57-79,181-198) and of the correction (:200-238) from the wall-normal
// conditions wn[side] of u (west, east), v (south, north), w (bottom, top): scheme faces and array-valued imposed faces are integrated on
// the device, constant imposed faces contribute condition * area here, anything else nothing; only scheme faces are corrected
struct ObPlan { ObFaces flux = {}, corr = {}; double host_flux = 0.0, scheme_area = 0.0; };
static ObPlan ob_plan(const ocn_grid_s *grid, double *const U[3], const ocn_bc_t wn[6], const OpenScheme sc[6], const double area[6]) {
    ObPlan P;
    for (int side = 0; side < 6; ++side) {
        if (!ob_wall(grid->d, side) || wn[side].kind != OCN_BC_OPEN) continue;
        const ObFace f = ob_face(grid, U[side / 2], side, wn[side].value, wn[side].array, sc[side]);
        if (sc[side].on) { ob_add(P.flux, f); ob_add(P.corr, f); P.scheme_area += area[side]; }
        else if (wn[side].array) ob_add(P.flux, f);
        else P.host_flux += (side & 1) ? -(wn[side].value * area[side]) : wn[side].value * area[side];
    }
    return P;
}
// enforce_open_boundary_mass_conservation! (boundary_mass_fluxes.jl:224-239): launch A, launch B; nothing without a scheme face (:216)
static int ob_enforce(const ocn_grid_s *grid, const ObPlan &P, double *partial) {
    if (P.corr.n == 0) return OCN_OK;
    hipLaunchKernelGGL(open_boundary_flux_kernel, dim3(P.flux.nblocks), dim3(OB_THREADS), 0, g_stream, P.flux, grid->d, partial);
    hipLaunchKernelGGL(open_boundary_correct_kernel, dim3(P.corr.nblocks), dim3(OB_THREADS), 0, g_stream, P.corr, (const double *)partial,
                       P.flux.nblocks, P.host_flux, P.scheme_area, (double *)nullptr);
    KERNEL_CHECK();
    return OCN_OK;
}

extern "C" int ocn_step_open_boundary(ocn_grid_t grid, double *field, const int loc[3], int side, double value, const double *value_array,
                                      double inflow_timescale, double outflow_timescale, double last_stage_dt) {
    NEED_INIT();
    if (!grid || !field || !loc) return fail(OCN_EINVAL, "NULL argument");
    if (side < 0 || side > 5) return fail(OCN_EINVAL, "side %d out of range (0..5 = west, east, south, north, bottom, top)", side);
    const int d = side / 2;
    for (int q = 0; q < 3; ++q)
        if (loc[q] != (q == d ? OCN_FACE : OCN_CENTER)) return fail(OCN_EINVAL, "a scheme steps the wall-normal velocity of its side");
    if (!ob_wall(grid->d, side)) return fail(OCN_EINVAL, "side %d is not the wall of a Bounded direction", side);
    if (!(inflow_timescale >= 0) || !(outflow_timescale >= 0)) return fail(OCN_EINVAL, "the timescales must be non-negative");
    OpenScheme sc;
    sc.on = true; sc.tin = inflow_timescale; sc.tout = outflow_timescale;
    ObFaces S = {};
    ob_add(S, ob_face(grid, field, side, value, value_array, sc));
    return ob_step(S, last_stage_dt);
}

extern "C" int ocn_open_boundary_mass_inflow(ocn_grid_t grid, const double *u, const double *v, const double *w, int sides_mask, double *value) {
    NEED_INIT();
    if (!grid || !value) return fail(OCN_EINVAL, "NULL argument");
    if (sides_mask < 0 || sides_mask > 63) return fail(OCN_EINVAL, "sides_mask is a mask of the bits 0 (west) .. 5 (top)");
    double *const U[3] = {const_cast<double *>(u), const_cast<double *>(v), const_cast<double *>(w)};
    ObFaces S = {};
    for (int side = 0; side < 6; ++side) {
        if (!(sides_mask >> side & 1)) continue;
        if (!ob_wall(grid->d, side)) return fail(OCN_EINVAL, "side %d is not the wall of a Bounded direction", side);
        if (!U[side / 2]) return fail(OCN_EINVAL, "NULL velocity for side %d", side);
        ob_add(S, ob_face(grid, U[side / 2], side, 0.0, nullptr, OpenScheme()));
    }
    *value = 0.0;
    if (S.n == 0) return OCN_OK;
    int rc = ob_partial_buffer(grid);
    if (rc) return rc;
    double *partial = grid->ob_partial, *total = partial + ob_blocks_of_all_faces(grid->d);
    hipLaunchKernelGGL(open_boundary_flux_kernel, dim3(S.nblocks), dim3(OB_THREADS), 0, g_stream, S, grid->d, partial);
    ObFaces none = {};
    hipLaunchKernelGGL(open_boundary_correct_kernel, dim3(1), dim3(OB_THREADS), 0, g_stream, none, (const double *)partial, S.nblocks, 0.0, 1.0,
                       total);
    KERNEL_CHECK();
    HIP_TRY(hipMemcpyAsync(value, total, sizeof(double), hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return OCN_OK;
}

extern "C" int ocn_enforce_open_boundary_mass_conservation(ocn_grid_t grid, double *u, double *v, double *w, const ocn_bc_t sides[6],
                                                           int scheme_mask) {
    NEED_INIT();
    if (!grid || !sides) return fail(OCN_EINVAL, "NULL argument");
    if (scheme_mask < 0 || scheme_mask > 63) return fail(OCN_EINVAL, "scheme_mask is a mask of the bits 0 (west) .. 5 (top)");
    double *const U[3] = {u, v, w};
    OpenScheme sc[6];
    double area[6];
    for (int side = 0; side < 6; ++side) {
        sc[side].on = (scheme_mask >> side & 1) != 0;
        if (sides[side].kind != OCN_BC_DEFAULT && sides[side].kind != OCN_BC_OPEN)
            return fail(OCN_EINVAL, "the wall-normal velocity of a side takes an Open condition or the default");
        if (sides[side].kind == OCN_BC_OPEN && !ob_wall(grid->d, side)) return fail(OCN_EINVAL, "side %d is not the wall of a Bounded direction", side);
        if (sc[side].on && sides[side].kind != OCN_BC_OPEN) return fail(OCN_EINVAL, "a scheme belongs to an Open condition (side %d)", side);
        if (sides[side].kind == OCN_BC_OPEN && (sc[side].on || sides[side].array) && !U[side / 2]) return fail(OCN_EINVAL, "NULL velocity for side %d", side);
        area[side] = ob_wall(grid->d, side) ? ob_face_area(grid, side) : 0.0;
    }
    const ObPlan P = ob_plan(grid, U, sides, sc, area);
    if (P.corr.n == 0) return OCN_OK;
    int rc = ob_partial_buffer(grid);
    if (rc) return rc;
    return ob_enforce(grid, P, grid->ob_partial);
}

// fill_halo_regions!(fields, clock, fields(model)) with fill_open_bcs = true on the first `nfields` prognostic fields: the sides with a scheme
// are skipped by the fill and stepped by ONE launch (perturbation_advection.jl:119-180); enforce: enforce_open_boundary_mass_conservation!
// follows (pressure_correction.jl:12-14). A model without scheme sides makes the fill call it always made.
static int fill_open_boundaries(ocn_model_s *m, int nfields, bool enforce) {
    if (!m->n_scheme) return fill_halo_regions(m->opt, m->grid, m->U, m->loc, nfields, true, m->any_bc ? m->bcs : nullptr);
    ocn_bc_t bcs[OCN_MAX_FIELDS][6], wn[6];
    memcpy(bcs, m->bcs, sizeof bcs);
    for (int side = 0; side < 6; ++side) {
        wn[side] = m->bcs[side / 2][side];
        if (m->ob[side].on) bcs[side / 2][side].kind = OCN_BC_OPEN_SCHEME;
    }
    int rc = fill_halo_regions(m->opt, m->grid, m->U, m->loc, nfields, true, bcs);
    if (rc) return rc;
    const ObPlan P = ob_plan(m->grid, m->U, wn, m->ob, m->ob_area);
    if ((rc = ob_step(P.corr, m->last_stage_dt))) return rc;
    return enforce ? ob_enforce(m->grid, P, m->grid->ob_partial) : OCN_OK;
}

// after the two sets of prognostic arrays have swapped (rk3_time_step): the scheme sides' boundary values, which the substep that wrote the
// new set never touches, follow the fields -- implicit_step! and the boundary step read them there. One launch, only with scheme sides.
static int carry_open_boundaries(ocn_model_s *m) {
    ObFaces S = {};
    for (int side = 0; side < 6; ++side) {
        if (!m->ob[side].on) continue;
        ObFace f = ob_face(m->grid, m->U[side / 2], side, 0.0, nullptr, m->ob[side]);
        f.from = m->U2[side / 2];
        ob_add(S, f);
    }
    if (S.n == 0) return OCN_OK;
    hipLaunchKernelGGL(open_boundary_carry_kernel, dim3(S.nblocks), dim3(OB_THREADS), 0, g_stream, S);
    KERNEL_CHECK();
    return OCN_OK;
}

// compute_pressure_correction! (pressure_correction.jl:8-20)
static int compute_pressure_correction(ocn_model_s *m) {
    int rc = fill_open_boundaries(m, 3, true);
    if (rc) return rc;
    if ((rc = solve_for_pressure(m->solver, m->U[0], m->U[1], m->U[2], m->p))) return rc;
    double *pp[1] = {m->p};
    const int pl[1][3] = {{OCN_CENTER, OCN_CENTER, OCN_CENTER}};
    return fill_halo_regions(m->opt, m->grid, pp, pl, 1, true);
}

// make_pressure_correction! (pressure_correction.jl:40-53)
static int make_pressure_correction(ocn_model_s *m, double dt) {
    const DGrid &g = m->grid->d;
    int rc = pressure_correction(g, m->U[0], m->U[1], m->U[2], m->p);
    if (rc) return rc;
    double dtp = std::fmax(2.220446049250313e-16, dt);
    return divide_interior(g, m->p, dtp);
}

// compute_pressure_correction! + make_pressure_correction! (pressure_correction.jl:8-53). With a split solver the inverse transform
// leaves the solution in a dense real array and ONE kernel corrects u, v, w from it and writes p / Δt⁺ into the haloed pressure field
// (was: strided C2R into the field, halo fill, correction kernel, divide kernel).
static int dist_pressure_step(ocn_model_s *m, double dt, bool tendencies_follow, bool keep_p);
// keep_p = false (stages 1 and 2 of an RK3 step): nothing can read pNHS before the next stage overwrites it (the time-step is one call), so the
// dense-solution path neither stores p / Δt⁺ nor fills its halos there -- after the step the field holds the last stage's pressure, as the
// reference's does
//
// Triply periodic grids on the dense-solution path fold the neighbouring passes into the two kernels of this step, on request of the
// time-step that calls it (never remembered in the model: set!, a restored checkpoint or ocn_model_update_state get their own fills):
//   fold_halos: the correction kernel leaves every halo of the prognostic fields and of a stored pNHS current, so the caller skips the
//               fill_halo_regions! at the head of the update_state! that follows, and the pNHS fill below is not launched;
//   pending:    the first RK3 substep has not been applied yet -- it rides in the source-term and correction kernels.
struct PendingSubstep { double dt, gamma; };
static bool periodic_dense_path(const ocn_model_s *m) {
    const ocn_poisson_s *s = m->solver;
    const DGrid &g = m->grid->d;
    // (an immersed grid folds nothing into the pressure step: its masks run between the passes that would be folded)
    return !m->dm && !is_immersed(m->grid) && s && s->split && m->opt.split_solve && m->opt.real_fft && !s->general && g.tx == OCN_PERIODIC &&
           g.ty == OCN_PERIODIC && g.tz == OCN_PERIODIC;
}
static bool can_fold_halo_fill(const ocn_model_s *m) { return periodic_dense_path(m) && m->opt.fused_halo; }
static bool can_fuse_stage1_source(const ocn_model_s *m) { return periodic_dense_path(m) && m->opt.fuse_substep; }

static int pressure_step(ocn_model_s *m, double dt, bool tendencies_follow = true, bool keep_p = true, const PendingSubstep *pending = nullptr,
                         bool fold_halos = false) {
    if (m->dm) return dist_pressure_step(m, dt, tendencies_follow, keep_p || !m->opt.skip_stage_pressure);
    int rc;
    // "Mask immersed velocities" (pressure_correction.jl:10-12): first thing in compute_pressure_correction!, before the velocities' halo
    // fill and the source term; one launch for all three. The solve is the underlying grid's (approximate near the boundary,
    // NonhydrostaticModels.jl:42-58); the correction that follows leaves -Δt ∂p on the immersed faces until the next mask.
    if ((rc = mask_immersed_fields(m->grid, m->U, m->loc, 3, 0.0))) return rc;
    ocn_poisson_s *s = m->solver;
    if ((pending || fold_halos) && !periodic_dense_path(m)) return fail(OCN_ESTATE, "folded pressure step off the periodic dense-solution path");
    if (!(s->split && m->opt.split_solve && m->opt.real_fft && !s->general)) {
        if ((rc = compute_pressure_correction(m))) return rc;
        return make_pressure_correction(m, dt);
    }
    const DGrid &g = m->grid->d;
    // triply periodic: the divergence reads its upper neighbours at the wrapped interior index, so fill_halo_regions!(velocities)
    // (pressure_correction.jl:10) is not needed here -- update_state! fills every halo again before anything else reads one
    const bool ppp = g.tx == OCN_PERIODIC && g.ty == OCN_PERIODIC && g.tz == OCN_PERIODIC;
    if (!ppp && (rc = fill_open_boundaries(m, 3, true))) return rc;
    if (pending) {
        SubstepArgs a;
        int nx, ny, nz;
        if ((rc = fill_substep_args(g, a, m->U, m->Gn, nullptr, m->loc, m->nf, true, &nx, &ny, &nz))) return rc;
        hipLaunchKernelGGL(substep_source_kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, a, pending->dt, pending->gamma, s->rrhs,
                           s->kind == 1);
        KERNEL_CHECK();
    } else if ((rc = source_term(g, m->U[0], m->U[1], m->U[2], s->rrhs, s->kind == 1, true, SourceLayout{{}, false, ppp ? 7 : 0}))) return rc;
    if ((rc = poisson_solve_real_split(s))) return rc;
    const double dtp = std::fmax(2.220446049250313e-16, dt);
    const bool store_p = keep_p || !m->opt.skip_stage_pressure;
    if (pending || fold_halos) {
        FieldList tr;
        tr.n = fold_halos ? m->ntr : 0;
        for (int t = 0; t < tr.n; ++t) tr.p[t] = m->U[3 + t];
        const auto kernel = fold_halos ? (pending ? pressure_correction_periodic_kernel<true, true> : pressure_correction_periodic_kernel<true, false>)
                                       : pressure_correction_periodic_kernel<false, true>;
        hipLaunchKernelGGL(kernel, grid3(g.Nx, g.Ny, g.Nz, BLK), BLK, 0, g_stream, g, make_view(g, m->U[0], LOC_U), make_view(g, m->U[1], LOC_V),
                           make_view(g, m->U[2], LOC_W), (const double *)s->rrhs, make_view(g, m->p, LOC_C), dtp, store_p, tr,
                           (const double *)m->Gn[0], (const double *)m->Gn[1], (const double *)m->Gn[2], pending ? pending->dt : 0.0,
                           pending ? pending->gamma : 0.0);
    } else          // the whole grid as one column range, x wrapped
        launch_pressure_correction_dense(g, m->U[0], m->U[1], m->U[2], DenseSolution{s->rrhs, {}}, nullptr, m->p, dtp, store_p, 1, g.Nx);
    KERNEL_CHECK();
    if (!store_p || fold_halos) return OCN_OK;
    double *pp[1] = {m->p};
    const int pl[1][3] = {{OCN_CENTER, OCN_CENTER, OCN_CENTER}};
    return fill_halo_regions(m->opt, m->grid, pp, pl, 1, true);
}

extern "C" int ocn_model_set_buoyancy(ocn_model_t m, int kind, int b_or_T_index, int S_index, double grav, double alpha, double beta) {
    if (m) m->epoch += 1;
    NEED_INIT();
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    if (kind < 0 || kind > 2) return fail(OCN_EINVAL, "buoyancy kind must be 0 (nothing), 1 (BuoyancyTracer) or 2 (linear SeawaterBuoyancy)");
    if (kind && (b_or_T_index < 0 || b_or_T_index >= m->ntr)) return fail(OCN_EINVAL, "tracer index %d out of range", b_or_T_index);
    if (kind == 2 && (S_index < 0 || S_index >= m->ntr)) return fail(OCN_EINVAL, "tracer index %d out of range", S_index);
    int rc;
    if (kind && (rc = alloc_parent_zeroed(m->grid, LOC_C, &m->pHY))) return rc;
    Buoyancy b = m->buoyancy;               // the gravity_unit_vector stays: it has its own setter
    b.kind = kind; b.bT = b_or_T_index; b.S = kind == 2 ? S_index : b_or_T_index;
    b.grav = grav; b.alpha = alpha; b.beta = beta;
    m->buoyancy = b;
    return OCN_OK;
}

extern "C" int ocn_model_set_coriolis(ocn_model_t m, int enabled, double f) {
    if (m) m->epoch += 1;
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    m->coriolis = Coriolis{enabled ? Coriolis::FPLANE : Coriolis::NONE, f};
    return OCN_OK;
}

extern "C" int ocn_model_set_cartesian_coriolis(ocn_model_t m, int enabled, double fx, double fy, double fz) {
    if (m) m->epoch += 1;
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    if (int rc_ = refuse_immersed(m->grid, "ConstantCartesianCoriolis")) return rc_;
    if (m->dm) return fail(OCN_ENOTSUP, "ConstantCartesianCoriolis is not served on a partitioned model");
    m->coriolis = Coriolis{enabled ? Coriolis::CARTESIAN : Coriolis::NONE, 0.0, fx, fy, fz};
    return OCN_OK;
}

extern "C" int ocn_model_set_gravity_unit_vector(ocn_model_t m, int enabled, double gx, double gy, double gz) {
    if (m) m->epoch += 1;
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    if (int rc_ = refuse_immersed(m->grid, "BuoyancyForce(gravity_unit_vector)")) return rc_;
    if (m->dm) return fail(OCN_ENOTSUP, "gravity_unit_vector is not served on a partitioned model");
    Buoyancy &b = m->buoyancy;
    if (!enabled) { b.tilted = false; b.ghat[0] = 0.0; b.ghat[1] = 0.0; b.ghat[2] = 1.0; return OCN_OK; }      // NegativeZDirection()
    // validate_unit_vector (Grids/input_validation.jl:177-186): ex^2 + ey^2 + ez^2 ≈ 1, isapprox with rtol = sqrt(eps)
    const double n2 = gx * gx + gy * gy + gz * gz;
    if (!std::isfinite(gx) || !std::isfinite(gy) || !std::isfinite(gz) || !(std::fabs(n2 - 1.0) <= std::sqrt(DBL_EPSILON) * std::fmax(std::fabs(n2), 1.0)))
        return fail(OCN_EINVAL, "unit vector must satisfy gx^2 + gy^2 + gz^2 ≈ 1");
    b.tilted = true;
    b.ghat[0] = -gx; b.ghat[1] = -gy; b.ghat[2] = -gz;      // ĝ = -gravity_unit_vector (buoyancy_force.jl:52-54)
    return OCN_OK;
}

// stokes_drift = UniformStokesDrift(∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ) (StokesDrifts.jl:125-178) as host tables per level: ∂z at centres (Nz) and faces
// (Nz + 1), ∂t at centres (Nz); NULL: zeros. Replaces any earlier drift whole; enabled = 0 is stokes_drift = nothing. The tables are copied
// into one device block of the model on the library stream; a refused call leaves the model untouched.
extern "C" int ocn_model_set_stokes_drift(ocn_model_t m, int enabled, const double *dzu_c, const double *dzu_f, const double *dzv_c,
                                          const double *dzv_f, const double *dtu_c, const double *dtv_c) {
    NEED_INIT();
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    if (int rc_ = refuse_immersed(m->grid, "stokes_drift")) return rc_;
    if (m->dm) return fail(OCN_ENOTSUP, "a Stokes drift is not served on a partitioned model");
    const DGrid &g = m->grid->d;
    if (g.tz == OCN_FLAT) return fail(OCN_EINVAL, "a UniformStokesDrift varies with z: the grid needs a z direction");
    StokesDrift sd;
    if (enabled) {
        const int Nz = g.Nz;
        const double *src[6] = {dzu_c, dzu_f, dzv_c, dzv_f, dtu_c, dtv_c};
        const int len[6] = {Nz, Nz + 1, Nz, Nz + 1, Nz, Nz};
        std::vector<double> h((size_t)6 * Nz + 2, 0.0);
        const double *view[6];
        size_t off = 0;
        for (int q = 0; q < 6; ++q) {
            if (src[q]) memcpy(h.data() + off, src[q], sizeof(double) * len[q]);
            off += len[q];
        }
        hipError_t e = dev_alloc((void **)&sd.block, h.size() * sizeof(double));
        if (e != hipSuccess) return fail((int)e, "dev_alloc(stokes drift tables): %s", hipGetErrorString(e));
        e = hipMemcpyAsync(sd.block, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);          // `h` goes away; work already queued may still read the old block
        if (e != hipSuccess) { hipFree(sd.block); return fail((int)e, "stokes drift tables: %s", hipGetErrorString(e)); }
        off = 0;
        for (int q = 0; q < 6; ++q) { view[q] = sd.block + off; off += len[q]; }
        sd.tables = StokesTables{view[0], view[1], view[2], view[3], view[4], view[5]};
        sd.on = true;
    } else {
        hipError_t e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) return fail((int)e, "hipStreamSynchronize: %s", hipGetErrorString(e));
    }
    hipFree(m->stokes.block);
    m->stokes = sd;
    m->epoch += 1;
    return OCN_OK;
}

// particles = LagrangianParticles(x, y, z; restitution, dynamics = DroguedParticleDynamics(depths) | no_dynamics) (LagrangianParticleTracking.jl:
// 60-102) from HOST arrays of n values, copied into one device block of the model on the library stream; replaces the earlier particles
// whole, their tracked properties included. n = 0 with arrays: zero particles (the model steps and launches nothing for them); n = 0 with
// x = y = z = NULL: particles = nothing. A refused call leaves the model untouched.
extern "C" int ocn_model_set_particles(ocn_model_t m, int n, const double *x, const double *y, const double *z, double restitution,
                                       const double *depths) {
    NEED_INIT();
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    if (int rc_ = refuse_immersed(m->grid, "particles (LagrangianParticles)")) return rc_;
    if (m->dm) return fail(OCN_ENOTSUP, "particles are not served on a partitioned model (they would have to migrate between ranks)");
    if (n < 0) return fail(OCN_EINVAL, "the number of particles must not be negative");
    const bool clear = n == 0 && !x && !y && !z && !depths;
    if (!clear && (!x || !y || !z)) return fail(OCN_EINVAL, "NULL argument: x, y and z are arrays of n values");
    if (!clear && !m->grid->has_nodes) return fail(OCN_ESTATE, "the grid has no node coordinates: call ocn_grid_set_nodes");
    Particles P;
    if (!clear) {
        const size_t len = (size_t)n, arrays = depths ? 4 : 3;
        hipError_t e = dev_alloc((void **)&P.block, (len * arrays + 1) * sizeof(double));
        if (e != hipSuccess) return fail((int)e, "dev_alloc(particles): %s", hipGetErrorString(e));
        const double *src[4] = {x, y, z, depths};
        for (size_t q = 0; q < arrays && e == hipSuccess && len; ++q)
            e = hipMemcpyAsync(P.block + q * len, src[q], len * sizeof(double), hipMemcpyHostToDevice, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);          // the host arrays are the caller's; queued work may still read the old block
        if (e != hipSuccess) { hipFree(P.block); return fail((int)e, "particles: %s", hipGetErrorString(e)); }
        P.x = P.block; P.y = P.block + len; P.z = P.block + 2 * len; P.depths = depths ? P.block + 3 * len : nullptr;
        P.on = true; P.n = n; P.restitution = restitution;
    } else {
        hipError_t e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) return fail((int)e, "hipStreamSynchronize: %s", hipGetErrorString(e));
    }
    hipFree(m->particles.block);
    for (int q = 0; q < m->particles.ntracked; ++q) hipFree(m->particles.tracked[q].values);
    m->particles = P;
    m->epoch += 1;
    return OCN_OK;
}

// tracked_fields = (property = field,) (LagrangianParticleTracking.jl:89-102): before every move the particles' `property` is set to the
// model field `field_name` interpolated at them. field_name: "u", "v", "w", "c<n>", "p", "pHY" or "nu_e", looked up like ocn_model_field.
// At most OCN_MAX_TRACKED (8) properties; naming a property again replaces its field.
extern "C" int ocn_model_track_particle_field(ocn_model_t m, const char *property, const char *field_name) {
    NEED_INIT();
    if (!m || !property || !field_name) return fail(OCN_EINVAL, "NULL argument");
    Particles &P = m->particles;
    if (!P.on) return fail(OCN_ESTATE, "the model has no particles");
    if (!property[0] || strlen(property) >= sizeof P.tracked[0].property || strlen(field_name) >= sizeof P.tracked[0].field)
        return fail(OCN_EINVAL, "property or field name is empty or too long");
    if (!strcmp(property, "x") || !strcmp(property, "y") || !strcmp(property, "z"))
        return fail(OCN_EINVAL, "x, y and z are the particles' position, not tracked properties");
    const bool served = field_index(m, field_name) >= 0 || !strcmp(field_name, "p") || !strcmp(field_name, "pHY") || !strcmp(field_name, "nu_e");
    if (!served) return fail(OCN_EINVAL, "a tracked field is a velocity, a tracer c<n>, p, pHY or nu_e; got '%s'", field_name);
    double **slot;
    int *loc;
    const int rc = field_lookup(m, field_name, &slot, &loc);
    if (rc) return rc;
    int q = 0;
    while (q < P.ntracked && strcmp(P.tracked[q].property, property)) ++q;
    if (q == OCN_MAX_TRACKED) return fail(OCN_EINVAL, "at most %d tracked properties", OCN_MAX_TRACKED);
    if (q == P.ntracked) {
        double *values = nullptr;
        const size_t bytes = ((size_t)P.n + 1) * sizeof(double);
        hipError_t e = dev_alloc((void **)&values, bytes);
        if (e != hipSuccess) return fail((int)e, "dev_alloc(tracked property): %s", hipGetErrorString(e));
        e = hipMemsetAsync(values, 0, bytes, g_stream);
        if (e != hipSuccess) { hipFree(values); return fail((int)e, "hipMemset(tracked property): %s", hipGetErrorString(e)); }
        P.tracked[q].values = values;
        strcpy(P.tracked[q].property, property);
        P.ntracked += 1;
    }
    strcpy(P.tracked[q].field, field_name);
    P.tracked[q].slot = slot;
    P.tracked[q].loc = loc;
    m->epoch += 1;
    return OCN_OK;
}

// "x" | "y" | "z" | "depths" | a tracked property -> the device array of n values
static int particle_array(ocn_model_s *m, const char *name, double **ptr) {
    Particles &P = m->particles;
    if (!P.on) return fail(OCN_ESTATE, "the model has no particles");
    *ptr = nullptr;
    if (!strcmp(name, "x")) *ptr = P.x;
    else if (!strcmp(name, "y")) *ptr = P.y;
    else if (!strcmp(name, "z")) *ptr = P.z;
    else if (!strcmp(name, "depths")) *ptr = P.depths;
    else
        for (int q = 0; q < P.ntracked; ++q)
            if (!strcmp(P.tracked[q].property, name)) *ptr = P.tracked[q].values;
    if (!*ptr) return fail(OCN_EINVAL, "the particles have no property '%s' on the device", name);
    return OCN_OK;
}

// particles.properties.<name> -> host_out (n doubles), after everything queued on the library stream
extern "C" int ocn_model_particle_property(ocn_model_t m, const char *name, double *host_out) {
    NEED_INIT();
    if (!m || !name || !host_out) return fail(OCN_EINVAL, "NULL argument");
    double *src;
    const int rc = particle_array(m, name, &src);
    if (rc) return rc;
    if (m->particles.n) HIP_TRY(hipMemcpyAsync(host_out, src, (size_t)m->particles.n * sizeof(double), hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return OCN_OK;
}

extern "C" int ocn_model_set_particle_property(ocn_model_t m, const char *name, const double *host_in) {
    NEED_INIT();
    if (!m || !name || !host_in) return fail(OCN_EINVAL, "NULL argument");
    double *dst;
    const int rc = particle_array(m, name, &dst);
    if (rc) return rc;
    if (m->particles.n) HIP_TRY(hipMemcpyAsync(dst, host_in, (size_t)m->particles.n * sizeof(double), hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    m->epoch += 1;
    return OCN_OK;
}

// length(particles); 0 for particles = nothing
extern "C" int ocn_model_particle_count(ocn_model_t m, int *count) {
    if (!m || !count) return fail(OCN_EINVAL, "NULL argument");
    *count = m->particles.on ? m->particles.n : 0;
    return OCN_OK;
}

// closure = ScalarDiffusivity(ν = nu, κ = kappa[tracer]); replaces any other closure, and with all zeros it is closure = nothing
extern "C" int ocn_model_set_closure(ocn_model_t m, double nu, const double *kappa) {
    if (m) m->epoch += 1;
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    if (nu < 0) return fail(OCN_EINVAL, "viscosity must be non-negative");
    Closure c;
    c.vi = m->closure.vi;                   // the time discretisation has its own setter (and is false with the closures this one replaces)
    c.nu = nu;
    bool any = nu != 0.0;
    for (int t = 0; t < m->ntr; ++t) {
        c.kappa[t] = kappa ? kappa[t] : 0.0;
        if (c.kappa[t] < 0) return fail(OCN_EINVAL, "diffusivity must be non-negative");
        any = any || c.kappa[t] != 0.0;
    }
    c.kind = any ? Closure::SCALAR : Closure::NONE;
    m->closure = c;
    return OCN_OK;
}

// time_discretization of the model's ScalarDiffusivity (scalar_diffusivity.jl:116-141): VerticallyImplicitTimeDiscretization() when
// `enabled`. implicit_diffusion_solver (vertically_implicit_diffusion_solver.jl:149-153) refuses a grid whose z is not Bounded. The eddy-
// coefficient closures have per-column coefficients, which the per-level tables do not serve: the setting is refused with them, and
// ocn_model_set_amd / ocn_model_set_smagorinsky clear it.
extern "C" int ocn_model_set_vertically_implicit(ocn_model_t m, int enabled) {
    if (m) m->epoch += 1;
    NEED_INIT();
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    if (int rc_ = refuse_immersed(m->grid, "VerticallyImplicitTimeDiscretization")) return rc_;
    if (!enabled) { m->closure.vi = false; return OCN_OK; }
    if (m->grid->d.tz != OCN_BOUNDED)
        return fail(OCN_EINVAL, "VerticallyImplicitTimeDiscretization can only be specified on grids that are Bounded in the z-direction.");
    if (m->closure.eddy())
        return fail(OCN_ENOTSUP, "VerticallyImplicitTimeDiscretization is accelerated for ScalarDiffusivity with constant coefficients only");
    int rc = ivd_workspace(m->grid);       // (allocated here: not inside a captured step)
    if (rc) return rc;
    m->closure.vi = true;
    return OCN_OK;
}

// implicit_step! of every prognostic field after its substep (runge_kutta_3.jl:185-200, quasi_adams_bashforth_2.jl:133-152); a field
// whose coefficient is zero has the identity system
static int implicit_step(ocn_model_s *m, double dt) {
    if (m->closure.kind != Closure::SCALAR || !m->closure.vi) return OCN_OK;
    const int form = model_ivd_form(m);
    for (int f = 0; f < m->nf; ++f) {
        const double coef = f < 3 ? m->closure.nu : m->closure.kappa[f - 3];
        if (coef == 0.0) continue;
        const int rc = implicit_step_z(m->grid, m->U[f], m->loc[f], coef, dt, form);
        if (rc) return rc;
    }
    return OCN_OK;
}

static int bf_remove(ocn_model_s *m, int f, int side);
// name.side = FluxBoundaryCondition((ξ, η, t, φ, p) -> a + b φ, field_dependencies = dep) (continuous_boundary_function.jl:128-161)
extern "C" int ocn_model_set_linear_flux_bc(ocn_model_t m, const char *name, int side, double a, double b, const char *dep) {
    if (!m || !name || !dep) return fail(OCN_EINVAL, "NULL argument");
    m->epoch += 1;
    const int f = field_index(m, name), fd = field_index(m, dep);
    if (f < 0 || fd < 0) return fail(OCN_EINVAL, "name %s not found in model.velocities or model.tracers.", f < 0 ? name : dep);
    int rc = validate_bc(m->grid->d, m->loc[f], side, OCN_BC_FLUX);
    if (rc) return rc;
    for (int q = 0; q < 3; ++q)
        if (m->loc[fd][q] != m->loc[f][q])
            return fail(OCN_ENOTSUP, "the field dependency %s must sit at the location of %s (identity interpolation to the boundary)", dep, name);
    if ((rc = bf_remove(m, f, side))) return rc;         // the linear family replaces a function on this side
    m->bcs[f][side].kind = OCN_BC_FLUX; m->bcs[f][side].value = 0.0; m->bcs[f][side].array = nullptr;   // halos of a Flux side: zero gradient
    m->any_bc = true;
    m->lin[f][side].on = true; m->lin[f][side].dep = fd; m->lin[f][side].a = a; m->lin[f][side].b = b;
    m->any_linear_flux = true;
    return OCN_OK;
}

// forcing = (name = F,) of the model constructor (Forcings/model_forcing.jl, relaxation.jl, forcing.jl:165-177, multiple_forcings.jl):
// the descriptors of field `field` are replaced; the device-resident table is rewritten (ocn_forcing.h)
// background_fields = (name = parent,) (background_fields.jl:97-116 after regularisation: an array at the field's location)
extern "C" int ocn_model_set_background_field(ocn_model_t m, const char *name, const double *parent) {
    NEED_INIT();
    if (m) m->epoch += 1;
    if (!m || !name) return fail(OCN_EINVAL, "NULL argument");
    if (int rc_ = refuse_immersed(m->grid, "background_fields")) return rc_;
    if (m->dm) return fail(OCN_ENOTSUP, "background fields are not served on a partitioned model");
    const int f = field_index(m, name);
    if (f < 0) return fail(OCN_EINVAL, "background fields can be set on u, v, w and the tracers c0..c%d; got '%s'", m->ntr - 1, name);
    // the total-velocity buffer of this component: made here, never inside a (captured) time-step
    int rc;
    if (f < 3 && parent && (rc = alloc_parent_zeroed(m->grid, m->loc[f], &m->tot[f]))) return rc;
    m->bg[f] = parent;
    return OCN_OK;
}

extern "C" int ocn_model_set_forcing(ocn_model_t m, int field, const ocn_forcing_t *terms, int nterms) {
    NEED_INIT();
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    if (field < 0 || field >= m->nf) return fail(OCN_EINVAL, "forcing field index %d outside 0..%d", field, m->nf - 1);
    if (nterms < 0 || nterms > OCN_MAX_FORCING_TERMS) return fail(OCN_EINVAL, "nterms = %d outside 0..%d", nterms, OCN_MAX_FORCING_TERMS);
    if (nterms > 0 && !terms) return fail(OCN_EINVAL, "NULL terms");
    const DGrid &g = m->grid->d;
    const int T[3] = {g.tx, g.ty, g.tz};
    int P[3];
    parent_size(g, m->loc[field], P);
    for (int q = 0; q < nterms; ++q) {
        const ocn_forcing_t &t = terms[q];
        if (t.kind == OCN_FORCING_ARRAY) {
            if (!t.array) return fail(OCN_EINVAL, "term %d: Forcing(array) with a NULL array", q);
        } else if (t.kind == OCN_FORCING_RELAXATION) {
            const int dirs[2] = {t.mask_dir, t.target_dir};
            const double *tabs[2] = {t.mask_table, t.target_table};
            for (int w = 0; w < 2; ++w) {
                if (dirs[w] < -1 || dirs[w] > 2) return fail(OCN_EINVAL, "term %d: %s direction %d is not -1, 0, 1 or 2", q, w ? "target" : "mask", dirs[w]);
                if (dirs[w] >= 0 && !tabs[w]) return fail(OCN_EINVAL, "term %d: NULL %s table", q, w ? "target" : "mask");
                if (dirs[w] >= 0 && T[dirs[w]] == OCN_FLAT)
                    return fail(OCN_EINVAL, "term %d: a %s along %c, which is Flat (relaxation.jl has no method for it)", q, w ? "target" : "mask", "xyz"[dirs[w]]);
            }
        } else if (t.kind == OCN_FORCING_FUNCTION) {
            if (m->dm) return fail(OCN_ENOTSUP, "term %d: forcing functions are not served on a partitioned model", q);
            const int rc = bf_validate_program(t.program, t.n, t.ndeps, nullptr, 2);
            if (rc) return rc;
            if (t.ndeps > 0 && !t.dep_names) return fail(OCN_EINVAL, "term %d: NULL dependency names", q);
        } else return fail(OCN_EINVAL, "term %d: unknown forcing kind %d", q, t.kind);
    }
    // function terms (ocn_forcing_function.h): built, their tables allocated, before anything of the previous forcing changes
    FfFunction made[OCN_MAX_FORCING_TERMS];
    int nmade = 0, kept = 0;
    auto release_made = [&]() { for (int q = 0; q < nmade; ++q) hipFree(made[q].tab); };
    for (int q = 0; q < m->ff.h.n; ++q) kept += m->ff.h.fn[q].field != field ? 1 : 0;
    for (int q = 0; q < nterms; ++q) {
        const ocn_forcing_t &t = terms[q];
        if (t.kind != OCN_FORCING_FUNCTION) continue;
        if (kept + nmade == FF_MAX_FUNCTIONS) { release_made(); return fail(OCN_EINVAL, "a model carries at most %d forcing functions", FF_MAX_FUNCTIONS); }
        int dep_field[BF_MAX_DEPS], dep_locs[BF_MAX_DEPS][3], rc = OCN_OK;
        for (int s = 0; s < t.ndeps && !rc; ++s) {
            dep_field[s] = t.dep_names[s] ? field_index(m, t.dep_names[s]) : -1;
            if (dep_field[s] < 0) rc = fail(OCN_EINVAL, "name %s not found in model.velocities or model.tracers.", t.dep_names[s] ? t.dep_names[s] : "(NULL)");
            else memcpy(dep_locs[s], m->loc[dep_field[s]], sizeof(int) * 3);
        }
        if (!rc) rc = ff_make_function(m->grid, t.program, t.n, m->loc[field], dep_field, dep_locs, t.ndeps, &made[nmade]);
        if (rc) { release_made(); return rc; }
        made[nmade].field = field; made[nmade].term = q;
        ++nmade;
    }
    // device copies of the tables first: nothing of the previous forcing is released before the new one is complete
    double *dev[OCN_MAX_FORCING_TERMS][2] = {};
    auto release = [&]() { for (auto &d : dev) { hipFree(d[0]); hipFree(d[1]); } release_made(); };
    for (int q = 0; q < nterms; ++q)
        for (int w = 0; w < 2; ++w) {
            const int dir = w ? terms[q].target_dir : terms[q].mask_dir;
            if (terms[q].kind != OCN_FORCING_RELAXATION || dir < 0) continue;
            const size_t bytes = (size_t)P[dir] * sizeof(double);
            hipError_t e = dev_alloc((void **)&dev[q][w], bytes);
            if (e == hipSuccess) e = hipMemcpyAsync(dev[q][w], w ? terms[q].target_table : terms[q].mask_table, bytes, hipMemcpyHostToDevice, g_stream);
            if (e != hipSuccess) { release(); return fail((int)e, "forcing table: %s", hipGetErrorString(e)); }
        }
    if (!m->forcing_d) {
        hipError_t e = dev_alloc((void **)&m->forcing_d, sizeof(ForcingTable));
        if (e != hipSuccess) { m->forcing_d = nullptr; release(); return fail((int)e, "dev_alloc(forcing table): %s", hipGetErrorString(e)); }
    }
    // the table must not change under work already queued that reads it
    hipError_t e = hipStreamSynchronize(g_stream);
    if (e != hipSuccess) { release(); return fail((int)e, "hipStreamSynchronize: %s", hipGetErrorString(e)); }
    // the new host table is completed and copied first; the model's table and the old device tables change only once that succeeded
    ForcingTable h = m->forcing_h;
    h.nterms[field] = nterms;
    for (int q = 0; q < OCN_MAX_FORCING_TERMS; ++q) {
        ForcingTerm &d = h.t[field][q];
        d = ForcingTerm{};
        if (q >= nterms) continue;
        const ocn_forcing_t &t = terms[q];
        d.kind = t.kind;                                    // OCN_FORCING_FUNCTION: the function is FfTable::fn_of[field][q]
        d.array = t.kind == OCN_FORCING_ARRAY ? t.array : nullptr;
        d.mask_dir = t.kind == OCN_FORCING_RELAXATION ? t.mask_dir : -1;
        d.target_dir = t.kind == OCN_FORCING_RELAXATION ? t.target_dir : -1;
        d.rate_mask = t.rate_mask; d.target = t.target;
        d.mask_table = dev[q][0]; d.target_table = dev[q][1];
    }
    for (int f = 0; f < m->nf; ++f) {
        h.r[f] = default_range(g, m->loc[f], f < 3);
        const FView v = make_view(g, nullptr, m->loc[f]);
        h.s1[f] = v.s1; h.s2[f] = v.s2; h.off[f] = v.off;
    }
    const FView a = make_view(g, nullptr, LOC_C);
    h.as1 = a.s1; h.as2 = a.s2; h.aoff = a.off;
    // the functions of the other fields stay, this field's are replaced by the new ones; fn_of follows
    auto nf = std::make_unique<FfTable>();
    *nf = FfTable{};
    for (int q = 0; q < m->ff.h.n; ++q)
        if (m->ff.h.fn[q].field != field) nf->fn[nf->n++] = m->ff.h.fn[q];
    for (int q = 0; q < nmade; ++q) nf->fn[nf->n++] = made[q];
    memset(nf->fn_of, -1, sizeof(nf->fn_of));
    for (int q = 0; q < nf->n; ++q) nf->fn_of[nf->fn[q].field][nf->fn[q].term] = (signed char)q;
    if (nf->n > 0 && !m->ff.d) {
        e = dev_alloc((void **)&m->ff.d, sizeof(FfTable));
        if (e != hipSuccess) { m->ff.d = nullptr; release(); return fail((int)e, "dev_alloc(forcing function table): %s", hipGetErrorString(e)); }
    }
    if (m->ff.d) e = hipMemcpy(m->ff.d, nf.get(), sizeof(FfTable), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->forcing_d, &h, sizeof(ForcingTable), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        // the device copies may be partial: try to restore the previous tables (whose tables are still allocated) before reporting
        (void)hipMemcpy(m->forcing_d, &m->forcing_h, sizeof(ForcingTable), hipMemcpyHostToDevice);
        if (m->ff.d) (void)hipMemcpy(m->ff.d, &m->ff.h, sizeof(FfTable), hipMemcpyHostToDevice);
        release();
        return fail((int)e, "forcing table: %s", hipGetErrorString(e));
    }
    m->forcing_h = h;
    for (int q = 0; q < m->ff.h.n; ++q)
        if (m->ff.h.fn[q].field == field) hipFree(m->ff.h.fn[q].tab);
    m->ff.h = *nf;
    m->ff.reads_time = false; m->ff.cell_max = m->ff.ins_max = 0; m->ff.Lmax = 1; m->ff.cell_arith = m->ff.ins_arith = true;
    for (int q = 0; q < nf->n; ++q) {
        const FfFunction &fn = nf->fn[q];
        m->ff.reads_time = m->ff.reads_time || fn.reads_time;
        m->ff.cell_arith = m->ff.cell_arith && ff_arithmetic_only(fn.cell, fn.n_cell); m->ff.ins_arith = m->ff.ins_arith && ff_arithmetic_only(fn.ins, fn.n);
        m->ff.cell_max = std::max(m->ff.cell_max, fn.n_cell); m->ff.ins_max = std::max(m->ff.ins_max, fn.n);
        m->ff.Lmax = std::max(m->ff.Lmax, std::max(fn.L[0], std::max(fn.L[1], fn.L[2])));
    }
    for (int q = 0; q < OCN_MAX_FORCING_TERMS; ++q)
        for (int w = 0; w < 2; ++w) { hipFree(m->forcing_tables[field][q][w]); m->forcing_tables[field][q][w] = dev[q][w]; }
    m->epoch += 1;                  // a captured time-step graph launches other kernels now
    // the tables of the new functions, once everything above is settled: those of programs that do not read t are filled here and never again
    if (nmade > 0) {
        ff_launch_lines(m->ff.d, m->ff.h.n, m->ff.Lmax, m->time, false);
        KERNEL_CHECK();
    }
    return OCN_OK;
}

// closure = AnisotropicMinimumDissipation(Cν = Cnu, Cκ = Ckappa[tracer]; Cb = nothing); replaces any other closure
extern "C" int ocn_model_set_amd(ocn_model_t m, double Cnu, const double *Ckappa) {
    if (m) m->epoch += 1;
    NEED_INIT();
    if (!m || (m->ntr > 0 && !Ckappa)) return fail(OCN_EINVAL, "NULL argument");
    if (int rc_ = refuse_immersed(m->grid, "AnisotropicMinimumDissipation")) return rc_;
    const DGrid &g = m->grid->d;
    if (g.tx == OCN_FLAT || g.ty == OCN_FLAT || g.tz == OCN_FLAT)
        return fail(OCN_ENOTSUP, "AnisotropicMinimumDissipation needs a grid without Flat directions");
    int rc = alloc_parent_zeroed(m->grid, LOC_C, &m->nu_e);
    for (int t = 0; t < m->ntr && !rc; ++t) rc = alloc_parent_zeroed(m->grid, LOC_C, &m->kappa_e[t]);
    if (rc) return rc;
    Closure c;
    c.kind = Closure::AMD;
    c.Cnu = Cnu;
    for (int t = 0; t < m->ntr; ++t) c.Ckappa[t] = Ckappa[t];
    m->closure = c;
    return OCN_OK;
}

// closure = Smagorinsky(coefficient = C, Pr) (lilly = 0) | SmagorinskyLilly(C, Cb, Pr) (smagorinsky.jl:62-83, lilly_coefficient.jl); replaces
// any other closure. The buoyancy of the Lilly coefficient is what ocn_model_set_buoyancy says when a step runs.
extern "C" int ocn_model_set_smagorinsky(ocn_model_t m, double C, double Cb, int lilly, const double *Pr) {
    if (m) m->epoch += 1;
    NEED_INIT();
    if (!m || (m->ntr > 0 && !Pr)) return fail(OCN_EINVAL, "NULL argument");
    if (int rc_ = refuse_immersed(m->grid, "Smagorinsky")) return rc_;
    const DGrid &g = m->grid->d;
    if (g.tx == OCN_FLAT || g.ty == OCN_FLAT || g.tz == OCN_FLAT) return fail(OCN_EINVAL, "Smagorinsky needs a grid without Flat directions");
    if (!(C >= 0)) return fail(OCN_EINVAL, "the Smagorinsky coefficient must be non-negative");
    for (int t = 0; t < m->ntr; ++t)
        if (!(Pr[t] > 0)) return fail(OCN_EINVAL, "the Prandtl number must be positive");
    int rc = alloc_parent_zeroed(m->grid, LOC_C, &m->nu_e);
    if (rc) return rc;
    Closure c;
    c.kind = Closure::SMAGORINSKY;
    c.C = C; c.Cb = Cb; c.lilly = lilly != 0;
    for (int t = 0; t < m->ntr; ++t) c.Pr[t] = Pr[t];
    m->closure = c;
    return OCN_OK;
}

// closure = Smagorinsky(coefficient = DynamicCoefficient(averaging, schedule = IterationInterval(interval, offset), minimum_numerator), Pr)
// (dynamic_coefficient.jl:114-117, smagorinsky.jl:62-66); replaces any other closure. Every coefficient field and the scratch of the filtered
// velocities is allocated here, and the reductions' partial-result slab is grown here, so that a step allocates nothing.
extern "C" int ocn_model_set_dynamic_smagorinsky(ocn_model_t m, int averaging_mask, double minimum_numerator, int64_t interval, int64_t offset,
                                                 const double *Pr) {
    if (m) m->epoch += 1;
    NEED_INIT();
    if (!m || (m->ntr > 0 && !Pr)) return fail(OCN_EINVAL, "NULL argument");
    if (int rc_ = refuse_immersed(m->grid, "DynamicSmagorinsky")) return rc_;
    if (m->dm) return fail(OCN_ENOTSUP, "a dynamic Smagorinsky coefficient is not built for a partitioned model");
    if (averaging_mask < 0 || averaging_mask > 7) return fail(OCN_EINVAL, "averaging_mask %d: bits 0..2 name the averaged directions, 0 is LagrangianAveraging", averaging_mask);
    if (interval < 1) return fail(OCN_EINVAL, "the interval of the schedule must be positive");
    if (minimum_numerator != minimum_numerator) return fail(OCN_EINVAL, "minimum_numerator is NaN");
    for (int t = 0; t < m->ntr; ++t)
        if (!(Pr[t] > 0)) return fail(OCN_EINVAL, "the Prandtl number must be positive");
    int rc = dynamic_smagorinsky_check_grid(m->grid, averaging_mask);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(g_stream));          // a launch already queued may still read the fields of the closure that leaves
    dynamic_fields_free(m->dyn);
    DynFields &F = m->dyn;
    rc = alloc_parent_zeroed(m->grid, LOC_C, &m->nu_e);
    double **full[] = {&F.Sigma, &F.Sigma_bar};
    for (double **p : full)
        if (!rc) rc = alloc_parent_zeroed(m->grid, LOC_C, p);
    if (!rc) rc = alloc_parent_zeroed(m->grid, LOC_U, &F.ub);
    if (!rc) rc = alloc_parent_zeroed(m->grid, LOC_V, &F.vb);
    if (!rc) rc = alloc_parent_zeroed(m->grid, LOC_W, &F.wb);
    if (!rc && averaging_mask == 0) {
        double **lag[] = {&F.J_LM, &F.J_MM, &F.J_LM_prev, &F.J_MM_prev};
        for (double **p : lag)
            if (!rc) rc = alloc_parent_zeroed(m->grid, LOC_C, p);
        if (!rc && dev_alloc((void **)&F.mean, 2 * sizeof(double)) != hipSuccess) rc = fail(OCN_ESTATE, "dev_alloc(means)");
        // (the slab of the two full means)
        if (!rc) rc = dynamic_average(m->grid, F.J_LM, 7, false, F.mean);
    } else if (!rc) {
        rc = alloc_parent_zeroed(m->grid, LOC_C, &F.LM);
        if (!rc) rc = alloc_parent_zeroed(m->grid, LOC_C, &F.MM);
        // the reduced fields: the parent extent along every kept direction, one point along an averaged one
        int P[3];
        parent_size(m->grid->d, LOC_C, P);
        size_t n = 1;
        for (int d = 0; d < 3; ++d) n *= ((averaging_mask >> d) & 1) ? 1 : (size_t)P[d];
        double **red[] = {&F.J_LM, &F.J_MM};
        for (double **p : red) {
            if (rc) break;
            if (dev_alloc((void **)p, n * sizeof(double)) != hipSuccess) { *p = nullptr; rc = fail(OCN_ESTATE, "dev_alloc(reduced field)"); }
            else if (hipMemsetAsync(*p, 0, n * sizeof(double), g_stream) != hipSuccess) rc = fail(OCN_ESTATE, "hipMemset(reduced field)");
        }
        if (!rc) rc = dynamic_average(m->grid, F.LM, averaging_mask, true, F.J_LM);
    }
    if (rc) {
        dynamic_fields_free(m->dyn);
        if (m->closure.dynamic) m->closure = Closure();          // its fields are gone
        return rc;
    }
    Closure c;
    c.kind = Closure::SMAGORINSKY;
    c.dynamic = true;
    c.averaging_mask = averaging_mask; c.minimum_numerator = minimum_numerator; c.interval = interval; c.offset = offset;
    for (int t = 0; t < m->ntr; ++t) c.Pr[t] = Pr[t];
    m->closure = c;
    m->dyn_previous_time = m->time;
    m->dyn_uninitialised = true;
    return OCN_OK;
}

// the device-resident table of the model's programs, after the host copy changed (never inside a captured step)
static int bf_upload(ocn_model_s *m) {
    auto &B = m->bf;
    B.reads_time = false;
    for (int q = 0; q < B.n; ++q)
        for (int w = 0; w < B.slot[q].fn.n; ++w) B.reads_time = B.reads_time || B.slot[q].fn.ins[w].op == OCN_EXPR_TIME;
    if (B.n == 0) return OCN_OK;
    HIP_TRY(hipStreamSynchronize(g_stream));          // a launch already queued still reads the table as it was
    if (!B.table_d) HIP_TRY(dev_alloc((void **)&B.table_d, sizeof(BfFunction) * BF_MAX_FUNCTIONS));
    BfFunction h[BF_MAX_FUNCTIONS];
    for (int q = 0; q < B.n; ++q) h[q] = B.slot[q].fn;
    HIP_TRY(hipMemcpy(B.table_d, h, sizeof(BfFunction) * (size_t)B.n, hipMemcpyHostToDevice));
    return OCN_OK;
}

// the function of side `side` of field f leaves (another condition replaces it): its array is freed; the caller sets the side's condition
static int bf_remove(ocn_model_s *m, int f, int side) {
    auto &B = m->bf;
    for (int q = 0; q < B.n; ++q)
        if (B.slot[q].f == f && B.slot[q].side == side) {
            HIP_TRY(hipStreamSynchronize(g_stream));
            hipFree(B.slot[q].fn.out);
            for (int w = q; w + 1 < B.n; ++w) B.slot[w] = B.slot[w + 1];
            B.n -= 1;
            if (m->bcs[f][side].kind == OCN_BC_FLUX) m->bcs[f][side].array = nullptr;
            return bf_upload(m);
        }
    return OCN_OK;
}

// name.side = FluxBoundaryCondition(func, field_dependencies = dep_names, ...) with the program of func
extern "C" int ocn_model_set_flux_bc_function(ocn_model_t m, const char *name, int side, const ocn_expr_ins_t *program, int n,
                                              const char *const *dep_names, int ndeps) {
    NEED_INIT();
    if (m) m->epoch += 1;
    if (!m || !name) return fail(OCN_EINVAL, "NULL argument");
    if (m->dm) return fail(OCN_ENOTSUP, "boundary functions are not served on a partitioned model");
    const int f = field_index(m, name);
    if (f < 0) return fail(OCN_EINVAL, "name %s not found in model.velocities or model.tracers.", name);
    bool reads_time;
    int rc = bf_validate_program(program, n, ndeps, &reads_time);
    if (rc) return rc;
    if (ndeps > 0 && !dep_names) return fail(OCN_EINVAL, "NULL dependency names");
    int dep_field[BF_MAX_DEPS], dep_locs[BF_MAX_DEPS][3];
    for (int s = 0; s < ndeps; ++s) {
        dep_field[s] = dep_names[s] ? field_index(m, dep_names[s]) : -1;
        if (dep_field[s] < 0) return fail(OCN_EINVAL, "name %s not found in model.velocities or model.tracers.", dep_names[s] ? dep_names[s] : "(NULL)");
        memcpy(dep_locs[s], m->loc[dep_field[s]], sizeof(int) * 3);
    }
    if ((rc = validate_bc(m->grid->d, m->loc[f], side, OCN_BC_FLUX))) return rc;
    BfFunction fn;
    if ((rc = bf_make_function(m->grid, program, n, m->loc[f], side, dep_field, dep_locs, ndeps, nullptr, &fn))) return rc;
    auto &B = m->bf;
    int q = 0;
    while (q < B.n && !(B.slot[q].f == f && B.slot[q].side == side)) ++q;
    if (q == BF_MAX_FUNCTIONS) return fail(OCN_EINVAL, "a model carries at most %d boundary functions", BF_MAX_FUNCTIONS);
    if (q < B.n) fn.out = B.slot[q].fn.out;          // the side had a function: its array stays (the extents are the side's)
    else {
        const size_t bytes = sizeof(double) * (size_t)fn.Na * fn.Nb;
        HIP_TRY(dev_alloc((void **)&fn.out, bytes));
        HIP_TRY(hipMemsetAsync(fn.out, 0, bytes, g_stream));
        B.n += 1;
    }
    B.slot[q].f = f; B.slot[q].side = side; B.slot[q].fn = fn;
    m->bcs[f][side].kind = OCN_BC_FLUX; m->bcs[f][side].value = 0.0; m->bcs[f][side].array = fn.out;
    m->any_bc = m->any_flux_bc = true;
    m->lin[f][side].on = false;                 // the function replaces a linear field-dependent condition on this side
    m->any_linear_flux = false;
    for (int a = 0; a < m->nf; ++a)
        for (int sd = 0; sd < 6; ++sd) m->any_linear_flux = m->any_linear_flux || m->lin[a][sd].on;
    return bf_upload(m);
}

extern "C" int ocn_model_boundary_function_values(ocn_model_t m, const char *name, int side, double *host_out) {
    NEED_INIT();
    if (!m || !name || !host_out) return fail(OCN_EINVAL, "NULL argument");
    const int f = field_index(m, name);
    for (int q = 0; q < m->bf.n; ++q)
        if (m->bf.slot[q].f == f && m->bf.slot[q].side == side) {
            const BfFunction &fn = m->bf.slot[q].fn;
            return ocn_memcpy_d2h(host_out, fn.out, sizeof(double) * (size_t)fn.Na * fn.Nb);
        }
    return fail(OCN_EINVAL, "%s carries no boundary function on side %d", name, side);
}

static int model_set_bc(ocn_model_t m, const char *name, int side, int kind, double value, const double *array) {
    if (m) m->epoch += 1;
    if (!m || !name) return fail(OCN_EINVAL, "NULL argument");
    // the diffusivity fields of an LES closure carry boundary conditions too (anisotropic_minimum_dissipation.jl:339-352: νₑ, κₑ are
    // CenterFields built with the conditions the user passes as boundary_conditions = (νₑ = ..., κₑ = (b = ...,))); their halos are
    // filled with them after compute_diffusivities!
    if (!strcmp(name, "nu_e") || (!strncmp(name, "kappa_e", 7) && name[7] >= '0' && name[7] <= '9' && !name[8])) {
        const int q = name[0] == 'n' ? 0 : 1 + (name[7] - '0');
        if (q > 0 && m->closure.kind == Closure::SMAGORINSKY) return fail(OCN_ESTATE, "a Smagorinsky closure has the eddy viscosity nu_e only");
        if (q > m->ntr) return fail(OCN_EINVAL, "no tracer %d", q - 1);
        if (kind == OCN_BC_FLUX || kind == OCN_BC_OPEN) return fail(OCN_EINVAL, "a diffusivity field takes Value or Gradient conditions");
        int rcq = validate_bc(m->grid->d, LOC_C, side, kind);
        if (rcq) return rcq;
        m->kbcs[q][side].kind = kind;
        m->kbcs[q][side].value = value;
        m->kbcs[q][side].array = array;
        m->any_kbc = false;
        for (int a = 0; a <= m->ntr; ++a)
            for (int sd = 0; sd < 6; ++sd) m->any_kbc = m->any_kbc || m->kbcs[a][sd].kind != OCN_BC_DEFAULT;
        return OCN_OK;
    }
    const int f = field_index(m, name);
    if (f < 0) return fail(OCN_EINVAL, "boundary conditions can be set on u, v, w and the tracers c0..c%d; got '%s'", m->ntr - 1, name);
    int rc = validate_bc(m->grid->d, m->loc[f], side, kind);
    if (rc) return rc;
    if (array && kind == OCN_BC_DEFAULT) return fail(OCN_EINVAL, "an array-valued condition needs a classification (Flux, Value, Gradient, Open)");
    if ((rc = bf_remove(m, f, side))) return rc;        // a plain condition replaces a function on this side
    m->bcs[f][side].kind = kind;
    m->bcs[f][side].value = value;
    m->bcs[f][side].array = array;
    if (kind != OCN_BC_OPEN && f < 3 && side / 2 == f && m->ob[side].on) { m->ob[side].on = false; m->n_scheme -= 1; }   // the scheme belongs to an Open condition
    m->lin[f][side].on = false;                 // a plain condition replaces a field-dependent one on this side
    m->any_linear_flux = false;
    for (int q = 0; q < m->nf; ++q)
        for (int sd = 0; sd < 6; ++sd) m->any_linear_flux = m->any_linear_flux || m->lin[q][sd].on;
    m->any_bc = m->any_flux_bc = false;
    for (int q = 0; q < m->nf; ++q)
        for (int sd = 0; sd < 6; ++sd) {
            if (m->bcs[q][sd].kind != OCN_BC_DEFAULT) m->any_bc = true;
            if (m->bcs[q][sd].kind == OCN_BC_FLUX && (m->bcs[q][sd].value != 0.0 || m->bcs[q][sd].array)) m->any_flux_bc = true;
        }
    return OCN_OK;
}

extern "C" int ocn_model_set_boundary_condition(ocn_model_t m, const char *name, int side, int kind, double value) {
    return model_set_bc(m, name, side, kind, value, nullptr);
}

// the same with an array-valued condition (getbc(condition::AbstractArray, i, j, grid, args...) = condition[i, j], boundary_condition.jl:164)
extern "C" int ocn_model_set_boundary_condition_array(ocn_model_t m, const char *name, int side, int kind, const double *device_array) {
    if (!device_array) return fail(OCN_EINVAL, "NULL array");
    return model_set_bc(m, name, side, kind, 0.0, device_array);
}

// name.side = OpenBoundaryCondition(value; scheme = PerturbationAdvection(inflow_timescale, outflow_timescale)) (perturbation_advection.jl:57-63)
extern "C" int ocn_model_set_open_boundary_scheme(ocn_model_t m, const char *name, int side, int enabled, double inflow_timescale,
                                                  double outflow_timescale) {
    if (m) m->epoch += 1;
    NEED_INIT();
    if (!m || !name) return fail(OCN_EINVAL, "NULL argument");
    if (int rc_ = refuse_immersed(m->grid, "an OpenBoundaryCondition with a scheme")) return rc_;
    if (m->dm) return fail(OCN_ENOTSUP, "open boundaries with a scheme are not served on a partitioned model");
    const int f = field_index(m, name);
    if (side < 0 || side > 5 || f < 0 || f > 2 || side / 2 != f || !ob_wall(m->grid->d, side))
        return fail(OCN_EINVAL, "a scheme belongs to the wall-normal velocity of a Bounded direction (u west / east, v south / north, w bottom / top)");
    if (m->bcs[f][side].kind != OCN_BC_OPEN) return fail(OCN_EINVAL, "a scheme belongs to an Open condition: set the side's condition first");
    if (enabled && (!(inflow_timescale >= 0) || !(outflow_timescale >= 0))) return fail(OCN_EINVAL, "the timescales must be non-negative");
    if (enabled) {
        int rc = ob_partial_buffer(m->grid);
        if (rc) return rc;
        for (int sd = 0; sd < 6; ++sd) m->ob_area[sd] = ob_wall(m->grid->d, sd) ? ob_face_area(m->grid, sd) : 0.0;
    }
    m->ob[side].on = enabled != 0;
    m->ob[side].tin = inflow_timescale;
    m->ob[side].tout = outflow_timescale;
    m->n_scheme = 0;
    for (int sd = 0; sd < 6; ++sd) m->n_scheme += m->ob[sd].on ? 1 : 0;
    return OCN_OK;
}

extern "C" int ocn_model_update_state(ocn_model_t m, int compute_tendencies_flag) {
    NEED_INIT();
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    return update_state(m, compute_tendencies_flag != 0);
}

extern "C" int ocn_model_set_finalize(ocn_model_t m, int enforce_incompressibility) {
    NEED_INIT();
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    int rc = fill_open_boundaries(m, m->nf, false);     // set!(ϕ, value); fill_halo_regions!(ϕ, model.clock, fields(model)) per field
    if (rc) return rc;
    // "Apply a mask" (set_nonhydrostatic_model.jl:47-49): tracers, then velocities, before update_state!
    if ((rc = mask_immersed_fields(m->grid, m->U + 3, m->loc + 3, m->ntr, 0.0))) return rc;
    if ((rc = mask_immersed_fields(m->grid, m->U, m->loc, 3, 0.0))) return rc;
    if ((rc = update_state(m, false))) return rc;
    if (enforce_incompressibility) {
        if ((rc = pressure_step(m, 1.0, false))) return rc;
        if ((rc = update_state(m, false))) return rc;
    }
    return OCN_OK;
}

static void tick(ocn_model_s *m, double dt, bool stage) {       // clock.jl:128-143
    m->time += dt;
    if (stage) { m->stage += 1; m->last_stage_dt = dt; }
    else { m->iteration += 1; m->stage = 1; m->last_dt = dt; m->last_stage_dt = dt; }
}

// cache_previous_tendencies! (store_tendencies.jl:12-22). G⁻ <- Gⁿ followed by a full recomputation of Gⁿ is a
// pointer swap on this architecture: cells the tendency kernels never write (halos, excluded periphery) are zero in
// both buffers for the model's lifetime.
static int cache_previous_tendencies(ocn_model_s *m) {
    if (m->opt.swap_tendencies) {
        for (int f = 0; f < m->nf; ++f) std::swap(m->Gn[f], m->Gm[f]);
        return OCN_OK;
    }
    SubstepArgs a;
    int nx, ny, nz;
    int rc = fill_substep_args(m->grid->d, a, m->Gm, m->Gn, nullptr, m->loc, m->nf, false, &nx, &ny, &nz);
    if (rc) return rc;
    hipLaunchKernelGGL(cache_tendencies_kernel, grid3(nx, ny, nz * m->nf, BLK), BLK, 0, g_stream, a);
    KERNEL_CHECK();
    return OCN_OK;
}

// step_lagrangian_particles!(model, Δt) (LagrangianParticleTracking.jl:138-149), after a stage's update_state!: one launch, none without
// particles. It reads m->U -- the stage's corrected, halo-filled fields -- so where the next substep rode in the tendency launch (it wrote
// U2) the call comes BEFORE the two sets swap. The total velocities are the ones update_state! has just formed.
static int step_particles(ocn_model_s *m, double dt) {
    const Particles &P = m->particles;
    if (!P.on || P.n == 0) return OCN_OK;
    const DGrid &g = m->grid->d;
    ParticleStepArgs a = {};
    a.n = P.n; a.x = P.x; a.y = P.y; a.z = P.z; a.depths = P.depths; a.restitution = P.restitution; a.dt = dt; a.advect = 1;
    a.u = make_view(g, total_velocity(m, 0), LOC_U); a.v = make_view(g, total_velocity(m, 1), LOC_V); a.w = make_view(g, total_velocity(m, 2), LOC_W);
    a.ntracked = P.ntracked;
    for (int q = 0; q < P.ntracked; ++q) {
        const double *field = *P.tracked[q].slot;
        if (!field) return fail(OCN_ESTATE, "the tracked field %s does not exist any more", P.tracked[q].field);
        a.tracked[q] = TrackedField{make_view(g, field, P.tracked[q].loc), loc_bits(P.tracked[q].loc), P.tracked[q].values};
    }
    return launch_particles(m->grid->pg, a);
}

// time_step!(model::AbstractModel{<:RungeKutta3TimeStepper}, Δt) (TimeSteppers/runge_kutta_3.jl:93-170)
static int rk3_time_step(ocn_model_s *m, double dt) {
    const DGrid &g = m->grid->d;
    int rc;
    if (m->iteration == 0 && (rc = update_state(m, true))) return rc;
    const double g1 = OCN_RK3_G1, g2 = OCN_RK3_G2, g3 = OCN_RK3_G3, z2 = OCN_RK3_Z2, z3 = OCN_RK3_Z3;
    const double dt1 = dt * g1, dt2 = dt * (g2 + z2), dt3 = dt * (g3 + z3);
    const double tn1 = m->time + dt;
    const double gam[3] = {g1, g2, g3}, zet[3] = {0.0, z2, z3}, sdt[3] = {dt1, dt2, dt3};
    // stages 2 and 3: rk3_substep! fused into the tendency evaluation that precedes it (the cell's new tendency and its
    // previous one are at hand when the cell is closed) -- possible when the fused kernel runs, tendencies are cached by
    // pointer swap and no Flux boundary condition is added to G after the kernel
    const bool can_fuse = plan(m).fuse_substep;
    // triply periodic grids: the first substep rides in the pressure step's source-term and correction kernels, and the correction kernel
    // of every stage leaves all halos current, so the update_state! that follows fills none (pressure_step)
    const bool fuse_stage1 = can_fuse_stage1_source(m), fold = can_fold_halo_fill(m);
    const PendingSubstep stage1{dt, g1};
    m->stage1_source_fused = fuse_stage1;
    m->halo_fill_folded = fold;
    bool substep_done = false;
    for (int stage = 0; stage < 3; ++stage) {
        const bool pending = stage == 0 && fuse_stage1;
        if (!substep_done && (rc = compute_flux_bc_tendencies(m))) return rc;
        if (!substep_done && !pending && (rc = rk3_substep(g, m->U, m->Gn, m->Gm, m->loc, m->nf, dt, gam[stage], zet[stage], stage > 0))) return rc;
        substep_done = false;
        if ((rc = implicit_step(m, sdt[stage]))) return rc;          // after the substep -- on its own or ridden in the tendency launch -- and before tick!
        if (stage < 2) tick(m, sdt[stage], true);
        else {
            double corrected = tn1 - m->time;
            tick(m, dt3, false);
            m->last_stage_dt = corrected;
            m->last_dt = dt;
        }
        if ((rc = pressure_step(m, sdt[stage], true, stage == 2, pending ? &stage1 : nullptr, fold))) return rc;
        if (stage < 2 && (rc = cache_previous_tendencies(m))) return rc;
        if (stage < 2 && can_fuse) {
            FusedSubstep sub{m->U2, m->Gm, dt, gam[stage + 1], zet[stage + 1], 1};
            sub.store_G = stage != 1 || !m->opt.skip_dead_tendency_store;        // G(U²): read by the third stage's substep only
            if ((rc = update_state(m, true, &sub, fold))) return rc;
            if ((rc = step_particles(m, sdt[stage]))) return rc;         // before the swap: the particles see this stage's fields
            for (int f = 0; f < m->nf; ++f) std::swap(m->U[f], m->U2[f]);
            if (m->n_scheme && (rc = carry_open_boundaries(m))) return rc;
            substep_done = true;
        } else {
            if ((rc = update_state(m, true, nullptr, fold))) return rc;
            if ((rc = step_particles(m, sdt[stage]))) return rc;         // runge_kutta_3.jl:128,144,167: the third with (γ³ + ζ³)Δt
        }
    }
    return OCN_OK;
}

struct ClockState { double time, last_dt, last_stage_dt; int64_t iteration; int stage; };
static ClockState save_clock(const ocn_model_s *m) { return {m->time, m->last_dt, m->last_stage_dt, m->iteration, m->stage}; }
static void restore_clock(ocn_model_s *m, const ClockState &c) {
    m->time = c.time; m->last_dt = c.last_dt; m->last_stage_dt = c.last_stage_dt; m->iteration = c.iteration; m->stage = c.stage;
}

extern "C" int ocn_model_time_step(ocn_model_t m, double dt) {
    NEED_INIT();
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    // graphs: not on the first step (it also evaluates the initial tendencies), not while tendency launches are being timed, and only
    // on a stream the library owns (a borrowed stream may be the legacy default stream, which cannot be captured)
    if (m->dm) {
        // a step that fails after make_pressure_correction! has started the halo exchange of the coming update_state! must not leave that
        // exchange "in flight": the next call would report it instead of the original error
        const int rc = rk3_time_step(m, dt);
        if (rc) dist_abandon_exchange(m);
        return rc;
    }
    // ... and not with a scheme side: the boundary step takes last_stage_Δt, whose corrected third-stage value changes from step to step
    // ... nor with a boundary function or a forcing function that reads t: the time is an argument of its launch
    // ... nor with a dynamic Smagorinsky coefficient: whether an update runs, which branch it takes and its Δt are decided on the host
    if (!m->opt.use_graph || m->profile || m->iteration == 0 || !g_stream_owned || m->n_scheme || m->bf.reads_time || m->ff.reads_time ||
        m->closure.dynamic)
        return rk3_time_step(m, dt);
    if (m->graph_exec && m->graph_dt == dt && m->graph_epoch == m->epoch * 1000003ull + g_epoch) {
        hipError_t e = hipGraphLaunch(m->graph_exec, g_stream);
        if (e != hipSuccess) return fail((int)e, "hipGraphLaunch: %s", hipGetErrorString(e));
        // the host side of the step: the clock (tick! x 3, runge_kutta_3.jl:120-168)
        const double dt1 = dt * OCN_RK3_G1, dt2 = dt * (OCN_RK3_G2 + OCN_RK3_Z2), dt3 = dt * (OCN_RK3_G3 + OCN_RK3_Z3);
        const double tn1 = m->time + dt;
        tick(m, dt1, true);
        tick(m, dt2, true);
        const double corrected = tn1 - m->time;
        tick(m, dt3, false);
        m->last_stage_dt = corrected;
        m->last_dt = dt;
        m->graph_replays += 1;
        return OCN_OK;
    }
    if (m->graph_failures >= 2) return rk3_time_step(m, dt);          // capture does not work here: stop trying
    if (m->graph_exec) { hipGraphExecDestroy(m->graph_exec); m->graph_exec = nullptr; }
    const ClockState before = save_clock(m);
    double *U0[OCN_MAX_FIELDS], *G0[OCN_MAX_FIELDS];
    for (int f = 0; f < m->nf; ++f) { U0[f] = m->U[f]; G0[f] = m->Gn[f]; }
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(g_stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { (void)hipGetLastError(); m->graph_failures += 1; return rk3_time_step(m, dt); }
    int rc = rk3_time_step(m, dt);
    e = hipStreamEndCapture(g_stream, &graph);
    bool same = true;                           // a step must leave every pointer where it found it, or a replay would be wrong
    for (int f = 0; f < m->nf; ++f) same = same && U0[f] == m->U[f] && G0[f] == m->Gn[f];
    if (rc == OCN_OK && e == hipSuccess && graph && same) e = hipGraphInstantiate(&m->graph_exec, graph, nullptr, nullptr, 0);
    if (graph) hipGraphDestroy(graph);
    if (rc != OCN_OK || e != hipSuccess || !m->graph_exec || !same) {
        // nothing ran on the GPU during the capture: undo the host side and take the step the ordinary way
        (void)hipGetLastError();
        if (m->graph_exec) { hipGraphExecDestroy(m->graph_exec); m->graph_exec = nullptr; }
        restore_clock(m, before);
        for (int f = 0; f < m->nf; ++f) {
            if (m->U[f] != U0[f]) std::swap(m->U[f], m->U2[f]);
            if (m->Gn[f] != G0[f]) std::swap(m->Gn[f], m->Gm[f]);
        }
        m->graph_failures += 1;
        return rk3_time_step(m, dt);
    }
    m->graph_dt = dt; m->graph_epoch = m->epoch * 1000003ull + g_epoch; m->graph_captures += 1;
    e = hipGraphLaunch(m->graph_exec, g_stream);            // the captured step itself (its host side already happened above)
    if (e != hipSuccess) return fail((int)e, "hipGraphLaunch: %s", hipGetErrorString(e));
    return OCN_OK;
}

// time_step!(model::AbstractModel{<:QuasiAdamsBashforth2TimeStepper}, Δt; euler) (TimeSteppers/quasi_adams_bashforth_2.jl:74-123)
extern "C" int ocn_model_time_step_ab2(ocn_model_t m, double dt, double chi, int euler) {
    NEED_INIT();
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    const DGrid &g = m->grid->d;
    int rc;
    if (m->iteration == 0 && (rc = update_state(m, true))) return rc;
    const bool eul = euler != 0 || dt != m->last_dt;            // Δt changed, or first step (last_Δt = Inf)
    const double x = eul ? -0.5 : chi;
    if ((rc = compute_flux_bc_tendencies(m))) return rc;                                   // quasi_adams_bashforth_2.jl:99
    if ((rc = ab2_step(g, m->U, m->Gn, m->Gm, m->loc, m->nf, dt, x))) return rc;
    if ((rc = implicit_step(m, dt))) return rc;                                            // quasi_adams_bashforth_2.jl:143-151
    tick(m, dt, false);
    const bool fold = can_fold_halo_fill(m);
    m->stage1_source_fused = false;
    m->halo_fill_folded = fold;
    if ((rc = pressure_step(m, dt, true, true, nullptr, fold))) return rc;
    if ((rc = cache_previous_tendencies(m))) return rc;
    if ((rc = update_state(m, true, nullptr, fold))) return rc;
    return step_particles(m, dt);                                                          // quasi_adams_bashforth_2.jl:108
}

// reset!(model.clock) + reset!(model.timestepper) (TimeSteppers/clock.jl reset!, runge_kutta_3.jl / quasi_adams_bashforth_2.jl reset!):
// time 0, iteration 0, stage 1, last Δt = Inf, both tendency sets zero
extern "C" int ocn_model_reset(ocn_model_t m) {
    NEED_INIT();
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    m->time = 0; m->iteration = 0; m->stage = 1; m->last_dt = INFINITY; m->last_stage_dt = INFINITY;
    m->dyn_previous_time = 0.0;            // (a dynamic Smagorinsky coefficient starts again, as after ocn_model_set_clock)
    m->dyn_uninitialised = true;
    const DGrid &g = m->grid->d;
    for (int f = 0; f < m->nf; ++f) {
        int P[3];
        parent_size(g, m->loc[f], P);
        const size_t bytes = (size_t)P[0] * P[1] * P[2] * sizeof(double);
        HIP_TRY(hipMemsetAsync(m->Gn[f], 0, bytes, g_stream));
        HIP_TRY(hipMemsetAsync(m->Gm[f], 0, bytes, g_stream));
    }
    return OCN_OK;
}

extern "C" int ocn_model_clock(ocn_model_t m, double *time, int64_t *iteration, int *stage, double *last_dt, double *last_stage_dt) {
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    if (time) *time = m->time;
    if (iteration) *iteration = m->iteration;
    if (stage) *stage = m->stage;
    if (last_dt) *last_dt = m->last_dt;
    if (last_stage_dt) *last_stage_dt = m->last_stage_dt;
    return OCN_OK;
}

// set!(model, checkpointed_clock) (OutputWriters/checkpointer.jl:226-229): the clock of a restored state. The caller then copies the
// checkpointed parent arrays into the model's fields and tendencies (ocn_model_field) and calls ocn_model_update_state.
extern "C" int ocn_model_set_clock(ocn_model_t m, double time, int64_t iteration, int stage, double last_dt, double last_stage_dt) {
    if (!m) return fail(OCN_EINVAL, "NULL argument");
    if (iteration < 0 || stage < 1 || stage > 3) return fail(OCN_EINVAL, "invalid clock (iteration %lld, stage %d)", (long long)iteration, stage);
    m->epoch += 1;
    m->time = time; m->iteration = iteration; m->stage = stage; m->last_dt = last_dt; m->last_stage_dt = last_stage_dt;
    // a dynamic Smagorinsky coefficient starts again from the fields the caller restores: no time has passed since "the previous call", and
    // the 𝒥 fields (not part of a checkpoint) are initialised by the next update that fires
    m->dyn_previous_time = time;
    m->dyn_uninitialised = true;
    return OCN_OK;
}

extern "C" int ocn_model_profile_read(ocn_model_t m, double *tendency_ms, int *count) {
    NEED_INIT();
    if (!m || !tendency_ms || !count) return fail(OCN_EINVAL, "NULL argument");
    HIP_TRY(hipStreamSynchronize(g_stream));
    double total = 0;
    for (size_t q = 0; q < m->events_used; ++q) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, m->events[q].first, m->events[q].second));
        total += ms;
    }
    *tendency_ms = total;
    *count = (int)m->events_used;
    m->events_used = 0;
    return OCN_OK;
}

// debug / test hook: number of significands (of 2^23) in the binade 2^(exponent) for which the fast Float32 reciprocal
// differs from the IEEE divide
#include "ocn_dist.h"

extern "C" int ocn_debug_rcp_check(int variant, int exponent, unsigned long long *mismatches) {
    NEED_INIT();
    if (!mismatches || exponent < -126 || exponent > 127) return fail(OCN_EINVAL, "invalid argument");      // every binade of normal numbers
    unsigned long long *d;
    HIP_TRY(dev_alloc((void **)&d, 8));
    HIP_TRY(hipMemsetAsync(d, 0, 8, g_stream));
    const int eb = exponent + 127;
    if (variant == 1) hipLaunchKernelGGL(rcp_check_kernel<1>, dim3((1u << 23) / 256), dim3(256), 0, g_stream, eb, d);
    else if (variant == 2) hipLaunchKernelGGL(rcp_check_kernel<2>, dim3((1u << 23) / 256), dim3(256), 0, g_stream, eb, d);
    else hipLaunchKernelGGL(rcp_check_kernel<0>, dim3((1u << 23) / 256), dim3(256), 0, g_stream, eb, d);
    HIP_TRY(hipMemcpyAsync(mismatches, d, 8, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipFree(d));
    return OCN_OK;
}

extern "C" int ocn_debug_rcp64_check(unsigned long long nsamples, int exp_lo, int exp_hi, unsigned long long seed,
                                     unsigned long long *mismatches) {
    NEED_INIT();
    if (!mismatches || exp_lo < -1022 || exp_hi > 1023 || exp_lo > exp_hi || nsamples == 0 || nsamples > (1ull << 36))
        return fail(OCN_EINVAL, "invalid argument");
    unsigned long long *d;
    HIP_TRY(dev_alloc((void **)&d, 8));
    HIP_TRY(hipMemsetAsync(d, 0, 8, g_stream));
    hipLaunchKernelGGL(rcp64_check_kernel, dim3((unsigned)((nsamples + 255) / 256)), dim3(256), 0, g_stream, nsamples, exp_lo, exp_hi, seed, d);
    HIP_TRY(hipMemcpyAsync(mismatches, d, 8, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipFree(d));
    return OCN_OK;
}

// where permute_indices! (line_gather_kernel, mode 1) / unpermute_indices! (line_scatter_kernel, mode 2) of the cosine-transform path
// send element i of a line of length N: destination[i - 1], 1-based like Solvers/index_permutations.jl:5-35
extern "C" int ocn_debug_permute_indices(int N, int backward, int *destination) {
    NEED_INIT();
    if (N < 1 || N > (1 << 20) || !destination) return fail(OCN_EINVAL, "invalid argument");
    std::vector<double2> h((size_t)N);
    for (int i = 0; i < N; ++i) h[i] = make_double2((double)(i + 1), 0.0);
    double2 *a, *b;
    HIP_TRY(dev_alloc((void **)&a, sizeof(double2) * (size_t)N));
    HIP_TRY(dev_alloc((void **)&b, sizeof(double2) * (size_t)N));
    HIP_TRY(hipMemcpyAsync(a, h.data(), sizeof(double2) * (size_t)N, hipMemcpyHostToDevice, g_stream));
    const dim3 blk(64, 4, 1), grd((N + 63) / 64, 1, 1);
    if (!backward) hipLaunchKernelGGL(line_gather_kernel, grd, blk, 0, g_stream, (const double2 *)a, b, N, 1, 1, 0, 1);
    else hipLaunchKernelGGL(line_scatter_kernel, grd, blk, 0, g_stream, (const double2 *)a, b, N, 1, 1, 0, 2);
    HIP_TRY(hipMemcpyAsync(h.data(), b, sizeof(double2) * (size_t)N, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipFree(a));
    HIP_TRY(hipFree(b));
    for (int m = 0; m < N; ++m) destination[(int)h[m].x - 1] = m + 1;      // position m holds source h[m].x
    return OCN_OK;
}

// maximum over the cells 1..Nx x 1..Ny x 1..Nz of `grid` of the inverse advective timescale |u| Δx⁻¹ + |v| Δy⁻¹ + |w| Δzᶠ⁻¹
static int max_inverse_advection_timescale(ocn_grid_t grid, const double *u, const double *v, const double *w, double *value) {
    const DGrid &g = grid->d;
    const int nb = 1024;
    double *blockmax;
    HIP_TRY(dev_alloc((void **)&blockmax, nb * sizeof(double)));
    hipLaunchKernelGGL(advection_timescale_kernel, dim3(nb), dim3(256), 0, g_stream, g, make_view(g, u, LOC_U), make_view(g, v, LOC_V),
                       make_view(g, w, LOC_W), blockmax);
    double m = 0;
    int rc = reduce_blockmax(blockmax, nb, &m);
    hipFree(blockmax);
    *value = m;
    return rc;
}

// the cells of `grid` only: on the local grid of a partitioned model this is the rank's own timescale (no model, no communicator here)
extern "C" int ocn_cell_advection_timescale(ocn_grid_t grid, const double *u, const double *v, const double *w, double *tau) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !tau) return fail(OCN_EINVAL, "NULL argument");
    double m = 0;
    int rc = max_inverse_advection_timescale(grid, u, v, w, &m);
    if (rc) return rc;
    *tau = 1.0 / m;              // Inf for a fluid at rest, like the reference's 1 / 0
    return OCN_OK;
}

// on a partitioned model the minimum over ALL ranks (the reference all-reduces, distributed_fields.jl:144-196): the MAXIMUM of the inverse
// timescale crosses the communicator before the one divide, so every rank returns the bits the serial model returns on the global grid
// (the ranks' cells 1..Nx x 1..Ny x 1..Nz tile the global ones; the wall face Nx + 1 of a LeftConnected rank carries no flow).
// Collective there: every rank of the model's communicator makes the call.
extern "C" int ocn_model_cell_advection_timescale(ocn_model_t m, double *tau) {
    NEED_INIT();
    if (!m || !tau) return fail(OCN_EINVAL, "NULL argument");
    double inv = 0;
    // cell_advection_timescale(model) uses total_velocities(model) (NonhydrostaticModels.jl:77-81): formed here from the fields as they are
    int rc = has_background_velocity(m) ? update_total_velocities(m) : OCN_OK;
    if (rc) return rc;
    rc = max_inverse_advection_timescale(m->grid, total_velocity(m, 0), total_velocity(m, 1), total_velocity(m, 2), &inv);
    if (rc) return rc;
    if (m->dm && (rc = ocn_dist_allreduce_max(m->dm->dist, &inv))) return rc;
    *tau = 1.0 / inv;
    return OCN_OK;
}

extern "C" int ocn_hasnan(const double *data, size_t n, int *result) {
    NEED_INIT();
    if (!data || !result) return fail(OCN_EINVAL, "NULL argument");
    int *flag;
    HIP_TRY(dev_alloc((void **)&flag, sizeof(int)));
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), g_stream);
    if (e == hipSuccess && n) {
        const int nb = (int)std::min<size_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(hasnan_kernel, dim3(nb), dim3(256), 0, g_stream, data, (long)n, flag);
        e = hipGetLastError();
    }
    int h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    hipFree(flag);
    if (e != hipSuccess) return fail((int)e, "hasnan: %s", hipGetErrorString(e));
    *result = h;
    return OCN_OK;
}

extern "C" int ocn_max_abs_divergence(ocn_grid_t grid, const double *u, const double *v, const double *w, double *value) {
    NEED_INIT();
    if (!grid || !u || !v || !w || !value) return fail(OCN_EINVAL, "NULL argument");
    const DGrid &g = grid->d;
    const int nb = 1024;
    double *blockmax;
    HIP_TRY(dev_alloc((void **)&blockmax, nb * sizeof(double)));
    hipLaunchKernelGGL(max_abs_div_kernel, dim3(nb), dim3(256), 0, g_stream, g, make_view(g, u, LOC_U), make_view(g, v, LOC_V),
                       make_view(g, w, LOC_W), blockmax);
    std::vector<double> h(nb);
    hipError_t e = hipMemcpyAsync(h.data(), blockmax, nb * sizeof(double), hipMemcpyDeviceToHost, g_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
    hipFree(blockmax);
    if (e != hipSuccess) return fail((int)e, "max_abs_divergence: %s", hipGetErrorString(e));
    double mx = 0;
    for (double x : h) mx = std::max(mx, x);
    *value = mx;
    return OCN_OK;
}

extern "C" int ocn_model_max_abs_divergence(ocn_model_t m, double *value) {
    NEED_INIT();
    if (!m || !value) return fail(OCN_EINVAL, "NULL argument");
    return ocn_max_abs_divergence(m->grid, m->U[0], m->U[1], m->U[2], value);
}
