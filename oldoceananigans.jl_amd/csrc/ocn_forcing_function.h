// ocn_forcing_function.h -- forcings that are functions, evaluated in the volume: F = program(x, y, z, t, deps...) at the forced field's
// (i, j, k), the dependencies interpolated to its location (Forcings/continuous_forcing.jl:119-142; Relaxation with a function mask or
// target, relaxation.jl:80-101). The program is the recorded list of ocn_boundary_function.h (ocn_expr_ins_t, SSA).
//
// This pass runs at every cell of every forced field at every stage, so the program is not interpreted whole per cell. The host gives
// every value the set of inputs it depends on (ff_make_plan, ocn_api.hip): a value that depends on no coordinate and no field is UNIFORM,
// one that depends on one coordinate is a LINE value, everything else is a CELL value. Uniform and line values that a cell instruction
// consumes (roots) are evaluated once per evaluation moment into 1-D tables by forcing_line_kernel; forcing_function_kernel interprets
// only the cell instructions, whose root operands have become table loads (FF_OP_TABLE, an op the public enum does not have). Nothing
// is simplified or reassociated: every instruction is the same IEEE operation on the same operand bits wherever it runs, so the hoisted
// evaluation equals the unhoisted one (option forcing_function_hoist = 0: the recorded program per cell) bit for bit.
//
// forcing_function_kernel completes the tendency of every field that has at least one function term: ALL its terms in the sum order of
// multiple_forcings.jl (arrays and table relaxations through forcing_one), G = G + F over ForcingTable::r. Fields without a function
// term stay with add_forcing_kernel. 64 lanes along x, 2 rows, blockIdx.z = level x field. The values of a thread are indexed at run
// time, so they live in LDS, slot-major, sized by the longest per-cell program of the launch: n x 128 x 8 B (at most 64 KB; a short
// program leaves the CU to several blocks). A thread only ever touches its own column: no barrier.
#pragma once
#include "ocn_boundary_function.h"
#include "ocn_forcing.h"

#define OCN_FORCING_KIND_FUNCTION 3
#define FF_MAX_FUNCTIONS 16      // function terms of one model
#define FF_OP_TABLE 24           // per-cell leaf: a = offset of the root's table in FfFunction::tab, b = its direction (3: uniform)
#define FF_UNIFORM 0             // value classes: FF_LINE + d is the line class of direction d
#define FF_LINE 1
#define FF_CELL 4
#define FF_LANES 64
#define FF_ROWS 2
#define FF_THREADS (FF_LANES * FF_ROWS)

// a dependency read at the forced field's (i, j, k): the corner of its interpolation stencil at (1, 1, 1), its parent strides and the
// interpolated directions, lowest first
struct FfDep {
    int field;                // slot of BfFields::p
    int n;                    // interpolated directions (0..3)
    long off, s1, s2;
    long st[3];
};

struct FfFunction {
    int field, term;          // the model field and the term of its sum this function is (the model's table)
    int n, n_cell, ndeps;     // instructions recorded, instructions per cell
    int reads_time;
    int L[3];                 // points of a line table along x / y / z: the index range of the field's location
    const double *x[3];       // node coordinates at the field's location (device tables of the grid), element index - 1
    double *tab;              // the root tables, one block (owned by whoever made the function)
    FfDep dep[BF_MAX_DEPS];
    ocn_expr_ins_t ins[BF_MAX_INS];      // the recorded program
    ocn_expr_ins_t cell[BF_MAX_INS];     // the per-cell program
    int root[BF_MAX_INS];     // per recorded value: the offset of its table in tab, -1 when it is no root
    signed char cls[BF_MAX_INS];
};

struct FfTable {
    int n;
    signed char fn_of[OCN_MAX_FIELDS][OCN_MAX_FORCING_TERMS];       // the function of (field, term), -1: none
    FfFunction fn[FF_MAX_FUNCTIONS];
};

// one recorded operation on its operand values (every op but the leaves); *c is read by OCN_EXPR_SELECT only. The two kernels here share
// it. boundary_function_kernel keeps its own switch: with this function in its place the compiler schedules that kernel differently
// (26 more instructions), and its recorded resources are a yardstick. ARITH: the caller's programs hold none of exp, log,
// sin, cos, tanh, pow -- without their inlined bodies forcing_function_kernel allocates 40 VGPRs instead of 121.
template <bool ARITH>
__device__ __forceinline__ double expr_apply(int op, double x, double y, const double *c) {
    if constexpr (!ARITH) {
        switch (op) {
        case OCN_EXPR_EXP: return exp(x);
        case OCN_EXPR_LOG: return log(x);
        case OCN_EXPR_SIN: return sin(x);
        case OCN_EXPR_COS: return cos(x);
        case OCN_EXPR_TANH: return tanh(x);
        case OCN_EXPR_POW: return pow(x, y);
        default: break;
        }
    }
    switch (op) {
    case OCN_EXPR_ADD: return x + y;
    case OCN_EXPR_SUB: return x - y;
    case OCN_EXPR_MUL: return x * y;
    case OCN_EXPR_DIV: return x / y;
    case OCN_EXPR_NEG: return -x;
    case OCN_EXPR_ABS: return fabs(x);
    case OCN_EXPR_MIN: return jl_min(x, y);
    case OCN_EXPR_MAX: return jl_max(x, y);
    case OCN_EXPR_SQRT: return sqrt(x);
    case OCN_EXPR_LT: return x < y ? 1.0 : 0.0;
    case OCN_EXPR_LE: return x <= y ? 1.0 : 0.0;
    case OCN_EXPR_GT: return x > y ? 1.0 : 0.0;
    case OCN_EXPR_GE: return x >= y ? 1.0 : 0.0;
    default: return x != 0.0 ? y : *c;          // OCN_EXPR_SELECT
    }
}

// ℑ of a dependency: 0.5 (f[low] + f[low + 1]) per direction, nested with st[0] (the lowest direction) innermost, as bf_dependency
__device__ __forceinline__ double ff_interp1(const double *q, long s0) { return 0.5 * (q[0] + q[s0]); }
__device__ __forceinline__ double ff_interp2(const double *q, long s0, long s1) { return 0.5 * (ff_interp1(q, s0) + ff_interp1(q + s1, s0)); }
__device__ __forceinline__ double ff_dependency(const FfDep &d, const double *p, int i, int j, int k) {
    const double *q = p + (d.off + (i - 1) + d.s1 * (j - 1) + d.s2 * (k - 1));
    if (d.n == 0) return q[0];
    if (d.n == 1) return ff_interp1(q, d.st[0]);
    if (d.n == 2) return ff_interp2(q, d.st[0], d.st[1]);
    return 0.5 * (ff_interp2(q, d.st[0], d.st[1]) + ff_interp2(q + d.st[2], d.st[0], d.st[1]));
}

// the line and uniform values of every function into their tables: blockIdx.z = function, blockIdx.y = direction (3: the uniform values,
// one thread), one thread per index of the line. A thread evaluates the recorded instructions of its own class and of the uniform class;
// their operands are of those classes too. time_only: functions that do not read t keep the tables they were given when they were set.
__global__ void __launch_bounds__(FF_THREADS) forcing_line_kernel(const FfTable *table, double time, int time_only) {
    __shared__ double vals[BF_MAX_INS][FF_THREADS];
    const FfFunction &fn = table->fn[blockIdx.z];
    if (time_only && !fn.reads_time) return;
    const int d = blockIdx.y, mine = d == 3 ? FF_UNIFORM : FF_LINE + d;
    const int idx = blockIdx.x * FF_THREADS + threadIdx.x;
    if (idx >= (d == 3 ? 1 : fn.L[d])) return;
    const int t = threadIdx.x, n = fn.n;
    for (int q = 0; q < n; ++q) {
        const int c = fn.cls[q];
        if (c != FF_UNIFORM && c != mine) continue;
        const ocn_expr_ins_t ins = fn.ins[q];
        double r;
        switch (ins.op) {
        case OCN_EXPR_CONST: r = ins.imm; break;
        case OCN_EXPR_COORD: r = fn.x[d == 3 ? 0 : d][idx]; break;          // a line value of direction d reads coordinate d only
        case OCN_EXPR_TIME: r = time; break;
        default: r = expr_apply<false>(ins.op, vals[ins.a][t], vals[ins.b][t], &vals[ins.c][t]); break;
        }
        vals[q][t] = r;
        if (c == mine && fn.root[q] >= 0) fn.tab[fn.root[q] + idx] = r;
    }
}

// one function at (i, j, k): `prog` is the per-cell program or the recorded one; vals is the thread's column of the LDS slots
template <bool ARITH>
__device__ __forceinline__ double ff_evaluate(const FfFunction &fn, const ocn_expr_ins_t *prog, int n, double *vals, const BfFields &fields, int i,
                                              int j, int k, double time) {
    double r = 0.0;
    for (int q = 0; q < n; ++q) {
        const ocn_expr_ins_t ins = prog[q];
        switch (ins.op) {
        case OCN_EXPR_CONST: r = ins.imm; break;
        case OCN_EXPR_COORD: r = fn.x[ins.a][(ins.a == 0 ? i : (ins.a == 1 ? j : k)) - 1]; break;
        case OCN_EXPR_TIME: r = time; break;
        case OCN_EXPR_FIELD: r = ff_dependency(fn.dep[ins.a], fields.p[fn.dep[ins.a].field], i, j, k); break;
        case FF_OP_TABLE: r = fn.tab[ins.a + (ins.b == 0 ? i - 1 : (ins.b == 1 ? j - 1 : (ins.b == 2 ? k - 1 : 0)))]; break;
        // operands: validated on the host to name earlier values (unused ones are 0)
        default: r = expr_apply<ARITH>(ins.op, vals[ins.a * FF_THREADS], vals[ins.b * FF_THREADS], &vals[ins.c * FF_THREADS]); break;
        }
        vals[q * FF_THREADS] = r;
    }
    return r;
}

template <bool ARITH>
__device__ __forceinline__ double ff_term(const ForcingTable *__restrict__ tab, const FfTable *__restrict__ ft, int f, int w, const DGrid &g,
                                          double *vals, const BfFields &fields, int i, int j, int k, double phi, double time, int hoist) {
    const ForcingTerm &T = tab->t[f][w];
    if (T.kind != OCN_FORCING_KIND_FUNCTION) return forcing_one(tab, T, g, i, j, k, phi);
    const FfFunction &fn = ft->fn[ft->fn_of[f][w]];
    return ff_evaluate<ARITH>(fn, hoist ? fn.cell : fn.ins, hoist ? fn.n_cell : fn.n, vals, fields, i, j, k, time);
}

// G[f] = G[f] + F (assign: G[f] = F, the raw evaluation) for every field of the launch, all terms in the reference's association order
// (forcing_sum). Dynamic LDS: (longest program of the launch) x FF_THREADS doubles. ARITH: no program of the launch holds exp .. pow
// (the host knows; with hoisting that is the usual case, the transcendentals of a mask sit in its line values): 8 waves per SIMD
// instead of 4.
template <bool ARITH>
__global__ void __launch_bounds__(FF_THREADS) forcing_function_kernel(DGrid g, const ForcingTable *__restrict__ tab, const FfTable *__restrict__ ft,
                                                                      ForcingLaunch L, BfFields fields, int nk, double time, int hoist, int assign) {
    extern __shared__ double ff_vals[];
    const int q = blockIdx.z / nk, kk = blockIdx.z - q * nk;
    const int f = L.f[q];
    const Range6 r = tab->r[f];
    const int i = r.i0 + blockIdx.x * FF_LANES + threadIdx.x, j = r.j0 + blockIdx.y * FF_ROWS + threadIdx.y, k = r.k0 + kk;
    if (i > r.i1 || j > r.j1 || k > r.k1) return;
    const long o = tab->off[f] + i + (long)tab->s1[f] * j + tab->s2[f] * k;
    const double phi = assign ? 0.0 : L.U[q][o];
    double *vals = ff_vals + (threadIdx.y * FF_LANES + threadIdx.x);
    const int n = tab->nterms[f];
    double s = 0.0;              // N <= 4: F₁ + F₂ + ...; N > 4: ((0.0 + F₁) + F₂) + ... (ocn_forcing.h)
#pragma unroll 1
    for (int w = 0; w < n; ++w) {
        const double F = ff_term<ARITH>(tab, ft, f, w, g, vals, fields, i, j, k, phi, time, hoist);
        s = (w == 0 && n <= 4) ? F : s + F;
    }
    L.G[q][o] = assign ? s : L.G[q][o] + s;
}
